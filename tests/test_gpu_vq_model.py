"""compression.py on the synthetic scene (about 2 000 rows, K = 64, 3 Lloyd iterations): the same seed gives the same bits,
`apply` writes codebook entries into the existing parameter storage, every row's index is the nearest centroid within the
fp32 bound of tests/test_gpu_vq_rows.py, and the file round trip reproduces the bits."""
import pytest
import torch

import compression
import synthetic_scene as S

pytestmark = pytest.mark.gpu

N, K, ITERS = 2003, 64, 3


@pytest.fixture(scope="module")
def scene(device):
    pc = S.SyntheticGaussianModel(N, 160, 96, seed=0, device=device)
    return pc, compression.compress(pc, groups={"f_rest": K}, iters=ITERS, seed=3)


def test_same_seed_same_bits_and_nearest_centroids(device, scene):
    pc, cm = scene
    cb, idx, shape = cm.groups["f_rest"]
    again = compression.compress(pc, groups={"f_rest": K}, iters=ITERS, seed=3).groups["f_rest"]
    assert torch.equal(cb, again[0]) and torch.equal(idx, again[1])
    assert cb.shape == (K, 45) and idx.dtype == torch.int32 and shape == (N, 15, 3)
    x, c = pc._features_rest.detach().reshape(N, 45).double().cpu(), cb.double().cpu()
    d = ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    bound = 4.0 * 47 * 2.0 ** -24 * (x.norm(dim=1) + c.norm(dim=1).max()) ** 2
    assert bool((d.gather(1, idx.cpu().long()[:, None])[:, 0] - d.min(dim=1).values <= bound).all())
    before, after = cm.nbytes()
    assert before == N * 59 * 4 and after == N * 14 * 4 + K * 45 * 4 + N * 2 and after < before


def test_apply_and_file_round_trip(device, scene, tmp_path):
    pc, cm = scene
    cb, idx, _ = cm.groups["f_rest"]
    target = S.SyntheticGaussianModel(N, 160, 96, seed=0, device=device)
    ptr, xyz = target._features_rest.data_ptr(), target._xyz.detach().clone()
    cm.apply(target)
    assert target._features_rest.data_ptr() == ptr and torch.equal(target._xyz.detach(), xyz)
    assert torch.equal(target._features_rest.detach().reshape(N, 45), cb[idx.long()])
    cm.save(tmp_path / "model.npz")
    other = S.SyntheticGaussianModel(N, 160, 96, seed=1, device=device)
    compression.CompressedModel.load(tmp_path / "model.npz", device=device).apply(other)
    for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        assert torch.equal(getattr(other, name).detach(), getattr(target, name).detach()), name


def test_degree_zero_is_skipped_and_wide_rows_are_refused(device):
    pc = S.SyntheticGaussianModel(50, 160, 96, seed=0, device=device)
    pc._features_rest = torch.nn.Parameter(torch.zeros(50, 0, 3, device=device))
    cm = compression.compress(pc, groups={"f_rest": K}, iters=1)
    assert not cm.groups and cm.raw["f_rest"].shape == (50, 0, 3)
    pc._features_rest = torch.nn.Parameter(torch.zeros(50, 22, 3, device=device))
    with pytest.raises(ValueError, match="at most 64"):
        compression.compress(pc, groups={"f_rest": K}, iters=1)
    few = compression.compress(S.SyntheticGaussianModel(50, 160, 96, seed=0, device=device), groups={"f_rest": K}, iters=1)
    assert few.groups["f_rest"][0].shape == (50, 45)  # K capped at the number of rows
