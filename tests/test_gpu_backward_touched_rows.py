"""-m gpu: the composite backward rounds only the rows K10 touched (include/gsraster.h: `touched` of gsr_render_backward).

K10 adds into [P,9] fp64 sums and flags the rows it adds into; the rounding pass then visits the flagged rows only and
every other row of the fp32 record keeps the 0.0f the forward's composite kernel left there.  The full pass
(touched = NULL or record_is_zero = 0: every row read and rounded) is the reference: the fp64 sums make both deterministic, so the
two records are compared BIT FOR BIT, through the operator, on shapes that reach the edge paths of both kernels --
images that are no multiple of the 16-pixel tile or the 8-pixel quadrant (clamped loads of the MFMA operand at the right
and bottom edges), a single tile, P = 1 / 7 / 1000 (odd P: the forward's clear ends in a tail of < 16 bytes), nothing
visible at all."""
import pytest
import torch

import diff_gaussian_rasterization as dgr
import synthetic_scene as S
from helpers import KEYS, cam_kwargs, elem_excess, rel_err, settings_from

pytestmark = pytest.mark.gpu

RTOL = 1e-4  # the parity tests' bar (tests/test_gpu_parity.py)


def _front(P, spread=0.25, z=4.0, seed=0):
    """P Gaussians in front of the identity camera, all inside a small image"""
    gen = torch.Generator().manual_seed(seed)
    xy = (torch.rand(P, 2, generator=gen) - 0.5) * 2 * spread * z
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=gen), dim=1)
    return dict(means3D=torch.cat([xy, torch.full((P, 1), z) + torch.rand(P, 1, generator=gen)], 1),
                scales=torch.full((P, 3), 0.08) * (0.5 + torch.rand(P, 3, generator=gen)), rotations=q,
                shs=torch.rand(P, 16, 3, generator=gen) * 0.4, opacities=0.2 + 0.7 * torch.rand(P, 1, generator=gen))


def layered_scene():
    """650 nearly opaque Gaussians in five dense sheets at z = 2.0 .. 2.2 that cover a 64 x 48 image, 350 small ones at
    z = 8 behind them: every pixel's transmittance falls below 1e-4 inside the sheets, the far layer is in the tile
    lists but no pixel ever blends it"""
    gen = torch.Generator().manual_seed(11)
    xs, ys = torch.linspace(-1.25, 1.25, 13), torch.linspace(-0.95, 0.95, 10)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    near = torch.cat([torch.stack([gx.reshape(-1), gy.reshape(-1), torch.full((130,), 2.0 + 0.05 * k)], 1)
                      for k in range(5)])
    far = torch.cat([(torch.rand(350, 2, generator=gen) - 0.5) * torch.tensor([8.0, 6.0]), torch.full((350, 1), 8.0)], 1)
    P = 1000
    return dict(means3D=torch.cat([near, far]),
                scales=torch.cat([torch.full((650, 3), 0.35), torch.full((350, 3), 0.05)]),
                rotations=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1),
                shs=torch.rand(P, 16, 3, generator=gen) * 0.4, opacities=torch.full((P, 1), 0.99)), 650


def _culled(P):
    g = _front(P)
    g["means3D"][:, 2] = -3.0  # behind the camera: radii 0, empty lists
    return g


SCENES = {
    "64x48": lambda: (S.make_gaussians(1000, 64, 48, seed=3, scale_coef=0.02), 64, 48),
    "37x21": lambda: (S.make_gaussians(1000, 37, 21, seed=4, scale_coef=0.03), 37, 21),
    "16x16": lambda: (S.make_gaussians(1000, 16, 16, seed=5, scale_coef=0.03), 16, 16),
    "P1": lambda: (_front(1), 64, 48),
    "P7": lambda: (_front(7), 64, 48),
    "P1000": lambda: (_front(1000, seed=2), 64, 48),
    "culled": lambda: (_culled(7), 64, 48),
    "layered": lambda: (layered_scene()[0], 64, 48),
}


def _weights(W, H):
    return torch.rand(3, H, W, generator=torch.Generator().manual_seed(2))


def _backward(device, g, W, H, touched_rows, twice=False):
    """render + backward through the operator -> (image, {name: gradient}, the backward's [(record, sums, flags)])"""
    cam = S.SyntheticCamera(0, W, H)
    rast = dgr.GaussianRasterizer(settings_from(cam, torch.tensor([0.1, 0.4, 0.9])))
    mask = torch.ones((H + 15) // 16, (W + 15) // 16, dtype=torch.bool, device=device)
    gg = {k: v.to(device).requires_grad_(True) for k, v in g.items()}
    kept = []
    old = dgr._TOUCHED_ROWS[0], dgr._KEEP_BACKWARD_BUFFERS[0]
    dgr._TOUCHED_ROWS[0], dgr._KEEP_BACKWARD_BUFFERS[0] = touched_rows, kept
    try:
        m2, rgb, co, radii, depths = rast.preprocess_gaussians(*[gg[k] for k in KEYS], {})
        img, _, _, _ = rast.render_gaussians(m2, co, rgb, depths, radii, mask, None, {})
        loss = (img * _weights(W, H).to(device)).sum()
        loss.backward(retain_graph=twice)
        grads = [{k: gg[k].grad.clone() for k in KEYS}]
        if twice:
            for k in KEYS:
                gg[k].grad = None
            loss.backward()
            grads.append({k: gg[k].grad.clone() for k in KEYS})
        torch.cuda.synchronize()
    finally:
        dgr._TOUCHED_ROWS[0], dgr._KEEP_BACKWARD_BUFFERS[0] = old
    return img.detach(), grads, kept


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def runs(device):
    """every scene once with the flagged pass and once with the full pass (shared by the tests below, never modified)"""
    out = {}
    for name, make in SCENES.items():
        g, W, H = make()
        out[name] = (g, W, H, _backward(device, g, W, H, True), _backward(device, g, W, H, False))
    return out


@pytest.mark.parametrize("name", ["64x48", "37x21", "16x16", "P1", "P7", "P1000", "culled"])
def test_flagged_pass_equals_full_pass_bitwise(runs, name):
    g, W, H, (img_t, grads_t, kept_t), (img_f, grads_f, kept_f) = runs[name]
    P = g["means3D"].shape[0]
    (rec_t, acc_t, flags), (rec_f, acc_f, none) = kept_t[0], kept_f[0]
    assert flags is not None and flags.shape == (P,) and none is None, "the two runs did not take the two passes"
    assert rec_t.shape == rec_f.shape == (P, 9) and rec_t.dtype == torch.float32
    assert torch.equal(img_t, img_f)
    assert torch.equal(_bits(rec_t), _bits(rec_f)), "record of the flagged pass differs from the full pass"
    assert bool(((flags == 0) | (flags == 1)).all())
    for k in KEYS:
        assert torch.equal(_bits(grads_t[0][k]), _bits(grads_f[0][k])), k
    if name == "culled":
        assert int(flags.sum()) == 0 and not bool(_bits(rec_t).any()), "nothing visible: no flag, record all +0.0f"
    else:
        assert int(flags.sum()) > 0


def test_rows_behind_an_opaque_layer_are_skipped_and_zero(runs):
    g, W, H, (_, _, kept_t), (_, _, kept_f) = runs["layered"]
    P, n_near = g["means3D"].shape[0], layered_scene()[1]
    rec, acc, flags = kept_t[0]
    n = int(flags.sum())
    print(f"[layered] {n} of {P} rows flagged ({int(flags[:n_near].sum())} near, {int(flags[n_near:].sum())} far)")
    assert 0 < n < P
    assert int(flags[n_near:].sum()) == 0, "a pixel blended a Gaussian behind the opaque sheets"
    on = flags.bool()
    assert not bool(_bits(rec[~on]).any()), "an unflagged row is not bitwise 0.0f"
    assert torch.equal(_bits(rec[on]), _bits(acc[on].float())), "a flagged row is not its fp64 sum rounded once"
    assert not bool((acc[~on] != 0).any())
    assert torch.equal(_bits(rec), _bits(kept_f[0][0]))


def test_second_backward_over_one_forward_equals_the_first(device):
    g, W, H = SCENES["64x48"]()
    _, grads, kept = _backward(device, g, W, H, True, twice=True)
    assert len(kept) == 2 and kept[0][2] is not None and kept[1][2] is None  # flagged pass, then the full pass
    assert torch.equal(_bits(kept[0][0]), _bits(kept[1][0]))
    for k in KEYS:
        assert torch.equal(_bits(grads[0][k]), _bits(grads[1][k])), k


@pytest.mark.parametrize("name", ["37x21", "64x48"])
def test_edge_tiles_match_the_fp64_autograd_oracle(runs, name):
    """the right / bottom tiles of these images are partial (37 x 21: a quadrant with pixels on both sides of the image
    edge in x AND y), where K10's MFMA operand is loaded from clamped addresses and selected by the bounds"""
    from oracle import torch_oracle as O

    g, W, H, (img, grads, _), _ = runs[name]
    cam = S.SyntheticCamera(0, W, H)
    mask = torch.ones((H + 15) // 16, (W + 15) // 16, dtype=torch.bool)
    ins = {k: v.double().clone().requires_grad_(True) for k, v in g.items()}
    m2o, rgbo, coo, radiio, deptho = O.preprocess(*[ins[k] for k in KEYS], **cam_kwargs(cam, 3))
    imgo, _, _ = O.render(m2o, coo, rgbo, deptho, radiio, mask, bg=torch.tensor([0.1, 0.4, 0.9]), W=W, H=H)
    (imgo * _weights(W, H).double()).sum().backward()
    assert rel_err(img, imgo) < RTOL
    for k in KEYS:
        e, x = rel_err(grads[0][k], ins[k].grad), elem_excess(grads[0][k], ins[k].grad)
        print(f"[{name}] {k}: rel {e:.2e}, p99 element-wise excess {x:.2f}")
        assert e < RTOL, k
        assert x <= 1.0, f"{k}: p99 element-wise"
