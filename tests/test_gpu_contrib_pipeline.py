"""-m gpu: contribution statistics through GaussianRasterizer (cuda_args["contributions"]) and prune_by_contribution.

Scene on a 64 x 48 frame, identity camera: 50 small splats in front (a grid: each owns its centre pixel), eight
frame-filling walls of opacity 0.8 at increasing depth, 200 small splats behind them.  Behind k walls T is about 0.2^k
(the walls' standard deviation is 400 px: alpha >= 0.79 on every pixel), so on a pixel no front splat covers wall 5 (the
sixth) is where K8 stops: T = 3.2e-4 in front of it, 6.4e-5 behind -- a factor of 1.5 and more from the 1e-4 threshold
on both sides.  A front splat only lowers T, so the stop is never later: walls 5-7 and every splat behind are blended on
no pixel, although K1 gives each of them radii > 0 -- which is all `denom` / `min_opacity` know about them."""
import math

import pytest
import torch

import densification_ops as D
import diff_gaussian_rasterization as dgr
import synthetic_scene as S
from fused_optim import FusedAdam

pytestmark = pytest.mark.gpu

W, H = 64, 48
N_FRONT, N_WALL, N_BACK = 50, 8, 200
P = N_FRONT + N_WALL + N_BACK
WALLS_BLENDED = 5           # 0.2^5 = 3.2e-4 >= 1e-4 > 0.2^6
FX = 0.9 * W
U = 2.0 ** -24
CLAMP = float(torch.tensor(0.99, dtype=torch.float32))


def _scene():
    """activated attributes (means3D, scales, rotations, shs, opacities) on the host; rows: front, walls, back"""
    g = torch.Generator().manual_seed(11)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0

    def at(px, py, z):  # world position that projects to pixel (px, py) at depth z
        return torch.stack([(px - cx) * z / FX, (py - cy) * z / FX, z], dim=1)

    k = torch.arange(N_FRONT)
    zf = 1.9 + 0.2 * torch.rand(N_FRONT, generator=g)
    front = at(5.0 + 6.0 * (k % 10), 6.0 + 9.0 * (k // 10), zf)
    s_front = (1.2 * zf / FX)[:, None].expand(-1, 3)
    zw = 3.0 + 0.1 * torch.arange(N_WALL)
    walls = at(torch.full((N_WALL,), cx), torch.full((N_WALL,), cy), zw)
    s_wall = (400.0 * zw / FX)[:, None].expand(-1, 3)
    zb = 6.0 + 2.0 * torch.rand(N_BACK, generator=g)
    back = at(4.0 + 56.0 * torch.rand(N_BACK, generator=g), 4.0 + 40.0 * torch.rand(N_BACK, generator=g), zb)
    s_back = (2.0 * zb / FX)[:, None].expand(-1, 3)
    means3D = torch.cat([front, walls, back]).float()
    scales = torch.cat([s_front, s_wall, s_back]).float().contiguous()
    rot = torch.zeros(P, 4)
    rot[:, 0] = 1.0
    op = torch.cat([0.5 + 0.4 * torch.rand(N_FRONT, generator=g), torch.full((N_WALL,), 0.8),
                    0.3 + 0.6 * torch.rand(N_BACK, generator=g)])[:, None].float()
    shs = torch.zeros(P, 16, 3)
    shs[:, 0] = (torch.rand(P, 3, generator=g) - 0.5) / 0.28209479177387814
    return means3D, scales, rot, shs, op


def _rasterizer(device, bg=(0.0, 0.0, 0.0)):
    cam = S.SyntheticCamera(0, W, H, device=device)
    rs = dgr.GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2),
                                           torch.tensor(bg, device=device), 1.0, cam.world_view_transform,
                                           cam.full_proj_transform, 3, cam.camera_center, False, False)
    return dgr.GaussianRasterizer(rs)


def _render(rast, attrs, stats=None, white=False):
    """-> (image, radii, n_contrib) of the activated attributes, the statistics into `stats` when given"""
    with torch.no_grad():
        m2, rgb, co, radii, depths = rast.preprocess_gaussians(*attrs, {})
        if white:
            rgb = torch.ones_like(rgb)
        ca = {"stats_collector": {}}
        if stats is not None:
            ca["contributions"] = stats
        img, _, _, nc = rast.render_gaussians(m2, co, rgb, depths, radii, None, None, ca)
    torch.cuda.synchronize()
    return img, radii, nc, ca


@pytest.fixture(scope="module")
def view(device):
    attrs = tuple(t.to(device) for t in _scene())
    rast = _rasterizer(device)
    stats = dgr.ContributionStats(P, device)
    img, radii, nc, ca = _render(rast, attrs, stats, white=True)
    return dict(attrs=attrs, rast=rast, stats=stats, img=img, radii=radii, nc=nc, ca=ca)


def test_hidden_rows_are_visible_to_radii_and_blended_nowhere(view):
    hits, radii = view["stats"].hits.cpu(), view["radii"].cpu()
    hidden = torch.zeros(P, dtype=torch.bool)
    hidden[N_FRONT + WALLS_BLENDED:] = True
    print(f"CONTRIB-PIPE rows with radii > 0: {int((radii > 0).sum())} of {P}; with hits > 0: {int((hits > 0).sum())}; "
          f"largest n_contrib {int(view['nc'].max())}")
    assert bool((radii[hidden] > 0).all()), "a hidden row is culled by K1: the scene does not show what it is meant to"
    assert not bool(hits[hidden].any()), f"hidden rows with hits: {torch.nonzero(hits * hidden).reshape(-1)[:8].tolist()}"
    assert bool((hits[~hidden] > 0).all()), f"rows in front without a hit: {torch.nonzero((hits == 0) & ~hidden).reshape(-1).tolist()}"
    assert int(view["nc"].max()) < 64


def test_the_three_statistics_vanish_together_and_add_up_to_the_image(view):
    st = view["stats"]
    hits, wmax, wsum = st.hits.cpu(), st.wmax.cpu(), st.wsum.cpu()
    assert torch.equal(hits == 0, wmax == 0) and torch.equal(hits == 0, wsum == 0)
    assert float(wmax.max()) <= CLAMP and float(wmax.min()) >= 0.0
    assert bool((hits <= W * H).all())
    # rgb = 1, bg = 0: a pixel's value is the sum of its blend weights (K8: an fp32 sum of under 64 terms <= 1)
    total_img = float(view["img"][0].double().sum())
    total_w = float(wsum.sum())
    print(f"CONTRIB-PIPE sum wsum {total_w:.9g}, sum image {total_img:.9g}, difference {abs(total_w - total_img):.3g}, "
          f"bound {W * H * 64 * U:.3g}")
    assert abs(total_w - total_img) <= W * H * 64 * U
    for kind, ref in (("max", wmax), ("sum", wsum.float()), ("hits", hits.float())):
        assert torch.equal(st.importance(kind).cpu(), ref)
    with pytest.raises(ValueError):
        st.importance("median")


def test_the_pair_count_is_not_deferred_and_the_key_is_opt_in(view, device):
    """with the key the render op settles its pair count itself (nothing is queued for the caller to settle, so K8 is
    never redrawn under the statistics), and the image is bit for bit the one without the key"""
    late = []
    ca = {"stats_collector": {}, "_gsr_pending": late, "contributions": dgr.ContributionStats(P, device)}
    with torch.no_grad():
        m2, rgb, co, radii, depths = view["rast"].preprocess_gaussians(*view["attrs"], {})
        img, n_render, _, _ = view["rast"].render_gaussians(m2, co, torch.ones_like(rgb), depths, radii, None, None, ca)
    assert late == [] and n_render > 0
    plain, _, _, _ = _render(view["rast"], view["attrs"], None, white=True)
    assert torch.equal(img, plain) and torch.equal(view["img"], plain)
    assert torch.equal(ca["contributions"].hits, view["stats"].hits)
    assert torch.equal(ca["contributions"].wmax, view["stats"].wmax)


def test_the_key_raises_under_capture_and_on_host_tensors(view, device, monkeypatch):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.ContributionStats(P, "cpu")
    st = dgr.ContributionStats(P, device)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.merge_rows(torch.zeros(P, dtype=torch.int32), st)
    with torch.no_grad():
        m2, rgb, co, radii, depths = view["rast"].preprocess_gaussians(*view["attrs"], {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.contribution_stats(torch.zeros(13, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), m2, co,
                               torch.zeros(H, W, dtype=torch.int32), torch.ones(12, dtype=torch.uint8), W, H, st)
    with pytest.raises(ValueError):  # a record of another length
        view["rast"].render_gaussians(m2, co, rgb, depths, radii, None, None,
                                      {"contributions": dgr.ContributionStats(P + 1, device)})
    monkeypatch.setattr(dgr, "_CAPTURE", [object()])  # what capturing() returns inside a graph capture
    assert dgr.capturing() is not None
    with pytest.raises(RuntimeError, match="capture"):
        view["rast"].render_gaussians(m2, co, rgb, depths, radii, None, None, {"contributions": st})
    monkeypatch.undo()
    assert dgr.capturing() is None and not bool(st.hits.any())


def test_merge_rows_adds_hits_takes_the_max_and_skips_negative_rows(device):
    dst = dgr.ContributionStats(4, device)
    dst.hits += 7
    dst.wmax += 0.5
    dst.wsum += 3.25
    src = dgr.ContributionStats.of(torch.tensor([1, 2, 0, 4, 5], device=device),
                                   torch.tensor([0.25, 0.75, 0.0, 0.6, 0.1], device=device),
                                   torch.tensor([0.5, 1.5, 0.0, 2.0, 0.125], dtype=torch.float64, device=device))
    idx = torch.tensor([0, 1, 2, 1, -1], dtype=torch.int32, device=device)  # row 1 twice, a padding row, a row without hits
    dst.merge_rows(idx, src)
    assert dst.hits.tolist() == [8, 13, 7, 7]
    assert dst.wmax.tolist() == [0.5, 0.75, 0.5, 0.5]
    assert dst.wsum.tolist() == [3.75, 6.75, 3.25, 3.25]
    assert dst.zero_() is dst and not bool(dst.hits.any() | (dst.wmax != 0).any() | (dst.wsum != 0).any())


def test_prune_by_contribution_removes_exactly_the_hidden_rows(device):
    means3D, scales, rot, shs, op = (t.to(device) for t in _scene())
    m = S.SyntheticGaussianModel(P, W, H, seed=3, device=device)
    with torch.no_grad():
        m._xyz.copy_(means3D)
        m._scaling.copy_(torch.log(scales))
        m._rotation.copy_(rot)
        m._opacity.copy_(torch.log(op / (1 - op)))
        m._features_dc.copy_(shs[:, 0:1])
        m._features_rest.copy_(shs[:, 1:])
    m.optimizer = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15)
    for _ in range(2):  # populate exp_avg / exp_avg_sq (lr = 0: the parameters stay)
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.max_radii2D = torch.arange(P, device=device).float()
    rast = _rasterizer(device, bg=(0.1, 0.2, 0.3))

    def attrs():
        return m.get_xyz, m.get_scaling, m.get_rotation, m.get_features, m.get_opacity

    stats = dgr.ContributionStats(P, device)
    before, _, _, _ = _render(rast, attrs(), stats)
    hidden = torch.zeros(P, dtype=torch.bool, device=device)
    hidden[N_FRONT + WALLS_BLENDED:] = True
    assert torch.equal(stats.hits == 0, hidden)
    with pytest.raises(ValueError):
        D.prune_by_contribution(m, dgr.ContributionStats(P - 1, device))
    xyz_kept = m._xyz.detach()[~hidden].clone()
    assert D.prune_by_contribution(m, stats) == int(hidden.sum()) == N_WALL - WALLS_BLENDED + N_BACK
    assert torch.equal(m._xyz.detach(), xyz_kept) and m._opacity.shape[0] == P - int(hidden.sum())
    assert torch.equal(m.max_radii2D, torch.arange(P, device=device).float()[~hidden])
    assert m.optimizer.state[m._xyz]["exp_avg"].shape[0] == m._xyz.shape[0]
    after, _, _, _ = _render(rast, attrs())
    worst = float((after.double() - before.double()).abs().max())
    print(f"CONTRIB-PIPE image before / after the prune: worst pixel difference {worst:.3g}, bound {64 * U:.3g}")
    assert worst <= 64 * U
    # a threshold on the largest weight as well: the walls behind the first blend with T <= 0.2 alpha
    stats2 = dgr.ContributionStats(m._xyz.shape[0], device)
    _render(rast, attrs(), stats2)
    n_low = int((stats2.wmax < 0.1).sum())
    assert 0 < n_low < stats2.P
    assert D.prune_by_contribution(m, stats2, min_wmax=0.1) == n_low and m._xyz.shape[0] == stats2.P - n_low
    assert D.install(type("M", (), {})).prune_by_contribution is D.prune_by_contribution
