"""Depth-normal consistency (csrc/normals.hip): the surfel-row kernels and the fused image-space loss against the float64
restatements of tests/normal_refs.py through helpers.assert_rows_close (K = 8 times the float32 reference's own worst
relative error, exact zeros exact).  The kernels are called through the C ABI on outputs pre-filled with NaN -- an
element that is not written fails --, and the autograd wrappers must return the same bits.  Rows of the checks: one
Gaussian, one pixel.  The gradient planes: per pixel wherever the float32 reference is itself within ROW_UNIT_CAP / 4 of
the pixel's largest component; the few other pixels (a gather of four terms that cancels, or a border pixel beside a
hole, whose gradient through z is analytically zero) have no per-pixel float32 yardstick and are held to their plane's
norm, with every other element.  Then the mode through the Python layers at bsz 2 against float64 autograd through
oracle.torch_oracle, under FusedAdam(fuse_backward=True) as well, and the three refusals."""
import pytest
import torch

import normal_refs as NR
import synthetic_scene as S
from helpers import ROW_UNIT_CAP, assert_rows_close, cam_kwargs, rel_err

gpu = pytest.mark.gpu
TX, TY = 64, 8  # the loss kernels' tile (diff_gaussian_rasterization.NORMALS_TILE, asserted below)
TANX, TANY, WEIGHT, G_LOSS = 0.6, 0.45, 0.7, 0.75
NAN = float("nan")


def _ptr(t):
    return t.data_ptr()


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _views():
    return [torch.eye(4), S.orbit_cameras(4, 64, 48)[1].world_view_transform.float().cpu()]


@gpu
@pytest.mark.parametrize("view", [0, 1], ids=["identity", "orbit"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_surfel_rows_and_their_gradients(device, P, view):
    import diff_gaussian_rasterization as dgr

    lib = dgr._lib.lib
    V = _views()[view]
    xyz, scaling, rot, radii = NR.surfel_inputs(P, V, seed=100 * view + P)
    g = torch.randn(P, 5, generator=torch.Generator().manual_seed(P))
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = [t.to(dt, copy=True).requires_grad_(True) for t in (xyz, scaling, rot)]
        rows = NR.rows_ref(*leaves, radii, V)
        d_xyz, d_rot = torch.autograd.grad(rows, [leaves[0], leaves[2]], g.to(dt))
        ref[dt] = dict(rows=rows.detach(), d_xyz=d_xyz, d_rot=d_rot)
    r64 = ref[torch.float64]
    if P >= 63:  # the construction: every position of the minimum, culled rows, and every live normal faces the camera
        assert set(scaling.argmin(1).tolist()) == {0, 1, 2} and bool((radii == 0).any())
        facing = (r64["rows"][:, 2:] * (xyz.double() @ V.double()[:3, :3] + V.double()[3, :3])).sum(1)
        assert bool((facing[radii > 0] < 0).all()) and bool((facing[radii == 0] == 0).all())
    x, s, q, r, Vd, gd = [t.to(device).contiguous() for t in (xyz, scaling, rot, radii, V, g)]
    got = dict(rows=torch.full((P, 5), NAN, device=device), d_xyz=torch.full((P, 3), NAN, device=device),
               d_rot=torch.full((P, 4), NAN, device=device))
    assert lib.gsr_normal_rows_forward(P, _ptr(x), _ptr(s), _ptr(q), _ptr(r), _ptr(Vd), _ptr(got["rows"]),
                                       dgr._stream()) == 0
    assert lib.gsr_normal_rows_backward(P, _ptr(x), _ptr(s), _ptr(q), _ptr(r), _ptr(Vd), _ptr(gd), _ptr(got["d_xyz"]),
                                        _ptr(got["d_rot"]), dgr._stream()) == 0
    leaves = [t.clone().requires_grad_(True) for t in (x, s, q)]
    rows = dgr.normal_rows(*leaves, r, Vd)
    rows.backward(gd)
    torch.cuda.synchronize()
    assert _bits_equal(rows, got["rows"]) and _bits_equal(leaves[0].grad, got["d_xyz"]) and \
        _bits_equal(leaves[2].grad, got["d_rot"]) and leaves[1].grad is None, "the wrapper and the C ABI differ"
    for k in got:
        unit, worst = assert_rows_close(got[k], r64[k], ref[torch.float32][k], 8, f"P={P} view={view} {k}")
        print(f"NORMALS rows P={P} view={view} {k}: unit {unit:.3g}, worst {worst:.3g} of 8")


def _pixels(t):
    return t.reshape(t.shape[0], -1).T


@gpu
@pytest.mark.parametrize("holes", [False, True], ids=["smooth", "holes"])
@pytest.mark.parametrize("W,H", [(1, 1), (3, 3), (5, 4), (TX + 1, 4), (4, TY + 1), (2 * TX + 3, 2 * TY + 1)])
def test_consistency_loss_normals_and_gradients(device, W, H, holes):
    import diff_gaussian_rasterization as dgr

    lib = dgr._lib.lib
    assert dgr.NORMALS_TILE == (TX, TY)
    F = NR.surfel_map(W, H, holes, seed=7 * W + H, tile=(TX, TY))
    ref = {}
    for dt in (torch.float64, torch.float32):
        Fd = F.to(dt, copy=True).requires_grad_(True)
        loss, n_d = NR.consistency_ref(Fd, TANX, TANY, WEIGHT)
        (dF,) = torch.autograd.grad(loss, Fd, torch.tensor(G_LOSS, dtype=dt))
        ref[dt] = dict(loss=loss.detach().reshape(1, 1), n_d=n_d, dF=dF)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    Fd, gl = F.to(device), torch.tensor(G_LOSS, device=device)
    partials = torch.full((lib.gsr_normal_consistency_num_partials(W, H),), NAN, dtype=torch.float64, device=device)
    loss, n_d = torch.full((), NAN, device=device), torch.full((3, H, W), NAN, device=device)
    assert lib.gsr_normal_consistency_forward(W, H, _ptr(Fd), TANX, TANY, WEIGHT, _ptr(partials), _ptr(loss), _ptr(n_d),
                                              dgr._stream()) == 0
    runs = [torch.full((5, H, W), NAN, device=device) for _ in range(2)]
    for dF in runs:
        assert lib.gsr_normal_consistency_backward(W, H, _ptr(Fd), TANX, TANY, WEIGHT, _ptr(gl), _ptr(dF),
                                                   dgr._stream()) == 0
    Fg = Fd.clone().requires_grad_(True)
    loss_w, n_w = dgr.normal_consistency(Fg, TANX, TANY, WEIGHT, return_normals=True)
    loss_w.backward(gl)
    torch.cuda.synchronize()
    assert _bits_equal(runs[0], runs[1]), "two runs on the same input differ in bits"
    assert _bits_equal(loss_w, loss) and _bits_equal(n_w, n_d) and _bits_equal(Fg.grad, runs[0]), \
        "the wrapper and the C ABI differ"
    # the pixels with a float32 yardstick of their own (module docstring), from the references alone
    p64, p32 = _pixels(r64["dF"]), _pixels(r32["dF"]).double()
    fine = (p32 - p64).abs().amax(1) <= ROW_UNIT_CAP / 4 * p64.abs().amax(1)
    assert int((~fine).sum()) <= max(2, W * H // 100), "too many ill-conditioned pixels: change the inputs of this case"
    checks = [("loss", loss.reshape(1, 1), r64["loss"], r32["loss"]),
              ("n_d per pixel", _pixels(n_d), _pixels(r64["n_d"]), _pixels(r32["n_d"])),
              ("dF per pixel", _pixels(runs[0])[fine.to(device)], p64[fine], p32[fine]),
              ("dF per plane", runs[0], r64["dF"], r32["dF"])]
    for k, got, want64, want32 in checks:
        unit, worst = assert_rows_close(got, want64, want32, 8, f"{W}x{H} {k}")
        print(f"NORMALS map {W}x{H} holes={holes} {k} ({int((~fine).sum())} coarse pixels): unit {unit:.3g}, "
              f"worst {worst:.3g} of 8")


# ---------------------------------------------------------------------------------------------------- the pipeline
N, PW, PH, DEG, SCALE, SEED, VIEWS, PWEIGHT = 300, 64, 48, 1, 0.03, 11, (0, 1), 0.5
NAMES = ["_xyz", "_rotation", "_opacity", "_scaling"]


def _single_rank(bsz):
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils

    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=bsz, no_heuristics_update=True))
    utils.set_img_size(PH, PW)
    utils.set_cur_iter(1)
    wd._BALANCE["mode"] = "exact"
    gr._PLANNERS.clear()


def _render_batch(model, dev, on):
    import gaussian_renderer as gr
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    cams = S.orbit_cameras(4, PW, PH, device=dev)
    batch = [cams[v] for v in VIEWS]
    strategies, _ = start_strategy_final(batch, DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0))
    pipe = type("P", (), {"debug": False})()
    gr.set_normal_consistency(on)
    try:
        pkg = distributed_preprocess3dgs_and_all2all_final(batch, model, pipe, torch.zeros(3, device=dev),
                                                           batched_strategies=strategies, mode="train")
        images, _ = render_final(pkg, strategies)
    finally:
        gr.set_normal_consistency(False)
    return images, pkg, batch


def _oracle_term():
    """float64 on the host: the term of the two views and its gradients"""
    from oracle import torch_oracle as O

    m = S.SyntheticGaussianModel(N, PW, PH, seed=SEED, sh_degree=DEG, device="cpu", scale_coef=SCALE)
    raw = {n: getattr(m, n).detach().double().clone().requires_grad_(True) for n in NAMES}
    shs = torch.cat([m._features_dc, m._features_rest], dim=1).detach().double()
    mask = torch.ones((PH + 15) // 16 * ((PW + 15) // 16), dtype=torch.bool)
    total = 0
    for v in VIEWS:
        cam = S.orbit_cameras(4, PW, PH)[v]
        kw = cam_kwargs(cam, DEG)
        m2, rgb, co, radii, depths = O.preprocess(raw["_xyz"], torch.exp(raw["_scaling"]),
                                                  torch.nn.functional.normalize(raw["_rotation"]), shs,
                                                  torch.sigmoid(raw["_opacity"]), **kw)
        rows = NR.rows_ref(raw["_xyz"], raw["_scaling"], raw["_rotation"], radii, cam.world_view_transform.double())
        binning = O.bin_and_sort(m2, radii, depths, mask, PW, PH)
        maps = []
        for cols in (rows[:, 0:3], torch.cat([rows[:, 3:5], torch.zeros(N, 1, dtype=torch.float64)], dim=1)):
            img, _, _ = O.render(m2, co, cols, depths, radii, mask, bg=torch.zeros(3, dtype=torch.float64), W=PW, H=PH,
                                 binning=binning)
            maps.append(img)
        fmap = torch.cat(maps)[:5]
        total = total + NR.consistency_ref(fmap, kw["tanfovx"], kw["tanfovy"], PWEIGHT)[0]
    return float(total), dict(zip(NAMES, torch.autograd.grad(total, [raw[n] for n in NAMES])))


@gpu
def test_mode_at_bsz_two_against_float64_autograd(device):
    from gaussian_renderer.loss_distribution import normal_consistency_loss

    want, grads = _oracle_term()
    _single_rank(2)
    model = S.SyntheticGaussianModel(N, PW, PH, seed=SEED, sh_degree=DEG, device=device, scale_coef=SCALE)
    images, pkg, batch = _render_batch(model, device, True)
    rows = pkg["_features_rows"]
    assert isinstance(rows, list) and len(rows) == 2 and not torch.equal(rows[0], rows[1])
    assert all(f.shape == (5, PH, PW) for f in pkg["batched_features"])
    loss = normal_consistency_loss(pkg, batch, PWEIGHT)
    loss.backward()
    torch.cuda.synchronize()
    e = abs(float(loss) - want) / abs(want)
    print(f"NORMALS pipe loss {float(loss):.9g} vs {want:.9g} ({e:.3g})")
    assert e < 1e-4
    for n in NAMES:
        e = rel_err(getattr(model, n).grad, grads[n])
        print(f"NORMALS pipe d{n}: rel err {e:.3g}")
        assert e < 1e-4 and bool(grads[n].any()), n
    # FusedAdam(fuse_backward=True): the rows' gradients arrive as `.grad`, so the projection backward is not fused
    # (declined at its node, or materialized by the step, whichever autograd runs first): the unfused gradients
    from fused_optim import FusedAdam

    _single_rank(2)
    fused = S.SyntheticGaussianModel(N, PW, PH, seed=SEED, sh_degree=DEG, device=device, scale_coef=SCALE)
    opt = FusedAdam(fused.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True)
    try:
        _, pkg2, _ = _render_batch(fused, device, True)
        normal_consistency_loss(pkg2, batch, PWEIGHT).backward()
        opt.step()
        torch.cuda.synchronize()
        print(f"NORMALS pipe fuse_backward: materialized {opt.materialized_steps}, fused {opt.fused_steps}")
        assert opt.fused_steps == 0
        for n in NAMES:
            assert rel_err(getattr(fused, n).grad, getattr(model, n).grad) < 1e-6, n
    finally:
        opt.set_fuse_backward(False)
    # with the mode off nothing new is left behind
    _single_rank(2)
    _, off, _ = _render_batch(model, device, False)
    assert "_features_rows" not in off and "batched_features" not in off
    assert not any("features" in k for ca in off["batched_cuda_args"] for k in ca)


# ---------------------------------------------------------------------------------------------------- the refusals
def test_the_three_refusals(monkeypatch):
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr
    import utils.general_utils as utils
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final as prep

    _single_rank(1)
    monkeypatch.setattr(gr, "_FEATURES", [True])
    with pytest.raises(ValueError, match="together with set_features"):
        gr.set_normal_consistency(True)
    monkeypatch.setattr(gr, "_NORMALS", [True])  # (GSR_NORMALS=1 beside GSR_FEATURES=1: the call itself refuses)
    with pytest.raises(ValueError, match="together with set_features"):
        prep([], None, None, None, batched_strategies=[])
    monkeypatch.setattr(gr, "_FEATURES", [False])

    class Two(utils.SingleGPUGroup):
        def size(self):
            return 2

    monkeypatch.setattr(utils, "DEFAULT_GROUP", Two())
    with pytest.raises(NotImplementedError, match="world size"):
        prep([], None, None, None, batched_strategies=[])
    monkeypatch.setattr(utils, "DEFAULT_GROUP", utils.SingleGPUGroup())
    monkeypatch.setattr(dgr, "_CAPTURE", [object()])  # what capturing() returns inside a graph capture
    with pytest.raises(RuntimeError, match="graph capture"):
        prep([], None, None, None, batched_strategies=[])
    monkeypatch.undo()
    assert not gr.get_normal_consistency() and dgr.capturing() is None
