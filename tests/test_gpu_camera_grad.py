"""Camera pose gradients dL/d(viewmatrix, projmatrix, campos): the kernel (gsr_preprocess_backward_cams) against the
float64 autograd oracle, its hygiene and shard additivity, and the operator / renderer paths that hand the gradient to
autograd.  The bound is the project's norm-wise 1e-4 per camera and block; the float32 run of the same oracle must stay
within a quarter of it (asserted), so the bound is never eaten by fp32 itself."""
import ctypes
import functools
import math

import pytest
import torch

import synthetic_scene as S
from helpers import KEYS, rel_err, settings_from
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

W, H = 64, 48
BOUND = 1e-4        # norm-wise, every hand-written backward of this project
FP32_SHARE = 2.5e-5  # what the float32 oracle may differ from the float64 oracle on the test's scenes
CASES = [(1, 1, 3), (63, 3, 3), (257, 3, 0), (3001, 3, 3), (3001, 3, 1), (3001, 3, 2)]
BLOCKS = ("view", "proj", "campos")


def _tan(cam):
    return math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)


def _oracle_camera_grads(ins, cam, deg, loss_of, dt):
    """-> (dL/dview [4,4], dL/dproj [4,4], dL/dcampos [3], radii) of loss_of(means2D, rgb, conic_opacity, radii, depths)"""
    v = cam.world_view_transform.to(dt).clone().requires_grad_()
    p = cam.full_proj_transform.to(dt).clone().requires_grad_()
    c = cam.camera_center.to(dt).clone().requires_grad_()
    tx, ty = _tan(cam)
    m2, rgb, co, radii, depths = O.preprocess(*[t.to(dt) for t in ins], viewmatrix=v, projmatrix=p, campos=c, W=W, H=H,
                                              tanfovx=tx, tanfovy=ty, sh_degree=deg)
    loss_of(m2, rgb, co, radii, depths).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731  (campos at degree 0)
    return zero(v), zero(p), zero(c), radii


@functools.lru_cache(maxsize=None)
def _scene(N, B, deg):
    """scene, fixed incoming gradients and the float64 oracle gradients of one case (computed once, never modified)"""
    g = S.make_gaussians(N, W, H, seed=11 + N)
    cams = S.orbit_cameras(B, W, H)
    tx, _ = _tan(cams[0])
    n = min(8, N // 4)  # rows that exercise the Jacobian clamp: far outside the frustum in x, and large
    if n:
        sign = torch.tensor([1.0, -1.0]).repeat(4)[:n]
        g["means3D"][:n, 0] = sign * 1.5 * tx * g["means3D"][:n, 2]
        g["scales"][:n] *= 12.0
    gen = torch.Generator().manual_seed(1000 + N + deg)
    G2, Gco, Grgb = (torch.randn(B, N, k, generator=gen) for k in (2, 4, 3))
    ins = [g[k] for k in KEYS]
    ref, worst32 = [], 0.0
    for b, cam in enumerate(cams):
        def loss_of(m2, rgb, co, radii, depths, b=b):
            dt = m2.dtype
            return (m2 * G2[b].to(dt)).sum() + (co * Gco[b].to(dt)).sum() + (rgb * Grgb[b].to(dt)).sum()

        r64 = _oracle_camera_grads(ins, cam, deg, loss_of, torch.float64)
        r32 = _oracle_camera_grads(ins, cam, deg, loss_of, torch.float32)
        worst32 = max([worst32] + [rel_err(a, e) for a, e in zip(r32[:3], r64[:3]) if float(e.norm()) > 0])
        ref.append(r64)
    if n:  # camera 0 is the identity: t = p
        t = g["means3D"]
        hit = (ref[0][3] > 0) & ((t[:, 0] / t[:, 2]).abs() > 1.3 * tx)
        assert int(hit.sum()) >= 1, "no visible Gaussian of camera 0 exercises the Jacobian clamp"
    assert worst32 <= FP32_SHARE, f"float32 oracle differs from the float64 oracle by {worst32:.2e} on this scene"
    return g, cams, (G2, Gco, Grgb), ref, worst32


_FORWARD = {}


def _forward(N, B, deg, device):
    """what K1 saves for the backward, per camera, on the device (once per case)"""
    key = (N, B, deg)
    if key in _FORWARD:
        return _FORWARD[key]
    import diff_gaussian_rasterization as dgr

    g, cams, (G2, Gco, Grgb), _, _ = _scene(N, B, deg)
    d = {k: v.to(device).contiguous() for k, v in g.items()}
    radii = torch.empty((B, N), dtype=torch.int32, device=device)
    clamped = torch.empty((B, N, 3), dtype=torch.uint8, device=device)
    cov3D = torch.zeros((N, 6), dtype=torch.float32, device=device)
    recs = []
    for b, cam in enumerate(cams):
        rs = settings_from(cam, torch.zeros(3), sh_degree=deg, device=device)
        recs.append(dgr.pack_camera(rs))
        m2, dep, co, rgb = (torch.empty((N, k), dtype=torch.float32, device=device) for k in (2, 1, 4, 3))
        cov_b = torch.empty((N, 6), dtype=torch.float32, device=device)  # (the one-camera K1 zeroes culled rows)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        dgr.check(dgr.lib.gsr_preprocess_forward(
            N, deg, 16, p(d["means3D"]), p(d["scales"]), 1.0, p(d["rotations"]), p(d["shs"]), p(d["opacities"]),
            p(rs.viewmatrix), p(rs.projmatrix), p(rs.campos), W, H, float(rs.tanfovx), float(rs.tanfovy), p(m2), p(dep),
            p(radii[b]), p(cov_b), p(co), p(rgb), p(clamped[b]), None), "gsr_preprocess_forward")
        cov3D = torch.where((radii[b] > 0)[:, None], cov_b, cov3D)  # camera independent where it is defined
    torch.cuda.synchronize()
    out = dict(d=d, cams=torch.stack(recs), radii=radii, clamped=clamped, cov3D=cov3D,
               G2=G2.to(device).contiguous(), Gco=Gco.to(device).contiguous(), Grgb=Grgb.to(device).contiguous())
    _FORWARD[key] = out
    return out


def _run(f, deg, stride=0, raw=False, rows=None, workspace=None, grads=None):
    """the kernel on (a row slice of) a case -> dL_dcams [B,40]"""
    import diff_gaussian_rasterization as dgr

    sl = slice(None) if rows is None else slice(*rows)
    d = f["d"]
    shs = d["shs"][sl].contiguous()
    sh = (shs[:, :1].contiguous(), shs[:, 1:].contiguous()) if raw else shs
    G2, Gco, Grgb = [t[:, sl].contiguous() for t in (grads or (f["G2"], f["Gco"], f["Grgb"]))]
    B, P = G2.shape[:2]
    if stride == 9:  # column views of ONE [B*P,9] record: means2D 0:2, rgb 2:5, conic_opacity 5:9 (K10's layout)
        rec = torch.cat([G2, Grgb, Gco], dim=2).view(B * P, 9).contiguous()
        g2, grgb, gco = rec[:, 0:2], rec[:, 2:5], rec[:, 5:9]
    else:
        g2, grgb, gco = G2, Grgb, Gco
    return dgr.preprocess_backward_cameras(d["means3D"][sl].contiguous(), sh, f["cams"], W, H, deg,
                                           f["radii"][:, sl].contiguous(), f["cov3D"][sl].contiguous(),
                                           f["clamped"][:, sl].contiguous(), g2, gco, grgb, gstride=stride,
                                           workspace=workspace)


def _blocks(rec):
    return rec[0:16].view(4, 4), rec[16:32].view(4, 4), rec[32:35]


def _assert_structural_zeros(out, deg):
    o = out.cpu()
    assert torch.equal(o[:, 35:40], torch.zeros_like(o[:, 35:40])), "record words 35..39"
    assert torch.equal(o[:, 3:16:4], torch.zeros_like(o[:, 3:16:4])), "column 3 of the view matrix"
    assert torch.equal(o[:, 18:32:4], torch.zeros_like(o[:, 18:32:4])), "column 2 of the projection matrix"
    if deg == 0:
        assert torch.equal(o[:, 32:35], torch.zeros_like(o[:, 32:35])), "campos at degree 0"


@pytest.mark.parametrize("raw", [False, True], ids=["shs", "dc_rest"])
@pytest.mark.parametrize("stride", [0, 9])
@pytest.mark.parametrize("N,B,deg", CASES)
def test_kernel_matches_float64_oracle(device, N, B, deg, stride, raw):
    """Measured on MI355X: worst block and camera 4.6e-6 ... 6.5e-6 over the six cases, the same for all four forms
    (EXPERIMENTS.md, 'Camera pose gradients'); each figure is printed before it is asserted."""
    _, _, _, ref, worst32 = _scene(N, B, deg)
    out = _run(_forward(N, B, deg, device), deg, stride=stride, raw=raw)
    assert out.shape == (B, 40) and bool(torch.isfinite(out).all())
    _assert_structural_zeros(out, deg)
    worst = 0.0
    for b in range(B):
        for name, a, e in zip(BLOCKS, _blocks(out[b]), ref[b][:3]):
            err = rel_err(a, e)
            worst = max(worst, err)
            print(f"camera-grad N={N} B={B} deg={deg} stride={stride} raw={int(raw)} cam={b} {name}: rel_err {err:.3e} "
                  f"|ref| {float(e.norm()):.3e}")
            assert err <= BOUND, (b, name, err)
    assert int((ref[0][3] > 0).sum()) > 0, "camera 0 sees nothing: the case checks nothing"
    print(f"camera-grad case N={N} B={B} deg={deg} stride={stride} raw={int(raw)}: worst {worst:.3e} "
          f"(float32 oracle {worst32:.3e})")


def test_hygiene(device):
    """culled rows are never read, the workspace need not be clean, two runs agree bit for bit, empty inputs give zeros"""
    import diff_gaussian_rasterization as dgr

    N, B, deg = 3001, 3, 3
    f = _forward(N, B, deg, device)
    base = _run(f, deg)
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    culled = f["radii"] <= 0
    assert int(culled.sum()) > 0
    for stride in (0, 9):
        poisoned = []
        for t in (f["G2"], f["Gco"], f["Grgb"]):
            t = t.clone()
            t[culled] = float("nan")
            poisoned.append(t)
        assert torch.equal(_run(f, deg, stride=stride, grads=poisoned), base), f"NaN rows of culled Gaussians, stride {stride}"
    nbytes = dgr.lib.gsr_preprocess_backward_cams_bytes(N, B)
    dirty = torch.full((nbytes,), 255, dtype=torch.uint8, device=device)
    assert torch.equal(_run(f, deg, workspace=dirty), base), "0xFF workspace"
    assert torch.equal(_run(f, deg), base), "run-to-run"
    # P == 0: zeros, whatever the output held
    out = torch.full((B, 40), 7.0, device=device)
    ws = torch.empty(dgr.lib.gsr_preprocess_backward_cams_bytes(0, B), dtype=torch.uint8, device=device)
    dgr.check(dgr.lib.gsr_preprocess_backward_cams(0, B, deg, 16, None, None, 48, None, 48, None, W, H, None, None, None,
                                                   None, None, None, 0, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                                   ctypes.c_void_p(out.data_ptr()), None), "P == 0")
    assert torch.equal(out.cpu(), torch.zeros(B, 40))
    # every Gaussian behind the camera: K1 culls them all (the saved cov3D / clamp flags are then never looked at)
    g = {k: v.clone() for k, v in f["d"].items()}
    g["means3D"][:, 2] = -g["means3D"][:, 2]
    rs = settings_from(S.orbit_cameras(1, W, H)[0], torch.zeros(3), device=device)
    radii = dgr.GaussianRasterizer(rs).preprocess_gaussians(*[g[k] for k in KEYS], {})[3]
    assert int((radii > 0).sum()) == 0
    out = dgr.preprocess_backward_cameras(g["means3D"], g["shs"], dgr.pack_camera(rs).view(1, 40), W, H, deg,
                                          radii.view(1, N), f["cov3D"], f["clamped"][:1].contiguous(), f["G2"][0],
                                          f["Gco"][0], f["Grgb"][0])
    assert torch.equal(out.cpu(), torch.zeros(1, 40))


def test_shard_additivity(device):
    """what world size > 1 relies on: the result is the sum over shards of Gaussians.  fp32 per-lane sums of at most a
    few rows (one row at this size), fp64 from there on, one rounding per shard result: nothing above ~1e-7 is left
    (two roundings to fp32 of the parts against one of the whole).  Measured on MI355X: 6.0e-10 ... 6.3e-8."""
    N, B, deg = 3001, 3, 3
    f = _forward(N, B, deg, device)
    whole = _run(f, deg)
    parts = _run(f, deg, rows=(0, 1500)).double() + _run(f, deg, rows=(1500, 3001)).double()
    for b in range(B):
        for name, a, e in zip(BLOCKS, _blocks(parts[b]), _blocks(whole[b])):
            err = rel_err(a, e)
            print(f"camera-grad shard additivity cam={b} {name}: rel_err {err:.3e}")
            assert err <= 1e-6, (b, name, err)


# ------------------------------------------------------------------------------------------ through the operator
E2E_N, E2E_SEED = 2000, 3


@functools.lru_cache(maxsize=None)
def _e2e_reference():
    """float64 oracle chain (preprocess + render) of the end-to-end scene for two orbit cameras; the float32 chain has
    to stay within FP32_SHARE of it"""
    m = S.SyntheticGaussianModel(E2E_N, W, H, seed=E2E_SEED, scale_coef=0.02)
    cams = S.orbit_cameras(2, W, H)
    gen = torch.Generator().manual_seed(9)
    wgt = torch.rand(3, H, W, generator=gen) + 0.1 * torch.arange(W).float() / W  # fixed, non-constant
    bg = torch.tensor([0.2, 0.5, 0.1])
    with torch.no_grad():
        ins = [m._xyz.double(), torch.exp(m._scaling.double()), torch.nn.functional.normalize(m._rotation.double()),
               torch.cat((m._features_dc, m._features_rest), dim=1).double(), torch.sigmoid(m._opacity.double())]
    mask = torch.ones((H + 15) // 16, (W + 15) // 16, dtype=torch.bool)
    ref = []
    for cam in cams:
        def loss_of(m2, rgb, co, radii, depths):
            img, _, _ = O.render(m2, co, rgb, depths, radii, mask, bg=bg, W=W, H=H)
            return (img * wgt.to(img.dtype)).sum()

        r64 = _oracle_camera_grads(ins, cam, 3, loss_of, torch.float64)
        r32 = _oracle_camera_grads(ins, cam, 3, loss_of, torch.float32)
        for name, a, e in zip(BLOCKS, r32[:3], r64[:3]):
            assert rel_err(a, e) <= FP32_SHARE, f"float32 oracle chain, {name}: {rel_err(a, e):.2e} (pick another seed)"
        ref.append(r64[:3])
    return m, cams, wgt, bg, mask, ref


def _render_loss(dgr, cam, bg, mask, wgt, deg, outs, device):
    rast = dgr.GaussianRasterizer(settings_from(cam, bg, sh_degree=deg, device=device))
    m2, rgb, co, radii, depths = outs
    img, _, _, _ = rast.render_gaussians(m2, co, rgb, depths, radii, mask.to(device), None, {})
    return (img * wgt.to(device)).sum()


def test_end_to_end_single_camera_ops(device):
    """GaussianRasterizer.preprocess_gaussians / _raw with camera leaves -> render -> backward: `.grad` of the three"""
    import diff_gaussian_rasterization as dgr

    m, cams, wgt, bg, mask, ref = _e2e_reference()
    raw = [getattr(m, n).detach().to(device) for n in ("_xyz", "_scaling", "_rotation", "_features_dc",
                                                       "_features_rest", "_opacity")]
    act = [raw[0], torch.exp(raw[1]), torch.nn.functional.normalize(raw[2]), torch.cat((raw[3], raw[4]), dim=1),
           torch.sigmoid(raw[5])]
    for b, cam in enumerate(cams):
        for form in ("activated", "raw"):
            leaves = [t.to(device).clone().requires_grad_() for t in
                      (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
            rs = settings_from(cam, bg, device=device)._replace(viewmatrix=leaves[0], projmatrix=leaves[1],
                                                                campos=leaves[2])
            rast = dgr.GaussianRasterizer(rs)
            outs = rast.preprocess_gaussians(*act, {}) if form == "activated" else \
                rast.preprocess_gaussians_raw(*raw, {})
            _render_loss(dgr, cam, bg, mask, wgt, 3, outs, device).backward()
            for name, leaf, e in zip(BLOCKS, leaves, ref[b]):
                assert leaf.grad is not None and leaf.grad.shape == leaf.shape
                err = rel_err(leaf.grad, e)
                print(f"camera-grad end-to-end {form} cam={b} {name}: rel_err {err:.3e}")
                assert err <= BOUND, (form, b, name, err)


def test_end_to_end_batched_op(device):
    """preprocess_gaussians_raw_batched with cams.requires_grad_(), B = 2"""
    import diff_gaussian_rasterization as dgr

    m, cams, wgt, bg, mask, ref = _e2e_reference()
    raw = [getattr(m, n).detach().to(device).requires_grad_() for n in ("_xyz", "_scaling", "_rotation", "_features_dc",
                                                                        "_features_rest", "_opacity")]
    rss = [settings_from(c, bg, device=device) for c in cams]
    rec = torch.stack([dgr.pack_camera(rs) for rs in rss]).requires_grad_()
    per_cam = dgr.preprocess_gaussians_raw_batched(*raw, rec, 3, 1.0, W, H)
    loss = sum(_render_loss(dgr, cam, bg, mask, wgt, 3, [per_cam[c][b] for c in range(5)], device)
               for b, cam in enumerate(cams))
    loss.backward()
    assert rec.grad is not None and rec.grad.shape == (2, 40) and all(t.grad is not None for t in raw)
    _assert_structural_zeros(rec.grad, 3)
    for b in range(2):
        for name, a, e in zip(BLOCKS, _blocks(rec.grad[b]), ref[b]):
            err = rel_err(a, e)
            print(f"camera-grad end-to-end batched cam={b} {name}: rel_err {err:.3e}")
            assert err <= BOUND, (b, name, err)


def _batched_run(device, cams_grad, fuse=False, timer=False):
    """one forward + backward through the batched op with a loss on its own outputs (deterministic: no atomics between
    the loss and the node) -> (cams.grad, parameter gradients or updated parameters, kernel_timer records)"""
    import diff_gaussian_rasterization as dgr
    from fused_optim import FusedAdam

    N, B = 3001, 2
    m = S.SyntheticGaussianModel(N, W, H, seed=4, device=device, scale_coef=0.02)
    names = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")
    before = [getattr(m, n).detach().clone() for n in names]
    rss = [settings_from(c, torch.zeros(3), device=device) for c in S.orbit_cameras(B, W, H)]
    rec = torch.stack([dgr.pack_camera(rs) for rs in rss])
    if cams_grad:
        rec.requires_grad_()
    gen = torch.Generator().manual_seed(5)
    ws = [[torch.randn(s, generator=gen).to(device) for s in [(N, 2), (N, 3), (N, 4)]] for _ in range(B)]
    opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=fuse)
    dgr.kernel_timer.reset()
    dgr.kernel_timer.enabled = timer
    try:
        m2, rgb, co, radii, depths = dgr.preprocess_gaussians_raw_batched(
            *[getattr(m, n) for n in names], rec, 3, 1.0, W, H, tanfov0=(rss[0].tanfovx, rss[0].tanfovy))
        loss = sum((m2[k] * ws[k][0]).sum() + (rgb[k] * ws[k][1]).sum() + (co[k] * ws[k][2]).sum() for k in range(B))
        loss.backward()
        torch.cuda.synchronize()
        records = {k: len(v) for k, v in dgr.kernel_timer.records.items()}
        grads = [getattr(m, n).grad for n in names]
        if fuse:
            assert all(g is None for g in grads), "the fused step owns the parameter gradients"
            opt.step()
            assert opt.fused_steps == 1
            torch.cuda.synchronize()
        after = [getattr(m, n).detach().clone() for n in names]
    finally:
        dgr.kernel_timer.enabled = False
        dgr.kernel_timer.reset()
        opt.set_fuse_backward(False)
    return rec.grad, grads, records, before, after


def test_no_behaviour_change_without_camera_grad(device):
    """no camera tensor requires grad: no launch, no range, None for `cams`; with it: exactly one launch per backward,
    and the six parameter gradients are the same bits"""
    g0, p0, r0, _, _ = _batched_run(device, cams_grad=False, timer=True)
    g1, p1, r1, _, _ = _batched_run(device, cams_grad=True, timer=True)
    assert g0 is None and "preprocess_backward_camera" not in r0 and r0.get("preprocess_backward") == 1
    assert g1 is not None and r1.get("preprocess_backward_camera") == 1 and r1.get("preprocess_backward") == 1
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)


def test_fused_adam_sink_keeps_the_camera_gradient(device):
    """with the fused K11 + Adam sink installed the camera launch happens in backward(), before the offer: cams.grad is
    the non-fused run's bit for bit, and the step updates the parameters.  (The loss sits directly on the op's outputs:
    K10's atomics would make two renders differ in the last bits; test_fused_adam_sink_through_the_render checks the
    fused path through the render against the oracle.)"""
    g_plain, _, _, _, _ = _batched_run(device, cams_grad=True)
    g_fused, _, _, before, after = _batched_run(device, cams_grad=True, fuse=True)
    assert g_fused is not None and torch.equal(g_fused, g_plain)
    assert all(not torch.equal(a, b) for a, b in zip(before, after)), "the fused step did not move the parameters"


def test_fused_adam_sink_through_the_render(device):
    """the end-to-end path of test_end_to_end_batched_op (render, then the weighted image loss) with the fused
    K11 + Adam sink installed: cams.grad against the float64 oracle chain at the same bound, the six parameters get no
    `.grad` and are moved by the step"""
    import diff_gaussian_rasterization as dgr
    from fused_optim import FusedAdam

    _, cams, wgt, bg, mask, ref = _e2e_reference()
    m = S.SyntheticGaussianModel(E2E_N, W, H, seed=E2E_SEED, device=device, scale_coef=0.02)  # the reference's scene
    names = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")
    before = [getattr(m, n).detach().clone() for n in names]
    rec = torch.stack([dgr.pack_camera(settings_from(c, bg, device=device)) for c in cams]).requires_grad_()
    opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True)
    try:
        per_cam = dgr.preprocess_gaussians_raw_batched(*[getattr(m, n) for n in names], rec, 3, 1.0, W, H)
        loss = sum(_render_loss(dgr, cam, bg, mask, wgt, 3, [per_cam[c][b] for c in range(5)], device)
                   for b, cam in enumerate(cams))
        loss.backward()
        assert all(getattr(m, n).grad is None for n in names), "the fused step owns the parameter gradients"
        opt.step()
        assert opt.fused_steps == 1
        torch.cuda.synchronize()
    finally:
        opt.set_fuse_backward(False)
    assert rec.grad is not None and rec.grad.shape == (2, 40)
    _assert_structural_zeros(rec.grad, 3)
    for b in range(2):
        for name, a, e in zip(BLOCKS, _blocks(rec.grad[b]), ref[b]):
            err = rel_err(a, e)
            print(f"camera-grad end-to-end batched, fused sink cam={b} {name}: rel_err {err:.3e}")
            assert err <= BOUND, (b, name, err)
    assert all(not torch.equal(a, getattr(m, n).detach()) for a, n in zip(before, names)), "the step moved nothing"


# ------------------------------------------------------------------------------------------ renderer mirror
@pytest.fixture
def single_rank_world():
    """one rank, batch size 1, the test's image size; the globals of utils.general_utils are put back afterwards"""
    import utils.general_utils as utils

    fields = ("ARGS", "GLOBAL_RANK", "WORLD_SIZE", "DEFAULT_GROUP", "IN_NODE_GROUP", "IMG_H", "IMG_W", "TILE_Y", "TILE_X",
              "CUR_ITER")
    saved = {k: getattr(utils, k) for k in fields if hasattr(utils, k)}
    utils.GLOBAL_RANK, utils.WORLD_SIZE = 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=1))
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    try:
        yield utils
    finally:
        for k, v in saved.items():
            setattr(utils, k, v)


def test_renderer_mirror_delivers_pose_gradients_and_the_graphed_step_refuses(device, single_rank_world):
    utils = single_rank_world
    from fused_optim import FusedAdam
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final
    from graphed_step import GraphedIteration

    N = 2000
    cam = S.orbit_cameras(8, W, H, device=device)[1]  # (a fresh object: the pose tensors assigned below stay local)
    base = cam.world_view_transform.clone()
    delta = torch.eye(4, device=device).requires_grad_()
    bg = torch.zeros(3, device=device)
    pipe = type("P", (), {"debug": False})()
    m = S.SyntheticGaussianModel(N, W, H, seed=7, device=device, scale_coef=0.02)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset([cam]), 1, 0)
    gen = torch.Generator().manual_seed(3)
    wgt = torch.rand(3, H, W, generator=gen).to(device)
    seen = []
    for it in range(2):
        utils.set_cur_iter(it + 1)
        wv = base @ delta
        cam.world_view_transform = wv
        cam.full_proj_transform = wv @ cam.projection_matrix
        cam.camera_center = torch.inverse(wv.cpu())[3, :3].to(device)
        st, tasks = start_strategy_final([cam], hist)
        pkg = distributed_preprocess3dgs_and_all2all_final([cam], m, pipe, bg, batched_strategies=st)
        images, _ = render_final(pkg, st)
        (images[0] * wgt).sum().backward()  # (a stale cached record would fail here in the second iteration)
        assert delta.grad is not None and bool(torch.isfinite(delta.grad).all()) and float(delta.grad.abs().max()) > 0
        assert not hasattr(cam, "_gsr_packed")
        seen.append(delta.grad.clone())
        delta.grad = None
        for p in m.parameters():
            p.grad = None
    assert rel_err(seen[1], seen[0]) < 1e-3  # same pose, same scene: the same gradient (up to K10's atomics)
    step = GraphedIteration(FusedAdam(m.param_groups(), lr=0.0, eps=1e-15), lambda *a: None)
    with pytest.raises(ValueError, match="requires grad"):
        step([cam], st, tasks)
