"""K1 / K11 through the C ABI, every row against the float64 autograd oracle at the projection's edges.

The three root forms -- gsr_preprocess_forward / _backward (activated inputs), the _raw pair and the camera-batched
_raw_batched pair -- on the scene families of tests/projection_refs.py: `radii` and `clamped` equal on every row, every
float tensor through helpers.assert_rows_close (per row: max error <= K = 8 times the float32 oracle's own worst per-row
relative error, times the row's largest value; zero rows exactly zero; nothing excluded).  K11 reads the device's own
K1 outputs, as in training; outputs are pre-filled with NaN, and the incoming gradient rows of culled Gaussians are NaN.
The fused, `_dyn` and sparse forms stay tied to these roots by the bit-equality tests of tests/test_gpu_sparse_adam.py
and tests/test_gpu_loss_and_step.py; the last test here states that tie on two of the new families.

Each figure (unit in 2^-24, worst ratio) is printed before it is asserted: EXPERIMENTS.md, 'Projection rows against
float64', has the table measured on the MI355X."""
import ctypes
import functools
import math

import pytest
import torch

import projection_refs as R
import synthetic_scene as S
from helpers import KEYS, assert_rows_close
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def _p(t):
    return t.data_ptr() if t is not None else None


def _nan(shape, device):
    return torch.full(shape, NAN, dtype=torch.float32, device=device)


def _cam_args(cam, device):
    """viewmatrix, projmatrix, campos on the device (kept alive by the caller) and the float32 tangents"""
    mats = [t.to(device).float().contiguous() for t in (cam.world_view_transform, cam.full_proj_transform,
                                                         cam.camera_center)]
    return mats, R.tanfov(cam)


def _forward(form, d, cams, deg, M, sm, W, H, device, P=None):
    """K1 of one form into NaN-filled outputs -> (code, dict of the outputs [B,N,...]; cov3D [N,6])"""
    lib = _lib()
    N = d[next(iter(d))].shape[0]
    B = len(cams)
    out = dict(means2D=_nan((B, N, 2), device), depths=_nan((B, N), device), conic_opacity=_nan((B, N, 4), device),
               rgb=_nan((B, N, 3), device), cov3D=_nan((N, 6), device),
               radii=torch.full((B, N), -7, dtype=torch.int32, device=device),
               clamped=torch.full((B, N, 3), 9, dtype=torch.uint8, device=device))
    tail = [_p(out[k]) for k in ("means2D", "depths", "radii", "cov3D", "conic_opacity", "rgb", "clamped")]
    P = N if P is None else P
    if form == "rawb":
        packed = R.pack_cameras(cams).to(device)
        code = lib.gsr_preprocess_forward_raw_batched(P, B, deg, M, _p(d["xyz"]), _p(d["scaling"]), sm, _p(d["rotation"]),
                                                      _p(d["features_dc"]), _p(d["features_rest"]), _p(d["opacity"]),
                                                      _p(packed), W, H, *tail, _stream())
    else:
        assert B == 1
        mats, (tx, ty) = _cam_args(cams[0], device)
        if form == "raw":
            code = lib.gsr_preprocess_forward_raw(P, deg, M, _p(d["xyz"]), _p(d["scaling"]), sm, _p(d["rotation"]),
                                                  _p(d["features_dc"]), _p(d["features_rest"]), _p(d["opacity"]),
                                                  *[_p(t) for t in mats], W, H, tx, ty, *tail, _stream())
        else:
            code = lib.gsr_preprocess_forward(P, deg, M, _p(d["means3D"]), _p(d["scales"]), sm, _p(d["rotations"]),
                                              _p(d["shs"]), _p(d["opacities"]), *[_p(t) for t in mats], W, H, tx, ty,
                                              *tail, _stream())
    torch.cuda.synchronize()
    return code, out


def _grad_views(G2, Gco, Grgb, stride):
    """dense tensors (stride 0) or column views of ONE [B*N,9] record: means2D 0:2, rgb 2:5, conic_opacity 5:9"""
    B, N = G2.shape[:2]
    if stride == 0:
        return None, G2.contiguous(), Gco.contiguous(), Grgb.contiguous()
    assert stride == 9
    rec = torch.cat([G2, Grgb, Gco], dim=2).reshape(B * N, 9).contiguous()
    return rec, rec[:, 0:2], rec[:, 5:9], rec[:, 2:5]


def _backward(form, d, cams, deg, M, sm, W, H, device, fwd, grads_in, stride, P=None):
    """K11 of one form on the device's own K1 outputs into NaN-filled gradients -> (code, dict)"""
    lib = _lib()
    N = d[next(iter(d))].shape[0]
    B = len(cams)
    keep, g2, gco, grgb = _grad_views(*grads_in, stride)
    saved = [_p(fwd["radii"]), _p(fwd["cov3D"]), _p(fwd["clamped"]), _p(g2), _p(gco), _p(grgb), stride]
    P = N if P is None else P
    if form == "act":
        out = dict(d_means3D=_nan((N, 3), device), d_scales=_nan((N, 3), device), d_rotations=_nan((N, 4), device),
                   d_shs=_nan((N, M, 3), device), d_opacities=_nan((N, 1), device))
        mats, (tx, ty) = _cam_args(cams[0], device)
        code = lib.gsr_preprocess_backward(P, deg, M, _p(d["means3D"]), _p(d["scales"]), sm, _p(d["rotations"]),
                                           _p(d["shs"]), *[_p(t) for t in mats], W, H, tx, ty, *saved,
                                           *[_p(out[k]) for k in R.GRADS_ACT], _stream())
    else:
        out = dict(d_xyz=_nan((N, 3), device), d_scaling=_nan((N, 3), device), d_rotation=_nan((N, 4), device),
                   d_features_dc=_nan((N, 1, 3), device), d_features_rest=_nan((N, M - 1, 3), device),
                   d_opacity=_nan((N, 1), device))
        params = [_p(d["xyz"]), _p(d["scaling"]), sm, _p(d["rotation"]), _p(d["features_dc"]), _p(d["features_rest"]),
                  _p(d["opacity"])]
        if form == "raw":
            mats, (tx, ty) = _cam_args(cams[0], device)
            code = lib.gsr_preprocess_backward_raw(P, deg, M, *params, *[_p(t) for t in mats], W, H, tx, ty, *saved,
                                                   *[_p(out[k]) for k in R.GRADS_RAW], _stream())
        else:
            packed = R.pack_cameras(cams).to(device)
            code = lib.gsr_preprocess_backward_raw_batched(P, B, deg, M, *params, _p(packed), W, H, *saved,
                                                           *[_p(out[k]) for k in R.GRADS_RAW], _stream())
    torch.cuda.synchronize()
    del keep
    return code, out


_RESULTS = {}


def _device_run(case, device):
    """K1, then K11 on K1's own outputs, of one case -> dict of CPU tensors (computed once per case, never modified)"""
    if case.id in _RESULTS:
        return _RESULTS[case.id]
    ins, cams = case.inputs()
    d = {k: v.to(device).contiguous() for k, v in ins.items()}
    code, fwd = _forward(case.form, d, cams, case.deg, case.M, case.sm, case.W, case.H, device)
    assert code == 0, f"K1 returned {code}"
    culled = fwd["radii"] <= 0
    grads_in = []
    for t in R.upstream(case.B, case.N):
        t = t.to(device).clone()
        t[culled] = NAN  # the incoming gradient rows of culled Gaussians are never to be used
        grads_in.append(t)
    code, bwd = _backward(case.form, d, cams, case.deg, case.M, case.sm, case.W, case.H, device, fwd, grads_in,
                          case.stride)
    assert code == 0, f"K11 returned {code}"
    res = {k: v.cpu() for k, v in {**fwd, **bwd}.items()}
    _RESULTS[case.id] = res
    return res


@functools.lru_cache(maxsize=None)
def _cov3d_reference(case):
    """the batched K1 writes cov3D [N,6] once, for every row, whichever cameras see it: Sigma from the getters' values"""
    ins, _ = case.inputs()
    return tuple(O.cov3d_from_scale_rot(a["scales"], a["rotations"], case.sm)
                 for a in (R.activate(ins, torch.float64), R.activate(ins, torch.float32)))


# ------------------------------------------------------------------------------------------------ 1. the root forms
@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_every_row_against_float64(device, case):
    r64, r32 = case.references()
    got = _device_run(case, device)
    N, B = case.N, case.B
    assert torch.equal(got["radii"], r64["radii"]), \
        f"radii differ on rows {torch.nonzero(got['radii'] != r64['radii'])[:8].tolist()}"
    assert torch.equal(got["clamped"].bool(), r64["clamped"]) and int(got["clamped"].max()) <= 1, "clamped"
    culled = r64["radii"] <= 0
    worst_of = {}
    for k in R.OUTPUTS:
        if k == "cov3D" and case.form == "rawb":
            c64, c32 = _cov3d_reference(case)
            for b in range(B):  # (where a camera sees the row, its oracle's Sigma is this one)
                vis = ~culled[b]
                assert torch.equal(r64["cov3D"][b][vis], c64[vis])
            unit, worst = assert_rows_close(got[k], c64, c32, what=f"{case.id} cov3D")
        else:
            unit = worst = 0.0
            for b in range(B):
                g = got[k][b] if k != "cov3D" else got[k]
                u, w = assert_rows_close(g, r64[k][b], r32[k][b], what=f"{case.id} {k} camera {b}")
                unit, worst = max(unit, u), max(worst, w)
                assert not bool(g[culled[b]].any()), f"{k}: a culled row of camera {b} is not zero"  # (NaN counts)
        worst_of[k] = (unit, worst)
    culled_all = culled.all(dim=0)
    for k in case.tensors()[len(R.OUTPUTS):]:
        worst_of[k] = assert_rows_close(got[k], r64[k], r32[k], what=f"{case.id} {k}")
        assert not bool(got[k][culled_all].any()), f"{k}: a culled row is not zero"
    for k, (unit, worst) in worst_of.items():
        print(f"ROWS hip {case.id} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")
    assert all(w <= 8 for _, w in worst_of.values())
    assert int((~culled).sum()) > 0, "nothing visible: the case checks nothing"


# ------------------------------------------------------------------------------------------------ 2. above the degree
LOW_DEGREE = [c for c in R.CASES if c.deg < 3 and c.M == 16]


@pytest.mark.parametrize("case", LOW_DEGREE, ids=[c.id for c in LOW_DEGREE])
def test_gradients_above_the_active_degree_are_zero(device, case):
    """the words of SH coefficients above the active degree: exactly zero, on every row (the per-row check alone would
    let them be as large as its tolerance times the row's dc gradient)"""
    got = _device_run(case, device)
    nc = (case.deg + 1) ** 2
    if case.form == "act":
        above, below = got["d_shs"][:, nc:], got["d_shs"][:, :nc]
    else:
        above, below = got["d_features_rest"][:, nc - 1:], got["d_features_dc"]
    assert above.shape[1] == 16 - nc and not bool(above.any()), "a gradient word above the active degree is not zero"
    assert bool(below.any()), "the gradient at the active degree is all zero: the case checks nothing"


# ------------------------------------------------------------------------------------------------ 3. exact rows of K1
@pytest.mark.parametrize("form", ["act", "raw", "rawb"])
def test_exact_cull_rows_of_k1(device, form):
    """the identity camera, where t = p exactly in float32: t.z == 0.2f is culled (<=), the next float is kept, t.z < 0 is
    culled, a row in front whose rect holds no tile is culled; P = 0 returns success and writes nothing"""
    W, H = R.FRAMES[0]
    cam = S.SyntheticCamera(0, W, H)
    assert torch.equal(cam.world_view_transform, torch.eye(4))
    near = torch.tensor(0.2, dtype=torch.float32)
    nxt = torch.nextafter(near, torch.tensor(1.0))
    assert float(nxt) > float(near)
    tanx = math.tan(cam.FoVx / 2)
    means = torch.tensor([[0.0, 0.0, float(near)], [0.0, 0.0, float(nxt)], [0.0, 0.0, -1.0], [5.0 * 3.0 * tanx, 0.0, 3.0],
                          [0.1, 0.1, 3.0]])
    n = means.shape[0]
    act = dict(means3D=means, scales=torch.full((n, 3), 0.01) * means[:, 2:3].abs(),
               rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1),
               shs=torch.cat([torch.full((n, 1, 3), 1.0), torch.zeros(n, 15, 3)], dim=1), opacities=torch.full((n, 1), 0.5))
    ins = act if form == "act" else R.to_raw(act)
    d = {k: v.to(device).contiguous() for k, v in ins.items()}
    code, out = _forward(form, d, [cam], 3, 16, 1.0, W, H, device)
    assert code == 0
    radii = out["radii"][0].cpu()
    assert (radii > 0).tolist() == [False, True, False, False, True], radii.tolist()
    assert out["depths"][0].cpu()[1].view(torch.int32) == nxt.view(torch.int32), "depth of the kept row: t.z itself"
    for k in ("means2D", "depths", "conic_opacity", "rgb"):
        assert not bool(out[k][0].cpu()[radii <= 0].any()), f"{k}: culled rows are zero"
    # P = 0: success, and not one word written
    code, out = _forward(form, d, [cam], 3, 16, 1.0, W, H, device, P=0)
    assert code == 0
    assert all(bool(torch.isnan(out[k]).all()) for k in R.OUTPUTS)
    assert bool((out["radii"] == -7).all()) and bool((out["clamped"] == 9).all())
    fwd = dict(radii=torch.ones((1, n), dtype=torch.int32, device=device), cov3D=torch.ones((n, 6), device=device),
               clamped=torch.zeros((1, n, 3), dtype=torch.uint8, device=device))
    grads_in = [t.to(device) for t in R.upstream(1, n)]
    for stride in (0, 9):
        code, g = _backward(form, d, [cam], 3, 16, 1.0, W, H, device, fwd, grads_in, stride, P=0)
        assert code == 0 and all(bool(torch.isnan(t).all()) for t in g.values())


# ------------------------------------------------------------------------------------------------ 4. the derived forms
@pytest.mark.parametrize("fam", ["jclamp", "clamped"])
def test_fused_and_sparse_forms_equal_the_root_pair_on_the_new_families(device, fam, monkeypatch):
    """gsr_preprocess_backward_adam_raw_batched == root K11, then gsr_adam_step_multi, bit for bit, and the sparse form
    the same on the active rows -- with the helpers of tests/test_gpu_sparse_adam.py, on (B, deg, N) = (3, 3, 1031)"""
    import test_gpu_sparse_adam as SA

    B, deg, N = 3, 3, 1031
    W, H = R.FRAMES[1] if fam == "jclamp" else R.FRAMES[0]
    monkeypatch.setattr(SA, "W", W)  # the helpers take the frame from their module
    monkeypatch.setattr(SA, "H", H)
    act, cams = R.family(fam, N, W, H, deg, seed=100 + 7 * N + deg, B=B)
    raw = R.to_raw(act)
    c = SA._Case.__new__(SA._Case)
    c.B, c.deg, c.N, c.device = B, deg, N, device
    c.params = [raw[k].to(device).contiguous() for k in R.RAW_KEYS]
    c.packed = R.pack_cameras(cams).to(device)
    c.radii, c.cov3D, c.clamped = SA._forward(c.params, c.packed, deg)
    G2, Gco, Grgb = R.upstream(B, N)
    c.rec = torch.cat([G2, Grgb, Gco], dim=2).reshape(B * N, 9).to(device).contiguous()
    gen = torch.Generator().manual_seed(5)
    c.ms = [(0.01 * torch.randn(t.shape, generator=gen)).to(device) for t in c.params]
    c.vs = [(a.cpu() ** 2 * (1.0 + torch.rand(a.shape, generator=gen)) + 1e-8).to(device) for a in c.ms]
    c.grad_scale = 1.0 / B
    active, want, dense, _ = c.expected()
    assert 0 < int(active.sum()) < N
    for gstride in (0, 9):
        code, got, act_out, num = c.run(gstride)
        assert code == 0 and int(num) == int(active.sum()) and torch.equal(act_out.cpu().bool(), active)
        SA._assert_state(got, want, f"sparse form, {fam}, stride {gstride}")
        g2, grgb, gco = c.grads(gstride)
        p, m, v = [t.clone() for t in c.params], [t.clone() for t in c.ms], [t.clone() for t in c.vs]
        code = SA._lib().gsr_preprocess_backward_adam_raw_batched(
            N, B, deg, 16, SA._p(p[0]), SA._p(p[1]), 1.0, SA._p(p[2]), SA._p(p[3]), SA._p(p[4]), SA._p(p[5]),
            SA._p(c.packed), W, H, SA._p(c.radii), SA._p(c.cov3D), SA._p(c.clamped), SA._p(g2), SA._p(gco), SA._p(grgb),
            gstride, SA.VP(*[SA._p(t) for t in m]), SA.VP(*[SA._p(t) for t in v]), SA.D6(*SA.LRS), SA.D6(*SA.B1S),
            SA.D6(*SA.B2S), SA.D6(*SA.EPSS), SA.I64(*SA.STEPS), c.grad_scale, None, SA._stream())
        torch.cuda.synchronize()
        assert code == 0
        SA._assert_state((p, m, v), dense, f"fused form, {fam}, stride {gstride}")
