"""K1 / K11 under gsr_set_antialiasing(1) through the C ABI, every row against the float64 restatement of
tests/antialias_refs.py (there is no reference call site for the switch), in the manner of tests/test_gpu_projection_rows.py
whose launch helpers are reused by import: outputs pre-filled with NaN, NaN incoming gradients on culled rows, `radii`
and `clamped` equal on every row, every float tensor through helpers.assert_rows_close with K = 8, nothing excluded.
The activated form's K11 is gsr_preprocess_backward_aa.  Then: every K1 output but conic_opacity.w keeps its mode-0
bits; the fused, `_dyn` and sparse forms equal root K11 + gsr_adam_step_multi bit for bit under mode 1; mode 0 after
mode 1 is mode 0 again.

Each figure (unit in 2^-24, worst ratio) is printed before it is asserted: EXPERIMENTS.md, 'Anti-aliased rows against
float64', has the table measured on the MI355X.  Every test leaves the library in mode 0."""
import pytest
import torch

import antialias_refs as A
import projection_refs as R
import test_gpu_projection_rows as PR
from helpers import assert_rows_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
_p = PR._p


def _set_mode(mode):
    """through the operator's own setter, which remembers what it last told the library"""
    import diff_gaussian_rasterization as dgr

    dgr._lib_antialiasing(mode)


@pytest.fixture
def mode1():
    _set_mode(1)
    try:
        yield
    finally:
        _set_mode(0)


def _backward(form, d, cams, deg, M, sm, W, H, device, fwd, grads_in, stride, aa_entry=True, P=None):
    """PR._backward, with the activated form through gsr_preprocess_backward_aa (which takes the opacity)"""
    if form != "act" or not aa_entry:
        return PR._backward(form, d, cams, deg, M, sm, W, H, device, fwd, grads_in, stride, P=P)
    N = d["means3D"].shape[0]
    keep, g2, gco, grgb = PR._grad_views(*grads_in, stride)
    out = dict(d_means3D=PR._nan((N, 3), device), d_scales=PR._nan((N, 3), device), d_rotations=PR._nan((N, 4), device),
               d_shs=PR._nan((N, M, 3), device), d_opacities=PR._nan((N, 1), device))
    mats, (tx, ty) = PR._cam_args(cams[0], device)
    code = PR._lib().gsr_preprocess_backward_aa(
        N if P is None else P, deg, M, _p(d["means3D"]), _p(d["scales"]), sm, _p(d["rotations"]), _p(d["shs"]),
        _p(d["opacities"]), *[_p(t) for t in mats], W, H, tx, ty, _p(fwd["radii"]), _p(fwd["cov3D"]), _p(fwd["clamped"]),
        _p(g2), _p(gco), _p(grgb), stride, *[_p(out[k]) for k in R.GRADS_ACT], PR._stream())
    torch.cuda.synchronize()
    del keep
    return code, out


def _run(case, device, aa_entry=True):
    """K1, then K11 on K1's own outputs, under whatever mode the library is in -> dict of CPU tensors"""
    ins, cams = case.inputs()
    d = {k: v.to(device).contiguous() for k, v in ins.items()}
    code, fwd = PR._forward(case.form, d, cams, case.deg, case.M, case.sm, case.W, case.H, device)
    assert code == 0, f"K1 returned {code}"
    culled = fwd["radii"] <= 0
    grads_in = []
    for t in case.upstream():
        t = t.to(device).clone()
        t[culled] = NAN  # the incoming gradient rows of culled Gaussians are never to be used
        grads_in.append(t)
    code, bwd = _backward(case.form, d, cams, case.deg, case.M, case.sm, case.W, case.H, device, fwd, grads_in,
                          case.stride, aa_entry)
    assert code == 0, f"K11 returned {code}"
    return {k: v.cpu() for k, v in {**fwd, **bwd}.items()}


_MODE1 = {}


def _mode1_run(case, device):
    if case.id not in _MODE1:
        _set_mode(1)
        try:
            _MODE1[case.id] = _run(case, device)
        finally:
            _set_mode(0)
    return _MODE1[case.id]


# ------------------------------------------------------------------------------------------------ 1. the root forms
@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_every_row_against_float64_under_mode_1(device, case):
    r64, r32 = case.references()
    got = _mode1_run(case, device)
    B = case.B
    assert torch.equal(got["radii"], r64["radii"]), \
        f"radii differ on rows {torch.nonzero(got['radii'] != r64['radii'])[:8].tolist()}"
    assert torch.equal(got["clamped"].bool(), r64["clamped"]) and int(got["clamped"].max()) <= 1, "clamped"
    culled = r64["radii"] <= 0
    worst_of = {}
    for k in R.OUTPUTS:
        if k == "cov3D" and case.form == "rawb":
            ins, _ = case.inputs()
            c64, c32 = (PR.O.cov3d_from_scale_rot(a["scales"], a["rotations"], case.sm)
                        for a in (R.activate(ins, torch.float64), R.activate(ins, torch.float32)))
            worst_of[k] = assert_rows_close(got[k], c64, c32, what=f"{case.id} cov3D")
            continue
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
        print(f"ROWS aa {case.id} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")
    assert all(w <= 8 for _, w in worst_of.values())
    assert int((~culled).sum()) > 0, "nothing visible: the case checks nothing"


# ------------------------------------------------------------------------------------------------ 2. what K1 keeps
K1_CASES = [c for c in A.CASES if c.N >= 257 and c.fam in ("plain", "aaclamp", "tiny", "huge", "behind", "raw")]


@pytest.mark.parametrize("case", K1_CASES, ids=[c.id for c in K1_CASES])
def test_k1_keeps_every_other_output_bit(device, case):
    """mode 1 against the mode-0 launch on the same inputs: only conic_opacity.w may differ (and does, somewhere)"""
    ins, cams = case.inputs()
    d = {k: v.to(device).contiguous() for k, v in ins.items()}
    outs = []
    try:
        for mode in (0, 1):
            _set_mode(mode)
            code, fwd = PR._forward(case.form, d, cams, case.deg, case.M, case.sm, case.W, case.H, device)
            assert code == 0
            outs.append({k: v.cpu() for k, v in fwd.items()})
    finally:
        _set_mode(0)
    o0, o1 = outs
    for k in ("radii", "clamped"):
        assert torch.equal(o0[k], o1[k]), k
    for k in ("means2D", "depths", "rgb", "cov3D"):
        assert torch.equal(o0[k].view(torch.int32), o1[k].view(torch.int32)), k
    assert torch.equal(o0["conic_opacity"][..., :3].contiguous().view(torch.int32),
                       o1["conic_opacity"][..., :3].contiguous().view(torch.int32)), "conic"
    vis = o0["radii"] > 0
    w0, w1 = o0["conic_opacity"][..., 3][vis], o1["conic_opacity"][..., 3][vis]
    assert bool((w1 < w0).all()) and bool((w1 >= 0.005 * w0 * (1 - 1e-6)).all()), "0.005 <= rho < 1 on visible rows"
    assert not bool(o1["conic_opacity"][..., 3][~vis].any())


# ------------------------------------------------------------------------------------------------ 3. the derived forms
def test_fused_dyn_and_sparse_forms_equal_the_root_pair_under_mode_1(device, monkeypatch, mode1):
    """gsr_preprocess_backward_adam_raw_batched and _dyn == root K11, then gsr_adam_step_multi, bit for bit, and the
    sparse form the same on its active rows with the others untouched -- `aaclamp`, (B, deg, N) = (3, 3, 1031), both
    strides, with the helpers of tests/test_gpu_sparse_adam.py"""
    import test_gpu_sparse_adam as SA

    B, deg, N = 3, 3, 1031
    W, H = R.FRAMES[0]
    monkeypatch.setattr(SA, "W", W)  # the helpers take the frame from their module
    monkeypatch.setattr(SA, "H", H)
    act, cams = A.family("aaclamp", N, W, H, deg, seed=100 + 7 * N + deg, B=B)
    raw = R.to_raw(act)
    c = SA._Case.__new__(SA._Case)
    c.B, c.deg, c.N, c.device = B, deg, N, device
    c.params = [raw[k].to(device).contiguous() for k in R.RAW_KEYS]
    c.packed = R.pack_cameras(cams).to(device)
    c.radii, c.cov3D, c.clamped = SA._forward(c.params, c.packed, deg)
    G2, Gco, Grgb = A.upstream_aa(B, N)
    c.rec = torch.cat([G2, Grgb, Gco], dim=2).reshape(B * N, 9).to(device).contiguous()
    gen = torch.Generator().manual_seed(5)
    c.ms = [(0.01 * torch.randn(t.shape, generator=gen)).to(device) for t in c.params]
    c.vs = [(a.cpu() ** 2 * (1.0 + torch.rand(a.shape, generator=gen)) + 1e-8).to(device) for a in c.ms]
    c.grad_scale = 1.0 / B
    active, want, dense, grads1 = c.expected()
    assert 0 < int(active.sum()) < N
    # the root K11 of this case does depend on the mode: otherwise nothing below is about anti-aliasing
    _set_mode(0)
    grads0 = c.expected()[3]
    _set_mode(1)
    assert not torch.equal(grads0[1], grads1[1]) and not torch.equal(grads0[5], grads1[5])
    hyper = [SA.LRS[t] / (1.0 - SA.B1S[t] ** SA.STEPS[t]) for t in range(6)] + \
            [1.0 / (1.0 - SA.B2S[t] ** SA.STEPS[t]) ** 0.5 for t in range(6)]
    dyn = torch.tensor(hyper, dtype=torch.float32, device=device)
    for gstride in (0, 9):
        code, got, act_out, num = c.run(gstride)
        assert code == 0 and int(num) == int(active.sum()) and torch.equal(act_out.cpu().bool(), active)
        SA._assert_state(got, want, f"sparse form, stride {gstride}")  # (want: the rows that are not active untouched)
        g2, grgb, gco = c.grads(gstride)
        for use_dyn in (False, True):
            p, m, v = [t.clone() for t in c.params], [t.clone() for t in c.ms], [t.clone() for t in c.vs]
            args = [N, B, deg, 16, SA._p(p[0]), SA._p(p[1]), 1.0, SA._p(p[2]), SA._p(p[3]), SA._p(p[4]), SA._p(p[5]),
                    SA._p(c.packed), W, H, SA._p(c.radii), SA._p(c.cov3D), SA._p(c.clamped), SA._p(g2), SA._p(gco),
                    SA._p(grgb), gstride, SA.VP(*[SA._p(t) for t in m]), SA.VP(*[SA._p(t) for t in v]),
                    None if use_dyn else SA.D6(*SA.LRS), SA.D6(*SA.B1S), SA.D6(*SA.B2S), SA.D6(*SA.EPSS),
                    None if use_dyn else SA.I64(*SA.STEPS), c.grad_scale, None]
            if use_dyn:
                code = SA._lib().gsr_preprocess_backward_adam_raw_batched_dyn(*args, SA._p(dyn), None, SA._stream())
            else:
                code = SA._lib().gsr_preprocess_backward_adam_raw_batched(*args, SA._stream())
            torch.cuda.synchronize()
            assert code == 0
            SA._assert_state((p, m, v), dense, f"fused form, dyn {use_dyn}, stride {gstride}")


def test_one_camera_fused_form_equals_the_root_pair_under_mode_1(device, mode1):
    """B = 1 with the host tangents: the one-camera K11 + Adam kernel against gsr_preprocess_backward_raw + Adam"""
    import test_gpu_sparse_adam as SA

    case = [c for c in A.CASES if c.form == "raw" and c.fam == "aaclamp" and c.N == 1031][0]
    ins, cams = case.inputs()
    W, H, deg, N = case.W, case.H, case.deg, case.N
    d = {k: v.to(device).contiguous() for k, v in ins.items()}
    code, fwd = PR._forward("raw", d, cams, deg, 16, 1.0, W, H, device)
    assert code == 0
    grads_in = [t.to(device) for t in case.upstream()]
    code, bwd = PR._backward("raw", d, cams, deg, 16, 1.0, W, H, device, fwd, grads_in, 0)
    assert code == 0
    params = [d[k] for k in R.RAW_KEYS]
    gen = torch.Generator().manual_seed(5)
    ms = [(0.01 * torch.randn(t.shape, generator=gen)).to(device) for t in params]
    vs = [(a.cpu() ** 2 * (1.0 + torch.rand(a.shape, generator=gen)) + 1e-8).to(device) for a in ms]
    want = SA._adam(params, [bwd[k] for k in R.GRADS_RAW], ms, vs, SA.LRS, SA.STEPS, 1.0)
    p, m, v = [t.clone() for t in params], [t.clone() for t in ms], [t.clone() for t in vs]
    packed = R.pack_cameras(cams).to(device)
    _, g2, gco, grgb = PR._grad_views(*grads_in, 0)
    tf = (SA.ctypes.c_float * 2)(*R.tanfov(cams[0]))
    code = SA._lib().gsr_preprocess_backward_adam_raw_batched(
        N, 1, deg, 16, _p(p[0]), _p(p[1]), 1.0, _p(p[2]), _p(p[3]), _p(p[4]), _p(p[5]), _p(packed), W, H,
        _p(fwd["radii"]), _p(fwd["cov3D"]), _p(fwd["clamped"]), _p(g2), _p(gco), _p(grgb), 0,
        SA.VP(*[_p(t) for t in m]), SA.VP(*[_p(t) for t in v]), SA.D6(*SA.LRS), SA.D6(*SA.B1S), SA.D6(*SA.B2S),
        SA.D6(*SA.EPSS), SA.I64(*SA.STEPS), 1.0, tf, SA._stream())
    torch.cuda.synchronize()
    assert code == 0
    SA._assert_state((p, m, v), want, "one-camera fused form")


# ------------------------------------------------------------------------------------------------ 4. the mode
MODE_CASES = [[c for c in A.CASES if c.form == f and c.fam == "aaclamp" and c.N == 257][0] for f in ("act", "raw", "rawb")]


@pytest.mark.parametrize("case", MODE_CASES, ids=[c.id for c in MODE_CASES])
def test_mode_0_after_mode_1_is_mode_0(device, case):
    """every form reproduces its earlier mode-0 bits after mode 1 -> 0 (mode 1 in between did differ), and under mode 0
    gsr_preprocess_backward_aa gives gsr_preprocess_backward's bits"""
    try:
        _set_mode(0)
        before = _run(case, device, aa_entry=False)
        _set_mode(1)
        between = _run(case, device)
        _set_mode(0)
        after = _run(case, device, aa_entry=False)
        after_aa = _run(case, device, aa_entry=True)
    finally:
        _set_mode(0)
    k_op = "d_opacities" if case.form == "act" else "d_opacity"
    assert not torch.equal(before["conic_opacity"], between["conic_opacity"]) and \
        not torch.equal(before[k_op], between[k_op])
    for k, t in before.items():
        bits = (lambda x: x.view(torch.int32)) if t.dtype == torch.float32 else (lambda x: x)
        assert torch.equal(bits(t), bits(after[k])), f"{k}: mode 0 after mode 1 differs from mode 0 before"
        assert torch.equal(bits(t), bits(after_aa[k])), f"{k}: the _aa entry point under mode 0 differs"


def test_refusals_under_mode_1(device, mode1):
    """gsr_preprocess_backward and gsr_preprocess_backward_cams refuse real arguments under mode 1 (and write nothing);
    with P = 0 both succeed, the latter zero-filling dL_dcams"""
    lib = PR._lib()
    case = MODE_CASES[0]
    ins, cams = case.inputs()
    d = {k: v.to(device).contiguous() for k, v in ins.items()}
    code, fwd = PR._forward("act", d, cams, case.deg, 16, 1.0, case.W, case.H, device)
    assert code == 0
    grads_in = [t.to(device) for t in case.upstream()]
    code, out = PR._backward("act", d, cams, case.deg, 16, 1.0, case.W, case.H, device, fwd, grads_in, 0)
    assert code == -1 and all(bool(torch.isnan(t).all()) for t in out.values())
    code, _ = PR._backward("act", d, cams, case.deg, 16, 1.0, case.W, case.H, device, fwd, grads_in, 0, P=0)
    assert code == 0
    N = case.N
    packed = R.pack_cameras(cams).to(device)
    ws = torch.empty(int(lib.gsr_preprocess_backward_cams_bytes(N, 1)) // 8 + 1, dtype=torch.float64, device=device)
    d_cams = PR._nan((1, 40), device)
    _, g2, gco, grgb = PR._grad_views(*grads_in, 0)

    def cams_call(P):
        code = lib.gsr_preprocess_backward_cams(P, 1, case.deg, 16, _p(d["means3D"]), _p(d["shs"]), 48,
                                                d["shs"].data_ptr() + 12, 48, _p(packed), case.W, case.H,
                                                _p(fwd["radii"]), _p(fwd["cov3D"]), _p(fwd["clamped"]), _p(g2), _p(gco),
                                                _p(grgb), 0, _p(ws), ws.numel() * 8, _p(d_cams), PR._stream())
        torch.cuda.synchronize()
        return code

    assert cams_call(N) == -1 and bool(torch.isnan(d_cams).all())
    assert cams_call(0) == 0 and not bool(d_cams.any())
