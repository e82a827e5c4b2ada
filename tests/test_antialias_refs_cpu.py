"""The references of the anti-aliasing tests checked before a GPU is involved: the closed-form backward of rho against
plain float64 autograd, the conditioning of every case (helpers.ROW_UNIT_CAP), the clamp's two sides, three corrupted
results that the per-row check must refuse, and the host-only part of the C ABI (include/gsraster.h:
gsr_set_antialiasing) and of the Python setting."""
import os
import subprocess
import sys

import pytest
import torch

import antialias_refs as A
import projection_refs as R
from helpers import assert_rows_close

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def test_closed_form_backward_equals_float64_autograd():
    """Rho's backward == autograd of sqrt(clamp(det0 / det, min=0.000025)), to 1e-12 relative, on `plain` (and on
    `aaclamp`, where part of the rows sit on the clamp and receive exactly nothing)"""
    W, H = R.FRAMES[0]
    for fam in ("plain", "aaclamp"):
        act, cams = A.family(fam, 257, W, H, 3, seed=100 + 7 * 257 + 3, B=3)
        for cam in cams:
            q, front = A.q64(act, cam, W, H)
            ix = front.nonzero().squeeze(1)
            got, want = [], []
            for fn, res in ((A.Rho.apply, got), (A.rho_plain, want)):
                leaves = [act[k][ix].double().clone().requires_grad_() for k in ("means3D", "scales", "rotations")]
                a0, b, c0 = A.cov2d_abc(*leaves, cam, W, H)
                abc = [t.detach().clone().requires_grad_() for t in (a0, b, c0)]
                rho = fn(*abc)
                g = torch.linspace(-1.0, 2.0, rho.numel(), dtype=torch.float64)
                res += [rho.detach()] + list(torch.autograd.grad(rho, abc, g))
                res += list(torch.autograd.grad(fn(a0, b, c0), leaves, g))  # ... and carried on to the parameters
            for k, (x, y) in enumerate(zip(got, want)):
                scale = y.abs().reshape(y.shape[0], -1).amax(dim=1).clamp(min=1e-300)
                err = ((x - y).abs().reshape(y.shape[0], -1).amax(dim=1) / scale).max()
                assert float(err) <= 1e-12, (fam, k, float(err))
            if fam == "aaclamp":
                clamped = q[ix] <= A.QMIN
                assert bool(clamped.any()) and not bool(got[1][clamped].any()), "a clamped row has a gradient"


@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_float32_reference_stays_under_the_cap(case):
    """every tensor of every case: the float32 reference against the float64 one through assert_rows_close (which asserts
    the cap first), and both dtypes put every visible row on the same side of the clamp"""
    r64, r32 = case.references()
    assert torch.equal(r64["radii"], r32["radii"]) and torch.equal(r64["clamped"], r32["clamped"])
    assert torch.equal(r64["q_clamped"], r32["q_clamped"]), "float32 and float64 disagree about the clamp on some row"
    for k in case.tensors():
        if k in R.OUTPUTS:
            for b in range(case.B):
                assert_rows_close(r32[k][b], r64[k][b], r32[k][b], what=f"{case.id} {k} camera {b}")
        else:
            assert_rows_close(r32[k], r64[k], r32[k], what=f"{case.id} {k}")
    assert int((r64["radii"] > 0).sum()) > 0


def test_aaclamp_sits_on_both_sides_of_the_clamp():
    cases = [c for c in A.CASES if c.fam == "aaclamp" and (c.W, c.H) == R.FRAMES[0] and c.N >= 127]
    assert cases
    for c in cases:
        r64, r32 = c.references()
        vis = r64["radii"] > 0
        share = float(r64["q_clamped"][vis].double().mean())
        assert 0.25 <= share <= 0.75, (c.id, share)
        assert torch.equal(r64["q_clamped"], r32["q_clamped"])
    tiny = [c for c in A.CASES if c.fam == "tiny"][0].references()[0]
    assert bool(tiny["q_clamped"][tiny["radii"] > 0].all())
    huge = [c for c in A.CASES if c.fam == "huge"][0].references()[0]
    assert not bool(huge["q_clamped"].any())


# ------------------------------------------------------------------------------------------------ the check has teeth
def _case(form, fam):
    return [c for c in A.CASES if c.form == form and c.fam == fam and c.N >= 257][0]


def _fails(got, r64, r32, what):
    with pytest.raises(AssertionError):
        assert_rows_close(got, r64, r32, what=what)


def test_rho_left_out_of_the_opacity_gradient_fails():
    c = _case("act", "aaclamp")
    r64, r32 = c.references()
    plain = R.reference(c.inputs()[0], c.inputs()[1], c.deg, c.upstream(), torch.float64, False, c.sm)
    _fails(plain["d_opacities"], r64["d_opacities"], r32["d_opacities"], "rho left out of d_opacities")


class _RhoThroughTheClamp(torch.autograd.Function):
    """the covariance term added on clamped rows as well"""

    @staticmethod
    def forward(ctx, a0, b, c0):
        return A.Rho.forward(ctx, a0, b, c0)

    @staticmethod
    def backward(ctx, g):
        a0, b, c0, det, q, rho = ctx.saved_tensors
        w = g / (2.0 * rho)
        h = 0.3 * (a0 + c0) + 0.09
        d2 = det * det
        return (w * ((0.3 * (c0 * c0 + b * b) + 0.09 * c0) / d2), w * (-2.0 * b * h / d2),
                w * ((0.3 * (a0 * a0 + b * b) + 0.09 * a0) / d2))


def test_covariance_term_on_clamped_rows_fails():
    c = _case("act", "aaclamp")
    r64, r32 = c.references()
    bad = A.reference_aa(c.inputs()[0], c.inputs()[1], c.deg, c.upstream(), torch.float64, False, c.sm,
                         rho_fn=_RhoThroughTheClamp.apply)
    _fails(bad["d_scales"], r64["d_scales"], r32["d_scales"], "covariance term on clamped rows")


def test_quotient_rule_in_float32_on_huge_fails():
    c = _case("act", "huge")
    r64, r32 = c.references()
    bad = A.reference_aa(c.inputs()[0], c.inputs()[1], c.deg, c.upstream(), torch.float32, False, c.sm,
                         rho_fn=A.rho_plain)
    _fails(bad["d_scales"], r64["d_scales"], r32["d_scales"], "float32 quotient rule on huge")


# ------------------------------------------------------------------------------------------------ host-only ABI
def test_switch_and_refusals_without_a_device():
    """dummy non-zero integers stand for device pointers: every call below returns before anything is dereferenced or
    launched.  (gsr_preprocess_backward_cams with P = 0 zero-fills dL_dcams with a launch, so its success at P = 0 is
    checked on the GPU, tests/test_gpu_antialias_rows.py; here only that the refusal does not reach P = 0.)"""
    lib = _lib()
    d = 0x1000
    bwd = lambda P: lib.gsr_preprocess_backward(P, 3, 16, d, d, 1.0, d, d, d, d, d, 64, 64, 0.5, 0.5, d, d, d, d, d, d, 0,  # noqa: E731
                                                d, d, d, d, d, None)
    cams = lambda P: lib.gsr_preprocess_backward_cams(P, 1, 3, 16, d, d, 3, d, 45, d, 64, 64, d, d, d, d, d, d, 0, d,  # noqa: E731
                                                      1 << 20, d, None)
    try:
        assert lib.gsr_set_antialiasing(0) in (0, 1)
        assert lib.gsr_set_antialiasing(1) == 0 and lib.gsr_set_antialiasing(1) == 1
        assert lib.gsr_set_antialiasing(2) == EINVAL and lib.gsr_set_antialiasing(-1) == EINVAL
        assert lib.gsr_set_antialiasing(1) == 1, "a refused mode changed the mode"
        assert bwd(10) == EINVAL and cams(10) == EINVAL
        assert bwd(0) == 0
        assert lib.gsr_preprocess_backward_aa(0, 3, 16, d, d, 1.0, d, d, d, d, d, d, 64, 64, 0.5, 0.5, d, d, d, d, d, d, 0,
                                              d, d, d, d, d, None) == 0
        # mode 1 needs the opacity
        assert lib.gsr_preprocess_backward_aa(10, 3, 16, d, d, 1.0, d, d, None, d, d, d, 64, 64, 0.5, 0.5, d, d, d, d, d,
                                              d, 0, d, d, d, d, d, None) == EINVAL
        assert lib.gsr_set_antialiasing(0) == 1
    finally:
        lib.gsr_set_antialiasing(0)


@pytest.mark.parametrize("env, want", [(None, False), ("0", False), ("1", True)])
def test_setting_follows_the_environment_in_a_fresh_process(env, want):
    e = {k: v for k, v in os.environ.items() if k != "GSR_ANTIALIASING"}
    if env is not None:
        e["GSR_ANTIALIASING"] = env
    code = ("import sys; sys.path.insert(0, %r); import diff_gaussian_rasterization as d; "
            "print(d.get_antialiasing()); d.set_antialiasing(not d.get_antialiasing()); print(d.get_antialiasing())"
            % os.path.join(ROOT, "grendel-gs_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(want), str(not want)]
