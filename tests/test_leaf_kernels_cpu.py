"""CPU side of the leaf-kernel edge tests (tests/test_gpu_loss_edges.py, test_gpu_adam_edges.py): the identity the HIP
loss backward relies on, and the proof that the element-wise tolerance K * max(fp32 self-error, floor) of
helpers.assert_elem_close still separates the reference from references with one deliberate mistake."""
import pytest
import torch

import leaf_refs as R
from helpers import assert_elem_close, elem_tolerance
from oracle.loss_oracle import ssim_grad_maps, ssim_map, window_1d

K = 8  # the margin the GPU files use (EXPERIMENTS.md, "leaf-kernel element-wise noise")


@pytest.mark.parametrize("H,W", [(33, 36), (11, 11)])
def test_backward_identity_of_the_three_maps(H, W):
    """w*M1 + 2x (w*M2) + y (w*M3) == autograd's d(sum ssim)/dx, in fp64 to 1e-10"""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(H * W)
    x = torch.rand(3, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    y = torch.randint(0, 256, (3, H, W), generator=g).double() / 255.0
    (want,) = torch.autograd.grad(ssim_map(x, y).sum(), x)
    ssim, M1, M2, M3 = ssim_grad_maps(x.detach(), y)
    assert torch.equal(ssim, ssim_map(x.detach(), y))
    w1 = window_1d().double()
    w2 = (w1[:, None] @ w1[None, :]).expand(3, 1, 11, 11).contiguous()
    cv = [F.conv2d(m.unsqueeze(0), w2, padding=5, groups=3).squeeze(0) for m in (M1, M2, M3)]
    got = cv[0] + 2 * x.detach() * cv[1] + y * cv[2]
    assert float((got - want).abs().max()) <= 1e-10


def test_parametrised_restatement_is_the_oracle_at_its_defaults():
    x, gt, _ = R.loss_inputs("noise", 3, 33, 36)
    a = ssim_grad_maps(x.double(), gt.double() / 255.0)
    b = R._terms(x.double(), gt.double() / 255.0, window_1d().double(), 0.03 ** 2)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_assert_elem_close_reports_ratio_and_fails_on_one_element():
    r64 = torch.linspace(-1, 1, 101, dtype=torch.float64)
    r32 = r64 + 1e-6
    unit = max(1e-6, 4 * 2.0 ** -24)
    got = r64.clone()
    got[17] += 3 * unit
    assert abs(assert_elem_close(got, r64, r32, K=8) - 3.0) < 1e-6
    got[17] += 6 * unit
    with pytest.raises(AssertionError, match=r"element \(17,\)"):
        assert_elem_close(got, r64, r32, K=8, what="x")
    got[17] = float("nan")
    with pytest.raises(AssertionError):
        assert_elem_close(got, r64, r32, K=8)
    # the floor: a reference that is exact in fp32 still allows 4 half-ulps of the largest value
    assert elem_tolerance(r64, r64, K=8) == 8 * 4 * 2.0 ** -24


_CASES = {"33x36": (3, 33, 36, 0, 33), "96x100_band27_70": (3, 96, 100, 27, 70)}
_CACHE = {}


def _loss_case(name):
    if name in _CACHE:
        return _CACHE[name]
    C, H, W, y0, y1 = _CASES[name]
    x, gt, ties = R.loss_inputs("noise", C, H, W)
    _CACHE[name] = dict(x=x, gt=gt, y0=y0, y1=y1, r64=R.loss_reference(x, gt, y0, y1, torch.float64),
                        r32=R.loss_reference(x, gt, y0, y1, torch.float32))
    return _CACHE[name]


def _worst_margin(wrong, r64, r32, names=("M1", "M2", "M3", "g0", "g1")):
    """max over the checked tensors of max|wrong - ref64| / tolerance"""
    def tensors(r):
        return dict(M1=r["M"][0], M2=r["M"][1], M3=r["M"][2], g0=r["grads"][0], g1=r["grads"][1])

    w, a, b = tensors(wrong), tensors(r64), tensors(r32)
    return max(float((w[n] - a[n]).abs().max()) / elem_tolerance(a[n], b[n], K) for n in names)


# ("pad" needs neighbouring rows: a band that is the whole image has none)
@pytest.mark.parametrize("case,wrong", [(c, w) for c in _CASES for w in ("tap", "pad", "y256", "c2")
                                        if not (w == "pad" and c == "33x36")])
def test_loss_tolerance_rejects_a_wrong_reference(case, wrong):
    c = _loss_case(case)
    bad = R.loss_reference(c["x"], c["gt"], c["y0"], c["y1"], torch.float64, wrong=wrong)
    margin = _worst_margin(bad, c["r64"], c["r32"])
    print(f"wrong={wrong}: worst |wrong - ref| / tolerance = {margin:.3g}")
    assert margin > 4.0
    # and the fp32 run of the right reference is inside the tolerance, by construction (ratio <= 1)
    for got, a, b in zip(c["r32"]["M"] + tuple(c["r32"]["grads"]), c["r64"]["M"] + tuple(c["r64"]["grads"]),
                         c["r32"]["M"] + tuple(c["r32"]["grads"])):
        assert assert_elem_close(got, a, b, K=K) <= 1.0


@pytest.mark.parametrize("C,H,W,y0,y1", [(3, 33, 36, 0, 33), (3, 96, 100, 27, 70)])
def test_loss_tolerance_rejects_sign_of_zero_plus_one(C, H, W, y0, y1):
    x, gt, ties = R.loss_inputs("ties", C, H, W)
    assert int(ties[:, y0:y1].sum()) > 0
    r64 = R.loss_reference(x, gt, y0, y1, torch.float64)
    r32 = R.loss_reference(x, gt, y0, y1, torch.float32)
    bad = R.loss_reference(x, gt, y0, y1, torch.float64, wrong="sign0")
    margin = _worst_margin(bad, r64, r32, names=("g0", "g1"))
    print(f"wrong=sign0: worst |wrong - ref| / tolerance = {margin:.3g}")
    assert margin > 4.0
    # torch.abs's backward is the rule: exactly zero L1 gradient at the ties
    from oracle.loss_oracle import l1_map

    xb = x[:, y0:y1].double().requires_grad_(True)
    (gl1,) = torch.autograd.grad(l1_map(xb, gt[:, y0:y1].double() / 255.0).sum(), xb)
    assert float(gl1[ties[:, y0:y1]].abs().max()) == 0.0 and float(gl1[~ties[:, y0:y1]].abs().min()) == 1.0


@pytest.mark.parametrize("family", R.FAMILIES)
def test_kernel_order_restatement_stays_inside_the_tolerance(family):
    """The kernel's order of operations restated in float32 (separable 11 + 11 taps, products before the taps, exact
    division) is inside K times the conv2d reference's fp32 self-error on every family: the order alone needs no larger
    margin.  (What v_rcp_f32 adds is measured on the GPU.)"""
    x, gt, _ = R.loss_inputs(family, 3, 33, 36)
    r64 = R.loss_reference(x, gt, 0, 33, torch.float64)
    r32 = R.loss_reference(x, gt, 0, 33, torch.float32)
    ko = R.loss_kernel_order_fp32(x, gt, 0, 33)
    for name, got, a, b in zip(("M1", "M2", "M3", "g0", "g1"), ko["M"] + tuple(ko["grads"]),
                               r64["M"] + tuple(r64["grads"]), r32["M"] + tuple(r32["grads"])):
        ratio = assert_elem_close(got, a, b, K=K, what=f"{family} {name}")
        print(f"{family} {name}: kernel-order fp32 ratio {ratio:.3g}")


@pytest.mark.parametrize("wrong", ["eps_before", "no_scale"])
def test_adam_tolerance_rejects_a_wrong_reference(wrong):
    n = 4097
    p, g, m, v = R.adam_inputs(n, seed=5)
    # eps large enough to matter next to sqrt(v) / sqrt(bc2) at step 1 (bc2 = 1e-3): the two placements differ by
    # eps * (1/sqrt(bc2) - 1) in the denominator
    hp = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-3, step=1, grad_scale=0.25)
    r64 = R.adam_reference(p, g, m, v, **hp)
    r32 = R.adam_torch32(p, g, m, v, **hp)
    bad = R.adam_reference(p, g, m, v, wrong=wrong, **hp)
    margin = max(float((w - a).abs().max()) / elem_tolerance(a, b, K) for w, a, b in zip(bad, r64, r32))
    print(f"wrong={wrong}: worst |wrong - ref| / tolerance = {margin:.3g}")
    assert margin > 4.0
    for got, a, b in zip(r32, r64, r32):
        assert assert_elem_close(got, a, b, K=K) <= 1.0
