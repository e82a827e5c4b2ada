"""CPU checks of the absolute-gradient references (tests/absgrad_refs.py), of the C ABI's refusals and of the switch.

On every case of tests/composite_refs.py:
* the closed form's SIGNED sums equal the float64 autograd d_means2D of composite_refs.references (up to the sign of the
  Definition) to 1e-11 of each row's largest value: this pins the per-pixel term the magnitudes are taken of;
* absgrad >= |signed| on every element, and rows that no pixel blends are exactly 0;
* the float32 closed form stays under helpers.ROW_UNIT_CAP;
* the CPU emulation of composite_absgrad_kernel's order of operations stays within HALF of K = K_GROUP["d_means2D"].
The two new symbols exist, refuse what include/gsraster.h says they refuse before any device work, return 0 for
P == 0 / n == 0, and gsr_abi_version() is still 15.  With gaussian_renderer.set_absgrad off, cuda_args carry no new key."""
import ctypes

import pytest
import torch

import absgrad_refs as AR
import composite_refs as R
from helpers import ROW_UNIT_CAP, rows_unit

U = 2.0 ** -24
CASES = R.cases()
IDS = [c.id for c in CASES]
GSR_EINVAL = -1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_signed_sums_equal_float64_autograd_and_magnitudes_dominate(case):
    r64, _ = R.references(case)
    cf = AR.closed_form(case, torch.float64)
    want = -r64["d_means2D"]
    assert cf["signed"].shape == want.shape == cf["absgrad"].shape == (case.P, 2)
    s = want.abs().amax(dim=1, keepdim=True) if case.P else want
    err = (cf["signed"] - want).abs()
    rel = float((err / s.clamp(min=1e-300)).max()) if case.P else 0.0
    print(f"ABSGRAD closed form {case.id}: signed sums off by {rel:.3g} of a row's largest value")
    assert bool((err <= 1e-11 * s).all()), f"{case.id}: {rel} > 1e-11"
    assert bool((cf["absgrad"] >= cf["signed"].abs()).all())
    nowhere = cf["hits"] == 0
    assert not bool(cf["absgrad"][nowhere].any()) and not bool(r64["d_means2D"][nowhere].any())
    listed = torch.zeros(case.P, dtype=torch.bool)
    for t in range(case.tiles):
        if bool(case.compute_locally[t]):
            listed[case.lists[t]] = True
    assert bool(nowhere[~listed].all()), "a row in no local list is blended somewhere"
    if case.family in ("lengths", "deep", "saturating", "clamp", "offtile", "edges") and case.P > 3:
        assert bool((cf["absgrad"][~nowhere] > 0).any())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_closed_form_is_under_the_row_unit_cap(case):
    c64, c32 = AR.closed_form(case, torch.float64), AR.closed_form(case, torch.float32)
    assert c32["absgrad"].dtype == torch.float32 and torch.equal(c32["hits"], c64["hits"])
    unit = rows_unit(c64["absgrad"], c32["absgrad"])
    print(f"ABSGRAD unit {case.id}: {unit / U:.0f} x 2^-24")
    assert unit <= ROW_UNIT_CAP


def _worst_ratio(got, ref64, ref32):
    unit = rows_unit(ref64, ref32)
    s = ref64.abs().amax(dim=1, keepdim=True)
    err = (got.double() - ref64).abs()
    assert not bool(err[(s == 0).expand_as(err)].any()), "a row of zeros in the reference is not zero"
    live = (s > 0).reshape(-1)
    return float((err[live] / (unit * s[live])).max()) if bool(live.any()) else 0.0


@pytest.mark.parametrize("case", [c for c in CASES if c.P > 0], ids=[c.id for c in CASES if c.P > 0])
def test_the_kernels_order_of_operations_stays_within_half_of_k(case):
    c64, c32 = AR.closed_form(case, torch.float64), AR.closed_form(case, torch.float32)
    em = AR.kernel_emulation(case)
    w = _worst_ratio(em, c64["absgrad"], c32["absgrad"])
    print(f"ABSGRAD emulation {case.id}: worst ratio {w:.3g} (K = {AR.K})")
    assert AR.K == R.K_GROUP["d_means2D"] and AR.K <= 16
    assert 2.0 * w <= AR.K, f"{case.id}: the formulation alone takes {w:.3g} of K = {AR.K}"


def test_abi_surface_refusals_and_empty_calls():
    from diff_gaussian_rasterization._lib import ABI_VERSION, SIGNATURES, lib

    assert lib.gsr_abi_version() == 15 == ABI_VERSION
    assert "gsr_render_absgrad" in SIGNATURES and "gsr_absgrad_merge_rows" in SIGNATURES
    buf = ctypes.create_string_buffer(64)   # a host address that is never dereferenced: every call below is refused
    p = ctypes.addressof(buf)               # (or is empty) before any device work
    ptrs = [p] * 10
    f = lib.gsr_render_absgrad
    assert f(-1, 16, 16, *ptrs, 0, 0, p, p, None) == GSR_EINVAL
    assert f(1, 0, 16, *ptrs, 0, 0, p, p, None) == GSR_EINVAL
    assert f(1, 16, -2, *ptrs, 0, 0, p, p, None) == GSR_EINVAL
    assert f(0, 16, 0, *ptrs, 0, 0, p, p, None) == GSR_EINVAL
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9):   # (point_list may be missing: every list can be empty)
        args = list(ptrs)
        args[i] = None
        assert f(1, 16, 16, *args, 0, 0, p, p, None) == GSR_EINVAL, f"argument {i}"
    assert f(1, 16, 16, *ptrs, 0, 0, None, p, None) == GSR_EINVAL
    assert f(1, 16, 16, *ptrs, 0, 0, p, None, None) == GSR_EINVAL
    assert f(0, 16, 16, *([None] * 10), 0, 0, None, None, None) == 0
    m = lib.gsr_absgrad_merge_rows
    assert m(-1, p, p, p, None) == GSR_EINVAL
    for i in range(3):
        args = [p, p, p]
        args[i] = None
        assert m(4, *args, None) == GSR_EINVAL
    assert m(0, None, None, None, None) == 0
    assert buf.raw == b"\0" * 64


def test_the_switch_is_off_by_default_and_adds_no_key_when_off():
    import gaussian_renderer as gr
    import utils.general_utils as utils

    utils.set_args(utils.default_args(bsz=1))
    utils.set_cur_iter(1)
    strategy = type("S", (), {"world_size": 1, "rank": 0})()
    was = gr.get_absgrad()
    try:
        gr.set_absgrad(False)
        off = gr.get_cuda_args_final(strategy, "train")
        assert "absgrad" not in off and not any("absgrad" in k for k in off)
        gr.set_absgrad(True)
        on = gr.get_cuda_args_final(strategy, "train")
        assert on["absgrad"] is True and {k: v for k, v in on.items() if k != "absgrad"} == off
    finally:
        gr.set_absgrad(was)
