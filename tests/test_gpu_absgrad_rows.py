"""-m gpu: gsr_render_absgrad and gsr_absgrad_merge_rows through the C ABI on explicit lists: every Gaussian row against
the float64 closed form.

Per case of tests/composite_refs.py: K8 (gsr_render_forward, as tests/test_gpu_composite_pixels.py calls it) gives the
view's n_contrib and final_T, then the new entry point walks the same lists with the case's dL/dpixels.  The [P,2] result
goes through helpers.assert_rows_close against tests/absgrad_refs.closed_form in float64, its float32 run the unit,
K = composite_refs.K_GROUP["d_means2D"], nothing excluded.  The result, and the fp64 scratch the call clears itself, are
pre-filled with NaN.  Rows blended nowhere are +0.0f.  Host-band and device-band launches give the whole-grid launch's
bits, and so does a second launch into the same buffers.  The merge entry is compared with index_add_.

Each figure (unit in 2^-24, worst ratio) is printed before it is asserted."""
import pytest
import torch

import absgrad_refs as AR
import composite_refs as R
import test_gpu_composite_pixels as PX
from helpers import assert_rows_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
GSR_EINVAL = -1
CASES = R.cases()
IDS = [c.id for c in CASES]
assert {c.family for c in CASES} == set(R.FAMILIES)

_FWD, _ROOT = {}, {}


def _k8(case, device):
    """K8's (final_T, n_contrib) of the case (whole grid, no segments): computed once and never modified"""
    if case.id not in _FWD:
        fwd = PX._forward(PX._dev(case, device))
        assert fwd[0] == 0, f"gsr_render_forward returned {fwd[0]}"
        _FWD[case.id] = (fwd[2], fwd[3])
    return _FWD[case.id]


def _launch(case, device, band=(0, 0), into=None):
    """gsr_render_absgrad into NaN-filled buffers (or `into`) -> (code, absgrad [max(P,1),2], acc64)"""
    d = PX._dev(case, device)
    fT, nc = _k8(case, device)
    n = max(case.P, 1)
    if into is None:
        into = (torch.full((n, 2), NAN, dtype=torch.float32, device=device),
                torch.full((n, 2), NAN, dtype=torch.float64, device=device))
    out, acc = into
    p = PX._p
    code = PX._lib().gsr_render_absgrad(case.P, case.W, case.H, p(d.ranges), p(d.point_list), p(d.means2D), p(d.co),
                                        p(d.rgb), p(d.mask), p(d.bg), p(fT), p(nc), p(d.g), band[0], band[1], p(out),
                                        p(acc), PX._stream())
    torch.cuda.synchronize()
    return code, out, acc


def _root(case, device):
    if case.id not in _ROOT:
        code, out, acc = _launch(case, device)
        assert code == 0, f"gsr_render_absgrad returned {code}"
        _ROOT[case.id] = (out, acc)
    return _ROOT[case.id]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_row_against_the_float64_closed_form(device, case):
    out, _ = _root(case, device)
    _, nc = _k8(case, device)
    assert torch.equal(nc.cpu(), R.references(case)[0]["n_contrib"]), "K8's n_contrib is not the reference's"
    if case.P == 0:  # the call succeeds and writes not one word
        assert bool(torch.isnan(out).all())
        return
    c64, c32 = AR.closed_form(case, torch.float64), AR.closed_form(case, torch.float32)
    got = out.cpu()[:case.P]
    unit, worst = assert_rows_close(got, c64["absgrad"], c32["absgrad"], AR.K, f"{case.id} absgrad")
    print(f"ABSGRAD {case.id}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")
    nowhere = c64["hits"] == 0
    assert not bool(_bits(got[nowhere]).any()), "a row that is blended nowhere is not +0.0f"
    assert bool((got >= 0).all())
    # the magnitudes dominate K10's signed sums (the float64 ones, with room for the kernel's K units)
    signed = R.references(case)[0]["d_means2D"].abs()
    slack = AR.K * unit * c64["absgrad"].amax(dim=1, keepdim=True)
    assert bool((got.double() + slack >= signed).all())


VARIANTS = [c for c in CASES if c.family in R.VARIANT_FAMILIES and c.P > 0]
assert any(c.band is not None for c in VARIANTS), "no case with a proper row band"


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
@pytest.mark.parametrize("kind", ["host", "device", "device-larger"])
def test_row_bands_are_bit_equal_to_the_whole_grid(device, case, kind):
    out0, _ = _root(case, device)
    lo, hi = case.band if case.band is not None else case.hull
    assert (lo, hi) == case.hull and hi > lo
    band = (lo, hi) if kind == "host" else (-1, hi - lo if kind == "device" else case.gy)
    code, out, _ = _launch(case, device, band=band)
    assert code == 0 and torch.equal(_bits(out), _bits(out0)), f"{case.id} band {kind}: the rows differ"
    assert bool(out0.any()) == (case.id != "inert-P1")


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
def test_a_second_launch_into_the_same_buffers_gives_the_same_bits(device, case):
    out0, _ = _root(case, device)
    code, out, acc = _launch(case, device)
    assert code == 0
    first = out.clone()
    code, out, acc = _launch(case, device, into=(out, acc))  # (the sums of the first launch are still in `acc`)
    assert code == 0 and torch.equal(_bits(out), _bits(first)) and torch.equal(_bits(out), _bits(out0))


def test_p1_and_the_refused_calls(device):
    lib = PX._lib()
    case = next(c for c in CASES if c.id == "inert-P1")
    out, _ = _root(case, device)  # one listed row, blended nowhere: a zero row
    assert not bool(_bits(out).any())
    d = PX._dev(case, device)
    fT, nc = _k8(case, device)
    p = PX._p
    out = torch.full((1, 2), NAN, dtype=torch.float32, device=device)
    acc = torch.full((1, 2), NAN, dtype=torch.float64, device=device)
    args = [p(d.ranges), p(d.point_list), p(d.means2D), p(d.co), p(d.rgb), p(d.mask), p(d.bg), p(fT), p(nc), p(d.g)]
    st = PX._stream()
    assert lib.gsr_render_absgrad(-1, 16, 16, *args, 0, 0, p(out), p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_absgrad(1, 0, 16, *args, 0, 0, p(out), p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_absgrad(1, 16, -3, *args, 0, 0, p(out), p(acc), st) == GSR_EINVAL
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9):  # (point_list may be missing: every list can be empty)
        a = list(args)
        a[i] = None
        assert lib.gsr_render_absgrad(1, 16, 16, *a, 0, 0, p(out), p(acc), st) == GSR_EINVAL, f"argument {i}"
    assert lib.gsr_render_absgrad(1, 16, 16, *args, 0, 0, None, p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_absgrad(1, 16, 16, *args, 0, 0, p(out), None, st) == GSR_EINVAL
    assert lib.gsr_render_absgrad(0, 16, 16, *args, 0, 0, p(out), p(acc), st) == 0
    torch.cuda.synchronize()
    # every refusal came before any device work, and P == 0 touched nothing
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(acc).all())


def test_merge_rows_against_index_add(device):
    """n = 3000 rows (24 workgroups' worth of elements, the last one partly filled) into P = 700: duplicates add, rows
    with a negative index are skipped; the sums are of non-negative values, compared in float64 with K = 8"""
    import diff_gaussian_rasterization as dgr

    gen = torch.Generator().manual_seed(23)
    n, P = 3000, 700
    idx = torch.randint(-2, P, (n,), generator=gen).to(torch.int32)
    idx[:5] = 17  # a heavily duplicated row
    src = torch.rand(n, 2, generator=gen)
    src[::7] = 0.0
    base = torch.rand(P, 2, generator=gen)
    keep = idx >= 0
    assert bool((~keep).any()) and int(keep.sum()) > P
    want64 = base.double().index_add(0, idx[keep].long(), src[keep].double())
    want32 = base.index_add(0, idx[keep].long(), src[keep])
    got = dgr.absgrad_rows(idx.to(device), src.to(device), P, dst=base.clone().to(device))
    unit, worst = assert_rows_close(got.cpu(), want64, want32, 8, "merge into a filled tensor")
    print(f"ABSGRAD merge: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")
    fresh = dgr.absgrad_rows(idx.to(device), src.to(device), P)
    z64 = torch.zeros(P, 2, dtype=torch.float64).index_add(0, idx[keep].long(), src[keep].double())
    z32 = torch.zeros(P, 2).index_add(0, idx[keep].long(), src[keep])
    assert_rows_close(fresh.cpu(), z64, z32, 8, "merge into zeros")
    untouched = torch.ones(P, dtype=torch.bool)
    untouched[idx[keep].long()] = False
    assert not bool(_bits(fresh.cpu()[untouched]).any())
    lib, p = PX._lib(), PX._p
    a, b, c = idx.to(device), src.to(device), base.clone().to(device)
    assert lib.gsr_absgrad_merge_rows(-1, p(a), p(b), p(c), PX._stream()) == GSR_EINVAL
    assert lib.gsr_absgrad_merge_rows(4, None, p(b), p(c), PX._stream()) == GSR_EINVAL
    assert lib.gsr_absgrad_merge_rows(0, None, None, None, PX._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(c.cpu(), base)
