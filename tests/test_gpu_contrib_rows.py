"""-m gpu: gsr_render_contrib through the C ABI on explicit lists: every Gaussian row against the float64 reference.

Per case of tests/composite_refs.py: K8 (gsr_render_forward, as tests/test_gpu_composite_pixels.py calls it) gives the
view's n_contrib, then gsr_render_contrib walks the same lists.  From zeroed accumulators `hits` equals the float64
reference of tests/contrib_refs.py on every row, and wmax / wsum go through helpers.assert_rows_close with K = 8 (the
project's value: the kernel forms alpha and T as K8 does, whose image holds K = 8 on these cases).  Into PRE-FILLED
accumulators (hits 7, wmax 0.5, wsum 3.25, 16 guard rows behind P) the kernel accumulates: hits = 7 + reference, wmax =
max(0.5, .), wsum - 3.25 by the same rule, and every row nobody blended -- and every guard row -- keeps its bits.  Two
launches into one accumulator double hits exactly, leave wmax bit-equal and double wsum within the rounding of a row's
fp64 additions (contrib_refs.fp64_add_bound).  The banded cases launched with the host band, the device hull at
capacity = hull and at capacity = grid rows give the whole-grid launch's hits and wmax bit for bit.

Each figure (unit in 2^-24, worst ratio) is printed before it is asserted."""
import pytest
import torch

import composite_refs as R
import contrib_refs as CR
import test_gpu_composite_pixels as PX
from helpers import assert_rows_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K = 8
GUARD = 16
FILL = (7, 0.5, 3.25)
CASES = R.cases()
IDS = [c.id for c in CASES]


def _acc(case, device, fill=(0, 0.0, 0.0)):
    n = case.P + GUARD
    return (torch.full((n,), fill[0], dtype=torch.int64, device=device),
            torch.full((n,), fill[1], dtype=torch.float32, device=device),
            torch.full((n,), fill[2], dtype=torch.float64, device=device))


_NC = {}


def _n_contrib(case, device):
    """K8's n_contrib of the case (whole grid, no segments): computed once and never modified"""
    if case.id not in _NC:
        fwd = PX._forward(PX._dev(case, device))
        assert fwd[0] == 0, f"gsr_render_forward returned {fwd[0]}"
        _NC[case.id] = fwd[3]
    return _NC[case.id]


def _contrib(case, device, acc, band=(0, 0)):
    d = PX._dev(case, device)
    nc = _n_contrib(case, device)
    hits, wmax, wsum = acc
    code = PX._lib().gsr_render_contrib(case.P, case.W, case.H, PX._p(d.ranges), PX._p(d.point_list), PX._p(d.means2D),
                                        PX._p(d.co), PX._p(d.mask), PX._p(nc), band[0], band[1], PX._p(hits), PX._p(wmax),
                                        PX._p(wsum), PX._stream())
    torch.cuda.synchronize()
    assert code == 0, f"gsr_render_contrib returned {code}"
    return tuple(t.cpu() for t in acc)


_ZERO = {}


def _from_zero(case, device):
    """one launch over the whole grid into zeroed accumulators: computed once per case and never modified"""
    if case.id not in _ZERO:
        _ZERO[case.id] = _contrib(case, device, _acc(case, device))
    return _ZERO[case.id]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _check_rows(case, wmax, wsum, what):
    r64, r32 = CR.references(case)
    fig = dict(wmax=assert_rows_close(wmax[:case.P].reshape(-1, 1), r64["wmax"], r32["wmax"], K, f"{what} wmax"),
               wsum=assert_rows_close(wsum[:case.P].reshape(-1, 1), r64["wsum"], r32["wsum"], K, f"{what} wsum"))
    for k, (unit, worst) in fig.items():
        print(f"CONTRIB {what} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")
    return fig


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_from_zero_against_float64(device, case):
    if case.P == 0:  # success, and not one word written
        hits, wmax, wsum = _contrib(case, device, _acc(case, device, FILL))
        assert bool((hits == FILL[0]).all() & (wmax == FILL[1]).all() & (wsum == FILL[2]).all())
        return
    hits, wmax, wsum = _from_zero(case, device)
    r64, _ = CR.references(case)
    P = case.P
    assert torch.equal(hits[:P], r64["hits"]), \
        f"{case.id}: hits differ on rows {torch.nonzero(hits[:P] != r64['hits']).reshape(-1)[:8].tolist()}"
    _check_rows(case, wmax, wsum, case.id)
    assert not bool(hits[P:].any() | _bits(wmax[P:]).any() | _bits(wsum[P:]).any()), "a guard row was written"
    assert float(wmax.max()) <= float(torch.tensor(0.99, dtype=torch.float32))  # the clamp, as the kernel's float holds it


@pytest.mark.parametrize("case", [c for c in CASES if c.P > 0], ids=[c.id for c in CASES if c.P > 0])
def test_accumulates_into_prefilled_rows(device, case):
    P = case.P
    z_hits, z_wmax, z_wsum = _from_zero(case, device)
    hits, wmax, wsum = _contrib(case, device, _acc(case, device, FILL))
    r64, _ = CR.references(case)
    assert torch.equal(hits[:P], FILL[0] + r64["hits"])
    want = torch.maximum(torch.full_like(z_wmax, FILL[1]), z_wmax)
    assert torch.equal(_bits(wmax), _bits(want)), "wmax is not max(0.5, the launch's own maximum)"
    _check_rows(case, z_wmax, wsum - FILL[2], f"{case.id} prefilled")
    # rows nobody blended, and the guard rows, keep their bits
    still = torch.cat([r64["hits"] == 0, torch.ones(GUARD, dtype=torch.bool)])
    ref = tuple(t.cpu() for t in _acc(case, "cpu", FILL))
    for got, fill, name in zip((hits, wmax, wsum), ref, ("hits", "wmax", "wsum")):
        assert torch.equal(_bits(got[still]), _bits(fill[still])), \
            f"{name}: a row that blends nowhere (or a guard row) was written"


@pytest.mark.parametrize("case", [c for c in CASES if c.P > 0], ids=[c.id for c in CASES if c.P > 0])
def test_two_launches_into_one_accumulator(device, case):
    z_hits, z_wmax, z_wsum = _from_zero(case, device)
    acc = _acc(case, device)
    _contrib(case, device, acc)
    hits, wmax, wsum = _contrib(case, device, acc)
    assert torch.equal(hits, 2 * z_hits)
    assert torch.equal(_bits(wmax), _bits(z_wmax))
    err = (wsum - 2.0 * z_wsum).abs()
    bound = CR.fp64_add_bound(case) * (2.0 * z_wsum).abs()
    print(f"CONTRIB {case.id} twice: worst |wsum - 2 x once| / (2 x once) = "
          f"{float((err / (2.0 * z_wsum).clamp(min=1e-300)).max()):.3g}, bound {CR.fp64_add_bound(case):.3g}")
    assert bool((err <= bound).all()), f"rows {torch.nonzero(err > bound).reshape(-1)[:8].tolist()}"


BANDED = [c for c in CASES if c.band is not None]
assert BANDED, "no case with a proper row band"


@pytest.mark.parametrize("case", BANDED, ids=[c.id for c in BANDED])
@pytest.mark.parametrize("kind", ["host", "device", "device-larger"])
def test_row_bands(device, case, kind):
    z_hits, z_wmax, z_wsum = _from_zero(case, device)
    lo, hi = case.band
    assert (lo, hi) == case.hull and 0 < hi - lo < case.gy
    band = (lo, hi) if kind == "host" else (-1, hi - lo if kind == "device" else case.gy)
    hits, wmax, wsum = _contrib(case, device, _acc(case, device), band=band)
    assert torch.equal(hits, z_hits) and torch.equal(_bits(wmax), _bits(z_wmax))
    err = (wsum - z_wsum).abs()
    assert bool((err <= CR.fp64_add_bound(case) * z_wsum.abs()).all())
    assert bool(z_hits.any()), "the band blends nothing: the comparison is empty"
