"""-m gpu: gsr_render_invdepth, gsr_render_invdepth_backward and gsr_depth_backward_means3d through the C ABI on explicit
lists: every pixel of the map and every Gaussian row of the record against the float64 reference.

Per case of tests/composite_refs.py, extended by tests/invdepth_refs.py with depths and dL/dinvdepth: K8
(gsr_render_forward, as tests/test_gpu_composite_pixels.py calls it) gives the view's n_contrib and final_T, then the two
new entry points walk the same lists.  The map and the four gradient groups go through helpers.assert_rows_close against
float64 autograd through oracle.torch_oracle.render (rgb = (v, 0, 0), bg = 0): K = 8 for the map and d_depth,
composite_refs.K_GROUP for d_means2D, d_conic, d_opacity.  Outputs, and the fp64 scratch the call clears itself, are
pre-filled with NaN and nothing is excluded.  Pixels of tiles that are not ours are +0, rows blended nowhere are +0.0f.
Host-band and device-band launches give the whole-grid launch's map and record bit for bit, and so does a second run of
the backward.

Each figure (unit in 2^-24, worst ratio) is printed before it is asserted."""
import pytest
import torch

import composite_refs as R
import contrib_refs as CR
import invdepth_refs as IR
import test_gpu_composite_pixels as PX
from helpers import assert_rows_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
GSR_EINVAL = -1
CASES = R.cases()
IDS = [c.id for c in CASES]

_FWD, _DEP, _ROOT = {}, {}, {}


def _k8(case, device):
    """K8's (final_T, n_contrib) of the case (whole grid, no segments): computed once and never modified"""
    if case.id not in _FWD:
        fwd = PX._forward(PX._dev(case, device))
        assert fwd[0] == 0, f"gsr_render_forward returned {fwd[0]}"
        _FWD[case.id] = (fwd[2], fwd[3])
    return _FWD[case.id]


def _depths(case, device):
    if case.id not in _DEP:
        _DEP[case.id] = (IR.depths_of(case).to(device).contiguous(), IR.g_of(case).to(device).contiguous())
    return _DEP[case.id]


def _map(case, device, band=(0, 0)):
    """gsr_render_invdepth into a NaN-filled map -> (code, map [H,W] on the device)"""
    d = PX._dev(case, device)
    fT, nc = _k8(case, device)
    dep, _ = _depths(case, device)
    out = torch.full((case.H, case.W), NAN, dtype=torch.float32, device=device)
    code = PX._lib().gsr_render_invdepth(case.P, case.W, case.H, PX._p(d.ranges), PX._p(d.point_list), PX._p(d.means2D),
                                         PX._p(d.co), PX._p(dep), PX._p(d.mask), PX._p(nc), band[0], band[1],
                                         PX._p(out), PX._stream())
    torch.cuda.synchronize()
    return code, out


def _record(case, device, inv, band=(0, 0)):
    """gsr_render_invdepth_backward into a NaN-filled record and NaN-filled sums -> (code, record [max(P,1),7])"""
    d = PX._dev(case, device)
    fT, nc = _k8(case, device)
    dep, g = _depths(case, device)
    n = max(case.P, 1)
    rec = torch.full((n, 7), NAN, dtype=torch.float32, device=device)
    acc = torch.full((n, 7), NAN, dtype=torch.float64, device=device)
    code = PX._lib().gsr_render_invdepth_backward(case.P, case.W, case.H, PX._p(d.ranges), PX._p(d.point_list),
                                                  PX._p(d.means2D), PX._p(d.co), PX._p(dep), PX._p(d.mask), PX._p(nc),
                                                  PX._p(fT), PX._p(inv), PX._p(g), band[0], band[1], PX._p(rec),
                                                  PX._p(acc), PX._stream())
    torch.cuda.synchronize()
    return code, rec


def _root(case, device):
    """whole-grid map and record of one case: computed once per case and never modified"""
    if case.id not in _ROOT:
        code, inv = _map(case, device)
        assert code == 0, f"gsr_render_invdepth returned {code}"
        code, rec = _record(case, device, inv)
        assert code == 0, f"gsr_render_invdepth_backward returned {code}"
        _ROOT[case.id] = (inv, rec)
    return _ROOT[case.id]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_pixel_and_every_row_against_float64(device, case):
    inv, rec = _root(case, device)
    r64, r32 = IR.references(case)
    _, nc = _k8(case, device)
    assert torch.equal(nc.cpu(), r64["n_contrib"]), "K8's n_contrib is not the reference's: the comparison is void"
    inv_c = inv.cpu()
    for t in range(case.tiles):
        if not bool(case.compute_locally[t]):
            x0, y0, x1, y1 = case.tile_box(t)
            assert not bool(_bits(inv_c[y0:y1, x0:x1]).any()), f"{case.id}: map of tile {t} (not ours) is not +0"
    fig = dict(invdepth=assert_rows_close(inv_c.reshape(-1, 1), r64["invdepth"], r32["invdepth"], IR.K_MAP,
                                          f"{case.id} invdepth"))
    if case.P == 0:  # the all-zero map; the backward succeeds and writes not one word
        assert not bool(_bits(inv_c).any()) and bool(torch.isnan(rec).all())
    else:
        got = IR.split_record(rec.cpu()[:case.P])
        for k in IR.GROUPS:
            fig[k] = assert_rows_close(got[k], r64[k], r32[k], IR.K_GROUP[k], f"{case.id} {k}")
        nowhere = CR.references(case)[0]["hits"] == 0
        assert not bool(_bits(rec.cpu()[:case.P][nowhere]).any()), "a row that is blended nowhere is not +0.0f"
    for k, (unit, worst) in fig.items():
        print(f"INVDEPTH {case.id} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")


VARIANTS = [c for c in CASES if c.family in R.VARIANT_FAMILIES and c.P > 0]
assert any(c.band is not None for c in VARIANTS), "no case with a proper row band"


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
@pytest.mark.parametrize("kind", ["host", "device", "device-larger"])
def test_row_bands_are_bit_equal_to_the_whole_grid(device, case, kind):
    """the launch covers the band's tiles only (host rows; or row_lo = -1 with a capacity, the band read from the hull
    behind the range table).  A case whose local tiles span every tile row has the whole grid as its band."""
    inv0, rec0 = _root(case, device)
    lo, hi = case.band if case.band is not None else case.hull
    assert (lo, hi) == case.hull and hi > lo
    band = (lo, hi) if kind == "host" else (-1, hi - lo if kind == "device" else case.gy)
    code, inv = _map(case, device, band=band)
    assert code == 0 and torch.equal(_bits(inv), _bits(inv0)), f"{case.id} band {kind}: the map differs"
    code, rec = _record(case, device, inv, band=band)
    assert code == 0 and torch.equal(_bits(rec), _bits(rec0)), f"{case.id} band {kind}: the record differs"
    # (inert-P1 blends nothing by construction; everywhere else an empty map would make the comparison empty)
    assert bool(inv0.any()) == bool(IR.references(case)[0]["invdepth"].any()) == (case.id != "inert-P1")


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
def test_two_runs_of_the_backward_are_bit_equal(device, case):
    inv0, rec0 = _root(case, device)
    code, rec = _record(case, device, inv0)
    assert code == 0 and torch.equal(_bits(rec), _bits(rec0))


def test_p1_and_the_refused_calls(device):
    lib = PX._lib()
    case = next(c for c in CASES if c.id == "inert-P1")
    inv, rec = _root(case, device)  # one listed row, blended nowhere: a zero map and a zero row
    assert not bool(_bits(inv).any()) and not bool(_bits(rec).any())
    d = PX._dev(case, device)
    fT, nc = _k8(case, device)
    dep, g = _depths(case, device)
    out = torch.full((case.H, case.W), NAN, dtype=torch.float32, device=device)
    rec = torch.full((1, 7), NAN, dtype=torch.float32, device=device)
    acc = torch.full((1, 7), NAN, dtype=torch.float64, device=device)
    p = PX._p
    fwd = [p(d.ranges), p(d.point_list), p(d.means2D), p(d.co), p(dep), p(d.mask), p(nc)]
    bwd = fwd + [p(fT), p(inv), p(g)]
    st = PX._stream()
    assert lib.gsr_render_invdepth(-1, 16, 16, *fwd, 0, 0, p(out), st) == GSR_EINVAL
    assert lib.gsr_render_invdepth(1, 0, 16, *fwd, 0, 0, p(out), st) == GSR_EINVAL
    assert lib.gsr_render_invdepth(1, 16, -3, *fwd, 0, 0, p(out), st) == GSR_EINVAL
    assert lib.gsr_render_invdepth(1, 16, 16, *fwd, 0, 0, None, st) == GSR_EINVAL
    for i in (0, 2, 3, 4, 5, 6):  # (point_list may be missing: every list can be empty)
        args = list(fwd)
        args[i] = None
        assert lib.gsr_render_invdepth(1, 16, 16, *args, 0, 0, p(out), st) == GSR_EINVAL, f"forward argument {i}"
    assert lib.gsr_render_invdepth_backward(-1, 16, 16, *bwd, 0, 0, p(rec), p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_invdepth_backward(1, 16, 0, *bwd, 0, 0, p(rec), p(acc), st) == GSR_EINVAL
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9):
        args = list(bwd)
        args[i] = None
        assert lib.gsr_render_invdepth_backward(1, 16, 16, *args, 0, 0, p(rec), p(acc), st) == GSR_EINVAL, f"backward argument {i}"
    assert lib.gsr_render_invdepth_backward(1, 16, 16, *bwd, 0, 0, None, p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_invdepth_backward(1, 16, 16, *bwd, 0, 0, p(rec), None, st) == GSR_EINVAL
    assert lib.gsr_depth_backward_means3d(-1, p(nc), p(fT), p(fT), 1, p(out), 0, st) == GSR_EINVAL
    assert lib.gsr_depth_backward_means3d(4, p(nc), p(fT), p(fT), 0, p(out), 0, st) == GSR_EINVAL
    assert lib.gsr_depth_backward_means3d(4, None, p(fT), p(fT), 1, p(out), 0, st) == GSR_EINVAL
    assert lib.gsr_depth_backward_means3d(0, None, None, None, 1, None, 0, st) == 0
    torch.cuda.synchronize()
    # every refusal came before any device work
    assert bool(torch.isnan(out).all() & torch.isnan(rec).all()) and bool(torch.isnan(acc).all())


@pytest.mark.parametrize("stride", [1, 7])
@pytest.mark.parametrize("overwrite", [0, 1])
def test_depth_backward_means3D_every_row(device, stride, overwrite):
    """P = 1000 is four workgroups (the last one partly filled); radii 0 and negative rows are skipped"""
    gen = torch.Generator().manual_seed(17 + stride)
    P = 1000
    view = torch.randn(4, 4, generator=gen)
    radii = torch.randint(-1, 4, (P,), generator=gen).to(torch.int32)
    src = torch.randn(P, stride, generator=gen)
    col = stride - 1  # (stride 7: column 6 of a [P,7] record)
    base = torch.randn(P, 3, generator=gen)
    out = base.clone().to(device)
    src_d, view_d, radii_d = src.to(device), view.to(device), radii.to(device)
    code = PX._lib().gsr_depth_backward_means3d(P, PX._p(radii_d), PX._p(view_d), src_d.data_ptr() + 4 * col, stride,
                                                PX._p(out), overwrite, PX._stream())
    torch.cuda.synchronize()
    assert code == 0
    want64 = IR.depth_to_means3D(src[:, col].double(), radii, view.double())
    want32 = IR.depth_to_means3D(src[:, col], radii, view)
    if not overwrite:
        want64, want32 = base.double() + want64, base + want32
    unit, worst = assert_rows_close(out.cpu(), want64, want32, 8, f"stride {stride} overwrite {overwrite}")
    print(f"INVDEPTH means3D stride {stride} overwrite {overwrite}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")
    skipped = radii <= 0
    assert bool(skipped.any())
    if overwrite:
        assert not bool(_bits(out.cpu()[skipped]).any()), "a skipped row is not +0.0f"
    else:
        assert torch.equal(_bits(out.cpu()[skipped]), _bits(base[skipped])), "a skipped row was written"
