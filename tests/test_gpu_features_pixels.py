"""-m gpu: gsr_render_features and gsr_render_features_backward through the C ABI on explicit lists: every pixel of every
channel of the map and every Gaussian row of both records against the float64 reference.

Per case of tests/composite_refs.py, extended by tests/features_refs.py with features [P,C] and dL/dout [C,H,W]: K8
(gsr_render_forward, as tests/test_gpu_composite_pixels.py calls it) gives the view's n_contrib and final_T, then the two
new entry points walk the same lists.  The map and the four gradient groups go through helpers.assert_rows_close against
float64 autograd through oracle.torch_oracle.render (three channels at a time, bg = 0): K = 8 for the map and d_features,
features_refs.K_GROUP for d_means2D, d_conic, d_opacity.  Outputs, and the fp64 scratch the call clears itself, are
pre-filled with NaN and nothing is excluded.  Pixels of tiles that are not ours are +0, rows blended nowhere are +0.0f.

Every case at C = 4; the channel sweep C in {1, 2, CH - 1, CH, CH + 1, 2 CH + 3} on the `edges` family and one `lengths`
case (a chunk boundary, a partial last chunk, a partial image tile).  Channel c of a C-channel forward is the one-channel
forward of column c bit for bit; host-band and device-band launches give the whole-grid launch's bits, and so does a
second run of the backward; without dL_dfeatures the [P,6] record keeps its bits and the feature buffer is not touched;
an all-ones column gives 1 - final_T.

Each figure (unit in 2^-24, worst ratio) is printed before it is asserted."""
import pytest
import torch

import composite_refs as R
import contrib_refs as CR
import features_refs as FR
import test_gpu_composite_pixels as PX
from helpers import assert_rows_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
GSR_EINVAL = -1
CASES = R.cases()
IDS = [c.id for c in CASES]
SWEEP_CASES = [c for c in CASES if c.family == "edges"] + [c for c in CASES if c.id == "lengths-65"]
SWEEP = [(c, C) for c in SWEEP_CASES for C in FR.SWEEP]

_FWD, _IN, _ROOT = {}, {}, {}


def _k8(case, device):
    """K8's (final_T, n_contrib) of the case (whole grid, no segments): computed once and never modified"""
    if case.id not in _FWD:
        fwd = PX._forward(PX._dev(case, device))
        assert fwd[0] == 0, f"gsr_render_forward returned {fwd[0]}"
        _FWD[case.id] = (fwd[2], fwd[3])
    return _FWD[case.id]


def _inputs(case, C, device):
    if (case.id, C) not in _IN:
        _IN[case.id, C] = (FR.features_of(case, C).to(device).contiguous(), FR.g_of(case, C).to(device).contiguous())
    return _IN[case.id, C]


def _map(case, device, feat, band=(0, 0)):
    """gsr_render_features of `feat` [P,C] into a NaN-filled map -> (code, map [C,H,W] on the device)"""
    d = PX._dev(case, device)
    fT, nc = _k8(case, device)
    C = feat.shape[1]
    out = torch.full((C, case.H, case.W), NAN, dtype=torch.float32, device=device)
    code = PX._lib().gsr_render_features(case.P, C, case.W, case.H, PX._p(d.ranges), PX._p(d.point_list),
                                         PX._p(d.means2D), PX._p(d.co), PX._p(feat), PX._p(d.mask), PX._p(nc), band[0],
                                         band[1], PX._p(out), PX._stream())
    torch.cuda.synchronize()
    return code, out


def _records(case, device, feat, g, band=(0, 0), feature_grad=True):
    """gsr_render_features_backward into NaN-filled records and NaN-filled sums -> (code, record [max(P,1),6],
    dL_dfeatures [max(P,1),C]); feature_grad False: NULL is passed and the NaN-filled buffer comes back as it was"""
    d = PX._dev(case, device)
    fT, nc = _k8(case, device)
    C = feat.shape[1]
    n = max(case.P, 1)
    rec = torch.full((n, 6), NAN, dtype=torch.float32, device=device)
    dfe = torch.full((n, C), NAN, dtype=torch.float32, device=device)
    acc = torch.full((n, 6 + C if feature_grad else 6), NAN, dtype=torch.float64, device=device)
    code = PX._lib().gsr_render_features_backward(case.P, C, case.W, case.H, PX._p(d.ranges), PX._p(d.point_list),
                                                  PX._p(d.means2D), PX._p(d.co), PX._p(feat), PX._p(d.mask), PX._p(nc),
                                                  PX._p(fT), PX._p(g), band[0], band[1], PX._p(rec),
                                                  PX._p(dfe) if feature_grad else None, PX._p(acc), PX._stream())
    torch.cuda.synchronize()
    return code, rec, dfe


def _root(case, C, device):
    """whole-grid map and records of one (case, C): computed once and never modified"""
    if (case.id, C) not in _ROOT:
        feat, g = _inputs(case, C, device)
        code, out = _map(case, device, feat)
        assert code == 0, f"gsr_render_features returned {code}"
        code, rec, dfe = _records(case, device, feat, g)
        assert code == 0, f"gsr_render_features_backward returned {code}"
        _ROOT[case.id, C] = (out, rec, dfe)
    return _ROOT[case.id, C]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _against_float64(device, case, C):
    out, rec, dfe = _root(case, C, device)
    r64, r32 = FR.references(case, C)
    _, nc = _k8(case, device)
    assert torch.equal(nc.cpu(), r64["n_contrib"]), "K8's n_contrib is not the reference's: the comparison is void"
    out_c = out.cpu()
    for t in range(case.tiles):
        if not bool(case.compute_locally[t]):
            x0, y0, x1, y1 = case.tile_box(t)
            assert not bool(_bits(out_c[:, y0:y1, x0:x1]).any()), f"{case.id}: map of tile {t} (not ours) is not +0"
    fig = dict(map=assert_rows_close(FR.map_rows(out_c), r64["map"], r32["map"], FR.K_MAP, f"{case.id} C={C} map"))
    if case.P == 0:  # the all-zero map; the backward succeeds and writes not one word
        assert not bool(_bits(out_c).any()) and bool(torch.isnan(rec).all()) and bool(torch.isnan(dfe).all())
    else:
        got = FR.split_records(rec.cpu()[:case.P], dfe.cpu()[:case.P])
        for k in FR.GROUPS:
            fig[k] = assert_rows_close(got[k], r64[k], r32[k], FR.K_GROUP[k], f"{case.id} C={C} {k}")
        nowhere = CR.references(case)[0]["hits"] == 0
        assert not bool(_bits(rec.cpu()[:case.P][nowhere]).any()), "a row that is blended nowhere is not +0.0f"
        assert not bool(_bits(dfe.cpu()[:case.P][nowhere]).any()), "a feature row that is blended nowhere is not +0.0f"
    for k, (unit, worst) in fig.items():
        print(f"FEATURES {case.id} C={C} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_pixel_and_every_row_against_float64(device, case):
    _against_float64(device, case, 4)


@pytest.mark.parametrize("case,C", SWEEP, ids=[f"{c.id}-C{C}" for c, C in SWEEP])
def test_channel_sweep_against_float64(device, case, C):
    _against_float64(device, case, C)


@pytest.mark.parametrize("case,C", [(c, C) for c in SWEEP_CASES[-3:] for C in (4, FR.CH + 1, 2 * FR.CH + 3)],
                         ids=[f"{c.id}-C{C}" for c in SWEEP_CASES[-3:] for C in (4, FR.CH + 1, 2 * FR.CH + 3)])
def test_a_channel_is_its_one_channel_forward_bit_for_bit(device, case, C):
    out, _, _ = _root(case, C, device)
    feat, _ = _inputs(case, C, device)
    for c in sorted({0, 3, C // 2, C - 1}):
        code, one = _map(case, device, feat[:, c:c + 1].contiguous())
        assert code == 0 and torch.equal(_bits(one[0]), _bits(out[c])), f"{case.id}: channel {c} of {C} differs"
    assert bool(out.any())


VARIANTS = [c for c in CASES if c.family in R.VARIANT_FAMILIES and c.P > 0]
assert any(c.band is not None for c in VARIANTS), "no case with a proper row band"


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
@pytest.mark.parametrize("kind", ["host", "device", "device-larger"])
def test_row_bands_are_bit_equal_to_the_whole_grid(device, case, kind):
    """the launch covers the band's tiles only (host rows; or row_lo = -1 with a capacity, the band read from the hull
    behind the range table).  A case whose local tiles span every tile row has the whole grid as its band."""
    C = 4
    out0, rec0, dfe0 = _root(case, C, device)
    feat, g = _inputs(case, C, device)
    lo, hi = case.band if case.band is not None else case.hull
    assert (lo, hi) == case.hull and hi > lo
    band = (lo, hi) if kind == "host" else (-1, hi - lo if kind == "device" else case.gy)
    code, out = _map(case, device, feat, band=band)
    assert code == 0 and torch.equal(_bits(out), _bits(out0)), f"{case.id} band {kind}: the map differs"
    code, rec, dfe = _records(case, device, feat, g, band=band)
    assert code == 0 and torch.equal(_bits(rec), _bits(rec0)), f"{case.id} band {kind}: the record differs"
    assert torch.equal(_bits(dfe), _bits(dfe0)), f"{case.id} band {kind}: the feature gradient differs"
    # (inert-P1 blends nothing by construction; everywhere else an empty map would make the comparison empty)
    assert bool(out0.any()) == bool(FR.references(case, C)[0]["map"].any()) == (case.id != "inert-P1")


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
def test_two_runs_of_the_backward_are_bit_equal(device, case):
    out0, rec0, dfe0 = _root(case, 4, device)
    feat, g = _inputs(case, 4, device)
    code, rec, dfe = _records(case, device, feat, g)
    assert code == 0 and torch.equal(_bits(rec), _bits(rec0)) and torch.equal(_bits(dfe), _bits(dfe0))


@pytest.mark.parametrize("case,C", [(c, C) for c in SWEEP_CASES[-3:] for C in (4, FR.CH + 1)],
                         ids=[f"{c.id}-C{C}" for c in SWEEP_CASES[-3:] for C in (4, FR.CH + 1)])
def test_without_the_feature_gradient_the_record_keeps_its_bits(device, case, C):
    _, rec0, _ = _root(case, C, device)
    feat, g = _inputs(case, C, device)
    code, rec, dfe = _records(case, device, feat, g, feature_grad=False)
    assert code == 0 and torch.equal(_bits(rec), _bits(rec0)), f"{case.id}: the [P,6] record differs"
    assert bool(torch.isnan(dfe).all()), "the feature buffer was written though NULL was passed"
    assert bool(rec0.any())


@pytest.mark.parametrize("case", SWEEP_CASES + [c for c in CASES if c.family == "saturating"],
                         ids=[c.id for c in SWEEP_CASES + [c for c in CASES if c.family == "saturating"]])
def test_an_all_ones_column_is_the_accumulated_opacity(device, case):
    """sum of w over the blended entries = 1 - final_T; the reference's float64 and float32 final_T are the arbiter and
    the unit"""
    ones = torch.ones(case.P, 1, dtype=torch.float32, device=device)
    code, out = _map(case, device, ones)
    assert code == 0
    c64, c32 = R.references(case)
    local = torch.zeros(case.H, case.W, dtype=torch.bool)
    for t in range(case.tiles):
        if bool(case.compute_locally[t]):
            x0, y0, x1, y1 = case.tile_box(t)
            local[y0:y1, x0:x1] = True
    m = local.reshape(-1, 1)
    want64 = torch.where(m, 1.0 - c64["final_T"].double(), torch.zeros((), dtype=torch.float64))
    want32 = torch.where(m, 1.0 - c32["final_T"].float(), torch.zeros(()))
    unit, worst = assert_rows_close(out.cpu().reshape(-1, 1), want64, want32, 8, f"{case.id} alpha map")
    print(f"FEATURES {case.id} alpha map: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")


def test_p0_p1_and_the_refused_calls(device):
    lib = PX._lib()
    p0 = next(c for c in CASES if c.id == "inert-P0")
    out, rec, dfe = _root(p0, 4, device)  # P == 0: the forward clears the map, the backward succeeds and writes nothing
    assert not bool(_bits(out).any()) and bool(torch.isnan(rec).all()) and bool(torch.isnan(dfe).all())
    case = next(c for c in CASES if c.id == "inert-P1")
    out, rec, dfe = _root(case, 4, device)  # one listed row, blended nowhere: a zero map and zero rows
    assert not bool(_bits(out).any()) and not bool(_bits(rec).any()) and not bool(_bits(dfe).any())
    d = PX._dev(case, device)
    fT, nc = _k8(case, device)
    feat, g = _inputs(case, 4, device)
    out = torch.full((4, case.H, case.W), NAN, dtype=torch.float32, device=device)
    rec = torch.full((1, 6), NAN, dtype=torch.float32, device=device)
    dfe = torch.full((1, 4), NAN, dtype=torch.float32, device=device)
    acc = torch.full((1, 10), NAN, dtype=torch.float64, device=device)
    p = PX._p
    fwd = [p(d.ranges), p(d.point_list), p(d.means2D), p(d.co), p(feat), p(d.mask), p(nc)]
    bwd = fwd + [p(fT), p(g)]
    st = PX._stream()
    tail = (0, 0, p(rec), p(dfe), p(acc), st)
    for C in (0, -1, FR.CAP + 1):
        assert lib.gsr_render_features(1, C, 16, 16, *fwd, 0, 0, p(out), st) == GSR_EINVAL, f"forward C = {C}"
        assert lib.gsr_render_features_backward(1, C, 16, 16, *bwd, *tail) == GSR_EINVAL, f"backward C = {C}"
    assert lib.gsr_render_features(-1, 4, 16, 16, *fwd, 0, 0, p(out), st) == GSR_EINVAL
    assert lib.gsr_render_features(1, 4, 0, 16, *fwd, 0, 0, p(out), st) == GSR_EINVAL
    assert lib.gsr_render_features(1, 4, 16, -3, *fwd, 0, 0, p(out), st) == GSR_EINVAL
    assert lib.gsr_render_features(1, 4, 16, 16, *fwd, 0, 0, None, st) == GSR_EINVAL
    for i in (0, 2, 3, 4, 5, 6):  # (point_list may be missing: every list can be empty; 4 = features)
        args = list(fwd)
        args[i] = None
        assert lib.gsr_render_features(1, 4, 16, 16, *args, 0, 0, p(out), st) == GSR_EINVAL, f"forward argument {i}"
    assert lib.gsr_render_features_backward(-1, 4, 16, 16, *bwd, *tail) == GSR_EINVAL
    assert lib.gsr_render_features_backward(1, 4, 16, 0, *bwd, *tail) == GSR_EINVAL
    for i in (0, 2, 3, 4, 5, 6, 7, 8):
        args = list(bwd)
        args[i] = None
        assert lib.gsr_render_features_backward(1, 4, 16, 16, *args, *tail) == GSR_EINVAL, f"backward argument {i}"
    assert lib.gsr_render_features_backward(1, 4, 16, 16, *bwd, 0, 0, None, p(dfe), p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_features_backward(1, 4, 16, 16, *bwd, 0, 0, p(rec), p(dfe), None, st) == GSR_EINVAL
    assert lib.gsr_render_features_backward(0, 4, 16, 16, *([None] * 9), 0, 0, None, None, None, st) == 0
    torch.cuda.synchronize()
    # every refusal came before any device work
    assert bool(torch.isnan(out).all() & torch.isnan(rec).all() & torch.isnan(dfe).all()) and bool(torch.isnan(acc).all())
