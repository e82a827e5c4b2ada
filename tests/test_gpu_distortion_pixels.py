"""-m gpu: gsr_render_distortion and gsr_render_distortion_backward through the C ABI on explicit lists: every pixel of
the four maps and every Gaussian row of the record against the float64 pairwise reference (tests/distortion_refs.py).

Per case of tests/composite_refs.py plus the `far-thin` family, K8 (as tests/test_gpu_composite_pixels.py calls it) gives
n_contrib and final_T, then the two new entry points walk the same lists.  Outputs, and the fp64 scratch the call clears
itself, are pre-filled with NaN and nothing is excluded; mu and S are compared where A > 0 (elsewhere they are +0, with
all pixels of tiles that are not ours); rows blended nowhere are +0.0f.  The unit is the float32 REFERENCE's own error.
The three mappings run on distortion_refs.MAPPING_CASE.  Host-band, device-band and device-larger launches give the
whole-grid launch's bits, and so does a second run of the backward.

K (distortion_refs.K_of): the composite kernels' and the inverse-depth map's where they hold, else twice the worst
ratio measured, for the reasons given there.
Each figure (unit in 2^-24, worst ratio) is printed before it is asserted; EXPERIMENTS.md records them."""
import pytest
import torch

import composite_refs as R
import distortion_refs as DR
import test_gpu_composite_pixels as PX
from helpers import assert_rows_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
GSR_EINVAL = -1
CASES = DR.cases()
RUNS = [(c, "depth") for c in CASES] + [(c, m) for c in CASES if c.id == DR.MAPPING_CASE for m in ("inverse", "ndc")]

_FWD, _ROOT = {}, {}


def _k8(case, device):
    """K8's (final_T, n_contrib) of the case (whole grid, no segments): computed once and never modified"""
    if case.id not in _FWD:
        fwd = PX._forward(PX._dev(case, device))
        assert fwd[0] == 0, f"gsr_render_forward returned {fwd[0]}"
        _FWD[case.id] = (fwd[2], fwd[3])
    return _FWD[case.id]


def _inputs(case, device):
    d = PX._dev(case, device)
    if not hasattr(d, "distortion"):
        d.distortion = (DR.depths_of(case).to(device).contiguous(), DR.IR.g_of(case).to(device).contiguous())
    return [PX._p(t) for t in (d.ranges, d.point_list, d.means2D, d.co, d.distortion[0], d.mask, _k8(case, device)[1])]


def _maps(case, device, mapping="depth", band=(0, 0)):
    """gsr_render_distortion into NaN-filled maps -> (code, maps [4,H,W] on the device)"""
    out = torch.full((4, case.H, case.W), NAN, dtype=torch.float32, device=device)
    code = PX._lib().gsr_render_distortion(case.P, case.W, case.H, *_inputs(case, device), *DR.COEF[mapping], band[0],
                                           band[1], PX._p(out), PX._stream())
    torch.cuda.synchronize()
    return code, out


def _record(case, device, maps, mapping="depth", band=(0, 0)):
    """gsr_render_distortion_backward into a NaN-filled record and NaN-filled sums -> (code, record [max(P,1),7])"""
    n = max(case.P, 1)
    rec = torch.full((n, 7), NAN, dtype=torch.float32, device=device)
    acc = torch.full((n, 7), NAN, dtype=torch.float64, device=device)
    args = _inputs(case, device)
    g = PX._dev(case, device).distortion[1]
    code = PX._lib().gsr_render_distortion_backward(case.P, case.W, case.H, *args, *DR.COEF[mapping],
                                                    PX._p(_k8(case, device)[0]), PX._p(maps), PX._p(g), band[0], band[1],
                                                    PX._p(rec), PX._p(acc), PX._stream())
    torch.cuda.synchronize()
    return code, rec


def _root(case, device, mapping="depth"):
    """whole-grid maps and record of one (case, mapping): computed once and never modified"""
    if (case.id, mapping) not in _ROOT:
        code, maps = _maps(case, device, mapping)
        assert code == 0, f"gsr_render_distortion returned {code}"
        code, rec = _record(case, device, maps, mapping)
        assert code == 0, f"gsr_render_distortion_backward returned {code}"
        _ROOT[case.id, mapping] = (maps, rec)
    return _ROOT[case.id, mapping]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case,mapping", RUNS, ids=[f"{c.id}-{m}" for c, m in RUNS])
def test_every_pixel_and_every_row_against_float64(device, case, mapping):
    maps, rec = _root(case, device, mapping)
    r64, r32 = DR.references(case, mapping)
    assert torch.equal(_k8(case, device)[1].cpu(), r64["n_contrib"]), "K8's n_contrib is not the reference's: the comparison is void"
    got = maps.cpu()
    for t in range(case.tiles):
        if not bool(case.compute_locally[t]):
            x0, y0, x1, y1 = case.tile_box(t)
            assert not bool(_bits(got[:, y0:y1, x0:x1]).any()), f"{case.id}: maps of tile {t} (not ours) are not +0"
    seen = r64["A"].reshape(-1) > 0
    assert not bool(_bits(got.reshape(4, -1)[:, ~seen]).any()), "a pixel that blends nothing is not +0 in every map"
    fig = {}
    for i, k in enumerate(DR.MAPS):
        rows = seen if k in ("mu", "S") else slice(None)
        fig[k] = assert_rows_close(got[i].reshape(-1, 1)[rows], r64[k][rows], r32[k][rows], DR.K_of(case, k), f"{case.id} {k}")
    if case.P == 0:  # the all-zero maps; the backward succeeds and writes not one word
        assert not bool(_bits(got).any()) and bool(torch.isnan(rec).all())
    else:
        rows = DR.split_record(rec.cpu()[:case.P])
        for k in DR.GROUPS:
            fig[k] = assert_rows_close(rows[k], r64[k], r32[k], DR.K_of(case, k), f"{case.id} {k}")
        assert not bool(_bits(rec.cpu()[:case.P][~r64["blended"]]).any()), "a row that is blended nowhere is not +0.0f"
    for k, (unit, worst) in fig.items():
        print(f"DISTORTION {case.id} {mapping} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")


VARIANTS = [c for c in CASES if c.family in R.VARIANT_FAMILIES and c.P > 0]
assert any(c.band is not None for c in VARIANTS), "no case with a proper row band"


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
@pytest.mark.parametrize("kind", ["host", "device", "device-larger", "again"])
def test_row_bands_and_a_second_backward_are_bit_equal_to_the_whole_grid(device, case, kind):
    """the launch covers the band's tiles only (host rows; or row_lo = -1 with a capacity, the band read from the hull
    behind the range table); "again": the whole grid once more"""
    maps0, rec0 = _root(case, device)
    lo, hi = case.band if case.band is not None else case.hull
    assert (lo, hi) == case.hull and hi > lo
    band = {"host": (lo, hi), "device": (-1, hi - lo), "device-larger": (-1, case.gy), "again": (0, 0)}[kind]
    code, maps = _maps(case, device, band=band)
    assert code == 0 and torch.equal(_bits(maps), _bits(maps0)), f"{case.id} {kind}: the maps differ"
    code, rec = _record(case, device, maps, band=band)
    assert code == 0 and torch.equal(_bits(rec), _bits(rec0)), f"{case.id} {kind}: the record differs"
    assert bool(maps0[1].any()) == (case.id != "inert-P1")  # (an empty map would make the comparison empty)


def test_p1_and_the_refused_calls(device):
    lib = PX._lib()
    case = next(c for c in CASES if c.id == "inert-P1")
    maps, rec = _root(case, device)  # one listed row, blended nowhere: zero maps and a zero row
    assert not bool(_bits(maps).any()) and not bool(_bits(rec).any())
    out = torch.full((4, case.H, case.W), NAN, dtype=torch.float32, device=device)
    rec = torch.full((1, 7), NAN, dtype=torch.float32, device=device)
    acc = torch.full((1, 7), NAN, dtype=torch.float64, device=device)
    p, st, c = PX._p, PX._stream(), DR.COEF["ndc"]
    fwd = _inputs(case, device)
    tail = [p(_k8(case, device)[0]), p(maps), p(PX._dev(case, device).distortion[1])]
    for P, W, H, o in ((-1, 16, 16, p(out)), (1, 0, 16, p(out)), (1, 16, -3, p(out)), (1, 16, 16, None)):
        assert lib.gsr_render_distortion(P, W, H, *fwd, *c, 0, 0, o, st) == GSR_EINVAL
    for i in (0, 2, 3, 4, 5, 6):  # (point_list may be missing: every list can be empty)
        args = list(fwd)
        args[i] = None
        assert lib.gsr_render_distortion(1, 16, 16, *args, *c, 0, 0, p(out), st) == GSR_EINVAL, f"forward argument {i}"
        assert lib.gsr_render_distortion_backward(1, 16, 16, *args, *c, *tail, 0, 0, p(rec), p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_distortion_backward(-1, 16, 16, *fwd, *c, *tail, 0, 0, p(rec), p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_distortion_backward(1, 16, 0, *fwd, *c, *tail, 0, 0, p(rec), p(acc), st) == GSR_EINVAL
    for i in range(3):
        args = list(tail)
        args[i] = None
        assert lib.gsr_render_distortion_backward(1, 16, 16, *fwd, *c, *args, 0, 0, p(rec), p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_distortion_backward(1, 16, 16, *fwd, *c, *tail, 0, 0, None, p(acc), st) == GSR_EINVAL
    assert lib.gsr_render_distortion_backward(1, 16, 16, *fwd, *c, *tail, 0, 0, p(rec), None, st) == GSR_EINVAL
    torch.cuda.synchronize()
    # every refusal came before any device work
    assert bool(torch.isnan(out).all() & torch.isnan(rec).all()) and bool(torch.isnan(acc).all())
