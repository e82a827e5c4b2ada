"""-m gpu: gsr_render_surfels and gsr_render_surfels_backward through the C ABI on explicit lists: every pixel of the nine
float maps and of median_pos, and every Gaussian row of both records, against float64 (tests/surfel_refs.py).

K8 (as tests/test_gpu_composite_pixels.py calls it) gives n_contrib and final_T; outputs and the fp64 scratch are
pre-filled with NaN (-7 for median_pos).  mu and S are compared where A > 0; med, median_pos and the d_z rows leave out
the NEAR pixels and the rows they feed, on every case (surfel_refs' docstring).  The N maps of `median-mixed` cross
zero, so each is compared as ONE row: against the map's largest value, not the pixel's.  K: surfel_refs.K_of.  Each
figure (unit in 2^-24, worst ratio) is printed before it is asserted; EXPERIMENTS.md records them."""
import pytest
import torch

import surfel_refs as SR
import test_gpu_composite_pixels as PX
from helpers import assert_rows_close

pytestmark = pytest.mark.gpu

R, p = SR.R, PX._p
U, NAN, GSR_EINVAL = 2.0 ** -24, float("nan"), -1
CASES = SR.cases()
RUNS = [(c, "depth") for c in CASES] + [(c, m) for c in CASES if c.id == SR.MAPPING_CASE for m in ("inverse", "ndc")]
_ROOT = {}


def _inputs(case, device):
    """the seven list / row pointers, K8's final_T, and the upstream maps: uploaded and computed once per case"""
    d = PX._dev(case, device)
    if not hasattr(d, "surfels"):
        fwd = PX._forward(d)
        assert fwd[0] == 0, f"gsr_render_forward returned {fwd[0]}"
        d.k8 = (fwd[2], fwd[3])
        d.surfels = [t.to(device).contiguous() for t in SR.draw(case)]  # rows, dL/dsurfel, dL/ddist, dL/dmedian
    return [p(t) for t in (d.ranges, d.point_list, d.means2D, d.co, d.surfels[0], d.mask, d.k8[1])], d.k8[0], d.surfels[1:]


def _maps(case, device, mapping="depth", band=(0, 0)):
    """-> (code, (surfel [5,H,W], aux [4,H,W], median_pos [H,W]))"""
    out = (torch.full((5, case.H, case.W), NAN, device=device), torch.full((4, case.H, case.W), NAN, device=device),
           torch.full((case.H, case.W), -7, dtype=torch.int32, device=device))
    code = PX._lib().gsr_render_surfels(case.P, case.W, case.H, *_inputs(case, device)[0], *SR.COEF[mapping], *band,
                                        *map(p, out), PX._stream())
    torch.cuda.synchronize()
    return code, out


def _records(case, device, maps, mapping="depth", band=(0, 0), use=(True, True, True), zeros=False):
    """-> (code, dL_record [max(P,1),6], dL_rows [.,5]).  `use`: which of dL/dsurfel, dL/ddist, dL/dmedian are passed; the
    others are NULL, or all-zero maps with `zeros`"""
    n = max(case.P, 1)
    rec, drows = torch.full((n, 6), NAN, device=device), torch.full((n, 5), NAN, device=device)
    acc = torch.full((n, 10), NAN, dtype=torch.float64, device=device)
    args, fT, ups = _inputs(case, device)
    ups = [g if u else (torch.zeros_like(g) if zeros else None) for g, u in zip(ups, use)]
    code = PX._lib().gsr_render_surfels_backward(case.P, case.W, case.H, *args, *SR.COEF[mapping], p(fT), *map(p, maps),
                                                 *map(p, ups), *band, p(rec), p(drows), p(acc), PX._stream())
    torch.cuda.synchronize()
    return code, rec, drows


def _root(case, device, mapping="depth"):
    """whole-grid maps and records of one (case, mapping): computed once and never modified"""
    if (case.id, mapping) not in _ROOT:
        code, maps = _maps(case, device, mapping)
        code2, rec, drows = _records(case, device, maps, mapping)
        assert code == 0 and code2 == 0, (code, code2)
        _ROOT[case.id, mapping] = (maps, rec, drows)
    return _ROOT[case.id, mapping]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case,mapping", RUNS, ids=[f"{c.id}-{m}" for c, m in RUNS])
def test_every_pixel_and_every_row_against_float64(device, case, mapping):
    maps, rec, drows = _root(case, device, mapping)
    r64, r32 = SR.references(case, mapping)
    assert torch.equal(PX._dev(case, device).k8[1].cpu(), r64["n_contrib"]), "K8's n_contrib is not the reference's"
    assert (SR.near_fraction(case, mapping) > SR.NEAR_CAP) == (case.id in SR.OVER_CAP)
    both = torch.cat([maps[0], maps[1]]).cpu()  # (A, D, N | Dist, mu, S, med)
    got, mpos = both.reshape(9, -1), maps[2].cpu()
    for t in range(case.tiles):
        if not bool(case.compute_locally[t]):
            x0, y0, x1, y1 = case.tile_box(t)
            assert not bool(_bits(both[:, y0:y1, x0:x1]).any()) and not bool(mpos[y0:y1, x0:x1].any()), f"tile {t} (not ours) is not +0"
    seen, far = r64["A"].reshape(-1) > 0, ~r64["near"]
    assert not bool(_bits(got[:, ~seen]).any()) and not bool(mpos.reshape(-1)[~seen].any()), \
        "a pixel that blends nothing is not +0 in every map"
    fig = {}
    for i, k in enumerate(SR.MAPS):
        rows = seen if k in ("mu", "S") else far if k == "med" else slice(None)
        shape = (1, -1) if case.id == "median-mixed" and k[0] == "N" else (-1, 1)
        fig[k] = assert_rows_close(got[i].reshape(-1, 1)[rows].reshape(shape), r64[k][rows].reshape(shape),
                                   r32[k][rows].reshape(shape), SR.K_of(case, k), f"{case.id} {k}")
    assert torch.equal(mpos.reshape(-1)[far], r64["median_pos"][far]), "median_pos differs outside the near pixels"
    if case.P == 0:  # the all-zero maps; the backward succeeds and writes not one word
        assert bool(torch.isnan(rec).all()) and bool(torch.isnan(drows).all())
    else:
        groups = SR.split_records(rec.cpu()[:case.P], drows.cpu()[:case.P])
        for k in SR.GROUPS:
            rows = ~r64["near_rows"] if k == "d_z" else slice(None)
            fig[k] = assert_rows_close(groups[k][rows], r64[k][rows], r32[k][rows], SR.K_of(case, k), f"{case.id} {k}")
        recs = torch.cat([rec, drows], dim=1).cpu()[:case.P]
        assert not bool(_bits(recs[~r64["blended"]]).any()), "a row that is blended nowhere is not +0.0f"
        assert not bool(_bits(recs[:, 6]).any()), "column 0 of dL_rows is not +0"
    for k, (unit, worst) in fig.items():
        print(f"SURFELS {case.id} {mapping} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")


SEPARATION = [c for c in CASES if c.id in ("lengths-65", "edges-37x21-holes", "median-cross-64")]


@pytest.mark.parametrize("case", SEPARATION, ids=[c.id for c in SEPARATION])
@pytest.mark.parametrize("use", [(True, False, False), (False, True, False), (False, False, True)],
                         ids=["surfel-only", "dist-only", "median-only"])
def test_a_null_upstream_map_is_an_all_zero_one_bit_for_bit(device, case, use):
    """NULL against zeros; with dL/dsurfel NULL the matrix-pipe part is compiled out, with zeros it runs"""
    maps = _root(case, device)[0]
    null, zero = _records(case, device, maps, use=use), _records(case, device, maps, use=use, zeros=True)
    assert null[0] == 0 and zero[0] == 0
    assert torch.equal(_bits(null[1]), _bits(zero[1])) and torch.equal(_bits(null[2]), _bits(zero[2]))
    assert bool(null[1].any()) or bool(null[2].any())  # (an empty record would make the comparison empty)


VARIANTS = [c for c in CASES if c.family in R.VARIANT_FAMILIES and c.P > 0]
assert any(c.band is not None for c in VARIANTS), "no case with a proper row band"


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
@pytest.mark.parametrize("kind", ["host", "device", "device-larger", "again"])
def test_row_bands_and_a_second_backward_are_bit_equal_to_the_whole_grid(device, case, kind):
    maps0, rec0, drows0 = _root(case, device)
    lo, hi = case.band if case.band is not None else case.hull
    assert (lo, hi) == case.hull and hi > lo
    band = {"host": (lo, hi), "device": (-1, hi - lo), "device-larger": (-1, case.gy), "again": (0, 0)}[kind]
    code, maps = _maps(case, device, band=band)
    assert code == 0 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(maps, maps0)), f"{case.id} {kind}: the maps differ"
    code, rec, drows = _records(case, device, maps, band=band)
    assert code == 0 and torch.equal(_bits(rec), _bits(rec0)) and torch.equal(_bits(drows), _bits(drows0))
    assert bool(maps0[0][0].any()) == (case.id != "inert-P1")  # (an empty map would make the comparison empty)


def test_p1_and_the_refused_calls(device):
    lib, st, c = PX._lib(), PX._stream(), SR.COEF["ndc"]
    case = next(c for c in CASES if c.id == "inert-P1")
    maps, rec, drows = _root(case, device)  # one listed row, blended nowhere: zero maps and zero rows
    assert not any(bool(_bits(t).any()) for t in (*maps, rec, drows))
    outs = [torch.full((5, 16, 16), NAN, device=device), torch.full((4, 16, 16), NAN, device=device),
            torch.full((16, 16), -7, dtype=torch.int32, device=device)]
    dsts = [torch.full((1, 6), NAN, device=device), torch.full((1, 5), NAN, device=device),
            torch.full((1, 10), NAN, dtype=torch.float64, device=device)]
    args, fT, ups = _inputs(case, device)
    # the argument lists of the two calls, and in each the positions that must not be NULL (point_list, position 1 of the
    # lists, and the three upstream maps may be missing)
    fwd = [1, 16, 16, *args, *c, 0, 0, *map(p, outs), st]
    bwd = [1, 16, 16, *args, *c, p(fT), *map(p, maps), *map(p, ups), 0, 0, *map(p, dsts), st]
    for fn, full, needed in ((lib.gsr_render_surfels, fwd, [3, 5, 6, 7, 8, 9, 15, 16, 17]),
                             (lib.gsr_render_surfels_backward, bwd, [3, 5, 6, 7, 8, 9, 13, 14, 15, 16, 22, 23, 24])):
        bad = [[v if j != i else None for j, v in enumerate(full)] for i in needed]
        bad += [[P, W, H] + full[3:] for P, W, H in ((-1, 16, 16), (1, 0, 16), (1, 16, -3))]
        for call in bad:
            assert fn(*call) == GSR_EINVAL, call
    assert lib.gsr_render_surfels_backward(0, *bwd[1:]) == 0  # P == 0: nothing to do
    torch.cuda.synchronize()
    # every refusal came before any device work
    assert all(bool(torch.isnan(t).all()) for t in (outs[0], outs[1], *dsts)) and bool((outs[2] == -7).all())
