"""tests/binning_refs.py against the second statement of the reference (oracle/gsraster_ref.c through oracle.cref), the
families against what they promise, and check_lists against lists that are wrong in one place."""
import numpy as np
import pytest
import torch

import binning_refs as R

CASES = R.all_cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_upper_lists_equal_the_c_reference(case):
    from oracle import cref as C

    pl, ranges, touched = C.bin_and_sort(torch.tensor(case.means2D), torch.tensor(case.radii), torch.tensor(case.depths),
                                         torch.tensor(case.mask), case.W, case.H)
    up = R.upper_lists(case, edge="oracle")  # the C file's spelling of the upper edge, p + r + BLOCK - 1
    assert up.count == pl.numel() == int(touched.sum())
    assert np.array_equal(up.gid, pl.numpy().astype(np.int64))
    assert np.array_equal(up.ranges, ranges.numpy().astype(np.int64))
    assert np.array_equal(np.bincount(up.gid, minlength=case.P), touched.numpy())
    # common.h's spelling, (p + r) + 15 -- what the kernels are held to: the same lists on every family but `borders`,
    # whose rows sit on the ulp where the two spellings part (test_the_two_spellings_of_the_upper_edge_part_on_borders)
    mine = R.upper_lists(case)
    same = mine.count == up.count and np.array_equal(mine.gid, up.gid) and np.array_equal(mine.ranges, up.ranges)
    assert same == (case.name != "borders"), case.name


def test_the_two_spellings_of_the_upper_edge_part_on_borders():
    """gsr_get_rect (common.h) sums (p + r) + 15, oracle/gsraster_ref.c ((p + r) + 16) - 1.  On the
    rows of `borders` whose p + r + 15 lies within an ulp of a multiple of 16 the C file's rect is one tile wider or
    narrower: 27 pairs of 15 701, 16 of them pairs that float64 says contribute (alpha 0.9: radius 1, the centre an ulp
    below a tile border).  Known and kept: K1, K2 and K3 share gsr_get_rect, and changing its order of additions changes
    the lists of ordinary scenes -- rarely, but a training run does not forgive one pair (EXPERIMENTS.md)."""
    (case,) = R.borders()
    a, b = R.upper_lists(case), R.upper_lists(case, edge="oracle")
    ka, kb = a.tile * case.P + a.gid, b.tile * case.P + b.gid
    only_a, only_b = np.setdiff1d(ka, kb), np.setdiff1d(kb, ka)
    print(f"borders: {a.count} pairs by common.h, {b.count} by the C file; {only_a.size} only in the former, {only_b.size} "
          f"only in the latter")
    assert only_a.size + only_b.size > 0
    rows = np.unique(np.concatenate([only_a, only_b]) % case.P)
    s = np.stack([case.means2D[rows, 0], case.means2D[rows, 1]], axis=1) + case.radii[rows, None].astype(np.float32)
    edge = (s + np.float32(15)) / np.float32(16)
    near = np.abs(edge - np.round(edge)) <= 2.0 ** -20  # within an ulp or two of a whole tile, in x or in y
    assert near.any(axis=1).all()
    mk = R.must_keep(case, only_b // case.P, only_b % case.P)
    print(f"borders: {int(mk.sum())} of the {only_b.size} pairs only the C file lists may not be dropped by its rule")
    assert (only_a.size, only_b.size, int(mk.sum())) == (0, 27, 16)


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_family_has_pairs_that_must_be_kept(family):
    for case in R.FAMILIES[family]():
        n = int(R.must_keep_upper(case).sum())
        print(f"{case.name}: P {case.P}, upper pairs {R.upper_lists(case).count}, must_keep {n}")
        empty = case.name in ("masks none", "counts all radii 0")
        assert (n == 0 and R.upper_lists(case).count == 0) if empty else n > 0, case.name


def test_needles_hold_improper_conics():
    (case,) = R.needles()
    gen = case.meta["generated"]
    bad = R.improper(case)
    print(f"needles: {int(bad[:gen].sum())} of {gen} generated conics have a float32 A C - B B <= 0")
    assert 1900 <= gen <= 2000 and case.P == gen + 6 * len(R.NEEDLE_TRIPLES)
    assert int(bad[:gen].sum()) >= 5
    co = case.conic_opacity[gen:gen + len(R.NEEDLE_TRIPLES), :3]
    assert np.array_equal(co, np.array(R.NEEDLE_TRIPLES, dtype=np.float32))
    assert (case.conic_opacity[:, 3] == np.float32(0.9)).all()
    assert ((case.radii >= 40) & (case.radii <= 400)).all()
    xy = case.means2D
    assert (xy == np.round(xy)).all() and (xy >= 0).all() and (xy < 256).all()
    # the improper ones are not inert: the reference blends them on many tiles
    up, mk = R.upper_lists(case), R.must_keep_upper(case)
    assert np.bincount(up.gid[mk], minlength=case.P)[bad].min() >= 1


def test_opacity_cut_counts():
    (case,) = R.opacity_cut()
    o = case.conic_opacity[:, 3]
    cut = np.float32(1.0 / 255.0)
    assert [float(v) for v in R.OPACITIES[3:]] == [float(np.float32(0.99)), 1.0, 1.5]
    assert R.OPACITIES[0] < cut == R.OPACITIES[1] < R.OPACITIES[2]
    assert R.OPACITIES[1].view(np.uint32) - R.OPACITIES[0].view(np.uint32) == 1
    assert R.OPACITIES[2].view(np.uint32) - R.OPACITIES[1].view(np.uint32) == 1
    for v in R.OPACITIES:
        assert int((o == v).sum()) == case.meta["per_opacity"]
    # every centre is a pixel centre inside the frame: power == 0 is reached, so a splat is kept on its own tile exactly
    # when its opacity is at or above the cut
    xy = case.means2D
    assert (xy == np.round(xy)).all() and (xy >= 0).all() and (xy[:, 0] < case.W).all() and (xy[:, 1] < case.H).all()
    up, mk = R.upper_lists(case), R.must_keep_upper(case)
    own = (xy[:, 1] // 16).astype(np.int64) * case.gx + (xy[:, 0] // 16).astype(np.int64)
    on_own = up.tile == own[up.gid]
    assert np.array_equal(np.bincount(up.gid[on_own], minlength=case.P), np.ones(case.P, dtype=np.int64))
    kept_own = np.zeros(case.P, dtype=bool)
    kept_own[up.gid[on_own]] = mk[on_own]
    assert np.array_equal(kept_own, o >= cut)
    assert not mk[o[up.gid] < cut].any()


def test_rect_sizes_have_the_stated_shapes():
    (case,) = R.rect_sizes()
    shapes = case.meta["shapes"]
    assert {int(w * h) for w, h in shapes} >= {63, 64, 65} and case.W >= 1040 and case.H >= 1040
    up, mk = R.upper_lists(case), R.must_keep_upper(case)
    for g, (w, h) in enumerate(shapes):  # the tiles the ellipse itself reaches: a w x h box
        t = up.tile[mk & (up.gid == g)]
        tx, ty = t % case.gx, t // case.gx
        assert (tx.max() - tx.min() + 1, ty.max() - ty.min() + 1) == (w, h), (g, w, h)


def test_position_tie_runs_are_short():
    (case,) = R.position_ties()
    n = np.unique(R.depth_bits(case), return_counts=True)[1]
    assert n.min() >= 2 and n.max() <= 32 and case.P == 4000
    a, p = R.upper_lists(case), R.upper_lists(case, "position")
    assert a.count == p.count and np.array_equal(a.tile, p.tile) and not np.array_equal(a.gid, p.gid)


# ---------------------------------------------------------------------------------------------- check_lists has teeth
def _teeth_case():
    return R.masks()[-1]  # all tiles local


def _band_case():
    W, H = 333, 211
    g = R.masks()[0]
    mask = np.zeros((14, 21), dtype=bool)
    mask[3:9, :] = True  # a whole-row band: no non-local tile inside the hull
    return R.make_case("band", g.means2D, g.depths, g.radii, g.conic_opacity, W, H, mask=mask)


def test_check_lists_accepts_the_upper_lists():
    for case in (_teeth_case(), _band_case(), R.whole_frame()[0], R.depth_keys()[0]):
        pl, rg, D = R.as_lists(case)
        got = R.check_lists(pl, rg, D, case, exact=True)
        assert got["kept"] == D and got["dropped"] == 0
    (case,) = R.position_ties()
    R.check_lists(*R.as_lists(case, "position"), case, tie="position", exact=True)
    with pytest.raises(AssertionError, match="order"):
        R.check_lists(*R.as_lists(case, "position"), case, tie="arrival")
    with pytest.raises(AssertionError, match="order"):
        R.check_lists(*R.as_lists(case, "arrival"), case, tie="position")


def _remove(pl, rg, D, j):
    """the lists without entry j"""
    pl, rg = np.delete(pl, j), rg.copy()
    body = rg[:-1]
    live = body[:, 1] > body[:, 0]
    body[live & (body[:, 0] > j), 0] -= 1
    body[live & (body[:, 1] > j), 1] -= 1
    return pl, rg, D - 1


def test_check_lists_accepts_dropping_what_cannot_contribute_and_rejects_a_must_keep_pair():
    case = _teeth_case()
    pl, rg, D = R.as_lists(case)
    mk = R.must_keep_upper(case)
    assert (~mk).any() and mk.any()
    j = int(np.flatnonzero(~mk)[len(np.flatnonzero(~mk)) // 2])
    got = R.check_lists(*_remove(pl, rg, D, j), case)
    assert got["dropped"] == 1
    with pytest.raises(AssertionError, match="missing"):
        R.check_lists(*_remove(pl, rg, D, j), case, exact=True)
    j = int(np.flatnonzero(mk)[len(np.flatnonzero(mk)) // 2])
    with pytest.raises(AssertionError, match="would have contributed"):
        R.check_lists(*_remove(pl, rg, D, j), case)


def test_check_lists_rejects_swapped_depth_ties():
    case = R.depth_keys()[0]  # all depths equal: every neighbour pair inside a tile is a tie
    pl, rg, D = R.as_lists(case)
    t = int(np.flatnonzero(rg[:-1, 1] - rg[:-1, 0] >= 2)[3])
    j = int(rg[t, 0])
    pl[[j, j + 1]] = pl[[j + 1, j]]
    with pytest.raises(AssertionError, match="order"):
        R.check_lists(pl, rg, D, case)


def test_check_lists_rejects_a_pair_from_outside_the_rect():
    case = _teeth_case()
    pl, rg, D = R.as_lists(case)
    up = R.upper_lists(case)
    t = int(np.flatnonzero(rg[:-1, 1] > rg[:-1, 0])[5])
    outside = np.setdiff1d(np.arange(case.P), up.gid[up.tile == t])
    g = int(outside[np.argmin(np.abs(R.depth_bits(case)[outside] - R.depth_bits(case)[pl[rg[t, 0]]]))])
    j = int(rg[t, 0])
    pl2, rg2 = np.insert(pl, j, g), rg.copy()
    body = rg2[:-1]
    live = body[:, 1] > body[:, 0]
    body[live & (body[:, 0] > j), 0] += 1
    body[live & (body[:, 1] > j), 1] += 1
    with pytest.raises(AssertionError, match="does not put there"):
        R.check_lists(pl2, rg2, D + 1, case)


@pytest.mark.parametrize("col,delta", [(1, -1), (1, 1), (0, 1), (0, -1)])
def test_check_lists_rejects_a_range_end_off_by_one(col, delta):
    case = _teeth_case()
    pl, rg, D = R.as_lists(case)
    t = int(np.flatnonzero(rg[:-1, 1] - rg[:-1, 0] >= 2)[7])
    rg[t, col] += delta
    with pytest.raises(AssertionError):
        R.check_lists(pl, rg, D, case)
    pl, rg, D = R.as_lists(case)
    with pytest.raises(AssertionError):  # ... and the last range against D
        R.check_lists(pl, rg, D + 1, case)


def test_check_lists_rejects_a_non_local_tile_with_a_range():
    case = _band_case()
    pl, rg, D = R.as_lists(case)
    R.check_lists(pl, rg, D, case)
    rg[2 * 21 + 4] = (0, 3)
    with pytest.raises(AssertionError, match="non-local"):
        R.check_lists(pl, rg, D, case)


def test_check_lists_rejects_a_wrong_hull_row():
    case = _band_case()
    for hull in ((3, 10), (2, 9), (0, 0), (0, 14)):
        pl, rg, D = R.as_lists(case)
        rg[-1] = hull
        with pytest.raises(AssertionError, match="hull"):
            R.check_lists(pl, rg, D, case)
    pl, rg, D = R.as_lists(case)
    with pytest.raises(AssertionError, match="tiles \\+ 1 rows"):
        R.check_lists(pl, rg[:-1], D, case)


def test_check_lists_bounds_the_slots_between_ranges_by_the_hull():
    """a mask with non-local tiles inside its hull: slots between the ranges are allowed, up to the pairs of those tiles"""
    case = [c for c in R.masks() if c.name == "masks band with holes"][0]
    up = R.upper_lists(case)
    assert up.hole_pairs > 0
    rg = np.concatenate([up.ranges, np.array([R.hull(case.mask)], dtype=np.int64)])
    R.check_lists(up.gid, rg, up.count, case, exact=True)
    shift = rg.copy()
    last = int(np.flatnonzero(rg[:-1, 1] > rg[:-1, 0])[-1])
    shift[last, :] += up.hole_pairs
    pl = np.concatenate([up.gid[:rg[last, 0]], np.zeros(up.hole_pairs, dtype=np.int64), up.gid[rg[last, 0]:]])
    R.check_lists(pl, shift, up.count + up.hole_pairs, case, exact=True)
    shift[last, :] += 1
    with pytest.raises(AssertionError, match="slots outside"):
        R.check_lists(np.insert(pl, int(rg[last, 0]), 0), shift, up.count + up.hole_pairs + 1, case, exact=True)
