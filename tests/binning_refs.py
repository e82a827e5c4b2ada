"""The contract of K3-K7 (binning) in plain numpy, and hand-built input families at the edges of K3's integer decisions.

No torch on a GPU and no project kernel in here.  The inputs are K1's OUTPUTS, given directly (`Case`): means2D [P,2]
f32, depths [P] f32, radii [P] i32, conic_opacity [P,4] f32, mask [gy,gx] bool, W, H.

  upper_lists(case)   the reference rule (csrc/common.h gsr_get_rect): 3-sigma tile rect with C
                      truncation in float32, clamped to the grid, radius <= 0 dropped, the mask applied to the tiles, and
                      inside a tile the order (depth bits as uint32, index) -- or, tie="position", (depth bits, x, y,
                      index).  Every list the kernels give must be an order-preserving subsequence of these.
  must_keep(case, tile, gid)
                      float64, per (tile, Gaussian) pair: some pixel centre of the tile, clipped to the image, has
                      power <= 0 and o exp(power) >= 1/255 with power = -0.5 (A dx^2 + C dy^2) - B dx dy.  A pair for which
                      this holds may never be dropped.  No margin.
  check_lists(...)    asserts all of it on every tile and every pair (a lexsort over the pairs, no loop over tiles).

The pair count D that the kernels report covers the rects clipped to the ROW HULL of the mask: pairs on tiles inside the
hull that are not computed locally are counted and sorted too (in place behind an empty range by the (row, column) forms,
behind the last tile by the generic tile-id sort; tests/test_gpu_parity.py::test_sort_forms_alternate_on_one_kept_scratch
documents the same).  So the local ranges tile [0, D) exactly when the hull has no such tile; when it has, the ranges
must still ascend in tile order without overlap inside [0, D], and the slots between them may not outnumber the
reference's pairs on those tiles.
"""
import functools
from typing import NamedTuple

import numpy as np

BLOCK = 16
F32 = np.float32
CUT32 = np.float32(1.0 / 255.0)


class Case:
    """one view's inputs (read-only arrays); hashed by identity, so the references are cached per case"""

    def __init__(self, name, means2D, depths, radii, conic_opacity, mask, W, H, meta):
        self.name, self.means2D, self.depths, self.radii = name, means2D, depths, radii
        self.conic_opacity, self.mask, self.W, self.H, self.meta = conic_opacity, mask, W, H, meta

    def __repr__(self):
        return self.name

    @property
    def P(self):
        return self.means2D.shape[0]

    @property
    def gx(self):
        return (self.W + BLOCK - 1) // BLOCK

    @property
    def gy(self):
        return (self.H + BLOCK - 1) // BLOCK

    @property
    def tiles(self):
        return self.gx * self.gy


def make_case(name, means2D, depths, radii, conic_opacity, W, H, mask=None, **meta):
    gx, gy = (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK
    if mask is None:
        mask = np.ones((gy, gx), dtype=bool)
    c = Case(name, np.ascontiguousarray(means2D, dtype=F32).reshape(-1, 2), np.ascontiguousarray(depths, dtype=F32),
             np.ascontiguousarray(radii, dtype=np.int32), np.ascontiguousarray(conic_opacity, dtype=F32).reshape(-1, 4),
             np.ascontiguousarray(mask, dtype=bool), int(W), int(H), meta)
    assert c.mask.shape == (gy, gx) and c.depths.shape == (c.P,) and c.radii.shape == (c.P,)
    assert c.conic_opacity.shape == (c.P, 4)
    assert np.isfinite(c.means2D).all() and np.isfinite(c.conic_opacity).all() and not np.isnan(c.depths).any()
    for a in (c.means2D, c.depths, c.radii, c.conic_opacity, c.mask):
        a.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------------ the contract
def rects(case, edge="common.h"):
    """-> int64 minx, miny, maxx, maxy [P]: the reference's tile rect, empty (max = min) for radius <= 0.  The arithmetic
    is float32 throughout, truncated toward zero, then clamped.  The upper edge has two spellings in this project, and
    in float32 they are two functions: edge="common.h", (p + r) + 15 -- gsr_get_rect, SURVEY.md A.2 step 7: what the
    kernels are held to -- and edge="oracle", `p + r + BLOCK - 1` as C evaluates it, ((p + r) + 16) - 1 with a third
    rounding -- oracle/gsraster_ref.c.  They part by an ulp when the sums cross a power of two, which moves the edge by a
    whole tile when it lies on a multiple of 16 (the family `borders` has such rows)."""
    px, py = case.means2D[:, 0], case.means2D[:, 1]
    r = case.radii.astype(F32)
    b, one = F32(BLOCK), F32(1)

    def cut(v, g):
        assert (np.abs(v) < 2.0 ** 31).all(), "the reference's own conversion is undefined past 2^31"
        return np.clip(np.trunc(v).astype(np.int64), 0, g)

    minx, miny = cut((px - r) / b, case.gx), cut((py - r) / b, case.gy)
    if edge == "oracle":
        maxx, maxy = cut((px + r + b - one) / b, case.gx), cut((py + r + b - one) / b, case.gy)
    else:
        assert edge == "common.h"
        maxx, maxy = cut((px + r + (b - one)) / b, case.gx), cut((py + r + (b - one)) / b, case.gy)
    dead = (case.radii <= 0) | (maxx <= minx) | (maxy <= miny)
    maxx, maxy = np.where(dead, minx, maxx), np.where(dead, miny, maxy)
    return minx, miny, maxx, maxy


def _rect_pairs(minx, miny, maxx, maxy, gx):
    """every (tile, Gaussian) of the rects, Gaussian-major"""
    w, h = maxx - minx, maxy - miny
    n = w * h
    gid = np.repeat(np.arange(n.shape[0], dtype=np.int64), n)
    k = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    wg = np.maximum(w[gid], 1)
    tile = (miny[gid] + k // wg) * gx + minx[gid] + k % wg
    return tile, gid


def depth_bits(case):
    return case.depths.view(np.uint32).astype(np.int64)


def _order(case, tile, gid, tie):
    bits = depth_bits(case)[gid]
    if tie == "position":
        return np.lexsort((gid, case.means2D[gid, 1], case.means2D[gid, 0], bits, tile))
    assert tie == "arrival"
    return np.lexsort((gid, bits, tile))


def hull(mask):
    """-> (first row with a local tile, one past the last), (0, 0) for an empty mask"""
    rows = np.flatnonzero(mask.any(axis=1))
    return (int(rows[0]), int(rows[-1]) + 1) if rows.size else (0, 0)


class Upper(NamedTuple):
    tile: np.ndarray     # int64 [N], ascending
    gid: np.ndarray      # int64 [N], reference order inside a tile
    ranges: np.ndarray   # int64 [tiles, 2]
    count: int           # N: pairs on local tiles
    hole_pairs: int      # the reference's pairs on tiles inside the row hull that are not local


@functools.lru_cache(maxsize=None)
def upper_lists(case, tie="arrival", edge="common.h"):
    tile, gid = _rect_pairs(*rects(case, edge), case.gx)
    local = case.mask.reshape(-1)[tile]
    lo, hi = hull(case.mask)
    in_hull = (tile // case.gx >= lo) & (tile // case.gx < hi)
    hole_pairs = int((~local & in_hull).sum())
    tile, gid = tile[local], gid[local]
    o = _order(case, tile, gid, tie)
    tile, gid = tile[o], gid[o]
    n = np.bincount(tile, minlength=case.tiles).astype(np.int64)
    end = np.cumsum(n)
    ranges = np.stack([end - n, end], axis=1)
    ranges[n == 0] = 0
    for a in (tile, gid, ranges):
        a.setflags(write=False)
    return Upper(tile, gid, ranges, int(tile.shape[0]), hole_pairs)


def max_alpha(case, tile, gid, chunk=8192):
    """float64 [n]: the largest o exp(power) over the pixel centres of `tile` (clipped to the image) with power <= 0,
    -inf where no pixel has power <= 0"""
    tile, gid = np.asarray(tile, dtype=np.int64), np.asarray(gid, dtype=np.int64)
    out = np.empty(tile.shape[0], dtype=np.float64)
    m2, co = case.means2D.astype(np.float64), case.conic_opacity.astype(np.float64)
    off = np.arange(BLOCK, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s in range(0, tile.shape[0], chunk):
            t, g = tile[s:s + chunk], gid[s:s + chunk]
            X = ((t % case.gx) * BLOCK)[:, None] + off[None, :]
            Y = ((t // case.gx) * BLOCK)[:, None] + off[None, :]
            dx, dy = m2[g, 0:1] - X, m2[g, 1:2] - Y
            A, B, C, o = co[g, 0:1], co[g, 1:2], co[g, 2:3], co[g, 3]
            power = -0.5 * ((A * dx * dx)[:, None, :] + (C * dy * dy)[:, :, None]) - (B * dx)[:, None, :] * dy[:, :, None]
            alpha = o[:, None, None] * np.exp(power)
            ok = (power <= 0) & (X < case.W)[:, None, :] & (Y < case.H)[:, :, None]
            out[s:s + chunk] = np.where(ok, alpha, -np.inf).reshape(t.shape[0], -1).max(axis=1)
    return out


def must_keep(case, tile, gid):
    return max_alpha(case, tile, gid) >= 1.0 / 255.0


@functools.lru_cache(maxsize=None)
def must_keep_upper(case):
    """must_keep over every pair of the (arrival order) upper lists; computed once per case"""
    up = upper_lists(case)
    mk = must_keep(case, up.tile, up.gid)
    mk.setflags(write=False)
    return mk


def as_lists(case, tie="arrival"):
    """the upper lists in the shape the kernels give: point_list int64 [D], ranges int64 [tiles + 1, 2] (row `tiles`: the
    hull), D -- for a mask without non-local tiles inside its hull"""
    up = upper_lists(case, tie)
    assert up.hole_pairs == 0
    return up.gid.copy(), np.concatenate([up.ranges, np.array([hull(case.mask)], dtype=np.int64)]), up.count


def check_lists(point_list, ranges, D, case, tie="arrival", exact=False):
    """Assert the contract on every tile and pair.  point_list: integer [>= D]; ranges: integer [tiles + 1, 2] with the hull
    in row `tiles`; exact: the lists must EQUAL the upper lists (nothing may be narrowed away).  -> dict(kept, dropped,
    tile, gid): the kernel's pairs in list order."""
    pl = np.asarray(point_list).astype(np.int64).reshape(-1)
    rg = np.asarray(ranges).astype(np.int64)
    D = int(D)
    up = upper_lists(case, tie)
    tiles, P = case.tiles, case.P
    assert rg.shape == (tiles + 1, 2), f"{case.name}: ranges must have tiles + 1 rows, got {rg.shape}"
    assert tuple(rg[tiles]) == hull(case.mask), f"{case.name}: hull row {tuple(rg[tiles])} != {hull(case.mask)}"
    s, e = rg[:tiles, 0], rg[:tiles, 1]
    local = case.mask.reshape(-1)
    bad = np.flatnonzero(~local & (e != s))
    assert bad.size == 0, f"{case.name}: non-local tile {bad[:1]} has the range {rg[bad[:1]]}"
    assert 0 <= D <= pl.shape[0] or D == 0, f"{case.name}: D = {D} but point_list holds {pl.shape[0]}"
    bad = np.flatnonzero((e < s) | (s < 0) | (e > D))
    assert bad.size == 0, f"{case.name}: tile {bad[:1]} has the range {rg[bad[:1]]} outside [0, {D}]"
    ne = np.flatnonzero(e > s)  # tile order
    gaps = np.diff(np.concatenate([[0], np.stack([s[ne], e[ne]], axis=1).reshape(-1), [D]]))[::2]
    assert (gaps >= 0).all(), f"{case.name}: ranges overlap or do not ascend in tile order at tile {ne[np.argmax(gaps[:-1] < 0)] if ne.size else -1}"
    if up.hole_pairs == 0:
        assert (gaps == 0).all(), f"{case.name}: the local ranges leave a gap in [0, {D}) (sizes {gaps[gaps != 0][:4]})"
    else:
        assert gaps.sum() <= up.hole_pairs, f"{case.name}: {gaps.sum()} slots outside the local ranges, the hull's non-local tiles have {up.hole_pairs} pairs"
    n = e[ne] - s[ne]
    ktile = np.repeat(ne, n)
    kgid = pl[np.repeat(s[ne], n) + np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)]
    assert ((kgid >= 0) & (kgid < P)).all(), f"{case.name}: an index outside [0, {P})"
    # position of every kernel pair in the upper list; the upper keys ascend with the tile, not inside it, so sort them
    ukey = up.tile * P + up.gid
    uo = np.argsort(ukey, kind="stable")
    kkey = ktile * P + kgid
    pos = np.searchsorted(ukey[uo], kkey)
    found = (pos < ukey.shape[0]) & (ukey[uo][np.minimum(pos, max(ukey.shape[0] - 1, 0))] == kkey) if ukey.size else \
        np.zeros(kkey.shape, dtype=bool)
    if not found.all():
        j = int(np.flatnonzero(~found)[0])
        raise AssertionError(f"{case.name}: tile {ktile[j]} lists Gaussian {kgid[j]}, which the reference rect does not put there")
    rank = uo[pos]  # index in the upper list = (tile, reference order)
    bad = np.flatnonzero(np.diff(rank) <= 0)
    if bad.size:
        j = int(bad[0])
        raise AssertionError(f"{case.name}: tile {ktile[j]}: Gaussians {kgid[j]}, {kgid[j + 1]} are repeated or not in the "
                             f"reference's ({tie}) order")
    kept = np.zeros(up.count, dtype=bool)
    kept[rank] = True
    mt, mg = up.tile[~kept], up.gid[~kept]
    if exact:
        assert mt.size == 0, f"{case.name}: {mt.size} pairs of the upper lists are missing, e.g. tile {mt[:1]} Gaussian {mg[:1]}"
    ma = max_alpha(case, mt, mg)
    bad = np.flatnonzero(ma >= 1.0 / 255.0)
    if bad.size:
        j = int(bad[np.argmax(ma[bad])])
        raise AssertionError(f"{case.name}: {bad.size} dropped pairs would have contributed (of {mt.size} dropped, "
                             f"{int(kept.sum())} kept); worst: tile {mt[j]} (x {mt[j] % case.gx}, y {mt[j] // case.gx}) "
                             f"Gaussian {mg[j]} fp64 alpha {ma[j]:.6g}, conic_opacity {case.conic_opacity[mg[j]]}, "
                             f"centre {case.means2D[mg[j]]}, radius {case.radii[mg[j]]}")
    return dict(kept=int(kept.sum()), dropped=int(mt.size), tile=ktile, gid=kgid)


# -------------------------------------------------------------------------------------------------------- the families
def _conic_from_cov(a, b, c):
    """K1's arithmetic in float32: + 0.3 on the diagonal, then the inverse"""
    a, b, c = a.astype(F32) + F32(0.3), b.astype(F32), c.astype(F32) + F32(0.3)
    det = a * c - b * b
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):  # (a det of 0: the caller drops the row)
        inv = F32(1.0) / det
        return c * inv, -b * inv, a * inv, det


def _cov(rng, n, s_major, s_minor):
    th = rng.uniform(0, np.pi, n).astype(F32)
    cs, sn = np.cos(th), np.sin(th)
    l1, l2 = (s_major * s_major).astype(F32), (s_minor * s_minor).astype(F32)
    return cs * cs * l1 + sn * sn * l2, cs * sn * (l1 - l2), sn * sn * l1 + cs * cs * l2


def _ordinary(rng, n, W, H, smax=12.0):
    """ordinary splats: sigma 0.5 .. smax px, any angle, centres up to 20 px outside the frame, opacity 0 .. 1 (some below
    the cut), radius = ceil(3 sigma_major) like K1's"""
    s1 = rng.uniform(0.5, smax, n).astype(F32)
    s2 = (s1 * rng.uniform(0.2, 1.0, n)).astype(F32)
    A, B, C, det = _conic_from_cov(*_cov(rng, n, s1, s2))
    assert (det > 0).all()
    xy = np.stack([rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)], axis=1).astype(F32)
    radii = np.ceil(3.0 * np.sqrt(s1 * s1 + 0.3)).astype(np.int32)
    o = rng.uniform(0.0, 1.0, n).astype(F32)
    depths = rng.uniform(0.5, 20.0, n).astype(F32)
    return xy, depths, radii, np.stack([A, B, C, o], axis=1)


NEEDLE_TRIPLES = [(1, 1, 1), (1, -1, 1), (1e-3, 1e-3, 1e-3), (0, 0, 0), (1, 2, 1), (1e-12, 0, 1e-12)]
NEEDLE_SEED = 0


def _needle_conics(seed, n):
    rng = np.random.default_rng(seed)
    m = 2 * n  # a float32 det of exactly 0 has no inverse (K1 culls such a row): draw spares, keep the first n finite
    s1 = rng.choice(np.array([300.0, 3000.0, 10000.0], dtype=F32), m)
    s2 = rng.uniform(0.0, 0.5, m).astype(F32)
    A, B, C, det = _conic_from_cov(*_cov(rng, m, s1, s2))
    ok = np.flatnonzero(np.isfinite(A) & np.isfinite(B) & np.isfinite(C))[:n]
    assert ok.shape[0] == n
    return A[ok], B[ok], C[ok], rng


@functools.lru_cache(maxsize=None)
def needles():
    W = H = 256
    A, B, C, rng = _needle_conics(NEEDLE_SEED, 1960)
    tri = np.array(NEEDLE_TRIPLES * 6, dtype=F32)  # each explicit triple at six places
    A, B, C = np.concatenate([A, tri[:, 0]]), np.concatenate([B, tri[:, 1]]), np.concatenate([C, tri[:, 2]])
    n = A.shape[0]
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(F32)  # pixel centres inside the frame
    radii = rng.integers(40, 401, n).astype(np.int32)
    co = np.stack([A, B, C, np.full(n, 0.9, dtype=F32)], axis=1)
    depths = rng.uniform(0.5, 50.0, n).astype(F32)
    return (make_case("needles", xy, depths, radii, co, W, H, generated=n - tri.shape[0]),)


def improper(case):
    """float32 A C - B B <= 0, products and difference each rounded (no contraction)"""
    co = case.conic_opacity
    return (co[:, 0] * co[:, 2] - co[:, 1] * co[:, 1]) <= 0


OPACITIES = [np.nextafter(CUT32, F32(0)), CUT32, np.nextafter(CUT32, F32(1)), F32(0.99), F32(1.0), F32(1.5)]


@functools.lru_cache(maxsize=None)
def opacity_cut():
    W, H = 100, 70
    conics = [(0.5, 0.0, 0.5, 6), (0.02, 0.0, 0.02, 22), (0.3, 0.1, 0.05, 14), (4.0, 0.0, 4.0, 2)]
    centres = [(16, 16), (31, 15), (40, 33), (0, 0), (99, 69), (47, 48)]  # pixel centres; tile corners and edges among them
    rows = [(x, y, r, (A, B, C, o)) for o in OPACITIES for (A, B, C, r) in conics for (x, y) in centres]
    xy = np.array([(x, y) for x, y, _, _ in rows], dtype=F32)
    radii = np.array([r for _, _, r, _ in rows], dtype=np.int32)
    co = np.array([c for _, _, _, c in rows], dtype=F32)
    depths = np.random.default_rng(5).uniform(0.5, 9.0, len(rows)).astype(F32)
    return (make_case("opacity_cut", xy, depths, radii, co, W, H, per_opacity=len(conics) * len(centres)),)


def _ulps(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


@functools.lru_cache(maxsize=None)
def borders():
    W, H = 333, 211
    rows = []  # (x, y, radius, sigma)
    for k in (0, 1, 7, 13, 20, 21):
        for r in (1, 5, 37):
            for v in _ulps(16 * k + r):          # x - r = 16 k and one ulp either side
                rows += [(v, 100.0, r, r / 3), (150.0, v, r, r / 3)]
            for v in _ulps(16 * k + 1 - r):      # x + r + 15 = 16 (k + 1) and one ulp either side
                rows += [(v, 100.0, r, r / 3), (150.0, v, r, r / 3)]
        for c in (16 * k, 16 * k - 0.5, 16 * k + 15):
            for r in (1, 7, 16):
                rows += [(c, c * 0.6, r, r / 3), (c * 0.6, c, r, r / 3), (c, c, r, r / 3)]
    for d in (10.0, 10.5, 40.0):                 # off-screen by less and by more than the radius, on all four sides
        for r in (5, 20, 64):
            rows += [(-d, 100.0, r, r / 3), (W - 1 + d, 100.0, r, r / 3), (150.0, -d, r, r / 3), (150.0, H - 1 + d, r, r / 3),
                     (-d, -d, r, r / 3), (W - 1 + d, H - 1 + d, r, r / 3)]
    big = np.iinfo(np.int32).max
    for r in (1, 1 << 20, big):
        for sg in (2.0, 100.0, 1e6):             # (sigma 1e6: conic 1e-12, the extent is millions of pixels)
            rows += [(160.0, 100.0, r, sg), (0.0, 0.0, r, sg), (332.0, 210.0, r, sg), (1e9, 100.0, r, sg), (-1e9, 100.0, r, sg),
                     (150.0, 1e9, r, sg), (150.0, -1e9, r, sg), (1e9, -1e9, r, sg), (-1e6, 100.0, r, sg), (150.0, 1e6, r, sg)]
    x = np.array([t[0] for t in rows], dtype=F32)
    y = np.array([t[1] for t in rows], dtype=F32)
    radii = np.array([t[2] for t in rows], dtype=np.int32)
    sg = np.array([t[3] for t in rows], dtype=np.float64)
    inv = (1.0 / (sg * sg)).astype(F32)
    co = np.stack([inv, np.zeros_like(inv), inv, np.full(inv.shape, 0.9, dtype=F32)], axis=1)
    depths = np.random.default_rng(11).uniform(0.5, 9.0, len(rows)).astype(F32)
    return (make_case("borders", np.stack([x, y], axis=1), depths, radii, co, W, H),)


RECT_SHAPES = [(7, 9), (9, 7), (1, 63), (63, 1), (3, 21), (8, 8), (1, 64), (64, 1), (4, 16), (2, 32), (5, 13), (13, 5),
               (1, 65), (65, 1), (2, 33), (33, 2)]


@functools.lru_cache(maxsize=None)
def rect_sizes():
    """axis-aligned splats whose alpha >= 1/255 box (gsr_alpha_extent: sqrt(2 tau) sigma * 1.01 + 0.5 px), and whose true
    ellipse too, spans exactly w x h tiles: centre 16 t0 + 8 w (a pixel centre), half extent 8 w - 4.5, i.e. 4.5 px inside
    the outermost tiles on both sides -- more than the 1 % + 0.5 px between the two.  The 3-sigma radius covers the frame."""
    W = H = 1040  # 65 x 65 tiles
    o = 0.9
    tau2 = 2.0 * np.log(255.0 * float(F32(o)))
    rows = []
    for (w, h) in RECT_SHAPES:
        for place in (0, 1, 2):  # flush left / top, in the middle, flush right / bottom
            tx = (0, (65 - w) // 2, 65 - w)[place]
            ty = (0, (65 - h) // 2, 65 - h)[(place + 1) % 3]
            sx = (8 * w - 4.5 - 0.5) / (1.01 * np.sqrt(tau2))
            sy = (8 * h - 4.5 - 0.5) / (1.01 * np.sqrt(tau2))
            rows.append((16 * tx + 8 * w, 16 * ty + 8 * h, 1.0 / (sx * sx), 1.0 / (sy * sy), w, h))
    rng = np.random.default_rng(21)
    xy0, d0, r0, co0 = _ordinary(rng, 300, W, H)
    xy = np.concatenate([np.array([(t[0], t[1]) for t in rows], dtype=F32), xy0])
    co = np.concatenate([np.array([(t[2], 0.0, t[3], o) for t in rows], dtype=F32), co0])
    radii = np.concatenate([np.full(len(rows), 4000, dtype=np.int32), r0])
    depths = np.concatenate([rng.uniform(0.5, 20.0, len(rows)).astype(F32), d0])
    shapes = np.array([(t[4], t[5]) for t in rows], dtype=np.int64)
    return (make_case("rect_sizes", xy, depths, radii, co, W, H, shapes=shapes),)


def _covering(n, W, H, depths):
    """n splats that cover every tile: a radius beyond the frame and a conic whose alpha box is wider still"""
    xy = np.array([(W // 2, H // 2), (0, 0), (W - 1, H - 1)], dtype=F32)[np.arange(n) % 3]
    co = np.tile(np.array([1e-9, 0.0, 1e-9, 0.9], dtype=F32), (n, 1))
    return xy, np.asarray(depths, dtype=F32), np.full(n, 8192, dtype=np.int32), co


@functools.lru_cache(maxsize=None)
def whole_frame():
    out = [make_case("whole_frame 4096x4096", *_covering(3, 4096, 4096, [2.0, 1.0, 2.0]), 4096, 4096, exact=True)]
    for W, H in ((4112, 16), (16, 4112), (4096, 16), (1, 1), (15, 15), (17, 17)):
        rng = np.random.default_rng(W * 7 + H)
        a = _covering(3, W, H, [2.0, 1.0, 2.0])
        b = _ordinary(rng, 60, W, H)
        out.append(make_case(f"whole_frame {W}x{H}", *[np.concatenate([u, v]) for u, v in zip(a, b)], W, H))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def masks():
    W, H = 333, 211  # 21 x 14 tiles
    g = _ordinary(np.random.default_rng(31), 3000, W, H)
    gy, gx = 14, 21
    yy, xx = np.mgrid[0:gy, 0:gx]
    one = np.zeros((gy, gx), dtype=bool)
    one[5, 9] = True
    last = np.zeros((gy, gx), dtype=bool)
    last[-1, :] = True
    band = np.zeros((gy, gx), dtype=bool)
    band[3:9, :] = True
    band[4, 2:7] = False
    band[6, :] = False
    band[8, ::3] = False
    ms = [("none", np.zeros((gy, gx), dtype=bool)), ("one tile", one), ("checkerboard", (yy + xx) % 2 == 0),
          ("last row", last), ("band with holes", band), ("all", np.ones((gy, gx), dtype=bool))]
    return tuple(make_case(f"masks {name}", *g, W, H, mask=m) for name, m in ms)


@functools.lru_cache(maxsize=None)
def counts():
    W, H = 200, 120
    out = []
    for P in (1, 63, 64, 65, 4095, 4096, 4097):
        xy, d, r, co = _ordinary(np.random.default_rng(P), P, W, H, smax=6.0)
        xy = np.clip(xy, 0, [W - 1, H - 1]).astype(F32)  # (live: every rect meets the frame)
        co[:, 3] = np.maximum(co[:, 3], F32(0.05))
        out.append(make_case(f"counts P={P}", xy, d, r, co, W, H, live=P))
    xy, d, r, co = _ordinary(np.random.default_rng(77), 500, W, H)
    out.append(make_case("counts all radii 0", xy, d, np.zeros(500, dtype=np.int32), co, W, H, live=0))
    xy, d, r, co = _ordinary(np.random.default_rng(78), 10001, W, H)
    dead = np.arange(10001) != 6789
    xy[dead], d[dead], r[dead], co[dead] = 0, 0, 0, 0  # K1 leaves culled rows all-zero
    xy[6789], r[6789], co[6789] = (100.0, 60.0), 20, (0.02, 0.0, 0.02, 0.8)
    out.append(make_case("counts one live of 10001", xy, d, r, co, W, H, live=1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def depth_keys():
    W, H = 333, 211
    P = 5000
    rng = np.random.default_rng(41)
    xy, _, r, co = _ordinary(rng, P, W, H)
    i = np.arange(P)
    adj = (np.float32(3.0).view(np.uint32) + (rng.integers(0, 3, P)).astype(np.uint32)).view(F32)
    wide = np.exp(rng.uniform(np.log(0.2), np.log(3e38), P)).astype(F32)
    wide[rng.integers(0, P, 40)] = np.inf
    wide[:2] = (0.2, 3e38)
    ds = [("all equal", np.full(P, 1.5, dtype=F32)), ("two values", np.where(i % 2 == 0, 4.0, 2.5).astype(F32)),
          ("adjacent bits", adj), ("0.2 .. 3e38, inf", wide)]
    return tuple(make_case(f"depth_keys {name}", xy, d, r, co, W, H) for name, d in ds)


@functools.lru_cache(maxsize=None)
def long_list():
    rng = np.random.default_rng(51)
    n = 20000  # all on tile (1, 1) of a 64 x 64 frame: centre 19 .. 29, radius 2
    xy = rng.integers(19, 30, (n, 2)).astype(F32)
    co = np.tile(np.array([4.0, 0.0, 4.0, 0.5], dtype=F32), (n, 1))
    d = (rng.integers(0, 4000, n) * 0.01 + 0.5).astype(F32)  # ~5 Gaussians per depth value
    one = make_case("long_list one tile", xy, d, np.full(n, 2, dtype=np.int32), co, 64, 64)
    n = 3000
    xy = rng.integers(0, 256, (n, 2)).astype(F32)
    co = np.tile(np.array([1e-8, 0.0, 1e-8, 0.5], dtype=F32), (n, 1))
    d = (rng.integers(0, 1000, n) * 0.01 + 0.5).astype(F32)
    cover = make_case("long_list whole frame", xy, d, np.full(n, 400, dtype=np.int32), co, 256, 256, exact=True)
    return one, cover


@functools.lru_cache(maxsize=None)
def position_ties():
    W, H = 333, 211
    P = 4000
    rng = np.random.default_rng(61)
    xy, _, r, co = _ordinary(rng, P, W, H)
    xy = np.round(xy * 4) / 4
    run, start, k = np.empty(P, dtype=np.int64), 0, 0
    while start < P:  # depth runs of length 2 .. 32
        n = min(int(rng.integers(2, 33)), P - start)
        if P - start - n == 1:
            n += 1 if n < 32 else -1
        run[start:start + n] = k
        kind = k % 4
        if kind == 1:    # equal x, different y
            xy[start:start + n, 0] = xy[start, 0]
        elif kind == 2:  # fully equal positions (the index decides)
            xy[start:start + n] = xy[start]
        elif kind == 3:  # pairs of equal positions among different ones
            xy[start + 1:start + n:2] = xy[start:start + n - 1:2][:len(xy[start + 1:start + n:2])]
        start, k = start + n, k + 1
    d = (0.5 + 0.01 * rng.permutation(k)[run]).astype(F32)
    p = rng.permutation(P)  # the runs are scattered over the index range
    return (make_case("position_ties", xy[p].astype(F32), d[p], r[p], co[p], W, H, runs=k,
                      longest=int(np.bincount(run).max())),)


FAMILIES = dict(needles=needles, opacity_cut=opacity_cut, borders=borders, rect_sizes=rect_sizes, whole_frame=whole_frame,
                masks=masks, counts=counts, depth_keys=depth_keys, long_list=long_list, position_ties=position_ties)


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]
