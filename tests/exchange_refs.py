"""The contract of the device side of the pixel-partition exchange (csrc/exchange.hip) in plain numpy, and hand-built
input families at the edges of its integer decisions.

No torch and no project code in here.  The inputs are K1's OUTPUTS for a batch of B cameras, given directly (`Case`):
means2D [B,P,2] f32, rgb [B,P,3] f32, conic_opacity [B,P,4] f32, radii [B,P] i32, depths [B,P] f32, and the band table
bands [B,W,2] i32 -- rank g renders the tile rows [lo, hi) of camera k.  Everything the kernels produce is a copy of
input bits or an integer count, so every reference below is EXACT and is kept as int32 bit patterns (a float NaN with a
payload, -0.0 and a denormal are just 32 bits here).

The rule (csrc/common.h gsr_get_rect, SURVEY.md A.2 step 7, then K2): the tile rect of a row is float32 arithmetic,
minimum (p - r) / 16, maximum ((p + r) + 15) / 16, truncated toward zero, clamped to [0, g].  Row i of camera k goes to
rank g iff radius > 0, the rect is non-empty in both axes, hi > lo, and max(lo, miny) < min(hi, maxy).

  need(case)                      bool [W,B,P]
  counts(case, c0, cn)            (chunkcnt int32 [W * cn, chunks], counts int32 [W, cn]) of the cameras [c0, c0 + cn)
  pack(case, k0, nb)              (msg bits int32 [n,11], send_idx int32 [n], segment offsets, segments) in
                                  (destination, camera, row) order
  pack_slab(case, caps, k0, nb)   the same into capacity slabs: records that do not fit dropped, the tail of a slab all
                                  zero bits with send index -1
  unpack(msg)                     the five tensors of the render op
  first_difference(...) / assert_same_message(...)   comparison that names the first wrong row

Limits the families keep, so that every float -> int conversion of the rule is in range on both sides: a non-finite
position only ever comes with radius <= 0 (such a row is culled before its position means anything), and finite
positions stay within +-1e6.
"""
import functools

import numpy as np

BLOCK = 16
XCHUNK = 1024  # rows per chunk of the per-chunk counts (csrc/exchange.hip)
F32 = np.float32
REC = 11  # words of a record: means2D 2, rgb 3, conic_opacity 4, radius bits, depth

# row kinds of the families
IN_FRAME, CULLED, CULLED_NONFINITE, NEGATIVE, CLAMPED_EMPTY, ON_EDGE, HUGE, NAN_RADIUS = range(8)
KIND_NAMES = ["in-frame", "radius 0", "radius 0, non-finite", "radius -5", "empty after the clamp", "edge on a multiple of 16",
              "radius 2^20", "radius with NaN bits"]
MIX = (0.40, 0.10, 0.08, 0.05, 0.12, 0.12, 0.05, 0.08)
NAN_RADII = (0x7F800001, 0x7FC00001)  # int32 radii whose bits read as a float are a signalling / a quiet NaN
# payload specials: -0.0, the smallest and the largest denormal (one negative), +-inf, NaNs with payloads
SPECIAL_BITS = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFA54321, 0x7F800002],
                        dtype=np.uint32).view(np.int32)
NONFINITE_BITS = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0xFFC00abc], dtype=np.uint32).view(np.int32)


class Case:
    """one camera batch (read-only arrays); hashed by identity, so the references are cached per case"""

    def __init__(self, name, means2D, rgb, conic_opacity, radii, depths, bands, width, height, kinds, meta):
        self.name, self.means2D, self.rgb, self.conic_opacity, self.radii, self.depths = \
            name, means2D, rgb, conic_opacity, radii, depths
        self.bands, self.width, self.height, self.kinds, self.meta = bands, int(width), int(height), kinds, meta
        self.B, self.P = radii.shape
        self.W = bands.shape[1]
        assert means2D.shape == (self.B, self.P, 2) and rgb.shape == (self.B, self.P, 3)
        assert conic_opacity.shape == (self.B, self.P, 4) and depths.shape == (self.B, self.P)
        assert bands.shape == (self.B, self.W, 2) and bands.dtype == np.int32 and radii.dtype == np.int32
        for a in (means2D, rgb, conic_opacity, radii, depths, bands, kinds):
            a.setflags(write=False)

    def __repr__(self):
        return self.name

    @property
    def gx(self):
        return (self.width + BLOCK - 1) // BLOCK

    @property
    def gy(self):
        return (self.height + BLOCK - 1) // BLOCK

    @property
    def chunks(self):
        return max((self.P + XCHUNK - 1) // XCHUNK, 1)


# ------------------------------------------------------------------------------------------------------ the contract
def rect(case, k):
    """-> int64 minx, miny, maxx, maxy [P] of camera k, and live [P] = radius > 0.  float32 throughout, truncated toward
    zero, then clamped.  Rows with radius <= 0 are evaluated at (0, 0) with radius 0: their position means nothing."""
    rad = case.radii[k]
    live = rad > 0
    p = np.where(live[:, None], case.means2D[k], F32(0)).astype(F32)
    assert np.isfinite(p).all() and (np.abs(p) <= 1e6).all(), "a live row must have a finite position within +-1e6"
    r = np.where(live, rad, 0).astype(F32)
    b, last = F32(BLOCK), F32(BLOCK - 1)

    def cut(v, g):
        assert v.dtype == F32 and (np.abs(v) < 2.0 ** 31).all()
        return np.clip(np.trunc(v).astype(np.int64), 0, g)

    minx, miny = cut((p[:, 0] - r) / b, case.gx), cut((p[:, 1] - r) / b, case.gy)
    maxx, maxy = cut(((p[:, 0] + r) + last) / b, case.gx), cut(((p[:, 1] + r) + last) / b, case.gy)
    return minx, miny, maxx, maxy, live


@functools.lru_cache(maxsize=None)
def hits(case, k):
    """bool [W,P]: rank g needs row i of camera k"""
    minx, miny, maxx, maxy, live = rect(case, k)
    ok = live & (maxx > minx) & (maxy > miny)
    lo = case.bands[k, :, 0].astype(np.int64)[:, None]
    hi = case.bands[k, :, 1].astype(np.int64)[:, None]
    out = ok[None, :] & (hi > lo) & (np.maximum(lo, miny[None, :]) < np.minimum(hi, maxy[None, :]))
    out.setflags(write=False)
    return out


def need(case):
    return np.stack([hits(case, k) for k in range(case.B)], axis=1)  # [W,B,P]


@functools.lru_cache(maxsize=None)
def counts(case, c0=0, cn=None):
    cn = case.B - c0 if cn is None else cn
    W, n = case.W, case.chunks
    chunkcnt = np.zeros((W * cn, n), dtype=np.int32)
    cnt = np.zeros((W, cn), dtype=np.int32)
    for kk in range(cn):
        h = hits(case, c0 + kk)
        pad = np.zeros((W, n * XCHUNK), dtype=np.int32)
        pad[:, :case.P] = h
        per = pad.reshape(W, n, XCHUNK).sum(2)
        for g in range(W):
            chunkcnt[g * cn + kk] = per[g]
        cnt[:, kk] = h.sum(1)
    return chunkcnt, cnt


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def records(case, k):
    """int32 [P,11]: the record of every row of camera k, as bits"""
    out = np.concatenate([_bits(case.means2D[k]), _bits(case.rgb[k]), _bits(case.conic_opacity[k]),
                          case.radii[k][:, None], _bits(case.depths[k])[:, None]], axis=1)
    assert out.shape == (case.P, REC) and out.dtype == np.int32
    return out


def _segments(case, k0, nb):
    """(destination g, camera kk of the launch, row ids) in message order"""
    for g in range(case.W):
        for kk in range(nb):
            yield g, kk, np.flatnonzero(hits(case, k0 + kk)[g])


@functools.lru_cache(maxsize=None)
def pack(case, k0=0, nb=None):
    """-> (msg int32 [n,11], send_idx int32 [n], offsets list [W * nb], segments list of (g, kk, first, end))"""
    nb = case.B - k0 if nb is None else nb
    msgs, idxs, off, segs, o = [], [], [], [], 0
    for g, kk, ids in _segments(case, k0, nb):
        msgs.append(records(case, k0 + kk)[ids])
        idxs.append((kk * case.P + ids).astype(np.int32))
        off.append(o)
        segs.append((g, kk, o, o + ids.size))
        o += ids.size
    return (np.concatenate(msgs).reshape(-1, REC), np.concatenate(idxs), off, segs)


def pack_slab(case, capacities, k0=0, nb=None):
    """-> (msg int32 [sum caps,11], send_idx int32 [sum caps], segments, stats dict rows sent / segments overflowed /
    padding rows)"""
    nb = case.B - k0 if nb is None else nb
    capacities = [int(c) for c in capacities]
    assert len(capacities) == case.W * nb and min(capacities) >= 0
    n = sum(capacities)
    msg = np.zeros((n, REC), dtype=np.int32)
    idx = np.full((n,), -1, dtype=np.int32)
    segs, o, sent, over = [], 0, 0, 0
    for (g, kk, ids), cap in zip(_segments(case, k0, nb), capacities):
        over += ids.size > cap
        ids = ids[:cap]
        msg[o:o + ids.size] = records(case, k0 + kk)[ids]
        idx[o:o + ids.size] = kk * case.P + ids
        segs.append((g, kk, o, o + cap))
        sent += ids.size
        o += cap
    return msg, idx, segs, dict(sent=sent, overflowed=int(over), padding=n - sent)


def unpack(msg):
    """message bits int32 [n,11] -> bits of means2D [n,2], rgb [n,3], conic_opacity [n,4], radii [n], depths [n]"""
    msg = np.asarray(msg).reshape(-1, REC)
    return (np.ascontiguousarray(msg[:, 0:2]), np.ascontiguousarray(msg[:, 2:5]), np.ascontiguousarray(msg[:, 5:9]),
            np.ascontiguousarray(msg[:, 9]), np.ascontiguousarray(msg[:, 10]))


RELATIONS = ("above", "equal", "below", "no room", "room for nothing", "nothing")


def relation(cap, n):
    """which of the six capacity relations a slab is in"""
    if n > 0:
        return "no room" if cap == 0 else "above" if cap > n else "equal" if cap == n else "below"
    return "room for nothing" if cap > 0 else "nothing"


def mixed_capacities(cnt, salt=0):
    """a slab layout that cycles the segments with rows through below / above / equal / no room and the segments
    without rows through room / no room, from the true counts int [W, nb]"""
    caps, a, b = [], salt, salt
    for n in np.asarray(cnt).reshape(-1).tolist():
        if n > 0:
            caps.append([n // 2, n + 1 + 41 * (a % 7), n, 0][a % 4])
            a += 1
        else:
            caps.append([17, 0][b % 2])
            b += 1
    return caps


# ------------------------------------------------------------------------------------------------------ comparison
def first_difference(want_msg, want_idx, got_msg, got_idx, segments):
    """None when (message bits, send index) agree everywhere; otherwise a sentence that names the first wrong row"""
    want_msg, got_msg = np.asarray(want_msg).reshape(-1, REC), np.asarray(got_msg)
    want_idx, got_idx = np.asarray(want_idx).reshape(-1), np.asarray(got_idx)
    if got_msg.dtype != np.int32 or got_idx.dtype != np.int32:
        return f"the message and the index must be given as int32 bits, got {got_msg.dtype} / {got_idx.dtype}"
    if got_msg.shape != want_msg.shape or got_idx.shape != want_idx.shape:
        return f"shapes: message {got_msg.shape} for {want_msg.shape}, index {got_idx.shape} for {want_idx.shape}"
    bad_row = (want_msg != got_msg).any(1) | (want_idx != got_idx)
    if not bad_row.any():
        return None
    r = int(np.argmax(bad_row))
    where = "outside every segment"
    for g, kk, first, end in segments:
        if first <= r < end:
            where = f"segment (destination {g}, camera {kk}) rows [{first}, {end}), position {r - first}"
            break
    if want_idx[r] != got_idx[r]:
        what = f"send index: expected {int(want_idx[r])}, found {int(got_idx[r])}"
    else:
        c = int(np.argmax(want_msg[r] != got_msg[r]))
        what = f"column {c}: expected bits 0x{int(want_msg[r, c]) & 0xFFFFFFFF:08x}, found 0x{int(got_msg[r, c]) & 0xFFFFFFFF:08x}"
    return f"row {r} of {want_idx.size} ({int(bad_row.sum())} wrong rows), {where}, {what}"


def assert_same_message(want_msg, want_idx, got_msg, got_idx, segments, label=""):
    d = first_difference(want_msg, want_idx, got_msg, got_idx, segments)
    assert d is None, f"{label}: {d}"


def assert_same_ints(want, got, label=""):
    """integer arrays (counts, chunk counts, masks, unpacked tensors): equal everywhere, or the first wrong element"""
    want, got = np.asarray(want), np.asarray(got)
    assert want.shape == got.shape, f"{label}: shape {got.shape} for {want.shape}"
    bad = want != got
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} wrong elements, first at {at}: expected {int(want[at])}, "
                             f"found {int(got[at])}")


# ------------------------------------------------------------------------------------------------------ the families
def _payload(rng, n, words, nonfinite_rows):
    bits = rng.standard_normal((n, words)).astype(F32).view(np.int32).copy()
    special = rng.random((n, words)) < 0.12
    bits[special] = SPECIAL_BITS[rng.integers(0, SPECIAL_BITS.size, int(special.sum()))]
    m = int(nonfinite_rows.sum())
    bits[nonfinite_rows] = NONFINITE_BITS[rng.integers(0, NONFINITE_BITS.size, (m, words))]
    return bits


def _camera_rows(rng, P, width, height, mix):
    """one camera's rows: kinds [P], means2D bits [P,2], radii [P], payload bits [P,8]"""
    gx, gy = (width + BLOCK - 1) // BLOCK, (height + BLOCK - 1) // BLOCK
    kind = rng.choice(len(mix), size=P, p=mix)
    kind[0] = IN_FRAME
    kind[P - 1] = HUGE  # the last row goes everywhere: a lane past P that re-read it and kept it would show
    x = (rng.random(P) * (width * 1.2) - 20.0).astype(F32)
    y = (rng.random(P) * min(height * 1.2, 1e6) - 20.0).astype(F32)
    below_fits = gy * BLOCK + 59 + 1000 <= 1e6  # (a frame taller than the +-1e6 limit has no room below it)
    rad = rng.integers(1, 60, P).astype(np.int32)
    r = rad.astype(F32)
    u = (rng.random(P) * 1000.0).astype(F32)
    # empty after the clamp: the whole rect left of, right of, above or below the grid (x + r <= 0 gives maxx = 0)
    side = rng.integers(0, 4, P)
    ce = kind == CLAMPED_EMPTY
    x = np.where(ce & (side == 0), -r - u, x)
    x = np.where(ce & (side == 1), F32(gx * BLOCK) + r + u, x)
    y = np.where(ce & (side == 2), -r - u, y)
    y = np.where(ce & (side == 3), F32(gy * BLOCK) + r + u if below_fits else -r - u, y)
    # an edge of the row interval exactly on a multiple of 16 (small integers: every sum is exact), and one ulp either side
    m = rng.integers(0, min(gy, 62000) + 1, P).astype(F32) * F32(BLOCK)
    edge = np.where(rng.random(P) < 0.5, m + r, m - F32(BLOCK - 1) - r).astype(F32)
    nudge = rng.integers(0, 3, P)
    edge = np.where(nudge == 1, np.nextafter(edge, F32(-np.inf)), np.where(nudge == 2, np.nextafter(edge, F32(np.inf)), edge))
    y = np.where(kind == ON_EDGE, edge, y).astype(F32)
    # far rows: anywhere within +-1e6
    far = (kind == HUGE) | (kind == NAN_RADIUS)
    spread = rng.random(P) < 0.5
    x = np.where(far & spread, (rng.random(P) * 2e6 - 1e6), x).astype(F32)
    y = np.where(far & spread, (rng.random(P) * 2e6 - 1e6), y).astype(F32)
    rad = np.where(kind == HUGE, 1 << 20, rad)
    rad = np.where(kind == NAN_RADIUS, np.array(NAN_RADII, dtype=np.int64)[rng.integers(0, 2, P)], rad)
    rad = np.where((kind == CULLED) | (kind == CULLED_NONFINITE), 0, rad)
    rad = np.where(kind == NEGATIVE, -5, rad).astype(np.int32)
    m2 = np.stack([x, y], axis=1).astype(F32).view(np.int32).copy()
    nf = kind == CULLED_NONFINITE
    n_nf = int(nf.sum())
    bad = NONFINITE_BITS[rng.integers(0, NONFINITE_BITS.size, (n_nf, 2))]
    keep_one = rng.integers(0, 3, n_nf)  # 0: both coordinates non-finite, 1: only x, 2: only y
    cur = m2[nf]
    cur[:, 0] = np.where(keep_one != 2, bad[:, 0], cur[:, 0])
    cur[:, 1] = np.where(keep_one != 1, bad[:, 1], cur[:, 1])
    m2[nf] = cur
    return kind.astype(np.int8), m2, rad, _payload(rng, P, 8, nf)


def _cut_rows(rng, gy, m):
    inner = np.sort(rng.choice(np.arange(1, gy), size=m - 1, replace=False)) if m > 1 else np.array([], dtype=np.int64)
    return [0] + inner.tolist() + [gy]


BAND_KINDS = ("cut", "nothing", "empty", "reversed", "beyond", "same rows", "everything", "inside")


def band_table(rng, B, W, gy, styles):
    """bands int32 [B,W,2] and the set of band kinds it holds.  One style per camera, in turn:
    partition: random cuts of the tile rows into W bands, one per rank in a random order;
    cuts     : random cuts into fewer bands handed to a random subset of the ranks; the other ranks get, in turn,
               (0, 0), an empty band lo == hi > 0, a reversed band and a band with lo >= gy;
    overlap  : two ranks render the same rows, the others random intervals;
    specials : one rank renders everything, the others get the empty / reversed / beyond bands in turn;
    nested   : one rank renders everything, the others random intervals inside."""
    bands = np.zeros((B, W, 2), dtype=np.int32)
    seen, turn = set(), 0

    def odd_one(t):
        c = int(rng.integers(1, gy + 1))
        return [("nothing", (0, 0)), ("empty", (c, c)), ("reversed", (min(c + 3, gy), max(c - 2, 0))),
                ("beyond", (gy + (t % 2) * 3, gy + 5 + (t % 2) * 4))][t % 4]

    def interval():
        a = int(rng.integers(0, gy))
        return a, int(rng.integers(a + 1, gy + 1))

    for k in range(B):
        style = styles[k % len(styles)]
        order = rng.permutation(W)
        if style in ("partition", "cuts"):
            m = min(W, gy) if style == "partition" else int(rng.integers(min(2, W), min(W, gy) + 1))
            assert style == "cuts" or m == W, "a partition needs a tile row per rank"
            cuts = _cut_rows(rng, gy, m)
            for j in range(m):
                bands[k, order[j]] = cuts[j], cuts[j + 1]
            seen.add("cut")
            for g in order[m:]:
                name, rows = odd_one(turn)
                turn += 1
                bands[k, g] = rows
                seen.add(name)
        elif style == "overlap":
            rows = interval()
            for j, g in enumerate(order):
                bands[k, g] = rows if j < 2 else interval()
            seen.add("same rows" if W > 1 else "inside")
        elif style in ("specials", "nested"):
            bands[k, order[0]] = 0, gy
            seen.add("everything")
            for g in order[1:]:
                if style == "nested":
                    bands[k, g] = interval()
                    seen.add("inside")
                else:
                    name, rows = odd_one(turn + 1)  # (0, 0) comes last here
                    turn += 1
                    bands[k, g] = rows
                    seen.add(name)
        else:
            raise ValueError(style)
    return bands, seen


def make_case(name, seed, P, B, W, width, height, styles, mix=MIX, **meta):
    rng = np.random.default_rng(seed)
    gy = (height + BLOCK - 1) // BLOCK
    rows = [_camera_rows(rng, P, width, height, mix) for _ in range(B)]
    kinds = np.stack([r[0] for r in rows])
    m2 = np.stack([r[1] for r in rows]).view(F32)
    radii = np.stack([r[2] for r in rows]).astype(np.int32)
    pay = np.stack([r[3] for r in rows])
    bands, band_kinds = band_table(rng, B, W, gy, styles)
    return Case(name, m2, np.ascontiguousarray(pay[:, :, 0:3]).view(F32), np.ascontiguousarray(pay[:, :, 3:7]).view(F32),
                radii, np.ascontiguousarray(pay[:, :, 7]).view(F32), bands, width, height, kinds,
                dict(meta, band_kinds=band_kinds, styles=tuple(styles)))


SMALL_P = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
# (count_first, count_cameras) -> the (k0, nb) packed from that count
SUBRANGES = {(0, 5): ((0, 5), (2, 2), (4, 1)), (1, 3): ((2, 1), (1, 3))}
MANY_CHUNKS_P = 1024 * 1025 + 1


@functools.lru_cache(maxsize=None)
def small_p():
    """wave round and chunk edges of the row count: the last, partly filled round and chunk"""
    return tuple(make_case(f"small_p[{P}]", 100 + P, P, 2, 3, 160, 96, ("cuts", "specials")) for P in SMALL_P)


@functools.lru_cache(maxsize=None)
def segment_limit():
    """W x B = 512 segments, the most the ABI takes: the last offset word, and all four position registers of the pack"""
    return (make_case("segment_limit", 256, 3000, 2, 256, 320, 4100, ("partition", "cuts")),)


@functools.lru_cache(maxsize=None)
def wide_w():
    """200 destinations: the fourth position register of the pack partly used (the ragged block of eight destinations is
    the small families', W = 3)"""
    return (make_case("wide_w", 200, 3000, 2, 200, 320, 4100, ("partition", "cuts")),)


@functools.lru_cache(maxsize=None)
def camera_subranges():
    """packs of camera sub-ranges out of one count, and a count that does not start at camera 0"""
    return (make_case("camera_subranges", 5, 2500, 5, 2, 320, 200, ("cuts", "specials", "overlap", "specials", "specials"),
                      subranges=SUBRANGES),)


@functools.lru_cache(maxsize=None)
def many_chunks():
    """1026 chunks: the second trip of the sum kernel (1024 chunks a trip) and of the pack's prefix loop"""
    mix = (0.30, 0.30, 0.08, 0.05, 0.10, 0.10, 0.03, 0.04)
    return (make_case("many_chunks", 1026, MANY_CHUNKS_P, 1, 2, 640, 360, ("nested",), mix=mix),)


@functools.lru_cache(maxsize=None)
def slab_layouts():
    """every relation between a slab's capacity and its count, in one layout, and the all-zero layout"""
    return (make_case("slab_layouts", 7000, 7000, 2, 3, 640, 360, ("cuts", "specials")),)


@functools.lru_cache(maxsize=None)
def tall_frame():
    """65535 tile rows, the most the count and pack kernels take: a row interval that fills its 16 + 16 bits"""
    return (make_case("tall_frame", 65535, 700, 1, 3, 64, 65535 * BLOCK, ("cuts",)),)


def slab_capacities(case):
    """{layout name: capacities} of the slab family: all six relations in one layout, each of above / equal / below
    alone, and all zero"""
    cnt = counts(case)[1].reshape(-1).tolist()
    return {"mixed": mixed_capacities(cnt), "above": [n + 200 for n in cnt], "equal": list(cnt),
            "below": [max(n - 37, 0) for n in cnt], "zero": [0] * len(cnt)}


FAMILIES = dict(small_p=small_p, segment_limit=segment_limit, wide_w=wide_w, camera_subranges=camera_subranges,
                many_chunks=many_chunks, slab_layouts=slab_layouts, tall_frame=tall_frame)


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]


def launches(case):
    """[(count_first, count_cameras, [(k0, nb), ...])]: the counts to run on a case and the packs to run from each"""
    sub = case.meta.get("subranges")
    if sub:
        return [(c0, cn, list(packs)) for (c0, cn), packs in sub.items()]
    return [(0, case.B, [(0, case.B)])]


# ------------------------------------------------------------------------------------------------------ the lattice of the KNN check
def lattice(nx, ny, nz, seed=0):
    """a shuffled lattice of points (i - 7, 2 j + 3, 4 k - 11): every coordinate and every squared distance is an exact
    float32.  In the interior of x the three nearest other points are at squared distance 1, 1 (x - 1, x + 1) and 4 (two
    steps in x or one in y): mean 2.0.  On the x-boundary there is one neighbour at 1 and the next two are at 4: mean
    3.0.  A step in z is 16 away.  -> (points f32 [n,3], expected f32 [n])"""
    assert nx >= 3 and ny >= 2 and nz >= 2
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    pts = np.stack([i - 7, 2 * j + 3, 4 * k - 11], axis=-1).reshape(-1, 3).astype(F32)
    want = np.where((i == 0) | (i == nx - 1), F32(3.0), F32(2.0)).reshape(-1).astype(F32)
    perm = np.random.default_rng(seed).permutation(pts.shape[0])
    return np.ascontiguousarray(pts[perm]), np.ascontiguousarray(want[perm])
