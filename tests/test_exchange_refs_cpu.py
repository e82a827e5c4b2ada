"""CPU checks of tests/exchange_refs.py: the numpy statement of the exchange agrees with the repository's torch
restatement (oracle/exchange_oracle.py) on every family, every family does what it is for, the comparison helpers see a
message that is wrong in one place, and the entry points refuse what the header says they refuse (nothing is launched)."""
import numpy as np
import pytest
import torch

import exchange_refs as R
from oracle import cref as C
from oracle import exchange_oracle as XO

CASES = R.all_cases()
BY_NAME = {c.name: c for c in CASES}


def _f32(a):
    """float32 array -> torch tensor with the same bits (a NaN payload survives: the bytes are moved as integers)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).view(torch.float32)


def _i32(t):
    t = t.contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).numpy()


def _torch_inputs(case):
    return (_f32(case.means2D), _f32(case.rgb), _f32(case.conic_opacity), torch.from_numpy(case.radii.copy()),
            _f32(case.depths), torch.from_numpy(case.bands.copy()))


# ------------------------------------------------------------------------------------------------ oracle agreement
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_numpy_statement_equals_the_torch_oracle(case):
    m2, rgb, co, radii, depths, bands = _torch_inputs(case)
    w, h = case.width, case.height
    for c0, cn, packs in R.launches(case):
        cc, cnt = R.counts(case, c0, cn)
        cc_o, cnt_o = XO.exchange_count(m2, radii, bands, c0, cn, w, h)
        R.assert_same_ints(cnt, cnt_o.numpy(), f"{case} counts [{c0}, {c0 + cn})")
        R.assert_same_ints(cc, cc_o.numpy(), f"{case} chunk counts [{c0}, {c0 + cn})")
        for k0, nb in packs:
            msg, idx, off, segs = R.pack(case, k0, nb)
            msg_o, idx_o = XO.exchange_pack(m2, rgb, co, radii, depths, bands, None, off, idx.size, k0, nb, w, h)
            R.assert_same_message(msg, idx, _i32(msg_o), idx_o.numpy(), segs, f"{case} pack ({k0}, {nb})")
            caps = R.mixed_capacities(R.counts(case, k0, nb)[1], salt=k0)
            smsg, sidx, ssegs, _ = R.pack_slab(case, caps, k0, nb)
            smsg_o, sidx_o = XO.exchange_pack_slab(m2, rgb, co, radii, depths, bands, None, None, caps, k0, nb, w, h)
            R.assert_same_message(smsg, sidx, _i32(smsg_o), sidx_o.numpy(), ssegs, f"{case} slab ({k0}, {nb})")
            for name, a, b in zip(("means2D", "rgb", "conic_opacity", "radii", "depths"), R.unpack(smsg),
                                  XO.exchange_unpack(smsg_o)):
                R.assert_same_ints(a, _i32(b).reshape(a.shape), f"{case} unpack {name}")


def test_slab_family_layouts_equal_the_torch_oracle():
    case = R.slab_layouts()[0]
    m2, rgb, co, radii, depths, bands = _torch_inputs(case)
    for name, caps in R.slab_capacities(case).items():
        smsg, sidx, ssegs, _ = R.pack_slab(case, caps)
        smsg_o, sidx_o = XO.exchange_pack_slab(m2, rgb, co, radii, depths, bands, None, None, caps, 0, case.B, case.width,
                                               case.height)
        R.assert_same_message(smsg, sidx, _i32(smsg_o), sidx_o.numpy(), ssegs, f"slab layout {name}")


def test_need_mask_sums_to_the_counts():
    for case in CASES:
        need = R.need(case)
        assert need.shape == (case.W, case.B, case.P)
        R.assert_same_ints(R.counts(case)[1], need.sum(2), f"{case}")


# ------------------------------------------------------------------------------------------------ family conditions
def test_families_have_the_stated_shapes():
    shapes = {c.name: (c.P, c.B, c.W, c.width, c.height) for c in CASES}
    for P in (1, 63, 64, 65, 1023, 1024, 1025, 4097):
        assert shapes[f"small_p[{P}]"] == (P, 2, 3, 160, 96)
    assert shapes["segment_limit"] == (3000, 2, 256, 320, 4100) and 256 * 2 == 512
    assert shapes["wide_w"] == (3000, 2, 200, 320, 4100)
    assert shapes["camera_subranges"] == (2500, 5, 2, 320, 200)
    assert shapes["many_chunks"] == (1024 * 1025 + 1, 1, 2, 640, 360)
    assert shapes["slab_layouts"] == (7000, 2, 3, 640, 360)
    assert shapes["tall_frame"][4] == 65535 * 16 and BY_NAME["tall_frame"].gy == 65535
    assert BY_NAME["camera_subranges"].meta["subranges"] == {(0, 5): ((0, 5), (2, 2), (4, 1)), (1, 3): ((2, 1), (1, 3))}


@pytest.mark.parametrize("name,W", [("segment_limit", 256), ("wide_w", 200)])
def test_every_destination_of_the_wide_families_receives_rows(name, W):
    case = BY_NAME[name]
    cnt = R.counts(case)[1]
    assert cnt.shape == (W, 2) and int((cnt.sum(1) > 0).sum()) == W
    assert (cnt[:, 0] > 0).all(), "camera 0 is a partition into W bands: every rank has rows of it"
    if W == 256:  # the last offset word, off[512], is the end of a segment that holds rows
        assert R.pack(case)[3][-1][0:2] == (255, 1)


def test_row_kinds_and_band_kinds_are_all_there():
    for case in CASES:
        if case.P >= 1023:
            assert set(np.unique(case.kinds).tolist()) == set(range(8)), case
    seen = set()
    for case in CASES:
        seen |= case.meta["band_kinds"]
    assert seen == set(R.BAND_KINDS)
    # said of the tables themselves, not of the generator's labels
    gy = {c.name: c.gy for c in CASES}
    lo = lambda c: c.bands[:, :, 0]  # noqa: E731
    hi = lambda c: c.bands[:, :, 1]  # noqa: E731
    assert any(((lo(c) == hi(c)) & (lo(c) > 0)).any() for c in CASES), "an empty band"
    assert any((hi(c) < lo(c)).any() for c in CASES), "a reversed band"
    assert any(((lo(c) >= gy[c.name]) & (hi(c) > lo(c))).any() for c in CASES), "a band beyond the grid"
    assert any(((lo(c) == 0) & (hi(c) == gy[c.name])).any() for c in CASES), "one rank with everything"
    same = False
    for c in CASES:
        for k in range(c.B):
            rows = [tuple(b) for b in c.bands[k].tolist() if b[1] > b[0]]
            same |= len(set(rows)) < len(rows)
    assert same, "two ranks with the same rows"


def test_rows_on_the_edges_of_the_rule():
    """the kinds are what they say: clamped-empty rows have radius > 0 and an empty rect on each of the four sides,
    edge rows put y - r or y + r + 15 exactly on a multiple of 16"""
    case = BY_NAME["slab_layouts"]
    sides = set()
    for k in range(case.B):
        minx, miny, maxx, maxy, live = R.rect(case, k)
        ce = case.kinds[k] == R.CLAMPED_EMPTY
        assert live[ce].all() and ((maxx[ce] == minx[ce]) | (maxy[ce] == miny[ce])).all()
        x, y = case.means2D[k][ce, 0], case.means2D[k][ce, 1]
        sides |= {s for s, m in (("left", x < 0), ("right", x > case.width), ("above", y < 0), ("below", y > case.height))
                  if (m & ((maxx[ce] == minx[ce]) | (maxy[ce] == miny[ce]))).any()}
        e = case.kinds[k] == R.ON_EDGE
        y, r = case.means2D[k][e, 1].astype(np.float64), case.radii[k][e].astype(np.float64)
        assert int((((y - r) % 16 == 0) | ((y + r + 15) % 16 == 0)).sum()) >= e.sum() // 4
    assert sides == {"left", "right", "above", "below"}


def test_count_offset_family_cannot_pass_with_a_wrong_camera():
    """chunk counts of camera j and of camera count_first + j differ, destination by destination, so a pack that read
    chunkcnt at the camera of the batch instead of the camera of the count (or the reverse) writes to the wrong rows"""
    case = BY_NAME["camera_subranges"]
    assert case.chunks == 3
    cc_all = R.counts(case, 0, 5)[0].reshape(case.W, 5, case.chunks)
    cc_sub = R.counts(case, 1, 3)[0].reshape(case.W, 3, case.chunks)
    for j in range(3):
        R.assert_same_ints(cc_all[:, 1 + j], cc_sub[:, j], "a count over [1, 4) is the rows of the count over [0, 5)")
        assert (cc_all[:, j, :-1] != cc_sub[:, j, :-1]).any(), j  # (the prefix the pack forms skips the last chunk)
    # camera kk of a pack of [k0, k0 + nb) reads row k0 - count_first + kk of the count; the rows a wrong offset would read
    # instead (kk: the offset forgotten; k0 + kk: count_first forgotten) hold other numbers
    checked = {}
    for (c0, cn), packs in R.SUBRANGES.items():
        cc = {0: cc_all, 1: cc_sub}[c0]
        for k0, nb in packs:
            for kk in range(nb):
                right = k0 - c0 + kk
                for wrong in {kk, k0 + kk} - {right}:
                    if wrong < cn:
                        assert (cc[:, right, :-1] != cc[:, wrong, :-1]).any(), (c0, cn, k0, kk, wrong)
                        checked[(c0, cn)] = checked.get((c0, cn), 0) + 1
    assert checked[(0, 5)] >= 3 and checked[(1, 3)] >= 3, checked


def test_slab_family_contains_all_six_relations():
    case = BY_NAME["slab_layouts"]
    cnt = R.counts(case)[1].reshape(-1).tolist()
    layouts = R.slab_capacities(case)
    assert {R.relation(c, n) for c, n in zip(layouts["mixed"], cnt)} == set(R.RELATIONS)
    assert set(layouts["zero"]) == {0} and sum(cnt) > 0
    for name in ("above", "equal", "below"):
        assert {R.relation(c, n) for c, n in zip(layouts[name], cnt) if n > 0} == {name}
    # every other family's mixed layout overflows somewhere and pads somewhere
    for c in CASES:
        if c.P >= 63:
            _, _, _, stats = R.pack_slab(c, R.mixed_capacities(R.counts(c)[1]))
            assert stats["overflowed"] > 0 and stats["padding"] > 0 and stats["sent"] > 0, (c, stats)


def test_no_culled_and_no_nonfinite_row_is_ever_sent():
    nan_radius_rows = 0
    for case in CASES:
        for k in range(case.B):
            sent = R.hits(case, k).any(0)
            assert (case.radii[k][sent] > 0).all(), case
            assert np.isfinite(case.means2D[k][sent]).all(), case
            nf = ~np.isfinite(case.means2D[k]).all(1)
            assert (case.radii[k][nf] <= 0).all() and not sent[nf].any(), case
            assert (np.abs(case.means2D[k][~nf]) <= 1e6).all(), case
            if case.P >= 1023:
                assert nf.any() and (case.radii[k] == -5).any() and (case.radii[k] == 0).any()
        msg = R.pack(case)[0]
        for bits in R.NAN_RADII:
            n = int((msg[:, 9] == bits).sum())
            nan_radius_rows += n
            if case.P >= 1023:
                assert n > 0, (case, hex(bits))
                assert np.isnan(np.array([bits], dtype=np.int32).view(np.float32)[0])
    assert nan_radius_rows > 0


def test_the_torch_oracle_keeps_the_bits_of_a_nan_radius_and_of_the_payload():
    case = BY_NAME["small_p[1025]"]
    m2, rgb, co, radii, depths, bands = _torch_inputs(case)
    msg, idx, off, segs = R.pack(case)
    msg_o, _ = XO.exchange_pack(m2, rgb, co, radii, depths, bands, None, off, idx.size, 0, case.B, case.width, case.height)
    got = _i32(msg_o)
    assert (got[:, 9] == 0x7F800001).any() and (got[:, 9] == 0x7FC00001).any()
    for bits in R.SPECIAL_BITS.tolist():
        assert (got[:, 2:9] == bits).any() and (msg[:, 2:9] == bits).any(), hex(bits & 0xFFFFFFFF)


def test_many_chunks_family_reaches_the_second_trip():
    case = BY_NAME["many_chunks"]
    cc, cnt = R.counts(case)
    assert case.chunks == 1026 and cc.shape == (2, 1026)
    assert (cc[:, 64:] > 0).all() and (cc[:, 1024:] > 0).all(), "every chunk of every destination holds rows"
    assert cc[:, 1025].tolist() == [1, 1], "the last chunk is the one row past 1025 full chunks, and it goes everywhere"
    assert int(cnt.sum()) == int(cc.sum())


# ------------------------------------------------------------------------------------------------ helper sensitivity
def _slab_with_padding_and_overflow():
    case = BY_NAME["slab_layouts"]
    caps = R.slab_capacities(case)["mixed"]
    return (case, caps) + R.pack_slab(case, caps)


def test_helpers_accept_the_reference_and_name_a_wrong_row():
    case = BY_NAME["slab_layouts"]
    msg, idx, off, segs = R.pack(case)
    assert R.first_difference(msg, idx, msg.copy(), idx.copy(), segs) is None
    g, kk, first, end = next(s for s in segs if s[3] - s[2] >= 10)
    # two rows of one segment swapped
    m, i = msg.copy(), idx.copy()
    m[[first + 3, first + 4]], i[[first + 3, first + 4]] = m[[first + 4, first + 3]], i[[first + 4, first + 3]]
    d = R.first_difference(msg, idx, m, i, segs)
    assert d is not None and f"destination {g}, camera {kk}" in d and "position 3" in d and "2 wrong rows" in d, d
    # one send index off by one
    i = idx.copy()
    i[end - 1] += 1
    d = R.first_difference(msg, idx, msg.copy(), i, segs)
    assert d is not None and f"position {end - 1 - first}" in d and "send index" in d and str(int(idx[end - 1])) in d, d
    # one bit of one radius
    m = msg.copy()
    m[first + 7, 9] ^= 1 << 22
    d = R.first_difference(msg, idx, m, idx.copy(), segs)
    assert d is not None and "position 7" in d and "column 9" in d and "1 wrong rows" in d, d
    assert f"0x{int(msg[first + 7, 9]) & 0xFFFFFFFF:08x}" in d and f"0x{int(m[first + 7, 9]) & 0xFFFFFFFF:08x}" in d
    with pytest.raises(AssertionError, match="column 9"):
        R.assert_same_message(msg, idx, m, idx.copy(), segs, "x")
    # the sign of a zero, seen only as bits
    m = msg.copy()
    r, c = np.argwhere(msg[:, 2:9] == np.int32(-2 ** 31))[0]
    m[r, 2 + c] = 0
    assert R.first_difference(msg, idx, m, idx.copy(), segs) is not None
    assert R.first_difference(msg, idx, msg.view(np.float32), idx, segs) is not None  # floats are not accepted


def test_helpers_see_wrong_padding_and_a_kept_overflow():
    case, caps, msg, idx, segs, stats = _slab_with_padding_and_overflow()
    assert stats["overflowed"] > 0 and stats["padding"] > 0
    cnt = R.counts(case)[1].reshape(-1).tolist()
    # a padding row with index 0 in place of -1
    s = next(j for j, (c, n) in enumerate(zip(caps, cnt)) if c > n)
    g, kk, first, end = segs[s]
    i = idx.copy()
    assert i[end - 1] == -1 and (msg[end - 1] == 0).all()
    i[end - 1] = 0
    d = R.first_difference(msg, idx, msg.copy(), i, segs)
    assert d is not None and "expected -1, found 0" in d and f"destination {g}, camera {kk}" in d, d
    # a record that overflowed a slab kept instead of dropped: it lands on the first row of the next slab
    s = next(j for j, (c, n) in enumerate(zip(caps, cnt)) if 0 < c < n and j + 1 < len(caps) and caps[j + 1] > 0)
    g, kk, first, end = segs[s]
    ids = np.flatnonzero(R.hits(case, kk)[g])
    m, i = msg.copy(), idx.copy()
    m[end] = R.records(case, kk)[ids[caps[s]]]
    i[end] = kk * case.P + ids[caps[s]]
    d = R.first_difference(msg, idx, m, i, segs)
    assert d is not None and f"row {end} " in d and "position 0" in d, d
    with pytest.raises(AssertionError):
        R.assert_same_ints(np.arange(6).reshape(2, 3), np.array([[0, 1, 2], [3, 9, 5]]), "x")


# ------------------------------------------------------------------------------------------------ refused calls
def test_exchange_entry_points_refuse_a_frame_of_more_than_65535_tile_rows():
    """dummy non-zero integers stand for device pointers: every call below is refused, or returns, before anything is
    dereferenced on the device or launched.  (The height that gsr_exchange_count accepts cannot be told from the refusal
    here, its next check answers the same; tests/test_gpu_exchange_edges.py runs it at 65535 tile rows.)"""
    import ctypes

    import diff_gaussian_rasterization as dgr

    lib, d = dgr._lib.lib, 0x1000
    ok, tall = 65535 * 16, 65536 * 16
    assert lib.gsr_exchange_count(10, 1, 0, 1, 2, 64, tall, d, d, d, d, d, None) == -1
    assert lib.gsr_exchange_count(10, 1, 0, 1, 2, 64, 2 ** 31 - 1, d, d, d, d, d, None) == -1
    zeros = (ctypes.c_int32 * 2)(0, 0)
    # pack: a message of no rows returns before anything else is looked at -- but not for a frame that tall
    assert lib.gsr_exchange_pack(10, 1, 0, 1, 2, 64, ok, 1, 0, d, d, d, d, d, d, d, zeros, 0, d, d, None) == 0
    assert lib.gsr_exchange_pack(10, 1, 0, 1, 2, 64, tall, 1, 0, d, d, d, d, d, d, d, zeros, 0, d, d, None) == -1
    assert lib.gsr_exchange_pack(10, 1, 0, 1, 2, 64, tall, 1, 0, d, d, d, d, d, d, d, zeros, 5, d, d, None) == -1
    # slab: capacities that sum to no rows pass every check and return
    assert lib.gsr_exchange_pack_slab(10, 1, 0, 1, 2, 64, ok, 1, 0, d, d, d, d, d, d, d, d, zeros, 0, d, d, None) == 0
    assert lib.gsr_exchange_pack_slab(10, 1, 0, 1, 2, 64, tall, 1, 0, d, d, d, d, d, d, d, d, zeros, 0, d, d, None) == -1
    ones = (ctypes.c_int32 * 2)(3, 2)
    assert lib.gsr_exchange_pack_slab(10, 1, 0, 1, 2, 64, tall, 1, 0, d, d, d, d, d, d, d, d, ones, 5, d, d, None) == -1


def test_exchange_unpack_refuses_misaligned_outputs():
    import diff_gaussian_rasterization as dgr

    lib, d = dgr._lib.lib, 0x1000
    assert lib.gsr_exchange_unpack(0, d, d, d, d + 4, d, d, None) == 0  # nothing to do: nothing looked at
    assert lib.gsr_exchange_unpack(-1, d, d, d, d, d, d, None) == -1
    for off in (4, 8, 12):
        assert lib.gsr_exchange_unpack(5, d, d, d, d + off, d, d, None) == -1, off  # conic_opacity: 16 bytes
    assert lib.gsr_exchange_unpack(5, d, d + 4, d, d, d, d, None) == -1  # means2D: 8 bytes
    assert lib.gsr_exchange_unpack(5, d, d + 12, d, d, d, d, None) == -1
    assert lib.gsr_exchange_unpack(5, None, d, d, d, d, d, None) == -1


def test_the_header_states_the_tile_row_limit():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "gsraster.h")).read().split())
    assert "more than 65535 tile rows" in text and "GSR_EINVAL for a frame" in text


# ------------------------------------------------------------------------------------------------ the KNN lattice
@pytest.mark.parametrize("shape", [(3, 2, 2), (7, 5, 4), (40, 33, 21)])
def test_lattice_closed_form_is_the_brute_force_answer(shape):
    pts, want = R.lattice(*shape, seed=sum(shape))
    assert set(np.unique(want).tolist()) == {2.0, 3.0}
    got = C.knn_mean_dist2(torch.from_numpy(pts)).numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
