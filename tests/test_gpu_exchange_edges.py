"""-m gpu: the device side of the exchange (csrc/exchange.hip) on the hand-built families of tests/exchange_refs.py, every
record, index and count against the exact numpy statement there -- bit for bit, all rows, nothing excluded -- and the
small kernels that decide whether a captured replay counts (capacity check, flag, publish, band mask) against their truth
tables.  The only comparison with a tolerance is the float32 sum of gsr_scatter_add_rows, held to the textbook bound.

The entry points are called directly, on outputs filled with a sentinel (NaN message, index -7), so that a row the
kernels did not write is seen."""
import ctypes

import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import exchange_refs as R

pytestmark = pytest.mark.gpu

lib, _p, _s = dgr.lib, dgr._ptr, dgr._stream
CASES = R.all_cases()
_DEVICE_INPUTS = {}


def _f32(a, device):
    """float32 array -> device tensor with the same bits (moved as integers)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(device).view(torch.float32)


def _inputs(case, device):
    if case.name not in _DEVICE_INPUTS:
        _DEVICE_INPUTS.clear()  # one case at a time: the largest is ~50 MB
        _DEVICE_INPUTS[case.name] = dict(
            m2=_f32(case.means2D, device), rgb=_f32(case.rgb, device), co=_f32(case.conic_opacity, device),
            radii=torch.from_numpy(case.radii.copy()).to(device), depths=_f32(case.depths, device),
            bands=torch.from_numpy(case.bands.copy()).to(device))
    return _DEVICE_INPUTS[case.name]


def _bits(t):
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy()


def _same(want, got, label):
    """torch.equal on the int32 bits of everything; exchange_refs names the first wrong element when it fails"""
    want = torch.from_numpy(np.ascontiguousarray(want))
    g = (got.view(torch.int32) if got.dtype == torch.float32 else got).cpu().reshape(want.shape).to(want.dtype)
    if not torch.equal(g, want):
        R.assert_same_ints(want.numpy(), g.numpy(), label)
    assert torch.equal(g, want), label


def _same_message(want_msg, want_idx, msg, idx, segs, label):
    assert msg.dtype == torch.float32 and idx.dtype == torch.int32
    wm, wi = torch.from_numpy(want_msg.reshape(-1, R.REC)), torch.from_numpy(want_idx)
    gm, gi = msg.view(torch.int32).cpu(), idx.cpu()
    if not (gm.shape == wm.shape and torch.equal(gm, wm) and torch.equal(gi, wi)):
        R.assert_same_message(want_msg, want_idx, gm.numpy(), gi.numpy(), segs, label)
    assert torch.equal(gm, wm) and torch.equal(gi, wi), label


def _count(case, x, c0, cn):
    dev = x["radii"].device
    n = lib.gsr_exchange_chunks(case.P)
    assert n == case.chunks
    cc = torch.full((case.W * cn, n), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((case.W, cn), -7, dtype=torch.int32, device=dev)
    dgr.check(lib.gsr_exchange_count(case.P, case.B, c0, cn, case.W, case.width, case.height, _p(x["m2"]), _p(x["radii"]),
                                     _p(x["bands"]), _p(cc), _p(cnt), _s()), "gsr_exchange_count")
    return cc, cnt


def _message(n, dev):
    return (torch.full((n, R.REC), float("nan"), dtype=torch.float32, device=dev),
            torch.full((n,), -7, dtype=torch.int32, device=dev))


def _pack(case, x, cc, c0, cn, k0, nb, off, n_send):
    msg, idx = _message(n_send, x["radii"].device)
    seg = (ctypes.c_int32 * (case.W * nb))(*off)
    dgr.check(lib.gsr_exchange_pack(case.P, case.B, k0, nb, case.W, case.width, case.height, cn, c0, _p(x["m2"]),
                                    _p(x["rgb"]), _p(x["co"]), _p(x["radii"]), _p(x["depths"]), _p(x["bands"]), _p(cc), seg,
                                    n_send, _p(msg), _p(idx), _s()), "gsr_exchange_pack")
    return msg, idx


def _pack_slab(case, x, cc, cnt, c0, cn, k0, nb, caps):
    n = int(sum(caps))
    msg, idx = _message(n, x["radii"].device)
    arr = (ctypes.c_int32 * (case.W * nb))(*caps)
    dgr.check(lib.gsr_exchange_pack_slab(case.P, case.B, k0, nb, case.W, case.width, case.height, cn, c0, _p(x["m2"]),
                                         _p(x["rgb"]), _p(x["co"]), _p(x["radii"]), _p(x["depths"]), _p(x["bands"]), _p(cc),
                                         _p(cnt), arr, n, _p(msg), _p(idx), _s()), "gsr_exchange_pack_slab")
    return msg, idx


def _unpack(recv, guard=3):
    """gsr_exchange_unpack into outputs with `guard` sentinel rows behind them -> the five tensors [n + guard, .]"""
    n, dev = recv.shape[0], recv.device
    assert recv.is_contiguous() and recv.dtype == torch.float32 and recv.shape[1] == R.REC
    outs = [torch.full((n + guard, w), float("nan"), dtype=torch.float32, device=dev) for w in (2, 3, 4)]
    radii = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    depths = torch.full((n + guard,), float("nan"), dtype=torch.float32, device=dev)
    dgr.check(lib.gsr_exchange_unpack(n, _p(recv), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(radii), _p(depths), _s()),
              "gsr_exchange_unpack")
    return outs[0], outs[1], outs[2], radii, depths


NAN_BITS = int(torch.tensor([float("nan")]).view(torch.int32)[0])
NAMES = ("means2D", "rgb", "conic_opacity", "radii", "depths")


def _check_unpack(want_msg_bits, recv, label, guard=3):
    outs = _unpack(recv, guard)
    n = recv.shape[0]
    for name, want, got in zip(NAMES, R.unpack(want_msg_bits), outs):
        _same(want, got[:n], f"{label} unpack {name}")
        tail = _bits(got[n:])
        assert (tail == (-7 if name == "radii" else NAN_BITS)).all(), f"{label} unpack {name}: wrote past row {n}"


# ------------------------------------------------------------------------------------------ need, count, pack, unpack
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_need_count_pack_slab_unpack_bit_for_bit(device, case):
    x = _inputs(case, device)
    W, B, P = case.W, case.B, case.P
    need = torch.full((W, B, P), 7, dtype=torch.uint8, device=device)
    ncnt = torch.full((W, B), -7, dtype=torch.int32, device=device)
    dgr.check(lib.gsr_exchange_need(P, B, W, case.width, case.height, _p(x["m2"]), _p(x["radii"]), _p(x["bands"]), _p(need),
                                    _p(ncnt), _s()), "gsr_exchange_need")
    _same(R.need(case).astype(np.uint8), need, f"{case} need")
    _same(R.counts(case)[1], ncnt, f"{case} need counts")
    assert torch.equal(need.sum(2, dtype=torch.int32), ncnt)
    for c0, cn, packs in R.launches(case):
        cc_ref, cnt_ref = R.counts(case, c0, cn)
        cc, cnt = _count(case, x, c0, cn)
        # (the packs below are sized from the reference's counts: they are launched only once the device agrees)
        _same(cnt_ref, cnt, f"{case} counts of [{c0}, {c0 + cn})")
        _same(cc_ref, cc, f"{case} chunk counts of [{c0}, {c0 + cn})")
        for k0, nb in packs:
            label = f"{case} count [{c0}, {c0 + cn}) pack ({k0}, {nb})"
            want_msg, want_idx, off, segs = R.pack(case, k0, nb)
            msg, idx = _pack(case, x, cc, c0, cn, k0, nb, off, want_idx.size)
            _same_message(want_msg, want_idx, msg, idx, segs, label)
            caps = R.mixed_capacities(R.counts(case, k0, nb)[1], salt=k0)
            want_msg, want_idx, segs, stats = R.pack_slab(case, caps, k0, nb)
            msg, idx = _pack_slab(case, x, cc, cnt, c0, cn, k0, nb, caps)
            _same_message(want_msg, want_idx, msg, idx, segs, label + " slab")
            _check_unpack(want_msg, msg, label)
            print(f"{label}: exact message {R.pack(case, k0, nb)[1].size} rows; slab {stats['sent']} rows sent, "
                  f"{stats['overflowed']} of {len(caps)} segments overflowed, {stats['padding']} padding rows")


def test_slab_layouts_every_capacity_relation(device):
    case = R.slab_layouts()[0]
    x = _inputs(case, device)
    cnt_ref = R.counts(case)[1]
    cc, cnt = _count(case, x, 0, case.B)
    _same(cnt_ref, cnt, "counts")
    for name, caps in R.slab_capacities(case).items():
        want_msg, want_idx, segs, stats = R.pack_slab(case, caps)
        msg, idx = _pack_slab(case, x, cc, cnt, 0, case.B, 0, case.B, caps)
        _same_message(want_msg, want_idx, msg, idx, segs, f"slab layout {name}")
        if msg.shape[0]:
            _check_unpack(want_msg, msg, f"slab layout {name}")
        print(f"slab layout {name}: relations {sorted({R.relation(c, n) for c, n in zip(caps, cnt_ref.reshape(-1).tolist())})}, "
              f"{stats['sent']} rows sent, {stats['overflowed']} segments overflowed, {stats['padding']} padding rows")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 512, 513])
def test_unpack_block_edges_at_every_alignment(device, n):
    """a slab that starts 0, 44, 88 and 132 bytes into a buffer: only the first is 16-byte aligned (vector staging of full
    256-row blocks), the others take the scalar staging; the last block is partial for every n but 256 and 512"""
    g = torch.Generator().manual_seed(n)
    buf = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 8, R.REC), generator=g, dtype=torch.int64).to(torch.int32)
    dbuf = buf.to(device).view(torch.float32)
    for first in (0, 1, 2, 3):
        recv = dbuf[first:first + n]
        assert (recv.data_ptr() % 16 == 0) == (first == 0)
        _check_unpack(buf[first:first + n].numpy(), recv, f"n {n} offset {first}")


def test_unpack_grid_stride_trip(device):
    """more rows than 16384 workgroups of 256: the first 300 rows' workgroups make a second trip"""
    n = 16384 * 256 + 300
    g = torch.Generator(device=device).manual_seed(1)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, R.REC), generator=g, dtype=torch.int64, device=device).to(torch.int32)
    outs = _unpack(bits.view(torch.float32), guard=2)
    for name, got, cols in zip(NAMES, outs, (slice(0, 2), slice(2, 5), slice(5, 9), 9, 10)):
        assert torch.equal(got[:n].view(torch.int32), bits[:, cols].contiguous()), name
        assert bool((got[n:].view(torch.int32) == (-7 if name == "radii" else NAN_BITS)).all()), name


# ------------------------------------------------------------------------------------------------ scatter-add
def test_scatter_add_rows_within_the_float32_sum_bound(device):
    """300 000 rows into 5 000 (the grid-stride trip needs more than 233 016 rows), into a prefilled dst.  A float32 sum
    of k + 1 numbers in ANY order is within (k + 1) u (sum of the magnitudes), u = 2^-24, of the true sum (Higham,
    Accuracy and Stability of Numerical Algorithms, eq. 4.4, first order; the factor 1.01 covers the higher orders for
    k u < 0.01); the float64 reference's own error is 2^-29 of that.  k = terms of the element that are not zero."""
    n, rows = 300_000, 5_000
    g = torch.Generator().manual_seed(21)
    idx = torch.randint(0, 4000, (n,), generator=g, dtype=torch.int32)
    idx[290_000:290_900] = torch.arange(4000, 4900, dtype=torch.int32)  # rows 4000 .. 4899: exactly one term each
    idx[290_900:] = torch.randint(0, 4000, (n - 290_900,), generator=g, dtype=torch.int32)  # rows 4900 ..: none
    src = torch.randn(n, 9, generator=g) * torch.exp(3.0 * torch.randn(n, 1, generator=g))
    idx[torch.rand(n, generator=g) < 0.05] = -1          # slab padding rows: skipped, whatever they hold
    src[torch.rand(n, generator=g) < 0.10] = 0.0         # zero rows
    src[290_017] = 0.0                                    # ... one of them the only term of its row
    src[12_345] = float("nan")
    idx[12_345] = 17
    dst0 = torch.randn(rows, 9, generator=g)
    dst0[4000:4500] = 0.0
    dst0[4900:4950] = 0.0
    out = dst0.to(device)
    got = dgr.scatter_add_rows(idx.to(device), src.to(device), rows, dst=out)
    assert got is out
    out = out.cpu()
    keep = idx >= 0
    ref = dst0.double().index_add_(0, idx[keep].long(), src[keep].double())
    mag = dst0.abs().double().index_add_(0, idx[keep].long(), src[keep].abs().double())
    k = torch.zeros(rows, 9, dtype=torch.float64).index_add_(0, idx[keep].long(), (src[keep] != 0).double())
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and int(torch.isnan(ref).sum()) == 9
    assert bool(torch.isnan(out[17]).all())
    fin = ~torch.isnan(ref)
    bound = 1.01 * (k + 1) * 2.0 ** -24 * mag
    err = (out.double() - ref).abs()
    ratio = torch.where(fin & (bound > 0), err / bound.clamp_min(1e-300), torch.zeros_like(err))
    print(f"scatter-add: largest k {int(k.max())}, largest |out - ref| / bound {float(ratio.max()):.4f}")
    assert bool((err[fin] <= bound[fin]).all()), float(ratio.max())
    exact = fin & (k <= 1) & (dst0 == 0)
    assert int(exact[4000:4500].sum()) >= 400 * 9 and int((k == 0).sum()) >= 100 * 9
    assert torch.equal(out[exact].double(), ref[exact])
    assert torch.equal(out[4900:], dst0[4900:]), "rows without a term keep their bits"


def test_scatter_add_rows_distinct_indices_is_exact(device):
    n = 300_000
    g = torch.Generator().manual_seed(22)
    idx = torch.randperm(n, generator=g).to(torch.int32)
    src, dst0 = torch.randn(n, 9, generator=g), torch.randn(n, 9, generator=g)
    src[::11] = 0.0
    out = dgr.scatter_add_rows(idx.to(device), src.to(device), n, dst=dst0.to(device)).cpu()
    ref = dst0.double().index_add_(0, idx.long(), src.double())
    assert torch.equal(out.double(), ref.float().double())  # one float32 addition an element: correctly rounded


# ------------------------------------------------------------------------------------------------ flags
OTHER_BITS = 0x50  # bits of the flag word that belong to nobody here


def _check(all_counts, caps, W, B, me, mask, few, device, flag0=OTHER_BITS):
    flag = torch.tensor([flag0], dtype=torch.int32, device=device)
    host = torch.zeros(W * W * B, dtype=torch.int32).pin_memory()
    host.fill_(-7)
    dgr.exchange_check(all_counts.to(device).contiguous(), caps.to(device).contiguous(), W, B, me, mask, few, flag, host)
    torch.cuda.synchronize()
    assert torch.equal(host, all_counts.reshape(-1)), "the pinned copy is the counts"
    return int(flag.item())


def _check_rule(all_counts, caps, me, mask, few):
    """FLAG_SLAB when a count exceeds its capacity; FLAG_FEW when a camera this rank renders (bit k of the mask)
    receives, summed over the senders, fewer than `few` rows"""
    bits = dgr.FLAG_SLAB if bool((all_counts > caps).any()) else 0
    for k in range(all_counts.shape[2]):
        if (mask >> k) & 1 and int(all_counts[:, me, k].sum()) < few:
            bits |= dgr.FLAG_FEW
    return bits


@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_exchange_check_truth_table(device, W, B):
    assert (dgr.FLAG_SLAB | dgr.FLAG_FEW) & OTHER_BITS == 0 and dgr.FLAG_SLAB != dgr.FLAG_FEW
    few, n = 10, W * W * B
    every = (1 << B) - 1
    g = torch.Generator().manual_seed(W * 100 + B)
    for me in sorted({0, W - 1}):
        caps = torch.randint(20, 100, (W, W, B), generator=g, dtype=torch.int32)
        # over capacity: equal is not over; one above is, wherever the word sits
        assert _check(caps.clone(), caps, W, B, me, every, few, device) == OTHER_BITS
        for at in sorted({0, n - 1, n // 2} | ({256, 257} if n > 257 else set())):
            c = caps.clone()
            c.view(-1)[at] += 1
            assert _check(c, caps, W, B, me, every, few, device) == OTHER_BITS | dgr.FLAG_SLAB, at
            c.view(-1)[at] -= 2
            assert _check(c, caps, W, B, me, every, few, device) == OTHER_BITS, at
        # too few rows: the rows camera k receives on this rank are the sum over the senders i of [i][me][k]
        for k in sorted({0, B - 1, B // 2}):
            c = caps.clone()
            c[:, me, k] = 0
            c[W - 1, me, k] = few - (W - 1)  # with (W - 1) ones below: exactly `few`
            c[:W - 1, me, k] = 1
            assert int(c[:, me, k].sum()) == few and bool((c <= caps).all())
            assert _check(c, caps, W, B, me, every, few, device) == OTHER_BITS, k
            c[W - 1, me, k] -= 1
            assert _check(c, caps, W, B, me, every, few, device) == OTHER_BITS | dgr.FLAG_FEW, k
            assert _check(c, caps, W, B, me, 1 << k, few, device) == OTHER_BITS | dgr.FLAG_FEW, k
            assert _check(c, caps, W, B, me, every & ~(1 << k), few, device) == OTHER_BITS, (k, "not rendered")
            assert _check(c, caps, W, B, me, 0, few, device) == OTHER_BITS, (k, "nothing rendered")
            if B > 1:  # the neighbouring bit alone does not stand for camera k
                assert _check(c, caps, W, B, me, 1 << ((k + 1) % B), few, device) == OTHER_BITS, k
            if W > 1:  # what another rank receives is not this rank's business
                c = caps.clone()
                c[:, (me + 1) % W, k] = 0
                assert _check(c, caps, W, B, me, every, few, device) == OTHER_BITS, k
            # both at once, and a few random tables, against the rule written out
            c = caps.clone()
            c[:, me, k] = 0
            c.view(-1)[n - 1] = caps.view(-1)[n - 1] + 1
            want = _check_rule(c, caps, me, every, few)
            assert want & dgr.FLAG_SLAB
            assert _check(c, caps, W, B, me, every, few, device) == OTHER_BITS | want, k
        for _ in range(4):
            c = torch.randint(0, 30, (W, W, B), generator=g, dtype=torch.int32)
            mask = int(torch.randint(0, 2 ** 62, (1,), generator=g)) << 2 & every | (1 << (B - 1))
            tight = torch.where(torch.rand(W, W, B, generator=g) < 0.02, c - 1, c)
            for cp in (tight, c, c + 3):
                assert _check(c, cp, W, B, me, mask, few, device) == OTHER_BITS | _check_rule(c, cp, me, mask, few)
    if B == 64:
        assert every >> 63 == 1  # bit 63 of the mask was set in every call above that rendered everything


def test_flag_if_greater(device):
    bit = 0x8
    for value, limit, over in ((5, 5, False), (6, 5, True), (0, 0, False), (1, 0, True), (4, 5, False),
                               (0x7FFFFFFF, 0x7FFFFFFF, False), (0x80000000, 0x7FFFFFFF, True),
                               (0xFFFFFFFF, 0xFFFFFFFE, True), (0xFFFFFFFF, 0xFFFFFFFF, False), (3, 0xFFFFFFFF, False)):
        v = torch.tensor([value], dtype=torch.int64).to(torch.int32).to(device) if value < 2 ** 31 else \
            torch.tensor([value - 2 ** 32], dtype=torch.int32, device=device)
        for flag0 in (0, OTHER_BITS, OTHER_BITS | bit):
            flag = torch.tensor([flag0], dtype=torch.int32, device=device)
            host = torch.zeros(1, dtype=torch.int32).pin_memory()
            host.fill_(-7)
            dgr.check(lib.gsr_flag_if_greater(_p(v), limit, _p(flag), bit, host.data_ptr(), _s()), "gsr_flag_if_greater")
            torch.cuda.synchronize()
            assert int(flag.item()) == flag0 | (bit if over else 0), (value, limit, flag0)
            assert int(host.item()) & 0xFFFFFFFF == value, (value, limit)
        flag = torch.tensor([OTHER_BITS], dtype=torch.int32, device=device)  # no host copy asked for
        dgr.check(lib.gsr_flag_if_greater(_p(v), limit, _p(flag), bit, None, _s()), "gsr_flag_if_greater")
        assert int(flag.item()) == OTHER_BITS | (bit if over else 0)


@pytest.mark.parametrize("slots", [1, 4, 7])
def test_publish_flag_lands_in_slot_seq_mod_slots(device, slots):
    for seq in (0, slots - 1, slots, 2 * slots + 3, 2 ** 31 + 5):
        for flag0 in (0, 0x6):
            ring = torch.zeros((slots, 2), dtype=torch.int32).pin_memory()
            ring.fill_(-7)
            flag = torch.tensor([flag0], dtype=torch.int32, device=device)
            s = torch.tensor([seq if seq < 2 ** 31 else seq - 2 ** 32], dtype=torch.int32, device=device)
            dgr.check(lib.gsr_publish_flag(_p(flag), _p(s), ring.data_ptr(), slots, _s()), "gsr_publish_flag")
            torch.cuda.synchronize()
            want = torch.full((slots, 2), -7, dtype=torch.int32)
            want[seq % slots, 0] = flag0
            want[seq % slots, 1] = int(s.item())
            assert torch.equal(ring, want), (seq, slots, ring.tolist())
            assert int(flag.item()) == flag0  # publishing does not clear the word


@pytest.mark.parametrize("stride", [2, 7])
def test_band_mask_strides_and_grid_trip(device, stride):
    gx, gy, B = 80, 68, 13
    assert gx * gy * B > 256 * 256  # more elements than the launch has threads: the grid-stride trip runs
    rows = [(3, 9), (0, gy), (5, 5), (gy, gy + 12), (9, 3), (60, 100), (0, 1), (gy - 1, gy), (-4, 2), (0, 0), (67, 68),
            (gy + 3, gy + 9), (1, gy - 1)]
    assert len(rows) == B
    words = torch.full((B, stride), 12345, dtype=torch.int32)
    words[:, 0:2] = torch.tensor(rows, dtype=torch.int32)
    mask = torch.full((B, gy, gx), 7, dtype=torch.uint8, device=device)
    dgr.check(lib.gsr_band_mask(gx, gy, B, _p(words.to(device)), stride, _p(mask), _s()), "gsr_band_mask")
    ty = np.arange(gy)[None, :, None]
    lo, hi = np.array(rows)[:, 0][:, None, None], np.array(rows)[:, 1][:, None, None]
    want = np.broadcast_to((ty >= lo) & (ty < hi), (B, gy, gx)).astype(np.uint8)
    assert want[2].sum() == 0 and want[3].sum() == 0 and want[4].sum() == 0 and want[1].all()
    _same(want, mask, f"band mask, stride {stride}")
