"""-m gpu: the row movers of csrc/compact.hip and the radix configuration behind them, bit for bit.

gsr_group_rows and gsr_knn_mean_dist2 are the only callers of radix_sort_pairs outside binning; above 2^22 rows
(RADIX_SHORT_N) the sort runs its 512-thread configuration, which redistribution of a real model reaches and no other
test of these two entry points does.  gsr_gather_rows / gsr_scatter_rows move 4-byte words of up to 32 tensors in one
launch: odd widths, strided rows on either side, row0, the identity order and the grid-stride trip.  And the shape check
of densify_stats, whose kernel cannot check sizes."""
import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import exchange_refs as R
from oracle import densify_oracle as O

pytestmark = pytest.mark.gpu

SHORT_N = 1 << 22  # RADIX_SHORT_N of csrc/radix.h


# ------------------------------------------------------------------------------------------------ group_rows
@pytest.mark.parametrize("groups", [1, 255])
@pytest.mark.parametrize("n", [SHORT_N - 1, SHORT_N, SHORT_N + 1, SHORT_N + 4097])
def test_group_rows_across_the_long_sort_boundary(device, n, groups):
    """order and counts equal the stable sort; rows whose destination is -1, G or 2^31 - 1 are dropped (sorted last, in
    their original order).  Above 2^22 rows the 512-thread sort runs, and its values land directly in `order`."""
    g = torch.Generator().manual_seed(n + groups)
    dest = torch.randint(0, groups, (n,), generator=g, dtype=torch.int32)
    odd = torch.rand(n, generator=g)
    dest[odd < 0.05] = -1
    dest[(odd >= 0.05) & (odd < 0.10)] = groups
    dest[(odd >= 0.10) & (odd < 0.15)] = 2 ** 31 - 1
    dest[0], dest[n - 1], dest[n // 2] = 2 ** 31 - 1, -1, groups
    order, counts = dgr.group_rows(dest.to(device), groups)
    ref_order, ref_counts = O.group_rows(dest, groups)
    assert counts == ref_counts and sum(counts) == n and counts[groups] > n // 10
    assert torch.equal(order.cpu(), ref_order)


# ------------------------------------------------------------------------------------------------ gather / scatter
WIDTHS = (1, 2, 3, 4, 11, 48)
SENT = -7


def _random_bits(shape, g):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)


def _sources(N, g, device):
    """six tensors of the six widths: dense ones (1-D, [N,3], int32 [N,4], [N,16,3]) and two column blocks of a wider
    record matrix (row stride 80 words).  float32 tensors carry arbitrary bits (NaN payloads included)."""
    rec = _random_bits((N, 80), g).to(device)
    return [_random_bits((N,), g).to(device).view(torch.float32), rec.view(torch.float32)[:, 0:2],
            _random_bits((N, 3), g).to(device).view(torch.float32), _random_bits((N, 4), g).to(device),
            rec[:, 5:16], _random_bits((N, 16, 3), g).to(device).view(torch.float32)]


def _i32(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _flat(t, n=None):
    t = _i32(t)
    return t.reshape(t.shape[0], -1)[:n]


def test_gather_rows_widths_strides_row0_and_grid_trip(device):
    N, n_out, row0 = 50_000, 44_000, 123
    assert n_out * max(WIDTHS) > 8192 * 256  # more words than the launch has threads: the grid-stride trip runs
    g = torch.Generator().manual_seed(31)
    srcs = _sources(N, g, device)
    assert [int(np.prod(s.shape[1:])) for s in srcs] == list(WIDTHS)
    order = torch.randperm(N, generator=g).to(torch.int32).to(device)
    sel = order[row0:row0 + n_out].long()
    rec = torch.full((n_out + 5, 70), SENT, dtype=torch.int32, device=device)
    big = torch.full((n_out + 20, 4), SENT, dtype=torch.int32, device=device)
    dsts = [torch.full((n_out,), SENT, dtype=torch.int32, device=device).view(torch.float32),
            torch.full((n_out, 2), SENT, dtype=torch.int32, device=device).view(torch.float32),
            rec.view(torch.float32)[:, 0:3],   # a column block: row stride 70 for 3 words
            big[7:7 + n_out],                  # a view of an existing tensor
            rec[:, 10:21],
            torch.full((n_out, 16, 3), SENT, dtype=torch.int32, device=device).view(torch.float32)]
    out = dgr.gather_rows(order, n_out, srcs, dsts, row0=row0)
    assert all(a is b for a, b in zip(out, dsts))
    for w, s, d in zip(WIDTHS, srcs, dsts):
        assert torch.equal(_flat(d, n_out), _flat(s)[sel]), w
    want = torch.full_like(rec, SENT)
    want[:n_out, 0:3], want[:n_out, 10:21] = _flat(srcs[2])[sel], _flat(srcs[4])[sel]
    assert torch.equal(rec, want), "the words of the record matrix between and behind the column blocks keep their bits"
    want = torch.full_like(big, SENT)
    want[7:7 + n_out] = srcs[3][sel]
    assert torch.equal(big, want)
    # the identity order, into fresh dense tensors
    dense = dgr.gather_rows(None, n_out, srcs)
    for w, s, d in zip(WIDTHS, srcs, dense):
        assert d.is_contiguous() and d.shape == (n_out,) + tuple(s.shape[1:]) and d.dtype == s.dtype
        assert torch.equal(_flat(d), _flat(s, n_out)), w


def test_scatter_rows_inverts_gather_rows(device):
    N = 50_000
    g = torch.Generator().manual_seed(32)
    srcs = _sources(N, g, device)
    perm = torch.randperm(N, generator=g).to(torch.int32).to(device)
    moved = dgr.gather_rows(perm, N, srcs)
    for s, m in zip(srcs, moved):
        assert torch.equal(_flat(m), _flat(s)[perm.long()])
    # back into tensors laid out like the sources (two of them column blocks of one record matrix)
    rec = torch.full((N, 80), SENT, dtype=torch.int32, device=device)
    back = [torch.full(tuple(s.shape), SENT, dtype=torch.int32, device=device).view(s.dtype) for s in srcs]
    back[1], back[4] = rec.view(torch.float32)[:, 0:2], rec[:, 5:16]
    dgr.scatter_rows(perm, N, moved, back)
    for w, s, b in zip(WIDTHS, srcs, back):
        assert torch.equal(_flat(b), _flat(s)), w
    assert bool((rec[:, 2:5] == SENT).all()) and bool((rec[:, 16:] == SENT).all())
    # a few rows only, through row0: the rows `order` does not name keep their sentinel
    n_in, row0 = 1000, 77
    part = [torch.full(tuple(s.shape), SENT, dtype=torch.int32, device=device).view(s.dtype) for s in srcs]
    named = perm[row0:row0 + n_in].long()
    dgr.scatter_rows(perm, n_in, moved, part, row0=row0)
    for w, m, p in zip(WIDTHS, moved, part):
        want = torch.full_like(_flat(p), SENT)
        want[named] = _flat(m, n_in)
        assert torch.equal(_flat(p), want), w


# ------------------------------------------------------------------------------------------------ KNN
def test_knn_lattice_above_the_long_sort_boundary(device):
    """4 199 040 points, shuffled, whose answer is known in closed form (exchange_refs.lattice; the CPU file holds the
    closed form to the brute-force restatement on small lattices): exactly 3.0 on the x-boundary, 2.0 elsewhere.  The
    search is exact whatever the order of the points, but only if every point is there once: a Morton sort that lost
    or doubled a point changes some point's neighbours, and every point is checked."""
    pts, want = R.lattice(162, 162, 160, seed=7)
    assert pts.shape[0] == 4_199_040 > SHORT_N
    out = dgr.knn_mean_dist2(torch.from_numpy(pts).to(device)).cpu()
    assert torch.equal(out, torch.from_numpy(want)), int((out != torch.from_numpy(want)).sum())


# ------------------------------------------------------------------------------------------------ densify_stats
def _stats_buffers(P, device, **rows):
    g = torch.Generator().manual_seed(P)
    radii = torch.randint(0, 40, (rows.get("radii", P),), generator=g, dtype=torch.int32).to(device)
    rec = torch.randn((rows.get("grad", P), 9), generator=g).to(device)
    return (radii, rec[:, 0:2], torch.zeros(rows.get("max_radii2D", P), device=device),
            torch.zeros((rows.get("accum", P), 1), device=device), torch.zeros((rows.get("denom", P), 1), device=device))


@pytest.mark.parametrize("short", ["grad", "max_radii2D", "accum", "denom"])
@pytest.mark.parametrize("delta", [-1, 1, -100])
def test_densify_stats_refuses_buffers_of_another_row_count(device, monkeypatch, short, delta):
    """a buffer left over from before a densification event: ValueError, and the entry point is not reached.  The library
    function is replaced by a recording stub for the test, so no launch with a short buffer can happen whatever the
    wrapper does."""
    calls = []
    monkeypatch.setattr(dgr.lib, "gsr_densify_stats", lambda *a: calls.append(a) or 0)
    P = 100
    with pytest.raises(ValueError, match="densify_stats"):
        dgr.densify_stats(*_stats_buffers(P, device, **{short: P + delta}))
    assert calls == []
    dgr.densify_stats(*_stats_buffers(P, device))  # matching shapes go through
    assert len(calls) == 1 and calls[0][0] == P


def test_densify_stats_with_matching_shapes_still_computes(device):
    P = 3001
    radii, grad, max_r, accum, denom = _stats_buffers(P, device)
    vis = radii > 0
    assert 0 < int(vis.sum()) < P
    for _ in range(2):
        dgr.densify_stats(radii, grad, max_r, accum, denom)
    assert torch.equal(max_r, torch.where(vis, radii.float(), torch.zeros_like(max_r)))
    assert torch.equal(denom[:, 0], 2.0 * vis.float())
    ref = 2.0 * torch.where(vis, torch.norm(grad.double(), dim=-1), torch.zeros(P, dtype=torch.float64, device=device))
    # (the bound of tests/test_gpu_densify.py::test_densification_statistics_without_boolean_indexing)
    assert float((accum[:, 0].double() - ref).abs().max()) <= 4e-7 * float(ref.max())
    assert bool((accum[~vis] == 0).all())
