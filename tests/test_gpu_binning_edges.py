"""-m gpu: K3-K7 on the hand-built families of tests/binning_refs.py, every tile list against the contract stated there
(reference rect, reference order, nothing dropped that float64 says can reach alpha >= 1/255), through every form of
the pipeline.

Per case and cull setting the first form's result goes through binning_refs.check_lists -- every tile, every pair -- and
every other form, through the sized and through the bounded (speculative) sort, must give the same bits: pair count,
ranges (hull row included) and point_list[:D].  The generic tile-id sort moves the pairs of non-local tiles inside the
mask's row hull behind the last tile instead of leaving them in place, so on masks that have such tiles it is held to
check_lists of its own, the same pair count and the same list in every tile; it has no exact tile culling, so it runs
with culling off only."""
import numpy as np
import pytest
import torch

import binning_refs as R
import diff_gaussian_rasterization as dgr

pytestmark = pytest.mark.gpu

# name -> (set_bin_persistent, set_bin_rowmajor, GSR_BINNING=generic, persistent launches per call with pairs: prepare, sort)
FORMS = {
    "lookback": ("off", False, False, (0, 0)),
    "persistent prepare": ("prepare", False, False, (1, 0)),
    "persistent sort": ("sort", False, False, (0, 1)),
    "persistent both": ("both", False, False, (1, 1)),
    "row-major": ("off", True, False, (0, 0)),
    "generic": ("off", False, True, (0, 0)),
}


def _device_inputs(case, device, perm=None):
    arrs = (case.means2D, case.depths, case.radii, case.conic_opacity)
    if perm is not None:
        arrs = tuple(a[perm] for a in arrs)
    t = [torch.tensor(np.ascontiguousarray(a)).to(device) for a in arrs]
    return t + [torch.tensor(case.mask.reshape(-1).astype(np.uint8)).to(device)]


def _bin(x, case):
    """-> (point_list[:D] on the device, ranges with the hull row on the device, D)"""
    pl, rg, D = dgr.bin_gaussians(*x, case.W, case.H)
    full = rg._base if rg._base is not None else rg  # (the op returns the per-tile rows of a tiles + 1 row table)
    assert full.shape == (case.tiles + 1, 2)
    return pl[:D].clone(), full.clone(), int(D)


def _per_tile(pl, rg):
    """the lists of all tiles back to back, whatever their offsets"""
    body = rg[:-1].long()
    n = body[:, 1] - body[:, 0]
    first = torch.repeat_interleave(body[:, 0] - (torch.cumsum(n, 0) - n), n)
    return n, pl[first + torch.arange(int(n.sum()), device=pl.device)]


def _run_forms(case, device, monkeypatch, forms, cull, tie="arrival", perm=None):
    """every form in `forms`, sized sort and bounded sort -> {form: (pl, rg, D)}, after asserting the two sorts agree and
    that a form said to be persistent launched its barrier kernels"""
    x = _device_inputs(case, device, perm)
    out = {}
    dgr.set_tile_cull(cull)
    for name in forms:
        persist, rows, generic, (lp, ls) = FORMS[name]
        dgr.set_bin_persistent(persist)
        dgr.set_bin_rowmajor(rows)
        if generic:
            monkeypatch.setenv("GSR_BINNING", "generic")
        try:
            dgr.release_workspaces()
            torch.cuda.synchronize()
            done = dgr.bin_persist_status()["done"]
            dgr.set_speculative_sort(False)
            sized = _bin(x, case)
            dgr.set_speculative_sort(True)  # the second call finds the first one's scratch: the bounded sort, where one exists
            _bin(x, case)
            bounded = _bin(x, case)
            torch.cuda.synchronize()
            launched = (dgr.bin_persist_status()["done"] - done) & 0xFFFFFFFF
        finally:
            monkeypatch.delenv("GSR_BINNING", raising=False)
        assert bounded[2] == sized[2], (case.name, name, cull)
        assert torch.equal(bounded[1], sized[1]) and torch.equal(bounded[0], sized[0]), (case.name, name, cull, "bounded sort")
        if tie == "position":
            lp = 0  # (the persistent prepare kernel does not take the position order: look-back prepare)
        if case.gx > 256 or case.gy > 256:
            ls = 0  # (tile-id keys: no persistent sort kernel)
        want = 3 * ((lp if case.P > 0 else 0) + (ls if sized[2] > 0 else 0))
        print(f"{case.name} | {name} cull={cull}: D {sized[2]}, persistent launches {launched} (expected {want})")
        assert launched == want, (case.name, name, cull, launched, want)
        out[name] = sized
    return out


def _check_case(case, device, monkeypatch, forms=tuple(FORMS), tie="arrival"):
    results = {}
    all_forms = forms
    for cull in (False, True):
        # (exact tile culling exists on the (row, column) path only: the generic sort has one setting)
        forms = tuple(f for f in all_forms if not (cull and FORMS[f][2]))
        got = _run_forms(case, device, monkeypatch, forms, cull, tie)
        first = forms[0]
        pl, rg, D = got[first]
        exact = bool(case.meta.get("exact")) and not cull
        info = R.check_lists(pl.cpu().numpy(), rg.cpu().numpy(), D, case, tie=tie, exact=exact)
        up = R.upper_lists(case, tie)
        print(f"{case.name} cull={cull}: D {D}, kept {info['kept']} of {up.count} upper pairs")
        for name in forms[1:]:
            fpl, frg, fD = got[name]
            assert fD == D, (case.name, name, cull, fD, D)
            if FORMS[name][2] and up.hole_pairs:
                R.check_lists(fpl.cpu().numpy(), frg.cpu().numpy(), fD, case, tie=tie, exact=exact)
                n, lists = _per_tile(pl, rg)
                fn, flists = _per_tile(fpl, frg)
                assert torch.equal(fn, n) and torch.equal(flists, lists), (case.name, name, cull)
                assert torch.equal(frg[-1], rg[-1])
            else:
                assert torch.equal(frg, rg), (case.name, name, cull, "ranges")
                assert torch.equal(fpl, pl), (case.name, name, cull, "point_list")
        results[cull] = info
    return results


@pytest.fixture
def binning_switches(monkeypatch):
    monkeypatch.setenv("GSR_BIN_PERSIST_MAXD", "1000000000")  # the persistent sort kernel whatever the pair count
    monkeypatch.setenv("GSR_BIN_ROWS_MIN", "1")               # the row-major pipeline whatever the pair count
    try:
        yield
    finally:
        dgr.set_bin_persistent("env")
        dgr.set_bin_rowmajor("env")
        dgr.set_tile_cull("env")
        dgr.set_tie_order("arrival")
        dgr.set_speculative_sort(True)
        dgr.release_workspaces()


@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f != "rect_sizes"])
def test_family_through_every_form(device, monkeypatch, binning_switches, family):
    for case in R.FAMILIES[family]():
        _check_case(case, device, monkeypatch)


def test_rect_sizes_through_every_form(device, monkeypatch, binning_switches):
    """... and, exact culling off, the narrowed rect of every shaped splat has exactly its w x h tiles (63, 64, 65 among
    them: the culling's 64-tile mask applies, just applies, does not apply)"""
    (case,) = R.rect_sizes()
    res = _check_case(case, device, monkeypatch)
    shapes = case.meta["shapes"]
    for cull in (False, True):
        n = np.bincount(res[cull]["gid"], minlength=case.P)[:len(shapes)]
        if not cull:
            assert np.array_equal(n, shapes[:, 0] * shapes[:, 1]), (n, shapes)
        else:
            assert (n <= shapes[:, 0] * shapes[:, 1]).all()
            big = shapes[:, 0] * shapes[:, 1] > 64  # (rects above 64 tiles keep every tile)
            assert np.array_equal(n[big], (shapes[:, 0] * shapes[:, 1])[big])


def test_position_tie_order(device, monkeypatch, binning_switches):
    """set_tie_order("position"): inside a tile (depth bits, x, y, index), checked on every list; and the lists do not
    depend on the order of the rows -- rows that agree in depth, x and y keep their relative order in the permutation,
    since between those the index decides by definition"""
    (case,) = R.position_ties()
    forms = ("lookback", "persistent sort", "row-major", "generic")
    dgr.set_tie_order("position")
    _check_case(case, device, monkeypatch, forms=forms, tie="position")
    rng = np.random.default_rng(3)
    new_of = rng.permutation(case.P)  # new_of[original row] = its row in the permuted arrays
    _, group = np.unique(np.stack([R.depth_bits(case).astype(np.float64), case.means2D[:, 0], case.means2D[:, 1]], axis=1),
                         axis=0, return_inverse=True)
    group = group.reshape(-1)
    by_orig = np.lexsort((np.arange(case.P), group))
    by_new = np.lexsort((new_of, group))
    new_of[by_orig] = new_of[by_new]  # inside a group the new rows ascend with the original index
    perm = np.empty(case.P, dtype=np.int64)
    perm[new_of] = np.arange(case.P)  # permuted arrays = original[perm]
    assert (np.sort(perm) == np.arange(case.P)).all() and (perm != np.arange(case.P)).sum() > case.P // 2
    for cull in (False, True):
        a = _run_forms(case, device, monkeypatch, ("lookback",), cull, "position")["lookback"]
        b = _run_forms(case, device, monkeypatch, ("lookback",), cull, "position", perm=perm)["lookback"]
        assert a[2] == b[2] and torch.equal(a[1], b[1])
        back = torch.tensor(perm, device=device)[b[0].long()].to(a[0].dtype)
        assert torch.equal(back, a[0]), f"cull={cull}: the lists depend on the order of the rows"
    # the arrival order on the same rows, for contrast: it must differ, and it must hold its own contract
    dgr.set_tie_order("arrival")
    arr = _run_forms(case, device, monkeypatch, ("lookback",), False)["lookback"]
    R.check_lists(arr[0].cpu().numpy(), arr[1].cpu().numpy(), arr[2], case)
    with pytest.raises(AssertionError, match="order"):
        R.check_lists(arr[0].cpu().numpy(), arr[1].cpu().numpy(), arr[2], case, tie="position")
