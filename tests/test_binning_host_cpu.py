"""The host side of K3-K7 (csrc/binning_host.h) without a device: the workspace arithmetic and the argument checks that
return before the first HIP call.

tests/golden/binning_layout_parent.json holds what the five sizing entry points answered BEFORE the host side was
rewritten around BinFrame / BinDevice / SortPlan.  It was recorded by running this file as a script against the library
built from the commit before that change,

    GSRASTER_LIB=<that build>/libgsraster.so python tests/test_binning_host_cpu.py --record

which evaluates `_table` below and writes the file.  The layouts are an interface: the operator sizes its buffers with
them and reads device words at gsr_bin_total_offset / gsr_bin_segments_offset, so equality is exact.
"""
import ctypes
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binning_layout_parent.json")

PS = (0, 1, 4095, 4096, 4097, 8193, 1_000_000)
DS = (0, 1, 4096, 4097, (5 << 20) - 1, 5 << 20, 6 << 20, (6 << 20) + 1, (1 << 31) - 1)
SCRATCH = (0, 1 << 20, 256 << 20, 22 << 30)
# 4096 x 4096: 256 x 256 tiles, the last (row, column) frame; 4112 x 4096: 257 tile columns, generic (capacity 0)
FRAMES = ((16, 16), (333, 211), (1920, 1080), (4096, 4096), (4112, 4096), (8000, 8000))
EINVAL = -1


def _table(lib):
    t = {"prepare_bytes": {}, "total_offset": {}, "segments_offset": {}, "sort_bytes": {}, "sort_capacity": {}}
    for W, H in FRAMES:
        for P in PS:
            k = f"{P},{W},{H}"
            t["prepare_bytes"][k] = lib.gsr_bin_prepare_bytes(P, W, H)
            t["total_offset"][k] = lib.gsr_bin_total_offset(P, W, H)
            t["segments_offset"][k] = lib.gsr_bin_segments_offset(P, W, H)
            for D in DS:
                t["sort_bytes"][f"{P},{D},{W},{H}"] = lib.gsr_bin_sort_bytes(P, D, W, H)
            for nbytes in SCRATCH:
                t["sort_capacity"][f"{P},{nbytes},{W},{H}"] = lib.gsr_bin_sort_capacity(P, nbytes, W, H)
    return t


def _lib():
    import diff_gaussian_rasterization as dgr

    return dgr._lib.lib


def test_layouts_equal_the_recorded_parent_table():
    lib = _lib()
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _table(lib)
    assert set(got) == set(want)
    for name in want:
        assert set(got[name]) == set(want[name]), name
        bad = {k: (got[name][k], v) for k, v in want[name].items() if got[name][k] != v}
        assert not bad, (name, dict(list(bad.items())[:5]))
    # orientation (read off the parent): the table holds them too
    assert want["sort_bytes"][f"1000000,{5 << 20},1920,1080"] == lib.gsr_bin_sort_bytes(1000, 5 << 20, 1920, 1080) == 86_605_056
    assert want["prepare_bytes"]["4097,1920,1080"] == 261_120
    assert lib.gsr_bin_sort_capacity(1000, 1 << 28, 4112, 4096) == 0


def test_argument_checks_that_return_before_any_device_call():
    """codes of the parent, each checked against its build; dummy non-zero integers stand for device pointers -- every
    call below returns before anything is dereferenced, launched or asked of the HIP runtime"""
    lib = _lib()
    d = 0x1000
    # the three switches: an out-of-range mode is refused.  Only the return code can be checked without a device (no
    # sizing entry point depends on a mode); a valid mode is still accepted afterwards
    for setter, bad in ((lib.gsr_set_bin_persistent, (-2, 4)), (lib.gsr_set_bin_rowmajor, (-2, 2)),
                        (lib.gsr_set_tile_cull, (-2, 3))):
        for mode in bad:
            assert setter(mode) == EINVAL, (setter.__name__, mode)
    assert lib.gsr_set_bin_rowmajor(-1) == 0 and lib.gsr_set_tile_cull(-1) == 0
    # tile sort
    assert lib.gsr_bin_sort_bounded(10, 64, 64, d, d, 0, d, 1 << 20, d, d, None) == EINVAL  # capacity 0
    assert lib.gsr_bin_sort(10, 0, 64, d, d, 100, d, 1 << 20, d, d, None) == EINVAL         # width 0
    assert lib.gsr_bin_sort(10, 64, 64, d, d, 100, d, 1 << 20, d, None, None) == EINVAL     # no ranges
    # prepare step
    assert lib.gsr_bin_prepare_async(10, 64, 64, d, d, d, d, d, d, 1 << 20, None, None) == EINVAL  # no ticket
    assert lib.gsr_bin_speculative_async(10, 64, 64, d, d, d, d, d, d, 1 << 20, 0, None, 0, None, d, None,
                                         ctypes.byref(ctypes.c_int(0)), None) == EINVAL            # no ticket
    ticket = ctypes.c_uint32(7)
    assert lib.gsr_bin_prepare_async(0, 64, 64, d, d, d, d, d, d, 0, ctypes.byref(ticket), None) == 0
    assert ticket.value == 0  # P = 0: nothing launched, the count is 0
    count = ctypes.c_int64(5)
    assert lib.gsr_bin_count_wait(0, ctypes.byref(count), None) == 0 and count.value == 0


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit(__doc__)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "grendel-gs_amd"))
    with open(GOLDEN, "w") as f:
        json.dump(_table(_lib()), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
