"""Mesh cleaning without a GPU: the reference of tests/meshclean_refs.py against a brute-force closure, the refusals of
the gsr_mesh_* entry points (they come before any device work: dummy aligned integers stand for device pointers), and the
new names in the header, the library and the ctypes table."""
import ctypes
import os

import numpy as np
import pytest
import torch

import meshclean_refs as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gsr_mesh_clean_bytes", "gsr_mesh_components", "gsr_mesh_select", "gsr_mesh_compact")


@pytest.mark.parametrize("name", ["ties", "interleaved"])
def test_reference_agrees_with_the_closure(name):
    import diff_gaussian_rasterization as dgr

    faces, V = MR.cases(dgr.MESH_CHUNK_FACES, dgr.MESH_WINDOW_VERTICES)[name]
    labels, tri_count = MR.components(faces, V)
    assert np.array_equal(labels, MR.closure_labels(faces, V))
    assert tri_count.sum() == len(faces) and np.all(tri_count[labels != np.arange(V)] == 0)
    if name == "ties":  # counts 7 at the labels 0, 19, 28, then 4 and 2: ties go to the lowest label
        assert {int(l): int(tri_count[l]) for l in np.unique(labels)} == {0: 7, 9: 4, 15: 2, 19: 7, 28: 7}
        kept = lambda k, m: np.flatnonzero(MR.kept_labels(labels, tri_count, k, m)).tolist()
        assert [kept(k, 0) for k in (1, 2, 3, 4)] == [[0], [0, 19], [0, 19, 28], [0, 9, 19, 28]]
        assert kept(4, 5) == [0, 19, 28] and kept(0, 3) == [0, 9, 19, 28] and kept(0, 0) == [0, 9, 15, 19, 28]


def test_the_refusals_come_before_any_device_work():
    import diff_gaussian_rasterization as dgr

    lib, d, big = dgr.lib, 0x1000, 1 << 40
    assert lib.gsr_mesh_clean_bytes(-1, 0) == 0 and lib.gsr_mesh_clean_bytes(0, 1 << 31) == 0
    assert lib.gsr_mesh_clean_bytes(1000, 2000) >= 1000 * 9 and lib.gsr_mesh_clean_bytes((1 << 31) - 1, (1 << 31) - 1) > 1 << 34
    comp = (10, 20, d, d, d, d, d, big, None)
    sel = (10, 20, d, d, d, 1, 0, d, big, d, None)
    cmp_ = (10, 20, d, d, d, d, d, big, 5, 5, d, d, d, None)
    edit = lambda a, i, v: a[:i] + (v,) + a[i + 1:]
    for bad in (edit(comp, 0, -1), edit(comp, 1, -1), edit(comp, 0, 1 << 31), edit(comp, 2, None), edit(comp, 3, None),
                edit(comp, 4, None), edit(comp, 5, None), edit(comp, 6, None), edit(comp, 0, 0)):
        assert lib.gsr_mesh_components(*bad) == -1, bad
    assert lib.gsr_mesh_components(*edit(comp, 7, 64)) == -2
    for bad in (edit(sel, 0, -1), edit(sel, 1, 1 << 31), edit(sel, 5, -1), edit(sel, 6, -1), edit(sel, 2, None),
                edit(sel, 3, None), edit(sel, 4, None), edit(sel, 7, None), edit(sel, 9, None)):
        assert lib.gsr_mesh_select(*bad) == -1, bad
    assert lib.gsr_mesh_select(*edit(sel, 8, 64)) == -2
    for bad in (edit(cmp_, 0, -1), edit(cmp_, 8, 11), edit(cmp_, 9, -1), edit(cmp_, 3, None), edit(cmp_, 11, None),
                edit(cmp_, 2, None), edit(cmp_, 4, None), edit(cmp_, 5, None), edit(cmp_, 6, None), edit(cmp_, 10, None),
                edit(cmp_, 12, None)):
        assert lib.gsr_mesh_compact(*bad) == -1, bad
    assert lib.gsr_mesh_compact(*edit(cmp_, 7, 64)) == -2
    assert lib.gsr_mesh_compact(0, 0, *([None] * 5), 0, 0, 0, None, None, None, None) == 0  # nothing to do: no launch
    assert lib.gsr_mesh_compact(10, 20, *([None] * 5), 0, 0, 0, None, None, None, None) == 0
    faces = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.mesh_components(faces, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.mesh_filter(torch.zeros(3, 3), faces)


def test_the_new_names_are_declared_exported_and_bound():
    import diff_gaussian_rasterization as dgr

    header = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    raw = ctypes.CDLL(dgr._lib.LIB_PATH)
    for n in NAMES:
        assert f" {n}(" in header and hasattr(raw, n) and n in dgr._lib.SIGNATURES
    assert "mesh_components" in dgr.__all__ and "mesh_filter" in dgr.__all__
    assert dgr.lib.gsr_abi_version() == 15
