"""The cases of tests/backward_slot_cases.py have the property each is named after, and keep the conditions
composite_refs asks of a case: inputs a margin away from the blend's decisions in both precisions, the plain-fp32 C
restatement within K / 2 of the float64 reference, and the CPU emulation of K10's order of operations below half of each
group's K (so a row over K on the GPU is not the moment expansion's own cancellation).  Seeds were chosen here, on the
CPU, never from a kernel's output."""
import pytest
import torch

import backward_slot_cases as B
import composite_refs as R
import forward_slot_cases as S
from helpers import ROW_UNIT_CAP, assert_rows_close, rows_unit

CASES = B.cases()
IDS = [c.id for c in CASES]


def _by(name):
    return [c for c in CASES if c.name == name][0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inputs_keep_away_from_the_decisions(case):
    mg = R.margins(case)
    r64, r32 = R.references(case)
    assert mg["same"] and torch.equal(r64["n_contrib"], r32["n_contrib"]), "the two precisions decide differently"
    assert mg["gap_a"] >= R.M and mg["gap_T"] >= R.M, mg
    assert mg["dev_a"] <= R.M / 16 and mg["dev_T"] <= R.M / 16, mg
    for k in R.TENSORS:
        assert rows_unit(r64[k], r32[k]) <= ROW_UNIT_CAP, k


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_c_restatement_passes_the_rule_with_half_of_k(case):
    r64, r32 = R.references(case)
    cr = R.cref_results(case)
    assert torch.equal(cr["n_contrib"], r64["n_contrib"])
    for k in R.TENSORS:
        assert_rows_close(cr[k], r64[k], r32[k], K=R.K_FORWARD / 2, what=f"{case.id} C restatement {k}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_k10_formulation_stays_below_half_of_k(case):
    r64, r32 = R.references(case)
    emu = R.k10_emulation(case)
    for k in R.GROUPS:
        assert_rows_close(emu[k], r64[k], r32[k], K=R.K_GROUP[k] / 2, what=f"{case.id} K10 emulation {k}")


@pytest.mark.parametrize("n", B.COUNTS)
def test_relevant_count_of_quadrant_0(n):
    """K10 compacts exactly n entries for (quadrant 0, the one chunk); the narrow splats leave the other quadrants none"""
    case = _by(f"count-{n}")
    got = B.walked_counts(case)
    assert got.shape[0] == 1 and int(got[0, 0]) == n, got.tolist()
    if 0 < n <= 17:
        assert got[0, 1:].tolist() == [0, 0, 0]
        # and they do not sit in the first n chunk positions: a slot's compacted position differs from its chunk index
        rel = S.quadrant_relevance(case)[:, 0]
        assert not bool(rel[:n].all())
    elif n:
        assert got[0, 1:].tolist() == [n, n, n]


@pytest.mark.parametrize("name,q0,others", [("q0-64-others-9", 64, 9), ("q0-24-others-7", 24, 7)])
def test_counts_differ_between_the_quadrants(name, q0, others):
    got = B.walked_counts(_by(name))
    assert got.tolist() == [[q0, others, others, others]], got.tolist()


def test_middle_chunk_is_all_fillers_for_three_quadrants():
    case = _by("middle-fillers")
    got = B.walked_counts(case)
    assert got.shape[0] == 3
    assert got[1, 1:].tolist() == [0, 0, 0] and int(got[1, 0]) > 0
    assert bool((got[0] > 0).all()) and bool((got[2] > 0).all()), "the chunks around it are walked in every quadrant"


@pytest.mark.parametrize("name,last", [("last-0", 1), ("last-63", 64), ("last-64", 65)])
def test_last_blended_entry(name, last):
    nc = R.references(_by(name))[0]["n_contrib"]
    assert int(nc.max()) == last and bool((nc == last).sum() >= 64), "the broad entry is the last one of most pixels"


def test_zero_opacity_among_live_ones():
    case = _by("zero-opacity")
    z = case.conic_opacity[case.lists[0], 3] == 0
    assert int(z.sum()) == 3 and not bool(z[0]) and not bool(z[-1])
    r64 = R.references(case)[0]
    rows = case.lists[0][z]
    assert not bool(torch.cat([r64[k][rows] for k in R.GROUPS], dim=1).any())


def test_every_pixel_takes_every_entry():
    case = _by("w-130")
    d = R.decisions(case)[0]
    assert d["L"] == 130 and bool(d["blended"].all())
    assert B.walked_counts(case).tolist() == [[64] * 4, [64] * 4, [2] * 4]


def test_partial_tile():
    case = _by("13x13")
    assert case.tiles == 1 and case.W == 13 and case.H == 13
    assert int(R.references(case)[0]["n_contrib"].max()) > 8
