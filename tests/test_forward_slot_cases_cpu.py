"""The cases of tests/forward_slot_cases.py have the property each is named after, and keep the conditions
composite_refs asks of a case: inputs a margin away from the blend's decisions in both precisions, and the plain-fp32 C
restatement within K / 2 of the float64 reference (so K leaves a kernel a factor of two over an independent fp32
implementation).  Seeds were chosen here, on the CPU, never from a kernel's output."""
import pytest
import torch

import composite_refs as R
import forward_slot_cases as S
from helpers import ROW_UNIT_CAP, assert_rows_close, rows_unit

CASES = S.cases()
IDS = [c.id for c in CASES]
U = 2.0 ** -24


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
    line = []
    for k in R.TENSORS:
        unit, w = assert_rows_close(cr[k], r64[k], r32[k], K=R.K_FORWARD / 2, what=f"{case.id} C restatement {k}")
        line.append(f"{k} {unit / U:.0f} / {w:.2f}")
    print(f"CREF {case.id}: unit x 2^-24 / worst ratio: " + ", ".join(line))


@pytest.mark.parametrize("case", [c for c in CASES if c.tiles == 1], ids=[c.id for c in CASES if c.tiles == 1])
def test_k10_formulation_stays_below_half_of_k(case):
    """the CPU emulation of K10's order of operations (never a reference): these inputs leave the backward's formulation
    half of each group's K, so a row over K on the GPU is not the moment expansion's own cancellation"""
    r64, r32 = R.references(case)
    emu = R.k10_emulation(case)
    for k in R.GROUPS:
        assert_rows_close(emu[k], r64[k], r32[k], K=R.K_GROUP[k] / 2, what=f"{case.id} K10 emulation {k}")


@pytest.mark.parametrize("name", ["interleave-64", "interleave-100", "last-63"])
def test_compacted_position_differs_from_chunk_index(name):
    """in every quadrant some entry that blends sits behind an entry that is irrelevant there"""
    case = _by(name)
    rel = S.quadrant_relevance(case)
    d = R.decisions(case)[0]
    for q in range(4):
        blends = d["blended"].reshape(d["L"], 16, 16)[:, (q // 2) * 8:(q // 2) * 8 + 8, (q % 2) * 8:(q % 2) * 8 + 8]
        blends = blends.reshape(d["L"], -1).any(dim=1)
        r, b = rel[:64, q], blends[:64]  # (the first chunk)
        pos = torch.cumsum(r.to(torch.int64), 0) - 1
        assert bool((pos[b] != torch.arange(r.numel())[b]).any()), f"{name}: quadrant {q}"
        assert not bool(rel[:, q].all()) and bool(rel[:, q].any())


@pytest.mark.parametrize("name,last", [("last-0", 1), ("last-63", 64), ("last-64", 65)])
def test_last_blended_entry(name, last):
    nc = R.references(_by(name))[0]["n_contrib"]
    assert int(nc.max()) == last and bool((nc == last).sum() >= 64), "the broad entry is the last one of most pixels"


@pytest.mark.parametrize("r", [1, 2, 3])
def test_residues(r):
    for name, chunk in ((f"res{r}-then-full", 0), (f"full-then-res{r}", 1)):
        case = _by(name)
        rel = S.quadrant_relevance(case)
        n = rel[64 * chunk:64 * chunk + 64].sum(dim=0)
        assert bool((n == 4 + r).all()), (name, n.tolist())
        assert bool(rel[64 * (1 - chunk):64 * (1 - chunk) + 64].all())
        assert int(R.references(case)[0]["n_contrib"].max()) > 64


def test_zero_opacity_among_live_ones():
    case = _by("zero-opacity")
    z = case.conic_opacity[case.lists[0], 3] == 0
    assert int(z.sum()) == 3 and not bool(z[0]) and not bool(z[-1])
    r64 = R.references(case)[0]
    rows = case.lists[0][z]
    assert not bool(torch.cat([r64[k][rows] for k in R.GROUPS], dim=1).any())


def test_partial_tiles():
    case = _by("20x20")
    assert case.tiles == 4 and case.W % 16 and case.H % 16 and bool(case.compute_locally.all())
