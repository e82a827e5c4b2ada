"""No GPU: the references of tests/contrib_refs.py are what tests/test_gpu_contrib_rows.py needs them to be, and the
C-ABI of the contribution statistics (include/gsraster.h: gsr_render_contrib, gsr_contrib_merge_rows) is in place.

On every case of composite_refs.cases(): `hits` is the same in float32 and float64 (the cases keep 2^-10 from both of the
blend's decisions); the float32 reference's per-row error on wmax and wsum is under helpers.ROW_UNIT_CAP; the rows the
families promise to leave unblended are there (the fillers of `deep-long`, the tail behind every pixel's stop of the
saturating cases); and the weights of a pixel add up to what the pixel lost: sum_i wsum_i = sum over pixels of
(1 - final_T), against composite_refs.references in float64."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

import composite_refs as R
import contrib_refs as CR
from helpers import ROW_UNIT_CAP, rows_unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
CASES = R.cases()
IDS = [c.id for c in CASES]
NAMES = ("gsr_render_contrib", "gsr_contrib_merge_rows")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_facts(case):
    r64, r32 = CR.references(case)
    assert torch.equal(r64["hits"], r32["hits"]), f"{case.id}: float32 and float64 blend different pairs"
    for k in CR.COLUMNS:
        unit = rows_unit(r64[k], r32[k])
        print(f"CONTRIB-REF {case.id} {k}: unit {unit / U:.0f} x 2^-24")
        assert unit <= ROW_UNIT_CAP, f"{case.id} {k}: unit {unit / U:.0f} x 2^-24 over the cap"
    # hits, wmax and wsum vanish together, and a weight never exceeds the alpha clamp
    h0 = r64["hits"] == 0
    assert torch.equal(h0, r64["wmax"].reshape(-1) == 0) and torch.equal(h0, r64["wsum"].reshape(-1) == 0)
    assert case.P == 0 or float(r64["wmax"].max()) <= 0.99
    assert bool((r64["wsum"].reshape(-1) <= r64["hits"] * r64["wmax"].reshape(-1) * (1 + 1e-12)).all())
    nohit = int(h0.sum())
    if case.id == "deep-long":
        assert nohit >= 4100, nohit
    if case.family == "saturating":
        assert 15 <= nohit <= 22, nohit


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weights_add_up_to_the_lost_transmittance(case):
    r64, _ = CR.references(case)
    lost = float((1.0 - R.references(case)[0]["final_T"]).sum())  # (final_T is exactly 1 on tiles that are not ours)
    got = float(r64["wsum"].sum())
    assert abs(got - lost) <= 1e-11 * max(1.0, lost), (got, lost)


def test_entry_points_are_declared_bound_and_exported():
    from diff_gaussian_rasterization import _lib

    header = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is not declared in include/gsraster.h"
        assert n in _lib.SIGNATURES and hasattr(raw, n), n
    assert "no counterpart" in header[header.index("CONTRIBUTION"):header.index("int gsr_render_contrib(")]
    assert _lib.ABI_VERSION == 15 and _lib.lib.gsr_abi_version() == 15  # additive entry points: the ABI stays
    spec = importlib.util.spec_from_file_location("gsr_build_for_test", os.path.join(ROOT, "grendel-gs_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "contrib" in mod.UNITS and mod.UNITS.index("contrib") < mod.UNITS.index("api")
    assert any(h.endswith("composite_math.h") for h in mod.HEADERS)


def test_shared_math_header_is_the_only_copy():
    """composite.hip and contrib.hip include composite_math.h and neither restates what it holds
    (profiles/contrib_shared_math_isa.txt: K8 / K10 compile to the same code as before the move)"""
    csrc = os.path.join(ROOT, "grendel-gs_amd", "csrc")
    hdr = open(os.path.join(csrc, "composite_math.h")).read()
    for needle in ("entry_exponent(", "entry_alpha_raw(", "entry_power_ok(", "entry_opacity_term(", "load_entry(",
                   "constexpr float ALPHA_MIN", "constexpr float T_STOP", "constexpr float LOG2E", "#define GSR_LOG2O 1"):
        assert needle in hdr, needle
    for unit in ("composite.hip", "contrib.hip"):
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "composite_math.h"' in src, unit
        for needle in ("float entry_exponent(", "float entry_alpha_raw(", "bool entry_power_ok(", "Entry load_entry(",
                       "constexpr float ALPHA_MIN", "#define GSR_LOG2O"):
            assert needle not in src, f"{unit} restates {needle}"
    isa = open(os.path.join(ROOT, "profiles", "contrib_shared_math_isa.txt")).read().split("\n")
    lines = [l for l in isa if l.strip()]
    assert len(lines) >= 6 and all(l.startswith("SAME") for l in lines), "a composite kernel changed with the move"


def test_validation_happens_before_any_device_work():
    """dummy non-zero integers stand for device pointers: every call below is refused, or returns, before anything is
    dereferenced or launched"""
    from diff_gaussian_rasterization import _lib

    lib = _lib.lib
    d = 0x1000

    def contrib(P, W, H, ptrs=None, band=(0, 0)):
        p = [d] * 9 if ptrs is None else ptrs
        return lib.gsr_render_contrib(P, W, H, *p[:6], band[0], band[1], *p[6:], None)

    assert contrib(-1, 16, 16) == -1
    assert contrib(1, 0, 16) == -1 and contrib(1, 16, 0) == -1 and contrib(1, -16, 16) == -1
    assert contrib(0, 16, 16, [None] * 9) == 0          # nothing to do, nothing touched
    assert contrib(0, 0, 16, [None] * 9) == -1          # the frame is checked first
    for missing in (0, 2, 3, 4, 5, 6, 7, 8):            # every pointer but point_list (index 1: all lists may be empty)
        p = [d] * 9
        p[missing] = None
        assert contrib(1, 16, 16, p) == -1, missing
    assert lib.gsr_contrib_merge_rows(-1, *([d] * 7), None) == -1
    assert lib.gsr_contrib_merge_rows(0, *([None] * 7), None) == 0
    for missing in range(7):
        p = [d] * 7
        p[missing] = None
        assert lib.gsr_contrib_merge_rows(5, *p, None) == -1, missing
