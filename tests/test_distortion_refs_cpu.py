"""CPU checks of the depth distortion references (tests/distortion_refs.py).

* on every case, the closed-form float64 restatement of the header's backward (e, q, u) equals autograd through the
  pairwise Definition to 1e-11 of each group's largest value, and D = A S, the identity behind the totals;
* the float32 reference stays under helpers.ROW_UNIT_CAP for every compared group of every case, `far-thin` included (a
  case that does not gets other inputs, never another cap);
* on `far-thin`, raw power sums in float32 are off by more than the cap."""
import pytest
import torch

import distortion_refs as DR
from helpers import ROW_UNIT_CAP, rows_unit

U = 2.0 ** -24
CASES = DR.cases()
RUNS = [(c, None) for c in CASES] + [(c, m) for c in CASES if c.id == DR.MAPPING_CASE for m in ("inverse", "ndc")]


@pytest.mark.parametrize("case,mapping", RUNS, ids=[c.id + ("-" + m if m else "") for c, m in RUNS])
def test_closed_form_equals_float64_autograd_and_the_unit_is_under_the_cap(case, mapping):
    r64, r32 = DR.references(case, mapping)
    cf = DR.closed_form(case, mapping)
    for k in DR.GROUPS:
        scale = float(r64[k].abs().max()) if r64[k].numel() else 0.0
        err = float((cf[k] - r64[k]).abs().max()) if r64[k].numel() else 0.0
        print(f"DISTORTION closed form {case.id} {k}: error {err:.3g}, largest value {scale:.3g}")
        # (+ 1e-13 |m|: a single blended entry has an exactly zero gradient, the closed form's w m / w is off by an fp64 ulp)
        floor = 1e-13 * max(1.0, float(DR.depths_of(case).max())) if case.P else 0.0
        assert err <= 1e-11 * scale + floor, f"{case.id} {k}: {err} > 1e-11 x {scale}"
    assert float((r64["D"] - r64["A"] * r64["S"]).abs().max()) <= 1e-12 * max(float(r64["D"].max()), 1e-300)
    assert float(r64["D"].max()) > 0 or case.family in ("lengths", "inert"), "an empty map compares nothing"
    seen = r64["A"].reshape(-1) > 0
    for k in DR.MAPS + DR.GROUPS:
        rows = seen if k in ("mu", "S") else slice(None)
        unit = rows_unit(r64[k][rows], r32[k][rows])
        print(f"DISTORTION unit {case.id} {k}: {unit / U:.0f} x 2^-24")
        assert unit <= ROW_UNIT_CAP, f"{case.id} {k}: change the inputs of this case"


def test_far_thin_is_where_raw_power_sums_fail():
    """the family's point: depths ascending within [50, 50.5], and in float32 sum w m^2 - (sum w m)^2 / sum w is off by
    more than the cap allows while the pairwise reference is not (asserted above)"""
    for case in [c for c in CASES if c.family == "far-thin"]:
        d = DR.depths_of(case)[case.lists[0]]
        assert float(d.min()) >= 50.0 and float(d.max()) <= 50.5 and bool((d[1:] >= d[:-1]).all())
        r64, _ = DR.references(case)
        m2, co, dep = case.means2D, case.conic_opacity, DR.depths_of(case)
        (*_, w, m), = DR._tiles(case, m2, co, dep, "depth")
        raw = (w * m * m).sum(0) - (w * m).sum(0) ** 2 / w.sum(0)
        S = r64["S"].reshape(-1)
        assert float(((raw.double() - S).abs() / S).max()) > ROW_UNIT_CAP
