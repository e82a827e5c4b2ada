"""CPU checks of the feature-map references (tests/features_refs.py) and of the switch that asks for the map.

* the closed forms of include/gsraster.h, written out in float64 without autograd, equal autograd through
  oracle.torch_oracle.render (three channels at a time, bg = 0) to 1e-12 of each tensor's largest value on the `lengths`
  and `edges` families at C = 4, and across the channel sweep on the cases the GPU sweep uses;
* the float32 reference stays under helpers.ROW_UNIT_CAP for every group of every (case, C) the GPU tests use (a case
  that does not gets other features, never another cap);
* the CPU emulation of composite_features_backward_kernel's order of operations stays within HALF of each K of
  features_refs.K_GROUP on every (case, C) of EMULATED (the kernel keeps a factor of two over its own formulation);
* features = 1 / depth with C = 1 reproduces invdepth_refs.references: the inverse-depth map is the one-channel case;
* with gaussian_renderer.set_features off, cuda_args carry none of the new keys."""
import pytest
import torch

import composite_refs as R
import features_refs as FR
import invdepth_refs as IR
from helpers import ROW_UNIT_CAP, rows_unit
from oracle import torch_oracle as O

U = 2.0 ** -24
CASES = R.cases()
IDS = [c.id for c in CASES]
EXACT = [c for c in CASES if c.family in ("lengths", "edges")]
# the channel sweep of tests/test_gpu_features_pixels.py: the `edges` family and one `lengths` case
SWEEP_CASES = [c for c in CASES if c.family == "edges"] + [c for c in CASES if c.id == "lengths-65"]
USED = [(c, 4) for c in CASES] + [(c, C) for c in SWEEP_CASES for C in FR.SWEEP]
# the emulation is a Python loop per (tile, entry, quadrant): every case at C = 4 (one narrow chunk), and two chunks with
# a partial second one on the smallest cases of the sweep
EMULATED = [(c, 4) for c in CASES if c.P > 0] + \
           [(c, FR.CH + 1) for c in CASES if c.id in ("edges-8x8", "edges-17x17", "lengths-65")]


def _ids(pairs):
    return [f"{c.id}-C{C}" for c, C in pairs]


def test_inputs_are_float32_in_range_and_the_map_shares_k8s_decisions():
    assert FR.CAP >= 64 and FR.CH >= 1 and len(set(FR.SWEEP)) == len(FR.SWEEP) and max(FR.SWEEP) <= FR.CAP
    for case in CASES:
        f, g = FR.features_of(case, 4), FR.g_of(case, 4)
        assert f.dtype == torch.float32 and f.shape == (case.P, 4)
        assert g.dtype == torch.float32 and g.shape == (4, case.H, case.W)
        assert case.P == 0 or (float(f.min()) >= 0.0 and float(f.max()) <= 1.0)
        r64, r32 = FR.references(case, 4)
        c64, _ = R.references(case)
        assert torch.equal(r64["n_contrib"], c64["n_contrib"]) and torch.equal(r32["n_contrib"], c64["n_contrib"])
        assert torch.equal(r64["final_T"], c64["final_T"])


@pytest.mark.parametrize("case,C", [(c, 4) for c in EXACT] + [(c, C) for c in SWEEP_CASES[-2:] for C in FR.SWEEP],
                         ids=_ids([(c, 4) for c in EXACT] + [(c, C) for c in SWEEP_CASES[-2:] for C in FR.SWEEP]))
def test_closed_forms_equal_float64_autograd(case, C):
    r64, _ = FR.references(case, C)
    cf = FR.closed_form(case, C)
    for k in ["map"] + FR.GROUPS:
        scale = float(r64[k].abs().max()) if r64[k].numel() else 0.0
        err = float((cf[k] - r64[k]).abs().max()) if r64[k].numel() else 0.0
        print(f"FEATURES closed form {case.id} C={C} {k}: error {err:.3g}, largest value {scale:.3g}")
        assert err <= 1e-12 * scale, f"{case.id} C={C} {k}: {err} > 1e-12 x {scale}"
    # pixels of tiles that are not ours are exactly 0 in the reference too
    m = r64["map"].t().reshape(C, case.H, case.W)
    for t in range(case.tiles):
        if not bool(case.compute_locally[t]):
            x0, y0, x1, y1 = case.tile_box(t)
            assert not bool(m[:, y0:y1, x0:x1].any())


@pytest.mark.parametrize("case,C", USED, ids=_ids(USED))
def test_float32_reference_is_under_the_row_unit_cap(case, C):
    r64, r32 = FR.references(case, C)
    for k in ["map"] + FR.GROUPS:
        unit = rows_unit(r64[k], r32[k])
        print(f"FEATURES unit {case.id} C={C} {k}: {unit / U:.0f} x 2^-24")
        assert unit <= ROW_UNIT_CAP, f"{case.id} C={C} {k}: change the features of this case"


def _worst_ratio(got, ref64, ref32):
    unit = rows_unit(ref64, ref32)
    s = ref64.abs().amax(dim=1, keepdim=True)
    err = (got.double() - ref64).abs()
    assert not bool(err[(s == 0).expand_as(err)].any()), "a row of zeros in the reference is not zero"
    live = (s > 0).reshape(-1)
    return float((err[live] / (unit * s[live])).max()) if bool(live.any()) else 0.0


@pytest.mark.parametrize("case,C", EMULATED, ids=_ids(EMULATED))
def test_the_kernels_order_of_operations_stays_within_half_of_k(case, C):
    r64, r32 = FR.references(case, C)
    em = FR.kernel_emulation(case, C)
    for k in FR.GROUPS:
        w = _worst_ratio(em[k], r64[k], r32[k])
        print(f"FEATURES emulation {case.id} C={C} {k}: worst ratio {w:.3g} (K = {FR.K_GROUP[k]})")
        assert 2.0 * w <= FR.K_GROUP[k], f"{case.id} C={C} {k}: the formulation alone takes {w:.3g} of K = {FR.K_GROUP[k]}"
    assert all(v <= 16 for v in FR.K_GROUP.values()) and FR.K_MAP == 8 and FR.K_GROUP["d_features"] == 8


@pytest.mark.parametrize("case", [c for c in EXACT if c.P > 0], ids=[c.id for c in EXACT if c.P > 0])
def test_one_channel_of_inverse_depths_is_the_inverse_depth_reference(case):
    """the Definition with C = 1 and f = 1 / depth against invdepth_refs.references: the same map, the same geometry
    gradients, and dL/df = -depth^2 dL/ddepth"""
    dt = torch.float64
    dep = IR.depths_of(case).to(dt)
    m2 = case.means2D.clone().to(dt).requires_grad_(True)
    co = case.conic_opacity.clone().to(dt).requires_grad_(True)
    f = (1.0 / dep).reshape(-1, 1).clone().requires_grad_(True)
    rgb = torch.cat([f, torch.zeros(case.P, 2, dtype=dt)], dim=1)
    img, fT, nc = O.render(m2, co, rgb, None, None, case.compute_locally, bg=torch.zeros(3, dtype=dt), W=case.W, H=case.H,
                           binning=(case.point_list, case.ranges[:case.tiles], None))
    if img.requires_grad:
        gm, gc, gf = torch.autograd.grad((img[0] * IR.g_of(case).to(dt)).sum(), [m2, co, f])
    else:  # (an empty list: the map does not depend on the inputs)
        gm, gc, gf = torch.zeros_like(m2), torch.zeros_like(co), torch.zeros_like(f)
    i64, _ = IR.references(case)
    want = dict(invdepth=img[0].detach().reshape(-1, 1), d_means2D=gm, d_conic=gc[:, :3], d_opacity=gc[:, 3:],
                d_depth=-(gf.reshape(-1) / (dep * dep)).reshape(-1, 1))
    for k, v in want.items():
        scale = float(i64[k].abs().max())
        assert float((v - i64[k]).abs().max()) <= 1e-12 * scale, f"{case.id} {k}"


def test_the_switch_is_off_by_default_and_adds_no_key_when_off():
    import gaussian_renderer as gr
    import utils.general_utils as utils

    utils.set_args(utils.default_args(bsz=1))
    utils.set_cur_iter(1)
    strategy = type("S", (), {"world_size": 1, "rank": 0})()
    was = gr.get_features()
    try:
        gr.set_features(False)
        off = gr.get_cuda_args_final(strategy, "train")
        assert "features" not in off and not any("features" in k for k in off)
        gr.set_features(True)
        on = gr.get_cuda_args_final(strategy, "train")
        assert on["features"] is True and {k: v for k, v in on.items() if k != "features"} == off
    finally:
        gr.set_features(was)
