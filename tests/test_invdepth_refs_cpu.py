"""CPU checks of the inverse-depth references (tests/invdepth_refs.py) and of the switch that asks for the map.

* the closed forms of include/gsraster.h, written out in float64 without autograd, equal autograd through
  oracle.torch_oracle.render (rgb = (v, 0, 0), bg = 0) to 1e-12 of each tensor's largest value on the `lengths` and
  `edges` families;
* the float32 reference stays under helpers.ROW_UNIT_CAP for every group of every case (a case that does not gets other
  depths, never another cap);
* the CPU emulation of composite_invdepth_backward_kernel's order of operations stays within HALF of each K of
  invdepth_refs.K_GROUP on every case (the kernel keeps a factor of two over its own formulation);
* dL/dmeans3D = dL/ddepth x the view matrix's third column, against autograd of ([p,1] @ view)[2];
* with gaussian_renderer.set_invdepth off, cuda_args carry none of the new keys."""
import pytest
import torch

import composite_refs as R
import invdepth_refs as IR
from helpers import ROW_UNIT_CAP, rows_unit

U = 2.0 ** -24
CASES = R.cases()
IDS = [c.id for c in CASES]
EXACT = [c for c in CASES if c.family in ("lengths", "edges")]


def test_depths_are_float32_in_range_and_the_map_shares_k8s_decisions():
    for case in CASES:
        d = IR.depths_of(case)
        assert d.dtype == torch.float32 and d.shape == (case.P,)
        assert case.P == 0 or (float(d.min()) >= IR.DEPTH_LO and float(d.max()) <= IR.DEPTH_HI)
        r64, r32 = IR.references(case)
        c64, _ = R.references(case)
        assert torch.equal(r64["n_contrib"], c64["n_contrib"]) and torch.equal(r32["n_contrib"], c64["n_contrib"])
        assert torch.equal(r64["final_T"], c64["final_T"])


@pytest.mark.parametrize("case", EXACT, ids=[c.id for c in EXACT])
def test_closed_forms_equal_float64_autograd(case):
    r64, _ = IR.references(case)
    cf = IR.closed_form(case)
    for k in ["invdepth"] + IR.GROUPS:
        scale = float(r64[k].abs().max()) if r64[k].numel() else 0.0
        err = float((cf[k] - r64[k]).abs().max()) if r64[k].numel() else 0.0
        print(f"INVDEPTH closed form {case.id} {k}: error {err:.3g}, largest value {scale:.3g}")
        assert err <= 1e-12 * scale, f"{case.id} {k}: {err} > 1e-12 x {scale}"
    # pixels of tiles that are not ours are exactly 0 in the reference too
    inv = r64["invdepth"].reshape(case.H, case.W)
    for t in range(case.tiles):
        if not bool(case.compute_locally[t]):
            x0, y0, x1, y1 = case.tile_box(t)
            assert not bool(inv[y0:y1, x0:x1].any())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_reference_is_under_the_row_unit_cap(case):
    r64, r32 = IR.references(case)
    for k in ["invdepth"] + IR.GROUPS:
        unit = rows_unit(r64[k], r32[k])
        print(f"INVDEPTH unit {case.id} {k}: {unit / U:.0f} x 2^-24")
        assert unit <= ROW_UNIT_CAP, f"{case.id} {k}: change the depths of this case"


def _worst_ratio(got, ref64, ref32):
    unit = rows_unit(ref64, ref32)
    s = ref64.abs().amax(dim=1, keepdim=True)
    err = (got.double() - ref64).abs()
    assert not bool(err[(s == 0).expand_as(err)].any()), "a row of zeros in the reference is not zero"
    live = (s > 0).reshape(-1)
    return float((err[live] / (unit * s[live])).max()) if bool(live.any()) else 0.0


@pytest.mark.parametrize("case", [c for c in CASES if c.P > 0], ids=[c.id for c in CASES if c.P > 0])
def test_the_kernels_order_of_operations_stays_within_half_of_k(case):
    r64, r32 = IR.references(case)
    em = IR.kernel_emulation(case)
    for k in IR.GROUPS:
        w = _worst_ratio(em[k], r64[k], r32[k])
        print(f"INVDEPTH emulation {case.id} {k}: worst ratio {w:.3g} (K = {IR.K_GROUP[k]})")
        assert 2.0 * w <= IR.K_GROUP[k], f"{case.id} {k}: the formulation alone takes {w:.3g} of K = {IR.K_GROUP[k]}"
    assert all(v <= 16 for v in IR.K_GROUP.values()) and IR.K_MAP == 8


def test_depth_to_means3D_against_autograd():
    g = torch.Generator().manual_seed(3)
    P = 37
    p = torch.randn(P, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    view = torch.randn(4, 4, generator=g, dtype=torch.float64)
    radii = torch.randint(0, 3, (P,), generator=g).to(torch.int32)
    d_depth = torch.randn(P, generator=g, dtype=torch.float64)
    depth = (torch.cat([p, torch.ones(P, 1, dtype=torch.float64)], dim=1) @ view)[:, 2]
    seen = torch.where(radii > 0, depth, depth.detach())  # a culled row has no depth gradient
    want, = torch.autograd.grad((seen * d_depth).sum(), p)
    got = IR.depth_to_means3D(d_depth, radii, view)
    assert bool((radii <= 0).any()) and bool((radii > 0).any())
    assert float((got - want).abs().max()) <= 1e-15 * float(want.abs().max())
    assert not bool(got[radii <= 0].any())


def test_the_switch_is_off_by_default_and_adds_no_key_when_off():
    import gaussian_renderer as gr
    import utils.general_utils as utils
    from gaussian_renderer.loss_distribution import invdepth_weight

    utils.set_args(utils.default_args(bsz=1))
    utils.set_cur_iter(1)
    strategy = type("S", (), {"world_size": 1, "rank": 0})()
    was = gr.get_invdepth()
    try:
        gr.set_invdepth(False)
        off = gr.get_cuda_args_final(strategy, "train")
        assert "invdepth" not in off and not any("invdepth" in k for k in off)
        gr.set_invdepth(True)
        on = gr.get_cuda_args_final(strategy, "train")
        assert on["invdepth"] is True and {k: v for k, v in on.items() if k != "invdepth"} == off
    finally:
        gr.set_invdepth(was)
    # the official exponential schedule: log-linear between the ends, constant behind max_steps, 0 for (0, 0)
    assert invdepth_weight(0, 1.0, 0.01, 1000) == pytest.approx(1.0)
    assert invdepth_weight(500, 1.0, 0.01, 1000) == pytest.approx(0.1)
    assert invdepth_weight(5000, 1.0, 0.01, 1000) == pytest.approx(0.01)
    assert invdepth_weight(10, 0.0, 0.0, 1000) == 0.0 and invdepth_weight(-1, 1.0, 0.01, 1000) == 0.0
