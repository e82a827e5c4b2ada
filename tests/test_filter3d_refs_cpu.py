"""CPU checks of tests/filter3d_refs.py -- the arbiter of the 3D smoothing filter's GPU tests -- against itself, and of the
host-side pieces of the feature (no kernel runs here)."""
import math

import numpy as np
import pytest
import torch

import filter3d_refs as R

SHAPES = [(N, C) for N in (1, 63, 64, 65, 257, 4099) for C in (1, 2, 37)] + \
         [(257, R.CAM_CHUNK), (257, R.CAM_CHUNK + 1), (65, 2 * R.CAM_CHUNK + 1)]


@pytest.mark.parametrize("N,C", SHAPES)
def test_every_pair_of_every_built_case_is_decisive(N, C):
    case = R.build_distance_case(N, C, seed=N + C)
    assert case["xyz"].shape == (N, 3) and case["xyz"].dtype == np.float32 and case["cams"].shape == (C, 40)
    _, _, m, valid = R.pairs64(case["xyz"], case["cams"], case["W"], case["H"])
    assert float(np.abs(m).min()) >= R.MARGIN
    # the margins' signs ARE the rule
    assert np.array_equal(valid, (m > 0).all(-1))


def test_the_built_cases_hold_the_intended_rows():
    case = R.build_distance_case(257, 1, seed=3)
    ref = R.filter_ref(case["xyz"], case["cams"], case["W"], case["H"])
    sp = case["special"]
    assert set(sp) == set(R.SPECIAL)
    v0 = ref["valid"][:, 0]
    assert v0[sp["inside_margin"]] and v0[sp["margin_y"]] and v0[sp["near_in"]]
    assert not v0[sp["outside_margin"]] and not v0[sp["near_out"]] and not v0[sp["behind_all"]]
    # `inside_margin` is off the screen: only the 15 % margin makes it count
    t = R.pairs64(case["xyz"], case["cams"], case["W"], case["H"])[0][sp["inside_margin"], 0]
    fx = case["W"] / (2.0 * float(case["cams"][0, 35]))
    assert 0.5 * case["W"] < abs(fx * t[0] / t[2]) < 0.65 * case["W"]
    assert 0 < ref["seen"].sum() < 257 and ref["gmax"] == ref["dist"].max()
    # unseen rows take the largest distance of the seen ones
    f = ref["filter"]
    assert np.all(f[~ref["seen"]] == f[ref["seen"]].max()) and np.all(f > 0)
    many = R.build_distance_case(4099, 37, seed=5)
    ref = R.filter_ref(many["xyz"], many["cams"], many["W"], many["H"])
    assert (ref["n_valid"] == 0).sum() > 10 and (ref["n_valid"] == 1).sum() > 10 and (ref["n_valid"] > 1).sum() > 10
    assert (ref["tz"] <= R.Z_NEAR).all(1).sum() >= 1, "no row behind every camera"
    # focal_max is not camera 0's
    fxs = many["W"] / (2.0 * many["cams"][:, 35].astype(np.float64))
    assert fxs.argmax() != 0 and R.focal_max64(many["cams"], many["W"]) == fxs.max()
    none = R.build_distance_case(257, 2, seed=1, unseen=True)
    ref = R.filter_ref(none["xyz"], none["cams"], none["W"], none["H"])
    assert not ref["seen"].any() and ref["gmax"] == 0.0 and not ref["filter"].any()


def test_packed_records_are_pack_camera_s():
    import diff_gaussian_rasterization as dgr

    cams = R.make_cameras(3, 64, 48, seed=2)
    block = R.pack_cameras(cams)
    for k, c in enumerate(cams):
        rs = dgr.GaussianRasterizationSettings(48, 64, math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5), None, 1.0,
                                               c.world_view_transform, c.full_proj_transform, 3, c.camera_center,
                                               False, False)
        assert np.array_equal(dgr.pack_camera(rs).numpy(), block[k])
    # the host-side focal_max: K1's float32 expression
    fm = dgr.filter3d_focal_max(block[:, 35], 64)
    want = max(np.float32(64) / (np.float32(2.0) * t) for t in block[:, 35])
    assert fm == float(want) and abs(fm - R.focal_max64(block, 64)) <= 2.0 ** -23 * fm


@pytest.mark.parametrize("N", [1, 63, 65, 1000])
def test_backward_restatement_is_the_autograd_of_the_forward(N):
    c = R.build_apply_case(N)
    x, o, f = (torch.from_numpy(c[k].astype(np.float64)) for k in ("x", "o", "f"))
    x.requires_grad_(True)
    o.requires_grad_(True)
    s, q = R._forward_torch(x, o, f)
    gs, go = torch.from_numpy(c["gs"].astype(np.float64)), torch.from_numpy(c["go"].astype(np.float64))
    ((s * gs).sum() + (q * go).sum()).backward()
    ds, do, Ms, Mo = R.apply_backward_ref(c["x"], c["o"], c["f"], c["gs"], c["go"])
    # both are exact formulas in float64: 1e-12 relative to the sum of the magnitudes of the terms of each element
    assert np.all(np.abs(x.grad.numpy() - ds) <= 1e-12 * Ms)
    assert np.all(np.abs(o.grad.numpy() - do) <= 1e-12 * Mo)
    assert np.isfinite(ds).all() and np.isfinite(do).all()


def test_the_two_forms_of_the_forward_restatement_agree():
    """apply_forward_ref evaluates opacity_eff as o + log c - log1p((1 - c) e^o) (no cancelling addends: the value),
    _forward_torch as log(sigma c) - log(1 - p) (no cancelling derivative terms: the autograd check above)"""
    c = R.build_apply_case(1000)
    s, q, Ms, Mo = R.apply_forward_ref(c["x"], c["o"], c["f"])
    x, o, f = (torch.from_numpy(c[k].astype(np.float64)) for k in ("x", "o", "f"))
    s2, q2 = R._forward_torch(x, o, f)
    nz = c["f"][:, 0] != 0
    assert np.all(np.abs(s2.numpy() - s)[nz] <= 4e-16 * Ms[nz])
    # log sigma and log(1 - p) are each rounded to 2^-53 of their own magnitude, at most |o| + L + log 2
    bound = 8 * 2.0 ** -53 * (np.abs(c["o"].astype(np.float64)) + Mo + 1.0)
    assert np.all(np.abs(q2.numpy() - q)[nz] <= bound[nz])


def test_forward_restatement_is_the_definition():
    """s'_k = sqrt(s_k^2 + f^2), o' = sigmoid(o) prod s_k / s'_k, where the plain formulas are well conditioned"""
    c = R.build_apply_case(1000)
    s, q, _, _ = R.apply_forward_ref(c["x"], c["o"], c["f"])
    x, o, f = (c[k].astype(np.float64) for k in ("x", "o", "f"))
    want = np.sqrt(np.exp(2 * x) + f * f)
    assert np.allclose(np.exp(s), want, rtol=1e-12, atol=0)
    big = (f[:, 0] >= 1e-3 * np.exp(x).min(1))  # (below that the plain quotient loses c's distance from 1)
    o2 = 1.0 / (1.0 + np.exp(-o)) * np.prod(np.exp(x) / want, axis=1, keepdims=True)
    assert big.sum() > 100 and np.allclose(1.0 / (1.0 + np.exp(-q[big])), o2[big], rtol=1e-9, atol=0)


@pytest.mark.parametrize("N", [1, 63, 65, 1000])
def test_zero_filter_is_the_identity(N):
    c = R.build_apply_case(N)
    z = np.zeros_like(c["f"])
    s, q, _, _ = R.apply_forward_ref(c["x"], c["o"], z)
    assert np.array_equal(s, c["x"].astype(np.float64)) and np.array_equal(q, c["o"].astype(np.float64))
    ds, do, _, _ = R.apply_backward_ref(c["x"], c["o"], z, c["gs"], c["go"])
    assert np.array_equal(ds, c["gs"].astype(np.float64)) and np.array_equal(do, c["go"].astype(np.float64))
    # the float32 evaluation: bit for bit, also for the rows of the grid that have f == 0
    s32, q32 = R.apply_forward_f32(c["x"], c["o"], c["f"])
    ds32, do32 = R.apply_backward_f32(c["x"], c["o"], c["f"], c["gs"], c["go"])
    ident = c["f"][:, 0] == 0
    for got, src in ((s32, c["x"]), (q32, c["o"]), (ds32, c["gs"]), (do32, c["go"])):
        assert got.dtype == np.float32 and np.array_equal(got[ident].view(np.int32), src[ident].view(np.int32))


def test_float32_evaluation_stays_within_a_few_units_of_float64():
    """what the GPU test derives the kernels' tolerance from: printed here, and bounded loosely so that a mistake in the
    float32 restatement cannot hand the kernels a tolerance of thousands of units (every output is a handful of
    float32 operations on well-conditioned quantities: 32 units of 2^-24 of its addends is generous)"""
    worst = {}
    for N in (1, 63, 65, 1000):
        c = R.build_apply_case(N)
        s, q, Ms, Mo = R.apply_forward_ref(c["x"], c["o"], c["f"])
        s32, q32 = R.apply_forward_f32(c["x"], c["o"], c["f"])
        ds, do, Mds, Mdo = R.apply_backward_ref(c["x"], c["o"], c["f"], c["gs"], c["go"])
        ds32, do32 = R.apply_backward_f32(c["x"], c["o"], c["f"], c["gs"], c["go"])
        for name, e in (("scaling_eff", R.worst_units(s32, s, Ms)), ("opacity_eff", R.worst_units(q32, q, Mo)),
                        ("d_scaling", R.worst_units(ds32, ds, Mds)), ("d_opacity", R.worst_units(do32, do, Mdo))):
            worst[name] = max(worst.get(name, 0.0), e)
    print("FILTER3D-REFS float32 numpy vs float64, worst error in units of 2^-24 of the addends:", worst)
    assert all(np.isfinite(v) and v <= 32.0 for v in worst.values()), worst


def test_bake_composed_with_the_activations_is_the_filtered_model():
    """exp(scaling_eff) = s' and sigmoid(opacity_eff) = o': bake()'s contract, on the float64 restatement"""
    c = R.build_apply_case(1000)
    s, q, _, _ = R.apply_forward_ref(c["x"], c["o"], c["f"])
    x, o, f = (c[k].astype(np.float64) for k in ("x", "o", "f"))
    u = f * f * np.exp(-2 * x)
    s_prime = np.exp(x) * np.sqrt(1.0 + u)
    coef = np.prod(1.0 / np.sqrt(1.0 + u), axis=1, keepdims=True)
    o_prime = coef / (1.0 + np.exp(-o))
    assert np.allclose(np.exp(s), s_prime, rtol=1e-12, atol=0)
    assert np.allclose(1.0 / (1.0 + np.exp(-q)), o_prime, rtol=1e-11, atol=0)


def test_switch_and_errors_without_a_device():
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr

    assert gr.get_filter3d() is False
    gr.set_filter3d(True)
    assert gr.get_filter3d() is True
    gr.set_filter3d(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.filter3d_apply(torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dgr.compute_filter3d(torch.zeros(4, 3), torch.zeros(1, 40), 64, 48)
    lib = dgr._lib.lib
    assert [lib.gsr_filter3d_num_partials(n) for n in (-1, 0, 1, 256, 257)] == [0, 0, 1, 1, 2]
    d = 0x1000
    assert lib.gsr_filter3d_apply_forward(0, None, None, None, None, None, None) == 0
    assert lib.gsr_filter3d_apply_forward(4, None, d, d, d, d, None) == -1
    assert lib.gsr_filter3d_apply_backward(0, *([None] * 7), None) == 0
    assert lib.gsr_filter3d_apply_backward(4, d, d, d, d, d, d, None, None) == -1
    assert lib.gsr_filter3d_distance(0, 3, None, None, 64, 48, None, None, None, None) == 0
    assert lib.gsr_filter3d_distance(4, 3, d, d, 0, 48, d, d, d, None) == -1
    assert lib.gsr_filter3d_distance(4, 3, d, None, 64, 48, d, d, d, None) == -1
    assert lib.gsr_filter3d_finalize(4, d, d, None, 1, None, 100.0, d, None) == -1  # neither partials nor a global max
    assert lib.gsr_filter3d_finalize(4, d, d, d, 2, None, 100.0, d, None) == -1     # not num_partials(4)
    assert lib.gsr_filter3d_finalize(4, d, d, d, 1, None, 0.0, d, None) == -1       # focal_max
    assert lib.gsr_abi_version() == 15
