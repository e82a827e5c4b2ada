"""The inputs, the references and the per-row check of tests/test_gpu_projection_rows.py, without a GPU: the generators
produce what they are named for and keep their margins; every case's float32 reference stays under the cap of
helpers.assert_rows_close; the plain-C float32 restatement with its hand-written backward (oracle/cref.py) passes the
check on every activated-path case; and the check catches a single corrupted row that the norm-wise and p99 measures of
tests/test_gpu_parity.py let through."""
import pytest
import torch

import projection_refs as R
from helpers import KEYS, ROW_UNIT_CAP, assert_rows_close, elem_excess, rel_err, rows_unit
from oracle import cref as C
from oracle import torch_oracle as O

U = 2.0 ** -24
N_GEN = 257
LOWER = {"plain": 0, "jclamp": 1, "near": 1, "aniso": 2, "aniso_mild": 2, "tiny": 0, "huge": 1, "clamped": 2, "behind": 0,
         "raw": 1}
ACT_CASES = [c for c in R.CASES if c.form == "act"]


def _radii64(act, cam, deg):
    tx, ty = R.tanfov(cam)
    with torch.no_grad():
        out = O.preprocess(*[act[k].double() for k in KEYS], viewmatrix=cam.world_view_transform,
                           projmatrix=cam.full_proj_transform, campos=cam.camera_center, W=cam.image_width,
                           H=cam.image_height, tanfovx=tx, tanfovy=ty, sh_degree=deg, return_aux=True)
    return out[3], out[6]


# ------------------------------------------------------------------------------------------------ 1. generators
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("fam,deg", [(f, d) for f in R.FAMILIES for d in (3, LOWER[f])])
def test_generator_properties(fam, deg, B):
    N, (W, H) = N_GEN, R.FRAMES[0]
    ins, cams = R.family(fam, N, W, H, deg, seed=11, B=B)
    again, _ = R._family.__wrapped__(fam, N, W, H, deg, 11, B, 1.0, 16)  # past the cache: drawn anew
    assert all(torch.equal(ins[k], again[k]) for k in ins), "the generator is not deterministic"
    other, _ = R._family.__wrapped__(fam, N, W, H, deg, 12, B, 1.0, 16)
    assert not torch.equal(other[next(iter(other))], ins[next(iter(ins))]), "the seed is ignored"
    act = R.activate(ins) if fam == "raw" else ins
    assert all(v.dtype == torch.float32 and v.shape[0] == N for v in ins.values())
    assert not bool(R.margin_violations(act, cams, W, H, deg).any())
    # the margins, spelled out once more for camera 0 (margin_violations is what the generator itself used)
    g = R.geometry(act, cams[0], W, H, deg)
    f = g["front"]
    assert float((g["t"][:, 2] - R.NEAR).abs().min()) >= R.M_NEAR
    assert float(R._frac_dist(g["r3"][f]).min()) >= R.M_RADIUS
    assert float(g["colour"][f].abs().min()) >= R.M_COLOUR
    assert float(torch.minimum((g["rx"][f] - 1).abs(), (g["ry"][f] - 1).abs()).min()) >= R.M_JCLAMP
    r = torch.ceil(g["r3"][f])
    for c in (g["px"][f], g["py"][f]):
        assert float(torch.minimum(R._frac_dist((c - r) / 16), R._frac_dist((c + r) / 16)).min()) >= R.M_TILE
    # rows of the kind the family is named for: at least N // 8; at most half of the rows culled
    radii, clamped = _radii64(act, cams[0], deg)
    vis = radii > 0
    culled_everywhere = ~vis
    for cam in cams[1:]:
        culled_everywhere &= ~(_radii64(act, cam, deg)[0] > 0)
    assert int((~vis).sum()) <= N // 2 and int(culled_everywhere.sum()) <= N // 2
    s = act["scales"].double()
    kind = {
        "plain": vis,
        "jclamp": vis & ((g["rx"] > 1) | (g["ry"] > 1)),
        "near": vis & (g["t"][:, 2] < 0.5),
        "aniso": s.amax(1) / s.amin(1) >= 200.0,
        "aniso_mild": s.amax(1) / s.amin(1) >= 2.0,
        "tiny": s.amax(1) <= 2e-7,
        "huge": s.amin(1) >= 2.0,
        "behind": ~vis,
        "raw": (ins["rotation"].norm(dim=1) - 1).abs() > 0.5 if fam == "raw" else None,
    }
    if fam == "clamped":
        n_cl = clamped.sum(dim=1)
        for k in (1, 2, 3):
            assert int((vis & (n_cl == k)).sum()) >= N // 8, f"rows with {k} clamped channels"
    else:
        assert int(kind[fam].sum()) >= N // 8, f"{fam}: {int(kind[fam].sum())} rows of its kind"
    if fam == "jclamp":  # both axes, both signs
        t = g["t"]
        for axis, rr in ((0, g["rx"]), (1, g["ry"])):
            for sg in (1, -1):
                assert int((vis & (rr > 1) & (torch.sign(t[:, axis]) == sg)).sum()) >= 1, (axis, sg)
    if fam == "behind":
        assert int((g["t"][:, 2] < 0).sum()) >= N // 8 and int((f & ~vis).sum()) >= N // 16, "behind / off screen"


# ------------------------------------------------------------------------------------------------ 2. the cap
@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_cap_holds_for_every_gpu_case(case):
    r64, r32 = case.references()
    assert torch.equal(r64["radii"], r32["radii"]) and torch.equal(r64["clamped"], r32["clamped"]), \
        "a radius or a clamp bit flips between the float32 and the float64 oracle: the margins do not do their job"
    for k in case.tensors():
        pairs = [(r64[k][b], r32[k][b]) for b in range(case.B)] if k in R.OUTPUTS else [(r64[k], r32[k])]
        unit = max(rows_unit(a, b) for a, b in pairs)
        assert unit <= ROW_UNIT_CAP, f"{case.id} {k}: unit {unit / U:.0f} x 2^-24"
    assert int((r64["radii"] > 0).sum()) > 0, "nothing visible: the case checks nothing"


# ------------------------------------------------------------------------------------------------ 3. C restatement
def _c_run(case):
    """the float32 C restatement on an activated-path case -> dict of its outputs [N,...] and gradients"""
    ins, cams = case.inputs()
    cam = cams[0]
    tx, ty = R.tanfov(cam)
    kw = dict(viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center,
              W=case.W, H=case.H, tanfovx=tx, tanfovy=ty, sh_degree=case.deg, scale_modifier=case.sm)
    m2, rgb, co, radii, depths, cov3D, clamped = C.preprocess_forward(*[ins[k] for k in KEYS], **kw)
    G2, Gco, Grgb = R.upstream(1, case.N)
    grads = C.preprocess_backward(ins["means3D"], ins["scales"], ins["rotations"], ins["shs"], radii, cov3D, clamped,
                                  G2[0], Gco[0], Grgb[0], **kw)
    out = dict(means2D=m2, depths=depths, conic_opacity=co, rgb=rgb, cov3D=cov3D, radii=radii, clamped=clamped)
    out.update(zip(R.GRADS_ACT, grads))
    return out


def _ref_of(case, r, k):
    return r[k][0] if k in R.OUTPUTS else r[k]


@pytest.mark.parametrize("case", ACT_CASES, ids=[c.id for c in ACT_CASES])
def test_c_restatement_passes_the_row_check(case):
    """Worst ratio over these cases, per tensor (printed): EXPERIMENTS.md, 'Projection rows against float64'."""
    r64, r32 = case.references()
    got = _c_run(case)
    assert torch.equal(got["radii"], r64["radii"][0]), "radii"
    assert torch.equal(got["clamped"].bool(), r64["clamped"][0]), "clamped"
    for k in case.tensors():
        unit, worst = assert_rows_close(got[k].reshape(_ref_of(case, r64, k).shape), _ref_of(case, r64, k),
                                        _ref_of(case, r32, k), what=f"C {case.id} {k}")
        print(f"ROWS cref {case.id} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")


# ------------------------------------------------------------------------------------------------ 4. teeth
def _case(fam, N):
    return next(c for c in ACT_CASES if c.fam == fam and c.N == N and c.deg == 3)


def test_a_small_wrong_row_is_caught_and_the_tensor_wide_measures_miss_it():
    """one row of d_scales off by 1 % of its own value: the per-row check raises; rel_err < 1e-4 and
    elem_excess(q = 0.99) <= 1 (tests/test_gpu_parity.py's two measures) both still pass -- the gap, on record"""
    case = _case("plain", 1031)
    r64, r32 = case.references()
    good = _c_run(case)["d_scales"]
    ref = r64["d_scales"]
    s = ref.abs().amax(dim=1)
    live = torch.nonzero(s > 0).flatten()
    assert float(s[live].max() / s[live].min()) > 1e2, "the rows do not span two decades: pick another scene"
    row = int(live[s[live].argmin()])
    bad = good.clone()
    bad[row] *= 1.01
    assert_rows_close(good, ref, r32["d_scales"], what="uncorrupted")
    with pytest.raises(AssertionError, match=f"row {row}"):
        assert_rows_close(bad, ref, r32["d_scales"], what="corrupted")
    assert rel_err(bad, ref) < 1e-4 and elem_excess(bad, ref) <= 1


def test_a_missing_jacobian_clamp_multiplier_is_caught():
    """one component of one Jacobian-clamp row's d_means3D as K11 would give it without the zero multiplier"""
    case = _case("jclamp", 1031)
    ins, cams = case.inputs()
    r64, r32 = case.references()
    g = R.geometry(ins, cams[0], case.W, case.H, case.deg)
    Gco = R.upstream(1, case.N)[1][0]
    front = g["front"]
    sub = {k: v[front] for k, v in ins.items()}
    delta = torch.zeros(case.N, 3, dtype=torch.float64)
    delta[front] = R.conic_grad_means(sub, cams[0], case.W, case.H, Gco[front, :3], straight_through=True) - \
        R.conic_grad_means(sub, cams[0], case.W, case.H, Gco[front, :3])
    hit = (r64["radii"][0] > 0) & (g["rx"] > 1) & (Gco.abs().amax(1) > 0)
    inside = (r64["radii"][0] > 0) & (g["rx"] < 1) & (g["ry"] < 1)
    assert float(delta[inside].abs().max()) == 0.0, "rows inside the limit: the two variants are the same"
    rows = torch.nonzero(hit & (delta[:, 0] != 0)).flatten()
    assert rows.numel() >= 8
    good = _c_run(case)["d_means3D"]
    assert_rows_close(good, r64["d_means3D"], r32["d_means3D"], what="uncorrupted")
    for row in rows[:8].tolist():
        bad = good.clone()
        bad[row, 0] += float(delta[row, 0])
        with pytest.raises(AssertionError, match=f"row {row}, column 0"):
            assert_rows_close(bad, r64["d_means3D"], r32["d_means3D"], what="no zero multiplier")


def test_a_nan_and_a_nonzero_culled_row_are_caught():
    case = _case("behind", 257)
    r64, r32 = case.references()
    good = _c_run(case)
    culled = torch.nonzero(r64["radii"][0] <= 0).flatten()
    vis = torch.nonzero(r64["radii"][0] > 0).flatten()
    assert culled.numel() and vis.numel()
    bad = good["rgb"].clone()
    bad[int(vis[3]), 1] = float("nan")
    with pytest.raises(AssertionError, match=f"row {int(vis[3])}, column 1"):
        assert_rows_close(bad, r64["rgb"][0], r32["rgb"][0], what="NaN")
    for k in ("rgb", "d_scales", "d_shs"):
        bad = good[k].clone().reshape(case.N, -1)
        bad[int(culled[1]), -1] = 1e-30
        with pytest.raises(AssertionError, match=f"row {int(culled[1])}"):
            assert_rows_close(bad.reshape(r64[k].shape[-good[k].dim():]), _ref_of(case, r64, k), _ref_of(case, r32, k),
                              what="culled row not zero")


def test_the_cap_is_asserted_before_the_result_is_looked_at():
    ref = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64)
    with pytest.raises(AssertionError, match="over the cap"):
        assert_rows_close(ref.float(), ref, ref * (1 + 2 * ROW_UNIT_CAP))
    unit, worst = assert_rows_close(ref.float(), ref, ref.float())
    assert unit == 4 * U and worst == 0.0
    unit, worst = assert_rows_close(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, 3))
    assert worst == 0.0
