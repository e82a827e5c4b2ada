"""3DGS-MCMC on the device (csrc/mcmc.hip, mcmc.MCMCStrategy) against the restatements of tests/mcmc_refs.py.

Integers (the relocation plan) are compared for equality.  Floating-point results are compared element by element with
bounds computed in fp64 from the reference values; every bound counts the roundings the kernel performs:

* relocation apply: the kernel evaluates o', D, f, log(f) and the logit in fp64 and rounds to fp32 at three places --
  log(f) once, the sum raw_scale + log(f) once, the logit once.  With u = 2^-24:
      |scale - ref| <= u |log f| + u |ref| + e64_f,      |opacity - ref| <= u |logit| + e64_o
  e64 is what the fp64 evaluation itself can be off by, from the reference's own terms (mcmc_refs.relocation: `cond_D`
  weighs term k of the alternating sum with the number of fp64 roundings behind it): e64_f = 2^-53 cond_D +
  2^-52 (1 + |log f|), e64_o = 2^-53 (8 / (1 - o') + 4 (1 + |logit|)) -- o' carries 8 ulp (log1p, quotient, expm1), the
  logit's quotient and logarithm two each.  Both are five orders below u.
* position noise: mcmc_refs.noise states its bound with the gate's slope explicit.
* regulariser: the added term carries exp's 2 u and a product (scale), or the sigmoid's 4 u absolute through o (1 - o)
  (opacity); the sum rounds once: u |result|.
"""
import math
import types

import numpy as np
import pytest
import torch

import densification_ops as D
import diff_gaussian_rasterization as dgr
import mcmc_refs as M
import synthetic_scene as S
from fused_optim import FusedAdam
from mcmc import MCMCStrategy

pytestmark = pytest.mark.gpu

MIN_OP = 0.005
SEED = 0x9abcdef012345678
U = M.U


def _opacities(P, dead_every=10, rng_seed=0):
    """fixed fp32 opacities in [0.01, 0.99], every `dead_every`-th row dead (0.002)"""
    o = (0.01 + 0.98 * np.random.default_rng(rng_seed + P).random(P)).astype(np.float32)
    if dead_every:
        o[::dead_every] = 0.002
    return o


def _plan(device, opacity, n_add, event=3, seed=SEED):
    src, count, totals = dgr.mcmc_relocate_plan(torch.from_numpy(opacity).to(device), n_add, MIN_OP, seed, event)
    return src.cpu().numpy(), count.cpu().numpy(), tuple(totals.cpu().tolist())


# ------------------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("n_add", [0, 3, 250])
@pytest.mark.parametrize("P", [1, 7, 1000, 5000])
def test_plan_is_the_restatement(device, P, n_add):
    opacity = _opacities(P, dead_every=10 if P > 1 else 0)
    src, count, totals = _plan(device, opacity, n_add)
    want_src, want_count, want_totals = M.relocate_plan(opacity, n_add, MIN_OP, SEED, 3)
    assert src.dtype == np.int32 and src.shape == (P + n_add,) and count.shape == (P,)
    assert np.array_equal(src, want_src) and np.array_equal(count, want_count) and totals == want_totals


def test_plan_special_cases(device):
    # all rows dead: no live row to draw from
    src, count, totals = _plan(device, np.full(100, 0.001, np.float32), 5)
    assert np.all(src == -1) and np.all(count == 0) and totals == (100, 0)
    # no row dead, but rows to add: only the new rows are destinations
    o = _opacities(300, dead_every=0)
    src, count, totals = _plan(device, o, 17)
    want = M.relocate_plan(o, 17, MIN_OP, SEED, 3)
    assert np.all(src[:300] == -1) and np.all(src[300:] >= 0) and count.sum() == 17 and totals == (0, 300)
    assert np.array_equal(src, want[0]) and np.array_equal(count, want[1])
    # one live row among 60 dead ones: every destination names it
    o = np.full(61, 0.001, np.float32)
    o[37] = 0.8
    src, count, totals = _plan(device, o, 0)
    assert np.all(np.delete(src, 37) == 37) and src[37] == -1 and count[37] == 60 and count.sum() == 60
    assert totals == (60, 1)
    # exactly min_opacity is dead, the next float above it is alive
    lo = np.float32(MIN_OP)
    o = np.array([lo, np.nextafter(lo, np.float32(1)), 0.5], dtype=np.float32)
    src, count, totals = _plan(device, o, 0)
    assert src[0] in (1, 2) and src[1] == -1 and src[2] == -1 and totals == (1, 2)
    # an empty model
    src, count, totals = dgr.mcmc_relocate_plan(torch.empty(0, device=device), 4, MIN_OP, SEED, 0)
    assert src.cpu().tolist() == [-1] * 4 and count.numel() == 0 and totals.cpu().tolist() == [0, 0]


def test_plan_is_deterministic_and_keyed_by_event_and_seed(device):
    o = _opacities(5000)
    a, b = _plan(device, o, 250, event=3), _plan(device, o, 250, event=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c, d = _plan(device, o, 250, event=4), _plan(device, o, 250, event=3, seed=SEED + 1)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[0], d[0])
    assert np.array_equal(a[0] >= 0, c[0] >= 0)  # the same destinations, other sources
    # buffers of the caller, larger than needed (the arena's): the same plan
    dev_o = torch.from_numpy(o).to(device)
    src, count, _ = dgr.mcmc_relocate_plan(dev_o, 250, MIN_OP, SEED, 3, torch.empty(9000, dtype=torch.int32, device=device),
                                           torch.empty(9000, dtype=torch.int32, device=device),
                                           torch.empty(30000, dtype=torch.int64, device=device))
    assert np.array_equal(src.cpu().numpy(), a[0]) and np.array_equal(count.cpu().numpy(), a[1])


# ----------------------------------------------------------------------------------------------------------- apply
def _model(device, n, seed=0, world=2, dead=None):
    torch.manual_seed(seed)
    m = S.SyntheticGaussianModel(n, 320, 240, seed=seed, device=device, scale_coef=0.02)
    if dead is not None:
        with torch.no_grad():
            m._opacity[dead] = math.log(0.004 / 0.996)
    m.optimizer = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15)
    for _ in range(2):  # populate exp_avg / exp_avg_sq
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.percent_dense = 0.01
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    m.xyz_gradient_accum = torch.rand(n, 1, device=device, generator=g)
    m.denom = torch.ones(n, 1, device=device)
    m.max_radii2D = torch.rand(n, device=device, generator=g)
    m.sum_visible_count_in_one_batch = torch.rand(n, device=device, generator=g)
    m.send_to_gpui_cnt = torch.randint(0, 9, (n, world), dtype=torch.int, device=device, generator=g)
    return m


def _named_tensors(m):
    """the 18 optimizer tensors and send_to_gpui_cnt with their roles, as MCMCStrategy hands them to the kernel"""
    out = []
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        st = m.optimizer.state[p]
        role = {"opacity": dgr.MCMC_ROLE_OPACITY, "scaling": dgr.MCMC_ROLE_SCALING}.get(g["name"], dgr.MCMC_ROLE_COPY)
        out += [(g["name"] + ".exp_avg", st["exp_avg"], dgr.MCMC_ROLE_MOMENT),
                (g["name"] + ".exp_avg_sq", st["exp_avg_sq"], dgr.MCMC_ROLE_MOMENT), (g["name"], p.detach(), role)]
    out.append(("send_to_gpui_cnt", m.send_to_gpui_cnt, dgr.MCMC_ROLE_COPY))
    return out


def _check_apply(device, m, n_add, event):
    P = m._xyz.shape[0]
    named = _named_tensors(m)
    assert len(named) == 19
    # every tensor extended by n_add rows of a marker value, so that a row left unwritten shows
    work = [torch.cat([t, torch.full((n_add,) + tuple(t.shape[1:]), 7, dtype=t.dtype, device=device)]).contiguous()
            for _, t, _ in named]
    old = {name: w.clone() for (name, _, _), w in zip(named, work)}
    opacity_act = m.get_opacity.detach().reshape(-1).contiguous()
    src, count, _ = dgr.mcmc_relocate_plan(opacity_act, n_add, MIN_OP, SEED, event)
    dgr.mcmc_relocate_apply(src, count, opacity_act, MIN_OP, work, [r for _, _, r in named])
    new = {name: w for (name, _, _), w in zip(named, work)}
    src_h, count_h, o_h = src.cpu().numpy(), count.cpu().numpy(), opacity_act.cpu().numpy()
    want_src, want_count, _ = M.relocate_plan(o_h, n_add, MIN_OP, SEED, event)
    assert np.array_equal(src_h, want_src) and np.array_equal(count_h, want_count)
    dest = torch.from_numpy(src_h >= 0).to(device)
    from_rows = torch.from_numpy(src_h[src_h >= 0].astype(np.int64)).to(device)
    source = torch.zeros(P + n_add, dtype=torch.bool, device=device)
    source[:P] = torch.from_numpy(count_h > 0).to(device)
    assert not bool((dest & source).any()) and bool(dest[P:].all())
    untouched = ~(dest | source)
    assert int(untouched.sum()) > 0 or P < 100
    for name, _, role in named:
        a, b = new[name], old[name]
        assert torch.equal(a[untouched], b[untouched]), f"{name}: an untouched row changed"  # bit-equal, all 19
        if role == dgr.MCMC_ROLE_MOMENT:
            assert not bool(a[dest].any()) and not bool(a[source].any()), f"{name}: moments not zeroed"
        elif role == dgr.MCMC_ROLE_COPY:
            assert torch.equal(a[dest], b[from_rows]), f"{name}: a destination is not its source's old row"
            assert torch.equal(a[source], b[source]), f"{name}: a source row changed"
        else:  # a destination carries its source's NEW opacity / scale, bit for bit
            assert torch.equal(a[dest], a[from_rows]), f"{name}: destination != source's new value"
    # the new values against the 60-digit reference, element by element
    rows = np.nonzero(count_h > 0)[0]
    new_op = new["opacity"].double().cpu().numpy().reshape(-1)
    new_sc, old_sc = new["scaling"].double().cpu().numpy(), old["scaling"].double().cpu().numpy()
    worst_o = worst_s = 0.0
    for i in rows:
        n = min(int(count_h[i]) + 1, 51)
        r = M.relocation(o_h[i], n, MIN_OP)
        e64_o = 2.0 ** -53 * (8 / (1 - r["o_new"]) + 4 * (1 + abs(r["logit"])))
        e64_f = 2.0 ** -53 * r["cond_D"] + 2.0 ** -52 * (1 + abs(r["log_f"]))
        bound_o = U * abs(r["logit"]) + e64_o
        ro = abs(new_op[i] - r["logit"]) / bound_o
        ref_s = old_sc[i] + r["log_f"]
        bound_s = U * abs(r["log_f"]) + U * np.abs(ref_s) + e64_f
        rs = float((np.abs(new_sc[i] - ref_s) / bound_s).max())
        assert ro <= 1.0 and rs <= 1.0, (i, n, o_h[i], ro, rs)
        worst_o, worst_s = max(worst_o, ro), max(worst_s, rs)
    print(f"[mcmc apply] P {P} n_add {n_add}: {len(rows)} sources, max n {int(count_h.max()) + 1}; "
          f"worst error / bound: opacity {worst_o:.3f}, scale {worst_s:.3f}")
    return src_h, count_h, new, old


def test_apply_on_a_model_with_moments(device):
    P = 3000
    m = _model(device, P, dead=torch.arange(0, P, 10, device=device))
    src, count, new, old = _check_apply(device, m, 150, event=5)
    n_dead = int((m.get_opacity.detach().reshape(-1) <= MIN_OP).sum())  # the 300 made dead and the scene's own faint rows
    assert n_dead >= 300 and (src >= 0).sum() == n_dead + 150 and count.max() >= 2


def test_apply_sixty_destinations_on_one_source(device):
    """the read-after-write hazard: 60 destinations read one source's OLD scale while it is replaced; n clamps at 51"""
    m = _model(device, 61, seed=3, dead=torch.tensor([i for i in range(61) if i != 37], device=device))
    with torch.no_grad():
        m._opacity[37] = math.log(0.9 / 0.1)
    src, count, new, old = _check_apply(device, m, 3, event=1)
    assert count[37] == 63 and np.all(np.delete(src, 37) == 37)
    r = M.relocation(m.get_opacity[37].item(), 51, MIN_OP)  # n = min(63 + 1, 51)
    got = new["scaling"][0].double().cpu().numpy() - old["scaling"][37].double().cpu().numpy()
    assert np.all(np.abs(got - r["log_f"]) <= 3 * U * (abs(r["log_f"]) + np.abs(old["scaling"][37].double().cpu().numpy())))
    assert torch.equal(new["xyz"][5], old["xyz"][37]) and torch.equal(new["rotation"][63], old["rotation"][37])


# -------------------------------------------------------------------------------------------------------- strategy
def _ptrs(m):
    out = {}
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        out[g["name"]] = p.data_ptr()
        for k in ("exp_avg", "exp_avg_sq"):
            out[g["name"] + "." + k] = m.optimizer.state[p][k].data_ptr()
    out["send_to_gpui_cnt"] = m.send_to_gpui_cnt.data_ptr()
    return out


def _consistent(m, n):
    params = [g["params"][0] for g in m.optimizer.param_groups]
    assert set(m.optimizer.state.keys()) == set(params)  # re-keyed: no stale Parameter owns state
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        assert p is getattr(m, D._ATTR[g["name"]]) and p.shape[0] == n and p.requires_grad
        st = m.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
    assert m.xyz_gradient_accum.shape == (n, 1) and m.denom.shape == (n, 1) and m.max_radii2D.shape == (n,)
    assert m.sum_visible_count_in_one_batch.shape == (n,) and m.send_to_gpui_cnt.shape[0] == n
    for s in ("xyz_gradient_accum", "denom", "max_radii2D", "sum_visible_count_in_one_batch"):
        assert not bool(getattr(m, s).any())


def test_strategy_grows_to_the_cap_in_place(device):
    P = 4000
    m = _model(device, P, seed=1, dead=torch.arange(3, P, 10, device=device))
    st = MCMCStrategy(cap_max=4300, seed=11)
    assert st.relocate_and_grow(m, 100) == 200 and m._xyz.shape[0] == 4200
    _consistent(m, 4200)
    assert torch.isfinite(m._xyz).all() and torch.isfinite(m._scaling).all() and torch.isfinite(m._opacity).all()
    assert float(m.get_opacity.detach().min()) >= MIN_OP * (1 - 1e-5)  # no dead row is left: each took a live row's place
    ptrs1 = _ptrs(m)
    assert st.relocate_and_grow(m, 200) == 100 and m._xyz.shape[0] == 4300
    _consistent(m, 4300)
    assert _ptrs(m) == ptrs1  # the longer views of the same arena rows: nothing moved
    objs = [g["params"][0] for g in m.optimizer.param_groups]
    with torch.no_grad():
        m._opacity[::9] = math.log(0.001 / 0.999)  # some rows die again
    before = {k: v.clone() for k, v in (("xyz", m._xyz.detach()), ("opacity", m._opacity.detach()))}
    assert st.relocate_and_grow(m, 300) == 0 and m._xyz.shape[0] == 4300
    _consistent(m, 4300)
    assert _ptrs(m) == ptrs1
    assert all(a is b for a, b in zip(objs, [g["params"][0] for g in m.optimizer.param_groups]))  # at the cap: no re-key
    dead = torch.zeros(4300, dtype=torch.bool, device=device)
    dead[::9] = True
    assert torch.equal(m._xyz.detach()[~dead][:50], before["xyz"][~dead][:50])
    assert not torch.equal(m._opacity.detach()[dead], before["opacity"][dead])
    assert float(m.get_opacity.detach().min()) >= MIN_OP * (1 - 1e-5)
    assert m._row_arena.capacity == 4300 and m._row_arena.growths == 0
    for p in m.parameters():  # the optimizer still steps on the rows it holds
        p.grad = torch.randn_like(p)
    m.optimizer.step()


def test_growth_free_event_leaves_the_render_alone(device):
    """A growth-free event on a scene whose every tenth row is dead (opacity 0.004; a few more of the scene's own rows lie
    below min_opacity and count as dead too): the render changes by no more than what the dead rows themselves could
    contribute.  Removing a Gaussian of alpha a changes a pixel by at most a times
    the largest colour in play (its own term, and the (1 - a) it took from everything behind it), and alpha <= opacity, so
        |image' - image| <= sum over dead rows of opacity_i * max(colour)
    on every pixel.  The relocation itself (the sources' new opacity and scale, the copies on top of them) preserves the
    composited opacity exactly only at a Gaussian's centre; what it changes elsewhere is part of the measured figure.
    Measured on the MI355X (printed by this test): max |image' - image| 9.9e-02 (mean 4.8e-03) on an image whose largest
    value is 1.51, against a bound of 1.53 from the dead rows' opacities; also in profiles/mcmc_ab.txt."""
    from helpers import settings_from

    W, H, P = 320, 240, 2000
    m = _model(device, P, seed=2, dead=torch.arange(0, P, 10, device=device))
    dead = m.get_opacity.detach().reshape(-1) <= MIN_OP
    assert 200 <= int(dead.sum()) <= 260
    cam = S.orbit_cameras(4, W, H, device=device)[0]
    rast = dgr.GaussianRasterizer(settings_from(cam, torch.zeros(3), sh_degree=3))
    mask = torch.ones((H + 15) // 16, (W + 15) // 16, dtype=torch.bool, device=device)

    def render():
        with torch.no_grad():
            ca = {"stats_collector": {}}
            m2, rgb, co, radii, depths = rast.preprocess_gaussians(m.get_xyz, m.get_scaling, m.get_rotation,
                                                                   m.get_features, m.get_opacity, ca)
            img = rast.render_gaussians(means2D=m2, conic_opacity=co, rgb=rgb, depths=depths, radii=radii,
                                        compute_locally=mask, extended_compute_locally=None, cuda_args=ca)[0]
            return img.double(), rgb.double()

    img0, rgb0 = render()
    bound = float(m.get_opacity.detach().double()[dead].sum() * rgb0.abs().max())
    objs = [g["params"][0] for g in m.optimizer.param_groups]
    assert MCMCStrategy(cap_max=P, seed=5).relocate_and_grow(m, 7) == 0
    assert all(a is b for a, b in zip(objs, [g["params"][0] for g in m.optimizer.param_groups]))
    img1, _ = render()
    diff = float((img1 - img0).abs().max())
    print(f"[mcmc render] max |image' - image| {diff:.4e} (mean {float((img1 - img0).abs().mean()):.3e}), bound from the "
          f"dead rows' opacities {bound:.4e}, image max {float(img0.max()):.3f}")
    assert float(m.get_opacity.detach().min()) >= MIN_OP * (1 - 1e-5)
    assert diff <= bound


# ----------------------------------------------------------------------------------------------------------- noise
def _noise_inputs(P, seed=0):
    rng = np.random.default_rng(100 + P + seed)
    xyz = rng.uniform(-10, 10, (P, 3)).astype(np.float32)
    s = rng.uniform(-20, 3, (P, 3)).astype(np.float32)
    q = rng.standard_normal((P, 4)).astype(np.float32)
    q[0::2] *= np.float32(1e-3)
    q[1::2] *= np.float32(1e3)
    op = rng.permutation(np.linspace(-20, 20, P)).astype(np.float32).reshape(P, 1)
    xi = rng.standard_normal((P, 3)).astype(np.float32)
    return xyz, s, q, op, xi


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000])
def test_noise_against_fp64(device, P):
    xyz, s, q, op, xi = _noise_inputs(P)
    scaler = 0.01
    dev = [torch.from_numpy(a).to(device) for a in (xyz, s, q, op, xi)]
    got = dgr.mcmc_noise(dev[0], dev[1], dev[2], dev[3], scaler, xi=dev[4]).double().cpu().numpy()
    want, bound, disp = M.noise(xyz, s, q, op, scaler, xi)
    ratio = np.abs(got - want) / bound
    print(f"[mcmc noise] P {P}: worst error / bound {ratio.max():.3f}; largest displacement {np.abs(disp).max():.3e}")
    assert np.all(np.isfinite(got)) and ratio.max() <= 1.0, np.unravel_index(ratio.argmax(), ratio.shape)
    if P >= 63:
        assert np.abs(disp).max() > 1e-3  # the faint rows do move


@pytest.mark.parametrize("P", [1, 65, 1000])
def test_fused_draw_is_the_supplied_draw(device, P):
    xyz, s, q, op, _ = _noise_inputs(P, seed=1)
    a = [torch.from_numpy(t).to(device) for t in (xyz, s, q, op)]
    b = [t.clone() for t in a]
    xi = dgr.mcmc_normals(P, SEED, 42, device=device)
    dgr.mcmc_noise(a[0], a[1], a[2], a[3], 0.02, xi=None, seed=SEED, step=42)
    dgr.mcmc_noise(b[0], b[1], b[2], b[3], 0.02, xi=xi)
    assert torch.equal(a[0], b[0])
    for t, u in zip(a[1:], b[1:]):
        assert torch.equal(t, u)  # inputs untouched
    if P > 1:
        assert not torch.equal(a[0], torch.from_numpy(xyz).to(device))


def test_solid_gaussians_stay_where_they_are(device):
    """Rows with opacity >= 0.1 move by less than one ulp of their position.  The gate makes it so: x = 1 - o <= 0.9 gives
    g <= 1 / (1 + e^9.5) = 7.5e-5.  With the end-of-schedule scaler 5e5 * 1.6e-6 = 0.8, scales up to 0.01 (S = sum of
    squared scales <= 3e-4) and |xi|_2 <= 5.89 sqrt(3), the displacement is at most 0.8 * 7.5e-5 * 3e-4 * 10.2 = 1.8e-7,
    below HALF an ulp of a coordinate of magnitude >= 4 (2.4e-7): the add rounds back to the old position.  The
    precondition is asserted in fp64 per row; the positions are then required to keep their bits."""
    P, scaler = 2000, 0.8
    rng = np.random.default_rng(9)
    xyz = (rng.uniform(4, 8, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3))).astype(np.float32)
    s = rng.uniform(-9, math.log(0.01), (P, 3)).astype(np.float32)
    q = rng.standard_normal((P, 4)).astype(np.float32)
    o = np.linspace(0.1, 0.999, P)
    op = np.log(o / (1 - o)).astype(np.float32).reshape(P, 1)
    op[0] = np.nextafter(np.float32(math.log(0.1 / 0.9)), np.float32(1))  # sigmoid >= 0.1 after the fp32 rounding
    dev = [torch.from_numpy(a).to(device) for a in (xyz, s, q, op)]
    xi = dgr.mcmc_normals(P, SEED, 7, device=device)
    _, _, disp = M.noise(xyz, s, q, op, scaler, xi.cpu().numpy())
    half_ulp = np.spacing(np.abs(xyz)).astype(np.float64) / 2
    assert np.all(np.abs(disp) < 0.9 * half_ulp)  # the precondition, with room for the kernel's own roundings
    dgr.mcmc_noise(dev[0], dev[1], dev[2], dev[3], scaler, xi=None, seed=SEED, step=7)
    assert torch.equal(dev[0], torch.from_numpy(xyz).to(device))


def test_normals(device):
    n = 65536
    z = dgr.mcmc_normals(n, SEED, 1, device=device)
    assert z.shape == (n, 3) and z.dtype == torch.float32
    zz = z.double().cpu().numpy().reshape(-1)
    N = zz.size
    assert N == 196608 and np.all(np.isfinite(zz)) and np.abs(zz).max() <= 6.0  # 24-bit Box-Muller: at most 5.89
    mean, var = zz.mean(), zz.var()
    print(f"[mcmc normals] mean {mean:.3e} var-1 {var - 1:.3e} max |z| {np.abs(zz).max():.3f}")
    assert abs(mean) <= 9 / math.sqrt(n) and abs(var - 1) <= 9 * math.sqrt(2 / n)
    for c in range(3):  # each component on its own, and no pair correlated
        col = z[:, c].double().cpu().numpy()
        assert abs(col.mean()) <= 9 / math.sqrt(n) and abs(col.var() - 1) <= 9 * math.sqrt(2 / n)
    zc = z.double().cpu().numpy()
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs((zc[:, a] * zc[:, b]).mean()) <= 9 / math.sqrt(n)
    assert torch.equal(z, dgr.mcmc_normals(n, SEED, 1, device=device))  # deterministic
    assert torch.equal(z[:1000], dgr.mcmc_normals(1000, SEED, 1, device=device))  # a row's draw does not depend on the grid
    other_step, other_seed = dgr.mcmc_normals(n, SEED, 2, device=device), dgr.mcmc_normals(n, SEED ^ 1, 1, device=device)
    assert float((z == other_step).float().mean()) < 1e-3 and float((z == other_seed).float().mean()) < 1e-3


def test_strategy_noise_is_keyed_by_seed_rank_and_iteration(device):
    m = _model(device, 500, seed=4)
    with torch.no_grad():
        m._opacity.fill_(-8.0)  # faint: everything moves
    st = MCMCStrategy(cap_max=500, seed=3, rank=1)
    xyz0 = m._xyz.detach().clone()
    st.inject_noise(m, 17, 1.6e-4)
    want = xyz0.clone()
    dgr.mcmc_noise(want, m._scaling.detach(), m._rotation.detach(), m._opacity.detach(), 5e5 * 1.6e-4,
                   xi=dgr.mcmc_normals(500, st.device_seed(), 17, device=device))
    assert torch.equal(m._xyz.detach(), want) and not torch.equal(want, xyz0)
    assert st.device_seed() != MCMCStrategy(cap_max=500, seed=3, rank=0).device_seed()


# ----------------------------------------------------------------------------------------------------- regulariser
@pytest.mark.parametrize("P", [1, 1000])
def test_regulariser_gradients_match_autograd(device, P):
    rng = np.random.default_rng(P)
    op = rng.uniform(-6, 6, (P, 1)).astype(np.float32)
    s = rng.uniform(-9, 2, (P, 3)).astype(np.float32)
    g_op, g_s = rng.standard_normal((P, 1)).astype(np.float32) * 1e-4, rng.standard_normal((P, 3)).astype(np.float32) * 1e-4
    lam_o, lam_s = 0.01, 0.01
    m = types.SimpleNamespace(_xyz=torch.zeros(P, 3, device=device), optimizer=types.SimpleNamespace(fuse_backward=False),
                              _opacity=torch.nn.Parameter(torch.from_numpy(op).to(device)),
                              _scaling=torch.nn.Parameter(torch.from_numpy(s).to(device)))
    m._opacity.grad, m._scaling.grad = torch.from_numpy(g_op).to(device), torch.from_numpy(g_s).to(device)
    MCMCStrategy(cap_max=P, opacity_reg=lam_o, scale_reg=lam_s).add_regulariser_grads(m)
    t_op = torch.from_numpy(op).double().requires_grad_(True)
    t_s = torch.from_numpy(s).double().requires_grad_(True)
    (lam_o * torch.sigmoid(t_op).mean() + lam_s * torch.exp(t_s).mean()).backward()
    add_o, add_s = t_op.grad.numpy(), t_s.grad.numpy()
    ref_o, ref_s = M.reg_grads(op, s, lam_o / P, lam_s / (3 * P))
    assert np.allclose(add_o, ref_o, rtol=1e-12, atol=0) and np.allclose(add_s, ref_s, rtol=1e-12, atol=0)
    want_o, want_s = g_op.astype(np.float64) + add_o, g_s.astype(np.float64) + add_s
    c_o = float(np.float32(lam_o / P))
    # opacity: the sigmoid carries 4 u (exp 2 u, add, divide), ABSOLUTE since o <= 1, and so does o (1 - o) to first order;
    # its two roundings, the constant's own and the product's: 4 u relative.  scale: exp 2 u, constant u, product u, slack u
    bound_o = U * np.abs(want_o) + 4 * U * abs(c_o) + 4 * U * np.abs(add_o)
    bound_s = U * np.abs(want_s) + 5 * U * np.abs(add_s)
    got_o, got_s = m._opacity.grad.double().cpu().numpy(), m._scaling.grad.double().cpu().numpy()
    ro, rs = (np.abs(got_o - want_o) / bound_o).max(), (np.abs(got_s - want_s) / bound_s).max()
    print(f"[mcmc reg] P {P}: worst error / bound: opacity {ro:.3f}, scale {rs:.3f}")
    assert ro <= 1.0 and rs <= 1.0
    assert not np.array_equal(got_s, g_s.astype(np.float64)) and not np.array_equal(got_o, g_op.astype(np.float64))
