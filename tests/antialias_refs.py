"""Inputs and references of the anti-aliasing tests (include/gsraster.h: gsr_set_antialiasing), built on
tests/projection_refs.py: the same oracle (oracle/torch_oracle.preprocess with autograd, float64 the arbiter, float32 the
yardstick of helpers.assert_rows_close) with conic_opacity.w of every visible row multiplied by rho.  There is no
reference call site for the switch; what is restated here is the header's definition:

    a0, b, c0 = T Sigma T^T before the dilation;  det0 = a0 c0 - b^2;  a = a0 + 0.3, c = c0 + 0.3, det = a c - b^2;
    q = det0 / det;  rho = sqrt(max(0.000025, q));
    d rho / d(a0, b, c0) = 1 / (2 rho) * dq/d(a, b, c) where q > 0.000025, zero where the clamp holds, with
    dq/da = (0.3 (c0^2 + b^2) + 0.09 c0) / det^2, dq/dc = (0.3 (a0^2 + b^2) + 0.09 a0) / det^2,
    dq/db = -2 b (0.3 (a0 + c0) + 0.09) / det^2.

Plain module: importable without a GPU; nothing here comes from the code under test."""
import functools
import math

import torch

import projection_refs as R
from helpers import KEYS
from oracle import torch_oracle as O

QMIN = 0.000025
M_QCLAMP = 1e-3  # |q / QMIN - 1| of every (row, camera) in front of the near plane, in float64
FAMILIES = ("plain", "aaclamp", "jclamp", "near", "aniso_mild", "tiny", "huge", "clamped", "behind", "raw")


class Rho(torch.autograd.Function):
    """rho(a0, b, c0) with the closed-form backward of the definition (b: the one scalar in both off-diagonal places)"""

    @staticmethod
    def forward(ctx, a0, b, c0):
        det0 = a0 * c0 - b * b
        det = (a0 + 0.3) * (c0 + 0.3) - b * b
        q = det0 / det
        rho = torch.sqrt(torch.clamp(q, min=QMIN))
        ctx.save_for_backward(a0, b, c0, det, q, rho)
        return rho

    @staticmethod
    def backward(ctx, g):
        a0, b, c0, det, q, rho = ctx.saved_tensors
        w = torch.where(q > QMIN, g / (2.0 * rho), torch.zeros_like(g))
        h = 0.3 * (a0 + c0) + 0.09
        d2 = det * det
        return (w * ((0.3 * (c0 * c0 + b * b) + 0.09 * c0) / d2), w * (-2.0 * b * h / d2),
                w * ((0.3 * (a0 * a0 + b * b) + 0.09 * a0) / d2))


def rho_plain(a0, b, c0):
    """the same value for plain autograd (the quotient rule): what Rho's backward is checked against in float64"""
    return torch.sqrt(torch.clamp((a0 * c0 - b * b) / ((a0 + 0.3) * (c0 + 0.3) - b * b), min=QMIN))


def cov2d_abc(means3D, scales, rotations, cam, W, H, scale_modifier=1.0):
    """(a0, b, c0) of rows in front of the near plane for one camera, from the given leaves, with projection_refs._cov2d"""
    dt = means3D.dtype
    view = cam.world_view_transform.to(dt)
    tx, ty = R.tanfov(cam)
    t = torch.cat([means3D, torch.ones(means3D.shape[0], 1, dtype=dt)], dim=1) @ view[:, :3]
    c6 = O.cov3d_from_scale_rot(scales, rotations, scale_modifier)
    cov2 = R._cov2d(t[:, 0], t[:, 1], t[:, 2], c6, view, W, H, tx, ty)
    return cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]


def q64(act, cam, W, H, scale_modifier=1.0):
    """float64 (q [N], front [N]) of one camera; q of rows behind the near plane is 1 (never looked at)"""
    a = {k: v.double() for k, v in act.items()}
    view = cam.world_view_transform.double()
    tz = (torch.cat([a["means3D"], torch.ones(a["means3D"].shape[0], 1, dtype=torch.float64)], dim=1) @ view[:, :3])[:, 2]
    front = tz > R.NEAR
    q = torch.ones_like(tz)
    ix = front.nonzero().squeeze(1)
    a0, b, c0 = cov2d_abc(a["means3D"][ix], a["scales"][ix], a["rotations"][ix], cam, W, H, scale_modifier)
    q[ix] = (a0 * c0 - b * b) / ((a0 + 0.3) * (c0 + 0.3) - b * b)
    return q, front


def qclamp_violations(act, cams, W, H, scale_modifier=1.0):
    """bool [N]: rows whose q comes closer than M_QCLAMP (relative) to the clamp's threshold for SOME camera"""
    bad = torch.zeros(act["means3D"].shape[0], dtype=torch.bool)
    for cam in cams:
        q, front = q64(act, cam, W, H, scale_modifier)
        bad |= front & ((q / QMIN - 1.0).abs() < M_QCLAMP)
    return bad


# ------------------------------------------------------------------------------------------------ the new family
def _draw_aaclamp(gen, n, W, H):
    """projection_refs' base rows with scales of 0.04 px at the row's depth (fx = 0.9 W), times m log-uniform in
    10^+-0.5 per row and u uniform in 0.8 .. 1.2 per axis: q = det0 / det lies on both sides of 0.000025"""
    g = R._base(gen, n, W, H)
    z = g["means3D"][:, 2]
    m = 10.0 ** (torch.rand(n, generator=gen) - 0.5)
    u = 0.8 + 0.4 * torch.rand(n, 3, generator=gen)
    g["scales"] = (0.04 * z / (0.9 * W) * m)[:, None] * u
    return g


@functools.lru_cache(maxsize=None)
def _family(name, N, W, H, deg, seed, B, scale_modifier, sh_coeffs):
    """rows that keep every margin of projection_refs AND the clamp's, re-drawn where they do not (none is masked)"""
    cams = R.cameras(B, W, H)
    if name == "aaclamp":
        gen = torch.Generator().manual_seed(seed)

        def draw(n):
            return {k: v.float().contiguous() for k, v in _draw_aaclamp(gen, n, W, H).items()}

        rows = draw(N)
        act = lambda r: r  # noqa: E731
    else:
        rows, _ = R.family(name, N, W, H, deg, seed, B, scale_modifier, sh_coeffs)
        rows = {k: v.clone() for k, v in rows.items()}  # (projection_refs shares its tensors: never modified)
        gen = torch.Generator().manual_seed(seed + 1000003)
        idx_all = torch.arange(N)

        def draw_idx(ix):
            g = R._draw(name, gen, ix, W, H)
            if name == "raw":
                g = R._raw_from_plain(gen, g, W, H)
            return {k: v.float().contiguous() for k, v in g.items()}

        act = lambda r: R.activate(r) if name == "raw" else r  # noqa: E731

    def violations(r):
        a = {k: v for k, v in act(r).items()}
        return R.margin_violations(a, cams, W, H, deg, scale_modifier) | qclamp_violations(a, cams, W, H, scale_modifier)

    for _ in range(R.REDRAW_ROUNDS):
        bad = violations(rows)
        if not bool(bad.any()):
            break
        new = draw(int(bad.sum())) if name == "aaclamp" else draw_idx(idx_all[bad])
        for k in rows:
            rows[k][bad] = new[k]
    assert not bool(violations(rows).any()), f"family {name}: rows inside a margin after {R.REDRAW_ROUNDS} rounds"
    return rows, cams


def family(name, N, W, H, deg, seed, B=1, scale_modifier=1.0, sh_coeffs=16):
    """projection_refs.family with the clamp's margin on top, and the `aaclamp` family.  Shared tensors: do not modify."""
    assert name in FAMILIES and (W, H) in R.FRAMES and sh_coeffs == 16
    return _family(name, N, W, H, deg, seed, B, float(scale_modifier), sh_coeffs)


def upstream_aa(B, N, seed=5):
    """projection_refs.upstream with ONE sign per row, across the cameras, in column 3 of dL_dconic_opacity:
    |g| sign(g of camera 0).  dL/dopacity = sum_b g_b rho_b; with independent signs that sum cancels, and a row's float32
    reference is then far off relative to the row's (small) result -- a property of the inputs, not of any kernel."""
    G2, Gco, Grgb = R.upstream(B, N, seed)
    Gco = Gco.clone()
    Gco[:, :, 3] = Gco[:, :, 3].abs() * torch.sign(Gco[0, :, 3])[None, :]
    return G2, Gco, Grgb


# ------------------------------------------------------------------------------------------------ the reference
def reference_aa(inputs, cams, deg, upstream, dtype, raw, scale_modifier=1.0, rho_fn=Rho.apply):
    """projection_refs.reference with conic_opacity[:, 3] multiplied by rho on the visible rows.  rho comes from `rho_fn`
    over (a0, b, c0) of projection_refs._cov2d on the same leaves; the conic's incoming gradient still goes through
    k11_conic_gradient.  Also returns q_clamped bool [B,N]: visible rows on which the clamp of q holds."""
    W, H = cams[0].image_width, cams[0].image_height
    G2, Gco, Grgb = (t.to(dtype) for t in upstream)
    if raw:
        leaves = [inputs[k].to(dtype).clone().requires_grad_() for k in R.RAW_KEYS]
        a = R.activate(dict(zip(R.RAW_KEYS, leaves)), dtype)
        ins = [a[k] for k in KEYS]
    else:
        leaves = [inputs[k].to(dtype).clone().requires_grad_() for k in KEYS]
        ins = leaves
    N = ins[0].shape[0]
    names = R.OUTPUTS + ("radii", "clamped", "q_clamped")
    out = {k: [] for k in names}
    total = None
    for b, cam in enumerate(cams):
        tx, ty = R.tanfov(cam)
        m2, rgb, co, radii, depths, cov3D, clamped = O.preprocess(
            *ins, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center,
            W=W, H=H, tanfovx=tx, tanfovy=ty, sh_degree=deg, scale_modifier=scale_modifier, return_aux=True)
        ix = (radii > 0).nonzero().squeeze(1)
        a0, bb, c0 = cov2d_abc(ins[0][ix], ins[1][ix], ins[2][ix], cam, W, H, scale_modifier)
        rho = rho_fn(a0, bb, c0)
        factor = torch.ones(N, dtype=dtype).index_copy(0, ix, rho)
        co_aa = torch.cat([co[:, :3], co[:, 3:] * factor[:, None]], dim=1)
        qc = torch.zeros(N, dtype=torch.bool)
        qc[ix] = ((a0 * c0 - bb * bb) / ((a0 + 0.3) * (c0 + 0.3) - bb * bb)).detach() <= QMIN
        grads = torch.autograd.grad([m2, co_aa, rgb], leaves, [G2[b], R.k11_conic_gradient(co.detach(), Gco[b]), Grgb[b]],
                                    allow_unused=True, retain_graph=True)
        grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
        total = grads if total is None else [t + g for t, g in zip(total, grads)]
        for k, v in zip(names, (m2, depths, co_aa, rgb, cov3D, radii, clamped, qc)):
            out[k].append(v.detach())
    res = {k: torch.stack(v) for k, v in out.items()}
    res.update(zip(R.GRADS_RAW if raw else R.GRADS_ACT, total))
    return res


# ------------------------------------------------------------------------------------------------ the cases
class Case(R.Case):
    """projection_refs.Case over this module's families, incoming gradients and references"""

    def __init__(self, form, fam, deg, N, frame=0, B=1, stride=0, sm=1.0):
        assert fam in FAMILIES
        R.Case.__init__(self, form, fam, deg, N, frame=frame, B=B, stride=stride, sm=sm)
        self.id = "aa-" + self.id

    def inputs(self):
        return _inputs(self.is_raw, self.fam, self.N, self.W, self.H, self.deg, self.seed, self.B, self.sm)

    def upstream(self):
        return upstream_aa(self.B, self.N)

    def references(self):
        """-> (float64 reference, float32 reference), computed once and shared: do not modify"""
        return _references(self.is_raw, self.fam, self.N, self.W, self.H, self.deg, self.seed, self.B, self.sm)


@functools.lru_cache(maxsize=None)
def _inputs(raw, fam, N, W, H, deg, seed, B, sm):
    ins, cams = family(fam, N, W, H, deg, seed, B, sm)
    if raw and fam != "raw":
        ins = R.to_raw(ins)
    return ins, cams


@functools.lru_cache(maxsize=None)
def _references(raw, fam, N, W, H, deg, seed, B, sm):
    ins, cams = _inputs(raw, fam, N, W, H, deg, seed, B, sm)
    up = upstream_aa(B, N)
    return (reference_aa(ins, cams, deg, up, torch.float64, raw, sm), reference_aa(ins, cams, deg, up, torch.float32, raw, sm))


def _cases():
    """Per root form: `plain` and `aaclamp` at every N of {1, 127, 128, 129, 257, 1031} (K1's workgroup is 256 rows,
    K11's 128), the two gradient strides alternating, the degrees spread and B in {1, 3, 5} for the batched form as in
    projection_refs._cases; then once each at degree 3 and N = 257 the families at the projection's other edges (`raw`
    where the form takes raw parameters); scale_modifier 0.7 once.  The hard `aniso` family is left out: det0 itself
    cancels there and the float32 reference is far over helpers.ROW_UNIT_CAP."""
    cs = []
    n_deg_b = ((1031, 3, 3), (257, 3, 5), (129, 2, 1), (128, 1, 3), (127, 0, 5), (1, 3, 5))
    for form in ("act", "raw", "rawb"):
        for j, (N, deg, B) in enumerate(n_deg_b):
            B = B if form == "rawb" else 1
            cs.append(Case(form, "plain", deg, N, frame=j % 2, B=B, stride=9 * (j % 2)))
            cs.append(Case(form, "aaclamp", deg, N, frame=(j + 1) % 2, B=B, stride=9 * ((j + 1) % 2)))
        others = ("jclamp", "near", "aniso_mild", "tiny", "huge", "clamped", "behind") + (("raw",) if form != "act" else ())
        for j, fam in enumerate(others):
            cs.append(Case(form, fam, 3, 257, frame=0, B=(1, 3)[j % 2] if form == "rawb" else 1, stride=9 * (j % 2)))
    cs.append(Case("rawb", "plain", 3, 257, frame=0, B=3, stride=9, sm=0.7))
    return cs


CASES = _cases()
