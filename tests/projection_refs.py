"""Inputs and float64 references of the per-row projection tests (K1 / K11): seeded scene families that sit at the edges
of the projection -- the Jacobian clamp, the near plane, extreme scales, clamped colours, culled rows -- with every
discrete decision (cull, radius, tile rect, colour clamp, Jacobian clamp) kept at a distance from its threshold by
construction, so that a float32 kernel and the float64 oracle decide alike and every row can be compared.

Plain module: importable without a GPU.  The reference is oracle/torch_oracle.preprocess with autograd, run in float64
(the arbiter) and in float32 (the yardstick of helpers.assert_rows_close); nothing here comes from the code under test."""
import functools
import math

import torch

import synthetic_scene as S
from helpers import KEYS
from oracle import torch_oracle as O

RAW_KEYS = ("xyz", "scaling", "rotation", "features_dc", "features_rest", "opacity")
FAMILIES = ("plain", "jclamp", "near", "aniso", "aniso_mild", "tiny", "huge", "clamped", "behind", "raw")
# scales of the two anisotropic families.  `aniso` (1e-3 : 0.3 : 1e-2) is for the activated entry points.  With respect to
# LOG-scales a row's gradient is 2 s_r^2 (u_r^T G u_r), u_r the axis projected to the screen and G = dL/dcov2D, so the
# long axis is the row's largest entry -- and it is the one that K11's formula (the CUDA backward's, shared by the C
# restatement) conditions worst: it forms G = -conic Gin conic entry by entry, and along the splat's long direction conic
# has its SMALL eigenvalue, so the entry is a difference of terms (lambda_max / lambda_min)^2 times its size.  Measured at
# 1e-2 : 0.3 : 3e-2, row 155 of the N = 257 case: kernel and C restatement both 1.8e-3 off (bit-equal), the float32
# autograd oracle 5.7e-5.  The raw entry points therefore get `aniso_mild`, 0.1 : 0.3 : 0.15: eigenvalue ratio <= 9,
# amplification <= 81 x 2^-24, below K times the unit measured there (38 .. 81).  EXPERIMENTS.md has the finding.
ANISO = {"aniso": (1e-3, 0.3, 1e-2), "aniso_mild": (0.1, 0.3, 0.15)}
FRAMES = ((80, 64), (333, 211))
NEAR = 0.2
OUTPUTS = ("means2D", "depths", "conic_opacity", "rgb", "cov3D")
GRADS_ACT = ("d_means3D", "d_scales", "d_rotations", "d_shs", "d_opacities")
GRADS_RAW = ("d_xyz", "d_scaling", "d_rotation", "d_features_dc", "d_features_rest", "d_opacity")

# the margins (module docstring): distances that the float64 geometry of every (row, camera) keeps from a threshold
M_NEAR = 1e-4     # |t.z - 0.2|
M_RADIUS = 1e-3   # 3 sqrt(lambda) from an integer
M_COLOUR = 1e-3   # a raw colour channel from 0
M_BRIGHT = 0.2    # the brightest raw colour channel of a row that is not clamped in all three (see margin_violations)
M_JCLAMP = 1e-3   # |t.x / t.z| and |t.y / t.z| from 1.3 tanfov, relative
M_TILE = 1e-3     # (px +- r) / 16, (py +- r) / 16 and the rounded-up upper edges from an integer
REDRAW_ROUNDS = 20


def tanfov(cam):
    """(tanfovx, tanfovy) as the float32 values that the kernels receive"""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    return f32(math.tan(cam.FoVx / 2)), f32(math.tan(cam.FoVy / 2))


def cameras(B, W, H):
    """the first B of eight orbit cameras; camera 0 is the identity, so the families are laid out in its view space"""
    return S.orbit_cameras(8, W, H)[:B]


def pack_cameras(cams):
    """[B,40] float32 records { viewmatrix, projmatrix, campos, tanfovx, tanfovy, 0, 0, 0 } of the batched entry points"""
    recs = []
    for c in cams:
        recs.append(torch.cat([c.world_view_transform.reshape(16).float(), c.full_proj_transform.reshape(16).float(),
                               c.camera_center.reshape(3).float(), torch.tensor(tanfov(c) + (0.0, 0.0, 0.0))]))
    return torch.stack(recs).contiguous()


def activate(raw, dtype=torch.float64):
    """the getters of the raw parameters (exp, normalize, cat, sigmoid) in `dtype` -> the five activated tensors"""
    r = {k: v.to(dtype) for k, v in raw.items()}
    return dict(means3D=r["xyz"], scales=torch.exp(r["scaling"]), rotations=torch.nn.functional.normalize(r["rotation"]),
                shs=torch.cat((r["features_dc"], r["features_rest"]), dim=1), opacities=torch.sigmoid(r["opacity"]))


def to_raw(act):
    """raw parameters whose getters give (to rounding) the activated tensors of a family: log, logit, split"""
    op = act["opacities"].double().clamp(1e-6, 1 - 1e-6)
    return dict(xyz=act["means3D"].clone(), scaling=torch.log(act["scales"].double()).float(),
                rotation=act["rotations"].clone(), features_dc=act["shs"][:, :1].contiguous(),
                features_rest=act["shs"][:, 1:].contiguous(), opacity=torch.log(op / (1 - op)).float().reshape(-1, 1))


# ------------------------------------------------------------------------------------------------ geometry, float64
def _cov2d(t0, t1, tz, c6, view, W, H, tanx, tany, straight_through=False):
    """J Wc Sigma Wc^T J^T [N,2,2] with the Jacobian's clamp of t.x / t.z and t.y / t.z to +-1.3 tanfov.  A clamped
    component is a constant for autograd, as K11 treats it; straight_through=True keeps the clamped VALUE but lets the
    gradient pass as if it were not clamped -- what K11 would compute without its zero multiplier (the CPU file's
    corruption of a Jacobian-clamp row)."""
    N = tz.shape[0]
    limx, limy = 1.3 * tanx, 1.3 * tany
    txc = (torch.clamp(t0 / tz, -limx, limx) * tz).detach()
    tyc = (torch.clamp(t1 / tz, -limy, limy) * tz).detach()
    out_x, out_y = (t0 / tz).abs() > limx, (t1 / tz).abs() > limy
    if straight_through:
        txc, tyc = txc + (t0 - t0.detach()), tyc + (t1 - t1.detach())
    tx, ty = torch.where(out_x, txc, t0), torch.where(out_y, tyc, t1)
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], dim=1).view(N, 2, 3)
    Sig = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]],
                      dim=1).view(N, 3, 3)
    M = J @ view[:3, :3].t()
    return M @ Sig @ M.transpose(1, 2)


def conic_grad_means(act, cam, W, H, g_conic, scale_modifier=1.0, straight_through=False):
    """float64 dL/dmeans3D [N,3] through the conic alone for incoming conic gradients g_conic [N,3] (rows in front of the
    near plane only make sense), with or without the Jacobian clamp's zero multiplier (see _cov2d)"""
    dt = torch.float64
    a = {k: v.to(dt) for k, v in act.items()}
    p = a["means3D"].clone().requires_grad_()
    view = cam.world_view_transform.to(dt)
    tx_, ty_ = tanfov(cam)
    t = torch.cat([p, torch.ones(p.shape[0], 1, dtype=dt)], dim=1) @ view[:, :3]
    c6 = O.cov3d_from_scale_rot(a["scales"], a["rotations"], scale_modifier)
    cov2 = _cov2d(t[:, 0], t[:, 1], t[:, 2], c6, view, W, H, tx_, ty_, straight_through)
    ca, cb, cc = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = ca * cc - cb * cb
    conic = torch.stack([cc / det, -cb / det, ca / det], dim=1)
    return torch.autograd.grad(conic, p, g_conic.to(dt))[0]


def geometry(act, cam, W, H, deg, scale_modifier=1.0):
    """float64 quantities of every row for one camera that the discrete decisions of K1 depend on (restated here from
    oracle/torch_oracle._preprocess_core, which does not return them): t, t.x/t.z and t.y/t.z over their limits,
    3 sqrt(lambda), the pixel centre and the raw colour.  Rows behind the near plane carry NaN-free junk; `front` tells."""
    dt = torch.float64
    a = {k: v.to(dt) for k, v in act.items()}
    N = a["means3D"].shape[0]
    view, proj, campos = (t.to(dt) for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center))
    tx_, ty_ = tanfov(cam)
    ph = torch.cat([a["means3D"], torch.ones(N, 1, dtype=dt)], dim=1)
    t = ph @ view[:, :3]
    front = t[:, 2] > NEAR
    tz = torch.where(front, t[:, 2], torch.ones_like(t[:, 2]))  # (junk but finite behind the plane)
    p_hom = ph @ proj
    p_w = 1.0 / (p_hom[:, 3] + 0.0000001)
    px = ((p_hom[:, 0] * p_w + 1.0) * W - 1.0) * 0.5
    py = ((p_hom[:, 1] * p_w + 1.0) * H - 1.0) * 0.5
    limx, limy = 1.3 * tx_, 1.3 * ty_
    rx, ry = (t[:, 0] / tz).abs() / limx, (t[:, 1] / tz).abs() / limy
    c6 = O.cov3d_from_scale_rot(a["scales"], a["rotations"], scale_modifier)
    cov2 = _cov2d(t[:, 0], t[:, 1], tz, c6, view, W, H, tx_, ty_)
    ca, cb, cc = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    mid = 0.5 * (ca + cc)
    lam = mid + torch.sqrt(torch.clamp(mid * mid - (ca * cc - cb * cb), min=0.1))
    r3 = 3.0 * torch.sqrt(lam)
    d = a["means3D"] - campos[None, :]
    colour = O.sh_to_rgb_raw(deg, a["shs"], d / d.norm(dim=1, keepdim=True)) + 0.5
    return dict(t=t, front=front, rx=rx, ry=ry, r3=r3, px=px, py=py, colour=colour)


def _frac_dist(x):
    """distance of x from the nearest integer"""
    return (x - torch.round(x)).abs()


def margin_violations(act, cams, W, H, deg, scale_modifier=1.0):
    """bool [N]: rows that come closer than a margin to one of K1's thresholds for SOME camera"""
    bad = torch.zeros(act["means3D"].shape[0], dtype=torch.bool)
    for cam in cams:
        g = geometry(act, cam, W, H, deg, scale_modifier)
        bad |= (g["t"][:, 2] - NEAR).abs() < M_NEAR
        b = _frac_dist(g["r3"]) < M_RADIUS
        b |= (g["colour"].abs() < M_COLOUR).any(dim=1)
        # not a threshold but conditioning: colour = 0.5 + a sum of O(1) terms, so float32 carries an absolute error of a
        # few ulps of 1 (~2e-7) whatever the result; a row whose brightest channel is 0.004 is then off by 1e-5 of
        # itself in ANY float32 evaluation (seen: the C restatement at 17 units on such a row, where the float32 oracle
        # happened to be exact).  From 0.2 up, four ulps of 1 are 20 x 2^-24 of the row: inside K times the floor unit.
        top = g["colour"].amax(dim=1)
        b |= (top > 0) & (top < M_BRIGHT)
        b |= ((g["rx"] - 1.0).abs() < M_JCLAMP) | ((g["ry"] - 1.0).abs() < M_JCLAMP)
        r = torch.ceil(g["r3"])
        for c in (g["px"], g["py"]):
            for edge in (c - r, c + r, c + r + 15.0):  # the rect's lower and upper edge, and the upper one as rounded up
                b |= _frac_dist(edge / 16.0) < M_TILE
        bad |= b & g["front"]
    return bad


# ------------------------------------------------------------------------------------------------ families
def _base(gen, n, W, H, scale_coef=0.01, rest_sigma=0.1):
    """rows of synthetic_scene.make_gaussians' distributions, from the caller's generator"""
    u = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    tanx, tany = W / (1.8 * W), H / (1.8 * W)
    z = u(n) * 8.0 + 2.0
    x = (u(n) * 2.3 - 1.15) * z * tanx
    y = (u(n) * 2.3 - 1.15) * z * tany
    q = torch.randn(n, 4, generator=gen)
    return dict(means3D=torch.stack([x, y, z], dim=1),
                scales=torch.exp(torch.log(scale_coef * z)[:, None] + 0.5 * torch.randn(n, 3, generator=gen)),
                rotations=q / q.norm(dim=1, keepdim=True),
                shs=torch.cat([(u(n, 1, 3) * 2.0 - 1.0) / O.SH_C0, rest_sigma * torch.randn(n, 15, 3, generator=gen)], dim=1),
                opacities=torch.sigmoid(2.0 * torch.randn(n, 1, generator=gen)))


def _draw(name, gen, idx, W, H):
    """the rows `idx` (their index decides their kind) of family `name` -> the five activated tensors"""
    n = idx.numel()
    u = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    sign = lambda *s: torch.where(u(*s) < 0.5, -1.0, 1.0)  # noqa: E731
    tanx, tany = W / (1.8 * W), H / (1.8 * W)
    if name in ("plain", "raw"):
        return _base(gen, n, W, H)
    if name == "jclamp":
        # kinds by index: x beyond +, x beyond -, y beyond +, y beyond -, both beyond, an ordinary row
        g = _base(gen, n, W, H, scale_coef=0.02)
        kind = idx % 6
        z = g["means3D"][:, 2]
        beyond = 1.3 * (1.31 + 0.59 * u(n, 2))  # 1.31 .. 1.9 times the limit, in units of tanfov
        sx = torch.where(kind == 0, 1.0, torch.where(kind == 1, -1.0, sign(n)))
        sy = torch.where(kind == 2, 1.0, torch.where(kind == 3, -1.0, sign(n)))
        x_out, y_out = (kind <= 1) | (kind == 4), ((kind >= 2) & (kind <= 4))
        g["means3D"][:, 0] = torch.where(x_out, sx * beyond[:, 0] * tanx * z, g["means3D"][:, 0])
        g["means3D"][:, 1] = torch.where(y_out, sy * beyond[:, 1] * tany * z, g["means3D"][:, 1])
        g["scales"] = torch.where((kind < 5)[:, None], 8.0 * g["scales"], g["scales"])
        return g
    if name == "near":
        g = _base(gen, n, W, H)
        z = torch.where(idx % 5 == 4, g["means3D"][:, 2], 0.2002 + 0.2998 * u(n))
        g["scales"] = g["scales"] * (z / g["means3D"][:, 2])[:, None]
        g["means3D"] = g["means3D"] * (z / g["means3D"][:, 2])[:, None]
        return g
    if name in ANISO:
        g = _base(gen, n, W, H)
        s = torch.tensor(ANISO[name]) * (0.9 + 0.2 * u(n, 3))
        g["scales"] = torch.stack([s[torch.arange(n), (idx + k) % 3] for k in range(3)], dim=1)  # the long axis rotates
        return g
    if name == "tiny":
        g = _base(gen, n, W, H)
        g["scales"] = 1e-7 * (0.8 + 0.4 * u(n, 3))
        return g
    if name == "huge":
        g = _base(gen, n, W, H)
        g["scales"] = 2.0 + 3.0 * u(n, 3)
        return g
    if name == "clamped":
        # row i drives i % 4 of its channels below zero with the dc term, starting at channel (i // 4) % 3
        g = _base(gen, n, W, H, rest_sigma=0.03)
        k, first = idx % 4, (idx // 4) % 3
        ch = torch.arange(3)[None, :]
        neg = ((ch - first[:, None]) % 3) < k[:, None]
        level = 0.25 + 0.75 * u(n, 3)  # |colour| of the dc term alone
        g["shs"][:, 0] = (torch.where(neg, -level, level) - 0.5) / O.SH_C0
        return g
    if name == "behind":
        g = _base(gen, n, W, H)
        kind = idx % 7
        back = torch.tensor([-50.0, 0.0, -44.0]) + 0.5 * (u(n, 3) - 0.5)  # behind every orbit camera
        z = g["means3D"][:, 2]
        off = torch.stack([sign(n) * (3.0 + u(n)) * tanx * z, sign(n) * (3.0 + u(n)) * tany * z, z], dim=1)
        g["means3D"] = torch.where((kind == 0)[:, None], back, torch.where((kind == 3)[:, None], off, g["means3D"]))
        return g
    raise ValueError(name)


def _raw_from_plain(gen, g, W, H):
    """the `raw` family: un-normalised quaternions (|q| in 0.1 .. 10), log-scales with a jitter within +-0.5, logits
    within +-6 (beyond those the float64 gradient itself is ill-conditioned: s(1-s) and the normalisation cancel)"""
    n = g["means3D"].shape[0]
    z = g["means3D"][:, 2]
    return dict(xyz=g["means3D"], scaling=torch.log(0.01 * z)[:, None] + (torch.rand(n, 3, generator=gen) - 0.5),
                rotation=g["rotations"] * 10.0 ** (2.0 * torch.rand(n, 1, generator=gen) - 1.0),
                features_dc=g["shs"][:, :1].contiguous(), features_rest=g["shs"][:, 1:].contiguous(),
                opacity=(2.0 * torch.randn(n, 1, generator=gen)).clamp(-6.0, 6.0))


@functools.lru_cache(maxsize=None)
def _family(name, N, W, H, deg, seed, B, scale_modifier, sh_coeffs):
    gen = torch.Generator().manual_seed(seed)
    idx = torch.arange(N)

    def draw(ix):
        g = _draw(name, gen, ix, W, H)
        if name == "raw":
            g = _raw_from_plain(gen, g, W, H)
        for k in ("shs", "features_rest"):
            if k in g:
                g[k] = g[k][:, : sh_coeffs - (k == "features_rest")].contiguous()
        return {k: v.float().contiguous() for k, v in g.items()}

    cams = cameras(B, W, H)
    rows = draw(idx)
    act = lambda r: activate(r) if name == "raw" else r  # noqa: E731
    for _ in range(REDRAW_ROUNDS):
        bad = margin_violations(act(rows), cams, W, H, deg, scale_modifier)
        if not bool(bad.any()):
            break
        new = draw(idx[bad])
        for k in rows:
            rows[k][bad] = new[k]
    assert not bool(margin_violations(act(rows), cams, W, H, deg, scale_modifier).any()), \
        f"family {name}: rows inside a margin after {REDRAW_ROUNDS} rounds of re-drawing"
    return rows, cams


def family(name, N, W, H, deg, seed, B=1, scale_modifier=1.0, sh_coeffs=16):
    """-> (inputs, cams): N rows of family `name` for the first B orbit cameras, every margin holding in float64 for
    every camera (offending rows are re-drawn from the same generator; none is masked out).  inputs: the five activated
    tensors (KEYS), for `raw` the six raw parameters (RAW_KEYS); float32.  The tensors are shared: do not modify them."""
    assert name in FAMILIES and (W, H) in FRAMES
    return _family(name, N, W, H, deg, seed, B, float(scale_modifier), sh_coeffs)


def upstream(B, N, seed=5):
    """incoming gradients (dL_dmeans2D [B,N,2], dL_dconic_opacity [B,N,4], dL_drgb [B,N,3]): randn from a fixed seed,
    every third row all zero for all cameras"""
    gen = torch.Generator().manual_seed(seed)
    G2, Gco, Grgb = (torch.randn(B, N, k, generator=gen) for k in (2, 4, 3))
    for t in (G2, Gco, Grgb):
        t[:, 1::3] = 0.0
    return G2, Gco, Grgb


# ------------------------------------------------------------------------------------------------ references
def k11_conic_gradient(conic_opacity, g_conic_opacity):
    """K11 as include/gsraster.h defines it (and the CUDA backward it restates) differentiates conic = (c, -b, a) / det
    with 1 / (det^2 + 1e-7) in the place of 1 / det^2: its dL/d(a, b, c) is the true one times det^2 / (det^2 + 1e-7),
    up to 1.2e-5 below it at det = 0.09, the smallest cov2D.  Autograd does not know, and the per-row check sees it (the
    `tiny` rows, 25 units off before this was restated).  dL/d(a, b, c) is linear in the incoming (gA, gB, gC), so the
    defined gradient is autograd's for (gA, gB, gC) / (1 + 1e-7 (AC - B^2)^2), AC - B^2 = 1 / det: that is returned."""
    A, Bc, Cc = conic_opacity[:, 0], conic_opacity[:, 1], conic_opacity[:, 2]
    f = 1.0 / (1.0 + 0.0000001 * (A * Cc - Bc * Bc) ** 2)
    return torch.cat([g_conic_opacity[:, :3] * f[:, None], g_conic_opacity[:, 3:]], dim=1)


def reference(inputs, cams, deg, upstream, dtype, raw, scale_modifier=1.0):
    """oracle/torch_oracle.preprocess(..., return_aux=True) per camera in `dtype`, and torch.autograd.grad with the given
    incoming gradients.  -> dict: means2D [B,N,2], depths [B,N], conic_opacity [B,N,4], rgb [B,N,3], cov3D [B,N,6],
    radii int32 [B,N], clamped bool [B,N,3] (zeros for culled rows), and the input gradients summed over the cameras --
    GRADS_ACT with respect to the activated tensors, or for raw=True GRADS_RAW with respect to the raw parameters, the
    getters applied first in the same dtype.  The conic's incoming gradient goes through k11_conic_gradient first."""
    W, H = cams[0].image_width, cams[0].image_height
    G2, Gco, Grgb = (t.to(dtype) for t in upstream)
    if raw:
        leaves = [inputs[k].to(dtype).clone().requires_grad_() for k in RAW_KEYS]
        a = activate(dict(zip(RAW_KEYS, leaves)), dtype)
        ins = [a[k] for k in KEYS]
    else:
        leaves = [inputs[k].to(dtype).clone().requires_grad_() for k in KEYS]
        ins = leaves
    out = {k: [] for k in OUTPUTS + ("radii", "clamped")}
    total = None
    for b, cam in enumerate(cams):
        tx, ty = tanfov(cam)
        m2, rgb, co, radii, depths, cov3D, clamped = O.preprocess(
            *ins, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center,
            W=W, H=H, tanfovx=tx, tanfovy=ty, sh_degree=deg, scale_modifier=scale_modifier, return_aux=True)
        grads = torch.autograd.grad([m2, co, rgb], leaves, [G2[b], k11_conic_gradient(co.detach(), Gco[b]), Grgb[b]],
                                    allow_unused=True, retain_graph=True)
        grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
        total = grads if total is None else [t + g for t, g in zip(total, grads)]
        for k, v in zip(OUTPUTS + ("radii", "clamped"), (m2, depths, co, rgb, cov3D, radii, clamped)):
            out[k].append(v.detach())
    res = {k: torch.stack(v) for k, v in out.items()}
    res.update(zip(GRADS_RAW if raw else GRADS_ACT, total))
    return res


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    """one case of the GPU file (and of the CPU file's cap / C-restatement checks): which entry points, which rows"""

    def __init__(self, form, fam, deg, N, frame=0, B=1, stride=0, sm=1.0, M=16):
        assert form in ("act", "raw", "rawb") and (form == "rawb" or B == 1) and (fam != "raw" or form != "act")
        self.form, self.fam, self.deg, self.N, self.B, self.stride, self.sm, self.M = form, fam, deg, N, B, stride, sm, M
        self.W, self.H = FRAMES[frame]
        self.seed = 100 + 7 * N + deg
        self.id = f"{form}-{fam}-d{deg}-N{N}-{self.W}x{self.H}-B{B}-s{stride}" + (f"-sm{sm}" if sm != 1.0 else "") + \
            (f"-M{M}" if M != 16 else "")

    @property
    def is_raw(self):
        return self.form != "act"

    def inputs(self):
        """-> (inputs of the case's entry points, cams)"""
        ins, cams = family(self.fam, self.N, self.W, self.H, self.deg, self.seed, self.B, self.sm, self.M)
        if self.is_raw and self.fam != "raw":
            ins = _to_raw_cached(self.fam, self.N, self.W, self.H, self.deg, self.seed, self.B, self.sm, self.M)
        return ins, cams

    def references(self):
        """-> (float64 reference, float32 reference), computed once and shared: do not modify"""
        return _references(self.form != "act", self.fam, self.N, self.W, self.H, self.deg, self.seed, self.B, self.sm,
                           self.M)

    def tensors(self):
        """the float tensors that go through assert_rows_close: outputs per camera, then the gradients"""
        return OUTPUTS + (GRADS_RAW if self.is_raw else GRADS_ACT)


@functools.lru_cache(maxsize=None)
def _to_raw_cached(fam, N, W, H, deg, seed, B, sm, M):
    return to_raw(family(fam, N, W, H, deg, seed, B, sm, M)[0])


@functools.lru_cache(maxsize=None)
def _references(raw, fam, N, W, H, deg, seed, B, sm, M):
    ins, cams = family(fam, N, W, H, deg, seed, B, sm, M)
    if raw and fam != "raw":
        ins = _to_raw_cached(fam, N, W, H, deg, seed, B, sm, M)
    up = upstream(B, N)
    return (reference(ins, cams, deg, up, torch.float64, raw, sm), reference(ins, cams, deg, up, torch.float32, raw, sm))


def _cases():
    """Not the full product.  Per root form: `plain` and `jclamp` at every N of {1, 127, 128, 129, 257, 1031} (K1's
    workgroup is 256 rows, K11's 128: full, ragged and single-row last workgroups) with the two gradient strides
    alternating between them; every other family at degree 3 and at one lower degree; degrees 0 .. 3 with 16 coefficients
    and one raw case with 4 (the unstaged branch of the raw K11); scale_modifier 0.7 once per form; both frames; the
    batched form with B in {1, 3, 5} (5 is past the camera queue's first refill)."""
    cs = []
    n_deg_b = ((1031, 3, 3), (257, 3, 5), (129, 2, 1), (128, 1, 3), (127, 0, 5), (1, 3, 5))
    others = (("near", 3, 257), ("near", 1, 129), ("aniso", 3, 257), ("aniso", 2, 127), ("tiny", 3, 129), ("tiny", 0, 257),
              ("huge", 3, 128), ("huge", 1, 257), ("clamped", 3, 257), ("clamped", 2, 129), ("behind", 3, 257),
              ("behind", 0, 128))
    for form in ("act", "raw", "rawb"):
        for j, (N, deg, B) in enumerate(n_deg_b):
            B = B if form == "rawb" else 1
            cs.append(Case(form, "plain", deg, N, frame=j % 2, B=B, stride=9 * (j % 2)))
            cs.append(Case(form, "jclamp", deg, N, frame=(j + 1) % 2, B=B, stride=9 * ((j + 1) % 2)))
        for j, (fam, deg, N) in enumerate(others):
            B = (1, 3, 5)[j % 3] if form == "rawb" else 1
            B = 3 if (form == "rawb" and N > 200 and B == 5) else B  # (keeps the float64 oracle's share of a case small)
            fam = "aniso_mild" if (fam == "aniso" and form != "act") else fam
            cs.append(Case(form, fam, deg, N, frame=0, B=B, stride=9 * (j % 2)))
        cs.append(Case(form, "plain", 3, 257, frame=0, B=3 if form == "rawb" else 1, stride=9, sm=0.7))
        if form != "act":
            cs.append(Case(form, "raw", 3, 257, frame=1, B=3 if form == "rawb" else 1, stride=9))
            cs.append(Case(form, "raw", 1, 129, frame=0, B=5 if form == "rawb" else 1, stride=0))
    cs.append(Case("raw", "plain", 1, 129, frame=0, stride=9, M=4))
    cs.append(Case("raw", "jclamp", 1, 257, frame=0, stride=0, M=4))
    return cs


CASES = _cases()
