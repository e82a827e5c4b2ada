"""Float64 restatements of the 3D smoothing filter (include/gsraster.h: gsr_filter3d_*), a float32 numpy evaluation of
the apply kernels' formulas (one rounding per operation, no code under test), and the builders of the edge inputs.
Host code only: the CPU tests check this file against itself, the GPU tests check the kernels against it.

The distance builder guarantees that every (row, camera) pair decides each of the three inequalities
    t.z > 0.2f,   |fx t.x| <= 0.65f W t.z,   |fy t.y| <= 0.65f H t.z
at least MARGIN = 1e-4 relative away from equality in float64 (rows that do not are redrawn), so that a float32 kernel,
whose two sides carry a few 2^-24 of relative error, can never decide differently from the float64 rule.  There are no
rows placed exactly on a threshold."""
import math

import numpy as np
import torch

import synthetic_scene as S

MARGIN = 1e-4
Z_NEAR = float(np.float32(0.2))
SCREEN = float(np.float32(0.65))
K_FILTER = float(np.float32(math.sqrt(0.2)))
CAM_CHUNK = 64  # cameras csrc/filter3d.hip stages in LDS per pass (F3D_CAM_CHUNK)


# ------------------------------------------------------------------------------------------------ cameras and rows
def make_cameras(C, W, H, seed=0):
    """C cameras in the box [-1,1]^2 x [-1,0] looking along +z with a yaw of up to 40 degrees, focal lengths between
    0.7 W and 1.6 W with camera 0 the SHORTEST (focal_max is never camera 0's when C > 1)"""
    rnd = np.random.RandomState(1000 + seed)
    cams = []
    for k in range(C):
        th = math.radians(rnd.uniform(-40.0, 40.0)) if k else 0.0
        fx = W * (0.7 if k == 0 else rnd.uniform(0.8, 1.6))
        fy = fx * (1.0 if k % 2 == 0 else 1.25)
        Rw2c = torch.tensor([[math.cos(th), 0.0, -math.sin(th)], [0.0, 1.0, 0.0], [math.sin(th), 0.0, math.cos(th)]],
                            dtype=torch.float64)
        pos = torch.tensor([rnd.uniform(-1, 1), rnd.uniform(-1, 1), rnd.uniform(-1, 0)], dtype=torch.float64)
        cams.append(S.SyntheticCamera(k, W, H, fx=fx, fy=fy, R=Rw2c.t(), T=-(Rw2c @ pos)))
    return cams


def pack_cameras(cams):
    """[C,40] float32: what diff_gaussian_rasterization.pack_camera builds per camera"""
    rows = []
    for c in cams:
        tail = [math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5), 0.0, 0.0, 0.0]
        rows.append(np.concatenate([c.world_view_transform.reshape(16).numpy(), c.full_proj_transform.reshape(16).numpy(),
                                    c.camera_center.reshape(3).numpy(), np.asarray(tail)]).astype(np.float32))
    return np.stack(rows) if rows else np.zeros((0, 40), np.float32)


def pairs64(xyz, cams, W, H):
    """float64, per (row, camera): t [N,C,3], sum of |terms| of t.z [N,C], the three relative margins [N,C,3]
    (positive: the inequality holds) and valid [N,C]"""
    p = np.asarray(xyz, np.float64)
    V = np.asarray(cams, np.float64)[:, :16].reshape(-1, 4, 4)  # row-vector convention: t = [p, 1] V
    t = np.einsum("nk,ckj->ncj", p, V[:, :3, :3]) + V[None, :, 3, :3]
    terms = np.abs(p[:, None, :] * V[None, :, :3, 2]).sum(-1) + np.abs(V[None, :, 3, 2])
    tan = np.asarray(cams, np.float64)[:, 35:37]
    fx, fy = W / (2.0 * tan[:, 0]), H / (2.0 * tan[:, 1])

    def rel(lhs, rhs):  # (rhs - lhs) relative to the larger side
        return (rhs - lhs) / np.maximum(np.maximum(np.abs(lhs), np.abs(rhs)), 1e-300)

    tz = t[..., 2]
    m = np.stack([rel(np.full_like(tz, Z_NEAR), tz),
                  rel(np.abs(fx[None] * t[..., 0]), SCREEN * W * tz),
                  rel(np.abs(fy[None] * t[..., 1]), SCREEN * H * tz)], axis=-1)
    valid = (tz > Z_NEAR) & (np.abs(fx[None] * t[..., 0]) <= SCREEN * W * tz) & \
        (np.abs(fy[None] * t[..., 1]) <= SCREEN * H * tz)
    return t, terms, m, valid


def decisive(margins):
    """[N] bool: every inequality of every pair of the row is at least MARGIN away from equality"""
    return (np.abs(margins) >= MARGIN).all(axis=(1, 2))


def _world_from_camera(cam_row, pc):
    """world point (float64) whose camera-space position under the packed record is pc"""
    V = np.asarray(cam_row, np.float64)[:16].reshape(4, 4)
    return (np.asarray(pc, np.float64) - V[3, :3]) @ np.linalg.inv(V[:3, :3])


def special_rows(cams, W, H):
    """rows placed against CAMERA 0 (float64, then rounded to float32 by the caller), name -> world point:
    `inside_margin` projects at 0.60 W from the image centre (off the screen, inside the 15 % margin: valid),
    `outside_margin` at 0.70 W (not valid), `margin_y` the same along y at 0.62 H, `near_in` / `near_out` at depths
    0.25 / 0.15 on the axis, `behind_all` far behind every camera of make_cameras."""
    tanx, tany = float(cams[0, 35]), float(cams[0, 36])
    z = 5.0
    rows = {
        "inside_margin": _world_from_camera(cams[0], [0.60 * 2.0 * tanx * z, 0.0, z]),
        "outside_margin": _world_from_camera(cams[0], [-0.70 * 2.0 * tanx * z, 0.0, z]),
        "margin_y": _world_from_camera(cams[0], [0.0, 0.62 * 2.0 * tany * z, z]),
        "near_in": _world_from_camera(cams[0], [0.0, 0.0, 0.25]),
        "near_out": _world_from_camera(cams[0], [0.0, 0.0, 0.15]),
        "behind_all": np.array([0.3, -0.2, -50.0]),
    }
    return rows


SPECIAL = ("inside_margin", "outside_margin", "margin_y", "near_in", "near_out", "behind_all")


def build_distance_case(N, C, W=64, H=48, seed=0, unseen=False):
    """-> dict(xyz [N,3] f32, cams [C,40] f32, W, H, special {name: row index}).  Random rows in a box around the
    cameras' view (in front, to the sides and behind), the special rows first while they fit; `unseen`: every row lies
    behind every camera.  Rows whose margins are not decisive are redrawn."""
    cams = pack_cameras(make_cameras(C, W, H, seed))
    rnd = np.random.RandomState(seed * 7919 + 13 * N + C)
    rows, special = [], {}
    if not unseen:
        for name, p in special_rows(cams, W, H).items():
            if len(rows) < N and (N >= len(SPECIAL) or name in ("inside_margin",)):
                special[name] = len(rows)
                rows.append(np.asarray(p, np.float64).astype(np.float32))
    xyz = np.stack(rows) if rows else np.zeros((0, 3), np.float32)
    if len(rows):
        assert decisive(pairs64(xyz, cams, W, H)[2]).all(), "a special row is not decisive"
    while xyz.shape[0] < N:
        n = 2 * (N - xyz.shape[0]) + 8
        if unseen:
            cand = np.stack([rnd.uniform(-8, 8, n), rnd.uniform(-8, 8, n), rnd.uniform(-60, -20, n)], 1)
        else:
            cand = np.stack([rnd.uniform(-9, 9, n), rnd.uniform(-7, 7, n), rnd.uniform(-4, 14, n)], 1)
        cand = cand.astype(np.float32)
        cand = cand[decisive(pairs64(cand, cams, W, H)[2])]
        xyz = np.concatenate([xyz, cand[:N - xyz.shape[0]]])
    return dict(xyz=np.ascontiguousarray(xyz), cams=cams, W=W, H=H, special=special)


# ------------------------------------------------------------------------------------------------ (a) + (b), float64
def focal_max64(cams, W):
    return float((W / (2.0 * np.asarray(cams, np.float64)[:, 35])).max())


def filter_ref(xyz, cams, W, H, global_max=None):
    """-> dict(seen [N] bool, n_valid [N], dist [N] (0 when unseen), gmax, filter [N], tol [N]): the float64 rule.
    `global_max`: the max over all shards' seen rows in place of this shard's.  tol: the bound of the float32 filter
    against `filter`, 8 x 2^-24 x (sum of |terms| of the deciding t.z) x sqrt(0.2) / focal_max -- four float32 roundings
    in the dot product, doubled."""
    t, terms, _, valid = pairs64(xyz, cams, W, H)
    N = t.shape[0]
    tz = np.where(valid, t[..., 2], np.inf)
    seen = valid.any(1) if valid.shape[1] else np.zeros(N, bool)
    arg = tz.argmin(1) if valid.shape[1] else np.zeros(N, int)
    dist = np.where(seen, tz[np.arange(N), arg] if valid.shape[1] else 0.0, 0.0)
    tsum = terms[np.arange(N), arg] if valid.shape[1] else np.zeros(N)
    if seen.any():
        top = int(np.where(seen, dist, -1.0).argmax())
        gmax, gterm = float(dist[top]), float(tsum[top])
    else:
        gmax, gterm = 0.0, 0.0
    if global_max is not None:
        gmax, gterm = global_max
    fm = focal_max64(cams, W) if len(cams) else 1.0
    d = np.where(seen, dist, gmax)
    f = K_FILTER * d / fm if gmax > 0 else np.zeros(N)
    tol = 8.0 * 2.0 ** -24 * np.where(seen, tsum, gterm) * K_FILTER / fm
    return dict(seen=seen, n_valid=valid.sum(1), dist=dist, gmax=gmax, gterm=gterm, filter=f, tol=tol, valid=valid,
                tz=t[..., 2])


# ------------------------------------------------------------------------------------------------ (c), float64
def _forward_torch(x, o, f):
    """torch float64, differentiable: the definition in a form whose value AND whose autograd derivative are sums of
    terms of one sign (no cancellation anywhere on the input grid).  u_k = f^2 / s_k^2;
    log s'_k = x_k + log1p(u_k) / 2;  log c = -sum_k log1p(u_k) / 2;  with sigma = sigmoid(o), p = sigma c:
    logit(p) = (log sigma + log c) - log((1 - sigma) + sigma (1 - c))"""
    u = (f * f) * torch.exp(-2.0 * x)
    half = 0.5 * torch.log1p(u)
    logc = -half.sum(dim=1, keepdim=True)
    log_sigma = -torch.log1p(torch.exp(-o))
    # (not torch.sigmoid: its backward forms 1 - sigma from the rounded sigma, 5e-8 relative at o = 20)
    sigma, one_minus_sigma = 1.0 / (1.0 + torch.exp(-o)), 1.0 / (1.0 + torch.exp(o))
    return x + half, (log_sigma + logc) - torch.log(one_minus_sigma + sigma * -torch.expm1(logc))


def apply_forward_ref(x, o, f):
    """(_scaling [N,3], _opacity [N,1], f [N,1]) -> (scaling_eff, opacity_eff, Ms, Mo) in float64; a row with f == 0
    returns its inputs (the definition).  M: the sum of the magnitudes of the addends an output is formed from in
    opacity_eff = o + log c - log1p((1 - c) e^o) and scaling_eff = x + log(s' / s): the unit of a float32 evaluation's
    rounding error is 2^-24 M"""
    x, o, f = (torch.from_numpy(np.asarray(a, np.float64)) for a in (x, o, f))
    # (the VALUE in the form whose addends do not cancel; _forward_torch's form, made for its derivative, loses
    # 1e-16 absolute where log sigma and log(1 - p) cancel, which is large against an opacity_eff of 1e-12)
    u = (f * f) * torch.exp(-2.0 * x)
    half = 0.5 * torch.log1p(u)
    L = half.sum(dim=1, keepdim=True)
    tail = torch.log1p(-torch.expm1(-L) * torch.exp(o))
    s, q = torch.where(f == 0, x, x + half), torch.where(f == 0, o, (o - L) - tail)
    Ms = x.abs() + half
    Mo = o.abs() + L + tail
    return s.numpy(), q.numpy(), Ms.numpy(), Mo.numpy()


def apply_backward_ref(x, o, f, gs, go):
    """closed form, float64 -> (d_scaling, d_opacity, Ms, Mo):
    d_scaling_k = g_s_k r_k + g_o (1 - r_k) / (1 - p),  d_opacity = g_o (1 - sigma) / (1 - p), with
    r_k = 1 / (1 + u_k), 1 - r_k = u_k / (1 + u_k), 1 - sigma = 1 / (1 + e^o), 1 - p = (1 - sigma) + sigma (1 - c)"""
    x, o, f, gs, go = (np.asarray(a, np.float64) for a in (x, o, f, gs, go))
    u = (f * f) * np.exp(-2.0 * x)
    r, omr = 1.0 / (1.0 + u), u / (1.0 + u)
    omc = -np.expm1(-(0.5 * np.log1p(u)).sum(1, keepdims=True))
    sig, oms = 1.0 / (1.0 + np.exp(-o)), 1.0 / (1.0 + np.exp(o))
    omp = oms + sig * omc
    a, b = gs * r, go * omr / omp
    do = go * (oms / omp)  # (f == 0: omp is oms and the quotient is exactly 1)
    return a + b, do, np.abs(a) + np.abs(b), np.abs(do)


# ------------------------------------------------------------------------------------------------ (c), float32 numpy
F32 = np.float32


def _row32(x, f):
    """the per-axis quantities of csrc/filter3d.hip's f3d_row in numpy float32, one rounding per operation"""
    with np.errstate(all="ignore"):
        q = f * np.exp(-x)
        small = q <= F32(1)
        iq = F32(1) / q
        w = np.where(small, q * q, iq * iq).astype(F32)
        h = F32(0.5) * np.log1p(w)
        inv = F32(1) / (F32(1) + w)
        l = np.where(small, h, np.log(q) + h).astype(F32)
        ls = np.where(small, x + h, np.log(f) + h).astype(F32)
        r = np.where(small, inv, w * inv).astype(F32)
        omr = np.where(small, w * inv, inv).astype(F32)
        L = ((l[:, 0:1] + l[:, 1:2]) + l[:, 2:3]).astype(F32)
        omc = (-np.expm1(-L)).astype(F32)
    return ls, r, omr, L, omc


def apply_forward_f32(x, o, f):
    x, o, f = (np.asarray(a, F32) for a in (x, o, f))
    ls, _, _, L, omc = _row32(x, f)
    with np.errstate(all="ignore"):
        lo = (o - L) - np.log1p(omc * np.exp(o))
        hi = -L - np.log(np.exp(-np.minimum(o, F32(80))) + omc)
        q = np.where(o <= F32(60), lo, hi).astype(F32)
    ident = f == 0
    return np.where(ident, x, ls).astype(F32), np.where(ident, o, q).astype(F32)


def apply_backward_f32(x, o, f, gs, go):
    x, o, f, gs, go = (np.asarray(a, F32) for a in (x, o, f, gs, go))
    _, r, omr, _, omc = _row32(x, f)
    with np.errstate(all="ignore"):
        e = np.exp(np.where(o <= 0, o, -np.minimum(o, F32(80)))).astype(F32)
        D = np.where(o <= 0, F32(1) + e * omc, e + omc).astype(F32)
        u = ((F32(1) + e) / D).astype(F32)
        v = np.where(o <= 0, F32(1) / D, e / D).astype(F32)
        ds = (gs * r + (go * omr) * u).astype(F32)
        do = (go * v).astype(F32)
    ident = f == 0
    return np.where(ident, gs, ds).astype(F32), np.where(ident, go, do).astype(F32)


# ------------------------------------------------------------------------------------------------ (c), inputs
SCALINGS = (-18.0, -7.0, 0.0, 5.0)
FILTERS = (0.0, 1e-6, 1e-3, 1.0, 1e3)
OPACITIES = (-20.0, -2.0, 0.0, 2.0, 20.0)


def build_apply_case(N, seed=0):
    """N rows over the issue's grid: every axis of _scaling drawn from SCALINGS on its own (the three axes mixed), f
    from FILTERS, _opacity from OPACITIES; the first rows walk the (f, opacity) grid so that a case of 25 rows or more
    holds every pair; gradients of mixed sign.  -> dict of float32 arrays x [N,3], o [N,1], f [N,1], gs [N,3], go [N,1]"""
    rnd = np.random.RandomState(77 + seed + N)
    x = np.asarray(SCALINGS, F32)[rnd.randint(0, len(SCALINGS), (N, 3))]
    idx = np.arange(N)
    f = np.asarray(FILTERS, F32)[np.where(idx < 25, idx % 5, rnd.randint(0, 5, N))].reshape(N, 1)
    o = np.asarray(OPACITIES, F32)[np.where(idx < 25, (idx // 5) % 5, rnd.randint(0, 5, N))].reshape(N, 1)
    gs = (rnd.standard_normal((N, 3)) * np.exp(rnd.uniform(-3, 3, (N, 3)))).astype(F32)
    go = (rnd.standard_normal((N, 1)) * np.exp(rnd.uniform(-3, 3, (N, 1)))).astype(F32)
    return dict(x=x, o=o, f=f, gs=gs, go=go)


def worst_units(got, ref, M):
    """the largest |got - ref| in units of 2^-24 M over the elements (M == 0 with got == ref counts as 0)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    unit = 2.0 ** -24 * M
    with np.errstate(all="ignore"):
        e = np.where(err == 0, 0.0, err / unit)
    return float(np.nanmax(e)) if e.size else 0.0
