"""Plain numpy restatements of the two rules of csrc/tsdf.hip in a dtype of the caller's choice (float64:
the arbiter; float32 on the CPU: the yardstick of helpers.assert_elem_close), and the scenes of the TSDF tests.
integrate(): the per-voxel, per-view rule on dense [Z,Y,X] arrays; integrate_refs() runs it in both dtypes on the SAME
fp32 inputs and marks the voxels whose decisions an fp32 rounding can flip (`fragile`).  mesh(): marching tetrahedra on
the Kuhn split; the triangle rule is logic here (parities of permutations), a 16-row table in the kernel."""
import itertools
import math

import numpy as np

PERMS = list(itertools.permutations(range(3)))


def _parity(p):
    p, s = list(p), 1
    for i in range(len(p)):
        while p[i] != i:
            j = p[i]
            p[i], p[j] = p[j], p[i]
            s = -s
    return s


def tet_triangles(mask):
    """the triangles of a POSITIVELY oriented tetrahedron (det[p1 - p0, p2 - p0, p3 - p0] > 0) whose vertex q is inside
    iff bit q of `mask`: a list of triples of edges (a, b), a < b, wound so that the normal leaves the inside"""
    ins = [q for q in range(4) if mask >> q & 1]
    out = [q for q in range(4) if not mask >> q & 1]
    edge = lambda a, b: (min(a, b), max(a, b))
    if len(ins) in (1, 3):
        i = (ins if len(ins) == 1 else out)[0]
        j, k, l = [q for q in range(4) if q != i]
        if _parity((i, j, k, l)) < 0:
            k, l = l, k
        tri = [edge(i, j), edge(i, k), edge(i, l)]
        return [tri if len(ins) == 1 else [tri[0], tri[2], tri[1]]]
    if len(ins) == 2:
        (i, j), (k, l) = ins, out
        if _parity((i, j, k, l)) < 0:
            k, l = l, k
        a, b, c, d = edge(i, k), edge(i, l), edge(j, l), edge(j, k)
        return [[a, b, c], [a, c, d]]
    return []


def tets():
    """[(corner ids of v0..v3, orientation)] of the Kuhn split of the unit cell"""
    return [((0, 1 << a, 1 << a | 1 << b, 7), _parity((a, b, c))) for a, b, c in PERMS]


# ------------------------------------------------------------------------------------------------ integration
def integrate(dtype, origin, voxel_size, dims, trunc, depths, views, tanfovx, tanfovy, colors=None, weights=None,
              depth_trunc=math.inf, near=0.2):
    """-> (tsdf, weight, rgb or None) dense [Z,Y,X] / [3,Z,Y,X] in `dtype`, and the float margins the fragile mask is
    made of.  depths fp32 [V,H,W], views fp32 [V,4,4] (row-vector convention), colors fp32 [V,3,H,W] or None."""
    f = dtype
    X, Y, Z = dims
    V, H, W = depths.shape
    o = [f(np.float32(v)) for v in origin]
    vs, tr, nr, dt = f(np.float32(voxel_size)), f(np.float32(trunc)), f(np.float32(near)), f(np.float32(depth_trunc))
    tx, ty = f(np.float32(tanfovx)), f(np.float32(tanfovy))
    iz, iy, ix = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    p = [o[0] + vs * ix.astype(f), o[1] + vs * iy.astype(f), o[2] + vs * iz.astype(f)]
    tsdf, wgt = np.ones((Z, Y, X), f), np.zeros((Z, Y, X), f)
    rgb = np.zeros((3, Z, Y, X), f) if colors is not None else None
    fragile = np.zeros((Z, Y, X), bool)
    half = lambda a: np.abs(a - np.floor(a) - 0.5)  # distance to the nearest half-integer
    for v in range(V):
        m = views[v].astype(f)
        x = m[0, 0] * p[0] + m[1, 0] * p[1] + m[2, 0] * p[2] + m[3, 0]
        y = m[0, 1] * p[0] + m[1, 1] * p[1] + m[2, 1] * p[2] + m[3, 1]
        z = m[0, 2] * p[0] + m[1, 2] * p[1] + m[2, 2] * p[2] + m[3, 2]
        front = ~(z <= nr)
        with np.errstate(all="ignore"):
            px = ((x / (z * tx) + f(1)) * f(W) - f(1)) * f(0.5)
            py = ((y / (z * ty) + f(1)) * f(H) - f(1)) * f(0.5)
        rx, ry = np.rint(px), np.rint(py)
        inside = front & (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
        jx, jy = np.where(inside, rx, 0).astype(np.int64), np.where(inside, ry, 0).astype(np.int64)
        d = depths[v][jy, jx].astype(f)
        seen = inside & (d > 0) & (d <= dt)
        sdf = d - z
        take = seen & (sdf >= -tr) & (sdf <= tr)
        wv = f(1) if weights is None else f(np.float32(weights[v]))
        wn = wgt + wv
        tsdf = np.where(take, (tsdf * wgt + (sdf / tr) * wv) / wn, tsdf)
        if rgb is not None:
            c = colors[v][:, jy, jx].astype(f)
            rgb = np.where(take[None], (rgb * wgt[None] + c * wv) / wn[None], rgb)
        wgt = np.where(take, wn, wgt)
        with np.errstate(all="ignore"):
            fragile |= np.abs(z - nr) <= 1e-4
            fragile |= front & ((half(px) <= 1e-3) | (half(py) <= 1e-3))
            fragile |= seen & (np.abs(np.abs(sdf) - tr) <= 1e-4 * tr)
    return tsdf, wgt, rgb, fragile


def integrate_refs(*args, **kw):
    """-> (ref64, ref32, fragile): (tsdf, weight, rgb) of both dtypes, and the voxels that are not held to the reference"""
    t64, w64, c64, frag = integrate(np.float64, *args, **kw)
    t32, w32, c32, _ = integrate(np.float32, *args, **kw)
    return (t64, w64, c64), (t32, w32, c32), frag | (w32.astype(np.float64) != w64)


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """fp32 [4,4] view matrix in the row-vector convention (t = [p, 1] @ M): +z towards the target, +y down"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(-np.asarray(up, np.float64), fwd)  # (y down: x = down x forward ... = up' x fwd with up' = -up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])  # world -> camera rows
    M = np.eye(4)
    M[:3, :3] = R.T
    M[3, :3] = -R @ eye
    return M.astype(np.float32)


SPHERE_C, SPHERE_R, PLANE_Y = np.array([0.05, -0.1, 0.1]), 0.45, 0.55  # the plane y = PLANE_Y lies below the sphere (+y is down)


def render_depth(view, W, H, tanfovx, tanfovy):
    """z-depth fp32 [H,W] of the sphere above the plane by analytic fp64 ray intersections, 0 where a ray misses both;
    colour fp32 [3,H,W]: a smooth function of the hit point"""
    M = view.astype(np.float64)
    R, eye = M[:3, :3].T, -M[:3, :3] @ M[3, :3]  # p_cam = R (p - eye)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dcam = np.stack([((2 * i + 1) / W - 1) * tanfovx, ((2 * j + 1) / H - 1) * tanfovy, np.ones((H, W))], -1)
    dw = dcam @ R  # rows: R^T dcam
    oc = eye - SPHERE_C
    a, b, c = (dw * dw).sum(-1), 2 * (dw @ oc), oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    with np.errstate(all="ignore"):
        s_sph = np.where(disc > 0, (-b - np.sqrt(np.abs(disc))) / (2 * a), np.inf)
        s_pl = (PLANE_Y - eye[1]) / dw[..., 1]
    s_sph = np.where(s_sph > 0, s_sph, np.inf)
    s_pl = np.where(s_pl > 0, s_pl, np.inf)
    s = np.minimum(s_sph, s_pl)
    hit = np.isfinite(s)
    pt = eye + dw * np.where(hit, s, 0.0)[..., None]
    col = np.stack([0.5 + 0.4 * np.sin(3 * pt[..., 0]), 0.5 + 0.4 * np.cos(2 * pt[..., 2]), np.where(s_sph < s_pl, 0.9, 0.2)])
    return np.where(hit, s, 0.0).astype(np.float32), (col * hit).astype(np.float32)


def scene():
    """the integration scene: a 24 x 16 x 32 volume (3 x 2 x 4 bricks) around the sphere, five cameras on a ring and one
    whose centre lies inside the volume (near plane, bricks behind the camera), 64 x 48 images, tanfovx != tanfovy"""
    W, H, tanx, tany = 64, 48, 0.7, 0.5
    dims, vs = (24, 16, 32), 0.1
    origin = (-1.17, -0.83, -1.52)
    eyes = [(3.0 * math.sin(a), -0.6, 3.0 * math.cos(a)) for a in (0.3, 1.5, 2.9, 4.1, 5.4)] + [(0.8, -0.35, -1.0)]
    views = np.stack([look_at(e, SPHERE_C) for e in eyes])
    maps = [render_depth(v, W, H, tanx, tany) for v in views]
    return dict(origin=origin, voxel_size=vs, dims=dims, trunc=0.3, tanfovx=tanx, tanfovy=tany,
                views=views, depths=np.stack([m[0] for m in maps]), colors=np.stack([m[1] for m in maps]))


def integration_cases():
    """name -> keyword arguments of integrate() on top of the scene's: V in {1, 6}, colour, weights, depth_trunc"""
    return {"one_view": dict(V=1, color=False), "one_view_color": dict(V=1, color=True),
            "six": dict(V=6, color=False), "six_color_weights": dict(V=6, color=True, weights=[1, 2, 1, 2, 2, 1]),
            "six_weights": dict(V=6, color=False, weights=[2, 1, 1, 2, 1, 2]),
            "six_color_trunc": dict(V=6, color=True, depth_trunc=3.0)}


def case_refs(sc, V, color, weights=None, depth_trunc=math.inf):
    return integrate_refs(sc["origin"], sc["voxel_size"], sc["dims"], sc["trunc"], sc["depths"][:V], sc["views"][:V],
                          sc["tanfovx"], sc["tanfovy"], colors=sc["colors"][:V] if color else None, weights=weights,
                          depth_trunc=depth_trunc)


# ------------------------------------------------------------------------------------------------- extraction
def mesh(dtype, tsdf, weight, origin, voxel_size, min_weight=0.0, rgb=None):
    """-> (vertices [Nv,3], faces int [Nf,3], colors [Nv,3] or None) of dense [Z,Y,X] planes, vertices in order of first
    use (the kernel's order differs: compare as sets)"""
    f = dtype
    Z, Y, X = tsdf.shape
    t = tsdf.astype(f)
    o, vs = [f(np.float32(v)) for v in origin], f(np.float32(voxel_size))
    valid = (weight > 0) & (weight >= min_weight)
    ok = np.ones((Z - 1, Y - 1, X - 1), bool)
    mixed_lo, mixed_hi = np.zeros_like(ok), np.zeros_like(ok)
    for c in range(8):
        sl = tuple(slice(c >> a & 1, n - 1 + (c >> a & 1)) for a, n in ((2, Z), (1, Y), (0, X)))
        ok &= valid[sl]
        mixed_lo |= t[sl] < 0
        mixed_hi |= ~(t[sl] < 0)
    verts, cols, faces, index = [], [], [], {}
    pos = lambda q: np.array([o[0] + vs * f(q[0]), o[1] + vs * f(q[1]), o[2] + vs * f(q[2])], f)

    def vertex(q0, q1):
        key = (q0, q1)
        if key not in index:
            t0, t1 = t[q0[2], q0[1], q0[0]], t[q1[2], q1[1], q1[0]]
            w = t0 / (t0 - t1)
            p0, p1 = pos(q0), pos(q1)
            index[key] = len(verts)
            verts.append(p0 + (p1 - p0) * w)
            if rgb is not None:
                c0, c1 = rgb[:, q0[2], q0[1], q0[0]].astype(f), rgb[:, q1[2], q1[1], q1[0]].astype(f)
                cols.append(c0 + (c1 - c0) * w)
        return index[key]

    for z, y, x in zip(*np.nonzero(ok & mixed_lo & mixed_hi)):
        corner = lambda c: (int(x) + (c & 1), int(y) + (c >> 1 & 1), int(z) + (c >> 2))
        for cs, sign in tets():
            m = sum(1 << q for q in range(4) if t[corner(cs[q])[::-1]] < 0)
            for tri in tet_triangles(m):
                ids = [vertex(corner(cs[a]), corner(cs[b])) for a, b in tri]
                faces.append(ids if sign > 0 else [ids[0], ids[2], ids[1]])
    return (np.array(verts, f).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3),
            np.array(cols, f).reshape(-1, 3) if rgb is not None else None)


MESH_ORIGIN, MESH_VOXEL = (-1.5, -1.0, -2.0), 0.125  # dyadic: every grid position is exact in fp32 and fp64


def mesh_cases():
    """name -> (tsdf [Z,Y,X] fp32, weight fp32, closed).  The sphere's centre is generic, so that no two vertices tie in
    a coordinate unless both lie exactly on a grid plane (where fp32 and fp64 agree to the bit)."""
    def sphere(dims, c, r):
        X, Y, Z = dims
        iz, iy, ix = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
        p = [MESH_ORIGIN[a] + MESH_VOXEL * i for a, i in enumerate((ix, iy, iz))]
        dist = np.sqrt(sum((p[a] - c[a]) ** 2 for a in range(3))) - r
        return np.clip(dist / (3 * MESH_VOXEL), -1, 1).astype(np.float32)

    big, c = (24, 16, 32), (0.0137, -0.0071, 0.0213)
    s = sphere(big, c, 0.8)
    one = np.ones_like(s)
    half = one.copy()
    half[:, :, :11] = 0  # (the cut runs inside the second brick in x)
    iz, iy, ix = np.meshgrid(np.arange(32), np.arange(16), np.arange(24), indexing="ij")
    plane = ((ix - iz + 3) * 0.25).clip(-1, 1).astype(np.float32)  # zero exactly on the voxels ix - iz = -3
    small = sphere((8, 8, 8), (-1.0713, -0.5571, -1.5537), 0.31)
    return {"sphere": (s, one, True), "sphere_open": (s, half, False), "plane_zero_corners": (plane, np.ones_like(plane), False),
            "one_brick": (small, np.ones_like(small), True)}


def canonical(verts, faces):
    """the mesh as sets: (unique vertices sorted lexicographically, their multiplicities, faces as sorted rows of unique
    ids, each rotated to start at its smallest id).  Vertices that coincide exactly (tsdf == 0 corners) share an id."""
    uniq, inv, count = np.unique(verts, axis=0, return_inverse=True, return_counts=True)
    f = inv.reshape(-1)[faces]
    k = f.argmin(axis=1)
    f = np.stack([np.take_along_axis(f, ((k + s) % 3)[:, None], 1)[:, 0] for s in range(3)], 1) if len(f) else f
    return uniq, count, f[np.lexsort(f.T[::-1])] if len(f) else f


def closed_surface_figures(verts, faces):
    """-> (every directed edge has its opposite exactly once and itself once, V - E + F over unique positions, signed
    volume) of a triangle mesh with faces over `verts`"""
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    fwd = {}
    for a, b in d.tolist():
        fwd[(a, b)] = fwd.get((a, b), 0) + 1
    manifold = all(n == 1 and fwd.get((b, a), 0) == 1 for (a, b), n in fwd.items())
    euler = len(np.unique(faces)) - len(fwd) // 2 + len(faces)
    p = verts.astype(np.float64)
    vol = float(np.einsum("ij,ij->i", p[faces[:, 0]], np.cross(p[faces[:, 1]], p[faces[:, 2]])).sum() / 6)
    return manifold, euler, vol
