"""Plain numpy / Python restatement of the definitions of csrc/meshclean.hip (include/gsraster.h) and the
meshes of its tests.  Integer work only: every comparison with it is exact."""
import functools

import numpy as np


def components(faces, V):
    """-> (labels int32 [V]: the smallest vertex index of each vertex's component, tri_count int32 [V])"""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in faces.tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)  # (the root is then the minimum of its tree)
    labels = np.array([find(v) for v in range(V)], dtype=np.int32).reshape(V)
    tri_count = np.bincount(labels[faces[:, 0]], minlength=V).astype(np.int32) if len(faces) else np.zeros(V, np.int32)
    return labels, tri_count


def kept_labels(labels, tri_count, keep_largest, min_triangles):
    """-> bool [V]: True at the labels of the components the selection keeps"""
    roots = np.flatnonzero(labels == np.arange(len(labels)))  # increasing label
    order = roots[np.argsort(-tri_count[roots].astype(np.int64), kind="stable")]  # count descending, label ascending
    if keep_largest > 0:
        order = order[:keep_largest]
    keep = np.zeros(len(labels), bool)
    keep[order[tri_count[order] >= max(min_triangles, 1)]] = True
    return keep


def mesh_filter(vertices, faces, colors, keep_largest, min_triangles, comps=None):
    labels, tri_count = comps or components(faces, len(vertices))
    keep = kept_labels(labels, tri_count, keep_largest, min_triangles)
    vkeep = keep[labels]
    fkeep = vkeep[faces[:, 0]] if len(faces) else np.zeros(0, bool)
    remap = (np.cumsum(vkeep) - 1).astype(np.int32)
    return vertices[vkeep], remap[faces[fkeep]].reshape(-1, 3), None if colors is None else colors[vkeep]


def closure_labels(faces, V):
    """the labels by brute force: powers of the boolean adjacency matrix to the fixed point"""
    A = np.eye(V, dtype=bool)
    for j, k in ((0, 1), (1, 2), (2, 0)):
        A[faces[:, j], faces[:, k]] = A[faces[:, k], faces[:, j]] = True
    while True:
        B = (A.astype(np.float32) @ A.astype(np.float32)) > 0  # (sums of at most V ones: exact in fp32)
        if np.array_equal(A, B):
            return A.argmax(axis=1).astype(np.int32)
        A = B


def strip(n, first=0, step=1):
    """a triangle strip of n faces on the vertices first, first + step, ..."""
    t = np.arange(n, dtype=np.int32)[:, None]
    return first + step * (t + np.arange(3, dtype=np.int32)[None])


def islands(sizes, order=None):
    """strips of the given sizes on vertex blocks of their own; faces in the order given, vertex blocks in `order`"""
    order = list(range(len(sizes))) if order is None else order
    first, at = {}, 0
    for i in order:
        first[i], at = at, at + sizes[i] + 2
    return np.concatenate([strip(n, first[i]) for i, n in enumerate(sizes)]), at


def with_orphans(faces, V, gaps):
    """insert unused vertices: gaps = [(index before which they go, how many)], indices in the old numbering"""
    shift = np.zeros(V + 1, np.int32)
    for at, n in gaps:
        shift[at:] += n
    return (faces + shift[faces]).astype(np.int32), V + int(shift[V])


@functools.lru_cache(maxsize=None)
def cases(chunk, window):
    """name -> (faces int32 [F,3], V); chunk / window: the union kernel's faces per workgroup and LDS vertex window"""
    rng = np.random.default_rng(7)
    n = 3 * chunk + 37
    ordered = strip(n)
    perm = rng.permutation(n + 2).astype(np.int32)
    confetti, cv = islands([1 + (i % 97 == 5) + 2 * (i % 211 == 9) for i in range(1500)])
    ties, tv = islands([4, 7, 7, 7, 2], order=[3, 0, 4, 2, 1])
    m = 700
    inter = np.stack([strip(m, 0, 2), strip(m, 1, 2)], 1).reshape(-1, 3)
    # orphans: in front, in the middle of the first chunk's vertices (more than a window: that chunk has edges inside the
    # window, outside it and across its end) and at the end
    orphans, ov = with_orphans(ordered, n + 2, [(0, 3), (chunk // 2, window + 5), (n + 2, 4)])
    return {"strip_ordered": (ordered, n + 2), "strip_shuffled": (perm[ordered][rng.permutation(n)], n + 2),
            "confetti": (confetti, cv), "ties": (ties, tv), "interleaved": (inter, 2 * (m + 2)), "orphans": (orphans, ov)}
