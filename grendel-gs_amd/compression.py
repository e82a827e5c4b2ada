"""Codebook compression of a trained model: k-means over the rows of a parameter (by default the 45 SH coefficients above
DC, 76 % of a row's bytes), a 16-bit index per row, the codebook in fp32 -- the vector quantisation of Compact3D,
LightGaussian and "Compressed 3D Gaussian Splatting".  The reference has no compression: nothing here mirrors a reference
call site.

The Lloyd iterations run on the HIP kernels of vq.hip (`vq_assign` on the fp32 matrix pipe, `vq_update` with fixed-order
fp64 sums), so the same seed gives the same bits.  A fine-tune of the codebook needs only `vq_decode`, whose gradient with
respect to the codebook is the per-cluster sum of the row gradients.  With more than one rank every rank compresses its
own shard with its own codebook; nothing is communicated.
"""
import numpy as np
import torch

from diff_gaussian_rasterization import vq_assign, vq_decode, vq_update

_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
         "scaling": "_scaling", "rotation": "_rotation"}
MAX_D, MAX_K = 64, 65536


def kmeans(rows, K, iters=10, seed=0, weights=None):
    """Lloyd's algorithm on rows fp32 [P,D] (device): returns (codebook fp32 [K',D], idx int32 [P]), K' = min(K, P).
    Initial centroids: K' distinct rows from a seeded host permutation.  After every update the empty clusters are moved
    onto the rows farthest from their centroid, in the order (dist2 descending, row index ascending).  `weights` [P]
    enters the update only.  The returned idx is the assignment to the returned codebook."""
    P = rows.shape[0]
    K = min(K, P)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))[:K]
    codebook = rows[perm.to(rows.device)].clone()
    for _ in range(iters):
        idx, dist = vq_assign(rows, codebook, return_dist=True)
        count, _ = vq_update(rows, idx, codebook, weights)
        empty = (count == 0).nonzero().flatten()
        n = empty.numel()
        if n:
            # at most K candidates unless distances tie at the threshold; a stable sort keeps row order inside a tie
            cand = (dist >= torch.topk(dist, n).values[-1]).nonzero().flatten()
            far = cand[torch.sort(dist[cand], descending=True, stable=True).indices[:n]]
            codebook[empty[:far.numel()]] = rows[far]
    return codebook, vq_assign(rows, codebook)


class CompressedModel:
    """per compressed group the codebook (fp32 [K,D]) and the indices (int32 [P] on the device, uint16 on disk), the
    other parameters as they are"""

    def __init__(self, groups, raw):
        self.groups = groups  # name -> (codebook, idx, shape of the parameter)
        self.raw = raw        # name -> tensor

    def nbytes(self):
        """(bytes of the fp32 parameters, bytes of this representation with 16-bit indices)"""
        raw = sum(t.numel() * t.element_size() for t in self.raw.values())
        before = raw + sum(4 * int(np.prod(shape)) for _, _, shape in self.groups.values())
        after = raw + sum(4 * cb.numel() + 2 * idx.numel() for cb, idx, _ in self.groups.values())
        return before, after

    def apply(self, pc):
        """decode into the EXISTING parameter storage of `pc` (the pointers an optimizer or a captured graph holds stay
        valid)"""
        with torch.no_grad():
            for name, (cb, idx, shape) in self.groups.items():
                p = getattr(pc, _ATTR[name])
                if tuple(p.shape) != tuple(shape):
                    raise ValueError(f"{name}: the model holds {tuple(p.shape)}, the compressed group {tuple(shape)}")
                p.view(idx.shape[0], -1).copy_(vq_decode(cb.to(p.device), idx.to(p.device)))
            for name, t in self.raw.items():
                getattr(pc, _ATTR[name]).copy_(t)
        return pc

    def save(self, path):
        arrays = {}
        for name, (cb, idx, shape) in self.groups.items():
            arrays["codebook." + name] = cb.cpu().numpy()
            arrays["index." + name] = idx.cpu().numpy().astype(np.uint16)  # K <= 65536
            arrays["shape." + name] = np.asarray(shape, dtype=np.int64)
        for name, t in self.raw.items():
            arrays["raw." + name] = t.cpu().numpy()
        with open(path, "wb") as f:
            np.savez_compressed(f, **arrays)

    @classmethod
    def load(cls, path, device="cuda"):
        groups, raw = {}, {}
        with np.load(path) as z:
            for key in z.files:
                kind, name = key.split(".", 1)
                if kind == "raw":
                    raw[name] = torch.from_numpy(z[key]).to(device)
                elif kind == "codebook":
                    groups[name] = (torch.from_numpy(z[key]).to(device),
                                    torch.from_numpy(z["index." + name].astype(np.int32)).to(device),
                                    tuple(int(v) for v in z["shape." + name]))
        return cls(groups, raw)


def compress(pc, groups=None, iters=10, seed=0, weights=None):
    """Quantise the named parameter groups of `pc` (a GaussianModel: _xyz, _features_dc, _features_rest, _opacity,
    _scaling, _rotation) -> CompressedModel.  groups: name -> K, names as the optimizer's ("f_rest", "f_dc", ...); each
    parameter is flattened to [P,D]; D > 64 raises, a group with D == 0 (SH degree 0) is skipped, K is capped at 65536
    by the 16-bit index and at P.  weights: optional importance fp32 [P] (the contribution statistics of
    `score_contributions` are the intended source).  `pc` itself is not changed: see CompressedModel.apply."""
    groups = {"f_rest": 4096} if groups is None else dict(groups)
    for name, K in groups.items():
        if name not in _ATTR:
            raise ValueError(f"unknown parameter group {name!r}; one of {sorted(_ATTR)}")
        if not (1 <= K <= MAX_K):
            raise ValueError(f"{name}: 1 <= K <= {MAX_K}, got {K}")
    done, raw = {}, {}
    for name, attr in _ATTR.items():
        p = getattr(pc, attr, None)
        if p is None:
            continue
        p = p.detach()
        D = p[0].numel() if p.shape[0] else 0
        if name in groups and D > MAX_D:
            raise ValueError(f"{name}: rows of {D} values, at most {MAX_D} can share a codebook")
        if name in groups and D > 0:
            cb, idx = kmeans(p.reshape(p.shape[0], D).float().contiguous(), groups[name], iters, seed, weights)
            done[name] = (cb, idx, tuple(p.shape))
        else:
            raw[name] = p.clone()
    return CompressedModel(done, raw)
