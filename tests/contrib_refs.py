"""References for the per-Gaussian contribution statistics (grendel-gs_amd/csrc/contrib.hip) on the cases of
tests/composite_refs.py, unchanged.

Per local tile `composite_refs.decisions(case, dtype)` says which (entry, pixel) pairs are BLENDED (not skipped, in front
of the pixel's stop).  Here alpha and the transmittance are formed once more in the same arithmetic -- alpha =
min(0.99, o exp(min(power, 0))), T in front of an entry = the product of (1 - alpha) over the blended entries before it --
and w = alpha T on the blended pairs.  Per row: hits = the number of blended pairs, wmax = the largest w, wsum = the sum
of w, over all local tiles.  `references(case)` -> (float64 results, float32 results): the arbiter and the unit of
helpers.assert_rows_close (the reference's own fp32 error, never a kernel's)."""
import functools

import torch

import composite_refs as R

COLUMNS = ["wmax", "wsum"]


def _stats(case, dtype):
    m2, co = case.means2D.to(dtype), case.conic_opacity.to(dtype)
    hits = torch.zeros(case.P, dtype=torch.int64)
    wmax = torch.zeros(case.P, dtype=dtype)
    wsum = torch.zeros(case.P, dtype=dtype)
    for d in R.decisions(case, dtype):
        ids = d["ids"]
        x0, y0, x1, y1 = case.tile_box(d["tile"])
        py, px = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        pxf, pyf = px.reshape(-1).to(dtype), py.reshape(-1).to(dtype)
        xy, con = m2[ids], co[ids]
        dx, dy = xy[:, 0:1] - pxf[None, :], xy[:, 1:2] - pyf[None, :]
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        alpha = torch.clamp(con[:, 3:4] * torch.exp(torch.clamp(power, max=0.0)), max=0.99)
        blended = d["blended"]
        a_eff = torch.where(blended, alpha, torch.zeros_like(alpha))
        T_behind = torch.cumprod(1.0 - a_eff, dim=0)
        T_front = torch.cat([torch.ones_like(T_behind[:1]), T_behind[:-1]], dim=0)
        w = a_eff * T_front  # zero where the pair is not blended
        hits.index_add_(0, ids, blended.sum(dim=1))
        wmax[ids] = torch.maximum(wmax[ids], w.amax(dim=1))  # (ids are distinct within a tile)
        wsum.index_add_(0, ids, w.sum(dim=1))
    return dict(hits=hits, wmax=wmax.reshape(-1, 1), wsum=wsum.reshape(-1, 1))


@functools.lru_cache(maxsize=None)
def references(case):
    """-> (float64 results, float32 results): dict(hits int64 [P], wmax [P,1], wsum [P,1]); computed once per case and
    never modified"""
    return _stats(case, torch.float64), _stats(case, torch.float32)


def local_tiles(case):
    return int(case.compute_locally.sum())


def fp64_add_bound(case):
    """relative bound on a row's wsum between two orders of its fp64 additions: a launch adds at most one value per
    (local tile, quadrant) into a row, n = 4 x local tiles additions of non-negative numbers, each rounding 2^-53"""
    return 4 * local_tiles(case) * 2.0 ** -53
