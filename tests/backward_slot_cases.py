"""Cases for the slots of K10's walk (grendel-gs_amd/csrc/composite.hip), built with forward_slot_cases.kinds_case.

K10 compacts the entries of a 64-entry chunk that can touch a wave's 8 x 8 quadrant into pair records, back to front,
and walks them a pair at a time on a trip count: whether a pixel blended an entry is `position + 1 <= n_contrib` with the
position read from the record, an odd count leaves one inert record behind the last entry, every eight slots (and once
more for what is left) the (q, w) rows go through the matrix pipe, and the row of the result table an entry's sums go to
is its position word minus the chunk's first position.  What can go wrong there depends on HOW MANY entries of a chunk
are relevant in a quadrant and where they sit, so the lists are strings of forward_slot_cases' kinds (B, 0-3, F, Z, W).

The narrow splats keep to quadrant 0's corner, for the reason forward_slot_cases gives: K10's moment expansion about the
tile origin is itself at the tolerance off the other three corners.  A `0` splat is relevant in quadrant 0 alone, a `W`
or `B` in all four, so a chunk of n `0`, w `W` and fillers has n + w relevant entries in quadrant 0 and w in the others.

What the kernel counts in a (wave, chunk) is the relevant entries in front of the quadrant's deepest n_contrib (it loads
nothing behind that); `walked_counts` gives that number from the float64 decisions, and
tests/test_backward_slot_cases_cpu.py checks each case against the property it is named after."""
import functools

import torch

import composite_refs as R
import forward_slot_cases as S

COUNTS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64)


def _shuffled(seed, kinds):
    g = R._gen(seed)
    return "".join(kinds[int(i)] for i in torch.randperm(len(kinds), generator=g))


def walked_counts(case):
    """[chunks, 4] of the one-tile 16 x 16 case: relevant entries (float64: alpha >= 1/255 on a pixel of the quadrant) of
    each 64-entry chunk in front of the quadrant's deepest n_contrib -- what K10 compacts for that (wave, chunk)"""
    rel = S.quadrant_relevance(case)
    nc = R.references(case)[0]["n_contrib"].reshape(16, 16)
    L = rel.shape[0]
    out = torch.zeros((L + 63) // 64, 4, dtype=torch.int64)
    for q in range(4):
        wmax = int(nc[(q // 2) * 8:(q // 2) * 8 + 8, (q % 2) * 8:(q % 2) * 8 + 8].max())
        r = rel[:, q] & (torch.arange(L) < wmax)
        for ch in range(out.shape[0]):
            out[ch, q] = int(r[64 * ch:64 * ch + 64].sum())
    return out


def _case(name, kinds, seed, **kw):
    """kinds_case under a family of its own: the GPU tests cache uploads and root results by case id"""
    c = S.kinds_case(name, kinds, seed, **kw)
    c.family, c.id = "bwd-slots", f"bwd-slots-{name}"
    return c


def count_kinds(n):
    """one chunk with n relevant entries in quadrant 0: narrow splats up to 17, faint broad ones for 63 and 64 (64 narrow
    splats on one corner would saturate it after a few of them)"""
    return ("W" if n > 17 else "0") * n + "F" * (64 - n)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # relevant count of quadrant 0 in one chunk: odd (the inert slot), multiples of eight (the batch boundary), none
    for n in COUNTS:
        out.append(_case(f"count-{n}", _shuffled(500 + n, count_kinds(n)), 600 + n))
    # different counts in the quadrants of one chunk: the longest-walking wave and the table rows differ per wave
    out.append(_case("q0-64-others-9", _shuffled(41, "W" * 9 + "0" * 55), 641))
    out.append(_case("q0-24-others-7", _shuffled(42, "W" * 7 + "0" * 17 + "F" * 40), 642))
    # three chunks, the middle one all fillers for quadrants 1 to 3 (and walked: the third chunk blends everywhere)
    out.append(_case("middle-fillers", S._mix(43, 64, "W0F") + S._mix(44, 64, "0FF") + S._mix(45, 20, "WF") + "W", 643))
    # the pixel's last blended entry at chunk index 0, 63 and 64 (n_contrib 1, 64, 65)
    out.append(_case("last-0", "B" + "F" * 69, 644))
    out.append(_case("last-63", S._mix(46, 63, "0FF") + "B" + "F" * 6, 645))
    out.append(_case("last-64", S._mix(47, 64, "0FF") + "B" + "F" * 5, 646))
    # opacity exactly 0 among live ones
    out.append(_case("zero-opacity", "BZB0ZFB0BZFB0", 647))
    # every pixel takes every entry: every batch of all four waves is full (two chunks and two entries)
    out.append(_case("w-130", "W" * 130, 648))
    # a partial tile
    out.append(_case("13x13", S._mix(48, 40, "B0F"), 649, W=13, H=13))
    return tuple(out)
