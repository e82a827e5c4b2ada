"""Cases for the slots of K8's walk (grendel-gs_amd/csrc/composite.hip), built with the generators of composite_refs.

K8 compacts the entries of a 64-entry chunk that can touch a wave's 8 x 8 quadrant into pair records and walks them four
slots at a time; the value n_contrib takes comes from the record (the entry's list position + 1), and the up-to-three
slots behind the last entry of a chunk are inert records.  What can go wrong there depends on WHERE in a chunk the
relevant entries sit, not on how they blend, so every list here is a string of kinds, one per list position:

    B   a broad soft splat just outside the tile (composite_refs.lengths_case's: relevant in every quadrant)
    0-3 a small splat off the corner of that quadrant: relevant there, irrelevant in the opposite quadrant
    F   a filler 150 px and more away: relevant nowhere
    Z   a broad splat with opacity exactly 0
    W   a very broad, faint splat (composite_refs.deep_case's: alpha of about 0.006 to 0.02 on EVERY pixel of the tile)

Only quadrant 0's corner is used in `cases()`.  K10 rebuilds sum q dx^2 from raw moments about the TILE origin
(ex^2 M0 - 2 ex Ax + Axx), which for a narrow splat off one of the other three corners is a small difference of terms
(ex / dx)^2 times larger: the CPU emulation of K10's order of operations (composite_refs.k10_emulation, library exp2 and
a correctly rounded division) is itself at 12 to 16 units on d_conic there, against K = 12.  That is a property of the
backward's formulation, not of the forward's slots; off the origin corner ex and the pixel offsets add up and the
emulation stays below K / 2, which tests/test_forward_slot_cases_cpu.py asserts.  For a wave a splat that is relevant
in another quadrant only is the same thing as a filler.

`cases()` is a fixed tuple; tests/test_forward_slot_cases_cpu.py checks on the CPU that each case has the property it
is named after and keeps the conditions composite_refs asks of a case."""
import functools
import math

import torch

import composite_refs as R


def kinds_case(name, kinds, seed, W=16, H=16):
    """one 16 x 16 tile whose list is `kinds`; three rows more than the list holds stay out of it"""
    gen = R._gen(seed)
    L = len(kinds)
    P = L + 3
    nb = sum(k in "BZ" for k in kinds)
    amax = min(0.3, 4.0 / max(nb, 1))  # sum of alpha of the broad ones <= 4
    m, c, o, rgb = R._soft(gen, P, (2.0, 2.0), (8.0, 8.0), (8.0, 16.0), (0.25 * amax, amax))
    m = R._outside(gen, m)
    ids = torch.randperm(P, generator=gen)[:L]
    for pos, k in enumerate(kinds):
        i = int(ids[pos])
        if k in "0123":
            q = int(k)
            d = R._u(gen, 2, 1.5, 3.0)
            m[i, 0] = -d[0] if q % 2 == 0 else 16.0 + d[0]
            m[i, 1] = -d[1] if q // 2 == 0 else 16.0 + d[1]
            s = R._u(gen, 2, 2.0, 2.6)
            c[i] = R.conics(s[0:1], s[1:2], R._u(gen, 1, 0.0, math.pi))[0]
            o[i] = R._u(gen, 1, 0.3, 0.6)[0]
        elif k == "F":
            m[i] = m[i] + 150.0 + R._u(gen, 1, 0.0, 50.0)[0]
            s = R._u(gen, 2, 2.0, 4.0)
            c[i] = R.conics(s[0:1], s[1:2], R._u(gen, 1, 0.0, math.pi))[0]
            o[i] = R._u(gen, 1, 0.3, 0.9)[0]
        elif k == "Z":
            o[i] = 0.0
        elif k == "W":
            s = R._u(gen, 2, 40.0, 90.0)
            c[i] = R.conics(s[0:1], s[1:2], R._u(gen, 1, 0.0, math.pi))[0]
            o[i] = R._u(gen, 1, 0.0075, 0.02)[0]
    live = ids[torch.tensor([k != "F" for k in kinds], dtype=torch.bool)] if L else ids
    rgb = R._falling_colours(gen, rgb, live)
    return R.Case("slots", name, W, H, m, c, o, rgb, [0.0, 0.0, 0.0], [True], [ids], seed)


def _mix(seed, n, alphabet):
    g = R._gen(seed)
    return "".join(alphabet[int(i)] for i in torch.randint(0, len(alphabet), (n,), generator=g))


def quadrant_relevance(case):
    """[L, 4] bool of the one-tile case: the entry reaches alpha >= 1/255 on a pixel of quadrant q (float64; a subset of the
    kernel's box test, which may also keep an entry that touches the box between pixel centres)"""
    d = R.decisions(case)[0]
    a = (d["r_a"] >= 1.0).reshape(d["L"], 16, 16)
    return torch.stack([a[:, (q // 2) * 8:(q // 2) * 8 + 8, (q % 2) * 8:(q % 2) * 8 + 8].reshape(d["L"], -1).any(dim=1)
                        for q in range(4)], dim=1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # relevant and irrelevant entries interleave: a slot's compacted position differs from its chunk index
    out.append(kinds_case("interleave-64", _mix(1, 64, "B0F"), 301))
    out.append(kinds_case("interleave-100", _mix(2, 100, "BB0F"), 302))
    # the last blended entry at chunk index 0, 63 and 64 (n_contrib 1, 64, 65)
    out.append(kinds_case("last-0", "B" + "F" * 69, 303))
    out.append(kinds_case("last-63", _mix(3, 63, "0FF") + "B" + "F" * 6, 304))
    out.append(kinds_case("last-64", _mix(4, 64, "0FF") + "B" + "F" * 5, 305))
    # 1, 2, 3 relevant entries in the last group of a chunk (5, 6, 7 of 64), the chunk behind it full -- and the other way
    # round, where the inert slots of the second chunk lie on records the full one left in the slab
    for r in (1, 2, 3):
        g = R._gen(310 + r)
        first = ["F"] * 64
        for p in torch.randperm(64, generator=g)[:4 + r].tolist():
            first[p] = "W"
        out.append(kinds_case(f"res{r}-then-full", "".join(first) + "W" * 64, 320 + r))
        out.append(kinds_case(f"full-then-res{r}", "W" * 64 + "".join(first), 330 + r))
    # opacity exactly 0 among live ones
    out.append(kinds_case("zero-opacity", "BZB0ZFB0BZFB0", 340))
    # partial tiles
    out.append(R.edges_case("20x20", 20, 20, [True] * 4, 350))
    return tuple(out)
