"""CPU checks of tests/surfel_refs.py, the arbiter of the surfel geometry pass: the vectorised reference against one
brute-force loop per pixel on two cases, and the cap on NEAR pixels (surfel_refs' docstring) on every case used."""
import pytest
import torch

import surfel_refs as SR

R = SR.R
CASES = SR.cases()


def _brute(case):
    """per pixel, entry by entry in float64: the maps by their definitions (the distortion as the double sum over pairs),
    the median by the header's rule, and the parts of dL/drows that are linear in w"""
    dt = torch.float64
    rows, g_s, g_dist, g_med = (t.to(dt) for t in SR.draw(case))
    m2, co = case.means2D.to(dt), case.conic_opacity.to(dt)
    nc = R.references(case)[0]["n_contrib"]
    maps = torch.zeros(9, case.H, case.W, dtype=dt)
    medpos = torch.zeros(case.H, case.W, dtype=torch.int32)
    d_n, d_z_lin = torch.zeros(case.P, 3, dtype=dt), torch.zeros(case.P, dtype=dt)
    for t in range(case.tiles):
        if not bool(case.compute_locally[t]):
            continue
        x0, y0, x1, y1 = case.tile_box(t)
        for y in range(y0, y1):
            for x in range(x0, x1):
                T, ws, zs, chosen = 1.0, [], [], -1
                for k, i in enumerate(case.lists[t].tolist()):
                    dx, dy = float(m2[i, 0]) - x, float(m2[i, 1]) - y
                    power = -0.5 * (float(co[i, 0]) * dx * dx + float(co[i, 2]) * dy * dy) - float(co[i, 1]) * dx * dy
                    alpha = min(0.99, float(co[i, 3] * torch.exp(torch.tensor(min(power, 0.0), dtype=dt))))
                    if not (k + 1 <= int(nc[y, x]) and power <= 0 and alpha >= R.ALPHA_MIN):
                        continue
                    if T > 0.5:
                        chosen = i
                        medpos[y, x] = k + 1
                    w = alpha * T
                    T -= w
                    ws.append(w)
                    zs.append(float(rows[i, 1]))
                    maps[0, y, x] += w
                    maps[1:5, y, x] += w * rows[i, 1:5]
                    d_n[i] += w * g_s[2:5, y, x]
                    d_z_lin[i] += w * g_s[1, y, x]
                maps[5, y, x] = sum(ws[a] * ws[b] * (zs[a] - zs[b]) ** 2 for a in range(len(ws)) for b in range(a))
                if chosen >= 0:
                    maps[8, y, x] = rows[chosen, 1]
                    d_z_lin[chosen] += g_med[y, x]
    return maps, medpos, d_n, d_z_lin


@pytest.mark.parametrize("cid", ["lengths-9", "edges-17x17"])
def test_reference_against_a_brute_force_loop(cid):
    case = next(c for c in CASES if c.id == cid)
    r64 = SR.references(case)[0]  # mapping "depth": m = z
    maps, medpos, d_n, d_z_lin = _brute(case)
    for i, k in ((0, "A"), (1, "D"), (2, "N0"), (3, "N1"), (4, "N2"), (5, "Dist"), (8, "med")):
        torch.testing.assert_close(r64[k].reshape(-1), maps[i].reshape(-1), rtol=1e-12, atol=1e-14, msg=f"{cid} {k}")
    assert torch.equal(r64["median_pos"], medpos.reshape(-1))
    torch.testing.assert_close(r64["d_n"], d_n, rtol=1e-12, atol=1e-14)
    # dL/dz with the distortion's upstream map taken out: the reference's d_z minus distortion_refs' own d_depth
    d_dist = SR.DR.references(case)[0]["d_depth"].reshape(-1)
    torch.testing.assert_close(r64["d_z"].reshape(-1) - d_dist, d_z_lin, rtol=1e-9, atol=1e-12)


def test_the_cap_on_near_pixels_and_the_median_edges():
    for case in CASES:
        frac = SR.near_fraction(case)
        print(f"SURFELS near {case.id}: {100 * frac:.2f} %")
        # OVER_CAP names exactly the cases over the cap; the cap is never raised
        assert (frac > SR.NEAR_CAP) == (case.id in SR.OVER_CAP), f"{case.id}: {100 * frac:.2f} % near"
    pos = {c.name: SR.references(c)[0]["median_pos"] for c in CASES if c.family == "median"}
    nct = {c.name: SR.references(c)[0]["n_contrib"].reshape(-1) for c in CASES if c.family == "median"}
    assert bool((pos["first"] == 1).all()) and bool((pos["open"] == nct["open"]).all()) and bool((pos["open"] > 0).all())
    assert bool((pos["cross-64"] == 64).all()) and bool((pos["cross-65"] == 65).all())
