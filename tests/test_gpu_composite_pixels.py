"""K8 / K10 through the C ABI on explicit lists: every pixel and every Gaussian row against the float64 reference.

gsr_render_forward / gsr_render_backward on the cases of tests/composite_refs.py -- the lists are given to the kernels, so
neither binning nor K1 stands between the inputs and the result, and every case keeps its inputs a margin away from the
blend's two discrete decisions.  `n_contrib` equals the float64 reference on every pixel; the image, final_T and the four
gradient groups (means2D, conic, opacity, rgb: separate tensors, their magnitudes differ by orders) go through
helpers.assert_rows_close (K = 8 for the image and final_T, composite_refs.K_GROUP for the gradient groups; per row: error <= K times the float32 reference's own worst per-row relative error,
times the row's largest value; zero rows exactly zero; a NaN fails; nothing excluded).  Outputs are pre-filled with NaN
(-7 for n_contrib), and so are the fp64 sums and the record where the call clears them itself.

The root form (no segments, whole grid, full rounding pass) runs every case; the segment workspace, the host and device
row bands and the flagged rounding pass run the `deep`, `edges` and `inert` families: the forward bit-equal to the root,
the backward against the same float64 rule (with segments it starts from checkpoints and is not bit-equal by design).

Each figure (unit in 2^-24, worst ratio) is printed before it is asserted: EXPERIMENTS.md, 'Composite pixels and rows
against float64', has the table measured on the MI355X."""
import pytest
import torch

import composite_refs as R
from helpers import assert_rows_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K = R.K_FORWARD
NAN = float("nan")
GSR_EINVAL, GSR_ENOSPACE = -1, -2


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def _p(t):
    return t.data_ptr() if t is not None and t.numel() else None


class _Dev:
    """the case's inputs on the device (uploaded once per case, never written)"""

    def __init__(self, case, device):
        self.case = case
        self.means2D, self.co, self.rgb = (t.to(device).contiguous() for t in (case.means2D, case.conic_opacity, case.rgb))
        self.bg = case.bg.to(device)
        self.mask = case.compute_locally.to(torch.uint8).to(device)
        self.ranges = case.ranges.to(torch.int32).to(device).contiguous()
        self.point_list = case.point_list.to(torch.int32).to(device).contiguous()  # (ids < 2^31: the bits of uint32)
        self.g = case.dL_dpixels.to(device).contiguous()
        self.device = device


_DEV = {}


def _dev(case, device):
    if case.id not in _DEV:
        _DEV[case.id] = _Dev(case, device)
    return _DEV[case.id]


def _seg_ws(case, device):
    n = int(_lib().gsr_render_seg_bytes(case.W, case.H))
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=device), n


def _forward(d, seg=None, band=(0, 0), zero=None):
    """K8 into NaN / -7 filled outputs -> (code, image [3,H,W], final_T [H,W], n_contrib [H,W]) on the device"""
    c = d.case
    img = torch.full((3, c.H, c.W), NAN, dtype=torch.float32, device=d.device)
    fT = torch.full((c.H, c.W), NAN, dtype=torch.float32, device=d.device)
    nc = torch.full((c.H, c.W), -7, dtype=torch.int32, device=d.device)
    ws, ws_bytes = seg if seg is not None else (None, 0)
    code = _lib().gsr_render_forward(c.P, c.W, c.H, _p(d.ranges), _p(d.point_list), _p(d.means2D), _p(d.co), _p(d.rgb),
                                     _p(d.mask), _p(d.bg), _p(img), _p(fT), _p(nc), _p(ws), ws_bytes, band[0], band[1],
                                     _p(zero), zero.numel() if zero is not None else 0, _stream())
    torch.cuda.synchronize()
    return code, img, fT, nc


def _backward(d, fwd, seg=None, band=(0, 0), flagged=None):
    """K10 on the forward's own final_T / n_contrib -> (code, record [P,9], touched or None).  Full pass: NaN-filled record
    and sums, record_is_zero = 0.  flagged = the [72 P | 36 P | P padded to 16] buffer the forward cleared."""
    c = d.case
    _, img, fT, nc = fwd
    n = max(c.P, 1)
    if flagged is None:
        rec = torch.full((n, 9), NAN, dtype=torch.float32, device=d.device)
        acc = torch.full((n, 9), NAN, dtype=torch.float64, device=d.device)
        touched, riz = None, 0
    else:
        acc = flagged[:72 * c.P].view(torch.float64).view(c.P, 9)
        rec = flagged[72 * c.P:108 * c.P].view(torch.float32).view(c.P, 9)
        touched, riz = flagged[108 * c.P:], 1
    ws, ws_bytes = seg if seg is not None else (None, 0)
    code = _lib().gsr_render_backward(c.P, c.W, c.H, _p(d.ranges), _p(d.point_list), _p(d.means2D), _p(d.co), _p(d.rgb),
                                      _p(d.mask), _p(d.bg), _p(fT), _p(nc), _p(d.g), _p(rec), _p(img) if seg is not None else None,
                                      _p(ws), ws_bytes, band[0], band[1], riz, _p(acc), _p(touched), _stream())
    torch.cuda.synchronize()
    return code, rec, touched


_ROOT = {}


def _root(case, device):
    """the root form of one case: (forward tuple, record) -- computed once per case and never modified"""
    if case.id not in _ROOT:
        d = _dev(case, device)
        fwd = _forward(d)
        assert fwd[0] == 0, f"gsr_render_forward returned {fwd[0]}"
        code, rec, _ = _backward(d, fwd)
        assert code == 0, f"gsr_render_backward returned {code}"
        _ROOT[case.id] = (fwd, rec)
    return _ROOT[case.id]


def _check_forward(case, fwd, what):
    """n_contrib on every pixel, image and final_T by the row rule, pixels of tiles that are not ours exactly 0 / 1 / 0
    -> {tensor: (unit, worst ratio)}"""
    r64, r32 = R.references(case)
    _, img, fT, nc = fwd
    img, fT, nc = img.cpu(), fT.cpu(), nc.cpu()
    assert torch.equal(nc, r64["n_contrib"]), \
        f"{what}: n_contrib differs on pixels (y, x) {torch.nonzero(nc != r64['n_contrib'])[:8].tolist()}"
    for t in range(case.tiles):
        if not bool(case.compute_locally[t]):
            x0, y0, x1, y1 = case.tile_box(t)
            assert not bool(img[:, y0:y1, x0:x1].view(torch.int32).any()), f"{what}: image of tile {t} (not ours) is not +0"
            assert bool((fT[y0:y1, x0:x1] == 1).all()) and not bool(nc[y0:y1, x0:x1].any()), f"{what}: tile {t} (not ours)"
    irows, trows = R.as_rows(img, fT)
    return dict(image=assert_rows_close(irows, r64["image"], r32["image"], K, f"{what} image"),
                final_T=assert_rows_close(trows, r64["final_T"], r32["final_T"], K, f"{what} final_T"))


def _check_record(case, rec, what):
    """the four gradient groups of a [P,9] record by the row rule -> {group: (unit, worst ratio)}"""
    r64, r32 = R.references(case)
    got = R.split_record(rec.cpu()[:case.P])
    return {k: assert_rows_close(got[k], r64[k], r32[k], R.K_GROUP[k], f"{what} {k}") for k in R.GROUPS}


def _print(tag, case, figures):
    for k, (unit, worst) in figures.items():
        print(f"PIXELS {tag} {case.id} {k}: unit {unit / U:.0f} x 2^-24, worst ratio {worst:.3g}")


# ------------------------------------------------------------------------------------------------ 1. the root form
@pytest.mark.parametrize("case", R.cases(), ids=[c.id for c in R.cases()])
def test_root_form_every_pixel_and_row_against_float64(device, case):
    fwd, rec = _root(case, device)
    fig = _check_forward(case, fwd, case.id)
    if case.P > 0:
        fig.update(_check_record(case, rec, case.id))
    else:  # P = 0: success, and not one word written
        assert bool(torch.isnan(rec).all()), "gsr_render_backward with P = 0 wrote into the record"
    _print("root", case, fig)


# ------------------------------------------------------------------------------------------------ 2. the variants
VARIANTS = [c for c in R.cases() if c.family in R.VARIANT_FAMILIES]
BANDED = [c for c in VARIANTS if c.band is not None]
assert BANDED, "no case with a proper row band"


def _assert_forward_bits(fwd, root, what):
    for a, b, name in zip(fwd[1:], root[1:], ("image", "final_T", "n_contrib")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: {name} is not bit-equal to the root form"


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
def test_segment_workspace(device, case):
    """forward with the workspace: bit-equal to the root; backward from the checkpoints: the float64 rule -- `deep-long`
    walks 17 boundaries, one more than may carry a checkpoint"""
    root, _ = _root(case, device)
    d = _dev(case, device)
    seg = _seg_ws(case, device)
    fwd = _forward(d, seg=seg)
    assert fwd[0] == 0
    _assert_forward_bits(fwd, root, f"{case.id} segments")
    if case.P == 0:
        return
    code, rec, _ = _backward(d, fwd, seg=seg)
    assert code == 0
    fig = _check_record(case, rec, f"{case.id} segments")
    _print("segments", case, fig)
    queued = int(seg[0][:4].view(torch.int32).item())
    want = sum(min(b, R.SEG_MAXJ) for b in R.boundaries_walked(case).values())
    assert queued == want, f"K8 queued {queued} segments, the float64 reference's walk crosses {want} boundaries"


@pytest.mark.parametrize("case", BANDED, ids=[c.id for c in BANDED])
@pytest.mark.parametrize("kind", ["host", "device", "device-larger"])
def test_row_bands(device, case, kind):
    """the launch covers the band's tiles only (host rows; or row_lo = -1 with a capacity, the band read from the hull
    behind the range table): forward bit-equal to the root, backward by the float64 rule"""
    root, _ = _root(case, device)
    d = _dev(case, device)
    lo, hi = case.band
    assert (lo, hi) == case.hull and 0 < hi - lo < case.gy
    band = (lo, hi) if kind == "host" else (-1, hi - lo if kind == "device" else case.gy)
    fwd = _forward(d, band=band)
    assert fwd[0] == 0
    _assert_forward_bits(fwd, root, f"{case.id} band {kind}")
    code, rec, _ = _backward(d, fwd, band=band)
    assert code == 0
    fig = _check_record(case, rec, f"{case.id} band {kind}")
    _print(f"band-{kind}", case, fig)


FLAGGED = [c for c in VARIANTS if c.family in ("inert", "edges") and c.P > 0]


@pytest.mark.parametrize("case", FLAGGED, ids=[c.id for c in FLAGGED])
def test_flagged_rounding(device, case):
    """the forward clears [72 P | 36 P | P padded to 16] bytes, the backward rounds the rows K10 flagged: the record is
    bit-equal to the root's, and `touched` is 1 exactly on the rows whose float64 reference row is non-zero"""
    root, root_rec = _root(case, device)
    d = _dev(case, device)
    P = case.P
    buf = torch.full((108 * P + ((P + 15) & ~15),), 0xFF, dtype=torch.uint8, device=device)
    fwd = _forward(d, zero=buf)
    assert fwd[0] == 0
    _assert_forward_bits(fwd, root, f"{case.id} flagged")
    assert not bool(buf.any()), "the forward did not clear the whole range"
    code, rec, touched = _backward(d, fwd, flagged=buf)
    assert code == 0
    assert torch.equal(rec.view(torch.int32), root_rec.view(torch.int32)), "record differs from the full rounding pass"
    r64, _ = R.references(case)
    live = torch.cat([r64[k] != 0 for k in R.GROUPS], dim=1).any(dim=1)
    assert torch.equal(touched[:P].cpu(), live.to(torch.uint8)), \
        f"touched differs on rows {torch.nonzero(touched[:P].cpu() != live.to(torch.uint8)).reshape(-1)[:8].tolist()}"
    assert not bool(touched[P:].any())


def test_too_small_segment_workspace_is_refused(device):
    case = R.family("edges")[2]
    root, _ = _root(case, device)
    d = _dev(case, device)
    ws, n = _seg_ws(case, device)
    fwd = _forward(d, seg=(ws, n - 1))
    assert fwd[0] == GSR_ENOSPACE
    assert bool(torch.isnan(fwd[1]).all()) and bool(torch.isnan(fwd[2]).all()) and bool((fwd[3] == -7).all())
    assert bool((ws == 0xA5).all()), "the refused forward wrote into the workspace"
    code, rec, _ = _backward(d, root, seg=(ws, n - 1))
    assert code == GSR_EINVAL and bool(torch.isnan(rec).all())
