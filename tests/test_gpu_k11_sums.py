"""K11 + Adam reading K10's fp64 sums and row flags (gsr_preprocess_backward_adam_raw_batched_sums) against the path it
replaces: gsr_render_record_materialize rounds the flagged rows into a zeroed fp32 record, then
gsr_preprocess_backward_adam_raw_batched reads that record through its row stride.  The inputs of one step are built
directly -- parameters, moments, radii / cov3D / clamped (K1 of a small scene, radii then edited), sums and flags -- so
every flag pattern is placed where a lane, a wave or a workgroup (K11_BLOCK = 128 rows) ends.  The record path is the
reference; it is held to float64 by tests/test_gpu_projection_rows.py and tests/test_gpu_adam_edges.py.

Sums of rows WITHOUT a flag hold NaN: the record path never reads them (their record rows are the cleared zeros), and a
sums kernel that did would poison the row.  All six parameters and twelve moments are compared with torch.equal (-0.0
and 0.0 compare equal: a visible row without a gradient takes the zero-gradient branch now, see include/gsraster.h)."""
import ctypes
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

W, H = 320, 208
NAMES = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")
LRS = [1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2]
B1S, B2S, EPSS = [0.9] * 6, [0.999] * 6, [1e-15] * 6
STEPS = [3, 4, 5, 6, 7, 9]
VP, D6, I64 = ctypes.c_void_p * 6, ctypes.c_double * 6, ctypes.c_int64 * 6
PATTERNS = ("none", "all", "block_edges", "between_culled", "visible_unflagged")


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def _p(t):
    return t.data_ptr() if t is not None else None


def _flags(pattern, P, radii):
    """-> flags [B,P] uint8 (host), radii [B,P] int32 (host, edited for the pattern)"""
    B = radii.shape[0]
    radii = radii.clone()
    fl = torch.zeros((B, P), dtype=torch.uint8)
    if pattern == "all":  # (rows behind the cameras keep their radius 0: a flag on a culled row changes nothing)
        fl[:] = 1
    elif pattern == "block_edges":  # first and last row of every workgroup's 128, and the last row there is
        for r in sorted({r for b in range(0, P, 128) for r in (b, min(b + 127, P - 1))}):
            fl[:, r] = 1
            radii[:, r] = torch.clamp(radii[:, r], min=3)
    elif pattern == "between_culled":  # a touched row whose neighbours are culled, in every camera
        for r in range(1, P, 5):
            fl[:, r] = 1
            radii[:, r] = torch.clamp(radii[:, r], min=3)
            radii[:, r - 1] = 0
            if r + 1 < P:
                radii[:, r + 1] = 0
    elif pattern == "visible_unflagged":  # every row visible, every third one touched -- in camera 0 only when B > 1
        radii[:] = torch.clamp(radii, min=2)
        fl[0, ::3] = 1
        if B > 1:
            fl[1, 1::3] = 1
    return fl, radii


class _Scene:
    """parameters, moments and K1's outputs of one (P, B) scene: built once, never changed (launches run on clones)"""

    def __init__(self, P, B, device):
        import diff_gaussian_rasterization as dgr
        import synthetic_scene as S
        from helpers import settings_from

        self.P, self.B, self.device = P, B, device
        m = S.SyntheticGaussianModel(max(P, 8), W, H, seed=3, device=device, scale_coef=0.02)
        self.params = [getattr(m, n).detach()[:P].clone().contiguous() for n in NAMES]
        with torch.no_grad():
            self.params[0][::7] = torch.tensor([-50.0, 0.0, -44.0], device=device)  # behind all cameras
        cams = S.orbit_cameras(8, W, H, device=device)[:B]
        rasts = [dgr.GaussianRasterizer(settings_from(c, torch.zeros(3), sh_degree=3)) for c in cams]
        self.packed = torch.stack([dgr.pack_camera(r.raster_settings) for r in rasts]).contiguous()
        self.tanfov = (ctypes.c_float * 2)(float(rasts[0].raster_settings.tanfovx),
                                           float(rasts[0].raster_settings.tanfovy))
        f32 = dict(dtype=torch.float32, device=device)
        m2, depths, co, rgb = (torch.empty(s, **f32) for s in ((B, P, 2), (B, P), (B, P, 4), (B, P, 3)))
        self.radii = torch.empty((B, P), dtype=torch.int32, device=device)
        self.cov3D = torch.empty((P, 6), **f32)
        self.clamped = torch.empty((B, P, 3), dtype=torch.uint8, device=device)
        p = self.params
        assert _lib().gsr_preprocess_forward_raw_batched(
            P, B, 3, 16, _p(p[0]), _p(p[1]), 1.0, _p(p[2]), _p(p[3]), _p(p[4]), _p(p[5]), _p(self.packed), W, H, _p(m2),
            _p(depths), _p(self.radii), _p(self.cov3D), _p(co), _p(rgb), _p(self.clamped), _stream()) == 0
        torch.cuda.synchronize()
        gen = torch.Generator().manual_seed(11 + P)
        # fp64 sums that no float holds exactly: the (float) conversion has to round, as the rounding launch does
        self.sums = torch.randn((B, P, 9), generator=gen, dtype=torch.float64) * (1.0 + 2.0 ** -30)
        self.ms = [(0.01 * torch.randn(t.shape, generator=gen)).to(device) for t in self.params]
        self.vs = [(a.cpu() ** 2 * (1.0 + torch.rand(a.shape, generator=gen)) + 1e-8).to(device) for a in self.ms]

    def tables(self, m, v):
        return [VP(*[_p(t) for t in m]), VP(*[_p(t) for t in v]), D6(*LRS), D6(*B1S), D6(*B2S), D6(*EPSS), I64(*STEPS),
                1.0 / self.B]

    def head(self, p, radii):
        return [self.P, self.B, 3, 16, _p(p[0]), _p(p[1]), 1.0, _p(p[2]), _p(p[3]), _p(p[4]), _p(p[5]), _p(self.packed),
                W, H, _p(radii), _p(self.cov3D), _p(self.clamped)]

    def run(self, pattern, sums_path, one_camera_kernel=True):
        """one step on clones -> (parameters, exp_avg, exp_avg_sq)"""
        lib, dev, P, B = _lib(), self.device, self.P, self.B
        fl_h, radii_h = _flags(pattern, P, self.radii.cpu())
        acc_h = torch.where(fl_h.bool().unsqueeze(-1), self.sums, torch.full_like(self.sums, float("nan")))
        accs = [acc_h[c].contiguous().to(dev) for c in range(B)]
        flags = [fl_h[c].contiguous().to(dev) for c in range(B)]
        radii = radii_h.to(dev)
        p, m, v = [t.clone() for t in self.params], [t.clone() for t in self.ms], [t.clone() for t in self.vs]
        tf = self.tanfov if (B == 1 and one_camera_kernel) else None
        if sums_path:
            PB = ctypes.c_void_p * B
            code = lib.gsr_preprocess_backward_adam_raw_batched_sums(
                *self.head(p, radii), PB(*[_p(a) for a in accs]), PB(*[_p(f) for f in flags]), *self.tables(m, v), tf,
                None, None, _stream())
        else:
            rec = torch.zeros((B, P, 9), dtype=torch.float32, device=dev)  # (what the forward's clear leaves)
            for c in range(B):
                assert lib.gsr_render_record_materialize(P, _p(accs[c]), _p(flags[c]), _p(rec[c]), 1, _stream()) == 0
            r2 = rec.view(B * P, 9)
            code = lib.gsr_preprocess_backward_adam_raw_batched(
                *self.head(p, radii), _p(r2[:, 0:2]), _p(r2[:, 5:9]), _p(r2[:, 2:5]), 9, *self.tables(m, v), tf,
                _stream())
        assert code == 0
        torch.cuda.synchronize()
        return p, m, v


@functools.lru_cache(maxsize=None)
def _scene(P, B, device):
    return _Scene(P, B, device)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("P", [1, 127, 128, 129, 257])
def test_sums_step_equals_the_record_step(device, P, B):
    sc = _scene(P, B, str(device))
    for pattern in PATTERNS:
        for one_camera_kernel in ((True, False) if B == 1 else (False,)):  # B == 1 through the batched kernel too
            want = sc.run(pattern, sums_path=False, one_camera_kernel=one_camera_kernel)
            got = sc.run(pattern, sums_path=True, one_camera_kernel=one_camera_kernel)
            for role, gs, ws in zip(("parameter", "exp_avg", "exp_avg_sq"), got, want):
                for n, a, b in zip(NAMES, gs, ws):
                    assert torch.equal(a, b), \
                        f"P {P} B {B} {pattern} one-camera {one_camera_kernel}: {role} {n}: " \
                        f"{int((a != b).sum())} of {a.numel()} values differ"
            if pattern == "all":  # the case is not vacuous: a flagged visible row moved, by a gradient that is not zero
                assert any(not torch.equal(a, b) for a, b in zip(got[1], sc.ms))


def test_materialize_writes_the_whole_record_when_it_was_not_cleared(device):
    P = 257
    gen = torch.Generator().manual_seed(4)
    acc = (torch.randn((P, 9), generator=gen, dtype=torch.float64) * (1.0 + 2.0 ** -30)).to(device)
    fl = (torch.rand(P, generator=gen) < 0.3).to(torch.uint8).to(device)
    want = torch.where(fl.bool().unsqueeze(-1), acc.float(), torch.zeros((), device=device))
    for cleared in (1, 0):
        rec = torch.zeros((P, 9), device=device) if cleared else torch.full((P, 9), float("nan"), device=device)
        assert _lib().gsr_render_record_materialize(P, _p(acc), _p(fl), _p(rec), cleared, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(rec, want)


def test_sums_entry_point_validates_before_any_launch(device):
    sc = _scene(129, 2, str(device))
    p, m, v = [t.clone() for t in sc.params], [t.clone() for t in sc.ms], [t.clone() for t in sc.vs]
    acc = torch.zeros((129, 9), dtype=torch.float64, device=device)
    fl = torch.zeros(129, dtype=torch.uint8, device=device)
    lib = _lib()

    def call(B, accs, flags):
        head = sc.head(p, sc.radii)
        head[1] = B
        PB = ctypes.c_void_p * len(accs)
        return lib.gsr_preprocess_backward_adam_raw_batched_sums(*head, PB(*accs), PB(*flags), *sc.tables(m, v), None,
                                                                 None, None, _stream())

    assert call(9, [_p(acc)] * 9, [_p(fl)] * 9) == -1          # more cameras than one launch takes
    assert call(2, [_p(acc), None], [_p(fl), _p(fl)]) == -1    # a null table entry
    assert call(2, [_p(acc), _p(acc) + 4], [_p(fl), _p(fl)]) == -1  # sums not 8-byte aligned
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(p + m + v, sc.params + sc.ms + sc.vs))
