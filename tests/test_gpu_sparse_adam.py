"""Sparse (lazy) Adam: gsr_preprocess_backward_adam_raw_batched_sparse and FusedAdam(fuse_backward=True, sparse=True).

The expected values never come from the code under test: `active` is computed in torch (on the host: no flushing of
denormals) from radii and the gradient tensors by the definition of include/gsraster.h, the dense result of a step by the
parent's unfused pair on clones -- gsr_preprocess_backward_raw_batched, then gsr_adam_step_multi -- and
expected = where(active, dense, before).  Scenes: 320 x 208, every 7th row behind all cameras, the nine gradient words
of every row with i % 3 == 1 zeroed for all cameras."""
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
GSR_EINVAL, GSR_ENOSPACE = -1, -2
NAMES = ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity")
LRS = [1.6e-4, 5e-3, 1e-3, 2.5e-3, 1.25e-4, 5e-2]
B1S, B2S, EPSS = [0.9] * 6, [0.999] * 6, [1e-15] * 6
STEPS = [3, 4, 5, 6, 7, 9]  # the 1-based counts AFTER the update: every case starts from step counts > 1
VP, D6, I64 = ctypes.c_void_p * 6, ctypes.c_double * 6, ctypes.c_int64 * 6


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def _p(t):
    return t.data_ptr() if t is not None else None


def _packed_cams(B, deg, device):
    import diff_gaussian_rasterization as dgr
    import synthetic_scene as S
    from helpers import settings_from

    cams = S.orbit_cameras(8, W, H, device=device)[:B]
    rasts = [dgr.GaussianRasterizer(settings_from(c, torch.zeros(3), sh_degree=deg)) for c in cams]
    return torch.stack([dgr.pack_camera(r.raster_settings) for r in rasts]).contiguous()


def _forward(params, packed, deg):
    """K1 of the batch through the C ABI -> radii [B,N] int32, cov3D [N,6], clamped [B,N,3] uint8"""
    N, B, dev = params[0].shape[0], packed.shape[0], params[0].device
    f32 = dict(dtype=torch.float32, device=dev)
    m2, depths, co, rgb = (torch.empty(s, **f32) for s in ((B, N, 2), (B, N), (B, N, 4), (B, N, 3)))
    radii = torch.empty((B, N), dtype=torch.int32, device=dev)
    cov3D = torch.empty((N, 6), **f32)
    clamped = torch.empty((B, N, 3), dtype=torch.uint8, device=dev)
    assert _lib().gsr_preprocess_forward_raw_batched(
        N, B, deg, 16, *[_p(t) for t in params[:2]], 1.0, *[_p(t) for t in params[2:]], _p(packed), W, H, _p(m2),
        _p(depths), _p(radii), _p(cov3D), _p(co), _p(rgb), _p(clamped), _stream()) == 0
    return radii, cov3D, clamped


def _active(radii, g2, grgb, gco):
    """the definition, in torch on the host: some camera sees the row and one of its nine words compares != 0"""
    B, N = radii.shape
    nz = (g2.cpu().reshape(B, N, 2) != 0).any(-1) | (grgb.cpu().reshape(B, N, 3) != 0).any(-1) | \
        (gco.cpu().reshape(B, N, 4) != 0).any(-1)
    return ((radii.cpu() > 0) & nz).any(0)


def _k11(params, packed, deg, radii, cov3D, clamped, g2, grgb, gco, gstride):
    """the parent's unfused camera-batched K11 (at every B, 1 included) -> the six gradients"""
    N, B = params[0].shape[0], packed.shape[0]
    p = params
    grads = [torch.full_like(t, float("nan")) for t in p]
    assert _lib().gsr_preprocess_backward_raw_batched(
        N, B, deg, 16, _p(p[0]), _p(p[1]), 1.0, _p(p[2]), _p(p[3]), _p(p[4]), _p(p[5]), _p(packed), W, H, _p(radii),
        _p(cov3D), _p(clamped), _p(g2), _p(gco), _p(grgb), gstride, *[_p(g) for g in grads], _stream()) == 0
    return grads


def _adam(params, grads, ms, vs, lrs, steps, grad_scale):
    """gsr_adam_step_multi on clones -> (parameters, exp_avg, exp_avg_sq) x 6"""
    p, m, v = [t.clone() for t in params], [t.clone() for t in ms], [t.clone() for t in vs]
    assert _lib().gsr_adam_step_multi(6, I64(*[t.numel() for t in p]), VP(*[_p(t) for t in p]),
                                      VP(*[_p(t) for t in grads]), VP(*[_p(t) for t in m]), VP(*[_p(t) for t in v]),
                                      D6(*lrs), D6(*B1S), D6(*B2S), D6(*EPSS), I64(*steps), grad_scale, _stream()) == 0
    return p, m, v


def _dense_pair(params, ms, vs, packed, deg, radii, cov3D, clamped, g2, grgb, gco, gstride, lrs, steps, grad_scale):
    """the parent's unfused pair on clones -> (parameters, exp_avg, exp_avg_sq) x 6, and K11's six gradients"""
    grads = _k11(params, packed, deg, radii, cov3D, clamped, g2, grgb, gco, gstride)
    return _adam(params, grads, ms, vs, lrs, steps, grad_scale) + (grads,)


def _sparse_call(params, ms, vs, packed, deg, radii, cov3D, clamped, g2, grgb, gco, gstride, lrs, steps, grad_scale,
                 dyn=None, skip=None, ws=None, ws_bytes=None, active_out=None, num_active=None, edit=None, sh_coeffs=16,
                 P=None, tables=True):
    lib = _lib()
    N, B = params[0].shape[0], packed.shape[0]
    args = [N if P is None else P, B, deg, sh_coeffs, _p(params[0]), _p(params[1]), 1.0, _p(params[2]), _p(params[3]),
            _p(params[4]), _p(params[5]), _p(packed), W, H, _p(radii), _p(cov3D), _p(clamped), _p(g2), _p(gco), _p(grgb),
            gstride, VP(*[_p(t) for t in ms]) if tables else None, VP(*[_p(t) for t in vs]),
            D6(*lrs) if lrs is not None else None, D6(*B1S), D6(*B2S), D6(*EPSS),
            I64(*steps) if steps is not None else None, grad_scale, _p(dyn), _p(skip), _p(ws),
            ws_bytes if ws_bytes is not None else (ws.numel() * 8 if ws is not None else 0), _p(active_out),
            _p(num_active), _stream()]
    if edit is not None:
        args[edit[0]] = edit[1]
    return lib.gsr_preprocess_backward_adam_raw_batched_sparse(*args)


def _workspace(N, device):
    need = int(_lib().gsr_sparse_step_workspace_bytes(N))
    return torch.empty((need + 7) // 8, dtype=torch.int64, device=device)


class _Case:
    """one (B, deg, N) scene with its gradients, its moments in progress and the dense pair's result: built once, shared
    by the tests and never changed (every launch under test runs on clones)"""

    def __init__(self, B, deg, N, device, zero_rows=True):
        import synthetic_scene as S

        self.B, self.deg, self.N, self.device = B, deg, N, device
        m = S.SyntheticGaussianModel(N, W, H, seed=2, device=device, scale_coef=0.01)
        with torch.no_grad():
            m._xyz[::7] = torch.tensor([-50.0, 0.0, -44.0], device=device)  # behind all cameras
        self.params = [getattr(m, n).detach().clone().contiguous() for n in NAMES]
        self.packed = _packed_cams(B, deg, device)
        self.radii, self.cov3D, self.clamped = _forward(self.params, self.packed, deg)
        gen = torch.Generator().manual_seed(5)
        rec = torch.randn((B, N, 9), generator=gen)
        if zero_rows:
            rec[:, 1::3, :] = 0.0
        self.rec = rec.to(device).reshape(B * N, 9).contiguous()
        self.ms = [(0.01 * torch.randn(t.shape, generator=gen)).to(device) for t in self.params]
        self.vs = [(a.cpu() ** 2 * (1.0 + torch.rand(a.shape, generator=gen)) + 1e-8).to(device) for a in self.ms]
        self.grad_scale = 1.0 / B

    def grads(self, gstride, rec=None):
        rec = self.rec if rec is None else rec
        g2, grgb, gco = rec[:, 0:2], rec[:, 2:5], rec[:, 5:9]
        if gstride == 0:
            # (copies, not .contiguous(): a one-row column view already counts as contiguous and would stay a view)
            g2, grgb, gco = (t.clone(memory_format=torch.contiguous_format) for t in (g2, grgb, gco))
        return g2, grgb, gco

    def expected(self, rec=None, lrs=LRS, steps=STEPS):
        """-> active [N] bool (host), (p, m, v) expected, (p, m, v) dense, K11's gradients"""
        g2, grgb, gco = self.grads(0, rec)
        active = _active(self.radii, g2, grgb, gco)
        p, m, v, grads = _dense_pair(self.params, self.ms, self.vs, self.packed, self.deg, self.radii, self.cov3D,
                                     self.clamped, g2, grgb, gco, 0, lrs, steps, self.grad_scale)
        a = active.to(self.device)

        def pick(new, old):
            return [torch.where(a.view(-1, *([1] * (o.dim() - 1))), n, o) for n, o in zip(new, old)]

        return active, (pick(p, self.params), pick(m, self.ms), pick(v, self.vs)), (p, m, v), grads

    def run(self, gstride, rec=None, lrs=LRS, steps=STEPS, **kw):
        """the launch under test on clones -> code, (p, m, v), active_out, num_active"""
        g2, grgb, gco = self.grads(gstride, rec)
        p, m, v = [t.clone() for t in self.params], [t.clone() for t in self.ms], [t.clone() for t in self.vs]
        act = torch.full((self.N,), 7, dtype=torch.uint8, device=self.device)
        num = torch.full((1,), -5, dtype=torch.int32, device=self.device)
        code = _sparse_call(p, m, v, self.packed, self.deg, self.radii, self.cov3D, self.clamped, g2, grgb, gco, gstride,
                            lrs, steps, self.grad_scale, ws=_workspace(self.N, self.device), active_out=act,
                            num_active=num, **kw)
        torch.cuda.synchronize()
        return code, (p, m, v), act, num


@functools.lru_cache(maxsize=None)
def _case(B, deg, N, device, zero_rows=True):
    return _Case(B, deg, N, device, zero_rows), {}


def _case_expected(B, deg, N, device):
    c, memo = _case(B, deg, N, str(device))
    if "exp" not in memo:
        memo["exp"] = c.expected()
    return c, memo["exp"]


def _assert_state(got, want, what):
    for role, gs, wsn in zip(("parameter", "exp_avg", "exp_avg_sq"), got, want):
        for n, a, b in zip(NAMES, gs, wsn):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                f"{what}: {role} {n}: {int((a.view(torch.int32) != b.view(torch.int32)).sum())} words differ"


def _assert_shares(active, N):
    if N >= 777:  # a test that classifies everything one way shows nothing
        assert int(active.sum()) >= N // 8 and int((~active).sum()) >= N // 4, (int(active.sum()), N)


# ------------------------------------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize("gstride", [0, 9])
@pytest.mark.parametrize("B,deg,N", [(1, 3, 4099), (3, 3, 4099), (2, 0, 777), (1, 1, 129), (2, 3, 63), (1, 3, 1),
                                     # more cameras than the update's camera queue holds (its refill runs more than once
                                     # per loop), the list ending in a ragged only / last workgroup
                                     (5, 3, 300), (4, 1, 129)])
def test_sparse_step_equals_the_dense_pair_on_active_rows(device, B, deg, N, gstride):
    c, (active, want, dense, _) = _case_expected(B, deg, N, device)
    _assert_shares(active, N)
    code, got, act, num = c.run(gstride)
    assert code == 0
    assert torch.equal(act.cpu().bool(), active) and int(act.max()) <= 1
    assert int(num) == int(active.sum())
    _assert_state(got, want, f"B={B} deg={deg} N={N} stride={gstride}")
    ia = (~active).to(device)
    if int(ia.sum()):  # inactive rows are SEEN not to decay: the dense pair did change their moments
        assert not torch.equal(dense[1][0][ia], c.ms[0][ia]) and torch.equal(got[1][0][ia], c.ms[0][ia])
        assert not torch.equal(dense[2][4][ia], c.vs[4][ia]) and torch.equal(got[2][4][ia], c.vs[4][ia])
    if int(active.sum()):
        a = active.to(device)
        assert not torch.equal(got[0][0][a], c.params[0][a])


# ------------------------------------------------------------------------------------------------ 2. edge words
def test_edge_words_classify_as_defined(device):
    B, deg, N = 2, 3, 777
    c, _ = _case(B, deg, N, str(device))
    radii = c.radii.cpu()
    vis_all = torch.nonzero((radii > 0).all(0)).flatten().tolist()
    vis0_only = torch.nonzero((radii[0] > 0) & (radii[1] <= 0)).flatten().tolist()
    assert len(vis_all) >= 3 and len(vis0_only) >= 1
    r_negzero, r_denorm, r_spare = vis_all[:3]
    r_culled = vis0_only[0]
    rec = c.rec.clone().reshape(B, N, 9)
    rec[:, [r_negzero, r_denorm, r_culled], :] = 0.0
    bits = rec.view(torch.int32)                     # (written as bits: no kernel in between can flush or normalise them)
    bits[1, r_negzero, 3] = -2 ** 31                 # the only non-zero BITS of the row: -0.0
    bits[0, r_denorm, 7] = 713                       # one denormal word, 713 * 2^-149
    rec[1, r_culled, :] = 3.0                        # non-zero only for the camera in which the row is culled
    culled = torch.nonzero(c.radii <= 0)             # NaN in the gradient rows of every culled (k, i) ...
    rec[culled[:, 0], culled[:, 1], :] = float("nan")
    rec[1, r_culled, :] = 3.0                        # ... but this one keeps its finite words
    assert float(rec[1, r_negzero, 3].cpu()) == 0.0 and bool(torch.signbit(rec[1, r_negzero, 3].cpu()))
    assert 0.0 < float(rec[0, r_denorm, 7].cpu().double()) < 1.1754944e-38
    rec = rec.reshape(B * N, 9).contiguous()
    active, want, _, _ = c.expected(rec)
    assert not active[r_negzero] and active[r_denorm] and not active[r_culled] and active[r_spare]
    _assert_shares(active, N)
    for gstride in (0, 9):
        code, got, act, num = c.run(gstride, rec)
        assert code == 0
        a = act.cpu().bool()
        assert not a[r_negzero] and a[r_denorm] and not a[r_culled]
        assert torch.equal(a, active) and int(num) == int(active.sum())
        assert not any(bool(torch.isnan(t).any()) for role in got for t in role)
        _assert_state(got, want, f"edge words stride={gstride}")


# ------------------------------------------------------------------------------------------------ 3. all / none
def _all_active_case(B, deg, N, device, count=None):
    """the rows of an N-row scene that some camera sees (the first `count` of them), every gradient word non-zero"""
    full = _Case(B, deg, N, str(device), zero_rows=False)
    keep = torch.nonzero((full.radii > 0).any(0)).flatten()[:count]
    full.N = int(keep.numel())
    full.params = [t[keep].contiguous() for t in full.params]
    full.ms, full.vs = [t[keep].contiguous() for t in full.ms], [t[keep].contiguous() for t in full.vs]
    full.rec = full.rec.reshape(B, N, 9)[:, keep].reshape(B * full.N, 9).contiguous()
    full.radii, full.cov3D, full.clamped = _forward(full.params, full.packed, deg)
    return full


@pytest.mark.parametrize("gstride", [0, 9])
def test_list_of_exactly_two_full_workgroups(device, gstride):
    """all 256 rows of a 256-row scene active: the list fills the grid's two workgroups exactly (no clamped lane)"""
    B, deg = 3, 3
    full = _all_active_case(B, deg, 500, device, count=256)
    assert full.N == 256
    active, want, dense, _ = full.expected()
    assert bool(active.all())
    code, got, act, num = full.run(gstride)
    assert code == 0 and int(num) == 256 and bool(act.bool().all())
    _assert_state(got, dense, f"256 of 256 rows active stride={gstride}")


def test_all_rows_active_and_no_row_active(device):
    B, deg, N = 2, 3, 777
    c, _ = _case(B, deg, N, str(device))
    # all rows active: a scene in which every row is seen by camera 0, every gradient word non-zero
    full = _all_active_case(1, deg, 333, device)
    assert full.N >= 100
    active, want, dense, _ = full.expected()
    assert bool(active.all())
    code, got, act, num = full.run(9)
    assert code == 0 and int(num) == full.N and bool(act.bool().all())
    _assert_state(got, dense, "all rows active")
    # no row active: all gradients zero
    zero = torch.zeros_like(c.rec)
    for gstride in (0, 9):
        code, got, act, num = c.run(gstride, zero)
        assert code == 0 and int(num) == 0 and int(act.max()) == 0
        _assert_state(got, (c.params, c.ms, c.vs), "no row active")


# ------------------------------------------------------------------------------------------------ 4. dyn / skip
def test_dyn_block_and_skip_word(device):
    B, deg, N = 3, 3, 4099
    c, (active, want, _, _) = _case_expected(B, deg, N, device)
    # what FusedAdam.graph_hyper computes for the next step: lr / (1 - beta1^t) x 6, then 1 / sqrt(1 - beta2^t) x 6
    hyper = [LRS[t] / (1.0 - B1S[t] ** STEPS[t]) for t in range(6)] + \
            [1.0 / (1.0 - B2S[t] ** STEPS[t]) ** 0.5 for t in range(6)]
    dyn = torch.tensor(hyper, dtype=torch.float32, device=device)
    code, got, act, num = c.run(9, lrs=None, steps=None, dyn=dyn)
    assert code == 0 and int(num) == int(active.sum()) and torch.equal(act.cpu().bool(), active)
    _assert_state(got, want, "dyn_dev")
    skip = torch.ones(1, dtype=torch.int32, device=device)
    for kw in (dict(), dict(lrs=None, steps=None, dyn=dyn)):
        code, got, act, num = c.run(9, skip=skip, **kw)
        assert code == 0
        _assert_state(got, (c.params, c.ms, c.vs), "skip word")
        assert int(num) == -5 and bool((act == 7).all())  # left as they were
    skip.zero_()
    code, got, act, num = c.run(0, skip=skip)
    assert code == 0 and int(num) == int(active.sum())
    _assert_state(got, want, "skip word == 0")


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_argument_validation(device):
    B, deg, N = 2, 3, 63
    c, _ = _case(B, deg, N, str(device))
    lib = _lib()
    need = int(lib.gsr_sparse_step_workspace_bytes(N))

    def call(**kw):
        g2, grgb, gco = c.grads(9)
        p, m, v = [t.clone() for t in c.params], [t.clone() for t in c.ms], [t.clone() for t in c.vs]
        kw.setdefault("ws", _workspace(N, device))
        code = _sparse_call(p, m, v, c.packed, deg, c.radii, c.cov3D, c.clamped, g2, grgb, gco, 9, LRS, STEPS,
                            c.grad_scale, **kw)
        torch.cuda.synchronize()
        _assert_state((p, m, v), (c.params, c.ms, c.vs), f"rejected call {sorted(kw)}")  # nothing launched
        return code

    for idx in (4, 5, 7, 8, 9, 10, 11, 14, 15, 16, 17, 18, 19, 22, 24, 25, 26):  # every pointer but lrs / steps
        assert call(edit=(idx, None)) == GSR_EINVAL, idx
    assert call(edit=(23, None)) == GSR_EINVAL and call(edit=(27, None)) == GSR_EINVAL  # lrs / steps without dyn_dev
    assert call(tables=False) == GSR_EINVAL
    assert call(ws=None) == GSR_EINVAL
    assert call(sh_coeffs=4) == GSR_EINVAL and call(sh_coeffs=15) == GSR_EINVAL
    assert call(P=-1) == GSR_EINVAL
    assert call(edit=(1, 0)) == GSR_EINVAL and call(edit=(12, -W)) == GSR_EINVAL and call(edit=(20, -9)) == GSR_EINVAL
    assert call(ws_bytes=need - 1) == GSR_ENOSPACE and call(ws_bytes=0) == GSR_ENOSPACE
    ws = _workspace(N + 2, device)
    assert call(edit=(31, ws.data_ptr() + 4), ws=ws) == GSR_ENOSPACE  # not 8-byte aligned
    assert call(P=0) == 0


# ------------------------------------------------------------------------------------------------ 6. FusedAdam
@pytest.mark.parametrize("B,deg,N", [(1, 3, 4099), (3, 3, 4099), (2, 0, 777)])
def test_fused_adam_sparse_over_four_steps(device, B, deg, N):
    """the optimizer's sparse mode through autograd == a loop that applies the expected values of the bit-equality test
    step by step (K1 through the C ABI on the loop's own parameters, K11 + gsr_adam_step_multi on clones, where(active));
    then a step the mode cannot fuse: the plain dense Adam, counted"""
    import diff_gaussian_rasterization as dgr
    import synthetic_scene as S
    from fused_optim import FusedAdam

    packed = _packed_cams(B, deg, device)
    gen = torch.Generator().manual_seed(5)
    ws = [[torch.randn(s, generator=gen) for s in [(N, 2), (N, 3), (N, 4)]] for _ in range(B)]
    for k in range(B):
        for t in ws[k]:
            t[1::3] = 0.0
    ws = [[t.to(device) for t in wk] for wk in ws]
    m = S.SyntheticGaussianModel(N, W, H, seed=2, device=device, scale_coef=0.01)
    with torch.no_grad():
        m._xyz[::7] = torch.tensor([-50.0, 0.0, -44.0], device=device)
    opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, grad_scale=1.0 / B, sparse=True)
    by_param = {id(p): g for g in opt.param_groups for p in g["params"]}
    groups = [by_param[id(getattr(m, n))] for n in NAMES]
    for g, lr in zip(groups, LRS):
        g["lr"] = lr
    exp_p = [getattr(m, n).detach().clone() for n in NAMES]
    exp_m, exp_v = [torch.zeros_like(t) for t in exp_p], [torch.zeros_like(t) for t in exp_p]

    def backward(it):
        raw = [getattr(m, n) for n in NAMES]
        m2, rgb, co, radii, depths = dgr.preprocess_gaussians_raw_batched(*raw, packed, deg, 1.0, W, H, tanfov0=None)
        loss = sum((m2[k] * ws[k][0]).sum() + (rgb[k] * ws[k][1]).sum() + (co[k] * ws[k][2]).sum()
                   for k in range(B)) * (1.0 + it)
        loss.backward()

    def expected_step(it, mask=True):
        nonlocal exp_p, exp_m, exp_v
        radii, cov3D, clamped = _forward(exp_p, packed, deg)
        g2, grgb, gco = (torch.stack([ws[k][j] for k in range(B)]).reshape(B * N, -1) * (1.0 + it) for j in range(3))
        active = _active(radii, g2, grgb, gco)
        p, mm, vv, _ = _dense_pair(exp_p, exp_m, exp_v, packed, deg, radii, cov3D, clamped, g2.contiguous(),
                                   grgb.contiguous(), gco.contiguous(), 0, [g["lr"] for g in groups], [it + 1] * 6,
                                   1.0 / B)
        if mask:
            a = active.to(device)
            sel = lambda new, old: [torch.where(a.view(-1, *([1] * (o.dim() - 1))), n, o) for n, o in zip(new, old)]
            p, mm, vv = sel(p, exp_p), sel(mm, exp_m), sel(vv, exp_v)
        exp_p, exp_m, exp_v = p, mm, vv
        return active

    try:
        for it in range(4):
            backward(it)
            assert all(getattr(m, n).grad is None for n in NAMES)
            opt.step()
            opt.zero_grad(set_to_none=True)
            active = expected_step(it)
            _assert_shares(active, N)
            assert int(opt.last_num_active) == int(active.sum())
            got = ([getattr(m, n).detach() for n in NAMES], [opt.state[getattr(m, n)]["exp_avg"] for n in NAMES],
                   [opt.state[getattr(m, n)]["exp_avg_sq"] for n in NAMES])
            _assert_state(got, (exp_p, exp_m, exp_v), f"step {it}")
            assert all(float(opt.state[getattr(m, n)]["step"]) == it + 1 for n in NAMES)
        assert opt.sparse_steps == 4 and opt.fused_steps == 4 and opt.dense_fallback_steps == 0
        assert opt.materialized_steps == 0
        # a second backward before the step materializes both (.grad = K11(first) + K11(second)): that step is the plain
        # dense Adam on every row, counted as a fallback
        it, factors = 4, (5.0, 0.5)
        for f in factors:
            raw = [getattr(m, n) for n in NAMES]
            m2, rgb, co, radii, depths = dgr.preprocess_gaussians_raw_batched(*raw, packed, deg, 1.0, W, H, tanfov0=None)
            (sum((m2[k] * ws[k][0]).sum() + (rgb[k] * ws[k][1]).sum() + (co[k] * ws[k][2]).sum()
                 for k in range(B)) * f).backward()
        assert all(getattr(m, n).grad is not None for n in NAMES)
        opt.step()
        opt.zero_grad(set_to_none=True)
        assert opt.dense_fallback_steps == 1 and opt.sparse_steps == 4 and opt.materialized_steps == 2
        assert all(float(opt.state[getattr(m, n)]["step"]) == 5 for n in NAMES)
        radii, cov3D, clamped = _forward(exp_p, packed, deg)
        total = None
        for f in factors:
            g2, grgb, gco = (torch.stack([ws[k][j] for k in range(B)]).reshape(B * N, -1).contiguous() * f
                             for j in range(3))
            grads = _k11(exp_p, packed, deg, radii, cov3D, clamped, g2, grgb, gco, 0)
            total = grads if total is None else [a.add_(b) for a, b in zip(total, grads)]
        exp_p, exp_m, exp_v = _adam(exp_p, total, exp_m, exp_v, [g["lr"] for g in groups], [5] * 6, 1.0 / B)
        got = ([getattr(m, n).detach() for n in NAMES], [opt.state[getattr(m, n)]["exp_avg"] for n in NAMES],
               [opt.state[getattr(m, n)]["exp_avg_sq"] for n in NAMES])
        _assert_state(got, (exp_p, exp_m, exp_v), "dense fallback step")
    finally:
        opt.set_fuse_backward(False)


# ------------------------------------------------------------------------------------------------ 7. captured
def test_captured_sparse_iteration_equals_the_eager_sparse_loop(device, monkeypatch):
    import fused_optim
    import test_gpu_graphed_step as G

    made = []

    class Recording(fused_optim.FusedAdam):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setenv("GSR_SPARSE_ADAM", "1")  # read at construction: the shared loop builds a sparse optimizer
    monkeypatch.setattr(fused_optim, "FusedAdam", Recording)
    steps = 7
    ref = G._train(device, steps, 1, graph=False)
    run = G._train(device, steps, 1, graph=True)
    st = run[3]
    assert st["disabled"] is None, st
    assert st["captured"] == 1 and st["eager"] == 2 and st["replayed"] == steps - 2 and st["redone"] == 0, st
    assert len(made) == 2 and all(o.sparse for o in made)
    assert made[0].sparse_steps == steps and made[1].sparse_steps == steps
    assert made[0].dense_fallback_steps == 0 and made[1].dense_fallback_steps == 0
    G._compare(run, ref, steps)
    n_eager, n_replay = int(made[0].last_num_active), int(made[1].last_num_active)
    N = int(os.environ.get("GSR_TEST_SCENE", "60000,640,368").split(",")[0])
    assert 0 < n_eager < N and n_replay == n_eager, (n_eager, n_replay, N)


# ------------------------------------------------------------------------------------------------ 8. independent
def test_updated_rows_agree_with_fp64_adam(device):
    """the updated rows against the fp64 restatement of Adam (tests/leaf_refs.py) on K11's gradients, with the tolerance
    the dense kernel gets in tests/test_gpu_adam_edges.py (helpers.assert_elem_close, K = 8)"""
    import leaf_refs as R
    from helpers import assert_elem_close

    B, deg, N = 2, 3, 63
    c, (active, want, dense, grads) = _case_expected(B, deg, N, device)
    assert 0 < int(active.sum()) < N
    code, got, act, num = c.run(9)
    assert code == 0
    for j, n in enumerate(NAMES):
        rows = lambda t: t[active.to(t.device)].reshape(-1).cpu()
        args = (rows(c.params[j]), rows(grads[j]), rows(c.ms[j]), rows(c.vs[j]))
        hp = dict(lr=LRS[j], b1=B1S[j], b2=B2S[j], eps=EPSS[j], step=STEPS[j], grad_scale=c.grad_scale)
        r64, r32 = R.adam_reference(*args, **hp), R.adam_torch32(*args, **hp)
        for role, a, b, c32 in zip("pmv", (got[0][j], got[1][j], got[2][j]), r64, r32):
            ratio = assert_elem_close(rows(a), b, c32, K=8, what=f"{n} {role}")
            print(f"RATIO sparse adam {n} {role} {ratio:.4g}")
