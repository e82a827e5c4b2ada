"""csrc/activations.hip at its edges: every SH width (the float4 path and the generic one), sizes that straddle a
256-thread block, saturating inputs and absent output gradients; forward outputs and the five input gradients element by
element against torch in fp64 (exp, F.normalize(eps=1e-12), sigmoid, cat and their autograd), guard bands around every
buffer of the direct C-ABI calls.  Tolerance: helpers.assert_elem_close against the same torch code in fp32."""
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_elem_close
from leaf_refs import Guard

pytestmark = pytest.mark.gpu

K = 8
f32, i32 = torch.float32, torch.int32
SHAPES = lambda N, rest: [(N, 3), (N, 4), (N, 1), (N, 1, 3), (N, rest, 3)]  # noqa: E731  (the five raw parameters)


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def _inputs(N, rest, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * rest + N)
    sc = torch.randn(N, 3, generator=g) - 3.0
    rot = torch.randn(N, 4, generator=g)
    op = 2.0 * torch.randn(N, 1, generator=g)
    dc, fr = torch.randn(N, 1, 3, generator=g), torch.randn(N, rest, 3, generator=g)
    ws = [torch.rand(s, generator=g) + 0.5 for s in [(N, 3), (N, 4), (N, 1), (N, 1 + rest, 3)]]
    return [sc, rot, op, dc, fr], ws


def _reference(params, ws, dtype, use=(0, 1, 2, 3)):
    """-> (outputs, input gradients of sum_k (out_k * w_k).sum() over the outputs in `use`)"""
    leaf = [p.to(dtype).clone().requires_grad_(True) for p in params]
    outs = (torch.exp(leaf[0]), F.normalize(leaf[1], eps=1e-12), torch.sigmoid(leaf[2]), torch.cat((leaf[3], leaf[4]), dim=1))
    loss = sum((outs[k] * ws[k].to(dtype)).sum() for k in use)
    grads = torch.autograd.grad(loss, leaf, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, leaf)]
    return [o.detach() for o in outs], grads


@pytest.mark.parametrize("N", [1, 5, 21, 22, 257, 3001])
@pytest.mark.parametrize("rest", [0, 3, 8, 15, 24])
def test_activations_every_element_direct_abi(device, rest, N):
    lib = _lib()
    params, ws = _inputs(N, rest)
    o64, g64 = _reference(params, ws, torch.float64)
    o32, g32 = _reference(params, ws, torch.float32)
    width = (1 + rest) * 3
    gin = [Guard(p.numel(), f32, device) for p in params]
    for b, p in zip(gin, params):
        b.t.copy_(p.reshape(-1))
    gout = [Guard(n, f32, device) for n in (3 * N, 4 * N, N, N * width)]
    for b in gin + gout:
        b.seal()
    assert lib.gsr_activate_forward(N, rest, *[b.ptr for b in gin], *[b.ptr for b in gout], _stream()) == 0
    torch.cuda.synchronize()
    for b in gin:
        b.check("forward input", whole=True)
    for b in gout:
        b.check("forward output")
    tag = f"rest={rest} N={N}"
    outs = [b.t.cpu().reshape(o.shape) for b, o in zip(gout, o64)]
    for name, got, a, b in zip(("scales", "rotations", "opacities"), outs, o64, o32):
        print(f"RATIO act {name} {tag} {assert_elem_close(got, a, b, K=K, what=f'{tag} {name}'):.4g}")
    assert torch.equal(outs[3].view(i32), o32[3].view(i32)), f"{tag}: shs is a copy"
    # backward: rotation, the forward's scales and opacities, the four output gradients
    gw = [Guard(w.numel(), f32, device) for w in ws]
    for b, w in zip(gw, ws):
        b.t.copy_(w.reshape(-1))
    gd = [Guard(p.numel(), f32, device) for p in params]
    for b in gin + gout + gw + gd:
        b.seal()
    assert lib.gsr_activate_backward(N, rest, gin[1].ptr, gout[0].ptr, gout[2].ptr, *[b.ptr for b in gw],
                                     *[b.ptr for b in gd], _stream()) == 0
    torch.cuda.synchronize()
    for b in gin + gout + gw:
        b.check("backward input", whole=True)
    for b in gd:
        b.check("backward output")
    grads = [b.t.cpu().reshape(g.shape) for b, g in zip(gd, g64)]
    for name, got, a, b in zip(("d_scaling", "d_rotation", "d_opacity"), grads, g64, g32):
        print(f"RATIO act {name} {tag} {assert_elem_close(got, a, b, K=K, what=f'{tag} {name}'):.4g}")
    assert torch.equal(grads[3].view(i32), g32[3].view(i32)) and torch.equal(grads[4].view(i32), g32[4].view(i32)), \
        f"{tag}: d_dc / d_rest are copies"


@pytest.mark.parametrize("rest", [0, 8, 15])
@pytest.mark.parametrize("use", [(3,), (1,)], ids=["only_shs", "only_rotations"])
def test_activations_absent_output_gradients(device, rest, use):
    """a loss that uses one output only: autograd hands the backward None for the others -- their inputs get exactly 0"""
    from diff_gaussian_rasterization import fused_activations

    N = 257
    params, ws = _inputs(N, rest, seed=9)
    _, g64 = _reference(params, ws, torch.float64, use=use)
    _, g32 = _reference(params, ws, torch.float32, use=use)
    leaf = [p.to(device).requires_grad_(True) for p in params]
    outs = fused_activations(*leaf)
    sum((outs[k] * ws[k].to(device)).sum() for k in use).backward()
    used = {3: (3, 4), 1: (1,)}[use[0]]
    for k, p in enumerate(leaf):
        got = p.grad.cpu()
        if k in used:
            if k in (3, 4):
                assert torch.equal(got.view(i32), g32[k].view(i32))
            else:
                assert_elem_close(got, g64[k], g32[k], K=K, what=f"rest={rest} use={use} grad {k}")
        else:
            assert bool((got == 0).all()), f"gradient {k} must be exactly zero"


def test_activations_saturating_rows(device):
    """scaling in {-100, 0, 88, 89}, opacity in {-100, -20, 20, 100}, a quaternion that is exactly zero and norms from
    1e-6 to 1e3.  Where torch's fp32 result is inf or 0 the kernel's is the same; the other elements within 8 ulp of the
    fp64 value (+ 2^-126: results below the normal range may be flushed), d_opacity within 8 * 2^-24 |g| (an error of
    one ulp(1) in s moves s (1 - s) by at most that), d_rotation within 16 * 2^-24 max|g_row| / max(|x|, 1e-12) (the
    rounding of the cancelling difference g - y (y.g), scaled like the result)."""
    from diff_gaussian_rasterization import fused_activations

    N, rest = 16, 15
    params, ws = _inputs(N, rest, seed=4)
    sc, rot, op = params[0], params[1], params[2]
    sc[:] = torch.tensor([-100.0, 0.0, 88.0, 89.0]).repeat(4)[:, None]
    op[:] = torch.tensor([-100.0, -20.0, 20.0, 100.0]).repeat_interleave(4)[:, None]
    norms = torch.logspace(-6, 3, N - 1, dtype=torch.float64)
    rot[1:] = (F.normalize(rot[1:].double()) * norms[:, None]).float()
    rot[0] = 0.0
    o64, g64 = _reference(params, ws, torch.float64)
    o32, g32 = _reference(params, ws, torch.float32)
    leaf = [p.to(device).requires_grad_(True) for p in params]
    outs = fused_activations(*leaf)
    sum((o * w.to(device)).sum() for o, w in zip(outs, ws)).backward()
    got_o = [o.detach().cpu() for o in outs]
    got_g = [p.grad.cpu() for p in leaf]
    tiny = 2.0 ** -126
    n_row = rot.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    tol_g = {0: None, 1: 16 * 2.0 ** -24 * ws[1].double().abs().amax(dim=1, keepdim=True) / n_row,
             2: 8 * 2.0 ** -24 * ws[2].double().abs()}

    def check(got, r64, r32, tol, what):
        exact = torch.isinf(r32) | (r32 == 0)
        assert bool(exact.any()) or what in ("rotations", "d_rotation"), what
        assert torch.equal(got[exact], r32[exact]), f"{what}: inf / 0 results differ from torch's fp32 ones"
        rest_ = ~exact
        t = (8 * 2.0 ** -23 * r64.abs() + tiny) if tol is None else tol.expand_as(r64) + 8 * 2.0 ** -23 * r64.abs()
        err = (got.double() - r64).abs()
        assert bool((err[rest_] <= t[rest_]).all()), f"{what}: {float((err[rest_] / t[rest_]).max()):.3g} x the bound"

    for k, name in enumerate(("scales", "rotations", "opacities")):
        check(got_o[k], o64[k], o32[k], None, name)
    assert torch.equal(got_o[3].view(i32), o32[3].view(i32))
    for k, name in enumerate(("d_scaling", "d_rotation", "d_opacity")):
        check(got_g[k], g64[k], g32[k], tol_g[k], name)


def test_activations_empty_model_and_argument_checks(device):
    lib = _lib()
    s = _stream()
    assert lib.gsr_activate_forward(0, 15, *([None] * 9), s) == 0
    assert lib.gsr_activate_backward(0, 15, *([None] * 12), s) == 0
    assert lib.gsr_activate_forward(-1, 15, *([None] * 9), s) == -1
    assert lib.gsr_activate_forward(4, 15, *([None] * 9), s) == -1
    assert lib.gsr_activate_backward(4, -1, *([None] * 12), s) == -1
