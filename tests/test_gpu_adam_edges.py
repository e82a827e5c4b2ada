"""csrc/optim.hip at its edges: gsr_adam_step and gsr_adam_step_multi element by element against the update of gsr_adam1
written in fp64 (leaf_refs.adam_reference), sizes around the float4 groups, the 256-thread block and the multi kernel's
4096-element block table, per-tensor hyper-parameters, NaN gaps between the tensors of one launch, the argument checks,
and FusedAdam's split into launches of 16.  Tolerance: helpers.assert_elem_close against torch.optim.Adam in fp32."""
import ctypes

import pytest
import torch

import leaf_refs as R
from helpers import assert_elem_close
from leaf_refs import Guard

pytestmark = pytest.mark.gpu

K = 8
GSR_EINVAL = -1
f32, i32 = torch.float32, torch.int32


def _lib():
    from diff_gaussian_rasterization import _lib as L

    return L.lib


def _stream():
    from diff_gaussian_rasterization import _stream as s

    return s()


def _check(got, r64, r32, tag):
    for name, a, b, c in zip("pmv", got, r64, r32):
        ratio = assert_elem_close(a, b, c, K=K, what=f"{tag} {name}")
        print(f"RATIO adam {name} {tag} {ratio:.4g}")


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("step0", [1, 30000])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097])
def test_adam_step_single_tensor(device, n, step0, grad_scale):
    lib = _lib()
    hp = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-15)
    p, g, m, v = R.adam_inputs(n, seed=n + step0)
    if step0 == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    bufs = [Guard(n, f32, device) for _ in range(4)]
    for b, t in zip(bufs, (p, g, m, v)):
        b.t.copy_(t)
    s64, s32 = (p.double(), m.double(), v.double()), (p, m, v)
    for it in range(3):
        g_it = R.adam_inputs(n, seed=7 * n + it)[1] if it else g
        bufs[1].t.copy_(g_it)
        for b in bufs:
            b.seal()
        assert lib.gsr_adam_step(n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, hp["lr"], hp["b1"], hp["b2"],
                                 hp["eps"], step0 + it, grad_scale, _stream()) == 0
        torch.cuda.synchronize()
        bufs[1].check("gradient", whole=True)
        for b in (bufs[0], bufs[2], bufs[3]):
            b.check("parameter / moment")
        s64 = R.adam_reference(s64[0], g_it, s64[1], s64[2], step=step0 + it, grad_scale=grad_scale, **hp)
        s32 = R.adam_torch32(s32[0], g_it, s32[1], s32[2], step=step0 + it, grad_scale=grad_scale, **hp)
        _check([bufs[i].t.cpu() for i in (0, 2, 3)], s64, s32, f"single n={n} step={step0 + it} gs={grad_scale}")


class _Packed:
    """all tensors of one role (parameters, gradients, first or second moments) of a multi-tensor launch in ONE guarded
    allocation, at 16-byte-aligned offsets with gaps of 4..7 NaN floats: a block that looks up the wrong tensor, or runs past
    the end of its own, lands in a gap or in a neighbour"""

    def __init__(self, tensors, device):
        self.off, pos = [], 0
        for t in tensors:
            self.off.append(pos)
            pos += (t.numel() + 3) // 4 * 4 + 4
        self.g = Guard(pos, f32, device)
        self.sizes = [t.numel() for t in tensors]
        self.gap = torch.ones(pos, dtype=torch.bool, device=device)
        for o, t in zip(self.off, tensors):
            self.g.t[o:o + t.numel()] = t.to(device)
            self.gap[o:o + t.numel()] = False

    def ptrs(self):
        return [self.g.ptr + 4 * o if n else None for o, n in zip(self.off, self.sizes)]

    def get(self):
        host = self.g.t.cpu()
        return [host[o:o + n].clone() for o, n in zip(self.off, self.sizes)]

    def check(self, what, whole=False):
        self.g.check(what, whole=whole)
        self.g.untouched(self.gap, what + " (gap between two tensors)")


def _hyper(k):
    """per-tensor lr, betas, eps and step"""
    return dict(lr=1e-3 * (1 + k), b1=0.9 - 0.02 * (k % 5), b2=0.999 - 0.003 * (k % 3), eps=[1e-15, 1e-8, 1e-6][k % 3],
                step=[1, 2, 7, 30000, 1000][k % 5])


def _multi_args(packs, numels, hps):
    T = len(numels)
    VP, D, I64 = ctypes.c_void_p * T, ctypes.c_double * T, ctypes.c_int64 * T
    return [T, I64(*numels)] + [VP(*p.ptrs()) for p in packs] + \
           [D(*[h[k] for h in hps]) for k in ("lr", "b1", "b2", "eps")] + [I64(*[h["step"] for h in hps])]


@pytest.mark.parametrize("numels", [[1, 4096, 0, 4097, 3, 8191, 16389, 4], list(range(4093, 4109))],
                         ids=["block_table_edges", "sixteen_tensors"])
def test_adam_step_multi_direct(device, numels):
    lib = _lib()
    grad_scale = 0.25
    ins = [R.adam_inputs(n, seed=100 + k) for k, n in enumerate(numels)]
    hps = [_hyper(k) for k in range(len(numels))]
    packs = [_Packed([t[i] for t in ins], device) for i in range(4)]  # p, g, m, v
    # per-tensor gsr_adam_step on copies: the same gsr_adam1 with identically derived constants -> the same bits
    singles = []
    for (p, g, m, v), h in zip(ins, hps):
        n = p.numel()
        if n == 0:
            singles.append((p, m, v))
            continue
        b = [Guard(n, f32, device) for _ in range(4)]
        for q, t in zip(b, (p, g, m, v)):
            q.t.copy_(t)
        assert lib.gsr_adam_step(n, b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, h["lr"], h["b1"], h["b2"], h["eps"],
                                 h["step"], grad_scale, _stream()) == 0
        singles.append(tuple(b[i].t.cpu() for i in (0, 2, 3)))
    for pk in packs:
        pk.g.seal()
    assert lib.gsr_adam_step_multi(*_multi_args(packs, numels, hps), grad_scale, _stream()) == 0
    torch.cuda.synchronize()
    packs[1].check("gradients", whole=True)
    for pk in (packs[0], packs[2], packs[3]):
        pk.check("parameters / moments")
    got = list(zip(packs[0].get(), packs[2].get(), packs[3].get()))
    for k, ((p, g, m, v), h) in enumerate(zip(ins, hps)):
        for name, a, b in zip("pmv", got[k], singles[k]):
            assert torch.equal(a.view(i32), b.view(i32)), f"tensor {k} (n={numels[k]}) {name}: multi != single launch"
        if numels[k] == 0:
            continue
        r64 = R.adam_reference(p, g, m, v, grad_scale=grad_scale, **h)
        r32 = R.adam_torch32(p, g, m, v, grad_scale=grad_scale, **h)
        _check(got[k], r64, r32, f"multi tensor {k} n={numels[k]}")
        z = (g == 0) & (m != 0)  # invisible Gaussians: the moments still decay, the parameter still moves
        if int(z.sum()):
            assert bool((got[k][1][z].abs() < m[z].abs()).all()) and bool((got[k][2][z] < v[z]).all())
            assert bool((got[k][0][z] != p[z]).any())


def test_adam_argument_checks_modify_nothing(device):
    lib = _lib()
    numels = [5, 4097, 12]
    ins = [R.adam_inputs(n, seed=k) for k, n in enumerate(numels)]
    hps = [_hyper(k) for k in range(3)]
    packs = [_Packed([t[i] for t in ins], device) for i in range(4)]
    for pk in packs:
        pk.g.seal()
    s = _stream()

    def call(numels_, hps_, ptr_edit=None, T=None):
        args = _multi_args(packs, numels_, hps_)
        if ptr_edit is not None:
            role, k, value = ptr_edit
            args[2 + role][k] = value
        if T is not None:
            args[0] = T
        return lib.gsr_adam_step_multi(*args, 1.0, s)

    assert call(numels, [dict(h, step=0) if k == 1 else h for k, h in enumerate(hps)]) == GSR_EINVAL
    assert call([5, -1, 12], hps) == GSR_EINVAL
    for role in range(4):
        assert call(numels, hps, ptr_edit=(role, 1, packs[role].ptrs()[1] + 4)) == GSR_EINVAL  # 4 B off
        assert call(numels, hps, ptr_edit=(role, 2, None)) == GSR_EINVAL  # null with numel > 0
    # 17 tensors (every table is 17 long: the check comes before anything is read)
    T = 17
    VP, D, I64 = ctypes.c_void_p * T, ctypes.c_double * T, ctypes.c_int64 * T
    p17 = [VP(*([packs[i].ptrs()[0]] * T)) for i in range(4)]
    assert lib.gsr_adam_step_multi(T, I64(*([5] * T)), *p17, D(*([1e-3] * T)), D(*([0.9] * T)), D(*([0.999] * T)),
                                   D(*([1e-8] * T)), I64(*([1] * T)), 1.0, s) == GSR_EINVAL
    # the single-tensor entry point
    a = [pk.ptrs()[1] for pk in packs]
    assert lib.gsr_adam_step(4097, a[0], a[1], a[2], a[3], 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, s) == GSR_EINVAL
    assert lib.gsr_adam_step(-1, a[0], a[1], a[2], a[3], 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, s) == GSR_EINVAL
    assert lib.gsr_adam_step(4097, a[0] + 4, a[1], a[2], a[3], 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, s) == GSR_EINVAL
    assert lib.gsr_adam_step(4097, a[0], None, a[2], a[3], 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, s) == GSR_EINVAL
    assert lib.gsr_adam_step(0, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, s) == 0
    torch.cuda.synchronize()
    for pk in packs:
        pk.check("argument checks", whole=True)


def test_fused_adam_two_launches_empty_and_skipped_parameters(device):
    """18 parameters (two launches of the multi kernel), one of shape (7, 0, 3), one without a gradient; two steps"""
    from fused_optim import FusedAdam

    shapes = [(4093 + k,) for k in range(8)] + [(7, 0, 3)] + [(33, 1 + k, 3) for k in range(8)] + [(5,)]
    assert len(shapes) == 18
    skipped = 4
    ins = [R.adam_inputs(max(1, int(torch.tensor(s).prod())), seed=40 + k) for k, s in enumerate(shapes)]
    host = [t[0][:int(torch.tensor(s).prod())].reshape(s) for t, s in zip(ins, shapes)]
    params = [h.clone().to(device).requires_grad_(True) for h in host]
    lrs = [1e-3 * (1 + k) for k in range(18)]
    betas = [(0.9 - 0.01 * (k % 4), 0.999 - 0.002 * (k % 3)) for k in range(18)]
    opt = FusedAdam([{"params": [p], "lr": lr, "betas": b} for p, lr, b in zip(params, lrs, betas)], lr=0.0, eps=1e-15)
    grad_scale = 0.25
    s64 = [(h.double(), torch.zeros_like(h).double(), torch.zeros_like(h).double()) for h in host]
    s32 = [(h, torch.zeros_like(h), torch.zeros_like(h)) for h in host]
    for it in range(2):
        grads = []
        for k, (p, s) in enumerate(zip(params, shapes)):
            g = R.adam_inputs(max(1, p.numel()), seed=500 + 31 * it + k)[1][:p.numel()].reshape(s)
            grads.append(g)
            p.grad = None if k == skipped else g.clone().to(device)
        opt.step(grad_scale=grad_scale)
        torch.cuda.synchronize()
        for k in range(18):
            if k == skipped:
                continue
            hp = dict(lr=lrs[k], b1=betas[k][0], b2=betas[k][1], eps=1e-15, step=it + 1, grad_scale=grad_scale)
            s64[k] = R.adam_reference(s64[k][0], grads[k], s64[k][1], s64[k][2], **hp)
            flat32 = [t.reshape(-1) for t in s32[k]]
            s32[k] = tuple(t.reshape(shapes[k]) for t in
                           R.adam_torch32(flat32[0], grads[k].reshape(-1), flat32[1], flat32[2], **hp))
            st = opt.state[params[k]]
            assert float(st["step"]) == it + 1
            _check((params[k].detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()), s64[k], s32[k],
                   f"FusedAdam tensor {k} step {it + 1}")
    assert len(opt.state[params[skipped]]) == 0
    assert torch.equal(params[skipped].detach().cpu(), host[skipped])
    assert params[8].shape == (7, 0, 3) and float(opt.state[params[8]]["step"]) == 2
