"""Inputs, plain references and deliberately wrong references of the leaf-kernel edge tests (loss, Adam): shared by the
CPU file that shows the tolerances separate right from wrong and by the GPU files that apply them to the HIP kernels."""
import torch
import torch.nn.functional as F

from oracle.loss_oracle import l1_map, ssim_grad_maps, ssim_map, window_1d

FAMILIES = ["noise", "smooth", "flat", "range", "ties"]
COEFS = [(1.0, 1.0, 0.8 / 7.0, -0.2 / 7.0), (0.3, -2.0, 1.0, 1.0)]  # (g_l1, g_ssim, scale_l1, scale_ssim)


# ---------------------------------------------------------------------------------------------- loss inputs
def loss_inputs(family, C, H, W, seed=0):
    """-> (image float32 [C,H,W], ground truth uint8 [C,H,W], tie mask bool [C,H,W]) of one input family.  x is moved away
    from y wherever 0 < |x - y| < 1e-4, so that sign(x - y) is the same in fp32 (y = u8 * (1/255f)) and in fp64."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * C + 13 * H + W + 7 * FAMILIES.index(family))
    ties = torch.zeros(C, H, W, dtype=torch.bool)
    if family in ("noise", "ties"):
        x = torch.rand(C, H, W, generator=g)
        gt = torch.randint(0, 256, (C, H, W), generator=g, dtype=torch.uint8)
        if family == "ties":
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            ties = (((yy + xx) % 2) == 0).expand(C, H, W).clone()
            gt[ties] = 0
            x[ties] = 0.0
    elif family == "smooth":
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        s = torch.stack([0.5 + 0.45 * torch.sin(0.11 * xx + 0.07 * yy + 1.3 * c) for c in range(C)])
        gt = torch.round(s * 255.0).to(torch.uint8)
        x = (gt.double() / 255.0 + 0.02 * torch.randn(C, H, W, generator=g, dtype=torch.float64)).float()
    elif family == "flat":
        gt = torch.full((C, H, W), 128, dtype=torch.uint8)
        x = (0.5 + 1e-3 * torch.randn(C, H, W, generator=g, dtype=torch.float64)).float()
    elif family == "range":
        x = torch.rand(C, H, W, generator=g) * 2.0 - 0.5
        gt = (torch.randint(0, 2, (C, H, W), generator=g) * 255).to(torch.uint8)
    else:
        raise ValueError(family)
    y = gt.double() / 255.0
    d = x.double() - y
    near = (d.abs() < 1e-4) & ~ties
    x = torch.where(near, (y + torch.where(d >= 0, 2e-4, -2e-4)).float(), x)
    d = x.double() - y
    assert bool(((d.abs() >= 1e-4) | ties).all()) and bool((d[ties] == 0).all())
    return x.contiguous(), gt.contiguous(), ties


# ---------------------------------------------------------------------------------------------- loss references
def _terms(x, y, w1, C2):
    """ssim_grad_maps with the window and C2 as parameters (the wrong references change them)"""
    ch = x.shape[-3]
    w2 = (w1[:, None] @ w1[None, :]).expand(ch, 1, 11, 11).contiguous()

    def conv(t):
        return F.conv2d(t.unsqueeze(0), w2, padding=5, groups=ch).squeeze(0)

    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    C1 = 0.01 ** 2
    A, B = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    Cd, Dd = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    ssim = A * B / (Cd * Dd)
    return (ssim, 2 * mu2 * (B - A) / (Cd * Dd) - ssim * 2 * mu1 * (Dd - Cd) / (Cd * Dd), -ssim / Dd,
            2 * A / (Cd * Dd))


def loss_reference(image, gt_u8, y0, y1, dtype, wrong=None):
    """The band-local loss of rows [y0, y1) of `image` [C,H,W] against gt_u8 [C,H,W] (only its band rows are used), computed
    in `dtype` on the CPU: dict(l1, ssim: the two sums; M: (M1, M2, M3) [C,rows,W]; grads: d/dx of
    g_l1 * scale_l1 * l1 + g_ssim * scale_ssim * ssim for every entry of COEFS, by autograd).  wrong=None is the reference
    (oracle.loss_oracle's l1_map / ssim_map / ssim_grad_maps); the others restate it with ONE deliberate mistake:
    "tap" (outermost window tap zeroed), "pad" (the band padded with the image's neighbouring rows, not zeros),
    "y256" (y = gt / 256), "sign0" (sign(0) = +1 in the L1 gradient), "c2" (C2 = 0.03)."""
    x = image[:, y0:y1].to(dtype).clone().requires_grad_(True)
    y = gt_u8[:, y0:y1].to(dtype) / (256.0 if wrong == "y256" else 255.0)
    if wrong is None:
        ssim, M1, M2, M3 = ssim_grad_maps(x, y)
        sm = ssim_map(x, y)
        l1 = l1_map(x, y).sum()
    elif wrong == "pad":
        H = image.shape[1]
        a, b = max(0, y0 - 5), min(H, y1 + 5)
        lead = image[:, a:y0].to(dtype), image[:, y1:b].to(dtype)
        xe = torch.cat([lead[0], x, lead[1]], dim=1)
        ye = gt_u8[:, a:b].to(dtype) / 255.0
        sl = slice(y0 - a, y0 - a + (y1 - y0))
        ssim, M1, M2, M3 = [t[:, sl] for t in _terms(xe, ye, window_1d().to(dtype), 0.03 ** 2)]
        sm = ssim
        l1 = l1_map(x, y).sum()
    else:
        w1 = window_1d().to(dtype)
        if wrong == "tap":
            w1 = w1.clone()
            w1[-1] = 0.0
        ssim, M1, M2, M3 = _terms(x, y, w1, 0.03 if wrong == "c2" else 0.03 ** 2)
        sm = ssim
        l1 = l1_map(x, y).sum()
    ss = sm.sum()
    grads = []
    for g_l1, g_ssim, s_l1, s_ssim in COEFS:
        (gr,) = torch.autograd.grad(g_l1 * s_l1 * l1 + g_ssim * s_ssim * ss, x, retain_graph=True)
        if wrong == "sign0":
            gr = gr + g_l1 * s_l1 * (x.detach() == y).to(dtype)
        grads.append(gr.detach())
    return dict(l1=l1.detach(), ssim=ss.detach(), M=(M1.detach(), M2.detach(), M3.detach()), grads=grads)


def loss_kernel_order_fp32(image, gt_u8, y0, y1):
    """The HIP forward's own order of operations in float32 on the CPU -- products formed before the taps, separable
    11 + 11 taps accumulated in tap order (horizontal first), exact division in place of v_rcp_f32 -- and the backward's
    (separable convolution of the three maps): -> dict like loss_reference (grads by the kernel's formula)."""
    f = torch.float32
    x = image[:, y0:y1].to(f)
    y = gt_u8[:, y0:y1].to(f) * torch.tensor(1.0 / 255.0, dtype=f)
    w = [float(v) for v in window_1d().to(f)]

    def sep(t):
        C, R, W = t.shape
        p = F.pad(t, (5, 5, 0, 0))
        h = torch.zeros_like(t)
        for k in range(11):
            h = h + p[:, :, k:k + W] * w[k]
        p = F.pad(h, (0, 0, 5, 5))
        v = torch.zeros_like(t)
        for k in range(11):
            v = v + p[:, k:k + R, :] * w[k]
        return v

    mu1, mu2, e11, e22, e12 = sep(x), sep(y), sep(x * x), sep(y * y), sep(x * y)
    C1, C2 = torch.tensor(0.01, dtype=f) ** 2, torch.tensor(0.03, dtype=f) ** 2
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - m11, e22 - m22, e12 - m12
    A, B = 2 * m12 + C1, 2 * s12 + C2
    Cd, Dd = m11 + m22 + C1, s1 + s2 + C2
    inv_d = 1.0 / Dd
    inv = (1.0 / Cd) * inv_d
    ssim = A * B * inv
    M1 = 2 * mu2 * (B - A) * inv - ssim * 2 * mu1 * (Dd - Cd) * inv
    M2 = -ssim * inv_d
    M3 = 2 * A * inv
    d = x - y
    sgn = (d > 0).to(f) - (d < 0).to(f)
    c1, c2, c3 = sep(M1), sep(M2), sep(M3)
    grads = []
    for g_l1, g_ssim, s_l1, s_ssim in COEFS:
        gl1 = torch.tensor(g_l1, dtype=f) * torch.tensor(s_l1, dtype=f)
        gss = torch.tensor(g_ssim, dtype=f) * torch.tensor(s_ssim, dtype=f)
        grads.append(gl1 * sgn + gss * (c1 + 2 * x * c2 + y * c3))
    return dict(l1=d.abs().double().sum(), ssim=ssim.double().sum(), M=(M1, M2, M3), grads=grads)


# ---------------------------------------------------------------------------------------------- Adam
def adam_inputs(n, seed):
    """-> (p, g, m, v) float32 [n]: gradients exactly 0 (every third element) or |g| in [1e-3, 10]; the moments are those of a
    run in progress (v > 0 wherever m != 0), so m / sqrt(v) stays well conditioned"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    mag = torch.exp(torch.rand(n, generator=gen) * (torch.log(torch.tensor(10.0)) - torch.log(torch.tensor(1e-3))) +
                    torch.log(torch.tensor(1e-3))).clamp(1e-3, 10.0)
    sgn = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g = mag * sgn
    g[2::3] = 0.0
    m = 0.1 * torch.randn(n, generator=gen)
    v = m * m * (1.0 + torch.rand(n, generator=gen)) + 1e-6
    return p, g, m, v


def adam_reference(p, g, m, v, lr, b1, b2, eps, step, grad_scale, dtype=torch.float64, wrong=None):
    """One update of gsr_adam1 in `dtype`: lr / bc1, 1 / sqrt(bc2), eps added after the scaling.  wrong="eps_before": eps
    added to sqrt(v) before the 1/sqrt(bc2) scaling; wrong="no_scale": grad_scale forgotten.  -> (p, m, v)"""
    p, g, m, v = [t.to(dtype) for t in (p, g, m, v)]
    if wrong != "no_scale":
        g = g * grad_scale
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    if wrong == "eps_before":
        denom = (v.sqrt() + eps) / bc2 ** 0.5
    else:
        denom = v.sqrt() / bc2 ** 0.5 + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def adam_torch32(p, g, m, v, lr, b1, b2, eps, step, grad_scale):
    """The same update by torch.optim.Adam(foreach=False) in float32 on the CPU -> (p, m, v)"""
    q = p.clone().float().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone().float(), exp_avg_sq=v.clone().float())
    q.grad = g.float() * torch.tensor(grad_scale, dtype=torch.float32)
    opt.step()
    st = opt.state[q]
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


# ---------------------------------------------------------------------------------------------- guard bands
class Guard:
    """A device buffer handed to the C ABI as a slice of a larger allocation: PAD elements of padding on each side (NaN for
    float, 0xA5 bytes otherwise) plus `offset` elements of deliberate misalignment in front.  The slice itself starts as
    padding too (an output element that is never written shows up as NaN); check() proves that the padding -- or, for an
    input, the whole allocation -- is bit-identical after the call."""
    PAD = 256

    def __init__(self, n, dtype, device, offset=0):
        total = n + 2 * self.PAD + offset
        if dtype.is_floating_point:
            self.buf = torch.full((total,), float("nan"), dtype=dtype, device=device)
        else:
            self.buf = torch.empty((total,), dtype=dtype, device=device)
            self.buf.view(torch.uint8).fill_(0xA5)
        self.lo, self.n = self.PAD + offset, n
        self.t = self.buf[self.lo:self.lo + n]
        self.before = None

    @staticmethod
    def _bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t

    def seal(self):
        self.before = self.buf.clone()
        return self

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what, whole=False):
        now, was = self._bits(self.buf), self._bits(self.before)
        if whole:
            assert torch.equal(now, was), f"{what}: an input buffer was written"
            return
        assert torch.equal(now[:self.lo], was[:self.lo]), f"{what}: padding in front of the buffer was written"
        assert torch.equal(now[self.lo + self.n:], was[self.lo + self.n:]), f"{what}: padding behind the buffer was written"

    def untouched(self, mask, what):
        """the elements of the slice selected by `mask` (bool, the slice's shape flattened) still hold their old bits"""
        now, was = self._bits(self.t), self._bits(self.before[self.lo:self.lo + self.n])
        assert torch.equal(now[mask], was[mask]), f"{what}: elements outside the contract were written"
