"""numpy / Python-int restatements of csrc/mcmc.hip (3DGS-MCMC relocation, position noise, regulariser), shared by
test_mcmc_refs_cpu.py and test_gpu_mcmc.py.  Integers are exact (Python ints, uint64 arrays); the relocation formulas are
evaluated with 60 decimal digits and the double sum of the paper with exact integer binomials (math.comb); everything
else is fp64."""
import math
from decimal import Decimal, getcontext

import numpy as np

DOMAIN_RELOCATE, DOMAIN_NOISE = 1, 2
M32 = 0xFFFFFFFF
U = 2.0 ** -24  # unit roundoff of fp32: |fl(x) - x| <= U |x|


# ------------------------------------------------------------------------------------------------ Philox4x32-10
def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (Python ints) -> 4 words"""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox_rows(rows, third, domain, seed):
    """the four words of counter (row low, row high, third, domain) under key (seed low, seed high), for an array of
    rows: uint64 arrays [4, n]"""
    rows = np.asarray(rows, dtype=np.uint64)
    m = np.uint64(M32)
    c = [rows & m, rows >> np.uint64(32), np.full_like(rows, int(third) & M32), np.full_like(rows, int(domain))]
    k0, k1 = np.uint64(int(seed) & M32), np.uint64((int(seed) >> 32) & M32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return np.stack(c)


# ------------------------------------------------------------------------------------------------ relocation plan
def weights(opacity, min_opacity):
    """-> (w uint64 [P], dead bool [P]): dead iff opacity <= min_opacity (both fp32); w = (uint32)(opacity * 2^24)"""
    o = np.asarray(opacity, dtype=np.float32)
    dead = ~(o > np.float32(min_opacity))
    w = (np.clip(o, 0, 1).astype(np.float64) * 16777216.0).astype(np.uint64)  # exact: a power-of-two scaling, truncated
    w[dead] = 0
    return w, dead


def draw(prefix, total, x0, x1):
    """the row drawn by the Philox words (x0, x1): r = mulhi64(x0 | x1 << 32, total), the unique i with
    prefix[i] <= r < prefix[i] + w[i] = the last i whose exclusive prefix is <= r"""
    r = ((int(x0) | (int(x1) << 32)) * int(total)) >> 64
    return int(np.searchsorted(prefix, np.uint64(r), side="right")) - 1


def relocate_plan(opacity, n_add, min_opacity, seed, event):
    """-> (src int32 [P+n_add], count int32 [P], (n_dead, n_alive))"""
    w, dead = weights(opacity, min_opacity)
    P = w.shape[0]
    prefix = np.concatenate([np.zeros(1, np.uint64), np.cumsum(w, dtype=np.uint64)])[:P]
    total = int(w.sum(dtype=np.uint64))
    src = np.full(P + n_add, -1, dtype=np.int32)
    count = np.zeros(P, dtype=np.int32)
    dests = np.concatenate([np.nonzero(dead)[0], np.arange(P, P + n_add)]).astype(np.int64)
    if total > 0 and dests.size:
        x = philox_rows(dests, event, DOMAIN_RELOCATE, seed)
        for d, x0, x1 in zip(dests, x[0], x[1]):
            i = draw(prefix, total, x0, x1)
            src[d] = i
            count[i] += 1
    return src, count, (int(dead.sum()), int(P - dead.sum()))


# ------------------------------------------------------------------------------------------------ relocation values
def _dec(x):
    return Decimal(float(x))


def relocation(o, n, min_opacity):
    """What n Gaussians on one spot must be for the image of one Gaussian of opacity o (an fp32 value) to stay:
        o' = 1 - (1 - o)^(1/n),  D = sum_{i=1..n} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1),  f = o / D,
    o' then clamped to [min_opacity, 1 - 2^-23].  60 digits.  Returns a dict of floats: o_new (clamped), o_raw (unclamped),
    D, f, logit (of the clamped o'), log_f, and what the error bounds of the fp64 device evaluation need: `cond_D` =
    sum_k |single-sum term_k| * (9 k + n + 13) / |D| (the fp64 roundings of term k: k multiplications behind o'^(k+1),
    product, root, quotient, the sum's n roundings; and the 8 ulp of o' itself, which enter term k (k+1)-fold)."""
    getcontext().prec = 60
    o, n = _dec(np.float32(o)), int(n)
    one = Decimal(1)
    op = one - ((one - o).ln() / n).exp() if o < one else one
    pw = [op ** (k + 1) / Decimal(k + 1).sqrt() for k in range(n)]
    D = sum(sum(math.comb(i - 1, k) * (-1) ** k * pw[k] for k in range(i)) for i in range(1, n + 1))
    cond = sum(math.comb(n, k + 1) * pw[k] * (9 * k + n + 13) for k in range(n)) / abs(D)
    f = o / D
    lo, hi = _dec(np.float32(min_opacity)), one - Decimal(2) ** -23
    oc = min(max(op, lo), hi)
    return {"o_new": float(oc), "o_raw": float(op), "D": float(D), "f": float(f), "logit": float((oc / (one - oc)).ln()),
            "log_f": float(f.ln()), "cond_D": float(cond)}


def single_sum_D(o_new, n):
    """the hockey-stick form the kernel evaluates: sum_{k=0..n-1} C(n,k+1) (-1)^k o'^(k+1) / sqrt(k+1), 60 digits"""
    getcontext().prec = 60
    op = _dec(o_new)
    return sum(math.comb(n, k + 1) * (-1) ** k * op ** (k + 1) / Decimal(k + 1).sqrt() for k in range(n))


def double_sum_D(o_new, n):
    getcontext().prec = 60
    op = _dec(o_new)
    pw = [op ** (k + 1) / Decimal(k + 1).sqrt() for k in range(n)]
    return sum(sum(math.comb(i - 1, k) * (-1) ** k * pw[k] for k in range(i)) for i in range(1, n + 1))


# ------------------------------------------------------------------------------------------------ position noise
def rotation_matrix(q):
    """R(q / max(|q|, 1e-12)) [P,3,3] in fp64, the reference's build_rotation"""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def noise(xyz, scaling_raw, rotation_raw, opacity_raw, scaler, xi):
    """fp64: xyz + scaler * g(1 - sigmoid(opacity_raw)) * Sigma xi, and the per-element error bound of the fp32 kernel.

    Bound, with u = 2^-24 and the kernel's order of operations (x = 1 / (1 + exp(opacity_raw)), E = -100 (x - 0.995f),
    g = 1 / (1 + exp(E)), v = R (s^2 .* (R^T xi)), out = xyz + (scaler g) v):
      * x carries 4 u relative (exp 2 u, add, divide); 0.995f is 2^-25 off; the difference rounds by u |x - 0.995|;
        THE GATE'S SLOPE multiplies all of it by 100, and E rounds once more:
            dE = 100 (4 u x + u / 2 + u |x - 0.995|) + u |E|
        g = 1 / (1 + exp(E)) then carries dE + 4 u relative (exp 2 u, add, divide; d ln g / dE = -(1 - g), at most 1).
        Beyond E = 80, g is below 2^-115 and exp(E) approaches the fp32 overflow: the whole displacement is allowed.
      * every entry of R is within 32 u (absolute) of the exact one: the four normalised components carry 5 u each
        (three roundings of the norm's sum of squares halved by the root, the root, the reciprocal, the product), an
        entry is 1 - 2 (a a + b b) or 2 (a b +- c d) of such components, at most 1 in magnitude: 2 (2 * 5 u + u) + 3 u
        and a doubling, rounded up.
      * t_j = e_j^2 (R^T xi)_j: the dot is off by (32 u + 3 u) |xi|_1, e_j^2 carries 5 u, the product u;
        v_c = sum_j R_cj t_j adds 32 u |t|_1 and three more roundings; with |t_j| <= e_j^2 |xi|_1 and S = sum_j e_j^2:
            dv <= (2 * 32 + 12) u S |xi|_1 = 76 u S |xi|_1
      * scaler * g and its product with v_c round once each, the final add once, RELATIVE TO THE NEW POSITION:
            bound_c = |scaler| g (76 u S |xi|_1 + |v_c| (dE + 6 u)) + u |out_c|
    Returns (out [P,3], bound [P,3], displacement [P,3])."""
    xyz, s = np.asarray(xyz, dtype=np.float64), np.asarray(scaling_raw, dtype=np.float64)
    op, xi = np.asarray(opacity_raw, dtype=np.float64).reshape(-1), np.asarray(xi, dtype=np.float64)
    x = 1.0 / (1.0 + np.exp(op))
    E = -100.0 * (x - 0.995)
    g = 1.0 / (1.0 + np.exp(E))
    R = rotation_matrix(rotation_raw)
    e2 = np.exp(2.0 * s)
    t = e2 * np.einsum("pjc,pj->pc", R, xi)
    v = np.einsum("pcj,pj->pc", R, t)
    disp = scaler * g[:, None] * v
    out = xyz + disp
    dE = 100.0 * (4 * U * x + U / 2 + U * np.abs(x - 0.995)) + U * np.abs(E)
    S, xi1 = e2.sum(axis=1), np.abs(xi).sum(axis=1)
    bound = abs(scaler) * g[:, None] * (76 * U * (S * xi1)[:, None] + np.abs(v) * (dE + 6 * U)[:, None]) + U * np.abs(out)
    bound = np.where((E > 80.0)[:, None], bound + np.abs(disp), bound)
    return out, bound, disp


# ------------------------------------------------------------------------------------------------ regulariser
def reg_grads(opacity_raw, scaling_raw, c_opacity, c_scale):
    """fp64 gradients of c_opacity * sum(sigmoid(opacity_raw)) + c_scale * sum(exp(scaling_raw))"""
    op, s = np.asarray(opacity_raw, dtype=np.float64), np.asarray(scaling_raw, dtype=np.float64)
    o = 1.0 / (1.0 + np.exp(-op))
    return c_opacity * o * (1.0 - o), c_scale * np.exp(s)
