// mcmc.hip -- the fixed-budget alternative to clone / split / prune: 3DGS-MCMC ("3D Gaussian Splatting as Markov Chain
// Monte Carlo") on the device.  Neither the reference nor its rasterizer has any of it; the formulas are the paper's.
//   gsr_mcmc_relocate_plan : which live row every dead (and every new) row is teleported onto, drawn in proportion to
//                            opacity from an exact integer CDF -- a plain three-launch scan, no look-back, no spin-wait;
//   gsr_mcmc_relocate_apply: rows written IN PLACE; the source's opacity and scale corrected (fp64) so the image stays;
//   gsr_mcmc_noise         : xyz += scaler * gate(1 - opacity) * Sigma * xi, one launch per iteration;
//   gsr_mcmc_normals       : exactly the xi the noise kernel draws;
//   gsr_mcmc_reg_grad      : closed-form gradients of the opacity / scale regulariser, added in place.
// Every row index that came from the device (src[], count[]) is clamped or re-checked before it forms an address.
#include "common.h"

// no FMA contraction in this file: the draw (gsr_mcmc_normals) and its use (gsr_mcmc_noise), and the two phases of the
// apply step, evaluate the same expressions in different kernels and must produce the same bits
#pragma clang fp contract(off)

namespace {
constexpr int MCMC_THREADS = 256;
constexpr int MCMC_ITEMS = 4;
constexpr int MCMC_TILE = MCMC_THREADS * MCMC_ITEMS;  // rows per scan tile
constexpr uint32_t DOMAIN_RELOCATE = 1u, DOMAIN_NOISE = 2u;  // fourth counter word: keeps the two streams apart
constexpr int MCMC_MAX_TENSORS = 32;
constexpr int MCMC_MAX_WIDTH = 4096;
constexpr int APPLY_ROWS = 64, APPLY_THREADS = 256;

// ---------------------------------------------------------------------------------------------- Philox4x32-10
struct U4 {
    uint32_t x, y, z, w;
};

__host__ __device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = U4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// ---------------------------------------------------------------------------------------------- relocation plan
struct RelocLayout {
    size_t prefix, tile_sum, tile_dead, total, bytes;
    long long tiles;
};

RelocLayout reloc_layout(int64_t rows) {
    RelocLayout L;
    L.tiles = (rows + MCMC_TILE - 1) / MCMC_TILE;
    if (L.tiles < 1) L.tiles = 1;
    size_t o = 0;
    L.prefix = o; o += sizeof(uint64_t) * (size_t)(rows > 0 ? rows : 1);
    L.tile_sum = o; o += sizeof(uint64_t) * (size_t)L.tiles;
    L.tile_dead = o; o += sizeof(uint64_t) * (size_t)L.tiles;
    L.total = o; o += sizeof(uint64_t);
    L.bytes = o;
    return L;
}

// a row is dead iff opacity <= min_opacity (a NaN counts as dead: it must never be drawn); a live row weighs
// (uint32)(opacity * 2^24): the product is a power-of-two scaling, the truncation exact.  Opacities above 1 weigh 2^24.
__device__ __forceinline__ bool row_alive(float o, float min_opacity) { return o > min_opacity; }
__device__ __forceinline__ uint32_t row_weight(float o, float min_opacity) {
    if (!row_alive(o, min_opacity)) return 0u;
    return (uint32_t)(fminf(fmaxf(o, 0.0f), 1.0f) * 16777216.0f);
}

// launch 1: per tile of MCMC_TILE rows, the exclusive prefix sums of the weights INSIDE the tile (uint64), the tile's sum
// and its number of dead rows.  Integer sums: the same CDF whatever the association.
__global__ void __launch_bounds__(MCMC_THREADS)
mcmc_tile_prefix_kernel(long long P, const float *__restrict__ opacity, float min_opacity,
                        uint64_t *__restrict__ prefix, uint64_t *__restrict__ tile_sum,
                        uint64_t *__restrict__ tile_dead) {
    __shared__ uint64_t s_w[MCMC_THREADS];
    __shared__ uint32_t s_d[MCMC_THREADS];
    const long long base = (long long)blockIdx.x * MCMC_TILE + (long long)threadIdx.x * MCMC_ITEMS;
    uint32_t w[MCMC_ITEMS];
    uint64_t mine = 0;
    uint32_t dead = 0;
#pragma unroll
    for (int k = 0; k < MCMC_ITEMS; k++) {
        const long long i = base + k;
        w[k] = 0u;
        if (i < P) {
            const float o = opacity[i];
            w[k] = row_weight(o, min_opacity);
            dead += row_alive(o, min_opacity) ? 0u : 1u;
        }
        mine += w[k];
    }
    s_w[threadIdx.x] = mine;
    s_d[threadIdx.x] = dead;
    __syncthreads();
    // Hillis-Steele inclusive scan over the 256 per-thread sums
    for (int off = 1; off < MCMC_THREADS; off <<= 1) {
        uint64_t a = 0;
        uint32_t b = 0;
        if ((int)threadIdx.x >= off) {
            a = s_w[threadIdx.x - off];
            b = s_d[threadIdx.x - off];
        }
        __syncthreads();
        s_w[threadIdx.x] += a;
        s_d[threadIdx.x] += b;
        __syncthreads();
    }
    uint64_t run = s_w[threadIdx.x] - mine;
#pragma unroll
    for (int k = 0; k < MCMC_ITEMS; k++) {
        const long long i = base + k;
        if (i < P) prefix[i] = run;
        run += w[k];
    }
    if (threadIdx.x == MCMC_THREADS - 1) {
        tile_sum[blockIdx.x] = s_w[threadIdx.x];
        tile_dead[blockIdx.x] = s_d[threadIdx.x];
    }
}

// launch 2: ONE workgroup turns the tile sums into exclusive tile offsets (in place) and writes the total weight and
// totals = {n_dead, n_alive}.  tiles = P / 1024: 40 000 words at 40 M rows, off the hot path.
__global__ void __launch_bounds__(MCMC_THREADS)
mcmc_tile_scan_kernel(long long P, long long tiles, uint64_t *__restrict__ tile_sum,
                      const uint64_t *__restrict__ tile_dead, uint64_t *__restrict__ total,
                      int64_t *__restrict__ totals) {
    __shared__ uint64_t s_w[MCMC_THREADS], s_d[MCMC_THREADS];
    uint64_t carry_w = 0, carry_d = 0;
    for (long long t0 = 0; t0 < tiles; t0 += MCMC_THREADS) {
        const long long t = t0 + threadIdx.x;
        const uint64_t w = t < tiles ? tile_sum[t] : 0, d = t < tiles ? tile_dead[t] : 0;
        s_w[threadIdx.x] = w;
        s_d[threadIdx.x] = d;
        __syncthreads();
        for (int off = 1; off < MCMC_THREADS; off <<= 1) {
            uint64_t a = 0, b = 0;
            if ((int)threadIdx.x >= off) {
                a = s_w[threadIdx.x - off];
                b = s_d[threadIdx.x - off];
            }
            __syncthreads();
            s_w[threadIdx.x] += a;
            s_d[threadIdx.x] += b;
            __syncthreads();
        }
        if (t < tiles) tile_sum[t] = carry_w + s_w[threadIdx.x] - w;
        carry_w += s_w[MCMC_THREADS - 1];
        carry_d += s_d[MCMC_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total = carry_w;
        totals[0] = (int64_t)carry_d;
        totals[1] = (int64_t)(P - (long long)carry_d);
    }
}

// launch 3: destination row d (dead, or one of the n_add new rows) makes ONE draw by itself: Philox keyed by the seed,
// counter (d, event, DOMAIN_RELOCATE); r = mulhi64(x0 | x1 << 32, total) in [0, total); the source is the LAST row whose
// exclusive prefix is <= r -- the unique i with prefix[i] <= r < prefix[i] + w_i, since a row of weight 0 shares its
// prefix with the row after it.  Two binary searches: over the tile offsets, then inside the tile.  The result depends
// on (seed, event, d) and the opacities alone, not on the grid.
__global__ void __launch_bounds__(MCMC_THREADS)
mcmc_draw_kernel(long long P, long long n_add, const float *__restrict__ opacity, float min_opacity, uint32_t seed_lo,
                 uint32_t seed_hi, uint32_t event, const uint64_t *__restrict__ prefix,
                 const uint64_t *__restrict__ tile_off, long long tiles, const uint64_t *__restrict__ total_p,
                 int32_t *__restrict__ src, int32_t *__restrict__ count) {
    const long long d = (long long)blockIdx.x * MCMC_THREADS + threadIdx.x;
    if (d >= P + n_add) return;
    const uint64_t total = *total_p;
    const bool dest = d >= P || !row_alive(opacity[d], min_opacity);
    if (!dest || total == 0 || P <= 0) {
        src[d] = -1;
        return;
    }
    const U4 x = philox4x32_10(U4{(uint32_t)d, (uint32_t)((uint64_t)d >> 32), event, DOMAIN_RELOCATE}, seed_lo, seed_hi);
    const uint64_t r = __umul64hi((uint64_t)x.x | ((uint64_t)x.y << 32), total);
    long long lo = 0, hi = tiles - 1;  // last tile whose offset is <= r (tile_off[0] == 0 <= r)
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (tile_off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t rr = r - tile_off[lo];
    const long long first = lo * MCMC_TILE;
    long long a = first, b = first + MCMC_TILE - 1 < P - 1 ? first + MCMC_TILE - 1 : P - 1;
    if (a > b) a = b;
    while (a < b) {
        const long long mid = (a + b + 1) >> 1;
        if (prefix[mid] <= rr) a = mid;
        else b = mid - 1;
    }
    long long i = a;  // in [0, P) by construction; clamped all the same before it is used as an address
    i = i < 0 ? 0 : (i > P - 1 ? P - 1 : i);
    src[d] = (int32_t)i;
    atomicAdd(&count[i], 1);
}

// ---------------------------------------------------------------------------------------------- relocation apply
struct ApplyArgs {
    uint32_t *ptr[MCMC_MAX_TENSORS];
    int32_t width[MCMC_MAX_TENSORS], role[MCMC_MAX_TENSORS];
    int64_t stride[MCMC_MAX_TENSORS];  // in words
};

// What n Gaussians of opacity o' and scale f * s on one spot must be for the image of ONE Gaussian (o, s) to stay
// (the paper's eq. 9, gsplat's compute_relocation), in fp64: the alternating sum cancels by ~100x at o = 0.99, n = 51
// and 1 - (1 - o)^(1/n) loses digits in fp32 for small o.
//   o' = -expm1(log1p(-o) / n),  D = sum_{k=0}^{n-1} C(n,k+1) (-1)^k o'^(k+1) / sqrt(k+1)  (the hockey-stick form of the
//   paper's double sum),  f = o / D.  o' is clamped to [min_opacity, 1 - 2^-23] AFTER D is formed.
// -> the new raw opacity log(o' / (1 - o')) and log(f), each rounded to fp32 once.
__device__ __forceinline__ void relocation_values(float o32, int n, float min_opacity, float &new_opacity_raw,
                                                  float &log_f) {
    const double o = (double)o32;
    double op = -expm1(log1p(-o) / (double)n);
    double D = 0.0, binom = (double)n, pw = op;  // C(n,1), o'^1
    for (int k = 0; k < n; k++) {
        const double term = binom * pw / sqrt((double)(k + 1));
        D += (k & 1) ? -term : term;
        binom = binom * (double)(n - k - 1) / (double)(k + 2);  // C(n,k+2): an exact integer below 2^53 for n <= 51
        pw *= op;
    }
    const double f = o / D;
    const double hi = 1.0 - 1.1920928955078125e-07, lo = (double)min_opacity;
    op = op < lo ? lo : op;
    op = op > hi ? hi : op;
    new_opacity_raw = (float)log(op / (1.0 - op));
    log_f = (float)log(f);
}

// One kernel, two launches, IN PLACE.  Ordering argument for the hazard "many destinations share one source whose
// opacity and scale are overwritten": launch 1 (DEST) writes every destination row and only READS source rows; launch 2
// (SOURCES, same stream, hence after launch 1 has finished) updates the source rows.  Sources are live rows below P,
// destinations are dead rows or rows >= P, so the two sets are disjoint and launch 1 reads nothing that it writes.
// Both launches derive (o', f) from the untouched opacity_act input and count[], through the same function above, so a
// destination's opacity and scale carry its source's new bits.
// A workgroup takes APPLY_ROWS consecutive rows: one thread per row decides and evaluates the fp64 correction (LDS),
// then for every tensor one thread per 4-byte word of the active rows.  Most groups have no active row and leave after
// reading src[] / count[].
template <bool DEST>
__global__ void __launch_bounds__(APPLY_THREADS)
mcmc_apply_kernel(long long P, long long n_add, const int32_t *__restrict__ src, const int32_t *__restrict__ count,
                  const float *__restrict__ opacity, float min_opacity, int n_max, int num_tensors, ApplyArgs a) {
    __shared__ long long s_from[APPLY_ROWS];
    __shared__ float s_op[APPLY_ROWS], s_logf[APPLY_ROWS];
    __shared__ int s_any;
    const long long rows = DEST ? P + n_add : P;
    const long long base = (long long)blockIdx.x * APPLY_ROWS;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    if (threadIdx.x < APPLY_ROWS) {
        const long long d = base + threadIdx.x;
        long long from = -1;
        float nop = 0.f, lf = 0.f;
        if (d < rows) {
            if (DEST) {
                // a destination is re-derived from the opacities, not taken on src[]'s word: a live row is never written
                const bool dest = d >= P || !row_alive(opacity[d], min_opacity);
                long long s = src[d];
                if (dest && s >= 0) {
                    s = s > P - 1 ? P - 1 : s;  // clamped into [0, P) before it is an address
                    if (row_alive(opacity[s], min_opacity)) from = s;
                }
            } else if (count[d] > 0 && row_alive(opacity[d], min_opacity)) {
                from = d;
            }
            if (from >= 0) {
                long long c = count[from];
                c = c < 0 ? 0 : c;
                const int n = (int)(c + 1 < (long long)n_max ? c + 1 : (long long)n_max);
                relocation_values(opacity[from], n, min_opacity, nop, lf);
                s_any = 1;
            }
        }
        s_from[threadIdx.x] = from;
        s_op[threadIdx.x] = nop;
        s_logf[threadIdx.x] = lf;
    }
    __syncthreads();
    if (!s_any) return;
    const int nrows = (int)(rows - base < APPLY_ROWS ? rows - base : APPLY_ROWS);
    for (int k = 0; k < num_tensors; k++) {
        const int role = a.role[k];
        if (!DEST && role == GSR_MCMC_ROLE_COPY) continue;  // a source keeps everything but opacity, scale and moments
        const uint32_t w = (uint32_t)a.width[k];
        uint32_t *__restrict__ p = a.ptr[k];
        const int64_t st = a.stride[k];
        const uint32_t total = (uint32_t)nrows * w;
        for (uint32_t t = threadIdx.x; t < total; t += APPLY_THREADS) {
            const uint32_t r = t / w, col = t - r * w;
            const long long from = s_from[r];
            if (from < 0) continue;
            uint32_t v;
            if (role == GSR_MCMC_ROLE_MOMENT) v = 0u;
            else if (role == GSR_MCMC_ROLE_OPACITY) v = __float_as_uint(s_op[r]);
            else if (role == GSR_MCMC_ROLE_SCALING) v = __float_as_uint(__uint_as_float(p[from * st + col]) + s_logf[r]);
            else v = p[from * st + col];
            p[(base + r) * st + col] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------- position noise
// xi of row `row` at `step`: Philox keyed by the seed, counter (row, step, DOMAIN_NOISE); Box-Muller on
// u = ((x >> 8) + 0.5) * 2^-24.  In fp32 the sum (x >> 8) + 0.5 rounds for the upper half of the range, so u lies in
// [2^-25, 1]: u = 1 gives radius 0, never inf or NaN; the largest radius is sqrt(50 ln 2) = 5.89.  The hardware
// v_cos_f32 / v_sin_f32 take their argument in revolutions, which u already is.
__device__ __forceinline__ float unit24(uint32_t x) { return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-08f; }
__device__ __forceinline__ void draw_normals(long long row, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, float &z0,
                                             float &z1, float &z2) {
    const U4 x = philox4x32_10(U4{(uint32_t)row, (uint32_t)((uint64_t)row >> 32), step, DOMAIN_NOISE}, seed_lo, seed_hi);
    // -2 ln u = -2 ln 2 * log2 u
    const float r0 = __fsqrt_rn(-1.3862943611198906f * __builtin_amdgcn_logf(unit24(x.x)));
    const float r1 = __fsqrt_rn(-1.3862943611198906f * __builtin_amdgcn_logf(unit24(x.z)));
    const float a0 = unit24(x.y), a1 = unit24(x.w);
    z0 = r0 * __builtin_amdgcn_cosf(a0);
    z1 = r0 * __builtin_amdgcn_sinf(a0);
    z2 = r1 * __builtin_amdgcn_cosf(a1);
}

__global__ void __launch_bounds__(MCMC_THREADS)
mcmc_normals_kernel(long long n, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, float *__restrict__ out) {
    __shared__ float s[MCMC_THREADS * 3];
    const long long base = (long long)blockIdx.x * MCMC_THREADS;
    const int nrows = (int)(n - base < MCMC_THREADS ? n - base : MCMC_THREADS);
    if ((int)threadIdx.x < nrows)
        draw_normals(base + threadIdx.x, seed_lo, seed_hi, step, s[threadIdx.x * 3], s[threadIdx.x * 3 + 1],
                     s[threadIdx.x * 3 + 2]);
    __syncthreads();
    for (int t = threadIdx.x; t < nrows * 3; t += MCMC_THREADS) out[base * 3 + t] = s[t];
}

// One lane per row, MCMC_THREADS rows per workgroup.  The 12-byte rows (xyz, scale, xi) go through LDS so that global
// loads and the store are consecutive dwords across the workgroup (a lane's three LDS words are 3 apart: no bank
// conflict); the quaternion is one 16-byte load per lane, the opacity one dword.  44 B read (56 with a caller's xi) and
// 12 B written per row, no scratch.
//   xyz += scaler * g * R (s^2 .* (R^T xi)),  R = R(q / max(|q|, 1e-12)),  s = exp(scaling_raw),
//   g = 1 / (1 + exp(-100 (x - 0.995))),  x = 1 - sigmoid(opacity_raw) evaluated as 1 / (1 + exp(opacity_raw)), which
//   keeps its relative accuracy where x is small.
template <bool HAVE_XI>
__global__ void __launch_bounds__(MCMC_THREADS)
mcmc_noise_kernel(long long P, float *__restrict__ xyz, const float *__restrict__ scaling,
                  const float4 *__restrict__ rotation, const float *__restrict__ opacity, float scaler,
                  const float *__restrict__ xi, uint32_t seed_lo, uint32_t seed_hi, uint32_t step) {
    __shared__ float s_xyz[MCMC_THREADS * 3], s_sc[MCMC_THREADS * 3], s_xi[HAVE_XI ? MCMC_THREADS * 3 : 1];
    const long long base = (long long)blockIdx.x * MCMC_THREADS;
    const int nrows = (int)(P - base < MCMC_THREADS ? P - base : MCMC_THREADS);
    for (int t = threadIdx.x; t < nrows * 3; t += MCMC_THREADS) {
        s_xyz[t] = xyz[base * 3 + t];
        s_sc[t] = scaling[base * 3 + t];
        if (HAVE_XI) s_xi[t] = xi[base * 3 + t];
    }
    __syncthreads();
    if ((int)threadIdx.x < nrows) {
        const long long i = base + threadIdx.x;
        const float4 q = rotation[i];
        const float x1m = 1.0f / (1.0f + expf(opacity[i]));
        const float g = 1.0f / (1.0f + expf(-100.0f * (x1m - 0.995f)));
        float z0, z1, z2;
        if (HAVE_XI) {
            z0 = s_xi[threadIdx.x * 3];
            z1 = s_xi[threadIdx.x * 3 + 1];
            z2 = s_xi[threadIdx.x * 3 + 2];
        } else {
            draw_normals(i, seed_lo, seed_hi, step, z0, z1, z2);
        }
        const float inv = 1.0f / fmaxf(__fsqrt_rn(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
        const float w = q.x * inv, x = q.y * inv, y = q.z * inv, z = q.w * inv;
        const float r00 = 1.0f - 2.0f * (y * y + z * z), r01 = 2.0f * (x * y - w * z), r02 = 2.0f * (x * z + w * y);
        const float r10 = 2.0f * (x * y + w * z), r11 = 1.0f - 2.0f * (x * x + z * z), r12 = 2.0f * (y * z - w * x);
        const float r20 = 2.0f * (x * z - w * y), r21 = 2.0f * (y * z + w * x), r22 = 1.0f - 2.0f * (x * x + y * y);
        const float e0 = expf(s_sc[threadIdx.x * 3]), e1 = expf(s_sc[threadIdx.x * 3 + 1]),
                    e2 = expf(s_sc[threadIdx.x * 3 + 2]);
        const float t0 = e0 * e0 * (r00 * z0 + r10 * z1 + r20 * z2);
        const float t1 = e1 * e1 * (r01 * z0 + r11 * z1 + r21 * z2);
        const float t2 = e2 * e2 * (r02 * z0 + r12 * z1 + r22 * z2);
        const float sg = scaler * g;
        s_xyz[threadIdx.x * 3] += sg * (r00 * t0 + r01 * t1 + r02 * t2);
        s_xyz[threadIdx.x * 3 + 1] += sg * (r10 * t0 + r11 * t1 + r12 * t2);
        s_xyz[threadIdx.x * 3 + 2] += sg * (r20 * t0 + r21 * t1 + r22 * t2);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nrows * 3; t += MCMC_THREADS) xyz[base * 3 + t] = s_xyz[t];
}

// ---------------------------------------------------------------------------------------------- regulariser
// d/d raw of  c_o * sum sigmoid(opacity_raw) + c_s * sum exp(scaling_raw):  c_o * o (1 - o)  and  c_s * exp(s); one
// thread per scale element, the first P of them take an opacity element too.
__global__ void __launch_bounds__(MCMC_THREADS)
mcmc_reg_grad_kernel(long long P, const float *__restrict__ opacity, const float *__restrict__ scaling, float c_opacity,
                     float c_scale, float *__restrict__ grad_opacity, float *__restrict__ grad_scaling) {
    const long long t = (long long)blockIdx.x * MCMC_THREADS + threadIdx.x;
    if (t >= 3 * P) return;
    grad_scaling[t] += c_scale * expf(scaling[t]);
    if (t < P) {
        const float o = 1.0f / (1.0f + expf(-opacity[t]));
        grad_opacity[t] += c_opacity * (o * (1.0f - o));
    }
}

constexpr long long MCMC_MAX_ROWS = 0x7fffffffLL;  // src[] / count[] are int32
}  // namespace

extern "C" size_t gsr_mcmc_relocate_bytes(int64_t rows) {
    if (rows < 0 || rows > MCMC_MAX_ROWS) return 0;
    return reloc_layout(rows).bytes;
}

extern "C" int gsr_mcmc_relocate_plan(int64_t P, int64_t n_add, const float *opacity_act, float min_opacity,
                                      uint64_t seed, uint32_t event, int32_t *src, int32_t *count, int64_t *totals,
                                      void *workspace, size_t workspace_bytes, gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (P < 0 || n_add < 0 || P > MCMC_MAX_ROWS || n_add > MCMC_MAX_ROWS || P + n_add > MCMC_MAX_ROWS) return GSR_EINVAL;
    if (!(min_opacity >= 0.0f)) return GSR_EINVAL;
    if (P == 0) return 0;  // nothing to draw from: no launch, nothing is written
    if (!opacity_act || !src || !count || !totals || !workspace) return GSR_EINVAL;
    const RelocLayout L = reloc_layout(P);
    if (workspace_bytes < L.bytes) return GSR_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return GSR_EINVAL;
    char *base = reinterpret_cast<char *>(workspace);
    uint64_t *prefix = reinterpret_cast<uint64_t *>(base + L.prefix);
    uint64_t *tile_sum = reinterpret_cast<uint64_t *>(base + L.tile_sum);
    uint64_t *tile_dead = reinterpret_cast<uint64_t *>(base + L.tile_dead);
    uint64_t *total = reinterpret_cast<uint64_t *>(base + L.total);
    GSR_HIP(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)P, stream));
    hipLaunchKernelGGL(mcmc_tile_prefix_kernel, dim3((unsigned)L.tiles), dim3(MCMC_THREADS), 0, stream, (long long)P,
                       opacity_act, min_opacity, prefix, tile_sum, tile_dead);
    hipLaunchKernelGGL(mcmc_tile_scan_kernel, dim3(1), dim3(MCMC_THREADS), 0, stream, (long long)P, L.tiles, tile_sum,
                       tile_dead, total, totals);
    const long long rows = P + n_add;
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3((unsigned)((rows + MCMC_THREADS - 1) / MCMC_THREADS)), dim3(MCMC_THREADS),
                       0, stream, (long long)P, (long long)n_add, opacity_act, min_opacity, (uint32_t)seed,
                       (uint32_t)(seed >> 32), event, prefix, tile_sum, L.tiles, total, src, count);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_mcmc_relocate_apply(int64_t P, int64_t n_add, const int32_t *src, const int32_t *count,
                                       const float *opacity_act, float min_opacity, int n_max, int num_tensors,
                                       void *const *tensors, const int32_t *widths, const int64_t *strides,
                                       const int32_t *roles, gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (P < 0 || n_add < 0 || P > MCMC_MAX_ROWS || n_add > MCMC_MAX_ROWS || P + n_add > MCMC_MAX_ROWS) return GSR_EINVAL;
    if (n_max < 1 || n_max > GSR_MCMC_N_MAX || num_tensors < 0 || num_tensors > MCMC_MAX_TENSORS) return GSR_EINVAL;
    if (!(min_opacity >= 0.0f)) return GSR_EINVAL;
    if (P == 0 || num_tensors == 0) return 0;
    if (!src || !count || !opacity_act || !tensors || !widths || !strides || !roles) return GSR_EINVAL;
    ApplyArgs a{};
    for (int k = 0; k < num_tensors; k++) {
        if (!tensors[k] || widths[k] <= 0 || widths[k] > MCMC_MAX_WIDTH || strides[k] < widths[k]) return GSR_EINVAL;
        switch (roles[k]) {
        case GSR_MCMC_ROLE_COPY:
        case GSR_MCMC_ROLE_MOMENT:
            break;
        case GSR_MCMC_ROLE_OPACITY:
            if (widths[k] != 1) return GSR_EINVAL;
            break;
        case GSR_MCMC_ROLE_SCALING:
            if (widths[k] != 3) return GSR_EINVAL;
            break;
        default:
            return GSR_EINVAL;
        }
        a.ptr[k] = reinterpret_cast<uint32_t *>(tensors[k]);
        a.width[k] = widths[k];
        a.role[k] = roles[k];
        a.stride[k] = strides[k];
    }
    const long long rows = P + n_add;
    hipLaunchKernelGGL(mcmc_apply_kernel<true>, dim3((unsigned)((rows + APPLY_ROWS - 1) / APPLY_ROWS)),
                       dim3(APPLY_THREADS), 0, stream, (long long)P, (long long)n_add, src, count, opacity_act,
                       min_opacity, n_max, num_tensors, a);
    hipLaunchKernelGGL(mcmc_apply_kernel<false>, dim3((unsigned)((P + APPLY_ROWS - 1) / APPLY_ROWS)),
                       dim3(APPLY_THREADS), 0, stream, (long long)P, (long long)n_add, src, count, opacity_act,
                       min_opacity, n_max, num_tensors, a);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_mcmc_normals(int64_t n, uint64_t seed, uint32_t step, float *out, gsr_stream_t stream_) {
    if (n < 0 || n > MCMC_MAX_ROWS) return GSR_EINVAL;
    if (n == 0) return 0;
    if (!out) return GSR_EINVAL;
    hipLaunchKernelGGL(mcmc_normals_kernel, dim3((unsigned)((n + MCMC_THREADS - 1) / MCMC_THREADS)),
                       dim3(MCMC_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), (long long)n, (uint32_t)seed,
                       (uint32_t)(seed >> 32), step, out);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_mcmc_noise(int64_t P, float *xyz, const float *scaling_raw, const float *rotation_raw,
                              const float *opacity_raw, float scaler, const float *xi, uint64_t seed, uint32_t step,
                              gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (P < 0 || P > MCMC_MAX_ROWS) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!xyz || !scaling_raw || !rotation_raw || !opacity_raw) return GSR_EINVAL;
    if (reinterpret_cast<uintptr_t>(rotation_raw) & 15) return GSR_EINVAL;  // one 16-byte load per quaternion
    const dim3 grid((unsigned)((P + MCMC_THREADS - 1) / MCMC_THREADS)), block(MCMC_THREADS);
    const float4 *rot = reinterpret_cast<const float4 *>(rotation_raw);
    if (xi)
        hipLaunchKernelGGL(mcmc_noise_kernel<true>, grid, block, 0, stream, (long long)P, xyz, scaling_raw, rot,
                           opacity_raw, scaler, xi, 0u, 0u, 0u);
    else
        hipLaunchKernelGGL(mcmc_noise_kernel<false>, grid, block, 0, stream, (long long)P, xyz, scaling_raw, rot,
                           opacity_raw, scaler, xi, (uint32_t)seed, (uint32_t)(seed >> 32), step);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_mcmc_reg_grad(int64_t P, const float *opacity_raw, const float *scaling_raw, float c_opacity,
                                 float c_scale, float *grad_opacity, float *grad_scaling, gsr_stream_t stream_) {
    if (P < 0 || P > MCMC_MAX_ROWS) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!opacity_raw || !scaling_raw || !grad_opacity || !grad_scaling) return GSR_EINVAL;
    hipLaunchKernelGGL(mcmc_reg_grad_kernel, dim3((unsigned)((3 * P + MCMC_THREADS - 1) / MCMC_THREADS)),
                       dim3(MCMC_THREADS), 0, reinterpret_cast<hipStream_t>(stream_), (long long)P, opacity_raw,
                       scaling_raw, c_opacity, c_scale, grad_opacity, grad_scaling);
    GSR_LAUNCH_CHECK();
    return 0;
}
