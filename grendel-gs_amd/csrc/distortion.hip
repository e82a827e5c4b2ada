// distortion.hip -- the DEPTH DISTORTION term of Mip-NeRF 360 / 2DGS of one rendered view from the tile lists, and its
// backward (gfx950 / wave64).
//
// A side pass in the shape of tile_walk.h.  Per pixel p, over what K8 blended (w = alpha T),
//     D[p] = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2,        m = c0 + c1 depth + c2 / depth  (three host scalars),
// which is quadratic in the weights: no feature map expresses it.  m is formed once per staged entry in stage_chunk's
// word(id) callback and rides in q1.w of the record; inert slots carry 0.  (0, 1, 0) is the view-space depth, (0, 0, 1)
// the inverse depth, (far / (far - near), 0, -far near / (far - near)) the NDC mapping of 2DGS.  K8 / K10 and the other
// side passes are untouched; a trainer that does not ask for the term never launches these.
//
// Forward (composite_distortion_kernel): front to back from T = 1, each pixel carries T, A, mu, S, D in registers --
// A = sum w, mu = the weighted mean of m, S = the weighted CENTRED second moment, by West's update:
//     d = m - mu;  D += w (A d^2 + S);  A' = A + w;  r = w > 0 ? w / A' : 0;  mu' = mu + r d;  S += w d (m - mu').
// A d^2 + S is sum_{j<i} w_j (m_i - m_j)^2 about the running mean.  Raw sums (sum w m, sum w m^2) cancel
// catastrophically once a pixel's depth spread is small against the depth itself -- the state the regulariser drives
// towards -- and are not used.  w / A' is a correctly rounded division: on a pixel's first entry it is exactly 1, mu is
// exactly m and S stays exactly 0 (a pixel that blends one entry has D = S = 0 and passes no gradient on); A' >= w > 0
// wherever it is formed, and r is SELECTED on w > 0, so a pixel that has blended nothing never sees 0 / 0.  One store
// per pixel and map at the end into [4, H, W] = (D, A, mu, S); the maps are cleared by a fill in front of the launch, so pixels of tiles that are not
// ours or outside the band are +0 and the bands of several ranks assemble by SUM.
// (LDS: the inverse-depth forward's two-quad slab, 4 x (64 + CB) x 2 float4 = 9.0 KiB per workgroup; 94 VGPRs, five
// waves per SIMD -- the inverse-depth forward has 86 and five.)
//
// Backward (composite_distortion_backward_kernel): K10's chain, back to front from final_T, with ONE scalar recurrence.
// With the pixel's totals (A, mu, S) read from the forward's maps and g = dL/dD[p], the "colour" of entry i on this
// pixel is e = dD/dw_i = A (m - mu)^2 + S (= sum_j w_j (m_i - m_j)^2: it differs from pixel to pixel), and
//     Tn = T / (1 - alpha);  dot = e - rho;  q = alpha_raw g Tn dot (dL/dpower; the 0.99 clamp is the identity as in K10);
//     u = 2 g alpha Tn A (m - mu) (dL/dm of the pair);  rho = fma(alpha, dot, rho);  T = Tn.
// A lane that does not take an entry runs this with alpha = 0 and stores (0, 0).  (q, u) go through tile_walk.h's
// wave-private [slot][pixel] transpose; phase B (lane = (slot, row)) forms sum q, sum q dx, sum q dx^2, sum u over its row
// in pixel order, the dy moments as products, three xor steps combine the rows, and lane k < 7 of a slot adds value k of
// [means2D 2 | conic 3 | opacity | m] into the caller's fp64 sums [P,7].  Entries no pixel of the quadrant blends issue
// nothing.  The prologue and the pair decision are spelled out as in composite_invdepth_backward_kernel, whose body
// this one shares but for phase A's terms (the helpers measured slower there; EXPERIMENTS.md, 2026-11-26).
// (LDS: 4.1 KiB matrix + 3.7 KiB slab and ids per wave, 31.1 KiB per workgroup -- five workgroups per CU of its 160 KiB;
// 73 VGPRs, five waves per SIMD = five workgroups, so neither bounds the other.  Figures from the compiler's resource
// report, as the inverse-depth backward's 31.1 KiB and 78.)
// distortion_record_kernel then rounds each fp64 sum once into the fp32 record [P,7]; column 6 becomes dL/ddepth =
// (c1 - c2 / depth^2) sum u in fp64 first; rows blended nowhere are +0.0f.  gsr_depth_backward_means3d (invdepth.hip)
// carries column 6 on into xyz.
#include "common.h"
#include "composite_math.h"
#include "tile_walk.h"

namespace {

__global__ void __launch_bounds__(256)
composite_distortion_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                            const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                            const float4 *__restrict__ conic_opacity, const float *__restrict__ depths,
                            const uint8_t *__restrict__ compute_locally, const int32_t *__restrict__ n_contrib,
                            float c0, float c1, float c2, int band, int band_first, int band_tiles,
                            float *__restrict__ maps) {
    Quadrant qd;
    if (!quadrant_begin(qd, W, H, gx, tiles, ranges, compute_locally, n_contrib, band, band_first, band_tiles)) return;

    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * 2];  // [wave][slot]: {x, y, a2, b2 | c2, o, position + 1, m}
    float4 *wslab = slab[qd.wave];
    float T = 1.0f, A = 0.f, mu = 0.f, S = 0.f, D = 0.f;
    for (int c = 0; c < qd.wlen; c += 64) {  // wave-uniform
        const int nrel = stage_chunk<FRONT_TO_BACK, 2>(
            c, qd.lane, qd.wlen, qd.range.x, qd.qx0, qd.qy0, point_list, means2D, conic_opacity, wslab,
            [&](uint32_t id) {
                const float z = depths[id];
                return c0 + c1 * z + c2 / z;
            },
            [](int, uint32_t) {}, [](int) {});  // (inert: m = 0)
        __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
        for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const float4 q0 = wslab[2 * (b0 + s)], q1 = wslab[2 * (b0 + s) + 1];  // wave-uniform address: LDS broadcasts
                const Pair p = pair_decision(q0, q1, qd.pxf, qd.pyf, qd.last);
                const float w = p.take ? p.alpha * T : 0.f;  // (selected, never multiplied: an inert slot's alpha is not used)
                T -= w;  // T (1 - alpha) as K8 forms it: T - alpha T
                // West's update; with w = 0 every line leaves its register as it was
                const float m = q1.w;
                const float d = m - mu;
                D = fmaf(w, fmaf(A * d, d, S), D);
                A += w;
                const float r = w > 0.f ? w / A : 0.f;  // (A >= w > 0 where the quotient is formed; exactly 1 on the first entry)
                mu = fmaf(r, d, mu);
                S = fmaf(w * d, m - mu, S);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
    }
    if (qd.inside) {
        const size_t hw = (size_t)W * H;
        maps[qd.pid] = D;
        maps[hw + qd.pid] = A;
        maps[2 * hw + qd.pid] = mu;
        maps[3 * hw + qd.pid] = S;
    }
}

__global__ void __launch_bounds__(256)
composite_distortion_backward_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                                     const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                                     const float4 *__restrict__ conic_opacity, const float *__restrict__ depths,
                                     const uint8_t *__restrict__ compute_locally, const int32_t *__restrict__ n_contrib,
                                     float c0, float c1, float c2, const float *__restrict__ final_T,
                                     const float *__restrict__ maps, const float *__restrict__ dL_dD, int band,
                                     int band_first, int band_tiles, double *__restrict__ acc64) {
    // tile_walk.h's quadrant_begin, spelled out as in composite_invdepth_backward_kernel (measured slower through the helper)
    const int tile = side_pass_tile_of_block(ranges, gx, tiles, band, band_first, band_tiles);
    if (tile < 0 || !compute_locally[tile]) return;  // (no workgroup barrier below: waves leave on their own)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx = tile % gx, ty = tile / gx;
    const int qx0 = tx * GSR_BLOCK_X + (wave & 1) * 8, qy0 = ty * GSR_BLOCK_Y + (wave >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const size_t pid = (size_t)py * W + px;
    const int2 range = ranges[tile];
    const int n = range.y - range.x;
    const float pxf = (float)px, pyf = (float)py;
    const int last = inside ? min(n_contrib[pid], n) : 0;
    int wlen = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wlen = max(wlen, __shfl_xor(wlen, d, 64));
    if (wlen <= 0) return;
    const size_t hw = (size_t)W * H;
    const float g = inside ? dL_dD[pid] : 0.f;
    // the pixel's totals: e = At (m - mut)^2 + St is the entry's "colour" on this pixel
    const float At = inside ? maps[hw + pid] : 0.f, mut = inside ? maps[2 * hw + pid] : 0.f;
    const float St = inside ? maps[3 * hw + pid] : 0.f;
    const float gA2 = 2.f * g * At;
    const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;

    // [wave][slot]: {x, y, a2, b2 | c2, o, position + 1, m | A, B, C, opacity}, the ids beside them
    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * 3];
    __shared__ uint32_t sids[4][64 + CB];
    __shared__ __attribute__((aligned(16))) float2 qmat[4][CB * MSTR];  // [wave][slot of the batch][pixel] = (q, u)
    float4 *wslab = slab[wave];
    uint32_t *wid = sids[wave];
    float2 *wm = qmat[wave];
    const int bslot = lane >> 3, bpart = lane & 7;  // phase B: this lane's slot of the batch and its row of the quadrant
    float T = inside ? final_T[pid] : 1.0f;
    float rho = 0.f;  // (w e blended BEHIND the current position) / (the transmittance behind the current position)
    for (int c = ((wlen - 1) / 64) * 64; c >= 0; c -= 64) {  // wave-uniform, back to front
        const int nrel = stage_chunk<BACK_TO_FRONT, 3>(
            c, lane, wlen, range.x, qx0, qy0, point_list, means2D, conic_opacity, wslab,
            [&](uint32_t id) {
                const float z = depths[id];
                return c0 + c1 * z + c2 / z;
            },
            [&](int slot, uint32_t id) {
                wslab[3 * slot + 2] = conic_opacity[id];
                wid[slot] = id;
            },
            [&](int slot) {  // an opacity that divides
                wslab[3 * slot + 2] = make_float4(0.f, 0.f, 0.f, 1.f);
                wid[slot] = 0u;
            });
        __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
        for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
            // phase A, lane = pixel.  A lane that does not take an entry runs the same arithmetic with alpha = 0:
            // T / (1 - 0) and rho + 0 (...) leave its state untouched and it stores (0, 0)
            unsigned int any8 = 0u;  // bit s: some pixel of the quadrant blended slot s (a scalar register)
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const float4 q0 = wslab[3 * (b0 + s)], q1 = wslab[3 * (b0 + s) + 1];  // wave-uniform address: LDS broadcasts
                // tile_walk.h's pair_decision, spelled out as in composite_invdepth_backward_kernel
                const float pe = entry_exponent(q0, q1, q0.x - pxf, q0.y - pyf);
                const float aar = entry_alpha_raw(q1, pe);  // o exp(power), unclamped
                const float aal = fminf(0.99f, aar);
                const bool take = __float_as_int(q1.z) <= last && entry_power_ok(q1, pe) && aal >= ALPHA_MIN;
                const float ar = take ? aar : 0.f, al = take ? aal : 0.f;  // (selected, never multiplied)
                const float Tn = T / (1.f - al);          // transmittance in front of the entry
                const float dm = q1.w - mut;              // m - mu of the pixel
                const float e = fmaf(At * dm, dm, St);    // dD/dw of the entry on this pixel
                const float dot = e - rho;                // e - (what lies behind, normalised)
                const float gT = g * Tn;
                wm[s * MSTR + lane] = make_float2(ar * (gT * dot), al * (Tn * (gA2 * dm)));
                rho = fmaf(al, dot, rho);
                T = Tn;
                any8 |= (__ballot(take) != 0ull ? 1u : 0u) << s;
            }
            __builtin_amdgcn_wave_barrier();
            // phase B, lane = (slot, row): the row's eight pixels in order, then the rows by xor 1, 2, 4
            const float4 p0 = wslab[3 * (b0 + bslot)];
            const float ex = p0.x - (float)qx0, dy = p0.y - (float)(qy0 + bpart);
            const float4 *qr = reinterpret_cast<const float4 *>(wm + bslot * MSTR + 8 * bpart);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, su = 0.f;
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const float4 t = qr[h];  // pixels 2 h, 2 h + 1 of the row: (q, u, q, u)
                const float dxa = ex - (float)(2 * h), dxb = ex - (float)(2 * h + 1);
                s0 += t.x;
                s1 = fmaf(t.x, dxa, s1);
                s2 = fmaf(t.x * dxa, dxa, s2);
                su += t.y;
                s0 += t.z;
                s1 = fmaf(t.z, dxb, s1);
                s2 = fmaf(t.z * dxb, dxb, s2);
                su += t.w;
            }
            float M0 = s0, Mx = s1, My = dy * s0, Mxx = s2, Mxy = dy * s1, Myy = dy * (dy * s0), Su = su;
#pragma unroll
            for (int d = 1; d <= 4; d <<= 1) {
                M0 += __shfl_xor(M0, d, 64);
                Mx += __shfl_xor(Mx, d, 64);
                My += __shfl_xor(My, d, 64);
                Mxx += __shfl_xor(Mxx, d, 64);
                Mxy += __shfl_xor(Mxy, d, 64);
                Myy += __shfl_xor(Myy, d, 64);
                Su += __shfl_xor(Su, d, 64);
            }
            // every lane of the slot holds the seven sums; lane k < 7 adds value k of the row
            const float4 co = wslab[3 * (b0 + bslot) + 2];
            float val = -(co.x * Mx + co.y * My) * ddelx_dx;
            val = bpart == 1 ? -(co.y * Mx + co.z * My) * ddely_dy : val;
            val = bpart == 2 ? -0.5f * Mxx : val;
            val = bpart == 3 ? -Mxy : val;
            val = bpart == 4 ? -0.5f * Myy : val;
            val = bpart == 5 ? (M0 == 0.f ? 0.f : M0 / co.w) : val;
            val = bpart == 6 ? Su : val;
            if (bpart < 7 && ((any8 >> bslot) & 1u) && val != 0.f)
                atomicAdd(acc64 + 7 * (size_t)wid[b0 + bslot] + bpart, (double)val);
            __builtin_amdgcn_wave_barrier();  // the next batch overwrites the matrix only after these reads
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
    }
}

// the fp64 sums rounded once into the fp32 record, which is written whole; column 6: sum u -> dL/ddepth =
// (c1 - c2 / depth^2) sum u
__global__ void distortion_record_kernel(const double *__restrict__ acc, const float *__restrict__ depths, double c1,
                                         double c2, float *__restrict__ rec, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = acc[i];
    if (i % 7 == 6 && a != 0.0) {  // (a row blended nowhere may carry any depth, 0 included: it is not read)
        const double d = (double)depths[i / 7];
        a *= c1 - c2 / (d * d);
    }
    rec[i] = a == 0.0 ? 0.0f : (float)a;
}

}  // namespace

int gsr_launch_composite_distortion(int P, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                    const float *means2D, const float *conic_opacity, const float *depths,
                                    const uint8_t *compute_locally, const int32_t *n_contrib, float c0, float c1,
                                    float c2, int row_lo, int row_hi, float *maps, hipStream_t stream) {
    GSR_HIP(hipMemsetAsync(maps, 0, sizeof(float) * 4 * (size_t)W * H, stream));
    if (P == 0) return 0;
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    hipLaunchKernelGGL(composite_distortion_kernel, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, W, H,
                       gx, gx * gy, reinterpret_cast<const int2 *>(ranges), point_list,
                       reinterpret_cast<const float2 *>(means2D), reinterpret_cast<const float4 *>(conic_opacity),
                       depths, compute_locally, n_contrib, c0, c1, c2, b.band ? 1 : 0, b.band_first, b.band_tiles, maps);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_composite_distortion_backward(int P, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                             const float *means2D, const float *conic_opacity, const float *depths,
                                             const uint8_t *compute_locally, const int32_t *n_contrib, float c0,
                                             float c1, float c2, const float *final_T, const float *maps,
                                             const float *dL_dD, int row_lo, int row_hi, float *dL_record,
                                             double *acc64, hipStream_t stream) {
    GSR_HIP(hipMemsetAsync(acc64, 0, sizeof(double) * 7 * (size_t)P, stream));
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    hipLaunchKernelGGL(composite_distortion_backward_kernel, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream,
                       W, H, gx, gx * gy, reinterpret_cast<const int2 *>(ranges), point_list,
                       reinterpret_cast<const float2 *>(means2D), reinterpret_cast<const float4 *>(conic_opacity),
                       depths, compute_locally, n_contrib, c0, c1, c2, final_T, maps, dL_dD, b.band ? 1 : 0,
                       b.band_first, b.band_tiles, acc64);
    GSR_LAUNCH_CHECK();
    const size_t nrec = 7 * (size_t)P;
    hipLaunchKernelGGL(distortion_record_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, stream, acc64,
                       depths, (double)c1, (double)c2, dL_record, nrec);
    GSR_LAUNCH_CHECK();
    return 0;
}
