// invdepth.hip -- the INVERSE-DEPTH map of one rendered view from the tile lists, and its backward (gfx950 / wave64).
//
// K8 (composite.hip) decides what every pixel blends; the kernels here walk the same lists once more and blend
// v = 1 / depth instead of a colour: invdepth[p] = sum over the blended entries of w v, w = alpha T (the official 3DGS
// rasterizer's inverse-depth output: no background term, no division by 1 - T_final).  Nothing is re-decided: a pixel's
// walk ends where K8's ended (n_contrib), and the (pixel, entry) pairs taken are K10's `take` rule -- position + 1 <=
// n_contrib, power <= 0, alpha >= 1/255 -- in the arithmetic of composite_math.h, which K8, K10 and the contribution
// kernel compile too.  Those kernels are untouched; a trainer that does not ask for the map never launches these.
//
// Forward (composite_invdepth_kernel): the contribution kernel's shape.  One wave = one 8x8 quadrant, lane = pixel; the
// list is walked in 64-entry chunks, one entry per lane (index read + gather + quadrant test + 1 / depth), the relevant
// entries are compacted in list order into records in a wave-private LDS slab (v beside the position word) and read back
// with wave-uniform addresses; the walk of a wave ends at the largest n_contrib of its quadrant.  Per blended entry one
// fma into a register, one store per pixel at the end.  The map is cleared by a fill in front of the launch: pixels of
// tiles that are not ours, and of tiles outside a band launch, are exactly 0 (the map is assembled across bands by SUM).
//
// Backward (composite_invdepth_backward_kernel): K10's chain.  The walk goes back to front from final_T: with alpha of
// the entry, Tn = T / (1 - alpha) is the transmittance in front of it and rho = (what is blended behind it) / (its own
// T (1 - alpha)) one scalar recurrence, so that
//     dL/dalpha = g Tn (v - rho)            (= g (T_i v_i - S_i / (1 - alpha_i)), g = dL/dinvdepth[p])
//     q = o G dL/dalpha                      (G = exp(power); the min(0.99, .) clamp is the identity in the backward)
//     u = g alpha Tn                         (dL/dv of the pair)
// and every gradient of the entry is a sum over the pixels of q or u times a polynomial of (dx, dy) = entry - pixel:
//     dL/dmean = -(A Mx + B My, B Mx + C My) (W/2, H/2),  dL/d(A, B, C) = -(Mxx / 2, Mxy, Myy / 2),  dL/do = M0 / o,
//     dL/dv = sum u,      M0 = sum q, Mx = sum q dx, My = sum q dy, Mxx = sum q dx^2, Mxy = sum q dx dy, Myy = sum q dy^2.
// The reduction over the quadrant's 64 pixels is an LDS TRANSPOSE over a batch of CB = 8 entries (contrib.hip's): phase A
// (lane = pixel) stores (q, u) of every entry of the batch into a wave-private matrix [slot][pixel]; phase B (lane =
// (slot, row of the quadrant)) reads its row's eight pixels, forms sum q, sum q dx, sum q dx^2 and sum u over them in pixel
// order -- dy is constant along a row, so the moments in dy are products of those -- and three xor steps combine the rows:
// a fixed order, fp32, about dx itself (no expansion about a tile origin).  Every lane of a slot then holds the seven
// sums; lane k < 7 of the slot maps them to value k of the row [means2D 2 | conic 3 | opacity | v] and adds it into the
// caller's fp64 sums [P,7], seven adjacent lanes per (quadrant, entry) into one 56-byte row.  Entries no pixel of the
// quadrant blends issue nothing.  (LDS: 4.1 KiB matrix + 3.7 KiB slab and ids per wave, 31.1 KiB per workgroup -- five
// workgroups per CU of its 160 KiB, 78 VGPRs; seven full [slot][pixel] matrices would have been 15 KiB per wave and two
// workgroups.)
// A rounding pass then writes the whole fp32 record: each sum rounded once, the v column turned into dL/ddepth =
// -(sum u) / depth^2 in fp64 first; rows that are blended nowhere are 0.0f.  The fp32 result does not depend on the order
// the tiles finish except where an fp64 sum lies within fp64 rounding of an fp32 rounding boundary (K10's reason).
//
// depth_to_means3D_kernel: depth = ([p, 1] viewmatrix)[2] (row-vector convention), so dL/dp = dL/ddepth times the
// third column of the view matrix's upper three rows.
#include "common.h"
#include "composite_math.h"

namespace {

constexpr int CB = 8;                   // entries per batch (forward: per unrolled group of the walk)
constexpr int MSTR = 66;                // row stride of the (q, u) matrix in 8-byte elements (16-byte aligned rows)
constexpr int NO_POS = 0x7fffffff;      // position word of an inert slot: no n_contrib reaches it

// block -> tile as in K8 / the contribution kernel; -1: this workgroup has no tile
__device__ __forceinline__ int invdepth_tile_of_block(const int2 *__restrict__ ranges, int gx, int tiles, int band,
                                                      int band_first, int band_tiles) {
    if (band) {
        if (band_first < 0) {  // `band_tiles` is a capacity, the band is the row hull behind the range table
            const int gy = tiles / gx;
            int2 hull = ranges[tiles];
            if (hull.x < 0 || hull.y > gy || hull.x >= hull.y) hull = make_int2(0, 0);
            band_first = hull.x * gx;
            band_tiles = min((hull.y - hull.x) * gx, band_tiles);
            if ((int)blockIdx.x >= band_tiles) return -1;
        }
        return band_first + gsr_xcd_span_of_block(blockIdx.x, band_tiles);
    }
    return composite_tile_of_block(ranges, gx, tiles);
}

__global__ void __launch_bounds__(256)
composite_invdepth_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                          const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                          const float4 *__restrict__ conic_opacity, const float *__restrict__ depths,
                          const uint8_t *__restrict__ compute_locally, const int32_t *__restrict__ n_contrib, int band,
                          int band_first, int band_tiles, float *__restrict__ invdepth) {
    const int tile = invdepth_tile_of_block(ranges, gx, tiles, band, band_first, band_tiles);
    if (tile < 0 || !compute_locally[tile]) return;  // (no workgroup barrier below: waves leave on their own)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx = tile % gx, ty = tile / gx;
    const int qx0 = tx * GSR_BLOCK_X + (wave & 1) * 8, qy0 = ty * GSR_BLOCK_Y + (wave >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const int2 range = ranges[tile];
    const int n = range.y - range.x;
    const float pxf = (float)px, pyf = (float)py;
    // where K8 stopped on this pixel; never beyond the list, whatever the caller's array holds
    const int last = inside ? min(n_contrib[(size_t)py * W + px], n) : 0;
    int wlen = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wlen = max(wlen, __shfl_xor(wlen, d, 64));
    if (wlen <= 0) return;  // (the map was cleared in front of the launch)

    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * 2];  // [wave][slot]: {x, y, a2, b2 | c2, o, position + 1, v}
    float4 *wslab = slab[wave];
    float T = 1.0f, acc = 0.f;
    for (int c = 0; c < wlen; c += 64) {  // wave-uniform
        const bool have = c + lane < wlen;
        const uint32_t id = have ? point_list[range.x + c + lane] : 0u;
        const Entry e = load_entry(have, id, means2D, conic_opacity, (float)qx0, (float)qy0);
        const unsigned long long m = __ballot(e.relevant);
        const int nrel = __popcll(m);
        if (e.relevant) {
            const int pos = __popcll(m & ((1ull << lane) - 1ull));
            wslab[2 * pos] = make_float4(e.x, e.y, e.a2, e.b2);
            wslab[2 * pos + 1] = make_float4(e.c2, e.o, __int_as_float(c + lane + 1), 1.0f / depths[id]);
        }
        {   // the walk takes CB slots at a time: the <= CB - 1 slots behind the last entry are made inert (both quads
            // written: nothing stale is ever read; v = 0)
            const int pad = (-nrel) & (CB - 1);
            if (lane < pad) {
                wslab[2 * (nrel + lane)] = make_float4(0.f, 0.f, 0.f, 0.f);
                wslab[2 * (nrel + lane) + 1] = make_float4(0.f, 0.f, __int_as_float(NO_POS), 0.f);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
        for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
            // alphas are independent, only the short T chain is sequential
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const float4 q0 = wslab[2 * (b0 + s)], q1 = wslab[2 * (b0 + s) + 1];  // wave-uniform address: LDS broadcasts
                const float pe = entry_exponent(q0, q1, q0.x - pxf, q0.y - pyf);
                const float al = fminf(0.99f, entry_alpha_raw(q1, pe));
                const bool take = __float_as_int(q1.z) <= last && entry_power_ok(q1, pe) && al >= ALPHA_MIN;
                const float w = take ? al * T : 0.f;  // (selected, never multiplied: an inert slot's alpha is not used)
                T -= w;  // T (1 - alpha) as K8 forms it: T - alpha T
                acc = fmaf(w, q1.w, acc);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
    }
    if (inside) invdepth[(size_t)py * W + px] = acc;
}

__global__ void __launch_bounds__(256)
composite_invdepth_backward_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                                   const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                                   const float4 *__restrict__ conic_opacity, const float *__restrict__ depths,
                                   const uint8_t *__restrict__ compute_locally, const int32_t *__restrict__ n_contrib,
                                   const float *__restrict__ final_T, const float *__restrict__ dL_dinvdepth, int band,
                                   int band_first, int band_tiles, double *__restrict__ acc64) {
    const int tile = invdepth_tile_of_block(ranges, gx, tiles, band, band_first, band_tiles);
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
    const float g = inside ? dL_dinvdepth[pid] : 0.f;
    const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;

    // [wave][slot]: {x, y, a2, b2 | c2, o, position + 1, v | A, B, C, opacity}, the ids beside them
    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * 3];
    __shared__ uint32_t sids[4][64 + CB];
    __shared__ __attribute__((aligned(16))) float2 qmat[4][CB * MSTR];  // [wave][slot of the batch][pixel] = (q, u)
    float4 *wslab = slab[wave];
    uint32_t *wid = sids[wave];
    float2 *wm = qmat[wave];
    const int bslot = lane >> 3, bpart = lane & 7;  // phase B: this lane's slot of the batch and its row of the quadrant
    float T = inside ? final_T[pid] : 1.0f;
    float rho = 0.f;  // (v blended BEHIND the current position) / (the transmittance behind the current position)
    for (int c = ((wlen - 1) / 64) * 64; c >= 0; c -= 64) {  // wave-uniform, back to front
        const bool have = c + lane < wlen;
        const uint32_t id = have ? point_list[range.x + c + lane] : 0u;
        const Entry e = load_entry(have, id, means2D, conic_opacity, (float)qx0, (float)qy0);
        const unsigned long long m = __ballot(e.relevant);
        const int nrel = __popcll(m);
        if (e.relevant) {  // compacted in WALK order: rank = relevant lanes above
            const int pos = __popcll((m >> lane) >> 1);
            wslab[3 * pos] = make_float4(e.x, e.y, e.a2, e.b2);
            wslab[3 * pos + 1] = make_float4(e.c2, e.o, __int_as_float(c + lane + 1), 1.0f / depths[id]);
            wslab[3 * pos + 2] = conic_opacity[id];
            wid[pos] = id;
        }
        {   // the <= CB - 1 slots behind the last entry are inert: every word written, an opacity that divides
            const int pad = (-nrel) & (CB - 1);
            if (lane < pad) {
                wslab[3 * (nrel + lane)] = make_float4(0.f, 0.f, 0.f, 0.f);
                wslab[3 * (nrel + lane) + 1] = make_float4(0.f, 0.f, __int_as_float(NO_POS), 0.f);
                wslab[3 * (nrel + lane) + 2] = make_float4(0.f, 0.f, 0.f, 1.f);
                wid[nrel + lane] = 0u;
            }
        }
        __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
        for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
            // phase A, lane = pixel.  A lane that does not take an entry runs the same arithmetic with alpha = 0:
            // T / (1 - 0) and rho + 0 (...) leave its state untouched and it stores (0, 0)
            unsigned int any8 = 0u;  // bit s: some pixel of the quadrant blended slot s (a scalar register)
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const float4 q0 = wslab[3 * (b0 + s)], q1 = wslab[3 * (b0 + s) + 1];  // wave-uniform address: LDS broadcasts
                const float pe = entry_exponent(q0, q1, q0.x - pxf, q0.y - pyf);
                const float aar = entry_alpha_raw(q1, pe);  // o exp(power), unclamped
                const float aal = fminf(0.99f, aar);
                const bool take = __float_as_int(q1.z) <= last && entry_power_ok(q1, pe) && aal >= ALPHA_MIN;
                const float ar = take ? aar : 0.f, al = take ? aal : 0.f;  // (selected, never multiplied)
                const float Tn = T / (1.f - al);      // transmittance in front of the entry
                const float dot = q1.w - rho;         // v - (what lies behind, normalised)
                const float gT = g * Tn;
                wm[s * MSTR + lane] = make_float2(ar * (gT * dot), al * gT);
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
            if (bpart < 7 && ((any8 >> bslot) & 1u) && val != 0.f) {
#ifndef GSR_ABL_INVDEPTH_NOATOMIC
                atomicAdd(acc64 + 7 * (size_t)wid[b0 + bslot] + bpart, (double)val);
#else  // ablation: everything but the atomics
                asm volatile("" ::"v"(val), "v"(wid[b0 + bslot]));
#endif
            }
            __builtin_amdgcn_wave_barrier();  // the next batch overwrites the matrix only after these reads
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
    }
}

// the fp64 sums rounded once into the fp32 record, which is written whole; column 6: sum u -> dL/ddepth = -(sum u) / depth^2
__global__ void invdepth_record_kernel(const double *__restrict__ acc, const float *__restrict__ depths,
                                       float *__restrict__ rec, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = acc[i];
    if (i % 7 == 6 && a != 0.0) {  // (a row blended nowhere may carry any depth, 0 included: it is not read)
        const double d = (double)depths[i / 7];
        a = -a / (d * d);
    }
    rec[i] = a == 0.0 ? 0.0f : (float)a;
}

__global__ void depth_to_means3D_kernel(int P, const int32_t *__restrict__ radii, const float *__restrict__ viewmatrix,
                                        const float *__restrict__ dL_ddepth, int row_stride,
                                        float *__restrict__ dL_dmeans3D, int overwrite) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= P) return;
    float *o = dL_dmeans3D + 3 * (size_t)i;
    if (radii[i] <= 0) {
        if (overwrite) o[0] = o[1] = o[2] = 0.f;
        return;
    }
    const float d = dL_ddepth[(size_t)i * row_stride];
    const float v0 = d * viewmatrix[2], v1 = d * viewmatrix[6], v2 = d * viewmatrix[10];
    if (overwrite) {
        o[0] = v0;  o[1] = v1;  o[2] = v2;
    } else {
        o[0] += v0; o[1] += v1; o[2] += v2;
    }
}

}  // namespace

int gsr_launch_composite_invdepth(int P, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                  const float *means2D, const float *conic_opacity, const float *depths,
                                  const uint8_t *compute_locally, const int32_t *n_contrib, int row_lo, int row_hi,
                                  float *invdepth, hipStream_t stream) {
    GSR_HIP(hipMemsetAsync(invdepth, 0, sizeof(float) * (size_t)W * H, stream));
    if (P == 0) return 0;
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    hipLaunchKernelGGL(composite_invdepth_kernel, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, W, H, gx,
                       gx * gy, reinterpret_cast<const int2 *>(ranges), point_list,
                       reinterpret_cast<const float2 *>(means2D), reinterpret_cast<const float4 *>(conic_opacity),
                       depths, compute_locally, n_contrib, b.band ? 1 : 0, b.band_first, b.band_tiles, invdepth);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_composite_invdepth_backward(int P, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                           const float *means2D, const float *conic_opacity, const float *depths,
                                           const uint8_t *compute_locally, const int32_t *n_contrib,
                                           const float *final_T, const float *dL_dinvdepth, int row_lo, int row_hi,
                                           float *dL_record, double *acc64, hipStream_t stream) {
    GSR_HIP(hipMemsetAsync(acc64, 0, sizeof(double) * 7 * (size_t)P, stream));
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    hipLaunchKernelGGL(composite_invdepth_backward_kernel, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, W,
                       H, gx, gx * gy, reinterpret_cast<const int2 *>(ranges), point_list,
                       reinterpret_cast<const float2 *>(means2D), reinterpret_cast<const float4 *>(conic_opacity),
                       depths, compute_locally, n_contrib, final_T, dL_dinvdepth, b.band ? 1 : 0, b.band_first,
                       b.band_tiles, acc64);
    GSR_LAUNCH_CHECK();
    const size_t nrec = 7 * (size_t)P;
    hipLaunchKernelGGL(invdepth_record_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, stream, acc64, depths,
                       dL_record, nrec);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_depth_to_means3D(int P, const int32_t *radii, const float *viewmatrix, const float *dL_ddepth,
                                int row_stride, float *dL_dmeans3D, int overwrite, hipStream_t stream) {
    hipLaunchKernelGGL(depth_to_means3D_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, P, radii,
                       viewmatrix, dL_ddepth, row_stride, dL_dmeans3D, overwrite);
    GSR_LAUNCH_CHECK();
    return 0;
}
