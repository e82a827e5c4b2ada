// absgrad.hip -- the ABSOLUTE screen-space gradient of one rendered view from the tile lists (gfx950 / wave64): per
// Gaussian the sum over the pixels of the MAGNITUDE of each pixel's contribution to dL/dmeans2D (the homodirectional
// gradient of AbsGS, `absgrad` of gsplat), the densification signal that does not cancel on a large Gaussian whose pixels
// pull its centre in opposite directions.
//
// The quantity needs dL/dalpha per (pixel, entry) BEFORE the sum over the pixels, which K10 (composite.hip) forms and
// contracts at once; K10 has no register left to carry a second contraction.  The kernel here walks the same lists once
// more, as contrib.hip and invdepth.hip do: a pixel's walk ends where K8's ended (n_contrib), the (pixel, entry) pairs
// taken are K10's `take` rule -- position + 1 <= n_contrib, power <= 0, alpha >= 1/255 -- in the arithmetic of
// composite_math.h, and the chain is K10's (its reciprocal refined by one Newton step).  K8 and K10 are untouched; a
// trainer that does not ask for the quantity never launches this.
//
// composite_absgrad_kernel: the shape of composite_invdepth_backward_kernel.  One wave = one 8x8 quadrant, lane = pixel;
// the list is walked back to front from final_T in 64-entry chunks, one entry per lane (index read + gather + quadrant
// test), the relevant entries compacted in walk order into records in a wave-private LDS slab -- the three colours
// beside the geometry -- and read back with wave-uniform addresses.  With alpha of the entry, inv = 1 / (1 - alpha),
// Tn = T inv the transmittance in front of it, rho = (the colour blended behind it) . g / (its own T (1 - alpha)) one
// scalar recurrence (K10 carries R . g, not R: the three channels only ever enter through the pixel's g),
//     dL/dalpha = (c . g - rho) Tn - inv T_final (bg . g)
//     q = o G dL/dalpha                      (G = exp(power); the min(0.99, .) clamp is the identity in the backward)
//     m = ( |q (2 a2 dx + b2 dy)| , |q (b2 dx + 2 c2 dy)| ),   (dx, dy) = entry - pixel,
// a2 = -A log2(e) / 2, b2 = -B log2(e), c2 = -C log2(e) / 2 the slab's pre-scaled conic: (2 a2, b2, 2 c2) is (A, B, C)
// times -log2(e), a factor that is constant over the pixels and whose sign the magnitude drops, so it is taken out of
// the sum and applied once per (quadrant, entry) as ln 2 -- the slab needs no second copy of the conic.
// The reduction over the quadrant's 64 pixels is the LDS TRANSPOSE of invdepth.hip over a batch of CB = 8 entries: phase
// A (lane = pixel) stores m of every entry of the batch into a wave-private matrix [slot][pixel]; phase B (lane = (slot,
// row of the quadrant)) adds its row's eight pixels in pixel order and three xor steps combine the rows: a fixed order,
// fp32, non-negative terms.  Lanes 0 and 1 of the slot scale the two sums by ln 2 (W/2, H/2) and add them into the
// caller's fp64 sums [P,2], two adjacent lanes per (quadrant, entry) into one 16-byte row.  Entries no pixel of the
// quadrant blends issue nothing.  The segment workspace of K8 / K10 is not used: the walk is the whole list.
// (LDS: 4.1 KiB matrix + 3.7 KiB slab and ids per wave, 31.1 KiB per workgroup -- five workgroups per CU of its 160 KiB,
// as the inverse-depth backward.)
// A rounding pass then writes the whole fp32 [P,2]: each sum rounded once; rows that are blended nowhere are 0.0f.  The
// fp32 result does not depend on the order the tiles finish except where an fp64 sum lies within fp64 rounding of an fp32
// rounding boundary (K10's reason).
//
// absgrad_merge_rows_kernel: dst[idx[r]][0:2] += src[r][0:2], the return trip of a multi-rank render.
#include "common.h"
#include "composite_math.h"

namespace {

constexpr int CB = 8;                   // entries per batch
constexpr int MSTR = 66;                // row stride of the magnitude matrix in 8-byte elements (16-byte aligned rows)
constexpr int NO_POS = 0x7fffffff;      // position word of an inert slot: no n_contrib reaches it
constexpr float LN2 = 0.6931471805599453f;  // 1 / log2(e): (2 a2, b2, 2 c2) -> -(A, B, C)

// block -> tile as in K8 / the contribution kernel; -1: this workgroup has no tile
__device__ __forceinline__ int absgrad_tile_of_block(const int2 *__restrict__ ranges, int gx, int tiles, int band,
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
composite_absgrad_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                         const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                         const float4 *__restrict__ conic_opacity, const float *__restrict__ rgb,
                         const uint8_t *__restrict__ compute_locally, const float *__restrict__ bg,
                         const int32_t *__restrict__ n_contrib, const float *__restrict__ final_T,
                         const float *__restrict__ dL_dpixels, int band, int band_first, int band_tiles,
                         double *__restrict__ acc64) {
    const int tile = absgrad_tile_of_block(ranges, gx, tiles, band, band_first, band_tiles);
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
    // where K8 stopped on this pixel; never beyond the list, whatever the caller's array holds
    const int last = inside ? min(n_contrib[pid], n) : 0;
    int wlen = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wlen = max(wlen, __shfl_xor(wlen, d, 64));
    if (wlen <= 0) return;
    const size_t HW = (size_t)H * W;
    const float g0 = inside ? dL_dpixels[pid] : 0.f, g1 = inside ? dL_dpixels[HW + pid] : 0.f,
                g2 = inside ? dL_dpixels[2 * HW + pid] : 0.f;
    float T = inside ? final_T[pid] : 1.0f;
    const float tb = inside ? T * (bg[0] * g0 + bg[1] * g1 + bg[2] * g2) : 0.f;  // T_final (bg . g), K10's
    const float sx = LN2 * (0.5f * W), sy = LN2 * (0.5f * H);

    // [wave][slot]: {x, y, a2, b2 | c2, o, position + 1, - | r, g, b, -}, the ids beside them
    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * 3];
    __shared__ uint32_t sids[4][64 + CB];
    __shared__ __attribute__((aligned(16))) float2 mmat[4][CB * MSTR];  // [wave][slot of the batch][pixel] = (m0, m1)
    float4 *wslab = slab[wave];
    uint32_t *wid = sids[wave];
    float2 *wm = mmat[wave];
    const int bslot = lane >> 3, bpart = lane & 7;  // phase B: this lane's slot of the batch and its row of the quadrant
    float rho = 0.f;  // (colour blended BEHIND the current position) . g / (the transmittance behind the current position)
    for (int c = ((wlen - 1) / 64) * 64; c >= 0; c -= 64) {  // wave-uniform, back to front
        const bool have = c + lane < wlen;
        const uint32_t id = have ? point_list[range.x + c + lane] : 0u;
        const Entry e = load_entry(have, id, means2D, conic_opacity, (float)qx0, (float)qy0);
        const unsigned long long m = __ballot(e.relevant);
        const int nrel = __popcll(m);
        if (e.relevant) {  // compacted in WALK order: rank = relevant lanes above
            const int pos = __popcll((m >> lane) >> 1);
            const float *col = rgb + 3 * (size_t)id;
            wslab[3 * pos] = make_float4(e.x, e.y, e.a2, e.b2);
            wslab[3 * pos + 1] = make_float4(e.c2, e.o, __int_as_float(c + lane + 1), 0.f);
            wslab[3 * pos + 2] = make_float4(col[0], col[1], col[2], 0.f);
            wid[pos] = id;
        }
        {   // the <= CB - 1 slots behind the last entry are inert: every word written
            const int pad = (-nrel) & (CB - 1);
            if (lane < pad) {
                wslab[3 * (nrel + lane)] = make_float4(0.f, 0.f, 0.f, 0.f);
                wslab[3 * (nrel + lane) + 1] = make_float4(0.f, 0.f, __int_as_float(NO_POS), 0.f);
                wslab[3 * (nrel + lane) + 2] = make_float4(0.f, 0.f, 0.f, 0.f);
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
                const float4 q2 = wslab[3 * (b0 + s) + 2];
                const float dx = q0.x - pxf, dy = q0.y - pyf;
                const float pe = entry_exponent(q0, q1, dx, dy);
                const float aar = entry_alpha_raw(q1, pe);  // o exp(power), unclamped
                const float aal = fminf(0.99f, aar);
                const bool take = __float_as_int(q1.z) <= last && entry_power_ok(q1, pe) && aal >= ALPHA_MIN;
                const float ar = take ? aar : 0.f, al = take ? aal : 0.f;  // (selected, never multiplied)
                // v_rcp_f32 and one Newton step: T is multiplied by it once per blended entry, and the magnitudes summed
                // here do not cancel a drift of T as K10's signed sums partly do (EXPERIMENTS.md: 8.3 of K = 14 on 600
                // blended entries with the bare reciprocal)
                const float om = 1.f - al;
                float inv = __builtin_amdgcn_rcpf(om);
                inv = fmaf(fmaf(-om, inv, 1.f), inv, inv);
                const float cg = fmaf(q2.z, g2, fmaf(q2.y, g1, q2.x * g0));
                const float Tn = T * inv;             // transmittance in front of the entry
                const float dot = cg - rho;           // (c - R) . g
                const float da = fmaf(dot, Tn, -(inv * tb));  // dL/dalpha
                const float q = ar * da;
                const float ux = fmaf(q0.z + q0.z, dx, q0.w * dy);  // -(A dx + B dy) log2(e)
                const float uy = fmaf(q0.w, dx, (q1.x + q1.x) * dy);  // -(B dx + C dy) log2(e)
                wm[s * MSTR + lane] = make_float2(fabsf(q * ux), fabsf(q * uy));
                rho = fmaf(al, dot, rho);
                T = Tn;
                any8 |= (__ballot(take) != 0ull ? 1u : 0u) << s;
            }
            __builtin_amdgcn_wave_barrier();
            // phase B, lane = (slot, row): the row's eight pixels in order, then the rows by xor 1, 2, 4
            const float4 *mr = reinterpret_cast<const float4 *>(wm + bslot * MSTR + 8 * bpart);
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const float4 t = mr[h];  // pixels 2 h, 2 h + 1 of the row: (m0, m1, m0, m1)
                s0 += t.x;
                s1 += t.y;
                s0 += t.z;
                s1 += t.w;
            }
#pragma unroll
            for (int d = 1; d <= 4; d <<= 1) {
                s0 += __shfl_xor(s0, d, 64);
                s1 += __shfl_xor(s1, d, 64);
            }
            // every lane of the slot holds the two sums; lanes 0 and 1 add the two columns of the row
            const float val = bpart == 0 ? s0 * sx : s1 * sy;
            if (bpart < 2 && ((any8 >> bslot) & 1u) && val != 0.f)
                atomicAdd(acc64 + 2 * (size_t)wid[b0 + bslot] + bpart, (double)val);
            __builtin_amdgcn_wave_barrier();  // the next batch overwrites the matrix only after these reads
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
    }
}

// the fp64 sums rounded once into the fp32 result, which is written whole
__global__ void absgrad_round_kernel(const double *__restrict__ acc, float *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // one lane per row
    if (i >= n) return;
    const double a0 = acc[2 * i], a1 = acc[2 * i + 1];
    out[2 * i] = a0 == 0.0 ? 0.0f : (float)a0;
    out[2 * i + 1] = a1 == 0.0 ? 0.0f : (float)a1;
}

// dst[idx[r]][0:2] += src[r][0:2]; two adjacent lanes per row; rows with idx < 0 are skipped
__global__ void __launch_bounds__(256)
absgrad_merge_rows_kernel(long long n, const int32_t *__restrict__ idx, const float *__restrict__ src,
                          float *__restrict__ dst) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n * 2;
         e += (long long)gridDim.x * blockDim.x) {
        const long long r = e >> 1;
        const float v = src[e];
        const int32_t row = idx[r];
        if (v != 0.f && row >= 0) atomicAdd(dst + (size_t)row * 2 + (e & 1), v);
    }
}

}  // namespace

int gsr_launch_composite_absgrad(int P, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                 const float *means2D, const float *conic_opacity, const float *rgb,
                                 const uint8_t *compute_locally, const float *bg, const float *final_T,
                                 const int32_t *n_contrib, const float *dL_dpixels, int row_lo, int row_hi,
                                 float *absgrad, double *acc64, hipStream_t stream) {
    GSR_HIP(hipMemsetAsync(acc64, 0, sizeof(double) * 2 * (size_t)P, stream));
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    hipLaunchKernelGGL(composite_absgrad_kernel, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, W, H, gx,
                       gx * gy, reinterpret_cast<const int2 *>(ranges), point_list,
                       reinterpret_cast<const float2 *>(means2D), reinterpret_cast<const float4 *>(conic_opacity), rgb,
                       compute_locally, bg, n_contrib, final_T, dL_dpixels, b.band ? 1 : 0, b.band_first, b.band_tiles,
                       acc64);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(absgrad_round_kernel, dim3((unsigned)(((size_t)P + 255) / 256)), dim3(256), 0, stream, acc64,
                       absgrad, (size_t)P);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_absgrad_merge_rows(long long n, const int32_t *idx, const float *src, float *dst, hipStream_t stream) {
    long long blocks = (n * 2 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(absgrad_merge_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, n, idx, src, dst);
    GSR_LAUNCH_CHECK();
    return 0;
}
