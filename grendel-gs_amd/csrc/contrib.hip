// contrib.hip -- per-Gaussian CONTRIBUTION statistics of one rendered view, from the tile lists (gfx950 / wave64).
//
// K8 (composite.hip) decides what every pixel blends; this kernel walks the same lists once more, forward only, and
// tells every Gaussian what it was worth in the image K8 drew: on how many pixels it was blended (`hits`), its largest
// blend weight w = alpha T on any of them (`wmax`: RadSplat's importance) and the sum of its weights (`wsum`:
// LightGaussian's).  Nothing is re-decided: a pixel's walk ends where K8's ended (n_contrib), and the (pixel, entry)
// pairs taken are K10's `take` rule -- position + 1 <= n_contrib, power <= 0, alpha >= 1/255 -- in the arithmetic of
// composite_math.h, which K8 and K10 compile too.  K8 and K10 themselves are untouched; a trainer that does not ask
// for the statistics never launches this kernel.
//
// Shape of the work: K8's.  One wave = one 8x8 quadrant, lane = pixel; the list is walked in 64-entry chunks, one entry
// per lane (index read + gather + quadrant test), the relevant entries are compacted in list order into records in a
// wave-private LDS slab and read back with wave-uniform addresses.  The walk of a wave ends at the largest n_contrib of
// its quadrant (K10's bound): entries behind every pixel's stop are never loaded.
// The reduction over the quadrant's pixels is an LDS TRANSPOSE over a batch of CB = 8 entries: phase A (lane = pixel)
// walks the batch, carries T, and stores every entry's w (0 where the pixel does not blend it) into a wave-private
// matrix [slot][pixel]; the blend ballot's popcount -- `hits` -- goes into one byte of a scalar register pair.  Phase B (lane = (slot, eighth of the quadrant)) reads its eight pixels with two 16-byte reads, takes
// their max and their sum in pixel order, and three xor steps combine the eighths: a fixed order, fp32.  Lane 8 * slot
// then holds the entry's three values, reads the entry's id from its record, and -- if hits > 0 -- issues three atomics
// into the caller's arrays: a 64-bit integer add, an unsigned 32-bit max on the float's bits (non-negative floats order
// as their bit patterns, so the max is exact and independent of the order) and an fp64 add (the quadrant's fp32 sum,
// widened).  (A 64-lane xor butterfly per entry instead -- twelve dependent cross-lane moves -- measured 3.9 x K8's time
// for this kernel alone; EXPERIMENTS.md.)  The slots behind a chunk's last relevant entry, up to the batch size, are
// INERT records: their position word fails `position + 1 <= n_contrib` on every pixel.
// The four quadrant waves of a tile never synchronise: each issues its own atomics, so a row receives at most
// 4 x local tiles fp64 additions per launch.  Rows that are blended nowhere are never written.
#include "common.h"
#include "composite_math.h"

namespace {

constexpr int CB = 8;            // entries per transpose batch
constexpr int WSTR = 64 + 4;     // row stride of the w matrix in floats: phase B's 16-byte reads of the 8 slots spread over the banks
constexpr int NO_POS = 0x7fffffff;  // position word of an inert slot: no n_contrib reaches it

__global__ void __launch_bounds__(256)
composite_contrib_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                         const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                         const float4 *__restrict__ conic_opacity, const uint8_t *__restrict__ compute_locally,
                         const int32_t *__restrict__ n_contrib, int band, int band_first, int band_tiles,
                         unsigned long long *__restrict__ hits, unsigned int *__restrict__ wmax,
                         double *__restrict__ wsum) {
    // block -> tile as in K8: the band's tiles only when the caller named the band (band_first < 0: `band_tiles` is a
    // capacity, the band is the row hull behind the range table), else XCD-contiguous spans of the hull's tiles first
    int tile;
    if (band) {
        if (band_first < 0) {
            const int gy = tiles / gx;
            int2 hull = ranges[tiles];
            if (hull.x < 0 || hull.y > gy || hull.x >= hull.y) hull = make_int2(0, 0);
            band_first = hull.x * gx;
            band_tiles = min((hull.y - hull.x) * gx, band_tiles);
            if ((int)blockIdx.x >= band_tiles) return;
        }
        tile = band_first + gsr_xcd_span_of_block(blockIdx.x, band_tiles);
    } else {
        tile = composite_tile_of_block(ranges, gx, tiles);
    }
    if (!compute_locally[tile]) return;  // (no workgroup barrier below: waves leave on their own)
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
    if (wlen <= 0) return;

    __shared__ __attribute__((aligned(16))) float4 slab[4][64 * 2];   // [wave][slot]: {x, y, a2, b2 | c2, o, position + 1, id}
    __shared__ __attribute__((aligned(16))) float wmat[4][CB * WSTR];  // [wave][slot of the batch][pixel] = w
    float4 *wslab = slab[wave];
    float *wm = wmat[wave];
    const int bslot = lane >> 3, bpart = lane & 7;  // phase B: this lane's slot of the batch and its eighth of the pixels
    float T = 1.0f;
    for (int c = 0; c < wlen; c += 64) {  // wave-uniform
        const bool have = c + lane < wlen;
        const uint32_t id = have ? point_list[range.x + c + lane] : 0u;
        const Entry e = load_entry(have, id, means2D, conic_opacity, (float)qx0, (float)qy0);
        const unsigned long long m = __ballot(e.relevant);
        const int nrel = __popcll(m);
        if (e.relevant) {
            const int pos = __popcll(m & ((1ull << lane) - 1ull));
            wslab[2 * pos] = make_float4(e.x, e.y, e.a2, e.b2);
            wslab[2 * pos + 1] = make_float4(e.c2, e.o, __int_as_float(c + lane + 1), __uint_as_float(id));
        }
        {   // the walk takes CB slots at a time: the <= CB - 1 slots behind the last entry are made inert (both quads
            // written: nothing stale is ever read)
            const int pad = (-nrel) & (CB - 1);
            if (lane < pad) {
                wslab[2 * (nrel + lane)] = make_float4(0.f, 0.f, 0.f, 0.f);
                wslab[2 * (nrel + lane) + 1] = make_float4(0.f, 0.f, __int_as_float(NO_POS), 0.f);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
        for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
            // phase A, lane = pixel: alphas are independent, only the short T chain is sequential
            unsigned long long cnt8 = 0ull;  // byte s: the pixels that blended slot s (<= 64), in a scalar register pair
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const float4 q0 = wslab[2 * (b0 + s)], q1 = wslab[2 * (b0 + s) + 1];  // wave-uniform address: LDS broadcasts
                const float pe = entry_exponent(q0, q1, q0.x - pxf, q0.y - pyf);
                const float al = fminf(0.99f, entry_alpha_raw(q1, pe));
                const bool take = __float_as_int(q1.z) <= last && entry_power_ok(q1, pe) && al >= ALPHA_MIN;
                const float w = take ? al * T : 0.f;  // (selected, never multiplied: an inert slot's alpha is not used)
                T -= w;  // T (1 - alpha) as K8 forms it: T - alpha T
                wm[s * WSTR + lane] = w;
                cnt8 |= (unsigned long long)__popcll(__ballot(take)) << (8 * s);
            }
            const int hv = (int)((cnt8 >> (8 * bslot)) & 0xffull);
            __builtin_amdgcn_wave_barrier();
            // phase B, lane = (slot, eighth): eight pixels in order, then the eighths by xor 1, 2, 4
            const float4 *wr = reinterpret_cast<const float4 *>(wm + bslot * WSTR + 8 * bpart);
            const float4 u = wr[0], v = wr[1];
            float rs = ((((((u.x + u.y) + u.z) + u.w) + v.x) + v.y) + v.z) + v.w;
            float rm = fmaxf(fmaxf(fmaxf(u.x, u.y), fmaxf(u.z, u.w)), fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
#pragma unroll
            for (int d = 1; d <= 4; d <<= 1) {
                rs += __shfl_xor(rs, d, 64);
                rm = fmaxf(rm, __shfl_xor(rm, d, 64));
            }
            if (bpart == 0 && hv > 0) {  // one lane per blended entry of the batch (an inert slot has no hits)
                const uint32_t eid = __float_as_uint(wslab[2 * (b0 + bslot) + 1].w);
#ifndef GSR_ABL_CONTRIB_NOATOMIC
                atomicAdd(hits + eid, (unsigned long long)hv);
                atomicMax(wmax + eid, __float_as_uint(rm));
                atomicAdd(wsum + eid, (double)rs);
#else  // ablation: everything but the three atomics
                asm volatile("" ::"v"(eid), "v"(rm), "v"(rs));
#endif
            }
            __builtin_amdgcn_wave_barrier();  // the next batch overwrites the matrix only after these reads
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
    }
}

// dst[idx[r]]: hits += src, wmax = max, wsum += src -- rows that arrive from other ranks (a Gaussian needed by two bands
// arrives twice, hence atomics); idx[r] < 0: a padding row
__global__ void contrib_merge_rows_kernel(int64_t n, const int32_t *__restrict__ idx,
                                          const unsigned long long *__restrict__ src_hits,
                                          const float *__restrict__ src_wmax, const double *__restrict__ src_wsum,
                                          unsigned long long *__restrict__ dst_hits, unsigned int *__restrict__ dst_wmax,
                                          double *__restrict__ dst_wsum) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t i = idx[r];
    if (i < 0) return;
    // (a component that is zero changes nothing: a row nobody blended on the sender costs no atomic)
    const unsigned long long h = src_hits[r];
    const float m = src_wmax[r];
    const double s = src_wsum[r];
    if (h != 0ull) atomicAdd(dst_hits + i, h);
    if (m > 0.f) atomicMax(dst_wmax + i, __float_as_uint(m));
    if (s != 0.0) atomicAdd(dst_wsum + i, s);
}

}  // namespace

int gsr_launch_composite_contrib(int P, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                 const float *means2D, const float *conic_opacity, const uint8_t *compute_locally,
                                 const int32_t *n_contrib, int row_lo, int row_hi, int64_t *hits, float *wmax,
                                 double *wsum, hipStream_t stream) {
    (void)P;
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    hipLaunchKernelGGL(composite_contrib_kernel, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, W, H, gx,
                       gx * gy, reinterpret_cast<const int2 *>(ranges), point_list,
                       reinterpret_cast<const float2 *>(means2D), reinterpret_cast<const float4 *>(conic_opacity),
                       compute_locally, n_contrib, b.band ? 1 : 0, b.band_first, b.band_tiles,
                       reinterpret_cast<unsigned long long *>(hits), reinterpret_cast<unsigned int *>(wmax), wsum);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_contrib_merge_rows(int64_t n, const int32_t *idx, const int64_t *src_hits, const float *src_wmax,
                                  const double *src_wsum, int64_t *dst_hits, float *dst_wmax, double *dst_wsum,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(contrib_merge_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, idx,
                       reinterpret_cast<const unsigned long long *>(src_hits), src_wmax, src_wsum,
                       reinterpret_cast<unsigned long long *>(dst_hits), reinterpret_cast<unsigned int *>(dst_wmax),
                       dst_wsum);
    GSR_LAUNCH_CHECK();
    return 0;
}
