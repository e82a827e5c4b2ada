// contrib.hip -- per-Gaussian CONTRIBUTION statistics of one rendered view, from the tile lists (gfx950 / wave64).
//
// K8 (composite.hip) decides what every pixel blends; this kernel walks the same lists once more, forward only, and
// tells every Gaussian what it was worth in the image K8 drew: on how many pixels it was blended (`hits`), its largest
// blend weight w = alpha T on any of them (`wmax`: RadSplat's importance) and the sum of its weights (`wsum`:
// LightGaussian's).  A side pass in the shape of tile_walk.h, front to back, the id in the record's last word.  K8 and
// K10 themselves are untouched; a trainer that does not ask for the statistics never launches this kernel.
//
// The reduction over the quadrant's pixels is the LDS transpose over a batch of CB = 8 entries: phase A (lane = pixel)
// walks the batch, carries T, and stores every entry's w (0 where the pixel does not blend it) into a wave-private
// matrix [slot][pixel]; the blend ballot's popcount -- `hits` -- goes into one byte of a scalar register pair.  Phase B (lane = (slot, eighth of the quadrant)) reads its eight pixels with two 16-byte reads, takes
// their max and their sum in pixel order, and three xor steps combine the eighths: a fixed order, fp32.  Lane 8 * slot
// then holds the entry's three values, reads the entry's id from its record, and -- if hits > 0 -- issues three atomics
// into the caller's arrays: a 64-bit integer add, an unsigned 32-bit max on the float's bits (non-negative floats order
// as their bit patterns, so the max is exact and independent of the order) and an fp64 add (the quadrant's fp32 sum,
// widened).  (A 64-lane xor butterfly per entry instead -- twelve dependent cross-lane moves -- measured 3.9 x K8's time
// for this kernel alone; EXPERIMENTS.md.)
// The four quadrant waves of a tile never synchronise: each issues its own atomics, so a row receives at most
// 4 x local tiles fp64 additions per launch.  Rows that are blended nowhere are never written.
#include "common.h"
#include "composite_math.h"
#include "tile_walk.h"

namespace {

constexpr int WSTR = 64 + 4;     // row stride of the w matrix in floats: phase B's 16-byte reads of the 8 slots spread over the banks

__global__ void __launch_bounds__(256)
composite_contrib_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                         const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                         const float4 *__restrict__ conic_opacity, const uint8_t *__restrict__ compute_locally,
                         const int32_t *__restrict__ n_contrib, int band, int band_first, int band_tiles,
                         unsigned long long *__restrict__ hits, unsigned int *__restrict__ wmax,
                         double *__restrict__ wsum) {
    Quadrant qd;
    if (!quadrant_begin(qd, W, H, gx, tiles, ranges, compute_locally, n_contrib, band, band_first, band_tiles)) return;

    __shared__ __attribute__((aligned(16))) float4 slab[4][64 * 2];   // [wave][slot]: {x, y, a2, b2 | c2, o, position + 1, id}
    __shared__ __attribute__((aligned(16))) float wmat[4][CB * WSTR];  // [wave][slot of the batch][pixel] = w
    float4 *wslab = slab[qd.wave];
    float *wm = wmat[qd.wave];
    const int bslot = qd.lane >> 3, bpart = qd.lane & 7;  // phase B: this lane's slot of the batch and its eighth of the pixels
    float T = 1.0f;
    for (int c = 0; c < qd.wlen; c += 64) {  // wave-uniform
        const int nrel = stage_chunk<FRONT_TO_BACK, 2>(
            c, qd.lane, qd.wlen, qd.range.x, qd.qx0, qd.qy0, point_list, means2D, conic_opacity, wslab,
            [](uint32_t id) { return __uint_as_float(id); }, [](int, uint32_t) {}, [](int) {});
        __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
        for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
            // phase A, lane = pixel: alphas are independent, only the short T chain is sequential
            unsigned long long cnt8 = 0ull;  // byte s: the pixels that blended slot s (<= 64), in a scalar register pair
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const float4 q0 = wslab[2 * (b0 + s)], q1 = wslab[2 * (b0 + s) + 1];  // wave-uniform address: LDS broadcasts
                const Pair p = pair_decision(q0, q1, qd.pxf, qd.pyf, qd.last);
                const float w = p.take ? p.alpha * T : 0.f;  // (selected, never multiplied: an inert slot's alpha is not used)
                T -= w;  // T (1 - alpha) as K8 forms it: T - alpha T
                wm[s * WSTR + qd.lane] = w;
                cnt8 |= (unsigned long long)__popcll(__ballot(p.take)) << (8 * s);
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
