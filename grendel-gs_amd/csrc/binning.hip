// binning.hip -- K3..K7 for gfx950: which locally computed tiles each Gaussian touches, and the
// per-tile front-to-back lists.
//
// The reference stage list (analyze_statistic.py:1972-1991 of the reference) is a device-wide
// 64-bit (tile<<32 | depth) CUB sort over all D (tile, Gaussian) pairs.  Here the same ORDER is
// produced with far less HBM traffic by splitting the key:
//   1. stable radix sort of the P Gaussians by depth bits (4 x 8-bit passes over P pairs);
//   2. emit the D pairs in that depth order, (ty, tx)-major inside a Gaussian;
//   3. stable radix sort of the D pairs by tile only: keys (row << xbits | column), pass 0 by column, pass 1 by row
//      (frames of <= 256 x 256 tiles; larger frames sort tile ids in ceil(log2(tiles)/8) passes).
// A stable sort by tile of a depth-ordered sequence is exactly the (tile, depth, arrival)
// order of SURVEY.md A.3.  Traffic: ~64 B per Gaussian + ~32 B per pair instead of ~200 B per pair.
//
// At the sizes of one camera (1e6 Gaussians, 1e7 pairs) every kernel of this stage lasts 10-70 us, so
// the stage is bound by the NUMBER of dependent launches as much as by bytes.  The sort is therefore a
// "one sweep" radix sort: the digit histograms of all passes are known BEFORE the keys are sorted -- the depth
// histograms are accumulated by K3 while it writes the keys, and the tile-sort histograms follow from the rects
// alone (a w x h rect adds h to every column digit it spans and w to every row digit) -- and each pass is a single
// kernel that obtains its workgroup's global digit offsets by decoupled look-back over the preceding
// workgroups' per-digit counts (no histogram / scan launches between passes).  Step 2 is fused into the first
// pass of step 3 (emit_scatter_kernel): the pairs are decoded into registers and scattered, never stored
// unsorted.  The offsets scan of K4 is a single-pass look-back scan that gathers its input through the sorted
// order.  Workgroups take their tile from a ticket counter, so a workgroup only ever waits for workgroups that
// are already running (forward progress without co-residency assumptions).
//
// All primitives are hand-written for wave64: ballot-based stable multisplit inside a wave,
// LDS per-wave digit tables, LDS digit-ordered staging for coalesced stores.
//
// The kernels of this file are the LOOK-BACK pipeline (nine launches) and the generic tile-id sort.  The same lists come
// out of K3-K4 as one persistent launch and K5-K7 as another (binning_persist.h: short chains, where launches dominate)
// and out of the row-major pipeline (binning_rows.h: one pass over the pairs, long chains).  Which of them runs is
// decided on the host, once per call, in binning_host.h: the prepare step tries the persistent kernel and falls back to
// the look-back chain; the form of the D-chain is a SortPlan (row-major, else (row, column) keys with the persistent
// sort kernel in front of the two look-back passes, else generic).  The second half of this file holds one launch
// function per form and the C entry points.
#include "common.h"

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "radix.h"
#ifndef GSR_EMIT_DECODE_BATCH
#define GSR_EMIT_DECODE_BATCH 2
#endif
#include "binning_persist.h"
#include "binning_rows.h"
#include "binning_host.h"

namespace {

// ------------------------------------------------------------ K4: offsets = exclusive scan of tt[ids[.]]
// Single pass with decoupled look-back (wave 0 inspects 64 predecessors per round).  out[n] = total.
__global__ void __launch_bounds__(SCAN_THREADS)
scan_gather_lookback_kernel(const uint32_t *__restrict__ src, int packed,
                            const uint32_t *__restrict__ idx, uint32_t *__restrict__ out, uint32_t *__restrict__ out2,
                            long long n, unsigned long long *__restrict__ state, uint32_t *__restrict__ ticket, int nb,
                            uint32_t *__restrict__ host_total, uint32_t seq,
                            const unsigned long long *__restrict__ early) {
    // Two scans in one sweep (round 6): out = exclusive scan of the pairs per Gaussian (-> the offsets of the Gaussian-major
    // emission) and out2 = exclusive scan of the rows of the Gaussian's rect (-> its row segments, binning_rows.h).  K3
    // leaves both in ONE word per Gaussian (`packed`: pairs | rows << 20 on frames of <= 256 x 256 tiles; else the pairs
    // alone): one random gather per element, as before the second scan existed.  Both running sums stay below 2^31
    // (RADIX_MAX_N) and share the 62 value bits of the look-back word: low 31 bits pairs, high 31 bits segments.
    __shared__ uint32_t smem[4];
    __shared__ uint32_t s_bid;
    __shared__ unsigned long long s_excl;
    if (threadIdx.x == 0) s_bid = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t bid = s_bid;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // each thread owns SCAN_ITEMS CONSECUTIVE elements so that one workgroup scan suffices
    const long long base = (long long)bid * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS], v2[SCAN_ITEMS];
    uint32_t s = 0, s2 = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        const uint32_t x = (base + k < n) ? src[idx[base + k]] : 0u;
        v[k] = packed ? (x & TT_MASK) : x;
        v2[k] = packed ? (x >> TT_SHIFT) : 0u;
        s += v[k];
        s2 += v2[k];
    }
    uint32_t tot, tot2;
    const uint32_t local = block_exclusive_scan(s, smem, &tot);
    const uint32_t local2 = block_exclusive_scan(s2, smem, &tot2);
    const unsigned long long tot64 = (unsigned long long)tot | ((unsigned long long)tot2 << 31);
    if (wave == 0) {
        if (lane == 0) st_agent64(&state[bid], tot64 | (bid == 0 ? LB64_PRE : LB64_AGG));
        unsigned long long excl = 0;
        if (bid > 0) {
            long long top = (long long)bid - 1;
            while (true) {
                const long long j = top - lane;
                unsigned long long x = j >= 0 ? ld_agent64(&state[j]) : LB64_PRE;  // virtual zero prefix before 0
                int fp;
                while (true) {
                    const unsigned long long empty = __ballot((x >> 62) == 0ull);
                    const unsigned long long pre = __ballot((x >> 62) >= 2ull);
                    fp = pre ? __ffsll((long long)pre) - 1 : 64;
                    const unsigned long long need = fp >= 63 ? ~0ull : ((2ull << fp) - 1ull);
                    if ((empty & need) == 0ull) break;
                    __builtin_amdgcn_s_sleep(1);
                    if ((x >> 62) == 0ull) x = ld_agent64(&state[j]);
                }
                unsigned long long part = lane <= fp ? (x & LB64_VAL) : 0ull;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
                excl += part;
                if (fp < 64) break;
                top -= 64;
            }
        }
        if (lane == 0) {
            if (bid > 0) st_agent64(&state[bid], ((excl + tot64) & LB64_VAL) | LB64_PRE);
            s_excl = excl;
            if ((int)bid == nb - 1) {
                // (the pair count on the device comes from K3's clean 64-bit sum when given: the packed low half would
                // wrap at 2^31 pairs, which the callers must see as "too many"; the host gets it from K3 as well)
                const unsigned long long dsum = early ? *early : ((excl + tot64) & 0x7FFFFFFFull);
                out[n] = clamp_pair_count(dsum);
                out2[n] = (uint32_t)((excl + tot64) >> 31) & 0x7FFFFFFFu;
                if (host_total) {
                    __hip_atomic_store(host_total, clamp_pair_count(dsum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(host_total + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
    }
    __syncthreads();
    uint32_t run = (uint32_t)(s_excl & 0x7FFFFFFFull) + local;
    uint32_t run2 = (uint32_t)((s_excl >> 31) & 0x7FFFFFFFull) + local2;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (base + k < n) {
            out[base + k] = run;
            out2[base + k] = run2;
        }
        run += v[k];
        run2 += v2[k];
    }
}

// ---------------------------------------------------------------------------------- K3 and friends
// K3: per Gaussian, the tile rect it can CONTRIBUTE to and the number of its tiles; depth sort keys and
// the digit histograms of the four depth-sort passes.
// The rect is the reference's 3-sigma-radius rect intersected with the
// bounding box of the alpha >= 1/255 ellipse (gsr_alpha_extent) and with the mask's row hull: tiles
// dropped by the intersection cannot receive a contribution under the alpha < 1/255 rule of A.4, so
// the image is unchanged while D (pairs to sort and to walk) shrinks.  Gaussians touching nothing get
// key 0xFFFFFFFF (depths are > 0.2, so real keys are < 0x7F800000) and sort to the end.
// Row hull of the locally computed tiles (computed by every workgroup from the 8-32 KB mask):
// [first tile row with a local tile, one past the last).  Grendel's final mode always passes whole-row
// bands, for which the hull IS the mask; for a general mask the tiles inside the hull that are not
// local are emitted with a sentinel key.
constexpr int TC_THREADS = 1024, TC_BLOCKS = 256;  // 16-wave persistent workgroups, one per CU (measured best)
__global__ void __launch_bounds__(TC_THREADS)
touch_count_kernel(int P, int gx, int gy, const float2 *__restrict__ means2D, const float *__restrict__ depths,
                   const int32_t *__restrict__ radii, const float4 *__restrict__ conic_opacity,
                   const uint8_t *__restrict__ mask, RadixPlan plan, uint32_t *__restrict__ tt,
                   uint32_t *__restrict__ keys, uint32_t *__restrict__ vals, TileRect *__restrict__ rects,
                   uint32_t *__restrict__ ghist, uint32_t *__restrict__ tile_hist, int32_t *__restrict__ hull_out,
                   int cull, unsigned long long *__restrict__ early, uint32_t *__restrict__ host_total, uint32_t seq,
                   uint4 *__restrict__ zero16, size_t zero16_n) {
    // (round 6) the control block of the tile sort that follows on this stream is cleared here instead of by a fill
    // launch between the two steps (gsr_bin_speculative_async)
    for (size_t i = (size_t)blockIdx.x * TC_THREADS + threadIdx.x; i < zero16_n; i += (size_t)gridDim.x * TC_THREADS)
        zero16[i] = make_uint4(0u, 0u, 0u, 0u);
    __shared__ int s_lo, s_hi;
    __shared__ unsigned long long s_nsum[TC_THREADS / 64];
    unsigned long long nsum = 0;  // this thread's share of the pair count D = sum of tiles_touched
    __shared__ uint32_t mh[RADIX_MAX_PASSES][RADIX_DIGITS];
    // digit histograms of the TILE sort (keys (y, x): pass 0 = column, pass 1 = row), known here without looking at
    // a single pair: a rect of w x h tiles adds h to every column digit in [minx, maxx) and w to every row digit in
    // [miny, maxy) -- two +/- entries in a difference array each, prefix-summed once per workgroup
    __shared__ int32_t dxy[3][RADIX_DIGITS + 1];
    __shared__ uint32_t tc_scan[TC_THREADS / 64];
    if (threadIdx.x <= RADIX_DIGITS) dxy[0][threadIdx.x] = dxy[1][threadIdx.x] = dxy[2][threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_lo = gy; s_hi = 0; }
    if (threadIdx.x < RADIX_DIGITS)
        for (int p = 0; p < RADIX_MAX_PASSES; p++) mh[p][threadIdx.x] = 0;
    __syncthreads();
    {  // every thread inspects a contiguous slice of the mask; rows are monotone in the byte index
        const int total = gx * gy;
        const int per = (total + TC_THREADS - 1) / TC_THREADS;
        const int b0 = threadIdx.x * per, b1 = min(b0 + per, total);
        int first = -1, last = -1;
        for (int b = b0; b < b1; b++)
            if (mask[b]) {
                if (first < 0) first = b;
                last = b;
            }
        if (first >= 0) {
            atomicMin(&s_lo, first / gx);
            atomicMax(&s_hi, last / gx + 1);
        }
    }
    __syncthreads();
    const int hull0 = s_lo, hull1 = s_hi;
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // K8 / K10 spread THE BAND over the XCDs (gsr_xcd_span_of_block_band)
        hull_out[0] = hull1 > hull0 ? hull0 : 0;
        hull_out[1] = hull1 > hull0 ? hull1 : 0;
    }
    for (long long base = (long long)blockIdx.x * TC_THREADS; base < P; base += (long long)gridDim.x * TC_THREADS) {
        const long long i = base + threadIdx.x;
        const bool valid = i < P;
        uint32_t key = 0xFFFFFFFFu;
        if (valid) {
            uint32_t n = 0;
            TileRect rect{0u, 0u, 0ull};
            const int rad = radii[i];
            if (rad > 0) {
                const float2 xy = means2D[i];
                const float4 co = conic_opacity[i];
                float ex, ey;
                if (gsr_alpha_extent(co, ex, ey)) {
                    int minx, miny, maxx, maxy;
                    gsr_get_rect(xy.x, xy.y, rad, gx, gy, minx, miny, maxx, maxy);
                    miny = max(miny, hull0);
                    maxy = min(maxy, hull1);
                    gsr_narrow_span(xy.x, ex, minx, maxx);
                    gsr_narrow_span(xy.y, ey, miny, maxy);
                    // (the tile count, the exact tile mask when culling is on, the tile sort's digit histograms)
                    if (maxx > minx && maxy > miny)
                        n = gsr_rect_tiles(xy, co, minx, miny, maxx, maxy, cull != 0, tile_hist ? dxy : nullptr, rect);
                }
            }
            if (n) key = __float_as_uint(depths[i]);
            nsum += n;
            // (with the rows of the rect -- its row segments, binning_rows.h -- in the upper bits on the (row, column) path)
            tt[i] = (tile_hist && n) ? (n | (((rect.ys >> 16) - (rect.ys & 0xFFFFu)) << TT_SHIFT)) : n;
            rects[i] = rect;
            keys[i] = key;
            vals[i] = (uint32_t)i;
        }
        multihist_add(mh, plan, key, valid);
    }
    nsum = wave_sum64(nsum);
    if ((threadIdx.x & 63) == 0) s_nsum[threadIdx.x >> 6] = nsum;
    __syncthreads();
    if (threadIdx.x == 0) {  // the pair count reaches the host HERE, not four sort passes and a scan later
        unsigned long long tot = 0;
        for (int wv = 0; wv < TC_THREADS / 64; wv++) tot += s_nsum[wv];
        publish_pair_count(early, tot, gridDim.x, host_total, seq);
    }
    multihist_flush(mh, plan, ghist);
    if (tile_hist) {  // kernel-uniform
        const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u;  // HW_REG_XCC_ID[3:0]
        for (int p = 0; p < 3; p++) {
            const uint32_t v = threadIdx.x < RADIX_DIGITS ? (uint32_t)dxy[p][threadIdx.x] : 0u;
            uint32_t all;
            const uint32_t c = block_exclusive_scan_n<TC_THREADS / 64>(v, tc_scan, &all) + v;  // inclusive: the count
            if (threadIdx.x < RADIX_DIGITS && c)
                __hip_atomic_fetch_add(&tile_hist[(xcc * RADIX_MAX_PASSES + p) * RADIX_DIGITS + threadIdx.x], c,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// K5: the D output pairs are cut into chunks of EMIT_CHUNK slots, one wave per chunk, so the work is
// balanced by OUTPUT (a near-camera splat covering thousands of tiles no longer serialises one wave).
// The wave finds the Gaussian that owns its first slot with a 64-ary search over the offsets (one
// coalesced probe per round), then walks windows of 64 depth-consecutive Gaussians staged in LDS; every
// slot locates its owner by a 6-step binary search in the window and is written with coalesced stores.
// The digit histograms of the tile-sort passes are accumulated on the way.
constexpr int EMIT_CHUNK = 1024;  // slots per wave (measured: 512-1024 best, 4096 8 % slower)
__global__ void __launch_bounds__(256)
emit_pairs_kernel(int P, long long D, int gx, int tiles, const TileRect *__restrict__ rects,
                  const uint8_t *__restrict__ mask, const uint32_t *__restrict__ sorted_ids,
                  const uint32_t *__restrict__ offsets, RadixPlan plan, uint32_t *__restrict__ keys,
                  uint32_t *__restrict__ vals, uint32_t *__restrict__ ghist) {
    __shared__ uint32_t s_off[4][65];
    __shared__ uint32_t s_g[4][64];
    __shared__ uint2 s_rect[4][64];
    __shared__ uint32_t mh[RADIX_MAX_PASSES][RADIX_DIGITS];
    for (int p = 0; p < RADIX_MAX_PASSES; p++) mh[p][threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long sb = ((long long)blockIdx.x * 4 + wave) * EMIT_CHUNK; sb < D;
         sb += (long long)gridDim.x * 4 * EMIT_CHUNK) {
        const uint32_t s_begin = (uint32_t)sb;
        const uint32_t s_end = (uint32_t)(sb + EMIT_CHUNK < D ? sb + EMIT_CHUNK : D);
        // largest j in [0, P] with offsets[j] <= s_begin  (offsets is non-decreasing, offsets[P] = D > s_begin)
        int lo = 0, hi = P;  // invariant: offsets[lo] <= s_begin < offsets[hi]
        while (hi - lo > 1) {
            const int step = (hi - lo + 63) / 64;
            const int idx = min(lo + lane * step, hi);
            const bool le = offsets[idx] <= s_begin;
            const int c = __popcll(__ballot(le));  // probes are monotone: the first c lanes say "<="
            const int nlo = lo + (c - 1) * step;
            hi = min(hi, nlo + step);
            lo = nlo;
        }
        int g0 = lo;
        uint32_t s = s_begin + lane;
        while (true) {  // one window of 64 Gaussians per iteration (wave-uniform control flow)
            const int j = g0 + lane;
            const uint32_t off = offsets[min(j, P)];
            const uint32_t end = offsets[min(j + 1, P)];
            const uint32_t g = (j < P && end > off) ? sorted_ids[j] : 0u;
            __builtin_amdgcn_wave_barrier();
            s_off[wave][lane] = off;
            if (lane == 63) s_off[wave][64] = end;
            s_g[wave][lane] = g;
            // (frames above 256 x 256 tiles: K3 keeps every tile of the rect, the mask is not looked at)
            s_rect[wave][lane] = (j < P && end > off) ? make_uint2(rects[g].xs, rects[g].ys) : make_uint2(0u, 0u);
            __builtin_amdgcn_wave_barrier();
            const uint32_t wend = min(__builtin_amdgcn_readlane(end, 63), s_end);
            while (__ballot(s < wend) != 0ull) {  // wave-uniform trip count (the histogram uses ballots)
                const bool valid = s < wend;
                uint32_t key = 0;
                if (valid) {
                    int a = 0, bnd = 63;
#pragma unroll
                    for (int it = 0; it < 6; it++) {
                        const int mid = (a + bnd + 1) >> 1;
                        if (s_off[wave][mid] <= s) a = mid; else bnd = mid - 1;
                    }
                    const uint2 r = s_rect[wave][a];
                    const uint32_t t = s - s_off[wave][a];
                    const uint32_t minx = r.x & 0xFFFFu, w = (r.x >> 16) - minx, miny = r.y & 0xFFFFu;
                    const uint32_t y = miny + t / w, x = minx + t % w;
                    const uint32_t tile = y * (uint32_t)gx + x;
                    key = mask[tile] ? tile : (uint32_t)tiles;  // non-local tile in the hull: sentinel, sorts last
                    keys[s] = key;
                    vals[s] = s_g[wave][a];
                }
                multihist_add(mh, plan, key, valid);
                if (valid) s += 64;
            }
            if (wend >= s_end) break;
            g0 += 64;
        }
    }
    __syncthreads();
    multihist_flush(mh, plan, ghist);
}

// K5 + first pass of K6 in one kernel (frames of <= 256 x 256 tiles).  The tile sort uses keys (row << xbits | column):
// pass 0 sorts by column, pass 1 by row, and both digit histograms are already known (K3).  So the pairs need not
// be written unsorted and read back: the workgroup that owns slots [4096 b, 4096 b + 4096) of the emission order
// decodes them into registers (owner search as in emit_pairs_kernel, one window of 64 depth-consecutive Gaussians
// at a time) and runs the pass-0 scatter on them directly.  All tiles of the rect are emitted, computed locally
// or not: K7 leaves the ranges of tiles that are not computed locally empty, and K8 / K10 never look at them.
template <int ITEMS, int THREADS>
__global__ void __launch_bounds__(THREADS, 8)  // <= 64 VGPRs: four 8-wave workgroups per CU
emit_scatter_kernel(int P, long long D, int xbits, const TileRect *__restrict__ rects,
                    const uint32_t *__restrict__ sorted_ids, const uint32_t *__restrict__ offsets,
                    const uint32_t *__restrict__ ghist, uint32_t *__restrict__ state, uint32_t *__restrict__ ticket,
                    uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out, bool bounded,
                    int32_t *__restrict__ ranges_flat, int ranges_words, const int32_t *__restrict__ hull) {
    constexpr int WAVES = THREADS / 64;
    __shared__ OnesweepSmem<ITEMS, THREADS> sm;
    // K7 only writes the tiles that own pairs: clear the range table here (it runs two kernels later on this stream)
    // instead of in a memset launch of its own.  Every workgroup takes part, before any of the early exits below.
    for (int t = blockIdx.x * THREADS + threadIdx.x; t < ranges_words; t += gridDim.x * THREADS) ranges_flat[t] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 2) ranges_flat[ranges_words + threadIdx.x] = hull[threadIdx.x];  // row `tiles`
    if (bounded) {  // the grid covers a capacity D; the true pair count is offsets[P] (K4's total)
        const long long d = offsets[P];
        if (d > D) return;
        D = d;
    }
    __shared__ uint32_t cflag[WAVES][ITEMS * 64 / 32];  // decode_chunk's 512 start bits per wave
    const uint32_t bid = onesweep_begin(sm, ticket);
    if ((long long)bid * (ITEMS * THREADS) >= D) return;
    const int wave = threadIdx.x >> 6;
    const long long wbase = (long long)bid * (ITEMS * THREADS) + (long long)wave * (ITEMS * 64);
    uint32_t key[ITEMS], val[ITEMS];
#pragma unroll
    for (int r = 0; r < ITEMS; r++) { key[r] = 0xFFFFFFFFu; val[r] = 0u; }
    if (wbase < D) {  // wave-uniform
        // the Gaussian that owns the chunk's first slot (64-ary search over the offsets), then the flag-word decode of
        // binning_persist.h (round 5: replaces the per-slot binary search in LDS windows of 64 Gaussians -- ~30 VALU
        // instructions per pair in a kernel that is 60-76 % VALU-busy -- by one broadcast read and a population count)
        const int g0 = owner_search(offsets, 0, P, (uint32_t)wbase);
        static_assert(ITEMS == PS_ITEMS, "decode_chunk decodes 8 rounds of 64 slots");
        decode_chunk<GSR_EMIT_DECODE_BATCH>(offsets, sorted_ids, rects, P, D, wbase, g0, xbits, cflag[wave], key, val);
    }
    onesweep_scatter(sm, key, val, bid, D, 0, xbits, ghist, state, keys_out, vals_out);
}

// K7 for (row << xbits | column) keys: four consecutive sorted pairs per thread; tiles that are not computed
// locally keep the empty range
__global__ void __launch_bounds__(GSR_ONE_DIM_BLOCK)
tile_ranges_yx_kernel(long long D, int gx, int xbits, const uint32_t *__restrict__ keys,
                      const uint8_t *__restrict__ mask, int2 *__restrict__ ranges,
                      const uint32_t *__restrict__ D_dev) {
    if (D_dev) {
        const long long d = *D_dev;
        if (d > D) return;
        D = d;
    }
    const long long j = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (j >= D) return;
    uint32_t k[6];  // k[0] = predecessor, k[1..4] = own, k[5] = successor
    k[0] = j > 0 ? keys[j - 1] : 0xFFFFFFFFu;
    if (j + 4 <= D) {
        const uint4 q = *reinterpret_cast<const uint4 *>(keys + j);
        k[1] = q.x; k[2] = q.y; k[3] = q.z; k[4] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) k[1 + i] = j + i < D ? keys[j + i] : 0xFFFFFFFFu;
    }
    k[5] = j + 4 < D ? keys[j + 4] : 0xFFFFFFFFu;
    const uint32_t xmask = (1u << xbits) - 1u;
#pragma unroll
    for (int i = 1; i <= 4; i++) {
        if (j + i - 1 >= D) break;
        const uint32_t kk = k[i];
        if (k[i - 1] != kk || k[i + 1] != kk) {
            const uint32_t t = (kk >> xbits) * (uint32_t)gx + (kk & xmask);
            if (!mask[t]) continue;
            if (k[i - 1] != kk) ranges[t].x = (int)(j + i - 1);
            if (k[i + 1] != kk) ranges[t].y = (int)(j + i);
        }
    }
}

// K7: four consecutive sorted pairs per thread
__global__ void __launch_bounds__(GSR_ONE_DIM_BLOCK)
tile_ranges_kernel(long long D, uint32_t tiles, const uint32_t *__restrict__ tile_of, int2 *__restrict__ ranges) {
    const long long j = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (j >= D) return;
    uint32_t k[6];  // k[0] = predecessor, k[1..4] = own, k[5] = successor
    k[0] = j > 0 ? tile_of[j - 1] : 0xFFFFFFFFu;
    if (j + 4 <= D) {
        const uint4 q = *reinterpret_cast<const uint4 *>(tile_of + j);
        k[1] = q.x; k[2] = q.y; k[3] = q.z; k[4] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) k[1 + i] = j + i < D ? tile_of[j + i] : 0xFFFFFFFFu;
    }
    k[5] = j + 4 < D ? tile_of[j + 4] : 0xFFFFFFFFu;
#pragma unroll
    for (int i = 1; i <= 4; i++) {
        if (j + i - 1 >= D) break;
        const uint32_t t = k[i];
        if (t >= tiles) continue;
        if (k[i - 1] != t) ranges[t].x = (int)(j + i - 1);
        if (k[i + 1] != t) ranges[t].y = (int)(j + i);
    }
}

// Optional (gsr_set_depth_tie_order(1)): order Gaussians of EXACTLY equal depth by their screen position instead of by
// their arrival index.  The reference breaks depth ties by the index in the array the op is given -- at world size
// > 1 that is (source rank, index on the source), gaussian_renderer/__init__.py:624-640 -- so two runs that shard or
// order the same Gaussians differently composite tied pairs in different orders (measured on the bench scene, whose
// generator produces ~N^2 / 3.6e7 exact ties: 1e-4 .. 1e-3 relative on the gradients).  (x, y) of means2D does not depend
// on who computed it.  After the stable depth sort tied Gaussians are adjacent: the first thread of a run (runs are a
// handful of elements; culled Gaussians, key 0xFFFFFFFF, are not a run) insertion-sorts its ids in place.
__global__ void __launch_bounds__(GSR_ONE_DIM_BLOCK)
depth_tie_fixup_kernel(long long n, const uint32_t *__restrict__ keys, uint32_t *__restrict__ ids,
                       const float2 *__restrict__ means2D) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k == 0xFFFFFFFFu || (i > 0 && keys[i - 1] == k) || i + 1 >= n || keys[i + 1] != k) return;
    long long e = i + 2;
    while (e < n && keys[e] == k) e++;
    auto before = [&](uint32_t a, uint32_t b) {
        const float2 pa = means2D[a], pb = means2D[b];
        if (pa.x != pb.x) return pa.x < pb.x;
        if (pa.y != pb.y) return pa.y < pb.y;
        return a < b;
    };
    for (long long a = i + 1; a < e; a++) {
        const uint32_t v = ids[a];
        long long b = a - 1;
        while (b >= i && before(v, ids[b])) {
            ids[b + 1] = ids[b];
            b--;
        }
        ids[b + 1] = v;
    }
}

__global__ void __launch_bounds__(GSR_ONE_DIM_BLOCK)
copy_u32_kernel(long long n, const uint32_t *__restrict__ src, uint32_t *__restrict__ dst) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dst[j] = src[j];
}
// ------------------------------------------------------------------------------------------ K3-K4: the prepare step
// K3-K4 on the look-back pipeline: K3, four one-sweep passes, the offsets scan (six launches)
int prepare_lookback(const PrepCall &c, const BinFrame &f, BinDevice &d, uint32_t *ticket) {
    const int P = c.P;
    hipStream_t stream = c.stream;
    const PrepLayout L = prep_layout(P);
    const PrepViews v = views(L, c.prep);
    GSR_HIP(hipMemsetAsync(v.early, 0, (L.ctrl - L.early) + L.C.total, stream));
    const RadixPlan plan = radix_plan(0, 32);
    uint32_t *host_total = nullptr;
    uint32_t seq = 0;
    int rc = take_ticket(d, &host_total, &seq);
    if (rc) return rc;
    uint32_t *tile_hist = f.yx ? v.thist : nullptr;
    // persistent workgroups (mask hull + LDS tables are per-workgroup set-up)
    const int blocks = gsr_div_up(P, TC_THREADS) < TC_BLOCKS ? gsr_div_up(P, TC_THREADS) : TC_BLOCKS;
    hipLaunchKernelGGL(touch_count_kernel, dim3(blocks), dim3(TC_THREADS), 0, stream, P, f.gx, f.gy,
                       reinterpret_cast<const float2 *>(c.means2D), c.depths, c.radii,
                       reinterpret_cast<const float4 *>(c.conic_opacity), c.compute_locally, plan, v.tt, v.kA, v.vA, v.rects,
                       reinterpret_cast<uint32_t *>(v.ctrl + L.C.ghist), tile_hist, v.hull, f.cull, v.early, host_total,
                       seq, reinterpret_cast<uint4 *>(c.zero_ptr), c.zero_bytes / 16);
    int in_first = 1;
    rc = radix_sort_pairs(v.kA, v.vA, v.kB, v.vB, P, plan, v.ctrl, L.C, &in_first, stream, nullptr);
    if (rc) return rc;
    // 4 passes -> back in (kA, vA); the sorted ids stay in vA for K5
    uint32_t *sorted_ids = in_first ? v.vA : v.vB;
    if (!in_first) {
        hipLaunchKernelGGL(copy_u32_kernel, dim3(gsr_div_up(P, GSR_ONE_DIM_BLOCK)), dim3(GSR_ONE_DIM_BLOCK), 0, stream,
                           (long long)P, v.vB, v.vA);
        sorted_ids = v.vA;
    }
    if (g_tie_order.load(std::memory_order_relaxed) == 1)
        hipLaunchKernelGGL(depth_tie_fixup_kernel, dim3(gsr_div_up(P, GSR_ONE_DIM_BLOCK)), dim3(GSR_ONE_DIM_BLOCK), 0,
                           stream, (long long)P, in_first ? v.kA : v.kB, sorted_ids,
                           reinterpret_cast<const float2 *>(c.means2D));
    const int nbs = gsr_div_up(P, SCAN_TILE);
    hipLaunchKernelGGL(scan_gather_lookback_kernel, dim3(nbs), dim3(SCAN_THREADS), 0, stream, v.tt,
                       tile_hist ? 1 : 0, sorted_ids, v.offsets, v.segoff, (long long)P,
                       reinterpret_cast<unsigned long long *>(v.ctrl + L.C.scan_state),
                       reinterpret_cast<uint32_t *>(v.ctrl + L.C.tickets), nbs, (uint32_t *)nullptr, seq, v.early);
    GSR_LAUNCH_CHECK();
    *ticket = seq;
    return 0;
}

// K3-K4 as ONE persistent launch (binning_persist.h).  -> 0 launched, 1 not applicable here (use the look-back
// pipeline), otherwise an error
int prepare_persistent(const PrepCall &c, const BinFrame &f, const BinHooks &h, BinDevice &d, uint32_t *ticket) {
    if (!(persist_effective_mode() & PERSIST_P) || g_tie_order.load(std::memory_order_relaxed) != 0) return 1;
    persist_caps(d);
    const int grid_p = lowered(h.grid_p, d.grid_p);
    // tiles of 4096 Gaussians, or of 8192 when that brings the launch down to one tile per workgroup
    long long nb = radix_blocks(c.P);
    int items = 4;
    if (nb > grid_p && (nb + 1) / 2 <= grid_p) {
        items = 8;
        nb = (nb + 1) / 2;
    }
    const int G = (int)(nb < grid_p ? nb : grid_p);
    if (G <= 0 || nb > (long long)G * h.max_tpw) return 1;  // (long sorts are bandwidth-bound: look-back pipeline)
    const long long admit = persist_admit(d, c.stream);
    if (admit < 0) return 1;
    const int P = c.P;
    const PrepLayout L = prep_layout(P);
    const PrepViews v = views(L, c.prep);
    const PersistLayoutP PL = persist_layout_p(G);
    GSR_HIP(hipMemsetAsync(v.early, 0, (L.ctrl - L.early) + PL.zero_bytes, c.stream));
    uint32_t *host_total = nullptr;
    uint32_t seq = 0;
    const int rc = take_ticket(d, &host_total, &seq);
    if (rc) return rc;
    PrepPersistArgs a{};
    a.P = P; a.gx = f.gx; a.gy = f.gy;
    a.means2D = reinterpret_cast<const float2 *>(c.means2D);
    a.conic_opacity = reinterpret_cast<const float4 *>(c.conic_opacity);
    a.depths = c.depths; a.radii = c.radii; a.mask = c.compute_locally;
    a.tt = v.tt; a.kA = v.kA; a.vA = v.vA; a.kB = v.kB; a.vB = v.vB;
    a.offsets = v.offsets; a.segoff = v.segoff; a.rects = v.rects;
    a.tile_hist = f.yx ? v.thist : nullptr;
    a.cull = f.cull;
    a.hull_out = v.hull;
    a.early = v.early;
    a.zero16 = reinterpret_cast<uint4 *>(c.zero_ptr);
    a.zero16_n = c.zero_bytes / 16;
    a.sync = sync_view(v.ctrl + PL.sync, G);
    a.tstamp = timeline_buffer(h.timeline, 0, G);
    a.grp = at<uint32_t>(v.ctrl, PL.grp); a.cnt = at<uint32_t>(v.ctrl, PL.cnt);
    a.wtot = at<unsigned long long>(v.ctrl, PL.wtot); a.bins = at<uint32_t>(v.ctrl, PL.bins);
    a.depth_buckets = h.depth_buckets ? 1 : 0;
    a.host_total = host_total; a.seq = seq;
    a.done_word = d.done; a.done_seq = (uint32_t)admit;
    a.timeout_ticks = 5000000ull;  // 50 ms of the 100 MHz clock at the first barrier
    a.force_abort = h.abort_p ? 1 : 0;
    if (items == 4) hipLaunchKernelGGL(bin_prepare_persist_kernel<4>, dim3(G), dim3(PP_THREADS), 0, c.stream, a);
    else hipLaunchKernelGGL(bin_prepare_persist_kernel<8>, dim3(G), dim3(PP_THREADS), 0, c.stream, a);
    GSR_LAUNCH_CHECK();
    *ticket = seq;
    return 0;
}

// ------------------------------------------------------------------------------------------- K5-K7: the tile sort
// what the four launch functions are given.  `bounded`: D is a CAPACITY; the kernels read the pair count from the prep
// workspace (K4's total) and do nothing past it
struct SortCall {
    BinFrame f;
    int P;
    const uint8_t *mask;
    PrepViews pv;  // (read only)
    int64_t D;
    void *scratch;
    uint32_t *point_list;
    int32_t *ranges;
    hipStream_t stream;
    bool bounded;
};

// the row-major pipeline (binning_rows.h): segments by row, their scan, ONE pass over the pairs
int launch_rows(const SortCall &s, const BinHooks &h, const BinDevice &d) {
    const BinFrame &f = s.f;
    const int P = s.P, gx = f.gx, gy = f.gy;
    const long long D = s.D;
    const RowsLayout R = rows_layout(D, gx, gy);
    auto u32 = [&s](size_t off) { return at<uint32_t>(s.scratch, off); };
    uint32_t *tickets = u32(R.tickets), *seg_key = u32(R.seg_key), *seg_gid = u32(R.seg_gid), *pairoff = u32(R.pairoff);
    uint32_t *tilebase = u32(R.tilebase);
    int32_t *tdiff = at<int32_t>(s.scratch, R.tdiff), *chunk_owner = at<int32_t>(s.scratch, R.chunk_owner);
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, (int)(&d - g_bin_devices));
    const uint32_t *thist = s.pv.thist, *segoff = s.pv.segoff, *offsets = s.pv.offsets;
    // grids: tiles are taken by ticket inside the kernels, so a grid only has to fill the device (the segment count
    // is not known on the host, and the pair count only as a capacity in a bounded launch)
    constexpr int TILE_B = 8 * ROWS_THREADS_B, TILE_D = 8 * ROWS_THREADS_D;
    auto tickets_of = [](long long tiles) { return (tiles + TICKET_TILES - 1) / TICKET_TILES; };
    const long long nbB = (D + TILE_B - 1) / TILE_B;
    const int fill_b = cus * 2, fill_d = cus * h.rows_fill_d;
    const int grid_b = (int)(tickets_of(nbB) < fill_b ? tickets_of(nbB) : fill_b);
    const long long nbs = (D + SEGSCAN_TILE - 1) / SEGSCAN_TILE;
    // (every workgroup costs a ticket -- an atomic on one word, ~15 ns each when hammered -- whether it finds work or not,
    // and the segment count is typically D / 3..6: a grid of two workgroups per CU loops over the tiles instead)
    const int grid_c = (int)(tickets_of(nbs) < cus * 2 ? tickets_of(nbs) : cus * 2);
    const long long nbt = (D + TILE_D - 1) / TILE_D + gy;
    const int grid_d = (int)(tickets_of(nbt) < fill_d ? tickets_of(nbt) : fill_d);
    hipLaunchKernelGGL((seg_scatter_kernel<8, ROWS_THREADS_B>), dim3(grid_b), dim3(ROWS_THREADS_B), 0, s.stream, P, D,
                       f.ybits, s.pv.rects, s.pv.vA, offsets, segoff, thist + 2 * RADIX_DIGITS, u32(R.seg_state), tickets,
                       seg_key, seg_gid, s.bounded, s.ranges, 2 * gx * gy, s.pv.hull, tdiff,
                       RADIX_REPLICAS * gy * (gx + 1));
    hipLaunchKernelGGL(seg_scan_kernel, dim3(grid_c), dim3(SCAN_THREADS), 0, s.stream, P, D, gx, gy, offsets, segoff,
                       seg_key, pairoff, at<unsigned long long>(s.scratch, R.scan_state), tickets + 1, tdiff, thist,
                       chunk_owner, s.bounded);
    hipLaunchKernelGGL(tile_base_kernel, dim3(gy), dim3(GSR_ONE_DIM_BLOCK), 0, s.stream, P, D, gx, gy, offsets, thist,
                       tdiff, s.mask, tilebase, reinterpret_cast<int2 *>(s.ranges), s.bounded);
    hipLaunchKernelGGL((pair_scatter_kernel<8, ROWS_THREADS_D>), dim3(grid_d), dim3(ROWS_THREADS_D), 0, s.stream, P, D, gx,
                       gy, f.xbits, offsets, segoff, seg_key, seg_gid, pairoff, thist, tilebase, chunk_owner, u32(R.pair_state),
                       tickets + 2, s.point_list, s.bounded);
    GSR_LAUNCH_CHECK();
    return 0;
}

// K5-K7 as ONE persistent launch (binning_persist.h) when the device can hold the grid and no barrier kernel of another
// stream may still be waiting.  -> 0 launched, 1 not now (the two look-back passes), otherwise an error
int launch_persist_sort(const SortCall &s, const BinHooks &h, BinDevice &d) {
    const BinFrame &f = s.f;
    if (!(persist_effective_mode() & PERSIST_S)) return 1;
    persist_caps(d);
    const int grid_s = lowered(h.grid_s, d.grid_s);
    const long long nbD = radix_blocks(s.D);
    const int G = (int)(nbD < grid_s ? nbD : grid_s);
    // long sorts are throughput-bound (VALU: the ranking) and the look-back pipeline, which reads every pair once
    // less, wins: measured cross-over between 2 and 14 million pairs (profiles/r05_binning_persistent.txt)
    if (!(G > 0 && d.done && s.D <= h.persist_maxd && !persist_sort_backoff(d, h.abort_s))) return 1;
    const long long admit = persist_admit(d, s.stream);
    if (admit < 0) return 1;
    const SortViews v = views(sort_layout(f, s.D), s.scratch);
    const PersistLayoutS PS = persist_layout_s(G);
    SortPersistArgs a{};
    a.P = s.P; a.gx = f.gx; a.xbits = f.xbits; a.ybits = f.ybits;
    a.D = s.D; a.bounded = s.bounded ? 1 : 0;
    a.rects = s.pv.rects; a.sorted_ids = s.pv.vA; a.offsets = s.pv.offsets; a.mask = s.mask;
    a.kA = v.kA; a.kB = v.kB; a.vB = v.vB; a.point_list = s.point_list;
    a.ranges = s.ranges; a.ranges_words = 2 * f.gx * f.gy;
    a.hull = s.pv.hull;
    a.sync = sync_view(v.ctrl + PS.sync, G);
    a.tstamp = timeline_buffer(h.timeline, 1, G);
    a.grp = at<uint32_t>(v.ctrl, PS.grp); a.cnt = at<uint32_t>(v.ctrl, PS.cnt);
    a.grp_solo = at<uint32_t>(v.ctrl, PS.grp_solo); a.cnt_solo = at<uint32_t>(v.ctrl, PS.cnt_solo);
    a.done_word = d.done; a.done_seq = (uint32_t)admit;
    // a quarter of a second at the first barrier, then workgroup 0 sorts the view alone (no trap, no host round
    // trip: binning_persist.h); GSR_BIN_SORT_TIMEOUT_MS overrides (tests)
    a.timeout_ticks = 100000ull * (unsigned long long)h.sort_timeout_ms;
    a.owners_cap = h.owners;
    a.force_abort = h.abort_s ? 1 : 0;
    hipLaunchKernelGGL(bin_sort_persist_kernel, dim3(G), dim3(PS_THREADS), 0, s.stream, a);
    GSR_LAUNCH_CHECK();
    return 0;
}

// (row, column) keys in two look-back passes: pass 0 (column digit) fused with the emission, pairs land in (kB, vB);
// pass 1 (row digit) -> (kA, point_list); K7
int launch_lookback_yx(const SortCall &s) {
    const BinFrame &f = s.f;
    const SortViews v = views(sort_layout(f, s.D), s.scratch);
    const long long D = s.D;
    const uint32_t *thist = s.pv.thist, *offsets = s.pv.offsets;
    const int nb = (int)radix_blocks(D);
    const uint32_t *D_dev = s.bounded ? offsets + s.P : nullptr;
    hipLaunchKernelGGL((emit_scatter_kernel<RADIX_TILE / 512, 512>), dim3(nb), dim3(512), 0, s.stream, s.P, D, f.xbits,
                       s.pv.rects, s.pv.vA, offsets, thist, v.state, v.tickets + 1, v.kB, v.vB, s.bounded, s.ranges,
                       2 * f.gx * f.gy, s.pv.hull);
    hipLaunchKernelGGL((radix_onesweep_kernel<RADIX_TILE / 512, 512>), dim3(nb), dim3(512), 0, s.stream, v.kB, v.vB, v.kA,
                       s.point_list, D, f.xbits, f.ybits, thist + RADIX_DIGITS, v.state + (size_t)nb * RADIX_DIGITS,
                       v.tickets + 2, D_dev);
    hipLaunchKernelGGL(tile_ranges_yx_kernel, dim3(gsr_div_up(gsr_div_up(D, 4), GSR_ONE_DIM_BLOCK)),
                       dim3(GSR_ONE_DIM_BLOCK), 0, s.stream, D, f.gx, f.xbits, v.kA, s.mask,
                       reinterpret_cast<int2 *>(s.ranges), D_dev);
    GSR_LAUNCH_CHECK();
    return 0;
}

// tile-id keys (frames above 256 x 256 tiles): K5, ceil(log2(tiles) / 8) look-back passes, K7
int launch_generic(const SortCall &s) {
    const BinFrame &f = s.f;
    const SortLayout S = sort_layout(f, s.D);
    const SortViews v = views(S, s.scratch);
    const RadixPlan radix = radix_plan(0, tile_bits(f.tiles));
    const long long D = s.D;
    hipLaunchKernelGGL(emit_pairs_kernel, dim3(gsr_div_up(gsr_div_up(D, EMIT_CHUNK), 4)), dim3(256), 0, s.stream, s.P, D,
                       f.gx, f.gx * f.gy, s.pv.rects, s.mask, s.pv.vA, s.pv.offsets, radix, v.kA, v.vA, v.ghist);
    int in_first = 1;
    // the last pass writes the Gaussian indices straight into point_list
    const int rc = radix_sort_pairs(v.kA, v.vA, v.kB, v.vB, D, radix, v.ctrl, S.C, &in_first, s.stream, s.point_list);
    if (rc) return rc;
    hipLaunchKernelGGL(tile_ranges_kernel, dim3(gsr_div_up(gsr_div_up(D, 4), GSR_ONE_DIM_BLOCK)),
                       dim3(GSR_ONE_DIM_BLOCK), 0, s.stream, D, (uint32_t)(f.gx * f.gy), in_first ? v.kA : v.kB,
                       reinterpret_cast<int2 *>(s.ranges));
    GSR_HIP(hipMemcpyAsync(s.ranges + 2 * (size_t)f.gx * f.gy, s.pv.hull, 2 * sizeof(int32_t), hipMemcpyDeviceToDevice,
                           s.stream));
    GSR_LAUNCH_CHECK();
    return 0;
}

// the plan's form; its zero region has been cleared, or is being cleared by the prepare step in front of it
int sort_run(const SortCall &s, const BinHooks &h, BinDevice &d, SortForm form) {
    if (form == SORT_ROWS) return launch_rows(s, h, d);
    if (form == SORT_GENERIC) return launch_generic(s);
    const int rc = launch_persist_sort(s, h, d);
    return rc == 1 ? launch_lookback_yx(s) : rc;
}

int bin_sort_impl(int P, int width, int height, const uint8_t *compute_locally, const void *prep, int64_t D,
                  void *scratch, size_t scratch_bytes, uint32_t *point_list, int32_t *ranges, hipStream_t stream,
                  bool bounded) {
    if (P < 0 || width <= 0 || height <= 0 || D < 0 || !ranges) return GSR_EINVAL;
    const BinFrame f = bin_frame(width, height);
    if (D == 0 || P == 0 || !f.yx)  // (the (row, column) forms clear the table inside their first kernel)
        GSR_HIP(hipMemsetAsync(ranges, 0, sizeof(int32_t) * 2 * ((size_t)f.gx * f.gy + 1), stream));  // + the hull row: (0, 0)
    if (D == 0 && P > 0 && prep)  // a view without pairs still has its band: K3 left the hull, as the bounded sort copies it
        GSR_HIP(hipMemcpyAsync(ranges + 2 * (size_t)f.gx * f.gy, views(prep_layout(P), const_cast<void *>(prep)).hull,
                               2 * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    if (D == 0 || P == 0) return 0;
    if (!compute_locally || !prep || !scratch || !point_list) return GSR_EINVAL;
    const BinHooks h = read_hooks();
    const SortPlan p = plan_sort(f, D, scratch_bytes, bounded, h.rows_min);
    if (p.err) return p.err;
    BinDevice *d = nullptr;
    int rc = bin_device(&d);
    if (!rc) rc = persist_fault_check(*d);
    if (rc) return rc;
    GSR_HIP(hipMemsetAsync(reinterpret_cast<char *>(scratch) + p.zero_off, 0, p.zero_bytes, stream));
    return sort_run({f, P, compute_locally, views(prep_layout(P), const_cast<void *>(prep)), D, scratch, point_list, ranges,
                     stream, bounded}, h, *d, p.form);
}
}  // namespace

// ----------------------------------------------------------------------------------- K3..K7 API
extern "C" size_t gsr_bin_prepare_bytes(int P, int width, int height) {
    if (P < 0 || width <= 0 || height <= 0) return 0;
    return prep_bytes_needed(P);
}

extern "C" size_t gsr_bin_total_offset(int P, int width, int height) {
    if (P < 0 || width <= 0 || height <= 0) return 0;
    return prep_layout(P).offsets + sizeof(uint32_t) * (size_t)P;  // offsets[P]: K4's total
}

extern "C" size_t gsr_bin_segments_offset(int P, int width, int height) {
    if (P < 0 || width <= 0 || height <= 0) return 0;
    return prep_layout(P).segoff + sizeof(uint32_t) * (size_t)P;  // segoff[P]: the row segments R
}

extern "C" size_t gsr_bin_sort_bytes(int P, int64_t num_rendered, int width, int height) {
    (void)P;
    if (num_rendered < 0 || width <= 0 || height <= 0) return 0;
    return sort_layout(bin_frame(width, height), num_rendered).total;
}

extern "C" int64_t gsr_bin_sort_capacity(int P, size_t scratch_bytes, int width, int height) {
    (void)P;
    if (width <= 0 || height <= 0) return 0;
    const BinFrame f = bin_frame(width, height);
    if (!f.yx) return 0;  // bounded launches exist for the (row, column) path only
    int64_t lo = 0, hi = RADIX_MAX_N;  // largest D whose layout fits scratch_bytes
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (sort_layout(f, mid).total <= scratch_bytes) lo = mid; else hi = mid - 1;
    }
    return lo;
}

extern "C" int gsr_bin_count_wait(uint32_t ticket, int64_t *num_rendered_host, gsr_stream_t stream_) {
    if (!num_rendered_host) return GSR_EINVAL;
    *num_rendered_host = 0;
    if (ticket == 0) return 0;
    BinDevice *d = nullptr;
    int rc = bin_device(&d);
    if (rc) return rc;
    if (!d->total_word) return GSR_EINVAL;  // (no ticket was ever taken on this device)
    uint32_t total = 0;
    rc = wait_total(reinterpret_cast<hipStream_t>(stream_), slot_of_ticket(*d, ticket), ticket, &total);
    if (rc) return rc;
    if (total == PAIRS_ABORTED) {
        // the persistent kernel gave up at its first barrier (the device is shared with another barrier kernel): the
        // same call again on the look-back pipeline.  A gsr_bin_sort_bounded launched meanwhile has written nothing
        // (it saw a count above any capacity): GSR_ERETRY tells the caller to sort again
        PrepCall c = d->calls[ticket % TOTAL_SLOTS];
        if (!c.persistent) return GSR_EINVAL;
        c.persistent = false;
        uint32_t again = 0;
        rc = prepare_lookback(c, bin_frame(c.width, c.height), *d, &again);
        if (rc) return rc;
        rc = wait_total(c.stream, slot_of_ticket(*d, again), again, &total);
        if (rc) return rc;
        *num_rendered_host = (int64_t)total;
        return GSR_ERETRY;
    }
    *num_rendered_host = (int64_t)total;
    return 0;
}

extern "C" int gsr_bin_prepare(int P, int width, int height, const float *means2D, const float *depths,
                               const int32_t *radii, const float *conic_opacity, const uint8_t *compute_locally,
                               void *prep, size_t prep_bytes, int64_t *num_rendered_host, gsr_stream_t stream_) {
    if (!num_rendered_host) return GSR_EINVAL;
    *num_rendered_host = 0;
    uint32_t ticket = 0;
    const int rc = gsr_bin_prepare_async(P, width, height, means2D, depths, radii, conic_opacity, compute_locally, prep,
                                         prep_bytes, &ticket, stream_);
    if (rc) return rc;
    const int rw = gsr_bin_count_wait(ticket, num_rendered_host, stream_);
    return rw == GSR_ERETRY ? 0 : rw;  // (no sort has been launched for this count yet)
}

extern "C" int gsr_bin_sort(int P, int width, int height, const uint8_t *compute_locally, const void *prep,
                            int64_t D, void *scratch, size_t scratch_bytes, uint32_t *point_list, int32_t *ranges,
                            gsr_stream_t stream_) {
    return bin_sort_impl(P, width, height, compute_locally, prep, D, scratch, scratch_bytes, point_list, ranges,
                         reinterpret_cast<hipStream_t>(stream_), false);
}

extern "C" int gsr_bin_sort_bounded(int P, int width, int height, const uint8_t *compute_locally, const void *prep,
                                    int64_t capacity, void *scratch, size_t scratch_bytes, uint32_t *point_list,
                                    int32_t *ranges, gsr_stream_t stream_) {
    if (capacity <= 0) return GSR_EINVAL;
    return bin_sort_impl(P, width, height, compute_locally, prep, capacity, scratch, scratch_bytes, point_list, ranges,
                         reinterpret_cast<hipStream_t>(stream_), true);
}

// K3-K7 of one view in ONE call for callers that keep a grow-only scratch (the operator's path): gsr_bin_prepare_async,
// then -- when `capacity` > 0 -- gsr_bin_sort_bounded into (scratch, point_list).  Nothing waits: *ticket names the
// pair count for gsr_bin_count_wait, which the caller may call after it has launched the kernels that consume the
// lists (they read the ranges, never the count) -- round 6: the host no longer stands between K3-K7 and K8.
// *sorted = 1 when the bounded sort was launched.  The sort is planned BEFORE the prepare step is launched: that step's
// first kernel clears the plan's zero region (no fill launch between the steps), and the same plan runs behind it.
extern "C" int gsr_bin_speculative_async(int P, int width, int height, const float *means2D, const float *depths,
                                         const int32_t *radii, const float *conic_opacity,
                                         const uint8_t *compute_locally, void *prep, size_t prep_bytes,
                                         int64_t capacity, void *scratch, size_t scratch_bytes, uint32_t *point_list,
                                         int32_t *ranges, uint32_t *ticket, int *sorted, gsr_stream_t stream_) {
    if (!ticket || !sorted) return GSR_EINVAL;
    *sorted = 0;
    if (P < 0 || width <= 0 || height <= 0) return GSR_EINVAL;
    *ticket = 0;  // 0: nothing was launched, the count is 0
    if (P == 0) return 0;
    if (!means2D || !depths || !radii || !conic_opacity || !compute_locally || !prep) return GSR_EINVAL;
    if (P > RADIX_MAX_N) return GSR_EINVAL;
    if (prep_bytes < prep_bytes_needed(P)) return GSR_ENOSPACE;
    const BinFrame f = bin_frame(width, height);
    if (f.gx > 0xFFFF || f.gy > 0xFFFF) return GSR_EINVAL;
    BinDevice *d = nullptr;
    int rc = bin_device(&d);
    if (!rc) rc = persist_fault_check(*d);
    if (rc) return rc;
    const BinHooks h = read_hooks();
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const bool sort = capacity > 0 && scratch && point_list;
    const SortPlan p = sort ? plan_sort(f, capacity, scratch_bytes, true, h.rows_min) : SortPlan{GSR_EINVAL};
    PrepCall c{P, width, height, means2D, depths, radii, conic_opacity, compute_locally, prep, stream, true, nullptr, 0};
    if (!p.err) {
        c.zero_ptr = reinterpret_cast<char *>(scratch) + p.zero_off;
        c.zero_bytes = p.zero_bytes;
    }
    rc = prepare_persistent(c, f, h, *d, ticket);
    if (rc == 1) {  // (not applicable here: the look-back pipeline)
        c.persistent = false;
        rc = prepare_lookback(c, f, *d, ticket);
    }
    if (rc) return rc;
    d->calls[*ticket % TOTAL_SLOTS] = c;
    d->calls[*ticket % TOTAL_SLOTS].zero_ptr = nullptr;  // (a repeat through gsr_bin_count_wait must not clear the
    d->calls[*ticket % TOTAL_SLOTS].zero_bytes = 0;      // control block of a sort in flight)
    if (!sort) return 0;
    if (!ranges) return GSR_EINVAL;
    if (!f.yx) GSR_HIP(hipMemsetAsync(ranges, 0, sizeof(int32_t) * 2 * ((size_t)f.gx * f.gy + 1), stream));
    if (p.err) return p.err;
    rc = sort_run({f, P, compute_locally, views(prep_layout(P), prep), capacity, scratch, point_list, ranges, stream, true},
                  h, *d, p.form);
    if (rc) return rc;
    *sorted = 1;
    return 0;
}

extern "C" int gsr_bin_prepare_async(int P, int width, int height, const float *means2D, const float *depths,
                                     const int32_t *radii, const float *conic_opacity, const uint8_t *compute_locally,
                                     void *prep, size_t prep_bytes, uint32_t *ticket, gsr_stream_t stream_) {
    int sorted = 0;
    return gsr_bin_speculative_async(P, width, height, means2D, depths, radii, conic_opacity, compute_locally, prep,
                                     prep_bytes, 0, nullptr, 0, nullptr, nullptr, ticket, &sorted, stream_);
}

extern "C" int gsr_set_depth_tie_order(int mode) {
    if (mode != 0 && mode != 1) return GSR_EINVAL;
    g_tie_order.store(mode, std::memory_order_relaxed);
    return 0;
}

extern "C" int gsr_set_tile_cull(int mode) {
    if (mode < -1 || mode > 2) return GSR_EINVAL;
    g_tile_cull.store(mode, std::memory_order_relaxed);
    return 0;
}

extern "C" int gsr_set_bin_rowmajor(int mode) {
    if (mode < -1 || mode > 1) return GSR_EINVAL;
    g_rows_override.store(mode, std::memory_order_relaxed);
    return 0;
}

extern "C" int gsr_set_bin_persistent(int mode) {
    if (mode < -1 || mode > 3) return GSR_EINVAL;
    g_persist_override.store(mode, std::memory_order_relaxed);
    // an explicit choice also ends the back-off that follows a one-workgroup recovery of the sort kernel
    std::lock_guard<std::mutex> guard(g_bin_mutex);
    for (BinDevice &d : g_bin_devices) {
        if (!d.done) continue;
        d.solo_seen = reinterpret_cast<volatile uint32_t *>(d.done)[3];
        d.backoff = 0;
    }
    return 0;
}

extern "C" int gsr_bin_persist_status(uint32_t *out4) {
    if (!out4) return GSR_EINVAL;
    BinDevice *d = nullptr;
    const int rc = bin_device(&d);
    if (rc && rc != GSR_EINVAL) return rc;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (rc || !d->done) return 0;  // (a device beyond the table has no persistent launches)
    const volatile uint32_t *w = d->done;
    out4[0] = w[0]; out4[1] = w[1]; out4[2] = w[2]; out4[3] = w[3];
    return 0;
}

extern "C" int gsr_bin_timeline(int which, unsigned long long *out, int max_words, int *grid) {
    if (which < 0 || which > 1 || !out || !grid || max_words < 0) return GSR_EINVAL;
    *grid = g_timeline_grid[which];
    if (!g_timeline[which]) return 0;
    const size_t n = (size_t)g_timeline_grid[which] * 32;
    GSR_HIP(hipDeviceSynchronize());
    GSR_HIP(hipMemcpy(out, g_timeline[which], sizeof(unsigned long long) * (n < (size_t)max_words ? n : (size_t)max_words),
                      hipMemcpyDeviceToHost));
    return 0;
}

#ifdef GSR_ROWS_TS
extern "C" int gsr_debug_rows_ts(unsigned long long *out, int words) {
    GSR_HIP(hipDeviceSynchronize());
    GSR_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rows_ts), sizeof(unsigned long long) * (size_t)words));
    return 0;
}
extern "C" int gsr_debug_rows_ts2(unsigned long long *out, int words) {
    GSR_HIP(hipDeviceSynchronize());
    GSR_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rows_ts2), sizeof(unsigned long long) * (size_t)words));
    return 0;
}
#endif
