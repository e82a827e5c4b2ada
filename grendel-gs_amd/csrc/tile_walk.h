// tile_walk.h -- what the SIDE PASSES over the tile lists share (gfx950 / wave64): contrib.hip, invdepth.hip, features.hip
// and absgrad.hip.  A new side pass starts here; K8 / K10 (composite.hip) keep their own tuned walks.
//
// K8 decides what every pixel blends; a side pass walks the same lists once more and blends, or differentiates,
// something else.  Nothing is re-decided: a pixel's walk ends where K8's ended (n_contrib), and the (pixel, entry) pairs
// taken are K10's `take` rule -- position + 1 <= n_contrib, power <= 0, alpha >= 1/255 -- in the arithmetic of
// composite_math.h, which K8 and K10 compile too.
//
// Shape of the work: K8's.  One workgroup = one tile (side_pass_tile_of_block), one wave = one 8x8 quadrant, lane =
// pixel.  The list is walked in 64-entry chunks, front to back from T = 1 or back to front from final_T: one entry per
// lane (index read + gather + quadrant test), the relevant entries compacted in WALK order (rank = the relevant lanes
// below, or above) into records in a wave-private LDS slab, {x, y, a2, b2 | c2, o, position + 1, . | the pass's own
// quads}, and read back with wave-uniform addresses, CB slots at a time.  The walk of a wave ends at the largest
// n_contrib of its quadrant (K10's bound): entries behind every pixel's stop are never loaded.  The <= CB - 1 slots
// behind a chunk's last relevant entry are INERT records, every word written: their position word NO_POS fails
// `position + 1 <= n_contrib` on every pixel, and an opacity that is divided by is 1.  The four quadrant waves of a
// tile never synchronise: a wave barrier follows the staging (the wave's own LDS stores precede its loads) and the batch
// loop (the next chunk overwrites the slab only after these reads).
//
// The backward passes reduce over the quadrant's 64 pixels by an LDS TRANSPOSE over a batch of CB entries: phase A (lane
// = pixel) stores its per-pixel terms of every entry of the batch into a wave-private matrix [slot][pixel] (row stride
// MSTR for two words per pixel); phase B (lane = (slot, row of the quadrant)) reads its row's eight pixels in pixel order
// and three xor steps combine the rows: a fixed order, fp32.
//
// Who calls what (EXPERIMENTS.md, 2026-11-26, "side passes: one header", has the figures): stage_chunk all six walks;
// quadrant_begin the contribution kernel and the inverse-depth forward (in the other four it grows VGPRs or measured
// slower, and they spell the prologue out); pair_decision all but composite_invdepth_backward_kernel and
// composite_absgrad_kernel (measured slower).  Phase B is each backward's own: as a helper it grows the VGPRs of the
// features backward.  A fix to the prologue still has to visit those four kernels and this header.
#pragma once
#include "common.h"
#include "composite_math.h"

namespace {

constexpr int CB = 8;               // entries per batch (forward: per unrolled group of the walk)
constexpr int MSTR = 66;            // row stride of a two-word phase A matrix in 8-byte elements (16-byte aligned rows)
constexpr int NO_POS = 0x7fffffff;  // position word of an inert slot: no n_contrib reaches it

// block -> tile as in K8: the band's tiles only when the caller named the band (band_first < 0: `band_tiles` is a
// capacity, the band is the row hull behind the range table), else XCD-contiguous spans of the hull's tiles first.
// -1: this workgroup has no tile
__device__ __forceinline__ int side_pass_tile_of_block(const int2 *__restrict__ ranges, int gx, int tiles, int band,
                                                       int band_first, int band_tiles) {
    if (band) {
        if (band_first < 0) {
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

// a wave's quadrant of its tile and this lane's pixel of it
struct Quadrant {
    int lane, wave;
    int qx0, qy0;  // origin of the quadrant
    int px, py;    // this lane's pixel
    bool inside;   // ... is a pixel of the image
    size_t pid;    // py * W + px
    int2 range;    // the tile's list in point_list
    int last;      // where K8 stopped on this pixel
    int wlen;      // the largest `last` of the quadrant: the length of the wave's walk
    float pxf, pyf;
};

// false: the wave has nothing to walk (no tile, not our tile, or no pixel of the quadrant blended anything).  No workgroup
// barrier may follow: waves leave on their own.
__device__ __forceinline__ bool quadrant_begin(Quadrant &q, int W, int H, int gx, int tiles, const int2 *ranges,
                                               const uint8_t *compute_locally, const int32_t *n_contrib, int band,
                                               int band_first, int band_tiles) {
    const int tile = side_pass_tile_of_block(ranges, gx, tiles, band, band_first, band_tiles);
    if (tile < 0 || !compute_locally[tile]) return false;
    q.lane = threadIdx.x & 63, q.wave = threadIdx.x >> 6;
    const int tx = tile % gx, ty = tile / gx;
    q.qx0 = tx * GSR_BLOCK_X + (q.wave & 1) * 8, q.qy0 = ty * GSR_BLOCK_Y + (q.wave >> 1) * 8;
    q.px = q.qx0 + (q.lane & 7), q.py = q.qy0 + (q.lane >> 3);
    q.inside = q.px < W && q.py < H;
    q.pid = (size_t)q.py * W + q.px;
    const int2 range = ranges[tile];
    q.range.x = range.x, q.range.y = range.y;
    const int n = range.y - range.x;
    q.pxf = (float)q.px, q.pyf = (float)q.py;
    // where K8 stopped on this pixel; never beyond the list, whatever the caller's array holds
    q.last = q.inside ? min(n_contrib[q.pid], n) : 0;
    q.wlen = q.last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) q.wlen = max(q.wlen, __shfl_xor(q.wlen, d, 64));
    return q.wlen > 0;
}

enum WalkDir { FRONT_TO_BACK, BACK_TO_FRONT };

// Stage the chunk [c, c + 64) of the wave's list (`first` = its start in point_list, `wlen` = the length of the walk):
// one entry per lane, the relevant ones compacted in walk order into slots of REC float4,
// {x, y, a2, b2 | c2, o, position + 1, word(id) | the kernel's own quads}.  `extra(slot, id)` writes the kernel's own
// quads and id word of a relevant entry behind the two geometry quads, `inert(slot)` writes them for an inert slot.  The
// walk takes CB slots at a time, so the <= CB - 1 slots behind the last entry are made inert, EVERY word written: nothing
// stale is ever read.  Returns the number of relevant entries; the caller places the wave barriers.
template <WalkDir DIR, int REC, class Word, class Extra, class Inert>
__device__ __forceinline__ int stage_chunk(int c, int lane, int wlen, int first, int qx0, int qy0,
                                           const uint32_t *point_list, const float2 *means2D,
                                           const float4 *conic_opacity, float4 *wslab, Word &&word, Extra &&extra,
                                           Inert &&inert) {
    const bool have = c + lane < wlen;
    const uint32_t id = have ? point_list[first + c + lane] : 0u;
    const Entry e = load_entry(have, id, means2D, conic_opacity, (float)qx0, (float)qy0);
    const unsigned long long m = __ballot(e.relevant);
    const int nrel = __popcll(m);
    if (e.relevant) {  // rank in WALK order: the relevant lanes below (front to back) or above (back to front)
        const int pos = DIR == BACK_TO_FRONT ? __popcll((m >> lane) >> 1) : __popcll(m & ((1ull << lane) - 1ull));
        wslab[REC * pos] = make_float4(e.x, e.y, e.a2, e.b2);
        wslab[REC * pos + 1] = make_float4(e.c2, e.o, __int_as_float(c + lane + 1), word(id));
        extra(pos, id);
    }
    const int pad = (-nrel) & (CB - 1);
    if (lane < pad) {
        wslab[REC * (nrel + lane)] = make_float4(0.f, 0.f, 0.f, 0.f);
        wslab[REC * (nrel + lane) + 1] = make_float4(0.f, 0.f, __int_as_float(NO_POS), 0.f);
        inert(nrel + lane);
    }
    return nrel;
}

// The decision on one (pixel, entry) pair of a staged record (q0, q1): K10's `take` rule, the one spelling of it among
// the side passes.  `raw` is o exp(power), `alpha` its min(0.99, .); neither means anything where `take` is false (an
// inert slot's alpha is not used: select on `take`, never multiply by it).
struct Pair {
    float raw, alpha;
    bool take;
};
__device__ __forceinline__ Pair pair_decision(const float4 q0, const float4 q1, float pxf, float pyf, int last) {
    const float pe = entry_exponent(q0, q1, q0.x - pxf, q0.y - pyf);
    const float raw = entry_alpha_raw(q1, pe);
    const float alpha = fminf(0.99f, raw);
    const bool take = __float_as_int(q1.z) <= last && entry_power_ok(q1, pe) && alpha >= ALPHA_MIN;
    return {raw, alpha, take};
}

}  // namespace
