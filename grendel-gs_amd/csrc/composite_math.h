// composite_math.h -- what every walk over the tile lists has to agree on: the alpha arithmetic of K8 / K10
// (composite.hip) and of the contribution kernel (contrib.hip), the block -> tile map, and the launch geometry of a row
// band.  One copy, so that the kernels can only ever take the SAME skip / blend decisions on a (pixel, entry) pair.
#pragma once
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float ALPHA_MIN = 1.0f / 255.0f;
constexpr float T_STOP = 0.0001f;

// lane-resident entry of the tile list
struct Entry {
    float x, y;        // pixel centre
    float a2, b2, c2;  // conic pre-scaled to log2 units: p2 = a2 dx^2 + b2 dx dy + c2 dy^2 = power * log2(e)
    float o;           // opacity, or log2(opacity) with GSR_LOG2O (see entry_exponent)
    bool relevant;
};

// alpha = min(0.99, o exp(power)) of a broadcast entry (q0 = x, y, a2, b2; q1 = c2, o, r, g) at offset (dx, dy).
// GSR_LOG2O (default): the opacity is folded into the exponent, o exp2(p2) = exp2(p2 + log2 o), one multiply less
// per (pixel, entry); K8 and K10 share these helpers, so the forward and the backward always take the SAME
// skip / blend decisions.  `power > 0 -> skip` becomes  exponent > log2 o.
#ifndef GSR_NO_LOG2O
#define GSR_LOG2O 1
#endif
__device__ __forceinline__ float entry_exponent(const float4 q0, const float4 q1, float dx, float dy) {
#ifdef GSR_LOG2O
    return fmaf(fmaf(q0.z, dx, q0.w * dy), dx, fmaf(q1.x * dy, dy, q1.y));
#else
    return (q0.z * dx + q0.w * dy) * dx + q1.x * dy * dy;
#endif
}
__device__ __forceinline__ float entry_alpha_raw(const float4 q1, float pe) {
#ifdef GSR_LOG2O
    return __builtin_amdgcn_exp2f(pe);
#else
    return q1.y * __builtin_amdgcn_exp2f(pe);
#endif
}
__device__ __forceinline__ bool entry_power_ok(const float4 q1, float pe) {
#ifdef GSR_LOG2O
    return pe <= q1.y;
#else
    return pe <= 0.f;
#endif
}

__device__ __forceinline__ float entry_opacity_term(float o) {
#ifdef GSR_LOG2O
    return __log2f(o);
#else
    return o;
#endif
}

// Load entry `idx` (or an inert one) and test it against the quadrant [qx0,qx0+7]x[qy0,qy0+7].
__device__ __forceinline__ Entry load_entry(bool have, uint32_t id, const float2 *__restrict__ means2D,
                                            const float4 *__restrict__ conic_opacity, float qx0, float qy0) {
    Entry e;
    e.x = e.y = e.a2 = e.b2 = e.c2 = e.o = 0.f;
    e.relevant = false;
    if (have) {
        const float2 xy = means2D[id];
        const float4 co = conic_opacity[id];
        e.x = xy.x;
        e.y = xy.y;
        e.a2 = -0.5f * LOG2E * co.x;
        e.b2 = -LOG2E * co.y;
        e.c2 = -0.5f * LOG2E * co.z;
        e.o = entry_opacity_term(co.w);
        e.relevant = gsr_can_touch_box(xy, co, qx0, qy0, qx0 + 7.0f, qy0 + 7.0f);
    }
    return e;
}

// block -> tile: XCD-contiguous spans of the BAND this rank renders.  The binning leaves the band (the row hull of the
// mask, [lo, hi) tile rows) in row `tiles` of the range table (include/gsraster.h: gsr_bin_sort); anything implausible
// there falls back to spans of the whole grid.
__device__ __forceinline__ int composite_tile_of_block(const int2 *__restrict__ ranges, int gx, int tiles) {
    const int2 hull = ranges[tiles];
    const int gy = tiles / gx;
    if (hull.x < 0 || hull.y > gy || hull.x >= hull.y) return gsr_xcd_span_of_block(blockIdx.x, tiles);
    return gsr_xcd_span_of_block_band(blockIdx.x, tiles, hull.x * gx, (hull.y - hull.x) * gx);
}

// The launch geometry of a row band [row_lo, row_hi) of tile rows (include/gsraster.h: 0, 0 = the whole grid; row_lo == -1:
// `row_hi` tile rows are a CAPACITY, the band is read from the device, see composite_forward_kernel).
struct BandGrid {
    bool band;       // the grid covers band_tiles tiles instead of all of them
    int band_first;  // first tile of the band, -1: device band
    int band_tiles;
};
inline BandGrid band_grid_of(int row_lo, int row_hi, int gx, int gy) {
    const bool dyn = row_lo == -1 && row_hi > 0 && row_hi <= gy;
    const bool band = dyn || (row_lo >= 0 && row_lo < row_hi && row_hi <= gy && !(row_lo == 0 && row_hi == gy));
    return {band, dyn ? -1 : band ? row_lo * gx : 0, dyn ? row_hi * gx : band ? (row_hi - row_lo) * gx : 0};
}

}  // namespace
