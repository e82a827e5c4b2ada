// tsdf.hip -- mesh extraction for gfx950 (include/gsraster.h: gsr_tsdf_*): fusion of depth maps into a truncated signed
// distance volume, and marching tetrahedra on it.  The reference has no mesh extraction, so there is NO reference call
// site: plain float64 numpy on the host is the arbiter (tests/tsdf_refs.py, tests/test_gpu_tsdf.py).  DESIGN.md 3.21.
//
// VOLUME -- a regular grid of X x Y x Z voxels (multiples of 8), voxel (i, j, k) centred at origin + voxel_size (i, j, k),
// stored BRICK-MAJOR: a plane is [Z/8][Y/8][X/8][8][8][8] floats, one 8^3 brick = 2 KiB contiguous.  One workgroup of
// 256 lanes owns one brick, lane t the voxels t and t + 256 of it (coalesced 1 KiB rows).
//
// INTEGRATION (tsdf_integrate_kernel), one launch per batch of up to 16 views.  Per voxel and per view, in view order:
//   (x, y, z) = [p, 1] viewmatrix;  z <= near skips;  px = ((x / (z tanfovx) + 1) W - 1) / 2, py alike;  the nearest
//   pixel (rint), outside the image skips;  d there, d <= 0 or d > depth_trunc skips;  sdf = d - z outside
//   [-trunc, trunc] skips;  tsdf = (tsdf w + (sdf / trunc) wv) / (w + wv), rgb alike, w += wv.
// A voxel's state stays in registers across the batch and is stored once, and only if a view updated it: every plane is
// read and written at most once per launch, there are no atomics, and the result does not depend on how the views are
// split into batches (the same operations in the same order).  The batch's camera records (12 words of the view matrix
// and the view's weight) are staged in LDS and read at wave-uniform addresses.
//   * brick culling: tsdf_tiles_kernel reduces every depth map to (min, max) of its valid depths per 16 x 16 tile; lane v
//     of the first wave projects the 8 corners of the brick grown by half a voxel into view v -> [zmin, zmax] and a pixel
//     box (grown by a pixel).  The view is dropped for the brick when zmax <= near, when the box misses the image, or
//     when over the tiles the box overlaps zmin > dmax + trunc or zmax < dmin - trunc: z is affine, so every voxel's z
//     lies in [zmin, zmax] with half a voxel to spare, its pixel in the box, its d in [dmin, dmax] if valid -- the
//     per-voxel rule would skip each of them.  A brick with a corner at or behind the near plane, or a box of more than
//     TS_CULL_MAX_TILES tiles, is kept.  A workgroup whose view mask is empty returns before it loads a voxel.
//
// EXTRACTION -- marching tetrahedra on the Kuhn split (six tetrahedra 0 -> e_a -> e_a + e_b -> (1,1,1) per cell, one per
// axis permutation: face diagonals agree between neighbouring cells by construction).  A cell is processed iff its 8
// corners are valid (weight > 0 and >= min_weight); a corner is inside iff tsdf < 0.  Every voxel owns the 7 edges
// towards +x +y +z +xy +yz +xz +xyz; an owned edge carries a vertex iff its ends differ in sign and a processed cell
// uses it (the cells whose base is the voxel, or one less along an axis the edge does not move in).
//   tsdf_count_kernel   a workgroup per brick stages tsdf and weight with a one-voxel halo (10^3 x 2 floats) and the 9^3
//                       cell flags in LDS; per voxel the 7-bit edge mask and the triangle count, scanned over the brick
//                       in voxel order -> record = mask | vertex offset in the brick << 7 | triangle offset << 19, and
//                       the brick's totals;
//   tsdf_scan_kernel    ONE workgroup scans the brick totals (1024 per trip, a carry in registers): no look-back, no wait;
//   tsdf_emit_kernel    stages again, writes the voxel's vertices, then the triangles of its cell: the index of a
//                       vertex is its owner's brick base + offset + popcount(mask below the edge's bit), the owner's
//                       record read from the count pass's output (it may lie in a neighbouring brick).
// The output order is a pure function of the voxel order: the same volume gives the same bits on every run.
#include "common.h"

#pragma clang fp contract(off)  // one rounding per operation: the rule is restated in float32 on the host

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_BRICK = 512;          // voxels per brick
constexpr int TS_MAX_VIEWS = 16;
constexpr int TS_TILE = 16;            // pixels per side of a depth tile
constexpr int TS_CAM_WORDS = 13;       // v[3 r + c] = viewmatrix[r][c], c < 3; word 12: the view's weight
constexpr int TS_CULL_MAX_TILES = 64;  // a larger pixel box is not tested against the depth tiles
constexpr int TS_HALO = 10, TS_HALO3 = 1000, TS_CELLS = 9, TS_CELLS3 = 729;
constexpr int TS_SCAN_THREADS = 1024;

struct TsdfGrid {
    float ox, oy, oz, vs;
    int bx, by, bz;  // bricks per axis
};

__device__ __forceinline__ float ts_wave_min(float v) {
#pragma unroll
    for (int o = GSR_WAVE / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, GSR_WAVE));
    return v;
}
__device__ __forceinline__ float ts_wave_max(float v) {
#pragma unroll
    for (int o = GSR_WAVE / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, GSR_WAVE));
    return v;
}

// (min, max) of the valid depths of every 16 x 16 tile: (+inf, -inf) for a tile without one
__global__ void __launch_bounds__(TS_THREADS)
tsdf_tiles_kernel(int W, int H, const float *__restrict__ depths, float depth_trunc, float2 *__restrict__ tiles) {
    __shared__ float smin[TS_THREADS / GSR_WAVE], smax[TS_THREADS / GSR_WAVE];
    const int x = blockIdx.x * TS_TILE + (threadIdx.x & 15), y = blockIdx.y * TS_TILE + (threadIdx.x >> 4);
    float lo = __builtin_inff(), hi = -__builtin_inff();
    if (x < W && y < H) {
        const float d = depths[((size_t)blockIdx.z * H + y) * W + x];
        if (d > 0.f && d <= depth_trunc) lo = hi = d;
    }
    lo = ts_wave_min(lo);
    hi = ts_wave_max(hi);
    if ((threadIdx.x & (GSR_WAVE - 1)) == 0) {
        smin[threadIdx.x / GSR_WAVE] = lo;
        smax[threadIdx.x / GSR_WAVE] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < TS_THREADS / GSR_WAVE; w++) {
            lo = fminf(lo, smin[w]);
            hi = fmaxf(hi, smax[w]);
        }
        tiles[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = make_float2(lo, hi);
    }
}

__device__ __forceinline__ void ts_view(const float *c, float p0, float p1, float p2, float &x, float &y, float &z) {
    x = c[0] * p0 + c[3] * p1 + c[6] * p2 + c[9];
    y = c[1] * p0 + c[4] * p1 + c[7] * p2 + c[10];
    z = c[2] * p0 + c[5] * p1 + c[8] * p2 + c[11];
}
__device__ __forceinline__ float ts_pix(float x, float z, float tanfov, float S) {
    return ((x / (z * tanfov) + 1.0f) * S - 1.0f) * 0.5f;
}

// can view `c` update a voxel of brick (bx, by, bz)?  Only ever answers "no" where the per-voxel rule skips every voxel.
__device__ bool ts_brick_visible(const float *c, const TsdfGrid &g, int bx, int by, int bz, int W, int H, int TW,
                                 float tanfovx, float tanfovy, float near, float trunc,
                                 const float2 *__restrict__ tiles) {
    const float lo[3] = {g.ox + g.vs * ((float)(8 * bx) - 0.5f), g.oy + g.vs * ((float)(8 * by) - 0.5f),
                         g.oz + g.vs * ((float)(8 * bz) - 0.5f)};
    const float hi[3] = {g.ox + g.vs * ((float)(8 * bx) + 7.5f), g.oy + g.vs * ((float)(8 * by) + 7.5f),
                         g.oz + g.vs * ((float)(8 * bz) + 7.5f)};
    const float inf = __builtin_inff();
    float zmin = inf, zmax = -inf, xmin = inf, xmax = -inf, ymin = inf, ymax = -inf;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        float x, y, z;
        ts_view(c, (k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2], x, y, z);
        zmin = fminf(zmin, z);
        zmax = fmaxf(zmax, z);
        const float px = ts_pix(x, z, tanfovx, (float)W), py = ts_pix(y, z, tanfovy, (float)H);
        xmin = fminf(xmin, px);
        xmax = fmaxf(xmax, px);
        ymin = fminf(ymin, py);
        ymax = fmaxf(ymax, py);
    }
    if (!(zmax > near)) return false;              // wholly at or behind the near plane (or no finite corner at all)
    if (!(zmin > fmaxf(near, 0.f))) return true;   // straddles it: the corners' pixels bound nothing
    if (!(fabsf(xmin) < inf && fabsf(xmax) < inf && fabsf(ymin) < inf && fabsf(ymax) < inf)) return true;
    // all corners in front: the projection of the box lies inside the corners' pixel box; one pixel more than rint needs
    const float x0 = floorf(xmin) - 1.0f, x1 = ceilf(xmax) + 1.0f, y0 = floorf(ymin) - 1.0f, y1 = ceilf(ymax) + 1.0f;
    if (x1 < 0.f || y1 < 0.f || x0 > (float)(W - 1) || y0 > (float)(H - 1)) return false;
    const int tx0 = (int)fmaxf(x0, 0.f) / TS_TILE, tx1 = (int)fminf(x1, (float)(W - 1)) / TS_TILE;
    const int ty0 = (int)fmaxf(y0, 0.f) / TS_TILE, ty1 = (int)fminf(y1, (float)(H - 1)) / TS_TILE;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > TS_CULL_MAX_TILES) return true;
    float dmin = inf, dmax = -inf;
    for (int ty = ty0; ty <= ty1; ty++)
        for (int tx = tx0; tx <= tx1; tx++) {
            const float2 t = tiles[(size_t)ty * TW + tx];
            dmin = fminf(dmin, t.x);
            dmax = fmaxf(dmax, t.y);
        }
    return !(zmin > dmax + trunc || zmax < dmin - trunc);  // (no valid depth under the box: dmax = -inf, dropped)
}

template <bool COLOR>
__global__ void __launch_bounds__(TS_THREADS)
tsdf_integrate_kernel(TsdfGrid g, int V, int W, int H, int TW, int TH, const float *__restrict__ views,
                      const float *__restrict__ view_weights, float tanfovx, float tanfovy, float near,
                      float depth_trunc, float trunc, const float *__restrict__ depths,
                      const float *__restrict__ colors, const float2 *__restrict__ tiles, float *__restrict__ tsdf,
                      float *__restrict__ weight, float *__restrict__ rgb, size_t nvox) {
    __shared__ float cam_s[TS_MAX_VIEWS * TS_CAM_WORDS];
    __shared__ uint32_t mask_s;
    const int tid = threadIdx.x;
    const int b = blockIdx.x, bx = b % g.bx, by = (b / g.bx) % g.by, bz = b / (g.bx * g.by);
    for (int w = tid; w < V * TS_CAM_WORDS; w += TS_THREADS) {
        const int c = w / TS_CAM_WORDS, j = w - c * TS_CAM_WORDS;
        cam_s[w] = j < 12 ? views[c * 16 + (j / 3) * 4 + (j % 3)] : (view_weights ? view_weights[c] : 1.0f);
    }
    __syncthreads();
    if (tid < GSR_WAVE) {  // one lane per view tests the brick
        bool keep = false;
        if (tid < V)
            keep = ts_brick_visible(cam_s + tid * TS_CAM_WORDS, g, bx, by, bz, W, H, TW, tanfovx, tanfovy, near, trunc,
                                    tiles + (size_t)tid * TW * TH);
        const unsigned long long m = __ballot(keep);
        if (tid == 0) mask_s = (uint32_t)m;
    }
    __syncthreads();
    const uint32_t mask = mask_s;
    if (mask == 0) return;  // (uniform: the whole workgroup leaves before it loads a voxel)

    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int l = tid + k * TS_THREADS;
        const size_t idx = (size_t)b * TS_BRICK + l;
        const float p0 = g.ox + g.vs * (float)(8 * bx + (l & 7));
        const float p1 = g.oy + g.vs * (float)(8 * by + ((l >> 3) & 7));
        const float p2 = g.oz + g.vs * (float)(8 * bz + (l >> 6));
        float t = tsdf[idx], w = weight[idx], col[3] = {0.f, 0.f, 0.f};
        if (COLOR) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) col[ch] = rgb[ch * nvox + idx];
        }
        bool touched = false;
        for (uint32_t m = mask; m; m &= m - 1) {
            const int v = __ffs(m) - 1;
            const float *c = cam_s + v * TS_CAM_WORDS;  // wave-uniform address: an LDS broadcast
            float x, y, z;
            ts_view(c, p0, p1, p2, x, y, z);
            if (z <= near) continue;
            const float rx = rintf(ts_pix(x, z, tanfovx, (float)W)), ry = rintf(ts_pix(y, z, tanfovy, (float)H));
            if (!(rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H)) continue;
            const size_t pix = (size_t)(int)ry * W + (int)rx;
            const float d = depths[v * plane + pix];
            if (!(d > 0.f && d <= depth_trunc)) continue;
            const float sdf = d - z;
            if (!(sdf >= -trunc && sdf <= trunc)) continue;
            const float wv = c[12], wn = w + wv;
            t = (t * w + (sdf / trunc) * wv) / wn;
            if (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++)
                    col[ch] = (col[ch] * w + colors[((size_t)v * 3 + ch) * plane + pix] * wv) / wn;
            }
            w = wn;
            touched = true;
        }
        if (touched) {
            tsdf[idx] = t;
            weight[idx] = w;
            if (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) rgb[ch * nvox + idx] = col[ch];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ extraction
// the 7 owned edges as corner bits (x = 1, y = 2, z = 4), and the edge of a direction
__constant__ const uint8_t TS_EDGE_DIR[7] = {1, 2, 4, 3, 6, 5, 7};
__constant__ const uint8_t TS_EDGE_OF_DIR[8] = {0, 0, 1, 3, 2, 5, 4, 6};
// the Kuhn tetrahedra as cube corners v0 < v1 < v2 < v3 and whether det[v1 - v0, v2 - v0, v3 - v0] < 0
__constant__ const uint8_t TS_TET[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ const uint8_t TS_TET_FLIP[6] = {0, 1, 1, 0, 0, 1};
// tetrahedron edges 0..5 = (01, 02, 03, 12, 13, 23) as (lower, upper) vertex
__constant__ const uint8_t TS_TEDGE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// the triangles of a positively oriented tetrahedron by its inside mask (bit q: vertex q), normals leaving the inside.
// One inside vertex i: with (i, j, k, l) an even permutation the triangle (ij, ik, il); three: the same, reversed; two
// (i < j inside, k < l outside, k and l swapped if (i, j, k, l) is odd): the quad ik, il, jl, jk cut along ik - jl.
struct TsTetCase {
    uint8_t n, e[6];
};
__constant__ const TsTetCase TS_CASE[16] = {
    {0, {0, 0, 0, 0, 0, 0}}, {1, {0, 1, 2, 0, 0, 0}}, {1, {0, 4, 3, 0, 0, 0}}, {2, {1, 2, 4, 1, 4, 3}},
    {1, {1, 3, 5, 0, 0, 0}}, {2, {2, 0, 3, 2, 3, 5}}, {2, {0, 4, 5, 0, 5, 1}}, {1, {2, 4, 5, 0, 0, 0}},
    {1, {2, 5, 4, 0, 0, 0}}, {2, {0, 1, 5, 0, 5, 4}}, {2, {3, 0, 2, 3, 2, 5}}, {1, {1, 5, 3, 0, 0, 0}},
    {2, {1, 3, 4, 1, 4, 2}}, {1, {0, 3, 4, 0, 0, 0}}, {1, {0, 2, 1, 0, 0, 0}}, {0, {0, 0, 0, 0, 0, 0}}};

// brick-major address of voxel (x, y, z) of the volume
__device__ __forceinline__ size_t ts_addr(const TsdfGrid &g, int x, int y, int z) {
    return ((size_t)((z >> 3) * g.by + (y >> 3)) * g.bx + (x >> 3)) * TS_BRICK + (((z & 7) * 8 + (y & 7)) * 8 + (x & 7));
}
__device__ __forceinline__ int ts_halo(int hx, int hy, int hz) { return (hz * TS_HALO + hy) * TS_HALO + hx; }
__device__ __forceinline__ int ts_cell(int cx, int cy, int cz) { return (cz * TS_CELLS + cy) * TS_CELLS + cx; }

// the brick's tsdf and weight with a one-voxel halo (halo index = brick-local coordinate + 1; a voxel outside the volume
// is invalid), then the flags of the 9^3 cells whose base is brick-local -1 .. 7 (cell index = base + 1)
__device__ void ts_stage(const TsdfGrid &g, int bx, int by, int bz, const float *__restrict__ tsdf,
                         const float *__restrict__ weight, float min_weight, float *s_t, float *s_w, uint8_t *s_cell) {
    const int X = 8 * g.bx, Y = 8 * g.by, Z = 8 * g.bz;
    for (int e = threadIdx.x; e < TS_HALO3; e += TS_THREADS) {
        const int hx = e % TS_HALO, hy = (e / TS_HALO) % TS_HALO, hz = e / (TS_HALO * TS_HALO);
        const int x = 8 * bx + hx - 1, y = 8 * by + hy - 1, z = 8 * bz + hz - 1;
        float t = 0.f, w = -1.f;
        if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) {
            const size_t a = ts_addr(g, x, y, z);
            t = tsdf[a];
            w = weight[a];
        }
        s_t[e] = t;
        s_w[e] = w;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TS_CELLS3; e += TS_THREADS) {
        const int cx = e % TS_CELLS, cy = (e / TS_CELLS) % TS_CELLS, cz = e / (TS_CELLS * TS_CELLS);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float w = s_w[ts_halo(cx + (k & 1), cy + ((k >> 1) & 1), cz + (k >> 2))];
            ok = ok && w > 0.f && w >= min_weight;
        }
        s_cell[e] = ok ? 1 : 0;
    }
    __syncthreads();
}

// voxel (lx, ly, lz) of the staged brick: its edge mask, the inside bits of its cell's corners, and the triangle count
__device__ __forceinline__ void ts_voxel(const float *s_t, const uint8_t *s_cell, int lx, int ly, int lz, uint32_t &mask,
                                         uint32_t &corners, uint32_t &ntri) {
    const int h0 = ts_halo(lx + 1, ly + 1, lz + 1);
    corners = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        corners |= (s_t[h0 + (k & 1) + TS_HALO * ((k >> 1) & 1) + TS_HALO * TS_HALO * (k >> 2)] < 0.f ? 1u : 0u) << k;
    mask = 0;
#pragma unroll
    for (int e = 0; e < 7; e++) {
        const int d = TS_EDGE_DIR[e];
        if (((corners >> d) & 1u) == (corners & 1u)) continue;
        bool used = false;
#pragma unroll
        for (int o = 0; o < 8; o++)  // the cells with base voxel - o that contain both ends
            if ((o & d) == 0) used = used || s_cell[ts_cell(lx + 1 - (o & 1), ly + 1 - ((o >> 1) & 1), lz + 1 - (o >> 2))];
        if (used) mask |= 1u << e;
    }
    ntri = 0;
    if (s_cell[ts_cell(lx + 1, ly + 1, lz + 1)]) {
#pragma unroll
        for (int q = 0; q < 6; q++) {
            uint32_t m4 = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) m4 |= ((corners >> TS_TET[q][j]) & 1u) << j;
            ntri += TS_CASE[m4].n;
        }
    }
}

// exclusive scan over the workgroup in lane order; `total` in every lane (`red`: one word per wave)
__device__ __forceinline__ uint32_t ts_block_scan(uint32_t v, uint32_t *red, uint32_t &total) {
    const int lane = threadIdx.x & (GSR_WAVE - 1), wave = threadIdx.x / GSR_WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < GSR_WAVE; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, GSR_WAVE);
        if (lane >= o) inc += u;
    }
    __syncthreads();  // (the previous use of `red`)
    if (lane == GSR_WAVE - 1) red[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < TS_THREADS / GSR_WAVE; w++) {
        if (w < wave) before += red[w];
        total += red[w];
    }
    return before + inc - v;
}

__global__ void __launch_bounds__(TS_THREADS)
tsdf_count_kernel(TsdfGrid g, const float *__restrict__ tsdf, const float *__restrict__ weight, float min_weight,
                  uint32_t *__restrict__ rec, uint2 *__restrict__ btot) {
    __shared__ float s_t[TS_HALO3], s_w[TS_HALO3];
    __shared__ uint8_t s_cell[TS_CELLS3];
    __shared__ uint32_t red[TS_THREADS / GSR_WAVE];
    const int b = blockIdx.x, bx = b % g.bx, by = (b / g.bx) % g.by, bz = b / (g.bx * g.by);
    ts_stage(g, bx, by, bz, tsdf, weight, min_weight, s_t, s_w, s_cell);
    uint32_t carry = 0;  // vertices | triangles << 16 of the voxels before: at most 3584 and 6144 in a brick
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int l = threadIdx.x + k * TS_THREADS;
        uint32_t mask, corners, ntri, total;
        ts_voxel(s_t, s_cell, l & 7, (l >> 3) & 7, l >> 6, mask, corners, ntri);
        const uint32_t off = carry + ts_block_scan(__popc(mask) | (ntri << 16), red, total);
        rec[(size_t)b * TS_BRICK + l] = mask | ((off & 0xFFFFu) << 7) | ((off >> 16) << 19);
        carry += total;
    }
    if (threadIdx.x == 0) btot[b] = make_uint2(carry & 0xFFFFu, carry >> 16);
}

// exclusive scan of the brick totals by ONE workgroup, 1024 bricks per trip; totals[0..1] = vertices, triangles
__global__ void __launch_bounds__(TS_SCAN_THREADS)
tsdf_scan_kernel(int nb, const uint2 *__restrict__ btot, uint2 *__restrict__ bbase, long long *__restrict__ totals) {
    __shared__ unsigned long long red[2][TS_SCAN_THREADS / GSR_WAVE];
    const int lane = threadIdx.x & (GSR_WAVE - 1), wave = threadIdx.x / GSR_WAVE;
    unsigned long long cv = 0, ct = 0;
    for (int base = 0; base < nb; base += TS_SCAN_THREADS) {
        const int i = base + threadIdx.x;
        const uint2 v = i < nb ? btot[i] : make_uint2(0, 0);
        unsigned long long iv = v.x, it = v.y;
#pragma unroll
        for (int o = 1; o < GSR_WAVE; o <<= 1) {
            const unsigned long long uv = __shfl_up(iv, o, GSR_WAVE), ut = __shfl_up(it, o, GSR_WAVE);
            if (lane >= o) {
                iv += uv;
                it += ut;
            }
        }
        __syncthreads();  // (the previous trip has read `red`)
        if (lane == GSR_WAVE - 1) {
            red[0][wave] = iv;
            red[1][wave] = it;
        }
        __syncthreads();
        unsigned long long bv = 0, bt = 0, tv = 0, tt = 0;
        for (int w = 0; w < TS_SCAN_THREADS / GSR_WAVE; w++) {
            if (w < wave) {
                bv += red[0][w];
                bt += red[1][w];
            }
            tv += red[0][w];
            tt += red[1][w];
        }
        // (bases past 2^32 - 1 wrap here; the host refuses such totals before anything reads them)
        if (i < nb) bbase[i] = make_uint2((uint32_t)(cv + bv + iv - v.x), (uint32_t)(ct + bt + it - v.y));
        cv += tv;
        ct += tt;
    }
    if (threadIdx.x == 0) {
        totals[0] = (long long)cv;
        totals[1] = (long long)ct;
    }
}

template <bool COLOR>
__global__ void __launch_bounds__(TS_THREADS)
tsdf_emit_kernel(TsdfGrid g, const float *__restrict__ tsdf, const float *__restrict__ weight,
                 const float *__restrict__ rgb, size_t nvox, float min_weight, const uint32_t *__restrict__ rec,
                 const uint2 *__restrict__ bbase, uint32_t nv, uint32_t nt, float *__restrict__ verts,
                 int32_t *__restrict__ faces, float *__restrict__ vcolors) {
    __shared__ float s_t[TS_HALO3], s_w[TS_HALO3];
    __shared__ uint8_t s_cell[TS_CELLS3];
    const int b = blockIdx.x, bx = b % g.bx, by = (b / g.bx) % g.by, bz = b / (g.bx * g.by);
    ts_stage(g, bx, by, bz, tsdf, weight, min_weight, s_t, s_w, s_cell);
    const uint2 base = bbase[b];
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const int l = threadIdx.x + k * TS_THREADS;
        const int lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
        const uint32_t r = rec[(size_t)b * TS_BRICK + l];
        const uint32_t mask = r & 0x7Fu;
        const int x = 8 * bx + lx, y = 8 * by + ly, z = 8 * bz + lz;
        if (mask) {
            const int h0 = ts_halo(lx + 1, ly + 1, lz + 1);
            const float t0 = s_t[h0];
            const float p0[3] = {g.ox + g.vs * (float)x, g.oy + g.vs * (float)y, g.oz + g.vs * (float)z};
            const size_t a0 = (size_t)b * TS_BRICK + l;
            uint32_t vi = base.x + ((r >> 7) & 0xFFFu);
            for (int e = 0; e < 7; e++) {
                if (!((mask >> e) & 1u)) continue;
                const int d = TS_EDGE_DIR[e], dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
                const float t1 = s_t[h0 + dx + TS_HALO * dy + TS_HALO * TS_HALO * dz];
                const float f = t0 / (t0 - t1);
                const float p1[3] = {g.ox + g.vs * (float)(x + dx), g.oy + g.vs * (float)(y + dy),
                                     g.oz + g.vs * (float)(z + dz)};
                if (vi < nv) {
#pragma unroll
                    for (int c = 0; c < 3; c++) verts[(size_t)vi * 3 + c] = p0[c] + (p1[c] - p0[c]) * f;
                    if (COLOR) {
                        const size_t a1 = ts_addr(g, x + dx, y + dy, z + dz);  // (inside the volume: a processed cell uses it)
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            const float c0 = rgb[c * nvox + a0], c1 = rgb[c * nvox + a1];
                            vcolors[(size_t)vi * 3 + c] = c0 + (c1 - c0) * f;
                        }
                    }
                }
                vi++;
            }
        }
        if (!s_cell[ts_cell(lx + 1, ly + 1, lz + 1)]) continue;
        uint32_t corners = 0;
        {
            const int h0 = ts_halo(lx + 1, ly + 1, lz + 1);
#pragma unroll
            for (int c = 0; c < 8; c++)
                corners |= (s_t[h0 + (c & 1) + TS_HALO * ((c >> 1) & 1) + TS_HALO * TS_HALO * (c >> 2)] < 0.f ? 1u : 0u) << c;
        }
        if (corners == 0 || corners == 0xFFu) continue;
        uint32_t ti = base.y + (r >> 19);
        for (int q = 0; q < 6; q++) {
            uint32_t m4 = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) m4 |= ((corners >> TS_TET[q][j]) & 1u) << j;
            const TsTetCase cs = TS_CASE[m4];
            for (int n = 0; n < cs.n; n++) {
                int32_t id[3];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const int te = cs.e[3 * n + j];
                    const int ca = TS_TET[q][TS_TEDGE[te][0]], cb = TS_TET[q][TS_TEDGE[te][1]];  // ca is a subset of cb
                    const int e = TS_EDGE_OF_DIR[cb & ~ca];
                    // the owner: voxel + ca, inside the volume because this cell is processed
                    const int ox = x + (ca & 1), oy = y + ((ca >> 1) & 1), oz = z + (ca >> 2);
                    const size_t oa = ts_addr(g, ox, oy, oz);
                    const uint32_t orec = rec[oa];
                    id[j] = (int32_t)(bbase[oa / TS_BRICK].x + ((orec >> 7) & 0xFFFu) + __popc(orec & ((1u << e) - 1u)));
                }
                if (ti < nt) {
                    const bool flip = TS_TET_FLIP[q];
                    faces[(size_t)ti * 3] = id[0];
                    faces[(size_t)ti * 3 + 1] = flip ? id[2] : id[1];
                    faces[(size_t)ti * 3 + 2] = flip ? id[1] : id[2];
                }
                ti++;
            }
        }
    }
}

bool ts_grid(int X, int Y, int Z, float ox, float oy, float oz, float vs, TsdfGrid &g, long long &nb) {
    if (X <= 0 || Y <= 0 || Z <= 0 || (X & 7) || (Y & 7) || (Z & 7) || !(vs > 0.f)) return false;
    nb = (long long)(X / 8) * (Y / 8) * (Z / 8);
    if (nb > 0x7FFFFFFFLL / 8) return false;  // (brick ids, and 3 x brick id in a launch bound, stay in an int)
    g = TsdfGrid{ox, oy, oz, vs, X / 8, Y / 8, Z / 8};
    return true;
}

}  // namespace

extern "C" size_t gsr_tsdf_integrate_bytes(int views, int width, int height) {
    if (views < 0 || views > TS_MAX_VIEWS || width <= 0 || height <= 0) return 0;
    return (size_t)views * gsr_div_up(width, TS_TILE) * gsr_div_up(height, TS_TILE) * sizeof(float2);
}

extern "C" int gsr_tsdf_integrate(int X, int Y, int Z, float ox, float oy, float oz, float voxel_size, float trunc,
                                  float *tsdf, float *weight, float *rgb, int views, int width, int height,
                                  const float *viewmatrices, float tanfovx, float tanfovy, const float *depths,
                                  const float *colors, const float *view_weights, float depth_trunc, float near,
                                  void *workspace, size_t workspace_bytes, gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    TsdfGrid g;
    long long nb;
    if (!ts_grid(X, Y, Z, ox, oy, oz, voxel_size, g, nb) || !(trunc > 0.f) || views < 0 || views > TS_MAX_VIEWS ||
        width <= 0 || height <= 0 || !(tanfovx > 0.f) || !(tanfovy > 0.f) || !(near >= 0.f) || depth_trunc != depth_trunc)
        return GSR_EINVAL;
    if (!tsdf || !weight) return GSR_EINVAL;
    if (views == 0) return 0;
    if (!viewmatrices || !depths || (rgb && !colors) || !workspace) return GSR_EINVAL;
    if (workspace_bytes < gsr_tsdf_integrate_bytes(views, width, height)) return GSR_ENOSPACE;
    const int TW = gsr_div_up(width, TS_TILE), TH = gsr_div_up(height, TS_TILE);
    float2 *tiles = reinterpret_cast<float2 *>(workspace);
    hipLaunchKernelGGL(tsdf_tiles_kernel, dim3(TW, TH, views), dim3(TS_THREADS), 0, stream, width, height, depths,
                       depth_trunc, tiles);
    const size_t nvox = (size_t)nb * TS_BRICK;
    if (rgb)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, dim3((unsigned)nb), dim3(TS_THREADS), 0, stream, g, views, width,
                           height, TW, TH, viewmatrices, view_weights, tanfovx, tanfovy, near, depth_trunc, trunc, depths,
                           colors, tiles, tsdf, weight, rgb, nvox);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, dim3((unsigned)nb), dim3(TS_THREADS), 0, stream, g, views, width,
                           height, TW, TH, viewmatrices, view_weights, tanfovx, tanfovy, near, depth_trunc, trunc, depths,
                           colors, tiles, tsdf, weight, rgb, nvox);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t gsr_tsdf_extract_bytes(int X, int Y, int Z) {
    TsdfGrid g;
    long long nb;
    if (!ts_grid(X, Y, Z, 0.f, 0.f, 0.f, 1.f, g, nb)) return 0;
    return (size_t)nb * 2 * sizeof(uint2);  // the brick totals, then the brick bases
}

extern "C" int gsr_tsdf_count(int X, int Y, int Z, const float *tsdf, const float *weight, float min_weight,
                              uint32_t *records, void *workspace, size_t workspace_bytes, int64_t *totals,
                              gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    TsdfGrid g;
    long long nb;
    if (!ts_grid(X, Y, Z, 0.f, 0.f, 0.f, 1.f, g, nb) || min_weight != min_weight) return GSR_EINVAL;
    if (!tsdf || !weight || !records || !workspace || !totals) return GSR_EINVAL;
    if (workspace_bytes < gsr_tsdf_extract_bytes(X, Y, Z)) return GSR_ENOSPACE;
    uint2 *btot = reinterpret_cast<uint2 *>(workspace), *bbase = btot + nb;
    hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)nb), dim3(TS_THREADS), 0, stream, g, tsdf, weight, min_weight,
                       records, btot);
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(TS_SCAN_THREADS), 0, stream, (int)nb, btot, bbase,
                       reinterpret_cast<long long *>(totals));
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_tsdf_emit(int X, int Y, int Z, float ox, float oy, float oz, float voxel_size, const float *tsdf,
                             const float *weight, const float *rgb, float min_weight, const uint32_t *records,
                             const void *workspace, size_t workspace_bytes, int64_t num_vertices, int64_t num_triangles,
                             float *vertices, int32_t *faces, float *vertex_colors, gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    TsdfGrid g;
    long long nb;
    if (!ts_grid(X, Y, Z, ox, oy, oz, voxel_size, g, nb) || min_weight != min_weight || num_vertices < 0 ||
        num_triangles < 0 || num_vertices > 0x7FFFFFFFLL || num_triangles > 0x7FFFFFFFLL)
        return GSR_EINVAL;  // int32 indices
    if (!tsdf || !weight || !records || !workspace || (vertex_colors && !rgb)) return GSR_EINVAL;
    if (workspace_bytes < gsr_tsdf_extract_bytes(X, Y, Z)) return GSR_ENOSPACE;
    if (num_vertices == 0 && num_triangles == 0) return 0;
    if ((num_vertices && !vertices) || (num_triangles && !faces)) return GSR_EINVAL;
    const uint2 *bbase = reinterpret_cast<const uint2 *>(workspace) + nb;
    const size_t nvox = (size_t)nb * TS_BRICK;
    if (vertex_colors)
        hipLaunchKernelGGL(tsdf_emit_kernel<true>, dim3((unsigned)nb), dim3(TS_THREADS), 0, stream, g, tsdf, weight, rgb,
                           nvox, min_weight, records, bbase, (uint32_t)num_vertices, (uint32_t)num_triangles, vertices,
                           faces, vertex_colors);
    else
        hipLaunchKernelGGL(tsdf_emit_kernel<false>, dim3((unsigned)nb), dim3(TS_THREADS), 0, stream, g, tsdf, weight, rgb,
                           nvox, min_weight, records, bbase, (uint32_t)num_vertices, (uint32_t)num_triangles, vertices,
                           faces, vertex_colors);
    GSR_LAUNCH_CHECK();
    return 0;
}
