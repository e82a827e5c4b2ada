// bilagrid.hip -- per-image bilateral-grid colour correction (slice forward / backward, total variation) for gfx950.
//
// One camera's grid G[12][L][GH][GW] holds a [3,4] affine colour transform per lattice node; a pixel at (x, y) of a
// W x H image with rendered colour c = (r, g, b) samples it trilinearly at
//   px = (x + 0.5) / W * (GW - 1),  py = (y + 0.5) / H * (GH - 1),  pz = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) * (L - 1)
// (lower node i0 = min(floor(p), size - 2), t = p - i0, every axis as a + t (b - a): x, then y, then z) and leaves
// x' = A_M c + b_M (include/gsraster.h, N1g).
//
// Work split, the same for the forward and the backward: a workgroup owns a PIECE -- at most 32 x 32 pixels of ONE
// xy-cell of the lattice, walked as chunks of 32 x 8 pixels with one lane per pixel.  All pixels of a piece share their
// four xy-corners, so the 4 * L * 12 node values they can touch (at most 3 KiB) are staged in LDS once, whatever the grid
// and image sizes: there is no "does not fit" path.  A cell's pixel range comes from the SAME float expression the pixels
// use (a binary search over the monotonic pixel -> cell map), so cells partition the image exactly as the pixels see it.
//
// Lattice gradient (deterministic, no floating-point atomics): the pixel lanes of a chunk leave (g' (x) [c, 1], the four
// xy-corner weights, tz) in LDS; then every wave walks ITS 64 pixels level by level of the guide axis (a ballot of
// z0 == l, set bits in lane order) with 48 owner lanes, one per (xy-corner, coefficient), adding the two levels a pixel
// feeds in fp64 registers and, per level, into the wave's own LDS sums.  A piece writes the four waves' sums, added in
// wave order, once (fp32), and a finalize pass adds the pieces of the up to four cells around each node in a fixed order
// in fp64 and rounds once.
#include "common.h"

namespace {

constexpr int BT = 256;            // threads per workgroup = pixels per chunk
constexpr int PW = 32, PH = 32;    // pixels of a piece
constexpr int CW = 32, CH = BT / CW;  // a chunk: 32 x 8 pixels
constexpr int MAXL = 16;
constexpr int PSTR = 17;           // floats per staged pixel record (odd: conflict-free writes)

// pixel / row index -> continuous lattice coordinate and the cell (lower node) it falls in.  Host and device evaluate
// the same three correctly-rounded operations; nothing here can contract to an fma.
__host__ __device__ inline float bg_coord(int i, int n, int g) { return ((float)i + 0.5f) / (float)n * (float)(g - 1); }
__host__ __device__ inline int bg_cell(float p, int g) {
    const int c = (int)p;
    return c < g - 2 ? c : g - 2;
}
// the first i in [0, n] whose cell is >= c (the map is monotonic): cell c holds [bg_first(c), bg_first(c + 1))
__device__ inline int bg_first(int c, int n, int g) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bg_cell(bg_coord(mid, n, g), g) >= c) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

struct Piece {
    int cx, cy;          // the xy-cell
    int xa, xb, ya, yb;  // its pixels [xa, xb) x [ya, yb) (rows not yet clipped to the band)
    int tx0, ty0;        // first pixel of this workgroup's first tile
};

// block -> (cell, piece of the cell); -> false: the piece holds no pixel of the band
__device__ inline bool bg_piece(Piece &p, int W, int H, int gw, int gh, int npx, int npy, int y0, int y1) {
    int b = blockIdx.x;
    const int px = b % npx;
    b /= npx;
    const int py = b % npy;
    b /= npy;
    p.cx = b % (gw - 1);
    p.cy = b / (gw - 1);
    p.xa = bg_first(p.cx, W, gw);
    p.xb = bg_first(p.cx + 1, W, gw);
    p.ya = bg_first(p.cy, H, gh);
    p.yb = bg_first(p.cy + 1, H, gh);
    p.tx0 = p.xa + PW * px;
    p.ty0 = p.ya + PH * py;
    return p.tx0 < p.xb && p.ty0 < min(p.yb, y1) && p.yb > y0;
}

// the 4 * L * 12 node values of the cell: sG[(q * L + l) * 12 + j], q = 2 dy + dx the xy-corner
__device__ inline void bg_stage_nodes(float *sG, const float *__restrict__ grid, const Piece &p, int gw, int gh, int gl) {
    const int per = gl * 12;
    for (int s = threadIdx.x; s < 4 * per; s += BT) {
        const int q = s / per, r = s - q * per;
        const int l = r / 12, j = r - l * 12;
        sG[s] = grid[(((size_t)j * gl + l) * gh + (p.cy + (q >> 1))) * gw + (p.cx + (q & 1))];
    }
}

// luminance with every rounding spelled out (the fp32 restatement forms the same bits), -> z0, tz; live = the guide has
// a derivative here (0 < lum < 1: torch's border rule gives exactly 0 at and beyond the ends)
__device__ inline void bg_guide(float r, float g, float b, int gl, int &z0, float &tz, bool &live) {
    const float lum = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, r), __fmul_rn(0.587f, g)), __fmul_rn(0.114f, b));
    live = lum > 0.f && lum < 1.f;
    const float pz = fminf(fmaxf(lum, 0.f), 1.f) * (float)(gl - 1);
    z0 = min((int)pz, gl - 2);
    tz = pz - (float)z0;
}

__device__ inline float bg_lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// M[j] = the trilinear sample of coefficient j; DZ: also dM[j] = dM_j / dpz, the bilinear sample of G[z0 + 1] - G[z0]
template <bool DZ>
__device__ inline void bg_sample(const float *sG, int gl, float tx, float ty, int z0, float tz, float *M, float *dM) {
    const int per = gl * 12;
    const float *n0 = sG + z0 * 12;
#pragma unroll
    for (int j = 0; j < 12; j++) {
        const float a00 = n0[j], a10 = n0[per + j], a01 = n0[2 * per + j], a11 = n0[3 * per + j];
        const float b00 = n0[12 + j], b10 = n0[per + 12 + j], b01 = n0[2 * per + 12 + j], b11 = n0[3 * per + 12 + j];
        const float lo = bg_lerp(bg_lerp(a00, a10, tx), bg_lerp(a01, a11, tx), ty);
        const float hi = bg_lerp(bg_lerp(b00, b10, tx), bg_lerp(b01, b11, tx), ty);
        M[j] = bg_lerp(lo, hi, tz);
        if (DZ) dM[j] = bg_lerp(bg_lerp(b00 - a00, b10 - a10, tx), bg_lerp(b01 - a01, b11 - a11, tx), ty);
    }
}

__global__ void __launch_bounds__(BT)
bilagrid_forward_kernel(int W, int H, int y0, int y1, const float *__restrict__ image, long long cs,
                        const float *__restrict__ grid, int gw, int gh, int gl, int npx, int npy,
                        float *__restrict__ out, long long ocs) {
    __shared__ float sG[4 * MAXL * 12];
    Piece p;
    if (!bg_piece(p, W, H, gw, gh, npx, npy, y0, y1)) return;
    bg_stage_nodes(sG, grid, p, gw, gh, gl);
    __syncthreads();
    const int lx = threadIdx.x & (CW - 1), ly = threadIdx.x / CW;
    const int ylo = max(p.ya, y0), yhi = min(p.yb, y1);
    for (int ty = p.ty0; ty < yhi; ty += PH * npy) {
        for (int tx = p.tx0; tx < p.xb; tx += PW * npx) {
            for (int sub = 0; sub < PH / CH; sub++) {
                const int x = tx + lx, y = ty + sub * CH + ly;
                if (x >= p.xb || y < ylo || y >= yhi) continue;
                const size_t at = (size_t)y * W + x;
                const float r = image[at], g = image[at + cs], b = image[at + 2 * cs];
                int z0;
                float tz, M[12];
                bool live;
                bg_guide(r, g, b, gl, z0, tz, live);
                bg_sample<false>(sG, gl, bg_coord(x, W, gw) - (float)p.cx, bg_coord(y, H, gh) - (float)p.cy, z0, tz, M,
                                 nullptr);
#pragma unroll
                for (int c = 0; c < 3; c++)
                    out[at + c * ocs] = fmaf(M[4 * c], r, fmaf(M[4 * c + 1], g, fmaf(M[4 * c + 2], b, M[4 * c + 3])));
            }
        }
    }
}

__global__ void __launch_bounds__(BT)
bilagrid_backward_kernel(int W, int H, int y0, int y1, const float *__restrict__ image, long long cs,
                         const float *__restrict__ grid, int gw, int gh, int gl, int npx, int npy,
                         const float *__restrict__ gout, long long gcs, float *__restrict__ gimg, long long ics,
                         float *__restrict__ partials) {
    __shared__ float sG[4 * MAXL * 12];
    __shared__ float sP[BT * PSTR];
    extern __shared__ double sA[];  // [BT / 64][4 * gl * 12]: every wave's own corner sums
    const int per = gl * 12, nslots = 4 * per;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = tid; s < (BT / 64) * nslots; s += BT) sA[s] = 0.0;
#ifdef GSR_ABL_BILAGRID_FIXEDPOINT
    __shared__ unsigned long long sAcc[4 * MAXL * 12];
    for (int s = tid; s < nslots; s += BT) sAcc[s] = 0ull;
#endif
    // lanes 0..47 of a wave own one (xy-corner, coefficient) pair each, at every level of the guide axis
    const int oq = min(lane / 12, 3), oj = lane % 12;
    double *const mine = sA + (size_t)wave * nslots + oq * per + oj;  // + 12 l: this lane's sum at level l
    const float *const wrec = sP + wave * 64 * PSTR;                   // the records of this wave's own 64 pixels
    Piece p;
    if (bg_piece(p, W, H, gw, gh, npx, npy, y0, y1)) {
        bg_stage_nodes(sG, grid, p, gw, gh, gl);
        __syncthreads();
        const int lx = tid & (CW - 1), ly = tid / CW;
        const int ylo = max(p.ya, y0), yhi = min(p.yb, y1);
        for (int ty = p.ty0; ty < yhi; ty += PH * npy) {
            for (int tx = p.tx0; tx < p.xb; tx += PW * npx) {
                for (int sub = 0; sub < PH / CH; sub++) {
                    const int cy0 = ty + sub * CH;
                    if (cy0 >= yhi || cy0 + CH <= ylo) continue;  // (uniform) no row of the chunk is in the band
                    const int x = tx + lx, y = cy0 + ly;
                    float rec[17];  // g' (x) [c, 1] (12), the four xy-corner weights, tz
                    int z0 = -1;    // (a lane without a pixel matches no level)
#pragma unroll
                    for (int i = 0; i < 17; i++) rec[i] = 0.f;
                    if (x < p.xb && y >= ylo && y < yhi) {
                        const size_t at = (size_t)y * W + x;
                        const float c[3] = {image[at], image[at + cs], image[at + 2 * cs]};
                        const float g[3] = {gout[at], gout[at + gcs], gout[at + 2 * gcs]};
                        float tz, M[12], dM[12];
                        bool live;
                        bg_guide(c[0], c[1], c[2], gl, z0, tz, live);
                        const float fx = bg_coord(x, W, gw) - (float)p.cx, fy = bg_coord(y, H, gh) - (float)p.cy;
                        bg_sample<true>(sG, gl, fx, fy, z0, tz, M, dM);
                        float D = 0.f;
#pragma unroll
                        for (int ch = 0; ch < 3; ch++) {
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const float o = k < 3 ? g[ch] * c[k] : g[ch];
                                rec[4 * ch + k] = o;
                                D = fmaf(dM[4 * ch + k], o, D);
                            }
                        }
                        D = live ? D * (float)(gl - 1) : 0.f;
                        const float lw[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
                        for (int k = 0; k < 3; k++)
                            gimg[at + k * ics] = fmaf(lw[k], D, fmaf(M[k], g[0], fmaf(M[4 + k], g[1], M[8 + k] * g[2])));
                        const float wx0 = 1.f - fx, wy0 = 1.f - fy;
                        rec[12] = wx0 * wy0;
                        rec[13] = fx * wy0;
                        rec[14] = wx0 * fy;
                        rec[15] = fx * fy;
                        rec[16] = tz;
                    }
#ifdef GSR_ABL_BILAGRID_FIXEDPOINT
                    // A rejected variant (EXPERIMENTS.md): every pixel lane adds its 8 x 12 contributions to the
                    // piece's sums with 64-bit INTEGER LDS atomics at a fixed scale of 2^40 -- order-independent, but
                    // the absolute resolution of 2^-40 is a relative one only for gradients of a known magnitude
                    // (|sum| < 2^23 per piece), which a loss divided by the pixel count does not have.
                    if (z0 >= 0) {
#pragma unroll
                        for (int q = 0; q < 4; q++)
#pragma unroll
                            for (int dz = 0; dz < 2; dz++) {
                                const float w = rec[12 + q] * (dz ? rec[16] : 1.f - rec[16]);
#pragma unroll
                                for (int j = 0; j < 12; j++)
                                    atomicAdd(&sAcc[(q * gl + z0 + dz) * 12 + j],
                                              (unsigned long long)__double2ll_rn((double)(w * rec[j]) * 1099511627776.0));
                            }
                    }
                    continue;
#endif
#pragma unroll
                    for (int i = 0; i < 17; i++) sP[tid * PSTR + i] = rec[i];
                    __syncthreads();
                    // The wave walks ITS 64 pixels level by level of the guide axis, within a level in lane order (the
                    // set bits of a ballot): a pixel at level l feeds the sums of levels l and l + 1 only, so the owner
                    // lanes keep those two in registers (fp64) and add them to the wave's LDS sums when the level is
                    // done.  Every lane of the wave reads the same record: broadcast reads.
                    for (int l = 0; l < gl - 1; l++) {
                        unsigned long long m = __ballot(z0 == l);
                        if (!m) continue;
                        double lo = 0.0, hi = 0.0;
                        do {
                            const float *pr = wrec + __builtin_ctzll(m) * PSTR;
                            m &= m - 1;
                            const float tz = pr[16], wxy = pr[12 + oq], o = pr[oj];
                            lo += (double)((wxy * (1.f - tz)) * o);
                            hi += (double)((wxy * tz) * o);
                        } while (m);
                        if (lane < 48) {
                            mine[12 * l] += lo;
                            mine[12 * l + 12] += hi;
                        }
                    }
                    __syncthreads();
                }
            }
        }
    }
    __syncthreads();
    // every workgroup writes its piece's row, zeros included (the finalize reads all of them): the four waves' sums in
    // wave order
    float *row = partials + (size_t)blockIdx.x * nslots;
    for (int s = tid; s < nslots; s += BT) {
#ifdef GSR_ABL_BILAGRID_FIXEDPOINT
        row[s] = (float)((double)(long long)sAcc[s] * (1.0 / 1099511627776.0));
#else
        row[s] = (float)(((sA[s] + sA[nslots + s]) + sA[2 * nslots + s]) + sA[3 * nslots + s]);
#endif
    }
}

// grad_grid[j][l][gy][gx] = the sum, in a fixed order in fp64, of corner q of every piece of the up to four cells around
// the node; rounded once.  Threads run j fastest so that neighbouring lanes read neighbouring floats of a piece's row.
__global__ void __launch_bounds__(BT)
bilagrid_finalize_kernel(int gw, int gh, int gl, int npieces, const float *__restrict__ partials,
                         float *__restrict__ grad_grid) {
    const int t = blockIdx.x * BT + threadIdx.x;
    const int per = gl * 12;
    if (t >= per * gw * gh) return;
    const int r = t % per, node = t / per;
    const int l = r / 12, j = r - l * 12;
    const int gx = node % gw, gy = node / gw;
    double a = 0.0;
    for (int dy = 1; dy >= 0; dy--) {
        const int cy = gy - dy;
        if (cy < 0 || cy > gh - 2) continue;
        for (int dx = 1; dx >= 0; dx--) {
            const int cx = gx - dx;
            if (cx < 0 || cx > gw - 2) continue;
            const float *src = partials + ((size_t)(cy * (gw - 1) + cx) * npieces * 4 + (2 * dy + dx)) * per + r;
            for (int pc = 0; pc < npieces; pc++) a += (double)src[(size_t)pc * 4 * per];
        }
    }
    grad_grid[(((size_t)j * gl + l) * gh + gy) * gw + gx] = (float)a;
}

// ------------------------------------------------------------------------------------------- total variation
// T = (1/N) sum over the axes of mean((G shifted by one - G)^2); one lane per element adds weight * dT/dG into grad:
// dT/dG[i] = sum_axis 2 / (N cnt_axis) * ((G[i] - G[i - 1]) - (G[i + 1] - G[i])), a missing neighbour dropping its term.
// sx, sy, sz = weight * 2 / (N cnt_axis); vx, vy, vz = 1 / cnt_axis (the value's forward differences, fp64 sums).
template <bool VALUE>
__global__ void __launch_bounds__(BT)
bilagrid_tv_kernel(long long n, int gw, int gh, int gl, const float *__restrict__ G, float sx, float sy, float sz,
                   float *__restrict__ grad, double vx, double vy, double vz, double *__restrict__ partials) {
    const long long i = (long long)blockIdx.x * BT + threadIdx.x;
    double e = 0.0;
    if (i < n) {
        const int x = (int)(i % gw), y = (int)((i / gw) % gh), z = (int)((i / ((long long)gw * gh)) % gl);
        const long long ys = gw, zs = (long long)gw * gh;
        const float v = G[i];
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (x > 0) dx = v - G[i - 1];
        if (y > 0) dy = v - G[i - ys];
        if (z > 0) dz = v - G[i - zs];
        if (x < gw - 1) {
            const float d = G[i + 1] - v;
            dx -= d;
            if (VALUE) e += vx * ((double)d * (double)d);
        }
        if (y < gh - 1) {
            const float d = G[i + ys] - v;
            dy -= d;
            if (VALUE) e += vy * ((double)d * (double)d);
        }
        if (z < gl - 1) {
            const float d = G[i + zs] - v;
            dz -= d;
            if (VALUE) e += vz * ((double)d * (double)d);
        }
        grad[i] += fmaf(sx, dx, fmaf(sy, dy, sz * dz));
    }
    if (VALUE) {
        __shared__ double red[BT / 64];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) e += __shfl_xor(e, d, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
        __syncthreads();
        if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// one workgroup: value = scale * the sum of the block sums, lanes 256 apart, then a fixed tree
__global__ void __launch_bounds__(BT)
bilagrid_tv_finalize_kernel(int nb, const double *__restrict__ partials, double scale, float *__restrict__ value) {
    __shared__ double red[BT];
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += BT) a += partials[i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = BT / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *value = (float)(red[0] * scale);
}

constexpr int MAX_EXTENT = 1 << 24;  // pixel indices are formed as floats

bool sizes_ok(int gw, int gh, int gl) { return gw >= 2 && gw <= 64 && gh >= 2 && gh <= 64 && gl >= 2 && gl <= MAXL; }

// pieces one cell needs along an axis of n pixels under g nodes: its widest cell in pixels / 32, rounded up (>= 1)
int pieces_along(int n, int g, int span) {
    int widest = 1, run = 0, prev = -1;
    for (int i = 0; i < n; i++) {
        const int c = bg_cell(bg_coord(i, n, g), g);
        run = c == prev ? run + 1 : 1;
        prev = c;
        if (run > widest) widest = run;
    }
    return gsr_div_up(widest, span);
}

}  // namespace

extern "C" int64_t gsr_bilagrid_num_partials(int width, int height, int gw, int gh, int gl) {
    if (width <= 0 || height <= 0 || width > MAX_EXTENT || height > MAX_EXTENT || !sizes_ok(gw, gh, gl)) return 0;
    return (int64_t)(gw - 1) * (gh - 1) * pieces_along(width, gw, PW) * pieces_along(height, gh, PH) * 4 * gl * 12;
}

static int slice_args(int width, int height, int y0, int y1, int gw, int gh, int gl) {
    if (width <= 0 || height <= 0 || width > MAX_EXTENT || height > MAX_EXTENT || !sizes_ok(gw, gh, gl)) return GSR_EINVAL;
    if (y0 < 0 || y1 > height || y0 > y1) return GSR_EINVAL;
    return 0;
}

extern "C" int gsr_bilagrid_slice_forward(int width, int height, int y0, int y1, const float *image,
                                          int64_t image_channel_stride, const float *grid, int gw, int gh, int gl,
                                          float *out, int64_t out_channel_stride, gsr_stream_t stream) {
    if (slice_args(width, height, y0, y1, gw, gh, gl) || !image || !grid || !out) return GSR_EINVAL;
    if (y0 == y1) return 0;
    const int npx = pieces_along(width, gw, PW), npy = pieces_along(height, gh, PH);
    const long long blocks = (long long)(gw - 1) * (gh - 1) * npx * npy;
    if (blocks > 0x7fffffffLL) return GSR_EINVAL;
    hipLaunchKernelGGL(bilagrid_forward_kernel, dim3((unsigned)blocks), dim3(BT), 0, reinterpret_cast<hipStream_t>(stream),
                       width, height, y0, y1, image, (long long)image_channel_stride, grid, gw, gh, gl, npx, npy, out,
                       (long long)out_channel_stride);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_bilagrid_slice_backward(int width, int height, int y0, int y1, const float *image,
                                           int64_t image_channel_stride, const float *grid, int gw, int gh, int gl,
                                           const float *grad_out, int64_t grad_out_channel_stride, float *grad_image,
                                           int64_t grad_image_channel_stride, float *partials, float *grad_grid,
                                           gsr_stream_t stream) {
    if (slice_args(width, height, y0, y1, gw, gh, gl)) return GSR_EINVAL;
    if (!image || !grid || !grad_out || !grad_image || !partials || !grad_grid) return GSR_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t nodes = (size_t)12 * gl * gh * gw;
    if (y0 == y1) {
        GSR_HIP(hipMemsetAsync(grad_grid, 0, nodes * sizeof(float), st));
        return 0;
    }
    const int npx = pieces_along(width, gw, PW), npy = pieces_along(height, gh, PH);
    const long long blocks = (long long)(gw - 1) * (gh - 1) * npx * npy;
    if (blocks > 0x7fffffffLL) return GSR_EINVAL;
    const size_t wave_sums = (size_t)(BT / 64) * 4 * gl * 12 * sizeof(double);  // <= 24 KiB of dynamic LDS
    hipLaunchKernelGGL(bilagrid_backward_kernel, dim3((unsigned)blocks), dim3(BT), wave_sums, st, width, height, y0, y1, image,
                       (long long)image_channel_stride, grid, gw, gh, gl, npx, npy, grad_out,
                       (long long)grad_out_channel_stride, grad_image, (long long)grad_image_channel_stride, partials);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(bilagrid_finalize_kernel, dim3(gsr_div_up((long long)nodes, BT)), dim3(BT), 0, st, gw, gh, gl,
                       npx * npy, partials, grad_grid);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_bilagrid_tv_num_partials(int num_grids, int gw, int gh, int gl) {
    if (num_grids <= 0 || !sizes_ok(gw, gh, gl)) return 0;
    return gsr_div_up((long long)num_grids * 12 * gl * gh * gw, BT);
}

extern "C" int gsr_bilagrid_tv(int num_grids, int gw, int gh, int gl, const float *grids, float weight, float *grad,
                               double *partials, float *value, gsr_stream_t stream) {
    if (num_grids <= 0 || !sizes_ok(gw, gh, gl) || !grids || !grad) return GSR_EINVAL;
    if ((value != nullptr) != (partials != nullptr)) return GSR_EINVAL;
    const long long n = (long long)num_grids * 12 * gl * gh * gw;
    const long long blocks = gsr_div_up(n, BT);
    if (n > (1LL << 38)) return GSR_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double cx = 12.0 * (gw - 1) * gh * gl, cy = 12.0 * gw * (gh - 1) * gl, cz = 12.0 * gw * gh * (gl - 1);
    const double s = 2.0 * (double)weight / num_grids;
    if (value) {
        hipLaunchKernelGGL(bilagrid_tv_kernel<true>, dim3((unsigned)blocks), dim3(BT), 0, st, n, gw, gh, gl, grids,
                           (float)(s / cx), (float)(s / cy), (float)(s / cz), grad, 1.0 / cx, 1.0 / cy, 1.0 / cz, partials);
        GSR_LAUNCH_CHECK();
        hipLaunchKernelGGL(bilagrid_tv_finalize_kernel, dim3(1), dim3(BT), 0, st, (int)blocks, partials,
                           1.0 / num_grids, value);
    } else {
        hipLaunchKernelGGL(bilagrid_tv_kernel<false>, dim3((unsigned)blocks), dim3(BT), 0, st, n, gw, gh, gl, grids,
                           (float)(s / cx), (float)(s / cy), (float)(s / cz), grad, 0.0, 0.0, 0.0, (double *)nullptr);
    }
    GSR_LAUNCH_CHECK();
    return 0;
}
