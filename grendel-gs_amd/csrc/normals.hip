// normals.hip -- depth-normal consistency for gfx950 (include/gsraster.h: gsr_normal_rows_*, gsr_normal_consistency_*).
//
// The regulariser of 2DGS / PGSR / RaDe-GS / GOF / CityGaussianV2, loss = weight / (H W) sum_p (1 - A* N . n_d):
//   normal_rows_forward_kernel          one lane per Gaussian: the row (1, t_z, n) gsr_render_features blends into
//                                       F = (A, D, N): shortest axis of the raw row, rotated into the camera, flipped to
//                                       face it.  40 + 4 B in, 20 B out per row; the view matrix through the scalar cache
//   normal_rows_backward_kernel         its backward into xyz (through t_z) and the raw quaternion (through R[:,k] and the
//                                       normalisation); sigma and k are constants.  60 + 4 B in, 28 B out, no atomics
//   normal_consistency_forward_kernel   one workgroup per 64 x 8 pixel tile: z = D / A once per pixel into an LDS tile
//                                       with a one-pixel halo, n_d and e in registers, one fp64 partial per workgroup
//   normal_consistency_finalize_kernel  the partials in a fixed order -> the fp32 loss
//   normal_consistency_backward_kernel  gather form, two LDS phases (z with a two-pixel halo; g_x = dL/d(dx), g_y =
//                                       dL/d(dy) on the tile plus one pixel), no atomics: the same bits on every run
// wave64, 256-lane workgroups.  In the tile phases a wave is one row of 64 pixels: every LDS access of a wave, the +-1
// gathers in x and in y included, is 64 consecutive words, free of bank conflicts whatever the stride.  The halo phases
// walk their region linearly with the region's own width as the stride: consecutive words again (where they read the
// wider z tile, a wave that wraps a row skips two words: at most two lanes share a bank).
#include "common.h"

// one rounding per operation: t_z is K1's `depths` bit for bit (preprocess.hip carries the same pragma), the decisions
// (argmin, the sign, A > 1e-6, |c|^2 > 1e-24) are those of a plain float32 evaluation, and a hole (z = 0 on all four
// neighbours) gives c = 0 exactly
#pragma clang fp contract(off)

namespace {

constexpr int NR_BLOCK = GSR_ONE_DIM_BLOCK;
constexpr int NC_TX = GSR_NORMALS_TILE_X, NC_TY = GSR_NORMALS_TILE_Y;
constexpr int NC_BLOCK = 256;
constexpr int NC_ROWS_PER_LANE = NC_TX * NC_TY / NC_BLOCK;  // 2: a lane takes the rows ly and ly + 4 of its column
constexpr int NC_WAVES = NC_BLOCK / GSR_WAVE;
constexpr int NC_FW = NC_TX + 2, NC_FH = NC_TY + 2;         // forward: z on the tile + 1
constexpr int NC_ZW = NC_TX + 4, NC_ZH = NC_TY + 4;         // backward: z on the tile + 2
constexpr int NC_GW = NC_TX + 2, NC_GH = NC_TY + 2;         // backward: g_x, g_y on the tile + 1
static_assert(NC_TX == GSR_WAVE, "a wave is one row of the tile");
static_assert(NC_TX * NC_TY % NC_BLOCK == 0, "whole rows per lane");

// ------------------------------------------------------------------------------------------- (a) surfel rows
struct NrRow {
    float t[3];    // position in camera space
    float4 q;      // normalised quaternion
    float qnr, qn;
    int k;         // the shortest axis
    float ac[3];   // R[:,k] in camera space
    float sigma;
};

__device__ __forceinline__ void nr_quat_to_R(const float4 q, float R[3][3]) {  // preprocess.hip's quat_to_R
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    R[0][0] = 1.f - 2.f * (y * y + z * z);
    R[0][1] = 2.f * (x * y - r * z);
    R[0][2] = 2.f * (x * z + r * y);
    R[1][0] = 2.f * (x * y + r * z);
    R[1][1] = 1.f - 2.f * (x * x + z * z);
    R[1][2] = 2.f * (y * z - r * x);
    R[2][0] = 2.f * (x * z - r * y);
    R[2][1] = 2.f * (y * z + r * x);
    R[2][2] = 1.f - 2.f * (x * x + y * y);
}

__device__ __forceinline__ NrRow nr_row(size_t i, const float *__restrict__ xyz, const float *__restrict__ scaling,
                                        const float *__restrict__ rotation, const float (&v)[16]) {
    NrRow o;
    const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    // view_transform of preprocess.hip, in its order of operations
    o.t[0] = v[0] * p[0] + v[4] * p[1] + v[8] * p[2] + v[12];
    o.t[1] = v[1] * p[0] + v[5] * p[1] + v[9] * p[2] + v[13];
    o.t[2] = v[2] * p[0] + v[6] * p[1] + v[10] * p[2] + v[14];
    const float s0 = scaling[3 * i], s1 = scaling[3 * i + 1], s2 = scaling[3 * i + 2];
    int k = 0;  // raw log-scales order like the scales; a tie keeps the lowest index
    float sm = s0;
    if (s1 < sm) {
        sm = s1;
        k = 1;
    }
    if (s2 < sm) k = 2;
    o.k = k;
    const float4 qr = *reinterpret_cast<const float4 *>(rotation + 4 * i);
    o.qnr = sqrtf(qr.x * qr.x + qr.y * qr.y + qr.z * qr.z + qr.w * qr.w);
    o.qn = fmaxf(o.qnr, 1e-12f);
    o.q = make_float4(qr.x / o.qn, qr.y / o.qn, qr.z / o.qn, qr.w / o.qn);
    float R[3][3];
    nr_quat_to_R(o.q, R);
    float aw[3];
#pragma unroll
    for (int m = 0; m < 3; m++) aw[m] = k == 0 ? R[m][0] : (k == 1 ? R[m][1] : R[m][2]);
#pragma unroll
    for (int j = 0; j < 3; j++) o.ac[j] = aw[0] * v[j] + aw[1] * v[4 + j] + aw[2] * v[8 + j];
    const float d = o.ac[0] * o.t[0] + o.ac[1] * o.t[1] + o.ac[2] * o.t[2];
    o.sigma = d > 0.f ? -1.f : 1.f;
    return o;
}

__global__ void __launch_bounds__(NR_BLOCK)
normal_rows_forward_kernel(int P, const float *__restrict__ xyz, const float *__restrict__ scaling,
                           const float *__restrict__ rotation, const int32_t *__restrict__ radii,
                           const float *__restrict__ view, float *__restrict__ rows) {
    const long long il = (long long)blockIdx.x * NR_BLOCK + threadIdx.x;
    if (il >= P) return;
    const size_t i = (size_t)il;
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = view[j];  // wave-uniform: scalar loads
    float out[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (radii[i] > 0) {
        const NrRow r = nr_row(i, xyz, scaling, rotation, v);
        out[0] = 1.f;
        out[1] = r.t[2];
        out[2] = r.sigma * r.ac[0];
        out[3] = r.sigma * r.ac[1];
        out[4] = r.sigma * r.ac[2];
    }
#pragma unroll
    for (int c = 0; c < 5; c++) rows[5 * i + c] = out[c];
}

__global__ void __launch_bounds__(NR_BLOCK)
normal_rows_backward_kernel(int P, const float *__restrict__ xyz, const float *__restrict__ scaling,
                            const float *__restrict__ rotation, const int32_t *__restrict__ radii,
                            const float *__restrict__ view, const float *__restrict__ g, float *__restrict__ d_xyz,
                            float *__restrict__ d_rotation) {
    const long long il = (long long)blockIdx.x * NR_BLOCK + threadIdx.x;
    if (il >= P) return;
    const size_t i = (size_t)il;
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = view[j];
    float dp[3] = {0.f, 0.f, 0.f};
    float4 dq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (radii[i] > 0) {
        const NrRow r = nr_row(i, xyz, scaling, rotation, v);
        const float g1 = g[5 * i + 1];
        dp[0] = g1 * v[2];
        dp[1] = g1 * v[6];
        dp[2] = g1 * v[10];
        const float dac[3] = {r.sigma * g[5 * i + 2], r.sigma * g[5 * i + 3], r.sigma * g[5 * i + 4]};
        float dR[3][3];  // only column k carries a gradient
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const float daw = dac[0] * v[4 * m] + dac[1] * v[4 * m + 1] + dac[2] * v[4 * m + 2];
#pragma unroll
            for (int j = 0; j < 3; j++) dR[m][j] = j == r.k ? daw : 0.f;
        }
        const float r_ = r.q.x, x = r.q.y, y = r.q.z, z = r.q.w;
        // dR -> dq, cov3d_backward's expressions (preprocess.hip)
        dq.x = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
        dq.y = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r_ * dR[1][2] + z * dR[2][0] +
                      r_ * dR[2][1] - 2.f * x * dR[2][2]);
        dq.z = 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r_ * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r_ * dR[2][0] +
                      z * dR[2][1] - 2.f * y * dR[2][2]);
        dq.w = 2.f * (-2.f * z * dR[0][0] - r_ * dR[0][1] + x * dR[0][2] + r_ * dR[1][0] - 2.f * z * dR[1][1] +
                      y * dR[1][2] + x * dR[2][0] + y * dR[2][1]);
        // through q = x / max(|x|, 1e-12): the clamp rule of cov3d_backward<RAW = true>
        const float dot = r.qnr > 1e-12f ? (r.q.x * dq.x + r.q.y * dq.y + r.q.z * dq.z + r.q.w * dq.w) : 0.f;
        dq = make_float4((dq.x - r.q.x * dot) / r.qn, (dq.y - r.q.y * dot) / r.qn, (dq.z - r.q.z * dot) / r.qn,
                         (dq.w - r.q.w * dot) / r.qn);
    }
    d_xyz[3 * i] = dp[0];
    d_xyz[3 * i + 1] = dp[1];
    d_xyz[3 * i + 2] = dp[2];
    *reinterpret_cast<float4 *>(d_rotation + 4 * i) = dq;
}

// ------------------------------------------------------------------------------------------- (b) consistency loss
// the pixel-centre ray of project_geometry: ((2 i + 1) / n - 1) tan
__device__ __forceinline__ float nc_ray(int i, int n, float tanfov) {
    return ((float)(2 * i + 1) / (float)n - 1.f) * tanfov;
}

__device__ __forceinline__ float nc_depth(const float *__restrict__ F, size_t plane, int W, int H, int x, int y) {
    if (x < 0 || y < 0 || x >= W || y >= H) return 0.f;
    const size_t p = (size_t)y * W + x;
    const float A = F[p];
    return A > 1e-6f ? F[plane + p] / A : 0.f;
}

struct NcGeom {
    float dx[3], dy[3], c[3], l2;
};

// the finite differences of X = z ray around the interior pixel (x, y) and c = dy x dx
__device__ __forceinline__ NcGeom nc_geom(float zl, float zr, float zu, float zd, int x, int y, int W, int H, float tanx,
                                          float tany) {
    const float rxl = nc_ray(x - 1, W, tanx), rxc = nc_ray(x, W, tanx), rxr = nc_ray(x + 1, W, tanx);
    const float ryu = nc_ray(y - 1, H, tany), ryc = nc_ray(y, H, tany), ryd = nc_ray(y + 1, H, tany);
    NcGeom o;
    o.dx[0] = zr * rxr - zl * rxl;
    o.dx[1] = zr * ryc - zl * ryc;
    o.dx[2] = zr - zl;
    o.dy[0] = zd * rxc - zu * rxc;
    o.dy[1] = zd * ryd - zu * ryu;
    o.dy[2] = zd - zu;
    o.c[0] = o.dy[1] * o.dx[2] - o.dy[2] * o.dx[1];
    o.c[1] = o.dy[2] * o.dx[0] - o.dy[0] * o.dx[2];
    o.c[2] = o.dy[0] * o.dx[1] - o.dy[1] * o.dx[0];
    o.l2 = o.c[0] * o.c[0] + o.c[1] * o.c[1] + o.c[2] * o.c[2];
    return o;
}

__device__ __forceinline__ double nc_wave_sum(double v) {
#pragma unroll
    for (int o = GSR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GSR_WAVE);
    return v;
}

__global__ void __launch_bounds__(NC_BLOCK)
normal_consistency_forward_kernel(int W, int H, int tiles_x, int n_tiles, const float *__restrict__ F, float tanx,
                                  float tany, float *__restrict__ nd_out, double *__restrict__ partials) {
    __shared__ float zs[NC_FH * NC_FW];
    __shared__ double red[NC_WAVES];
    const int tile = gsr_xcd_span_of_block(blockIdx.x, n_tiles);
    const int x0 = (tile % tiles_x) * NC_TX, y0 = (tile / tiles_x) * NC_TY;
    const size_t plane = (size_t)W * H;
    for (int idx = threadIdx.x; idx < NC_FH * NC_FW; idx += NC_BLOCK) {
        const int ry = idx / NC_FW, rx = idx - ry * NC_FW;
        zs[idx] = nc_depth(F, plane, W, H, x0 + rx - 1, y0 + ry - 1);
    }
    __syncthreads();
    const int lx = threadIdx.x & (NC_TX - 1), ly0 = threadIdx.x / NC_TX;
    const int x = x0 + lx;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < NC_ROWS_PER_LANE; r++) {
        const int ly = ly0 + r * (NC_BLOCK / NC_TX), y = y0 + ly;
        if (x >= W || y >= H) continue;
        const size_t p = (size_t)y * W + x;
        float n[3] = {0.f, 0.f, 0.f};
        if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {
            const int ctr = (ly + 1) * NC_FW + lx + 1;
            const NcGeom gm = nc_geom(zs[ctr - 1], zs[ctr + 1], zs[ctr - NC_FW], zs[ctr + NC_FW], x, y, W, H, tanx, tany);
            if (gm.l2 > 1e-24f) {
                const float len = sqrtf(gm.l2);
                n[0] = gm.c[0] / len;
                n[1] = gm.c[1] / len;
                n[2] = gm.c[2] / len;
            }
            const float dot = F[2 * plane + p] * n[0] + F[3 * plane + p] * n[1] + F[4 * plane + p] * n[2];
            acc += (double)(1.f - F[p] * dot);
        }
        if (nd_out) {
            nd_out[p] = n[0];
            nd_out[plane + p] = n[1];
            nd_out[2 * plane + p] = n[2];
        }
    }
    acc = nc_wave_sum(acc);
    if ((threadIdx.x & (GSR_WAVE - 1)) == 0) red[threadIdx.x / GSR_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
#pragma unroll
        for (int w = 1; w < NC_WAVES; w++) s += red[w];
        partials[tile] = s;
    }
}

__global__ void __launch_bounds__(NC_BLOCK)
normal_consistency_finalize_kernel(int n_partials, const double *__restrict__ partials, double scale,
                                   float *__restrict__ loss) {
    __shared__ double red[NC_BLOCK];
    double s = 0.0;
    for (int k = threadIdx.x; k < n_partials; k += NC_BLOCK) s += partials[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = NC_BLOCK / 2; o > 0; o >>= 1) {  // a fixed tree: the same bits on every run
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] * scale);
}

__global__ void __launch_bounds__(NC_BLOCK)
normal_consistency_backward_kernel(int W, int H, int tiles_x, int n_tiles, const float *__restrict__ F, float tanx,
                                   float tany, float scale, const float *__restrict__ g_loss, float *__restrict__ dF) {
    __shared__ float zs[NC_ZH * NC_ZW];
    __shared__ float gs[6][NC_GH * NC_GW];  // planes 0..2: g_x, 3..5: g_y
    const int tile = gsr_xcd_span_of_block(blockIdx.x, n_tiles);
    const int x0 = (tile % tiles_x) * NC_TX, y0 = (tile / tiles_x) * NC_TY;
    const size_t plane = (size_t)W * H;
    const float k = -(g_loss ? scale * g_loss[0] : scale);  // -weight / (H W) times the incoming gradient
    for (int idx = threadIdx.x; idx < NC_ZH * NC_ZW; idx += NC_BLOCK) {
        const int ry = idx / NC_ZW, rx = idx - ry * NC_ZW;
        zs[idx] = nc_depth(F, plane, W, H, x0 + rx - 2, y0 + ry - 2);
    }
    __syncthreads();
    // phase 1: g_x = dL/d(dx) = v x dy and g_y = dL/d(dy) = dx x v on the tile plus one pixel; dL/dN on the tile
    for (int idx = threadIdx.x; idx < NC_GH * NC_GW; idx += NC_BLOCK) {
        const int ry = idx / NC_GW, rx = idx - ry * NC_GW;
        const int x = x0 + rx - 1, y = y0 + ry - 1;
        float gx[3] = {0.f, 0.f, 0.f}, gy[3] = {0.f, 0.f, 0.f}, dN[3] = {0.f, 0.f, 0.f};
        if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {
            const int ctr = (ry + 1) * NC_ZW + rx + 1;
            const NcGeom gm = nc_geom(zs[ctr - 1], zs[ctr + 1], zs[ctr - NC_ZW], zs[ctr + NC_ZW], x, y, W, H, tanx, tany);
            if (gm.l2 > 1e-24f) {
                const size_t p = (size_t)y * W + x;
                const float len = sqrtf(gm.l2);
                const float n[3] = {gm.c[0] / len, gm.c[1] / len, gm.c[2] / len};
                const float s = k * F[p];  // A is a constant here (the detached weight of 2DGS)
                const float dn[3] = {s * F[2 * plane + p], s * F[3 * plane + p], s * F[4 * plane + p]};
                const float d = n[0] * dn[0] + n[1] * dn[1] + n[2] * dn[2];
                const float v[3] = {(dn[0] - n[0] * d) / len, (dn[1] - n[1] * d) / len, (dn[2] - n[2] * d) / len};
                gx[0] = v[1] * gm.dy[2] - v[2] * gm.dy[1];
                gx[1] = v[2] * gm.dy[0] - v[0] * gm.dy[2];
                gx[2] = v[0] * gm.dy[1] - v[1] * gm.dy[0];
                gy[0] = gm.dx[1] * v[2] - gm.dx[2] * v[1];
                gy[1] = gm.dx[2] * v[0] - gm.dx[0] * v[2];
                gy[2] = gm.dx[0] * v[1] - gm.dx[1] * v[0];
                dN[0] = s * n[0];
                dN[1] = s * n[1];
                dN[2] = s * n[2];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            gs[c][idx] = gx[c];
            gs[3 + c][idx] = gy[c];
        }
        if (rx >= 1 && rx <= NC_TX && ry >= 1 && ry <= NC_TY && x < W && y < H) {
            const size_t p = (size_t)y * W + x;
            dF[2 * plane + p] = dN[0];
            dF[3 * plane + p] = dN[1];
            dF[4 * plane + p] = dN[2];
        }
    }
    __syncthreads();
    // phase 2: dL/dX(p) = g_x(p - e_x) - g_x(p + e_x) + g_y(p - e_y) - g_y(p + e_y), then z = D / A
    const int lx = threadIdx.x & (NC_TX - 1), ly0 = threadIdx.x / NC_TX;
    const int x = x0 + lx;
#pragma unroll
    for (int r = 0; r < NC_ROWS_PER_LANE; r++) {
        const int ly = ly0 + r * (NC_BLOCK / NC_TX), y = y0 + ly;
        if (x >= W || y >= H) continue;
        const size_t p = (size_t)y * W + x;
        const int ctr = (ly + 1) * NC_GW + lx + 1;
        float dX[3];
#pragma unroll
        for (int c = 0; c < 3; c++)
            dX[c] = ((gs[c][ctr - 1] - gs[c][ctr + 1]) + gs[3 + c][ctr - NC_GW]) - gs[3 + c][ctr + NC_GW];
        const float dz = dX[0] * nc_ray(x, W, tanx) + dX[1] * nc_ray(y, H, tany) + dX[2];
        const float A = F[p];
        float dA = 0.f, dD = 0.f;
        if (A > 1e-6f) {
            dD = dz / A;
            dA = -(dz * F[plane + p]) / (A * A);
        }
        dF[p] = dA;
        dF[plane + p] = dD;
    }
}

}  // namespace

int gsr_launch_normal_rows_forward(int P, const float *xyz, const float *scaling, const float *rotation,
                                   const int32_t *radii, const float *viewmatrix, float *rows, hipStream_t stream) {
    hipLaunchKernelGGL(normal_rows_forward_kernel, dim3(gsr_div_up(P, NR_BLOCK)), dim3(NR_BLOCK), 0, stream, P, xyz,
                       scaling, rotation, radii, viewmatrix, rows);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_normal_rows_backward(int P, const float *xyz, const float *scaling, const float *rotation,
                                    const int32_t *radii, const float *viewmatrix, const float *g, float *d_xyz,
                                    float *d_rotation, hipStream_t stream) {
    hipLaunchKernelGGL(normal_rows_backward_kernel, dim3(gsr_div_up(P, NR_BLOCK)), dim3(NR_BLOCK), 0, stream, P, xyz,
                       scaling, rotation, radii, viewmatrix, g, d_xyz, d_rotation);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_normal_consistency_tiles(int W, int H, int *tiles_x) {
    const int tx = gsr_div_up(W, NC_TX), ty = gsr_div_up(H, NC_TY);
    if (tiles_x) *tiles_x = tx;
    return tx * ty;
}

int gsr_launch_normal_consistency_forward(int W, int H, const float *F, float tanfovx, float tanfovy, float weight,
                                          double *partials, float *loss, float *normals, hipStream_t stream) {
    int tiles_x;
    const int n_tiles = gsr_normal_consistency_tiles(W, H, &tiles_x);
    hipLaunchKernelGGL(normal_consistency_forward_kernel, dim3(n_tiles), dim3(NC_BLOCK), 0, stream, W, H, tiles_x,
                       n_tiles, F, tanfovx, tanfovy, normals, partials);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(normal_consistency_finalize_kernel, dim3(1), dim3(NC_BLOCK), 0, stream, n_tiles, partials,
                       (double)weight / ((double)H * (double)W), loss);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_normal_consistency_backward(int W, int H, const float *F, float tanfovx, float tanfovy, float weight,
                                           const float *g_loss, float *dL_dF, hipStream_t stream) {
    int tiles_x;
    const int n_tiles = gsr_normal_consistency_tiles(W, H, &tiles_x);
    hipLaunchKernelGGL(normal_consistency_backward_kernel, dim3(n_tiles), dim3(NC_BLOCK), 0, stream, W, H, tiles_x,
                       n_tiles, F, tanfovx, tanfovy, weight / ((float)H * (float)W), g_loss, dL_dF);
    GSR_LAUNCH_CHECK();
    return 0;
}
