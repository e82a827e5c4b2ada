// filter3d.hip -- the 3D smoothing filter of Mip-Splatting for gfx950 (include/gsraster.h: gsr_filter3d_*).
//
// Per Gaussian one scalar f: sqrt(0.2) x (depth in the nearest training camera that sees it) / (largest focal length),
// i.e. the world-space size of 0.2^(1/2) of that camera's sampling interval.  It acts through the scales and the
// opacity only,   s'_k = sqrt(s_k^2 + f^2),   o' = sigmoid(_opacity) prod_k s_k / s'_k,
// both row-wise maps of the RAW parameters: the apply kernels hand K1 / K11 "effective raw parameters" in log and logit
// space and no projection, binning, composite or loss kernel knows about the filter.
//   filter3d_distance_kernel        one lane per row, all cameras inside the lane: 12 B in, 5 B out per row
//   filter3d_finalize_kernel        max of the workgroup partials, fill of the unseen rows, scale: 5 B in, 4 B out
//   filter3d_apply_forward_kernel   20 B in, 16 B out per row
//   filter3d_apply_backward_kernel  36 B in, 16 B out per row (everything is recomputed from the raw row)
// wave64, 256-lane workgroups, no atomics: the results do not depend on the launch geometry.
#include "common.h"

// one rounding per operation: the distance kernel restates K1's view transform and must give K1's bits (preprocess.hip
// is compiled the same way), and the apply kernels are checked against a float32 evaluation of the same formulas
#pragma clang fp contract(off)

namespace {

constexpr int F3D_BLOCK = 256;
constexpr int F3D_CAM_CHUNK = 64;   // cameras staged in LDS per pass
constexpr int F3D_CAM_WORDS = 14;   // 12 words of the view matrix (its last column is not needed) + fx + fy
constexpr int F3D_CAM_STRIDE = 40;  // floats per packed camera record (pack_camera)
constexpr int F3D_FIN_ROWS = 4;     // rows per lane of the finalize kernel

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = GSR_WAVE / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, GSR_WAVE));
    return v;
}

// max over the workgroup, in every lane (`red`: one word per wave)
__device__ __forceinline__ float block_max(float v, float *red) {
    v = wave_max(v);
    __syncthreads();  // (the previous use of `red`)
    if ((threadIdx.x & (GSR_WAVE - 1)) == 0) red[threadIdx.x / GSR_WAVE] = v;
    __syncthreads();
    float m = red[0];
#pragma unroll
    for (int w = 1; w < F3D_BLOCK / GSR_WAVE; w++) m = fmaxf(m, red[w]);
    return m;
}

__global__ void __launch_bounds__(F3D_BLOCK)
filter3d_distance_kernel(int N, int C, const float *__restrict__ xyz, const float *__restrict__ cams, int W, int H,
                         float *__restrict__ dist, uint8_t *__restrict__ seen, float *__restrict__ partials) {
    __shared__ float cam_s[F3D_CAM_CHUNK * F3D_CAM_WORDS];
    __shared__ float red[F3D_BLOCK / GSR_WAVE];
    const long long i = (long long)blockIdx.x * F3D_BLOCK + threadIdx.x;
    const bool live = i < N;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
        p[0] = xyz[3 * (size_t)i];
        p[1] = xyz[3 * (size_t)i + 1];
        p[2] = xyz[3 * (size_t)i + 2];
    }
    // Mip-Splatting's 15 % screen margin, |x_pix - W/2| <= 0.65 W, without the division by t.z
    const float limx = 0.65f * (float)W, limy = 0.65f * (float)H;
    float best = 0.f;  // 0: no camera sees the row (every valid t.z is > 0.2)
    for (int c0 = 0; c0 < C; c0 += F3D_CAM_CHUNK) {
        const int nc = min(F3D_CAM_CHUNK, C - c0);
        __syncthreads();  // (the previous chunk has been read)
        for (int w = threadIdx.x; w < nc * F3D_CAM_WORDS; w += F3D_BLOCK) {
            const int c = w / F3D_CAM_WORDS, j = w - c * F3D_CAM_WORDS;
            const float *cp = cams + (size_t)(c0 + c) * F3D_CAM_STRIDE;
            float v;
            if (j < 12) v = cp[(j / 3) * 4 + (j % 3)];              // v[4 r + col], col < 3
            else if (j == 12) v = W / (2.0f * cp[35]);              // fx, K1's expression
            else v = H / (2.0f * cp[36]);                           // fy
            cam_s[w] = v;
        }
        __syncthreads();
        for (int c = 0; c < nc; c++) {
            const float *v = cam_s + c * F3D_CAM_WORDS;  // wave-uniform address: an LDS broadcast
            // view_transform of preprocess.hip: t = [p, 1] * viewmatrix, in its order of operations
            const float tx = v[0] * p[0] + v[3] * p[1] + v[6] * p[2] + v[9];
            const float ty = v[1] * p[0] + v[4] * p[1] + v[7] * p[2] + v[10];
            const float tz = v[2] * p[0] + v[5] * p[1] + v[8] * p[2] + v[11];
            const bool valid = tz > 0.2f && fabsf(v[12] * tx) <= limx * tz && fabsf(v[13] * ty) <= limy * tz;
            if (valid) best = best > 0.f ? fminf(best, tz) : tz;
        }
    }
    if (live) {
        dist[i] = best;
        seen[i] = best > 0.f ? 1 : 0;
    }
    const float m = block_max(live ? best : 0.f, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

__global__ void __launch_bounds__(F3D_BLOCK)
filter3d_finalize_kernel(int N, const float *__restrict__ dist, const uint8_t *__restrict__ seen,
                         const float *__restrict__ partials, int n_partials, const float *__restrict__ global_max,
                         float focal_max, float *__restrict__ filter_out) {
    __shared__ float red[F3D_BLOCK / GSR_WAVE];
    float gmax;
    if (global_max) {
        gmax = global_max[0];
    } else {  // every workgroup forms the same max (order does not matter for a max of non-NaN floats)
        float m = 0.f;
        for (int k = threadIdx.x; k < n_partials; k += F3D_BLOCK) m = fmaxf(m, partials[k]);
        gmax = block_max(m, red);
    }
    const float k = 0.4472135954999579f;  // sqrt(0.2)
#pragma unroll
    for (int r = 0; r < F3D_FIN_ROWS; r++) {
        const long long i = ((long long)blockIdx.x * F3D_FIN_ROWS + r) * F3D_BLOCK + threadIdx.x;
        if (i < N) {
            const float d = seen[i] ? dist[i] : gmax;  // Mip-Splatting: distance[~valid] = distance[valid].max()
            filter_out[i] = gmax > 0.f ? (k * d) / focal_max : 0.f;
        }
    }
}

// What both apply kernels derive from one raw row, per axis, from q = f / s_k = f exp(-x_k) alone (x_k = _scaling_k):
//   q <= 1:  w = q^2,      log(s'_k / s_k) = log1p(w) / 2,           log s'_k = x_k + log1p(w) / 2
//   q >  1:  w = 1 / q^2,  log(s'_k / s_k) = log q + log1p(w) / 2,   log s'_k = log f + log1p(w) / 2
//   r_k = s_k^2 / s'_k^2 = 1 / (1 + q^2)  and  1 - r_k = f^2 / s'_k^2 = q^2 / (1 + q^2), as quotients of w.
// expf is exact to an ulp of ITS result, so q carries two roundings; going through log f^2 - 2 x_k instead would put the
// rounding of a logarithm (an ulp of |log f|, many ulps of q) into every output.  No square of a scale is formed:
// nothing under- or overflows for scales near 1e-7 or f near 1e3.  L = sum_k log(s'_k / s_k) = -log c >= 0 (a sum of
// non-negative terms) and 1 - c = -expm1(-L).
struct F3DRow {
    float ls[3];   // log s'_k
    float r[3];    // r_k
    float omr[3];  // 1 - r_k
    float L, omc;
};

__device__ __forceinline__ F3DRow f3d_row(const float x[3], float f) {
    F3DRow o;
    const float lf = logf(f);
    float L = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float q = f * expf(-x[k]);
        float l;
        if (q <= 1.0f) {
            const float w = q * q, h = 0.5f * log1pf(w), inv = 1.0f / (1.0f + w);
            l = h;
            o.ls[k] = x[k] + h;
            o.r[k] = inv;
            o.omr[k] = w * inv;
        } else {
            const float iq = 1.0f / q, w = iq * iq, h = 0.5f * log1pf(w), inv = 1.0f / (1.0f + w);
            l = logf(q) + h;
            o.ls[k] = lf + h;
            o.r[k] = w * inv;
            o.omr[k] = inv;
        }
        L = k == 0 ? l : L + l;
    }
    o.L = L;
    o.omc = -expm1f(-L);
    return o;
}

__global__ void __launch_bounds__(F3D_BLOCK)
filter3d_apply_forward_kernel(int N, const float *__restrict__ scaling, const float *__restrict__ opacity,
                              const float *__restrict__ filter, float *__restrict__ scaling_eff,
                              float *__restrict__ opacity_eff) {
    const long long i = (long long)blockIdx.x * F3D_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float x[3] = {scaling[3 * (size_t)i], scaling[3 * (size_t)i + 1], scaling[3 * (size_t)i + 2]};
    const float o = opacity[i], f = filter[i];
    if (f == 0.f) {  // the identity filter keeps every bit (the formulas below would only turn a -0 into +0)
        scaling_eff[3 * (size_t)i] = x[0];
        scaling_eff[3 * (size_t)i + 1] = x[1];
        scaling_eff[3 * (size_t)i + 2] = x[2];
        opacity_eff[i] = o;
        return;
    }
    const F3DRow r = f3d_row(x, f);
#pragma unroll
    for (int k = 0; k < 3; k++) scaling_eff[3 * (size_t)i + k] = r.ls[k];
    // logit(sigmoid(o) c) = o + log c - log1p((1 - c) e^o); above o = 60 (sigmoid(o) == 1 in fp32 long before) e^o is
    // kept from overflowing by the equal form log c - log(e^-o + (1 - c))
    opacity_eff[i] = o <= 60.f ? (o - r.L) - log1pf(r.omc * expf(o))
                               : -r.L - logf(expf(-fminf(o, 80.f)) + r.omc);
}

__global__ void __launch_bounds__(F3D_BLOCK)
filter3d_apply_backward_kernel(int N, const float *__restrict__ scaling, const float *__restrict__ opacity,
                               const float *__restrict__ filter, const float *__restrict__ g_scaling,
                               const float *__restrict__ g_opacity, float *__restrict__ d_scaling,
                               float *__restrict__ d_opacity) {
    const long long i = (long long)blockIdx.x * F3D_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float gs[3] = {g_scaling[3 * (size_t)i], g_scaling[3 * (size_t)i + 1], g_scaling[3 * (size_t)i + 2]};
    const float go = g_opacity[i], f = filter[i];
    if (f == 0.f) {
        d_scaling[3 * (size_t)i] = gs[0];
        d_scaling[3 * (size_t)i + 1] = gs[1];
        d_scaling[3 * (size_t)i + 2] = gs[2];
        d_opacity[i] = go;
        return;
    }
    const float x[3] = {scaling[3 * (size_t)i], scaling[3 * (size_t)i + 1], scaling[3 * (size_t)i + 2]};
    const float o = opacity[i];
    const F3DRow r = f3d_row(x, f);
    // with sigma = sigmoid(o), p = sigma c:  1 - p = (1 - sigma) + sigma (1 - c), a sum of non-negative terms, so
    //   u = 1 / (1 - p)  and  v = (1 - sigma) / (1 - p)  come without a subtraction:
    //   o <= 0:  D = 1 + e^o (1 - c),     u = (1 + e^o) / D,   v = 1 / D
    //   o >  0:  D = e^-o + (1 - c),      u = (e^-o + 1) / D,  v = e^-o / D
    float u, v;
    if (o <= 0.f) {
        const float e = expf(o), D = 1.0f + e * r.omc;
        u = (1.0f + e) / D;
        v = 1.0f / D;
    } else {
        const float e = expf(-fminf(o, 80.f)), D = e + r.omc;
        u = (e + 1.0f) / D;
        v = e / D;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) d_scaling[3 * (size_t)i + k] = gs[k] * r.r[k] + (go * r.omr[k]) * u;
    d_opacity[i] = go * v;
}

}  // namespace

extern "C" int gsr_filter3d_num_partials(int N) { return N <= 0 ? 0 : gsr_div_up(N, F3D_BLOCK); }

extern "C" int gsr_filter3d_distance(int N, int C, const float *xyz, const float *cams, int width, int height,
                                     float *dist, uint8_t *seen, float *partials, gsr_stream_t stream) {
    if (N < 0 || C < 0 || width <= 0 || height <= 0) return GSR_EINVAL;
    if (N == 0) return 0;
    if (!xyz || (C > 0 && !cams) || !dist || !seen || !partials) return GSR_EINVAL;
    hipLaunchKernelGGL(filter3d_distance_kernel, dim3(gsr_div_up(N, F3D_BLOCK)), dim3(F3D_BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), N, C, xyz, cams, width, height, dist, seen, partials);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_filter3d_finalize(int N, const float *dist, const uint8_t *seen, const float *partials,
                                     int n_partials, const float *global_max, float focal_max, float *filter_out,
                                     gsr_stream_t stream) {
    if (N < 0 || n_partials < 0) return GSR_EINVAL;
    if (N == 0) return 0;
    if (!dist || !seen || !filter_out || (!global_max && (!partials || n_partials != gsr_filter3d_num_partials(N))))
        return GSR_EINVAL;
    if (!(focal_max > 0.f)) return GSR_EINVAL;
    hipLaunchKernelGGL(filter3d_finalize_kernel, dim3(gsr_div_up(N, F3D_BLOCK * F3D_FIN_ROWS)), dim3(F3D_BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), N, dist, seen, partials, n_partials, global_max, focal_max,
                       filter_out);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_filter3d_apply_forward(int N, const float *scaling, const float *opacity, const float *filter,
                                          float *scaling_eff, float *opacity_eff, gsr_stream_t stream) {
    if (N < 0) return GSR_EINVAL;
    if (N == 0) return 0;
    if (!scaling || !opacity || !filter || !scaling_eff || !opacity_eff) return GSR_EINVAL;
    hipLaunchKernelGGL(filter3d_apply_forward_kernel, dim3(gsr_div_up(N, F3D_BLOCK)), dim3(F3D_BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), N, scaling, opacity, filter, scaling_eff, opacity_eff);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_filter3d_apply_backward(int N, const float *scaling, const float *opacity, const float *filter,
                                           const float *g_scaling, const float *g_opacity, float *d_scaling,
                                           float *d_opacity, gsr_stream_t stream) {
    if (N < 0) return GSR_EINVAL;
    if (N == 0) return 0;
    if (!scaling || !opacity || !filter || !g_scaling || !g_opacity || !d_scaling || !d_opacity) return GSR_EINVAL;
    hipLaunchKernelGGL(filter3d_apply_backward_kernel, dim3(gsr_div_up(N, F3D_BLOCK)), dim3(F3D_BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), N, scaling, opacity, filter, g_scaling, g_opacity,
                       d_scaling, d_opacity);
    GSR_LAUNCH_CHECK();
    return 0;
}
