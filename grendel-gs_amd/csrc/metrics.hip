// metrics.hip -- fused evaluation metrics of one row band (forward only) for gfx950.
//
// Replaces the stock-PyTorch sequence of the reference's training_report (train_internal.py:471-478: two clamps,
// l1_loss(...).mean(), psnr(...).mean() -> utils/image_utils.py:19-21) and of metrics.py:78-79 (ssim / psnr of the saved
// PNGs) -- about ten element-wise launches over an image that every rank first all-reduces in full -- by ONE launch over
// the rows [y0, y1) a rank rendered.  Everything the reference prints is a sum over pixels, so the band sums of the
// ranks add up to the image's:
//   x = clamp(image, 0, 1)            (QUANTIZE: x = q / 255, q = floor(clamp(x * 255 + 0.5, 0, 255)), the byte a PNG holds)
//   y = gt * (1 / 255f)               (as loss.hip forms it)
//   per channel: sum |x - y|, sum (x - y)^2, sum ssim_map(x, y)
// The SSIM map is loss.hip's (11x11 window, sigma 1.5, C1 = 0.01^2, C2 = 0.03^2, same tile, same register sliding
// windows, same packed pairs) with ONE difference: the window reads the image's rows [max(0, y0 - 5), min(H, y1 + 5)), the
// zero padding is at the IMAGE's edges only.  A rank finds its neighbours' five rows in its own full-size image (they
// are exchanged as strips, evaluation.py), so the band sums of the SSIM map add up as well.
// With NO_SSIM the launch is a pure stream over the band (no halo, no LDS staging) with the same partial layout.
#include "common.h"

namespace {

__constant__ const float WIN[11] = {1.0283801239e-03f, 7.5987582095e-03f, 3.6000773311e-02f, 1.0936068743e-01f,
                                    2.1300552785e-01f, 2.6601171494e-01f, 2.1300552785e-01f, 1.0936068743e-01f,
                                    3.6000773311e-02f, 7.5987582095e-03f, 1.0283801239e-03f};
constexpr int LT = 512;                    // threads per workgroup of the SSIM form (the loss forward's choice)
constexpr int VO = 1024 / LT;              // vertical outputs per thread
constexpr int TW = 32, TH = 32;            // output tile of one workgroup (both forms: one partial triple per tile)
constexpr int HW = TW + 10, HH = TH + 10;  // halo tile
constexpr int HSTR = TW + 8;               // row stride of the horizontal-pass results (4 rows = 32 banks apart)
constexpr int HV = (TW + 16) / 4;          // aligned 4-element vectors per halo row: columns [ox - 8, ox + TW + 8)
constexpr int ST = 256;                    // threads per workgroup of the stream form: 4 adjacent pixels each
constexpr float SSIM_C1 = 0.01f * 0.01f;
constexpr float SSIM_C2 = 0.03f * 0.03f;
static_assert(HH * HV <= LT, "one halo vector per thread");
static_assert(ST * 4 == TW * TH, "the stream form covers a tile with one 4-pixel group per thread");

typedef float v2f __attribute__((ext_vector_type(2)));

template <int NT>
__device__ __forceinline__ float block_sum(float v, float *smem) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if (lane == 0) smem[wave] = v;
    __syncthreads();
    float r = 0.f;
    for (int w = 0; w < NT / 64; w++) r += smem[w];
    __syncthreads();
    return r;
}

// A product / sum that is rounded on its own.  (The rounded-operation intrinsics of the HIP headers are the plain
// operators, which the compiler is free to contract with a neighbouring operation into one fma; contraction is switched
// off for exactly these two.)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
// y of a ground-truth byte, and x of a quantised one: the SAME rounded product, so that x == y exactly when q == gt
__device__ __forceinline__ float unit_of_byte(float b) { return mul_rn(b, 1.0f / 255.0f); }

// the byte render.py saves: mul(255).add_(0.5).clamp_(0, 255).to(uint8) on the clamped value -- multiply and add rounded
// separately, so that q is that sequence's bit for bit
__device__ __forceinline__ float quantize_byte(float x01) {
    const float t = add_rn(mul_rn(x01, 255.0f), 0.5f);
    return floorf(fminf(fmaxf(t, 0.f), 255.f));
}
template <bool QUANT>
__device__ __forceinline__ float stage_x(float v) {
    const float x = fminf(fmaxf(v, 0.f), 1.f);
    return QUANT ? unit_of_byte(quantize_byte(x)) : x;
}
// the byte of a staged value: a quantised x is q * (1/255f), which rounds back to q exactly (q <= 255)
template <bool QUANT>
__device__ __forceinline__ uint8_t byte_of(float x) {
    return (uint8_t)(QUANT ? rintf(x * 255.0f) : quantize_byte(x));
}

template <bool VEC, bool QUANT>
__global__ void __launch_bounds__(LT)
image_metrics_kernel(int H, int W, int y0, int y1, int gxT, int gyT, const float *__restrict__ image,
                     long long img_cstride, const uint8_t *__restrict__ gt, long long gt_cstride,
                     float *__restrict__ partials, uint8_t *__restrict__ out_u8) {
    __shared__ v2f sXY[HH][HW + 1];     // (x, y): staged rendered rows / ground truth
    __shared__ v2f hAB[HH][HSTR];       // horizontal pass of (x, y)
    __shared__ v2f hCD[HH][HSTR];       // ... of (x^2, y^2)
    __shared__ float hE[HH][HSTR];      // ... of x y
    __shared__ float red[LT / 64];
    const int nwg = gridDim.x;
    const int tile_id = gsr_xcd_span_of_block(blockIdx.x, nwg);
    const int c = tile_id / (gxT * gyT);
    const int rem = tile_id - c * (gxT * gyT);
    const int by = rem / gxT;
    const int ox = (rem - by * gxT) * TW, oy = y0 + by * TH;
    const int tid = threadIdx.x;
    const int r_lo = max(0, y0 - 5), r_hi = min(H, y1 + 5);  // the rows the window may read
    const float *img_c = image + (long long)c * img_cstride;
    const uint8_t *gt_c = gt + (long long)c * gt_cstride;
    if (VEC) {
        if (tid < HH * HV) {
            const int ly = tid / HV, q = tid - ly * HV;
            const int gy = oy + ly - 5, gx0 = ox - 8 + 4 * q;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            uchar4 y = make_uchar4(0, 0, 0, 0);
            const bool in = gy >= r_lo && gy < r_hi && gx0 >= 0 && gx0 < W;  // W % 4 == 0: inside or outside as a whole
            if (in) {
                x = *reinterpret_cast<const float4 *>(img_c + (size_t)gy * W + gx0);
                y = *reinterpret_cast<const uchar4 *>(gt_c + (size_t)gy * W + gx0);
            }
            const float xs[4] = {x.x, x.y, x.z, x.w};
            const float ys[4] = {(float)y.x, (float)y.y, (float)y.z, (float)y.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int lx = 4 * q - 3 + i;
                if (lx >= 0 && lx < HW)
                    sXY[ly][lx] = in ? v2f{stage_x<QUANT>(xs[i]), unit_of_byte(ys[i])} : v2f{0.f, 0.f};
            }
        }
    } else {
        for (int idx = tid; idx < HH * HW; idx += LT) {
            const int ly = idx / HW, lx = idx % HW;
            const int gy = oy + ly - 5, gx = ox + lx - 5;
            v2f v = {0.f, 0.f};
            if (gy >= r_lo && gy < r_hi && gx >= 0 && gx < W) {
                v.x = stage_x<QUANT>(img_c[(size_t)gy * W + gx]);
                v.y = unit_of_byte((float)gt_c[(size_t)gy * W + gx]);
            }
            sXY[ly][lx] = v;
        }
    }
    __syncthreads();
    for (int task = tid; task < HH * (TW / 4); task += LT) {
        const int r = task / (TW / 4), cx0 = (task % (TW / 4)) * 4;
        v2f xy[14], sq[14];
        float pr[14];
#pragma unroll
        for (int i = 0; i < 14; i++) {
            xy[i] = sXY[r][cx0 + i];
            sq[i] = xy[i] * xy[i];
            pr[i] = xy[i].x * xy[i].y;
        }
#pragma unroll
        for (int o = 0; o < 4; o++) {
            v2f a = {0.f, 0.f}, b = {0.f, 0.f};
            float e = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float w = WIN[k];
                a += xy[o + k] * w;
                b += sq[o + k] * w;
                e += pr[o + k] * w;
            }
            hAB[r][cx0 + o] = a;
            hCD[r][cx0 + o] = b;
            hE[r][cx0 + o] = e;
        }
    }
    __syncthreads();
    const int tx = tid % TW, ty0 = (tid / TW) * VO;
    v2f vab[VO], vcd[VO];
    float ve[VO];
    {
        v2f p[10 + VO], q[10 + VO];
        float t[10 + VO];
#pragma unroll
        for (int i = 0; i < 10 + VO; i++) {
            p[i] = hAB[ty0 + i][tx];
            q[i] = hCD[ty0 + i][tx];
            t[i] = hE[ty0 + i][tx];
        }
#pragma unroll
        for (int o = 0; o < VO; o++) {
            v2f a = {0.f, 0.f}, b = {0.f, 0.f};
            float e = 0.f;
#pragma unroll
            for (int k = 0; k < 11; k++) {
                const float w = WIN[k];
                a += p[o + k] * w;
                b += q[o + k] * w;
                e += t[o + k] * w;
            }
            vab[o] = a;
            vcd[o] = b;
            ve[o] = e;
        }
    }
    const int gx = ox + tx;
    float l1 = 0.f, sse = 0.f, ssim_sum = 0.f;
#pragma unroll
    for (int o = 0; o < VO; o++) {
        const int ty = ty0 + o, gy = oy + ty;
        if (gy < y1 && gx < W) {
            const float mu1 = vab[o].x, mu2 = vab[o].y, e11 = vcd[o].x, e22 = vcd[o].y, e12 = ve[o];
            const v2f cxy = sXY[ty + 5][tx + 5];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
            const float A = 2.f * mu12 + SSIM_C1, B = 2.f * s12 + SSIM_C2;
            const float Cd = mu1_sq + mu2_sq + SSIM_C1, Dd = s1 + s2 + SSIM_C2;
            const float inv = __builtin_amdgcn_rcpf(Cd) * __builtin_amdgcn_rcpf(Dd);  // Cd, Dd >= C1, C2 > 0
            ssim_sum += A * B * inv;
            const float d = cxy.x - cxy.y;
            l1 += fabsf(d);
            sse += d * d;
            if (out_u8) out_u8[((size_t)c * (y1 - y0) + (gy - y0)) * W + gx] = byte_of<QUANT>(cxy.x);
        }
    }
    const float sl1 = block_sum<LT>(l1, red);
    const float sse_ = block_sum<LT>(sse, red);
    const float sss = block_sum<LT>(ssim_sum, red);
    if (tid == 0) {  // indexed by tile, not by workgroup: the finalize adds them in the same fixed order either way
        partials[3 * (size_t)tile_id] = sl1;
        partials[3 * (size_t)tile_id + 1] = sse_;
        partials[3 * (size_t)tile_id + 2] = sss;
    }
}

// NO_SSIM: 15 bytes per pixel in (fp32 image, uint8 ground truth, three channels), nothing else -- what the training
// report needs (it prints L1 and PSNR).  One 32x32 tile per workgroup as above, a thread owns 4 adjacent pixels of a row.
template <bool VEC, bool QUANT>
__global__ void __launch_bounds__(ST)
image_metrics_stream_kernel(int W, int y0, int y1, int gxT, int gyT, const float *__restrict__ image,
                            long long img_cstride, const uint8_t *__restrict__ gt, long long gt_cstride,
                            float *__restrict__ partials, uint8_t *__restrict__ out_u8) {
    __shared__ float red[ST / 64];
    const int tile_id = blockIdx.x;
    const int c = tile_id / (gxT * gyT);
    const int rem = tile_id - c * (gxT * gyT);
    const int by = rem / gxT;
    const int tid = threadIdx.x;
    const int gy = y0 + by * TH + tid / (TW / 4), gx0 = (rem - by * gxT) * TW + 4 * (tid % (TW / 4));
    float l1 = 0.f, sse = 0.f;
    if (gy < y1 && gx0 < W) {
        const float *ip = image + (long long)c * img_cstride + (size_t)gy * W + gx0;
        const uint8_t *gp = gt + (long long)c * gt_cstride + (size_t)gy * W + gx0;
        float xs[4] = {0.f, 0.f, 0.f, 0.f}, ys[4] = {0.f, 0.f, 0.f, 0.f};
        const int n = min(4, W - gx0);
        if (VEC) {  // W % 4 == 0: n == 4
            const float4 x = *reinterpret_cast<const float4 *>(ip);
            const uchar4 y = *reinterpret_cast<const uchar4 *>(gp);
            xs[0] = x.x, xs[1] = x.y, xs[2] = x.z, xs[3] = x.w;
            ys[0] = (float)y.x, ys[1] = (float)y.y, ys[2] = (float)y.z, ys[3] = (float)y.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < n) {
                    xs[i] = ip[i];
                    ys[i] = (float)gp[i];
                }
        }
        uint8_t *op = out_u8 ? out_u8 + ((size_t)c * (y1 - y0) + (gy - y0)) * W + gx0 : nullptr;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < n) {
                const float x = stage_x<QUANT>(xs[i]);
                const float d = x - unit_of_byte(ys[i]);  // y rounded first, as the staged y of the SSIM form
                l1 += fabsf(d);
                sse += d * d;
                if (op) op[i] = byte_of<QUANT>(x);
            }
    }
    const float sl1 = block_sum<ST>(l1, red);
    const float sse_ = block_sum<ST>(sse, red);
    if (tid == 0) {
        partials[3 * (size_t)tile_id] = sl1;
        partials[3 * (size_t)tile_id + 1] = sse_;
        partials[3 * (size_t)tile_id + 2] = 0.f;
    }
}

// one workgroup per channel: its tiles' partials are contiguous; a thread adds every 256th triple in fp64, then a fixed
// shuffle tree and a fixed order over the four waves -- two runs on the same partials give the same bits
__global__ void __launch_bounds__(256) image_metrics_finalize_kernel(int per_channel, const float *__restrict__ partials,
                                                                      double *__restrict__ sums) {
    __shared__ double red[3][4];
    const float *p = partials + 3 * (size_t)blockIdx.x * per_channel;
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < per_channel; i += 256) {
#pragma unroll
        for (int j = 0; j < 3; j++) a[j] += (double)p[3 * (size_t)i + j];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a[j] += __shfl_xor(a[j], d, 64);
        if ((threadIdx.x & 63) == 0) red[j][threadIdx.x >> 6] = a[j];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int j = threadIdx.x;
        sums[3 * (size_t)blockIdx.x + j] = ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
    }
}

}  // namespace

static inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" int gsr_image_metrics_num_partials(int channels, int rows, int width) {
    if (channels <= 0 || rows <= 0 || width <= 0) return 0;
    return channels * gsr_div_up(rows, TH) * gsr_div_up(width, TW);
}

template <bool VEC, bool QUANT>
static void launch_metrics(bool ssim, int grid, hipStream_t s, int H, int W, int y0, int y1, int gxT, int gyT,
                           const float *image, long long ics, const uint8_t *gt, long long gcs, float *partials,
                           uint8_t *out_u8) {
    if (ssim)
        hipLaunchKernelGGL((image_metrics_kernel<VEC, QUANT>), dim3(grid), dim3(LT), 0, s, H, W, y0, y1, gxT, gyT, image,
                           ics, gt, gcs, partials, out_u8);
    else
        hipLaunchKernelGGL((image_metrics_stream_kernel<VEC, QUANT>), dim3(grid), dim3(ST), 0, s, W, y0, y1, gxT, gyT,
                           image, ics, gt, gcs, partials, out_u8);
}

extern "C" int gsr_image_metrics(int channels, int height, int width, const float *image, int64_t image_channel_stride,
                                 const uint8_t *gt, int64_t gt_channel_stride, int y0, int y1, int flags,
                                 float *partials, uint8_t *out_u8, gsr_stream_t stream) {
    if (channels <= 0 || height <= 0 || width <= 0) return GSR_EINVAL;
    if (!image || !gt || !partials) return GSR_EINVAL;
    if (y0 < 0 || y0 >= y1 || y1 > height) return GSR_EINVAL;
    if (flags & ~(GSR_METRICS_QUANTIZE | GSR_METRICS_NO_SSIM)) return GSR_EINVAL;
    if (image_channel_stride < (int64_t)height * width || gt_channel_stride < (int64_t)height * width) return GSR_EINVAL;
    const int gxT = gsr_div_up(width, TW), gyT = gsr_div_up(y1 - y0, TH);
    const int grid = gxT * gyT * channels;
    const bool vec = width % 4 == 0 && image_channel_stride % 4 == 0 && gt_channel_stride % 4 == 0 &&
                     aligned_to(image, 16) && aligned_to(gt, 4);
    const bool quant = (flags & GSR_METRICS_QUANTIZE) != 0, ssim = !(flags & GSR_METRICS_NO_SSIM);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long ics = image_channel_stride, gcs = gt_channel_stride;
    if (vec && quant)
        launch_metrics<true, true>(ssim, grid, s, height, width, y0, y1, gxT, gyT, image, ics, gt, gcs, partials, out_u8);
    else if (vec)
        launch_metrics<true, false>(ssim, grid, s, height, width, y0, y1, gxT, gyT, image, ics, gt, gcs, partials, out_u8);
    else if (quant)
        launch_metrics<false, true>(ssim, grid, s, height, width, y0, y1, gxT, gyT, image, ics, gt, gcs, partials, out_u8);
    else
        launch_metrics<false, false>(ssim, grid, s, height, width, y0, y1, gxT, gyT, image, ics, gt, gcs, partials, out_u8);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_image_metrics_finalize(int channels, int num_partials, const float *partials, double *sums,
                                          gsr_stream_t stream) {
    if (channels <= 0 || num_partials <= 0 || num_partials % channels != 0 || !partials || !sums) return GSR_EINVAL;
    if (!aligned_to(partials, 4) || !aligned_to(sums, 8)) return GSR_EINVAL;
    hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3(channels), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       num_partials / channels, partials, sums);
    GSR_LAUNCH_CHECK();
    return 0;
}
