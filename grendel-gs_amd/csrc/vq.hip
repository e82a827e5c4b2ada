// vq.hip -- vector-quantised codebooks for the per-Gaussian parameter rows (the SH coefficients above DC are 45 of the 59
// values of a row): nearest-centroid assignment, the Lloyd update / per-cluster sums, and the decode.  The reference has
// no compression, so there is NO reference call site: plain float64 torch on the host is the arbiter
// (tests/test_gpu_vq_rows.py).  The method is the codebook of Compact3D / LightGaussian / "Compressed 3D Gaussian
// Splatting": k-means over the rows, a 16-bit index per row, the codebook trained on the summed gradients of its rows.
//
// ASSIGNMENT (vq_assign_kernel) -- P x K x D multiply-adds, the one dense contraction of this library, on the matrix pipe
// in exact fp32 (v_mfma_f32_16x16x4_f32; no reduced-precision operand):  s(i, k) = |c_k|^2 - 2 x_i . c_k,  idx_i = the
// lowest k that attains min_k s(i, k).
//   * work split: a workgroup (4 waves) owns 256 rows, a wave 64 of them as four 16-row blocks.  Centroids sit on M, rows
//     on N:  D[m][n] += A[m][k] B[k][n]  with A = 16 centroids x 4 columns from LDS and B = 4 columns x 16 rows from
//     REGISTERS.  A lane's row operands (16-row block rb, its row n = lane & 15, the four columns of its k-slot
//     lane >> 4, every K-step) are loaded once, zero-filled past D and past P by predicate -- nothing is read past a row --
//     and live in 4 x 4 NG registers for the whole kernel (NG = the number of 16-column groups, ceil(D / 16)).
//   * the contraction index is permuted so that one ds_read_b128 feeds four K-steps: K-step 4 g + jj of k-slot q
//     contracts column 16 g + 4 q + jj.  A and B use the same map, so the product is the plain dot product summed in
//     another (fixed) order.  Every A fragment read from LDS is used by four MFMAs (the four row blocks).
//   * the codebook streams through LDS in tiles of 64 centroids, double-buffered: the next tile's global loads are issued
//     before the current tile's MFMAs and stored after them.  Row stride 16 NG + 4 floats: 16-byte aligned, and
//     stride / 4 is odd, so the sixteen b128 reads of one k-slot fall on sixteen different 4-bank groups (conflict-free);
//     the four pad columns and the columns past D are zeroed once and never written again.  |c_k|^2 is computed once per
//     tile entry (four lanes per centroid) into a 64-float table; tail centroids are zero rows with |c|^2 = +inf and
//     are never read from global memory.
//   * a lane owns the accumulator elements (centroid 4 (lane >> 4) + r of every 16-centroid block, row lane & 15): it
//     meets its centroids in increasing k and keeps (best score, best index) per row block under a strict <, so a tie
//     keeps the lowest index; ONE lexicographic (score, index) reduction over the four k-slots (two xor-shuffles) ends the
//     kernel.  A NaN never passes <, and the index starts at 0: the result is in [0, K) for any input.
// dist2 (optional) is recomputed directly as the plain fp32 sum of squared differences to the chosen centroid.
//
// SEGMENT SUMS (update / gradient of the decode) -- no floating-point atomics, the same bits every run, fp64 accumulation
// rounded once, cost bounded under skew:
//   1. keys = idx (out of range -> the sentinel K), values = row id; the stable one-sweep radix sort of radix.h;
//   2. vq_chunk_kernel: a wave per 128 consecutive sorted entries, one lane per column; runs of equal keys are summed in
//      order in fp64.  A run strictly inside the chunk is a whole cluster and is finished there; the run that touches the
//      chunk's start (head) or its end (tail) goes to a partial slot;
//   3. vq_finalize_kernel: a wave per cluster finds its range by binary search in the sorted keys and adds the partials of
//      its chunks in chunk order.
// A cluster holding most rows is spread over P / 128 waves in step 2 and costs one add per chunk in step 3.
#include "common.h"

#include "radix.h"

namespace {

constexpr int VQ_MAX_K = 65536, VQ_MAX_D = 64;
constexpr int VQ_THREADS = 256;
constexpr int VQ_RB = 4;                                        // 16-row blocks per wave
constexpr int VQ_ROWS = (VQ_THREADS / 64) * VQ_RB * 16;         // rows per workgroup
constexpr int VQ_TILE = 64;                                     // centroids per LDS tile
constexpr int VQ_CHUNK = 128;                                   // sorted entries per wave of the segment reduction
constexpr int VQ_PSTRIDE = 66;                                  // a partial: 64 column sums, sum of weights, count

typedef float vq_f32x4 __attribute__((ext_vector_type(4)));

template <int NG>
__global__ void __launch_bounds__(VQ_THREADS)
vq_assign_kernel(int P, int K, int D, const float *__restrict__ rows, const float *__restrict__ cb,
                 int32_t *__restrict__ idx) {
    constexpr int STRIDE = 16 * NG + 4;
    constexpr int NPRE = 4 * NG;  // VQ_TILE * 16 NG floats over VQ_THREADS threads
    __shared__ __attribute__((aligned(16))) float stile[2][VQ_TILE * STRIDE];
    __shared__ __attribute__((aligned(16))) float snorm[2][VQ_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, kq = lane >> 4;
    const float inv_d = 1.0f / (float)D;

    for (int e = tid; e < 2 * VQ_TILE * STRIDE; e += VQ_THREADS) (&stile[0][0])[e] = 0.f;

    // B operands: row n16 of block rb, columns 16 g + 4 kq + jj
    const long long row0 = (long long)blockIdx.x * VQ_ROWS + wave * (VQ_RB * 16) + n16;
    float X[VQ_RB][4 * NG];
#pragma unroll
    for (int rb = 0; rb < VQ_RB; rb++) {
        const long long row = row0 + rb * 16;
        const bool live = row < P;
        const float *xr = rows + (size_t)(live ? row : 0) * D;
#pragma unroll
        for (int g = 0; g < NG; g++)
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int d = 16 * g + 4 * kq + jj;
                X[rb][4 * g + jj] = (live && d < D) ? xr[d] : 0.f;
            }
    }

    // a tile is min(VQ_TILE, K - k0) * D consecutive floats of the codebook; element e goes to row e / D, column e % D
    auto fetch = [&](int k0, float (&v)[NPRE]) {
        const int n = min(VQ_TILE, K - k0) * D;
        const float *src = cb + (size_t)k0 * D;
#pragma unroll
        for (int r = 0; r < NPRE; r++) {
            const int e = tid + r * VQ_THREADS;
            v[r] = e < n ? src[e] : 0.f;
        }
    };
    auto stash = [&](int buf, const float (&v)[NPRE]) {
#pragma unroll
        for (int r = 0; r < NPRE; r++) {
            const int e = tid + r * VQ_THREADS;
            if (e < VQ_TILE * D) {
                const int c = (int)(((float)e + 0.5f) * inv_d);  // e / D: e < 4096, (e + 0.5) / D is >= 1/128 off an integer
                stile[buf][c * STRIDE + (e - c * D)] = v[r];
            }
        }
    };
    auto norms = [&](int buf, int k0) {
        const int c = tid >> 2, q = tid & 3;
        float s = 0.f;
        for (int d = q; d < D; d += 4) {
            const float v = stile[buf][c * STRIDE + d];
            s = fmaf(v, v, s);
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (q == 0) snorm[buf][c] = (k0 + c < K) ? s : __builtin_inff();
    };

    float pre[NPRE];
    fetch(0, pre);
    __syncthreads();
    stash(0, pre);
    __syncthreads();
    norms(0, 0);
    __syncthreads();

    float bs[VQ_RB];
    int bi[VQ_RB];
#pragma unroll
    for (int rb = 0; rb < VQ_RB; rb++) {
        bs[rb] = __builtin_inff();
        bi[rb] = 0;
    }
    const int ntiles = (K + VQ_TILE - 1) / VQ_TILE;
    for (int t = 0; t < ntiles; t++) {
        const int buf = t & 1, k0 = t * VQ_TILE;
        const bool more = t + 1 < ntiles;
        if (more) fetch(k0 + VQ_TILE, pre);
        const float *tile = stile[buf];
#pragma unroll 1
        for (int mb = 0; mb < VQ_TILE / 16; mb++) {
            vq_f32x4 acc[VQ_RB];
#pragma unroll
            for (int rb = 0; rb < VQ_RB; rb++) acc[rb] = vq_f32x4{0.f, 0.f, 0.f, 0.f};
            const float *arow = tile + (mb * 16 + n16) * STRIDE + 4 * kq;  // A: centroid mb * 16 + (lane & 15)
#pragma unroll
            for (int g = 0; g < NG; g++) {
                const vq_f32x4 a = *reinterpret_cast<const vq_f32x4 *>(arow + 16 * g);
#pragma unroll
                for (int jj = 0; jj < 4; jj++)
#pragma unroll
                    for (int rb = 0; rb < VQ_RB; rb++)
                        acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[jj], X[rb][4 * g + jj], acc[rb], 0, 0, 0);
            }
            // C: centroid mb * 16 + 4 kq + r in register r, row lane & 15
            const vq_f32x4 nn = *reinterpret_cast<const vq_f32x4 *>(&snorm[buf][mb * 16 + 4 * kq]);
            const int kbase = k0 + mb * 16 + 4 * kq;
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int rb = 0; rb < VQ_RB; rb++) {
                    const float s = fmaf(-2.0f, acc[rb][r], nn[r]);
                    if (s < bs[rb]) {
                        bs[rb] = s;
                        bi[rb] = kbase + r;
                    }
                }
        }
        if (more) stash(buf ^ 1, pre);  // the other buffer was last read before the barriers that ended tile t - 1
        __syncthreads();
        if (more) norms(buf ^ 1, k0 + VQ_TILE);
        __syncthreads();
    }

#pragma unroll
    for (int rb = 0; rb < VQ_RB; rb++) {
        float s = bs[rb];
        int i = bi[rb];
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float os = __shfl_xor(s, off, 64);
            const int oi = __shfl_xor(i, off, 64);
            if (os < s || (os == s && oi < i)) {
                s = os;
                i = oi;
            }
        }
        const long long row = row0 + rb * 16;
        if (kq == 0 && row < P) idx[row] = i;
    }
}

__global__ void __launch_bounds__(VQ_THREADS)
vq_dist2_kernel(int P, int D, const float *__restrict__ rows, const float *__restrict__ cb,
                const int32_t *__restrict__ idx, float *__restrict__ dist2) {
    const long long i = (long long)blockIdx.x * VQ_THREADS + threadIdx.x;
    if (i >= P) return;
    const float *x = rows + (size_t)i * D, *c = cb + (size_t)idx[i] * D;
    float s = 0.f;
    for (int d = 0; d < D; d++) {
        const float t = x[d] - c[d];
        s = fmaf(t, t, s);
    }
    dist2[i] = s;
}

__global__ void __launch_bounds__(VQ_THREADS)
vq_decode_kernel(long long n, int K, int D, const float *__restrict__ cb, const int32_t *__restrict__ idx,
                 float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * VQ_THREADS + threadIdx.x;
    if (e >= n) return;
    const long long i = e / D;
    const int d = (int)(e - i * D);
    const int k = idx[i];
    out[e] = (k >= 0 && k < K) ? cb[(size_t)k * D + d] : 0.f;
}

// sort keys: the cluster, or the sentinel K for an index outside [0, K); the digit histograms of every pass on the way
__global__ void __launch_bounds__(RADIX_THREADS)
vq_keys_kernel(int P, int K, const int32_t *__restrict__ idx, RadixPlan plan, uint32_t *__restrict__ keys,
               uint32_t *__restrict__ vals, uint32_t *__restrict__ ghist) {
    __shared__ uint32_t mh[RADIX_MAX_PASSES][RADIX_DIGITS];
    for (int p = 0; p < RADIX_MAX_PASSES; p++) mh[p][threadIdx.x] = 0;
    __syncthreads();
    for (long long base = (long long)blockIdx.x * blockDim.x; base < P; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const bool valid = i < P;
        uint32_t key = 0;
        if (valid) {
            const int k = idx[i];
            key = (k >= 0 && k < K) ? (uint32_t)k : (uint32_t)K;
            keys[i] = key;
            vals[i] = (uint32_t)i;
        }
        multihist_add(mh, plan, key, valid);
    }
    __syncthreads();
    multihist_flush(mh, plan, ghist);
}

// the result of cluster k from its fp64 sums (lane = column).  UPDATE: the weighted mean, count and sum of weights; a
// cluster whose weights do not sum to a positive number keeps its centroid.  Otherwise the plain sum.
template <bool UPDATE>
__device__ __forceinline__ void vq_write_cluster(int k, int D, int lane, double acc, double wacc, double cnt,
                                                 float *__restrict__ out, int32_t *__restrict__ count,
                                                 float *__restrict__ wsum) {
    if (UPDATE) {
        if (lane < D && wacc > 0.0) out[(size_t)k * D + lane] = (float)(acc / wacc);
        if (lane == 0) {
            count[k] = (int32_t)cnt;
            wsum[k] = (float)wacc;
        }
    } else if (lane < D) {
        out[(size_t)k * D + lane] = (float)acc;
    }
}

template <bool UPDATE>
__global__ void __launch_bounds__(VQ_THREADS)
vq_chunk_kernel(int P, int K, int D, const float *__restrict__ rows, const float *__restrict__ w,
                const uint32_t *__restrict__ ks, const uint32_t *__restrict__ vs, double *__restrict__ part,
                float *__restrict__ out, int32_t *__restrict__ count, float *__restrict__ wsum) {
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * (VQ_THREADS / 64) + (threadIdx.x >> 6);
    const long long cbeg = c * VQ_CHUNK;
    if (cbeg >= P) return;  // (the kernel has no barrier)
    const int n = (int)min((long long)VQ_CHUNK, (long long)P - cbeg);
    // entry h * 64 + lane of the chunk; past the end: the largest key, which ends the walk like the sentinel does
    uint32_t kreg[VQ_CHUNK / 64], vreg[VQ_CHUNK / 64];
    float wreg[VQ_CHUNK / 64];
#pragma unroll
    for (int h = 0; h < VQ_CHUNK / 64; h++) {
        const int e = h * 64 + lane;
        kreg[h] = e < n ? ks[cbeg + e] : 0xFFFFFFFFu;
        vreg[h] = e < n ? vs[cbeg + e] : 0u;
        wreg[h] = (UPDATE && w && kreg[h] < (uint32_t)K) ? w[vreg[h]] : 1.0f;
    }
    uint32_t cur = __shfl(kreg[0], 0, 64);
    if (cur >= (uint32_t)K) return;  // sorted: nothing but skipped rows from here on
    double acc = 0.0, wacc = 0.0, cnt = 0.0;
    int rs = 0;
    // the run [rs, re) of cluster `cur` is complete: a partial when it touches an end of the chunk, else the cluster
    auto flush = [&](int re) {
        if (rs == 0 || re == n) {
            double *p = part + (size_t)(2 * c + (rs == 0 ? 0 : 1)) * VQ_PSTRIDE;
            p[lane] = acc;
            if (lane == 0) {
                p[64] = wacc;
                p[65] = cnt;
            }
        } else {
            vq_write_cluster<UPDATE>((int)cur, D, lane, acc, wacc, cnt, out, count, wsum);
        }
    };
    bool open = true;
    for (int e0 = 0; e0 < VQ_CHUNK && open; e0 += 8) {
        uint32_t key[8];
        float wv[8], x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {  // the eight row loads are in flight together
            const int h = (e0 + u) >> 6, l = (e0 + u) & 63;
            key[u] = __shfl(h ? kreg[1] : kreg[0], l, 64);
            const uint32_t rid = __shfl(h ? vreg[1] : vreg[0], l, 64);
            wv[u] = __shfl(h ? wreg[1] : wreg[0], l, 64);
            x[u] = (key[u] < (uint32_t)K && lane < D) ? rows[(size_t)rid * D + lane] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (!open) break;
            if (key[u] >= (uint32_t)K) {  // the sentinel, or the end of a short chunk (e0 + u == n)
                flush(e0 + u);
                open = false;
                break;
            }
            if (key[u] != cur) {
                flush(e0 + u);
                cur = key[u];
                rs = e0 + u;
                acc = wacc = cnt = 0.0;
            }
            acc += (double)wv[u] * (double)x[u];  // exact product
            wacc += (double)wv[u];
            cnt += 1.0;
        }
    }
    if (open) flush(n);  // n == VQ_CHUNK and the last entry belongs to a cluster
}
static_assert(VQ_CHUNK == 128, "vq_chunk_kernel selects between two entry registers");

template <bool UPDATE>
__global__ void __launch_bounds__(VQ_THREADS)
vq_finalize_kernel(int P, int K, int D, const uint32_t *__restrict__ ks, const double *__restrict__ part,
                   float *__restrict__ out, int32_t *__restrict__ count, float *__restrict__ wsum) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (VQ_THREADS / 64) + (threadIdx.x >> 6);
    if (k >= K) return;
    auto lower_bound = [&](uint32_t key) {
        int lo = 0, hi = P;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (ks[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const int s = lower_bound((uint32_t)k), e = lower_bound((uint32_t)k + 1u);
    if (s == e) {  // no rows: the centroid stays (update), the sum is zero
        vq_write_cluster<UPDATE>(k, D, lane, 0.0, 0.0, 0.0, out, count, wsum);
        return;
    }
    const int c0 = s / VQ_CHUNK, c1 = (e - 1) / VQ_CHUNK;
    const long long c0beg = (long long)c0 * VQ_CHUNK, c0end = min((long long)P, c0beg + VQ_CHUNK);
    if (s > c0beg && e < c0end) return;  // strictly inside one chunk: vq_chunk_kernel finished it
    double acc = 0.0, wacc = 0.0, cnt = 0.0;
#pragma unroll 8
    for (int c = c0; c <= c1; c++) {
        const double *p = part + (size_t)(2 * (long long)c + ((c == c0 && s > c0beg) ? 1 : 0)) * VQ_PSTRIDE;
        acc += p[lane];
        wacc += p[64];
        cnt += p[65];
    }
    vq_write_cluster<UPDATE>(k, D, lane, acc, wacc, cnt, out, count, wsum);
}

struct VqLayout {
    size_t ctrl, kA, vA, kB, vB, part, total;
    CtrlLayout C;
};
VqLayout vq_layout(int P) {
    VqLayout L;
    size_t o = 0;
    L.ctrl = o;
    L.C = ctrl_layout(P, 3, false);  // keys of at most 17 bits: three passes
    o += L.C.total;
    const size_t np = align_up((size_t)(P + 1) * 4);
    L.kA = o; o += np;
    L.vA = o; o += np;
    L.kB = o; o += np;
    L.vB = o; o += np;
    L.part = o; o += align_up((size_t)(gsr_div_up(P, VQ_CHUNK) + 1) * 2 * VQ_PSTRIDE * sizeof(double));
    L.total = o;
    return L;
}

bool vq_shape_ok(int P, int K, int D) { return P >= 0 && K >= 1 && K <= VQ_MAX_K && D >= 1 && D <= VQ_MAX_D; }

template <bool UPDATE>
int vq_segment_reduce(int P, int K, int D, const float *rows, const int32_t *idx, const float *w, float *out,
                      int32_t *count, float *wsum, void *workspace, size_t workspace_bytes, hipStream_t stream) {
    const VqLayout L = vq_layout(P);
    if (workspace_bytes < L.total) return GSR_ENOSPACE;
    char *base = reinterpret_cast<char *>(workspace);
    char *ctrl = base + L.ctrl;
    uint32_t *kA = reinterpret_cast<uint32_t *>(base + L.kA), *vA = reinterpret_cast<uint32_t *>(base + L.vA);
    uint32_t *kB = reinterpret_cast<uint32_t *>(base + L.kB), *vB = reinterpret_cast<uint32_t *>(base + L.vB);
    double *part = reinterpret_cast<double *>(base + L.part);
    GSR_HIP(hipMemsetAsync(ctrl, 0, L.C.total, stream));
    int bits = 1;
    while ((K >> bits) != 0) bits++;  // the sentinel K is the largest key
    const RadixPlan plan = radix_plan(0, bits);
    const int grid = gsr_div_up(P, RADIX_THREADS) < 512 ? gsr_div_up(P, RADIX_THREADS) : 512;
    hipLaunchKernelGGL(vq_keys_kernel, dim3(grid), dim3(RADIX_THREADS), 0, stream, P, K, idx, plan, kA, vA,
                       reinterpret_cast<uint32_t *>(ctrl + L.C.ghist));
    int in_first = 1;
    const int rc = radix_sort_pairs(kA, vA, kB, vB, P, plan, ctrl, L.C, &in_first, stream, nullptr);
    if (rc) return rc;
    const uint32_t *ks = in_first ? kA : kB, *vs = in_first ? vA : vB;
    constexpr int WAVES = VQ_THREADS / 64;
    hipLaunchKernelGGL(vq_chunk_kernel<UPDATE>, dim3(gsr_div_up(gsr_div_up(P, VQ_CHUNK), WAVES)), dim3(VQ_THREADS), 0,
                       stream, P, K, D, rows, w, ks, vs, part, out, count, wsum);
    hipLaunchKernelGGL(vq_finalize_kernel<UPDATE>, dim3(gsr_div_up(K, WAVES)), dim3(VQ_THREADS), 0, stream, P, K, D, ks,
                       part, out, count, wsum);
    GSR_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" size_t gsr_vq_workspace_bytes(int P, int K, int D) {
    if (!vq_shape_ok(P, K, D)) return 0;
    return vq_layout(P).total;
}

extern "C" int gsr_vq_assign(int P, int K, int D, const float *rows, const float *codebook, int32_t *idx, float *dist2,
                             gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!vq_shape_ok(P, K, D)) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!rows || !codebook || !idx) return GSR_EINVAL;
    const dim3 grid(gsr_div_up(P, VQ_ROWS)), block(VQ_THREADS);
    switch ((D + 15) / 16) {
        case 1: hipLaunchKernelGGL(vq_assign_kernel<1>, grid, block, 0, stream, P, K, D, rows, codebook, idx); break;
        case 2: hipLaunchKernelGGL(vq_assign_kernel<2>, grid, block, 0, stream, P, K, D, rows, codebook, idx); break;
        case 3: hipLaunchKernelGGL(vq_assign_kernel<3>, grid, block, 0, stream, P, K, D, rows, codebook, idx); break;
        default: hipLaunchKernelGGL(vq_assign_kernel<4>, grid, block, 0, stream, P, K, D, rows, codebook, idx); break;
    }
    if (dist2)
        hipLaunchKernelGGL(vq_dist2_kernel, dim3(gsr_div_up(P, VQ_THREADS)), block, 0, stream, P, D, rows, codebook, idx,
                           dist2);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_vq_update(int P, int K, int D, const float *rows, const int32_t *idx, const float *weights,
                             float *codebook, int32_t *count, float *wsum, void *workspace, size_t workspace_bytes,
                             gsr_stream_t stream_) {
    if (!vq_shape_ok(P, K, D)) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!rows || !idx || !codebook || !count || !wsum || !workspace) return GSR_EINVAL;
    return vq_segment_reduce<true>(P, K, D, rows, idx, weights, codebook, count, wsum, workspace, workspace_bytes,
                                   reinterpret_cast<hipStream_t>(stream_));
}

extern "C" int gsr_vq_segment_sum(int P, int K, int D, const float *rows, const int32_t *idx, float *sums,
                                  void *workspace, size_t workspace_bytes, gsr_stream_t stream_) {
    if (!vq_shape_ok(P, K, D)) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!rows || !idx || !sums || !workspace) return GSR_EINVAL;
    return vq_segment_reduce<false>(P, K, D, rows, idx, nullptr, sums, nullptr, nullptr, workspace, workspace_bytes,
                                    reinterpret_cast<hipStream_t>(stream_));
}

extern "C" int gsr_vq_decode(int P, int K, int D, const float *codebook, const int32_t *idx, float *out,
                             gsr_stream_t stream_) {
    if (!vq_shape_ok(P, K, D)) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!codebook || !idx || !out) return GSR_EINVAL;
    const long long n = (long long)P * D;
    hipLaunchKernelGGL(vq_decode_kernel, dim3(gsr_div_up(n, VQ_THREADS)), dim3(VQ_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream_), n, K, D, codebook, idx, out);
    GSR_LAUNCH_CHECK();
    return 0;
}
