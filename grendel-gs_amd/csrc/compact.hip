// compact.hip -- N4 row primitives behind densification / redistribution of the Gaussian shards.
//
// The reference prunes, clones, splits and redistributes Gaussians with boolean indexing on each of its ~23
// per-Gaussian tensors (6 parameters, 12 Adam moments, 5 statistics: scene/gaussian_model.py:775-921 prune /
// cat, 922-1007 split / clone, 1073-1098 one masked copy PER DESTINATION RANK per tensor).  Every
// `tensor[mask]` is a nonzero (host sync) plus an index kernel.  Here the row selection is computed ONCE:
//   gsr_group_rows : stable grouping of row indices by destination (one one-sweep radix pass, radix.h) ->
//                    order[] (rows of destination 0, then 1, ... then the dropped rows) and per-group counts;
//   gsr_gather_rows: one launch copies the selected rows of up to 32 tensors (any row width / strides), e.g.
//                    into compacted tensors (prune), into the columns of ONE record matrix that a single
//                    all-to-all-v redistributes (the reference's disabled "implementation_2",
//                    scene/gaussian_model.py:1206-1238), or back out of it.
// and, on top of the same idea, the whole densification event as two launches (bottom of this file):
//   gsr_densify_plan: one single-sweep scan over a class byte per row -> ranks in four categories + four counts;
//   gsr_densify_move: one launch writes every row of the clone / split / prune result for all tensors.
#include "common.h"

#include "radix.h"

// no FMA contraction in this file: a split child's position is evaluated with the roundings of the reference's elementwise
// torch expressions (child_rotation_row below); the only fused operation left is the explicit fmaf of densify_stats_kernel
#pragma clang fp contract(off)

namespace {

constexpr int GROUP_THREADS = 256;
constexpr int GATHER_MAX_TENSORS = 32;

__global__ void __launch_bounds__(GROUP_THREADS)
group_keys_kernel(int N, int G, const int32_t *__restrict__ dest, RadixPlan plan, uint32_t *__restrict__ keys,
                  uint32_t *__restrict__ vals, uint32_t *__restrict__ ghist) {
    __shared__ uint32_t mh[RADIX_MAX_PASSES][RADIX_DIGITS];
    for (int p = 0; p < RADIX_MAX_PASSES; p++) mh[p][threadIdx.x] = 0;
    __syncthreads();
    for (long long base = (long long)blockIdx.x * blockDim.x; base < N; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const bool valid = i < N;
        uint32_t key = 0;
        if (valid) {
            const int32_t d = dest[i];
            key = (d >= 0 && d < G) ? (uint32_t)d : (uint32_t)G;  // anything else: dropped, sorts last
            keys[i] = key;
            vals[i] = (uint32_t)i;
        }
        multihist_add(mh, plan, key, valid);
    }
    __syncthreads();
    multihist_flush(mh, plan, ghist);
}

__global__ void group_counts_kernel(int G, const uint32_t *__restrict__ ghist, int64_t *__restrict__ counts) {
    const int d = threadIdx.x;
    if (d > G) return;
    uint32_t c = 0;
    for (int x = 0; x < RADIX_REPLICAS; x++) c += ghist[(size_t)x * RADIX_MAX_PASSES * RADIX_DIGITS + d];
    counts[d] = (int64_t)c;
}

struct GatherArgs {
    const uint32_t *src[GATHER_MAX_TENSORS];
    uint32_t *dst[GATHER_MAX_TENSORS];
    int32_t width[GATHER_MAX_TENSORS];  // 4-byte words per row
    int64_t src_stride[GATHER_MAX_TENSORS], dst_stride[GATHER_MAX_TENSORS];  // in words
};

// blockIdx.y = tensor; one thread per 4-byte word of the selected rows.  SCATTER: dst[order[r]] = src[r] instead of
// dst[r] = src[order[r]] (the inverse of a gather with the same order: N2 writes the reduced compact rows back)
template <bool SCATTER>
__global__ void __launch_bounds__(256)
gather_rows_kernel(long long n_out, const int32_t *__restrict__ order, GatherArgs a) {
    const int k = blockIdx.y;
    const int w = a.width[k];
    const long long total = n_out * w;
    const uint32_t *__restrict__ src = a.src[k];
    uint32_t *__restrict__ dst = a.dst[k];
    const int64_t ss = a.src_stride[k], ds = a.dst_stride[k];
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const long long r = e / w;
        const int c = (int)(e - r * w);
        const long long sr = order ? (long long)order[r] : r;
        if (SCATTER) dst[sr * ds + c] = src[r * ss + c];
        else dst[r * ds + c] = src[sr * ss + c];
    }
}

struct GroupLayout {
    size_t ctrl, kA, vA, kB, total;
    CtrlLayout C;
};
GroupLayout group_layout(long long N) {
    GroupLayout L;
    size_t o = 0;
    L.ctrl = o;
    L.C = ctrl_layout(N, 1, false);
    o += L.C.total;
    const size_t np = align_up((size_t)(N + 1) * 4);
    L.kA = o; o += np;
    L.vA = o; o += np;
    L.kB = o; o += np;
    L.total = o;
    return L;
}
}  // namespace

// The per-iteration densification statistics (densification.py:13-25 of the reference, after every backward of the
// densification phase -- half of a 30 000-iteration run): for the Gaussians visible in the view (radius > 0)
//   max_radii2D = max(max_radii2D, radius);  xyz_gradient_accum += |d loss / d means2D|;  denom += 1
// as ONE launch over the P rows instead of the reference's boolean indexing (two `nonzero` host syncs, six gather / scatter
// kernels).  `grad`: the means2D gradient, rows `grad_stride` floats apart (2 for a dense [P,2]; 9 for the view of K10's
// [P,9] record the operator hands out).  An invisible Gaussian's gradient row is exactly 0 (K10 never touches it), so the
// accumulators of invisible rows keep their bits whether or not the row is skipped; it IS skipped (radius 0).
__global__ void __launch_bounds__(256)
densify_stats_kernel(long long P, const int32_t *__restrict__ radii, const float *__restrict__ grad,
                     long long grad_stride, float *__restrict__ max_radii2D, float *__restrict__ accum,
                     float *__restrict__ denom) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int32_t r = radii[i];
    if (r <= 0) return;
    const float gx = grad[i * grad_stride], gy = grad[i * grad_stride + 1];
    max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
    accum[i] += sqrtf(__builtin_fmaf(gy, gy, __fmul_rn(gx, gx)));
    denom[i] += 1.0f;
}

extern "C" int gsr_densify_stats(int64_t P, const int32_t *radii, const float *grad, int64_t grad_stride,
                                 float *max_radii2D, float *accum, float *denom, gsr_stream_t stream) {
    if (P < 0 || grad_stride < 2) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!radii || !grad || !max_radii2D || !accum || !denom) return GSR_EINVAL;
    hipLaunchKernelGGL(densify_stats_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), (long long)P, radii, grad, (long long)grad_stride,
                       max_radii2D, accum, denom);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t gsr_group_rows_bytes(int64_t N) {
    if (N < 0) return 0;
    return group_layout(N).total;
}

extern "C" int gsr_group_rows(int64_t N, int G, const int32_t *dest, int32_t *order, int64_t *counts, void *workspace,
                              size_t workspace_bytes, gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (N < 0 || G < 1 || G > 255 || !counts) return GSR_EINVAL;
    GSR_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)(G + 1), stream));
    if (N == 0) return 0;
    if (!dest || !order || !workspace) return GSR_EINVAL;
    if (N > RADIX_MAX_N) return GSR_EINVAL;
    const GroupLayout L = group_layout(N);
    if (workspace_bytes < L.total) return GSR_ENOSPACE;
    char *base = reinterpret_cast<char *>(workspace);
    char *ctrl = base + L.ctrl;
    uint32_t *kA = reinterpret_cast<uint32_t *>(base + L.kA), *vA = reinterpret_cast<uint32_t *>(base + L.vA);
    uint32_t *kB = reinterpret_cast<uint32_t *>(base + L.kB);
    GSR_HIP(hipMemsetAsync(ctrl, 0, L.C.total, stream));
    const RadixPlan plan = radix_plan(0, 8);
    const int grid = gsr_div_up(N, GROUP_THREADS) < 512 ? gsr_div_up(N, GROUP_THREADS) : 512;
    uint32_t *ghist = reinterpret_cast<uint32_t *>(ctrl + L.C.ghist);
    hipLaunchKernelGGL(group_keys_kernel, dim3(grid), dim3(GROUP_THREADS), 0, stream, (int)N, G, dest, plan, kA, vA,
                       ghist);
    hipLaunchKernelGGL(group_counts_kernel, dim3(1), dim3(256), 0, stream, G, ghist, counts);
    int in_first = 1;
    // single pass: the values (row indices) land directly in `order`; vB is never written
    int rc = radix_sort_pairs(kA, vA, kB, nullptr, N, plan, ctrl, L.C, &in_first, stream,
                              reinterpret_cast<uint32_t *>(order));
    if (rc) return rc;
    GSR_LAUNCH_CHECK();
    return 0;
}

namespace {
int launch_rows(bool scatter, int64_t n_out, const int32_t *order, int num_tensors, const void *const *srcs,
                void *const *dsts, const int32_t *widths, const int64_t *src_strides, const int64_t *dst_strides,
                hipStream_t stream) {
    if (n_out < 0 || num_tensors < 0 || num_tensors > GATHER_MAX_TENSORS) return GSR_EINVAL;
    if (n_out == 0 || num_tensors == 0) return 0;
    if (!srcs || !dsts || !widths || !src_strides || !dst_strides) return GSR_EINVAL;
    GatherArgs a{};
    long long widest = 0;
    for (int k = 0; k < num_tensors; k++) {
        if (!srcs[k] || !dsts[k] || widths[k] <= 0) return GSR_EINVAL;
        a.src[k] = reinterpret_cast<const uint32_t *>(srcs[k]);
        a.dst[k] = reinterpret_cast<uint32_t *>(dsts[k]);
        a.width[k] = widths[k];
        a.src_stride[k] = src_strides[k];
        a.dst_stride[k] = dst_strides[k];
        widest = widths[k] > widest ? widths[k] : widest;
    }
    long long blocks = (n_out * widest + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (scatter)
        hipLaunchKernelGGL(gather_rows_kernel<true>, dim3((unsigned)blocks, (unsigned)num_tensors), dim3(256), 0, stream,
                           (long long)n_out, order, a);
    else
        hipLaunchKernelGGL(gather_rows_kernel<false>, dim3((unsigned)blocks, (unsigned)num_tensors), dim3(256), 0,
                           stream, (long long)n_out, order, a);
    GSR_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int gsr_gather_rows(int64_t n_out, const int32_t *order, int num_tensors, const void *const *srcs,
                               void *const *dsts, const int32_t *widths, const int64_t *src_strides,
                               const int64_t *dst_strides, gsr_stream_t stream_) {
    return launch_rows(false, n_out, order, num_tensors, srcs, dsts, widths, src_strides, dst_strides,
                       reinterpret_cast<hipStream_t>(stream_));
}

extern "C" int gsr_scatter_rows(int64_t n_in, const int32_t *order, int num_tensors, const void *const *srcs,
                                void *const *dsts, const int32_t *widths, const int64_t *src_strides,
                                const int64_t *dst_strides, gsr_stream_t stream_) {
    if (n_in > 0 && !order) return GSR_EINVAL;
    return launch_rows(true, n_in, order, num_tensors, srcs, dsts, widths, src_strides, dst_strides,
                       reinterpret_cast<hipStream_t>(stream_));
}

// ------------------------------------------------------------------------------------------------------------------
// One-pass densification event.  The reference's clone -> split -> prune sequence (scene/gaussian_model.py:789-921 the
// row surgery, :922-1044 densify_and_split / densify_and_clone / densify_and_prune) has a closed-form result in terms of
// the ORIGINAL rows: [kept originals | kept clones | first children | second children], original order inside each
// segment (DESIGN.md "One-pass densification").  The host classifies every row into a byte; the plan ranks the rows of
// the four categories in one sweep and the move writes every destination row of every tensor from the plan.
namespace {

constexpr int PLAN_THREADS = 256, PLAN_ITEMS = 8, PLAN_TILE = PLAN_THREADS * PLAN_ITEMS, PLAN_WAVES = PLAN_THREADS / 64;
constexpr int PLAN_CATS = 4;
// category order of ranks[] and counts[] (the class bit each one tests): kept original, kept clone, parent whose
// children are kept, split parent
__host__ __device__ constexpr uint32_t plan_bit(int c) {
    return c == 0 ? GSR_DENSIFY_KEEP_ORIGINAL : c == 1 ? GSR_DENSIFY_KEEP_CLONE
         : c == 2 ? GSR_DENSIFY_KEEP_CHILDREN : GSR_DENSIFY_SPLIT_PARENT;
}

struct PlanLayout {
    size_t ticket, state, total;
    long long tiles;
};
PlanLayout plan_layout(long long P) {
    PlanLayout L;
    L.tiles = (P + PLAN_TILE - 1) / PLAN_TILE;
    L.ticket = 0;
    L.state = 256;
    L.total = L.state + (((size_t)(L.tiles > 0 ? L.tiles : 1) * PLAN_CATS * sizeof(uint32_t) + 255) & ~(size_t)255);
    return L;
}

// Single-sweep scan, decoupled look-back on the state words of radix.h (0 = nothing yet, bit 31 = inclusive prefix,
// otherwise aggregate + 1; an aggregate is at most PLAN_TILE).  Tiles are taken by ticket, so every tile a workgroup
// looks back at is held by a workgroup that already runs.  Wave w owns PLAN_ITEMS consecutive rounds of 64 rows; the rank
// of a row inside its wave's chunk is (rows of the earlier rounds) + popcount(ballot below the lane), one ballot per
// category.
__global__ void __launch_bounds__(PLAN_THREADS)
densify_plan_kernel(long long P, const uint8_t *__restrict__ cls, int32_t *__restrict__ ranks,
                    int32_t *__restrict__ split_rows, int64_t *__restrict__ counts, uint32_t *__restrict__ ticket,
                    uint32_t *__restrict__ state, uint32_t tiles) {
    __shared__ uint32_t s_bid;
    __shared__ uint32_t s_wave[PLAN_WAVES][PLAN_CATS];  // totals, then exclusive offsets of the waves inside the tile
    __shared__ uint32_t s_base[PLAN_CATS];
    if (threadIdx.x == 0) s_bid = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t bid = s_bid;
    if (bid >= tiles) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const long long wbase = (long long)bid * PLAN_TILE + (long long)wave * (PLAN_ITEMS * 64);
    uint8_t code[PLAN_ITEMS];
    uint16_t local[PLAN_ITEMS][PLAN_CATS];
    uint32_t run[PLAN_CATS] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < PLAN_ITEMS; r++) {
        const long long j = wbase + r * 64 + lane;
        code[r] = j < P ? cls[j] : (uint8_t)0;
#pragma unroll
        for (int c = 0; c < PLAN_CATS; c++) {
            const unsigned long long m = __ballot((code[r] & plan_bit(c)) != 0);
            local[r][c] = (uint16_t)(run[c] + (uint32_t)__popcll(m & lt));
            run[c] += (uint32_t)__popcll(m);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < PLAN_CATS; c++) s_wave[wave][c] = run[c];
    }
    __syncthreads();
    if (threadIdx.x < PLAN_CATS) {
        const int c = threadIdx.x;
        uint32_t tot = 0;
        for (int w = 0; w < PLAN_WAVES; w++) {
            const uint32_t v = s_wave[w][c];
            s_wave[w][c] = tot;
            tot += v;
        }
        st_agent(&state[(size_t)bid * PLAN_CATS + c], bid == 0 ? (tot | LB_PRE) : (tot + 1u));
        uint32_t excl = 0;
        if (bid > 0) {
            long long j = (long long)bid - 1;
            for (;;) {
                uint32_t x = ld_agent(&state[(size_t)j * PLAN_CATS + c]);
                while (x == 0u) {
                    __builtin_amdgcn_s_sleep(1);
                    x = ld_agent(&state[(size_t)j * PLAN_CATS + c]);
                }
                if (x & LB_PRE) {
                    excl += x & LB_VAL;
                    break;
                }
                excl += x - 1u;
                j--;
            }
            st_agent(&state[(size_t)bid * PLAN_CATS + c], ((excl + tot) & LB_VAL) | LB_PRE);
        }
        s_base[c] = excl;
        if (bid == tiles - 1) counts[c] = (int64_t)(excl + tot);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PLAN_ITEMS; r++) {
        const long long j = wbase + r * 64 + lane;
        if (j < P) {
#pragma unroll
            for (int c = 0; c < PLAN_CATS; c++) {
                const uint32_t rk = s_base[c] + s_wave[wave][c] + local[r][c];
                ranks[(size_t)c * P + j] = (int32_t)rk;
                if (c == 3 && split_rows && (code[r] & GSR_DENSIFY_SPLIT_PARENT)) split_rows[rk] = (int32_t)j;
            }
        }
    }
}

constexpr int MOVE_THREADS = 256, MOVE_ROWS = 256;  // rows per workgroup and round
constexpr int MOVE_UNROLL = 4;                      // words a thread has in flight
constexpr int MOVE_MAX_WIDTH = 1 << 20;             // MOVE_ROWS * width stays far inside 32 bits

struct MoveArgs {
    const uint32_t *src[GATHER_MAX_TENSORS];
    const uint32_t *alt[GATHER_MAX_TENSORS];
    uint32_t *dst[GATHER_MAX_TENSORS];
    int32_t width[GATHER_MAX_TENSORS], role[GATHER_MAX_TENSORS];
    int64_t src_stride[GATHER_MAX_TENSORS], dst_stride[GATHER_MAX_TENSORS];  // in words
};

// row `c` of R(q) exactly as the reference's build_rotation (utils/general_utils.py:416-439) evaluates it elementwise:
// the norm with a correctly rounded sqrtf, true divisions, every product and sum rounded on its own (contraction is off
// in this file, no fast-math)
__device__ __forceinline__ void child_rotation_row(int c, const float *__restrict__ q4, float &r0, float &r1, float &r2) {
    const float a = q4[0], b = q4[1], cc = q4[2], d = q4[3];
    const float norm = sqrtf(a * a + b * b + cc * cc + d * d);
    const float w = a / norm, x = b / norm, y = cc / norm, z = d / norm;
    if (c == 0) {
        r0 = 1.0f - 2.0f * (y * y + z * z);
        r1 = 2.0f * (x * y - w * z);
        r2 = 2.0f * (x * z + w * y);
    } else if (c == 1) {
        r0 = 2.0f * (x * y + w * z);
        r1 = 1.0f - 2.0f * (x * x + z * z);
        r2 = 2.0f * (y * z - w * x);
    } else {
        r0 = 2.0f * (x * z - w * y);
        r1 = 2.0f * (y * z + w * x);
        r2 = 1.0f - 2.0f * (x * x + y * y);
    }
}

// A workgroup takes MOVE_ROWS consecutive SOURCE rows per round: one thread per row turns class + ranks into the
// destination rows (LDS), then for every tensor one thread per 4-byte word of those rows reads the word once and writes
// it wherever the row goes.  Consecutive threads hold consecutive words of consecutive rows, and the kept rows of a
// segment land on consecutive destination rows, so reads are coalesced and writes are coalesced runs.
__global__ void __launch_bounds__(MOVE_THREADS)
densify_move_kernel(long long P, const uint8_t *__restrict__ cls, const int32_t *__restrict__ ranks, long long n_orig,
                    long long n_clone, long long n_child, long long n_split, int copies, int num_tensors,
                    const float *__restrict__ rotation, const float *__restrict__ samples, MoveArgs a) {
    __shared__ long long s_orig[MOVE_ROWS], s_clone[MOVE_ROWS], s_child[MOVE_ROWS];
    __shared__ int32_t s_sample[MOVE_ROWS];
    __shared__ uint8_t s_kind[MOVE_ROWS];  // bit 0: the original stays, bit 1: a clone, bit 2: children; 0: dropped
    const long long child0 = n_orig + n_clone;
    const long long rounds = (P + MOVE_ROWS - 1) / MOVE_ROWS;
    for (long long rd = blockIdx.x; rd < rounds; rd += gridDim.x) {
        const long long base = rd * MOVE_ROWS;
        const int nrows = (int)(P - base < MOVE_ROWS ? P - base : MOVE_ROWS);
        if ((int)threadIdx.x < nrows) {
            const long long i = base + threadIdx.x;
            const uint8_t code = cls[i];
            long long o = -1, c = -1, ch = -1;
            int32_t sj = 0;
            // (a destination outside the result -- class bytes that do not belong to this plan -- is dropped, never written)
            if (code & GSR_DENSIFY_KEEP_ORIGINAL) {
                o = ranks[i];
                if (o >= n_orig) o = -1;
            }
            if (code & GSR_DENSIFY_KEEP_CLONE) {
                c = n_orig + ranks[(size_t)P + i];
                if (c >= child0) c = -1;
            }
            if ((code & GSR_DENSIFY_KEEP_CHILDREN) && (code & GSR_DENSIFY_SPLIT_PARENT)) {
                const long long rk = ranks[(size_t)2 * P + i];
                sj = ranks[(size_t)3 * P + i];
                if (rk < n_child && (long long)sj < n_split) ch = child0 + rk;
            }
            s_orig[threadIdx.x] = o;
            s_clone[threadIdx.x] = c;
            s_child[threadIdx.x] = ch;
            s_sample[threadIdx.x] = sj;
            s_kind[threadIdx.x] = (uint8_t)((o >= 0 ? 1 : 0) | (c >= 0 ? 2 : 0) | (ch >= 0 ? 4 : 0));
        }
        __syncthreads();
        for (int k = 0; k < num_tensors; k++) {
            const uint32_t w = (uint32_t)a.width[k];
            const int role = a.role[k];
            const uint32_t *__restrict__ src = a.src[k];
            uint32_t *__restrict__ dst = a.dst[k];
            const int64_t ss = a.src_stride[k], ds = a.dst_stride[k];
            const uint32_t total = (uint32_t)nrows * w;
            // word t of the round is (row t / w, column t % w); a thread's words are MOVE_THREADS apart, so row and column
            // advance by a constant with at most one carry: one division per tensor instead of one per word
            const uint32_t q = MOVE_THREADS / w, rem = MOVE_THREADS % w;
            uint32_t r = threadIdx.x / w, col = threadIdx.x - r * w;
            for (uint32_t t = threadIdx.x; t < total; t += MOVE_UNROLL * MOVE_THREADS) {
                uint32_t rr[MOVE_UNROLL], cc[MOVE_UNROLL], v[MOVE_UNROLL];
                uint8_t kind[MOVE_UNROLL];
#pragma unroll
                for (int u = 0; u < MOVE_UNROLL; u++) {  // all loads of the group first
                    rr[u] = r;
                    cc[u] = col;
                    kind[u] = t + (uint32_t)u * MOVE_THREADS < total ? s_kind[r] : (uint8_t)0;
                    // a dropped row is not even read, nor is a moment row whose original goes (its new rows are zero)
                    v[u] = (kind[u] & (role == GSR_DENSIFY_ROLE_MOMENT ? 1 : 7)) ? src[(base + r) * ss + col] : 0u;
                    col += rem;
                    r += q;
                    if (col >= w) {
                        col -= w;
                        r++;
                    }
                }
#pragma unroll
                for (int u = 0; u < MOVE_UNROLL; u++) {
                    if (kind[u] & 1) dst[s_orig[rr[u]] * ds + cc[u]] = v[u];
                    if (kind[u] & 2) dst[s_clone[rr[u]] * ds + cc[u]] = role == GSR_DENSIFY_ROLE_MOMENT ? 0u : v[u];
                    if (kind[u] & 4) {
                        const long long i = base + rr[u], ch = s_child[rr[u]];
                        uint32_t cv = v[u];
                        if (role == GSR_DENSIFY_ROLE_MOMENT) cv = 0u;
                        else if (role == GSR_DENSIFY_ROLE_SCALING) cv = a.alt[k][i * 3 + cc[u]];
                        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
                        if (role == GSR_DENSIFY_ROLE_XYZ) child_rotation_row((int)cc[u], rotation + i * 4, r0, r1, r2);
                        for (int cp = 0; cp < copies; cp++) {
                            if (role == GSR_DENSIFY_ROLE_XYZ) {  // R . sample + xyz, the dot summed left to right
                                const float *s3 = samples + ((long long)cp * n_split + s_sample[rr[u]]) * 3;
                                cv = __float_as_uint(r0 * s3[0] + r1 * s3[1] + r2 * s3[2] + __uint_as_float(v[u]));
                            }
                            dst[(ch + (long long)cp * n_child) * ds + cc[u]] = cv;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}
}  // namespace

extern "C" size_t gsr_densify_plan_bytes(int64_t P) {
    if (P < 0) return 0;
    return plan_layout(P).total;
}

extern "C" int gsr_densify_plan(int64_t P, const uint8_t *cls, int32_t *ranks, int32_t *split_rows, int64_t *counts,
                                void *workspace, size_t workspace_bytes, gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (P < 0 || P > RADIX_MAX_N) return GSR_EINVAL;
    if (P == 0) {
        if (counts) GSR_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * PLAN_CATS, stream));
        return 0;
    }
    if (!cls || !ranks || !counts || !workspace) return GSR_EINVAL;
    const PlanLayout L = plan_layout(P);
    if (workspace_bytes < L.total) return GSR_ENOSPACE;
    char *base = reinterpret_cast<char *>(workspace);
    GSR_HIP(hipMemsetAsync(base, 0, L.total, stream));
    hipLaunchKernelGGL(densify_plan_kernel, dim3((unsigned)L.tiles), dim3(PLAN_THREADS), 0, stream, (long long)P, cls,
                       ranks, split_rows, counts, reinterpret_cast<uint32_t *>(base + L.ticket),
                       reinterpret_cast<uint32_t *>(base + L.state), (uint32_t)L.tiles);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_densify_move(int64_t P, const uint8_t *cls, const int32_t *ranks, int64_t n_orig, int64_t n_clone,
                                int64_t n_child, int64_t n_split, int copies, int num_tensors,
                                const void *const *srcs, void *const *dsts, const void *const *alts,
                                const int32_t *widths, const int32_t *roles, const int64_t *src_strides,
                                const int64_t *dst_strides, int64_t dst_rows, const float *rotation,
                                const float *samples, gsr_stream_t stream_) {
    if (P < 0 || P > RADIX_MAX_N || n_orig < 0 || n_clone < 0 || n_child < 0 || n_split < 0 || copies < 1 ||
        copies > 16 || num_tensors < 0 || num_tensors > GATHER_MAX_TENSORS || dst_rows < 0)
        return GSR_EINVAL;
    if (n_orig > P || n_clone > P || n_split > P || n_child > n_split) return GSR_EINVAL;
    if (n_orig + n_clone + (int64_t)copies * n_child > dst_rows) return GSR_EINVAL;
    if (P == 0 || num_tensors == 0) return 0;
    if (!cls || !ranks || !srcs || !dsts || !widths || !roles || !src_strides || !dst_strides) return GSR_EINVAL;
    MoveArgs a{};
    for (int k = 0; k < num_tensors; k++) {
        if (!srcs[k] || !dsts[k] || widths[k] <= 0 || widths[k] > MOVE_MAX_WIDTH) return GSR_EINVAL;
        if (src_strides[k] < widths[k] || dst_strides[k] < widths[k]) return GSR_EINVAL;
        switch (roles[k]) {
        case GSR_DENSIFY_ROLE_COPY:
        case GSR_DENSIFY_ROLE_MOMENT:
            break;
        case GSR_DENSIFY_ROLE_XYZ:
            if (widths[k] != 3 || (n_child > 0 && (!rotation || !samples))) return GSR_EINVAL;
            break;
        case GSR_DENSIFY_ROLE_SCALING:
            if (widths[k] != 3 || !alts || !alts[k]) return GSR_EINVAL;
            break;
        default:
            return GSR_EINVAL;
        }
        a.src[k] = reinterpret_cast<const uint32_t *>(srcs[k]);
        a.dst[k] = reinterpret_cast<uint32_t *>(dsts[k]);
        a.alt[k] = alts ? reinterpret_cast<const uint32_t *>(alts[k]) : nullptr;
        a.width[k] = widths[k];
        a.role[k] = roles[k];
        a.src_stride[k] = src_strides[k];
        a.dst_stride[k] = dst_strides[k];
    }
    long long blocks = (P + MOVE_ROWS - 1) / MOVE_ROWS;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(densify_move_kernel, dim3((unsigned)blocks), dim3(MOVE_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream_), (long long)P, cls, ranks, (long long)n_orig,
                       (long long)n_clone, (long long)n_child, (long long)n_split, copies, num_tensors,
                       rotation, samples, a);
    GSR_LAUNCH_CHECK();
    return 0;
}
