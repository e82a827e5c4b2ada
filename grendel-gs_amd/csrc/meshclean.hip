// meshclean.hip -- mesh cleaning for gfx950 (include/gsraster.h: gsr_mesh_*): the connected components of an indexed
// triangle mesh, their triangle counts, the selection of the largest ones and the stable compaction of what is kept --
// what 2DGS / PGSR / GOF do with Open3D's cluster_connected_triangles on the host after the fusion.  The reference has
// no mesh path, so there is NO reference call site: a plain numpy union-find on the host is the arbiter
// (tests/meshclean_refs.py, tests/test_gpu_meshclean.py).  Integer work only: every result is exact.  DESIGN.md 3.22.
//
// DEFINITIONS
//   component    two vertices are connected if some triangle uses both; a component is a class of the transitive closure.
//                A triangle belongs to the component of its vertices.  On the manifold output of tsdf_extract this is the
//                partition Open3D's edge adjacency gives (two triangles sharing a vertex there share an edge fan).
//   label        the smallest vertex index of the component: labels[v], int32 [V].  A vertex no triangle uses is its own
//                component with zero triangles.
//   tri_count    tri_count[l], int32 [V]: the triangles of the component whose label is l; 0 where l is not a label.
//   selection    a component is kept iff tri_count >= max(min_triangles, 1) and, with keep_largest = k > 0, it is among
//                the first k in the order (tri_count descending, label ascending) taken over ALL components, before the
//                min_triangles test.  k = 0: no limit.
//   compaction   kept vertices and kept triangles keep their relative order (stable), faces are re-indexed, positions
//                and colours are copied bit for bit.  A vertex of a kept component is used by a kept triangle, so no
//                unreferenced vertex survives.  The output is a pure function of the input: the same bits on every run.
//
// KERNELS
//   mc_init_kernel      labels[v] = v (the forest lives in `labels`), tri_count[v] = 0.
//   mc_union_kernel     union-find.  Hooking always points the LARGER root at the SMALLER with a compare-and-swap on the
//                       parent word, so the root of a finished tree is its minimum whatever order the hardware took, and
//                       parents only ever decrease: every loop is bounded, nothing waits on another workgroup.
//                       A workgroup takes MC_CHUNK contiguous faces and the window of MC_WINDOW vertex indices from the
//                       chunk's smallest one (tsdf_emit writes brick by brick: almost every edge of a chunk stays in a
//                       narrow window).  Edges inside the window are united in LDS (LDS atomics, path halving); the local
//                       trees are then flattened and every window vertex that is not its local root is united ONCE with
//                       that root in global memory.  Only edges with an end outside the window take the global path
//                       directly; a mesh numbered arbitrarily takes it for everything (correct, slower).
//   mc_flatten_kernel   pointer jumping to the root; writes labels.
//   mc_count_kernel     per triangle an integer atomicAdd into tri_count[labels[faces[t][0]]]; a run of equal labels in a
//                       wave is merged into one atomic.
//   mc_flag_count_kernel / mc_scan_kernel / mc_flag_emit_kernel
//                       the count / one-workgroup scan / emit pattern of tsdf.hip over a 0/1 flag per item (is a root;
//                       vertex kept; face kept): the roots in increasing label order, and the new index of every vertex.
//   mc_select_kernel    ONE workgroup: the count of the k-th largest component by radix select (8-bit digits, most
//                       significant first) over the compacted roots, ties at that count by a stable scan in label order,
//                       one keep flag per root.
//   mc_compact_kernel   one pass: vertices and colours to their new rows, faces scanned per block and re-indexed.
#include "common.h"

namespace {

constexpr int MC_THREADS = 256;
// (MC_CHUNK and MC_WINDOW are mirrored as MESH_CHUNK_FACES / MESH_WINDOW_VERTICES in diff_gaussian_rasterization)
constexpr int MC_CHUNK = 2048;    // faces per workgroup of the union kernel (8 per lane)
constexpr int MC_WINDOW = 4096;   // vertex indices a workgroup holds in LDS: 16 KiB, nine workgroups per CU by LDS
constexpr int MC_BLOCK = 1024;    // items per workgroup of the flag kernels (4 per lane)
constexpr int MC_SCAN_THREADS = 1024;
enum { MC_ROOT = 0, MC_VERT = 1, MC_FACE = 2 };

#define MC_AGENT __HIP_MEMORY_SCOPE_AGENT
#define MC_WG __HIP_MEMORY_SCOPE_WORKGROUP

template <int SCOPE>
__device__ __forceinline__ int32_t mc_load(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// the root of x as far as this lane can see, halving the path on the way.  x strictly decreases: bounded.
template <int SCOPE>
__device__ __forceinline__ int32_t mc_find(int32_t *parent, int32_t x) {
    for (;;) {
        const int32_t p = mc_load<SCOPE>(parent + x);
        if (p == x) return x;
        const int32_t g = mc_load<SCOPE>(parent + p);
        if (g == p) return p;
        __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, SCOPE);  // (x is no root and never becomes one again)
        x = g;
    }
}

// unite the trees of a and b: the larger root is pointed at the smaller.  A compare-and-swap that fails hands back a
// smaller parent, so a + b strictly decreases from trip to trip: bounded, and no lane waits for another.
template <int SCOPE>
__device__ __forceinline__ void mc_union(int32_t *parent, int32_t a, int32_t b) {
    for (;;) {
        a = mc_find<SCOPE>(parent, a);
        b = mc_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        int32_t expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return;
        a = expected;
    }
}

__global__ void __launch_bounds__(MC_THREADS) mc_init_kernel(int V, int32_t *__restrict__ labels, int32_t *__restrict__ tri_count) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v < V) {
        labels[v] = (int32_t)v;
        tri_count[v] = 0;
    }
}

__device__ __forceinline__ int32_t mc_wave_min(int32_t v) {
#pragma unroll
    for (int o = GSR_WAVE / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, GSR_WAVE));
    return v;
}

__global__ void __launch_bounds__(MC_THREADS)
mc_union_kernel(long long F, const int32_t *__restrict__ faces, int32_t *parent) {
    __shared__ int32_t lp[MC_WINDOW];
    __shared__ int32_t s_lo[MC_THREADS / GSR_WAVE], s_hi[MC_THREADS / GSR_WAVE];
    constexpr int PER = MC_CHUNK / MC_THREADS;
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * MC_CHUNK;
    int32_t f[PER][3];
    int32_t lo = 0x7FFFFFFF, hi = -1;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const long long t = t0 + k * MC_THREADS + tid;
        if (t < F) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                f[k][j] = faces[(size_t)t * 3 + j];
                lo = min(lo, f[k][j]);
                hi = max(hi, f[k][j]);
            }
        } else {
            f[k][0] = f[k][1] = f[k][2] = -1;
        }
    }
    lo = mc_wave_min(lo);
    hi = -mc_wave_min(-hi);
    if ((tid & (GSR_WAVE - 1)) == 0) {
        s_lo[tid / GSR_WAVE] = lo;
        s_hi[tid / GSR_WAVE] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < MC_THREADS / GSR_WAVE; w++) {
        lo = min(lo, s_lo[w]);
        hi = max(hi, s_hi[w]);
    }
    // the window: [lo, lo + wn), wn <= MC_WINDOW (the chunk holds a face: lo <= hi)
    const uint32_t wn = (uint32_t)min((long long)MC_WINDOW, (long long)hi - lo + 1);
    for (uint32_t i = tid; i < wn; i += MC_THREADS) lp[i] = (int32_t)i;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; k++) {
        if (f[k][0] < 0) continue;
#pragma unroll
        for (int e = 0; e < 2; e++) {  // (a, b) and (b, c) connect the three
            const int32_t a = f[k][e], b = f[k][e + 1];
            const uint32_t la = (uint32_t)(a - lo), lb = (uint32_t)(b - lo);
            if (la < wn && lb < wn)
                mc_union<MC_WG>(lp, (int32_t)la, (int32_t)lb);
            else
                mc_union<MC_AGENT>(parent, a, b);
        }
    }
    __syncthreads();
    // the local trees are final: every vertex that is not its local root meets that root once in global memory
    for (uint32_t i = tid; i < wn; i += MC_THREADS) {
        int32_t r = lp[i];
        if (r == (int32_t)i) continue;
        for (int32_t p = lp[r]; p != r; p = lp[r]) r = p;
        mc_union<MC_AGENT>(parent, lo + (int32_t)i, lo + r);
    }
}

__global__ void __launch_bounds__(MC_THREADS) mc_flatten_kernel(int V, int32_t *labels) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V) return;
    // (other lanes store roots into the words this walk reads: either value is an ancestor, the end is the same root)
    int32_t x = (int32_t)v, p = mc_load<MC_AGENT>(labels + x);
    while (p != x) {
        x = p;
        p = mc_load<MC_AGENT>(labels + x);
    }
    __hip_atomic_store(labels + v, x, __ATOMIC_RELAXED, MC_AGENT);
}

__global__ void __launch_bounds__(MC_THREADS)
mc_count_kernel(long long F, const int32_t *__restrict__ faces, const int32_t *__restrict__ labels, int32_t *tri_count) {
    const long long t = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (GSR_WAVE - 1);
    const int32_t l = t < F ? labels[faces[(size_t)t * 3]] : -1;
    const int32_t before = __shfl_up(l, 1, GSR_WAVE);
    const bool head = lane == 0 || before != l;
    const unsigned long long above = (__ballot(head) >> lane) >> 1;  // the heads after this lane
    if (head && l >= 0) atomicAdd(tri_count + l, above ? __ffsll(above) : GSR_WAVE - lane);
}

// exclusive scan over the workgroup in lane order; `total` in every lane (`red`: one word per wave)
template <int NT>
__device__ __forceinline__ uint32_t mc_block_scan(uint32_t v, uint32_t *red, uint32_t &total) {
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
    for (int w = 0; w < NT / GSR_WAVE; w++) {
        if (w < wave) before += red[w];
        total += red[w];
    }
    return before + inc - v;
}

struct McFlagArgs {
    const int32_t *labels, *faces;
    const uint8_t *keep;
};
template <int MODE>
__device__ __forceinline__ uint32_t mc_flag(const McFlagArgs &a, long long i) {
    if (MODE == MC_ROOT) return a.labels[i] == (int32_t)i ? 1u : 0u;
    if (MODE == MC_VERT) return a.keep[a.labels[i]];
    return a.keep[a.labels[a.faces[(size_t)i * 3]]];
}

// the flags of block `blk` of `n` items, scanned in item order: pos[k] = the number of set flags before item
// blk * MC_BLOCK + k * MC_THREADS + lane inside the block; -> the block's total
template <int MODE>
__device__ __forceinline__ uint32_t mc_block_flags(const McFlagArgs &a, long long blk, long long n, uint32_t *red,
                                                   uint32_t (&flag)[MC_BLOCK / MC_THREADS],
                                                   uint32_t (&pos)[MC_BLOCK / MC_THREADS]) {
    uint32_t carry = 0;
#pragma unroll
    for (int k = 0; k < MC_BLOCK / MC_THREADS; k++) {
        const long long i = blk * MC_BLOCK + k * MC_THREADS + threadIdx.x;
        flag[k] = i < n ? mc_flag<MODE>(a, i) : 0u;
        uint32_t total;
        pos[k] = carry + mc_block_scan<MC_THREADS>(flag[k], red, total);
        carry += total;
    }
    return carry;
}

// block totals: blocks [0, nb0) over the n0 items of MODE0, blocks [nb0, ..) over the n1 items of MODE0 + 1
template <int MODE0>
__global__ void __launch_bounds__(MC_THREADS)
mc_flag_count_kernel(McFlagArgs a, long long n0, long long nb0, long long n1, uint32_t *__restrict__ btot) {
    __shared__ uint32_t red[MC_THREADS / GSR_WAVE];
    uint32_t flag[MC_BLOCK / MC_THREADS], pos[MC_BLOCK / MC_THREADS], total;
    const long long b = blockIdx.x;
    if (b < nb0)
        total = mc_block_flags<MODE0>(a, b, n0, red, flag, pos);
    else
        total = mc_block_flags<MODE0 + 1>(a, b - nb0, n1, red, flag, pos);
    if (threadIdx.x == 0) btot[b] = total;
}

// exclusive scan of the block totals by ONE workgroup, 1024 blocks per trip: segment 0 = blocks [0, nb0) -> tot0 (and
// dup0 if given), segment 1 = blocks [nb0, nb0 + nb1) -> tot1.  No look-back, no wait.
__global__ void __launch_bounds__(MC_SCAN_THREADS)
mc_scan_kernel(long long nb0, long long nb1, const uint32_t *__restrict__ btot, uint32_t *__restrict__ bbase,
               long long *__restrict__ tot0, long long *__restrict__ dup0, long long *__restrict__ tot1) {
    __shared__ uint32_t red[MC_SCAN_THREADS / GSR_WAVE];
    for (int seg = 0; seg < 2; seg++) {
        const long long first = seg ? nb0 : 0, nb = seg ? nb1 : nb0;
        long long *tot = seg ? tot1 : tot0;
        if (!tot) continue;
        uint32_t carry = 0;  // (a segment's total is at most 2^31 - 1 items)
        for (long long base = 0; base < nb; base += MC_SCAN_THREADS) {
            const long long i = base + threadIdx.x;
            const uint32_t v = i < nb ? btot[first + i] : 0u;
            uint32_t total;
            const uint32_t ex = mc_block_scan<MC_SCAN_THREADS>(v, red, total);
            if (i < nb) bbase[first + i] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) {
            *tot = (long long)carry;
            if (!seg && dup0) *dup0 = (long long)carry;
        }
    }
}

// MC_ROOT: out[base + pos] = the root (the roots in increasing label order);  MC_VERT: out[v] = its new index, or -1
template <int MODE>
__global__ void __launch_bounds__(MC_THREADS)
mc_flag_emit_kernel(McFlagArgs a, long long n, const uint32_t *__restrict__ bbase, int32_t *__restrict__ out) {
    __shared__ uint32_t red[MC_THREADS / GSR_WAVE];
    uint32_t flag[MC_BLOCK / MC_THREADS], pos[MC_BLOCK / MC_THREADS];
    mc_block_flags<MODE>(a, blockIdx.x, n, red, flag, pos);
    const uint32_t base = bbase[blockIdx.x];
#pragma unroll
    for (int k = 0; k < MC_BLOCK / MC_THREADS; k++) {
        const long long i = (long long)blockIdx.x * MC_BLOCK + k * MC_THREADS + threadIdx.x;
        if (i >= n) continue;
        if (MODE == MC_ROOT) {
            if (flag[k]) out[base + pos[k]] = (int32_t)i;
        } else {
            out[i] = flag[k] ? (int32_t)(base + pos[k]) : -1;
        }
    }
}

// ONE workgroup.  With 0 < k < R: T = the count of the k-th largest component by radix select, most significant digit
// first (a histogram of the candidates' digit in LDS, the digit that holds the `rem`-th from the top, the candidates
// narrowed to it); `rem` then says how many components with count == T the order admits, and a stable scan over the roots
// (increasing label) hands those places to the lowest labels.  Otherwise T = 0 and every component passes the order.
__global__ void __launch_bounds__(MC_SCAN_THREADS)
mc_select_kernel(const long long *__restrict__ nroots, const int32_t *__restrict__ roots,
                 const int32_t *__restrict__ tri_count, int k, int min_triangles, uint8_t *__restrict__ keep) {
    __shared__ uint32_t hist[256], red[MC_SCAN_THREADS / GSR_WAVE], s_prefix, s_rem;
    const int tid = threadIdx.x;
    const long long R = *nroots;
    uint32_t T = 0, rem = 0xFFFFFFFFu;
    if (k > 0 && k < R) {  // (uniform)
        uint32_t prefix = 0, mask = 0;
        rem = (uint32_t)k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (long long i = tid; i < R; i += MC_SCAN_THREADS) {
                const uint32_t c = (uint32_t)tri_count[roots[i]];
                if ((c & mask) == prefix) atomicAdd(&hist[(c >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t before = 0;
                int d = 255;
                for (; d > 0 && before + hist[d] < rem; d--) before += hist[d];  // (at least `rem` candidates: d = 0 holds it)
                s_prefix = prefix | ((uint32_t)d << shift);
                s_rem = rem - before;
            }
            __syncthreads();
            prefix = s_prefix;
            rem = s_rem;
            mask |= 255u << shift;
        }
        T = prefix;
    }
    const uint32_t need = (uint32_t)max(min_triangles, 1);
    uint32_t carry = 0;
    for (long long base = 0; base < R; base += MC_SCAN_THREADS) {
        const long long i = base + tid;
        const int32_t r = i < R ? roots[i] : 0;
        const uint32_t c = i < R ? (uint32_t)tri_count[r] : 0u;
        const uint32_t eq = (i < R && c == T) ? 1u : 0u;
        uint32_t total;
        const uint32_t rank = carry + mc_block_scan<MC_SCAN_THREADS>(eq, red, total);
        if (i < R) keep[r] = ((c > T || (eq && rank < rem)) && c >= need) ? 1 : 0;
        carry += total;
    }
}

__global__ void mc_zero_totals_kernel(long long *a, long long *b) {
    if (a) a[0] = 0;
    if (b) b[0] = 0;
}

// block b moves the vertices [b MC_BLOCK, ..) to their new rows (words, not floats: bit for bit) and writes the kept
// faces of [b MC_BLOCK, ..) at the block's base + their rank, re-indexed.  Nothing is written past nv rows / nt faces.
template <bool COLOR>
__global__ void __launch_bounds__(MC_THREADS)
mc_compact_kernel(McFlagArgs a, long long V, long long F, long long nfb, const uint32_t *__restrict__ vertices,
                  const uint32_t *__restrict__ colors, const int32_t *__restrict__ vmap,
                  const uint32_t *__restrict__ fbase, uint32_t nv, uint32_t nt, uint32_t *__restrict__ out_vertices,
                  uint32_t *__restrict__ out_colors, int32_t *__restrict__ out_faces) {
    __shared__ uint32_t red[MC_THREADS / GSR_WAVE];
    const long long b = blockIdx.x;
#pragma unroll
    for (int k = 0; k < MC_BLOCK / MC_THREADS; k++) {
        const long long v = b * MC_BLOCK + k * MC_THREADS + threadIdx.x;
        if (v >= V) continue;
        const int32_t m = vmap[v];
        if (m < 0 || (uint32_t)m >= nv) continue;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            out_vertices[(size_t)m * 3 + c] = vertices[(size_t)v * 3 + c];
            if (COLOR) out_colors[(size_t)m * 3 + c] = colors[(size_t)v * 3 + c];
        }
    }
    if (b >= nfb) return;  // (uniform)
    uint32_t flag[MC_BLOCK / MC_THREADS], pos[MC_BLOCK / MC_THREADS];
    mc_block_flags<MC_FACE>(a, b, F, red, flag, pos);
    const uint32_t base = fbase[b];
#pragma unroll
    for (int k = 0; k < MC_BLOCK / MC_THREADS; k++) {
        const long long t = b * MC_BLOCK + k * MC_THREADS + threadIdx.x;
        const uint32_t o = base + pos[k];
        if (!flag[k] || o >= nt) continue;  // (flag is 0 past F)
#pragma unroll
        for (int c = 0; c < 3; c++) out_faces[(size_t)o * 3 + c] = vmap[a.faces[(size_t)t * 3 + c]];
    }
}

// the workspace: roots int32 [V] | vmap int32 [V] | block totals uint32 [nvb + nfb] | block bases alike | the number of
// roots, int64 | keep uint8 [V]
struct McLayout {
    long long nvb, nfb;
    size_t roots, vmap, btot, bbase, nroots, keep, total;
};
bool mc_layout(int64_t V, int64_t F, McLayout &L) {
    if (V < 0 || F < 0 || V > 0x7FFFFFFFLL || F > 0x7FFFFFFFLL) return false;
    L.nvb = (V + MC_BLOCK - 1) / MC_BLOCK;
    L.nfb = (F + MC_BLOCK - 1) / MC_BLOCK;
    const size_t nb = (size_t)(L.nvb + L.nfb), v4 = ((size_t)V * 4 + 15) & ~(size_t)15, b4 = (nb * 4 + 15) & ~(size_t)15;
    L.roots = 0;
    L.vmap = v4;
    L.btot = 2 * v4;
    L.bbase = L.btot + b4;
    L.nroots = L.bbase + b4;
    L.keep = L.nroots + 16;
    L.total = L.keep + (((size_t)V + 15) & ~(size_t)15);
    return true;
}
template <typename T>
T *mc_at(void *ws, size_t off) {
    return reinterpret_cast<T *>(static_cast<char *>(ws) + off);
}

}  // namespace

extern "C" size_t gsr_mesh_clean_bytes(int64_t V, int64_t F) {
    McLayout L;
    return mc_layout(V, F, L) ? L.total : 0;
}

extern "C" int gsr_mesh_components(int64_t V, int64_t F, const int32_t *faces, int32_t *labels, int32_t *tri_count,
                                   int64_t *num_components, void *workspace, size_t workspace_bytes,
                                   gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    McLayout L;
    if (!mc_layout(V, F, L) || !num_components) return GSR_EINVAL;
    if ((V > 0 && (!labels || !tri_count || !workspace)) || (F > 0 && (!faces || V == 0))) return GSR_EINVAL;
    if (V > 0 && workspace_bytes < L.total) return GSR_ENOSPACE;
    long long *nc = reinterpret_cast<long long *>(num_components);
    if (V == 0) {
        hipLaunchKernelGGL(mc_zero_totals_kernel, dim3(1), dim3(1), 0, stream, nc, (long long *)nullptr);
        GSR_LAUNCH_CHECK();
        return 0;
    }
    const unsigned vgrid = (unsigned)gsr_div_up(V, MC_THREADS);
    hipLaunchKernelGGL(mc_init_kernel, dim3(vgrid), dim3(MC_THREADS), 0, stream, (int)V, labels, tri_count);
    if (F > 0) {
        hipLaunchKernelGGL(mc_union_kernel, dim3((unsigned)gsr_div_up(F, MC_CHUNK)), dim3(MC_THREADS), 0, stream,
                           (long long)F, faces, labels);
        hipLaunchKernelGGL(mc_flatten_kernel, dim3(vgrid), dim3(MC_THREADS), 0, stream, (int)V, labels);
        hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)gsr_div_up(F, MC_THREADS)), dim3(MC_THREADS), 0, stream,
                           (long long)F, faces, labels, tri_count);
    }
    const McFlagArgs a{labels, faces, nullptr};
    uint32_t *btot = mc_at<uint32_t>(workspace, L.btot), *bbase = mc_at<uint32_t>(workspace, L.bbase);
    hipLaunchKernelGGL(mc_flag_count_kernel<MC_ROOT>, dim3((unsigned)L.nvb), dim3(MC_THREADS), 0, stream, a, (long long)V,
                       L.nvb, 0LL, btot);
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, stream, L.nvb, 0LL, btot, bbase,
                       mc_at<long long>(workspace, L.nroots), nc, (long long *)nullptr);
    hipLaunchKernelGGL(mc_flag_emit_kernel<MC_ROOT>, dim3((unsigned)L.nvb), dim3(MC_THREADS), 0, stream, a, (long long)V,
                       bbase, mc_at<int32_t>(workspace, L.roots));
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_mesh_select(int64_t V, int64_t F, const int32_t *faces, const int32_t *labels,
                               const int32_t *tri_count, int64_t keep_largest, int64_t min_triangles, void *workspace,
                               size_t workspace_bytes, int64_t *totals, gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    McLayout L;
    if (!mc_layout(V, F, L) || keep_largest < 0 || min_triangles < 0 || !totals) return GSR_EINVAL;
    long long *tot = reinterpret_cast<long long *>(totals);
    if (V == 0 || F == 0) {  // no triangle: nothing is kept
        hipLaunchKernelGGL(mc_zero_totals_kernel, dim3(1), dim3(1), 0, stream, tot, tot + 1);
        GSR_LAUNCH_CHECK();
        return 0;
    }
    if (!faces || !labels || !tri_count || !workspace) return GSR_EINVAL;
    if (workspace_bytes < L.total) return GSR_ENOSPACE;
    // (a component has at most F <= 2^31 - 1 triangles and there are at most V of them: larger arguments say the same)
    const int k = (int)(keep_largest > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : keep_largest);
    const int mt = (int)(min_triangles > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : min_triangles);
    uint8_t *keep = mc_at<uint8_t>(workspace, L.keep);
    uint32_t *btot = mc_at<uint32_t>(workspace, L.btot), *bbase = mc_at<uint32_t>(workspace, L.bbase);
    hipLaunchKernelGGL(mc_select_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, stream, mc_at<long long>(workspace, L.nroots),
                       mc_at<int32_t>(workspace, L.roots), tri_count, k, mt, keep);
    const McFlagArgs a{labels, faces, keep};
    hipLaunchKernelGGL(mc_flag_count_kernel<MC_VERT>, dim3((unsigned)(L.nvb + L.nfb)), dim3(MC_THREADS), 0, stream, a,
                       (long long)V, L.nvb, (long long)F, btot);
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, stream, L.nvb, L.nfb, btot, bbase, tot,
                       (long long *)nullptr, tot + 1);
    hipLaunchKernelGGL(mc_flag_emit_kernel<MC_VERT>, dim3((unsigned)L.nvb), dim3(MC_THREADS), 0, stream, a, (long long)V,
                       bbase, mc_at<int32_t>(workspace, L.vmap));
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_mesh_compact(int64_t V, int64_t F, const float *vertices, const float *colors, const int32_t *faces,
                                const int32_t *labels, const void *workspace, size_t workspace_bytes,
                                int64_t num_vertices, int64_t num_triangles, float *out_vertices, float *out_colors,
                                int32_t *out_faces, gsr_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    McLayout L;
    if (!mc_layout(V, F, L) || num_vertices < 0 || num_triangles < 0 || num_vertices > V || num_triangles > F)
        return GSR_EINVAL;
    if ((out_colors != nullptr) != (colors != nullptr)) return GSR_EINVAL;
    if (num_vertices == 0 && num_triangles == 0) return 0;
    if (!vertices || !faces || !labels || !workspace) return GSR_EINVAL;
    if ((num_vertices && !out_vertices) || (num_triangles && !out_faces)) return GSR_EINVAL;
    if (workspace_bytes < L.total) return GSR_ENOSPACE;
    void *ws = const_cast<void *>(workspace);
    const McFlagArgs a{labels, faces, mc_at<uint8_t>(ws, L.keep)};
    const unsigned grid = (unsigned)(L.nvb > L.nfb ? L.nvb : L.nfb);
    const uint32_t *vin = reinterpret_cast<const uint32_t *>(vertices), *cin = reinterpret_cast<const uint32_t *>(colors);
    uint32_t *vout = reinterpret_cast<uint32_t *>(out_vertices), *cout = reinterpret_cast<uint32_t *>(out_colors);
    if (colors)
        hipLaunchKernelGGL(mc_compact_kernel<true>, dim3(grid), dim3(MC_THREADS), 0, stream, a, (long long)V, (long long)F,
                           L.nfb, vin, cin, mc_at<int32_t>(ws, L.vmap), mc_at<uint32_t>(ws, L.bbase) + L.nvb,
                           (uint32_t)num_vertices, (uint32_t)num_triangles, vout, cout, out_faces);
    else
        hipLaunchKernelGGL(mc_compact_kernel<false>, dim3(grid), dim3(MC_THREADS), 0, stream, a, (long long)V, (long long)F,
                           L.nfb, vin, cin, mc_at<int32_t>(ws, L.vmap), mc_at<uint32_t>(ws, L.bbase) + L.nvb,
                           (uint32_t)num_vertices, (uint32_t)num_triangles, vout, cout, out_faces);
    GSR_LAUNCH_CHECK();
    return 0;
}
