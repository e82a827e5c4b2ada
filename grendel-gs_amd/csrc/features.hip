// features.hip -- an N-CHANNEL FEATURE MAP of one rendered view from the tile lists, and its backward (gfx950 / wave64).
//
// K8 (composite.hip) decides what every pixel blends; the kernels here walk the same lists once more and blend a
// per-Gaussian vector f_i in R^C instead of a colour: out[c][p] = sum over the blended entries of w f[c], w = alpha T (no
// background term, no division by 1 - T_final).  Nothing is re-decided: a pixel's walk ends where K8's ended (n_contrib),
// and the (pixel, entry) pairs taken are K10's `take` rule -- position + 1 <= n_contrib, power <= 0, alpha >= 1/255 -- in
// the arithmetic of composite_math.h.  The inverse-depth map (invdepth.hip) is the case C = 1, f = 1 / depth; these
// kernels have its shape and generalise it.  K8 / K10 / the contribution / invdepth / absgrad kernels are untouched; a
// trainer that does not ask for a feature map never launches these.
//
// CHANNEL CHUNKS.  The C channels are processed CH = 16 at a time (four float4 beside the entry's record in the slab), by
// a loop INSIDE the kernel: every chunk walks the quadrant's list again and recomputes alpha -- alpha is never stored per
// (pixel, entry) in HBM.  A request of C <= 4 channels runs the narrow instantiation (one float4, NQ = 1) of the same
// code, so that a one-channel map does not pay sixteen fmas per pair.  Channels beyond C in the last chunk are zeros in
// the slab and are never stored.  The arithmetic of a channel does not depend on C, on the chunk it falls in or on the
// instantiation: w is the same float and a channel's sum is one fmaf chain in list order.
//
// Forward (composite_features_kernel<NQ>): invdepth's forward.  One wave = one 8x8 quadrant, lane = pixel; the list is
// walked in 64-entry chunks, one entry per lane (index read + gather + quadrant test + the chunk's features), the relevant
// entries are compacted in list order into records in a wave-private LDS slab (the features beside the position word)
// and read back with wave-uniform addresses.  Per blended entry one fma per channel into registers, one store per channel
// per pixel at the end of the channel chunk.  The map is cleared by a fill in front of the launch.
//   LDS: (2 + NQ) float4 x 72 slots per wave: 6.75 KiB per wave, 27 KiB per workgroup at NQ = 4 (five workgroups per CU of
//   its 160 KiB); 3.4 KiB / 13.5 KiB at NQ = 1.  119 VGPRs (16 accumulators, and the eight entries of a group in flight
//   together): four waves per SIMD.
//
// Backward (composite_features_backward_kernel<NQ, FG>): K10's chain, back to front from final_T.  With alpha of the
// entry, Tn = T / (1 - alpha) is the transmittance in front of it.  The issue's per-channel recurrences rho_c = (what is
// blended behind in channel c) / (the transmittance behind) enter the result only through  sum_c g_c rho_c,  and that sum
// obeys the same recurrence with dot in place of (f_c - rho_c) -- so, as in K10, ONE scalar is carried:
//     cg  = sum_c g_c f_c                      (one fma per channel of the chunk, fixed order)
//     dot = cg - rho                            (= sum_c g_c (f_c - rho_c))
//     q   = o G Tn dot                          (= o G dL/dalpha of the chunk; G = exp(power), the clamp is the identity)
//     u   = alpha Tn                            (= w, the weight of the pair)
//     rho <- rho + alpha dot
// q is linear in the channels, so the chunks' moments simply add in the fp64 sums.
//   Geometry: invdepth's LDS transpose over a batch of CB = 8 entries -- phase A (lane = pixel) stores (q, u) into a wave-
//   private matrix [slot][pixel], phase B (lane = (slot, row of the quadrant)) forms the row's sums about dx itself and
//   three xor steps combine the rows; lane k < 6 of a slot adds value k of [means2D 2 | conic 3 | opacity] into acc64.
//   Feature gradient (FG): dL/df_i[c] = sum_p u[p] g_c[p] over the quadrant's 64 pixels is the contraction
//   [8 slots x 64 pixels] . [64 pixels x CH channels], on the MATRIX pipe: 16 K-steps of v_mfma_f32_16x16x4_f32 (exact fp32,
//   an fmaf chain; two accumulators as in K10).  Lane (k = lane >> 4, i = lane & 15) reads the u component of slot i & 7,
//   pixel 4 t + k of the SAME matrix phase A wrote (conflict-free with the row stride of 66) -- rows 8-15 of A repeat rows
//   0-7 and their results are not used -- against a per-lane B operand that is constant for the channel chunk: column j =
//   g_{chunk + j} of the pixel, zero outside the image and beyond C.  Result register r of a lane with k < 2 is (slot 4 k +
//   r, channel j): 16 adjacent lanes add 16 adjacent doubles of that Gaussian's row of acc64.  With FG = false (the caller
//   passes no dL_dfeatures: a constant feature such as an all-ones alpha column) the B operand, the MFMAs and these
//   atomics are compiled out and acc64 rows are six wide.
//   Entries no pixel of the quadrant blends issue nothing.
//   LDS per wave: (3 + NQ) float4 x 72 slots = 7.9 KiB slab, 288 B ids, 4.1 KiB matrix: 12.3 KiB per wave, 49.1 KiB per
//   workgroup at NQ = 4 (three workgroups per CU of its 160 KiB); 8.9 KiB / 35.6 KiB at NQ = 1 (four).  VGPRs at NQ = 4:
//   164 with FG (16 g, 16 B operand, 8 MFMA accumulators, the eight entries of a batch in flight), 115 without; 136 / 88
//   at NQ = 1: two to three waves per SIMD.
// A rounding pass then writes both fp32 records whole: each fp64 sum rounded once; rows blended nowhere are +0.0f.
#include "common.h"
#include "composite_math.h"

namespace {

typedef float feat_f32x4 __attribute__((ext_vector_type(4)));

constexpr int CB = 8;                   // entries per batch (forward: per unrolled group of the walk)
constexpr int MSTR = 66;                // row stride of the (q, u) matrix in 8-byte elements (16-byte aligned rows)
constexpr int NO_POS = 0x7fffffff;      // position word of an inert slot: no n_contrib reaches it
constexpr int CH = GSR_FEATURES_CHUNK;  // channels per chunk of the wide instantiation (NQ = 4 float4)

// block -> tile as in K8 / the contribution kernel; -1: this workgroup has no tile
__device__ __forceinline__ int features_tile_of_block(const int2 *__restrict__ ranges, int gx, int tiles, int band,
                                                      int band_first, int band_tiles) {
    if (band) {
        if (band_first < 0) {  // `band_tiles` is a capacity, the band is the row hull behind the range table
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

// channels [ch0 + 4 k, ch0 + 4 k + 4) of row `id` of the [P, C] table, zeros beyond C (rows are not 16-byte aligned)
__device__ __forceinline__ float4 feature_quad(const float *__restrict__ features, uint32_t id, int C, int c0) {
    const float *f = features + (size_t)id * C;
    float4 v;
    v.x = c0 + 0 < C ? f[c0 + 0] : 0.f;
    v.y = c0 + 1 < C ? f[c0 + 1] : 0.f;
    v.z = c0 + 2 < C ? f[c0 + 2] : 0.f;
    v.w = c0 + 3 < C ? f[c0 + 3] : 0.f;
    return v;
}

template <int NQ>
__global__ void __launch_bounds__(256)
composite_features_kernel(int C, int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                          const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                          const float4 *__restrict__ conic_opacity, const float *__restrict__ features,
                          const uint8_t *__restrict__ compute_locally, const int32_t *__restrict__ n_contrib, int band,
                          int band_first, int band_tiles, float *__restrict__ out) {
    constexpr int REC = 2 + NQ;  // float4 per slot: {x, y, a2, b2 | c2, o, position + 1, - | NQ feature quads}
    const int tile = features_tile_of_block(ranges, gx, tiles, band, band_first, band_tiles);
    if (tile < 0 || !compute_locally[tile]) return;  // (no workgroup barrier below: waves leave on their own)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx = tile % gx, ty = tile / gx;
    const int qx0 = tx * GSR_BLOCK_X + (wave & 1) * 8, qy0 = ty * GSR_BLOCK_Y + (wave >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const size_t pid = (size_t)py * W + px, HW = (size_t)H * W;
    const int2 range = ranges[tile];
    const int n = range.y - range.x;
    const float pxf = (float)px, pyf = (float)py;
    // where K8 stopped on this pixel; never beyond the list, whatever the caller's array holds
    const int last = inside ? min(n_contrib[pid], n) : 0;
    int wlen = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wlen = max(wlen, __shfl_xor(wlen, d, 64));
    if (wlen <= 0) return;  // (the map was cleared in front of the launch)

    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * REC];
    float4 *wslab = slab[wave];
    for (int ch0 = 0; ch0 < C; ch0 += 4 * NQ) {  // channel chunks: the whole walk again, alpha recomputed
        float T = 1.0f;
        float acc[4 * NQ];
#pragma unroll
        for (int k = 0; k < 4 * NQ; k++) acc[k] = 0.f;
        for (int c = 0; c < wlen; c += 64) {  // wave-uniform
            const bool have = c + lane < wlen;
            const uint32_t id = have ? point_list[range.x + c + lane] : 0u;
            const Entry e = load_entry(have, id, means2D, conic_opacity, (float)qx0, (float)qy0);
            const unsigned long long m = __ballot(e.relevant);
            const int nrel = __popcll(m);
            if (e.relevant) {
                const int pos = __popcll(m & ((1ull << lane) - 1ull));
                wslab[REC * pos] = make_float4(e.x, e.y, e.a2, e.b2);
                wslab[REC * pos + 1] = make_float4(e.c2, e.o, __int_as_float(c + lane + 1), 0.f);
#pragma unroll
                for (int k = 0; k < NQ; k++) wslab[REC * pos + 2 + k] = feature_quad(features, id, C, ch0 + 4 * k);
            }
            {   // the walk takes CB slots at a time: the <= CB - 1 slots behind the last entry are made inert (every word
                // written: nothing stale is ever read; features = 0)
                const int pad = (-nrel) & (CB - 1);
                if (lane < pad) {
                    wslab[REC * (nrel + lane)] = make_float4(0.f, 0.f, 0.f, 0.f);
                    wslab[REC * (nrel + lane) + 1] = make_float4(0.f, 0.f, __int_as_float(NO_POS), 0.f);
#pragma unroll
                    for (int k = 0; k < NQ; k++) wslab[REC * (nrel + lane) + 2 + k] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
            for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
#pragma unroll
                for (int s = 0; s < CB; s++) {
                    const float4 q0 = wslab[REC * (b0 + s)], q1 = wslab[REC * (b0 + s) + 1];  // wave-uniform: LDS broadcasts
                    const float pe = entry_exponent(q0, q1, q0.x - pxf, q0.y - pyf);
                    const float al = fminf(0.99f, entry_alpha_raw(q1, pe));
                    const bool take = __float_as_int(q1.z) <= last && entry_power_ok(q1, pe) && al >= ALPHA_MIN;
                    const float w = take ? al * T : 0.f;  // (selected, never multiplied: an inert slot's alpha is not used)
                    T -= w;  // T (1 - alpha) as K8 forms it: T - alpha T
#pragma unroll
                    for (int k = 0; k < NQ; k++) {
                        const float4 f = wslab[REC * (b0 + s) + 2 + k];
                        acc[4 * k + 0] = fmaf(w, f.x, acc[4 * k + 0]);
                        acc[4 * k + 1] = fmaf(w, f.y, acc[4 * k + 1]);
                        acc[4 * k + 2] = fmaf(w, f.z, acc[4 * k + 2]);
                        acc[4 * k + 3] = fmaf(w, f.w, acc[4 * k + 3]);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
        }
        if (inside) {
#pragma unroll
            for (int k = 0; k < 4 * NQ; k++)
                if (ch0 + k < C) out[(size_t)(ch0 + k) * HW + pid] = acc[k];
        }
    }
}

template <int NQ, bool FG>
__global__ void __launch_bounds__(256)
composite_features_backward_kernel(int C, int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                                   const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                                   const float4 *__restrict__ conic_opacity, const float *__restrict__ features,
                                   const uint8_t *__restrict__ compute_locally, const int32_t *__restrict__ n_contrib,
                                   const float *__restrict__ final_T, const float *__restrict__ dL_dout, int band,
                                   int band_first, int band_tiles, double *__restrict__ acc64) {
    constexpr int REC = 3 + NQ;  // float4 per slot: {x, y, a2, b2 | c2, o, position + 1, - | A, B, C, opacity | NQ feature quads}
    const int tile = features_tile_of_block(ranges, gx, tiles, band, band_first, band_tiles);
    if (tile < 0 || !compute_locally[tile]) return;  // (no workgroup barrier below: waves leave on their own)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx = tile % gx, ty = tile / gx;
    const int qx0 = tx * GSR_BLOCK_X + (wave & 1) * 8, qy0 = ty * GSR_BLOCK_Y + (wave >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < W && py < H;
    const size_t pid = (size_t)py * W + px, HW = (size_t)H * W;
    const int2 range = ranges[tile];
    const int n = range.y - range.x;
    const float pxf = (float)px, pyf = (float)py;
    const int last = inside ? min(n_contrib[pid], n) : 0;
    int wlen = last;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wlen = max(wlen, __shfl_xor(wlen, d, 64));
    if (wlen <= 0) return;
    const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;
    const size_t rs = FG ? (size_t)(6 + C) : (size_t)6;  // doubles per row of acc64
    const float T_final = inside ? final_T[pid] : 1.0f;

    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * REC];
    __shared__ uint32_t sids[4][64 + CB];
    __shared__ __attribute__((aligned(16))) float2 qmat[4][CB * MSTR];  // [wave][slot of the batch][pixel] = (q, u)
    float4 *wslab = slab[wave];
    uint32_t *wid = sids[wave];
    float2 *wm = qmat[wave];
    const int bslot = lane >> 3, bpart = lane & 7;  // phase B: this lane's slot of the batch and its row of the quadrant
    // MFMA operands of this lane: A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15], result register r = row 4 k + r
    const int kq = lane >> 4, mj = lane & 15;
    const float *arow = reinterpret_cast<const float *>(wm + (mj & 7) * MSTR + kq) + 1;  // the u component

    for (int ch0 = 0; ch0 < C; ch0 += 4 * NQ) {  // channel chunks: the whole walk again, alpha recomputed
        float g[4 * NQ];
#pragma unroll
        for (int k = 0; k < 4 * NQ; k++) g[k] = (inside && ch0 + k < C) ? dL_dout[(size_t)(ch0 + k) * HW + pid] : 0.f;
        [[maybe_unused]] float Bop[16];
        if (FG) {
            // K-step t contracts the pixels 4 t + k: column qx0 + k + 4 (t & 1), row qy0 + (t >> 1).  All sixteen values
            // are loaded from clamped addresses (in flight together) and selected by the bounds afterwards
            const bool chan = mj < 4 * NQ && ch0 + mj < C;
            const float *gb = dL_dout + (size_t)(chan ? ch0 + mj : 0) * HW;
            const int gx0 = qx0 + kq;
            const int cx0 = min(gx0, W - 1), cx1 = min(gx0 + 4, W - 1);
#pragma unroll
            for (int t = 0; t < 16; t++) Bop[t] = gb[(size_t)min(qy0 + (t >> 1), H - 1) * W + ((t & 1) ? cx1 : cx0)];
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const bool inb = ((t & 1) ? gx0 + 4 : gx0) < W && qy0 + (t >> 1) < H;
                Bop[t] = (chan && inb) ? Bop[t] : 0.f;
            }
        }
        float T = T_final;
        float rho = 0.f;  // sum_c g_c (channel c blended BEHIND the current position) / (the transmittance behind it)
        for (int c = ((wlen - 1) / 64) * 64; c >= 0; c -= 64) {  // wave-uniform, back to front
            const bool have = c + lane < wlen;
            const uint32_t id = have ? point_list[range.x + c + lane] : 0u;
            const Entry e = load_entry(have, id, means2D, conic_opacity, (float)qx0, (float)qy0);
            const unsigned long long m = __ballot(e.relevant);
            const int nrel = __popcll(m);
            if (e.relevant) {  // compacted in WALK order: rank = relevant lanes above
                const int pos = __popcll((m >> lane) >> 1);
                wslab[REC * pos] = make_float4(e.x, e.y, e.a2, e.b2);
                wslab[REC * pos + 1] = make_float4(e.c2, e.o, __int_as_float(c + lane + 1), 0.f);
                wslab[REC * pos + 2] = conic_opacity[id];
#pragma unroll
                for (int k = 0; k < NQ; k++) wslab[REC * pos + 3 + k] = feature_quad(features, id, C, ch0 + 4 * k);
                wid[pos] = id;
            }
            {   // the <= CB - 1 slots behind the last entry are inert: every word written, an opacity that divides
                const int pad = (-nrel) & (CB - 1);
                if (lane < pad) {
                    wslab[REC * (nrel + lane)] = make_float4(0.f, 0.f, 0.f, 0.f);
                    wslab[REC * (nrel + lane) + 1] = make_float4(0.f, 0.f, __int_as_float(NO_POS), 0.f);
                    wslab[REC * (nrel + lane) + 2] = make_float4(0.f, 0.f, 0.f, 1.f);
#pragma unroll
                    for (int k = 0; k < NQ; k++) wslab[REC * (nrel + lane) + 3 + k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    wid[nrel + lane] = 0u;
                }
            }
            __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
            for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
                // phase A, lane = pixel.  A lane that does not take an entry runs the same arithmetic with alpha = 0:
                // T / (1 - 0) and rho + 0 (...) leave its state untouched and it stores (0, 0)
                unsigned int any8 = 0u;  // bit s: some pixel of the quadrant blended slot s (a scalar register)
#pragma unroll
                for (int s = 0; s < CB; s++) {
                    const float4 q0 = wslab[REC * (b0 + s)], q1 = wslab[REC * (b0 + s) + 1];  // wave-uniform: LDS broadcasts
                    const float pe = entry_exponent(q0, q1, q0.x - pxf, q0.y - pyf);
                    const float aar = entry_alpha_raw(q1, pe);  // o exp(power), unclamped
                    const float aal = fminf(0.99f, aar);
                    const bool take = __float_as_int(q1.z) <= last && entry_power_ok(q1, pe) && aal >= ALPHA_MIN;
                    const float ar = take ? aar : 0.f, al = take ? aal : 0.f;  // (selected, never multiplied)
                    float cg = 0.f;  // sum_c g_c f_c over the chunk, channel order
#pragma unroll
                    for (int k = 0; k < NQ; k++) {
                        const float4 f = wslab[REC * (b0 + s) + 3 + k];
                        cg = fmaf(g[4 * k + 0], f.x, cg);
                        cg = fmaf(g[4 * k + 1], f.y, cg);
                        cg = fmaf(g[4 * k + 2], f.z, cg);
                        cg = fmaf(g[4 * k + 3], f.w, cg);
                    }
                    const float Tn = T / (1.f - al);      // transmittance in front of the entry
                    const float dot = cg - rho;           // sum_c g_c (f_c - what lies behind, normalised)
                    wm[s * MSTR + lane] = make_float2(ar * (Tn * dot), al * Tn);
                    rho = fmaf(al, dot, rho);
                    T = Tn;
                    any8 |= (__ballot(take) != 0ull ? 1u : 0u) << s;
                }
                __builtin_amdgcn_wave_barrier();
                // phase B, lane = (slot, row): the row's eight pixels in order, then the rows by xor 1, 2, 4
                const float4 p0 = wslab[REC * (b0 + bslot)];
                const float ex = p0.x - (float)qx0, dy = p0.y - (float)(qy0 + bpart);
                const float4 *qr = reinterpret_cast<const float4 *>(wm + bslot * MSTR + 8 * bpart);
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const float4 t = qr[h];  // pixels 2 h, 2 h + 1 of the row: (q, u, q, u)
                    const float dxa = ex - (float)(2 * h), dxb = ex - (float)(2 * h + 1);
                    s0 += t.x;
                    s1 = fmaf(t.x, dxa, s1);
                    s2 = fmaf(t.x * dxa, dxa, s2);
                    s0 += t.z;
                    s1 = fmaf(t.z, dxb, s1);
                    s2 = fmaf(t.z * dxb, dxb, s2);
                }
                float M0 = s0, Mx = s1, My = dy * s0, Mxx = s2, Mxy = dy * s1, Myy = dy * (dy * s0);
#pragma unroll
                for (int d = 1; d <= 4; d <<= 1) {
                    M0 += __shfl_xor(M0, d, 64);
                    Mx += __shfl_xor(Mx, d, 64);
                    My += __shfl_xor(My, d, 64);
                    Mxx += __shfl_xor(Mxx, d, 64);
                    Mxy += __shfl_xor(Mxy, d, 64);
                    Myy += __shfl_xor(Myy, d, 64);
                }
                // every lane of the slot holds the six sums; lane k < 6 adds value k of the row
                const float4 co = wslab[REC * (b0 + bslot) + 2];
                float val = -(co.x * Mx + co.y * My) * ddelx_dx;
                val = bpart == 1 ? -(co.y * Mx + co.z * My) * ddely_dy : val;
                val = bpart == 2 ? -0.5f * Mxx : val;
                val = bpart == 3 ? -Mxy : val;
                val = bpart == 4 ? -0.5f * Myy : val;
                val = bpart == 5 ? (M0 == 0.f ? 0.f : M0 / co.w) : val;
                if (bpart < 6 && ((any8 >> bslot) & 1u) && val != 0.f)
                    atomicAdd(acc64 + rs * (size_t)wid[b0 + bslot] + bpart, (double)val);
                if (FG) {
                    // [8 slots x 64 pixels] . [64 pixels x channels]: the u column of the matrix against the chunk's g
                    feat_f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};  // two chains: back-to-back issue
#pragma unroll
                    for (int t = 0; t < 16; t += 2) {
                        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[8 * t], Bop[t], a0, 0, 0, 0);  // pixel 4 t + k: 8 floats on
                        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[8 * t + 8], Bop[t + 1], a1, 0, 0, 0);
                    }
                    a0 += a1;
                    if (kq < 2 && mj < 4 * NQ && ch0 + mj < C) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int slot = 4 * kq + r;
                            if (((any8 >> slot) & 1u) && a0[r] != 0.f)
                                atomicAdd(acc64 + rs * (size_t)wid[b0 + slot] + 6 + ch0 + mj, (double)a0[r]);
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();  // the next batch overwrites the matrix only after these reads
            }
            __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
        }
    }
}

// the fp64 sums rounded once into the two fp32 records, which are written whole: columns 0:6 of a row into dL_record,
// the rest (when the feature gradient was formed) into dL_dfeatures
__global__ void features_record_kernel(const double *__restrict__ acc, int rs, float *__restrict__ rec,
                                       float *__restrict__ dfeat, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = acc[i];
    const float v = a == 0.0 ? 0.0f : (float)a;
    const size_t row = i / (size_t)rs;
    const int col = (int)(i - row * (size_t)rs);
    if (col < 6)
        rec[6 * row + col] = v;
    else
        dfeat[(size_t)(rs - 6) * row + (col - 6)] = v;
}

}  // namespace

int gsr_launch_composite_features(int P, int C, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                  const float *means2D, const float *conic_opacity, const float *features,
                                  const uint8_t *compute_locally, const int32_t *n_contrib, int row_lo, int row_hi,
                                  float *out, hipStream_t stream) {
    GSR_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)C * W * H, stream));
    if (P == 0) return 0;
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    auto kern = C <= 4 ? composite_features_kernel<1> : composite_features_kernel<CH / 4>;
    hipLaunchKernelGGL(kern, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, C, W, H, gx, gx * gy,
                       reinterpret_cast<const int2 *>(ranges), point_list, reinterpret_cast<const float2 *>(means2D),
                       reinterpret_cast<const float4 *>(conic_opacity), features, compute_locally, n_contrib,
                       b.band ? 1 : 0, b.band_first, b.band_tiles, out);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_composite_features_backward(int P, int C, int W, int H, const int32_t *ranges,
                                           const uint32_t *point_list, const float *means2D,
                                           const float *conic_opacity, const float *features,
                                           const uint8_t *compute_locally, const int32_t *n_contrib,
                                           const float *final_T, const float *dL_dout, int row_lo, int row_hi,
                                           float *dL_record, float *dL_dfeatures, double *acc64, hipStream_t stream) {
    const bool fg = dL_dfeatures != nullptr;
    const int rs = fg ? 6 + C : 6;
    GSR_HIP(hipMemsetAsync(acc64, 0, sizeof(double) * (size_t)rs * (size_t)P, stream));
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    auto kern = C <= 4 ? (fg ? composite_features_backward_kernel<1, true> : composite_features_backward_kernel<1, false>)
                       : (fg ? composite_features_backward_kernel<CH / 4, true>
                             : composite_features_backward_kernel<CH / 4, false>);
    hipLaunchKernelGGL(kern, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, C, W, H, gx, gx * gy,
                       reinterpret_cast<const int2 *>(ranges), point_list, reinterpret_cast<const float2 *>(means2D),
                       reinterpret_cast<const float4 *>(conic_opacity), features, compute_locally, n_contrib, final_T,
                       dL_dout, b.band ? 1 : 0, b.band_first, b.band_tiles, acc64);
    GSR_LAUNCH_CHECK();
    const size_t nrec = (size_t)rs * (size_t)P;
    hipLaunchKernelGGL(features_record_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, stream, acc64, rs,
                       dL_record, dL_dfeatures, nrec);
    GSR_LAUNCH_CHECK();
    return 0;
}
