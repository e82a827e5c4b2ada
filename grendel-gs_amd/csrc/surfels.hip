// surfels.hip -- the SURFEL GEOMETRY PASS of one rendered view from the tile lists: accumulated opacity, expected depth,
// blended normal, median depth and the depth distortion term in ONE forward walk, and their gradients in ONE backward
// walk (gfx950 / wave64).
//
// A side pass in the shape of tile_walk.h with a FIXED channel set.  Per-Gaussian input is the [P,5] surfel rows of
// gsr_normal_rows_forward, (1, z, n_x, n_y, n_z): columns 1..4 are read, column 0 is the constant 1.  The distortion
// measure is m = c0 + c1 z + c2 / z (three host scalars, as in distortion.hip; all zero: m = 0 and a zero distortion
// map).  What features.hip blends as C = 5 inside a 16-channel chunk, what distortion.hip walks the lists for a second
// time for, and the median depth that no kernel formed, share the `take` rule, w = alpha T and the transmittance
// recurrence; the backward chain is linear in the per-pixel "colour" of an entry, so the terms' colours add into one
// scalar recurrence.  K8 / K10 and the other side passes are untouched; a trainer that does not ask for the pass never
// launches these.
//
// Both kernels go through tile_walk.h's quadrant_begin, stage_chunk and pair_decision.  The helpers were NOT measured
// against a spelled-out prologue and pair decision here (four of the six older walks spell them out because the helpers
// measured slower or grew their VGPRs): an open measurement, not a finding.
//
// Forward (composite_surfels_kernel): front to back from T = 1, stage_chunk<FRONT_TO_BACK, 3>.  Slot record {x, y, a2, b2 | c2, o, position + 1, m | z, n_x, n_y, n_z}; m is formed once per staged
// entry in the word(id) callback; inert slots have every word written.  Per pixel in registers: T, A = sum w, D = sum w z,
// N = sum w n (fmaf chains in list order), mu, S, Dist by West's centred update exactly as composite_distortion_kernel
// forms it (never raw power sums; r = w / A' selected on w > 0), and the MEDIAN: per taken entry, before T is updated,
//     if (T > 0.5f) { med = z; medpos = position + 1; }
// -- the depth of the last taken entry whose transmittance in front of it exceeds 0.5 (2DGS's rule on the Gaussian
// centre's view depth).  A pixel that blends anything has a median (its first entry sees T = 1); one that blends
// nothing has med = +0, medpos = 0.  Every update is SELECTED on `take`, never multiplied by it.  One store per pixel
// and map at the end: surfel [5,H,W] = (A, D, N) (the layout normal_consistency takes), aux [4,H,W] = (Dist, mu, S,
// med), median_pos int32 [H,W]; the maps are cleared by fills in front of the launch, so tiles that are not ours and
// pixels that blend nothing are +0 and the bands of several launches assemble by SUM.
//   LDS: 3 float4 x 72 slots per wave = 3.4 KiB, 13.5 KiB per workgroup; 122 VGPRs, four waves per SIMD (the
//   compiler's resource report; features.hip's C = 16 forward has 119 and four).
//
// Backward (composite_surfels_backward_kernel<FG>): K10's chain, back to front from final_T, ONE scalar recurrence.  Per
// pixel: g_A, g_D, g_N[3] (dL/dsurfel), g_Dist, g_med -- any of the three upstream pointers may be null = zeros -- and
// the totals A, mu, S and medpos of the forward's maps.  Per (pixel, entry):
//     e   = g_A + g_D z + g_N . n + g_Dist (A (m - mu)^2 + S)
//     Tn  = T / (1 - alpha);  dot = e - rho;  q = alpha_raw Tn dot;  w = alpha Tn
//     v   = w 2 g_Dist A (m - mu) m'(z) + (position + 1 == medpos ? g_med : 0),   m'(z) = c1 - c2 / z^2
//     rho = fma(alpha, dot, rho);  T = Tn
// A lane that does not take the entry runs this with alpha = 0, and the median term is selected on `take` as well.  The
// discrete choice of the median passes no gradient to alpha or the geometry (as in 2DGS): g_med reaches only the depth
// of the chosen entry, for one compare in phase A.  m' RIDES IN THE SLAB beside m (formed once per staged entry), so v
// is dL/dz of the pair and acc64 keeps one depth column.  Slot record {x, y, a2, b2 | c2, o, position + 1, m | A, B, C,
// opacity | z, n_x, n_y, n_z | m', id, 0, 0}.
//   Transpose: (q, w) go through tile_walk.h's wave-private [slot][pixel] matrix and v through a one-word matrix beside it
//   (row stride VSTR); phase B (lane = (slot, row)) forms sum q and its five moments about dx, dy, plus sum v: the
//   distortion backward's seven sums, [means2D 2 | conic 3 | opacity | depth].
//   Matrix pipe (FG): the four sums that are linear in w with pixel-constant coefficients, sum_p w g_D (added to the
//   depth column) and sum_p w g_N[k], are the contraction [8 slots x 64 pixels] . [64 pixels x 4] as
//   composite_features_backward_kernel<.., FG> does it: 16 K-steps of v_mfma_f32_16x16x4_f32, the A operand read from
//   the w component of the matrix phase A wrote, the B operand (columns g_D, g_Nx, g_Ny, g_Nz, zero beyond) loaded ONCE
//   per wave, since g does not change over the walk.  With dL/dsurfel null (FG = false) this part is compiled out; phase
//   A is the same code, so the record is the same bits as with an all-zero map.  The distortion's depth sum is NOT formed
//   this way: m_i sum w g A - sum w g A mu cancels where the regulariser succeeds.
//   Entries no pixel of the quadrant blends issue nothing.  fp64 atomics into acc64 [P,10] = [means2D 2 | conic 3 |
//   opacity | z | n 3]; surfels_record_kernel rounds each sum once into dL_record [P,6] and dL_rows [P,5] (column 0 is
//   +0); rows blended nowhere are +0.0f.
//   LDS per wave: 5 float4 x 72 slots = 5.6 KiB slab (the ids ride in it), 4.1 KiB (q, w) matrix, 2.1 KiB v matrix: 11.9
//   KiB per wave, 47.5 KiB per workgroup -- three workgroups per CU of its 160 KiB, three waves per SIMD.  132
//   VGPRs with FG (16 B operand, 8 MFMA accumulators, the eight entries of a batch in flight), 106 without: the LDS
//   bounds the occupancy, not the registers (figures from the compiler's resource report; the NQ = 4 feature backward
//   has 49.1 KiB and 164).  Full-width 2- or 6-word matrices for every sum would leave two workgroups per CU.
#include "common.h"
#include "composite_math.h"
#include "tile_walk.h"

namespace {

typedef float surf_f32x4 __attribute__((ext_vector_type(4)));

constexpr int VSTR = 68;  // row stride of the one-word phase A matrix in floats (16-byte aligned rows)

__global__ void __launch_bounds__(256)
composite_surfels_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                         const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                         const float4 *__restrict__ conic_opacity, const float *__restrict__ rows,
                         const uint8_t *__restrict__ compute_locally, const int32_t *__restrict__ n_contrib, float c0,
                         float c1, float c2, int band, int band_first, int band_tiles, float *__restrict__ surfel,
                         float *__restrict__ aux, int32_t *__restrict__ median_pos) {
    Quadrant qd;
    if (!quadrant_begin(qd, W, H, gx, tiles, ranges, compute_locally, n_contrib, band, band_first, band_tiles)) return;

    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * 3];  // [wave][slot]: see the header
    float4 *wslab = slab[qd.wave];
    float T = 1.0f, A = 0.f, D = 0.f, Nx = 0.f, Ny = 0.f, Nz = 0.f, mu = 0.f, S = 0.f, Dist = 0.f, med = 0.f;
    int medpos = 0;
    for (int c = 0; c < qd.wlen; c += 64) {  // wave-uniform
        const int nrel = stage_chunk<FRONT_TO_BACK, 3>(
            c, qd.lane, qd.wlen, qd.range.x, qd.qx0, qd.qy0, point_list, means2D, conic_opacity, wslab,
            [&](uint32_t id) {
                const float z = rows[5 * (size_t)id + 1];
                return c0 + c1 * z + c2 / z;
            },
            [&](int slot, uint32_t id) {
                const float *r = rows + 5 * (size_t)id;  // (rows are not 16-byte aligned)
                wslab[3 * slot + 2] = make_float4(r[1], r[2], r[3], r[4]);
            },
            [&](int slot) { wslab[3 * slot + 2] = make_float4(0.f, 0.f, 0.f, 0.f); });
        __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
        for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const float4 q0 = wslab[3 * (b0 + s)], q1 = wslab[3 * (b0 + s) + 1];  // wave-uniform address: LDS broadcasts
                const float4 q2 = wslab[3 * (b0 + s) + 2];
                const Pair p = pair_decision(q0, q1, qd.pxf, qd.pyf, qd.last);
                const float w = p.take ? p.alpha * T : 0.f;  // (selected, never multiplied: an inert slot's alpha is not used)
                const bool front = p.take && T > 0.5f;       // the transmittance IN FRONT of the entry
                med = front ? q2.x : med;
                medpos = front ? __float_as_int(q1.z) : medpos;
                T -= w;  // T (1 - alpha) as K8 forms it: T - alpha T
                D = fmaf(w, q2.x, D);
                Nx = fmaf(w, q2.y, Nx);
                Ny = fmaf(w, q2.z, Ny);
                Nz = fmaf(w, q2.w, Nz);
                // West's update; with w = 0 every line leaves its register as it was
                const float m = q1.w;
                const float d = m - mu;
                Dist = fmaf(w, fmaf(A * d, d, S), Dist);
                A += w;
                const float r = w > 0.f ? w / A : 0.f;  // (A >= w > 0 where the quotient is formed; exactly 1 on the first entry)
                mu = fmaf(r, d, mu);
                S = fmaf(w * d, m - mu, S);
            }
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
    }
    if (qd.inside) {
        const size_t hw = (size_t)W * H;
        surfel[qd.pid] = A;
        surfel[hw + qd.pid] = D;
        surfel[2 * hw + qd.pid] = Nx;
        surfel[3 * hw + qd.pid] = Ny;
        surfel[4 * hw + qd.pid] = Nz;
        aux[qd.pid] = Dist;
        aux[hw + qd.pid] = mu;
        aux[2 * hw + qd.pid] = S;
        aux[3 * hw + qd.pid] = med;
        median_pos[qd.pid] = medpos;
    }
}

template <bool FG>
__global__ void __launch_bounds__(256)
composite_surfels_backward_kernel(int W, int H, int gx, int tiles, const int2 *__restrict__ ranges,
                                  const uint32_t *__restrict__ point_list, const float2 *__restrict__ means2D,
                                  const float4 *__restrict__ conic_opacity, const float *__restrict__ rows,
                                  const uint8_t *__restrict__ compute_locally, const int32_t *__restrict__ n_contrib,
                                  float c0, float c1, float c2, const float *__restrict__ final_T,
                                  const float *__restrict__ surfel, const float *__restrict__ aux,
                                  const int32_t *__restrict__ median_pos, const float *__restrict__ dL_dsurfel,
                                  const float *__restrict__ dL_ddist, const float *__restrict__ dL_dmedian, int band,
                                  int band_first, int band_tiles, double *__restrict__ acc64) {
    constexpr int REC = 5;
    Quadrant qd;
    if (!quadrant_begin(qd, W, H, gx, tiles, ranges, compute_locally, n_contrib, band, band_first, band_tiles)) return;
    const int lane = qd.lane, qx0 = qd.qx0, qy0 = qd.qy0;
    const bool inside = qd.inside;
    const size_t pid = qd.pid, hw = (size_t)W * H;
    // the upstream gradients of this pixel (a null map is zeros; phase A is the same code either way)
    const bool hs = inside && dL_dsurfel != nullptr;
    const float gA = hs ? dL_dsurfel[pid] : 0.f, gD = hs ? dL_dsurfel[hw + pid] : 0.f;
    const float gN0 = hs ? dL_dsurfel[2 * hw + pid] : 0.f, gN1 = hs ? dL_dsurfel[3 * hw + pid] : 0.f;
    const float gN2 = hs ? dL_dsurfel[4 * hw + pid] : 0.f;
    const float gDist = (inside && dL_ddist != nullptr) ? dL_ddist[pid] : 0.f;
    const float gmed = (inside && dL_dmedian != nullptr) ? dL_dmedian[pid] : 0.f;
    // the pixel's totals: A (m - mu)^2 + S is the distortion's "colour" of an entry on this pixel
    const float At = inside ? surfel[pid] : 0.f, mut = inside ? aux[hw + pid] : 0.f;
    const float St = inside ? aux[2 * hw + pid] : 0.f;
    const int medpos = inside ? median_pos[pid] : 0;  // (0: no entry's position + 1)
    const float gA2 = 2.f * gDist * At;
    const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;

    __shared__ __attribute__((aligned(16))) float4 slab[4][(64 + CB) * REC];
    __shared__ __attribute__((aligned(16))) float2 qmat[4][CB * MSTR];  // [wave][slot of the batch][pixel] = (q, w)
    __shared__ __attribute__((aligned(16))) float vmat[4][CB * VSTR];   // [wave][slot of the batch][pixel] = v
    float4 *wslab = slab[qd.wave];
    float2 *wm = qmat[qd.wave];
    float *vm = vmat[qd.wave];
    const int bslot = lane >> 3, bpart = lane & 7;  // phase B: this lane's slot of the batch and its row of the quadrant
    // MFMA operands of this lane: A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15], result register r = row 4 k + r
    const int kq = lane >> 4, mj = lane & 15;
    const float *arow = reinterpret_cast<const float *>(wm + (mj & 7) * MSTR + kq) + 1;  // the w component
    [[maybe_unused]] float Bop[16];
    if (FG) {
        // K-step t contracts the pixels 4 t + k: column qx0 + k + 4 (t & 1), row qy0 + (t >> 1).  Column j < 4 of B is
        // channel 1 + j of dL/dsurfel (g_D, g_Nx, g_Ny, g_Nz).  All sixteen values are loaded from clamped addresses (in
        // flight together) and selected by the bounds afterwards
        const bool chan = mj < 4;
        const float *gb = dL_dsurfel + (size_t)(chan ? 1 + mj : 1) * hw;
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
    float T = inside ? final_T[pid] : 1.0f;
    float rho = 0.f;  // (w e blended BEHIND the current position) / (the transmittance behind the current position)
    for (int c = ((qd.wlen - 1) / 64) * 64; c >= 0; c -= 64) {  // wave-uniform, back to front
        const int nrel = stage_chunk<BACK_TO_FRONT, REC>(
            c, lane, qd.wlen, qd.range.x, qx0, qy0, point_list, means2D, conic_opacity, wslab,
            [&](uint32_t id) {
                const float z = rows[5 * (size_t)id + 1];
                return c0 + c1 * z + c2 / z;
            },
            [&](int slot, uint32_t id) {
                const float *r = rows + 5 * (size_t)id;
                const float z = r[1];
                wslab[REC * slot + 2] = conic_opacity[id];
                wslab[REC * slot + 3] = make_float4(z, r[2], r[3], r[4]);
                wslab[REC * slot + 4] = make_float4(c1 - c2 / (z * z), __uint_as_float(id), 0.f, 0.f);
            },
            [&](int slot) {  // an opacity that divides
                wslab[REC * slot + 2] = make_float4(0.f, 0.f, 0.f, 1.f);
                wslab[REC * slot + 3] = make_float4(0.f, 0.f, 0.f, 0.f);
                wslab[REC * slot + 4] = make_float4(0.f, 0.f, 0.f, 0.f);
            });
        __builtin_amdgcn_wave_barrier();  // the wave's own LDS stores above precede its loads below
        for (int b0 = 0; b0 < nrel; b0 += CB) {  // wave-uniform
            // phase A, lane = pixel.  A lane that does not take an entry runs the same arithmetic with alpha = 0:
            // T / (1 - 0) and rho + 0 (...) leave its state untouched and it stores (0, 0) and 0
            unsigned int any8 = 0u;  // bit s: some pixel of the quadrant blended slot s (a scalar register)
#pragma unroll
            for (int s = 0; s < CB; s++) {
                const float4 q0 = wslab[REC * (b0 + s)], q1 = wslab[REC * (b0 + s) + 1];  // wave-uniform: LDS broadcasts
                const float4 q3 = wslab[REC * (b0 + s) + 3];
                const float mp = wslab[REC * (b0 + s) + 4].x;
                const Pair p = pair_decision(q0, q1, qd.pxf, qd.pyf, qd.last);
                const float ar = p.take ? p.raw : 0.f, al = p.take ? p.alpha : 0.f;  // (selected, never multiplied)
                const float Tn = T / (1.f - al);  // transmittance in front of the entry
                const float dm = q1.w - mut;      // m - mu of the pixel
                float e = fmaf(gD, q3.x, gA);
                e = fmaf(gN0, q3.y, e);
                e = fmaf(gN1, q3.z, e);
                e = fmaf(gN2, q3.w, e);
                e = fmaf(gDist, fmaf(At * dm, dm, St), e);
                const float dot = e - rho;  // e - (what lies behind, normalised)
                const float w = al * Tn;
                wm[s * MSTR + lane] = make_float2(ar * (Tn * dot), w);
                const bool hit = p.take && __float_as_int(q1.z) == medpos;
                vm[s * VSTR + lane] = fmaf(w * (gA2 * dm), mp, hit ? gmed : 0.f);
                rho = fmaf(al, dot, rho);
                T = Tn;
                any8 |= (__ballot(p.take) != 0ull ? 1u : 0u) << s;
            }
            __builtin_amdgcn_wave_barrier();
            // phase B, lane = (slot, row): the row's eight pixels in order, then the rows by xor 1, 2, 4
            const float4 p0 = wslab[REC * (b0 + bslot)];
            const float ex = p0.x - (float)qx0, dy = p0.y - (float)(qy0 + bpart);
            const float4 *qr = reinterpret_cast<const float4 *>(wm + bslot * MSTR + 8 * bpart);
            const float4 *vr = reinterpret_cast<const float4 *>(vm + bslot * VSTR + 8 * bpart);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const float4 t = qr[h];  // pixels 2 h, 2 h + 1 of the row: (q, w, q, w)
                const float dxa = ex - (float)(2 * h), dxb = ex - (float)(2 * h + 1);
                s0 += t.x;
                s1 = fmaf(t.x, dxa, s1);
                s2 = fmaf(t.x * dxa, dxa, s2);
                s0 += t.z;
                s1 = fmaf(t.z, dxb, s1);
                s2 = fmaf(t.z * dxb, dxb, s2);
            }
            const float4 va = vr[0], vb = vr[1];  // the row's eight v in pixel order
            const float sv = ((((((va.x + va.y) + va.z) + va.w) + vb.x) + vb.y) + vb.z) + vb.w;
            float M0 = s0, Mx = s1, My = dy * s0, Mxx = s2, Mxy = dy * s1, Myy = dy * (dy * s0), Sv = sv;
#pragma unroll
            for (int d = 1; d <= 4; d <<= 1) {
                M0 += __shfl_xor(M0, d, 64);
                Mx += __shfl_xor(Mx, d, 64);
                My += __shfl_xor(My, d, 64);
                Mxx += __shfl_xor(Mxx, d, 64);
                Mxy += __shfl_xor(Mxy, d, 64);
                Myy += __shfl_xor(Myy, d, 64);
                Sv += __shfl_xor(Sv, d, 64);
            }
            // every lane of the slot holds the seven sums; lane k < 7 adds value k of the row
            const float4 co = wslab[REC * (b0 + bslot) + 2];
            float val = -(co.x * Mx + co.y * My) * ddelx_dx;
            val = bpart == 1 ? -(co.y * Mx + co.z * My) * ddely_dy : val;
            val = bpart == 2 ? -0.5f * Mxx : val;
            val = bpart == 3 ? -Mxy : val;
            val = bpart == 4 ? -0.5f * Myy : val;
            val = bpart == 5 ? (M0 == 0.f ? 0.f : M0 / co.w) : val;
            val = bpart == 6 ? Sv : val;
            if (bpart < 7 && ((any8 >> bslot) & 1u) && val != 0.f)
                atomicAdd(acc64 + 10 * (size_t)__float_as_uint(wslab[REC * (b0 + bslot) + 4].y) + bpart, (double)val);
            if (FG) {
                // [8 slots x 64 pixels] . [64 pixels x 4]: the w column of the matrix against (g_D, g_Nx, g_Ny, g_Nz)
                surf_f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};  // two chains: back-to-back issue
#pragma unroll
                for (int t = 0; t < 16; t += 2) {
                    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[8 * t], Bop[t], a0, 0, 0, 0);  // pixel 4 t + k: 8 floats on
                    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[8 * t + 8], Bop[t + 1], a1, 0, 0, 0);
                }
                a0 += a1;
                if (kq < 2 && mj < 4) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int slot = 4 * kq + r;
                        if (((any8 >> slot) & 1u) && a0[r] != 0.f)
                            atomicAdd(acc64 + 10 * (size_t)__float_as_uint(wslab[REC * (b0 + slot) + 4].y) + 6 + mj,
                                      (double)a0[r]);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();  // the next batch overwrites the matrices only after these reads
        }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the slab only after these reads
    }
}

// the fp64 sums rounded once into the two fp32 records, which are written whole: columns 0:6 of a row into dL_record,
// 6:10 into columns 1:5 of dL_rows, whose column 0 (the constant 1) is +0
__global__ void surfels_record_kernel(const double *__restrict__ acc, float *__restrict__ rec, float *__restrict__ drows,
                                      size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = acc[i];
    const float v = a == 0.0 ? 0.0f : (float)a;
    const size_t row = i / 10;
    const int col = (int)(i - row * 10);
    if (col < 6) {
        rec[6 * row + col] = v;
    } else {
        drows[5 * row + (col - 5)] = v;
        if (col == 6) drows[5 * row] = 0.0f;
    }
}

}  // namespace

int gsr_launch_composite_surfels(int P, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                 const float *means2D, const float *conic_opacity, const float *rows,
                                 const uint8_t *compute_locally, const int32_t *n_contrib, float c0, float c1, float c2,
                                 int row_lo, int row_hi, float *surfel, float *aux, int32_t *median_pos,
                                 hipStream_t stream) {
    const size_t hw = (size_t)W * H;
    GSR_HIP(hipMemsetAsync(surfel, 0, sizeof(float) * 5 * hw, stream));
    GSR_HIP(hipMemsetAsync(aux, 0, sizeof(float) * 4 * hw, stream));
    GSR_HIP(hipMemsetAsync(median_pos, 0, sizeof(int32_t) * hw, stream));
    if (P == 0) return 0;
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    hipLaunchKernelGGL(composite_surfels_kernel, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, W, H, gx,
                       gx * gy, reinterpret_cast<const int2 *>(ranges), point_list,
                       reinterpret_cast<const float2 *>(means2D), reinterpret_cast<const float4 *>(conic_opacity), rows,
                       compute_locally, n_contrib, c0, c1, c2, b.band ? 1 : 0, b.band_first, b.band_tiles, surfel, aux,
                       median_pos);
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_composite_surfels_backward(int P, int W, int H, const int32_t *ranges, const uint32_t *point_list,
                                          const float *means2D, const float *conic_opacity, const float *rows,
                                          const uint8_t *compute_locally, const int32_t *n_contrib, float c0, float c1,
                                          float c2, const float *final_T, const float *surfel, const float *aux,
                                          const int32_t *median_pos, const float *dL_dsurfel, const float *dL_ddist,
                                          const float *dL_dmedian, int row_lo, int row_hi, float *dL_record,
                                          float *dL_rows, double *acc64, hipStream_t stream) {
    GSR_HIP(hipMemsetAsync(acc64, 0, sizeof(double) * 10 * (size_t)P, stream));
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const BandGrid b = band_grid_of(row_lo, row_hi, gx, gy);
    auto kern = dL_dsurfel != nullptr ? composite_surfels_backward_kernel<true> : composite_surfels_backward_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(b.band ? b.band_tiles : gx * gy), dim3(256), 0, stream, W, H, gx, gx * gy,
                       reinterpret_cast<const int2 *>(ranges), point_list, reinterpret_cast<const float2 *>(means2D),
                       reinterpret_cast<const float4 *>(conic_opacity), rows, compute_locally, n_contrib, c0, c1, c2,
                       final_T, surfel, aux, median_pos, dL_dsurfel, dL_ddist, dL_dmedian, b.band ? 1 : 0, b.band_first,
                       b.band_tiles, acc64);
    GSR_LAUNCH_CHECK();
    const size_t nrec = 10 * (size_t)P;
    hipLaunchKernelGGL(surfels_record_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, stream, acc64,
                       dL_record, dL_rows, nrec);
    GSR_LAUNCH_CHECK();
    return 0;
}
