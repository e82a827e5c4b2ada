// preprocess.hip -- K1 (per-Gaussian projection + SH colour) and K11 (its backward) for gfx950.
//
// One lane per Gaussian: 256-thread workgroups (4 waves) forward, 128-thread workgroups (K11_BLOCK, 2 waves) backward.
// Both kernels are pure HBM streaming:
// 236 B in / 44+31 B out per Gaussian forward, 552 B per Gaussian backward.
// Camera matrices are wave-uniform and are read through the scalar cache into SGPRs.
//
// What the kernels compute restates SURVEY.md Appendix A.2 / A.6 (reference call site
// gaussian_renderer/__init__.py:949-960).  The forward geometry is compiled with FP contraction
// off so that integer outputs (radii, tile rects) are reproducible against a plain C evaluation.
#include "common.h"

#include <atomic>
#include <initializer_list>
#include <type_traits>

// no FMA contraction in this file: see the header comment (memory-bound kernels, no cost)
#pragma clang fp contract(off)

namespace {

__constant__ const float SH_C0 = 0.28209479177387814f;
__constant__ const float SH_C1 = 0.4886025119029199f;
__constant__ const float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                     -1.0925484305920792f, 0.5462742152960396f};
__constant__ const float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                     0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                     -0.5900435899266435f};

struct Cam {
    float v[16];  // viewmatrix, row-major, row-vector convention
    float p[16];  // full projection
    float c[3];   // camera centre
};

__device__ __forceinline__ Cam load_cam(const float *__restrict__ view, const float *__restrict__ proj,
                                        const float *__restrict__ campos) {
    Cam cam;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        cam.v[i] = view[i];
        cam.p[i] = proj[i];
    }
    cam.c[0] = campos[0];
    cam.c[1] = campos[1];
    cam.c[2] = campos[2];
    return cam;
}

__device__ __forceinline__ void quat_to_R(const float4 q, float R[3][3]) {
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

// T = J * Wc (2x3) with the +-1.3 tanfov clamp applied for the Jacobian only
__device__ __forceinline__ void compute_T(const float t[3], const float *v, float fx, float fy, float tanfovx,
                                          float tanfovy, float T[2][3], float tc[3], bool &xin, bool &yin) {
    const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
    const float txtz = t[0] / t[2], tytz = t[1] / t[2];
    xin = !(txtz < -limx || txtz > limx);
    yin = !(tytz < -limy || tytz > limy);
    tc[0] = fminf(limx, fmaxf(-limx, txtz)) * t[2];
    tc[1] = fminf(limy, fmaxf(-limy, tytz)) * t[2];
    tc[2] = t[2];
    const float J00 = fx / tc[2], J02 = -(fx * tc[0]) / (tc[2] * tc[2]);
    const float J11 = fy / tc[2], J12 = -(fy * tc[1]) / (tc[2] * tc[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        T[0][k] = J00 * v[k * 4 + 0] + J02 * v[k * 4 + 2];
        T[1][k] = J11 * v[k * 4 + 1] + J12 * v[k * 4 + 2];
    }
}

template <int DEG>
__device__ __forceinline__ void eval_sh(const float *__restrict__ sh, float x, float y, float z, float out[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float r = SH_C0 * sh[0 * 3 + c];
        if (DEG > 0) {
            r = r - SH_C1 * y * sh[1 * 3 + c] + SH_C1 * z * sh[2 * 3 + c] - SH_C1 * x * sh[3 * 3 + c];
            if (DEG > 1) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                r = r + SH_C2[0] * xy * sh[4 * 3 + c] + SH_C2[1] * yz * sh[5 * 3 + c] +
                    SH_C2[2] * (2.f * zz - xx - yy) * sh[6 * 3 + c] + SH_C2[3] * xz * sh[7 * 3 + c] +
                    SH_C2[4] * (xx - yy) * sh[8 * 3 + c];
                if (DEG > 2) {
                    r = r + SH_C3[0] * y * (3.f * xx - yy) * sh[9 * 3 + c] + SH_C3[1] * xy * z * sh[10 * 3 + c] +
                        SH_C3[2] * y * (4.f * zz - xx - yy) * sh[11 * 3 + c] +
                        SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * sh[12 * 3 + c] +
                        SH_C3[4] * x * (4.f * zz - xx - yy) * sh[13 * 3 + c] +
                        SH_C3[5] * z * (xx - yy) * sh[14 * 3 + c] + SH_C3[6] * x * (xx - 3.f * yy) * sh[15 * 3 + c];
                }
            }
        }
        out[c] = r;
    }
}

// ------------------------------------------------------------------- the projection math, one copy
// Every kernel below is built from these pieces.  They only compute: what is loaded where, what is stored where and in
// which order partial gradients are added stays with the kernels (with contraction off the same expression gives the
// same bits wherever it is inlined, so the fused, batched and camera-gradient kernels agree with K11 exactly).

// t = [p, 1] * viewmatrix: the position in camera space
__device__ __forceinline__ void view_transform(const float *v, const float (&p)[3], float (&t)[3]) {
    t[0] = v[0] * p[0] + v[4] * p[1] + v[8] * p[2] + v[12];
    t[1] = v[1] * p[0] + v[5] * p[1] + v[9] * p[2] + v[13];
    t[2] = v[2] * p[0] + v[6] * p[1] + v[10] * p[2] + v[14];
}

// [p, 1] * projmatrix: x, y and mw = 1 / (w + 1e-7)
__device__ __forceinline__ void project_hom(const float *pm, const float (&p)[3], float &phx, float &phy, float &mw) {
    phx = pm[0] * p[0] + pm[4] * p[1] + pm[8] * p[2] + pm[12];
    phy = pm[1] * p[0] + pm[5] * p[1] + pm[9] * p[2] + pm[13];
    const float phw = pm[3] * p[0] + pm[7] * p[1] + pm[11] * p[2] + pm[15];
    mw = 1.0f / (phw + 0.0000001f);
}

// the getters' activations of the raw parameters (scene/gaussian_model.py:109-129)
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float4 quat_normalize(const float4 q, float &qnr, float &qn) {
    qnr = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    qn = fmaxf(qnr, 1e-12f);
    return make_float4(q.x / qn, q.y / qn, q.z / qn, q.w / qn);
}

// Sigma = R S S R^T from the ACTIVATED quaternion and scales (s includes the scale modifier)
__device__ __forceinline__ void cov3d_from_scale_rot(const float4 q, const float (&s)[3], float (&S)[3][3]) {
    float R[3][3];
    quat_to_R(q, R);
    float L[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) L[a][b] = R[a][b] * s[b];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) S[a][b] = L[a][0] * L[b][0] + L[a][1] * L[b][1] + L[a][2] * L[b][2];
}
// the six stored words of Sigma (upper triangle) as the full matrix
__device__ __forceinline__ void cov3d_unpack(const float *cv, float (&S)[3][3]) {
    S[0][0] = cv[0]; S[0][1] = cv[1]; S[0][2] = cv[2];
    S[1][0] = cv[1]; S[1][1] = cv[3]; S[1][2] = cv[4];
    S[2][0] = cv[2]; S[2][1] = cv[4]; S[2][2] = cv[5];
}

// cov2D = T Sigma T^T + 0.3 I = [[a, b], [b, c]]; ST0 / ST1 = Sigma T^T's columns, which the backward needs again.
// a0, c0: the diagonal BEFORE the dilation, for the anti-aliased variant (taken here, not a - 0.3f afterwards: that
// difference has lost a0's low bits wherever a0 < 0.3); a caller that does not use them pays nothing.
__device__ __forceinline__ void cov2d_abc(const float (&S)[3][3], const float (&T)[2][3], float (&ST0)[3],
                                          float (&ST1)[3], float &a, float &b, float &c, float &a0, float &c0) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ST0[r] = S[r][0] * T[0][0] + S[r][1] * T[0][1] + S[r][2] * T[0][2];
        ST1[r] = S[r][0] * T[1][0] + S[r][1] * T[1][1] + S[r][2] * T[1][2];
    }
    a0 = T[0][0] * ST0[0] + T[0][1] * ST0[1] + T[0][2] * ST0[2];
    a = a0 + 0.3f;
    b = T[0][0] * ST1[0] + T[0][1] * ST1[1] + T[0][2] * ST1[2];
    c0 = T[1][0] * ST1[0] + T[1][1] * ST1[1] + T[1][2] * ST1[2];
    c = c0 + 0.3f;
}

// ---- anti-aliasing (the 2D Mip filter; include/gsraster.h: gsr_set_antialiasing).  AA is a template argument of every
// piece and kernel below that it reaches: the AA = false instantiations are the code without it, instruction for
// instruction.  q = det0 / det, the share of the dilated splat's energy that the undilated one had; the opacity is
// scaled by rho = sqrt(max(AA_QMIN, q)), 0.005 <= rho < 1.
constexpr float AA_QMIN = 0.000025f;
__device__ __forceinline__ float aa_q(float a0, float b, float c0, float det) { return (a0 * c0 - b * b) / det; }
__device__ __forceinline__ float aa_rho(float q) { return sqrtf(fmaxf(AA_QMIN, q)); }

// The geometry of one (Gaussian, camera) pair in front of the near plane (the caller culls t[2] <= 0.2 BEFORE it loads
// what Sigma is made of): conic, radius and pixel centre.  false: culled (singular cov2D, or a rect of no tiles); g is
// then not to be used.  Straight-line on purpose, with ONE test at the end: with a return after each of the two culls
// the camera-batched forward needed 4-6 registers more and lost a wave per SIMD at degrees 0 and 1.
struct Geom2D {
    int rad;
    float2 xy;
    float conic[3];
    float rho;  // AA: the opacity's factor (1 otherwise)
};
template <bool AA>
__device__ __forceinline__ bool project_geometry(const Cam &cam, float tanfovx, float tanfovy, float fx, float fy, int W,
                                                 int H, int gx, int gy, const float (&p)[3], const float (&t)[3],
                                                 const float (&S)[3][3], Geom2D &g) {
    float phx, phy, pw;
    project_hom(cam.p, p, phx, phy, pw);
    const float pprojx = phx * pw, pprojy = phy * pw;
    float T[2][3], tc[3];
    bool xin, yin;
    compute_T(t, cam.v, fx, fy, tanfovx, tanfovy, T, tc, xin, yin);
    float ST0[3], ST1[3], a, b, c, a0, c0;
    cov2d_abc(S, T, ST0, ST1, a, b, c, a0, c0);
    const float det = a * c - b * b;
    const float det_inv = 1.f / det;
    g.rho = AA ? aa_rho(aa_q(a0, b, c0, det)) : 1.f;
    const float mid = 0.5f * (a + c);
    const float lam = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
    g.rad = (int)ceilf(3.f * sqrtf(lam));
    const float px = ((pprojx + 1.0f) * W - 1.0f) * 0.5f;
    const float py = ((pprojy + 1.0f) * H - 1.0f) * 0.5f;
    int minx, miny, maxx, maxy;
    gsr_get_rect(px, py, g.rad, gx, gy, minx, miny, maxx, maxy);
    g.xy = make_float2(px, py);
    g.conic[0] = c * det_inv;
    g.conic[1] = -b * det_inv;
    g.conic[2] = a * det_inv;
    return det != 0.0f && (maxx - minx) * (maxy - miny) != 0;
}

// colour from SH along the world-space view direction, +0.5, clamped at 0 (cl: which channels clamped)
template <int DEG>
__device__ __forceinline__ void shade(const float (&campos)[3], const float (&p)[3], const float *__restrict__ sh,
                                      float (&col)[3], bool (&cl)[3]) {
    float d[3] = {p[0] - campos[0], p[1] - campos[1], p[2] - campos[2]};
    const float inv = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    d[0] *= inv;
    d[1] *= inv;
    d[2] *= inv;
    eval_sh<DEG>(sh, d[0], d[1], d[2], col);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        col[k] += 0.5f;
        cl[k] = col[k] < 0.f;
        col[k] = fmaxf(col[k], 0.f);
    }
}

// conic gradient (gA, gB, gC) -> cov2D -> T = J Wc -> (Sigma, t) of one (Gaussian, camera) pair
struct Cov2DGrad {
    bool live;       // 1 / (denom^2 + 1e-7) != 0: otherwise dL/d(a, b, c) and dcov are zero
    float dcov[6];   // this pair's dL/dSigma, upper triangle (off-diagonal entries count both halves)
    float dT0[3], dT1[3];
    float dt[3], tc[3];  // dL/dt, and t with the Jacobian's clamp
    float dmean[3];      // dt through the view matrix: the pair's cov2D part of dL/dmean
    float rho;           // AA: the forward's factor of the opacity, recomputed (1 otherwise)
};
// AA: gop = dL/dconic_opacity.w times the uncompensated opacity.  With w = gop / (2 rho) = dL/dq, w dq/d(a, b, c) joins
// the conic's dL/d(a, b, c) before these feed dcov, dT and dt -- unless the forward clamped q (q <= AA_QMIN: rho is then
// a constant).  dq/d(a, b, c) in closed form, h = det - det0 = 0.3 (a0 + c0) + 0.09 (the quotient rule's
// c0 det - det0 c cancels for large splats, q -> 1), over the TRUE det^2, not the conic part's det^2 + 1e-7.
template <bool AA = false>
__device__ __forceinline__ Cov2DGrad cov2d_backward(const float *v, float fx, float fy, float tanfovx, float tanfovy,
                                                    const float (&p)[3], const float (&S)[3][3], float gA, float gB,
                                                    float gC, float gop = 0.f) {
    Cov2DGrad o;
    float t[3];
    view_transform(v, p, t);
    float T[2][3];
    bool xin, yin;
    compute_T(t, v, fx, fy, tanfovx, tanfovy, T, o.tc, xin, yin);
    float ST0[3], ST1[3], a, b, c, a0, c0;
    cov2d_abc(S, T, ST0, ST1, a, b, c, a0, c0);
    const float denom = a * c - b * b;
    const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
    const float q = AA ? aa_q(a0, b, c0, denom) : 1.f;
    o.rho = AA ? aa_rho(q) : 1.f;
    float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
#pragma unroll
    for (int e = 0; e < 6; e++) o.dcov[e] = 0.f;
    o.live = denom2inv != 0.f;
    if (o.live) {
        dL_da = denom2inv * (-c * c * gA + b * c * gB + (denom - a * c) * gC);
        dL_dc = denom2inv * (-a * a * gC + a * b * gB + (denom - a * c) * gA);
        dL_db = denom2inv * (2.f * b * c * gA - (denom + 2.f * b * b) * gB + 2.f * a * b * gC);
        if (AA && q > AA_QMIN) {
            const float w = gop / (2.f * o.rho), di = 1.f / denom;
            const float h = 0.3f * (a0 + c0) + 0.09f;
            dL_da += w * ((0.3f * (c0 * c0 + b * b) + 0.09f * c0) * di * di);
            dL_dc += w * ((0.3f * (a0 * a0 + b * b) + 0.09f * a0) * di * di);
            dL_db += w * ((-2.f * b * h) * di * di);
        }
        o.dcov[0] = T[0][0] * T[0][0] * dL_da + T[0][0] * T[1][0] * dL_db + T[1][0] * T[1][0] * dL_dc;
        o.dcov[3] = T[0][1] * T[0][1] * dL_da + T[0][1] * T[1][1] * dL_db + T[1][1] * T[1][1] * dL_dc;
        o.dcov[5] = T[0][2] * T[0][2] * dL_da + T[0][2] * T[1][2] * dL_db + T[1][2] * T[1][2] * dL_dc;
        o.dcov[1] = 2.f * T[0][0] * T[0][1] * dL_da + (T[0][0] * T[1][1] + T[0][1] * T[1][0]) * dL_db +
                    2.f * T[1][0] * T[1][1] * dL_dc;
        o.dcov[2] = 2.f * T[0][0] * T[0][2] * dL_da + (T[0][0] * T[1][2] + T[0][2] * T[1][0]) * dL_db +
                    2.f * T[1][0] * T[1][2] * dL_dc;
        o.dcov[4] = 2.f * T[0][2] * T[0][1] * dL_da + (T[0][1] * T[1][2] + T[0][2] * T[1][1]) * dL_db +
                    2.f * T[1][1] * T[1][2] * dL_dc;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.dT0[k] = 2.f * ST0[k] * dL_da + ST1[k] * dL_db;
        o.dT1[k] = 2.f * ST1[k] * dL_dc + ST0[k] * dL_db;
    }
    const float dJ00 = o.dT0[0] * v[0] + o.dT0[1] * v[4] + o.dT0[2] * v[8];
    const float dJ02 = o.dT0[0] * v[2] + o.dT0[1] * v[6] + o.dT0[2] * v[10];
    const float dJ11 = o.dT1[0] * v[1] + o.dT1[1] * v[5] + o.dT1[2] * v[9];
    const float dJ12 = o.dT1[0] * v[2] + o.dT1[1] * v[6] + o.dT1[2] * v[10];
    const float tz = 1.f / o.tc[2], tz2 = tz * tz, tz3 = tz2 * tz;
    o.dt[0] = (xin ? 1.f : 0.f) * (-fx * tz2 * dJ02);
    o.dt[1] = (yin ? 1.f : 0.f) * (-fy * tz2 * dJ12);
    o.dt[2] = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2.f * fx * o.tc[0]) * tz3 * dJ02 + (2.f * fy * o.tc[1]) * tz3 * dJ12;
#pragma unroll
    for (int k = 0; k < 3; k++) o.dmean[k] = v[k * 4 + 0] * o.dt[0] + v[k * 4 + 1] * o.dt[1] + v[k * 4 + 2] * o.dt[2];
    return o;
}

// the perspective divide of means2D (NDC-scaled): mw = 1 / (w + 1e-7), mul1 = x mw^2, mul2 = y mw^2
__device__ __forceinline__ void perspective_backward(const float *pm, const float (&p)[3], float &mw, float &mul1,
                                                     float &mul2) {
    float phx, phy;
    project_hom(pm, p, phx, phy, mw);
    mul1 = phx * mw * mw;
    mul2 = phy * mw * mw;
}
// ... and the means2D part of dL/dmean that K11 forms from it
__device__ __forceinline__ void means2d_to_mean(const float *pm, const float (&p)[3], const float2 g2, float (&dm)[3]) {
    float mw, mul1, mul2;
    perspective_backward(pm, p, mw, mul1, mul2);
#pragma unroll
    for (int k = 0; k < 3; k++)
        dm[k] = (pm[k * 4 + 0] * mw - pm[k * 4 + 3] * mul1) * g2.x + (pm[k * 4 + 1] * mw - pm[k * 4 + 3] * mul2) * g2.y;
}

// the accessors and sinks of sh_backward below (named functors: hipcc 7.2 crashes in its inliner on closures here)
struct ShRegs {  // coefficients in registers, [k][ch]
    const float *sh;
    __device__ __forceinline__ float operator()(int k, int ch) const { return sh[k * 3 + ch]; }
};
struct ShStagedOrRegs {  // the batched kernel: the coefficients above DC in the LDS stage, or all of them in registers
    bool staged;
    const float *lds, *sh;
    __device__ __forceinline__ float operator()(int k, int ch) const { return staged ? lds[k * 3 + ch - 3] : sh[k * 3 + ch]; }
};
struct DshAssign {
    float *dsh;
    __device__ __forceinline__ void operator()(int k, int ch, float v) const { dsh[k * 3 + ch] = v; }
};
struct DshAdd {
    float *dsh;
    __device__ __forceinline__ void operator()(int k, int ch, float v) const { dsh[k * 3 + ch] += v; }
};
struct DshDrop {
    __device__ __forceinline__ void operator()(int, int, float) const {}
};

// Colour gradient g (0 for a clamped channel) -> SH coefficients and unit view direction (x, y, z).
//   sh(k, ch):        coefficient k >= 1 of channel ch -- registers, or the LDS stage of the batched kernel
//   dsh(k, ch, v):    receives dL/d(coefficient k of channel ch) -- assigned by the one-camera body, accumulated over
//                     the cameras by the batched one, dropped by K11c
//   ddir:             d colour / d direction contracted with g
template <int DEG, typename SH, typename DSH>
__device__ __forceinline__ void sh_backward(const SH &sh, float x, float y, float z, const float (&g3)[3],
                                            const DSH &dsh, float (&ddir)[3]) {
    ddir[0] = ddir[1] = ddir[2] = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const float g = g3[ch];
        float dx = 0.f, dy = 0.f, dz = 0.f;
        dsh(0, ch, SH_C0 * g);
        if (DEG > 0) {
            dsh(1, ch, -SH_C1 * y * g);
            dsh(2, ch, SH_C1 * z * g);
            dsh(3, ch, -SH_C1 * x * g);
            dx = -SH_C1 * sh(3, ch);
            dy = -SH_C1 * sh(1, ch);
            dz = SH_C1 * sh(2, ch);
            if (DEG > 1) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                dsh(4, ch, SH_C2[0] * xy * g);
                dsh(5, ch, SH_C2[1] * yz * g);
                dsh(6, ch, SH_C2[2] * (2.f * zz - xx - yy) * g);
                dsh(7, ch, SH_C2[3] * xz * g);
                dsh(8, ch, SH_C2[4] * (xx - yy) * g);
                dx += SH_C2[0] * y * sh(4, ch) + SH_C2[2] * 2.f * -x * sh(6, ch) + SH_C2[3] * z * sh(7, ch) +
                      SH_C2[4] * 2.f * x * sh(8, ch);
                dy += SH_C2[0] * x * sh(4, ch) + SH_C2[1] * z * sh(5, ch) + SH_C2[2] * 2.f * -y * sh(6, ch) +
                      SH_C2[4] * 2.f * -y * sh(8, ch);
                dz += SH_C2[1] * y * sh(5, ch) + SH_C2[2] * 2.f * 2.f * z * sh(6, ch) + SH_C2[3] * x * sh(7, ch);
                if (DEG > 2) {
                    dsh(9, ch, SH_C3[0] * y * (3.f * xx - yy) * g);
                    dsh(10, ch, SH_C3[1] * xy * z * g);
                    dsh(11, ch, SH_C3[2] * y * (4.f * zz - xx - yy) * g);
                    dsh(12, ch, SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * g);
                    dsh(13, ch, SH_C3[4] * x * (4.f * zz - xx - yy) * g);
                    dsh(14, ch, SH_C3[5] * z * (xx - yy) * g);
                    dsh(15, ch, SH_C3[6] * x * (xx - 3.f * yy) * g);
                    dx += SH_C3[0] * sh(9, ch) * 3.f * 2.f * xy + SH_C3[1] * sh(10, ch) * yz +
                          SH_C3[2] * sh(11, ch) * -2.f * xy + SH_C3[3] * sh(12, ch) * -3.f * 2.f * xz +
                          SH_C3[4] * sh(13, ch) * (-3.f * xx + 4.f * zz - yy) + SH_C3[5] * sh(14, ch) * 2.f * xz +
                          SH_C3[6] * sh(15, ch) * 3.f * (xx - yy);
                    dy += SH_C3[0] * sh(9, ch) * 3.f * (xx - yy) + SH_C3[1] * sh(10, ch) * xz +
                          SH_C3[2] * sh(11, ch) * (-3.f * yy + 4.f * zz - xx) + SH_C3[3] * sh(12, ch) * -3.f * 2.f * yz +
                          SH_C3[4] * sh(13, ch) * -2.f * xy + SH_C3[5] * sh(14, ch) * -2.f * yz +
                          SH_C3[6] * sh(15, ch) * -3.f * 2.f * xy;
                    dz += SH_C3[1] * sh(10, ch) * xy + SH_C3[2] * sh(11, ch) * 4.f * 2.f * yz +
                          SH_C3[3] * sh(12, ch) * 3.f * (2.f * zz - xx - yy) + SH_C3[4] * sh(13, ch) * 4.f * 2.f * xz +
                          SH_C3[5] * sh(14, ch) * (xx - yy);
                }
            }
        }
        ddir[0] += dx * g;
        ddir[1] += dy * g;
        ddir[2] += dz * g;
    }
}
// ... with the direction formed from p - campos in front and carried back to the position behind: dm is the pair's
// view-direction part of dL/dmean (and minus its part of dL/dcampos)
template <int DEG, typename SH, typename DSH>
__device__ __forceinline__ void viewdir_backward(const float (&campos)[3], const float (&p)[3], const SH &sh,
                                                 const float (&g3)[3], const DSH &dsh, float (&dm)[3]) {
    const float dox = p[0] - campos[0], doy = p[1] - campos[1], doz = p[2] - campos[2];
    const float len = sqrtf(dox * dox + doy * doy + doz * doz);
    const float x = dox / len, y = doy / len, z = doz / len;
    float ddir[3];
    sh_backward<DEG>(sh, x, y, z, g3, dsh, ddir);
    const float dot = x * ddir[0] + y * ddir[1] + z * ddir[2];
    dm[0] = (ddir[0] - x * dot) / len;
    dm[1] = (ddir[1] - y * dot) / len;
    dm[2] = (ddir[2] - z * dot) / len;
}

// dL/dSigma (dcov, as Cov2DGrad's) -> scales and quaternion.  Sigma = M^T M, M = S R^T.  RAW: q and sc are the raw
// parameters and the gradients go through their activations (normalize, exp) as well.
template <bool RAW>
__device__ __forceinline__ void cov3d_backward(const float4 qraw, const float (&scraw)[3], float scale_modifier,
                                               const float (&dcov)[6], float (&gsc)[3], float4 &dq) {
    float4 q = qraw;
    float sc[3] = {scraw[0], scraw[1], scraw[2]};
    float qn = 1.f, qnr = 1.f;
    if (RAW) {
        q = quat_normalize(qraw, qnr, qn);
        sc[0] = expf(sc[0]);
        sc[1] = expf(sc[1]);
        sc[2] = expf(sc[2]);
    }
    float R[3][3];
    quat_to_R(q, R);
    const float s[3] = {scale_modifier * sc[0], scale_modifier * sc[1], scale_modifier * sc[2]};
    float Mm[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int cc = 0; cc < 3; cc++) Mm[r][cc] = s[r] * R[cc][r];
    const float dS[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                            {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                            {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
    float dM[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int cc = 0; cc < 3; cc++)
            dM[r][cc] = 2.f * (Mm[r][0] * dS[0][cc] + Mm[r][1] * dS[1][cc] + Mm[r][2] * dS[2][cc]);
    float dR[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        gsc[r] = (RAW ? sc[r] : 1.f) *  // d exp(x) = exp(x) dx
                 scale_modifier * (R[0][r] * dM[r][0] + R[1][r] * dM[r][1] + R[2][r] * dM[r][2]);
#pragma unroll
        for (int j = 0; j < 3; j++) dR[j][r] = s[r] * dM[r][j];
    }
    const float r_ = q.x, x = q.y, y = q.z, z = q.w;
    dq.x = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
    dq.y = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r_ * dR[1][2] + z * dR[2][0] +
                  r_ * dR[2][1] - 2.f * x * dR[2][2]);
    dq.z = 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r_ * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r_ * dR[2][0] +
                  z * dR[2][1] - 2.f * y * dR[2][2]);
    dq.w = 2.f * (-2.f * z * dR[0][0] - r_ * dR[0][1] + x * dR[0][2] + r_ * dR[1][0] - 2.f * z * dR[1][1] +
                  y * dR[1][2] + x * dR[2][0] + y * dR[2][1]);
    if (RAW) {  // through q = x / max(|x|, 1e-12)
        const float dot = qnr > 1e-12f ? (q.x * dq.x + q.y * dq.y + q.z * dq.z + q.w * dq.w) : 0.f;
        dq = make_float4((dq.x - q.x * dot) / qn, (dq.y - q.y * dot) / qn, (dq.z - q.z * dot) / qn,
                         (dq.w - q.w * dot) / qn);
    }
}

// ------------------------------------------------------------------------------------------- K1
// RAW = true: the inputs are the RAW parameters of GaussianModel (log-scales, un-normalised quaternions,
// opacity logits, SH split into _features_dc [N,1,3] = `shs` and _features_rest [N,M-1,3] = `shs_rest`) and the
// getters' activations (scene/gaussian_model.py:109-129: exp, normalize, sigmoid, cat) are applied in
// registers -- no activated copies of the 59 floats per Gaussian are written to / re-read from HBM.
template <int DEG, bool RAW, bool AA>
__global__ void __launch_bounds__(GSR_ONE_DIM_BLOCK)
preprocess_forward_kernel(int P, int M, const float *__restrict__ means3D, const float *__restrict__ scales,
                          float scale_modifier, const float *__restrict__ rotations, const float *__restrict__ shs,
                          const float *__restrict__ shs_rest, const float *__restrict__ opacities, const float *__restrict__ view,
                          const float *__restrict__ proj, const float *__restrict__ campos, int W, int H,
                          float tanfovx, float tanfovy, float2 *__restrict__ means2D, float *__restrict__ depths,
                          int32_t *__restrict__ radii, float *__restrict__ cov3D, float4 *__restrict__ conic_opacity,
                          float *__restrict__ rgb, uint8_t *__restrict__ clamped) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const Cam cam = load_cam(view, proj, campos);
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const float fx = W / (2.0f * tanfovx), fy = H / (2.0f * tanfovy);

    int radius = 0;
    float2 xy = make_float2(0.f, 0.f);
    float depth = 0.f;
    float cov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 co = make_float4(0.f, 0.f, 0.f, 0.f);
    float col[3] = {0.f, 0.f, 0.f};
    bool cl[3] = {false, false, false};

    const float p[3] = {means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]};
    float t[3];
    view_transform(cam.v, p, t);
    do {
        if (t[2] <= 0.2f) break;  // near-plane cull
        float4 q = *reinterpret_cast<const float4 *>(rotations + 4 * (size_t)i);
        float sc[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
        if (RAW) {
            float qnr, qn;
            q = quat_normalize(q, qnr, qn);
            sc[0] = expf(sc[0]);
            sc[1] = expf(sc[1]);
            sc[2] = expf(sc[2]);
        }
        const float s[3] = {scale_modifier * sc[0], scale_modifier * sc[1], scale_modifier * sc[2]};
        float S[3][3];
        cov3d_from_scale_rot(q, s, S);
        Geom2D g;
        if (!project_geometry<AA>(cam, tanfovx, tanfovy, fx, fy, W, H, gx, gy, p, t, S, g)) break;

        float shl[(DEG + 1) * (DEG + 1) * 3];
        const float *shp = shs + (size_t)i * M * 3;
        if (RAW) {
            shl[0] = shs[3 * (size_t)i];
            shl[1] = shs[3 * (size_t)i + 1];
            shl[2] = shs[3 * (size_t)i + 2];
            const float *rp = shs_rest + (size_t)i * (M - 1) * 3;
#pragma unroll
            for (int k = 3; k < (DEG + 1) * (DEG + 1) * 3; k++) shl[k] = rp[k - 3];
        } else if (DEG == 3 && M == 16) {
            const float4 *s4 = reinterpret_cast<const float4 *>(shp);
#pragma unroll
            for (int k = 0; k < 12; k++) {
                const float4 v = s4[k];
                shl[4 * k] = v.x;
                shl[4 * k + 1] = v.y;
                shl[4 * k + 2] = v.z;
                shl[4 * k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < (DEG + 1) * (DEG + 1) * 3; k++) shl[k] = shp[k];
        }
        shade<DEG>(cam.c, p, shl, col, cl);
        radius = g.rad;
        xy = g.xy;
        depth = t[2];
        cov[0] = S[0][0]; cov[1] = S[0][1]; cov[2] = S[0][2];
        cov[3] = S[1][1]; cov[4] = S[1][2]; cov[5] = S[2][2];
        co = make_float4(g.conic[0], g.conic[1], g.conic[2], RAW ? sigmoidf(opacities[i]) : opacities[i]);
        if (AA) co.w *= g.rho;
    } while (false);

    radii[i] = radius;
    means2D[i] = xy;
    depths[i] = depth;
    conic_opacity[i] = co;
#pragma unroll
    for (int k = 0; k < 6; k++) cov3D[6 * (size_t)i + k] = cov[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        rgb[3 * (size_t)i + k] = col[k];
        clamped[3 * (size_t)i + k] = cl[k] ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------ K11
// incoming gradients: dense [P,2] / [P,4] / [P,3] (gstride == 0, vector loads) or columns of rows that are
// `gstride` floats apart -- e.g. the [P,9] gradient record K10 accumulates into (no repacking pass in between)
__device__ __forceinline__ float2 grad_ld2(const float *__restrict__ p, size_t i, int gstride) {
    if (gstride == 0) return reinterpret_cast<const float2 *>(p)[i];
    const float *q = p + (size_t)gstride * i;
    return make_float2(q[0], q[1]);
}
__device__ __forceinline__ float4 grad_ld4(const float *__restrict__ p, size_t i, int gstride) {
    if (gstride == 0) return reinterpret_cast<const float4 *>(p)[i];
    const float *q = p + (size_t)gstride * i;
    return make_float4(q[0], q[1], q[2], q[3]);
}

constexpr int REST_W = 45;  // (16 - 1) * 3 floats of _features_rest per Gaussian
// workgroup size of K11 (one lane per Gaussian): the LDS stage below costs 180 B per lane whatever the size, so the
// resident waves per CU are the same; smaller workgroups interleave their load / compute / store phases more finely
#ifndef GSR_K11_BLOCK
#define GSR_K11_BLOCK 128
#endif
constexpr int K11_BLOCK = GSR_K11_BLOCK;
constexpr int K11_WAVES_PER_EU = 3;  // (hipcc's second launch bound is WAVES PER SIMD) 180 B of LDS per lane admit
                                     // 12 waves per CU whatever the block size: <= 168 registers
#ifndef GSR_K11_UN
#define GSR_K11_UN 4
#endif
// workgroup-cooperative, coalesced copy of the block's rows of a [P, 45] array into / out of LDS.  The way in is split
// in two: ISSUE loads the lane's twelve 16-byte pieces into registers (clamped indices, no branches: all twelve loads
// are in flight together -- a copy loop of load / wait / LDS-write iterations exposed the memory latency eleven times
// per workgroup, and three workgroups of four waves per CU cannot hide that), COMMIT writes them to LDS; the caller
// puts its own per-lane loads between the two.
constexpr int REST_SLOTS = (REST_W + 3) / 4;  // 16-byte pieces per lane: ceil(45 / 4) whatever the block size
struct RestStage {
    float4 v[REST_SLOTS];
};
__device__ __forceinline__ RestStage rest_stage_issue(const float *__restrict__ g, int P) {
    const size_t row0 = (size_t)blockIdx.x * K11_BLOCK;
    const int nw = (int)min((size_t)K11_BLOCK, (size_t)P - row0) * REST_W;
    const float4 *src4 = reinterpret_cast<const float4 *>(g + row0 * REST_W);  // 46080-byte blocks: 16-byte aligned
    const int n4 = nw / 4;  // >= 11
    RestStage st;
#pragma unroll
    for (int u = 0; u < REST_SLOTS; u++) st.v[u] = src4[min((int)threadIdx.x + u * K11_BLOCK, n4 - 1)];
    return st;
}
__device__ __forceinline__ void rest_stage_commit(float *__restrict__ s_rest, RestStage &st,
                                                  const float *__restrict__ g, int P) {
    const size_t row0 = (size_t)blockIdx.x * K11_BLOCK;
    const int nw = (int)min((size_t)K11_BLOCK, (size_t)P - row0) * REST_W;
    float4 *s4 = reinterpret_cast<float4 *>(s_rest);
    // the values are pinned in registers HERE (an empty asm that claims to modify them): without it the compiler sinks
    // every load into the conditional LDS write that uses it -- load, wait, write, twelve times in a row
#pragma unroll
    for (int u = 0; u < REST_SLOTS; u++)
        asm volatile("" : "+v"(st.v[u].x), "+v"(st.v[u].y), "+v"(st.v[u].z), "+v"(st.v[u].w));
#pragma unroll
    for (int u = 0; u < REST_SLOTS; u++) {
        const int k = (int)threadIdx.x + u * K11_BLOCK;
        if (k < nw / 4) s4[k] = st.v[u];
    }
    for (int k = (nw & ~3) + threadIdx.x; k < nw; k += K11_BLOCK) s_rest[k] = g[row0 * REST_W + k];
}
__device__ __forceinline__ void rest_stage_in(float *__restrict__ s_rest, const float *__restrict__ g, int P) {
    RestStage st = rest_stage_issue(g, P);
    rest_stage_commit(s_rest, st, g, P);
}
__device__ __forceinline__ void rest_stage_out(const float *__restrict__ s_rest, float *__restrict__ g, int P) {
    const size_t row0 = (size_t)blockIdx.x * K11_BLOCK;
    const int nw = (int)min((size_t)K11_BLOCK, (size_t)P - row0) * REST_W;
    float4 *dst4 = reinterpret_cast<float4 *>(g + row0 * REST_W);
    const float4 *s4 = reinterpret_cast<const float4 *>(s_rest);
    // streaming stores: this gradient (180 of the 236 gradient bytes per Gaussian) is read exactly once, by the
    // optimizer, and written with cacheable stores it evicts the PARAMETERS from the 256 MB memory-side cache -- which
    // the optimizer and the next iteration's K1 would otherwise hit (measured: Adam 0.253 -> 0.238 ms, K11 +0.004 ms)
    typedef float vf4 __attribute__((ext_vector_type(4)));
    for (int k = threadIdx.x; k < nw / 4; k += K11_BLOCK) {
        const float4 v = s4[k];
        __builtin_nontemporal_store(vf4{v.x, v.y, v.z, v.w}, reinterpret_cast<vf4 *>(dst4 + k));
    }
    for (int k = (nw & ~3) + threadIdx.x; k < nw; k += K11_BLOCK) g[row0 * REST_W + k] = s_rest[k];
}

// Fused K11 + Adam (ADAM = true): the six parameter gradients never reach HBM.  A Gaussian's gradient is complete
// when its lane leaves the camera loop (every band's contribution arrived through the exchange before the launch), so
// the dense Adam update of scene/gaussian_model.py:292's optimizer is applied right there: the 14 per-lane floats
// (xyz, scaling, rotation, features_dc, opacity) by the lane that owns them, the workgroup's 256 x 45 floats of
// _features_rest in the coalesced order of the LDS stage-out (the gradient is read from LDS instead of being
// streamed to HBM and back).  Saves the 236 B gradient write of K11, the 236 B gradient read and (through L2) most of
// the 236 B parameter read of the optimizer per Gaussian; the arithmetic is gsr_adam1's, bit for bit
// (tests/test_gpu_loss_and_step.py::test_fused_backward_step_equals_k11_then_adam).
// Tensor order: xyz, scaling, rotation, features_dc, features_rest, opacity.
struct K11Adam {
    float *m[6], *v[6];
    float lr_c[6], b1[6], b2[6], omb1[6], omb2[6], inv_sqrt_bc2[6], eps[6];
    float grad_scale;
    // hipGraph mode (gsr_preprocess_backward_adam_raw_batched_dyn): what changes from step to step is read from DEVICE
    // memory instead of the kernel arguments, so that one captured launch serves every replay --
    //   dyn[0..5] = lr / (1 - beta1^t), dyn[6..11] = 1 / sqrt(1 - beta2^t) per tensor (the host refreshes them with an
    //   asynchronous copy in front of the replay);  skip: a word that is non-zero when an earlier kernel of the SAME
    //   replay found a capacity exceeded (tile sort / exchange slab): the step then changes nothing and the host
    //   repeats the iteration eagerly.
    const float *dyn;
    const uint32_t *skip;
};
// the per-step constants of the captured launch (wave-uniform scalar loads, once per workgroup)
__device__ __forceinline__ K11Adam k11_adam_resolve(const K11Adam &in) {
    K11Adam ad = in;
    if (in.dyn) {
#pragma unroll
        for (int t = 0; t < 6; t++) {
            ad.lr_c[t] = in.dyn[t];
            ad.inv_sqrt_bc2[t] = in.dyn[6 + t];
        }
    }
    return ad;
}

// The 14 per-lane values (xyz 0-2, scaling 3-5, rotation 6-9, features_dc 10-12, opacity 13) are updated together at
// the END of the lane's work (the first version updated each tensor where its gradient fell out, five exposed moment
// latencies, and ran 0.50 ms against 0.355 ms for the two kernels it replaces), after the stage-out, when the
// _features_rest stage is free, with the moments of the five small tensors moved through LDS: every (tensor, moment)
// chunk of the workgroup -- K11_BLOCK rows of 12 / 16 / 4 bytes, contiguous -- is read and written as ONE 16-byte
// streaming access per lane, and a lane picks its 14 + 14 values out of LDS.  Per-lane 4-byte accesses to the moments
// (the version before this one) have to stay cacheable (a streaming load drops the line between a lane's pieces:
// +0.027 ms measured, streaming stores alone +0.010 ms), and 224 MB of cacheable moment traffic per 10^6 Gaussians
// pushes the PARAMETERS out of the 256 MB memory-side cache -- the next iteration's K1 then reads them from HBM
// (0.057 -> 0.075 ms).  Through LDS the moments stream past the cache like the optimizer kernel's.
__device__ __forceinline__ void k11_adam_small_lds(float *__restrict__ lds, const K11Adam &ad, int P, int i,
                                                   float *__restrict__ xyz, float *__restrict__ scaling,
                                                   float *__restrict__ rotation, float *__restrict__ f_dc,
                                                   float *__restrict__ opacity, const float (&pv)[14],
                                                   const float (&g)[14]) {
    constexpr int NT = 5;
    constexpr int TT[NT] = {0, 1, 2, 3, 5}, KK[NT] = {3, 3, 4, 3, 1}, OFF[NT] = {0, 3, 6, 10, 13};  // x K11_BLOCK words
    constexpr int MV = 14 * K11_BLOCK;  // words of one moment of the five tensors
    typedef float vf4 __attribute__((ext_vector_type(4)));
    const size_t row0 = (size_t)blockIdx.x * K11_BLOCK;
    const int rows = (int)min((size_t)K11_BLOCK, (size_t)P - row0);
    const int e4 = 4 * (int)threadIdx.x;
    // ---- in: one 16-byte piece per lane, tensor and moment -- ten independent loads, clamped instead of branched
    // around so that they stay together (a ragged last block takes the scalar loop)
    if (rows == K11_BLOCK) {
        vf4 in[NT][2];
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int mv = 0; mv < 2; mv++) {
                const float *src = (mv ? ad.v[TT[j]] : ad.m[TT[j]]) + row0 * KK[j];
                in[j][mv] = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(src + min(e4, K11_BLOCK * KK[j] - 4)));
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int mv = 0; mv < 2; mv++)
                if (e4 < K11_BLOCK * KK[j])
                    *reinterpret_cast<vf4 *>(lds + mv * MV + OFF[j] * K11_BLOCK + e4) = in[j][mv];
    } else {
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int mv = 0; mv < 2; mv++) {
                const float *src = (mv ? ad.v[TT[j]] : ad.m[TT[j]]) + row0 * KK[j];
                for (int e = threadIdx.x; e < rows * KK[j]; e += K11_BLOCK) lds[mv * MV + OFF[j] * K11_BLOCK + e] = src[e];
            }
    }
    __syncthreads();
    // ---- the lane's 14 values
    if (i < P) {
        constexpr int T[14] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 5};
        constexpr int J[14] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4};
        constexpr int C[14] = {0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 0};
        float *const base[6] = {xyz, scaling, rotation, f_dc, nullptr, opacity};
#pragma unroll
        for (int e = 0; e < 14; e++) {
            const int t = T[e], k = KK[J[e]];
            float *lm = lds + OFF[J[e]] * K11_BLOCK + (int)threadIdx.x * k + C[e];
            float p = pv[e], m = lm[0], v = lm[MV];
            gsr_adam1(p, __fmul_rn(g[e], ad.grad_scale), m, v, ad.lr_c[t], ad.b1[t], ad.b2[t], ad.omb1[t], ad.omb2[t],
                      ad.inv_sqrt_bc2[t], ad.eps[t]);
            base[t][(size_t)i * k + C[e]] = p;
            lm[0] = m;
            lm[MV] = v;
        }
    }
    __syncthreads();
    // ---- out
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
        for (int mv = 0; mv < 2; mv++) {
            float *dst = (mv ? ad.v[TT[j]] : ad.m[TT[j]]) + row0 * KK[j];
            if (rows == K11_BLOCK) {
                if (e4 < K11_BLOCK * KK[j])
                    __builtin_nontemporal_store(*reinterpret_cast<const vf4 *>(lds + mv * MV + OFF[j] * K11_BLOCK + e4),
                                                reinterpret_cast<vf4 *>(dst + e4));
            } else {
                for (int e = threadIdx.x; e < rows * KK[j]; e += K11_BLOCK) dst[e] = lds[mv * MV + OFF[j] * K11_BLOCK + e];
            }
        }
}

// the workgroup's rows of _features_rest: gradient from LDS, parameter (just staged in by this workgroup: L2) and
// both moments from HBM, 16 bytes per lane and access, FOUR accesses per lane in flight before the first is used
// (three workgroups of four waves per CU do not cover the memory latency with one).
__device__ __forceinline__ void rest_adam_out(const float *__restrict__ s_rest, float *__restrict__ param,
                                              const K11Adam &ad, int P) {
    constexpr int t = 4, UN = GSR_K11_UN;
    const size_t row0 = (size_t)blockIdx.x * K11_BLOCK;
    const int nw = (int)min((size_t)K11_BLOCK, (size_t)P - row0) * REST_W;
    typedef float vf4 __attribute__((ext_vector_type(4)));
    vf4 *p4 = reinterpret_cast<vf4 *>(param + row0 * REST_W);
    vf4 *m4 = reinterpret_cast<vf4 *>(ad.m[t] + row0 * REST_W);
    vf4 *v4 = reinterpret_cast<vf4 *>(ad.v[t] + row0 * REST_W);
    const float4 *s4 = reinterpret_cast<const float4 *>(s_rest);
    const float gs = ad.grad_scale, lr_c = ad.lr_c[t], b1 = ad.b1[t], b2 = ad.b2[t], omb1 = ad.omb1[t],
                omb2 = ad.omb2[t], isb = ad.inv_sqrt_bc2[t], eps = ad.eps[t];
    const int n4 = nw / 4;  // >= 11: a block holds at least one row of 45 words
    for (int k0 = threadIdx.x; k0 < n4; k0 += K11_BLOCK * UN) {
        vf4 pn[UN], mn[UN], vn[UN];
#pragma unroll
        for (int u = 0; u < UN; u++) {  // clamped, not branched around: the loads stay together
            const int k = min(k0 + u * K11_BLOCK, n4 - 1);
            pn[u] = p4[k];
            mn[u] = __builtin_nontemporal_load(m4 + k);
            vn[u] = __builtin_nontemporal_load(v4 + k);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const int k = k0 + u * K11_BLOCK;
            if (k < n4) {
                const float4 g = s4[k];
                float pa[4] = {pn[u].x, pn[u].y, pn[u].z, pn[u].w}, ma[4] = {mn[u].x, mn[u].y, mn[u].z, mn[u].w},
                      va[4] = {vn[u].x, vn[u].y, vn[u].z, vn[u].w};
                const float ga[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int c = 0; c < 4; c++)
                    gsr_adam1(pa[c], __fmul_rn(ga[c], gs), ma[c], va[c], lr_c, b1, b2, omb1, omb2, isb, eps);
                p4[k] = vf4{pa[0], pa[1], pa[2], pa[3]};
                __builtin_nontemporal_store(vf4{ma[0], ma[1], ma[2], ma[3]}, m4 + k);
                __builtin_nontemporal_store(vf4{va[0], va[1], va[2], va[3]}, v4 + k);
            }
        }
    }
    for (int k = (nw & ~3) + threadIdx.x; k < nw; k += K11_BLOCK) {
        const size_t o = row0 * REST_W + k;
        float p = param[o], m = ad.m[t][o], v = ad.v[t][o];
        gsr_adam1(p, __fmul_rn(s_rest[k], gs), m, v, lr_c, b1, b2, omb1, omb2, isb, eps);
        param[o] = p;
        ad.m[t][o] = m;
        ad.v[t][o] = v;
    }
}

// Everything one lane reads from HBM in the one-camera K11 besides its _features_rest row, loaded TOGETHER at the top of
// the kernel (unconditionally: an invisible Gaussian costs its ~130 bytes of reads): the body used to fetch each piece
// where it was first needed -- radius, then position and conic gradient, then the covariance, ... -- six dependent
// waits per lane in a kernel whose occupancy (46 KB of LDS per workgroup) cannot hide them.
struct K11In {
    int32_t rad;
    float p[3], sc[3], dc[3], op;
    float4 q;
    float cv[6];
    float4 gco;
    float2 g2;
    float grgb[3];
    uint8_t cl[3];
};
// (AA with activated inputs: `opacities_raw` is the activated opacity, which the factor's gradient needs)
template <bool RAW, bool AA = false>
__device__ __forceinline__ K11In k11_load(size_t i, const float *__restrict__ means3D, const float *__restrict__ scales,
                                          const float *__restrict__ rotations, const float *__restrict__ shs,
                                          const float *__restrict__ opacities_raw, const int32_t *__restrict__ radii,
                                          const float *__restrict__ cov3D, const uint8_t *__restrict__ clamped,
                                          const float *__restrict__ dL_dmeans2D,
                                          const float *__restrict__ dL_dconic_opacity,
                                          const float *__restrict__ dL_drgb, int gstride) {
    K11In in;
    in.rad = radii[i];
#pragma unroll
    for (int e = 0; e < 3; e++) {
        in.p[e] = means3D[3 * i + e];
        in.sc[e] = scales[3 * i + e];
        in.dc[e] = RAW ? shs[3 * i + e] : 0.f;
        in.cl[e] = clamped[3 * i + e];
        in.grgb[e] = dL_drgb[(gstride ? gstride : 3) * i + e];
    }
    in.op = (RAW || AA) ? opacities_raw[i] : 0.f;
    in.q = *reinterpret_cast<const float4 *>(rotations + 4 * i);
#pragma unroll
    for (int e = 0; e < 6; e++) in.cv[e] = cov3D[6 * i + e];
    in.gco = grad_ld4(dL_dconic_opacity, i, gstride);
    in.g2 = grad_ld2(dL_dmeans2D, i, gstride);
    return in;
}

// Where the fused dense kernels (K11 + Adam, one camera and camera-batched) take the incoming gradient from.
// GradRecord: fp32 gradients, dense or columns of a record (grad_ld2 above) -- what every other K11 kernel reads; the
// record kernels keep the three pointers and the stride as arguments of their own, the struct only bundles them on the host.
// GradSums: K10's own [P,9] fp64 sums and [P] row flags of each camera (gsr_render_backward_sums), before anything has
// rounded them into a record.  A lane converts the nine doubles of a flagged row with one (float) each, in the record's
// column order (means2D 0:2, rgb 2:5, conic_opacity 5:9): the bits record_from_f64_touched_kernel would have stored.
// A row whose flag is clear received nothing: its record row would be the forward's zeros, so it takes the kernels'
// zero-gradient path as a culled row does, and neither its sums nor its cov3D / clamp flags are read.
struct GradRecord {
    const float *means2D, *conic_opacity, *rgb;
    int gstride;
};
constexpr int K11_SUMS_CAMS = 8;  // cameras one GradSums launch takes (the tables travel in the kernel arguments)
struct GradSums {
    const double *acc[K11_SUMS_CAMS];
    const uint8_t *flags[K11_SUMS_CAMS];
};
#ifndef GSR_K11_SUMS_COV_ALWAYS
#define GSR_K11_SUMS_COV_ALWAYS 0  // 1 (A/B): cov3D and the clamp flags are loaded for every row, only the sums wait
#endif

// k11_load with GradSums.  `rad` and `flag` are the lane's radius and row flag, which the caller requested FIRST: they
// decide the loads at the bottom, and the wait for them leaves every other load of the lane in flight.
__device__ __forceinline__ K11In k11_load_sums(size_t i, int32_t rad, uint8_t flag, const float *__restrict__ xyz,
                                               const float *__restrict__ scaling, const float *__restrict__ rotation,
                                               const float *__restrict__ f_dc, const float *__restrict__ opacity,
                                               const float *__restrict__ cov3D, const uint8_t *__restrict__ clamped,
                                               const double *__restrict__ acc) {
    K11In in;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        in.p[e] = xyz[3 * i + e];
        in.sc[e] = scaling[3 * i + e];
        in.dc[e] = f_dc[3 * i + e];
        in.cl[e] = GSR_K11_SUMS_COV_ALWAYS ? clamped[3 * i + e] : (uint8_t)0;
        in.grgb[e] = 0.f;
    }
    in.op = opacity[i];
    in.q = *reinterpret_cast<const float4 *>(rotation + 4 * i);
#pragma unroll
    for (int e = 0; e < 6; e++) in.cv[e] = GSR_K11_SUMS_COV_ALWAYS ? cov3D[6 * i + e] : 0.f;
    in.gco = make_float4(0.f, 0.f, 0.f, 0.f);
    in.g2 = make_float2(0.f, 0.f);
    __builtin_amdgcn_sched_barrier(0);  // the loads above are issued before the flag is waited for
    const bool live = flag && rad > 0;
    in.rad = live ? rad : 0;
    if (live) {
        const double *a = acc + 9 * i;
        double v[9];
#pragma unroll
        for (int k = 0; k < 9; k++) v[k] = a[k];
        if (!GSR_K11_SUMS_COV_ALWAYS) {
#pragma unroll
            for (int e = 0; e < 6; e++) in.cv[e] = cov3D[6 * i + e];
#pragma unroll
            for (int e = 0; e < 3; e++) in.cl[e] = clamped[3 * i + e];
        }
        in.g2 = make_float2((float)v[0], (float)v[1]);
#pragma unroll
        for (int e = 0; e < 3; e++) in.grgb[e] = (float)v[2 + e];
        in.gco = make_float4((float)v[5], (float)v[6], (float)v[7], (float)v[8]);
    }
    return in;
}

// dL/dopacity of one row from g = the summed dL/dconic_opacity.w (AA: each camera's times its rho): through the sigmoid
// for the raw forms, into the fused step's slot 13 or to HBM
template <bool RAW, bool ADAM>
__device__ __forceinline__ void k11_opacity_out(float op, float g, const int i, float (&sp)[14], float (&sg)[14],
                                                float *__restrict__ dL_dopacities) {
    if (ADAM) {
        const float so = sigmoidf(op);
        sp[13] = op;
        sg[13] = g * so * (1.0f - so);
    } else if (RAW) {
        const float so = sigmoidf(op);
        dL_dopacities[i] = g * so * (1.0f - so);
    } else {
        dL_dopacities[i] = g;
    }
}

template <int DEG, bool RAW, bool ADAM = false, bool AA = false>
__device__ __forceinline__ void
preprocess_backward_body(const K11In &in, float (&sp)[14], float (&sg)[14], const int i,
                         const float *__restrict__ rest_in, float *__restrict__ rest_out, int M, float scale_modifier,
                         const float *__restrict__ shs, const float *__restrict__ view, const float *__restrict__ proj,
                         const float *__restrict__ campos, int W, int H, float tanfovx, float tanfovy,
                         float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dscales,
                         float4 *__restrict__ dL_drotations, float *__restrict__ dL_dshs,
                         float *__restrict__ dL_dopacities) {
    constexpr int NC = (DEG + 1) * (DEG + 1);
    float *dsh_out = dL_dshs + (size_t)i * M * 3;

    if (ADAM && in.rad <= 0) {  // invisible: zero gradient, the moments still decay and still move the parameter
#pragma unroll
        for (int e = 0; e < 3; e++) {
            sp[e] = in.p[e];
            sp[3 + e] = in.sc[e];
            sp[10 + e] = in.dc[e];
        }
        sp[6] = in.q.x; sp[7] = in.q.y; sp[8] = in.q.z; sp[9] = in.q.w;
        sp[13] = in.op;
#pragma unroll
        for (int e = 0; e < 14; e++) sg[e] = 0.f;
        float *rp = rest_out;
        for (int k = 0; k < (M - 1) * 3; k++) rp[k] = 0.f;
        return;
    }
    if (RAW && in.rad <= 0) {
        dL_dmeans3D[3 * (size_t)i] = dL_dmeans3D[3 * (size_t)i + 1] = dL_dmeans3D[3 * (size_t)i + 2] = 0.f;
        dL_dscales[3 * (size_t)i] = dL_dscales[3 * (size_t)i + 1] = dL_dscales[3 * (size_t)i + 2] = 0.f;
        dL_drotations[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        dL_dopacities[i] = 0.f;
        dL_dshs[3 * (size_t)i] = dL_dshs[3 * (size_t)i + 1] = dL_dshs[3 * (size_t)i + 2] = 0.f;
        float *rp = rest_out;
        for (int k = 0; k < (M - 1) * 3; k++) rp[k] = 0.f;
        return;
    }
    if (in.rad <= 0) {
        dL_dmeans3D[3 * (size_t)i] = dL_dmeans3D[3 * (size_t)i + 1] = dL_dmeans3D[3 * (size_t)i + 2] = 0.f;
        dL_dscales[3 * (size_t)i] = dL_dscales[3 * (size_t)i + 1] = dL_dscales[3 * (size_t)i + 2] = 0.f;
        dL_drotations[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        dL_dopacities[i] = 0.f;
        for (int k = 0; k < M * 3; k++) dsh_out[k] = 0.f;
        return;
    }
    const Cam cam = load_cam(view, proj, campos);
    const float fx = W / (2.0f * tanfovx), fy = H / (2.0f * tanfovy);
    const float p[3] = {in.p[0], in.p[1], in.p[2]};
    const float4 gco = in.gco;
    const float gA = gco.x, gB = gco.y, gC = gco.z;
    if (!AA) k11_opacity_out<RAW, ADAM>(in.op, gco.w, i, sp, sg, dL_dopacities);

    // ---- conic -> cov2D -> (cov3D, t)
    float S[3][3];
    cov3d_unpack(in.cv, S);
    const Cov2DGrad cg = cov2d_backward<AA>(cam.v, fx, fy, tanfovx, tanfovy, p, S, gA, gB, gC,
                                            AA ? gco.w * (RAW ? sigmoidf(in.op) : in.op) : 0.f);
    if (AA) k11_opacity_out<RAW, ADAM>(in.op, gco.w * cg.rho, i, sp, sg, dL_dopacities);
    float dmean[3];
#pragma unroll
    for (int k = 0; k < 3; k++) dmean[k] = cg.dmean[k];

    // ---- means2D (NDC-scaled) -> mean through the perspective divide
    {
        float dm[3];
        means2d_to_mean(cam.p, p, in.g2, dm);
#pragma unroll
        for (int k = 0; k < 3; k++) dmean[k] += dm[k];
    }

    // ---- colour -> SH coefficients and view direction
    {
        float sh[NC * 3];
        if (RAW) {
            sh[0] = in.dc[0];
            sh[1] = in.dc[1];
            sh[2] = in.dc[2];
            const float *rp = rest_in;
#pragma unroll
            for (int k = 3; k < NC * 3; k++) sh[k] = rp[k - 3];
        } else {
            const float *sp = shs + (size_t)i * M * 3;
#pragma unroll
            for (int k = 0; k < NC * 3; k++) sh[k] = sp[k];
        }
        const float g3[3] = {in.cl[0] ? 0.f : in.grgb[0], in.cl[1] ? 0.f : in.grgb[1], in.cl[2] ? 0.f : in.grgb[2]};
        float dsh[NC * 3], dm[3];
        viewdir_backward<DEG>(cam.c, p, ShRegs{sh}, g3, DshAssign{dsh}, dm);
        dmean[0] += dm[0];
        dmean[1] += dm[1];
        dmean[2] += dm[2];
        if (RAW) {
            if (ADAM) {
#pragma unroll
                for (int e = 0; e < 3; e++) {
                    sp[10 + e] = sh[e];
                    sg[10 + e] = dsh[e];
                }
            } else {
                dL_dshs[3 * (size_t)i] = dsh[0];
                dL_dshs[3 * (size_t)i + 1] = dsh[1];
                dL_dshs[3 * (size_t)i + 2] = dsh[2];
            }
            float *rp = rest_out;
#pragma unroll
            for (int k = 3; k < NC * 3; k++) rp[k - 3] = dsh[k];
            for (int k = NC * 3; k < M * 3; k++) rp[k - 3] = 0.f;
        } else if (DEG == 3 && M == 16) {
            float4 *o4 = reinterpret_cast<float4 *>(dsh_out);
#pragma unroll
            for (int k = 0; k < 12; k++) o4[k] = make_float4(dsh[4 * k], dsh[4 * k + 1], dsh[4 * k + 2], dsh[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < NC * 3; k++) dsh_out[k] = dsh[k];
            for (int k = NC * 3; k < M * 3; k++) dsh_out[k] = 0.f;
        }
    }
    if (ADAM) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
            sp[e] = p[e];
            sg[e] = dmean[e];
        }
    } else {
        dL_dmeans3D[3 * (size_t)i] = dmean[0];
        dL_dmeans3D[3 * (size_t)i + 1] = dmean[1];
        dL_dmeans3D[3 * (size_t)i + 2] = dmean[2];
    }

    // ---- cov3D -> scales, rotations
    {
        float gsc[3];
        float4 dq;
        cov3d_backward<RAW>(in.q, in.sc, scale_modifier, cg.dcov, gsc, dq);
        if (ADAM) {
#pragma unroll
            for (int e = 0; e < 3; e++) {
                sp[3 + e] = in.sc[e];
                sg[3 + e] = gsc[e];
            }
            sp[6] = in.q.x; sp[7] = in.q.y; sp[8] = in.q.z; sp[9] = in.q.w;
            sg[6] = dq.x; sg[7] = dq.y; sg[8] = dq.z; sg[9] = dq.w;
        } else {
#pragma unroll
            for (int r = 0; r < 3; r++) dL_dscales[3 * (size_t)i + r] = gsc[r];
            dL_drotations[i] = dq;
        }
    }
}

// K11 kernel: with the raw parameter layout and 16 SH coefficients the workgroup's 256 x 45 floats of
// _features_rest (and of its gradient) are contiguous in HBM; per-lane rows are 180 bytes apart, so reading them
// lane by lane touches a different cache line in every lane of every load.  They are staged through LDS with
// coalesced 16-byte accesses instead (row stride 45 words: conflict-free), both ways.
template <int DEG, bool RAW, bool AA>
__global__ void __launch_bounds__(K11_BLOCK, K11_WAVES_PER_EU)
preprocess_backward_kernel(int P, int M, const float *__restrict__ means3D, const float *__restrict__ scales,
                           float scale_modifier, const float *__restrict__ rotations, const float *__restrict__ shs,
                           const float *__restrict__ shs_rest, const float *__restrict__ opacities_raw,
                           const float *__restrict__ view, const float *__restrict__ proj,
                           const float *__restrict__ campos, int W, int H, float tanfovx, float tanfovy,
                           const int32_t *__restrict__ radii, const float *__restrict__ cov3D,
                           const uint8_t *__restrict__ clamped, const float *__restrict__ dL_dmeans2D,
                           const float *__restrict__ dL_dconic_opacity, const float *__restrict__ dL_drgb, int gstride,
                           float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dscales,
                           float4 *__restrict__ dL_drotations, float *__restrict__ dL_dshs,
                           float *__restrict__ dL_dshs_rest, float *__restrict__ dL_dopacities) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float ad[14], ad2[14];  // (the fused kernel's per-lane parameter / gradient slots: unused here)
    const size_t ic = (size_t)min(i, P - 1);  // lanes past the end load the last Gaussian's inputs and compute nothing
    if constexpr (RAW) {
        __shared__ float s_rest[K11_BLOCK * REST_W];
        if (M == 16) {  // block-uniform
            RestStage st = rest_stage_issue(shs_rest, P);
            const K11In in = k11_load<RAW, AA>(ic, means3D, scales, rotations, shs, opacities_raw, radii, cov3D, clamped,
                                               dL_dmeans2D, dL_dconic_opacity, dL_drgb, gstride);
            __builtin_amdgcn_sched_barrier(0);  // every load of the lane is issued before the first result is used
            rest_stage_commit(s_rest, st, shs_rest, P);
            __syncthreads();
            if (i < P)
                preprocess_backward_body<DEG, RAW, false, AA>(in, ad, ad2, i, s_rest + threadIdx.x * REST_W,
                                                              s_rest + threadIdx.x * REST_W, M, scale_modifier, shs,
                                                              view, proj, campos, W, H, tanfovx, tanfovy, dL_dmeans3D,
                                                              dL_dscales, dL_drotations, dL_dshs, dL_dopacities);
            __syncthreads();
            rest_stage_out(s_rest, dL_dshs_rest, P);
            return;
        }
    }
    if (i >= P) return;
    const K11In in = k11_load<RAW, AA>(ic, means3D, scales, rotations, shs, opacities_raw, radii, cov3D, clamped,
                                       dL_dmeans2D, dL_dconic_opacity, dL_drgb, gstride);
    preprocess_backward_body<DEG, RAW, false, AA>(in, ad, ad2, i, RAW ? shs_rest + (size_t)i * (M - 1) * 3 : nullptr,
                                                  RAW ? dL_dshs_rest + (size_t)i * (M - 1) * 3 : nullptr, M,
                                                  scale_modifier, shs, view, proj, campos, W, H, tanfovx, tanfovy,
                                                  dL_dmeans3D, dL_dscales, dL_drotations, dL_dshs, dL_dopacities);
}

// K11 + Adam, one camera, 16-coefficient model (the launcher checks): the same body with the stores replaced by the
// optimizer update (K11Adam above).  Own kernel name so that traces and counters tell the fused launch apart.
// GRAD: GradNone -- the gradients are the three fp32 pointers and their row stride (preprocess_backward_adam_kernel) --
// or GradSums (preprocess_backward_adam_sums_kernel: the row's flag and radius are requested first, k11_load_sums).
struct GradNone {};
template <int DEG, bool AA, typename GRAD>
__device__ __forceinline__ void
preprocess_backward_adam_body(int P, float *__restrict__ xyz, float *__restrict__ scaling, float scale_modifier,
                              float *__restrict__ rotation, float *__restrict__ f_dc, float *__restrict__ f_rest,
                              float *__restrict__ opacity, const float *__restrict__ view,
                              const float *__restrict__ proj, const float *__restrict__ campos, int W, int H,
                              float tanfovx, float tanfovy, const int32_t *__restrict__ radii,
                              const float *__restrict__ cov3D, const uint8_t *__restrict__ clamped,
                              const float *__restrict__ dL_dmeans2D, const float *__restrict__ dL_dconic_opacity,
                              const float *__restrict__ dL_drgb, int gstride, const GRAD &sums, const K11Adam &ad_in) {
    if (ad_in.skip && *ad_in.skip) return;  // wave-uniform: a capacity overflowed earlier in this replay
    const K11Adam ad = k11_adam_resolve(ad_in);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ float s_rest[K11_BLOCK * REST_W];
    const size_t ic = (size_t)min(i, P - 1);
    int32_t rad = 0;
    uint8_t flag = 0;
    if constexpr (std::is_same<GRAD, GradSums>::value) {
        rad = radii[ic];
        flag = sums.flags[0][ic];
    }
    RestStage st = rest_stage_issue(f_rest, P);
    K11In in;
    if constexpr (std::is_same<GRAD, GradSums>::value)
        in = k11_load_sums(ic, rad, flag, xyz, scaling, rotation, f_dc, opacity, cov3D, clamped, sums.acc[0]);
    else
        in = k11_load<true>(ic, xyz, scaling, rotation, f_dc, opacity, radii, cov3D, clamped, dL_dmeans2D,
                            dL_dconic_opacity, dL_drgb, gstride);
    __builtin_amdgcn_sched_barrier(0);  // every load of the lane is issued before the first result is used
    rest_stage_commit(s_rest, st, f_rest, P);
    __syncthreads();
    float sp[14], sg[14];
    if (i < P)
        preprocess_backward_body<DEG, true, true, AA>(in, sp, sg, i, s_rest + threadIdx.x * REST_W,
                                                      s_rest + threadIdx.x * REST_W, 16, scale_modifier, f_dc, view,
                                                      proj, campos, W, H, tanfovx, tanfovy, nullptr, nullptr, nullptr,
                                                      nullptr, nullptr);
    __syncthreads();
    rest_adam_out(s_rest, f_rest, ad, P);
    __syncthreads();  // the stage is free: the moments of the small tensors go through it
    k11_adam_small_lds(s_rest, ad, P, i, xyz, scaling, rotation, f_dc, opacity, sp, sg);
}
template <int DEG, bool AA>
__global__ void __launch_bounds__(K11_BLOCK, K11_WAVES_PER_EU)
preprocess_backward_adam_kernel(int P, float *__restrict__ xyz, float *__restrict__ scaling, float scale_modifier,
                                float *__restrict__ rotation, float *__restrict__ f_dc, float *__restrict__ f_rest,
                                float *__restrict__ opacity, const float *__restrict__ view,
                                const float *__restrict__ proj, const float *__restrict__ campos, int W, int H,
                                float tanfovx, float tanfovy, const int32_t *__restrict__ radii,
                                const float *__restrict__ cov3D, const uint8_t *__restrict__ clamped,
                                const float *__restrict__ dL_dmeans2D, const float *__restrict__ dL_dconic_opacity,
                                const float *__restrict__ dL_drgb, int gstride, const K11Adam ad_in) {
    preprocess_backward_adam_body<DEG, AA>(P, xyz, scaling, scale_modifier, rotation, f_dc, f_rest, opacity, view, proj,
                                           campos, W, H, tanfovx, tanfovy, radii, cov3D, clamped, dL_dmeans2D,
                                           dL_dconic_opacity, dL_drgb, gstride, GradNone{}, ad_in);
}
template <int DEG, bool AA>
__global__ void __launch_bounds__(K11_BLOCK, K11_WAVES_PER_EU)
preprocess_backward_adam_sums_kernel(int P, float *__restrict__ xyz, float *__restrict__ scaling, float scale_modifier,
                                     float *__restrict__ rotation, float *__restrict__ f_dc,
                                     float *__restrict__ f_rest, float *__restrict__ opacity,
                                     const float *__restrict__ view, const float *__restrict__ proj,
                                     const float *__restrict__ campos, int W, int H, float tanfovx, float tanfovy,
                                     const int32_t *__restrict__ radii, const float *__restrict__ cov3D,
                                     const uint8_t *__restrict__ clamped, const GradSums sums, const K11Adam ad_in) {
    preprocess_backward_adam_body<DEG, AA>(P, xyz, scaling, scale_modifier, rotation, f_dc, f_rest, opacity, view, proj,
                                           campos, W, H, tanfovx, tanfovy, radii, cov3D, clamped, nullptr, nullptr,
                                           nullptr, 0, sums, ad_in);
}

// ------------------------------------------------------------------------- K1 / K11, batched over cameras
// A batch of B cameras (Grendel's --bsz B; every rank projects ITS Gaussians for ALL cameras of the batch,
// gaussian_renderer/__init__.py:919-963) in ONE launch each way: a lane reads its Gaussian's 59 raw floats
// once, loops over the cameras (40 floats each, wave-uniform -> scalar loads) and, in the backward, sums the
// cameras' gradients in registers before the single store.  HBM traffic 236 + B*44 forward and
// 236 + B*79 + 236 backward per Gaussian instead of B*(236+44) and B*552, and 2 launches instead of 2B.
// cams[b] = { view[16], proj[16], campos[3], tanfovx, tanfovy, pad[3] }.
constexpr int CAM_STRIDE = 40;

__device__ __forceinline__ Cam load_cam_packed(const float *__restrict__ c) {
    Cam cam;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        cam.v[i] = c[i];
        cam.p[i] = c[16 + i];
    }
    cam.c[0] = c[32];
    cam.c[1] = c[33];
    cam.c[2] = c[34];
    return cam;
}

template <int DEG, bool AA>
__global__ void __launch_bounds__(GSR_ONE_DIM_BLOCK)
preprocess_forward_batched_kernel(int P, int B, int M, const float *__restrict__ xyz, const float *__restrict__ scaling,
                                  float scale_modifier, const float *__restrict__ rotation,
                                  const float *__restrict__ f_dc, const float *__restrict__ f_rest,
                                  const float *__restrict__ opacity, const float *__restrict__ cams, int W, int H,
                                  float2 *__restrict__ means2D, float *__restrict__ depths,
                                  int32_t *__restrict__ radii, float *__restrict__ cov3D,
                                  float4 *__restrict__ conic_opacity, float *__restrict__ rgb,
                                  uint8_t *__restrict__ clamped) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int NC = (DEG + 1) * (DEG + 1);
    if (i >= P) return;
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    // ---- camera-independent part, once
    const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    float qnr, qn;
    const float4 q = quat_normalize(*reinterpret_cast<const float4 *>(rotation + 4 * (size_t)i), qnr, qn);
    const float s[3] = {scale_modifier * expf(scaling[3 * (size_t)i]), scale_modifier * expf(scaling[3 * (size_t)i + 1]),
                        scale_modifier * expf(scaling[3 * (size_t)i + 2])};
    const float op = sigmoidf(opacity[i]);
    float S[3][3];
    cov3d_from_scale_rot(q, s, S);
    cov3D[6 * (size_t)i + 0] = S[0][0]; cov3D[6 * (size_t)i + 1] = S[0][1]; cov3D[6 * (size_t)i + 2] = S[0][2];
    cov3D[6 * (size_t)i + 3] = S[1][1]; cov3D[6 * (size_t)i + 4] = S[1][2]; cov3D[6 * (size_t)i + 5] = S[2][2];
    float shl[NC * 3];
    shl[0] = f_dc[3 * (size_t)i];
    shl[1] = f_dc[3 * (size_t)i + 1];
    shl[2] = f_dc[3 * (size_t)i + 2];
    {
        // (staging these 180-byte rows through LDS as K11 does does not pay here: with a copy loop 78 -> 96 us in round 2,
        // with K11's issue / commit split and 128-lane workgroups 60.5 -> 60.0 us at 10^6 and 342 -> 343 us at 6 10^6
        // Gaussians in round 3 -- the forward has the occupancy to hide the strided rows)
        const float *rp = f_rest + (size_t)i * (M - 1) * 3;
#pragma unroll
        for (int k = 3; k < NC * 3; k++) shl[k] = rp[k - 3];
    }
    // ---- per camera
    for (int bc = 0; bc < B; bc++) {
        const float *cp = cams + (size_t)bc * CAM_STRIDE;
        const Cam cam = load_cam_packed(cp);
        const float tanfovx = cp[35], tanfovy = cp[36];
        const float fx = W / (2.0f * tanfovx), fy = H / (2.0f * tanfovy);
        int radius = 0;
        float2 xy = make_float2(0.f, 0.f);
        float depth = 0.f;
        float4 co = make_float4(0.f, 0.f, 0.f, 0.f);
        float col[3] = {0.f, 0.f, 0.f};
        bool cl[3] = {false, false, false};
        float t[3];
        view_transform(cam.v, p, t);
        do {
            if (t[2] <= 0.2f) break;  // near-plane cull
            Geom2D g;
            if (!project_geometry<AA>(cam, tanfovx, tanfovy, fx, fy, W, H, gx, gy, p, t, S, g)) break;
            shade<DEG>(cam.c, p, shl, col, cl);
            radius = g.rad;
            xy = g.xy;
            depth = t[2];
            co = make_float4(g.conic[0], g.conic[1], g.conic[2], AA ? op * g.rho : op);
        } while (false);
        const size_t o = (size_t)bc * P + i;
        radii[o] = radius;
        means2D[o] = xy;
        depths[o] = depth;
        conic_opacity[o] = co;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            rgb[3 * o + k] = col[k];
            clamped[3 * o + k] = cl[k] ? 1 : 0;
        }
    }
}

// What one lane reads per CAMERA in the batched K11: radius, the nine floats of the camera's [P,9] gradient record row and the
// three clamp flags.  Round 6: the loop used to fetch them where they were first needed -- radius, branch, conic gradient,
// ..., position gradient, colour gradient: three dependent trips to memory per camera in a kernel that holds two waves per
// SIMD -- and ran at 0.47 of the HBM peak at four cameras against 0.78 for the one-camera kernel.  Now a queue of
// K11_CAMQ cameras is always in flight: the first ones are requested at the top of the kernel together with the
// Gaussian's own 59 floats and the _features_rest block, camera c + K11_CAMQ while camera c is being differentiated.
#ifndef GSR_K11_CAMQ
#define GSR_K11_CAMQ 2
#endif
constexpr int K11_CAMQ = GSR_K11_CAMQ;
#ifndef GSR_K11B_WAVES
#define GSR_K11B_WAVES 2
#endif
constexpr int K11B_WAVES_PER_EU = GSR_K11B_WAVES;  // waves per SIMD the camera-batched K11 kernels are compiled for
struct K11CamSH {  // the colour part's share
    int32_t rad;
    float grgb[3];
    uint8_t cl[3];
};
struct K11CamGeo {  // the geometry part's share
    int32_t rad;
    float4 gco;
    float2 g2;
};
__device__ __forceinline__ K11CamSH k11_cam_load_sh(size_t o, const int32_t *__restrict__ radii,
                                                    const uint8_t *__restrict__ clamped,
                                                    const float *__restrict__ dL_drgb, int gstride) {
    K11CamSH c;
    c.rad = radii[o];
#pragma unroll
    for (int e = 0; e < 3; e++) {
        c.grgb[e] = dL_drgb[(gstride ? gstride : 3) * o + e];
        c.cl[e] = clamped[3 * o + e];
    }
    return c;
}
__device__ __forceinline__ K11CamGeo k11_cam_load_geo(size_t o, const int32_t *__restrict__ radii,
                                                      const float *__restrict__ dL_dmeans2D,
                                                      const float *__restrict__ dL_dconic_opacity, int gstride) {
    K11CamGeo c;
    c.rad = radii[o];
    c.gco = grad_ld4(dL_dconic_opacity, o, gstride);
    c.g2 = grad_ld2(dL_dmeans2D, o, gstride);
    return c;
}
// The same two with GradSums: `live` = the camera's flag of the row is set and the row is visible there (the body reads
// every camera's flag and radius once, at the top); o = camera * P + row as above, a = the camera's sums of the row.
// A camera that is not live loads nothing and comes back with radius 0: the loops skip it.
__device__ __forceinline__ K11CamSH k11_cam_load_sh_sums(size_t o, bool live, const uint8_t *__restrict__ clamped,
                                                         const double *__restrict__ a) {
    K11CamSH c;
    c.rad = live ? 1 : 0;
#pragma unroll
    for (int e = 0; e < 3; e++) {
        c.grgb[e] = 0.f;
        c.cl[e] = 0;
    }
    if (live) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
            c.grgb[e] = (float)a[2 + e];
            c.cl[e] = clamped[3 * o + e];
        }
    }
    return c;
}
__device__ __forceinline__ K11CamGeo k11_cam_load_geo_sums(bool live, const double *__restrict__ a) {
    K11CamGeo c;
    c.rad = live ? 1 : 0;
    c.gco = make_float4(0.f, 0.f, 0.f, 0.f);
    c.g2 = make_float2(0.f, 0.f);
    if (live) {
        c.g2 = make_float2((float)a[0], (float)a[1]);
        c.gco = make_float4((float)a[5], (float)a[6], (float)a[7], (float)a[8]);
    }
    return c;
}

// Where the lanes of the camera-batched body find their rows.  DenseRows: lane i of the grid owns row i, a workgroup's
// rows are contiguous (the LDS stage moves them in 16-byte pieces).  ListRows (the sparse update, ADAM and 16
// coefficients only): lane e of workgroup c owns row list[c * K11_BLOCK + e] where that is below count, and the caller
// has sent home the workgroups with c * K11_BLOCK >= count; the rows lie anywhere, so the stage and the moments are
// gathered word by word through the row table in LDS with the three device functions below.  Everything between
// stage-in and update -- both camera loops, the SH gradient over the stage, the 14 slots -- is one text for both
// (DESIGN.md 3.3 on why it is a parameter of the body and not a set of shared helpers).
struct DenseRows {};
struct ListRows {
    const uint32_t *list;
    uint32_t count;
};
constexpr int SA_UN = 5;  // words per lane in flight in the gathered stage's copies: 45 = 9 x 5
// word e of the workgroup's K11_BLOCK x 45 stage -> its offset in a [P, 45] array, through the row list in LDS
__device__ __forceinline__ size_t sa_rest_offset(const uint32_t *__restrict__ s_rows, int e) {
    const int r = e / REST_W;
    return (size_t)s_rows[r] * REST_W + (size_t)(e - r * REST_W);
}
// the listed rows' SH coefficients above DC into the stage (nw: words of the workgroup's rows)
__device__ __forceinline__ void sa_rest_stage_in(float *__restrict__ s_rest, const uint32_t *__restrict__ s_rows,
                                                 const float *__restrict__ f_rest, int nw) {
    for (int k0 = 0; k0 < REST_W; k0 += SA_UN) {
        float v[SA_UN];
#pragma unroll
        for (int u = 0; u < SA_UN; u++)
            v[u] = f_rest[sa_rest_offset(s_rows, min((k0 + u) * K11_BLOCK + (int)threadIdx.x, nw - 1))];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < SA_UN; u++) {
            const int e = (k0 + u) * K11_BLOCK + (int)threadIdx.x;
            if (e < nw) s_rest[e] = v[u];
        }
    }
}
// the 14 per-lane values of row ic: a gathered row's moments are 12 / 16 / 4 bytes here and there, read by the lane
__device__ __forceinline__ void sa_adam_small(const K11Adam &ad, size_t ic, float *__restrict__ xyz,
                                              float *__restrict__ scaling, float *__restrict__ rotation,
                                              float *__restrict__ f_dc, float *__restrict__ opacity,
                                              const float (&sp)[14], const float (&sg)[14]) {
    constexpr int T[14] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 5};
    constexpr int KK[14] = {3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 3, 3, 3, 1};
    constexpr int C[14] = {0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 0};
    float *const base[6] = {xyz, scaling, rotation, f_dc, nullptr, opacity};
    float m[14], v[14];
#pragma unroll
    for (int e = 0; e < 14; e++) {
        m[e] = ad.m[T[e]][ic * KK[e] + C[e]];
        v[e] = ad.v[T[e]][ic * KK[e] + C[e]];
    }
#pragma unroll
    for (int e = 0; e < 14; e++) {
        const int t = T[e];
        float pe = sp[e];
        gsr_adam1(pe, __fmul_rn(sg[e], ad.grad_scale), m[e], v[e], ad.lr_c[t], ad.b1[t], ad.b2[t], ad.omb1[t],
                  ad.omb2[t], ad.inv_sqrt_bc2[t], ad.eps[t]);
        base[t][ic * KK[e] + C[e]] = pe;
        ad.m[t][ic * KK[e] + C[e]] = m[e];
        ad.v[t][ic * KK[e] + C[e]] = v[e];
    }
}
// _features_rest of the listed rows: gradient from the stage, parameter and moments gathered in the stage's order
__device__ __forceinline__ void sa_rest_adam_out(const float *__restrict__ s_rest, const uint32_t *__restrict__ s_rows,
                                                 float *__restrict__ f_rest, const K11Adam &ad, int nw) {
    constexpr int t = 4;
    float *const mr = ad.m[t], *const vr = ad.v[t];
    const float gs = ad.grad_scale, lr_c = ad.lr_c[t], b1 = ad.b1[t], b2 = ad.b2[t], omb1 = ad.omb1[t],
                omb2 = ad.omb2[t], isb = ad.inv_sqrt_bc2[t], eps = ad.eps[t];
    for (int k0 = 0; k0 < REST_W; k0 += SA_UN) {
        size_t off[SA_UN];
        float pn[SA_UN], mn[SA_UN], vn[SA_UN];
#pragma unroll
        for (int u = 0; u < SA_UN; u++) {
            off[u] = sa_rest_offset(s_rows, min((k0 + u) * K11_BLOCK + (int)threadIdx.x, nw - 1));
            pn[u] = f_rest[off[u]];
            mn[u] = mr[off[u]];
            vn[u] = vr[off[u]];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < SA_UN; u++) {
            const int e = (k0 + u) * K11_BLOCK + (int)threadIdx.x;
            if (e < nw) {
                gsr_adam1(pn[u], __fmul_rn(s_rest[e], gs), mn[u], vn[u], lr_c, b1, b2, omb1, omb2, isb, eps);
                f_rest[off[u]] = pn[u];
                mr[off[u]] = mn[u];
                vr[off[u]] = vn[u];
            }
        }
    }
}

template <int DEG, bool ADAM, bool AA, typename ROWS = DenseRows, bool SUMS = false>
__device__ __forceinline__ void
preprocess_backward_batched_body(int P, int B, int M, const float *__restrict__ xyz,
                                   const float *__restrict__ scaling, float scale_modifier,
                                   const float *__restrict__ rotation, const float *__restrict__ f_dc,
                                   const float *__restrict__ f_rest, const float *__restrict__ opacity,
                                   const float *__restrict__ cams, int W, int H, const int32_t *__restrict__ radii,
                                   const float *__restrict__ cov3D, const uint8_t *__restrict__ clamped,
                                   const float *__restrict__ dL_dmeans2D,
                                   const float *__restrict__ dL_dconic_opacity, const float *__restrict__ dL_drgb,
                                   int gstride,
                                   float *__restrict__ dL_dxyz, float *__restrict__ dL_dscaling,
                                   float4 *__restrict__ dL_drotation, float *__restrict__ dL_ddc,
                                   float *__restrict__ dL_drest, float *__restrict__ dL_dopacity, const K11Adam &ad,
                                   const ROWS rows = ROWS{}, const GradSums *sums = nullptr) {
    constexpr bool LIST = std::is_same<ROWS, ListRows>::value;
    static_assert(!LIST || ADAM, "ListRows is the sparse K11 + Adam update (and takes M == 16)");
    static_assert(!SUMS || (ADAM && !LIST), "GradSums (B <= K11_SUMS_CAMS) feeds the fused dense kernel only");
    __shared__ float s_rest[K11_BLOCK * REST_W];
    __shared__ uint32_t s_rows[LIST ? K11_BLOCK : 1];  // ListRows: the workgroup's rows, for the gathers
    const bool staged = M == 16;  // _features_rest in, its gradient out: coalesced through LDS (ADAM: always)
    constexpr int NC = (DEG + 1) * (DEG + 1);
    // ---- every load of the lane that does not depend on another is issued here, before the first result is used
    // (clamped index: lanes past the end load the last Gaussian's / the list's last row's inputs and compute nothing)
    int i, nrows = 0;  // the lane's row;  ListRows: the workgroup's share of the list
    size_t ic;
    RestStage st;
    uint32_t live = 0;  // GradSums: bit c = camera c added into the row (flag set) and the row is visible there
    if constexpr (LIST) {
        const size_t first = (size_t)blockIdx.x * K11_BLOCK;
        nrows = (int)min((size_t)K11_BLOCK, (size_t)rows.count - first);
        const uint32_t irow = rows.list[first + min((int)threadIdx.x, nrows - 1)];
        s_rows[threadIdx.x] = irow;
        i = (int)irow;
        ic = irow;
    } else {
        i = blockIdx.x * blockDim.x + threadIdx.x;
        ic = (size_t)min(i, P - 1);
        if constexpr (SUMS) {  // every camera's flag and radius of the row first: they decide the loads of the queue
            int32_t rd[K11_SUMS_CAMS];
            uint8_t fl[K11_SUMS_CAMS];
#pragma unroll
            for (int u = 0; u < K11_SUMS_CAMS; u++) {
                const int c = min(u, B - 1);
                rd[u] = radii[(size_t)c * P + ic];
                fl[u] = sums->flags[c][ic];
            }
            if (staged) st = rest_stage_issue(f_rest, P);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < K11_SUMS_CAMS; u++) live |= (u < B && fl[u] && rd[u] > 0) ? 1u << u : 0u;
        } else if (staged) st = rest_stage_issue(f_rest, P);
    }
    const float p[3] = {xyz[3 * ic], xyz[3 * ic + 1], xyz[3 * ic + 2]};
    float cvr[6];
#pragma unroll
    for (int e = 0; e < 6; e++) cvr[e] = SUMS ? 0.f : cov3D[6 * ic + e];
    if (SUMS && live) {
#pragma unroll
        for (int e = 0; e < 6; e++) cvr[e] = cov3D[6 * ic + e];
    }
    const float dc[3] = {f_dc[3 * ic], f_dc[3 * ic + 1], f_dc[3 * ic + 2]};
    const float oraw = opacity[ic];
    const float4 qraw = *reinterpret_cast<const float4 *>(rotation + 4 * ic);
    const float scraw[3] = {scaling[3 * ic], scaling[3 * ic + 1], scaling[3 * ic + 2]};
    // (ListRows has no camera queue: its lanes load a camera's words inside the loops.  With the queue the sparse launch
    // measured 4-6 % slower at one camera, where the queue's slots hold the same camera twice: EXPERIMENTS.md)
    K11CamSH shq[K11_CAMQ];
    K11CamGeo geoq[K11_CAMQ];
    if constexpr (!LIST) {
#pragma unroll
        for (int u = 0; u < K11_CAMQ; u++) {
            const size_t o = (size_t)min(u, B - 1) * P + ic;
            if constexpr (SUMS) {
                const int c = min(u, B - 1);
                const double *a = sums->acc[c] + 9 * ic;
                shq[u] = k11_cam_load_sh_sums(o, (live >> c) & 1u, clamped, a);
                geoq[u] = k11_cam_load_geo_sums((live >> c) & 1u, a);
            } else {
                shq[u] = k11_cam_load_sh(o, radii, clamped, dL_drgb, gstride);
                geoq[u] = k11_cam_load_geo(o, radii, dL_dmeans2D, dL_dconic_opacity, gstride);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (LIST) {
        __syncthreads();  // the row table is complete
        sa_rest_stage_in(s_rest, s_rows, f_rest, nrows * REST_W);
        __syncthreads();
    } else if (staged) {
        rest_stage_commit(s_rest, st, f_rest, P);
        __syncthreads();
    }
    float sp[14], sg[14];  // ADAM: the per-lane parameters / gradients, updated after the stage-out (below)
    if (LIST ? (int)threadIdx.x < nrows : i < P) {
    float S[3][3];
    cov3d_unpack(cvr, S);
    // the SH coefficients above the DC term: read from the LDS stage where they are needed (staged), not held in 45
    // registers across the camera loop next to the 48 accumulators (the kernel needed 270 registers and spilled)
    const float *const shl = s_rest + threadIdx.x * REST_W;  // (an LDS address: ds_read, not a flat load)
    float sh[NC * 3];
    sh[0] = dc[0];
    sh[1] = dc[1];
    sh[2] = dc[2];
    if (!staged) {
        const float *rp = f_rest + (size_t)i * (M - 1) * 3;
#pragma unroll
        for (int k = 3; k < NC * 3; k++) sh[k] = rp[k - 3];
    }
    float dmean[3] = {0.f, 0.f, 0.f};
    float dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dsh[NC * 3];
#pragma unroll
    for (int k = 0; k < NC * 3; k++) dsh[k] = 0.f;
    float dop = 0.f;
    const float op_act = AA ? sigmoidf(oraw) : 0.f;  // AA: the uncompensated opacity, for the factor's gradient

    // Two loops over the cameras (round 6): the colour part first -- its 48 accumulators and the coefficients it reads
    // from the LDS stage are dead before the geometry part starts, whose covariance chain then has the registers to
    // itself (one loop needed 270 registers and spilled; the sums per camera are unchanged, dmean's order of summation
    // is colour part of all cameras, then geometry part of all cameras).
    for (int bc = 0; bc < B; bc++) {
        const K11CamSH cin = LIST ? k11_cam_load_sh((size_t)bc * P + ic, radii, clamped, dL_drgb, gstride) : shq[0];
        if constexpr (!LIST) {
#pragma unroll
            for (int u = 0; u + 1 < K11_CAMQ; u++) shq[u] = shq[u + 1];
            if (bc + K11_CAMQ < B) {  // (uniform) the camera K11_CAMQ ahead: in flight while this one is differentiated
                if constexpr (SUMS)
                    shq[K11_CAMQ - 1] =
                        k11_cam_load_sh_sums((size_t)(bc + K11_CAMQ) * P + i, (live >> (bc + K11_CAMQ)) & 1u, clamped,
                                             sums->acc[bc + K11_CAMQ] + 9 * (size_t)i);
                else
                    shq[K11_CAMQ - 1] =
                        k11_cam_load_sh((size_t)(bc + K11_CAMQ) * P + i, radii, clamped, dL_drgb, gstride);
            }
        }
        if (cin.rad <= 0) continue;
        if (staged) asm volatile("" ::: "memory");  // (keeps the LDS reads of the coefficients inside the loop)
        const float *cp = cams + (size_t)bc * CAM_STRIDE;
        const float camc[3] = {cp[32], cp[33], cp[34]};
        const float g3[3] = {cin.cl[0] ? 0.f : cin.grgb[0], cin.cl[1] ? 0.f : cin.grgb[1],
                             cin.cl[2] ? 0.f : cin.grgb[2]};
        float dm[3];
        viewdir_backward<DEG>(camc, p, ShStagedOrRegs{staged, shl, sh}, g3, DshAdd{dsh}, dm);
        dmean[0] += dm[0];
        dmean[1] += dm[1];
        dmean[2] += dm[2];
    }
    // the colour gradient is complete: DC to the per-lane slots / HBM, the rest over the coefficients in the stage
    if constexpr (ADAM) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
            sp[10 + e] = sh[e];
            sg[10 + e] = dsh[e];
        }
    } else {
        dL_ddc[3 * (size_t)i] = dsh[0];
        dL_ddc[3 * (size_t)i + 1] = dsh[1];
        dL_ddc[3 * (size_t)i + 2] = dsh[2];
    }
    {
        float *rp = staged ? s_rest + threadIdx.x * REST_W : dL_drest + (size_t)i * (M - 1) * 3;
#pragma unroll
        for (int k = 3; k < NC * 3; k++) rp[k - 3] = dsh[k];
        for (int k = NC * 3; k < M * 3; k++) rp[k - 3] = 0.f;
    }
    for (int bc = 0; bc < B; bc++) {
        const K11CamGeo cin =
            LIST ? k11_cam_load_geo((size_t)bc * P + ic, radii, dL_dmeans2D, dL_dconic_opacity, gstride) : geoq[0];
        if constexpr (!LIST) {
#pragma unroll
            for (int u = 0; u + 1 < K11_CAMQ; u++) geoq[u] = geoq[u + 1];
            if (bc + K11_CAMQ < B) {
                if constexpr (SUMS)
                    geoq[K11_CAMQ - 1] = k11_cam_load_geo_sums((live >> (bc + K11_CAMQ)) & 1u,
                                                               sums->acc[bc + K11_CAMQ] + 9 * (size_t)i);
                else
                    geoq[K11_CAMQ - 1] = k11_cam_load_geo((size_t)(bc + K11_CAMQ) * P + i, radii, dL_dmeans2D,
                                                          dL_dconic_opacity, gstride);
            }
        }
        if (cin.rad <= 0) continue;
        const float *cp = cams + (size_t)bc * CAM_STRIDE;
        const Cam cam = load_cam_packed(cp);
        const float tanfovx = cp[35], tanfovy = cp[36];
        const float fx = W / (2.0f * tanfovx), fy = H / (2.0f * tanfovy);
        const float4 gco = cin.gco;
        const float gA = gco.x, gB = gco.y, gC = gco.z;
        if (!AA) dop += gco.w;
        const Cov2DGrad cg = cov2d_backward<AA>(cam.v, fx, fy, tanfovx, tanfovy, p, S, gA, gB, gC,
                                                AA ? gco.w * op_act : 0.f);
        if (AA) dop += gco.w * cg.rho;
        if (cg.live) {
#pragma unroll
            for (int e = 0; e < 6; e++) dcov[e] += cg.dcov[e];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) dmean[k] += cg.dmean[k];
        float dm[3];
        means2d_to_mean(cam.p, p, cin.g2, dm);
#pragma unroll
        for (int k = 0; k < 3; k++) dmean[k] += dm[k];
    }
    // ---- stores + the camera-independent tail (cov3D -> scale / quaternion, activations), once
    if constexpr (ADAM) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
            sp[e] = p[e];
            sg[e] = dmean[e];
        }
    } else {
        dL_dxyz[3 * (size_t)i] = dmean[0];
        dL_dxyz[3 * (size_t)i + 1] = dmean[1];
        dL_dxyz[3 * (size_t)i + 2] = dmean[2];
    }
    {
        const float so = sigmoidf(oraw);
        if constexpr (ADAM) {
            sp[13] = oraw;
            sg[13] = dop * so * (1.0f - so);
        } else {
            dL_dopacity[i] = dop * so * (1.0f - so);
        }
    }
    {
        float gsc[3];
        float4 gq;
        cov3d_backward<true>(qraw, scraw, scale_modifier, dcov, gsc, gq);
        if constexpr (ADAM) {
#pragma unroll
            for (int e = 0; e < 3; e++) {
                sp[3 + e] = scraw[e];
                sg[3 + e] = gsc[e];
            }
            sp[6] = qraw.x; sp[7] = qraw.y; sp[8] = qraw.z; sp[9] = qraw.w;
            sg[6] = gq.x; sg[7] = gq.y; sg[8] = gq.z; sg[9] = gq.w;
        } else {
#pragma unroll
            for (int r = 0; r < 3; r++) dL_dscaling[3 * (size_t)i + r] = gsc[r];
            dL_drotation[i] = gq;
        }
    }
    if constexpr (LIST)
        sa_adam_small(ad, ic, const_cast<float *>(xyz), const_cast<float *>(scaling), const_cast<float *>(rotation),
                      const_cast<float *>(f_dc), const_cast<float *>(opacity), sp, sg);
    }  // the lane has a row
    if constexpr (LIST) {
        __syncthreads();
        sa_rest_adam_out(s_rest, s_rows, const_cast<float *>(f_rest), ad, nrows * REST_W);
    } else if (staged) {
        __syncthreads();
        if constexpr (ADAM) {
            rest_adam_out(s_rest, const_cast<float *>(f_rest), ad, P);
            __syncthreads();  // the stage is free: the moments of the small tensors go through it
            k11_adam_small_lds(s_rest, ad, P, i, const_cast<float *>(xyz), const_cast<float *>(scaling),
                               const_cast<float *>(rotation), const_cast<float *>(f_dc), const_cast<float *>(opacity),
                               sp, sg);
        } else {
            rest_stage_out(s_rest, dL_drest, P);
        }
    }
}

template <int DEG, bool AA>
__global__ void __launch_bounds__(K11_BLOCK, K11B_WAVES_PER_EU)
preprocess_backward_batched_kernel(int P, int B, int M, const float *__restrict__ xyz,
                                   const float *__restrict__ scaling, float scale_modifier,
                                   const float *__restrict__ rotation, const float *__restrict__ f_dc,
                                   const float *__restrict__ f_rest, const float *__restrict__ opacity,
                                   const float *__restrict__ cams, int W, int H, const int32_t *__restrict__ radii,
                                   const float *__restrict__ cov3D, const uint8_t *__restrict__ clamped,
                                   const float *__restrict__ dL_dmeans2D,
                                   const float *__restrict__ dL_dconic_opacity, const float *__restrict__ dL_drgb,
                                   int gstride, float *__restrict__ dL_dxyz, float *__restrict__ dL_dscaling,
                                   float4 *__restrict__ dL_drotation, float *__restrict__ dL_ddc,
                                   float *__restrict__ dL_drest, float *__restrict__ dL_dopacity) {
    preprocess_backward_batched_body<DEG, false, AA>(P, B, M, xyz, scaling, scale_modifier, rotation, f_dc, f_rest,
                                                     opacity, cams, W, H, radii, cov3D, clamped, dL_dmeans2D,
                                                     dL_dconic_opacity, dL_drgb, gstride, dL_dxyz, dL_dscaling,
                                                     dL_drotation, dL_ddc, dL_drest, dL_dopacity, K11Adam{});
}

template <int DEG, bool AA>
__global__ void __launch_bounds__(K11_BLOCK, K11B_WAVES_PER_EU)
preprocess_backward_adam_batched_kernel(int P, int B, float *__restrict__ xyz, float *__restrict__ scaling,
                                        float scale_modifier, float *__restrict__ rotation,
                                        float *__restrict__ f_dc, float *__restrict__ f_rest,
                                        float *__restrict__ opacity, const float *__restrict__ cams, int W, int H,
                                        const int32_t *__restrict__ radii, const float *__restrict__ cov3D,
                                        const uint8_t *__restrict__ clamped, const float *__restrict__ dL_dmeans2D,
                                        const float *__restrict__ dL_dconic_opacity,
                                        const float *__restrict__ dL_drgb, int gstride, const K11Adam ad_in) {
    if (ad_in.skip && *ad_in.skip) return;
    const K11Adam ad = k11_adam_resolve(ad_in);
    preprocess_backward_batched_body<DEG, true, AA>(P, B, 16, xyz, scaling, scale_modifier, rotation, f_dc, f_rest,
                                                    opacity, cams, W, H, radii, cov3D, clamped, dL_dmeans2D,
                                                    dL_dconic_opacity, dL_drgb, gstride, nullptr, nullptr, nullptr,
                                                    nullptr, nullptr, nullptr, ad);
}
// (GradSums: B <= K11_SUMS_CAMS cameras)
template <int DEG, bool AA>
__global__ void __launch_bounds__(K11_BLOCK, K11B_WAVES_PER_EU)
preprocess_backward_adam_batched_sums_kernel(int P, int B, float *__restrict__ xyz, float *__restrict__ scaling,
                                             float scale_modifier, float *__restrict__ rotation,
                                             float *__restrict__ f_dc, float *__restrict__ f_rest,
                                             float *__restrict__ opacity, const float *__restrict__ cams, int W, int H,
                                             const int32_t *__restrict__ radii, const float *__restrict__ cov3D,
                                             const uint8_t *__restrict__ clamped, const GradSums sums,
                                             const K11Adam ad_in) {
    if (ad_in.skip && *ad_in.skip) return;
    const K11Adam ad = k11_adam_resolve(ad_in);
    preprocess_backward_batched_body<DEG, true, AA, DenseRows, true>(
        P, B, 16, xyz, scaling, scale_modifier, rotation, f_dc, f_rest, opacity, cams, W, H, radii, cov3D, clamped,
        nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ad, DenseRows{}, &sums);
}

// ------------------------------------------------------------------- sparse (lazy) K11 + Adam
// gsr_preprocess_backward_adam_raw_batched_sparse: the fused update for the rows that received a gradient, nothing for
// the others (include/gsraster.h has the definition of "active").  Three launches on one stream, no host read-back:
//   reset     one lane: the workspace's counter = 0
//   classify  one pass over radii [B,P] and the gradient rows of the visible (camera, row) pairs -> active_out, and the
//             compacted list of active rows: ballots per wave, ONE atomic per workgroup of SA_CROWS rows to claim slots
//             (the list is ascending inside a workgroup's slots; the workgroups' order is the atomics')
//   update    a grid of fixed size, ceil(P / K11_BLOCK) workgroups; workgroup c takes list[c * K11_BLOCK ...] and leaves
//             at once when that is past the count it reads from the workspace.  One lane per active row: the row's
//             arithmetic is preprocess_backward_batched_body's (the same body, instantiated with ListRows, so the
//             same bits), its _features_rest row and the three arrays' 180 bytes per row move through the LDS stage --
//             lane e of the workgroup's 45 x K11_BLOCK words reads word e % 45 of row list[e / 45]: consecutive lanes
//             read consecutive words of a 180-byte row.
// Bytes: 4 B (+ 36 B where visible) per row and camera for the classification, + 4 B per row for active_out; per ACTIVE row
// 4 (list) + 56 + 24 (parameters, cov3D) + B * 43 (radius, record row, clamp flags) + 180 (SH) read, 236 parameters
// written, 2 * 236 moments read and written: 236 * 6 + 84 + 43 B.
constexpr int SA_CBLOCK = 256;          // lanes of a classify workgroup ...
constexpr int SA_CPER = 4;              // ... and rows per lane: one slot-claiming atomic per 1024 rows
constexpr int SA_CROWS = SA_CBLOCK * SA_CPER;
struct SparseWs {  // head of the caller's workspace; the list of active rows follows
    uint32_t count, pad[3];
};

__device__ __forceinline__ bool sa_nonzero(float x) {  // != 0.0f on the bits: -0.0 is zero, a denormal and a NaN are not
    return (__float_as_uint(x) & 0x7fffffffu) != 0u;
}

__global__ void sparse_adam_reset_kernel(const uint32_t *__restrict__ skip, SparseWs *__restrict__ ws) {
    if (skip && *skip) return;
    ws->count = 0u;
}

__global__ void __launch_bounds__(SA_CBLOCK)
sparse_adam_classify_kernel(int P, int B, const int32_t *__restrict__ radii, const float *__restrict__ dL_dmeans2D,
                            const float *__restrict__ dL_dconic_opacity, const float *__restrict__ dL_drgb, int gstride,
                            const uint32_t *__restrict__ skip, SparseWs *__restrict__ ws, uint32_t *__restrict__ list,
                            uint8_t *__restrict__ active_out) {
    if (skip && *skip) return;
    constexpr int NW = SA_CBLOCK / GSR_WAVE;
    __shared__ uint32_t s_cnt[SA_CPER * NW];
    __shared__ uint32_t s_base;
    const size_t row0 = (size_t)blockIdx.x * SA_CROWS;
    const int wave = threadIdx.x / GSR_WAVE;
    bool act[SA_CPER];
    uint32_t rank[SA_CPER];
#pragma unroll
    for (int j = 0; j < SA_CPER; j++) {
        const size_t i = row0 + (size_t)j * SA_CBLOCK + threadIdx.x;
        bool a = false;
        if (i < (size_t)P) {
            for (int bc = 0; bc < B; bc++) {
                const size_t o = (size_t)bc * P + i;
                if (radii[o] <= 0) continue;  // the gradient words of a culled pair are not even read
                const float2 g2 = grad_ld2(dL_dmeans2D, o, gstride);
                const float4 gco = grad_ld4(dL_dconic_opacity, o, gstride);
                const float *gr = dL_drgb + (size_t)(gstride ? gstride : 3) * o;
                a = a || sa_nonzero(g2.x) || sa_nonzero(g2.y) || sa_nonzero(gr[0]) || sa_nonzero(gr[1]) ||
                    sa_nonzero(gr[2]) || sa_nonzero(gco.x) || sa_nonzero(gco.y) || sa_nonzero(gco.z) ||
                    sa_nonzero(gco.w);
            }
            if (active_out) active_out[i] = a ? 1 : 0;
        }
        const unsigned long long bal = __ballot(a);
        act[j] = a;
        rank[j] = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if ((threadIdx.x & (GSR_WAVE - 1)) == 0) s_cnt[j * NW + wave] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // exclusive scan of the 16 counts, in the order of the rows; one atomic for the workgroup
        uint32_t run = 0;
        for (int k = 0; k < SA_CPER * NW; k++) {
            const uint32_t c = s_cnt[k];
            s_cnt[k] = run;
            run += c;
        }
        s_base = run ? atomicAdd(&ws->count, run) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SA_CPER; j++)
        if (act[j])  // (slot < P: every row is counted at most once)
            list[s_base + s_cnt[j * NW + wave] + rank[j]] = (uint32_t)(row0 + (size_t)j * SA_CBLOCK + threadIdx.x);
}

template <int DEG, bool AA>
__global__ void __launch_bounds__(K11_BLOCK, K11B_WAVES_PER_EU)
sparse_adam_update_kernel(int P, int B, float *__restrict__ xyz, float *__restrict__ scaling, float scale_modifier,
                          float *__restrict__ rotation, float *__restrict__ f_dc, float *__restrict__ f_rest,
                          float *__restrict__ opacity, const float *__restrict__ cams, int W, int H,
                          const int32_t *__restrict__ radii, const float *__restrict__ cov3D,
                          const uint8_t *__restrict__ clamped, const float *__restrict__ dL_dmeans2D,
                          const float *__restrict__ dL_dconic_opacity, const float *__restrict__ dL_drgb, int gstride,
                          const K11Adam ad_in, const SparseWs *__restrict__ ws, const uint32_t *__restrict__ list,
                          uint32_t *__restrict__ num_active) {
    if (ad_in.skip && *ad_in.skip) return;
    const uint32_t count = min(ws->count, (uint32_t)P);
    if (blockIdx.x == 0 && threadIdx.x == 0 && num_active) *num_active = count;
    if ((size_t)blockIdx.x * K11_BLOCK >= count) return;  // (uniform) past the list: at a tenth of the rows active, nine
                                                          // workgroups of ten
    const K11Adam ad = k11_adam_resolve(ad_in);
    preprocess_backward_batched_body<DEG, true, AA>(P, B, 16, xyz, scaling, scale_modifier, rotation, f_dc, f_rest,
                                                    opacity, cams, W, H, radii, cov3D, clamped, dL_dmeans2D,
                                                    dL_dconic_opacity, dL_drgb, gstride, nullptr, nullptr, nullptr,
                                                    nullptr, nullptr, nullptr, ad, ListRows{list, count});
}

// ------------------------------------------------------------------- K11c: camera (pose) gradients
// dL/d(viewmatrix, projmatrix, campos) of a batch of cameras: per visible Gaussian and camera the 27 sums below,
// reduced over the whole shard.  The per-Gaussian quantities are K11's own (the same dL_da/db/dc with its
// 1 / (denom^2 + 1e-7), the same treatment of the Jacobian clamp), so camera and parameter gradients are consistent.
//   sums  0..11  viewmatrix[r][k], r = 0..3, k = 0..2:  [p,1]_r * dL/dt_k, plus (r < 3) the path through
//                Wc = viewmatrix[:3,:3]^T in T = J Wc:  [k][0] += J00 dT0_k, [k][1] += J11 dT1_k,
//                [k][2] += J02 dT0_k + J12 dT1_k   (column 3 of the view matrix is not read by the forward)
//   sums 12..23  projmatrix[r][c], c in {0, 1, 3}:  [p,1]_r * dL/dp_hom_c  (column 2 only feeds the unused p_proj.z)
//   sums 24..26  campos:  minus the SH view-direction part of dL/dmean (0 at degree 0 and for clamped channels)
// A lane walks its rows with a grid stride and accumulates in fp32 registers (the grid grows with P up to KC_RESIDENT
// workgroups for all cameras: 8 rows per lane and camera at 10^6 Gaussians); from there on every addition is fp64 and in a fixed order -- xor
// butterfly inside the wave, the workgroup's waves through LDS, one partial row per workgroup and camera into the
// caller's workspace, and the finalize kernel over the workgroups.  No atomics: bit-identical from run to run.
// Traffic per visible Gaussian and camera: 4 (radius) + 12 + 24 + 45 * 4 (position, covariance, SH above DC) + 36
// (gradient record row) + 3 (clamp flags) = 259 B at degree 3.  The DC coefficient does not depend on the view
// direction: never read.
constexpr int KC_BLOCK = 256;
constexpr int KC_WAVES = KC_BLOCK / 64;
constexpr int KC_NS = 27;            // non-trivial sums per camera
// workgroups of a launch, all cameras together: what the device holds at once (256 CUs x 2: two waves per SIMD, four
// per workgroup).  One resident round measured fastest at 10^6 Gaussians (every workgroup ends with 27 fp64 butterflies
// and a pass through LDS) -- main kernel with one / four cameras, by row blocks per camera: 1024: 70 / 216 us,
// 512: 63 / 185, 256: 84 / 171, 128: 143 / 164; three waves per SIMD (168 registers, 18 spilled): 74-77 / 202-211
constexpr int KC_RESIDENT = 512;
constexpr int KC_FIN_SLICES = 32;                 // the finalize adds the partial rows in this many contiguous slices

// one (Gaussian, camera) pair: adds its 27 contributions to acc
template <int DEG>
__device__ __forceinline__ void cams_accumulate(float (&acc)[KC_NS], const float *__restrict__ cp, int W, int H,
                                                const float (&p)[3], const float (&cv)[6],
                                                const float *__restrict__ sh, const float4 gco, const float2 g2,
                                                const float (&g3)[3]) {
    const Cam cam = load_cam_packed(cp);
    const float tanfovx = cp[35], tanfovy = cp[36];
    const float fx = W / (2.0f * tanfovx), fy = H / (2.0f * tanfovy);
    const float ph[4] = {p[0], p[1], p[2], 1.f};
    // ---- conic -> cov2D -> T = J Wc -> (t, Wc): K11's chain
    float S[3][3];
    cov3d_unpack(cv, S);
    const Cov2DGrad cg = cov2d_backward(cam.v, fx, fy, tanfovx, tanfovy, p, S, gco.x, gco.y, gco.z);
    const float(&tc)[3] = cg.tc;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) acc[r * 3 + k] += ph[r] * cg.dt[k];
    const float J00 = fx / tc[2], J02 = -(fx * tc[0]) / (tc[2] * tc[2]);
    const float J11 = fy / tc[2], J12 = -(fy * tc[1]) / (tc[2] * tc[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        acc[k * 3 + 0] += J00 * cg.dT0[k];
        acc[k * 3 + 1] += J11 * cg.dT1[k];
        acc[k * 3 + 2] += J02 * cg.dT0[k] + J12 * cg.dT1[k];
    }
    // ---- means2D (NDC-scaled) -> p_hom through the perspective divide
    {
        float mw, mul1, mul2;
        perspective_backward(cam.p, p, mw, mul1, mul2);
        const float dh[3] = {mw * g2.x, mw * g2.y, -(mul1 * g2.x + mul2 * g2.y)};
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) acc[12 + r * 3 + k] += ph[r] * dh[k];
    }
    // ---- colour -> view direction -> campos (the coefficient gradients are not wanted here)
    if constexpr (DEG > 0) {
        float dm[3];
        viewdir_backward<DEG>(cam.c, p, ShRegs{sh}, g3, DshDrop{}, dm);
        acc[24] -= dm[0];
        acc[25] -= dm[1];
        acc[26] -= dm[2];
    }
}

// One workgroup = one (row block, camera) pair; partials: [nb][B][KC_NS] doubles, every word written (the workspace
// need not be zero on entry).  27 fp32 accumulators per camera next to K11's chain leave room for one camera per lane
// (two cameras: 256 registers and spills), so the B cameras of a row block are B workgroups -- numbered so that they
// follow each other on the SAME XCD (workgroup w runs on XCD w % 8): position, covariance and coefficients of a row
// come from HBM once and from that XCD's L2 for the other cameras.
template <int DEG>
__global__ void __launch_bounds__(KC_BLOCK, 2)
preprocess_backward_cams_kernel(int P, int B, int nb, const float *__restrict__ means3D,
                                const float *__restrict__ sh_rest, int rest_stride, const float *__restrict__ cams,
                                int W, int H, const int32_t *__restrict__ radii, const float *__restrict__ cov3D,
                                const uint8_t *__restrict__ clamped, const float *__restrict__ dL_dmeans2D,
                                const float *__restrict__ dL_dconic_opacity, const float *__restrict__ dL_drgb,
                                int gstride, double *__restrict__ partials) {
    constexpr int NC = (DEG + 1) * (DEG + 1);
    const int q = blockIdx.x >> 3;
    const int rb = (blockIdx.x & 7) + 8 * (q / B), bc = q % B;  // row block, camera
    if (rb >= nb) return;                                       // (the grid is rounded up to 8 row blocks)
    const float *cp = cams + (size_t)bc * CAM_STRIDE;
    float acc[KC_NS];
#pragma unroll
    for (int s = 0; s < KC_NS; s++) acc[s] = 0.f;
    const size_t step = (size_t)nb * KC_BLOCK;
    for (size_t i = (size_t)rb * KC_BLOCK + threadIdx.x; i < (size_t)P; i += step) {
        const size_t o = (size_t)bc * P + i;
        if (radii[o] <= 0) continue;  // culled: contributes nothing, its gradient row is never looked at
        // every load of the row is issued before the first result is used
        const float p[3] = {means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]};
        float cv[6];
#pragma unroll
        for (int e = 0; e < 6; e++) cv[e] = cov3D[6 * i + e];
        const float4 gco = grad_ld4(dL_dconic_opacity, o, gstride);
        const float2 g2 = grad_ld2(dL_dmeans2D, o, gstride);
        float sh[NC * 3], g3[3] = {0.f, 0.f, 0.f};
        sh[0] = sh[1] = sh[2] = 0.f;  // (the DC term has no view-direction derivative: never read)
        if constexpr (DEG > 0) {
            const float *rp = sh_rest + (size_t)rest_stride * i;
#pragma unroll
            for (int k = 3; k < NC * 3; k++) sh[k] = rp[k - 3];
#pragma unroll
            for (int e = 0; e < 3; e++)
                g3[e] = clamped[3 * o + e] ? 0.f : dL_drgb[(size_t)(gstride ? gstride : 3) * o + e];
        }
        cams_accumulate<DEG>(acc, cp, W, H, p, cv, sh, gco, g2, g3);
    }
    // ---- wave (fp64 butterfly: every lane ends with the same sum), then the workgroup's waves in order
    __shared__ double s_part[KC_WAVES][KC_NS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < KC_NS; s++) {
        double v = (double)acc[s];
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if (lane == 0) s_part[wave][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < KC_NS) {
        double v = s_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < KC_WAVES; w++) v += s_part[w][threadIdx.x];
        partials[((size_t)rb * B + bc) * KC_NS + threadIdx.x] = v;
    }
}

// one workgroup per camera: the nb partial rows in a fixed order (KC_FIN_SLICES contiguous slices, then the slices), one
// rounding to fp32, scattered into the 40-word record of `cams` with its structural zeros (nb == 0: all zeros).  32
// slices of at most 32 rows with the loads unrolled: eight slices of 128 dependent-latency loads took 39 us
__global__ void __launch_bounds__(KC_FIN_SLICES * 32)
preprocess_backward_cams_finalize_kernel(int nb, int B, const double *__restrict__ partials,
                                         float *__restrict__ dL_dcams) {
    __shared__ double sl[KC_FIN_SLICES][32];
    const int b = blockIdx.x, j = threadIdx.x & 31, sidx = threadIdx.x >> 5;
    double v = 0.0;
    if (j < KC_NS) {
        const int per = (nb + KC_FIN_SLICES - 1) / KC_FIN_SLICES;
        const int lo = min(nb, sidx * per), hi = min(nb, lo + per);
#pragma unroll 8
        for (int k = lo; k < hi; k++) v += partials[((size_t)k * B + b) * KC_NS + j];
    }
    sl[sidx][j] = v;
    __syncthreads();
    const int w = threadIdx.x;
    if (w >= CAM_STRIDE) return;
    int idx = -1;
    if (w < 16) {
        if ((w & 3) < 3) idx = (w >> 2) * 3 + (w & 3);
    } else if (w < 32) {
        const int r = (w - 16) >> 2, c = (w - 16) & 3;
        if (c != 2) idx = 12 + r * 3 + (c == 3 ? 2 : c);
    } else if (w < 35) {
        idx = 24 + (w - 32);
    }
    float out = 0.f;
    if (idx >= 0) {
        double t = sl[0][idx];
#pragma unroll
        for (int q = 1; q < KC_FIN_SLICES; q++) t += sl[q][idx];
        out = (float)t;
    }
    dL_dcams[(size_t)b * CAM_STRIDE + w] = out;
}

// row blocks per camera: KC_RESIDENT workgroups shared by the B cameras (a multiple of 8, one per XCD, at least 8)
inline int kc_blocks(int P, int B) {
    const int nb = P <= 0 ? 0 : (int)gsr_div_up(P, KC_BLOCK);
    int cap = (KC_RESIDENT / (B > 0 ? B : 1) + 7) & ~7;
    if (cap < 8) cap = 8;
    return nb < cap ? nb : cap;
}

// -------------------------------------------------------------------------------------------- K2
__global__ void __launch_bounds__(GSR_ONE_DIM_BLOCK)
local2j_kernel(int P, int W, int H, int ws, const float2 *__restrict__ means2D, const int32_t *__restrict__ radii,
               const int32_t *__restrict__ div, uint8_t *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    const int rad = radii[i];
    int minx = 0, miny = 0, maxx = 0, maxy = 0;
    if (rad > 0) {
        const float2 xy = means2D[i];
        gsr_get_rect(xy.x, xy.y, rad, gx, gy, minx, miny, maxx, maxy);
    }
    const bool nonempty = rad > 0 && maxx > minx && maxy > miny;
    for (int j = 0; j < ws; j++) {
        const int lo = div[j], hi = div[j + 1];
        bool hit = false;
        if (nonempty) {
            // rows of the rect whose tile-id span [y*gx+minx, y*gx+maxx-1] meets [lo,hi)
            // y*gx+minx < hi  <=> y <= (hi-1-minx)/gx ;  y*gx+maxx-1 >= lo <=> y >= ceil((lo-maxx+1)/gx)
            const int num_hi = hi - 1 - minx;
            const int y_hi = num_hi < 0 ? -1 : num_hi / gx;
            const int num_lo = lo - maxx + 1;
            const int y_lo = num_lo <= 0 ? 0 : (num_lo + gx - 1) / gx;
            hit = max(y_lo, miny) <= min(y_hi, maxy - 1);
        }
        out[(size_t)i * ws + j] = hit ? 1 : 0;
    }
}

}  // namespace

#define GSR_DISPATCH_DEG(D, ...)                 \
    switch (D) {                                 \
        case 0: { constexpr int DEG = 0; __VA_ARGS__; } break; \
        case 1: { constexpr int DEG = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int DEG = 2; __VA_ARGS__; } break; \
        default: { constexpr int DEG = 3; __VA_ARGS__; } break; \
    }
// ... and over the anti-aliasing variant: `aa` is what the entry point read from the switch, ONCE, on the host
#define GSR_DISPATCH_DEG_AA(D, aa, ...)                                     \
    if (aa) { constexpr bool AA = true; GSR_DISPATCH_DEG(D, __VA_ARGS__) }  \
    else { constexpr bool AA = false; GSR_DISPATCH_DEG(D, __VA_ARGS__) }

// gsr_set_antialiasing: process-wide, like the binning switches (g_tile_cull, g_tie_order in binning_host.h).  Every
// K1 / K11 entry point loads it once per call and picks the instantiation; what is already enqueued or captured keeps
// the kernel it was launched with.
static std::atomic<int> g_antialiasing{0};
int gsr_antialiasing_mode() { return g_antialiasing.load(std::memory_order_relaxed); }
extern "C" int gsr_set_antialiasing(int mode) {
    if (mode != 0 && mode != 1) return GSR_EINVAL;
    return g_antialiasing.exchange(mode, std::memory_order_relaxed);
}

int gsr_launch_preprocess_forward(int P, int D, int M, const float *means3D, const float *scales, float scale_modifier,
                                  const float *rotations, const float *shs, const float *shs_rest,
                                  const float *opacities,
                                  const float *viewmatrix, const float *projmatrix, const float *campos, int W, int H,
                                  float tanfovx, float tanfovy, float *means2D, float *depths, int32_t *radii,
                                  float *cov3D, float *conic_opacity, float *rgb, uint8_t *clamped, int aa,
                                  hipStream_t stream) {
    if (P == 0) return 0;
    const dim3 grid(gsr_div_up(P, GSR_ONE_DIM_BLOCK)), block(GSR_ONE_DIM_BLOCK);
#define GSR_FWD(RAWF)                                                                                              \
    GSR_DISPATCH_DEG_AA(D, aa, hipLaunchKernelGGL((preprocess_forward_kernel<DEG, RAWF, AA>), grid, block, 0,      \
                                           stream, P, M,                                                           \
                                           means3D, scales, scale_modifier, rotations, shs, shs_rest, opacities,   \
                                           viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy,                 \
                                           reinterpret_cast<float2 *>(means2D), depths, radii, cov3D,              \
                                           reinterpret_cast<float4 *>(conic_opacity), rgb, clamped))
    if (shs_rest) { GSR_FWD(true); } else { GSR_FWD(false); }
#undef GSR_FWD
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_preprocess_backward(int P, int D, int M, const float *means3D, const float *scales,
                                   float scale_modifier, const float *rotations, const float *shs,
                                   const float *shs_rest, const float *opacities_raw, const float *viewmatrix, const float *projmatrix, const float *campos, int W,
                                   int H, float tanfovx, float tanfovy, const int32_t *radii, const float *cov3D,
                                   const uint8_t *clamped, const float *dL_dmeans2D, const float *dL_dconic_opacity,
                                   const float *dL_drgb, int grad_row_stride, float *dL_dmeans3D, float *dL_dscales, float *dL_drotations,
                                   float *dL_dshs, float *dL_dshs_rest, float *dL_dopacities, int aa,
                                   hipStream_t stream) {
    if (P == 0) return 0;
    const dim3 grid(gsr_div_up(P, K11_BLOCK)), block(K11_BLOCK);
#define GSR_BWD(RAWF)                                                                                              \
    GSR_DISPATCH_DEG_AA(D, aa, hipLaunchKernelGGL((preprocess_backward_kernel<DEG, RAWF, AA>), grid, block, 0,     \
                                           stream, P, M,                                                           \
                                           means3D, scales, scale_modifier, rotations, shs, shs_rest,              \
                                           opacities_raw, viewmatrix, projmatrix, campos, W, H, tanfovx, tanfovy,  \
                                           radii, cov3D, clamped, dL_dmeans2D, dL_dconic_opacity, dL_drgb,           \
                                           grad_row_stride,                                                          \
                                           dL_dmeans3D, dL_dscales, reinterpret_cast<float4 *>(dL_drotations),     \
                                           dL_dshs, dL_dshs_rest, dL_dopacities))
    if (shs_rest) { GSR_BWD(true); } else { GSR_BWD(false); }
#undef GSR_BWD
    GSR_LAUNCH_CHECK();
    return 0;
}

int gsr_launch_local2j(int P, int W, int H, int ws, const float *means2D, const int32_t *radii, const int32_t *div,
                       uint8_t *out, hipStream_t stream) {
    if (P == 0) return 0;
    hipLaunchKernelGGL(local2j_kernel, dim3(gsr_div_up(P, GSR_ONE_DIM_BLOCK)), dim3(GSR_ONE_DIM_BLOCK), 0, stream, P,
                       W, H, ws, reinterpret_cast<const float2 *>(means2D), radii, div, out);
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_preprocess_forward_raw_batched(int P, int B, int sh_degree, int sh_coeffs, const float *xyz,
                                                  const float *scaling, float scale_modifier, const float *rotation,
                                                  const float *features_dc, const float *features_rest,
                                                  const float *opacity, const float *cams, int width, int height,
                                                  float *means2D, float *depths, int32_t *radii, float *cov3D,
                                                  float *conic_opacity, float *rgb, uint8_t *clamped,
                                                  gsr_stream_t stream) {
    if (P < 0 || B < 1 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < 2 ||
        sh_coeffs < (sh_degree + 1) * (sh_degree + 1) || width <= 0 || height <= 0)
        return GSR_EINVAL;
    if (P == 0) return 0;
    if (!xyz || !scaling || !rotation || !features_dc || !features_rest || !opacity || !cams || !means2D || !depths ||
        !radii || !cov3D || !conic_opacity || !rgb || !clamped)
        return GSR_EINVAL;
    const dim3 grid(gsr_div_up(P, GSR_ONE_DIM_BLOCK)), block(GSR_ONE_DIM_BLOCK);
    GSR_DISPATCH_DEG_AA(sh_degree, gsr_antialiasing_mode(),
                     hipLaunchKernelGGL((preprocess_forward_batched_kernel<DEG, AA>), grid, block, 0,
                                        reinterpret_cast<hipStream_t>(stream), P, B, sh_coeffs, xyz, scaling,
                                        scale_modifier, rotation, features_dc, features_rest, opacity, cams, width,
                                        height, reinterpret_cast<float2 *>(means2D), depths, radii, cov3D,
                                        reinterpret_cast<float4 *>(conic_opacity), rgb, clamped));
    GSR_LAUNCH_CHECK();
    return 0;
}

extern "C" int gsr_preprocess_backward_raw_batched(int P, int B, int sh_degree, int sh_coeffs, const float *xyz,
                                                   const float *scaling, float scale_modifier, const float *rotation,
                                                   const float *features_dc, const float *features_rest,
                                                   const float *opacity, const float *cams, int width, int height,
                                                   const int32_t *radii, const float *cov3D, const uint8_t *clamped,
                                                   const float *dL_dmeans2D, const float *dL_dconic_opacity,
                                                   const float *dL_drgb, int grad_row_stride, float *dL_dxyz, float *dL_dscaling,
                                                   float *dL_drotation, float *dL_dfeatures_dc,
                                                   float *dL_dfeatures_rest, float *dL_dopacity, gsr_stream_t stream) {
    if (P < 0 || B < 1 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < 2 ||
        sh_coeffs < (sh_degree + 1) * (sh_degree + 1) || width <= 0 || height <= 0)
        return GSR_EINVAL;
    if (P == 0) return 0;
    if (!xyz || !scaling || !rotation || !features_dc || !features_rest || !opacity || !cams || !radii || !cov3D ||
        !clamped || !dL_dmeans2D || !dL_dconic_opacity || !dL_drgb || !dL_dxyz || !dL_dscaling || !dL_drotation ||
        !dL_dfeatures_dc || !dL_dfeatures_rest || !dL_dopacity)
        return GSR_EINVAL;
    const dim3 grid(gsr_div_up(P, K11_BLOCK)), block(K11_BLOCK);
    GSR_DISPATCH_DEG_AA(sh_degree, gsr_antialiasing_mode(),
                     hipLaunchKernelGGL((preprocess_backward_batched_kernel<DEG, AA>), grid, block, 0,
                                        reinterpret_cast<hipStream_t>(stream), P, B, sh_coeffs, xyz, scaling,
                                        scale_modifier, rotation, features_dc, features_rest, opacity, cams, width,
                                        height, radii, cov3D, clamped, dL_dmeans2D, dL_dconic_opacity, dL_drgb,
                                        grad_row_stride, dL_dxyz,
                                        dL_dscaling, reinterpret_cast<float4 *>(dL_drotation), dL_dfeatures_dc,
                                        dL_dfeatures_rest, dL_dopacity));
    GSR_LAUNCH_CHECK();
    return 0;
}

// What the fused entry points below share once P > 0: the null checks of the arguments all of them take (the thirteen
// device arrays of K11, then the tables), and the kernels' K11Adam from the host tables (lrs .. steps as in gsr_adam_step_multi; with dyn_dev the step-dependent factors
// come from the device block and lrs / steps are not read).  -> true: GSR_EINVAL.
static bool k11_adam_fill(K11Adam &ad, std::initializer_list<const void *> device_arrays, float *const *exp_avgs,
                          float *const *exp_avg_sqs, const double *lrs, const double *beta1s, const double *beta2s,
                          const double *epss, const int64_t *steps, float grad_scale, const float *dyn_dev,
                          const uint32_t *skip_flag_dev) {
    for (const void *a : device_arrays)
        if (!a) return true;
    if (!exp_avgs || !exp_avg_sqs || !beta1s || !beta2s || !epss || (!dyn_dev && (!lrs || !steps))) return true;
    ad.dyn = dyn_dev;
    ad.skip = skip_flag_dev;
    ad.grad_scale = grad_scale;
    for (int t = 0; t < 6; t++) {
        if (!exp_avgs[t] || !exp_avg_sqs[t] || (!dyn_dev && steps[t] < 1)) return true;
        const double bc1 = dyn_dev ? 1.0 : 1.0 - pow(beta1s[t], (double)steps[t]);
        const double bc2 = dyn_dev ? 1.0 : 1.0 - pow(beta2s[t], (double)steps[t]);
        ad.m[t] = exp_avgs[t];
        ad.v[t] = exp_avg_sqs[t];
        ad.lr_c[t] = dyn_dev ? 0.f : (float)(lrs[t] / bc1);
        ad.b1[t] = (float)beta1s[t];
        ad.b2[t] = (float)beta2s[t];
        ad.omb1[t] = (float)(1.0 - beta1s[t]);
        ad.omb2[t] = (float)(1.0 - beta2s[t]);
        ad.inv_sqrt_bc2[t] = (float)(1.0 / sqrt(bc2));
        ad.eps[t] = (float)epss[t];
    }
    return false;
}

// The dense fused launch once the arguments are checked and `ad` is filled: alignment of what is moved in 16-byte
// pieces, then the one-camera kernel (B == 1 with the host tangents) or the camera-batched one, for either source.
template <typename SRC>
static int k11_adam_launch(int P, int B, int sh_degree, float *xyz, float *scaling, float scale_modifier, float *rotation,
                           float *features_dc, float *features_rest, float *opacity, const float *cams, int width,
                           int height, const int32_t *radii, const float *cov3D, const uint8_t *clamped, const SRC &src,
                           const K11Adam &ad, const float *tanfov0, gsr_stream_t stream) {
    uintptr_t al = (uintptr_t)features_rest | (uintptr_t)rotation;
    for (int t = 0; t < 6; t++) al |= (uintptr_t)ad.m[t] | (uintptr_t)ad.v[t];
    if (al & 15) return GSR_EINVAL;  // 16-byte accesses on the moments and the _features_rest block
    const dim3 grid(gsr_div_up(P, K11_BLOCK)), block(K11_BLOCK);
    const int aa = gsr_antialiasing_mode();
    if (B == 1 && tanfov0) {  // one camera: the leaner kernel without accumulators
        if constexpr (std::is_same<SRC, GradSums>::value) {
            GSR_DISPATCH_DEG_AA(sh_degree, aa,
                             hipLaunchKernelGGL((preprocess_backward_adam_sums_kernel<DEG, AA>), grid, block, 0,
                                                reinterpret_cast<hipStream_t>(stream), P, xyz, scaling, scale_modifier,
                                                rotation, features_dc, features_rest, opacity, cams, cams + 16,
                                                cams + 32, width, height, tanfov0[0], tanfov0[1], radii, cov3D, clamped,
                                                src, ad));
        } else {
            GSR_DISPATCH_DEG_AA(sh_degree, aa,
                             hipLaunchKernelGGL((preprocess_backward_adam_kernel<DEG, AA>), grid, block, 0,
                                                reinterpret_cast<hipStream_t>(stream), P, xyz, scaling, scale_modifier,
                                                rotation, features_dc, features_rest, opacity, cams, cams + 16,
                                                cams + 32, width, height, tanfov0[0], tanfov0[1], radii, cov3D, clamped,
                                                src.means2D, src.conic_opacity, src.rgb, src.gstride, ad));
        }
        GSR_LAUNCH_CHECK();
        return 0;
    }
    if constexpr (std::is_same<SRC, GradSums>::value) {
        GSR_DISPATCH_DEG_AA(sh_degree, aa,
                         hipLaunchKernelGGL((preprocess_backward_adam_batched_sums_kernel<DEG, AA>), grid, block, 0,
                                            reinterpret_cast<hipStream_t>(stream), P, B, xyz, scaling, scale_modifier,
                                            rotation, features_dc, features_rest, opacity, cams, width, height, radii,
                                            cov3D, clamped, src, ad));
    } else {
        GSR_DISPATCH_DEG_AA(sh_degree, aa,
                         hipLaunchKernelGGL((preprocess_backward_adam_batched_kernel<DEG, AA>), grid, block, 0,
                                            reinterpret_cast<hipStream_t>(stream), P, B, xyz, scaling, scale_modifier,
                                            rotation, features_dc, features_rest, opacity, cams, width, height, radii,
                                            cov3D, clamped, src.means2D, src.conic_opacity, src.rgb, src.gstride, ad));
    }
    GSR_LAUNCH_CHECK();
    return 0;
}

// K11 for a batch of cameras fused with the optimizer step of the six tensors it differentiates (see K11Adam):
// xyz .. opacity are read AND updated in place, exp_avgs / exp_avg_sqs are the moments in the tensor order
// xyz, scaling, rotation, features_dc, features_rest, opacity; lrs .. steps as in gsr_adam_step_multi.  tanfov0: HOST
// pointer to { tanfovx, tanfovy } of the camera when B == 1 (selects the one-camera kernel, as
// gsr_preprocess_backward_raw does), or NULL.
extern "C" int gsr_preprocess_backward_adam_raw_batched(
    int P, int B, int sh_degree, int sh_coeffs, float *xyz, float *scaling, float scale_modifier, float *rotation,
    float *features_dc, float *features_rest, float *opacity, const float *cams, int width, int height,
    const int32_t *radii, const float *cov3D, const uint8_t *clamped, const float *dL_dmeans2D,
    const float *dL_dconic_opacity, const float *dL_drgb, int grad_row_stride, float *const *exp_avgs,
    float *const *exp_avg_sqs, const double *lrs, const double *beta1s, const double *beta2s, const double *epss,
    const int64_t *steps, float grad_scale, const float *tanfov0, gsr_stream_t stream) {
    return gsr_preprocess_backward_adam_raw_batched_dyn(
        P, B, sh_degree, sh_coeffs, xyz, scaling, scale_modifier, rotation, features_dc, features_rest, opacity, cams,
        width, height, radii, cov3D, clamped, dL_dmeans2D, dL_dconic_opacity, dL_drgb, grad_row_stride, exp_avgs,
        exp_avg_sqs, lrs, beta1s, beta2s, epss, steps, grad_scale, tanfov0, nullptr, nullptr, stream);
}

// The same launch for a captured (hipGraph) iteration: `dyn_dev` (DEVICE, 12 floats: lr / (1 - beta1^t) and
// 1 / sqrt(1 - beta2^t) of the six tensors, in the tensor order above) replaces what `lrs` / `steps` would give -- both
// may then be NULL -- and `skip_flag_dev` (DEVICE word, may be NULL) turns the whole launch into a no-op when it is
// non-zero at execution time.  With both NULL this is gsr_preprocess_backward_adam_raw_batched.
extern "C" int gsr_preprocess_backward_adam_raw_batched_dyn(
    int P, int B, int sh_degree, int sh_coeffs, float *xyz, float *scaling, float scale_modifier, float *rotation,
    float *features_dc, float *features_rest, float *opacity, const float *cams, int width, int height,
    const int32_t *radii, const float *cov3D, const uint8_t *clamped, const float *dL_dmeans2D,
    const float *dL_dconic_opacity, const float *dL_drgb, int grad_row_stride, float *const *exp_avgs,
    float *const *exp_avg_sqs, const double *lrs, const double *beta1s, const double *beta2s, const double *epss,
    const int64_t *steps, float grad_scale, const float *tanfov0, const float *dyn_dev, const uint32_t *skip_flag_dev,
    gsr_stream_t stream) {
    if (P < 0 || B < 1 || sh_degree < 0 || sh_degree > 3 || sh_coeffs != 16 || width <= 0 || height <= 0)
        return GSR_EINVAL;  // the fused step needs the LDS stage of a 16-coefficient model
    if (P == 0) return 0;
    K11Adam ad{};
    if (k11_adam_fill(ad, {xyz, scaling, rotation, features_dc, features_rest, opacity, cams, radii, cov3D, clamped,
                           dL_dmeans2D, dL_dconic_opacity, dL_drgb},
                      exp_avgs, exp_avg_sqs, lrs, beta1s, beta2s, epss, steps, grad_scale, dyn_dev, skip_flag_dev))
        return GSR_EINVAL;
    return k11_adam_launch(P, B, sh_degree, xyz, scaling, scale_modifier, rotation, features_dc, features_rest, opacity,
                           cams, width, height, radii, cov3D, clamped,
                           GradRecord{dL_dmeans2D, dL_dconic_opacity, dL_drgb, grad_row_stride}, ad, tanfov0, stream);
}

// The same launch with K10's fp64 sums and row flags as the gradient source (GradSums above; include/gsraster.h):
// acc64[c] / touched[c] are camera c's [P,9] sums and [P] flags, HOST tables of B <= 8 device pointers.
extern "C" int gsr_preprocess_backward_adam_raw_batched_sums(
    int P, int B, int sh_degree, int sh_coeffs, float *xyz, float *scaling, float scale_modifier, float *rotation,
    float *features_dc, float *features_rest, float *opacity, const float *cams, int width, int height,
    const int32_t *radii, const float *cov3D, const uint8_t *clamped, const double *const *acc64,
    const uint8_t *const *touched, float *const *exp_avgs, float *const *exp_avg_sqs, const double *lrs,
    const double *beta1s, const double *beta2s, const double *epss, const int64_t *steps, float grad_scale,
    const float *tanfov0, const float *dyn_dev, const uint32_t *skip_flag_dev, gsr_stream_t stream) {
    if (P < 0 || B < 1 || B > K11_SUMS_CAMS || sh_degree < 0 || sh_degree > 3 || sh_coeffs != 16 || width <= 0 ||
        height <= 0)
        return GSR_EINVAL;
    if (P == 0) return 0;
    if (!acc64 || !touched) return GSR_EINVAL;
    GradSums src{};
    for (int c = 0; c < K11_SUMS_CAMS; c++) {  // (the slots past B repeat the last camera: never read, never NULL)
        src.acc[c] = acc64[c < B ? c : B - 1];
        src.flags[c] = touched[c < B ? c : B - 1];
        if (!src.acc[c] || !src.flags[c] || ((uintptr_t)src.acc[c] & 7)) return GSR_EINVAL;
    }
    K11Adam ad{};
    if (k11_adam_fill(ad, {xyz, scaling, rotation, features_dc, features_rest, opacity, cams, radii, cov3D, clamped},
                      exp_avgs, exp_avg_sqs, lrs, beta1s, beta2s, epss, steps, grad_scale, dyn_dev, skip_flag_dev))
        return GSR_EINVAL;
    return k11_adam_launch(P, B, sh_degree, xyz, scaling, scale_modifier, rotation, features_dc, features_rest, opacity,
                           cams, width, height, radii, cov3D, clamped, src, ad, tanfov0, stream);
}

// The sparse (lazy) form of the fused launch: see the kernels above and include/gsraster.h.
extern "C" size_t gsr_sparse_step_workspace_bytes(int P) {
    return sizeof(SparseWs) + sizeof(uint32_t) * 2 * (((size_t)(P > 0 ? P : 1) + 1) / 2);  // a multiple of 8 bytes
}

extern "C" int gsr_preprocess_backward_adam_raw_batched_sparse(
    int P, int B, int sh_degree, int sh_coeffs, float *xyz, float *scaling, float scale_modifier, float *rotation,
    float *features_dc, float *features_rest, float *opacity, const float *cams, int width, int height,
    const int32_t *radii, const float *cov3D, const uint8_t *clamped, const float *dL_dmeans2D,
    const float *dL_dconic_opacity, const float *dL_drgb, int grad_row_stride, float *const *exp_avgs,
    float *const *exp_avg_sqs, const double *lrs, const double *beta1s, const double *beta2s, const double *epss,
    const int64_t *steps, float grad_scale, const float *dyn_dev, const uint32_t *skip_flag_dev, void *workspace,
    size_t workspace_bytes, uint8_t *active_out, uint32_t *num_active_dev, gsr_stream_t stream) {
    if (P < 0 || B < 1 || sh_degree < 0 || sh_degree > 3 || sh_coeffs != 16 || width <= 0 || height <= 0 ||
        grad_row_stride < 0 || (grad_row_stride != 0 && grad_row_stride < 9))
        return GSR_EINVAL;
    if (P == 0) return 0;
    if (!workspace) return GSR_EINVAL;
    K11Adam ad{};
    if (k11_adam_fill(ad, {xyz, scaling, rotation, features_dc, features_rest, opacity, cams, radii, cov3D, clamped,
                           dL_dmeans2D, dL_dconic_opacity, dL_drgb},
                      exp_avgs, exp_avg_sqs, lrs, beta1s, beta2s, epss, steps, grad_scale, dyn_dev, skip_flag_dev))
        return GSR_EINVAL;
    if ((uintptr_t)rotation & 15) return GSR_EINVAL;  // the quaternion is one 16-byte load
    if (grad_row_stride == 0 && (((uintptr_t)dL_dmeans2D & 7) || ((uintptr_t)dL_dconic_opacity & 15)))
        return GSR_EINVAL;  // dense gradients are read with 8- / 16-byte loads
    if (((uintptr_t)workspace & 7) || workspace_bytes < gsr_sparse_step_workspace_bytes(P)) return GSR_ENOSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    SparseWs *ws = static_cast<SparseWs *>(workspace);
    uint32_t *list = reinterpret_cast<uint32_t *>(ws + 1);
    hipLaunchKernelGGL(sparse_adam_reset_kernel, dim3(1), dim3(1), 0, st, skip_flag_dev, ws);
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sparse_adam_classify_kernel, dim3(gsr_div_up(P, SA_CROWS)), dim3(SA_CBLOCK), 0, st, P, B, radii,
                       dL_dmeans2D, dL_dconic_opacity, dL_drgb, grad_row_stride, skip_flag_dev, ws, list, active_out);
    GSR_LAUNCH_CHECK();
    const dim3 grid(gsr_div_up(P, K11_BLOCK)), block(K11_BLOCK);
    GSR_DISPATCH_DEG_AA(sh_degree, gsr_antialiasing_mode(),
                     hipLaunchKernelGGL((sparse_adam_update_kernel<DEG, AA>), grid, block, 0, st, P, B, xyz, scaling,
                                        scale_modifier, rotation, features_dc, features_rest, opacity, cams, width,
                                        height, radii, cov3D, clamped, dL_dmeans2D, dL_dconic_opacity, dL_drgb,
                                        grad_row_stride, ad, ws, list, num_active_dev));
    GSR_LAUNCH_CHECK();
    return 0;
}

// K11c (see the kernels above): dL_dcams [B][40] in the layout of `cams` for the B cameras of a batch.
extern "C" size_t gsr_preprocess_backward_cams_bytes(int P, int B) {
    const int nb = kc_blocks(P, 1);  // (the most row blocks any B takes: non-decreasing in P and in B)
    return (size_t)(nb > 0 ? nb : 1) * (size_t)(B > 0 ? B : 1) * KC_NS * sizeof(double);
}

extern "C" int gsr_preprocess_backward_cams(int P, int B, int sh_degree, int sh_coeffs, const float *means3D,
                                            const float *sh_dc, int sh_dc_stride, const float *sh_rest,
                                            int sh_rest_stride, const float *cams, int width, int height,
                                            const int32_t *radii, const float *cov3D, const uint8_t *clamped,
                                            const float *dL_dmeans2D, const float *dL_dconic_opacity,
                                            const float *dL_drgb, int grad_row_stride, void *workspace,
                                            size_t workspace_bytes, float *dL_dcams, gsr_stream_t stream) {
    if (P < 0 || B < 1 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < 1 ||
        sh_coeffs < (sh_degree + 1) * (sh_degree + 1) || width <= 0 || height <= 0 || sh_dc_stride < 0 ||
        sh_rest_stride < 0 || grad_row_stride < 0 || (grad_row_stride != 0 && grad_row_stride < 9) || !dL_dcams)
        return GSR_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (P == 0) {
        hipLaunchKernelGGL(preprocess_backward_cams_finalize_kernel, dim3(B), dim3(KC_FIN_SLICES * 32), 0, st, 0, B, nullptr,
                           dL_dcams);
        GSR_LAUNCH_CHECK();
        return 0;
    }
    if (gsr_antialiasing_mode() != 0)
        return GSR_EINVAL;  // the factor of the opacity depends on the pose too, and this entry point has no opacity
    if (!means3D || !sh_dc || (!sh_rest && sh_coeffs > 1) || !cams || !radii || !cov3D || !clamped || !dL_dmeans2D ||
        !dL_dconic_opacity || !dL_drgb || !workspace || ((uintptr_t)workspace & 7))
        return GSR_EINVAL;
    if (grad_row_stride == 0 && (((uintptr_t)dL_dmeans2D & 7) || ((uintptr_t)dL_dconic_opacity & 15)))
        return GSR_EINVAL;  // dense gradients are read with 8- / 16-byte loads
    if (sh_rest_stride < 3 * ((sh_degree + 1) * (sh_degree + 1) - 1))
        return GSR_EINVAL;  // a row of sh_rest holds less than the degree reads
    if (workspace_bytes < gsr_preprocess_backward_cams_bytes(P, B)) return GSR_ENOSPACE;
    const int nb = kc_blocks(P, B);
    double *partials = static_cast<double *>(workspace);
    const dim3 grid(8u * (unsigned)gsr_div_up(nb, 8) * (unsigned)B), block(KC_BLOCK);
    GSR_DISPATCH_DEG(sh_degree,
                     hipLaunchKernelGGL(preprocess_backward_cams_kernel<DEG>, grid, block, 0, st, P, B, nb, means3D,
                                        sh_rest, sh_rest_stride, cams, width, height, radii, cov3D, clamped,
                                        dL_dmeans2D, dL_dconic_opacity, dL_drgb, grad_row_stride, partials));
    GSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(preprocess_backward_cams_finalize_kernel, dim3(B), dim3(KC_FIN_SLICES * 32), 0, st, nb, B, partials,
                       dL_dcams);
    GSR_LAUNCH_CHECK();
    return 0;
}
