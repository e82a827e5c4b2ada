// api.hip -- the extern "C" entry points declared in include/gsraster.h (argument checking +
// dispatch to the kernels' launchers).  No torch types cross this boundary.
#include "common.h"

extern "C" {

const char *gsr_error_string(int code) {
    if (code == 0) return "success";
    if (code == GSR_EINVAL) return "gsraster: invalid argument";
    if (code == GSR_ENOSPACE) return "gsraster: workspace too small";
    if (code == GSR_ERETRY) return "gsraster: pair count valid, bounded sort must be repeated";
    if (code == GSR_EFAULT)
        return "gsraster: a persistent binning kernel of an earlier call timed out at a grid barrier (hung or preempted "
               "device); that view's lists are incomplete; the look-back pipeline is used from now on";
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "gsraster: unknown error";
}

int gsr_abi_version(void) { return 15; }

int gsr_get_block_xy(int *block_x, int *block_y, int *one_dim_block) {
    if (!block_x || !block_y || !one_dim_block) return GSR_EINVAL;
    *block_x = GSR_BLOCK_X;
    *block_y = GSR_BLOCK_Y;
    *one_dim_block = GSR_ONE_DIM_BLOCK;
    return 0;
}

int gsr_preprocess_forward(int P, int sh_degree, int sh_coeffs, const float *means3D, const float *scales,
                           float scale_modifier, const float *rotations, const float *shs, const float *opacities,
                           const float *viewmatrix, const float *projmatrix, const float *campos, int width,
                           int height, float tanfovx, float tanfovy, float *means2D, float *depths, int32_t *radii,
                           float *cov3D, float *conic_opacity, float *rgb, uint8_t *clamped, gsr_stream_t stream) {
    if (P < 0 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1) || width <= 0 ||
        height <= 0 || !(tanfovx > 0.f) || !(tanfovy > 0.f))
        return GSR_EINVAL;
    if (P == 0) return 0;
    if (!means3D || !scales || !rotations || !shs || !opacities || !viewmatrix || !projmatrix || !campos ||
        !means2D || !depths || !radii || !cov3D || !conic_opacity || !rgb || !clamped)
        return GSR_EINVAL;
    return gsr_launch_preprocess_forward(P, sh_degree, sh_coeffs, means3D, scales, scale_modifier, rotations, shs,
                                         nullptr, opacities, viewmatrix, projmatrix, campos, width, height, tanfovx, tanfovy,
                                         means2D, depths, radii, cov3D, conic_opacity, rgb, clamped,
                                         gsr_antialiasing_mode(), reinterpret_cast<hipStream_t>(stream));
}

int gsr_preprocess_backward(int P, int sh_degree, int sh_coeffs, const float *means3D, const float *scales,
                            float scale_modifier, const float *rotations, const float *shs, const float *viewmatrix,
                            const float *projmatrix, const float *campos, int width, int height, float tanfovx,
                            float tanfovy, const int32_t *radii, const float *cov3D, const uint8_t *clamped,
                            const float *dL_dmeans2D, const float *dL_dconic_opacity, const float *dL_drgb,
                            int grad_row_stride, float *dL_dmeans3D, float *dL_dscales, float *dL_drotations,
                            float *dL_dshs, float *dL_dopacities, gsr_stream_t stream) {
    if (P < 0 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1) || width <= 0 ||
        height <= 0 || !(tanfovx > 0.f) || !(tanfovy > 0.f) || grad_row_stride < 0)
        return GSR_EINVAL;
    if (P == 0) return 0;
    if (gsr_antialiasing_mode() != 0) return GSR_EINVAL;  // needs the opacity: gsr_preprocess_backward_aa
    if (!means3D || !scales || !rotations || !shs || !viewmatrix || !projmatrix || !campos || !radii || !cov3D ||
        !clamped || !dL_dmeans2D || !dL_dconic_opacity || !dL_drgb || !dL_dmeans3D || !dL_dscales || !dL_drotations ||
        !dL_dshs || !dL_dopacities)
        return GSR_EINVAL;
    return gsr_launch_preprocess_backward(P, sh_degree, sh_coeffs, means3D, scales, scale_modifier, rotations, shs,
                                          nullptr, nullptr, viewmatrix, projmatrix, campos, width, height, tanfovx, tanfovy, radii,
                                          cov3D, clamped, dL_dmeans2D, dL_dconic_opacity, dL_drgb, grad_row_stride,
                                          dL_dmeans3D, dL_dscales, dL_drotations, dL_dshs, nullptr, dL_dopacities, 0,
                                          reinterpret_cast<hipStream_t>(stream));
}

int gsr_preprocess_backward_aa(int P, int sh_degree, int sh_coeffs, const float *means3D, const float *scales,
                               float scale_modifier, const float *rotations, const float *shs, const float *opacities,
                               const float *viewmatrix, const float *projmatrix, const float *campos, int width,
                               int height, float tanfovx, float tanfovy, const int32_t *radii, const float *cov3D,
                               const uint8_t *clamped, const float *dL_dmeans2D, const float *dL_dconic_opacity,
                               const float *dL_drgb, int grad_row_stride, float *dL_dmeans3D, float *dL_dscales,
                               float *dL_drotations, float *dL_dshs, float *dL_dopacities, gsr_stream_t stream) {
    if (P < 0 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1) || width <= 0 ||
        height <= 0 || !(tanfovx > 0.f) || !(tanfovy > 0.f) || grad_row_stride < 0)
        return GSR_EINVAL;
    if (P == 0) return 0;
    const int aa = gsr_antialiasing_mode();
    if (!means3D || !scales || !rotations || !shs || (aa && !opacities) || !viewmatrix || !projmatrix || !campos ||
        !radii || !cov3D || !clamped || !dL_dmeans2D || !dL_dconic_opacity || !dL_drgb || !dL_dmeans3D || !dL_dscales ||
        !dL_drotations || !dL_dshs || !dL_dopacities)
        return GSR_EINVAL;
    return gsr_launch_preprocess_backward(P, sh_degree, sh_coeffs, means3D, scales, scale_modifier, rotations, shs,
                                          nullptr, aa ? opacities : nullptr, viewmatrix, projmatrix, campos, width,
                                          height, tanfovx, tanfovy, radii, cov3D, clamped, dL_dmeans2D,
                                          dL_dconic_opacity, dL_drgb, grad_row_stride, dL_dmeans3D, dL_dscales,
                                          dL_drotations, dL_dshs, nullptr, dL_dopacities, aa,
                                          reinterpret_cast<hipStream_t>(stream));
}

int gsr_preprocess_forward_raw(int P, int sh_degree, int sh_coeffs, const float *xyz, const float *scaling,
                               float scale_modifier, const float *rotation, const float *features_dc,
                               const float *features_rest, const float *opacity, const float *viewmatrix,
                               const float *projmatrix, const float *campos, int width, int height, float tanfovx,
                               float tanfovy, float *means2D, float *depths, int32_t *radii, float *cov3D,
                               float *conic_opacity, float *rgb, uint8_t *clamped, gsr_stream_t stream) {
    if (P < 0 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < 2 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1) ||
        width <= 0 || height <= 0 || !(tanfovx > 0.f) || !(tanfovy > 0.f))
        return GSR_EINVAL;
    if (P == 0) return 0;
    if (!xyz || !scaling || !rotation || !features_dc || !features_rest || !opacity || !viewmatrix || !projmatrix ||
        !campos || !means2D || !depths || !radii || !cov3D || !conic_opacity || !rgb || !clamped)
        return GSR_EINVAL;
    return gsr_launch_preprocess_forward(P, sh_degree, sh_coeffs, xyz, scaling, scale_modifier, rotation, features_dc,
                                         features_rest, opacity, viewmatrix, projmatrix, campos, width, height,
                                         tanfovx, tanfovy, means2D, depths, radii, cov3D, conic_opacity, rgb, clamped,
                                         gsr_antialiasing_mode(), reinterpret_cast<hipStream_t>(stream));
}

int gsr_preprocess_backward_raw(int P, int sh_degree, int sh_coeffs, const float *xyz, const float *scaling,
                                float scale_modifier, const float *rotation, const float *features_dc,
                                const float *features_rest, const float *opacity, const float *viewmatrix,
                                const float *projmatrix, const float *campos, int width, int height, float tanfovx,
                                float tanfovy, const int32_t *radii, const float *cov3D, const uint8_t *clamped,
                                const float *dL_dmeans2D, const float *dL_dconic_opacity, const float *dL_drgb,
                                int grad_row_stride, float *dL_dxyz, float *dL_dscaling, float *dL_drotation,
                                float *dL_dfeatures_dc, float *dL_dfeatures_rest, float *dL_dopacity,
                                gsr_stream_t stream) {
    if (P < 0 || sh_degree < 0 || sh_degree > 3 || sh_coeffs < 2 || sh_coeffs < (sh_degree + 1) * (sh_degree + 1) ||
        width <= 0 || height <= 0 || !(tanfovx > 0.f) || !(tanfovy > 0.f) || grad_row_stride < 0)
        return GSR_EINVAL;
    if (P == 0) return 0;
    if (!xyz || !scaling || !rotation || !features_dc || !features_rest || !opacity || !viewmatrix || !projmatrix ||
        !campos || !radii || !cov3D || !clamped || !dL_dmeans2D || !dL_dconic_opacity || !dL_drgb || !dL_dxyz ||
        !dL_dscaling || !dL_drotation || !dL_dfeatures_dc || !dL_dfeatures_rest || !dL_dopacity)
        return GSR_EINVAL;
    return gsr_launch_preprocess_backward(P, sh_degree, sh_coeffs, xyz, scaling, scale_modifier, rotation, features_dc,
                                          features_rest, opacity, viewmatrix, projmatrix, campos, width, height,
                                          tanfovx, tanfovy, radii, cov3D, clamped, dL_dmeans2D, dL_dconic_opacity,
                                          dL_drgb, grad_row_stride, dL_dxyz, dL_dscaling, dL_drotation, dL_dfeatures_dc,
                                          dL_dfeatures_rest, dL_dopacity, gsr_antialiasing_mode(),
                                          reinterpret_cast<hipStream_t>(stream));
}

int gsr_get_local2j_ids_bool(int P, int width, int height, int world_size, const float *means2D,
                             const int32_t *radii, const int32_t *dist_global_strategy, uint8_t *out,
                             gsr_stream_t stream) {
    if (P < 0 || width <= 0 || height <= 0 || world_size <= 0) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!means2D || !radii || !dist_global_strategy || !out) return GSR_EINVAL;
    return gsr_launch_local2j(P, width, height, world_size, means2D, radii, dist_global_strategy, out,
                              reinterpret_cast<hipStream_t>(stream));
}

size_t gsr_render_seg_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return gsr_composite_seg_bytes(width, height);
}

int gsr_render_forward(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                       const float *means2D, const float *conic_opacity, const float *rgb,
                       const uint8_t *compute_locally, const float *bg, float *out_color, float *final_T,
                       int32_t *n_contrib, void *seg_ws, size_t seg_bytes, int row_lo, int row_hi, void *zero_ptr,
                       size_t zero_bytes, gsr_stream_t stream) {
    if (P < 0 || width <= 0 || height <= 0) return GSR_EINVAL;
    if (!ranges || !compute_locally || !bg || !out_color || !final_T || !n_contrib) return GSR_EINVAL;
    if (P > 0 && (!means2D || !conic_opacity || !rgb)) return GSR_EINVAL;
    return gsr_launch_composite_forward(P, width, height, ranges, point_list, means2D, conic_opacity, rgb,
                                        compute_locally, bg, out_color, final_T, n_contrib, seg_ws, seg_bytes, row_lo,
                                        row_hi, zero_ptr, zero_bytes, reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_backward(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                        const float *means2D, const float *conic_opacity, const float *rgb,
                        const uint8_t *compute_locally, const float *bg, const float *final_T,
                        const int32_t *n_contrib, const float *dL_dpixels, float *dL_record, const float *out_color,
                        void *seg_ws, size_t seg_bytes, int row_lo, int row_hi, int record_is_zero, double *acc64,
                        uint8_t *touched, gsr_stream_t stream) {
    if (P < 0 || width <= 0 || height <= 0) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!ranges || !compute_locally || !bg || !final_T || !n_contrib || !dL_dpixels || !means2D || !conic_opacity ||
        !rgb || !dL_record || !acc64)
        return GSR_EINVAL;
    return gsr_launch_composite_backward(P, width, height, ranges, point_list, means2D, conic_opacity, rgb,
                                         compute_locally, bg, final_T, n_contrib, dL_dpixels, dL_record, out_color,
                                         seg_ws, seg_bytes, row_lo, row_hi, record_is_zero ? 1 : 0, acc64, touched, 1,
                                         reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_backward_sums(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                             const float *means2D, const float *conic_opacity, const float *rgb,
                             const uint8_t *compute_locally, const float *bg, const float *final_T,
                             const int32_t *n_contrib, const float *dL_dpixels, const float *out_color, void *seg_ws,
                             size_t seg_bytes, int row_lo, int row_hi, double *acc64, uint8_t *touched,
                             gsr_stream_t stream) {
    if (P < 0 || width <= 0 || height <= 0) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!ranges || !compute_locally || !bg || !final_T || !n_contrib || !dL_dpixels || !means2D || !conic_opacity ||
        !rgb || !acc64 || !touched)
        return GSR_EINVAL;
    return gsr_launch_composite_backward(P, width, height, ranges, point_list, means2D, conic_opacity, rgb,
                                         compute_locally, bg, final_T, n_contrib, dL_dpixels, nullptr, out_color,
                                         seg_ws, seg_bytes, row_lo, row_hi, 1, acc64, touched, 0,
                                         reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_record_materialize(int P, const double *acc64, const uint8_t *touched, float *dL_record,
                                  int record_is_zero, gsr_stream_t stream) {
    if (P < 0) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!acc64 || !touched || !dL_record) return GSR_EINVAL;
    return gsr_launch_record_materialize(P, acc64, touched, dL_record, record_is_zero ? 1 : 0,
                                         reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_contrib(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                       const float *means2D, const float *conic_opacity, const uint8_t *compute_locally,
                       const int32_t *n_contrib, int row_lo, int row_hi, int64_t *hits, float *wmax, double *wsum,
                       gsr_stream_t stream) {
    if (P < 0 || width <= 0 || height <= 0) return GSR_EINVAL;
    if (P == 0) return 0;
    // (point_list may be NULL: every list can be empty)
    if (!ranges || !means2D || !conic_opacity || !compute_locally || !n_contrib || !hits || !wmax || !wsum)
        return GSR_EINVAL;
    return gsr_launch_composite_contrib(P, width, height, ranges, point_list, means2D, conic_opacity, compute_locally,
                                        n_contrib, row_lo, row_hi, hits, wmax, wsum,
                                        reinterpret_cast<hipStream_t>(stream));
}

int gsr_contrib_merge_rows(int64_t n, const int32_t *idx, const int64_t *src_hits, const float *src_wmax,
                           const double *src_wsum, int64_t *dst_hits, float *dst_wmax, double *dst_wsum,
                           gsr_stream_t stream) {
    if (n < 0) return GSR_EINVAL;
    if (n == 0) return 0;
    if (!idx || !src_hits || !src_wmax || !src_wsum || !dst_hits || !dst_wmax || !dst_wsum) return GSR_EINVAL;
    return gsr_launch_contrib_merge_rows(n, idx, src_hits, src_wmax, src_wsum, dst_hits, dst_wmax, dst_wsum,
                                         reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_invdepth(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                        const float *means2D, const float *conic_opacity, const float *depths,
                        const uint8_t *compute_locally, const int32_t *n_contrib, int row_lo, int row_hi,
                        float *invdepth, gsr_stream_t stream) {
    if (P < 0 || width <= 0 || height <= 0 || !invdepth) return GSR_EINVAL;
    // (point_list may be NULL: every list can be empty)
    if (P > 0 && (!ranges || !means2D || !conic_opacity || !depths || !compute_locally || !n_contrib)) return GSR_EINVAL;
    return gsr_launch_composite_invdepth(P, width, height, ranges, point_list, means2D, conic_opacity, depths,
                                         compute_locally, n_contrib, row_lo, row_hi, invdepth,
                                         reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_invdepth_backward(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                                 const float *means2D, const float *conic_opacity, const float *depths,
                                 const uint8_t *compute_locally, const int32_t *n_contrib, const float *final_T,
                                 const float *invdepth, const float *dL_dinvdepth, int row_lo, int row_hi,
                                 float *dL_record, double *acc64, gsr_stream_t stream) {
    if (P < 0 || width <= 0 || height <= 0) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!ranges || !means2D || !conic_opacity || !depths || !compute_locally || !n_contrib || !final_T || !invdepth ||
        !dL_dinvdepth || !dL_record || !acc64)
        return GSR_EINVAL;
    // (the walk goes back to front from final_T, as K10's does: the forward's map is part of the interface, not read)
    return gsr_launch_composite_invdepth_backward(P, width, height, ranges, point_list, means2D, conic_opacity, depths,
                                                  compute_locally, n_contrib, final_T, dL_dinvdepth, row_lo, row_hi,
                                                  dL_record, acc64, reinterpret_cast<hipStream_t>(stream));
}

int gsr_depth_backward_means3d(int P, const int32_t *radii, const float *viewmatrix, const float *dL_ddepth,
                               int row_stride, float *dL_dmeans3D, int overwrite, gsr_stream_t stream) {
    if (P < 0 || row_stride < 1) return GSR_EINVAL;
    if (P == 0) return 0;
    if (!radii || !viewmatrix || !dL_ddepth || !dL_dmeans3D) return GSR_EINVAL;
    return gsr_launch_depth_to_means3D(P, radii, viewmatrix, dL_ddepth, row_stride, dL_dmeans3D, overwrite ? 1 : 0,
                                       reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_features(int P, int C, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                        const float *means2D, const float *conic_opacity, const float *features,
                        const uint8_t *compute_locally, const int32_t *n_contrib, int row_lo, int row_hi, float *out,
                        gsr_stream_t stream) {
    if (P < 0 || C < 1 || C > GSR_FEATURES_MAX || width <= 0 || height <= 0 || !out) return GSR_EINVAL;
    // (point_list may be NULL: every list can be empty)
    if (P > 0 && (!ranges || !means2D || !conic_opacity || !features || !compute_locally || !n_contrib)) return GSR_EINVAL;
    return gsr_launch_composite_features(P, C, width, height, ranges, point_list, means2D, conic_opacity, features,
                                         compute_locally, n_contrib, row_lo, row_hi, out,
                                         reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_features_backward(int P, int C, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                                 const float *means2D, const float *conic_opacity, const float *features,
                                 const uint8_t *compute_locally, const int32_t *n_contrib, const float *final_T,
                                 const float *dL_dout, int row_lo, int row_hi, float *dL_record, float *dL_dfeatures,
                                 double *acc64, gsr_stream_t stream) {
    if (P < 0 || C < 1 || C > GSR_FEATURES_MAX || width <= 0 || height <= 0) return GSR_EINVAL;
    if (P == 0) return 0;
    // (dL_dfeatures may be NULL: the feature gradient is then not formed)
    if (!ranges || !means2D || !conic_opacity || !features || !compute_locally || !n_contrib || !final_T || !dL_dout ||
        !dL_record || !acc64)
        return GSR_EINVAL;
    return gsr_launch_composite_features_backward(P, C, width, height, ranges, point_list, means2D, conic_opacity,
                                                  features, compute_locally, n_contrib, final_T, dL_dout, row_lo, row_hi,
                                                  dL_record, dL_dfeatures, acc64, reinterpret_cast<hipStream_t>(stream));
}

int gsr_render_absgrad(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                       const float *means2D, const float *conic_opacity, const float *rgb,
                       const uint8_t *compute_locally, const float *bg, const float *final_T, const int32_t *n_contrib,
                       const float *dL_dpixels, int row_lo, int row_hi, float *absgrad, double *acc64,
                       gsr_stream_t stream) {
    if (P < 0 || width <= 0 || height <= 0) return GSR_EINVAL;
    if (P == 0) return 0;
    // (point_list may be NULL: every list can be empty)
    if (!ranges || !means2D || !conic_opacity || !rgb || !compute_locally || !bg || !final_T || !n_contrib ||
        !dL_dpixels || !absgrad || !acc64)
        return GSR_EINVAL;
    return gsr_launch_composite_absgrad(P, width, height, ranges, point_list, means2D, conic_opacity, rgb,
                                        compute_locally, bg, final_T, n_contrib, dL_dpixels, row_lo, row_hi, absgrad,
                                        acc64, reinterpret_cast<hipStream_t>(stream));
}

int gsr_absgrad_merge_rows(int64_t n, const int32_t *idx, const float *src, float *dst, gsr_stream_t stream) {
    if (n < 0) return GSR_EINVAL;
    if (n == 0) return 0;
    if (!idx || !src || !dst) return GSR_EINVAL;
    return gsr_launch_absgrad_merge_rows((long long)n, idx, src, dst, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
