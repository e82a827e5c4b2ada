/*
 * gsraster.h -- C-ABI of the MI355X (gfx950) Gaussian-splatting rasterizer: the drop-in boundary.
 *
 * Every entry point below is what the reference's Python wrapper module
 * `diff_gaussian_rasterization` (un-vendored submodule, .gitmodules:4-6 of the reference) binds
 * through its `_C` extension for the hot path; the reference-side call sites are cited per function
 * (paths relative to the reference root).  The host-side mirror that re-creates the reference's
 * operator surface on top of this ABI is grendel-gs_amd/diff_gaussian_rasterization/__init__.py;
 * the binding a maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - all data pointers are DEVICE pointers (HBM) unless the name ends in `_host`;
 *  - fp32 / int32 / uint8, dense row-major ("contiguous") layouts, shapes in the comments;
 *  - `stream` is a hipStream_t passed as void* (0 = the null stream); every call only ENQUEUES
 *    work on that stream unless stated otherwise;
 *  - return value: 0 on success, otherwise a hipError_t value (>0) or a GSR_E* code (<0);
 *    gsr_error_string() explains either.  No call aborts the process.
 *  - matrices are in the reference's row-vector convention (scene/cameras.py:84-100):
 *    p_view = [p,1] @ viewmatrix, p_clip = [p,1] @ projmatrix, both 4x4 row-major.
 *  - tiles are 16x16 pixels (utils/general_utils.py:78-93); tile id = ty * tiles_x + tx.
 */
#ifndef GSRASTER_H
#define GSRASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_BLOCK_X 16
#define GSR_BLOCK_Y 16
#define GSR_ONE_DIM_BLOCK 256

#define GSR_EINVAL (-1)   /* bad argument (negative size, null pointer, sh_degree > 3, ...) */
#define GSR_ENOSPACE (-2) /* caller-provided workspace too small */
#define GSR_ERETRY (-3)   /* gsr_bin_count_wait: the count is valid, but a gsr_bin_sort_bounded launched for it wrote nothing */
#define GSR_EFAULT (-4)   /* a persistent binning kernel of an EARLIER call gave up at a barrier behind its first one (a hung or
                             heavily preempted device): that call's lists are incomplete (in bounds); reported once, the
                             device keeps to the look-back pipeline afterwards (gsr_bin_persist_status has the code) */

typedef void *gsr_stream_t;

const char *gsr_error_string(int code);

/* ABI version of this library (bumped when a signature changes or a symbol is removed; new symbols alone do not). */
int gsr_abi_version(void);

/* `_C.get_block_XY()` -- arguments/__init__.py:254-257.  Always (16, 16, 256). */
int gsr_get_block_xy(int *block_x, int *block_y, int *one_dim_block);

/* ---------------------------------------------------------------------------------------------
 * K1  preprocess forward -- GaussianRasterizer.preprocess_gaussians,
 *     gaussian_renderer/__init__.py:949-956 (outputs consumed at :960).
 * in : means3D [P,3], scales [P,3] (activated), rotations [P,4] (r,x,y,z, normalised),
 *      shs [P,sh_coeffs,3], opacities [P] (activated), viewmatrix/projmatrix [4,4], campos [3]
 * out: means2D [P,2] (pixels), depths [P], radii int32 [P] (0 = culled), cov3D [P,6],
 *      conic_opacity [P,4] = (A,B,C,opacity), rgb [P,3], clamped uint8 [P,3]
 * Culled Gaussians get radii 0 and zeros everywhere else. */
int gsr_preprocess_forward(int P, int sh_degree, int sh_coeffs, const float *means3D, const float *scales,
                           float scale_modifier, const float *rotations, const float *shs, const float *opacities,
                           const float *viewmatrix, const float *projmatrix, const float *campos, int width,
                           int height, float tanfovx, float tanfovy, float *means2D, float *depths, int32_t *radii,
                           float *cov3D, float *conic_opacity, float *rgb, uint8_t *clamped, gsr_stream_t stream);

/* K11 preprocess backward -- autograd backward of the call above (train_internal.py:194-196).
 * in : the forward inputs, the saved radii / cov3D / clamped, and the incoming gradients
 *      dL_dmeans2D [P,2] (NDC-scaled units, scene/gaussian_model.py:1046-1064),
 *      dL_dconic_opacity [P,4] (true partials wrt A,B,C,opacity), dL_drgb [P,3].
 *      grad_row_stride == 0: the three are dense; > 0: each pointer addresses a column block of rows that are
 *      grad_row_stride floats apart (e.g. columns 0, 5 and 2 of gsr_render_backward's [P,9] record, stride 9),
 *      so K10's output feeds K11 without a repacking pass
 * out: dL_dmeans3D [P,3], dL_dscales [P,3], dL_drotations [P,4], dL_dshs [P,sh_coeffs,3],
 *      dL_dopacities [P]   (fully overwritten, zeros for culled Gaussians) */
int gsr_preprocess_backward(int P, int sh_degree, int sh_coeffs, const float *means3D, const float *scales,
                            float scale_modifier, const float *rotations, const float *shs, const float *viewmatrix,
                            const float *projmatrix, const float *campos, int width, int height, float tanfovx,
                            float tanfovy, const int32_t *radii, const float *cov3D, const uint8_t *clamped,
                            const float *dL_dmeans2D, const float *dL_dconic_opacity, const float *dL_drgb,
                            int grad_row_stride, float *dL_dmeans3D, float *dL_dscales, float *dL_drotations,
                            float *dL_dshs, float *dL_dopacities, gsr_stream_t stream);

/* Anti-aliased splatting: opacity compensation in K1 / K11 (the 2D Mip filter of Mip-Splatting, the `antialiasing`
 * switch of later 3DGS rasterizers).  No reference call site: the reference dilates every projected covariance by
 * 0.3 px^2 and leaves the opacity alone, so a Gaussian far smaller than a pixel is drawn as a 0.55 px blob at its full
 * opacity.  Process-wide switch, read ONCE per call, on the host, by every K1 / K11 entry point of this header (the
 * activated, raw, camera-batched, fused K11 + Adam, _dyn and sparse forms): a launch already enqueued or captured keeps
 * the mode it was launched with.  mode 0 (default): the reference's behaviour, bit for bit.  mode 1, for a visible row
 * (radii > 0) and one camera, with a0, b, c0 = T Sigma T^T BEFORE the dilation:
 *   det0 = a0 c0 - b^2;  a = a0 + 0.3, c = c0 + 0.3, det = a c - b^2 (the value the conic is made of);  q = det0 / det;
 *   rho = sqrt(max(0.000025, q)), so 0.005 <= rho < 1.
 * Forward: conic_opacity.w = opacity * rho (opacity: activated, uncompensated); every other output keeps its bits --
 *   radii, conic, depths, rgb, clamped, cov3D -- and culled rows stay all zero.
 * Backward, g = dL/dconic_opacity.w: dL/dopacity = g rho (the raw forms then multiply by the sigmoid's derivative, as
 *   before); if q > 0.000025, w = g opacity / (2 rho) times dq/d(a, b, c) is added to the conic's dL/d(a, b, c) before
 *   these go on to Sigma, T and t, so scales, rotation and mean all receive it; if q <= 0.000025 nothing is added.  With
 *   h = det - det0 = 0.3 (a0 + c0) + 0.09:
 *     dq/da = (0.3 (c0^2 + b^2) + 0.09 c0) / det^2,  dq/dc = (0.3 (a0^2 + b^2) + 0.09 a0) / det^2,
 *     dq/db = -2 b h / det^2   (b: the one scalar in both off-diagonal places, as dL/db already is)
 *   in these closed forms (the quotient rule cancels for large splats) and with the true 1 / det^2; the conic part keeps
 *   its 1 / (det^2 + 1e-7).
 * Nothing else changes: binning, composite, exchange and loss see the compensated opacity where they saw the opacity.
 * -> the previous mode, or GSR_EINVAL for a mode other than 0 and 1 (the mode is then unchanged).
 * Under mode 1 gsr_preprocess_backward and gsr_preprocess_backward_cams return GSR_EINVAL (for P > 0, before any device
 * work) rather than an incomplete gradient: the activated K11 needs the opacity (gsr_preprocess_backward_aa below), and
 * camera-pose gradients under anti-aliasing -- rho depends on the pose as well, and the _cams entry point has no opacity
 * input -- are not implemented. */
int gsr_set_antialiasing(int mode);
/* gsr_preprocess_backward with `opacities` [P] (activated, the forward's input) behind `shs`.  Mode 1: K11 as defined
 * above.  Mode 0: `opacities` is not read (may be NULL) and the results are gsr_preprocess_backward's bits. */
int gsr_preprocess_backward_aa(int P, int sh_degree, int sh_coeffs, const float *means3D, const float *scales,
                               float scale_modifier, const float *rotations, const float *shs, const float *opacities,
                               const float *viewmatrix, const float *projmatrix, const float *campos, int width,
                               int height, float tanfovx, float tanfovy, const int32_t *radii, const float *cov3D,
                               const uint8_t *clamped, const float *dL_dmeans2D, const float *dL_dconic_opacity,
                               const float *dL_drgb, int grad_row_stride, float *dL_dmeans3D, float *dL_dscales,
                               float *dL_drotations, float *dL_dshs, float *dL_dopacities, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2 `_C.get_local2j_ids_bool` -- gaussian_renderer/workload_division.py:721-744.
 * dist_global_strategy int32 [world_size+1]: band j owns flattened tile ids [d[j], d[j+1]).
 * out uint8 (bool) [P, world_size]: Gaussian i must be sent to band j. */
int gsr_get_local2j_ids_bool(int P, int width, int height, int world_size, const float *means2D,
                             const int32_t *radii, const int32_t *dist_global_strategy, uint8_t *out,
                             gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K3-K7  binning of one camera's (received) Gaussians into the locally computed tiles, in two
 * calls because the number of (tile, Gaussian) pairs D ("num_rendered") sizes the second one.
 * Part of GaussianRasterizer.render_gaussians, gaussian_renderer/__init__.py:1271-1282.
 *
 * gsr_bin_prepare : per Gaussian, count the locally computed tiles it can contribute to (its 3-sigma
 *   rect intersected with the box around its alpha >= 1/255 ellipse: tiles outside that box get
 *   nothing under the alpha < 1/255 rule, so dropping them changes no pixel), order the
 *   Gaussians by depth (stable) and prefix-sum the counts in that order.  Writes D to
 *   *num_rendered_host once the device has produced it (the one host wait of the render op: the host polls a
 *   pinned word the last workgroup writes, and falls back to synchronising `stream` after 2 ms).
 *   `prep` is an opaque device workspace of gsr_bin_prepare_bytes(P, width, height) bytes that must stay
 *   untouched until gsr_bin_sort returns.
 * gsr_bin_sort    : emit the D pairs in depth order and stable-sort them by tile id, giving
 *   point_list uint32 [D] (Gaussian index per pair, grouped by tile, front-to-back inside a
 *   tile, ties by Gaussian index) and ranges int32 [tiles + 1, 2]: rows 0 .. tiles-1 = [start,end) per tile, row `tiles`
 *   = [lo, hi) the tile ROWS that contain locally computed tiles (the band this rank renders; (0,0) when there is
 *   none or P is 0; also written when D is 0) -- gsr_render_forward / _backward read it to spread the band, not the
 *   whole grid, over the eight XCDs.
 *   The caller allocates tiles + 1 rows (ABI 7).
 *   `scratch` is a device workspace of gsr_bin_sort_bytes(P, D, width, height) bytes. */
size_t gsr_bin_prepare_bytes(int P, int width, int height);
int gsr_bin_prepare(int P, int width, int height, const float *means2D, const float *depths, const int32_t *radii,
                    const float *conic_opacity, const uint8_t *compute_locally, void *prep, size_t prep_bytes,
                    int64_t *num_rendered_host, gsr_stream_t stream);
size_t gsr_bin_sort_bytes(int P, int64_t num_rendered, int width, int height);
int gsr_bin_sort(int P, int width, int height, const uint8_t *compute_locally, const void *prep,
                 int64_t num_rendered, void *scratch, size_t scratch_bytes, uint32_t *point_list, int32_t *ranges,
                 gsr_stream_t stream);
/* The same two steps WITHOUT the idle GPU between them.  The reference's rasterizer (and gsr_bin_prepare above) reads
 * num_rendered back to size its sort buffers, and the GPU has nothing to do until the host has seen the count and
 * launched the sort (~25-35 us per view).  Callers that keep a grow-only scratch can instead
 *   gsr_bin_prepare_async  : launch K3-K4; `*ticket` identifies the count (0 = P was 0, the count is 0);
 *   gsr_bin_sort_bounded   : launch the sort for up to `capacity` pairs -- the kernels read the pair count D from the
 *                            prep workspace ON THE DEVICE and do nothing past it; if D > capacity they write nothing
 *                            useful, and the caller, who learns D from gsr_bin_count_wait, must run gsr_bin_sort with
 *                            buffers of the right size.  point_list must hold `capacity` words.  Only frames of
 *                            <= 256 x 256 tiles (GSR_EINVAL otherwise: use gsr_bin_sort);
 *   gsr_bin_count_wait     : the pair count of `ticket` (polls a pinned word; up to 64 counts may be outstanding per
 *                            device);
 *   gsr_bin_sort_capacity  : the largest num_rendered whose gsr_bin_sort_bytes fits `scratch_bytes` (0 when bounded
 *                            launches do not apply to this frame size). */
/* Process-wide switch for the order of Gaussians with EXACTLY equal depth inside a tile list.  0 (default): by their
 * index in the arrays the op is given -- the reference's order; at world size > 1 that index is (source rank, index on
 * the source), gaussian_renderer/__init__.py:624-640, so the tie order depends on how the Gaussians are sharded.
 * 1: by screen position (means2D.x, then .y, then index): independent of the number of ranks and of the order of the
 * Gaussians; one extra P-sized kernel in gsr_bin_prepare*.  Takes effect for subsequent gsr_bin_prepare* calls. */
int gsr_set_depth_tie_order(int mode);
int gsr_bin_prepare_async(int P, int width, int height, const float *means2D, const float *depths, const int32_t *radii,
                          const float *conic_opacity, const uint8_t *compute_locally, void *prep, size_t prep_bytes,
                          uint32_t *ticket, gsr_stream_t stream);
int gsr_bin_count_wait(uint32_t ticket, int64_t *num_rendered_host, gsr_stream_t stream);
int64_t gsr_bin_sort_capacity(int P, size_t scratch_bytes, int width, int height);
/* The first two calls above as ONE host-side call per view: prepare, then -- `capacity` > 0 -- the bounded sort into
 * (scratch, point_list [capacity]); *ticket names the pair count for gsr_bin_count_wait, *sorted = 1 when the bounded
 * sort was launched.  Lists and ranges are complete when *sorted = 1, gsr_bin_count_wait returns 0 and the count is
 * <= capacity; otherwise (no capacity given, the count outgrew it, or the persistent prepare kernel had to repeat itself
 * -- gsr_bin_count_wait returns GSR_ERETRY, see gsr_set_bin_persistent) the caller runs gsr_bin_sort with buffers for the
 * counted pairs.  The kernels that consume the lists (K8, K10) read the range table, never the count, so the caller
 * launches them FIRST and looks at the count afterwards: in the incomplete case the bounded sort wrote nothing and left
 * every range empty -- the consumer drew the background -- and the caller repeats gsr_bin_sort + the consumer with exact
 * sizes.
 * Stands where the reference's rasterizer reads `num_rendered` back between its sort-key emission and its sort
 * (analyze_statistic.py:1972-1991 stage list: "24 updateDistributedStatLocally.updateTileTouched" -> "50 SortPairs"). */
int gsr_bin_speculative_async(int P, int width, int height, const float *means2D, const float *depths,
                              const int32_t *radii, const float *conic_opacity, const uint8_t *compute_locally, void *prep,
                              size_t prep_bytes, int64_t capacity, void *scratch, size_t scratch_bytes,
                              uint32_t *point_list, int32_t *ranges, uint32_t *ticket, int *sorted, gsr_stream_t stream);
/* K3-K7 run as TWO persistent launches whose workgroups meet at grid-wide barriers (ABI 11; csrc/binning_persist.h)
 * instead of the nine launches of the look-back pipeline, when the device can hold the grid at once, the frame has
 * <= 256 x 256 tiles and P <= 8 x 4096 x CUs.  Lists, ranges and offsets are bit-identical.  A barrier kernel needs
 * its whole grid resident: the library never has two of them in flight on different streams of one process (the second
 * call takes the look-back pipeline); a device shared with ANOTHER PROCESS's barrier kernel is covered by a time-out at
 * the first barrier -- the prepare step then repeats itself on the look-back pipeline inside gsr_bin_count_wait, which
 * returns GSR_ERETRY (the count is valid; a gsr_bin_sort_bounded already launched for it wrote nothing: call
 * gsr_bin_sort); in the sort step the time-out (250 ms) is decided for the whole grid, every workgroup but one leaves and
 * that one sorts the view alone inside the same launch -- correct lists, no host round trip, works in a captured graph --
 * after which the next 64 sorts of the device take the look-back pipeline (ABI 12; ABI 11 trapped here).  No kernel of
 * this library traps: a time-out at a LATER barrier (whole grid resident: a hung or preempted device) leaves a code in the
 * status words and the next binning call on the device returns GSR_EFAULT.  mode: -1 the environment's GSR_BIN_PERSIST (0 | 1 | p | s,
 * default 1), 0 off, 1 prepare only, 2 sort only, 3 both. */
int gsr_set_bin_persistent(int mode);
/* K5-K7 with ONE pass over the D (tile, Gaussian) pairs (ABI 12; csrc/binning_rows.h): the h ROW SEGMENTS of every rect
 * (R = sum of heights ~ D / 3..6) are sorted stably by tile row, the pairs are emitted from that order and scattered
 * stably by column inside their row, straight into point_list; the ranges follow from per-tile counts.  Replaces the two
 * D-sized sort passes + K7 of the split-key pipelines (their ranking is bound by VALU issue at every size: 0.28-0.33 of
 * the HBM peak) where it applies: frames of <= 256 x 256 tiles, uncut rects (gsr_set_tile_cull off).  Lists, ranges and
 * counts are bit-identical.  mode: -1 the environment's GSR_BIN_ROWS (0 | 1, default 1), 0 off, 1 on.
 * Reference stages replaced: 40 duplicateWithKeys, 50 SortPairs, 60 identifyTileRanges (analyze_statistic.py:1972-1991). */
int gsr_set_bin_rowmajor(int mode);
/* Exact tile culling in K3 (ABI 11; csrc/binning_persist.h: gsr_tile_mask): per tile row of a Gaussian's rect the exact span
 * of tiles its alpha >= 1/255 ellipse reaches (the quadratic form and tolerance of the composite kernels' own skip test),
 * kept as a 64-bit mask (rects of <= 64 tiles on frames of <= 256 x 256 tiles).  The lists stay order-preserving
 * subsequences of the uncut ones -- a dropped (tile, Gaussian) has alpha < 1/255 on every pixel of the tile -- so the image
 * and the gradients are unchanged up to the summation order of the blend; D shrinks by 9-19 %.  OFF by default: measured
 * neutral (K3 pays per Gaussian what the D-sized passes and the composite kernels save per pair).  mode: -1 the
 * environment's GSR_TILE_CULL (0 | 1 | auto, default 0), 0 off, 1 on, 2 auto = on for frames of more than
 * GSR_TILE_CULL_TILES (default 16384) tiles -- a static rule: the lists do not depend on earlier views. */
int gsr_set_tile_cull(int mode);
/* Diagnostics of the persistent launches on the current device: out4 = { sequence number of the last launch that passed
 * its last barrier, code of the last barrier fault (0x100 + n: barrier n of the prepare kernel, 0x200 + n: of the sort
 * kernel; 0 = none), number of faults (each is reported once as GSR_EFAULT by the next binning call), number of views
 * the sort kernel finished with one workgroup after its first barrier timed out }.  ABI 12: four words (ABI 11: three). */
int gsr_bin_persist_status(uint32_t *out4);
/* Diagnostics (GSR_BIN_TIMELINE=1 in the environment): the per-workgroup phase stamps (100 MHz clock, 32 per workgroup)
 * of the last persistent prepare (which = 0) / sort (which = 1) launch; *grid = its workgroups.  Synchronises. */
int gsr_bin_timeline(int which, unsigned long long *out, int max_words, int *grid);
/* Byte offset, inside the prep workspace of gsr_bin_prepare*, of the uint32 pair count D that K4 leaves on the DEVICE
 * (what gsr_bin_sort_bounded's kernels read).  For callers that capture the iteration in a hipGraph and therefore
 * cannot take D through gsr_bin_count_wait inside a replay: they copy the word out / test it with
 * gsr_flag_if_greater.  Stands where the reference reads `num_rendered` back (its rasterizer's forward). */
size_t gsr_bin_total_offset(int P, int width, int height);
/* The same for the uint32 count of ROW SEGMENTS R = sum of the rects' heights (ABI 12; the R-sized steps of
 * csrc/binning_rows.h work on it; 0 on frames above 256 x 256 tiles).  A measurement aid: bench.py reads it in its
 * instrumented replay to state the bytes the row-major pipeline moves (68 P + 28 R + 4 D). */
size_t gsr_bin_segments_offset(int P, int width, int height);

/* Capacity checks of a captured (hipGraph) training iteration -- the reference sizes everything from counts it reads
 * back (num_rendered; the exchange's i2j sizes, gaussian_renderer/__init__.py:572-585), a replayed graph cannot.
 * Buffers are sized from earlier iterations instead and these launches raise bits of ONE device word when a capacity
 * does not hold; gsr_preprocess_backward_adam_raw_batched_dyn skips its update when the word is non-zero and the host,
 * which reads the word after the replay, repeats the iteration eagerly.
 *   gsr_flag_if_greater : *flag_dev |= bit  when  *value_dev > limit  (e.g. the pair count against the sort capacity)
 *   gsr_exchange_check  : all_counts_dev / caps_dev int32 [W][W][B] (rows rank i sends rank j of camera k, and the
 *                         slab reserved for them): bit_over when a count exceeds its slab; bit_few when a band this
 *                         rank (`me`) renders -- bit k of rendered_mask -- receives fewer than `few` rows in total
 *                         (the reference's < 10-Gaussian stand-in rule, gaussian_renderer/__init__.py:1260-1269).
 *   Both also leave what they looked at in PINNED, device-accessible host memory when host_copy_pinned is not NULL
 *   (the value / the W*W*B counts, system-scope stores): the host reads them after the replay, no copy node needed.
 *   gsr_publish_flag    : last launch of a captured iteration: { *flag_dev, *seq_dev } are stored (system scope, the
 *                         stamp last) into words 2 s, 2 s + 1 of a pinned, device-accessible ring of `slots` pairs,
 *                         s = *seq_dev % slots; seq_dev is a device word the host refreshes in front of every replay.
 *                         The host polls the stamp instead of synchronising the stream. */
/* A device timestamp inside a captured iteration (ABI 13): word `index` (< per_slot) of slot *seq_dev % slots of a pinned,
 * device-accessible ring of uint64 receives the 100 MHz s_memrealtime counter when the launch runs (seq_dev NULL: slot 0).
 * Two stamps around a group of launches are what the HIP event pair of the eager loop measures (events recorded inside a
 * capture cannot be read): the load balancer's render / loss times (workload_division.py:953-966 of the reference) under
 * graph replay.  Valid for the host once gsr_publish_flag's stamp of the same replay has landed. */
int gsr_stamp(const uint32_t *seq_dev, uint64_t *host_ring_pinned, uint32_t slots, uint32_t per_slot, uint32_t index,
              gsr_stream_t stream);
/* compute_locally of B row bands from DEVICE data (ABI 13): mask uint8 [B][grid_y][grid_x], mask[k][ty][.] = lo_k <= ty <
 * hi_k with { lo_k, hi_k } = the first two words of record k of band_rows_dev (records of stride_words int32).  What
 * DivisionStrategyFinal.get_compute_locally (workload_division.py:773-787 of the reference) builds on the host per
 * partition, as a launch a hipGraph can replay for any partition. */
int gsr_band_mask(int grid_x, int grid_y, int B, const int32_t *band_rows_dev, int stride_words, uint8_t *mask,
                  gsr_stream_t stream);
int gsr_publish_flag(const uint32_t *flag_dev, const uint32_t *seq_dev, uint32_t *host_ring_pinned, uint32_t slots,
                     gsr_stream_t stream);
int gsr_flag_if_greater(const uint32_t *value_dev, uint32_t limit, uint32_t *flag_dev, uint32_t bit,
                        uint32_t *host_copy_pinned, gsr_stream_t stream);
int gsr_exchange_check(const int32_t *all_counts_dev, const int32_t *caps_dev, int W, int B, int me,
                       uint64_t rendered_mask, int few, uint32_t *flag_dev, uint32_t bit_over, uint32_t bit_few,
                       int32_t *host_copy_pinned, gsr_stream_t stream);
int gsr_bin_sort_bounded(int P, int width, int height, const uint8_t *compute_locally, const void *prep,
                         int64_t capacity, void *scratch, size_t scratch_bytes, uint32_t *point_list, int32_t *ranges,
                         gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K8  composite forward -- the rest of render_gaussians (gaussian_renderer/__init__.py:1271-1282).
 * out_color [3,H,W]: sum c*alpha*T + T_final*bg on locally computed tiles, exactly 0 elsewhere
 * (images are assembled by SUM all-reduce, train_internal.py:466-469); final_T [H,W];
 * n_contrib int32 [H,W] (1-based position of the last blended entry of the tile's list).
 *
 * K10 composite backward -- autograd backward of render_gaussians.
 * out (fully overwritten): dL_record [P,9], one row per Gaussian =
 *   [0:2] dL_dmeans2D (pixel gradient x (W/2, H/2)), [2:5] dL_drgb, [5:9] dL_dconic_opacity
 * -- the column order of the exchange's differentiable record (means2D, rgb, conic_opacity:
 * gaussian_renderer/__init__.py:647-650), so that at world size > 1 the record IS the message of the mirror
 * all-to-all.  One record instead of three arrays lets the kernel flush the 9 sums of a (tile, Gaussian) pair
 * from 9 adjacent lanes into one row: ~8x fewer memory-side atomic requests.
 * acc64 (required): [P,9] doubles, device scratch of the caller.  K10 adds its per-tile contributions into it in fp64
 * and each sum is rounded once into the record.  fp64 adds still depend on their order, but the fp32 result of a sum of
 * fp32 terms then differs only in the rare case that the fp64 sum lies within fp64 rounding of an fp32 rounding boundary:
 * on one GPU the record is reproducible from run to run in practice, where fp32 adds would make it depend on the order the
 * tiles finish.  (At N > 1 the exchange's gradient scatter still adds in fp32.)
 *
 * Optional arguments; each feature is off when its argument is absent.
 *
 * seg_ws, seg_bytes -- list SEGMENTS.  One workgroup per tile walks the tile's list serially, so a launch lasts at least
 *   as long as its longest list takes one wave -- which is the whole kernel on a thin row band (one round of resident
 *   workgroups at world size 8).  The backward can be cut exactly: per pixel it needs the transmittance and the colour
 *   accumulated IN FRONT of a list position, which the forward knows when it passes that position.  With a workspace of
 *   gsr_render_seg_bytes(width, height) bytes (caller-allocated, alive and untouched until the backward has run) the
 *   forward leaves a checkpoint every 256 list entries it really walks -- per pixel T, the colour blended since the
 *   previous checkpoint and, filled in when the walk ends, the colour blended behind this one: 7 KiB per tile and
 *   boundary -- and queues the segment that starts there; the backward, given the same workspace, runs segment 0 of every tile in its usual workgroups and hands
 *   the queued segments to persistent worker workgroups.  The colour BEHIND a boundary is the forward's own sum over the
 *   entries behind it (the checkpoints carry per-segment colour sums; the image minus the colour in front of the
 *   boundary would carry the image's rounding divided by the boundary's T).  out_color = the forward's image is still
 *   required with a workspace, for callers of earlier versions; the kernel no longer reads it.  Early termination is
 *   untouched (segments exist only for entries the forward walked); gradients equal the one-segment kernel's up to fp32
 *   rounding (the checkpointed T replaces a chain of divisions).  A second backward over one forward walks the same
 *   segments again.
 *   seg_ws == NULL: no segments; seg_bytes is ignored and out_color may be NULL in the backward.
 *   A workspace that is too small: GSR_ENOSPACE (forward), GSR_EINVAL (backward; also for out_color == NULL).
 *
 * row_lo, row_hi -- the TILE ROWS [row_lo, row_hi) of the caller's band when it knows them on the host (Grendel's
 *   strategies do: compute_locally must then be false outside these rows).  The launches then cover the band's tiles
 *   only; a grid over all tiles costs a constant ~30 us (forward) / ~60 us (backward) of workgroup dispatch for tiles
 *   that are not ours, whatever the band.  The forward still leaves every pixel outside the band exactly 0.
 *   row_lo = row_hi = 0 (or any pair that is not a proper sub-range of the grid's rows): the whole grid.
 *   row_lo == -1: the band is DEVICE data -- row_hi (1 .. grid rows) is only the CAPACITY of the launch in tile rows,
 *   the band itself is the row hull of compute_locally that the tile sort left behind the range table (row `tiles` of
 *   `ranges`, written by gsr_bin_sort / _bounded / gsr_bin_speculative_async on the device).  A band of more rows than
 *   row_hi is the caller's error: its last rows are not drawn.  One launch captured in a hipGraph then serves every band
 *   of at most row_hi rows (graphed_step.py: one graph for all cameras of a live partition, workload_division.py:806-849
 *   of the reference moves the cut points per camera); workgroups above the band's tile count only help clearing the
 *   pixels outside.
 *
 * zero_ptr, zero_bytes (forward) / record_is_zero, touched (backward) -- the backward's clears moved into the forward.
 *   K10 adds into acc64 with atomics, so the sums start at zero.  record_is_zero == 0: the backward clears acc64 itself
 *   with a fill at its head (72 MB per 10^6 Gaussians) and rounds every row into the record.  Instead the forward can
 *   clear [zero_ptr, zero_ptr + zero_bytes) -- 16-byte aligned, a multiple of 4 bytes, else GSR_EINVAL -- from the
 *   composite kernel's own workgroups (the kernel is bound by VALU issue, its memory pipes are idle); zero_bytes == 0:
 *   nothing is cleared.  The caller passes acc64 there (72 P bytes) and record_is_zero = 1 to the backward, which then
 *   skips its fill.  Nothing else may write the cleared buffers in between.
 *   touched: [P] bytes.  K10 sets touched[row] = 1 wherever it adds into a row of acc64, and only those rows are rounded
 *   into the record (K10 reaches about a tenth of the rows of a 10^6-Gaussian scene; the full pass reads 72 and writes
 *   36 bytes for every row).  For that the FORWARD must have cleared the sums, the record and the flags: the caller lays
 *   them out as one buffer, [72 P | 36 P | P, padded to 16] bytes = acc64, record, touched, and passes all of it as
 *   (zero_ptr, zero_bytes); record_is_zero = 1 says so.  The record is then complete when the call returns, bit for bit
 *   what the full pass writes.  touched == NULL or record_is_zero == 0: the full rounding pass.
 *
 * gsr_render_backward with P == 0 returns 0 and touches nothing. */
size_t gsr_render_seg_bytes(int width, int height);
int gsr_render_forward(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                       const float *means2D, const float *conic_opacity, const float *rgb,
                       const uint8_t *compute_locally, const float *bg, float *out_color, float *final_T,
                       int32_t *n_contrib, void *seg_ws, size_t seg_bytes, int row_lo, int row_hi, void *zero_ptr,
                       size_t zero_bytes, gsr_stream_t stream);
int gsr_render_backward(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                        const float *means2D, const float *conic_opacity, const float *rgb,
                        const uint8_t *compute_locally, const float *bg, const float *final_T,
                        const int32_t *n_contrib, const float *dL_dpixels, float *dL_record, const float *out_color,
                        void *seg_ws, size_t seg_bytes, int row_lo, int row_hi, int record_is_zero, double *acc64,
                        uint8_t *touched, gsr_stream_t stream);
/* Deferred rounding.  gsr_render_backward_sums is gsr_render_backward without its last launch: K10 adds into acc64 and
 * sets touched[], nothing is rounded and no record is written.  Both must have been cleared by the forward (zero_ptr);
 * the caller may then leave the record's 36 P bytes out of the cleared range (diff_gaussian_rasterization does not: it
 * measured nothing, and a record that was cleared reads as zeros until it is rounded).  The sums and flags are what gsr_preprocess_backward_adam_raw_batched_sums (below) reads in place of a record.
 * gsr_render_record_materialize runs the rounding left out, on any stream ordered behind that backward: the record is
 * then bit for bit what gsr_render_backward would have written (record_is_zero == 0: the record was not cleared, the
 * rows without a flag are written too), so deferring is never a one-way door.
 * gsr_set_deferred_rounding(mode): the process-wide switch a caller that owns the record consults before it defers
 * (gsr_deferred_rounding() -> 0 | 1); -1 = the environment's GSR_DEFER_ROUNDING (0 | 1, default 1), 0 off, 1 on.  The
 * library itself never defers: the two entry points above do what they say whatever the switch. */
int gsr_render_backward_sums(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                             const float *means2D, const float *conic_opacity, const float *rgb,
                             const uint8_t *compute_locally, const float *bg, const float *final_T,
                             const int32_t *n_contrib, const float *dL_dpixels, const float *out_color, void *seg_ws,
                             size_t seg_bytes, int row_lo, int row_hi, double *acc64, uint8_t *touched,
                             gsr_stream_t stream);
int gsr_render_record_materialize(int P, const double *acc64, const uint8_t *touched, float *dL_record,
                                  int record_is_zero, gsr_stream_t stream);
int gsr_set_deferred_rounding(int mode);
int gsr_deferred_rounding(void);
/* Measurement aid (bench.py's roofline leg; the reference has nothing to bind here): list entries the composite kernels
 * WALKED since the last reset, summed over launches -- out2[0] K8, out2[1] K10; per tile the entries its longest-walking
 * quadrant goes through (K8: up to the chunk in which the last pixel saturates; K10: the largest n_contrib of the
 * tile).  Early termination leaves most of every list untouched, so D-based byte formulas over-credit these kernels.
 * Synchronous (a device-to-host copy of two words); reset != 0 zeroes the counters afterwards. */
int gsr_composite_walked(unsigned long long *out2, int reset);

/* Per-Gaussian CONTRIBUTION statistics of a rendered view (the reference has no counterpart: its only per-Gaussian
 * signals are radii > 0, the screen-space gradient norm and the opacity, none of which says whether a Gaussian was ever
 * blended into a pixel).  A forward-only walk over the lists gsr_render_forward drew from, with that call's n_contrib:
 * the entry at list position k (0-based) of a local tile is BLENDED on a pixel iff k + 1 <= n_contrib[pixel],
 * power <= 0 and alpha = min(0.99, o exp(power)) >= 1/255 -- gsr_render_backward's rule, in the composite kernels' own
 * arithmetic, so the statistics describe exactly the image that was drawn; the stop is the forward's, nothing is
 * re-decided.  Per pixel T starts at 1; a blended pair has the weight w = alpha T, then T <- T (1 - alpha).  Takes no
 * rgb, bg or final_T.  ranges, point_list, means2D, conic_opacity, compute_locally, row_lo / row_hi: as
 * gsr_render_forward (whole grid, host band, -1 = device hull behind the range table).
 * The three arrays are the CALLER's, zeroed by the caller, and are ACCUMULATED into, never overwritten -- several views
 * (or bands) add up in one record:
 *   hits int64 [P] += the number of pixels that blended the row;
 *   wmax fp32  [P]  = max(old, largest w over those pixels) -- an unsigned 32-bit atomic max on the bits (values are
 *                     non-negative), exact and independent of the order;
 *   wsum fp64  [P] += the sum of w over those pixels: per 8x8 quadrant in fp32 in a fixed order, then one fp64 atomic add
 *                     (at most 4 x local tiles additions per row and launch).
 * Rows that are blended nowhere in the launch receive no write.  P < 0, a non-positive frame, or a missing pointer with
 * P > 0: GSR_EINVAL before any device work; P == 0 returns 0 and touches nothing.
 * gsr_contrib_merge_rows: dst[idx[r]] gets hits += src_hits[r], wmax = max(., src_wmax[r]), wsum += src_wsum[r] for the
 * n rows of a record that came back from another rank -- the counterpart of gsr_scatter_add_rows for this record: rows
 * with idx[r] < 0 are skipped, duplicate indices are allowed (a Gaussian needed by two bands arrives twice; atomics).
 * n < 0 or a missing pointer with n > 0: GSR_EINVAL; n == 0 returns 0 and touches nothing. */
int gsr_render_contrib(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                       const float *means2D, const float *conic_opacity, const uint8_t *compute_locally,
                       const int32_t *n_contrib, int row_lo, int row_hi, int64_t *hits, float *wmax, double *wsum,
                       gsr_stream_t stream);
int gsr_contrib_merge_rows(int64_t n, const int32_t *idx, const int64_t *src_hits, const float *src_wmax,
                           const double *src_wsum, int64_t *dst_hits, float *dst_wmax, double *dst_wsum,
                           gsr_stream_t stream);

/* INVERSE-DEPTH map of a rendered view, with gradients (depth supervision).  The reference's rasterizer renders no depth
 * of any kind, so there is NO reference call site for these three entry points: the quantity is the inverse-depth output
 * of the official 3DGS rasterizer, and oracle/torch_oracle.py's `render` with rgb = (v, 0, 0), bg = 0 -- differentiated
 * by autograd in float64 -- is the arbiter.  New symbols only: gsr_abi_version does not move.
 * A walk over the lists gsr_render_forward drew from, with that call's n_contrib (and, backward, final_T): the entry at
 * list position k (0-based) of a local tile is BLENDED on a pixel iff k + 1 <= n_contrib[pixel], power <= 0 and
 * alpha = min(0.99, o exp(power)) >= 1/255 -- gsr_render_contrib's rule, in the composite kernels' own arithmetic;
 * nothing is re-decided.  Per pixel T starts at 1; a blended entry i has the weight w_i = alpha_i T_i, then T <- T - w_i.
 * v_i = 1.0f / depths[id_i], depths = K1's view-space z.  CALLER'S CONDITION: every listed row has depth > 0 (K1 lists
 * rows with radii > 0 only, whose depth exceeds 0.2); rows in no list may carry any depth, 0 included.
 * ranges, point_list, means2D, conic_opacity, compute_locally, row_lo / row_hi: as gsr_render_contrib (whole grid, host
 * band, -1 = device hull behind the range table).
 *
 * gsr_render_invdepth: invdepth fp32 [H,W], FULLY overwritten:
 *   invdepth[p] = sum over the blended entries of w_i v_i -- no background term, no division by 1 - T_final; pixels of
 *   tiles that are not ours (and of tiles outside the band of a band launch) are exactly 0: the map is assembled across
 *   bands by a SUM, as the image is.  P == 0 writes the all-zero map and touches nothing else.
 *
 * gsr_render_invdepth_backward: with g = dL_dinvdepth[p] ([H,W]; read on the local tiles only),
 *   dL/dv_i     = sum_p g w_i, hence dL/ddepth_i = -(sum_p g w_i) / depth_i^2;
 *   dL/dalpha_i = g (T_i v_i - S_i / (1 - alpha_i)), S_i = the sum of w_j v_j over the blended j behind i;
 *   from dL/dalpha on, gsr_render_backward's chain to opacity, conic (A, B, C) and means2D, including its treatment of
 *   the 0.99 clamp (the identity in the backward); means2D gradients in its units: pixel gradient x (W/2, H/2).
 *   dL_record fp32 [P,7], FULLY overwritten: [0:2] dL_dmeans2D, [2:6] dL_dconic_opacity, [6] dL_ddepth; rows that are
 *   blended nowhere are 0.0f.  acc64: [P,7] doubles, device scratch of the caller, cleared by the call: the per-quadrant
 *   sums (fp32, a fixed order over the 64 pixels) are added into it in fp64 and each sum is rounded once into the record
 *   (gsr_render_backward's reason: the fp32 result does not depend on the order the tiles finish, but for the rare sum
 *   within fp64 rounding of an fp32 rounding boundary).  final_T and invdepth are the forward calls' outputs; the walk
 *   goes back to front from final_T, and `invdepth` is not read by this implementation (a front-to-back walk would take
 *   S_i from it).  P == 0 returns 0 and touches nothing.
 *
 * gsr_depth_backward_means3d: depth = ([p,1] viewmatrix)[2] in the row-vector convention (viewmatrix: 16 floats on the
 *   device, row-major), so dL_dmeans3D[i] (+)= dL_ddepth[i * row_stride] * (view[0][2], view[1][2], view[2][2]);
 *   row_stride in floats (1 dense, 7 = column 6 of the record above).  Rows with radii <= 0 are skipped.  overwrite == 0:
 *   += into the caller's (zeroed) [P,3]; overwrite != 0: every row is written, skipped rows as zeros.
 *
 * All three: a negative size, a non-positive frame (row_stride < 1), or a missing pointer with P > 0: GSR_EINVAL before
 * any device work (the forward needs `invdepth` for P == 0 too). */
int gsr_render_invdepth(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                        const float *means2D, const float *conic_opacity, const float *depths,
                        const uint8_t *compute_locally, const int32_t *n_contrib, int row_lo, int row_hi,
                        float *invdepth, gsr_stream_t stream);
int gsr_render_invdepth_backward(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                                 const float *means2D, const float *conic_opacity, const float *depths,
                                 const uint8_t *compute_locally, const int32_t *n_contrib, const float *final_T,
                                 const float *invdepth, const float *dL_dinvdepth, int row_lo, int row_hi,
                                 float *dL_record, double *acc64, gsr_stream_t stream);
int gsr_depth_backward_means3d(int P, const int32_t *radii, const float *viewmatrix, const float *dL_ddepth,
                               int row_stride, float *dL_dmeans3D, int overwrite, gsr_stream_t stream);

/* N-CHANNEL FEATURE MAP of a rendered view, with gradients (semantic logits, distilled 2D features, normals, an
 * accumulated-opacity map, expected depth, ...).  The reference's rasterizer blends three colour channels only, so there is
 * NO reference call site: oracle/torch_oracle.py's `render` with bg = 0, three channels at a time, differentiated by
 * autograd in float64, is the arbiter (tests/features_refs.py).  New symbols only: gsr_abi_version does not move.
 * Inputs as gsr_render_invdepth, with `features` fp32 [P, C] row-major in place of `depths` and 1 <= C <=
 * GSR_FEATURES_MAX; the inverse-depth map is the case C = 1, f = 1 / depth.  The same walk: the entry at list position k
 * (0-based) of a local tile is BLENDED on a pixel p iff k + 1 <= n_contrib[p], power <= 0 and alpha_i = min(0.99, o_i
 * exp(power)) >= 1/255, in the composite kernels' own arithmetic; nothing is re-decided.  T starts at 1, w_i = alpha_i T_i,
 * T <- T - w_i.
 *
 * gsr_render_features: out fp32 [C,H,W], FULLY overwritten:
 *   out[c][p] = sum over the blended entries of w_i f_i[c] -- no background term, no division by 1 - T_final; pixels of
 *   tiles that are not ours (and of tiles outside the band of a band launch) are exactly +0.  A channel's values do not
 *   depend on C or on the other channels.  P == 0 writes the all-zero map and touches nothing else.
 *
 * gsr_render_features_backward: with g_c = dL_dout[c][p] ([C,H,W]; read on the local tiles only),
 *   dL/df_i[c]  = sum_p g_c w_i;
 *   dL/dalpha_i = sum_c g_c (T_i f_i[c] - S_i[c] / (1 - alpha_i)), S_i[c] = the sum of w_j f_j[c] over the blended j behind i;
 *   from dL/dalpha on, gsr_render_backward's chain: q = o G dL/dalpha (the 0.99 clamp is the identity in the backward),
 *   (dx, dy) = mean - pixel, dL/dmean = -(A sum q dx + B sum q dy, B sum q dx + C sum q dy) (W/2, H/2),
 *   dL/d(A, B, C) = -(sum q dx^2 / 2, sum q dx dy, sum q dy^2 / 2), dL/do = sum q / o.
 *   dL_record fp32 [P,6], FULLY overwritten: [0:2] dL_dmeans2D, [2:6] dL_dconic_opacity.  dL_dfeatures fp32 [P,C], FULLY
 *   overwritten -- or NULL: the feature gradient is not formed (a constant feature, such as an all-ones column whose map
 *   is the accumulated opacity 1 - T_final), dL_record is the same bits.  Rows blended nowhere are +0.0f in both.
 *   acc64: device scratch of the caller, cleared by the call: [P, 6 + C] doubles, or [P, 6] with dL_dfeatures == NULL;
 *   per-quadrant fp32 sums (a fixed order over the 64 pixels) are added into it in fp64 and each sum is rounded once
 *   (gsr_render_backward's reason).  The channels are processed GSR_FEATURES_CHUNK at a time; every chunk walks the lists
 *   again from final_T and recomputes alpha (nothing per (pixel, entry) is kept in device memory), and the chunks'
 *   geometry sums add in fp64.  P == 0 returns 0 and touches nothing.
 *
 * row_lo / row_hi: whole grid (0, 0), host band, or -1 = the device hull behind the range table, as gsr_render_invdepth.
 * Both: a negative size, a non-positive frame, C outside [1, GSR_FEATURES_MAX], or a missing pointer with P > 0:
 * GSR_EINVAL before any device work (the forward needs `out` for P == 0 too). */
#define GSR_FEATURES_MAX 256
#define GSR_FEATURES_CHUNK 16
int gsr_render_features(int P, int C, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                        const float *means2D, const float *conic_opacity, const float *features,
                        const uint8_t *compute_locally, const int32_t *n_contrib, int row_lo, int row_hi, float *out,
                        gsr_stream_t stream);
int gsr_render_features_backward(int P, int C, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                                 const float *means2D, const float *conic_opacity, const float *features,
                                 const uint8_t *compute_locally, const int32_t *n_contrib, const float *final_T,
                                 const float *dL_dout, int row_lo, int row_hi, float *dL_record, float *dL_dfeatures,
                                 double *acc64, gsr_stream_t stream);

/* ABSOLUTE screen-space gradient of a rendered view (densification).  The reference accumulates the norm of the signed
 * means2D gradient, which cancels on a large Gaussian whose pixels pull its centre in opposite directions; this is the
 * homodirectional gradient of AbsGS (`absgrad` of gsplat): the magnitude of every pixel's contribution, summed.  There is
 * NO reference call site.  The float64 closed form of tests/absgrad_refs.py is the arbiter; its signed sums are, up to the
 * sign, columns 0:2 of gsr_render_backward's record.  New symbols only: gsr_abi_version does not move.
 * A walk over the lists gsr_render_forward drew from, with that call's final_T and n_contrib and the dL_dpixels
 * gsr_render_backward is given: the entry at list position k (0-based) of a local tile is BLENDED on a pixel p iff
 * k + 1 <= n_contrib[p], power <= 0 and alpha_i = min(0.99, o_i exp(power)) >= 1/255 -- gsr_render_backward's rule, in the
 * composite kernels' own arithmetic; nothing is re-decided.  With g_c = dL_dpixels[c][p], T_i the transmittance in front
 * of i, w_j = alpha_j T_j and G_i = exp(power),
 *   dL/dalpha_i(p) = sum_c g_c (T_i c_i,c - S_i,c / (1 - alpha_i)) - (T_final / (1 - alpha_i)) sum_c bg_c g_c,
 *   S_i,c          = the sum of w_j c_j,c over the blended j behind i,
 *   q_i(p)         = o_i G_i dL/dalpha_i(p)      (the 0.99 clamp is the identity in the backward, as in gsr_render_backward),
 *   (dx, dy)       = mean_i - pixel,
 *   absgrad[i]     = ( (W/2) sum_p | q_i(p) (A dx + B dy) | ,  (H/2) sum_p | q_i(p) (B dx + C dy) | ),
 * the sums over the pixels of all local tiles (of the band, for a band launch) that blend i.  Without the absolute values
 * the two sums are -dL_dmeans2D of gsr_render_backward; the units are the same: pixel gradient x (W/2, H/2).  Only the
 * colour loss's dL_dpixels enters (a loss on the inverse-depth map does not).
 * ranges, point_list, means2D, conic_opacity, rgb, compute_locally, bg, row_lo / row_hi: as gsr_render_forward (whole
 * grid, host band, -1 = device hull behind the range table).  The segment workspace is not used: the walk goes back to
 * front over the whole list from final_T.
 *   absgrad fp32 [P,2], FULLY overwritten; rows that are blended nowhere are exactly 0.0f.
 *   acc64: [P,2] doubles, device scratch of the caller, cleared by the call: the per-quadrant sums (fp32, a fixed order
 *   over the 64 pixels) are added into it in fp64 and each sum is rounded once into `absgrad` (gsr_render_backward's reason:
 *   the fp32 result does not depend on the order the tiles finish, but for the rare sum within fp64 rounding of an fp32
 *   rounding boundary).
 * gsr_absgrad_merge_rows: dst[idx[r]][0:2] += src[r][0:2] for the n rows that came back from another rank -- the two-column
 * counterpart of gsr_scatter_add_rows: rows with idx[r] < 0 are skipped, duplicate indices add (atomics).
 * P < 0 (n < 0), a non-positive frame, or a missing pointer with P > 0 (n > 0; point_list may be NULL: every list can be
 * empty): GSR_EINVAL before any device work; P == 0 (n == 0) returns 0 and touches nothing. */
int gsr_render_absgrad(int P, int width, int height, const int32_t *ranges, const uint32_t *point_list,
                       const float *means2D, const float *conic_opacity, const float *rgb,
                       const uint8_t *compute_locally, const float *bg, const float *final_T, const int32_t *n_contrib,
                       const float *dL_dpixels, int row_lo, int row_hi, float *absgrad, double *acc64,
                       gsr_stream_t stream);
int gsr_absgrad_merge_rows(int64_t n, const int32_t *idx, const float *src, float *dst, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N1  fused band-local L1 + SSIM loss -- the arithmetic of final_system_loss_computation,
 * gaussian_renderer/loss_distribution.py:2536-2585 (pixelwise_l1_with_mask / pixelwise_ssim_with_mask,
 * utils/loss_utils.py:88-132): 11x11 Gaussian window (sigma 1.5), zero padding at the band edges,
 * C1 = 0.01^2, C2 = 0.03^2, ground truth = uint8 / 255.
 * `image` points at the band's first row of channel 0 inside a [C, H, W] image (row stride = width,
 * channel stride = image_channel_stride elements); gt is the dense uint8 band [C, rows, width].
 * forward : partials [gsr_l1_ssim_num_partials()][2] = per-workgroup (sum |x-y|, sum ssim_map); the
 *           caller adds them up.  dm_* [C, rows, width] receive the derivative maps the backward
 *           needs (all three NULL for a forward-only evaluation).
 * backward: grad_image (same addressing as `image`, channel stride grad_channel_stride) =
 *           scale_l1 * *grad_l1_sum * sign(x - y) + scale_ssim * *grad_ssim_sum * d(sum ssim)/dx ; the two device
 *           scalars are read on the device (no host sync) -- a caller whose loss is c_l1 * S_l1 + c_ssim * S_ssim passes
 *           the incoming dL/dloss for both pointers and (c_l1, c_ssim) as the scales: no glue kernel. */
int gsr_l1_ssim_num_partials(int channels, int rows, int width);
int gsr_l1_ssim_forward(int channels, int rows, int width, const float *image, int64_t image_channel_stride,
                        const uint8_t *gt, float *partials, float *dm_dmu1, float *dm_dE11, float *dm_dE12,
                        gsr_stream_t stream);
int gsr_l1_ssim_backward(int channels, int rows, int width, const float *image, int64_t image_channel_stride,
                         const uint8_t *gt, const float *dm_dmu1, const float *dm_dE11, const float *dm_dE12,
                         const float *grad_l1_sum, const float *grad_ssim_sum, float scale_l1, float scale_ssim,
                         float *grad_image, int64_t grad_channel_stride, gsr_stream_t stream);
/* The same pair for a band whose rows are DEVICE data (ABI 13; one captured launch for every band of a camera):
 * band_rows = { y0, y1 } int32 pixel rows of `image` (NOT offset: the full image's base pointer) on the device;
 * rows_capacity >= y1 - y0 sizes the launch, the partials (gsr_l1_ssim_num_partials(C, rows_capacity, width): the slots
 * above the band's own count receive zeros) and the CHANNEL STRIDE of gt and dm_* ([C, rows_capacity, width], the band
 * in the first y1 - y0 rows of every channel).  Tile ids and the order of the partial sums are those of a launch sized
 * for the band: the finalized loss is bit-equal to gsr_l1_ssim_forward's on the same rows. */
int gsr_l1_ssim_forward_band(int channels, int rows_capacity, int width, const float *image, int64_t image_channel_stride,
                             const uint8_t *gt, float *partials, float *dm_dmu1, float *dm_dE11, float *dm_dE12,
                             const int32_t *band_rows, gsr_stream_t stream);
int gsr_l1_ssim_backward_band(int channels, int rows_capacity, int width, const float *image,
                              int64_t image_channel_stride, const uint8_t *gt, const float *dm_dmu1, const float *dm_dE11,
                              const float *dm_dE12, const float *grad_l1_sum, const float *grad_ssim_sum, float scale_l1,
                              float scale_ssim, float *grad_image, int64_t grad_channel_stride, const int32_t *band_rows,
                              gsr_stream_t stream);
/* finalize: adds the partials up (fixed order, fp64 accumulation) and forms the band's loss terms in one
 * launch: out3[0] = c_l1 * S_l1 + c_ssim * S_ssim + bias  (batched_loss_computation's
 * (1 - lambda) * Ll1 + lambda * (1 - ssim) with c_l1 = (1-lambda)/n, c_ssim = -lambda/n, bias = lambda;
 * gaussian_renderer/loss_distribution.py:2627-2629), out3[1] = S_l1 * inv_n, out3[2] = S_ssim * inv_n. */
int gsr_l1_ssim_finalize(int num_partials, const float *partials, float c_l1, float c_ssim, float bias, float inv_n,
                         float *out3, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N1x  per-camera exposure compensation fused into N1.  `exposure` E = [A | b]: 12 floats on the device, row-major
 * [3,4], read by the kernels (a captured launch serves changing values).  For every pixel INSIDE the band
 *   x'[c] = A[c][0] x[0] + A[c][1] x[1] + A[c][2] x[2] + b[c]     (no clamp)
 * and the loss is N1's band-local loss of x' against the ground truth: same window, constants, y = u8 * (1/255f), sums
 * and derivative maps.  The zero padding of the SSIM window is a padding of x': outside the band's rows and the image's
 * columns x' is exactly 0 -- not b, and not a transform of what lies in memory there.  Gradients, with
 * g'[c] = dL/dx'[c] (what gsr_l1_ssim_backward writes for its input):
 *   dL/dx[k] = sum_c A[c][k] g'[c],   dL/dA[c][k] = sum_pixels g'[c] x[k],   dL/db[c] = sum_pixels g'[c].
 * There is no reference call site (the reference has no exposure model); the arbiter is the fp64 torch restatement of
 * the lines above (tests/test_gpu_exposure_loss.py).  channels must be 3.
 *
 * gsr_l1_ssim_forward_exposure: the arguments of gsr_l1_ssim_forward_band plus `exposure`.  band_rows == NULL selects
 * the static form: `image` then points at the band's first row and rows_capacity is the row count.  Partials: layout
 * and count of the plain launch of the same shape (gsr_l1_ssim_num_partials; gsr_l1_ssim_finalize adds them up).  With
 * an identity E every output is bit-equal to the plain launch's.  No reference call site; arbiter as above.
 * GSR_EINVAL before any device work: channels != 3, a null exposure / image / gt / partials, one or two null maps. */
int gsr_l1_ssim_forward_exposure(int channels, int rows_capacity, int width, const float *image,
                                 int64_t image_channel_stride, const uint8_t *gt, float *partials, float *dm_dmu1,
                                 float *dm_dE11, float *dm_dE12, const int32_t *band_rows, const float *exposure,
                                 gsr_stream_t stream);
/* The number of 12-float rows gsr_l1_ssim_backward_exposure writes to exposure_partials: one per 32x32 tile of the
 * band (of the capacity, for a device band).  Pure host arithmetic; exists for the exposure model only (no reference
 * call site). */
int gsr_l1_ssim_exposure_num_partials(int rows, int width);
/* gsr_l1_ssim_backward_exposure: the arguments of gsr_l1_ssim_backward_band (band_rows optional as in the forward) plus
 * `exposure`, exposure_partials [gsr_l1_ssim_exposure_num_partials(rows_capacity, width)][12] (scratch, fully written:
 * per tile the sums dL/dA[c][k] at [4c + k], dL/db[c] at [4c + 3]; the rows above a device band's own tile count
 * receive zeros) and grad_exposure (12 floats, row-major [3,4], fully overwritten).  One workgroup per tile recomputes
 * x' at its pixels, walks the three channels for g', writes grad_image = A^T g' (the band's rows of all three
 * channels) and publishes its 12 sums; a second launch adds the rows in a fixed order in fp64 and rounds each sum
 * once: no atomics, bit-identical from run to run.  The definition is the one at the head of this section; no reference
 * call site, the arbiter is the fp64 torch restatement.  GSR_EINVAL before any device work: channels != 3, a null
 * exposure / exposure_partials / grad_exposure or any null pointer gsr_l1_ssim_backward refuses. */
int gsr_l1_ssim_backward_exposure(int channels, int rows_capacity, int width, const float *image,
                                  int64_t image_channel_stride, const uint8_t *gt, const float *dm_dmu1,
                                  const float *dm_dE11, const float *dm_dE12, const float *grad_l1_sum,
                                  const float *grad_ssim_sum, float scale_l1, float scale_ssim, float *grad_image,
                                  int64_t grad_channel_stride, const int32_t *band_rows, const float *exposure,
                                  float *exposure_partials, float *grad_exposure, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N1m  per-pixel loss masks fused into N1 / N1x (new symbols of ABI 15; nothing above changes).  `mask`: one uint8 per
 * pixel, shared by the channels, laid out like ONE channel of the ground-truth band: [rows, width] in the static form,
 * [rows_capacity, width] with the band in its first rows in the device-band form.  m = byte * (1/255f) in fp32: exactly 1
 * for byte 255, exactly 0 for byte 0, within 1.5 ulp of byte / 255 in between.  For every pixel INSIDE the band
 *   x' = m x          (with an exposure E = [A | b]:  x' = m (A x + b), A x + b formed as in N1x)
 *   y' = m (gt * (1/255f))
 * and outside the band x' = y' = 0 (the zero padding of N1).  Everything behind that is N1 on (x', y'): the L1 sum, the
 * SSIM map and the maps dm_* keep their form, n = H * W * 3 of the full image and gsr_l1_ssim_finalize are unchanged
 * (the loss is NOT renormalised by the mask's pixel count).  Both images are multiplied (gsplat's `masks`); the official
 * trainer's `image *= alpha_mask` is the same loss wherever the ground truth is already black under the mask.
 * Backward, with g' = dL/dx' (N1's formula evaluated at (x', y')):
 *   dL/dx = m g'        with an exposure:  dL/dx[k] = m sum_c A[c][k] g'[c],
 *                       dL/dA[c][k] = sum_pixels m g'[c] x[k],  dL/db[c] = sum_pixels m g'[c].
 * Two exact properties:
 *  1. An all-255 mask gives, bit for bit, the partial sums, the three maps, the image gradient and (with an exposure)
 *     the exposure gradient of the corresponding unmasked launch (gsr_l1_ssim_forward / _backward, their _band forms,
 *     the _exposure pair): m = 1 enters as single multiplications, and the masked backward rounds every product and
 *     sum of g' on its own, which is what the unmasked kernels' code does.
 *  2. Where m = 0 the gradient is exactly +0 and no output bit depends on the finite value of x there.
 * No reference call site (the reference has no loss mask); the arbiter is the fp64 torch restatement of the lines above
 * (tests/masked_loss_refs.py).
 *
 * gsr_l1_ssim_forward_masked: the arguments of gsr_l1_ssim_forward_exposure plus `mask` behind `gt`.  band_rows == NULL
 * selects the static form (`image` points at the band's first row, rows_capacity is the row count); exposure == NULL
 * means no exposure (any channel count).  The mask is fetched four bytes at a time when its base pointer is 4-byte
 * aligned and width % 4 == 0 (and the image / gt allow the vector path); otherwise the launch takes the scalar path --
 * the results are the same bits.  Partials: layout and count of the plain launch of the same shape.
 * gsr_l1_ssim_backward_masked: the arguments of gsr_l1_ssim_backward_exposure plus `mask` behind `gt`;
 * exposure_partials / grad_exposure are looked at only with an exposure.  grad_image: the band's rows, fully written.
 * GSR_EINVAL before any device work: a null mask, channels / rows_capacity / width <= 0, an exposure with channels != 3
 * (backward: or without exposure_partials / grad_exposure), or any null pointer the unmasked launch refuses. */
int gsr_l1_ssim_forward_masked(int channels, int rows_capacity, int width, const float *image,
                               int64_t image_channel_stride, const uint8_t *gt, const uint8_t *mask, float *partials,
                               float *dm_dmu1, float *dm_dE11, float *dm_dE12, const int32_t *band_rows,
                               const float *exposure, gsr_stream_t stream);
int gsr_l1_ssim_backward_masked(int channels, int rows_capacity, int width, const float *image,
                                int64_t image_channel_stride, const uint8_t *gt, const uint8_t *mask,
                                const float *dm_dmu1, const float *dm_dE11, const float *dm_dE12,
                                const float *grad_l1_sum, const float *grad_ssim_sum, float scale_l1, float scale_ssim,
                                float *grad_image, int64_t grad_channel_stride, const int32_t *band_rows,
                                const float *exposure, float *exposure_partials, float *grad_exposure,
                                gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N1e  fused evaluation metrics of one row band, forward only -- what training_report prints
 * (train_internal.py:471-478: clamp both, l1_loss(...).mean(), psnr(...).mean()), the per-channel PSNR of
 * utils/image_utils.py:19-21, and the SSIM / PSNR metrics.py:78-79 takes of the saved PNGs -- as SUMS over the rows
 * [y0, y1) of a full [C, height, width] fp32 image against the full uint8 ground truth (row stride = width, channel
 * strides in elements, >= height * width).  Per element x = clamp(image, 0, 1) -- with GSR_METRICS_QUANTIZE
 * x = q / 255, q = floor(clamp(x * 255 + 0.5, 0, 255)) formed exactly like mul(255).add_(0.5).clamp_(0, 255).to(uint8) --
 * and y = gt * (1/255f).  partials [gsr_image_metrics_num_partials(C, y1 - y0, width)][3] = per 32x32 tile
 * (sum |x-y|, sum (x-y)^2, sum ssim_map); the tiles of a channel are contiguous.  The SSIM window (N1's: 11x11,
 * sigma 1.5, C1 = 0.01^2, C2 = 0.03^2) reads rows [max(0, y0 - 5), min(height, y1 + 5)) of both buffers: zero padding at
 * the IMAGE's edges only, so the band sums of a partition add up to the full image's.  GSR_METRICS_NO_SSIM: no window,
 * no halo rows are read, the third sum is 0.  out_u8 (optional) [C, y1 - y0, width] receives the quantised band q
 * whether or not the sums use it.  GSR_EINVAL: a null image / gt / partials, y0 < 0, y0 >= y1, y1 > height, an
 * unknown flag bit, a channel stride below height * width.
 * finalize: sums [C][3] (double) = each channel's partials added in a fixed order in fp64 (bit-reproducible);
 * num_partials = the count of the launch that wrote them (a multiple of channels). */
#define GSR_METRICS_QUANTIZE 1
#define GSR_METRICS_NO_SSIM 2
int gsr_image_metrics_num_partials(int channels, int rows, int width);
int gsr_image_metrics(int channels, int height, int width, const float *image, int64_t image_channel_stride,
                      const uint8_t *gt, int64_t gt_channel_stride, int y0, int y1, int flags,
                      float *partials, uint8_t *out_u8, gsr_stream_t stream);
int gsr_image_metrics_finalize(int channels, int num_partials, const float *partials, double *sums, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N3  fused Adam step for one parameter tensor of n fp32 elements (16-byte aligned, dense):
 * the update stock torch.optim.Adam performs as configured at scene/gaussian_model.py:292
 * (no weight decay, no amsgrad), with the reference's `grad /= bsz` (train_internal.py:319-324)
 * folded in as grad_scale.  `step` is the 1-based step count AFTER this update (bias correction).
 * Hyper-parameters are doubles so that 1 - beta and the bias corrections round like the stock optimizer's. */
int gsr_adam_step(int64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, double lr,
                  double beta1, double beta2, double eps, int64_t step, float grad_scale, gsr_stream_t stream);

/* The same update for up to 16 parameter tensors in ONE launch (the reference's optimizer walks its six param
 * groups, scene/gaussian_model.py:244-292: xyz, f_dc, f_rest, opacity, scaling, rotation): arrays of length
 * num_tensors with each tensor's element count, pointers and its group's hyper-parameters / step count.
 * Tensors with 0 elements are skipped. */
int gsr_adam_step_multi(int num_tensors, const int64_t *numels, float *const *params, const float *const *grads,
                        float *const *exp_avgs, float *const *exp_avg_sqs, const double *lrs, const double *beta1s,
                        const double *beta2s, const double *epss, const int64_t *steps, float grad_scale,
                        gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2 for a whole camera batch, in the layout of the exchange (rows a5/a6).  The reference calls
 * get_local2j_ids_bool once per camera and then nonzero() per (camera, band) (workload_division.py:721-744,
 * gaussian_renderer/__init__.py:586-622).  With the camera-batched K1 the state is [B,P,.]:
 * means2D fp32 [B,P,2], radii int32 [B,P]; bands int32 [B][W][2] = tile rows [lo,hi) of camera k rendered by
 * GLOBAL rank g ((0,0): none); need uint8 [W][B][P] = 1 iff the Gaussian's 3-sigma tile rect (the K2 rule)
 * meets that band -- flattened, this is the (destination, camera, Gaussian) send order of the all-to-all-v;
 * counts int32 [W][B] = row sums of need (zeroed here).  W <= 256. */
int gsr_exchange_need(int P, int B, int W, int width, int height, const float *means2D, const int32_t *radii,
                      const int32_t *bands, uint8_t *need, int32_t *counts, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The exchange without the mask (rows a5/a6; what the mirror's _batched_exchange_final calls).  The reference's
 * all_to_all_communication_final (gaussian_renderer/__init__.py:542-698) runs K2, then nonzero() per (camera, band),
 * index_select + cat per destination; its autograd backward is an index_put with accumulate.  Here, for the cameras
 * [k0, k0 + B) of a batch of B_total whose state is camera-major ([B_total,P,.] arrays):
 *   gsr_exchange_count : counts int32 [W][B] (every entry written here) = number of Gaussians rank g needs of camera
 *       k0 + kk, and chunkcnt int32 [W * B][gsr_exchange_chunks(P)] = the same per 1024-Gaussian chunk (a workspace for
 *       pack; counts is its row sums, formed by a second launch -- no atomics);
 *   gsr_exchange_pack  : after the caller has turned the counts of all ranks into the layout of its send buffer --
 *       segment_offsets[g * B + kk] (HOST array, W * B <= 512 entries) = first row of the (destination g, camera
 *       k0 + kk) segment -- writes the 11-float records (means2D 2, rgb 3, conic_opacity 4, radius bits, depth) into
 *       msg fp32 [n_send][11] in (destination, camera, local index) order and send_idx int32 [n_send] = kk * P + i,
 *       the row each record came from; chunkcnt is what gsr_exchange_count wrote for the camera range
 *       [count_first, count_first + count_cameras) (which must contain [k0, k0 + B): one count launch for the batch,
 *       one pack launch per camera when the exchanges are pipelined);
 *   gsr_scatter_add_rows : dst[idx[r]][0:9] += src[r][0:9] -- the backward's mirror step on the gradient rows the
 *       peers send back (dst fp32 [rows][9], zeroed by the caller; a Gaussian needed by two bands is added twice);
 *       rows with idx[r] < 0 are skipped.
 * Tile-row limit: gsr_exchange_count, gsr_exchange_pack and gsr_exchange_pack_slab keep a Gaussian's tile-row interval
 * in 16 + 16 bits, so they return GSR_EINVAL for a frame of more than 65535 tile rows (height > 65535 * 16 = 1 048 560
 * pixels).  gsr_exchange_need keeps full ints and has no such limit. */
size_t gsr_exchange_chunks(int P);
int gsr_exchange_count(int P, int B_total, int k0, int B, int W, int width, int height, const float *means2D,
                       const int32_t *radii, const int32_t *bands, int32_t *chunkcnt, int32_t *counts,
                       gsr_stream_t stream);
int gsr_exchange_pack(int P, int B_total, int k0, int B, int W, int width, int height, int count_cameras,
                      int count_first, const float *means2D,
                      const float *rgb, const float *conic_opacity, const int32_t *radii, const float *depths,
                      const int32_t *bands, const int32_t *chunkcnt, const int32_t *segment_offsets, int64_t n_send,
                      float *msg, int32_t *send_idx, gsr_stream_t stream);
int gsr_scatter_add_rows(int64_t n, const int32_t *idx, const float *src, float *dst, gsr_stream_t stream);
/* The exchange WITHOUT the host read-back (round 3).  gsr_exchange_pack needs the segment layout, i.e. the counts of
 * this very step on the host: the reference's `.cpu()` of gaussian_renderer/__init__.py:572-585, one device round trip
 * per iteration in the middle of the forward.  gsr_exchange_pack_slab instead packs into CAPACITY slabs the caller
 * chose beforehand (from earlier iterations): capacities[g * B + kk] (HOST, W * B <= 512 entries, sum == n_rows) rows
 * are reserved for (destination g, camera k0 + kk), back to back; the records go to the front of their slab in the
 * same (local index) order, records past the capacity are dropped, and the unused tail of every slab is written as
 * all-zero records (radius 0: the receiving rank's binning culls them) with send_idx -1 (gsr_scatter_add_rows skips
 * negative rows).  `counts` is the DEVICE array gsr_exchange_count wrote (same launch as chunkcnt).  The caller sends
 * whole slabs (all-to-all-v with the capacities as split sizes), learns the true counts later (an asynchronous copy
 * that has long completed when it polls the pair count of the first render) and repeats the exchange with
 * gsr_exchange_pack when any count exceeded its capacity -- the same speculate / verify scheme as
 * gsr_bin_sort_bounded.  Received rows keep the reference's order (source rank, then the source's index); padding
 * rows sit between the sources' blocks. */
/* gsr_exchange_unpack: the received message recv fp32 [n][11] (any mix of records and padding rows) -> the five dense
 * tensors of the render op: means2D [n,2], rgb [n,3], conic_opacity [n,4], radii int32 [n] (the record's radius BITS),
 * depths [n].  gsr_zero_async: hipMemsetAsync(ptr, 0, bytes) on the caller's stream (the gradient record the mirror
 * exchange's scatter-add accumulates into). */
int gsr_exchange_unpack(int64_t n, const float *recv, float *means2D, float *rgb, float *conic_opacity, int32_t *radii,
                        float *depths, gsr_stream_t stream);
int gsr_zero_async(void *ptr, size_t bytes, gsr_stream_t stream);
int gsr_exchange_pack_slab(int P, int B_total, int k0, int B, int W, int width, int height, int count_cameras,
                           int count_first, const float *means2D, const float *rgb, const float *conic_opacity,
                           const int32_t *radii, const float *depths, const int32_t *bands, const int32_t *chunkcnt,
                           const int32_t *counts, const int32_t *capacities, int64_t n_rows, float *msg,
                           int32_t *send_idx, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4  `simple_knn._C.distCUDA2(points)` (scene/gaussian_model.py:20,163-166; submodule
 * https://gitlab.inria.fr/bkerbl/simple-knn, .gitmodules:1-3, absent from the reference tree):
 * mean_dist2[i] = mean of the squared distances from point i to its 3 nearest OTHER points (only i itself is
 * excluded, by index; coincident points count with distance 0).  Exact (Morton order + bounded boxes only
 * prune the search).  With fewer than 4 points the mean runs over the neighbours that exist (0 for one point).
 * points: fp32 [P,3]; workspace: gsr_knn_workspace_bytes(P) bytes of device memory, any content. */
size_t gsr_knn_workspace_bytes(int P);
int gsr_knn_mean_dist2(int P, const float *points, float *mean_dist2, void *workspace, size_t workspace_bytes,
                       gsr_stream_t stream);

/* N4: the per-iteration densification statistics in ONE launch (ABI 12) -- densification.py:13-25 of the reference, run after
 * every backward of the densification phase: for the rows with radii > 0
 *   max_radii2D = max(max_radii2D, radii);  xyz_gradient_accum += |grad[:, :2]|;  denom += 1
 * (scene/gaussian_model.py:1046-1052 `add_densification_stats` + the max_radii2D update in front of it), without the
 * reference's boolean indexing (two `nonzero` host syncs + six gather / scatter kernels per camera and iteration).
 * grad: the means2D gradient (NDC-scaled, as the op returns it), rows `grad_stride` floats apart -- 9 for the view of K10's
 * [P,9] record that the operator hands out as means2D.grad, 2 for a dense [P,2]. */
int gsr_densify_stats(int64_t P, const int32_t *radii, const float *grad, int64_t grad_stride, float *max_radii2D,
                      float *accum, float *denom, gsr_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * N4  row primitives for densification / redistribution of the Gaussian shard.  The reference selects rows
 * with boolean indexing once PER TENSOR (and per destination rank): prune_points / _prune_optimizer
 * scene/gaussian_model.py:775-835, densify_and_clone / densify_and_split :922-1007, all2all_gaussian_state
 * :1073-1098.  Here the selection is computed once and applied to all tensors in one launch.
 *
 * gsr_group_rows: dest[i] in [0,G) = group of row i, anything else = dropped.  order[] receives the row
 *   indices grouped by destination, original order kept inside a group (group 0, 1, ..., G-1, then the dropped
 *   rows); counts[0..G-1] = group sizes, counts[G] = number dropped (device int64).  1 <= G <= 255.
 * gsr_gather_rows: for every tensor k, dst_k[r, 0:width_k] = src_k[order ? order[r] : r, 0:width_k] for
 *   r < n_out.  Rows are 4-byte words (fp32 / int32); strides are in words, so a dst may be a column block of a
 *   wider record matrix (one all-to-all-v for all per-Gaussian state) and a src may be such a block.
 *   srcs/dsts/widths/strides are HOST arrays of num_tensors <= 32 entries. */
size_t gsr_group_rows_bytes(int64_t N);
int gsr_group_rows(int64_t N, int G, const int32_t *dest, int32_t *order, int64_t *counts, void *workspace,
                   size_t workspace_bytes, gsr_stream_t stream);
int gsr_gather_rows(int64_t n_out, const int32_t *order, int num_tensors, const void *const *srcs, void *const *dsts,
                    const int32_t *widths, const int64_t *src_strides, const int64_t *dst_strides,
                    gsr_stream_t stream);
/* gsr_scatter_rows: the inverse, dst_k[order[r], 0:width_k] = src_k[r, 0:width_k] for r < n_in (rows not named in
 * order[0:n_in] keep their contents).  N2 (scene/gaussian_model.py:1350-1391, the sparse gradient sync of the
 * replicated-storage mode) packs the touched rows of the six gradient tensors into ONE compact [nnz,59] buffer with
 * gsr_gather_rows, all-reduces it, and writes the sums back with this call. */
int gsr_scatter_rows(int64_t n_in, const int32_t *order, int num_tensors, const void *const *srcs, void *const *dsts,
                     const int32_t *widths, const int64_t *src_strides, const int64_t *dst_strides,
                     gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4  one-pass densification event (new symbols, ABI unchanged).  The reference's densify_and_prune runs clone, split
 * and prune one after the other, each a boolean-index gather or a cat of every parameter and both Adam moments
 * (scene/gaussian_model.py:789-921: _prune_optimizer, prune_points, cat_tensors_to_optimizer, densification_postfix;
 * :922-1044: densify_and_split, densify_and_clone, densify_and_prune).  The result of that sequence is, in terms of the
 * ORIGINAL P rows,
 *     [ kept originals | kept clones | first children of the split rows whose children survive | second children ]
 * with the original order inside each segment, so it can be written in one pass.  The host classifies every row into one
 * byte (bits below); the plan ranks the rows, the move writes the result.
 *
 * gsr_densify_plan: one single-sweep scan (decoupled look-back, no sort) over cls[P].  ranks is int32 [4,P]: ranks[c*P+i]
 *   = number of rows j < i whose class has the bit of category c, categories in the order kept original, kept clone,
 *   parent with kept children, split parent.  counts (device int64 [4]) = {n_orig, n_clone, n_child, n_split} in the same
 *   order; n_child counts PARENTS (the result holds copies * n_child child rows).  split_rows (int32 [P], may be NULL):
 *   split_rows[ranks[3*P+i]] = i for every split parent, i.e. the first n_split entries list the split rows in order
 *   (the rows whose scales are the standard deviations of the reference's torch.normal draw, :933-936).
 *   P == 0 zeroes counts and returns 0.  P <= 2^31 - 1.
 * gsr_densify_move: one launch writes every destination row of num_tensors <= 32 tensors (4-byte words, strides in
 *   words, HOST tables as for gsr_gather_rows).  n_* are the plan's counts read back by the caller; dst_rows is the
 *   number of rows every destination can hold (>= n_orig + n_clone + copies * n_child, GSR_EINVAL otherwise).  Roles:
 *     COPY    every segment copies the source row (parameters other than xyz / scaling, send_to_gpui_cnt);
 *     MOMENT  kept originals copy, all new rows are zero (exp_avg / exp_avg_sq: cat_tensors_to_optimizer :854-893);
 *     XYZ     width 3; child k of parent i is R(rotation[i]) . samples[k * n_split + ranks[3*P+i]] + xyz[i] (:937-939,
 *             R as utils/general_utils.py:416-439 builds it: a correctly rounded sqrtf, true divisions, every product
 *             and sum rounded on its own -- the kernel is compiled without FP contraction; the dot is summed left to right);
 *     SCALING width 3; children take row i of alts[k], a dense [P,3] tensor (log(get_scaling / (0.8 * copies)), :940).
 *   rotation: dense [P,4]; samples: dense [copies * n_split, 3].  A source never aliases a destination.
 *   Arguments are validated before any device work; P == 0 returns 0. */
#define GSR_DENSIFY_KEEP_ORIGINAL 1
#define GSR_DENSIFY_KEEP_CLONE 2
#define GSR_DENSIFY_SPLIT_PARENT 4
#define GSR_DENSIFY_KEEP_CHILDREN 8
#define GSR_DENSIFY_ROLE_COPY 0
#define GSR_DENSIFY_ROLE_MOMENT 1
#define GSR_DENSIFY_ROLE_XYZ 2
#define GSR_DENSIFY_ROLE_SCALING 3
size_t gsr_densify_plan_bytes(int64_t P);
int gsr_densify_plan(int64_t P, const uint8_t *cls, int32_t *ranks, int32_t *split_rows, int64_t *counts,
                     void *workspace, size_t workspace_bytes, gsr_stream_t stream);
int gsr_densify_move(int64_t P, const uint8_t *cls, const int32_t *ranks, int64_t n_orig, int64_t n_clone,
                     int64_t n_child, int64_t n_split, int copies, int num_tensors, const void *const *srcs,
                     void *const *dsts, const void *const *alts, const int32_t *widths, const int32_t *roles,
                     const int64_t *src_strides, const int64_t *dst_strides, int64_t dst_rows, const float *rotation,
                     const float *samples, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * N4  fixed-budget densification: 3DGS-MCMC (new symbols, ABI unchanged; csrc/mcmc.hip).  Neither the reference nor its
 * rasterizer has it; the formulas are those of "3D Gaussian Splatting as Markov Chain Monte Carlo".  Dead rows are
 * teleported IN PLACE onto live rows drawn in proportion to opacity, the population grows by a host-known n_add rows,
 * and a state-dependent noise term moves the positions after every optimizer step.  No call reads anything back.
 * Determinism: every draw is Philox4x32-10 keyed by `seed` (low word first) with counter (row low, row high, event or
 * step, domain) -- domain 1 for the relocation draws, 2 for the noise -- so the same seed, event / step and inputs give
 * the same bits on any grid.  All arguments are validated before any launch (GSR_EINVAL); P == 0 returns 0 without one.
 * P + n_add <= 2^31 - 1.
 *
 * gsr_mcmc_relocate_bytes(rows) answers: how large a workspace does a plan over `rows` rows need (8-byte aligned)?
 * gsr_mcmc_relocate_plan answers: which row does every destination take its values from, and how often is each row
 *   drawn?  opacity_act: the ACTIVATED opacity, dense fp32 [P].  A row is dead iff opacity <= min_opacity (or NaN).
 *   Destinations: the dead rows and the new rows P .. P+n_add-1.  Weights w_i = dead ? 0 : (uint32)(opacity_i * 2^24),
 *   exclusive prefix sums in uint64 (three plain launches: tile sums, scan of the tile sums, draw).  Destination d draws
 *   r = mulhi64(x0 | x1 << 32, total) and takes the unique i with prefix[i] <= r < prefix[i] + w_i.
 *   src int32 [P+n_add]: the source row, -1 for a row that is no destination; count int32 [P]: draws per row; totals
 *   int64 [2] on the device: {n_dead, n_alive}.  total == 0 (no live row): every src is -1.  P == 0 writes nothing.
 *   A workspace smaller than gsr_mcmc_relocate_bytes(P), or not 8-byte aligned: GSR_EINVAL.
 * gsr_mcmc_relocate_apply answers: what do the rows hold after the event?  In place on num_tensors <= 32 tensors of
 *   4-byte words with at least P + n_add rows (HOST tables; strides in words).  With n = min(count_i + 1, n_max),
 *   1 <= n_max <= GSR_MCMC_N_MAX, evaluated in fp64 from opacity_act (o):
 *       o' = -expm1(log1p(-o) / n),   D = sum_{k=0}^{n-1} C(n,k+1) (-1)^k o'^(k+1) / sqrt(k+1),   f = o / D,
 *   o' then clamped to [min_opacity, 1 - 2^-23].  Roles:
 *     COPY     a destination copies its source's row bit for bit; sources keep theirs;
 *     OPACITY  width 1; source and destination become log(o' / (1 - o'));
 *     SCALING  width 3; source and destination become the source's OLD raw scale + log(f);
 *     MOMENT   zero on every source and every destination row, untouched elsewhere.
 *   Two launches: destinations first (they only read source rows), then the sources.  A destination is re-derived from
 *   opacity_act (row >= P or dead); src[] is clamped into [0, P) and must name a live row, else the row is left alone.
 * gsr_mcmc_noise answers: where are the positions after this iteration's noise?  In place, one launch:
 *       xyz += scaler * g(1 - sigmoid(opacity_raw)) * Sigma * xi,    g(x) = 1 / (1 + exp(-100 (x - 0.995))),
 *       Sigma = R diag(exp(scaling_raw))^2 R^T,  R = R(q / |q|) of rotation_raw (16-byte aligned, dense [P,4]).
 *   xi != NULL: dense [P,3] supplied by the caller; xi == NULL: drawn in the kernel, Box-Muller on
 *   u = ((x >> 8) + 0.5) * 2^-24 of the Philox words of (row, step): finite, |xi| <= 5.89.
 * gsr_mcmc_normals answers: which xi would gsr_mcmc_noise draw for rows 0 .. n-1 at (seed, step)?  out: dense [n,3].
 * gsr_mcmc_reg_grad answers: what are the gradients once the regulariser c_opacity * sum(sigmoid(opacity_raw)) +
 *   c_scale * sum(exp(scaling_raw)) is added?  In place: grad_opacity [P] += c_opacity * o (1 - o), grad_scaling [P,3]
 *   += c_scale * exp(s).  The caller folds lambda / count into the constants. */
#define GSR_MCMC_ROLE_COPY 0
#define GSR_MCMC_ROLE_MOMENT 1
#define GSR_MCMC_ROLE_OPACITY 2
#define GSR_MCMC_ROLE_SCALING 3
#define GSR_MCMC_N_MAX 51
size_t gsr_mcmc_relocate_bytes(int64_t rows);
int gsr_mcmc_relocate_plan(int64_t P, int64_t n_add, const float *opacity_act, float min_opacity, uint64_t seed,
                           uint32_t event, int32_t *src, int32_t *count, int64_t *totals, void *workspace,
                           size_t workspace_bytes, gsr_stream_t stream);
int gsr_mcmc_relocate_apply(int64_t P, int64_t n_add, const int32_t *src, const int32_t *count,
                            const float *opacity_act, float min_opacity, int n_max, int num_tensors,
                            void *const *tensors, const int32_t *widths, const int64_t *strides, const int32_t *roles,
                            gsr_stream_t stream);
int gsr_mcmc_noise(int64_t P, float *xyz, const float *scaling_raw, const float *rotation_raw,
                   const float *opacity_raw, float scaler, const float *xi, uint64_t seed, uint32_t step,
                   gsr_stream_t stream);
int gsr_mcmc_normals(int64_t n, uint64_t seed, uint32_t step, float *out, gsr_stream_t stream);
int gsr_mcmc_reg_grad(int64_t P, const float *opacity_raw, const float *scaling_raw, float c_opacity, float c_scale,
                      float *grad_opacity, float *grad_scaling, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K1 / K11 on the RAW parameters of GaussianModel (scene/gaussian_model.py:219-242): `scaling` log-scales
 * [P,3], `rotation` un-normalised quaternions [P,4], `opacity` logits [P,1], `features_dc` [P,1,3],
 * `features_rest` [P,sh_coeffs-1,3].  The getters' activations (scene/gaussian_model.py:109-129: exp,
 * normalize with eps 1e-12, sigmoid, cat) are applied in registers, so the activated copies are never
 * written to or re-read from HBM; outputs / saved tensors are those of gsr_preprocess_forward, and the
 * backward returns gradients with respect to the raw parameters.  Used by this package's
 * gaussian_renderer mirror; the reference-shaped entry points above remain the drop-in surface. */
int gsr_preprocess_forward_raw(int P, int sh_degree, int sh_coeffs, const float *xyz, const float *scaling,
                               float scale_modifier, const float *rotation, const float *features_dc,
                               const float *features_rest, const float *opacity, const float *viewmatrix,
                               const float *projmatrix, const float *campos, int width, int height, float tanfovx,
                               float tanfovy, float *means2D, float *depths, int32_t *radii, float *cov3D,
                               float *conic_opacity, float *rgb, uint8_t *clamped, gsr_stream_t stream);
int gsr_preprocess_backward_raw(int P, int sh_degree, int sh_coeffs, const float *xyz, const float *scaling,
                                float scale_modifier, const float *rotation, const float *features_dc,
                                const float *features_rest, const float *opacity, const float *viewmatrix,
                                const float *projmatrix, const float *campos, int width, int height, float tanfovx,
                                float tanfovy, const int32_t *radii, const float *cov3D, const uint8_t *clamped,
                                const float *dL_dmeans2D, const float *dL_dconic_opacity, const float *dL_drgb,
                                int grad_row_stride, float *dL_dxyz, float *dL_dscaling, float *dL_drotation, float *dL_dfeatures_dc,
                                float *dL_dfeatures_rest, float *dL_dopacity, gsr_stream_t stream);

/* The same for a BATCH of B cameras (--bsz B: every rank projects its Gaussians for all cameras of the batch,
 * gaussian_renderer/__init__.py:919-963) in one launch each way: a Gaussian's raw parameters are read once,
 * the backward sums the cameras' gradients in registers.  cams [B][40] floats on the device, per camera
 * { viewmatrix[16], projmatrix[16], campos[3], tanfovx, tanfovy, pad[3] }; outputs / incoming gradients are
 * camera-major [B,P,...]; cov3D [P,6] is camera independent. */
int gsr_preprocess_forward_raw_batched(int P, int B, int sh_degree, int sh_coeffs, const float *xyz,
                                       const float *scaling, float scale_modifier, const float *rotation,
                                       const float *features_dc, const float *features_rest, const float *opacity,
                                       const float *cams, int width, int height, float *means2D, float *depths,
                                       int32_t *radii, float *cov3D, float *conic_opacity, float *rgb,
                                       uint8_t *clamped, gsr_stream_t stream);
int gsr_preprocess_backward_raw_batched(int P, int B, int sh_degree, int sh_coeffs, const float *xyz,
                                        const float *scaling, float scale_modifier, const float *rotation,
                                        const float *features_dc, const float *features_rest, const float *opacity,
                                        const float *cams, int width, int height, const int32_t *radii,
                                        const float *cov3D, const uint8_t *clamped, const float *dL_dmeans2D,
                                        const float *dL_dconic_opacity, const float *dL_drgb, int grad_row_stride, float *dL_dxyz,
                                        float *dL_dscaling, float *dL_drotation, float *dL_dfeatures_dc,
                                        float *dL_dfeatures_rest, float *dL_dopacity, gsr_stream_t stream);

/* Camera (pose) gradients of K11: dL_dcams [B][40] in the layout of `cams` -- [0:16] dL/dviewmatrix (4x4 row-major,
 * row-vector convention), [16:32] dL/dprojmatrix, [32:35] dL/dcampos, [35:40] zeros (gradients with respect to tanfovx /
 * tanfovy are NOT provided).  Per visible Gaussian (radii > 0) and camera, with t = [p,1] viewmatrix[:, :3] and
 * p_hom = [p,1] projmatrix:
 *   viewmatrix[:, :3] += [p,1]^T (x) dL/dt, dL/dt from cov2D through the Jacobian exactly as K11 computes it (the same
 *     dL_da/db/dc with 1 / (denom^2 + 1e-7); a t.x / t.y clamped to +-1.3 tanfov is a constant);
 *   viewmatrix[:3, :3] += the gradient through Wc in cov2D = (J Wc) Sigma (J Wc)^T;  column 3 is exactly 0 (unused);
 *   projmatrix += [p,1]^T (x) dL/dp_hom from means2D (incoming gradient in K11's NDC-scaled convention); column 2 is
 *     exactly 0, column 3 (w) is not;
 *   campos -= the SH view-direction part of dL/dmean (clamped channels contribute 0; exactly 0 at sh_degree 0).
 * The reference's rasterizer has no camera gradient, so there is no reference call site for this entry point: the
 * formulas are the derivatives of its forward and oracle/torch_oracle.py's autograd is the arbiter.
 * SH coefficients: coefficient 0 at sh_dc + i * sh_dc_stride, coefficients 1.. at sh_rest + i * sh_rest_stride (strides
 * in floats) -- activated shs [P,M,3]: (shs, 3M, shs + 3, 3M); raw: (features_dc, 3, features_rest, 3(M-1)); sh_rest may
 * be NULL when sh_coeffs == 1; sh_rest_stride >= 3 ((sh_degree + 1)^2 - 1) (GSR_EINVAL otherwise).  sh_dc must not be
 * NULL but is never read (reserved): coefficient 0 does not depend on the view direction, so it has no camera gradient.  radii [B,P], clamped [B,P,3], cov3D [P,6] as saved by the forward; the three incoming
 * gradients are camera-major with the grad_row_stride convention of gsr_preprocess_backward (0 dense, 9 = column views
 * of a [B*P,9] record).  Rows with radii <= 0 contribute nothing and their gradient rows are never read.  The sums are
 * reduced without atomics (per-workgroup fp64 partial rows in `workspace`, which need not be zeroed, then a fixed-order
 * fp64 finalize): bit-identical from run to run.  workspace: 8-byte aligned, >= gsr_preprocess_backward_cams_bytes(P, B)
 * (GSR_ENOSPACE otherwise).  P == 0 writes zeros. */
size_t gsr_preprocess_backward_cams_bytes(int P, int B);
int gsr_preprocess_backward_cams(int P, int B, int sh_degree, int sh_coeffs, const float *means3D, const float *sh_dc,
                                 int sh_dc_stride, const float *sh_rest, int sh_rest_stride, const float *cams,
                                 int width, int height, const int32_t *radii, const float *cov3D,
                                 const uint8_t *clamped, const float *dL_dmeans2D, const float *dL_dconic_opacity,
                                 const float *dL_drgb, int grad_row_stride, void *workspace, size_t workspace_bytes,
                                 float *dL_dcams, gsr_stream_t stream);

/* K11 of a batch FUSED with the optimizer step of the six tensors it differentiates (N3 inside a9's neighbour: the
 * reference runs `loss.backward()` and then `gaussians.optimizer.step()` over the same 59 floats per Gaussian,
 * train_internal.py:195 and :316-328, scene/gaussian_model.py:292).  A Gaussian's gradient is complete when its lane
 * leaves the camera loop, so the dense Adam update (gsr_adam_step_multi's arithmetic, bit for bit) is applied there and
 * the gradients never reach HBM: xyz .. opacity are read AND updated in place; exp_avgs / exp_avg_sqs are host arrays of
 * the six device pointers of the moments in the order xyz, scaling, rotation, features_dc, features_rest, opacity; lrs ..
 * steps host arrays of the six groups' hyper-parameters (steps = the 1-based count AFTER this update); grad_scale as
 * in gsr_adam_step.  Needs sh_coeffs == 16 (GSR_EINVAL otherwise: run the two unfused calls).  tanfov0: HOST pointer
 * to { tanfovx, tanfovy } when B == 1 (selects the one-camera kernel like gsr_preprocess_backward_raw), or NULL. */
int gsr_preprocess_backward_adam_raw_batched(int P, int B, int sh_degree, int sh_coeffs, float *xyz, float *scaling,
                                             float scale_modifier, float *rotation, float *features_dc,
                                             float *features_rest, float *opacity, const float *cams, int width,
                                             int height, const int32_t *radii, const float *cov3D,
                                             const uint8_t *clamped, const float *dL_dmeans2D,
                                             const float *dL_dconic_opacity, const float *dL_drgb,
                                             int grad_row_stride, float *const *exp_avgs, float *const *exp_avg_sqs,
                                             const double *lrs, const double *beta1s, const double *beta2s,
                                             const double *epss, const int64_t *steps, float grad_scale,
                                             const float *tanfov0, gsr_stream_t stream);
/* The same launch for an iteration captured in a hipGraph (train_internal.py:134-208,316-329 replayed as one graph):
 * what changes from step to step is read from DEVICE memory at execution time -- dyn_dev: 12 floats, lr / (1 - beta1^t)
 * of the six tensors then 1 / sqrt(1 - beta2^t) of the six tensors (lrs / steps may then be NULL) -- and skip_flag_dev
 * (DEVICE uint32, may be NULL) makes the launch a no-op when non-zero (a capacity check of the same replay failed, see
 * gsr_flag_if_greater).  With both NULL this is gsr_preprocess_backward_adam_raw_batched. */
int gsr_preprocess_backward_adam_raw_batched_dyn(int P, int B, int sh_degree, int sh_coeffs, float *xyz, float *scaling,
                                                 float scale_modifier, float *rotation, float *features_dc,
                                                 float *features_rest, float *opacity, const float *cams, int width,
                                                 int height, const int32_t *radii, const float *cov3D,
                                                 const uint8_t *clamped, const float *dL_dmeans2D,
                                                 const float *dL_dconic_opacity, const float *dL_drgb,
                                                 int grad_row_stride, float *const *exp_avgs,
                                                 float *const *exp_avg_sqs, const double *lrs, const double *beta1s,
                                                 const double *beta2s, const double *epss, const int64_t *steps,
                                                 float grad_scale, const float *tanfov0, const float *dyn_dev,
                                                 const uint32_t *skip_flag_dev, gsr_stream_t stream);
/* The same dense launch reading K10's fp64 sums and row flags (gsr_render_backward_sums) where the others read a
 * record: acc64 / touched are HOST arrays of B <= 8 device pointers, camera c's [P,9] sums and [P] flags (GSR_EINVAL
 * for more cameras, a null entry or sums that are not 8-byte aligned).  A row whose flag is set in camera c and whose
 * radius there is > 0 has its nine sums converted with one (float) each -- means2D 0:2, rgb 2:5, conic_opacity 5:9, the
 * bits gsr_render_record_materialize stores -- and is differentiated as above.  A row whose flag is clear contributes
 * nothing for that camera, exactly as a culled one: its record row would be zeros.  Its sums, cov3D and clamp flags
 * are not read.  Parameters and second moments come out bit for bit as from the record; a first moment that is an
 * exact zero may differ in its sign (the zero-gradient path adds +0.0f where K11's arithmetic on zeros could add
 * -0.0f).  dyn_dev / skip_flag_dev as in _dyn, may be NULL. */
int gsr_preprocess_backward_adam_raw_batched_sums(int P, int B, int sh_degree, int sh_coeffs, float *xyz, float *scaling,
                                                  float scale_modifier, float *rotation, float *features_dc,
                                                  float *features_rest, float *opacity, const float *cams, int width,
                                                  int height, const int32_t *radii, const float *cov3D,
                                                  const uint8_t *clamped, const double *const *acc64,
                                                  const uint8_t *const *touched, float *const *exp_avgs,
                                                  float *const *exp_avg_sqs, const double *lrs, const double *beta1s,
                                                  const double *beta2s, const double *epss, const int64_t *steps,
                                                  float grad_scale, const float *tanfov0, const float *dyn_dev,
                                                  const uint32_t *skip_flag_dev, gsr_stream_t stream);

/* Sparse Adam: the fused K11 + Adam update over the rows that received a gradient (opt-in; LAZY Adam, not what the
 * reference's dense optimizer does -- so there is no reference call site for this entry point: the dense pair
 * gsr_preprocess_backward_raw_batched + gsr_adam_step_multi, restricted to the active rows, is the arbiter).
 * Row i is ACTIVE in a step iff some camera k < B has radii[k,i] > 0 and at least one of that camera's nine incoming
 * gradient words for the row compares != 0.0f.  The nine words are 2 of dL_dmeans2D, 3 of dL_drgb and 4 of
 * dL_dconic_opacity.
 *   - -0.0 counts as zero.
 *   - A NaN counts as non-zero, so a poisoned gradient is never hidden.
 *   - The gradient words of a (k,i) with radii[k,i] <= 0 must not influence anything.
 * K11 is linear in the incoming gradients and yields zeros for culled Gaussians, so the inactive rows are exactly the
 * rows whose six parameter gradients are zero by construction in the dense path.
 *   - Active rows get the dense fused update: the same K11 sums in the same order as the camera-batched kernel, then
 *     gsr_adam_step_multi's arithmetic with grad_scale.  Bias corrections come from the group's global step count
 *     (steps / dyn_dev), not from a count per row.
 *   - Inactive rows are not touched: parameters and both moments stay bit for bit what they were (the moments do not
 *     decay, the parameter does not coast on its momentum), and nothing is read from them beyond radii and, where
 *     radii > 0, the gradient words.
 *   - The caller advances the step counters of all six groups by one per step, as in the dense path.
 * P .. grad_row_stride and exp_avgs .. grad_scale exactly as in gsr_preprocess_backward_adam_raw_batched_dyn (there is
 * no tanfov0: one kernel serves every B, tanfov comes from the camera record), dyn_dev and skip_flag_dev as there.
 * Needs sh_coeffs == 16.  Three launches on `stream` and no host read-back (capturable in a hipGraph): the active rows
 * are compacted into a list in `workspace` (8-byte aligned, >= gsr_sparse_step_workspace_bytes(P), need not be zeroed,
 * private to the call until it has executed) and the update runs a grid of fixed size that takes the count from there.
 * The order of the list is not defined; every row is updated by exactly one lane, so the results do not depend on it.
 * active_out (DEVICE, [P] bytes, may be NULL): 1 for every updated row, 0 for the others.  num_active_dev (DEVICE word,
 * may be NULL): the number of active rows.  A non-zero skip word makes the call change nothing at all: active_out and
 * num_active_dev are then left untouched too.  Arguments are validated before any device work -- GSR_EINVAL: a null
 * pointer, sh_coeffs != 16, a negative size, rotation (or, with grad_row_stride == 0, a gradient) not aligned for its
 * vector loads; GSR_ENOSPACE: a workspace that is too small or not 8-byte aligned.  P == 0 returns 0. */
size_t gsr_sparse_step_workspace_bytes(int P);
int gsr_preprocess_backward_adam_raw_batched_sparse(int P, int B, int sh_degree, int sh_coeffs, float *xyz,
                                                    float *scaling, float scale_modifier, float *rotation,
                                                    float *features_dc, float *features_rest, float *opacity,
                                                    const float *cams, int width, int height, const int32_t *radii,
                                                    const float *cov3D, const uint8_t *clamped,
                                                    const float *dL_dmeans2D, const float *dL_dconic_opacity,
                                                    const float *dL_drgb, int grad_row_stride,
                                                    float *const *exp_avgs, float *const *exp_avg_sqs,
                                                    const double *lrs, const double *beta1s, const double *beta2s,
                                                    const double *epss, const int64_t *steps, float grad_scale,
                                                    const float *dyn_dev, const uint32_t *skip_flag_dev,
                                                    void *workspace, size_t workspace_bytes, uint8_t *active_out,
                                                    uint32_t *num_active_dev, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a19  fused parameter activations -- GaussianModel.get_scaling / get_rotation / get_opacity /
 * get_features (scene/gaussian_model.py:109-129): scales = exp(_scaling) [N,3], rotations =
 * normalize(_rotation) [N,4] (eps 1e-12), opacities = sigmoid(_opacity) [N,1], shs = cat(_features_dc
 * [N,1,3], _features_rest [N,sh_rest,3]) [N,1+sh_rest,3]; and the matching backward. */
int gsr_activate_forward(int N, int sh_rest, const float *scaling, const float *rotation, const float *opacity,
                         const float *features_dc, const float *features_rest, float *scales, float *rotations,
                         float *opacities, float *shs, gsr_stream_t stream);
int gsr_activate_backward(int N, int sh_rest, const float *rotation, const float *scales, const float *opacities,
                          const float *g_scales, const float *g_rotations, const float *g_opacities,
                          const float *g_shs, float *d_scaling, float *d_rotation, float *d_opacity,
                          float *d_features_dc, float *d_features_rest, gsr_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024), the companion of gsr_set_antialiasing's 2D filter.
 * There is NO reference call site for these five entry points: the reference has no such filter.  The float64
 * restatements of tests/filter3d_refs.py are the arbiter.
 *
 * Per Gaussian one scalar f >= 0, a world-space length: a Gaussian may not be smaller than the sampling interval of the
 * nearest training camera that sees it.  f acts through the scales and the opacity only,
 *     s'_k = sqrt(s_k^2 + f^2)  (k = 0..2, s = exp(_scaling)),      o' = sigmoid(_opacity) c,  c = prod_k s_k / s'_k.
 *
 * gsr_filter3d_distance: xyz [N,3], cams [C,40] (the records of the camera-batched K1: viewmatrix in floats 0..15,
 *   tanfovx / tanfovy in floats 35 / 36).  Per (row, camera): t = [p, 1] * viewmatrix with K1's expression, in K1's order
 *   and with one rounding per operation, so t.z has the bits K1 writes to `depths`; fx = width / (2 tanfovx) and
 *   fy = height / (2 tanfovy) as in K1.  The pair is VALID iff
 *       t.z > 0.2f,   |fx t.x| <= (0.65f width) t.z,   |fy t.y| <= (0.65f height) t.z
 *   (Mip-Splatting's 15 % margin around the screen, written without the division).  Per row: dist [N] = min t.z over the
 *   valid cameras (0 when there is none) and seen [N] = 1 / 0.  partials [gsr_filter3d_num_partials(N)]: per workgroup
 *   the max of dist over its rows; 0 = none seen, which no valid t.z can be.  No atomics.
 * gsr_filter3d_finalize: m = *global_max when global_max != NULL (a device float: the max over ALL ranks' partials, which
 *   a caller at world size > 1 forms with one MAX all-reduce between the two calls; partials may then be NULL), else the
 *   max of the n_partials partials (n_partials must be gsr_filter3d_num_partials(N)).  filter_out [N]:
 *       f = (float32(sqrt(0.2)) d) / focal_max,   d = dist of a seen row,  d = m of an unseen row
 *   (Mip-Splatting's distance[~valid] = distance[valid].max()), and f = 0 for every row when m == 0: the identity filter.
 *   focal_max: the largest fx over the cameras, formed by the caller on the host; must be > 0.
 * gsr_filter3d_apply_forward: (_scaling [N,3], _opacity [N], filter [N]) -> the EFFECTIVE RAW parameters
 *       scaling_eff_k = log s'_k = (1/2) log(exp(2 _scaling_k) + f^2),      opacity_eff = logit(sigmoid(_opacity) c),
 *   which the raw K1 / K11 entry points take in place of _scaling / _opacity.  Computed in log space -- with
 *   d_k = log(f^2 / s_k^2):  log(s'_k / s_k) = (max(d_k, 0) + log1p(exp(-|d_k|))) / 2,  log c = -(their sum),
 *   opacity_eff = _opacity + log c - log1p((1 - c) exp(_opacity)) -- so that no product of squared scales is formed.
 *   A row with f == 0 returns its inputs bit for bit.
 * gsr_filter3d_apply_backward: with g_s [N,3], g_o [N] the gradients of the effective tensors, sigma = sigmoid(_opacity),
 *   r_k = s_k^2 / s'_k^2 and p = sigma c:
 *       d_scaling_k = g_s_k r_k + g_o (1 - r_k) / (1 - p),      d_opacity = g_o (1 - sigma) / (1 - p),
 *   with 1 - r_k = f^2 / s'_k^2 and 1 - p = (1 - sigma) + sigma (1 - c) formed without a subtraction.  f gets no
 *   gradient.  A row with f == 0 returns g_s, g_o bit for bit.
 * All: N == 0 returns 0 without a launch; a NULL pointer that would be dereferenced, N < 0, C < 0 or a non-positive
 * image size return GSR_EINVAL. */
int gsr_filter3d_num_partials(int N);
int gsr_filter3d_distance(int N, int C, const float *xyz, const float *cams, int width, int height, float *dist,
                          uint8_t *seen, float *partials, gsr_stream_t stream);
int gsr_filter3d_finalize(int N, const float *dist, const uint8_t *seen, const float *partials, int n_partials,
                          const float *global_max, float focal_max, float *filter_out, gsr_stream_t stream);
int gsr_filter3d_apply_forward(int N, const float *scaling, const float *opacity, const float *filter,
                               float *scaling_eff, float *opacity_eff, gsr_stream_t stream);
int gsr_filter3d_apply_backward(int N, const float *scaling, const float *opacity, const float *filter,
                                const float *g_scaling, const float *g_opacity, float *d_scaling, float *d_opacity,
                                gsr_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * N1g  bilateral-grid colour correction per training image (Wang et al., "Bilateral Guided Radiance Field Processing").
 * There is no reference call site (the reference has no such model); the arbiter is the fp64 torch restatement of the
 * lines below (tests/bilagrid_refs.py).  New symbols only: gsr_abi_version does not move.
 *
 * One camera's grid G[12][gl][gh][gw], float32, 2 <= gl <= 16, 2 <= gh, gw <= 64; coefficient j = 4c + k is entry [c][k]
 * of a row-major [3,4] matrix [A | b].  For the pixel (x, y) of a width x height image with colour c = (r, g, b):
 *       px = (x + 0.5) / width * (gw - 1),   py = (y + 0.5) / height * (gh - 1),
 *       pz = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) * (gl - 1)      (products and sums rounded one by one, in this order),
 *       M  = the trilinear sample of the 12 planes: lower node i0 = min(floor(p), size - 2), t = p - i0, every axis as
 *            a + t (b - a) (x, then y, then z) -- grid_sample(bilinear, align_corners, border) of a 5-D input,
 *       x' = A_M c + b_M        (no clamp; an identity grid returns c bit for bit).
 * y is the row of the FULL image.  `image`, `out`, `grad_out`, `grad_image` point at row 0 of channel 0 of [3, height,
 * width] images (rows dense, channels their stride apart); only the rows [y0, y1) are read or written.
 *
 * gsr_bilagrid_slice_forward: out <- x' for the rows of the band.
 * gsr_bilagrid_slice_backward: with g' = grad_out,
 *       grad_grid[j][node] = sum over the band's pixels of w_node g'_c (c_k, or 1 for k = 3)      (fully overwritten:
 *            nodes no pixel of the band reaches get zeros),
 *       grad_image[k] = sum_c A_M[c][k] g'_c + lum_k (gl - 1) D,    D = sum_j dM_j/dpz (g' (x) [c, 1])_j,
 *            dM_j/dpz = the bilinear-in-xy sample of G[j][i0z + 1] - G[j][i0z],  D = 0 exactly where the luminance is
 *            <= 0 or >= 1 (the band's rows, fully written).
 *   A workgroup owns at most 32 x 32 pixels of one xy-cell and writes its 4 * gl * 12 corner sums once to `partials`
 *   (gsr_bilagrid_num_partials(...) floats, scratch, fully written); a second launch adds the rows around each node in a
 *   fixed order in fp64 and rounds once.  No floating-point atomics: the same bits on every run.
 * gsr_bilagrid_num_partials: pure host arithmetic; 0 for sizes the launches refuse.
 * Both: GSR_EINVAL before any device work for a null pointer, grid sizes out of range, width or height <= 0 (or > 2^24),
 * y0 < 0, y1 > height, y0 > y1.  An empty band (y0 == y1) launches nothing, except that the backward clears grad_grid. */
int gsr_bilagrid_slice_forward(int width, int height, int y0, int y1, const float *image, int64_t image_channel_stride,
                               const float *grid, int gw, int gh, int gl, float *out, int64_t out_channel_stride,
                               gsr_stream_t stream);
int64_t gsr_bilagrid_num_partials(int width, int height, int gw, int gh, int gl);
int gsr_bilagrid_slice_backward(int width, int height, int y0, int y1, const float *image, int64_t image_channel_stride,
                                const float *grid, int gw, int gh, int gl, const float *grad_out,
                                int64_t grad_out_channel_stride, float *grad_image, int64_t grad_image_channel_stride,
                                float *partials, float *grad_grid, gsr_stream_t stream);
/* Total variation of num_grids grids [num_grids][12][gl][gh][gw]:
 *       T = (1 / num_grids) sum over the axes z, y, x of mean((G shifted by one along the axis - G)^2),
 * the mean over the 12 (size_axis - 1) (other two sizes) differences of one grid.  gsr_bilagrid_tv ADDS weight * dT/dG to
 * `grad` (same shape) in one launch.  value != NULL: also *value = T, the per-workgroup sums in fp64 through `partials`
 * (gsr_bilagrid_tv_num_partials(...) doubles) and one more single-workgroup launch that adds them in a fixed order;
 * value and partials are given together or not at all.  GSR_EINVAL before any device work: num_grids <= 0, sizes out of
 * range, a null grids / grad, one of value / partials without the other.  The optimizer step is gsr_adam_step. */
int gsr_bilagrid_tv_num_partials(int num_grids, int gw, int gh, int gl);
int gsr_bilagrid_tv(int num_grids, int gw, int gh, int gl, const float *grids, float weight, float *grad,
                    double *partials, float *value, gsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRASTER_H */
