/*
 * gsr.h -- C ABI of libgsr_hip.so: the MI355X (gfx950) Gaussian-splatting
 * rasterizer that replaces the third-party CUDA extension
 * `diff_gaussian_rasterization` (requirements.txt:17 of the reference) behind
 * the reference's own call site src/model/decoder/cuda_splatting.py:101-129.
 *
 * Plain C: device pointers, sizes, a hipStream_t passed as void*.  No torch
 * types, no global state, re-entrant per stream, never throws; every entry
 * point returns 0 or a negative GSR_E* code.  The caller owns ALL memory
 * (outputs, the opaque workspace that carries geometry/binning/image state
 * from forward to backward -- the counterpart of upstream's geomBuffer /
 * binningBuffer / imgBuffer).
 *
 * Reference interface each entry point replaces:
 *   gsr_forward   <- _C.rasterize_gaussians(...)           as invoked by
 *                    GaussianRasterizer.forward, cuda_splatting.py:120-129
 *                    (one call per view there; V views per call here)
 *   gsr_backward  <- _C.rasterize_gaussians_backward(...)  invoked by autograd
 *                    for the same call (grads for means3D, means2D, shs /
 *                    colors_precomp, opacities, cov3D_precomp, theta, rho)
 *   GsrView       <- GaussianRasterizationSettings fields  cuda_splatting.py:101-115
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_EINVAL (-1)     /* bad dimension / null pointer / unsupported degree */
#define GSR_ENOSPACE (-2)   /* workspace_bytes too small for (dims, pair_capacity) */
#define GSR_ELAUNCH (-3)    /* a kernel launch failed (hipGetLastError != success) */

#define GSR_TILE 16
#define GSR_VIEW_FLOATS 64

/* Per-view camera block, 64 floats = 256 B, array of V in DEVICE memory.
 * Matrices are the row-vector ("transposed") 4x4 form the reference passes
 * (cuda_splatting.py:85-88), flat index m[4*r+c]. */
typedef struct GsrView {
    float viewmatrix[16];     /* settings.viewmatrix      (:108) */
    float projmatrix[16];     /* settings.projmatrix      (:109) */
    float projmatrix_raw[16]; /* settings.projmatrix_raw  (:110) */
    float campos[3];          /* settings.campos          (:112) */
    float tanfovx, tanfovy;   /* settings.tanfovx/y       (:104-105) */
    float bg[3];              /* settings.bg              (:106) */
    float scale;              /* scene scale folded into the kernel: means*scale, cov*scale^2
                                 (the make_scale_invariant step, cuda_splatting.py:65-72); 1 = none */
    float pad[7];
} GsrView;

/* Problem dimensions.  V = B * Vt views are rendered per call; view v looks at
 * the Gaussians of scene v / Vt (the (b v) flattening of
 * decoder_splatting_cuda.py:51-63 WITHOUT replicating the Gaussian arrays). */
typedef struct GsrDims {
    int32_t B;          /* scenes (independent Gaussian sets) */
    int32_t Vt;         /* views per scene */
    int32_t G;          /* Gaussians per scene */
    int32_t H, W;       /* image size (all views) */
    int32_t M;          /* SH coefficients per channel in `shs` (G,M,3); 0 => `shs` is precomputed RGB (G,3) */
    int32_t sh_degree;  /* active degree 0..4, (sh_degree+1)^2 <= M */
    int32_t flags;      /* GSR_FLAG_* */
    void *profile;      /* optional GsrProfile* (gsr_profile_create): per-stage hipEvent timing; NULL = off */
} GsrDims;

#define GSR_FLAG_NTOUCHED 1  /* forward: also count n_touched (one extra global atomic per tile and splat) */
#define GSR_FLAG_COV9 2      /* cov6 / dL_dcov6 are full row-major 3x3 matrices (B,G,3,3): the kernels read the
                                upper triangle and write the gradient there (lower triangle 0), which is what
                                autograd produces for covariances[:, triu] (cuda_splatting.py:118,126) */
#define GSR_FLAG_PHASE_BIN 4     /* gsr_forward: enqueue only preprocess + tile scan.  `status` is FINAL after them
                                    (pair count, overflow), so the host can read it back while nothing expensive is
                                    queued, grow the workspace if needed, and then ...                              */
#define GSR_FLAG_PHASE_RENDER 8  /* ... call gsr_forward again with identical arguments + this flag: scatter, per-tile
                                    sort and composite run on the workspace the PHASE_BIN call prepared.  The host
                                    then returns with ~1 ms of GPU work still queued, which hides the launch latency
                                    of everything it enqueues next (loss, backward).  Neither flag: all stages.     */

#define GSR_FLAG_PREZERO_GRADS 16 /* gsr_forward: the composite kernel also zeroes the workspace's per-(view, Gaussian) gradient
                                    accumulators (126 MB at the headline size; that kernel is VALU-bound, HBM is idle under it).
                                    gsr_backward with the same flag then skips its own memset.  Valid for the FIRST backward
                                    after the forward only: the backward leaves the accumulators dirty. */
#define GSR_FLAG_BIN_BALLOT 32    /* K1 / K3 bin with wave-aggregated global atomics (the path of images beyond 4 096 tiles per view) even where
                                    the per-workgroup LDS histograms apply: A/B runs and the equivalence test */
#define GSR_FLAG_K6_SWAP_SUM 64   /* gsr_backward without a depth gradient: the composite backward sums its nine per-splat partials with the two
                                    permlane-swap levels (the form before the LDS transpose, and still the one of the depth-gradient kernel)
                                    instead of through the LDS: A/B runs and the parity test.  Same sums up to the order of a 64-term fp32 add */
#define GSR_FLAG_SORT_KEYS_SHIFT 8   /* bits 8-9: LDS budget of the per-tile depth sort: 0 = 4096 keys (default), 1 = 1024,
                                       2 = 2048.  Pick the smallest budget >= the longest per-tile list expected
                                       (status[GSR_ST_MAX_TILE] of an earlier call): more workgroups fit a CU.  Longer lists
                                       remain correct (sorted in global memory), only slower. */
#define GSR_FLAG_SEG_SHIFT 10        /* bits 10-12: length L of the depth segments the composite backward cuts a tile's list into (one
                                        work unit per segment, started from a checkpoint the composite forward stored at its end):
                                        0 = by size (gsr_common.h seg_len), 1 = 64, 2 = 128, 3 = 192, 4 = 256, 5 = 384, 7 = one segment
                                        per tile.  Part of the workspace layout: the forward and the backward of a call pass the same. */

#define GSR_FLAG_STYLES_CHUNK_SHIFT 13 /* bits 13-15, gsr_forward_styles only: the most styles one composite launch shades, 2 .. 4 (0 = 4).
                                        More styles are served by further composite launches over the same sorted lists. */

/* status words written by gsr_forward (device int32[GSR_STATUS_WORDS]) */
#define GSR_STATUS_WORDS 8
#define GSR_ST_PAIRS 0       /* R: total (tile, Gaussian) pairs over all views (low 32 bits) */
#define GSR_ST_OVERFLOW 1    /* 1 if R > pair_capacity: outputs are INVALID, re-run with a larger capacity */
#define GSR_ST_MAX_TILE 2    /* longest per-tile list */
#define GSR_ST_PAIRS_HI 3    /* high 32 bits of R */
#define GSR_ST_UNITS 4       /* work units of the composite backward (GsrLayout.unit_order); 0 on overflow */

/* Named offsets into the workspace (bytes), for the parity tests and the bench. */
typedef struct GsrLayout {
    size_t records;      /* SplatRec[V*G], 48 B each: x,y,depth,radius+flags | conic A,B,C,opacity | r,g,b,extents */
    size_t tile_count;   /* uint32[V*T]     per-tile list length */
    size_t tile_offset;  /* uint32[V*T+1]   exclusive scan; ranges[t] = [off[t], off[t+1]) */
    size_t tile_cursor;  /* uint32[V*T]     scatter cursors */
    size_t pairs;        /* uint64[cap]     (depth_bits << 32 | id), bucketed by (view, tile) */
    size_t point_list;   /* uint32[cap]     per-tile depth-sorted Gaussian ids in bits 0..27 (GSR_ID_MASK; G < 2^28 by the record-offset limit
                            below).  Bits 28..31 are written by the composite forward and read by the backward: bit 28 + q = the entry's
                            alpha >= 1/255 footprint can reach 8x8 quadrant q (TL, TR, BL, BR) of its tile -- what the forward hands
                            the backward instead of a separate mask stream (round 6; rounds 2-5: a byte, then a 32-bit word per entry) */
    size_t final_T;      /* float[V*H*W] */
    size_t n_contrib;    /* uint32[V*H*W] */
    size_t grad_rec;     /* float[V*G*12]   backward per-(view,Gaussian) accumulators */
    size_t status;       /* int32[GSR_STATUS_WORDS] internal copy */
    size_t tile_order;   /* uint32[V*T]     (view*T + tile) ids, longest list first: launch order of the composite kernels */
    size_t pairs_alt;    /* uint64[cap]     bucket space of the per-tile sort for lists longer than its LDS budget */
    size_t loss_partial; /* float[V*T + V]  fused MSE: per-tile sums of squared errors, then per-view sums (fixed-order reduction) */
    size_t loss_ticket;  /* uint32[V + 1]   fused MSE: arrival counters of a view's tiles / of the views; zeroed by the tile scan */
    size_t loss_diff;    /* float[V*3*H*W]  fused MSE: image - target as the composite forward had it in registers; the backward scales it
                            to dL/dimage (one 12-byte read per pixel, as with a dL_dimage from outside) */
    size_t final_C;      /* float4[V*H*W]   (r, g, b, depth) accumulated by the composite forward, background not added; written for tiles
                            of more than one depth segment (the backward's segments start from final_C minus a checkpoint) */
    size_t ckpt;         /* checkpoint slots of 256 pixels, 5 KiB each: float4 (T, r, g, b prefix)[4 quadrants][64 lanes], then float depth
                            prefix[4][64].  Tile t's boundary m L (m = 1, 2, ...) is slot tile_offset[t] / L + m - 1: at most cap / L slots */
    size_t unit_order;   /* uint32[2][units] (view*T + tile, depth segment) work units of the composite backward, longest first */
    size_t geo;          /* float4[V*G]     bit-exact copy of each record's first 16 bytes (x, y, depth, radius+flags): the scatter and the
                            preprocess backward stream these instead of striding through the 48-byte records */
    size_t opac;         /* float[B*G]      the opacities the forward read, kept for the preprocess backward */
    size_t scan;         /* uint32[1024 + 8 * ceil(V*T / 256)]  what the launches of the tile scan hand each other: class counts, class cursors,
                            per-workgroup partial sums */
    size_t total;        /* total bytes */
} GsrLayout;

#define GSR_ID_MASK 0x0fffffffu
#define GSR_QUAD_SHIFT 28

/* Size/offsets of the workspace for (dims, pair_capacity).  Returns GSR_OK or GSR_EINVAL.
 * Limits: pair_capacity < 2^32; G * 48 bytes < 2^32 (the composite kernels address one view's records with 32-bit byte offsets; hence
 * ids < 2^27 and the four mask bits of a point_list word are free). */
int gsr_workspace_layout(const GsrDims *dims, int64_t pair_capacity, GsrLayout *out);

/*
 * Forward for V = B*Vt views.  All pointers are device pointers.
 *   views   GsrView[V]
 *   means   float (B,G,3); cov6 float (B,G,6) xx,xy,xz,yy,yz,zz; opac float (B,G);
 *   shs     float (B,G,M,3) or, when M == 0, RGB (B,G,3)
 * Outputs: image (V,3,H,W), depth (V,H,W), opacity (V,H,W), radii int32 (V,G),
 *          n_touched int32 (V,G) (may be NULL unless GSR_FLAG_NTOUCHED),
 *          status int32[GSR_STATUS_WORDS] -- device memory, or device-accessible pinned HOST memory: the tile scan stores the
 *          words there directly and the host reads them behind an event, no copy kernel.
 * The call only enqueues work on `stream` (no host sync).  If status[GSR_ST_OVERFLOW]
 * is set the images are invalid and the call must be repeated with
 * pair_capacity >= status[GSR_ST_PAIRS].
 */
int gsr_forward(const GsrDims *dims, const GsrView *views, const float *means, const float *cov6,
                const float *opac, const float *shs, int64_t pair_capacity, void *workspace,
                size_t workspace_bytes, float *image, float *depth, float *opacity, int32_t *radii,
                int32_t *n_touched, int32_t *status, void *stream);

/*
 * Backward of the same call (workspace must be the one the forward filled).
 *   dL_dimage (V,3,H,W); dL_ddepth (V,H,W) or NULL.
 * Outputs (overwritten): dL_dmeans (B,G,3), dL_dcov6 (B,G,6), dL_dopac (B,G),
 *   dL_dshs (B,G,M,3) or (B,G,3); optional (NULL to skip): dL_dmeans2D (V,G,3)
 *   screen-space mean gradient (z = 0), dL_dtau (V,6) = (rho, theta) pose gradient
 *   of a left se(3) perturbation of each view's world->camera transform.
 */
int gsr_backward(const GsrDims *dims, const GsrView *views, const float *means, const float *cov6,
                 const float *shs, int64_t pair_capacity, void *workspace, size_t workspace_bytes,
                 const float *dL_dimage, const float *dL_ddepth, float *dL_dmeans, float *dL_dcov6,
                 float *dL_dopac, float *dL_dshs, float *dL_dmeans2D, float *dL_dtau, void *stream);

/*
 * The same two calls with the per-step host / launch overhead folded into the kernels (round 6).  `fx` may be NULL (= the plain calls).
 *   tile_count   optional PERSISTENT per-tile counters, uint32[V*T] of device memory the caller zeroed ONCE at allocation and keeps per
 *                stream: the preprocess counts into them and the tile scan leaves them zero again, so no memset runs in front of the
 *                forward.  NULL: the counters of the workspace, zeroed by the call itself.
 *   mse_target   optional (V,3,H,W): `LossMse.forward` (src/loss/loss_mse.py:22-31) fused into the composite kernels --
 *                forward: the composite kernel sums (image - target)^2 per tile while the pixels are still in registers, the last tile of
 *                  every view and the last view add the partials in index order (deterministic), mse_loss[0] = mse_weight * mean;
 *                backward: the composite kernel forms dL/dimage = dL_dimage (may be NULL) + 2 mse_weight / n * mse_grad_loss[0] *
 *                  (image - target) in its prologue from the difference the forward left in the workspace -- two kernels less than
 *                  gsr_mse_forward / gsr_mse_backward around the plain calls, same values.  (The backward needs mse_target only as the
 *                  "fused" switch and mse_weight / mse_grad_loss for the coefficient.)
 *   mse_grad_loss  device fp32[1], the upstream gradient of the loss; NULL = 1.
 */
typedef struct GsrFused {
    uint32_t *tile_count;
    const float *mse_target;
    float mse_weight;
    float *mse_loss;             /* forward: out, device fp32[1] */
    const float *mse_grad_loss;  /* backward: in */
} GsrFused;
int gsr_forward_fused(const GsrDims *dims, const GsrView *views, const float *means, const float *cov6,
                      const float *opac, const float *shs, int64_t pair_capacity, void *workspace,
                      size_t workspace_bytes, float *image, float *depth, float *opacity, int32_t *radii,
                      int32_t *n_touched, int32_t *status, const GsrFused *fx, void *stream);
int gsr_backward_fused(const GsrDims *dims, const GsrView *views, const float *means, const float *cov6,
                       const float *shs, int64_t pair_capacity, void *workspace, size_t workspace_bytes,
                       const float *dL_dimage, const float *dL_ddepth, float *dL_dmeans, float *dL_dcov6,
                       float *dL_dopac, float *dL_dshs, float *dL_dmeans2D, float *dL_dtau, const GsrFused *fx,
                       void *stream);

/*
 * The composite backward's nine-value wave reduction on its own.  variant 0: the LDS transpose (default of the depth-free kernel),
 * 1: the permlane-swap form (GSR_FLAG_K6_SWAP_SUM).
 *   gsr_k6_blocks_per_cu  hipOccupancyMaxActiveBlocksPerMultiprocessor of the depth-free composite backward (64 threads, its static LDS);
 *                         negative: GSR_ELAUNCH
 *   gsr_test_reduce9      test entry: `blocks` single-wave workgroups, each runs `rounds` reductions back to back as the kernel does on
 *                         consecutive (tile, splat) pairs.  in: device fp32 (blocks, rounds, 9, 64), value i of lane l; out: device fp32
 *                         (blocks, rounds, 9), the totals, each stored by the lane the variant's slot map names.
 */
int gsr_k6_blocks_per_cu(int variant);
int gsr_test_reduce9(const float *in, float *out, int rounds, int blocks, int variant, void *stream);

/*
 * Multi-style forward (inference): S Gaussian sets that share means / covariances / opacities and differ only in colour, rendered
 * through the same V views in one pass.  Geometry, binning, tile scan, scatter and the per-tile depth sort run ONCE (the kernels of
 * gsr_forward); the composite walks every tile's list once per launch of up to 4 styles and accumulates all of their colours.
 *   shs      HOST array of S device pointers, each (B,G,M,3) or, when M == 0, RGB (B,G,3)
 *   extra    device memory of gsr_styles_extra_bytes(dims, S) bytes (0 for S == 1, then it may be NULL): the colours of styles 1..S-1,
 *            16 bytes per (style, view, Gaussian) -- per (style, scene, Gaussian) at sh_degree 0 / M == 0, where the colour does not
 *            depend on the view.  Style 0's colour lives in the workspace's splat records as in gsr_forward.
 *   tile_count  optional persistent per-tile counters, as GsrFused.tile_count (NULL: the workspace's, zeroed by the call)
 * Outputs: image (S,V,3,H,W); ONE depth (V,H,W), opacity (V,H,W), radii (V,G); status as gsr_forward.
 * The workspace is the one of gsr_workspace_layout, unchanged, and is left as gsr_forward on style 0 leaves it (sorted lists with the
 * quadrant-mask bits, final_T, n_contrib) except for what only a backward reads: there is NO backward for this call, and
 * GSR_FLAG_NTOUCHED / GSR_FLAG_PREZERO_GRADS are rejected (GSR_EINVAL).  GSR_FLAG_PHASE_BIN / _RENDER work as in gsr_forward.
 * S == 1 forwards to gsr_forward.
 */
size_t gsr_styles_extra_bytes(const GsrDims *dims, int32_t S);   /* 0 for invalid dims or S < 1 */
int gsr_forward_styles(const GsrDims *dims, int32_t S, const GsrView *views, const float *means, const float *cov6,
                       const float *opac, const float *const *shs, int64_t pair_capacity, void *workspace, size_t workspace_bytes,
                       void *extra, size_t extra_bytes, uint32_t *tile_count, float *image, float *depth, float *opacity,
                       int32_t *radii, int32_t *status, void *stream);

/*
 * Camera set-up of `render_cuda` (cuda_splatting.py:65-88) for V views in ONE launch: the 1/near rescale
 * of make_scale_invariant, get_fov (projection.py:247-261), get_projection_matrix (:16-43), inverse(c2w)^T
 * and view @ proj, written as GsrView[V].  Replaces ~100 tiny device ops of the torch formulation.
 *   c2w (V,4,4) camera-to-world, K (V,3,3) normalised intrinsics, near/far (V), bg (V,3) -- device, row-major.
 */
int gsr_build_views(const float *c2w, const float *K, const float *near, const float *far, const float *bg, int32_t V,
                    int32_t scale_invariant, GsrView *out, void *stream);

/*
 * MSE consumer of the rendered colour, `LossMse.forward` (src/loss/loss_mse.py:22-31):
 *   loss = weight * mean((pred - target)^2)            -- one launch, deterministic (ticketed partial sums)
 *   dL/dpred = (2 weight / n) * grad_loss[0] * (pred - target)   -- one launch, upstream gradient read on device
 * pred/target/grad_pred: device fp32[n], 16-byte aligned; loss, grad_loss: device fp32[1];
 * scratch: device buffer of gsr_mse_scratch_bytes() bytes, zeroed ONCE by the caller at allocation (the
 * kernel re-arms it), not shared between streams.
 */
size_t gsr_mse_scratch_bytes(void);
int gsr_mse_forward(const float *pred, const float *target, int64_t n, float weight, void *scratch, float *loss,
                    void *stream);
int gsr_mse_backward(const float *pred, const float *target, const float *grad_loss, int64_t n, float weight,
                     float *grad_pred, void *stream);

/*
 * Edge-aware depth smoothness, `LossDepth.forward` (src/loss/loss_depth.py:26-60), for N = b * v views, device fp32, contiguous:
 *   n    = (max(min(depth, hi), lo) - lo) / (hi - lo) with lo = log(near[view]), hi = log(far[view]) -- the bounds are logs, the depth is
 *          NOT logged: that is the reference's arithmetic and it is reproduced
 *   t_x  = n[x+1] - n[x], or with second_derivative (n[x+2] - n[x+1]) - (n[x+1] - n[x]); t_y the same down the columns
 *   image (N,3,H,W) given: t_x *= exp(-sigma_image * c_x), c_x = max over the channels of the SIGNED difference image[x+1] - image[x]
 *          (second_derivative: the larger of the two neighbouring c_x); t_y likewise.  image NULL: no bilateral term, sigma_image unread
 *   loss = weight * (mean |t_x| + mean |t_y|)     (the two means have N H (W-k) and N (H-k) W elements, k = 1 or 2)
 * fwd: one pass + a one-workgroup fold of per-workgroup float64 partials in a fixed order: two launches, no atomics, bit-identical from
 *      run to run.  bwd: one launch in gather form, every element of grad_depth (N,H,W) written exactly once, nothing to zero:
 *      dL/ddepth = weight * grad_loss[0] / count_axis / (hi - lo) * (sum of the signs x weights of the differences the pixel is part of)
 *      * (1 inside the bounds, 1/2 exactly at a bound, 0 outside: torch's minimum / maximum), with sign(0) = 0.  grad_loss: device fp32[1],
 *      NULL = 1.  lo, hi, 1 / (hi - lo) in float64 from the fp32 near / far, per-pixel arithmetic fp32.  Rows need no alignment.
 * scratch: device memory of gsr_depth_smooth_scratch_bytes() (0 for invalid dimensions), no initialisation, not shared between
 * concurrent calls.  GSR_EINVAL before any launch: N < 1, H or W < 2 (< 3 with second_derivative; the reference returns NaN, the mean
 * of an empty tensor), more than 2^24 - 1 tiles of 128 x 8 pixels, NULL depth / near / far / loss / grad_depth / scratch.
 */
size_t gsr_depth_smooth_scratch_bytes(int64_t N, int H, int W);
int gsr_depth_smooth_fwd(const float *depth, const float *image, const float *near, const float *far, int64_t N, int H, int W,
                         float weight, float sigma_image, int second_derivative, void *scratch, float *loss, void *stream);
int gsr_depth_smooth_bwd(const float *depth, const float *image, const float *near, const float *far, const float *grad_loss,
                         int64_t N, int H, int W, float weight, float sigma_image, int second_derivative, float *grad_depth,
                         void *stream);

/*
 * Image scores of the test step (src/evaluation/metrics.py:11-52) for N image pairs (N,C,H,W), device fp32, contiguous:
 *   ssim[n] = mean over c of skimage structural_similarity(gt[n], pred[n], win_size=11, gaussian_weights=True, channel_axis=0,
 *             data_range=1.0): Gaussian window sigma 1.5 / radius 5, sample covariance (x 121/120), C1 = 1e-4, C2 = 9e-4, the map
 *             averaged over the (H-10) x (W-10) pixels left after skimage's crop of 5; inputs NOT clipped
 *   mse[n]  = mean over C*H*W of (clip(gt,0,1) - clip(pred,0,1))^2, the argument of compute_psnr's -10 log10
 * Two launches (one pass over both images, one fold of per-tile partials per image in index order): deterministic, and image n's
 * scores do not depend on N.  H, W >= 11 (else GSR_EINVAL), C >= 1.  scratch: device memory of gsr_image_scores_scratch_bytes()
 * (0 for invalid dimensions), no initialisation needed, not shared between concurrent calls.
 */
size_t gsr_image_scores_scratch_bytes(int64_t N, int C, int H, int W);
int gsr_image_scores(const float *gt, const float *pred, int64_t N, int C, int H, int W, float *ssim, float *mse, void *scratch,
                     void *stream);

/*
 * One pose step of test_step_align (src/model/model_wrapper_style.py:430-440) for n views, one launch:
 *   Adam (torch.optim.Adam: beta1, beta2, eps, bias correction by `step` >= 1, two learning rates as its two parameter groups) on the
 *   deltas (rot, trans), which are zero before every step; then c2w <- (SE3_exp(trans, rot) c2w^-1)^-1 (src/misc/cam_utils.py:67-137,
 *   including the angle < 1e-5 series), the pose arithmetic in fp64.
 *   c2w (n,4,4) in/out; m, v (n,6) Adam moments, (rot xyz, trans xyz) per view, zeroed by the caller before step 1;
 *   grad_rot, grad_trans (n,3) dL/d(cam_rot_delta), dL/d(cam_trans_delta).  All device fp32, contiguous.
 */
int gsr_pose_adam_update(float *c2w, float *m, float *v, const float *grad_rot, const float *grad_trans, int64_t n, int step,
                         float lr_rot, float lr_trans, float beta1, float beta2, float eps, void *stream);

/*
 * Initial relative pose from predicted geometry, `get_pnp_pose` (src/misc/cam_utils.py:158-178) without the host round trip through
 * cv2.solvePnPRansac: P independent problems in one call, all on `stream`, no host synchronisation, no float atomics; a problem's
 * outputs are bit-identical whether it is solved alone or in a batch.  The contract is the geometry, not OpenCV's random stream.
 *   pts3d (P,N,3), opacity (P,N): device fp32, N = H*W in row-major pixel order; point i is observed at pixel
 *     (x, y) = (i % W + pixel_offset, i / W + pixel_offset)  (pixel_offset 0 = the reference's np.mgrid grid);
 *   K (P,3,3): device fp32 pixel-unit intrinsics (fx, skew, cx / 0, fy, cy / 0, 0, 1); points with opacity > opacity_threshold take part;
 *   `iterations` (1..4096) six-point hypotheses drawn with a counter-based generator keyed by (seed, hypothesis, draw), each
 *   scored against every masked point (inlier: in front of the camera, reprojection distance <= reprojection_error pixels, integer
 *   counts, ties to the lowest index), then a fixed number of Levenberg-Marquardt steps on the points within the bound.
 *   c2w (P,4,4) fp32: inverse of the estimated world->camera; inlier_mask (P,N) uint8 or NULL: the points within the bound under it;
 *   status (P,4) int32: masked points, inliers, index of the winning hypothesis (-1: none), code (0 ok, 1 fewer than 6 masked points,
 *   2 no valid hypothesis).  A non-zero code leaves c2w = identity and an empty mask; it is never a fault.
 *   scratch: device memory of gsr_pnp_ransac_scratch_bytes() (0 for invalid dimensions), no initialisation needed.
 * GSR_EINVAL before any launch for null pointers, N != H*W, P < 1 or > 65535, iterations out of range, reprojection_error <= 0.
 */
size_t gsr_pnp_ransac_scratch_bytes(int64_t P, int H, int W, int iterations);
int gsr_pnp_ransac(const float *pts3d, const float *opacity, const float *K, int64_t P, int H, int W, int64_t N, float opacity_threshold,
                   float reprojection_error, int iterations, uint64_t seed, float pixel_offset, float *c2w, uint8_t *inlier_mask,
                   int32_t *status, void *scratch, void *stream);

/*
 * The structure term of `ssim(X, Y, data_range=1, win_size=11, retrun_seprate=True)` (src/loss/loss_ssim.py:80-124) that the pose
 * refinement adds to its objective (src/evaluation/pose_evaluator.py:128-133), for (N,C,H,W) device fp32 images, contiguous, H, W >= 11:
 *   valid 11 x 11 filter with the 11 `window` taps (HOST pointer: _fspecial_gauss_1d(11, 1.5) as the caller's framework rounds it),
 *   compensation 1, sigma^2 clamped below at finfo(float32).eps^2, |sigma12| capped at sqrt(sigma1^2 sigma2^2), C3 = C2 / 2,
 *   structure_map = (sigma12 + C3) / (sigma1 sigma2 + C3) clamped above at 0.98;
 *   structure[n] = mean over the (H-10) x (W-10) pixels and the C channels of image n (the reference's scalar is their mean over n).
 * fwd: two launches (the pass + an ordered fold of per-tile float64 partials): deterministic, image n's value does not depend on N.
 *   maps: NULL, or device fp32 [3][N*C*(H-10)*(W-10)] that receives the per-pixel adjoints d/d mu2, d/d E[y^2], d/d E[xy] (zero where
 *   the 0.98 clamp is active) for the backward.  scratch: gsr_ssim_structure_scratch_bytes() of device memory, uninitialised.
 * bwd: grad_pred[n] = grad_structure[n] * d structure[n] / d pred[n] -- the transposed filter of the three maps combined with the pixel's
 *   own target / pred value; one launch, every element of grad_pred is written.  grad_structure: device fp32 [N].
 */
size_t gsr_ssim_structure_scratch_bytes(int64_t N, int C, int H, int W);
int gsr_ssim_structure_fwd(const float *target, const float *pred, int64_t N, int C, int H, int W, const float *window, float *structure,
                           float *maps, void *scratch, void *stream);
int gsr_ssim_structure_bwd(const float *target, const float *pred, const float *maps, const float *grad_structure, int64_t N, int C, int H,
                           int W, const float *window, float *grad_pred, void *stream);

/*
 * Point-map distillation (csrc/gsr_points.hip): the frozen DUSt3R / MASt3R teacher's head post-processing and the Regr3D loss
 * (src/loss/loss_point.py:188-254) of the student's means against the teacher's point maps.  Device fp32, nothing syncs with the host,
 * no float atomics, a launch sequence that depends on (B, N, mode) only; two runs give the same bits.
 *
 * pointmap_post: raw (P,4,H,W) head output -> pts3d (P,H,W,3) = xyz / max(|xyz|, 1e-8) * expm1(|xyz|), conf (P,H,W) = 1 + exp(raw[3]).
 *
 * regr3d_fwd: gt1, gt2 (B,N,3) and conf1, conf2 (B,N) contiguous; pr1, pr2 (B,N,3) with the (N,3) block of an image contiguous and
 *   their own batch stride in floats (>= 3 N: the caller hands in means[:, 0] and means[:, 1] of a (b,v,h,w,1,3) tensor uncopied).
 *     dis = |gt| per point; per (view, image) the 0.2 % and 99.8 % quantiles of dis exactly as torch.quantile's linear interpolation
 *     (rank float32(q) * float32(N - 1), torch's lerp), found by radix selection, not by a sort; a NaN in a map makes both NaN;
 *     valid = qlo <= dis <= qhi and conf >= 3;  with dist_clip > 0 instead: valid = dis <= dist_clip (no quantiles, no confidence gate);
 *     norm = 1 ('avg_dis'): per image, jointly over both views, s = sum_valid |p| / (nnz1 + nnz2 + 1e-8), clipped below at 1e-8; the
 *       prediction is divided by its s (with gradient), the teacher points by theirs; norm = 0: no normalisation;
 *     loss = mean over view 1's valid points (all images together) of |pr1 - gt1| + the same for view 2; disable_view1 drops the first.
 *   Deviation from the reference: a view without any valid point contributes 0 with a zero gradient (the reference returns NaN, the mean
 *   of an empty tensor); status reports it.
 *   status (2,B,2) int32: [view][image] = valid count, GSR_PT_* bits.  quantiles: NULL or (2,B,2) fp32 (zeros under dist_clip).
 *   valid: NULL or (2,B,N) uint8.  scratch: regr3d_scratch_bytes(B, N) of device memory, uninitialised; the backward reads what the
 *   forward left in it.
 * regr3d_bwd: grad_pr1, grad_pr2 (B,N,3) contiguous = grad_loss[0] * d loss / d pr; every element is written (0 off the valid set and
 *   where pr == gt); under norm = 1 the term through s is included.
 * GSR_EINVAL before any launch: null pointers, B < 1, N < 2, a batch stride below 3 N, norm outside {0, 1}.
 */
#define GSR_PT_EMPTY_MAP 1    /* this (view, image) has no valid point */
#define GSR_PT_NAN 2          /* |gt| of this map holds a NaN: NaN quantiles, nothing valid */
#define GSR_PT_EMPTY_VIEW 4   /* the whole view has no valid point: its term is 0 */
int gsr_pointmap_post(const float *raw, int64_t P, int H, int W, float *pts3d, float *conf, void *stream);
size_t gsr_regr3d_scratch_bytes(int B, int64_t N);
int gsr_regr3d_fwd(const float *gt1, const float *gt2, const float *conf1, const float *conf2, const float *pr1, const float *pr2,
                   int64_t pr1_batch_stride, int64_t pr2_batch_stride, int B, int64_t N, int norm, int disable_view1, float dist_clip,
                   void *scratch, float *loss, int32_t *status, float *quantiles, uint8_t *valid, void *stream);
int gsr_regr3d_bwd(const float *gt1, const float *gt2, const float *pr1, const float *pr2, int64_t pr1_batch_stride,
                   int64_t pr2_batch_stride, int B, int64_t N, int norm, int disable_view1, const float *grad_loss, const void *scratch,
                   float *grad_pr1, float *grad_pr2, void *stream);

/*
 * Scene outputs (csrc/gsr_outputs.hip): the cameras of a fly-through video, the video as bytes and the vertex table of a .ply export
 * (src/visualization/camera_trajectory/{interpolation,wobble}.py, src/misc/utils.py::vis_depth_map, src/visualization/layout.py,
 * src/model/ply_export.py).  Device pointers only, nothing syncs with the host, no float atomics, two runs give the same bits.
 * scratch: gsr_outputs_scratch_bytes() of device memory, uninitialised, for depth_range and ply_normalizer.
 *
 * trajectory: P endpoint pairs c2w_a, c2w_b (P,4,4), K_a, K_b (P,3,3), t (F) -> c2w (P,F,4,4), K (P,F,3,3).
 *     tm = t * t_scale + t_shift, formed in fp32 (the exaggerated video's t * 5 - 2; outside [0, 1] is legal).
 *     c2w = interpolate_extrinsics(A, B, tm, eps): look vectors a, b = third columns, parallel iff ||a.b| - 1| < eps; pivot = midpoint of
 *       the origins if parallel, else the least-squares intersection of the look rays; pivot frame [y x z, y, z] with z = a,
 *       y = normalize(a x b') and b' = b, replaced by (0,0,1) and then (0,1,0) while parallel to a; per endpoint 3 translations in
 *       [y x look, y, look] and the Y and Z angles of the intrinsic "YXZ" Euler decomposition of frame^T R (X dropped; at gimbal lock the
 *       third angle is 0); translations linear, angles by interpolate_circular (mod 2 pi, shorter way, the reference's tie rules);
 *       back through pivot_parameters_to_extrinsics.  float64 throughout, ONE rounding to fp32 (the reference rounds before the last step).
 *     K = K_a + (K_b - K_a) * tm in fp32, bit-identical to interpolate_intrinsics.
 *     hold_a: pose and intrinsics of A for every frame.
 *     wobble_factor != 0: c2w is right-multiplied by the transform with tf[0,3] = sin(2 pi n t) r, tf[1,3] = -cos(2 pi n t) r on the
 *       UNMAPPED t, n = wobble_rotations, r = wobble_factor * (wobble_radius ? wobble_radius[p] : |o_a - o_b|), times t if
 *       wobble_scale_with_t.  wobble_radius: NULL or device fp32 [P].
 *   Finite orthonormal inputs never give a NaN.
 *
 * depth_range: over the first min(n, max_elems) depths in flat order, range[1] = far = log(q_0.99 of all), range[0] = near =
 *     log(q_0.01 of the positive ones), both with torch.quantile's linear interpolation (radix selection, no sort), the logarithm
 *     correctly rounded; range[2], range[3] = the two quantiles themselves.  status[0] = count of positive depths, status[1] =
 *     GSR_DEPTH_NO_POSITIVE if there is none, and then near = 0 (the reference's except branch).  A NaN depth makes far NaN.
 *   Deviation from the reference: the positive set is "the positives among the first max_elems elements", the reference's is "the first
 *   max_elems positives"; the two differ only above max_elems (16 000 000 there) depths.
 *
 * pack_frames: n_panels <= 4 panels of F frames, each planar RGB (F,3,H,W) or, where is_depth[i] != 0, a depth (F,H,W), device fp32,
 *     contiguous; `panels` and `is_depth` are HOST arrays.  out: uint8 (F', H_out, W_out, 3), pixel-interleaved.  Panels follow each other
 *     along axis (0: rows, vcat; 1: columns, hcat) with `gap` pixels of value 255 between them; loop_reverse appends frames F-2 .. 1,
 *     F' = F + max(F - 2, 0).  RGB byte = uint8(clip(x, 0, 1) * 255), truncating, the product in fp32 (NaN -> 0).  Depth:
 *     x = 1 - (log d - near) / (far - near) with range = (near, far) on the device; NaN -> black, else turbo[min(int(clip(x,0,1) * 256), 255)]
 *     (matplotlib's 256 nodes as bytes, csrc/gsr_turbo_lut.h).  One streaming launch; a lane writes 4 pixels as 3 dwords.
 *
 * ply_normalizer: export_ply(shift_and_scale=True): out[0..2] = torch.median's lower median of means (G,3) per axis, out[3] = max over
 *     axes of the 95 % quantile of |means - median|; G >= 2.
 * ply_rows: rows (G, 17 + n_rest) fp32 in construct_list_of_attributes order: x y z, nx ny nz (0), f_dc_0..2, f_rest_* (unless
 *     dc_only; n_rest = 3 (d_sh - 1), index c (d_sh - 1) + k - 1 for harmonics[g][c][k]), opacity (raw), scale_0..2 = log(scales),
 *     rot_0..3 = (w,x,y,z) of scipy's from_quat(xyzw).as_matrix() -> from_matrix().as_quat() round trip in float64, rounded once.
 *     normalizer: NULL, or the 4 floats of ply_normalizer: then (means - median) / factor and log(scales / factor).
 * GSR_EINVAL before any launch: null pointers, P, F, n, G, H, W, d_sh < 1 (ply_normalizer: G < 2), n_panels outside 1..4, axis outside
 * {0, 1}, gap < 0, eps <= 0, a depth panel without range.
 */
#define GSR_DEPTH_NO_POSITIVE 1
int gsr_trajectory(const float *c2w_a, const float *c2w_b, const float *K_a, const float *K_b, const float *t, int P, int F, float t_scale,
                   float t_shift, float eps, int hold_a, float wobble_factor, int wobble_rotations, int wobble_scale_with_t,
                   const float *wobble_radius, float *c2w, float *K, void *stream);
size_t gsr_outputs_scratch_bytes(void);
int gsr_depth_range(const float *depth, int64_t n, int64_t max_elems, void *scratch, float *range, int32_t *status, void *stream);
int gsr_pack_frames(const float *const *panels, const int32_t *is_depth, int n_panels, int F, int H, int W, int axis, int gap,
                    int loop_reverse, const float *range, uint8_t *out, void *stream);
int gsr_ply_normalizer(const float *means, int64_t G, void *scratch, float *out, void *stream);
int gsr_ply_rows(const float *means, const float *scales, const float *rotations, const float *harmonics, const float *opacities, int64_t G,
                 int d_sh, int dc_only, const float *normalizer, float *rows, void *stream);

/*
 * Scene inputs (csrc/gsr_inputs.hip): decoded frames -> the planar fp32 images of a batch, bit-equal to the reference's per-image
 * host path (src/dataset/shims/crop_shim.py::rescale -- uint8, PIL's 8-bit Lanczos resize, / 255 -- then center_crop, after the
 * flip of augmentation_shim.py::reflect_views).
 *
 * resample_plan (HOST ONLY, no device call): the plan of one axis, n input samples -> m output samples, in float64 with libm's sin.
 *     *ksize = 2 ceil(3 max(n / m, 1)) + 1 is always written; bounds and coeffs are both NULL (size query) or both given:
 *     bounds (m,2) int32 = (first tap, tap count), coeffs (m,ksize) int32 = the normalised Lanczos-3 weights in 22-bit fixed point,
 *     zero behind the count.  A "device plan" below is these two arrays in one buffer, bounds first: m * (2 + ksize) int32.
 * resample_crop: N source images of H x W -- uint8 (N,H,W,3) interleaved, or fp32 (N,3,H,W) planar when src_is_f32 (quantised as
 *     uint8(clip(x * 255, 0, 255)), fp32 product, truncating cast, NaN -> 0) -- are scaled to scaled_h x scaled_w and the window
 *     (top, left, out_h, out_w) of the scaled image is written as fp32 (N,3,out_h,out_w) = byte / 255.
 *     plan_x / plan_y: device plans of (W -> scaled_w) / (H -> scaled_h); NULL exactly when that size does not change (the axis is
 *     then not filtered).  Horizontal pass first, bytes between the passes.  flip: NULL or (N) int32 on the device; image n is read
 *     mirrored along x (at the source, before the filter) where flip[n] != 0.  Only the window's columns and the rows its vertical
 *     taps touch are computed.  scratch: resample_scratch_bytes() of device memory (4-byte aligned, uninitialised; 0 for invalid
 *     dimensions).  flags: 0, or GSR_RESAMPLE_DIRECT (tests: the horizontal pass reads global memory tap by tap, as it does by itself
 *     when a block's source segment does not fit its LDS; same bytes).  Two launches, no host sync, no atomics.
 * GSR_EINVAL before any launch: null src / scratch / out, N < 1 or > 21845, a size < 1 or > 2^24, a window outside the scaled image,
 * a plan that is NULL although the size changes (or given although it does not), unknown flags; GSR_ENOSPACE: scratch too small.
 */
#define GSR_RESAMPLE_DIRECT 1
int gsr_resample_plan(int n, int m, int32_t *ksize, int32_t *bounds, int32_t *coeffs);
size_t gsr_resample_scratch_bytes(int64_t N, int H, int W, int scaled_h, int scaled_w, int top, int left, int out_h, int out_w);
int gsr_resample_crop(const void *src, int src_is_f32, int64_t N, int H, int W, const int32_t *plan_x, int scaled_w, const int32_t *plan_y,
                      int scaled_h, int top, int left, int out_h, int out_w, const int32_t *flip, void *scratch, size_t scratch_bytes,
                      float *out, int flags, void *stream);

/*
 * View selection (csrc/gsr_views.hip): the mutual overlap of view pairs, as the reference's evaluation-index generator computes it
 * (src/evaluation/evaluation_index_generator.py: get_world_rays of sample_image_grid, then src/geometry/epipolar_lines.py::project_rays
 * with near = far = None, epsilon 1e-6).  counts[p][0] is the number of the H * W pixel rays of view pairs[p][0] whose projected
 * segment overlaps the image of view pairs[p][1]; counts[p][1] is the same with the two views swapped.  float32(count) / float32(H * W)
 * is the reference's overlaps_image.float().mean() bit for bit.
 *     extrinsics (V,4,4) camera-to-world and intrinsics (V,3,3) normalised, fp32 on the device, widened to float64; both inverses
 *     (3 x 3, general 4 x 4) are formed on the device in float64 by a prologue launch that also re-arms the counters.  Pixel
 *     coordinates are (idx + 0.5) / length in fp32, widened; everything after them is float64 without contraction.
 *     pairs (P,2) int32 and counts (P,2) int32 on the device.  A pair that names a view outside [0, V) gets -1 in both slots and no
 *     camera is read for it.  Singular cameras give what IEEE arithmetic gives.
 *     scratch: the scratch_bytes query's size in device memory (8-byte aligned, uninitialised; the query answers 0 for invalid V / P).
 *     Two launches, no host sync, integer atomics only: two runs give the same counts.
 * GSR_EINVAL before any launch: null pointers, V < 1, P < 1 or > 2^22, H or W < 1, H * W > 2^24 (the bound that keeps the fp32 mean
 * exact); GSR_ENOSPACE: scratch too small.
 */
size_t gsr_view_overlap_scratch_bytes(int V, int64_t P);
int gsr_view_overlap(const float *extrinsics, const float *intrinsics, int V, const int32_t *pairs, int64_t P, int H, int W, void *scratch,
                     size_t scratch_bytes, int32_t *counts, void *stream);

/*
 * Multi-view consistency of rendered colour sets over ONE geometry (csrc/gsr_consistency.hip): view pairs[p][0] (src, i) is warped onto
 * view pairs[p][1] (dst, j) through dst's depth map and the exact cameras -- a geometric warp, no optical flow -- and compared with dst
 * where the point is visible in both.
 *     images (S,V,3,H,W) fp32 planar in [0,1]; depth (V,H,W) fp32, camera-space z in the units of the cameras' translations;
 *     c2w (V,4,4) and K (V,3,3) FLOAT64 on the device: camera-to-world with an orthonormal rotation (world -> camera is R^T (X - t), no
 *     inverse is formed) and normalised intrinsics of which only fx, fy, cx, cy are read; pairs (P,2) int32.
 * Per dst pixel (x, y), in float64 without contraction, in the order of metrics.warp_consistency_expression:
 *     d = depth[j,y,x] finite and > 0;  u = (x + 0.5) / W, v = (y + 0.5) / H;  Xc = ((u - cx_j) / fx_j * d, (v - cy_j) / fy_j * d, d);
 *     Xw = R_j Xc + t_j;  Xi = R_i^T (Xw - t_i), z = Xi.z > 0;  px = (fx_i Xi.x / z + cx_i) W - 0.5 in [0, W - 1], py likewise;
 *     x0 = min(floor(px), W - 2), ax = px - x0 (y likewise): four taps with weights (1-ax)(1-ay), ax(1-ay), (1-ax)ay, ax ay, summed in
 *     that order;  D = the taps of depth[i], each finite and > 0;  visible: |z - D| <= depth_tol * D.
 *     Per set s and channel c the taps of images[s,i,c] are summed in float64 and rounded once to fp32: warped[s,p,c,y,x] (0 at invalid
 *     pixels; warped may be NULL).  The squared difference of that fp32 value and images[s,j,c,y,x], summed over c in float64, goes to
 *     sse[s,p] (float64 (S,P)); mask[p,y,x] (uint8) is 1 at valid pixels and count[p] (int32) is their number.
 * A pair that names a view outside [0, V) has no valid pixel (mask 0, count 0, sse 0) and no camera or image is read for it.
 * Two launches: one lane per dst pixel in tiles of GSR_CONSISTENCY_TILE_W x GSR_CONSISTENCY_TILE_H, one record (count + S float64 sums)
 * per workgroup, then a one-workgroup fold of the records in a fixed order.  No atomics, bit-identical from run to run; every element
 * of every output is written on every call.  scratch: the scratch_bytes query's size in device memory, 8-byte aligned, no
 * initialisation, not shared between concurrent calls (the query answers 0 for dimensions the entry refuses).
 * GSR_EINVAL before any launch: S < 1 or > GSR_CONSISTENCY_MAX_SETS (callers with more sets call in chunks: the geometry is cheap next
 * to the colour reads), V < 1, P < 1 or > 2^24, H or W < 2 or > 16384, more than 2^31 - 1 tiles, depth_tol negative or NaN, NULL
 * images / depth / c2w / K / pairs / mask / count / sse / scratch, scratch not 8-byte aligned.  GSR_ENOSPACE: scratch too small.
 */
#define GSR_CONSISTENCY_MAX_SETS 8
#define GSR_CONSISTENCY_TILE_W 32
#define GSR_CONSISTENCY_TILE_H 8
size_t gsr_warp_consistency_scratch_bytes(int64_t P, int S, int H, int W);
int gsr_warp_consistency(const float *images, const float *depth, const double *c2w, const double *K, const int32_t *pairs, int S, int V,
                         int64_t P, int H, int W, double depth_tol, float *warped, uint8_t *mask, int32_t *count, double *sse, void *scratch,
                         size_t scratch_bytes, void *stream);

/*
 * Lens undistortion of 8-bit frames (csrc/gsr_undistort.hip; the reference's COLMAP drivers: initUndistortRectifyMap + remap with
 * INTER_LINEAR and a zero border + the crop to the valid-pixel ROI, per image on the host).  src (N,H,W,3) and dst (N,roi_h,roi_w,3)
 * are interleaved bytes on the device, dst 4-byte aligned.  Frame n belongs to camera frame_cam[n]; frame_cam is an int32 (N) array
 * on the HOST: it is checked here and handed to the kernel in its argument block.  cams is a device table of n_cams rows of
 * GSR_UNDISTORT_CAM_DOUBLES float64, 8-byte aligned:
 *       [0..3] fx fy cx cy of the distorted camera   [4..7] k1 k2 p1 p2   [8..11] fx' fy' cx' cy' of the undistorted camera
 *       [12,13] x, y of the ROI origin in the full undistorted frame (integers)   [14] 0: no distortion, the frame is copied through its
 *       window; otherwise remap   [15] reserved, 0
 * Output pixel (u, v) is pixel (u + x, v + y) of the full W x H undistorted frame.  Its source coordinate is evaluated in float64
 * without contraction -- x = (u - cx') / fx', y = (v - cy') / fy', r2 = x x + y y, kr = 1 + (k2 r2 + k1) r2,
 * xd = x kr + p1 (2 x y) + p2 (r2 + 2 x x), yd = y kr + p1 (r2 + 2 y y) + p2 (2 x y), mx = float32(fx xd + cx), my = float32(fy yd + cy)
 * -- and sampled in 1/32-pixel fixed point: sx = rint(mx * 32) half to even, ix = sx >> 5, a = sx & 31 (iy, b likewise),
 * byte = ((32 - a)(32 - b) p00 + a (32 - b) p01 + (32 - a) b p10 + a b p11 + 512) >> 10 with 0 for a tap outside the image; a non-finite
 * coordinate or one with |m| * 32 >= 2^30 gives 0.  The table's values are the caller's: every source read is bounds-checked whatever
 * they are.  One launch per GSR_UNDISTORT_FRAMES_PER_LAUNCH frames, no map arrays, no scratch, no atomics, no host sync.
 * GSR_EINVAL before any launch: null pointers, misaligned cams / dst, N < 1 or > 2^24, H or W < 1 or > 32767, n_cams < 1 or > 65535,
 * a frame_cam entry outside [0, n_cams), roi_w or roi_h < 1 (an empty ROI) or > 32767.
 */
#define GSR_UNDISTORT_CAM_DOUBLES 16
#define GSR_UNDISTORT_FRAMES_PER_LAUNCH 1024
int gsr_undistort(const uint8_t *src, int64_t N, int H, int W, const double *cams, int n_cams, const int32_t *frame_cam, int roi_w,
                  int roi_h, uint8_t *dst, void *stream);

/*
 * JPEG frames (csrc/gsr_jpeg_entropy.h on the host, csrc/gsr_jpeg.hip on the device; the reference's loader decodes one frame at a
 * time with PIL, src/dataset/dataset_re10k_style.py::convert_images).  The Huffman stage is serial per image and stays on the host; the
 * rest -- dequantisation, the "islow" integer IDCT, fancy chroma upsampling, YCbCr -> RGB -- is integer arithmetic per pixel and runs
 * on the device.  The bytes are those of libjpeg-turbo (JDCT_ISLOW, fancy upsampling), bit for bit.
 *
 * Fast path: SOF0 / SOF1, 8-bit samples, Huffman coding, ONE interleaved scan; one component, or three (YCbCr: a JFIF marker, or no
 * Adobe marker, or Adobe transform 1) with luma sampled 1x1, 2x1 or 2x2 and chroma 1x1; any restart interval, any Huffman tables.
 * A valid stream outside it (progressive, arithmetic, 12-bit, CMYK / YCCK, RGB, 4:4:0, 4:1:1, several scans, 16-bit tables in SOF0) is
 * GSR_JPEG_UNSUPPORTED, and so is an image one of whose dequantised 8 x 8 blocks fails the coefficient gate: the sum of |coef * q|
 * over a column above GSR_JPEG_MAX_COLUMN_L1, or over the block above GSR_JPEG_MAX_BLOCK_L1 (inside the gate neither
 * the kernel's 32-bit arithmetic nor the 16-bit lanes of the reference's SIMD code can overflow; uniform noise encoded at quality
 * 100 reaches about a third of the column bound and a quarter of the block bound).  A truncated or invalid stream is GSR_JPEG_CORRUPT.  The stream is untrusted: no read
 * outside [data, data + len), no write outside the image's coefficient region, whatever the bytes say.
 *
 * jpeg_probe (HOST ONLY): the markers up to the scan header.  info->width / height / components are filled as far as a frame header
 *     was read, sampling is a GSR_JPEG_* class for GSR_OK and -1 otherwise.  Returns GSR_OK, GSR_JPEG_UNSUPPORTED, GSR_JPEG_CORRUPT,
 *     or GSR_EINVAL for a null pointer.
 * jpeg_entropy (HOST ONLY, no device call): N streams of ONE picture size H x W -> coefficient blocks.  coefs: jpeg_coef_bytes(N, H, W)
 *     bytes of host memory (pinned by the caller when a device is the target).  Image n owns desc[n].coef_count int16 values from
 *     coefs + desc[n].coef_offset, the images one behind the other (the used prefix ends at the last image's offset + count):
 *     component after component, each a grid of bw[c] x bh[c] blocks in whole MCUs, row-major, every block 64 coefficients in natural
 *     (de-zigzagged, row-major) order, zero where the stream coded none.  desc[n].quant[c] is component c's quantisation table in
 *     natural order.  status[n] is GSR_OK, GSR_JPEG_UNSUPPORTED or GSR_JPEG_CORRUPT per image (then desc[n].sampling = -1, count 0);
 *     one bad image does not fail the call.  threads is clamped to [1, 16] and to N; the images are independent.
 *     GSR_EINVAL before any work: null pointers, N < 1 or > 2^24, H or W outside [1, 65535].
 * jpeg_pixels: the device stage.  coefs_dev / desc_dev are the arrays above on the device (coefs 16-byte aligned -- every block
 *     then is --, desc 8-byte aligned); out is (N,H,W,3) interleaved bytes, 4-byte aligned: the layout gsr_resample_crop reads.  Images
 *     of one call may differ in sampling class and tables.  An image whose desc[n].sampling is negative is written as zeros.
 *     scratch: jpeg_scratch_bytes(N, H, W) of device memory, 16-byte aligned, uninitialised (the byte planes between the launches; 0 for
 *     invalid dimensions).  The descriptors are the caller's: block grids and offsets are checked against H, W and the scratch
 *     size ON THE DEVICE before they are used, and an image that fails is written as zeros.  Two launches (IDCT to byte planes;
 *     upsampling + colour), no atomics, no host sync, every output byte written exactly once.
 *       dequantise  coef * q
 *       IDCT        8 x 8 "islow": CONST_BITS 13, PASS1_BITS 2; columns first, descaled by 11 with rounding; then rows, descaled by 18
 *       range       s = v & 1023, s -= 1024 if s >= 512, byte = clamp(s + 128, 0, 255)
 *       upsample    cw = ceil(W / 2) chroma columns (ch likewise).  cw <= 2: replication.  h2v1: out[2i] = (3 in[i] + in[i-1] + 1) >> 2,
 *                   out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2, the two ends copied.  h2v2: cs = 3 row + neighbour row (above for even
 *                   output rows, below for odd ones, clamped to [0, ch - 1]); out[2i] = (3 cs[i] + cs[i-1] + 8) >> 4,
 *                   out[2i+1] = (3 cs[i] + cs[i+1] + 7) >> 4, ends (4 cs[0] + 8) >> 4 and (4 cs[cw-1] + 7) >> 4
 *       colour      cb -= 128, cr -= 128; R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 *                   G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), clamped; one component: R = G = B = Y
 *     GSR_EINVAL before any launch: null pointers, misaligned coefs / desc / scratch / out, N < 1 or > 2^24, H or W outside
 *     [1, 65535]; GSR_ENOSPACE: scratch too small.
 */
#define GSR_JPEG_UNSUPPORTED 1
#define GSR_JPEG_CORRUPT 2
#define GSR_JPEG_GRAY 0
#define GSR_JPEG_444 1
#define GSR_JPEG_422 2
#define GSR_JPEG_420 3
#define GSR_JPEG_MAX_COLUMN_L1 5888
#define GSR_JPEG_MAX_BLOCK_L1 14080
typedef struct gsr_jpeg_info {
    int32_t width, height, components, sampling, restart_interval;
} gsr_jpeg_info;
typedef struct gsr_jpeg_desc {
    int32_t sampling;      /* GSR_JPEG_GRAY / _444 / _422 / _420; negative: not decoded */
    int32_t ncomp;         /* 1 or 3 */
    int32_t bw[3], bh[3];  /* blocks per row / block rows of each component, whole MCUs */
    int64_t coef_offset;   /* int16 values from `coefs` to component 0, block 0 */
    int64_t coef_count;    /* int16 values of all components */
    uint16_t quant[3][64]; /* per component, natural order */
} gsr_jpeg_desc;
int gsr_jpeg_probe(const uint8_t *data, size_t len, gsr_jpeg_info *info);
size_t gsr_jpeg_coef_bytes(int64_t N, int H, int W);
int gsr_jpeg_entropy(const uint8_t *const *data, const size_t *len, int64_t N, int H, int W, int16_t *coefs, gsr_jpeg_desc *desc,
                     int32_t *status, int threads);
size_t gsr_jpeg_scratch_bytes(int64_t N, int H, int W);
int gsr_jpeg_pixels(const int16_t *coefs_dev, const gsr_jpeg_desc *desc_dev, int64_t N, int H, int W, void *scratch, size_t scratch_bytes,
                    uint8_t *out, void *stream);

/*
 * PNG frames (csrc/gsr_png.hip; the reference's src/misc/image_io.py saves every picture through PIL): N pictures of one size H x W with
 * C = 3 or 4 channels -> the zlib stream of each picture's IDAT chunk, on the device.  A picture is cut into chunks of whole rows, the most
 * rows whose filtered bytes rows * (1 + W * C) fit GSR_PNG_CHUNK_BYTES; one workgroup codes one chunk, all chunks of all pictures in one launch.
 *
 * png_chunks: src is GSR_PNG_SRC_U8 -- uint8 (N,H,W,C) interleaved -- or GSR_PNG_SRC_F32_PLANAR -- fp32 (N,C,H,W), converted in the load
 *     as (clip(x, 0, 1) * 255) truncated, NaN -> 0.  filter_mode 0: per row the PNG filter 0..4 with the smallest sum of min(b, 256 - b) over
 *     the filtered bytes, ties to the lowest number (the row above the first is zeros); 1: filter 0 on every row.  Tokens are byte runs
 *     only (distance 1, zlib's Z_RLE); the literal / length code is a 15-bit-limited Huffman code built as the head of gsr_png.hip states,
 *     sent with the repeat codes 16 / 17 / 18; the block is BTYPE 2, BFINAL 0, followed by an empty stored block, or -- when that is not
 *     smaller than the chunk's bytes + 5 -- one stored block.  Per chunk the scratch receives the payload, its size and the Adler-32 partial.
 * png_assemble: per picture `78 01`, the payloads, `01 00 00 FF FF`, the Adler-32 big-endian, at out + n * out_stride
 *     (out_stride >= png_stream_bound); lengths[n] = bytes of the stream (int32).  Bytes beyond the length are not written.
 * scratch: png_scratch_bytes(N, H, W, C) of device memory, 16-byte aligned, uninitialised; the same buffer for both calls.
 * png_scratch_bytes / png_stream_bound return 0 for sizes the calls refuse.  No atomics on global memory, no read-back, two launches.
 * Returns GSR_OK; GSR_PNG_ROW_TOO_WIDE when 1 + W * C > GSR_PNG_CHUNK_BYTES (nothing is launched; the caller's fallback encodes it);
 * GSR_EINVAL before any launch: null pointers, N < 1 or > 2^24, H or W < 1 or > 2^20, C not 3 or 4, an unknown src_kind / filter_mode,
 * scratch not 16-byte aligned, fp32 src or lengths not 4-byte aligned, a stream bound above 2^31 - 1, out_stride below the bound;
 * GSR_ENOSPACE: scratch_bytes too small.
 */
#define GSR_PNG_CHUNK_BYTES 16384 /* at most 65535: a chunk can always be one stored block */
#define GSR_PNG_SLOT_BYTES (GSR_PNG_CHUNK_BYTES + 8) /* scratch per chunk payload (worst case chunk + 5, rounded for word stores) */
#define GSR_PNG_SRC_U8 0
#define GSR_PNG_SRC_F32_PLANAR 1
#define GSR_PNG_ROW_TOO_WIDE 1
size_t gsr_png_scratch_bytes(int64_t N, int H, int W, int C);
size_t gsr_png_stream_bound(int H, int W, int C);
int gsr_png_chunks(const void *src, int src_kind, int64_t N, int H, int W, int C, int filter_mode, void *scratch, size_t scratch_bytes,
                   void *stream);
int gsr_png_assemble(const void *scratch, size_t scratch_bytes, int64_t N, int H, int W, int C, uint8_t *out, size_t out_stride,
                     int32_t *lengths, void *stream);

/*
 * JPEG frames out (csrc/gsr_jpeg_enc.hip; the reference saves its videos and .jpg pictures through ffmpeg / PIL): N pictures of one size
 * H x W, three channels -> the entropy-coded scan of a baseline JPEG for each, ending with the EOI marker FF D9, on the device.  The bytes
 * are libjpeg's: its integer colour conversion, box downsampling, "islow" DCT, quantisation and the Annex K Huffman tables (DESIGN.md R25
 * states every rule).  The markers in front of the scan (SOI .. SOS) are the caller's; styl3r_amd/image_io.py jpeg_header writes them.
 *
 * jpeg_enc_scans: src is GSR_JPEG_ENC_SRC_U8 -- uint8 (N,H,W,3) interleaved -- or GSR_JPEG_ENC_SRC_F32_PLANAR -- fp32 (N,3,H,W), converted in
 *     the load as (clip(x, 0, 1) * 255) truncated, NaN -> 0.  sampling is GSR_JPEG_444, GSR_JPEG_422 or GSR_JPEG_420.  quant: HOST memory,
 *     128 values 1 .. 255, the luminance then the chrominance table in natural (row-major) order; they travel as a kernel argument.
 *     The scan of picture n goes to out + n * out_stride (out_stride >= jpeg_enc_stream_bound), lengths[n] = its bytes (int32); bytes
 *     beyond the length are not written.  Four launches on `stream`, no atomics on global memory, no read-back.
 * scratch: jpeg_enc_scratch_bytes(N, H, W, sampling) of device memory, 16-byte aligned, uninitialised.  After the call it begins with the
 *     quantised coefficients, int16 (N, blocks, 64): blocks in coding order (MCU after MCU; in an MCU the Y blocks row-major, Cb, Cr),
 *     each in zig-zag order, entry 0 being the DC DIFFERENCE to the block of the same component before it.
 * jpeg_enc_scratch_bytes / jpeg_enc_stream_bound return 0 for sizes the call refuses.  The bound is the worst case of the code, 22 + 63 * 26
 * bits per block and every byte stuffed; no content or table reaches it.
 * Returns GSR_OK; GSR_JPEG_ENC_TOO_LARGE for a picture of more than 2 500 000 blocks (nothing is launched; the caller's fallback encodes
 * it); GSR_EINVAL before any launch: null pointers, N < 1 or > 2^24, H or W < 1 or > 65535, an unknown src_kind / sampling, a quantiser
 * outside 1 .. 255, scratch not 16-byte aligned, fp32 src or lengths not 4-byte aligned, out_stride below the bound or above 2^31 - 1;
 * GSR_ENOSPACE: scratch_bytes too small.
 */
#define GSR_JPEG_ENC_SRC_U8 0
#define GSR_JPEG_ENC_SRC_F32_PLANAR 1
#define GSR_JPEG_ENC_TOO_LARGE 1
size_t gsr_jpeg_enc_scratch_bytes(int64_t N, int H, int W, int sampling);
size_t gsr_jpeg_enc_stream_bound(int H, int W, int sampling);
int gsr_jpeg_enc_scans(const void *src, int src_kind, int64_t N, int H, int W, int sampling, const uint16_t *quant, void *scratch,
                       size_t scratch_bytes, uint8_t *out, size_t out_stride, int32_t *lengths, void *stream);

/*
 * gsr_draw_layers (validation visuals; the reference's src/visualization/drawing/): anti-aliased lines and points drawn over B planar
 * fp32 images (B,3,H,W) on the device, `out` = `images` for in-place.  Image b carries the ordered layers image_layers[b] ..
 * image_layers[b + 1] - 1 (int32 (B + 1,)); layer l carries the records layer_prims[l] .. layer_prims[l + 1] - 1 (int32 (NL + 1,)) and is
 * drawn with layer_msaa[l] in {0, 1} MSAA passes: one layer is one render_over_image(subdivision = 8) of the reference -- centre sample
 * per pixel, top primitive = highest covering index, RGBA (colour[top], 1) or (colour[first], 0); a pixel that differs from any of its
 * 8 neighbours inside the image is re-sampled at 8 x 8 offsets, colour = sum(c a) / (sum(a) + 1e-10), alpha = mean(a); then
 * image (1 - alpha) + colour alpha.  Layers composite in order in float64, the pixel is rounded to fp32 once.  An empty layer draws nothing.
 *     prims (NP, GSR_DRAW_RECORD_DOUBLES) float64 on the device, 16-byte aligned, pixel space:
 *       [0] kind GSR_DRAW_*   [1] colour class: lowest index WITHIN the layer of a primitive with the same colour
 *       line : [2,3] start  [4,5] end  [6,7] (end - start) / |end - start| (NaN when degenerate)  [8] |end - start| + extra
 *              [9] -extra  [10] width / 2  [11..13] RGB, with extra = width / 2 for square caps and 0 otherwise
 *       point: [2,3] centre  [8] inner radius  [10] radius  [11..13] RGB
 *     The tables are the caller's: indices outside [0, NL] / [0, NP] are clamped, never followed.  Colours must be finite.
 *     One launch, no atomics, no host sync: two runs give the same bits.  O(pixels x primitives), no primitive cap.
 * GSR_EINVAL before the launch: null pointers, B < 1 or > 65535, H or W < 1, H * W > 2^28, NP > 2^30, prims not 16-byte aligned.
 */
#define GSR_DRAW_RECORD_DOUBLES 16
#define GSR_DRAW_CHUNK 32 /* records staged through LDS at a time */
#define GSR_DRAW_BUTT 0
#define GSR_DRAW_ROUND 1
#define GSR_DRAW_SQUARE 2
#define GSR_DRAW_POINT 3
int gsr_draw_layers(const float *images, float *out, int B, int H, int W, const int32_t *image_layers, const int32_t *layer_prims,
                    const int32_t *layer_msaa, int NL, const double *prims, int64_t NP, void *stream);

/*
 * Optional per-stage timing with hipEvents recorded on the caller's stream
 * between the kernels of gsr_forward / gsr_backward (bench.py's live roofline
 * measurement).  A profile holds event pairs for `max_calls` forward and
 * `max_calls` backward calls; gsr_profile_read waits for them, returns the
 * summed milliseconds and launch counts per stage and resets the profile.
 */
#define GSR_N_STAGES 7
#define GSR_STAGE_PREPROCESS 0
#define GSR_STAGE_SCAN 1
#define GSR_STAGE_SCATTER 2
#define GSR_STAGE_SORT 3
#define GSR_STAGE_COMPOSITE_FWD 4
#define GSR_STAGE_COMPOSITE_BWD 5
#define GSR_STAGE_PREPROCESS_BWD 6
typedef struct GsrProfile GsrProfile;
GsrProfile *gsr_profile_create(int max_calls);
void gsr_profile_destroy(GsrProfile *prof);
int gsr_profile_read(GsrProfile *prof, float *ms_sum /* [GSR_N_STAGES] */, int32_t *count /* [GSR_N_STAGES] */);
/* Restrict the timing to the stages whose bit (1 << GSR_STAGE_*) is set in `stage_mask` (default: all).  Every timed stage puts two event
 * records between kernels that would otherwise follow each other back to back (~5 us per boundary); a caller that wants the duration of the
 * composite kernels INSIDE a wall-clock-timed region asks for those two only.  Stages outside the mask read back with count 0. */
int gsr_profile_set_stages(GsrProfile *prof, uint32_t stage_mask);

/* Text of the HIP error behind the calling thread's last GSR_ELAUNCH ("" if none). */
const char *gsr_last_error(void);

/* Library / build identification ("gsr-hip gfx950 <version>"). */
const char *gsr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H */
