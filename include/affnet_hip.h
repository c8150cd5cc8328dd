/*
 * affnet_hip.h - C ABI of libaffnet_hip.so: the MI355X (gfx950) implementation of the
 * ScaleSpaceAffinePatchExtractor hot path of ducha-aiki/affnet.
 *
 * The reference has no FFI: its "plugin API" for this path is Python duck typing
 * (SURVEY.md section 8b).  Each entry point below names the reference function(s) it replaces
 * (file:line relative to the reference repo).  The host-side mirror that binds these
 * symbols with ctypes is affnet_amd/_lib.py; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *  - every `d_*` pointer is a DEVICE pointer owned by the caller (torch tensors in the
 *    Python mirror); the library never allocates or frees device memory;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call only
 *    enqueues work on it and returns - no host synchronisation, no host read-back, except
 *    the explicitly named affnet_read_counts();
 *  - all functions return AFFNET_OK (0) or a negative error code; affnet_last_error(ctx)
 *    returns a human readable message for the last failure on that context;
 *  - a context is not re-entrant: one thread / one stream at a time per context (the
 *    reference object is stateful in the same way, SparseImgRepresenter.py:55); DIFFERENT contexts may be
 *    driven from different host threads / streams concurrently - the library keeps no process-global state;
 *  - a context is bound to one HIP device (affnet_ctx_create): every entry point makes that device current for
 *    the duration of the call and restores the caller's current device before returning, so a multi-GPU process
 *    does not have to hipSetDevice around library calls.  Pointers must belong to the context's device;
 *  - batching: a context created with cfg->batch = B processes B equally sized images per call.  Every
 *    per-image array then has a leading batch dimension: d_img (B,H,W); row arrays (B,cap,...) with image
 *    b's rows at b*cap (cap = affnet_capacity_prefilter / _final as documented per entry point, or the
 *    n_max argument); d_count (B).  Rows >= count[b] of image b are zero.  B = 1 is the reference's shape;
 *  - all image / LAF / descriptor arithmetic is IEEE fp32, compiled with
 *    -ffp-contract=off; fused multiply-adds are used only where the reference's CPU
 *    kernels use them ("bit-exact detector").
 */
#ifndef AFFNET_HIP_H
#define AFFNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFFNET_OK 0
#define AFFNET_ERR_INVALID (-1)   /* bad argument / unsupported configuration          */
#define AFFNET_ERR_HIP (-2)       /* a HIP runtime call failed (message has details)   */
#define AFFNET_ERR_CAPACITY (-3)  /* a fixed-capacity device list overflowed           */
#define AFFNET_ERR_EMPTY (-4)     /* no detections in any image of the call: returned by
                                   * affnet_read_counts (reference: torch.cat([]) raises,
                                   * SparseImgRepresenter.py:100)                       */

#define AFFNET_MAX_OCTAVES 16
#define AFFNET_MAX_LEVELS 8       /* n_levels + 2 <= 8                                 */
#define AFFNET_MAX_TAPS 37        /* Gaussian kernels up to 37 x 37 (nlevels = 1: 35)  */

/* Network kinds for the 32x32-patch CNNs. */
#define AFFNET_NET_AFFNET 0       /* architectures.py:204-252 AffNetFast               */
#define AFFNET_NET_ORINET 1       /* architectures.py:33-82   OriNetFast               */
#define AFFNET_NET_HARDNET 2      /* HardNet.py:61-101        HardNet                  */
#define AFFNET_NET_AFFNET_FULLCONV 3 /* architectures.py:629-674 AffNetFastFullConv: same state-dict layout as AffNetFast (the
                                      * shipped AffNet.pth loads unchanged), evaluated densely on whole images (OnePassSIR)   */

/* Arithmetic of the CNN contractions (the 3x3 conv layers conv1..conv5 of AffNetFast / OriNetFast / HardNet / AffNetFastFullConv and the
 * HardNet 8x8 head; architectures.py:204-252,33-82,629-674, HardNet.py:61-101).  Everything else - pyramid, detector, sampler, conv0, the
 * AffNet / OriNet heads, normalisations - is IEEE fp32 in both modes.
 *   FP32_MFMA   (default): v_mfma_f32_16x16x4_f32, every product and sum in fp32 (an fmaf chain in k order).
 *   FP32_SPLIT3 : every fp32 operand x is carried as x = x0 + x1 + x2 with each term rounded to bf16 (exact: 3 x 8 significand bits);
 *                 a product w * a is the six bf16 products w_i * a_j with i + j <= 2 on v_mfma_f32_16x16x32_bf16 (each exact in the
 *                 fp32 accumulator), accumulated in fp32.  Operands stay fp32 at every interface (weights, activations between layers,
 *                 outputs); the dropped terms are <= 2^-24 relative per product, i.e. this is another fp32 summation, not narrower
 *                 arithmetic (K = 8192 dot product: 2.6e-7 of sum|a||b| vs 2.1e-7 for the fmaf chain).  Results
 *                 differ from FP32_MFMA by summation order only (descriptors ~1e-6); the parity bars are the same for both modes.
 *   FP32_SPLIT2H: every fp32 operand x is carried as x ~ h + l with h = fp16(x), l = fp16(x - h) (round to nearest even both; x - h is
 *                 exact): 11 + 11 significand bits + the sign of the remainder = 23 of fp32's 24 bits, |x - h - l| <= 2^-23 |x| (rms
 *                 ~2^-24.4) for |x| >= 2^-2; the operands are NOT scaled per element, so below 2^-2 the low term fp16(x - h) is a subnormal
 *                 fp16 and the bound becomes ABSOLUTE: |x - h - l| <= 2^-25 whatever |x| (2^-22 |x| at 2^-3, 2^-17 |x| at 2^-8).  A product w * a is the THREE fp16 products w_h a_h + w_l a_h + w_h a_l on v_mfma_f32_16x16x32_f16 (each exact
 *                 in the fp32 accumulator; the dropped w_l a_l is <= 2^-24 relative), accumulated in fp32 - half the matrix instructions
 *                 of FP32_SPLIT3.  NOT bit-faithful fp32 operands like FP32_SPLIT3, but the same error class as an fp32 summation: a
 *                 K-term dot product against fp64 on the same data: 2.0e-8 rms of sum|w||a| vs 3.6e-8 for the fmaf chain of FP32_MFMA
 *                 and 2.4e-8 for FP32_SPLIT3 (the accumulation roundings dominate all three).  fp16 has a 5-bit
 *                 exponent, so the weights of a layer are packed times a power of two 2^e that puts the layer's largest |w| into
 *                 [2^13, 2^14) and the layer's sums are multiplied by 2^-e (both exact); activations are used as they are: |a| < 65504
 *                 is REQUIRED (the reference's nets are BatchNorm-ed, |a| stays below ~50; a larger value becomes inf and the output
 *                 non-finite - HardNet descriptors NaN, AffNet / OriNet outputs NaN or saturated - it does not pass as a plausible number) and an activation below 2^-2 keeps an
 *                 ABSOLUTE error of 2^-25 instead of a relative one, as stated above (subnormal fp16 operands are honoured by the MFMA,
 *                 tools/probes/f16_split_probe.hip).  Against the O(1) sums of the BatchNorm-ed layers of the shipped nets an absolute 2^-25
 *                 per activation is fp32-level; a net whose activations are UNIFORMLY small (all |a| << 2^-2) loses relative precision in
 *                 this mode - use AFFNET_ARITH_FP32_SPLIT3 (exact operands) or the default there.  Same interfaces (fp32
 *                 everywhere), same parity bars. */
#define AFFNET_ARITH_FP32_MFMA 0
#define AFFNET_ARITH_FP32_SPLIT3 1
#define AFFNET_ARITH_FP32_SPLIT2H 2

typedef struct affnet_ctx affnet_ctx;

/*
 * Static description of one extractor instance.  The host mirror fills it with the
 * reference's own formulas (ScalePyramid.__init__/forward, HandCraftedModules.py:14-56;
 * CircularGaussKernel, Utils.py:92-114) so that no Gaussian / sigma formula is baked into
 * device code (SURVEY.md section 7 "hard parts": py2-vs-py3 semantics live on the host).
 */
typedef struct affnet_config {
    int32_t height, width;                 /* input image size                                         */
    int32_t n_octaves;                     /* result of the stop rule (HandCraftedModules.py:50)       */
    int32_t levels_per_octave;             /* nLevels + 2 (5)                                          */
    int32_t oct_h[AFFNET_MAX_OCTAVES];     /* octave sizes: avg_pool2d(k=1,s=2) => ceil(h/2)           */
    int32_t oct_w[AFFNET_MAX_OCTAVES];
    float level_sigma[AFFNET_MAX_OCTAVES][AFFNET_MAX_LEVELS];  /* sigmas[o][l]  (centroid weights)    */
    float level_sigma4[AFFNET_MAX_OCTAVES][AFFNET_MAX_LEVELS]; /* float32(sigma**4) (HessianResp)     */
    double level_sigma_px[AFFNET_MAX_OCTAVES][AFFNET_MAX_LEVELS]; /* sigma*pix_dist, float64 (LAF.py:459) */
    int32_t first_blur_taps;               /* 0 = no initial blur (init_sigma <= 0.5)                  */
    float first_blur[AFFNET_MAX_TAPS * AFFNET_MAX_TAPS];       /* k x k, row-major                    */
    int32_t level_blur_taps[AFFNET_MAX_LEVELS];                /* blur producing level l (l>=1)       */
    float level_blur[AFFNET_MAX_LEVELS][AFFNET_MAX_TAPS * AFFNET_MAX_TAPS];
    /* Octave 0 only, when its blurs differ from the later octaves' (init_sigma <= 0.5: octave 0 starts at curSigma = 0.5,
     * every later octave restarts at init_sigma, HandCraftedModules.py:25-31,49).  level_blur0_taps[1] == 0: octave 0 uses
     * level_blur like every other octave (the usual case, init_sigma > 0.5). */
    int32_t level_blur0_taps[AFFNET_MAX_LEVELS];
    float level_blur0[AFFNET_MAX_LEVELS][AFFNET_MAX_TAPS * AFFNET_MAX_TAPS];
    int32_t lazy_shape_rows;               /* fused path, AffNetFast, one shape iteration: AffNet first runs on this many of the response-sorted
                                            * candidates and on the rest only if fewer than N of them survive the shape filter (device-side
                                            * decision, identical output rows).  0 = evaluate all C candidates at once like the reference,
                                            * < 0 = default (1.2 N)                                                              */
    int32_t onepass;                       /* != 0: context for the OnePassSIR path (OnePassSIR.py:14-153): the workspace also holds a
                                            * dense affine-shape map per octave + the dense net's scratch; num_prefilter must equal
                                            * num_features (no shape-filter stage) and every octave must be >= 34 px (LocalNorm2d(33)
                                            * reflect-pads by 16: the reference's scripts use border = 15)                       */
    float mr_size;                         /* mrSize (ctor kwarg, SparseImgRepresenter.py:19)          */
    float threshold;                       /* th; responses are clamp(resp - th, 0) (:77)              */
    int32_t num_features;                  /* N; <= 0: keep everything (th given => num = -1, :33-35)  */
    int32_t num_prefilter;                 /* C = int(1.5 N) if Baumberg iters > 0 else N (:192-194)   */
    int32_t max_raw_per_octave_div;        /* raw-maxima capacity of octave o = h*w / div (default 4)  */
    int32_t max_keep;                      /* capacity of the selected list when N <= 0                */
    int32_t batch;                         /* images per call, all of size height x width (<= 0: 1).
                                            * The reference is batch-size-1 (HandCraftedModules.py:283-284) and
                                            * loops in Python; here one launch covers the batch (BASELINE configs[2]). */
    int32_t baum_iters;                    /* num_Baum_iters (ctor kwarg, SparseImgRepresenter.py:22): AffNet shape iterations with
                                            * re-extraction (:127-146); <= 0: 1 when AffNet weights are passed, else none    */
    int32_t arith;                         /* AFFNET_ARITH_*: arithmetic of the CNN contractions of this context's calls (0 = exact fp32
                                            * MFMA, the default); may be changed later with affnet_set_arith                        */
} affnet_config;

/* Fills *cfg for an height x width image with the reference's own formulas, so that a caller that is not Python can create a context
 * without re-deriving them: the pyramid stop rule (minSize = 2 border + 3), octave sizes, level sigmas, the incremental blur sigmas and
 * their k x k Gaussian tap tables (k = int(6 sigma + 1) | 1, taps at linspace(-k/2, k/2, k): Python-3 true division), sigma^4 and
 * sigma x pixel distance.  Replaces ScalePyramid.__init__ / forward's bookkeeping (HandCraftedModules.py:14-56) and
 * CircularGaussKernel / GaussianBlur.calculate_weights (Utils.py:92-114,155-161).  All intermediates are doubles evaluated like the
 * numpy expressions of the reference (affnet_amd/host_plan.py is the Python mirror's restatement; a CPU test compares the two structs
 * byte for byte).  Arguments = the ScaleSpaceAffinePatchExtractor ctor kwargs (SparseImgRepresenter.py:15-24): n_levels (nlevels, 3),
 * init_sigma (1.6), border, mr_size (mrSize), threshold (th; 0 when None), num_features (N; <= 0 with a threshold),
 * num_prefilter (C = int(1.5 N) when baum_iters > 0, else N), batch (images per call), baum_iters (num_Baum_iters).
 * The remaining fields get their defaults (max_raw_per_octave_div 4, max_keep 16384, lazy_shape_rows -1, onepass 0,
 * arith AFFNET_ARITH_FP32_MFMA) and may be changed before affnet_ctx_create.
 * Returns AFFNET_ERR_INVALID for n_levels outside 1..AFFNET_MAX_LEVELS-2, more than AFFNET_MAX_OCTAVES octaves or a Gaussian of more than
 * AFFNET_MAX_TAPS taps (there is no context yet to hold a message). */
int affnet_config_fill(affnet_config* cfg, int height, int width, int n_levels, double init_sigma, int border, double mr_size,
                       double threshold, int num_features, int num_prefilter, int batch, int baum_iters);

/* ---- context ------------------------------------------------------------------------------- */

/* Creates a context bound to HIP device `device` (one context per (device, stream) user).
 * cfg == NULL creates a utility context for the stand-alone stage calls that do not touch the
 * pyramid (gauss_blur, hessian_response, laf_grid_sample, cnn32_forward, apply_rotation, scale_lafs). */
int affnet_ctx_create(affnet_ctx** out, int device, const affnet_config* cfg);
void affnet_ctx_destroy(affnet_ctx* ctx);
const char* affnet_last_error(const affnet_ctx* ctx);
/* Library / build identification, e.g. "affnet_hip 0.1 gfx950". */
const char* affnet_version(void);
/* Arithmetic mode (AFFNET_ARITH_*) of the CNN contractions launched through this context from now on (utility contexts too).  The
 * packed weight blobs serve all modes; switching back to AFFNET_ARITH_FP32_MFMA restores the default path bit for bit.  A graph
 * captured earlier (affnet_graph_capture_extract) keeps the mode it was captured with. */
int affnet_set_arith(affnet_ctx* ctx, int arith);
int affnet_get_arith(const affnet_ctx* ctx);

/* Form of the fused AffNet shape pass of affnet_describe_detected (exact fp32 arithmetic only; the split-operand modes, OnePassSIR and the
 * stand-alone affnet_cnn32_forward / _pyr calls always run the direct kernel):
 *   AFFNET_SHAPE_FORM_DIRECT   : every candidate by the direct-form trunk.
 *   AFFNET_SHAPE_FORM_WINOGRAD : (default) every candidate by a trunk with conv1 / conv3 / conv5 as Winograd F(2x2, 3x3); a margin rule then flags the
 *                                candidates whose shape-filter decision could turn on the last bits of A (about 2 %), and the direct-form trunk
 *                                recomputes exactly those, so every decision - counts, ids, responses - is the direct form's.  A of an unflagged
 *                                row differs from the direct form's by at most 4e-6 per head output.
 *   AFFNET_SHAPE_FORM_POLYPHASE: form 1 with the stride-2 layers conv2 / conv4 of that first trunk as polyphase Winograd F(2x2, 2x2) (25 instead of 36
 *                                products per 2x2 output tile, no constant but 1); the same margin rule, thresholds and re-evaluation, so every decision is
 *                                again the direct form's and A of an unflagged row stays within the same 4e-6.  Not the default: its rounding of A moves one
 *                                LAF row of the 1024 x 768 golden comparison past 1e-3 px.
 * Read when a call is enqueued; a graph captured earlier keeps the form it was captured with.  The number of re-evaluated candidates per image
 * is counter 4 of affnet_counter_offset. */
#define AFFNET_SHAPE_FORM_DIRECT 0
#define AFFNET_SHAPE_FORM_WINOGRAD 1
#define AFFNET_SHAPE_FORM_POLYPHASE 2
int affnet_set_shape_form(affnet_ctx* ctx, int form);
int affnet_get_shape_form(const affnet_ctx* ctx);

/* Form of the HardNet trunk of the fused calls (affnet_describe_detected and what is built on it; exact fp32 arithmetic only; the split-operand modes, contexts of
 * the OnePassSIR path (cfg.onepass) and the stand-alone affnet_cnn32_forward / _pyr calls always run form 0):
 *   AFFNET_DESC_FORM_DIRECT    : conv2 / conv4 (stride 2) in the direct form.
 *   AFFNET_DESC_FORM_POLYPHASE : conv2 / conv4 as polyphase Winograd F(2x2, 2x2): 25 instead of 36 products per input channel, output channel and 2x2 output
 *                                tile.  Descriptors differ from form 0 by rounding only (both within 1e-6 of a float64 forward); nothing else of a call changes.
 *   AFFNET_DESC_FORM_F43       : form 1 with conv3 (64 -> 64 at 16 x 16) as Winograd F(4x4, 3x3) instead of F(2x2, 3x3): 36 products per 16 outputs instead of 16
 *                                per 4.  Descriptors within 1e-6 of a float64 forward as well (about 3x the direct form's rounding); nothing else of a call changes.
 *   AFFNET_DESC_FORM_F43_CONV5 : form 2 with conv5 (128 -> 128 at 8 x 8) moved out of the trunk kernel: the trunk stores conv4's tensor into the 32 KB slot of the patch
 *                                and a second kernel runs conv5 as Winograd F(4x4, 3x3) for four patches per workgroup (36 instead of 64 products per 16 outputs), in place
 *                                in those slots.  One launch and one 32 KB round trip per patch more; descriptors differ by rounding only.
 *   AFFNET_DESC_FORM_F43_CONV1 : (default) form 3 with conv1 (32 -> 32 at 32 x 32) as Winograd F(4x4, 3x3) as well: conv0 and conv1 run as a pair streamed over conv1's input channels,
 *                                conv0 one block of 16 channels at a time, conv1's transformed input 8 channels at a time, so that both fit the trunk's LDS.  288 instead of
 *                                512 matrix instructions per wave in conv1; descriptors differ by rounding only (within 2e-6 of a float64 forward).
 * Read when a call is enqueued; a graph captured earlier keeps the form it was captured with. */
#define AFFNET_DESC_FORM_DIRECT 0
#define AFFNET_DESC_FORM_POLYPHASE 1
#define AFFNET_DESC_FORM_F43 2
#define AFFNET_DESC_FORM_F43_CONV5 3
#define AFFNET_DESC_FORM_F43_CONV1 4
int affnet_set_desc_form(affnet_ctx* ctx, int form);
int affnet_get_desc_form(const affnet_ctx* ctx);

/* Bytes of caller-owned device workspace the context needs (pyramid + detector lists +
 * CNN scratch).  Offsets into it are exposed so the host mirror can present the pyramid as
 * tensors (`scale_pyr`, SparseImgRepresenter.py:55). */
size_t affnet_workspace_bytes(const affnet_ctx* ctx);
/* d_workspace must be 256-byte aligned device memory of the context's device (checked with hipPointerGetAttributes). */
int affnet_bind_workspace(affnet_ctx* ctx, void* d_workspace, size_t bytes);
/* Float offset (from the workspace base) of pyramid level (o, l) of image 0; -1 if out of range. */
int64_t affnet_pyramid_level_offset(const affnet_ctx* ctx, int octave, int level);
/* Floats between the pyramids of consecutive images of the batch. */
int64_t affnet_pyramid_image_stride(const affnet_ctx* ctx);
/* Images per call (cfg->batch). */
int affnet_batch(const affnet_ctx* ctx);
/* Maximum number of rows the detector / shape stages can emit (C and N capacities). */
int affnet_capacity_prefilter(const affnet_ctx* ctx);
int affnet_capacity_final(const affnet_ctx* ctx);

/* ---- stage entry points -------------------------------------------------------------------- */

/* Gaussian blur of one image: replicate padding + full 2-D k x k cross-correlation
 * accumulated with fmaf in row-major tap order (bit-identical to the reference's conv2d on
 * CPU).  Replaces Utils.py:150-166 (GaussianBlur.forward).  `h_taps` is a HOST pointer to
 * k*k floats. */
int affnet_gauss_blur(affnet_ctx* ctx, const float* d_in, float* d_out, int h, int w,
                      const float* h_taps, int k, void* stream);

/* Whole scale pyramid into the bound workspace.  Replaces ScalePyramid.forward,
 * HandCraftedModules.py:23-56.  d_img: (H, W) fp32, 0..255. */
int affnet_pyramid_build(affnet_ctx* ctx, const float* d_img, void* stream);

/* Hessian response of one level (for the RespNet slot / tests).  Replaces
 * HessianResp.forward, HandCraftedModules.py:74-78.  sigma4 = float32(sigma**4). */
int affnet_hessian_response(affnet_ctx* ctx, const float* d_in, float* d_out, int h, int w,
                            float sigma4, void* stream);

/* Detector on the pyramid in the workspace: Hessian response, clamp(resp - th, 0), 3-D NMS,
 * border zeroing, octaveMap masking (uint8 wrap emulated), response-weighted 27-tap
 * centroid, per-level and global top-k (C = num_prefilter), x mrSize.
 * Replaces SparseImgRepresenter.py:53-111,198 + HandCraftedModules.py:208-291 +
 * Utils.py:116-148 + LAF.py:431-441.
 * Outputs (capacity affnet_capacity_prefilter rows; rows >= count are zero):
 *   d_resp (cap) fp32, d_lafs (cap,2,3) fp32 normalised LAFs (A scaled by mrSize),
 *   d_ids (cap,3) int32 = (octave, level-1 "prevBlur", flat pixel index),
 *   d_count (1) int32 number of valid rows.
 * Row order = the reference's: descending response when more than C candidates exist,
 * otherwise (octave, level, pixel) order. */
int affnet_detect(affnet_ctx* ctx, float* d_resp, float* d_lafs, int32_t* d_ids,
                  int32_t* d_count, void* stream);

/* Same detector on RESPONSE maps supplied by the caller - the RespNet slot of the reference (SparseImgRepresenter.py:24,38-41:
 * any callable RespNet(level (1,1,h,w), sigma) -> (1,1,h,w)).  d_responses is laid out like the pyramid in the workspace
 * (affnet_pyramid_level_offset - offset of level (0,0), affnet_pyramid_image_stride); clamp(r - th, 0) is applied here. */
int affnet_detect_responses(affnet_ctx* ctx, const float* d_responses, float* d_resp, float* d_lafs, int32_t* d_ids,
                            int32_t* d_count, void* stream);

/* Affine patch sampler: affine_grid + bilinear grid_sample, zeros padding,
 * align_corners=False, including the reference's fp32 coordinate round trip.
 * Replaces LAF.py:313-324,326-372 (generate_patch_grid_from_normalized_LAFs,
 * batched_grid_apply, extract_patches).  d_img (h,w) one level; d_lafs (n,2,3) normalised;
 * d_out (n, ps, ps). */
int affnet_laf_grid_sample(affnet_ctx* ctx, const float* d_img, int h, int w,
                           const float* d_lafs, int n, int ps, float* d_out, void* stream);

/* Same, gathering each patch from pyramid level d_ids[i] = (octave, level, *) of the bound
 * workspace; only rows < *d_count are written (d_count may be NULL => n_max rows).
 * Replaces LAF.py:376-404 (inverted index + per-level extraction). */
int affnet_pyr_grid_sample(affnet_ctx* ctx, const float* d_lafs, const int32_t* d_ids,
                           const int32_t* d_count, int n_max, int ps, float* d_out, void* stream);

/* ---- CNNs ---------------------------------------------------------------------------------- */

/* Number of floats of the packed (BN-folded, MFMA-ordered) weight blob of a network.  Sections, in this order: the fp32 trunk
 * (per layer [tap][cin/16][(c/4)%4][cout][c%4] + bias) and head, the three-bf16-term and two-fp16-term copies of the split
 * arithmetic modes, and LAST - HardNet only, every older offset keeps its value - the Winograd F(2x2, 3x3) weights of the
 * stride-1 layers conv1 / conv3 / conv5: U = G g G^T of the same BN-folded fp32 taps (s = g0 + g2; (g0, 0.5 (s + g1),
 * 0.5 (s - g1), g2) along x, then along y; one fp32 rounding per operation), 16 * cin * cout floats per layer as
 * [xi = 4 i + j (16)][cin/16][(c/4)%4][cout][c%4].  The exact path's Winograd loops read these; the tap copies of the same
 * layers serve the split modes and the debug paths. */
size_t affnet_cnn32_packed_floats(int net_kind);
/* Offset (in floats) of the Winograd section of trunk layer `layer` (0..5) inside the packed blob of `net_kind`; -1 when the
 * layer has none (every layer of AffNet / OriNet / FullConv, the stride-2 layers and conv0 of HardNet). */
int64_t affnet_cnn32_winograd_offset(int net_kind, int layer);
/* Packs a state dict on the HOST.  conv_w[i] (i=0..5): trunk conv weights (Cout,Cin,3,3);
 * bn_mean[i], bn_var[i]: running stats (eps 1e-5, affine=False) folded into weight+bias;
 * head_w / head_b: final conv (AffNet (3,64,8,8)+bias, OriNet (2,64,8,8)+bias,
 * HardNet (128,128,8,8), no bias, followed by BN head_bn_mean/var).
 * h_out receives affnet_cnn32_packed_floats(kind) floats; the caller uploads them.
 * Replaces the nn.Sequential definitions architectures.py:207-229,36-59, HardNet.py:67-89. */
int affnet_cnn32_pack_weights(int net_kind, const float* const* conv_w, const float* const* bn_mean,
                              const float* const* bn_var, const float* head_w, const float* head_b,
                              const float* head_bn_mean, const float* head_bn_var, float* h_out);

/* Forward of one network on n 32x32 patches (d_patches (n,32,32) fp32, raw intensities; the
 * per-patch mean / unbiased-std normalisation is fused).
 *   AffNet : d_out (n,2,2) rectified affine shape      (architectures.py:246-252, LAF.py:285-291)
 *   OriNet : d_out (n,2,2) rotation matrix             (architectures.py:76-82,  LAF.py:276-283)
 *   HardNet: d_out (n,128) L2-normalised descriptor    (HardNet.py:98-101)
 * Only rows < *d_count are computed when d_count != NULL.  d_scratch: HardNet n*(8192+512) floats (conv5 tensor = A
 * operand of the head GEMM + its split-K partials), AffNet / OriNet n*144 floats (per-wave partial sums of the head). */
int affnet_cnn32_forward(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patches,
                         const int32_t* d_count, int n_max, float* d_out, float* d_scratch, void* stream);

/* Same, but each 32x32 input patch is sampled on the fly from the pyramid in the workspace
 * (fused affnet_pyr_grid_sample + affnet_cnn32_forward; no patch tensor in HBM). */
int affnet_cnn32_forward_pyr(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_lafs,
                             const int32_t* d_ids, const int32_t* d_count, int n_max, float* d_out,
                             float* d_scratch, void* stream);

/* ---- fully-convolutional AffNet + 2-D NMS (the OnePassSIR path) ------------------------------- */

/* LocalNorm2d(33): (x - mean33) / (sqrt|E33[x^2] - mean33^2| + 1e-10) clamped to [-6, 6], reflect padding; the 33 x 33 box sums are
 * accumulated in the reference's CPU order (bit-identical sums; the normalised value agrees to 1 ulp).  Replaces
 * architectures.py:21-31.  h, w >= 17. */
int affnet_local_norm(affnet_ctx* ctx, const float* d_in, float* d_out, int h, int w, void* stream);

/* Bytes of device scratch affnet_fullconv_forward needs for an h x w image (0 if the image is too small: h, w >= 34). */
size_t affnet_fullconv_scratch_bytes(int h, int w);

/* Dense affine-shape map of one image: d_img (h, w) fp32 0..255 -> d_out (4, h, w) planar (a11, 0, a21, a22) = the rectified
 * per-pixel shape matrix.  d_packed: affnet_cnn32_pack_weights(AFFNET_NET_AFFNET_FULLCONV, ...) blob on the device.
 * Replaces AffNetFastFullConv.forward, architectures.py:666-674 (LocalNorm2d, reflect pad 14, six conv+BN+ReLU, 8x8 head,
 * bilinear upsampling, tanh, rectifyAffineTransformationUpIsUpFullyConv LAF.py:293-297). */
int affnet_fullconv_forward(affnet_ctx* ctx, const float* d_packed, const float* d_img, int h, int w, float* d_out, float* d_scratch,
                            void* stream);

/* NMS2d: out = x where x - maxpool3x3(x) + 1e-5 > 0 (and x > threshold when threshold > 1e-5), else 0.
 * Replaces HandCraftedModules.py:194-206 (as shipped its constructor raises under Python 3: `padding = kernel_size/2`). */
int affnet_nms2d(affnet_ctx* ctx, const float* d_in, float* d_out, int h, int w, float threshold, void* stream);

/* ---- hand-crafted slot fillers --------------------------------------- */

#define AFFNET_HC_ORIENTATION 0   /* HandCraftedModules.py:133-192 OrientationDetector(patch_size=19)    */
#define AFFNET_HC_BAUMBERG 1      /* HandCraftedModules.py:81-132  AffineShapeEstimator(patch_size=19)   */

/* n 19x19 patches (d_patches (n,19,19) fp32) -> d_out (n,2,2): rotation matrix [[cos,sin],[-sin,cos]] of the dominant
 * gradient orientation (kind 0; d_angles (n) optional) or the rectified Baumberg shape matrix (kind 1).
 * h_weights: HOST pointer to the 19x19 Gaussian window (kind 0: 10 * CircularGaussKernel(kernlen=19); kind 1:
 * CircularGaussKernel(kernlen=19, sigma=19/2/3), Utils.py:92-114 - computed by the host mirror). */
int affnet_handcrafted_forward(affnet_ctx* ctx, int kind, const float* d_patches, int n, const float* h_weights, float* d_out,
                               float* d_angles, void* stream);
/* Same, each patch sampled from the pyramid in the workspace (rows < d_count[image]). */
int affnet_handcrafted_forward_pyr(affnet_ctx* ctx, int kind, const float* d_lafs, const int32_t* d_ids, const int32_t* d_count,
                                   int n_max, const float* h_weights, float* d_out, void* stream);

/* ---- SIFT descriptor ------------------------------------------------- */

/* Host helper (no GPU): h_out[32 * 32] = the Gaussian window of SIFTNet(patch_size = 32), CircularGaussKernel(kernlen = 32) of
 * pytorch_sift.py:31-44 under Python 3 (halfSize = 16.0, sigma^2 = 0.9 * 256, zero where the squared distance is >= 256), evaluated in
 * double and cast to float.  AFFNET_ERR_INVALID unless patch_size == 32.  The caller uploads it once: the d_window of the calls below. */
int affnet_sift_host_window(int patch_size, float* h_out);
/* SIFTNet(patch_size = 32, num_ang_bins = 8, num_spatial_bins = 4, clipval).forward (pytorch_sift.py:69-94) on n 32x32 patches
 * (d_patches (n,32,32) fp32): centred gradients with replicate padding, magnitude x d_window, soft binning into 8 orientations,
 * 11 x 11 stride-6 pooling (getPoolingKernel, :19-25) into 4 x 4 cells, L2 norm, clamp to [0, clipval], L2 norm.
 * d_desc (n,128), index = bin * 16 + cell row * 4 + cell column.  Plain fp32 whatever the context's arithmetic mode; the summation
 * order is fixed (bit-reproducible, independent of n and of the batch). */
int affnet_sift_forward(affnet_ctx* ctx, const float* d_patches, int n, const float* d_window, float clipval, float* d_desc, void* stream);
/* Same, each patch sampled from the pyramid in the workspace along what affnet_level_select(..., ps = 32, ...) produced: normalised
 * LAFs (B,n_max,2,3) and (octave, level, *) ids (B,n_max,3), rows < d_count[image] (d_count NULL => n_max rows).  d_desc (B,n_max,128);
 * rows >= d_count[image] are zero.  Bit-identical to affnet_pyr_grid_sample(ps = 32) + affnet_sift_forward on the same frames.
 * The SIFT path without host synchronisation: affnet_extract_features(d_desc = NULL), affnet_level_select on its pixel LAFs and this
 * call, on one stream. */
int affnet_sift_forward_pyr(affnet_ctx* ctx, const float* d_lafs_norm, const int32_t* d_ids, const int32_t* d_count, int n_max,
                            const float* d_window, float clipval, float* d_desc, void* stream);

/* ---- HardTFeat descriptor -------------------------------------------- */

/* HardTFeatNet.forward in eval mode (HardNet.py:30-59): input norm (mean, unbiased std + 1e-7), conv 1 -> 32 7x7 + tanh, max-pool 2x2,
 * conv 32 -> 64 6x6 + tanh, conv 64 -> 128 8x8 + tanh, x / sqrt(sum x^2 + 1e-8).  Floats of its packed weight blob: */
size_t affnet_tfeat_packed_floats(void);
/* Host only (no GPU): the six learned tensors in the reference's shapes - features.0 (32,1,7,7) + (32), features.3 (64,32,6,6) + (64),
 * classifier.1 (128,64,8,8) + (128) - into h_out[affnet_tfeat_packed_floats()].  The element orders (csrc/weights_layout.h), among them
 * the classifier's k order, are the packer's and the kernels' contract, not the caller's. */
int affnet_tfeat_pack_weights(const float* conv1_w, const float* conv1_b, const float* conv2_w, const float* conv2_b, const float* cls_w,
                              const float* cls_b, float* h_out);
/* Floats of device scratch the two calls below need for `rows` rows in all (B * n_max for the pyramid form): conv2's output and the
 * split-K partial sums of the classifier. */
size_t affnet_tfeat_scratch_floats(int rows);
/* Descriptors of d_patches (n_max,32,32) fp32, rows < d_count[0] (d_count NULL => n_max rows); d_desc (n_max,128), rows >= the count are
 * zero.  d_packed: the uploaded blob.  Exact fp32 on the fp32 matrix cores whatever the context's arithmetic mode; every sum has a fixed
 * order (no float atomics): a row does not depend on n_max, on the other rows or on its position.  No host synchronisation. */
int affnet_tfeat_forward(affnet_ctx* ctx, const float* d_packed, const float* d_patches, const int32_t* d_count, int n_max, float* d_desc,
                         float* d_scratch, void* stream);
/* Same, each patch sampled from the pyramid in the workspace along what affnet_level_select(..., ps = 32, ...) produced: normalised
 * LAFs (B,n_max,2,3) and (octave, level, *) ids (B,n_max,3), rows < d_count[image] (d_count NULL => n_max rows).  d_desc (B,n_max,128);
 * rows >= d_count[image] are zero.  Bit-identical to affnet_pyr_grid_sample(ps = 32) + affnet_tfeat_forward on the same frames.  Exact
 * fp32 whatever the context's arithmetic mode.  The HardTFeat path without host synchronisation: affnet_extract_features(d_desc = NULL),
 * affnet_level_select on its pixel LAFs and this call, on one stream. */
int affnet_tfeat_forward_pyr(affnet_ctx* ctx, const float* d_packed, const float* d_lafs_norm, const int32_t* d_ids, const int32_t* d_count,
                             int n_max, float* d_desc, float* d_scratch, void* stream);

/* ---- LAF stages ---------------------------------------------------------------------------- */

/* base_A = A; new_LAF = [A * LAF_2x2 | centre]; keep rows with 1/6 < |l1/(l2+1e-8)| < 6 and
 * all four frame corners inside [0,1]^2; if more than N survive take the N largest
 * responses (bad rows zeroed first), else keep survivors in order.
 * Replaces SparseImgRepresenter.py:121-162 (num_Baum_iters == 1), Utils.py:168-175,
 * LAF.py:91-104.  Inputs have *d_count_in valid rows (capacity C); outputs capacity N
 * (or C when N <= 0). */
int affnet_shape_filter_select(affnet_ctx* ctx, const float* d_resp_in, const float* d_lafs_in,
                               const int32_t* d_ids_in, const float* d_A, const int32_t* d_count_in,
                               float* d_resp_out, float* d_lafs_out, int32_t* d_ids_out,
                               int32_t* d_count_out, void* stream);

/* One step of the iterated shape estimation (num_Baum_iters > 1, SparseImgRepresenter.py:127-146), rows < d_count[image] of
 * capacity affnet_capacity_prefilter(ctx):
 *   mode 0: d_lafs_out = [d_base * LAF_2x2 | centre]                                   (the frames the next patches are cut from)
 *   mode 1: d_base = d_A * d_base (in place), then d_lafs_out as above                 (d_A = the shape net's output on those patches)
 * d_A may be NULL in mode 0. */
int affnet_shape_iterate(affnet_ctx* ctx, const float* d_A, float* d_base, const float* d_lafs, const int32_t* d_count, int mode,
                         float* d_lafs_out, void* stream);

/* LAF_2x2 <- LAF_2x2 * R for rows < *d_count.  SparseImgRepresenter.py:173-177. */
int affnet_apply_rotation(affnet_ctx* ctx, float* d_lafs, const float* d_R, const int32_t* d_count,
                          int n_max, void* stream);

/* LAFs <- LAFs * [[m,m,W],[m,m,H]] (inverse=0) or / (inverse=1), m = min(H,W).
 * LAF.py:407-429 (denormalizeLAFs / normalizeLAFs). */
int affnet_scale_lafs(affnet_ctx* ctx, const float* d_in, float* d_out, const int32_t* d_count, int n_max,
                      int w, int h, int inverse, void* stream);

/* Pixel LAFs (n,2,3) -> Oxford ellipses (n,5) = x y a b c with [a b; b c] = (A A^T)^-1 through the closed-form 2x2 SVD.
 * Replaces LAF.py:35-51 (LAFs2ellT) + :106-144 (bsvd2x2).  Rows >= count are zero. */
int affnet_lafs_to_ellipses(affnet_ctx* ctx, const float* d_lafs, const int32_t* d_count, int n_max, float* d_out, void* stream);

/* The inverse: Oxford ellipses (n,5) = x y a b c -> pixel LAFs (n,2,3) with A = up-is-up rectified ([a b; b c])^-1/2.
 * Replaces LAF.py:76-89 (ells2LAFsT) + :52-74 (invSqrtTorch) + :285-291 (rectifyAffineTransformationUpIsUp), operation by
 * operation in fp32.  The centres pass through bit for bit.  Rows >= count are zero (d_count NULL => n_max rows). */
int affnet_ellipses_to_lafs(affnet_ctx* ctx, const float* d_ell, const int32_t* d_count, int n_max, float* d_lafs, void* stream);

/* Pyramid level for descriptor patches: argmin over (o,l) of |sigma[o][l]*2^o - sqrt|det A|/PS|
 * in float64, first minimum wins; also writes normalised LAFs (by pyr[0][0] size).
 * Replaces LAF.py:450-472 (host scipy cdist round trip) + SparseImgRepresenter.py:181-188.
 * d_lafs_px (n,2,3) pixel LAFs -> d_ids (n,3) (octave, level, 0), d_lafs_norm (n,2,3). */
int affnet_level_select(affnet_ctx* ctx, const float* d_lafs_px, const int32_t* d_count, int n_max,
                        int ps, int32_t* d_ids, float* d_lafs_norm, void* stream);

/* ---- descriptor matching ------------------------------------------ */

/* Bytes of device scratch affnet_match_snn / affnet_distance_matrix need for n1 x n2 descriptors. */
size_t affnet_match_scratch_bytes(int n1, int n2);

/* Full distance matrix sqrt(|a|^2 + |b|^2 - 2 a.b + 1e-6): d_out (n1, n2).  Replaces Losses.py:5-13
 * (distance_matrix_vector).  dim must be 128. */
int affnet_distance_matrix(affnet_ctx* ctx, const float* d_desc1, int n1, const float* d_desc2, int n2, int dim, float* d_out,
                           void* d_scratch, void* stream);

/* Nearest / "second nearest" neighbour ratio test exactly as train_AffNet_test_on_graffity.py:292-300 does it (the second
 * minimum runs over the columns that are nobody's nearest neighbour: dist_matrix[:, idxs_in_2] = 100000); the distance
 * matrix is never materialised.  Outputs: d_min_dist (n1), d_idx (n1), d_min2_dist (n1), d_tent (n1,2) int32 = the pairs
 * (i, idx[i]) with min/(min2+1e-8) <= snn_threshold in row order, d_count (1). */
int affnet_match_snn(affnet_ctx* ctx, const float* d_desc1, int n1, const float* d_desc2, int n2, int dim, float snn_threshold,
                     float* d_min_dist, int32_t* d_idx, float* d_min2_dist, int32_t* d_tent, int32_t* d_count, void* d_scratch,
                     void* stream);

/* Pixel LAFs (n,2,3) through the homography h_H (HOST pointer, 9 floats row-major): centre = H x / z, shape = linH(H, x) A.
 * Replaces ReprojectionStuff.py:9-40 (linH, reprojectLAFs). */
int affnet_reproject_lafs(affnet_ctx* ctx, const float* d_lafs, int n, const float* h_H, float* d_out, void* stream);

/* For every query LAF (image-1 LAFs): nearest reference LAF centre (reprojected image-2 LAFs), distance computed like
 * ReprojectionStuff.py:78-86 on the 2-D centres (sqrt(| |a|^2 + |p|^2 - 2 p.a | + 1e-12), fp32).
 * Replaces the distance / min part of ReprojectionStuff.py:126-137 (get_GT_correspondence_indexes). */
int affnet_centre_nn(affnet_ctx* ctx, const float* d_query_lafs, int nq, const float* d_ref_lafs, int nr, float* d_min_dist,
                     int32_t* d_idx, void* stream);

/* ---- spatial verification of tentative matches from their affine frames ------------------------ */

/* One tentative match of two local affine frames fixes an affine map F2 F1^-1 (spatial matching, Philbin et al. 2007): T tentatives are
 * T hypotheses, every one is scored against all T matches, the best one is refined by least-squares refits on its inliers.
 * Deterministic, bounded work, no host synchronisation; all buffers are the caller's.
 *
 * Common inputs: d_lafs1 (n1,2,3), d_lafs2 (n2,2,3) pixel frames; d_tent (t_max,2) int32 as affnet_match_snn writes it; d_count one
 * int32 on the device or NULL (= t_max rows are valid) - rows at or beyond the count are neither read nor written in any output;
 * inl_th pixels; d_scratch affnet_verify_scratch_bytes(t_max) bytes, 16-byte aligned.
 *
 * Scoring (fp32): hypothesis h = tent[h] = (i, j), M = L2 L1^-1 through det L1.  h is invalid - scores 0, is never chosen - when
 * !(|det| > 1e-12), when one of its twelve numbers is not finite or when an index is outside [0,n1) / [0,n2) (tested before any load).
 * Match t is an inlier of h when | M (c1_t - c1_h) - (c2_t - c2_h) |^2 <= inl_th^2 and t has valid indices and finite centres.
 * d_counts (t_max) int32 = inliers per hypothesis (>= 1 for a valid one: it counts itself). */
#define AFFNET_VERIFY_AFFINE 0
#define AFFNET_VERIFY_HOMOGRAPHY 1
#define AFFNET_VERIFY_TILE 128    /* hypotheses per workgroup of the scoring kernel */
#define AFFNET_VERIFY_CHUNK 128   /* matches per chunk of the scoring kernel        */

/* Host only. */
size_t affnet_verify_scratch_bytes(int t_max);

/* The scoring stage alone: d_counts, and d_best int32[2] = {smallest h with the largest count, that count}, {-1, 0} when no hypothesis
 * is valid. */
int affnet_verify_score(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent,
                        const int32_t* d_count, int t_max, float inl_th, int32_t* d_counts, int32_t* d_best, void* d_scratch,
                        void* stream);

/* Score + select + local optimisation in fp64: lo_iters (0..8) times { stop with flag 2 below 4 (homography) / 3 (affine) pairs in the
 * mask; Hartley-normalise the masked pairs; fit (homography: inhomogeneous DLT with h33 = 1, 8 x 8 normal equations; affine: 6
 * parameters), a pivot below 1e-12 x the largest diagonal entry or coincident points stop with flag 4; denormalise to H[2][2] = 1; new
 * mask = transfer error | pi(H p1) - p2 |^2 <= inl_th^2 with w > 0 }, keeping the model with the largest mask (ties: the earliest).
 * Model 0 is the affine hypothesis itself with its fp32 inlier set.
 * model: AFFNET_VERIFY_AFFINE / _HOMOGRAPHY.  Outputs: d_counts (t_max); d_model double[9] row-major; d_inlier (t_max) uint8;
 * d_summary int32[4] = {best, counts[best], final inlier count, flags}, flags 1 = no valid hypothesis (best = -1, identity model),
 * 2 = too few inliers to refit, 4 = degenerate system.  t_max == 0 is valid and gives {-1, 0, 0, 1}. */
int affnet_verify_matches(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent,
                          const int32_t* d_count, int t_max, float inl_th, int model, int lo_iters, int32_t* d_counts, double* d_model,
                          uint8_t* d_inlier, int32_t* d_summary, void* d_scratch, void* stream);

/* ---- many image pairs in one call (shortlist re-ranking: one query against K images, all pairs of a small set) ---- */

/* P pairs per call, the pair index on a grid dimension of every kernel: P x the workgroups of one pair per launch, the same number of
 * launches as for one pair.  All descriptors of side 1 lie in one (rows1,128) buffer, their frames in one (rows1,2,3) buffer; side 2 is
 * laid out the same way and may be the same buffers.  d_pairs (P,4) int32 on the device = {row1, n1, row2, n2} per pair: the pair's
 * segments are rows [row1, row1 + n1) of side 1 and [row2, row2 + n2) of side 2.  The host passes only caps (n1_max, n2_max, t_max), so
 * no grid size needs a read-back.
 *
 * Every kernel tests its table row BEFORE any load through it.  A row is out of range when a field is negative, row1 + n1 > rows1,
 * row2 + n2 > rows2, n1 > n1_max or n2 > n2_max: nothing is read or written through such a row, its count is 0 and its summary
 * {-1, 0, 0, 1 | AFFNET_VERIFY_FLAG_PAIR_RANGE} with the identity model.  n1 == 0 or n2 == 0 is a valid empty pair (count 0, summary {-1, 0, 0, 1}).
 *
 * Per row and per hypothesis the kernels run the device code of the single-pair calls (the same functions): every output of pair p is,
 * bit for bit, what affnet_match_snn / affnet_verify_matches write for that pair's segments, with indices LOCAL to the segments.
 * Outputs are pair-major with the caps as row pitch; rows at or beyond a pair's n1 / count are neither read nor written.
 * n_pairs == 0 is valid and launches nothing; n_pairs <= 65535.  No allocation, no synchronisation, all work on `stream`. */
#define AFFNET_VERIFY_FLAG_PAIR_RANGE 8   /* d_summary[3] flag 8: pair row out of range (the single-pair calls never set it) */

/* Host only.  Bytes of d_scratch of affnet_match_snn_many. */
size_t affnet_match_many_scratch_bytes(int n_pairs, int n1_max, int n2_max);

/* affnet_match_snn per pair.  d_min_dist, d_idx, d_min2_dist (P,n1_max); d_tent (P,n1_max,2); d_count (P).  dim must be 128. */
int affnet_match_snn_many(affnet_ctx* ctx, const float* d_desc1, int rows1, const float* d_desc2, int rows2, int dim, const int32_t* d_pairs,
                          int n_pairs, int n1_max, int n2_max, float snn_threshold, float* d_min_dist, int32_t* d_idx, float* d_min2_dist,
                          int32_t* d_tent, int32_t* d_count, void* d_scratch, void* stream);

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_verify_matches_many. */
size_t affnet_verify_many_scratch_bytes(int n_pairs, int t_max);

/* affnet_verify_matches per pair.  d_tent (P,t_max,2) as affnet_match_snn_many writes it with n1_max = t_max (so a row with n1 > t_max is
 * out of range here as it is there; there is no cap on n2); d_count (P) or NULL (= t_max rows are valid in every pair).
 * d_counts (P,t_max); d_model (P,9) double; d_inlier (P,t_max) uint8; d_summary (P,4). */
int affnet_verify_matches_many(affnet_ctx* ctx, const float* d_lafs1, int rows1, const float* d_lafs2, int rows2, const int32_t* d_pairs,
                               int n_pairs, const int32_t* d_tent, const int32_t* d_count, int t_max, float inl_th, int model, int lo_iters,
                               int32_t* d_counts, double* d_model, uint8_t* d_inlier, int32_t* d_summary, void* d_scratch, void* stream);

/* ---- epipolar verification of tentative matches: a fundamental matrix from affine frames ---------- */

/* The planar models above report only the inliers of the dominant plane of a scene with depth.  An affine frame is three point
 * correspondences (its centre and its two axis tips), so three tentative matches give nine - enough for the linear 8-point solve of a
 * fundamental matrix F, x2^T F x1 = 0, F row-major.  Same design as above: deterministic, bounded work, all hypotheses scored against
 * all matches, a best-first refit in fp64, no host synchronisation, all buffers the caller's.  Inputs as for affnet_verify_matches;
 * d_scratch affnet_epipolar_scratch_bytes(t_max, rounds) bytes, 16-byte aligned.  T below is the device-side row count.
 *
 * Known limit (not detected here): when most matches lie on one plane, F is one of a family - every F compatible with the plane's
 * homography explains them - and the matches off the plane decide which; the returned F is then reliable only as an inlier test.
 * affnet_epipolar_verify_planar (the section after this one) is the call for such scenes: it estimates the plane first and takes F
 * from the matches off it.
 *
 * Prep, per tentative t: indices are tested before any load.  Match t is usable (can be an inlier) when its indices are in range and
 * its two centres are finite, otherwise its points are NaN; it is usable as a MEMBER of a hypothesis when all twelve numbers of its
 * two frames are finite.  A frame [a b x; c d y] gives the points c = (x, y), c + (a, c), c + (b, d), formed in fp64 from the fp32 numbers.
 *
 * Hypotheses: h = s * rounds + r, s in [0,T), r in [0,rounds), 1 <= rounds <= AFFNET_EPI_MAX_ROUNDS.  Members m0 = s and, for k = 1, 2,
 * m_k = j with x = lowbias32((s * 0x9E3779B1) ^ (r * 0x85EBCA77) ^ (k * 0xC2B2AE3D) ^ seed) in uint32 wrap-around arithmetic,
 * lowbias32(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16;  j = ((uint64)x * T) >> 32, and while j
 * equals an earlier member j = (j + 1) % T.  A hypothesis is invalid - NaN model, count 0, never chosen - when T < 3, when a member is
 * not usable as one, when a normalisation scale is zero or not finite, when a pivot is below 1e-12 or when the final norm is zero or
 * not finite.
 *
 * Solve (fp64, no fused multiply-add, one thread per hypothesis): the nine correspondences in the order m0: centre, tip 0, tip 1; m1;
 * m2.  Per image Hartley normalisation of the nine points: centroid (sums left to right, / 9), mean distance (sum of
 * sqrt(dx*dx + dy*dy) left to right, / 9), s = sqrt(2) / mean, point -> (p - centroid) * s.  Equation row
 * [u*x, u*y, u, v*x, v*y, v, x, y, 1], (x, y) in image 1 and (u, v) in image 2; only the first eight rows are used.  Null vector by Gaussian
 * elimination with complete pivoting (largest remaining |entry|, ties to the smallest row, then the smallest column; row r below pivot
 * row k: f = A[r][k] / A[k][k], A[r][c] = A[r][c] - f * A[k][c]), the free unknown is 1, back-substitution
 * y[i] = -(A[i][8] + A[i][i+1] y[i+1] + ... + A[i][7] y[7]) / A[i][i] summed left to right, column permutation undone.
 * Denormalisation F = T2^T Fn T1 with T = [s 0 -s cx; 0 s -s cy; 0 0 1]: G[r] = (Fn[r][0] s1, Fn[r][1] s1, (Fn[r][0] (-s1 cx1) +
 * Fn[r][1] (-s1 cy1)) + Fn[r][2]), F[0] = s2 G[0], F[1] = s2 G[1], F[2] = ((-s2 cx2) G[0] + (-s2 cy2) G[1]) + G[2].  Then F / sqrt(sum of
 * squares, row-major, left to right), and the sign that makes the largest-magnitude entry (the first in row-major order on ties)
 * positive.  Stored as nine fp32 numbers.
 *
 * Score (fp32, no fused multiply-add), match centres (x, y), (u, v): l_k = (F[k][0]*x + F[k][1]*y) + F[k][2], k = 0..2;
 * m_k = (F[0][k]*u + F[1][k]*v) + F[2][k], k = 0, 1; r = (u*l_0 + v*l_1) + l_2; e = (r*r) / (((l_0*l_0 + l_1*l_1) + m_0*m_0) + m_1*m_1)
 * (the Sampson error).  Inlier iff e <= inl_th*inl_th; NaN and a zero denominator give false.  Select: the smallest h with the largest
 * count, -1 when that count is 0.
 *
 * Local optimisation (fp64): model 0 is the best hypothesis widened to double (not forced to rank 2), its mask the fp32 inlier set.
 * lo_iters (0..8) times { fewer than 8 matches in the mask: stop with flag 2; Hartley-normalise the masked centres; N = A^T A (9 x 9) of
 * the rows above; eigenvectors of N by cyclic Jacobi: exactly 12 sweeps over p < q in row-major order, a rotation skipped when
 * a_pq == 0, else theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta*theta + 1)) (sign(0) = +1),
 * c = 1 / sqrt(t*t + 1), s = t*c, columns p, q of A, then rows p, q of A, then columns p, q of V through
 * (x_p, x_q) <- (c x_p - s x_q, s x_p + c x_q); the eigenvector of the smallest diagonal entry (the first on ties); stop with flag 4
 * when the second-smallest diagonal entry is <= 1e-12 x the largest or anything is not finite; rank 2: Fn <- Fn - (Fn v) v^T with v the
 * smallest eigenvector of Fn^T Fn (same Jacobi, n = 3); denormalise, unit norm, sign as above; new mask = Sampson error in fp64, same
 * expression tree, <= inl_th^2 }, keeping the model with the largest mask (ties: the earliest). */
#define AFFNET_EPI_MAX_ROUNDS 64
#define AFFNET_EPI_TILE 128       /* hypotheses per workgroup of the scoring kernel */
#define AFFNET_EPI_CHUNK 128      /* matches per chunk of the scoring kernel        */
#define AFFNET_EPI_SOLVE_TILE 64  /* hypotheses per workgroup of the solve kernel   */

/* Host only.  Negative arguments count as 0. */
size_t affnet_epipolar_scratch_bytes(int t_max, int rounds);

/* Prep + solve + score + select.  d_hyp (t_max*rounds, 9) fp32 or NULL; d_counts (t_max*rounds) int32; d_best int32[2] = {smallest h with
 * the largest count, that count}, {-1, 0} when no hypothesis is valid.  Rows at or beyond the count and hypotheses at or beyond
 * count*rounds are neither read nor written.  AFFNET_ERR_INVALID: a NULL pointer (but d_count, d_hyp), inl_th not finite or <= 0, rounds
 * outside [1, AFFNET_EPI_MAX_ROUNDS], t_max < 0 or t_max * rounds above INT32_MAX. */
int affnet_epipolar_score(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent,
                          const int32_t* d_count, int t_max, float inl_th, int rounds, uint32_t seed, float* d_hyp, int32_t* d_counts,
                          int32_t* d_best, void* d_scratch, void* stream);

/* The above + local optimisation.  d_model double[9] row-major, unit Frobenius norm; d_inlier (t_max) uint8; d_summary int32[4] =
 * {best h, counts[best], final inlier count, flags}, flags 1 = no valid hypothesis (best = -1, model all zero), 2 = too few inliers to
 * refit, 4 = degenerate.  t_max == 0 is valid and gives {-1, 0, 0, 1}.  lo_iters outside 0..8 is AFFNET_ERR_INVALID. */
int affnet_epipolar_verify(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent,
                           const int32_t* d_count, int t_max, float inl_th, int rounds, uint32_t seed, int lo_iters, int32_t* d_counts,
                           double* d_model, uint8_t* d_inlier, int32_t* d_summary, void* d_scratch, void* stream);

/* ---- plane-aware epipolar verification: plane-and-parallax F ----
 *
 * A wall with a few things in front of it: most matches lie on one plane, and the 8-point F above is then one of a family.  With the
 * plane's homography H known, every match (x1, x2) OFF the plane gives a line l = (H x1) x x2 through the epipole e of image 2; two
 * lines give e, and F = [e]x H.  This call runs the two existing verifications, builds that model from the matches off the plane and
 * keeps whichever has more inliers.  Deterministic, bounded work, no host synchronisation, all buffers the caller's.  Inputs as for
 * affnet_epipolar_verify plus plane_th (pixels, finite and > 0); d_scratch affnet_epipolar_planar_scratch_bytes(t_max, rounds) bytes,
 * 16-byte aligned.  fp64 below is without fused multiply-add, in the written order.  T is the device-side row count.
 *
 * 1. Plane: affnet_verify_matches(model = AFFNET_VERIFY_HOMOGRAPHY, inl_th = plane_th, lo_iters) -> d_plane double[9] (H),
 *    d_plane_inlier (t_max) uint8, d_plane_summary int32[4], with the bytes of that call.
 * 2. Plain F: affnet_epipolar_verify(inl_th, rounds, seed, lo_iters) -> d_model, d_inlier, d_counts, d_summary, with the bytes of that call.
 * 3. Off-plane list: match t is off the plane when it is usable (indices in range, tested before any load, and both centres finite) and
 *    d_plane_inlier[t] == 0.  The list holds these t in ascending order; U is its length.  Stages 4 to 7 are skipped - the result is
 *    the plain one - when d_plane_summary[3] has flag 1 or U < 2.
 * 4. Parallax line (fp64) of a match with centres (x, y), (u, v): p_k = (H[k][0]*x + H[k][1]*y) + H[k][2]; l0 = p1 - p2*v,
 *    l1 = p2*u - p0, l2 = p0*v - p1*u; n = sqrt(l0*l0 + l1*l1); the line is unusable when n is zero or not finite, else l^ = l / n.
 * 5. Hypotheses: h = a * rounds + r, a in [0,U), r in [0,rounds); partner b = ((uint64)x * U) >> 32 with
 *    x = lowbias32((a * 0x9E3779B1) ^ (r * 0x85EBCA77) ^ (1 * 0xC2B2AE3D) ^ seed) (the hash above), and b = (b + 1) % U when b == a.
 *    a and b index the list.  e = l^_a x l^_b: e0 = la1*lb2 - la2*lb1, e1 = la2*lb0 - la0*lb2, e2 = la0*lb1 - la1*lb0.  F = [e]x H:
 *    F[0][c] = e1*H[2][c] - e2*H[1][c], F[1][c] = e2*H[0][c] - e0*H[2][c], F[2][c] = e0*H[1][c] - e1*H[0][c].  Then F / sqrt(sum of
 *    squares) and the sign rule, as above; stored as nine fp32.  Invalid - NaN model, count 0, never chosen - when a line is unusable
 *    or the norm is zero or not finite.  Hypotheses at or beyond U * rounds are neither read nor written.
 * 6. Score and select: the fp32 Sampson scoring above of the U * rounds hypotheses against all T matches, and the same selection.
 * 7. Refit (fp64), model 0 = the best hypothesis widened to double with its fp32 inlier set as mask; lo_iters times { S = matches in the
 *    current mask that are off the plane and have a usable line; fewer than 2: stop with flag 2; N = sum over S of l^ l^T (3 x 3);
 *    eigenvectors by the cyclic Jacobi above with n = 3; e = the eigenvector of the smallest diagonal entry (the first on ties); stop
 *    with flag 4 when the second-smallest entry is <= 1e-12 x the largest or anything is not finite; F = [e]x H, unit norm, sign (a
 *    zero or non-finite norm: flag 4); new mask = Sampson error in fp64 <= inl_th^2 over all T }, keeping the model with the largest
 *    mask (ties: the earliest).
 * 8. Decision: when the final inlier count of stage 7 is strictly larger than d_summary[2] of stage 2, d_model and d_inlier become the
 *    plane-and-parallax model and mask, and d_summary = {best h of stage 6, its count, final inlier count, flags of stage 7 |
 *    AFFNET_EPI_FLAG_PLANAR}.  Otherwise they stay affnet_epipolar_verify's bytes.  d_counts is always stage 2's.
 *
 * d_planar_info int32[4] = {U, best hypothesis of stage 6, its count, final inlier count of stage 7}; {U, -1, 0, 0} when the stages
 * did not run or no hypothesis was valid.  t_max == 0, T < 3, U in {0, 1}, a plane summary with flag 1 and a pure plane are valid
 * inputs and give the plain result.  An input of random matches only is valid too, but not special: every match is an affine
 * hypothesis that counts itself, so stage 1 reports "a plane" of one or a few matches, the stages run (two lines always meet, so a
 * hypothesis has at least its two members as inliers) and rule 8 decides - such an input may return AFFNET_EPI_FLAG_PLANAR with a
 * handful of inliers, as affnet_epipolar_verify returns a handful for it. */
#define AFFNET_EPI_FLAG_PLANAR 16   /* d_summary[3]: the result is the plane-and-parallax model */

/* Host only.  Negative arguments count as 0. */
size_t affnet_epipolar_planar_scratch_bytes(int t_max, int rounds);

/* Stages 1 and 3 to 6, for tests.  d_list (t_max) int32: the off-plane list, U entries; d_n_off int32[2] = {U, U as stages 4 to 7 use
 * it: 0 when they are skipped}; d_hyp (t_max*rounds, 9) fp32 or NULL; d_counts (t_max*rounds) int32; d_best int32[2] as in
 * affnet_epipolar_score.  List rows at or beyond U and hypotheses at or beyond U * rounds are neither read nor written.
 * AFFNET_ERR_INVALID as for affnet_epipolar_verify_planar. */
int affnet_epipolar_planar_score(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent,
                                 const int32_t* d_count, int t_max, float inl_th, float plane_th, int rounds, uint32_t seed, int lo_iters,
                                 double* d_plane, uint8_t* d_plane_inlier, int32_t* d_plane_summary, int32_t* d_list, int32_t* d_n_off,
                                 float* d_hyp, int32_t* d_counts, int32_t* d_best, void* d_scratch, void* stream);

/* All eight stages.  AFFNET_ERR_INVALID in front of the first launch: every check of affnet_epipolar_verify, plane_th not finite or
 * <= 0, a NULL d_plane, d_plane_inlier, d_plane_summary or d_planar_info. */
int affnet_epipolar_verify_planar(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const int32_t* d_tent,
                                  const int32_t* d_count, int t_max, float inl_th, float plane_th, int rounds, uint32_t seed,
                                  int lo_iters, int32_t* d_counts, double* d_model, uint8_t* d_inlier, int32_t* d_summary,
                                  double* d_plane, uint8_t* d_plane_inlier, int32_t* d_plane_summary, int32_t* d_planar_info,
                                  void* d_scratch, void* stream);

/* ---- guided matching: the descriptors searched again under a verified model ----
 *
 * affnet_match_snn refuses every match whose global second-nearest ratio is poor, also where the model that affnet_verify_matches /
 * affnet_epipolar_verify found afterwards would have made it unambiguous (repeated structure, a strong viewpoint change).  Here every
 * keypoint of image 1 is matched among the keypoints of image 2 that the model allows; the caller refits on the result.
 *
 * Inputs: d_desc1 (n1,128), d_desc2 (n2,128); d_lafs1 (n1,2,3), d_lafs2 (n2,2,3), of which the centres are read; d_model double[9]
 * row-major ON THE DEVICE (what a verification call wrote: no read-back in between); kind; radius r in px; snn_threshold thr; max_dist; flags.
 *
 * Model: m[k] = (float)d_model[k].  Everything below is fp32, one rounding per written operation (no fused multiply-add).
 *
 * Admissible pair (i, j), centres (x, y) of d_lafs1[i] and (u, v) of d_lafs2[j]:
 *   AFFNET_GUIDED_PLANAR (any 3x3 map of image 1 to image 2: the homography or the affine model of affnet_verify_matches)
 *     X = (m0*x + m1*y) + m2, Y = (m3*x + m4*y) + m5, W = (m6*x + m7*y) + m8; px = X / W, py = Y / W; dx = px - u, dy = py - v;
 *     admissible iff W > 0 && (dx*dx + dy*dy) <= r*r.
 *   AFFNET_GUIDED_EPIPOLAR (x2^T F x1 = 0: the model of affnet_epipolar_verify), the scoring tree of that call with th = r:
 *     l0 = (m0*x + m1*y) + m2, l1 = (m3*x + m4*y) + m5, l2 = (m6*x + m7*y) + m8; m0' = (m0*u + m3*v) + m6, m1' = (m1*u + m4*v) + m7;
 *     rr = (u*l0 + v*l1) + l2; e = (rr*rr) / (((l0*l0 + l1*l1) + m0'*m0') + m1'*m1'); admissible iff e <= r*r.
 *   A non-finite centre, model entry or intermediate makes the comparison false.  The per-point terms (px, py, W > 0 / l0, l1, l2 per point
 *   of image 1; m0', m1' per point of image 2) are computed once and read by every stage, so no two stages disagree about a pair.
 *
 * Distance of a pair: the element affnet_distance_matrix writes for it, bit for bit.  Order of candidates: a NaN distance in front of
 * every number, then the smaller distance, then the smaller index (affnet_knn's order).
 *   d_dist (n1,2), d_idx (n1,2): per row i the first two admissible columns in that order; an unfilled slot is (+inf, -1).
 *   With AFFNET_GUIDED_MUTUAL, back[j] = the first admissible row of column j in that order, or -1 (kept in the scratch).
 *
 * Selection, in row order: (i, idx[i][0]) is kept iff idx[i][0] >= 0 && dist[i][0] <= max_dist &&
 * dist[i][0] / (dist[i][1] + 1e-8f) <= thr (with one admissible column the ratio is 0) && (no AFFNET_GUIDED_MUTUAL || back[idx[i][0]] == i).
 * A NaN nearest distance is refused, as affnet_match_snn refuses it.  d_tent (n1,2) int32 receives the kept pairs, d_count their number;
 * rows of d_tent at or beyond the count are not written.
 *
 * Gate: d_gate, optional, is the d_summary int32[4] of a verification call.  When it is not NULL and d_gate[3] & 1 (no valid hypothesis -
 * affnet_verify_matches then leaves the identity as its model) nothing is matched: the count is 0, the lists are unfilled.
 *
 * The search runs like affnet_knn's: row blocks x n_chunks column chunks, a merge over the chunks; n_chunks = 0: the library chooses; the
 * result does not depend on it.  The backward pass is the same kernel with the sides exchanged.  One linear chain of launches on `stream`,
 * no allocation, no synchronisation.  n1 == 0 or n2 == 0 is valid and gives count 0.
 * AFFNET_ERR_INVALID in front of the first launch: dim != 128, an unknown kind or flag bit, a radius that is not finite and > 0, a NaN
 * max_dist, a negative size, n_chunks outside 0..65535, a NULL pointer other than d_gate. */
#define AFFNET_GUIDED_PLANAR 0
#define AFFNET_GUIDED_EPIPOLAR 1
#define AFFNET_GUIDED_MUTUAL 1    /* flags bit 0: keep (i, j) only if i is also the first admissible row of column j */

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_match_guided called with this n_chunks (0: enough for whatever the library
 * may choose) and of affnet_guided_mask at these sizes.  Negative arguments count as 0. */
size_t affnet_match_guided_scratch_bytes(int n1, int n2, int n_chunks);

int affnet_match_guided(affnet_ctx* ctx, const float* d_desc1, int n1, const float* d_desc2, int n2, int dim, const float* d_lafs1,
                        const float* d_lafs2, const double* d_model, int kind, float radius, float snn_threshold, float max_dist, int flags,
                        int n_chunks, const int32_t* d_gate, float* d_dist, int32_t* d_idx, int32_t* d_tent, int32_t* d_count,
                        void* d_scratch, void* stream);

/* d_mask (n1,n2) uint8: 1 where the pair is admissible by the rule above - the very function affnet_match_guided applies.  For tests and
 * inspection.  d_scratch: affnet_match_guided_scratch_bytes(n1, n2, 1).  AFFNET_ERR_INVALID: an unknown kind, a radius that is not finite
 * and > 0, a negative size, a NULL pointer. */
int affnet_guided_mask(affnet_ctx* ctx, const float* d_lafs1, int n1, const float* d_lafs2, int n2, const double* d_model, int kind,
                       float radius, uint8_t* d_mask, void* d_scratch, void* stream);

/* ---- epipolar verification and guided matching for many image pairs in one call ----
 *
 * The rules of the *_many block above hold here word for word: the same pair table d_pairs (P,4) = {row1, n1, row2, n2} on the device, every
 * kernel tests its table row BEFORE any load through it, indices are LOCAL to the pair's segments, outputs are pair-major with the caps as
 * row pitch, rows at or beyond a pair's n1 / count are neither read nor written.  Per pair the kernels run the device code of the
 * single-pair calls (the same functions): every output of pair p is, bit for bit, what affnet_epipolar_verify / affnet_match_guided write
 * for that pair's segments.  n_pairs == 0 is valid and launches nothing; n_pairs <= 65535.  No allocation, no synchronisation, all work on
 * `stream`; the number of launches does not depend on P. */

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_epipolar_verify_many.  Negative arguments count as 0. */
size_t affnet_epipolar_many_scratch_bytes(int n_pairs, int t_max, int rounds);

/* affnet_epipolar_verify per pair, with one inl_th, rounds, seed and lo_iters for all.  d_tent (P,t_max,2) as affnet_match_snn_many /
 * affnet_match_guided_many write it with n1_max = t_max (so a row with n1 > t_max is out of range here as it is there; there is no cap on
 * n2); d_count (P) or NULL (= t_max rows are valid in every pair).  d_counts (P,t_max*rounds), hypothesis h = s * rounds + r of pair p at
 * d_counts[p * t_max * rounds + h]; d_model (P,9) double; d_inlier (P,t_max) uint8; d_summary (P,4).
 * A row out of range: summary {-1, 0, 0, 1 | AFFNET_VERIFY_FLAG_PAIR_RANGE}, the model all zero (what flag 1 leaves in
 * affnet_epipolar_verify, not the identity), nothing written to d_counts or d_inlier.  A valid empty pair (count 0): {-1, 0, 0, 1}.
 * AFFNET_ERR_INVALID in front of the first launch: every check of affnet_epipolar_verify, a NULL d_pairs, a negative rows1, rows2,
 * n_pairs or t_max, n_pairs > 65535, t_max * rounds above INT32_MAX. */
int affnet_epipolar_verify_many(affnet_ctx* ctx, const float* d_lafs1, int rows1, const float* d_lafs2, int rows2, const int32_t* d_pairs,
                                int n_pairs, const int32_t* d_tent, const int32_t* d_count, int t_max, float inl_th, int rounds, uint32_t seed,
                                int lo_iters, int32_t* d_counts, double* d_model, uint8_t* d_inlier, int32_t* d_summary, void* d_scratch,
                                void* stream);

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_match_guided_many called with this n_chunks (0: enough for whatever the
 * library may choose).  Negative arguments count as 0. */
size_t affnet_match_guided_many_scratch_bytes(int n_pairs, int n1_max, int n2_max, int n_chunks);

/* affnet_match_guided per pair, with one kind, radius, snn_threshold, max_dist and flags for all.  Descriptors and frames of a side lie
 * in one (rows,128) and one (rows,2,3) buffer as for affnet_match_snn_many.  Per pair: its own model, row p of d_model (P,9) double, read
 * on the device where a *_many verification left it; its own gate, row p of d_gate (P,4) - the d_summary of that verification - or NULL;
 * its own per-point terms, squared norms and backward lists (in the scratch).  d_dist, d_idx (P,n1_max,2); d_tent (P,n1_max,2);
 * d_count (P).  n_chunks column chunks per launch, 0: the library chooses, counting the row blocks of all P pairs; the result does not
 * depend on it.
 * A row out of range (the rule above, with both caps): count 0, nothing else written.  n1 == 0: count 0, nothing else written; n2 == 0
 * or a gate row with d_gate[4 p + 3] & 1 (which an out-of-range row of a *_many verification carries too): count 0, the pair's lists
 * unfilled.
 * AFFNET_ERR_INVALID in front of the first launch: every check of affnet_match_guided, a NULL d_pairs, a negative rows1, rows2, n_pairs,
 * n1_max or n2_max, n_pairs > 65535, a d_scratch that is not 16-byte aligned. */
int affnet_match_guided_many(affnet_ctx* ctx, const float* d_desc1, int rows1, const float* d_desc2, int rows2, int dim, const float* d_lafs1,
                             const float* d_lafs2, const int32_t* d_pairs, int n_pairs, int n1_max, int n2_max, const double* d_model, int kind,
                             float radius, float snn_threshold, float max_dist, int flags, int n_chunks, const int32_t* d_gate, float* d_dist,
                             int32_t* d_idx, int32_t* d_tent, int32_t* d_count, void* d_scratch, void* stream);

/* ---- ratio-test matching: per-row second nearest, first geometrically inconsistent neighbour, mutual check ----
 *
 * affnet_match_snn reproduces the reference's evaluation script, whose "second nearest" is the row minimum after the columns of EVERY row's
 * nearest neighbour were struck out; affnet_match_guided has the per-row list of two but needs a verified model.  This is the matcher in
 * front of verification: Lowe's ratio test against the row's own second neighbour, or - radius >= 0 - against the first neighbour that is
 * geometrically inconsistent with the nearest one (FGINN, Mishkin et al., MODS 2015): a detector that fires several times on one structure
 * makes the second nearest descriptor of a good match the same physical point, and the plain ratio then refuses the match.
 *
 * Inputs: d_desc1 (n1,128), d_desc2 (n2,128); d_lafs2 (n2,2,3), of which the centres u = lafs2[6j+2], v = lafs2[6j+5] are read, may be NULL
 * iff radius < 0; radius r in px; snn_threshold thr; max_dist; flags.  Everything below is fp32, one rounding per written operation (no
 * fused multiply-add).
 *
 * Distance of a pair: the element affnet_distance_matrix writes for it, bit for bit.  Order of candidates: a NaN distance in front of
 * every number, then the smaller distance, then the smaller index (affnet_knn's order).
 *   d_dist (n1,2), d_idx (n1,2): slot 0 of row i is the first column in that order over all columns - for every radius what
 *   affnet_knn(k = 1) writes.  Slot 1 is the first column j != idx[i][0] that is inconsistent with slot 0:
 *     radius < 0: every such column is inconsistent; the two slots are what affnet_knn(k = 2) writes.
 *     radius >= 0, j1 = idx[i][0]: du = u[j] - u[j1], dv = v[j] - v[j1]; inconsistent iff !((du*du + dv*dv) <= r*r).  A non-finite centre
 *     makes the comparison false, so the column counts as inconsistent.
 *   An unfilled slot is (+inf, -1).
 *   With AFFNET_RATIO_MUTUAL, back[j] = the first row of column j in that order, with no geometry, or -1 (kept in the scratch).
 *
 * Selection, in row order: (i, idx[i][0]) is kept iff idx[i][0] >= 0 && dist[i][0] <= max_dist &&
 * dist[i][0] / (dist[i][1] + 1e-8f) <= thr (with no inconsistent column the ratio is 0) && (no AFFNET_RATIO_MUTUAL || back[idx[i][0]] == i).
 * A NaN nearest distance is refused, as affnet_match_snn refuses it.  d_tent (n1,2) int32 receives the kept pairs, d_count their number;
 * rows of d_tent at or beyond the count are not written.
 *
 * The search runs like affnet_knn's: row blocks x n_chunks column chunks, a merge over the chunks; n_chunks = 0: the library chooses
 * (affnet_knn_chunks); the result does not depend on it.  radius < 0 is one pass with lists of two; radius >= 0 is exact too and takes two
 * passes (the nearest column, then the first inconsistent one: no list of fixed length holds it once enough detections share a place).
 * The backward pass is the forward kernel with the sides exchanged.  One linear chain of launches on `stream`, no allocation, no
 * synchronisation.  n1 == 0 or n2 == 0 is valid and gives count 0.
 * AFFNET_ERR_INVALID in front of the first launch: dim != 128, an unknown flag bit, a radius that is NaN or +inf, d_lafs2 == NULL with
 * radius >= 0, a NaN max_dist, a negative size, n_chunks outside 0..65535, any other NULL pointer, a d_scratch that is not 16-byte aligned. */
#define AFFNET_RATIO_MUTUAL 1    /* flags bit 0: keep (i, j) only if i is also the first row of column j */

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_match_ratio called with this n_chunks (0: enough for whatever the library
 * may choose).  Negative arguments count as 0. */
size_t affnet_match_ratio_scratch_bytes(int n1, int n2, int n_chunks);

int affnet_match_ratio(affnet_ctx* ctx, const float* d_desc1, int n1, const float* d_desc2, int n2, int dim, const float* d_lafs2, float radius,
                       float snn_threshold, float max_dist, int flags, int n_chunks, float* d_dist, int32_t* d_idx, int32_t* d_tent,
                       int32_t* d_count, void* d_scratch, void* stream);

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_match_ratio_many called with this n_chunks (0: enough for whatever the
 * library may choose).  Negative arguments count as 0. */
size_t affnet_match_ratio_many_scratch_bytes(int n_pairs, int n1_max, int n2_max, int n_chunks);

/* affnet_match_ratio per pair, with one radius, snn_threshold, max_dist and flags for all; the rules of the *_many blocks above hold word
 * for word.  Descriptors of a side lie in one (rows,128) buffer, the frames of side 2 in one (rows2,2,3) buffer, as for
 * affnet_match_snn_many.  Per pair: its own squared norms, nearest columns and backward lists (in the scratch).  d_dist, d_idx
 * (P,n1_max,2); d_tent (P,n1_max,2); d_count (P).  Every output of pair p is, bit for bit, what affnet_match_ratio writes for that pair's
 * segments, with indices LOCAL to the segments.  n_chunks column chunks per launch, 0: the library chooses, counting the row blocks of all
 * P pairs; the result does not depend on it.  The number of launches does not depend on P.
 * A row out of range (the rule above, with both caps): count 0, nothing else written.  n1 == 0: count 0, nothing else written; n2 == 0:
 * count 0, the pair's lists unfilled.
 * AFFNET_ERR_INVALID in front of the first launch: every check of affnet_match_ratio, a NULL d_pairs, a negative rows1, rows2, n_pairs,
 * n1_max or n2_max, n_pairs > 65535. */
int affnet_match_ratio_many(affnet_ctx* ctx, const float* d_desc1, int rows1, const float* d_desc2, int rows2, int dim, const float* d_lafs2,
                            const int32_t* d_pairs, int n_pairs, int n1_max, int n2_max, float radius, float snn_threshold, float max_dist,
                            int flags, int n_chunks, float* d_dist, int32_t* d_idx, int32_t* d_tent, int32_t* d_count, void* d_scratch,
                            void* stream);

/* ---- descriptor index: k nearest neighbours over many images, shortlist by votes ---- */

/* The front of the retrieval loop extract -> index -> shortlist -> verify: the rows of all database images lie back to back in one (n2,128)
 * buffer (side 2 of the *_many calls above), a query image's rows are searched against all of them at once, and every image collects votes
 * from the neighbours found among its rows.  No allocation, no synchronisation, all work on `stream`; all buffers are the caller's. */
#define AFFNET_KNN_MAX_K 8

/* Host only.  The library's own choice of column chunks for an n1 x n2 search, >= 1 for every size: enough chunks to give the device of `ctx`
 * (NULL: a 256-CU part) a few workgroups per CU, but no chunk below a floor of 16-column tiles (descriptor index). */
int affnet_knn_chunks(const affnet_ctx* ctx, int n1, int n2);

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_knn called with this n_chunks; n_chunks = 0: enough for whatever affnet_knn_chunks
 * may choose.  Negative arguments count as 0. */
size_t affnet_knn_scratch_bytes(int n1, int n2, int k, int n_chunks);

/* For every row of d_q (n1,128) the k rows of d_db (n2,128) at the smallest distance sqrt(|a|^2 + |b|^2 - 2 a.b + 1e-6): d_dist (n1,k) ascending,
 * d_idx (n1,k) the database rows.  Every distance is, bit for bit, the element affnet_distance_matrix writes for that (row, column), and with
 * no skip range column 0 is what affnet_match_snn writes to d_min_dist / d_idx.  Order: a NaN distance (the fp32 expansion can go below -1e-6
 * for near-identical vectors) in front of every number, then the smaller distance, then the smaller database row - a total order, so the
 * result does not depend on n_chunks.
 * Rows skip_row <= c < skip_row + skip_n of the database are no candidates (a query against an index that contains the query's own image);
 * the range is clipped to [0, n2), skip_n = 0 is no skip.  Slots for which no candidate is left hold idx = -1, dist = +inf; n2 = 0 is valid
 * and gives only such slots; n1 = 0 writes nothing.
 * The search runs on a grid of cdiv(n1, 64) x n_chunks workgroups: chunk c owns the 16-column tiles [c * tpc, (c + 1) * tpc),
 * tpc = cdiv(cdiv(n2, 16), n_chunks) (a chunk that starts behind n2 is empty), and a second kernel merges the chunks' lists per row.
 * n_chunks = 0: affnet_knn_chunks(ctx, n1, n2); at most 65535.
 * AFFNET_ERR_INVALID in front of the first launch: k outside 1..AFFNET_KNN_MAX_K, dim != 128, a negative size, n_chunks < 0, a NULL pointer. */
int affnet_knn(affnet_ctx* ctx, const float* d_q, int n1, const float* d_db, int n2, int dim, int k, int skip_row, int skip_n, int n_chunks,
               float* d_dist, int32_t* d_idx, void* d_scratch, void* stream);

/* One vote per (query row, image) from the neighbours affnet_knn found: d_votes (n_images) int32 is zeroed, then row r takes its LAST slot as the
 * background distance d_last = dist[r][k-1], and neighbour j < k-1 with idx >= 0 votes for image d_row_image[idx] iff
 * !(dist[r][j] > ratio * d_last) (one fp32 multiply, one compare: a NaN distance votes, and so does every neighbour of a row whose last slot is
 * unfilled, +inf) and no earlier neighbour of the row voted for that image.  A row gives at most k-1 votes, at most one per image:
 * k - 1 is the largest number of database images that can show the same feature and still all receive its vote.  k = 1 gives all zeros.
 * (Plain counting of neighbours ranks images by their size; the ratio gate counts a neighbour only when it stands out from the background.)
 * d_row_image (n2) int32 = the image of every database row.  An idx outside [0, n2) other than -1 and an image outside [0, n_images) are
 * skipped, not trusted.  Integer atomics: the result does not depend on the order of execution. */
int affnet_knn_vote(affnet_ctx* ctx, const float* d_dist, const int32_t* d_idx, int n1, int k, float ratio, const int32_t* d_row_image, int n2,
                    int n_images, int32_t* d_votes, void* stream);

/* ---- descriptor index on int8 descriptors: exact integer k-NN on the i8 matrix instruction ---- */

/* The same search over descriptors stored as 8-bit integers (132 bytes per row with its squared norm instead of 512): the shortlist needs ranks and
 * a ratio gate only, and the exact fp32 matcher and the spatial verification still decide what is reported about a pair.  d_dist / d_idx of
 * affnet_knn_q8 have the shapes and the order affnet_knn_vote reads.  No allocation, no synchronisation, all work on `stream`. */

/* d_desc (n,128) float -> d_q (n,128) int8, d_sq (n) int32.  The rule, in fp32: q = clamp(rintf(x * scale), -127, 127) - one multiply, round half
 * to even, NaN -> 0, +-inf -> +-127; d_sq[r] = the sum of q^2 over the row, exact (at most 128 * 127^2).  d_desc and d_q are 16-byte aligned.
 * n = 0 is a no-op.  AFFNET_ERR_INVALID in front of the first launch: dim != 128, a negative n, scale not finite or <= 0, a NULL pointer. */
int affnet_quantize_desc(affnet_ctx* ctx, const float* d_desc, int n, int dim, float scale, int8_t* d_q, int32_t* d_sq, void* stream);

/* Host only.  The most column chunks the library chooses for an n1 x n2 int8 search, >= 1 for every size: what k <= 2 takes - enough chunks to
 * give the device of `ctx` (NULL: a 256-CU part) the workgroups it keeps resident, but no chunk below a floor of 32-column steps; k > 2 runs
 * on twice the row blocks and takes about half (descriptor index, int8). */
int affnet_knn_q8_chunks(const affnet_ctx* ctx, int n1, int n2);

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_knn_q8 called with this n_chunks; n_chunks = 0: enough for whatever
 * affnet_knn_q8_chunks may choose.  Negative arguments count as 0. */
size_t affnet_knn_q8_scratch_bytes(int n1, int n2, int k, int n_chunks);

/* For every row of d_q (n1,128) int8 the k rows of d_db (n2,128) int8 at the smallest d2 = (qsq[r] + dbsq[c]) - 2 dot(q[r], db[c]), all in int32:
 * exact, 0 <= d2 <= 128 * 254^2 = 8 258 048 < 2^24.  d_qsq (n1) / d_dbsq (n2): the rows' sums of squares as affnet_quantize_desc writes them.
 * Order: the smaller d2, then the smaller database row - a total order without NaN, so the result does not depend on n_chunks.
 * Outputs, (n1,k) each, ascending in that order: d_dist2 = d2; d_dist = sqrtf((float)d2) / scale, exactly these two correctly rounded fp32
 * operations ((float)d2 is exact), the distance in the units of the descriptors that were quantised with `scale`; d_idx = the database row.
 * With descriptors whose entries were not clipped by the quantiser, d_dist is within sqrt(128) / scale of the true Euclidean distance (each
 * row moves by at most 0.5 sqrt(128) / scale in the 2-norm).  Slots for which no candidate is left hold (INT32_MAX, +inf, -1).
 * skip_row / skip_n, n_chunks (0 = the library's choice for this k, at most affnet_knn_q8_chunks(ctx, n1, n2); at most 65535), n2 = 0 and
 * n1 = 0 as in affnet_knn.
 * The search runs on a grid of cdiv(n1, R) x n_chunks workgroups, R = 256 query rows for k <= 2 and 128 above: chunk c owns the 32-column steps
 * [c * spc, (c + 1) * spc), spc = cdiv(cdiv(n2, 32), n_chunks), and a second kernel merges the chunks' lists per row.  d_q and d_db are
 * 16-byte aligned.
 * AFFNET_ERR_INVALID in front of the first launch: k outside 1..AFFNET_KNN_MAX_K, dim != 128, a negative size, n_chunks < 0 or > 65535, scale
 * not finite or <= 0, a NULL pointer. */
int affnet_knn_q8(affnet_ctx* ctx, const int8_t* d_q, const int32_t* d_qsq, int n1, const int8_t* d_db, const int32_t* d_dbsq, int n2, int dim,
                  int k, int skip_row, int skip_n, int n_chunks, float scale, int32_t* d_dist2, float* d_dist, int32_t* d_idx, void* d_scratch,
                  void* stream);

/* ---- descriptor index, inverted file: the search over the rows of a few k-means cells ---- */

/* A codebook of n_cells centroids cuts the database rows into cells; the rows are stored a second time in cell order, and a query row is
 * compared with the rows of its nprobe nearest cells only.  The tables of an index over n2 rows:
 *   d_sorted (n2,128)        the database rows, permuted so that each cell's rows are contiguous;
 *   d_sorted_sq (n2)         their squared norms (affnet_ivf_sqnorm);
 *   d_perm (n2) int32        sorted position -> original database row, ASCENDING INSIDE EVERY CELL (a stable sort of the assignment);
 *   d_cell_start (n_cells+1) int32, cell c owns the positions [cell_start[c], cell_start[c+1]); cells may be empty and start anywhere;
 *   d_centroids (n_cells,128).
 * The distances are affnet_knn's, bit for bit, and so is the order; what is approximate is which rows are looked at.  d_dist / d_idx have the
 * shapes and the order affnet_knn_vote reads, d_idx holds ORIGINAL database rows. */
#define AFFNET_IVF_MAX_PROBE 8

/* d_sq[r] = the squared norm of row r of d_x (n,128), by the reduction affnet_knn applies to its rows (the same bits).  n = 0 is a no-op.
 * AFFNET_ERR_INVALID in front of the first launch: dim != 128, a negative n, a NULL pointer. */
int affnet_ivf_sqnorm(affnet_ctx* ctx, const float* d_x, int n, int dim, float* d_sq, void* stream);

/* The update of one Lloyd iteration: d_centroids[c] = (float)(sum / count) over the rows d_rows[d_perm[p]], p in [cell_start[c], cell_start[c+1]),
 * summed in ascending p into double accumulators (no floating-point atomics: the bytes repeat run to run); an empty cell keeps its centroid.
 * d_perm (n) / d_cell_start (n_cells+1) as above, for the assignment of the n rows of d_rows (n,128).  n = 0 is a no-op.
 * AFFNET_ERR_INVALID in front of the first launch: dim != 128, a negative n, n_cells < 1, a NULL pointer. */
int affnet_ivf_cell_means(affnet_ctx* ctx, const float* d_rows, int n, int dim, const int32_t* d_perm, const int32_t* d_cell_start, int n_cells,
                          float* d_centroids, void* stream);

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_ivf_search.  Negative arguments count as 0. */
size_t affnet_ivf_scratch_bytes(int n1, int n_cells, int nprobe, int k);

/* For every row of d_q (n1,128) the k nearest among the database rows of its nprobe nearest cells: d_dist (n1,k) ascending, d_idx (n1,k) the
 * original rows, order and unfilled slots (+inf, -1) as in affnet_knn.  Original rows skip_row <= c < skip_row + skip_n are no candidates.
 * Steps, one linear chain of launches on `stream`, no allocation, no synchronisation: the coarse step affnet_knn(d_q, d_centroids, k = nprobe)
 * (ties go to the smaller cell; with n_cells < nprobe the last probe slots are -1 and are skipped) -> d_probes (n1,nprobe) int32 when not NULL;
 * the (row, cell) pairs grouped by cell on the device (integer atomics, a scan, a scatter; the order inside a group may vary from run to run,
 * the result cannot: every pair is processed once and every selection uses a total order); one workgroup per (cell, block of 16 rows of its
 * group) - their number is known on the device only, the grid is cdiv(n1 * nprobe, 16) + min(n_cells, n1 * nprobe) and a workgroup past the
 * last item returns at once; per row a merge of its nprobe partial lists.  A cell is not split over workgroups by columns: one very large
 * cell is searched correctly and slowly.
 * n1 = 0 is a no-op; n2 = 0 (d_cell_start all zeros) gives only unfilled slots.
 * AFFNET_ERR_INVALID in front of the first launch: dim != 128, k outside 1..AFFNET_KNN_MAX_K, nprobe outside 1..AFFNET_IVF_MAX_PROBE,
 * n_cells < 1, a negative size, n1 * nprobe * k above 2^31 - 1, a NULL pointer other than d_probes. */
int affnet_ivf_search(affnet_ctx* ctx, const float* d_q, int n1, const float* d_sorted, const float* d_sorted_sq, const int32_t* d_perm, int n2,
                      const int32_t* d_cell_start, const float* d_centroids, int n_cells, int dim, int k, int nprobe, int skip_row, int skip_n,
                      float* d_dist, int32_t* d_idx, int32_t* d_probes, void* d_scratch, void* stream);

/* ---- descriptor index, inverted file over int8 rows: the cells hold the quantised rows, the distances inside them are affnet_knn_q8's ---- */

/* The two ideas combined: the codebook, the coarse step and the cell layout of affnet_ivf_search, the rows of the cells stored as int8
 * (affnet_quantize_desc) with their int32 sums of squares.  The tables of an index over n2 rows:
 *   d_sorted_q (n2,128) int8   the quantised database rows in cell order (row p = the quantised original row d_perm[p]);
 *   d_sorted_sq (n2) int32     their sums of squares, in cell order;
 *   d_perm, d_cell_start, d_centroids (float) as above.
 * 136 bytes per database row.  Every reported d2 is exact, the order (d2, ORIGINAL row) is total, so the result is a function of the inputs. */

/* Host only.  Bytes of d_scratch (16-byte aligned) of affnet_ivf_search_q8.  Negative arguments count as 0. */
size_t affnet_ivf_q8_scratch_bytes(int n1, int n_cells, int nprobe, int k);

/* For every query row the k nearest, by the exact integer d2 of affnet_knn_q8, among the database rows of its nprobe nearest cells.
 * d_q (n1,128) float: the query rows, read by the coarse step only - affnet_knn(d_q, d_centroids, k = nprobe) as it stands, so the cells looked
 * at (d_probes (n1,nprobe) when not NULL, -1 where the codebook has fewer cells) are bit for bit affnet_ivf_search's for the same rows and
 * centroids.  d_qq (n1,128) int8 / d_qsq (n1): the same rows quantised with `scale` (affnet_quantize_desc).
 * Inside the cells d2 = (qsq[r] + sorted_sq[c]) - 2 dot(qq[r], sorted_q[c]) in int32; order: the smaller d2, then the smaller ORIGINAL row.
 * Outputs, (n1,k) each, exactly as affnet_knn_q8 writes them: d_dist2 = d2, d_dist = sqrtf((float)d2) / scale, d_idx = the original row;
 * unfilled slots hold (INT32_MAX, +inf, -1).  Original rows skip_row <= c < skip_row + skip_n are no candidates.  With every cell probed
 * the three outputs are affnet_knn_q8's bytes on the unpermuted int8 rows.
 * Steps, one linear chain of launches on `stream`, no allocation, no synchronisation: the coarse step and the grouping of affnet_ivf_search
 * (the result does not depend on the order in which its atomics hand out places); one workgroup per (cell, block of 16 rows of its group),
 * each wave walking 64-column steps of the cell on v_mfma_i32_16x16x64_i8; per row the merge of its nprobe partial lists.  A cell is not split
 * over workgroups by columns.  d_qq and d_sorted_q are 16-byte aligned.
 * n1 = 0 is a no-op; n2 = 0 (d_cell_start all zeros) gives only unfilled slots.
 * AFFNET_ERR_INVALID in front of the first launch: dim != 128, k outside 1..AFFNET_KNN_MAX_K, nprobe outside 1..AFFNET_IVF_MAX_PROBE,
 * n_cells < 1, a negative size, n1 * nprobe * k above 2^31 - 1, scale not finite or <= 0, a NULL pointer other than d_probes. */
int affnet_ivf_search_q8(affnet_ctx* ctx, const float* d_q, const int8_t* d_qq, const int32_t* d_qsq, int n1, const int8_t* d_sorted_q,
                         const int32_t* d_sorted_sq, const int32_t* d_perm, int n2, const int32_t* d_cell_start, const float* d_centroids,
                         int n_cells, int dim, int k, int nprobe, int skip_row, int skip_n, float scale, int32_t* d_dist2, float* d_dist,
                         int32_t* d_idx, int32_t* d_probes, void* d_scratch, void* stream);

/* ---- fused pipeline ------------------------------------------------------------------------ */

typedef struct affnet_nets {
    const float* d_affnet;   /* packed AffNet weights, NULL => num_Baum_iters = 0            */
    const float* d_orinet;   /* packed OriNet weights, NULL => do_ori must be 0              */
    const float* d_hardnet;  /* packed HardNet weights, NULL => no descriptors               */
    /* The reference's default slot fillers (SparseImgRepresenter.py:42-49), used when the CNN of the slot is NULL:       */
    const float* h_orientation_window;  /* HOST, 361 floats: OrientationDetector(19) when do_ori and d_orinet == NULL     */
    const float* h_baumberg_window;     /* HOST, 361 floats: AffineShapeEstimator(19) when baum_iters > 0, d_affnet NULL   */
} affnet_nets;

/* Whole path, image resident -> results resident, zero host synchronisation:
 * pyramid -> detect -> [AffNet shape + filter] -> [OriNet] -> denormalise ->
 * [level select -> sample -> HardNet].
 * Replaces ScaleSpaceAffinePatchExtractor.forward (SparseImgRepresenter.py:189-209) +
 * extract_patches_from_pyr (:181-188) + HardNet forward = get_geometry_and_descriptors
 * (train_OriNet_test_on_graffity.py:293-298).
 * Outputs (capacity affnet_capacity_final rows): d_lafs_px (cap,2,3), d_resp (cap),
 * d_ids (cap,3) (octave, level-1, pixel) of the detection, d_desc (cap,128) or NULL,
 * d_count (1). */
int affnet_extract_features(affnet_ctx* ctx, const affnet_nets* nets, const float* d_img, int do_ori,
                            float* d_lafs_px, float* d_resp, int32_t* d_ids, float* d_desc,
                            int32_t* d_count, void* stream);

/* The two halves of affnet_extract_features, so that a caller can software-pipeline images over two
 * streams (detector of image i+1 next to the CNN stages of image i; the caller orders the streams with
 * events and must not start affnet_detect_image on a context before the previous
 * affnet_describe_detected on it has finished):
 *   affnet_detect_image      = pyramid + detector into the context's internal candidate list;
 *   affnet_describe_detected = AffNet shape + filter, OriNet, denormalise, level select, HardNet. */
int affnet_detect_image(affnet_ctx* ctx, const float* d_img, void* stream);
/* Detector half on caller-supplied response maps (custom RespNet slot; the pyramid must have been built with
 * affnet_pyramid_build): candidates go to the internal list consumed by affnet_describe_detected. */
int affnet_detect_image_responses(affnet_ctx* ctx, const float* d_responses, void* stream);
int affnet_describe_detected(affnet_ctx* ctx, const affnet_nets* nets, int do_ori, float* d_lafs_px, float* d_resp,
                             int32_t* d_ids, float* d_desc, int32_t* d_count, void* stream);

/* OnePassSIR detector half (context created with cfg->onepass): replaces OnePassSIR.multiScaleDetectorAff + the x mrSize of
 * OnePassSIR.forward (OnePassSIR.py:53-115,146), NMS3dAndComposeAAff (HandCraftedModules.py:292-363), sc_y_x_and_A2LAFs
 * (LAF.py:442-449) and the boundary test of OnePassSIR.py:91.
 *   d_img != NULL: the pyramid is built first; NULL: it has been built with affnet_pyramid_build;
 *   d_packed_fullconv != NULL (affnet_cnn32_pack_weights(AFFNET_NET_AFFNET_FULLCONV, ...)): the dense affine-shape map of every
 *   octave is computed from its level 0 (OnePassSIR.py:69); NULL: the caller has written the maps of a foreign dense AffNet,
 *   planar (4, h_o, w_o) per octave, at affnet_affmap_offset(ctx, o) (+ affnet_affmap_image_stride per image).
 * Follow with affnet_describe_detected(nets->d_affnet = NULL, ...): orientation, denormalisation, descriptors. */
int affnet_detect_image_onepass(affnet_ctx* ctx, const float* d_packed_fullconv, const float* d_img, void* stream);
/* Same with a custom RespNet slot (OnePassSIR.py:24,38-41,71: RespNet(level, sigma) per pyramid level): the pyramid has been built
 * with affnet_pyramid_build and d_responses holds the slot's response maps laid out like the pyramid (affnet_pyramid_level_offset /
 * affnet_pyramid_image_stride); only clamp(r - th, 0) is applied to them. */
int affnet_detect_image_onepass_responses(affnet_ctx* ctx, const float* d_packed_fullconv, const float* d_responses, void* stream);

/* Copies the context's internal detection list (what affnet_detect_image / _responses / _onepass produced and
 * affnet_describe_detected consumes) into caller buffers of capacity affnet_capacity_prefilter(ctx) rows per image: responses,
 * NORMALISED LAFs (x mrSize), (octave, level, pixel) ids, row counts.  For callers that run a foreign (Python) OriNet / AffNet /
 * descriptor between the stages (SparseImgRepresenter.py:38-49, OnePassSIR.py:44-47) on exactly the rows the fused path would use. */
int affnet_detected_list(affnet_ctx* ctx, float* d_resp, float* d_lafs, int32_t* d_ids, int32_t* d_count, void* stream);
/* Caller-supplied keypoint frames instead of a detector half: fills the context's internal detection list (and the per-image
 * counters behind affnet_read_counts / affnet_counter_offset) as a detector half leaves them, for B images, without a host
 * synchronisation.  Follow with affnet_describe_detected; the pyramid must have been built with affnet_pyramid_build.
 * This is the way in that the reference's public getAffineShape / getOrientation (SparseImgRepresenter.py:113-180) offer: any
 * frames, not only the Hessian detector's.
 *   d_lafs  (B,n_max,2,3), n_max <= affnet_capacity_prefilter(ctx) (else AFFNET_ERR_INVALID).  normalised = 0: pixel frames as
 *           affnet_extract_features returns them - they describe the whole measurement region, mrSize is not applied again; they
 *           are normalised with affnet_scale_lafs(inverse = 1)'s constants.  normalised = 1: the reference's normalised frames, as
 *           getAffineShape takes them (what affnet_detected_list returns).
 *   d_ids   NULL: (octave, level) of every frame by the rule of get_pyramid_and_level_index_for_LAFs (LAF.py:450-472) at patch
 *           size ps, bit-identical to affnet_level_select (normalised frames are denormalised like affnet_scale_lafs first), and
 *           column 2 = the source row index i.  Otherwise (B,n_max,3), copied through: columns 0 / 1 are the reference's
 *           final_pyr_idxs / final_level_idxs (the samplers clamp them to the pyramid), column 2 is an opaque caller tag.  Column 2
 *           survives the shape stage into affnet_describe_detected's d_ids: every output row names the input row it came from.
 *   d_resp  NULL: the response of row i is (float)(n_max - i), strictly decreasing: caller order is kept and a top-N keeps the
 *           first N survivors of the shape filter.  Otherwise (B,n_max).
 *   d_count NULL: n_max rows in every image.  Otherwise (B); a count above n_max is clamped to n_max (below 0: to 0) and bit 16
 *           of the overflow flag is set.
 * The rows are taken as response-sorted (lazy second AffNet pass, prefix selection) only if this call has verified that the
 * responses of the rows < count are non-increasing; unsorted rows take the general paths with identical results.
 * A row with a non-finite frame entry or response is stored as an all-zero frame with response 0 and bit 32 of the overflow flag
 * is set: affnet_read_counts then returns AFFNET_ERR_INVALID.  The results of such a call are unspecified, but no non-finite
 * coordinate reaches a sampler. */
int affnet_load_frames(affnet_ctx* ctx, const float* d_lafs, int normalised, const float* d_resp, const int32_t* d_ids,
                       const int32_t* d_count, int n_max, int ps, void* stream);

/* affnet_pyramid_build (skipped when d_img == NULL: the pyramid of the image is already in the workspace),
 * affnet_load_frames(d_lafs_px, normalised = 0, ids NULL, ps = the patch size of the first slot that samples: 32 for AffNetFast /
 * OriNetFast / HardNet, 19 for the hand-crafted windows) and affnet_describe_detected in one call: "frames in, shapes, orientations
 * and descriptors out" (examples/SIFT-AffNet-HardNet-kornia-matching.ipynb of the reference) with pyramid-level sampling, the
 * shape filter / top-N and the batch per launch of the fused path.  d_lafs_px (B,n_max,2,3) pixel frames, d_resp_in (B,n_max) or
 * NULL, d_count_in (B) or NULL as for affnet_load_frames; outputs as for affnet_extract_features, d_ids[..., 2] = source row. */
int affnet_describe_frames(affnet_ctx* ctx, const affnet_nets* nets, const float* d_img, const float* d_lafs_px, const float* d_resp_in,
                           const int32_t* d_count_in, int n_max, int do_ori, float* d_lafs_px_out, float* d_resp, int32_t* d_ids,
                           float* d_desc, int32_t* d_count, void* stream);

/* Float offset (from the workspace base) of the (4, h_o, w_o) affine-shape map of octave o of image 0, and the floats between the
 * maps of consecutive images; -1 / 0 when the context has no OnePassSIR areas. */
int64_t affnet_affmap_offset(const affnet_ctx* ctx, int octave);
int64_t affnet_affmap_image_stride(const affnet_ctx* ctx);

/* The whole path as ONE HIP graph.  affnet_graph_capture_extract stream-captures affnet_extract_features with exactly these buffers
 * (same arguments; `stream` must be an explicit, non-null stream; nothing executes during capture) and instantiates the graph;
 * affnet_graph_launch replays it: one launch instead of ~45 for callers that process one image at a time
 * (hesaffnet.py:35-60 per image).  The captured buffers (image, outputs, workspace, packed weights) must stay alive and in place;
 * new image content is copied into the captured d_img before a launch.  A later capture on the same context replaces the graph. */
int affnet_graph_capture_extract(affnet_ctx* ctx, const affnet_nets* nets, const float* d_img, int do_ori, float* d_lafs_px, float* d_resp,
                                 int32_t* d_ids, float* d_desc, int32_t* d_count, void* stream);
int affnet_graph_launch(affnet_ctx* ctx, void* stream);

/* Stage timing with HIP events recorded on the caller's stream around the stages of
 * affnet_extract_features (no host synchronisation while enabled; a ring of 256 calls).
 * Stages: 0 pyramid, 1 detector, 2 AffNet trunk(+sampling), 3 shape filter/select, 4 OriNet(+rotation),
 * 5 denormalise + level select (with a native OriNet and descriptors this work is done by OriNet's finish kernel, i.e. inside
 * stage 4, and stage 5 is empty), 6 HardNet trunk (+sampling), 7 HardNet head GEMM. */
#define AFFNET_PROFILE_STAGES 8
int affnet_profile_enable(affnet_ctx* ctx, int on);
/* After the caller synchronised the stream(s): sums the elapsed milliseconds per stage over the
 * calls recorded since the last read, returns the number of calls in *n_calls and clears the ring. */
int affnet_profile_read(affnet_ctx* ctx, double sum_ms[AFFNET_PROFILE_STAGES], int32_t* n_calls);

/* The one optional read-back: copies counters to the host after synchronising `stream`:
 * out[0] = rows after detection, out[1] = rows after shape filter, out[2] = capacity-overflow
 * flag, out[3] = raw maxima found (sums / OR over the images of the batch).
 * Returns AFFNET_ERR_CAPACITY when a fixed-capacity device list overflowed (results would be truncated: treat as an
 * error), AFFNET_ERR_EMPTY when no image of the call produced a detection (out[] is still filled), else AFFNET_OK.
 * Bits of the flag: 1 raw-maxima list, 2 candidate list, 4 selected list, 8 shape-stage output, 16 a device row count handed to
 * affnet_load_frames exceeded its n_max (clamped), 32 affnet_load_frames met a non-finite row: that one is the caller's input, not a
 * capacity, and returns AFFNET_ERR_INVALID. */
int affnet_read_counts(affnet_ctx* ctx, int32_t out[4], void* stream);

/* The same counters without a host synchronisation: int32 offset (from the workspace base) of a per-image device counter of image 0
 * and the int32 stride between images.  which: 0 = capacity-overflow flag, 1 = rows after detection, 2 = rows after the shape filter,
 * 3 = candidates the shape CNN was actually evaluated on (cfg->lazy_shape_rows), 4 = evaluated candidates that the direct-form trunk
 * recomputed (affnet_set_shape_form; 0 in form AFFNET_SHAPE_FORM_DIRECT).
 * Valid once the enqueued work has completed on the stream; -1 for a context without a workspace layout. */
int64_t affnet_counter_offset(const affnet_ctx* ctx, int which);
int64_t affnet_counter_stride(const affnet_ctx* ctx);

/* Host helper (no GPU): out[ps] = affine_grid base coordinates (linspace(-1,1,ps)*(ps-1))/ps with
 * torch's CPU rounding; exported so the CPU test-suite can pin it against torch.linspace. */
int affnet_host_base_grid(int ps, float* out);

#ifdef __cplusplus
}
#endif
#endif /* AFFNET_HIP_H */
