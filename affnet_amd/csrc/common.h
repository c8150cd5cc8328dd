// Shared host/device declarations of libaffnet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/affnet_hip.h"
#include "../../include/affnet_hip_debug.h"
#include "weights_layout.h"

#define AFF_WAVE 64

// Counter block kept at the start of the workspace "lists" area (int32 each).
enum {
    CNT_RAW0 = 0,                            // CNT_RAW0 + o : raw maxima of octave o
    CNT_CAND = AFFNET_MAX_OCTAVES,           // accepted candidates (all octaves)
    CNT_OVERFLOW,                            // != 0 : some fixed-capacity list overflowed
    CNT_SEL,                                 // rows selected by the global top-k
    CNT_EQ_TAKEN,                            // ties at the threshold already taken
    CNT_SEL_MODE,                            // 1 = top-k (descending response), 0 = keep all (key order)
    CNT_SEL_THRESH,                          // order-preserving uint key of the C-th largest response
    CNT_SEL_NEED_EQ,                         // how many keys == threshold to take
    CNT_DET,                                 // rows emitted by the detector
    CNT_SHAPED,                              // rows after the shape filter
    CNT_SURVIVED,                            // survivors of the shape filter before top-N
    CNT_CAND2,                               // OnePassSIR: candidates that passed the per-level top-k and the boundary test
    CNT_AFF_EVAL,                            // candidates the shape CNN was actually evaluated on (lazy second pass, pipeline.hip)
    CNT_SURVIVED1,                           // survivors of the first (lazy) shape pass, frozen before the second pass starts
    CNT_SEL_EQ_TOTAL,                        // candidates whose response equals the top-k threshold (ties: taken in key order)
    CNT_SEL_TIE_LO, CNT_SEL_TIE_HI,          // ties at the threshold are taken up to this (octave, level, pixel) key (64 bits, two halves)
    CNT_AFF_REEVAL,                          // shape form 1: evaluated candidates the margin rule flagged, recomputed by the direct AffNet trunk (both passes)
    CNT_POS0 = AFFNET_MAX_OCTAVES + 24,      // CNT_POS0 + (level-1)*AFFNET_MAX_OCTAVES + o : positive maxima of (octave, level)
    CNT_HYP0 = AFFNET_MAX_OCTAVES + 24 + (AFFNET_MAX_LEVELS - 2) * AFFNET_MAX_OCTAVES,   // CNT_HYP0 + 8 * o + k: positives of (octave o, level,
                                             // hypothesis) k = 0: level 1; 1 + h1: level 2 given level 1 applied (h1); 3 + h1 + 2 h2: level 3
    CNT_TOTAL = AFFNET_MAX_OCTAVES + 24 + (AFFNET_MAX_LEVELS - 2) * AFFNET_MAX_OCTAVES + 8 * AFFNET_MAX_OCTAVES
};

// CNT_OVERFLOW bits of affnet_load_frames (the detector and the shape stage use 1, 2, 4, 8; include/affnet_hip.h, affnet_read_counts)
#define OVF_FRAMES_COUNT 16        // a device row count above n_max was clamped
#define OVF_FRAMES_NONFINITE 32    // a row with a non-finite entry was stored as a zero row

#define SEL_HIST_BINS 2048     // first digit (11 bits) of the global top-k's radix select, histogrammed by many workgroups

struct RawMax {            // one 3-D local maximum found by hessian_nms_kernel
    int32_t pix;           // flat pixel index y*w+x in the octave
    int32_t lvl;           // detection level 1..nLevels
    float val;             // NMS'ed (border-zeroed) response
    float s, y, x;         // normalised centroid scale / row / column
    float prev[2];         // NMS'ed responses of the SAME pixel at detection levels lvl-1 and lvl-2 when it is a raw maximum there too (else 0):
                           // what the octaveMap replay of this pixel needs (detect.hip, resolve_*_kernel); used for <= 3 detection levels
};

struct OctaveGeom {
    int32_t h, w;
    int64_t pyr_off;       // float offset of level 0 inside the pyramid area
    int64_t map_off;       // byte offset of the uint8 octaveMap
    int64_t raw_off;       // RawMax offset of this octave's raw list
    int32_t raw_cap;
};

struct affnet_ctx {
    int device = 0;
    affnet_config cfg;
    // Image batch: every workspace area holds B images back to back ([image][...]); kernels take the image
    // index from blockIdx.y / .z and offset their pointers by the per-image strides below.
    int B = 1;
    size_t pyr_stride = 0;             // floats between the pyramids of consecutive images
    size_t map_stride = 0;             // bytes between octaveMaps
    size_t raw_stride = 0;             // RawMax entries between raw lists
    std::string err;
    OctaveGeom oct[AFFNET_MAX_OCTAVES];
    // workspace layout (byte offsets from the workspace base)
    size_t off_pyr = 0, off_map = 0, off_raw = 0, off_cnt = 0, off_hist = 0, off_cand = 0, off_sel = 0, off_stage = 0;
    // OnePassSIR extras (cfg.onepass != 0): dense affine-shape maps (4, h_o, w_o) per octave, the dense net's scratch, a second
    // candidate list and the per-(octave, level) top-k table
    size_t off_affmap = 0, off_dense = 0, off_cand2 = 0, off_lvltab = 0;
    size_t aff_stride = 0;             // floats between the affine maps of consecutive images
    size_t aff_off[AFFNET_MAX_OCTAVES] = {0};   // float offset of octave o's (4, h, w) map inside one image's block
    size_t dense_stride = 0;           // floats of dense-net scratch per image
    float* affmap = nullptr; float* dense = nullptr;
    float* cand2_resp = nullptr; float* cand2_syx = nullptr; int32_t* cand2_ids = nullptr;
    int32_t* lvltab = nullptr;
    size_t ws_bytes = 0;
    size_t pyr_floats = 0, map_bytes = 0, raw_total = 0, cand_cap = 0;
    int cap_pre = 0, cap_final = 0;
    char* ws = nullptr;
    // convenience pointers into the workspace (valid after bind)
    float* pyr = nullptr;
    uint8_t* omap = nullptr;
    RawMax* raw = nullptr;
    int32_t* cnt = nullptr;
    uint32_t* sel_hist = nullptr;        // B x SEL_HIST_BINS: histogram of the top 11 key bits of the candidate responses
    float* cand_resp = nullptr; float* cand_syx = nullptr; int32_t* cand_ids = nullptr;
    float* sel_resp = nullptr; float* sel_syx = nullptr; int32_t* sel_ids = nullptr;
    // pipeline stage buffers
    float* st_det_resp = nullptr; float* st_det_lafs = nullptr; int32_t* st_det_ids = nullptr;
    int32_t* st_det_count = nullptr;     // B contiguous detector row counts (kernels index count[image])
    float* st_A = nullptr; float* st_key = nullptr; int32_t* st_good = nullptr;
    float* st_A2 = nullptr; float* st_lafs_iter = nullptr;   // AffNet iterations > 1: current A, re-extraction LAFs
    float* st_R = nullptr; float* st_lafs_norm = nullptr; int32_t* st_lvl_ids = nullptr;
    float* st_hard_scratch = nullptr;
    float* st_lafs_shaped = nullptr;
    int32_t* st_rank = nullptr;          // partial ranks / positions of the two selection stages (cap_pre ints)
    // stage profiling (HIP events on the caller's stream)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;   // ring: PROF_RING calls x PROF_EVENTS events
    int prof_calls = 0;
    // tuning aid (include/affnet_hip_debug.h): s_memtime stamp buffer of THIS context's CNN launches, or NULL
    unsigned long long* dbg_time = nullptr;
    int shape_form = AFFNET_SHAPE_FORM_WINOGRAD;   // fused exact-fp32 shape pass (affnet_set_shape_form): Winograd trunk (form 2, selectable: with polyphase conv2 / conv4) + direct re-evaluation of the margin rule's rows, or direct only
    int arith = AFFNET_ARITH_FP32_MFMA;   // arithmetic of the CNN contractions (cfg.arith / affnet_set_arith): exact fp32 MFMA or fp32 = 3 x bf16 split operands
    int split3_variant = 0;            // tuning aid (affnet_debug_split3_variant): bit 0 = alternating wave priorities in the split HardNet loops (round 3's
                                       // tile-major loops gained 2.5 % from it, the term-major loops of round 4 lose 1 %: off)
    // the whole path captured as one HIP graph (affnet_graph_capture_extract): one launch instead of ~45 for latency-bound callers
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    // The transformed weights that are no blob sections (weights_layout.h: DerivedU, a region per net), derived from the caller's blob in front of every trunk launch that
    // reads them (derive_u.hip: aff_derive_u); the only device memory a context owns, allocated on first use (aff_derived_u_ensure)
    float* derived_u = nullptr;
    int desc_form = AFFNET_DESC_FORM_F43_CONV1;     // fused exact-fp32 HardNet trunk (affnet_set_desc_form): stride-2 layers in the direct form, or as polyphase Winograd F(2x2, 2x2), or that with conv3 as F(4x4, 3x3), or that with conv5 as F(4x4, 3x3) in a kernel of its own, or that with conv1 as F(4x4, 3x3) streamed with conv0
    ~affnet_ctx() {
        if (derived_u) (void)hipFree(derived_u);
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (graph) (void)hipGraphDestroy(graph);
        for (auto& e : prof_ev) (void)hipEventDestroy(e);
    }
};

// Every entry point that launches work makes the context's device current for the duration of the call and restores
// the caller's device afterwards (a context is bound to ONE device, affnet_ctx_create; the caller's current device
// may be another one in a multi-GPU process).  Tolerates a host without a GPU (CPU-side argument checks still run).
struct AffDeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit AffDeviceGuard(const affnet_ctx* ctx) {
        if (!ctx) return;
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; return; }
        if (prev != ctx->device) switched = hipSetDevice(ctx->device) == hipSuccess;
    }
    ~AffDeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    AffDeviceGuard(const AffDeviceGuard&) = delete;
    AffDeviceGuard& operator=(const AffDeviceGuard&) = delete;
};
#define AFF_DEVICE(ctx) AffDeviceGuard aff_device_guard_(ctx)

#define PROF_RING 256
#define PROF_EVENTS (AFFNET_PROFILE_STAGES + 2)   // 9 stage boundaries + end-of-detector (index 9)

#define AFF_HIP(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return aff_fail(ctx, AFFNET_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                                   \
    } while (0)

#define AFF_LAUNCH_CHECK(ctx)                                                                      \
    do {                                                                                           \
        hipError_t e_ = hipGetLastError();                                                         \
        if (e_ != hipSuccess)                                                                      \
            return aff_fail(ctx, AFFNET_ERR_HIP, "kernel launch failed: %s (%s:%d)",                \
                            hipGetErrorString(e_), __FILE__, __LINE__);                            \
    } while (0)

// up to 8 device-side fills in one launch (aff_zero_multi_async)
struct AffZeroSegs {
    unsigned char* p[8];
    size_t bytes[8];
    int n = 0;
    bool overflow = false;   // more than 8 segments were added: aff_zero_multi_async refuses the launch instead of leaving an area uncleared
    void add(void* ptr, size_t nbytes) {
        if (!ptr || !nbytes) return;
        if (n >= 8) { overflow = true; return; }
        p[n] = (unsigned char*)ptr; bytes[n] = nbytes; ++n;
    }
};

static inline size_t aff_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
static inline int aff_cdiv(int a, int b) { return (a + b - 1) / b; }

// One row {row1, n1, row2, n2} of the pair table of the *_many calls (include/affnet_hip.h), tested against the buffers' row counts and the
// launch's caps before anything is loaded through it.  false: out of range (the row's fields are then not to be used).
struct AffPairRow { int row1, n1, row2, n2; };
__device__ __forceinline__ bool aff_pair_row(const int32_t* __restrict__ pairs, int p, int rows1, int rows2, int n1_max, int n2_max, AffPairRow& r) {
    r.row1 = pairs[4 * (size_t)p]; r.n1 = pairs[4 * (size_t)p + 1]; r.row2 = pairs[4 * (size_t)p + 2]; r.n2 = pairs[4 * (size_t)p + 3];
    return r.row1 >= 0 && r.n1 >= 0 && r.row2 >= 0 && r.n2 >= 0 && (long long)r.row1 + r.n1 <= rows1 && (long long)r.row2 + r.n2 <= rows2 &&
           r.n1 <= n1_max && r.n2 <= n2_max;
}

// Level pointers of the pyramid of image 0 in the workspace (+ img_stride floats per further image of the batch).
struct PyrTable {
    const float* lvl[AFFNET_MAX_OCTAVES][AFFNET_MAX_LEVELS];
    int h[AFFNET_MAX_OCTAVES], w[AFFNET_MAX_OCTAVES];
    int n_octaves, n_levels;
    size_t img_stride;
};

// Constants of the denormalisation + pyramid-level choice of one row (device helpers: shape_filter.h); filled by aff_denorm_sel_fill
struct LevelTable { double sig[AFFNET_MAX_OCTAVES * AFFNET_MAX_LEVELS]; int n_oct, n_lvl; };
struct DenormSel {           // per-launch constants + outputs (pointers of image 0, rows of image b at b * n_max); out_px == NULL: not fused
    float* out_px; int32_t* ids; float* lafs_norm;
    float c_a, c_x, c_y, ps, ca, cx, cy;
    LevelTable lt;
};

// ---- internal interface: every function that crosses a file boundary -----------------------------------------------------
// Each non-static aff_* function of the library is declared HERE, once, under the file that defines it.  The .hip files carry no
// declarations of their own, so a definition and its callers are compiled against the same prototype.  No default arguments.
// The plain types and constants that only such prototypes and the kernels behind them share come first.

// the 32x32-patch CNNs: cnn32.hip (host layer), cnn_trunk.h (trunk kernels, instantiated per net in cnn_trunk_*.hip), cnn_heads.hip
// floats of head partials per patch that an AffNet / OriNet trunk leaves for its finish kernel ([wave][4] / [wave][18])
#define HEAD_PART_AFF 32
#define HEAD_PART_ORI 144
// HardNet head GEMM (cnn_heads.hip): K quarters per patch block, K chunk per LDS slab and its row stride
#define HEAD_KSPLIT 4
#define HEAD_KC 128
#define HEAD_AS (HEAD_KC + 4)    // row stride: 16-byte aligned rows

struct PyrSrc {            // pyramid sampling source (fused sampler)
    PyrTable t;            // the samplers' level table
    float base[32];        // affine_grid base coordinates for PS = 32
};

struct CnnArgs {
    const float* packed;
    NetOffsets off;
    const float* wino_u;   // the net's region of derived weights (aff_derive_u in front of this launch), NULL for a form that reads none.  Exact OriNet, Winograd AffNet:
                           // Wino16 (U = G g G^T of conv1, conv3 and conv5, the polyphase U of conv2 and conv4 behind them); HardNet form 1: Poly32 (the polyphase U of
                           // conv2 and conv4); form 2: behind it at F43::BASE the F(4x4, 3x3) U of conv1 / conv3 (F43)
    const int32_t* reeval; // direct AffNet trunk behind the Winograd one (shape form 1): per-row flags of the margin rule [image * n_max + row], a workgroup whose flag is 0 returns at once; NULL = every row
    const float* patches;  // (n,32,32) or NULL -> sample from the pyramid
    const float* lafs;     // normalised LAFs when sampling
    const int32_t* ids;    // (octave, level, *) when sampling
    const int32_t* count;
    int n_max;
    float* out;            // AffNet/OriNet: (n,2,2); HardNet: trunk output (n,8192)
    int dbg_layer;         // >= 0: dump activations after this trunk layer of patch 0 and exit
    int s3_alt;            // tuning variant bits of the split-operand trunks (affnet_debug_split3_variant): bit 0 = the two waves of a SIMD alternate at the higher priority inside the HardNet loops
    float* dbg_out;
    unsigned long long* dbg_time;   // != NULL: s_memtime stamps [patch][wave][32] at the phase boundaries (tuning aid)
    // Row window [row_begin, row_begin + gridDim.x) of every image, and the lazy-evaluation predicate of the fused pipeline: when
    // skip_cnt != NULL the launch does nothing for an image whose detections are response-sorted (CNT_SEL_MODE == 1) and whose first
    // pass already produced skip_n survivors of the shape filter (CNT_SURVIVED1) - pipeline.hip, affnet_describe_detected.
    int row_begin;
    const int32_t* skip_cnt;
    int skip_n;
    // Shape-stage bookkeeping done by thread 0 of workgroup (0, image) of the AffNet trunk launches (each was a 5 us launch of its
    // own): shape_op 1 = first pass: survivor / evaluation counters = 0; 2 = second (lazy) pass: freeze the first pass's survivor
    // count (CNT_SURVIVED1) for the predicate of the finish + filter kernel that follows this launch.  The trunk workgroups
    // themselves test CNT_SURVIVED, which nothing changes while a trunk launch runs.
    int32_t* shape_cnt;
    int shape_op;
};

// Forms of a trunk: the values of cnn32_trunk_kernel<KIND, NW, STAMPS, S3>'s last template argument, part of the kernels' names.  What a (net, form) pair runs: TrunkTraits (cnn_trunk.h); which pairs are built: aff_trunk_kernel (cnn32.hip).
constexpr int TRUNK_EXACT = 0;       // exact fp32.  AffNet: every layer direct; OriNet: conv1 / conv3 / conv5 Winograd F(2x2, 3x3), conv2 / conv4 polyphase; HardNet: descriptor form 0
constexpr int TRUNK_WINO = 1;        // exact fp32.  AffNet: conv1 / conv3 / conv5 Winograd (shape form 1); HardNet: TRUNK_EXACT with conv2 / conv4 polyphase (descriptor form 1)
constexpr int TRUNK_SPLIT2 = 2;      // two fp16 terms per operand (AFFNET_ARITH_FP32_SPLIT2H); the value is the number of terms
constexpr int TRUNK_SPLIT3 = 3;      // three bf16 terms per operand (AFFNET_ARITH_FP32_SPLIT3); the value is the number of terms
constexpr int TRUNK_WINO_F43 = 4;    // exact fp32, HardNet: TRUNK_WINO with conv3 as Winograd F(4x4, 3x3) (descriptor form 2)
constexpr int TRUNK_WINO_POLY = 5;   // exact fp32, AffNet: TRUNK_WINO with conv2 / conv4 polyphase (shape form 2)
constexpr int TRUNK_WINO_F43_C5 = 6; // exact fp32, HardNet: TRUNK_WINO_F43 cut behind conv4, whose tensor goes to HBM; conv5 follows as hardnet_conv5_f43_kernel, four patches per workgroup (descriptor form 3)
constexpr int TRUNK_WINO_F43_C1 = 7; // exact fp32, HardNet: TRUNK_WINO_F43_C5 with conv0 + conv1 streamed over conv1's K, conv1 as Winograd F(4x4, 3x3) (descriptor form 4)
constexpr int TRUNK_FORMS = 8;

// the lazy-evaluation predicate above, for the trunk and finish kernels
__device__ __forceinline__ bool lazy_skip(const int32_t* skip_cnt, int skip_n, int image, int which = CNT_SURVIVED1) {
    if (!skip_cnt) return false;
    const int32_t* c = skip_cnt + (size_t)image * CNT_TOTAL;
    return c[CNT_SEL_MODE] == 1 && c[which] >= skip_n;
}

struct ShapeFuse {           // finish + shape filter in one kernel (pointers of image 0; strides like shape_filter_kernel)
    const float* resp; const float* lafs; float* key; int32_t* good; int32_t* cnt;
};

// One CNN call: trunk launch + the net's finish stage.  Callers set the fields they mean by name; the rest keep these defaults.
struct CnnCall {
    int kind = -1;                                                   // AFFNET_NET_AFFNET / _ORINET / _HARDNET
    const float* packed = nullptr;
    const float* patches = nullptr;                                  // (n,32,32), or NULL: sample from the pyramid with lafs / ids
    const float* lafs = nullptr; const int32_t* ids = nullptr;
    const int32_t* count = nullptr; int n_max = 0;
    float* out = nullptr; float* scratch = nullptr;
    hipStream_t st = nullptr;
    int dbg_layer = -1; float* dbg_out = nullptr;                    // layer >= 0: dump this trunk layer of patch 0, no finish stage
    bool mark_head = false;                                          // stage mark 7 between trunk and head (affnet_describe_detected)
    int row_begin = 0, row_count = -1;                               // row window of every image; -1 = up to n_max
    const int32_t* skip_cnt = nullptr; int skip_n = 0;               // lazy-evaluation predicate (see CnnArgs)
    const ShapeFuse* fuse = nullptr; int shape_op = 0;               // AffNet: shape filter in the finish kernel, counter bookkeeping in the trunk
    int desc_form = AFFNET_DESC_FORM_DIRECT;                         // HardNet, exact fp32: AFFNET_DESC_FORM_* - 1: conv2 / conv4 as polyphase Winograd F(2x2, 2x2), 2: conv3 as F(4x4, 3x3) besides, 3: conv5 as F(4x4, 3x3) in a kernel of its own besides, 4: conv0 + conv1 streamed, conv1 as F(4x4, 3x3) besides
    int wino_reeval = 0;                                             // AffNet, exact fp32, fused filter: 1 / 2 = Winograd trunk of that shape form, margin rule, direct trunk on the flagged rows; 0 = direct only
    float* rot_lafs = nullptr; const DenormSel* denorm = nullptr;    // OriNet: LAF <- LAF * R in the finish kernel (+ denormalisation and level choice)
};

// kernel of one trunk instantiation
typedef void (*TrunkKernel)(CnnArgs, PyrSrc);

// hardnet_conv5_f43_kernel (hardnet_conv5_f43.hip): conv5 of HardNet's descriptor form 3 over the rows [row_begin, row_end) of every image, in place in the trunk's 32 KB slots
struct Conv5Args {
    float* io;                       // slot of row r of image b at io + (b * n_max + r) * 8192: conv4's tensor [c / 4][pixel][4] in, conv5's [pixel][channel] out
    const float* U;                  // derived F(4x4, 3x3) weights of layer 5 (DerivedU: F43C5), [xi (36)][8][kq][128][4]
    const float* bias;               // conv5's bias [128]
    const int32_t* count; int n_max; // rows per image as the trunk reads them (count may be NULL)
    int row_begin, row_end;
    const int32_t* skip_cnt; int skip_n;   // the trunk's lazy-evaluation predicate
    unsigned long long* dbg_time;    // stamped instantiation: stamps 24 .. 31 of every wave in the record of the group's first patch (the trunk writes 0 .. 23 of the same record)
};

// One area of the workspace: THE table that affnet_ctx_create sizes the workspace from, affnet_bind_workspace takes its pointers from and
// affnet_probe_workspace_areas (debug.hip) reports - aff_ws_layout (context.hip) is the only place that knows the carve.
// parent < 0: a carve unit; units start on the library's alignment (aff_align), in table order, and tile the workspace.  parent >= 0: a view inside
// that unit (off is still from the workspace base); the views of a list unit lie back to back, the views of the CNN scratch overlap (a union).
enum { AFF_WS_F32 = 0, AFF_WS_I32 = 1, AFF_WS_U8 = 2, AFF_WS_RECORDS = 3, AFF_WS_GROUP = 4 };   // = AFFNET_WS_* (include/affnet_hip_probes.h)
struct AffWsArea {
    const char* name;
    size_t off, bytes;
    int kind;              // AFF_WS_*; GROUP: a unit of mixed kinds, described by its views
    int cleared;           // 1: the detector half of every fused call clears it (detect.hip: detect_candidates / clear_outputs)
    int parent;
};
#define AFF_WS_MAX_AREAS 64
// The detector's replay of the octaveMap (detect.hip): up to 3 detection levels run as resolve_count / resolve_apply from RawMax::prev, with no octaveMap in
// memory; more levels run level_resolve_kernel on the octaveMap area, which the call then clears.  One predicate for the detector and for the ledger's flag.
static inline bool aff_detect_two_pass(const affnet_config& c) { return c.levels_per_octave - 2 <= 3; }

// context.hip
int aff_fail(affnet_ctx* ctx, int code, const char* fmt, ...);
// the areas of ctx's workspace from its capacities, strides and config (set by affnet_ctx_create before the call) -> out[AFF_WS_MAX_AREAS]; returns their number,
// or -1 when the table holds more than AFF_WS_MAX_AREAS (nothing is written past the array)
int aff_ws_layout(const affnet_ctx* ctx, AffWsArea* out);
// Device-side fills and copies as plain kernels of this library instead of hipMemsetAsync / hipMemcpyAsync: the runtime's blit
// path shares per-queue state with captured graph nodes (replaying a captured graph after eager null-stream memsets faulted on
// ROCm 7.2), and a kernel of our own is also what a stream capture records most cheaply.
int aff_zero_async(affnet_ctx* ctx, void* dst, size_t bytes, hipStream_t st);
int aff_zero_multi_async(affnet_ctx* ctx, const AffZeroSegs& z, hipStream_t st);
int aff_copy_async(affnet_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t st);
// rows x width_bytes, row r at dst + r * dpitch / src + r * spitch (all multiples of 4 bytes)
int aff_copy2d_async(affnet_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes, size_t rows, hipStream_t st);
// base[ps] = (linspace(-1,1,ps) * (ps-1)) / ps exactly as torch does on CPU (linspace = fma(step, i, start) /
// fma(-step, ps-1-i, end); verified bit-for-bit in tests/test_host_mirror.py)
void aff_base_grid(int ps, float* base);

// pipeline.hip: record stage boundary `idx` of the current call (no-op when disabled)
void aff_prof_mark(affnet_ctx* ctx, int idx, hipStream_t st);

// detect.hip: the two detector halves; candidates of the one-pass form go to the context's internal detection list
int aff_detect_impl(affnet_ctx* ctx, const float* d_responses, float* d_resp, float* d_lafs, int32_t* d_ids, int32_t* d_count, void* stream);
int aff_detect_onepass_impl(affnet_ctx* ctx, const float* d_packed_fullconv, const float* d_responses, hipStream_t st);

// fullconv.hip: dense AffNetFastFullConv maps of B images of one size
int aff_fullconv_launch(affnet_ctx* ctx, const float* packed, const float* img, size_t img_stride, int h, int w, float* out, size_t out_stride,
                        float* scratch, size_t scratch_stride, int B, hipStream_t st);

// handcrafted.hip: hand-crafted slot fillers (AFFNET_HC_*)
int aff_handcrafted_launch(affnet_ctx* ctx, int kind, const float* patches, const float* lafs, const int32_t* ids, const int32_t* count,
                           int n_max, const float* h_weights, float* out, float* out_angle, hipStream_t st);

// laf_ops.hip: pyramid table of the samplers, selection of the shape stage, AffNet iterations > 1, denormalisation + level choice
void aff_fill_pyr_table(const affnet_ctx* ctx, PyrTable* t);
int aff_shape_select(affnet_ctx* ctx, const float* d_resp_in, const float* d_lafs_in, const int32_t* d_ids_in, const float* d_A,
                     const int32_t* d_count_in, float* d_resp_out, float* d_lafs_out, int32_t* d_ids_out, int32_t* d_count_out, hipStream_t st);
int aff_shape_iterate(affnet_ctx* ctx, const float* A, float* base, const float* lafs, const int32_t* count, int mode, float* lafs_out,
                      hipStream_t st);
void aff_denorm_sel_fill(affnet_ctx* ctx, int ps, float* d_lafs_px, int32_t* d_ids, float* d_lafs_norm, DenormSel* ds);
int aff_denorm_level_select(affnet_ctx* ctx, const float* d_lafs_norm_in, float* d_lafs_px, const int32_t* d_count, int n_max, int ps, int32_t* d_ids,
                            float* d_lafs_norm, hipStream_t st);

// cnn32.hip: the fused launches of affnet_describe_detected (AffNet + shape filter on a row window, OriNet + rotation, HardNet with
// the stage mark between trunk and head)
int aff_affnet_filter_rows(affnet_ctx* ctx, const float* packed, const float* resp, const float* lafs, const int32_t* ids, const int32_t* count,
                           float* out, float* scratch, int row_begin, int row_count, bool lazy, int shape_op, hipStream_t st);
int aff_orinet_rotate(affnet_ctx* ctx, const float* packed, float* lafs, const int32_t* ids, const int32_t* count, int n_max, float* out, float* scratch,
                      hipStream_t st, const DenormSel* denorm);
int aff_hardnet_forward_pyr_marked(affnet_ctx* ctx, const float* packed, const float* lafs, const int32_t* ids, const int32_t* count,
                                   int n_max, float* out, float* scratch, hipStream_t st);

// cnn32.hip: HardNet on a patch tensor in descriptor form `form` (1, 2, 3 or 4), for the probe library (the public patch-tensor calls run form 0); dbg_layer >= 0: layer dump of patch 0
int aff_hardnet_poly_patches(affnet_ctx* ctx, const float* packed, const float* patches, int n, float* out, float* scratch, int dbg_layer, hipStream_t st,
                             int form = AFFNET_DESC_FORM_POLYPHASE);
// cnn32.hip: the instantiation of net `kind` in trunk form `form` (TRUNK_*) [phase stamps]; NULL for a pair that is not built
TrunkKernel aff_trunk_kernel(int kind, int form, bool stamps);
// cnn32.hip: one trunk launch of `c` on `grid` = (rows, images), derived weights in front.  wino: AffNet's Winograd instantiation of shape form 1 / 2, 0 = none; reeval: the margin rule's flags for the direct AffNet trunk behind it; shape_op: see CnnArgs
int aff_trunk_launch(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, dim3 grid, int wino, const int32_t* reeval, int shape_op);

// cnn_trunk_*.hip: the unit's instantiations, by trunk form [phase stamps]; NULL for a form the unit does not build.  Called by aff_trunk_kernel only.
TrunkKernel aff_trunk_affnet(int form, bool stamps), aff_trunk_affnet_poly(int form, bool stamps), aff_trunk_orinet(int form, bool stamps);
TrunkKernel aff_trunk_hardnet(int form, bool stamps), aff_trunk_hardnet_poly(int form, bool stamps), aff_trunk_hardnet_f43(int form, bool stamps);
TrunkKernel aff_trunk_hardnet_c5(int form, bool stamps), aff_trunk_hardnet_c1(int form, bool stamps);
// hardnet_conv5_f43.hip: conv5 of descriptor form 3 behind its trunk launch, on `groups` groups of four rows of B images
int aff_hardnet_conv5_f43(affnet_ctx* ctx, const Conv5Args& a, int groups, int B, bool stamps, hipStream_t st);
// derive_u.hip: allocate the context's buffer of derived weights (before a stream capture begins: no allocation inside one)
int aff_derived_u_ensure(affnet_ctx* ctx);
// derive_u.hip: derive what trunk form `form` of net `kind` reads from `packed` into that net's region of the context's buffer; *region = it (CnnArgs::wino_u), or NULL and no launch for a form that reads none
int aff_derive_u(affnet_ctx* ctx, int kind, int form, const float* packed, const NetLayout& L, hipStream_t st, const float** region);

// cnn_heads.hip: what cnn_launch runs behind a trunk launch: AffNet / OriNet finish kernel on `rows` rows of the window of B images, HardNet
// head GEMM + finish kernel over all rows
int aff_finish_affnet(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int rows, int B);
// shape form 1: the margin rule (shape_filter.h) on the Winograd trunk's partials of the window's evaluated rows -> flags[image * n_max + row], CNT_AFF_REEVAL
int aff_margin_affnet(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int rows, int B, int32_t* flags);
int aff_finish_orinet(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int rows, int B);
int aff_hardnet_head(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, int B);

// match.hip: out[r] = |x[r]|^2 of n rows (n <= 0: no launch) by the matcher's own kernel - the one reduction behind every distance of the matcher
// and of the descriptor index (knn.hip, ivf.hip), which is what makes their distances equal bit for bit
void aff_sqnorm_launch(hipStream_t st, const float* x, int n, int dim, float* out);
// match.hip: the same per pair of a *_many call (sqnorm_many_kernel): a_sq (P, n1_max) and b_sq (P, n2_max) of the pairs' segments; a pair out
// of range or with an empty side gets neither (no distance of such a pair is ever formed)
void aff_sqnorm_many_launch(hipStream_t st, const float* desc1, int rows1, const float* desc2, int rows2, int dim, const int32_t* pairs, int n_pairs,
                            int n1_max, int n2_max, float* a_sq, float* b_sq);
// knn.hip: the n_lists partial lists (n1, n_lists, k) of every row -> its k neighbours (knn_merge_kernel; the chunks of affnet_knn, the probed cells of affnet_ivf_search)
void aff_knn_merge_launch(hipStream_t st, const float* part_d, const int32_t* part_i, int n1, int n_lists, int k, float* out_d, int32_t* out_i);
// knn.hip: the same per pair of a *_many call (knn_merge_pairs_kernel): side 0 merges each pair's n1 rows (pitch n1_max), side 1 its n2 rows (pitch
// n2_max), of pair-major partial lists (P, pitch, n_lists, k) into (P, pitch, k); pairs out of range or with n1 == 0 and rows at or beyond a pair's
// count are neither read nor written
void aff_knn_merge_pairs_launch(hipStream_t st, const float* part_d, const int32_t* part_i, const int32_t* pairs, int n_pairs, int rows1, int rows2,
                                int n1_max, int n2_max, int side, int n_lists, int k, float* out_d, int32_t* out_i);
// knn_q8.hip: the same for int lists (knn_q8_merge_kernel; the chunks of affnet_knn_q8, the probed cells of affnet_ivf_search_q8): partial d2 and rows
// (n1, n_lists, k), unfilled slots hold row -1 -> d2, sqrtf((float)d2) / scale and rows (n1, k), unfilled slots (INT32_MAX, +inf, -1)
void aff_knn_q8_merge_launch(hipStream_t st, const int32_t* part_d, const int32_t* part_i, int n1, int n_lists, int k, float scale, int32_t* out_d2,
                             float* out_f, int32_t* out_i);

// ---- host helpers of the descriptor index's searches (knn.hip, knn_q8.hip, ivf.hip) ---------------
// the rows [skip_row, skip_row + skip_n) that are no candidates, as [lo, hi) inside [0, n2); lo >= hi: no skip
struct AffSkip { int lo, hi; };
static inline AffSkip aff_skip_range(int skip_row, int skip_n, int n2) {
    const long long lo64 = skip_row < 0 ? 0 : skip_row, hi64 = (long long)skip_row + skip_n;
    return {(int)(lo64 < n2 ? lo64 : n2), (int)(hi64 < 0 ? 0 : (hi64 < n2 ? hi64 : n2))};
}

// capacity of the register lists (topk.h) that hold k candidates: the kernels are built for 1, 2, 4 and 8
static inline int aff_topk_cap(int k) { return k == 1 ? 1 : (k == 2 ? 2 : (k <= 4 ? 4 : 8)); }
// f(std::integral_constant<int, aff_topk_cap(k)>()): the capacity as a compile-time constant, for the kernels' template argument
template <typename F>
static inline void aff_topk_dispatch(int k, F f) {
    switch (aff_topk_cap(k)) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}

// Chunks of the database a search of `row_blocks` blocks of query rows is cut into (grid = row blocks x chunks): enough for workgroups_per_cu
// workgroups on every CU (256 CUs without a context, or where the count cannot be read), no chunk below min_units of the `units` the tile loop
// walks, at most max_chunks, at least 1.
static inline int aff_chunk_choice(const affnet_ctx* ctx, long long row_blocks, long long units, int workgroups_per_cu, int min_units, int max_chunks) {
    int cus = 256;
    if (ctx) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && v > 0) cus = v;
        else (void)hipGetLastError();
    }
    const long long want = ((long long)workgroups_per_cu * cus + row_blocks - 1) / row_blocks, most = units / min_units;
    long long nc = want < most ? want : most;
    if (nc > max_chunks) nc = max_chunks;
    return nc < 1 ? 1 : (int)nc;
}

// ---- sampler math shared by laf_ops.hip, handcrafted.hip and cnn_trunk.h --------------------------
// LDS-staged footprint of one patch (north_star: "coalesced HBM reads and LDS-staged image tiles"): the affine frame of a PS x PS
// patch covers an axis-aligned box of the level image; when that box is small its rows are loaded once with coalesced row-segment
// loads (zeros outside the image = grid_sample's zero padding) and the four bilinear taps of every sample come from LDS.  The
// arithmetic of a sample is untouched (same weights, same fmaf chain), so staged and direct sampling are bit-identical.
struct AffTile {
    int x0, y0, tw, th;      // box origin in level pixels (may be negative), width / height; tw == 0: not staged
};

// Box that contains every tap of the patch (1-px margin for the fp32 round trip of the coordinates); staged iff it fits `cap` floats
// and is small enough that loading it costs fewer requests than the 4 * ps * ps gathers it replaces.
__device__ __forceinline__ AffTile aff_tile_box(float t00, float t01, float t02, float t10, float t11, float t12, int ps, int cap) {
    const float um = (float)(ps - 1) / (float)ps;
    const float hx = (fabsf(t00) + fabsf(t01)) * um, hy = (fabsf(t10) + fabsf(t11)) * um;
    const float cx = t02 - 0.5f, cy = t12 - 0.5f;
    AffTile t;
    t.tw = 0; t.th = 0; t.x0 = 0; t.y0 = 0;
    if (!(hx < 4096.0f && hy < 4096.0f && fabsf(cx) < 1.0e6f && fabsf(cy) < 1.0e6f)) return t;     // also rejects NaN / inf frames
    const int x0 = (int)floorf(cx - hx) - 1, x1 = (int)floorf(cx + hx) + 2;
    const int y0 = (int)floorf(cy - hy) - 1, y1 = (int)floorf(cy + hy) + 2;
    const int tw = x1 - x0 + 1, th = y1 - y0 + 1;
    if (tw * th > cap || tw * th > 2 * ps * ps) return t;
    t.x0 = x0; t.y0 = y0; t.tw = tw; t.th = th;
    return t;
}

// Cooperative load of the box into LDS (NTHR threads; the caller synchronises afterwards).
template <int NTHR>
__device__ __forceinline__ void aff_tile_load(float* tile, const AffTile t, const float* __restrict__ img, int h, int w, int tid) {
    const int n = t.tw * t.th;
    for (int i = tid; i < n; i += NTHR) {
        const int ty = i / t.tw, tx = i - ty * t.tw;
        const int gy = t.y0 + ty, gx = t.x0 + tx;
        tile[i] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? img[(size_t)gy * w + gx] : 0.0f;
    }
}

// Device: one bilinear sample.  Follows LAF.py:313-324 + F.affine_grid + F.grid_sample
// (align_corners=False, zeros padding) operation by operation in fp32:
//   theta = LAF * [[m,m,w],[m,m,h]];  g = fma(1,t02, fma(v,t01, u*t00));
//   gn = 2*g/size - 1;  i = fma(gn+1, size/2, -0.5);  out = fma chain nw,ne,sw,se.
__device__ __forceinline__ float aff_sample_bilinear(const float* __restrict__ img, int h, int w,
                                                     float t00, float t01, float t02, float t10,
                                                     float t11, float t12, float u, float v) {
    float gx = fmaf(1.0f, t02, fmaf(v, t01, u * t00));
    float gy = fmaf(1.0f, t12, fmaf(v, t11, u * t10));
    const float fw = (float)w, fh = (float)h;
    gx = 2.0f * gx / fw - 1.0f;
    gy = 2.0f * gy / fh - 1.0f;
    const float ix = fmaf(gx + 1.0f, fw * 0.5f, -0.5f);
    const float iy = fmaf(gy + 1.0f, fh * 0.5f, -0.5f);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float x1f = x0f + 1.0f, y1f = y0f + 1.0f;
    const float wx1 = ix - x0f, wx0 = x1f - ix, wy1 = iy - y0f, wy0 = y1f - iy;
    const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
    // float -> int after range clamping so that huge coordinates cannot overflow
    const float cx0 = fminf(fmaxf(x0f, -2.0f), fw + 1.0f), cy0 = fminf(fmaxf(y0f, -2.0f), fh + 1.0f);
    const int x0 = (int)cx0, y0 = (int)cy0, x1 = x0 + 1, y1 = y0 + 1;
    const bool xin0 = (x0 >= 0) & (x0 < w), xin1 = (x1 >= 0) & (x1 < w);
    const bool yin0 = (y0 >= 0) & (y0 < h), yin1 = (y1 >= 0) & (y1 < h);
    const float vnw = (xin0 & yin0) ? img[(size_t)y0 * w + x0] : 0.0f;
    const float vne = (xin1 & yin0) ? img[(size_t)y0 * w + x1] : 0.0f;
    const float vsw = (xin0 & yin1) ? img[(size_t)y1 * w + x0] : 0.0f;
    const float vse = (xin1 & yin1) ? img[(size_t)y1 * w + x1] : 0.0f;
    return fmaf(vse, se, fmaf(vsw, sw, fmaf(vne, ne, vnw * nw)));
}

// Same sample with the four taps taken from a staged box (zeros are already in the tile for pixels outside the image).  A tap
// outside the box (cannot happen for a box from aff_tile_box; guarded anyway) falls back to the predicated global load.
__device__ __forceinline__ float aff_sample_bilinear_tile(const float* tile, const AffTile tl, const float* __restrict__ img, int h, int w,
                                                          float t00, float t01, float t02, float t10, float t11, float t12, float u, float v) {
    float gx = fmaf(1.0f, t02, fmaf(v, t01, u * t00));
    float gy = fmaf(1.0f, t12, fmaf(v, t11, u * t10));
    const float fw = (float)w, fh = (float)h;
    gx = 2.0f * gx / fw - 1.0f;
    gy = 2.0f * gy / fh - 1.0f;
    const float ix = fmaf(gx + 1.0f, fw * 0.5f, -0.5f);
    const float iy = fmaf(gy + 1.0f, fh * 0.5f, -0.5f);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float x1f = x0f + 1.0f, y1f = y0f + 1.0f;
    const float wx1 = ix - x0f, wx0 = x1f - ix, wy1 = iy - y0f, wy0 = y1f - iy;
    const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
    const float cx0 = fminf(fmaxf(x0f, -2.0f), fw + 1.0f), cy0 = fminf(fmaxf(y0f, -2.0f), fh + 1.0f);
    const int x0 = (int)cx0, y0 = (int)cy0;
    const int lx = x0 - tl.x0, ly = y0 - tl.y0;
    float vnw, vne, vsw, vse;
    if (lx >= 0 && ly >= 0 && lx + 1 < tl.tw && ly + 1 < tl.th) {
        const float* p = tile + ly * tl.tw + lx;
        vnw = p[0]; vne = p[1]; vsw = p[tl.tw]; vse = p[tl.tw + 1];
    } else {
        const int x1 = x0 + 1, y1 = y0 + 1;
        const bool xin0 = (x0 >= 0) & (x0 < w), xin1 = (x1 >= 0) & (x1 < w);
        const bool yin0 = (y0 >= 0) & (y0 < h), yin1 = (y1 >= 0) & (y1 < h);
        vnw = (xin0 & yin0) ? img[(size_t)y0 * w + x0] : 0.0f;
        vne = (xin1 & yin0) ? img[(size_t)y0 * w + x1] : 0.0f;
        vsw = (xin0 & yin1) ? img[(size_t)y1 * w + x0] : 0.0f;
        vse = (xin1 & yin1) ? img[(size_t)y1 * w + x1] : 0.0f;
    }
    return fmaf(vse, se, fmaf(vsw, sw, fmaf(vne, ne, vnw * nw)));
}
