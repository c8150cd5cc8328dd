// Host layer of the 32x32-patch CNNs (AffNetFast / OriNetFast / HardNet): argument checks, the trunk launch and every entry point built on it.
// Every entry point fills a CnnCall and cnn_launch runs cnn_check -> aff_trunk_launch -> aff_finish_affnet / aff_finish_orinet / aff_hardnet_head.
// No device code here: the trunk kernels are cnn_trunk.h, instantiated per net in cnn_trunk_affnet.hip / _orinet.hip / _hardnet.hip (design:
// DESIGN.md section 4 and the head of cnn_trunk.h); the finish and head kernels with their launchers are cnn_heads.hip.  CnnCall, CnnArgs and the
// prototypes that cross files are in common.h.
#include "common.h"

static void aff_fill_pyr_src(const affnet_ctx* ctx, PyrSrc* s) {
    memset(s, 0, sizeof(*s));                            // no workspace bound (patch-tensor calls): an all-zero table
    if (ctx->ws) aff_fill_pyr_table(ctx, &s->t);
    aff_base_grid(32, s->base);
}

// Argument checks, in this order.  *rows = rows per image to launch; 0 with AFFNET_OK = nothing to do.
static int cnn_check(affnet_ctx* ctx, const CnnCall& c, int* rows) {
    *rows = 0;
    if (c.kind < 0 || c.kind > 2) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: unknown net kind %d", c.kind);
    if (!c.packed || !c.out || c.n_max < 0 || (!c.patches && (!c.lafs || !c.ids))) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: null argument");
    if (!c.patches && !ctx->ws) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: sampling from the pyramid needs a bound workspace");
    if (c.dbg_layer < 0 && !c.scratch)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: d_scratch is required (HardNet n*(8192+512) floats, AffNet / OriNet n*144 floats)");
    if (c.dbg_layer >= 0 && ctx->arith != AFFNET_ARITH_FP32_MFMA)     // the split trunks have no per-layer dump: the exact kernel would answer
        return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: layer dumps exist for AFFNET_ARITH_FP32_MFMA only (context is in arithmetic mode %d)", ctx->arith);
    if (c.n_max == 0) return AFFNET_OK;
    if (c.kind == AFFNET_NET_HARDNET && c.n_max > 65535)
        return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: n_max=%d (HardNet head: max 65535 rows per image)", c.n_max);
    const int row_count = c.row_count < 0 ? c.n_max - c.row_begin : c.row_count;
    if (c.row_begin < 0 || row_count < 0 || c.row_begin + row_count > c.n_max) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: bad row window");
    *rows = row_count;
    return AFFNET_OK;
}

// The built instantiations, by (net, trunk form): the unit that holds each (the units are separate for the inliner's sake, see their heads)
TrunkKernel aff_trunk_kernel(int kind, int form, bool stamps) {
    typedef TrunkKernel (*Unit)(int, bool);
    static_assert(AFFNET_NET_AFFNET == 0 && AFFNET_NET_ORINET == 1 && AFFNET_NET_HARDNET == 2 && TRUNK_EXACT == 0 && TRUNK_WINO == 1 && TRUNK_SPLIT2 == 2 && TRUNK_SPLIT3 == 3 &&
                  TRUNK_WINO_F43 == 4 && TRUNK_WINO_POLY == 5 && TRUNK_WINO_F43_C5 == 6 && TRUNK_WINO_F43_C1 == 7 && TRUNK_FORMS == 8, "order of the table");
    static const Unit unit[3][TRUNK_FORMS] = {{aff_trunk_affnet, aff_trunk_affnet, aff_trunk_affnet, aff_trunk_affnet, nullptr, aff_trunk_affnet_poly, nullptr, nullptr},
                                              {aff_trunk_orinet, nullptr, aff_trunk_orinet, aff_trunk_orinet, nullptr, nullptr, nullptr, nullptr},
                                              {aff_trunk_hardnet, aff_trunk_hardnet_poly, aff_trunk_hardnet, aff_trunk_hardnet, aff_trunk_hardnet_f43, nullptr, aff_trunk_hardnet_c5, aff_trunk_hardnet_c1}};
    if (kind < 0 || kind > 2 || form < 0 || form >= TRUNK_FORMS || !unit[kind][form]) return nullptr;
    return unit[kind][form](form, stamps);
}

int aff_trunk_launch(affnet_ctx* ctx, const CnnCall& c, const NetLayout& L, dim3 grid, int wino, const int32_t* reeval, int shape_op) {
    // the trunk form, once: the split forms follow the context's arithmetic; exact AffNet runs the Winograd form asked for (wino = shape form 1 / 2), exact HardNet the call's descriptor form
    int form = TRUNK_EXACT;
    if (ctx->arith != AFFNET_ARITH_FP32_MFMA) form = ctx->arith == AFFNET_ARITH_FP32_SPLIT2H ? TRUNK_SPLIT2 : TRUNK_SPLIT3;
    else if (c.kind == AFFNET_NET_AFFNET && wino) form = wino == 2 ? TRUNK_WINO_POLY : TRUNK_WINO;
    else if (c.kind == AFFNET_NET_HARDNET && c.desc_form != AFFNET_DESC_FORM_DIRECT)
        form = c.desc_form == AFFNET_DESC_FORM_F43_CONV1 ? TRUNK_WINO_F43_C1 : (c.desc_form == AFFNET_DESC_FORM_F43_CONV5 ? TRUNK_WINO_F43_C5 : (c.desc_form == AFFNET_DESC_FORM_F43 ? TRUNK_WINO_F43 : TRUNK_WINO));
    const bool stamps = ctx->dbg_time || c.dbg_layer >= 0;             // the stamped instantiation: dbg_time or a layer dump (exact mode only, see cnn_check)
    const TrunkKernel kernel = aff_trunk_kernel(c.kind, form, stamps);
    if (!kernel) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32: no trunk kernel of net %d in form %d is built", c.kind, form);
    CnnArgs a;
    a.packed = c.packed; a.off = to_offsets(L, ctx->arith);            // the split copy of the active mode
    a.reeval = reeval;
    const int rc = aff_derive_u(ctx, c.kind, form, c.packed, L, c.st, &a.wino_u);
    if (rc) return rc;
    a.patches = c.patches; a.lafs = c.lafs; a.ids = c.ids; a.count = c.count; a.n_max = c.n_max;
    a.out = (c.dbg_layer < 0) ? c.scratch : c.out;      // trunk kernels: HardNet conv5 tensor / AffNet, OriNet head partials
    a.dbg_layer = c.dbg_layer; a.dbg_out = c.dbg_out; a.dbg_time = ctx->dbg_time;
    a.row_begin = c.row_begin; a.skip_cnt = c.skip_cnt; a.skip_n = c.skip_n;
    a.shape_cnt = (c.fuse && shape_op) ? c.fuse->cnt : nullptr; a.shape_op = shape_op;
    a.s3_alt = ctx->split3_variant;
    PyrSrc ps;
    aff_fill_pyr_src(ctx, &ps);
    hipLaunchKernelGGL(kernel, grid, dim3(512), 0, c.st, a, ps);
    AFF_LAUNCH_CHECK(ctx);
    if ((form == TRUNK_WINO_F43_C5 || form == TRUNK_WINO_F43_C1) && c.dbg_layer < 0) {
        // descriptor forms 3 / 4 are a pair: the trunk left conv4's tensor in the slots of a.out, hardnet_conv5_f43_kernel rewrites them in place - the same rows under the same predicate
        Conv5Args v;
        v.io = a.out; v.U = a.wino_u + F43C5::BASE; v.bias = c.packed + L.b_off[5];
        v.count = c.count; v.n_max = c.n_max; v.row_begin = c.row_begin; v.row_end = c.row_begin + (int)grid.x;
        v.skip_cnt = c.skip_cnt; v.skip_n = c.skip_n; v.dbg_time = ctx->dbg_time;
        return aff_hardnet_conv5_f43(ctx, v, aff_cdiv((int)grid.x, 4), (int)grid.y, stamps, c.st);
    }
    return AFFNET_OK;
}

static int cnn_launch(affnet_ctx* ctx, const CnnCall& c) {
    int rows;
    int rc = cnn_check(ctx, c, &rows);
    if (rc || rows == 0) return rc;
    const NetLayout L = net_layout(c.kind);
    const int B = c.patches ? 1 : ctx->B;                // patch tensors are single-"image"; pyramid sampling covers the batch
    // Shape forms 1 / 2 (CnnCall::wino_reeval; exact AffNet with the fused filter only; form 2 = form 1's trunk with conv2 / conv4 as polyphase Winograd): Winograd trunk on every row of the window (it does the counter work), the margin
    // rule on its partials (flags in the unused part of the scratch: 144 floats per row, 32 of them partials), the direct trunk on the flagged rows, which
    // overwrites their partials, then the finish + filter kernel as ever.  The same window, row counts and lazy predicate for all; nothing here depends on B or rows.
    const bool form1 = c.wino_reeval && c.kind == AFFNET_NET_AFFNET && c.fuse && c.dbg_layer < 0 && ctx->arith == AFFNET_ARITH_FP32_MFMA;
    rc = aff_trunk_launch(ctx, c, L, dim3(rows, B), form1 ? c.wino_reeval : 0, nullptr, c.shape_op);
    if (rc) return rc;
    if (form1) {
        int32_t* flags = reinterpret_cast<int32_t*>(c.scratch + (size_t)B * c.n_max * HEAD_PART_AFF);
        rc = aff_margin_affnet(ctx, c, L, rows, B, flags);
        if (rc) return rc;
        rc = aff_trunk_launch(ctx, c, L, dim3(rows, B), 0, flags, 0);
        if (rc) return rc;
    }
    if (c.dbg_layer < 0 && c.kind != AFFNET_NET_HARDNET) {
        rc = c.kind == AFFNET_NET_AFFNET ? aff_finish_affnet(ctx, c, L, rows, B) : aff_finish_orinet(ctx, c, L, rows, B);
        if (rc) return rc;
    }
    if (c.mark_head) aff_prof_mark(ctx, 7, c.st);
    if (c.dbg_layer < 0 && c.kind == AFFNET_NET_HARDNET) return aff_hardnet_head(ctx, c, L, B);
    return AFFNET_OK;
}

extern "C" int affnet_cnn32_forward(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patches, const int32_t* d_count,
                                    int n_max, float* d_out, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_patches) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32_forward: null argument");
    CnnCall c;
    c.kind = net_kind; c.packed = d_packed; c.patches = d_patches; c.count = d_count; c.n_max = n_max; c.out = d_out; c.scratch = d_scratch; c.st = (hipStream_t)stream;
    return cnn_launch(ctx, c);
}

extern "C" int affnet_cnn32_forward_pyr(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_lafs, const int32_t* d_ids,
                                        const int32_t* d_count, int n_max, float* d_out, float* d_scratch, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx) return AFFNET_ERR_INVALID;
    CnnCall c;
    c.kind = net_kind; c.packed = d_packed; c.lafs = d_lafs; c.ids = d_ids; c.count = d_count; c.n_max = n_max; c.out = d_out; c.scratch = d_scratch; c.st = (hipStream_t)stream;
    return cnn_launch(ctx, c);
}

// AffNet on a row window with the shape filter of every evaluated row fused into the finish kernel (key / good / survivor count in
// the context's stage buffers) and the shape-stage counter bookkeeping done by the trunk launch (shape_op: see CnnArgs); lazy = under
// the lazy-evaluation predicate.
int aff_affnet_filter_rows(affnet_ctx* ctx, const float* packed, const float* resp, const float* lafs, const int32_t* ids, const int32_t* count,
                           float* out, float* scratch, int row_begin, int row_count, bool lazy, int shape_op, hipStream_t st) {
    ShapeFuse sf;
    sf.resp = resp; sf.lafs = lafs; sf.key = ctx->st_key; sf.good = ctx->st_good; sf.cnt = ctx->cnt;
    CnnCall c;
    c.kind = AFFNET_NET_AFFNET; c.packed = packed; c.lafs = lafs; c.ids = ids; c.count = count; c.n_max = ctx->cap_pre; c.out = out; c.scratch = scratch; c.st = st;
    c.row_begin = row_begin; c.row_count = row_count;
    c.skip_cnt = lazy ? ctx->cnt : nullptr; c.skip_n = ctx->cfg.num_features;
    c.fuse = &sf; c.shape_op = shape_op;
    c.wino_reeval = ctx->shape_form;      // AFFNET_SHAPE_FORM_*: 0 = direct only
    return cnn_launch(ctx, c);
}

// OriNet with LAF <- LAF * R applied by the finish kernel (d_lafs rotated in place).
// denorm != NULL: the finish kernel also denormalises the rotated frame, chooses its pyramid level and writes the re-normalised frame (aff_denorm_level_select's
// work, one launch less per call).
int aff_orinet_rotate(affnet_ctx* ctx, const float* packed, float* lafs, const int32_t* ids, const int32_t* count, int n_max, float* out, float* scratch,
                      hipStream_t st, const DenormSel* denorm) {
    CnnCall c;
    c.kind = AFFNET_NET_ORINET; c.packed = packed; c.lafs = lafs; c.ids = ids; c.count = count; c.n_max = n_max; c.out = out; c.scratch = scratch; c.st = st;
    c.rot_lafs = lafs; c.denorm = denorm;
    return cnn_launch(ctx, c);
}

int aff_hardnet_forward_pyr_marked(affnet_ctx* ctx, const float* packed, const float* lafs, const int32_t* ids, const int32_t* count,
                                   int n_max, float* out, float* scratch, hipStream_t st) {
    CnnCall c;
    c.kind = AFFNET_NET_HARDNET; c.packed = packed; c.lafs = lafs; c.ids = ids; c.count = count; c.n_max = n_max; c.out = out; c.scratch = scratch; c.st = st;
    c.mark_head = true;
    // descriptor forms 1 / 2; a OnePassSIR context keeps form 0: its fused descriptors equal the staged path's, which describes with the stand-alone forward
    c.desc_form = ctx->cfg.onepass ? AFFNET_DESC_FORM_DIRECT : ctx->desc_form;
    return cnn_launch(ctx, c);
}

int aff_hardnet_poly_patches(affnet_ctx* ctx, const float* packed, const float* patches, int n, float* out, float* scratch, int dbg_layer, hipStream_t st, int form) {
    if (ctx->arith != AFFNET_ARITH_FP32_MFMA) return aff_fail(ctx, AFFNET_ERR_INVALID, "hardnet_poly: AFFNET_ARITH_FP32_MFMA only");
    if ((form == AFFNET_DESC_FORM_F43_CONV5 || form == AFFNET_DESC_FORM_F43_CONV1) && dbg_layer > 4) return aff_fail(ctx, AFFNET_ERR_INVALID, "hardnet_poly: the trunk of forms 3 / 4 ends behind layer 4 (conv5: affnet_probe_hardnet_c5_layer)");
    if (form == AFFNET_DESC_FORM_F43_CONV1 && dbg_layer == 0) return aff_fail(ctx, AFFNET_ERR_INVALID, "hardnet_poly: form 4 streams conv0 into conv1, 16 channels at a time: the tensor of layer 0 never exists");
    CnnCall c;
    c.kind = AFFNET_NET_HARDNET; c.packed = packed; c.patches = patches; c.n_max = n; c.out = out; c.scratch = scratch; c.st = st;
    c.dbg_layer = dbg_layer; c.dbg_out = dbg_layer >= 0 ? out : nullptr;
    c.desc_form = form;
    return cnn_launch(ctx, c);
}

extern "C" int affnet_debug_split3_variant(affnet_ctx* ctx, int bits) {
    if (!ctx) return AFFNET_ERR_INVALID;
    ctx->split3_variant = bits;             // bit 0: HardNet loops with alternating wave priorities (A/B aid; default off since round 4)
    return AFFNET_OK;
}

extern "C" int affnet_cnn32_debug_timing(affnet_ctx* ctx, unsigned long long* d_stamps) {
    if (!ctx) return AFFNET_ERR_INVALID;
    ctx->dbg_time = d_stamps;   // device buffer of n_patches * waves * 32 uint64, or NULL to switch the stamps off (this context only)
    return AFFNET_OK;
}

extern "C" int affnet_cnn32_debug_layer(affnet_ctx* ctx, int net_kind, const float* d_packed, const float* d_patch, int layer, float* d_out,
                                        void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_patch || !d_out || layer < 0 || layer > 5) return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32_debug_layer: bad argument");
    CnnCall c;
    c.kind = net_kind; c.packed = d_packed; c.patches = d_patch; c.n_max = 1; c.out = d_out; c.st = (hipStream_t)stream;
    c.dbg_layer = layer; c.dbg_out = d_out;
    return cnn_launch(ctx, c);
}

extern "C" int affnet_cnn32_debug_winograd_u(affnet_ctx* ctx, int net_kind, const float* d_packed, int layer, float* d_out, void* stream) {
    AFF_DEVICE(ctx);
    if (!ctx || !d_packed || !d_out || (net_kind != AFFNET_NET_AFFNET && net_kind != AFFNET_NET_ORINET) || (layer != 1 && layer != 3 && layer != 5))
        return aff_fail(ctx, AFFNET_ERR_INVALID, "cnn32_debug_winograd_u: AffNet / OriNet, layer 1, 3 or 5");
    const float* u;
    const int rc = aff_derive_u(ctx, net_kind, net_kind == AFFNET_NET_AFFNET ? TRUNK_WINO : TRUNK_EXACT, d_packed, net_layout(net_kind), (hipStream_t)stream, &u);
    if (rc) return rc;
    return aff_copy_async(ctx, d_out, u + Wino16::offset(layer), (size_t)Wino16::floats(layer) * sizeof(float), (hipStream_t)stream);
}
