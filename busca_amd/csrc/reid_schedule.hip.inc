// Host schedule of the ReID extractor: the workspace plan, which kernel runs for each of the 53 convs in each arithmetic flavour, and the forward.
// Context-wide state arrives as `const ReidState&`, everything of the running forward as `const ReidPass&` (reid_state.hip.inc).
// Workspace plan (halves per crop unless noted):
namespace reid_ws {
constexpr size_t IN4 = 384 * 128 * 4, STEM = 192 * 64 * 64, X0 = 96 * 32 * 64, R1 = 96 * 32 * 128, R2 = 96 * 32 * 64,
                 R3 = 96 * 32 * 256, RD = R3, XA = R3, XB = R3;
constexpr size_t HALVES = IN4 + STEM + X0 + R1 + R2 + R3 + RD + XA + XB;
constexpr size_t PART_FLOATS = 49152;         // per crop: max over convs of gridM*2*Cout / n (32-pixel tiles of conv_kwave_kernel: 96 x 2 x 256)
constexpr size_t TICKET_BYTES = 64 * (32 + 128) * 4;   // arrival counters (zero between launches): [conv][64-channel column] of bn_reduce_finalize_kernel, then [conv][16-channel group] of bn_quadform_kernel
constexpr size_t GRAM_PART_FLOATS = (size_t)24 << 20;  // chunk partials of one Gram pass (see gram_plan; weighted passes use shorter chunks: one crop at most)
constexpr size_t GRAM_G_DOUBLES = 512 * 512 + 512 + 8 * 2 * 2048;     // G, sum vector, quadratic-form partials [8][2][Cout]
constexpr size_t X3_GRAM_PART_DOUBLES = (size_t)512 * (64 * 64 + 64) > (size_t)256 * (128 * 128 + 128) ? (size_t)512 * (64 * 64 + 64) : (size_t)256 * (128 * 128 + 128);   // x3_gram_kernel partials
constexpr size_t X3_GRAM_G_DOUBLES = 128 * 128 + 128 + 2 * 2048;
inline size_t bytes(int n, size_t es = 2) {
    const size_t nn = n < 1 ? 1 : n;
    return TICKET_BYTES + nn * HALVES * es + 24 * 256 + (nn * PART_FLOATS + 2 * 2 * 2048 + nn * 2048 + nn * 512 + 2 * 26560) * 4 + (size_t)64 * 2 * 2048 * 8 +
           (es == 2 ? GRAM_PART_FLOATS * 4 + GRAM_G_DOUBLES * 8 : (X3_GRAM_PART_DOUBLES + X3_GRAM_G_DOUBLES) * 8 + 512);
}
}
// ---- statistics through the Gram matrix (reid_gram.hip.inc) ------------------------------------------------------
struct GramPlan { int cw, ngroups, npairs, steps, nchunks; };
static GramPlan gram_plan(int M, int Cin, int align_px = 0) {
    GramPlan p;
    p.cw = Cin == 128 ? 8 : 4;                                           // 128-wide tiles only where one group covers Cin (no spare registers for two)
    p.ngroups = Cin / (16 * p.cw);
    p.npairs = p.ngroups * (p.ngroups + 1) / 2;
    const int wsteps = (M + 127) / 128;                                  // rounds of 4 waves x 32 pixels
    // CW 8 holds 288 accumulator registers and 132 KB of LDS: one workgroup per CU, so one wave of workgroups
    const int target = std::max(1, (p.cw == 8 ? 256 : 768) / p.npairs);
    p.steps = (wsteps + target - 1) / target;
    if (align_px > 0) {                                                  // weighted statistics: a chunk (128 steps pixels) must not straddle two crops
        const int per = align_px / 128;                                  // 128-pixel rounds per crop (the caller checked align_px % 128 == 0)
        p.steps = std::max(1, std::min(p.steps, per));
        while (per % p.steps) --p.steps;
    }
    p.nchunks = (wsteps + p.steps - 1) / p.steps;
    return p;
}
static bool gram_fits(int M, int Cin, int align_px) {
    const GramPlan p = gram_plan(M, Cin, align_px);
    return (size_t)p.nchunks * p.npairs * (size_t)(16 * p.cw) * (16 * p.cw) <= reid_ws::GRAM_PART_FLOATS;
}
// `ohw`: output pixels per crop of the bottleneck (M = crops x ohw)
static bool reid_use_gram(const ReidState& R, const ReidPass& P, int layer, int M, int ohw) {
    if (R.prec != BUSCA_PREC_F16 || layer > 2) return false;            // layer4: M ~ Cin, the quadratic form costs more than it saves
    if (P.wts != nullptr && layer > 1) return false;                    // weighted statistics (Gram chunks inside one crop): 3072 / 768 pixels per crop in layers 1-2 are multiples of 128, layer 3's 192 are not
    const bool use = R.k.gram_mode >= 0 ? R.k.gram_mode >= 1 : M >= R.k.gram_min_pixels;
    if (!use) return false;
    // a weighted pass cuts its chunks at crop boundaries (nchunks ~ crops): beyond ~600 distinct crops the chunk partials of a 256-channel
    // input no longer fit the scratch - take the direct-statistics schedule then (conv3's input has 64 << layer channels, the first
    // block's downsample input 64 / 256 / 512)
    const int al = P.wts != nullptr ? ohw : 0;
    return gram_fits(M, 64 << layer, al) && gram_fits(M, layer == 0 ? 64 : 128 << layer, al);
}
// BN (scale, shift) of a 1x1 conv (stride `stride`, weights w [Cout][Cin] fp16) over an n x H x W x Cin input x, from x alone.
struct GramConv { const _Float16* x; const float* in_ss; int H, W, Cin, stride; const _Float16* w; int Cout; const float* gamma; const float* beta; float* ss_out;
                  int* qticket; };      // qticket: the conv's arrival counters of bn_quadform_kernel, or NULL (a finalise launch of its own)
static int gram_stats_launch(busca_ctx* c, const ReidPass& P, const GramConv& q) {
    hipStream_t s = P.s; const float* wts = P.wts; float* gpart = P.gpart; double* gG = P.gG; int* qticket = q.qticket;
    const int n = P.n, H = q.H, W = q.W, Cin = q.Cin, stride = q.stride, Cout = q.Cout;
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1, M = n * OH * OW;
    if (wts != nullptr && (OH * OW) % 128) return fail(c, BUSCA_EINVAL, "weighted Gram statistics need a multiple of 128 pixels per crop (%d)", OH * OW);
    const double invM = 1.0 / ((wts != nullptr ? P.wsum : (double)n) * (double)(OH * OW));
    if ((Cin & (Cin - 1)) || Cin < 64 || Cin > 512 || Cout < QF_CPB || Cout % QF_CPB || Cout > 2048 || (stride != 1 && OW % 8))
        return fail(c, BUSCA_EINVAL, "Gram statistics: unsupported shape (Cin %d, Cout %d, M %d)", Cin, Cout, M);
    const GramPlan p = gram_plan(M, Cin, wts != nullptr ? OH * OW : 0);
    const int gw = 16 * p.cw, tile = gw * gw;
    if ((size_t)p.nchunks * p.npairs * tile > reid_ws::GRAM_PART_FLOATS)
        return fail(c, BUSCA_EINVAL, "Gram statistics: unsupported shape (Cin %d, Cout %d, M %d)", Cin, Cout, M);
    GramArgs g{};
    g.x = q.x; g.in_ss = q.in_ss; g.M = M; g.Cin = Cin; g.OHW = OH * OW; g.OW = OW; g.HW = H * W; g.W = W; g.stride = stride;
    g.steps = p.steps; g.ngroups = p.ngroups; g.nchunks = p.nchunks; g.npairs = p.npairs; g.partials = gpart;
    double* gsum = gG + (size_t)512 * 512;
    const size_t lds = (size_t)2 * tile * 4 + (size_t)2 * Cin * 4;
    const size_t lds_max = (size_t)2 * tile * 4 + (size_t)2 * 512 * 4;   // the attribute is set once per kernel: use the largest Cin
    const dim3 ggrid(((p.nchunks + 7) / 8) * 8 * p.npairs), rgrid(tile / 64, p.npairs);
    if (p.cw == 4) {
        if (p.ngroups == 1) hipLaunchKernelGGL((gram_kernel<4, false>), ggrid, dim3(256), lds, s, g);
        else hipLaunchKernelGGL((gram_kernel<4, true>), ggrid, dim3(256), lds, s, g);
        hipLaunchKernelGGL((gram_reduce_kernel<4>), rgrid, dim3(1024), 0, s, (const float*)gpart, p.nchunks, p.npairs, p.ngroups, Cin, gG, gsum, wts, 128 * p.steps, OH * OW);
    } else {
        { int rc = ensure_lds(c, (const void*)gram_kernel<8, false>, lds_max); if (rc) return rc; }
        hipLaunchKernelGGL((gram_kernel<8, false>), ggrid, dim3(256), lds, s, g);
        hipLaunchKernelGGL((gram_reduce_kernel<8>), rgrid, dim3(1024), 0, s, (const float*)gpart, p.nchunks, p.npairs, p.ngroups, Cin, gG, gsum, wts, 128 * p.steps, OH * OW);
    }
    const size_t qlds = ((size_t)16 * (Cin + 2) + 2 * 4 * 16) * 8;
    { int rc = ensure_lds(c, (const void*)bn_quadform_kernel_t<_Float16>, ((size_t)16 * (512 + 2) + 2 * 4 * 16) * 8); if (rc) return rc; }
    const int JS = Cin <= 128 ? 1 : Cin / 64;                            // tile-pair slices; small matrices finish inside the kernel
    double* qpart = gsum + 512;                                          // [JS][2][Cout]
    if (Cout / QF_CPB > 128) qticket = nullptr;
    hipLaunchKernelGGL(bn_quadform_kernel_t<_Float16>, dim3(Cout / QF_CPB, JS), dim3(256), qlds, s, (const double*)gG, (const double*)gsum, q.w, Cin, Cout, qpart,
                       invM, q.gamma, q.beta, q.ss_out, JS > 1 ? qticket : (int*)nullptr);
    if (JS > 1 && qticket == nullptr) hipLaunchKernelGGL(bn_quadform_finalize_kernel, dim3((Cout + 255) / 256), dim3(256), 0, s, (const double*)qpart, JS, Cout, invM, q.gamma, q.beta, q.ss_out);
    return BUSCA_OK;
}
static int reid_gram_stats(busca_ctx* c, const ReidState& R, const ReidPass& P, int idx, const _Float16* x, const float* in_ss, int H, int W) {
    const ReidConv& cv = R.convs[idx];
    if (P.skip_stats) return BUSCA_OK;                                  // running-statistics pass: the consumers read the fixed table
    if (cv.k != 1) return fail(c, BUSCA_EINVAL, "internal: Gram statistics on a %dx%d conv", cv.k, cv.k);
    int* qt = (P.tickets != nullptr && idx < 64 && !R.k.two_launch_stats) ? P.tickets + 64 * 32 + idx * 128 : nullptr;
    return gram_stats_launch(c, P, {x, in_ss, H, W, cv.cin, cv.stride, (const _Float16*)R.d_w + cv.w_off, cv.cout, R.d_f + cv.g_off, R.d_f + cv.b_off, P.ssb + cv.ss_off, qt});
}
// BatchNorm (scale, shift) of conv `idx` from its per-tile statistics [gridM][2][cout]: ONE launch either way - the direct kernel
// for few tiles, reduce + finalise-by-the-last-arriver beyond (tickets: [conv][64-channel column] words of the workspace).
static void bn_finalize_launch(const ReidState& R, const ReidPass& P, int idx, int gridM, double invM) {
    if (P.skip_stats) return;                                           // running-statistics pass: the per-tile partials the conv epilogues wrote stay unused
    const ReidConv& cv = R.convs[idx];
    hipStream_t s = P.s; const float* partials = P.partials; double* red = P.red; float* ss_out = P.ssb + cv.ss_off;
    const float* gamma = R.d_f + cv.g_off; const float* beta = R.d_f + cv.b_off;
    if (gridM <= R.k.direct_rows) {
        hipLaunchKernelGGL(bn_finalize_direct_kernel, dim3((cv.cout + 63) / 64), dim3(1024), 0, s, partials, gridM, cv.cout, invM, gamma, beta, ss_out);
    } else if (P.tickets != nullptr && idx < 64 && (cv.cout + 63) / 64 <= 32 && !R.k.two_launch_stats) {
        hipLaunchKernelGGL(bn_reduce_finalize_kernel, dim3((cv.cout + 63) / 64, BN_SLICES), dim3(256), 0, s, partials, gridM, cv.cout, red, P.tickets + idx * 32, invM, gamma, beta, ss_out);
    } else {
        hipLaunchKernelGGL(bn_reduce_kernel, dim3((cv.cout + 63) / 64, BN_SLICES), dim3(256), 0, s, partials, gridM, cv.cout, red);
        hipLaunchKernelGGL(bn_finalize_kernel, dim3((cv.cout + 255) / 256), dim3(256), 0, s, (const double*)red, cv.cout, invM, gamma, beta, ss_out);
    }
}

// ---- F16X3 flavour (reid_x3.hip.inc): one kernel family for every conv ---------------------------------------------------------
template <int WC, int WP, int CT, int PT, int STG, int KS, int EPI, int SK = 0>
static int x3_launch_one(busca_ctx* c, hipStream_t s, const X3Args& a) {
    constexpr int tables = (STG == X3_BN || STG == X3_POOLIN) ? 1 : STG == X3_MRG ? 2 : 0;
    const size_t lds = x3_lds_bytes<WC, WP, CT, PT>(a.Cin, tables, EPI == X3_MERGE_C1, SK == 3 && STG == X3_BN, SK == 3 && STG == X3_STEM, EPI == X3_POOL);
    { int rc = ensure_lds(c, (const void*)conv_x3_kernel<WC, WP, CT, PT, STG, KS, EPI, 0, SK>, x3_lds_bytes<WC, WP, CT, PT>(2048, tables, EPI == X3_MERGE_C1, SK == 3 && STG == X3_BN, SK == 3 && STG == X3_STEM, EPI == X3_POOL)); if (rc) return rc; }
    const unsigned nb = (unsigned)(((a.gridM + 7) / 8) * 8 * a.gridN);
    TimedLaunch tl(c, s);
    hipLaunchKernelGGL((conv_x3_kernel<WC, WP, CT, PT, STG, KS, EPI, 0, SK>), dim3(nb), dim3(64 * WC * WP), lds, s, a);
    return BUSCA_OK;
}
// BatchNorm (scale, shift) of 1x1 conv `idx` (C -> 4 C, C = 64 / 128) from the float32-equivalent Gram matrix of its input (x3_gram_kernel)
template <int C>
static int x3_gram_stats_c(busca_ctx* c, const ReidState& R, const ReidPass& P, int idx, const float* x, const float* in_ss, int ohw) {
    const ReidConv& cv = R.convs[idx];
    hipStream_t s = P.s; double* part = P.x3part; double* G = P.x3G; float* ss_out = P.ssb + cv.ss_off;
    const int M = P.n * ohw, ntiles = (M + 127) / 128;
    const int nwg = std::min(ntiles, C == 64 ? 512 : 256);
    X3GramArgs a{};
    a.x = x; a.in_ss = in_ss; a.wts = P.wts; a.part = part; a.M = M; a.OHW = ohw; a.ntiles = ntiles;
    constexpr size_t lds = (size_t)2 * 128 * 2 * C + (size_t)C * 8;        // two row-major fp16 planes of the tile (the channel-sum scratch of the end reuses them), BatchNorm table
    { int rc = ensure_lds(c, (const void*)x3_gram_kernel<C>, lds); if (rc) return rc; }
    double* sum = G + (size_t)C * C;
    double* qpart = sum + C;
    {
        TimedLaunch tl(c, s);
        hipLaunchKernelGGL((x3_gram_kernel<C>), dim3(nwg), dim3(4 * C), lds, s, a);
    }
    hipLaunchKernelGGL((x3_gram_reduce_kernel<C>), dim3((C * C + C + 63) / 64), dim3(256), 0, s, (const double*)part, nwg, G, sum);
    const size_t qlds = ((size_t)16 * (C + 2) + 2 * 4 * 16) * 8;
    { int rc = ensure_lds(c, (const void*)bn_quadform_kernel_t<float>, ((size_t)16 * (512 + 2) + 2 * 4 * 16) * 8); if (rc) return rc; }
    const double invM = 1.0 / (P.wsum * (double)ohw);
    hipLaunchKernelGGL(bn_quadform_kernel_t<float>, dim3(cv.cout / QF_CPB, 1), dim3(256), qlds, s, (const double*)G, (const double*)sum, (const float*)R.d_w + cv.w_off, C, cv.cout, qpart,
                       invM, (const float*)(R.d_f + cv.g_off), (const float*)(R.d_f + cv.b_off), ss_out, (int*)nullptr);
    return BUSCA_OK;
}

// Persistent fused tail (reid_x3p.hip.inc) of a 1x1 conv3 with 64 / 128 input channels: one workgroup per CU for the whole launch.  Returns -1 when the
// shape is not one the kernel is built for (the caller then launches the one-shot kernel: same results bit for bit).
template <int KC, int C1, int NW, bool W2P, bool W3P>
static int x3_ptail_launch_one(busca_ctx* c, hipStream_t s, const ReidState& R, const X3PArgs& p) {
    constexpr size_t lds = x3p_lds_bytes<KC, C1>();
    { int rc = ensure_lds(c, (const void*)x3_ptail_kernel<KC, C1, NW, W2P, W3P>, lds); if (rc) return rc; }
    const int per = 8 * p.gridN;
    int nwg = (R.num_cu / per) * per;                   // a multiple of 8 x gridN: the workgroups of a pixel tile sit on one XCD
    if (nwg <= 0) return -1;
    TimedLaunch tl(c, s);
    hipLaunchKernelGGL((x3_ptail_kernel<KC, C1, NW, W2P, W3P>), dim3(nwg), dim3(64 * NW), lds, s, p);
    return BUSCA_OK;
}
static int x3_ptail_launch(busca_ctx* c, hipStream_t s, const ReidState& R, const X3Args& a) {
    if (R.k.x3_ptail_min <= 0 || a.M % 128 != 0 || a.OHWo % 128 != 0 || a.Cout % 256 != 0 || a.in_ss == nullptr) return -1;
    const int ntiles = a.M / 128, gridN = a.Cout / 256;
    if ((long)ntiles * gridN < (long)R.k.x3_ptail_min || R.num_cu < 8 * gridN) return -1;
    X3PArgs p{};
    p.in = a.in; p.in_ss = a.in_ss; p.w = a.w; p.inv = a.inv; p.out = a.out; p.out_ss = a.out_ss; p.idt = a.idt; p.idt_ss = a.idt_ss;
    p.c1_w = a.c1_w; p.c1_inv = a.c1_inv; p.c1_out = a.c1_out; p.partials = a.partials; p.wts = a.wts;
    p.M = a.M; p.Cout = a.Cout; p.OHWo = a.OHWo; p.ntiles = ntiles; p.gridN = gridN;
    if (a.Cin == 64 && a.Cout == 256 && a.c1_w != nullptr && a.c1_cout == 64) return x3_ptail_launch_one<1, 64, 4, true, true>(c, s, R, p);
    if (a.Cin == 64 && a.Cout == 256 && a.c1_w != nullptr && a.c1_cout == 128) return x3_ptail_launch_one<1, 128, 4, false, false>(c, s, R, p);
    if (a.Cin == 64 && a.c1_w == nullptr) return x3_ptail_launch_one<1, 0, 8, true, true>(c, s, R, p);
    if (a.Cin == 128 && a.c1_w == nullptr) return x3_ptail_launch_one<2, 0, 8, true, true>(c, s, R, p);
    return -1;
}

// One conv of the forward: conv `idx` over `in` (H x W per crop; in_ss: the (scale, shift) to apply while staging a RAW input, NULL for final values) into `out`;
// the optional parts are absent unless named.  T: the activation type (fp16 flavour: _Float16; exact-f32 and split-fp16: float).
template <typename T>
struct ConvCall {
    int idx; const T* in; const float* in_ss; int H, W; T* out; int mode = CONV_NORMAL;
    const T* idt = nullptr; const float* idt_ss = nullptr;                                                // CONV_MERGE: the identity branch of the block tail
    int ds_idx = -1; const T* ds_in = nullptr; int dsH = 0, dsW = 0; const float* ds_in_ss = nullptr;     // CONV_MERGE_DS: the downsample conv accumulated by the tail
    const T* mrg_idt = nullptr; const float* mrg_idt_ss = nullptr; T* mrg_out = nullptr;                  // the previous block's deferred tail, formed while staging
    int c1_idx = -1; T* c1_out = nullptr;                                                                 // the next bottleneck's conv1 carried in the tail
};

static int reid_x3_conv(busca_ctx* c, const ReidState& R, const ReidPass& P, const ConvCall<float>& q, int* OHo, int* OWo) {
    const ReidKnobs& K = R.k;
    hipStream_t s = P.s;
    const int idx = q.idx, n = P.n, H = q.H, W = q.W, mode = q.mode, c1_idx = q.c1_idx;
    const float* in = q.in; const float* in_ss = q.in_ss; float* out = q.out; const float* mrg_idt = q.mrg_idt; float* mrg_out = q.mrg_out; float* c1_out = q.c1_out;
    const ReidConv& cv = R.convs[idx];
    if (cv.wx3_off == (size_t)-1 || R.d_wx3 == nullptr) return fail(c, BUSCA_EINVAL, "internal: conv %d has no split-fp16 weights", idx);
    const bool stem = cv.cin == 3;
    X3Args a{};
    a.in = in; a.in_ss = in_ss; a.w = R.d_wx3 + cv.wx3_off; a.inv = R.d_f + cv.inv_off; a.out = out; a.partials = P.partials; a.zero = (const float*)R.d_zero;
    a.wts = P.wts; a.out_ss = P.rss + cv.ss_off; a.idt = q.idt; a.idt_ss = q.idt_ss;
    a.mrg_idt = mrg_idt; a.mrg_idt_ss = q.mrg_idt_ss; a.mrg_out = mrg_out;
    if (stem && K.x3_stem_halo && P.stem_crops != nullptr) { a.stem_crops = P.stem_crops; a.stem_zero = P.stem_zn; a.stem_lut = R.d_x3_lut; }
    const bool pool_out = stem && K.x3_stem_halo && P.pool_q != nullptr && mode == CONV_NORMAL;                  // the stem writes the pooled parts instead of its raw map (`out` = P)
    const bool pool_in = !stem && P.pool_q != nullptr && in == P.pool_p && in_ss != nullptr && cv.k == 1 && cv.stride == 1 && cv.cin == 64 && mode == CONV_NORMAL;
    if (pool_out) { a.pool_gamma = R.d_f + cv.g_off; a.pool_p = out; a.pool_q = P.pool_q; }
    if (pool_in) a.pool_q = P.pool_q;
    if (!stem && P.pool_q != nullptr && in == P.pool_p && !pool_in) return fail(c, BUSCA_EINVAL, "internal: conv %d cannot read the pooled stem parts", idx);
    if (mrg_out != nullptr && !(cv.k == 1 && cv.stride == 1 && in_ss && mrg_idt && mode == CONV_NORMAL && cv.cout % 256 == 0))
        return fail(c, BUSCA_EINVAL, "internal: conv %d cannot form its input from the previous block's tail", idx);
    a.H = H; a.W = W; a.Cin = stem ? 4 : cv.cin; a.Cout = cv.cout; a.stride = cv.stride; a.pad = cv.pad;
    a.OH = (H + 2 * cv.pad - cv.k) / cv.stride + 1; a.OW = (W + 2 * cv.pad - cv.k) / cv.stride + 1;
    a.M = n * a.OH * a.OW; a.OHWo = a.OH * a.OW;
    a.gridM = (a.M + 127) / 128;
    if (c1_idx >= 0) {
        // fused tail + the next bottleneck's conv1 (X3_MERGE_C1): one channel block of 256, 128-pixel tiles
        const ReidConv& cn = R.convs[c1_idx];
        if (!(mode == CONV_MERGE && cv.k == 1 && cv.cout == 256 && in_ss && cn.k == 1 && cn.stride == 1 && cn.cin == 256 && (cn.cout == 64 || cn.cout == 128) && cn.wx3_off != (size_t)-1 && c1_out))
            return fail(c, BUSCA_EINVAL, "internal: conv %d cannot carry conv %d in its tail", idx, c1_idx);
        a.c1_w = R.d_wx3 + cn.wx3_off; a.c1_inv = R.d_f + cn.inv_off; a.c1_out = c1_out; a.c1_cout = cn.cout; a.gridN = 1;
        int rc = x3_ptail_launch(c, s, R, a);
        if (rc < 0) rc = x3_launch_one<8, 1, 2, 8, X3_BN, 1, X3_MERGE_C1>(c, s, a);
        if (rc) return rc;
        *OHo = a.OH; *OWo = a.OW;
        bn_finalize_launch(R, P, c1_idx, a.gridM, 1.0 / (P.wsum * (double)(a.OH * a.OW)));
        return BUSCA_OK;
    }
    const int epi = mode == CONV_NORMAL ? X3_RAW : mode == CONV_STATS_ONLY ? X3_STATS : X3_MERGE;
    if (mode != CONV_NORMAL && mode != CONV_STATS_ONLY && mode != CONV_MERGE) return fail(c, BUSCA_EINVAL, "internal: split-fp16 conv mode %d", mode);
    // 3x3, stride 1, 128-pixel tiles made of whole image rows (layers 1-2): one staging per kernel row serves its three taps (conv_x3_kernel ROW3)
    const bool row3_any = K.x3_row3 > 0 && cv.k == 3 && cv.stride == 1 && cv.pad == 1 && (a.OW == 8 || a.OW == 16 || a.OW == 32) && cv.cin % 64 == 0 && (cv.cin & (cv.cin - 1)) == 0 && in_ss;
    const bool row3 = row3_any && (a.OH * a.OW) % 128 == 0 && a.OW >= 16;
    const bool row3_64 = row3_any && K.x3_row3 >= 2 && (a.OH * a.OW) % 64 == 0 && cv.cout % 256 == 0 && epi == X3_RAW;     // 64-pixel tiles (layers 3-4: 24 x 8 maps)
    int rc = BUSCA_EINVAL;
    if (stem) { a.gridN = 1; rc = pool_out ? x3_launch_one<2, 2, 2, 4, X3_STEM, 7, X3_POOL, 3>(c, s, a) : K.x3_stem_halo ? x3_launch_one<2, 2, 2, 4, X3_STEM, 7, X3_RAW, 3>(c, s, a) : x3_launch_one<2, 2, 2, 4, X3_STEM, 7, X3_RAW>(c, s, a); }
    else if (cv.cout % 256 == 0 && cv.k == 3 && in_ss && epi == X3_RAW && K.x3_narrow3 > 0 && ((a.M + 63) / 64) * (cv.cout / 256) < K.x3_narrow3) {
        // small batches: the 3x3 convs of layers 3-4 on four-wave workgroups of 64 pixels x 128 channels, two per CU (a workgroup's serial K loop sets the
        // duration of such a launch; twice the workgroups, each with half the products per step)
        a.gridN = cv.cout / 128; a.gridM = (a.M + 63) / 64;
        rc = x3_launch_one<4, 1, 2, 4, X3_BN, 3, X3_RAW>(c, s, a);
    }
    else if (row3_64 && !(K.x3_narrow3 > 0 && ((a.M + 63) / 64) * (cv.cout / 256) < K.x3_narrow3)) {
        a.gridN = cv.cout / 256; a.gridM = (a.M + 63) / 64;
        rc = x3_launch_one<8, 1, 2, 4, X3_BN, 3, X3_RAW, 3>(c, s, a);
    }
    else if (cv.cout % 256 == 0) {
        a.gridN = cv.cout / 256;
        // launches that would not fill the chip twice run on 64-pixel tiles (twice the workgroups, each with half the serial K loop's work):
        // tracker-sized batches (40-150 crops) put layers 3-4 at 30-230 tiles of 128 pixels
        // x3_half_blocks < 0 (default): whichever tile height takes fewer ROUNDS of one-workgroup-per-CU launches, a 64-pixel round priced at 0.52 of a
        // 128-pixel one (measured: layer 3's 3x3 94 / 48 us per round): 88 crops put layer 3 at 132 tiles of 128 pixels = ONE round, where 264 tiles of 64
        // pixels take two (88 crops 4.70 -> 4.59 ms, 150 crops 6.34 -> 6.15)
        bool half = a.gridM * a.gridN < K.x3_half_blocks;
        if (K.x3_half_blocks < 0) {
            const long t128 = (long)a.gridM * a.gridN, t64 = (long)((a.M + 63) / 64) * a.gridN, ncu = R.num_cu > 0 ? R.num_cu : 256;
            half = t128 < 2 * ncu && (double)((t64 + ncu - 1) / ncu) * 0.52 < (double)((t128 + ncu - 1) / ncu);       // (beyond two rounds the 64-pixel tiles measured equal or slower)
        }
        if (half) a.gridM = (a.M + 63) / 64;
#define X3_L(S_, K_, E_) (half ? x3_launch_one<8, 1, 2, 4, S_, K_, E_>(c, s, a) : x3_launch_one<8, 1, 2, 8, S_, K_, E_>(c, s, a))
        if (pool_in) rc = X3_L(X3_POOLIN, 1, X3_RAW);
        else if (mrg_out != nullptr) rc = X3_L(X3_MRG, 1, X3_RAW);
        else if (cv.k == 3 && in_ss && epi == X3_RAW) rc = X3_L(X3_BN, 3, X3_RAW);
        else if (cv.k == 1 && in_ss && epi == X3_RAW) rc = X3_L(X3_BN, 1, X3_RAW);
        else if (cv.k == 1 && in_ss && epi == X3_STATS) rc = X3_L(X3_BN, 1, X3_STATS);
        else if (cv.k == 1 && in_ss && epi == X3_MERGE) {
            rc = cv.stride == 1 ? x3_ptail_launch(c, s, R, a) : -1;         // layers 1-2, large batches: persistent workgroups (same results bit for bit)
            if (rc < 0) rc = X3_L(X3_BN, 1, X3_MERGE);
        }
        else if (cv.k == 1 && !in_ss && epi == X3_RAW) rc = X3_L(X3_PLAIN, 1, X3_RAW);
#undef X3_L
    } else if (cv.cout == 128 && epi == X3_RAW) {
        a.gridN = 1;
        if (cv.k == 3 && in_ss && row3) rc = x3_launch_one<4, 1, 2, 8, X3_BN, 3, X3_RAW, 3>(c, s, a);
        else if (cv.k == 3 && in_ss) rc = x3_launch_one<4, 1, 2, 8, X3_BN, 3, X3_RAW>(c, s, a);
        else if (cv.k == 1 && !in_ss) rc = x3_launch_one<4, 1, 2, 8, X3_PLAIN, 1, X3_RAW>(c, s, a);
    } else if (cv.cout == 64 && epi == X3_RAW) {
        a.gridN = 1;
        if (pool_in) rc = x3_launch_one<2, 2, 2, 4, X3_POOLIN, 1, X3_RAW>(c, s, a);
        else if (cv.k == 3 && in_ss && row3 && K.x3_ptail_min > 0 && cv.cin == 64 && a.OW == 32 && a.OH % 4 == 0 && a.M % 128 == 0 && a.M / 128 >= 16) {
            // layer 1's stride-1 3x3 convs: persistent halo-resident workgroups, weights in registers (x3_p3x3_kernel; the one-shot ROW3 kernel's results bit for bit)
            X3P3Args p{};
            p.in = a.in; p.in_ss = a.in_ss; p.w = a.w; p.inv = a.inv; p.out = a.out; p.partials = a.partials; p.wts = a.wts;
            p.M = a.M; p.OH = a.OH; p.OHWo = a.OHWo; p.ntiles = a.M / 128;
            rc = ensure_lds(c, (const void*)x3_p3x3_kernel, x3p3_lds_bytes());
            if (!rc) {
                TimedLaunch tl(c, s);
                hipLaunchKernelGGL(x3_p3x3_kernel, dim3(std::min(p.ntiles, R.num_cu)), dim3(256), x3p3_lds_bytes(), s, p);
            }
        }
        else if (cv.k == 3 && in_ss && row3) rc = x3_launch_one<2, 2, 2, 4, X3_BN, 3, X3_RAW, 3>(c, s, a);
        else if (cv.k == 3 && in_ss) rc = x3_launch_one<2, 2, 2, 4, X3_BN, 3, X3_RAW>(c, s, a);
        else if (cv.k == 1 && !in_ss) rc = x3_launch_one<2, 2, 2, 4, X3_PLAIN, 1, X3_RAW>(c, s, a);
    }
    if (rc == BUSCA_EINVAL) return fail(c, BUSCA_EINVAL, "internal: no split-fp16 kernel for conv %d (k %d, %d -> %d, %s input, mode %d)", idx, cv.k, cv.cin, cv.cout, in_ss ? "raw" : "final", mode);
    if (rc) return rc;
    *OHo = a.OH; *OWo = a.OW;
    if (mode == CONV_MERGE) return BUSCA_OK;
    bn_finalize_launch(R, P, idx, a.gridM, 1.0 / (P.wsum * (double)(a.OH * a.OW)));
    return BUSCA_OK;
}

#ifdef BUSCA_CONV_PROBE
// Phase stamps [workgroup][8] of ONE launch (probe builds only: the kernels stamp under -DBUSCA_CONV_PROBE).  arm() before the launch gives the zeroed buffer for
// the kernel's `ts` argument; means() after it synchronises the stream and averages, over the first `nwg` workgroups that ran to their end, the time between
// consecutive stamps of `seq` (d[k] = seq[k] - seq[k-1]) and the lifetime, in units of 100 s_memtime ticks.
struct PhaseProbe {
    static constexpr int NWG = 4096;
    struct Means { double d[8] = {0, 0, 0, 0, 0, 0, 0, 0}, life = 0; int cnt = 0; };
    static unsigned long long* buf() { static unsigned long long* p = nullptr; if (!p) hipMalloc((void**)&p, (size_t)NWG * 8 * 8); return p; }
    static unsigned long long* arm(hipStream_t s) { hipMemsetAsync(buf(), 0, (size_t)NWG * 8 * 8, s); return buf(); }
    static Means means(hipStream_t s, int nwg, const int* seq, int nseq) {
        hipStreamSynchronize(s);
        std::vector<unsigned long long> h((size_t)NWG * 8);
        hipMemcpy(h.data(), buf(), h.size() * 8, hipMemcpyDeviceToHost);
        Means m;
        for (int b = 0; b < NWG && b < nwg; ++b) {
            const unsigned long long* r = &h[(size_t)b * 8];
            if (!r[0] || !r[7]) continue;
            ++m.cnt; m.life += (double)(r[7] - r[0]);
            for (int k = 1; k < nseq; ++k) if (r[seq[k]] && r[seq[k - 1]]) m.d[k] += (double)(r[seq[k]] - r[seq[k - 1]]);
        }
        m.life /= m.cnt * 100.0;
        for (double& v : m.d) v /= m.cnt * 100.0;
        return m;
    }
};
#endif

// The argument block of the LDS-tiled conv kernels on 128-pixel tiles.  ConvArgs names its activations and weights _Float16; conv_f32_kernel reads the same
// fields as float, so both flavours hand them over untyped.
static ConvArgs conv_args(const ReidState& R, const ReidPass& P, const ReidConv& cv, const void* in, const float* in_ss, int H, int W, void* out, const void* w) {
    ConvArgs g{};
    g.in = (const _Float16*)in; g.w = (const _Float16*)w; g.in_ss = in_ss; g.out = (_Float16*)out; g.partials = P.partials;
    g.n = P.n; g.H = H; g.W = W; g.Cin = cv.cin; g.Cout = cv.cout; g.KH = cv.k; g.KW = cv.k; g.stride = cv.stride; g.pad = cv.pad;
    g.OH = (H + 2 * cv.pad - cv.k) / cv.stride + 1; g.OW = (W + 2 * cv.pad - cv.k) / cv.stride + 1;
    g.M = P.n * g.OH * g.OW; g.wts = P.wts; g.OHWo = g.OH * g.OW;
    g.gridM = (g.M + 127) / 128; g.gridN = cv.cout == 64 ? 1 : cv.cout / 128;
    g.out_ss = P.rss + cv.ss_off; g.zero = (const _Float16*)R.d_zero;
    return g;
}

// ---- fp16 flavour: halo-resident 3x3 / pipelined weights-direct / K split across waves / LDS-tiled GEMM --------------------------
// u8 crops -> raw, max-pooled stem output in one kernel (normalisation folded into the halo staging; reid_halo.hip.inc).  Returns the stem's (scale, shift):
// x0 is RAW, its consumers apply the stem's BatchNorm + ReLU while staging.
static const float* reid_f16_stem_pool(const ReidState& R, const ReidPass& P, const uint8_t* crops, const uint8_t* zero_norm, _Float16* x0) {
    StemArgs a{};
    a.crops = crops; a.zero_norm = zero_norm; a.w = R.d_wpk + R.stem_wpk_off; a.lut = R.d_wpk + R.stem_lut_off; a.partials = P.partials; a.n = P.n; a.gridM = P.n * 48;
    a.wts = P.wts;
    a.out = x0; a.negmask = R.stem_negmask;      // already max-pooled (min where gamma < 0): see stem_pool_kernel
    hipLaunchKernelGGL((stem_pool_kernel<2>), dim3(a.gridM), dim3(256), 0, P.s, a);
    bn_finalize_launch(R, P, 0, a.gridM, 1.0 / (P.wsum * 192.0 * 64.0));
    return P.rss + R.convs[0].ss_off;
}
static int reid_f16_conv(busca_ctx* c, const ReidState& R, const ReidPass& P, const ConvCall<_Float16>& q, int* OHo, int* OWo) {
    const ReidKnobs& K = R.k; const ReidConv& cv = R.convs[q.idx]; hipStream_t s = P.s;
    const int idx = q.idx, n = P.n, H = q.H, W = q.W, mode = q.mode;
    const _Float16* in = q.in; const float* in_ss = q.in_ss; _Float16* out = q.out; float* partials = P.partials;
    if (q.mrg_out != nullptr) return fail(c, BUSCA_EINVAL, "internal: deferred block tail outside the split-fp16 flavour");
    ConvArgs g = conv_args(R, P, cv, in, in_ss, H, W, out, (const _Float16*)R.d_w + cv.w_off);
    const double invM = 1.0 / (P.wsum * (double)(g.OH * g.OW));    // statistics count: sum of multiplicities x pixels per crop
    int gridM = g.gridM;
    g.idt = q.idt; g.idt_ss = q.idt_ss;
    if (mode == CONV_MERGE_DS) {
        const ReidConv& dv = R.convs[q.ds_idx];
        g.ds_in = q.ds_in; g.ds_w = (const _Float16*)R.d_w + dv.w_off;
        g.ds_H = q.dsH; g.ds_W = q.dsW; g.ds_Cin = dv.cin; g.ds_stride = dv.stride; g.ds_in_ss = q.ds_in_ss;
        g.idt_ss = P.rss + dv.ss_off;
    }
    const unsigned nblocks = (unsigned)(((gridM + 7) / 8) * 8 * g.gridN);
#ifdef BUSCA_CONV_PROBE
    // BUSCA_CONV_TS=<conv index>[,<mode>]: per-workgroup phase stamps of that launch (experiments)
    static const char* const ts_env = getenv("BUSCA_CONV_TS");
    static const int ts_idx = ts_env ? atoi(ts_env) : -1, ts_mode = ts_env && strchr(ts_env, ',') ? atoi(strchr(ts_env, ',') + 1) : -1;
    const bool ts_on = ts_env != nullptr && idx == ts_idx && (ts_mode < 0 || ts_mode == mode) && nblocks <= (unsigned)PhaseProbe::NWG;
    if (ts_on) g.ts = PhaseProbe::arm(s);
#endif
    // stride-1 3x3 convs with enough tiles to fill the chip: halo-resident kernel (reid_halo.hip.inc)
    int halo = 0;
    if (mode == CONV_NORMAL && K.halo && cv.k == 3 && cv.wpk_off != (size_t)-1 && R.d_wpk != nullptr && cv.cin <= 512) {
        if (W == 32 && H % 4 == 0 && cv.cout == 64 && cv.cin == 64) halo = 1;        // (its kernels take Cin = 64 as a compile-time single chunk)
        else if (W == 16 && H % 8 == 0 && cv.cout == 128) halo = 2;
        else if (W == 8 && H == 24 && cv.cout == 256) halo = 3;
        const int tiles = halo == 3 ? n : g.M / 128;
        if (halo && tiles * (cv.cout == 256 ? 2 : 1) < K.halo_min_blocks) halo = 0;      // too few workgroups: the K-split-across-waves kernel does better
    }
    // large launches of raw-output convs (1x1 / 3x3, stride 1 / 2): pipelined weights-direct kernel (reid_pipe.hip.inc)
    int pipe = 0;
    if (mode == CONV_NORMAL && !halo && (cv.k == 1 || cv.k == 3) && cv.cin % 64 == 0 && cv.cin <= 2048 && cv.cout % 128 == 0 &&
        cv.wkw_off != (size_t)-1 && R.d_wkw != nullptr && K.pipe_min_tiles > 0) {
        const int nct = cv.cout % 256 == 0 ? 4 : 2;
        const int t = ((g.M + 127) / 128) * (cv.cout / (64 * nct));
        // measured IN the 512-crop pass against conv_gemm64_kernel / conv1x1_wd_kernel (profiles/r03_*): the 3x3 convs of layers 3-4
        // 170-175 -> 152-167 us, layer 4's downsample 140 -> 113, its conv1 127 -> 118 / 70 -> 65-69; layer 3's conv1 (1024 -> 256:
        // 768 tiles = 1.5 rounds of workgroups) and the 128-channel convs of layer 2 are equal or slower, so they keep the old kernels
        const bool wins = nct == 4 && (cv.k == 3 || cv.cout >= 512);
        if (t >= K.pipe_min_tiles && (wins || K.pipe_all)) pipe = nct;
    }
    if (pipe) {
        PipeArgs a{};
        a.in = in; a.in_ss = in_ss; a.wkw = R.d_wkw + cv.wkw_off; a.out = out; a.partials = partials; a.zero = (const _Float16*)R.d_zero;
        a.wts = P.wts; a.M = g.M; a.Cin = cv.cin; a.Cout = cv.cout; a.H = H; a.W = W; a.OH = g.OH; a.OW = g.OW; a.stride = cv.stride; a.pad = cv.pad; a.OHWo = g.OHWo;
        gridM = (g.M + 127) / 128;
        a.gridN = cv.cout / (64 * pipe);
        // fewer workgroups than slots (2 per CU): 64-pixel tiles - a workgroup's serial K loop sets the duration of such a launch
        const bool half_tiles = pipe == 4 && gridM * a.gridN < K.pipe_half_blocks;
        if (half_tiles) gridM = (g.M + 63) / 64;
        a.gridM = gridM;
        const unsigned pb = (unsigned)(((gridM + 7) / 8) * 8 * a.gridN);
        TimedLaunch tl(c, s);
#define PIPE_LAUNCH(...) hipLaunchKernelGGL((conv_pipe_kernel<__VA_ARGS__>), dim3(pb), dim3(256), 0, s, a)
#define PIPE_PICK(N_, ...)  /* by kernel size and raw / final input; the trailing arguments: the 64-pixel-tile flavour */                          \
        do { if (cv.k == 3) { if (in_ss) PIPE_LAUNCH(N_, STG_BN, 3, ##__VA_ARGS__); else PIPE_LAUNCH(N_, STG_PLAIN, 3, ##__VA_ARGS__); }         \
             else { if (in_ss) PIPE_LAUNCH(N_, STG_BN, 1, ##__VA_ARGS__); else PIPE_LAUNCH(N_, STG_PLAIN, 1, ##__VA_ARGS__); } } while (0)
        if (half_tiles) PIPE_PICK(4, true, 4);
        else if (pipe == 4) PIPE_PICK(4);
        else PIPE_PICK(2);
#undef PIPE_PICK
#undef PIPE_LAUNCH
    }
    // Launches that would leave the LDS-tiled kernel with few workgroups per CU: K split across the waves of a workgroup
    // (reid_kwave.hip.inc) - smaller tiles, no barrier in the K loop, no f32 round trip through HBM.
    int kwave = 0, kw_nw = 4, kw_pt = 4;
    if (!pipe && (mode == CONV_NORMAL || mode == CONV_STATS_ONLY || mode == CONV_MERGE) && cv.cin >= 64 && cv.cin % 64 == 0 && cv.cout % 64 == 0 && cv.k <= 3 &&
        K.kwave_blocks > 0 && cv.wkw_off != (size_t)-1 && R.d_wkw != nullptr && (double)n * H * W * cv.cin < 2.0e9 && g.M < (1 << 24)) {
        const int blocks = ((g.M + 127) / 128) * g.gridN;
        if (blocks < K.kwave_blocks && (!halo || blocks < K.kwave_halo_blocks)) {
            const int nsteps = cv.k * cv.k * (cv.cin / 64), cb = cv.cout / 64;
            kw_pt = ((g.M + 63) / 64) * cb >= 256 ? 4 : 2;
            const int tiles = ((g.M + 16 * kw_pt - 1) / (16 * kw_pt)) * cb;
            kw_nw = 4;
            if (tiles * 4 < 1024 && nsteps >= 8) kw_nw = 8;
            if (kw_pt == 2 && tiles * 8 < 1024 && nsteps >= 16) kw_nw = 16;
            if (K.kwave_pt == 2 || K.kwave_pt == 4) kw_pt = K.kwave_pt;
            if (K.kwave_nw == 4 || K.kwave_nw == 8 || (K.kwave_nw == 16 && kw_pt == 2)) kw_nw = K.kwave_nw;
            // its 64 x 64 tiles read (16 PT + 64) K operand bytes x 2 per tile from L2: beyond a few hundred MB per launch the
            // L2 becomes the limit (88 crops, layer 4's 3x3: 623 MB, 63 us against 56 us for split-K + reduce)
            const double mb = (double)tiles * (16 * kw_pt + 64) * nsteps * 64 * 2 / 1e6;
            const bool thin = blocks >= 192 && nsteps < 8;          // beyond the small-batch regime only the long-K convs (4+ steps per wave)
            if (mb <= K.kwave_max_mb && !thin) { kwave = 1; halo = 0; }
        }
    }
    // (launched only now: the K-split kernel above may have taken the conv instead - BUSCA_REID_KWAVE_HALO)
    if (halo) {
        HaloArgs h{};
        h.in = in; h.wpk = R.d_wpk + cv.wpk_off; h.in_ss = in_ss; h.out = out; h.partials = partials;
        h.n = n; h.H = H; h.Cin = cv.cin; h.Cout = cv.cout; h.zero = (const _Float16*)R.d_zero; h.wts = P.wts;
        h.gridN = cv.cout == 256 ? 2 : 1;
        // layer 3: a workgroup per image leaves CUs idle below 128 crops -> half images (12 rows, 96 pixels) per workgroup
        const bool half_img = halo == 3 && n * 2 < K.halo_half_blocks;
        gridM = halo == 3 ? (half_img ? 2 * n : n) : g.M / 128;
        // layer 1 at very large batches: 2 x 2 waves on 256-pixel tiles (BUSCA_REID_HALO_WPX / _WPX_MIN, reid_halo.hip.inc)
        const bool wpx = halo == 1 && K.halo_wpx != 0 && g.M % 256 == 0 && g.M / 256 >= K.halo_wpx_min;
        if (wpx) gridM = g.M / 256;
        h.gridM = gridM;
        const unsigned hb = (unsigned)(((gridM + 7) / 8) * 8 * h.gridN);
        if (wpx) { hipLaunchKernelGGL((conv3x3_halo_kernel<2, 32, 8, 2>), dim3(hb), dim3(256), 0, s, h); gridM *= 2; }   // two partial-sum rows per tile
        else if (halo == 1) hipLaunchKernelGGL((conv3x3_halo_kernel<1, 32, 4>), dim3(hb), dim3(256), 0, s, h);
        else if (halo == 2) hipLaunchKernelGGL((conv3x3_halo_kernel<2, 16, 8>), dim3(hb), dim3(256), 0, s, h);
        else if (half_img) hipLaunchKernelGGL((conv3x3_halo_kernel<2, 8, 12>), dim3(hb), dim3(256), 0, s, h);
        else hipLaunchKernelGGL((conv3x3_halo_kernel<2, 8, 24>), dim3(hb), dim3(256), 0, s, h);
    }
    if (kwave) {
        const int bm = 16 * kw_pt;
        gridM = (g.M + bm - 1) / bm;
        g.gridM = gridM; g.gridN = cv.cout / 64; g.wkw = R.d_wkw + cv.wkw_off;
        const unsigned kb = (unsigned)(((gridM + 7) / 8) * 8 * g.gridN);
        const int nsl = kw_nw / 2 > 4 ? kw_nw / 2 : 4;
        const size_t tileb = std::max((size_t)nsl * 4 * kw_pt * 1024, (size_t)kw_nw * 16 * kw_pt * 128);
        const size_t lds = tileb + (size_t)2 * cv.cin * 4 + (size_t)2 * kw_nw * 64 * 4;
        const size_t lds_max = tileb + (size_t)2 * 2048 * 4 + (size_t)2 * kw_nw * 64 * 4;
#define KW_ONE(NW_, PT_, M_, DB_) { int rc = ensure_lds(c, (const void*)conv_kwave_kernel<NW_, PT_, M_, DB_>, lds_max); if (rc) return rc;         \
                                   hipLaunchKernelGGL((conv_kwave_kernel<NW_, PT_, M_, DB_>), dim3(kb), dim3(NW_ * 64), lds, s, g); }
#define KW_LAUNCH(NW_, PT_, DB_) do { if (mode == CONV_NORMAL) KW_ONE(NW_, PT_, CONV_NORMAL, DB_) else if (mode == CONV_STATS_ONLY) KW_ONE(NW_, PT_, CONV_STATS_ONLY, DB_) \
                                      else KW_ONE(NW_, PT_, CONV_MERGE, DB_) } while (0)
        if (kw_pt == 4 && kw_nw == 4) KW_LAUNCH(4, 4, 2);
        else if (kw_pt == 4) KW_LAUNCH(8, 4, 2);
        else if (kw_nw == 4) KW_LAUNCH(4, 2, 2);
        else if (kw_nw == 8) KW_LAUNCH(8, 2, 2);
        else KW_LAUNCH(16, 2, 1);
#undef KW_LAUNCH
#undef KW_ONE
    }
    if (!(halo || kwave || pipe)) {                     // LDS-tiled GEMM
        TimedLaunch tl(c, s);
        if (cv.cin == 3) hipLaunchKernelGGL((conv_gemm_kernel<1, true>), dim3(nblocks), dim3(256), 0, s, g);
        else if (cv.cout == 64) hipLaunchKernelGGL((conv_gemm64_kernel<1, CONV_NORMAL>), dim3(nblocks), dim3(256), 0, s, g);
        else if (mode == CONV_MERGE_DS) hipLaunchKernelGGL((conv_gemm64_kernel<2, CONV_MERGE_DS>), dim3(nblocks), dim3(256), 0, s, g);
        else if (mode == CONV_STATS_ONLY) hipLaunchKernelGGL((conv_gemm64_kernel<2, CONV_STATS_ONLY>), dim3(nblocks), dim3(256), 0, s, g);
        else if (mode == CONV_MERGE) hipLaunchKernelGGL((conv_gemm64_kernel<2, CONV_MERGE>), dim3(nblocks), dim3(256), 0, s, g);
        else hipLaunchKernelGGL((conv_gemm64_kernel<2, CONV_NORMAL>), dim3(nblocks), dim3(256), 0, s, g);
    }
#ifdef BUSCA_CONV_PROBE
    if (ts_on) {
        // stamps: 0 start, 1 after the prologue; third K step: 2 before staging, 3 after the LDS writes, 4 after barrier 1, 5 after
        // load issue + MFMAs, 6 after barrier 2 (conv_kwave_kernel: 6 = after its K loop); 7 end.
        const int seq[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        const PhaseProbe::Means m = PhaseProbe::means(s, PhaseProbe::NWG, seq, 8);
        fprintf(stderr, "[conv_ts] conv %d mode %d M %d Cin %d Cout %d k %d: %d workgroups, mean lifetime %.1f; prologue %.1f | step3: wait+stage %.1f, barrier %.1f, loads+mma %.1f, barrier %.1f | 1->2 %.1f, 6->7 %.1f\n",
                idx, mode, g.M, cv.cin, cv.cout, cv.k, m.cnt, m.life, m.d[1], m.d[3], m.d[4], m.d[5], m.d[6], m.d[2], m.d[7]);
    }
#endif
    *OHo = g.OH; *OWo = g.OW;
    if (mode == CONV_MERGE || mode == CONV_MERGE_DS) return BUSCA_OK;   // block tail: statistics were final before the launch
    bn_finalize_launch(R, P, idx, gridM, invM);
    return BUSCA_OK;
}

// ---- exact-f32 flavour: one kernel family, raw output + statistics -----------------------------------------------------------------
static int reid_f32_conv(busca_ctx* c, const ReidState& R, const ReidPass& P, const ConvCall<float>& q, int* OHo, int* OWo) {
    const ReidConv& cv = R.convs[q.idx]; hipStream_t s = P.s;
    if (q.mode != CONV_NORMAL || q.mrg_out != nullptr || q.c1_idx >= 0) return fail(c, BUSCA_EINVAL, "internal: fused block tail in the exact-f32 flavour (conv %d, mode %d)", q.idx, q.mode);
    const ConvArgs g = conv_args(R, P, cv, q.in, q.in_ss, q.H, q.W, q.out, (const float*)R.d_w + cv.w_off);
    const unsigned nblocks = (unsigned)(((g.gridM + 7) / 8) * 8 * g.gridN);
    if (TimedLaunch tl(c, s); cv.cin == 3) hipLaunchKernelGGL((conv_f32_kernel<1, true>), dim3(nblocks), dim3(256), 0, s, g);
    else if (cv.cout == 64) hipLaunchKernelGGL((conv_f32_kernel<1, false>), dim3(nblocks), dim3(256), 0, s, g);
    else hipLaunchKernelGGL((conv_f32_kernel<2, false>), dim3(nblocks), dim3(256), 0, s, g);
    *OHo = g.OH; *OWo = g.OW;
    bn_finalize_launch(R, P, q.idx, g.gridM, 1.0 / (P.wsum * (double)(g.OH * g.OW)));
    return BUSCA_OK;
}

static void ew_preprocess(hipStream_t s, const uint8_t* crops, const uint8_t* zn, size_t npix, _Float16* o) { hipLaunchKernelGGL(reid_preprocess_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, crops, zn, npix, o); }
static void ew_preprocess(hipStream_t s, const uint8_t* crops, const uint8_t* zn, size_t npix, float* o) { hipLaunchKernelGGL(reid_preprocess_f32_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, crops, zn, npix, o); }
static void ew_maxpool(hipStream_t s, const _Float16* raw, const float* ss, int n, _Float16* o) { const size_t t = (size_t)n * 96 * 32 * 8; hipLaunchKernelGGL(maxpool_bn_relu_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, raw, ss, n, o); }
static void ew_maxpool(hipStream_t s, const float* raw, const float* ss, int n, float* o) { const size_t t = (size_t)n * 96 * 32 * 16; hipLaunchKernelGGL(maxpool_bn_relu_f32_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, raw, ss, n, o); }
static void ew_merge(hipStream_t s, const float* r3, const float* ss3, const float* idt, const float* ssd, size_t npix, int C, float* o) { const size_t t = npix * (C / 4); hipLaunchKernelGGL(block_merge_f32_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, r3, ss3, idt, ssd, npix, C, o); }
static void ew_gpool(hipStream_t s, const _Float16* x, int n, int HW, int C, float* o) { const size_t t = (size_t)n * C; hipLaunchKernelGGL(global_maxpool_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, x, n, HW, C, o); }
static void ew_gpool(hipStream_t s, const float* x, int n, int HW, int C, float* o) { const size_t t = (size_t)n * C; hipLaunchKernelGGL(global_maxpool_f32_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, x, n, HW, C, o); }

// ---- the three arithmetic flavours: activation type + conv launcher, chosen ONCE per forward (busca_reid_forward_w) ----------------
struct ReidF16 { using T = _Float16; static constexpr int prec = BUSCA_PREC_F16; static constexpr auto conv = reid_f16_conv; };
struct ReidF32 { using T = float; static constexpr int prec = BUSCA_PREC_F32; static constexpr auto conv = reid_f32_conv; };
struct ReidX3 { using T = float; static constexpr int prec = BUSCA_PREC_F16X3; static constexpr auto conv = reid_x3_conv; };

// The workspace of the stream that calls: found, or claimed from the pool of 4, grown when the batch is larger than any before
// (device synchronisation + hipMalloc - busca_reid_reserve moves that out of the forward).
static int reid_ws_acquire(busca_ctx* c, int n, void* stream, size_t es, ReidState::WS** out) {
    ReidState& R = *c->reid;
    ReidState::WS* w = nullptr;
    for (auto& e : R.ws) if (e.ptr && e.stream == stream) { w = &e; break; }
    if (!w) for (auto& e : R.ws) if (!e.ptr) { w = &e; w->stream = stream; break; }
    if (!w) { HIP_TRY(c, hipDeviceSynchronize()); w = &R.ws[0]; w->stream = stream; }   // pool exhausted: recycle slot 0
    if (w->n < n) {
        if (w->ptr) { HIP_TRY(c, hipDeviceSynchronize()); HIP_TRY(c, hipFree(w->ptr)); w->ptr = nullptr; w->n = 0; }
        const size_t bytes = reid_ws::bytes(n, es);
        if (hipMalloc(&w->ptr, bytes) != hipSuccess) return fail(c, BUSCA_ENOMEM, "cannot allocate %zu bytes of ReID workspace for %d crops", bytes, n);
        w->bytes = bytes; w->n = n;
        HIP_TRY(c, hipMemset(w->ptr, 0, reid_ws::TICKET_BYTES));
    }
    *out = w;
    return BUSCA_OK;
}

template <typename T>                 // activation tensors of one forward (reid_ws: elements per crop)
struct ReidBufs { T *in4, *stem, *x0, *r1, *r2, *r3, *rd, *xa, *xb; float* pool; };

// u8 crops -> x0, the input of layer 1.  *x0_ss: the (scale, shift) the consumers of x0 must apply, or NULL when x0 holds final values.
template <class F>
static int reid_stem(busca_ctx* c, const ReidState& R, const ReidPass& P, const ReidBufs<typename F::T>& B, const uint8_t* crops, const uint8_t* zero_norm, const float** x0_ss) {
    using T = typename F::T;
    const float* ss0 = P.rss + R.convs[0].ss_off;
    if constexpr (F::prec == BUSCA_PREC_F16) if (R.k.halo) { *x0_ss = reid_f16_stem_pool(R, P, crops, zero_norm, B.x0); return BUSCA_OK; }
    int OH, OW;
    if (P.stem_crops == nullptr) ew_preprocess(P.s, crops, zero_norm, (size_t)P.n * 384 * 128, B.in4);   // (else the stem fills its input halo from the bytes: no normalised copy of the batch)
    // pooled: the stem writes the max pool of its RAW output (x sign(gamma)) in two parts - x0 = P, `stem` = Q - and layer 1's first conv1 / downsample conv
    // stage relu(bn(max(P, Q above))): the full-resolution raw map (1.6 GB per 512 crops) and the pooling pass are gone
    const bool pooled = P.pool_q != nullptr;
    { int rc = F::conv(c, R, P, {0, B.in4, nullptr, 384, 128, pooled ? B.x0 : B.stem}, &OH, &OW); if (rc) return rc; }            // 192 x 64
    if (!pooled) ew_maxpool(P.s, (const T*)B.stem, ss0, P.n, B.x0);
    *x0_ss = pooled ? ss0 : nullptr;
    return BUSCA_OK;
}

// One bottleneck as its tail sees it: conv1, conv2 and (unless fused) the downsample conv are enqueued; the tail strategy forms the block output in `nxt`.
template <typename T>
struct ReidBlock {
    int li, b, i1, i2, i3, id, inext;                // layer 0-3, block of the layer; conv indices: conv1-3, the downsample conv (b == 0), conv1 of the NEXT bottleneck
    const T* cur; const float* cur_ss; int H, W;     // block input
    T* nxt; int h2, w2;                              // block output; conv2's output size
    const T* idt; const float* ssd;                  // identity branch: the block input, or the raw downsample output and its BatchNorm
    bool fuse_ds, fuse_c1;                           // fp16 flavour: the tail accumulates the downsample conv / also runs the next bottleneck's conv1
    int h3, w3; bool conv1_done;                     // results: output size; the next bottleneck's conv1 (raw, in r1) and its statistics are done
};
// split-fp16 flavour, layers whose tail is not a conv3 epilogue: the tail relu(bn3(raw3) + identity) is DEFERRED into the next
// bottleneck's conv1, which forms it while staging its operand and writes it out as the next identity (no block_merge pass)
template <typename T>
struct ReidPending { const T* raw = nullptr; const float* ss = nullptr; const T* idt = nullptr; const float* idt_ss = nullptr; T* out = nullptr; };

// fp16 flavour: block tail + the NEXT bottleneck's conv1 in one kernel (reid_halo.hip.inc): that conv never re-reads this output.  `ds`: with the downsample conv.
static void f16_tail_c1(const ReidState& R, const ReidPass& P, const ReidBufs<_Float16>& B, ReidBlock<_Float16>& k, bool ds) {
    hipStream_t s = P.s; const ReidConv& c3 = R.convs[k.i3]; const ReidConv& cn = R.convs[k.inext];
    TailC1Args ta{};
    ta.in = B.r2; ta.in_ss = P.rss + R.convs[k.i2].ss_off; ta.w3 = (const _Float16*)R.d_w + c3.w_off;
    ta.out_ss = P.rss + c3.ss_off; ta.idt = k.cur; ta.out = k.nxt;
    if (ds) { ta.ds_in = k.cur; ta.ds_w = (const _Float16*)R.d_w + R.convs[k.id].w_off; ta.idt_ss = P.rss + R.convs[k.id].ss_off; ta.ds_in_ss = k.cur_ss; }
    ta.w1pk = R.d_wpk + cn.wpk_off; ta.out2 = B.r1; ta.partials2 = P.partials; ta.M = P.n * k.h2 * k.w2;
    ta.wts = P.wts; ta.OHW = k.h2 * k.w2;
    const int li = k.li, gm = ta.M / (li == 2 ? 64 : 128);
#ifdef BUSCA_CONV_PROBE
    static const int tts_idx = getenv("BUSCA_TAIL_TS") ? atoi(getenv("BUSCA_TAIL_TS")) : -1;      // BUSCA_TAIL_TS=<index of conv3>: phase stamps of that fused tail
    const bool tts_on = tts_idx == k.i3;
    if (tts_on) ta.ts = PhaseProbe::arm(s);
#endif
    if (ds) hipLaunchKernelGGL((tail_conv1_kernel<128, 64, 256, 64, true>), dim3(gm), dim3(256), 0, s, ta);
    else if (li == 0 && cn.cout == 64) hipLaunchKernelGGL((tail_conv1_kernel<128, 64, 256, 64, false>), dim3(gm), dim3(256), 0, s, ta);
    else if (li == 0) hipLaunchKernelGGL((tail_conv1_kernel<128, 64, 256, 128, false>), dim3(gm), dim3(256), 0, s, ta);
    else if (li == 1 && cn.cout == 128) hipLaunchKernelGGL((tail_conv1_kernel<128, 128, 512, 128, false>), dim3(gm), dim3(512), 0, s, ta);
    else if (li == 1) hipLaunchKernelGGL((tail_conv1_kernel<128, 128, 512, 256, false>), dim3(gm), dim3(512), 0, s, ta);
    else if (cn.cout == 256) hipLaunchKernelGGL((tail_conv1_kernel<64, 256, 1024, 256, false>), dim3(gm), dim3(1024), 0, s, ta);
    else hipLaunchKernelGGL((tail_conv1_kernel<64, 256, 1024, 512, false>), dim3(gm), dim3(1024), 0, s, ta);
#ifdef BUSCA_CONV_PROBE
    if (tts_on) {
        const int seq[7] = {0, 1, 2, 3, 4, 5, 7};
        const PhaseProbe::Means m = PhaseProbe::means(s, gm, seq, 7);
        fprintf(stderr, "[tail_ts] conv3 %d (%d -> %d, next conv1 -> %d) M %d: %d workgroups, mean lifetime %.1f | load+stage A %.1f, conv3 MFMAs %.1f, raw tile + epilogue %.1f, barrier %.1f, conv1 MFMAs %.1f, stats + stores %.1f   (100 s_memtime ticks)\n",
                k.i3, c3.cin, c3.cout, cn.cout, ta.M, m.cnt, m.life, m.d[1], m.d[2], m.d[3], m.d[4], m.d[5], m.d[6]);
    }
#endif
    bn_finalize_launch(R, P, k.inext, gm, 1.0 / (P.wsum * (double)(k.h2 * k.w2)));
    k.h3 = k.h2; k.w3 = k.w2; k.conv1_done = true;
}

// Tail, fp16 flavour with Gram statistics: BN3 (and the downsample's BN) statistics from Gram matrices of the 4x narrower inputs; then ONE conv3 pass
// whose epilogue is the block tail, with the downsample conv accumulated by the same workgroup
static int tail_f16_gram(busca_ctx* c, const ReidState& R, const ReidPass& P, const ReidBufs<_Float16>& B, ReidBlock<_Float16>& k) {
    const float* ss2 = P.rss + R.convs[k.i2].ss_off;
    { int rc = reid_gram_stats(c, R, P, k.i3, B.r2, ss2, k.h2, k.w2); if (rc) return rc; }
    if (k.b == 0 && k.fuse_ds) { int rc = reid_gram_stats(c, R, P, k.id, k.cur, k.cur_ss, k.H, k.W); if (rc) return rc; }
    if (k.b == 0 && k.fuse_ds && k.fuse_c1) { f16_tail_c1(R, P, B, k, true); return BUSCA_OK; }
    if (k.b == 0 && k.fuse_ds) {
        ConvCall<_Float16> q{k.i3, B.r2, ss2, k.h2, k.w2, k.nxt, CONV_MERGE_DS};
        q.ds_idx = k.id; q.ds_in = k.cur; q.dsH = k.H; q.dsW = k.W; q.ds_in_ss = k.cur_ss;
        return reid_f16_conv(c, R, P, q, &k.h3, &k.w3);
    }
    if (k.fuse_c1 && k.b > 0) { f16_tail_c1(R, P, B, k, false); return BUSCA_OK; }
    return reid_f16_conv(c, R, P, {k.i3, B.r2, ss2, k.h2, k.w2, k.nxt, CONV_MERGE, k.idt, k.ssd}, &k.h3, &k.w3);
}

// Tail, fp16 flavour without Gram statistics: conv3 twice - statistics-only pass, then a pass whose epilogue is the block tail (no raw3 tensor)
static int tail_f16_stats(busca_ctx* c, const ReidState& R, const ReidPass& P, const ReidBufs<_Float16>& B, ReidBlock<_Float16>& k) {
    const float* ss2 = P.rss + R.convs[k.i2].ss_off;
    if (!P.skip_stats) { int rc = reid_f16_conv(c, R, P, {k.i3, B.r2, ss2, k.h2, k.w2, B.r3, CONV_STATS_ONLY}, &k.h3, &k.w3); if (rc) return rc; }   // (the tail pass below sets h3 / w3 too)
    if (k.fuse_c1 && k.b > 0 && R.k.fuse_c1_small && (P.n * k.h2 * k.w2) % (k.li == 2 ? 64 : 128) == 0) {
        f16_tail_c1(R, P, B, k, false);       // the tail also runs the next bottleneck's conv1 (statistics came from the pass above)
        return BUSCA_OK;
    }
    return reid_f16_conv(c, R, P, {k.i3, B.r2, ss2, k.h2, k.w2, k.nxt, CONV_MERGE, k.idt, k.ssd}, &k.h3, &k.w3);
}

// Tail, split-fp16 flavour (layers in x3_merge_layers): BN3 statistics first - from the Gram matrix of conv3's 4x narrower input where that is built (64 / 128
// channels, tiles inside one crop), else a statistics-only pass of conv3 - then a pass whose epilogue is the block tail (the 4x wider raw tensor is never
// written or read back)
static int tail_x3_fused(busca_ctx* c, const ReidState& R, const ReidPass& P, const ReidBufs<float>& B, ReidBlock<float>& k) {
    const ReidKnobs& K = R.k; const ReidConv& c3 = R.convs[k.i3];
    const int n = P.n, h2 = k.h2, w2 = k.w2;
    const float* ss2 = P.rss + R.convs[k.i2].ss_off;
    if (K.x3_gram && (c3.cin == 64 || c3.cin == 128) && (h2 * w2) % 128 == 0 && (size_t)n * h2 * w2 * c3.cin >= (size_t)K.x3_gram_min && c3.cout % QF_CPB == 0) {
        int rc = c3.cin == 64 ? x3_gram_stats_c<64>(c, R, P, k.i3, B.r2, ss2, h2 * w2) : x3_gram_stats_c<128>(c, R, P, k.i3, B.r2, ss2, h2 * w2);
        if (rc) return rc;
    } else
    { int rc = reid_x3_conv(c, R, P, {k.i3, B.r2, ss2, h2, w2, B.r3, CONV_STATS_ONLY}, &k.h3, &k.w3); if (rc) return rc; }
    // layer 1: the tail pass also runs the next bottleneck's conv1 (256 -> 64, or layer 2's 256 -> 128) on the tile it holds - that conv never re-reads
    // the 4x wide block output (1.6 GB per 512 crops)
    const bool c1_in_tail = K.x3_fuse_c1 && c3.cout == 256 && k.inext < (int)R.convs.size() && R.convs[k.inext].k == 1 && R.convs[k.inext].stride == 1 &&
                            R.convs[k.inext].cin == 256 && (R.convs[k.inext].cout == 64 || R.convs[k.inext].cout == 128) &&
                            (size_t)n * h2 * w2 * 256 >= (size_t)K.x3_fuse_c1_min;
    ConvCall<float> q{k.i3, B.r2, ss2, h2, w2, k.nxt, CONV_MERGE, k.idt, k.ssd};
    if (c1_in_tail) { q.c1_idx = k.inext; q.c1_out = B.r1; }
    const int rc = reid_x3_conv(c, R, P, q, &k.h3, &k.w3);
    if (!rc && c1_in_tail) k.conv1_done = true;
    return rc;
}

// Tail, plain (exact f32; split-fp16 layers outside x3_merge_layers): raw conv3 output, then the merge pass - or, split-fp16, the merge deferred into the next conv1
template <class F>
static int tail_raw_merge(busca_ctx* c, const ReidState& R, const ReidPass& P, const ReidBufs<float>& B, ReidBlock<float>& k, ReidPending<float>& pend) {
    const ReidKnobs& K = R.k;
    { int rc = F::conv(c, R, P, {k.i3, B.r2, P.rss + R.convs[k.i2].ss_off, k.h2, k.w2, B.r3}, &k.h3, &k.w3); if (rc) return rc; }
    const int C = R.convs[k.i3].cout;
    const size_t npix = (size_t)P.n * k.h3 * k.w3;
    const float* ss3 = P.rss + R.convs[k.i3].ss_off; const bool last = k.i3 + 1 >= (int)R.convs.size();
    if (F::prec == BUSCA_PREC_F16X3 && K.x3_merge_in && !last && npix * C >= (size_t)K.x3_merge_in_min && R.convs[k.inext].k == 1 && R.convs[k.inext].stride == 1 && R.convs[k.inext].cout % 256 == 0) {
        pend.raw = B.r3; pend.ss = ss3; pend.idt = k.idt; pend.idt_ss = k.ssd; pend.out = k.nxt;
    } else
        ew_merge(P.s, (const float*)B.r3, ss3, k.idt, k.ssd, npix, C, k.nxt);
    return BUSCA_OK;
}

template <class F>
static int reid_forward_impl(busca_ctx* c, const uint8_t* crops, const uint8_t* zero_norm, int32_t n, const float* weights, double weight_sum, float* feats, void* stream,
                             const ReidBnMode& bn = ReidBnMode()) {
    using T = typename F::T;
    if (n < 0) return fail(c, BUSCA_EINVAL, "negative batch");
    if (n == 0) return BUSCA_OK;
    if (!crops || !feats) return fail(c, BUSCA_EINVAL, "null pointer");
    ReidState::WS* w = nullptr;
    { int rc = reid_ws_acquire(c, n, stream, sizeof(T), &w); if (rc) return rc; }
    const ReidState& R = *c->reid; const ReidKnobs& K = R.k;      // (from here on the forward only reads the extractor's state)
    ReidPass P;
    hipStream_t s = P.s = (hipStream_t)stream; P.n = n; P.wts = weights; P.wsum = weights != nullptr ? weight_sum : (double)n;
    // carve
    char* p = (char*)w->ptr;
    auto take = [&](size_t bytes) { char* q = p; p += (bytes + 255) & ~(size_t)255; return q; };
    const size_t nn = n;
    P.tickets = (int*)take(reid_ws::TICKET_BYTES);   // first block: its offset does not depend on n
    // every arrival counter is zero before the pass starts (a memset node ahead of the launches: a pass that was cut short - an error,
    // a cancelled stream - must not leave a ticket behind for the next one; the last arrivers also put theirs back to zero)
    P.ssb = (float*)take((size_t)2 * 26560 * 4);           // (scale, shift) of every BN channel of THIS batch; right behind the tickets: ONE memset node zeroes both (the
                                                           // split-fp16 flavour's end-of-pass scan for non-finite entries must never read a stale word)
    HIP_TRY(c, hipMemsetAsync(P.tickets, 0, reid_ws::TICKET_BYTES + (size_t)2 * 26560 * 4, s));
    // running-statistics pass (include/busca_reid_bn.h): the consumers read the extractor's fixed table.  The split-fp16 flavour keeps every statistics launch - they
    // write the workspace table, which the end-of-pass scan reads: an operand beyond its range is reported exactly as in a batch-statistics pass (DESIGN.md K-REID)
    P.rss = bn.running ? R.d_rss : P.ssb; P.skip_stats = bn.running && F::prec != BUSCA_PREC_F16X3;
    auto acts = [&](size_t per_crop) { return (T*)take(nn * per_crop * sizeof(T)); };
    ReidBufs<T> B;
    B.in4 = acts(reid_ws::IN4); B.stem = acts(reid_ws::STEM); B.x0 = acts(reid_ws::X0); B.r1 = acts(reid_ws::R1); B.r2 = acts(reid_ws::R2);
    B.r3 = acts(reid_ws::R3); B.rd = acts(reid_ws::RD); B.xa = acts(reid_ws::XA); B.xb = acts(reid_ws::XB);
    P.partials = (float*)take((nn * reid_ws::PART_FLOATS + 2 * 2 * 2048) * 4);
    B.pool = (float*)take(nn * 2048 * 4);
    P.red = (double*)take((size_t)BN_SLICES * 2 * 2048 * 8);
    take(nn * 512 * 4);                                   // (fc7: unused since the reduction writes the features in place)
    if constexpr (F::prec == BUSCA_PREC_F16) { P.gpart = (float*)take(reid_ws::GRAM_PART_FLOATS * 4); P.gG = (double*)take(reid_ws::GRAM_G_DOUBLES * 8); }
    else { P.x3part = (double*)take(reid_ws::X3_GRAM_PART_DOUBLES * 8); P.x3G = (double*)take(reid_ws::X3_GRAM_G_DOUBLES * 8); }
    if constexpr (F::prec == BUSCA_PREC_F16X3) {
        if (K.x3_stem_halo && K.x3_stem_u8 && R.d_x3_lut != nullptr) { P.stem_crops = crops; P.stem_zn = zero_norm; }
        if (K.x3_stem_halo && K.x3_stem_pool) { P.pool_p = B.x0; P.pool_q = B.stem; }
    }

    const float* x0_ss = nullptr;
    { int rc = reid_stem<F>(c, R, P, B, crops, zero_norm, &x0_ss); if (rc) return rc; }
    int ci = 1, H = 96, W = 32;
    T* cur = B.x0; T* nxt = B.xa;
    const int nblk[4] = {3, 4, 6, 3};
    bool conv1_done = false;
    ReidPending<T> pend;
    for (int li = 0; li < 4; ++li)
        for (int b = 0; b < nblk[li]; ++b) {
            ReidBlock<T> k{};
            k.li = li; k.b = b; k.i1 = ci; k.i2 = ci + 1; k.i3 = ci + 2; k.id = ci + 3; k.inext = ci + (b == 0 ? 4 : 3);
            k.cur = cur; k.cur_ss = (li == 0 && b == 0) ? x0_ss : nullptr; k.H = H; k.W = W; k.nxt = nxt;      // only the first bottleneck reads the (raw, pooled) stem tensor
            int h1, w1, hd, wd;
            // conv1
            if (conv1_done) { h1 = H; w1 = W; conv1_done = false; }            // produced by the previous block's fused tail
            else if (pend.out != nullptr) {
                ConvCall<T> q{k.i1, pend.raw, pend.ss, H, W, B.r1};
                q.mrg_idt = pend.idt; q.mrg_idt_ss = pend.idt_ss; q.mrg_out = pend.out;
                int rc = F::conv(c, R, P, q, &h1, &w1);
                if (rc) return rc;
                pend.out = nullptr;                      // cur (== the old pend.out) now holds the previous block's output
            }
            else { int rc = F::conv(c, R, P, {k.i1, cur, k.cur_ss, H, W, B.r1}, &h1, &w1); if (rc) return rc; }
            // conv2
            { int rc = F::conv(c, R, P, {k.i2, B.r1, P.rss + R.convs[k.i1].ss_off, h1, w1, B.r2}, &k.h2, &k.w2); if (rc) return rc; }
            // downsample conv of the layer's first block, unless the fp16 tail accumulates it
            const bool gram = reid_use_gram(R, P, li, n * k.h2 * k.w2, k.h2 * k.w2);
            k.fuse_ds = gram && K.gram_mode != 2 && ((K.fuse_ds_layers >> li) & 1);
            k.fuse_c1 = (li == 0 || (li <= K.fuse_c1_layers - 1 && b > 0)) && K.halo && K.fuse_c1;
            k.idt = cur; k.ssd = nullptr;
            if (b == 0 && !k.fuse_ds) {
                { int rc = F::conv(c, R, P, {k.id, cur, k.cur_ss, H, W, B.rd}, &hd, &wd); if (rc) return rc; }
                k.idt = B.rd; k.ssd = P.rss + R.convs[k.id].ss_off;
            }
            // tail
            int rc;
            if constexpr (F::prec == BUSCA_PREC_F16) rc = gram ? tail_f16_gram(c, R, P, B, k) : tail_f16_stats(c, R, P, B, k);
            else if (F::prec == BUSCA_PREC_F16X3 && ((K.x3_merge_layers >> li) & 1)) rc = tail_x3_fused(c, R, P, B, k);
            else rc = tail_raw_merge<F>(c, R, P, B, k, pend);
            if (rc) return rc;
            conv1_done = k.conv1_done; ci = k.inext; H = k.h3; W = k.w3;
            cur = nxt; nxt = (cur == B.xa) ? B.xb : B.xa;
        }
    ew_gpool(s, (const T*)cur, n, H * W, 2048, B.pool);
    if (n >= 128)
        hipLaunchKernelGGL((reid_tail_gemv_kernel<8>), dim3((n + 7) / 8, 8), dim3(256), 0, s, (const float*)B.pool, (const float*)(R.d_f + R.red_w_off),
                           (const float*)(R.d_f + R.red_b_off), feats, n);
    else
        hipLaunchKernelGGL((reid_tail_gemv_kernel<1>), dim3(n, 8), dim3(256), 0, s, (const float*)B.pool, (const float*)(R.d_f + R.red_w_off),
                           (const float*)(R.d_f + R.red_b_off), feats, n);
    // (split-fp16 flavour: the same launch scans this pass's BatchNorm (scale, shift) table and the features for non-finite values -> "reid_status")
    int* const flag = F::prec == BUSCA_PREC_F16X3 ? R.xerr_dev : (int*)nullptr;
    if (bn.output == BUSCA_REID_OUT_NORM) hipLaunchKernelGGL(reid_l2norm_kernel<false>, dim3(n), dim3(256), 0, s, feats, (const float*)P.ssb, 2 * 26560, flag);
    else hipLaunchKernelGGL(reid_l2norm_kernel<true>, dim3(n), dim3(256), 0, s, feats, (const float*)P.ssb, 2 * 26560, flag);
    if (bn.momentum != 0.0) {
        // train-mode update of the running statistics from this pass's finished table, then the fixed table again (reid_bn.hip.inc)
        ReidBnCounts m = R.bn_counts;
        for (int i = 0; i < REID_NCONV; ++i) m.count[i] *= (double)n;
        hipLaunchKernelGGL(reid_bn_update_kernel, dim3((26560 + 255) / 256), dim3(256), 0, s, (const float*)P.ssb, (const float*)R.d_f, R.bn_map, m, bn.momentum, R.d_run);
        hipLaunchKernelGGL(reid_bn_table_kernel, dim3((26560 + 255) / 256), dim3(256), 0, s, (const float*)R.d_run, (const float*)R.d_f, R.bn_map, R.d_rss);
    }
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}
