// Host-side state of the ReID extractor: what a loaded extractor owns (ReidState), its schedule knobs and the ONE table that names them
// (ReidKnobs / REID_KNOBS), and what belongs to a single forward (ReidPass).
struct ReidConv { int cout, cin, k, stride, pad; size_t w_off, g_off, b_off, ss_off; size_t wpk_off = (size_t)-1; size_t wkw_off = (size_t)-1;
                  size_t wx3_off = (size_t)-1, inv_off = 0; };   // F16X3: hi / lo fragment-ordered weights (halves into d_wx3), per-channel descale (floats into d_f)   // offsets into dev arrays; wpk: fragment-packed copy (reid_halo.hip.inc)

// Schedule knobs: defaults here, names in REID_KNOBS below (the list of record).  A (re)load starts from these defaults + the environment.
struct ReidKnobs {
    int gram_mode = -1;               // -1 auto (large batches), 0 never, 1 always (see reid_gram.hip.inc)
    int gram_min_pixels = 65536;      // Gram statistics from this many output pixels on
    int direct_rows = 512;            // statistics of up to this many tiles are reduced + finalised by ONE launch
    bool two_launch_stats = false;    // 1: separate reduce + finalise launches beyond direct_rows (A/B; default: one launch, last arriver finalises)
    int fuse_ds_layers = 3;           // bit l: the first block of layer l+1 accumulates its downsample conv inside the fused tail (Gram statistics for its BatchNorm);
                                      // 0 bits: separate raw-output conv.  Layer 3 is NOT fused since round 3: its downsample as a conv_pipe_kernel launch (131 us) + a plain
                                      // fused-tail pass replace the 170 us Gram chain of the branch and the two-accumulator tail: 512 crops 8.30 -> 8.14 ms
    bool fuse_c1 = true;              // 0: tails without the fused next conv1 (A/B testing); BUSCA_REID_FUSE_C1=1/2/3 also sets fuse_c1_layers
    int fuse_c1_layers = 2;           // layer 3 (64-pixel tiles, 16 waves) measured slower: 9.76 -> 10.25 ms at 512 crops; opt-in with BUSCA_REID_FUSE_C1=3
    bool fuse_c1_small = true;        // fused tail + next conv1 also behind a statistics-only pass (small batches, no Gram)
    bool halo = true;                 // 0 disables the halo-resident 3x3 kernel (A/B testing)
    int halo_min_blocks = 128;        // halo 3x3 kernel from this many workgroups on (below: generic / split-K)
    int halo_wpx = 1;                 // layer 1's 3x3: 2 x 2-wave halo kernel on 256-pixel tiles (0: never)
    int halo_wpx_min = 5120;          // ... from this many 256-pixel tiles on (427 crops)
    int halo_half_blocks = 384;       // layer-3 halo kernel on half images below this many full-image workgroups
    int pipe_min_tiles = 192;         // conv_pipe_kernel (reid_pipe.hip.inc) for raw-output convs from this many 128-pixel x 256-channel tiles on (0 = never)
    int pipe_half_blocks = 448;       // ... on 64-pixel tiles while 128-pixel tiles would give fewer workgroups than this (0 = never)
    bool pipe_all = false;            // ... for every eligible conv instead of the shapes where it measured faster (tests;
                                      // the default: measured equal to the tiled kernel, 83 vs 85 us per layer-3/4 conv1 at 512 crops)
    int kwave_blocks = 288;           // conv_kwave_kernel instead of the LDS-tiled kernel below this many 128x128 tiles (0 = never)
    int kwave_halo_blocks = 0;        // ... also instead of the halo 3x3 kernel below this many tiles
    double kwave_max_mb = 600.0;      // ... and only while its operand traffic per launch stays below this many MB
    int kwave_nw = 0, kwave_pt = 0;   // forced waves per workgroup / pixel fragments per tile (experiments; 0 = automatic)
    // split-fp16 flavour (BUSCA_PREC_F16X3)
    int x3_merge_layers = 3;          // bit l = layer l+1 runs conv3 as statistics pass + fused-tail pass (no raw conv3 tensor) instead of raw output + merge pass
    int x3_half_blocks = -1;          // 64-pixel tiles while 128-pixel tiles would give fewer workgroups than this (0 = never; -1 = by the number of workgroup rounds, see reid_x3_conv)
    int x3_ptail_min = 128;           // the fused tails of layers 1-2 run as PERSISTENT workgroups (reid_x3p.hip.inc) from this many (128-pixel tile, 256-channel block)
                                      // work items up (measured: 22 crops 2.212 -> 2.198 ms, 40 crops 2.595 -> 2.558 against 512); 0 = never
    bool x3_gram = true;              // BN3 statistics of layers 1-2 from the Gram matrix of conv3's input (x3_gram_kernel) instead of a statistics-only conv pass
    int x3_gram_min = 4 << 20;        // ... and only from this many input elements (pixels x channels) up: below, the statistics-only pass is faster
    bool x3_merge_in = true;          // a block tail that is not a conv3 epilogue is formed by the NEXT conv1 while it stages (0: block_merge pass)
    int x3_merge_in_min = 8 << 20;    // ... from this many block-output elements up (below, the separate pass is as fast)
    bool x3_fuse_c1 = true;           // layer 1's fused tails also run the next bottleneck's conv1 (X3_MERGE_C1)
    int x3_fuse_c1_min = 0;           // ... from this many block-output elements up
    int x3_row3 = 1;                  // stride-1 3x3 convs of layers 1-2 stage once per kernel row (ROW3; 0: once per tap; 2: also 64-pixel tiles in layers 3-4)
    int x3_narrow3 = 200;             // 3x3 convs with fewer 64-pixel x 256-channel workgroups than this run on 64 x 128 four-wave workgroups (0 = never; 32 crops 2.60 -> 2.47 ms, equal at 88, slower from ~100)
    bool x3_stem_halo = true;         // the stem stages its input rows once per tile as an LDS halo (STEMH; 0: tap by tap)
    bool x3_stem_u8 = true;           // the stem reads the u8 crops itself (0: through the normalised float copy)
    bool x3_stem_pool = true;         // the stem writes the max pool of its raw output instead of the raw map (0: raw map + pooling pass)
};

// One entry per knob: the environment variable busca_reid_load_weights reads, the busca_set_option / busca_get_option name (NULL: environment only - A/B runs;
// named: the ones a test flips between two forwards of a loaded extractor, tests/test_reid_gpu.py) and the field, whose type says how a value is taken:
// int as it is, bool as `!= 0`, double through atof.
struct ReidKnobDesc {
    const char* env; const char* opt;
    int ReidKnobs::*i = nullptr; bool ReidKnobs::*b = nullptr; double ReidKnobs::*d = nullptr;
    constexpr ReidKnobDesc(const char* e, const char* o, int ReidKnobs::*p) : env(e), opt(o), i(p) {}
    constexpr ReidKnobDesc(const char* e, const char* o, bool ReidKnobs::*p) : env(e), opt(o), b(p) {}
    constexpr ReidKnobDesc(const char* e, const char* o, double ReidKnobs::*p) : env(e), opt(o), d(p) {}
    void from_text(ReidKnobs& k, const char* t) const { if (i) k.*i = atoi(t); else if (b) k.*b = atoi(t) != 0; else k.*d = atof(t); }
    void set(ReidKnobs& k, int32_t v) const { if (i) k.*i = v; else if (b) k.*b = v != 0; else k.*d = (double)v; }
    int32_t get(const ReidKnobs& k) const { return i ? k.*i : b ? (k.*b ? 1 : 0) : (int32_t)(k.*d); }
};
static const ReidKnobDesc REID_KNOBS[] = {
    // fp16 flavour: BatchNorm statistics
    {"BUSCA_REID_GRAM", "reid_gram", &ReidKnobs::gram_mode}, {"BUSCA_REID_GRAM_MIN", nullptr, &ReidKnobs::gram_min_pixels},
    {"BUSCA_REID_DIRECT_ROWS", nullptr, &ReidKnobs::direct_rows}, {"BUSCA_REID_STATS2", nullptr, &ReidKnobs::two_launch_stats},
    // ... fused tails (BUSCA_REID_FUSE_C1 also sets fuse_c1_layers: reid_knobs_from_env)
    {"BUSCA_REID_FUSE_DS_LAYERS", nullptr, &ReidKnobs::fuse_ds_layers}, {"BUSCA_REID_FUSE_C1", "reid_fuse_c1", &ReidKnobs::fuse_c1},
    {"BUSCA_REID_FUSE_C1_SMALL", nullptr, &ReidKnobs::fuse_c1_small},
    // ... which conv kernel
    {"BUSCA_REID_HALO", "reid_halo", &ReidKnobs::halo}, {"BUSCA_REID_HALO_MIN", nullptr, &ReidKnobs::halo_min_blocks}, {"BUSCA_REID_HALO_HALF", nullptr, &ReidKnobs::halo_half_blocks},
    {"BUSCA_REID_HALO_WPX", nullptr, &ReidKnobs::halo_wpx}, {"BUSCA_REID_HALO_WPX_MIN", nullptr, &ReidKnobs::halo_wpx_min},
    {"BUSCA_REID_PIPE_MIN", nullptr, &ReidKnobs::pipe_min_tiles}, {"BUSCA_REID_PIPE_ALL", nullptr, &ReidKnobs::pipe_all}, {"BUSCA_REID_PIPE_HALF", nullptr, &ReidKnobs::pipe_half_blocks},
    {"BUSCA_REID_KWAVE_BLOCKS", nullptr, &ReidKnobs::kwave_blocks}, {"BUSCA_REID_KWAVE_HALO", nullptr, &ReidKnobs::kwave_halo_blocks}, {"BUSCA_REID_KWAVE_MB", nullptr, &ReidKnobs::kwave_max_mb},
    {"BUSCA_REID_KWAVE_NW", nullptr, &ReidKnobs::kwave_nw}, {"BUSCA_REID_KWAVE_PT", nullptr, &ReidKnobs::kwave_pt},
    // split-fp16 flavour
    {"BUSCA_REID_X3_MERGE_LAYERS", nullptr, &ReidKnobs::x3_merge_layers}, {"BUSCA_REID_X3_HALF", nullptr, &ReidKnobs::x3_half_blocks}, {"BUSCA_REID_X3_PTAIL", "reid_x3_ptail", &ReidKnobs::x3_ptail_min},
    {"BUSCA_REID_X3_GRAM", nullptr, &ReidKnobs::x3_gram}, {"BUSCA_REID_X3_GRAM_MIN", "reid_x3_gram_min", &ReidKnobs::x3_gram_min},
    {"BUSCA_REID_X3_MERGE_IN", nullptr, &ReidKnobs::x3_merge_in}, {"BUSCA_REID_X3_MERGE_IN_MIN", "reid_x3_merge_in_min", &ReidKnobs::x3_merge_in_min},
    {"BUSCA_REID_X3_FUSE_C1", "reid_x3_fuse_c1", &ReidKnobs::x3_fuse_c1}, {"BUSCA_REID_X3_FUSE_C1_MIN", nullptr, &ReidKnobs::x3_fuse_c1_min},
    {"BUSCA_REID_X3_ROW3", "reid_x3_row3", &ReidKnobs::x3_row3}, {"BUSCA_REID_X3_NARROW3", nullptr, &ReidKnobs::x3_narrow3},
    {"BUSCA_REID_X3_STEM_HALO", "reid_x3_stem_halo", &ReidKnobs::x3_stem_halo}, {"BUSCA_REID_X3_STEM_U8", "reid_x3_stem_u8", &ReidKnobs::x3_stem_u8},
    {"BUSCA_REID_X3_STEM_POOL", "reid_x3_stem_pool", &ReidKnobs::x3_stem_pool},
};
static const ReidKnobDesc* reid_knob_by_option(const char* name) {
    for (const ReidKnobDesc& e : REID_KNOBS) if (e.opt && !strcmp(e.opt, name)) return &e;
    return nullptr;
}
static void reid_knobs_from_env(ReidKnobs& k) {
    for (const ReidKnobDesc& e : REID_KNOBS) if (const char* t = getenv(e.env)) e.from_text(k, t);
    // the one irregular knob: BUSCA_REID_FUSE_C1=N (N > 0) is also the last layer whose tails carry the next conv1
    if (const char* t = getenv("BUSCA_REID_FUSE_C1")) if (atoi(t) > 0) k.fuse_c1_layers = std::min(3, std::max(1, atoi(t)));
}

struct ReidState {
    bool loaded = false;
    int prec = BUSCA_PREC_F16;        // element type of activations / conv weights
    ReidKnobs k;
    std::vector<ReidConv> convs;      // forward order (53); w_off in ELEMENTS
    void* d_w = nullptr;              // all packed conv weights (fp16 or f32)
    _Float16* d_wpk = nullptr;        // fragment-ordered copies of the stride-1 3x3 and stem weights + stem byte table (fp16 flavour)
    _Float16* d_wkw = nullptr;        // fragment-ordered copies of every non-stem conv, half-step major (reid_kwave.hip.inc)
    _Float16* d_wx3 = nullptr;        // F16X3: hi / lo fragment-ordered, per-channel pre-scaled copies of every conv (reid_x3.hip.inc)
    unsigned* d_x3_lut = nullptr;     // F16X3: [3][256] pre-split normalised values of the stem's byte input (reid_x3.hip.inc STEMH)
    size_t stem_wpk_off = 0, stem_lut_off = 0;
    float* d_f = nullptr;             // gamma/beta for every BN, red weight^T [2048][512], red bias
    float* d_ss = nullptr;            // scale/shift per BN channel [sum C][2]
    size_t red_w_off = 0, red_b_off = 0;
    unsigned long long stem_negmask = 0;   // bit c: the stem BatchNorm's gamma of channel c is negative (stem_pool_kernel pools it with min)
    void* d_zero = nullptr;           // 256 zero bytes: the load target of padded / out-of-range operand pieces
    int num_cu = 256;                 // compute units of the device (persistent launches: one workgroup per CU)
    // running-statistics BatchNorm (include/busca_reid_bn.h): absent until busca_reid_load_running_stats / _reset_running_stats, dropped with the weights
    float* d_run = nullptr;           // per conv in blob order running_mean[Cout], running_var[Cout]
    float* d_rss = nullptr;           // the FIXED (scale, shift) table built from them, laid out as a pass's own table ([sum C][2])
    bool run_loaded = false;
    ReidBnMap bn_map{};               // which channels, affine parameters and output pixels per crop each conv's BatchNorm has (reid_bn.hip.inc)
    ReidBnCounts bn_counts{};
    int* xerr = nullptr; int* xerr_dev = nullptr;    // F16X3: status word in host-mapped memory ("reid_status": 2 = a staged operand left the fp16 range in a forward since it was last cleared)
    // workspaces: one per stream that has called busca_reid_forward (the two BN batches of a step may run
    // concurrently on two streams); reused, grown on demand
    struct WS { void* stream = nullptr; void* ptr = nullptr; size_t bytes = 0; int n = 0; };
    WS ws[4];
};

// What belongs to ONE forward: built on the stack of reid_forward_impl while it enqueues and handed to the helpers by reference, so two forwards that are
// enqueued at the same time (two streams, a workspace each) share nothing but the read-only ReidState.
struct ReidPass {
    hipStream_t s = nullptr; int n = 0;                              // stream, crops
    const float* wts = nullptr; double wsum = 0.0;                   // per-crop multiplicities (busca_reid_forward_w; else NULL) and their sum (= n without weights)
    int* tickets = nullptr;                                          // arrival counters: [conv][64-channel column] of bn_reduce_finalize_kernel, then [conv][16-channel group] of bn_quadform_kernel
    const uint8_t* stem_crops = nullptr; const uint8_t* stem_zn = nullptr;   // F16X3 stem with byte input: the crops / padding flags
    const float* pool_p = nullptr; float* pool_q = nullptr;          // F16X3: the pooled stem parts (X3_POOL / X3_POOLIN)
    float *ssb = nullptr, *partials = nullptr; double* red = nullptr;   // (scale, shift) of every BN channel of THIS batch; per-tile statistics of the running conv, their slice sums
    // Two tables: `ssb` (workspace) is what the statistics finalisers WRITE and reid_l2norm_kernel scans; `rss` is what every consumer of a BatchNorm READS -
    // ssb itself in a batch-statistics pass, the extractor's fixed table (ReidState::d_rss) in a running-statistics pass.
    const float* rss = nullptr;
    bool skip_stats = false;                                         // running-statistics pass of the exact-f32 / fp16 flavours: nothing whose only product is statistics is launched
    float* gpart = nullptr; double* gG = nullptr; double *x3part = nullptr, *x3G = nullptr;   // Gram scratch of the fp16 (gram_stats_launch) / split-fp16 (x3_gram_stats_c) flavour
};

static void reid_free(ReidState& r) {
    if (r.d_w) hipFree(r.d_w);
    if (r.d_wpk) hipFree(r.d_wpk);
    if (r.d_wkw) hipFree(r.d_wkw);
    if (r.d_wx3) hipFree(r.d_wx3);
    if (r.d_x3_lut) { hipFree(r.d_x3_lut); r.d_x3_lut = nullptr; }
    if (r.d_f) hipFree(r.d_f);
    if (r.d_ss) hipFree(r.d_ss);
    if (r.d_run) hipFree(r.d_run);
    if (r.d_rss) hipFree(r.d_rss);
    if (r.d_zero) hipFree(r.d_zero);
    for (auto& w : r.ws) if (w.ptr) hipFree(w.ptr);
    if (r.xerr) hipHostFree(r.xerr);
    r = ReidState();
}
