// "Unique rows" flavour of dt_fused_kernel (DESIGN.md "K-DT", Unique rows): one track per workgroup, unsplit, f32 / x3.  Included by dt_kernel.hip.inc
// (inside its fp-contract(off) region); instantiated by busca_dt_f32.hip / busca_dt_x3.hip through dt_launch, which owns the rule.
//
// With the separator encoded as the reference (DTParams::sep_can == 0) the SEP tokens of the P candidate pairs and of the NON pair are the same input row
// (tok_sep, reference box, the time bucket of their place in the pair), and an encoder without positional mask keeps equal rows equal through every layer.
// This kernel holds each distinct row once: U = T - P rows in NU = MT - 1 tiles,
//   rows 0 .. n-1         the decoder's rows (CAN 0 .. P-1, NON [, BAD]; n = P + nspec) - decoder row j at row j, as the pruned layer has it,
//   rows n .. n+L-1       the memory tokens,
//   row  n+L              the shared SEP,          row n+L+1  the BAD pair's SEP (fake box; nspec == 2 only),        then zero padding.
// Everything local to a token (embed, Q, attention queries, out-proj, LayerNorms, FFN) runs on these NU tiles - the text of dt_layer_tail.hip.inc with
// DT_NQL = NU, as the pruned layer uses it.  K and V are projected for all MT key tiles in the ORIGINAL token order: lane a of key tile i reads the operand row
// of the unique row that holds token 16 i + a (gemm_stream XT), so a duplicated key reads the bits of its original, K^T, V, every softmax sum and every
// P V product have the key order and the bits of dt_fused_kernel, and so has every row: logits, probabilities, argmax and the x3 range status are the same.
// No hidden states, no attention maps (such launches take dt_fused_kernel).
template <int PREC, int MT, int D, int FF, int E, int NCHUNK_FF>
__global__ void __launch_bounds__(256, 1) dt_fused_unique_kernel(const DTParams p) {
    typedef Prec<PREC> PR;
    typedef typename AttPrec<PREC>::type APR;
    static_assert(PREC != 1 && MT >= 2, "unique rows: the f32 / x3 flavours of two token tiles or more");
    constexpr int NU = MT - 1;              // row tiles of the workgroup
    // what the layer tail's text reads of the flavour: one track, not split, residual in registers; MTL != DT_NQL: no attention maps
    // (SPLIT / TWO depend on a template parameter so that their branches of the tail are discarded, not compiled)
    constexpr int NTRK = 1, MTL = MT;
    constexpr bool SPLIT = MT < 0, TWO = MT < 0;
    typedef DTLds<PREC, NU, D, FF, E, NCHUNK_FF, 1> LD;
    constexpr int EP = PR::EP, CHUNK = PR::CHUNK, CW = PR::CW;
    constexpr int TP = 16 * NU;
    constexpr int HD = D / 4, NTW = D / 64, FT = HD / 16;
    constexpr int KC_D = D / CHUNK, KC_E = E / CHUNK, KC_FFC = LD::FFC / CHUNK, KC_FF = FF / CHUNK;
    constexpr int FTW = LD::FFC / 64;
    constexpr int WMAX = NTW > 4 ? 8 : 4;
    constexpr int QNW = FT;
    constexpr int FSUB = FTW > WMAX ? WMAX : FTW;
    constexpr int RSP = D * 4 + 16;         // row stride of the f32 residual parked in HB (pruned last layer)
    constexpr int NSUB = FTW / FSUB;
    constexpr int XM = (PREC != 0 && D == 256 && MT <= 3) ? 1 : 0;
    constexpr int PF = PREC == 2 ? 2 : (WMAX == 8 ? 2 : (KC_D >= 4 ? 4 : KC_D));
    constexpr int NCF = APR::nchunks(FT), NCK = APR::nchunks(MT);
    static_assert(FT == NTW && FTW % FSUB == 0 && KC_E % PF == 0 && KC_FFC % PF == 0, "geometry");
    static_assert(16 * NU * RSP <= LD::HB_BYTES, "pruned layer: the parked residual does not fit HB");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* xop = smem + LD::OFF_XOP;
    char* hb = smem + LD::OFF_HB;
    float* red1 = (float*)(smem + LD::OFF_RED1);
    float* red2 = (float*)(smem + LD::OFF_RED2);
    int* ids = (int*)(smem + LD::OFF_IDS);

    const int trk = blockIdx.x;             // (the grid is the launch's one-workgroup tracks: every index is a track)
    const int tile = 0, xslot = 0, tok0 = 0;                    // (read by the SPLIT / attention-map branches of the tail only)
    auto track_of = [&](int) { return trk; };
    auto park_x = [&]() {};
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int a = lane & 15, b = lane >> 4;
    const int L = p.L, P = p.P, T = p.T;
    const int n = P + p.nspec, U = T - P;   // decoder rows, unique rows (the host launches this kernel only where U <= 16 NU)
    const int fbase = wave * (D / 4);
    const bool prune = p.prune != 0;

    // unique row -> token of the track (T: a padding row), token -> the unique row that holds it (a padded key: a padding row where there is one, else the
    // last row - its score is masked and its probability is an exact zero, the row only has to be finite)
    auto tok_of = [&](int u) {
        if (u < n) return L + 2 * u + p.can_pos;
        if (u < n + L) return u - n;
        if (u == n + L) return L + 2 * P + 1 - p.can_pos;                            // the NON pair's SEP stands for all P + 1
        if (u == n + L + 1 && p.nspec == 2) return L + 2 * (P + 1) + 1 - p.can_pos;
        return T;
    };
    auto row_of = [&](int t) {
        if (t >= T) return U < TP ? U : TP - 1;
        if (t < L) return n + t;
        const int k = t - L, j = k >> 1;
        if ((k & 1) == p.can_pos) return j;
        return (p.nspec == 2 && j == P + 1) ? n + L + 1 : n + L;
    };

    const u32x4* w_emb = p.w_embed + (size_t)(wave * NTW) * KC_E * CW + lane;
    auto wq_of = [&](const DTLayerW& W, int part) { return W.w_in + (size_t)((part * D + wave * HD) / 16) * KC_D * CW + lane; };

    typename PR::op_t wf[PF][WMAX];
    bool clipped = false;
    DT_STAMP(0);
    gemm_prefetch<PREC, NTW, PF, WMAX>(wf, w_emb, KC_E * CW);

    // ---- P0: bucket ids + the ReID features, in unique-row order ---------------------------------------------------
    if (tid < TP) {
        int ixy = 0, isz = 0, it = 0;
        const int t = tok_of(tid);
        if (t < T) token_bucket(p.mem_ltrb, p.can_ltrb, trk, t, L, P, p.fake_f64, p.can_pos, p.nspec, p.sep_can, ixy, isz, it);
        ids[tid] = ixy; ids[TP + tid] = isz; ids[2 * TP + tid] = it;
    }
    {
        constexpr int NPC = TP * (E / 4) / 256;
        constexpr int NB = NPC > 24 ? NPC / 2 : NPC;
        static_assert(NPC % NB == 0, "staging batches");
#pragma unroll
        for (int q0 = 0; q0 < NPC; q0 += NB) {
            f32x4 v[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int i = tid + 256 * (q0 + q);
                const int row = i / (E / 4), e4 = i % (E / 4);
                const int t = tok_of(row);
                // (loaded unconditionally, rows without a feature multiplied by zero: see dt_fused_kernel)
                const int k = t - L, j = k >> 1;
                const bool is_mem = t < L, is_can = !is_mem && t < T && (k & 1) == p.can_pos && j < P;
                const float* src = is_can ? p.can_feat + ((size_t)trk * P + j) * E + e4 * 4 : p.mem_feat + ((size_t)trk * L + (is_mem ? t : 0)) * E + e4 * 4;
                const f32x4 ld = *(const f32x4*)src;
                v[q] = ld * ((is_mem || is_can) ? 1.0f : 0.0f);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int i = tid + 256 * (q0 + q);
                clipped |= PR::store4(hb + (i / (E / 4)) * LD::RSE + (i % (E / 4)) * 4 * EP, v[q], (LD::RSE - 16) / 2);
            }
        }
    }
    __syncthreads();
    DT_STAMP(1);

    // ---- P1: token embed + assembly + encoding -> X in registers ------------------------------------------------------
    f32x4 X[NTW][NU];
    {
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
            for (int tt = 0; tt < NU; ++tt) X[ft][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        gemm_stream<PREC, NTW, NU, KC_E, PF, true, QNW, WMAX, XM>(X, wf, w_emb, KC_E * CW, hb + a * LD::RSE + b * 16, LD::RSE, wq_of(p.layer[0], 1), KC_D * CW);
        DT_STAMP(2);
        const float sq = sqrtf((float)D);
        const int c = p.lut_c;
#pragma unroll
        for (int tt = 0; tt < NU; ++tt) {
            const int row = 16 * tt + a;
            const int t = tok_of(row);
            int kind;  // 0 embed row, 1 SEP, 2 NON, 3 BAD, 4 padding
            if (t >= T) kind = 4;
            else if (t < L) kind = 0;
            else { const int k = t - L, j = k >> 1; kind = (k & 1) == p.can_pos ? (j < P ? 0 : (j == P ? 2 : 3)) : 1; }
            const _Float16* rxy = p.lut_xy + ids[row] * c;
            const _Float16* rsz = p.lut_sz + ids[TP + row] * c - c;
            const _Float16* rt = p.lut_t + ids[2 * TP + row] * c - 2 * c;
            const float* tokv = kind == 2 ? p.tok_non : (kind == 3 ? p.tok_bad : p.tok_sep);
#pragma unroll
            for (int ft = 0; ft < NTW; ++ft) {
                const int f0 = fbase + 16 * ft + 4 * b;
                const f32x4 be = *(const f32x4*)(p.b_embed + f0);
                const f32x4 tk = *(const f32x4*)(tokv + f0);
                const f32x4 xu = PR::unscale(X[ft][tt]);
                f32x4 enc;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = f0 + r;
                    const _Float16* src = f < c ? rxy : (f < 2 * c ? rsz : rt);
                    enc[r] = (float)src[f];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float base = kind == 0 ? (xu[r] + be[r]) * sq : tk[r];
                    X[ft][tt][r] = kind == 4 ? 0.f : base + enc[r];
                }
            }
        }
    }
    clipped |= store_rows<PREC, NTW, NU>(X, xop, LD::RSX, a, b, fbase);
    __syncthreads();
    DT_STAMP(3);

    const float invD = 1.0f / (float)D;
    const float qscale = 1.0f / sqrtf((float)HD);
    // byte offset of the operand row that this lane reads for key tile i: the unique row of token 16 i + a
    int koff[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) koff[i] = row_of(16 * i + a) * LD::RSX;

    // ---- encoder layers: K and V on all MT key tiles, everything else on the NU unique tiles --------------------------------
#pragma unroll 1
    for (int l = 0; l < p.nlayers; ++l) {
        const DTLayerW& W = p.layer[l];
        const DTLayerW& Wn = p.layer[l + 1 < p.nlayers ? l + 1 : l];
        const u32x4* w_out = W.w_out + (size_t)(wave * NTW) * KC_D * CW + lane;
        const int sl = 4 + 12 * l;
        u32x4 qf[NU][NCF], kf[MT][NCF], vf[1][FT][NCK];
        f32x4 kown[1][FT], vown[1][FT];                               // (SPLIT only)
        constexpr size_t XW = 0; const unsigned xstamp = 0;           // (SPLIT only)
        const char* xl = xop + a * LD::RSX + b * 16;
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        {
            f32x4 acc[FT][MT];
            f32x4 bk[FT]; float bv[FT];
            load_vec4<FT>(bk, W.b_in, D + wave * HD + 4 * b);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                for (int tt = 0; tt < MT; ++tt) acc[ft][tt] = zero4;
            gemm_stream<PREC, FT, MT, KC_D, PF, true, FT, WMAX, XM, true>(acc, wf, wq_of(W, 1), KC_D * CW, xop + b * 16, LD::RSX, wq_of(W, 2), KC_D * CW, koff);
            DT_STAMP(sl + 0);
#pragma unroll
            for (int tt = 0; tt < MT; ++tt) {
                f32x4 tl[FT];
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) tl[ft] = PR::unscale(acc[ft][tt]) + bk[ft];
#pragma unroll
                for (int c = 0; c < NCF; ++c) kf[tt][c] = APR::template frag<FT>(tl, c);
            }
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) bv[ft] = W.b_in[2 * D + wave * HD + 16 * ft + a];
#pragma unroll
            for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                for (int tt = 0; tt < MT; ++tt) acc[ft][tt] = zero4;
            gemm_stream<PREC, FT, MT, KC_D, PF, false, FT, WMAX, XM, true>(acc, wf, wq_of(W, 2), KC_D * CW, xop + b * 16, LD::RSX, wq_of(W, 0), KC_D * CW, koff);
            DT_STAMP(sl + 1);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                f32x4 tl[MT];
#pragma unroll
                for (int tt = 0; tt < MT; ++tt) tl[tt] = PR::unscale(acc[ft][tt]) + bv[ft];
#pragma unroll
                for (int c = 0; c < NCK; ++c) vf[0][ft][c] = APR::template frag<MT>(tl, c);
            }
        }
        if (prune && l == p.nlayers - 1) {
            // Pruned last layer: the decoder reads rows 0 .. n-1 only; the rows above them replicate row n-1 and are discarded, so that the layer's operands - and
            // with them the x3 range status - are those of dt_fused_kernel's pruned layer.  Through HB as f32 (dead at a layer's start).
#pragma unroll
            for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
                for (int tt = 0; tt < NU; ++tt) *(f32x4*)(hb + (16 * tt + a) * RSP + (fbase + 16 * ft + 4 * b) * 4) = X[ft][tt];
            __syncthreads();               // every wave is done reading Xop (K, V); the parked rows are visible
#pragma unroll
            for (int tt = 0; tt < NU; ++tt) {
                const int r = 16 * tt + a < n ? 16 * tt + a : n - 1;
#pragma unroll
                for (int ft = 0; ft < NTW; ++ft) X[ft][tt] = *(const f32x4*)(hb + r * RSP + (fbase + 16 * ft + 4 * b) * 4);
            }
            clipped |= store_rows<PREC, NTW, NU>(X, xop, LD::RSX, a, b, fbase);
            __syncthreads();
        }
        {
            f32x4 acc[FT][NU];
            f32x4 bq[FT];
            load_vec4<FT>(bq, W.b_in, wave * HD + 4 * b);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                for (int tt = 0; tt < NU; ++tt) acc[ft][tt] = zero4;
            gemm_stream<PREC, FT, NU, KC_D, PF, true, NTW, WMAX, XM>(acc, wf, wq_of(W, 0), KC_D * CW, xl, LD::RSX, w_out, KC_D * CW);
            DT_STAMP(sl + 2);
#pragma unroll
            for (int tt = 0; tt < NU; ++tt) {
                f32x4 tl[FT];
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) tl[ft] = (PR::unscale(acc[ft][tt]) + bq[ft]) * qscale;
#pragma unroll
                for (int c = 0; c < NCF; ++c) qf[tt][c] = APR::template frag<FT>(tl, c);
            }
        }
#define DT_NQL NU
#define DT_NQT NU
#define DT_XQ X
#define DT_KNEXT true
#include "dt_layer_tail.hip.inc"
#undef DT_NQL
#undef DT_NQT
#undef DT_XQ
#undef DT_KNEXT
    }

    // ---- epilogue: decoder LN + Linear(d,1), softmax, argmax; candidate j sits in row j ---------------------------------------
    {
        f32x4 dg[NTW], db[NTW];
        load_vec4<NTW>(dg, p.dec_g, fbase + 4 * b);
        load_vec4<NTW>(db, p.dec_b, fbase + 4 * b);
        layer_norm_regs<NTW, NU>(X, dg, db, red1, red2, wave, a, b, invD);
    }
    f32x4 dw[NTW];
    load_vec4<NTW>(dw, p.dec_w, fbase + 4 * b);
#pragma unroll
    for (int tt = 0; tt < NU; ++tt) {
        float s = 0.f;
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft) {
#pragma unroll
            for (int r = 0; r < 4; ++r) s = dt_fma(X[ft][tt][r], dw[ft][r], s);
        }
        s = xor_sum_b(s);
        if (b == 0) red1[wave * TP + 16 * tt + a] = s;
    }
    __syncthreads();
    if (wave == 0) {
        float lg = -INFINITY;
        if (lane < n) {
            lg = ((red1[lane] + red1[TP + lane]) + (red1[2 * TP + lane] + red1[3 * TP + lane])) + p.dec_bias;
            p.logits[(size_t)trk * n + lane] = lg;
        }
        float m = lg;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const float e = lane < n ? expf(lg - m) : 0.f;
        float sum = e;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
        const float pr = e / sum;
        if (p.probs != nullptr && lane < n) p.probs[(size_t)trk * n + lane] = pr;
        float bv = lane < n ? pr : -1.f;
        int bi = lane;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (p.argmax != nullptr && lane == 0) p.argmax[trk] = bi;
    }
    if (PREC == 2 && clipped && p.xerr != nullptr) *p.xerr = 2;
    DT_STAMP(4 + 12 * DT_MAX_LAYERS);
}
