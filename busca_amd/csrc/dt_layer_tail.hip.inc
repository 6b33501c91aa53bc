// One encoder layer of dt_fused_kernel from the attention on: softmax(Q K^T) V, out-proj + LayerNorm1, FFN + LayerNorm2.  Included by dt_kernel.hip.inc INSIDE the
// kernel body (and by dt_unique_kernel.hip.inc inside its own), once per row-tile count: the text is the same for a full layer, for the pruned last layer (DTParams::prune)
// and for the layers of the unique-rows kernel, so every row sees the same
// products in the same order whichever tile and lane hold it.  (Text inclusion rather than a generic lambda: with the lambda hipcc allocated registers
// differently in EVERY flavour of the kernel - the f16 and d = 512 ones gained scratch; as included text the flavours that do not prune keep their instruction stream.)
// The including scope defines
//   DT_NQL    query / row tiles per track (MTL in a full layer, MT - 1 in the pruned layer and in the unique-rows kernel), DT_NQT = DT_NQL * NTRK those of the workgroup,
//   DT_XQ     the residual stream f32x4 [NTW][DT_NQT],
//   DT_KNEXT  whether the GEMM that follows this layer in the weight stream is a K projection (SPLIT, or the pruned layer comes next) rather than a Q projection,
// and the layer's l, sl, W, Wn, w_out, xstamp, XW, qf[DT_NQT][NCF], kf, vf (all MT key tiles), kown, vown (SPLIT).
        // -- A2: S^T = K Q^T, softmax over keys, O^T = V^T P^T, all in registers -----------------------------------
        // SPLIT: the other tiles of the track(s), in token order (this workgroup's own slot is waited for and read like the others - its values are then
        // taken from the registers -, so that no access depends on which tile this is).  One poll covers every flag, one batch of loads every tile.
        f32x4 kt[SPLIT ? NTRK : 1][SPLIT ? MT : 1][FT], vt[SPLIT ? NTRK : 1][SPLIT ? MT : 1][FT];
        if constexpr (SPLIT) {
            // Take: wave 0 waits for the flags of every tile of the track(s) and acquires at agent scope (buffer_inv sc1: this CU's L1) ONCE for the workgroup; the
            // workgroup barrier behind it orders the other waves' loads after that acquire.  A tile's flag is raised by its workgroup's wave 0 after ALL four
            // waves' stores (barrier + release above), so one flag per (track, tile) covers the four heads.
            if (wave == 0) dt_xwait<MT, NTRK>(p.xflag + (size_t)xslot * MT * DT_XFLAGS, DT_XFLAGS, xstamp, p.xerr, MT * DT_XFLAGS);
            __syncthreads();
#pragma unroll
            for (int tk = 0; tk < NTRK; ++tk) {
                const unsigned long long* xbase = p.xch + ((size_t)(xslot + tk) * 2 + (l & 1)) * MT * 4 * XW + wave * XW;       // + tile * 4 * XW
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int ft = 0; ft < FT; ++ft) {
                        const f32x4 kp = dt_xload(xbase + (size_t)i * 4 * XW + ft * 128, lane), vp = dt_xload(xbase + (size_t)i * 4 * XW + (FT + ft) * 128, lane);
                        kt[tk][i][ft] = tile == i ? kown[tk][ft] : kp; vt[tk][i][ft] = tile == i ? vown[tk][ft] : vp;
                    }
            }
        }
#pragma unroll
        for (int tk = 0; tk < NTRK; ++tk) {         // attention never crosses tracks
            constexpr int KB = SPLIT ? 0 : MT, VB = SPLIT ? 0 : 1;       // SPLIT: kf / vf hold the current track only
            if constexpr (SPLIT) {
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int c = 0; c < NCF; ++c) kf[i][c] = APR::template frag<FT>(kt[tk][i], c);
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) {
                    f32x4 tl[MT];
#pragma unroll
                    for (int i = 0; i < MT; ++i) tl[i] = vt[tk][i][ft];
#pragma unroll
                    for (int c = 0; c < NCK; ++c) vf[0][ft][c] = APR::template frag<MT>(tl, c);
                }
            }
            f32x4 S[DT_NQL /*query tile j (of this workgroup)*/][MT /*key tile i*/];
#pragma unroll
            for (int j = 0; j < DT_NQL; ++j)
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < NCF; ++c) APR::mma(s, kf[tk * KB + i][c], qf[tk * DT_NQL + j][c]);
                    S[j][i] = s;   // lane (a,b) r : S[query 16j + a][key 16i + 4b + r]
                }
            DT_STAMP(sl + 3);
#pragma unroll
            for (int j = 0; j < DT_NQL; ++j) {
                float m = -INFINITY;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (16 * i + 4 * b + r >= T) S[j][i][r] = -INFINITY;   // padded keys
                        m = fmaxf(m, S[j][i][r]);
                    }
                m = xor_max_b(m);
                float sum = 0.f;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float e = PR::exp(S[j][i][r] - m); S[j][i][r] = e; sum += e; }
                sum = xor_sum_b(sum);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int i = 0; i < MT; ++i) S[j][i] = S[j][i] * inv;
            }
            DT_STAMP(sl + 4);
            if (DT_NQL == MTL && p.att != nullptr) {      // (a pruned layer is never asked for its attention maps)
#pragma unroll
                for (int j = 0; j < DT_NQL; ++j)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int q = 16 * j + a + tok0, k = 16 * i + 4 * b + r;
                            if (q < T && k < T)
                                p.att[((((size_t)l * p.B + track_of(tk)) * 4 + wave) * T + q) * T + k] = S[j][i][r];
                        }
            }
#pragma unroll
            for (int j = 0; j < DT_NQL; ++j) {
                u32x4 pf[NCK];
#pragma unroll
                for (int c = 0; c < NCK; ++c) pf[c] = APR::template frag<MT>(S[j], c);
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) {
                    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < NCK; ++c) APR::mma(o, vf[tk * VB][ft][c], pf[c]);
                    // lane (a,b) r : O[query 16j + a][feature wave*HD + 16ft + 4b + r]
                    clipped |= PR::store4((TWO ? xop : hb) + (tk * 16 * DT_NQL + 16 * j + a) * LD::RSO + (wave * HD + 16 * ft + 4 * b) * EP, o, (LD::RSO - 16) / 2);
                }
            }
        }
        DT_STAMP(sl + 5);
        __syncthreads();
        DT_STAMP(sl + 6);
        // -- A3: out-proj (swapped) on top of the residual, then LayerNorm1 ------------------------------------------
        {
            f32x4 bo[NTW], g1[NTW], be1[NTW];
            load_vec4<NTW>(bo, W.b_out, fbase + 4 * b);
            load_vec4<NTW>(g1, W.g1, fbase + 4 * b);
            load_vec4<NTW>(be1, W.be1, fbase + 4 * b);
            const int hf0 = wave * (LD::FFC / 4);
            if constexpr (TWO) {
                static_assert(LD::RSO == LD::RSX, "O is staged in the Xop region");
#pragma unroll
                for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
                    for (int tt = 0; tt < DT_NQT; ++tt) DT_XQ[ft][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                gemm_stream<PREC, NTW, DT_NQT, KC_D, PF, true, FSUB, WMAX, XM>(DT_XQ, wf, w_out, KC_D * CW, xop + a * LD::RSO + b * 16, LD::RSO,
                                                                 W.w1 + (size_t)(hf0 / 16) * KC_D * CW + lane, KC_D * CW);
                DT_STAMP(sl + 7);
#pragma unroll
                for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
                    for (int tt = 0; tt < DT_NQT; ++tt)          // residual comes back from its parking place
                        DT_XQ[ft][tt] += bo[ft] + *(const f32x4*)(hb + (16 * tt + a) * RSP + (fbase + 16 * ft + 4 * b) * 4);
            } else {
#pragma unroll
            for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
                for (int tt = 0; tt < DT_NQT; ++tt) DT_XQ[ft][tt] = PR::prescale(DT_XQ[ft][tt]);       // (x3: the residual joins the scaled accumulation; a power of two, exact)
            gemm_stream<PREC, NTW, DT_NQT, KC_D, PF, true, FSUB, WMAX, XM>(DT_XQ, wf, w_out, KC_D * CW, hb + a * LD::RSO + b * 16, LD::RSO,
                                                             W.w1 + (size_t)(hf0 / 16) * KC_D * CW + lane, KC_D * CW);
            DT_STAMP(sl + 7);
#pragma unroll
            for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
                for (int tt = 0; tt < DT_NQT; ++tt) DT_XQ[ft][tt] = PR::unscale(DT_XQ[ft][tt]) + bo[ft];
            }
            layer_norm_regs<NTW, DT_NQT>(DT_XQ, g1, be1, red1, red2, wave, a, b, invD);
            // the two barriers inside the LayerNorm also order every wave's reads of Xop (QKV) and HB (O)
            // before the writes below / in the FFN.
            clipped |= store_rows<PREC, NTW, DT_NQT>(DT_XQ, xop, LD::RSX, a, b, fbase);
        }
        __syncthreads();
        DT_STAMP(sl + 8);
        // -- F: FFN in NCHUNK_FF chunks of the hidden dimension, FSUB hidden tiles at a time -------------------------
        f32x4 b2[NTW], g2[NTW], be2[NTW];
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
            for (int tt = 0; tt < DT_NQT; ++tt) DT_XQ[ft][tt] = PR::prescale(DT_XQ[ft][tt]);
#pragma unroll
        for (int ch = 0; ch < NCHUNK_FF; ++ch) {
            const u32x4* w2 = W.w2 + ((size_t)(wave * NTW) * KC_FF + ch * KC_FFC) * CW + lane;
#pragma unroll
            for (int sb = 0; sb < NSUB; ++sb) {
                f32x4 h[FSUB][DT_NQT];
                const int hloc = wave * (LD::FFC / 4) + sb * FSUB * 16;      // first hidden feature (within the chunk)
                const int hf0 = ch * LD::FFC + hloc;
                f32x4 b1[FSUB];
                load_vec4<FSUB>(b1, W.b1, hf0 + 4 * b);
#pragma unroll
                for (int ft = 0; ft < FSUB; ++ft)
#pragma unroll
                    for (int tt = 0; tt < DT_NQT; ++tt) h[ft][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                const u32x4* w1 = W.w1 + (size_t)(hf0 / 16) * KC_D * CW + lane;
                if (sb + 1 < NSUB)
                    gemm_stream<PREC, FSUB, DT_NQT, KC_D, PF, true, FSUB, WMAX, XM>(h, wf, w1, KC_D * CW, xop + a * LD::RSX + b * 16, LD::RSX,
                                                                      w1 + (size_t)FSUB * KC_D * CW, KC_D * CW);
                else
                    gemm_stream<PREC, FSUB, DT_NQT, KC_D, PF, true, NTW, WMAX, XM>(h, wf, w1, KC_D * CW, xop + a * LD::RSX + b * 16, LD::RSX, w2, KC_FF * CW);
                if (p.act == 0) {            // wave-uniform branch kept OUTSIDE the element loops (no erff for ReLU)
#pragma unroll
                    for (int ft = 0; ft < FSUB; ++ft)
#pragma unroll
                        for (int tt = 0; tt < DT_NQT; ++tt) {
                            f32x4 v = PR::unscale(h[ft][tt]) + b1[ft];
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                            clipped |= PR::store4(hb + (16 * tt + a) * LD::RSH + (hloc + 16 * ft + 4 * b) * EP, v, (LD::RSH - 16) / 2);
                        }
                } else {
#pragma unroll
                    for (int ft = 0; ft < FSUB; ++ft)
#pragma unroll
                        for (int tt = 0; tt < DT_NQT; ++tt) {
                            f32x4 v = PR::unscale(h[ft][tt]) + b1[ft];
                            v = PR::gelu(v);
                            clipped |= PR::store4(hb + (16 * tt + a) * LD::RSH + (hloc + 16 * ft + 4 * b) * EP, v, (LD::RSH - 16) / 2);
                        }
                }
            }
            __syncthreads();
            if (ch == NCHUNK_FF - 1) DT_STAMP(sl + 9);
            if (ch + 1 < NCHUNK_FF) {
                const int hfn = (ch + 1) * LD::FFC + wave * (LD::FFC / 4);
                gemm_stream<PREC, NTW, DT_NQT, KC_FFC, PF, true, FSUB, WMAX, XM>(DT_XQ, wf, w2, KC_FF * CW, hb + a * LD::RSH + b * 16, LD::RSH,
                                                                   W.w1 + (size_t)(hfn / 16) * KC_D * CW + lane, KC_D * CW);
                __syncthreads();           // HB is rewritten by the next chunk
            } else {
                // LayerNorm2's vectors are fetched here so that they are live only across the last FFN2 GEMM
                load_vec4<NTW>(b2, W.b2, fbase + 4 * b);
                load_vec4<NTW>(g2, W.g2, fbase + 4 * b);
                load_vec4<NTW>(be2, W.be2, fbase + 4 * b);
                gemm_stream<PREC, NTW, DT_NQT, KC_FFC, PF, true, QNW, WMAX, XM>(DT_XQ, wf, w2, KC_FF * CW, hb + a * LD::RSH + b * 16, LD::RSH,
                                                                 wq_of(Wn, DT_KNEXT ? 1 : 0), KC_D * CW);
            }
        }
        DT_STAMP(sl + 10);
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
            for (int tt = 0; tt < DT_NQT; ++tt) DT_XQ[ft][tt] = PR::unscale(DT_XQ[ft][tt]) + b2[ft];
        layer_norm_regs<NTW, DT_NQT>(DT_XQ, g2, be2, red1, red2, wave, a, b, invD);
        clipped |= store_rows<PREC, NTW, DT_NQT>(DT_XQ, xop, LD::RSX, a, b, fbase);
        if (TWO) park_x();                 // HB (the FFN hidden) is dead: the LayerNorm barriers are behind every wave's FFN2 reads
        __syncthreads();
        DT_STAMP(sl + 11);
