// Fused Decision-Transformer forward for gfx950 (MI355X).  One workgroup (4 waves) per lost track.
//
// Replaces, per track:  token embed (busca/network.py:203-204), token assembly (:103-165), bucket
// indices + encoding lookup (busca/encodings.py:43-94,150-272), 4 post-norm encoder layers
// (busca/custom_layers.py:30-41), decoder LayerNorm+Linear (network.py:93-94,231-232), softmax and
// argmax (network.py:403,415-421).
//
// Design (see DESIGN.md "K-DT"):
//  * the residual stream X[T,d] lives in REGISTERS for the whole kernel, in the MFMA accumulator layout
//    of a "swapped" product (weights are the A operand): lane (a = lane&15, b = lane>>4), tile (ft, tt),
//    reg r  <->  X[token 16*tt + a][feature wave_base + 16*ft + 4*b + r].  Each wave owns d/4 features.
//  * the C/D layout of a 16x16 MFMA tile (4 consecutive rows per lane) is exactly the A/B operand layout
//    of the next contraction (4 consecutive k per lane), so Q, K, V, the attention scores and the
//    probabilities never leave registers: wave h computes head h's Q^T, K^T (swapped) and V (normal)
//    and runs softmax(QK^T)V entirely in-register.  Only O, the LayerNorm output and the FFN hidden
//    go through LDS (they are re-read by all four waves as the K dimension of the next GEMM).
//  * weights are pre-packed on the host into MFMA operand-fragment order: one (16-row tile, 64-byte k
//    chunk) fragment is 64 lanes x 16 B = 1 KiB contiguous, fetched with one global_load_dwordx4 per
//    lane, software-prefetched PF chunks ahead; every weight byte is read once per workgroup.
//  * PREC 0: v_mfma_f32_16x16x4_f32 (exact f32, k permuted identically on both operands);
//    PREC 1: v_mfma_f32_16x16x32_f16 (f16 operands, f32 accumulate); LN/softmax/residual always f32.

// Every flavour of this kernel (one, two tracks per workgroup, one token tile per workgroup) must give a token the same bits: no implicit
// multiply-add contraction in this file (hipcc decides it per instantiation - packed or scalar, fused or not); where a fused multiply-add is wanted
// it is written as one (dt_fma).  Restored to the HIP default at the end of the file.
#pragma clang fp contract(off)

#include "dt_types.hpp"

static __device__ __forceinline__ float dt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
static __device__ __forceinline__ f32x4 dt_fma(f32x4 a, f32x4 b, f32x4 c) { return __builtin_elementwise_fma(a, b, c); }

#define DT_STAMP(slot) do { if (p.prof != nullptr && blockIdx.x == 0 && lane == 0) p.prof[wave * DT_PROF_SLOTS + (slot)] = (long long)__builtin_readcyclecounter(); } while (0)

template <int PREC> struct Prec;
// ES: bytes per element of an LDS operand row (x3: hi + lo planes), EP: bytes per element inside one plane, CHUNK: k per 64-byte chunk of a plane,
// CW: u32x4 per (weight tile, chunk) of the packed weight stream (x3: 64 hi fragments then 64 lo fragments), op_t: one GEMM operand fragment.
template <> struct Prec<0> {
    typedef float elem;
    typedef u32x4 op_t;
    static constexpr int ES = 4, EP = 4, CHUNK = 16, SUB = 4, CW = 64;   // bytes/elem, k per 64-byte chunk, k per lane
    static __device__ __forceinline__ op_t wload(const u32x4* __restrict__ w) { return *w; }
    static __device__ __forceinline__ op_t xload(const char* p, int) { return *(const u32x4*)p; }
    static __device__ __forceinline__ f32x4 unscale(f32x4 v) { return v; }
    static __device__ __forceinline__ f32x4 prescale(f32x4 v) { return v; }
    static __device__ __forceinline__ void mma(f32x4& acc, u32x4 a, u32x4 b) {
        f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[0], bf[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[1], bf[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[2], bf[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[3], bf[3], acc, 0, 0, 0);
    }
    // number of operand chunks that NT accumulator tiles (16 k each) form
    static constexpr int nchunks(int ntiles) { return ntiles; }
    template <int NT> static __device__ __forceinline__ u32x4 frag(const f32x4 (&t)[NT], int c) {
        return __builtin_bit_cast(u32x4, t[c]);
    }
    static __device__ __forceinline__ bool store4(char* p, f32x4 v, int = 0) { *(f32x4*)p = v; return false; }     // (returns: an operand was clipped - x3 only)
    static __device__ __forceinline__ float exp(float x) { return expf(x); }
    // exact GELU (torch.nn.functional.gelu, approximate='none'): libm erff
    static __device__ __forceinline__ f32x4 gelu(f32x4 v) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = 0.5f * v[r] * (1.0f + erff(v[r] * 0.70710678118654752440f));
        return v;
    }
};
template <> struct Prec<1> {
    typedef _Float16 elem;
    typedef u32x4 op_t;
    static constexpr int ES = 2, EP = 2, CHUNK = 32, SUB = 8, CW = 64;
    static __device__ __forceinline__ op_t wload(const u32x4* __restrict__ w) { return *w; }
    static __device__ __forceinline__ op_t xload(const char* p, int) { return *(const u32x4*)p; }
    static __device__ __forceinline__ f32x4 unscale(f32x4 v) { return v; }
    static __device__ __forceinline__ f32x4 prescale(f32x4 v) { return v; }
    static __device__ __forceinline__ void mma(f32x4& acc, u32x4 a, u32x4 b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), acc, 0, 0, 0);
    }
    static constexpr int nchunks(int ntiles) { return (ntiles + 1) / 2; }
    template <int NT> static __device__ __forceinline__ u32x4 frag(const f32x4 (&t)[NT], int c) {
        h16x8 h;
        f32x4 lo = t[2 * c];
        f32x4 hi = (2 * c + 1 < NT) ? t[(2 * c + 1 < NT) ? 2 * c + 1 : 0] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) { h[r] = (_Float16)lo[r]; h[4 + r] = (_Float16)hi[r]; }
        return __builtin_bit_cast(u32x4, h);
    }
    static __device__ __forceinline__ bool store4(char* p, f32x4 v, int = 0) {
        h16x4 h; h[0] = (_Float16)v[0]; h[1] = (_Float16)v[1]; h[2] = (_Float16)v[2]; h[3] = (_Float16)v[3];
        *(h16x4*)p = h;
        return false;
    }
    // exp2-based: ~2 ulp, far inside the f16-operand tolerance; -inf -> 0 as required by the key mask
    static __device__ __forceinline__ float exp(float x) { return __expf(x); }
    // GELU with erf(s) = sign(s) (1 - 2^(-|s| P5(|s|))), |s| clamped at 4 (erf(4) = 1 - 1.5e-8): ONE transcendental and no branch where erff is
    // two polynomial branches + an exp (~40 VALU instructions per element: at d = 256 / ff = 512 that was 5 VALU instructions per MFMA of the
    // whole forward, the largest non-matrix cost of the f16 kernels).  P5 is a minimax fit of -log2(erfc(s)) / s on [0, 4]: |erf error| <= 3.1e-7
    // evaluated in float32 (tools/fit_erf.py) - three orders below the fp16 rounding the hidden layer gets when it is stored as the next operand.
    static __device__ __forceinline__ f32x4 gelu(f32x4 v) {
        const f32x4 s = v * 0.70710678118654752440f;
        f32x4 ax = __builtin_elementwise_min(__builtin_elementwise_abs(s), (f32x4){4.f, 4.f, 4.f, 4.f});
        auto k4 = [](float c) { return (f32x4){c, c, c, c}; };
        f32x4 q = dt_fma(ax, k4(-0.00014198364806361496f), k4(0.0036634085699915886f));
        q = dt_fma(q, ax, k4(-0.030893569812178612f));
        q = dt_fma(q, ax, k4(0.1496966928243637f));
        q = dt_fma(q, ax, k4(0.9181665182113647f));
        q = dt_fma(q, ax, k4(1.627924919128418f));
        const f32x4 m = q * -ax;
        f32x4 e;
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = __builtin_amdgcn_exp2f(m[r]);
        f32x4 erf_ = 1.0f - e;
#pragma unroll
        for (int r = 0; r < 4; ++r) erf_[r] = __builtin_copysignf(erf_[r], s[r]);
        return (v * 0.5f) * (erf_ + 1.0f);
    }
};

// PREC 2 ("x3", round 5): float32-EQUIVALENT products on the fp16 matrix cores for the GEMMs (embed, Q / K / V, out-proj, FFN1, FFN2 = 96 % of the FLOPs):
// every f32 operand is the sum of two fp16 numbers hi = fp16(x), lo = fp16(x - hi) (22 mantissa bits); a product block is THREE v_mfma_f32_16x16x32_f16
// (lo hi, hi lo, hi hi; lo lo is below f32 rounding) into the f32 accumulator - 3 x 16 cycles per 32 k against 8 x 32 cycles of the f32 MFMA.  Weights are split
// on the host (pre-multiplied by DT_X3_WS so that lo stays a normal fp16 number), activations when they are stored as the next GEMM's operand (x DT_X3_XS,
// clamped at the fp16 range), two fp16 planes per LDS row; accumulators carry the factor DT_X3_WS * DT_X3_XS (a power of two: exact) and are unscaled
// where the f32 kernel reads them.  Attention (scores, probabilities x V), LayerNorm, softmax, GELU and the residual stream are the f32 kernel's, bit for bit
// the same code: Q, K, V never leave their f32 registers.
struct X3Op { u32x4 hi, lo; };
typedef _Float16 dt_h16x2 __attribute__((ext_vector_type(2)));
typedef float dt_f32x2 __attribute__((ext_vector_type(2)));
// two f32 -> packed (hi, hi) and (lo, lo) fp16 pairs, lo = fp16(t - hi): t - hi is exact in f32, so ONE mixed-precision fma per element does the fp16 -> f32
// conversion, the subtraction and the rounding (hipcc emits 2 v_cvt_f32_f16 + v_pk_add_f32 + v_cvt_pk_f16_f32 for the plain expression; same bits - the idiom
// of the ReID kernels, reid_x3.hip.inc x3_split2)
static __device__ __forceinline__ void dt_split2(float t0, float t1, unsigned& hi, unsigned& lo) {
    const dt_h16x2 h = __builtin_convertvector((dt_f32x2){t0, t1}, dt_h16x2);
    hi = __builtin_bit_cast(unsigned, h);
    unsigned l;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(hi), "v"(t0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(hi), "v"(t1));
    lo = l;
}
template <> struct Prec<2> {
    typedef _Float16 elem;
    typedef X3Op op_t;
    static constexpr int ES = 4, EP = 2, CHUNK = 32, SUB = 8, CW = 128;
    static __device__ __forceinline__ op_t wload(const u32x4* __restrict__ w) { op_t o; o.hi = w[0]; o.lo = w[64]; return o; }
    static __device__ __forceinline__ op_t xload(const char* p, int po) { op_t o; o.hi = *(const u32x4*)p; o.lo = *(const u32x4*)(p + po); return o; }
    static __device__ __forceinline__ void mma(f32x4& acc, op_t a, op_t b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a.lo), __builtin_bit_cast(h16x8, b.hi), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a.hi), __builtin_bit_cast(h16x8, b.lo), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a.hi), __builtin_bit_cast(h16x8, b.hi), acc, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 unscale(f32x4 v) { return v * (1.0f / (DT_X3_XS * DT_X3_WS)); }
    static __device__ __forceinline__ f32x4 prescale(f32x4 v) { return v * (DT_X3_XS * DT_X3_WS); }
    // po: byte offset of the lo plane in the row.  Returns true when an operand had to be clipped (|x| > 65504 / DT_X3_XS = 1023.5): the kernel reports it
    // (DTParams::xerr) instead of clipping silently - this flavour promises float32-equivalent results.
    static __device__ __forceinline__ bool store4(char* p, f32x4 v, int po) {
        const f32x4 lim = {65504.f, 65504.f, 65504.f, 65504.f};
        const f32x4 sv = v * DT_X3_XS, av = __builtin_elementwise_abs(sv);
        const bool clipped = fmaxf(fmaxf(av[0], av[1]), fmaxf(av[2], av[3])) > 65504.f;
        const f32x4 s = __builtin_elementwise_min(__builtin_elementwise_max(sv, -lim), lim);
        unsigned h0, h1, l0, l1;
        dt_split2(s[0], s[1], h0, l0);
        dt_split2(s[2], s[3], h1, l1);
        *(u32x2*)p = (u32x2){h0, h1};
        *(u32x2*)(p + po) = (u32x2){l0, l1};
        return clipped;
    }
    // softmax exponential: exp2-based (v_exp_f32 on x log2 e: ~1e-6 relative for the arguments a softmax sees, -88 .. 0) - a tenth of this flavour's own
    // 1e-5 distance from the exact kernel, a quarter of libm expf's instructions
    static __device__ __forceinline__ float exp(float x) { return __expf(x); }
    static __device__ __forceinline__ f32x4 gelu(f32x4 v) { return Prec<0>::gelu(v); }
};
// the precision the attention runs in (operands straight from the f32 accumulators for f32 and x3)
template <int PREC> struct AttPrec { typedef Prec<PREC == 2 ? 0 : PREC> type; };

// Weight streaming.  The whole kernel is one long stream of weight fragments (embed, then per layer
// Q, K, V, out-proj, FFN1, FFN2).  `wf[PF][WMAX]` always holds the next PF chunks of the stream: while a GEMM
// consumes its last PF chunks it already fetches the first PF chunks of the NEXT GEMM, so the load latency of a
// phase start hides under the previous phase's epilogue (bias / softmax / LayerNorm / LDS stores / barriers).

template <int PREC, int NW, int PF, int WMAX>
__device__ __forceinline__ void gemm_prefetch(typename Prec<PREC>::op_t (&wf)[PF][WMAX], const u32x4* __restrict__ w, int tstride) {
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int i = 0; i < NW; ++i) wf[p][i] = Prec<PREC>::wload(w + i * tstride + p * Prec<PREC>::CW);
}

// acc[NW][NX] (+)= W-tiles x X-tiles over NKC 64-byte k chunks.
//  wf  : on entry chunks 0..PF-1 of this GEMM's NW weight tiles; on exit chunks 0..PF-1 of the next GEMM's NWN tiles.
//  w   : fragment (tile 0, chunk 0) of this wave's weight tiles, already offset by lane; consecutive tiles are
//        `tstride` u32x4 apart, consecutive chunks 64 apart.  wn/tstride_n: the same for the next GEMM.
//  lds : activation rows, already offset by (lane&15)*RS + (lane>>4)*16 (+ first_chunk*64).
//  W_IS_A: weights are the MFMA A operand (swapped product -> lane holds 4 consecutive FEATURES of one
//        token); else activations are A (normal product -> 4 consecutive TOKENS of one feature).
// XM: how the activation fragments come out of the LDS.
//  0  each chunk's NX fragments are read right in front of its MFMAs (hipcc clusters two chunks' reads and waits for them there);
//  1  one chunk AHEAD into a second register set, so the ds_read latency of chunk k+1 sits under the NW*NX MFMAs of chunk k; a
//     sched_barrier pins the reads (hipcc otherwise sinks them back in front of their own MFMAs).  Costs 4*NX registers: only the
//     one-track f16 d = 256 flavour has them (same box: 0.102 -> 0.094 ms for 256 tracks; two tracks per workgroup, d = 512 and f32
//     spill or lose 3-9 %).  A register-free rolling variant (tile-major MFMA order, a tile's next fragment read into the same
//     registers right after its MFMAs) lost 3-10 % everywhere: the per-tile scheduling fences cost more than the reads they hide.
// XT: activation tile j starts at byte offset xt[j] from `lds` (per lane: the row each lane reads is looked up, dt_unique_kernel.hip.inc) instead of j * 16 * RS.
template <int PREC, int NW, int NX, int NKC, int PF, bool W_IS_A, int NWN, int WMAX, int XM = 0, bool XT = false>
__device__ __forceinline__ void gemm_stream(f32x4 (&acc)[NW][NX], typename Prec<PREC>::op_t (&wf)[PF][WMAX], const u32x4* __restrict__ w, int tstride,
                                            const char* lds, int RS, const u32x4* __restrict__ wn, int tstride_n, const int* xt = nullptr) {
    static_assert(NKC % PF == 0 && NW <= WMAX && NWN <= WMAX && (XM != 1 || PF % 2 == 0), "bad streaming geometry");
    typedef Prec<PREC> PR;
    constexpr int CW = PR::CW;
    const int po = (RS - 16) / 2;          // x3: the lo plane of a row starts half way (every row stride is K * ES + 16)
    typename PR::op_t xf[XM == 1 ? 2 : 1][NX];
    auto xrow = [&](int j) { if constexpr (XT) return xt[j]; else return j * 16 * RS; };
    if constexpr (XM == 1) {
#pragma unroll
        for (int j = 0; j < NX; ++j) xf[0][j] = PR::xload(lds + xrow(j), po);
    }
#pragma unroll 1
    for (int k0 = 0; k0 < NKC; k0 += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int kx = k0 + p + 1 < NKC ? k0 + p + 1 : NKC - 1;      // (the last chunk re-reads itself: no branch, no stray address)
            if constexpr (XM == 1) {
#pragma unroll
                for (int j = 0; j < NX; ++j) xf[(p + 1) & 1][j] = PR::xload(lds + xrow(j) + kx * 64, po);
                __builtin_amdgcn_sched_barrier(0);
            } else {
#pragma unroll
                for (int j = 0; j < NX; ++j) xf[0][j] = PR::xload(lds + xrow(j) + (k0 + p) * 64, po);
            }
            constexpr int XS = XM == 1 ? 1 : 0;
#pragma unroll
            for (int i = 0; i < NW; ++i)
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    if (W_IS_A) Prec<PREC>::mma(acc[i][j], wf[p][i], xf[p & XS][j]);
                    else        Prec<PREC>::mma(acc[i][j], xf[p & XS][j], wf[p][i]);
                }
            const int kn = k0 + p + PF;
            if (kn < NKC) {
#pragma unroll
                for (int i = 0; i < NW; ++i) wf[p][i] = PR::wload(w + i * tstride + kn * CW);
            } else if (NWN > 0) {
#pragma unroll
                for (int i = 0; i < NWN; ++i) wf[p][i] = PR::wload(wn + i * tstride_n + (kn - NKC) * CW);
            }
        }
    }
}

static __device__ __forceinline__ float xor_sum_b(float v) {   // sum over the 4 lane groups b = lane>>4
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
static __device__ __forceinline__ float xor_max_b(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

// ---- bucket indices (busca/encodings.py:150-272) -----------------------------------------------------
// R = float reproduces torch float32 tensor math, R = double the float64 promotion of the candidate side.
template <typename R> static __device__ __forceinline__ R log_r(R x);
template <> __device__ __forceinline__ float log_r<float>(float x) { return (float)log((double)x); }  // correctly rounded f32
template <> __device__ __forceinline__ double log_r<double>(double x) { return log(x); }

template <typename R>
static __device__ __forceinline__ void bucket_xy_size(R x1, R y1, R x2, R y2, float rx1, float ry1, float rx2,
                                                      float ry2, int& ixy, int& isz) {
#pragma clang fp contract(off)   // torch evaluates every op separately; an fma here could flip a bucket
    // reference box terms are float32 tensors in the reference (encodings.py:240-244)
    const float w_ref = rx2 - rx1 + 1.f, h_ref = ry2 - ry1 + 1.f;
    const float cx_ref = 0.5f * (rx1 + rx2), cy_ref = 0.5f * (ry1 + ry2);
    const R w = x2 - x1 + (R)1, h = y2 - y1 + (R)1;
    const R cx = (R)0.5 * (x1 + x2), cy = (R)0.5 * (y1 + y2);
    R dx = (cx - (R)cx_ref) / w; dx = dx * dx;
    R dy = (cy - (R)cy_ref) / h; dy = dy * dy;
    const R eps = (R)1e-3;                       // python scalar 1e-3 converted to the tensor dtype
    R xy = log_r<R>(sqrt(dx + dy) + eps);
    R sz = log_r<R>(w / (R)w_ref + eps) + log_r<R>(h / (R)h_ref + eps);
    xy = xy * (R)15; sz = sz * (R)15;
    xy = fmin(fmax(xy, (R)-105), (R)105);
    sz = fmin(fmax(sz, (R)-105), (R)105);
    ixy = (int)xy + 105;                          // .to(torch.long) truncates toward zero
    isz = (int)sz + 105;
}

// token t of track `trk` -> (xy, size, time) bucket.  Token order [MEM*L, pair*P, pair(NON), pair(BAD)?] with pair = (SEP, CAN) for the
// MEM-SEP-CAN flavours (can_pos 1) or (CAN, SEP) for MEM-CAN-SEP (can_pos 0); nspec = 2 with the BAD token, 1 without (network.py:
// 103-165).  Boxes (encodings.py:112-146): a candidate pair is encoded with (reference box, candidate box) - or twice the candidate
// box when sep_can (encode_separator_as_reference = false) -, the NON pair with the reference box, the BAD pair with the distant fake box.
static __device__ __forceinline__ void token_bucket(const float* mem_ltrb, const float* can_ltrb, int trk, int t,
                                                    int L, int P, int fake_f64, int can_pos, int nspec, int sep_can,
                                                    int& ixy, int& isz, int& it) {
    const float* ref = mem_ltrb + ((size_t)trk * L + (L - 1)) * 4;
    const float rx1 = ref[0], ry1 = ref[1], rx2 = ref[2], ry2 = ref[3];
    if (t < L) {
        const float* bx = mem_ltrb + ((size_t)trk * L + t) * 4;
        int v = (t - L + 1) * 2; v = v < -30 ? -30 : (v > 30 ? 30 : v);
        it = v + 30;
        bucket_xy_size<float>(bx[0], bx[1], bx[2], bx[3], rx1, ry1, rx2, ry2, ixy, isz);
        return;
    }
    const int k = t - L, j = k >> 1, odd = k & 1;
    it = odd ? 34 : 32;                           // [1,2]*2 + 30: by position in the pair, whatever the flavour (encodings.py:150-172)
    float x1 = rx1, y1 = ry1, x2 = rx2, y2 = ry2; // SEP / NON tokens are encoded with the reference box
    bool fake = false;
    if (nspec == 2 && j == P + 1) fake = true;    // BAD pair: distant fake bbox, ltwh values used as ltrb
    else if (j < P && (odd == can_pos || sep_can)) { const float* bx = can_ltrb + ((size_t)trk * P + j) * 4; x1 = bx[0]; y1 = bx[1]; x2 = bx[2]; y2 = bx[3]; }
    if (fake_f64) {
        double X1 = x1, Y1 = y1, X2 = x2, Y2 = y2;
        if (fake) { const double m = -3.4028234663852886e38; X1 = m; Y1 = m; X2 = -m / 100.0; Y2 = -m / 100.0; }
        bucket_xy_size<double>(X1, Y1, X2, Y2, rx1, ry1, rx2, ry2, ixy, isz);
    } else {
        if (fake) { const float m = -3.4028234663852886e38f; x1 = m; y1 = m; x2 = -m / 100.0f; y2 = -m / 100.0f; }
        bucket_xy_size<float>(x1, y1, x2, y2, rx1, ry1, rx2, ry2, ixy, isz);
    }
}

#ifdef BUSCA_DT_BUCKET_KERNEL      // a non-template kernel: defined in ONE translation unit (busca_hip.hip), launched through dt_bucket_ids_launch
__global__ void dt_bucket_ids_kernel(const float* mem_ltrb, const float* can_ltrb, int B, int L, int P, int fake_f64, int can_pos, int nspec,
                                     int sep_can, int* ids) {
    const int T = L + 2 * (P + nspec);
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * T) return;
    int ixy, isz, it;
    token_bucket(mem_ltrb, can_ltrb, gid / T, gid % T, L, P, fake_f64, can_pos, nspec, sep_can, ixy, isz, it);
    ids[gid * 3 + 0] = ixy; ids[gid * 3 + 1] = isz; ids[gid * 3 + 2] = it;
}
#endif

// ---- LDS plan ---------------------------------------------------------------------------------------------
template <int PREC, int MT, int D, int FF, int E, int NCHUNK_FF, int NTRK = 1>
struct DTLds {
    static constexpr int ES = Prec<PREC>::ES;
    static constexpr int TP = 16 * MT * NTRK;          // token rows of the workgroup: NTRK tracks stacked, 16*MT rows each
    static constexpr int FFC = FF / NCHUNK_FF;
    static constexpr int RSX = D * ES + 16;            // Xop row stride
    static constexpr int RSO = D * ES + 16;            // attention output rows (aliases HB)
    static constexpr int RSH = FFC * ES + 16;          // FFN hidden rows (aliases HB)
    static constexpr int RSE = E * ES + 16;            // staged ReID features (aliases HB)
    static constexpr int cmax(int a, int b) { return a > b ? a : b; }
    static constexpr int HB_BYTES = TP * cmax(cmax(RSO, RSH), RSE);
    static constexpr int OFF_XOP = 0;
    static constexpr int OFF_HB = OFF_XOP + TP * RSX;
    static constexpr int OFF_RED1 = OFF_HB + HB_BYTES;
    static constexpr int OFF_RED2 = OFF_RED1 + 4 * TP * 4;
    static constexpr int OFF_IDS = OFF_RED2 + 4 * TP * 4;
    static constexpr int OFF_MISC = OFF_IDS + 3 * TP * 4;
    static constexpr int TOTAL = OFF_MISC + 64 * 4;
};

template <int NTW, int MT>
static __device__ __forceinline__ void layer_norm_regs(f32x4 (&x)[NTW][MT], const f32x4 (&gamma)[NTW],
                                                       const f32x4 (&beta)[NTW], float* red1, float* red2,
                                                       int wave, int a, int b, float invD) {
    constexpr int TP = 16 * MT;
    float mean[MT], rstd[MT];
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
        float s = 0.f;
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft) s += (x[ft][tt][0] + x[ft][tt][1]) + (x[ft][tt][2] + x[ft][tt][3]);
        s = xor_sum_b(s);
        if (b == 0) red1[wave * TP + 16 * tt + a] = s;
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
        const int tok = 16 * tt + a;
        mean[tt] = ((red1[tok] + red1[TP + tok]) + (red1[2 * TP + tok] + red1[3 * TP + tok])) * invD;
        float q = 0.f;
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float c = x[ft][tt][r] - mean[tt]; q = dt_fma(c, c, q); }
        q = xor_sum_b(q);
        if (b == 0) red2[wave * TP + tok] = q;
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
        const int tok = 16 * tt + a;
        const float var = ((red2[tok] + red2[TP + tok]) + (red2[2 * TP + tok] + red2[3 * TP + tok])) * invD;
        rstd[tt] = 1.0f / sqrtf(var + 1e-5f);
    }
#pragma unroll
    for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
        for (int tt = 0; tt < MT; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) x[ft][tt][r] = dt_fma((x[ft][tt][r] - mean[tt]) * rstd[tt], gamma[ft][r], beta[ft][r]);
}

// this lane's 4 consecutive entries of a per-feature vector, for each of its NT feature tiles
template <int NT>
static __device__ __forceinline__ void load_vec4(f32x4 (&dst)[NT], const float* __restrict__ v, int f0) {
#pragma unroll
    for (int ft = 0; ft < NT; ++ft) dst[ft] = *(const f32x4*)(v + f0 + 16 * ft);
}

template <int PREC, int NTW, int MT>
static __device__ __forceinline__ bool store_rows(const f32x4 (&x)[NTW][MT], char* base, int RS, int a, int b, int fbase) {
    constexpr int EP = Prec<PREC>::EP;
    bool clipped = false;
#pragma unroll
    for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
        for (int tt = 0; tt < MT; ++tt)
            clipped |= Prec<PREC>::store4(base + (16 * tt + a) * RS + (fbase + 16 * ft + 4 * b) * EP, x[ft][tt], (RS - 16) / 2);
    return clipped;
}


// =========================================================================================================
// NTRK tracks per workgroup (1 or 2): the tracks are stacked as extra token tiles, so every weight fragment a wave streams
// feeds NTRK*MT token tiles (f16: the kernel is bound by the weight stream, 2 tracks halve the bytes per FLOP); attention,
// padding masks and the decoder epilogue stay per track.
// (A two-workgroups-per-CU register diet of the single-track flavour was measured in round 2 - co-residency overlapped 1.34x, the
// diet cost 1.28x per workgroup - and removed.)
//
// SPLIT (round 5): the workgroup holds ONE of the MT 16-token tiles of its track, its MT - 1 partner workgroups the others.  Everything but the
// attention is local to a token; per layer each wave publishes the K^T and V tiles of its head for its 16 tokens (8 KiB at d = 256) with agent-scope
// stores, raises its flag, runs the Q projection, and then takes the partner waves' tiles - so a track runs on MT CUs (or shares them: these small
// workgroups fit two to a CU).  Every token sees the same products in the same order as in the one-workgroup flavour: bit-identical.  Used for the tail of a launch that would leave most CUs idle (640
// tracks on 256 CUs = 2.5 rounds took three; a single 32-track step kept 32 CUs busy).
// A/B only (BUSCA_SPLIT_RELAXED=1 python -m busca_amd.build): the hand-off without its fences, i.e. on the hardware's own ordering of 8-byte agent-scope atomics
#ifdef BUSCA_SPLIT_RELAXED
#define DT_XFENCE_RELEASE() do { } while (0)
#define DT_XFENCE_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup")
#else
#define DT_XFENCE_RELEASE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent")
#define DT_XFENCE_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#endif
static __device__ __forceinline__ void dt_xstore(unsigned long long* dst, int lane, f32x4 v) {
    const u32x4 u = __builtin_bit_cast(u32x4, v);
    __hip_atomic_store(dst + lane, (unsigned long long)u[0] | ((unsigned long long)u[1] << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(dst + 64 + lane, (unsigned long long)u[2] | ((unsigned long long)u[3] << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
static __device__ __forceinline__ f32x4 dt_xload(const unsigned long long* src, int lane) {
    const unsigned long long lo = __hip_atomic_load(src + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load(src + 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u32x4 u; u[0] = (unsigned)lo; u[1] = (unsigned)(lo >> 32); u[2] = (unsigned)hi; u[3] = (unsigned)(hi >> 32);
    return __builtin_bit_cast(f32x4, u);
}
// wait until the N flags flag[0], flag[stride], ... have all reached `value`: the N loads of a poll are in flight together (one round trip to the
// coherence point per poll, not N).  Bounded: a partner that never comes - which in-order dispatch rules out - must not hang the GPU.
template <int N, int M = 1>
static __device__ __forceinline__ void dt_xwait(const unsigned* flag, int stride, unsigned value, int* err, int stride2 = 0) {
    int spins = 0;
    for (;;) {
        unsigned v[M][N];
#pragma unroll
        for (int k = 0; k < M; ++k)
#pragma unroll
            for (int i = 0; i < N; ++i) v[k][i] = __hip_atomic_load(flag + k * stride2 + i * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < M; ++k)
#pragma unroll
            for (int i = 0; i < N; ++i) ok = ok && (int)(v[k][i] - value) >= 0;
        if (ok) break;
        __builtin_amdgcn_s_sleep(2);
        if (++spins > (1 << 22)) { *err = 1; break; }
    }
    // the partner is another workgroup, usually on another XCD: AGENT-scope acquire (buffer_inv sc1) pairs with the producer's agent-scope release before its
    // flag store.  (The payload accesses are 8-byte agent-scope atomics on both sides, which gfx950 serves coherently on their own; the fences make the
    // hand-off correct by the memory model, not only by the hardware's store-ack ordering.)
    DT_XFENCE_ACQUIRE();
}

template <int PREC, int MT, int D, int FF, int E, int NCHUNK_FF, int NTRK = 1, bool SPLIT = false>
__global__ void __launch_bounds__(256, (SPLIT && PREC == 0 && D <= 256 && NTRK == 1) ? 2 : 1) dt_fused_kernel(const DTParams p) {
    typedef Prec<PREC> PR;
    typedef typename AttPrec<PREC>::type APR;       // attention operands
    static_assert(!SPLIT || (MT >= 2 && NTRK <= 2), "token split: one 16-token tile of one or two tracks per workgroup");
    constexpr int MTL = SPLIT ? 1 : MT;             // token tiles of a track that this workgroup holds
    typedef DTLds<PREC, MTL, D, FF, E, NCHUNK_FF, NTRK> LD;
    constexpr int EP = PR::EP, CHUNK = PR::CHUNK, CW = PR::CW;
    constexpr int TP1 = 16 * MTL;           // token rows of one track in this workgroup
    constexpr int MTT = MTL * NTRK;         // token tiles of the workgroup
    constexpr int TP = 16 * MTT;
    constexpr int HD = D / 4;               // head dim (nhead == 4)
    constexpr int NTW = D / 64;             // feature tiles per wave for d-wide outputs (== tiles per head)
    constexpr int FT = HD / 16;
    constexpr int KC_D = D / CHUNK, KC_E = E / CHUNK, KC_FFC = LD::FFC / CHUNK, KC_FF = FF / CHUNK;
    constexpr int FTW = LD::FFC / 64;       // hidden feature tiles per wave per FF chunk
    constexpr int WMAX = NTW > 4 ? 8 : 4;   // weight tiles a GEMM call streams at once
    constexpr bool TWO = NTRK > 1 && !SPLIT;        // the residual stream is parked in LDS (HB) while Q/K/V and the attention run
    constexpr bool DIET = TWO;              // register diet: Q/K/V and FFN1 in half-width passes
    constexpr int QNW = DIET ? FT / 2 : FT; // weight tiles per Q/K/V pass
    constexpr int FSUB = DIET ? (FTW > 2 ? 2 : FTW) : (FTW > WMAX ? WMAX : FTW);         // FFN1 hidden tiles processed per call
    constexpr int RSP = D * 4 + 16;         // row stride of the parked f32 residual (TWO)
    static_assert(!TWO || (FT % 2 == 0 && RSP * 1 <= LD::HB_BYTES / TP), "multi-track flavour: residual does not fit HB");
    constexpr int NSUB = FTW / FSUB;
    constexpr int XM = (PREC != 0 && NTRK == 1 && D == 256 && MT <= 3) ? 1 : 0;       // (x3 too: 640 tracks 0.604 -> 0.593 ms)   // LDS operand reads one chunk ahead where the registers allow (gemm_stream)
    // prefetch depth of the weight stream in 64-byte chunks: f16 MFMAs retire a chunk in ~200 cycles, so the
    // window must be deeper than for f32 (~1500 cycles per chunk) to cover the L2 latency under load
    // (x3: a window of two chunks - with four the three-tile kernel spills 29 registers, needs scratch and is 6 % slower: 2 048 tracks 1.68 -> 1.57 ms)
    constexpr int PF = PREC == 2 ? 2 : (NTRK > 1) ? (KC_D >= 4 ? 4 : KC_D)
                                : ((PREC == 1 && WMAX == 4 && KC_D >= 8) ? 8 : ((PREC != 1 && WMAX == 8) ? 2 : (KC_D >= 4 ? 4 : KC_D)));
    constexpr int NCF = APR::nchunks(FT);   // operand chunks over a head's features
    constexpr int NCK = APR::nchunks(MT);   // operand chunks over the keys
    static_assert(FT == NTW && FTW % FSUB == 0 && KC_E % PF == 0 && KC_FFC % PF == 0, "geometry");
    // Pruned last layer (DTParams::prune; one track per workgroup, unsplit, f32 / x3): the decoder reads only the P + nspec candidate rows, so the last layer
    // projects K and V for every token but runs Q, the attention queries, out-proj, LayerNorm1, the FFN and LayerNorm2 on those rows alone, compacted into
    // NQP = MT - 1 tiles (the host sets the flag only where they fit).
    constexpr bool PRUNABLE = NTRK == 1 && !SPLIT && MT >= 2 && PREC != 1;
    constexpr int NQP = PRUNABLE ? MT - 1 : 1;
    static_assert(!PRUNABLE || 16 * NQP * RSP <= LD::HB_BYTES, "pruned layer: the compact residual does not fit HB");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* xop = smem + LD::OFF_XOP;
    char* hb = smem + LD::OFF_HB;
    float* red1 = (float*)(smem + LD::OFF_RED1);
    float* red2 = (float*)(smem + LD::OFF_RED2);
    int* ids = (int*)(smem + LD::OFF_IDS);

    // workgroup index: tracks trk*NTRK .. trk*NTRK + NTRK-1.  SPLIT: workgroups MT k .. MT k + MT - 1 hold the token tiles of track nsingle + k (partners sit
    // next to each other in dispatch order, so a workgroup only ever waits for workgroups that are resident or next in line)
    // (SPLIT with NTRK == 2: the SAME tile of two tracks, so that every streamed weight fragment feeds two token tiles - a one-tile workgroup is bound
    // by its weight stream through the CU's vector memory path)
    const int tile = SPLIT ? (int)(blockIdx.x % MT) : 0, xslot = SPLIT ? (int)(blockIdx.x / MT) * NTRK : 0;       // tile: which token tile of its track(s) a SPLIT workgroup holds; xslot: exchange slot of the first track
    const int tbase = SPLIT ? p.nsingle + xslot : (int)blockIdx.x * NTRK;      // first track of the workgroup
    const int tok0 = SPLIT ? tile * TP1 : 0;        // first token of the track held here
    auto track_of = [&](int k) { const int t = tbase + k; return t < p.B ? t : p.B - 1; };   // (an odd tail recomputes the last track)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int a = lane & 15, b = lane >> 4;
    const int L = p.L, P = p.P, T = p.T;
    const int fbase = wave * (D / 4);       // first feature this wave owns in d-wide tensors
    const bool prune = PRUNABLE && p.prune != 0;        // (a constant false in the flavours that cannot prune: their code is what it was without it)

    // this wave's slice of every weight matrix (fragment (tile 0, chunk 0) + lane)
    const u32x4* w_emb = p.w_embed + (size_t)(wave * NTW) * KC_E * CW + lane;
    auto wq_of = [&](const DTLayerW& W, int part) { return W.w_in + (size_t)((part * D + wave * HD) / 16) * KC_D * CW + lane; };

    typename PR::op_t wf[PF][WMAX];      // the weight stream window
    bool clipped = false;                // x3: an operand exceeded the split-fp16 range somewhere in this workgroup
    DT_STAMP(0);
    gemm_prefetch<PREC, NTW, PF, WMAX>(wf, w_emb, KC_E * CW);

    // ---- P0: bucket ids + stage the ReID features in token order -------------------------------------------
    if (tid < TP) {
        int ixy = 0, isz = 0, it = 0;
        const int tk = tid / TP1, tt_ = tid % TP1;
        if (tt_ + tok0 < T) token_bucket(p.mem_ltrb, p.can_ltrb, track_of(tk), tt_ + tok0, L, P, p.fake_f64, p.can_pos, p.nspec, p.sep_can, ixy, isz, it);
        ids[tid] = ixy; ids[TP + tid] = isz; ids[2 * TP + tid] = it;
    }
    {
        // TP*(E/4)/256 float4 pieces per thread; all loads are issued before the first LDS store so their
        // latencies overlap (they were serialised by the convert+store of the previous piece before)
        constexpr int NPC = TP * (E / 4) / 256;
        constexpr int NB = NPC > 24 ? NPC / 2 : NPC;    // pieces per batch (a batch's loads are all in flight together)
        static_assert(NPC % NB == 0, "staging batches");
#pragma unroll
        for (int q0 = 0; q0 < NPC; q0 += NB) {
            f32x4 v[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int i = tid + 256 * (q0 + q);
                const int row = i / (E / 4), e4 = i % (E / 4);
                const int t = row % TP1 + tok0;
                const size_t gtrk = (size_t)track_of(row / TP1);
                // every piece is loaded UNCONDITIONALLY (rows that hold no feature - SEP / NON / BAD / padding - read a valid dummy row and are multiplied
                // by zero): a conditional load sits in its own block and hipcc then waits for each one before it issues the next (24 serialised
                // round trips, 15 k cycles of the x3 prologue)
                const int k = t - L, j = k >> 1;
                const bool is_mem = t < L, is_can = !is_mem && t < T && (k & 1) == p.can_pos && j < P;
                const float* src = is_can ? p.can_feat + (gtrk * P + j) * E + e4 * 4 : p.mem_feat + (gtrk * L + (is_mem ? t : 0)) * E + e4 * 4;
                const f32x4 ld = *(const f32x4*)src;
                v[q] = ld * ((is_mem || is_can) ? 1.0f : 0.0f);          // (a multiply, not a select: hipcc sinks the load under a select's branch again)
            }
            __builtin_amdgcn_sched_barrier(0);      // (hipcc otherwise pairs every load with its own convert + store)
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int i = tid + 256 * (q0 + q);
                clipped |= PR::store4(hb + (i / (E / 4)) * LD::RSE + (i % (E / 4)) * 4 * EP, v[q], (LD::RSE - 16) / 2);
            }
        }
    }
    __syncthreads();
    DT_STAMP(1);

    // ---- P1: token embed (swapped product) + assembly + encoding -> X in registers ----------------------------
    f32x4 X[NTW][MTT];
    {
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
            for (int tt = 0; tt < MTT; ++tt) X[ft][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        gemm_stream<PREC, NTW, MTT, KC_E, PF, true, QNW, WMAX, XM>(X, wf, w_emb, KC_E * CW, hb + a * LD::RSE + b * 16, LD::RSE,
                                                       wq_of(p.layer[0], (SPLIT || (prune && p.nlayers == 1)) ? 1 : 0), KC_D * CW);
        DT_STAMP(2);
        const float sq = sqrtf((float)D);
        const int c = p.lut_c;
        // branch-free: every lane issues all its LUT / token-vector loads up front (padding tokens read row 0)
#pragma unroll
        for (int tt = 0; tt < MTT; ++tt) {
            const int row = 16 * tt + a;
            const int t = 16 * (tt % MTL) + a + tok0;       // token index within its track
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
    clipped |= store_rows<PREC, NTW, MTT>(X, xop, LD::RSX, a, b, fbase);
    __syncthreads();                       // Xop visible; every wave is done with the staged features in HB
    DT_STAMP(3);
    // TWO: each lane parks / fetches its own residual values (same addresses both ways: no barrier of its own)
    auto park_x = [&]() {
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
            for (int tt = 0; tt < MTT; ++tt) *(f32x4*)(hb + (16 * tt + a) * RSP + (fbase + 16 * ft + 4 * b) * 4) = X[ft][tt];
    };
    if (TWO) park_x();

    const float invD = 1.0f / (float)D;
    const float qscale = 1.0f / sqrtf((float)HD);

    // ---- encoder layers -------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int l = 0; l < p.nlayers - (prune ? 1 : 0); ++l) {        // (pruned: the last layer follows the loop)
        const DTLayerW& W = p.layer[l];
        const DTLayerW& Wn = p.layer[l + 1 < p.nlayers ? l + 1 : l];   // next layer (or a harmless re-read on the last)
        const u32x4* w_out = W.w_out + (size_t)(wave * NTW) * KC_D * CW + lane;
        const int sl = 4 + 12 * l;          // profile slot base of this layer
        // -- A1: head `wave`: Q^T, K^T (swapped) and V (normal) from Xop --------------------------------------
        u32x4 qf[MTT][NCF], kf[SPLIT ? MT : MTT][NCF], vf[SPLIT ? 1 : NTRK][FT][NCK];
        f32x4 kown[SPLIT ? MTT : 1][FT], vown[SPLIT ? MTT : 1][FT];     // SPLIT: this workgroup's K^T / V tiles (per track), kept for the attention
        constexpr size_t XW = (size_t)2 * FT * 128;                      // u64 per (parity, tile, wave) of the exchange: 2 FT tiles of 64 lanes x 16 bytes
        const unsigned xstamp = p.xepoch * 16u + (unsigned)(l + 1);
        if constexpr (SPLIT) {
            // K^T and V first: they are published while the Q projection runs, the partners' are taken after it (inside the attention loop below)
            const char* xl = xop + a * LD::RSX + b * 16;
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            f32x4 acc[FT][MTT];
            {
                f32x4 bk[FT];
                load_vec4<FT>(bk, W.b_in, D + wave * HD + 4 * b);
#pragma unroll
                for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                    for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = zero4;
                gemm_stream<PREC, FT, MTT, KC_D, PF, true, FT, WMAX, XM>(acc, wf, wq_of(W, 1), KC_D * CW, xl, LD::RSX, wq_of(W, 2), KC_D * CW);
                DT_STAMP(sl + 0);
#pragma unroll
                for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                    for (int tt = 0; tt < MTT; ++tt) kown[tt][ft] = PR::unscale(acc[ft][tt]) + bk[ft];
            }
            {
                float bv[FT];
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) bv[ft] = W.b_in[2 * D + wave * HD + 16 * ft + a];
#pragma unroll
                for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                    for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = zero4;
                gemm_stream<PREC, FT, MTT, KC_D, PF, false, FT, WMAX, XM>(acc, wf, wq_of(W, 2), KC_D * CW, xl, LD::RSX, wq_of(W, 0), KC_D * CW);
                DT_STAMP(sl + 1);
#pragma unroll
                for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                    for (int tt = 0; tt < MTT; ++tt) vown[tt][ft] = PR::unscale(acc[ft][tt]) + bv[ft];
            }
#pragma unroll
            for (int tk = 0; tk < NTRK; ++tk) {
                unsigned long long* xo = p.xch + ((size_t)(xslot + tk) * 2 + (l & 1)) * MT * 4 * XW + wave * XW + (size_t)tile * 4 * XW;
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) { dt_xstore(xo + ft * 128, lane, kown[tk][ft]); dt_xstore(xo + (FT + ft) * 128, lane, vown[tk][ft]); }
            }
            // Publish: ONE agent-scope release per workgroup.  Every wave drains its own tile stores, the workgroup meets, wave 0 releases (buffer_wbl2 sc1 + wait) and
            // raises the flag of this (track, tile); the other waves go on into the Q projection at once.  (Round 6 first fenced per wave: four waves of a CU fencing
            // at the same time take ~4x a single fence each - MI355X_MICROARCH.md price list - and the 640-track launch lost 45 us = 3.2 %, a single step 9 %; one
            // fence per workgroup and side: see DESIGN.md section 9.)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (wave == 0) {
                DT_XFENCE_RELEASE();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (restates the fence's wait where hipcc's scoreboard pass cannot drop it)
                if (lane < NTRK) __hip_atomic_store(p.xflag + ((size_t)(xslot + lane) * MT + tile) * DT_XFLAGS, xstamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            {
                f32x4 bq[FT];
                load_vec4<FT>(bq, W.b_in, wave * HD + 4 * b);
#pragma unroll
                for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                    for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = zero4;
                gemm_stream<PREC, FT, MTT, KC_D, PF, true, NTW, WMAX, XM>(acc, wf, wq_of(W, 0), KC_D * CW, xl, LD::RSX, w_out, KC_D * CW);
                DT_STAMP(sl + 2);
#pragma unroll
                for (int tt = 0; tt < MTT; ++tt) {
                    f32x4 tl[FT];
#pragma unroll
                    for (int ft = 0; ft < FT; ++ft) tl[ft] = (PR::unscale(acc[ft][tt]) + bq[ft]) * qscale;
#pragma unroll
                    for (int c = 0; c < NCF; ++c) qf[tt][c] = APR::template frag<FT>(tl, c);
                }
            }
        } else if constexpr (DIET) {
            // half-width passes: QNW weight tiles (= NCF/2 operand chunks of the head) at a time, so one accumulator set is
            // QNW x MTT tiles; the weight stream is unchanged (each pass prefetches the next pass's first chunks)
            constexpr int HC = NCF / 2;             // operand chunks per half
            static_assert(NCF % 2 == 0, "multi-track flavour needs an even number of head chunks");
            const char* xl = xop + a * LD::RSX + b * 16;
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int part = 0; part < 2; ++part) {              // 0: Q^T (scaled), 1: K^T - swapped products
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    f32x4 acc[QNW][MTT];
                    f32x4 bs[QNW];
                    load_vec4<QNW>(bs, W.b_in, part * D + wave * HD + h * QNW * 16 + 4 * b);
#pragma unroll
                    for (int ft = 0; ft < QNW; ++ft)
#pragma unroll
                        for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = zero4;
                    const u32x4* wp = wq_of(W, part) + (size_t)(h * QNW) * KC_D * CW;
                    const u32x4* wnx = h == 0 ? wp + (size_t)QNW * KC_D * CW : wq_of(W, part + 1);
                    gemm_stream<PREC, QNW, MTT, KC_D, PF, true, QNW, WMAX, XM>(acc, wf, wp, KC_D * CW, xl, LD::RSX, wnx, KC_D * CW);
                    const float sc = part == 0 ? qscale : 1.0f;
#pragma unroll
                    for (int tt = 0; tt < MTT; ++tt) {
                        f32x4 tl[QNW];
#pragma unroll
                        for (int ft = 0; ft < QNW; ++ft) tl[ft] = (acc[ft][tt] + bs[ft]) * sc;
#pragma unroll
                        for (int c = 0; c < HC; ++c) {
                            if (part == 0) qf[tt][h * HC + c] = APR::template frag<QNW>(tl, c);
                            else           kf[tt][h * HC + c] = APR::template frag<QNW>(tl, c);
                        }
                    }
                }
                DT_STAMP(sl + part);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {                       // V (normal product: lane holds 4 consecutive TOKENS of a feature)
                f32x4 acc[QNW][MTT];
                float bv[QNW];
#pragma unroll
                for (int ft = 0; ft < QNW; ++ft) bv[ft] = W.b_in[2 * D + wave * HD + 16 * (h * QNW + ft) + a];
#pragma unroll
                for (int ft = 0; ft < QNW; ++ft)
#pragma unroll
                    for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = zero4;
                const u32x4* wp = wq_of(W, 2) + (size_t)(h * QNW) * KC_D * CW;
                if (h == 0) gemm_stream<PREC, QNW, MTT, KC_D, PF, false, QNW, WMAX, XM>(acc, wf, wp, KC_D * CW, xl, LD::RSX, wp + (size_t)QNW * KC_D * CW, KC_D * CW);
                else        gemm_stream<PREC, QNW, MTT, KC_D, PF, false, NTW, WMAX, XM>(acc, wf, wp, KC_D * CW, xl, LD::RSX, w_out, KC_D * CW);
#pragma unroll
                for (int ft = 0; ft < QNW; ++ft) {
#pragma unroll
                    for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] += bv[ft];
#pragma unroll
                    for (int k = 0; k < NTRK; ++k) {
                        f32x4 tl[MT];
#pragma unroll
                        for (int i = 0; i < MT; ++i) tl[i] = acc[ft][k * MT + i];
#pragma unroll
                        for (int c = 0; c < NCK; ++c) vf[k][h * QNW + ft][c] = APR::template frag<MT>(tl, c);
                    }
                }
            }
            DT_STAMP(sl + 2);
            if (TWO) __syncthreads();   // O goes to Xop (HB holds the parked residual): every wave must be done reading Xop
        } else
        {
            const char* xl = xop + a * LD::RSX + b * 16;
            f32x4 acc[FT][MTT];
            // small per-feature vectors are fetched BEFORE the GEMM that precedes their use, so their global
            // latency hides under the MFMAs (accumulators start at zero, the bias is added in the epilogue)
            // (each bias is fetched right before its own GEMM so only one of them is live at a time)
            f32x4 bq[FT], bk[FT]; float bv[FT];
            load_vec4<FT>(bq, W.b_in, wave * HD + 4 * b);
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            // Q
#pragma unroll
            for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = zero4;
            gemm_stream<PREC, FT, MTT, KC_D, PF, true, FT, WMAX, XM>(acc, wf, wq_of(W, 0), KC_D * CW, xl, LD::RSX, wq_of(W, 1), KC_D * CW);
            DT_STAMP(sl + 0);
#pragma unroll
            for (int tt = 0; tt < MTT; ++tt) {
                f32x4 tl[FT];
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) tl[ft] = (PR::unscale(acc[ft][tt]) + bq[ft]) * qscale;
#pragma unroll
                for (int c = 0; c < NCF; ++c) qf[tt][c] = APR::template frag<FT>(tl, c);
            }
            // K
            load_vec4<FT>(bk, W.b_in, D + wave * HD + 4 * b);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = zero4;
            gemm_stream<PREC, FT, MTT, KC_D, PF, true, FT, WMAX, XM>(acc, wf, wq_of(W, 1), KC_D * CW, xl, LD::RSX, wq_of(W, 2), KC_D * CW);
            DT_STAMP(sl + 1);
#pragma unroll
            for (int tt = 0; tt < MTT; ++tt) {
                f32x4 tl[FT];
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) tl[ft] = PR::unscale(acc[ft][tt]) + bk[ft];
#pragma unroll
                for (int c = 0; c < NCF; ++c) kf[tt][c] = APR::template frag<FT>(tl, c);
            }
            // V (normal product: lane holds 4 consecutive TOKENS of feature 16*ft + a)
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) bv[ft] = W.b_in[2 * D + wave * HD + 16 * ft + a];
#pragma unroll
            for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = zero4;
            gemm_stream<PREC, FT, MTT, KC_D, PF, false, NTW, WMAX, XM>(acc, wf, wq_of(W, 2), KC_D * CW, xl, LD::RSX, w_out, KC_D * CW);
            DT_STAMP(sl + 2);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
#pragma unroll
                for (int tt = 0; tt < MTT; ++tt) acc[ft][tt] = PR::unscale(acc[ft][tt]) + bv[ft];
#pragma unroll
                for (int k = 0; k < NTRK; ++k) {
                    f32x4 tl[MT];                       // the MT key tiles of track k
#pragma unroll
                    for (int i = 0; i < MT; ++i) tl[i] = acc[ft][k * MT + i];
#pragma unroll
                    for (int c = 0; c < NCK; ++c) vf[k][ft][c] = APR::template frag<MT>(tl, c);
                }
            }
        }
#define DT_NQL MTL
#define DT_NQT MTT
#define DT_XQ X
#define DT_KNEXT (SPLIT || (prune && l + 2 == p.nlayers))
#include "dt_layer_tail.hip.inc"
#undef DT_NQL
#undef DT_NQT
#undef DT_XQ
#undef DT_KNEXT
    }

    // ---- the last layer, pruned: K and V of every token, everything else on the candidate rows ----------------------------------------
    // Compact row r < P + nspec <-> token row L + 2 r + can_pos; the rows above them replicate the last valid one and are discarded.
    if constexpr (PRUNABLE) if (prune) {
        // (this block's own copies of the lane coordinates, opaque to hipcc: otherwise it keeps the addresses and key indices it derives from them for the
        // layer loop alive for this block too, and the d = 512 x3 flavour spills them)
        int lane_ = tid & 63;
        asm volatile("" : "+v"(lane_));
        const int lane = lane_, a = lane & 15, b = lane >> 4;
        f32x4 Xc[NTW][NQP];
        const int l = p.nlayers - 1, sl = 4 + 12 * l, n = P + p.nspec;
        const DTLayerW& W = p.layer[l];
        const u32x4* w_out = W.w_out + (size_t)(wave * NTW) * KC_D * CW + lane;
        // the candidate rows of the residual, as f32, to their compact places in HB (dead at a layer's start; O goes there only after they are back in registers)
#pragma unroll
        for (int tt = 0; tt < MT; ++tt) {
            const int k = 16 * tt + a - L;
            if (k >= 0 && (k & 1) == p.can_pos && (k >> 1) < n) {
#pragma unroll
                for (int ft = 0; ft < NTW; ++ft) *(f32x4*)(hb + (k >> 1) * RSP + (fbase + 16 * ft + 4 * b) * 4) = X[ft][tt];
            }
        }
        u32x4 qf[NQP][NCF], kf[MT][NCF], vf[1][FT][NCK];
        f32x4 kown[1][FT], vown[1][FT];         // (SPLIT only)
        const char* xl = xop + a * LD::RSX + b * 16;
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        {
            // K and V first, on all MT tiles (the accumulators are independent of the order; the weight stream was pointed at K by the GEMM before)
            f32x4 acc[FT][MT];
            f32x4 bk[FT]; float bv[FT];
            load_vec4<FT>(bk, W.b_in, D + wave * HD + 4 * b);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                for (int tt = 0; tt < MT; ++tt) acc[ft][tt] = zero4;
            gemm_stream<PREC, FT, MT, KC_D, PF, true, FT, WMAX, XM>(acc, wf, wq_of(W, 1), KC_D * CW, xl, LD::RSX, wq_of(W, 2), KC_D * CW);
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
            gemm_stream<PREC, FT, MT, KC_D, PF, false, FT, WMAX, XM>(acc, wf, wq_of(W, 2), KC_D * CW, xl, LD::RSX, wq_of(W, 0), KC_D * CW);
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
        __syncthreads();                   // every wave is done reading Xop (K, V); the compact residual is visible
#pragma unroll
        for (int j = 0; j < NQP; ++j) {
            const int r = 16 * j + a < n ? 16 * j + a : n - 1;
#pragma unroll
            for (int ft = 0; ft < NTW; ++ft) Xc[ft][j] = *(const f32x4*)(hb + r * RSP + (fbase + 16 * ft + 4 * b) * 4);
        }
        clipped |= store_rows<PREC, NTW, NQP>(Xc, xop, LD::RSX, a, b, fbase);     // (store4 is a function of the value alone: the operand the full layer would have read)
        __syncthreads();
        {
            f32x4 acc[FT][NQP];
            f32x4 bq[FT];
            load_vec4<FT>(bq, W.b_in, wave * HD + 4 * b);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft)
#pragma unroll
                for (int tt = 0; tt < NQP; ++tt) acc[ft][tt] = zero4;
            gemm_stream<PREC, FT, NQP, KC_D, PF, true, NTW, WMAX, XM>(acc, wf, wq_of(W, 0), KC_D * CW, xl, LD::RSX, w_out, KC_D * CW);
            DT_STAMP(sl + 2);
#pragma unroll
            for (int tt = 0; tt < NQP; ++tt) {
                f32x4 tl[FT];
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) tl[ft] = (PR::unscale(acc[ft][tt]) + bq[ft]) * qscale;
#pragma unroll
                for (int c = 0; c < NCF; ++c) qf[tt][c] = APR::template frag<FT>(tl, c);
            }
        }
        const DTLayerW& Wn = W;             // (the last FFN2 prefetches a harmless re-read, as in a full last layer)
        constexpr size_t XW = 0; const unsigned xstamp = 0;       // (SPLIT only)
#define DT_NQL NQP
#define DT_NQT NQP
#define DT_XQ Xc
#define DT_KNEXT false
#include "dt_layer_tail.hip.inc"
#undef DT_NQL
#undef DT_NQT
#undef DT_XQ
#undef DT_KNEXT
        // back into the first NQP tiles of X for the decoder epilogue; the last tile repeats one of them (finite, discarded), so that no register of X
        // is live across this layer
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
            for (int j = 0; j < MT; ++j) X[ft][j] = Xc[ft][j < NQP ? j : NQP - 1];
    }

    // ---- epilogue: optional hidden states, decoder LN + Linear(d,1), softmax, argmax ----------------------------------
    if (p.hidden != nullptr) {
#pragma unroll
        for (int ft = 0; ft < NTW; ++ft)
#pragma unroll
            for (int tt = 0; tt < MTT; ++tt) {
                const int t = 16 * (tt % MTL) + a + tok0, gt = tbase + tt / MTL;
                if (t < T && gt < p.B) *(f32x4*)(p.hidden + ((size_t)gt * T + t) * D + fbase + 16 * ft + 4 * b) = X[ft][tt];
            }
    }
    {
        f32x4 dg[NTW], db[NTW];
        load_vec4<NTW>(dg, p.dec_g, fbase + 4 * b);
        load_vec4<NTW>(db, p.dec_b, fbase + 4 * b);
        layer_norm_regs<NTW, MTT>(X, dg, db, red1, red2, wave, a, b, invD);
    }
    f32x4 dw[NTW];
    load_vec4<NTW>(dw, p.dec_w, fbase + 4 * b);
#pragma unroll
    for (int tt = 0; tt < MTT; ++tt) {
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
    if constexpr (SPLIT) {
        // the workgroups of the later tiles hand the decoder products of their 16 tokens (per track) to the first one, which finishes the track(s)
        const unsigned stamp = p.xepoch * 16u + 1u;
        if (wave == 0 && tile != 0) {
            if (lane < 16 * NTRK) {
                const float v = (red1[lane] + red1[TP + lane]) + (red1[2 * TP + lane] + red1[3 * TP + lane]);
                __hip_atomic_store(p.xlg + ((size_t)(xslot + lane / 16) * MT + tile) * 16 + (lane & 15), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            DT_XFENCE_RELEASE();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane < NTRK) __hip_atomic_store(p.xflag + ((size_t)(xslot + lane) * MT + tile) * DT_XFLAGS + 4, stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (wave < NTRK && tile == 0) dt_xwait<MT - 1>(p.xflag + ((size_t)(xslot + wave) * MT + 1) * DT_XFLAGS + 4, DT_XFLAGS, stamp, p.xerr);
    }
    if (wave < NTRK && tbase + wave < p.B && !(SPLIT && tile != 0)) {         // wave k finishes track k of the workgroup
        const int n = P + p.nspec;
        const size_t trk_ = (size_t)tbase + wave;
        float lg = -INFINITY;
        if (lane < n) {
            const int tg = L + 2 * lane + p.can_pos, t = prune ? lane : wave * TP1 + tg;       // token of the track, its row in this workgroup (pruned: compact)
            if (SPLIT && tg >= TP1) lg = __hip_atomic_load(p.xlg + (size_t)(xslot + wave) * MT * 16 + tg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + p.dec_bias;
            else lg = ((red1[t] + red1[TP + t]) + (red1[2 * TP + t] + red1[3 * TP + t])) + p.dec_bias;
            p.logits[trk_ * n + lane] = lg;
        }
        float m = lg;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const float e = lane < n ? expf(lg - m) : 0.f;
        float sum = e;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
        const float pr = e / sum;
        if (p.probs != nullptr && lane < n) p.probs[trk_ * n + lane] = pr;
        float bv = lane < n ? pr : -1.f;
        int bi = lane;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (p.argmax != nullptr && lane == 0) p.argmax[trk_] = bi;
    }
    if (PREC == 2 && clipped && p.xerr != nullptr) *p.xerr = 2;       // host-mapped: the next call reports it (busca_dt_forward)
    DT_STAMP(4 + 12 * DT_MAX_LAYERS);      // end of the kernel: behind the slots of every layer, whatever p.nlayers is
}

// Instantiations that crash hipcc's 'AMDGPU Rewrite AGPR-Copy-MFMA' pass (ROCm 7.2, -mllvm -amdgpu-mfma-vgpr-form) - which of the register-starved f16
// flavours (300-700 spilled registers) it is changes with every edit of this file, so all three live here: they are compiled in their own
// translation unit WITHOUT that flag (busca_dt_aux.hip) and only declared in the main one.  X(PREC, MT, D, FF, E, NCHUNK_FF, NTRK, SPLIT).
#define BUSCA_DT_AUX_INSTANCES(X) X(1, 3, 512, 1024, 512, 1, 1, false) X(1, 4, 512, 1024, 512, 2, 1, false) X(1, 5, 256, 512, 512, 1, 1, false)
#ifndef BUSCA_DT_AUX_TU
#define BUSCA_DT_AUX_DECL(PR, M, DD, F, EE, NC, NT, SP) extern template __global__ void dt_fused_kernel<PR, M, DD, F, EE, NC, NT, SP>(const DTParams);
BUSCA_DT_AUX_INSTANCES(BUSCA_DT_AUX_DECL)
#undef BUSCA_DT_AUX_DECL
#endif

// the "unique rows" flavour of the one-track f32 / x3 kernel (same helpers, same layer tail text)
#include "dt_unique_kernel.hip.inc"

#pragma clang fp contract(fast)
