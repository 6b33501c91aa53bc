// ReID crop feature extractor: busca/reid/resnet.py:266-322 (ResNet-50 Bottleneck [3,4,6,3], max pool,
// red Linear 2048->512, L2 norm) driven as busca/network.py:542-575 does, i.e. with EVERY BatchNorm using
// batch statistics at inference (network.py:553-556).  One forward == one BN batch.
//
// Design (DESIGN.md "K-REID"):
//  * activations are fp16 NHWC; every conv is an implicit GEMM on v_mfma_f32_16x16x32_f16 with f32
//    accumulation: M = n*OH*OW pixels, N = Cout, K = KH*KW*Cin walked in 32-channel slices, so a K slice of
//    one pixel is 64 contiguous bytes of the input tensor.
//  * train-mode BN cannot be folded into the conv.  Instead: the conv epilogue writes the RAW conv output
//    plus per-(tile, channel) partial sums / sums of squares taken from the f32 accumulators
//    (deterministic two-level reduction, no atomics); `bn_finalize_kernel` turns them into per-channel
//    scale/shift; the NEXT conv applies relu(x*scale+shift) while it stages its A operand.  So each
//    activation tensor is written once and read once per consumer; no separate normalise pass exists.
//  * the products are "swapped" (weights are the MFMA A operand) so that a lane ends up with 4 consecutive
//    channels of one pixel -> 8-byte stores straight into NHWC.
//  * LDS tiles use a 16-byte-slot XOR swizzle (slot ^ ((row>>1)&3)) which makes the ds_read_b128 operand
//    reads conflict-free for 64-byte rows.


// Sum over the 16 lanes of a DPP row (lanes 16k .. 16k+15) as four VALU adds: xor 1, xor 2 (quad permutes), then the other quad
// of the 8-lane half (row_half_mirror) and the other half (row_mirror) - after the quad steps every lane of a quad holds the same
// value, so the mirrored lane carries exactly what the xor-4 / xor-8 butterfly partner would (bit-identical to the __shfl_xor
// butterfly, without its four LDS-crossbar round trips per value).
template <int CTRL> static __device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
static __device__ __forceinline__ float row16_sum(float x) {
    x += dpp_mov<0xB1>(x); x += dpp_mov<0x4E>(x); x += dpp_mov<0x141>(x); x += dpp_mov<0x140>(x);
    return x;
}
static __device__ __forceinline__ float row8_sum(float x) {          // over the 8-lane halves of a row
    x += dpp_mov<0xB1>(x); x += dpp_mov<0x4E>(x); x += dpp_mov<0x141>(x);
    return x;
}
// m / d for 0 <= m < 2^24 without the 40-instruction integer division (rd = 1.0f / d)
static __device__ __forceinline__ int fast_div(int m, int d, float rd) {
    int q = (int)((float)m * rd);
    const int r = m - q * d;
    if (r < 0) --q; else if (r >= d) ++q;
    return q;
}

struct ConvArgs {
    const _Float16* in;      // NHWC [n,H,W,Cin]   (stem: NHWC4 [n,384,128,4])
    const _Float16* w;       // [Cout][KH][KW][Cin] (stem: [64][7][8][4])
    const float* in_ss;      // [Cin][2] scale/shift applied (+ReLU) to the input while staging, or NULL
    _Float16* out;           // raw conv output NHWC [n,OH,OW,Cout]
    float* partials;         // [gridM][2][Cout] per-tile channel sums / sums of squares
    int n, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad;
    int M;                   // n*OH*OW
    int gridM, gridN;        // pixel tiles, channel blocks (1-D launch of 8*ceil(gridM/8)*gridN blocks)
    // fused block tail (conv_gemm64_kernel MODE 2): y = relu(out_ss(conv) + identity), identity = idt or idt_ss(idt)
    const float* out_ss;     // [Cout][2] scale/shift of THIS conv's BatchNorm
    const _Float16* idt;     // NHWC [M][Cout]
    const float* idt_ss;     // [Cout][2] or NULL
    // fused downsample branch (MODE 3): identity = idt_ss(ds_w * ds_in), a 1x1 conv of stride ds_stride accumulated in
    // a second set of registers by the same workgroup - its raw output never exists in HBM
    const _Float16* ds_in;   // NHWC [n,ds_H,ds_W,ds_Cin] (the bottleneck's input, final values)
    const _Float16* ds_w;    // [Cout][ds_Cin]
    const float* ds_in_ss;   // [ds_Cin][2] or NULL: ds_in is raw, the branch reads relu(ds_in * scale + shift)
    int ds_H, ds_W, ds_Cin, ds_stride;
    const _Float16* zero;    // >= 16 readable zero bytes (what out-of-image pieces load)
    // weighted BatchNorm statistics (busca_reid_forward_w): wts[crop] = how many times the crop occurs in the BatchNorm batch the
    // reference would have built (a candidate batch repeats the same detection for many tracks); NULL = every crop once.
    // The conv output of a repeated crop is the same every time, so each distinct crop is computed ONCE and only its
    // contribution to the batch statistics is multiplied.
    const float* wts; int OHWo;   // output pixels per crop (row m belongs to crop m / OHWo)
    unsigned long long* ts;       // BUSCA_CONV_TS: s_memtime stamps [workgroup][8] (wave 0), or NULL
    const _Float16* wkw;          // conv_kwave_kernel: this conv's weights in MFMA-fragment order [Cout/16][half step][lane][8]
};

// Phase stamps (BUSCA_CONV_TS) are compiled in only with -DBUSCA_CONV_PROBE: even the untaken branches cost ~1 % in the K loop.
#ifdef BUSCA_CONV_PROBE
#define CONV_TS(k) do { if (g.ts != nullptr && threadIdx.x == 0) g.ts[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define CONV_PROBE_ON(g_) ((g_).ts != nullptr)
#else
#define CONV_TS(k) do { } while (0)
#define CONV_PROBE_ON(g_) false
#endif
enum { CONV_NORMAL = 0, CONV_STATS_ONLY = 1, CONV_MERGE = 2, CONV_MERGE_DS = 3 };
struct SubConv { const _Float16* in; const _Float16* w; const float* in_ss; int H, W, Cin, KH, KW, stride, pad; };

static __device__ __forceinline__ int swz(int row, int slot) { return row * 64 + ((slot ^ ((row >> 1) & 3)) << 4); }

// BM = 128 pixels per block; BN = 64*WN channels per block; 4 waves arranged (4/WN) x WN.
template <int WN, bool STEM>
__global__ void __launch_bounds__(256) conv_gemm_kernel(const ConvArgs g) {
    constexpr int BM = 128, BN = 64 * WN, WM = 4 / WN;
    constexpr int PT = BM / WM / 16;                    // pixel tiles per wave (2 or 4)
    constexpr int NB_PIECES = BN * 4 / 256;             // 16-byte weight pieces per thread (1 or 2)
    __shared__ __attribute__((aligned(16))) char sA[BM * 64];
    __shared__ __attribute__((aligned(16))) char sB[BN * 64];
    __shared__ float sred[2][WM][BN];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int a = lane & 15, b = lane >> 4;
    // XCD-aware tile order: hardware block id L runs on XCD L % 8.  Each XCD walks its own pixel tiles
    // (xcd, xcd+8, ...) and, for one pixel tile, all channel blocks back to back - so an activation tile is
    // pulled from HBM once and re-read from that XCD's private L2 by the other gridN-1 channel blocks.
    const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
    const int mt = (seq / g.gridN) * 8 + xcd, nb = seq % g.gridN;
    if (mt >= g.gridM) return;
    const int m0 = mt * BM, c0 = nb * BN;

    // ---- per-thread staging coordinates: 2 activation pieces (row = tid/4 + 64*q, slot = tid%4) -------------
    const int slot = tid & 3;
    int prow[2]; long pbase[2]; int pih0[2], piw0[2]; bool pval[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        prow[q] = (tid >> 2) + 64 * q;
        const int m = m0 + prow[q];
        pval[q] = m < g.M;
        const int mm = pval[q] ? m : 0;
        const int img = mm / (g.OH * g.OW), rem = mm % (g.OH * g.OW);
        const int oh = rem / g.OW, ow = rem % g.OW;
        pih0[q] = oh * g.stride - g.pad;
        piw0[q] = ow * g.stride - g.pad;
        pbase[q] = (long)img * g.H * g.W;
    }
    const int cchunks = STEM ? 1 : g.Cin / 32;
    const int nsteps = STEM ? 7 : g.KH * g.KW * cchunks;
    const int Kw = STEM ? 224 : g.KH * g.KW * g.Cin;   // weight row length (halves)

    f32x4 acc[4][PT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    u32x4 ra[2], rb[NB_PIECES];
    auto load_step = [&](int s) {
        int kh, kw, cc;
        if (STEM) { kh = s; kw = 0; cc = 0; }
        else { cc = s % cchunks; const int t = s / cchunks; kw = t % g.KW; kh = t / g.KW; }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            u32x4 v = {0u, 0u, 0u, 0u};
            const int ih = pih0[q] + kh;
            if (pval[q] && ih >= 0 && ih < g.H) {
                if (STEM) {
                    // 8 kw taps x 4 channels = 64 B; this piece = taps 2*slot, 2*slot+1 (tap 7 has zero weights)
                    const int iw = piw0[q] + 2 * slot;
                    const _Float16* p = g.in + ((pbase[q] + (long)ih * g.W + iw) * 4);
                    u32x2 lo = {0u, 0u}, hi = {0u, 0u};
                    if (iw >= 0 && iw < g.W) lo = *(const u32x2*)p;
                    if (iw + 1 >= 0 && iw + 1 < g.W) hi = *(const u32x2*)(p + 4);
                    v = (u32x4){lo[0], lo[1], hi[0], hi[1]};
                } else {
                    const int iw = piw0[q] + kw;
                    if (iw >= 0 && iw < g.W) {
                        const int ch = cc * 32 + slot * 8;
                        v = *(const u32x4*)(g.in + ((pbase[q] + (long)ih * g.W + iw) * g.Cin + ch));
                        if (g.in_ss != nullptr) {
                            rh8 h = __builtin_bit_cast(rh8, v);
                            const f32x4* ss = (const f32x4*)(g.in_ss + 2 * ch);   // (scale,shift) pairs
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const f32x4 t = ss[e];
                                h[2 * e] = (_Float16)fmaxf(fmaf((float)h[2 * e], t[0], t[1]), 0.f);
                                h[2 * e + 1] = (_Float16)fmaxf(fmaf((float)h[2 * e + 1], t[2], t[3]), 0.f);
                            }
                            v = __builtin_bit_cast(u32x4, h);
                        }
                    }
                }
            }
            ra[q] = v;
        }
#pragma unroll
        for (int q = 0; q < NB_PIECES; ++q) {
            const int row = (tid >> 2) + 64 * q;
            rb[q] = *(const u32x4*)(g.w + (size_t)(c0 + row) * Kw + s * 32 + slot * 8);
        }
    };

    load_step(0);
    for (int s = 0; s < nsteps; ++s) {
#pragma unroll
        for (int q = 0; q < 2; ++q) *(u32x4*)(sA + swz(prow[q], slot)) = ra[q];
#pragma unroll
        for (int q = 0; q < NB_PIECES; ++q) *(u32x4*)(sB + swz((tid >> 2) + 64 * q, slot)) = rb[q];
        __syncthreads();
        if (s + 1 < nsteps) load_step(s + 1);            // global loads in flight during the MFMAs
        u32x4 wf[4], xf[PT];
#pragma unroll
        for (int i = 0; i < 4; ++i) wf[i] = *(const u32x4*)(sB + swz(wn * 64 + 16 * i + a, b));
#pragma unroll
        for (int j = 0; j < PT; ++j) xf[j] = *(const u32x4*)(sA + swz(wm * (BM / WM) + 16 * j + a, b));
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < PT; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, wf[i]), __builtin_bit_cast(h16x8, xf[j]), acc[i][j], 0, 0, 0);
        __syncthreads();
    }

    // ---- epilogue: raw output (fp16) + per-channel partial statistics from the f32 accumulators ---------------
    // acc[i][j] lane (a,b) r : channel c0 + wn*64 + 16i + 4b + r, pixel m0 + wm*(BM/WM) + 16j + a
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int m = m0 + wm * (BM / WM) + 16 * j + a;
            const f32x4 v = acc[i][j];
            if (m < g.M) {
                rh4 h; h[0] = (_Float16)v[0]; h[1] = (_Float16)v[1]; h[2] = (_Float16)v[2]; h[3] = (_Float16)v[3];
                *(rh4*)(g.out + (size_t)m * g.Cout + c0 + wn * 64 + 16 * i + 4 * b) = h;
                if (g.wts != nullptr) { const f32x4 wv = v * g.wts[m / g.OHWo]; s1 += wv; s2 += wv * v; }
                else { s1 += v; s2 += v * v; }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float x = s1[r], y = s2[r];
            x = row16_sum(x); y = row16_sum(y);
            if (a == 0) { sred[0][wm][wn * 64 + 16 * i + 4 * b + r] = x; sred[1][wm][wn * 64 + 16 * i + 4 * b + r] = y; }
        }
    }
    __syncthreads();
    if (tid < 2 * BN) {
        const int st = tid / BN, ch = tid % BN;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WM; ++w) t += sred[st][w][ch];
        g.partials[((size_t)mt * 2 + st) * g.Cout + c0 + ch] = t;
    }
}

// ---- v2 conv kernel for every non-stem layer ---------------------------------------------------------------------
// BK = 64 channels per step: a K slice of one pixel is a full 128-byte line, half as many barriers as BK = 32 and
// 32 MFMAs per wave between barriers.  128-byte LDS rows with an 8-slot XOR swizzle (slot ^ (row & 7)) keep the
// ds_read_b128 operand reads conflict-free.  The output tile is staged through LDS (reusing the operand tiles) and
// written as full rows (BN*2 contiguous bytes per pixel) instead of 8-byte fragments.

// MODE CONV_NORMAL: raw output + statistics.  CONV_STATS_ONLY: statistics only (first pass of a bottleneck's conv3:
// its 4x-expanded raw output is never written).  CONV_MERGE: second pass of conv3 - the epilogue applies this conv's
// BatchNorm, adds the identity (optionally through the downsample BatchNorm), ReLU, and writes the block output
// (resnet.py:108-128) - bit-identical to raw output + block_merge_kernel, minus one tensor write and two reads.
// One K step of register look-ahead: deeper rings were measured equal or slower at every batch size in rounds 1-2 and removed.
template <int WN, int MODE>
__global__ void __launch_bounds__(256) conv_gemm64_kernel(const ConvArgs g) {
    constexpr int BM = 128, BN = 64 * WN, WM = 4 / WN, PFD = 1;
    constexpr int PT = BM / WM / 16;                    // pixel tiles per wave (2 or 4)
    constexpr int NA = BM * 8 / 256;                    // 16-byte activation pieces per thread (4)
    constexpr int NB = BN * 8 / 256;                    // 16-byte weight pieces per thread (2 or 4)
    constexpr int ORS = BN * 2 + 16;                    // row stride (bytes) of the staged output tile
    constexpr int SMEM = (BM + BN) * 128 > BM * ORS ? (BM + BN) * 128 : BM * ORS;
    __shared__ __attribute__((aligned(16))) char smem[SMEM];
    __shared__ float sred[2][WM][BN];
    __shared__ __attribute__((aligned(16))) float sss[2 * 2048];   // (scale, shift) of every input channel (Cin <= 2048)
    char* sA = smem;
    char* sB = smem + BM * 128;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int a = lane & 15, b = lane >> 4;
    const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
    const int mt = (seq / g.gridN) * 8 + xcd, nb = seq % g.gridN;
    if (mt >= g.gridM) return;
    const int m0 = mt * BM, c0 = nb * BN;
    CONV_TS(0);

    // staging coordinates: piece q of this thread = row (tid>>3) + 32*q, 16-byte slot tid&7
    const int slot = tid & 7, r0 = tid >> 3;
    auto run_gemm = [&](const SubConv sc, f32x4 (&acc)[4][PT]) {
    // Per-thread address state is set up ONCE: the element offset of tap (0,0) / channel chunk 0 of every activation piece,
    // a bit mask of the taps that fall inside the image, and the weight-row offsets.  A K step then adds one wave-uniform
    // (scalar) offset per load.
    long abase[NA]; unsigned tapmask[NA];
    if (sc.KH == 1 && sc.stride == 1) {                 // 1x1, stride 1: input pixel = output pixel, no index arithmetic
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const int m = m0 + r0 + 32 * q;
            abase[q] = (long)m * sc.Cin + slot * 8;
            tapmask[q] = m < g.M ? 1u : 0u;
        }
    } else {
        const int ohw = g.OH * g.OW;
        const float rhw = 1.0f / (float)ohw, rw = 1.0f / (float)g.OW;
        const bool small = g.M < (1 << 24);
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const int m = m0 + r0 + 32 * q;
            const bool pv = m < g.M;
            const int mm = pv ? m : 0;
            const int img = small ? fast_div(mm, ohw, rhw) : mm / ohw, rem = mm - img * ohw;
            const int oh = small ? fast_div(rem, g.OW, rw) : rem / g.OW, ow = rem - oh * g.OW;
            const int ih0 = oh * sc.stride - sc.pad, iw0 = ow * sc.stride - sc.pad;
            abase[q] = ((long)img * sc.H * sc.W + (long)ih0 * sc.W + iw0) * sc.Cin + slot * 8;
            unsigned cm = 0, tm = 0;                    // column mask (kw) replicated over the valid kernel rows; KH, KW <= 3 here
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
                if (kw < sc.KW && iw0 + kw >= 0 && iw0 + kw < sc.W) cm |= 1u << kw;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
                if (kh < sc.KH && ih0 + kh >= 0 && ih0 + kh < sc.H) tm |= cm << (kh * sc.KW);
            tapmask[q] = pv ? tm : 0u;
        }
    }
    const int cchunks = sc.Cin / 64;
    const int nsteps_all = sc.KH * sc.KW * cchunks;
    const int sbeg = 0, send = nsteps_all;
    const int Kw = sc.KH * sc.KW * sc.Cin;
    unsigned wofs[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) wofs[q] = (unsigned)(c0 + r0 + 32 * q) * (unsigned)Kw + slot * 8;

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // The input transform relu(x*scale + shift) (the producer's train-mode BatchNorm) is applied when a prefetched
    // piece is written to LDS, NOT when it is loaded: consuming the value inside the load step would stall the wave
    // for the whole global latency and nothing would overlap with the MFMAs.  Scale/shift live in LDS.
    const bool tr = sc.in_ss != nullptr;
    u32x4 ra[PFD][NA], rb[PFD][NB];
    unsigned vmask[PFD];                                // bit q: piece q of this step lies inside the image
    auto load_step = [&](int s, u32x4 (&qa)[NA], u32x4 (&qb)[NB], unsigned& vm) {
        const int cc = s % cchunks, t = s / cchunks, kw = t % sc.KW, kh = t / sc.KW;
        const _Float16* sbase = sc.in + ((long)(kh * sc.W + kw) * sc.Cin + cc * 64);   // wave-uniform
        vm = 0;
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            const unsigned ok = (tapmask[q] >> t) & 1u;
            const _Float16* p = ok ? sbase + abase[q] : g.zero;          // padding / tail pixels read a zero line
            qa[q] = *(const u32x4*)p;
            vm |= ok << q;
        }
        const _Float16* wbase = sc.w + s * 64;
#pragma unroll
        for (int q = 0; q < NB; ++q) qb[q] = *(const u32x4*)(wbase + wofs[q]);
    };
    auto stage_step = [&](int s, const u32x4 (&qa)[NA], const u32x4 (&qb)[NB], unsigned vm) {
        if (tr) {
            const int ch = (s % cchunks) * 64 + slot * 8;
            f32x4 ss[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) ss[e] = *(const f32x4*)(sss + 2 * ch + 4 * e);   // (scale,shift) pairs
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                rh8 h = __builtin_bit_cast(rh8, qa[q]);
                if (vm & (1u << q)) {                   // zero padding stays zero (it is applied after BN + ReLU)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        h[2 * e] = (_Float16)fmaxf(fmaf((float)h[2 * e], ss[e][0], ss[e][1]), 0.f);
                        h[2 * e + 1] = (_Float16)fmaxf(fmaf((float)h[2 * e + 1], ss[e][2], ss[e][3]), 0.f);
                    }
                }
                *(rh8*)(sA + swz8(r0 + 32 * q, slot)) = h;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NA; ++q) *(u32x4*)(sA + swz8(r0 + 32 * q, slot)) = qa[q];
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) *(u32x4*)(sB + swz8(r0 + 32 * q, slot)) = qb[q];
    };

    CONV_TS(1);
#pragma unroll
    for (int d = 0; d < PFD; ++d)
        if (sbeg + d < send) load_step(sbeg + d, ra[d], rb[d], vmask[d]);
    if (tr) {                                           // behind the first operand loads: one exposed round trip instead of two
        for (int i = tid; i < sc.Cin / 2; i += 256) *(f32x4*)(sss + 4 * i) = *(const f32x4*)(sc.in_ss + 4 * i);
        __syncthreads();
    }
    auto mma_step = [&]() {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            u32x4 wf[4], xf[PT];
#pragma unroll
            for (int i = 0; i < 4; ++i) wf[i] = *(const u32x4*)(sB + swz8(wn * 64 + 16 * i + a, kk * 4 + b));
#pragma unroll
            for (int j = 0; j < PT; ++j) xf[j] = *(const u32x4*)(sA + swz8(wm * (BM / WM) + 16 * j + a, kk * 4 + b));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < PT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, wf[i]), __builtin_bit_cast(h16x8, xf[j]), acc[i][j], 0, 0, 0);
        }
    };
    int s0 = sbeg;
#pragma unroll 1
    for (; s0 < send; s0 += PFD) {
#pragma unroll
        for (int d = 0; d < PFD; ++d) {
            const int s = s0 + d;
            if (s < send) {
                const bool probe = CONV_PROBE_ON(g) && s == sbeg + 2;          // BUSCA_CONV_TS: phases of the third K step
                if (probe) CONV_TS(2);
                stage_step(s, ra[d], rb[d], vmask[d]);
                if (probe) CONV_TS(3);
                __syncthreads();
                if (probe) CONV_TS(4);
                if (s + PFD < send) load_step(s + PFD, ra[d], rb[d], vmask[d]);   // global loads fly during the MFMAs
                mma_step();
                if (probe) CONV_TS(5);
                __syncthreads();
                if (probe) CONV_TS(6);
            }
        }
    }
    };
    f32x4 acc[4][PT];
    run_gemm(SubConv{g.in, g.w, g.in_ss, g.H, g.W, g.Cin, g.KH, g.KW, g.stride, g.pad}, acc);
    f32x4 accd[4][PT];                                  // downsample branch (MODE 3 only; dead code otherwise)
    if constexpr (MODE == CONV_MERGE_DS) run_gemm(SubConv{g.ds_in, g.ds_w, g.ds_in_ss, g.ds_H, g.ds_W, g.ds_Cin, 1, 1, g.ds_stride, 0}, accd);

    // ---- epilogue: statistics from the f32 accumulators, output tile staged in LDS, full-row stores ----------------
    // acc[i][j] lane (a,b) r : channel (local) wn*64 + 16i + 4b + r, pixel (local) wm*(BM/WM) + 16j + a
    constexpr bool STATS = MODE == CONV_NORMAL || MODE == CONV_STATS_ONLY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
        f32x4 o01 = {}, o23 = {}, d01 = {}, d23 = {};   // (scale, shift) pairs of this lane's 4 channels: conv3's BN, downsample's BN
        if constexpr (MODE == CONV_MERGE_DS) {
            const int ch = c0 + wn * 64 + 16 * i + 4 * b;
            o01 = *(const f32x4*)(g.out_ss + 2 * ch); o23 = *(const f32x4*)(g.out_ss + 2 * ch + 4);
            d01 = *(const f32x4*)(g.idt_ss + 2 * ch); d23 = *(const f32x4*)(g.idt_ss + 2 * ch + 4);
        }
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int pl = wm * (BM / WM) + 16 * j + a;
            const f32x4 v = acc[i][j];
            if (MODE != CONV_STATS_ONLY) {
                rh4 h; h[0] = (_Float16)v[0]; h[1] = (_Float16)v[1]; h[2] = (_Float16)v[2]; h[3] = (_Float16)v[3];
                if constexpr (MODE == CONV_MERGE_DS) {  // same roundings as the two-kernel path: both raw conv outputs pass through fp16
                    const f32x4 dv = accd[i][j];
                    rh4 dh; dh[0] = (_Float16)dv[0]; dh[1] = (_Float16)dv[1]; dh[2] = (_Float16)dv[2]; dh[3] = (_Float16)dv[3];
                    h[0] = (_Float16)fmaxf(fmaf((float)h[0], o01[0], o01[1]) + fmaf((float)dh[0], d01[0], d01[1]), 0.f);
                    h[1] = (_Float16)fmaxf(fmaf((float)h[1], o01[2], o01[3]) + fmaf((float)dh[1], d01[2], d01[3]), 0.f);
                    h[2] = (_Float16)fmaxf(fmaf((float)h[2], o23[0], o23[1]) + fmaf((float)dh[2], d23[0], d23[1]), 0.f);
                    h[3] = (_Float16)fmaxf(fmaf((float)h[3], o23[2], o23[3]) + fmaf((float)dh[3], d23[2], d23[3]), 0.f);
                }
                *(rh4*)(smem + pl * ORS + (wn * 64 + 16 * i + 4 * b) * 2) = h;
            }
            if (STATS && m0 + pl < g.M) {
                if (g.wts != nullptr) { const f32x4 wv = v * g.wts[(m0 + pl) / g.OHWo]; s1 += wv; s2 += wv * v; }
                else { s1 += v; s2 += v * v; }
            }
        }
        if (STATS) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float x = s1[r], y = s2[r];
                x = row16_sum(x); y = row16_sum(y);
                if (a == 0) { sred[0][wm][wn * 64 + 16 * i + 4 * b + r] = x; sred[1][wm][wn * 64 + 16 * i + 4 * b + r] = y; }
            }
        }
    }
    __syncthreads();
    if (MODE != CONV_STATS_ONLY) {
        constexpr int PPR = BN * 2 / 16;                // 16-byte pieces per output row (8 or 16)
        constexpr int RPI = 256 / PPR;                  // rows per iteration
        const int pc = tid % PPR, pr = tid / PPR;
        float osc[8], osh[8], isc[8], ish[8];
        if (MODE == CONV_MERGE) {                       // this thread's 8 channels are the same for every row
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ch = c0 + pc * 8 + e;
                osc[e] = g.out_ss[2 * ch]; osh[e] = g.out_ss[2 * ch + 1];
                isc[e] = g.idt_ss ? g.idt_ss[2 * ch] : 1.f; ish[e] = g.idt_ss ? g.idt_ss[2 * ch + 1] : 0.f;
            }
        }
        // the identity rows of ALL this thread's pieces are requested up front: inside the loop every load would have to stay
        // behind the previous iteration's store (out and idt may alias as far as the compiler knows) - 8 exposed round trips
        u32x4 idq[MODE == CONV_MERGE ? BM / RPI : 1];
        if (MODE == CONV_MERGE) {
#pragma unroll
            for (int it = 0; it < BM / RPI; ++it) {
                const int row = pr + RPI * it;
                idq[it] = m0 + row < g.M ? *(const u32x4*)(g.idt + (size_t)(m0 + row) * g.Cout + c0 + pc * 8) : (u32x4){0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int it = 0; it < BM / RPI; ++it) {
            const int row = pr + RPI * it;
            if (m0 + row < g.M) {
                u32x4 v = *(const u32x4*)(smem + row * ORS + pc * 16);
                if (MODE == CONV_MERGE) {
                    const rh8 x = __builtin_bit_cast(rh8, v);
                    const rh8 d = __builtin_bit_cast(rh8, idq[it]);
                    rh8 o;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float val = fmaf((float)x[e], osc[e], osh[e]);
                        float id = (float)d[e];
                        if (g.idt_ss != nullptr) id = fmaf(id, isc[e], ish[e]);
                        o[e] = (_Float16)fmaxf(val + id, 0.f);
                    }
                    v = __builtin_bit_cast(u32x4, o);
                }
                *(u32x4*)(g.out + (size_t)(m0 + row) * g.Cout + c0 + pc * 8) = v;
            }
        }
    }
    if (STATS && tid < 2 * BN) {
        const int st = tid / BN, ch = tid % BN;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WM; ++w) t += sred[st][w][ch];
        g.partials[((size_t)mt * 2 + st) * g.Cout + c0 + ch] = t;
    }
    CONV_TS(7);
}

// Stage 1 of the statistics reduction: [gridM][2][C] f32 tile partials -> [BN_SLICES][2][C] f64.
// grid = (ceil(C/64), BN_SLICES); rows are split in contiguous slices so the reduction order is fixed.
#define BN_SLICES 64
__global__ void __launch_bounds__(256) bn_reduce_kernel(const float* __restrict__ partials, int gridM, int C, double* __restrict__ red) {
    __shared__ double sh[2][4][64];
    const int cl = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int rps = (gridM + BN_SLICES - 1) / BN_SLICES;
    const int r0 = blockIdx.y * rps, r1 = min(gridM, r0 + rps);
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        // independent loads, fixed summation order: 8 rows are requested before the first add (the loop was a chain of L2 latencies)
        int r = r0 + part;
        for (; r + 28 < r1; r += 32) {
            float a[8], b[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { a[k] = partials[((size_t)(r + 4 * k) * 2 + 0) * C + c]; b[k] = partials[((size_t)(r + 4 * k) * 2 + 1) * C + c]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) { s1 += (double)a[k]; s2 += (double)b[k]; }
        }
        for (; r < r1; r += 4) {
            s1 += (double)partials[((size_t)r * 2 + 0) * C + c];
            s2 += (double)partials[((size_t)r * 2 + 1) * C + c];
        }
    }
    sh[0][part][cl] = s1; sh[1][part][cl] = s2;
    __syncthreads();
    if (part == 0 && c < C) {
        red[((size_t)blockIdx.y * 2 + 0) * C + c] = (sh[0][0][cl] + sh[0][1][cl]) + (sh[0][2][cl] + sh[0][3][cl]);
        red[((size_t)blockIdx.y * 2 + 1) * C + c] = (sh[1][0][cl] + sh[1][1][cl]) + (sh[1][2][cl] + sh[1][3][cl]);
    }
}

// Stage 2: scale = gamma / sqrt(var + eps), shift = beta - mean*scale with the biased batch variance
// (nn.BatchNorm2d in train mode, eps 1e-5).
__global__ void __launch_bounds__(256) bn_finalize_kernel(const double* __restrict__ red, int C, double invM,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ ss) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int r = 0; r < BN_SLICES; ++r) { s1 += red[((size_t)r * 2 + 0) * C + c]; s2 += red[((size_t)r * 2 + 1) * C + c]; }
    const double mean = s1 * invM;
    double var = s2 * invM - mean * mean;
    if (var < 0.0) var = 0.0;
    const double sc = (double)gamma[c] / sqrt(var + 1e-5);
    ss[2 * c] = (float)sc;
    ss[2 * c + 1] = (float)((double)beta[c] - mean * sc);
}

// Both stages in ONE launch (round 3; 23 reduce + finalise pairs per 512-crop pass were 12.7 us each).  Stage 1 is bn_reduce_kernel's;
// the LAST workgroup of a 64-channel column to arrive - an agent-scope ticket per column - runs stage 2 for that column.
// Hand-off without fences: the slice sums leave as 8-byte agent-scope (write-through) stores, every storing wave drains its stores
// (s_waitcnt vmcnt(0)) before the workgroup's ticket increment, and the last arriver reads them back with agent-scope (L1-bypassing)
// loads - the "8-byte agent atomics on both sides" form of the inter-workgroup rules (no dependence on placement or dispatch
// order).  The last arriver puts the ticket back to zero, so the words need no per-call reset; they are zeroed when the workspace
// is allocated.  Deterministic: fixed slice order (four groups of 16 slices, then pairwise), whatever the arrival order.
typedef unsigned long long __attribute__((address_space(1))) gu64_t;
__global__ void __launch_bounds__(256) bn_reduce_finalize_kernel(const float* __restrict__ partials, int gridM, int C, double* red, int* ticket, double invM,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ ss) {
    __shared__ double sh[2][4][64];
    __shared__ int last;
    const int cl = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int rps = (gridM + BN_SLICES - 1) / BN_SLICES;
    const int r0 = blockIdx.y * rps, r1 = min(gridM, r0 + rps);
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        int r = r0 + part;
        for (; r + 28 < r1; r += 32) {
            float a[8], b[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { a[k] = partials[((size_t)(r + 4 * k) * 2 + 0) * C + c]; b[k] = partials[((size_t)(r + 4 * k) * 2 + 1) * C + c]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) { s1 += (double)a[k]; s2 += (double)b[k]; }
        }
        for (; r < r1; r += 4) {
            s1 += (double)partials[((size_t)r * 2 + 0) * C + c];
            s2 += (double)partials[((size_t)r * 2 + 1) * C + c];
        }
    }
    sh[0][part][cl] = s1; sh[1][part][cl] = s2;
    __syncthreads();
    if (part == 0 && c < C) {
        const double t1 = (sh[0][0][cl] + sh[0][1][cl]) + (sh[0][2][cl] + sh[0][3][cl]);
        const double t2 = (sh[1][0][cl] + sh[1][1][cl]) + (sh[1][2][cl] + sh[1][3][cl]);
        __hip_atomic_store((gu64_t*)(red + ((size_t)blockIdx.y * 2 + 0) * C + c), __builtin_bit_cast(unsigned long long, t1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store((gu64_t*)(red + ((size_t)blockIdx.y * 2 + 1) * C + c), __builtin_bit_cast(unsigned long long, t2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // every storing wave drains before the ticket
    __syncthreads();
    if (threadIdx.x == 0) {
        const int old = __hip_atomic_fetch_add(ticket + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = old == BN_SLICES - 1 ? 1 : 0;
        if (last) __hip_atomic_store(ticket + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return;
    // stage 2 for this column: thread (cl, part) sums slices 16 part .. 16 part + 15 in order, all 32 loads requested first
    double q1 = 0.0, q2 = 0.0;
    if (c < C) {
        unsigned long long v1[16], v2[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            v1[k] = __hip_atomic_load((gu64_t*)(red + ((size_t)(16 * part + k) * 2 + 0) * C + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            v2[k] = __hip_atomic_load((gu64_t*)(red + ((size_t)(16 * part + k) * 2 + 1) * C + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) { q1 += __builtin_bit_cast(double, v1[k]); q2 += __builtin_bit_cast(double, v2[k]); }
    }
    __syncthreads();                                    // sh is reused
    sh[0][part][cl] = q1; sh[1][part][cl] = q2;
    __syncthreads();
    if (part == 0 && c < C) {
        const double t1 = (sh[0][0][cl] + sh[0][1][cl]) + (sh[0][2][cl] + sh[0][3][cl]);
        const double t2 = (sh[1][0][cl] + sh[1][1][cl]) + (sh[1][2][cl] + sh[1][3][cl]);
        const double mean = t1 * invM;
        double var = t2 * invM - mean * mean;
        if (var < 0.0) var = 0.0;
        const double sc = (double)gamma[c] / sqrt(var + 1e-5);
        ss[2 * c] = (float)sc;
        ss[2 * c + 1] = (float)((double)beta[c] - mean * sc);
    }
}

// Small grids (few tiles): one kernel does both stages.  64 channels per block, 16 row lanes (1024 threads): the kernel
// is a chain of dependent loads, so its duration is the number of rows one lane walks.
__global__ void __launch_bounds__(1024) bn_finalize_direct_kernel(const float* __restrict__ partials, int gridM, int C, double invM,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  float* __restrict__ ss) {
    __shared__ double sh[2][16][64];
    const int cl = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        int r = part;
        for (; r + 112 < gridM; r += 128) {          // 8 independent row loads in flight per lane, same summation order
            float a[8], b[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { a[k] = partials[((size_t)(r + 16 * k) * 2 + 0) * C + c]; b[k] = partials[((size_t)(r + 16 * k) * 2 + 1) * C + c]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) { s1 += (double)a[k]; s2 += (double)b[k]; }
        }
        for (; r < gridM; r += 16) {
            s1 += (double)partials[((size_t)r * 2 + 0) * C + c];
            s2 += (double)partials[((size_t)r * 2 + 1) * C + c];
        }
    }
    sh[0][part][cl] = s1; sh[1][part][cl] = s2;
    __syncthreads();
    if (part == 0 && c < C) {
        s1 = 0.0; s2 = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { s1 += sh[0][k][cl]; s2 += sh[1][k][cl]; }
        const double mean = s1 * invM;
        double var = s2 * invM - mean * mean;
        if (var < 0.0) var = 0.0;
        const double sc = (double)gamma[c] / sqrt(var + 1e-5);
        ss[2 * c] = (float)sc;
        ss[2 * c + 1] = (float)((double)beta[c] - mean * sc);
    }
}

// u8 BGR crops [n,384,128,3] -> fp16 NHWC4 RGB0, normalised as network.py:470-476 (ghost std 0.299)
__global__ void __launch_bounds__(256) reid_preprocess_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ zero_norm, size_t npix,
                                                              _Float16* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    if (zero_norm != nullptr && zero_norm[i / (384 * 128)]) { *(rh4*)(out + i * 4) = (rh4){(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f}; return; }
    const double mean[3] = {0.406, 0.456, 0.485}, stdv[3] = {0.225, 0.224, 0.299};
    float n3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = (float)crops[i * 3 + c] / 255.0f;
        x = (float)((double)x - mean[c]);
        n3[c] = (float)((double)x / stdv[c]);
    }
    rh4 hv; hv[0] = (_Float16)n3[2]; hv[1] = (_Float16)n3[1]; hv[2] = (_Float16)n3[0]; hv[3] = (_Float16)0.f;
    *(rh4*)(out + i * 4) = hv;
}

// relu(bn1(stem)) then MaxPool2d(3, 2, 1): raw [n,192,64,64] -> ready [n,96,32,64]; thread = 8 channels of one output pixel
__global__ void __launch_bounds__(256) maxpool_bn_relu_kernel(const _Float16* __restrict__ raw, const float* __restrict__ ss, int n,
                                                              _Float16* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)n * 96 * 32 * 8;
    if (i >= total) return;
    const int cg = i & 7; size_t p = i >> 3;
    const int ow = p % 32; p /= 32;
    const int oh = p % 96; const int img = p / 96;
    float sc[8], sf[8], best[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = ss[2 * (cg * 8 + e)]; sf[e] = ss[2 * (cg * 8 + e) + 1]; best[e] = -INFINITY; }
    for (int dy = 0; dy < 3; ++dy) {
        const int ih = 2 * oh - 1 + dy;
        if (ih < 0 || ih >= 192) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int iw = 2 * ow - 1 + dx;
            if (iw < 0 || iw >= 64) continue;
            const rh8 h = *(const rh8*)(raw + (((size_t)img * 192 + ih) * 64 + iw) * 64 + cg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) best[e] = fmaxf(best[e], fmaxf(fmaf((float)h[e], sc[e], sf[e]), 0.f));
        }
    }
    rh8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (_Float16)best[e];
    *(rh8*)(out + (((size_t)img * 96 + oh) * 32 + ow) * 64 + cg * 8) = o;
}

// y = relu(bn3(raw3) + identity), identity = ready tensor or bn_ds(raw_ds)   (resnet.py:108-128)
__global__ void __launch_bounds__(256) block_merge_kernel(const _Float16* __restrict__ raw3, const float* __restrict__ ss3,
                                                          const _Float16* __restrict__ idt, const float* __restrict__ ssd,
                                                          size_t npix, int C, _Float16* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int cgs = C / 8;
    if (i >= npix * cgs) return;
    const int c = (int)(i % cgs) * 8;
    const rh8 x = *(const rh8*)(raw3 + i * 8);
    const rh8 d = *(const rh8*)(idt + i * 8);
    rh8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = fmaf((float)x[e], ss3[2 * (c + e)], ss3[2 * (c + e) + 1]);
        float id = (float)d[e];
        if (ssd != nullptr) id = fmaf(id, ssd[2 * (c + e)], ssd[2 * (c + e) + 1]);
        o[e] = (_Float16)fmaxf(v + id, 0.f);
    }
    *(rh8*)(out + i * 8) = o;
}

// AdaptiveMaxPool2d(1) over the 12x4 map: ready [n,48,2048] -> f32 [n,2048]
__global__ void __launch_bounds__(256) global_maxpool_kernel(const _Float16* __restrict__ x, int n, int HW, int C, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * C) return;
    const int c = i % C; const int img = i / C;
    float m = -INFINITY;
    const _Float16* xp = x + (size_t)img * HW * C + c;
    int p = 0;
    for (; p + 7 < HW; p += 8) {                       // 8 positions in flight (max is order-independent)
        _Float16 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = xp[(size_t)(p + u) * C];
#pragma unroll
        for (int u = 0; u < 8; ++u) m = fmaxf(m, (float)v[u]);
    }
    for (; p < HW; ++p) m = fmaxf(m, (float)xp[(size_t)p * C]);
    out[i] = m;
}

// fc7 = pool @ red.weight^T + red.bias (resnet.py:300-301); wt = red.weight transposed [2048][512].
// grid (ceil(n/CB), 8): a block owns 64 outputs of CB crops (each weight is fetched once per CB crops), its 4 waves split
// K; per output the summation order is fixed (k = kg, kg+4, ... as an fmaf chain, then pairwise) whatever the batch size.
// CB = 8 for large batches; CB = 1 keeps small batches spread over n*8 workgroups (the kernel is latency-bound there).
template <int GEMV_CB>
__global__ void __launch_bounds__(256) reid_tail_gemv_kernel(const float* __restrict__ pool, const float* __restrict__ wt,
                                                             const float* __restrict__ bias, float* __restrict__ raw, int n) {
    __shared__ float sp[GEMV_CB][2048];
    const int img0 = blockIdx.x * GEMV_CB, o = blockIdx.y * 64 + (threadIdx.x & 63), kg = threadIdx.x >> 6;
    const int nc = min(GEMV_CB, n - img0);
    for (int c = 0; c < nc; ++c)
        for (int k = threadIdx.x; k < 2048; k += 256) sp[c][k] = pool[(size_t)(img0 + c) * 2048 + k];
    __syncthreads();
    float acc[GEMV_CB];
#pragma unroll
    for (int c = 0; c < GEMV_CB; ++c) acc[c] = 0.f;
    // 16 weight loads in flight per thread (the loop is otherwise a chain of L2 round trips: 45-60 us for 1 MFLOP per crop);
    // every accumulator still sums its k in ascending order
    for (int k0 = kg; k0 < 2048; k0 += 64) {
        float w[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) w[u] = wt[(size_t)(k0 + 4 * u) * 512 + o];
#pragma unroll
        for (int u = 0; u < 16; ++u)
#pragma unroll
            for (int c = 0; c < GEMV_CB; ++c) acc[c] = fmaf(sp[c][k0 + 4 * u], w[u], acc[c]);     // rows >= nc hold stale data; never stored
    }
    __syncthreads();
    float (*part)[4][64] = (float (*)[4][64])&sp[0][0];                       // [crop][kg][64], over the pooled rows
#pragma unroll
    for (int c = 0; c < GEMV_CB; ++c) part[c][kg][threadIdx.x & 63] = acc[c];
    __syncthreads();
    if (kg == 0)
        for (int c = 0; c < nc; ++c)
            raw[(size_t)(img0 + c) * 512 + o] = ((part[c][0][threadIdx.x] + part[c][1][threadIdx.x]) + (part[c][2][threadIdx.x] + part[c][3][threadIdx.x])) + bias[o];
}

// feats = F.normalize(fc7, p=2, dim=1) (resnet.py:322, eps 1e-12); in place, one block per crop
// `flag` (split-fp16 flavour; host-mapped, else NULL): the pass's (scale, shift) table `ss` [nss] and the features are scanned for non-finite values - an
// operand that left the fp16 range while it was staged (reid_x3.hip.inc does not clamp) makes its conv's output and BatchNorm statistics non-finite -
// and the pass reports 2 ("reid_status") instead of returning features computed from clipped activations.
// NORMALISE false (`output` = norm, include/busca_reid_bn.h): fc7 stays as it is; the scan is the same.
template <bool NORMALISE>
__global__ void __launch_bounds__(256) reid_l2norm_kernel(float* __restrict__ feats, const float* __restrict__ ss, int nss, int* flag) {
    __shared__ float sr[4];
    const int img = blockIdx.x, tid = threadIdx.x;
    const float o0 = feats[(size_t)img * 512 + tid], o1 = feats[(size_t)img * 512 + tid + 256];
    float q = o0 * o0 + o1 * o1;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
    if ((tid & 63) == 0) sr[tid >> 6] = q;
    __syncthreads();
    const float tot = (sr[0] + sr[1]) + (sr[2] + sr[3]);
    const float nrm = fmaxf(sqrtf(tot), 1e-12f);
    if (NORMALISE) {
        feats[(size_t)img * 512 + tid] = o0 / nrm;
        feats[(size_t)img * 512 + tid + 256] = o1 / nrm;
    }
    if (flag != nullptr) {
        bool bad = !(fabsf(tot) <= 3.0e38f);
        for (int i = img * 256 + tid; i < nss; i += gridDim.x * 256) bad = bad || !(fabsf(ss[i]) <= 3.0e38f);
        if (bad) *flag = 2;
    }
}
