// Running-statistics BatchNorm of the ReID extractor (include/busca_reid_bn.h): the two kernels that stand between torch's `running_mean` / `running_var` and the
// (scale, shift) tables every conv kernel reads.  One thread per BatchNorm channel (26 560 of them); both run once per statistics change, never in a forward.
constexpr int REID_NCONV = 53;
constexpr int REID_BN_CHANNELS = 26560;

// Host-built at weight load, handed to the kernels by value: conv i owns the channels first[i] .. first[i + 1] - 1.  Its statistics sit at run[2 first[i]] (mean[C], then
// var[C]), its pairs at ss[2 first[i]] ([C][2]), its gamma / beta at f[g_off[i]] / f[b_off[i]].
struct ReidBnMap { int first[REID_NCONV + 1]; int g_off[REID_NCONV], b_off[REID_NCONV]; };
struct ReidBnCounts { double count[REID_NCONV]; };       // M of a batch: crops x output pixels of the conv (at load: the pixels per crop)

// What a forward does with the running statistics.
struct ReidBnMode {
    bool running = false;        // read the fixed table instead of the batch's
    int output = 0;              // BUSCA_REID_OUT_*
    double momentum = 0.0;       // != 0: update the running statistics from the batch's, rebuild the fixed table
};

__device__ inline int reid_bn_conv_of(const ReidBnMap& m, int ch) {
    int i = 0;
    while (i + 1 < REID_NCONV && ch >= m.first[i + 1]) ++i;
    return i;
}

// (scale, shift) as torch's inference BatchNorm forms them, in float32: alpha = gamma / sqrt(var + eps), beta' = beta - mean * alpha
__global__ void __launch_bounds__(256) reid_bn_table_kernel(const float* __restrict__ run, const float* __restrict__ f, ReidBnMap m, float* __restrict__ ss) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= REID_BN_CHANNELS) return;
    const int i = reid_bn_conv_of(m, ch), j = ch - m.first[i], C = m.first[i + 1] - m.first[i];
    const float mean = run[2 * m.first[i] + j], var = run[2 * m.first[i] + C + j];
    const float inv = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, 1e-5f)));
    const float alpha = __fmul_rn(f[m.g_off[i] + j], inv);
    ss[2 * ch] = alpha;
    ss[2 * ch + 1] = __fsub_rn(f[m.b_off[i] + j], __fmul_rn(mean, alpha));
}

// torch's train-mode update from the finished (scale, shift) table of a batch-statistics pass: the finalisers wrote scale = gamma / sqrt(var + eps) and
// shift = beta - mean * scale (var the biased batch variance), so mean = (beta - shift) / scale and var + eps = (gamma / scale)^2, in float64.  torch keeps the
// UNBIASED variance var * M / (M - 1).  A channel with gamma == 0 has the pair (0, beta): nothing of the batch is left in it - and none of its outputs depends on
// its statistics; it keeps what it has, as does a channel whose pair is not finite (a split-fp16 pass that left its range).
__global__ void __launch_bounds__(256) reid_bn_update_kernel(const float* __restrict__ ss, const float* __restrict__ f, ReidBnMap m, ReidBnCounts cnt, double momentum,
                                                             float* __restrict__ run) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= REID_BN_CHANNELS) return;
    const int i = reid_bn_conv_of(m, ch), j = ch - m.first[i], C = m.first[i + 1] - m.first[i];
    const double gamma = (double)f[m.g_off[i] + j], beta = (double)f[m.b_off[i] + j];
    const double sc = (double)ss[2 * ch], sh = (double)ss[2 * ch + 1];
    if (gamma == 0.0 || sc == 0.0 || !(fabs(sc) <= 3.0e38) || !(fabs(sh) <= 3.0e38)) return;
    const double mean = (beta - sh) / sc;
    const double r = gamma / sc;
    double var = r * r - 1e-5;
    if (var < 0.0) var = 0.0;
    const double M = cnt.count[i];
    if (M > 1.0) var *= M / (M - 1.0);
    float* pm = run + 2 * m.first[i] + j;
    float* pv = run + 2 * m.first[i] + C + j;
    *pm = (float)((1.0 - momentum) * (double)*pm + momentum * mean);
    *pv = (float)((1.0 - momentum) * (double)*pv + momentum * var);
}
