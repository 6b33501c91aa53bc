// Weights of the ReID extractor: the conv list, the blob layout and the repacking into the operand layouts of each flavour's kernels.

struct ReidSpec { int cout, cin, k, stride, pad; };

// Forward order of the 53 convs (resnet.py:169-182, _make_layer :225-252): stem, then per bottleneck
// conv1 1x1, conv2 3x3 (stride on the first block of layer2-4), conv3 1x1, [downsample 1x1 stride s].
static std::vector<ReidSpec> reid_specs() {
    std::vector<ReidSpec> v;
    v.push_back({64, 3, 7, 2, 3});
    const int nblk[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512};
    int inpl = 64;
    for (int li = 0; li < 4; ++li)
        for (int b = 0; b < nblk[li]; ++b) {
            const int s = (b == 0 && li > 0) ? 2 : 1, p = planes[li];
            v.push_back({p, inpl, 1, 1, 0});
            v.push_back({p, p, 3, s, 1});
            v.push_back({p * 4, p, 1, 1, 0});
            if (b == 0) v.push_back({p * 4, inpl, 1, s, 0});
            inpl = p * 4;
        }
    return v;
}

extern "C" size_t busca_reid_blob_floats(void) {
    size_t n = 0;
    for (const ReidSpec& s : reid_specs()) n += (size_t)s.cout * s.cin * s.k * s.k + 2 * (size_t)s.cout;
    return n + 512 * 2048 + 512;
}

extern "C" int busca_reid_load_weights(busca_ctx* c, const float* blob, size_t blob_floats) {
    return busca_reid_load_weights_ex(c, blob, blob_floats, BUSCA_PREC_F16);
}

extern "C" int busca_reid_load_weights_ex(busca_ctx* c, const float* blob, size_t blob_floats, int32_t precision) {
    if (!c) return BUSCA_EINVAL;
    if (!blob || blob_floats != busca_reid_blob_floats()) return fail(c, BUSCA_EINVAL, "ReID blob has %zu floats, expected %zu", blob_floats, busca_reid_blob_floats());
    if (precision != BUSCA_PREC_F16 && precision != BUSCA_PREC_F32 && precision != BUSCA_PREC_F16X3) return fail(c, BUSCA_EINVAL, "bad ReID precision %d", precision);
    HIP_TRY(c, hipSetDevice(c->device));
    ReidState& R = *c->reid;
    if (R.loaded) { HIP_TRY(c, hipDeviceSynchronize()); reid_free(R); }
    R.prec = precision;
    if (precision == BUSCA_PREC_F16X3) {
        HIP_TRY(c, hipHostMalloc((void**)&R.xerr, sizeof(int), hipHostMallocMapped)); *R.xerr = 0;
        HIP_TRY(c, hipHostGetDevicePointer((void**)&R.xerr_dev, R.xerr, 0));
    }
    reid_knobs_from_env(R.k);
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) R.num_cu = prop.multiProcessorCount; }
    std::vector<_Float16> hx3;        // F16X3: hi / lo fragment-ordered weights
    std::vector<float> hw;            // packed conv weights as floats (converted to fp16 below when needed)
    std::vector<float> hf;
    std::vector<_Float16> hpk;        // fragment-packed 3x3 weights
    std::vector<_Float16> hkw;        // fragment-packed copies of every non-stem conv for conv_kwave_kernel
    size_t ss_total = 0;
    const float* cur = blob;
    for (const ReidSpec& s : reid_specs()) {
        ReidConv cv{s.cout, s.cin, s.k, s.stride, s.pad, 0, 0, 0, 0};
        const float* W = cur; cur += (size_t)s.cout * s.cin * s.k * s.k;   // torch layout [co][ci][kh][kw]
        while (hw.size() % 8) hw.push_back(0.f);                            // 16-byte aligned rows in either precision
        cv.w_off = hw.size();
        if (s.cin == 3) {                                                   // stem -> [64][7][8][4], RGB channel order kept
            for (int co = 0; co < s.cout; ++co)
                for (int kh = 0; kh < 7; ++kh)
                    for (int kw = 0; kw < 8; ++kw)
                        for (int ci = 0; ci < 4; ++ci)
                            hw.push_back((kw < 7 && ci < 3) ? W[((size_t)(co * 3 + ci) * 7 + kh) * 7 + kw] : 0.f);
        } else {
            for (int co = 0; co < s.cout; ++co)
                for (int kh = 0; kh < s.k; ++kh)
                    for (int kw = 0; kw < s.k; ++kw)
                        for (int ci = 0; ci < s.cin; ++ci)
                            hw.push_back(W[((size_t)(co * s.cin + ci) * s.k + kh) * s.k + kw]);
        }
        const bool pk3 = s.k == 3 && s.stride == 1 && s.cin % 64 == 0 && (s.cout == 64 || s.cout == 128 || s.cout == 256);
        const bool pk1 = s.k == 1 && ((s.cin == 256 && (s.cout == 64 || s.cout == 128)) || (s.cin == 512 && (s.cout == 128 || s.cout == 256)) ||
                                       (s.cin == 1024 && (s.cout == 256 || s.cout == 512)));   // conv1 fused into the layer-1/2/3 tails
        if (precision == BUSCA_PREC_F16 && (pk3 || pk1)) {
            // fragment order for conv3x3_halo_kernel / tail_conv1_kernel: [Cout/16][step = chunk*taps + tap][kk][lane = 16b + a][8]:
            //   W[co = 16ct + a][kh][kw][ci = chunk*64 + kk*32 + 8b + e]
            cv.wpk_off = hpk.size();
            const int taps = s.k * s.k, nsteps = (s.cin / 64) * taps;
            hpk.resize(hpk.size() + (size_t)s.cout * s.cin * taps);
            _Float16* dst = hpk.data() + cv.wpk_off;
            for (int ct = 0; ct < s.cout / 16; ++ct)
                for (int st = 0; st < nsteps; ++st)
                    for (int kk = 0; kk < 2; ++kk)
                        for (int ln = 0; ln < 64; ++ln)
                            for (int e = 0; e < 8; ++e) {
                                const int a = ln & 15, b = ln >> 4, chunk = st / taps, tap = st % taps;
                                const int co = 16 * ct + a, ci = chunk * 64 + kk * 32 + 8 * b + e;
                                dst[((((size_t)ct * nsteps + st) * 2 + kk) * 64 + ln) * 8 + e] = (_Float16)hw[cv.w_off + ((size_t)co * taps + tap) * s.cin + ci];
                            }
        }
        if (precision == BUSCA_PREC_F16 && s.cin % 64 == 0 && s.cout % 64 == 0) {
            // fragment order for conv_kwave_kernel: [Cout/16][half step h = 2 (tap*chunks + chunk) + kk][lane = 16b + a][8] =
            //   W[co = 16ct + a][tap][ci = chunk*64 + kk*32 + 8b + e]  - a wave fetches an MFMA operand as 1 KiB of contiguous memory
            cv.wkw_off = hkw.size();
            const int taps = s.k * s.k, cch = s.cin / 64, nhalf = 2 * taps * cch;
            hkw.resize(hkw.size() + (size_t)s.cout * s.cin * taps);
            _Float16* dst = hkw.data() + cv.wkw_off;
            for (int ct = 0; ct < s.cout / 16; ++ct)
                for (int h = 0; h < nhalf; ++h)
                    for (int ln = 0; ln < 64; ++ln)
                        for (int e = 0; e < 8; ++e) {
                            const int a = ln & 15, b = ln >> 4, st = h >> 1, kk = h & 1, tap = st / cch, chunk = st % cch;
                            const int co = 16 * ct + a, ci = chunk * 64 + kk * 32 + 8 * b + e;
                            dst[(((size_t)ct * nhalf + h) * 64 + ln) * 8 + e] = (_Float16)hw[cv.w_off + ((size_t)co * taps + tap) * s.cin + ci];
                        }
        }
        if (precision == BUSCA_PREC_F16X3) {
            // [Cout/16][half step h][hi, lo][lane = 16b + a][8]: W'[co = 16ct + a][k(h, b, e)], W' = W * 2^kc[co] with max |W'| in [2^12, 2^13)
            //   convs: h = 2 (tap * chunks + chunk) + kk, k = (tap, ci = chunk*64 + kk*32 + 8b + e)
            //   stem:  h = kernel row kh (0..7, row 7 zero), k = (tap kw = 2b + (e >> 2), channel e & 3)   - the [64][7][8][4] layout above
            const bool stem = s.cin == 3;
            const int taps = s.k * s.k, cch = stem ? 1 : s.cin / 64, nhalf = stem ? 8 : 2 * taps * cch;
            const size_t krow = stem ? 224 : (size_t)taps * s.cin;
            cv.wx3_off = hx3.size();
            hx3.resize(hx3.size() + (size_t)s.cout * nhalf * 32 * 2);
            cv.inv_off = hf.size();
            hf.resize(hf.size() + s.cout);
            _Float16* dst = hx3.data() + cv.wx3_off;
            for (int co = 0; co < s.cout; ++co) {
                float m = 0.f;
                for (size_t k = 0; k < krow; ++k) m = std::max(m, std::fabs(hw[cv.w_off + (size_t)co * krow + k]));
                int ex = 0, kc = 0;
                if (m > 0.f && std::isfinite(m)) { std::frexp(m, &ex); kc = std::min(40, std::max(-40, 13 - ex)); }
                hf[cv.inv_off + co] = std::ldexp(1.0f, -kc) / X3_XS;
                const int ct = co / 16, a = co % 16;
                for (int h = 0; h < nhalf; ++h)
                    for (int b = 0; b < 4; ++b)
                        for (int e = 0; e < 8; ++e) {
                            float w;
                            if (stem) w = h < 7 ? hw[cv.w_off + ((size_t)(co * 7 + h) * 8 + 2 * b + (e >> 2)) * 4 + (e & 3)] : 0.f;
                            else { const int st = h >> 1, kk = h & 1, tap = st / cch, chunk = st % cch; w = hw[cv.w_off + ((size_t)co * taps + tap) * s.cin + chunk * 64 + kk * 32 + 8 * b + e]; }
                            const float ws = std::ldexp(w, kc);
                            const _Float16 hi = (_Float16)ws, lo = (_Float16)(ws - (float)hi);
                            const size_t base = (((size_t)ct * nhalf + h) * 2) * 512 + (size_t)(16 * b + a) * 8 + e;
                            dst[base] = hi; dst[base + 512] = lo;
                        }
            }
        }
        if (s.cin == 3)
            for (int co = 0; co < 64; ++co) if (cur[co] < 0.f) R.stem_negmask |= 1ull << co;      // sign of the stem BatchNorm's gamma
        cv.g_off = hf.size(); hf.insert(hf.end(), cur, cur + s.cout); cur += s.cout;
        cv.b_off = hf.size(); hf.insert(hf.end(), cur, cur + s.cout); cur += s.cout;
        cv.ss_off = ss_total; ss_total += 2 * (size_t)s.cout;
        R.convs.push_back(cv);
    }
    if (precision == BUSCA_PREC_F16) {
        // stem: fragment-ordered weights [4][7][64][8] from the [64][7][8][4] layout, and the byte -> normalised fp16 table
        const ReidConv& c0 = R.convs[0];
        R.stem_wpk_off = hpk.size();
        for (int ct = 0; ct < 4; ++ct)
            for (int kh = 0; kh < 7; ++kh)
                for (int ln = 0; ln < 64; ++ln)
                    for (int e = 0; e < 8; ++e) {
                        const int a = ln & 15, b = ln >> 4;
                        hpk.push_back((_Float16)hw[c0.w_off + ((size_t)((16 * ct + a) * 7 + kh) * 8 + 2 * b) * 4 + e]);
                    }
        R.stem_lut_off = hpk.size();
        const double mean[3] = {0.406, 0.456, 0.485}, stdv[3] = {0.225, 0.224, 0.299};   // BGR, network.py:470-476
        for (int ch = 0; ch < 3; ++ch)
            for (int v = 0; v < 256; ++v) {
                float x = (float)v / 255.0f;
                x = (float)((double)x - mean[ch]);
                hpk.push_back((_Float16)(float)((double)x / stdv[ch]));
            }
    }
    R.red_w_off = hf.size();
    hf.resize(hf.size() + (size_t)2048 * 512);
    for (int o = 0; o < 512; ++o)
        for (int k = 0; k < 2048; ++k) hf[R.red_w_off + (size_t)k * 512 + o] = cur[(size_t)o * 2048 + k];
    cur += (size_t)512 * 2048;
    R.red_b_off = hf.size(); hf.insert(hf.end(), cur, cur + 512);
    if (precision == BUSCA_PREC_F16) {
        std::vector<_Float16> h16(hw.size());
        for (size_t i = 0; i < hw.size(); ++i) h16[i] = (_Float16)hw[i];
        HIP_TRY(c, hipMalloc(&R.d_w, h16.size() * sizeof(_Float16)));
        HIP_TRY(c, hipMemcpy(R.d_w, h16.data(), h16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    } else {
        HIP_TRY(c, hipMalloc(&R.d_w, hw.size() * sizeof(float)));
        HIP_TRY(c, hipMemcpy(R.d_w, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (!hpk.empty()) {
        HIP_TRY(c, hipMalloc((void**)&R.d_wpk, hpk.size() * sizeof(_Float16)));
        HIP_TRY(c, hipMemcpy(R.d_wpk, hpk.data(), hpk.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    }
    if (!hkw.empty()) {
        HIP_TRY(c, hipMalloc((void**)&R.d_wkw, hkw.size() * sizeof(_Float16)));
        HIP_TRY(c, hipMemcpy(R.d_wkw, hkw.data(), hkw.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    }
    if (!hx3.empty()) {
        HIP_TRY(c, hipMalloc((void**)&R.d_wx3, hx3.size() * sizeof(_Float16)));
        HIP_TRY(c, hipMemcpy(R.d_wx3, hx3.data(), hx3.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        // the stem's byte table: exactly reid_preprocess_f32_kernel's arithmetic per (channel, byte), x 2^6, clamped, split as x3_split2 splits
        std::vector<unsigned> lut(768);
        const double mean[3] = {0.406, 0.456, 0.485}, stdv[3] = {0.225, 0.224, 0.299};   // BGR, network.py:470-476
        for (int ch = 0; ch < 3; ++ch)
            for (int v = 0; v < 256; ++v) {
                float x = (float)v / 255.0f;
                x = (float)((double)x - mean[ch]);
                x = (float)((double)x / stdv[ch]);
                float t = x * X3_XS;
                t = t < -X3_XMAX ? -X3_XMAX : (t > X3_XMAX ? X3_XMAX : t);
                const _Float16 hi = (_Float16)t, lo = (_Float16)(t - (float)hi);
                unsigned short hb, lb; memcpy(&hb, &hi, 2); memcpy(&lb, &lo, 2);
                lut[ch * 256 + v] = (unsigned)hb | ((unsigned)lb << 16);
            }
        HIP_TRY(c, hipMalloc((void**)&R.d_x3_lut, 768 * 4));
        HIP_TRY(c, hipMemcpy(R.d_x3_lut, lut.data(), 768 * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(c, hipMalloc((void**)&R.d_f, hf.size() * sizeof(float)));
    HIP_TRY(c, hipMalloc((void**)&R.d_ss, ss_total * sizeof(float)));
    HIP_TRY(c, hipMalloc(&R.d_zero, 256));
    HIP_TRY(c, hipMemset(R.d_zero, 0, 256));
    if (ss_total != (size_t)2 * 26560) return fail(c, BUSCA_EINVAL, "internal: BN channel count %zu", ss_total / 2);
    {   // the BatchNorm map of the running-statistics kernels (reid_bn.hip.inc): channels, affine parameters, output pixels per crop of every conv in forward order
        if ((int)R.convs.size() != REID_NCONV) return fail(c, BUSCA_EINVAL, "internal: %zu convs", R.convs.size());
        int H = 96, W = 32, i = 1;
        const int nblk[4] = {3, 4, 6, 3};
        R.bn_counts.count[0] = 192.0 * 64.0;
        for (int li = 0; li < 4; ++li)
            for (int b = 0; b < nblk[li]; ++b) {
                const int st = R.convs[i + 1].stride, H2 = (H - 1) / st + 1, W2 = (W - 1) / st + 1;
                R.bn_counts.count[i++] = (double)(H * W);
                R.bn_counts.count[i++] = (double)(H2 * W2);
                R.bn_counts.count[i++] = (double)(H2 * W2);
                if (b == 0) R.bn_counts.count[i++] = (double)(H2 * W2);
                H = H2; W = W2;
            }
        for (int k = 0; k < REID_NCONV; ++k) {
            R.bn_map.first[k] = (int)(R.convs[k].ss_off / 2); R.bn_map.g_off[k] = (int)R.convs[k].g_off; R.bn_map.b_off[k] = (int)R.convs[k].b_off;
        }
        R.bn_map.first[REID_NCONV] = REID_BN_CHANNELS;
    }
    HIP_TRY(c, hipMemcpy(R.d_f, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice));
    R.loaded = true;
    return BUSCA_OK;
}
