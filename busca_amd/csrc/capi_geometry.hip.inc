// C-ABI entry points for the geometry / crop kernels.

extern "C" int busca_pairwise(busca_ctx* c, const double* a, int32_t nA, const double* b, int32_t nB, int32_t mode,
                              const double* scores_b, double* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (nA < 0 || nB < 0 || mode < BUSCA_PAIR_CENTER || mode > BUSCA_PAIR_IOU_COST) return fail(c, BUSCA_EINVAL, "bad pairwise arguments");
    if (nA == 0 || nB == 0) return BUSCA_OK;
    if (!a || !b || !out) return fail(c, BUSCA_EINVAL, "null pointer");
    dim3 grid((nB + PW_TB - 1) / PW_TB, (nA + PW_TA - 1) / PW_TA);
    TimedLaunch tl(c, (hipStream_t)stream);
    hipLaunchKernelGGL(pairwise_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, nA, b, nB, mode,
                       mode == BUSCA_PAIR_IOU_COST ? scores_b : nullptr, out);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_topk_rows(busca_ctx* c, const double* dist, int32_t B, int32_t N, int32_t P, int32_t* idx, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (B < 0 || N < 0 || P < 1) return fail(c, BUSCA_EINVAL, "bad top-k arguments");
    if (B == 0) return BUSCA_OK;
    if (!idx || (N > 0 && !dist)) return fail(c, BUSCA_EINVAL, "null pointer");
    TimedLaunch tl(c, (hipStream_t)stream);
    hipStream_t s = (hipStream_t)stream;
    if (N <= 256) hipLaunchKernelGGL((topk_rank_kernel<1>), dim3(B), dim3(256), 0, s, dist, N, P, idx);             // tracker sizes: one workgroup per row, ranks from one LDS pass
    else if (N <= 512) hipLaunchKernelGGL((topk_rank_kernel<2>), dim3(B), dim3(256), 0, s, dist, N, P, idx);
    // longer rows: P selection rounds (the rank kernel's N^2 / 256 compares per thread lose beyond ~500 columns: 300 x 1000, P = 16 measured 135 us against 78)
    else hipLaunchKernelGGL(topk_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, s, dist, B, N, P, idx);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

static int crop_scratch(busca_ctx* c, hipStream_t s, int n) {     // per-crop pad value + integer extents
    if (c->crop_fill_cap < n) {
        if (c->crop_fill) { HIP_TRY(c, hipStreamSynchronize(s)); HIP_TRY(c, hipFree(c->crop_fill)); c->crop_fill = nullptr; }
        const int cap = n < 256 ? 256 : n * 2;
        HIP_TRY(c, hipMalloc((void**)&c->crop_fill, (size_t)cap * 8 * sizeof(int)));      // [cap] pad values, [cap][4] extents, [cap] 64-bit destinations
        c->crop_fill_cap = cap;
    }
    return BUSCA_OK;
}

static int crop_launch(busca_ctx* c, hipStream_t s, const uint8_t* frame, int H, int W, int stride, const int* rects, int n,
                       uint8_t* out_u8, const unsigned long long* dst, void* out_f16) {
    // rects / dst may be pinned host tables: the first kernel copies them next to its pad values, the second reads the copies
    int* rects_dev = c->crop_fill + c->crop_fill_cap;
    unsigned long long* dst_dev = (unsigned long long*)(c->crop_fill + 6 * (size_t)c->crop_fill_cap);
    TimedLaunch tl(c, s);                   // one bracket around the pair (bench.py hbm_kernels)
    hipLaunchKernelGGL(crop_fill_kernel, dim3(n), dim3(256), 0, s, frame, H, W, stride, rects, n, c->crop_fill, dst, rects_dev, dst_dev);
    // u8 outputs (pool slots / packed batch): the LDS-staged band kernel; the fp16 ReID-input side output keeps the one-thread-per-pixel kernel
    if (out_f16 == nullptr && c->opt.crop_band != 0)
        hipLaunchKernelGGL(crop_band_kernel, dim3(CROP_H / CROP_RB, n), dim3(256), 0, s, frame, H, W, stride, (const int*)rects_dev,
                           (const int*)c->crop_fill, out_u8, dst != nullptr ? (const unsigned long long*)dst_dev : nullptr);
    else
    hipLaunchKernelGGL(crop_resize_kernel, dim3(CROP_H * CROP_W / 256, n), dim3(256), 0, s, frame, H, W, stride, (const int*)rects_dev,
                       (const int*)c->crop_fill, out_u8, dst != nullptr ? (const unsigned long long*)dst_dev : nullptr, (_Float16*)out_f16);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_crop_gather(busca_ctx* c, const uint8_t* frame, int32_t H, int32_t W, int32_t stride,
                                 const float* boxes, int32_t n, uint8_t* out_u8, void* out_f16, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (H <= 0 || W <= 0 || stride < 3 * W || n < 0) return fail(c, BUSCA_EINVAL, "bad frame geometry");
    if (n == 0) return BUSCA_OK;
    if (!frame || !boxes || (!out_u8 && !out_f16)) return fail(c, BUSCA_EINVAL, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    { int rc = crop_scratch(c, s, n); if (rc) return rc; }
    int* rects = c->crop_fill + c->crop_fill_cap;
    hipLaunchKernelGGL(crop_rects_kernel, dim3((n + 255) / 256), dim3(256), 0, s, boxes, n, rects);
    return crop_launch(c, s, frame, H, W, stride, rects, n, out_u8, nullptr, out_f16);
}

extern "C" int busca_crop_gather_ex(busca_ctx* c, const uint8_t* frame, int32_t H, int32_t W, int32_t stride, const int32_t* rects,
                                    int32_t n, const uint64_t* dst_u8, uint8_t* out_u8, void* out_f16, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (H <= 0 || W <= 0 || stride < 3 * W || n < 0) return fail(c, BUSCA_EINVAL, "bad frame geometry");
    if (n == 0) return BUSCA_OK;
    if (!frame || !rects || (!out_u8 && !out_f16 && !dst_u8)) return fail(c, BUSCA_EINVAL, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    { int rc = crop_scratch(c, s, n); if (rc) return rc; }
    return crop_launch(c, s, frame, H, W, stride, (const int*)rects, n, out_u8, (const unsigned long long*)dst_u8, out_f16);
}

extern "C" int busca_crop_gather_sized(busca_ctx* c, const uint8_t* frame, int32_t H, int32_t W, int32_t stride, const int32_t* rects,
                                       int32_t n, int32_t out_h, int32_t out_w, uint8_t* out_u8, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (H <= 0 || W <= 0 || stride < 3 * W || n < 0 || out_h < 1 || out_w < 1 || (long)out_h * out_w > (1l << 26)) return fail(c, BUSCA_EINVAL, "bad frame / output geometry");
    if (n == 0) return BUSCA_OK;
    if (!frame || !rects || !out_u8) return fail(c, BUSCA_EINVAL, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    { int rc = crop_scratch(c, s, n); if (rc) return rc; }
    int* rects_dev = c->crop_fill + c->crop_fill_cap;
    unsigned long long* dst_dev = (unsigned long long*)(c->crop_fill + 6 * (size_t)c->crop_fill_cap);
    hipLaunchKernelGGL(crop_fill_kernel, dim3(n), dim3(256), 0, s, frame, H, W, stride, (const int*)rects, n, c->crop_fill, (const unsigned long long*)nullptr, rects_dev, dst_dev);
    hipLaunchKernelGGL(crop_resize_any_kernel, dim3((unsigned)((out_h * out_w + 255) / 256), n), dim3(256), 0, s, frame, H, W, stride, (const int*)rects_dev,
                       (const int*)c->crop_fill, out_u8, out_h, out_w);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_gather_crops(busca_ctx* c, const uint64_t* src, int32_t n, uint8_t* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0) return fail(c, BUSCA_EINVAL, "busca_gather_crops: negative count");
    if (n == 0) return BUSCA_OK;
    if (!src || !out) return fail(c, BUSCA_EINVAL, "busca_gather_crops: null pointer");
    TimedLaunch tl(c, (hipStream_t)stream);
    hipLaunchKernelGGL(crop_ptr_gather_kernel, dim3(CROP_BYTES / 16384, n), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)src, out);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}


extern "C" int busca_coverage(busca_ctx* c, const int32_t* rects, int32_t n, int32_t H, int32_t W, uint64_t* count, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || H <= 0 || W <= 0 || !count) return fail(c, BUSCA_EINVAL, "bad coverage arguments");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(c, hipMemsetAsync(count, 0, sizeof(uint64_t), s));
    if (n == 0) return BUSCA_OK;
    if (!rects) return fail(c, BUSCA_EINVAL, "null pointer");
    const long npix = (long)H * W;
    hipLaunchKernelGGL(coverage_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, (const int*)rects, n, H, W, (unsigned long long*)count);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_kalman_multi_predict(busca_ctx* c, double* mean, double* cov, const uint8_t* not_tracked, int32_t n, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || (n > 0 && (!mean || !cov))) return fail(c, BUSCA_EINVAL, "busca_kalman_multi_predict: bad argument");
    if (n == 0) return BUSCA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kalman_predict_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, mean, cov, not_tracked, n);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_kalman_update(busca_ctx* c, double* mean, double* cov, const double* meas, int32_t n, int32_t* status, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || (n > 0 && (!mean || !cov || !meas))) return fail(c, BUSCA_EINVAL, "busca_kalman_update: bad argument");
    if (n == 0) return BUSCA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kalman_update_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, mean, cov, meas, n, (int*)status);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_kalman_initiate(busca_ctx* c, const double* meas, int32_t n, double* mean, double* cov, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || (n > 0 && (!meas || !mean || !cov))) return fail(c, BUSCA_EINVAL, "busca_kalman_initiate: bad argument");
    if (n == 0) return BUSCA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kalman_initiate_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, meas, n, mean, cov);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_kalman_boxes(busca_ctx* c, const double* mean, int32_t n, int32_t tlbr, double* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || (tlbr != 0 && tlbr != 1) || (n > 0 && (!mean || !out))) return fail(c, BUSCA_EINVAL, "busca_kalman_boxes: bad argument");
    if (n == 0) return BUSCA_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kalman_boxes_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, mean, n, tlbr, out);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_kalman_gating(busca_ctx* c, const double* mean, const double* cov, int32_t n, const double* meas, int32_t m,
                                   int32_t only_position, int32_t metric, double* out, int32_t* status, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (n < 0 || m < 0 || (only_position != 0 && only_position != 1) || (metric != 0 && metric != 1))
        return fail(c, BUSCA_EINVAL, "busca_kalman_gating: bad argument");
    if (n == 0 || m == 0) return BUSCA_OK;
    if (!mean || !cov || !meas || !out) return fail(c, BUSCA_EINVAL, "busca_kalman_gating: null pointer");
    const int tiles = (m + KALMAN_GATE_TILE - 1) / KALMAN_GATE_TILE;
    if (tiles > 65535) return fail(c, BUSCA_EINVAL, "busca_kalman_gating: more than %d measurements", 65535 * KALMAN_GATE_TILE);
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kalman_gating_kernel, dim3(n, tiles), dim3(64), 0, (hipStream_t)stream, mean, cov, n, meas, m, only_position, metric, out,
                       (int*)status);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_duplicate_masks(busca_ctx* c, const double* cost, int32_t nA, int32_t nB, const int32_t* ageA, const int32_t* ageB,
                                     double thresh, uint8_t* keepA, uint8_t* keepB, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (nA < 0 || nB < 0) return fail(c, BUSCA_EINVAL, "busca_duplicate_masks: negative size");
    if ((nA > 0 && (!keepA || !ageA)) || (nB > 0 && (!keepB || !ageB)) || (nA > 0 && nB > 0 && !cost)) return fail(c, BUSCA_EINVAL, "busca_duplicate_masks: null pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (nA > 0) HIP_TRY(c, hipMemsetAsync(keepA, 1, nA, s));
    if (nB > 0) HIP_TRY(c, hipMemsetAsync(keepB, 1, nB, s));
    const long tot = (long)nA * nB;
    if (tot > 0) hipLaunchKernelGGL(duplicate_mark_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, cost, nA, nB, ageA, ageB, thresh, keepA, keepB);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

// ---- camera-motion compensation --------------------------------------------------------------------------------------
// Inverse of a small symmetric-positive matrix in double (Gauss-Jordan with partial pivoting), rounded to float like the
// CV_32F `hessian.inv()` of ecc.cpp.  Returns false when singular.
static bool ecc_invert(const double* a, int n, float* out) {
    double m[6][12];
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { m[i][j] = a[i * n + j]; m[i][n + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r) if (fabs(m[r][c]) > fabs(m[piv][c])) piv = r;
        if (fabs(m[piv][c]) < 1e-300) return false;
        if (piv != c) for (int j = 0; j < 2 * n; ++j) std::swap(m[c][j], m[piv][j]);
        const double d = 1.0 / m[c][c];
        for (int j = 0; j < 2 * n; ++j) m[c][j] *= d;
        for (int r = 0; r < n; ++r) if (r != c) { const double f = m[r][c]; if (f != 0.0) for (int j = 0; j < 2 * n; ++j) m[r][j] -= f * m[c][j]; }
    }
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) out[i * n + j] = (float)m[i][n + j];
    return true;
}

// The workspace of the ECC calls: 5 float images (template, input, gx, gy, one temporary) + the partial sums.  Growth waits for `s` (work
// queued on it may still read the old block), frees and allocates.
static int ecc_ws_reserve(busca_ctx* c, const char* who, size_t need, hipStream_t s) {
    if (c->ecc_ws_bytes < need) {
        if (c->ecc_ws) { HIP_TRY(c, hipStreamSynchronize(s)); HIP_TRY(c, hipFree(c->ecc_ws)); c->ecc_ws = nullptr; c->ecc_ws_bytes = 0; }
        if (hipMalloc(&c->ecc_ws, need) != hipSuccess) return fail(c, BUSCA_ENOMEM, "%s: cannot allocate %zu bytes", who, need);
        c->ecc_ws_bytes = need;
    }
    return BUSCA_OK;
}
static size_t ecc_img_bytes(int H, int W) { return ((size_t)H * W * 4 + 255) & ~(size_t)255; }
static size_t ecc_ws_need(int H, int W) { return 5 * ecc_img_bytes(H, W) + (size_t)(ECC_MAX_BLOCKS + 1) * ECC_NS(6) * 8; }

// The iterations of cv2.findTransformECC on a blurred template T, a blurred image I and its gradients: one ecc_iter_kernel<P> pass + the P x P
// solve on the host per iteration (P = 2 translation, 3 Euclidean, 6 affine).  `who` names the entry point in the messages.
static int ecc_iterate(busca_ctx* c, const char* who, const float* T, const float* I, const float* gx, const float* gy, int H, int W, int P, double* partials,
                       int max_iters, double eps, float* warp, double* cc, int32_t* iters_out, hipStream_t s) {
    const size_t npix = (size_t)H * W;
    const int NS = ECC_NS(P);
    double* sums_d = partials + (size_t)ECC_MAX_BLOCKS * ECC_NS(6);
    const int nblocks = (int)std::min<size_t>(ECC_MAX_BLOCKS, (npix + 1023) / 1024);
    float M[6];
    for (int i = 0; i < 6; ++i) M[i] = warp[i];
    double rho = -1.0, last_rho = -eps;
    int it = 1;
    for (; it <= max_iters && fabs(rho - last_rho) >= eps; ++it) {
        EccIterArgs a{};
        a.T = T; a.I = I; a.gx = gx; a.gy = gy; a.H = H; a.W = W; a.partials = partials;
        for (int i = 0; i < 6; ++i) a.m[i] = (double)M[i];
        a.h0 = M[0]; a.h1 = M[3];
        if (P == 2) hipLaunchKernelGGL((ecc_iter_kernel<2>), dim3(nblocks), dim3(256), 0, s, a);
        else if (P == 3) hipLaunchKernelGGL((ecc_iter_kernel<3>), dim3(nblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((ecc_iter_kernel<6>), dim3(nblocks), dim3(256), 0, s, a);
        hipLaunchKernelGGL(ecc_reduce_kernel, dim3(1), dim3(64), 0, s, (const double*)partials, nblocks, NS, sums_d);
        double S[ECC_NS(6)];
        HIP_TRY(c, hipMemcpyAsync(S, sums_d, NS * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        const double n = S[0];
        if (n < 1.0) return fail(c, BUSCA_EINVAL, "%s: the warped image does not overlap the template", who);
        const double mI = S[1] / n, mT = S[2] / n;
        const double img2 = S[3] - n * mI * mI, tmp2 = S[4] - n * mT * mT;      // n * variance
        const double corr = S[5] - n * mI * mT;
        double hess[36]; float hinv[36], ip[6], tp[6], iph[6];
        int k = 6 + 3 * P;
        for (int i = 0; i < P; ++i)
            for (int j = i; j < P; ++j) { const float v = (float)S[k++]; hess[i * P + j] = v; hess[j * P + i] = v; }   // CV_32F hessian
        if (!ecc_invert(hess, P, hinv)) return fail(c, BUSCA_EINVAL, "%s: singular Hessian", who);
        for (int i = 0; i < P; ++i) { ip[i] = (float)(S[6 + P + i] - mI * S[6 + i]); tp[i] = (float)(S[6 + 2 * P + i] - mT * S[6 + i]); }
        last_rho = rho;
        rho = corr / (sqrt(img2) * sqrt(tmp2));
        if (rho != rho) return fail(c, BUSCA_EINVAL, "%s: NaN encountered", who);
        for (int i = 0; i < P; ++i) { float v = 0.f; for (int j = 0; j < P; ++j) v += hinv[i * P + j] * ip[j]; iph[i] = v; }
        double ipd = 0.0, tpd = 0.0;
        for (int i = 0; i < P; ++i) { ipd += (double)ip[i] * (double)iph[i]; tpd += (double)tp[i] * (double)iph[i]; }
        const double lam_n = img2 - ipd, lam_d = corr - tpd;
        if (lam_d <= 0.0) return fail(c, BUSCA_EINVAL, "%s: the algorithm stopped before its convergence (correlation is going to be minimized)", who);
        const double lam = lam_n / lam_d;
        float ep[6], dp[6];
        for (int i = 0; i < P; ++i)       // J^T (lambda Tzm - Izm), by linearity from the unrounded sums
            ep[i] = (float)(lam * (S[6 + 2 * P + i] - mT * S[6 + i]) - (S[6 + P + i] - mI * S[6 + i]));
        for (int i = 0; i < P; ++i) { float v = 0.f; for (int j = 0; j < P; ++j) v += hinv[i * P + j] * ep[j]; dp[i] = v; }
        if (P == 2) {
            M[2] += dp[0]; M[5] += dp[1];
        } else if (P == 3) {
            const float th = asinf(M[3]) + dp[0];
            M[2] += dp[1]; M[5] += dp[2];
            M[0] = M[4] = cosf(th); M[3] = sinf(th); M[1] = -M[3];
        } else {
            M[0] += dp[0]; M[3] += dp[1]; M[1] += dp[2]; M[4] += dp[3]; M[2] += dp[4]; M[5] += dp[5];
        }
    }
    for (int i = 0; i < 6; ++i) warp[i] = M[i];
    if (cc) *cc = rho;
    if (iters_out) *iters_out = it - 1;
    return BUSCA_OK;
}

extern "C" int busca_ecc_align(busca_ctx* c, const uint8_t* prev, const uint8_t* cur, int32_t H, int32_t W, int32_t stride_prev,
                               int32_t stride_cur, int32_t motion, int32_t max_iters, double eps, float* warp, double* cc, int32_t* iters_out,
                               void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (!prev || !cur || !warp || H < 8 || W < 8 || stride_prev < 3 * W || stride_cur < 3 * W || max_iters < 1 || (motion != 0 && motion != 1))
        return fail(c, BUSCA_EINVAL, "busca_ecc_align: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t img = ecc_img_bytes(H, W);
    if (int rc = ecc_ws_reserve(c, "busca_ecc_align", ecc_ws_need(H, W), s)) return rc;
    char* base = (char*)c->ecc_ws;
    float *T = (float*)base, *I = (float*)(base + img), *gx = (float*)(base + 2 * img), *gy = (float*)(base + 3 * img), *tmp = (float*)(base + 4 * img);
    double* partials = (double*)(base + 5 * img);
    const dim3 g2((W + 255) / 256, H), b2(256);
    hipLaunchKernelGGL(ecc_gray_kernel, g2, b2, 0, s, prev, H, W, stride_prev, tmp);
    hipLaunchKernelGGL(ecc_blur_h_kernel, g2, b2, 0, s, (const float*)tmp, H, W, gx);
    hipLaunchKernelGGL(ecc_blur_v_kernel, g2, b2, 0, s, (const float*)gx, H, W, T);
    hipLaunchKernelGGL(ecc_gray_kernel, g2, b2, 0, s, cur, H, W, stride_cur, tmp);
    hipLaunchKernelGGL(ecc_blur_h_kernel, g2, b2, 0, s, (const float*)tmp, H, W, gx);
    hipLaunchKernelGGL(ecc_blur_v_kernel, g2, b2, 0, s, (const float*)gx, H, W, I);
    hipLaunchKernelGGL(ecc_grad_kernel, g2, b2, 0, s, (const float*)I, H, W, gx, gy);
    HIP_TRY(c, hipGetLastError());
    return ecc_iterate(c, "busca_ecc_align", T, I, gx, gy, H, W, motion == 0 ? 3 : 6, partials, max_iters, eps, warp, cc, iters_out, s);
}

// ---- GHOST's camera-motion estimate (include/busca_ecc.h) --------------------------------------------------------------------
static bool ecc_ksize_ok(int32_t k) { return k >= 1 && k <= ECC_KMAX && (k & 1); }

extern "C" int busca_ecc_gauss_taps(int32_t ksize, float* taps) {
    if (!taps || !ecc_ksize_ok(ksize)) return BUSCA_EINVAL;
    static const float small[4][7] = {{1.f}, {0.25f, 0.5f, 0.25f}, {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                      {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    if (ksize <= 7) {
        for (int i = 0; i < ksize; ++i) taps[i] = small[ksize >> 1][i];
        return BUSCA_OK;
    }
    const double sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8, scale2 = -0.5 / (sigma * sigma);
    double v[ECC_KMAX], sum = 0.0;
    for (int i = 0; i < ksize; ++i) { const double x = i - (ksize - 1) * 0.5; v[i] = exp(scale2 * x * x); sum += v[i]; }
    for (int i = 0; i < ksize; ++i) taps[i] = (float)(v[i] / sum);
    return BUSCA_OK;
}

extern "C" int busca_ecc_prepare(busca_ctx* c, const float* img, int32_t channels, int32_t H, int32_t W, int64_t stride_c, int64_t stride_row,
                                 int64_t stride_col, int32_t ksize, float* out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (!ecc_ksize_ok(ksize)) return fail(c, BUSCA_EINVAL, "busca_ecc_prepare: ksize %d is not an odd size in 1 .. %d", ksize, ECC_KMAX);
    const int lo = std::max(8, ksize / 2 + 1);
    if (H < lo || W < lo) return fail(c, BUSCA_EINVAL, "busca_ecc_prepare: a %d x %d frame is below %d x %d (ksize %d)", H, W, lo, lo, ksize);
    if (channels != 1 && channels != 3) return fail(c, BUSCA_EINVAL, "busca_ecc_prepare: %d channels (1 or 3)", channels);
    if (!img || !out) return fail(c, BUSCA_EINVAL, "busca_ecc_prepare: null pointer");
    if (stride_row < 0 || stride_col <= 0 || (channels == 3 && stride_c < 0)) return fail(c, BUSCA_EINVAL, "busca_ecc_prepare: bad stride");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ecc_ws_reserve(c, "busca_ecc_prepare", ecc_ws_need(H, W), s)) return rc;
    float* tmp = (float*)((char*)c->ecc_ws + 4 * ecc_img_bytes(H, W));
    EccTaps taps{};
    busca_ecc_gauss_taps(ksize, taps.k);
    const dim3 g2((W + ECC_TILE - 1) / ECC_TILE, H), b2(ECC_TILE);
    hipLaunchKernelGGL(ecc_prep_h_kernel, g2, b2, 0, s, img, channels, H, W, (long)stride_c, (long)stride_row, (long)stride_col, taps, ksize, tmp);
    hipLaunchKernelGGL(ecc_blur_vk_kernel, g2, b2, 0, s, (const float*)tmp, H, W, taps, ksize, out);
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_ecc_align_planes(busca_ctx* c, const float* templ, const float* input, int32_t H, int32_t W, int32_t motion, int32_t max_iters,
                                      double eps, float* warp, double* cc, int32_t* iters_out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (!templ || !input || !warp || H < 8 || W < 8 || max_iters < 1 || motion < 0 || motion > 2)
        return fail(c, BUSCA_EINVAL, "busca_ecc_align_planes: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t img = ecc_img_bytes(H, W);
    if (int rc = ecc_ws_reserve(c, "busca_ecc_align_planes", ecc_ws_need(H, W), s)) return rc;
    char* base = (char*)c->ecc_ws;
    float *gx = (float*)(base + 2 * img), *gy = (float*)(base + 3 * img);
    hipLaunchKernelGGL(ecc_grad_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, input, H, W, gx, gy);
    HIP_TRY(c, hipGetLastError());
    static const int P_OF[3] = {3, 6, 2};
    return ecc_iterate(c, "busca_ecc_align_planes", templ, input, gx, gy, H, W, P_OF[motion], (double*)(base + 5 * img), max_iters, eps, warp, cc, iters_out, s);
}
