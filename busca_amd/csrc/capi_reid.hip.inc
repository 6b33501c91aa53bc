// C-ABI entry points of the ReID extractor's forward side (weights: reid_weights.hip.inc; the schedule behind them: reid_schedule.hip.inc).

extern "C" size_t busca_reid_workspace_bytes(int32_t n) { return reid_ws::bytes(n, 2); }   // fp16 flavour; f32 needs 2x the activation part

// Stand-alone entry (unit tests, include/busca_hip.h): scratch is allocated per call, and the pass holds nothing but it.
extern "C" int busca_bn_stats_1x1(busca_ctx* c, const void* x, const float* in_ss, int32_t n, int32_t H, int32_t W, int32_t Cin, int32_t stride,
                                  const void* w, int32_t Cout, const float* gamma, const float* beta, float* ss_out, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (!x || !w || !gamma || !beta || !ss_out || n < 1 || H < 1 || W < 1 || stride < 1) return fail(c, BUSCA_EINVAL, "busca_bn_stats_1x1: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    ReidPass P;
    P.s = (hipStream_t)stream; P.n = n;
    HIP_TRY(c, hipMalloc((void**)&P.gpart, reid_ws::GRAM_PART_FLOATS * 4));
    if (hipMalloc((void**)&P.gG, reid_ws::GRAM_G_DOUBLES * 8) != hipSuccess) { hipFree(P.gpart); return fail(c, BUSCA_ENOMEM, "busca_bn_stats_1x1: scratch"); }
    const int rc = gram_stats_launch(c, P, {(const _Float16*)x, in_ss, H, W, Cin, stride, (const _Float16*)w, Cout, gamma, beta, ss_out, nullptr});
    hipStreamSynchronize(P.s);
    hipFree(P.gpart); hipFree(P.gG);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    return BUSCA_OK;
}

extern "C" int busca_reid_forward_w(busca_ctx* c, const uint8_t* crops, int32_t n, const uint8_t* zero_norm, const float* weights, double weight_sum,
                                    float* feats, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (!c->reid->loaded) return fail(c, BUSCA_ENOWEIGHTS, "busca_reid_forward before busca_reid_load_weights");
    if (weights != nullptr && !(weight_sum >= 1.0)) return fail(c, BUSCA_EINVAL, "busca_reid_forward_w: weight_sum must be the (>= 1) sum of the multiplicities");
    switch (c->reid->prec) {
        case BUSCA_PREC_F16: return reid_forward_impl<ReidF16>(c, crops, zero_norm, n, weights, weight_sum, feats, stream);
        case BUSCA_PREC_F16X3: return reid_forward_impl<ReidX3>(c, crops, zero_norm, n, weights, weight_sum, feats, stream);
        default: return reid_forward_impl<ReidF32>(c, crops, zero_norm, n, weights, weight_sum, feats, stream);
    }
}

extern "C" int busca_reid_forward_ex(busca_ctx* c, const uint8_t* crops, int32_t n, const uint8_t* zero_norm, float* feats, void* stream) {
    return busca_reid_forward_w(c, crops, n, zero_norm, nullptr, 0.0, feats, stream);
}

extern "C" int busca_reid_forward(busca_ctx* c, const uint8_t* crops, int32_t n, float* feats, void* stream) {
    return busca_reid_forward_ex(c, crops, n, nullptr, feats, stream);
}

extern "C" int busca_reid_reserve(busca_ctx* c, int32_t n, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (!c->reid->loaded) return fail(c, BUSCA_ENOWEIGHTS, "busca_reid_reserve before busca_reid_load_weights");
    if (n < 1) return fail(c, BUSCA_EINVAL, "busca_reid_reserve: n = %d", n);
    HIP_TRY(c, hipSetDevice(c->device));
    ReidState::WS* w = nullptr;
    return reid_ws_acquire(c, n, stream, c->reid->prec != BUSCA_PREC_F16 ? 4 : 2, &w);
}
