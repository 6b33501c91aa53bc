// C-ABI entry points of the running-statistics BatchNorm (include/busca_reid_bn.h; kernels: reid_bn.hip.inc, the pass: reid_schedule.hip.inc).

extern "C" size_t busca_reid_running_floats(void) { return (size_t)2 * REID_BN_CHANNELS; }

extern "C" int busca_reid_load_running_stats(busca_ctx* c, const float* stats, size_t floats) {
    if (!c) return BUSCA_EINVAL;
    ReidState& R = *c->reid;
    if (!R.loaded) return fail(c, BUSCA_ENOWEIGHTS, "busca_reid_load_running_stats before busca_reid_load_weights");
    if (!stats || floats != busca_reid_running_floats()) return fail(c, BUSCA_EINVAL, "ReID running statistics have %zu floats, expected %zu", floats, busca_reid_running_floats());
    for (int i = 0; i < REID_NCONV; ++i) {
        const int c0 = R.bn_map.first[i], C = R.bn_map.first[i + 1] - c0;
        for (int j = 0; j < C; ++j) {
            const float mean = stats[2 * c0 + j], var = stats[2 * c0 + C + j];
            if (!std::isfinite(mean) || !std::isfinite(var)) return fail(c, BUSCA_EINVAL, "ReID running statistics: conv %d channel %d is not finite", i, j);
            if (!(var + 1e-5f > 0.f)) return fail(c, BUSCA_EINVAL, "ReID running statistics: conv %d channel %d has var + eps = %g <= 0", i, j, (double)(var + 1e-5f));
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());                 // no forward in flight reads the table that is about to change
    if (!R.d_run) HIP_TRY(c, hipMalloc((void**)&R.d_run, floats * sizeof(float)));
    if (!R.d_rss) HIP_TRY(c, hipMalloc((void**)&R.d_rss, floats * sizeof(float)));
    HIP_TRY(c, hipMemcpy(R.d_run, stats, floats * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(reid_bn_table_kernel, dim3((REID_BN_CHANNELS + 255) / 256), dim3(256), 0, (hipStream_t)nullptr, (const float*)R.d_run, (const float*)R.d_f, R.bn_map, R.d_rss);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipDeviceSynchronize());
    R.run_loaded = true;
    return BUSCA_OK;
}

extern "C" int busca_reid_reset_running_stats(busca_ctx* c) {
    if (!c) return BUSCA_EINVAL;
    if (!c->reid->loaded) return fail(c, BUSCA_ENOWEIGHTS, "busca_reid_reset_running_stats before busca_reid_load_weights");
    const ReidBnMap& m = c->reid->bn_map;
    std::vector<float> h(busca_reid_running_floats(), 0.f);
    for (int i = 0; i < REID_NCONV; ++i) {
        const int c0 = m.first[i], C = m.first[i + 1] - c0;
        for (int j = 0; j < C; ++j) h[2 * c0 + C + j] = 1.f;
    }
    return busca_reid_load_running_stats(c, h.data(), h.size());
}

extern "C" int busca_reid_get_running_stats(busca_ctx* c, float* host_out, size_t floats, void* stream) {
    if (!c) return BUSCA_EINVAL;
    const ReidState& R = *c->reid;
    if (!R.loaded) return fail(c, BUSCA_ENOWEIGHTS, "busca_reid_get_running_stats before busca_reid_load_weights");
    if (!R.run_loaded) return fail(c, BUSCA_EINVAL, "busca_reid_get_running_stats: no running statistics are loaded");
    if (!host_out || floats != busca_reid_running_floats()) return fail(c, BUSCA_EINVAL, "busca_reid_get_running_stats: %zu floats, expected %zu", floats, busca_reid_running_floats());
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(host_out, R.d_run, floats * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(c, hipStreamSynchronize((hipStream_t)stream));
    return BUSCA_OK;
}

static int reid_bn_forward(busca_ctx* c, const uint8_t* crops, int32_t n, const uint8_t* zero_norm, float* feats, void* stream, const ReidBnMode& bn) {
    switch (c->reid->prec) {
        case BUSCA_PREC_F16: return reid_forward_impl<ReidF16>(c, crops, zero_norm, n, nullptr, 0.0, feats, stream, bn);
        case BUSCA_PREC_F16X3: return reid_forward_impl<ReidX3>(c, crops, zero_norm, n, nullptr, 0.0, feats, stream, bn);
        default: return reid_forward_impl<ReidF32>(c, crops, zero_norm, n, nullptr, 0.0, feats, stream, bn);
    }
}

extern "C" int busca_reid_forward_running(busca_ctx* c, const uint8_t* crops, int32_t n, const uint8_t* zero_norm, int32_t output, float* feats, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (!c->reid->loaded) return fail(c, BUSCA_ENOWEIGHTS, "busca_reid_forward_running before busca_reid_load_weights");
    if (!c->reid->run_loaded) return fail(c, BUSCA_EINVAL, "busca_reid_forward_running: no running statistics are loaded (busca_reid_load_running_stats / _reset_running_stats)");
    if (output != BUSCA_REID_OUT_PLAIN && output != BUSCA_REID_OUT_NORM) return fail(c, BUSCA_EINVAL, "busca_reid_forward_running: output %d", output);
    ReidBnMode bn; bn.running = true; bn.output = output;
    return reid_bn_forward(c, crops, n, zero_norm, feats, stream, bn);
}

extern "C" int busca_reid_adapt(busca_ctx* c, const uint8_t* crops, int32_t n, const uint8_t* zero_norm, double momentum, int32_t output, float* feats, void* stream) {
    if (!c) return BUSCA_EINVAL;
    if (!c->reid->loaded) return fail(c, BUSCA_ENOWEIGHTS, "busca_reid_adapt before busca_reid_load_weights");
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(c, BUSCA_EINVAL, "busca_reid_adapt: momentum %g outside [0, 1]", momentum);
    if (momentum != 0.0 && !c->reid->run_loaded) return fail(c, BUSCA_EINVAL, "busca_reid_adapt: no running statistics to update (busca_reid_load_running_stats / _reset_running_stats)");
    if (output != BUSCA_REID_OUT_PLAIN && output != BUSCA_REID_OUT_NORM) return fail(c, BUSCA_EINVAL, "busca_reid_adapt: output %d", output);
    ReidBnMode bn; bn.output = output; bn.momentum = momentum;
    return reid_bn_forward(c, crops, n, zero_norm, feats, stream, bn);
}
