/*
 * busca_reid_bn.h - running-statistics BatchNorm of the ReID extractor of libbusca_hip.so: what torch's BatchNorm2d does with `running_mean` /
 * `running_var` (eval-mode forward, train-mode update, reset_running_stats) for the ResNet-50 of busca_reid_* (busca_hip.h), as GHOST runs its
 * encoder (adapters/GHOST/src/base_tracker.py:76-77 and :296-349).  Same conventions as busca_hip.h (return codes, dev / host pointers, `stream`, one
 * ctx per GPU/process); the context and the error codes are the ones declared there.
 *
 * The statistics are 2 x 26 560 floats: per conv in the order of the weight blob (busca_reid_load_weights) running_mean[Cout], then running_var[Cout].
 * They belong to the loaded weights of the context, for any arithmetic flavour: a (re)load of the weights drops them.  Loading them builds ONE table
 * of (scale, shift) pairs, scale = gamma / sqrt(var + 1e-5) and shift = beta - mean * scale in float32, as torch's inference BatchNorm forms them;
 * busca_reid_forward_running is busca_reid_forward_ex reading that table where the batch-statistics pass reads the table it has just computed.  The
 * exact-f32 and fp16 flavours then launch nothing that only computes statistics; the split-fp16 flavour keeps those launches (they write to the pass's
 * own table, which nothing reads but the end-of-pass scan), so that "reid_status" 2 is raised exactly as in a batch-statistics pass.
 *
 * Calls that change the statistics (load, reset, adapt with momentum != 0) and forwards that read them are ordered by the caller: on one stream, or
 * synchronised.
 */
#ifndef BUSCA_REID_BN_H
#define BUSCA_REID_BN_H

#include "busca_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `output` of busca_reid_forward_running / busca_reid_adapt (resnet.py:314-322) */
#define BUSCA_REID_OUT_PLAIN 0 /* F.normalize(fc7): what busca_reid_forward returns */
#define BUSCA_REID_OUT_NORM 1  /* fc7 as it is */

/* 2 x 26 560 */
size_t busca_reid_running_floats(void);

/* Upload `stats` (host, `floats` == busca_reid_running_floats()) and build the (scale, shift) table.  Synchronous, like a weight load.
 * BUSCA_ENOWEIGHTS before busca_reid_load_weights*; BUSCA_EINVAL for a wrong size, a non-finite entry or a variance with var + 1e-5 <= 0 (the
 * statistics of the context are then unchanged). */
int busca_reid_load_running_stats(busca_ctx* ctx, const float* stats, size_t floats);

/* BatchNorm2d.reset_running_stats(): mean 0, variance 1. */
int busca_reid_reset_running_stats(busca_ctx* ctx);

/* The statistics as they are once the work enqueued on `stream` so far is done (an adapt in flight there included): copied to `host_out` and the
 * stream synchronised.  BUSCA_EINVAL without loaded running statistics. */
int busca_reid_get_running_stats(busca_ctx* ctx, float* host_out, size_t floats, void* stream);

/* busca_reid_forward_ex on the table of the running statistics: crop i's features depend on crop i alone.  BUSCA_EINVAL without loaded running
 * statistics (none loaded since the last weight load). */
int busca_reid_forward_running(busca_ctx* ctx, const uint8_t* crops, int32_t n, const uint8_t* zero_norm, int32_t output, float* feats, void* stream);

/* A batch-statistics forward (busca_reid_forward_ex: same schedule, same features) that also updates the running statistics as torch's train mode
 * does, on the stream: running = (1 - momentum) * running + momentum * batch, the batch variance UNBIASED (var * M / (M - 1), M = n x output pixels of
 * that conv), and rebuilds the table.  The batch statistics are recovered in float64 from the pass's finished (scale, shift) table and the affine
 * parameters - mean = (beta - shift) / scale, var + 1e-5 = (gamma / scale)^2 - so a channel whose gamma is 0 KEEPS its running statistics: its
 * table entry (0, beta) holds no trace of the batch, and no output depends on them.  A channel whose pair is not finite (a split-fp16 pass that
 * reports "reid_status" 2) keeps them as well.
 * momentum in [0, 1].  0 leaves the statistics and the table untouched and needs none loaded: a batch-statistics forward with an `output` choice.
 * Otherwise BUSCA_EINVAL without loaded running statistics. */
int busca_reid_adapt(busca_ctx* ctx, const uint8_t* crops, int32_t n, const uint8_t* zero_norm, double momentum, int32_t output, float* feats, void* stream);

#ifdef __cplusplus
}
#endif

#endif
