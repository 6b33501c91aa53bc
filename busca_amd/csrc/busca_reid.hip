// libbusca_hip.so, ReID extractor: every flavour of the ResNet-50 kernels and their C-ABI (units: busca_internal.hpp).  gfx950 only.
#include "busca_internal.hpp"

#include "dt_kernel.hip.inc"          // (vector typedefs and the small device helpers the conv kernels share with the Decision Transformer)
#include "reid_kernel.hip.inc"
#include "reid_gram.hip.inc"
#include "reid_halo.hip.inc"
#include "reid_kwave.hip.inc"
#include "reid_pipe.hip.inc"
#include "reid_f32.hip.inc"
#include "reid_x3.hip.inc"
#include "reid_x3p.hip.inc"
#pragma GCC visibility push(default)
#include "../../include/busca_reid_bn.h"
#pragma GCC visibility pop
#include "reid_bn.hip.inc"
#include "reid_state.hip.inc"

ReidState* reid_state_new() { return new ReidState(); }
void reid_state_delete(ReidState* r) { if (r) { reid_free(*r); delete r; } }
bool reid_state_loaded(const ReidState* r) { return r && r->loaded; }

// "reid_*" names of busca_set_option / busca_get_option: the status word, and the schedule knobs REID_KNOBS names (reid_state.hip.inc).
int reid_set_option(busca_ctx* c, const char* name, int32_t value) {
    ReidState& R = *c->reid;
    if (!strcmp(name, "reid_status")) { if (R.xerr) *R.xerr = value; return BUSCA_OK; }      // 0 = the caller has read the status of its synchronised forwards and dealt with it
    if (!R.loaded) return fail(c, BUSCA_ENOWEIGHTS, "busca_set_option('%s'): ReID schedule options belong to a loaded extractor (load weights first)", name);
    if (const ReidKnobDesc* e = reid_knob_by_option(name)) { e->set(R.k, value); return BUSCA_OK; }
    return fail(c, BUSCA_EINVAL, "busca_set_option: unknown option '%s'", name);
}
int reid_get_option(busca_ctx* c, const char* name, int32_t* value) {
    const ReidState& R = *c->reid;
    // 0 ok, 2 = a split-fp16 (BUSCA_PREC_F16X3) forward since the status was last cleared staged an operand beyond |x| = 1023.5: its features are invalid (non-finite
    // statistics) - valid once the forwards' streams are synchronised
    if (!strcmp(name, "reid_status")) { *value = R.xerr ? *R.xerr : 0; return BUSCA_OK; }
    if (const ReidKnobDesc* e = reid_knob_by_option(name)) { *value = e->get(R.k); return BUSCA_OK; }
    return fail(c, BUSCA_EINVAL, "busca_get_option: unknown option '%s'", name);
}

#include "reid_weights.hip.inc"
#include "reid_schedule.hip.inc"
#include "capi_reid.hip.inc"
#include "capi_reid_bn.hip.inc"
