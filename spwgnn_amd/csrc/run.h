// The launch sequences behind the workspace entry points (host only): forward.hip, backward.hip.
#pragma once
#include "path.h"

namespace spw {

// spwgnn_run.prof_events: event pairs around the launches of kernel prof_kernel, in launch order
struct Prof {
    const spwgnn_run* r;
    hipStream_t st;
    mutable int k = 0;
    hipError_t before(int kid) const {
        if (r->prof_kernel != kid || !r->prof_events || k >= r->prof_count) return hipSuccess;
        return hipEventRecord(static_cast<hipEvent_t>(r->prof_events[2 * k]), st);
    }
    hipError_t after(int kid) const {
        if (r->prof_kernel != kid || !r->prof_events || k >= r->prof_count) return hipSuccess;
        hipError_t e = hipEventRecord(static_cast<hipEvent_t>(r->prof_events[2 * k + 1]), st);
        ++k;
        return e;
    }
};

#define SPW_CHECK(x)                                  \
    do {                                              \
        hipError_t e_ = (x);                          \
        if (e_ != hipSuccess) return (int32_t)e_;     \
    } while (0)
// a launch timed as kernel `kid`
#define SPW_TIMED(prof, kid, launch)      \
    do {                                  \
        SPW_CHECK((prof).before(kid));    \
        SPW_CHECK(launch);                \
        SPW_CHECK((prof).after(kid));     \
    } while (0)

// What a forward call asks for beyond (batch, run)
struct FwdCall {
    float* logits;             // the last step's row, the only one stored; with logit_step, [S][logit_step]
    bool keep_state = false;   // spwgnn_forward_state with a buffer: the last step leaves P_S in P_at(S) on every path
    int64_t logit_step = 0;    // spwgnn_forward_steps: step s stores its own row
    const float* gates = nullptr;   // spwgnn_forward_gated: one relation gate per edge slot (§3zz)
    int64_t gate_step = 0;          // spwgnn_forward_step_gated: gates is [S][gate_step], a row per step (§3zzc)
};

int32_t run_forward(const float* params, const spwgnn_batch* b, const spwgnn_run* r, const Ws& w, char* base,
                    const FwdCall& call, hipStream_t st);
int32_t run_backward(const spwgnn_batch* b, const spwgnn_run* r, const Ws& w, char* base, const BwdCall& call,
                     hipStream_t st);

}  // namespace spw
