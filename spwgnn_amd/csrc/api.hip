// C-ABI entry points of libspwgnn_hip.so: argument checks, then the launch sequences of forward.hip and
// backward.hip on the caller's workspace (workspace.h), or a single launch.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "run.h"
static_assert(SPWGNN_MATH_F32 == spw::MATH_F32 && SPWGNN_MATH_X6 == spw::MATH_X6 && SPWGNN_MATH_BF16 == spw::MATH_BF16 &&
                  SPWGNN_MATH_X3 == spw::MATH_X3 && SPWGNN_MATH_H3 == spw::MATH_H3,
              "math ids");

using namespace spw;

static int32_t validate(const spwgnn_batch* b, const spwgnn_run* r) {
    if (!b || !r) return SPWGNN_E_ARG;
    if (b->n_nodes < 1 || b->n_wtiles < 1 || b->n_eblocks < 1) return SPWGNN_E_SHAPE;
    if (b->nw_max < 1 || b->nw_max > kNwMaxLimit) return SPWGNN_E_SHAPE;
    if (r->mp_steps < 1 || r->mp_steps > 64) return SPWGNN_E_SHAPE;
    if (!b->pos || !b->wtile || !b->edge_src || !b->edge_dst || !b->blk_csr) return SPWGNN_E_ARG;
    if (r->dropout < 0.f || r->dropout >= 1.f) return SPWGNN_E_ARG;
    if (math_products(r->math) < 0) return SPWGNN_E_ARG;   // an id this library does not know
    if (r->training && r->dropout > 0.f && (!b->node_tower || !b->node_local)) return SPWGNN_E_ARG;
    return SPWGNN_OK;
}

extern "C" {

int64_t spwgnn_workspace_bytes(int32_t n_nodes, int32_t n_eblocks, int32_t mp_steps, int32_t training) {
    if (n_nodes < 1 || n_eblocks < 1 || mp_steps < 1) return -1;
    return make_ws(n_nodes, n_eblocks, mp_steps, training ? 1 : 0).total;
}

int32_t spwgnn_fused_path(const spwgnn_batch* batch, const spwgnn_run* run) {
    const int32_t stt = validate(batch, run);
    if (stt) return stt;
    const Path p = make_path(batch, run, make_ws(batch->n_nodes, batch->n_eblocks, run->mp_steps, run->training ? 1 : 0));
    return (p.fwd_fused ? 1 : 0) | (run->training && p.bwd_fused ? 2 : 0);
}

// the same answer for a call of this batch and run with relation gates (spwgnn_forward_gated / _backward_gated)
int32_t spwgnn_fused_path_gated(const spwgnn_batch* batch, const spwgnn_run* run) {
    const int32_t stt = validate(batch, run);
    if (stt) return stt;
    if (!math_split32(run->math)) return SPWGNN_E_SHAPE;
    const Path p = make_path(batch, run, make_ws(batch->n_nodes, batch->n_eblocks, run->mp_steps, run->training ? 1 : 0),
                             nullptr, true);
    return (p.fwd_fused ? 1 : 0) | (run->training && p.bwd_fused ? 2 : 0);
}

int32_t spwgnn_host_device_ptr(const void* host, void** dev) {
    if (!host || !dev) return SPWGNN_E_ARG;
    void* p = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&p, const_cast<void*>(host), 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // not this thread's next launch error
        return (int32_t)e;
    }
    if (!p) return SPWGNN_E_ARG;
    *dev = p;
    return SPWGNN_OK;
}

int32_t spwgnn_team_max_blocks(int32_t set) { return team_max_blocks(set); }
int32_t spwgnn_da_stored_steps(int32_t set) { return da_stored_steps(set); }
int32_t spwgnn_math_products(int32_t math) { return math_products(math); }
int32_t spwgnn_math_products_bwd(int32_t math) { return math_products_bwd(math); }
// relation gates: the split maths with fp32 storage (one template family of the wide kernels)
int32_t spwgnn_gates_supported(int32_t math) { return math_products(math) < 0 ? -1 : math_split32(math) ? 1 : 0; }

static int32_t status(hipError_t e) { return e == hipSuccess ? SPWGNN_OK : (int32_t)e; }
static bool mis16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 != 0; }

// The prologue of every workspace call, in the order the status codes keep: validate, E_NOTRAIN, the
// call's own argument checks (args_ok: the caller evaluates it first, so it follows neither batch nor
// run), E_WORKSPACE. Fills w on SPWGNN_OK. gated: a call with relation gates — its math is a shape question
// (SPWGNN_E_SHAPE where spwgnn_gates_supported answers 0), asked right after validate.
static int32_t enter(const spwgnn_batch* batch, const spwgnn_run* run, const void* workspace, int64_t bytes,
                     bool need_training, bool args_ok, Ws& w, bool gated = false) {
    if (int32_t stt = validate(batch, run)) return stt;
    if (gated && !math_split32(run->math)) return SPWGNN_E_SHAPE;
    if (need_training && !run->training) return SPWGNN_E_NOTRAIN;
    if (!args_ok || !workspace) return SPWGNN_E_ARG;
    w = make_ws(batch->n_nodes, batch->n_eblocks, run->mp_steps, run->training ? 1 : 0);
    return bytes < w.total ? SPWGNN_E_WORKSPACE : SPWGNN_OK;
}

int32_t spwgnn_forward(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                       int64_t workspace_bytes, float* logits, spwgnn_stream_t stream) {
    Ws w;
    if (int32_t stt = enter(batch, run, workspace, workspace_bytes, false, params && logits, w)) return stt;
    return run_forward(params, batch, run, w, static_cast<char*>(workspace), {logits}, static_cast<hipStream_t>(stream));
}

// spwgnn_forward_state (one logit row) and spwgnn_forward_steps (each step's node side given its own row,
// DESIGN.md §3zr): the forward, then the state's export
static int32_t forward_state(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                             int64_t workspace_bytes, float* logits, float* state_out, bool steps,
                             spwgnn_stream_t stream, const float* gates = nullptr, int64_t gate_step = 0,
                             bool gate_step_ok = true) {
    Ws w;
    if (int32_t stt = enter(batch, run, workspace, workspace_bytes, false,
                            params && logits && !mis16(state_out) && !mis16(gates) && gate_step_ok, w, gates != nullptr))
        return stt;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const FwdCall call{logits, state_out != nullptr, steps ? batch->n_nodes : 0, gates, gate_step};
    const int32_t stt = run_forward(params, batch, run, w, static_cast<char*>(workspace), call, st);
    if (stt || !state_out) return stt;
    const Ctx c{w, static_cast<char*>(workspace), false};
    const Prof prof{run, st};
    SPW_TIMED(prof, SPWGNN_K_STATE, launch_state_export(c.f(w.P_at(run->mp_steps)), state_out, batch->n_nodes, st));
    return SPWGNN_OK;
}

int32_t spwgnn_forward_state(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                             int64_t workspace_bytes, float* logits, float* state_out, spwgnn_stream_t stream) {
    return forward_state(params, batch, run, workspace, workspace_bytes, logits, state_out, false, stream);
}

// gates null: spwgnn_forward_state itself. Otherwise the argument checks of that call, the gate pointer's own,
// then the math (SPWGNN_E_SHAPE for one spwgnn_gates_supported answers 0 to) — all before any device work
int32_t spwgnn_forward_gated(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                             int64_t workspace_bytes, const float* gates, float* logits, float* state_out,
                             spwgnn_stream_t stream) {
    return forward_state(params, batch, run, workspace, workspace_bytes, logits, state_out, false, stream, gates);
}

// per-step gates: a row's stride holds the plan's slots and keeps every row 16-byte aligned.
// Asked only with gates; a null batch is enter's SPWGNN_E_ARG
static bool gate_step_ok(const spwgnn_batch* batch, const float* gates, int64_t gate_step) {
    return !gates || !batch || (gate_step % 4 == 0 && gate_step >= (int64_t)batch->n_eblocks * 32);
}

// gates null: spwgnn_forward_state itself. Otherwise spwgnn_forward_gated with row s of gates [mp_steps][gate_step]
// at step s: the same checks (and gate_step's: SPWGNN_E_ARG) before any device work, the same launches
int32_t spwgnn_forward_step_gated(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                                  int64_t workspace_bytes, const float* gates, int64_t gate_step, float* logits,
                                  float* state_out, spwgnn_stream_t stream) {
    return forward_state(params, batch, run, workspace, workspace_bytes, logits, state_out, false, stream, gates,
                         gates ? gate_step : 0, gate_step_ok(batch, gates, gate_step));
}

int32_t spwgnn_forward_steps(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                             int64_t workspace_bytes, float* step_logits, float* state_out, spwgnn_stream_t stream) {
    return forward_state(params, batch, run, workspace, workspace_bytes, step_logits, state_out, true, stream);
}

// every backward entry point: `ok` is the call's own argument check (params included: the packed copies the
// forward made on this workspace are what the kernels read)
static int32_t backward(const spwgnn_batch* batch, const spwgnn_run* run, void* workspace, int64_t workspace_bytes,
                        bool ok, const BwdCall& call, spwgnn_stream_t stream) {
    Ws w;
    if (int32_t stt = enter(batch, run, workspace, workspace_bytes, true, ok, w, call.gates != nullptr)) return stt;
    return run_backward(batch, run, w, static_cast<char*>(workspace), call, static_cast<hipStream_t>(stream));
}

int32_t spwgnn_backward(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                        int64_t workspace_bytes, const float* dlogits, float* grads, float* dprop,
                        spwgnn_stream_t stream) {
    return backward(batch, run, workspace, workspace_bytes, params && dlogits && grads, {dlogits, grads, dprop}, stream);
}

int32_t spwgnn_backward_state(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                              int64_t workspace_bytes, const float* dlogits, const float* dstate, float* grads,
                              float* dprop, spwgnn_stream_t stream) {
    const bool ok = params && dlogits && grads && !mis16(dstate);
    return backward(batch, run, workspace, workspace_bytes, ok, {dlogits, grads, dprop, nullptr, dstate}, stream);
}

// gates null: spwgnn_backward_state itself; the gates hold what the forward's held (the caller's contract)
int32_t spwgnn_backward_gated(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                              int64_t workspace_bytes, const float* gates, const float* dlogits, const float* dstate,
                              float* grads, float* dprop, spwgnn_stream_t stream) {
    const bool ok = params && dlogits && grads && !mis16(dstate) && !mis16(gates);
    BwdCall call{dlogits, grads, dprop, nullptr, dstate};
    call.gates = gates;
    return backward(batch, run, workspace, workspace_bytes, ok, call, stream);
}

// gates null: spwgnn_backward_state itself; row s of gates [mp_steps][gate_step] holds what the forward's held
int32_t spwgnn_backward_step_gated(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                                   int64_t workspace_bytes, const float* gates, int64_t gate_step, const float* dlogits,
                                   const float* dstate, float* grads, float* dprop, spwgnn_stream_t stream) {
    const bool ok = params && dlogits && grads && !mis16(dstate) && !mis16(gates) && gate_step_ok(batch, gates, gate_step);
    BwdCall call{dlogits, grads, dprop, nullptr, dstate};
    call.gates = gates;
    call.gate_step = gates ? gate_step : 0;
    return backward(batch, run, workspace, workspace_bytes, ok, call, stream);
}

int32_t spwgnn_backward_steps(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                              int64_t workspace_bytes, const float* dstep_logits, const float* dstate, float* grads,
                              float* dprop, spwgnn_stream_t stream) {
    const bool ok = params && dstep_logits && grads && !mis16(dstate);
    const int64_t dl_step = batch ? batch->n_nodes : 0;   // a null batch: enter's SPWGNN_E_ARG
    return backward(batch, run, workspace, workspace_bytes, ok, {dstep_logits, grads, dprop, nullptr, dstate, dl_step}, stream);
}

int32_t spwgnn_backward_inputs(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                               int64_t workspace_bytes, float* dpos, spwgnn_stream_t stream) {
    Ws w;
    if (int32_t stt = enter(batch, run, workspace, workspace_bytes, true, params && dpos && !mis16(dpos), w)) return stt;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Ctx c{w, static_cast<char*>(workspace), false};
    const ParamTable& pt = param_table();
    InputBwdArgs a{};
    a.n_wtiles = batch->n_wtiles;
    a.n_eblocks = batch->n_eblocks;
    a.n_nodes = batch->n_nodes;
    a.wtile = batch->wtile;
    a.esrc = batch->edge_src;
    a.edst = batch->edge_dst;
    a.dz1 = c.f(w.dz1);     // the Y operands of the rm.0 / om.0 weight gradients (backward.hip wg_rm0, wg_om0),
    a.dzo1 = c.f(w.dzo1);   // as the backward left them
    a.b16 = make_path(batch, run, w).b16;   // wg_rm0's kB16Y
    a.w_rm0 = params + pt.t[T_RM0K].offset;
    a.w_om0 = params + pt.t[T_OM0K].offset;
    a.dpos = reinterpret_cast<float4*>(dpos);
    const Prof prof{run, st};
    SPW_TIMED(prof, SPWGNN_K_INPUT_BWD, launch_input_bwd(a, st));
    return SPWGNN_OK;
}

// The rows k_rel_bwd reads are operands of the weight gradients, which every launch path (wide, receiver
// blocks, team / fused, the loop-end shortcuts) runs over all S steps after the step loop: A, U_s, V_s,
// G3_s of the W2 gradient (backward.hip wg_w2; U_0, V_0 unwritten under a null prop: uv_zero, as there) and
// g_s of the rmp.2 gradient (wg_node, bf16 under Path::n16). No path leaves one out, so none is refused.
int32_t spwgnn_backward_relations(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                                  int64_t workspace_bytes, float* drel, float* drel_steps, spwgnn_stream_t stream) {
    Ws w;
    if (int32_t stt = enter(batch, run, workspace, workspace_bytes, true, params && drel, w)) return stt;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Ctx c{w, static_cast<char*>(workspace), false};
    const ParamTable& pt = param_table();
    const Path p = make_path(batch, run, w);
    RelBwdArgs a{};
    a.n_eblocks = batch->n_eblocks;
    a.n_nodes = batch->n_nodes;
    a.S = run->mp_steps;
    a.uv_zero = !batch->prop;
    a.step_e = w.RN * kRowE;
    a.step_n = w.RN * kRowN;
    a.esrc = batch->edge_src;
    a.edst = batch->edge_dst;
    a.A = c.f(w.A);
    a.U = c.f(w.U);
    a.V = c.f(w.V);
    a.G3 = c.f(w.G3);
    a.g = c.f(w.g);
    a.w2 = params + pt.t[T_RMP1K].offset;
    a.b2 = params + pt.t[T_RMP1B].offset;
    a.b3 = params + pt.t[T_RMP2B].offset;
    a.drel = drel;
    a.drel_steps = drel_steps;
    const Prof prof{run, st};
    SPW_TIMED(prof, SPWGNN_K_REL_BWD, launch_rel_bwd(a, math_bwd(run->math), p.b16, p.n16, st));
    return SPWGNN_OK;
}

// DropEdge. rate in [0, 1) → drop_keep's threshold, as set_dropout forms the feature dropout's
static bool dropedge_thresh(float rate, uint32_t& thresh) {
    if (!(rate >= 0.f && rate < 1.f)) return false;   // NaN included
    thresh = (uint32_t)std::min(4294967295.0, std::floor((double)rate * 4294967296.0));
    return true;
}
constexpr int32_t kDropEdgeFlags = SPWGNN_DROPEDGE_SYMMETRIC | SPWGNN_DROPEDGE_RESCALE;

int32_t spwgnn_dropedge_keep_host_step(uint64_t key, uint32_t tower, uint32_t a, uint32_t b, uint32_t step, float rate,
                                       int32_t flags) {
    uint32_t thresh;
    if (!dropedge_thresh(rate, thresh) || (flags & ~kDropEdgeFlags)) return SPWGNN_E_ARG;
    return dropedge_keep(key, tower, a, b, (flags & SPWGNN_DROPEDGE_SYMMETRIC) != 0, thresh, step) ? 1 : 0;
}
int32_t spwgnn_dropedge_keep_host(uint64_t key, uint32_t tower, uint32_t a, uint32_t b, float rate, int32_t flags) {
    return spwgnn_dropedge_keep_host_step(key, tower, a, b, 0u, rate, flags);
}

// steps rows of gates at stride gate_step (one row: spwgnn_dropedge_gates), base rows at stride base_step
static int32_t dropedge_rows(const spwgnn_batch* batch, const spwgnn_run* run, float rate, int32_t flags,
                             const float* base, int64_t base_step, float* gates, int steps, int64_t gate_step,
                             spwgnn_stream_t stream) {
    if (!batch || !run || !gates) return SPWGNN_E_ARG;
    DropEdgeArgs a{};
    if (!dropedge_thresh(rate, a.thresh) || (flags & ~kDropEdgeFlags)) return SPWGNN_E_ARG;
    if (batch->n_nodes < 1 || batch->n_eblocks < 1 || batch->n_eblocks > (INT32_MAX >> 5)) return SPWGNN_E_SHAPE;
    if (steps < 1) return SPWGNN_E_SHAPE;
    if (steps > 1 || gate_step || base_step) {   // the per-step call's strides: whole rows, 16-byte aligned
        const int64_t slots = (int64_t)batch->n_eblocks * 32;
        if (gate_step < slots || gate_step % 4 || (base && base_step && (base_step < slots || base_step % 4)) || base_step < 0)
            return SPWGNN_E_ARG;
    }
    if (!batch->edge_src || !batch->edge_dst || !batch->node_tower || !batch->node_local) return SPWGNN_E_ARG;
    const auto mis = [](const void* q, uintptr_t al) { return reinterpret_cast<uintptr_t>(q) % al != 0; };
    if (mis(gates, 16) || mis(base, 4) || mis(batch->edge_src, 4) || mis(batch->edge_dst, 4) ||
        mis(batch->node_tower, 4) || mis(batch->node_local, 4) || mis(run->seed_dev, 8))
        return SPWGNN_E_ARG;
    a.slots = (int64_t)batch->n_eblocks * 32;
    a.n_nodes = batch->n_nodes;
    a.esrc = batch->edge_src;
    a.edst = batch->edge_dst;
    a.node_tower = batch->node_tower;
    a.node_local = batch->node_local;
    a.base = base;
    a.gates = gates;
    a.steps = steps;
    a.gate_step = gate_step;
    a.base_step = base ? base_step : 0;
    a.scale = (flags & SPWGNN_DROPEDGE_RESCALE) ? 1.0f / (1.0f - rate) : 1.0f;
    a.symmetric = (flags & SPWGNN_DROPEDGE_SYMMETRIC) ? 1 : 0;
    a.seed = run->seed;
    a.seed_dev = run->seed_dev;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Prof prof{run, st};
    SPW_TIMED(prof, SPWGNN_K_DROPEDGE, launch_dropedge(a, st));
    return SPWGNN_OK;
}

int32_t spwgnn_dropedge_gates(const spwgnn_batch* batch, const spwgnn_run* run, float rate, int32_t flags,
                              const float* base, float* gates, spwgnn_stream_t stream) {
    return dropedge_rows(batch, run, rate, flags, base, 0, gates, 1, 0, stream);
}

// one launch writes all mp_steps rows: row s drawn with feature s of the edge's row key, so row 0
// is spwgnn_dropedge_gates' mask
int32_t spwgnn_dropedge_step_gates(const spwgnn_batch* batch, const spwgnn_run* run, float rate, int32_t flags,
                                   const float* base, int64_t base_step, float* gates, int64_t gate_step,
                                   spwgnn_stream_t stream) {
    if (!run) return SPWGNN_E_ARG;
    if (run->mp_steps < 1) return SPWGNN_E_SHAPE;
    if (gate_step <= 0) return SPWGNN_E_ARG;
    return dropedge_rows(batch, run, rate, flags, base, base_step, gates, run->mp_steps, gate_step, stream);
}

// Argument checks of the device-plan calls (no device work): 0, or the status to return.
static int32_t plan_device_check(const spwgnn_plan_device* p) {
    if (!p) return SPWGNN_E_ARG;
    if (p->n_towers < 1 || p->n_nodes < 1 || p->n_wtiles < 1 || p->n_eblocks < 1) return SPWGNN_E_ARG;
    if (p->nw_max < 1 || p->nw_max > kNwMaxLimit) return SPWGNN_E_SHAPE;
    // whole towers of >= 1 node in tiles of >= 1 tower and >= 1 block; 32·n_eblocks must stay an int32
    if (p->n_towers > p->n_nodes || p->n_wtiles > p->n_towers || p->n_eblocks < p->n_wtiles ||
        p->n_eblocks > (INT32_MAX >> 5) || (int64_t)p->n_wtiles * p->nw_max < p->n_nodes)
        return SPWGNN_E_SHAPE;
    if (!p->wtile || !p->node_local || !p->wtile_tower || !p->edge_src || !p->edge_dst || !p->blk_csr || !p->status)
        return SPWGNN_E_ARG;
    const auto mis = [](const void* q, uintptr_t al) { return reinterpret_cast<uintptr_t>(q) % al != 0; };
    if (mis(p->wtile, 4) || mis(p->node_local, 4) || mis(p->wtile_tower, 4) || mis(p->tower_cap, 4) ||
        mis(p->edge_src, 4) || mis(p->edge_dst, 4) || mis(p->blk_csr, 16) || mis(p->pos, 16) ||
        mis(p->tower_edges, 4) || mis(p->status, 4))
        return SPWGNN_E_ARG;
    return SPWGNN_OK;
}

static int32_t plan_device_launch(const spwgnn_plan_device* p, PlanDevArgs& a, bool dense, hipStream_t st) {
    a.n_wtiles = p->n_wtiles;
    a.n_eblocks = p->n_eblocks;
    a.n_nodes = p->n_nodes;
    a.n_towers = p->n_towers;
    a.wtile = p->wtile;
    a.node_local = p->node_local;
    a.wtile_tower = p->wtile_tower;
    a.tower_cap = p->tower_cap;
    a.esrc = p->edge_src;
    a.edst = p->edge_dst;
    a.csr = p->blk_csr;
    a.tower_edges = p->tower_edges;
    a.status = p->status;
    if (p->prof_events) SPW_CHECK(hipEventRecord(static_cast<hipEvent_t>(p->prof_events[0]), st));
    SPW_CHECK(launch_plan_device(a, dense, st));
    if (p->prof_events) SPW_CHECK(hipEventRecord(static_cast<hipEvent_t>(p->prof_events[1]), st));
    return SPWGNN_OK;
}

int32_t spwgnn_plan_device_positions(const spwgnn_plan_device* plan, const float* raw, int32_t raw_stride,
                                     float threshold, float divisor, spwgnn_stream_t stream) {
    const int32_t stt = plan_device_check(plan);
    if (stt) return stt;
    if (!raw || reinterpret_cast<uintptr_t>(raw) % 4 || raw_stride < 2) return SPWGNN_E_ARG;
    if (plan->pos && raw_stride < 3) return SPWGNN_E_ARG;
    if (!(divisor > 0.f || divisor < 0.f)) return SPWGNN_E_ARG;   // zero or NaN
    PlanDevArgs a{};
    a.raw = raw;
    a.raw_stride = raw_stride;
    a.thr = threshold;
    a.divisor = divisor;
    a.pos = reinterpret_cast<float4*>(plan->pos);
    return plan_device_launch(plan, a, false, static_cast<hipStream_t>(stream));
}

int32_t spwgnn_plan_device_dense(const spwgnn_plan_device* plan, const float* Rs, const float* Rr, int32_t B,
                                 int32_t N, spwgnn_stream_t stream) {
    const int32_t stt = plan_device_check(plan);
    if (stt) return stt;
    if (B < 1 || N < 1 || plan->pos) return SPWGNN_E_ARG;
    // single-box towers have no relation slot (E = 0): their empty matrices may be null
    if (((!Rs || !Rr) && N > 1) || reinterpret_cast<uintptr_t>(Rs) % 4 || reinterpret_cast<uintptr_t>(Rr) % 4)
        return SPWGNN_E_ARG;
    if (N > plan->nw_max || B != plan->n_towers || (int64_t)B * N != plan->n_nodes) return SPWGNN_E_SHAPE;
    PlanDevArgs a{};
    a.Rs = Rs;
    a.Rr = Rr;
    a.N = N;
    a.E = N * (N - 1);
    return plan_device_launch(plan, a, true, static_cast<hipStream_t>(stream));
}

// spwgnn_loss_weights' own checks (no pointer followed past lw itself)
static bool loss_weights_ok(const spwgnn_loss_weights* lw) {
    return lw && lw->w && (lw->norm_dev || lw->norm > 0.0);
}
// The one-row loss's arguments (lw null: unweighted); spwgnn_bce_steps' rows start at the same pointers.
static BceArgs bce_args(const float* logits, const float* targets, int64_t n, float* out3, float* dlogits,
                        void* scratch, const double* weights3, double* total3, const spwgnn_loss_weights* lw) {
    BceArgs a{};
    a.w3 = weights3;
    a.tot3 = total3;
    a.logits = logits;
    a.targets = targets;
    a.n = n;
    a.dlogits = dlogits;
    a.partial = static_cast<float*>(scratch);
    a.out3 = out3;
    a.blocks = (int)std::min<int64_t>(256, (n + 255) / 256);
    if (lw) {
        a.w = lw->w;
        a.norm_dev = lw->norm_dev;
        a.norm = lw->norm_dev ? 0.f : (float)lw->norm;
    }
    return a;
}

// spwgnn_bce_backward (weighted false, lw null) and spwgnn_bce_backward_weighted
static int32_t bce_backward(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                            int64_t workspace_bytes, const float* logits, const float* targets, int64_t n,
                            float* out3, float* dlogits, void* bce_scratch, const double* weights3, double* total3,
                            float* grads, float* dprop, const spwgnn_loss_weights* lw, bool weighted,
                            spwgnn_stream_t stream) {
    // the folded loss indexes logits, targets and dlogits by plan node: one entry per node, no fewer
    const bool ok = batch && n == batch->n_nodes && params && grads && logits && targets && out3 && dlogits &&
                    bce_scratch && n >= 1 && (!weights3) == (!total3) && (!weighted || loss_weights_ok(lw));
    Ws w;
    if (int32_t stt = enter(batch, run, workspace, workspace_bytes, true, ok, w)) return stt;
    const BceArgs a = bce_args(logits, targets, n, out3, dlogits, bce_scratch, weights3, total3, lw);
    return run_backward(batch, run, w, static_cast<char*>(workspace), {dlogits, grads, dprop, &a},
                        static_cast<hipStream_t>(stream));
}

int32_t spwgnn_bce_backward(const float* params, const spwgnn_batch* batch, const spwgnn_run* run, void* workspace,
                            int64_t workspace_bytes, const float* logits, const float* targets, int64_t n,
                            float* out3, float* dlogits, void* bce_scratch, const double* weights3, double* total3,
                            float* grads, float* dprop, spwgnn_stream_t stream) {
    return bce_backward(params, batch, run, workspace, workspace_bytes, logits, targets, n, out3, dlogits, bce_scratch,
                        weights3, total3, grads, dprop, nullptr, false, stream);
}

int32_t spwgnn_bce_backward_weighted(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                                     void* workspace, int64_t workspace_bytes, const float* logits,
                                     const float* targets, int64_t n, float* out3, float* dlogits, void* bce_scratch,
                                     const double* weights3, double* total3, float* grads, float* dprop,
                                     const spwgnn_loss_weights* lw, spwgnn_stream_t stream) {
    return bce_backward(params, batch, run, workspace, workspace_bytes, logits, targets, n, out3, dlogits, bce_scratch,
                        weights3, total3, grads, dprop, lw, true, stream);
}

int64_t spwgnn_bce_scratch_bytes(int64_t n) {
    (void)n;
    return 256 * 3 * sizeof(float);   // [blocks][3] for the weighted loss; the unweighted one uses [blocks][2]
}

static int32_t bce_launch(const float* logits, const float* targets, int64_t n, float* out3, float* dlogits,
                          void* scratch, const double* weights3, double* total3, const spwgnn_loss_weights* lw,
                          spwgnn_stream_t stream) {
    if (!logits || !targets || !out3 || !scratch || n < 1) return SPWGNN_E_ARG;
    const BceArgs a = bce_args(logits, targets, n, out3, dlogits, scratch, weights3, total3, lw);
    return status(launch_bce(a, static_cast<hipStream_t>(stream)));
}

int32_t spwgnn_bce(const float* logits, const float* targets, int64_t n, float* out3, float* dlogits, void* scratch,
                   spwgnn_stream_t stream) {
    return bce_launch(logits, targets, n, out3, dlogits, scratch, nullptr, nullptr, nullptr, stream);
}

int32_t spwgnn_bce_accumulate(const float* logits, const float* targets, int64_t n, float* out3, float* dlogits,
                              void* scratch, const double* weights3, double* total3, spwgnn_stream_t stream) {
    if (!weights3 || !total3) return SPWGNN_E_ARG;
    return bce_launch(logits, targets, n, out3, dlogits, scratch, weights3, total3, nullptr, stream);
}

int32_t spwgnn_bce_weighted(const float* logits, const float* targets, int64_t n, const spwgnn_loss_weights* lw,
                            float* out3, float* dlogits, void* scratch, const double* weights3, double* total3,
                            spwgnn_stream_t stream) {
    if (!loss_weights_ok(lw) || (!weights3) != (!total3)) return SPWGNN_E_ARG;
    return bce_launch(logits, targets, n, out3, dlogits, scratch, weights3, total3, lw, stream);
}

// The tower-level loss: the node row's partials [256][3], then the towers' [kTowerBlocksMax][3]
int64_t spwgnn_bce_tower_scratch_bytes(int64_t n, int32_t n_towers) {
    if (n < 1 || n_towers < 1) return -1;
    return (int64_t)(256 + kTowerBlocksMax) * 3 * sizeof(float);
}

int32_t spwgnn_bce_tower(const float* logits, const float* targets, int64_t n, const spwgnn_loss_weights* lw,
                         const spwgnn_tower_loss* tl, float* out3, float* dlogits, void* scratch,
                         spwgnn_stream_t stream) {
    if (!logits || !tl || !out3 || !scratch || n < 1) return SPWGNN_E_ARG;
    if (!tl->tower_offsets || !tl->out6 || tl->n_towers < 1 || tl->reserved != 0) return SPWGNN_E_ARG;
    if (!std::isfinite(tl->mu) || !(tl->mu > 0.f) || !std::isfinite(tl->alpha) || tl->alpha < 0.f) return SPWGNN_E_ARG;
    if (!targets && !(tl->alpha == 0.f && tl->tower_targets)) return SPWGNN_E_ARG;
    if (!tl->norm_t_dev && !(tl->norm_t > 0.0)) return SPWGNN_E_ARG;
    if ((!tl->weights6) != (!tl->total6) || (lw && !loss_weights_ok(lw))) return SPWGNN_E_ARG;
    TowerLossArgs a{};
    a.b = bce_args(logits, targets, n, tl->out6, nullptr, scratch, nullptr, nullptr, lw);
    a.off = tl->tower_offsets;
    a.ttargets = tl->tower_targets;
    a.n_towers = tl->n_towers;
    a.tblocks = (int)std::min<int64_t>(kTowerBlocksMax, ((int64_t)tl->n_towers + 255) / 256);
    a.alpha = tl->alpha;
    a.mu = tl->mu;
    a.norm_t_dev = tl->norm_t_dev;
    a.norm_t = tl->norm_t_dev ? 0.f : (float)tl->norm_t;
    a.dlogits = dlogits;
    a.tpartial = static_cast<float*>(scratch) + 256 * 3;
    a.out3 = out3;
    a.out6 = tl->out6;
    a.per_tower = tl->per_tower;
    a.w6 = tl->weights6;
    a.tot6 = tl->total6;
    return status(launch_bce_tower(a, static_cast<hipStream_t>(stream)));
}

int64_t spwgnn_bce_steps_scratch_bytes(int64_t n, int32_t mp_steps) {
    (void)n;
    if (mp_steps < 1 || mp_steps > kMaxSteps) return -1;
    return (int64_t)mp_steps * 256 * 3 * sizeof(float);   // [S][blocks][3]
}

int32_t spwgnn_bce_steps(const float* step_logits, const float* targets, int64_t n, int32_t mp_steps,
                         const spwgnn_step_weights* sw, const spwgnn_loss_weights* lw, float* out3s, float* out3,
                         float* dlogits, void* scratch, const double* weights3, double* total3, double* total3s,
                         spwgnn_stream_t stream) {
    if (!step_logits || !targets || !out3s || !out3 || !scratch || !sw || n < 1) return SPWGNN_E_ARG;
    if (mp_steps < 1 || mp_steps > kMaxSteps || sw->count != mp_steps) return SPWGNN_E_ARG;
    if ((lw && !loss_weights_ok(lw)) || (!weights3) != (!total3) || (total3s && !weights3)) return SPWGNN_E_ARG;
    bool any = false;
    for (int s = 0; s < mp_steps; ++s) {
        const float l = sw->lambda[s];
        if (!std::isfinite(l) || l < 0.f) return SPWGNN_E_ARG;
        any = any || l != 0.f;
    }
    if (!any) return SPWGNN_E_ARG;
    BceStepsArgs a{};
    a.b = bce_args(step_logits, targets, n, out3, dlogits, scratch, weights3, total3, lw);
    a.S = mp_steps;
    a.out3s = out3s;
    a.tot3s = total3s;
    for (int s = 0; s < mp_steps; ++s) a.lambda[s] = sw->lambda[s];
    return status(launch_bce_steps(a, static_cast<hipStream_t>(stream)));
}

static float adam_lr_t(float lr, float beta1, float beta2, double t) {
    return (float)(lr * std::sqrt(1.0 - std::pow((double)beta2, t)) / (1.0 - std::pow((double)beta1, t)));
}

int32_t spwgnn_adam_lr_table(float lr, float beta1, float beta2, int32_t n, float* out) {
    if (!out || n < 2) return SPWGNN_E_ARG;
    out[0] = 0.f;   // step 0 never runs (steps count from 1)
    for (int32_t t = 1; t < n; ++t) out[t] = adam_lr_t(lr, beta1, beta2, (double)t);
    return SPWGNN_OK;
}

// what every Adam step shares; the caller adds lr_t (a host step count) or the device step word and table
static AdamArgs adam_args(float* params, const float* grads, float* m, float* v, int64_t n, float beta1, float beta2,
                          float eps, float l2, float grad_scale) {
    AdamArgs a{};
    a.p = params;
    a.g = grads;
    a.m = m;
    a.v = v;
    a.n = n;
    a.b1 = beta1;
    a.b2 = beta2;
    a.eps = eps;
    a.l2 = l2;
    a.gscale = grad_scale;
    return a;
}

int32_t spwgnn_adam_dev(float* params, const float* grads, float* m, float* v, int64_t n, const int32_t* step_dev,
                        const float* lr_table, int32_t table_len, float beta1, float beta2, float eps, float l2,
                        float grad_scale, spwgnn_stream_t stream) {
    if (!params || !grads || !m || !v || n < 1 || !step_dev || !lr_table || table_len < 2) return SPWGNN_E_ARG;
    AdamArgs a = adam_args(params, grads, m, v, n, beta1, beta2, eps, l2, grad_scale);
    a.step_dev = step_dev;
    a.lr_table = lr_table;
    a.table_len = table_len;
    return status(launch_adam(a, static_cast<hipStream_t>(stream)));
}

int32_t spwgnn_step_advance(uint64_t* key_dev, int32_t* step_dev, int32_t mode, uint64_t seed, int32_t rank,
                            spwgnn_stream_t stream) {
    if (!key_dev || !step_dev || mode < SPWGNN_STEP_KEY_COUNTER || mode > SPWGNN_STEP_KEY_SPLITMIX) return SPWGNN_E_ARG;
    return status(launch_step_advance(key_dev, step_dev, mode, seed, rank, static_cast<hipStream_t>(stream)));
}

int32_t spwgnn_adam(float* params, const float* grads, float* m, float* v, int64_t n, int32_t step, float lr,
                    float beta1, float beta2, float eps, float l2, float grad_scale, spwgnn_stream_t stream) {
    if (!params || !grads || !m || !v || n < 1 || step < 1) return SPWGNN_E_ARG;
    AdamArgs a = adam_args(params, grads, m, v, n, beta1, beta2, eps, l2, grad_scale);
    a.lr_t = adam_lr_t(lr, beta1, beta2, (double)step);
    return status(launch_adam(a, static_cast<hipStream_t>(stream)));
}

// ---- clipnorm / clipvalue / decay / the non-finite guard ----
float spwgnn_adam_lr_decayed(float lr, float decay, int64_t iterations) {
    if (!(decay > 0.f) || iterations <= 0) return lr;
    return (float)((double)lr * (1.0 / (1.0 + (double)decay * (double)iterations)));
}

int32_t spwgnn_adam_lr_table_decay(float lr, float decay, float beta1, float beta2, int32_t n, float* out) {
    if (!out || n < 2 || !(decay >= 0.f)) return SPWGNN_E_ARG;
    out[0] = 0.f;   // step 0 never runs (steps count from 1)
    for (int32_t t = 1; t < n; ++t)
        out[t] = adam_lr_t(spwgnn_adam_lr_decayed(lr, decay, (int64_t)t - 1), beta1, beta2, (double)t);
    return SPWGNN_OK;
}

int64_t spwgnn_clip_scratch_bytes(void) { return (int64_t)kClipBlocks * (int64_t)sizeof(float); }

// the checks both entry points share and the arguments they have in common; nothing is launched on an error
static int32_t clip_args(ClipArgs& c, float* params, const float* grads, float* m, float* v, int64_t n, float beta1,
                         float beta2, float eps, float l2, float grad_scale, const spwgnn_clip* clip, void* scratch) {
    if (!params || !grads || !m || !v || !clip || !scratch || !clip->out4) return SPWGNN_E_ARG;
    const ParamTable& pt = param_table();
    if (n != pt.total) return SPWGNN_E_ARG;
    if (!(clip->clipnorm >= 0.f) || !(clip->clipvalue >= 0.f)) return SPWGNN_E_ARG;   // negative or NaN
    c = ClipArgs{};
    c.a = adam_args(params, grads, m, v, n, beta1, beta2, eps, l2, grad_scale);
    if (pt.total > (int64_t)kClipRounds * kClipBlocks * 256) return SPWGNN_E_SHAPE;   // k_grad_sumsq's rounds
    for (int t = 0; t < kNumTensors; ++t) c.end[t] = (int32_t)(pt.t[t].offset + (int64_t)pt.t[t].rows * pt.t[t].cols);
    c.partial = static_cast<float*>(scratch);
    c.clipnorm = clip->clipnorm;
    c.clipvalue = clip->clipvalue;
    c.skip_nonfinite = clip->skip_nonfinite ? 1 : 0;
    c.out4 = clip->out4;
    c.tot4 = clip->total4;
    return SPWGNN_OK;
}

int32_t spwgnn_adam_clipped(float* params, const float* grads, float* m, float* v, int64_t n, int32_t step, float lr,
                            float beta1, float beta2, float eps, float l2, float grad_scale, const spwgnn_clip* clip,
                            void* scratch, spwgnn_stream_t stream) {
    if (step < 1) return SPWGNN_E_ARG;
    ClipArgs c;
    if (int32_t st = clip_args(c, params, grads, m, v, n, beta1, beta2, eps, l2, grad_scale, clip, scratch)) return st;
    c.a.lr_t = adam_lr_t(lr, beta1, beta2, (double)step);
    return status(launch_adam_clipped(c, static_cast<hipStream_t>(stream)));
}

int32_t spwgnn_adam_clipped_dev(float* params, const float* grads, float* m, float* v, int64_t n,
                                const int32_t* step_dev, const float* lr_table, int32_t table_len, float beta1,
                                float beta2, float eps, float l2, float grad_scale, const spwgnn_clip* clip,
                                void* scratch, spwgnn_stream_t stream) {
    if (!step_dev || !lr_table || table_len < 2) return SPWGNN_E_ARG;
    ClipArgs c;
    if (int32_t st = clip_args(c, params, grads, m, v, n, beta1, beta2, eps, l2, grad_scale, clip, scratch)) return st;
    c.a.step_dev = step_dev;
    c.a.lr_table = lr_table;
    c.a.table_len = table_len;
    return status(launch_adam_clipped(c, static_cast<hipStream_t>(stream)));
}

int32_t spwgnn_accumulate_out3(const float* out3, const double* weights3, double* total3, spwgnn_stream_t stream) {
    if (!out3 || !weights3 || !total3) return SPWGNN_E_ARG;
    return status(launch_accumulate_out3(out3, weights3, total3, static_cast<hipStream_t>(stream)));
}

int32_t spwgnn_copy_in(const void* host, void* dev, int64_t bytes, spwgnn_stream_t stream) {
    if (!host || !dev || bytes < 0 || bytes % 16 || reinterpret_cast<uintptr_t>(host) % 16 ||
        reinterpret_cast<uintptr_t>(dev) % 16)
        return SPWGNN_E_ARG;
    if (bytes == 0) return SPWGNN_OK;
    return status(launch_copy_in(host, dev, bytes / 16, static_cast<hipStream_t>(stream)));
}

int32_t spwgnn_sigmoid(const float* logits, float* probs, int64_t n, spwgnn_stream_t stream) {
    if (!logits || !probs || n < 1) return SPWGNN_E_ARG;
    return status(launch_sigmoid(logits, probs, n, static_cast<hipStream_t>(stream)));
}

int32_t spwgnn_tower_readout(const float* logits, const int32_t* tower_offsets, int32_t n_towers, int32_t mode,
                             float* out, spwgnn_stream_t stream) {
    if (!logits || !tower_offsets || !out || n_towers < 1 || mode < SPWGNN_READOUT_SUM_PROB ||
        mode > SPWGNN_READOUT_MEAN_LOGIT)
        return SPWGNN_E_ARG;
    return status(launch_tower_readout(logits, tower_offsets, n_towers, mode, out, static_cast<hipStream_t>(stream)));
}

static_assert(SPWGNN_EVAL_BINS == kEvalBins && SPWGNN_EVAL_SIZES == kEvalSizes, "evaluation table shapes");
int32_t spwgnn_eval_metrics(const float* logits, const float* targets, int64_t n, const spwgnn_eval* ev,
                            spwgnn_stream_t stream) {
    if (int32_t stt = eval_check(logits, targets, n, ev)) return stt;
    const auto u64 = [](int64_t* t) { return reinterpret_cast<unsigned long long*>(t); };
    EvalArgs a{};
    a.logits = logits;
    a.targets = targets;
    a.w = ev->w;
    a.off = ev->tower_offsets;
    a.n = n;
    a.R = ev->rows;
    a.n_towers = ev->n_towers;
    a.tau = ev->threshold;
    a.node4 = u64(ev->node4);
    a.tower6 = u64(ev->tower6);
    a.by_size = u64(ev->by_size);
    a.hist = u64(ev->hist);
    return status(launch_eval_metrics(a, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
