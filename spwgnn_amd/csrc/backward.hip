// The backward's launch sequence: the step loop in reverse, the encoders' backwards, the weight gradients
// and their batched reduction into the flat gradient buffer.
#include <cstring>
#include "run.h"

namespace spw {

static constexpr int kW2gWgs = 256;   // W2 gradient: one workgroup per CU (MI355X: 256 CUs)
// batched weight gradients (k_wgrad_ws_batch): the jobs share one grid, so a job need not fill the chip
// by itself — a workgroup takes ≥ kWsMinStages 32-row stages (its 160×160 slab, written here and read
// by the reduction, stays small against its operands) while a job keeps ≥ kWsMinWgs workgroups
static constexpr int kWsMinStages = 32;
static constexpr int kWsMinWgs = 32;
// ... and a small job (a small batch's: fewer than kWsMinWgs·kWsSmallStages stages) gives each
// workgroup ≥ kWsSmallStages stages: every workgroup writes a whole 160×160 slab (100 KB) that the
// reduction reads back, ≈ 2.5 stages' worth of operand bytes — one stage per workgroup made the slabs
// most of the small step's weight-gradient traffic (Keras fit at batch 32: ≈ 360 slabs, 36 MB)
#ifndef SPWGNN_WS_SMALL_STAGES
#define SPWGNN_WS_SMALL_STAGES 4
#endif
static constexpr int kWsSmallStages = SPWGNN_WS_SMALL_STAGES;

// ---------------------------------------------------------------- argument structs -----------
// dstate enters the step loop as step S−1's incoming dP (NodeBwdArgs::seeded), so the loop runs once for
// Σ dlogits·z + Σ dstate·P_S; with dl_step, step s's node backward puts row s of dlogits into x' row 100
static NodeBwdArgs node_bwd_args(const Ctx& c, const spwgnn_batch* b, const Path& p, const BwdCall& call, int s) {
    const Ws& w = c.w;
    const bool first = (s == w.S - 1);
    NodeBwdArgs nb{};
    nb.n_nodes = b->n_nodes;
    nb.first = first;
    nb.seeded = first && call.dstate != nullptr;
    nb.dPin = first && !call.dstate ? nullptr : c.f(w.dP_at(s + 1));
    nb.dU = first ? nullptr : c.f(w.dU_at(s + 1));
    nb.dV = first ? nullptr : c.f(w.dV_at(s + 1));
    nb.Pn = c.f(w.P_at(s + 1));
    nb.o1 = c.f(w.o1_at(s));
    nb.a = c.f(w.a_at(s));
    nb.dlogits = (first || call.dl_step) ? call.dlogits + s * call.dl_step : nullptr;
    nb.dx = c.f(w.dx_at(s));
    nb.do1 = c.f(w.do1_at(s));
    nb.g = c.f(w.g_at(s));
    nb.G3 = c.f(w.G3_at(s));
    nb.dPout = c.f(w.dP_at(s));
    nb.dco = c.f(w.dco);
    nb.dco_accumulate = !first;
    nb.dco_sum = p.node_bwd != MATH_F32;
    nb.w1bt = c.pk(PK_W1BT); nb.w1ct = c.pk(PK_W1CT);
    nb.wo2t = c.pk(PK_WO2T);
    nb.wo1ct = c.pk(PK_WO1CT); nb.wo1at = c.pk(PK_WO1AT); nb.wo1pt = c.pk(PK_WO1PT);
    nb.w3t = c.pk(PK_W3T);
    nb.x_w1bt = c.x6(X6_W1BT); nb.xh_w1bt = c.x6(X6_W1BT_H);
    nb.x_w1ct = c.x6(X6_W1CT); nb.xh_w1ct = c.x6(X6_W1CT_H);
    nb.x_wo2t = c.x6(X6_WO2T); nb.xh_wo2t = c.x6(X6_WO2T_H);
    nb.x_wo1ct = c.x6(X6_WO1CT); nb.xh_wo1ct = c.x6(X6_WO1CT_H);
    nb.x_wo1at = c.x6(X6_WO1AT); nb.xh_wo1at = c.x6(X6_WO1AT_H);
    nb.x_wo1pt = c.x6(X6_WO1PT); nb.xh_wo1pt = c.x6(X6_WO1PT_H);
    nb.x_w3t = c.x6(X6_W3T);
    nb.n16 = p.n16;
    nb.no_dP = s == 0 && !call.dprop;   // dP_0 feeds only the dprop pass (§3zh)
    return nb;
}

// the dprop pass: dP0 = dPpart + dU·W1bᵀ + dV·W1cᵀ
static NodeBwdArgs tail_args(const Ctx& c, const spwgnn_batch* b, const Path& p, float* dprop) {
    const Ws& w = c.w;
    NodeBwdArgs tl{};
    tl.n_nodes = b->n_nodes;
    tl.tail = 1;
    tl.dPin = c.f(w.dP_at(0));
    tl.dU = c.f(w.dU_at(0));
    tl.dV = c.f(w.dV_at(0));
    tl.dprop = dprop;
    tl.w1bt = c.pk(PK_W1BT); tl.w1ct = c.pk(PK_W1CT);
    tl.x_w1bt = c.x6(X6_W1BT); tl.xh_w1bt = c.x6(X6_W1BT_H);
    tl.x_w1ct = c.x6(X6_W1CT); tl.xh_w1ct = c.x6(X6_W1CT_H);
    tl.n16 = p.n16;
    return tl;
}

// gates: step s's row of a gated call (the fused loop takes row 0 and advances it by gate_step), or null
static EdgeBwdArgs edge_bwd_args(const Ctx& c, const spwgnn_batch* b, const Path& p, int s, const float* gates = nullptr,
                                 int64_t gate_step = 0) {
    const Ws& w = c.w;
    const int k = w.S - 1 - s;   // steps S−1 .. S−n_stored keep their dh1pre (§3zi)
    EdgeBwdArgs eb{};
    eb.n_wtiles = b->n_wtiles;
    eb.nw_max = b->nw_max;
    eb.wpg = b->nw_max <= 16 ? 4 : edge_wpg(edge_bwd_lds_per_wave(b->nw_max));
    eb.dA_accumulate = s != w.S - 1;
    eb.no_dA = p.rebuild_dA;
    eb.wtile = b->wtile;
    eb.esrc = b->edge_src; eb.edst = b->edge_dst;
    eb.csr = reinterpret_cast<const uint32_t*>(b->blk_csr);
    eb.mask1 = c.u(w.m1_at(s));
    eb.mask2 = c.u(w.m2_at(s));
    eb.dh2_out = nullptr;  // the W2 gradient recomputes dh2pre (YM_DH2)
    eb.G3 = c.f(w.G3_at(s));
    eb.w2t = c.pk(PK_W2T);
    eb.x_w2t = c.x6(X6_W2T);
    eb.dA = c.f(w.dA);
    eb.dU = c.f(w.dU_at(s));
    eb.dV = c.f(w.dV_at(s));
    eb.n16 = p.n16;
    eb.dh1_slab = k < p.n_stored ? c.f(w.dz4) + k * (w.dz3 - w.dz4) : nullptr;
    eb.gather_desc = p.gd_edge_bwd;
    eb.node_bytes = (uint32_t)(eb.gather_desc ? w.RN * kRowE * 4 : 0);
    eb.gates = gates ? gates + s * gate_step : nullptr;
    eb.gate_step = gate_step;
    return eb;
}

static DaArgs da_args(const Ctx& c, const spwgnn_batch* b, const Path& p) {
    const Ws& w = c.w;
    DaArgs da{};
    da.n_eblocks = b->n_eblocks;
    da.S = w.S;
    da.g3_step = w.G3_at(1) - w.G3_at(0);
    da.m1_step = w.m1_at(1) - w.m1_at(0);
    da.m2_step = w.m2_at(1) - w.m2_at(0);
    da.edst = b->edge_dst;
    da.mask1 = c.u(w.mask1);
    da.mask2 = c.u(w.mask2);
    da.G3 = c.f(w.G3);
    da.dA = c.f(w.dA);
    da.x_w2t = c.x6(X6_W2T);
    da.b16 = p.b16;
    da.n_stored = p.n_stored;
    da.slab_step = w.dz3 - w.dz4;
    da.slab = p.n_stored ? c.f(w.dz4) : nullptr;
    return da;
}

static float dropout_scale(const spwgnn_run* r) { return (r->dropout > 0.f) ? 1.0f / (1.0f - r->dropout) : 1.0f; }

static EncEdgeBwdArgs enc_edge_bwd_args(const Ctx& c, const spwgnn_batch* b, const spwgnn_run* r, const Path& p) {
    const Ws& w = c.w;
    EncEdgeBwdArgs eeb{};
    eeb.n_eblocks = b->n_eblocks;
    eeb.b16 = p.b16;
    eeb.dA = c.f(w.dA);
    eeb.zmask = c.u(w.zmask);
    eeb.w1at = c.pk(PK_W1AT); eeb.x_w1at = c.x6(X6_W1AT);
    eeb.rm3t = c.pk(PK_RM3T); eeb.x_rm3t = c.x6(X6_RM3T);
    eeb.rm2t = c.pk(PK_RM2T); eeb.x_rm2t = c.x6(X6_RM2T);
    eeb.rm1t = c.pk(PK_RM1T); eeb.x_rm1t = c.x6(X6_RM1T);
    eeb.dz4 = c.f(w.dz4);
    eeb.dz3 = c.f(w.dz3);
    eeb.dz2 = c.f(w.dz2);
    eeb.dz1 = c.f(w.dz1);
    eeb.scale = dropout_scale(r);
    return eeb;
}

static EncNodeBwdArgs enc_node_bwd_args(const Ctx& c, const spwgnn_batch* b, const spwgnn_run* r, const Path& p) {
    const Ws& w = c.w;
    EncNodeBwdArgs enb{};
    enb.n_nodes = b->n_nodes;
    enb.dco = c.f(w.dco);
    enb.co = c.f(w.co);
    enb.zo1 = p.z1_rebuilt ? nullptr : c.f(w.zo1);
    enb.pos = b->pos;
    enb.w_om0 = c.pk(PK_OM0); enb.b_om0 = c.pk(PB_OM0);
    enb.om1t = c.pk(PK_OM1T);
    enb.do1 = c.f(w.do1_at(0));
    enb.do1_step = w.do1_at(1) - w.do1_at(0);
    enb.S = w.S;
    enb.dzo2 = c.f(w.dzo2);
    enb.dzo1 = c.f(w.dzo1);
    enb.scale = dropout_scale(r);
    if (p.node_bwd != MATH_F32) {   // dc_o = (Σ_s do1_s)·Wo1cᵀ here (NodeBwdArgs::dco_sum)
        enb.wo1ct = c.pk(PK_WO1CT);
        enb.x_wo1ct = c.x6(X6_WO1CT); enb.xh_wo1ct = c.x6(X6_WO1CT_H);
        enb.x_om1t = c.x6(X6_OM1T); enb.xh_om1t = c.x6(X6_OM1T_H);
    }
    return enb;
}

// ---------------------------------------------------------------- weight gradients -----------
// One gradient dW = Σ_rows Xᵀ·Y: the operands (a: what run_wgrad leaves is filled per launch), the Keras
// tensor rows its reduction writes, and what only the k_wgrad_ws / k_wgrad_pos3 forms take
struct WgSpec {
    WgradArgs a;
    int tk = -1, tb = -1, k_rows = 0, k_row0 = 0, bias_row = -1, perm = 0;   // reduce target
    bool recompute = false;   // XM_H1 / YM_DH2: the W2 gradient
    int b16 = 0;              // kB16X / kB16Y: bf16-stored operands (bf16 math, Path::b16 / n16)
    bool skip0 = false;       // k_wgrad_ws: step 0's X rows are exactly zero — its stages are left out
    const float2* xd = nullptr;          // z1 rebuilt from d (k_wgrad_ws XD 1)
    const float4* xp = nullptr;          // zo1 rebuilt from the node positions (XD 2)
    const float *w0 = nullptr, *b0 = nullptr;
    WgSpec() {
        memset(&a, 0, sizeof a);   // it travels as a kernel argument: every byte defined, padding included
        a.x_ones = -1;
        a.x_count = a.y_count = 1;
    }
};

// What the weight gradients of one backward share. Each gradient writes its per-chunk slabs into its own
// slot (its index in rb); the ordered chunk sums of all of them run as one batched launch (reduce).
struct WgRun {
    const Ctx& c;
    const spwgnn_batch* b;
    const Path& p;
    hipStream_t st;
    const Prof& prof;
    float* grads;
    const float* gates;   // a gated call's relation gates (the W2 gradient's Y rows carry them), or null
    int64_t gate_step;    // ... a row per step (§3zzc), or 0
    WsBatch* wsb;      // the batched k_wgrad_ws launch being filled (null: one launch per gradient)
    ReduceBatch& rb;   // every gradient's reduction
    Pos3Batch& p3;     // the rm.0 / om.0 gradients (k_wgrad_pos3)
};

static int32_t run_wgrad(WgRun& q, const WgSpec& g) {
    const Ws& w = q.c.w;
    const Path& p = q.p;
    const int math = p.wgrad;
    WgradArgs a = g.a;
    if (a.rows <= 0) return SPWGNN_OK;
    if (q.rb.n >= kWgSlots) return SPWGNN_E_ARG;
    float* const slab = q.c.f(w.slab) + (int64_t)q.rb.n * w.slot_floats;
    // the row-chunked kernels: chunks of ≥ 512 rows, but at least one per CU (256) while a chunk
    // keeps ≥ one 32-row block — small batches spread over the chip instead of walking a few
    // chunks serially; at most 1024 chunks and what the slot holds
    const int64_t slot_chunks = w.slot_floats / ((int64_t)a.kx_pad * a.ny_pad);
    int64_t chunks = std::max<int64_t>((a.rows + 32 * 16 - 1) / (32 * 16), std::min<int64_t>((a.rows + 31) / 32, 256));
    chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, std::min<int64_t>(1024, slot_chunks)));
    a.rows_per_chunk = up((a.rows + chunks - 1) / chunks, 32);
    chunks = (a.rows + a.rows_per_chunk - 1) / a.rows_per_chunk;
    a.pos = q.b->pos;
    a.esrc = q.b->edge_src;
    a.edst = q.b->edge_dst;
    a.slab = slab;
    if (g.recompute) {
        a.A = q.c.f(w.A);
        a.U = q.c.f(w.U);
        a.V = q.c.f(w.V);
        a.G3 = q.c.f(w.G3);
        a.mask2 = q.c.u(w.mask2);
        a.RE = w.RE;
        a.RN = w.RN;
        a.S = (int)(a.rows / w.RE);
        a.a_b16 = (g.b16 & kB16A) != 0;
        a.uv16 = (g.b16 & kB16UV) != 0;
        a.wtile = q.b->wtile;
        a.n_wtiles = q.b->n_wtiles;
        a.nw_max = q.b->nw_max;
        a.w2_tile = !p.diag.w2g_gather;
        a.gather_desc = p.gd_w2;
        a.gates = q.gates;
        a.gate_step = q.gate_step;
    }
    // stored chunk-major operands in x6 math: the warp-specialized kernel, one workgroup per CU
    if (math != MATH_F32 && a.xmode == XM_CM && (a.ymode == YM_CM || a.ymode == YM_ROW) && !p.diag.wg_old) {
        WgWsArgs wa{};
        wa.x = a.x_ptr;
        wa.y = a.y_ptr;
        wa.slab = slab;
        wa.count = a.x_count;
        wa.S = a.rows / a.x_count;
        wa.nbs = (a.x_count + 31) / 32;
        wa.x_sb = a.x_stride / 32;
        wa.y_sb = a.y_stride / 32;
        wa.x_ones = a.x_ones;
        wa.xd = g.xd;
        wa.xp = g.xp;
        wa.w0 = g.w0;
        wa.b0 = g.b0;
        wa.skip0 = g.skip0;   // the partition below is that of all S steps either way (same chunk sums)
        const int64_t nst = wa.nbs * wa.S;
        int64_t wgs = std::min<int64_t>(nst, kW2gWgs);
        if (q.wsb) {
            wgs = std::min<int64_t>(wgs, std::max<int64_t>(kWsMinWgs, (nst + kWsMinStages - 1) / kWsMinStages));
            wgs = std::min<int64_t>(wgs, (nst + kWsSmallStages - 1) / kWsSmallStages);
        }
        wa.stages_per_wg = (nst + wgs - 1) / wgs;
        wgs = (nst + wa.stages_per_wg - 1) / wa.stages_per_wg;
        chunks = wgs;
        const bool yrow = a.ymode == YM_ROW;
        const bool mask = !(a.kx_pad == 160 && a.ny_pad == 160);   // node arrays: rows ≥ count masked
        if (q.wsb) {   // queued: every k_wgrad_ws gradient of the backward runs in one launch
            const int v = wgrad_ws_variant(wa, a.kx_pad, a.ny_pad, yrow, mask, math, g.b16);
            if (v == WSV_NONE || q.wsb->n >= kMaxWsJobs) return SPWGNN_E_ARG;
            WsJob& j = q.wsb->j[q.wsb->n++];
            j.a = wa;
            j.variant = v;
            j.wg0 = q.wsb->wgs;
            j.gn = j.gi = 0;
            q.wsb->wgs += (int)wgs;
        } else {
            SPW_TIMED(q.prof, SPWGNN_K_WGRAD_WS,
                      launch_wgrad_ws(wa, (int)wgs, a.kx_pad, a.ny_pad, yrow, mask, math, q.st, g.b16));
        }
    } else if (math != MATH_F32 && (a.xmode == XM_NODE_O || (a.xmode == XM_EDGE_D && g.xd))) {
        // the 3-column first-layer gradients: a vector-ALU stream over Y (k_wgrad_pos3)
        Pos3Args pa{};
        pa.y = a.y_ptr;
        pa.pos = reinterpret_cast<const float4*>(q.b->pos);
        pa.ed = g.xd;
        pa.esrc = q.b->edge_src;
        pa.slab = slab;
        pa.count = a.rows;
        pa.nblk = (a.rows + 31) / 32;
        const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(pa.nblk, std::min<int64_t>(512, slot_chunks)));
        pa.blk_per_wg = (pa.nblk + wgs - 1) / wgs;
        chunks = (pa.nblk + pa.blk_per_wg - 1) / pa.blk_per_wg;
        if (a.xmode == XM_NODE_O) { q.p3.n = pa; q.p3.cn = (int)chunks; }
        else { q.p3.e = pa; q.p3.ce = (int)chunks; q.p3.b16e = (g.b16 & kB16Y) != 0; }
    } else {
        // the x6 W2 gradient: one warp-specialized workgroup per CU over contiguous edge-block ranges
        const bool ws = g.recompute && math != MATH_F32 && (math == MATH_BF16 || !p.diag.w2g_old);
        int64_t bpw = 0;
        if (ws) {
            const int64_t nblk = w.RE / 32;
            const int64_t wgs = std::min<int64_t>(nblk, kW2gWgs);
            bpw = (nblk + wgs - 1) / wgs;
            chunks = (nblk + bpw - 1) / bpw;
        }
        // a small x6 batch: the W2 gradient runs inside the batched weight-gradient launch
        // (the copy in the batched launch is the descriptor form: the pointer form runs as its own launch)
        // (a gated call's too: k_w2grad_ws<…, GATE> is the pointer form)
        const bool w2_in_batch = ws && math_split32(math) && q.wsb && p.team_edges && a.gather_desc && !a.gates &&
                                 !p.diag.no_w2_merge;
        const bool timed = g.recompute && !w2_in_batch;
        if (timed) SPW_CHECK(q.prof.before(SPWGNN_K_WGRAD_W2));
        if (w2_in_batch) {
            q.wsb->w2 = a;
            q.wsb->w2_bpw = bpw;
            q.wsb->w2_wgs = (int)chunks;
        } else if (ws)
            SPW_CHECK(launch_w2grad_ws(a, (int)chunks, bpw, math, q.st));
        else if (math == MATH_BF16)
            SPW_CHECK(launch_wgrad_bf16(a, (int)chunks, q.st, g.b16));
        else if (g.b16)
            return SPWGNN_E_ARG;
        else
            SPW_CHECK(launch_wgrad(a, (int)chunks, math, q.st));
        if (timed) SPW_CHECK(q.prof.after(SPWGNN_K_WGRAD_W2));
    }
    const ParamTable& pt = param_table();
    ReduceArgs& ra = q.rb.r[q.rb.n++];
    ra = ReduceArgs{};
    ra.slab = slab;
    ra.chunks = (int)chunks;
    ra.kx_pad = a.kx_pad;
    ra.ny_pad = a.ny_pad;
    ra.out = q.grads;
    ra.kernel_off = g.tk >= 0 ? pt.t[g.tk].offset : -1;
    ra.kernel_rows = g.k_rows;
    ra.kernel_cols = g.tk >= 0 ? pt.t[g.tk].cols : pt.t[g.tb].cols;
    ra.kernel_row0 = g.k_row0;
    ra.bias_off = g.tb >= 0 ? pt.t[g.tb].offset : -1;
    ra.bias_row = g.bias_row;
    ra.perm = g.perm;
    return SPWGNN_OK;
}

// Jobs [first, first + n) of the batch read one operand in common (the node rows P / do1): run them
// as an interleaved group (k_wgrad_ws_batch) when their row ranges match — the same workgroup count,
// a multiple of the 8 XCDs, over the same stage partition; otherwise they stay in sequence.
static void ws_group(WsBatch* wsb, int first, int n) {
    if (!wsb || n < 2 || first < 0 || first + n > wsb->n) return;
    const WsJob& j0 = wsb->j[first];
    const int w0 = (first + 1 < wsb->n ? wsb->j[first + 1].wg0 : wsb->wgs) - j0.wg0;
    if (w0 <= 0 || w0 % 8) return;
    for (int i = 1; i < n; ++i) {
        const WsJob& ji = wsb->j[first + i];
        const int wi = (first + i + 1 < wsb->n ? wsb->j[first + i + 1].wg0 : wsb->wgs) - ji.wg0;
        if (wi != w0 || ji.a.stages_per_wg != j0.a.stages_per_wg || ji.a.nbs != j0.a.nbs || ji.a.S != j0.a.S) return;
    }
    for (int i = 0; i < n; ++i) {
        wsb->j[first + i].gn = n;
        wsb->j[first + i].gi = i;
    }
}

// an encoder layer over all RE edge rows: X and Y at workspace offsets, [kFE | 1] × kFE
static WgSpec edge_job(const Ctx& c, int64_t xoff, int64_t yoff, int xmode, int ymode, int tk, int tb) {
    WgSpec g;
    WgradArgs& a = g.a;
    a.xmode = xmode; a.ymode = ymode;
    a.x_ptr = c.f(xoff); a.x_ld = kLdE; a.x_width = kFE; a.x_ones = kFE; a.x_count = c.w.RE; a.x_stride = 0;
    a.y_ptr = c.f(yoff); a.y_ld = kLdE; a.y_width = kFE; a.y_count = c.w.RE; a.y_stride = 0;
    a.rows = c.w.RE; a.kx_pad = 160; a.ny_pad = 160;
    g.tk = tk; g.tb = tb; g.k_rows = kFE; g.k_row0 = 0; g.bias_row = kFE;
    return g;
}
// chunk-major node rows over all S steps (X step stride xstride: 0 = one array for every step); an array's
// row stride is its padded width (kLdN = 128, kLdE = 160)
static WgSpec node_job(const Ctx& c, int64_t nN, int64_t xoff, int xw, int xones, int64_t xstride, int kxp, int64_t yoff,
                       int yw, int nyp) {
    WgSpec g;
    WgradArgs& a = g.a;
    a.xmode = XM_CM; a.ymode = YM_CM;
    a.x_ptr = c.f(xoff); a.x_ld = kxp; a.x_width = xw; a.x_ones = xones; a.x_count = nN; a.x_stride = xstride;
    a.y_ptr = c.f(yoff); a.y_ld = nyp; a.y_width = yw; a.y_count = nN; a.y_stride = c.w.RN;
    a.rows = nN * c.w.S; a.kx_pad = kxp; a.ny_pad = nyp;
    return g;
}
static void target(WgSpec& g, int tk, int tb, int k_rows, int k_row0, int bias_row) {
    g.tk = tk; g.tb = tb; g.k_rows = k_rows; g.k_row0 = k_row0; g.bias_row = bias_row;
}

// the 3-column first layers, Y chunk-major and nyp wide: X = [d | 1] per edge (rm.0), [y, w | 1] per node (om.0)
static WgSpec first_layer_job(const Ctx& c, int xmode, int64_t rows, int64_t yoff, int yw, int nyp, int tk, int tb) {
    WgSpec g;
    g.a.xmode = xmode; g.a.ymode = YM_CM; g.a.kx_pad = 32; g.a.ny_pad = nyp; g.a.rows = rows;
    g.a.y_ptr = c.f(yoff); g.a.y_ld = nyp; g.a.y_width = yw; g.a.y_count = rows;
    target(g, tk, tb, 2, 0, 2);
    return g;
}
static int32_t wg_rm0(WgRun& q) {
    WgSpec g = first_layer_job(q.c, XM_EDGE_D, q.c.w.RE, q.c.w.dz1, kFE, 160, T_RM0K, T_RM0B);
    g.b16 = q.p.b16 ? kB16Y : 0;   // Y = dz1
    if (q.p.z1_rebuilt) g.xd = reinterpret_cast<const float2*>(q.c.f(q.c.w.ed));   // k_wgrad_pos3 reads d
    return run_wgrad(q, g);
}
static int32_t wg_om0(WgRun& q) {
    return run_wgrad(q, first_layer_job(q.c, XM_NODE_O, q.b->n_nodes, q.c.w.dzo1, kFN, 128, T_OM0K, T_OM0B));
}
// encoder layers: chunk-major activations and gradients; W1a: X = c_r (chunk-major), Y = dA (rows)
static int32_t wg_encoder(WgRun& q) {
    const Ctx& c = q.c;
    const Ws& w = c.w;
    const int b16y = q.p.b16 ? kB16Y : 0, b16xy = q.p.b16 ? (kB16X | kB16Y) : 0;
    WgSpec rm1 = edge_job(c, w.z1, w.dz2, XM_CM, YM_CM, T_RM1K, T_RM1B);
    if (q.p.z1_rebuilt) {
        rm1.xd = reinterpret_cast<const float2*>(c.f(w.ed));
        rm1.w0 = c.pk(PK_RM0);
        rm1.b0 = c.pk(PB_RM0);
    }
    rm1.b16 = b16y;   // X rebuilt from d; Y = dz2
    WgSpec rm2 = edge_job(c, w.z2, w.dz3, XM_CM, YM_CM, T_RM2K, T_RM2B);
    WgSpec rm3 = edge_job(c, w.z3, w.dz4, XM_CM, YM_CM, T_RM3K, T_RM3B);
    WgSpec w1a = edge_job(c, w.cr, w.dA, XM_CM, YM_ROW, T_RMP0K, T_RMP0B);
    rm2.b16 = rm3.b16 = w1a.b16 = b16xy;
    for (const WgSpec* g : {&rm1, &rm2, &rm3, &w1a})
        if (int32_t e = run_wgrad(q, *g)) return e;
    return SPWGNN_OK;
}
// rmp.1 (W2, b2): X = [h1 | 1], Y = dh2pre, both recomputed from the chunk-major A and node rows (U, V, G3)
// and the h2>0 mask, over all steps (row = s·RE + e)
static int32_t wg_w2(WgRun& q) {
    WgSpec g = edge_job(q.c, -1, -1, XM_H1, YM_DH2, T_RMP1K, T_RMP1B);
    g.a.x_count = g.a.y_count = g.a.rows = q.c.w.RE * q.c.w.S;
    g.recompute = true;
    g.b16 = (q.p.b16 ? kB16A : 0) | (q.p.n16 ? kB16UV : 0);   // U, V rows as the forward stored them (Path::uv16)
    g.a.uv_zero = !q.b->prop;
    return run_wgrad(q, g);
}
static int32_t wg_node(WgRun& q) {
    const Ctx& c = q.c;
    const Ws& w = c.w;
    const Path& p = q.p;
    const int64_t nN = q.b->n_nodes, RN = w.RN;
    const int n16y = p.n16 ? kB16Y : 0, n16xy = p.n16 ? (kB16X | kB16Y) : 0;
    // W1b, W1c, omp.0 P part (X = P), omp.0 effect part (Y = do1): one group
    WgSpec w1b = node_job(c, nN, w.P, kFN, -1, RN, 128, w.dU, kFE, 160);   // rmp.0 rows 150..249: Σ_s P_sᵀ dU_s
    target(w1b, T_RMP0K, -1, kFN, 150, -1);
    WgSpec w1c = node_job(c, nN, w.P, kFN, -1, RN, 128, w.dV, kFE, 160);   // rmp.0 rows 250..349
    target(w1c, T_RMP0K, -1, kFN, 250, -1);
    w1b.b16 = w1c.b16 = n16y;
    WgSpec o0p = node_job(c, nN, w.P, kFN, -1, RN, 128, w.do1, kFN, 128);   // omp.0 rows 200..299 (P part)
    target(o0p, T_OMP0K, -1, kFN, 200, -1);
    w1b.skip0 = w1c.skip0 = o0p.skip0 = p.ws_skip0;
    WgSpec o0a = node_job(c, nN, w.a, kFN, -1, RN, 128, w.do1, kFN, 128);   // omp.0 rows 100..199 (effect part)
    target(o0a, T_OMP0K, -1, kFN, 100, -1);
    WgSpec w3 = node_job(c, nN, w.H2s, kFE + 1, -1, RN, 160, w.g, kFN, 128);   // rmp.2 (W3, b3): X = [H2s | deg]
    target(w3, T_RMP2K, T_RMP2B, kFE, 0, kDegCol);
    // omp.0 rows 0..99 (c_o part, broadcast over steps) + bias
    WgSpec o0c = node_job(c, nN, w.co, kFN, kFN, 0, 128, w.do1, kFN, 128);
    target(o0c, T_OMP0K, T_OMP0B, kFN, 0, kFN);
    if (p.node_bwd != MATH_F32) {   // c_oᵀ·Σ_s do1_s: Σ do1 stored by k_enc_node_bwd
        o0c.a.y_ptr = c.f(w.dco);
        o0c.a.rows = nN;
        o0c.a.y_stride = 0;
    }
    WgSpec o1 = node_job(c, nN, w.o1, kFN, kFN, RN, 128, w.dx, kFN + 1, 128);   // omp.1 (Wo2, bo2), x' column order → Keras order
    target(o1, T_OMP1K, T_OMP1B, kFN, 0, kFN);
    o1.perm = 1;
    w3.b16 = o1.b16 = n16xy;
    const int grp0 = q.wsb ? q.wsb->n : 0;
    for (const WgSpec* g : {&w1b, &w1c, &o0p, &o0a})
        if (int32_t e = run_wgrad(q, *g)) return e;
    if (q.wsb && !p.diag.ws_nogroup) ws_group(q.wsb, grp0, q.wsb->n - grp0);
    for (const WgSpec* g : {&w3, &o0c, &o1})
        if (int32_t e = run_wgrad(q, *g)) return e;
    return SPWGNN_OK;
}
static int32_t wg_om1(WgRun& q) {   // om.1
    const Ctx& c = q.c;
    WgSpec g = node_job(c, q.b->n_nodes, c.w.zo1, kFN, kFN, 0, 128, c.w.dzo2, kFN, 128);
    g.a.rows = q.b->n_nodes; g.a.y_stride = 0;
    if (q.p.z1_rebuilt) {
        g.xp = reinterpret_cast<const float4*>(q.b->pos);
        g.w0 = c.pk(PK_OM0);
        g.b0 = c.pk(PB_OM0);
    }
    target(g, T_OM1K, T_OM1B, kFN, 0, kFN);
    return run_wgrad(q, g);
}

// the batched launch of `batch` (+ a small batch's rm.0 / om.0 gradients as trailing workgroups)
static int32_t launch_ws(WgRun& q, const WsBatch& batch, bool with_p3) {
    const bool any = batch.n > 0 || batch.w2_wgs > 0;
    const bool p3_in_batch = with_p3 && any && q.p.team_edges && !q.p.diag.no_pos3_merge;
    if (with_p3 && !p3_in_batch) SPW_CHECK(launch_wgrad_pos3(q.p3, q.st));
    if (any)
        SPW_TIMED(q.prof, SPWGNN_K_WGRAD_WS, launch_wgrad_ws_batch(batch, q.p.wgrad, q.st, p3_in_batch ? &q.p3 : nullptr));
    return SPWGNN_OK;
}

// The reductions of the gradients whose tensors lie in [t_lo, t_hi), and the zeroing of the float ranges
// of those tensors no such reduction writes: the reductions write the 22 Keras tensors' elements, not
// every float of the flat buffer, and the remaining ranges (alignment gaps, uncovered tensor rows) are
// zeroed by the same launch (tests/test_gpu_parity.py::test_backward_writes_every_gradient). More ranges
// than the launch carries (kMaxZero) or no reduction: one memset of those tensors instead (stream-ordered
// before the reduction, which then writes its ranges). loss: the unweighted loss sums as one more row.
static int32_t reduce(const ReduceBatch& rb, int t_lo, int t_hi, const BceArgs* loss, float* grads, hipStream_t st) {
    const ParamTable& pt = param_table();
    const int64_t lo = pt.t[t_lo].offset, hi = t_hi < kNumTensors ? pt.t[t_hi].offset : pt.total;
    ReduceBatch sub{};
    if (loss) {
        sub.bce_row = 1;
        sub.bce = *loss;
        sub.bce.dlogits = nullptr;   // written by the step loop
    }
    for (int k = 0; k < rb.n; ++k) {
        const int64_t off = rb.r[k].kernel_off >= 0 ? rb.r[k].kernel_off : rb.r[k].bias_off;
        if (off >= lo && off < hi) sub.r[sub.n++] = rb.r[k];
    }
    bool overflow = false;
    auto zero = [&](int64_t off, int64_t len) {
        if (len <= 0) return;
        if (sub.nzero > 0 && sub.zoff[sub.nzero - 1] + sub.zlen[sub.nzero - 1] == off) {   // merge
            sub.zlen[sub.nzero - 1] += (int32_t)len;
        } else if (sub.nzero < kMaxZero) {
            sub.zoff[sub.nzero] = off;
            sub.zlen[sub.nzero++] = (int32_t)len;
        } else {
            overflow = true;
        }
    };
    constexpr int kMaxRows = 512;   // the largest Keras tensor has 350 rows (rmp.0 kernel)
    uint8_t row[kMaxRows];
    for (int t = t_lo; t < t_hi && !overflow; ++t) {
        const TensorDesc& d = pt.t[t];
        if (d.rows > kMaxRows) return SPWGNN_E_ARG;
        const int64_t end = t + 1 < kNumTensors ? pt.t[t + 1].offset : pt.total;
        memset(row, 0, d.rows);   // rows (kernels) or the one bias row written by some job
        for (int k = 0; k < sub.n; ++k) {
            const ReduceArgs& ra = sub.r[k];
            if (d.rows > 1 && ra.kernel_off == d.offset)
                for (int q = 0; q < ra.kernel_rows; ++q)
                    if (ra.kernel_row0 + q < d.rows) row[ra.kernel_row0 + q] = 1;
            if (d.rows == 1 && ra.bias_off == d.offset) row[0] = 1;
        }
        for (int q = 0; q < d.rows; ++q)
            if (!row[q]) zero(d.offset + (int64_t)q * d.cols, d.cols);
        zero(d.offset + (int64_t)d.rows * d.cols, end - d.offset - (int64_t)d.rows * d.cols);
    }
    if (overflow || (sub.n == 0 && sub.nzero > 0)) {
        SPW_CHECK(hipMemsetAsync(grads + lo, 0, (hi - lo) * sizeof(float), st));
        sub.nzero = 0;
    }
    SPW_CHECK(launch_wgrad_reduce_all(sub, st));
    return SPWGNN_OK;
}

// ---------------------------------------------------------------- the sequence ---------------
// the packed weights are the copies the forward made on this workspace
int32_t run_backward(const spwgnn_batch* b, const spwgnn_run* r, const Ws& w, char* base, const BwdCall& call,
                     hipStream_t st) {
    const Ctx c{w, base, r->math != MATH_F32};
    const Path p = make_path(b, r, w, &call);
    const int S = r->mp_steps;
    const Prof prof{r, st};
    NodeBwdArgs tl{};   // all zero without a dprop request / without the dA rebuild (the fused launch carries them)
    if (call.dprop) tl = tail_args(c, b, p, call.dprop);
    DaArgs da{};
    if (p.rebuild_dA) da = da_args(c, b, p);
    da.gates = call.gates;
    da.gate_step = call.gate_step;
    const EncEdgeBwdArgs eeb = enc_edge_bwd_args(c, b, r, p);
    const EncNodeBwdArgs enb = enc_node_bwd_args(c, b, r, p);

    // spwgnn_bce_backward: anywhere but on the fused loop (Path::bce_inline) the loss launch runs first
    if (call.bce && !p.bce_inline) SPW_CHECK(launch_bce(*call.bce, st));
    if (call.dstate)   // dP_S ← dstate, chunk-major (the slot step S−2's node backward overwrites)
        SPW_TIMED(prof, SPWGNN_K_STATE, launch_state_import(call.dstate, c.f(w.dP_at(S)), b->n_nodes, st));
    auto edge_encoder_bwd = [&]() -> int32_t {   // dA rebuild + relation encoder backward (wide kernels)
        if (p.rebuild_dA) SPW_TIMED(prof, SPWGNN_K_DA, launch_dA(da, p.edge_bwd, st));
        SPW_TIMED(prof, SPWGNN_K_ENC_EDGE_BWD, launch_enc_edge_bwd(eeb, p.enc_edge_bwd, st));
        return SPWGNN_OK;
    };
    if (p.bwd_fused) {
        // small batch: the step loop, dA and both encoder backwards in one launch (timed as the node backward)
        BwdFusedArgs fa{};
        fa.nb = node_bwd_args(c, b, p, call, 0);
        fa.nb.dlogits = call.dlogits;            // row 0; the loop forms each step's own from dl_step
        fa.dl_step = call.dl_step;
        fa.nb.seeded = call.dstate != nullptr;   // step S−1's (the loop sets each step's own)
        fa.nb.dU = c.f(w.dU_at(1));   // step 0's incoming dU/dV (BwdFusedArgs)
        fa.nb.dV = c.f(w.dV_at(1));
        if (p.bce_inline) {
            fa.nb.bce_logits = call.bce->logits;
            fa.nb.bce_targets = call.bce->targets;
            fa.nb.bce_dlogits = call.bce->dlogits;
            fa.nb.bce_n = call.bce->n;
        }
        fa.tail = tl;
        fa.has_tail = call.dprop != nullptr;
        fa.eb = edge_bwd_args(c, b, p, 0, call.gates, call.gate_step);
        fa.da = da;
        fa.eeb = eeb;
        fa.enb = enb;
        fa.S = S;
        fa.rowsN = w.RN * kRowN;
        fa.rowsE = w.RN * kRowE;
        fa.m1_step = w.m1_at(1) - w.m1_at(0);
        fa.m2_step = w.m2_at(1) - w.m2_at(0);
        fa.encoders = p.diag.fused_enc;
        fa.dA_in_loop = !p.diag.da_pair;
        SPW_TIMED(prof, SPWGNN_K_NODE_BWD, launch_bwd_fused_team(fa, math_bwd(r->math), st));
        if (!fa.encoders)
            SPW_TIMED(prof, SPWGNN_K_ENC_EDGE_BWD,
                      launch_bwd_enc_pair_team(da, eeb, enb, math_bwd(r->math), !fa.dA_in_loop, st));
    } else {
        for (int s = S - 1; s >= 0; --s) {
            SPW_TIMED(prof, SPWGNN_K_NODE_BWD,
                      launch_node_bwd(node_bwd_args(c, b, p, call, s), p.node_bwd, st, call.dl_step != 0));
            if (s == 0 && p.skip_eb0) break;   // dU_0 / dV_0 stay unwritten: nothing reads them
            SPW_TIMED(prof, SPWGNN_K_EDGE_BWD, launch_edge_bwd(edge_bwd_args(c, b, p, s, call.gates, call.gate_step), p.edge_bwd, st));
        }
        if (call.dprop) SPW_CHECK(launch_node_bwd(tl, p.node_bwd, st));
        if (!p.split)
            if (int32_t e = edge_encoder_bwd()) return e;
        SPW_TIMED(prof, SPWGNN_K_ENC_NODE_BWD, launch_enc_node_bwd(enb, p.node_bwd, st));
    }

    // ---- weight gradients: every k_wgrad_ws job in one batched launch, every reduction in one launch ----
    WsBatch wsb{}, wsb2{};   // (split: the early group's, then the late group's)
    ReduceBatch rb{};
    Pos3Batch p3{};
    WgRun q{c, b, p, st, prof, call.grads, call.gates, call.gate_step, p.diag.ws_unbatched ? nullptr : &wsb, rb, p3};
    const BceArgs* const loss_row = p.bce_inline ? call.bce : nullptr;   // rides in the last reduction
    int32_t e = SPWGNN_OK;
    if (!p.split) {
        if ((e = wg_rm0(q)) || (e = wg_encoder(q)) || (e = wg_w2(q)) || (e = wg_node(q)) || (e = wg_om0(q)) ||
            (e = wg_om1(q)) || (e = launch_ws(q, wsb, true)))
            return e;
        return reduce(rb, 0, kNumTensors, loss_row, call.grads, st);
    }
    // two groups (spwgnn_run.grads_early_event): the node-side and W2 / W3 gradients need only the step loop
    // and the node encoder's backward (Σ do1, dzo2); then the event, dA, the relation encoder's backward
    // and the encoder-side gradients
    if ((e = wg_w2(q)) || (e = wg_node(q)) || (e = wg_om1(q)) || (e = launch_ws(q, wsb, false)) ||
        (e = reduce(rb, T_RMP1K, kNumTensors, nullptr, call.grads, st)))
        return e;
    SPW_CHECK(hipEventRecord(static_cast<hipEvent_t>(r->grads_early_event), st));
    if (!p.bwd_fused && (e = edge_encoder_bwd())) return e;
    if (q.wsb) q.wsb = &wsb2;
    if ((e = wg_rm0(q)) || (e = wg_om0(q)) || (e = wg_encoder(q)) || (e = launch_ws(q, wsb2, true))) return e;
    return reduce(rb, 0, T_RMP1K, loss_row, call.grads, st);
}

}  // namespace spw
