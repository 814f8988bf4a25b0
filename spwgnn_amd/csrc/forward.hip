// The forward's launch sequence: weight packs, encoders, S propagation steps.
#include <cmath>
#include "run.h"

namespace spw {

// packs and, for the split-bf16 maths, the x6 images: one launch (one of the ≈ 20 of a small step), which
// also runs a replayed step's first work (spwgnn_run.prologue)
static int32_t prep(const Ctx& c, const float* params, const spwgnn_run* r, hipStream_t st) {
    PrepArgs pa{};
    pa.params = params;
    pa.pk = c.f(c.w.pk);
    build_packs(c.w.ps, pa.desc);
    PrepX6Args xa{};
    if (c.images) {
        xa.img = reinterpret_cast<uint4*>(c.f(c.w.x6));
        build_x6(r->math, c.w.x6off, xa);
    }
    if (const spwgnn_prologue* p = r->prologue) {
        if (p->copy_bytes < 0 || p->copy_bytes % 16 || (p->copy_bytes && (!p->copy_src || !p->copy_dst)) ||
            reinterpret_cast<uintptr_t>(p->copy_src) % 16 || reinterpret_cast<uintptr_t>(p->copy_dst) % 16 ||
            (p->key && (!p->step || p->mode < SPWGNN_STEP_KEY_COUNTER || p->mode > SPWGNN_STEP_KEY_SPLITMIX)))
            return SPWGNN_E_ARG;
        pa.pro = {static_cast<const uint4*>(p->copy_src), static_cast<uint4*>(p->copy_dst), p->copy_bytes / 16,
                  p->key, p->step, p->mode, p->rank, p->seed};
        pa.pro_row = 1;
    }
    SPW_CHECK(launch_prep(pa, c.images ? &xa : nullptr, st));
    return SPWGNN_OK;
}

template <class Args>
static void set_dropout(Args& a, const spwgnn_run* r) {
    a.dropout_on = r->training && r->dropout > 0.f;
    a.thresh = (uint32_t)std::min(4294967295.0, std::floor((double)r->dropout * 4294967296.0));
    a.scale = a.dropout_on ? 1.0f / (1.0f - r->dropout) : 1.0f;
    a.seed = r->seed;
    a.seed_dev = r->seed_dev;
}

static EncNodeArgs enc_node_args(const Ctx& c, const spwgnn_batch* b, const spwgnn_run* r, const Path& p) {
    const Ws& w = c.w;
    EncNodeArgs en{};
    en.n_nodes = b->n_nodes;
    en.pos = b->pos;
    en.prop = b->prop;
    en.node_tower = b->node_tower;
    en.node_local = b->node_local;
    en.w_om0 = c.pk(PK_OM0); en.b_om0 = c.pk(PB_OM0);
    en.w_om1 = c.pk(PK_OM1); en.b_om1 = c.pk(PB_OM1);
    en.w1b = c.pk(PK_W1B); en.w1c = c.pk(PK_W1C);
    en.x_om1 = c.x6(X6_OM1); en.xh_om1 = c.x6(X6_OM1_H);
    en.x_w1b = c.x6(X6_W1B); en.x_w1c = c.x6(X6_W1C);
    en.zo1 = p.z1_rebuilt ? nullptr : c.f(w.zo1);
    en.co = c.f(w.co);
    en.P0 = c.f(w.P_at(0));
    en.U0 = c.f(w.U_at(0));
    en.V0 = c.f(w.V_at(0));
    en.uv16 = p.uv16;
    en.store_p0 = !(!b->prop && p.wide_node_side);   // the zero P0 rows have no reader there (§3zh)
    set_dropout(en, r);
    return en;
}

static EncEdgeArgs enc_edge_args(const Ctx& c, const spwgnn_batch* b, const spwgnn_run* r, const Path& p) {
    const Ws& w = c.w;
    EncEdgeArgs ee{};
    ee.n_eblocks = b->n_eblocks;
    ee.pos = b->pos;
    ee.esrc = b->edge_src; ee.edst = b->edge_dst;
    ee.node_tower = b->node_tower;
    ee.node_local = b->node_local;
    ee.w_rm0 = c.pk(PK_RM0); ee.b_rm0 = c.pk(PB_RM0);
    ee.w_rm1 = c.pk(PK_RM1); ee.b_rm1 = c.pk(PB_RM1);
    ee.w_rm2 = c.pk(PK_RM2); ee.b_rm2 = c.pk(PB_RM2);
    ee.w_rm3 = c.pk(PK_RM3); ee.b_rm3 = c.pk(PB_RM3);
    ee.w_w1a = c.pk(PK_W1A); ee.b_w1a = c.pk(PB_W1A);
    ee.x_rm1 = c.x6(X6_RM1); ee.x_rm2 = c.x6(X6_RM2);
    ee.x_rm3 = c.x6(X6_RM3); ee.x_w1a = c.x6(X6_W1A);
    ee.z1 = p.z1_rebuilt ? nullptr : c.f(w.z1);
    ee.ed = p.z1_rebuilt ? reinterpret_cast<float2*>(c.f(w.ed)) : nullptr;
    ee.z2 = c.f(w.z2);
    ee.z3 = c.f(w.z3);
    ee.cr = c.f(w.cr);
    ee.A = c.f(w.A);
    ee.zmask = c.u(w.zmask);
    ee.b16 = p.b16;
    set_dropout(ee, r);
    return ee;
}

// gates: step s's row of a gated call (the fused loop takes row 0 and advances it by gate_step), or null
static EdgeFwdArgs edge_fwd_args(const Ctx& c, const spwgnn_batch* b, const Path& p, int s, const float* gates = nullptr,
                                 int64_t gate_step = 0) {
    const Ws& w = c.w;
    EdgeFwdArgs ef{};
    ef.n_wtiles = b->n_wtiles;
    ef.nw_max = b->nw_max;
    ef.wpg = 4;
    ef.wtile = b->wtile;
    ef.esrc = b->edge_src; ef.edst = b->edge_dst;
    ef.csr = reinterpret_cast<const uint32_t*>(b->blk_csr);
    ef.A = c.f(w.A);
    ef.U = c.f(w.U_at(s));
    ef.V = c.f(w.V_at(s));
    ef.w2 = c.pk(PK_W2); ef.b2 = c.pk(PB_W2);
    ef.x_w2 = c.x6(X6_W2);
    ef.H2s = c.f(w.H2s_at(s));
    ef.mask1 = w.training ? c.u(w.m1_at(s)) : nullptr;
    ef.mask2 = w.training ? c.u(w.m2_at(s)) : nullptr;
    ef.h1_out = nullptr;   // the W2 gradient recomputes h1 (XM_H1)
    ef.a_b16 = p.b16;
    ef.n16 = p.n16;
    ef.uv16 = p.uv16;
    ef.n_nodes = b->n_nodes;
    ef.recv_blocks = p.recv_blocks;
    ef.uv_zero = s == 0 && !b->prop;   // 'propagation' = 0 (spwgnn.h): P0 = U0 = V0 = 0
    ef.gather_desc = p.gd_edge_fwd;
    ef.node_bytes = (uint32_t)(ef.gather_desc ? w.RN * kRowE * 4 : 0);
    ef.gates = gates ? gates + s * gate_step : nullptr;
    ef.gate_step = gate_step;
    return ef;
}

// every node forward stores through NodeFwdArgs::logits when it is set; step S−1 keeps its `last` shortcut
static NodeFwdArgs node_fwd_args(const Ctx& c, const spwgnn_batch* b, const Path& p, const FwdCall& call, int s) {
    const Ws& w = c.w;
    const int S = w.S;
    NodeFwdArgs nf{};
    nf.n_nodes = b->n_nodes;
    nf.H2s = c.f(w.H2s_at(s));
    nf.P = c.f(w.P_at(s));
    nf.co = c.f(w.co);
    nf.cw_out = (s == 0) ? c.f(w.cw) : nullptr;
    nf.cw_in = (s > 0) ? c.f(w.cw) : nullptr;
    nf.a_out = w.training ? c.f(w.a_at(s)) : nullptr;
    nf.o1_out = w.training ? c.f(w.o1_at(s)) : nullptr;
    nf.Pn = c.f(w.P_at(s + 1));
    nf.logits = (s == S - 1 || call.logit_step) ? call.logits + s * call.logit_step : nullptr;
    nf.U = (s + 1 < S) ? c.f(w.U_at(s + 1)) : nullptr;
    nf.V = (s + 1 < S) ? c.f(w.V_at(s + 1)) : nullptr;
    nf.w3a = c.pk(PK_W3A);
    nf.wo1c = c.pk(PK_WO1C); nf.wo1a = c.pk(PK_WO1A); nf.wo1p = c.pk(PK_WO1P);
    nf.wo2 = c.pk(PK_WO2);
    nf.w1b = c.pk(PK_W1B); nf.w1c = c.pk(PK_W1C);
    nf.bo1 = c.pk(PB_O1); nf.bo2p = c.pk(PB_O2P);
    nf.x_w3a = c.x6(X6_W3A); nf.xh_w3a = c.x6(X6_W3A_H);
    nf.x_wo1c = c.x6(X6_WO1C); nf.xh_wo1c = c.x6(X6_WO1C_H);
    nf.x_wo1a = c.x6(X6_WO1A); nf.xh_wo1a = c.x6(X6_WO1A_H);
    nf.x_wo1p = c.x6(X6_WO1P); nf.xh_wo1p = c.x6(X6_WO1P_H);
    nf.x_wo2 = c.x6(X6_WO2); nf.xh_wo2 = c.x6(X6_WO2_H);
    nf.x_w1b = c.x6(X6_W1B); nf.x_w1c = c.x6(X6_W1C);
    nf.n16 = p.n16;
    nf.uv16 = p.uv16;
    nf.p_zero = s == 0 && !b->prop;
    // P_S unwritten: its one reader must know (§3zh); a state request takes the general path (§3zo)
    nf.last = s == S - 1 && p.wide_node_side && !call.keep_state;
    return nf;
}

int32_t run_forward(const float* params, const spwgnn_batch* b, const spwgnn_run* r, const Ws& w, char* base,
                    const FwdCall& call, hipStream_t st) {
    const Ctx c{w, base, r->math != MATH_F32};
    const Path p = make_path(b, r, w, nullptr, call.gates != nullptr);
    if (int32_t e = prep(c, params, r, st)) return e;
    const EncNodeArgs en = enc_node_args(c, b, r, p);
    const EncEdgeArgs ee = enc_edge_args(c, b, r, p);
    const int S = r->mp_steps;
    const Prof prof{r, st};
    if (p.fwd_fused) {
        // small batch: the encoders and all S steps in one launch (timed as the relation encoder)
        FwdFusedArgs fa{};
        fa.ee = ee;
        fa.en = en;
        fa.ef = edge_fwd_args(c, b, p, 0, call.gates, call.gate_step);
        fa.nf = node_fwd_args(c, b, p, call, 0);
        fa.S = S;
        fa.training = r->training;
        fa.rowsN = w.RN * kRowN;
        fa.rowsE = w.RN * kRowE;
        fa.m1_step = r->training ? w.m1_at(1) - w.m1_at(0) : 0;
        fa.m2_step = r->training ? w.m2_at(1) - w.m2_at(0) : 0;
        fa.logits = call.logits;
        fa.logit_step = call.logit_step;
        // the encoders side by side in their own launch (a workgroup per block / node block) beat
        // running them one after the other inside each tile's workgroup
        fa.encoders = p.diag.fused_enc;
        SPW_CHECK(prof.before(SPWGNN_K_ENC_EDGE));
        if (!fa.encoders) SPW_CHECK(launch_enc_pair_team(ee, en, r->math, ee.z1 || ee.ed, st));
        SPW_CHECK(prof.after(SPWGNN_K_ENC_EDGE));
        SPW_TIMED(prof, SPWGNN_K_EDGE_FWD, launch_fwd_fused_team(fa, r->math, ee.z1 || ee.ed, st));
        return SPWGNN_OK;
    }
    if (p.enc_pair) {
        // small batch: both encoders in one launch (timed as the relation encoder)
        SPW_TIMED(prof, SPWGNN_K_ENC_EDGE, launch_enc_pair_team(ee, en, r->math, ee.z1 || ee.ed, st));
    } else {
        SPW_TIMED(prof, SPWGNN_K_ENC_NODE, launch_enc_node(en, r->math, st));
        SPW_TIMED(prof, SPWGNN_K_ENC_EDGE, launch_enc_edge(ee, p.enc_edge, st));
    }
    for (int s = 0; s < S; ++s) {
        SPW_TIMED(prof, SPWGNN_K_EDGE_FWD, launch_edge_fwd(edge_fwd_args(c, b, p, s, call.gates, call.gate_step), p.edge_fwd, st));
        SPW_TIMED(prof, SPWGNN_K_NODE_FWD, launch_node_fwd(node_fwd_args(c, b, p, call, s), p.node_fwd, st));
    }
    return SPWGNN_OK;
}

}  // namespace spw
