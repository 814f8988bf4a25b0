// Which kernels and storage formats a call takes (host only): every answer, decided once per call by
// make_path from (batch, run, workspace layout) and read by the launch sequences. The forward and the
// backward of a step derive the same Path from the same (batch, run), so the backward reads every array in
// the layout the forward wrote.
#pragma once
#include "../../include/spwgnn.h"
#include "workspace.h"

namespace spw {

// What a backward call asks for beyond (batch, run)
struct BwdCall {
    const float* dlogits;      // the last step's cotangent; with dl_step, row 0 of [S][dl_step] (§3zr)
    float* grads;
    float* dprop = nullptr;
    const BceArgs* bce = nullptr;     // spwgnn_bce_backward: the loss of the same call
    const float* dstate = nullptr;    // spwgnn_backward_state: the cotangent of P_S, row-major
    int64_t dl_step = 0;
    const float* gates = nullptr;     // spwgnn_backward_gated: the forward's relation gates (§3zz)
    int64_t gate_step = 0;            // spwgnn_backward_step_gated: gates is [S][gate_step], a row per step (§3zzc)
};

// Diagnosis switches (A/B of superseded kernels): environment variables read per call in -DSPWGNN_DIAG
// builds, all false in the shipping library
struct DiagSwitches {
    bool wg_old;          // SPWGNN_WG_OLD: the row-chunked weight-gradient kernels, stored z1 / zo1
    bool fused_enc;       // SPWGNN_FUSED_ENC: the encoders (and their backwards) inside the fused loops
    bool da_pair;         // SPWGNN_DA_PAIR: dA rebuilt by k_bwd_enc_pair_team, not summed in the fused loop
    bool w2g_gather;      // SPWGNN_W2G_GATHER: the per-edge gather W2 gradient (bf16)
    bool w2g_old;         // SPWGNN_W2G_OLD: the row-chunked W2 gradient (split maths)
    bool no_w2_merge;     // SPWGNN_NO_W2_MERGE: a small batch's W2 gradient as its own launch
    bool ws_unbatched;    // SPWGNN_WS_UNBATCHED: one k_wgrad_ws launch per gradient
    bool ws_nogroup;      // SPWGNN_WS_NOGROUP: no operand-sharing groups in the batched launch
    bool no_pos3_merge;   // SPWGNN_NO_POS3_MERGE: k_wgrad_pos3 as its own launch
};

struct Path {
    // the math each kernel family runs: the run's (backward families: math_bwd of it), or f32 for the
    // families SPWGNN_X6_KERNELS leaves out (diagnosis builds)
    int enc_edge, edge_fwd, node_fwd, node_bwd, edge_bwd, enc_edge_bwd, wgrad;
    // rm.1 / om.1 gradients rebuild z1 = relu(rm.0(d)) and zo1 = relu(om.0(y, w)) on the staging waves of
    // k_wgrad_ws: the encoders store d (8 bytes per edge) instead of the z1 rows and no zo1 rows
    bool z1_rebuilt;
    // dA = Σ_s dh1pre_s rebuilt once after the step loop (k_dA_x6 / k_dA_team) ...
    bool rebuild_dA;
    // ... reading back steps S−1 .. S−n_stored, kept by their edge backward in the slabs dz4..dz1 (§3zi)
    int n_stored;
    // bf16 math (training) stores what only ever feeds MFMA operands as bf16 (§3g): b16 the encoder-side
    // edge arrays z2, z3, c_r, dz4..dz1, dA and the step-invariant A; n16 also the node-side per-step
    // arrays H2s, o1, dU, dV, g, dx, when every writer and reader is a wide kernel; uv16 how U, V are
    // stored (kUvF32 / kUvRound / kUvB16: exactly when n16, §3ze)
    bool b16, n16;
    int uv16;
    bool fwd_fused, bwd_fused;   // the fused small-batch step loops (§3s)
    bool enc_pair;               // both encoders in one team launch
    // the node side runs only wide split-bf16 kernels, which know the loop-end rows are zero or unread (§3zh)
    bool wide_node_side;
    bool gd_w2, gd_edge_fwd, gd_edge_bwd;   // node rows through buffer descriptors (§3zk), per kernel
    bool recv_blocks;            // the receiver-block edge forward
    bool team_edges;             // team_blocks(n_eblocks): a small batch's gradients share launches
    // a gated call (relation gates, §3zz): the kernels of the ungated call — team, fused or wide — in their GATE
    // forms; the one-hot edge forward on a receiver-block plan, pointer-form gathers in the wide gated kernels, and
    // the small-batch W2 gradient as its own launch (the merged batch job is the descriptor form)
    bool gated;
    // a backward only (make_path with a BwdCall)
    bool ws_skip0;      // null prop: the k_wgrad_ws jobs over P leave step 0's stages out (§3zh)
    bool skip_eb0;      // ... and step 0's edge backward, which would write only dU_0 / dV_0, is not launched
    bool bce_inline;    // the fused loop computes dlogits itself; the loss sums ride in the last reduction
    bool split;         // spwgnn_run.grads_early_event: two weight-gradient groups
    DiagSwitches diag;
};

// gated: a forward with relation gates (a backward's are call->gates)
Path make_path(const spwgnn_batch* b, const spwgnn_run* r, const Ws& w, const BwdCall* call = nullptr,
               bool gated = false);

}  // namespace spw
