// make_path: the one place that decides a call's kernels and storage formats (path.h).
#include <atomic>
#include <cstdlib>
#include "path.h"

namespace spw {

// Diagnosis switches exist only in -DSPWGNN_DIAG builds; the shipping library's one environment-dependent
// choice is SPWGNN_GATHER_PTR (below). Per-kernel x6 selection for A/B diagnosis: SPWGNN_X6_KERNELS (bit mask of
// kX6*, default all) narrows a split-bf16 or bf16 math to some kernel families; the others run in f32 math.
enum : int { kX6EncEdge = 1, kX6EdgeFwd = 2, kX6NodeFwd = 4, kX6NodeBwd = 8, kX6EdgeBwd = 16, kX6EncEdgeBwd = 32,
             kX6Wgrad = 64 };
#ifdef SPWGNN_DIAG
static bool getenv_flag(const char* name) {
    const char* e = getenv(name);
    return e && *e && *e != '0';
}
static int kernel_mask() {
    static const int mask = [] {
        const char* e = getenv("SPWGNN_X6_KERNELS");
        return e ? (int)strtol(e, nullptr, 0) : -1;
    }();
    return mask;
}
#else
static bool getenv_flag(const char*) { return false; }
static int kernel_mask() { return -1; }
#endif

// K of the stored dh1pre steps is spwgnn_da_stored_steps, clamped per call to
// min(4, S−1): step 0 is always rebuilt (its edge backward may not run at all, §3zh).
#ifndef SPWGNN_DA_STORED
#define SPWGNN_DA_STORED 3   // same-box A/B at the headline batch: K = 3
#endif
static std::atomic<int> g_da_stored{SPWGNN_DA_STORED};
int da_stored_steps(int set) {
    return set >= 0 ? g_da_stored.exchange(set) : g_da_stored.load(std::memory_order_relaxed);
}

// Range guard of the buffer-descriptor gathers: the edge-side kernels address a node
// row by a 32-bit byte offset into one step's chunk-major array (U, V, G3: RN rows of kRowE floats), so
// that array must stay below 2^31 bytes; larger batches take the 64-bit pointer form of the same
// kernels. SPWGNN_GATHER_PTR (read per call: same-library A/B, tests) is a mask of kernels that take
// the pointer form anyway: 1 the W2 gradient, 2 the edge forward, 4 the edge backward (7: all).
enum : int { kGdW2 = 1, kGdEdgeFwd = 2, kGdEdgeBwd = 4 };
static bool gather_desc_fits(int64_t rows_padded) {
    return rows_padded * kRowE * (int64_t)sizeof(float) < (int64_t(1) << 31);
}

Path make_path(const spwgnn_batch* b, const spwgnn_run* r, const Ws& w, const BwdCall* call, bool gated) {
    Path p{};
    const int mask = kernel_mask(), mb = math_bwd(r->math);
    const auto family = [&](int bit, int m) { return (r->math != MATH_F32 && (mask & bit)) ? m : (int)MATH_F32; };
    p.enc_edge = family(kX6EncEdge, r->math);
    p.edge_fwd = family(kX6EdgeFwd, r->math);
    p.node_fwd = family(kX6NodeFwd, r->math);
    p.node_bwd = family(kX6NodeBwd, mb);
    p.edge_bwd = family(kX6EdgeBwd, mb);
    p.enc_edge_bwd = family(kX6EncEdgeBwd, mb);
    p.wgrad = family(kX6Wgrad, mb);
    p.diag = {getenv_flag("SPWGNN_WG_OLD"),      getenv_flag("SPWGNN_FUSED_ENC"),    getenv_flag("SPWGNN_DA_PAIR"),
              getenv_flag("SPWGNN_W2G_GATHER"),  getenv_flag("SPWGNN_W2G_OLD"),      getenv_flag("SPWGNN_NO_W2_MERGE"),
              getenv_flag("SPWGNN_WS_UNBATCHED"), getenv_flag("SPWGNN_WS_NOGROUP"), getenv_flag("SPWGNN_NO_POS3_MERGE")};
    // a gated call takes the path of the ungated one; what differs is listed at Path::gated. (Under a WideCall
    // team_blocks answers false below and in every launcher: the wide kernels for that call alone.)
    p.gated = gated || (call && call->gates);
    const bool team_tiles = team_blocks(b->n_wtiles), team_nodes = team_blocks((b->n_nodes + 31) / 32);
    const bool recv_plan = (b->flags & SPWGNN_BATCH_RECV_BLOCKS) != 0;
    p.team_edges = team_blocks(b->n_eblocks);

    p.z1_rebuilt = r->training && p.wgrad != MATH_F32 && !p.diag.wg_old;
    // plain read-add-writes of dA in the rebuild's order (SPWGNN_DA_RMW) exist for A/B only (§3f)
    p.rebuild_dA = b->nw_max <= 16 && p.edge_bwd != MATH_F32 &&
                   !(math_split32(p.edge_bwd) && !team_tiles && getenv_flag("SPWGNN_DA_RMW"));
    // every kernel that writes or reads a bf16-stored array must run in bf16 math for the layouts to agree
    p.b16 = r->training && r->math == MATH_BF16 && p.enc_edge == MATH_BF16 && p.enc_edge_bwd == MATH_BF16 &&
            p.wgrad == MATH_BF16 && p.rebuild_dA && !p.diag.wg_old;
    p.n16 = p.b16 && p.edge_fwd == MATH_BF16 && p.node_fwd == MATH_BF16 && p.node_bwd == MATH_BF16 &&
            p.edge_bwd == MATH_BF16 && b->nw_max <= 16 && !team_tiles && !team_nodes && !getenv_flag("SPWGNN_NODE_F32");
    p.uv16 = !(r->training && r->math == MATH_BF16) ? kUvF32 : p.n16 ? kUvB16 : kUvRound;

    const bool fwd_one = r->math == p.enc_edge && r->math == p.edge_fwd && r->math == p.node_fwd;
    const bool bwd_one = mb == p.node_bwd && mb == p.edge_bwd && mb == p.enc_edge_bwd;
    p.fwd_fused = fwd_one && fwd_fused_team(b->n_wtiles, b->nw_max, b->n_eblocks, b->n_nodes, r->math) && !recv_plan &&
                  !p.n16 && !getenv_flag("SPWGNN_NO_FWD_FUSED");
    p.bwd_fused = bwd_one && p.rebuild_dA && fwd_fused_team(b->n_wtiles, b->nw_max, b->n_eblocks, b->n_nodes, mb) &&
                  !recv_plan && !p.n16 && !getenv_flag("SPWGNN_NO_BWD_FUSED");
    p.enc_pair = r->math == p.enc_edge && enc_pair_team(b->n_eblocks, b->n_nodes, r->math) &&
                 !getenv_flag("SPWGNN_NO_ENC_PAIR");
    p.wide_node_side = r->math != MATH_F32 && p.node_fwd != MATH_F32 && !team_nodes &&
                       (!r->training || (p.node_bwd != MATH_F32 && p.wgrad != MATH_F32 && !p.diag.wg_old));
    p.recv_blocks = recv_plan && math_split32(p.edge_fwd) && b->n_eblocks == b->n_nodes && !getenv_flag("SPWGNN_RB_ONEHOT") &&
                    !p.gated;   // the column-sum kernel is not gated: the one-hot edge forward serves the plan

    // the wide x6 edge backward keeps dh1pre in dz4, dz3, dz2, dz1 — one chunk-major block per 32-edge
    // block, exactly a stored block's size — which nothing writes or reads between the previous backward's
    // weight gradients and this backward's relation-encoder pass: four slabs at one stride
    const int64_t slab_step = w.dz3 - w.dz4;
    if (p.rebuild_dA && math_split32(p.edge_bwd) && !team_tiles && !p.team_edges && !p.bwd_fused &&
        slab_step >= (int64_t)b->n_eblocks * kCmBlk && w.dz2 - w.dz3 == slab_step && w.dz1 - w.dz2 == slab_step)
        p.n_stored = std::max(0, std::min({da_stored_steps(-1), 4, r->mp_steps - 1}));

    const char* e = getenv("SPWGNN_GATHER_PTR");
    const int ptr_form = gather_desc_fits(w.RN) ? (e ? atoi(e) : 0) : -1;
    p.gd_w2 = !(ptr_form & kGdW2);
    p.gd_edge_fwd = !(ptr_form & kGdEdgeFwd);
    p.gd_edge_bwd = !(ptr_form & kGdEdgeBwd);

    if (call) {
        // a null prop is P0 = 0: step 0's rows add nothing to the W1b / W1c / omp.0-P gradients; dP_0,
        // dU_0 and dV_0 then feed only the dprop pass
        p.ws_skip0 = !b->prop && p.wgrad != MATH_F32 && !p.diag.wg_old;
        p.skip_eb0 = p.rebuild_dA && p.ws_skip0 && !call->dprop && !team_tiles;
        // on the fused loop (one loss workgroup) only; a weighted loss (bce->w) is never folded: its three
        // more kernel arguments cost the fused loop scratch and scalar spills (§3zl)
        p.bce_inline = call->bce && p.bwd_fused && call->bce->blocks == 1 && !call->bce->w;
        p.split = r->grads_early_event != nullptr;
    }
    return p;
}

}  // namespace spw
