/*
 * spwgnn.h — C-ABI of libspwgnn_hip.so, the MI355X (gfx950) propagation-network engine.
 *
 * The reference (irmakguzey/SPWGNN) has no FFI: its hot path is a Keras graph built by
 * PropagationNetwork.getModel (src/Networks.py:16-104) over MLP blocks (src/Blocks.py:12-91),
 * driven by model.fit (src/main.py:92-98) and model.predict (src/JengaBuilder.py:328-329,
 * src/TowerCreator.py:430-431). Each entry point below replaces one piece of that graph; the
 * cited lines say which. Everything is plain C: raw pointers, sizes, an int status. All device
 * memory is caller-owned; the library never allocates and never synchronises, so every
 * launch function is hipGraph-capturable on the caller's stream.
 *
 * Status codes: 0 = ok, SPWGNN_E_* below, or a positive hipError_t from a failed launch.
 */
#ifndef SPWGNN_H
#define SPWGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPWGNN_ABI_VERSION 8   /* 8: spwgnn_backward_inputs (+ added within 8: spwgnn_forward_state, spwgnn_backward_state; spwgnn_loss_weights, spwgnn_bce_weighted, spwgnn_bce_backward_weighted; SPWGNN_MATH_X3, spwgnn_math_products; SPWGNN_MATH_H3, spwgnn_math_products_bwd; spwgnn_plan_device, spwgnn_plan_device_positions, spwgnn_plan_device_dense; spwgnn_clip, spwgnn_adam_clipped, spwgnn_adam_clipped_dev, spwgnn_adam_lr_decayed, spwgnn_adam_lr_table_decay; spwgnn_forward_steps, spwgnn_backward_steps, spwgnn_step_weights, spwgnn_bce_steps; spwgnn_eval, spwgnn_eval_metrics; spwgnn_backward_relations; spwgnn_gates_supported, spwgnn_forward_gated, spwgnn_backward_gated; spwgnn_dropedge_gates, spwgnn_dropedge_keep_host; spwgnn_fused_path_gated); 7: spwgnn_da_stored_steps; 6: spwgnn_bce_backward; 5: spwgnn_team_max_blocks, spwgnn_host_device_ptr, spwgnn_plan_order, spwgnn_run.grads_early_event; 4: spwgnn_run.prologue; 3: spwgnn_batch.flags, receiver-block plans */

#define SPWGNN_OK 0
#define SPWGNN_E_ARG (-1)           /* bad argument (null pointer, negative size, …)          */
#define SPWGNN_E_SHAPE (-2)         /* shape outside what the kernels support                 */
#define SPWGNN_E_RELATION (-3)      /* relation matrix column is not one-hot / both-or-neither */
#define SPWGNN_E_WORKSPACE (-4)     /* workspace smaller than spwgnn_workspace_bytes()        */
#define SPWGNN_E_CAPACITY (-5)      /* caller-provided output array too small; device plans: a tower holds
                                     * more relations than its edge capacity                  */
#define SPWGNN_E_NOTRAIN (-6)       /* backward on a workspace run with training == 0         */

typedef void* spwgnn_stream_t;      /* a hipStream_t (NULL = default stream) */

/* ---------------------------------------------------------------- parameters ------------ */
/* The 22 Keras weight tensors of rm, om, rmp, omp (Networks.py:46-50, Blocks.py:20-28/60-68)
 * live in ONE flat fp32 buffer, Keras layout (kernel = [in][out] row-major, bias = [out]),
 * each tensor starting on a 64-float boundary. 209,501 real parameters. */
typedef struct spwgnn_param_info {
    const char* name;   /* e.g. "rmp.0.kernel" */
    int64_t offset;     /* in floats from the start of the flat buffer */
    int32_t rows;       /* kernel: in-features; bias: 1 */
    int32_t cols;       /* out-features */
} spwgnn_param_info;

int32_t spwgnn_version(void);
/* sizeof the ABI structs as this library was compiled (bindings check their own layouts against it):
 * which = 0 spwgnn_batch, 1 spwgnn_run, 2 spwgnn_plan_sizes, 3 spwgnn_param_info,
 * 4 spwgnn_loss_weights, 6 spwgnn_plan_device, 7 spwgnn_clip, 9 spwgnn_step_weights, 10 spwgnn_eval; -1
 * otherwise (5 and 8 are not used and stay -1). */
int32_t spwgnn_struct_size(int32_t which);
const char* spwgnn_strerror(int32_t status);
int32_t spwgnn_param_tensor_count(void);
int64_t spwgnn_param_count(void);                 /* padded flat length (floats)       */
int64_t spwgnn_param_real_count(void);            /* 209,501                           */
int32_t spwgnn_param_tensor(int32_t index, spwgnn_param_info* out);

/* ------------------------------------------------------------- host-side input builders -- */
/* Dense relation matrices → compact edge list. Replaces the one-hot batch_dot gathers of
 * Networks.py:27-33/:84-85 and the segment-sum of :88 at the input boundary: a column k
 * of (Rs, Rr) that is one-hot in both is edge k (sender, receiver); an all-zero column is an
 * inactive relation (it never reaches an output, Networks.py:88); a column one-hot in Rs only
 * also never reaches an output and is dropped; anything else → SPWGNN_E_RELATION.
 * Rs, Rr: host fp32 [B][N][E], E = N(N-1). Output edges are tower-major, slot order (the
 * sender-major enumeration of main.py:72-81). src/dst are GLOBAL node ids (b*N + local). */
int32_t spwgnn_dense_to_edges(const float* Rs, const float* Rr, int32_t B, int32_t N,
                              int32_t* src, int32_t* dst, int32_t* slot, int64_t capacity,
                              int64_t* n_edges, int32_t* tower_edge_count);

/* Work plan for the edge kernels: towers are packed into wave-tiles of whole towers with at
 * most nw_max nodes; each wave-tile's edges are cut into 32-edge blocks (last one padded with
 * -1). blk_csr holds, per block, the block's edge slots sorted by local receiver and by local
 * sender (deterministic segment sums). Two phases: sizes, then fill. Host memory. src/dst may
 * be NULL when no tower has an edge (single-box towers, or no relation under the threshold). */
typedef struct spwgnn_plan_sizes {
    int32_t n_wtiles;
    int32_t n_eblocks;
    int32_t nw_max;     /* max nodes in any wave-tile (<= requested nw_max) */
} spwgnn_plan_sizes;

int32_t spwgnn_plan_size(int32_t n_towers, const int32_t* tower_nodes, const int32_t* tower_edges,
                         int32_t nw_max, spwgnn_plan_sizes* out);
int32_t spwgnn_plan_fill(int32_t n_towers, const int32_t* tower_nodes, const int32_t* tower_edges,
                         const int32_t* src, const int32_t* dst, int32_t nw_max,
                         const spwgnn_plan_sizes* sizes, int32_t* wtile /* [n_wtiles][4] */,
                         int32_t* edge_src /* [n_eblocks*32] */, int32_t* edge_dst,
                         int32_t* edge_id /* [n_eblocks*32] original edge index or -1 */,
                         uint8_t* blk_csr /* [n_eblocks][128] */);
/* A tower ORDER for ragged batches (the plan packs whole towers in the order given): towers by
 * decreasing edge count, each into the open wave-tile (<= nw_max nodes) whose last 32-edge block has
 * room for its edges, else a new tile; order[k] = the k-th tower, each tile's towers consecutive.
 * Planned in this order a batch needs no more blocks than in its own order and usually far fewer
 * (BASELINE config 4's ragged 4-16-box thresholded towers: 67 % -> 78 % block fill):
 * both orders are sized as spwgnn_plan_size would (same nw_max), and where the packed one needs more
 * blocks the identity order[k] = k is returned.
 * The caller permutes its towers (node rows, edge lists, targets, propagation) and keeps each
 * tower's original id for the dropout key (TowerBatch tower_ids). Deterministic. Host memory. */
int32_t spwgnn_plan_order(int32_t n_towers, const int32_t* tower_nodes, const int32_t* tower_edges, int32_t nw_max,
                          int32_t* order);

/* The same plan with each tower's blocks sized for tower_edge_cap[t] >= tower_edges[t] edges
 * (e.g. N(N-1), every relation slot): the wave-tiles and block counts then depend only on the
 * tower sizes and capacities, so batches of the same shape share one plan geometry and one
 * captured hipGraph (the unused capacity is padding, index -1, which matches no node). */
int32_t spwgnn_plan_size_cap(int32_t n_towers, const int32_t* tower_nodes, const int32_t* tower_edge_cap,
                             int32_t nw_max, spwgnn_plan_sizes* out);
int32_t spwgnn_plan_fill_cap(int32_t n_towers, const int32_t* tower_nodes, const int32_t* tower_edges,
                             const int32_t* tower_edge_cap, const int32_t* src, const int32_t* dst, int32_t nw_max,
                             const spwgnn_plan_sizes* sizes, int32_t* wtile, int32_t* edge_src, int32_t* edge_dst,
                             int32_t* edge_id, uint8_t* blk_csr);

/* Receiver blocks: every node of a wave-tile owns ONE 32-edge block that holds its in-edges (≤ 32
 * per node; input order within a receiver; nodes without in-edges get an all-padding block), so
 * wtile[w] = (first block, #nodes, first node, #nodes) and block first_block + j feeds node
 * first_node + j alone. Set SPWGNN_BATCH_RECV_BLOCKS in spwgnn_batch.flags for such a plan: the
 * x6 edge forward then sums each block's messages as one column sum instead of a one-hot product
 * (large fully connected towers, BASELINE config 5). Every other kernel takes either layout. */
int32_t spwgnn_plan_size_recv(int32_t n_towers, const int32_t* tower_nodes, int32_t nw_max, spwgnn_plan_sizes* out);
int32_t spwgnn_plan_fill_recv(int32_t n_towers, const int32_t* tower_nodes, const int32_t* tower_edges,
                              const int32_t* src, const int32_t* dst, int32_t nw_max, const spwgnn_plan_sizes* sizes,
                              int32_t* wtile, int32_t* edge_src, int32_t* edge_dst, int32_t* edge_id,
                              uint8_t* blk_csr);

/* ------------------------------------------------- device-side plans (added within ABI 8) -- */
/* A capacity plan (spwgnn_plan_size_cap / spwgnn_plan_fill_cap) fixes its geometry — wtile, node_tower,
 * node_local, the block count — from the tower sizes and capacities alone; only edge_src, edge_dst and
 * blk_csr depend on the relation set. The two calls below fill those three on the DEVICE, from device
 * positions (the thresholded relation set of main.py:71-81) or from device relation matrices (the
 * semantics of spwgnn_dense_to_edges), exactly where spwgnn_plan_fill_cap puts them on the host: no
 * host round trip, no synchronisation, one launch each, hipGraph-capturable. Build the geometry once
 * per shape with spwgnn_plan_fill_cap given zero edges (tower_edges all 0, src = dst = NULL), upload
 * wtile and node_local, and add wtile_tower[w] = the index of wave-tile w's first tower.
 * Every pointer is device memory. wtile, node_local, wtile_tower (and tower_cap when given) are read
 * only and may be shared between batches of one shape.
 * Memory safety does not depend on the input data: an edge beyond its wave-tile's 32·#blocks slots, or
 * beyond its tower's capacity, is not written; *status (the caller zeroes it) then takes, by an atomic
 * max, the POSITIVE code −SPWGNN_E_CAPACITY; a relation column that spwgnn_dense_to_edges rejects
 * gives −SPWGNN_E_RELATION (the column counts as inactive), a geometry the kernel cannot serve
 * −SPWGNN_E_SHAPE. The arrays of a batch whose status is non-zero must not be run. */
typedef struct spwgnn_plan_device {
    int32_t n_towers;
    int32_t n_nodes;
    int32_t n_wtiles;
    int32_t n_eblocks;
    int32_t nw_max;             /* 1..32 */
    int32_t reserved;           /* 0 */
    const int32_t* wtile;       /* [n_wtiles][4] of the capacity plan                                */
    const int32_t* node_local;  /* [n_nodes]; a node with node_local == 0 starts a tower             */
    const int32_t* wtile_tower; /* [n_wtiles] index of each wave-tile's first tower                  */
    const int32_t* tower_cap;   /* [n_towers] the capacities the geometry was sized with; NULL =
                                 * N(N-1) per tower (every relation slot: cannot overflow)           */
    int32_t* edge_src;          /* out [n_eblocks*32]                                                */
    int32_t* edge_dst;          /* out [n_eblocks*32]                                                */
    uint8_t* blk_csr;           /* out [n_eblocks][128], 16-byte aligned                             */
    float* pos;                 /* out [n_nodes][4], 16-byte aligned: raw.xyz / divisor, 0 (positions
                                 * source; NULL = not written; must be NULL for the dense source)    */
    int32_t* tower_edges;       /* out [n_towers] active relations per tower; NULL = not written     */
    int32_t* status;            /* in/out device word, see above                                     */
    void** prof_events;         /* NULL, or two hipEvent_t recorded before / after the launch (the
                                 * timing hook of spwgnn_run, kernel id SPWGNN_K_PLAN_DEVICE)        */
} spwgnn_plan_device;

/* Relations from positions: raw [n_nodes][raw_stride >= 2] fp32 raw-pixel rows (x, y[, w, …]) in the
 * plan's node order. Slot (m, j != m) of a tower — the sender-major order of main.py:72-81 — is
 * active iff dx·dx + dy·dy < threshold·threshold, every operation rounded to fp32 on its own (no
 * contraction, no square root); threshold <= 0 or NaN = fully connected (JengaBuilder.py:309-326).
 * pos (when given; needs raw_stride >= 3) = raw.xyz / divisor in IEEE fp32 division (main.py:91: 170).
 * SPWGNN_E_ARG / SPWGNN_E_SHAPE before any device work for a null or misaligned pointer, sizes that do
 * not agree, nw_max outside 1..32, raw_stride < 2, a zero or NaN divisor. */
int32_t spwgnn_plan_device_positions(const spwgnn_plan_device* plan, const float* raw, int32_t raw_stride,
                                     float threshold, float divisor, spwgnn_stream_t stream);
/* Relations from dense matrices: Rs, Rr device fp32 [B][N][E], E = N(N-1), uniform towers (n_towers
 * == B, n_nodes == B·N, 1 <= N <= nw_max). Column k of tower b is the edge (row holding Rs's 1 → row
 * holding Rr's 1); no receiver = inactive; a value outside {0, 1}, two ones in a column or a receiver
 * without a sender = −SPWGNN_E_RELATION in *status. Same argument checks; N < 1 is SPWGNN_E_ARG; the
 * empty matrices of single-box towers (N == 1, E = 0) may be NULL. */
int32_t spwgnn_plan_device_dense(const spwgnn_plan_device* plan, const float* Rs, const float* Rr, int32_t B,
                                 int32_t N, spwgnn_stream_t stream);

/* ------------------------------------------------------------------- device batch ------- */
#define SPWGNN_BATCH_RECV_BLOCKS 1   /* spwgnn_batch.flags: the plan is a receiver-block plan */
typedef struct spwgnn_batch {
    int32_t n_towers;
    int32_t n_nodes;        /* Σ N over towers */
    int32_t n_wtiles;
    int32_t n_eblocks;
    int32_t nw_max;
    int32_t flags;          /* SPWGNN_BATCH_* (0: a plan of spwgnn_plan_fill / _fill_cap)      */
    const float* pos;           /* [n_nodes][4]: objects (x, y, w)/170 + 0 pad (Networks.py:22)   */
    const float* prop;          /* [n_nodes][100] 'propagation' input (Networks.py:29); NULL = 0  */
                                /* NULL is the fast case: the large-batch kernels skip the products with
                                 * the zero state instead of multiplying it (an all-zero array is not detected) */
    const int32_t* node_tower;  /* [n_nodes] tower id (dropout key)                                */
    const int32_t* node_local; /* [n_nodes] node index inside its tower (dropout key)             */
    const int32_t* wtile;       /* [n_wtiles][4] first block, #blocks, first node, #nodes         */
    const int32_t* edge_src;    /* [n_eblocks*32] global sender, -1 = padding                     */
    const int32_t* edge_dst;    /* [n_eblocks*32] global receiver, -1 = padding                   */
    const uint8_t* blk_csr;     /* [n_eblocks][128]                                                */
} spwgnn_batch;

/* A replayed training step's first work, folded into the forward's first launch (spwgnn_run.prologue):
 * the batch upload of spwgnn_copy_in (copy_bytes from copy_src — pinned, device-mapped — to copy_dst;
 * both 16-byte aligned, copy_bytes a multiple of 16; 0 = none) and the key/step advance of
 * spwgnn_step_advance (key NULL = none; mode SPWGNN_STEP_KEY_*). The same effects as those two calls
 * issued before the forward, two launches fewer; the forward's own kernels run after them. */
typedef struct spwgnn_prologue {
    const void* copy_src;
    void* copy_dst;
    int64_t copy_bytes;
    uint64_t* key;
    int32_t* step;
    int32_t mode;
    int32_t rank;
    uint64_t seed;
} spwgnn_prologue;

typedef struct spwgnn_run {
    int32_t mp_steps;   /* propagation steps; the reference hard-codes 5 (Networks.py:83)      */
    int32_t training;   /* 1: keep activations for backward + apply dropout                      */
    float dropout;      /* Dropout rate on the two encodings (Networks.py:77-78); 0 = off      */
    int32_t math;       /* SPWGNN_MATH_*: how the fp32 matrix products run on the matrix cores   */
    uint64_t seed;      /* dropout mask key                                                       */
    /* Optional timing hook (bench/profiling): for each launch of kernel `prof_kernel`
     * (SPWGNN_K_*), the library records caller-created hipEvent_t prof_events[2k] before and
     * prof_events[2k+1] after launch k (k < prof_count) on the call's stream. 0 = off. */
    int32_t prof_kernel;
    int32_t prof_count;
    void** prof_events;
    /* Replayable steps (hipGraph): when non-NULL the dropout key is read from this device word at
     * run time instead of `seed`, so a captured step draws new masks on every replay once
     * spwgnn_step_advance has moved the key on. NULL = use `seed`. */
    const uint64_t* seed_dev;
    /* spwgnn_forward only: work to run first (above); NULL = none. Read at call time. */
    const spwgnn_prologue* prologue;
    /* spwgnn_backward only: a hipEvent_t (NULL = none). When set, the weight gradients are issued in
     * two groups and this event is recorded on the call's stream as soon as the EARLY range of the
     * flat gradient buffer is final: from the offset of "rmp.1.kernel" to the end (rmp.1, rmp.2, omp.0,
     * omp.1 — they need only the propagation-step loop). The dA rebuild, the relation encoder's backward
     * and the late range (rm, om, rmp.0) follow. A data-parallel caller all-reduces the early range on
     * another stream after hipStreamWaitEvent, overlapped with the rest of the backward.
     * Same results as without the event. */
    void* grads_early_event;
} spwgnn_run;

/* Matrix-product arithmetic. F32 and X6 give fp32-class results, H3 fp32-class logits
 * and X6's gradients; X3 and BF16 do not:
 *   F32  v_mfma_f32_*_f32: one fp32 fma chain per output (the f32 MFMA rate, 157 TF)
 *   X6   each fp32 operand split into three bf16 parts, six bf16 MFMA products per fp32 product,
 *        fp32 accumulation (6/16 of the f32 MFMA cost; error O(2^-24) per product)
 *   BF16 operands rounded to bf16, one bf16 MFMA product, fp32 accumulation; in training the
 *        stored A, U, V (the three terms of h1) rounded to bf16 once (BASELINE configs 3-4 are
 *        quoted in bf16; error O(2^-9) per product — not the fp32 parity path)
 *   X3   (added within ABI 8) each fp32 operand x split into two bf16 parts,
 *        h = bf16_rne(x), m = bf16_rne(x − h) — the first two parts of X6's split, the third is not
 *        formed — and three bf16 MFMA products per fp32 product, acc += a_m·b_h, then a_h·b_m, then
 *        a_h·b_h, with fp32 accumulation: X6's order without the terms that hold a third part and
 *        without m·m. Operands carry a 16-bit mantissa over the whole fp32 exponent range (no
 *        scaling); error O(2^-17) per product. One-hot sums (the receiver sum of h2, the sender /
 *        receiver sums of dh1pre) and bias gradients sum the two-part roundings of their values.
 *        Everything X6 keeps in fp32 stays fp32 (every stored array, the vector-ALU first layers,
 *        bias / relu / tanh / dropout, BCE, Adam); X3 takes X6's kernels, launch paths and f32
 *        fallbacks with two parts. Not fp32-class and not the parity path: between BF16 and X6.
 *   H3   (added within ABI 8) a mixed math: the forward's matrix products (the
 *        encoders, the edge and node forward of every step, training and inference) split each fp32
 *        operand x into two IEEE half parts, h = f16_rne(x), m = f16_rne(x − h), subnormal halves
 *        kept, and run three f16 MFMA products per fp32 product in X3's order (a_m·b_h, a_h·b_m,
 *        a_h·b_h) with fp32 accumulation; the forward receiver sum of h2 multiplies the exact one-hot
 *        by the two parts. The operand error floor is 2^-25 absolute (22 mantissa bits for
 *        |x| ≥ 2^-14): fp32-class logits at X3's instruction count. Every backward product (edge and
 *        node backward, dA, every weight gradient, the encoder backwards, spwgnn_backward_inputs,
 *        spwgnn_backward_state) is X6's, unchanged: gradients shrink below fp16's range layer by
 *        layer, and fp16 parts there need per-tensor scales that are not built. Storage, workspace
 *        size and layout, launch paths and fallbacks are X6's.
 *        RANGE: an operand of a forward product (a weight, an activation, 'propagation') of
 *        magnitude ≥ 65,520 rounds to inf in fp16 (65,504 is the largest half) and the logits become
 *        inf / NaN; the library does not check this. Positions never enter a matrix product (the
 *        first layers run in fp32 on the vector ALU) and a 'propagation' that comes from the network
 *        is tanh-bounded. */
#define SPWGNN_MATH_F32 0
#define SPWGNN_MATH_X6 1
#define SPWGNN_MATH_BF16 2
#define SPWGNN_MATH_X3 3
#define SPWGNN_MATH_H3 4

/* 16-bit MFMA products per fp32 product of a math id: 6 (X6), 3 (X3, and H3: its forward's), 1 (BF16),
 * 0 (F32: none, the f32 matrix instructions); −1 for an id this library does not know. Bindings probe
 * support of a math with it and profilers price FLOPs by it. No device work. */
int32_t spwgnn_math_products(int32_t math);
/* (added within ABI 8) The same for the backward's products: 6 (X6 and H3), 3 (X3), 1 (BF16), 0 (F32),
 * −1 for an unknown id — what a profiler prices the backward kernels at. No device work. */
int32_t spwgnn_math_products_bwd(int32_t math);

#define SPWGNN_K_NONE 0
#define SPWGNN_K_EDGE_FWD 1
#define SPWGNN_K_NODE_FWD 2
#define SPWGNN_K_EDGE_BWD 3
#define SPWGNN_K_NODE_BWD 4
#define SPWGNN_K_ENC_EDGE 5
#define SPWGNN_K_ENC_EDGE_BWD 6
#define SPWGNN_K_WGRAD_W2 7
#define SPWGNN_K_DA 8          /* dA = Σ_s dh1pre_s rebuilt after the backward step loop (bf16 math) */
#define SPWGNN_K_WGRAD_WS 9    /* every stored-operand weight gradient (k_wgrad_ws family, split-bf16 maths) */
#define SPWGNN_K_ENC_NODE 10
#define SPWGNN_K_ENC_NODE_BWD 11
#define SPWGNN_K_INPUT_BWD 12  /* spwgnn_backward_inputs' one launch */
#define SPWGNN_K_PLAN_DEVICE 13 /* spwgnn_plan_device_positions / _dense's one launch (spwgnn_plan_device.prof_events) */
#define SPWGNN_K_STATE 14      /* the layout launch of spwgnn_forward_state (P_S out) / spwgnn_backward_state (dstate in) */
#define SPWGNN_K_REL_BWD 15    /* spwgnn_backward_relations' one launch */
#define SPWGNN_K_DROPEDGE 16   /* spwgnn_dropedge_gates' one launch */

/* Workspace bytes for (n_nodes, n_eblocks, mp_steps, training). */
int64_t spwgnn_workspace_bytes(int32_t n_nodes, int32_t n_eblocks, int32_t mp_steps, int32_t training);

/* Which launches a forward / backward of this batch and run takes (no device work): bit 0 = the
 * forward's fused small-batch step loop, bit 1 = the backward's; < 0 = an error
 * status. Profilers attribute kernel time and FLOPs by it instead of restating the library's gate. */
/* State-carrying calls (spwgnn_forward_state with a buffer, spwgnn_backward_state with a cotangent) take
 * the same path as the plain calls of the batch: the fused loops run the seeded first step themselves
 * (their resource use is unchanged), so this answer holds for them too. */
int32_t spwgnn_fused_path(const spwgnn_batch* batch, const spwgnn_run* run);
/* (added within ABI 8) The same bits for a call of this batch and run WITH relation gates (spwgnn_forward_gated /
 * spwgnn_backward_gated, below): a gated call takes the launches of the ungated one, in their gated forms.
 * SPWGNN_E_SHAPE for a math spwgnn_gates_supported answers 0 to. spwgnn_fused_path itself is unchanged. */
int32_t spwgnn_fused_path_gated(const spwgnn_batch* batch, const spwgnn_run* run);

/* Batches of at most this many 32-row blocks (edge blocks, node blocks, wave-tiles; counted per
 * launch) run the latency-oriented team kernels, larger ones the wide kernels the large-batch step
 * runs (both compute the same products in the same order). Default 512 (the
 * reference's batch 32 is ~30 blocks). set >= 0 sets the limit for the process and returns the
 * previous one; set < 0 only returns it. 0 puts every batch on the wide kernels (parity tests of the
 * large-batch path at oracle-sized batches). Read when a call plans its launches. */
int32_t spwgnn_team_max_blocks(int32_t set);

/* ABI 7. Stored steps of the dA sum on the wide x6 kernels: the edge backward of the
 * last K propagation steps also keeps its dh1pre, and the dA kernel reads those K steps back instead
 * of repeating their W2ᵀ products. Every K gives bitwise the same gradients; it trades matrix work for
 * streamed bytes. The slabs are workspace arrays that are dead meanwhile: no larger workspace. K is
 * clamped per call to min(4, mp_steps − 1) and is 0 for bf16 / fp32 math (x3 stores like x6), small (team) batches and
 * receiver-block plans. set >= 0 sets K for the process and returns the previous value; set < 0 only
 * returns it. Read when a call plans its launches. */
int32_t spwgnn_da_stored_steps(int32_t set);

/* Forward: the whole graph of Networks.py:31-96 → per-node logits z (the model output is
 * sigmoid(z), Networks.py:94). logits: [n_nodes] device fp32. */
int32_t spwgnn_forward(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                       void* workspace, int64_t workspace_bytes, float* logits,
                       spwgnn_stream_t stream);

/* Backward of the last spwgnn_forward on the same workspace (training == 1): dlogits [n_nodes]
 * → grads (flat, same layout as params; overwritten) and, if dprop != NULL, d/d propagation
 * [n_nodes][100]. Replaces TF autodiff of the graph (Networks.py:102 compile → fit).
 * dprop == NULL is the fast case: step 0's gradient of the state is then not computed at all (with
 * batch->prop == NULL too, the large-batch step loop also drops step 0's edge backward). The batch
 * must be the forward's, its prop pointer null or non-null as it was there. */
int32_t spwgnn_backward(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                        void* workspace, int64_t workspace_bytes, const float* dlogits,
                        float* grads, float* dprop, spwgnn_stream_t stream);

/* The final propagation state and its gradient (added within ABI 8: new symbols only, no existing
 * struct or signature changed). P_S = tanh(x[:, 1:] + P_{S-1}) of the last step (Networks.py:91) is the
 * value a caller feeds to the next call as batch->prop: a belief state carried across the frames of a
 * trajectory, a long propagation run in chunks, a loss on the state.
 *
 * spwgnn_forward_state: spwgnn_forward, and with state_out != NULL also P_S → state_out, [n_nodes][100]
 * device fp32 (16-byte aligned), rows in the plan's node order, every row written, nothing past them.
 * state_out == NULL is spwgnn_forward bit for bit; with a buffer the logits are the same bits as
 * without it. Training and inference, every math, every plan kind. One more launch (kernel id
 * SPWGNN_K_STATE); the large-batch split-bf16 node forward runs its last step without the "only the
 * logit is read" shortcut so that P_S exists. */
int32_t spwgnn_forward_state(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                             void* workspace, int64_t workspace_bytes, float* logits,
                             float* state_out /* [n_nodes][100] device fp32, plan node order; NULL = none */,
                             spwgnn_stream_t stream);
/* spwgnn_backward_state: spwgnn_backward, and with dstate != NULL the backward of
 *   Σ dlogits·z + Σ dstate·P_S
 * in ONE pass over the step loop: dstate ([n_nodes][100] device fp32, 16-byte aligned, plan node order)
 * enters as the incoming dP of step S-1. dstate == NULL is spwgnn_backward bit for bit. dlogits stays
 * required: a caller with no loss on the logits passes zeros. grads_early_event, spwgnn_backward_inputs
 * after it and the stored dh1pre steps work as after spwgnn_backward. One more launch (SPWGNN_K_STATE).
 * CONTRACT for dstate != NULL: the forward on this workspace was spwgnn_forward_state with a non-NULL
 * state_out and training == 1. After a plain spwgnn_forward the large-batch path has not written its
 * P_S rows and the result is undefined (the reads stay inside the workspace either way). The library
 * does not synchronise and cannot check this; the Python layer does (engine.Workspace). */
int32_t spwgnn_backward_state(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                              void* workspace, int64_t workspace_bytes, const float* dlogits,
                              const float* dstate /* [n_nodes][100] device fp32, plan node order; NULL = none */,
                              float* grads, float* dprop, spwgnn_stream_t stream);

/* ABI 8. d(loss)/d(batch->pos) of the last spwgnn_backward / spwgnn_bce_backward on this workspace
 * (same batch, same run; before the next forward on it): dpos [n_nodes][4] device fp32 (16-byte
 * aligned), column 3 = 0, every row written, rows in the plan's node order. The gradient with respect
 * to the objects rows (x, y, width)/170 of Networks.py:22: x and y through the relation encoder's
 * input pos[receiver].xy - pos[sender].xy (Networks.py:58-62), y and width through the object
 * encoder's (Networks.py:65-71). The relation set (a thresholded one included, main.py:71-81) is a
 * constant of the graph and is NOT differentiated. One launch that streams the first encoder layers'
 * pre-activation gradients the backward left in the workspace; sums in plan order without atomics
 * (the same bits on every run). `params` is the flat buffer the forward ran with. */
int32_t spwgnn_backward_inputs(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                               void* workspace, int64_t workspace_bytes, float* dpos, spwgnn_stream_t stream);

/* Relation gradients (added within ABI 8: a new symbol only, no existing struct or signature changed;
 * DESIGN.md §3zy): which contact a prediction rests on. Put a scalar gate w_k on every active edge
 * k = (src_k → dst_k) in the receiver sum of Networks.py:88 ALONE,
 *   eff_{i,s} = tanh(Σ_{k: dst_k = i} w_k · e_{k,s}),   e_{k,s} = the edge propagator's output at step s,
 * and take the gradient at the run's gates (w ≡ 1 after an ungated forward; the gates of
 * spwgnn_forward_gated / spwgnn_backward_gated after a gated one, below):
 *   r_{k,s} = ⟨g_s[dst_k], e_{k,s}⟩ = ⟨G3_s[dst_k], h2_{k,s}⟩ + ⟨g_s[dst_k], b3⟩,   r_k = Σ_s r_{k,s},
 * g_s = d loss / d (pre-tanh receiver sum of step s), G3_s = g_s·W3ᵀ, h2 = relu(relu(A + U_s[src] +
 * V_s[dst])·W2 + b2). In reference terms r_k is d loss / d receiver_relations[b, dst_k, k] through line 88
 * alone: NOT through the gathers of Networks.py:33 and :85, which read the same tensors.
 * Of the last spwgnn_backward / _state / _gated / _steps / spwgnn_bce_backward* on this workspace (same batch, same
 * run; before the next forward on it). One launch (kernel id SPWGNN_K_REL_BWD) that rebuilds h2 per
 * (32-edge block, step) from the stored rows on the run's backward product class (X6 and H3: six bf16
 * products, X3: three, BF16: one, F32: the f32 matrix instructions) and sums the steps per edge in step
 * order: no atomics, the same bits on every run.
 * drel [32·n_eblocks] device fp32 in the plan's edge-slot order (edge_src / edge_dst's): every slot is
 * written, a padding slot (edge_src < 0 or edge_dst < 0) with 0; drel_steps (NULL = none) [mp_steps]
 * [32·n_eblocks] holds r_{k,s} the same way. The workspace is only read: the gradients the backward
 * returned, spwgnn_backward_inputs and a second call of this one work before or after it. `params` is the
 * flat buffer the forward ran with. Ordinary, capacity-padded and receiver-block plans alike.
 * SPWGNN_E_ARG (a null params or drel), SPWGNN_E_NOTRAIN, SPWGNN_E_WORKSPACE before any device work. */
int32_t spwgnn_backward_relations(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                                  void* workspace, int64_t workspace_bytes,
                                  float* drel       /* [32·n_eblocks] plan edge-slot order */,
                                  float* drel_steps /* [mp_steps][32·n_eblocks], or NULL */,
                                  spwgnn_stream_t stream);

/* Relation gates (added within ABI 8: new symbols only, no existing struct or signature changed;
 * DESIGN.md §3zz): soft relations in the forward and the backward. One gate w_k per active edge, shared by
 * all mp_steps steps, any finite fp32 (0 and negative values included), in the receiver sum of
 * Networks.py:88 ALONE:
 *   eff_{i,s} = tanh(Σ_{k: dst_k = i} w_k · (h2_{k,s}·W3 + b3)) = tanh([Σ w_k·h2_{k,s} | Σ w_k]·[W3; b3]).
 * Nothing else in the graph sees the gate: the gathers of Networks.py:33 and :85 stay ungated. w_k = 0
 * MULTIPLIES, it does not delete: an edge whose message is infinite or NaN gives NaN under a zero gate
 * (0·inf), where a plan built without that edge would not.
 * gates: device fp32 [32·n_eblocks] (16-byte aligned) in the plan's edge-slot order (edge_src / edge_dst's,
 * the order of spwgnn_backward_relations' drel). A padding slot's value is never used: any bits there, NaN
 * included, leave every output unchanged.
 * gates == NULL: spwgnn_forward_state / spwgnn_backward_state bit for bit, with the same launches (the
 * team / fused small-batch path where it applies). With gates the call takes the launches of the ungated call
 * in their gated forms — the team kernels and the fused small-batch step loops included
 * (spwgnn_fused_path_gated), with the results of the wide gated kernels bit for bit — except that a
 * receiver-block plan runs the one-hot edge forward (the column-sum kernel is not gated), the wide gated kernels
 * gather through 64-bit pointers, and a small batch's W2 gradient runs as its own launch. Every plan kind (capacity, packed, device-filled with
 * all-padding blocks, wave-tiles of up to 32 nodes), a null or non-null prop, with or without dprop /
 * state_out / dstate, training and inference, every spwgnn_da_stored_steps setting.
 * Maths: spwgnn_gates_supported(math) is 1 for X6, X3 and H3, 0 for F32 and BF16 — a gated call in those
 * returns SPWGNN_E_SHAPE — and -1 for an id this library does not know. All argument errors (a
 * misaligned gates pointer: SPWGNN_E_ARG) return before any device work.
 * CONTRACT: the backward's gates hold the values the forward's held (the library cannot check it; the
 * Python layer does, engine.Workspace). After spwgnn_backward_gated, spwgnn_backward_inputs works as
 * before and spwgnn_backward_relations returns d loss / d w_k AT THESE GATES.
 * Per-step logits with gates and spwgnn_bce_backward with gates are not part of this. Per-step gates, one
 * w_{k,s} per edge and step, are spwgnn_forward_step_gated / spwgnn_backward_step_gated, below. */
int32_t spwgnn_gates_supported(int32_t math);
int32_t spwgnn_forward_gated(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                             void* workspace, int64_t workspace_bytes,
                             const float* gates /* [32·n_eblocks] plan edge-slot order; NULL = ungated */,
                             float* logits, float* state_out /* as spwgnn_forward_state */,
                             spwgnn_stream_t stream);
int32_t spwgnn_backward_gated(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                              void* workspace, int64_t workspace_bytes,
                              const float* gates /* the forward's; NULL = ungated */,
                              const float* dlogits, const float* dstate /* as spwgnn_backward_state */,
                              float* grads, float* dprop, spwgnn_stream_t stream);

/* Per-step relation gates (added within ABI 8: new symbols only): one gate w_{k,s} per active
 * edge k AND propagation step s, any finite fp32:
 *   eff_{i,s} = tanh(Σ_{k: dst_k = i} w_{k,s} · (h2_{k,s}·W3 + b3)),
 * everything else as the shared gates above (ungated gathers, multiplying zeros, padding slots never used).
 * gates: device fp32 [mp_steps][gate_step], row s in the order of spwgnn_forward_gated's gates; gate_step >=
 * 32·n_eblocks and a multiple of 4 (every row 16-byte aligned), else SPWGNN_E_ARG before any device work. The
 * slots [32·n_eblocks, gate_step) of a row are never read. gates == NULL (gate_step ignored): spwgnn_forward_state
 * / spwgnn_backward_state bit for bit. mp_steps equal rows give spwgnn_forward_gated / _backward_gated bit for
 * bit. The calls take the launches of the shared-gate calls (spwgnn_fused_path_gated), with their maths
 * (spwgnn_gates_supported; SPWGNN_E_SHAPE otherwise), plan kinds and options, and their CONTRACT: the backward's
 * gates hold what the forward's held. After spwgnn_backward_step_gated, spwgnn_backward_relations' drel_steps[s][k]
 * is d loss / d w_{k,s} at these gates and drel[k] its sum over s. */
int32_t spwgnn_forward_step_gated(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                                  void* workspace, int64_t workspace_bytes,
                                  const float* gates /* [mp_steps][gate_step]; NULL = ungated */, int64_t gate_step,
                                  float* logits, float* state_out, spwgnn_stream_t stream);
int32_t spwgnn_backward_step_gated(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                                   void* workspace, int64_t workspace_bytes,
                                   const float* gates /* the forward's; NULL = ungated */, int64_t gate_step,
                                   const float* dlogits, const float* dstate, float* grads, float* dprop,
                                   spwgnn_stream_t stream);

/* DropEdge (added within ABI 8: new symbols only): the relation gates of a random edge subset,
 * drawn per training step — the usual regulariser of a message-passing network, next to the feature dropout of
 * Networks.py:77-78. One launch (kernel id SPWGNN_K_DROPEDGE), no workspace, no host synchronisation: capturable.
 *   gates[k] = base[k] · (keep_k ? scale : 0)       for every edge slot k of the plan, base == NULL meaning 1,
 *   scale    = 1/(1 − rate) in fp32 with SPWGNN_DROPEDGE_RESCALE, else 1,
 *   keep_k   = mix32(rowkey(key, kind 3, tower, a, b) ^ 0) >= floor(rate·2^32)   (the feature dropout's key
 *              functions with kind 3 and feature 0: independent of its two masks, kinds 1 and 2),
 *   tower = node_tower[src_k], a = node_local[src_k], b = node_local[dst_k]; with SPWGNN_DROPEDGE_SYMMETRIC
 *   (a, b) becomes (min, max): the two directions of a contact are kept or dropped together,
 *   key = run->seed, or *run->seed_dev when set (a replayed step's device key word).
 * The key names an edge by its tower's id and its two local node indices alone, so a tower's mask does not depend
 * on plan order, packing, capacity padding, sharding or micro-batching. Every slot of gates [32·n_eblocks] (16-byte
 * aligned, device fp32, the order of spwgnn_forward_gated's gates) is written, a padding slot (edge_src < 0 or
 * edge_dst < 0) with +0 whatever base holds there. Of run only seed, seed_dev and the timing hook are read; of
 * batch n_nodes, n_eblocks, edge_src, edge_dst, node_tower, node_local.
 * SPWGNN_E_ARG before any device work: a null batch, run, gates or one of the four batch arrays, a misaligned
 * pointer, an unknown flag bit, a rate that is NaN or outside [0, 1). rate 0 keeps every edge. */
#define SPWGNN_DROPEDGE_SYMMETRIC 1
#define SPWGNN_DROPEDGE_RESCALE 2
int32_t spwgnn_dropedge_gates(const spwgnn_batch* batch, const spwgnn_run* run, float rate, int32_t flags,
                              const float* base /* [32·n_eblocks], or NULL */,
                              float* gates /* [32·n_eblocks], 16-byte aligned */, spwgnn_stream_t stream);
/* The keep decision of one edge on the host (no device): 1 kept, 0 dropped, SPWGNN_E_ARG for a bad rate or flag.
 * Only SPWGNN_DROPEDGE_SYMMETRIC changes the answer. */
int32_t spwgnn_dropedge_keep_host(uint64_t key, uint32_t tower, uint32_t a, uint32_t b, float rate, int32_t flags);
/* Layer-wise DropEdge: a fresh edge subset at every propagation step. One launch writes the
 * run->mp_steps rows of gates [mp_steps][gate_step] (gate_step as spwgnn_forward_step_gated's): row s is
 * spwgnn_dropedge_gates' mask drawn with feature s of the edge's row key in place of feature 0, so row 0 IS that
 * mask and every row is as independent of the plan as it is. base_step == 0: one base row [32·n_eblocks] (or NULL)
 * multiplied into every row; otherwise base is [mp_steps][base_step], base_step >= 32·n_eblocks and a multiple of
 * 4. Padding slots get +0 in every row; the slots [32·n_eblocks, gate_step) of a row are not written.
 * spwgnn_dropedge_keep_host_step is the host's keep decision of step `step` (step 0: spwgnn_dropedge_keep_host). */
int32_t spwgnn_dropedge_step_gates(const spwgnn_batch* batch, const spwgnn_run* run, float rate, int32_t flags,
                                   const float* base, int64_t base_step, float* gates, int64_t gate_step,
                                   spwgnn_stream_t stream);
int32_t spwgnn_dropedge_keep_host_step(uint64_t key, uint32_t tower, uint32_t a, uint32_t b, uint32_t step, float rate,
                                       int32_t flags);

/* Keras binary_crossentropy on sigmoid(logits) (Networks.py:102), mean over n:
 * out3 = {loss, sum of correct (binary_accuracy numerator), n}; dlogits = dloss/dlogit.
 * scratch: >= spwgnn_bce_scratch_bytes(n) device bytes. Deterministic. */
int64_t spwgnn_bce_scratch_bytes(int64_t n);
int32_t spwgnn_bce(const float* logits, const float* targets, int64_t n, float* out3,
                   float* dlogits, void* scratch, spwgnn_stream_t stream);
/* spwgnn_bce plus spwgnn_accumulate_out3 in the same launch: total3[k] += (double)out3[k] *
 * weights3[k] after out3 is written (model.fit's per-batch progress sums, main.py:92-98). */
int32_t spwgnn_bce_accumulate(const float* logits, const float* targets, int64_t n, float* out3,
                              float* dlogits, void* scratch, const double* weights3, double* total3,
                              spwgnn_stream_t stream);
/* ABI 6: spwgnn_bce (weights3 = total3 = NULL) or spwgnn_bce_accumulate, then spwgnn_backward on the
 * dlogits it wrote — one call, the same results bit for bit (logits: the forward's output on this
 * workspace). Where the backward runs its fused small-batch loop and the loss fits one workgroup
 * (n <= 256, the reference's batch 32), the loop computes dlogits itself (still stored to dlogits)
 * and the loss sums ride in the backward's last launch: a training step needs no loss launch of its
 * own (Keras fit, main.py:92-98). Replaces the Keras loss + autodiff pair of Networks.py:102.
 * SPWGNN_E_ARG unless n == batch->n_nodes (checked before any device work): the folded loss indexes
 * logits, targets and dlogits by plan node. */
int32_t spwgnn_bce_backward(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                            void* workspace, int64_t workspace_bytes, const float* logits,
                            const float* targets, int64_t n, float* out3, float* dlogits, void* bce_scratch,
                            const double* weights3, double* total3, float* grads, float* dprop,
                            spwgnn_stream_t stream);

/* Per-node loss weights (added within ABI 8: new symbols only, no existing struct or signature
 * changed). Keras 2.x weighted_masked_objective with the divisor supplied by the caller:
 *   loss = Σ_i w_i·bce_i / norm,   dlogits_i = w_i·(σ(z_i) − t_i) / norm  (0 where |z_i| >= the clip)
 * with norm = #{i : w_i != 0} for Keras's sample_weight / class_weight (model.fit, main.py:92-98); a
 * per-tower weight is that weight repeated over the tower's nodes. A zero weight is a MASK: the node
 * adds exactly 0 to the loss, gets dlogits_i = 0 and is not counted, whatever its logit and target hold
 * (NaN included). Weights are any finite floats; nothing validates them on the device. The caller gives
 * norm because the gradient needs it before any reduction is done: by value, or in a device float a
 * replayed step refills without recapture. (Keras divides by the count itself and gives NaN for an
 * all-zero batch; a caller passing max(count, 1) gets loss 0 and zero gradients there.)
 * out3 = {loss, correct predictions among the nodes with w != 0, number of nodes with w != 0}: with
 * every weight non-zero that is spwgnn_bce's out3 (Keras's metrics= are unweighted too); with zeros it
 * is the accuracy over the nodes that count — a deviation from Keras's unweighted metric.
 * With w ≡ 1 and norm = n (n < 2^24) every output equals the unweighted call's bit for bit.
 * scratch: >= spwgnn_bce_scratch_bytes(n), as for spwgnn_bce. */
typedef struct spwgnn_loss_weights {
    const float* w;         /* [n] device fp32 per-node weights, in the targets' order */
    const float* norm_dev;  /* device float holding the divisor; NULL = use norm         */
    double norm;            /* the divisor when norm_dev == NULL; must be > 0           */
} spwgnn_loss_weights;
/* spwgnn_bce (weights3 = total3 = NULL) / spwgnn_bce_accumulate with weights. SPWGNN_E_ARG: lw or
 * lw->w NULL, norm <= 0 with norm_dev == NULL, weights3 / total3 not both set or both NULL. */
int32_t spwgnn_bce_weighted(const float* logits, const float* targets, int64_t n, const spwgnn_loss_weights* lw,
                            float* out3, float* dlogits, void* scratch, const double* weights3, double* total3,
                            spwgnn_stream_t stream);
/* spwgnn_bce_backward with weights: spwgnn_bce_weighted then spwgnn_backward in one call, bit for bit.
 * The weighted loss launch runs first on every path — it is not folded into the fused small-batch
 * loop, whose kernel would pay scratch and scalar spills for the extra arguments.
 * Also SPWGNN_E_ARG unless n == batch->n_nodes. */
int32_t spwgnn_bce_backward_weighted(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                                     void* workspace, int64_t workspace_bytes, const float* logits,
                                     const float* targets, int64_t n, float* out3, float* dlogits, void* bce_scratch,
                                     const double* weights3, double* total3, float* grads, float* dprop,
                                     const spwgnn_loss_weights* lw, spwgnn_stream_t stream);

/* Per-step logits and their gradients: deep supervision over the S propagation steps (added within ABI
 * 8: new symbols only, no existing struct or signature changed). Column 0 of the node
 * MLP's output holds a stability logit at EVERY step (Networks.py:89-94); the model reads the last one.
 * Step s's logit of an S-step run is the final logit of the same network run with s + 1 steps.
 *
 * spwgnn_forward_steps: spwgnn_forward_state, with every step's logit row instead of the last one's:
 * step_logits [mp_steps][n_nodes] device fp32, row s = step s, nodes in the plan's order. Row
 * mp_steps − 1 holds the bits spwgnn_forward writes (the last step keeps its shortcuts); the other rows
 * are stores of values the step computed anyway. state_out as in spwgnn_forward_state (NULL = none).
 * Training and inference, every math, every plan kind, every launch path (the fused small-batch loop
 * forms row s from one stride); spwgnn_fused_path's answer holds. */
int32_t spwgnn_forward_steps(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                             void* workspace, int64_t workspace_bytes, float* step_logits /* [mp_steps][n_nodes] */,
                             float* state_out /* [n_nodes][100], or NULL */, spwgnn_stream_t stream);
/* spwgnn_backward_steps: spwgnn_backward_state for Σ_s Σ_i dstep_logits[s][i]·z_s[i] (+ Σ dstate·P_S) in
 * ONE pass over the step loop: step s's node backward puts row s into x' row 100 before dx' is stored
 * and multiplied by Wo2'ᵀ; everything downstream (the omp.1 gradient, dA, the encoders, dprop,
 * spwgnn_backward_inputs, grads_early_event) consumes what it consumed. dstep_logits [mp_steps][n_nodes]
 * device fp32. The last step keeps its "dx' is the logit row alone" shortcut and the earlier steps run
 * the products they always ran, so rows of +0 except the last give spwgnn_backward_state's bits.
 * The forward on this workspace may have been any of spwgnn_forward / _state / _steps (dstate != NULL
 * needs a state_out forward, as for spwgnn_backward_state). */
int32_t spwgnn_backward_steps(const float* params, const spwgnn_batch* batch, const spwgnn_run* run,
                              void* workspace, int64_t workspace_bytes, const float* dstep_logits /* [mp_steps][n_nodes] */,
                              const float* dstate /* [n_nodes][100], or NULL */, float* grads, float* dprop,
                              spwgnn_stream_t stream);

/* The loss of all S rows against one target row: Σ_s λ_s·BCE(z_s, t). One launch (two when n > 256, as
 * spwgnn_bce). The step weights travel by value in spwgnn_step_weights. lw == NULL: row s is spwgnn_bce's
 * arithmetic; lw set: spwgnn_bce_weighted's (same struct, same rules). Outputs:
 *   out3s   [S][3]  each step's {loss, correct, n} as the one-row call writes them (clip and divisor);
 *   out3    [3]     {Σ_s λ_s·loss_s (added in double, step order, zero λ skipped), correct_{S−1}, n_{S−1}};
 *   dlogits [S][n]  row s = λ_s · the one-row call's dlogits; λ_s == 0 writes +0 through a select, so a
 *                   NaN logit in a step of zero weight stays out of the gradient. NULL = not written.
 * With λ = (0, …, 0, 1) out3 and row S − 1 of dlogits are the bits of spwgnn_bce / spwgnn_bce_weighted.
 * weights3 / total3 as in spwgnn_bce_accumulate (both or neither; applied to out3); total3s (NULL = none;
 * needs weights3) [S][3] doubles: += out3s[s][k]·weights3[k] in the same launch — per-step epoch sums.
 * Deterministic (ordered partial sums, no atomics). scratch >= spwgnn_bce_steps_scratch_bytes(n, S).
 * SPWGNN_E_ARG: a null required pointer, n < 1, mp_steps outside 1..64, sw->count != mp_steps, a negative
 * or non-finite λ, λ all zero, lw given but invalid, weights3 / total3 not paired, total3s without them. */
typedef struct spwgnn_step_weights {
    int32_t count;       /* = mp_steps */
    int32_t reserved;    /* 0 */
    float lambda[64];    /* λ_s >= 0 for s < count; the rest is ignored */
} spwgnn_step_weights;
int64_t spwgnn_bce_steps_scratch_bytes(int64_t n, int32_t mp_steps);
int32_t spwgnn_bce_steps(const float* step_logits /* [mp_steps][n] */, const float* targets /* [n] */, int64_t n,
                         int32_t mp_steps, const spwgnn_step_weights* sw, const spwgnn_loss_weights* lw,
                         float* out3s, float* out3, float* dlogits, void* scratch, const double* weights3,
                         double* total3, double* total3s, spwgnn_stream_t stream);

/* Keras-2.x Adam (Networks.py:101: lr=5e-4, decay=0): in-place on the flat buffer.
 * g' = grad_scale*grad + 2*l2*param; lr_t = lr*sqrt(1-b2^t)/(1-b1^t);
 * m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2; p -= lr_t m/(sqrt(v)+eps). step = t >= 1. */
int32_t spwgnn_adam(float* params, const float* grads, float* m, float* v, int64_t n, int32_t step,
                    float lr, float beta1, float beta2, float eps, float l2, float grad_scale,
                    spwgnn_stream_t stream);

/* Replayable (hipGraph-captured) training steps: the per-step scalars live on the device.
 * spwgnn_step_advance (one thread, stream-ordered) starts a step: *step_dev += 1 and the dropout
 * key *key_dev becomes, for mode
 *   SPWGNN_STEP_KEY_COUNTER   *key_dev + 1  (the Keras front end's per-step seed counter), or
 *   SPWGNN_STEP_KEY_SPLITMIX  splitmix64 chain of (seed, step before the increment, rank, 0)
 *                             (spwgnn_amd.trainer.dropout_key — the Trainer's key).
 * spwgnn_adam_dev is spwgnn_adam with the step read from *step_dev and lr_t = lr_table[step]
 * (table_len entries, clamped), the table filled on the host by spwgnn_adam_lr_table with the
 * expression spwgnn_adam evaluates, so replayed and eager steps agree bit for bit. */
#define SPWGNN_STEP_KEY_COUNTER 0
#define SPWGNN_STEP_KEY_SPLITMIX 1
int32_t spwgnn_step_advance(uint64_t* key_dev, int32_t* step_dev, int32_t mode, uint64_t seed, int32_t rank,
                            spwgnn_stream_t stream);
int32_t spwgnn_adam_lr_table(float lr, float beta1, float beta2, int32_t n, float* out_host);
int32_t spwgnn_adam_dev(float* params, const float* grads, float* m, float* v, int64_t n, const int32_t* step_dev,
                        const float* lr_table, int32_t table_len, float beta1, float beta2, float eps, float l2,
                        float grad_scale, spwgnn_stream_t stream);

/* clipnorm, clipvalue, decay and a non-finite guard for the Adam step (added within ABI 8: new symbols
 * only; spwgnn_adam and spwgnn_adam_dev are unchanged). Keras 2.x Optimizer.get_gradients plus Adam's
 * `decay` (Networks.py:101 spells decay=0.0 out), restated — unpinned like the rest:
 *   g'   = grad_scale*grad + 2*l2*param                     (what spwgnn_adam forms; Keras's L2 is in its loss)
 *   norm = sqrt(Σ g'^2) over the REAL parameters: the ranges of spwgnn_param_tensor. The 64-float
 *          alignment padding between tensors is neither summed nor checked, whatever it holds.
 *   clipnorm  c > 0 and norm >= c:  g' *= c / norm; otherwise the applied scale is exactly 1.0f
 *   clipvalue v > 0:                g'  = clamp(g', -v, v), after clipnorm (a NaN stays a NaN)
 *   m, v, p  updated from that g' with spwgnn_adam's expressions.
 *   skip_nonfinite (not in Keras): when the computed Σ g'^2 is NaN or inf — a non-finite gradient, or a
 *          sum that overflows fp32 (|g'| above ~1.8e19 does) — the step writes nothing to params, m
 *          or v. The step COUNT is not held back: a replayed step advances its device step word in
 *          the forward's first launch, before the gradient exists, and the host mirror cannot learn
 *          of a skip without a sync; so a skipped step still uses up iteration t (bias correction and
 *          decay move on). Without the flag non-finite values propagate as in Keras.
 * `grads` is never modified. Two launches, one more than spwgnn_adam: 64 fixed blocks write partial
 * sums of Σ g'^2 (a per-thread strided sum of 13 terms, then a 256-wide tree; no atomics), and
 * every block of the update adds the 64 partials in the same order in double — the same bits in every
 * block, on every run and every device — before it applies the scale. Capturable.
 * out4 (device, required) = {norm, applied scale, skipped 0/1, clipped by norm 0/1 (0 on a skipped step)}.
 * total4 (device fp64, optional): += {norm if not skipped, clipped, skipped, 1} in the same launch, as
 * spwgnn_bce_accumulate does for the loss (model.fit's per-epoch sums without a host sync). */
typedef struct spwgnn_clip {
    float clipnorm;          /* c >= 0; 0 = off                                              */
    float clipvalue;         /* v >= 0; 0 = off                                              */
    int32_t skip_nonfinite;  /* 1: a step with a non-finite Σ g'^2 leaves params, m, v alone */
    int32_t reserved;        /* 0                                                            */
    float* out4;             /* device, 4 floats                                             */
    double* total4;          /* device, 4 doubles; NULL = none                               */
} spwgnn_clip;
/* Device bytes of the partial sums (`scratch` below; 4-byte aligned). */
int64_t spwgnn_clip_scratch_bytes(void);
/* spwgnn_adam's arguments plus the options and the scratch. SPWGNN_E_ARG before any launch: a null
 * pointer (clip, clip->out4 and scratch included), n != spwgnn_param_count() (the real ranges are the
 * library's own table), step < 1, a negative or NaN clipnorm / clipvalue. `lr` is the step's own: a
 * decayed one comes from spwgnn_adam_lr_decayed. */
int32_t spwgnn_adam_clipped(float* params, const float* grads, float* m, float* v, int64_t n, int32_t step,
                            float lr, float beta1, float beta2, float eps, float l2, float grad_scale,
                            const spwgnn_clip* clip, void* scratch, spwgnn_stream_t stream);
/* The same with spwgnn_adam_dev's step word and lr table (also E_ARG: step_dev / lr_table NULL,
 * table_len < 2). With decay the table is spwgnn_adam_lr_table_decay's. */
int32_t spwgnn_adam_clipped_dev(float* params, const float* grads, float* m, float* v, int64_t n,
                                const int32_t* step_dev, const float* lr_table, int32_t table_len, float beta1,
                                float beta2, float eps, float l2, float grad_scale, const spwgnn_clip* clip,
                                void* scratch, spwgnn_stream_t stream);
/* Keras 2.x Adam's decay (host): lr_eff = lr * 1/(1 + decay*iterations), evaluated in double and
 * rounded to fp32 once; iterations = the steps already taken (0 at the first step, t - 1 at step t).
 * decay <= 0 (or NaN) or iterations <= 0 returns lr itself. */
float spwgnn_adam_lr_decayed(float lr, float decay, int64_t iterations);
/* spwgnn_adam_lr_table with entry t built from spwgnn_adam_lr_decayed(lr, decay, t - 1): an eager step
 * that passes that lr to spwgnn_adam(_clipped) and a replayed one agree bit for bit; decay = 0 gives
 * spwgnn_adam_lr_table's bits. The device clamps the step at the table's last entry, so the decay
 * FREEZES there (the Python layer's tables hold 2^20 steps). SPWGNN_E_ARG also for decay < 0 or NaN. */
int32_t spwgnn_adam_lr_table_decay(float lr, float decay, float beta1, float beta2, int32_t n, float* out_host);

/* Epoch sums of model.fit's progress line (main.py:92-98): total3[k] += (double)out3[k] * weights3[k]
 * for k < 3 (out3 = spwgnn_bce's [loss, correct, n]; weights (n, 1, 1) make Σ loss·n) — one launch,
 * replayable, no host sync. */
int32_t spwgnn_accumulate_out3(const float* out3, const double* weights3, double* total3, spwgnn_stream_t stream);

/* Sigmoid readout (Networks.py:93-96) for predict(): probs[i] = 1/(1+exp(-logits[i])). */
int32_t spwgnn_sigmoid(const float* logits, float* probs, int64_t n, spwgnn_stream_t stream);

/* dev[0, bytes) ← host[0, bytes) by a kernel on `stream` (not a DMA copy): `host` must be pinned,
 * device-mapped memory (hipHostMalloc), both pointers 16-byte aligned, bytes a multiple of 16. A
 * replayed small-batch step makes it its first node, so the batch upload rides inside the graph. */
int32_t spwgnn_copy_in(const void* host, void* dev, int64_t bytes, spwgnn_stream_t stream);
/* The device address of pinned, device-mapped host memory (hipHostGetDevicePointer through the HIP
 * runtime this library runs on — the one the caller's allocator used), for spwgnn_copy_in and
 * spwgnn_prologue.copy_src. 0, or the hipError_t of a host range that is not device-mapped. */
int32_t spwgnn_host_device_ptr(const void* host, void** dev);

/* Per-tower readout over contiguous node ranges [tower_offsets[t], tower_offsets[t+1]):
 *   SUM_PROB   out[t] = Σ sigmoid(z)  — the stability sum of JengaBuilder.remove_to_demolish /
 *              TowerCreator.drop_to_demolish (JengaBuilder.py:252-256, TowerCreator.py:298-301),
 *              evaluated for a whole batch of candidate towers in one call;
 *   MEAN_PROB  the optional GlobalBlock-style mean pool (not in the reference);
 *   SUM_LOGIT / MEAN_LOGIT on the logits.
 * Summed sequentially in node order (deterministic). tower_offsets: n_towers + 1 int32, device. */
enum {
    SPWGNN_READOUT_SUM_PROB = 0,
    SPWGNN_READOUT_MEAN_PROB = 1,
    SPWGNN_READOUT_SUM_LOGIT = 2,
    SPWGNN_READOUT_MEAN_LOGIT = 3
};
int32_t spwgnn_tower_readout(const float* logits, const int32_t* tower_offsets, int32_t n_towers, int32_t mode,
                             float* out, spwgnn_stream_t stream);

/* Evaluation tables (added within ABI 8: new symbols only). model.evaluate's counts on
 * the device: the node confusion of (s > 0.5) == c (JengaBuilder.py:333-346), the per-tower and
 * per-tower-size confusions the paper tabulates and a logit histogram per class for ROC
 * curves. Every table is caller-zeroed int64 device memory, 8-byte aligned, and is ADDED TO: a data set
 * evaluated in batches is read once at the end, ranks combine tables by an integer sum. One launch, no
 * allocation, no synchronisation, no scratch; capturable. Integer sums: the same bits on every run.
 *
 * Row r, node i counted (w == NULL or w[i] != 0), z = logits[r][i], t = targets[i]:
 *   p = 1.f / (1.f + expf(-z))  (spwgnn_bce's expression);  pred = p > threshold (false for a NaN);
 *   ok = (pred ? 1.f : 0.f) == t;  the cell is TP (pred, ok), FP (pred, !ok), TN (!pred, ok), FN (!pred, !ok)
 *   — targets are 0 or 1; any other value counts as a wrong prediction on the predicted side.
 *   With threshold 0.5, TP + TN = out3[1] and the cell sum = out3[2] of spwgnn_bce / spwgnn_bce_weighted.
 *   bin = isnan(z) ? 0 : (int)floorf((fminf(fmaxf(z, -16.f), 15.9375f) + 16.f) * 8.f): 1/8-logit bins over
 *   [-16, 16) with the ends clamped; hist[r][t == 1.f][bin] += 1.
 * Tower u = nodes [tower_offsets[u], tower_offsets[u+1]) (every range is clamped to [0, n) before it is
 * walked; the offsets are the caller's contract: nondecreasing, from 0 to n). A tower with no counted node
 * is skipped. Otherwise exact = every counted node ok, pstable = every counted node pred, astable = every
 * counted t == 1.f; tower6 gets the tower, exact and the (pstable, astable) cell; by_size[r][k], k =
 * the tower's node count when that is 1..32 and 0 for any other size, gets the tower's node cells, the
 * tower and exact.
 * SPWGNN_E_ARG before any device work: a null logits, targets, ev or node4; n < 1; rows outside 1..64; a
 * threshold that is NaN or outside (0, 1); reserved != 0; n_towers < 0; n_towers > 0 without tower_offsets
 * or with neither tower6 nor by_size; n_towers == 0 with any of those three set; a table that is not
 * 8-byte aligned. */
#define SPWGNN_EVAL_BINS 256
#define SPWGNN_EVAL_SIZES 33           /* bucket k = towers of k nodes, 1..32; bucket 0 = any other size */
typedef struct spwgnn_eval {
    int32_t rows;        /* R in 1..64 logit rows scored against ONE target row: 1, or mp_steps for the
                            rows of spwgnn_forward_steps */
    int32_t n_towers;    /* 0 = node tables only */
    float threshold;     /* tau, finite, 0 < tau < 1; 0.5 is the reference's (JengaBuilder.py:343) */
    int32_t reserved;    /* 0 */
    const float* w;              /* [n] per-node weights or NULL; w == 0 masks the node out of EVERY table
                                    (a select, as in spwgnn_bce_weighted: NaN under it stays out) */
    const int32_t* tower_offsets;/* [n_towers+1], as spwgnn_tower_readout takes them */
    int64_t* node4;      /* [R][4]      += TP, TN, FP, FN                       (required)  */
    int64_t* tower6;     /* [R][6]      += towers, exact, tTP, tTN, tFP, tFN    (NULL = none) */
    int64_t* by_size;    /* [R][33][6]  += TP, TN, FP, FN, towers, exact        (NULL = none) */
    int64_t* hist;       /* [R][2][256] += logit histogram per class            (NULL = none) */
} spwgnn_eval;
int32_t spwgnn_eval_metrics(const float* logits /* [R][n] */, const float* targets /* [n] */, int64_t n,
                            const spwgnn_eval* ev, spwgnn_stream_t stream);

/* Tower-level loss (added within ABI 8: new symbols only). A binary cross-entropy on
 * "the whole tower stands", with the noisy-AND likelihood spwgnn_eval_metrics' tower tables imply: the
 * probability that every counted block of tower u stands is P_u = Π σ(z_i). A data set that records only
 * whether a tower stood or fell (the label of JengaBuilder.py:333-346 taken per tower) trains on it.
 *
 * Tower u = nodes [tower_offsets[u], tower_offsets[u+1]) as in spwgnn_eval_metrics (every range clamped
 * to [0, n) before it is walked; the offsets are the caller's contract: nondecreasing, from 0 to n —
 * dlogits of a node that lies in no tower is not written). Node i is counted when lw == NULL or
 * lw->w[i] != 0 (a select: NaN under a zero weight stays out); a tower with no counted node is skipped.
 *   q_i = max(−z_i, 0) + log1pf(expf(−|z_i|))         (−log σ(z_i))
 *   s_u = −Σ q_i over the counted nodes, in fp32, in node order           (log P_u)
 *   T_u = tower_targets[u] == 1.f, or without tower_targets: every counted targets[i] == 1.f
 *   lo = logf(1e-7f), hi = log1pf(−1e-7f), s~ = clamp(s_u, lo, hi), inside = lo < s_u < hi
 *   l_u = T_u ? −s~ : −log1mexp(s~),  log1mexp(x) = x > −ln 2 ? logf(−expm1f(x)) : log1pf(−expf(x))
 *   g_u = inside ? (T_u ? −1 : 1 / expm1f(−s_u)) : 0
 *   L_tower = Σ_u l_u / norm_t;  d_tower_i = ((mu·g_u)·(1 / (1 + expf(z_i)))) / norm_t  (counted nodes)
 * (Keras's clip of the probability to [1e-7, 1 − 1e-7], Networks.py:102, applied to P_u.) A tower is
 * correct when (every counted σ(z_i) > 0.5) == T_u: with derived targets, tower6's tTP + tTN at 0.5.
 * The objective is L = alpha·L_node + mu·L_tower with L_node spwgnn_bce's loss (lw NULL) or
 * spwgnn_bce_weighted's (lw set: its weights and divisor), and
 *   dlogits_i = alpha·d_node_i + d_tower_i   (each product and the sum rounded on its own; d_node_i the
 *   dlogits of those calls; alpha == 0 and a tower outside the clip are selects, not products).
 * out6 = {L_node, node correct, node count, L_tower, towers correct, towers counted}; its first three
 * hold the bits spwgnn_bce / spwgnn_bce_weighted write to out3 for the same inputs. out3 = {L, node
 * correct, node count}. alpha == 0 with tower_targets allows targets == NULL (tower-only labels): the node
 * row is then {0, 0, counted nodes}. dlogits may be NULL (loss only).
 * The sums are per-workgroup fp32 partials added in workgroup order in double: no atomics, the same bits
 * on every run. One launch when n <= 256 and n_towers <= 256, otherwise two. No allocation, no
 * synchronisation; capturable. scratch: >= spwgnn_bce_tower_scratch_bytes(n, n_towers) device bytes.
 * SPWGNN_E_ARG before any device work: a null logits, tl, out3, scratch, tl->tower_offsets or tl->out6;
 * targets NULL unless alpha == 0 and tower_targets is set; n < 1; n_towers < 1; reserved != 0; mu <= 0
 * or not finite; alpha < 0 or not finite; norm_t <= 0 without norm_t_dev; weights6 / total6 not both set
 * or both NULL; lw set but not a valid spwgnn_loss_weights. */
typedef struct spwgnn_tower_loss {
    int32_t n_towers;
    int32_t reserved;              /* 0 */
    const int32_t* tower_offsets;  /* [n_towers+1] device int32 */
    const float* tower_targets;    /* [n_towers] device fp32 0/1, or NULL = derived from targets */
    float alpha, mu;               /* alpha >= 0, mu > 0 */
    const float* norm_t_dev;       /* device float holding the tower divisor; NULL = use norm_t */
    double norm_t;                 /* the divisor (the counted towers) when norm_t_dev == NULL; > 0 */
    float* out6;                   /* [6] device */
    float* per_tower;              /* [n_towers] device: l_u (0 for a skipped tower), or NULL = none */
    const double* weights6;        /* with total6: total6[k] += (double)out6[k] * weights6[k], same launch */
    double* total6;
} spwgnn_tower_loss;
int64_t spwgnn_bce_tower_scratch_bytes(int64_t n, int32_t n_towers);
int32_t spwgnn_bce_tower(const float* logits, const float* targets, int64_t n,
                         const spwgnn_loss_weights* lw /* or NULL */, const spwgnn_tower_loss* tl, float* out3,
                         float* dlogits, void* scratch, spwgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPWGNN_H */
