// spwgnn_eval_metrics: the evaluation tables of R logit rows against one target row —
// node confusion, per-tower and per-tower-size confusion, a logit histogram per class — added to the
// caller's int64 tables in ONE launch. Integer sums only: the order of the adds does not matter, so the
// tables hold the same bits on every run without any ordering machinery.
#include "kernels.h"
#include <algorithm>

namespace spw {

constexpr int kEvalNodeBlocks = 512;    // capped grid of the node stream (two workgroups per CU), grid-strided
constexpr int kEvalTowerBlocks = 512;   // ... and of the tower walk (one thread per tower, grid-strided)
constexpr int kEvalHist = 2 * kEvalBins;               // one row's histogram, [class][bin]
constexpr int kEvalSizeCells = kEvalSizes * 6;         // one row's by_size table
constexpr int kEvalLds = kEvalHist + 4;                // node workgroups: the histogram, then the four cells
static_assert(kEvalSizeCells + 6 <= kEvalLds, "the tower workgroups' tables fit the same array");

// One node's verdict, the arithmetic of bce_row_block's accuracy (loss_blocks.h) at a threshold tau:
// the cell index 0 TP, 1 TN, 2 FP, 3 FN. A NaN p predicts "unstable" (p > tau is false).
__device__ __forceinline__ int eval_cell(float z, float t, float tau, bool& pred, bool& ok) {
    const float p = 1.f / (1.f + expf(-z));
    pred = p > tau;
    ok = (pred ? 1.f : 0.f) == t;
    return pred ? (ok ? 0 : 2) : (ok ? 1 : 3);
}
// 1/8-logit bins over [-16, 16), the ends clamped, NaN in bin 0: always in [0, kEvalBins). Power-of-two
// constants: every operation is exact or a single fp32 rounding, the same in numpy float32.
__device__ __forceinline__ int eval_bin(float z) {
    return z != z ? 0 : (int)floorf((fminf(fmaxf(z, -16.f), 15.9375f) + 16.f) * 8.f);
}
// the non-zero entries lds[0, count) of a workgroup's 32-bit table → the global int64 table
__device__ __forceinline__ void eval_flush(const uint32_t* lds, int k0, int count, unsigned long long* dst) {
    if (!dst) return;
    for (int k = threadIdx.x; k < count; k += 256) {
        const uint32_t v = lds[k0 + k];
        if (v) atomicAdd(dst + k, (unsigned long long)v);
    }
}

// Node workgroups: a grid-strided stream of the n nodes per row. Each thread keeps the four cells in
// registers (a workgroup sees at most 256·ceil(n / (256·node_blocks)) nodes per row: 32-bit counts hold for
// any n below 2^41), the waves add them into LDS after a shuffle reduction; the histogram is 32-bit LDS
// atomics. Per row one global add per non-zero entry and workgroup.
__device__ __forceinline__ void eval_nodes(const EvalArgs& a, uint32_t* lds) {
    for (int r = 0; r < a.R; ++r) {
        const float* z_row = a.logits + (int64_t)r * a.n;
        for (int k = threadIdx.x; k < kEvalLds; k += 256) lds[k] = 0;
        __syncthreads();
        uint32_t c[4] = {0, 0, 0, 0};
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)a.node_blocks * 256) {
            const float z = z_row[i], t = a.targets[i];
            const bool on = a.w ? a.w[i] != 0.f : true;   // a select: whatever a masked node holds stays out
            bool pred, ok;
            const int cell = eval_cell(z, t, a.tau, pred, ok);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] += (on && cell == k) ? 1u : 0u;
            if (a.hist && on) atomicAdd(&lds[(t == 1.f ? kEvalBins : 0) + eval_bin(z)], 1u);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_down(c[k], o, 64);
            if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd(&lds[kEvalHist + k], c[k]);
        }
        __syncthreads();
        eval_flush(lds, 0, kEvalHist, a.hist ? a.hist + (int64_t)r * kEvalHist : nullptr);
        eval_flush(lds, kEvalHist, 4, a.node4 + (int64_t)r * 4);
        __syncthreads();   // the next row zeroes the array
    }
}

// Tower workgroups: one thread per tower (grid-strided), walking its nodes in order as k_tower_readout
// does. Every range is clamped to [0, n): a bad offset table cannot read outside the logits. LDS holds
// the row's by_size table [33][6] and, after it, the six tower6 entries (32-bit: a workgroup's towers hold
// fewer than 2^32 nodes — n_towers is an int32 and a tower the network can run has at most 32 nodes).
__device__ __forceinline__ void eval_towers(const EvalArgs& a, uint32_t* lds) {
    const int64_t tb = (int64_t)blockIdx.x - a.node_blocks, ntb = (int64_t)gridDim.x - a.node_blocks;
    for (int r = 0; r < a.R; ++r) {
        const float* z_row = a.logits + (int64_t)r * a.n;
        for (int k = threadIdx.x; k < kEvalSizeCells + 6; k += 256) lds[k] = 0;
        __syncthreads();
        for (int64_t u = tb * 256 + threadIdx.x; u < a.n_towers; u += ntb * 256) {
            const int64_t o0 = a.off[u], o1 = a.off[u + 1];
            const int64_t b = std::min<int64_t>(std::max<int64_t>(o0, 0), a.n), e = std::min<int64_t>(std::max<int64_t>(o1, 0), a.n);
            uint32_t c[4] = {0, 0, 0, 0}, counted = 0;
            bool exact = true, pstable = true, astable = true;
            for (int64_t i = b; i < e; ++i) {
                if (a.w && !(a.w[i] != 0.f)) continue;
                const float t = a.targets[i];
                bool pred, ok;
                const int cell = eval_cell(z_row[i], t, a.tau, pred, ok);
#pragma unroll
                for (int k = 0; k < 4; ++k) c[k] += cell == k ? 1u : 0u;
                ++counted;
                exact = exact && ok;
                pstable = pstable && pred;
                astable = astable && t == 1.f;
            }
            if (!counted) continue;   // no counted node: the tower is in no table
            if (a.by_size) {
                const int64_t size = o1 - o0;
                uint32_t* q = lds + (size >= 1 && size < kEvalSizes ? (int)size : 0) * 6;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c[k]) atomicAdd(q + k, c[k]);
                atomicAdd(q + 4, 1u);
                if (exact) atomicAdd(q + 5, 1u);
            }
            if (a.tower6) {
                uint32_t* q = lds + kEvalSizeCells;
                atomicAdd(q, 1u);
                if (exact) atomicAdd(q + 1, 1u);
                atomicAdd(q + 2 + (pstable ? (astable ? 0 : 2) : (astable ? 3 : 1)), 1u);   // tTP, tTN, tFP, tFN
            }
        }
        __syncthreads();
        eval_flush(lds, 0, kEvalSizeCells, a.by_size ? a.by_size + (int64_t)r * kEvalSizeCells : nullptr);
        eval_flush(lds, kEvalSizeCells, 6, a.tower6 ? a.tower6 + (int64_t)r * 6 : nullptr);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_eval_metrics(EvalArgs a) {
    __shared__ uint32_t lds[kEvalLds];
    if ((int)blockIdx.x < a.node_blocks) eval_nodes(a, lds);   // uniform per workgroup
    else eval_towers(a, lds);
}

hipError_t launch_eval_metrics(const EvalArgs& a0, hipStream_t st) {
    EvalArgs a = a0;
    a.node_blocks = (int)std::min<int64_t>((a.n + 255) / 256, kEvalNodeBlocks);
    const int tower_blocks = (int)std::min<int64_t>(((int64_t)a.n_towers + 255) / 256, kEvalTowerBlocks);   // 0 without towers
    hipLaunchKernelGGL(k_eval_metrics, dim3((unsigned)(a.node_blocks + tower_blocks)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace spw
