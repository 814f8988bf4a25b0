// d(loss)/d(objects): the last linear map of the backward, from the first encoder layers'
// pre-activation gradients back to the node positions.
//   per edge e = (s → r):  q_e = dz1_e · W_rm0ᵀ   (d = pos[r].xy − pos[s].xy, Networks.py:58-62)
//   per node n:            p_n = dzo1_n · W_om0ᵀ  (o = (pos.y, pos.w),        Networks.py:65-71)
//   dpos[n] = (Σ_{r=n} q.x − Σ_{s=n} q.x,  Σ_{r=n} q.y − Σ_{s=n} q.y + p_n[0],  p_n[1],  0)
// A stream over the stored rows on the vector ALUs: 4 FLOPs per element against 4 (bf16 storage: 2)
// bytes of it. One wave owns a wave-tile — whole towers, so every edge of its nodes lies in its own
// blocks, in ordinary, capacity-padded and receiver-block plans alike. Lane (i, h) reads half h of
// row i, one chunk-major piece (16 bytes; a wave's load is 1 KiB contiguous) at a time, each stored
// row exactly once; the two halves meet in one cross-lane move. The wave then adds ±q_e into
// per-node register accumulators (lane n: x of node n, lane 32 + n: y) in plan order, edge by edge:
// no floating-point atomics, the same bits on every run. Every row of dpos is written, rows of
// nodes without edges included; nothing is written outside [0, n_nodes).
#include "kernels.h"

namespace spw {

constexpr int kInQE = kKhE / 4;   // 19 pieces per half of an edge row
constexpr int kInQN = kKhN / 4;   // 13 pieces per half of a node row

template <bool B16>
__global__ __launch_bounds__(256) void k_input_bwd(InputBwdArgs a) {
    // wE[h][q][k]: rm.0.kernel[k][76h + 4q .. + 3] (features ≥ 150: 0); wN the same for om.0 (KH = 52)
    __shared__ float4 wE[2][kInQE][2];
    __shared__ float4 wN[2][kInQN][2];
    __shared__ float2 qs[4][32];   // per wave: q_e of the block in flight
    __shared__ int2 ix[4][32];     //           its (sender, receiver) as tile-local node indices, -1 = none
    const int tid = threadIdx.x;
    if (tid < 2 * kInQE * 2 + 2 * kInQN * 2) {
        const bool edge = tid < 2 * kInQE * 2;
        const int t = edge ? tid : tid - 2 * kInQE * 2;
        const int nq = edge ? kInQE : kInQN, kh = edge ? kKhE : kKhN, width = edge ? kFE : kFN;
        const int h = t / (2 * nq), q = (t % (2 * nq)) >> 1, k = t & 1;
        const float* w = (edge ? a.w_rm0 : a.w_om0) + k * width;
        const int f = kh * h + 4 * q;
        const float4 v = make_float4(f < width ? w[f] : 0.f, f + 1 < width ? w[f + 1] : 0.f,
                                     f + 2 < width ? w[f + 2] : 0.f, f + 3 < width ? w[f + 3] : 0.f);
        if (edge) wE[h][q][k] = v;
        else wN[h][q][k] = v;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, i = lane & 31, h = lane >> 5;
    const int w = blockIdx.x * 4 + wave;
    if (w >= a.n_wtiles) return;
    const int b0 = __builtin_amdgcn_readfirstlane(a.wtile[4 * w]);
    const int nb = __builtin_amdgcn_readfirstlane(a.wtile[4 * w + 1]);
    const int n0 = __builtin_amdgcn_readfirstlane(a.wtile[4 * w + 2]);
    const int nn = __builtin_amdgcn_readfirstlane(a.wtile[4 * w + 3]);
    // a plan this kernel cannot serve writes nothing (never out of bounds)
    if (b0 < 0 || nb < 0 || nb > a.n_eblocks - b0 || n0 < 0 || nn < 0 || nn > 32 || nn > a.n_nodes - n0) return;

    float acc = 0.f;   // lane (n, h): d/dx (h = 0) or d/dy (h = 1) of node n0 + n, edge part
    for (int blk = b0; blk < b0 + nb; ++blk) {
        const int64_t e = (int64_t)blk * 32 + i;
        const int s = a.esrc[e], d = a.edst[e];
        const bool ok = s >= 0 && d >= 0;
        if (__ballot(ok) == 0) continue;   // an all-padding block (capacity plans): no row to read
        float4 y[kInQE];
        if constexpr (B16) {
            const uint16_t* row = reinterpret_cast<const uint16_t*>(a.dz1) + (int64_t)blk * kCmBlk + (h * 32 + i) * 4;
#pragma unroll
            for (int q = 0; q < kInQE; ++q) y[q] = unpack4_bf16(*reinterpret_cast<const uint2*>(row + q * 256));
        } else {
            const float* row = a.dz1 + (int64_t)blk * kCmBlk + (h * 32 + i) * 4;
#pragma unroll
            for (int q = 0; q < kInQE; ++q) y[q] = *reinterpret_cast<const float4*>(row + q * 256);
        }
        // features 150, 151 are the row's padding: never multiplied (a stored NaN must not reach q)
        if (h) y[kInQE - 1].z = y[kInQE - 1].w = 0.f;
        float q0 = 0.f, q1 = 0.f;
#pragma unroll
        for (int q = 0; q < kInQE; ++q) {
            const float4 w0 = wE[h][q][0], w1 = wE[h][q][1];
            q0 = __builtin_fmaf(y[q].x, w0.x, q0);
            q0 = __builtin_fmaf(y[q].y, w0.y, q0);
            q0 = __builtin_fmaf(y[q].z, w0.z, q0);
            q0 = __builtin_fmaf(y[q].w, w0.w, q0);
            q1 = __builtin_fmaf(y[q].x, w1.x, q1);
            q1 = __builtin_fmaf(y[q].y, w1.y, q1);
            q1 = __builtin_fmaf(y[q].z, w1.z, q1);
            q1 = __builtin_fmaf(y[q].w, w1.w, q1);
        }
        q0 += __shfl_xor(q0, 32, 64);
        q1 += __shfl_xor(q1, 32, 64);
        if (h == 0) {   // a padding row holds whatever its producer left: it gives no term
            qs[wave][i] = ok ? make_float2(q0, q1) : make_float2(0.f, 0.f);
            ix[wave][i] = ok ? make_int2(s - n0, d - n0) : make_int2(-1, -1);
        }
        wave_lds_sync();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {   // plan order: +q at the receiver, −q at the sender
            const int2 sd = ix[wave][k];
            const float2 qk = qs[wave][k];
            const float v = h ? qk.y : qk.x;
            if (sd.y == i) acc += v;
            if (sd.x == i) acc -= v;
        }
        wave_lds_sync();
    }

    // node part: row n0 + i of the 32-node blocks (a tile's nodes may straddle two of them)
    const bool has = i < nn;
    const int n = n0 + (has ? i : 0);
    float p0 = 0.f, p1 = 0.f;
    if (has) {
        const float* row = a.dzo1 + (int64_t)(n >> 5) * kCmBlkN + (h * 32 + (n & 31)) * 4;
        float4 y[kInQN];
#pragma unroll
        for (int q = 0; q < kInQN; ++q) y[q] = *reinterpret_cast<const float4*>(row + q * 256);
        if (h) y[kInQN - 1] = make_float4(0.f, 0.f, 0.f, 0.f);   // features 100..103: padding
#pragma unroll
        for (int q = 0; q < kInQN; ++q) {
            const float4 w0 = wN[h][q][0], w1 = wN[h][q][1];
            p0 = __builtin_fmaf(y[q].x, w0.x, p0);
            p0 = __builtin_fmaf(y[q].y, w0.y, p0);
            p0 = __builtin_fmaf(y[q].z, w0.z, p0);
            p0 = __builtin_fmaf(y[q].w, w0.w, p0);
            p1 = __builtin_fmaf(y[q].x, w1.x, p1);
            p1 = __builtin_fmaf(y[q].y, w1.y, p1);
            p1 = __builtin_fmaf(y[q].z, w1.z, p1);
            p1 = __builtin_fmaf(y[q].w, w1.w, p1);
        }
    }
    p0 += __shfl_xor(p0, 32, 64);
    p1 += __shfl_xor(p1, 32, 64);
    const float accy = __shfl_xor(acc, 32, 64);
    if (has && h == 0) a.dpos[n] = make_float4(acc, accy + p0, p1, 0.f);
}

hipError_t launch_input_bwd(const InputBwdArgs& a, hipStream_t st) {
    if (a.n_wtiles <= 0) return hipSuccess;
    const dim3 g((a.n_wtiles + 3) / 4), b(256);
    if (a.b16) hipLaunchKernelGGL((k_input_bwd<true>), g, b, 0, st, a);
    else hipLaunchKernelGGL((k_input_bwd<false>), g, b, 0, st, a);
    return hipGetLastError();
}

}  // namespace spw
