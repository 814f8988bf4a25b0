// Keras BCE loss (one row and per step), the tower-level loss, Keras Adam and its clipped form, the step
// counter, the read-outs, the replayed step's copy-in and the state layout kernels.
#include "kernels.h"
#include "loss_blocks.h"
#include <cstdlib>

namespace spw {

// ------------------------------------------------------------------------------------------------
// The one-row loss (launch_bce): thin kernels around loss_blocks.h. (Run as S = 1 of the per-step kernels
// below it gives the same bits, but their final sum took 27 µs against 18 µs here: DESIGN.md §3zt.)
template <bool W, bool FINAL>
__global__ __launch_bounds__(256) void k_bce_partial(BceArgs a) {
    bce_one_row<W, FINAL>(a, blockIdx.x);
}
template <bool W>
__global__ void k_bce_final(BceArgs a) {
    if (threadIdx.x != 0) return;
    constexpr int P = W ? 3 : 2;
    double ls = 0.0, cs = 0.0, ns = 0.0;
    for (int b = 0; b < a.blocks; ++b) {
        ls += a.partial[P * b];
        cs += a.partial[P * b + 1];
        if constexpr (W) ns += a.partial[P * b + 2];
    }
    float o[3];
    bce_row_store<W>(a.out3, a.tot3, a.w3, ls, cs, ns, W ? bce_norm(a) : 0.f, a.n, o);
}

// The per-step loss: all S logit rows [S][n] against one target row, each row
// loss_blocks.h's bce_row_block / bce_row_store. The combined row is {Σ_{λ_s ≠ 0} λ_s·loss_s summed in
// double in step order, correct_{S−1}, n_{S−1}}: with λ = e_{S−1} it is 0.0 + 1.0·loss_{S−1}, the
// one-row loss's bits.
template <bool W>
__device__ __forceinline__ void bce_steps_block(const BceStepsArgs& a, int s, int blk, float norm, float (&red)[3]) {
    const BceArgs& b = a.b;
    bce_row_block<W>(b.logits + (int64_t)s * b.n, b.dlogits ? b.dlogits + (int64_t)s * b.n : nullptr, b.targets, b.w,
                     b.n, b.blocks, blk, a.lambda[s], norm, red);
}
// Thread 0 only: row s's out3 from its sums, its share of the combined loss into `comb`, and the
// combined row after the last step.
template <bool W>
__device__ __forceinline__ void bce_steps_store(const BceStepsArgs& a, int s, float norm, double ls, double cs,
                                                double ns, double& comb) {
    const BceArgs& b = a.b;
    const float lam = a.lambda[s];
    float o[3];
    bce_row_store<W>(a.out3s + 3 * s, a.tot3s ? a.tot3s + 3 * s : nullptr, b.w3, ls, cs, ns, norm, b.n, o);
    if (lam != 0.f) comb += (double)lam * (double)o[0];
    if (s == a.S - 1) {
        const float c[3] = {(float)comb, o[1], o[2]};
        bce_put3(b.out3, b.tot3, b.w3, c);
    }
}
// b.blocks == 1 (n ≤ 256, the reference's batch 32): one workgroup walks the S rows and finishes
template <bool W>
__global__ __launch_bounds__(256) void k_bce_steps_one(BceStepsArgs a) {
    const float norm = W ? bce_norm(a.b) : (float)a.b.n;
    double comb = 0.0;
    for (int s = 0; s < a.S; ++s) {
        float red[3];
        bce_steps_block<W>(a, s, 0, norm, red);
        if (threadIdx.x == 0) bce_steps_store<W>(a, s, norm, (double)red[0], (double)red[1], W ? (double)red[2] : 0.0, comb);
    }
}
// larger n: grid (blocks, S) of partial sums, then one thread adds each row's partials in block order
template <bool W>
__global__ __launch_bounds__(256) void k_bce_steps_partial(BceStepsArgs a) {
    const int s = blockIdx.y;
    const float norm = W ? bce_norm(a.b) : (float)a.b.n;
    float red[3];
    bce_steps_block<W>(a, s, blockIdx.x, norm, red);
    if (threadIdx.x == 0) {
        float* q = a.b.partial + ((int64_t)s * a.b.blocks + blockIdx.x) * 3;
        q[0] = red[0];
        q[1] = red[1];
        if constexpr (W) q[2] = red[2];
    }
}
template <bool W>
__global__ void k_bce_steps_final(BceStepsArgs a) {
    if (threadIdx.x != 0) return;
    const float norm = W ? bce_norm(a.b) : 0.f;
    double comb = 0.0;
    for (int s = 0; s < a.S; ++s) {
        double ls = 0.0, cs = 0.0, ns = 0.0;
        const float* q = a.b.partial + (int64_t)s * a.b.blocks * 3;
        for (int k = 0; k < a.b.blocks; ++k) {
            ls += q[3 * k];
            cs += q[3 * k + 1];
            if constexpr (W) ns += q[3 * k + 2];
        }
        bce_steps_store<W>(a, s, norm, ls, cs, ns, comb);
    }
}

// ------------------------------------------------------------------------------------------------
// The tower-level loss (spwgnn_bce_tower; the definition is in spwgnn.h). Node workgroups
// [0, b.blocks) run the node row's sums exactly as the one-row loss does (bce_row_block without dlogits:
// the same blocks, the same order, so out6[0:3] carries spwgnn_bce's bits); tower workgroups walk one tower
// per thread, twice: once for s_u, T_u and the prediction, once to write dlogits = alpha·d_node + d_tower
// with d_node recomputed by bce_dlogit / bce_dlogit_w. Every dlogit is written by its tower's thread only.
__device__ __forceinline__ float log1mexp(float x) {
    return x > -0.69314718f ? logf(-expm1f(x)) : log1pf(-expf(x));
}
// a workgroup's tree sum of three values per thread (bce_row_block's tree); thread 0 holds the result
__device__ __forceinline__ void block_sum3(float (&v)[3]) {
    __shared__ float t0[256], t1[256], t2[256];
    t0[threadIdx.x] = v[0];
    t1[threadIdx.x] = v[1];
    t2[threadIdx.x] = v[2];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            t0[threadIdx.x] += t0[threadIdx.x + o];
            t1[threadIdx.x] += t1[threadIdx.x + o];
            t2[threadIdx.x] += t2[threadIdx.x + o];
        }
        __syncthreads();
    }
    v[0] = t0[0];
    v[1] = t1[0];
    v[2] = t2[0];
    __syncthreads();
}
// node workgroup `blk`: red = the node row's {Σ loss, correct, counted}; without targets {0, 0, counted}
template <bool W>
__device__ __forceinline__ void tower_node_block(const TowerLossArgs& a, int blk, float (&red)[3]) {
    const BceArgs& b = a.b;
    if (b.targets) {
        bce_row_block<W>(b.logits, nullptr, b.targets, b.w, b.n, b.blocks, blk, 1.0f, W ? bce_norm(b) : (float)b.n, red);
        return;
    }
    red[0] = red[1] = red[2] = 0.f;
    if constexpr (W) {
        for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < b.n; i += (int64_t)b.blocks * 256)
            red[2] += b.w[i] != 0.f ? 1.f : 0.f;
        block_sum3(red);
    }
}
// tower workgroup `blk` of a.tblocks: red = {Σ l_u, towers correct, towers counted} over its towers
template <bool W>
__device__ __forceinline__ void tower_block(const TowerLossArgs& a, int blk, float (&red)[3]) {
#pragma clang fp contract(off)   // every product and sum below is rounded on its own (spwgnn.h)
    const BceArgs& b = a.b;
    const float lo = logf(1e-7f), hi = log1pf(-1e-7f);
    const float norm_t = a.norm_t_dev ? *a.norm_t_dev : a.norm_t;
    const float inv_n = 1.0f / (W ? bce_norm(b) : (float)b.n);
    red[0] = red[1] = red[2] = 0.f;
    for (int64_t u = (int64_t)blk * 256 + threadIdx.x; u < a.n_towers; u += (int64_t)a.tblocks * 256) {
        const int64_t o0 = a.off[u], o1 = a.off[u + 1];
        const int64_t bg = std::min<int64_t>(std::max<int64_t>(o0, 0), b.n), en = std::min<int64_t>(std::max<int64_t>(o1, 0), b.n);
        float qs = 0.f;
        int counted = 0;
        bool pstable = true, astable = true;
        for (int64_t i = bg; i < en; ++i) {
            if constexpr (W)
                if (!(b.w[i] != 0.f)) continue;
            const float z = b.logits[i];
            qs = __fadd_rn(qs, __fadd_rn(fmaxf(-z, 0.f), log1pf(expf(-fabsf(z)))));
            pstable = pstable && 1.f / (1.f + expf(-z)) > 0.5f;
            if (!a.ttargets) astable = astable && b.targets[i] == 1.f;
            ++counted;
        }
        float l = 0.f, g = 0.f;
        bool inside = false;
        if (counted) {
            const bool T = a.ttargets ? a.ttargets[u] == 1.f : astable;
            const float s = -qs;
            const float sc = s < lo ? lo : (s > hi ? hi : s);   // selects: a NaN sum stays a NaN loss
            inside = lo < s && s < hi;
            l = T ? -sc : -log1mexp(sc);
            g = inside ? (T ? -1.f : 1.f / expm1f(-s)) : 0.f;
            red[0] += l;
            red[1] += pstable == T ? 1.f : 0.f;
            red[2] += 1.f;
        }
        if (a.per_tower) a.per_tower[u] = l;
        if (!a.dlogits) continue;
        const float c = __fmul_rn(a.mu, g);
        for (int64_t i = bg; i < en; ++i) {
            const float z = b.logits[i];
            bool on = true;
            float dn = 0.f;
            if constexpr (W) {
                const float w = b.w[i];
                on = w != 0.f;
                if (b.targets) dn = bce_dlogit_w(z, b.targets[i], w, inv_n);
            } else {
                if (b.targets) dn = bce_dlogit(z, b.targets[i], inv_n);
            }
            float d = a.alpha != 0.f ? __fmul_rn(a.alpha, dn) : 0.f;
            if (on && inside) d = __fadd_rn(d, __fdiv_rn(__fmul_rn(c, 1.f / (1.f + expf(z))), norm_t));
            a.dlogits[i] = d;
        }
    }
    block_sum3(red);
}
// One thread: out6, out3 and the totals from the node row's sums and the towers' sums (both in double)
template <bool W>
__device__ __forceinline__ void tower_store(const TowerLossArgs& a, const double (&ns)[3], const double (&ts)[3]) {
#pragma clang fp contract(off)
    const BceArgs& b = a.b;
    float o[6];
    if (b.targets) {
        float o3[3];
        bce_row_store<W>(a.out6, nullptr, nullptr, ns[0], ns[1], ns[2], W ? bce_norm(b) : 0.f, b.n, o3);
        o[0] = o3[0], o[1] = o3[1], o[2] = o3[2];
    } else {
        o[0] = o[1] = 0.f;
        o[2] = W ? (float)ns[2] : (float)b.n;
    }
    const float norm_t = a.norm_t_dev ? *a.norm_t_dev : a.norm_t;
    o[3] = (float)(ts[0] / (double)norm_t);
    o[4] = (float)ts[1];
    o[5] = (float)ts[2];
    for (int k = 0; k < 6; ++k) {
        a.out6[k] = o[k];
        if (a.tot6) a.tot6[k] += (double)o[k] * a.w6[k];
    }
    a.out3[0] = (float)((double)a.alpha * (double)o[0] + (double)a.mu * (double)o[3]);
    a.out3[1] = o[1];
    a.out3[2] = o[2];
}
// n <= 256 and n_towers <= 256 (the reference's batch): one workgroup, one launch
template <bool W>
__global__ __launch_bounds__(256) void k_bce_tower_one(TowerLossArgs a) {
    float nr[3], tr[3];
    tower_node_block<W>(a, 0, nr);
    tower_block<W>(a, 0, tr);
    if (threadIdx.x != 0) return;
    const double ns[3] = {(double)nr[0], (double)nr[1], W ? (double)nr[2] : 0.0};
    const double ts[3] = {(double)tr[0], (double)tr[1], (double)tr[2]};
    tower_store<W>(a, ns, ts);
}
template <bool W>
__global__ __launch_bounds__(256) void k_bce_tower_partial(TowerLossArgs a) {
    const int nb = a.b.blocks;
    float red[3];
    const bool node = (int)blockIdx.x < nb;   // uniform per workgroup
    if (node) tower_node_block<W>(a, blockIdx.x, red);
    else tower_block<W>(a, (int)blockIdx.x - nb, red);
    if (threadIdx.x != 0) return;
    float* q = node ? a.b.partial + 3 * blockIdx.x : a.tpartial + 3 * ((int)blockIdx.x - nb);
    q[0] = red[0];
    q[1] = red[1];
    q[2] = node && !W ? 0.f : red[2];
}
template <bool W>
__global__ void k_bce_tower_final(TowerLossArgs a) {
    if (threadIdx.x != 0) return;
    double ns[3] = {0.0, 0.0, 0.0}, ts[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < a.b.blocks; ++k)
        for (int j = 0; j < 3; ++j) ns[j] += a.b.partial[3 * k + j];
    for (int k = 0; k < a.tblocks; ++k)
        for (int j = 0; j < 3; ++j) ts[j] += a.tpartial[3 * k + j];
    tower_store<W>(a, ns, ts);
}
hipError_t launch_bce_tower(const TowerLossArgs& a, hipStream_t st) {
    if (a.b.blocks < 1 || a.tblocks < 1 || a.tblocks > kTowerBlocksMax) return hipErrorInvalidValue;
    const dim3 b(256);
    if (a.b.blocks == 1 && a.tblocks == 1) {
        if (a.b.w) hipLaunchKernelGGL(k_bce_tower_one<true>, dim3(1), b, 0, st, a);
        else hipLaunchKernelGGL(k_bce_tower_one<false>, dim3(1), b, 0, st, a);
        return hipGetLastError();
    }
    const dim3 g(a.b.blocks + a.tblocks);
    if (a.b.w) {
        hipLaunchKernelGGL(k_bce_tower_partial<true>, g, b, 0, st, a);
        hipLaunchKernelGGL(k_bce_tower_final<true>, dim3(1), dim3(64), 0, st, a);
    } else {
        hipLaunchKernelGGL(k_bce_tower_partial<false>, g, b, 0, st, a);
        hipLaunchKernelGGL(k_bce_tower_final<false>, dim3(1), dim3(64), 0, st, a);
    }
    return hipGetLastError();
}

__global__ void k_adam(AdamArgs a) {
    // replayable steps: the step count lives on the device; lr_t comes from the host-built table
    // (spwgnn_adam_lr_table: the same expression spwgnn_adam evaluates, so both paths agree bitwise)
    if (a.step_dev) a.lr_t = a.lr_table[min(max(*a.step_dev, 0), a.table_len - 1)];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = a.p[i];
        const float g = a.gscale * a.g[i] + 2.f * a.l2 * p;
        const float m = a.b1 * a.m[i] + (1.f - a.b1) * g;
        const float v = a.b2 * a.v[i] + (1.f - a.b2) * g * g;
        a.m[i] = m;
        a.v[i] = v;
        a.p[i] = p - a.lr_t * m / (sqrtf(v) + a.eps);
    }
}

// ------------------------------------------------------------------------------------------------
// Keras 2.x Optimizer.get_gradients (clipnorm, then clipvalue) and a non-finite guard in front of
// k_adam's update (spwgnn_adam_clipped). Two launches: the partial sums of Σg'², then
// the update, whose every block re-adds the partials in the same order and so derives the same scale
// and the same skip decision. k_adam itself is untouched: a step without these options runs it as before.

// Block `blockIdx.x` of kClipBlocks: Σg'² over its share of the REAL parameters, g' = gscale·g + 2·l2·p
// as k_adam forms it. Round k < kClipRounds, thread (b, t) takes flat element b·256 + t + k·16,384: all
// kClipRounds loads of g and of p go out first (they depend on nothing), then at most 13 squares are
// added in a row, then bce_row_block's LDS tree (8 levels). No atomics: the same bits on every run and device.
// Which elements are real is decided per WAVE with scalar code: tensors start on 64-float boundaries,
// so the 64 consecutive elements a wave covers in a round lie in one tensor's extent, and they are real
// up to that tensor's end c.end[t] if it falls inside the chunk, else all of them. An element that is
// off (padding, or past n) reads element 0 instead and adds a selected 0.f: whatever the padding holds
// stays out. (A loop of its own per tensor made 22 dependent round trips to memory: 12 µs)
__global__ __launch_bounds__(256) void k_grad_sumsq(ClipArgs c) {
    __shared__ float ss[256];
    const AdamArgs& a = c.a;
    const int i0 = (int)blockIdx.x * 256 + (int)threadIdx.x;
    float gv[kClipRounds], pv[kClipRounds];
    bool on[kClipRounds];
#pragma unroll
    for (int k = 0; k < kClipRounds; ++k) {
        const int i = i0 + k * kClipBlocks * 256;
        const int cb = __builtin_amdgcn_readfirstlane(i);   // lane 0's element: the wave's 64-aligned chunk
        int limit = min(cb + 64, (int)a.n);
#pragma unroll
        for (int t = 0; t < kNumTensors; ++t) limit = (c.end[t] > cb && c.end[t] < limit) ? c.end[t] : limit;
        on[k] = i < limit;
        const int j = on[k] ? i : 0;
        gv[k] = a.g[j];
        pv[k] = a.p[j];
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kClipRounds; ++k) {
        const float gp = a.gscale * gv[k] + 2.f * a.l2 * pv[k];
        s += on[k] ? gp * gp : 0.f;
    }
    ss[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) ss[threadIdx.x] += ss[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) c.partial[blockIdx.x] = ss[0];
}

// k_adam's update on g' · scale, clamped to ±clipvalue. Reads the partials, g, the step word and the lr
// table; writes p, m, v (elementwise, each by its own thread) and — block 0, thread 0 — out4 / tot4:
// nothing a block reads is written by another block of this launch.
__global__ __launch_bounds__(256) void k_adam_clipped(ClipArgs c) {
    __shared__ float sh[2];   // scale, skip
    AdamArgs a = c.a;
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int b = 0; b < kClipBlocks; ++b) sum += (double)c.partial[b];
        const float sumsq = (float)sum;   // inf where the fp32 sum overflows: that counts as not finite
        const float norm = sqrtf(sumsq);
        const bool finite = fabsf(sumsq) <= 3.402823466e38f;   // false for NaN and ±inf
        const bool skip = c.skip_nonfinite && !finite;
        const bool clip = c.clipnorm > 0.f && norm >= c.clipnorm;   // false for a NaN norm, as in Keras
        const float scale = clip ? c.clipnorm / norm : 1.0f;
        sh[0] = scale;
        sh[1] = skip ? 1.f : 0.f;
        if (blockIdx.x == 0) {
            const float o[4] = {norm, scale, skip ? 1.f : 0.f, (clip && !skip) ? 1.f : 0.f};
            const double t4[4] = {skip ? 0.0 : (double)norm, (double)o[3], (double)o[2], 1.0};
            for (int k = 0; k < 4; ++k) {
                c.out4[k] = o[k];
                if (c.tot4) c.tot4[k] += t4[k];
            }
        }
    }
    __syncthreads();
    if (sh[1] != 0.f) return;   // skipped: p, m and v keep their bits
    const float scale = sh[0], cv = c.clipvalue;
    if (a.step_dev) a.lr_t = a.lr_table[min(max(*a.step_dev, 0), a.table_len - 1)];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = a.p[i];
        const float g0 = a.gscale * a.g[i] + 2.f * a.l2 * p;
        float g = g0 * scale;   // scale == 1.0f: exact, k_adam's g
        if (cv > 0.f) g = g > cv ? cv : (g < -cv ? -cv : g);   // selects: a NaN stays a NaN, as in Keras
        const float m = a.b1 * a.m[i] + (1.f - a.b1) * g;
        const float v = a.b2 * a.v[i] + (1.f - a.b2) * g * g;
        a.m[i] = m;
        a.v[i] = v;
        a.p[i] = p - a.lr_t * m / (sqrtf(v) + a.eps);
    }
}

// Start of a replayable training step (one thread, device_common.h step_advance_dev).
__global__ void k_step_advance(uint64_t* key, int32_t* step, int mode, uint64_t seed, int32_t rank) {
    if (threadIdx.x == 0) step_advance_dev(key, step, mode, seed, rank);
}

__global__ void k_sigmoid(const float* z, float* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = 1.f / (1.f + expf(-z[i]));
}

// per-tower readout (one thread per tower, node order): modes as SPWGNN_READOUT_*
__global__ void k_tower_readout(const float* __restrict__ z, const int32_t* __restrict__ off, int n_towers, int mode,
                                float* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_towers) return;
    const int b = off[t], e = off[t + 1];
    float s = 0.f;
    for (int n = b; n < e; ++n) s += (mode <= 1) ? 1.f / (1.f + expf(-z[n])) : z[n];
    out[t] = ((mode & 1) && e > b) ? s / (float)(e - b) : s;
}

hipError_t launch_bce(const BceArgs& a, hipStream_t st) {
    const dim3 g(a.blocks), b(256);
    if (a.blocks == 1) {   // one launch
        if (a.w) hipLaunchKernelGGL((k_bce_partial<true, true>), g, b, 0, st, a);
        else hipLaunchKernelGGL((k_bce_partial<false, true>), g, b, 0, st, a);
    } else if (a.w) {
        hipLaunchKernelGGL((k_bce_partial<true, false>), g, b, 0, st, a);
        hipLaunchKernelGGL(k_bce_final<true>, dim3(1), dim3(64), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_bce_partial<false, false>), g, b, 0, st, a);
        hipLaunchKernelGGL(k_bce_final<false>, dim3(1), dim3(64), 0, st, a);
    }
    return hipGetLastError();
}
hipError_t launch_bce_steps(const BceStepsArgs& a, hipStream_t st) {
    if (a.S < 1 || a.S > kMaxSteps || a.b.blocks < 1) return hipErrorInvalidValue;
    if (a.b.blocks == 1) {
        if (a.b.w) hipLaunchKernelGGL(k_bce_steps_one<true>, dim3(1), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_bce_steps_one<false>, dim3(1), dim3(256), 0, st, a);
        return hipGetLastError();
    }
    const dim3 g(a.b.blocks, a.S);
    if (a.b.w) {
        hipLaunchKernelGGL(k_bce_steps_partial<true>, g, dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_bce_steps_final<true>, dim3(1), dim3(64), 0, st, a);
    } else {
        hipLaunchKernelGGL(k_bce_steps_partial<false>, g, dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_bce_steps_final<false>, dim3(1), dim3(64), 0, st, a);
    }
    return hipGetLastError();
}
hipError_t launch_adam(const AdamArgs& a, hipStream_t st) {
    const int64_t blocks = std::min<int64_t>((a.n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_adam_clipped(const ClipArgs& c, hipStream_t st) {
    hipLaunchKernelGGL(k_grad_sumsq, dim3(kClipBlocks), dim3(256), 0, st, c);
    const int64_t blocks = std::min<int64_t>((c.a.n + 255) / 256, 2048);   // k_adam's grid
    hipLaunchKernelGGL(k_adam_clipped, dim3((unsigned)blocks), dim3(256), 0, st, c);
    return hipGetLastError();
}
hipError_t launch_step_advance(uint64_t* key, int32_t* step, int mode, uint64_t seed, int32_t rank, hipStream_t st) {
    hipLaunchKernelGGL(k_step_advance, dim3(1), dim3(64), 0, st, key, step, mode, seed, rank);
    return hipGetLastError();
}
hipError_t launch_tower_readout(const float* z, const int32_t* off, int n_towers, int mode, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_tower_readout, dim3((n_towers + 255) / 256), dim3(256), 0, st, z, off, n_towers, mode, out);
    return hipGetLastError();
}
// A replayed small-batch step's batch arrays, pinned (device-mapped) host staging → the static device
// buffer, as the step's first kernel: the loads cross PCIe once, all in flight together (a few µs),
// where a DMA copy between two replays left the GPU idle for ≈ 26 µs.
__global__ __launch_bounds__(256) void k_copy_in(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256)
        dst[i] = ld_sys_u4(src + i);   // host staging the host rewrites between replays: system-coherent reads
}
hipError_t launch_copy_in(const void* src, void* dst, int64_t n16, hipStream_t st) {
    const int wgs = (int)std::min<int64_t>(64, (n16 + 1023) / 1024);   // ≤ 4 pieces per thread
    hipLaunchKernelGGL(k_copy_in, dim3(std::max(wgs, 1)), dim3(256), 0, st, static_cast<const uint4*>(src),
                       static_cast<uint4*>(dst), n16);
    return hipGetLastError();
}

__global__ void k_accumulate_out3(const float* out3, const double* w, double* tot) {
    const int k = threadIdx.x;
    if (k < 3) tot[k] += (double)out3[k] * w[k];
}
hipError_t launch_accumulate_out3(const float* out3, const double* w, double* tot, hipStream_t st) {
    hipLaunchKernelGGL(k_accumulate_out3, dim3(1), dim3(64), 0, st, out3, w, tot);
    return hipGetLastError();
}
hipError_t launch_sigmoid(const float* z, float* p, int64_t n, hipStream_t st) {
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_sigmoid, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0, st, z, p, n);
    return hipGetLastError();
}

// ---- the propagation state at the library's edge ----
// A 32-node block of a chunk-major 104-feature array is 26 slots of [node i < 32][4 floats]: slot
// 2q + h holds features 52h + 4q .. +3 (cm_offk<kKhN>), so thread (block, slot, i) owns the 16-byte
// piece at float 4·(its index) of the chunk-major array — that side is one contiguous stream — and
// the 16-byte piece 13h + q of row-major row 32·block + i (400-byte rows: every piece is aligned).
// Piece 25 is the chunk-major padding (features 100..103), not part of a row. Pure copies, one owner
// per piece: the same bits on every run.
constexpr int kStateSlots = 2 * (kKhN / 4);   // 26
static_assert(kStateSlots * 32 * 4 == kCmBlkN && cm_offk<kKhN>(0, kKhN) == 128, "chunk-major node block");
__device__ __forceinline__ bool state_piece(int64_t idx, int n_nodes, int64_t& n, int& piece) {
    const int i = (int)(idx & 31), slot = (int)((idx >> 5) % kStateSlots);
    n = (idx >> 5) / kStateSlots * 32 + i;
    piece = (slot >> 1) + (slot & 1) * (kKhN / 4);
    return n < n_nodes;
}
// P_S → state_out: rows < n_nodes only, 25 pieces each
__global__ __launch_bounds__(256) void k_state_export(const float4* __restrict__ P_cm, float4* __restrict__ state,
                                                      int n_nodes, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int64_t n;
    int piece;
    if (state_piece(idx, n_nodes, n, piece) && piece < kFN / 4) state[n * (kFN / 4) + piece] = P_cm[idx];
}
// dstate → the dP_S slot: rows < n_nodes from the cotangent; the padding piece and the last block's
// rows past n_nodes are zero, as store_cm leaves them in every other dP (the array is RN rows long)
__global__ __launch_bounds__(256) void k_state_import(const float4* __restrict__ dstate, float4* __restrict__ dP_cm,
                                                      int n_nodes, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int64_t n;
    int piece;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (state_piece(idx, n_nodes, n, piece) && piece < kFN / 4) v = dstate[n * (kFN / 4) + piece];
    dP_cm[idx] = v;
}
hipError_t launch_state_export(const float* P_cm, float* state, int n_nodes, hipStream_t st) {
    const int64_t total = (int64_t)((n_nodes + 31) / 32) * kStateSlots * 32;
    hipLaunchKernelGGL(k_state_export, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(P_cm), reinterpret_cast<float4*>(state), n_nodes, total);
    return hipGetLastError();
}
hipError_t launch_state_import(const float* dstate, float* dP_cm, int n_nodes, hipStream_t st) {
    const int64_t total = (int64_t)((n_nodes + 31) / 32) * kStateSlots * 32;
    hipLaunchKernelGGL(k_state_import, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(dstate), reinterpret_cast<float4*>(dP_cm), n_nodes, total);
    return hipGetLastError();
}

}  // namespace spw
