// The loss arithmetic, once: Keras binary_crossentropy (Networks.py:102) of one logit row against one
// target row, as one workgroup's sums (bce_row_block) and the row's out3 from those sums
// (bce_row_store). Every loss path runs these two: the one-row and the per-step kernels
// (kernels_loss.hip) and the loss row folded into the gradient reductions (kernels_wgrad.hip). The
// fused backward's inline dL/dz (kernels_team.hip) is bce_dlogit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace spw {

struct BceArgs {
    const float *logits, *targets;
    int64_t n;
    float* dlogits;
    float* partial;   // [blocks][2], with w [blocks][3]; the per-step kernels' [S][blocks][3]
    float* out3;
    int blocks;
    const double* w3;   // non-null: tot3[k] += (double)out3[k] * w3[k] by the thread that writes out3
    double* tot3;
    // per-node loss weights (spwgnn_bce_weighted; null w: the unweighted kernels).
    // loss = Σ w_i·bce_i / norm, dlogits_i = w_i ≠ 0 ? w_i·bce_dlogit(z_i, t_i, 1/norm) : 0, out3 =
    // {loss, correct among w ≠ 0, #{w ≠ 0}}. norm = *norm_dev when set.
    const float* w;
    const float* norm_dev;
    float norm;
};
__device__ __forceinline__ float bce_norm(const BceArgs& a) { return a.norm_dev ? *a.norm_dev : a.norm; }
// clip(ŷ, 1e-7, 1-1e-7) ≡ clamp(z, ±ln((1-ε)/ε)).
constexpr float kLogitClip = 16.11809565f;
// dL/dz of one node
__device__ __forceinline__ float bce_dlogit(float z0, float t, float inv_n) {
    const float p = 1.f / (1.f + expf(-z0));
    return fabsf(z0) < kLogitClip ? (p - t) * inv_n : 0.f;
}
// the weighted form: a zero weight is a mask (a select — a NaN target or logit under it stays out)
__device__ __forceinline__ float bce_dlogit_w(float z0, float t, float w, float inv_norm) {
    return w != 0.f ? w * bce_dlogit(z0, t, inv_norm) : 0.f;
}

// One workgroup's (256 threads, `blk` of `blocks`) sums of one logit row over its share of the n nodes;
// thread 0 returns them in red: {Σ loss, correct, and with W the number of nodes with w_i ≠ 0}.
// W = false: the plain sums, `norm` = (float)n. W = true (Keras 2.x weighted_masked_objective with the
// caller's divisor `norm`): each term times w_i, the correct count over the nodes with w_i ≠ 0; a zero
// weight is a select, so whatever its logit and target hold stays out. With w ≡ 1 and norm = n every
// value is the unweighted one (1.0f·x and the selects are exact). The third sum, its register and its
// LDS array exist only with W: the unweighted block keeps two 256-float arrays.
// d_row (may be null) takes dL/dz times the step weight: λ ≠ 0 ? λ·d : +0 — a select, so a NaN logit
// under a zero step weight stays out, and 1.0f·d = d. No atomics: the same bits on every run.
template <bool W>
__device__ __forceinline__ void bce_row_block(const float* z_row, float* d_row, const float* targets, const float* w_row,
                                              int64_t n, int blocks, int blk, float lam, float norm, float (&red)[3]) {
    __shared__ float sl[256], sc[256];
    float* sn = nullptr;
    if constexpr (W) {
        __shared__ float sn_w[256];
        sn = sn_w;
    }
    float ls = 0.f, cs = 0.f;
    [[maybe_unused]] float ns = 0.f;
    const float inv_n = 1.0f / (float)norm;
    for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < n; i += (int64_t)blocks * 256) {
        const float z0 = z_row[i], t = targets[i];
        const float z = fminf(fmaxf(z0, -kLogitClip), kLogitClip);
        const float l = fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z)));
        const float p = 1.f / (1.f + expf(-z0));
        float d;
        if constexpr (W) {
            const float w = w_row[i];
            const bool on = w != 0.f;
            ls += on ? w * l : 0.f;
            cs += (on && (p > 0.5f ? 1.f : 0.f) == t) ? 1.f : 0.f;
            ns += on ? 1.f : 0.f;
            d = bce_dlogit_w(z0, t, w, inv_n);
        } else {
            ls += l;
            cs += ((p > 0.5f ? 1.f : 0.f) == t) ? 1.f : 0.f;
            d = bce_dlogit(z0, t, inv_n);
        }
        if (d_row) d_row[i] = lam != 0.f ? lam * d : 0.f;
    }
    sl[threadIdx.x] = ls;
    sc[threadIdx.x] = cs;
    if constexpr (W) sn[threadIdx.x] = ns;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sl[threadIdx.x] += sl[threadIdx.x + o];
            sc[threadIdx.x] += sc[threadIdx.x + o];
            if constexpr (W) sn[threadIdx.x] += sn[threadIdx.x + o];
        }
        __syncthreads();
    }
    red[0] = sl[0];
    red[1] = sc[0];
    if constexpr (W) red[2] = sn[0];
    __syncthreads();   // the next row of this block reuses the arrays
}

// One thread: o = a row's {loss, correct, count} from its sums, in double precision — the weighted
// divisor is the float `norm`, the plain one n itself, and the plain count is n — written to out3
// and, with tot3, added into the fp64 totals: tot3[k] += (double)o[k]·w3[k].
__device__ __forceinline__ void bce_put3(float* out3, double* tot3, const double* w3, const float (&o)[3]) {
    for (int k = 0; k < 3; ++k) {
        out3[k] = o[k];
        if (tot3) tot3[k] += (double)o[k] * w3[k];
    }
}
template <bool W>
__device__ __forceinline__ void bce_row_store(float* out3, double* tot3, const double* w3, double ls, double cs,
                                              double ns, float norm, int64_t n, float (&o)[3]) {
    const double div = W ? (double)norm : (double)n;
    o[0] = (float)(ls / div);
    o[1] = (float)cs;
    o[2] = W ? (float)ns : (float)n;
    bce_put3(out3, tot3, w3, o);
}

// One workgroup of the one-row loss on `a` (step weight 1): FINAL (a.blocks == 1, e.g. the reference's
// batch 32) it also writes out3 — one launch instead of two, and the row the gradient reductions carry
// under spwgnn_bce_backward; otherwise its sums go to a.partial, [blocks][W ? 3 : 2].
template <bool W, bool FINAL>
__device__ __forceinline__ void bce_one_row(const BceArgs& a, int blk) {
    const float norm = W ? bce_norm(a) : (float)a.n;
    float red[3], o[3];
    bce_row_block<W>(a.logits, a.dlogits, a.targets, a.w, a.n, a.blocks, blk, 1.0f, norm, red);
    if (threadIdx.x != 0) return;
    if constexpr (FINAL) {
        bce_row_store<W>(a.out3, a.tot3, a.w3, (double)red[0], (double)red[1], W ? (double)red[2] : 0.0, norm, a.n, o);
    } else {
        float* q = a.partial + (W ? 3 : 2) * blk;
        q[0] = red[0];
        q[1] = red[1];
        if constexpr (W) q[2] = red[2];
    }
}

}  // namespace spw
