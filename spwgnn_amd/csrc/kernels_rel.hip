// d(loss)/d(relation gate): which support each stability logit hangs on.
// A scalar gate w_k on edge k = (src → dst) in the receiver sum of Networks.py:88 alone,
//   eff_{i,s} = tanh(Σ_{k: dst_k = i} w_k · e_{k,s}),   e_{k,s} = h2_{k,s}·W3 + b3,
// has at w ≡ 1 the gradient
//   r_{k,s} = ⟨g_s[dst], e_{k,s}⟩ = ⟨G3_s[dst], h2_{k,s}⟩ + ⟨g_s[dst], b3⟩,   r_k = Σ_s r_{k,s},
// g_s = d loss / d (pre-tanh receiver sum) and G3_s = g_s·W3ᵀ as the node backward stored them. The
// forward never forms a per-edge message (it sums h2 over receivers first), so h2 is rebuilt here:
//   h1 = relu(A + U_s[src] + V_s[dst]),   h2 = relu(h1·W2 + b2)
// — the edge forward's product per (32-edge block, step), followed by a dot with the gathered G3 row
// instead of the one-hot receiver sum.
// One wave owns a 32-edge block for all S steps. Transposed orientation: W2ᵀ tiles on the A lanes, the
// block's h1 rows on the B lanes, so lane (i, h) ends with features 32t + rho(r, h) of edge i in its
// accumulators; it multiplies them by the matching 16-byte pieces of G3_s[dst_i], adds its half of
// ⟨g_s[dst_i], b3⟩, and the two halves meet in one cross-lane move. Steps are added in registers in
// step order: no atomics, the same bits on every run. W2 is split once per workgroup from the flat
// parameters into LDS, in the edge forward's operand layout ([k-block·5 + tile][part][lane]): the
// packed W2 image of an h3 run holds f16 parts and the backward's product class is x6, so the bf16
// parts are formed here for every split math alike (the values k_prep splits, the same split).
// The kernel reads the workspace and writes only drel / drel_steps: a padding slot gets 0, an
// all-padding block reads no row, nothing is written outside [0, 32·n_eblocks).
#include <algorithm>
#include "kernels.h"

namespace spw {

constexpr int kRelWaves = 8;
constexpr int kRelQE = kKhE / 4;   // 19 pieces per half of a 152-feature row
constexpr int kRelQN = kKhN / 4;   // 13 pieces per half of a 104-feature row

// one 16-byte piece (4 features) of a chunk-major row stored as fp32, or as bf16 at the same element index
template <bool B16>
__device__ __forceinline__ float4 rel_piece(const float* base, int64_t elem) {
    if constexpr (B16) return unpack4_bf16(*reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(base) + elem));
    else return *reinterpret_cast<const float4*>(base + elem);
}

// The stored pieces of one k-block of h1 = relu(A + U_s[src] + V_s[dst]) for lane (i, h): chunks 2kb and
// 2kb + 1 of half h, kept as loaded (bf16 storage stays packed) until the k-block is multiplied
template <bool AB16, bool N16>
struct RelRaw {
    using AT = typename std::conditional<AB16, uint2, float4>::type;
    using UT = typename std::conditional<N16, uint2, float4>::type;
    AT a[2];
    UT u[2], v[2];
    template <class T>
    __device__ static __forceinline__ T ld(const float* base, int64_t elem) {
        if constexpr (sizeof(T) == 8) return *reinterpret_cast<const T*>(reinterpret_cast<const uint16_t*>(base) + elem);
        else return *reinterpret_cast<const T*>(base + elem);
    }
    // a padding slot reads nothing; chunk 19 does not exist: clamped, its W2 rows are zero
    __device__ __forceinline__ void load(const float* A, const float* U, const float* V, int64_t oA, int64_t oU, int64_t oV,
                                         int kb, bool ok, bool uvz) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int q = min(2 * kb + c, kRelQE - 1);
            a[c] = AT{};
            u[c] = v[c] = UT{};
            if (ok) {
                a[c] = ld<AT>(A, oA + 256 * q);
                if (!uvz) {
                    u[c] = ld<UT>(U, oU + 256 * q);
                    v[c] = ld<UT>(V, oV + 256 * q);
                }
            }
        }
    }
    __device__ __forceinline__ float4 h1(int c, bool ok, bool uvz) const {
        float4 x = unpack_uv(a[c]);
        if (!uvz) {
            const float4 uu = unpack_uv(u[c]), vv = unpack_uv(v[c]);
            x = make_float4(x.x + uu.x + vv.x, x.y + uu.y + vv.y, x.z + uu.z + vv.z, x.w + uu.w + vv.w);
        }
        return ok ? make_float4(relu(x.x), relu(x.y), relu(x.z), relu(x.w)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
};

// NP: the backward's product class — 3 (x6, h3), 2 (x3), 1 (bf16), 0 (f32: v_mfma_f32_32x32x2_f32)
// AB16: A stored as bf16 (Path::b16); N16: U, V and g stored as bf16 (Path::n16)
template <int NP, bool AB16, bool N16>
__global__ __launch_bounds__(64 * kRelWaves, 1) void k_rel_bwd(RelBwdArgs a) {
    constexpr bool F32 = NP == 0;
    // split maths: W2 as [kb·5 + T][part][lane] uint4 (lane (i, h): rows 76h + 8kb + e, column 32T + i);
    // f32: W2 as [k < 152][160] floats
    __shared__ uint4 wl[F32 ? (2 * kKhE * kLdE) / 4 : 50 * NP * 64];
    __shared__ float4 b2s[kLdE / 4];       // rmp.1 bias, features ≥ 150: 0
    __shared__ float4 b3s[2 * kRelQN];     // rmp.2 bias, features ≥ 100: 0
    const int tid = threadIdx.x;
    {
        const auto w2 = [&](int k, int col) { return (k < kFE && col < kFE) ? a.w2[k * kFE + col] : 0.f; };
        if constexpr (F32) {
            float* wf = reinterpret_cast<float*>(wl);
            for (int idx = tid; idx < 2 * kKhE * kLdE; idx += 64 * kRelWaves) wf[idx] = w2(idx / kLdE, idx % kLdE);
        } else {
            for (int idx = tid; idx < 50 * 64; idx += 64 * kRelWaves) {
                const int ln = idx & 63, u = idx >> 6, kb = u / 5, T = u - 5 * kb;
                const int col = 32 * T + (ln & 31), hh = ln >> 5;
                float w[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) w[e] = 8 * kb + e < kKhE ? w2(kKhE * hh + 8 * kb + e, col) : 0.f;
                uint32_t hw[4], mw[4], lw[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) split2(w[2 * m], w[2 * m + 1], hw[m], mw[m], lw[m]);
                uint4* o = wl + (int64_t)u * NP * 64 + ln;
                o[0] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
                if constexpr (NP >= 2) o[64] = make_uint4(mw[0], mw[1], mw[2], mw[3]);
                if constexpr (NP >= 3) o[128] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
            }
        }
        float* b2f = reinterpret_cast<float*>(b2s);
        float* b3f = reinterpret_cast<float*>(b3s);
        if (tid < kLdE) b2f[tid] = tid < kFE ? a.b2[tid] : 0.f;
        if (tid < 2 * kKhN) b3f[tid] = tid < kFN ? a.b3[tid] : 0.f;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, i = lane & 31, h = lane >> 5;
    const int64_t RE = (int64_t)a.n_eblocks * 32;

    for (int64_t blk = (int64_t)blockIdx.x * kRelWaves + wave; blk < a.n_eblocks; blk += (int64_t)gridDim.x * kRelWaves) {
        const int64_t e = blk * 32 + i;
        const int s = a.esrc[e], d = a.edst[e];
        const bool ok = s >= 0 && d >= 0 && s < a.n_nodes && d < a.n_nodes;
        if (__ballot(ok) == 0) {   // an all-padding block (capacity plans, receiver blocks of nodes without in-edges)
            if (h == 0) {
                a.drel[e] = 0.f;
                if (a.drel_steps)
                    for (int st = 0; st < a.S; ++st) a.drel_steps[st * RE + e] = 0.f;
            }
            continue;
        }
        const int sc = ok ? s : 0, dc = ok ? d : 0;
        // element offsets of piece (q = 0, half h) of the lane's rows; piece q lies 256 elements further
        const int64_t oA = blk * kCmBlk + (h * 32 + i) * 4;
        const int64_t oU = (int64_t)(sc >> 5) * kCmBlk + (h * 32 + (sc & 31)) * 4;
        const int64_t oV = (int64_t)(dc >> 5) * kCmBlk + (h * 32 + (dc & 31)) * 4;
        const int64_t oG = (int64_t)(dc >> 5) * kCmBlk;
        const int64_t og = (int64_t)(dc >> 5) * kCmBlkN + (h * 32 + (dc & 31)) * 4;
        float total = 0.f;
        for (int st = 0; st < a.S; ++st) {
            const bool uvz = a.uv_zero && st == 0;   // U_0 = V_0 = 0 and their rows may not exist (§3zh)
            const float* U = a.U + st * a.step_e;
            const float* V = a.V + st * a.step_e;
            // ⟨g_s[dst], b3⟩: half h of the 104-feature row (before the products: no accumulator is live yet)
            float r = 0.f;
            if (ok) {
                const float* gs = a.g + st * a.step_n;
#pragma unroll
                for (int q = 0; q < kRelQN; ++q) {
                    const float4 gv = rel_piece<N16>(gs, og + 256 * q);
                    const float4 b = b3s[kRelQN * h + q];
                    r = __builtin_fmaf(gv.x, b.x, r);
                    r = __builtin_fmaf(gv.y, b.y, r);
                    r = __builtin_fmaf(gv.z, b.z, r);
                    r = __builtin_fmaf(gv.w, b.w, r);
                }
            }
            f32x16 acc[5];
#pragma unroll
            for (int t = 0; t < 5; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {   // the bias first: regs 4q..4q+3 = features 32t + 8q + 4h ..
                    const float4 b = b2s[8 * t + 2 * q + h];
                    acc[t][4 * q] = b.x;
                    acc[t][4 * q + 1] = b.y;
                    acc[t][4 * q + 2] = b.z;
                    acc[t][4 * q + 3] = b.w;
                }
            if constexpr (F32) {
                const float* wf = reinterpret_cast<const float*>(wl);
                // h1 piece q of half hh of the lane's edge (0 on a padding slot, whose rows are not read)
                const auto h1_piece = [&](int q, int64_t half_off) {
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (ok) {
                        x = rel_piece<AB16>(a.A, oA + half_off + 256 * q);
                        if (!uvz) {
                            const float4 u = rel_piece<N16>(U, oU + half_off + 256 * q);
                            const float4 v = rel_piece<N16>(V, oV + half_off + 256 * q);
                            x = make_float4(x.x + u.x + v.x, x.y + u.y + v.y, x.z + u.z + v.z, x.w + u.w + v.w);
                        }
                        x = make_float4(relu(x.x), relu(x.y), relu(x.z), relu(x.w));
                    }
                    return x;
                };
#pragma unroll 1
                for (int hh = 0; hh < 2; ++hh)
#pragma unroll 1
                    for (int q = 0; q < kRelQE; ++q) {
                        // both lane halves read piece (q, hh): k-steps (f, f+1) and (f+2, f+3), f = 76hh + 4q;
                        // lane half h supplies row f + h of a k-step
                        const float4 x = h1_piece(q, (int64_t)(hh - h) * 128);
                        const int f = kKhE * hh + 4 * q;
                        const float x0 = h ? x.y : x.x, x1 = h ? x.w : x.z;
                        const float* w0 = wf + (f + h) * kLdE + i;
#pragma unroll
                        for (int t = 0; t < 5; ++t) {
                            acc[t] = mfma32(w0[32 * t], x0, acc[t]);
                            acc[t] = mfma32(w0[2 * kLdE + 32 * t], x1, acc[t]);
                        }
                    }
            } else {
                // one k-block (8 features per lane half) of stored pieces in flight beside the products of
                // the previous one; the loop stays rolled — unrolled, the ten k-blocks' loads are all
                // hoisted and the kernel spills
                RelRaw<AB16, N16> nxt;
                nxt.load(a.A, U, V, oA, oU, oV, 0, ok, uvz);
#pragma unroll 1
                for (int kb = 0; kb < 10; ++kb) {
                    const RelRaw<AB16, N16> cur = nxt;
                    if (kb + 1 < 10) nxt.load(a.A, U, V, oA, oU, oV, kb + 1, ok, uvz);
                    float4 x[2];
#pragma unroll
                    for (int c = 0; c < 2; ++c) x[c] = cur.h1(c, ok, uvz);
                    uint32_t hw[4], mw[4], lw[4];
                    split2(x[0].x, x[0].y, hw[0], mw[0], lw[0]);
                    split2(x[0].z, x[0].w, hw[1], mw[1], lw[1]);
                    split2(x[1].x, x[1].y, hw[2], mw[2], lw[2]);
                    split2(x[1].z, x[1].w, hw[3], mw[3], lw[3]);
                    bf16x8 bp[3];
                    bp[0] = as_bf16x8(make_uint4(hw[0], hw[1], hw[2], hw[3]));
                    bp[1] = as_bf16x8(make_uint4(mw[0], mw[1], mw[2], mw[3]));
                    bp[2] = as_bf16x8(make_uint4(lw[0], lw[1], lw[2], lw[3]));
#pragma unroll
                    for (int t = 0; t < 5; ++t) {
                        bf16x8 ap[3];
#pragma unroll
                        for (int p = 0; p < 3; ++p) ap[p] = as_bf16x8(wl[((kb * 5 + t) * NP + (p < NP ? p : 0)) * 64 + lane]);
                        acc[t] = mfma32_x6<NP>(ap, bp, acc[t]);
                    }
                }
            }
            // ⟨G3_s[dst], relu(h2pre)⟩ over the lane's features (150, 151 and tile 4's tail are padding)
            // (a tile's four pieces at a time: all 19 in flight beside the 80 accumulators spill)
            if (ok) {
                const float* G = a.G3 + st * a.step_e + oG;
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (32 * t + 8 * q + 4 < 2 * kKhE) {
                            float4 gv = *reinterpret_cast<const float4*>(G + cm_offk<kKhE>(dc & 31, 32 * t + 8 * q + 4 * h));
                            if (32 * t + 8 * q + 4 + 4 > kFE && h) gv.z = gv.w = 0.f;   // features 150, 151
                            r = __builtin_fmaf(relu(acc[t][4 * q]), gv.x, r);
                            r = __builtin_fmaf(relu(acc[t][4 * q + 1]), gv.y, r);
                            r = __builtin_fmaf(relu(acc[t][4 * q + 2]), gv.z, r);
                            r = __builtin_fmaf(relu(acc[t][4 * q + 3]), gv.w, r);
                        }
                    }
                }
            }
            r += __shfl_xor(r, 32, 64);
            if (!ok) r = 0.f;
            if (h == 0 && a.drel_steps) a.drel_steps[st * RE + e] = r;
            total += r;
        }
        if (h == 0) a.drel[e] = ok ? total : 0.f;
    }
}

hipError_t launch_rel_bwd(const RelBwdArgs& a, int math, bool b16, bool n16, hipStream_t st) {
    if (a.n_eblocks <= 0) return hipSuccess;
    const dim3 g(std::min((a.n_eblocks + kRelWaves - 1) / kRelWaves, 256)), b(64 * kRelWaves);
    if (math == MATH_F32) hipLaunchKernelGGL((k_rel_bwd<0, false, false>), g, b, 0, st, a);
    else if (math == MATH_BF16 && n16) hipLaunchKernelGGL((k_rel_bwd<1, true, true>), g, b, 0, st, a);
    else if (math == MATH_BF16 && b16) hipLaunchKernelGGL((k_rel_bwd<1, true, false>), g, b, 0, st, a);
    else if (math == MATH_BF16) hipLaunchKernelGGL((k_rel_bwd<1, false, false>), g, b, 0, st, a);
    else SPW_SPLIT32(math, NP, hipLaunchKernelGGL((k_rel_bwd<NP, false, false>), g, b, 0, st, a));
    return hipGetLastError();
}

// DropEdge: the relation gates of one training step's random edge subset. Thread e is edge
// slot e: gates[e] = base[e] · (keep ? scale : 0), keep drawn from the run's dropout key with kind 3 on (tower id,
// sender's local index, receiver's local index) — in ascending order under `symmetric`, so the two directions of
// a contact share one draw. The key names the edge by tower id and local indices alone: a tower's mask does not
// depend on where the plan put its edges. A padding slot (an index outside [0, n_nodes)) reads no node row and no
// base entry and gets +0. Reads esrc, edst, base at e < slots and node rows at checked indices; writes gates[e].
// Per-step masks (§3zzc): `steps` rows, row t at gates + t·gate_step drawn with feature t of the edge's row key
// (row 0 is the one-row mask) and multiplied by base[t·base_step + e]; slots [slots, gate_step) of a row stay unwritten.
__global__ __launch_bounds__(256) void k_dropedge(DropEdgeArgs a) {
    const uint64_t key = run_seed(a);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.slots; e += (int64_t)gridDim.x * 256) {
        const int s = a.esrc[e], d = a.edst[e];
        const bool active = s >= 0 && d >= 0 && s < a.n_nodes && d < a.n_nodes;
        uint32_t rk = 0u;
        if (active)
            rk = dropedge_row_key(key, (uint32_t)a.node_tower[s], (uint32_t)a.node_local[s], (uint32_t)a.node_local[d],
                                  a.symmetric != 0);
        for (int t = 0; t < a.steps; ++t) {
            float g = 0.f;
            if (active) {
                g = drop_keep(rk, (uint32_t)t, a.thresh) ? a.scale : 0.f;
                if (a.base) g = a.base[t * a.base_step + e] * g;
            }
            a.gates[t * a.gate_step + e] = g;
        }
    }
}

hipError_t launch_dropedge(const DropEdgeArgs& a, hipStream_t st) {
    if (a.slots <= 0) return hipSuccess;
    const dim3 g((unsigned)std::min<int64_t>((a.slots + 255) / 256, 1024)), b(256);
    hipLaunchKernelGGL(k_dropedge, g, b, 0, st, a);
    return hipGetLastError();
}

}  // namespace spw
