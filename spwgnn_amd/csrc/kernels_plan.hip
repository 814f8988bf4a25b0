// Batch plans filled on the device: the three data-dependent arrays of a capacity
// plan — edge_src, edge_dst, blk_csr — from device positions (the thresholded relation set of
// main.py:71-81) or from device relation matrices (the semantics of spwgnn_dense_to_edges), written
// where plan_fill_impl (host.cpp) puts them. The geometry (wtile, node_local, the first tower of each
// wave-tile) is static: spwgnn_plan_size_cap / spwgnn_plan_fill_cap with zero edges.
//
// One wave owns one wave-tile, whole towers of at most 32 nodes together (k_input_bwd's ownership).
//   1. towers: a node with node_local == 0 starts one. The tile's relation slots in the reference's
//      order — tower-major, sender-major, receiver j != m ascending — are node-major: node i sends
//      n_i − 1 slots, so a prefix sum over the nodes (soff) places every slot and a 5-step search in
//      it gives a slot's sender.
//   2. walk, 64 slots per pass: an active flag per lane, compacted with a ballot and a prefix
//      popcount. Kept edges go to LDS as (tile-local sender | receiver << 8) at their rank in the tile
//      (≤ 32·31 per tile); the rest of the buffer holds the padding key 0xFFFF.
//   3. emit, two 32-edge blocks per pass: edge_src / edge_dst from the keys (−1 = padding), and the
//      128-byte blk_csr row from the stable rank #{key_j < key_i} + #{j < i, key_j = key_i} of each
//      key among its block's 32 (LDS broadcast reads), staged in LDS and stored as 64 words.
// Integer work but for the distance test, no atomics but the status word. Nothing is written
// outside the tile's own 32·#blocks slots, #blocks rows and #nodes positions whatever the input holds:
// an edge beyond the tile's slots or its tower's capacity is dropped and the status word takes the
// positive error code (an ordinary atomic max).
#include "kernels.h"

namespace spw {

constexpr int kPlanSlots = 1024;   // key buffer per wave: >= 32·31 relation slots of a 32-node tile
constexpr int kPlanErrShape = 2, kPlanErrRelation = 3, kPlanErrCapacity = 5;   // −SPWGNN_E_*

__device__ __forceinline__ uint64_t bits_below(int n) {   // bits [0, n), n in [0, 64]
    return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

template <bool DENSE>
__global__ __launch_bounds__(256) void k_plan_device(PlanDevArgs a) {
    __shared__ uint16_t keys[4][kPlanSlots];
    __shared__ int32_t soff[4][33];     // slot offset of node i in the tile; [nn..32] = the tile's slot count
    __shared__ int32_t tst[4][32];      // first node of node i's tower (tile-local)
    __shared__ uint32_t rows[4][64];    // two blk_csr rows in flight
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int w = blockIdx.x * 4 + wave;
    if (w >= a.n_wtiles) return;   // no workgroup barrier below: waves run on their own
    const int b0 = __builtin_amdgcn_readfirstlane(a.wtile[4 * w]);
    const int nb = __builtin_amdgcn_readfirstlane(a.wtile[4 * w + 1]);
    const int n0 = __builtin_amdgcn_readfirstlane(a.wtile[4 * w + 2]);
    const int nn = __builtin_amdgcn_readfirstlane(a.wtile[4 * w + 3]);
    const int tw0 = __builtin_amdgcn_readfirstlane(a.wtile_tower[w]);
    // a geometry this kernel cannot serve writes nothing but the status
    if (b0 < 0 || nb < 0 || nb > a.n_eblocks - b0 || n0 < 0 || nn < 1 || nn > 32 || nn > a.n_nodes - n0 || tw0 < 0) {
        if (lane == 0) atomicMax(a.status, kPlanErrShape);
        return;
    }
    const uint64_t lt = bits_below(lane);
    const bool isnode = lane < nn;
    const int loc = isnode ? a.node_local[n0 + lane] : -1;
    const uint32_t sm = (uint32_t)__ballot(isnode && loc == 0);   // bit i: node i starts a tower
    if (!(sm & 1u)) {   // the tile must begin with a tower
        if (lane == 0) atomicMax(a.status, kPlanErrShape);
        return;
    }
    const int i5 = lane & 31;
    const uint32_t upto = sm & (i5 == 31 ? 0xFFFFFFFFu : ((2u << i5) - 1u));
    const uint32_t above = i5 == 31 ? 0u : (sm >> (i5 + 1));
    const int tstart = 31 - __clz((int)upto);                      // upto != 0: bit 0 is set
    const int tnext = above ? i5 + 1 + (__ffs((int)above) - 1) : nn;
    const int tsize = isnode ? tnext - tstart : 1;
    const bool isstart = isnode && ((sm >> i5) & 1u);
    const int nslots = isnode ? tsize - 1 : 0;
    int inc = nslots;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const int v = __shfl_up(inc, d, 64);
        if (lane >= d) inc += v;
    }
    const int total = __builtin_amdgcn_readfirstlane(__shfl(inc, 31, 64));   // <= 32·31
    if (lane < 32) {
        soff[wave][lane] = isnode ? inc - nslots : total;
        tst[wave][lane] = isnode ? tstart : 0;
    }
    if (lane == 32) soff[wave][32] = total;
    const int kept_max = min(nb * 32, kPlanSlots);
    for (int q = lane; q < kept_max; q += 64) keys[wave][q] = 0xFFFFu;

    // per tower, on its first node's lane: index, capacity, running count of active relations
    const int ti = tw0 + __popc(sm & (uint32_t)lt);
    int err = 0;
    int cap = 0, tc = 0;
    if (isstart) {
        if (ti >= a.n_towers) err = kPlanErrShape;
        else cap = a.tower_cap ? a.tower_cap[ti] : tsize * (tsize - 1);
    }

    float x = 0.f, y = 0.f;
    float thr2 = 0.f;
    bool fc = false;
    if constexpr (!DENSE) {
        if (isnode) {
            const float* r = a.raw + (int64_t)(n0 + lane) * a.raw_stride;
            x = r[0];
            y = r[1];
            const float z = a.raw_stride >= 3 ? r[2] : 0.f;
            if (a.pos)
                a.pos[n0 + lane] = make_float4(__fdiv_rn(x, a.divisor), __fdiv_rn(y, a.divisor),
                                               __fdiv_rn(z, a.divisor), 0.f);
        }
        fc = !(a.thr > 0.f);   // thr <= 0 or NaN: every relation (JengaBuilder.py:309-326)
        thr2 = __fmul_rn(a.thr, a.thr);
    }
    wave_lds_sync();

    int base = 0;   // edges kept so far in this tile
    for (int p0 = 0; p0 < total; p0 += 64) {
        const int g = p0 + lane;
        const bool valid = g < total;
        int s = 0, r = 0, ts = 0, tlo = 0;
        bool act = false;
        if (valid) {
            int sn = 0;   // the slot's sender-major node: the last i with soff[i] <= g
#pragma unroll
            for (int st = 16; st >= 1; st >>= 1)
                if (soff[wave][sn + st] <= g) sn += st;
            ts = tst[wave][sn];
            tlo = soff[wave][ts];
            const int jj = g - soff[wave][sn];
            s = sn;
            r = ts + jj + (jj >= sn - ts ? 1 : 0);
        }
        if constexpr (!DENSE) {
            const float xs = __shfl(x, s, 64), ys = __shfl(y, s, 64);
            const float xr = __shfl(x, r, 64), yr = __shfl(y, r, 64);
            const float dx = __fsub_rn(xs, xr), dy = __fsub_rn(ys, yr);
            const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));   // no contraction, no sqrt
            act = valid && (fc || d2 < thr2);
        } else {
            const int tsz = __shfl(tsize, ts, 64);
            if (valid) {
                const int node0 = n0 + ts;                       // the tower's first global node
                const int k = g - tlo;                           // slot inside the tower
                const int tb = node0 / a.N;
                // uniform towers only: this one must be rows [tb·N, tb·N + N) with E slots
                if (tsz != a.N || node0 % a.N != 0 || k >= a.E) {
                    err = max(err, kPlanErrShape);
                } else {
                    const float* rs = a.Rs + ((int64_t)tb * a.N) * a.E + k;
                    const float* rr = a.Rr + ((int64_t)tb * a.N) * a.E + k;
                    int si = -1, ri = -1, ns = 0, nr = 0;
                    bool bad = false;
                    for (int i = 0; i < a.N; ++i) {
                        const float av = rs[(int64_t)i * a.E], cv = rr[(int64_t)i * a.E];
                        if (av != 0.f) {
                            if (av != 1.f) bad = true;
                            si = i;
                            ++ns;
                        }
                        if (cv != 0.f) {
                            if (cv != 1.f) bad = true;
                            ri = i;
                            ++nr;
                        }
                    }
                    if (bad || ns > 1 || nr > 1 || (nr == 1 && ns == 0)) err = max(err, kPlanErrRelation);
                    else if (nr == 1) {
                        act = true;
                        s = ts + si;
                        r = ts + ri;
                    }
                }
            }
        }
        const uint64_t bal = __ballot(act);
        // rank inside the tower: its count before this pass + its active lanes below this one
        const int prev = __shfl(tc, ts, 64), capv = __shfl(cap, ts, 64);
        const uint64_t tbelow = lt & ~bits_below(max(tlo - p0, 0));
        const bool keep = act && prev + __popcll(bal & tbelow) < capv;
        if (isstart) {
            const int lo = min(max(soff[wave][lane] - p0, 0), 64);
            const int hi = min(max(soff[wave][lane + tsize] - p0, 0), 64);
            tc += __popcll(bal & bits_below(hi) & ~bits_below(lo));
        }
        const uint64_t kb = __ballot(keep);
        const int rank = base + __popcll(kb & lt);
        if (keep) {
            if (rank < kept_max) keys[wave][rank] = (uint16_t)(s | (r << 8));
            else err = max(err, kPlanErrCapacity);
        }
        base += __popcll(kb);
    }
    if (isstart) {
        if (tc > cap) err = max(err, kPlanErrCapacity);
        if (a.tower_edges && ti < a.n_towers) a.tower_edges[ti] = tc;
    }
    const int code = __ballot(err == kPlanErrCapacity) ? kPlanErrCapacity
                     : __ballot(err == kPlanErrRelation) ? kPlanErrRelation
                     : __ballot(err == kPlanErrShape) ? kPlanErrShape : 0;
    if (code && lane == 0) atomicMax(a.status, code);
    wave_lds_sync();

    const int h = lane >> 5;
    for (int bb = 0; bb < nb; bb += 2) {
        const int bi = bb + h;
        const bool bok = bi < nb;
        const int k0 = bi * 32;
        const bool inl = bok && k0 < kept_max;   // beyond the key buffer: padding (kept_max is a multiple of 32)
        const int me = inl ? keys[wave][k0 + i5] : 0xFFFF;
        const int sd = me & 0xFF, dd = me >> 8;   // 255 = padding
        if (bok) {
            const int64_t o = (int64_t)(b0 + bi) * 32 + i5;
            a.esrc[o] = sd == 255 ? -1 : n0 + sd;
            a.edst[o] = dd == 255 ? -1 : n0 + dd;
        }
        int rd = 0, rs = 0;
#pragma unroll 8
        for (int j = 0; j < 32; ++j) {
            const int kj = inl ? keys[wave][k0 + j] : 0xFFFF;
            const int sj = kj & 0xFF, dj = kj >> 8;
            rd += (dj < dd || (dj == dd && j < i5)) ? 1 : 0;
            rs += (sj < sd || (sj == sd && j < i5)) ? 1 : 0;
        }
        // csr[0:32] receiver order, [32:64] its keys, [64:96] sender order, [96:128] its keys
        uint8_t* row = reinterpret_cast<uint8_t*>(rows[wave]) + h * 128;
        row[rd] = (uint8_t)i5;
        row[32 + rd] = (uint8_t)dd;
        row[64 + rs] = (uint8_t)i5;
        row[96 + rs] = (uint8_t)sd;
        wave_lds_sync();
        if (bok) reinterpret_cast<uint32_t*>(a.csr + (int64_t)(b0 + bb) * 128)[lane] = rows[wave][lane];
        wave_lds_sync();
    }
}

hipError_t launch_plan_device(const PlanDevArgs& a, bool dense, hipStream_t st) {
    if (a.n_wtiles <= 0) return hipSuccess;
    const dim3 g((a.n_wtiles + 3) / 4), b(256);
    if (dense) hipLaunchKernelGGL((k_plan_device<true>), g, b, 0, st, a);
    else hipLaunchKernelGGL((k_plan_device<false>), g, b, 0, st, a);
    return hipGetLastError();
}

}  // namespace spw
