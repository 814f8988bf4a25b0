// The layout of a call's workspace (host only): float offsets of every array, and the typed view of a
// caller's buffer under that layout.
#pragma once
#include <algorithm>
#include "weights.h"

namespace spw {

inline int64_t up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

static constexpr int kMaxChunks = 256;   // slabs per weight gradient (the ws kernels: one per CU)
static constexpr int kWgSlots = kMaxReduce; // weight gradients per backward, reduced by one batched launch

struct Ws {
    int64_t total = 0;  // bytes
    int S = 0, training = 0;
    int64_t RN = 0, RE = 0, NB = 0;
    // floats offsets (bytes / 4) — every array starts on 256 bytes; -1: not in this workspace (inference)
    int64_t pk = -1;
    int64_t cw = -1;                                 // node: c_o·Wo1c (x6/bf16 node forward)
    int64_t zo1 = -1, co = -1, P = -1, a = -1, o1 = -1, U = -1, V = -1, H2s = -1;   // node
    int64_t A = -1, z1 = -1, z2 = -1, z3 = -1, cr = -1;                             // edge
    int64_t ed = -1;                                 // per-edge (dx, dy) float2 (training)
    int64_t mask1 = -1, mask2 = -1, zmask = -1;      // u32
    int64_t dx = -1, do1 = -1, g = -1, G3 = -1, dU = -1, dV = -1, dP = -1, dco = -1, dzo2 = -1, dzo1 = -1;   // node (bwd)
    int64_t dA = -1, dz4 = -1, dz3 = -1, dz2 = -1, dz1 = -1;                        // edge (bwd)
    int64_t slab = -1;
    int64_t slab_floats = 0, slot_floats = 0;   // weight-gradient slabs: kWgSlots slots of slot_floats
    PackSlots ps;
    int64_t x6 = -1;                                 // split-bf16 weight images (uint4 units below)
    int64_t x6off[X6_COUNT];
    int sP() const { return training ? S + 1 : 2; }
    int sStep() const { return training ? S : 1; }
    // node arrays are chunk-major (104 / 152 floats per row): a step's rows are RN/32 blocks
    int64_t P_at(int s) const { return P + (int64_t)(training ? s : (s & 1)) * RN * kRowN; }
    int64_t U_at(int s) const { return U + (int64_t)(training ? s : 0) * RN * kRowE; }
    int64_t V_at(int s) const { return V + (int64_t)(training ? s : 0) * RN * kRowE; }
    int64_t H2s_at(int s) const { return H2s + (int64_t)(training ? s : 0) * RN * kRowE; }
    int64_t a_at(int s) const { return a + (int64_t)s * RN * kRowN; }
    int64_t o1_at(int s) const { return o1 + (int64_t)s * RN * kRowN; }
    int64_t m1_at(int s) const { return mask1 + (int64_t)s * NB * kLdE; }
    int64_t m2_at(int s) const { return mask2 + (int64_t)s * NB * kM2Blk; }
    int64_t dx_at(int s) const { return dx + (int64_t)s * RN * kRowN; }
    int64_t do1_at(int s) const { return do1 + (int64_t)s * RN * kRowN; }
    int64_t g_at(int s) const { return g + (int64_t)s * RN * kRowN; }
    int64_t G3_at(int s) const { return G3 + (int64_t)s * RN * kRowE; }
    int64_t dU_at(int s) const { return dU + (int64_t)s * RN * kRowE; }
    int64_t dV_at(int s) const { return dV + (int64_t)s * RN * kRowE; }
    int64_t dP_at(int k) const { return dP + (int64_t)(k & 1) * RN * kRowN; }
};

inline Ws make_ws(int64_t n_nodes, int64_t n_eblocks, int S, int training) {
    Ws w;
    w.S = S;
    w.training = training;
    w.RN = up(std::max<int64_t>(n_nodes, 1), 32);
    w.NB = n_eblocks;
    w.RE = n_eblocks * 32;
    int64_t cur = 0;  // floats
    auto take = [&](int64_t nfl) {
        int64_t o = cur;
        cur += up(nfl, 64);
        return o;
    };
    // packs
    int64_t poff = 0;
    for (int id = 0; id < PK_COUNT; ++id) {
        w.ps.off[id] = poff;
        poff += up((int64_t)pack_rows(id) * pack_cols(id), 64);
    }
    w.ps.total = poff;
    w.pk = take(poff);
    {   // x6 images (uint4 = 4 floats each)
        int64_t o = 0;
        for (int id = 0; id < X6_COUNT; ++id) {
            w.x6off[id] = o;
            o += x6_image_uint4(id);
        }
        w.x6 = take(o * 4);
    }
    const int64_t nN = w.RN * kRowN, nE = w.RN * kRowE, eE = w.RE * kLdE;
    w.co = take(nN);
    w.cw = take(nN);
    w.P = take(nN * w.sP());
    w.U = take(nE * w.sStep());
    w.V = take(nE * w.sStep());
    w.H2s = take(nE * w.sStep());
    const int64_t eCM = w.NB * kCmBlk;   // chunk-major edge rows
    w.A = take(eCM);
    if (training) {
        w.zo1 = take(nN);
        w.a = take(nN * S);
        w.o1 = take(nN * S);
        w.z1 = take(eCM);
        w.ed = take(w.RE * 2);
        w.z2 = take(eCM);
        w.z3 = take(eCM);
        w.cr = take(eCM);
        w.mask1 = take(w.NB * kLdE * S);
        w.zmask = take(w.NB * 4 * 3 * 64);
        w.mask2 = take(w.NB * kM2Blk * S);
        w.dx = take(nN * S);
        w.do1 = take(nN * S);
        w.g = take(nN * S);
        w.G3 = take(nE * S);
        w.dU = take(nE * S);
        w.dV = take(nE * S);
        w.dP = take(nN * 2);
        w.dco = take(nN);
        w.dzo2 = take(nN);
        w.dzo1 = take(nN);
        w.dA = take(eE);
        w.dz4 = take(eCM);
        w.dz3 = take(eCM);
        w.dz2 = take(eCM);
        w.dz1 = take(eCM);
        // a slot holds ≥ 256 160×160 slabs (one per CU for the ws kernels) and up to 1024 for the
        // row-chunked kernels of large batches (chunks of ≥ 512 rows)
        const int64_t rows = std::max(w.RE, w.RN) * S;
        const int64_t slot_chunks = std::min<int64_t>(1024, std::max<int64_t>(kMaxChunks, (rows + 511) / 512));
        w.slot_floats = slot_chunks * 160 * 160;
        w.slab_floats = (int64_t)kWgSlots * w.slot_floats;
        w.slab = take(w.slab_floats);
    }
    w.total = cur * 4;
    return w;
}

// A caller's buffer under layout w; x6() is null when the run's math has no images (f32)
struct Ctx {
    const Ws& w;
    char* base;
    bool images;
    float* f(int64_t off) const { return off < 0 ? nullptr : reinterpret_cast<float*>(base) + off; }
    uint32_t* u(int64_t off) const { return off < 0 ? nullptr : reinterpret_cast<uint32_t*>(base) + off; }
    const float* pk(int id) const { return reinterpret_cast<const float*>(base) + w.pk + w.ps.off[id]; }
    const uint4* x6(int id) const {
        return images ? reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(base) + w.x6) + w.x6off[id] : nullptr;
    }
};

}  // namespace spw
