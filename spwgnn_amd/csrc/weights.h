// The packed weights of a call, described once (host only): one row per fp32 pack, one row per split-bf16
// image. k_prep's descriptors (PackDesc, X6Desc), the workspace slots and the pack_rows / pack_cols lookups
// are all read off these two tables; what must agree between them is checked when this header compiles.
#pragma once
#include <array>
#include "kernels.h"

namespace spw {

// A pack is a zero-padded [rows][cols] copy of rows row0.. of a Keras tensor: src_rows × src_cols valid
// elements in the destination's orientation before `transpose` (dst[r][c] = src[c + row0][r]); perm: omp.1's
// columns in x' order (wo2_perm). k4: the k4-blocked image of the transposed-orientation MLP chains' A
// operands (gemm_blocks.h) — W2 / W2ᵀ (LDS images built by the edge kernels), rm.0 / om.0 and the biases
// stay row-major. bias_row ≥ 0: that destination row is the vector bias_tensor.
struct PackRow {
    int id, rows, cols, tensor, src_rows, src_cols, row0, transpose, perm, k4, bias_row = -1, bias_tensor = -1;
};
constexpr PackRow kPacks[PK_COUNT] = {
    // pack    rows cols  tensor  src_rows src_cols row0  T perm k4
    {PK_RM1,   160, 160, T_RM1K,  150, 150,   0, 0, 0, 1},   // forward [in][out]
    {PK_RM2,   160, 160, T_RM2K,  150, 150,   0, 0, 0, 1},
    {PK_RM3,   160, 160, T_RM3K,  150, 150,   0, 0, 0, 1},
    {PK_W1A,   160, 160, T_RMP0K, 150, 150,   0, 0, 0, 1},
    {PK_OM1,   128, 128, T_OM1K,  100, 100,   0, 0, 0, 1},
    {PK_W1B,   128, 160, T_RMP0K, 100, 150, 150, 0, 0, 1},   // [P feature][U feature]
    {PK_W1C,   128, 160, T_RMP0K, 100, 150, 250, 0, 0, 1},
    {PK_W2,    160, 160, T_RMP1K, 150, 150,   0, 0, 0, 0},
    {PK_W3A,   160, 128, T_RMP2K, 150, 100,   0, 0, 0, 1, 150, T_RMP2B},   // row 150: the degree column multiplies it
    {PK_WO1C,  128, 128, T_OMP0K, 100, 100,   0, 0, 0, 1},   // omp.0 rows 0-99 / 100-199 / 200-299
    {PK_WO1A,  128, 128, T_OMP0K, 100, 100, 100, 0, 0, 1},
    {PK_WO1P,  128, 128, T_OMP0K, 100, 100, 200, 0, 0, 1},
    {PK_WO2,   128, 128, T_OMP1K, 100, 101,   0, 0, 1, 1},
    {PK_W2T,   160, 160, T_RMP1K, 150, 150,   0, 1, 0, 0},   // the backward's transposes
    {PK_W1BT,  160, 128, T_RMP0K, 100, 150, 150, 1, 0, 1},
    {PK_W1CT,  160, 128, T_RMP0K, 100, 150, 250, 1, 0, 1},
    {PK_WO2T,  128, 128, T_OMP1K, 100, 101,   0, 1, 1, 1},
    {PK_WO1CT, 128, 128, T_OMP0K, 100, 100,   0, 1, 0, 1},
    {PK_WO1AT, 128, 128, T_OMP0K, 100, 100, 100, 1, 0, 1},
    {PK_WO1PT, 128, 128, T_OMP0K, 100, 100, 200, 1, 0, 1},
    {PK_W3T,   128, 160, T_RMP2K, 150, 100,   0, 1, 0, 1},
    {PK_W1AT,  160, 160, T_RMP0K, 150, 150,   0, 1, 0, 1},
    {PK_RM3T,  160, 160, T_RM3K,  150, 150,   0, 1, 0, 1},
    {PK_RM2T,  160, 160, T_RM2K,  150, 150,   0, 1, 0, 1},
    {PK_RM1T,  160, 160, T_RM1K,  150, 150,   0, 1, 0, 1},
    {PK_OM1T,  128, 128, T_OM1K,  100, 100,   0, 1, 0, 1},
    {PB_RM1,     1, 160, T_RM1B,    1, 150,   0, 0, 0, 0},   // biases
    {PB_RM2,     1, 160, T_RM2B,    1, 150,   0, 0, 0, 0},
    {PB_RM3,     1, 160, T_RM3B,    1, 150,   0, 0, 0, 0},
    {PB_W1A,     1, 160, T_RMP0B,   1, 150,   0, 0, 0, 0},
    {PB_W2,      1, 160, T_RMP1B,   1, 150,   0, 0, 0, 0},
    {PB_OM1,     1, 128, T_OM1B,    1, 100,   0, 0, 0, 0},
    {PB_O1,      1, 128, T_OMP0B,   1, 100,   0, 0, 0, 0},
    {PB_O2P,     1, 128, T_OMP1B,   1, 101,   0, 0, 1, 0},   // permuted like PK_WO2
    {PK_RM0,     2, 160, T_RM0K,    2, 150,   0, 0, 0, 0},   // the first encoder layers
    {PK_OM0,     2, 128, T_OM0K,    2, 100,   0, 0, 0, 0},
    {PB_RM0,     1, 160, T_RM0B,    1, 150,   0, 0, 0, 0},
    {PB_OM0,     1, 128, T_OM0B,    1, 100,   0, 0, 0, 0},
};
inline int pack_rows(int id) { return kPacks[id].rows; }
inline int pack_cols(int id) { return kPacks[id].cols; }

// An image (kernels.h: X6Id, X6Desc) holds nkb k-blocks × nt_out output tiles of its pack. half: the id of
// its half-tile form (the 4-tile images of the chain kernels, §3w; -1: none), which differs in ht alone.
// fwd: a forward kernel reads it, so h3 math builds it as f16 parts; no backward kernel reads one of these.
struct X6Row { int id, pack, nt_out, nkb, kh, half, fwd; };
constexpr X6Row kX6Rows[] = {
    // image      pack     nt_out nkb kh     half       fwd
    {X6_RM1,   PK_RM1,   5, 10, 0,    -1,         1},   // relation encoder (chains)
    {X6_RM2,   PK_RM2,   5, 10, 0,    -1,         1},
    {X6_RM3,   PK_RM3,   5, 10, 0,    -1,         1},
    {X6_W1A,   PK_W1A,   5, 10, 0,    -1,         1},
    {X6_W1AT,  PK_W1AT,  5, 10, kKhE, -1,         0},   // its backward
    {X6_RM3T,  PK_RM3T,  5, 10, 0,    -1,         0},
    {X6_RM2T,  PK_RM2T,  5, 10, 0,    -1,         0},
    {X6_RM1T,  PK_RM1T,  5, 10, 0,    -1,         0},
    {X6_W2,    PK_W2,    5, 10, kKhE, -1,         1},   // edge side (LDS B operands)
    {X6_W2T,   PK_W2T,   5, 10, kKhE, -1,         0},
    {X6_W3A,   PK_W3A,   4, 10, kKhE, X6_W3A_H,   1},   // node side
    {X6_WO1C,  PK_WO1C,  4, 7,  kKhN, X6_WO1C_H,  1},
    {X6_WO1A,  PK_WO1A,  4, 7,  0,    X6_WO1A_H,  1},
    {X6_WO1P,  PK_WO1P,  4, 7,  kKhN, X6_WO1P_H,  1},
    {X6_WO2,   PK_WO2,   4, 7,  0,    X6_WO2_H,   1},
    {X6_W1B,   PK_W1B,   5, 7,  0,    -1,         1},
    {X6_W1C,   PK_W1C,   5, 7,  0,    -1,         1},
    {X6_W1BT,  PK_W1BT,  4, 10, kKhE, X6_W1BT_H,  0},   // its backward
    {X6_W1CT,  PK_W1CT,  4, 10, kKhE, X6_W1CT_H,  0},
    {X6_WO2T,  PK_WO2T,  4, 7,  0,    X6_WO2T_H,  0},
    {X6_WO1PT, PK_WO1PT, 4, 7,  0,    X6_WO1PT_H, 0},
    {X6_WO1CT, PK_WO1CT, 4, 7,  0,    X6_WO1CT_H, 0},
    {X6_WO1AT, PK_WO1AT, 4, 7,  0,    X6_WO1AT_H, 0},
    {X6_W3T,   PK_W3T,   5, 7,  0,    -1,         0},
    {X6_OM1,   PK_OM1,   4, 7,  0,    X6_OM1_H,   1},   // object encoder
    {X6_OM1T,  PK_OM1T,  4, 7,  0,    X6_OM1T_H,  0},   // its backward
};
// every image by id: the rows above, and each half-tile form as its base row with ht = 1. A half-tile
// image is empty (no k-block) unless the build has the half-tile kernels (kHT, kernels.h)
struct X6Image { int pack, nt_out, nkb, kh, ht, fwd; };
constexpr std::array<X6Image, X6_COUNT> kX6Images = [] {
    std::array<X6Image, X6_COUNT> a{};
    for (const X6Row& r : kX6Rows) {
        a[r.id] = {r.pack, r.nt_out, r.nkb, r.kh, 0, r.fwd};
        if (r.half >= 0) a[r.half] = {r.pack, r.nt_out, kHT ? r.nkb : 0, r.kh, 1, r.fwd};
    }
    return a;
}();
inline int64_t x6_image_uint4(int id) { return x6_chain_uint4(kX6Images[id].nt_out, kX6Images[id].nkb); }

constexpr bool weight_tables_ok() {
    const auto dim_ok = [](int n) { return n == 1 || n == 2 || n % 32 == 0; };
    for (int i = 0; i < PK_COUNT; ++i) {
        const PackRow& p = kPacks[i];
        if (p.id != i || !dim_ok(p.rows) || !dim_ok(p.cols)) return false;
        if ((p.transpose ? p.src_cols : p.src_rows) > p.rows || (p.transpose ? p.src_rows : p.src_cols) > p.cols) return false;
        if (p.bias_row >= p.rows || (p.bias_row >= 0) != (p.bias_tensor >= 0)) return false;
    }
    int n = 0, halves = 0;
    for (const X6Row& r : kX6Rows) {
        if (r.id != n++ || (r.half >= 0 && r.half != X6_W3A_H + halves++)) return false;
        // an image reads pack elements (k < rows, col < cols) only
        if ((r.kh ? 2 * r.kh : 16 * r.nkb) > kPacks[r.pack].rows || 32 * r.nt_out > kPacks[r.pack].cols) return false;
    }
    return n == X6_W3A_H && n + halves == X6_COUNT;
}
static_assert(weight_tables_ok(), "kPacks / kX6Rows: enum order, padded dimensions, images inside their packs");

// k_prep's pack descriptors: destination slots `ps`, sources from the parameter table
inline void build_packs(const PackSlots& ps, PackDesc (&desc)[PK_COUNT]) {
    const ParamTable& pt = param_table();
    for (const PackRow& p : kPacks) {
        const TensorDesc& t = pt.t[p.tensor];
        // dst_off, src_off, rows, cols, src_rows, src_cols, src_ld, src_row0, transpose, perm, k4, bias_row, bias_off
        desc[p.id] = PackDesc{ps.off[p.id], t.offset, p.rows, p.cols, p.src_rows, p.src_cols, t.cols, p.row0,
                              p.transpose, p.perm, p.k4, p.bias_row, p.bias_row >= 0 ? pt.t[p.bias_tensor].offset : 0};
    }
}
// ... and its image descriptors (the split-bf16 maths): x6off = each image's uint4 offset
inline void build_x6(int math, const int64_t (&x6off)[X6_COUNT], PrepX6Args& xa) {
    for (int id = 0; id < X6_PREP_COUNT; ++id) {
        const X6Image& im = kX6Images[id];
        xa.d[id] = X6Desc{im.pack, im.nt_out, im.nkb, im.kh, im.ht, math_fwd_f16(math) && im.fwd, x6off[id]};
    }
}

}  // namespace spw
