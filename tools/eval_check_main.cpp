// spwgnn_eval_metrics' argument checks (spw::eval_check, host.cpp) as a stand-alone CPU program, for a
// sanitizer run of the host code without a GPU and without loading anything into python:
//   clang++ -x c++ -std=c++20 -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Iinclude -Ispwgnn_amd/csrc \
//       -fsanitize=address,undefined -fno-sanitize-recover=all spwgnn_amd/csrc/host.cpp tools/eval_check_main.cpp \
//       -o tools/bin/eval_check && tools/bin/eval_check
#include <cmath>
#include <cstdio>
#include "../include/spwgnn.h"
#include "spwgnn_layout.h"

alignas(8) static int64_t tab[4 + 6 + 33 * 6 + 512];
static float z[8], t[8];
static int32_t off[3] = {0, 3, 8};

static int refused(const spwgnn_eval& ev, const float* logits = z, int64_t n = 8) {
    return spw::eval_check(logits, t, n, &ev) == SPWGNN_E_ARG ? 0 : 1;
}

int main() {
    const spwgnn_eval good{1, 2, 0.5f, 0, z, off, tab, tab + 4, tab + 10, tab + 208};
    int bad = spw::eval_check(z, t, 8, &good) != SPWGNN_OK;
    bad += refused(good, nullptr) + refused(good, z, 0) + (spw::eval_check(z, t, 8, nullptr) != SPWGNN_E_ARG);
    spwgnn_eval e = good;
    e.rows = 65, bad += refused(e), e = good;
    e.threshold = NAN, bad += refused(e), e.threshold = 1.f, bad += refused(e), e = good;
    e.reserved = 1, bad += refused(e), e = good;
    e.n_towers = -1, bad += refused(e), e.n_towers = 0, bad += refused(e), e = good;
    e.tower_offsets = nullptr, bad += refused(e), e = good;
    e.tower6 = e.by_size = nullptr, bad += refused(e), e = good;
    e.node4 = nullptr, bad += refused(e), e = good;
    e.hist = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(tab) + 4), bad += refused(e);
    std::printf("eval_check: %d unexpected status(es); struct_size(10) = %d\n", bad, spwgnn_struct_size(10));
    return bad != 0 || spwgnn_struct_size(10) != (int)sizeof(spwgnn_eval);
}
