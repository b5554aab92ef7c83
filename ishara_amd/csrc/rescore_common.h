// What nbest_rescore.hip and rescore_sweep.hip share: the limits, the by-value table of model pointers, the one rounded multiply-add of
// the score and the overlap test of the launchers.
#pragma once
#include "kernels.h"

static constexpr int NR_MAXN = 64;
static constexpr int NR_MAX_M = 8;

struct NrPtrs { const float* p[NR_MAX_M]; };

DEVI float nr_madd(float s, float w, float v) {
#pragma clang fp contract(off)
    const float p = w * v;
    return s + p;
}

static inline bool nr_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}
