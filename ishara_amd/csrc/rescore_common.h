// What nbest_rescore.hip and rescore_sweep.hip share: the limits, the by-value table of model pointers and the one rounded multiply-add
// of the score.
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
