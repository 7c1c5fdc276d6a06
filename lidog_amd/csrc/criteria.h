// What the criteria on logits [n, C] share (losses.hip, lovasz.hip): the fp32 row softmax and the dispatch on the class
// count, one instantiation per C.
#pragma once
#include "common.h"

#define DL_MAXC 20

template <int C>
__device__ __forceinline__ void softmax_row(const float *__restrict__ x, float (&p)[C]) {
    float m = x[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        p[c] = expf(x[c] - m);
        s += p[c];
    }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
}

// 7 classes in every configuration of the reference (configs/*: out_channels 7); the other counts (binary heads, 16-class
// nuScenes, 19 / 20-class SemanticKITTI label sets) cost one instantiation each
#define DICE_DISPATCH(CALL)                                                     \
    switch (C) {                                                                \
        case 2: CALL(2); break;                                                 \
        case 3: CALL(3); break;                                                 \
        case 4: CALL(4); break;                                                 \
        case 5: CALL(5); break;                                                 \
        case 6: CALL(6); break;                                                 \
        case 7: CALL(7); break;                                                 \
        case 8: CALL(8); break;                                                 \
        case 9: CALL(9); break;                                                 \
        case 10: CALL(10); break;                                               \
        case 11: CALL(11); break;                                               \
        case 12: CALL(12); break;                                               \
        case 13: CALL(13); break;                                               \
        case 14: CALL(14); break;                                               \
        case 15: CALL(15); break;                                               \
        case 16: CALL(16); break;                                               \
        case 17: CALL(17); break;                                               \
        case 18: CALL(18); break;                                               \
        case 19: CALL(19); break;                                               \
        case 20: CALL(20); break;                                               \
        default: LIDOG_REQUIRE(false, "dice: C must be in [2, 20]");            \
    }
