// The row arg-max shared by the evaluation and the training statistics (evalstats.hip, trainstats.hip).
#pragma once

// torch's CPU max(dim=1): the first maximal index; in a row holding a NaN the first NaN
__device__ __forceinline__ int ev_argmax(const float *__restrict__ x, int C) {
    float best = x[0];
    int idx = 0;
    for (int c = 0; c < C; ++c) {
        const float v = x[c];
        if (!(v <= best)) {
            best = v;
            idx = c;
            if (v != v) break;
        }
    }
    return idx;
}
