// rnn_cell.h -- cell math shared by the recurrence kernels (rnn.hip, lstm_step.hip, gru.hip).
#pragma once

#include <math.h>

// No a*b+c is contracted behind the source's back: every kernel evaluates the cell exactly as written here.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// LSTM cell backward of one (row, unit): gates v = {i, f, g, o}, returns dZ in v, updates dc
__device__ __forceinline__ void cell_bwd(float v[4], float ct, float cprev, float dh, float& dc) {
    const float ig = v[0], fg = v[1], gg = v[2], og = v[3];
    const float tc = tanhf(ct);
    const float dct = dc + dh * og * (1.0f - tc * tc);
    v[0] = dct * gg * ig * (1.0f - ig);
    v[1] = dct * cprev * fg * (1.0f - fg);
    v[2] = dct * ig * (1.0f - gg * gg);
    v[3] = dh * tc * og * (1.0f - og);
    dc = dct * fg;
}

}  // namespace
