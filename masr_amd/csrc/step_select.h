// The selection order and the step limit that the beam merges of the attention decoders share (decoder_step.hip: decoder: attention;
// decoder_joint.hip: decoder: joint).  Device code only; workgroups of 256 threads.
#pragma once
#include "common.h"

namespace masr {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The order of every selection here: the larger value first, of bit-equal values (-inf included) the smaller index first.
__device__ __forceinline__ bool before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// the block's first (value, index) in that order; 256 threads, red_* in LDS [4]; every thread returns the winner
__device__ __forceinline__ void block_first(float& v, int& i, float* red_v, int* red_i) {
    for (int off = 32; off > 0; off >>= 1) {
        const float w = __shfl_xor(v, off, 64);
        const int j = __shfl_xor(i, off, 64);
        if (j >= 0 && (i < 0 || before(w, j, v, i))) {
            v = w;
            i = j;
        }
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red_v[wave] = v;
        red_i[wave] = i;
    }
    __syncthreads();
    v = red_v[0];
    i = red_i[0];
    for (int w = 1; w < 4; ++w)
        if (red_i[w] >= 0 && (i < 0 || before(red_v[w], red_i[w], v, i))) {
            v = red_v[w];
            i = red_i[w];
        }
}

// steps the search of utterance b may run: min(valid encoder frames, max_len when positive, max_pos - 1, Lcap)
__device__ __forceinline__ int step_limit(int enc_len, int Tp, int max_len, int max_pos, int Lcap) {
    int lim = min(clampi(enc_len, 0, Tp), min(max_pos - 1, Lcap));
    if (max_len > 0) lim = min(lim, max_len);
    return lim;
}

}  // namespace masr
