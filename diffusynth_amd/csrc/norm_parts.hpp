// Parts shared by the normalisation kernels (groupnorm.hip, misc.hip's add_layernorm, clap_text.hip): the block tree sum and the LayerNorm row.
#pragma once
#include "common.hpp"

// Sum of v over the 256 threads of a block, in red[0] (every thread may read it after the call; a barrier before red is written again).
// THE ORDER OF THE ADDITIONS IS PART OF THE CONTRACT: level o = 128, 64, ... 1 adds red[tid + o] into red[tid], so the result's bits are a
// function of the 256 inputs alone — the kernels that use it promise bits that do not depend on the batch, the launch or the build.
// T: double (the norms) or int (a count).  The arrays are LDS and the loops say so (lds_ptr): through the generic pointer that a reference
// parameter is, the compiler folds the last level's addresses (two ds_read_b64 where the kernels had one ds_read2_b64).
template <typename T> using lds_ptr = __attribute__((address_space(3))) T*;
template <typename T>
__device__ __forceinline__ void block_tree_sum256(T (&red_)[256], T v) {
    const lds_ptr<T> red = (lds_ptr<T>)red_;
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
}
// ... of a pair (GroupNorm's sum and sum of squares): the same order for each, one barrier per level for both
template <typename T>
__device__ __forceinline__ void block_tree_sum256(T (&r1_)[256], T (&r2_)[256], T v1, T v2) {
    const lds_ptr<T> r1 = (lds_ptr<T>)r1_, r2 = (lds_ptr<T>)r2_;
    const int tid = threadIdx.x;
    r1[tid] = v1;
    r2[tid] = v2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            r1[tid] += r1[tid + o];
            r2[tid] += r2[tid + o];
        }
        __syncthreads();
    }
}

// One LayerNorm row of D values by a block of 256 threads: two passes (the mean, then the centred variance) in fp32 with double partial
// sums, then (v - mean) * rstd * gamma + beta.  value_at(i) gives the row's i-th value and is evaluated three times per element.
// red: 256 doubles that no thread still reads.
template <typename ValueAt>
__device__ __forceinline__ void layernorm_row(ValueAt value_at, int D, const float* gamma, const float* beta, float eps, float* out_row, double (&red)[256]) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < D; i += 256) s += (double)value_at(i);
    block_tree_sum256(red, s);
    const float mean = (float)(red[0] / D);
    __syncthreads();
    double q = 0.0;
    for (int i = tid; i < D; i += 256) {
        const float d = value_at(i) - mean;
        q += (double)d * d;
    }
    block_tree_sum256(red, q);
    const float rstd = 1.0f / sqrtf((float)(red[0] / D) + eps);
    for (int i = tid; i < D; i += 256) out_row[i] = (value_at(i) - mean) * rstd * gamma[i] + beta[i];
}
