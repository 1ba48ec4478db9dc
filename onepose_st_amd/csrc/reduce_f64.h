// The float64 reductions of the kernels that are pinned bit for bit to a float64 oracle, written once: the association order of a sum
// is part of that contract, so every such kernel takes its wave sum and its block tree from here.  A namespace of its own: tile.h's
// wave_sum(float) is an unrelated overload.  No products here, so contraction has nothing to fuse.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace red64 {

// the sum over the 64 lanes of a wave, to every lane: the xor butterfly, off = 32, 16, ... 1
__device__ __forceinline__ double wave_sum(double x) {
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);   // commutative pairs: every lane ends with the same sum
    return x;
}

// the value every lane holds, as a scalar: makes the branches on it provably wave-uniform
__device__ __forceinline__ double uniform(double x) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the sums of v[0 .. n) over a workgroup of Threads threads, to every thread: the fixed tree red[t] + red[t + s], s = Threads / 2 ... 1.
// red: n * Threads doubles of LDS, sum k in red[k * Threads ..).  A barrier before the writes (red may still be read from the call
// before), one after each level, and one after the result is read (red may be written right after the return)
template <int Threads>
__device__ __forceinline__ void block_sums(double* v, int n, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int k = 0; k < n; ++k) red[k * Threads + tid] = v[k];
    __syncthreads();
    for (int s = Threads / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < n; ++k) red[k * Threads + tid] = red[k * Threads + tid] + red[k * Threads + tid + s];
        __syncthreads();
    }
    for (int k = 0; k < n; ++k) v[k] = red[k * Threads];
    __syncthreads();
}

}  // namespace red64
