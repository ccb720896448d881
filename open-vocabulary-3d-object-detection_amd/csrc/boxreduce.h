// Workgroup reduction of a running box, shared by lift.hip and liftview.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kBoxThreads = 256;                // the workgroup of every kernel that reduces a box
constexpr int kBoxWaves = kBoxThreads / 64;

// Workgroup reduction of a running box (lo, hi, n) and the write of one (6) row + count; a count
// of 0 writes a row of zeros.  n sums to less than 2^31, so its trip through a double is exact.
// red: 7 * kBoxWaves doubles of LDS (224 B).
__device__ __forceinline__ void box_reduce_store(double lo[3], double hi[3], int n, double* red,
                                                 double* lohi_row, int32_t* count) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = fmax(hi[a], __shfl_xor(hi[a], off, 64));
        }
        n += __shfl_xor(n, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            red[wave * 7 + a] = lo[a];
            red[wave * 7 + 3 + a] = hi[a];
        }
        red[wave * 7 + 6] = (double)n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kBoxWaves; ++w) total += (int)red[w * 7 + 6];
        for (int a = 0; a < 3; ++a) {
            double l = red[a], h = red[3 + a];
            for (int w = 1; w < kBoxWaves; ++w) {
                l = fmin(l, red[w * 7 + a]);
                h = fmax(h, red[w * 7 + 3 + a]);
            }
            lohi_row[a] = total ? l : 0.0;
            lohi_row[3 + a] = total ? h : 0.0;
        }
        *count = total;
    }
}
