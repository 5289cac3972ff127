// dgram_scan_dev.h -- the workgroup scan helpers of the ragged copies, shared by unpack (datagram_dev.hip) and trim
// (wire_ragged_dev.hip): a row per thread and tile of 256 rows, per-tile sums, ONE workgroup that turns the tile sums into
// exclusive tile bases.  Everything has internal linkage: each translation unit that includes this gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kScanPer = 4;              // tile sums per thread and round of dgram_scan_tiles

// Exclusive scan of one value per thread over the workgroup (256 threads); *total = the sum.  Two barriers; sw is reusable after it.
__device__ inline unsigned long long block_scan_excl(unsigned long long v, unsigned long long *sw /* [kWaves] LDS */, unsigned long long *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();   // the previous use of sw is through
    if (lane == 63) sw[wave] = inc;
    __syncthreads();
    unsigned long long base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const unsigned long long t = sw[w];
        if (w < wave) base += t;
        all += t;
    }
    *total = all;
    return base + inc - v;
}

// One workgroup.  ts[t] becomes the sum of ts[0 .. t-1]; *total_out the sum of all.
__global__ __launch_bounds__(kThreads) void dgram_scan_tiles(unsigned long long *__restrict__ ts, int64_t T, int64_t *__restrict__ total_out)
{
    __shared__ unsigned long long sw[kWaves];
    unsigned long long carry = 0;
    for (int64_t base = 0; base < T; base += (int64_t)kThreads * kScanPer) {
        const int64_t i0 = base + (int64_t)threadIdx.x * kScanPer;
        unsigned long long v[kScanPer], sum = 0;
#pragma unroll
        for (int u = 0; u < kScanPer; u++) {
            v[u] = i0 + u < T ? ts[i0 + u] : 0ull;
            sum += v[u];
        }
        unsigned long long total;
        unsigned long long ex = carry + block_scan_excl(sum, sw, &total);
#pragma unroll
        for (int u = 0; u < kScanPer; u++) {
            if (i0 + u < T) ts[i0 + u] = ex;
            ex += v[u];
        }
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = (int64_t)carry;
}

}  // namespace
