// Workgroup prefix sum shared by the mask scans of select_rows.hip and densify_round.hip (gfx950 only).
#pragma once
#include "mom_common.h"

__device__ __forceinline__ int block_exclusive_scan_256(int v, int* s_wave, int& total)
{
    // exclusive prefix of one int per thread over 256 threads; total = sum over the workgroup
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; w++) base += s_wave[w];
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return base + incl - v;
}
