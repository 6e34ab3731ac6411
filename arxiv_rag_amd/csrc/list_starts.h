// `start` of topics.members' layout as the kernels read it (cluster.hip, ivf.hip): every value clamped into [0, n_members] and the
// sequence made non-decreasing by a running maximum, so list c owns order[s[c], s[c + 1]) whatever the device data holds.  The host
// definition is topics.clamp_starts.  Integers only: a maximum gives the same values under any association and any compile flags.
#pragma once
#include <stdint.h>

__device__ __forceinline__ int clamp_start(long long v, int n_members) {
    return v < 0 ? 0 : (v > n_members ? n_members : (int)v);
}

// s_start[0 .. n_lists] = running maximum of the clamped start values (one block; blockDim.x a multiple of 64, at most 1024; s_wave
// holds one int per wave, 16 at the most).  Ends in a barrier: every thread may read s_start on return.
__device__ __forceinline__ void scan_starts(const int64_t* __restrict__ start, int n_lists, int n_members, int* s_start, int* s_wave) {
    const int tid = threadIdx.x, bt = blockDim.x, lane = tid & 63, wave = tid >> 6, n = n_lists + 1;
    const int seg = (n + bt - 1) / bt;
    const int a = tid * seg < n ? tid * seg : n, b = a + seg < n ? a + seg : n;
    int mine = 0;
    for (int i = a; i < b; ++i) {
        const int v = clamp_start(start[i], n_members);
        mine = v > mine ? v : mine;
        s_start[i] = mine;                                    // (the segment's own running maximum; what came before is folded in below)
    }
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc = up > inc ? up : inc;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = __shfl_up(inc, 1);                           // the maximum of the lanes below, then of the waves below
    if (lane == 0) before = 0;
    for (int w = 0; w < wave; ++w) before = s_wave[w] > before ? s_wave[w] : before;
    for (int i = a; i < b; ++i) s_start[i] = s_start[i] > before ? s_start[i] : before;
    __syncthreads();
}
