// Exact "R largest 64-bit keys" lists in LDS, written once for the candidate scans (binary.hip: Hamming distances over sign bits;
// pq.hip: byte-table sums over product-quantiser codes).  A key is  high word << 32 | (0xffffffff - row):  larger is better, distinct
// for distinct rows, never 0 (0 = an empty slot; rows are below 2^31).  What the high word means is the caller's business.
//   KeyLists   NL lists of KEY_CAP keys, each with an integer slot counter and a threshold (0 until the list has been cut once;
//              afterwards its R-th largest key).
//   key_append a lane appends a key above the list's threshold through the slot counter (an integer LDS atomic).
//   key_cut    before a round of at most KEY_NT appends per list that could overflow a list, the lists that could are cut back to their
//              R largest by a block-wide bitonic sort (bm25.hip's, over all those lists in the same stages).  A key at or below the R-th
//              largest of keys already seen is not among the R largest of all, so a list cut at the end holds the exact R largest keys
//              of everything offered to it, sorted, whatever the order of the appends.
//   key_merge_kernel  one block per query over its parts * R keys of partial lists, any number of them, through the same list and cut
//              -> out_cand (the rows), out_hi (the high word, or 0x7fffffff - it) and out_count.
// Integer work only, no global atomics.  Every kernel that uses these runs KEY_NT threads.
#pragma once
#include "arx_common.h"

namespace {
constexpr int KEY_NT = 256;
constexpr int KEY_CAP = 1024;                   // keys of a list (8 KiB of LDS)
constexpr int KEY_R_MAX = 256;

template <int NL>
struct KeyLists {
    unsigned long long keys[NL][KEY_CAP];
    unsigned long long thr[NL];
    int cnt[NL];
};

// Cut the lists of `mask` (list l holds min(cnt[l], KEY_CAP) keys in any order) back to their n largest, sorted descending; updates cnt
// and thr.  The whole block; mask block-uniform; earlier writes to the lists are behind a barrier already; ends with a barrier.
template <int NL>
__device__ __forceinline__ void key_cut(KeyLists<NL>& sm, unsigned mask, int n) {
    const int tid = threadIdx.x;
    for (int t = tid; t < NL * KEY_CAP; t += KEY_NT) {
        const int l = t / KEY_CAP, i = t % KEY_CAP;
        if (((mask >> l) & 1u) && i >= sm.cnt[l]) sm.keys[l][i] = 0ull;
    }
    __syncthreads();
    for (int k = 2; k <= KEY_CAP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < NL * (KEY_CAP / 2); t += KEY_NT) {
                const int l = t / (KEY_CAP / 2), u = t % (KEY_CAP / 2);
                if (!((mask >> l) & 1u)) continue;
                const int i = ((u & ~(j - 1)) << 1) | (u & (j - 1)), p = i | j;           // p < KEY_CAP
                const unsigned long long a = sm.keys[l][i], b = sm.keys[l][p];
                if (((i & k) == 0) ? a < b : a > b) { sm.keys[l][i] = b; sm.keys[l][p] = a; }
            }
            __syncthreads();
        }
    if (tid < NL && ((mask >> tid) & 1u)) {
        const int c = sm.cnt[tid] < KEY_CAP ? sm.cnt[tid] : KEY_CAP;
        sm.cnt[tid] = c < n ? c : n;
        sm.thr[tid] = c >= n ? sm.keys[tid][n - 1] : 0ull;
    }
    __syncthreads();
}

// the lists (of the first nl) that the next round of at most KEY_NT appends each could overflow; block-uniform once cnt is stable
template <int NL>
__device__ __forceinline__ unsigned key_full_mask(const KeyLists<NL>& sm, int nl) {
    unsigned m = 0;
#pragma unroll
    for (int l = 0; l < NL; ++l) m |= (l < nl && sm.cnt[l] + KEY_NT > KEY_CAP) ? (1u << l) : 0u;
    return m;
}

template <int NL>
__device__ __forceinline__ void key_append(KeyLists<NL>& sm, int l, unsigned long long key) {
    if (key > sm.thr[l]) {
        const int pos = atomicAdd(&sm.cnt[l], 1);              // integer slot counter; pos < KEY_CAP: the lists are cut before a round that could overflow
        if (pos < KEY_CAP) sm.keys[l][pos] = key;
    }
}

// one block per query: the parts * R keys of its partial lists -> its R largest, as (row, high word), and their number.
// HI_DIRECT: out_hi is the key's high word itself (pq: the sum); otherwise 0x7fffffff - it (binary: the distance).
template <bool HI_DIRECT>
__global__ __launch_bounds__(KEY_NT) void key_merge_kernel(const unsigned long long* __restrict__ part_k, int64_t parts, int nq, int R,
                                                           int32_t* __restrict__ out_cand, int32_t* __restrict__ out_hi,
                                                           int64_t* __restrict__ out_count) {
    __shared__ KeyLists<1> sm;
    const int tid = threadIdx.x, q = blockIdx.x;
    if (tid == 0) { sm.cnt[0] = 0; sm.thr[0] = 0ull; }
    __syncthreads();
    const int64_t total = parts * R;
    for (int64_t e0 = 0; e0 < total; e0 += KEY_NT) {          // block-uniform
        const unsigned full = key_full_mask(sm, 1);
        __syncthreads();
        if (full) key_cut(sm, 1u, R);
        const int64_t e = e0 + tid;
        if (e < total) {
            const int64_t p = e / R;
            key_append(sm, 0, part_k[(p * nq + q) * R + (e - p * R)]);                   // (thr >= 0: an empty slot is never appended)
        }
        __syncthreads();
    }
    key_cut(sm, 1u, R);
    for (int r = tid; r < R; r += KEY_NT) {
        const unsigned long long key = r < sm.cnt[0] ? sm.keys[0][r] : 0ull;
        out_cand[(int64_t)q * R + r] = key ? (int32_t)(0xffffffffu - (uint32_t)key) : -1;
        if (out_hi) {
            const uint32_t hi = (uint32_t)(key >> 32);
            out_hi[(int64_t)q * R + r] = key ? (int32_t)(HI_DIRECT ? hi : 0x7fffffffu - hi) : -1;
        }
    }
    if (tid == 0) out_count[q] = sm.cnt[0];
}

// the workspace of a candidate scan: (part, query) lists of R keys, at most KEY_SLOTS_MAX of them (64 MiB at R = 256)
constexpr int KEY_QBATCH = 256;                 // queries per slice of a call
constexpr int64_t KEY_SLOTS_MAX = 1ll << 15;
struct KeyWs { int64_t slots, total; int qb; };
inline KeyWs key_layout(int64_t n_rows, int n_queries, int R) {
    KeyWs w;
    w.qb = n_queries < KEY_QBATCH ? n_queries : KEY_QBATCH;
    const int64_t parts = (n_rows + 63) / 64 > 0 ? (n_rows + 63) / 64 : 1;             // at the smallest rows_per_block
    w.slots = parts * w.qb < KEY_SLOTS_MAX ? parts * w.qb : KEY_SLOTS_MAX;
    if (w.slots < w.qb) w.slots = w.qb;
    w.total = round_up64(w.slots * R * 8, 256);
    return w;
}
}      // namespace
