// What the masked exact top-k searches share (filter.hip: one bitmap per call; prefix.hip: one row limit per query): the ordered keys of
// group maxima, the per-wave / per-block top-k merges of their tails and the merge of the exhaustive path's partial lists.
// Included inside the including file's anonymous namespace after search_tail.h; not a stand-alone header.
#pragma once

#define FILT_CAND_CAP_DEFAULT 1024      // candidate groups a query's block lists (4 KB of LDS); unit rows need about k of them
#define FILT_CAND_CAP_MAX 8192
#define FILT_PARTS_MAX 128              // per-query partial lists of the exhaustive path: parts * k <= 64 * 64 (one bit per slot and lane in the merge)
#define FILT_TAIL_NT 1024
#define FILT_REG_GROUPS 16              // group maxima a tail thread keeps in registers (16 x 1 024 groups = 1 M rows); beyond: re-read from L2

// floats ordered as unsigned integers (-inf lowest of the values pass A writes; 0 = "no such group")
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t key) {
    if (key <= 0x007fffffu) return -INFINITY;                  // -inf itself, or fewer than k groups
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// one wave: merge the scores of a group's (or a 64-entry stretch of the row list's) rows into the wave's running top-k, kept as entry
// `lane` of (cs, ci) for lanes < k.  Skipped when no new score reaches the k-th kept one (ties included: they may win on the row number).
__device__ __forceinline__ void wave_merge64(float& cs, int64_t& ci, float ns, int64_t ni, int k, int lane, float* w_s, int64_t* w_i) {
    const float kth = __shfl(cs, k - 1);
    if (!__any(ni >= 0 && ns >= kth)) return;                  // wave-uniform
    float s2[2] = {cs, ns};
    int64_t i2[2] = {ci, ni};
    wave_topk<2>(s2, i2, k, lane, w_s, w_i);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    cs = lane < k ? w_s[lane] : -INFINITY;
    ci = lane < k ? w_i[lane] : -1;
}
// the block's NW per-wave lists (entries of lanes < k in w_s / w_i) -> the final k, by wave 0, into fin_s / fin_i
template <int NW>
__device__ __forceinline__ void block_merge_lists(const float (*w_s)[KMAX], const int64_t (*w_i)[KMAX], int k, int lane, float* fin_s, int64_t* fin_i) {
    constexpr int R4 = (NW * KMAX + 63) / 64;
    float s[R4]; int64_t id[R4];
#pragma unroll
    for (int j = 0; j < R4; ++j) {
        const int i = j * 64 + lane;
        s[j] = i < NW * k ? w_s[i / k][i % k] : -INFINITY;
        id[j] = i < NW * k ? w_i[i / k][i % k] : -1;
    }
    wave_topk<R4>(s, id, k, lane, fin_s, fin_i);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// merge_kernel (search_tail.h) for the queries `only_if` flags: one wave per query over its P lists [parts][nq][k]
__global__ __launch_bounds__(256) void filter_merge_kernel(const float* __restrict__ ps, const int64_t* __restrict__ pi, int P, int nq, int k,
                                                            float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                            const int32_t* __restrict__ only_if, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq || (only_if && !only_if[q])) return;
    const int n = P * k;
    uint64_t taken = 0;
    for (int r = 0; r < k; ++r) {
        float bs = -INFINITY; int64_t bi = INT64_MAX; int bslot = -1;
        for (int c = lane, sl = 0; c < n; c += 64, ++sl) {
            if (taken >> sl & 1) continue;
            const int p = c / k, e = c % k;
            const int64_t o = ((int64_t)p * nq + q) * k + e;
            const float v = ps[o]; const int64_t vi = pi[o];
            if (vi < 0) continue;
            if (bslot < 0 || v > bs || (v == bs && vi < bi)) { bs = v; bi = vi; bslot = sl; }
        }
        float ws = bslot >= 0 ? bs : -INFINITY; int64_t wi = bslot >= 0 ? bi : INT64_MAX;
        wave_argbest(ws, wi);
        const bool found = wi != INT64_MAX;
        if (found && bslot >= 0 && bi == wi && bs == ws) taken |= (1ull << bslot);
        if (lane == 0) {
            out_s[(int64_t)q * k + r] = found ? ws : -INFINITY;
            out_i[(int64_t)q * k + r] = found ? wi : -1;
        }
    }
}
