// What the row-bitmap mask policies share (filter.hip, range.hip, grouped.hip: one bitmap per call; filter_multi.hip: a set of them): which
// bits of a word name rows of the shard, pass A's policy for one bitmap per call, the mask of a call that may come without a bitmap
// (an all-ones one in its workspace), and the exclusive scan of the words' popcounts that turns a bitmap into positions of a row list.
// Included inside the including file's anonymous namespace after masked_topk.h; not a stand-alone header.
#pragma once

__device__ __forceinline__ uint64_t valid_bits(int64_t n_rows, int64_t g) {      // the bits of word g that name rows of the shard
    const int64_t rem = n_rows - g * GROUP_ROWS;
    return rem >= GROUP_ROWS ? ~0ull : ((1ull << rem) - 1ull);
}

// ---- pass A with one bitmap for every query of the call: the pass-A part of a mask policy (masked_topk.h).  range.hip and grouped.hip,
// whose tails are their own, hand it to the kernels as it stands (AllowRows below); filter.hip's BitmapMask adds the tail's and the
// exhaustive path's parts ---------------------------------------------------------------------------------------------------------------------
struct BitmapRows {
    const uint64_t* allow;      // bit r & 63 of word r >> 6 = row r is visible
    struct LaneRows {           // the bits of the lane's 16 rows, taken once: they do not depend on the query
        bool on[GROUP_ROWS / 16][4];
        __device__ __forceinline__ const LaneRows& of_query(int, int) const { return *this; }
        __device__ __forceinline__ bool operator()(int j, int r) const { return on[j][r]; }
    };
    struct Tile {
        bool empty; uint64_t mine;
        __device__ __forceinline__ LaneRows lane_rows(int64_t, int lane) const {
            const uint32_t lrow = (uint32_t)(lane >> 4) * 4u;
            LaneRows s;
#pragma unroll
            for (int j = 0; j < GROUP_ROWS / 16; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) s.on[j][r] = (mine >> ((uint32_t)(j * 16 + r) + lrow)) & 1ull;
            return s;
        }
    };
    template <int BM>
    __device__ __forceinline__ Tile tile(int64_t n0, int wn, int, int, int64_t n_rows) const {
        const int64_t n_groups = (n_rows + GROUP_ROWS - 1) / GROUP_ROWS;
        uint64_t any = 0, mine = 0;                            // the tile's four words (block-uniform) and this wave's own
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t gj = (n0 >> 6) + j;
            const uint64_t w = gj < n_groups ? (allow[gj] & valid_bits(n_rows, gj)) : 0ull;
            any |= w;
            mine = j == wn ? w : mine;
        }
        return {any == 0ull, mine};
    }
};

// every row visible: the bitmap a call without one makes in its workspace
__global__ __launch_bounds__(256) void bitmap_ones_kernel(uint64_t* __restrict__ words, int64_t n_words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) words[i] = ~0ull;
}

// ---- the mask of range.hip and grouped.hip: BitmapRows for pass A and, for the scan driver (masked_topk.h), the host part of a mask
// policy.  allow == NULL means every row: the call makes an all-ones bitmap in its workspace, ahead of its first slice ------------------------
struct AllowRows : BitmapRows {
    int64_t n_allowed;          // the caller's count of the set bits, -1 = unknown: checked, not used
    uint64_t* ones;             // workspace: the all-ones bitmap `allow` points at when the caller gave none, else null (set by bind)

    bool given() const { return true; }
    int check(int64_t n_rows) const { ARX_REQUIRE(n_allowed >= -1 && n_allowed <= n_rows, "n_allowed=%lld", (long long)n_allowed); return ARX_OK; }
    static void own_bytes(const MaskedWs& L, int64_t, int64_t b[2]) { b[0] = L.n_groups * 8; b[1] = 0; }
    void bind(char* ws, const MaskedWs& L) { ones = allow ? nullptr : (uint64_t*)(ws + L.own[0]); allow = allow ? allow : ones; }
    int prepare_batch(int q0, int, int64_t n_rows, hipStream_t st) const {
        const int64_t n_words = (n_rows + GROUP_ROWS - 1) / GROUP_ROWS;
        if (ones && q0 == 0) {
            bitmap_ones_kernel<<<cdiv(n_words, 256), 256, 0, st>>>(ones, n_words);
            ARX_HIP_CHECK(hipGetLastError());
        }
        return ARX_OK;
    }
    int prepare_lists(int, int, int64_t, int64_t, const int*, hipStream_t) const { return ARX_OK; }
};
inline const BitmapRows& pass_a_mask(const AllowRows& mask) { return mask; }      // the kernels take the bitmap alone

// ---- the row list of the exhaustive path --------------------------------------------------------------------------------------------------
// offsets of the words' rows in the compacted list (exclusive scan of the popcounts; off[n_words] = the number of allowed rows).  One
// block per bitmap (block b: words allow[b * n_words ...], offsets off[b * (n_words + 1) ...]); thread t owns a contiguous run of words.
// `gate`: run only if *gate != 0 (the masked scan's "some query overflowed").
__global__ __launch_bounds__(1024) void filter_scan_kernel(const uint64_t* __restrict__ allow, int64_t n_words, int64_t n_rows,
                                                            int64_t* __restrict__ off, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    __shared__ int64_t wave_tot[16];
    allow += (int64_t)blockIdx.x * n_words;
    off += (int64_t)blockIdx.x * (n_words + 1);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t per = (n_words + 1023) / 1024;
    const int64_t a = (int64_t)tid * per, b = (a + per < n_words) ? a + per : n_words;
    int64_t mine = 0;
    for (int64_t i = a; i < b; ++i) mine += __popcll(allow[i] & valid_bits(n_rows, i));
    int64_t inc = mine;                                        // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t up = __shfl_up(inc, o);
        inc += lane >= o ? up : 0;
    }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    int64_t base = 0;
    for (int ww = 0; ww < w; ++ww) base += wave_tot[ww];
    int64_t run = base + inc - mine;
    for (int64_t i = a; i < b; ++i) {
        off[i] = run;
        run += __popcll(allow[i] & valid_bits(n_rows, i));
    }
    if (tid == 1023) off[n_words] = base + inc;
}

// one lane per row: the rows of the bitmap in ascending order, at the offsets filter_scan_kernel wrote (filter.hip, boosted.hip)
__global__ __launch_bounds__(256) void filter_scatter_kernel(const uint64_t* __restrict__ allow, int64_t n_words, int64_t n_rows,
                                                              const int64_t* __restrict__ off, int64_t* __restrict__ rows,
                                                              const int* __restrict__ gate) {
    if (gate && !*gate) return;
    const int lane = threadIdx.x & 63;
    const int64_t wd = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wd >= n_words) return;
    const uint64_t word = allow[wd] & valid_bits(n_rows, wd);
    if ((word >> lane) & 1ull) rows[off[wd] + __popcll(word & ((1ull << lane) - 1ull))] = wd * GROUP_ROWS + lane;
}
