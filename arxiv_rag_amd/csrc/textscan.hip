// arx_text_contains: which rows of a shard's chunk texts contain which byte patterns (C ABI in include/arx.h; Chroma's `where_document`).
// The producer of the row bitmaps arx_topk_search_filtered consumes (csrc/filter.hip reads the same layout).
//
// One block owns one 64-row group, hence one output word per pattern, which it writes once with a plain store: no atomics on
// global memory, no zero-fill pass, and the bits cannot depend on the order in which anything ran.  Inside the block wave w takes rows
// w, w + 4, ... of the group (a row belongs to one wave from start to end; neighbouring rows go to different waves, so a run of long
// rows is spread); a single very long row is scanned by one wave alone ("where_document").
//
// A wave streams its row in tiles of 1024 bytes, 16 B per lane, coalesced and 16-B aligned on the ADDRESS (the tile grid is laid over
// the blob's address, not over the row, so every full chunk is one global_load_dwordx4; the chunks that hang over either end of the
// blob are assembled from guarded byte loads).  The tile goes to LDS with a halo of max(max_len - 1, 3) bytes behind it, so a lane can
// finish a comparison that runs into its neighbours' bytes.  Each lane tests the 16 start positions of its own chunk: the 4-byte
// window at every position is built once per tile from five registers and compared with the pattern's first min(len, 4) bytes under
// a mask; for len <= 4 that is the whole answer, longer patterns compare the rest out of LDS at the (rare) surviving positions.
// A start position counts only if the whole match lies in [row_off[r], row_off[r + 1]): the blob has no separators, the bound is
// arithmetic.  A (row, pattern) that has matched is not tested again and the row ends when every pattern has.
//
// arx_text_regex: which rows contain a match of which regular expression (`$regex` / `$not_regex`), same output contract.  The host
// compiles a regex to a byte-level DFA (arxiv_rag_amd/regex_dfa.py); the kernel only walks tables.  The regex is blockIdx.y: a block
// stages ONE table in LDS (up to 256 x 256 transitions + 512 bytes of classes and flags = 66 048 B, so two blocks share a CU's 160 KiB;
// the eight worst-case tables of a call would not fit at once) and every wave of the block owns one 64-row group, hence one output
// word, which it ballots and writes once.  A DFA run is sequential in a row's bytes, so a lane owns a row and carries its state from
// start to end.  Unlike the substring scan, the text does not go through LDS: a lane reads its own row 16 bytes at a time (aligned on
// the address, the next chunk in flight while it walks this one) and steps through them in registers, two dependent LDS reads per
// byte (class, then transition).  A chunk staged for the whole group would cover few rows at a time at arXiv chunk lengths (~1 KB a
// row, 64 KB a group) and leave most lanes idle in a loop whose cost is the table walk, not the load; a 128-byte line is read by one
// lane in eight consecutive steps and stays in L1 / L2 meanwhile, so HBM is still read once.  A lane stops at a MATCHED or DEAD
// state (both absorbing, so looking at the flags once per chunk changes no bit) or at its row's end; the wave stops when all have.
#include "arx_common.h"

namespace {
constexpr int TS_NT = 256, TS_WAVES = TS_NT / 64;
constexpr int TS_TILE = 1024;                                 // bytes of start positions per wave step: 64 lanes x 16 B
constexpr int TS_MAXP = 32, TS_MAXLEN = 256;
constexpr int TS_HALO = 256;                                  // the 255 bytes a match starting at the tile's last byte runs on (its window's 3 are the first of them), in 16-B chunks
constexpr int TS_BUF = TS_TILE + TS_HALO;

// 16 bytes at blob[pos, pos + 16) (the address is 16-B aligned by construction); bytes outside [0, total) read as 0 and are never part of a match
__device__ __forceinline__ u32x4 ts_load_chunk(const uint8_t* __restrict__ blob, int64_t pos, int64_t total) {
    if (pos >= 0 && pos + 16 <= total) return *(const u32x4*)(blob + pos);
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (pos + 16 > 0 && pos < total) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t a = pos + i;
            const uint32_t b = (a >= 0 && a < total) ? (uint32_t)blob[a] << (8 * (i & 3)) : 0u;
            if (i < 4) w0 |= b; else if (i < 8) w1 |= b; else if (i < 12) w2 |= b; else w3 |= b;
        }
    }
    const u32x4 v = {w0, w1, w2, w3};
    return v;
}

// LDS traffic inside ONE wave (a write by one lane, a read by another): the hardware keeps a wave's DS operations in order; this keeps the compiler from
// moving them across and waits for the writes
__device__ __forceinline__ void ts_wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(TS_NT) void text_contains_kernel(const uint8_t* __restrict__ blob, const int64_t* __restrict__ row_off, int64_t n_rows,
                                                              const uint8_t* __restrict__ pat_blob, const int32_t* __restrict__ pat_off, int n_pat,
                                                              int64_t n_words, unsigned long long* __restrict__ out_bits) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[TS_WAVES][TS_BUF];
    __shared__ __attribute__((aligned(16))) uint8_t s_pat[TS_MAXP * TS_MAXLEN];
    __shared__ uint32_t s_pre[TS_MAXP], s_msk[TS_MAXP];
    __shared__ int s_len[TS_MAXP];
    __shared__ uint32_t s_found[64];
    __shared__ int s_maxlen;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t g = blockIdx.x;
    if (tid < 64) s_found[tid] = 0;
    if (tid < n_pat) {
        int len = pat_off[tid + 1] - pat_off[tid];
        if (len < 1 || len > TS_MAXLEN) len = 0;             // outside the contract: such a pattern matches nothing (and is not copied)
        s_len[tid] = len;
    }
    __syncthreads();
    for (int p = 0; p < n_pat; ++p) {
        const int len = s_len[p];
        const uint8_t* src = pat_blob + pat_off[p];
        for (int i = tid; i < len; i += TS_NT) s_pat[p * TS_MAXLEN + i] = src[i];
    }
    __syncthreads();
    if (tid < n_pat) {
        const int len = s_len[tid];
        uint32_t pre = 0;
        for (int i = 0; i < 4 && i < len; ++i) pre |= (uint32_t)s_pat[tid * TS_MAXLEN + i] << (8 * i);
        s_pre[tid] = pre;
        s_msk[tid] = len >= 4 ? 0xffffffffu : ((1u << (8 * len)) - 1u);
    }
    if (tid == 0) {
        int m = 1;
        for (int p = 0; p < n_pat; ++p) m = s_len[p] > m ? s_len[p] : m;
        s_maxlen = m;
    }
    __syncthreads();
    uint32_t live = 0;                                        // patterns that can match at all
    for (int p = 0; p < n_pat; ++p) live |= (s_len[p] > 0 ? 1u : 0u) << p;
    live = __builtin_amdgcn_readfirstlane(live);              // a scalar: the loops below that depend on it branch uniformly
    // the max_len - 1 bytes that a match starting at the tile's last byte runs on, and at least the 3 of the last lane's window; 1..16
    const int halo_chunks = ((s_maxlen > 4 ? s_maxlen - 1 : 3) + 15) >> 4;
    const int64_t total = row_off[n_rows];
    const int64_t shift = (int64_t)((uintptr_t)blob & 15);    // tile grid in v = pos + shift: v % 16 == 0 <=> the address is 16-B aligned
    const int64_t rows_left = n_rows - g * 64;
    const int rows_here = rows_left < 64 ? (int)rows_left : 64;
    uint8_t* tile = s_tile[wave];

    for (int r = __builtin_amdgcn_readfirstlane(wave); r < rows_here; r += TS_WAVES) {     // (wave-uniform: the whole loop nest branches on scalars)
        int64_t a = row_off[g * 64 + r], b = row_off[g * 64 + r + 1];
        a = a < 0 ? 0 : (a > total ? total : a);
        b = b < a ? a : (b > total ? total : b);
        uint32_t rem = live, found = 0;
        for (int64_t v = (a + shift) & ~(int64_t)15; v - shift < b && rem != 0; v += TS_TILE) {
            const int64_t lane_pos = v - shift + lane * 16;  // blob position of this lane's byte 0
            // (chunks wholly behind the row's end are not fetched: no valid start position reaches into them, what LDS holds there is never compared)
            if (lane_pos < b) *(u32x4*)(tile + lane * 16) = ts_load_chunk(blob, lane_pos, total);
            if (lane < halo_chunks && lane_pos + TS_TILE < b) *(u32x4*)(tile + TS_TILE + lane * 16) = ts_load_chunk(blob, lane_pos + TS_TILE, total);
            ts_wave_lds_fence();
            const u32x4 c = *(const u32x4*)(tile + lane * 16);
            const uint32_t c4 = *(const uint32_t*)(tile + lane * 16 + 16);
            const uint32_t w[5] = {c.x, c.y, c.z, c.w, c4};
            uint32_t win[16];                                 // the 4 bytes at each of the lane's 16 start positions
#pragma unroll
            for (int j = 0; j < 16; ++j)
                win[j] = (uint32_t)(((((uint64_t)w[j / 4 + 1]) << 32) | w[j / 4]) >> (8 * (j % 4)));
            const int64_t lo64 = a - lane_pos;
            const int lo = lo64 <= 0 ? 0 : (lo64 >= 16 ? 16 : (int)lo64);
            uint32_t todo = rem;
            while (todo) {                                    // wave-uniform
                const int p = __builtin_ctz(todo);
                todo &= todo - 1;
                const int len = s_len[p];
                const uint32_t pre = s_pre[p], msk = s_msk[p];
                const int64_t hi64 = b - len - lane_pos + 1;  // start positions j < hi end inside the row
                const int hi = hi64 <= 0 ? 0 : (hi64 >= 16 ? 16 : (int)hi64);
                uint32_t cm = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) cm |= ((win[j] & msk) == pre ? 1u : 0u) << j;
                cm &= hi > lo ? (((1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u;
                bool hit = false;
                if (len <= 4) {
                    hit = cm != 0;
                } else {
                    const uint8_t* pat = s_pat + p * TS_MAXLEN;
                    while (cm != 0 && !hit) {
                        const int j = __builtin_ctz(cm);
                        cm &= cm - 1;
                        const uint8_t* t = tile + lane * 16 + j;
                        int i = 4;
                        while (i < len && t[i] == pat[i]) ++i;
                        hit = i == len;
                    }
                }
                if (__any(hit ? 1 : 0)) { rem &= ~(1u << p); found |= 1u << p; }
            }
            ts_wave_lds_fence();                              // every lane is done with the tile before the next one overwrites it
        }
        if (lane == 0) s_found[r] = found;
    }
    __syncthreads();
    if (wave == 0) {
        const uint32_t f = lane < rows_here ? s_found[lane] : 0u;
        for (int p = 0; p < n_pat; ++p) {
            const unsigned long long word = __ballot((f >> p) & 1u);
            if (lane == 0) out_bits[(int64_t)p * n_words + g] = word;
        }
    }
}

constexpr int TR_MAXRE = 8, TR_MAXS = 256, TR_MAXC = 256;
constexpr int TR_HEAD = 4;                                    // uint16 n_states, uint16 n_classes, little-endian
constexpr uint32_t TR_MATCHED = 1, TR_ACCEPT_AT_END = 2, TR_DEAD = 4;

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void text_regex_kernel(const uint8_t* __restrict__ blob, const int64_t* __restrict__ row_off, int64_t n_rows,
                                                                const uint8_t* __restrict__ tables, const int32_t* __restrict__ table_off,
                                                                int64_t n_words, unsigned long long* __restrict__ out_bits) {
    __shared__ __attribute__((aligned(16))) uint8_t s_trans[TR_MAXS * TR_MAXC];
    __shared__ uint8_t s_cls[256], s_flags[TR_MAXS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int p = blockIdx.y;
    // the header and the table's size are device data: anything outside the contract makes this regex match no row, and every staged
    // class and transition is forced into range, so no index below can leave s_cls / s_flags / s_trans whatever the table holds
    const int64_t t0 = table_off[p], t_bytes = (int64_t)table_off[p + 1] - t0;
    const uint8_t* tab = tables + t0;
    int ns = 0, nc = 0;
    if (t0 >= 0 && t_bytes >= TR_HEAD) {
        ns = (int)tab[0] | ((int)tab[1] << 8);
        nc = (int)tab[2] | ((int)tab[3] << 8);
    }
    const bool ok = ns >= 1 && ns <= TR_MAXS && nc >= 1 && nc <= TR_MAXC && t_bytes >= TR_HEAD + 256 + ns + ns * nc;     // (block-uniform)
    if (ok) {
        for (int i = tid; i < 256; i += WAVES * 64) {
            const uint8_t c = tab[TR_HEAD + i];
            s_cls[i] = c < nc ? c : 0;
        }
        for (int i = tid; i < ns; i += WAVES * 64) s_flags[i] = tab[TR_HEAD + 256 + i];
        const uint8_t* tr = tab + TR_HEAD + 256 + ns;
        for (int i = tid; i < ns * nc; i += WAVES * 64) {
            const uint8_t t = tr[i];
            s_trans[i] = t < ns ? t : 0;
        }
    }
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * WAVES + wave;     // this wave's 64-row group
    if (g >= n_words) return;
    const int64_t total = row_off[n_rows];
    const int64_t shift = (int64_t)((uintptr_t)blob & 15);    // chunk grid laid over the address, as in text_contains_kernel
    const int64_t r = g * 64 + lane;
    int64_t a = 0, b = 0;
    if (r < n_rows) {
        a = row_off[r], b = row_off[r + 1];
        a = a < 0 ? 0 : (a > total ? total : a);
        b = b < a ? a : (b > total ? total : b);
    }
    uint32_t state = 0;
    bool run = ok && a < b && (s_flags[0] & (TR_MATCHED | TR_DEAD)) == 0;
    int64_t base = ((a + shift) & ~(int64_t)15) - shift;      // blob position of this lane's chunk; the address is 16-B aligned
    u32x4 cur = {0, 0, 0, 0};
    if (run) cur = ts_load_chunk(blob, base, total);
    while (__any(run ? 1 : 0)) {
        const bool more = run && base + 16 < b;
        u32x4 nxt = {0, 0, 0, 0};
        if (more) nxt = ts_load_chunk(blob, base + 16, total);
        if (run) {
            const int64_t lo64 = a - base, hi64 = b - base;   // bytes [lo, hi) of the chunk are the row's
            const int lo = lo64 <= 0 ? 0 : (int)lo64, hi = hi64 >= 16 ? 16 : (int)hi64;
            const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t byte = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                if (j >= lo && j < hi) state = s_trans[state * (uint32_t)nc + s_cls[byte]];
            }
            run = more && (s_flags[state] & (TR_MATCHED | TR_DEAD)) == 0;
        }
        cur = nxt;
        base += 16;
    }
    const bool hit = ok && r < n_rows && (s_flags[state] & (TR_MATCHED | TR_ACCEPT_AT_END)) != 0;
    const unsigned long long word = __ballot(hit ? 1 : 0);
    if (lane == 0) out_bits[(int64_t)p * n_words + g] = word;
}

// one block: the count is a plain store of one block's sum (nothing to zero, nothing to order)
__global__ __launch_bounds__(1024) void bitmap_count_kernel(const unsigned long long* __restrict__ bits, int64_t n_rows, long long* __restrict__ out) {
    __shared__ long long s_part[16];
    const int64_t n_words = (n_rows + 63) >> 6;
    const int tail = (int)(n_rows & 63);
    long long c = 0;
    for (int64_t i = threadIdx.x; i < n_words; i += 1024) {
        unsigned long long w = bits[i];
        if (tail && i == n_words - 1) w &= (1ull << tail) - 1ull;
        c += __popcll(w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int i = 0; i < 16; ++i) t += s_part[i];
        *out = t;
    }
}
}      // namespace

extern "C" int32_t arx_text_contains(const uint8_t* blob, const int64_t* row_off, int64_t n_rows, const uint8_t* pat_blob, const int32_t* pat_off,
                                     int32_t n_pat, uint64_t* out_bits, void* stream) {
    ARX_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 36), "n_rows=%lld must be in 1..2^36-1", (long long)n_rows);
    ARX_REQUIRE(n_pat >= 1 && n_pat <= TS_MAXP, "n_pat=%d out of range 1..%d", n_pat, TS_MAXP);
    // (a shard of empty rows only still passes a valid blob pointer: the row lengths are device data, the entry point cannot look)
    ARX_REQUIRE(blob && row_off && pat_blob && pat_off && out_bits, "null pointer argument");
    const int64_t n_words = (n_rows + 63) >> 6;
    text_contains_kernel<<<(unsigned)n_words, TS_NT, 0, (hipStream_t)stream>>>(blob, row_off, n_rows, pat_blob, pat_off, n_pat, n_words,
                                                                              (unsigned long long*)out_bits);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_text_regex_tuned(const uint8_t* blob, const int64_t* row_off, int64_t n_rows, const uint8_t* tables, const int32_t* table_off,
                                        int32_t n_re, uint64_t* out_bits, int32_t waves_per_block, void* stream) {
    ARX_REQUIRE(n_rows > 0 && n_rows < ((int64_t)1 << 36), "n_rows=%lld must be in 1..2^36-1", (long long)n_rows);
    ARX_REQUIRE(n_re >= 1 && n_re <= TR_MAXRE, "n_re=%d out of range 1..%d", n_re, TR_MAXRE);
    ARX_REQUIRE(blob && row_off && tables && table_off && out_bits, "null pointer argument");
    const int64_t n_words = (n_rows + 63) >> 6;
    const int waves = waves_per_block == 0 ? 8 : waves_per_block;         // 8: two blocks a CU (LDS) = 16 waves walking
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* out = (unsigned long long*)out_bits;
#define TR_LAUNCH(W)                                                                                                                  \
    case W:                                                                                                                           \
        text_regex_kernel<W><<<dim3((unsigned)((n_words + W - 1) / W), (unsigned)n_re), W * 64, 0, st>>>(blob, row_off, n_rows, tables, \
                                                                                                          table_off, n_words, out);  \
        break;
    switch (waves) {
        TR_LAUNCH(1) TR_LAUNCH(2) TR_LAUNCH(4) TR_LAUNCH(8) TR_LAUNCH(16)
        default: ARX_REQUIRE(false, "waves_per_block=%d must be 0 (default), 1, 2, 4, 8 or 16", waves_per_block);
    }
#undef TR_LAUNCH
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_text_regex(const uint8_t* blob, const int64_t* row_off, int64_t n_rows, const uint8_t* tables, const int32_t* table_off,
                                  int32_t n_re, uint64_t* out_bits, void* stream) {
    return arx_text_regex_tuned(blob, row_off, n_rows, tables, table_off, n_re, out_bits, 0, stream);
}

extern "C" int32_t arx_bitmap_count(const uint64_t* bits, int64_t n_rows, int64_t* out_count, void* stream) {
    ARX_REQUIRE(n_rows > 0, "n_rows=%lld must be positive", (long long)n_rows);
    ARX_REQUIRE(bits && out_count, "null pointer argument");
    bitmap_count_kernel<<<1, 1024, 0, (hipStream_t)stream>>>((const unsigned long long*)bits, n_rows, (long long*)out_count);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
