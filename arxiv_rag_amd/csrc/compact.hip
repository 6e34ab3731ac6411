// arx_compact_plan / arx_compact_rows / arx_compact_text: stable compaction of a shard's resident arrays under a row bitmap (gfx950; C ABI
// in include/arx.h).  What `HipCollection.compact()` runs to drop tombstoned rows from the fp16 shard, `group_of` and the text blob
// without a round trip through the host.
//
// Plan.  word_rank[w] = kept rows before 64-row word w, word_rank[n_words] = their total.  Three launches, on integers:
//   1. local   a block takes 256 words, scans their popcounts and stores the INCLUSIVE sums one entry up: word_rank[w + 1].  Its last
//              entry, word_rank[end of the block], is thereby the block's total.
//   2. totals  one block scans those last entries in place (inclusive): each becomes its final value, the last one the count.
//   3. add     block b >= 1 adds word_rank[first word of b] (final since 2) to its other entries.
// The block totals live in the output itself, so there is no workspace; no block ever waits for another inside a launch.
//
// Rows.  One block per 64-row word; a zero word costs its one load.  The kept rows of a word go to CONSECUTIVE rows of dst, so the
// block copies popcount x row_bytes bytes whose destination is one flat range: thread t moves units t, t + 256, ... of it (a unit is
// 16 bytes, or 1 byte when row_bytes or a pointer is not 16-byte aligned), four loads in flight before the four stores.  A unit's
// source row comes from a 64-entry LDS table of the word's set bits.  Only kept rows are read, only rows [0, count) written.
//
// Text.  new_row_off[new(r) + 1] = the kept rows' lengths, scanned the same three-launch way (a block takes 256 rows; its outputs are
// the consecutive entries (word_rank[first word], word_rank[end word]], the last of which holds its total); then one block per 64-row
// word moves the bytes, a wave per row: whole 16-byte chunks aligned on the DESTINATION address, each assembled from the two aligned
// 16-byte source chunks it straddles, and byte stores for the row's ragged head and tail (a neighbouring row owns the rest of those
// chunks).  Offsets are device data: a row is clamped into [0, row_off[n_rows]] as in csrc/textscan.hip, and a row that would be
// written beyond row_off[n_rows] bytes (possible only with offsets outside the contract) is skipped, so nothing is read or written
// out of range whatever the offsets hold.
// No float arithmetic, no atomics.
#include "arx_common.h"

namespace {

constexpr int CP_NT = 256, CP_WAVES = CP_NT / 64;
constexpr int CP_SCAN_NT = 1024;
constexpr int CP_TEXT_WORDS = CP_NT / 64;                     // keep-words a block of the text-length scan covers (a thread per row)
constexpr int CP_ROW_BYTES_MAX = 16384;

__device__ __forceinline__ unsigned long long keep_word(const unsigned long long* __restrict__ keep, int64_t w, int64_t n_rows) {
    unsigned long long v = keep[w];
    const int64_t left = n_rows - w * 64;                     // rows of this word: bits at or beyond n_rows may be garbage
    if (left < 64) v &= (1ull << left) - 1ull;
    return v;
}

// inclusive scan of one value per thread over a block of CP_NT threads; `total` = the block's sum
__device__ __forceinline__ long long block_scan(long long v, long long* s_wave, long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    long long before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < CP_WAVES; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    return before + inc;
}

// one block of CP_SCAN_NT threads: the m values get(0) .. get(m - 1) become their inclusive prefix sums through put(i, sum); -> the total
template <class Get, class Put>
__device__ __forceinline__ long long one_block_scan(int64_t m, Get get, Put put) {
    __shared__ long long s_sum[CP_SCAN_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seg = (m + CP_SCAN_NT - 1) / CP_SCAN_NT;
    const int64_t a = tid * seg < m ? tid * seg : m, b = a + seg < m ? a + seg : m;
    long long mine = 0;
    for (int64_t i = a; i < b; ++i) mine += get(i);
    long long inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) s_sum[wave] = inc;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CP_SCAN_NT / 64; ++w) {
        if (w < wave) before += s_sum[w];
        all += s_sum[w];
    }
    long long run = before + inc - mine;
    for (int64_t i = a; i < b; ++i) {
        run += get(i);
        put(i, run);
    }
    return all;
}

// ---- plan -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CP_NT) void plan_local_kernel(const unsigned long long* __restrict__ keep, int64_t n_rows, int64_t n_words,
                                                           long long* __restrict__ word_rank) {
    __shared__ long long s_wave[CP_WAVES];
    const int64_t w = (int64_t)blockIdx.x * CP_NT + threadIdx.x;
    long long total;
    const long long inc = block_scan(w < n_words ? (long long)__popcll(keep_word(keep, w, n_rows)) : 0, s_wave, total);
    if (w < n_words) word_rank[w + 1] = inc;
    if (w == 0) word_rank[0] = 0;
}

__device__ __forceinline__ int64_t plan_block_end(int64_t b, int64_t n_words) {
    return (b + 1) * CP_NT < n_words ? (b + 1) * CP_NT : n_words;
}

__global__ __launch_bounds__(CP_SCAN_NT) void plan_totals_kernel(int64_t n_words, int64_t n_blocks, long long* __restrict__ word_rank,
                                                                 long long* __restrict__ out_count) {
    const long long all = one_block_scan(
        n_blocks, [&](int64_t b) { return word_rank[plan_block_end(b, n_words)]; },
        [&](int64_t b, long long v) { word_rank[plan_block_end(b, n_words)] = v; });
    if (threadIdx.x == 0) *out_count = all;
}

__global__ __launch_bounds__(CP_NT) void plan_add_kernel(int64_t n_words, long long* __restrict__ word_rank) {
    const int64_t b = (int64_t)blockIdx.x + 1;               // (block 0 has nothing before it)
    const int64_t i = b * CP_NT + 1 + threadIdx.x;
    if (i < plan_block_end(b, n_words)) word_rank[i] += word_rank[b * CP_NT];
}

// ---- fixed-size rows ------------------------------------------------------------------------------------------------------------
// the set bits of `w` in ascending order -> s_row[0 .. popcount)
__device__ __forceinline__ void kept_rows_of(unsigned long long w, int* s_row) {
    const int tid = threadIdx.x;
    if (tid < 64 && ((w >> tid) & 1ull)) s_row[__popcll(w & ((1ull << tid) - 1ull))] = tid;
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(CP_NT) void compact_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, int units, int64_t n_rows,
                                                             const unsigned long long* __restrict__ keep,
                                                             const long long* __restrict__ word_rank, int64_t n_words) {
    __shared__ int s_row[64];
    const int64_t g = blockIdx.x;
    const unsigned long long w = keep_word(keep, g, n_rows);
    if (w == 0ull) return;                                    // (block-uniform)
    const int cnt = __popcll(w);
    const long long base = word_rank[g], count = word_rank[n_words];
    if (base < 0 || base + cnt > count || count > n_rows) return;      // a plan that is not this bitmap's: nothing is written out of dst's rows
    kept_rows_of(w, s_row);
    const T* s = src + g * 64 * units;
    T* d = dst + base * units;
    const int n = cnt * units;                                // <= 64 x 16 384
    const int dq = CP_NT / units, dr = CP_NT - dq * units;    // one step of CP_NT units = dq rows and dr units
    int j = (int)threadIdx.x / units, c = (int)threadIdx.x - j * units;
    for (int idx = threadIdx.x; idx < n; idx += 4 * CP_NT) {
        T v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (idx + k * CP_NT < n) v[k] = s[(int64_t)s_row[j] * units + c];
            c += dr; j += dq;
            if (c >= units) { c -= units; ++j; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (idx + k * CP_NT < n) d[idx + k * CP_NT] = v[k];
    }
}

// ---- texts ------------------------------------------------------------------------------------------------------------------------
// the row's bytes [a, b), clamped into the blob as csrc/textscan.hip clamps them
__device__ __forceinline__ void text_row(const int64_t* __restrict__ row_off, int64_t r, int64_t total, int64_t& a, int64_t& b) {
    a = row_off[r], b = row_off[r + 1];
    a = a < 0 ? 0 : (a > total ? total : a);
    b = b < a ? a : (b > total ? total : b);
}

__device__ __forceinline__ int64_t text_block_word(int64_t b, int64_t n_words) {
    return b * CP_TEXT_WORDS < n_words ? b * CP_TEXT_WORDS : n_words;
}

__global__ __launch_bounds__(CP_NT) void text_len_local_kernel(const int64_t* __restrict__ row_off, int64_t n_rows,
                                                               const unsigned long long* __restrict__ keep,
                                                               const long long* __restrict__ word_rank, int64_t n_words,
                                                               long long* __restrict__ new_row_off) {
    __shared__ long long s_wave[CP_WAVES];
    const int64_t r = (int64_t)blockIdx.x * CP_NT + threadIdx.x;
    const int64_t total = row_off[n_rows];
    const long long count = word_rank[n_words];
    bool kept = false;
    long long len = 0, pos = -1;
    if (r < n_rows) {
        const unsigned long long w = keep_word(keep, r >> 6, n_rows);
        if ((w >> (r & 63)) & 1ull) {
            pos = word_rank[r >> 6] + __popcll(w & ((1ull << (r & 63)) - 1ull));
            kept = pos >= 0 && pos < count && count <= n_rows;
            if (kept) {
                int64_t a, b;
                text_row(row_off, r, total, a, b);
                len = b - a;
            }
        }
    }
    long long block_total;
    const long long inc = block_scan(len, s_wave, block_total);
    if (kept) new_row_off[pos + 1] = inc;
    if (r == 0) new_row_off[0] = 0;
}

__global__ __launch_bounds__(CP_SCAN_NT) void text_len_totals_kernel(const long long* __restrict__ word_rank, int64_t n_words, int64_t n_blocks,
                                                                     long long* __restrict__ new_row_off) {
    const long long count = word_rank[n_words];
    auto span = [&](int64_t b, long long& first, long long& end) {      // block b wrote new_row_off(first, end]
        first = word_rank[text_block_word(b, n_words)];
        end = word_rank[text_block_word(b + 1, n_words)];
        return first >= 0 && end > first && end <= count;
    };
    one_block_scan(
        n_blocks,
        [&](int64_t b) { long long f, e; return span(b, f, e) ? new_row_off[e] : 0ll; },
        [&](int64_t b, long long v) { long long f, e; if (span(b, f, e)) new_row_off[e] = v; });
}

__global__ __launch_bounds__(CP_NT) void text_len_add_kernel(int64_t n_rows, const unsigned long long* __restrict__ keep,
                                                             const long long* __restrict__ word_rank, int64_t n_words,
                                                             long long* __restrict__ new_row_off) {
    const int64_t r = (int64_t)blockIdx.x * CP_NT + threadIdx.x;
    if (r >= n_rows) return;
    const long long count = word_rank[n_words];
    const long long first = word_rank[text_block_word(blockIdx.x, n_words)], end = word_rank[text_block_word((int64_t)blockIdx.x + 1, n_words)];
    if (first <= 0 || end <= first || end > count || count > n_rows) return;        // (first == 0: nothing before this block)
    const unsigned long long w = keep_word(keep, r >> 6, n_rows);
    if (!((w >> (r & 63)) & 1ull)) return;
    const long long at = word_rank[r >> 6] + __popcll(w & ((1ull << (r & 63)) - 1ull)) + 1;
    if (at > first && at < end) new_row_off[at] += new_row_off[first];               // (new_row_off[end] is final since the totals pass)
}

// 16 bytes at blob[pos, pos + 16), the address 16-B aligned; bytes outside [0, total) read as 0 and are never stored
__device__ __forceinline__ u32x4 text_load_chunk(const uint8_t* __restrict__ blob, int64_t pos, int64_t total) {
    if (pos >= 0 && pos + 16 <= total) return *(const u32x4*)(blob + pos);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (pos + 16 > 0 && pos < total) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t a = pos + i;
            if (a >= 0 && a < total) w[i >> 2] |= (uint32_t)blob[a] << (8 * (i & 3));
        }
    }
    const u32x4 v = {w[0], w[1], w[2], w[3]};
    return v;
}

// bytes [4 D + s, 4 D + s + 16) of the 32 bytes w[0..8), s in 0..3
template <int D>
__device__ __forceinline__ u32x4 text_shift(const uint32_t (&w)[8], int s) {
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (uint32_t)(((((uint64_t)w[k + D + 1]) << 32) | w[k + D]) >> (8 * s));
    const u32x4 v = {o[0], o[1], o[2], o[3]};
    return v;
}

__global__ __launch_bounds__(CP_NT) void compact_text_kernel(const uint8_t* __restrict__ blob, const int64_t* __restrict__ row_off, int64_t n_rows,
                                                             const unsigned long long* __restrict__ keep,
                                                             const long long* __restrict__ word_rank, int64_t n_words,
                                                             uint8_t* __restrict__ new_blob, const long long* __restrict__ new_row_off) {
    __shared__ int s_row[64];
    const int64_t g = blockIdx.x;
    const unsigned long long w = keep_word(keep, g, n_rows);
    if (w == 0ull) return;                                    // (block-uniform)
    const int cnt = __popcll(w);
    const long long base = word_rank[g], count = word_rank[n_words];
    if (base < 0 || base + cnt > count || count > n_rows) return;
    kept_rows_of(w, s_row);
    const int64_t total = row_off[n_rows];
    const int lane = threadIdx.x & 63;
    for (int j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); j < cnt; j += CP_WAVES) {       // (wave-uniform)
        int64_t a, b;
        text_row(row_off, g * 64 + s_row[j], total, a, b);
        const int64_t len = b - a, o = new_row_off[base + j];
        if (len == 0 || o < 0 || o + len > total) continue;   // (the second: offsets outside the contract; nothing goes beyond the old total)
        uint8_t* d = new_blob + o;
        const uint8_t* s = blob + a;
        int64_t head = (int64_t)((16 - ((uintptr_t)d & 15)) & 15);     // bytes before d's first aligned chunk
        if (head > len) head = len;
        if (lane < head) d[lane] = s[lane];
        const int64_t n_chunks = (len - head) >> 4;
        const int sh = (int)(((uintptr_t)s + head) & 15);     // the source's misalignment against the destination's chunk grid
        for (int64_t k = lane; k < n_chunks; k += 64) {
            const int64_t p = a + head + 16 * k;              // blob position of this chunk's byte 0
            u32x4 v;
            if (sh == 0) {
                v = text_load_chunk(blob, p, total);
            } else {
                const u32x4 lo = text_load_chunk(blob, p - sh, total), hi = text_load_chunk(blob, p - sh + 16, total);
                const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                switch (sh >> 2) {                            // (wave-uniform)
                    case 0: v = text_shift<0>(x, sh & 3); break;
                    case 1: v = text_shift<1>(x, sh & 3); break;
                    case 2: v = text_shift<2>(x, sh & 3); break;
                    default: v = text_shift<3>(x, sh & 3); break;
                }
            }
            *(u32x4*)(d + head + 16 * k) = v;
        }
        const int64_t done = head + 16 * n_chunks;
        if (lane < len - done) d[done + lane] = s[done + lane];
    }
}

bool rows_in_range(int64_t n_rows) { return n_rows >= 0 && n_rows < ((int64_t)1 << 36); }

}  // namespace

extern "C" int32_t arx_compact_plan(const uint64_t* keep, int64_t n_rows, int64_t* word_rank, int64_t* out_count, void* stream) {
    ARX_REQUIRE(rows_in_range(n_rows), "n_rows=%lld must be in [0, 2^36)", (long long)n_rows);
    ARX_REQUIRE(word_rank, "word_rank is a null pointer");
    ARX_REQUIRE(out_count, "out_count is a null pointer");
    ARX_REQUIRE(keep || n_rows == 0, "keep is a null pointer (n_rows=%lld)", (long long)n_rows);
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        ARX_HIP_CHECK(hipMemsetAsync(word_rank, 0, sizeof(int64_t), st));
        ARX_HIP_CHECK(hipMemsetAsync(out_count, 0, sizeof(int64_t), st));
        return ARX_OK;
    }
    const int64_t n_words = (n_rows + 63) >> 6, n_blocks = (n_words + CP_NT - 1) / CP_NT;
    const unsigned long long* k = (const unsigned long long*)keep;
    plan_local_kernel<<<(unsigned)n_blocks, CP_NT, 0, st>>>(k, n_rows, n_words, (long long*)word_rank);
    plan_totals_kernel<<<1, CP_SCAN_NT, 0, st>>>(n_words, n_blocks, (long long*)word_rank, (long long*)out_count);
    if (n_blocks > 1) plan_add_kernel<<<(unsigned)(n_blocks - 1), CP_NT, 0, st>>>(n_words, (long long*)word_rank);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_compact_rows(const void* src, void* dst, int64_t row_bytes, int64_t n_rows, const uint64_t* keep, const int64_t* word_rank,
                                    void* stream) {
    ARX_REQUIRE(rows_in_range(n_rows), "n_rows=%lld must be in [0, 2^36)", (long long)n_rows);
    ARX_REQUIRE(row_bytes >= 1 && row_bytes <= CP_ROW_BYTES_MAX, "row_bytes=%lld must be in [1, %d]", (long long)row_bytes, CP_ROW_BYTES_MAX);
    ARX_REQUIRE(src, "src is a null pointer");
    ARX_REQUIRE(dst, "dst is a null pointer");
    ARX_REQUIRE(keep, "keep is a null pointer");
    ARX_REQUIRE(word_rank, "word_rank is a null pointer");
    if (n_rows == 0) return ARX_OK;
    const int64_t n_words = (n_rows + 63) >> 6;
    const unsigned long long* k = (const unsigned long long*)keep;
    hipStream_t st = (hipStream_t)stream;
    if (row_bytes % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0)
        compact_rows_kernel<u32x4><<<(unsigned)n_words, CP_NT, 0, st>>>((const u32x4*)src, (u32x4*)dst, (int)(row_bytes / 16), n_rows, k,
                                                                         (const long long*)word_rank, n_words);
    else
        compact_rows_kernel<uint8_t><<<(unsigned)n_words, CP_NT, 0, st>>>((const uint8_t*)src, (uint8_t*)dst, (int)row_bytes, n_rows, k,
                                                                           (const long long*)word_rank, n_words);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_compact_text(const uint8_t* blob, const int64_t* row_off, int64_t n_rows, const uint64_t* keep, const int64_t* word_rank,
                                    uint8_t* new_blob, int64_t* new_row_off, void* stream) {
    ARX_REQUIRE(rows_in_range(n_rows), "n_rows=%lld must be in [0, 2^36)", (long long)n_rows);
    ARX_REQUIRE(blob, "blob is a null pointer");
    ARX_REQUIRE(row_off, "row_off is a null pointer");
    ARX_REQUIRE(word_rank, "word_rank is a null pointer");
    ARX_REQUIRE(new_blob, "new_blob is a null pointer");
    ARX_REQUIRE(new_row_off, "new_row_off is a null pointer");
    ARX_REQUIRE(keep || n_rows == 0, "keep is a null pointer (n_rows=%lld)", (long long)n_rows);
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        ARX_HIP_CHECK(hipMemsetAsync(new_row_off, 0, sizeof(int64_t), st));
        return ARX_OK;
    }
    const int64_t n_words = (n_rows + 63) >> 6, n_blocks = (n_rows + CP_NT - 1) / CP_NT;
    const unsigned long long* k = (const unsigned long long*)keep;
    const long long* wr = (const long long*)word_rank;
    long long* out = (long long*)new_row_off;
    text_len_local_kernel<<<(unsigned)n_blocks, CP_NT, 0, st>>>(row_off, n_rows, k, wr, n_words, out);
    text_len_totals_kernel<<<1, CP_SCAN_NT, 0, st>>>(wr, n_words, n_blocks, out);
    text_len_add_kernel<<<(unsigned)n_blocks, CP_NT, 0, st>>>(n_rows, k, wr, n_words, out);
    compact_text_kernel<<<(unsigned)n_words, CP_NT, 0, st>>>(blob, row_off, n_rows, k, wr, n_words, new_blob, out);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
