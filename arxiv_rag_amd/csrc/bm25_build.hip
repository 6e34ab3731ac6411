// arx_bm25_build_postings / arx_bm25_build_impacts: the BM25 keyword index of arxiv_rag_amd/keyword.py built on the device (gfx950;
// C ABI in include/arx.h).  The two calls compute `build_postings` and `impacts_f64(...).astype(float32)`, bit for bit.
//
// Postings.  Tokens arrive in row order, so a STABLE sort by term id alone leaves them in (term, row) order:
//   1. init      key[i] = pieces[i], row[i] = the document whose [doc_ptr[r], doc_ptr[r + 1]) holds i (a binary search: empty documents
//                own no token).  An id outside [0, vocab) sets the flag (a plain store of 1) and is sorted as term 0, so everything
//                after it stays in range.
//   2. sort      LSD radix sort, 8-bit digits, ceil(bits(vocab - 1) / 8) passes, the row as payload.  A pass is three launches: each
//                block counts the digits of its contiguous chunk of tokens in LDS (integer LDS atomics, the only atomics of this file)
//                and stores them digit-major; one block scans the 256 x blocks counts; each block then walks its chunk 256 tokens at
//                a time and scatters them in order: a token's place is its digit's running base + the tokens of that digit in earlier
//                waves of the round + those in lower lanes of its wave (eight ballots), which is the stable order whatever the chunk
//                size or the block count.
//   3. heads     position i heads a run when (key, row) differs from position i - 1.  Each block counts the heads of its chunk, one
//                block scans the counts (and stores P), each block then numbers its heads: slot[i] = heads before i, start[slot] = i.
//   4. emit      posting s: post_row = row[start[s]], post_tf = start[s + 1] - start[s] (n_tokens for the last one).
//   5. term_ptr  term_ptr[t] = slot of the first sorted position whose key is >= t (a binary search per term), P when there is none.
// The sorted order, the heads and their numbering are each one defined array, so the output does not depend on tile_tokens or on
// max_blocks.  No global atomics, no float atomics.
//
// Impacts.  One thread per posting: its term is the last t with term_ptr[t] <= s (a binary search), dl = doc_ptr[row + 1] - doc_ptr[row],
//   norm = K1 * ((1.0 - B) + (B * dl) / avgdl);  w = ((idf[t] * tf) * (K1 + 1.0)) / (tf + norm)     in float64, numpy's operation order,
// rounded once to f32.  No FMA contraction: this file is compiled with -ffp-contract=off (csrc/build.sh) AND carries the pragma below;
// the f64 divisions are the compiler's IEEE-rounded sequence (no fast-math flag is given).  idf comes from the host, so log1p never
// runs here.
#include "arx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLD_NT = 256;                 // threads of a block = tokens of a round = radix
constexpr int BLD_WAVES = BLD_NT / 64;
constexpr int BLD_TILE = 2048;              // default tile_tokens: a block's chunk is a whole number of tiles
constexpr int BLD_TILE_MAX = 65536;
constexpr int BLD_MAX_BLOCKS = 2048;        // the workspace's histogram area is sized for this many
constexpr int SCAN_NT = 1024;
constexpr double BM25_K1 = 1.2, BM25_B = 0.75;

struct Chunks {                             // block b owns tokens [b * chunk, min(n, (b + 1) * chunk))
    long long n, chunk;
    int blocks;
};

__device__ __forceinline__ void chunk_range(const Chunks& c, long long& lo, long long& hi) {
    lo = (long long)blockIdx.x * c.chunk;
    hi = lo + c.chunk < c.n ? lo + c.chunk : c.n;
}

__global__ __launch_bounds__(BLD_NT) void build_init_kernel(const int32_t* __restrict__ pieces, long long n_tokens,
                                                            const long long* __restrict__ doc_ptr, long long n_docs, int vocab,
                                                            uint32_t* __restrict__ key, uint32_t* __restrict__ row, int32_t* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * BLD_NT + threadIdx.x;
    if (i >= n_tokens) return;
    int32_t p = pieces[i];
    if (p < 0 || p >= vocab) { *bad = 1; p = 0; }
    long long lo = 0, hi = n_docs - 1;                       // the last r in [0, n_docs) with doc_ptr[r] <= i
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (doc_ptr[mid] <= i) lo = mid; else hi = mid - 1;
    }
    key[i] = (uint32_t)p;
    row[i] = (uint32_t)lo;
}

__global__ __launch_bounds__(BLD_NT) void build_hist_kernel(const uint32_t* __restrict__ key, Chunks c, int shift, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[BLD_NT];
    h[threadIdx.x] = 0u;
    __syncthreads();
    long long lo, hi;
    chunk_range(c, lo, hi);
    for (long long i = lo + threadIdx.x; i < hi; i += BLD_NT) atomicAdd(&h[(key[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[(long long)threadIdx.x * c.blocks + blockIdx.x] = h[threadIdx.x];
}

// data[0 .. n) becomes its exclusive prefix sum; *total (when given) the sum.  One block.
__global__ __launch_bounds__(SCAN_NT) void build_scan_kernel(uint32_t* __restrict__ data, int n, long long* __restrict__ total) {
    __shared__ uint32_t wsum[SCAN_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = (n + SCAN_NT - 1) / SCAN_NT;
    const int a = tid * seg < n ? tid * seg : n, b = a + seg < n ? a + seg : n;
    uint32_t mine = 0u;
    for (int i = a; i < b; ++i) mine += data[i];
    uint32_t inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < SCAN_NT / 64; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    uint32_t run = before + inc - mine;
    for (int i = a; i < b; ++i) {
        const uint32_t v = data[i];
        data[i] = run;
        run += v;
    }
    if (total && tid == 0) *total = (long long)all;
}

__global__ __launch_bounds__(BLD_NT) void build_scatter_kernel(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ row_in,
                                                               Chunks c, int shift, const uint32_t* __restrict__ hist,
                                                               uint32_t* __restrict__ key_out, uint32_t* __restrict__ row_out) {
    __shared__ uint32_t base[BLD_NT];                        // where the next token of each digit goes
    __shared__ uint32_t cnt[BLD_WAVES][BLD_NT];              // tokens of each digit in each wave of this round
    __shared__ uint32_t woff[BLD_WAVES][BLD_NT];             // ... and where each wave's first one goes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    base[tid] = hist[(long long)tid * c.blocks + blockIdx.x];
#pragma unroll
    for (int w = 0; w < BLD_WAVES; ++w) cnt[w][tid] = 0u;
    long long lo, hi;
    chunk_range(c, lo, hi);
    __syncthreads();
    for (long long r = lo; r < hi; r += BLD_NT) {
        const long long i = r + tid;
        const bool valid = i < hi;
        uint32_t k = 0u, pay = 0u;
        if (valid) { k = key_in[i]; pay = row_in[i]; }
        const uint32_t d = (k >> shift) & 255u;
        unsigned long long same = __ballot(valid);           // the lanes of this wave with my digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long has = __ballot(valid && ((d >> bit) & 1u));
            same &= ((d >> bit) & 1u) ? has : ~has;
        }
        if (valid && (same & below) == 0ull) cnt[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        {                                                    // thread tid serves digit tid
            uint32_t run = base[tid];
#pragma unroll
            for (int w = 0; w < BLD_WAVES; ++w) {
                woff[w][tid] = run;
                run += cnt[w][tid];
                cnt[w][tid] = 0u;
            }
            base[tid] = run;
        }
        __syncthreads();
        if (valid) {
            const uint32_t dst = woff[wave][d] + (uint32_t)__popcll(same & below);
            key_out[dst] = k;
            row_out[dst] = pay;
        }
    }
}

__device__ __forceinline__ bool is_head(const uint32_t* __restrict__ key, const uint32_t* __restrict__ row, long long i) {
    return i == 0 || key[i] != key[i - 1] || row[i] != row[i - 1];
}

__global__ __launch_bounds__(BLD_NT) void build_head_count_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ row, Chunks c,
                                                                  uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[BLD_WAVES];
    long long lo, hi;
    chunk_range(c, lo, hi);
    uint32_t mine = 0u;
    for (long long i = lo + threadIdx.x; i < hi; i += BLD_NT) mine += is_head(key, row, i) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0u;
#pragma unroll
        for (int w = 0; w < BLD_WAVES; ++w) all += wsum[w];
        counts[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(BLD_NT) void build_head_slot_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ row, Chunks c,
                                                                 const uint32_t* __restrict__ counts, uint32_t* __restrict__ slot,
                                                                 uint32_t* __restrict__ start) {
    __shared__ uint32_t wcnt[2][BLD_WAVES];                  // (two copies: one barrier per round)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    long long lo, hi;
    chunk_range(c, lo, hi);
    uint32_t run = counts[blockIdx.x];                       // heads before this round
    int buf = 0;
    for (long long r = lo; r < hi; r += BLD_NT, buf ^= 1) {
        const long long i = r + tid;
        const bool valid = i < hi;
        const bool head = valid && is_head(key, row, i);
        const unsigned long long heads = __ballot(head);
        if (lane == 0) wcnt[buf][wave] = (uint32_t)__popcll(heads);
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (int w = 0; w < BLD_WAVES; ++w) {
            if (w < wave) before += wcnt[buf][w];
            all += wcnt[buf][w];
        }
        if (valid) {
            const uint32_t s = run + before + (uint32_t)__popcll(heads & below);
            slot[i] = s;
            if (head) start[s] = (uint32_t)i;
        }
        run += all;
    }
}

__global__ __launch_bounds__(BLD_NT) void build_emit_kernel(const uint32_t* __restrict__ row, const uint32_t* __restrict__ start,
                                                            long long n_tokens, const long long* __restrict__ n_post,
                                                            uint32_t* __restrict__ post_row, int32_t* __restrict__ post_tf) {
    const long long s = (long long)blockIdx.x * BLD_NT + threadIdx.x, P = *n_post;      // P <= n_tokens
    if (s >= n_tokens || s >= P) return;
    const uint32_t a = start[s];
    const long long b = s + 1 < P ? (long long)start[s + 1] : n_tokens;
    post_row[s] = row[a];
    post_tf[s] = (int32_t)(b - (long long)a);
}

__global__ __launch_bounds__(BLD_NT) void build_term_ptr_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ slot,
                                                                long long n_tokens, const long long* __restrict__ n_post, int vocab,
                                                                long long* __restrict__ term_ptr) {
    const long long t = (long long)blockIdx.x * BLD_NT + threadIdx.x;
    if (t > vocab) return;
    long long lo = 0, hi = n_tokens;                         // the first i with key[i] >= t
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)key[mid] < t) lo = mid + 1; else hi = mid;
    }
    term_ptr[t] = lo < n_tokens ? (long long)slot[lo] : *n_post;
}

__global__ __launch_bounds__(BLD_NT) void build_impacts_kernel(const long long* __restrict__ term_ptr, const uint32_t* __restrict__ post_row,
                                                               const int32_t* __restrict__ post_tf, long long n_post,
                                                               const long long* __restrict__ doc_ptr, long long n_docs,
                                                               const double* __restrict__ idf, int vocab, double avgdl,
                                                               float* __restrict__ post_w) {
    const long long s = (long long)blockIdx.x * BLD_NT + threadIdx.x;
    if (s >= n_post) return;
    int lo = 0, hi = vocab - 1;                              // the last t in [0, vocab) with term_ptr[t] <= s
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (term_ptr[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const long long r = (long long)post_row[s];
    const double dl = r < n_docs ? (double)(doc_ptr[r + 1] - doc_ptr[r]) : 0.0;
    const double tf = (double)post_tf[s];
    const double bdl = BM25_B * dl;
    const double rel = bdl / avgdl;
    const double norm = BM25_K1 * ((1.0 - BM25_B) + rel);
    const double num = (idf[lo] * tf) * (BM25_K1 + 1.0);
    post_w[s] = (float)(num / (tf + norm));
}

int radix_passes(int vocab) {
    int bits = 0;
    while (bits < 32 && ((int64_t)1 << bits) < (int64_t)vocab) ++bits;      // bits(vocab - 1)
    return (bits + 7) / 8;
}

bool build_limits_ok(int64_t n_tokens, int64_t n_docs, int32_t vocab) {
    return n_tokens >= 0 && n_tokens < ((int64_t)1 << 31) && n_docs >= 0 && n_docs < ((int64_t)1 << 32) && vocab >= 1 && vocab <= (1 << 24);
}

}  // namespace

extern "C" int64_t arx_bm25_build_workspace_bytes(int64_t n_tokens, int64_t n_docs, int32_t vocab) {
    if (!build_limits_ok(n_tokens, n_docs, vocab)) return -1;
    return 4 * round_up64(4 * n_tokens, 256) + round_up64((int64_t)4 * 256 * BLD_MAX_BLOCKS, 256);
}

extern "C" int32_t arx_bm25_build_postings_tuned(const int32_t* pieces, int64_t n_tokens, const int64_t* doc_ptr, int64_t n_docs, int32_t vocab,
                                                 int64_t* term_ptr, uint32_t* post_row, int32_t* post_tf, int64_t* n_postings, int32_t* bad_id,
                                                 void* ws, int64_t ws_bytes, int32_t tile_tokens, int32_t max_blocks, void* stream) {
    ARX_REQUIRE(pieces && doc_ptr && term_ptr && post_row && post_tf && n_postings && bad_id, "null pointer argument");
    ARX_REQUIRE(n_tokens >= 0 && n_tokens < ((int64_t)1 << 31), "n_tokens=%lld must be in [0, 2^31)", (long long)n_tokens);
    ARX_REQUIRE(n_docs >= 0 && n_docs < ((int64_t)1 << 32), "n_docs=%lld must be in [0, 2^32)", (long long)n_docs);
    ARX_REQUIRE(vocab >= 1 && vocab <= (1 << 24), "vocab=%d must be in [1, 2^24]", vocab);
    ARX_REQUIRE(tile_tokens == 0 || (tile_tokens >= BLD_NT && tile_tokens <= BLD_TILE_MAX && tile_tokens % BLD_NT == 0),
                "tile_tokens=%d must be 0 or a multiple of %d in [%d, %d]", tile_tokens, BLD_NT, BLD_NT, BLD_TILE_MAX);
    ARX_REQUIRE(max_blocks >= 0 && max_blocks <= BLD_MAX_BLOCKS, "max_blocks=%d must be in [0, %d]", max_blocks, BLD_MAX_BLOCKS);
    const int64_t need = arx_bm25_build_workspace_bytes(n_tokens, n_docs, vocab);
    ARX_REQUIRE(ws && ws_bytes >= need, "workspace too small: %lld bytes given, %lld needed", (long long)(ws ? ws_bytes : 0), (long long)need);
    hipStream_t st = (hipStream_t)stream;
    ARX_HIP_CHECK(hipMemsetAsync(bad_id, 0, sizeof(int32_t), st));
    if (n_tokens == 0 || n_docs == 0) {
        ARX_HIP_CHECK(hipMemsetAsync(term_ptr, 0, sizeof(int64_t) * ((size_t)vocab + 1), st));
        ARX_HIP_CHECK(hipMemsetAsync(n_postings, 0, sizeof(int64_t), st));
        return ARX_OK;
    }
    const int64_t arr = round_up64(4 * n_tokens, 256);
    uint32_t* key[2] = {(uint32_t*)ws, (uint32_t*)((char*)ws + 2 * arr)};
    uint32_t* row[2] = {(uint32_t*)((char*)ws + arr), (uint32_t*)((char*)ws + 3 * arr)};
    uint32_t* hist = (uint32_t*)((char*)ws + 4 * arr);
    const int64_t tile = tile_tokens ? tile_tokens : BLD_TILE;
    const int64_t tiles = (n_tokens + tile - 1) / tile, cap = max_blocks ? max_blocks : BLD_MAX_BLOCKS;
    const int64_t per = (tiles + cap - 1) / cap;             // tiles of a block
    Chunks c;
    c.n = n_tokens; c.chunk = per * tile; c.blocks = (int)((tiles + per - 1) / per);
    const int token_blocks = cdiv(n_tokens, BLD_NT);
    build_init_kernel<<<token_blocks, BLD_NT, 0, st>>>(pieces, n_tokens, (const long long*)doc_ptr, n_docs, vocab, key[0], row[0], bad_id);
    int cur = 0;
    const int passes = radix_passes(vocab);
    for (int p = 0; p < passes; ++p, cur ^= 1) {
        build_hist_kernel<<<c.blocks, BLD_NT, 0, st>>>(key[cur], c, 8 * p, hist);
        build_scan_kernel<<<1, SCAN_NT, 0, st>>>(hist, 256 * c.blocks, nullptr);
        build_scatter_kernel<<<c.blocks, BLD_NT, 0, st>>>(key[cur], row[cur], c, 8 * p, hist, key[cur ^ 1], row[cur ^ 1]);
    }
    uint32_t *slot = key[cur ^ 1], *start = row[cur ^ 1];    // the other pair is free now
    build_head_count_kernel<<<c.blocks, BLD_NT, 0, st>>>(key[cur], row[cur], c, hist);
    build_scan_kernel<<<1, SCAN_NT, 0, st>>>(hist, c.blocks, (long long*)n_postings);
    build_head_slot_kernel<<<c.blocks, BLD_NT, 0, st>>>(key[cur], row[cur], c, hist, slot, start);
    build_emit_kernel<<<token_blocks, BLD_NT, 0, st>>>(row[cur], start, n_tokens, (const long long*)n_postings, post_row, post_tf);
    build_term_ptr_kernel<<<cdiv((int64_t)vocab + 1, BLD_NT), BLD_NT, 0, st>>>(key[cur], slot, n_tokens, (const long long*)n_postings, vocab,
                                                                                (long long*)term_ptr);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int32_t arx_bm25_build_postings(const int32_t* pieces, int64_t n_tokens, const int64_t* doc_ptr, int64_t n_docs, int32_t vocab,
                                           int64_t* term_ptr, uint32_t* post_row, int32_t* post_tf, int64_t* n_postings, int32_t* bad_id,
                                           void* ws, int64_t ws_bytes, void* stream) {
    return arx_bm25_build_postings_tuned(pieces, n_tokens, doc_ptr, n_docs, vocab, term_ptr, post_row, post_tf, n_postings, bad_id, ws, ws_bytes,
                                         0, 0, stream);
}

extern "C" int32_t arx_bm25_build_impacts(const int64_t* term_ptr, const uint32_t* post_row, const int32_t* post_tf, int64_t n_postings,
                                          const int64_t* doc_ptr, int64_t n_docs, const double* idf, int32_t vocab, double avgdl, float* post_w,
                                          void* stream) {
    ARX_REQUIRE(term_ptr && post_row && post_tf && doc_ptr && idf && post_w, "null pointer argument");
    ARX_REQUIRE(n_postings >= 0 && n_postings < ((int64_t)1 << 31), "n_postings=%lld must be in [0, 2^31)", (long long)n_postings);
    ARX_REQUIRE(n_docs >= 0 && n_docs < ((int64_t)1 << 32), "n_docs=%lld must be in [0, 2^32)", (long long)n_docs);
    ARX_REQUIRE(vocab >= 1 && vocab <= (1 << 24), "vocab=%d must be in [1, 2^24]", vocab);
    ARX_REQUIRE(avgdl >= 0.0, "avgdl=%g must not be negative", avgdl);      // (refuses nan too)
    if (n_postings == 0) return ARX_OK;
    build_impacts_kernel<<<cdiv(n_postings, BLD_NT), BLD_NT, 0, (hipStream_t)stream>>>((const long long*)term_ptr, post_row, post_tf, n_postings,
                                                                                     (const long long*)doc_ptr, n_docs, idf, vocab, avgdl, post_w);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
