// arx_binary_pack / arx_binary_candidates: sign-bit codes of the rows and the exact Hamming candidate lists over them (gfx950; C ABI in
// include/arx.h; the host layer is arxiv_rag_amd/binary.py; the definition is INTEGRATION.md "Binary-code search").
//
// A code is one bit per dimension: bit j & 63 of word j >> 6 is set iff (float)x[j] > centre[j] (strict, f32; NaN -> 0), the bit
// convention of the row bitmaps.  d(q, r) = sum_w popcount(codes[r][w] ^ qcodes[q][w]) is an integer, so the candidate set is defined
// exactly: C(q) = the first min(R, visible) visible rows by (d asc, row asc).  Everything here is integer work; the exact rescore of
// C(q) is arx_ivf_search over the candidate lists (the header says how the two calls compose).
//   pack    a wave packs 64 consecutive words: step i reads the 64 halves of word g0 + i coalesced (a row's words and the rows are
//           contiguous, so word g covers the flat elements [64 g, 64 g + 64)), one ballot gives the word, lane i keeps it; one coalesced
//           8-byte store per lane.  Every word is written once, no atomics.
//   keys    (0x7fffffff - d) << 32 | (0xffffffff - row): larger is better, distinct for distinct rows, never 0 (0 = an empty slot).
//   scan    key_lists.h's key_scan_kernel (shared with pq.hip) over tiles of BIN_QT = 8 queries.  The tile's query words sit in LDS,
//           word-major; a lane reads its row's words once and keeps the eight distances in registers.  The merge is key_lists.h's too.
// No float work at all, no global atomics.  A query's outputs are the R largest of a set of distinct integer keys: they depend on its
// qcodes row, codes and allow alone, not on the batch, the tile or rows_per_block.  codes, qcodes and allow are device data of which
// every bit pattern is a legal value; bits of allow at or beyond n_rows are masked off before use.
#include "arx_common.h"
#include "key_lists.h"

namespace {
constexpr int BIN_NT = KEY_NT, BIN_NW = BIN_NT / 64;
constexpr int BIN_QT = 8;                       // queries of a tile
constexpr int BIN_R_MAX = KEY_R_MAX;
constexpr int BIN_W_MAX = 128;                  // dim 8192

__global__ __launch_bounds__(BIN_NT) void binary_pack_kernel(const f16_t* __restrict__ x, int64_t n_words, int W,
                                                             const float* __restrict__ centre, uint64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t g0 = ((int64_t)blockIdx.x * BIN_NW + (threadIdx.x >> 6)) * 64;      // wave-uniform
    uint64_t mine = 0ull;
    for (int i = 0; i < 64; ++i) {
        const int64_t g = g0 + i;
        if (g >= n_words) break;                               // wave-uniform
        const float v = (float)x[g * 64 + lane];
        const float c = centre ? centre[(g % W) * 64 + lane] : 0.f;
        const uint64_t b = __ballot(v > c);                    // false for NaN on either side
        mine = lane == i ? b : mine;
    }
    if (g0 + lane < n_words) out[g0 + lane] = mine;
}

// The sign-bit code as key_scan_kernel sees it.  V: 64-bit words per load (2: a 16-byte load, W even; 1: any W)
template <int V>
struct BinaryCode {
    using Word = uint64_t;
    static constexpr int QT = BIN_QT;
    const uint64_t* codes; int W; const uint64_t* qcodes;       // [n_rows][W]; the slice's [nq][W]
    struct Lds { KeyLists<BIN_QT>& lists; uint64_t (&qs)[BIN_W_MAX][BIN_QT]; };
    __device__ __forceinline__ Lds lds() const {
        __shared__ KeyLists<BIN_QT> sm;
        __shared__ __attribute__((aligned(16))) uint64_t qs[BIN_W_MAX][BIN_QT];          // word-major: a word's eight query words are adjacent
        return {sm, qs};
    }
    __device__ __forceinline__ void stage(const Lds s, int q0, int nl) const {
        for (int t = threadIdx.x; t < W * BIN_QT; t += BIN_NT) {
            const int l = t % BIN_QT, ww = t / BIN_QT;
            s.qs[ww][l] = l < nl ? qcodes[(int64_t)(q0 + l) * W + ww] : 0ull;
        }
    }
    __device__ __forceinline__ void high_words(const Lds s, int64_t row, uint32_t (&h)[BIN_QT]) const {
        const uint64_t* c = codes + row * W;
        int d[BIN_QT] = {};                                                               // the distances, in registers
        for (int ww = 0; ww < W; ww += V) {
            uint64_t x[V];
            if constexpr (V == 2) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(c + ww);
                x[0] = v.x; x[1] = v.y;
            } else {
                x[0] = c[ww];
            }
#pragma unroll
            for (int e = 0; e < V; ++e)
#pragma unroll
                for (int l = 0; l < BIN_QT; ++l) d[l] += __popcll(x[e] ^ s.qs[ww + e][l]);
        }
#pragma unroll
        for (int l = 0; l < BIN_QT; ++l) h[l] = 0x7fffffffu - (uint32_t)d[l];
    }
};

struct BinaryScan {                                            // the host side of the code, for key_scan
    static constexpr bool HI_DIRECT = false;                   // out_dist is the distance, 0x7fffffff - the high word
    static constexpr const char* WORKSPACE_FN = "arx_binary_workspace_bytes";
    const uint64_t *codes, *qcodes; int W;
    int tile() const { return BIN_QT; }
    int32_t launch(const KeyScanArgs& a, int q0) const {
        const uint64_t* Q = qcodes + (int64_t)q0 * W;
        return W % 2 == 0 ? key_scan_launch<BinaryCode<2>>(a, codes, W, Q, 0) : key_scan_launch<BinaryCode<1>>(a, codes, W, Q, 0);
    }
};

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
bool bin_dim_ok(int32_t dim) { return dim >= 64 && dim % 64 == 0 && dim <= 64 * BIN_W_MAX; }
bool bin_shape_ok(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t R) {
    return n_rows >= 0 && n_rows < (1ll << 31) && n_queries >= 1 && bin_dim_ok(dim) && R >= 1 && R <= BIN_R_MAX;
}
}      // namespace

extern "C" int32_t arx_binary_pack(const void* rows, int64_t n_rows, int32_t dim, const float* centre, uint64_t* out_codes, void* stream) {
    ARX_REQUIRE(bin_dim_ok(dim), "dim=%d must be a multiple of 64 in 64..%d", dim, 64 * BIN_W_MAX);
    ARX_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "n_rows=%lld out of range 0..2^31-1", (long long)n_rows);
    if (n_rows == 0) return ARX_OK;
    ARX_REQUIRE(rows && out_codes, "null pointer argument");
    ARX_REQUIRE((uintptr_t)rows % 2 == 0 && (uintptr_t)out_codes % 8 == 0 && (uintptr_t)centre % 4 == 0,
                "rows must be 2-byte, centre 4-byte and out_codes 8-byte aligned");
    const int W = dim / 64;
    const int64_t n_words = n_rows * W;                        // < 2^38
    binary_pack_kernel<<<(unsigned)((n_words + BIN_NT - 1) / BIN_NT), BIN_NT, 0, (hipStream_t)stream>>>((const f16_t*)rows, n_words, W, centre,
                                                                                                       out_codes);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}

extern "C" int64_t arx_binary_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t dim, int32_t n_candidates) {
    if (!bin_shape_ok(n_rows, n_queries, dim, n_candidates)) return -1;
    return key_layout(n_rows, n_queries, n_candidates).total;
}

extern "C" int32_t arx_binary_candidates_tuned(const uint64_t* codes, int64_t n_rows, int32_t dim, const uint64_t* qcodes, int32_t n_queries,
                                               const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_dist,
                                               int64_t* out_count, void* ws, int64_t ws_bytes, int32_t rows_per_block, void* stream) {
    const int R = n_candidates;
    ARX_REQUIRE(R >= 1 && R <= BIN_R_MAX, "n_candidates=%d out of range 1..%d", R, BIN_R_MAX);
    ARX_REQUIRE(bin_dim_ok(dim), "dim=%d must be a multiple of 64 in 64..%d", dim, 64 * BIN_W_MAX);
    ARX_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "n_rows=%lld out of range 0..2^31-1", (long long)n_rows);
    ARX_REQUIRE(n_queries >= 1, "n_queries=%d: empty query set", n_queries);
    KEY_REQUIRE_ROWS_PER_BLOCK(rows_per_block);
    ARX_REQUIRE(qcodes && out_cand && out_count && ws && (codes || n_rows == 0), "null pointer argument");
    ARX_REQUIRE(((uintptr_t)codes | (uintptr_t)ws) % 16 == 0, "codes and ws must be 16-byte aligned");
    ARX_REQUIRE(((uintptr_t)qcodes | (uintptr_t)allow | (uintptr_t)out_count) % 8 == 0, "qcodes, allow and out_count must be 8-byte aligned");
    ARX_REQUIRE(((uintptr_t)out_cand | (uintptr_t)out_dist) % 4 == 0, "out_cand and out_dist must be 4-byte aligned");
    return key_scan(BinaryScan{codes, qcodes, dim / 64}, n_rows, n_queries, allow, R, rows_per_block, ws, ws_bytes, out_cand, out_dist, out_count,
                    (hipStream_t)stream);
}

extern "C" int32_t arx_binary_candidates(const uint64_t* codes, int64_t n_rows, int32_t dim, const uint64_t* qcodes, int32_t n_queries,
                                         const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_dist, int64_t* out_count,
                                         void* ws, int64_t ws_bytes, void* stream) {
    return arx_binary_candidates_tuned(codes, n_rows, dim, qcodes, n_queries, allow, n_candidates, out_cand, out_dist, out_count, ws, ws_bytes, 0,
                                       stream);
}
