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
//   scan    block (stretch p of rows_per_block rows, tile t of BIN_QT = 8 queries), four waves.  The tile's query words sit in LDS; a
//           round gives every lane one row (a wave's 64 rows are one contiguous span of the code array and one word of `allow`: a zero
//           word costs that one load), the lane reads its row's words once and keeps the eight distances in registers, so the code
//           array is read once per query tile.  Each query keeps a list of KEY_CAP keys in LDS (key_lists.h, shared with pq.hip): a
//           lane appends a key above the list's threshold, and the lists are cut back to their R largest by a block-wide sort before a
//           round that could overflow one, so the block's final list is the exact R largest keys of its stretch, sorted, whatever the
//           order of the appends.  -> part_k [parts][nq][R] (0 = none).
//   merge   key_lists.h's: one block per query over its parts * R keys, any number of them -> out_cand / out_dist / out_count.
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
constexpr int BIN_BLOCKS_TARGET = 1024;         // the default rows_per_block aims at this many scan blocks
constexpr int BIN_RPB_MIN_DEFAULT = 2048;
constexpr int BIN_RPB_LIMIT = 1 << 20;

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

// V: 64-bit words per load (2: a 16-byte load, W even; 1: any W)
template <int V>
__global__ __launch_bounds__(BIN_NT) void binary_scan_kernel(const uint64_t* __restrict__ codes, int64_t n_rows, int W,
                                                             const uint64_t* __restrict__ qcodes, int nq, const uint64_t* __restrict__ allow,
                                                             int R, int64_t rpb, unsigned long long* __restrict__ part_k) {
    __shared__ KeyLists<BIN_QT> sm;
    __shared__ __attribute__((aligned(16))) uint64_t qs[BIN_W_MAX][BIN_QT];              // word-major: a word's eight query words are adjacent
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = blockIdx.y * BIN_QT;
    const int nl = nq - q0 < BIN_QT ? nq - q0 : BIN_QT;       // the tile's queries
    for (int t = tid; t < W * BIN_QT; t += BIN_NT) {
        const int l = t % BIN_QT, ww = t / BIN_QT;
        qs[ww][l] = l < nl ? qcodes[(int64_t)(q0 + l) * W + ww] : 0ull;
    }
    if (tid < BIN_QT) { sm.cnt[tid] = 0; sm.thr[tid] = 0ull; }
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * rpb;             // a multiple of 64
    const int64_t hi = lo + rpb < n_rows ? lo + rpb : n_rows;
    for (int64_t base = lo; base < hi; base += BIN_NT) {      // block-uniform
        const unsigned full = key_full_mask(sm, nl);
        __syncthreads();                                       // everyone has read cnt before anyone appends or cuts
        if (full) key_cut(sm, full, R);
        const int64_t r0 = base + (int64_t)w * 64;             // the wave's 64 rows: one word of allow
        uint64_t vis = 0ull;
        if (r0 < hi) {
            const int64_t left = hi - r0;
            vis = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
            if (allow) vis &= allow[r0 >> 6];
        }
        if (vis != 0ull) {                                     // wave-uniform
            const int64_t row = r0 + lane;
            const bool on = (vis >> lane) & 1ull;
            const uint64_t* c = codes + (on ? row : r0) * W;   // (a lane without a row reads the wave's first row: inside the array)
            int d[BIN_QT];
#pragma unroll
            for (int l = 0; l < BIN_QT; ++l) d[l] = 0;
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
                    for (int l = 0; l < BIN_QT; ++l) d[l] += __popcll(x[e] ^ qs[ww + e][l]);
            }
            if (on) {
                const unsigned long long low = (unsigned long long)(0xffffffffu - (uint32_t)row);
#pragma unroll
                for (int l = 0; l < BIN_QT; ++l)
                    if (l < nl) key_append(sm, l, ((unsigned long long)(0x7fffffffu - (uint32_t)d[l]) << 32) | low);
            }
        }
        __syncthreads();
    }
    key_cut(sm, (1u << nl) - 1u, R);
    for (int t = tid; t < nl * R; t += BIN_NT) {
        const int l = t / R, r = t % R;
        part_k[((int64_t)blockIdx.x * nq + q0 + l) * R + r] = r < sm.cnt[l] ? sm.keys[l][r] : 0ull;
    }
}

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
    ARX_REQUIRE(rows_per_block == 0 || (rows_per_block >= 64 && rows_per_block % 64 == 0 && rows_per_block <= BIN_RPB_LIMIT),
                "rows_per_block=%d: 0 (default) or a multiple of 64 in 64..%d", rows_per_block, BIN_RPB_LIMIT);
    ARX_REQUIRE(qcodes && out_cand && out_count && ws && (codes || n_rows == 0), "null pointer argument");
    ARX_REQUIRE(((uintptr_t)codes | (uintptr_t)ws) % 16 == 0, "codes and ws must be 16-byte aligned");
    ARX_REQUIRE(((uintptr_t)qcodes | (uintptr_t)allow | (uintptr_t)out_count) % 8 == 0, "qcodes, allow and out_count must be 8-byte aligned");
    ARX_REQUIRE(((uintptr_t)out_cand | (uintptr_t)out_dist) % 4 == 0, "out_cand and out_dist must be 4-byte aligned");
    const KeyWs L = key_layout(n_rows, n_queries, R);
    ARX_REQUIRE(ws_bytes >= L.total, "workspace too small: %lld < %lld (arx_binary_workspace_bytes)", (long long)ws_bytes, (long long)L.total);
    hipStream_t st = (hipStream_t)stream;
    const int W = dim / 64;
    unsigned long long* part_k = (unsigned long long*)ws;
    for (int q0 = 0; q0 < n_queries; q0 += KEY_QBATCH) {
        const int nq = (n_queries - q0) < KEY_QBATCH ? (n_queries - q0) : KEY_QBATCH;
        const int tiles = (nq + BIN_QT - 1) / BIN_QT;
        int64_t rpb = rows_per_block;
        if (rpb == 0) {
            const int64_t want = BIN_BLOCKS_TARGET / tiles > 0 ? BIN_BLOCKS_TARGET / tiles : 1;
            rpb = round_up64((n_rows + want - 1) / want, 256);
            if (rpb < BIN_RPB_MIN_DEFAULT) rpb = BIN_RPB_MIN_DEFAULT;
        }
        const int64_t max_parts = L.slots / nq;                 // >= 1: the partial lists the workspace holds per query
        if ((n_rows + rpb - 1) / rpb > max_parts) rpb = round_up64((n_rows + max_parts - 1) / max_parts, 64);
        const int64_t parts = (n_rows + rpb - 1) / rpb > 0 ? (n_rows + rpb - 1) / rpb : 1;
        ARX_REQUIRE(parts <= max_parts && parts < (1ll << 31), "grid too large");
        const dim3 grid((unsigned)parts, (unsigned)tiles);
        const uint64_t* Q = qcodes + (int64_t)q0 * W;
        if (W % 2 == 0) binary_scan_kernel<2><<<grid, BIN_NT, 0, st>>>(codes, n_rows, W, Q, nq, allow, R, rpb, part_k);
        else binary_scan_kernel<1><<<grid, BIN_NT, 0, st>>>(codes, n_rows, W, Q, nq, allow, R, rpb, part_k);
        ARX_HIP_CHECK(hipGetLastError());
        key_merge_kernel<false><<<nq, BIN_NT, 0, st>>>(part_k, parts, nq, R, out_cand + (int64_t)q0 * R,
                                                   out_dist ? out_dist + (int64_t)q0 * R : nullptr, out_count + q0);
        ARX_HIP_CHECK(hipGetLastError());
    }
    return ARX_OK;
}

extern "C" int32_t arx_binary_candidates(const uint64_t* codes, int64_t n_rows, int32_t dim, const uint64_t* qcodes, int32_t n_queries,
                                         const uint64_t* allow, int32_t n_candidates, int32_t* out_cand, int32_t* out_dist, int64_t* out_count,
                                         void* ws, int64_t ws_bytes, void* stream) {
    return arx_binary_candidates_tuned(codes, n_rows, dim, qcodes, n_queries, allow, n_candidates, out_cand, out_dist, out_count, ws, ws_bytes, 0,
                                       stream);
}
