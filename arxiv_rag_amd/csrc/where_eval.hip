// arx_where_eval: Chroma `where` filters evaluated over HBM-resident metadata columns (C ABI in include/arx.h; the lowering that writes
// the programs is arxiv_rag_amd/where_device.py).  The producer of the row bitmaps arx_topk_search_filtered(_multi) consumes.
//
// One launch fills the bitmaps of all filters of the call: grid (word tiles, filters), a wave owns one 64-row word of one filter and a lane
// one row.  The filter is blockIdx.y, so the whole program (tokens, leaf descriptors, column addresses, the operands of short sets) is
// wave-uniform and read through uniform loads out of read-only memory; per lane there are only kind[r] (1 B) and val[r] (8 B) of each leaf's
// column, both coalesced (64 B + 512 B per wave and leaf), and the binary search of a long `$in` set.  Every comparison is in f64.
//
// The postfix program folds on a bit stack in ONE 32-bit register per lane (bit 0 = top of the stack; depth <= 32 is the lowering's
// contract).  The lane's result goes through __ballot into the 64-bit word, rows at or beyond n_rows are cleared, the `and_with` word is
// and-ed in and lane 0 stores it with a plain vector store: every word is written exactly once, nothing is zero-filled, no atomics.  A
// second launch with one block per filter counts the bits.
//
// A damaged program reads nothing out of range: leaf, column and set indices are clamped to what the call declares, the stack is a register.
#include "arx_common.h"

namespace {
constexpr int WE_NT = 256, WE_WAVES = WE_NT / 64;
constexpr int WE_MAX_FILTERS = 64;
constexpr int WE_LINEAR_SET = 8;                              // sets up to this long are scanned with uniform loads, longer ones searched per lane
enum { WE_EQ = 0, WE_GT = 1, WE_GE = 2, WE_LT = 3, WE_LE = 4, WE_IN = 5, WE_NEVER = 6 };
enum { WE_LEAF = 0, WE_AND = 1, WE_OR = 2 };

// x in s[0, len) (ascending, distinct, no NaN), by value: -0.0 finds 0.0, a NaN finds nothing
__device__ __forceinline__ bool we_in_set(const double* __restrict__ s, int len, double x) {
    if (len <= 0) return false;
    if (len <= WE_LINEAR_SET) {
        bool hit = false;
        for (int j = 0; j < len; ++j) hit = hit || (s[j] == x);        // (j and s are uniform: the operands arrive as scalars)
        return hit;
    }
    int base = 0;
    for (int n = len; n > 1;) {                               // branch-free lower bound: n is uniform, only `base` differs between lanes
        const int half = n >> 1;
        base = (s[base + half - 1] < x) ? base + half : base;
        n -= half;
    }
    const int idx = base + ((s[base] < x) ? 1 : 0);
    return idx < len && s[idx] == x;
}

__global__ __launch_bounds__(WE_NT) void where_eval_kernel(const long long* __restrict__ col_table, int n_cols, int64_t n_rows, int64_t n_words,
                                                           const arx_where_leaf* __restrict__ leaves, const int32_t* __restrict__ leaf_off,
                                                           const int32_t* __restrict__ tokens, const int32_t* __restrict__ token_off,
                                                           const double* __restrict__ set_vals, int64_t n_set_vals,
                                                           const unsigned long long* __restrict__ and_with, int64_t and_stride,
                                                           unsigned long long* __restrict__ out_bits) {
    const int f = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * WE_WAVES + wave;
    if (word >= n_words) return;                              // (wave-uniform)
    const int64_t row = word * 64 + lane;
    const bool live = row < n_rows;
    const int64_t r = live ? row : n_rows - 1;                // the last word's spare lanes read the last row; their bits are cleared below
    const int l0 = leaf_off[f], n_leaf = leaf_off[f + 1] - l0;
    const int t0 = token_off[f], t1 = token_off[f + 1];
    uint32_t stack = 0;
    for (int t = t0; t < t1; ++t) {
        const int tok = tokens[t];
        const int code = tok & 3, arg = tok >> 2;
        if (code == WE_LEAF) {
            bool b = false;
            if (n_leaf > 0) {
                const int li = arg < 0 ? 0 : (arg >= n_leaf ? n_leaf - 1 : arg);
                const arx_where_leaf L = leaves[l0 + li];
                const int c = L.column < 0 ? 0 : (L.column >= n_cols ? n_cols - 1 : L.column);
                const uint8_t* __restrict__ kind = (const uint8_t*)col_table[2 * c];
                const double* __restrict__ val = (const double*)col_table[2 * c + 1];
                const int k = kind[r];
                const double v = val[r], x = L.operand;
                bool hit = false;
                switch (L.op) {                               // (uniform)
                    case WE_EQ: hit = v == x; break;
                    case WE_GT: hit = v > x; break;
                    case WE_GE: hit = v >= x; break;
                    case WE_LT: hit = v < x; break;
                    case WE_LE: hit = v <= x; break;
                    case WE_IN: {
                        const int64_t so = L.set_off < 0 ? 0 : (L.set_off > n_set_vals ? n_set_vals : (int64_t)L.set_off);
                        const int64_t room = n_set_vals - so;
                        const int sl = L.set_len < 0 ? 0 : (L.set_len > room ? (int)room : L.set_len);
                        hit = we_in_set(set_vals + so, sl, v);
                        break;
                    }
                    default: break;                           // WE_NEVER, or an op this build does not know
                }
                b = ((k == L.want_kind) && hit) != (L.negate != 0);
            }
            stack = (stack << 1) | (b ? 1u : 0u);
        } else {
            const int n = arg < 1 ? 1 : (arg > 32 ? 32 : arg);
            const uint32_t mask = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
            const uint32_t top = stack & mask;
            const bool res = code == WE_AND ? top == mask : top != 0u;
            stack = n >= 32 ? 0u : (stack >> n);
            stack = (stack << 1) | (res ? 1u : 0u);
        }
    }
    unsigned long long w = __ballot((live && (stack & 1u)) ? 1 : 0);
    if (and_with) w &= and_with[(int64_t)f * and_stride + word];
    if (lane == 0) out_bits[(int64_t)f * n_words + word] = w;
}

// one block per filter: the count is a plain store of one block's sum (the bits at or beyond n_rows were written as 0 by the kernel above)
__global__ __launch_bounds__(1024) void where_count_kernel(const unsigned long long* __restrict__ bits, int64_t n_words, long long* __restrict__ out) {
    __shared__ long long s_part[16];
    const unsigned long long* mine = bits + (int64_t)blockIdx.x * n_words;
    long long c = 0;
    for (int64_t i = threadIdx.x; i < n_words; i += 1024) c += __popcll(mine[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int i = 0; i < 16; ++i) t += s_part[i];
        out[blockIdx.x] = t;
    }
}
}      // namespace

extern "C" int32_t arx_where_eval(const int64_t* col_table, int32_t n_cols, int64_t n_rows, const arx_where_leaf* leaves, const int32_t* leaf_off,
                                  const int32_t* tokens, const int32_t* token_off, const double* set_vals, int64_t n_set_vals, int32_t n_filters,
                                  const uint64_t* and_with, int64_t and_stride, uint64_t* out_bits, int64_t* out_counts, void* stream) {
    static_assert(sizeof(arx_where_leaf) == 32, "arx_where_leaf is 32 bytes (include/arx.h, where_device.LEAF_DTYPE)");
    ARX_REQUIRE(n_filters >= 1 && n_filters <= WE_MAX_FILTERS, "n_filters=%d out of range 1..%d", n_filters, WE_MAX_FILTERS);
    ARX_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 36), "n_rows=%lld must be in 1..2^36-1", (long long)n_rows);
    ARX_REQUIRE(n_cols >= 1, "n_cols=%d must be at least 1", n_cols);
    ARX_REQUIRE(n_set_vals >= 0 && n_set_vals <= ((int64_t)1 << 20), "n_set_vals=%lld out of range 0..2^20", (long long)n_set_vals);
    ARX_REQUIRE(and_stride >= 0, "and_stride=%lld must not be negative", (long long)and_stride);
    ARX_REQUIRE(col_table, "null pointer argument: col_table");
    ARX_REQUIRE(leaves, "null pointer argument: leaves");
    ARX_REQUIRE(leaf_off, "null pointer argument: leaf_off");
    ARX_REQUIRE(tokens, "null pointer argument: tokens");
    ARX_REQUIRE(token_off, "null pointer argument: token_off");
    ARX_REQUIRE(set_vals || n_set_vals == 0, "null pointer argument: set_vals (n_set_vals=%lld)", (long long)n_set_vals);
    ARX_REQUIRE(out_bits, "null pointer argument: out_bits");
    ARX_REQUIRE(out_counts, "null pointer argument: out_counts");
    const int64_t n_words = (n_rows + 63) >> 6;
    const dim3 grid((unsigned)((n_words + WE_WAVES - 1) / WE_WAVES), (unsigned)n_filters);
    where_eval_kernel<<<grid, WE_NT, 0, (hipStream_t)stream>>>((const long long*)col_table, n_cols, n_rows, n_words, leaves, leaf_off, tokens, token_off,
                                                               set_vals, n_set_vals, (const unsigned long long*)and_with, and_stride,
                                                               (unsigned long long*)out_bits);
    ARX_HIP_CHECK(hipGetLastError());
    where_count_kernel<<<(unsigned)n_filters, 1024, 0, (hipStream_t)stream>>>((const unsigned long long*)out_bits, n_words, (long long*)out_counts);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
}
