// Exact "R largest 64-bit keys" lists in LDS and the candidate scan over them, written once for binary.hip (Hamming distances over sign
// bits) and pq.hip (byte-table sums over product-quantiser codes).  A key is  high word << 32 | (0xffffffff - row):  larger is better, distinct
// for distinct rows, never 0 (0 = an empty slot; rows are below 2^31).  What the high word means is the caller's business.
//   KeyLists   NL lists of KEY_CAP keys, each with an integer slot counter and a threshold (0 until the list has been cut once;
//              afterwards its R-th largest key).
//   key_append a lane appends a key above the list's threshold through the slot counter (an integer LDS atomic).
//   key_cut    before a round of at most KEY_NT appends per list that could overflow a list, the lists that could are cut back to their
//              R largest by a block-wide bitonic sort (bm25.hip's, over all those lists in the same stages).  A key at or below the R-th
//              largest of keys already seen is not among the R largest of all, so a list cut at the end holds the exact R largest keys
//              of everything offered to it, sorted, whatever the order of the appends.
//   key_scan_kernel  block (stretch p of rows_per_block rows, tile t of Code::QT queries), four waves, the tile's query-side data in LDS.
//              A round gives every lane one row (a wave's 64 rows: one contiguous span of the code array and one word of `allow`), read
//              once per query tile; its QT high words stay in registers.  The block's final lists -> part_k [parts][nq][R] (0 = none).
//   key_merge_kernel  one block per query over its parts * R keys of partial lists, any number of them, through the same list and cut
//              -> out_cand (the rows), out_hi (the high word, or 0x7fffffff - it) and out_count.
//   key_scan   the host driver of a call: slices of KEY_QBATCH queries, each one scan launch (none over an empty shard) and one merge.
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

// The scan.  `Code` is what differs between the codes.  The kernel builds it as Code{codes, width, qdata}, so that the pointers stay
// its own __restrict__ arguments: a Code declares exactly these three members first, in this order, both arrays of one element type.
//   Word, QT                  that element type; queries of a tile (compile time)
//   lds()                     the block's LDS as a handle, `.lists` (KeyLists<QT>&) and the Code's query-side storage; it goes on by value
//                             (by reference its fields are reloaded after every LDS store until inlining, and the loops differ)
//   stage(lds, q0, nl)        the whole block brings the data of queries q0 .. q0 + nl - 1 into that storage (zeros for l >= nl)
//   high_words(lds, row, h)   a lane reads the code of `row` and writes the QT high words of its keys (larger is better)
template <typename Code>
__global__ __launch_bounds__(KEY_NT) void key_scan_kernel(const typename Code::Word* __restrict__ codes, int64_t n_rows, int width,
                                                          const typename Code::Word* __restrict__ qdata, int nq, const uint64_t* __restrict__ allow,
                                                          int R, int64_t rpb, unsigned long long* __restrict__ part_k) {
    constexpr int QT = Code::QT;
    const Code code{codes, width, qdata};
    const auto lds = code.lds();
    KeyLists<QT>& sm = lds.lists;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = blockIdx.y * QT;
    const int nl = nq - q0 < QT ? nq - q0 : QT;               // the tile's queries
    code.stage(lds, q0, nl);
    if (tid < QT) { sm.cnt[tid] = 0; sm.thr[tid] = 0ull; }
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * rpb;             // a multiple of 64
    const int64_t hi = lo + rpb < n_rows ? lo + rpb : n_rows;
    for (int64_t base = lo; base < hi; base += KEY_NT) {      // block-uniform
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
            uint32_t h[QT];
            code.high_words(lds, on ? row : r0, h);            // (a lane without a row reads the wave's first row: inside the array)
            if (on) {
                const unsigned long long low = (unsigned long long)(0xffffffffu - (uint32_t)row);
#pragma unroll
                for (int l = 0; l < QT; ++l)
                    if (l < nl) key_append(sm, l, ((unsigned long long)h[l] << 32) | low);
            }
        }
        __syncthreads();
    }
    key_cut(sm, (1u << nl) - 1u, R);
    for (int t = tid; t < nl * R; t += KEY_NT) {
        const int l = t / R, r = t % R;
        part_k[((int64_t)blockIdx.x * nq + q0 + l) * R + r] = r < sm.cnt[l] ? sm.keys[l][r] : 0ull;
    }
}

struct KeyScanArgs { dim3 grid; hipStream_t st; int64_t n_rows; int nq; const uint64_t* allow; int R; int64_t rpb; unsigned long long* part_k; };
template <typename Code>
int32_t key_scan_launch(const KeyScanArgs& a, const typename Code::Word* codes, int width, const typename Code::Word* qdata, int smem) {
    if (smem > 0) ARX_HIP_CHECK(arx_func_smem((const void*)key_scan_kernel<Code>, smem));   // the Code's dynamic LDS (0: its LDS is static)
    key_scan_kernel<Code><<<a.grid, KEY_NT, smem, a.st>>>(codes, a.n_rows, width, qdata, a.nq, a.allow, a.R, a.rpb, a.part_k);
    ARX_HIP_CHECK(hipGetLastError());
    return ARX_OK;
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

constexpr int KEY_BLOCKS_TARGET = 1024, KEY_RPB_MIN_DEFAULT = 2048, KEY_RPB_LIMIT = 1 << 20;   // the default rows_per_block aims at that many scan blocks
#define KEY_REQUIRE_ROWS_PER_BLOCK(rpb)                                                                                      \
    ARX_REQUIRE((rpb) == 0 || ((rpb) >= 64 && (rpb) % 64 == 0 && (rpb) <= KEY_RPB_LIMIT),                                    \
                "rows_per_block=%d: 0 (default) or a multiple of 64 in 64..%d", rpb, KEY_RPB_LIMIT)

// The driver of a call, n_queries >= 1, after the caller's own argument checks (KEY_REQUIRE_ROWS_PER_BLOCK among them).  `Scan` is the
// host side of a code: HI_DIRECT (key_merge_kernel's), WORKSPACE_FN (the name the size refusal gives), tile() (the QT its kernels run) and
// launch(args, q0), which picks the instantiation and launches it for the slice of queries q0 .. q0 + args.nq - 1.
template <typename Scan>
int32_t key_scan(const Scan& scan, int64_t n_rows, int n_queries, const uint64_t* allow, int R, int rows_per_block, void* ws, int64_t ws_bytes,
                 int32_t* out_cand, int32_t* out_hi, int64_t* out_count, hipStream_t st) {
    const KeyWs L = key_layout(n_rows, n_queries, R);
    ARX_REQUIRE(ws_bytes >= L.total, "workspace too small: %lld < %lld (%s)", (long long)ws_bytes, (long long)L.total, Scan::WORKSPACE_FN);
    unsigned long long* part_k = (unsigned long long*)ws;
    for (int q0 = 0; q0 < n_queries; q0 += KEY_QBATCH) {
        const int nq = (n_queries - q0) < KEY_QBATCH ? (n_queries - q0) : KEY_QBATCH;
        const int tiles = (nq + scan.tile() - 1) / scan.tile();
        int64_t parts = 0;                                     // an empty shard launches no scan: the merge of no parts writes -1 and 0
        if (n_rows > 0) {
            int64_t rpb = rows_per_block;
            if (rpb == 0) {
                const int64_t want = KEY_BLOCKS_TARGET / tiles > 0 ? KEY_BLOCKS_TARGET / tiles : 1;
                rpb = round_up64((n_rows + want - 1) / want, 256);
                if (rpb < KEY_RPB_MIN_DEFAULT) rpb = KEY_RPB_MIN_DEFAULT;
            }
            const int64_t max_parts = L.slots / nq;             // >= 1: the partial lists the workspace holds per query
            if ((n_rows + rpb - 1) / rpb > max_parts) rpb = round_up64((n_rows + max_parts - 1) / max_parts, 64);
            parts = (n_rows + rpb - 1) / rpb;
            ARX_REQUIRE(parts <= max_parts && parts < (1ll << 31), "grid too large");
            const int32_t rc = scan.launch(KeyScanArgs{dim3((unsigned)parts, (unsigned)tiles), st, n_rows, nq, allow, R, rpb, part_k}, q0);
            if (rc != ARX_OK) return rc;
        }
        key_merge_kernel<Scan::HI_DIRECT><<<nq, KEY_NT, 0, st>>>(part_k, parts, nq, R, out_cand + (int64_t)q0 * R,
                                                                 out_hi ? out_hi + (int64_t)q0 * R : nullptr, out_count + q0);
        ARX_HIP_CHECK(hipGetLastError());
    }
    return ARX_OK;
}
}      // namespace
