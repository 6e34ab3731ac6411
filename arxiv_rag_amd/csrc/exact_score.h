// exact_row_score: the one definition of a (row, query) score that the exact searches (search_tail.h, masked_topk.h) and the k-means
// assign (cluster_assign.hip) rank by.  Needs arx_common.h (f16_t, f16x8) before it.
#pragma once

// exact score of corpus row `row` against the query row staged in LDS: 8 lanes per row (l8 = lane & 7), two FMA chains per
// lane over its 16-B chunks, then a 3-step butterfly -> every lane of the octet holds the sum.  The ONE definition of a score
// in this file: pass B2 and the certificate's fallback both rank by it.
__device__ __forceinline__ float exact_row_score(const f16_t* __restrict__ crow, const f16_t* qs, int nch, int l8, bool ok) {
    float a0 = 0.f, a1 = 0.f;
    // chunks l8, l8 + 8, ... in ascending order, whatever the batching below: the sum's order (hence its bits) is fixed; the batches
    // only decide how many of the row's 16-B loads are in flight at once (six: a 768-d row is two dependent round trips instead of three)
    auto fma8 = [&](const f16x8& cv, const f16x8& qq) {
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            a0 = fmaf((float)cv[e], (float)qq[e], a0);
            a1 = fmaf((float)cv[e + 1], (float)qq[e + 1], a1);
        }
    };
    if (ok) {
        int ch = l8;
#pragma unroll 1
        for (; ch + 40 < nch; ch += 48) {
            f16x8 cv[6];
#pragma unroll
            for (int u = 0; u < 6; ++u) cv[u] = *reinterpret_cast<const f16x8*>(crow + (ch + 8 * u) * 8);
#pragma unroll
            for (int u = 0; u < 6; ++u) fma8(cv[u], *reinterpret_cast<const f16x8*>(qs + (ch + 8 * u) * 8));
        }
#pragma unroll 1
        for (; ch + 8 < nch; ch += 16) {
            f16x8 cv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) cv[u] = *reinterpret_cast<const f16x8*>(crow + (ch + 8 * u) * 8);
#pragma unroll
            for (int u = 0; u < 2; ++u) fma8(cv[u], *reinterpret_cast<const f16x8*>(qs + (ch + 8 * u) * 8));
        }
        for (; ch < nch; ch += 8) fma8(*reinterpret_cast<const f16x8*>(crow + ch * 8), *reinterpret_cast<const f16x8*>(qs + ch * 8));
    }
    float a = a0 + a1;
    a += __shfl_xor(a, 4); a += __shfl_xor(a, 2); a += __shfl_xor(a, 1);
    return a;
}
