// sorted_lists.h -- "sort (key, value) pairs, then find where each key's list starts": what aiap.hip, hashgrid.hip and
// knn.hip share of it (internal).  The sort itself is radix_sort.hip's stable LSD sort (launch_sort_pairs, common.h).
#pragma once
#include "common.h"

// The pair sort's buffers.  The sort ping-pongs between (k0, v0) and (k1, v1), one hop per pass of 8 key bits.
struct PairSort {
    uint32_t *k0, *v0, *k1, *v1, *hist;
    // the carve for M pairs, in the order of the members
    static PairSort carve(Carver& c, size_t M) {
        PairSort p;
        p.k0 = c.take<uint32_t>(M);
        p.v0 = c.take<uint32_t>(M);
        p.k1 = c.take<uint32_t>(M);
        p.v1 = c.take<uint32_t>(M);
        p.hist = c.take<uint32_t>(sort_table_words(M));
        return p;
    }
    // where a sort on key bits [0, bits) leaves its result: an odd number of passes ends in buffer 1 (the one place that
    // knows; a sort of no pairs moves nothing, and nobody reads its result)
    const uint32_t* sorted_keys(int bits) const { return (radix_passes(bits) & 1) ? k1 : k0; }
    const uint32_t* sorted_vals(int bits) const { return (radix_passes(bits) & 1) ? v1 : v0; }
    // the per-pass digit totals, for a kernel in front of the sort to clear on the side (launch_sort_pairs: totals_zeroed)
    ZeroJob totals_job(int64_t n, int bits) const {
        ZeroJob z;
        sort_totals_region(hist, n, bits, &z.ptr, &z.words);
        return z;
    }
    int sort(int64_t n, int bits, hipStream_t s) const { return launch_sort_pairs(k0, v0, k1, v1, hist, n, bits, true, 0, s); }
};

// The hand-off of one lane's long job to its whole wave -- "for every lane whose flag is set, in lane order: broadcast its
// values with __shfl(., lane) and run the wave-uniform body" -- is written out where it is used (below, aiap_bwd_kernel,
// hg_entries_kernel): as a helper taking the body as a lambda it did not compile to the same loop (5-14 % more
// instructions in aiap_bwd_kernel, other register allocation in hg_entries_kernel).

// list_starts: start[e] = the first sorted pair whose key is >= e, e = 0 .. n_keys, from the M sorted keys `ks` (all
// <= n_keys).  Thread q = 0 .. M (q = M: a virtual pair of key n_keys) writes start[prev key + 1 .. key] = q: every word is
// written exactly once, by the pair that ends the gap in front of it; a gap longer than a wave is filled by the whole
// wave.  Every lane of a wave must call it (q > M: nothing to write).
__device__ __forceinline__ void list_starts(const uint32_t* __restrict__ ks, long long M, uint32_t n_keys, long long q,
                                            uint32_t* __restrict__ start) {
    const int lane = threadIdx.x & (WAVE - 1);
    long long lo = 0, hi = -1;  // this pair writes start[lo .. hi] = q
    if (q <= M) {
        const long long key = q < M ? (long long)ks[q] : (long long)n_keys;
        const long long prev = q > 0 ? (long long)ks[q - 1] : -1;
        lo = prev + 1;
        hi = key;
    }
    const bool big = hi - lo + 1 > WAVE;
    if (!big)
        for (long long t = lo; t <= hi; t++) start[t] = (uint32_t)q;
    unsigned long long bal = __ballot(big);
    while (bal) {  // (wave-uniform)
        const int L = __ffsll((long long)bal) - 1;
        bal &= bal - 1;
        const long long blo = (long long)__shfl((int)lo, L), bhi = (long long)__shfl((int)hi, L);
        const uint32_t bq = (uint32_t)__shfl((int)q, L);
        for (long long t = blo + lane; t <= bhi; t += WAVE) start[t] = bq;
    }
}
