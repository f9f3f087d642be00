// tirt_pairs.h -- what the pair lists (tirt_pairs.hip; include/tirt.h "Point pairs" / "Triangle pairs") share between the device and the host: the key of a
// pair, THE ORDER of a row as a sorting network over any storage, the decomposition of THE SCAN that turns row lengths into row_start, and the capacity
// rule.  __host__ __device__, so that tirt_kat_pairs_host runs this text on the host.
//
// KEY.  (uint64) bits(D2) << 32 | prim.  An element of a row has D2 >= +0 and D2 < +inf and is never a NaN (NnList::member, tirt_nearest.h), and no D2 is -0
// (a sum of squares), so the order of the bit patterns is the order of the floats: unsigned comparison of the keys is "D2 ascending, at equal D2 bits the
// smaller primitive id first", cp_accept's order (tirt_closest_point.h).  The keys of one row are distinct (a primitive is met at most once).
// ORDER.  A bitonic sorting network in the form whose compare-exchanges all point the same way -- the smaller key to the smaller index:
//     for k = 2, 4, 8, ... while k / 2 < len:   the flip step: inside every block of k slots, slot o < k / 2 against slot k - 1 - o;
//                                               then for j = k / 4, k / 8, ..., 1: slot i against slot i + j where bit j of i is clear
// A compare-exchange whose upper slot is >= len is left out.  That is the network on the next power of two with the slots from len on holding +inf: they
// are the upper operand of every exchange they take part in and never move, so the network sorts any length in place.  Each step's exchanges touch disjoint
// pairs of slots: the wave runs them side by side (t = lane, lane + 64, ...) with a barrier between steps, the host one after the other.  The result is
// the sorted row, which for distinct keys does not depend on how the row came.
// SCAN.  row_start[i + 1] holds the length of row i when the scan begins and the inclusive prefix sum when it ends; row_start[0] = 0.  Three passes over
// blocks of PAIRS_SCAN_BLOCK lengths -- the sum of every block, the exclusive sums of those sums (one block), each block's own inclusive sums plus its
// offset -- as k_pixel_count / k_pixel_scan / k_pixel_scatter (tirt_adaptive.hip): no block waits for another.
// CAPACITY.  A row is written iff it fits entirely: 0 <= row_start[i] <= row_start[i + 1] <= capacity (pairs_row_fits).  The prefix sums only grow, so
// the rows that fit are a prefix of the rows; no partial row is ever written -- its content would depend on the order of the walk.
#pragma once
#include <stdint.h>
#include "tirt_nearest.h"

#define PAIRS_HD __host__ __device__ inline

namespace tirt {

constexpr int PAIRS_LDS_ROW = 1024;          // the longest row that is ordered in LDS (8 KiB of keys: the walk's own LDS budget); a longer one in place in the caller's arrays
constexpr int PAIRS_SCAN_BLOCK = 1024;       // lengths per block of the scan

PAIRS_HD uint64_t pairs_key(uint32_t d2_bits, int prim) { return ((uint64_t)d2_bits << 32) | (uint32_t)prim; }

// the number of the rows that fit and their lengths (the rule of the head)
PAIRS_HD bool pairs_row_fits(int64_t r0, int64_t r1, int64_t capacity) { return (r0 >= 0) & (r0 <= r1) & (r1 <= capacity); }
// the length of a row that fits as an int, 0 for one that does not (a row has at most one pair per primitive: it fits an int)
PAIRS_HD int pairs_row_len(int64_t r0, int64_t r1, int64_t capacity)
{
    const int64_t len = r1 - r0;
    return pairs_row_fits(r0, r1, capacity) ? (int)(len < 0x7fffffff ? len : 0x7fffffff) : 0;
}

// exchange number t of the step (k, j) of the network: its two slots lo < hi (j == 0: the flip step of the merge of blocks of k)
// (k and j are powers of two: o = t mod h, and 2 (t - o) is the first slot of the block of 2 h slots that exchange t lies in)
PAIRS_HD void pairs_step_slots(int k, int j, int64_t t, int64_t &lo, int64_t &hi)
{
    const int64_t h = j == 0 ? (k >> 1) : j, o = t & (h - 1), first = (t - o) << 1;
    lo = first + o;
    hi = j == 0 ? first + (k - 1 - o) : lo + j;
}
// the exchanges of a step that can have hi < len: t < len suffices (lo >= t); half the next power of two is the tighter count
PAIRS_HD int64_t pairs_step_count(int64_t len) { int64_t p = 1; while (p < len) p <<= 1; return p >> 1; }

// one exchange on the storage M: key(i) -> uint64, swap(i, j)
template <class M>
PAIRS_HD void pairs_exchange(M &m, int k, int j, int64_t t, int64_t len)
{
    int64_t lo, hi;
    pairs_step_slots(k, j, t, lo, hi);
    if (hi < len) { if (m.key(hi) < m.key(lo)) m.swap(lo, hi); }
}

// the steps of the network in order: step(k, j) has to run exchanges 0 .. pairs_step_count(len) - 1 of that step, all of them before the next step begins
template <class Step>
PAIRS_HD void pairs_sort_steps(int64_t len, Step step)
{
    for (int64_t k = 2; (k >> 1) < len; k <<= 1) {
        step((int)k, 0);
        for (int64_t j = k >> 2; j >= 1; j >>= 1) step((int)k, (int)j);
    }
}

// the three passes of the scan over rs = row_start + 1 (n lengths in, n inclusive sums out), as the host runs them: `sums` holds a block's sum, then its offset
inline int64_t pairs_scan_blocks(int64_t n) { return (n + PAIRS_SCAN_BLOCK - 1) / PAIRS_SCAN_BLOCK; }
inline void pairs_scan_host(int64_t *row_start, int64_t n, int64_t *sums)
{
    int64_t *rs = row_start + 1;
    const int64_t nb = pairs_scan_blocks(n);
    for (int64_t b = 0; b < nb; b++) {                                                   // (1)
        int64_t s = 0;
        for (int64_t i = b * PAIRS_SCAN_BLOCK; i < n && i < (b + 1) * PAIRS_SCAN_BLOCK; i++) s += rs[i];
        sums[b] = s;
    }
    int64_t carry = 0;
    for (int64_t b = 0; b < nb; b++) { const int64_t s = sums[b]; sums[b] = carry; carry += s; }      // (2)
    for (int64_t b = 0; b < nb; b++) {                                                   // (3)
        int64_t run = sums[b];
        for (int64_t i = b * PAIRS_SCAN_BLOCK; i < n && i < (b + 1) * PAIRS_SCAN_BLOCK; i++) { run += rs[i]; rs[i] = run; }
    }
    row_start[0] = 0;
}

}  // namespace tirt
