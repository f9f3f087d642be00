// tirt_multi_hit.h -- the hit list of k_multi_hit (tirt_multi_hit.hip; include/tirt.h "First K hits"): the k nearest hits of one ray, kept in the
// definition's order while candidates arrive in the order of the walk.  __host__ __device__, so that tirt_kat_hit_list runs this text on the host.
//
// ORDER.  t ascending; at equal t bits the LARGER compact leaf index first -- hit_before is trace_leaf_step's acceptance comparison (tirt_internal.h), so
// "sorts before the threshold" and "trace_leaf_step returns true against the threshold" are one rule.  A NaN compares false everywhere: never accepted.
// THRESHOLD.  (thr_t, thr_leaf) is what a candidate has to sort before in order to join: (bound, -1) while the list has room -- leaf -1 switches the
// equal-distance term off, so t == bound is out --, the last (worst) entry's key once it holds k.  It lives in registers: a rejected candidate
// costs no memory access.
// THE LIST is sorted by insertion from the back: entries that sort behind the candidate move down one slot, the one in slot k - 1 of a full list falls out.
// An ordered walk meets candidates nearly in order, so a typical insertion touches the last slot or two.  Equal keys keep their order of arrival (the
// later one goes behind, and is rejected by a full list whose threshold it equals): the list is what a stable sort of the accepted candidates by
// (t, -leaf) would begin with.  `L` is the storage: get(e) / set(e, entry) of slot e (device: the chunk scratch [entry][ray]; host: a vector).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MH_HD __host__ __device__ inline
#else
#define MH_HD inline
#endif

namespace tirt {

struct MhEntry { float t, u, v; int leaf; };      // 16 bytes: the hit (t, u, v) and the compact index of its leaf (the primitive is that row's)

MH_HD bool hit_before(float t, int leaf, float thr_t, int thr_leaf)
{ return (t < thr_t) | ((t == thr_t) & (thr_leaf >= 0) & (leaf > thr_leaf)); }

// the state of one ray's list beside the storage: entries held, and the threshold
struct MhList {
    int k, n;
    float thr_t; int thr_leaf;
    MH_HD MhList(int k_, float bound) : k(k_), n(0), thr_t(bound), thr_leaf(-1) {}
    MH_HD bool wants(float t, int leaf) const { return (k > 0) & (t > 0.0f) & hit_before(t, leaf, thr_t, thr_leaf); }
    // a candidate that `wants` said yes to (k > 0)
    template <class L>
    MH_HD void insert(L &list, const MhEntry c)
    {
        int pos = n < k ? n : k - 1;                  // the slot that opens: behind the last entry, or the last entry's (it falls out)
        MhEntry last = c;                             // what ends up in slot k - 1 of a full list
        bool moved = false;
        while (pos > 0) {
            const MhEntry e = list.get(pos - 1);
            if (!hit_before(c.t, c.leaf, e.t, e.leaf)) break;      // (entries hold real leaves: >= 0)
            list.set(pos, e);
            if (!moved) { last = e; moved = true; }
            pos--;
        }
        list.set(pos, c);
        if (n < k) n++;
        if (n == k) { thr_t = last.t; thr_leaf = last.leaf; }
    }
};

}  // namespace tirt
