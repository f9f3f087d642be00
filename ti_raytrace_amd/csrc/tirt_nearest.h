// tirt_nearest.h -- the neighbour list of k_nn_walk / k_nn_scan (tirt_nearest.hip; include/tirt.h "K nearest primitives"): the k nearest primitives of one
// query point, kept in the definition's order while candidates arrive in the order of the walk.  __host__ __device__, so that tirt_kat_nearest_list runs
// this text on the host.
//
// ORDER.  D2 ascending; at equal D2 bits the SMALLER primitive id first -- cp_accept's comparison (tirt_closest_point.h), so "sorts before the threshold"
// and "would replace the closest point's answer" are one rule.  A NaN compares false everywhere and +inf is not below +inf: neither is ever accepted.
// THRESHOLD.  (thr_d2, thr_prim) is what a candidate has to sort before in order to join: "nothing" = (+inf, -1) while the list has room -- then the lim2
// term of cp_accept alone decides, which is membership of the set N --, the last (worst) entry's key once it holds k.  It lives in registers: a rejected
// candidate costs no memory access.
// THE LIST is sorted by insertion from the back, as MhList::insert (tirt_multi_hit.h): entries that sort behind the candidate move down one slot, the one in
// slot k - 1 of a full list falls out.  A best-first walk meets candidates nearly in order, so a typical insertion touches the last slot or two.  The keys
// of one query are distinct (a primitive is met at most once), so the list is the first k of the accepted candidates in a total order: it does not depend
// on the order in which they come.  `L` is the storage: get(e) / set(e, entry) of slot e (device: the chunk scratch [entry][query]; host: two arrays).
// An entry is 8 bytes, (D2 bits, prim); Q, u and v are not kept: k_nn_resolve forms them again from the primitive's record.
#pragma once
#include "tirt_closest_point.h"

#define NN_HD __host__ __device__ inline

namespace tirt {

struct NnEntry { float d2; int prim; };

// the state of one query's list beside the storage: entries held, and the threshold
struct NnList {
    int k, n;
    float thr_d2; int thr_prim;
    NN_HD explicit NnList(int k_) : k(k_), n(0), thr_d2(__builtin_inff()), thr_prim(-1) {}
    // is the candidate an element of N: D2 <= lim2 and D2 < +inf (cp_accept against "nothing")
    static NN_HD bool member(float d2, int prim, float lim2) { return cp_accept(d2, prim, lim2, __builtin_inff(), -1); }
    NN_HD bool wants(float d2, int prim, float lim2) const { return (k > 0) & cp_accept(d2, prim, lim2, thr_d2, thr_prim); }
    // a candidate that `wants` said yes to (k > 0)
    template <class L>
    NN_HD void insert(L &list, const NnEntry c)
    {
        int pos = n < k ? n : k - 1;                  // the slot that opens: behind the last entry, or the last entry's (it falls out)
        NnEntry last = c;                             // what ends up in slot k - 1 of a full list
        bool moved = false;
        while (pos > 0) {
            const NnEntry e = list.get(pos - 1);
            if (!cp_accept(c.d2, c.prim, __builtin_inff(), e.d2, e.prim)) break;
            list.set(pos, e);
            if (!moved) { last = e; moved = true; }
            pos--;
        }
        list.set(pos, c);
        if (n < k) n++;
        if (n == k) { thr_d2 = last.d2; thr_prim = last.prim; }
    }
};

}  // namespace tirt
