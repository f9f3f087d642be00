// stand-alone: the neighbour list of csrc/tirt_nearest.h on the host, on exactly-sized heap arrays, against std::stable_sort
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "tirt_nearest.h"
using namespace tirt;
struct HostList {
    float *d2; int *prim;
    NnEntry get(int e) const { NnEntry r; r.d2 = d2[e]; r.prim = prim[e]; return r; }
    void set(int e, const NnEntry c) const { d2[e] = c.d2; prim[e] = c.prim; }
};
int main()
{
    std::mt19937 rng(7);
    const float vals[] = {0.0f, 0.5f, 2.5f, 2.5000002f, 7.0f, NAN, INFINITY};
    const float lims[] = {-1.0f, 0.0f, 2.5f, INFINITY};
    long checked = 0;
    for (int k : {0, 1, 2, 7, 64}) for (int n = 0; n <= 200; n++) for (float lim2 : lims) {
        std::vector<int> ids(4 * n + 8); for (size_t i = 0; i < ids.size(); i++) ids[i] = (int)i;
        std::shuffle(ids.begin(), ids.end(), rng);
        std::vector<NnEntry> c(n);
        for (int i = 0; i < n; i++) { c[i].d2 = vals[rng() % 7]; c[i].prim = ids[i]; }
        float *od = new float[k]; int *op = new int[k];      // exactly k: an access to slot k is out of bounds
        HostList list = {od, op};
        NnList L(k);
        int members = 0;
        for (const NnEntry &e : c) { if (NnList::member(e.d2, e.prim, lim2)) members++; if (L.wants(e.d2, e.prim, lim2)) L.insert(list, e); }
        std::vector<NnEntry> w;
        for (const NnEntry &e : c) if (e.d2 <= lim2 && e.d2 < INFINITY) w.push_back(e);
        std::stable_sort(w.begin(), w.end(), [](const NnEntry &a, const NnEntry &b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.prim < b.prim); });
        const int held = (int)std::min<size_t>(w.size(), (size_t)k);
        if (L.n != held || members != (int)w.size()) { printf("FAIL counts k %d n %d lim2 %g: %d %d %d %zu\n", k, n, lim2, L.n, held, members, w.size()); return 1; }
        for (int j = 0; j < held; j++) if (memcmp(&od[j], &w[j].d2, 4) || op[j] != w[j].prim) { printf("FAIL entry k %d n %d j %d\n", k, n, j); return 1; }
        delete[] od; delete[] op; checked++;
    }
    printf("nn_list_main: %ld cases equal std::stable_sort\n", checked);
    return 0;
}
