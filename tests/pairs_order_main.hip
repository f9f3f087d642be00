// stand-alone: the scan and the sorting network of csrc/tirt_pairs.h on the host, on exactly-sized heap arrays, against std::stable_sort
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "tirt_pairs.h"
using namespace tirt;
struct HostRow {
    float *d2; int *prim;
    uint64_t key(int64_t i) const { uint32_t b; memcpy(&b, &d2[i], 4); return pairs_key(b, prim[i]); }
    void swap(int64_t i, int64_t j) const { std::swap(d2[i], d2[j]); std::swap(prim[i], prim[j]); }
};
struct Entry { float d2; int prim; };
int main()
{
    std::mt19937 rng(7);
    const float vals[] = {0.0f, 1e-45f, 1e-40f, 0.5f, 2.5f, 2.5000002f, 7.0f};
    long checked = 0;
    for (int len : {0, 1, 2, 3, 5, 6, 7, 63, 64, 65, 100, 1023, 1024, 1025, 3000}) for (int rep = 0; rep < 4; rep++) {
        std::vector<int> ids(4 * len + 8); for (size_t i = 0; i < ids.size(); i++) ids[i] = (int)i;
        std::shuffle(ids.begin(), ids.end(), rng);
        float *d2 = new float[len]; int *prim = new int[len];      // exactly len: an exchange that reaches slot len is out of bounds
        std::vector<Entry> w(len);
        for (int i = 0; i < len; i++) { d2[i] = w[i].d2 = vals[rng() % 7]; prim[i] = w[i].prim = ids[i]; }
        HostRow m = {d2, prim};
        const int64_t cnt = pairs_step_count(len);
        pairs_sort_steps(len, [&](int k, int j) { for (int64_t t = 0; t < cnt; t++) pairs_exchange(m, k, j, t, (int64_t)len); });
        std::stable_sort(w.begin(), w.end(), [](const Entry &a, const Entry &b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.prim < b.prim); });
        for (int j = 0; j < len; j++) if (memcmp(&d2[j], &w[j].d2, 4) || prim[j] != w[j].prim) { printf("FAIL entry len %d j %d\n", len, j); return 1; }
        delete[] d2; delete[] prim; checked++;
    }
    for (int64_t n : {0, 1, 1023, 1024, 1025, 5000}) {                 // the scan: n lengths behind row_start[0], block sums of their own
        int64_t *rs = new int64_t[n + 1], *sums = new int64_t[pairs_scan_blocks(n)];
        std::vector<int64_t> want(n + 1, 0);
        for (int64_t i = 0; i < n; i++) { rs[i + 1] = rng() % 9; want[i + 1] = want[i] + rs[i + 1]; }
        rs[0] = -5;
        pairs_scan_host(rs, n, sums);
        for (int64_t i = 0; i <= n; i++) if (rs[i] != want[i]) { printf("FAIL scan n %ld i %ld\n", (long)n, (long)i); return 1; }
        if (n && (pairs_row_fits(rs[n - 1], rs[n], rs[n] - 1) || !pairs_row_fits(rs[n - 1], rs[n], rs[n]))) { printf("FAIL capacity rule n %ld\n", (long)n); return 1; }
        delete[] rs; delete[] sums; checked++;
    }
    printf("pairs_order_main: %ld cases equal std::stable_sort / the running sum\n", checked);
    return 0;
}
