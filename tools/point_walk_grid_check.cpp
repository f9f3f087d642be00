// The grid arithmetic behind the point walks' stacks (point_walk_grid, csrc/tirt_point_walk.h) as a stand-alone host program, for the host sanitizers:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=undefined,address -fno-sanitize-recover=all tools/point_walk_grid_check.cpp -o point_walk_grid_check
// It touches no device.  For every combination below: at least one block, no more blocks than the work has, and, whenever there is more than one
// block, tails that fit CP_SPILL_BYTES_MAX -- the buffer PointStack indexes as [entry][grid * CP_BLOCK].  tests/test_point_walk_host.py builds and runs it.
#include "../ti_raytrace_amd/csrc/tirt_point_walk.h"

int main()
{
    using namespace tirt;
    const int cus[] = {1, 64, 256, 100000}, stacks[] = {1, CP_LDS_DEPTH, CP_LDS_DEPTH + 1, 4096}, waves[] = {16, 20};
    const size_t entries[] = {4, 8};
    const int64_t works[] = {1, (int64_t)1 << 20};
    int bad = 0, cases = 0;
    for (int cu : cus) for (int stack : stacks) for (int w : waves) for (size_t e : entries) for (int64_t work : works) {
        size_t tail = ~(size_t)0;
        const int grid = point_walk_grid(cu, stack, e, w, work, tail);
        const size_t want_tail = stack > CP_LDS_DEPTH ? (size_t)(stack - CP_LDS_DEPTH) * e : 0;
        const bool ok = grid >= 1 && grid <= work && tail == want_tail && (grid == 1 || tail * CP_BLOCK * (size_t)grid <= CP_SPILL_BYTES_MAX) &&
                        (grid == work || grid == (int64_t)cu * w || (tail && (size_t)(grid + 1) * tail * CP_BLOCK > CP_SPILL_BYTES_MAX));      // (and no smaller than it has to be)
        if (!ok) { printf("FAIL cu %d stack %d waves %d entry %zu work %lld: grid %d tail %zu\n", cu, stack, w, e, (long long)work, grid, tail); bad++; }
        cases++;
    }
    printf("point_walk_grid: %d cases, %d failed\n", cases, bad);
    return bad ? 1 : 0;
}
