// The layout behind the staging of the queries' host entries (stage_layout, csrc/tirt_query_stage.h) as a stand-alone host program, for the host sanitizers:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all tools/query_stage_check.cpp -o query_stage_check
// It touches no device.  The column lists are those the seven host routes declare to QueryStage (trace_host, trace_hits_host, closest_point_host, tirt_nearest,
// tirt_mesh_distance, pairs_host for points and for triangles, tirt_sweep), each with every column there and with every optional column left out, for
// n in {1, 2, 3, 255, 256, 257}, k in {0, 1, 3, 64} and pair capacities {0, 1, 7}.  For every list: each offset is a multiple of its column's element size,
// the columns do not overlap, the total covers the last column and is no less than the sum of the column sizes, and a malloc of exactly the total is
// written through every column end to end -- under ASan a byte too many is a report -- and read back: a column that another one overwrote shows.
// tests/test_query_stage_host.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../ti_raytrace_amd/csrc/tirt_query_stage.h"

using tirt::StageColumn;
typedef std::vector<StageColumn> List;

static int cases = 0, bad = 0;

static void check(const char *route, size_t n, size_t k, size_t cap, const List &cols)
{
    std::vector<size_t> off(cols.size(), ~(size_t)0);
    const size_t total = tirt::stage_layout(cols.data(), cols.size(), off.data());
    bool ok = true;
    size_t sum = 0, end = 0;
    for (size_t i = 0; i < cols.size(); i++) {
        const size_t bytes = cols[i].elem * cols[i].count;
        ok = ok && off[i] % cols[i].elem == 0;       // aligned to its element
        ok = ok && off[i] >= end;                    // behind everything before it
        end = off[i] + bytes;
        sum += bytes;
    }
    ok = ok && total >= end && total >= sum;
    if (ok) {
        unsigned char *buf = (unsigned char *)malloc(total);      // (exactly the total: malloc(0) may be null, and nothing is written then)
        for (size_t i = 0; i < cols.size(); i++) if (cols[i].count) memset(buf + off[i], (int)(i + 1), cols[i].elem * cols[i].count);
        for (size_t i = 0; i < cols.size(); i++)
            for (size_t b = 0; b < cols[i].elem * cols[i].count; b++) ok = ok && buf[off[i] + b] == (unsigned char)(i + 1);
        free(buf);
    }
    if (!ok) { printf("FAIL %s n %zu k %zu capacity %zu: total %zu\n", route, n, k, cap, total); bad++; }
    cases++;
}

// every column of the list, then the list with the optional ones (those marked) left out: QueryStage gives a column that is not there 0 elements
struct Opt { StageColumn col; bool optional; };
static void both(const char *route, size_t n, size_t k, size_t cap, const std::vector<Opt> &cols)
{
    List full, least;
    for (const Opt &o : cols) { full.push_back(o.col); least.push_back(StageColumn{o.col.elem, o.optional ? 0 : o.col.count}); }
    check(route, n, k, cap, full);
    check(route, n, k, cap, least);
}

int main()
{
    const size_t ns[] = {1, 2, 3, 255, 256, 257}, ks[] = {0, 1, 3, 64}, caps[] = {0, 1, 7};
    const size_t F = 4, I = 4, B = 1, L = 8;      // float, int32, a byte, int2 / int64
    for (size_t n : ns) {
        for (size_t wide : {(size_t)1, (size_t)13})      // tirt_trace_shadow: t; tirt_trace_closest: the record
            both("trace_host", n, 0, 0, {{{F, 6 * n}, false}, {{F, wide * n}, false}, {{I, n}, false}, {{L, n}, true}});
        both("closest_point_host", n, 0, 0, {{{F, 3 * n}, false}, {{F, n}, true}, {{F, n}, false}, {{I, n}, false}, {{F, 3 * n}, false}, {{F, 2 * n}, false}, {{L, n}, true}, {{F, n}, true}});
        both("tirt_mesh_distance", n, 0, 0, {{{F, 9 * n}, false}, {{F, n}, true}, {{F, n}, false}, {{I, n}, false}, {{I, n}, false}, {{F, 6 * n}, false}, {{L, n}, true}});
        both("tirt_sweep", n, 0, 0, {{{F, 6 * n}, false}, {{F, n}, true}, {{F, n}, true}, {{F, n}, true}, {{I, n}, true}, {{I, n}, true}, {{F, 3 * n}, true}, {{F, 2 * n}, true},
                                    {{F, 3 * n}, true}, {{B, n}, false}, {{L, n}, true}});
        for (size_t k : ks) {
            both("trace_hits_host", n, k, 0, {{{F, 6 * n}, false}, {{F, n}, true}, {{F, k * n}, true}, {{I, k * n}, true}, {{F, 13 * k * n}, true}, {{I, n}, true}, {{L, n}, true}});
            both("tirt_nearest", n, k, 0, {{{F, 3 * n}, false}, {{F, n}, true}, {{I, n}, true}, {{F, k * n}, true}, {{I, k * n}, true}, {{F, 3 * k * n}, true}, {{F, 2 * k * n}, true}, {{L, n}, true}});
        }
        for (size_t cap : caps) {
            both("pairs_host (points)", n, 0, cap, {{{L, n + 1}, false}, {{F, 3 * n}, false}, {{F, n}, true}, {{F, cap}, true}, {{I, cap}, true}, {{I, 0}, true}, {{F, 3 * cap}, true}, {{F, 2 * cap}, true}, {{L, n}, true}});
            both("pairs_host (triangles)", n, 0, cap, {{{L, n + 1}, false}, {{F, 9 * n}, false}, {{F, n}, true}, {{F, cap}, true}, {{I, cap}, true}, {{I, cap}, true}, {{F, 6 * cap}, true}, {{F, 0}, true}, {{L, n}, true}});
        }
    }
    printf("query_stage: %d cases, %d failed\n", cases, bad);
    return bad ? 1 : 0;
}
