// tirt_query_stage.h -- how the host entries of the queries (tirt_trace_closest / _shadow, tirt_trace_hits, tirt_closest_point / tirt_signed_distance,
// tirt_nearest, tirt_mesh_distance, tirt_point_pairs / tirt_mesh_pairs, tirt_sweep) stage their arrays in device memory, in two layers:
//   stage_layout   where each column of a list lies and how long the whole is: plain arithmetic, no HIP and no context (tools/query_stage_check.cpp runs it
//                  under the host sanitizers for the column lists of all these entries)
//   QueryStage     the columns of one call in the context's staging buffer (trace_stage: used by these entries alone, and each of their calls ends with a
//                  sync of the stream that used it, so growing it waits for nothing)
// The size of the buffer is the layout's total and nothing else: no entry writes a byte count or a pointer chain of its own.
#pragma once
#include <stddef.h>

namespace tirt {

struct StageColumn { size_t elem, count; };      // bytes of an element (a power of two: 1, 4, 8) and elements
// offset[i] = where column i starts, a multiple of its element size, in the order given; returns the bytes of the whole
inline size_t stage_layout(const StageColumn *col, size_t n, size_t *offset)
{
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t e = col[i].elem;
        at = (at + e - 1) / e * e;
        offset[i] = at;
        at += e * col[i].count;
    }
    return at;
}

}  // namespace tirt

#ifdef __HIP__
#include "tirt_internal.h"

namespace tirt {

template <class T> struct StageCol { int i; };      // a column of a QueryStage, by its element type

// One call's columns.  in() / out() declare them; begin() lays them out, grows the buffer and copies the inputs up; ptr() is a column's device pointer;
// after the launches finish() copies down every output whose host pointer is not null (fetch() one of them earlier, or only its head), waits for the
// stream and returns the launches' error.
class QueryStage {
    struct Col { const void *up; void *down; bool present; };
    tirt_ctx *c;
    std::vector<StageColumn> shape;      // (a column that is not on the device has 0 elements)
    std::vector<Col> cols;
    std::vector<size_t> offset;
    template <class T> StageCol<T> add(size_t count, const void *up, void *down, bool present)
    {
        shape.push_back(StageColumn{sizeof(T), present ? count : 0});
        cols.push_back(Col{up, down, present});
        return StageCol<T>{(int)cols.size() - 1};
    }
    char *at(size_t i) const { return c->trace_stage.as<char>() + offset[i]; }
    int fetch_column(size_t i, size_t count)
    {
        if (count > shape[i].count) count = shape[i].count;      // (never beyond the column)
        if (cols[i].down && count) TIRT_HIP(hipMemcpyAsync(cols[i].down, at(i), shape[i].elem * count, hipMemcpyDeviceToHost, c->stream));
        cols[i].down = nullptr;
        return TIRT_OK;
    }
public:
    explicit QueryStage(tirt_ctx *c_) : c(c_) {}
    // an input: `count` elements at `host`; a null host pointer is an array the caller left out: no column, a null device pointer
    template <class T> StageCol<T> in(const T *host, size_t count) { return add<T>(count, host, nullptr, host != nullptr); }
    // an output: on the device iff `present` (what the kernels are handed), copied back iff `host` is not null
    template <class T> StageCol<T> out(T *host, size_t count, bool present = true) { return add<T>(count, nullptr, present ? host : nullptr, present); }
    // N_box / N_leaf per query: there iff the caller gave the array and asked for TIRT_COUNT_NODES
    StageCol<int2> out_counts(int32_t *counts, int flags, size_t n) { return out((int2 *)counts, n, counts && (flags & TIRT_COUNT_NODES)); }
    int begin()
    {
        offset.resize(cols.size());
        if (c->trace_stage.ensure(stage_layout(shape.data(), shape.size(), offset.data()))) return TIRT_ERR_HIP;
        for (size_t i = 0; i < cols.size(); i++)
            if (cols[i].up && shape[i].count) TIRT_HIP(hipMemcpyAsync(at(i), cols[i].up, shape[i].elem * shape[i].count, hipMemcpyHostToDevice, c->stream));
        return TIRT_OK;
    }
    template <class T> T *ptr(StageCol<T> k) const { return cols[k.i].present ? (T *)at(k.i) : nullptr; }
    // the first `count` elements of an output now, or all of it (finish() leaves the column alone then)
    template <class T> int fetch(StageCol<T> k, size_t count) { return fetch_column(k.i, count); }
    template <class T> int fetch(StageCol<T> k) { return fetch_column(k.i, shape[k.i].count); }
    int sync() { TIRT_HIP(hipStreamSynchronize(c->stream)); return TIRT_OK; }
    int finish()
    {
        for (size_t i = 0; i < cols.size(); i++) if (int rc = fetch_column(i, shape[i].count)) return rc;
        TIRT_HIP(hipStreamSynchronize(c->stream));
        TIRT_HIP(hipGetLastError());
        return TIRT_OK;
    }
};

}  // namespace tirt
#endif
