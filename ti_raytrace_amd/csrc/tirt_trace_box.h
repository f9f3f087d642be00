// tirt_trace_box.h -- the box arithmetic of a RAY over the quantised 4-wide nodes `cnode` (tirt_internal.h), once, for k_trace (tirt_trace.hip) and
// k_multi_hit (tirt_multi_hit.hip): the per-ray set-up of one axis (TR_GRID_AXIS) and the test of one child's box (TR_CBOX).  They are macros over the
// NAMES of the kernel that expands them, as they were inside k_trace (moved here as text: k_trace's instructions are the ones they were):
//   TR_GRID_AXIS  reads  mc__ (trace_margin_cells of trace_origin_rho's expression), c_ic0 .. c_ic2 (BvhView::inv_cell), c_ce0 .. c_ce2 (BvhView::cell)
//   TR_CBOX       reads  grotx / groty / grotz, gAx .. gAz, gBnx .. gBnz, gBfx .. gBfz (what TR_GRID_AXIS made), lim_i (the bits of the cull distance, > 0), MISS
// What they compute, and why the margin is conservative: k_trace's per-lane ray state (tirt_trace.hip) and trace_margin_cells (tirt_internal.h).
#pragma once
#include "tirt_internal.h"

namespace tirt {
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
// The distance cull of the ordered walk: a child whose entry distance exceeds min(TR_CULL_SLACK * threshold distance, TR_BOUND_SLACK * bound, INF_VALUE) is
// skipped.  The threshold is the closest hit so far (k_trace) or the list's worst entry (k_multi_hit); the bound is a shadow ray's target distance or a query's tmax.
constexpr float TR_CULL_SLACK = 1.0001f, TR_BOUND_SLACK = 1.01f;
}  // namespace tirt

#define TR_GRID_AXIS(rel, dd, idd, k, gA, gBn, gBf, grot)                                            \
                    do {                                                                             \
                        if (absf(dd) < 0.000001f) {      /* the reference's parallel case: origin inside the slab or no hit */ \
                            const float og__ = -(rel) * (k == 0 ? c_ic0 : (k == 1 ? c_ic1 : c_ic2));                               \
                            gA = 1.0e30f; gBn = (-og__ - (mc__ + 1.0f)) * 1.0e30f; gBf = (-og__ + (mc__ + 1.0f)) * 1.0e30f; grot = 0; \
                        } else {                                                                     \
                            gA = (k == 0 ? c_ce0 : (k == 1 ? c_ce1 : c_ce2)) * (idd);                                                  \
                            const float gB__ = (rel) * (idd);                                        \
                            const float m__ = mc__ * absf(gA);                                       \
                            gBn = gB__ - m__; gBf = gB__ + m__; grot = gA < 0.0f ? 16 : 0;           \
                        }                                                                            \
                    } while (0)

#define TR_CBOX(X, Y, Z, dist)                                                                       \
                    do {                                                                             \
                        const unsigned ux__ = __builtin_amdgcn_alignbit((X), (X), grotx);            \
                        const unsigned uy__ = __builtin_amdgcn_alignbit((Y), (Y), groty);            \
                        const unsigned uz__ = __builtin_amdgcn_alignbit((Z), (Z), grotz);            \
                        const h2v hx__ = __builtin_bit_cast(h2v, ux__), hy__ = __builtin_bit_cast(h2v, uy__), hz__ = __builtin_bit_cast(h2v, uz__); \
                        const float nx__ = __builtin_fmaf((float)hx__.x, gAx, gBnx), fx__ = __builtin_fmaf((float)hx__.y, gAx, gBfx); \
                        const float ny__ = __builtin_fmaf((float)hy__.x, gAy, gBny), fy__ = __builtin_fmaf((float)hy__.y, gAy, gBfy); \
                        const float nz__ = __builtin_fmaf((float)hz__.x, gAz, gBnz), fz__ = __builtin_fmaf((float)hz__.y, gAz, gBfz); \
                        const float tn__ = __builtin_fmaxf(__builtin_fmaxf(nx__, ny__), __builtin_fmaxf(nz__, 0.0f)); \
                        /* the far distance in the INTEGER domain (v_min_i32 / v_min3_i32: no canonicalisation of `lim` per step):   \
                           exact for non-negative floats, and a negative operand (box behind the ray) gives a negative result */      \
                        const int tfi__ = min(min(__float_as_int(fx__), __float_as_int(fy__)), min(__float_as_int(fz__), lim_i));     \
                        const float tf__ = __int_as_float(tfi__);                                    \
                        dist = (tn__ <= tf__) ? tn__ : MISS;                                         \
                    } while (0)
