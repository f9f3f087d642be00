// tirt_temporal.hip -- temporal accumulation: the previous view's film and moment records reprojected into the current view and merged with it
// (tirt_temporal_device, tirt_motion_temporal_device, and the context's own history behind tirt_temporal_enable / _accumulate / _reset / _download / _export_device /
// _denoise_var, with the motion records of tirt_motion_enable / _download / _export_device).
//
// No reference counterpart.  This is the temporal part of SVGF (Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017) for a world that
// stands still: the backprojection goes through the first-hit surface point of the feature records (tirt_aov.hip) instead of motion vectors, the
// consistency tests are SVGF's normal and depth tests on the same records, and the merge is the pairwise update of Chan, Golub and LeVeque on the
// moment records (tirt_moments.hip) instead of an exponential blend -- capped at max_history samples, which makes it one.  include/tirt.h states the
// arithmetic; tests/temporal_expected.py restates it in numpy and the device has to give its bits, so every operation below is one f32 rounding in
// the order written there (-ffp-contract=off).
//
// k_temporal: one thread per current pixel p = i * H + j, the lanes along j, the contiguous axis.  Memory-bound: per pixel the current records
// (12 + 32 + 32 B, coalesced), up to four taps of the history, and 12 + 32 B out.  A tap's two 16-byte guide words are tested before its moment words
// and its hdr are fetched, so a rejected tap costs 32 B instead of 76; neighbouring lanes' taps are neighbouring pixels of the history (the
// reprojection of a small camera move is close to a translation), so their loads share cache lines.  No LDS, no atomics; the registers and the scratch
// the compiler reports are in DESIGN.md section 6.  Stores are plain (not non-temporal): the output is the next call's history and the filter's input.
//
// Moving geometry (tirt_motion_enable): SVGF's backprojection through the surface's own motion.  k_motion_resolve, one thread per pixel behind Debug's
// pixel-centre rays and their closest hits (debug_trace), evaluates the hit's barycentric point and shading normal on the vertex rows as they are and on
// the snapshot tirt_dynamic.hip took before the first update since the last accumulate: the record is (snapshot - current).  k_temporal<true> adds it to
// the surface point and to the current normal of step 1 (two more 16-byte loads per pixel); k_temporal<false> is the kernel as it was.
#include <string.h>
#include "tirt_internal.h"

namespace tirt {

TD bool tp_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // false for NaN

// what of the previous camera the kernel reads, and the parameters as the kernel uses them
struct TemporalPrev { float view[12]; float eye[3]; float fx, fy, cx, cy; };
struct TemporalParams { float max_history, sn2, sigma_z; };

// the barycentric point and the shading normal of a triangle hit on vertex rows, with hit_attributes' own expressions
TD void motion_point(const float *__restrict__ rows, int vi, float a, float u, float v, v3 &P, v3 &N)
{
    const float *r1 = rows + (size_t)vi * VER_VEC, *r2 = r1 + VER_VEC, *r3 = r2 + VER_VEC;
    const v3 v1 = V(r1[0], r1[1], r1[2]), v2 = V(r2[0], r2[1], r2[2]), v3_ = V(r3[0], r3[1], r3[2]);
    const v3 n1 = V(r1[3], r1[4], r1[5]), n2 = V(r2[3], r2[4], r2[5]), n3 = V(r3[3], r3[4], r3[5]);
    P = (v1 * a + v2 * u) + v3_ * v;
    N = normalized((n1 * a + n2 * u) + n3 * v);
}

// One thread per local pixel k (tile_count == 1: every pixel of the film), behind debug_trace at frame 0.  A miss and a hit on a shape: eight zeros.
// Both row sets hold nv rows and a triangle's vi + 2 < nv (tirt_scene_upload checks it); rec holds W * H records.
__global__ __launch_bounds__(256) void k_motion_resolve(const float *__restrict__ vertex, const float *__restrict__ snapshot, const int *__restrict__ primitive,
                                                        TileMap tm, int P, const float4 *__restrict__ hit, float4 *__restrict__ rec)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int p = local_to_pixel(tm, k);
    const float4 h = hit[k];
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
    if (h.x < INF_VALUE) {
        const int *pr = primitive + (size_t)__float_as_int(h.w) * PRI_VEC;
        if (pr[0] == PRIMITIVE_TRI) {
            const int vi = pr[1];
            const float a = 1.0f - h.y - h.z;
            v3 Pc, Nc, Ps, Ns;
            motion_point(vertex, vi, a, h.y, h.z, Pc, Nc);
            motion_point(snapshot, vi, a, h.y, h.z, Ps, Ns);
            r0 = make_float4(Ps.x - Pc.x, Ps.y - Pc.y, Ps.z - Pc.z, 1.0f);
            r1 = make_float4(Ns.x - Nc.x, Ns.y - Nc.y, Ns.z - Nc.z, 0.0f);
        }
    }
    rec[2 * (size_t)p] = r0; rec[2 * (size_t)p + 1] = r1;
}

template <bool MOTION>
__global__ __launch_bounds__(256) void k_temporal(const float *__restrict__ hdr_c, const float4 *__restrict__ aov_c, const float4 *__restrict__ mom_c,
                                                  const float *__restrict__ hdr_h, const float4 *__restrict__ aov_h, const float4 *__restrict__ mom_h,
                                                  float *__restrict__ hdr_o, float4 *__restrict__ mom_o, int W, int H, int NP,
                                                  CameraView cur, TemporalPrev prev, TemporalParams prm, const float4 *__restrict__ mv)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const int i = p / H, j = p - i * H;
    const float4 lo = aov_c[2 * (size_t)p], hi = aov_c[2 * (size_t)p + 1];
    const float4 c0 = mom_c[2 * (size_t)p], c1 = mom_c[2 * (size_t)p + 1];      // (n, mean.rgb), (M2.rgb, bad)
    const float *hc = hdr_c + 3 * (size_t)p;
    const float h0 = hc[0], h1 = hc[1], h2 = hc[2];
    float o0 = h0, o1 = h1, o2 = h2;                       // 6. no history: the current pixel, bit for bit
    float4 r0 = c0, r1 = c1;

    float ncx = lo.w, ncy = hi.x, ncz = hi.y;
    const float z = hi.z, al = hi.w;
    if (al > 0.0f) {
        // 1. the surface point the pixel's camera rays met, on the ray through the pixel centre
        const float zc = z / al;
        const v3 D = camera_ray_direction(cur, i, j, 0.0f, 0.0f);
        float Xx = cur.eye[0] + D.x * zc, Xy = cur.eye[1] + D.y * zc, Xz = cur.eye[2] + D.z * zc;
        if constexpr (MOTION) {                            // to where the surface was, with the normal it had
            const float4 d0 = mv[2 * (size_t)p], d1 = mv[2 * (size_t)p + 1];
            Xx = Xx + d0.x; Xy = Xy + d0.y; Xz = Xz + d0.z;
            ncx = ncx + d1.x; ncy = ncy + d1.y; ncz = ncz + d1.z;
        }
        // 2. where the previous camera saw it
        const float *V = prev.view;
        const float qx = ((V[0] * Xx + V[1] * Xy) + V[2] * Xz) + V[3];
        const float qy = ((V[4] * Xx + V[5] * Xy) + V[6] * Xz) + V[7];
        const float qz = ((V[8] * Xx + V[9] * Xy) + V[10] * Xz) + V[11];
        if (qz < 0.0f) {
            const float nz = -qz;
            const float fi = (qx / nz) * prev.fx + prev.cx, fj = (qy / nz) * prev.fy + prev.cy;
            if (fi > -1.0f && fi < (float)W && fj > -1.0f && fj < (float)H) {      // else no tap lies inside the film (NaN included)
                const float fi0 = __builtin_floorf(fi), fj0 = __builtin_floorf(fj);
                const int i0 = (int)fi0, j0 = (int)fj0;                            // -1 .. W-1, -1 .. H-1
                const float wi = fi - fi0, wj = fj - fj0;
                const float ex = Xx - prev.eye[0], ey = Xy - prev.eye[1], ez = Xz - prev.eye[2];
                const float d_exp = tm_sqrt((ex * ex + ey * ey) + ez * ez);
                const float ztol = prm.sigma_z * d_exp;
                // 3. the four bilinear taps
                float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
                float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f, m5 = 0.0f, m6 = 0.0f, m7 = 0.0f;
#pragma unroll
                for (int a = 0; a < 2; a++) {
                    const int ti = i0 + a;
                    if (ti < 0 || ti >= W) continue;
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const int tj = j0 + b;
                        if (tj < 0 || tj >= H) continue;
                        const size_t q = (size_t)ti * H + tj;
                        const float4 glo = aov_h[2 * q], ghi = aov_h[2 * q + 1];
                        if (!(ghi.w > 0.0f)) continue;
                        const float n0 = ncx - glo.w, n1 = ncy - ghi.x, n2 = ncz - ghi.y;
                        const float dn = (n0 * n0 + n1 * n1) + n2 * n2;
                        if (!(dn <= prm.sn2)) continue;
                        const float zh = ghi.z / ghi.w;
                        if (!(__builtin_fabsf(d_exp - zh) <= ztol)) continue;
                        const float4 t0 = mom_h[2 * q], t1 = mom_h[2 * q + 1];
                        if (!(t0.x > 0.0f)) continue;
                        const float *hh = hdr_h + 3 * q;
                        const float g0 = hh[0], g1 = hh[1], g2 = hh[2];
                        if (!(tp_finite(g0) && tp_finite(g1) && tp_finite(g2) && tp_finite(t0.y) && tp_finite(t0.z) && tp_finite(t0.w) &&
                              tp_finite(t1.x) && tp_finite(t1.y) && tp_finite(t1.z))) continue;
                        const float k = (a ? wi : 1.0f - wi) * (b ? wj : 1.0f - wj);
                        sw += k;
                        s0 += g0 * k; s1 += g1 * k; s2 += g2 * k;
                        m0 += t0.x * k; m1 += t0.y * k; m2 += t0.z * k; m3 += t0.w * k;
                        m4 += t1.x * k; m5 += t1.y * k; m6 += t1.z * k; m7 += t1.w * k;
                    }
                }
                if (sw >= 1e-3f) {
                    const float g0 = s0 / sw, g1 = s1 / sw, g2 = s2 / sw;
                    float nh = m0 / sw;
                    const float e0 = m1 / sw, e1 = m2 / sw, e2 = m3 / sw;
                    float q0 = m4 / sw, q1 = m5 / sw, q2 = m6 / sw, bh = m7 / sw;
                    // 4. the cap
                    if (nh > prm.max_history) {
                        const float f = prm.max_history / nh;
                        nh = prm.max_history;
                        q0 = q0 * f; q1 = q1 * f; q2 = q2 * f; bh = bh * f;
                    }
                    // 5. the merge
                    const float nc = c0.x, N = nh + nc;
                    bool merged = true;
                    if (nc == 0.0f) {
                        r0 = make_float4(nh, e0, e1, e2); r1 = make_float4(q0, q1, q2, bh);
                        o0 = g0; o1 = g1; o2 = g2;
                    } else if (N == 0.0f) {
                        merged = false;
                    } else {
                        const float w = nc / N, nw = nh * w;
                        const float d0 = c0.y - e0, d1 = c0.z - e1, d2 = c0.w - e2;
                        r0 = make_float4(N, e0 + d0 * w, e1 + d1 * w, e2 + d2 * w);
                        r1 = make_float4((q0 + c1.x) + (d0 * d0) * nw, (q1 + c1.y) + (d1 * d1) * nw, (q2 + c1.z) + (d2 * d2) * nw, bh + c1.w);
                        o0 = g0 + (h0 - g0) * w; o1 = g1 + (h1 - g1) * w; o2 = g2 + (h2 - g2) * w;
                    }
                    if (merged && !(tp_finite(h0) && tp_finite(h1) && tp_finite(h2))) { o0 = h0; o1 = h1; o2 = h2; }      // the film's NaN pixels stay
                }
            }
        }
    }
    float *ho = hdr_o + 3 * (size_t)p;
    ho[0] = o0; ho[1] = o1; ho[2] = o2;
    mom_o[2 * (size_t)p] = r0; mom_o[2 * (size_t)p + 1] = r1;
}

static const tirt_temporal_t TP_DEFAULTS = {TIRT_TEMPORAL_MAX_HISTORY, 0.3f, 0.1f};

static int temporal_check_params(const std::string &fn, const tirt_temporal_t *&prm)
{
    if (!prm) prm = &TP_DEFAULTS;
    const float s[3] = {prm->max_history, prm->sigma_n, prm->sigma_z};
    for (float v : s) TIRT_REQUIRE(v > 0.0f && v < __builtin_inff(), fn + ": max_history, sigma_n and sigma_z must be finite and > 0");
    return TIRT_OK;
}

// the kernel on the context's stream; the parameters have passed temporal_check_params
static int temporal_launch(tirt_ctx *c, const float *hdr_c, const float *aov_c, const float *mom_c, const float *hdr_h, const float *aov_h, const float *mom_h,
                           const tirt_temporal_camera_t &cur, const tirt_temporal_camera_t &prev, float *hdr_o, float *mom_o, int W, int H,
                           const tirt_temporal_t &prm, const float *motion = nullptr)
{
    CameraView cv;
    memcpy(cv.view_inv, cur.view_inv, sizeof(float) * 12);
    memcpy(cv.eye, cur.eye, sizeof(float) * 3);
    cv.fx = cur.fx; cv.fy = cur.fy; cv.cx = cur.cx; cv.cy = cur.cy;
    TemporalPrev pv;
    memcpy(pv.view, prev.view, sizeof(float) * 12);
    memcpy(pv.eye, prev.eye, sizeof(float) * 3);
    pv.fx = prev.fx; pv.fy = prev.fy; pv.cx = prev.cx; pv.cy = prev.cy;
    const TemporalParams kp = {prm.max_history, prm.sigma_n * prm.sigma_n, prm.sigma_z};
    const int NP = W * H, B = 256;
    const dim3 G((unsigned)((NP + B - 1) / B));
    if (motion)
        hipLaunchKernelGGL(k_temporal<true>, G, dim3(B), 0, c->stream, hdr_c, (const float4 *)aov_c, (const float4 *)mom_c, hdr_h, (const float4 *)aov_h,
                           (const float4 *)mom_h, hdr_o, (float4 *)mom_o, W, H, NP, cv, pv, kp, (const float4 *)motion);
    else
        hipLaunchKernelGGL(k_temporal<false>, G, dim3(B), 0, c->stream, hdr_c, (const float4 *)aov_c, (const float4 *)mom_c, hdr_h, (const float4 *)aov_h,
                           (const float4 *)mom_h, hdr_o, (float4 *)mom_o, W, H, NP, cv, pv, kp, (const float4 *)nullptr);
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int temporal_device(tirt_ctx *c, const float *hdr_c, const float *aov_c, const float *mom_c, const float *hdr_h, const float *aov_h, const float *mom_h,
                    const tirt_temporal_camera_t *cur, const tirt_temporal_camera_t *prev, float *hdr_o, float *mom_o, int W, int H,
                    const tirt_temporal_t *prm, const float *motion, void *stream)
{
    const std::string fn = motion ? "tirt_motion_temporal_device" : "tirt_temporal_device";      // (a null motion array: tirt_motion_temporal_device has refused it)
    TIRT_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 30), fn + ": bad size");
    if (int rc = temporal_check_params(fn, prm)) return rc;
    TIRT_REQUIRE(cur && prev, fn + ": null camera");
    if (int rc = require_caller_stream(c, fn, stream, "the accumulation")) return rc;
    const size_t NP = (size_t)W * H;
    const int NA = motion ? 9 : 8;                         // the outputs are a[6] and a[7]
    const struct { const char *name; const void *p; size_t words; bool out; } a[9] = {
        {"hdr_c", hdr_c, 3, false}, {"aov_c", aov_c, TIRT_AOV_WORDS, false}, {"mom_c", mom_c, TIRT_MOM_WORDS, false},
        {"hdr_h", hdr_h, 3, false}, {"aov_h", aov_h, TIRT_AOV_WORDS, false}, {"mom_h", mom_h, TIRT_MOM_WORDS, false},
        {"hdr_o", hdr_o, 3, true}, {"mom_o", mom_o, TIRT_MOM_WORDS, true}, {"motion", motion, TIRT_MOTION_WORDS, false}};
    bool null = false, overlap = false, aligned = true;
    for (int k = 0; k < NA; k++) {
        null = null || !a[k].p;
        aligned = aligned && (a[k].words == 3 || ((uintptr_t)a[k].p & 15) == 0);      // the records go as float4, hdr word by word
    }
    for (int o = 6; o < 8; o++)
        for (int k = 0; k < NA; k++) {
            if (k == o) continue;
            const uintptr_t o0 = (uintptr_t)a[o].p, o1 = o0 + sizeof(float) * a[o].words * NP, b0 = (uintptr_t)a[k].p, b1 = b0 + sizeof(float) * a[k].words * NP;
            overlap = overlap || !(o1 <= b0 || b1 <= o0);
        }
    TIRT_REQUIRE(!null, fn + ": null pointer");
    for (int k = 0; k < NA; k++)
        if (int rc = require_device_ptr(c, a[k].p, (fn + ": " + a[k].name).c_str())) return rc;
    TIRT_REQUIRE(!overlap, fn + ": an output overlaps an input or the other output");
    TIRT_REQUIRE(aligned, fn + ": the feature and moment arrays" + (motion ? " and the motion records" : "") + " must be 16-byte aligned");
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = temporal_launch(c, hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, *cur, *prev, hdr_o, mom_o, W, H, *prm, motion)) return rc;
    return query_end(c, stream);
}

// ---- the context's own history: two sets of {aov 8, mom 8, hdr 3} f32 per pixel in tp_mem, the records first so that they are 16-byte aligned ----
namespace {
struct TemporalSet { float *aov, *mom, *hdr; };
size_t temporal_set_bytes(const tirt_ctx *c) { return ((sizeof(float) * 19 * (size_t)c->W * c->H) + 15) & ~(size_t)15; }
TemporalSet temporal_set(const tirt_ctx *c, int k)
{
    const size_t NP = (size_t)c->W * c->H;
    float *base = (float *)(c->tp_mem.as<char>() + (size_t)k * temporal_set_bytes(c));
    return TemporalSet{base, base + 8 * NP, base + 16 * NP};
}
}  // namespace

// the entry points of tirt_api.hip have flushed, and ordered the main stream after the last film and record update where the records are read
int temporal_enable(tirt_ctx *c, int on)
{
    const std::string fn = "tirt_temporal_enable";
    TIRT_REQUIRE(c->hdr.p, fn + ": film not created");
    TIRT_REQUIRE(on || !c->mv_rec.p, fn + ": motion records are on and need the history (tirt_motion_enable(0) first)");
    if (sync_all(c)) return TIRT_ERR_HIP;
    c->tp_valid = false; c->mv_moved = false;
    if (!on) { c->tp_mem.release(); return TIRT_OK; }
    TIRT_REQUIRE(c->aov.p, fn + ": feature buffers not enabled (tirt_aov_enable)");
    TIRT_REQUIRE(c->mom.p, fn + ": moment buffers not enabled (tirt_moments_enable)");
    TIRT_REQUIRE(c->tile_count == 1, fn + ": tile_count > 1 -- this context's film is partial: reduce the films and the records, then tirt_temporal_device");
    if (c->tp_mem.ensure(2 * temporal_set_bytes(c))) return TIRT_ERR_HIP;
    c->tp_cur = 0;
    return TIRT_OK;
}

static size_t motion_bytes(const tirt_ctx *c) { return sizeof(float) * TIRT_MOTION_WORDS * (size_t)c->W * c->H; }

int motion_enable(tirt_ctx *c, int on)
{
    const std::string fn = "tirt_motion_enable";
    TIRT_REQUIRE(c->hdr.p, fn + ": film not created");
    TIRT_REQUIRE(!on || c->tp_mem.p, fn + ": temporal accumulation not enabled (tirt_temporal_enable)");
    if (sync_all(c)) return TIRT_ERR_HIP;
    if (!on) {
        if (c->mv_moved) c->tp_valid = false;              // the history is of geometry that has moved since, and nothing says how any more
        c->mv_rec.release(); c->mv_snap.release();
        c->mv_moved = false; c->mv_rec_valid = false;
        return TIRT_OK;
    }
    if (c->mv_rec.p) return TIRT_OK;                       // already on: the snapshot and its flag stay
    if (c->mv_rec.ensure(motion_bytes(c))) return TIRT_ERR_HIP;
    c->mv_moved = false; c->mv_rec_valid = false;
    return TIRT_OK;
}

// generate, trace, resolve: the record of every pixel into c->mv_rec, on the main stream (the caller has checked the build and the camera)
static int motion_resolve(tirt_ctx *c)
{
    DebugRays r;
    if (int rc = debug_trace(c, 0, 0, 64, 0, r)) return rc;
    const int P = (int)c->npix_local, B = 256;
    hipLaunchKernelGGL(k_motion_resolve, dim3((unsigned)((P + B - 1) / B)), dim3(B), 0, c->stream, (const float *)c->vertex.as<float>(),
                       (const float *)c->mv_snap.as<float>(), (const int *)c->primitive.as<int>(), r.tm, P, (const float4 *)r.hit, c->mv_rec.as<float4>());
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int motion_copy_out(tirt_ctx *c, const char *fn, void *dst, hipMemcpyKind kind)
{
    TIRT_REQUIRE(c->mv_rec.p, std::string(fn) + ": motion records not enabled (tirt_motion_enable)");
    TIRT_REQUIRE(c->tp_valid && c->mv_rec_valid, std::string(fn) + ": nothing accumulated yet (tirt_temporal_accumulate)");
    TIRT_REQUIRE(dst, std::string(fn) + ": null pointer");
    TIRT_HIP(hipMemcpyAsync(dst, c->mv_rec.p, motion_bytes(c), kind, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int temporal_accumulate(tirt_ctx *c, const tirt_temporal_t *prm)
{
    const std::string fn = "tirt_temporal_accumulate";
    TIRT_REQUIRE(c->tp_mem.p, fn + ": temporal accumulation not enabled (tirt_temporal_enable)");
    TIRT_REQUIRE(c->cam_set, fn + ": camera not set");
    if (int rc = temporal_check_params(fn, prm)) return rc;
    const bool moved = c->mv_rec.p && c->tp_valid && c->mv_moved;      // geometry updates since the last accumulate: through the motion records
    TIRT_REQUIRE(!moved || c->built, fn + ": LBVH not built (tirt_lbvh_build must follow the vertex update)");
    tirt_temporal_camera_t cur;
    memcpy(cur.view, c->view, sizeof(float) * 16);
    memset(cur.view_inv, 0, sizeof(cur.view_inv));
    memcpy(cur.view_inv, c->cam.view_inv, sizeof(float) * 12);
    cur.view_inv[15] = 1.0f;
    memcpy(cur.eye, c->cam.eye, sizeof(float) * 3);
    cur.fx = c->cam.fx; cur.fy = c->cam.fy; cur.cx = c->cam.cx; cur.cy = c->cam.cy;
    const size_t NP = (size_t)c->W * c->H;
    const TemporalSet h = temporal_set(c, c->tp_cur), o = temporal_set(c, c->tp_cur ^ 1);
    if (moved) { if (int rc = motion_resolve(c)) return rc; }
    else if (c->mv_rec.p) TIRT_HIP(hipMemsetAsync(c->mv_rec.p, 0, motion_bytes(c), c->stream));      // nothing moved: the records say so
    if (c->tp_valid) {
        if (int rc = temporal_launch(c, c->hdr.as<float>(), c->aov.as<float>(), c->mom.as<float>(), h.hdr, h.aov, h.mom, cur, c->tp_cam, o.hdr, o.mom,
                                     c->W, c->H, *prm, moved ? c->mv_rec.as<float>() : nullptr)) return rc;
    } else {                                                // an empty history: the current film and records as they are
        TIRT_HIP(hipMemcpyAsync(o.hdr, c->hdr.p, sizeof(float) * 3 * NP, hipMemcpyDeviceToDevice, c->stream));
        TIRT_HIP(hipMemcpyAsync(o.mom, c->mom.p, sizeof(float) * TIRT_MOM_WORDS * NP, hipMemcpyDeviceToDevice, c->stream));
    }
    TIRT_HIP(hipMemcpyAsync(o.aov, c->aov.p, sizeof(float) * TIRT_AOV_WORDS * NP, hipMemcpyDeviceToDevice, c->stream));
    c->tp_cam = cur;
    c->tp_cur ^= 1;
    c->tp_valid = true;
    c->mv_moved = false; c->mv_rec_valid = c->mv_rec.p != nullptr;
    return TIRT_OK;
}

int temporal_copy_out(tirt_ctx *c, const char *fn, void *hdr_dst, void *mom_dst, hipMemcpyKind kind)
{
    TIRT_REQUIRE(c->tp_mem.p, std::string(fn) + ": temporal accumulation not enabled (tirt_temporal_enable)");
    TIRT_REQUIRE(c->tp_valid, std::string(fn) + ": nothing accumulated yet (tirt_temporal_accumulate)");
    const size_t NP = (size_t)c->W * c->H;
    const TemporalSet s = temporal_set(c, c->tp_cur);
    if (hdr_dst) TIRT_HIP(hipMemcpyAsync(hdr_dst, s.hdr, sizeof(float) * 3 * NP, kind, c->stream));
    if (mom_dst) TIRT_HIP(hipMemcpyAsync(mom_dst, s.mom, sizeof(float) * TIRT_MOM_WORDS * NP, kind, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

int temporal_denoise_var(tirt_ctx *c, const tirt_denoise_var_t *prm)
{
    const std::string fn = "tirt_temporal_denoise_var";
    TIRT_REQUIRE(c->tp_mem.p, fn + ": temporal accumulation not enabled (tirt_temporal_enable)");
    TIRT_REQUIRE(c->tp_valid, fn + ": nothing accumulated yet (tirt_temporal_accumulate)");
    const TemporalSet s = temporal_set(c, c->tp_cur);
    return denoise_into_film_buffer(c, fn, s.hdr, s.aov, s.mom, prm);
}

}  // namespace tirt
