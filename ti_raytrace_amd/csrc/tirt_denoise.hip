// tirt_denoise.hip -- edge-avoiding a-trous wavelet denoiser over the film and its feature buffers (tirt_denoise / tirt_denoise_device), and its
// variance-guided mode (tirt_denoise_var / tirt_denoise_var_device).
//
// No reference counterpart.  The filter is the joint-bilateral a-trous wavelet of Dammertz, Sewtz, Hanika and Lensch, "Edge-Avoiding A-Trous
// Wavelet Transform for fast Global Illumination Filtering" (HPG 2010), guided by the first-hit normal and depth of the feature buffers
// (tirt_aov.hip) and run on albedo-demodulated radiance.  include/tirt.h states the arithmetic; tests/denoise_expected.py restates it in numpy
// and the device has to give its bits, so every operation below is one f32 rounding in the order written there (-ffp-contract=off).
//
// The variance-guided mode (VAR; tests/denoise_var_expected.py) is SVGF's a-trous (Schied et al., "Spatiotemporal Variance-Guided Filtering",
// HPG 2017) without its temporal part, steered by the sample moments of tirt_moments.hip: the colour edge-stopping term is scaled by the pixel's
// own variance of the mean s, and that variance is filtered along with the colour.  Both modes are one set of kernels over the same scratch; the
// fourth words of the two records differ (below), because computing rz per pixel and level cost the plain filter 0.5-1 % (profiles/denoise_rate.txt).
//
// Pixel p = i * H + j as hdr; one thread per pixel with the lanes along j, the contiguous axis, so a wave's 25 taps are 25 contiguous runs.
//
//   k_dn_prepare<false>         hdr, feature record                -> A0[p] = (e.rgb, z), G[p] = (n.xyz, rz), D[p] = d.rgb     (e = hdr / d)
//   k_dn_prepare<true>          hdr, feature record, moment record -> A0[p] = (e.rgb, s), G[p] = (n.xyz, z),  D[p] = d.rgb
//   k_dn_prefilter              VAR only.  A0 -> A1: s smoothed once over 3 x 3 (SVGF's variance prefilter), e copied
//   k_dn_atrous<VAR, false> x l A[cur] -> A[1 - cur], taps `step` = 1 << l apart (one launch per level, ping-pong; VAR starts from the prefiltered A1);
//                               plain: z rides along in A and rz is loaded; VAR: s' is written and rz is computed for the centre pixel
//   k_dn_atrous<VAR, true>      the last level: the same taps, then out[p] = e' * d, stored non-temporally     (the remodulation fused: same bits)
//
// A tap is two 16-byte loads.  At 1024^2 the three records are 48 MB, which the L2s and the Infinity Cache hold between the levels; for
// step >= 4 the taps of a block lie further apart than any LDS tile reaches, so there is no LDS variant (none was built or measured).
// The weight goes through tm_exp (tirt_math.h, a double-precision core): 25 of them per pixel and level are what the kernel computes.
//
// s is "known" when 0 <= s < inf; anything else (prepare writes -1 for a pixel with fewer than two samples, or whose record gives no such number)
// switches the colour term off for that pixel and is skipped wherever variances are summed: no weight becomes NaN because of it.
#include "tirt_internal.h"

namespace tirt {

TD bool dn_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // false for NaN
TD bool dn_known(float s) { return s >= 0.0f && s < __builtin_inff(); }           // false for NaN, for the -1 of "no variance" and for an overflowed sum

// `mom` is read only under VAR.
template <bool VAR>
__global__ __launch_bounds__(256) void k_dn_prepare(const float *hdr, const float *aov, const float *mom, int NP, float4 *A, float4 *G, float *D)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const float4 lo = ((const float4 *)aov)[2 * (size_t)p], hi = ((const float4 *)aov)[2 * (size_t)p + 1];
    const float z = hi.z, al = hi.w;
    const float miss = 1.0f - al;                         // the missed share of a pixel counts as albedo 1
    const float d0 = __builtin_fmaxf(lo.x + miss, 1e-3f), d1 = __builtin_fmaxf(lo.y + miss, 1e-3f), d2 = __builtin_fmaxf(lo.z + miss, 1e-3f);
    const float *h = hdr + 3 * (size_t)p;
    float s = -1.0f;
    if constexpr (VAR) {
        const float4 m0 = ((const float4 *)mom)[2 * (size_t)p], m1 = ((const float4 *)mom)[2 * (size_t)p + 1];
        const float n = m0.x;
        if (n >= 2.0f) {
            const float nn = n * (n - 1.0f);
            const float v0 = m1.x / nn, v1 = m1.y / nn, v2 = m1.z / nn;
            const float t = (v0 / (d0 * d0) + v1 / (d1 * d1)) + v2 / (d2 * d2);
            if (dn_known(t)) s = t;
        }
    }
    if constexpr (VAR) {
        A[p] = make_float4(h[0] / d0, h[1] / d1, h[2] / d2, s);
        G[p] = make_float4(lo.w, hi.x, hi.y, z);
    } else {
        A[p] = make_float4(h[0] / d0, h[1] / d1, h[2] / d2, z);
        G[p] = make_float4(lo.w, hi.x, hi.y, 1.0f / __builtin_fmaxf(z * z, 1e-12f));
    }
    float *d = D + 3 * (size_t)p;
    d[0] = d0; d[1] = d1; d[2] = d2;
}

__global__ __launch_bounds__(256) void k_dn_prefilter(const float4 *__restrict__ src, float4 *__restrict__ dst, int W, int H, int NP)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const int i = p / H, j = p - i * H;
    float4 ep = src[p];
    if (dn_known(ep.w)) {
        const float hk[2] = {0.5f, 0.25f};
        float ss = 0.0f, sk = 0.0f;
#pragma unroll
        for (int di = -1; di <= 1; di++) {
            const int qi = i + di;
            if (qi < 0 || qi >= W) continue;
#pragma unroll
            for (int dj = -1; dj <= 1; dj++) {
                const int qj = j + dj;
                if (qj < 0 || qj >= H) continue;
                const float sq = src[qi * H + qj].w;
                const float k = hk[di < 0 ? -di : di] * hk[dj < 0 ? -dj : dj];
                if (dn_known(sq)) { ss += k * sq; sk += k; }
            }
        }
        ep.w = ss / sk;                                   // (the centre tap is known: sk >= 0.25)
    }
    dst[p] = ep;
}

// One level.  LAST: the remodulated pixel goes to `out` (W*H*3) instead of the record to `dst`.  cw weighs the colour term: plain mode multiplies
// by it (1 / sigma_c^2 of this level), VAR divides by cw * s_p + 1e-12 (cw = sigma_c^2) where s_p is known and drops the term where it is not.
template <bool VAR, bool LAST>
__global__ __launch_bounds__(256) void k_dn_atrous(const float4 *__restrict__ src, const float4 *__restrict__ G, const float *__restrict__ D,
                                                   float4 *__restrict__ dst, float *__restrict__ out, int W, int H, int NP, int step,
                                                   float cw, float in, float iz)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const int i = p / H, j = p - i * H;
    const float4 ep = src[p], gp = G[p];
    const float rz = VAR ? 1.0f / __builtin_fmaxf(gp.w * gp.w, 1e-12f) : gp.w;
    const bool colour = VAR && dn_known(ep.w);
    const float cden = cw * ep.w + 1e-12f;                // (VAR only)
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sw = 0.0f, sv = 0.0f, swv = 0.0f;
    const float hk[3] = {0.375f, 0.25f, 0.0625f};
#pragma unroll
    for (int di = -2; di <= 2; di++) {
        const int qi = i + di * step;
        if (qi < 0 || qi >= W) continue;
#pragma unroll
        for (int dj = -2; dj <= 2; dj++) {
            const int qj = j + dj * step;
            if (qj < 0 || qj >= H) continue;
            const int q = qi * H + qj;
            const float4 eq = src[q], gq = G[q];
            const float k = hk[di < 0 ? -di : di] * hk[dj < 0 ? -dj : dj];
            const float c0 = ep.x - eq.x, c1 = ep.y - eq.y, c2 = ep.z - eq.z;
            const float dc = (c0 * c0 + c1 * c1) + c2 * c2;
            const float n0 = gp.x - gq.x, n1 = gp.y - gq.y, n2 = gp.z - gq.z;
            const float dn = (n0 * n0 + n1 * n1) + n2 * n2;
            const float zd = VAR ? gp.w - gq.w : ep.w - eq.w;
            const float dz = (zd * zd) * rz;
            float xc;
            if constexpr (VAR) xc = colour ? dc / cden : 0.0f;
            else xc = dc * cw;
            const float x = (xc + dn * in) + dz * iz;
            const float w = k * tm_exp(-x);
            if (dn_finite(w) && dn_finite(eq.x) && dn_finite(eq.y) && dn_finite(eq.z)) {
                s0 += eq.x * w; s1 += eq.y * w; s2 += eq.z * w; sw += w;
                if constexpr (VAR) {
                    if (dn_known(eq.w)) { sv += (w * w) * eq.w; swv += w; }
                }
            }
        }
    }
    float r0 = s0 / sw, r1 = s1 / sw, r2 = s2 / sw;
    if (!(dn_finite(ep.x) && dn_finite(ep.y) && dn_finite(ep.z))) { r0 = ep.x; r1 = ep.y; r2 = ep.z; }      // the film's NaN pixels stay as they are
    if constexpr (LAST) {
        const float *d = D + 3 * (size_t)p;
        float *o = out + 3 * (size_t)p;
        __builtin_nontemporal_store(r0 * d[0], &o[0]);
        __builtin_nontemporal_store(r1 * d[1], &o[1]);
        __builtin_nontemporal_store(r2 * d[2], &o[2]);
    } else {
        const float sn = (colour && swv > 0.0f) ? sv / (swv * swv) : ep.w;      // (plain: z rides along)
        dst[p] = make_float4(r0, r1, r2, sn);
    }
}

static const tirt_denoise_t DN_DEFAULTS = {5, 1.0f, 0.3f, 0.1f}, DNV_DEFAULTS = {5, TIRT_DENOISE_VAR_SIGMA_C, 0.3f, 0.1f};

static int denoise_check_params(const std::string &fn, const tirt_denoise_t *&prm, const tirt_denoise_t &defaults)
{
    if (!prm) prm = &defaults;
    TIRT_REQUIRE(prm->levels >= 1 && prm->levels <= 8, fn + ": levels 1..8");
    const float s[3] = {prm->sigma_c, prm->sigma_n, prm->sigma_z};
    for (float v : s) TIRT_REQUIRE(v > 0.0f && v < __builtin_inff(), fn + ": sigma_c, sigma_n and sigma_z must be finite and > 0");
    return TIRT_OK;
}

// Scratch of W*H pixels: A0, A1, G (16 B each), D (12 B).  Growing the buffer waits for the work queued on the context's stream, which may
// still read the old one.
static int denoise_prepare(tirt_ctx *c, size_t NP)
{
    const size_t bytes = NP * 60;
    if (bytes > c->dn_mem.bytes) {
        TIRT_HIP(hipStreamSynchronize(c->stream));
        if (c->dn_mem.ensure(bytes)) return TIRT_ERR_HIP;
    }
    return TIRT_OK;
}

// prepare, (the prefilter,) the levels, the remodulation: all on the context's stream.  mom != nullptr selects the variance-guided mode.  The
// parameters have passed denoise_check_params.
static int denoise_launch(tirt_ctx *c, const float *hdr, const float *aov, const float *mom, float *out, int W, int H, const tirt_denoise_t &prm)
{
    const bool var = mom != nullptr;
    const int NP = W * H, B = 256;
    const dim3 g((unsigned)((NP + B - 1) / B));
    float4 *A[2] = {c->dn_mem.as<float4>(), c->dn_mem.as<float4>() + (size_t)NP};
    float4 *G = A[1] + (size_t)NP;
    float *D = (float *)(G + (size_t)NP);
    hipLaunchKernelGGL(var ? k_dn_prepare<true> : k_dn_prepare<false>, g, dim3(B), 0, c->stream, hdr, aov, mom, NP, A[0], G, D);
    if (var) hipLaunchKernelGGL(k_dn_prefilter, g, dim3(B), 0, c->stream, (const float4 *)A[0], A[1], W, H, NP);
    const int first = var ? 1 : 0;                          // level 0 reads the prefiltered A1
    const float in = 1.0f / (prm.sigma_n * prm.sigma_n), iz = 1.0f / (prm.sigma_z * prm.sigma_z);
    for (int l = 0; l < prm.levels; l++) {
        const float s = ldexpf(prm.sigma_c, -l);            // sigma_c * 2^-l, exact
        const float cw = var ? prm.sigma_c * prm.sigma_c : 1.0f / (s * s);
        const bool last = l + 1 == prm.levels;
        hipLaunchKernelGGL(var ? (last ? k_dn_atrous<true, true> : k_dn_atrous<true, false>) : (last ? k_dn_atrous<false, true> : k_dn_atrous<false, false>),
                           g, dim3(B), 0, c->stream, (const float4 *)A[(l + first) & 1], (const float4 *)G, (const float *)D, A[(l + first + 1) & 1], out,
                           W, H, NP, 1 << l, cw, in, iz);
    }
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

// tirt_denoise / tirt_denoise_var: the context's film and records into the context's own buffer.  The caller (tirt_api.hip) has ordered the stream
// after the last film update (which covers the moments) and the last k_aov.
int denoise_film(tirt_ctx *c, const tirt_denoise_t *prm, bool var)
{
    const std::string fn = var ? "tirt_denoise_var" : "tirt_denoise";
    TIRT_REQUIRE(c->hdr.p, fn + ": film not created");
    TIRT_REQUIRE(c->aov.p, fn + ": feature buffers not enabled (tirt_aov_enable)");
    if (var) TIRT_REQUIRE(c->mom.p, fn + ": moment buffers not enabled (tirt_moments_enable)");
    TIRT_REQUIRE(c->tile_count == 1, fn + ": tile_count > 1 -- this context's film is partial: reduce the films and the records, then " + fn + "_device");
    return denoise_into_film_buffer(c, fn, c->hdr.as<float>(), c->aov.as<float>(), var ? c->mom.as<float>() : nullptr, prm);
}

// Context-owned arrays of the film's size (the film and its records, or the temporal history of tirt_temporal.hip) into the context's own buffer;
// mom != nullptr selects the variance-guided mode.
int denoise_into_film_buffer(tirt_ctx *c, const std::string &fn, const float *hdr, const float *aov, const float *mom, const tirt_denoise_t *prm)
{
    if (int rc = denoise_check_params(fn, prm, mom ? DNV_DEFAULTS : DN_DEFAULTS)) return rc;
    const size_t NP = (size_t)c->W * c->H;
    if (int rc = denoise_prepare(c, NP)) return rc;
    if (c->dn_out.ensure(sizeof(float) * 3 * NP)) return TIRT_ERR_HIP;      // (allocates once per film: tirt_film_create drops it)
    return denoise_launch(c, hdr, aov, mom, c->dn_out.as<float>(), c->W, c->H, *prm);
}

// tirt_denoise_device / tirt_denoise_var_device.  `var` and not `mom` says which: a null mom in the variance-guided mode is refused like any other.
int denoise_device(tirt_ctx *c, bool var, const float *hdr, const float *aov, const float *mom, float *out, int W, int H, const tirt_denoise_t *prm, void *stream)
{
    const std::string fn = var ? "tirt_denoise_var_device" : "tirt_denoise_device";
    TIRT_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 30), fn + ": bad size");
    if (int rc = denoise_check_params(fn, prm, var ? DNV_DEFAULTS : DN_DEFAULTS)) return rc;
    if (int rc = require_caller_stream(c, fn, stream, "the filter")) return rc;
    const struct { const char *name; const float *p; size_t words; } in[3] = {{"hdr", hdr, 3}, {"aov", aov, TIRT_AOV_WORDS}, {"mom", mom, TIRT_MOM_WORDS}};
    const int nin = var ? 3 : 2;
    const size_t NP = (size_t)W * H;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + sizeof(float) * 3 * NP;
    bool null = !out, overlap = false, aligned = true;
    for (int k = 0; k < nin; k++) {
        const uintptr_t b0 = (uintptr_t)in[k].p, b1 = b0 + sizeof(float) * in[k].words * NP;
        null = null || !in[k].p;
        overlap = overlap || !(o1 <= b0 || b1 <= o0);
        aligned = aligned && (k == 0 || (b0 & 15) == 0);    // prepare reads the records, not hdr, as float4
    }
    TIRT_REQUIRE(!null, fn + ": null pointer");
    for (int k = 0; k < nin; k++)
        if (int rc = require_device_ptr(c, in[k].p, (fn + ": " + in[k].name).c_str())) return rc;
    if (int rc = require_device_ptr(c, out, (fn + ": out").c_str())) return rc;
    TIRT_REQUIRE(!overlap, fn + (var ? ": out overlaps hdr, aov or mom" : ": out overlaps hdr or aov"));
    TIRT_REQUIRE(aligned, fn + (var ? ": aov and mom" : ": aov") + " must be 16-byte aligned");
    if (int rc = denoise_prepare(c, NP)) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = denoise_launch(c, hdr, aov, var ? mom : nullptr, out, W, H, *prm)) return rc;
    return query_end(c, stream);
}

}  // namespace tirt
