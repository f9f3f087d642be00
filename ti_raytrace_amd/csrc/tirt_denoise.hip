// tirt_denoise.hip -- edge-avoiding a-trous wavelet denoiser over the film and its feature buffers (tirt_denoise / tirt_denoise_device).
//
// No reference counterpart.  The filter is the joint-bilateral a-trous wavelet of Dammertz, Sewtz, Hanika and Lensch, "Edge-Avoiding A-Trous
// Wavelet Transform for fast Global Illumination Filtering" (HPG 2010), guided by the first-hit normal and depth of the feature buffers
// (tirt_aov.hip) and run on albedo-demodulated radiance.  include/tirt.h states the arithmetic; tests/denoise_expected.py restates it in numpy
// and the device has to give its bits, so every operation below is one f32 rounding in the order written there (-ffp-contract=off).
//
// Pixel p = i * H + j as hdr; one thread per pixel with the lanes along j, the contiguous axis, so a wave's 25 taps are 25 contiguous runs.
//
//   k_dn_prepare            hdr, feature record -> A0[p] = (e.rgb, z), G[p] = (n.xyz, rz), D[p] = d.rgb       (e = hdr / d)
//   k_dn_atrous<false> x l  A[cur] -> A[1 - cur], taps `step` = 1 << l apart; z rides along                   (one launch per level, ping-pong)
//   k_dn_atrous<true>       the last level: the same taps, then out[p] = e' * d, stored non-temporally        (the remodulation fused: same bits)
//
// A tap is two 16-byte loads.  At 1024^2 the three records are 48 MB, which the L2s and the Infinity Cache hold between the levels; for
// step >= 4 the taps of a block lie further apart than any LDS tile reaches, so there is no LDS variant (none was built or measured).
// The weight goes through tm_exp (tirt_math.h, a double-precision core): 25 of them per pixel and level are what the kernel computes.
//
// The variance-guided mode (tirt_denoise_var / tirt_denoise_var_device; tests/denoise_var_expected.py) is SVGF's a-trous (Schied et al., "Spatiotemporal
// Variance-Guided Filtering", HPG 2017) without its temporal part, steered by the sample moments of tirt_moments.hip: the colour edge-stopping term is
// scaled by the pixel's own variance of the mean, and that variance is filtered along with the colour.  Same scratch, other packing -- a tap is still two
// 16-byte loads:
//
//   k_dnv_prepare            hdr, feature record, moment record -> A0[p] = (e.rgb, s), G[p] = (n.xyz, z), D[p] = d.rgb
//   k_dnv_prefilter          A0 -> A1: s smoothed once over 3 x 3 (SVGF's variance prefilter), e copied
//   k_dnv_atrous<false> x l  A[cur] -> A[1 - cur] starting from A1; rz is computed for the centre pixel
//   k_dnv_atrous<true>       the last level with the remodulation
//
// s is "known" when 0 <= s < inf; anything else (prepare writes -1 for a pixel with fewer than two samples, or whose record gives no such number)
// switches the colour term off for that pixel and is skipped wherever variances are summed: no weight becomes NaN because of it.
#include "tirt_internal.h"

namespace tirt {

TD bool dn_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // false for NaN

__global__ __launch_bounds__(256) void k_dn_prepare(const float *hdr, const float *aov, int NP, float4 *A, float4 *G, float *D)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const float4 lo = ((const float4 *)aov)[2 * (size_t)p], hi = ((const float4 *)aov)[2 * (size_t)p + 1];
    const float z = hi.z, al = hi.w;
    const float miss = 1.0f - al;                         // the missed share of a pixel counts as albedo 1
    const float d0 = __builtin_fmaxf(lo.x + miss, 1e-3f), d1 = __builtin_fmaxf(lo.y + miss, 1e-3f), d2 = __builtin_fmaxf(lo.z + miss, 1e-3f);
    const float *h = hdr + 3 * (size_t)p;
    A[p] = make_float4(h[0] / d0, h[1] / d1, h[2] / d2, z);
    G[p] = make_float4(lo.w, hi.x, hi.y, 1.0f / __builtin_fmaxf(z * z, 1e-12f));
    float *d = D + 3 * (size_t)p;
    d[0] = d0; d[1] = d1; d[2] = d2;
}

// One level.  LAST: the remodulated pixel goes to `out` (W*H*3) instead of the record to `dst`.
template <bool LAST>
__global__ __launch_bounds__(256) void k_dn_atrous(const float4 *__restrict__ src, const float4 *__restrict__ G, const float *__restrict__ D,
                                                   float4 *__restrict__ dst, float *__restrict__ out, int W, int H, int NP, int step,
                                                   float ic, float in, float iz)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const int i = p / H, j = p - i * H;
    const float4 ep = src[p], gp = G[p];
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
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
            const float zd = ep.w - eq.w;
            const float dz = (zd * zd) * gp.w;
            const float x = (dc * ic + dn * in) + dz * iz;
            const float w = k * tm_exp(-x);
            if (dn_finite(w) && dn_finite(eq.x) && dn_finite(eq.y) && dn_finite(eq.z)) {
                s0 += eq.x * w; s1 += eq.y * w; s2 += eq.z * w; sw += w;
            }
        }
    }
    float r0 = s0 / sw, r1 = s1 / sw, r2 = s2 / sw;
    if (!(dn_finite(ep.x) && dn_finite(ep.y) && dn_finite(ep.z))) { r0 = ep.x; r1 = ep.y; r2 = ep.z; }      // the film's NaN pixels stay as they are
    if (LAST) {
        const float *d = D + 3 * (size_t)p;
        float *o = out + 3 * (size_t)p;
        __builtin_nontemporal_store(r0 * d[0], &o[0]);
        __builtin_nontemporal_store(r1 * d[1], &o[1]);
        __builtin_nontemporal_store(r2 * d[2], &o[2]);
    } else {
        dst[p] = make_float4(r0, r1, r2, ep.w);
    }
}

static const tirt_denoise_t DN_DEFAULTS = {5, 1.0f, 0.3f, 0.1f};

static int denoise_check_params(const char *fn, const tirt_denoise_t *&prm)
{
    if (!prm) prm = &DN_DEFAULTS;
    TIRT_REQUIRE(prm->levels >= 1 && prm->levels <= 8, std::string(fn) + ": levels 1..8");
    const float s[3] = {prm->sigma_c, prm->sigma_n, prm->sigma_z};
    for (float v : s) TIRT_REQUIRE(v > 0.0f && v < __builtin_inff(), std::string(fn) + ": sigma_c, sigma_n and sigma_z must be finite and > 0");
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

// prepare, the levels, the remodulation: all on the context's stream.  The parameters have passed denoise_check_params.
static int denoise_launch(tirt_ctx *c, const float *hdr, const float *aov, float *out, int W, int H, const tirt_denoise_t &prm)
{
    const int NP = W * H, B = 256;
    const dim3 g((unsigned)((NP + B - 1) / B));
    float4 *A[2] = {c->dn_mem.as<float4>(), c->dn_mem.as<float4>() + (size_t)NP};
    float4 *G = A[1] + (size_t)NP;
    float *D = (float *)(G + (size_t)NP);
    hipLaunchKernelGGL(k_dn_prepare, g, dim3(B), 0, c->stream, hdr, aov, NP, A[0], G, D);
    const float in = 1.0f / (prm.sigma_n * prm.sigma_n), iz = 1.0f / (prm.sigma_z * prm.sigma_z);
    for (int l = 0; l < prm.levels; l++) {
        const float s = ldexpf(prm.sigma_c, -l);            // sigma_c * 2^-l, exact
        const float ic = 1.0f / (s * s);
        const float4 *src = A[l & 1];
        if (l + 1 < prm.levels) hipLaunchKernelGGL(k_dn_atrous<false>, g, dim3(B), 0, c->stream, src, (const float4 *)G, (const float *)D, A[(l + 1) & 1], (float *)nullptr, W, H, NP, 1 << l, ic, in, iz);
        else hipLaunchKernelGGL(k_dn_atrous<true>, g, dim3(B), 0, c->stream, src, (const float4 *)G, (const float *)D, (float4 *)nullptr, out, W, H, NP, 1 << l, ic, in, iz);
    }
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

// tirt_denoise: the context's film and records into the context's own buffer.  The caller (tirt_api.hip) has ordered the stream after the
// last film update and the last k_aov.
int denoise_film(tirt_ctx *c, const tirt_denoise_t *prm)
{
    const char *fn = "tirt_denoise";
    TIRT_REQUIRE(c->hdr.p, "tirt_denoise: film not created");
    TIRT_REQUIRE(c->aov.p, "tirt_denoise: feature buffers not enabled (tirt_aov_enable)");
    TIRT_REQUIRE(c->tile_count == 1, "tirt_denoise: tile_count > 1 -- this context's film is partial: reduce the films and the records, then tirt_denoise_device");
    if (int rc = denoise_check_params(fn, prm)) return rc;
    const size_t NP = (size_t)c->W * c->H;
    if (int rc = denoise_prepare(c, NP)) return rc;
    if (c->dn_out.ensure(sizeof(float) * 3 * NP)) return TIRT_ERR_HIP;      // (allocates once per film: tirt_film_create drops it)
    return denoise_launch(c, c->hdr.as<float>(), c->aov.as<float>(), c->dn_out.as<float>(), c->W, c->H, *prm);
}

int denoise_device(tirt_ctx *c, const float *hdr, const float *aov, float *out, int W, int H, const tirt_denoise_t *prm, void *stream)
{
    const char *fn = "tirt_denoise_device";
    TIRT_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 30), "tirt_denoise_device: bad size");
    if (int rc = denoise_check_params(fn, prm)) return rc;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) {
        (void)hipGetLastError();
        set_error("tirt_denoise_device: the caller's stream is not a stream of this process's HIP runtime");
        return TIRT_ERR_ARG;
    }
    TIRT_REQUIRE(cs == hipStreamCaptureStatusNone, "tirt_denoise_device: the caller's stream is capturing a graph (the filter cannot be captured)");
    TIRT_REQUIRE(hdr && aov && out, "tirt_denoise_device: null pointer");
    if (int rc = require_device_ptr(c, hdr, "tirt_denoise_device: hdr")) return rc;
    if (int rc = require_device_ptr(c, aov, "tirt_denoise_device: aov")) return rc;
    if (int rc = require_device_ptr(c, out, "tirt_denoise_device: out")) return rc;
    const size_t NP = (size_t)W * H;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + sizeof(float) * 3 * NP, h0 = (uintptr_t)hdr, h1 = h0 + sizeof(float) * 3 * NP,
                    a0 = (uintptr_t)aov, a1 = a0 + sizeof(float) * TIRT_AOV_WORDS * NP;
    TIRT_REQUIRE((o1 <= h0 || h1 <= o0) && (o1 <= a0 || a1 <= o0), "tirt_denoise_device: out overlaps hdr or aov");
    TIRT_REQUIRE((a0 & 15) == 0, "tirt_denoise_device: aov must be 16-byte aligned");
    if (int rc = denoise_prepare(c, NP)) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = denoise_launch(c, hdr, aov, out, W, H, *prm)) return rc;
    return query_end(c, stream);
}

// ---- variance-guided mode ------------------------------------------------------------------------------------------------------------------

TD bool dnv_known(float s) { return s >= 0.0f && s < __builtin_inff(); }      // false for NaN, for the -1 of "no variance" and for an overflowed sum

__global__ __launch_bounds__(256) void k_dnv_prepare(const float *hdr, const float *aov, const float *mom, int NP, float4 *A, float4 *G, float *D)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const float4 lo = ((const float4 *)aov)[2 * (size_t)p], hi = ((const float4 *)aov)[2 * (size_t)p + 1];
    const float4 m0 = ((const float4 *)mom)[2 * (size_t)p], m1 = ((const float4 *)mom)[2 * (size_t)p + 1];
    const float z = hi.z, al = hi.w;
    const float miss = 1.0f - al;
    const float d0 = __builtin_fmaxf(lo.x + miss, 1e-3f), d1 = __builtin_fmaxf(lo.y + miss, 1e-3f), d2 = __builtin_fmaxf(lo.z + miss, 1e-3f);
    const float *h = hdr + 3 * (size_t)p;
    float s = -1.0f;
    const float n = m0.x;
    if (n >= 2.0f) {
        const float nn = n * (n - 1.0f);
        const float v0 = m1.x / nn, v1 = m1.y / nn, v2 = m1.z / nn;
        const float t = (v0 / (d0 * d0) + v1 / (d1 * d1)) + v2 / (d2 * d2);
        if (dnv_known(t)) s = t;
    }
    A[p] = make_float4(h[0] / d0, h[1] / d1, h[2] / d2, s);
    G[p] = make_float4(lo.w, hi.x, hi.y, z);
    float *d = D + 3 * (size_t)p;
    d[0] = d0; d[1] = d1; d[2] = d2;
}

__global__ __launch_bounds__(256) void k_dnv_prefilter(const float4 *__restrict__ src, float4 *__restrict__ dst, int W, int H, int NP)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const int i = p / H, j = p - i * H;
    float4 ep = src[p];
    if (dnv_known(ep.w)) {
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
                if (dnv_known(sq)) { ss += k * sq; sk += k; }
            }
        }
        ep.w = ss / sk;                                   // (the centre tap is known: sk >= 0.25)
    }
    dst[p] = ep;
}

template <bool LAST>
__global__ __launch_bounds__(256) void k_dnv_atrous(const float4 *__restrict__ src, const float4 *__restrict__ G, const float *__restrict__ D,
                                                    float4 *__restrict__ dst, float *__restrict__ out, int W, int H, int NP, int step,
                                                    float sc2, float in, float iz)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NP) return;
    const int i = p / H, j = p - i * H;
    const float4 ep = src[p], gp = G[p];
    const float rz = 1.0f / __builtin_fmaxf(gp.w * gp.w, 1e-12f);
    const bool colour = dnv_known(ep.w);
    const float cden = sc2 * ep.w + 1e-12f;
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
            const float zd = gp.w - gq.w;
            const float dz = (zd * zd) * rz;
            const float xc = colour ? dc / cden : 0.0f;
            const float x = (xc + dn * in) + dz * iz;
            const float w = k * tm_exp(-x);
            if (dn_finite(w) && dn_finite(eq.x) && dn_finite(eq.y) && dn_finite(eq.z)) {
                s0 += eq.x * w; s1 += eq.y * w; s2 += eq.z * w; sw += w;
                if (dnv_known(eq.w)) { sv += (w * w) * eq.w; swv += w; }
            }
        }
    }
    float r0 = s0 / sw, r1 = s1 / sw, r2 = s2 / sw;
    if (!(dn_finite(ep.x) && dn_finite(ep.y) && dn_finite(ep.z))) { r0 = ep.x; r1 = ep.y; r2 = ep.z; }
    if (LAST) {
        const float *d = D + 3 * (size_t)p;
        float *o = out + 3 * (size_t)p;
        __builtin_nontemporal_store(r0 * d[0], &o[0]);
        __builtin_nontemporal_store(r1 * d[1], &o[1]);
        __builtin_nontemporal_store(r2 * d[2], &o[2]);
    } else {
        const float sn = (colour && swv > 0.0f) ? sv / (swv * swv) : ep.w;
        dst[p] = make_float4(r0, r1, r2, sn);
    }
}

static const tirt_denoise_var_t DNV_DEFAULTS = {5, TIRT_DENOISE_VAR_SIGMA_C, 0.3f, 0.1f};

static int denoise_var_check_params(const char *fn, const tirt_denoise_var_t *&prm)
{
    if (!prm) prm = &DNV_DEFAULTS;
    TIRT_REQUIRE(prm->levels >= 1 && prm->levels <= 8, std::string(fn) + ": levels 1..8");
    const float s[3] = {prm->sigma_c, prm->sigma_n, prm->sigma_z};
    for (float v : s) TIRT_REQUIRE(v > 0.0f && v < __builtin_inff(), std::string(fn) + ": sigma_c, sigma_n and sigma_z must be finite and > 0");
    return TIRT_OK;
}

static int denoise_var_launch(tirt_ctx *c, const float *hdr, const float *aov, const float *mom, float *out, int W, int H, const tirt_denoise_var_t &prm)
{
    const int NP = W * H, B = 256;
    const dim3 g((unsigned)((NP + B - 1) / B));
    float4 *A[2] = {c->dn_mem.as<float4>(), c->dn_mem.as<float4>() + (size_t)NP};
    float4 *G = A[1] + (size_t)NP;
    float *D = (float *)(G + (size_t)NP);
    hipLaunchKernelGGL(k_dnv_prepare, g, dim3(B), 0, c->stream, hdr, aov, mom, NP, A[0], G, D);
    hipLaunchKernelGGL(k_dnv_prefilter, g, dim3(B), 0, c->stream, (const float4 *)A[0], A[1], W, H, NP);
    const float sc2 = prm.sigma_c * prm.sigma_c, in = 1.0f / (prm.sigma_n * prm.sigma_n), iz = 1.0f / (prm.sigma_z * prm.sigma_z);
    for (int l = 0; l < prm.levels; l++) {
        const float4 *src = A[(l + 1) & 1];                 // level 0 reads the prefiltered A1
        if (l + 1 < prm.levels) hipLaunchKernelGGL(k_dnv_atrous<false>, g, dim3(B), 0, c->stream, src, (const float4 *)G, (const float *)D, A[l & 1], (float *)nullptr, W, H, NP, 1 << l, sc2, in, iz);
        else hipLaunchKernelGGL(k_dnv_atrous<true>, g, dim3(B), 0, c->stream, src, (const float4 *)G, (const float *)D, (float4 *)nullptr, out, W, H, NP, 1 << l, sc2, in, iz);
    }
    TIRT_HIP(hipGetLastError());
    return TIRT_OK;
}

// tirt_denoise_var: the caller (tirt_api.hip) has ordered the stream after the last film update (which covers the moments) and the last k_aov.
int denoise_var_film(tirt_ctx *c, const tirt_denoise_var_t *prm)
{
    const char *fn = "tirt_denoise_var";
    TIRT_REQUIRE(c->hdr.p, "tirt_denoise_var: film not created");
    TIRT_REQUIRE(c->aov.p, "tirt_denoise_var: feature buffers not enabled (tirt_aov_enable)");
    TIRT_REQUIRE(c->mom.p, "tirt_denoise_var: moment buffers not enabled (tirt_moments_enable)");
    TIRT_REQUIRE(c->tile_count == 1, "tirt_denoise_var: tile_count > 1 -- this context's film is partial: reduce the films and the records, then tirt_denoise_var_device");
    if (int rc = denoise_var_check_params(fn, prm)) return rc;
    const size_t NP = (size_t)c->W * c->H;
    if (int rc = denoise_prepare(c, NP)) return rc;
    if (c->dn_out.ensure(sizeof(float) * 3 * NP)) return TIRT_ERR_HIP;
    return denoise_var_launch(c, c->hdr.as<float>(), c->aov.as<float>(), c->mom.as<float>(), c->dn_out.as<float>(), c->W, c->H, *prm);
}

int denoise_var_device(tirt_ctx *c, const float *hdr, const float *aov, const float *mom, float *out, int W, int H, const tirt_denoise_var_t *prm, void *stream)
{
    const char *fn = "tirt_denoise_var_device";
    TIRT_REQUIRE(W >= 1 && H >= 1 && (long long)W * H < (1ll << 30), "tirt_denoise_var_device: bad size");
    if (int rc = denoise_var_check_params(fn, prm)) return rc;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) {
        (void)hipGetLastError();
        set_error("tirt_denoise_var_device: the caller's stream is not a stream of this process's HIP runtime");
        return TIRT_ERR_ARG;
    }
    TIRT_REQUIRE(cs == hipStreamCaptureStatusNone, "tirt_denoise_var_device: the caller's stream is capturing a graph (the filter cannot be captured)");
    TIRT_REQUIRE(hdr && aov && mom && out, "tirt_denoise_var_device: null pointer");
    if (int rc = require_device_ptr(c, hdr, "tirt_denoise_var_device: hdr")) return rc;
    if (int rc = require_device_ptr(c, aov, "tirt_denoise_var_device: aov")) return rc;
    if (int rc = require_device_ptr(c, mom, "tirt_denoise_var_device: mom")) return rc;
    if (int rc = require_device_ptr(c, out, "tirt_denoise_var_device: out")) return rc;
    const size_t NP = (size_t)W * H;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + sizeof(float) * 3 * NP, h0 = (uintptr_t)hdr, h1 = h0 + sizeof(float) * 3 * NP,
                    a0 = (uintptr_t)aov, a1 = a0 + sizeof(float) * TIRT_AOV_WORDS * NP, m0 = (uintptr_t)mom, m1 = m0 + sizeof(float) * TIRT_MOM_WORDS * NP;
    TIRT_REQUIRE((o1 <= h0 || h1 <= o0) && (o1 <= a0 || a1 <= o0) && (o1 <= m0 || m1 <= o0), "tirt_denoise_var_device: out overlaps hdr, aov or mom");
    TIRT_REQUIRE((a0 & 15) == 0 && (m0 & 15) == 0, "tirt_denoise_var_device: aov and mom must be 16-byte aligned");
    if (int rc = denoise_prepare(c, NP)) return rc;
    if (int rc = query_begin(c, stream)) return rc;
    if (int rc = denoise_var_launch(c, hdr, aov, mom, out, W, H, *prm)) return rc;
    return query_end(c, stream);
}

}  // namespace tirt
