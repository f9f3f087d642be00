// tirt_moments.hip -- per-pixel sample moments of PT_RGB: how many pixel-samples a pixel has, their mean and their sum of squared deviations.
//
// No reference counterpart.  At the end of a wavefront batch PathState::fr / fg / fb[slot] hold the final radiance of every pixel-sample; k_film
// folds them into the film's running mean.  k_moments is one more reader of those three streams: per local pixel it folds the F samples of the
// batch, in frame order, into the pixel's TIRT_MOM_WORDS record with Welford's update (include/tirt.h states the arithmetic, tests/moments_expected.py
// restates it in numpy and the device has to give its bits: one f32 rounding per operation, -ffp-contract=off, the division IEEE's).
//
// n is the record's own count, not the frame index: the record is a valid set of moments over whatever was rendered since the last clear, in
// whatever order and at whatever seeds.  As an f32 it is exact up to 2^24 samples per pixel (n + 1 == n beyond that).
//
// Ordering.  The recurrence is order dependent and batches run on different lanes.  k_moments needs fr / fg / fb, which are complete only when the
// batch's last launch is -- exactly where k_film runs -- and k_film already makes the lane's stream wait for last_film, the film update of the
// previous batch, before it starts.  k_moments is queued on the same stream straight after k_film and BEFORE the lane records its film_done, so
// (i) it inherits that wait: the previous batch's k_moments lies before the previous film_done, (ii) film_done now stands for "film and moments
// updated", and every main-stream consumer that waits for last_film (downloads, clear, the filter) is ordered after the moments as well, (iii) with
// the records off nothing at all is added.  An event chain of its own, as k_aov has (last_aov), would buy nothing here: k_aov runs after bounce 0
// and must not wait for the END of the previous batch, whereas k_moments sits at the end of its batch anyway, behind a wait that is already there.
//
// PT_RGB only: tirt_pt_spec_render's per-sample values are four hero-wavelength radiances that k_film_spec turns into XYZ -> RGB, BDPT splats
// into the film, Debug overwrites it: none of them leaves RGB radiance per pixel-sample in fr / fg / fb, and none of them touches the records.
#include "tirt_internal.h"

namespace tirt {

TD bool mom_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }      // false for NaN

// One thread per local pixel k.  The three sample words of a slot are streams, read once: non-temporal.  The loads of frame f + 1 are issued
// before frame f's dependent arithmetic (three divisions on one chain per channel).
// LIST: the batch's local pixels are a pixel set's list (mapped_pixel, tirt_internal.h).
template <bool LIST>
__global__ __launch_bounds__(256) void k_moments(const float *fr, const float *fg, const float *fb, TileMap tm, int P, int F, float *mom)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int p = mapped_pixel<LIST>(tm, k);
    float4 *const px = (float4 *)(mom + (size_t)p * TIRT_MOM_WORDS);
    const float4 lo = px[0], hi = px[1];
    float n = lo.x, m0 = lo.y, m1 = lo.z, m2 = lo.w, q0 = hi.x, q1 = hi.y, q2 = hi.z, bad = hi.w;
    int s = frame_pixel_to_slot(tm, P, 0, k);
    float x0 = __builtin_nontemporal_load(&fr[s]), x1 = __builtin_nontemporal_load(&fg[s]), x2 = __builtin_nontemporal_load(&fb[s]);
    for (int f = 0; f < F; f++) {
        float y0 = x0, y1 = x1, y2 = x2;
        if (f + 1 < F) {
            s = frame_pixel_to_slot(tm, P, f + 1, k);
            y0 = __builtin_nontemporal_load(&fr[s]); y1 = __builtin_nontemporal_load(&fg[s]); y2 = __builtin_nontemporal_load(&fb[s]);
        }
        if (mom_finite(x0) && mom_finite(x1) && mom_finite(x2)) {
            n += 1.0f;
            const float d0 = x0 - m0, d1 = x1 - m1, d2 = x2 - m2;
            m0 = m0 + d0 / n; m1 = m1 + d1 / n; m2 = m2 + d2 / n;
            q0 = q0 + d0 * (x0 - m0); q1 = q1 + d1 * (x1 - m1); q2 = q2 + d2 * (x2 - m2);
        } else {
            bad += 1.0f;
        }
        x0 = y0; x1 = y1; x2 = y2;
    }
    px[0] = make_float4(n, m0, m1, m2);
    px[1] = make_float4(q0, q1, q2, bad);
}

// Queued by pt_render on the lane's stream straight after k_film (which has waited for last_film) and before film_done is recorded.
int moments_launch(tirt_ctx *c, Lane &L, const TileMap &tm, int P, int F)
{
    const int B = 256;
    hipLaunchKernelGGL(tm.pixels ? k_moments<true> : k_moments<false>, dim3((P + B - 1) / B), dim3(B), 0, L.stream, (const float *)L.ps.fr, (const float *)L.ps.fg, (const float *)L.ps.fb,
                       tm, P, F, c->mom.as<float>());
    return TIRT_OK;
}

// tirt_moments_converged: one pass over the records of this context's own pixels; counts are summed over the wave, then one atomic per wave into
// LDS and one per block and counter into memory, as k_shade does for its statistics.  Integers: the result does not depend on the order.
TD unsigned long long mom_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_moments_converged(const float *mom, TileMap tm, int P, float t2, unsigned long long *out)
{
    __shared__ unsigned long long s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long measured = 0ull, noisy = 0ull, bad = 0ull;
    if (k < P) {                                           // (no early return: every lane takes part in the wave sums)
        const float4 *px = (const float4 *)(mom + (size_t)local_to_pixel(tm, k) * TIRT_MOM_WORDS);
        const float4 lo = px[0], hi = px[1];
        const float n = lo.x;
        if (n >= 2.0f) {
            measured = 1ull;
            const float nn = n * (n - 1.0f);
            const float v = (hi.x / nn + hi.y / nn) + hi.z / nn;
            const float Y = ((lo.y + lo.z) + lo.w) / 3.0f;
            if (v > t2 * (Y * Y)) noisy = 1ull;
        }
        if (hi.w > 0.0f) bad = 1ull;
    }
    measured = mom_wave_sum(measured); noisy = mom_wave_sum(noisy); bad = mom_wave_sum(bad);
    if ((threadIdx.x & 63) == 0) {
        if (measured) atomicAdd(&s_cnt[0], measured);
        if (noisy) atomicAdd(&s_cnt[1], noisy);
        if (bad) atomicAdd(&s_cnt[2], bad);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_cnt[threadIdx.x]);
}

// The caller (tirt_api.hip) has ordered the main stream after the last film and moment update and checked the arguments.
int moments_converged(tirt_ctx *c, float t2, uint64_t out[3])
{
    out[0] = out[1] = out[2] = 0;
    const long P = c->npix_local;
    if (P <= 0) return TIRT_OK;
    if (c->mom_cnt.ensure(3 * sizeof(unsigned long long))) return TIRT_ERR_HIP;
    TIRT_HIP(hipMemsetAsync(c->mom_cnt.p, 0, 3 * sizeof(unsigned long long), c->stream));
    TileMap tm = {c->tile_rank, c->tile_count, c->tile_size, c->H, c->tile_blocked, 0};
    const int B = 256;
    hipLaunchKernelGGL(k_moments_converged, dim3((unsigned)((P + B - 1) / B)), dim3(B), 0, c->stream, c->mom.as<float>(), tm, (int)P, t2,
                       c->mom_cnt.as<unsigned long long>());
    unsigned long long h[3] = {0, 0, 0};
    TIRT_HIP(hipMemcpyAsync(h, c->mom_cnt.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    TIRT_HIP(hipGetLastError());
    for (int i = 0; i < 3; i++) out[i] = h[i];
    return TIRT_OK;
}

}  // namespace tirt
