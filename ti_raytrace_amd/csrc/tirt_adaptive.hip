// tirt_adaptive.hip -- the pixel set of PT_RGB (a list of pixels the next renders are restricted to), its selection from the sample moments, and the
// driver that renders pass after pass on the pixels still noisy.
//
// No reference counterpart.  include/tirt.h states the semantics; tests/adaptive_expected.py restates the selection in numpy.  What makes a list pass exact:
// the random numbers are counter-based on (seed, pixel, frame, dimension) and k_film's weight is 1 / (frame + 1), so nothing a pixel receives depends on which
// other pixels share its batch or on its slot in it.  A batch of a set is an ordinary wavefront batch of P' = n local pixels whose map to the film is the list
// (TileMap::pixels, read by the LIST instantiations of k_generate, k_shade, k_aov, k_film and k_moments); its camera rays go through k_trace alone, the
// candidate lists of tirt_pvb.hip being indexed by the tiles' local pixel.
//
// The list lives in one buffer of 4 * npix_local bytes.  It is written here only, on the main stream, after sync_all: no batch that reads it is in flight.
//
// k_pixel_select is three launches: (1) every block of 256 local pixels counts its listed ones, (2) one block turns the counts into exclusive offsets and the
// total, (3) every block writes its listed pixels behind its offset -- rank inside the wave from the ballot (mbcnt), the waves of the block through LDS.  The
// list is therefore in ascending local order whatever the scheduler does (one atomicAdd per wave to claim space would make the order the scheduler's), and the
// pixels of an 8 x 8 block stay neighbours in it: the camera rays of a wave stay a bundle.  The predicate is evaluated twice (32 bytes per pixel each time)
// rather than kept: the records are not written in between.
#include "tirt_internal.h"

namespace tirt {

constexpr int SEL_BLOCK = 256, SCAN_BLOCK = 1024;

// tirt_moments_converged's expressions in its operand order (k_moments_converged); a comparison with a NaN is false
TD bool pixel_listed(const float4 lo, const float4 hi, float t2, float fmin, float fmax)
{
    const float n = lo.x, total = n + hi.w;
    if (!(total < fmax)) return false;
    if (total < fmin || n < 2.0f) return true;
    const float nn = n * (n - 1.0f);
    const float v = (hi.x / nn + hi.y / nn) + hi.z / nn;
    const float Y = ((lo.y + lo.z) + lo.w) / 3.0f;
    return v > t2 * (Y * Y);
}

// (1) block_count[b] = listed pixels among local pixels 256 b ..; with expect >= 0 also res[1] += pixels whose total differs from it, res[2] += pixels whose
// record is not all zero bits (the adaptive driver's check of its starting film: integers, the sums do not depend on the order)
__global__ __launch_bounds__(SEL_BLOCK) void k_pixel_count(const float *mom, TileMap tm, int P, float t2, float fmin, float fmax, float expect, int *block_count, unsigned *res)
{
    __shared__ unsigned s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    bool listed = false, other = false, nonzero = false;
    if (k < P) {                                           // (no early return: every lane takes part in the ballots)
        const float4 *px = (const float4 *)(mom + (size_t)local_to_pixel(tm, k) * TIRT_MOM_WORDS);
        const float4 lo = px[0], hi = px[1];
        listed = pixel_listed(lo, hi, t2, fmin, fmax);
        if (expect >= 0.0f) {
            other = !(lo.x + hi.w == expect);
            nonzero = ((__float_as_uint(lo.x) | __float_as_uint(lo.y) | __float_as_uint(lo.z) | __float_as_uint(lo.w) |
                        __float_as_uint(hi.x) | __float_as_uint(hi.y) | __float_as_uint(hi.z) | __float_as_uint(hi.w)) != 0u);
        }
    }
    const unsigned nl = (unsigned)__popcll(__ballot(listed)), no = (unsigned)__popcll(__ballot(other)), nz = (unsigned)__popcll(__ballot(nonzero));
    if ((threadIdx.x & 63) == 0) {
        if (nl) atomicAdd(&s_cnt[0], nl);
        if (no) atomicAdd(&s_cnt[1], no);
        if (nz) atomicAdd(&s_cnt[2], nz);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_count[blockIdx.x] = (int)s_cnt[0];
        if (s_cnt[1]) atomicAdd(&res[1], s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&res[2], s_cnt[2]);
    }
}

// (2) one block: block_count[0 .. nb) -> its exclusive prefix sums in place, res[0] = the total.  1024 counts per trip: a shuffle scan inside each wave, the
// sixteen wave totals through LDS, the carry of the earlier trips.
__global__ __launch_bounds__(SCAN_BLOCK) void k_pixel_scan(int *block_count, int nb, unsigned *res)
{
    __shared__ int s_w[SCAN_BLOCK / 64];
    __shared__ int s_carry;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += SCAN_BLOCK) {          // (the same trips for every thread)
        const int i = base + (int)threadIdx.x;
        const int v = i < nb ? block_count[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        if (lane == 63) s_w[wid] = inc;
        __syncthreads();
        int before = s_carry;
#pragma unroll
        for (int w = 0; w < SCAN_BLOCK / 64; w++) if (w < wid) before += s_w[w];
        if (i < nb) block_count[i] = before + inc - v;
        __syncthreads();                                         // s_carry and s_w have been read by all
        if (threadIdx.x == SCAN_BLOCK - 1) s_carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) res[0] = (unsigned)s_carry;
}

// (3) the listed pixels of block b to list[block_offset[b] ..], in ascending k
__global__ __launch_bounds__(SEL_BLOCK) void k_pixel_scatter(const float *mom, TileMap tm, int P, float t2, float fmin, float fmax, const int *block_offset, int *list)
{
    __shared__ int s_w[SEL_BLOCK / 64];
    const int wid = threadIdx.x >> 6;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    bool listed = false;
    int p = 0;
    if (k < P) {
        p = local_to_pixel(tm, k);
        const float4 *px = (const float4 *)(mom + (size_t)p * TIRT_MOM_WORDS);
        listed = pixel_listed(px[0], px[1], t2, fmin, fmax);
    }
    const unsigned long long mask = __ballot(listed);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));      // listed lanes below this one
    if ((threadIdx.x & 63) == 0) s_w[wid] = __popcll(mask);
    __syncthreads();
    int at = block_offset[blockIdx.x] + rank;
#pragma unroll
    for (int w = 0; w < SEL_BLOCK / 64; w++) if (w < wid) at += s_w[w];
    if (listed && at < P) list[at] = p;                    // (at < P always: the counts are of the same predicate over the same records)
}

// local index of pixel p in this context's order (the inverse of local_to_pixel), or -1 for a pixel of another rank's tile
static long pixel_to_local(const tirt_ctx *c, long p)
{
    const long t = p / c->tile_size;
    if (t % c->tile_count != c->tile_rank) return -1;
    long within = p - t * c->tile_size;
    if (c->tile_blocked) {
        const long col = within / c->H, row = within - col * c->H, rows = c->H >> 3;
        within = ((((col >> 3) * rows + (row >> 3)) << 6) | ((col & 7) << 3) | (row & 7));
    }
    return (t / c->tile_count) * c->tile_size + within;
}

static int ensure_list(tirt_ctx *c)
{ return c->pixset.ensure(sizeof(int) * (size_t)(c->npix_local > 0 ? c->npix_local : 1)); }

int pixel_set_upload(tirt_ctx *c, const int32_t *pixels, int64_t n)
{
    TIRT_REQUIRE(c->hdr.p, "tirt_pixel_set_upload: film not created");
    TIRT_REQUIRE(n >= 0 && (n == 0) == (pixels == nullptr), "tirt_pixel_set_upload: n < 0, a list without entries or entries without a list");
    const long NP = (long)c->W * c->H;
    long last = -1;
    for (int64_t e = 0; e < n; e++) {
        const long p = pixels[e];
        TIRT_REQUIRE(p >= 0 && p < NP, "tirt_pixel_set_upload: entry " + std::to_string(e) + " outside [0, W*H)");
        const long k = pixel_to_local(c, p);
        TIRT_REQUIRE(k >= 0 && k < c->npix_local, "tirt_pixel_set_upload: entry " + std::to_string(e) + " is a pixel of another rank's tile");
        TIRT_REQUIRE(k > last, "tirt_pixel_set_upload: entry " + std::to_string(e) + " is not after its predecessor in this context's local order");
        last = k;
    }
    if (sync_all(c)) return TIRT_ERR_HIP;
    if (ensure_list(c)) return TIRT_ERR_HIP;
    if (n > 0) TIRT_HIP(hipMemcpy(c->pixset.p, pixels, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    c->pixset_n = (long)n;
    return TIRT_OK;
}

int pixel_set_clear(tirt_ctx *c)
{
    if (c->pixset_n < 0) return TIRT_OK;
    if (sync_all(c)) return TIRT_ERR_HIP;
    c->pixset_n = -1;
    return TIRT_OK;
}

// The arguments are checked (tirt_api.hip).  expect_total >= 0: check[0] = pixels of this context whose total differs from it, check[1] = pixels whose record is
// not all zero, and the set is installed only if one of the two is 0 (the caller refuses otherwise).
int pixel_set_select(tirt_ctx *c, float t2, int min_samples, int max_samples, long expect_total, int64_t *count, int64_t check[2])
{
    if (sync_all(c)) return TIRT_ERR_HIP;
    const int P = (int)c->npix_local;
    const int nb = (P + SEL_BLOCK - 1) / SEL_BLOCK;
    unsigned h[3] = {0u, 0u, 0u};
    if (P > 0) {
        if (ensure_list(c) || c->pixset_tmp.ensure(sizeof(int) * ((size_t)nb + 4))) return TIRT_ERR_HIP;
        int *const block_count = c->pixset_tmp.as<int>() + 4;
        unsigned *const res = c->pixset_tmp.as<unsigned>();
        const TileMap tm = {c->tile_rank, c->tile_count, c->tile_size, c->H, c->tile_blocked, 0};
        const float *mom = c->mom.as<float>();
        const float fmin = (float)min_samples, fmax = (float)max_samples, expect = expect_total >= 0 ? (float)expect_total : -1.0f;
        TIRT_HIP(hipMemsetAsync(res, 0, 4 * sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(k_pixel_count, dim3(nb), dim3(SEL_BLOCK), 0, c->stream, mom, tm, P, t2, fmin, fmax, expect, block_count, res);
        hipLaunchKernelGGL(k_pixel_scan, dim3(1), dim3(SCAN_BLOCK), 0, c->stream, block_count, nb, res);
        hipLaunchKernelGGL(k_pixel_scatter, dim3(nb), dim3(SEL_BLOCK), 0, c->stream, mom, tm, P, t2, fmin, fmax, (const int *)block_count, c->pixset.as<int>());
        TIRT_HIP(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        TIRT_HIP(hipStreamSynchronize(c->stream));          // the one host wait: the next pass's launch sizes need the count
        TIRT_HIP(hipGetLastError());
    }
    if (check) { check[0] = h[1]; check[1] = h[2]; }
    if (count) *count = h[0];
    if (!(expect_total >= 0 && h[1] != 0u && h[2] != 0u)) c->pixset_n = (long)h[0];
    return TIRT_OK;
}

int render_adaptive(tirt_ctx *c, uint32_t frame_begin, uint32_t seed, int max_depth, int stack_size, int flags, const tirt_adaptive_t *a, tirt_adaptive_result_t *out)
{
    const float t2 = a->threshold * a->threshold;
    tirt_adaptive_result_t r = {0, 0, 0, 0};
    long start = -1;
    int rc = TIRT_OK;
    for (;;) {
        int64_t count = 0, chk[2] = {0, 0};
        const bool first = start < 0;
        if ((rc = pixel_set_select(c, t2, a->min_samples, a->max_samples, first ? (long)frame_begin : -1, &count, chk))) break;
        if (first) {
            if (chk[0] == 0) start = (long)frame_begin;
            else if (chk[1] == 0) start = 0;
            else {
                set_error("tirt_pt_rgb_render_adaptive: " + std::to_string((long long)chk[0]) + " pixels have another sample count than frame_begin (" +
                          std::to_string(frame_begin) + "): the film must be a dense prefix of frame_begin frames, or its moment records all zero");
                rc = TIRT_ERR_ARG;
                break;
            }
        }
        if (count == 0) break;
        const long left = (long)a->max_samples - start - r.frames;          // >= 1: a listed pixel has total = start + frames < max_samples
        const int F = (int)(left < a->pass_frames ? left : a->pass_frames);
        if (F < 1) break;
        if ((rc = pt_render(c, frame_begin + (uint32_t)r.frames, F, seed, max_depth, stack_size, flags))) break;
        r.passes++; r.pixel_samples += count * F; r.frames += F;
        if (start + r.frames >= a->max_samples) { r.pixels_at_max = count; break; }
    }
    // the set goes, the buffer stays: the batches in flight keep reading it, and nothing writes it before a sync_all
    c->pixset_n = -1;
    if (rc == TIRT_OK && out) *out = r;
    return rc;
}

}  // namespace tirt
