// tirt_envsample.hip -- the sampling table of the environment image: one weight per lookup cell, quantised to integers, summed along rows and over rows.
//
// No reference counterpart: integrator/PT_RGB.py:127-132 reads the environment only where a BSDF-sampled ray misses.  With tirt_env_sampling on, k_shade's
// SF_ENV_SAMPLE twins (tirt_render.hip, shade_path) take their light sample from the environment by its brightness and weight it against BSDF sampling;
// this file builds what they sample from.  include/tirt.h ("Importance sampling of the environment") states every operation; tests/env_sampling_expected.py
// restates it in numpy and the device has to give its bits.
//
// Why integers: q(i, j) = rint(weight * 2^24) is the last floating-point value.  Row sums and the marginal are 64-bit integer sums, so every scan order gives
// the same table, and the choice of a cell from a 24-bit random is an exact integer comparison (env_pick, tirt_device.h).
//
// Where it lives: behind the texels, in the allocation SceneView::env points to (env_table_offset, tirt_device.h).  SceneView is an argument of every shading
// kernel; a new member would move the argument block of the kernels that do not sample, and with it their code.
//
//   k_env_cells      q of every cell, as the unsummed row entries                         one thread per cell   (k_env_cells_hdr: the same of an RGBE8 image)
//   k_env_row_scan   inclusive sum of a row in place, its total into the marginal          one 256-thread block per row: wave scans + a carry per 256-entry chunk
//   k_env_marg_scan  inclusive sum of the marginal in place, total and share into the head one block
#include "tirt_internal.h"
#include <vector>

namespace tirt {

__global__ __launch_bounds__(256) void k_env_cells(const int *img, int w, int h, env_u64 *rows)
{
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (size_t)w * h) return;
    const int j = (int)(c / (size_t)w), i = (int)(c - (size_t)j * w);
    rows[c] = (env_u64)env_cell_q(img, w, h, i, j);
}

// an RGBE8 image (include/tirt.h, "HDR environment"): the level of the decoded texels, scaled by 2^(152 - e_max).  A kernel of its own: k_env_cells keeps its
// argument block and its code
__global__ __launch_bounds__(256) void k_env_cells_hdr(const int *img, int w, int h, env_u64 *rows, int e_max)
{
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (size_t)w * h) return;
    const int j = (int)(c / (size_t)w), i = (int)(c - (size_t)j * w);
    rows[c] = (env_u64)env_cell_q_hdr(img, w, h, i, j, e_max);
}

// inclusive sum over the 256 threads of a block; every thread of the block calls it
TD env_u64 env_block_scan(env_u64 v, env_u64 *s_wave)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const env_u64 u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
    __syncthreads();                           // (s_wave of the previous chunk has been read)
    if (lane == 63) s_wave[wid] = v;
    __syncthreads();
    for (int k = 0; k < wid; k++) v += s_wave[k];
    return v;
}

__global__ __launch_bounds__(256) void k_env_scan(env_u64 *data, int n, env_u64 *total_out, size_t total_stride)
{
    __shared__ env_u64 s_wave[4];
    __shared__ env_u64 s_carry;
    env_u64 *row = data + (size_t)blockIdx.x * n;
    env_u64 carry = 0ull;
    for (int base = 0; base < n; base += 256) {
        const int k = base + (int)threadIdx.x;
        const env_u64 v = env_block_scan(k < n ? row[k] : 0ull, s_wave) + carry;
        if (k < n) row[k] = v;
        if (threadIdx.x == 255) s_carry = v;
        __syncthreads();
        carry = s_carry;
    }
    if (threadIdx.x == 0 && total_out) total_out[(size_t)blockIdx.x * total_stride] = carry;
}

__global__ void k_env_head(env_u64 *head, const env_u64 *marg, int h, float share)
{
    head[0] = marg[h - 1];
    ((float *)head)[2] = share; ((float *)head)[3] = 0.0f;
}

static bool env_table_wanted(const tirt_ctx *c)
{ return c->env_sample_on && c->env.p && c->env_power != 0.0f && env_sample_dims_ok(c->env_w, c->env_h); }

int env_table_refresh(tirt_ctx *c)
{
    c->env_tab_valid = false;
    if (!env_table_wanted(c)) return TIRT_OK;
    const int w = c->env_w, h = c->env_h;
    const size_t off = env_table_offset(w, h), need = off + env_table_bytes(w, h);
    if (c->env.bytes < need) {                 // the texels move into an allocation with room for the table behind them
        DevBuf grown;
        if (grown.ensure(need)) return TIRT_ERR_HIP;
        const hipError_t e = hipMemcpyAsync(grown.p, c->env.p, sizeof(int32_t) * (size_t)w * h, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) { grown.release(); set_error(std::string("env_table_refresh: ") + hipGetErrorString(e)); return TIRT_ERR_HIP; }
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e2 != hipSuccess) { grown.release(); set_error(std::string("env_table_refresh: ") + hipGetErrorString(e2)); return TIRT_ERR_HIP; }
        c->env.release();
        c->env = grown;
    }
    env_u64 *head = (env_u64 *)((char *)c->env.p + off), *marg = head + 2, *rows = marg + h;
    const size_t cells = (size_t)w * h;
    if (c->env_format == 1) hipLaunchKernelGGL(k_env_cells_hdr, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, c->env.as<int>(), w, h, rows, c->env_emax);
    else hipLaunchKernelGGL(k_env_cells, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, c->env.as<int>(), w, h, rows);
    hipLaunchKernelGGL(k_env_scan, dim3((unsigned)h), dim3(256), 0, c->stream, rows, w, marg, (size_t)1);
    hipLaunchKernelGGL(k_env_scan, dim3(1), dim3(256), 0, c->stream, marg, h, (env_u64 *)nullptr, (size_t)0);
    hipLaunchKernelGGL(k_env_head, dim3(1), dim3(1), 0, c->stream, head, marg, h, c->env_share);
    TIRT_HIP(hipGetLastError());
    env_u64 total = 0ull;
    TIRT_HIP(hipMemcpyAsync(&total, head, sizeof(total), hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    c->env_tab_valid = total > 0ull;           // a black image: no table
    return TIRT_OK;
}

// the share alone has changed and the table stands: the head's four bytes, no cells, no scans
int env_table_set_share(tirt_ctx *c)
{
    if (!c->env_tab_valid) return env_table_refresh(c);
    env_u64 *head = (env_u64 *)((char *)c->env.p + env_table_offset(c->env_w, c->env_h));
    hipLaunchKernelGGL(k_env_head, dim3(1), dim3(1), 0, c->stream, head, head + 2, c->env_h, c->env_share);
    TIRT_HIP(hipGetLastError());
    TIRT_HIP(hipStreamSynchronize(c->stream));
    return TIRT_OK;
}

bool env_table_exists_host(const int32_t *env, int w, int h, float power)
{
    if (!env || power == 0.0f || !env_sample_dims_ok(w, h)) return false;
    for (int j = 0; j < h; j++) for (int i = 0; i < w; i++) if (env_cell_q(env, w, h, i, j) > 0u) return true;
    return false;
}

int env_hdr_check(const char *fn, const int32_t *rgbe, int w, int h, int *e_max)
{
    int top = 0;
    const size_t count = (size_t)w * h;
    for (size_t k = 0; k < count; k++) {
        const unsigned t = (unsigned)rgbe[k];
        const int e = (int)(t >> 24);
        TIRT_REQUIRE(e != 0 || (t & 0x00FFFFFFu) == 0u, std::string(fn) + ": texel " + std::to_string(k) + " has exponent byte 0 and a mantissa that is not 0 (E == 0 is black only)");
        if ((t & 0x00FFFFFFu) != 0u && e > top) top = e;
    }
    *e_max = top;
    return TIRT_OK;
}

bool env_table_exists_host_hdr(const int32_t *env, int w, int h, float power, int e_max)
{
    if (!env || power == 0.0f || !env_sample_dims_ok(w, h)) return false;
    for (int j = 0; j < h; j++) for (int i = 0; i < w; i++) if (env_cell_q_hdr(env, w, h, i, j, e_max) > 0u) return true;
    return false;
}

int env_table_download(tirt_ctx *c, uint32_t *q, uint64_t *row_sums, uint64_t *marginal, int32_t info[4])
{
    TIRT_REQUIRE(info, "tirt_env_table_download: null info");
    info[0] = c->env_w; info[1] = c->env_h; info[2] = c->env_tab_valid ? 1 : 0; info[3] = env_sample_active(c) ? 1 : 0;
    if (!c->env_tab_valid) return TIRT_OK;
    const int w = c->env_w, h = c->env_h;
    const env_u64 *marg = (const env_u64 *)((const char *)c->env.p + env_table_offset(w, h)) + 2, *rows = marg + h;
    if (marginal) TIRT_HIP(hipMemcpyAsync(marginal, marg, sizeof(uint64_t) * (size_t)h, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint64_t> tmp;
    uint64_t *rs = row_sums;
    if (q && !rs) { tmp.resize((size_t)w * h); rs = tmp.data(); }
    if (rs) TIRT_HIP(hipMemcpyAsync(rs, rows, sizeof(uint64_t) * (size_t)w * h, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    if (q) for (int j = 0; j < h; j++) for (int i = 0; i < w; i++) q[(size_t)j * w + i] = (uint32_t)(rs[(size_t)j * w + i] - (i ? rs[(size_t)j * w + i - 1] : 0ull));
    return TIRT_OK;
}

// ---- known-answer entries (tirt_kat_env_sample / tirt_kat_env_pdf): env_sample / env_pdf of tirt_device.h, the functions shade_path calls, row i on thread i ----
__global__ void k_kat_env(SceneView sc, int which, const float *in, int in_stride, float *out, int out_stride, int n)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float *a = in + (size_t)r * in_stride;
    float *o = out + (size_t)r * out_stride;
    const EnvTable et = env_table(sc);
    if (which == 0) {
        const EnvSample es = env_sample(et, sc.env_w, sc.env_h, a[0], a[1]);
        const EnvPdf ep = env_pdf(et, sc.env_w, sc.env_h, es.d);
        o[0] = __int_as_float(es.i); o[1] = __int_as_float(es.j); o[2] = es.tx; o[3] = es.ty; o[4] = es.d.x; o[5] = es.d.y; o[6] = es.d.z;
        o[7] = ep.pdf; o[8] = __int_as_float(ep.i); o[9] = __int_as_float(ep.j);
    } else {
        const EnvPdf ep = env_pdf(et, sc.env_w, sc.env_h, V(a[0], a[1], a[2]));
        o[0] = __int_as_float(ep.i); o[1] = __int_as_float(ep.j); o[2] = ep.tx; o[3] = ep.ty; o[4] = ep.pdf;
    }
}

// tirt_kat_env_lookup: env_lookup of tirt_device.h, the function shade_path's miss branch and environment sample call, in the format of the uploaded image
__global__ void k_kat_env_lookup(SceneView sc, int hdr, const float *in, int in_stride, float *out, int out_stride, int n)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float *a = in + (size_t)r * in_stride;
    float *o = out + (size_t)r * out_stride;
    const v3 e = hdr ? env_lookup<true>(sc.env, sc.env_w, sc.env_h, a[0], a[1]) : env_lookup<false>(sc.env, sc.env_w, sc.env_h, a[0], a[1]);
    o[0] = e.x; o[1] = e.y; o[2] = e.z;
}

int kat_env_lookup(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(c->env.p && c->env_w >= 1 && c->env_h >= 1, "tirt_kat_env_lookup: no environment image (tirt_env_upload, tirt_env_upload_hdr or a scene upload)");
    if (n == 0) return TIRT_OK;
    if (sync_all(c)) return TIRT_ERR_HIP;
    return kat_round_trip(c, "tirt_kat_env_lookup", {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_env_lookup, dim3((n + 63) / 64), dim3(64), 0, c->stream, scene_view(c), c->env_format == 1 ? 1 : 0, (const float *)din[0], in_stride, (float *)dout, out_stride, n);
    });
}

int kat_env(tirt_ctx *c, int which, const float *in, int in_stride, float *out, int out_stride, int n)
{
    const char *fn = which == 0 ? "tirt_kat_env_sample" : "tirt_kat_env_pdf";
    TIRT_REQUIRE(c->env_tab_valid, std::string(fn) + ": no sampling table (tirt_env_sampling on, env_power != 0, an image that is not black)");
    if (which == 0) for (int i = 0; i < n; i++) for (int k = 0; k < 2; k++) {
        const float r = in[(size_t)i * in_stride + k];
        TIRT_REQUIRE(r >= 0.0f && r < 1.0f, std::string(fn) + ": row " + std::to_string(i) + ": a random outside [0, 1)");
    }
    if (n == 0) return TIRT_OK;
    if (sync_all(c)) return TIRT_ERR_HIP;
    return kat_round_trip(c, fn, {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_env, dim3((n + 63) / 64), dim3(64), 0, c->stream, scene_view(c), which, (const float *)din[0], in_stride, (float *)dout, out_stride, n);
    });
}

}  // namespace tirt
