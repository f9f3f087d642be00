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

// ---- emitters chosen by power (include/tirt.h, "Choosing emitters by power"): the table behind the light records (tirt_device.h, light_table).  Here because it shares
// the scan.  Weights come from the light records -- the emission and get_prim_area k_light_records put there --, their maximum from an atomic maximum over the bits of
// positive floats (exact and order-free: such bits order as the floats do), the sums from the integer scan above: every order of threads gives one table.
//   k_light_weights  bits of w_i (0: takes no part) into the unsummed entries, their maximum into the head      one thread per entry
//   k_light_quant    e_max from the maximum, q_i in the entries' place                                          one thread per entry
//   k_env_scan       inclusive sum in place                                                                       one block
//   k_light_head     total, uniform share and e_max into the head
//   k_light_phit     P_i into the spare word of the shading record of the primitive entry i names (or 0 there)  one thread per entry
__global__ __launch_bounds__(256) void k_light_weights(const float4 *lrec, int n, env_u64 *cum, unsigned *max_bits)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 *r = lrec + (size_t)i * LIGHT_REC_QUADS;
    const unsigned b = light_weight_bits(r[3].w, r[4].w, r[5].w, r[0].w);
    cum[i] = (env_u64)b;
    if (b) atomicMax(max_bits, b);
}
__global__ __launch_bounds__(256) void k_light_quant(env_u64 *cum, int n, const unsigned *max_bits)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cum[i] = (env_u64)light_weight_q((unsigned)cum[i], light_weight_emax(*max_bits));
}
__global__ void k_light_head(env_u64 *head, const env_u64 *cum, int n, float u)
{
    const unsigned max_bits = ((const unsigned *)head)[4];
    head[0] = cum[n - 1];
    ((float *)head)[2] = u; ((int *)head)[3] = light_weight_emax(max_bits);
}
__global__ __launch_bounds__(256) void k_light_phit(SceneView s, float4 *shade_rec, int on)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.light_count) return;
    const int prim = s.light[i];
    if (prim < 0 || prim >= s.n) return;
    float P = 0.0f;
    if (on) { const LightTable t = light_table(s); P = light_choice_P(t.cum[i] - (i > 0 ? t.cum[i - 1] : 0ull), t.total, t.u, s.light_count); }
    float4 *r = shade_rec + (size_t)prim * 8;
    if (s.primitive[(size_t)prim * PRI_VEC] == PRIMITIVE_TRI) r[4].w = P; else r[2].x = P;
}

int light_table_sync(tirt_ctx *c)
{
    bool rebuilt = false;
    if (!c->light_tab_valid) {
        c->light_tab_total = 0ull; c->light_tab_emax = 0;
        if (light_power_wanted(c)) {
            const int n = c->light_count;
            env_u64 *head = (env_u64 *)((char *)c->light_rec.p + light_table_offset(n)), *cum = head + LIGHT_TABLE_HEAD / 8;
            TIRT_HIP(hipMemsetAsync(head, 0, LIGHT_TABLE_HEAD, c->stream));
            hipLaunchKernelGGL(k_light_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->light_rec.as<float4>(), n, cum, (unsigned *)head + 4);
            hipLaunchKernelGGL(k_light_quant, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, cum, n, (const unsigned *)head + 4);
            hipLaunchKernelGGL(k_env_scan, dim3(1), dim3(256), 0, c->stream, cum, n, (env_u64 *)nullptr, (size_t)0);
            hipLaunchKernelGGL(k_light_head, dim3(1), dim3(1), 0, c->stream, head, cum, n, c->light_uniform_share);
            TIRT_HIP(hipGetLastError());
            env_u64 h[2] = {0ull, 0ull};
            TIRT_HIP(hipMemcpyAsync(h, head, sizeof(h), hipMemcpyDeviceToHost, c->stream));
            TIRT_HIP(hipStreamSynchronize(c->stream));
            c->light_tab_total = h[0]; c->light_tab_emax = (int)(h[1] >> 32);
        }
        c->light_tab_valid = true;
        rebuilt = true;
    }
    const bool want = light_power_active(c);
    if (c->light_count > 0 && ((want && (rebuilt || !c->light_phit_written)) || (!want && c->light_phit_written))) {
        hipLaunchKernelGGL(k_light_phit, dim3((unsigned)((c->light_count + 255) / 256)), dim3(256), 0, c->stream, scene_view(c), c->shade_rec.as<float4>(), want ? 1 : 0);
        TIRT_HIP(hipGetLastError());
        c->light_phit_written = want;
    }
    return TIRT_OK;
}

// the rule of light_table_sync on host tables: does an entry of the list have a weight that takes part (get_prim_area's expressions, Scene.py:324-350)
bool light_table_exists_host(const float *material, int nm, const int32_t *primitive, int n, const float *shape, int ns, const float *vertex, int nv, const int32_t *light, int light_count)
{
    for (int i = 0; i < light_count; i++) {
        if (light[i] < 0 || light[i] >= n) continue;
        const int32_t *pr = primitive + (size_t)light[i] * PRI_VEC;
        if (pr[2] < 0 || pr[2] >= nm) continue;
        const float *m = material + (size_t)pr[2] * MAT_VEC;
        float area = 0.0f;
        if (pr[0] == PRIMITIVE_TRI) {
            if (pr[1] < 0 || pr[1] + 2 >= nv) continue;
            const float *p1 = vertex + (size_t)pr[1] * VER_VEC, *p2 = p1 + VER_VEC, *p3 = p2 + VER_VEC;
            float len[3];
            const float *ea[3] = {p1, p1, p3}, *eb[3] = {p2, p3, p2};
            for (int k = 0; k < 3; k++) {
                const float x = ea[k][0] - eb[k][0], y = ea[k][1] - eb[k][1], z = ea[k][2] - eb[k][2];
                len[k] = tm_sqrt((x * x + y * y) + z * z);
            }
            const float sum = (len[0] + len[1] + len[2]) * 0.5f;
            area = tm_sqrt(sum * (sum - len[0]) * (sum - len[1]) * (sum - len[2]));
        } else {
            if (pr[1] < 0 || pr[1] >= ns) continue;
            const float *sh = shape + (size_t)pr[1] * SHA_VEC;
            const int st = (int)sh[0];
            if (st == SHAPE_SPHERE || st == SHAPE_SPOT || st == SHAPE_LASER) area = sh[4] * sh[4] * PI_SCENE;
        }
        if (light_weight_bits(m[2], m[3], m[4], area)) return true;
    }
    return false;
}

int light_table_download(tirt_ctx *c, uint32_t *q, uint64_t *prefix, float *P, int32_t info[4])
{
    TIRT_REQUIRE(info, "tirt_light_table_download: null info");
    if (c->n >= 1 && ensure_shade_records(c)) return TIRT_ERR_HIP;
    const bool built = c->n >= 1 && light_power_wanted(c);
    info[0] = c->light_count; info[1] = c->light_tab_emax; info[2] = c->n >= 1 && light_power_active(c) ? 1 : 0; info[3] = built ? 1 : 0;
    if (!built || !(q || prefix || P)) return TIRT_OK;
    const int n = c->light_count;
    std::vector<uint64_t> cum((size_t)n);
    TIRT_HIP(hipMemcpyAsync(cum.data(), (const char *)c->light_rec.p + light_table_offset(n) + LIGHT_TABLE_HEAD, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    TIRT_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) {
        const uint64_t qi = cum[(size_t)i] - (i ? cum[(size_t)i - 1] : 0ull);
        if (q) q[i] = (uint32_t)qi;
        if (prefix) prefix[i] = cum[(size_t)i];
        if (P) P[i] = c->light_tab_total ? light_choice_P(qi, c->light_tab_total, c->light_uniform_share, n) : 0.0f;
    }
    return TIRT_OK;
}

// ---- known-answer entry (tirt_kat_light_pick): light_pick of tirt_device.h, the function shade_path calls, row i on thread i ----
__global__ void k_kat_light_pick(SceneView sc, const float *in, int in_stride, float *out, int out_stride, int n)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    float P;
    const int i = light_pick(light_table(sc), sc.light_count, in[(size_t)r * in_stride], P);
    float *o = out + (size_t)r * out_stride;
    o[0] = __int_as_float(i); o[1] = P;
}

int kat_light_pick(tirt_ctx *c, const float *in, int in_stride, float *out, int out_stride, int n)
{
    TIRT_REQUIRE(c->n >= 1, "tirt_kat_light_pick: no scene");
    for (int i = 0; i < n; i++) {
        const float r = in[(size_t)i * in_stride];
        TIRT_REQUIRE(r >= 0.0f && r <= 1.0f, "tirt_kat_light_pick: row " + std::to_string(i) + ": a random outside [0, 1]");
    }
    if (sync_all(c) || ensure_shade_records(c)) return TIRT_ERR_HIP;
    TIRT_REQUIRE(light_power_active(c), "tirt_kat_light_pick: no table (tirt_light_sampling mode 1, triangle and sphere emitters only, total > 0)");
    if (n == 0) return TIRT_OK;
    return kat_round_trip(c, "tirt_kat_light_pick", {{in, kat_row_bytes(n, in_stride)}}, out, kat_row_bytes(n, out_stride), [&](const void *const *din, void *dout) {
        hipLaunchKernelGGL(k_kat_light_pick, dim3((n + 63) / 64), dim3(64), 0, c->stream, scene_view(c), (const float *)din[0], in_stride, (float *)dout, out_stride, n);
    });
}

}  // namespace tirt
