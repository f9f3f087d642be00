"""numpy restatement of the environment's sampling table, its inverse and its pdf (include/tirt.h, "Importance sampling of the environment"),
operation by operation: float32 with one rounding per operation up to the quantised weights, Python / uint64 integers from there on.  pow, cos, sin, atan2
and sqrt are the shared tm_* functions through the oracle's orc_kat_math (tests/test_math.py and tests/test_gpu_math.py hold the device to them), so the
device must give these bits.

  table(img, power)         {"w", "h", "q" [h, w] uint32, "row_sums" [h, w] uint64, "marginal" [h] uint64, "total" int} or None (no table)
  sample(tab, ra, rb)       (i, j, tx, ty, d [n, 3]) of randoms in [0, 1)
  pdf(tab, d)               (i, j, tx, ty, pdf) of directions
  env_radiance(img, tx, ty) srgb_to_lrgb(texture2D(env, tx, ty)), the miss branch's value before env_power
  nee_env(...)              one bounce's environment sample: contribution weight and shadow record, given the Disney evaluation
"""
import numpy as np

import oracle_api as oa
import texture_expected as te

f = np.float32
PI_SCENE = f(3.1415926)
TWO_PI_SQ = f(f(f(2.0) * PI_SCENE) * PI_SCENE)
MAX_DIM = 16384
MAX_CELLS = 1 << 25
SHADOW_DIST = f(2000000.0)
TWO24 = f(16777216.0)


def _math(fn, x, y=None):
    x = np.ascontiguousarray(x, f)
    y = np.zeros(x.size, f) if y is None else np.ascontiguousarray(np.broadcast_to(np.asarray(y, f), x.shape), f)
    out = np.zeros(x.size, f)
    if x.size:
        oa.load().orc_kat_math(int(fn), x.reshape(-1), y.reshape(-1), out, x.size)
    return out.reshape(x.shape)


def sin(x): return _math(0, x)
def cos(x): return _math(1, x)
def pow_(x, y): return _math(4, x, y)
def atan2(y, x): return _math(5, y, x)


def srgb_to_lrgb(c):
    c = np.asarray(c, f)
    lo = (c / f(12.92)).astype(f)
    hi = pow_(((c + f(0.055)).astype(f) / f(1.055)).astype(f), f(2.4))
    return np.where(c < f(0.04045), lo, hi).astype(f)


def texel_lum(img):
    """[w, h] float32: ((l.r + l.g) + l.b) / 3 of srgb_to_lrgb(texel / 255); img is Texture.np_img, [w, h] packed 0xRRGGBB"""
    img = np.asarray(img).astype(np.int64)
    ch = [(((img >> s) & 255).astype(f) / f(255.0)).astype(f) for s in (16, 8, 0)]
    l = [srgb_to_lrgb(c) for c in ch]
    return (((l[0] + l[1]).astype(f) + l[2]).astype(f) / f(3.0)).astype(f)


def cell_q(img):
    """[h, w] uint32: q(i, j) at [j, i]"""
    w, h = img.shape
    lum = texel_lum(img)
    x1 = np.minimum(np.arange(w) + 1, w - 1)
    y1 = np.minimum(np.arange(h) + 1, h - 1)
    l00, l10, l01, l11 = lum, lum[x1, :], lum[:, y1], lum[x1, :][:, y1]
    m = (((l00 + l10).astype(f) + (l01 + l11).astype(f)).astype(f) * f(0.25)).astype(f)          # [w, h]
    el = ((((np.arange(h).astype(f) + f(0.5)).astype(f) / f(h)).astype(f) - f(0.5)).astype(f) * PI_SCENE).astype(f)
    wgt = (m * cos(el)[None, :]).astype(f)
    s = np.rint((wgt * TWO24).astype(f))
    return np.where(s > 0, s, 0).astype(np.uint32).T.copy()


def table(img, power=1.0):
    w, h = np.asarray(img).shape
    if float(power) == 0.0 or max(w, h) > MAX_DIM or w * h > MAX_CELLS:
        return None
    q = cell_q(img)
    rows = np.cumsum(q.astype(np.uint64), axis=1, dtype=np.uint64)
    marg = np.cumsum(rows[:, -1], dtype=np.uint64)
    total = int(marg[-1])
    if total == 0:
        return None
    return {"w": w, "h": h, "q": q, "row_sums": rows, "marginal": marg, "total": total}


def _pick(cum, k, tot):
    """(entry, offset float32) for one 24-bit integer k; cum a uint64 inclusive sum with cum[-1] == tot; Python integers throughout"""
    prod = int(k) * int(tot)
    t, fb = prod >> 24, prod & 0xFFFFFF
    e = int(np.searchsorted(cum, np.uint64(t), side="right"))
    below = int(cum[e - 1]) if e else 0
    qq = int(cum[e]) - below
    off = ((((t - below) << 24) | fb) // qq)
    assert 0 <= off < (1 << 24)
    return e, f(off) * f(5.9604644775390625e-08)


def direction(tx, ty):
    tx, ty = np.asarray(tx, f), np.asarray(ty, f)
    az = (((tx * f(2.0)).astype(f) * PI_SCENE).astype(f) - PI_SCENE).astype(f)
    el = ((ty - f(0.5)).astype(f) * PI_SCENE).astype(f)
    ce = cos(el)
    return np.stack([(ce * cos(az)).astype(f), sin(el), (ce * sin(az)).astype(f)], axis=-1).astype(f)


def sample(tab, ra, rb):
    ra, rb = np.asarray(ra, f).reshape(-1), np.asarray(rb, f).reshape(-1)
    w, h = tab["w"], tab["h"]
    ka = (ra * TWO24).astype(f).astype(np.uint32) & 0xFFFFFF
    kb = (rb * TWO24).astype(f).astype(np.uint32) & 0xFFFFFF
    n = ra.size
    ci, cj, offx, offy = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, f), np.zeros(n, f)
    for r in range(n):
        j, oy = _pick(tab["marginal"], ka[r], tab["total"])
        i, ox = _pick(tab["row_sums"][j], kb[r], int(tab["row_sums"][j, -1]))
        ci[r], cj[r], offx[r], offy[r] = i, j, ox, oy
    tx = ((ci.astype(f) + offx).astype(f) / f(w)).astype(f)
    ty = ((cj.astype(f) + offy).astype(f) / f(h)).astype(f)
    return ci, cj, tx, ty, direction(tx, ty)


def lookup_coords(d):
    """(dis, tx, ty) of the miss branch (integrator/PT_RGB.py:127-130)"""
    d = np.asarray(d, f).reshape(-1, 3)
    with np.errstate(all="ignore"):
        dis = np.sqrt(((d[:, 0] * d[:, 0]).astype(f) + (d[:, 2] * d[:, 2]).astype(f)).astype(f)).astype(f)
        tx = (((atan2(d[:, 2], d[:, 0]) + PI_SCENE).astype(f) / PI_SCENE).astype(f) / f(2.0)).astype(f)
        ty = ((atan2(d[:, 1], dis) / PI_SCENE).astype(f) + f(0.5)).astype(f)
    return dis, tx, ty


def _cell(t, n):
    x = np.minimum(f(n) - f(1.0), np.maximum(f(0.0), (t * f(n)).astype(f))).astype(f)
    return np.clip(np.floor(x).astype(np.int64), 0, n - 1).astype(np.int32)


def pdf(tab, d):
    w, h = tab["w"], tab["h"]
    dis, tx, ty = lookup_coords(d)
    i, j = _cell(tx, w), _cell(ty, h)
    q = tab["q"][j, i].astype(f)
    with np.errstate(all="ignore"):
        p = (((q / np.uint64(tab["total"]).astype(f)).astype(f) * f(f(w) * f(h))).astype(f) / (TWO_PI_SQ * dis).astype(f)).astype(f)
    return i, j, tx, ty, np.where(dis >= f(0.000001), p, f(0.0)).astype(f)


def env_radiance(img, tx, ty):
    """srgb_to_lrgb(texture2D(env, tx, ty)) [n, 3]: the clamped lookup of texture_expected (wrap 0 applies no step 2; tx, ty are finite)"""
    return srgb_to_lrgb(te.tex_albedo(img, 0, np.asarray(tx, f), np.asarray(ty, f)))


def power_heuristic(a, b):
    a, b = np.asarray(a, f), np.asarray(b, f)
    with np.errstate(all="ignore"):
        t = (a * a).astype(f)
        return (t / ((b * b).astype(f) + t).astype(f)).astype(f)


def nee_env(img, power, tab, p_env, ra, rb, fnormal, throughput, reflect_color, e_brdf, e_pdf, metal):
    """One row's environment sample (step 5): dict with taken, d, expect, c [3].  e_brdf / e_pdf: the Disney evaluation towards d, given by the caller;
    metal: word 5 of the material row (the diffuse lobe is chosen with probability 0.5 * (1 - metal), drawn by cos / pi and stated as 1 / pi)."""
    _, _, _, _, d = sample(tab, [ra], [rb])
    _, _, tx, ty, p = pdf(tab, d)
    fn = np.asarray(fnormal, f)
    ndl = f(f(f(fn[0] * d[0, 0]) + f(fn[1] * d[0, 1])) + f(fn[2] * d[0, 2]))
    out = {"d": d[0], "taken": bool(ndl > 0 and p[0] > 0), "expect": -2, "c": np.zeros(3, f), "pdf": p[0], "ndl": ndl}
    if out["taken"] and e_pdf > 0:
        pdf_l = f(f(p_env) * p[0])
        wgt = f(power_heuristic(pdf_l, f(e_pdf)) / max(f(0.0001), pdf_l))
        c = ((env_radiance(img, tx, ty)[0] * f(power)).astype(f) * wgt).astype(f)
        c = (c * np.asarray(throughput, f)).astype(f)
        c = (c * np.asarray(reflect_color, f)).astype(f)
        c = (c * f(e_brdf)).astype(f)
        c = (c * np.abs(ndl)).astype(f)
        dr = f(f(0.5) * f(f(1.0) - f(metal)))
        drawn = max(f(0.0), f(f(e_pdf) + f(f(dr * f(1.0 / 3.1415956)) * f(ndl - f(1.0)))))
        c = (c * f(drawn / f(e_pdf))).astype(f)
        out["c"], out["expect"] = c, -1
    return out


def _s3(a, b):
    """dot of two float32 triples, ((x + y) + z)"""
    return f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2]))


def _norm1(a):
    a = np.asarray(a, f)
    with np.errstate(all="ignore"):
        inv = f(f(1.0) / _math(7, [_s3(a, a)])[0])
        return (a * inv).astype(f)


SHAPE_SPHERE, SHAPE_SPOT, SHAPE_LASER = 1, 3, 4          # SceneData.py


def nee_light(lrec, light_count, p_env, r, ra, rb, hit_pos, hit_prim, fnormal, view, mat_row, throughput, reflect_color):
    """One row's emitter sample with the table (step 5, "otherwise"): Scene.sample_li on the light records (tirt_shade_table_download, which 1: [lights, 32])
    with the rescaled random r' = (r - p_env) / (1 - p_env) and light_pdf * (1 - p_env).  dict: lidx, taken, o, d, c, expect, dist."""
    one_m = f(f(1.0) - f(p_env))
    with np.errstate(all="ignore"):
        r2 = f(f(f(r) - f(p_env)) / one_m)
        lidx = min(int(f(r2 * f(light_count))), light_count - 1)
        R = np.asarray(lrec[lidx], f).reshape(8, 4)
        kind = int(R[2, 3:4].view(np.int32)[0])
        emission, choice, p0, p1 = np.array([R[3, 3], R[4, 3], R[5, 3]], f), R[1, 3], R[1, 0], R[1, 1]
        a, b = f(ra), f(rb)
        if kind == -1:
            if f(a + b) > f(1.0):
                a, b = f(f(1.0) - a), f(f(1.0) - b)
            lpos = ((R[0, :3] + (R[1, :3] * a).astype(f)).astype(f) + (R[2, :3] * b).astype(f)).astype(f)
            c0 = f(f(f(1.0) - a) - b)
            normal = _norm1((((R[3, :3] * c0).astype(f) + (R[4, :3] * a).astype(f)).astype(f) + (R[5, :3] * b).astype(f)).astype(f))
        elif kind == SHAPE_SPHERE:
            z = f(f(1.0) - f(f(2.0) * a))
            rr = _math(7, [min(f(1.0), max(f(0.0), f(f(1.0) - f(z * z))))])[0]
            phi = f(f(2.0 * 3.1415926) * b)
            normal = np.array([f(rr * cos([phi])[0]), f(rr * sin([phi])[0]), z], f)
            lpos = (R[0, :3] + (normal * p0).astype(f)).astype(f)
        else:
            normal, lpos = R[3, :3].copy(), R[0, :3].copy()
        ln = _norm1(_norm1(normal))
        ld = (np.asarray(hit_pos, f) - lpos).astype(f)
        dist = _math(7, [_s3(ld, ld)])[0]
        ld = (ld / dist).astype(f)
        vis = f(1.0)
        if kind == SHAPE_SPOT:
            x = _math(6, [abs(_s3(ld, ln))])[0]
            if x > p1:
                vis = f(0.0)
            elif x > p0:
                vis = f(f(1.0) * f(f(1.0) - f(f(x - p0) / f(p1 - p0))))
        elif kind == SHAPE_LASER:
            proj = f(_s3(ld, ln) * dist)
            if _math(7, [f(f(dist * dist) - f(proj * proj))])[0] > p0:
                vis = f(0.0)
        em = (emission * vis).astype(f)
        nds, ndl = _s3(np.asarray(fnormal, f), ld), _s3(ln, ld)
        out = {"lidx": lidx, "kind": kind, "taken": bool(nds < 0 and ndl > 0), "o": lpos, "d": ld, "c": np.zeros(3, f), "expect": -2, "dist": dist}
        if out["taken"]:
            ev = np.zeros(2, f)
            oa.load().orc_kat_disney(np.ascontiguousarray(mat_row, f), np.ascontiguousarray(fnormal, f), np.ascontiguousarray(view, f), np.ascontiguousarray(-ld, f), ev)
            lpdf = f(f(f(f(dist * dist) * choice) / ndl) * one_m)
            if ev[1] > 0:
                wgt = f(power_heuristic(lpdf, ev[1]) / max(f(0.0001), lpdf))
                c = (em * wgt).astype(f)
                c = (c * np.asarray(throughput, f)).astype(f)
                c = (c * np.asarray(reflect_color, f)).astype(f)
                c = (c * ev[0]).astype(f)
                c = (c * abs(nds)).astype(f)
                out["c"], out["expect"] = c, int(hit_prim)
    return out


def sun_sky(*a, **kw):
    """scenes.sun_sky_image: [h, w, 3] uint8, one texel at 255 on a floor (row 0 the top of the image)"""
    from ti_raytrace_amd import scenes
    return scenes.sun_sky_image(*a, **kw)


# ---- one shading step with the table (step 5 of include/tirt.h) as a change to the switch-off step ------------------------------------------------
# `lrec`: the light records (which 1: [lights, 32]).  Every row is restated (full is all True, kept for the callers): a row with r >= p_env takes the emitter
# sample of nee_light.
# `off` is the step without the bit (the oracle's orc_kat_shade_step, which the device's other instantiations are held to); `rec` the shading records
# (tirt_shade_table_download, which 0: [n_prims, 32] float32).  Returns (want [n, 28] float32, full [n] bool, branch [n] of str): rows with full == False
# took the emitter sample (r >= p_env) -- their contribution sh_c needs the whole of Scene.sample_li and is not restated here; every other word of
# theirs is, for the rows whose rescaled random names the light the plain random named.
def _dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(f) + a[..., 2] * b[..., 2]).astype(f)


def _normalized(a):
    with np.errstate(all="ignore"):
        inv = (f(1.0) / np.sqrt(_dot(a, a))).astype(f)
        return (a * inv[..., None]).astype(f)


def _rand(seed, pixel, frame, dim):
    L = oa.load()
    return np.array([L.orc_kat_rand(int(s), int(p), int(fr), int(d)) for s, p, fr, d in zip(seed, pixel, frame, dim)], f)


def behind_shading_normal(rows, rec, material_np):
    """indices of the triangle-hit rows on Disney materials with dot(fnormal, -direction) <= 0: the rows where Disney.evaluate_pdf returns pdf -1 for every
    light direction (a tilted vertex normal on the far side of the face), i.e. the rows that force e_pdf <= 0"""
    rows = np.ascontiguousarray(rows)
    rf, ri = rows.view(f), rows.view(np.int32)
    with np.errstate(all="ignore"):
        hit = np.where((rf[:, 11] < f(1000000.0)) & np.isfinite(rf[:, 8:11]).all(axis=1))[0]
        r = rec[ri[hit, 14]].reshape(-1, 8, 4)
        tri = r[:, 1, 3].view(np.int32) == 1
        mtype = material_np[r[:, 0, 3].view(np.int32)][:, 0].astype(np.int32)
        u, v = rf[hit, 12], rf[hit, 13]
        a = ((f(1.0) - u).astype(f) - v).astype(f)
        nn = ((r[:, 3, :3] * a[:, None]).astype(f) + (r[:, 4, :3] * u[:, None]).astype(f)).astype(f) + (r[:, 5, :3] * v[:, None]).astype(f)
        nor = _normalized(nn.astype(f))
        view = (-rf[hit, 8:11]).astype(f)
        sd = _dot(view, r[:, 6, :3])
        fn = (nor * np.sign(sd).astype(f)[:, None]).astype(f)
        return hit[tri & (mtype == 0) & (_dot(fn, view) <= 0) & (sd != 0)]


def step_on(rows, off, rec, material_np, light_count, img, power, tab, share, lrec=None):
    rows = np.ascontiguousarray(rows)
    rf, ri = rows.view(f), rows.view(np.int32)
    n = rows.shape[0]
    want = np.array(off[:, :28], f, copy=True)
    wi = want.view(np.int32)
    full = np.ones(n, bool)
    branch = np.array(["glass_or_dead"] * n, dtype=object)
    p_env = f(1.0) if light_count == 0 else f(share)
    one_m = f(f(1.0) - p_env)
    direction, thr, rad_in, brdf_pdf, spec = rf[:, 8:11], rf[:, 15:18], rf[:, 18:21], rf[:, 21], ri[:, 22]
    t = rf[:, 11]
    with np.errstate(all="ignore"):
        miss = ~(t < f(1000000.0))
        # -- miss: the environment term times its MIS weight
        k = np.where(miss)[0]
        if k.size:
            _, _, tx, ty, p = pdf(tab, direction[k])
            e = env_radiance(img, tx, ty)
            w = np.where(spec[k] == 1, f(1.0), power_heuristic(brdf_pdf[k], (p_env * p).astype(f))).astype(f)
            term = (((e * thr[k]).astype(f) * f(power)).astype(f) * w[:, None]).astype(f)
            want[k, 0:3] = (rad_in[k] + term).astype(f)
            branch[k] = np.where(spec[k] == 1, "miss_spec", "miss_mis")
        # -- hits
        hit = np.where(~miss)[0]
        prim = ri[hit, 14]
        r = rec[prim].reshape(-1, 8, 4)
        mat = r[:, 0, 3].view(np.int32)
        m = material_np[mat]
        mtype = m[:, 0].astype(np.int32)
        tri = r[:, 1, 3].view(np.int32) == 1
        u, v = rf[hit, 12], rf[hit, 13]
        a = ((f(1.0) - u).astype(f) - v).astype(f)
        pos_t = ((r[:, 0, :3] * a[:, None]).astype(f) + (r[:, 1, :3] * u[:, None]).astype(f)).astype(f) + (r[:, 2, :3] * v[:, None]).astype(f)
        nn_t = ((r[:, 3, :3] * a[:, None]).astype(f) + (r[:, 4, :3] * u[:, None]).astype(f)).astype(f) + (r[:, 5, :3] * v[:, None]).astype(f)
        # spheres (hit_attributes_rec): pos = o + d * t, nn = pos - c with the SCALAR c of intersect_sphere
        o, d = rf[hit, 5:8], direction[hit]
        oc = (r[:, 0, :3] - o).astype(f)
        doc2, dop = _dot(oc, oc), _dot(d, oc)
        dcp = np.sqrt((doc2 - (dop * dop).astype(f)).astype(f)).astype(f)
        rad = r[:, 1, 0]
        c_s = np.where(dcp < rad, (doc2 - (rad * rad).astype(f)).astype(f), f(0.0)).astype(f)
        pos_s = (o + (d * t[hit][:, None]).astype(f)).astype(f)
        sphere = ~tri & (r[:, 1, 1].astype(np.int32) == 1)
        nn = np.where(tri[:, None], nn_t.astype(f), np.where(sphere[:, None], (pos_s - c_s[:, None]).astype(f), f(0.0))).astype(f)
        pos = np.where(tri[:, None], pos_t.astype(f), np.where(sphere[:, None], pos_s, f(0.0))).astype(f)
        nor = _normalized(nn)
        gnor = np.where(tri[:, None], r[:, 6, :3], nor).astype(f)
        area = np.where(tri, r[:, 6, 3], r[:, 1, 2]).astype(f)
        # -- emitter hit
        el = mtype == 2
        k = hit[el]
        if k.size:
            fcos = np.abs(_dot(direction[k], gnor[el]))
            ar = (area[el] * f(light_count)).astype(f)
            lpdf = (((t[k] * t[k]).astype(f) / (ar * fcos).astype(f)).astype(f) * one_m).astype(f)
            wgt = power_heuristic(brdf_pdf[k], lpdf)
            mis = (rad_in[k] + ((thr[k] * wgt[:, None]).astype(f) * m[el, 2:5]).astype(f)).astype(f)
            want[k, 0:3] = np.where((spec[k] == 1)[:, None], off[k, 0:3], mis)
            branch[k] = np.where(spec[k] == 1, "emitter_spec", "emitter_mis")
        # -- Disney hit: the light sample
        dis = np.where(mtype == 0)[0]
        k = hit[dis]
        branch[k] = "disney"
        if k.size:
            dim0 = (2 + 8 * ri[k, 3].astype(np.int64)).astype(np.uint32)
            seed, pixel, frame = rows[k, 0], rows[k, 1], rows[k, 2]
            rl = _rand(seed, pixel, frame, dim0)
            take = rl < p_env
            sd = _dot((-d[dis]).astype(f), gnor[dis])
            sgn = np.where(sd > 0, f(1.0), np.where(sd < 0, f(-1.0), f(0.0))).astype(f)
            fn = (nor[dis] * sgn[:, None]).astype(f)
            L = oa.load()
            lrgb = srgb_to_lrgb(m[dis, 2:5])
            for q in np.where(take)[0]:
                row = k[q]
                ra, rb = _rand([seed[q]] * 2, [pixel[q]] * 2, [frame[q]] * 2, [dim0[q] + 1, dim0[q] + 2])
                _, _, _, _, dd = sample(tab, [ra], [rb])
                ev = np.zeros(2, f)
                L.orc_kat_disney(np.ascontiguousarray(m[dis[q]], f), np.ascontiguousarray(fn[q]), np.ascontiguousarray(-d[dis[q]], f), np.ascontiguousarray(dd[0]), ev)
                s = nee_env(img, power, tab, p_env, ra, rb, fn[q], thr[row], lrgb[q], ev[0], ev[1], m[dis[q], 5])
                want[row, 16:28] = 0; wi[row, 26] = -2
                branch[row] = "env_below_horizon"
                if s["taken"]:
                    so = np.zeros(3, f)
                    L.orc_kat_offset_ray(np.ascontiguousarray(pos[dis[q]]), np.ascontiguousarray(fn[q]), so)
                    wi[row, 16] = 1
                    want[row, 17:20], want[row, 20:23], want[row, 23:26], want[row, 27] = so, s["d"], s["c"], SHADOW_DIST
                    wi[row, 26] = s["expect"]
                    branch[row] = "env_taken" if s["expect"] == -1 else "env_pdf0"
            lt = np.where(~take)[0]
            if lt.size and light_count > 0:
                for q in lt:
                    row = k[q]
                    ra, rb = _rand([seed[q]] * 2, [pixel[q]] * 2, [frame[q]] * 2, [dim0[q] + 1, dim0[q] + 2])
                    s = nee_light(lrec, light_count, p_env, rl[q], ra, rb, pos[dis[q]], ri[row, 14], fn[q], (-d[dis[q]]).astype(f), m[dis[q]], thr[row], lrgb[q])
                    plain = min(int(f(rl[q] * f(light_count))), light_count - 1)
                    want[row, 16:28] = 0; wi[row, 26] = -2
                    branch[row] = "light_not_facing"
                    if s["taken"]:
                        wi[row, 16] = 1
                        want[row, 17:20], want[row, 20:23], want[row, 23:26], want[row, 27] = s["o"], s["d"], s["c"], s["dist"]
                        wi[row, 26] = s["expect"]
                        branch[row] = ("light_same" if s["lidx"] == plain else "light_other") if s["expect"] >= 0 else "light_pdf0"
    return want, full, branch
