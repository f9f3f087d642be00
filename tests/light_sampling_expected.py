"""numpy restatement of include/tirt.h, "Choosing emitters by power": weights, quantised weights, prefix sums, the pick, P, and one shading step with the
table as a change to a step without it.  Every float operation is one float32 operation in the header's order; the sums and the inverse are integers.  The GPU
tests hold the device to these bits (tests/test_gpu_light_sampling.py); the host tests hold this file to the header's claims (tests/test_light_sampling_host.py)."""
import numpy as np

f = np.float32
FLT_MAX = f(3.4028234e38)
PI_SCENE = f(3.1415926)
TWO24 = 1 << 24


# ---- steps 1..3 -----------------------------------------------------------------------------------------------------------------------
def _norm3(a):
    with np.errstate(all="ignore"):
        return np.sqrt((((a[..., 0] * a[..., 0]).astype(f) + (a[..., 1] * a[..., 1]).astype(f)).astype(f) + (a[..., 2] * a[..., 2]).astype(f)).astype(f)).astype(f)


def prim_area(vertex, primitive, shape, prim):
    """get_prim_area (Scene.py:324-350) of primitive `prim`: Heron on float32, or r * r * PI_SCENE for a sphere, spot or laser"""
    pr = primitive[prim]
    with np.errstate(all="ignore"):
        if pr[0] == 1:
            v1, v2, v3 = (np.asarray(vertex[pr[1] + k, 0:3], f) for k in range(3))
            a, b, c = _norm3((v1 - v2).astype(f)), _norm3((v1 - v3).astype(f)), _norm3((v3 - v2).astype(f))
            s = f(f(f(a + b) + c) * f(0.5))
            return np.sqrt(f(f(f(s * f(s - a)) * f(s - b)) * f(s - c))).astype(f)
        sh = shape[pr[1]]
        if int(sh[0]) in (1, 3, 4):
            return f(f(f(sh[4]) * f(sh[4])) * PI_SCENE)
        return f(0.0)


def scene_lists(scene):
    """(emission [N, 3], area [N]) of the light list of a packed host scene (Scene.setup_data_cpu)"""
    n = scene.light_count
    em = np.zeros((n, 3), f); area = np.zeros(n, f)
    for i in range(n):
        prim = int(scene.light_np[i])
        em[i] = scene.material_np[scene.primitive_np[prim, 2], 2:5]
        area[i] = prim_area(scene.vertex_np, scene.primitive_np, scene.shape_np, prim)
    return em, area


def record_lists(lrec):
    """(emission [N, 3], area [N]) from the light records (tirt_shade_table_download, which 1: [N, 8, 4]), where the device takes them from"""
    r = np.asarray(lrec, f).reshape(-1, 8, 4)
    return np.stack([r[:, 3, 3], r[:, 4, 3], r[:, 5, 3]], axis=1), r[:, 0, 3].copy()


def weights(emission, area):
    em = np.asarray(emission, f).reshape(-1, 3)
    with np.errstate(all="ignore"):
        level = ((em[:, 0] + em[:, 1]).astype(f) + em[:, 2]).astype(f) / f(3.0)
        return (level.astype(f) * np.asarray(area, f)).astype(f)


def table(emission, area, u=0.0):
    """{"n", "w", "e_max", "q" uint32, "prefix" uint64, "total" int, "u", "P" float32}"""
    w = weights(emission, area)
    with np.errstate(all="ignore"):
        part = (w > 0) & (w <= FLT_MAX)
    n = w.shape[0]
    q = np.zeros(n, np.uint32)
    e_max = 0
    if part.any():
        e_max = int(np.frexp(w[part].max())[1])
        s = np.rint(np.ldexp(w[part], 24 - e_max).astype(f))
        q[part] = np.maximum(s, 1).astype(np.uint32)
    prefix = np.cumsum(q.astype(np.uint64), dtype=np.uint64)
    total = int(prefix[-1]) if n else 0
    tab = {"n": n, "w": w, "e_max": e_max, "q": q, "prefix": prefix, "total": total, "u": f(u)}
    tab["P"] = choice_P(tab, np.arange(n)) if total else np.zeros(n, f)
    return tab


def choice_P(tab, i):
    """P_i = u / N + (1 - u) * ((float)q_i / (float)total)"""
    u, n = tab["u"], tab["n"]
    qf = tab["q"][i].astype(np.uint64).astype(f)
    return (f(u / f(n)) + (f(f(1.0) - u) * (qf / f(np.uint64(tab["total"]))).astype(f)).astype(f)).astype(f)


def pick(tab, r):
    """(index int32 [m], P float32 [m], uniform bool [m]) for light randoms r in [0, 1]"""
    r = np.asarray(r, f).reshape(-1)
    u, n, total = tab["u"], tab["n"], tab["total"]
    idx = np.zeros(r.shape[0], np.int32)
    uni = r < u
    with np.errstate(all="ignore"):
        if uni.any():
            idx[uni] = np.minimum(((r[uni] / u).astype(f) * f(n)).astype(f).astype(np.int64), n - 1)
        rest = ~uni
        k = np.minimum((((r[rest] - u).astype(f) / f(f(1.0) - u)).astype(f) * f(TWO24)).astype(f).astype(np.int64), TWO24 - 1)
    if total < 1 << 40:                                                   # k * total fits 64 bits
        t = (k.astype(np.uint64) * np.uint64(total)) >> np.uint64(24)
    else:
        t = np.array([(int(x) * total) >> 24 for x in k], np.uint64)
    idx[rest] = np.searchsorted(tab["prefix"], t, side="right").astype(np.int32)
    return idx, choice_P(tab, idx), uni


# ---- step 5: one shading step with the table, as a change to the step of the same instantiation without bit 4096 --------------------------
def _ee():
    import env_sampling_expected as ee
    return ee


def nee_light(tab, lrec, p_env, r, ra, rb, hit_pos, hit_prim, fnormal, view, mat_row, throughput, reflect_color):
    """One row's emitter sample: Scene.sample_li on the light records with the entry and P of step 4 in the place of lidx and 1 / (N * area).  Under bit 1024 the
    random is the rescaled one and light_pdf carries (1 - p_env) (p_env = 0 otherwise: both are then exact identities).  dict: lidx, uniform, taken, o, d, c, expect, dist."""
    ee = _ee()
    one_m = f(f(1.0) - f(p_env))
    with np.errstate(all="ignore"):
        r2 = f(f(f(r) - f(p_env)) / one_m)
        li, P, uni = pick(tab, [r2])
        lidx = int(li[0])
        R = np.asarray(lrec[lidx], f).reshape(8, 4)
        kind = int(R[2, 3:4].view(np.int32)[0])
        emission, area, p0 = np.array([R[3, 3], R[4, 3], R[5, 3]], f), R[0, 3], R[1, 0]
        choice = f(P[0] / area)
        a, b = f(ra), f(rb)
        if kind == -1:
            if f(a + b) > f(1.0):
                a, b = f(f(1.0) - a), f(f(1.0) - b)
            lpos = ((R[0, :3] + (R[1, :3] * a).astype(f)).astype(f) + (R[2, :3] * b).astype(f)).astype(f)
            c0 = f(f(f(1.0) - a) - b)
            normal = ee._norm1((((R[3, :3] * c0).astype(f) + (R[4, :3] * a).astype(f)).astype(f) + (R[5, :3] * b).astype(f)).astype(f))
        else:
            assert kind == ee.SHAPE_SPHERE, kind
            z = f(f(1.0) - f(f(2.0) * a))
            rr = ee._math(7, [min(f(1.0), max(f(0.0), f(f(1.0) - f(z * z))))])[0]
            phi = f(f(2.0 * 3.1415926) * b)
            normal = np.array([f(rr * ee.cos([phi])[0]), f(rr * ee.sin([phi])[0]), z], f)
            lpos = (R[0, :3] + (normal * p0).astype(f)).astype(f)
        ln = ee._norm1(ee._norm1(normal))
        ld = (np.asarray(hit_pos, f) - lpos).astype(f)
        dist = ee._math(7, [ee._s3(ld, ld)])[0]
        ld = (ld / dist).astype(f)
        nds, ndl = ee._s3(np.asarray(fnormal, f), ld), ee._s3(ln, ld)
        out = {"lidx": lidx, "uniform": bool(uni[0]), "taken": bool(nds < 0 and ndl > 0), "o": lpos, "d": ld, "c": np.zeros(3, f), "expect": -2, "dist": dist}
        if out["taken"]:
            ev = np.zeros(2, f)
            ee.oa.load().orc_kat_disney(np.ascontiguousarray(mat_row, f), np.ascontiguousarray(fnormal, f), np.ascontiguousarray(view, f), np.ascontiguousarray(-ld, f), ev)
            lpdf = f(f(f(f(dist * dist) * choice) / ndl) * one_m)
            if ev[1] > 0:
                wgt = f(ee.power_heuristic(lpdf, ev[1]) / max(f(0.0001), lpdf))
                c = (emission * wgt).astype(f)
                c = (c * np.asarray(throughput, f)).astype(f)
                c = (c * np.asarray(reflect_color, f)).astype(f)
                c = (c * ev[0]).astype(f)
                c = (c * abs(nds)).astype(f)
                out["c"], out["expect"] = c, int(hit_prim)
    return out


def step_on(rows, base, rec, material_np, tab, lrec, phit, p_env=0.0, with_mask=False):
    """`base`: the step of the sibling instantiation (no bit 4096) on the same rows, [n, 28]; `rec` the shading records [n_prims, 32] WITHOUT the spare words,
    `phit` [n_prims] the P of the entry naming each primitive (0 elsewhere); `p_env`: the environment's share under bit 1024, else 0.  Rows must have finite
    directions.  Returns (want [n, 28], branch [n] of str): rows of the branches "emitter_mis", "light_*" are restated, every other row is the sibling's.  with_mask: also `over` [n, 28] bool, the words that were restated (they do not depend on `base`)."""
    ee = _ee()
    rows = np.ascontiguousarray(rows)
    rf, ri = rows.view(f), rows.view(np.int32)
    n = rows.shape[0]
    want = np.array(base[:, :28], f, copy=True)
    wi = want.view(np.int32)
    branch = np.array(["other"] * n, dtype=object)
    over = np.zeros((n, 28), bool)
    p_env = f(p_env)
    one_m = f(f(1.0) - p_env)
    direction, thr, rad_in, brdf_pdf, spec = rf[:, 8:11], rf[:, 15:18], rf[:, 18:21], rf[:, 21], ri[:, 22]
    t = rf[:, 11]
    with np.errstate(all="ignore"):
        hit = np.where(t < f(1000000.0))[0]
        prim = ri[hit, 14]
        r = rec[prim].reshape(-1, 8, 4)
        m = material_np[r[:, 0, 3].view(np.int32)]
        mtype = m[:, 0].astype(np.int32)
        tri = r[:, 1, 3].view(np.int32) == 1
        u, v = rf[hit, 12], rf[hit, 13]
        a = ((f(1.0) - u).astype(f) - v).astype(f)
        pos_t = ((r[:, 0, :3] * a[:, None]).astype(f) + (r[:, 1, :3] * u[:, None]).astype(f)).astype(f) + (r[:, 2, :3] * v[:, None]).astype(f)
        nn_t = ((r[:, 3, :3] * a[:, None]).astype(f) + (r[:, 4, :3] * u[:, None]).astype(f)).astype(f) + (r[:, 5, :3] * v[:, None]).astype(f)
        o, d = rf[hit, 5:8], direction[hit]
        oc = (r[:, 0, :3] - o).astype(f)
        doc2, dop = ee._dot(oc, oc), ee._dot(d, oc)
        dcp = np.sqrt((doc2 - (dop * dop).astype(f)).astype(f)).astype(f)
        rad = r[:, 1, 0]
        c_s = np.where(dcp < rad, (doc2 - (rad * rad).astype(f)).astype(f), f(0.0)).astype(f)
        pos_s = (o + (d * t[hit][:, None]).astype(f)).astype(f)
        sphere = ~tri & (r[:, 1, 1].astype(np.int32) == 1)
        nn = np.where(tri[:, None], nn_t.astype(f), np.where(sphere[:, None], (pos_s - c_s[:, None]).astype(f), f(0.0))).astype(f)
        pos = np.where(tri[:, None], pos_t.astype(f), np.where(sphere[:, None], pos_s, f(0.0))).astype(f)
        nor = ee._normalized(nn)
        gnor = np.where(tri[:, None], r[:, 6, :3], nor).astype(f)
        area = np.where(tri, r[:, 6, 3], r[:, 1, 2]).astype(f)
        # -- emitter hit: light_pdf = (t * t) * (P_hit / area) / fCosTheta [* (1 - p_env)]
        el = mtype == 2
        k = hit[el]
        if k.size:
            fcos = np.abs(ee._dot(direction[k], gnor[el]))
            lpdf = (((t[k] * t[k]).astype(f) * (phit[prim[el]].astype(f) / area[el]).astype(f)).astype(f) / fcos).astype(f)
            if p_env != 0:
                lpdf = (lpdf * one_m).astype(f)
            wgt = ee.power_heuristic(brdf_pdf[k], lpdf)
            mis = (rad_in[k] + ((thr[k] * wgt[:, None]).astype(f) * m[el, 2:5]).astype(f)).astype(f)
            want[k, 0:3] = np.where((spec[k] == 1)[:, None], base[k, 0:3], mis)
            over[k, 0:3] = (spec[k] != 1)[:, None]
            branch[k] = np.where(spec[k] == 1, "emitter_spec", "emitter_mis")
        # -- Disney hit: the light sample
        dis = np.where(mtype == 0)[0]
        k = hit[dis]
        if k.size:
            dim0 = (2 + 8 * ri[k, 3].astype(np.int64)).astype(np.uint32)
            seed, pixel, frame = rows[k, 0], rows[k, 1], rows[k, 2]
            rl = ee._rand(seed, pixel, frame, dim0)
            sd = ee._dot((-d[dis]).astype(f), gnor[dis])
            sgn = np.where(sd > 0, f(1.0), np.where(sd < 0, f(-1.0), f(0.0))).astype(f)
            fn = (nor[dis] * sgn[:, None]).astype(f)
            lrgb = ee.srgb_to_lrgb(m[dis, 2:5])
            for q in np.where(~(rl < p_env))[0]:
                row = k[q]
                ra, rb = ee._rand([seed[q]] * 2, [pixel[q]] * 2, [frame[q]] * 2, [dim0[q] + 1, dim0[q] + 2])
                s = nee_light(tab, lrec, p_env, rl[q], ra, rb, pos[dis[q]], ri[row, 14], fn[q], (-d[dis[q]]).astype(f), m[dis[q]], thr[row], lrgb[q])
                want[row, 16:28] = 0; wi[row, 26] = -2
                over[row, 16:28] = True
                branch[row] = "light_not_facing"
                if s["taken"]:
                    wi[row, 16] = 1
                    want[row, 17:20], want[row, 20:23], want[row, 23:26], want[row, 27] = s["o"], s["d"], s["c"], s["dist"]
                    wi[row, 26] = s["expect"]
                    branch[row] = ("light_uniform" if s["uniform"] else "light_power") if s["expect"] >= 0 else "light_pdf0"
    return (want, branch, over) if with_mask else (want, branch)


# ---- a small direct-lighting estimator on host tables (tests/test_light_sampling_host.py) ----------------------------------------------------
def direct_light_samples(scene, tab, point, normal, count, seed):
    """`count` one-sample estimates of the irradiance-weighted radiance a Lambertian point receives from the triangle emitters of a packed host scene, the
    emitter drawn with the probabilities tab["P"], the point uniformly on it.  float64: this is about the estimator's statistics, not about bits."""
    rng = np.random.RandomState(seed)
    P = tab["P"].astype(np.float64)
    P = P / P.sum()
    idx = rng.choice(tab["n"], size=count, p=P)
    prim = scene.light_np[idx]
    v0 = scene.primitive_np[prim, 1]
    p1, p2, p3 = (scene.vertex_np[v0 + k, 0:3].astype(np.float64) for k in range(3))
    e = scene.material_np[scene.primitive_np[prim, 2], 2:5].astype(np.float64).mean(axis=1)
    a, b = rng.rand(count), rng.rand(count)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    x = p1 + (p3 - p1) * a[:, None] + (p2 - p1) * b[:, None]
    cr = np.cross(p2 - p1, p3 - p1)
    area = 0.5 * np.linalg.norm(cr, axis=1)
    ln = cr / np.linalg.norm(cr, axis=1, keepdims=True)
    dvec = x - np.asarray(point, np.float64)
    dist = np.linalg.norm(dvec, axis=1)
    wdir = dvec / dist[:, None]
    cos_s = np.maximum(0.0, wdir @ np.asarray(normal, np.float64))
    cos_l = np.maximum(0.0, -(wdir * ln).sum(axis=1))
    return e * cos_s * cos_l / (dist * dist) * area / P[idx]
