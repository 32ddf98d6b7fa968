"""AOIntegrator::Li (pbrt-v3 src/integrators/ao.cpp:57-103) restated in numpy for triangle scenes: the float64 truth the device's
ambient occlusion integrator is held to (no oracle has AO), the same formulas in float32, the small scenes both are used on, and
the closed forms.

`li(tri_p, flags, cam_o, cam_d, u, cossample, dtype)` takes the triangles and flag words `HostScene.bvh()` / `prim_flags()` return (BVH
order), camera rays and, per camera sample, the nsamples entries u[i, j] of the sampler's 2D array, and returns an `AoTruth`:

    L      (n,)  the sum over j, in j order, of Dot(wi, n) / (pdf * nSamples) over the unoccluded rays; 0 where the camera ray misses
    hit    (n,)  the camera ray found a surface
    kept   (n,)  the camera ray and all its occlusion rays are `decided` in trace_ref's sense, and no occlusion ray leaves the
                 surface at |wi.z| < trace_ref.GRAZE (local frame): only those samples are compared

The closest hit and every occlusion query go through `trace_ref.brute_force`, so no tree is read. The frame is built from the
triangle's vertices: n = Normalize(Cross(p0 - p2, p1 - p2)), negated under IILE_PRIM_FLIP, dp/du from the (default or given) uv as
Triangle::Intersect has it; s = Normalize(dpdu), t = Cross(n, s) with the n that is NOT face-forwarded, wi = s x + t y + nf z with
nf = Faceforward(n, -d), as the reference has it (ao.cpp:77-79, 94-96). An occlusion ray starts at the hit point itself and is
tested against every triangle but its own (a plane cannot occlude the half space above it; pbrt gets the same from
OffsetRayOrigin), so the truth needs no epsilon.

dtype = float32 evaluates the same formulas — hemisphere maps, frame, wi, pdf, the term and the running sum — in float32 numpy from
the same hits (the occlusion queries stay brute force on the float32 rays). It is a restatement, not the code under test.

BAND, the per-sample band for |L_device - L_float64|, is 4 x the worst |L_float32 - L_float64| of that restatement over the kept
samples of the scenes of `cases()` (the GPU test's: 16 x 16, 2 spp, nsamples 16). Measured on the CPU by `python tests/ao_ref.py`
(measure()), which printed

    halton_cos: kept 1.0000 (hits 0.502), worst |L32 - L64| over kept 1.041e-06
    halton_uniform: kept 0.9160 (hits 0.502), worst |L32 - L64| over kept 6.886e-07
    sobol_cos: kept 1.0000 (hits 0.506), worst |L32 - L64| over kept 1.041e-06
    halton_cos_reversed: kept 1.0000 (hits 0.502), worst |L32 - L64| over kept 1.041e-06

so BAND = 4 x 1.041e-06 = 4.164e-06. (Under uniform sampling one ray in a hundred leaves below GRAZE, so some 15 % of the hits hold
one among their 16: the camera looks half into the sky so that the kept share stays above 0.9.)
"""
import numpy as np

import trace_ref

HEADER = """LookAt {eye} {look} {up}
Camera "perspective" "float fov" [{fov}]
Film "image" "integer xresolution" [{w}] "integer yresolution" [{h}] "string filename" "ao.pfm"{crop}
Sampler "{sampler}" "integer pixelsamples" [{spp}]
Integrator "{integrator}"{params}
WorldBegin
"""


def scene_text(body, w=16, h=16, spp=2, fov=60, eye="0 0 -5", look="0 0 0", up="0 1 0", sampler="halton", integrator="ambientocclusion",
               nsamples=None, cossample=None, crop=None, params=""):
    if nsamples is not None:
        params += f' "integer nsamples" [{nsamples}]'
    if cossample is not None:
        params += f' "bool cossample" "{"true" if cossample else "false"}"'
    crop = "" if crop is None else ' "float cropwindow" [' + " ".join(str(c) for c in crop) + "]"
    return HEADER.format(eye=eye, look=look, up=up, fov=fov, w=w, h=h, spp=spp, sampler=sampler, integrator=integrator, params=params,
                         crop=crop) + body + "\nWorldEnd\n"


def write_scene(tmp_path, body, name="ao.pbrt", **kw):
    p = tmp_path / name
    p.write_text(scene_text(body, **kw))
    return str(p)


def quad(p0, p1, p2, p3):
    pts = " ".join(f"{c:g}" for p in (p0, p1, p2, p3) for c in p)
    return f'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [{pts}]\n'


def box(lo, hi):
    """The 12 triangles of an axis-aligned box."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    idx = [0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 3, 7, 6, 3, 6, 2, 0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5]
    pts = " ".join(f"{v:g}" for p in c for v in p)
    return f'Shape "trianglemesh" "integer indices" [{" ".join(map(str, idx))}] "point P" [{pts}]\n'


FLOOR = quad((-4, -1, -4), (4, -1, -4), (4, -1, 4), (-4, -1, 4))
OCCLUDER = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-2.5 -0.2 0.5  1.5 0.6 -0.5  0.2 1.4 2.5]\n'
BOX = box((0.6, -1, -0.9), (1.7, 0.1, 0.4))
CAMERA = dict(eye="0.4 2.2 -5.5", look="0 0.5 0", fov=60)   # about half sky: under uniform sampling 15 % of the hits hold a grazing ray


def truth_body(reverse_floor=False):
    """The `Li` scene: a floor quad, a tilted occluding triangle and a 12-triangle box."""
    floor = ("AttributeBegin\nReverseOrientation\n" + FLOOR + "AttributeEnd\n") if reverse_floor else FLOOR
    return 'Material "matte"\n' + floor + OCCLUDER + BOX


def cases():
    """(name, scene keywords) of the per-sample `Li` cases: cossample true / false under Halton, one Sobol' case, one with the floor's
    orientation reversed."""
    base = dict(w=16, h=16, spp=2, nsamples=16, **CAMERA)
    return [("halton_cos", dict(base, cossample=True), False), ("halton_uniform", dict(base, cossample=False), False),
            ("sobol_cos", dict(base, cossample=True, sampler="sobol"), False), ("halton_cos_reversed", dict(base, cossample=True), True)]


# ---- the hemisphere maps (core/sampling.cpp:89-96, 113-130; core/sampling.h:159-165) -------------------------------------------
def concentric_disk(u, dt):
    one, two = dt(1), dt(2)
    ox, oy = two * u[..., 0] - one, two * u[..., 1] - one
    zero = (ox == 0) & (oy == 0)
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, ox, oy)
        theta = np.where(first, dt(np.pi / 4) * (oy / ox), dt(np.pi / 2) - dt(np.pi / 4) * (ox / oy))
    theta = np.where(zero, dt(0), theta).astype(dt)
    r = np.where(zero, dt(0), r).astype(dt)
    return r * np.cos(theta), r * np.sin(theta)


def cosine_hemisphere(u, dt):
    x, y = concentric_disk(u, dt)
    z = np.sqrt(np.maximum(dt(0), dt(1) - x * x - y * y))
    return np.stack([x, y, z], -1), np.abs(z) * dt(1 / np.pi)


def uniform_hemisphere(u, dt):
    z = u[..., 0]
    r = np.sqrt(np.maximum(dt(0), dt(1) - z * z))
    phi = dt(2) * dt(np.pi) * u[..., 1]
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1), np.full(z.shape, dt(1 / (2 * np.pi)), dt)


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def frames(P, flags, prim, cam_d, dt, uv=None):
    """(n, s, t, nf) of the hits on triangles `prim` (triangle.cpp:277-330 for n and dp/du, ao.cpp:77-79 for the rest)."""
    T = P[prim].astype(dt)
    p0, p1, p2 = T[:, 0:3], T[:, 3:6], T[:, 6:9]
    uvs = np.broadcast_to(np.array([0, 0, 1, 0, 1, 1], dt), (len(prim), 6)) if uv is None else np.asarray(uv, dt)[prim]
    duv02, duv12 = uvs[:, 0:2] - uvs[:, 4:6], uvs[:, 2:4] - uvs[:, 4:6]
    dp02, dp12 = p0 - p2, p1 - p2
    det = duv02[:, 0] * duv12[:, 1] - duv02[:, 1] * duv12[:, 0]
    dpdu = (duv12[:, 1:2] * dp02 - duv02[:, 1:2] * dp12) * (dt(1) / det)[:, None]
    n = _unit(np.cross(dp02, dp12))
    n = np.where(((flags[prim] & 8) != 0)[:, None], -n, n)
    s = _unit(dpdu)
    t = np.cross(n, s)
    nf = np.where(((n * -cam_d.astype(dt)).sum(1) < 0)[:, None], -n, n)
    return n, s, t, nf


class AoTruth:
    pass


def li(tri_p, flags, cam_o, cam_d, u, cossample, dtype=np.float64, uv=None):
    dt = dtype
    P = np.asarray(tri_p, np.float64).reshape(-1, 9)
    flags = np.asarray(flags)
    cam_o, cam_d = np.asarray(cam_o, np.float64).reshape(-1, 3), np.asarray(cam_d, np.float64).reshape(-1, 3)
    u = np.asarray(u, dt)
    n_cam, n_s = u.shape[0], u.shape[1]
    first = trace_ref.brute_force(P, cam_o, cam_d, np.full(n_cam, np.inf))
    r = AoTruth()
    r.hit = first.hit.copy()
    r.kept = first.decided.copy()
    r.L = np.zeros(n_cam, dt)
    idx = np.nonzero(first.hit)[0]
    if len(idx) == 0:
        return r
    # the camera ray's triangle: the nearest of its ties (a tie between two triangles is undecided or an abutting edge)
    tt = np.where(first.ties[idx], 0, 1)
    prim = tt.argmin(1)
    d = cam_d[idx]
    p = (cam_o[idx] + d * first.t_min[idx, None]).astype(dt)
    n, s, t, nf = frames(P, flags, prim, d, dt, uv)
    wl, pdf = (cosine_hemisphere if cossample else uniform_hemisphere)(u[idx], dt)   # (h, n_s, 3), (h, n_s)
    wi = s[:, None, :] * wl[..., 0:1] + t[:, None, :] * wl[..., 1:2] + nf[:, None, :] * wl[..., 2:3]
    with np.errstate(divide="ignore", invalid="ignore"):
        term = ((wi * nf[:, None, :]).sum(-1) / (pdf * dt(n_s))).astype(dt)
    occluded = np.zeros((len(idx), n_s), bool)
    decided = np.ones((len(idx), n_s), bool)
    for own in np.unique(prim):   # every triangle but the ray's own
        rows = np.nonzero(prim == own)[0]
        others = np.delete(P, own, axis=0)
        o = np.repeat(p[rows], n_s, axis=0).astype(np.float64)
        w = wi[rows].reshape(-1, 3).astype(np.float64)
        tr = trace_ref.brute_force(others, o, w, np.full(len(o), np.inf))
        occluded[rows] = tr.any_hit().reshape(len(rows), n_s)
        decided[rows] = tr.decided.reshape(len(rows), n_s)
    L = np.zeros(len(idx), dt)
    for j in range(n_s):   # `for (int i = 0; i < nSamples; ++i) if (!IntersectP) L += ...`: in order
        L = np.where(occluded[:, j], L, (L + term[:, j]).astype(dt)).astype(dt)
    r.L[idx] = L
    r.kept[idx] &= decided.all(1) & (np.abs(wl[..., 2]) >= trace_ref.GRAZE).all(1)
    r.prim = np.full(n_cam, -1)
    r.prim[idx] = prim
    return r


# ---- the inputs of a frame's camera samples, from the CPU oracle's sampler and camera ------------------------------------------
def sample_inputs(oracle, host, nsamples, px, py, k):
    """Camera rays (float32) and the (n, nsamples, 2) array entries of camera samples (px, py, k): entry j is dimensions 5 and 6 of
    the pixel's sample k nsamples + j (GlobalSampler::StartPixel, sampler.cpp:136-166)."""
    n = len(px)
    pfilm = np.empty((n, 2), np.float32)
    u = np.empty((n, nsamples, 2), np.float32)
    for i in range(n):
        x, y, kk = int(px[i]), int(py[i]), int(k[i])
        idx = oracle.sample_index(host, x, y, kk)
        pfilm[i] = (np.float32(x) + oracle.sample_dimension(host, idx, 0, x, y), np.float32(y) + oracle.sample_dimension(host, idx, 1, x, y))
        for j in range(nsamples):
            ia = oracle.sample_index(host, x, y, kk * nsamples + j)
            u[i, j] = (oracle.sample_dimension(host, ia, 5, x, y), oracle.sample_dimension(host, ia, 6, x, y))
    o, d = oracle.camera_rays(host, pfilm)
    return o, d, u


def frame_samples(host):
    """(px, py, k) of every camera sample of the scene's film (its sample bounds are the pixel bounds under the box filter)."""
    f = host.film
    ys, xs, ks = np.meshgrid(np.arange(f.samp_y0, f.samp_y1), np.arange(f.samp_x0, f.samp_x1), np.arange(host.info["spp"]), indexing="ij")
    return xs.ravel().astype(np.int32), ys.ravel().astype(np.int32), ks.ravel().astype(np.int32)


_CACHE = {}


def case_truth(binding, oracle, tmp_path_factory, case):
    """The float64 truth of one of cases(), computed once per session: (host, px, py, k, AoTruth)."""
    if case not in _CACHE:
        name, kw, reverse = cases()[case]
        path = write_scene(tmp_path_factory.mktemp("ao_truth"), truth_body(reverse), name=name + ".pbrt", **kw)
        host = binding.HostScene(path=path)
        px, py, k = frame_samples(host)
        o, d, u = sample_inputs(oracle, host, kw["nsamples"], px, py, k)
        _, tri_p, _ = host.bvh()
        tr = li(tri_p, host.prim_flags(), o, d, u, kw["cossample"])
        _CACHE[case] = (host, px, py, k, tr, (tri_p, o, d, u))
    return _CACHE[case]


# ---- closed forms --------------------------------------------------------------------------------------------------------------
def unoccluded():
    """Li of a point that sees nothing, per camera sample, under cosine sampling: every term is Dot(wi, n) / (cos / pi * n) = pi / n."""
    return np.pi


def under_disk(h, rho, r):
    """Li at a point of a plane a height h below a facing disk of radius r, rho off its axis: pi (1 - F), F the disk's form factor
    (quadric_ref.disk_irradiance_factor) — the estimator is that of the cosine-weighted visible solid angle under either sampling."""
    from quadric_ref import disk_irradiance_factor
    return np.pi * (1 - disk_irradiance_factor(h, rho, r))


# what measure() printed: per case the kept share and the worst |L_float32 - L_float64| over the kept samples
MEASURED = {"halton_cos": (1.0000, 1.041e-06), "halton_uniform": (0.9160, 6.886e-07), "sobol_cos": (1.0000, 1.041e-06),
            "halton_cos_reversed": (1.0000, 1.041e-06)}
BAND = 4 * 1.041e-06   # on L of the order of pi: some 17 units in the last place of a float32 sum of 16 terms


def measure():
    """python tests/ao_ref.py: the float32 restatement against the float64 truth on the scenes of cases()."""
    import pathlib
    import sys
    import tempfile
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
    import conftest
    import oracle_binding
    import __graft_entry__ as ge
    ge.build_if_needed()
    binding, oracle = conftest.load_binding(), oracle_binding.Oracle()

    class Factory:
        def mktemp(self, name):
            return pathlib.Path(tempfile.mkdtemp(prefix=name))
    worst = 0.0
    for c, (name, kw, _) in enumerate(cases()):
        host, px, py, k, tr, (tri_p, o, d, u) = case_truth(binding, oracle, Factory(), c)
        t32 = li(tri_p, host.prim_flags(), o, d, u, kw["cossample"], np.float32)
        keep = tr.kept & t32.kept
        err = np.abs(t32.L.astype(np.float64) - tr.L)[keep]
        print(f"{name}: kept {tr.kept.mean():.4f} (hits {tr.hit.mean():.3f}), worst |L32 - L64| over kept {err.max():.3e}, mean L {tr.L[keep].mean():.4f}")
        worst = max(worst, float(err.max()))
    print(f"worst {worst:.3e}; BAND = 4 x worst = {4 * worst:.3e}")


if __name__ == "__main__":
    measure()
