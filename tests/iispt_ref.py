"""The IISPT render runner, from hemi point to film pixel (pbrt-v3-IISPT src/integrators/iisptrenderrunner.cpp), restated in numpy
for small scenes: the float64 truth the oracle's and the device's iispt_hemi_points / iispt_gather / film monitors are held to, and
the same formulas in float32.

Written from the reference sources alone (line numbers are the reference's own). What is restated here:

  the hemi grid     iisptrenderrunner.cpp:249-258, 381-410: hemi points from (x0, y0) every `tilesize` pixels and at x1 - 1 / y1 - 1,
                    row by row; the four neighbours of a film pixel :434-464, IN THE ORDER OF neighbour_points[]: S, E, R, B (the
                    comment at :418-422 names another order; the array is what compute_fpixel_weights and sample_hemisphere walk,
                    hence the order of the random draws), with the min(.., x1 - 1) clamp
  the camera sample sampler_next_pixel (:943-956) puts the sampler on pixel (counter + 1, 0) before every item, hemi points first
                    (:262-265), then film pixels (:490-492); GetCameraSample(pixel) (sampler.cpp:41-47): pFilm = pixel + dims 0-1,
                    time dim 2, lens dims 3-4; find_intersection's Get2D calls start at dimension 5. The truth works out pixel,
                    index (sample 0 of that pixel) and dimension; the VALUES are the oracle's sample_dimension, pinned by the
                    Halton known answers; the camera ray is the oracle's camera_rays of that pFilm (held to camera truths elsewhere)
  first vertex      find_intersection (:657-757): scene.Intersect, Sample_f with BSDF_ALL (allowMultipleLobes = true: smooth glass is
                    one FresnelSpecular lobe), the black exit (f black or pdf 0: beta 0), the first non-specular vertex (beta not
                    updated), beta *= f AbsDot(wi, ns) / pdf along the specular chain, the beta.y() < 0 exit, 24 iterations;
                    "has a vertex" is `returned true and beta.y() > 0` (:293, :519-528)
  the aux ray       :300-314, :973-985: isect.n turned against ray.d (Dot > 0), SpawnRay along it. The truth has no OffsetRayOrigin:
                    its origin is the hit point itself (see hemi_point_bound)
  hemi camera       CreateHemisphericCamera (cameras/hemispheric.cpp:108-158): up = (0, 1, 0) when dir.x == dir.y == 0, else
                    (0, 0, 1); look = pos + dir; LookAt (core/transform.cpp:203-236): dir = Normalize(look - pos), right =
                    Normalize(Cross(Normalize(up), dir)), newUp = Cross(dir, right), camera-to-world columns right, newUp, dir;
                    get_light_sample_nn (:89-105): theta = Pi y / h, phi = Pi x / w, (sin theta cos phi, cos theta, sin theta sin phi)
                    to world; getLightSampleNn (:44-60): to camera space, theta = acos(y), phi = atan2(z, x), the int conversions
                    (truncation towards zero: phi in (-Pi / hemi, 0) still reads column 0), black outside the film;
                    get_camera_coord_jacobian (film/intensityfilm.cpp:53-66): image row hemi - 1 - y (ImageFilm::get, imagefilm.cpp:34-39,
                    over populate_from_float_array's order :176-200: row 0 is the first the network emits) times sin(M_PI (y / hemi))
  the gather        compute_fpixel_weights (:961-1037) over tools/iisptmathutils.h:43-53, 69-143, 189-205: wdpos, wdnor, wdd (zeros
                    for a missing camera), wod, max(0.0, 2.0 - wod) + 0.001 in double, the normalisation by the float total;
                    sample_hemisphere (:142-178): 16 tries per neighbour, rr < weight, samples_taken counted with or without a
                    camera, rx then ry from uniform_uint32(hemi), L / samples_taken; estimate_direct (:16-138): lightPdf = 1.0 / 6.28,
                    EM_RATIO 1.098, BSDF_RATIO 0.4394, both halves with PowerHeuristic (sampling.h:147-150); the pixel's record
                    f_beta * L with weight 0.5 (:575-577). The main camera's origin is getCameraWorldPosition (core/camera.cpp:115-124)
  random numbers    core/rng.h:62-156 in exact integer arithmetic: SetSequence, UniformUInt32, UniformUInt32(b) with its
                    rejection threshold, UniformFloat = min(OneMinusEpsilon, float(u32) * 2^-32): the float32 value itself, no band.
                    Film pixel j of a task (row-major) draws from RNG(rng_seed + j) (include/iile_scene.h: the reference has one
                    stream per thread, consumed in scheduling order)
  film monitors     IisptFilmMonitor::add_n_samples (iisptfilmmonitor.cpp:47-72), merge_into (:231-276) over IisptPixel::normalize
                    (iisptpixel.h:12-20), to_intensity_film (:158-213), in float64

ONE FACT THE SOURCES CANNOT SETTLE. `Point2f uScattering(rng->uniform_float(), rng->uniform_float())` (:95-98) leaves the order of the
two draws to the compiler. The truth evaluates the SECOND argument first (u.y is the first draw, u.x the second): g++'s order on
x86-64, the compiler and target the reference is built with.

What is NOT restated but reused: path_ref's Scene (brute-force hits, the hit's frame), BSDF, materials and Ctx with its recorded
branches; through it trace_ref, microfacet_ref, translucent_ref.

THE HAZARD OF ROW 0 AND COLUMN 0. Texel row y = 0 and column x = 0 of a hemisphere map to theta = 0 or phi = 0, directions with
sin theta sin phi = 0: exactly in the hemi camera's horizon. For a pixel in the plane of its hemi point BSDF::f's reflect test is
then undecided by construction, for a sixteenth of all light samples. Row 0 is black in any case (its jacobian is sin 0); the cases
blacken column 0 as well (an exact decision, and a legitimate network output), except where pixel and hemi-point normals differ.

DISCRETE DECISIONS, beyond path_ref's (hit identity, grazing directions, lobe choice, Fresnel choice, Refract): a pixel is kept only
if all of these are decided; the whole pixel drops otherwise, since every later draw depends on the earlier decisions:
  * rr < weight: the weight's chain is about 40 float32 operations on values <= 2: flagged within WEIGHT_BAND = 64 u
  * the texel indices of getLightSampleNn: v = hemi theta / Pi carries acos's conditioning, 16 u / sin theta on the argument's 16 u
    (a rotated unit vector), v = hemi phi / Pi atan2's 16 u / |(x, z)|, both 4 u hemi of their own: flagged within that of a whole
    number, the outer edge `hemi` included; 0 is no decision for truncation (both sides give 0)
  * the normal's turn against the ray: |Dot(n, d)| >= GRAZE; `dt < 0` of weighting_distance_normals is recorded and replayed but
    carries no band: both sides give 1 at dt = 0 (a floor pixel under a wall's hemi point has dt = 0 exactly), so it decides nothing
  * beta.y() > 0: beta is exactly 0 or a product of Fresnel factors: flagged below 1e-6

FLOAT32 MODE. gather(..., dtype=np.float32) evaluates the same formulas in single precision from the float64 run's recorded decisions,
as path_ref's does; LookAt's numerical inverse is taken as the transpose. Per pixel S = max-channel f_beta times the sum over the terms
added of max-channel |term|, over samples_taken, plus one float32 ulp of the largest texel. Per case B = the worst |L32 - L64| / S over the kept pixels;
the band for the oracle and the device is 4 B S. `python tests/iispt_ref.py` (measure()) printed the MEASURED table below.
"""
import sys
import warnings

import numpy as np

import path_ref as PR
from path_ref import _black, _dot, _cross, _lum, _normalize

U = PR.U
GRAZE = PR.GRAZE
WEIGHT_BAND = 64 * U
HEMI = 32
SAMPLES = 16               # HEMISPHERIC_IMPORTANCE_SAMPLES
M64 = (1 << 64) - 1
PCG32_DEFAULT_STATE, PCG32_MULT = 0x853c49e6748fea9b, 0x5851f42d4c957f2d
ONE_MINUS_EPSILON = PR.ONE_MINUS_EPSILON


# ---- core/rng.h ----------------------------------------------------------------------------------------------------------------
class Pcg32:
    """RNG(sequenceIndex), rng.h:71, 142-148. `initstate` is PCG32_DEFAULT_STATE there; the parameter lets the generator be pinned by
    the published PCG32 demo values (initstate 42, sequence 54)."""

    def __init__(self, seq, initstate=PCG32_DEFAULT_STATE):
        self.state, self.inc = 0, ((int(seq) << 1) | 1) & M64
        self.u32()
        self.state = (self.state + initstate) & M64
        self.u32()

    def u32(self):   # rng.h:150-156
        old = self.state
        self.state = (old * PCG32_MULT + self.inc) & M64
        xs = (((old >> 18) ^ old) >> 27) & 0xffffffff
        rot = old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xffffffff

    def uniform_u32(self, b):   # rng.h:77-83
        threshold = ((1 << 32) - b) % b
        while True:
            r = self.u32()
            if r >= threshold:
                return r % b

    def uniform_float(self):   # rng.h:85-92
        return min(ONE_MINUS_EPSILON, np.float32(np.float32(self.u32()) * np.float32(2.0 ** -32)))


# ---- the task's grid -----------------------------------------------------------------------------------------------------------
class Task:
    def __init__(self, x0, y0, x1, y1, tilesize, counter_base, rng_seed):
        self.x0, self.y0, self.x1, self.y1, self.tilesize, self.counter_base, self.rng_seed = x0, y0, x1, y1, tilesize, counter_base, rng_seed

    def args(self):
        return (self.x0, self.y0, self.x1, self.y1, self.tilesize, self.counter_base, self.rng_seed)

    @staticmethod
    def _axis(a0, a1, ts):   # :381-410
        out, t = [a0], a0
        while t != a1 - 1:
            t = min(t + ts, a1 - 1)
            out.append(t)
        return out

    def hemi_xs(self):
        return self._axis(self.x0, self.x1, self.tilesize)

    def hemi_ys(self):
        return self._axis(self.y0, self.y1, self.tilesize)

    def pixels(self):
        return [(fx, fy) for fy in range(self.y0, self.y1) for fx in range(self.x0, self.x1)]

    def neighbours(self, fx, fy):
        """:434-464: S, E, R, B as film coordinates."""
        ts = self.tilesize
        sx, sy = fx - (fx - self.x0) % ts, fy - (fy - self.y0) % ts
        ex, ey = min(sx + ts, self.x1 - 1), min(sy + ts, self.y1 - 1)
        return [(sx, sy), (ex, ey), (ex, sy), (sx, ey)]


def camera_sample(oracle, host, task, item, fx, fy):
    """(ray origin, direction, path_ref.Sampler at dimension 5) of the task's item-th camera sample, taken for film pixel (fx, fy)."""
    cx = task.counter_base + 1 + item
    idx = oracle.sample_index(host, cx, 0, 0)
    cache = {}

    def value(dim):
        if dim not in cache:
            cache[dim] = oracle.sample_dimension(host, idx, dim, cx, 0)
        return cache[dim]
    pfilm = np.array([[np.float32(fx) + value(0), np.float32(fy) + value(1)]], np.float32)
    o, d = oracle.camera_rays(host, pfilm)
    return o[0], d[0], value


# ---- find_intersection ---------------------------------------------------------------------------------------------------------
def find_intersection(scene, ctx, o, d, value):
    """:657-757 -> (found, hit or None, the ray's direction at the hit, beta, path length to the hit, bounces)."""
    dt = ctx.dt
    sampler = PR.Sampler(value)
    beta = np.ones(3, dt)
    ro, rd, own = o.astype(dt), d.astype(dt), -1
    length = 0.0
    for bounces in range(24):
        h = scene.closest(ctx, ro, rd, own)
        if h is None:
            ctx.stats["exit_none"] += 1
            return False, None, rd, np.zeros(3, dt), length, bounces
        length += float(np.linalg.norm((h.p - ro).astype(np.float64)))
        bsdf = scene.bsdf(h, dt)
        wi, f, pdf, flags = bsdf.sample_f(-rd, sampler.get2d(), ctx, True)
        if ctx.branch(_black(f) or pdf == 0):
            ctx.stats["exit_black"] += 1
            return True, h, rd, np.zeros(3, dt), length, bounces
        if not flags & PR.SPECULAR:
            ctx.stats["exit_vertex"] += 1
            ctx.stats["chain_vertex"] += bounces > 0
            return True, h, rd, beta, length, bounces
        beta = beta * f * abs(_dot(wi, h.ns)) / pdf
        if ctx.branch(_lum(beta) < 0 or np.isnan(_lum(beta))):
            return True, h, rd, np.zeros(3, dt), length, bounces
        ro, rd, own = h.p, wi, h.prim
    ctx.stats["exit_limit"] += 1
    return True, None, rd, np.zeros(3, dt), length, 24


def _has_vertex(ctx, found, beta):
    """:293, :519-528."""
    y = _lum(beta)
    if found and y != 0:
        ctx.flag(y, 1e-6)
    return ctx.branch(found and y > 0)


def _turned_normal(ctx, h, rd):
    """:300-310, :973-983."""
    n = h.n
    c = _dot(n, rd)
    ctx.flag(c, GRAZE)
    return -n if ctx.branch(c > 0) else n


def _new_ctx(dt, log=None):
    ctx = PR.Ctx(dt, log)
    ctx.stats.update(exit_none=0, exit_black=0, exit_vertex=0, exit_limit=0, chain_vertex=0, mis_light=0, mis_bsdf=0, bsdf_outside=0,
                     missing_drew=0, distinct_weights=0, n_estimates=0, multi_lobe=0)
    return ctx


class HemiTruth:
    pass


def hemi_points(scene, oracle, host, task):
    """The task's hemi points in float64: valid (ny, nx), pos, dir (ny, nx, 3), kept, bound (the distance a float32 SpawnRay origin
    may lie from pos: hemi_point_bound)."""
    xs, ys = task.hemi_xs(), task.hemi_ys()
    r = HemiTruth()
    r.valid, r.kept = np.zeros((len(ys), len(xs)), np.uint8), np.ones((len(ys), len(xs)), bool)
    r.pos, r.dir, r.bound = np.zeros((len(ys), len(xs), 3)), np.zeros((len(ys), len(xs), 3)), np.zeros((len(ys), len(xs)))
    r.stats = {}
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j, y in enumerate(ys):
            for i, x in enumerate(xs):
                ctx = _new_ctx(np.float64)
                o, d, value = camera_sample(oracle, host, task, j * len(xs) + i, x, y)
                found, h, rd, beta, length, bounces = find_intersection(scene, ctx, o, d, value)
                if _has_vertex(ctx, found, beta):
                    n = _turned_normal(ctx, h, rd)
                    r.valid[j, i], r.pos[j, i], r.dir[j, i] = 1, h.p, n
                    r.bound[j, i] = hemi_point_bound(scene, h, n, length, bounces)
                r.kept[j, i] = ctx.kept
                for k, v in ctx.stats.items():
                    r.stats[k] = r.stats.get(k, 0) + (v > 0)
    return r


GAMMA7 = 7 * 2.0 ** -24 / (1 - 7 * 2.0 ** -24)   # gamma(7), pbrt.h


def hemi_point_bound(scene, h, n, length, bounces):
    """How far a float32 aux-ray origin may lie from the truth's hit point. The float32 hit point lies within Triangle::Intersect's
    pError = gamma(7) (|b0 p0| + |b1 p1| + |b2 p2|) (triangle.cpp:316-320) of the true hit of ITS ray, component by component;
    OffsetRayOrigin (geometry.h) moves it Dot(|n|, pError) along n and rounds each component away by one ulp. Along a specular chain the
    float32 ray itself differs: each of `bounces` spawned rays starts within such an offset of the truth's and its direction carries
    the BSDF sample's roundings, under 512 u, over at most the path's length."""
    T = np.abs(scene.P[h.prim]).reshape(3, 3)
    err = GAMMA7 * T.sum(0)        # the barycentrics are in [0, 1]: |b_i p_i| <= |p_i|
    one = float(np.abs(n) @ err) + float(np.linalg.norm(err)) + 2 * U * float(np.abs(T).max()) * np.sqrt(3)
    return one * (bounces + 1) + bounces * 512 * U * length


# ---- the hemispheric camera ----------------------------------------------------------------------------------------------------
class HemiCamera:
    def __init__(self, pos, direction, film, dt):
        """pos, direction: the float32 aux ray as the runner hands it over; film (hemi, hemi, 3): the predicted image, row 0 first."""
        self.dt = dt
        self.pos, self.look_dir, self.film = np.asarray(pos, np.float32).astype(dt), np.asarray(direction, np.float32).astype(dt), film
        d = self.look_dir
        up = np.array([0, 1, 0] if (d[0] == 0 and d[1] == 0) else [0, 0, 1], dt)      # hemispheric.cpp:118-120
        look = self.pos + d
        z = _normalize(look - self.pos)                                                 # transform.cpp:212
        right = _normalize(_cross(_normalize(up), z))
        new_up = _cross(z, right)
        self.c2w = np.stack([right, new_up, z], 1)                                      # columns

    def to_world(self, v):
        m = self.c2w
        return np.array([m[0, 0] * v[0] + m[0, 1] * v[1] + m[0, 2] * v[2], m[1, 0] * v[0] + m[1, 1] * v[1] + m[1, 2] * v[2],
                         m[2, 0] * v[0] + m[2, 1] * v[1] + m[2, 2] * v[2]], self.dt)

    def to_camera(self, v):
        m = self.c2w
        return np.array([m[0, 0] * v[0] + m[1, 0] * v[1] + m[2, 0] * v[2], m[0, 1] * v[0] + m[1, 1] * v[1] + m[2, 1] * v[2],
                         m[0, 2] * v[0] + m[1, 2] * v[1] + m[2, 2] * v[2]], self.dt)

    def texel(self, x, y):
        """get_camera_coord_jacobian, intensityfilm.cpp:53-66."""
        dt = self.dt
        pix = self.film[HEMI - 1 - y, x].astype(dt)
        polar = dt(np.pi * float(dt(y) / dt(HEMI)))     # Float abs = y / height; Float polar = M_PI * abs (a double product)
        return pix * np.sin(polar)

    def light_sample_nn(self, x, y):
        """hemispheric.cpp:89-105 -> (Li, wi)."""
        dt = self.dt
        theta, phi = dt(np.pi) * dt(y) / dt(HEMI), dt(np.pi) * dt(x) / dt(HEMI)
        d = np.array([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], dt)
        return self.texel(x, y), self.to_world(d)

    def lookup(self, wi, ctx):
        """getLightSampleNn, hemispheric.cpp:44-60."""
        dt = self.dt
        if ctx.replay:
            x, y = ctx.choice(None)
        else:
            wc = self.to_camera(wi)
            cy = float(np.clip(wc[1], -1, 1))
            theta, phi = np.arccos(cy), np.arctan2(float(wc[2]), float(wc[0]))
            vy, vx = HEMI * theta / np.pi, HEMI * phi / np.pi
            my = HEMI / np.pi * 16 * U / max(np.sqrt(max(1 - cy * cy, 0.0)), 1e-9) + 4 * U * HEMI
            mx = HEMI / np.pi * 16 * U / max(np.hypot(float(wc[2]), float(wc[0])), 1e-9) + 4 * U * HEMI
            for v, m in ((vy, my), (vx, mx)):
                if round(v) != 0:
                    ctx.drop(abs(v - round(v)) <= m)
            x, y = ctx.choice((int(vx), int(vy)))      # int(): towards zero, as the C conversion
        if 0 <= x < HEMI and 0 <= y < HEMI:
            return self.texel(x, y)
        ctx.stats["bsdf_outside"] += 1
        return np.zeros(3, dt)


# ---- compute_fpixel_weights ----------------------------------------------------------------------------------------------------
def fpixel_weights(ctx, task, f_pixel, neigh, cams, aux_d, p, cam_origin):
    """:961-1037 -> the four probabilities, float32 values in float32 mode (the reference's types), float64 otherwise."""
    dt = ctx.dt
    f32 = dt is np.float32
    wod = []
    for (nx, ny), cam in zip(neigh, cams):
        dx, dy = dt(f_pixel[0] - nx), dt(f_pixel[1] - ny)
        pdist = np.sqrt(dx * dx + dy * dy)
        wdpos = min(max(pdist / dt(task.tilesize), dt(0)), dt(1))          # iisptmathutils.h:69-89 (tilesize >= 1)
        if cam is None:
            wdnor = wdd = dt(0)
        else:
            a, b = aux_d / np.sqrt(_dot(aux_d, aux_d)), cam.look_dir / np.sqrt(_dot(cam.look_dir, cam.look_dir))
            c = _dot(a, b)
            wdnor = dt(1) if ctx.branch(c < 0) else dt(1) - c               # :92-113
            to_cam = lambda q: np.sqrt(_dot(q - cam_origin, q - cam_origin))
            d_isect, d_sample = to_cam(p), to_cam(cam.pos)                   # :116-143 (never below 1e-10 here)
            wdd = min(max(dt(1) - abs(d_isect - d_sample) / d_isect, dt(0)), dt(1))
        wod.append(wdpos * wdnor + wdpos * wdd + wdpos)
    w = [max(0.0, 2.0 - float(v)) + 0.001 for v in wod]                     # :1032: double
    if f32:
        w = [np.float32(v) for v in w]
    tot = dt(0)
    for v in w:
        tot = tot + dt(v)
    return [dt(v) / tot for v in w]


def _power_heuristic(f, g):
    return (f * f) / (f * f + g * g)


def _estimate_direct(ctx, h, bsdf, wo, cam, rx, ry, rng, terms):
    """:16-138; `terms` collects max-channel |term| for S."""
    dt = ctx.dt
    light_pdf, bsdf_ratio, em_ratio = dt(np.float32(1.0 / 6.28)), dt(np.float32(0.4394)), dt(np.float32(1.098))
    Ld = np.zeros(3, dt)
    Li, wi = cam.light_sample_nn(rx, ry)
    if ctx.branch(not _black(Li)):
        f = bsdf.f(wo, wi, ctx) * abs(_dot(wi, h.ns))
        spdf = bsdf.pdf(wo, wi, ctx)
        if ctx.branch(not _black(f)):
            term = em_ratio * f * Li * _power_heuristic(light_pdf, spdf) / light_pdf
            ctx.stats["mis_light"] += 1
            terms.append(float(np.abs(term).max()))
            Ld = Ld + term
    first = rng.uniform_float()       # the SECOND argument of uScattering is evaluated first (module docstring)
    second = rng.uniform_float()
    wi, f, spdf, _ = bsdf.sample_f(wo, np.array([second, first], np.float32), ctx, False)
    f = f * abs(_dot(wi, h.ns))
    if ctx.branch(not _black(f) and spdf > 0):
        weight = _power_heuristic(spdf, light_pdf)
        Li = cam.lookup(wi, ctx)
        if ctx.branch(not _black(Li)):
            term = bsdf_ratio * f * Li * weight / spdf
            ctx.stats["mis_bsdf"] += 1
            terms.append(float(np.abs(term).max()))
            Ld = Ld + term
    return Ld


def _sample_hemisphere(ctx, h, bsdf, wo, weights, cams, rng, terms):
    """:142-178 -> (L, samples_taken)."""
    dt = ctx.dt
    L, taken = np.zeros(3, dt), 0
    for w, cam in zip(weights, cams):
        for _ in range(SAMPLES):
            rr = rng.uniform_float()
            ctx.flag(float(rr) - float(w), WEIGHT_BAND)
            if ctx.branch(rr < w):
                taken += 1
                if cam is None:
                    ctx.stats["missing_drew"] += 1
                else:
                    rx, ry = rng.uniform_u32(HEMI), rng.uniform_u32(HEMI)
                    ctx.stats["n_estimates"] += 1
                    L = L + _estimate_direct(ctx, h, bsdf, wo, cam, rx, ry, rng, terms)
    return (L / dt(taken) if taken > 0 else np.zeros(3, dt)), taken


class GatherTruth:
    pass


def gather(scene, oracle, host, task, valid, pos, direction, nn, dtype=np.float64, logs=None):
    """The task's film pixels: out (h, w, 4) {f_beta L, weight}, kept, S, has (a vertex), stats, logs. valid / pos / direction /
    nn: the hemi points as handed to iispt_gather (float32 values: exact inputs)."""
    dt = dtype
    xs, ys = task.hemi_xs(), task.hemi_ys()
    w, hgt = task.x1 - task.x0, task.y1 - task.y0
    r = GatherTruth()
    r.out, r.kept, r.S, r.has = np.zeros((hgt, w, 4), dt), np.ones((hgt, w), bool), np.zeros((hgt, w)), np.zeros((hgt, w), bool)
    r.taken, r.n_est = np.zeros((hgt, w), int), np.zeros((hgt, w), int)
    r.chain = np.zeros((hgt, w), int)        # specular bounces before the pixel's vertex
    r.angle = np.full((hgt, w), np.nan)      # the smallest angle (degrees) between the pixel's turned normal and its hemi points'
    r.stats, r.why, r.logs = {}, {}, []
    nn = np.asarray(nn, np.float32)
    floor = float(np.spacing(np.float32(nn.max()))) if nn.size else 0.0
    cams = {}
    for j, y in enumerate(ys):
        for i, x in enumerate(xs):
            cams[x, y] = HemiCamera(pos[j, i], direction[j, i], nn[j, i], dt) if valid[j, i] else None
    cam_origin = oracle.camera_rays(host, np.zeros((1, 2), np.float32))[0][0].astype(dt)      # camera.cpp:115-124
    n_hemi = len(xs) * len(ys)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j, (fx, fy) in enumerate(task.pixels()):
            ctx = _new_ctx(dt, None if logs is None else logs[j])
            o, d, value = camera_sample(oracle, host, task, n_hemi + j, fx, fy)
            found, h, rd, beta, _, bounces = find_intersection(scene, ctx, o, d, value)
            py, px = fy - task.y0, fx - task.x0
            r.chain[py, px] = bounces
            if _has_vertex(ctx, found, beta):
                r.has[py, px] = True
                neigh = task.neighbours(fx, fy)
                ncams = [cams[q] for q in neigh]
                aux_d = _turned_normal(ctx, h, rd)
                weights = fpixel_weights(ctx, task, (fx, fy), neigh, ncams, aux_d, h.p, cam_origin)
                cosines = [float(_dot(aux_d, c.look_dir)) for c in ncams if c is not None]
                if cosines:
                    r.angle[py, px] = np.degrees(np.arccos(np.clip(max(cosines), -1, 1)))
                if len(set(neigh)) == 4 and len({float(v) for v in weights}) == 4 and all(c is not None for c in ncams):
                    ctx.stats["distinct_weights"] += 1
                bsdf = scene.bsdf(h, dt)      # ComputeScatteringFunctions(f_ray, arena), :547
                ctx.stats["multi_lobe"] += len(bsdf.matching(False)) > 1
                terms = []
                L, taken = _sample_hemisphere(ctx, h, bsdf, -rd, weights, ncams, Pcg32(task.rng_seed + j), terms)
                r.out[py, px, :3], r.out[py, px, 3] = beta * L, 0.5
                r.S[py, px] = float(beta.max()) * sum(terms) / max(taken, 1) + floor
                r.taken[py, px], r.n_est[py, px] = taken, ctx.stats["n_estimates"]
            r.kept[py, px] = ctx.kept
            r.logs.append(ctx.log)
            if not ctx.kept:
                r.why[ctx.why] = r.why.get(ctx.why, 0) + 1
            for k, v in ctx.stats.items():
                r.stats[k] = r.stats.get(k, 0) + (v > 0 if k != "n_estimates" else v)
    return r


def rel_distance(out, truth):
    """max-channel |L - L64| / S per pixel (nan without a vertex)."""
    with np.errstate(invalid="ignore"):   # S is 0 where the runner records nothing
        return np.abs(np.asarray(out, np.float64)[..., :3] - truth.out[..., :3].astype(np.float64)).max(-1) / truth.S


# ---- the film monitors ---------------------------------------------------------------------------------------------------------
def film_add(film, task, out):
    """add_n_samples (iisptfilmmonitor.cpp:47-72) of a task's records into the (H, W, 4) float64 monitor: the float RGB of the
    Spectrum and the double weight are added to double sums. Pixels without a record hold zeros, which add nothing."""
    film[task.y0:task.y1, task.x0:task.x1] += np.asarray(out, np.float32).astype(np.float64).reshape(task.y1 - task.y0, task.x1 - task.x0, 4)
    return film


def film_merge(direct, indirect):
    """merge_into (:231-276) + to_intensity_film (:158-213) in float64: each monitor normalised where its weight is positive
    (iisptpixel.h:12-20), the two added; the merged weight is 1."""
    def norm(m):
        w = m[..., 3:4]
        return np.where(w > 0, m[..., :3] / np.where(w > 0, w, 1), m[..., :3])
    return norm(np.asarray(direct, np.float64)) + norm(np.asarray(indirect, np.float64))


# ---- the probe cameras' first-hit channels -------------------------------------------------------------------------------------
PROBE_MARGIN = 0.25     # pixels: the whole footprint, widened by this much on every side, must see one planar face
PROBE_GRID = 8          # direction samples per pixel and axis


class ProbeTruth:
    pass


def probe_first_hits(scene, pos, direction, hemi):
    """What IISPTdIntegrator::Li leaves in the distance and normal films at depth 0, bounce 0 (integrators/iispt_d.cpp:98-113), per
    probe pixel, without the probe sampler's jitter: pFilm lies somewhere in [x, x + 1] x [y, y + 1], so the distance |isect.p - ray.o|
    lies in [dmin, dmax], the footprint's nearest and farthest distance to the face's plane along HemisphericCamera::GenerateRay's
    directions (hemispheric.cpp:15-29: theta = Pi pFilm.y / h, phi = Pi pFilm.x / w), and the normal is WorldToCamera(isect.n): a
    Normal3f goes through the transpose of the transform's inverse (transform.h:244-249), here the transpose of camera-to-world,
    of the face's own normal (Cross(dp02, dp12), triangle.cpp:344, ReverseOrientation applied; not turned towards the ray).
    -> ok (h, h): the footprint widened by PROBE_MARGIN pixels sees one planar face only; dmin, dmax (h, h); normal (h, h, 3);
    slack (h, h): dmin and dmax are taken over a grid of PROBE_GRID + 1 directions an axis: between grid points the distance is
    monotone unless the cell holds the foot of the perpendicular or an edge's turning point, where it departs from the nearest grid
    value by at most d delta^2 (delta the cell's diagonal, 1.42 Pi / (h PROBE_GRID)); plus the float32 band of the hit point and the
    square root, 64 u of the largest coordinate involved."""
    import trace_ref
    cam = HemiCamera(pos, direction, None, np.float64)
    steps = np.arange(-PROBE_MARGIN, 1 + PROBE_MARGIN + 1e-9, 1.0 / PROBE_GRID)
    inner = (steps > -1e-9) & (steps < 1 + 1e-9)
    S = len(steps)
    f = (np.arange(hemi)[:, None] + steps[None, :]).ravel()          # film coordinate of every sample along one axis
    theta, phi = np.pi * f[:, None] / hemi, np.pi * f[None, :] / hemi
    dc = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta) * np.ones_like(phi), np.sin(theta) * np.sin(phi)], -1)
    dw = (dc.reshape(-1, 3) @ cam.c2w.T)
    o = np.broadcast_to(cam.pos, dw.shape)
    tr = trace_ref.brute_force(scene.P, o, dw, np.full(len(dw), np.inf))
    hit = np.isfinite(tr.t_min)
    prim = np.where(hit, np.argmax(tr.ties, 1), -1)
    # planar faces: triangles with one unit normal and one plane offset
    P = scene.P.reshape(-1, 3, 3)
    n = np.cross(P[:, 0] - P[:, 2], P[:, 1] - P[:, 2])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[scene.flip] *= -1
    keys = {}
    face = np.array([keys.setdefault(tuple(np.round(np.append(n[i], n[i] @ P[i, 0]), 6) + 0.0), len(keys)) for i in range(len(P))])
    fid = np.where(hit, face[np.maximum(prim, 0)], -1).reshape(hemi, S, hemi, S)
    t = tr.t_min.reshape(hemi, S, hemi, S)
    first = fid[:, 0, :, 0]
    r = ProbeTruth()
    r.ok = (first >= 0) & (fid == first[:, None, :, None]).all((1, 3))
    ti = np.where(r.ok[:, None, :, None], t, 0.0)[:, inner][:, :, :, inner]
    r.dmin, r.dmax = ti.min((1, 3)), ti.max((1, 3))
    face_normal = np.zeros((len(keys), 3))
    face_normal[face] = n
    r.normal = np.where(r.ok[..., None], face_normal[np.maximum(first, 0)] @ cam.c2w, 0.0)     # rows: the transpose of camera-to-world
    delta = 1.42 * np.pi / (hemi * PROBE_GRID)
    r.slack = r.dmax * delta * delta + 64 * U * (float(np.abs(scene.P).max()) + float(np.abs(cam.pos).max()))
    return r


def check_probe(tr, normals, distance, who):
    """The first-hit channels of one probe, [y][x] raster order, against its ProbeTruth."""
    ok = tr.ok
    d = np.asarray(distance, np.float64)
    assert (d[ok] >= (tr.dmin - tr.slack)[ok]).all() and (d[ok] <= (tr.dmax + tr.slack)[ok]).all(), (who, "distance outside the footprint's")
    err = np.abs(np.asarray(normals, np.float64) - tr.normal).max(-1)
    assert (err[ok] <= 64 * U).all(), (who, "camera-space normal", float(err[ok].max()))
    return float(ok.mean())


def host_with_probe_film(binding, path, hemi):
    """A HostScene of the file whose probe films are hemi x hemi. The loader always writes 32 x 32 probe films: the descriptor is edited
    in place, as test_probe_film_above_1024_pixels_bitwise does (the Gaussian filter's radius 2 sets the sample bounds)."""
    import ctypes
    host = binding.HostScene(path=path)
    if hemi != HEMI:
        probe = ctypes.cast(host.desc, ctypes.POINTER(binding.SceneDesc)).contents.probe
        assert probe.hemi_size == HEMI and probe.film.samp_x1 == HEMI + 2
        probe.hemi_size = hemi
        probe.film.xres = probe.film.yres = probe.film.crop_x1 = probe.film.crop_y1 = hemi
        probe.film.samp_x1 = probe.film.samp_y1 = hemi + 2
        host.info["probe_hemi_size"] = hemi
    return host


_PROBES = {}


def probe_truths(binding, oracle, tmp_path_factory, name, hemi):
    """(host with hemi x hemi probe films, positions, directions, the ProbeTruth of each of iispt_cases.PROBES[name]), once per session."""
    if (name, hemi) not in _PROBES:
        import iispt_cases
        c = case_truth(binding, oracle, tmp_path_factory, name)
        pos, dr = (np.array(a, np.float32) for a in iispt_cases.PROBES[name])
        _PROBES[name, hemi] = (host_with_probe_film(binding, c.path, hemi), pos, dr, [probe_first_hits(c.scene, p, d, hemi) for p, d in zip(pos, dr)])
    return _PROBES[name, hemi]


# ---- one case, once per session ------------------------------------------------------------------------------------------------
_CACHE = {}


class CaseTruth:
    pass


def case_truth(binding, oracle, tmp_path_factory, name):
    """The truth of one of iispt_cases.CASES: host, scene, per task (Task, binding.IisptTask, HemiTruth, the oracle's hemi points,
    the synthetic hemispheres, GatherTruth)."""
    if name not in _CACHE:
        import iispt_cases
        case = iispt_cases.CASES[name]
        scene, text, _ = case["build"]()
        p = tmp_path_factory.mktemp("iispt_truth") / (name + ".pbrt")
        p.write_text(text)
        c = CaseTruth()
        c.host, c.scene, c.tasks, c.path = binding.HostScene(path=str(p)), scene, [], str(p)
        for k, args in enumerate(case["tasks"]):
            task, btask = Task(*args), binding.IisptTask(*args)
            ht = hemi_points(scene, oracle, c.host, task)
            ov, op, od = oracle.iispt_hemi_points(c.host, btask)
            nn = iispt_cases.hemispheres(case, k, ov.shape)
            gt = gather(scene, oracle, c.host, task, ov, op, od, nn)
            c.tasks.append((task, btask, ht, (ov, op, od), nn, gt))
        _CACHE[name] = c
    return _CACHE[name]


def float32_distance(c, oracle):
    """B of a case: the worst rel_distance of the float32 mode over the kept pixels that have a vertex, over its tasks."""
    B = 0.0
    for task, _, _, (ov, op, od), nn, gt in c.tasks:
        g32 = gather(c.scene, oracle, c.host, task, ov, op, od, nn, np.float32, gt.logs)
        m = gt.kept & gt.has
        if m.any():
            B = max(B, float(rel_distance(g32.out, gt)[m].max()))
    return B


def summary(c):
    """(kept share over the pixels with a vertex, kept pixels, estimates per pixel with a vertex, summed stats) of a case."""
    has = sum(int(t[5].has.sum()) for t in c.tasks)
    kept = sum(int((t[5].has & t[5].kept).sum()) for t in c.tasks)
    est = sum(int(t[5].n_est.sum()) for t in c.tasks)
    stats = {}
    for t in c.tasks:
        for k, v in list(t[5].stats.items()) + [(k, v) for k, v in t[2].stats.items() if k.startswith("exit")]:
            stats[k] = stats.get(k, 0) + int(v)
    return kept / max(has, 1), kept, est / max(has, 1), stats


# what measure() printed: per case (kept share of the pixels with a vertex, kept pixels, B)
MEASURED = {
    "room": (0.9750, 117, 6.772e-07),   # 16.1 estimates per pixel; oracle 0.228 of the band; {'exit_vertex': 132, 'mis_light': 120, 'mis_bsdf': 120, 'bsdf_outside': 50, 'distinct_weights': 55, 'n_estimates': 1930, 'multi_lobe': 12}
    "offset": (0.9412, 112, 2.213e-07),   # 15.7 estimates per pixel; oracle 0.202 of the band; {'exit_black': 3, 'exit_vertex': 129, 'mis_light': 119, 'mis_bsdf': 119, 'bsdf_outside': 33, 'distinct_weights': 80, 'n_estimates': 1871, 'multi_lobe': 44}
    "specular": (0.9646, 109, 1.097e-06),   # 14.1 estimates per pixel; oracle 0.596 of the band; {'tir': 1, 'exit_black': 20, 'exit_vertex': 124, 'chain_vertex': 47, 'mis_light': 112, 'mis_bsdf': 112, 'bsdf_outside': 30, 'missing_drew': 35, 'distinct_weights': 36, 'n_estimates': 1595, 'multi_lobe': 52}
    "missing": (0.9733, 73, 5.052e-07),   # 11.0 estimates per pixel; oracle 0.312 of the band; {'exit_none': 39, 'exit_vertex': 80, 'mis_light': 73, 'mis_bsdf': 75, 'bsdf_outside': 14, 'missing_drew': 40, 'distinct_weights': 9, 'n_estimates': 826, 'multi_lobe': 17}
    "folded": (0.9167, 121, 3.370e-06),   # 15.9 estimates per pixel; oracle 0.238 of the band; {'ns_ng_disagree': 15, 'exit_vertex': 136, 'mis_light': 101, 'mis_bsdf': 104, 'bsdf_outside': 30, 'distinct_weights': 132, 'n_estimates': 2095}
    "up_rule": (0.9612, 99, 4.281e-06),   # 15.9 estimates per pixel; oracle 0.328 of the band; {'exit_black': 7, 'exit_vertex': 112, 'mis_light': 103, 'mis_bsdf': 103, 'distinct_weights': 93, 'n_estimates': 1636, 'multi_lobe': 46}
}


def measure():
    """python tests/iispt_ref.py: per case the kept share, B, estimates per pixel and the branch counts; the oracle's share of the band."""
    import pathlib
    import tempfile
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
    import conftest
    import oracle_binding
    import iispt_cases
    import __graft_entry__ as ge
    ge.build_if_needed()
    binding, oracle = conftest.load_binding(), oracle_binding.Oracle()

    class Factory:
        def mktemp(self, name):
            return pathlib.Path(tempfile.mkdtemp(prefix=name))
    only = sys.argv[1:]
    for name in iispt_cases.CASES:
        if only and name not in only:
            continue
        c = case_truth(binding, oracle, Factory(), name)
        share, kept, est, stats = summary(c)
        B = float32_distance(c, oracle)
        frac = 0.0
        for task, btask, ht, (ov, op, od), nn, gt in c.tasks:
            out = oracle.iispt_gather(c.host, btask, ov, op, od, nn)
            m = gt.kept & gt.has
            if m.any() and B:
                frac = max(frac, float(rel_distance(out, gt)[m].max()) / (4 * B))
        live = {k: v for k, v in stats.items() if v}
        why = {}
        for t in c.tasks:
            for k, v in t[5].why.items():
                why[k] = why.get(k, 0) + v
        print(f'    "{name}": ({share:.4f}, {kept}, {B:.3e}),   # {est:.1f} estimates per pixel; oracle {frac:.3f} of the band; {live}')
        print(f"# {name}: first flags of the dropped pixels, by line of path_ref.py / iispt_ref.py: {why}", file=sys.stderr)


if __name__ == "__main__":
    measure()
