"""How the path integrator chooses a light, restated in float64 from the reference alone: the three LightDistributions
(core/lightdistrib.cpp:47-299: uniform, power, and the spatial one with its voxel grid and ComputeDistribution over the
radical-inverse samples), Distribution1D and SampleDiscrete (core/sampling.h:57-100), and what ComputeDistribution asks of the
lights: Triangle::Sample and Area (shapes/triangle.cpp), Shape::Sample(ref) (core/shape.cpp), DiffuseAreaLight::Sample_Li / L /
Power (lights/diffuse.cpp), PointLight and SpotLight (lights/point.cpp, lights/spot.cpp). Point, spot and triangle area lights.

Every evaluation takes a dtype: float64 is the truth, float32 is the same formulas in single precision (numpy's order of
operations, not the device's) — the tests use it to see that a scene keeps inside the bands before a device is asked.

The bands. A device evaluates all this in float32, u = 2^-24 per rounding; R is the scene's largest coordinate. For light j of a
voxel, contrib_j is a sum of 128 terms t_i = Li.y / pdf >= 0 added in order:
    |float32 contrib_j - contrib_j| <= sum_i |dt_i| + 127 u contrib_j                      (sequential summation)
The sample po is a lerp of lerps of the bounds: 6 roundings at magnitude R, |dpo| <= 6 u R per coordinate. With w = pLight - po and
d = |w|: |dw| <= 6 u R + u |w| per coordinate, so d^2 moves by 2 sqrt(3) 6 u R d + 4 u d^2, i.e. by (21 R / d + 4) u relative, and
the direction w / d by (11 R / d + 6) u. A term is M_i g_i, M_i = Y / d_i^2 (Y = I.y, or L.y x area), g_i in [0, 1]:
  point     g = 1.  Li per channel, one division each, the luminance's 5 roundings:    |dt_i| <= u M_i (12 + 24 R / d_i)
  spot      g = Falloff: 0 below cosTotalWidth, 1 from cosFalloffStart on, delta^4 between, delta = (cos - cosTotalWidth) / W,
            W = cosFalloffStart - cosTotalWidth. cos moves by e_i = (8 + 12 R / d_i) u, delta by e_i / W, and delta^4 by at most
            4 delta^3 times that: a sample whose delta lies further than e_i / W outside [0, 1] has g exact.
                                                |dt_i| <= u M_i [(12 + 24 R / d_i) g_i + 4 delta_i^3 (8 + 12 R / d_i) / W]
            (delta_i, g_i taken e_i / W higher, capped at 1)
  triangle  the sampled point b0 p0 + b1 p1 + b2 p2 is 10 more roundings at magnitude R: |dw| <= 16 u R + u |w|, d^2 moves by
            (56 R / d + 4) u relative, the direction by (28 R / d + 6) u; the unit normal of a triangle whose edges at p0 enclose
            an angle with sine >= 0.3 (many_lights_scenes.py keeps to that) by 27 u. g = |cos| at the light (0 behind a one-sided
            one: continuous), M = L.y area / d^2 with area and 1 / pdf another 8 roundings:
                                                |dt_i| <= u M_i [(12 + 56 R / d_i) + (33 + 28 R / d_i)] = u M_i (45 + 84 R / d_i)
The finish: sum and average over n lights (an n-term running sum, (n + 2) u relative), the floor, then cdf_k = sum_{j<k} f_j / n
as a running sum ((k + 2) u relative on top of the f's own errors), the division by funcInt. finish() carries these through and
returns an absolute band per cdf step and a relative band per light's pdf; 2 u more for u itself being compared in float32.
"""
import numpy as np

U = 2.0 ** -24
N_SAMPLES, MAX_VOXELS = 128, 64
ONE_MINUS_EPSILON = np.float32(1) - np.float32(2.0 ** -24)


def lum(rgb):
    rgb = np.asarray(rgb)
    return 0.212671 * rgb[..., 0] + 0.715160 * rgb[..., 1] + 0.072169 * rgb[..., 2]


class Point:
    def __init__(self, pos, intensity):
        self.pos, self.I = np.array(pos, np.float32).astype(np.float64), np.array(intensity, np.float32).astype(np.float64)

    def power(self):  # point.cpp: 4 Pi I
        return lum(4 * np.pi * self.I)


class Spot:
    """CreateSpotLight: "from", "to", "coneangle", "conedeltaangle"; the cone's axis in world space is Normalize(to - from)."""

    def __init__(self, pos, to, intensity, cone=30.0, delta=5.0):
        self.pos, self.I = np.array(pos, np.float32).astype(np.float64), np.array(intensity, np.float32).astype(np.float64)
        axis = np.array(to, np.float32).astype(np.float64) - self.pos
        self.axis = axis / np.linalg.norm(axis)
        self.cos_total, self.cos_start = np.cos(np.radians(cone)), np.cos(np.radians(cone - delta))

    def power(self):  # spot.cpp: I 2 Pi (1 - .5 (cosFalloffStart + cosTotalWidth))
        return lum(self.I * 2 * np.pi * (1 - .5 * (self.cos_start + self.cos_total)))


class Tri:
    """A DiffuseAreaLight on one triangle declared under the identity transform (no normals: n = Normalize(Cross(p1 - p0, p2 - p0)))."""

    def __init__(self, p0, p1, p2, L, two_sided=False):
        self.p = [np.array(p, np.float32).astype(np.float64) for p in (p0, p1, p2)]
        self.L, self.two_sided = np.array(L, np.float32).astype(np.float64), bool(two_sided)

    def area(self):
        return 0.5 * np.linalg.norm(np.cross(self.p[1] - self.p[0], self.p[2] - self.p[0]))

    def power(self):  # diffuse.cpp: (twoSided ? 2 : 1) Lemit area Pi
        return lum((2 if self.two_sided else 1) * self.L * self.area() * np.pi)


def radical_inverse(base_index, a):
    """RadicalInverse(baseIndex, a) (lowdiscrepancy.cpp) for the first five primes: the float the reference returns."""
    base = (2, 3, 5, 7, 11)[base_index]
    if base == 2:
        return np.float32(int(format(a, "064b")[::-1], 2) * 2.0 ** -64)
    inv_base, inv_base_n, rev = np.float32(1) / np.float32(base), np.float32(1), 0
    while a:
        nxt = a // base
        rev = rev * base + (a - nxt * base)
        inv_base_n = np.float32(inv_base_n * inv_base)
        a = nxt
    return min(np.float32(np.float32(rev) * inv_base_n), ONE_MINUS_EPSILON)


SAMPLES = np.array([[radical_inverse(b, i) for b in range(5)] for i in range(N_SAMPLES)], np.float64)  # float32 values, held exactly


def finish(func, err, dtype=np.float64):
    """Distribution1D(func) (sampling.h:57-69) -> (cdf[n + 1], funcInt, cdf_band[n + 1], pdf_band[n]): err is the absolute band
    of each func entry as a float32 evaluation has it; cdf_band is absolute, pdf_band relative to SampleDiscrete's pdf."""
    func = np.asarray(func, dtype)
    n = len(func)
    cdf = np.zeros(n + 1, dtype)
    for i in range(1, n + 1):
        cdf[i] = cdf[i - 1] + func[i - 1] / dtype(n)
    func_int = cdf[n]
    f64, e64 = np.asarray(func, np.float64), np.asarray(err, np.float64)
    raw = np.concatenate([[0.0], np.cumsum(f64 / n)])
    raw_band = np.concatenate([[0.0], np.cumsum(e64 / n)]) + (np.arange(n + 1) + 2) * U * raw
    if func_int == 0:
        return np.arange(n + 1, dtype=dtype) / dtype(n), func_int, np.full(n + 1, 2 * U), np.zeros(n)
    total = raw[n]
    cdf_band = (raw_band + raw / total * raw_band[n]) / total + 2 * U
    pdf_band = e64 / np.maximum(f64, 1e-300) + raw_band[n] / total + 4 * U
    return cdf / func_int, func_int, cdf_band, pdf_band


def sample_discrete(cdf, func, func_int, u):
    """Distribution1D::SampleDiscrete (sampling.h:90-100) over FindInterval (pbrt.h:399-412) -> (offsets, pdf of each)."""
    n = len(func)
    off = np.clip(np.searchsorted(cdf, u, side="right") - 1, 0, n - 1)
    pdf = func[off] / (func_int * n) if func_int > 0 else np.zeros(len(off))
    return off, pdf


class Scene:
    """lights in the order the scene declares them; bounds = (pMin, pMax) of scene.WorldBound(), as float32 values."""

    def __init__(self, lights, bmin, bmax):
        self.lights = list(lights)
        self.bmin, self.bmax = np.array(bmin, np.float32).astype(np.float64), np.array(bmax, np.float32).astype(np.float64)
        diag = self.bmax - self.bmin
        # Bounds3::MaximumExtent (geometry.h): x if it is the largest, else y if larger than z, else z
        me = 0 if (diag[0] > diag[1] and diag[0] > diag[2]) else (1 if diag[1] > diag[2] else 2)
        self.nv = np.maximum(1, np.round(diag / diag[me] * MAX_VOXELS).astype(int))  # lightdistrib.cpp:98-111
        self.R = float(np.abs(np.concatenate([self.bmin, self.bmax])).max())
        self._cache = {}

    # ---- SpatialLightDistribution::Lookup's voxel (lightdistrib.cpp:134-150) ----
    def voxel_of(self, p):
        o = np.asarray(p, np.float64) - self.bmin
        ext = self.bmax - self.bmin
        o = np.where(ext > 0, o / np.where(ext > 0, ext, 1), o)
        pi = np.trunc(o * self.nv).astype(int)  # int(): towards zero
        return np.clip(pi, 0, self.nv - 1)

    def voxel_bounds(self, pi, dtype=np.float64):
        pi = np.asarray(pi)
        nv, lo, hi = self.nv.astype(dtype), self.bmin.astype(dtype), self.bmax.astype(dtype)
        p0, p1 = pi.astype(dtype) / nv, (pi + 1).astype(dtype) / nv
        return (1 - p0) * lo + p0 * hi, (1 - p1) * lo + p1 * hi  # Bounds3::Lerp over pbrt::Lerp

    # ---- ComputeDistribution ----
    def contributions(self, pi, dtype=np.float64):
        """-> (contrib[n], band[n]): the 128-sample sums of Li.y / pdf for voxel pi, and their absolute float32 bands."""
        vmin, vmax = self.voxel_bounds(pi, dtype)
        t = SAMPLES.astype(dtype)
        po = (1 - t[:, :3]) * vmin + t[:, :3] * vmax  # (128, 3)
        u0, u1 = t[:, 3], t[:, 4]
        contrib, band = np.zeros(len(self.lights)), np.zeros(len(self.lights))
        for j, lt in enumerate(self.lights):
            if isinstance(lt, Tri):
                p0, p1, p2 = [p.astype(dtype) for p in lt.p]
                su0 = np.sqrt(u0)  # UniformSampleTriangle, sampling.cpp
                b0, b1 = 1 - su0, u1 * su0
                ps = b0[:, None] * p0 + b1[:, None] * p1 + (1 - b0 - b1)[:, None] * p2
                cr = np.cross(p1 - p0, p2 - p0)
                nrm = cr / np.sqrt((cr * cr).sum())
                area = dtype(0.5) * np.sqrt((cr * cr).sum())
                w = ps - po
                d2 = (w * w).sum(axis=1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    wi = w / np.sqrt(d2)[:, None]
                    cos_l = -(nrm * wi).sum(axis=1)  # Dot(n, -wi)
                    pdf = (1 / area) * d2 / np.abs(cos_l)  # Shape::Sample(ref): area measure to solid angle
                    pdf = np.where((d2 == 0) | ~np.isfinite(pdf), 0, pdf)
                    emits = lt.two_sided | (cos_l > 0)  # DiffuseAreaLight::L
                    term = np.where((pdf > 0) & emits, dtype(lum(lt.L)) / pdf, 0)
                d = np.sqrt(d2.astype(np.float64))
                err = lum(lt.L) * float(area) / d ** 2 * (45 + 84 * self.R / d)
            else:
                w = lt.pos.astype(dtype) - po
                d2 = (w * w).sum(axis=1)
                d = np.sqrt(d2.astype(np.float64))
                mag = lum(lt.I) / d ** 2
                g = np.ones(N_SAMPLES, dtype)
                err = mag * (12 + 24 * self.R / d)
                if isinstance(lt, Spot):  # SpotLight::Falloff(-wi), spot.cpp:66-76
                    width = lt.cos_start - lt.cos_total
                    cos_t = -(w / np.sqrt(d2)[:, None] * lt.axis.astype(dtype)).sum(axis=1)
                    delta = (cos_t - dtype(lt.cos_total)) / dtype(width)
                    g = np.where(cos_t < lt.cos_total, 0, np.where(cos_t >= lt.cos_start, 1, (delta * delta) * (delta * delta)))
                    e_cos = 8 + 12 * self.R / d  # in units of u
                    margin = U * e_cos / width
                    d64 = delta.astype(np.float64)
                    hi = np.where((d64 < -margin) | (d64 > 1 + margin), np.where(d64 < 0, 0.0, 1.0), np.clip(d64 + margin, 0, 1))
                    slope = np.where((d64 < -margin) | (d64 > 1 + margin), 0.0, 4 * hi ** 3 / width)
                    err = mag * ((12 + 24 * self.R / d) * hi ** 4 + slope * e_cos)
                term = dtype(lum(lt.I)) * g / d2
            acc = dtype(0)
            for x in term.astype(dtype):
                acc = dtype(acc + x)
            contrib[j] = acc
            band[j] = U * err.sum() + (N_SAMPLES - 1) * U * float(acc)
        return contrib, band

    def spatial(self, pi, dtype=np.float64):
        key = (tuple(int(x) for x in pi), np.dtype(dtype).name)
        if key not in self._cache:
            contrib, band = self.contributions(np.array(pi), dtype)
            n = len(contrib)
            c = contrib.astype(dtype)
            total = dtype(0)
            for x in c:
                total = dtype(total + x)
            avg = dtype(total / dtype(N_SAMPLES * n))
            floor = dtype(.001 * np.float64(avg)) if avg > 0 else dtype(1)
            floor_band = .001 * (band.sum() + (n + 2) * U * contrib.sum()) / (N_SAMPLES * n) if avg > 0 else 0.0
            func = np.maximum(c, floor)
            err = np.maximum(band, floor_band)  # max(a, b) moves by no more than the larger of the two bands
            self._cache[key] = (func,) + finish(func, err, dtype)
        return self._cache[key]

    def fixed(self, strategy, dtype=np.float64):
        """UniformLightDistribution / PowerLightDistribution: one Distribution1D for every point."""
        if strategy == "uniform":
            func, err = np.ones(len(self.lights)), np.zeros(len(self.lights))
        else:
            func = np.array([lt.power() for lt in self.lights])
            err = 16 * U * func  # Power().y() itself is a float32 product of a few factors
        func = func.astype(dtype)
        return (func,) + finish(func, err, dtype)

    def choose(self, strategy, p, u, dtype=np.float64):
        """For every point p[i] and sample u[i]: (light chosen, pdf of each light there [m, n], undecided[m]: u[i] lies within the
        band of a cdf step between two lights, pdf_band[m, n] relative)."""
        p, u = np.asarray(p, np.float64), np.asarray(u, np.float64)
        m, n = len(u), len(self.lights)
        light, pdfs, undecided, bands = np.zeros(m, int), np.zeros((m, n)), np.zeros(m, bool), np.zeros((m, n))
        if strategy == "spatial":
            vox = self.voxel_of(p)
            groups = {}
            for i, v in enumerate(map(tuple, vox)):
                groups.setdefault(v, []).append(i)
            dists = [(np.array(ix), self.spatial(v, dtype)) for v, ix in groups.items()]
        else:
            dists = [(np.arange(m), self.fixed(strategy, dtype))]
        for ix, (func, cdf, func_int, cdf_band, pdf_band) in dists:
            light[ix], _ = sample_discrete(cdf, func, func_int, u[ix])
            pdfs[ix] = (func / (func_int * n)) if func_int > 0 else 0
            bands[ix] = pdf_band
            inner = np.arange(1, n)  # the steps between two lights (cdf[0] = 0 and cdf[n] = 1 decide nothing: FindInterval clamps)
            undecided[ix] = (np.abs(u[ix][:, None] - np.asarray(cdf, np.float64)[inner][None, :]) <= cdf_band[inner][None, :]).any(axis=1)
        return light, pdfs, undecided, bands


def rect_irradiance(corners, p, n):
    """Irradiance at point p (unit normal n) from a Lambertian polygon of unit radiance with the given corners, in order, all on
    the positive side of the surface at p: Lambert's formula, E = 1/2 sum_k angle(v_k, v_k+1) (v_k x v_k+1)/|..| . n."""
    v = np.asarray(corners, np.float64) - np.asarray(p, np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    e = 0.0
    for k in range(len(v)):
        a, b = v[k], v[(k + 1) % len(v)]
        c = np.cross(a, b)
        e += np.arccos(np.clip(np.dot(a, b), -1, 1)) * np.dot(c / np.linalg.norm(c), n)
    return abs(e) / 2
