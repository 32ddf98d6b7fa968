"""The BSDF math of pbrt-v3's metal and substrate materials restated in float64 numpy, for test_gpu_metal_substrate.py: FrConductor
(core/reflection.cpp:71-94), FresnelBlend's SchlickFresnel (reflection.h:485-488), TrowbridgeReitzDistribution's D, Lambda, G1, G,
Pdf and Sample_wh (core/microfacet.cpp:155-336, visible-area sampling), MicrofacetReflection::f / Sample_f / Pdf
(reflection.cpp:226-236, 405-423) and FresnelBlend::f / Sample_f / Pdf (reflection.cpp:285-298, 450-475). The oracle has neither
material, so this is the independent statement the device is held to. Directions are (n, 3) arrays in the shading frame (z up)."""
import numpy as np

ONE_MINUS_EPSILON = float.fromhex("0x1.fffffep-1")


def roughness_to_alpha(r):
    """TrowbridgeReitzDistribution::RoughnessToAlpha, microfacet.h:123-128."""
    x = np.log(max(r, 1e-3))
    return 1.62142 + 0.819955 * x + 0.1734 * x ** 2 + 0.0171201 * x ** 3 + 0.000640711 * x ** 4


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def fr_conductor(cos_i, eta, k):
    """FrConductor(cos, 1, eta, k) per RGB channel: (n,) cosines, (3,) eta and k -> (n, 3)."""
    c = np.clip(np.asarray(cos_i, np.float64), -1, 1)[:, None]
    eta, k = np.asarray(eta, np.float64)[None, :], np.asarray(k, np.float64)[None, :]
    c2 = c * c
    s2 = 1 - c2
    eta2, etak2 = eta * eta, k * k
    t0 = eta2 - etak2 - s2
    a2plusb2 = np.sqrt(t0 * t0 + 4 * eta2 * etak2)
    t1 = a2plusb2 + c2
    a = np.sqrt(0.5 * (a2plusb2 + t0))
    t2 = 2 * c * a
    rs = (t1 - t2) / (t1 + t2)
    t3 = c2 * a2plusb2 + s2 * s2
    t4 = t2 * s2
    rp = rs * (t3 - t4) / (t3 + t4)
    return 0.5 * (rp + rs)


def schlick(cos, rs):
    """FresnelBlend::SchlickFresnel: (n,) cosines, (3,) Rs -> (n, 3)."""
    rs = np.asarray(rs, np.float64)[None, :]
    return rs + ((1 - np.asarray(cos))[:, None] ** 5) * (1 - rs)


# ---- TrowbridgeReitzDistribution ----------------------------------------------------------------------------------------------
def _trig(w):
    cos2 = w[:, 2] ** 2
    sin2 = np.maximum(0, 1 - cos2)
    sin = np.sqrt(sin2)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos_phi = np.where(sin == 0, 1.0, np.clip(w[:, 0] / np.where(sin == 0, 1, sin), -1, 1))
        sin_phi = np.where(sin == 0, 0.0, np.clip(w[:, 1] / np.where(sin == 0, 1, sin), -1, 1))
    return cos2, sin2, cos_phi, sin_phi


def tr_d(wh, ax, ay):
    cos2, sin2, cp, sp = _trig(wh)
    with np.errstate(divide="ignore", invalid="ignore"):
        tan2 = sin2 / cos2
        e = (cp ** 2 / ax ** 2 + sp ** 2 / ay ** 2) * tan2
        d = 1 / (np.pi * ax * ay * cos2 * cos2 * (1 + e) ** 2)
    return np.where(np.isinf(tan2), 0.0, d)


def tr_lambda(w, ax, ay):
    cos2, sin2, cp, sp = _trig(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        abs_tan = np.abs(np.sqrt(sin2) / w[:, 2])
        alpha = np.sqrt(cp ** 2 * ax ** 2 + sp ** 2 * ay ** 2)
        lam = (-1 + np.sqrt(1 + (alpha * abs_tan) ** 2)) / 2
    return np.where(np.isinf(abs_tan), 0.0, lam)


def tr_g1(w, ax, ay):
    return 1 / (1 + tr_lambda(w, ax, ay))


def tr_g(wo, wi, ax, ay):
    return 1 / (1 + tr_lambda(wo, ax, ay) + tr_lambda(wi, ax, ay))


def tr_pdf(wo, wh, ax, ay):
    """MicrofacetDistribution::Pdf with sampleVisibleArea (microfacet.cpp:338-344)."""
    return tr_d(wh, ax, ay) * tr_g1(wo, ax, ay) * np.abs(_dot(wo, wh)) / np.abs(wo[:, 2])


def _sample11(cos_theta, u1, u2, dtype=np.float64):
    """TrowbridgeReitzSample11, microfacet.cpp:238-283; every operation in `dtype`."""
    n = len(cos_theta)
    sx, sy = np.empty(n, dtype), np.empty(n, dtype)
    normal = cos_theta > .9999
    r = np.sqrt(u1[normal] / (1 - u1[normal]))
    phi = 6.28318530718 * u2[normal]
    sx[normal], sy[normal] = r * np.cos(phi), r * np.sin(phi)
    o = ~normal
    c, U1, U2 = cos_theta[o], u1[o], u2[o]
    sin_t = np.sqrt(np.maximum(0, 1 - c * c))
    tan_t = sin_t / c
    a = 1 / tan_t
    G1 = 2 / (1 + np.sqrt(1 + 1 / (a * a)))
    A = 2 * U1 / G1 - 1
    tmp = np.minimum(1 / (A * A - 1), 1e10)
    B = tan_t
    D = np.sqrt(np.maximum(B * B * tmp * tmp - (A * A - B * B) * tmp, 0))
    s1, s2 = B * tmp - D, B * tmp + D
    x = np.where((A < 0) | (s2 > 1 / tan_t), s1, s2)
    S = np.where(U2 > 0.5, 1.0, -1.0).astype(dtype)
    U2 = np.where(U2 > 0.5, 2 * (U2 - .5), 2 * (.5 - U2))
    z = (U2 * (U2 * (U2 * 0.27385 - 0.73369) + 0.46341)) / (U2 * (U2 * (U2 * 0.093073 + 0.309420) - 1.000000) + 0.597999)
    sx[o], sy[o] = x, S * z * np.sqrt(1 + x * x)
    return sx, sy


def tr_sample_wh(wo, u0, u1, ax, ay, dtype=np.float64):
    """TrowbridgeReitzDistribution::Sample_wh, visible area (microfacet.cpp:285-336); dtype: float64, or the arithmetic of a wo, ax,
    ay given in another."""
    flip = wo[:, 2] < 0
    wi = np.where(flip[:, None], -wo, wo)
    ws = _normalize(np.stack([ax * wi[:, 0], ay * wi[:, 1], wi[:, 2]], 1))
    sx, sy = _sample11(ws[:, 2], np.asarray(u0, dtype), np.asarray(u1, dtype), dtype)
    _, _, cp, sp = _trig(ws)
    sx, sy = cp * sx - sp * sy, sp * sx + cp * sy
    wh = _normalize(np.stack([-ax * sx, -ay * sy, np.ones_like(sx)], 1))
    return np.where(flip[:, None], -wh, wh)


def _reflect(wo, n):
    return -wo + 2 * _dot(wo, n)[:, None] * n


def cosine_sample_hemisphere(u0, u1):
    """ConcentricSampleDisk + CosineSampleHemisphere, sampling.cpp:82-96, sampling.h:154-158."""
    ox, oy = 2 * np.asarray(u0, np.float64) - 1, 2 * np.asarray(u1, np.float64) - 1
    zero = (ox == 0) & (oy == 0)
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, ox, oy)
        theta = np.where(first, np.pi / 4 * (oy / ox), np.pi / 2 - np.pi / 4 * (ox / oy))
    x, y = np.where(zero, 0, r * np.cos(theta)), np.where(zero, 0, r * np.sin(theta))
    return np.stack([x, y, np.sqrt(np.maximum(0, 1 - x * x - y * y))], 1)


# ---- the two materials' BSDFs (one lobe each; BSDF::f / Pdf / Sample_f with ng = ns = +z) -------------------------------------
class Metal:
    """MetalMaterial: MicrofacetReflection(1, TR(ax, ay), FresnelConductor(1, eta, k))."""

    def __init__(self, eta, k, ax, ay):
        self.eta, self.k, self.ax, self.ay = np.asarray(eta, np.float64), np.asarray(k, np.float64), ax, ay

    def f(self, wo, wi):
        cos_o, cos_i = np.abs(wo[:, 2]), np.abs(wi[:, 2])
        wh = wi + wo
        ok = (cos_i != 0) & (cos_o != 0) & np.any(wh != 0, axis=1) & (wo[:, 2] * wi[:, 2] > 0) & (wo[:, 2] != 0)
        wh = _normalize(np.where(ok[:, None], wh, [[0, 0, 1]]))
        F = fr_conductor(np.abs(_dot(wi, wh)), self.eta, self.k)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = (tr_d(wh, self.ax, self.ay) * tr_g(wo, wi, self.ax, self.ay) / (4 * cos_i * cos_o))[:, None] * F
        return np.where(ok[:, None], v, 0.0)

    def pdf(self, wo, wi):
        same = (wo[:, 2] * wi[:, 2] > 0)
        wh = _normalize(np.where(same[:, None], wo + wi, [[0, 0, 1]]))
        return np.where(same, tr_pdf(wo, wh, self.ax, self.ay) / (4 * _dot(wo, wh)), 0.0)

    def sample(self, wo, u0, u1):
        """(wi, f, pdf); pdf 0 where the reflected direction leaves the hemisphere."""
        wh = tr_sample_wh(wo, u0, u1, self.ax, self.ay)
        wi = _reflect(wo, wh)
        same = wo[:, 2] * wi[:, 2] > 0
        pdf = np.where(same, tr_pdf(wo, wh, self.ax, self.ay) / (4 * _dot(wo, wh)), 0.0)
        return wi, np.where(same[:, None], self.f(wo, wi), 0.0), pdf


class Substrate:
    """SubstrateMaterial: FresnelBlend(Rd = Kd, Rs = Ks, TR(ax, ay))."""

    def __init__(self, kd, ks, ax, ay):
        self.kd, self.ks, self.ax, self.ay = np.asarray(kd, np.float64), np.asarray(ks, np.float64), ax, ay

    def f(self, wo, wi):
        p5 = lambda v: v ** 5
        diffuse = (28 / (23 * np.pi)) * self.kd[None, :] * (1 - self.ks[None, :]) * \
            ((1 - p5(1 - .5 * np.abs(wi[:, 2]))) * (1 - p5(1 - .5 * np.abs(wo[:, 2]))))[:, None]
        wh = wi + wo
        ok = np.any(wh != 0, axis=1) & (wo[:, 2] * wi[:, 2] > 0) & (wo[:, 2] != 0)
        wh = _normalize(np.where(ok[:, None], wh, [[0, 0, 1]]))
        spec = tr_d(wh, self.ax, self.ay) / (4 * np.abs(_dot(wi, wh)) * np.maximum(np.abs(wi[:, 2]), np.abs(wo[:, 2])))
        return np.where(ok[:, None], diffuse + spec[:, None] * schlick(_dot(wi, wh), self.ks), 0.0)

    def pdf(self, wo, wi):
        same = wo[:, 2] * wi[:, 2] > 0
        wh = _normalize(np.where(same[:, None], wo + wi, [[0, 0, 1]]))
        return np.where(same, .5 * (np.abs(wi[:, 2]) / np.pi + tr_pdf(wo, wh, self.ax, self.ay) / (4 * _dot(wo, wh))), 0.0)

    def sample(self, wo, u0, u1):
        u0 = np.asarray(u0, np.float64)
        diffuse = u0 < .5
        ua = np.where(diffuse, np.minimum(2 * u0, ONE_MINUS_EPSILON), np.minimum(2 * (u0 - .5), ONE_MINUS_EPSILON))
        wi_d = cosine_sample_hemisphere(ua, u1)
        wi_d[:, 2] *= np.where(wo[:, 2] < 0, -1, 1)
        wi_s = _reflect(wo, tr_sample_wh(wo, ua, u1, self.ax, self.ay))
        wi = np.where(diffuse[:, None], wi_d, wi_s)
        same = wo[:, 2] * wi[:, 2] > 0
        return wi, np.where(same[:, None], self.f(wo, wi), 0.0), np.where(same, self.pdf(wo, wi), 0.0)


def directional_albedo(bsdf, wo, n=2_000_000, seed=1):
    """rho(wo) = integral of f(wo, wi) |cos wi| over the sphere, by importance sampling the restated BSDF: (mean (3,), std err (3,))."""
    rng = np.random.default_rng(seed)
    wo = np.repeat(np.asarray(wo, np.float64)[None, :], n, 0)
    wi, f, pdf = bsdf.sample(wo, rng.random(n), rng.random(n))
    ok = pdf > 0
    v = np.where(ok[:, None], f * np.abs(wi[:, 2])[:, None] / np.where(ok, pdf, 1)[:, None], 0.0)
    return v.mean(0), v.std(0) / np.sqrt(n)
