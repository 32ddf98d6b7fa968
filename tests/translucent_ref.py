"""pbrt-v3's translucent material restated in float64 numpy, for test_gpu_translucent.py: TranslucentMaterial's BSDF
(materials/translucent.cpp:45-80) of LambertianReflection (core/reflection.cpp:178-180), LambertianTransmission (reflection.cpp:187-190,
391-403), MicrofacetReflection with FresnelDielectric(1, 1.5) (reflection.cpp:226-236, 405-423) and MicrofacetTransmission(1, 1.5) in
Radiance mode (reflection.cpp:244-266, 425-447), combined by BSDF::f / Pdf / Sample_f (reflection.cpp:686-801): the lobe picked by
u0, u0 remapped, the other lobes' pdfs summed and f re-evaluated with reflection or transmission decided by the geometric normal.
Directions are (n, 3) arrays in the shading frame (z up); ng is a unit vector of that frame (+z unless given)."""
import numpy as np

from microfacet_ref import ONE_MINUS_EPSILON, _dot, _normalize, cosine_sample_hemisphere, tr_d, tr_g, tr_pdf, tr_sample_wh

ETA = 1.5
LOBES = ("lam_r", "lam_t", "micro_r", "micro_t")  # BxDF order (translucent.cpp:62-78)


def fr_dielectric(cos_i, eta_i, eta_t, dtype=np.float64):
    """FrDielectric, reflection.cpp:47-68, elementwise over (n,) cosines; dtype: float64, or the arithmetic of etas given in another."""
    c = np.clip(np.asarray(cos_i, dtype), -1, 1)
    entering = c > 0
    ei, et = np.where(entering, eta_i, eta_t), np.where(entering, eta_t, eta_i)
    c = np.abs(c)
    sin_i = np.sqrt(np.maximum(0, 1 - c * c))
    sin_t = ei / et * sin_i
    cos_t = np.sqrt(np.maximum(0, 1 - sin_t * sin_t))
    with np.errstate(divide="ignore", invalid="ignore"):
        r_parl = (et * c - ei * cos_t) / (et * c + ei * cos_t)
        r_perp = (ei * c - et * cos_t) / (ei * c + et * cos_t)
        r = (r_parl ** 2 + r_perp ** 2) / 2
    return np.where(sin_t >= 1, 1.0, r)


def _same(wo, wi):
    return wo[:, 2] * wi[:, 2] > 0


class Translucent:
    """TranslucentMaterial with constant Kd, Ks, reflect, transmit and alpha = RoughnessToAlpha(roughness) (or roughness)."""

    def __init__(self, kd, ks, reflect, transmit, alpha):
        c = lambda v: np.maximum(np.asarray(v, np.float64), 0)  # Spectrum::Clamp()
        kd, ks, r, t = c(kd), c(ks), c(reflect), c(transmit)
        self.alpha = alpha
        self.coef = {"lam_r": r * kd, "lam_t": t * kd, "micro_r": r * ks, "micro_t": t * ks}
        on = {"lam_r": r.any() and kd.any(), "lam_t": t.any() and kd.any(), "micro_r": r.any() and ks.any(), "micro_t": t.any() and ks.any()}
        self.lobes = [k for k in LOBES if on[k]]

    # ---- the four lobes' f and Pdf ----
    def _f(self, lobe, wo, wi):
        n = len(wo)
        k = self.coef[lobe][None, :]
        if lobe in ("lam_r", "lam_t"):
            return np.repeat(k / np.pi, n, 0)
        a = self.alpha
        cos_o, cos_i = wo[:, 2], wi[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            if lobe == "micro_r":
                wh = wi + wo
                ok = (cos_i != 0) & (cos_o != 0) & np.any(wh != 0, axis=1)
                wh = _normalize(np.where(ok[:, None], wh, [[0, 0, 1]]))
                F = fr_dielectric(_dot(wi, wh), 1.0, ETA)
                v = tr_d(wh, a, a) * tr_g(wo, wi, a, a) * F / (4 * np.abs(cos_i) * np.abs(cos_o))
                return np.where(ok[:, None], v[:, None] * k, 0.0)
            ok = ~_same(wo, wi) & (cos_i != 0) & (cos_o != 0)
            eta = np.where(cos_o > 0, ETA, 1 / ETA)
            wh = _normalize(np.where(ok[:, None], wo + wi * eta[:, None], [[0, 0, 1]]))
            wh = np.where((wh[:, 2] < 0)[:, None], -wh, wh)
            F = fr_dielectric(_dot(wo, wh), 1.0, ETA)
            sd = _dot(wo, wh) + eta * _dot(wi, wh)
            factor = 1 / eta
            v = (1 - F) * np.abs(tr_d(wh, a, a) * tr_g(wo, wi, a, a) * eta * eta * np.abs(_dot(wi, wh)) * np.abs(_dot(wo, wh)) *
                                 factor * factor / (cos_i * cos_o * sd * sd))
            return np.where(ok[:, None], v[:, None] * k, 0.0)

    def _pdf(self, lobe, wo, wi):
        same = _same(wo, wi)
        if lobe == "lam_r":
            return np.where(same, np.abs(wi[:, 2]) / np.pi, 0.0)
        if lobe == "lam_t":
            return np.where(~same, np.abs(wi[:, 2]) / np.pi, 0.0)
        a = self.alpha
        with np.errstate(divide="ignore", invalid="ignore"):
            if lobe == "micro_r":
                wh = _normalize(np.where(same[:, None], wo + wi, [[0, 0, 1]]))
                return np.where(same, tr_pdf(wo, wh, a, a) / (4 * _dot(wo, wh)), 0.0)
            eta = np.where(wo[:, 2] > 0, ETA, 1 / ETA)
            wh = _normalize(np.where(~same[:, None], wo + wi * eta[:, None], [[0, 0, 1]]))
            sd = _dot(wo, wh) + eta * _dot(wi, wh)
            return np.where(~same, tr_pdf(wo, wh, a, a) * np.abs(eta * eta * _dot(wi, wh) / (sd * sd)), 0.0)

    def _density(self, lobe, wo, wi):
        """The density Sample_f draws the lobe's directions with. It is the lobe's Pdf except for MicrofacetTransmission, whose Pdf
        (reflection.cpp:435-447) also covers directions behind the microfacet, which a refraction at a sampled microfacet never
        yields: there the density is 0."""
        p = self._pdf(lobe, wo, wi)
        if lobe != "micro_t":
            return p
        # the microfacet a refraction of wo into wi needs, (wo + eta wi) / (1 - eta) up to length, which Sample_wh draws only facing
        # wo and on wo's side of the surface
        eta = np.where(wo[:, 2] > 0, ETA, 1 / ETA)
        wh = (wo + wi * eta[:, None]) / (1 - eta)[:, None]
        return np.where((_dot(wo, wh) > 0) & (wh[:, 2] * wo[:, 2] > 0), p, 0.0)

    def sampling_density(self, wo, wi):
        """What BSDF::Sample_f's directions are distributed with: the lobes' densities, each picked with probability 1 / m."""
        if not self.lobes:
            return np.zeros(len(wo))
        return sum(self._density(lobe, wo, wi) for lobe in self.lobes) / len(self.lobes)

    # ---- BSDF::f / Pdf / Sample_f ----
    def f(self, wo, wi, ng=(0, 0, 1)):
        ng = np.asarray(ng, np.float64)
        reflect = (wi @ ng) * (wo @ ng) > 0
        out = np.zeros((len(wo), 3))
        for lobe in self.lobes:
            want = reflect if lobe in ("lam_r", "micro_r") else ~reflect
            out += np.where(want[:, None], self._f(lobe, wo, wi), 0.0)
        return np.where((wo[:, 2] != 0)[:, None], out, 0.0)

    def pdf(self, wo, wi):
        if not self.lobes:
            return np.zeros(len(wo))
        p = sum(self._pdf(lobe, wo, wi) for lobe in self.lobes) / len(self.lobes)
        return np.where(wo[:, 2] != 0, p, 0.0)

    def sample(self, wo, u0, u1, ng=(0, 0, 1)):
        """(wi, f, pdf) as BSDF::Sample_f(BSDF_ALL) returns them; pdf 0 (and f 0) where the picked lobe gives no direction."""
        n, m = len(wo), len(self.lobes)
        wi, f, pdf = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
        if m == 0:
            return wi, f, pdf
        u0, u1 = np.asarray(u0, np.float64), np.asarray(u1, np.float64)
        comp = np.minimum(np.floor(u0 * m).astype(int), m - 1)
        ur0 = np.minimum(u0 * m - comp, ONE_MINUS_EPSILON)
        a = self.alpha
        for c, lobe in enumerate(self.lobes):
            s = comp == c
            if not s.any():
                continue
            w, v0, v1 = wo[s], ur0[s], u1[s]
            if lobe in ("lam_r", "lam_t"):
                d = cosine_sample_hemisphere(v0, v1)
                flip = (w[:, 2] < 0) if lobe == "lam_r" else (w[:, 2] > 0)
                d[:, 2] *= np.where(flip, -1, 1)
                p = self._pdf(lobe, w, d)
            elif lobe == "micro_r":
                wh = tr_sample_wh(w, v0, v1, a, a)
                d = -w + 2 * _dot(w, wh)[:, None] * wh
                with np.errstate(divide="ignore", invalid="ignore"):
                    p = np.where(_same(w, d), tr_pdf(w, wh, a, a) / (4 * _dot(w, wh)), 0.0)
            else:
                wh = tr_sample_wh(w, v0, v1, a, a)
                eta = np.where(w[:, 2] > 0, 1 / ETA, ETA)
                cos_i = _dot(wh, w)
                sin2_t = eta * eta * np.maximum(0, 1 - cos_i * cos_i)
                ok = sin2_t < 1
                cos_t = np.sqrt(np.maximum(0, 1 - sin2_t))
                d = eta[:, None] * -w + (eta * cos_i - cos_t)[:, None] * wh
                p = np.where(ok, self._pdf(lobe, w, d), 0.0)
            own = self._f(lobe, w, d)
            if m > 1:  # the other lobes' pdfs, then f re-evaluated by BSDF::f's rule
                p = np.where(p > 0, p + sum(self._pdf(o, w, d) for o in self.lobes if o != lobe), 0.0) / m
                own = self.f(w, d, ng)
            wi[s], f[s], pdf[s] = d, np.where((p > 0)[:, None], own, 0.0), p
        return wi, f, pdf


def radiance_point_light(bsdf, wo, wi, intensity, r2, ng=(0, 0, 1)):
    """f(wo, wi) I |cos theta_i| / r^2: what one point light contributes at maxdepth 1 (EstimateDirect of a delta light)."""
    return bsdf.f(wo, wi, ng) * np.asarray(intensity)[None, :] * np.abs(wi[:, 2:3]) / r2[:, None]
