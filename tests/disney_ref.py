"""pbrt-v3's Disney material restated in numpy, for test_disney_truth.py / test_gpu_disney.py / disney_path_cases.py: DisneyMaterial's
BSDF (materials/disney.cpp:475-588, "scatterdistance" black) of DisneyDiffuse (:104-111), DisneyFakeSS (:138-154), DisneyRetro
(:180-192), DisneySheen (:218-225), MicrofacetReflection (core/reflection.cpp:226-236, 405-423) over DisneyMicrofacetDistribution
(disney.cpp:351-360: Trowbridge-Reitz with the separable G) and DisneyFresnel (:330-346), DisneyClearcoat (:235-318),
MicrofacetTransmission (reflection.cpp:244-266, 425-447) and LambertianTransmission (reflection.cpp:187-190, 391-403), combined by
BSDF::f / Pdf / Sample_f (reflection.cpp:686-801). Written from the reference sources alone; the oracle has no Disney material.

The lobes, in the order the material adds them (the order Sample_f counts them in and Pdf averages over), none tested for black:
    diffuse, fakess (thin), retro, sheen (sheen > 0)   -- these four iff diffuseWeight = (1 - metallic)(1 - spectrans) > 0
    micro (always), coat (clearcoat > 0), mtrans (spectrans > 0), ltrans (thin)

float64 by default; `dtype=np.float32` evaluates the same formulas in single precision (numpy's order of operations), the
parameters being float32 values either way (what the scene file's numbers become in the loader). Directions are (n, 3) arrays in
the shading frame (z up); ng is a unit vector of that frame (+z unless given).

MEASURED below (python tests/disney_ref.py prints it): per case of test_gpu_disney.CASES the worst error of the float32 mode
against the float64 one on the direction sets the GPU tests use, in units of the device bands (1e-4 relative + 1e-7 max for
f and pdf over 99.95 % of the pairs; 2e-3 + 1e-6 max for all) — the evidence that the bands are wide enough for the formulas as
such, with a factor 4 to spare (test_disney_truth.test_float32_mode_stays_inside_the_device_bands)."""
import numpy as np

from microfacet_ref import ONE_MINUS_EPSILON, _dot, _normalize, cosine_sample_hemisphere, tr_d, tr_g, tr_g1, tr_pdf, tr_sample_wh
from translucent_ref import fr_dielectric

LOBES = ("diffuse", "fakess", "retro", "sheen", "micro", "coat", "mtrans", "ltrans")
REFLECTION_LOBES = LOBES[:6]
COSINE_LOBES = LOBES[:4]   # BxDF::Sample_f / BxDF::Pdf: the cosine hemisphere on wo's side
PARAMS = dict(color=(.5, .5, .5), metallic=0., eta=1.5, roughness=.5, speculartint=0., anisotropic=0., sheen=0., sheentint=.5,
              clearcoat=0., clearcoatgloss=1., spectrans=0., thin=False, flatness=0., difftrans=1.)


def _same(wo, wi):
    return wo[:, 2] * wi[:, 2] > 0


def schlick_weight(cos, dt):
    m = np.clip(dt(1) - cos, dt(0), dt(1))
    return (m * m) * (m * m) * m


def gtr1(cos, alpha, dt):
    a2 = dt(alpha) * dt(alpha)
    return (a2 - dt(1)) / (dt(np.pi) * np.log(a2) * (dt(1) + (a2 - dt(1)) * cos * cos))


def smith_g_ggx(cos, alpha, dt):
    a2 = dt(alpha) * dt(alpha)
    c2 = cos * cos
    return dt(1) / (cos + np.sqrt(a2 + c2 - a2 * c2))


def _lerp(t, a, b):
    return (1 - t) * a + t * b


class Disney:
    """DisneyMaterial with constant parameters: the BSDF at any hit."""

    def __init__(self, dtype=np.float64, **kw):
        unknown = set(kw) - set(PARAMS)
        assert not unknown, unknown
        p = dict(PARAMS, **kw)
        self.params = p
        dt = self.dt = np.dtype(dtype).type
        f = lambda name: dt(np.float32(p[name]))
        c = np.maximum(np.asarray(p["color"], np.float32), 0).astype(dt)   # Spectrum::Clamp()
        self.c = c
        metallic, e, strans, rough = f("metallic"), f("eta"), f("spectrans"), f("roughness")
        self.metallic, self.eta, self.rough, self.thin = metallic, e, rough, bool(p["thin"])
        dw = (dt(1) - metallic) * (dt(1) - strans)
        dtr = f("difftrans") / dt(2)
        lum = dt(0.212671) * c[0] + dt(0.715160) * c[1] + dt(0.072169) * c[2]
        one = np.ones(3, dt)
        ctint = c / lum if lum > 0 else one
        sheen_w = f("sheen")
        csheen = _lerp(f("sheentint"), one, ctint) if sheen_w > 0 else np.zeros(3, dt)
        self.coef, self.lobes = {}, []
        if dw > 0:
            if self.thin:
                flat = f("flatness")
                self._add("diffuse", dw * (dt(1) - flat) * (dt(1) - dtr) * c)
                self._add("fakess", dw * flat * (dt(1) - dtr) * c)
            else:
                self._add("diffuse", dw * c)
            self._add("retro", dw * c)
            if sheen_w > 0:
                self._add("sheen", dw * sheen_w * csheen)
        aspect = dt(np.sqrt(1 - np.float64(np.float32(p["anisotropic"])) * .9))   # std::sqrt(double), stored in a Float
        self.ax, self.ay = max(dt(.001), rough * rough / aspect), max(dt(.001), rough * rough * aspect)
        r0 = (e - dt(1)) * (e - dt(1)) / ((e + dt(1)) * (e + dt(1)))   # SchlickR0FromEta
        self.cspec0 = _lerp(metallic, r0 * _lerp(f("speculartint"), one, ctint), c)
        self._add("micro", c)
        self.coat_w, self.coat_alpha = f("clearcoat"), _lerp(f("clearcoatgloss"), dt(.1), dt(.001))
        if self.coat_w > 0:
            self._add("coat", np.full(3, self.coat_w, dt))
        self.t_ax, self.t_ay, self.t_smith = self.ax, self.ay, False
        if strans > 0:
            self._add("mtrans", strans * np.sqrt(c))
            if self.thin:   # a plain TrowbridgeReitzDistribution over the roughness scaled by the index of refraction
                rs = (dt(0.65) * e - dt(0.35)) * rough
                self.t_ax, self.t_ay, self.t_smith = max(dt(.001), rs * rs / aspect), max(dt(.001), rs * rs * aspect), True
        if self.thin:
            self._add("ltrans", dtr * c)

    def _add(self, lobe, coef):
        self.lobes.append(lobe)
        self.coef[lobe] = coef.astype(self.dt)

    # ---- the lobes' f and Pdf ----
    def _f(self, lobe, wo, wi):
        dt, n = self.dt, len(wo)
        k = self.coef[lobe][None, :]
        inv_pi = dt(1 / np.pi)
        cos_o, cos_i = np.abs(wo[:, 2]), np.abs(wi[:, 2])
        if lobe == "ltrans":
            return np.repeat(k * inv_pi, n, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            if lobe == "mtrans":
                ax, ay = self.t_ax, self.t_ay
                zo, zi = wo[:, 2], wi[:, 2]
                ok = ~_same(wo, wi) & (zi != 0) & (zo != 0)
                eta = np.where(zo > 0, self.eta, dt(1) / self.eta).astype(dt)
                wh = _normalize(np.where(ok[:, None], wo + wi * eta[:, None], dt(0) * wo + np.array([0, 0, 1], dt)))
                wh = np.where((wh[:, 2] < 0)[:, None], -wh, wh)
                F = fr_dielectric(_dot(wo, wh), dt(1), self.eta, dt).astype(dt)
                sd = _dot(wo, wh) + eta * _dot(wi, wh)
                factor = dt(1) / eta
                G = tr_g(wo, wi, ax, ay) if self.t_smith else tr_g1(wo, ax, ay) * tr_g1(wi, ax, ay)
                v = (dt(1) - F) * np.abs(tr_d(wh, ax, ay) * G * eta * eta * np.abs(_dot(wi, wh)) * np.abs(_dot(wo, wh)) *
                                         factor * factor / (zi * zo * sd * sd))
                return np.where(ok[:, None], v[:, None] * k, dt(0)).astype(dt)
            Fo, Fi = schlick_weight(cos_o, dt), schlick_weight(cos_i, dt)
            if lobe == "diffuse":
                return (k * inv_pi * (dt(1) - Fo / dt(2))[:, None] * (dt(1) - Fi / dt(2))[:, None]).astype(dt)
            wh = wi + wo
            ok = np.any(wh != 0, axis=1)
            if lobe == "micro":
                ok &= (cos_i != 0) & (cos_o != 0)
            wh = _normalize(np.where(ok[:, None], wh, dt(0) * wo + np.array([0, 0, 1], dt)))
            cos_d = _dot(wi, wh)
            if lobe == "fakess":
                fss90 = cos_d * cos_d * self.rough
                fss = _lerp(Fo, dt(1), fss90) * _lerp(Fi, dt(1), fss90)
                v = (dt(1.25) * (fss * (dt(1) / (cos_o + cos_i) - dt(.5)) + dt(.5)))[:, None] * (k * inv_pi)
            elif lobe == "retro":
                rr = dt(2) * self.rough * cos_d * cos_d
                v = (rr * (Fo + Fi + Fo * Fi * (rr - dt(1))))[:, None] * (k * inv_pi)
            elif lobe == "sheen":
                v = schlick_weight(cos_d, dt)[:, None] * k
            elif lobe == "coat":
                Dr = gtr1(np.abs(wh[:, 2]), self.coat_alpha, dt)
                Fr = _lerp(schlick_weight(_dot(wo, wh), dt), dt(.04), dt(1))
                Gr = smith_g_ggx(cos_o, .25, dt) * smith_g_ggx(cos_i, .25, dt)
                v = (dt(.25) * Gr * Fr * Dr)[:, None] * k
            else:   # micro: R = c, the separable G, DisneyFresnel
                fd = fr_dielectric(cos_d, dt(1), self.eta, dt).astype(dt)
                sw = schlick_weight(cos_d, dt)
                F = _lerp(self.metallic, fd[:, None], _lerp(sw[:, None], self.cspec0[None, :], dt(1)))
                G = tr_g1(wo, self.ax, self.ay) * tr_g1(wi, self.ax, self.ay)
                v = k * (tr_d(wh, self.ax, self.ay) * G)[:, None] * F / (dt(4) * cos_i * cos_o)[:, None]
            return np.where(ok[:, None], v, dt(0)).astype(dt)

    def _pdf(self, lobe, wo, wi):
        dt = self.dt
        same = _same(wo, wi)
        cosine = np.abs(wi[:, 2]) * dt(1 / np.pi)
        if lobe in COSINE_LOBES:
            return np.where(same, cosine, dt(0)).astype(dt)
        if lobe == "ltrans":
            return np.where(~same, cosine, dt(0)).astype(dt)
        up = dt(0) * wo + np.array([0, 0, 1], dt)
        with np.errstate(divide="ignore", invalid="ignore"):
            if lobe == "micro":
                wh = _normalize(np.where(same[:, None], wo + wi, up))
                return np.where(same, tr_pdf(wo, wh, self.ax, self.ay) / (dt(4) * _dot(wo, wh)), dt(0)).astype(dt)
            if lobe == "coat":
                wh = wo + wi
                ok = same & np.any(wh != 0, axis=1)
                wh = _normalize(np.where(ok[:, None], wh, up))
                return np.where(ok, gtr1(np.abs(wh[:, 2]), self.coat_alpha, dt) / (dt(4) * _dot(wo, wh)), dt(0)).astype(dt)
            eta = np.where(wo[:, 2] > 0, self.eta, dt(1) / self.eta).astype(dt)
            wh = _normalize(np.where(~same[:, None], wo + wi * eta[:, None], up))
            sd = _dot(wo, wh) + eta * _dot(wi, wh)
            return np.where(~same, tr_pdf(wo, wh, self.t_ax, self.t_ay) * np.abs(eta * eta * _dot(wi, wh) / (sd * sd)), dt(0)).astype(dt)

    def lobe_density(self, lobe, wo, wi):
        """The density the lobe's Sample_f draws its directions with (0 where it yields none). It is the lobe's Pdf except for
        MicrofacetTransmission, whose Pdf also covers directions that no refraction at a microfacet Sample_wh draws yields (the
        microfacet facing away from wo, or wi on wo's side of it), and for DisneyClearcoat, whose Sample_f draws wh from GTR1 with alpha fixed at 0.25
        (density D(wh) cos(theta_h) over the hemisphere, so D cos / (4 wo.wh) over wi) while its Pdf is GTR1 of the gloss's alpha
        without the cosine (disney.cpp:281-318: "there still seem to be some very occasional fireflies with clearcoat")."""
        dt = self.dt
        if lobe == "coat":
            same = _same(wo, wi)
            wh = wo + wi
            ok = same & np.any(wh != 0, axis=1)
            wh = _normalize(np.where(ok[:, None], wh, dt(0) * wo + np.array([0, 0, 1], dt)))
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(ok, gtr1(np.abs(wh[:, 2]), .25, dt) * np.abs(wh[:, 2]) / (dt(4) * _dot(wo, wh)), dt(0))
        p = self._pdf(lobe, wo, wi)
        if lobe != "mtrans":
            return p
        eta = np.where(wo[:, 2] > 0, self.eta, dt(1) / self.eta).astype(dt)
        wh = (wo + wi * eta[:, None]) / (dt(1) - eta)[:, None]
        return np.where((_dot(wo, wh) > 0) & (wh[:, 2] * wo[:, 2] > 0) & (_dot(wi, wh) < 0), p, dt(0))   # (wi behind the microfacet)

    def sampling_density(self, wo, wi):
        """What BSDF::Sample_f's directions are distributed with: the lobes' densities, each picked with probability 1 / m."""
        return sum(self.lobe_density(lobe, wo, wi) for lobe in self.lobes) / self.dt(len(self.lobes))

    # ---- BSDF::f / Pdf / Sample_f ----
    def _cast(self, *arrays):
        return [np.asarray(a, self.dt) for a in arrays]

    def f(self, wo, wi, ng=(0, 0, 1)):
        wo, wi, ng = self._cast(wo, wi, ng)
        reflect = (wi @ ng) * (wo @ ng) > 0
        out = np.zeros((len(wo), 3), self.dt)
        for lobe in self.lobes:
            want = reflect if lobe in REFLECTION_LOBES else ~reflect
            out = out + np.where(want[:, None], self._f(lobe, wo, wi), self.dt(0))
        return np.where((wo[:, 2] != 0)[:, None], out, self.dt(0))

    def pdf(self, wo, wi):
        wo, wi = self._cast(wo, wi)
        p = np.zeros(len(wo), self.dt)
        for lobe in self.lobes:
            p = p + self._pdf(lobe, wo, wi)
        return np.where(wo[:, 2] != 0, p / self.dt(len(self.lobes)), self.dt(0))

    def sample_lobe(self, lobe, wo, u0, u1):
        """The lobe's own Sample_f: (wi, pdf), pdf 0 where it yields no direction."""
        dt = self.dt
        if lobe in COSINE_LOBES or lobe == "ltrans":
            d = cosine_sample_hemisphere(u0, u1).astype(dt)
            flip = (wo[:, 2] > 0) if lobe == "ltrans" else (wo[:, 2] < 0)
            d[:, 2] *= np.where(flip, dt(-1), dt(1))
            return d, self._pdf(lobe, wo, d)
        with np.errstate(divide="ignore", invalid="ignore"):
            if lobe == "micro":
                wh = tr_sample_wh(wo, u0, u1, self.ax, self.ay, dt).astype(dt)
                d = -wo + dt(2) * _dot(wo, wh)[:, None] * wh
                return d, np.where(_same(wo, d), tr_pdf(wo, wh, self.ax, self.ay) / (dt(4) * _dot(wo, wh)), dt(0)).astype(dt)
            if lobe == "coat":
                a2 = dt(.25) * dt(.25)
                cos_t = np.sqrt(np.maximum(dt(0), (dt(1) - np.power(a2, dt(1) - u0)) / (dt(1) - a2)))
                sin_t = np.sqrt(np.maximum(dt(0), dt(1) - cos_t * cos_t))
                phi = dt(2) * dt(np.pi) * u1
                wh = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], 1).astype(dt)
                wh = np.where(_same(wo, wh)[:, None], wh, -wh)
                d = -wo + dt(2) * _dot(wo, wh)[:, None] * wh
                return d, np.where(_same(wo, d), self._pdf("coat", wo, d), dt(0)).astype(dt)
            wh = tr_sample_wh(wo, u0, u1, self.t_ax, self.t_ay, dt).astype(dt)
            eta = np.where(wo[:, 2] > 0, dt(1) / self.eta, self.eta).astype(dt)
            cos_i = _dot(wh, wo)
            sin2_t = eta * eta * np.maximum(dt(0), dt(1) - cos_i * cos_i)
            ok = sin2_t < 1
            cos_t = np.sqrt(np.maximum(dt(0), dt(1) - sin2_t))
            d = eta[:, None] * -wo + (eta * cos_i - cos_t)[:, None] * wh
            d = np.where(ok[:, None], d, -wo)
            return d, np.where(ok, self._pdf("mtrans", wo, d), dt(0)).astype(dt)

    def sample(self, wo, u0, u1, ng=(0, 0, 1)):
        """(wi, f, pdf) as BSDF::Sample_f returns them; pdf 0 (and f 0) where the picked lobe gives no direction."""
        dt = self.dt
        wo, u0, u1 = self._cast(wo, u0, u1)
        n, m = len(wo), len(self.lobes)
        wi, f, pdf = np.zeros((n, 3), dt), np.zeros((n, 3), dt), np.zeros(n, dt)
        comp = np.minimum(np.floor(u0 * dt(m)).astype(int), m - 1)
        ur0 = np.minimum(u0 * dt(m) - comp.astype(dt), dt(ONE_MINUS_EPSILON))
        for c, lobe in enumerate(self.lobes):
            s = comp == c
            if not s.any():
                continue
            w = wo[s]
            d, p = self.sample_lobe(lobe, w, ur0[s], u1[s])
            own = self._f(lobe, w, d)
            if m > 1:   # the other lobes' pdfs, then f re-evaluated by BSDF::f's rule
                total = p
                for o in self.lobes:
                    if o != lobe:
                        total = total + self._pdf(o, w, d)
                p = np.where(p > 0, total, dt(0)) / dt(m)
                own = self.f(w, d, ng)
            wi[s], f[s], pdf[s] = d, np.where((p > 0)[:, None], own, dt(0)), p
        return wi, f, pdf


def radiance_point_light(bsdf, wo, wi, intensity, r2, ng=(0, 0, 1)):
    """f(wo, wi) I |cos theta_i| / r^2: what one point light contributes at maxdepth 1 (EstimateDirect of a delta light)."""
    return bsdf.f(wo, wi, ng) * np.asarray(intensity)[None, :] * np.abs(np.asarray(wi)[:, 2:3]) / np.asarray(r2)[:, None]


# ---- path_ref-style lobes: scalar BxDFs over (3,) directions of ctx.dt -----------------------------------------------------------
REFLECTION, TRANSMISSION, DIFFUSE, GLOSSY = 1, 2, 4, 8
GRAZE = 0.01   # = trace_ref.GRAZE, path_ref's margin on |cos|


class Lobe:
    """One BxDF of a Disney BSDF with path_ref's interface: type, f, pdf, sample(wo, u, ctx) -> (wi, f, pdf, type). The arithmetic
    is the vectorised class's on arrays of one direction, in the Disney's own dtype."""

    def __init__(self, bsdf, name):
        self.b, self.name = bsdf, name
        self.type = {"mtrans": TRANSMISSION | GLOSSY, "ltrans": TRANSMISSION | DIFFUSE, "micro": REFLECTION | GLOSSY,
                     "coat": REFLECTION | GLOSSY}.get(name, REFLECTION | DIFFUSE)

    def f(self, wo, wi):
        return self.b._f(self.name, wo[None, :], wi[None, :])[0]

    def pdf(self, wo, wi):
        return self.b._pdf(self.name, wo[None, :], wi[None, :])[0]

    def sample(self, wo, u, ctx):
        dt = ctx.dt
        b, name = self.b, self.name
        u = np.asarray(u, dt)
        wi, p = b.sample_lobe(name, wo[None, :], u[0:1], u[1:2])
        wi, p = wi[0].astype(dt), dt(p[0])
        if name in COSINE_LOBES or name == "ltrans":
            ctx.branch(wo[2] < 0)   # the flip onto wo's side (or away from it): wo's own margin is BSDF::sample_f's
            return wi, self.f(wo, wi), p, self.type
        if name == "mtrans":   # Refract's total internal reflection, within path_ref's margin
            wh = tr_sample_wh(wo[None, :], u[0:1], u[1:2], b.t_ax, b.t_ay, dt)[0].astype(dt)
            eta = (dt(1) / b.eta) if wo[2] > 0 else b.eta
            cos_i = wh[0] * wo[0] + wh[1] * wo[1] + wh[2] * wo[2]
            sin2_t = eta * eta * max(dt(0), dt(1) - cos_i * cos_i)
            ctx.flag(sin2_t - 1, 256 * 2.0 ** -24)
            if ctx.branch(sin2_t >= 1):
                return wi, np.zeros(3, dt), dt(0), self.type
            ctx.flag(wi[2], GRAZE)
            if ctx.branch(p == 0):
                return wi, np.zeros(3, dt), dt(0), self.type
            return wi, self.f(wo, wi), p, self.type
        ctx.flag(wi[2], GRAZE)   # micro, coat: the reflected direction leaves wo's hemisphere
        if not ctx.branch(wo[2] * wi[2] > 0):
            return wi, np.zeros(3, dt), dt(0), self.type
        return wi, self.f(wo, wi), p, self.type


def lobes(dt, **params):
    """(the BxDFs of a Disney material in the order it adds them, BSDF::eta = 1: `BSDF(*si)`), for path_ref.BSDF."""
    b = Disney(dtype=dt, **params)
    return [Lobe(b, name) for name in b.lobes], np.dtype(dt).type(1)


class DisneyMaterial:
    """A Disney material for path_ref.Scene: .text() is its .pbrt statement, .lobes(dt) its BxDFs."""
    kind = "disney"

    def __init__(self, **params):
        assert not set(params) - set(PARAMS), params
        self.params = params

    def text(self):
        out = 'Material "disney"'
        for k, v in self.params.items():
            if k == "color":
                out += f' "rgb color" [{v[0]:g} {v[1]:g} {v[2]:g}]'
            elif k == "thin":
                out += f' "bool thin" "{"true" if v else "false"}"'
            else:
                out += f' "float {k}" [{v:g}]'
        return out + "\n"

    def lobes(self, dt):
        return lobes(dt, **self.params)


# ---- the cases of test_gpu_disney.py / test_disney_truth.py: the smallest set that reaches every lobe combination -----------------
CASES = {
    "default": {},                                              # diffuse, retro, micro
    "metal": dict(metallic=1.),                                 # micro alone: the matching == 1 path
    "coated": dict(color=(.6, .3, .1), sheen=.8, sheentint=.3, clearcoat=.7, clearcoatgloss=.4, anisotropic=.7, speculartint=.6),  # five lobes
    "glassy": dict(spectrans=.6, eta=1.3),                      # + mtrans
    "all_trans": dict(spectrans=1.),                            # micro + mtrans only
    "thin_default": dict(thin=True),                            # diffuse, fakess (weight 0), retro, micro, ltrans
    "thin_all": dict(thin=True, flatness=.4, difftrans=.8, spectrans=.5, sheen=.5, clearcoat=.6, clearcoatgloss=.5, color=(.2, .5, .7)),   # all eight
    "rough0": dict(roughness=0.),                               # the .001 clamp
    "rough1": dict(roughness=1.),
    "black": dict(color=(0., 0., 0.)),                          # Ctint = 1
    "gloss0": dict(clearcoat=1., clearcoatgloss=0.),            # the widest clearcoat
}


def material_line(case):
    return DisneyMaterial(**CASES[case]).text().strip()


# ---- the float32 mode against the float64 one, in units of the device bands ------------------------------------------------------
COAT_PEAK = 0.02      # sin^2(theta_h) under which a pair sits at the clearcoat's GTR1 peak
MICRO_PEAK = 1e4      # tan^2(theta_h) / (ax ay) under which a pair sits at the peak of a microfacet lobe whose ax ay < 1e-4


def peak_mask(bsdf, wo, wi):
    """The pairs at which an ill-conditioned lobe dominates: wo and wi on one side and the half vector within the peak of the
    clearcoat's GTR1 (1 + (alpha^2 - 1) cos^2 cancels to sin^2 + alpha^2 cos^2: one float32 rounding of cos^2, 6e-8, is a relative
    error of 6e-8 / (sin^2 + alpha^2), above a quarter of the inner band's 1e-4 only where that sum is below 2.4e-3; COAT_PEAK is
    eight times that) or, for a microfacet distribution at the 0.001 clamp, of Trowbridge-Reitz's D (tan^2 / alpha^2 takes
    sin^2 = 1 - cos^2, 6e-8 absolute, over 1e-6: an error of 0.06 in e, and of 0.12 / (1 + e) in D, above 2.5e-5 where e < 5e3;
    MICRO_PEAK is twice that). Only there may a band be wider than the project's."""
    wo, wi = np.asarray(wo, np.float64), np.asarray(wi, np.float64)
    same = _same(wo, wi)
    wh = wo + wi
    wh = wh / np.maximum(np.linalg.norm(wh, axis=1, keepdims=True), 1e-300)
    c2 = wh[:, 2] ** 2
    s2 = 1 - c2
    m = np.zeros(len(wo), bool)
    if "coat" in bsdf.lobes:
        m |= same & (s2 < COAT_PEAK)
    if float(bsdf.ax) * float(bsdf.ay) < 1e-4:
        m |= same & (s2 / np.maximum(c2, 1e-300) / (float(bsdf.ax) * float(bsdf.ay)) < MICRO_PEAK)
    return m


AZIMUTH_BOUND = 1e-3 / 4   # the bound on a sampled direction's float32 conditioning error under which the 99.9 % cap applies


def azimuth_conditioned(bsdf, wo, u0):
    """True for the samples whose direction float32 can resolve to a quarter of the sample test's 1e-3. Trowbridge-Reitz's Sample_wh
    stretches wo to ws = (ax wo.x, ay wo.y, wo.z), samples a slope and rotates it back by ws's azimuth (microfacet.cpp:306-322):
    cos(phi) = ws.x / sin(theta) with sin^2(theta) = 1 - cos^2(theta), which float32 knows to 2^-24 absolute. Where sin^2(theta) =
    (ax^2 x^2 + ay^2 y^2) / |ws|^2 is s2, the azimuth is off by about 2^-24 / s2 radians (all of it below 2^-24: reflection.h:68-75
    then says phi = 0), and the sampled microfacet normal by that times alpha r, r = sqrt(u / (1 - u)) the slope's length, the
    reflected direction by twice as much. The bound E = min(1, 2^-24 / s2) 2 max(ax, ay) r is a property of (wo, u0, alpha), worked
    out in float64 from the inputs alone; samples that pick the microfacet reflection lobe with E >= AZIMUTH_BOUND are set aside
    from the direction cap: for alphas at the 0.001 clamp s2 is 1e-6 tan^2(theta_o), so that is most near-normal wo with r above a
    half (6.6 % of rough0's samples); for every other case wo within a hundredth of the normal (0.14 % for `metal`, whose one lobe takes
    every sample; under 0.07 % otherwise)."""
    wo, u0 = np.asarray(wo, np.float64), np.asarray(u0, np.float64)
    m = len(bsdf.lobes)
    ax, ay = float(bsdf.ax), float(bsdf.ay)
    comp = np.minimum(np.floor(u0 * m).astype(int), m - 1)
    ur0 = np.minimum(u0 * m - comp, ONE_MINUS_EPSILON)
    q = ax * ax * wo[:, 0] ** 2 + ay * ay * wo[:, 1] ** 2
    s2 = q / (q + wo[:, 2] ** 2)
    r = np.sqrt(ur0 / (1 - ur0))
    with np.errstate(divide="ignore"):
        E = np.minimum(1.0, 2.0 ** -24 / s2) * 2 * max(ax, ay) * r
    return ~((comp == bsdf.lobes.index("micro")) & (E >= AZIMUTH_BOUND))


def band_errors(got, want):
    """Per pair (error in units of the inner band 1e-4 |want| + 1e-7 max|want|, in units of the outer band 2e-3 |want| + 1e-6 max|want|),
    the worst channel."""
    got, want = np.asarray(got, np.float64).reshape(len(want), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    scale = np.abs(want).max()
    err = np.abs(got - want)
    if scale == 0:   # (a black colour: every f is 0, and the other side's must be)
        bad = np.where(err.any(axis=1), np.inf, 0.0)
        return bad, bad
    return (err / (1e-4 * np.abs(want) + 1e-7 * scale)).max(axis=1), (err / (2e-3 * np.abs(want) + 1e-6 * scale)).max(axis=1)


def band_units(got, want, mask):
    """(inner, outer) units outside the mask, then inside it: inner = the worst once the worst 0.05 % of ALL pairs are set aside."""
    inner, outer = band_errors(got, want)
    q = lambda a: float(np.quantile(a, 0.9995, method="lower"))
    return q(np.where(mask, 0, inner)), float(np.where(mask, 0, outer).max()), q(np.where(mask, inner, 0)), float(np.where(mask, outer, 0).max())


# case: the float32 mode against the float64 one on test_gpu_disney's direction sets (`python tests/disney_ref.py` prints them, each
# rounded up in its third digit): f then pdf, each (inner, outer) band units outside peak_mask and (inner, outer) inside it; then the
# share of samples with pdf > 0 in both modes, the share disagreeing on pdf > 0, and the share of sampled directions further than
# 1e-3 apart among the samples of azimuth_conditioned.
# Outside the mask every figure must be <= 1/4: the project's bands hold there with a factor 4 to spare. Inside it a band is the
# project's unless the figure exceeds 1/4; then it is 4 x the figure (factor()) — never set from the device's output.
MEASURED = {
    "default": (0.00921, 0.00179, 0, 0, 0.0163, 0.00192, 0, 0, 0.9796, 0, 0),
    "metal": (0.0158, 0.00274, 0, 0, 0.0161, 0.00271, 0, 0, 0.9391, 0, 0),
    "coated": (0.0187, 0.00177, 0.285, 0.0236, 0.0268, 0.00189, 0.325, 0.0244, 0.9202, 0, 0),
    "glassy": (0.0678, 0.118, 0, 0, 0.0154, 0.00233, 0, 0, 0.9169, 0, 0),
    "all_trans": (0.0994, 0.24, 0, 0, 0.0181, 0.00262, 0, 0, 0.7980, 1.01e-05, 2.54e-05),
    "thin_default": (0.00843, 0.0022, 0, 0, 0.013, 0.00226, 0, 0, 0.9879, 0, 0),
    "thin_all": (0.0178, 0.022, 0.397, 0.0345, 0.022, 0.00819, 0.511, 0.0414, 0.9049, 0, 0),
    "rough0": (1.45e-07, 4.54e-07, 187, 131, 1.18e-06, 1.7e-07, 334, 179, 1.0000, 0, 1.08e-05),
    "rough1": (0.0028, 0.000241, 0, 0, 0.00344, 0.00029, 0, 0, 0.8930, 0, 1.14e-05),
    "black": (0, 0, 0, 0, 0.0146, 0.00273, 0, 0, 0.9805, 0, 0),
    "gloss0": (0.00746, 0.000848, 0.0566, 0.00525, 0.0182, 0.00228, 0.103, 0.008, 0.9019, 0, 0),
}
# The bands wider than the project's, all inside peak_mask: coated 1.14 / 1.3 (f / pdf, the 99.95 % band), thin_all 1.59 / 2.05
# (the clearcoat at gloss 0.4 / 0.5), rough0 748 / 1336 and, for all its masked pairs, 524 / 716 of the outer band (the microfacet
# lobe at the 0.001 clamp, whose peak of 1e5 float32 does not resolve: a weak check, and the one the rule gives; every pair of rough0
# outside the mask, 84 % of them, is held to the project's bands).


def factor(u):
    return 1.0 if u <= 0.25 else 4.0 * u


def band_factors(case, mask):
    """Per pair the multipliers of (f inner, f outer, pdf inner, pdf outer) bands: 1 outside the mask, factor(MEASURED) inside."""
    m = MEASURED[case]
    pick = lambda u: np.where(mask, factor(u), 1.0)
    return pick(m[2]), pick(m[3]), pick(m[6]), pick(m[7])


# rough0 alone may lower the floor on the share of samples with pdf > 0 in both the device and the restatement to what the float64
# restatement itself reaches; it reaches 1.0000 (MEASURED), so the floor stays the project's
ROUGH0_FLOOR = 0.5


def _up(v):
    """v rounded up in its third significant digit."""
    if v == 0 or not np.isfinite(v):
        return v
    e = 10.0 ** (np.floor(np.log10(abs(v))) - 2)
    return float(np.ceil(v / e) * e)


def figures(case):
    """The MEASURED tuple of a case, computed."""
    import test_disney_truth as T
    return T.float32_band_units(case) + T.float32_sampling_figures(case)


def measure():
    for case in CASES:
        fig = figures(case)
        print(f'    "{case}": ({", ".join("%.3g" % _up(v) for v in fig[:8])}, {fig[8]:.4f}, {_up(fig[9]):.3g}, {_up(fig[10]):.3g}),')


if __name__ == "__main__":
    measure()
