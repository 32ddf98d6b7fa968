"""PathIntegrator::Li (pbrt-v3 src/integrators/path.cpp:64-194) restated in numpy for small scenes: the float64 truth the oracle's
and the device's path integrator are held to, vertex by vertex, and the same formulas in float32.

Written from the reference sources alone. What is restated here:

  the loop       path.cpp:64-194: beta, specularBounce, etaScale, Le at bounce 0 and after specular bounces only (surface Le,
                 interaction.cpp:148-151 over DiffuseAreaLight::L, diffuse.h:56-58; the infinite light on escape), the
                 `bounces >= maxDepth` break, the NEE skip for a BSDF without a non-specular lobe, f AbsDot(wi, shading.n) / pdf,
                 the beta.y() < 0 || NaN return, Russian roulette on beta etaScale with bounces > 3
  direct light   UniformSampleOneLight and EstimateDirect (integrator.cpp:85-215) with handleMedia = false, specular = false:
                 both halves, no MIS for a delta light, PowerHeuristic (sampling.h:147-150), the BSDF half ending on the sampled
                 light only, or for an infinite light on escape
  the BSDF       BSDF::f / Pdf / Sample_f (reflection.cpp:686-801) over several lobes: the lobe picked by u0, u0 remapped, the other
                 lobes' pdfs, f re-evaluated with reflection or transmission decided by the geometric normal (only when more than
                 one lobe matches, :772); LambertianReflection (:178-180), OrenNayar (reflection.h:310-317, reflection.cpp:197-219),
                 MicrofacetReflection (:226-236, 405-423), SpecularReflection (:136-143), SpecularTransmission (:150-166),
                 FresnelSpecular (:477-511), BxDF::Sample_f / Pdf (:383-395), Refract (reflection.h:85-97)
  materials      matte.cpp:44-58, plastic.cpp:45-70, mirror.cpp:44-52, glass.cpp:46-82 (smooth: one FresnelSpecular lobe),
                 uber.cpp:45-101 (opacity < 1: the pass-through SpecularTransmission(1, 1) lobe first, BSDF::eta = 1)
  the hit        Triangle::Intersect's interaction (triangle.cpp:296-400): dp/du from the default uv, n, the shading frame from
                 per-vertex normals (ns, ss, ts), SetShadingGeometry with the reversed orientation (interaction.cpp:73-92) and
                 n = Faceforward(n, ns); the sphere's (sphere.cpp:98-133); the BSDF's frame (reflection.h:170-175)
  delta lights   PointLight, SpotLight, DistantLight::Sample_li and Power (point.cpp:43-57, spot.cpp:52-83, distant.cpp:52-71)
  the sampler    GlobalSampler::Get1D / Get2D (sampler.cpp:180-195): the truth keeps its own dimension counter, starting at 5 behind
                 the camera sample (film 0-1, time 2, lens 3-4; sampler.cpp:41-47), advanced by the reference's calls in their order:
                 the light choice (1D) whenever the scene has a light and the BSDF a non-specular lobe; nothing more at that vertex if
                 lightPdf == 0; else uLight (2D), uScattering (2D); the BSDF draw (2D); the roulette draw (1D) only inside the
                 roulette test. The VALUES come from the oracle's sample_dimension(index, dim), pinned by the Halton and Sobol' known
                 answers.

What is NOT restated but taken from the suite's other truths: closest hit and any hit are trace_ref.brute_force (no tree); area
light Sample_Li / Pdf_Li / L and the infinite light are lightsample_ref's; the light choice (uniform / power / spatial) and the
point and spot lights' data are lightdistrib_ref's; Trowbridge-Reitz and FrDielectric are microfacet_ref's / translucent_ref's;
the cosine hemisphere map is ao_ref's.

SPAWNED RAYS. As in ao_ref.py a spawned ray starts at the hit point itself and is tested against every primitive but its own, so
no OffsetRayOrigin epsilon is needed. A shadow ray runs to the sampled point, leaves out the sampled light's own primitive as well
and ends at 1 - ShadowEpsilon (light.h:130-134, pbrt.h:201). The sphere is an opaque emitter: rays only leave it outwards.

DISCRETE DECISIONS. Every branch of the control flow is recorded (`Ctx.branch`); a sample is `kept` only if every decision falls
on the same side for the float64 value and for the float32-rounding interval of its expression (u = 2^-24):
  * closest-hit identity, shadow and MIS rays hit / missed: trace_ref's `decided`; the sphere: |cos| at the hit >= GRAZE, the ray's
    distance from the centre further than SPHERE_EDGE r from r, the hit further than trace_ref.BAND from a triangle's
  * any direction whose |cos| to ns or to ng is below trace_ref.GRAZE = 0.01, at either end (wo, wi): this covers SameHemisphere,
    BSDF::f's reflect test, Faceforward and the side test of Le, whose arguments are dot products of unit vectors carrying some
    tens of u (2200 u = 1.3e-4 for a direction to a point 0.1 away in a scene of extent 4: lightsample_ref's band_wi)
  * the side test of DiffuseAreaLight::L in Sample_Li: lightsample_ref's side_flag; Pdf_Li of a triangle: its edge_flag; the frame of
    the sphere's cone, CoordinateSystem's |x| > |y| of the unit vector to the centre, within 32 u
  * the light chosen: lightdistrib_ref's `undecided` (u against the cdf steps, with their bands)
  * the lobe chosen: u0 * matching against a whole number within 4 u matching (u0 is a float32 value; the product one rounding)
  * FresnelSpecular's u < F: F evaluated at cos -+ 64 u; flagged when u lies within that spread + 64 u of F (total internal
    reflection is F = 1: the same flag); Refract's sin2ThetaT >= 1 within 256 u
  * the spot light's cone: cos against cosTotalWidth within SPOT_EDGE (the falloff is continuous, so only its zero matters)
  * mc < rrThreshold and ur < q: mc = MaxComponent(beta etaScale) carries RR_REL (bounces + 1) relative: beta is a product of one
    factor f |cos| / pdf per vertex, each some tens of roundings (<= 256 u: the microfacet quotient's D G F / (4 cos cos) / pdf is
    the longest, about 60 operations), q = max(.05, 1 - mc) the same absolute amount
  * IsBlack / pdf == 0 exits are consequences of the above (they are branches: recorded and replayed, never re-decided)

FLOAT32 MODE. li(..., dtype=np.float32) evaluates the same formulas in single precision (numpy's order of operations) from the
float64 run's recorded decisions: hit identities, light and lobe choices and every branch are replayed, never re-decided. The hit's
barycentrics are Triangle::Intersect's edge functions of the float32 ray against the recorded triangle in float32 (lightsample_ref's
restatement), the hit point then b0 p0 + b1 p1 + b2 p2 in float32 (triangle.cpp:322); the sphere's hit distance is the float64 root,
the point then reprojected onto the sphere in float32 (sphere.cpp:98). The reused microfacet_ref / translucent_ref functions take the dtype. It is a restatement, not the code under test.

RETURNS per sample (PathTruth): L (3), kept, nverts (surface hits found), dim (the sampler dimension reached), n_regular / n_shadow
(scene.Intersect / IntersectP calls: what Oracle.li counts), S = the sum over the terms added to L of max-channel |term| plus one
float32 ulp of the largest emitter radiance, and `stats`, the number of samples with: roulette survived / died, a specular-then-emitter
term, a non-zero BSDF-half term, an ns != ng disagreement between the reflect test and SameHemisphere, an etaScale update, a total
internal reflection, the pass-through lobe sampled, Le of the infinite light on escape, a BSDF-half ray that ends on another
emitter than the sampled one. For diagnosis: `cond`, the worst relative float32 band of a light pdf along the path (lightsample_ref's
band_pdf_rel), `why`, the line of the first flag raised against each dropped sample, and `logs`, the recorded decisions.

BAND. Per case B = the worst |L32 - L64| / S of this module's own float32 mode over the kept samples; the band for the oracle and the
device is 4 B S per sample. `python tests/path_ref.py` (measure()) printed

    "plain_room_d8": (0.9844, 9.062e-06),   # 256 samples, 4.95 vertices; oracle 0.245 of the band; {'rr_survived': 20, 'rr_died': 220, 'bsdf_half': 35}
    "plain_room_rr0": (0.9688, 1.394e-05),   # 256 samples, 8.10 vertices; oracle 0.192 of the band; {'bsdf_half': 46}
    "plain_room_rr10": (0.9844, 9.062e-06),   # 256 samples, 4.95 vertices; oracle 0.245 of the band; {'rr_survived': 20, 'rr_died': 220, 'bsdf_half': 35}
    "plain_room_d0": (1.0000, 0.000e+00),   # 1024 samples, 1.00 vertices; oracle 0.000 of the band; {}
    "plain_room_d1": (0.9971, 6.454e-06),   # 1024 samples, 1.98 vertices; oracle 0.250 of the band; {'bsdf_half': 25}
    "normals_quad_light_uniform": (0.9609, 6.949e-06),   # 256 samples, 4.82 vertices; oracle 0.910 of the band; {'rr_survived': 18, 'rr_died': 198, 'bsdf_half': 8, 'ns_ng_disagree': 7, 'other_emitter': 1}
    "normals_quad_light_power": (0.9609, 8.291e-06),   # 256 samples, 4.82 vertices; oracle 0.615 of the band; {'rr_survived': 18, 'rr_died': 198, 'bsdf_half': 16, 'ns_ng_disagree': 7, 'other_emitter': 2}
    "normals_quad_light_spatial": (0.9297, 3.953e-06),   # 256 samples, 4.82 vertices; oracle 0.894 of the band; {'rr_survived': 18, 'rr_died': 199, 'bsdf_half': 19, 'ns_ng_disagree': 7}
    "normals_quad_light_sobol": (0.9766, 1.557e-05),   # 256 samples, 4.77 vertices; oracle 0.389 of the band; {'rr_survived': 15, 'rr_died': 198, 'bsdf_half': 11, 'ns_ng_disagree': 3}
    "delta_lights_uniform": (1.0000, 8.854e-05),   # 576 samples, 3.79 vertices; oracle 0.250 of the band; {}
    "delta_lights_power": (1.0000, 6.933e-06),   # 576 samples, 3.79 vertices; oracle 0.330 of the band; {}
    "specular": (0.9531, 9.852e-05),   # 256 samples, 4.92 vertices; oracle 0.165 of the band; {'rr_survived': 33, 'rr_died': 207, 'specular_emitter': 7, 'bsdf_half': 4, 'eta_scale': 45, 'tir': 6, 'pass_through': 20}
    "infinite": (0.9912, 2.941e-05),   # 1024 samples, 0.42 vertices; oracle 0.251 of the band; {'bsdf_half': 411, 'escaped_le': 599}

(the line is the entry of MEASURED below: kept share, B). Where the oracle's share of the band is 0.25, its float32 result on the sample
that sets B is the float32 mode's own.
"""
import sys
import warnings

import numpy as np

import ao_ref
import lightdistrib_ref as LD
import lightsample_ref as LS
import microfacet_ref as MR
import trace_ref
from translucent_ref import fr_dielectric

U = 2.0 ** -24
GRAZE = trace_ref.GRAZE
SPHERE_EDGE = 1e-5      # relative distance of a ray from the sphere's silhouette under which hit-or-miss is undecided
SPOT_EDGE = 1e-4        # |cos - cosTotalWidth| under which the spot's zero is undecided (band_wi of a near point, see above)
RR_REL = 256 * U        # relative band of beta per vertex
SHADOW_EPSILON = 1e-4
ONE_MINUS_EPSILON = np.float32(1) - np.float32(2.0 ** -24)

REFLECTION, TRANSMISSION, DIFFUSE, GLOSSY, SPECULAR = 1, 2, 4, 8, 16
SPHERE = -2   # the sphere as a primitive id (triangles are 0 .. T - 1, -1 is a miss)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def _normalize(v):
    return v / np.sqrt(_dot(v, v))


def _black(s):
    return not (s != 0).any()


def _lum(s):
    return 0.212671 * s[0] + 0.715160 * s[1] + 0.072169 * s[2]


class Ctx:
    """One sample's record of decisions. float64: branches and choices are logged and margins judged (`kept`); any other dtype: they
    are replayed from `log`."""

    def __init__(self, dt, log=None):
        self.dt, self.replay = dt, log is not None
        self.log = log if log is not None else []
        self.pos, self.kept, self.why = 0, True, 0
        self.stats = dict(rr_survived=0, rr_died=0, specular_emitter=0, bsdf_half=0, ns_ng_disagree=0, eta_scale=0, tir=0, pass_through=0,
                          escaped_le=0, other_emitter=0)
        self.S, self.cond = 0.0, 0.0
        self.n_regular = self.n_shadow = self.nverts = 0

    def _next(self, v):
        if self.replay:
            v = self.log[self.pos]
            self.pos += 1
        else:
            self.log.append(v)
        return v

    def branch(self, cond):
        return self._next(bool(cond))

    def choice(self, v):
        return self._next(v)

    def flag(self, gap, margin):
        """The decision `gap > 0` (or its like) is undecided within `margin`."""
        self.drop(not (abs(float(gap)) > margin), 2)

    def drop(self, cond=True, up=1):
        if not self.replay and cond:
            if self.kept:
                self.why = sys._getframe(up).f_lineno   # the first flag raised, for measure()'s account of the flagged shares
            self.kept = False


# ---- BxDFs in the shading frame (z up); scalar: w is a (3,) array of ctx.dt ---------------------------------------------------
def _same_hemisphere(a, b):
    return a[2] * b[2] > 0


class Lambertian:
    type = REFLECTION | DIFFUSE

    def __init__(self, R):
        self.R = R

    def f(self, wo, wi):
        return self.R * wo.dtype.type(1 / np.pi)

    def pdf(self, wo, wi):  # BxDF::Pdf, reflection.cpp:393-395
        dt = wo.dtype.type
        return abs(wi[2]) * dt(1 / np.pi) if _same_hemisphere(wo, wi) else dt(0)

    def sample(self, wo, u, ctx):  # BxDF::Sample_f, reflection.cpp:383-391
        dt = ctx.dt
        w, _ = ao_ref.cosine_hemisphere(np.asarray(u, dt)[None, :], dt)
        wi = w[0].astype(dt)
        if ctx.branch(wo[2] < 0):
            wi = wi * np.array([1, 1, -1], dt)
        return wi, self.f(wo, wi), self.pdf(wo, wi), self.type


class OrenNayar(Lambertian):
    def __init__(self, R, sigma_deg):
        dt = R.dtype.type
        self.R = R
        sigma = dt(np.pi / 180) * dt(sigma_deg)   # Radians(sigma)
        s2 = sigma * sigma
        self.A = dt(1) - s2 / (dt(2) * (s2 + dt(0.33)))
        self.B = dt(0.45) * s2 / (s2 + dt(0.09))

    def f(self, wo, wi):
        dt = wo.dtype.type
        sin = lambda w: np.sqrt(np.maximum(dt(0), dt(1) - w[2] * w[2]))
        si, so = sin(wi), sin(wo)
        max_cos = dt(0)
        if si > 1e-4 and so > 1e-4:
            cphi = lambda w, s: np.clip(w[0] / s, dt(-1), dt(1))
            sphi = lambda w, s: np.clip(w[1] / s, dt(-1), dt(1))
            max_cos = np.maximum(dt(0), cphi(wi, si) * cphi(wo, so) + sphi(wi, si) * sphi(wo, so))
        if abs(wi[2]) > abs(wo[2]):
            sin_alpha, tan_beta = so, si / abs(wi[2])
        else:
            sin_alpha, tan_beta = si, so / abs(wo[2])
        return self.R * dt(1 / np.pi) * (self.A + self.B * max_cos * sin_alpha * tan_beta)


class Microfacet:
    """MicrofacetReflection over TrowbridgeReitzDistribution(alpha, alpha) and FresnelDielectric(eta_i, eta_t)."""
    type = REFLECTION | GLOSSY

    def __init__(self, R, alpha, eta_i, eta_t):
        self.R, self.alpha, self.eta_i, self.eta_t = R, alpha, eta_i, eta_t

    def f(self, wo, wi):
        dt = wo.dtype.type
        cos_o, cos_i = abs(wo[2]), abs(wi[2])
        wh = wi + wo
        if cos_i == 0 or cos_o == 0 or not wh.any():
            return np.zeros(3, dt)
        wh = _normalize(wh)
        F = dt(fr_dielectric(_dot(wi, wh), self.eta_i, self.eta_t, dt))
        a = self.alpha
        D, G = dt(MR.tr_d(wh[None, :], a, a)[0]), dt(MR.tr_g(wo[None, :], wi[None, :], a, a)[0])
        return self.R * D * G * F / (dt(4) * cos_i * cos_o)

    def _pdf_wh(self, wo, wh):
        dt = wo.dtype.type
        return dt(MR.tr_pdf(wo[None, :], wh[None, :], self.alpha, self.alpha)[0]) / (dt(4) * _dot(wo, wh))

    def pdf(self, wo, wi):
        if not _same_hemisphere(wo, wi):
            return wo.dtype.type(0)
        return self._pdf_wh(wo, _normalize(wo + wi))

    def sample(self, wo, u, ctx):
        dt = ctx.dt
        wh = MR.tr_sample_wh(wo[None, :], np.array([u[0]]), np.array([u[1]]), self.alpha, self.alpha, dt)[0].astype(dt)
        wi = -wo + dt(2) * _dot(wo, wh) * wh   # Reflect, reflection.h:81-83
        ctx.flag(wi[2], GRAZE)
        if not ctx.branch(_same_hemisphere(wo, wi)):
            return wi, np.zeros(3, dt), dt(0), self.type
        return wi, self.f(wo, wi), self._pdf_wh(wo, wh), self.type


def _refract(wi, n, eta, ctx):
    """Refract (reflection.h:85-97) -> wt or None."""
    dt = ctx.dt
    cos_i = _dot(n, wi)
    sin2_i = np.maximum(dt(0), dt(1) - cos_i * cos_i)
    sin2_t = eta * eta * sin2_i
    ctx.flag(sin2_t - 1, 256 * U)
    if ctx.branch(sin2_t >= 1):
        return None
    cos_t = np.sqrt(dt(1) - sin2_t)
    return eta * -wi + (eta * cos_i - cos_t) * n


class SpecularReflection:
    type = REFLECTION | SPECULAR

    def __init__(self, R, eta_i=None, eta_t=None):   # eta None: FresnelNoOp
        self.R, self.eta_i, self.eta_t = R, eta_i, eta_t

    def f(self, wo, wi):
        return np.zeros(3, wo.dtype)

    def pdf(self, wo, wi):
        return wo.dtype.type(0)

    def sample(self, wo, u, ctx):
        dt = ctx.dt
        wi = wo * np.array([-1, -1, 1], dt)
        F = dt(1) if self.eta_i is None else dt(fr_dielectric(wi[2], self.eta_i, self.eta_t, dt))
        return wi, F * self.R / abs(wi[2]), dt(1), self.type


class SpecularTransmission(SpecularReflection):
    type = TRANSMISSION | SPECULAR

    def __init__(self, T, eta_a, eta_b):
        self.T, self.eta_a, self.eta_b = T, eta_a, eta_b

    def sample(self, wo, u, ctx):
        dt = ctx.dt
        entering = ctx.branch(wo[2] > 0)
        eta_i, eta_t = (self.eta_a, self.eta_b) if entering else (self.eta_b, self.eta_a)
        n = np.array([0, 0, 1 if entering else -1], dt)   # Faceforward(Normal3f(0, 0, 1), wo)
        wi = _refract(wo, n, dt(eta_i) / dt(eta_t), ctx)
        if wi is None:
            return wo, np.zeros(3, dt), dt(0), self.type
        ft = self.T * (dt(1) - dt(fr_dielectric(wi[2], self.eta_a, self.eta_b, dt)))
        ft = ft * ((dt(eta_i) * dt(eta_i)) / (dt(eta_t) * dt(eta_t)))   # TransportMode::Radiance
        return wi, ft / abs(wi[2]), dt(1), self.type


class FresnelSpecular(SpecularReflection):
    type = REFLECTION | TRANSMISSION | SPECULAR

    def __init__(self, R, T, eta_a, eta_b):
        self.R, self.T, self.eta_a, self.eta_b = R, T, eta_a, eta_b

    def sample(self, wo, u, ctx):
        dt = ctx.dt
        F = dt(fr_dielectric(wo[2], self.eta_a, self.eta_b, dt))
        if not ctx.replay:
            c = float(wo[2])
            spread = max(abs(float(fr_dielectric(np.clip(c + s * 64 * U, -1, 1), self.eta_a, self.eta_b)) - float(F)) for s in (-1, 1))
            ctx.flag(float(u[0]) - float(F), spread + 64 * U)
        if ctx.branch(u[0] < F):
            ctx.stats["tir"] += F == 1
            wi = wo * np.array([-1, -1, 1], dt)
            return wi, F * self.R / abs(wi[2]), F, REFLECTION | SPECULAR
        entering = ctx.branch(wo[2] > 0)
        eta_i, eta_t = (self.eta_a, self.eta_b) if entering else (self.eta_b, self.eta_a)
        n = np.array([0, 0, 1 if entering else -1], dt)
        wi = _refract(wo, n, dt(eta_i) / dt(eta_t), ctx)
        if wi is None:
            return wo, np.zeros(3, dt), dt(0), TRANSMISSION | SPECULAR
        ft = self.T * (dt(1) - F) * ((dt(eta_i) * dt(eta_i)) / (dt(eta_t) * dt(eta_t)))
        return wi, ft / abs(wi[2]), dt(1) - F, TRANSMISSION | SPECULAR


class BSDF:
    """reflection.h:170-175 and reflection.cpp:686-801. ns, ng, ss in world space; ts = Cross(ns, ss)."""

    def __init__(self, lobes, ns, ng, ss, eta):
        self.lobes, self.ns, self.ng, self.ss, self.ts, self.eta = lobes, ns, ng, ss, _cross(ns, ss), eta

    def local(self, v):
        return np.array([_dot(v, self.ss), _dot(v, self.ts), _dot(v, self.ns)], v.dtype)

    def world(self, v):
        return self.ss * v[0] + self.ts * v[1] + self.ns * v[2]

    def matching(self, specular):
        return [b for b in self.lobes if specular or not b.type & SPECULAR]

    def _graze(self, ctx, wW, w):
        ctx.flag(w[2], GRAZE)
        ctx.flag(_dot(wW, self.ng), GRAZE)

    def _sum_f(self, woW, wiW, wo, wi, lobes, ctx):
        dt = ctx.dt
        reflect = ctx.branch(_dot(wiW, self.ng) * _dot(woW, self.ng) > 0)
        if not ctx.replay and reflect != bool(_same_hemisphere(wo, wi)):
            ctx.stats["ns_ng_disagree"] += 1
        f = np.zeros(3, dt)
        for b in lobes:
            if (reflect and b.type & REFLECTION) or (not reflect and b.type & TRANSMISSION):
                f = f + b.f(wo, wi)
        return f

    def f(self, woW, wiW, ctx):
        wi, wo = self.local(wiW), self.local(woW)
        self._graze(ctx, woW, wo), self._graze(ctx, wiW, wi)
        if ctx.branch(wo[2] == 0):
            return np.zeros(3, ctx.dt)
        return self._sum_f(woW, wiW, wo, wi, self.matching(False), ctx)

    def pdf(self, woW, wiW, ctx):
        dt = ctx.dt
        lobes = self.matching(False)
        wi, wo = self.local(wiW), self.local(woW)
        if not lobes or ctx.branch(wo[2] == 0):
            return dt(0)
        pdf = dt(0)
        for b in lobes:
            pdf = pdf + b.pdf(wo, wi)
        return pdf / dt(len(lobes))

    def sample_f(self, woW, u, ctx, specular):
        """-> (wiW, f, pdf, sampled type); pdf == 0 where the reference returns black."""
        dt = ctx.dt
        lobes = self.matching(specular)
        m = len(lobes)
        zero = (woW, np.zeros(3, dt), dt(0), 0)
        if m == 0:
            return zero
        x = u[0] * dt(m)
        if m > 1:
            ctx.flag(float(x) - round(float(x)), 4 * U * m)
        comp = ctx.choice(min(int(np.floor(x)), m - 1))
        bxdf = lobes[comp]
        ur = np.array([min(x - dt(comp), dt(ONE_MINUS_EPSILON)), u[1]], dt)
        wo = self.local(woW)
        self._graze(ctx, woW, wo)
        if ctx.branch(wo[2] == 0):
            return zero
        wi, f, pdf, stype = bxdf.sample(wo, ur, ctx)
        ctx.flag(wi[2], GRAZE)   # before the exit: |wi.z| / Pi is a pdf, and 0 only where float32 says so too
        if ctx.branch(pdf == 0):
            return zero
        wiW = self.world(wi)
        self._graze(ctx, wiW, wi)
        if not bxdf.type & SPECULAR and m > 1:
            for b in lobes:
                if b is not bxdf:
                    pdf = pdf + b.pdf(wo, wi)
        if m > 1:
            pdf = pdf / dt(m)
        if not bxdf.type & SPECULAR and m > 1:
            f = self._sum_f(woW, wiW, wo, wi, lobes, ctx)
        return wiW, f, pdf, stype


# ---- materials ------------------------------------------------------------------------------------------------------------------
class Material:
    """kind: matte / plastic / mirror / glass / uber, with the parameters of the .pbrt statement (defaults as Create*Material's)."""

    def __init__(self, kind, Kd=None, Ks=None, Kr=None, Kt=None, sigma=0.0, roughness=0.1, index=1.5, opacity=1.0):
        d = {"matte": (0.5, 0, 0, 0), "plastic": (0.25, 0.25, 0, 0), "mirror": (0, 0, 0.9, 0), "glass": (0, 0, 1, 1), "uber": (0.25, 0.25, 0, 0)}[kind]
        rgb = lambda v, dflt: np.full(3, dflt, np.float32) if v is None else np.broadcast_to(np.asarray(v, np.float32), (3,)).copy()
        self.kind, self.Kd, self.Ks, self.Kr, self.Kt = kind, rgb(Kd, d[0]), rgb(Ks, d[1]), rgb(Kr, d[2]), rgb(Kt, d[3])
        self.sigma, self.roughness, self.index, self.opacity = np.float32(sigma), np.float32(roughness), np.float32(index), rgb(opacity, 1.0)

    def text(self):
        s = lambda n, v: f' "rgb {n}" [{v[0]:g} {v[1]:g} {v[2]:g}]'
        k = self.kind
        if k == "matte":
            return f'Material "matte"{s("Kd", self.Kd)} "float sigma" [{self.sigma:g}]\n'
        if k == "plastic":
            return f'Material "plastic"{s("Kd", self.Kd)}{s("Ks", self.Ks)} "float roughness" [{self.roughness:g}]\n'
        if k == "mirror":
            return f'Material "mirror"{s("Kr", self.Kr)}\n'
        if k == "glass":
            return f'Material "glass"{s("Kr", self.Kr)}{s("Kt", self.Kt)} "float index" [{self.index:g}]\n'
        return (f'Material "uber"{s("Kd", self.Kd)}{s("Ks", self.Ks)}{s("Kr", self.Kr)}{s("Kt", self.Kt)}{s("opacity", self.opacity)}'
                f' "float roughness" [{self.roughness:g}] "float index" [{self.index:g}]\n')

    def _alpha(self, dt):
        return dt(MR.roughness_to_alpha(dt(self.roughness)))   # remaproughness defaults to true

    def lobes(self, dt):
        """(the BxDFs in the order the material adds them, BSDF::eta)."""
        c = lambda v: np.clip(v, 0, None).astype(dt)   # Spectrum::Clamp()
        k, out, eta = self.kind, [], dt(1)
        if k == "matte":
            if self.Kd.any():
                sig = np.clip(self.sigma, 0, 90)
                out.append(Lambertian(c(self.Kd)) if sig == 0 else OrenNayar(c(self.Kd), sig))
        elif k == "plastic":
            if self.Kd.any():
                out.append(Lambertian(c(self.Kd)))
            if self.Ks.any():
                out.append(Microfacet(c(self.Ks), self._alpha(dt), dt(1.5), dt(1)))
        elif k == "mirror":
            out.append(SpecularReflection(c(self.Kr)))
        elif k == "glass":
            eta = dt(self.index)
            if self.Kr.any() or self.Kt.any():
                out.append(FresnelSpecular(c(self.Kr), c(self.Kt), dt(1), eta))
        else:
            e, op = dt(self.index), c(self.opacity)
            t = np.clip(dt(1) - op, 0, None)
            if t.any():
                out.append(SpecularTransmission(t, dt(1), dt(1)))
            else:
                eta = e
            if (op * c(self.Kd)).any():
                out.append(Lambertian(op * c(self.Kd)))
            if (op * c(self.Ks)).any():
                out.append(Microfacet(op * c(self.Ks), self._alpha(dt), dt(1), e))
            if (op * c(self.Kr)).any():
                out.append(SpecularReflection(op * c(self.Kr), dt(1), e))
            if (op * c(self.Kt)).any():
                out.append(SpecularTransmission(op * c(self.Kt), dt(1), e))
        return out, eta


# ---- lights ---------------------------------------------------------------------------------------------------------------------
class LightSample:
    def __init__(self, wi, Li, pdf, target=None):
        self.wi, self.Li, self.pdf, self.target = wi, Li, pdf, target   # target None: the shadow ray runs to infinity


class AreaLight:
    """A DiffuseAreaLight on triangle `prim` or on the sphere: lightsample_ref's."""
    delta = infinite = False

    def __init__(self, ls, prim, choice):
        self.ls, self.prim, self.choice = ls, prim, choice

    def power(self):
        return self.choice.power()

    def sample_li(self, ctx, p, u):
        dt = ctx.dt
        s = self.ls.sample_li(p[None, :].astype(dt), np.asarray(u, dt)[None, :], dt)
        ctx.drop(bool(s.side_flag[0]) or bool(s.unconditioned[0]))
        if self.prim == SPHERE and not ctx.replay:   # CoordinateSystem's |x| > |y| (geometry.h:1020-1027) picks the cone's frame
            wc = self.ls.shape.pc - p.astype(np.float64)
            ctx.flag((abs(wc[0]) - abs(wc[1])) / np.linalg.norm(wc), 32 * U)
        ctx.cond = max(ctx.cond, float(s.band_pdf_rel[0]))
        return LightSample(s.wi[0].astype(dt), s.Li[0].astype(dt), dt(s.pdf[0]), s.p[0].astype(dt))

    def pdf_li(self, ctx, p, wi):
        dt = ctx.dt
        r = self.ls.pdf_li(p[None, :].astype(dt), wi[None, :].astype(dt), dt)
        ctx.drop(bool(r.edge_flag[0]))
        ctx.cond = max(ctx.cond, float(r.band_pdf_rel[0]))
        return dt(r.pdf[0])

    def L(self, n, w):   # diffuse.h:56-58
        dt = w.dtype.type
        return self.ls.L.astype(dt) if (self.ls.two_sided or _dot(n, w) > 0) else np.zeros(3, dt)


class SpherePower:
    def __init__(self, radius, L):
        self.radius, self.L = float(radius), np.asarray(L, np.float64)

    def power(self):  # diffuse.cpp: Lemit area Pi
        return LD.lum(self.L * 4 * np.pi * self.radius ** 2 * np.pi)


class PointLight:
    delta, infinite, prim = True, False, None

    def __init__(self, pos, I):
        self.choice = LD.Point(pos, I)

    def power(self):
        return self.choice.power()

    def _falloff(self, ctx, wi):
        return ctx.dt(1)

    def sample_li(self, ctx, p, u):   # point.cpp:43-53, spot.cpp:52-62
        dt = ctx.dt
        pl = self.choice.pos.astype(dt)
        w = pl - p
        d2 = _dot(w, w)
        wi = w / np.sqrt(d2)
        return LightSample(wi, self.choice.I.astype(dt) * self._falloff(ctx, wi) / d2, dt(1), pl)


class SpotLight(PointLight):
    def __init__(self, pos, to, I, cone=30.0, delta=5.0):
        self.choice = LD.Spot(pos, to, I, cone, delta)

    def _falloff(self, ctx, wi):   # spot.cpp:66-76: the cone's axis is +z of light space
        dt, c = ctx.dt, self.choice
        cos = -_dot(wi, c.axis.astype(dt))
        total, start = dt(np.float32(c.cos_total)), dt(np.float32(c.cos_start))
        ctx.flag(cos - total, SPOT_EDGE)
        if ctx.branch(cos < total):
            return dt(0)
        if ctx.branch(cos >= start):
            return dt(1)
        d = (cos - total) / (start - total)
        return (d * d) * (d * d)


class DistantLight:
    delta, infinite, prim = True, False, None

    def __init__(self, frm, to, L, world_radius):
        w = np.array(frm, np.float32).astype(np.float64) - np.array(to, np.float32).astype(np.float64)
        self.w, self.Lv, self.world_radius = w / np.linalg.norm(w), np.array(L, np.float32).astype(np.float64), float(world_radius)
        self.choice = self

    def power(self):   # distant.cpp:68-71
        return LD.lum(self.Lv * np.pi * self.world_radius ** 2)

    def sample_li(self, ctx, p, u):
        dt = ctx.dt
        return LightSample(self.w.astype(dt), self.Lv.astype(dt), dt(1), None)


class InfiniteLight:
    delta, infinite, prim = False, True, None

    def __init__(self, ls):
        self.ls, self.choice = ls, self

    def power(self):   # infinite.cpp:85-90
        return LD.lum(np.pi * self.ls.world_radius ** 2 * self.ls.mip.lookup(np.array([[0.5, 0.5]]), 0.5)[0])

    def sample_li(self, ctx, p, u):
        dt = ctx.dt
        s = self.ls.sample_li(p[None, :].astype(dt), np.asarray(u, np.float32)[None, :], dt)
        return LightSample(s.wi[0].astype(dt), s.Li[0].astype(dt), dt(s.pdf[0]), None)

    def pdf_li(self, ctx, p, wi):
        dt = ctx.dt
        r = self.ls.pdf_li(wi[None, :].astype(dt), dt)
        ctx.drop(bool(r.cell_flag[0]))
        return dt(r.pdf[0])

    def le(self, d):
        dt = d.dtype.type
        return self.ls.le(d[None, :], dt).L[0].astype(dt)


# ---- the scene ------------------------------------------------------------------------------------------------------------------
class Hit:
    pass


class Scene:
    """Triangles (declared under the identity transform, in the order of the file), at most one sphere, materials and lights.

    tris (T, 9) float32; normals (T, 9) with nan rows where the mesh has none; flip (T,): ReverseOrientation; tri_mat (T,): index into
    mats; sphere: None or dict(center, radius, mat, L); lights: the list in the scene's order (area lights where their shape is
    declared), built by path_cases."""

    def __init__(self, tris, normals, flip, tri_mat, mats, sphere, lights, max_depth, rr_threshold=1.0, strategy="spatial"):
        self.P = np.asarray(tris, np.float32).astype(np.float64).reshape(-1, 9)
        self.N = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 9)
        self.flip, self.tri_mat, self.mats, self.sphere, self.lights = np.asarray(flip, bool), np.asarray(tri_mat), mats, sphere, lights
        self.max_depth, self.rr_threshold = int(max_depth), float(np.float32(rr_threshold))
        self.strategy = "uniform" if len(lights) == 1 else strategy   # CreateLightSampleDistribution, lightdistrib.cpp:49
        self.tri_light = np.full(len(self.P), -1)
        self.sphere_light = -1
        for i, lt in enumerate(lights):
            if lt.prim == SPHERE:
                self.sphere_light = i
            elif lt.prim is not None:
                self.tri_light[lt.prim] = i
        self.infinite = [lt for lt in lights if lt.infinite]
        lo, hi = self.bounds()
        self.distrib = LD.Scene([lt.choice for lt in lights], lo, hi) if lights else None
        self._others, self._tri = {}, {}
        radiance = [np.abs(lt.ls.L).max() for lt in lights if isinstance(lt, AreaLight)] + [lt.ls.T for lt in self.infinite]
        radiance += [np.abs(lt.Lv).max() for lt in lights if isinstance(lt, DistantLight)]
        radiance += [np.abs(lt.choice.I).max() for lt in lights if isinstance(lt, PointLight)]
        self.floor = float(np.spacing(np.float32(max(radiance)))) if radiance else 0.0

    def bounds(self):
        """scene.WorldBound(): the union of the vertices and of the sphere's box, float32 values."""
        pts = self.P.reshape(-1, 3)
        lo, hi = pts.min(0), pts.max(0)
        if self.sphere:
            c, r = np.asarray(self.sphere["center"], np.float64), self.sphere["radius"]
            lo, hi = np.minimum(lo, np.float32(c - r)), np.maximum(hi, np.float32(c + r))
        return lo, hi

    def world_radius(self):   # Bounds3::BoundingSphere, geometry.h
        lo, hi = [np.asarray(b, np.float32) for b in self.bounds()]
        c = (lo + hi) / np.float32(2)
        return float(np.sqrt(((hi - c) ** 2).sum(dtype=np.float32)))

    def _without(self, skip):
        key = tuple(sorted(skip))
        if key not in self._others:
            keep = np.array([i for i in range(len(self.P)) if i not in key], int)
            self._others[key] = (keep, self.P[keep])
        return self._others[key]

    def _sphere_t(self, o, d, tmax):
        """The sphere's nearest root in (0, tmax) in float64 -> (t or inf, decided)."""
        if not self.sphere:
            return np.inf, True
        c, r = np.asarray(self.sphere["center"], np.float64), float(self.sphere["radius"])
        oc = o - c
        a, b, cc = d @ d, 2 * (d @ oc), oc @ oc - r * r
        h = np.sqrt(max(oc @ oc - (d @ oc) ** 2 / a, 0.0))   # the line's distance from the centre
        ahead = -(d @ oc) / a > 0 or cc < 0
        decided = abs(h - r) > SPHERE_EDGE * r or not ahead
        disc = b * b - 4 * a * cc
        if disc < 0:
            return np.inf, decided
        q = np.sqrt(disc)
        for t in sorted(((-b - q) / (2 * a), (-b + q) / (2 * a))):
            if 0 < t < tmax:
                n = (o + t * d - c) / r
                cos = abs(n @ d) / np.sqrt(a)
                return t, decided and cos >= GRAZE and t > trace_ref.T_SMALL * (np.linalg.norm(oc) + r)
        return np.inf, decided

    def closest(self, ctx, o, d, own):
        """scene.Intersect from (o, d), every primitive but `own` -> Hit or None."""
        dt = ctx.dt
        ctx.n_regular += 1
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        if not ctx.replay:
            keep, P = self._without(() if own in (-1, SPHERE) else (own,))
            tr = trace_ref.brute_force(P, o64[None, :], d64[None, :], [np.inf])
            ctx.drop(not tr.decided[0])
            t, prim = tr.t_min[0], -1
            if tr.hit[0]:
                ties = np.nonzero(tr.ties[0])[0]
                ctx.drop(len(ties) > 1)
                prim = int(keep[ties[0]])
            if own != SPHERE:
                ts, ok = self._sphere_t(o64, d64, np.inf)
                ctx.drop(not ok)
                if np.isfinite(ts) and np.isfinite(t):
                    ctx.drop(abs(ts - t) <= trace_ref.BAND * min(ts, t))
                if ts < t:
                    t, prim = ts, SPHERE
        prim = ctx.choice(prim if not ctx.replay else None)
        if prim == -1:
            return None
        ctx.nverts += 1
        h = Hit()
        h.prim = prim
        wo = -d
        if prim == SPHERE:
            t, _ = self._sphere_t(o64, d64, np.inf)
            c, r = np.asarray(self.sphere["center"], dt), dt(self.sphere["radius"])
            po = (o + dt(t) * d) - c
            po = po * (r / np.sqrt(_dot(po, po)))     # sphere.cpp:98
            ctx.drop(float(po[0] ** 2 + po[1] ** 2) < 1e-6 * float(r) ** 2)   # the pole: no dp/du
            h.p = c + po
            h.n = h.ns = _normalize(po)               # Cross(dpdu, dpdv) points outwards (thetaMax - thetaMin < 0)
            h.ss = _normalize(np.array([-po[1], po[0], 0], dt))   # dpdu = (-phiMax y, phiMax x, 0)
            h.mat, h.light = self.sphere["mat"], self.sphere_light
            return h
        T = self.P[prim]
        p0, p1, p2 = T[0:3].astype(dt), T[3:6].astype(dt), T[6:9].astype(dt)
        # the barycentrics as Triangle::Intersect has them (triangle.cpp:231-295, lightsample_ref's restatement of it in dt), from the
        # unoffset origin; the hit point is then triangle.cpp:322
        if prim not in self._tri:
            self._tri[prim] = LS.Triangle(T[0:3], T[3:6], T[6:9])
        _, b, _ = self._tri[prim]._intersect(o[None, :], d[None, :], dt)
        b0, b1, b2 = dt(b[0, 0]), dt(b[0, 1]), dt(b[0, 2])
        h.p = b0 * p0 + b1 * p1 + b2 * p2
        dp02, dp12 = p0 - p2, p1 - p2
        n = _normalize(_cross(dp02, dp12))
        dpdu = p1 - p0   # (duv12[1] dp02 - duv02[1] dp12) / det under the default uv (0,0) (1,0) (1,1): -dp02 + dp12
        flip = bool(self.flip[prim])
        if not np.isnan(self.N[prim, 0]):
            n0, n1, n2 = self.N[prim, 0:3].astype(dt), self.N[prim, 3:6].astype(dt), self.N[prim, 6:9].astype(dt)
            ns = _normalize(b0 * n0 + b1 * n1 + b2 * n2)
            ss = _normalize(dpdu)
            ts = _normalize(_cross(ss, ns))
            ss = _cross(ts, ns)
            sn = _normalize(_cross(ss, ts))            # SetShadingGeometry
            if flip:
                sn = -sn
            ctx.flag(_dot(n, sn), GRAZE)
            if ctx.branch(_dot(n, sn) < 0):            # n = Faceforward(n, shading.n), twice over
                n = -n
            h.n, h.ns, h.ss = n, sn, _normalize(ss)
        else:
            if flip:
                n = -n
            h.n = h.ns = n
            h.ss = _normalize(dpdu)
        h.mat, h.light = int(self.tri_mat[prim]), int(self.tri_light[prim])
        return h

    def occluded(self, ctx, o, target, d, skip):
        """!VisibilityTester::Unoccluded: IntersectP towards `target` (or along d without end), `skip` primitives left out."""
        ctx.n_shadow += 1
        if ctx.replay:
            return ctx.branch(None)
        o64 = o.astype(np.float64)
        if target is not None:
            d64, tmax = target.astype(np.float64) - o64, 1 - SHADOW_EPSILON
        else:
            d64, tmax = d.astype(np.float64), np.inf
        _, P = self._without([s for s in skip if s >= 0])
        tr = trace_ref.brute_force(P, o64[None, :], d64[None, :], [tmax])
        ctx.drop(not tr.decided[0])
        hit = bool(tr.any_hit()[0])
        if SPHERE not in skip:
            ts, ok = self._sphere_t(o64, d64, tmax)
            ctx.drop(not ok)
            hit |= bool(np.isfinite(ts))
        return ctx.branch(hit)

    def bsdf(self, h, dt):
        lobes, eta = self.mats[h.mat].lobes(dt)
        return BSDF(lobes, h.ns, h.n, h.ss, eta)

    def le(self, ctx, h, w):
        """SurfaceInteraction::Le(w)."""
        if h.light < 0:
            return np.zeros(3, ctx.dt)
        ctx.flag(_dot(h.n, w), GRAZE)
        return self.lights[h.light].L(h.n, w)


class Sampler:
    """GlobalSampler::Get1D / Get2D over the oracle's sample_dimension: the truth's own dimension counter."""

    def __init__(self, value, dim=5):
        self.value, self.dim = value, dim

    def get1d(self):
        self.dim += 1
        return self.value(self.dim - 1)

    def get2d(self):
        self.dim += 2
        return np.array([self.value(self.dim - 2), self.value(self.dim - 1)], np.float32)


def _power_heuristic(f, g):   # sampling.h:147-150 with nf = ng = 1
    return (f * f) / (f * f + g * g)


def _add(ctx, L, term):
    ctx.S += float(np.abs(term).max())
    return L + term


def _estimate_direct(scene, ctx, h, bsdf, wo, light, li, u_light, u_scat):
    dt = ctx.dt
    Ld = np.zeros(3, dt)
    # A point of the emitting sphere itself: OffsetRayOrigin towards the centre puts the origin inside (sphere.cpp:224-226, 285-287), so
    # Sample draws over the whole sphere, whose every other point faces away (L is black), and Pdf intersects the sphere along a ray
    # that leaves it outwards and misses (pdf 0).
    on_light = h.prim == SPHERE and light.prim == SPHERE
    s = LightSample(wo, np.zeros(3, dt), dt(0)) if on_light else light.sample_li(ctx, h.p, u_light)
    if ctx.branch(s.pdf > 0 and not _black(s.Li)):
        f = bsdf.f(wo, s.wi, ctx) * abs(_dot(s.wi, h.ns))
        spdf = bsdf.pdf(wo, s.wi, ctx)
        if ctx.branch(not _black(f)):
            if not scene.occluded(ctx, h.p, s.target, s.wi, (h.prim, light.prim if light.prim is not None else -1)):
                if light.delta:
                    Ld = Ld + f * s.Li / s.pdf
                else:
                    Ld = Ld + f * s.Li * _power_heuristic(s.pdf, spdf) / s.pdf
    if not light.delta:
        wi, f, spdf, _ = bsdf.sample_f(wo, u_scat, ctx, False)
        f = f * abs(_dot(wi, h.ns))
        if ctx.branch(not _black(f) and spdf > 0):
            lpdf = dt(0) if on_light else light.pdf_li(ctx, h.p, wi)
            if ctx.branch(lpdf == 0):
                return Ld
            weight = _power_heuristic(spdf, lpdf)
            h2 = scene.closest(ctx, h.p, wi, h.prim)
            ctx.nverts -= h2 is not None   # a light-sampling ray's hit is no path vertex
            Li = np.zeros(3, dt)
            if h2 is not None:
                if h2.light == li:
                    Li = scene.le(ctx, h2, -wi)
                elif h2.light >= 0 and not ctx.replay and scene.le(Ctx(dt), h2, -wi).any():
                    ctx.stats["other_emitter"] += 1   # lightIsect.primitive->GetAreaLight() != &light: no contribution
            elif light.infinite:
                Li = light.le(wi)
            if ctx.branch(not _black(Li)):
                term = f * Li * weight / spdf
                if not ctx.replay and term.any():
                    ctx.stats["bsdf_half"] += 1
                Ld = Ld + term
    return Ld


def _li_one(scene, ctx, o, d, sampler):
    dt = ctx.dt
    L, beta = np.zeros(3, dt), np.ones(3, dt)
    ro, rd, own = o.astype(dt), d.astype(dt), -1
    specular, eta_scale, bounces = False, dt(1), 0
    while True:
        h = scene.closest(ctx, ro, rd, own)
        if bounces == 0 or specular:
            if h is not None:
                Le = scene.le(ctx, h, -rd)
                if not ctx.replay and specular and Le.any():
                    ctx.stats["specular_emitter"] += 1
                L = _add(ctx, L, beta * Le)
            else:
                for lt in scene.infinite:
                    ctx.stats["escaped_le"] += 1
                    L = _add(ctx, L, beta * lt.le(rd))
        if h is None or bounces >= scene.max_depth:
            break
        bsdf = scene.bsdf(h, dt)
        wo = -rd
        if bsdf.matching(False) and scene.lights:      # UniformSampleOneLight
            u = sampler.get1d()
            p64 = h.p.astype(np.float64)[None, :]
            if ctx.replay:
                li, lpdf = ctx.choice(None)
                lpdf = dt(scene.distrib.choose(scene.strategy, p64, [u], dt)[1][0][li]) if dt is not np.float64 else lpdf
            else:
                ls, pdfs, undecided, _ = scene.distrib.choose(scene.strategy, p64, [u])
                ctx.drop(bool(undecided[0]))
                li, lpdf = ctx.choice((int(ls[0]), float(pdfs[0][ls[0]])))
            if not ctx.branch(lpdf == 0):
                u_light, u_scat = sampler.get2d(), sampler.get2d()
                Ld = _estimate_direct(scene, ctx, h, bsdf, wo, scene.lights[li], li, u_light, u_scat) / dt(lpdf)
                L = _add(ctx, L, beta * Ld)
        wi, f, pdf, flags = bsdf.sample_f(wo, sampler.get2d(), ctx, True)
        if ctx.branch(_black(f) or pdf == 0):
            break
        beta = beta * f * abs(_dot(wi, h.ns)) / pdf
        if ctx.branch(_lum(beta) < 0 or np.isnan(_lum(beta))):
            break
        specular = bool(flags & SPECULAR)
        if flags & SPECULAR and flags & TRANSMISSION:
            ctx.flag(_dot(wo, h.n), GRAZE)
            e2 = bsdf.eta * bsdf.eta
            eta_scale = eta_scale * (e2 if ctx.branch(_dot(wo, h.n) > 0) else dt(1) / e2)
            ctx.stats["eta_scale" if bsdf.eta != 1 else "pass_through"] += 1
        ro, rd, own = h.p, wi, h.prim
        mc = (beta * eta_scale).max()
        if bounces > 3:
            band = RR_REL * (bounces + 1) * float(mc)
            ctx.flag(float(mc) - scene.rr_threshold, band)
            if ctx.branch(mc < scene.rr_threshold):
                q = np.maximum(dt(0.05), dt(1) - mc)
                ur = sampler.get1d()
                ctx.flag(float(ur) - float(q), band)
                if ctx.branch(ur < q):
                    ctx.stats["rr_died"] += 1
                    break
                ctx.stats["rr_survived"] += 1
                beta = beta / (dt(1) - q)
        bounces += 1
    return L


class PathTruth:
    pass


def li(scene, cam_o, cam_d, sample_value, dtype=np.float64, logs=None):
    """Li of camera rays (cam_o[i], cam_d[i]); sample_value(i, dim) is the sampler's value of that camera sample in dimension dim.
    dtype other than float64 needs `logs`, the `logs` of the float64 run."""
    n = len(cam_o)
    r = PathTruth()
    r.L, r.kept, r.S, r.cond = np.zeros((n, 3), dtype), np.ones(n, bool), np.zeros(n), np.zeros(n)
    r.nverts, r.dim, r.n_regular, r.n_shadow = (np.zeros(n, int) for _ in range(4))
    r.stats, r.why = {}, {}
    r.logs = []
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")   # lightsample_ref on one-ray arrays: numpy's scalar-conversion deprecation, once per ray
        for i in range(n):
            ctx = Ctx(dtype, None if logs is None else logs[i])
            sampler = Sampler(lambda dim, i=i: sample_value(i, dim))
            r.L[i] = _li_one(scene, ctx, np.asarray(cam_o[i]), np.asarray(cam_d[i]), sampler)
            r.kept[i], r.S[i], r.nverts[i], r.dim[i] = ctx.kept, ctx.S + scene.floor, ctx.nverts, sampler.dim
            r.n_regular[i], r.n_shadow[i], r.cond[i] = ctx.n_regular, ctx.n_shadow, ctx.cond
            r.logs.append(ctx.log)
            if not ctx.kept:
                r.why[ctx.why] = r.why.get(ctx.why, 0) + 1
            for k, v in ctx.stats.items():
                r.stats[k] = r.stats.get(k, 0) + (v > 0)
    return r


# ---- the inputs of a frame's camera samples, from the CPU oracle's sampler and camera -------------------------------------------
def frame_inputs(oracle, host):
    """(px, py, k, camera origins, directions, sample_value(i, dim)) of every camera sample of the scene's film."""
    px, py, k = ao_ref.frame_samples(host)
    idx = [oracle.sample_index(host, int(x), int(y), int(kk)) for x, y, kk in zip(px, py, k)]
    pfilm = np.array([(np.float32(x) + oracle.sample_dimension(host, ix, 0, x, y), np.float32(y) + oracle.sample_dimension(host, ix, 1, x, y))
                      for x, y, ix in zip(px, py, idx)], np.float32)
    o, d = oracle.camera_rays(host, pfilm)
    cache = {}

    def value(i, dim):
        if (i, dim) not in cache:
            cache[i, dim] = oracle.sample_dimension(host, idx[i], dim, int(px[i]), int(py[i]))
        return cache[i, dim]
    return px, py, k, o, d, value


_CACHE = {}


def case_truth(binding, oracle, tmp_path_factory, name):
    """The float64 truth of one of path_cases.CASES, computed once per session: (host, px, py, k, PathTruth, (scene, o, d, value))."""
    if name not in _CACHE:
        import path_cases
        scene, text, files = path_cases.build(name)
        root = tmp_path_factory.mktemp("path_truth")
        p = root / (name + ".pbrt")
        p.write_text(text)
        for fname, rows in files.items():
            from test_image_light_scenes import write_pfm
            write_pfm(root / fname, rows)
        host = binding.HostScene(path=str(p))
        host.scene_path = str(p)
        px, py, k, o, d, value = frame_inputs(oracle, host)
        _CACHE[name] = (host, px, py, k, li(scene, o, d, value), (scene, o, d, value))
    return _CACHE[name]


def rel_distance(L, truth):
    """max-channel |L - L64| / S per sample."""
    return np.abs(np.asarray(L, np.float64) - truth.L).max(1) / truth.S


def float32_distance(name, binding, oracle, tmp_path_factory):
    """(B of the case: the worst rel_distance of the float32 mode over the kept samples, the float32 PathTruth)."""
    _, _, _, _, tr, (scene, o, d, value) = case_truth(binding, oracle, tmp_path_factory, name)
    t32 = li(scene, o, d, value, np.float32, tr.logs)
    return float(rel_distance(t32.L, tr)[tr.kept].max()), t32


# what measure() printed: per case (kept share, B)
MEASURED = {
    "plain_room_d8": (0.9844, 9.062e-06),   # 256 samples, 4.95 vertices; oracle 0.245 of the band; {'rr_survived': 20, 'rr_died': 220, 'bsdf_half': 35}
    "plain_room_rr0": (0.9688, 1.394e-05),   # 256 samples, 8.10 vertices; oracle 0.192 of the band; {'bsdf_half': 46}
    "plain_room_rr10": (0.9844, 9.062e-06),   # 256 samples, 4.95 vertices; oracle 0.245 of the band; {'rr_survived': 20, 'rr_died': 220, 'bsdf_half': 35}
    "plain_room_d0": (1.0000, 0.000e+00),   # 1024 samples, 1.00 vertices; oracle 0.000 of the band; {}
    "plain_room_d1": (0.9971, 6.454e-06),   # 1024 samples, 1.98 vertices; oracle 0.250 of the band; {'bsdf_half': 25}
    "normals_quad_light_uniform": (0.9609, 6.949e-06),   # 256 samples, 4.82 vertices; oracle 0.910 of the band; {'rr_survived': 18, 'rr_died': 198, 'bsdf_half': 8, 'ns_ng_disagree': 7, 'other_emitter': 1}
    "normals_quad_light_power": (0.9609, 8.291e-06),   # 256 samples, 4.82 vertices; oracle 0.615 of the band; {'rr_survived': 18, 'rr_died': 198, 'bsdf_half': 16, 'ns_ng_disagree': 7, 'other_emitter': 2}
    "normals_quad_light_spatial": (0.9297, 3.953e-06),   # 256 samples, 4.82 vertices; oracle 0.894 of the band; {'rr_survived': 18, 'rr_died': 199, 'bsdf_half': 19, 'ns_ng_disagree': 7}
    "normals_quad_light_sobol": (0.9766, 1.557e-05),   # 256 samples, 4.77 vertices; oracle 0.389 of the band; {'rr_survived': 15, 'rr_died': 198, 'bsdf_half': 11, 'ns_ng_disagree': 3}
    "delta_lights_uniform": (1.0000, 8.854e-05),   # 576 samples, 3.79 vertices; oracle 0.250 of the band; {}
    "delta_lights_power": (1.0000, 6.933e-06),   # 576 samples, 3.79 vertices; oracle 0.330 of the band; {}
    "specular": (0.9531, 9.852e-05),   # 256 samples, 4.92 vertices; oracle 0.165 of the band; {'rr_survived': 33, 'rr_died': 207, 'specular_emitter': 7, 'bsdf_half': 4, 'eta_scale': 45, 'tir': 6, 'pass_through': 20}
    "infinite": (0.9912, 2.941e-05),   # 1024 samples, 0.42 vertices; oracle 0.251 of the band; {'bsdf_half': 411, 'escaped_le': 599}
}


def measure():
    """python tests/path_ref.py: per case the kept share and the float32 mode's worst relative distance from the float64 truth."""
    import pathlib
    import sys
    import tempfile
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
    import conftest
    import oracle_binding
    import path_cases
    import __graft_entry__ as ge
    ge.build_if_needed()
    binding, oracle = conftest.load_binding(), oracle_binding.Oracle()

    class Factory:
        def mktemp(self, name):
            return pathlib.Path(tempfile.mkdtemp(prefix=name))
    for name in path_cases.CASES:
        host, px, py, k, tr, _ = case_truth(binding, oracle, Factory(), name)
        B, t32 = float32_distance(name, binding, oracle, Factory())
        L, nr = oracle.li(host, px, py, k)
        frac = rel_distance(L, tr)[tr.kept].max() / (4 * B) if B else 0.0
        live = {k_: int(v) for k_, v in tr.stats.items() if v}
        print(f'    "{name}": ({tr.kept.mean():.4f}, {B:.3e}),   # {len(px)} samples, {tr.nverts.mean():.2f} vertices; oracle {frac:.3f} of the band; {live}')


if __name__ == "__main__":
    measure()
