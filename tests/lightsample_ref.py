"""How the sampled lights are sampled, restated in float64 from the reference alone: the area lights on a sphere, a triangle, a
disk or a cylinder, and the infinite light over its environment map.

  Sphere       Sphere::Area, Sample(u), Sample(ref, u), Pdf(ref, wi) (shapes/sphere.cpp:217-306) over UniformSampleSphere
               (core/sampling.cpp:98-103), UniformConePdf (:112), CoordinateSystem (core/geometry.h:1020-1027), SphericalDirection
               (:1467-1472) and, for Pdf from inside, Sphere::Intersect (sphere.cpp:50-155)
  Triangle     Triangle::Area, Sample(u) (shapes/triangle.cpp:546-579) with the per-vertex-normal Faceforward and the orientation
               flip; UniformSampleTriangle (sampling.cpp:154-157)
  Disk         Disk::Area, Sample(u) (shapes/disk.cpp:125-138) over ConcentricSampleDisk (sampling.cpp:81-96): Sample draws over
               the whole disk of `radius` whatever innerradius and phimax say, Area and Pdf count the partial disk only
  Cylinder     Cylinder::Area, Sample(u) (shapes/cylinder.cpp:204-221)
  Shape        Shape::Sample(ref, u), Shape::Pdf(ref, wi) (core/shape.cpp:56-87). The reference Interaction has pError = 0, so
               OffsetRayOrigin (core/geometry.h:1428-1444) adds the offset Dot(Abs(n), pError) n = 0 and moves no coordinate: a
               ray leaves ref.p itself whatever ref.n is. Disk and cylinder intersections are quadric_ref.py's.
  Area light   DiffuseAreaLight::Sample_Li, Pdf_Li (lights/diffuse.cpp:68-87) and L (lights/diffuse.h:56-58), one- and two-sided
  1D and 2D    Distribution1D (constructor, SampleContinuous; core/sampling.h:57-89) over FindInterval (core/pbrt.h:399-412);
               Distribution2D (constructor core/sampling.cpp:159-174, SampleContinuous and Pdf core/sampling.h:127-141)
  Infinite     InfiniteAreaLight's scalar image (lights/infinite.cpp:64-83: filtered luminance x sin theta, fwidth = 0.5 /
               min(w, h)), Le (:92-96), Sample_Li (:98-122), Pdf_Li (:124-132) over SphericalTheta / SphericalPhi
               (geometry.h:1474-1481); the MIPMap and its lookups are mipmap_ref.py's

Every evaluation takes a dtype: float64 is the truth, float32 the same formulas in single precision (numpy's order of operations,
numpy's libm; not the device's) - the tests use it to see that every case keeps inside the bands and the caps before a device
is asked: every value is computed in that dtype, Shape::Pdf's intersection (triangle, sphere, disk, cylinder) and the infinite light's
bilinear lookup included; the bands and the flags always belong to the float64 evaluation. Scene data (matrices, vertices, radiance, the infinite light's tables) are float32 values held exactly.

THE BANDS. A device evaluates all this in float32: u = 2^-24 per rounding, the constant Pi is a float32 (one u), the portable
sin / cos / acos / atan2 lie within one float32 ulp of the true function of their float32 argument (<= 2 u for a value in
[-1, 1], <= 4 u for an angle up to Pi, <= 8 u up to 2 Pi). R is the largest coordinate a case touches (reference point, light).
Every band below is per sample and is returned beside the value it belongs to (fields named band_*; *_rel means relative to the
value). A difference of two float32 values is one rounding of the result: |d(a - b)| <= u |a - b|.

Shared: w = pLight - ref.p, d = |w|. If a coordinate of pLight moves by ep: a coordinate of w by ep + u |w_i|, d^2 by
(2 sqrt3 ep / d + 5 u) relative, the unit direction wi = w / d by
    band_wi = 2 sqrt3 ep / d + 4 u                                               per coordinate.
The cosine at the light is c = N / d, N = Dot(n, ref.p - pLight). With en the band of a coordinate of n and ep_off the part of ep
that leaves the tangent plane at pLight (a sample that slides along a flat emitter does not move N):
    eN = sqrt3 ep_off + (sqrt3 en + 4 u) d          band_side = eN / d
DiffuseAreaLight::L's side test Dot(n, -wi) > 0 is decided when |c| > band_side: side_flag marks the others. A two-sided light
has no side test and no flag. c itself moves by rc = band_side / |c| + sqrt3 ep / d + 3 u relative, and the area-to-solid-angle
pdf = d^2 / (|c| Area), with Area's own relative band ea and 4 u for the quotient's roundings, by
    band_pdf_rel = ea + 2 sqrt3 ep / d + 9 u + rc / (1 - rc)                     (= u (a + b R / d + c' / |cos|), ep ~ u R)
and where rc >= 1 the quotient is not conditioned at all: band_pdf_rel = inf there (the tests count those samples against
the 1 % cap of the side test, in whose neighbourhood they lie).

Sphere, seen from outside (cone sampling). v = pc - p, s2 = sinThetaMax2 = r^2 / |v|^2 carries 8 u relative (5 u of |v|^2, r^2,
the quotient); x = 1 - s2 moves by 8 u s2 + u x; cosThetaMax = cm = sqrt(x) by
    ecm = (8 u s2 + u x) / (2 cm) + u cm = u (4 s2 / cm + 1.5 cm).
1 - cm moves by ecm + u (1 - cm); 2 Pi (1 - cm) and the quotient are 4 u more (Pi among them):
    band_pdf_rel = (ecm + u (1 - cm)) / (1 - cm) + 5 u                           (= k u / (1 - cosThetaMax), k = 4 s2 / cm + 1.5 cm + (1 - cm)).
At d / r = 1000 that is 1.5 u / 5e-7 = 0.18: about three bits of the pdf are left, by the reference's own arithmetic.
The sampled point: cosTheta = ct = (1 - u0) + u0 cm moves by ect = 3 u + ecm; S = dc^2 sinTheta^2 with sinTheta^2 = 1 - ct^2
(moves by 2 ct ect + 2 u, the square root and its re-squaring 3 u relative) and dc^2 (8 u relative) by
    eS = dc^2 (2 ct ect + 2 u + 14 u sin^2); B = r^2 - S by eB = u r^2 + eS + u |B|; sqrt(B) by
    esB = min(eB / sqrt(B), sqrt(eB)) + u sqrt(B)                               <- the ds cancellation: at the silhouette B -> 0
ds = dc ct - sqrt(B) moves by eds = dc (ect + 5 u) + esB + u |ds|. cosAlpha = ca = (dc^2 + r^2 - ds^2) / (2 dc r):
    eca = [11 u dc^2 + 3 u r^2 + 2 |ds| eds + u ds^2] / (2 dc r) + 7 u |ca|.
sinAlpha = sa = sqrt(1 - ca^2): 1 - ca^2 moves by e1 = 2 |ca| eca + 2 u, esa = min(e1 / sa, sqrt(e1)) + u sa (at u0 -> 0, sa -> 0 and
the reference's own arithmetic leaves the square root of e1). The frame: wc = Normalize(v) 5 u per coordinate; wcX divides by a
length >= sqrt(1/2): 18 u; wcY = Cross(wc, wcX): 49 u; phi = u1 2 Pi 3 u relative (19 u), its sine and cosine 21 u. The normal
nWorld = sa cos(phi) (-wcX) + sa sin(phi) (-wcY) + ca (-wc), per coordinate (|cos wcX_i| + |sin wcY_i| <= sqrt2):
    band_n = 1.5 esa + eca + 100 u        band_p = r band_n + 2 u (|pc| + r)      (pWorld = pc + r nWorld)
A cone sample's N = Dot(n, ref.p - pWorld): n and pWorld = pc + r n move together, so the shared eN (which lets them move apart)
is far too wide close to the sphere, where d is small and sinAlpha is lost. With ref.p - pc = -dc wc: N = -dc Dot(n, wc) - r |n|^2 -
Dot(n, rounding of pWorld). Dot(n, wc) = -ca up to the frame's lack of orthogonality (12 u per pair, lengths 4 u): it moves by
eca + 70 u sa + 5 u and NOT by esa; |n|^2 - 1 by 2 (sa esa + |ca| eca) + 50 u <= 2 (e1 + eca) + 50 u; the rounding of pWorld is
2 u (|pc| + r) per coordinate; the dot product's own roundings 5 u d:
    eN = dc (eca + 70 u sa + 5 u) + r (2 e1 + 2 eca + 50 u) + 2 sqrt3 u (|pc| + r) + 5 u d        band_side = eN / d
Sphere, seen from inside (area sampling). z = 1 - 2 u0 one rounding; 1 - z^2 moves by 4 u, rr = sqrt(.) by
err = min(4 u / rr, 2 sqrt u) + u rr; phi and its sine and cosine as above. pObj = r (rr cos, rr sin, z) per coordinate
    eo = r (err + 30 u) + 8 u r                                                  (the reprojection r / |pObj| among them)
With sM = the largest absolute row sum of ObjectToWorld's 3 x 3 and sN of its inverse transpose, L = |mInv^T pObj|:
    band_p = sM eo + 4 u (sM r + |pc|)         band_n = 2 sqrt3 sN (eo + 4 u r) / L + 4 u
Area = phiMax r (zMax - zMin): ea = 4 u. The pdf is the shared area-to-solid-angle band with ep = band_p, en = band_n.
Sphere::Pdf from inside intersects the sphere from ref.p (one root ahead): the hit is reprojected onto the sphere, so it moves
along the surface only, by 40 u (R + r) / |c| per coordinate (the parametric distance's float32 error, EFloat-bounded in the
reference, turned by the obliquity); its normal by that over r. A partial sphere's clipping (zMin, zMax, phiMax) is hit-or-miss:
edge_flag marks hits within 64 u (R + r) / |c| of a clipping edge.

Triangle. b0 = 1 - sqrt(u0), b1 = u1 sqrt(u0), b2 = 1 - b0 - b1 move by 2 u, 2 u, 4 u; p = b0 p0 + b1 p1 + b2 p2 is ten more roundings
at magnitude R (the largest vertex coordinate): band_p = 16 u R per coordinate, of which the three products and two sums (5 u R) can
leave the triangle's plane: ep_off = 5 u R. The normal Normalize(Cross(e1, e2)), e1 = p1 - p0
and e2 = p2 - p0 one rounding each: a coordinate of the cross product moves by 5 u |e1| |e2|, its length is |e1| |e2| sin(gamma):
    band_n = (10 / sin(gamma) + 3) u          ea = (9 / sin(gamma) + 3) u          (Area = 0.5 |Cross|, pdf = 1 / Area)
gamma the angle of the edges at p0. Faceforward and the orientation flip only change the sign. Shape::Pdf intersects the triangle
(Triangle::Intersect, triangle.cpp:231-378; the hit is b0 p0 + b1 p1 + b2 p2, band_p as above with 6 u more for the barycentrics'
quotients). Its vertices are translated to the ray origin (P = p - o, u |P| per coordinate), permuted so that the ray's largest
component is z, and sheared: x' = Px + Sx Pz with Sx = -dx / dz, |Sx| <= 1, three roundings: x' moves by
    ex = u (|Px| + 3 |Sx Pz| + |x'|)                                              (ey likewise)
The edge function e0 = x1' y2' - y1' x2' (two products, one difference) by
    de0 = |y2'| ex1 + |x1'| ey2 + |x2'| ey1 + |y1'| ex2 + 2 u (|x1' y2'| + |y1' x2'|) + u |e0|
and the barycentric coordinate b_i = e_i / (e0 + e1 + e2) by
    eb_i = (de_i + |b_i| (de0 + de1 + de2)) / |e0 + e1 + e2| + 2 u                 (per ray, from its float64 values)
With D twice the largest coordinate of a translated vertex,
hit-or-miss is decided when every barycentric coordinate of the float64 intersection is further than its eb_i from 0 (and the
hit further than 64 u D along the ray): edge_flag marks the others.

Disk and cylinder. ConcentricSampleDisk: 6 roundings and one sine / cosine of an angle <= Pi / 2 whose quotient carries 2 u:
a coordinate of pObj moves by 12 u radius; Cylinder: 14 u (radius + |z|). Through ObjectToWorld (row sum sM, translation t):
    band_p = sM 14 u (radius + |z|) + 4 u (sM (radius + |z|) + |t|)
The normal is Normalize(ObjectToWorld(Normal3f)) of an object-space normal that moves by 24 u (cylinder; the disk's is exact):
band_n = 2 sqrt3 sN 24 u |nObj| / L + 12 u (the transform's own nine roundings and the normalisation). ea = 5 u. Shape::Pdf: the
hit moves by 40 u (R + size) / |c|; the edge flag marks every candidate hit within that (in object units, times sN) of an edge of
the partial shape, and rays that graze the cylinder (Quadric._edge_flag).

Distribution1D::SampleContinuous over a GIVEN float32 table: every comparison cdf[i] <= u is exact, so the offset is exact; du =
(u - cdf[o]) / (cdf[o + 1] - cdf[o]) carries 3 u relative and (o + du) / n moves by band_d = 5 u. func[o] / funcInt is one rounding.
Infinite light, Sample_Li: theta = d1 Pi moves by 7 Pi u, phi = d0 2 Pi by 14 Pi u; with the ulp of sine and cosine 24 u and
46 u; a coordinate of the light-space direction by 72 u, of wi = LightToWorld(.) (a rotation: row sums <= sqrt3, three products and
two sums) by band_wi = 136 u; the shadow ray's target ref.p + wi (2 worldRadius) by 2 worldRadius band_wi + 4 u (|ref.p| + 2 worldRadius). pdf = pdf0 pdf1 / (2 Pi^2 sinTheta): 9 roundings and sinTheta's 24 u:
    band_pdf_rel = (9 + 24 / sinTheta) u.
The radiance Lmap->Lookup(st) is MIPMap::triangle on level 0 (w x h texels, repeat): s w - 0.5 moves by (6 u w + u |s w|) texels, so
with G the map's largest difference between neighbouring texels (across the seam and, since t wraps as well, across the poles
too) and T its largest texel
    band_L = G (7 u w + 7 u h) (band_d / (5 u)) + 10 u T                          (bilinear: continuous; ten roundings at T)
Le and Pdf_Li of a world direction d: wl = WorldToLight(d) moves by 6 u |d| per coordinate (8 u once normalised, Le only); theta =
acos(z) by eth = e / sinTheta + 4 u, phi = atan2(y, x) by eph = sqrt2 e / sinTheta + 8 u (e = 6 u or 8 u; + 2 Pi for phi < 0
among them); s = phi Inv2Pi and t = theta InvPi 2 u more. Le: band_L = G (w (eph / 2 Pi + 2 u) + h (eth / Pi + 2 u) + u (w + h)) +
10 u T, capped at the map's whole range. Pdf_Li: Distribution2D::Pdf's cell is int(p0 w), int(p1 h) (clamped): cell_flag marks the
directions whose p0 w or p1 h lies within w (eph / 2 Pi + 3 u) or h (eth / Pi + 3 u) of a whole number (the seam at p0 = 0 or 1 too
where the two cells differ); the others carry band_pdf_rel = (eth + 2 u) / sinTheta + 8 u. A flagged direction is left out of the
comparison with the truth's own cell, but not of every comparison: its pdf is that of one of the (at most four) cells within
those distances, within the same band (pdf_alt) - a read outside the row, for one, is none of them.
The host's tables against the truth built from the image: see table_bands.
"""
import numpy as np

import quadric_ref as Q
from mipmap_ref import MipMap

U = 2.0 ** -24
SQRT3 = np.sqrt(3.0)


class Out(dict):
    """A record of per-sample arrays, fields by attribute."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _dot(a, b):
    return (a * b).sum(-1)


def _len(a):
    return np.sqrt(_dot(a, a))


def _normalize(a):
    return a / _len(a)[..., None]


def _f32data(a):
    """Scene data: float32 values, held exactly in float64."""
    return np.asarray(a, np.float32).astype(np.float64)


def _point(m, p, dtype):
    m = m.astype(dtype)
    return p @ m[:3, :3].T + m[:3, 3]


def _normal(minv, n, dtype):  # Transform::operator()(Normal3f), transform.h:244-252: the inverse's transpose
    return n @ minv.astype(dtype)[:3, :3]


def lum(rgb):
    return 0.212671 * rgb[..., 0] + 0.715160 * rgb[..., 1] + 0.072169 * rgb[..., 2]


# ---- core/sampling.cpp, core/geometry.h -------------------------------------------------------------------------------------------
def uniform_sample_sphere(u0, u1, dtype):
    z = 1 - 2 * u0
    r = np.sqrt(np.maximum(dtype(0), 1 - z * z))
    phi = 2 * dtype(np.pi) * u1
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


def concentric_sample_disk(u0, u1, dtype):
    ox, oy = 2 * u0 - 1, 2 * u1 - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.abs(ox) > np.abs(oy)
        r = np.where(first, ox, oy)
        theta = np.where(first, dtype(np.pi / 4) * (oy / ox), dtype(np.pi / 2) - dtype(np.pi / 4) * (ox / oy))
        out = np.stack([r * np.cos(theta), r * np.sin(theta)], -1)
    return np.where(((ox == 0) & (oy == 0))[..., None], dtype(0), out)


def uniform_sample_triangle(u0, u1):
    su0 = np.sqrt(u0)
    return 1 - su0, u1 * su0


def coordinate_system(v1):
    x, y, z = v1[..., 0], v1[..., 1], v1[..., 2]
    zero = np.zeros_like(x)
    a = np.stack([-z, zero, x], -1) / np.sqrt(x * x + z * z)[..., None]
    b = np.stack([zero, z, -y], -1) / np.sqrt(y * y + z * z)[..., None]
    v2 = np.where((np.abs(x) > np.abs(y))[..., None], a, b)
    return v2, np.cross(v1, v2)


def _solid_angle_pdf(ref_p, p, n, area, dtype, ep, en, ea, ep_off=None):
    """Shape::Sample(ref, u)'s conversion (shape.cpp:58-68) of the area pdf 1 / area at the sampled (p, n) -> (pdf, wi, cos at
    the light, band_pdf_rel, band_wi, band_side). ep_off: the part of ep that leaves the surface's tangent plane (default: all)."""
    ep_off = ep if ep_off is None else ep_off
    w = p - ref_p
    d2 = _dot(w, w)
    with np.errstate(divide="ignore", invalid="ignore"):
        wi = w / np.sqrt(d2)[..., None]
        c = _dot(n, -wi)
        pdf = (1 / area) * d2 / np.abs(c)
        pdf = np.where((d2 == 0) | ~np.isfinite(pdf), dtype(0), pdf)
        d = np.sqrt(d2.astype(np.float64))
        band_wi = np.where(d > 0, 2 * SQRT3 * ep / d + 4 * U, 0.0)
        side = SQRT3 * ep_off / d + SQRT3 * en + 4 * U  # eN / d
        ac = np.abs(c.astype(np.float64))
        rc = side / ac + SQRT3 * ep / d + 3 * U
        rel = np.where(rc < 1, ea + 2 * SQRT3 * ep / d + 9 * U + rc / np.maximum(1 - rc, 1e-300), np.inf)
    return pdf, np.where((d2 == 0)[..., None], dtype(0), wi), c, np.where(d2 == 0, 0.0, rel), band_wi, np.where(d2 == 0, 0.0, side)


# ---- the shapes -----------------------------------------------------------------------------------------------------------------
class Sphere:
    def __init__(self, o2w, o2w_inv, radius, zmin=None, zmax=None, phimax=360.0, reverse=False):
        """zmin, zmax, phimax as the .pbrt file gives them (degrees); the constructor's clamps are sphere.h:51-60."""
        self.m, self.inv = _f32data(o2w).reshape(4, 4), _f32data(o2w_inv).reshape(4, 4)
        self.radius = float(np.float32(radius))
        zmin, zmax = (-radius if zmin is None else zmin), (radius if zmax is None else zmax)
        self.zmin = float(np.float32(np.clip(min(zmin, zmax), -radius, radius)))
        self.zmax = float(np.float32(np.clip(max(zmin, zmax), -radius, radius)))
        self.phimax = float(np.float32(np.radians(np.float32(np.clip(phimax, 0, 360)))))
        self.reverse = bool(reverse)
        self.pc = self.m[:3, 3].copy()  # (*ObjectToWorld)(Point3f(0, 0, 0)): w = 1
        self.sM = np.abs(self.m[:3, :3]).sum(1).max()
        self.sN = np.abs(self.inv[:3, :3].T).sum(1).max()

    def area(self, dtype=np.float64):
        return dtype(self.phimax) * dtype(self.radius) * (dtype(self.zmax) - dtype(self.zmin))

    def inside(self, ref_p):
        """(DistanceSquared(pOrigin, pCenter) <= radius^2 in float64, |d / r - 1|: the tests keep that above 1e-3)."""
        d = _len(np.asarray(ref_p, np.float64) - self.pc)
        return d <= self.radius, np.abs(d / self.radius - 1)

    def sample_area(self, u, dtype=np.float64):
        """Sphere::Sample(u) -> Out(p, n, band_p, band_n)."""
        u = np.asarray(u, dtype)
        r = dtype(self.radius)
        pobj = r * uniform_sample_sphere(u[:, 0], u[:, 1], dtype)
        nraw = _normal(self.inv, pobj, dtype)
        n = _normalize(nraw)
        if self.reverse:
            n = -n
        pobj = pobj * (r / _len(pobj))[:, None]
        p = _point(self.m, pobj, dtype)
        z = 1 - 2 * u[:, 0].astype(np.float64)
        rr = np.sqrt(np.maximum(0.0, 1 - z * z))
        with np.errstate(divide="ignore"):
            err = np.minimum(4 * U / np.maximum(rr, 1e-300), 2 * np.sqrt(U)) + U * rr
        eo = self.radius * (err + 30 * U) + 8 * U * self.radius
        band_p = self.sM * eo + 4 * U * (self.sM * self.radius + np.abs(self.pc).max())
        band_n = 2 * SQRT3 * self.sN * (eo + 4 * U * self.radius) / _len(nraw.astype(np.float64)) + 4 * U
        return Out(p=p, n=n, band_p=band_p, band_n=band_n)

    def sample(self, ref_p, u, dtype=np.float64):
        """Sphere::Sample(ref, u) -> Out(p, n, pdf, band_p, band_n, band_pdf_rel, inside)."""
        ref_p, u = np.asarray(ref_p, dtype), np.asarray(u, dtype)
        r, pc = dtype(self.radius), self.pc.astype(dtype)
        inside = _dot(ref_p - pc, ref_p - pc) <= r * r
        out = Out(p=np.zeros((len(u), 3), dtype), n=np.zeros((len(u), 3), dtype), pdf=np.zeros(len(u), dtype), band_p=np.zeros(len(u)),
                  band_n=np.zeros(len(u)), band_pdf_rel=np.zeros(len(u)), band_side=np.zeros(len(u)), inside=inside)
        if inside.any():
            k = inside
            a = self.sample_area(u[k], dtype)
            pdf, _, _, rel, _, ec = _solid_angle_pdf(ref_p[k], a.p, a.n, self.area(dtype), dtype, a.band_p, a.band_n, 4 * U)
            out.p[k], out.n[k], out.pdf[k], out.band_p[k], out.band_n[k], out.band_pdf_rel[k] = a.p, a.n, pdf, a.band_p, a.band_n, rel
            out.band_side[k] = ec
        if (~inside).any():
            k = ~inside
            p, u0, u1 = ref_p[k], u[k, 0], u[k, 1]
            wc = _normalize(pc - p)
            wcx, wcy = coordinate_system(wc)
            s2 = r * r / _dot(p - pc, p - pc)
            cm = np.sqrt(np.maximum(dtype(0), 1 - s2))
            ct = (1 - u0) + u0 * cm
            st = np.sqrt(np.maximum(dtype(0), 1 - ct * ct))
            phi = u1 * 2 * dtype(np.pi)
            dc = _len(p - pc)
            B = r * r - dc * dc * st * st
            ds = dc * ct - np.sqrt(np.maximum(dtype(0), B))
            ca = (dc * dc + r * r - ds * ds) / (2 * dc * r)
            sa = np.sqrt(np.maximum(dtype(0), 1 - ca * ca))
            # SphericalDirection(sinAlpha, cosAlpha, phi, -wcX, -wcY, -wc)
            n = (sa * np.cos(phi))[:, None] * -wcx + (sa * np.sin(phi))[:, None] * -wcy + ca[:, None] * -wc
            out.p[k] = pc + r * n
            out.n[k] = -n if self.reverse else n
            out.pdf[k] = 1 / (2 * dtype(np.pi) * (1 - cm))
            # the bands, from the float64 values
            f = lambda a: np.asarray(a, np.float64)
            s2, cm, ct, dc, B, ds, ca, sa, rr = f(s2), f(cm), f(ct), f(dc), np.maximum(f(B), 0), f(ds), f(ca), f(sa), self.radius
            with np.errstate(divide="ignore", invalid="ignore"):
                ecm = U * (4 * s2 / cm + 1.5 * cm)
                out.band_pdf_rel[k] = (ecm + U * (1 - cm)) / (1 - cm) + 5 * U
                ect = 3 * U + ecm
                eS = dc * dc * (2 * ct * ect + 2 * U + 14 * U * (1 - ct * ct))
                eB = U * rr * rr + eS + U * B
                esB = np.minimum(eB / np.sqrt(B), np.sqrt(eB)) + U * np.sqrt(B)
                eds = dc * (ect + 5 * U) + esB + U * np.abs(ds)
                eca = (11 * U * dc * dc + 3 * U * rr * rr + 2 * np.abs(ds) * eds + U * ds * ds) / (2 * dc * rr) + 7 * U * np.abs(ca)
                e1 = 2 * np.abs(ca) * eca + 2 * U
                esa = np.minimum(e1 / sa, np.sqrt(e1)) + U * sa
            out.band_n[k] = 1.5 * esa + eca + 100 * U
            out.band_p[k] = rr * out.band_n[k] + 2 * U * (np.abs(self.pc).max() + rr)
            w = f(out.p[k]) - f(p)
            d = _len(w)
            with np.errstate(divide="ignore", invalid="ignore"):
                eN = dc * (eca + 70 * U * sa + 5 * U) + rr * (2 * e1 + 2 * eca + 50 * U) + 2 * SQRT3 * U * (np.abs(self.pc).max() + rr) + 5 * U * d
                out.band_side[k] = eN / d
        return out

    def pdf(self, ref_p, wi, dtype=np.float64):
        """Sphere::Pdf(ref, wi) -> Out(pdf, band_pdf_rel, edge_flag)."""
        ref_p, wi = np.asarray(ref_p, dtype), np.asarray(wi, dtype)
        r, pc = dtype(self.radius), self.pc.astype(dtype)
        inside = _dot(ref_p - pc, ref_p - pc) <= r * r
        with np.errstate(divide="ignore", invalid="ignore"):
            s2 = r * r / _dot(ref_p - pc, ref_p - pc)
            cm = np.sqrt(np.maximum(dtype(0), 1 - s2))
            pdf = 1 / (2 * dtype(np.pi) * (1 - cm))  # UniformConePdf
            s2d, cmd = s2.astype(np.float64), cm.astype(np.float64)
            rel = (U * (4 * s2d / cmd + 1.5 * cmd) + U * (1 - cmd)) / (1 - cmd) + 5 * U
        flag = np.zeros(len(wi), bool)
        if inside.any():  # Shape::Pdf: Sphere::Intersect from ref.p, whose nearer root lies behind it
            k = inside
            o = _point(self.inv, ref_p[k], dtype)
            d = wi[k] @ self.inv.astype(dtype)[:3, :3].T
            a, b, c = _dot(d, d), 2 * _dot(d, o), _dot(o, o) - r * r
            t1 = (-b + np.sqrt(np.maximum(b * b - 4 * a * c, dtype(0)))) / (2 * a)
            ph = o + t1[:, None] * d
            ph = ph * (r / _len(ph))[:, None]
            phi = np.arctan2(ph[:, 1], ph[:, 0])
            phi = np.where(phi < 0, phi + 2 * dtype(np.pi), phi)
            full = self.zmin <= -self.radius and self.zmax >= self.radius
            hit = np.ones(len(t1), bool)
            if not full:
                hit &= (ph[:, 2] >= self.zmin) & (ph[:, 2] <= self.zmax)
            hit &= phi <= dtype(self.phimax)
            pw = _point(self.m, ph, dtype)
            n = _normalize(_normal(self.inv, ph, dtype))  # dpdu x dpdv of a sphere is along pHit; the reverse flip leaves |cos| alone
            w = pw - ref_p[k]
            d2 = _dot(w, w)
            cos = np.abs(_dot(n, -_normalize(wi[k])))
            p_in = d2 / (cos * self.area(dtype))
            p_in = np.where(hit & np.isfinite(p_in), p_in, dtype(0))
            R = max(np.abs(ref_p).max(), np.abs(self.pc).max() + self.radius)
            c64 = cos.astype(np.float64)
            ep = 40 * U * (R + self.radius) / c64
            dd = np.sqrt(d2.astype(np.float64))
            ec = SQRT3 * (ep / self.radius + 4 * U + 2 * SQRT3 * ep / dd + 4 * U) + 3 * U
            rel_in = 4 * U + 2 * SQRT3 * ep / dd + 9 * U + ec / np.maximum(c64 - ec, 1e-300)
            edge = 64 * U * (R + self.radius) / c64
            fl = np.zeros(len(t1), bool)
            if not full:
                fl |= (np.abs(ph[:, 2] - self.zmin) <= edge) | (np.abs(ph[:, 2] - self.zmax) <= edge)
            if self.phimax < 2 * np.pi - 1e-6:
                rho = np.maximum(np.hypot(ph[:, 0], ph[:, 1]).astype(np.float64), 1e-300)
                fl |= (np.abs(phi - self.phimax) <= edge / rho + 8 * U) | (phi <= edge / rho + 8 * U) | (phi >= 2 * np.pi - edge / rho - 8 * U)
            pdf[k], rel[k], flag[k] = p_in, np.where(hit, rel_in, 0.0), fl
        return Out(pdf=pdf, band_pdf_rel=rel, edge_flag=flag)

    def solid_angle(self, ref_p):
        """The cap a sphere subtends from outside, 2 Pi (1 - cosThetaMax), in closed form."""
        d = _len(np.asarray(ref_p, np.float64) - self.pc)
        return 2 * np.pi * (1 - np.sqrt(1 - (self.radius / d) ** 2))


class Triangle:
    def __init__(self, p0, p1, p2, normals=None, flip=False):
        """World-space vertices (and per-vertex normals, or None); flip = reverseOrientation ^ transformSwapsHandedness."""
        self.v = [_f32data(p) for p in (p0, p1, p2)]
        self.nrm = None if normals is None else [_f32data(n) for n in normals]
        self.flip = bool(flip)
        e1, e2 = self.v[1] - self.v[0], self.v[2] - self.v[0]
        self.sin_gamma = np.linalg.norm(np.cross(e1, e2)) / (np.linalg.norm(e1) * np.linalg.norm(e2))
        self.R = max(np.abs(p).max() for p in self.v)
        self.band_n = (10 / self.sin_gamma + 3) * U
        self.ea = (9 / self.sin_gamma + 3) * U

    def area(self, dtype=np.float64):
        p0, p1, p2 = [p.astype(dtype) for p in self.v]
        return dtype(0.5) * _len(np.cross(p1 - p0, p2 - p0))

    def _normal_at(self, b0, b1, dtype):
        p0, p1, p2 = [p.astype(dtype) for p in self.v]
        n = np.broadcast_to(_normalize(np.cross(p1 - p0, p2 - p0)), (len(b0), 3)).copy()
        if self.nrm is not None:
            n0, n1, n2 = [x.astype(dtype) for x in self.nrm]
            ns = b0[:, None] * n0 + b1[:, None] * n1 + (1 - b0 - b1)[:, None] * n2
            n = np.where((_dot(n, ns) < 0)[:, None], -n, n)  # Faceforward(n, ns), geometry.h
        elif self.flip:
            n = -n
        return n

    def sample_area(self, u, dtype=np.float64):
        u = np.asarray(u, dtype)
        b0, b1 = uniform_sample_triangle(u[:, 0], u[:, 1])
        p0, p1, p2 = [p.astype(dtype) for p in self.v]
        p = b0[:, None] * p0 + b1[:, None] * p1 + (1 - b0 - b1)[:, None] * p2
        return Out(p=p, n=self._normal_at(b0, b1, dtype), band_p=np.full(len(u), 16 * U * self.R), band_n=np.full(len(u), self.band_n))

    def sample(self, ref_p, u, dtype=np.float64):
        """Shape::Sample(ref, u) over Triangle::Sample(u)."""
        a = self.sample_area(u, dtype)
        pdf, _, _, rel, _, side = _solid_angle_pdf(np.asarray(ref_p, dtype), a.p, a.n, self.area(dtype), dtype, a.band_p, a.band_n, self.ea,
                                                   ep_off=5 * U * self.R)
        return Out(p=a.p, n=a.n, pdf=pdf, band_p=a.band_p, band_n=a.band_n, band_pdf_rel=rel, band_side=side)

    def _intersect(self, o, d, dtype):
        """Triangle::Intersect (triangle.cpp:231-378) for rays (o, d) without an end, in dtype -> (hit, b (n, 3), t): the vertices
        translated to the origin, permuted so that the ray's largest component is z, sheared; the edge functions (in double
        where one is exactly 0 in single, :277-289), the sign test, the determinant, tScaled against it, b_i = e_i / det.
        (The conservative t > deltaT rejection, :305-339, is not restated: a hit that close to the origin is flagged.)"""
        o, d = np.asarray(o, dtype), np.asarray(d, dtype)
        kz = np.abs(d).argmax(axis=1)
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        take = lambda a, k: np.take_along_axis(a, k[:, None], 1)[:, 0]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            dx, dy, dz = take(d, kx), take(d, ky), take(d, kz)
            sx, sy, sz = -dx / dz, -dy / dz, 1 / dz
            xs, ys, zs = [], [], []
            for p in self.v:
                P = p.astype(dtype)[None, :] - o
                px, py, pz = take(P, kx), take(P, ky), take(P, kz)
                xs.append(px + sx * pz), ys.append(py + sy * pz), zs.append(pz * sz)
            e = []
            for j, k in ((1, 2), (2, 0), (0, 1)):  # e0 = p1t.x p2t.y - p1t.y p2t.x, and cyclically
                e.append(xs[j] * ys[k] - ys[j] * xs[k])
            if dtype is np.float32:
                zero = (e[0] == 0) | (e[1] == 0) | (e[2] == 0)
                for i, (j, k) in enumerate(((1, 2), (2, 0), (0, 1))):
                    x64 = np.float64(xs[j]) * np.float64(ys[k]) - np.float64(ys[j]) * np.float64(xs[k])
                    e[i] = np.where(zero, x64.astype(np.float32), e[i])
            e = np.stack(e, 1)
            mixed = (e < 0).any(axis=1) & (e > 0).any(axis=1)
            det = e[:, 0] + e[:, 1] + e[:, 2]
            t_scaled = e[:, 0] * zs[0] + e[:, 1] * zs[1] + e[:, 2] * zs[2]
            behind = ((det < 0) & (t_scaled >= 0)) | ((det > 0) & (t_scaled <= 0))
            inv_det = 1 / det
            b = e * inv_det[:, None]
            t = t_scaled * inv_det
        hit = ~mixed & (det != 0) & ~behind & np.isfinite(t)
        return hit, b, t

    def _pdf_value(self, o, d, dtype):
        """Shape::Pdf(ref, wi) in dtype -> (pdf, hit, b, t, |cos| at the hit, distance squared)."""
        o, d = np.asarray(o, dtype), np.asarray(d, dtype)
        hit, b, t = self._intersect(o, d, dtype)
        p0, p1, p2 = [p.astype(dtype) for p in self.v]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ph = b[:, 0:1] * p0 + b[:, 1:2] * p1 + b[:, 2:3] * p2
            n = self._normal_at(b[:, 0], b[:, 1], dtype)
            w = o - ph
            d2 = _dot(w, w)
            cos = np.abs(_dot(n, -d))  # AbsDot(isectLight.n, -wi): wi as it is given
            pdf = d2 / (cos * self.area(dtype))
            pdf = np.where(hit & np.isfinite(pdf), pdf, dtype(0))
        assert pdf.dtype == dtype
        return pdf, hit, b, t, cos, d2

    def pdf(self, ref_p, wi, dtype=np.float64):
        """Shape::Pdf(ref, wi) over Triangle::Intersect -> Out(pdf, band_pdf_rel, edge_flag, hit): pdf evaluated in dtype; the
        band, the edge flag and hit belong to the float64 evaluation. wi: unit directions, as the integrators pass them."""
        o, d = np.asarray(ref_p, np.float64), np.asarray(wi, np.float64)
        pdf, hit, bs, t, cos, d2 = self._pdf_value(o, d, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            dl = _len(d)
            D = 2 * np.max([np.abs(p[None, :] - o).max(axis=1) for p in self.v], axis=0)
            eb = self._barycentric_band(o, d)
            flag = (np.abs(bs) <= eb).any(axis=1) | (np.abs(t * dl) <= 64 * U * D) | ~np.isfinite(eb).all(axis=1)
            ep = 22 * U * self.R
            dd = np.sqrt(d2)
            rc = (SQRT3 * (self.band_n + 6 * U) + 3 * U) / cos  # wi is given: it carries no rounding of its own
            rel = np.where(rc < 1, self.ea + 2 * SQRT3 * ep / dd + 9 * U + rc / np.maximum(1 - rc, 1e-300), np.inf)
        if dtype is not np.float64:
            pdf = self._pdf_value(ref_p, wi, dtype)[0]
        return Out(pdf=pdf, band_pdf_rel=np.where(hit, rel, 0.0), edge_flag=flag & (cos > 0), hit=hit)

    def _barycentric_band(self, o, d):
        """The band of each barycentric coordinate of Triangle::Intersect's hit, (n, 3), per ray: see the module's docstring."""
        kz = np.abs(d).argmax(axis=1)
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        take = lambda a, k: np.take_along_axis(a, k[:, None], 1)[:, 0]
        dx, dy, dz = take(d, kx), take(d, ky), take(d, kz)
        sx, sy = -dx / dz, -dy / dz
        xs, ys, ex, ey = [], [], [], []
        for p in self.v:
            P = p[None, :] - o
            px, py, pz = take(P, kx), take(P, ky), take(P, kz)
            x, y = px + sx * pz, py + sy * pz
            xs.append(x), ys.append(y)
            ex.append(U * (np.abs(px) + 3 * np.abs(sx * pz) + np.abs(x)))
            ey.append(U * (np.abs(py) + 3 * np.abs(sy * pz) + np.abs(y)))
        e, de = [], []
        for j, k in ((1, 2), (2, 0), (0, 1)):  # e0 = p1.x p2.y - p1.y p2.x, and cyclically
            e.append(xs[j] * ys[k] - ys[j] * xs[k])
            de.append(np.abs(ys[k]) * ex[j] + np.abs(xs[j]) * ey[k] + np.abs(xs[k]) * ey[j] + np.abs(ys[j]) * ex[k] +
                      2 * U * (np.abs(xs[j] * ys[k]) + np.abs(ys[j] * xs[k])) + U * np.abs(e[-1]))
        e, de = np.stack(e, 1), np.stack(de, 1)
        det = e.sum(axis=1, keepdims=True)
        return (de + np.abs(e / det) * de.sum(axis=1, keepdims=True)) / np.abs(det) + 2 * U

    def solid_angle(self, ref_p):
        """Van Oosterom and Strackee: tan(Omega / 2) = a . (b x c) / (|a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|)."""
        o = np.asarray(ref_p, np.float64)
        a, b, c = [p[None, :] - o for p in self.v]
        la, lb, lc = _len(a), _len(b), _len(c)
        num = _dot(a, np.cross(b, c))
        den = la * lb * lc + _dot(a, b) * lc + _dot(a, c) * lb + _dot(b, c) * la
        return np.abs(2 * np.arctan2(num, den))


class Quadric:
    """A disk or a cylinder: quadric_ref's shape for Intersect, and Area / Sample(u) here."""

    def __init__(self, shape, o2w, o2w_inv, reverse=False):
        self.shape, self.kind = shape, ("disk" if isinstance(shape, Q.Disk) else "cylinder")
        self.m, self.inv = _f32data(o2w).reshape(4, 4), _f32data(o2w_inv).reshape(4, 4)
        self.reverse = bool(reverse)
        self.sM = np.abs(self.m[:3, :3]).sum(1).max()
        self.sN = np.abs(self.inv[:3, :3].T).sum(1).max()
        s = shape
        self.size = s.radius + (abs(s.height) if self.kind == "disk" else max(abs(s.zmin), abs(s.zmax)))

    def area(self, dtype=np.float64):
        s = self.shape
        if self.kind == "disk":  # phiMax * 0.5 * (radius^2 - innerRadius^2), the 0.5 a double
            return dtype(np.float64(dtype(np.float32(s.phimax))) * 0.5 * np.float64(dtype(s.radius) * dtype(s.radius) - dtype(s.inner) * dtype(s.inner)))
        return (dtype(s.zmax) - dtype(s.zmin)) * dtype(s.radius) * dtype(np.float32(s.phimax))

    def sample_area(self, u, dtype=np.float64):
        u, s = np.asarray(u, dtype), self.shape
        if self.kind == "disk":
            pd = concentric_sample_disk(u[:, 0], u[:, 1], dtype)
            pobj = np.stack([pd[:, 0] * dtype(s.radius), pd[:, 1] * dtype(s.radius), np.full(len(u), dtype(s.height))], -1)
            nobj = np.broadcast_to(np.array([0, 0, 1], dtype), pobj.shape)
            en_obj = 0.0
        else:
            z = (1 - u[:, 0]) * dtype(s.zmin) + u[:, 0] * dtype(s.zmax)  # Lerp, pbrt.h
            phi = u[:, 1] * dtype(np.float32(s.phimax))
            pobj = np.stack([dtype(s.radius) * np.cos(phi), dtype(s.radius) * np.sin(phi), z], -1)
            nobj = pobj * np.array([1, 1, 0], dtype)
            hit_rad = np.sqrt(pobj[:, 0] * pobj[:, 0] + pobj[:, 1] * pobj[:, 1])
            pobj = pobj * np.stack([dtype(s.radius) / hit_rad, dtype(s.radius) / hit_rad, np.ones_like(hit_rad)], -1)
            en_obj = 24 * U * s.radius
        nraw = _normal(self.inv, nobj, dtype)
        n = _normalize(nraw)
        if self.reverse:
            n = -n
        p = _point(self.m, pobj, dtype)
        band_p = self.sM * 14 * U * self.size + 4 * U * (self.sM * self.size + np.abs(self.m[:3, 3]).max())
        band_n = 2 * SQRT3 * self.sN * en_obj / _len(nraw.astype(np.float64)) + 12 * U
        return Out(p=p, n=n, band_p=np.full(len(u), band_p), band_n=band_n * np.ones(len(u)))

    def sample(self, ref_p, u, dtype=np.float64):
        a = self.sample_area(u, dtype)
        off = 4 * U * (self.sM * self.size + np.abs(self.m[:3, 3]).max()) if self.kind == "disk" else None  # a disk is flat
        pdf, _, _, rel, _, side = _solid_angle_pdf(np.asarray(ref_p, dtype), a.p, a.n, self.area(dtype), dtype, a.band_p, a.band_n, 5 * U, ep_off=off)
        return Out(p=a.p, n=a.n, pdf=pdf, band_p=a.band_p, band_n=a.band_n, band_pdf_rel=rel, band_side=side)

    def _pdf_value(self, o, d, dtype):
        """Shape::Pdf(ref, wi) in dtype -> (pdf, hit, |cos| at the hit, distance squared): quadric_ref's Intersect on dtype arrays
        (its shape parameters are plain numbers, so every operation stays in dtype), the hit through ObjectToWorld, the normal
        through the inverse's transpose, then shape.cpp:83-85."""
        o, d = np.asarray(o, dtype), np.asarray(d, dtype)
        shape = type(self.shape).__new__(type(self.shape))
        shape.__dict__.update({k: (float(v) if np.isscalar(v) else v) for k, v in self.shape.__dict__.items()})
        shape.m, shape.inv = self.m.astype(dtype), self.inv.astype(dtype)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t, pobj, _ = shape.intersect(o, d, np.inf)
            hit = np.isfinite(t)
            nobj = pobj * np.array([1, 1, 0], dtype) if self.kind == "cylinder" else np.broadcast_to(np.array([0, 0, 1], dtype), pobj.shape)
            n = _normalize(_normal(self.inv, nobj, dtype))
            pw = _point(self.m, pobj, dtype)
            w = pw - o
            d2 = _dot(w, w)
            cos = np.abs(_dot(n, -d))
            pdf = d2 / (cos * self.area(dtype))
            pdf = np.where(hit & np.isfinite(pdf), pdf, dtype(0))
        assert pdf.dtype == dtype and pobj.dtype == dtype and t.dtype == dtype
        return pdf, hit, cos, d2

    def pdf(self, ref_p, wi, dtype=np.float64):
        """Shape::Pdf(ref, wi) -> Out(pdf, band_pdf_rel, edge_flag, hit): pdf evaluated in dtype; the band, the edge flag and hit
        belong to the float64 evaluation. wi: unit directions."""
        o, d = np.asarray(ref_p, np.float64), np.asarray(wi, np.float64)
        pdf, hit, cos, d2 = self._pdf_value(o, d, np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            R = max(np.abs(o).max(), np.abs(self.m[:3, 3]).max() + self.sM * self.size)
            ep = 40 * U * (R + self.sM * self.size) / cos
            dd = np.sqrt(d2)
            en = 12 * U + (ep / (self.sM * self.shape.radius) if self.kind == "cylinder" else 0.0)
            rc = (SQRT3 * (en + 6 * U) + 3 * U) / cos
            rel = np.where(rc < 1, 5 * U + 2 * SQRT3 * ep / dd + 9 * U + rc / np.maximum(1 - rc, 1e-300), np.inf)
        if dtype is not np.float64:
            pdf = self._pdf_value(ref_p, wi, dtype)[0]
        return Out(pdf=pdf, band_pdf_rel=np.where(hit, rel, 0.0), edge_flag=self._edge_flag(o, d, 40 * U * (R + self.sM * self.size) * self.sN), hit=hit)

    def _edge_flag(self, o, d, e0):
        """Whether a float32 evaluation may decide hit-or-miss otherwise: a candidate hit (the plane's, or either root of the
        cylinder's quadratic ahead of the origin) within e0 / |cos| (object units) of an edge of the partial shape: radius, inner
        radius, zmin, zmax, phimax and phi = 0; or a ray that grazes the cylinder."""
        s = self.shape
        oo, dd = o @ self.inv[:3, :3].T + self.inv[:3, 3], d @ self.inv[:3, :3].T
        ln = _len(dd)
        partial = s.phimax < 2 * np.pi - 1e-6

        def near(p, e, edges_z):
            r = np.hypot(p[:, 0], p[:, 1])
            phi = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2 * np.pi)
            f = np.zeros(len(p), bool)
            for z in edges_z:
                f |= np.abs(p[:, 2] - z) <= e
            if partial:
                ea = e / np.maximum(r, 1e-300) + 8 * U
                f |= (np.abs(phi - s.phimax) <= ea) | (phi <= ea) | (phi >= 2 * np.pi - ea)
            return f, r

        with np.errstate(divide="ignore", invalid="ignore"):
            if self.kind == "disk":
                t = (s.height - oo[:, 2]) / dd[:, 2]
                p = oo + dd * t[:, None]
                e = e0 / (np.abs(dd[:, 2]) / ln)
                f, r = near(p, e, ())
                f |= (np.abs(r - s.radius) <= e) | ((s.inner > 0) & (np.abs(r - s.inner) <= e)) | (np.abs(t) * ln <= e)
                return np.where(np.isfinite(t) & (t > -e / ln), f, False) | ~np.isfinite(e)
            a = dd[:, 0] ** 2 + dd[:, 1] ** 2
            b = 2 * (dd[:, 0] * oo[:, 0] + dd[:, 1] * oo[:, 1])
            c = oo[:, 0] ** 2 + oo[:, 1] ** 2 - s.radius ** 2
            disc = b * b - 4 * a * c
            flag = np.abs(disc) <= 64 * U * (b * b + np.abs(4 * a * c))
            sq = np.sqrt(np.maximum(disc, 0))
            for t in ((-b - sq) / (2 * a), (-b + sq) / (2 * a)):
                p = oo + dd * t[:, None]
                cos = np.abs(dd[:, 0] * p[:, 0] + dd[:, 1] * p[:, 1]) / (ln * s.radius)
                e = e0 / cos
                f, _ = near(p, e, (s.zmin, s.zmax))
                flag |= (disc > 0) & (t > -e / ln) & (f | (np.abs(t) * ln <= e) | ~np.isfinite(e))
            return flag


# ---- DiffuseAreaLight -----------------------------------------------------------------------------------------------------------
class AreaLight:
    def __init__(self, shape, L, two_sided=False):
        self.shape, self.L, self.two_sided = shape, _f32data(L), bool(two_sided)

    def sample_li(self, ref_p, u, dtype=np.float64):
        """DiffuseAreaLight::Sample_Li -> Out(wi, Li, pdf, p, n, band_wi, band_pdf_rel, band_p, band_n, side_flag)."""
        ref_p = np.asarray(ref_p, dtype)
        s = self.shape.sample(ref_p, u, dtype)
        w = s.p - ref_p
        d2 = _dot(w, w)
        dead = (s.pdf == 0) | (d2 == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            wi = np.where(dead[:, None], dtype(0), w / np.sqrt(d2)[:, None])
            d = np.sqrt(d2.astype(np.float64))
            band_wi = np.where(d > 0, 2 * SQRT3 * s.band_p / d + 4 * U, 0.0)
        c = _dot(s.n, -wi)
        emits = self.two_sided | (c > 0)  # DiffuseAreaLight::L
        Li = np.where((emits & ~dead)[:, None], self.L.astype(dtype), dtype(0))
        side_flag = np.zeros(len(c), bool) if self.two_sided else (np.abs(c.astype(np.float64)) <= s.band_side) & ~dead
        return Out(wi=wi, Li=Li, pdf=np.where(dead, dtype(0), s.pdf), p=s.p, n=s.n, band_wi=band_wi, band_pdf_rel=s.band_pdf_rel,
                   band_p=s.band_p, band_n=s.band_n, side_flag=side_flag, cos=c, unconditioned=~np.isfinite(s.band_pdf_rel) & ~dead)

    def pdf_li(self, ref_p, wi, dtype=np.float64):
        return self.shape.pdf(ref_p, wi, dtype)


# ---- Distribution1D / Distribution2D ----------------------------------------------------------------------------------------------
def distribution1d(func, dtype=np.float64):
    """Distribution1D's constructor -> (func, cdf[n + 1], funcInt)."""
    func = np.asarray(func, dtype)
    n = len(func)
    cdf = np.zeros(n + 1, dtype)
    for i in range(1, n + 1):
        cdf[i] = cdf[i - 1] + func[i - 1] / dtype(n)
    func_int = cdf[n]
    if func_int == 0:
        cdf = np.arange(n + 1, dtype=dtype) / dtype(n)
    else:
        cdf = np.concatenate([[dtype(0)], cdf[1:] / func_int]).astype(dtype)
    return func, cdf, func_int


def sample_continuous(func, cdf, func_int, u, dtype=np.float64):
    """Distribution1D::SampleContinuous over FindInterval(cdf[i] <= u) -> (x, pdf, offset); the table is data, u float32 values."""
    n = len(func)
    u = np.asarray(u, np.float64)
    cdf64 = np.asarray(cdf, np.float64)
    off = np.clip(np.searchsorted(cdf64, u, side="right") - 1, 0, n - 1)
    c, f = np.asarray(cdf, dtype), np.asarray(func, dtype)
    du = u.astype(dtype) - c[off]
    w = c[off + 1] - c[off]
    du = np.where(w > 0, du / np.where(w > 0, w, 1), du)
    pdf = f[off] / dtype(func_int) if func_int > 0 else np.zeros(len(u), dtype)
    return (off.astype(dtype) + du) / dtype(n), pdf, off


class Table:
    """A Distribution2D as the host lays it out: h rows of {func[w], cdf[w + 1], funcInt}, then the marginal {func[h], cdf[h + 1],
    funcInt}: (2 w + 2) h + 2 h + 2 floats."""

    def __init__(self, flat, w, h):
        flat = np.asarray(flat)
        assert flat.shape == ((2 * w + 2) * h + 2 * h + 2,)
        self.w, self.h, self.flat = w, h, flat
        rows = flat[:(2 * w + 2) * h].reshape(h, 2 * w + 2)
        self.func, self.cdf, self.func_int = rows[:, :w], rows[:, w:2 * w + 1], rows[:, 2 * w + 1]
        m = flat[(2 * w + 2) * h:]
        self.mfunc, self.mcdf, self.mfunc_int = m[:h], m[h:2 * h + 1], m[2 * h + 1]

    @staticmethod
    def build(img, dtype=np.float64):
        """Distribution2D(img, nu, nv) (sampling.cpp:159-174) in the host's layout."""
        img = np.asarray(img, dtype)
        h, w = img.shape
        rows = [distribution1d(img[v], dtype) for v in range(h)]
        marg = distribution1d(np.array([r[2] for r in rows], dtype), dtype)
        flat = np.concatenate([np.concatenate([f, c, [fi]]) for f, c, fi in rows + [marg]]).astype(dtype)
        return Table(flat, w, h)


def scalar_image(mip, dtype=np.float64):
    """infinite.cpp:64-80: (2 h, 2 w) filtered luminance x sin theta of the level-0 size, fwidth = 0.5 / min(width, height)."""
    h0, w0, _ = mip.levels[0].shape
    w, h = 2 * w0, 2 * h0
    fwidth = 0.5 / min(w, h)
    v, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    st = np.stack([(uu + 0.5) / w, (v + 0.5) / h], -1)
    y = lum(mip.lookup(st.reshape(-1, 2), fwidth)).reshape(h, w)
    return (y * np.sin(np.pi * (v + 0.5) / h)).astype(dtype)


def table_bands(mip, img):
    """The absolute bands of a float32 table against Table.build(scalar_image(mip)): Out(func, cdf, func_int) for the rows
    ((h, w), (h, w + 1), (h,)) and mfunc, mcdf, mfunc_int for the marginal.
    A func entry: Lookup(st, fwidth) blends triangle() of two levels (each ten roundings at the level's largest texel T, (s, t)
    exact to 2 u of a texel coordinate <= the level's size, over texel differences <= T: 2 u size T), the level and its
    fraction from Log2 (6 u of the level number n: delta moves by 6 u n, the blend by that times T), the luminance five
    roundings, sin theta 4 u, the product one: e_f = u T (30 + 4 size_max + 6 n) + 6 u f. A running sum of n terms f_i / n carries
    (n + 2) u relative: cdf_k (before the division) moves by sum_{i<k} e_i / n + (n + 2) u c_k; funcInt is the last of them; the
    normalised cdf_k = c_k / funcInt by (e(c_k) + c_k e(funcInt) / funcInt) / funcInt + u. The marginal's func are the rows'
    funcInt, and so on once more."""
    T = max(float(lv.max()) for lv in mip.levels)
    n_lv = len(mip.levels)
    size = max(mip.levels[0].shape[:2])
    img = np.asarray(img, np.float64)
    e_f = U * T * (30 + 4 * size + 6 * n_lv) + 6 * U * img

    def one(func, e):
        n = func.shape[-1]
        c = np.concatenate([np.zeros(func.shape[:-1] + (1,)), np.cumsum(func / n, -1)], -1)
        ec = np.concatenate([np.zeros(func.shape[:-1] + (1,)), np.cumsum(e / n, -1)], -1) + (n + 2) * U * c
        fi, efi = c[..., -1], ec[..., -1]
        with np.errstate(divide="ignore", invalid="ignore"):
            en = np.where(fi[..., None] > 0, (ec + c * (efi / fi)[..., None]) / fi[..., None] + U, U)
        return en, efi

    e_cdf, e_fi = one(img, e_f)
    rows_fi = np.concatenate([[0.0], np.cumsum(img / img.shape[1], -1)[:, -1]])[1:]
    e_mcdf, e_mfi = one(rows_fi, e_fi)
    return Out(func=e_f, cdf=e_cdf, func_int=e_fi, mfunc=e_fi, mcdf=e_mcdf, mfunc_int=e_mfi)


# ---- InfiniteAreaLight ------------------------------------------------------------------------------------------------------------
class InfiniteLight:
    def __init__(self, image, L, l2w, w2l, table=None, world_radius=1.0):
        """image: (h, w, 3) as ReadImage returns it (row 0 the top scanline), or None (one texel); L multiplies it in float32
        (infinite.cpp:54-60). l2w, w2l: the light's 3 x 3 as the scene holds them. table: the host's Table (data), or None to
        build the truth's own."""
        L = np.asarray(L, np.float32)
        texels = L[None, None, :] if image is None else np.asarray(image, np.float32) * L[None, None, :]
        self.mip = MipMap(texels.astype(np.float64))
        self.l2w, self.w2l = _f32data(l2w).reshape(3, 3), _f32data(w2l).reshape(3, 3)
        self.img = scalar_image(self.mip)
        self.own = Table.build(self.img)
        self.table = self.own if table is None else table
        self.world_radius = float(np.float32(world_radius))
        lv = self.mip.levels[0]
        self.h0, self.w0 = lv.shape[:2]
        self.T = float(lv.max())
        self.G = float(max(np.abs(lv - np.roll(lv, 1, 0)).max(), np.abs(lv - np.roll(lv, 1, 1)).max(),
                           np.abs(lv - np.roll(np.roll(lv, 1, 0), 1, 1)).max(), np.abs(lv - np.roll(np.roll(lv, 1, 0), -1, 1)).max()))
        self.range = float(lv.max() - lv.min())

    def _lookup(self, st, dtype):
        """Lmap->Lookup(st): MIPMap::triangle on level 0 under repeat wrap (mipmap.h:263-274). float64: mipmap_ref's; any other
        dtype: the same four-texel blend written out here in that dtype, on the level's texels rounded to it."""
        if dtype is np.float64:
            return self.mip.lookup(np.asarray(st, np.float64))
        lv = self.mip.levels[0].astype(dtype)
        h, w, _ = lv.shape
        st = np.asarray(st, dtype)
        s, t = st[:, 0] * dtype(w) - dtype(0.5), st[:, 1] * dtype(h) - dtype(0.5)
        s0, t0 = np.floor(s).astype(int), np.floor(t).astype(int)
        ds, dt = (s - s0.astype(dtype))[:, None], (t - t0.astype(dtype))[:, None]
        tex = lambda a, b: lv[b % h, a % w]
        out = ((1 - ds) * (1 - dt) * tex(s0, t0) + (1 - ds) * dt * tex(s0, t0 + 1) + ds * (1 - dt) * tex(s0 + 1, t0) + ds * dt * tex(s0 + 1, t0 + 1))
        assert out.dtype == dtype
        return out

    def sample_li(self, ref_p, u, dtype=np.float64):
        """-> Out(wi, Li, pdf, target, row, col, band_wi, band_pdf_rel, band_L)."""
        t, u = self.table, np.asarray(u, np.float32)
        d1, pdf1, v = sample_continuous(t.mfunc, t.mcdf, t.mfunc_int, u[:, 1], dtype)
        d0, pdf0, col = np.zeros(len(u), dtype), np.zeros(len(u), dtype), np.zeros(len(u), int)
        for row in np.unique(v):
            k = v == row
            d0[k], pdf0[k], col[k] = sample_continuous(t.func[row], t.cdf[row], t.func_int[row], u[k, 0], dtype)
        map_pdf = pdf0 * pdf1
        theta, phi = d1 * dtype(np.pi), d0 * 2 * dtype(np.pi)
        st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
        wl = np.stack([st * cp, st * sp, ct], -1)
        wi = wl @ self.l2w.astype(dtype).T
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            pdf = map_pdf / (2 * dtype(np.pi) * dtype(np.pi) * st)
            pdf = np.where(st == 0, dtype(0), pdf)
            Li = self._lookup(np.stack([d0, d1], -1), dtype)
            dead = map_pdf == 0
            st64 = np.abs(st.astype(np.float64))
            rel = (9 + 24 / st64) * U
        band_L = self.G * (7 * U * self.w0 + 7 * U * self.h0) + 10 * U * self.T
        target = np.asarray(ref_p, dtype) + wi * (2 * dtype(self.world_radius))
        z = dtype(0)
        return Out(wi=np.where(dead[:, None], z, wi), Li=np.where(dead[:, None], z, Li), pdf=np.where(dead, z, pdf),
                   target=np.where(dead[:, None], z, target), row=v, col=col, band_wi=np.full(len(u), 136 * U),
                   band_pdf_rel=np.where(dead | (st == 0), 0.0, rel), band_L=np.full(len(u), band_L), dead=dead,
                   band_target=2 * self.world_radius * 136 * U + 4 * U * (np.abs(np.asarray(ref_p, np.float64)).max(axis=1) + 2 * self.world_radius))

    def _angles(self, wl, e):
        z = np.clip(wl[:, 2], -1, 1)
        theta = np.arccos(z)
        phi = np.arctan2(wl[:, 1], wl[:, 0])
        phi = np.where(phi < 0, phi + 2 * wl.dtype.type(np.pi), phi)
        with np.errstate(divide="ignore"):
            sin_t = np.sqrt(np.maximum(0.0, 1 - z.astype(np.float64) ** 2))
            eth = e / sin_t + 4 * U
            eph = np.sqrt(2.0) * e / sin_t + 8 * U
        return theta, phi, eth, eph

    def le(self, d, dtype=np.float64):
        """InfiniteAreaLight::Le for ray directions d -> Out(L, band_L)."""
        d = np.asarray(d, dtype)
        wl = _normalize(d @ self.w2l.astype(dtype).T)
        theta, phi, eth, eph = self._angles(wl, 8 * U)
        st = np.stack([phi * dtype(1 / (2 * np.pi)), theta * dtype(1 / np.pi)], -1)
        L = self._lookup(st, dtype)
        full = self.range + 10 * U * self.T
        ds = np.minimum(self.w0 * (eph / (2 * np.pi) + 2 * U) + self.h0 * (eth / np.pi + 2 * U) + U * (self.w0 + self.h0), 1e30)
        return Out(L=L, band_L=np.minimum(self.G * ds + 10 * U * self.T, full))

    def pdf_li(self, w, dtype=np.float64):
        """InfiniteAreaLight::Pdf_Li over Distribution2D::Pdf -> Out(pdf, band_pdf_rel, cell_flag)."""
        w = np.asarray(w, dtype)
        wl = w @ self.w2l.astype(dtype).T
        ln = _len(w.astype(np.float64))
        theta, phi, eth, eph = self._angles(wl, 6 * U * ln)  # (SphericalTheta of the vector as it is: callers pass unit directions)
        t = self.table
        # sin(acos(z)): 0 at both poles (z = +-1 after the clamp), where :129 returns 0
        sin_t = np.where(np.abs(np.clip(wl[:, 2], -1, 1)) == 1, dtype(0), np.sin(theta))
        p0, p1 = phi * dtype(1 / (2 * np.pi)), theta * dtype(1 / np.pi)
        x0, x1 = (p0 * dtype(t.w)).astype(np.float64), (p1 * dtype(t.h)).astype(np.float64)
        iu, iv = np.clip(np.trunc(x0).astype(int), 0, t.w - 1), np.clip(np.trunc(x1).astype(int), 0, t.h - 1)
        func = np.asarray(t.func, dtype)[iv, iu]
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf = (func / dtype(t.mfunc_int)) / (2 * dtype(np.pi) * dtype(np.pi) * sin_t)
            # an all-black map: the reference's Distribution2D::Pdf is 0 / 0 there; Sample_Li returns no direction at all
            # (mapPdf == 0), and the density of what is never sampled is 0
            pdf = np.where((sin_t == 0) | (t.mfunc_int == 0), dtype(0), pdf)
            e0, e1 = t.w * (eph / (2 * np.pi) + 3 * U), t.h * (eth / np.pi + 3 * U)
            f64 = np.asarray(t.func, np.float64)

            def differs(x, e, n, axis):
                lo, hi = np.clip(np.floor(x - e).astype(int), 0, n - 1), np.clip(np.floor(x + e).astype(int), 0, n - 1)
                a = f64[iv, lo] if axis == 0 else f64[lo, iu]
                b = f64[iv, hi] if axis == 0 else f64[hi, iu]
                wrap = (axis == 0) & ((x - e < 0) | (x + e >= n))  # the seam: phi on either side of 0
                return (lo != hi) | wrap
            e0c, e1c = np.minimum(e0, t.w), np.minimum(e1, t.h)
            flag = differs(x0, e0c, t.w, 0) | differs(x1, e1c, t.h, 1)
            rel = (eth + 2 * U) / np.abs(sin_t.astype(np.float64)) + 8 * U
            # what a flagged direction may give: the pdf with either neighbouring column (modulo w: the seam) and either row
            cols = [np.mod(np.floor(x0 - e0c).astype(int), t.w), np.mod(np.floor(x0 + e0c).astype(int), t.w)]
            rows = [np.clip(np.floor(x1 - e1c).astype(int), 0, t.h - 1), np.clip(np.floor(x1 + e1c).astype(int), 0, t.h - 1)]
            scale = np.where((sin_t == 0) | (t.mfunc_int == 0), 0.0, 1 / (np.float64(t.mfunc_int) * 2 * np.pi * np.pi * sin_t.astype(np.float64)))
            alt = np.stack([f64[r, c] * scale for r in rows for c in cols], 1)
        return Out(pdf=pdf, band_pdf_rel=np.where(sin_t == 0, 0.0, rel), cell_flag=flag & (sin_t != 0), pdf_alt=alt)
