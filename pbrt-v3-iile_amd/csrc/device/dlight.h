// dlight.h — light sampling: sphere, quadric and triangle emitters (Shape::Sample / Pdf), the infinite light over its
// environment map, shape_sample / shape_pdf, the power heuristic, and the delta lights (point, spot, distant, projection,
// goniometric). Part of dpath.h, which includes it ahead of estimate_direct_request, the step that joins lights and BSDF.
// (Included inside dpath.h's namespace iile, as dtrav.h is, and uses what dpath.h holds above it: the scene tables of dscene.h, Isect,
//  the sphere / quadric / triangle tests and interactions, offset_ray_origin.)
#pragma once
#include "dtex.h"  // the infinite light's and the projection / goniometric lights' maps are image textures
// ===========================================================================
// sphere emitter (shapes/sphere.cpp:219-306, core/shape.cpp:72-87)
// ===========================================================================
struct LightSample {
    F3 p, perr, n;
};
DEV float sphere_area(const DSphere &sp) { return sp.phi_max * sp.radius * (sp.zmax - sp.zmin); }
DEV LightSample sphere_sample_area(const DSphere &sp, float u0, float u1, float *pdf) {
    float z = 1 - 2 * u0;  // UniformSampleSphere, sampling.cpp:98-103
    float r = sqrtf(mx(0.f, 1.f - z * z));
    float phi = 2 * kPi * u1;
    float s, c;
    sincos_f(phi, &s, &c);
    F3 us = F3{r * c, r * s, z};
    F3 pobj = F3{0, 0, 0} + sp.radius * us;
    LightSample it;
    it.n = normalize(xf_normal(sp.o2w_inv, pobj));
    if (sp.reverse_orientation) it.n = it.n * -1.f;
    float scale = sp.radius / length(pobj);
    pobj = F3{pobj.x * scale, pobj.y * scale, pobj.z * scale};
    F3 pobj_err = kGamma5 * vabs(pobj);
    it.p = xf_point_err2(sp.o2w, pobj, pobj_err, &it.perr);
    *pdf = 1 / sphere_area(sp);
    return it;
}
DEV LightSample sphere_sample(const DSphere &sp, const Isect &ref, float u0, float u1, float *pdf) {
    const F3 pc = F3{sp.center[0], sp.center[1], sp.center[2]};  // (*ObjectToWorld)(Point3f(0, 0, 0)), see DSphere
    F3 porigin = offset_ray_origin(ref.p, ref.perr, ref.n, pc - ref.p);
    if (length_sq(porigin - pc) <= sp.radius * sp.radius) {
        LightSample intr = sphere_sample_area(sp, u0, u1, pdf);
        F3 wi = intr.p - ref.p;
        if (length_sq(wi) == 0)
            *pdf = 0;
        else {
            wi = normalize(wi);
            *pdf *= length_sq(ref.p - intr.p) / absdot(intr.n, -wi);
        }
        if (is_inf(*pdf)) *pdf = 0.f;
        return intr;
    }
    F3 wc = normalize(pc - ref.p);
    F3 wcx, wcy;
    coordinate_system(wc, &wcx, &wcy);
    float sin_tmax2 = sp.radius * sp.radius / length_sq(ref.p - pc);
    float cos_tmax = sqrtf(mx(0.f, 1 - sin_tmax2));
    float cos_t = (1 - u0) + u0 * cos_tmax;
    float sin_t = sqrtf(mx(0.f, 1 - cos_t * cos_t));
    float phi = u1 * 2 * kPi;
    float dc = length(ref.p - pc);
    float ds = dc * cos_t - sqrtf(mx(0.f, sp.radius * sp.radius - dc * dc * sin_t * sin_t));
    float cos_a = (dc * dc + sp.radius * sp.radius - ds * ds) / (2 * dc * sp.radius);
    float sin_a = sqrtf(mx(0.f, 1 - cos_a * cos_a));
    float sphi, cphi;
    sincos_f(phi, &sphi, &cphi);
    // SphericalDirection(sinAlpha, cosAlpha, phi, -wcX, -wcY, -wc), geometry.h:1467-1472
    F3 nw = sin_a * cphi * (-wcx) + sin_a * sphi * (-wcy) + cos_a * (-wc);
    F3 pw = pc + sp.radius * nw;
    LightSample it;
    it.p = pw;
    it.perr = kGamma5 * vabs(pw);
    it.n = nw;
    if (sp.reverse_orientation) it.n = it.n * -1.f;
    *pdf = 1 / (2 * kPi * (1 - cos_tmax));
    return it;
}
DEV float sphere_pdf(const DSphere &sp, const Isect &ref, F3 wi) {
    const F3 pc = F3{sp.center[0], sp.center[1], sp.center[2]};  // (*ObjectToWorld)(Point3f(0, 0, 0)), see DSphere
    F3 porigin = offset_ray_origin(ref.p, ref.perr, ref.n, pc - ref.p);
    if (length_sq(porigin - pc) <= sp.radius * sp.radius) {
        // Shape::Pdf, shape.cpp:72-87 — the shape alone, not a scene ray
        F3 ro = offset_ray_origin(ref.p, ref.perr, ref.n, wi);
        float t;
        F3 od, ph;
        if (!sphere_test(sp, ro, wi, IILE_INF, &t, &od, &ph)) return 0;
        Isect li;
        sphere_interaction(sp, od, ph, &li);
        float pdf = length_sq(ref.p - li.p) / (absdot(li.n, -wi) * sphere_area(sp));
        if (is_inf(pdf)) pdf = 0.f;
        return pdf;
    }
    float sin_tmax2 = sp.radius * sp.radius / length_sq(ref.p - pc);
    float cos_tmax = sqrtf(mx(0.f, 1 - sin_tmax2));
    return 1 / (2 * kPi * (1 - cos_tmax));
}
// disk and cylinder emitters: Area, Sample(u) (disk.cpp:125-138, cylinder.cpp:204-221) and the solid-angle Shape::Sample(ref, u) /
// Shape::Pdf(ref, wi) (core/shape.cpp:56-87)
DEV float quadric_area(const DQuadric &q) {
    if (q.kind == kQuadricDisk) return float(double(q.phi_max) * 0.5 * double(q.radius * q.radius - q.inner_radius * q.inner_radius));
    return (q.zmax - q.zmin) * q.radius * q.phi_max;
}
DEV LightSample quadric_sample_area(const DQuadric &q, float u0, float u1, float *pdf) {
    LightSample it;
    if (q.kind == kQuadricDisk) {
        // Disk::Sample draws over the full disk of `radius`, whatever innerradius and phimax say (disk.cpp:130-131), while
        // Area() and Pdf() count the partial disk only: reproduced as it is, not corrected
        float px, py;
        concentric_sample_disk(u0, u1, &px, &py);
        const F3 pobj = F3{px * q.radius, py * q.radius, q.height};
        it.n = normalize(xf_normal(q.o2w_inv, F3{0, 0, 1}));
        if (q.reverse_orientation) it.n = it.n * -1.f;
        it.p = xf_point_err2(q.o2w, pobj, F3{0, 0, 0}, &it.perr);
    } else {
        const float z = (1 - u0) * q.zmin + u0 * q.zmax;  // Lerp, pbrt.h
        const float phi = u1 * q.phi_max;
        float s, c;
        sincos_f(phi, &s, &c);
        F3 pobj = F3{q.radius * c, q.radius * s, z};
        it.n = normalize(xf_normal(q.o2w_inv, F3{pobj.x, pobj.y, 0}));
        if (q.reverse_orientation) it.n = it.n * -1.f;
        const float hit_rad = sqrtf(pobj.x * pobj.x + pobj.y * pobj.y);
        pobj.x *= q.radius / hit_rad;
        pobj.y *= q.radius / hit_rad;
        const F3 pobj_err = kGamma3 * vabs(F3{pobj.x, pobj.y, 0});
        it.p = xf_point_err2(q.o2w, pobj, pobj_err, &it.perr);
    }
    *pdf = 1 / quadric_area(q);
    return it;
}
DEV LightSample quadric_sample(const DQuadric &q, const Isect &ref, float u0, float u1, float *pdf) {
    LightSample intr = quadric_sample_area(q, u0, u1, pdf);  // Shape::Sample(ref, u, pdf), shape.cpp:56-70
    F3 wi = intr.p - ref.p;
    if (length_sq(wi) == 0)
        *pdf = 0;
    else {
        wi = normalize(wi);
        *pdf *= length_sq(ref.p - intr.p) / absdot(intr.n, -wi);
        if (is_inf(*pdf)) *pdf = 0.f;
    }
    return intr;
}
DEV float quadric_pdf(const DQuadric &q, const Isect &ref, F3 wi) {  // Shape::Pdf(ref, wi), shape.cpp:72-87: the shape alone
    const F3 ro = offset_ray_origin(ref.p, ref.perr, ref.n, wi);
    float t;
    F3 od, ph;
    if (!quadric_test(q, ro, wi, IILE_INF, &t, &od, &ph)) return 0;
    Isect li;
    quadric_interaction(q, od, ph, &li);
    float pdf = length_sq(ref.p - li.p) / (absdot(li.n, -wi) * quadric_area(q));
    if (is_inf(pdf)) pdf = 0.f;
    return pdf;
}
// InfiniteAreaLight (lights/infinite.cpp:42-174), operation for operation as the oracle's inf_* functions: Lmap is
// a host-built pyramid among the textures (one texel without an environment map), the Distribution2D a table
// in HBM: per row {func[w], cdf[w + 1], funcInt}, then the marginal {func[h], cdf[h + 1], funcInt}.
DEV F3 inf_lookup(const DScene &S, const DLight &lt, float s_, float t_) {  // Lmap->Lookup(st) -> triangle(0, st), mipmap.h:233-262
    return tex_triangle(S, S.textures[lt.env_tex], 0, s_, t_);
}
DEV float dist1d_sample(const float *d, int n, float u, float *pdf, int *off) {  // Distribution1D::SampleContinuous, sampling.h:71-89
    const float *cdf = d + n;
    // FindInterval(n + 1, cdf[i] <= u), pbrt.h:399-412
    int first = 0, len = n + 1;
    while (len > 0) {
        const int half = len >> 1, middle = first + half;
        if (cdf[middle] <= u) {
            first = middle + 1;
            len -= half + 1;
        } else
            len = half;
    }
    int offset = first - 1;
    offset = offset < 0 ? 0 : (offset > n - 1 ? n - 1 : offset);
    if (off) *off = offset;
    const float lo = cdf[offset], hi = cdf[offset + 1];
    float du = u - lo;
    if ((hi - lo) > 0) du /= (hi - lo);
    const float func_int = d[2 * n + 1];
    *pdf = (func_int > 0) ? d[offset] / func_int : 0.f;
    return (float(offset) + du) / float(n);
}
DEV const float *inf_cond(const DScene &S, const DLight &lt, int v) { return S.env_dist + lt.dist_offset + (long long)(2 * lt.dist_w + 2) * v; }
DEV F3 inf_w2l(const DLight &lt, F3 w) {
    return F3{lt.w2l[0] * w.x + lt.w2l[1] * w.y + lt.w2l[2] * w.z, lt.w2l[3] * w.x + lt.w2l[4] * w.y + lt.w2l[5] * w.z,
              lt.w2l[6] * w.x + lt.w2l[7] * w.y + lt.w2l[8] * w.z};
}
DEV float spherical_theta(F3 v) { return acos_f(clampf(v.z, -1, 1)); }  // geometry.h:1474-1481
DEV float spherical_phi(F3 v) {
    const float p = atan2_f(v.y, v.x);
    return (p < 0) ? (p + 2 * kPi) : p;
}
DEV F3 inf_le(const DScene &S, const DLight &lt, F3 d) {  // InfiniteAreaLight::Le, infinite.cpp:92-96
    const F3 w = normalize(inf_w2l(lt, d));
    return inf_lookup(S, lt, spherical_phi(w) * kInv2Pi, spherical_theta(w) * kInvPi);
}
DEV F3 inf_sample_li(const DScene &S, const DLight &lt, F3 ref_p, float u0, float u1, F3 *wi, float *pdf, F3 *target) {  // :98-122
    float pdf0, pdf1;
    int v;
    const float d1 = dist1d_sample(inf_cond(S, lt, lt.dist_h), lt.dist_h, u1, &pdf1, &v);
    const float d0 = dist1d_sample(inf_cond(S, lt, v), lt.dist_w, u0, &pdf0, nullptr);
    const float map_pdf = pdf0 * pdf1;
    *pdf = 0;
    if (map_pdf == 0) return F3{0, 0, 0};
    const float theta = d1 * kPi, phi = d0 * 2 * kPi;
    float sin_theta, cos_theta, sin_phi, cos_phi;
    sincos_f(theta, &sin_theta, &cos_theta);
    sincos_f(phi, &sin_phi, &cos_phi);
    const F3 wl = F3{sin_theta * cos_phi, sin_theta * sin_phi, cos_theta};
    *wi = F3{lt.l2w[0] * wl.x + lt.l2w[1] * wl.y + lt.l2w[2] * wl.z, lt.l2w[3] * wl.x + lt.l2w[4] * wl.y + lt.l2w[5] * wl.z,
             lt.l2w[6] * wl.x + lt.l2w[7] * wl.y + lt.l2w[8] * wl.z};
    *pdf = map_pdf / (2 * kPi * kPi * sin_theta);
    if (sin_theta == 0) *pdf = 0;
    *target = ref_p + *wi * (2 * lt.world_radius);
    return inf_lookup(S, lt, d0, d1);
}
DEV float inf_pdf_li(const DScene &S, const DLight &lt, F3 w) {  // :124-132 with Distribution2D::Pdf, sampling.h:135-142
    const F3 wi = inf_w2l(lt, w);
    const float theta = spherical_theta(wi), phi = spherical_phi(wi);
    float sin_theta, cos_theta;
    sincos_f(theta, &sin_theta, &cos_theta);
    // :129 tests sinTheta == 0, which float32 meets at +z only: acos(-1) is the float above pi, whose sine is -8.7e-8, and the pdf
    // came out negative there. Both poles return 0.
    if (sin_theta <= 0) return 0;
    // an all-black map: Distribution2D::Pdf would be 0 / 0. Sample_Li never returns a direction then (mapPdf == 0): the pdf is 0
    const float func_int = inf_cond(S, lt, lt.dist_h)[2 * lt.dist_h + 1];
    if (!(func_int > 0)) return 0;
    const float p0 = phi * kInv2Pi, p1 = theta * kInvPi;
    int iu = int(p0 * float(lt.dist_w)), iv = int(p1 * float(lt.dist_h));
    iu = iu < 0 ? 0 : (iu > lt.dist_w - 1 ? lt.dist_w - 1 : iu);
    iv = iv < 0 ? 0 : (iv > lt.dist_h - 1 ? lt.dist_h - 1 : iv);
    const float func = inf_cond(S, lt, iv)[iu];
    return (func / func_int) / (2 * kPi * kPi * sin_theta);
}

// Triangle emitter (shapes/triangle.cpp:546-579) through the generic Shape::Sample(ref, u) /
// Shape::Pdf(ref, wi) (core/shape.cpp:56-87), and the sphere / quadric / triangle dispatch of an area light
DEV float triangle_area(const DScene &S, int prim) {
    const float4 v0 = S.tri_verts[3 * size_t(prim)], v1 = S.tri_verts[3 * size_t(prim) + 1],
                 v2 = S.tri_verts[3 * size_t(prim) + 2];
    const F3 p0 = F3{v0.x, v0.y, v0.z}, p1 = F3{v1.x, v1.y, v1.z}, p2 = F3{v2.x, v2.y, v2.z};
    return float(0.5 * double(length(cross(p1 - p0, p2 - p0))));
}
DEV LightSample triangle_sample_area(const DScene &S, int prim, float u0, float u1, float *pdf) {
    const float su0 = sqrtf(u0);  // UniformSampleTriangle, sampling.cpp:154-157
    const float b0 = 1 - su0, b1 = u1 * su0;
    const float4 v0 = S.tri_verts[3 * size_t(prim)], v1 = S.tri_verts[3 * size_t(prim) + 1],
                 v2 = S.tri_verts[3 * size_t(prim) + 2];
    const F3 p0 = F3{v0.x, v0.y, v0.z}, p1 = F3{v1.x, v1.y, v1.z}, p2 = F3{v2.x, v2.y, v2.z};
    const uint32_t flags = f2b(v0.w);
    LightSample it;
    it.p = b0 * p0 + b1 * p1 + (1 - b0 - b1) * p2;
    it.n = normalize(cross(p1 - p0, p2 - p0));
    if (flags & 2u) {  // the mesh has normals
        const float4 a = S.tri_norms[3 * size_t(prim)], b = S.tri_norms[3 * size_t(prim) + 1],
                     c = S.tri_norms[3 * size_t(prim) + 2];
        const F3 ns = b0 * F3{a.x, a.y, a.z} + b1 * F3{b.x, b.y, b.z} + (1 - b0 - b1) * F3{c.x, c.y, c.z};
        it.n = faceforward(it.n, ns);
    } else if (flags & 8u)  // reverseOrientation ^ transformSwapsHandedness
        it.n = it.n * -1.f;
    const F3 abs_sum = vabs(b0 * p0) + vabs(b1 * p1) + vabs((1 - b0 - b1) * p2);
    it.perr = kGamma6 * abs_sum;
    *pdf = 1 / triangle_area(S, prim);
    return it;
}
DEV LightSample shape_sample(const DScene &S, const DLight &lt, const Isect &ref, float u0, float u1, float *pdf) {
    if (lt.type == kLightDiffuseArea) return sphere_sample(S.spheres[lt.sphere], ref, u0, u1, pdf);
    if (lt.type == kLightAreaQuadric) return quadric_sample(S.quadrics[lt.quadric], ref, u0, u1, pdf);
    LightSample intr = triangle_sample_area(S, lt.prim, u0, u1, pdf);  // Shape::Sample(ref, u, pdf), shape.cpp:56-70
    F3 wi = intr.p - ref.p;
    if (length_sq(wi) == 0)
        *pdf = 0;
    else {
        wi = normalize(wi);
        *pdf *= length_sq(ref.p - intr.p) / absdot(intr.n, -wi);
        if (is_inf(*pdf)) *pdf = 0.f;
    }
    return intr;
}
// n_tests / n_hits: Triangle::Intersect counts its calls wherever they come from (stats of the
// instrumented kernels)
DEV float shape_pdf(const DScene &S, const DLight &lt, const Isect &ref, F3 wi, unsigned long long *n_tests,
                    unsigned long long *n_hits) {
    if (lt.type == kLightDiffuseArea) return sphere_pdf(S.spheres[lt.sphere], ref, wi);
    if (lt.type == kLightAreaQuadric) return quadric_pdf(S.quadrics[lt.quadric], ref, wi);
    // Shape::Pdf(ref, wi), shape.cpp:72-87: intersect the shape alone
    const F3 o = offset_ray_origin(ref.p, ref.perr, ref.n, wi);
    const RayCtx rc = make_ray_ctx(o, wi);
    const int prim = lt.prim;
    const float4 v0 = S.tri_verts[3 * size_t(prim)], v1 = S.tri_verts[3 * size_t(prim) + 1],
                 v2 = S.tri_verts[3 * size_t(prim) + 2];
    const F3 p0 = F3{v0.x, v0.y, v0.z}, p1 = F3{v1.x, v1.y, v1.z}, p2 = F3{v2.x, v2.y, v2.z};
    float t, b0, b1, b2;
    ++*n_tests;
    if (!triangle_test(rc, IILE_INF, p0, p1, p2, &t, &b0, &b1, &b2)) return 0;
    ++*n_hits;
    Isect li;
    triangle_interaction(S, prim, f2b(v0.w), p0, p1, p2, wi, b0, b1, b2, &li);
    float pdf = length_sq(ref.p - li.p) / (absdot(li.n, -wi) * triangle_area(S, prim));
    if (is_inf(pdf)) pdf = 0.f;
    return pdf;
}
DEV float power_heuristic(float fpdf, float gpdf) {  // sampling.h:169-172 with nf = ng = 1
    float f = 1 * fpdf, g = 1 * gpdf;
    return (f * f) / (f * f + g * g);
}

// DiffuseAreaLight::L (lights/diffuse.h:56-58)
DEV F3 area_light_L(const DLight &lt, F3 n, F3 w) {
    return (lt.two_sided || dot(n, w) > 0) ? F3{lt.lemit[0], lt.lemit[1], lt.lemit[2]} : F3{0, 0, 0};
}
// ProjectionLight::Projection(w) (lights/projection.cpp:88-99); the map is projectionMap, a pyramid among the textures, or none
DEV F3 projection_light_projection(const DScene &S, const DLight &lt, F3 w) {
    const F3 wl = inf_w2l(lt, w);  // WorldToLight(w) on a vector, transform.h:236-241
    if (wl.z < lt.l2w[IILE_PROJ_HITHER]) return F3{0, 0, 0};  // :91
    // lightProjection(Point3f(wl.x, wl.y, wl.z)): Transform::operator()(Point3f), transform.h:222-233, with Point3 / wp as a
    // multiplication by 1 / wp (geometry.h:499-503). Perspective()'s rows 0, 1 and 3 are {m00, 0, 0, 0}, {0, m11, 0, 0} and
    // {0, 0, 1, 0} (transform.cpp:303-311): the products with their exact zeros add +-0 to a finite sum and are left out, the
    // values are the reference's (wl is finite; wp = 1 * wl.z >= hither)
    float xp = lt.l2w[IILE_PROJ_M00] * wl.x;
    float yp = lt.l2w[IILE_PROJ_M11] * wl.y;
    const float wp = wl.z;
    if (wp != 1) {
        const float inv = 1.f / wp;
        xp = inv * xp;
        yp = inv * yp;
    }
    const float *sb = lt.l2w + IILE_PROJ_BOUNDS;
    const float x0 = sb[0], y0 = sb[1], x1 = sb[2], y1 = sb[3];
    if (!(xp >= x0 && xp <= x1 && yp >= y0 && yp <= y1)) return F3{0, 0, 0};  // Inside(Point2f, Bounds2f), geometry.h:1370-1373
    if (lt.env_tex < 0) return F3{1, 1, 1};                                    // :96
    float ox = xp - x0, oy = yp - y0;  // screenBounds.Offset, geometry.h:729-734
    if (x1 > x0) ox /= x1 - x0;
    if (y1 > y0) oy /= y1 - y0;
    return inf_lookup(S, lt, ox, oy);  // projectionMap->Lookup(st), :98
}
// GonioPhotometricLight::Scale(w) (lights/goniometric.h:69-77)
DEV F3 goniometric_light_scale(const DScene &S, const DLight &lt, F3 w) {
    if (lt.env_tex < 0) return F3{1, 1, 1};  // !mipmap, :75
    const F3 wl = normalize(inf_w2l(lt, w));  // Normalize(WorldToLight(w))
    const F3 wp = F3{wl.x, wl.z, wl.y};       // std::swap(wp.y, wp.z)
    const float theta = spherical_theta(wp), phi = spherical_phi(wp);
    return inf_lookup(S, lt, phi * kInv2Pi, theta * kInvPi);  // mipmap->Lookup(Point2f(phi * Inv2Pi, theta * InvPi))
}
// Sample_Li of a delta light (iile_light_is_delta) at p: PointLight (lights/point.cpp:43-52), SpotLight with its Falloff
// (spot.cpp:53-76), DistantLight (distant.cpp:50-61), ProjectionLight (projection.cpp:77-86), GonioPhotometricLight
// (goniometric.cpp:43-53). The pdf is 1; *target is the light-side end of the shadow ray.
DEV F3 delta_light_li(const DScene &S, const DLight &lt, F3 p, F3 *wi, F3 *target) {
    const F3 pos = F3{lt.pos[0], lt.pos[1], lt.pos[2]};
    const F3 I = F3{lt.lemit[0], lt.lemit[1], lt.lemit[2]};
    if (lt.type == kLightDistant) {
        *wi = pos;                                  // wLight
        *target = p + pos * (2 * lt.world_radius);  // pOutside
        return I;
    }
    *wi = normalize(pos - p);
    *target = pos;  // pLight
    if (lt.type == kLightPoint) return sdiv(I, length_sq(pos - p));
    if (lt.type == kLightProjection) return sdiv(I * projection_light_projection(S, lt, -*wi), length_sq(pos - p));
    if (lt.type == kLightGoniometric) return sdiv(I * goniometric_light_scale(S, lt, -*wi), length_sq(pos - p));
    const F3 w = -*wi;
    const F3 wl = normalize(F3{lt.w2l[0] * w.x + lt.w2l[1] * w.y + lt.w2l[2] * w.z,
                               lt.w2l[3] * w.x + lt.w2l[4] * w.y + lt.w2l[5] * w.z,
                               lt.w2l[6] * w.x + lt.w2l[7] * w.y + lt.w2l[8] * w.z});
    const float cos_theta = wl.z;
    float falloff;
    if (cos_theta < lt.cos_total_width)
        falloff = 0;
    else if (cos_theta >= lt.cos_falloff_start)
        falloff = 1;
    else {
        const float delta = (cos_theta - lt.cos_total_width) / (lt.cos_falloff_start - lt.cos_total_width);
        falloff = (delta * delta) * (delta * delta);
    }
    return sdiv(I * falloff, length_sq(pos - p));
}
// ===========================================================================
// choosing a light: SpatialLightDistribution::Lookup (lightdistrib.cpp:134-226; the voxels are tabulated at scene creation,
// kernels_shade.hip) + Distribution1D::SampleDiscrete (sampling.h:90-100, FindInterval pbrt.h:399-412). The uniform and power
// strategies keep a grid of one voxel. A record is func[n] | cdf[n + 1] | funcInt; the whole table stays under 2^28 floats.
// ===========================================================================
DEV int sample_light(const DScene &S, F3 p, float u, float *pdf) {
    const F3 bmin = F3{S.root_box[0], S.root_box[1], S.root_box[2]}, bmax = F3{S.root_box[3], S.root_box[4], S.root_box[5]};
    F3 o = p - bmin;  // Bounds3::Offset, geometry.h:800-806
    if (bmax.x > bmin.x) o.x = o.x / (bmax.x - bmin.x);
    if (bmax.y > bmin.y) o.y = o.y / (bmax.y - bmin.y);
    if (bmax.z > bmin.z) o.z = o.z / (bmax.z - bmin.z);
    int pi0 = int(o.x * float(S.light_nv[0])), pi1 = int(o.y * float(S.light_nv[1])), pi2 = int(o.z * float(S.light_nv[2]));
    pi0 = pi0 < 0 ? 0 : (pi0 > S.light_nv[0] - 1 ? S.light_nv[0] - 1 : pi0);
    pi1 = pi1 < 0 ? 0 : (pi1 > S.light_nv[1] - 1 ? S.light_nv[1] - 1 : pi1);
    pi2 = pi2 < 0 ? 0 : (pi2 > S.light_nv[2] - 1 ? S.light_nv[2] - 1 : pi2);
    const int n = S.n_lights, size = n + 1;
    const float *d = S.light_dist + uint32_t((pi0 * S.light_nv[1] + pi1) * S.light_nv[2] + pi2) * light_record_floats(n);
    const float *cdf = d + n;
    int first = 0, len = size;
    while (len > 0) {
        const int half = len >> 1, middle = first + half;
        if (cdf[middle] <= u) {
            first = middle + 1;
            len -= half + 1;
        } else
            len = half;
    }
    int offset = first - 1;
    offset = offset < 0 ? 0 : (offset > size - 2 ? size - 2 : offset);
    const float func_int = d[2 * n + 1];
    *pdf = (func_int > 0) ? d[offset] / (func_int * float(n)) : 0.f;
    return offset;
}
