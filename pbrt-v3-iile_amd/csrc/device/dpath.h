// dpath.h — device functions of the wavefront path tracer: Halton sampling,
// camera rays, ray/primitive tests, BVH traversal with an LDS-resident stack (dtrav.h),
// surface interactions, BSDFs and light sampling.
//
// Citations are relative to /root/reference/src. The traversal keeps the
// reference's node layout and near-first order (bvh.cpp:686-692), so equal-t
// ties resolve to the same primitive as on the CPU.
#pragma once
#include "dscene.h"

namespace iile {

// ===========================================================================
// Halton sampler (samplers/halton.cpp:96-127, core/lowdiscrepancy.cpp:389-427)
// ===========================================================================
// exact a / base for any 32-bit a (Granlund-Montgomery round-up form)
DEV uint32_t div_magic(uint32_t a, uint32_t magic, uint32_t shift) {
    uint32_t t = __umulhi(magic, a);
    return (t + ((a - t) >> 1)) >> shift;
}

// Global Halton index of sample k of pixel (px, py): offset(pixel mod 128) +
// k * stride. 32-bit arithmetic is exact here: the render entry point rejects
// (spp + 1) * stride >= 2^32.
DEV uint32_t halton_index(const DScene &S, int px, int py, uint32_t k) {
    int pmx = px - (px / 128) * 128, pmy = py - (py / 128) * 128;  // Mod(), pbrt.h:310-314
    if (pmx < 0) pmx += 128;
    if (pmy < 0) pmy += 128;
    // offsetForCurrentPixel (halton.cpp:96-122), tabulated at scene upload
    return S.pixel_offsets[pmy * 128 + pmx] + k * uint32_t(S.sample_stride);
}

DEV float radical_inverse_base2(uint32_t a) {
    // ReverseBits64(a) * 0x1p-64 with a < 2^32: the reversed bits land in the
    // upper word (lowdiscrepancy.cpp:430-434); double product, one rounding to float.
    unsigned long long rev = (unsigned long long)__brev(a) << 32;
    return float(double(rev) * 0x1p-64);
}
DEV float radical_inverse_base3(uint32_t a0) {
    // RadicalInverseSpecialized<3> (lowdiscrepancy.cpp:389-407); digits peeled in double
    // arithmetic, exact for every u32 (see scrambled_radical_inverse)
    const float inv_base = 1.f / 3.f;
    double a = double(a0), reversed = 0;
    float inv_base_n = 1;
    while (a != 0) {
        const double next = __builtin_trunc((a + 0.5) * (1.0 / 3.0));
        reversed = __builtin_fma(reversed, 3.0, __builtin_fma(-next, 3.0, a));
        inv_base_n *= inv_base;
        a = next;
    }
    return mn(float(reversed) * inv_base_n, kOneMinusEpsilon);
}
// `perms` is the concatenated permutation table, either in HBM (const uint16_t *) or
// staged in LDS by the shade kernel (lds_u16 *): a path needs one table lookup per
// digit per dimension, ~30 dependent lookups per bounce.
typedef __attribute__((address_space(3))) uint16_t lds_u16;
// ScrambledRadicalInverseSpecialized (lowdiscrepancy.cpp:409-424). The digits are peeled in
// double arithmetic: next = trunc((a + 0.5) / base) is exact for every u32 a (the fractional
// part of (a + 0.5) / base stays >= 0.5 / base away from an integer, far more than the 2^-22
// the rounded product can be off by), digit = a - next * base and reversed * base + perm are
// exact integers below 2^53, and the final uint64 -> float conversion of the reference rounds
// the same integer the same way as double -> float here.
template <typename PermPtr>
DEV float scrambled_radical_inverse(const DScene &S, PermPtr perms, int dim, uint32_t a0) {
    const DHaltonDim hd = S.hdims[dim];
    PermPtr perm = perms + hd.perm_offset;
    double a = double(a0), reversed = 0;
    float inv_base_n = 1;
    while (a != 0) {
        const double next = __builtin_trunc(__builtin_fma(a, hd.inv_base_d, 0.5 * hd.inv_base_d));  // (a + 0.5) / base, one rounding
        const uint32_t digit = uint32_t(__builtin_fma(-next, hd.base_d, a));
        reversed = __builtin_fma(reversed, hd.base_d, double(uint32_t(perm[digit])));
        inv_base_n *= hd.inv_base;
        a = next;
    }
    return mn(inv_base_n * (float(reversed) + hd.perm0_term), kOneMinusEpsilon);
}
// N consecutive dimensions of one sample index, `dim0` wave-uniform: the per-dimension
// constants come through scalar loads, and the N digit chains advance together so that their
// LDS lookups overlap (one chain alone waits out one LDS round trip per digit).
typedef const __attribute__((address_space(4))) DHaltonDim *HaltonDimConst;
// An entry of the sphere / light table whose index is the same in every lane (the scene's only sphere, the only light):
// read through the constant address space its fields arrive by scalar loads into SGPRs, once per wavefront, instead of
// one vector-memory instruction per field with 64 identical addresses (k_shade spent ~13 of its ~30 loads per hit so).
// (a copy, field by field out of that address space: a reference would have to pass through a generic pointer, and the
// constant address space is lost on the way whenever the index folds to a constant; loads of unused fields are dropped)
template <typename T>
DEV T uniform_entry(const T *table, int idx) {
    typedef const __attribute__((address_space(4))) T *ConstPtr;
    T out;
    __builtin_memcpy(&out, (ConstPtr)(table) + __builtin_amdgcn_readfirstlane(idx), sizeof(T));
    return out;
}
template <int N, typename PermPtr>
DEV void scrambled_radical_inverse_n(const DScene &S, PermPtr perms, int dim0, uint32_t index, float *out) {
    const HaltonDimConst hd = (HaltonDimConst)(S.hdims) + dim0;
    double a[N], reversed[N];
    float inv_base_n[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        a[i] = double(index);
        reversed[i] = 0;
        inv_base_n[i] = 1;
    }
    // all chains run unpredicated while every one of them still has digits left ...
    for (;;) {
        bool all = true;
#pragma unroll
        for (int i = 0; i < N; ++i) all = all && a[i] != 0;
        if (!all) break;
        uint32_t digit[N], p[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double next = __builtin_trunc(__builtin_fma(a[i], hd[i].inv_base_d, 0.5 * hd[i].inv_base_d));  // (a + 0.5) / base, one rounding
            digit[i] = uint32_t(__builtin_fma(-next, hd[i].base_d, a[i]));
            a[i] = next;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = uint32_t(perms[hd[i].perm_offset + digit[i]]);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            reversed[i] = __builtin_fma(reversed[i], hd[i].base_d, double(p[i]));
            inv_base_n[i] *= hd[i].inv_base;
        }
    }
    // ... then the larger bases' last digit or two, chain by chain
#pragma unroll
    for (int i = 0; i < N; ++i) {
        while (a[i] != 0) {
            const double next = __builtin_trunc(__builtin_fma(a[i], hd[i].inv_base_d, 0.5 * hd[i].inv_base_d));  // (a + 0.5) / base, one rounding
            const uint32_t digit = uint32_t(__builtin_fma(-next, hd[i].base_d, a[i]));
            reversed[i] = __builtin_fma(reversed[i], hd[i].base_d, double(uint32_t(perms[hd[i].perm_offset + digit])));
            inv_base_n[i] *= hd[i].inv_base;
            a[i] = next;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
        out[i] = mn(inv_base_n[i] * (float(reversed[i]) + hd[i].perm0_term), kOneMinusEpsilon);
}
// ===========================================================================
// Sobol' sampler (samplers/sobol.cpp:42-59, core/lowdiscrepancy.h:229-274): the sampler the fork's path integrator
// renders with under IILE_PATH_SAMPLES_OVERRIDE (integrators/path.cpp:202-212). Indices stay below 2^32 (checked on the
// host), so 32 columns per generator matrix are kept.
// ===========================================================================
// XOR of the columns a 32-bit word selects, through its four bytes (byte tables: DScene::sobol_bt)
DEV uint32_t sobol_xor4(const uint32_t *bt, uint32_t w) {
    return bt[w & 255u] ^ bt[256u + ((w >> 8) & 255u)] ^ bt[512u + ((w >> 16) & 255u)] ^ bt[768u + (w >> 24)];
}
DEV uint32_t sobol_index(const DScene &S, int px, int py, uint32_t k) {
    const int m = S.sobol_log2res, m2 = 2 * m;
    // `for (c ...) if ((k >> c) & 1) delta ^= vdc[c]` ("add flipped column m + c + 1"; k < 2^(32 - 2m))
    const uint32_t delta = sobol_xor4(S.sobol_vdc_bt, k);
    const uint32_t b = ((uint32_t(px - S.samp_x0) << m) | uint32_t(py - S.samp_y0)) ^ delta;  // flipped b, < 2^(2m)
    // `for (c ...) if ((b >> c) & 1) index ^= vdc_inv[c]` ("add column 2 m - c")
    return (k << m2) ^ sobol_xor4(S.sobol_vdc_bt + 1024, b);
}
// SobolSampleFloat (scramble 0) followed by SobolSampler::SampleDimension's remapping of the two pixel dimensions
template <typename PermPtr>
DEV float sobol_sample_dimension(const DScene &S, PermPtr mats, uint32_t index, int dim, int px, int py) {
    // SobolSample: XOR of the generator-matrix columns the index's bits select (lowdiscrepancy.h:229-241)
    (void)mats;
    const uint32_t v = sobol_xor4(S.sobol_bt + size_t(dim) * 1024, index);
    float s = mn(float(v) * 0x1p-32f /* 1/2^32 */, kOneMinusEpsilon);
    if (dim == 0 || dim == 1) {  // s * resolution + sampleBounds.pMin[dim], then Clamp(s - currentPixel[dim], 0, OneMinusEpsilon)
        const int pmin = dim == 0 ? S.samp_x0 : S.samp_y0, cur = dim == 0 ? px : py;
        s = s * float(S.sobol_res) + float(pmin);
        s = s - float(cur);
        s = s < 0.f ? 0.f : (s > kOneMinusEpsilon ? kOneMinusEpsilon : s);
    }
    return s;
}

// The scene's sampler: GetIndexForSample / SampleDimension of HaltonSampler or SobolSampler. (px, py) is the sample's
// pixel — only SobolSampler's dimensions 0 and 1 depend on it.
DEV uint32_t sample_index(const DScene &S, int px, int py, uint32_t k) {
    return S.sobol ? sobol_index(S, px, py, k) : halton_index(S, px, py, k);
}
template <typename PermPtr>
DEV float sample_dimension(const DScene &S, PermPtr perms, uint32_t index, int dim, int px = 0, int py = 0) {
    if (S.sobol) return sobol_sample_dimension(S, perms, index, dim, px, py);
    if (S.sample_center && dim < 2) return 0.5f;  // "samplepixelcenter", halton.cpp:119
    if (dim == 0) return radical_inverse_base2(index >> S.base_exp0);
    if (dim == 1) return radical_inverse_base3(index / uint32_t(S.base_scale1));
    return scrambled_radical_inverse(S, perms, dim, index);
}
// the same for a dimension the caller knows to be >= 2 (every dimension after the camera sample's film position): none of the
// code — and none of the hoisted constants — of the two pixel dimensions
template <typename PermPtr>
DEV float sample_dimension_hi(const DScene &S, PermPtr perms, uint32_t index, int dim) {
    if (dim < 2) __builtin_unreachable();
    return sample_dimension(S, perms, index, dim);
}
DEV float sample_dimension(const DScene &S, uint32_t index, int dim, int px = 0, int py = 0) {
    return sample_dimension(S, S.perms, index, dim, px, py);
}
// N consecutive dimensions >= 2 of one sample (the shade kernel's batches)
template <int N, typename PermPtr>
DEV void sample_dimensions_n(const DScene &S, PermPtr perms, int dim0, bool dim_uniform, int dim_lane, uint32_t index, float *out) {
    if (dim_lane < 2) __builtin_unreachable();
    if (S.sobol) {
#pragma unroll
        for (int i = 0; i < N; ++i) out[i] = sobol_sample_dimension(S, perms, index, dim_lane + i, 0, 0);
    } else if (dim_uniform) {
        scrambled_radical_inverse_n<N>(S, perms, dim0, index, out);
    } else {
        for (int i = 0; i < N; ++i) out[i] = sample_dimension_hi(S, perms, index, dim_lane + i);
    }
}

// ===========================================================================
// sampling warps (core/sampling.cpp:113-130, core/sampling.h:159-163)
// ===========================================================================
DEV void concentric_sample_disk(float u0, float u1, float *dx, float *dy) {
    float ox = 2.f * u0 - 1, oy = 2.f * u1 - 1;
    if (ox == 0 && oy == 0) {
        *dx = 0;
        *dy = 0;
        return;
    }
    float theta, r;
    if (fabsf(ox) > fabsf(oy)) {
        r = ox;
        theta = kPiOver4 * (oy / ox);
    } else {
        r = oy;
        theta = kPiOver2 - kPiOver4 * (ox / oy);
    }
    float s, c;
    sincos_f(theta, &s, &c);
    *dx = r * c;
    *dy = r * s;
}
DEV F3 cosine_sample_hemisphere(float u0, float u1) {
    float dx, dy;
    concentric_sample_disk(u0, u1, &dx, &dy);
    float z = sqrtf(mx(0.f, 1 - dx * dx - dy * dy));
    return F3{dx, dy, z};
}

// ===========================================================================
// camera (cameras/perspective.cpp:100-149, cameras/environment.cpp:43-56, core/transform.h:251-264)
// ===========================================================================
// `zero` is 0.f: a caller inside a persistent loop passes one the compiler cannot see through (opaque_zero), so that the
// products of matrix entries (SGPRs) with it are worked out where they are used instead of being hoisted out of the loop
// into VGPRs that then live — or spill — across the whole kernel.
DEV float opaque_zero() {
    float z = 0.f;
    asm volatile("" : "+v"(z));
    return z;
}
// EnvironmentCamera::GenerateRay's direction (environment.cpp:47-50), not normalised. A call, not inline code: the kind is a
// scene constant, and inline the double-precision sine and cosine of this branch changed the register allocation (scratch,
// VGPRs) of every kernel that makes a perspective camera ray.
static __device__ __attribute__((noinline)) F3 env_camera_direction(float pfx, float pfy, int xres, int yres) {
    const float theta = kPi * pfy / float(yres);
    const float phi = 2 * kPi * pfx / float(xres);
    float st, ct, sp, cp;
    sincos_f(theta, &st, &ct);
    sincos_f(phi, &sp, &cp);
    return F3{st * cp, ct, st * sp};
}
// ANY_CAMERA = false: the perspective camera alone, for the two sites that make their camera ray inside a persistent traversal /
// shading loop (PassDesc::gen_fused, which a pass with an environment camera does not set): with the other camera's branch in
// them, k_extend<.., GEN> and the plain k_shade take more scratch, whichever way that branch is compiled.
template <bool ANY_CAMERA = true>
DEV void camera_ray(const DScene &S, float pfx, float pfy, float lu0, float lu1, F3 *o_out, F3 *d_out, float *tmax,
                    const float zero = 0.f) {
    F3 ro = F3{zero, zero, zero};
    F3 rd;
    if (ANY_CAMERA && S.env_camera) {
        // the origin is (0, 0, 0), there is no lens (environment.cpp:51). (S.xres / S.yres are the frame's: the probe pass,
        // which swaps them, makes probe_ray's rays.)
        rd = env_camera_direction(pfx, pfy, S.xres, S.yres);
    } else {
        F3 pcam = xf_point(S.raster_to_camera, F3{pfx, pfy, zero});
        rd = normalize(pcam);
        if (S.lens_radius > 0) {
            float lx, ly;
            concentric_sample_disk(lu0, lu1, &lx, &ly);
            lx = S.lens_radius * lx;
            ly = S.lens_radius * ly;
            float ft = S.focal_distance / rd.z;
            F3 pfocus = ro + rd * ft;
            ro = F3{lx, ly, zero};
            rd = normalize(pfocus - ro);
        }
    }
    F3 oerr;
    F3 o = xf_point_err(S.camera_to_world, ro, &oerr);
    F3 d = xf_vector(S.camera_to_world, rd);
    float len2 = length_sq(d);
    float tm = IILE_INF;
    if (len2 > 0) {
        float dt = dot(vabs(d), oerr) / len2;
        o = o + d * dt;
        tm -= dt;
    }
    *o_out = o;
    *d_out = d;
    *tmax = tm;
}

// HemisphericCamera::GenerateRay (hemispheric.cpp:15-41) + Transform::operator()(Ray) (transform.h:251-264)
DEV void probe_ray(const DScene &S, const DProbeCam &cam, float pfx, float pfy, F3 *o_out, F3 *d_out, float *tmax) {
    const float theta = kPi * pfy / float(S.yres);
    const float phi = kPi * pfx / float(S.xres);
    float st, ct, sp, cp;
    sincos_f(theta, &st, &ct);
    sincos_f(phi, &sp, &cp);
    const F3 dir = F3{st * cp, ct, st * sp};
    F3 oerr;
    F3 o = xf_point_err(cam.c2w, F3{0, 0, 0}, &oerr);
    const F3 d = xf_vector(cam.c2w, dir);
    const float len2 = length_sq(d);
    float tm = IILE_INF;
    if (len2 > 0) {
        const float dt = dot(vabs(d), oerr) / len2;
        o = o + d * dt;
        tm -= dt;
    }
    *o_out = o;
    *d_out = d;
    *tmax = tm;
}

// The auxiliary rays of the camera ray's RayDifferential: GenerateRayDifferential (perspective.cpp:124-148),
// Transform::operator()(RayDifferential) (transform.h:265-274) and the render loop's
// ScaleDifferentials(1 / sqrt(spp)) (geometry.h:908-913). (o, d) is the camera ray as camera_ray returns it.
struct RayDiff {
    F3 rxo, ryo, rxd, ryd;
};
// The environment camera has no GenerateRayDifferential of its own: Camera::GenerateRayDifferential (camera.cpp:60-96), the
// rays through the film points shifted by eps = 0.05 in x and in y, differenced (every ray's weight is 1, so the -0.05 retry
// never runs); then ScaleDifferentials
DEV RayDiff env_camera_differentials(const DScene &S, float pfx, float pfy, F3 o, F3 d) {
    const float eps = .05f;
    F3 xo, xd, yo, yd;
    float tm;
    camera_ray(S, pfx + eps, pfy, 0.f, 0.f, &xo, &xd, &tm);
    camera_ray(S, pfx, pfy + eps, 0.f, 0.f, &yo, &yd, &tm);
    const float inv = 1.f / eps;  // Vector3::operator/ multiplies by the reciprocal
    const F3 rxo = o + (xo - o) * inv, rxd = d + (xd - d) * inv;
    const F3 ryo = o + (yo - o) * inv, ryd = d + (yd - d) * inv;
    const float sc = S.diff_scale;
    RayDiff r;
    r.rxo = o + (rxo - o) * sc;
    r.ryo = o + (ryo - o) * sc;
    r.rxd = d + (rxd - d) * sc;
    r.ryd = d + (ryd - d) * sc;
    return r;
}
DEV RayDiff camera_differentials(const DScene &S, float pfx, float pfy, float lu0, float lu1, F3 o, F3 d) {
    if (S.env_camera) return env_camera_differentials(S, pfx, pfy, o, d);
    const F3 pcam = xf_point(S.raster_to_camera, F3{pfx, pfy, 0});
    const F3 dxc = F3{S.dx_camera[0], S.dx_camera[1], S.dx_camera[2]}, dyc = F3{S.dy_camera[0], S.dy_camera[1], S.dy_camera[2]};
    F3 rxo = F3{0, 0, 0}, ryo = F3{0, 0, 0}, rxd, ryd;
    if (S.lens_radius > 0) {
        float lx, ly;
        concentric_sample_disk(lu0, lu1, &lx, &ly);
        lx = S.lens_radius * lx;
        ly = S.lens_radius * ly;
        const F3 dx = normalize(pcam + dxc);
        float ft = S.focal_distance / dx.z;
        F3 pfocus = F3{0, 0, 0} + (ft * dx);
        rxo = F3{lx, ly, 0};
        rxd = normalize(pfocus - rxo);
        const F3 dy = normalize(pcam + dyc);
        ft = S.focal_distance / dy.z;
        pfocus = F3{0, 0, 0} + (ft * dy);
        ryo = F3{lx, ly, 0};
        ryd = normalize(pfocus - ryo);
    } else {
        rxd = normalize(pcam + dxc);
        ryd = normalize(pcam + dyc);
    }
    rxo = xf_point(S.camera_to_world, rxo);
    ryo = xf_point(S.camera_to_world, ryo);
    rxd = xf_vector(S.camera_to_world, rxd);
    ryd = xf_vector(S.camera_to_world, ryd);
    const float sc = S.diff_scale;
    RayDiff r;
    r.rxo = o + (rxo - o) * sc;
    r.ryo = o + (ryo - o) * sc;
    r.rxd = d + (rxd - d) * sc;
    r.ryd = d + (ryd - d) * sc;
    return r;
}
// Camera::GenerateRayDifferential (camera.cpp:60-96) for the hemispheric probe camera: the rays through the film
// points shifted by eps = 0.05 in x and in y, differenced; then ScaleDifferentials as above
DEV RayDiff probe_differentials(const DScene &S, const DProbeCam &cam, float pfx, float pfy, F3 o, F3 d) {
    const float eps = .05f;
    F3 xo, xd, yo, yd;
    float tm;
    probe_ray(S, cam, pfx + eps, pfy, &xo, &xd, &tm);
    probe_ray(S, cam, pfx, pfy + eps, &yo, &yd, &tm);
    const float inv = 1.f / eps;  // Vector3::operator/ multiplies by the reciprocal
    const F3 rxo = o + (xo - o) * inv, rxd = d + (xd - d) * inv;
    const F3 ryo = o + (yo - o) * inv, ryd = d + (yd - d) * inv;
    const float sc = S.diff_scale;
    RayDiff r;
    r.rxo = o + (rxo - o) * sc;
    r.ryo = o + (ryo - o) * sc;
    r.rxd = d + (rxd - d) * sc;
    r.ryd = d + (ryd - d) * sc;
    return r;
}

// ===========================================================================
// ray / primitive tests
// ===========================================================================
struct RayCtx {  // per-ray constants of the watertight test (triangle.cpp:206-226) and the slab test
    // origin as three scalars, not an F3: as a sub-struct it survived scalar replacement (the
    // vectorizer gave it overlapping float2 accesses) and lived in scratch / LDS, not registers
    float ox, oy, oz;
    DEV F3 o() const { return F3{ox, oy, oz}; }
    float Sx, Sy, Sz;
    F3 inv_dir;
    int neg_mask;  // bits 0..2: dirIsNeg[xyz] (bvh.cpp:667); bits 4..5: kz, the max-|d| axis;
                   // bit 7: some 1/d is infinite, so a slab product can be NaN (0 * inf);
                   // bytes 1..3: where the ray's ENTRY planes sit in a four-wide record (byte offsets of the x, y, z
                   // planes it meets first: min planes at 0 / 16 / 32, max planes 48 further on; trav_interior4)
};
DEV float comp(F3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }
DEV RayCtx make_ray_ctx(F3 o, F3 d) {
    RayCtx c;
    c.ox = o.x;
    c.oy = o.y;
    c.oz = o.z;
    F3 ad = vabs(d);
    const int kz = (ad.x > ad.y) ? ((ad.x > ad.z) ? 0 : 2) : ((ad.y > ad.z) ? 1 : 2);  // MaxDimension
    // Permute(d, kx, ky, kz) with kx = kz+1, ky = kx+1 (mod 3)
    const float dx = kz == 0 ? d.y : (kz == 1 ? d.z : d.x);
    const float dy = kz == 0 ? d.z : (kz == 1 ? d.x : d.y);
    const float dz = kz == 0 ? d.x : (kz == 1 ? d.y : d.z);
    c.Sx = -dx / dz;
    c.Sy = -dy / dz;
    c.inv_dir = F3{1 / d.x, 1 / d.y, 1 / d.z};  // bvh.cpp:666
    // Sz = 1.f / dz with dz the kz-th component of d: the quotient invDir already holds (one IEEE division less per ray)
    c.Sz = kz == 0 ? c.inv_dir.x : (kz == 1 ? c.inv_dir.y : c.inv_dir.z);
    c.neg_mask = (c.inv_dir.x < 0 ? 1 : 0) | (c.inv_dir.y < 0 ? 2 : 0) | (c.inv_dir.z < 0 ? 4 : 0) | (kz << 4);
    c.neg_mask |= int(((c.inv_dir.x < 0 ? 48u : 0u) << 8) | ((c.inv_dir.y < 0 ? 64u : 16u) << 16) | ((c.inv_dir.z < 0 ? 80u : 32u) << 24));
    if (!(fabsf(c.inv_dir.x) < IILE_INF && fabsf(c.inv_dir.y) < IILE_INF && fabsf(c.inv_dir.z) < IILE_INF)) c.neg_mask |= 0x80;
    return c;
}

// Triangle::Intersect up to the conservative t test (triangle.cpp:196-275);
// the SurfaceInteraction part is deferred to the shade kernel.
DEV bool triangle_test(const RayCtx &rc, float tmax, F3 p0, F3 p1, F3 p2, float *t_out, float *b0o, float *b1o,
                       float *b2o) {
    const F3 ro = rc.o();
    F3 a = p0 - ro, b = p1 - ro, c = p2 - ro;
    const int kz = (rc.neg_mask >> 4) & 3;
    // Permute(p, kx, ky, kz): kz == 0 -> (y,z,x); kz == 1 -> (z,x,y); kz == 2 -> (x,y,z)
    float ax = kz == 0 ? a.y : (kz == 1 ? a.z : a.x), ay = kz == 0 ? a.z : (kz == 1 ? a.x : a.y),
          az = kz == 0 ? a.x : (kz == 1 ? a.y : a.z);
    float bx = kz == 0 ? b.y : (kz == 1 ? b.z : b.x), by = kz == 0 ? b.z : (kz == 1 ? b.x : b.y),
          bz = kz == 0 ? b.x : (kz == 1 ? b.y : b.z);
    float cx = kz == 0 ? c.y : (kz == 1 ? c.z : c.x), cy = kz == 0 ? c.z : (kz == 1 ? c.x : c.y),
          cz = kz == 0 ? c.x : (kz == 1 ? c.y : c.z);
    ax += rc.Sx * az;
    ay += rc.Sy * az;
    bx += rc.Sx * bz;
    by += rc.Sy * bz;
    cx += rc.Sx * cz;
    cy += rc.Sy * cz;
    float e0 = bx * cy - by * cx;
    float e1 = cx * ay - cy * ax;
    float e2 = ax * by - ay * bx;
    if (e0 == 0.0f || e1 == 0.0f || e2 == 0.0f) {  // double-precision fallback on edges
        double p2txp1ty = (double)cx * (double)by;
        double p2typ1tx = (double)cy * (double)bx;
        e0 = (float)(p2typ1tx - p2txp1ty);
        double p0txp2ty = (double)ax * (double)cy;
        double p0typ2tx = (double)ay * (double)cx;
        e1 = (float)(p0typ2tx - p0txp2ty);
        double p1txp0ty = (double)bx * (double)ay;
        double p1typ0tx = (double)by * (double)ax;
        e2 = (float)(p1typ0tx - p1txp0ty);
    }
    if ((e0 < 0 || e1 < 0 || e2 < 0) && (e0 > 0 || e1 > 0 || e2 > 0)) return false;
    float det = e0 + e1 + e2;
    if (det == 0) return false;
    az *= rc.Sz;
    bz *= rc.Sz;
    cz *= rc.Sz;
    float t_scaled = e0 * az + e1 * bz + e2 * cz;
    if (det < 0 && (t_scaled >= 0 || t_scaled < tmax * det))
        return false;
    else if (det > 0 && (t_scaled <= 0 || t_scaled > tmax * det))
        return false;
    float inv_det = 1 / det;
    float b0 = e0 * inv_det, b1 = e1 * inv_det, b2 = e2 * inv_det;
    float t = t_scaled * inv_det;
    float max_zt = max3(fabsf(az), fabsf(bz), fabsf(cz));
    float delta_z = kGamma3 * max_zt;
    float max_xt = max3(fabsf(ax), fabsf(bx), fabsf(cx));
    float max_yt = max3(fabsf(ay), fabsf(by), fabsf(cy));
    float delta_x = kGamma5 * (max_xt + max_zt);
    float delta_y = kGamma5 * (max_yt + max_zt);
    float delta_e = 2 * (kGamma2 * max_xt * max_yt + delta_y * max_xt + delta_x * max_yt);
    float max_e = max3(fabsf(e0), fabsf(e1), fabsf(e2));
    float delta_t = 3 * (kGamma3 * max_e * max_zt + delta_e * max_zt + delta_z * max_e) * fabsf(inv_det);
    if (t <= delta_t) return false;
    *t_out = t;
    *b0o = b0;
    *b1o = b1;
    *b2o = b2;
    return true;
}

// Sphere::Intersect / IntersectP up to the hit decision (sphere.cpp:49-103), partial spheres included (zmin / zmax / phimax: the
// clipping branch of :89-104 — taken, and phi's atan2 evaluated, only for a sphere that is cut: a full sphere's test cannot fail).
// Outputs the object-space ray and refined hit point for sphere_interaction.
DEV bool sphere_test(const DSphere &sp, F3 ro, F3 rd, float tmax, float *t_hit, F3 *obj_d, F3 *phit) {
    F3 oerr, derr;
    F3 o = xf_point_err(sp.o2w_inv, ro, &oerr);
    F3 d = xf_vector_err(sp.o2w_inv, rd, &derr);
    float len2 = length_sq(d);
    if (len2 > 0) {  // transform.h:382-394 (tMax unchanged)
        float dt = dot(vabs(d), oerr) / len2;
        o = o + d * dt;
    }
    // Exact early-out on the value track of the interval arithmetic. Every EFloat
    // keeps lo <= v <= hi, and `v` never depends on lo/hi, so
    //   t0.v > tMax  =>  t0.hi > tMax   and   t1.v <= 0  =>  t1.lo <= 0,
    // i.e. the reference's rejection `t0.UpperBound() > tMax || t1.LowerBound() <= 0`
    // (sphere.cpp:72) is already decided. Shadow rays all end 1e-4 short of the
    // light they aim at, so nearly every sphere test on this path leaves here
    // without the ~40 next_up/next_down pairs of the interval track.
    {
        const float av = (d.x * d.x + d.y * d.y) + d.z * d.z;
        const float bv = 2.f * ((d.x * o.x + d.y * o.y) + d.z * o.z);
        const float cv = ((o.x * o.x + o.y * o.y) + o.z * o.z) - sp.radius * sp.radius;
        const double discrim = (double)bv * (double)bv - 4. * (double)av * (double)cv;
        if (discrim < 0.) return false;
        const float root = float(sqrt(discrim));
        const float qv = (bv < 0) ? -.5f * (bv - root) : -.5f * (bv + root);
        float t0v = qv / av, t1v = cv / qv;
        if (t0v > t1v) {
            const float tmp = t0v;
            t0v = t1v;
            t1v = tmp;
        }
        if (t0v > tmax || t1v <= 0) return false;
    }
    EF ox = ef(o.x, oerr.x), oy = ef(o.y, oerr.y), oz = ef(o.z, oerr.z);
    EF dx = ef(d.x, derr.x), dy = ef(d.y, derr.y), dz = ef(d.z, derr.z);
    EF a = dx * dx + dy * dy + dz * dz;
    EF b = ef(2.f) * (dx * ox + dy * oy + dz * oz);
    EF c = ox * ox + oy * oy + oz * oz - ef(sp.radius) * ef(sp.radius);
    EF t0, t1;
    if (!ef_quadratic(a, b, c, &t0, &t1)) return false;
    if (t0.hi > tmax || t1.lo <= 0) return false;
    EF ts = t0;
    if (ts.lo <= 0) {
        ts = t1;
        if (ts.hi > tmax) return false;
    }
    F3 ph = o + d * ts.v;
    float scale = sp.radius / length(ph);
    ph = F3{ph.x * scale, ph.y * scale, ph.z * scale};
    if (ph.x == 0 && ph.y == 0) ph.x = 1e-5f * sp.radius;
    const bool z_cut = sp.zmin > -sp.radius || sp.zmax < sp.radius, phi_cut = sp.phi_max < 6.2831853f;   // Radians(360) = 6.2831855f
    if (z_cut || phi_cut) {
        auto clipped = [&](F3 q) {
            bool out = (sp.zmin > -sp.radius && q.z < sp.zmin) || (sp.zmax < sp.radius && q.z > sp.zmax);
            if (phi_cut) {
                float phi = atan2_f(q.y, q.x);
                if (phi < 0) phi += 2 * kPi;
                out = out || phi > sp.phi_max;
            }
            return out;
        };
        if (clipped(ph)) {
            if (ts.v == t1.v) return false;
            if (t1.hi > tmax) return false;
            ts = t1;
            ph = o + d * ts.v;
            scale = sp.radius / length(ph);
            ph = F3{ph.x * scale, ph.y * scale, ph.z * scale};
            if (ph.x == 0 && ph.y == 0) ph.x = 1e-5f * sp.radius;
            if (clipped(ph)) return false;
        }
    }
    *t_hit = ts.v;
    *obj_d = d;
    *phit = ph;
    return true;
}

// What shading needs of a SurfaceInteraction (core/interaction.h)
struct Isect {
    F3 p, perr, n, wo, sn, sdpdu;
    // texture lookups (triangles): the hit's (u, v) and dp/du, dp/dv; dead code where no texture is read
    float u, v;
    F3 dpdu, dpdv;
    // bump mapping: shading.dpdv, shading.dndu / dndv, reverseOrientation ^ transformSwapsHandedness
    F3 sdpdv, dndu, dndv;
    bool flip;
};

// Sphere::Intersect's interaction + Transform::operator()(SurfaceInteraction)
// (sphere.cpp:104-155, interaction.cpp:44-70, transform.cpp:262-297)
template <bool DIFFS = false>
DEV void sphere_interaction(const DSphere &sp, F3 obj_d, F3 ph, Isect *is) {
    float theta = acos_f(clampf(ph.z / sp.radius, -1, 1));
    float z_radius = sqrtf(ph.x * ph.x + ph.y * ph.y);
    float inv_z_radius = 1 / z_radius;
    float cos_phi = ph.x * inv_z_radius;
    float sin_phi = ph.y * inv_z_radius;
    float st, ct;
    sincos_f(theta, &st, &ct);
    F3 dpdu = F3{-sp.phi_max * ph.y, sp.phi_max * ph.x, 0};
    F3 dpdv = (sp.theta_max - sp.theta_min) * F3{ph.z * cos_phi, ph.z * sin_phi, -sp.radius * st};
    F3 perr = kGamma5 * vabs(ph);
    F3 n = normalize(cross(dpdu, dpdv));
    F3 sn = n;
    if (sp.reverse_orientation ^ sp.swaps_handedness) {
        n = n * -1.f;
        sn = sn * -1.f;
    }
    F3 wo = normalize(-obj_d);
    is->p = xf_point_err2(sp.o2w, ph, perr, &is->perr);
    is->n = normalize(xf_normal(sp.o2w_inv, n));
    is->wo = normalize(xf_vector(sp.o2w, wo));
    F3 snw = normalize(xf_normal(sp.o2w_inv, sn));
    is->sdpdu = xf_vector(sp.o2w, dpdu);
    is->sn = faceforward(snw, is->n);
    if (DIFFS) {
        // what the direct pass's reflected-ray differentials need of a sphere hit (directprogressiveintegrator.cpp:165-184):
        // dpdu / dpdv for ComputeDifferentials and dndu / dndv from the fundamental forms (sphere.cpp:122-143), in world space
        // (transform.cpp:275-283: vectors by the matrix, Normal3f by the inverse transpose)
        const float dt = sp.theta_max - sp.theta_min;
        const F3 d2Pduu = (-sp.phi_max * sp.phi_max) * F3{ph.x, ph.y, 0};
        const F3 d2Pduv = (dt * ph.z * sp.phi_max) * F3{-sin_phi, cos_phi, 0.f};
        const F3 d2Pdvv = (-dt * dt) * F3{ph.x, ph.y, ph.z};
        const float E = dot(dpdu, dpdu), F = dot(dpdu, dpdv), G = dot(dpdv, dpdv);
        const F3 N = normalize(cross(dpdu, dpdv));
        const float e = dot(N, d2Pduu), f = dot(N, d2Pduv), g = dot(N, d2Pdvv);
        const float inv_egf2 = 1 / (E * G - F * F);
        const F3 dndu = ((f * F - e * G) * inv_egf2) * dpdu + ((e * F - f * E) * inv_egf2) * dpdv;
        const F3 dndv = ((g * F - f * G) * inv_egf2) * dpdu + ((f * F - g * E) * inv_egf2) * dpdv;
        is->dpdu = is->sdpdu;
        is->dpdv = is->sdpdv = xf_vector(sp.o2w, dpdv);
        is->dndu = xf_normal(sp.o2w_inv, dndu);
        is->dndv = xf_normal(sp.o2w_inv, dndv);
        // Point2f(u, v) of the hit (sphere.cpp:107-109); phi as Sphere::Intersect computes it from the refined hit point
        float phi = atan2_f(ph.y, ph.x);
        if (phi < 0) phi += 2 * kPi;
        is->u = phi / sp.phi_max;
        is->v = (theta - sp.theta_min) / (sp.theta_max - sp.theta_min);
        is->flip = sp.reverse_orientation ^ sp.swaps_handedness;
    }
}

// ===========================================================================
// Disk and cylinder (shapes/disk.cpp, shapes/cylinder.cpp)
// ===========================================================================
// Disk::Intersect / IntersectP up to the hit decision (disk.cpp:48-71, :99-122: the plane test, no error bounds) and
// Cylinder::Intersect / IntersectP (cylinder.cpp:48-103, :146-201: the EFloat quadratic, the refined hit, the clipping
// branch with its second root). Outputs the object-space ray direction and the refined hit point for quadric_interaction.
DEV bool quadric_test(const DQuadric &q, F3 ro, F3 rd, float tmax, float *t_hit, F3 *obj_d, F3 *phit) {
    F3 oerr, derr;
    F3 o = xf_point_err(q.o2w_inv, ro, &oerr);
    F3 d = xf_vector_err(q.o2w_inv, rd, &derr);
    float len2 = length_sq(d);
    if (len2 > 0) {  // transform.h:382-394 (tMax unchanged)
        float dt = dot(vabs(d), oerr) / len2;
        o = o + d * dt;
    }
    if (q.kind == kQuadricDisk) {
        if (d.z == 0) return false;  // disk.cpp:58-60
        const float ts = (q.height - o.z) / d.z;
        if (ts <= 0 || ts >= tmax) return false;
        F3 ph = o + d * ts;  // :63-71
        const float dist2 = ph.x * ph.x + ph.y * ph.y;
        if (dist2 > q.radius * q.radius || dist2 < q.inner_radius * q.inner_radius) return false;
        float phi = atan2_f(ph.y, ph.x);
        if (phi < 0) phi += 2 * kPi;
        if (phi > q.phi_max) return false;
        ph.z = q.height;  // :84, refined hit point
        *t_hit = ts;
        *obj_d = d;
        *phit = ph;
        return true;
    }
    EF ox = ef(o.x, oerr.x), oy = ef(o.y, oerr.y);
    EF dx = ef(d.x, derr.x), dy = ef(d.y, derr.y);
    EF a = dx * dx + dy * dy;  // cylinder.cpp:60-64
    EF b = ef(2.f) * (dx * ox + dy * oy);
    EF c = ox * ox + oy * oy - ef(q.radius) * ef(q.radius);
    EF t0, t1;
    if (!ef_quadratic(a, b, c, &t0, &t1)) return false;
    if (t0.hi > tmax || t1.lo <= 0) return false;  // :71-76
    EF ts = t0;
    if (ts.lo <= 0) {
        ts = t1;
        if (ts.hi > tmax) return false;
    }
    // hit point refined onto the cylinder, and its phi (:79-86)
    auto refined = [&](float t, float *phi) {
        F3 p = o + d * t;
        const float hit_rad = sqrtf(p.x * p.x + p.y * p.y);
        p.x *= q.radius / hit_rad;
        p.y *= q.radius / hit_rad;
        *phi = atan2_f(p.y, p.x);
        if (*phi < 0) *phi += 2 * kPi;
        return p;
    };
    float phi;
    F3 ph = refined(ts.v, &phi);
    if (ph.z < q.zmin || ph.z > q.zmax || phi > q.phi_max) {  // :89-103
        if (ts.v == t1.v) return false;
        ts = t1;
        if (t1.hi > tmax) return false;
        ph = refined(ts.v, &phi);
        if (ph.z < q.zmin || ph.z > q.zmax || phi > q.phi_max) return false;
    }
    *t_hit = ts.v;
    *obj_d = d;
    *phit = ph;
    return true;
}

// The SurfaceInteraction of a disk hit (disk.cpp:73-92: zero normal derivatives, zero error bounds) or a cylinder hit
// (cylinder.cpp:105-139: dn/du from the fundamental forms, pError = gamma(3) |(x, y, 0)|), through the SurfaceInteraction
// constructor (interaction.cpp:19-42) and Transform::operator()(SurfaceInteraction) (transform.cpp:262-297), as
// sphere_interaction. (With these dp/du, dp/dv the disk's geometric normal is -z in object space, while Disk::Sample gives
// +z: disk.cpp:78-80 and :133. Reproduced as it is.)
template <bool DIFFS = false>
DEV void quadric_interaction(const DQuadric &q, F3 obj_d, F3 ph, Isect *is) {
    float phi = atan2_f(ph.y, ph.x);
    if (phi < 0) phi += 2 * kPi;
    const float u = phi / q.phi_max;
    float v;
    F3 dpdu = F3{-q.phi_max * ph.y, q.phi_max * ph.x, 0};
    F3 dpdv, perr, dndu = F3{0, 0, 0}, dndv = F3{0, 0, 0};
    if (q.kind == kQuadricDisk) {
        const float r_hit = sqrtf(ph.x * ph.x + ph.y * ph.y);
        const float one_minus_v = ((r_hit - q.inner_radius) / (q.radius - q.inner_radius));
        v = 1 - one_minus_v;
        const float dr = q.radius - q.inner_radius, inv_r = 1 / r_hit;  // Vector3f / Float multiplies by the reciprocal
        dpdv = F3{(ph.x * dr) * inv_r, (ph.y * dr) * inv_r, (0.f * dr) * inv_r};
        perr = F3{0, 0, 0};
    } else {
        v = (ph.z - q.zmin) / (q.zmax - q.zmin);
        dpdv = F3{0, 0, q.zmax - q.zmin};
        if (DIFFS) {
            const F3 d2Pduu = (-q.phi_max * q.phi_max) * F3{ph.x, ph.y, 0};
            const float E = dot(dpdu, dpdu), F = dot(dpdu, dpdv), G = dot(dpdv, dpdv);
            const F3 N = normalize(cross(dpdu, dpdv));
            const float e = dot(N, d2Pduu), f = dot(N, F3{0, 0, 0}), g = dot(N, F3{0, 0, 0});
            const float inv_egf2 = 1 / (E * G - F * F);
            dndu = ((f * F - e * G) * inv_egf2) * dpdu + ((e * F - f * E) * inv_egf2) * dpdv;
            dndv = ((g * F - f * G) * inv_egf2) * dpdu + ((f * F - g * E) * inv_egf2) * dpdv;
        }
        perr = kGamma3 * vabs(F3{ph.x, ph.y, 0});
    }
    F3 n = normalize(cross(dpdu, dpdv));
    F3 sn = n;
    if (q.reverse_orientation ^ q.swaps_handedness) {
        n = n * -1.f;
        sn = sn * -1.f;
    }
    F3 wo = normalize(-obj_d);
    is->p = xf_point_err2(q.o2w, ph, perr, &is->perr);
    is->n = normalize(xf_normal(q.o2w_inv, n));
    is->wo = normalize(xf_vector(q.o2w, wo));
    F3 snw = normalize(xf_normal(q.o2w_inv, sn));
    is->sdpdu = xf_vector(q.o2w, dpdu);
    is->sn = faceforward(snw, is->n);
    if (DIFFS) {  // (u, v), dp/dv and dn/du, dn/dv for texture lookups, Material::Bump and the direct pass's differentials
        is->dpdu = is->sdpdu;
        is->dpdv = is->sdpdv = xf_vector(q.o2w, dpdv);
        is->dndu = xf_normal(q.o2w_inv, dndu);
        is->dndv = xf_normal(q.o2w_inv, dndv);
        is->u = u;
        is->v = v;
        is->flip = q.reverse_orientation ^ q.swaps_handedness;
    }
}

// The SurfaceInteraction of a closest hit on a sphere or a quadric, `shape` being the primitive's device prim_shape (>= 0: a
// sphere, ~index: a quadric): the shape's deterministic root selection is redone on the same ray at tMax = inf for the
// object-space ray and the refined hit point (every tMax-dependent branch of either test is a rejection). QUAD = false: a build
// that never sees a quadric (k_shade's plain build: a scene with quadrics runs the extended one)
template <bool DIFFS = false, bool QUAD = true>
DEV void shape_hit_interaction(const DScene &S, int shape, F3 ro, F3 rd, Isect *is) {
    float t;
    F3 od, ph;
    if (QUAD && shape < 0) {
        const DQuadric &q = S.quadrics[~shape];
        quadric_test(q, ro, rd, IILE_INF, &t, &od, &ph);
        quadric_interaction<DIFFS>(q, od, ph, is);
    } else {
        const DSphere &sp = S.spheres[shape];
        sphere_test(sp, ro, rd, IILE_INF, &t, &od, &ph);
        sphere_interaction<DIFFS>(sp, od, ph, is);
    }
}

// Triangle::Intersect's interaction (triangle.cpp:277-400) from the stored
// barycentrics of the closest hit.
DEV void triangle_interaction(const DScene &S, int prim, uint32_t flags, F3 p0, F3 p1, F3 p2, F3 ray_d, float b0,
                              float b1, float b2, Isect *is) {
    float uv00 = 0, uv01 = 0, uv10 = 1, uv11 = 0, uv20 = 1, uv21 = 1;  // triangle.h:98-108
    if (flags & 4u) {
        const float2 *u = S.tri_uv + 3 * size_t(prim);
        float2 a = u[0], b = u[1], c = u[2];
        uv00 = a.x;
        uv01 = a.y;
        uv10 = b.x;
        uv11 = b.y;
        uv20 = c.x;
        uv21 = c.y;
    }
    float duv02x = uv00 - uv20, duv02y = uv01 - uv21;
    float duv12x = uv10 - uv20, duv12y = uv11 - uv21;
    F3 dp02 = p0 - p2, dp12 = p1 - p2;
    float determinant = duv02x * duv12y - duv02y * duv12x;
    bool degenerate = double(fabsf(determinant)) < 1e-8;
    F3 dpdu = F3{0, 0, 0}, dpdv = F3{0, 0, 0};
    if (!degenerate) {
        float invdet = 1 / determinant;
        dpdu = (duv12y * dp02 - duv02y * dp12) * invdet;
        dpdv = (-duv12x * dp02 + duv02x * dp12) * invdet;
    }
    if (degenerate || length_sq(cross(dpdu, dpdv)) == 0)
        coordinate_system(normalize(cross(p2 - p0, p1 - p0)), &dpdu, &dpdv);
    float xs = (fabsf(b0 * p0.x) + fabsf(b1 * p1.x) + fabsf(b2 * p2.x));
    float ys = (fabsf(b0 * p0.y) + fabsf(b1 * p1.y) + fabsf(b2 * p2.y));
    float zs = (fabsf(b0 * p0.z) + fabsf(b1 * p1.z) + fabsf(b2 * p2.z));
    is->perr = kGamma7 * F3{xs, ys, zs};
    is->p = b0 * p0 + b1 * p1 + b2 * p2;
    is->u = b0 * uv00 + b1 * uv10 + b2 * uv20;  // uvHit, triangle.cpp:318
    is->v = b0 * uv01 + b1 * uv11 + b2 * uv21;
    is->dpdu = dpdu;
    is->dpdv = dpdv;
    is->wo = normalize(-ray_d);
    F3 n = normalize(cross(dp02, dp12));
    const bool flip = (flags & 8u) != 0;
    if (flags & 2u) {
        const float4 *nn = S.tri_norms + 3 * size_t(prim);
        float4 a = nn[0], b = nn[1], c = nn[2];
        F3 n0 = F3{a.x, a.y, a.z}, n1 = F3{b.x, b.y, b.z}, n2 = F3{c.x, c.y, c.z};
        F3 ns = (b0 * n0 + b1 * n1 + b2 * n2);
        if (length_sq(ns) > 0)
            ns = normalize(ns);
        else
            ns = n;
        F3 ss = normalize(dpdu);
        F3 ts = cross(ss, ns);
        if (length_sq(ts) > 0.f) {
            ts = normalize(ts);
            ss = cross(ts, ns);
        } else
            coordinate_system(ns, &ss, &ts);
        // dndu, dndv of the interpolated normal, triangle.cpp:374-392
        const F3 dn1 = n0 - n2, dn2 = n1 - n2;
        if (double(fabsf(determinant)) < 1e-8) {
            is->dndu = is->dndv = F3{0, 0, 0};
        } else {
            const float inv_det = 1 / determinant;
            is->dndu = (duv12y * dn1 - duv02y * dn2) * inv_det;
            is->dndv = (-duv12x * dn1 + duv02x * dn2) * inv_det;
        }
        F3 sn = normalize(cross(ss, ts));  // SetShadingGeometry, interaction.cpp:72-92
        if (flip) sn = -sn;
        n = faceforward(n, sn);
        is->sn = sn;
        is->sdpdu = ss;
        is->sdpdv = ts;
    } else {
        if (flip) n = -n;
        is->sn = n;
        is->sdpdu = dpdu;
        is->sdpdv = dpdv;
        is->dndu = is->dndv = F3{0, 0, 0};
    }
    is->flip = flip;
    is->n = n;
}

#include "dtrav.h"  // BVH traversal

// ===========================================================================
// BSDF (core/reflection.{h,cpp}, core/microfacet.cpp)
// ===========================================================================
struct Bsdf {
    F3 ns, ng, ss, ts;
    F3 kd, ks, kr, kt;
    float alpha, eta;
    float alpha_y;  // TrowbridgeReitzDistribution(alphax = alpha, alphay): uber's / glass's "vroughness"; the same value as alpha otherwise
    // UberMaterial's SpecularTransmission lobes (uber.cpp:53-61, 94-99): the pass-through of a surface that is not opaque —
    // SpecularTransmission(t0 = 1 - opacity, 1, 1), the FIRST lobe — and SpecularTransmission(kt = opacity Kt, 1, eta), the LAST;
    // path_eta = BSDF::eta (1 with the pass-through, else the material's: path.cpp:151-157 reads it)
    F3 t0;
    bool has_t0, has_t1;
    float path_eta;
    // rough glass (glass.cpp:66-90): MicrofacetReflection(kr -> ks, FresnelDielectric(1, eta)) is the microfacet lobe;
    // MicrofacetTransmission(kt, distrib, 1, eta, Radiance) — glossy, not specular
    bool has_mtrans;
    int n_lobes;  // nBxDFs; BxDF order: [pass-through], Lambertian, [Lambertian transmission], microfacet, specular reflection, [uber's Kt lobe]
    float on_a, on_b;  // Oren-Nayar constants of the diffuse lobe (oren_nayar set)
    bool oren_nayar;
    int mtype;    // kMat*: selects the Fresnel terms (plastic 1.5/1; uber 1/eta; mirror none; metal FresnelConductor(1, kr, kt))
                  // and, for glass, makes the specular lobe a FresnelSpecular(kr, kt, 1, eta)
    bool has_lambert, has_micro, has_spec;
    // metal (metal.cpp:58-79): the microfacet lobe is MicrofacetReflection(1, distrib, FresnelConductor(1, eta, k)), its eta and k
    // held in kr and kt (a metal has no specular lobe that would read them: has_spec is false)
    // substrate (substrate.cpp:45-66): FresnelBlend(Rd = kd, Rs = ks, distrib) — glossy reflection, the only lobe of its BSDF
    bool has_blend;
    // translucent (translucent.cpp:45-80): LambertianReflection(r kd) is the Lambertian lobe; LambertianTransmission(t kd), its T held
    // in kr (translucent has no specular lobe that would read it), comes next; MicrofacetReflection(r ks, FresnelDielectric(1, 1.5)) is
    // the microfacet lobe and MicrofacetTransmission(t ks, distrib, 1, 1.5) rough glass's
    bool has_ltrans;
};
DEV int n_nonspec(const Bsdf &b) {
    return (b.has_lambert ? 1 : 0) + (b.has_ltrans ? 1 : 0) + (b.has_micro ? 1 : 0) + (b.has_mtrans ? 1 : 0) + (b.has_blend ? 1 : 0);
}
DEV F3 to_local(const Bsdf &b, F3 v) { return F3{dot(v, b.ss), dot(v, b.ts), dot(v, b.ns)}; }
DEV F3 to_world(const Bsdf &b, F3 v) {
    return F3{b.ss.x * v.x + b.ts.x * v.y + b.ns.x * v.z, b.ss.y * v.x + b.ts.y * v.y + b.ns.y * v.z,
              b.ss.z * v.x + b.ts.z * v.y + b.ns.z * v.z};
}
// ===========================================================================
// image textures: SurfaceInteraction::ComputeDifferentials (interaction.cpp:103-149),
// UVMapping2D::Map (texture.cpp:93-99), MIPMap<RGBSpectrum>::Lookup / triangle / EWA / Texel
// (mipmap.h:210-355) over the host-built pyramid — operation for operation as the oracle's tex_* functions
// ===========================================================================
DEV bool solve_2x2(float a00, float a01, float a10, float a11, float b0, float b1, float *x0, float *x1) {  // transform.cpp:41-49
    const float det = a00 * a11 - a01 * a10;
    if (fabsf(det) < 1e-10f) return false;
    *x0 = (a11 * b0 - a01 * b1) / det;
    *x1 = (a00 * b1 - a10 * b0) / det;
    if (*x0 != *x0 || *x1 != *x1) return false;
    return true;
}
DEV bool is_inf_or_nan(float v) { return !(fabsf(v) < IILE_INF); }
// (dpdx / dpdy, interaction.cpp:117-118 — zero when the auxiliary rays miss the tangent plane —, are what the direct pass's
//  reflected-ray differentials start from; every other caller leaves them out)
DEV TexDiff compute_differentials(const Isect &is, const RayDiff &rd, F3 *dpdx = nullptr, F3 *dpdy = nullptr) {
    TexDiff t = TexDiff{0, 0, 0, 0};
    if (dpdx) *dpdx = *dpdy = F3{0, 0, 0};
    const F3 n = is.n, p = is.p;
    const float d = dot(n, p);
    const float tx = -(dot(n, rd.rxo) - d) / dot(n, rd.rxd);
    if (is_inf_or_nan(tx)) return t;
    const F3 px = rd.rxo + tx * rd.rxd;
    const float ty = -(dot(n, rd.ryo) - d) / dot(n, rd.ryd);
    if (is_inf_or_nan(ty)) return t;
    const F3 py = rd.ryo + ty * rd.ryd;
    if (dpdx) *dpdx = px - p, *dpdy = py - p;
    int d0, d1;
    if (fabsf(n.x) > fabsf(n.y) && fabsf(n.x) > fabsf(n.z)) {
        d0 = 1;
        d1 = 2;
    } else if (fabsf(n.y) > fabsf(n.z)) {
        d0 = 0;
        d1 = 2;
    } else {
        d0 = 0;
        d1 = 1;
    }
    const float a00 = comp(is.dpdu, d0), a01 = comp(is.dpdv, d0), a10 = comp(is.dpdu, d1), a11 = comp(is.dpdv, d1);
    const float bx0 = comp(px, d0) - comp(p, d0), bx1 = comp(px, d1) - comp(p, d1);
    const float by0 = comp(py, d0) - comp(p, d0), by1 = comp(py, d1) - comp(p, d1);
    if (!solve_2x2(a00, a01, a10, a11, bx0, bx1, &t.dudx, &t.dvdx)) t.dudx = t.dvdx = 0;
    if (!solve_2x2(a00, a01, a10, a11, by0, by1, &t.dudy, &t.dvdy)) t.dudy = t.dvdy = 0;
    return t;
}
DEV int mod_i(int a, int b) {  // pbrt.h:310-314
    const int r = a - (a / b) * b;
    return r < 0 ? r + b : r;
}
DEV F3 tex_texel(const DScene &S, const DTexture &t, int level, int s, int tt) {
    const int w = t.level_w[level], h = t.level_h[level];
    if (t.wrap == kWrapRepeat) {
        // level sizes are powers of two: Mod is a mask (two's complement handles negative s)
        s = s & (w - 1);
        tt = tt & (h - 1);
    } else if (t.wrap == kWrapClamp) {
        s = s < 0 ? 0 : (s > w - 1 ? w - 1 : s);
        tt = tt < 0 ? 0 : (tt > h - 1 ? h - 1 : tt);
    } else if (s < 0 || s >= w || tt < 0 || tt >= h) {
        return F3{0, 0, 0};
    }
    const float4 c = S.texels[t.level_offset[level] + (long long)tt * w + s];
    return F3{c.x, c.y, c.z};
}
DEV F3 tex_triangle(const DScene &S, const DTexture &t, int level, float st0, float st1) {
    level = level < 0 ? 0 : (level > t.n_levels - 1 ? t.n_levels - 1 : level);
    const float s = st0 * float(t.level_w[level]) - 0.5f;
    const float tt = st1 * float(t.level_h[level]) - 0.5f;
    const float fs = floorf(s), ft = floorf(tt);
    const int s0 = int(fs), t0 = int(ft);
    const float ds = s - float(s0), dt = tt - float(t0);
    return tex_texel(S, t, level, s0, t0) * ((1 - ds) * (1 - dt)) + tex_texel(S, t, level, s0, t0 + 1) * ((1 - ds) * dt) +
           tex_texel(S, t, level, s0 + 1, t0) * (ds * (1 - dt)) + tex_texel(S, t, level, s0 + 1, t0 + 1) * (ds * dt);
}
DEV F3 lerp_f3(float t, F3 a, F3 b) { return a * (1 - t) + b * t; }
DEV F3 tex_lookup_width(const DScene &S, const DTexture &t, float st0, float st1, float width) {  // mipmap.h:233-250
    const float level = float(t.n_levels - 1) + log2_f(mx(width, 1e-8f));
    if (level < 0) return tex_triangle(S, t, 0, st0, st1);
    if (level >= float(t.n_levels - 1)) return tex_texel(S, t, t.n_levels - 1, 0, 0);
    const int il = int(floorf(level));
    const float delta = level - float(il);
    return lerp_f3(delta, tex_triangle(S, t, il, st0, st1), tex_triangle(S, t, il + 1, st0, st1));
}
DEV F3 tex_ewa(const DScene &S, const DTexture &t, int level, float st0, float st1, float d00, float d01, float d10, float d11) {
    if (level >= t.n_levels) return tex_texel(S, t, t.n_levels - 1, 0, 0);
    const float w = float(t.level_w[level]), h = float(t.level_h[level]);
    st0 = st0 * w - 0.5f;
    st1 = st1 * h - 0.5f;
    d00 *= w;
    d01 *= h;
    d10 *= w;
    d11 *= h;
    float A = d01 * d01 + d11 * d11 + 1;
    float B = -2 * (d00 * d01 + d10 * d11);
    float C = d00 * d00 + d10 * d10 + 1;
    const float invF = 1 / (A * C - B * B * 0.25f);
    A *= invF;
    B *= invF;
    C *= invF;
    const float det = -B * B + 4 * A * C;
    const float inv_det = 1 / det;
    const float u_sqrt = sqrtf(det * C), v_sqrt = sqrtf(A * det);
    const int s0 = int(ceilf(st0 - 2 * inv_det * u_sqrt));
    const int s1 = int(floorf(st0 + 2 * inv_det * u_sqrt));
    const int t0 = int(ceilf(st1 - 2 * inv_det * v_sqrt));
    const int t1 = int(floorf(st1 + 2 * inv_det * v_sqrt));
    F3 sum = F3{0, 0, 0};
    float sum_wts = 0;
    for (int it = t0; it <= t1; ++it) {
        const float tt = float(it) - st1;
        for (int is = s0; is <= s1; ++is) {
            const float ss = float(is) - st0;
            const float r2 = A * ss * ss + B * ss * tt + C * tt * tt;
            if (r2 < 1) {
                int index = int(r2 * 128.f);
                index = index < 127 ? index : 127;
                const float weight = S.ewa_lut[index];
                sum = sum + tex_texel(S, t, level, is, it) * weight;
                sum_wts += weight;
            }
        }
    }
    return F3{sum.x / sum_wts, sum.y / sum_wts, sum.z / sum_wts};
}
DEV F3 tex_image(const DScene &S, int tex, float u, float v, const TexDiff &td) {
    const DTexture &t = S.textures[tex];
    float d00 = t.su * td.dudx, d01 = t.sv * td.dvdx, d10 = t.su * td.dudy, d11 = t.sv * td.dvdy;
    const float st0 = t.su * u + t.du, st1 = t.sv * v + t.dv;
    if (t.trilinear) {
        const float width = mx(mx(fabsf(d00), fabsf(d01)), mx(fabsf(d10), fabsf(d11)));
        return tex_lookup_width(S, t, st0, st1, 2 * width);
    }
    if (d00 * d00 + d01 * d01 < d10 * d10 + d11 * d11) {
        float tmp = d00;
        d00 = d10;
        d10 = tmp;
        tmp = d01;
        d01 = d11;
        d11 = tmp;
    }
    const float major = sqrtf(d00 * d00 + d01 * d01);
    float minor = sqrtf(d10 * d10 + d11 * d11);
    if (minor * t.max_aniso < major && minor > 0) {
        const float scale = major / (minor * t.max_aniso);
        d10 *= scale;
        d11 *= scale;
        minor *= scale;
    }
    if (minor == 0) return tex_triangle(S, t, 0, st0, st1);
    const float lod = mx(0.f, float(t.n_levels) - 1.f + log2_f(minor));
    const int ilod = int(floorf(lod));
    return lerp_f3(lod - float(ilod), tex_ewa(S, t, ilod, st0, st1, d00, d01, d10, d11),
                   tex_ewa(S, t, ilod + 1, st0, st1, d00, d01, d10, d11));
}
// ===========================================================================
// procedural textures (src/textures/checkerboard.h, uv.h, bilerp.h, scale.h, mix.h) over the mappings of src/core/texture.cpp.
// No recursion and no runtime-indexed arrays: a combiner (scale, mix, a checkerboard with a non-constant input) evaluates its
// inputs, each a leaf (an image, uv, bilerp, a checkerboard of constants), into named registers (the loader and the upload keep
// trees to these two levels)
// ===========================================================================
// (s, t) and its differentials: TextureMapping2D::Map
struct TexSt {
    float s, t, dsdx, dtdx, dsdy, dtdy;
};
DEV F3 tex_xf_point(const DTexture &t, F3 p) {  // Transform::operator()(Point3f) of an affine 3 x 4 (transform.h:217-232)
    return F3{t.xf[0] * p.x + t.xf[1] * p.y + t.xf[2] * p.z + t.xf[3], t.xf[4] * p.x + t.xf[5] * p.y + t.xf[6] * p.z + t.xf[7],
              t.xf[8] * p.x + t.xf[9] * p.y + t.xf[10] * p.z + t.xf[11]};
}
// SphericalMapping2D::sphere / CylindricalMapping2D::cylinder (texture.cpp:119-123, texture.h:92-95)
DEV void tex_sph_cyl(const DTexture &t, bool sph, F3 p, float *s, float *tt) {
    const F3 vec = normalize(tex_xf_point(t, p));
    const float phi = atan2_f(vec.y, vec.x);
    if (sph) {
        const float theta = acos_f(clampf(vec.z, -1, 1));  // SphericalTheta, SphericalPhi (geometry.h)
        *s = theta * kInvPi;
        *tt = (phi < 0 ? phi + 2 * kPi : phi) * kInv2Pi;
    } else {
        *s = (kPi + phi) * kInv2Pi;
        *tt = vec.z;
    }
}
DEV float tex_wrap_dt(float d) {  // the sphere / cylinder mapping's discontinuity fix-up of dt (texture.cpp:108-116, 133-141)
    if (d > .5f) return 1.f - d;
    if (d < -.5f) return -(d + 1);
    return d;
}
// diffs: whether the differentials are wanted (only the closed-form checkerboard reads them)
DEV TexSt tex_map2d(const DTexture &t, const TexCtx &c, bool diffs) {
    TexSt r = TexSt{0, 0, 0, 0, 0, 0};
    if (t.mapping == kMapUV) {  // UVMapping2D::Map, texture.cpp:93-99
        r.dsdx = t.su * c.td.dudx, r.dtdx = t.sv * c.td.dvdx;
        r.dsdy = t.su * c.td.dudy, r.dtdy = t.sv * c.td.dvdy;
        r.s = t.su * c.u + t.du, r.t = t.sv * c.v + t.dv;
    } else if (t.mapping == kMapPlanar) {  // PlanarMapping2D::Map, texture.cpp:147-153
        const F3 vs = F3{t.vs[0], t.vs[1], t.vs[2]}, vt = F3{t.vt[0], t.vt[1], t.vt[2]};
        r.dsdx = dot(c.dpdx, vs), r.dtdx = dot(c.dpdx, vt);
        r.dsdy = dot(c.dpdy, vs), r.dtdy = dot(c.dpdy, vt);
        r.s = t.du + dot(c.p, vs), r.t = t.dv + dot(c.p, vt);
    } else {  // SphericalMapping2D::Map (delta .1), CylindricalMapping2D::Map (delta .01), texture.cpp:101-145
        const bool sph = t.mapping == kMapSpherical;
        const float delta = sph ? .1f : .01f;
        // one copy of the mapping for the point and its two offsets
#pragma nounroll
        for (int k = 0; k < (diffs ? 3 : 1); ++k) {
            const F3 q = k == 0 ? c.p : c.p + delta * (k == 1 ? c.dpdx : c.dpdy);
            float s, tt;
            tex_sph_cyl(t, sph, q, &s, &tt);
            if (k == 0)
                r.s = s, r.t = tt;
            else if (k == 1)
                r.dsdx = s, r.dtdx = tt;
            else
                r.dsdy = s, r.dtdy = tt;
        }
        if (diffs) {
            const float inv = 1 / delta;  // Vector2f::operator/
            r.dsdx = (r.dsdx - r.s) * inv, r.dtdx = tex_wrap_dt((r.dtdx - r.t) * inv);
            r.dsdy = (r.dsdy - r.s) * inv, r.dtdy = tex_wrap_dt((r.dtdy - r.t) * inv);
        }
    }
    return r;
}
// Checkerboard2DTexture / Checkerboard3DTexture::Evaluate (checkerboard.h:65-103, 117-127) short of the lookups of tex1 / tex2:
// 0 or 1: tex1 or tex2 alone; 2: (1 - *area2) * tex1 + *area2 * tex2. st: the 2D mapping (with differentials for the closed form)
DEV int tex_checker(const DTexture &t, const TexCtx &c, const TexSt &st, float *area2) {
    if (t.kind == kTexChecker3D) {  // IdentityMapping3D::Map (texture.cpp:155-160)
        const F3 q = tex_xf_point(t, c.p);
        return (int(floorf(q.x)) + int(floorf(q.y)) + int(floorf(q.z))) % 2 == 0 ? 0 : 1;
    }
    if (t.aamode == kAANone) return (int(floorf(st.s)) + int(floorf(st.t))) % 2 == 0 ? 0 : 1;
    const float ds = mx(fabsf(st.dsdx), fabsf(st.dsdy)), dt = mx(fabsf(st.dtdx), fabsf(st.dtdy));
    const float s0 = st.s - ds, s1 = st.s + ds, t0 = st.t - dt, t1 = st.t + dt;
    if (floorf(s0) == floorf(s1) && floorf(t0) == floorf(t1)) return (int(floorf(st.s)) + int(floorf(st.t))) % 2 == 0 ? 0 : 1;
    auto bump_int = [](float x) { return float(int(floorf(x / 2))) + 2 * mx(x / 2 - float(int(floorf(x / 2))) - .5f, 0.f); };
    const float sint = (bump_int(s1) - bump_int(s0)) / (2 * ds), tint = (bump_int(t1) - bump_int(t0)) / (2 * dt);
    float a2 = sint + tint - 2 * sint * tint;
    if (ds > 1 || dt > 1) a2 = .5f;
    *area2 = a2;
    return 2;
}
DEV F3 tex_blend(float a2, F3 a, F3 b) {  // (1 - area2) * tex1 + area2 * tex2
    return F3{(1 - a2) * a.x + a2 * b.x, (1 - a2) * a.y + a2 * b.y, (1 - a2) * a.z + a2 * b.z};
}
DEV F3 tex_cval(const DTexture &t, int k) { return F3{t.cval[k][0], t.cval[k][1], t.cval[k][2]}; }
// a leaf that is not an image: uv (UVTexture, uv.h:54-60), bilerp (BilerpTexture, bilerp.h:56-62), a checkerboard of constants
DEV F3 tex_proc_leaf(const DTexture &t, const TexCtx &c) {
    TexSt st = TexSt{0, 0, 0, 0, 0, 0};
    if (t.kind != kTexChecker3D) st = tex_map2d(t, c, t.kind == kTexChecker2D && t.aamode == kAAClosedForm);
    if (t.kind == kTexUV) return F3{st.s - floorf(st.s), st.t - floorf(st.t), 0};
    if (t.kind == kTexBilerp) {
        const float a = (1 - st.s) * (1 - st.t), b = (1 - st.s) * st.t, d = st.s * (1 - st.t), e = st.s * st.t;
        return F3{a * t.bilerp[0][0] + b * t.bilerp[1][0] + d * t.bilerp[2][0] + e * t.bilerp[3][0],
                  a * t.bilerp[0][1] + b * t.bilerp[1][1] + d * t.bilerp[2][1] + e * t.bilerp[3][1],
                  a * t.bilerp[0][2] + b * t.bilerp[1][2] + d * t.bilerp[2][2] + e * t.bilerp[3][2]};
    }
    float a2 = 0;
    const int sel = tex_checker(t, c, st, &a2);
    return sel == 0 ? tex_cval(t, 0) : (sel == 1 ? tex_cval(t, 1) : tex_blend(a2, tex_cval(t, 0), tex_cval(t, 1)));
}
DEV F3 tex_leaf(const DScene &S, int tex, const TexCtx &c) {
    const DTexture &t = S.textures[tex];
    if (t.kind == kTexImage) return tex_image(S, tex, c.u, c.v, c.td);
    return tex_proc_leaf(t, c);
}
// a procedural texture (kind != kTexImage)
DEV F3 tex_procedural(const DScene &S, int tex, const TexCtx &c) {
    const DTexture &t = S.textures[tex];
    const bool checker = t.kind == kTexChecker2D || t.kind == kTexChecker3D;
    const bool combiner = t.kind == kTexScale || t.kind == kTexMix || (checker && (t.child[0] >= 0 || t.child[1] >= 0));
    if (!combiner) return tex_leaf(S, tex, c);
    // the combination as a sum (mix, checkerboard: w0 * in0 + w1 * in1, the inputs a checkerboard does not select left out, as
    // Evaluate leaves them) or a product (scale: in0 * in1), accumulated input by input: the same roundings as the reference's
    // expressions (0 + x and 1 * x are exact), with one value held instead of three
    float w0 = 1, w1 = 1;
    int need = 3;
    if (checker) {
        TexSt st = TexSt{0, 0, 0, 0, 0, 0};
        if (t.kind == kTexChecker2D) st = tex_map2d(t, c, t.aamode == kAAClosedForm);
        float a2 = 0;
        const int sel = tex_checker(t, c, st, &a2);
        if (sel == 2)
            w0 = 1 - a2, w1 = a2;
        else
            need = 1 << sel;
    }
    const bool prod = t.kind == kTexScale;  // ScaleTexture, scale.h:56-58
    F3 acc = prod ? F3{1, 1, 1} : F3{0, 0, 0};
    // MixTexture (mix.h:57-61): (1 - amt) * tex1 + amt * tex2, its amount (a float texture) looked up first
    const bool mix = t.kind == kTexMix;
#pragma nounroll
    for (int i = mix ? -1 : 0; i < 2; ++i) {  // one copy of the leaf code
        const int k = i < 0 ? 2 : i;
        if (k < 2 && !((need >> k) & 1)) continue;
        const int ch = t.child[k];
        const F3 r = ch < 0 ? tex_cval(t, k) : tex_leaf(S, ch, c);
        if (k == 2)
            w0 = 1 - r.x, w1 = r.x;
        else if (prod)
            acc = acc * r;
        else if (need != 3)
            acc = r;  // a checkerboard's selection
        else {
            const float w = k == 0 ? w0 : w1;
            acc = F3{acc.x + w * r.x, acc.y + w * r.y, acc.z + w * r.z};
        }
    }
    return acc;
}
// Texture::Evaluate(si) of any texture of the scene
DEV F3 tex_evaluate(const DScene &S, int tex, const TexCtx &c) {
    if (S.textures[tex].kind == kTexImage) return tex_image(S, tex, c.u, c.v, c.td);  // ImageTexture over UVMapping2D, as it always was
    return tex_procedural(S, tex, c);
}
DEV TexCtx tex_ctx(const Isect &is, const TexDiff &td, F3 dpdx, F3 dpdy) { return TexCtx{is.u, is.v, td, is.p, dpdx, dpdy}; }

// Material::Bump (material.cpp:45-86) with an ImageTexture<Float, Float> displacement, then
// SetShadingGeometry(dpdu, dpdv, dndu, dndv, false) (interaction.cpp:72-92)
DEV void bump(const DScene &S, int tex, const TexDiff &td, F3 dpdx, F3 dpdy, Isect *is) {
    TexCtx c = tex_ctx(*is, td, dpdx, dpdy);
    float du = .5f * (fabsf(td.dudx) + fabsf(td.dudy));
    if (du == 0) du = .0005f;
    c.u = is->u + du, c.v = is->v + 0.f, c.p = is->p + du * is->sdpdu;  // siEval.p = p + du * shading.dpdu, siEval.uv = uv + (du, 0)
    const float u_displace = tex_evaluate(S, tex, c).x;
    float dv = .5f * (fabsf(td.dvdx) + fabsf(td.dvdy));
    if (dv == 0) dv = .0005f;
    c.u = is->u + 0.f, c.v = is->v + dv, c.p = is->p + dv * is->sdpdv;
    const float v_displace = tex_evaluate(S, tex, c).x;
    c.u = is->u, c.v = is->v, c.p = is->p;
    const float displace = tex_evaluate(S, tex, c).x;
    const F3 dpdu = is->sdpdu + (u_displace - displace) / du * is->sn + displace * is->dndu;
    const F3 dpdv = is->sdpdv + (v_displace - displace) / dv * is->sn + displace * is->dndv;
    F3 sn = normalize(cross(dpdu, dpdv));
    if (is->flip) sn = -sn;
    sn = faceforward(sn, is->n);
    is->sn = sn;
    is->sdpdu = dpdu;
    is->sdpdv = dpdv;
}

// the material with its textured parameters looked up at the hit (Texture::Evaluate(*si))
DEV DMaterial textured_material(const DScene &S, const DMaterial &m, const Isect &is, const TexDiff &td, F3 dpdx, F3 dpdy) {
    DMaterial r = m;
    const TexCtx tc = tex_ctx(is, td, dpdx, dpdy);
    if (m.kd_tex >= 0) {
        const F3 c = tex_evaluate(S, m.kd_tex, tc);  // times the constant: 1, or a "scale" texture's factor
        r.kd[0] = c.x * m.kd[0], r.kd[1] = c.y * m.kd[1], r.kd[2] = c.z * m.kd[2];
    }
    if (m.ks_tex >= 0) {
        const F3 c = tex_evaluate(S, m.ks_tex, tc);  // times the constant: 1, or a "scale" texture's factor
        r.ks[0] = c.x * m.ks[0], r.ks[1] = c.y * m.ks[1], r.ks[2] = c.z * m.ks[2];
    }
    if (m.kr_tex >= 0) {
        const F3 c = tex_evaluate(S, m.kr_tex, tc);  // times the constant: 1, or a "scale" texture's factor
        r.kr[0] = c.x * m.kr[0], r.kr[1] = c.y * m.kr[1], r.kr[2] = c.z * m.kr[2];
    }
    if (m.sigma_tex >= 0) {  // sigma->Evaluate(*si), matte.cpp:56-61; OrenNayar's constants, reflection.h:414-420
        const float sig = clampf(tex_evaluate(S, m.sigma_tex, tc).x, 0.f, 90.f);
        r.on_a = 1.f;
        r.on_b = 0.f;
        if (sig != 0) {
            const float sg = (kPi / 180) * sig;
            const float sigma2 = sg * sg;
            r.on_a = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
            r.on_b = 0.45f * sigma2 / (sigma2 + 0.09f);
        }
    }
    if (m.rough_tex >= 0) {  // roughness->Evaluate(*si), then RoughnessToAlpha (microfacet.h:123-128)
        float rough = tex_evaluate(S, m.rough_tex, tc).x;
        if (m.remap_roughness) {
            rough = mx(rough, 1e-3f);
            const float x = log_f(rough);
            rough = 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
        }
        r.alpha = rough;
        if (m.rough_tex_v == -2) r.alpha_y = rough;   // roughv = roughu, uber.cpp:83-84 (plastic: one roughness)
    }
    if (m.rough_tex_v >= 0) {  // "vroughness" as a float image (uber.cpp:76, 83)
        float rough = tex_evaluate(S, m.rough_tex_v, tc).x;
        if (m.remap_roughness) {
            rough = mx(rough, 1e-3f);
            const float x = log_f(rough);
            rough = 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
        }
        r.alpha_y = rough;
    }
    if (m.opacity_tex >= 0) {  // opacity->Evaluate(*si), uber.cpp:53
        const F3 c = tex_evaluate(S, m.opacity_tex, tc);
        r.opacity[0] = c.x * m.opacity[0], r.opacity[1] = c.y * m.opacity[1], r.opacity[2] = c.z * m.opacity[2];
    }
    if (m.kt_tex >= 0) {
        const F3 c = tex_evaluate(S, m.kt_tex, tc);  // times the constant: 1, or a "scale" texture's factor
        r.kt[0] = c.x * m.kt[0], r.kt[1] = c.y * m.kt[1], r.kt[2] = c.z * m.kt[2];
    }
    return r;
}

// Matte / Plastic / Uber / Mirror / Glass / Metal / Substrate / Translucent ComputeScatteringFunctions (matte.cpp:45-62,
// plastic.cpp:45-70, uber.cpp:45-100, mirror.cpp:44-55, glass.cpp:45-92, metal.cpp:58-79, substrate.cpp:45-66, translucent.cpp:45-80)
// EXT = false: the scene has matte and plastic only (checked at upload); the specular lobes then fold away
template <bool EXT = true>
DEV Bsdf make_bsdf(const DMaterial &m, const Isect &is) {
    Bsdf b;
    b.ns = is.sn;
    b.ng = is.n;
    b.ss = normalize(is.sdpdu);
    b.ts = cross(b.ns, b.ss);
    b.n_lobes = 0;
    // the material's first 32 bytes as two 16-byte loads (field by field they come as four)
    float4 m_kd, m_ks;  // (bitcast type, kd), (ks, alpha)
    __builtin_memcpy(&m_kd, &m.type, 16);
    __builtin_memcpy(&m_ks, &m.ks[0], 16);
    keep_whole(m_kd);
    keep_whole(m_ks);
    const int m_type = int(f2b(m_kd.x));
    // UberMaterial (uber.cpp:53-61): op = opacity.Clamp(), t = (-op + Spectrum(1.f)).Clamp(); every other coefficient is op * K.Clamp()
    const bool uber = EXT && m_type == kMatUber;
    F3 op = F3{1.f, 1.f, 1.f};
    b.t0 = F3{0, 0, 0};
    b.has_t0 = b.has_t1 = false;
    if (uber) {
        op = F3{clampf(m.opacity[0], 0, IILE_INF), clampf(m.opacity[1], 0, IILE_INF), clampf(m.opacity[2], 0, IILE_INF)};
        b.t0 = F3{clampf(-op.x + 1.f, 0, IILE_INF), clampf(-op.y + 1.f, 0, IILE_INF), clampf(-op.z + 1.f, 0, IILE_INF)};
        b.has_t0 = !is_black(b.t0);
        if (b.has_t0) ++b.n_lobes;
    }
    b.kd = F3{clampf(m_kd.y, 0, IILE_INF), clampf(m_kd.z, 0, IILE_INF), clampf(m_kd.w, 0, IILE_INF)};
    if (uber) b.kd = op * b.kd;
    b.has_lambert = !is_black(b.kd) && !(EXT && m_type == kMatSubstrate);   // (substrate's Kd is FresnelBlend's Rd)
    if (b.has_lambert) ++b.n_lobes;
    b.ks = F3{0, 0, 0};
    b.has_micro = false;
    b.alpha = m_ks.w;
    b.alpha_y = (EXT && (m_type == kMatUber || m_type == kMatGlass || m_type == kMatMetal || m_type == kMatSubstrate)) ? m.alpha_y : b.alpha;   // (uber with a roughness image: textured_material sets both)
    b.oren_nayar = EXT && m_type == kMatMatte && m.on_b != 0.f;  // matte.cpp:56-61 (B == 0 iff sigma == 0)
    b.on_a = m.on_a;
    b.on_b = m.on_b;
    b.mtype = EXT ? m_type : kMatPlastic;
    b.eta = EXT ? m.eta : 1.f;  // (only uber, mirror and glass read it)
    b.path_eta = b.has_t0 ? 1.f : b.eta;   // BSDF(*si, 1.f) / BSDF(*si, e), uber.cpp:56-61
    if (m_type == kMatPlastic || (EXT && m_type == kMatUber)) {
        b.ks = F3{clampf(m_ks.x, 0, IILE_INF), clampf(m_ks.y, 0, IILE_INF), clampf(m_ks.z, 0, IILE_INF)};
        if (uber) b.ks = op * b.ks;
        b.has_micro = !is_black(b.ks);
        if (b.has_micro) ++b.n_lobes;
    }
    b.kr = F3{0, 0, 0};
    b.kt = F3{0, 0, 0};
    b.has_spec = false;
    if (EXT && (m_type == kMatUber || m_type == kMatMirror)) {
        b.kr = F3{clampf(m.kr[0], 0, IILE_INF), clampf(m.kr[1], 0, IILE_INF), clampf(m.kr[2], 0, IILE_INF)};
        if (uber) b.kr = op * b.kr;
        b.has_spec = !is_black(b.kr);
        if (b.has_spec) ++b.n_lobes;
    }
    if (uber) {   // SpecularTransmission(op * Kt.Clamp(), 1, e), uber.cpp:94-99
        b.kt = op * F3{clampf(m.kt[0], 0, IILE_INF), clampf(m.kt[1], 0, IILE_INF), clampf(m.kt[2], 0, IILE_INF)};
        b.has_t1 = !is_black(b.kt);
        if (b.has_t1) ++b.n_lobes;
    }
    b.has_mtrans = false;
    if (EXT && m_type == kMatGlass && (m_ks.w != 0.f || m.alpha_y != 0.f)) {  // glass.cpp:63-90: a rough dielectric (an alpha != 0)
        b.ks = F3{clampf(m.kr[0], 0, IILE_INF), clampf(m.kr[1], 0, IILE_INF), clampf(m.kr[2], 0, IILE_INF)};   // R: MicrofacetReflection
        b.kt = F3{clampf(m.kt[0], 0, IILE_INF), clampf(m.kt[1], 0, IILE_INF), clampf(m.kt[2], 0, IILE_INF)};   // T: MicrofacetTransmission
        b.has_micro = !is_black(b.ks);
        b.has_mtrans = !is_black(b.kt);
        if (b.has_micro) ++b.n_lobes;
        if (b.has_mtrans) ++b.n_lobes;
    } else if (EXT && m_type == kMatGlass) {  // glass.cpp:45-66 with isSpecular && allowMultipleLobes
        b.kr = F3{clampf(m.kr[0], 0, IILE_INF), clampf(m.kr[1], 0, IILE_INF), clampf(m.kr[2], 0, IILE_INF)};
        b.kt = F3{clampf(m.kt[0], 0, IILE_INF), clampf(m.kt[1], 0, IILE_INF), clampf(m.kt[2], 0, IILE_INF)};
        b.has_spec = !(is_black(b.kr) && is_black(b.kt));
        if (b.has_spec) ++b.n_lobes;
    }
    if (EXT && m_type == kMatMetal) {  // metal.cpp:66-78: MicrofacetReflection(1., TR(uRough, vRough), FresnelConductor(1., eta, k))
        b.ks = F3{1.f, 1.f, 1.f};
        b.has_micro = true;
        ++b.n_lobes;
        b.kr = F3{m.cond_eta[0], m.cond_eta[1], m.cond_eta[2]};   // eta
        b.kt = F3{m.cond_k[0], m.cond_k[1], m.cond_k[2]};         // k
    }
    b.has_blend = false;
    if (EXT && m_type == kMatSubstrate) {  // substrate.cpp:53-65: d = Kd.Clamp(), s = Ks.Clamp(); no lobe when both are black
        b.ks = F3{clampf(m_ks.x, 0, IILE_INF), clampf(m_ks.y, 0, IILE_INF), clampf(m_ks.z, 0, IILE_INF)};
        b.has_blend = !(is_black(b.kd) && is_black(b.ks));
        if (b.has_blend) ++b.n_lobes;
    }
    b.has_ltrans = false;
    if (EXT && m_type == kMatTranslucent) {  // translucent.cpp:51-78: r = reflect.Clamp(), t = transmit.Clamp(); no lobe when both are black
        const F3 r = F3{clampf(m.kr[0], 0, IILE_INF), clampf(m.kr[1], 0, IILE_INF), clampf(m.kr[2], 0, IILE_INF)};
        const F3 t = F3{clampf(m.kt[0], 0, IILE_INF), clampf(m.kt[1], 0, IILE_INF), clampf(m.kt[2], 0, IILE_INF)};
        const F3 kd = b.kd;   // Kd.Clamp()
        const F3 ks = F3{clampf(m_ks.x, 0, IILE_INF), clampf(m_ks.y, 0, IILE_INF), clampf(m_ks.z, 0, IILE_INF)};
        const bool r_on = !is_black(r), t_on = !is_black(t);
        b.kd = r * kd;   // LambertianReflection
        b.kr = t * kd;   // LambertianTransmission
        b.ks = r * ks;   // MicrofacetReflection
        b.kt = t * ks;   // MicrofacetTransmission
        b.has_lambert = r_on && !is_black(kd);
        b.has_ltrans = t_on && !is_black(kd);
        b.has_micro = r_on && !is_black(ks);
        b.has_mtrans = t_on && !is_black(ks);
        b.n_lobes = (b.has_lambert ? 1 : 0) + (b.has_ltrans ? 1 : 0) + (b.has_micro ? 1 : 0) + (b.has_mtrans ? 1 : 0);
    }
    return b;
}
// reflection.h:56-84
DEV float cos2_theta(F3 w) { return w.z * w.z; }
DEV float sin2_theta(F3 w) { return mx(0.f, 1.f - cos2_theta(w)); }
DEV float sin_theta(F3 w) { return sqrtf(sin2_theta(w)); }
DEV float tan_theta(F3 w) { return sin_theta(w) / w.z; }
DEV float tan2_theta(F3 w) { return sin2_theta(w) / cos2_theta(w); }
DEV float cos_phi(F3 w) {
    float st = sin_theta(w);
    return (st == 0) ? 1 : clampf(w.x / st, -1, 1);
}
DEV float sin_phi(F3 w) {
    float st = sin_theta(w);
    return (st == 0) ? 0 : clampf(w.y / st, -1, 1);
}
DEV float cos2_phi(F3 w) { return cos_phi(w) * cos_phi(w); }
DEV float sin2_phi(F3 w) { return sin_phi(w) * sin_phi(w); }
DEV bool same_hemisphere(F3 a, F3 b) { return a.z * b.z > 0; }
// FrDielectric, reflection.cpp:47-68
DEV float fr_dielectric(float cos_i, float eta_i, float eta_t) {
    cos_i = clampf(cos_i, -1, 1);
    bool entering = cos_i > 0.f;
    if (!entering) {
        float tmp = eta_i;
        eta_i = eta_t;
        eta_t = tmp;
        cos_i = fabsf(cos_i);
    }
    float sin_i = sqrtf(mx(0.f, 1 - cos_i * cos_i));
    float sin_t = eta_i / eta_t * sin_i;
    if (sin_t >= 1) return 1;
    float cos_t = sqrtf(mx(0.f, 1 - sin_t * sin_t));
    float r_parl = ((eta_t * cos_i) - (eta_i * cos_t)) / ((eta_t * cos_i) + (eta_i * cos_t));
    float r_perp = ((eta_i * cos_i) - (eta_t * cos_t)) / ((eta_i * cos_i) + (eta_t * cos_t));
    return (r_parl * r_parl + r_perp * r_perp) / 2;
}
// FrConductor, reflection.cpp:71-94, with etai = 1 (FresnelConductor(1., eta, k), metal.cpp:76-77): per channel, the Spectrum
// operations in the reference's order
DEV float fr_conductor_1(float cos_i, float eta, float k) {
    const float cos2 = cos_i * cos_i;
    const float sin2 = float(1. - double(cos2));
    const float eta2 = eta * eta, etak2 = k * k;
    const float t0 = eta2 - etak2 - sin2;
    const float a2plusb2 = sqrtf(t0 * t0 + 4 * eta2 * etak2);
    const float t1 = a2plusb2 + cos2;
    const float a = sqrtf(0.5f * (a2plusb2 + t0));
    const float t2 = (2.f * cos_i) * a;
    const float rs = (t1 - t2) / (t1 + t2);
    const float t3 = cos2 * a2plusb2 + sin2 * sin2;
    const float t4 = t2 * sin2;
    const float rp = rs * (t3 - t4) / (t3 + t4);
    return 0.5f * (rp + rs);
}
DEV F3 fr_conductor(float cos_i, F3 eta, F3 k) {
    cos_i = clampf(cos_i, -1, 1);
    return F3{fr_conductor_1(cos_i, eta.x, k.x), fr_conductor_1(cos_i, eta.y, k.y), fr_conductor_1(cos_i, eta.z, k.z)};
}
// TrowbridgeReitzDistribution::D / Lambda, microfacet.cpp:155-163, 176-184
// (ax, ay: alphax, alphay. Where the scene has no anisotropic material — the plain build always — the two are one value and the
//  expressions below compile to what they were with one alpha)
DEV float tr_d(F3 wh, float ax, float ay) {
    float t2 = tan2_theta(wh);
    if (is_inf(t2)) return 0.f;
    const float cos4 = cos2_theta(wh) * cos2_theta(wh);
    float e = (cos2_phi(wh) / (ax * ax) + sin2_phi(wh) / (ay * ay)) * t2;
    return 1 / (kPi * ax * ay * cos4 * (1 + e) * (1 + e));
}
DEV float tr_lambda(F3 w, float ax, float ay) {
    float abs_tan = fabsf(tan_theta(w));
    if (is_inf(abs_tan)) return 0.f;
    float alpha = sqrtf(cos2_phi(w) * ax * ax + sin2_phi(w) * ay * ay);
    float a2t2 = (alpha * abs_tan) * (alpha * abs_tan);
    return (-1 + sqrtf(1.f + a2t2)) / 2;
}
DEV float tr_g1(F3 w, float ax, float ay) { return 1 / (1 + tr_lambda(w, ax, ay)); }
DEV float tr_g(F3 wo, F3 wi, float ax, float ay) { return 1 / (1 + tr_lambda(wo, ax, ay) + tr_lambda(wi, ax, ay)); }
DEV float tr_pdf(F3 wo, F3 wh, float ax, float ay) { return tr_d(wh, ax, ay) * tr_g1(wo, ax, ay) * absdot(wo, wh) / fabsf(wo.z); }
// TrowbridgeReitzSample11, microfacet.cpp:238-283. The normal-incidence branch
// evaluates sqrt/cos/sin through the C (double) overloads in the reference.
DEV void tr_sample11(float cos_theta, float U1, float U2, float *slope_x, float *slope_y) {
    if (double(cos_theta) > .9999) {
        float r = float(sqrt(double(U1 / (1 - U1))));
        float phi = float(6.28318530718 * double(U2));
        double s, c;
        sincos_d(double(phi), &s, &c);
        *slope_x = float(double(r) * c);
        *slope_y = float(double(r) * s);
        return;
    }
    float sin_t = sqrtf(mx(0.f, 1.f - cos_theta * cos_theta));
    float tan_t = sin_t / cos_theta;
    float a = 1 / tan_t;
    float G1 = 2 / (1 + sqrtf(1.f + 1.f / (a * a)));
    float A = 2 * U1 / G1 - 1;
    float tmp = 1.f / (A * A - 1.f);
    if (double(tmp) > 1e10) tmp = 1e10f;
    float B = tan_t;
    float D = sqrtf(mx(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.f));
    float slope_x_1 = B * tmp - D;
    float slope_x_2 = B * tmp + D;
    *slope_x = (A < 0 || slope_x_2 > 1.f / tan_t) ? slope_x_1 : slope_x_2;
    float Sg;
    if (U2 > 0.5f) {
        Sg = 1.f;
        U2 = 2.f * (U2 - .5f);
    } else {
        Sg = -1.f;
        U2 = 2.f * (.5f - U2);
    }
    float z = (U2 * (U2 * (U2 * 0.27385f - 0.73369f) + 0.46341f)) /
              (U2 * (U2 * (U2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
    *slope_y = Sg * z * sqrtf(1.f + *slope_x * *slope_x);
}
// TrowbridgeReitzSample + Sample_wh (visible-area), microfacet.cpp:285-336
DEV F3 tr_sample_wh(F3 wo, float u0, float u1, float ax, float ay) {
    bool flip = wo.z < 0;
    F3 wi = flip ? -wo : wo;
    F3 ws = normalize(F3{ax * wi.x, ay * wi.y, wi.z});
    float sx, sy;
    tr_sample11(ws.z, u0, u1, &sx, &sy);
    float tmp = cos_phi(ws) * sx - sin_phi(ws) * sy;
    sy = sin_phi(ws) * sx + cos_phi(ws) * sy;
    sx = tmp;
    sx = ax * sx;
    sy = ay * sy;
    F3 wh = normalize(F3{-sx, -sy, 1.f});
    if (flip) wh = -wh;
    return wh;
}
// MicrofacetReflection::f, reflection.cpp:226-236, with FresnelDielectric(1.5, 1) (plastic) or (1, e) (uber, glass, translucent), or
// FresnelConductor(1, eta, k) (metal: its Evaluate takes |cos|, reflection.cpp:118-120)
DEV F3 micro_f(const Bsdf &b, F3 wo, F3 wi) {
    float cos_o = fabsf(wo.z), cos_i = fabsf(wi.z);
    F3 wh = wi + wo;
    if (cos_i == 0 || cos_o == 0) return F3{0, 0, 0};
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return F3{0, 0, 0};
    wh = normalize(wh);
    F3 F;
    if (b.mtype == kMatMetal) {
        F = fr_conductor(fabsf(dot(wi, wh)), b.kr, b.kt);
    } else {
        float Fr = (b.mtype == kMatUber || b.mtype == kMatGlass || b.mtype == kMatTranslucent) ? fr_dielectric(dot(wi, wh), 1.f, b.eta)
                                                                                              : fr_dielectric(dot(wi, wh), 1.5f, 1.f);
        F = F3{Fr, Fr, Fr};
    }
    return sdiv(b.ks * tr_d(wh, b.alpha, b.alpha_y) * tr_g(wo, wi, b.alpha, b.alpha_y) * F, 4 * cos_i * cos_o);
}
DEV float micro_pdf(const Bsdf &b, F3 wo, F3 wi) {
    if (!same_hemisphere(wo, wi)) return 0;
    F3 wh = normalize(wo + wi);
    return tr_pdf(wo, wh, b.alpha, b.alpha_y) / (4 * dot(wo, wh));
}
// FresnelBlend::f, reflection.cpp:285-298, and its SchlickFresnel, reflection.h:485-488
DEV float pow5(float v) { return (v * v) * (v * v) * v; }
DEV F3 blend_f(const Bsdf &b, F3 wo, F3 wi) {
    const F3 one = F3{1.f, 1.f, 1.f};
    const F3 diffuse = (28.f / (23.f * kPi)) * b.kd * (one - b.ks) * (1 - pow5(1 - .5f * fabsf(wi.z))) * (1 - pow5(1 - .5f * fabsf(wo.z)));
    F3 wh = wi + wo;
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return F3{0, 0, 0};
    wh = normalize(wh);
    const float s = tr_d(wh, b.alpha, b.alpha_y) / (4 * absdot(wi, wh) * mx(fabsf(wi.z), fabsf(wo.z)));
    const F3 schlick = b.ks + pow5(1 - dot(wi, wh)) * (one - b.ks);
    return diffuse + s * schlick;
}
// FresnelBlend::Pdf, reflection.cpp:470-475
DEV float blend_pdf(const Bsdf &b, F3 wo, F3 wi) {
    if (!same_hemisphere(wo, wi)) return 0;
    const F3 wh = normalize(wo + wi);
    const float pdf_wh = tr_pdf(wo, wh, b.alpha, b.alpha_y);
    return .5f * (fabsf(wi.z) * kInvPi + pdf_wh / (4 * dot(wo, wh)));
}
// LambertianReflection::f (reflection.cpp:178-180) or OrenNayar::f (reflection.cpp:197-219)
DEV F3 diffuse_f(const Bsdf &b, F3 wo, F3 wi) {
    if (!b.oren_nayar) return b.kd * kInvPi;
    const float sin_i = sin_theta(wi), sin_o = sin_theta(wo);
    float max_cos = 0;
    if (double(sin_i) > 1e-4 && double(sin_o) > 1e-4) {
        const float sin_phi_i = sin_phi(wi), cos_phi_i = cos_phi(wi);
        const float sin_phi_o = sin_phi(wo), cos_phi_o = cos_phi(wo);
        const float d_cos = cos_phi_i * cos_phi_o + sin_phi_i * sin_phi_o;
        max_cos = mx(0.f, d_cos);
    }
    float sin_alpha, tan_beta;
    if (fabsf(wi.z) > fabsf(wo.z)) {
        sin_alpha = sin_o;
        tan_beta = sin_i / fabsf(wi.z);
    } else {
        sin_alpha = sin_i;
        tan_beta = sin_o / fabsf(wo.z);
    }
    return b.kd * kInvPi * (b.on_a + b.on_b * max_cos * sin_alpha * tan_beta);
}
DEV float lambert_pdf(F3 wo, F3 wi) { return same_hemisphere(wo, wi) ? fabsf(wi.z) * kInvPi : 0; }
// LambertianTransmission::f / Pdf, reflection.cpp:187-190, 401-403: T / pi with no hemisphere test of its own (BSDF::f asks for a
// transmission lobe only where wi and wo lie on opposite sides of ng); T is held in kr
DEV F3 ltrans_f(const Bsdf &b) { return b.kr * kInvPi; }
DEV float ltrans_pdf(F3 wo, F3 wi) { return !same_hemisphere(wo, wi) ? fabsf(wi.z) * kInvPi : 0; }
// Refract, reflection.h:96-108
DEV bool refract_dir(F3 wi, F3 n, float eta, F3 *wt) {
    const float cos_i = dot(n, wi);
    const float sin2_i = mx(0.f, 1 - cos_i * cos_i);
    const float sin2_t = eta * eta * sin2_i;
    if (sin2_t >= 1) return false;
    const float cos_t = sqrtf(1 - sin2_t);
    *wt = eta * -wi + (eta * cos_i - cos_t) * n;
    return true;
}
// MicrofacetTransmission::f, reflection.cpp:244-266 (etaA = 1, etaB = b.eta, mode == Radiance)
DEV F3 mtrans_f(const Bsdf &b, F3 wo, F3 wi) {
    if (same_hemisphere(wo, wi)) return F3{0, 0, 0};
    const float cos_o = wo.z, cos_i = wi.z;
    if (cos_i == 0 || cos_o == 0) return F3{0, 0, 0};
    const float eta_a = 1.f, eta_b = b.eta;
    const float eta = wo.z > 0 ? (eta_b / eta_a) : (eta_a / eta_b);
    F3 wh = normalize(wo + wi * eta);
    if (wh.z < 0) wh = -wh;
    const float F = fr_dielectric(dot(wo, wh), eta_a, eta_b);
    const float sqrt_denom = dot(wo, wh) + eta * dot(wi, wh);
    const float factor = 1 / eta;
    const float omf = 1.f - F;
    return F3{omf, omf, omf} * b.kt *
           fabsf(tr_d(wh, b.alpha, b.alpha_y) * tr_g(wo, wi, b.alpha, b.alpha_y) * eta * eta * absdot(wi, wh) * absdot(wo, wh) * factor * factor /
                 (cos_i * cos_o * sqrt_denom * sqrt_denom));
}
// MicrofacetTransmission::Pdf, reflection.cpp:435-447
DEV float mtrans_pdf(const Bsdf &b, F3 wo, F3 wi) {
    if (same_hemisphere(wo, wi)) return 0;
    const float eta_a = 1.f, eta_b = b.eta;
    const float eta = wo.z > 0 ? (eta_b / eta_a) : (eta_a / eta_b);
    const F3 wh = normalize(wo + wi * eta);
    const float sqrt_denom = dot(wo, wh) + eta * dot(wi, wh);
    const float dwh_dwi = fabsf((eta * eta * dot(wi, wh)) / (sqrt_denom * sqrt_denom));
    return tr_pdf(wo, wh, b.alpha, b.alpha_y) * dwh_dwi;
}
DEV F3 lobes_f(const Bsdf &b, F3 wo, F3 wi) {
    F3 f = F3{0, 0, 0};
    if (b.has_lambert) f = f + diffuse_f(b, wo, wi);
    if (b.has_micro) f = f + micro_f(b, wo, wi);
    if (b.has_blend) f = f + blend_f(b, wo, wi);
    return f;
}
// the BSDF_TRANSMISSION lobes that are not specular, summed in BxDF order: `(!reflect && (bxdfs[i]->type & BSDF_TRANSMISSION))`
DEV F3 trans_lobes_f(const Bsdf &b, F3 wo, F3 wi) {
    F3 f = F3{0, 0, 0};
    if (b.has_ltrans) f = f + ltrans_f(b);
    if (b.has_mtrans) f = f + mtrans_f(b, wo, wi);
    return f;
}
// BSDF::f, reflection.cpp:686-699
DEV F3 bsdf_f(const Bsdf &b, F3 woW, F3 wiW) {
    F3 wi = to_local(b, wiW), wo = to_local(b, woW);
    if (wo.z == 0) return F3{0, 0, 0};
    bool reflect = dot(wiW, b.ng) * dot(woW, b.ng) > 0;
    if (reflect) return lobes_f(b, wo, wi);
    return trans_lobes_f(b, wo, wi);
}
// BSDF::Pdf, reflection.cpp:786-801
DEV float bsdf_pdf(const Bsdf &b, F3 woW, F3 wiW) {
    if (b.n_lobes == 0) return 0.f;
    F3 wo = to_local(b, woW), wi = to_local(b, wiW);
    if (wo.z == 0) return 0.f;
    float pdf = 0.f;
    if (b.has_lambert) pdf += lambert_pdf(wo, wi);
    if (b.has_ltrans) pdf += ltrans_pdf(wo, wi);
    if (b.has_micro) pdf += micro_pdf(b, wo, wi);
    if (b.has_mtrans) pdf += mtrans_pdf(b, wo, wi);
    if (b.has_blend) pdf += blend_pdf(b, wo, wi);
    const int matching = n_nonspec(b);  // flags = BSDF_ALL & ~BSDF_SPECULAR
    return matching > 0 ? pdf / matching : 0.f;
}
// BSDF::Sample_f, reflection.cpp:719-784. *pdf is untouched on the early
// `wo.z == 0` return, as in the reference.
DEV F3 bsdf_sample_f(const Bsdf &b, F3 woW, F3 *wiW, float u0, float u1, float *pdf, const bool allow_specular = false,
                     bool *sampled_specular = nullptr, bool *sampled_transmission = nullptr) {
    // `type` is BSDF_ALL (allow_specular) or BSDF_ALL & ~BSDF_SPECULAR
    if (sampled_specular) *sampled_specular = false;
    if (sampled_transmission) *sampled_transmission = false;
    const int matching = allow_specular ? b.n_lobes : n_nonspec(b);
    if (matching == 0) {
        *pdf = 0;
        return F3{0, 0, 0};
    }
    int comp = int(floorf(u0 * matching));
    if (comp > matching - 1) comp = matching - 1;
    // the comp-th present lobe in BxDF order: [3 uber's pass-through], 0 Lambertian, 1 microfacet, 2 specular reflection, [4 uber's Kt lobe]
    // (6: substrate's FresnelBlend, the one lobe of its BSDF; 7: translucent's LambertianTransmission, right behind its Lambertian)
    int pick, count = comp;
    if (allow_specular && b.has_t0 && count-- == 0)
        pick = 3;
    else if (b.has_lambert && count-- == 0)
        pick = 0;
    else if (b.has_ltrans && count-- == 0)
        pick = 7;
    else if (b.has_micro && count-- == 0)
        pick = 1;
    else if (b.has_mtrans && count-- == 0)
        pick = 5;   // rough glass: MicrofacetTransmission behind MicrofacetReflection (glass.cpp:74-90)
    else if (b.has_blend && count-- == 0)
        pick = 6;
    else if (!(allow_specular && b.has_t1) || (b.has_spec && count-- == 0))
        pick = 2;
    else
        pick = 4;
    // (comp < matching: the specular lobe is only ever picked when there is one — said aloud so that the builds whose
    // materials have none, where has_spec is a constant, drop that branch and the loads that feed it)
    if (pick == 2 && !b.has_spec) __builtin_unreachable();
    const float ur0 = mn(u0 * matching - comp, kOneMinusEpsilon);
    F3 wo = to_local(b, woW);
    if (wo.z == 0) return F3{0, 0, 0};
    *pdf = 0;
    F3 wi = F3{0, 0, 0}, f;
    if (pick == 0) {  // BxDF::Sample_f, reflection.cpp:378-385
        wi = cosine_sample_hemisphere(ur0, u1);
        if (wo.z < 0) wi.z *= -1;
        *pdf = lambert_pdf(wo, wi);
        f = diffuse_f(b, wo, wi);
    } else if (pick == 7) {  // LambertianTransmission::Sample_f, reflection.cpp:391-398: the hemisphere opposite wo
        wi = cosine_sample_hemisphere(ur0, u1);
        if (wo.z > 0) wi.z *= -1;
        *pdf = ltrans_pdf(wo, wi);
        f = ltrans_f(b);
    } else if (pick == 1) {  // MicrofacetReflection::Sample_f, reflection.cpp:405-417
        F3 wh = tr_sample_wh(wo, ur0, u1, b.alpha, b.alpha_y);
        wi = -wo + 2 * dot(wo, wh) * wh;
        if (!same_hemisphere(wo, wi))
            f = F3{0, 0, 0};
        else {
            *pdf = tr_pdf(wo, wh, b.alpha, b.alpha_y) / (4 * dot(wo, wh));
            f = micro_f(b, wo, wi);
        }
    } else if (pick == 6) {  // FresnelBlend::Sample_f, reflection.cpp:450-468
        float ua = ur0;
        if (ua < .5f) {
            ua = mn(2 * ua, kOneMinusEpsilon);
            wi = cosine_sample_hemisphere(ua, u1);
            if (wo.z < 0) wi.z *= -1;
        } else {
            ua = mn(2 * (ua - .5f), kOneMinusEpsilon);
            const F3 wh = tr_sample_wh(wo, ua, u1, b.alpha, b.alpha_y);
            wi = -wo + 2 * dot(wo, wh) * wh;
            if (!same_hemisphere(wo, wi)) return F3{0, 0, 0};  // `return Spectrum(0.f)`, pdf stays 0
        }
        *pdf = blend_pdf(b, wo, wi);
        f = blend_f(b, wo, wi);
    } else if (pick == 5) {  // MicrofacetTransmission::Sample_f, reflection.cpp:425-433
        const F3 wh = tr_sample_wh(wo, ur0, u1, b.alpha, b.alpha_y);
        const float eta_a = 1.f, eta_b = b.eta;
        const float eta = wo.z > 0 ? (eta_a / eta_b) : (eta_b / eta_a);
        if (!refract_dir(wo, wh, eta, &wi)) return F3{0, 0, 0};  // `return 0`, pdf stays 0
        *pdf = mtrans_pdf(b, wo, wi);
        f = mtrans_f(b, wo, wi);
    } else if (pick >= 3) {  // SpecularTransmission::Sample_f, reflection.cpp:154-170 (mode == Radiance)
        const float eta_a = 1.f, eta_b = pick == 3 ? 1.f : b.eta;
        const bool entering = wo.z > 0;
        const float eta_i = entering ? eta_a : eta_b, eta_t = entering ? eta_b : eta_a;
        // Refract(wo, Faceforward(Normal3f(0, 0, 1), wo), etaI / etaT, wi), reflection.h:96-108; -n carries negative zeros, as there
        const F3 n = (wo.z < 0.f) ? -F3{0, 0, 1} : F3{0, 0, 1};
        const float eta = eta_i / eta_t;
        const float cos_i = dot(n, wo);
        const float sin2_i = mx(0.f, 1 - cos_i * cos_i);
        const float sin2_t = eta * eta * sin2_i;
        if (sin2_t >= 1) return F3{0, 0, 0};  // `return 0`, pdf stays 0
        const float cos_t = sqrtf(1 - sin2_t);
        wi = eta * -wo + (eta * cos_i - cos_t) * n;
        *pdf = 1;
        F3 ft = (pick == 3 ? b.t0 : b.kt) * (1.f - fr_dielectric(wi.z, eta_a, eta_b));
        ft = ft * ((eta_i * eta_i) / (eta_t * eta_t));
        f = sdiv(ft, fabsf(wi.z));
        if (sampled_specular) *sampled_specular = true;
        if (sampled_transmission) *sampled_transmission = true;
    } else if (b.mtype == kMatGlass) {  // FresnelSpecular::Sample_f, reflection.cpp:477-511 (mode == Radiance)
        const float eta_a = 1.f, eta_b = b.eta;
        const float F = fr_dielectric(wo.z, eta_a, eta_b);
        if (ur0 < F) {
            wi = F3{-wo.x, -wo.y, wo.z};
            *pdf = F;
            f = sdiv(F * b.kr, fabsf(wi.z));
        } else {
            const bool entering = wo.z > 0;
            const float eta_i = entering ? eta_a : eta_b, eta_t = entering ? eta_b : eta_a;
            // Refract(wo, Faceforward(Normal3f(0, 0, 1), wo), etaI / etaT, wi), reflection.h:96-108;
            // -n carries negative zeros, as there
            const F3 n = (wo.z < 0.f) ? -F3{0, 0, 1} : F3{0, 0, 1};
            const float eta = eta_i / eta_t;
            const float cos_i = dot(n, wo);
            const float sin2_i = mx(0.f, 1 - cos_i * cos_i);
            const float sin2_t = eta * eta * sin2_i;
            if (sin2_t >= 1) return F3{0, 0, 0};  // total internal reflection: `return 0`, pdf stays 0
            const float cos_t = sqrtf(1 - sin2_t);
            wi = eta * -wo + (eta * cos_i - cos_t) * n;
            F3 ft = b.kt * (1 - F);
            ft = ft * ((eta_i * eta_i) / (eta_t * eta_t));
            *pdf = 1 - F;
            f = sdiv(ft, fabsf(wi.z));
            if (sampled_transmission) *sampled_transmission = true;
        }
        if (sampled_specular) *sampled_specular = true;
    } else {  // SpecularReflection::Sample_f, reflection.cpp:136-143
        wi = F3{-wo.x, -wo.y, wo.z};
        *pdf = 1;
        const float fr = b.mtype == kMatMirror ? 1.f : fr_dielectric(wi.z, 1.f, b.eta);
        f = sdiv(F3{fr, fr, fr} * b.kr, fabsf(wi.z));
        if (sampled_specular) *sampled_specular = true;
    }
    if (*pdf == 0) {
        if (sampled_specular) *sampled_specular = false;
        if (sampled_transmission) *sampled_transmission = false;
        return F3{0, 0, 0};
    }
    *wiW = to_world(b, wi);
    const bool glossy = pick < 2 || pick == 5 || pick == 6 || pick == 7;
    if (glossy && matching > 1) {  // a specular lobe's Pdf() and f() are 0
        if (pick != 0 && b.has_lambert) *pdf += lambert_pdf(wo, wi);
        if (pick != 7 && b.has_ltrans) *pdf += ltrans_pdf(wo, wi);
        if (pick != 1 && b.has_micro) *pdf += micro_pdf(b, wo, wi);
        if (pick != 5 && b.has_mtrans) *pdf += mtrans_pdf(b, wo, wi);
    }
    if (matching > 1) *pdf /= matching;
    if (glossy && matching > 1) {
        bool reflect = dot(*wiW, b.ng) * dot(woW, b.ng) > 0;
        f = reflect ? lobes_f(b, wo, wi) : trans_lobes_f(b, wo, wi);
    }
    return f;
}

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
DEV F3 inf_le(const DScene &S, const DLight &lt, F3 d) {  // InfiniteAreaLight::Le, infinite.cpp:99-104
    const F3 w = normalize(inf_w2l(lt, d));
    return inf_lookup(S, lt, spherical_phi(w) * kInv2Pi, spherical_theta(w) * kInvPi);
}
DEV F3 inf_sample_li(const DScene &S, const DLight &lt, F3 ref_p, float u0, float u1, F3 *wi, float *pdf, F3 *target) {  // :106-137
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
DEV float inf_pdf_li(const DScene &S, const DLight &lt, F3 w) {  // :139-148 with Distribution2D::Pdf, sampling.h:135-142
    const F3 wi = inf_w2l(lt, w);
    const float theta = spherical_theta(wi), phi = spherical_phi(wi);
    float sin_theta, cos_theta;
    sincos_f(theta, &sin_theta, &cos_theta);
    if (sin_theta == 0) return 0;
    const float p0 = phi * kInv2Pi, p1 = theta * kInvPi;
    int iu = int(p0 * float(lt.dist_w)), iv = int(p1 * float(lt.dist_h));
    iu = iu < 0 ? 0 : (iu > lt.dist_w - 1 ? lt.dist_w - 1 : iu);
    iv = iv < 0 ? 0 : (iv > lt.dist_h - 1 ? lt.dist_h - 1 : iv);
    const float func = inf_cond(S, lt, iv)[iu];
    return (func / inf_cond(S, lt, lt.dist_h)[2 * lt.dist_h + 1]) / (2 * kPi * kPi * sin_theta);
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

// One EstimateDirect call (integrator.cpp:108-215) as a REQUEST: the shadow ray (so, sd) of the light-sampling half with what it
// adds if unoccluded (A), the closest-hit ray (mo, md) of the BSDF-sampling half with what it adds if it ends on the sampled
// light (Bc). Returns NEE_HAS_SHADOW | NEE_HAS_MIS; an output is written only where its flag is set.
// The wavefront kernels turn the request into an NEE record (k_mis / k_mis_lit / k_shadow resolve it), the per-pixel pass for
// glass scenes (k_direct_tree) traces the two rays on the spot. ul0, ul1: uLight; us0, us1: uScattering.
// lsp: the light's sphere where the caller has it at hand, else nullptr (the scene's entry is then read where a sphere light
// needs it). EXT = false: the plain build, whose one light is an emitting sphere, *lsp (both wave-uniform, see uniform_entry).
// COUNT: the instrumented build, which traces every MIS ray (no can_reach skip) and counts Shape::Pdf's Triangle::Intersect
// calls in *n_pdf_tests / *n_pdf_hits.
template <bool EXT, bool COUNT>
DEV uint32_t estimate_direct_request(const DScene &S, const DLight &lt, const DSphere *lsp, const Isect &is, const Bsdf &bsdf, float ul0,
                                     float ul1, float us0, float us1, F3 &so, F3 &sd, F3 &A, F3 &mo, F3 &md, F3 &Bc,
                                     unsigned long long *n_pdf_tests, unsigned long long *n_pdf_hits) {
    uint32_t nee_flags = 0;
    if (EXT && lt.type == kLightInfinite) {
        // the light-sampling half through the environment map's Distribution2D, the BSDF-sampling half whose ray contributes
        // Le(ray) when it escapes (:209-210; k_mis marks escaped rays, k_mis_lit accepts them for an infinite light)
        float light_pdf = 0, scattering_pdf = 0;
        F3 wi = F3{0, 0, 0}, target = F3{0, 0, 0};
        const F3 Li = inf_sample_li(S, lt, is.p, ul0, ul1, &wi, &light_pdf, &target);
        if (light_pdf > 0 && !is_black(Li)) {
            const F3 f = bsdf_f(bsdf, is.wo, wi) * absdot(wi, is.sn);
            scattering_pdf = bsdf_pdf(bsdf, is.wo, wi);
            if (!is_black(f)) {
                so = offset_ray_origin(is.p, is.perr, is.n, target - is.p);
                sd = target - so;
                A = sdiv(f * Li * power_heuristic(light_pdf, scattering_pdf), light_pdf);
                nee_flags |= NEE_HAS_SHADOW;
            }
        }
        F3 f2 = bsdf_sample_f(bsdf, is.wo, &wi, us0, us1, &scattering_pdf);
        f2 = f2 * absdot(wi, is.sn);
        if (!is_black(f2) && scattering_pdf > 0) {
            const float lp = inf_pdf_li(S, lt, wi);
            if (lp != 0) {
                mo = offset_ray_origin(is.p, is.perr, is.n, wi);
                md = wi;
                Bc = sdiv(f2 * inf_le(S, lt, wi) * power_heuristic(scattering_pdf, lp), scattering_pdf);
                nee_flags |= NEE_HAS_MIS;
            }
        }
    } else if (EXT && iile_light_is_delta(lt.type)) {
        // a delta light (integrator.cpp:150-166): light sample only, weight 1
        F3 wi, target;
        const F3 Li = delta_light_li(S, lt, is.p, &wi, &target);
        if (!is_black(Li)) {
            const F3 f = bsdf_f(bsdf, is.wo, wi) * absdot(wi, is.sn);
            if (!is_black(f)) {
                // the light-side Interaction has neither normal nor error bounds: its OffsetRayOrigin is the point itself
                // (interaction.h:73-78)
                so = offset_ray_origin(is.p, is.perr, is.n, target - is.p);
                sd = target - so;
                A = sdiv(f * Li, 1.f);
                nee_flags |= NEE_HAS_SHADOW;
            }
        }
    } else {
        // light-sampling half (integrator.cpp:117-163)
        float light_pdf = 0, scattering_pdf = 0;
        F3 wi = F3{0, 0, 0}, Li = F3{0, 0, 0};
        const LightSample ps = EXT ? shape_sample(S, lt, is, ul0, ul1, &light_pdf) : sphere_sample(*lsp, is, ul0, ul1, &light_pdf);
        if (light_pdf == 0 || length_sq(ps.p - is.p) == 0) {
            light_pdf = 0;
        } else {
            wi = normalize(ps.p - is.p);
            Li = area_light_L(lt, ps.n, -wi);
        }
        if (light_pdf > 0 && !is_black(Li)) {
            const F3 f = bsdf_f(bsdf, is.wo, wi) * absdot(wi, is.sn);
            scattering_pdf = bsdf_pdf(bsdf, is.wo, wi);
            if (!is_black(f)) {
                // VisibilityTester -> SpawnRayTo(Interaction), interaction.h:73-78
                so = offset_ray_origin(is.p, is.perr, is.n, ps.p - is.p);
                const F3 target = offset_ray_origin(ps.p, ps.perr, ps.n, so - ps.p);
                sd = target - so;
                A = sdiv(f * Li * power_heuristic(light_pdf, scattering_pdf), light_pdf);
                nee_flags |= NEE_HAS_SHADOW;
            }
        }
        // BSDF-sampling half (integrator.cpp:165-213)
        F3 f2 = bsdf_sample_f(bsdf, is.wo, &wi, us0, us1, &scattering_pdf);
        f2 = f2 * absdot(wi, is.sn);
        if (!is_black(f2) && scattering_pdf > 0) {
            const F3 m_o = offset_ray_origin(is.p, is.perr, is.n, wi);
            // The ray only matters if its closest hit is the sampled light (integrator.cpp:205-209), and Sphere::Pdf is the cone's
            // pdf for ANY direction (sphere.cpp:294-306): most of these rays point away from the light. The traversal would run
            // Sphere::Intersect on this very ray with some tMax <= inf, and every rejection of that test that depends on tMax only
            // gets stricter as tMax shrinks (t0.hi > tMax, ts.hi > tMax): a ray the sphere test rejects at tMax = inf can never end
            // on the light, whatever else it hits (profiles/HISTORY.md §4 "MIS rays that cannot score"). Those rays are not traced
            // by the uninstrumented kernels (the instrumented build traces them all: the reference's ray counters are part of
            // parity), and nothing else of this half is worked out for them — the test comes first, so a wavefront whose rays all
            // miss skips the light's pdf, the weight and the contribution. Triangle emitters: Shape::Pdf intersects the triangle
            // with this ray anyway (lp == 0 on a miss).
            bool can_reach = true;
            if (!COUNT && lt.type == kLightDiffuseArea) {
                float t_l;
                F3 od_l, ph_l;
                can_reach = sphere_test(lsp ? *lsp : S.spheres[lt.sphere], m_o, wi, IILE_INF, &t_l, &od_l, &ph_l);
            } else if (EXT && !COUNT && lt.type == kLightAreaQuadric) {  // (the same holds of Disk / Cylinder::Intersect)
                float t_l;
                F3 od_l, ph_l;
                can_reach = quadric_test(S.quadrics[lt.quadric], m_o, wi, IILE_INF, &t_l, &od_l, &ph_l);
            }
            if (can_reach) {
                const float lp = EXT ? shape_pdf(S, lt, is, wi, n_pdf_tests, n_pdf_hits) : sphere_pdf(*lsp, is, wi);
                if (lp != 0) {
                    // Li is Lemit when the MIS ray finds this light facing it
                    mo = m_o;
                    md = wi;
                    Bc = sdiv(f2 * F3{lt.lemit[0], lt.lemit[1], lt.lemit[2]} * power_heuristic(scattering_pdf, lp), scattering_pdf);
                    nee_flags |= NEE_HAS_MIS;
                }
            }
        }
    }
    return nee_flags;
}

// Did the BSDF-sampled ray (mo, md) of EstimateDirect, whose closest hit was primitive `prim` of light `li` at (b0, b1, b2), end
// on the light's emitting side? (SurfaceInteraction::Le -> DiffuseAreaLight::L, integrator.cpp:205-209; the caller has checked
// `lightIsect.primitive->GetAreaLight() == &light`)
DEV bool mis_ray_lit(const DScene &S, int li, int prim, float b0, float b1, float b2, F3 mo, F3 md) {
    const DLight &lt = S.lights[li];
    Isect lis;
    if (lt.type == kLightAreaTriangle) {
        const float4 v0 = S.tri_verts[3 * size_t(prim)], v1 = S.tri_verts[3 * size_t(prim) + 1], v2 = S.tri_verts[3 * size_t(prim) + 2];
        triangle_interaction(S, prim, f2b(v0.w), F3{v0.x, v0.y, v0.z}, F3{v1.x, v1.y, v1.z}, F3{v2.x, v2.y, v2.z}, md, b0, b1, b2, &lis);
    } else {
        // the closest hit was this sphere or quadric: redo its root selection for the hit point
        shape_hit_interaction(S, lt.type == kLightAreaQuadric ? ~lt.quadric : lt.sphere, mo, md, &lis);
    }
    return lt.two_sided || dot(lis.n, -md) > 0;
}

}  // namespace iile
