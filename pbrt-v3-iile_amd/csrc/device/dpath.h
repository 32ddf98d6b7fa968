// dpath.h — device functions of the wavefront path tracer: Halton sampling,
// camera rays, ray/primitive tests and surface interactions, then, each in a header of its own
// included where it stood, BVH traversal with an LDS-resident stack (dtrav.h), textures (dtex.h),
// the BSDF (dbsdf.h) and light sampling (dlight.h), and last the path-level step that joins
// them: estimate_direct_request and mis_ray_lit.
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
// ---- array samples (Sampler::Request2DArray / Get2DArray, core/sampler.cpp:76-98; GlobalSampler::StartPixel, :136-166) ----
// A GlobalSampler fills a requested 2D array of n entries per pixel sample from the samples k n .. k n + n - 1 of the pixel:
// entry j of pixel sample k is {SampleDimension(GetIndexForSample(k n + j), dim), SampleDimension(.., dim + 1)}. Arrays start at
// arrayStartDim = 5, behind the camera sample's dimensions 0 .. 4, the 1D arrays first, then the 2D ones two dimensions each:
// `dim` is the array's own first dimension (5 for an integrator's only array). The sample number k n + j runs past the scene's
// pixelsamples, so this goes by the sampler's index and radical-inverse code, never by the sample table.
// (Not built: arrayEndDim, by which the ordinary dimensions of Get1D / Get2D step over the arrays, sampler.cpp:180-195 — nothing
//  here draws after an array yet. A caller that does adds the arrays' dimensions to its own counter.)
DEV void sample_array_2d(const DScene &S, int px, int py, uint32_t k, uint32_t n, uint32_t j, int dim, float *u0, float *u1) {
    const uint32_t idx = sample_index(S, px, py, k * n + j);
    *u0 = sample_dimension(S, idx, dim, px, py);
    *u1 = sample_dimension(S, idx, dim + 1, px, py);
}

// core/sampling.cpp:89-96
DEV F3 uniform_sample_hemisphere(float u0, float u1) {
    const float z = u0;
    const float r = sqrtf(mx(0.f, 1.f - z * z));
    const float phi = 2 * kPi * u1;
    float s, c;
    sincos_f(phi, &s, &c);
    return F3{r * c, r * s, z};
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

// ---- the sample table (DScene::stab_*): slots and back ----
// the slot of sample k of pixel (px, py): halton_index's pixel class, k fastest
DEV uint32_t sample_slot(const DScene &S, int px, int py, uint32_t k) {
    int pmx = px - (px / 128) * 128, pmy = py - (py / 128) * 128;  // Mod(), as halton_index
    if (pmx < 0) pmx += 128;
    if (pmy < 0) pmy += 128;
    return uint32_t(pmy * 128 + pmx) * S.stab_spp + k;
}
// the Halton index of a slot (the per-lane chains of a wavefront the table does not serve start from it)
DEV uint32_t slot_halton_index(const DScene &S, uint32_t slot) {
    const uint32_t cls = S.stab_spp > 1 ? div_magic(slot, S.stab_spp_magic, S.stab_spp_shift) : slot;
    return S.pixel_offsets[cls] + (slot - cls * S.stab_spp) * uint32_t(S.sample_stride);
}
// A vertex that began at dimension d0 = 5 + 7 bounce with record r[0..7] = dimensions d0 .. d0 + 7 draws its continuation at
// d0 + off: off = 0 (nothing drawn for direct light: a specular-only vertex, no lights), 1 (SampleDiscrete's sample alone: the
// chosen light had zero probability) or 5. Sample_f takes r[off], r[off + 1], the roulette r[off + 2].
DEV void record_continuation(const float4 &ra, const float4 &rb, int off, float *u0, float *u1, float *ur) {
    *u0 = off == 5 ? rb.y : (off == 1 ? ra.y : ra.x);
    *u1 = off == 5 ? rb.z : (off == 1 ? ra.z : ra.y);
    *ur = off == 5 ? rb.w : (off == 1 ? ra.w : ra.z);
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
// A moving camera's CameraToWorld at `time` (AnimatedTransform::Interpolate, transform.cpp:1144-1169, with Slerp and
// Quaternion::ToTransform, quaternion.cpp:41-59, 94-104): the stored start transform at or before the start time, the stored end
// transform at or after the end time — so a closed shutter is a static camera, bit for bit — and otherwise
// Translate(lerp T) * Slerp(dt, R0, R1).ToTransform() * Transform(lerp S), both products as Matrix4x4::Mul forms them. A call, like
// env_camera_direction and for its reason: whether the camera moves is a scene constant, and inline this branch would change the
// registers of every kernel that makes a camera ray for a camera that stands still. It gets the record's address and not the
// scene, which a kernel holds in registers.
static __device__ __attribute__((noinline)) M44 camera_to_world_motion(const DCameraMotion *mo, float time) {
    if (time <= mo->start_time) return mo->c2w_start;
    if (time >= mo->end_time) return mo->c2w_end;
    const float dt = (time - mo->start_time) / (mo->end_time - mo->start_time);
    const float *T0 = mo->T[0], *T1 = mo->T[1], *q1 = mo->R[0], *q2 = mo->R[1];
    const float tx = (1 - dt) * T0[0] + dt * T1[0], ty = (1 - dt) * T0[1] + dt * T1[1], tz = (1 - dt) * T0[2] + dt * T1[2];
    // Slerp(dt, R[0], R[1])
    float q[4];
    const float cos_theta = (q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2]) + q1[3] * q2[3];
    if (cos_theta > .9995f) {
        for (int i = 0; i < 4; ++i) q[i] = (1 - dt) * q1[i] + dt * q2[i];
        const float len = sqrtf((q[0] * q[0] + q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]), inv = 1.f / len;
        q[0] *= inv, q[1] *= inv, q[2] *= inv, q[3] = q[3] / len;  // Normalize: v /= f multiplies by the reciprocal, w /= f divides
    } else {
        const float theta = acos_f(mn(mx(cos_theta, -1.f), 1.f));
        const float thetap = theta * dt;
        float qp[4];
        for (int i = 0; i < 4; ++i) qp[i] = q2[i] - q1[i] * cos_theta;
        const float len = sqrtf((qp[0] * qp[0] + qp[1] * qp[1] + qp[2] * qp[2]) + qp[3] * qp[3]), inv = 1.f / len;
        qp[0] *= inv, qp[1] *= inv, qp[2] *= inv, qp[3] = qp[3] / len;
        float st, ct;
        sincos_f(thetap, &st, &ct);
        for (int i = 0; i < 4; ++i) q[i] = q1[i] * ct + qp[i] * st;
    }
    // rotate.ToTransform().m: the transpose of the matrix the quaternion spells out
    const float xx = q[0] * q[0], yy = q[1] * q[1], zz = q[2] * q[2];
    const float xy = q[0] * q[1], xz = q[0] * q[2], yz = q[1] * q[2];
    const float wx = q[0] * q[3], wy = q[1] * q[3], wz = q[2] * q[3];
    float R[16] = {1 - 2 * (yy + zz), 2 * (xy - wz), 2 * (xz + wy), 0,
                   2 * (xy + wz), 1 - 2 * (xx + zz), 2 * (yz - wx), 0,
                   2 * (xz - wy), 2 * (yz + wx), 1 - 2 * (xx + yy), 0,
                   0, 0, 0, 1};
    float Tm[16] = {1, 0, 0, tx, 0, 1, 0, ty, 0, 0, 1, tz, 0, 0, 0, 1};
    float Sm[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Sm[4 * i + j] = (1 - dt) * mo->S[0][3 * i + j] + dt * mo->S[1][3 * i + j];
    float TR[16];
    M44 out;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            TR[4 * i + j] = Tm[4 * i] * R[j] + Tm[4 * i + 1] * R[4 + j] + Tm[4 * i + 2] * R[8 + j] + Tm[4 * i + 3] * R[12 + j];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            out.m[4 * i + j] = TR[4 * i] * Sm[j] + TR[4 * i + 1] * Sm[4 + j] + TR[4 * i + 2] * Sm[8 + j] + TR[4 * i + 3] * Sm[12 + j];
    return out;
}
DEV M44 camera_to_world_at(const DScene &S, float time) { return camera_to_world_motion(camera_motion(S), time); }
// ray.time = Lerp(CameraSample::time, shutterOpen, shutterClose) (perspective.cpp:117, environment.cpp:52), in a moving camera's builds
DEV float camera_ray_time(const DScene &S, float u_time) {
    const DCameraMotion *mo = camera_motion(S);
    return (1 - u_time) * mo->shutter_open + u_time * mo->shutter_close;
}
// ANY_CAMERA = false: the perspective camera alone, for the two sites that make their camera ray inside a persistent traversal /
// shading loop (PassDesc::gen_fused, which a pass with an environment camera or a moving one does not set): with the other
// camera's branch in them, k_extend<.., GEN> and the plain k_shade take more scratch, whichever way that branch is compiled.
// MOVING = true: the kernel builds of a moving camera (LaunchCfg::camera_moves; k_generate<true>, k_camera_at, k_shade<.., MOT>), which
// send the ray through the transform at `time` (camera_ray_time). Every other build has none of that code and is, instruction for
// instruction, what it was before cameras moved.
template <bool ANY_CAMERA = true, bool MOVING = false>
DEV void camera_ray(const DScene &S, float pfx, float pfy, float lu0, float lu1, F3 *o_out, F3 *d_out, float *tmax,
                    const float zero = 0.f, const float time = 0.f) {
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
    F3 oerr, o, d;
    if (MOVING) {  // CameraToWorld(ray) of an AnimatedTransform, transform.cpp:1171-1181
        const M44 c2w = camera_to_world_at(S, time);
        o = xf_point_err(c2w, ro, &oerr);
        d = xf_vector(c2w, rd);
    } else {
        o = xf_point_err(S.camera_to_world, ro, &oerr);
        d = xf_vector(S.camera_to_world, rd);
    }
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
// (the two shifted rays are made from the same CameraSample, so at the same time)
template <bool MOVING>
DEV RayDiff env_camera_differentials(const DScene &S, float pfx, float pfy, F3 o, F3 d, float time) {
    const float eps = .05f;
    F3 xo, xd, yo, yd;
    float tm;
    camera_ray<true, MOVING>(S, pfx + eps, pfy, 0.f, 0.f, &xo, &xd, &tm, 0.f, time);
    camera_ray<true, MOVING>(S, pfx, pfy + eps, 0.f, 0.f, &yo, &yd, &tm, 0.f, time);
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
// MOVING (a moving camera's builds, as camera_ray): `time` is the camera ray's own, and the auxiliary rays go through the same
// interpolated transform (AnimatedTransform::operator()(RayDifferential), transform.cpp:1183-1193)
template <bool MOVING = false>
DEV RayDiff camera_differentials(const DScene &S, float pfx, float pfy, float lu0, float lu1, F3 o, F3 d, float time = 0.f) {
    if (S.env_camera) return env_camera_differentials<MOVING>(S, pfx, pfy, o, d, time);
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
    if (MOVING) {
        const M44 c2w = camera_to_world_at(S, time);
        rxo = xf_point(c2w, rxo);
        ryo = xf_point(c2w, ryo);
        rxd = xf_vector(c2w, rxd);
        ryd = xf_vector(c2w, ryd);
    } else {
        rxo = xf_point(S.camera_to_world, rxo);
        ryo = xf_point(S.camera_to_world, ryo);
        rxd = xf_vector(S.camera_to_world, rxd);
        ryd = xf_vector(S.camera_to_world, ryd);
    }
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

#include "dtrav.h"   // BVH traversal
#include "dtex.h"    // differentials at a hit, textures, bump, textured_material
#include "dbsdf.h"   // struct Bsdf, make_bsdf, bsdf_f / bsdf_pdf / bsdf_sample_f
#include "dlight.h"  // emitters and lights

// One EstimateDirect call (integrator.cpp:108-215) as a REQUEST: the shadow ray (so, sd) of the light-sampling half with what it
// adds if unoccluded (A), the closest-hit ray (mo, md) of the BSDF-sampling half with what it adds if it ends on the sampled
// light (Bc). Returns NEE_HAS_SHADOW | NEE_HAS_MIS; an output is written only where its flag is set.
// The wavefront kernels turn the request into an NEE record (k_mis / k_mis_lit / k_shadow resolve it), the per-pixel pass for
// glass scenes (k_direct_tree) traces the two rays on the spot. ul0, ul1: uLight; us0, us1: uScattering.
// lsp: the light's sphere where the caller has it at hand, else nullptr (the scene's entry is then read where a sphere light
// needs it). EXT = false: the plain build, whose one light is an emitting sphere, *lsp (both wave-uniform, see uniform_entry).
// COUNT: the instrumented build, which traces every MIS ray (no can_reach skip) and counts Shape::Pdf's Triangle::Intersect
// calls in *n_pdf_tests / *n_pdf_hits.
// BSDF: Bsdf, or the DIS builds' DisneyBsdf (dbsdf.h).
template <bool EXT, bool COUNT, class BSDF>
DEV uint32_t estimate_direct_request(const DScene &S, const DLight &lt, const DSphere *lsp, const Isect &is, const BSDF &bsdf, float ul0,
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
