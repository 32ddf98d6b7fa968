// dtex.h — what a hit point reads of its textures: ray differentials at the hit, image textures over the host-built pyramid
// (trilinear and EWA), the texture mappings, the procedural textures, bump mapping, and textured_material, which evaluates a
// material's textures into its constants. Part of dpath.h, which includes it behind the surface interactions it reads.
// (Included inside dpath.h's namespace iile, as dtrav.h is: it has no includes of its own and uses what dpath.h holds above it —
//  F3 and the math of dmath.h, DScene / DMaterial / DTexture of dscene.h, Isect, RayDiff — and TexDiff of dtrav.h.)
#pragma once
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
// TrowbridgeReitzDistribution::RoughnessToAlpha, microfacet.h:123-128
DEV float roughness_to_alpha(float rough) {
    rough = mx(rough, 1e-3f);
    const float x = log_f(rough);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
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
        if (m.remap_roughness) rough = roughness_to_alpha(rough);
        r.alpha = rough;
        if (m.rough_tex_v == -2) r.alpha_y = rough;   // roughv = roughu, uber.cpp:83-84 (plastic: one roughness)
    }
    if (m.rough_tex_v >= 0) {  // "vroughness" as a float image (uber.cpp:76, 83)
        float rough = tex_evaluate(S, m.rough_tex_v, tc).x;
        if (m.remap_roughness) rough = roughness_to_alpha(rough);
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
