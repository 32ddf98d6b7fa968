// dbsdf.h — the BSDF of a hit point: struct Bsdf and its shading frame, make_bsdf (the materials' ComputeScatteringFunctions),
// the Fresnel terms, the Trowbridge-Reitz distribution, each lobe's f / Pdf, and BSDF::f / Pdf / Sample_f over the lobes present.
// Part of dpath.h, which includes it behind dtex.h: a material comes here with its textures already evaluated.
// (Included inside dpath.h's namespace iile, as dtrav.h is: it has no includes of its own and uses what dpath.h holds above it —
//  F3 and the math of dmath.h, DMaterial and kMat* of dscene.h, Isect, keep_whole, cosine_sample_hemisphere.)
#pragma once
// ===========================================================================
// BSDF (core/reflection.{h,cpp}, core/microfacet.cpp)
// ===========================================================================
// The lobes a BSDF can hold, in the order the materials add their BxDFs (the order Sample_f counts them in): uber's pass-through
// SpecularTransmission(1 - opacity, 1, 1); LambertianReflection or OrenNayar; LambertianTransmission; MicrofacetReflection;
// MicrofacetTransmission; FresnelBlend; SpecularReflection or, for smooth glass, FresnelSpecular; uber's SpecularTransmission(Kt)
enum Lobe : int { kLobePassThrough, kLobeLambert, kLobeLambertTrans, kLobeMicro, kLobeMicroTrans, kLobeBlend, kLobeSpecular, kLobeSpecTrans };
DEV bool lobe_is_specular(Lobe l) { return l == kLobePassThrough || l == kLobeSpecular || l == kLobeSpecTrans; }   // BSDF_SPECULAR
struct Bsdf {
    F3 ns, ng, ss, ts;
    // One coefficient per lobe; lobes that never meet in one material share storage, each under its own name:
    F3 kd;                             // the Lambertian lobe's R (substrate: FresnelBlend's Rd)
    union { F3 micro_r, ks; };         // micro_r: MicrofacetReflection's R (Ks, rough glass's R, 1 for metal) | ks: FresnelBlend's Rs (substrate)
    union { F3 kr, ltrans_t, cond_eta; };   // the specular lobe's R | LambertianTransmission's T | the conductor's eta
    union { F3 kt, mtrans_t, cond_k; };     // the specular lobes' T | MicrofacetTransmission's T | the conductor's k
    float alpha, eta;
    float alpha_y;  // TrowbridgeReitzDistribution(alphax = alpha, alphay): uber's / glass's "vroughness"; the same value as alpha otherwise
    // UberMaterial's SpecularTransmission lobes (uber.cpp:53-61, 94-99): the pass-through of a surface that is not opaque —
    // SpecularTransmission(t0 = 1 - opacity, 1, 1), the FIRST lobe — and SpecularTransmission(kt = opacity Kt, 1, eta), the LAST;
    // path_eta = BSDF::eta (1 with the pass-through, else the material's: path.cpp:151-157 reads it)
    F3 t0;
    bool has_t0, has_t1;
    float path_eta;
    // rough glass (glass.cpp:66-90): MicrofacetReflection(micro_r = R, FresnelDielectric(1, eta)) is the microfacet lobe;
    // MicrofacetTransmission(mtrans_t = T, distrib, 1, eta, Radiance) — glossy, not specular
    bool has_mtrans;
    int n_lobes;  // nBxDFs
    float on_a, on_b;  // Oren-Nayar constants of the diffuse lobe (oren_nayar set)
    bool oren_nayar;
    int mtype;    // kMat*: selects the Fresnel terms (plastic 1.5/1; uber 1/eta; mirror none; metal FresnelConductor(1, cond_eta, cond_k))
                  // and, for glass, makes the specular lobe a FresnelSpecular(kr, kt, 1, eta)
    bool has_lambert, has_micro, has_spec;
    // metal (metal.cpp:58-79): the microfacet lobe is MicrofacetReflection(1, distrib, FresnelConductor(1, cond_eta, cond_k))
    // substrate (substrate.cpp:45-66): FresnelBlend(Rd = kd, Rs = ks, distrib) — glossy reflection, the only lobe of its BSDF
    bool has_blend;
    // translucent (translucent.cpp:45-80): LambertianReflection(r kd) is the Lambertian lobe; LambertianTransmission(ltrans_t = t kd)
    // comes next; MicrofacetReflection(r ks, FresnelDielectric(1, 1.5)) is the microfacet lobe and
    // MicrofacetTransmission(t ks, distrib, 1, 1.5) rough glass's
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
// Spectrum::Clamp(), spectrum.h:137-143, with its defaults: negatives to zero
DEV F3 clamp0(F3 c) { return F3{clampf(c.x, 0, IILE_INF), clampf(c.y, 0, IILE_INF), clampf(c.z, 0, IILE_INF)}; }
DEV F3 clamp0(const float c[3]) { return clamp0(F3{c[0], c[1], c[2]}); }

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
        op = clamp0(m.opacity);
        b.t0 = clamp0(F3{-op.x + 1.f, -op.y + 1.f, -op.z + 1.f});
        b.has_t0 = !is_black(b.t0);
        if (b.has_t0) ++b.n_lobes;
    }
    b.kd = clamp0(F3{m_kd.y, m_kd.z, m_kd.w});
    if (uber) b.kd = op * b.kd;
    b.has_lambert = !is_black(b.kd) && !(EXT && m_type == kMatSubstrate);   // (substrate's Kd is FresnelBlend's Rd)
    if (b.has_lambert) ++b.n_lobes;
    b.micro_r = F3{0, 0, 0};
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
        b.micro_r = clamp0(F3{m_ks.x, m_ks.y, m_ks.z});
        if (uber) b.micro_r = op * b.micro_r;
        b.has_micro = !is_black(b.micro_r);
        if (b.has_micro) ++b.n_lobes;
    }
    b.kr = F3{0, 0, 0};
    b.kt = F3{0, 0, 0};
    b.has_spec = false;
    if (EXT && (m_type == kMatUber || m_type == kMatMirror)) {
        b.kr = clamp0(m.kr);
        if (uber) b.kr = op * b.kr;
        b.has_spec = !is_black(b.kr);
        if (b.has_spec) ++b.n_lobes;
    }
    if (uber) {   // SpecularTransmission(op * Kt.Clamp(), 1, e), uber.cpp:94-99
        b.kt = op * clamp0(m.kt);
        b.has_t1 = !is_black(b.kt);
        if (b.has_t1) ++b.n_lobes;
    }
    b.has_mtrans = false;
    if (EXT && m_type == kMatGlass && (m_ks.w != 0.f || m.alpha_y != 0.f)) {  // glass.cpp:63-90: a rough dielectric (an alpha != 0)
        b.micro_r = clamp0(m.kr);
        b.mtrans_t = clamp0(m.kt);
        b.has_micro = !is_black(b.micro_r);
        b.has_mtrans = !is_black(b.mtrans_t);
        if (b.has_micro) ++b.n_lobes;
        if (b.has_mtrans) ++b.n_lobes;
    } else if (EXT && m_type == kMatGlass) {  // glass.cpp:45-66 with isSpecular && allowMultipleLobes
        b.kr = clamp0(m.kr);
        b.kt = clamp0(m.kt);
        b.has_spec = !(is_black(b.kr) && is_black(b.kt));
        if (b.has_spec) ++b.n_lobes;
    }
    if (EXT && m_type == kMatMetal) {  // metal.cpp:66-78: MicrofacetReflection(1., TR(uRough, vRough), FresnelConductor(1., eta, k))
        b.micro_r = F3{1.f, 1.f, 1.f};
        b.has_micro = true;
        ++b.n_lobes;
        b.cond_eta = F3{m.cond_eta[0], m.cond_eta[1], m.cond_eta[2]};
        b.cond_k = F3{m.cond_k[0], m.cond_k[1], m.cond_k[2]};
    }
    b.has_blend = false;
    if (EXT && m_type == kMatSubstrate) {  // substrate.cpp:53-65: d = Kd.Clamp(), s = Ks.Clamp(); no lobe when both are black
        b.ks = clamp0(F3{m_ks.x, m_ks.y, m_ks.z});
        b.has_blend = !(is_black(b.kd) && is_black(b.ks));
        if (b.has_blend) ++b.n_lobes;
    }
    b.has_ltrans = false;
    if (EXT && m_type == kMatTranslucent) {  // translucent.cpp:51-78: r = reflect.Clamp(), t = transmit.Clamp(); no lobe when both are black
        const F3 r = clamp0(m.kr);
        const F3 t = clamp0(m.kt);
        const F3 kd = b.kd;   // Kd.Clamp()
        const F3 ks = clamp0(F3{m_ks.x, m_ks.y, m_ks.z});
        const bool r_on = !is_black(r), t_on = !is_black(t);
        b.kd = r * kd;   // LambertianReflection
        b.ltrans_t = t * kd;   // LambertianTransmission
        b.micro_r = r * ks;    // MicrofacetReflection
        b.mtrans_t = t * ks;   // MicrofacetTransmission
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
        F = fr_conductor(fabsf(dot(wi, wh)), b.cond_eta, b.cond_k);
    } else {
        float Fr = (b.mtype == kMatUber || b.mtype == kMatGlass || b.mtype == kMatTranslucent) ? fr_dielectric(dot(wi, wh), 1.f, b.eta)
                                                                                              : fr_dielectric(dot(wi, wh), 1.5f, 1.f);
        F = F3{Fr, Fr, Fr};
    }
    return sdiv(b.micro_r * tr_d(wh, b.alpha, b.alpha_y) * tr_g(wo, wi, b.alpha, b.alpha_y) * F, 4 * cos_i * cos_o);
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
// transmission lobe only where wi and wo lie on opposite sides of ng)
DEV F3 ltrans_f(const Bsdf &b) { return b.ltrans_t * kInvPi; }
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
// What SpecularTransmission and FresnelSpecular's transmitted half share (reflection.cpp:154-170, 493-509; mode == Radiance), between
// eta_a above the surface and eta_b below: Refract(wo, Faceforward(Normal3f(0, 0, 1), wo), etaI / etaT, wi) (-n carries negative
// zeros, as there) and the scale etaI^2 / etaT^2 of the radiance that goes through. False: total internal reflection.
DEV bool specular_refract(F3 wo, float eta_a, float eta_b, F3 *wi, float *scale) {
    const bool entering = wo.z > 0;
    const float eta_i = entering ? eta_a : eta_b, eta_t = entering ? eta_b : eta_a;
    const F3 n = (wo.z < 0.f) ? -F3{0, 0, 1} : F3{0, 0, 1};
    if (!refract_dir(wo, n, eta_i / eta_t, wi)) return false;
    *scale = (eta_i * eta_i) / (eta_t * eta_t);
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
    return F3{omf, omf, omf} * b.mtrans_t *
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
    // the comp-th present lobe in BxDF order
    Lobe pick;
    int count = comp;
    if (allow_specular && b.has_t0 && count-- == 0)
        pick = kLobePassThrough;
    else if (b.has_lambert && count-- == 0)
        pick = kLobeLambert;
    else if (b.has_ltrans && count-- == 0)
        pick = kLobeLambertTrans;
    else if (b.has_micro && count-- == 0)
        pick = kLobeMicro;
    else if (b.has_mtrans && count-- == 0)
        pick = kLobeMicroTrans;
    else if (b.has_blend && count-- == 0)
        pick = kLobeBlend;
    else if (!(allow_specular && b.has_t1) || (b.has_spec && count-- == 0))
        pick = kLobeSpecular;
    else
        pick = kLobeSpecTrans;
    // (comp < matching: the specular lobe is only ever picked when there is one — said aloud so that the builds whose
    // materials have none, where has_spec is a constant, drop that branch and the loads that feed it)
    if (pick == kLobeSpecular && !b.has_spec) __builtin_unreachable();
    const float ur0 = mn(u0 * matching - comp, kOneMinusEpsilon);
    F3 wo = to_local(b, woW);
    if (wo.z == 0) return F3{0, 0, 0};
    *pdf = 0;
    F3 wi = F3{0, 0, 0}, f;
    if (pick == kLobeLambert) {  // BxDF::Sample_f, reflection.cpp:378-385
        wi = cosine_sample_hemisphere(ur0, u1);
        if (wo.z < 0) wi.z *= -1;
        *pdf = lambert_pdf(wo, wi);
        f = diffuse_f(b, wo, wi);
    } else if (pick == kLobeLambertTrans) {  // LambertianTransmission::Sample_f, reflection.cpp:391-398: the hemisphere opposite wo
        wi = cosine_sample_hemisphere(ur0, u1);
        if (wo.z > 0) wi.z *= -1;
        *pdf = ltrans_pdf(wo, wi);
        f = ltrans_f(b);
    } else if (pick == kLobeMicro) {  // MicrofacetReflection::Sample_f, reflection.cpp:405-417
        F3 wh = tr_sample_wh(wo, ur0, u1, b.alpha, b.alpha_y);
        wi = -wo + 2 * dot(wo, wh) * wh;
        if (!same_hemisphere(wo, wi))
            f = F3{0, 0, 0};
        else {
            *pdf = tr_pdf(wo, wh, b.alpha, b.alpha_y) / (4 * dot(wo, wh));
            f = micro_f(b, wo, wi);
        }
    } else if (pick == kLobeBlend) {  // FresnelBlend::Sample_f, reflection.cpp:450-468
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
    } else if (pick == kLobeMicroTrans) {  // MicrofacetTransmission::Sample_f, reflection.cpp:425-433
        const F3 wh = tr_sample_wh(wo, ur0, u1, b.alpha, b.alpha_y);
        const float eta_a = 1.f, eta_b = b.eta;
        const float eta = wo.z > 0 ? (eta_a / eta_b) : (eta_b / eta_a);
        if (!refract_dir(wo, wh, eta, &wi)) return F3{0, 0, 0};  // `return 0`, pdf stays 0
        *pdf = mtrans_pdf(b, wo, wi);
        f = mtrans_f(b, wo, wi);
    } else if (pick == kLobePassThrough || pick == kLobeSpecTrans) {  // SpecularTransmission::Sample_f, reflection.cpp:154-170 (mode == Radiance)
        const float eta_a = 1.f, eta_b = pick == kLobePassThrough ? 1.f : b.eta;
        float scale;
        if (!specular_refract(wo, eta_a, eta_b, &wi, &scale)) return F3{0, 0, 0};  // `return 0`, pdf stays 0
        *pdf = 1;
        const F3 ft = (pick == kLobePassThrough ? b.t0 : b.kt) * (1.f - fr_dielectric(wi.z, eta_a, eta_b));
        f = sdiv(ft * scale, fabsf(wi.z));
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
            float scale;
            if (!specular_refract(wo, eta_a, eta_b, &wi, &scale)) return F3{0, 0, 0};  // total internal reflection: `return 0`, pdf stays 0
            const F3 ft = b.kt * (1 - F);
            *pdf = 1 - F;
            f = sdiv(ft * scale, fabsf(wi.z));
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
    const bool glossy = !lobe_is_specular(pick);
    if (glossy && matching > 1) {  // a specular lobe's Pdf() and f() are 0
        if (pick != kLobeLambert && b.has_lambert) *pdf += lambert_pdf(wo, wi);
        if (pick != kLobeLambertTrans && b.has_ltrans) *pdf += ltrans_pdf(wo, wi);
        if (pick != kLobeMicro && b.has_micro) *pdf += micro_pdf(b, wo, wi);
        if (pick != kLobeMicroTrans && b.has_mtrans) *pdf += mtrans_pdf(b, wo, wi);
    }
    if (matching > 1) *pdf /= matching;
    if (glossy && matching > 1) {
        bool reflect = dot(*wiW, b.ng) * dot(woW, b.ng) > 0;
        f = reflect ? lobes_f(b, wo, wi) : trans_lobes_f(b, wo, wi);
    }
    return f;
}

// ===========================================================================
// Disney (materials/disney.cpp) — the DIS builds of the kernels only
// ===========================================================================
// DisneyMaterial's BSDF holds up to eight BxDFs, five of them its own, and is much larger than every other material's: it lives in
// a struct of its own behind the Bsdf the other materials fill, and the overloads below (make_bsdf_at, bsdf_f, bsdf_pdf,
// bsdf_sample_f, n_nonspec on a DisneyBsdf) are what the DIS builds call. A hit on any other material goes through the functions
// above unchanged; the builds without DIS never see this struct. Its lobes, in the order the material adds them (the order
// BSDF::Sample_f counts them in and Pdf averages over), none of them tested for black:
//   DisneyDiffuse, DisneyFakeSS (thin), DisneyRetro, DisneySheen (sheen > 0) — these four iff diffuseWeight > 0 —
//   MicrofacetReflection (always), DisneyClearcoat (clearcoat > 0), MicrofacetTransmission (spectrans > 0), LambertianTransmission (thin)
// The base's fields carry what they already mean: micro_r = c, (alpha, alpha_y) = DisneyMicrofacetDistribution(ax, ay), eta,
// mtrans_t = spectrans sqrt(c), ltrans_t = difftrans / 2 c, has_micro / has_mtrans / has_ltrans, n_lobes; path_eta = 1 (BSDF(*si)).
enum DisneyLobe : int { kDzDiffuse, kDzFakeSS, kDzRetro, kDzSheen, kDzMicro, kDzCoat, kDzMicroTrans, kDzLambertTrans };
struct DisneyBsdf : Bsdf {
    bool disney;               // the hit's material is Disney's; false: the Bsdf above is all there is
    bool dz_diffuse;           // diffuseWeight > 0: DisneyDiffuse, DisneyRetro and, with the flags below, DisneyFakeSS / DisneySheen
    bool dz_thin, dz_sheen, dz_coat;
    bool dz_trans_smith;       // MicrofacetTransmission over a plain TrowbridgeReitzDistribution (thin): Smith's G, not the separable one
    F3 r_diffuse, r_ss, r_retro, r_sheen;   // the four diffuse-type lobes' R
    F3 cspec0;                 // DisneyFresnel(R0 = Cspec0, metallic, eta)
    float metallic, rough;     // (rough: DisneyFakeSS's and DisneyRetro's roughness, as given)
    float coat_w, coat_alpha;  // DisneyClearcoat(weight, gloss): alpha = Lerp(gloss, .1, .001)
    float t_ax, t_ay;          // MicrofacetTransmission's distribution: (alpha, alpha_y) again, or thin's pair from the scaled roughness
};
template <bool DIS>
struct bsdf_of { using type = Bsdf; };
template <>
struct bsdf_of<true> { using type = DisneyBsdf; };
DEV float lerpf(float t, float a, float b) { return (1 - t) * a + t * b; }   // Lerp, pbrt.h:315
DEV F3 lerp3(float t, F3 a, F3 b) { return (1 - t) * a + t * b; }            // Lerp, spectrum.h:482-484
DEV float sqr(float x) { return x * x; }
// SchlickWeight / FrSchlick / SchlickR0FromEta, disney.cpp:71-86
DEV float schlick_weight(float cos_theta) {
    const float m = clampf(1 - cos_theta, 0, 1);
    return (m * m) * (m * m) * m;
}
DEV float fr_schlick(float r0, float cos_theta) { return lerpf(schlick_weight(cos_theta), r0, 1.f); }
DEV F3 fr_schlick3(F3 r0, float cos_theta) { return lerp3(schlick_weight(cos_theta), r0, F3{1.f, 1.f, 1.f}); }
DEV float schlick_r0_from_eta(float eta) { return sqr(eta - 1) / sqr(eta + 1); }

// DisneyMaterial::ComputeScatteringFunctions, disney.cpp:475-588, with "scatterdistance" black and its ten scalar textures constants
// (dz); c and the roughness arrive looked up at the hit (textured_material: kd, alpha)
DEV void make_disney(const DMaterial &m, const iile_disney &dz, DisneyBsdf *b) {
    b->disney = true;
    b->mtype = kMatDisney;
    b->t0 = b->kd = F3{0, 0, 0};
    b->has_t0 = b->has_t1 = b->has_lambert = b->has_spec = b->has_blend = b->oren_nayar = false;
    b->on_a = 1.f, b->on_b = 0.f;
    b->path_eta = 1.f;   // BSDF(*si): eta = 1
    const F3 c = clamp0(m.kd);
    const float metallic_w = dz.metallic;
    const float e = m.eta;
    const float strans = dz.spec_trans;
    const float diffuse_w = (1 - metallic_w) * (1 - strans);
    const float dt = dz.diff_trans / 2;
    const float rough = m.alpha;
    const float lum = lum_y(c);
    const F3 one = F3{1.f, 1.f, 1.f};
    const F3 ctint = lum > 0 ? sdiv(c, lum) : one;
    const float sheen_w = dz.sheen;
    F3 csheen = F3{0, 0, 0};
    if (sheen_w > 0) csheen = lerp3(dz.sheen_tint, one, ctint);
    int n = 0;
    b->dz_thin = dz.thin != 0;
    b->dz_diffuse = diffuse_w > 0;
    b->dz_sheen = false;
    b->r_diffuse = b->r_ss = b->r_retro = b->r_sheen = F3{0, 0, 0};
    b->rough = rough;
    if (b->dz_diffuse) {
        if (b->dz_thin) {
            const float flat = dz.flatness;
            b->r_diffuse = (diffuse_w * (1 - flat) * (1 - dt)) * c;
            b->r_ss = (diffuse_w * flat * (1 - dt)) * c;
            n += 2;
        } else {
            b->r_diffuse = diffuse_w * c;
            ++n;
        }
        b->r_retro = diffuse_w * c;
        ++n;
        if (sheen_w > 0) {
            b->dz_sheen = true;
            b->r_sheen = (diffuse_w * sheen_w) * csheen;
            ++n;
        }
    }
    // `std::sqrt(1 - anisotropic * .9)`: the double overload
    const float aspect = float(sqrt(1. - double(dz.anisotropic) * .9));
    b->alpha = mx(.001f, sqr(rough) / aspect);
    b->alpha_y = mx(.001f, sqr(rough) * aspect);
    b->cspec0 = lerp3(metallic_w, schlick_r0_from_eta(e) * lerp3(dz.specular_tint, one, ctint), c);
    b->metallic = metallic_w;
    b->eta = e;
    b->micro_r = c;
    b->has_micro = true;
    ++n;
    b->dz_coat = dz.clearcoat > 0;
    b->coat_w = dz.clearcoat;
    b->coat_alpha = lerpf(dz.clearcoat_gloss, .1f, .001f);
    if (b->dz_coat) ++n;
    b->has_mtrans = strans > 0;
    b->mtrans_t = F3{0, 0, 0};
    b->t_ax = b->alpha, b->t_ay = b->alpha_y;
    b->dz_trans_smith = false;
    if (b->has_mtrans) {
        b->mtrans_t = strans * F3{sqrtf(c.x), sqrtf(c.y), sqrtf(c.z)};
        if (b->dz_thin) {  // the roughness scaled by the index of refraction, over a plain TrowbridgeReitzDistribution
            const float rscaled = (0.65f * e - 0.35f) * rough;
            b->t_ax = mx(.001f, sqr(rscaled) / aspect);
            b->t_ay = mx(.001f, sqr(rscaled) * aspect);
            b->dz_trans_smith = true;
        }
        ++n;
    }
    b->has_ltrans = b->dz_thin;
    b->ltrans_t = F3{0, 0, 0};
    if (b->dz_thin) {
        b->ltrans_t = dt * c;
        ++n;
    }
    b->n_lobes = n;
}
// The hit's BSDF in a DIS build: DisneyMaterial's, or the other materials' through make_bsdf. `material`: the material's index (its
// entry of the scene's Disney table is read for a Disney material only)
template <bool EXT, bool DIS>
DEV typename bsdf_of<DIS>::type make_bsdf_at(const DScene &S, int material, const DMaterial &m, const Isect &is) {
    if constexpr (!DIS) {
        return make_bsdf<EXT>(m, is);
    } else {
        DisneyBsdf b;
        if (m.type == kMatDisney) {
            b.ns = is.sn;
            b.ng = is.n;
            b.ss = normalize(is.sdpdu);
            b.ts = cross(b.ns, b.ss);
            make_disney(m, disney_table(S)[material], &b);
        } else {
            static_cast<Bsdf &>(b) = make_bsdf<EXT>(m, is);
            b.disney = false;
        }
        return b;
    }
}
DEV int n_nonspec(const DisneyBsdf &b) { return b.disney ? b.n_lobes : n_nonspec(static_cast<const Bsdf &>(b)); }   // (no Disney lobe is specular)
// DisneyDiffuse / DisneyFakeSS / DisneyRetro / DisneySheen ::f, disney.cpp:104-111, 138-154, 180-192, 218-225
DEV F3 dz_diffuse_f(F3 R, F3 wo, F3 wi) {
    const float Fo = schlick_weight(fabsf(wo.z)), Fi = schlick_weight(fabsf(wi.z));
    return R * kInvPi * (1 - Fo / 2) * (1 - Fi / 2);
}
DEV F3 dz_fakess_f(F3 R, float roughness, F3 wo, F3 wi) {
    F3 wh = wi + wo;
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return F3{0, 0, 0};
    wh = normalize(wh);
    const float cos_d = dot(wi, wh);
    const float Fss90 = cos_d * cos_d * roughness;
    const float Fo = schlick_weight(fabsf(wo.z)), Fi = schlick_weight(fabsf(wi.z));
    const float Fss = lerpf(Fo, 1.f, Fss90) * lerpf(Fi, 1.f, Fss90);
    const float ss = 1.25f * (Fss * (1 / (fabsf(wo.z) + fabsf(wi.z)) - .5f) + .5f);
    return R * kInvPi * ss;
}
DEV F3 dz_retro_f(F3 R, float roughness, F3 wo, F3 wi) {
    F3 wh = wi + wo;
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return F3{0, 0, 0};
    wh = normalize(wh);
    const float cos_d = dot(wi, wh);
    const float Fo = schlick_weight(fabsf(wo.z)), Fi = schlick_weight(fabsf(wi.z));
    const float Rr = 2 * roughness * cos_d * cos_d;
    return R * kInvPi * Rr * (Fo + Fi + Fo * Fi * (Rr - 1));
}
DEV F3 dz_sheen_f(F3 R, F3 wo, F3 wi) {
    F3 wh = wi + wo;
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return F3{0, 0, 0};
    wh = normalize(wh);
    return R * schlick_weight(dot(wi, wh));
}
// GTR1 / smithG_GGX, disney.cpp:251-262
DEV float gtr1(float cos_theta, float alpha) {
    const float alpha2 = alpha * alpha;
    return (alpha2 - 1) / (kPi * log_f(alpha2) * (1 + (alpha2 - 1) * cos_theta * cos_theta));
}
DEV float smith_g_ggx(float cos_theta, float alpha) {
    const float alpha2 = alpha * alpha;
    const float cos2 = cos_theta * cos_theta;
    return 1 / (cos_theta + sqrtf(alpha2 + cos2 - alpha2 * cos2));
}
// DisneyClearcoat::f / Pdf, disney.cpp:264-279, 305-318 (`.25 * weight * Gr * Fr * Dr` is a double product, rounded once)
DEV F3 dz_coat_f(const DisneyBsdf &b, F3 wo, F3 wi) {
    F3 wh = wi + wo;
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return F3{0, 0, 0};
    wh = normalize(wh);
    const float Dr = gtr1(fabsf(wh.z), b.coat_alpha);
    const float Fr = fr_schlick(.04f, dot(wo, wh));
    const float Gr = smith_g_ggx(fabsf(wo.z), .25f) * smith_g_ggx(fabsf(wi.z), .25f);
    const float v = float(.25 * double(b.coat_w) * double(Gr) * double(Fr) * double(Dr));
    return F3{v, v, v};
}
DEV float dz_coat_pdf(const DisneyBsdf &b, F3 wo, F3 wi) {
    if (!same_hemisphere(wo, wi)) return 0;
    F3 wh = wi + wo;
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return 0;
    wh = normalize(wh);
    const float Dr = gtr1(fabsf(wh.z), b.coat_alpha);
    return Dr / (4 * dot(wo, wh));
}
// MicrofacetReflection::f (reflection.cpp:226-236) with R = c, DisneyMicrofacetDistribution (G = G1(wo) G1(wi), disney.cpp:356-359)
// and DisneyFresnel::Evaluate (disney.cpp:334-337)
DEV F3 dz_micro_f(const DisneyBsdf &b, F3 wo, F3 wi) {
    const float cos_o = fabsf(wo.z), cos_i = fabsf(wi.z);
    F3 wh = wi + wo;
    if (cos_i == 0 || cos_o == 0) return F3{0, 0, 0};
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return F3{0, 0, 0};
    wh = normalize(wh);
    const float cos_h = dot(wi, wh);
    const float fd = fr_dielectric(cos_h, 1.f, b.eta);
    const F3 F = lerp3(b.metallic, F3{fd, fd, fd}, fr_schlick3(b.cspec0, cos_h));
    const float G = tr_g1(wo, b.alpha, b.alpha_y) * tr_g1(wi, b.alpha, b.alpha_y);
    return sdiv(b.micro_r * tr_d(wh, b.alpha, b.alpha_y) * G * F, 4 * cos_i * cos_o);
}
// MicrofacetTransmission::f / Pdf (reflection.cpp:244-266, 435-447) over the Disney BSDF's transmission distribution
DEV F3 dz_mtrans_f(const DisneyBsdf &b, F3 wo, F3 wi) {
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
    const float G = b.dz_trans_smith ? tr_g(wo, wi, b.t_ax, b.t_ay) : tr_g1(wo, b.t_ax, b.t_ay) * tr_g1(wi, b.t_ax, b.t_ay);
    return F3{omf, omf, omf} * b.mtrans_t *
           fabsf(tr_d(wh, b.t_ax, b.t_ay) * G * eta * eta * absdot(wi, wh) * absdot(wo, wh) * factor * factor /
                 (cos_i * cos_o * sqrt_denom * sqrt_denom));
}
DEV float dz_mtrans_pdf(const DisneyBsdf &b, F3 wo, F3 wi) {
    if (same_hemisphere(wo, wi)) return 0;
    const float eta_a = 1.f, eta_b = b.eta;
    const float eta = wo.z > 0 ? (eta_b / eta_a) : (eta_a / eta_b);
    const F3 wh = normalize(wo + wi * eta);
    const float sqrt_denom = dot(wo, wh) + eta * dot(wi, wh);
    const float dwh_dwi = fabsf((eta * eta * dot(wi, wh)) / (sqrt_denom * sqrt_denom));
    return tr_pdf(wo, wh, b.t_ax, b.t_ay) * dwh_dwi;
}
// one Disney lobe's f / Pdf
DEV F3 dz_lobe_f(const DisneyBsdf &b, DisneyLobe l, F3 wo, F3 wi) {
    switch (l) {
    case kDzDiffuse: return dz_diffuse_f(b.r_diffuse, wo, wi);
    case kDzFakeSS: return dz_fakess_f(b.r_ss, b.rough, wo, wi);
    case kDzRetro: return dz_retro_f(b.r_retro, b.rough, wo, wi);
    case kDzSheen: return dz_sheen_f(b.r_sheen, wo, wi);
    case kDzMicro: return dz_micro_f(b, wo, wi);
    case kDzCoat: return dz_coat_f(b, wo, wi);
    case kDzMicroTrans: return dz_mtrans_f(b, wo, wi);
    default: return ltrans_f(b);
    }
}
DEV bool dz_has(const DisneyBsdf &b, DisneyLobe l) {
    switch (l) {
    case kDzDiffuse:
    case kDzRetro: return b.dz_diffuse;
    case kDzFakeSS: return b.dz_diffuse && b.dz_thin;
    case kDzSheen: return b.dz_sheen;
    case kDzMicro: return true;
    case kDzCoat: return b.dz_coat;
    case kDzMicroTrans: return b.has_mtrans;
    default: return b.has_ltrans;
    }
}
// the sum of BSDF::f over the Disney lobes on wi's side (BSDF_REFLECTION: the first six; BSDF_TRANSMISSION: the last two), in BxDF order
DEV F3 dz_lobes_f(const DisneyBsdf &b, bool reflect, F3 wo, F3 wi) {
    F3 f = F3{0, 0, 0};
    if (reflect) {
        if (b.dz_diffuse) {
            f = f + dz_diffuse_f(b.r_diffuse, wo, wi);
            if (b.dz_thin) f = f + dz_fakess_f(b.r_ss, b.rough, wo, wi);
            f = f + dz_retro_f(b.r_retro, b.rough, wo, wi);
            if (b.dz_sheen) f = f + dz_sheen_f(b.r_sheen, wo, wi);
        }
        f = f + dz_micro_f(b, wo, wi);
        if (b.dz_coat) f = f + dz_coat_f(b, wo, wi);
    } else {
        if (b.has_mtrans) f = f + dz_mtrans_f(b, wo, wi);
        if (b.has_ltrans) f = f + ltrans_f(b);
    }
    return f;
}
// the sum of the Disney lobes' Pdf in BxDF order, `skip` left out (-1: none). The four diffuse-type lobes have BxDF::Pdf, the
// cosine density on wo's side (reflection.cpp:387-389): it enters once per such lobe.
DEV float dz_lobes_pdf(const DisneyBsdf &b, int skip, F3 wo, F3 wi, float pdf) {
    const float cosine = lambert_pdf(wo, wi);
#pragma unroll
    for (int l = kDzDiffuse; l <= kDzSheen; ++l)
        if (l != skip && dz_has(b, DisneyLobe(l))) pdf += cosine;
    if (skip != kDzMicro) pdf += micro_pdf(b, wo, wi);
    if (skip != kDzCoat && b.dz_coat) pdf += dz_coat_pdf(b, wo, wi);
    if (skip != kDzMicroTrans && b.has_mtrans) pdf += dz_mtrans_pdf(b, wo, wi);
    if (skip != kDzLambertTrans && b.has_ltrans) pdf += ltrans_pdf(wo, wi);
    return pdf;
}
// BSDF::f / Pdf / Sample_f (reflection.cpp:686-699, 786-801, 719-784) in a DIS build
DEV F3 bsdf_f(const DisneyBsdf &b, F3 woW, F3 wiW) {
    if (!b.disney) return bsdf_f(static_cast<const Bsdf &>(b), woW, wiW);
    const F3 wi = to_local(b, wiW), wo = to_local(b, woW);
    if (wo.z == 0) return F3{0, 0, 0};
    const bool reflect = dot(wiW, b.ng) * dot(woW, b.ng) > 0;
    return dz_lobes_f(b, reflect, wo, wi);
}
DEV float bsdf_pdf(const DisneyBsdf &b, F3 woW, F3 wiW) {
    if (!b.disney) return bsdf_pdf(static_cast<const Bsdf &>(b), woW, wiW);
    const F3 wo = to_local(b, woW), wi = to_local(b, wiW);
    if (wo.z == 0) return 0.f;
    return dz_lobes_pdf(b, -1, wo, wi, 0.f) / b.n_lobes;   // (n_lobes >= 1: MicrofacetReflection is always there)
}
DEV F3 bsdf_sample_f(const DisneyBsdf &b, F3 woW, F3 *wiW, float u0, float u1, float *pdf, const bool allow_specular = false,
                     bool *sampled_specular = nullptr, bool *sampled_transmission = nullptr) {
    if (!b.disney) return bsdf_sample_f(static_cast<const Bsdf &>(b), woW, wiW, u0, u1, pdf, allow_specular, sampled_specular, sampled_transmission);
    if (sampled_specular) *sampled_specular = false;
    if (sampled_transmission) *sampled_transmission = false;
    const int matching = b.n_lobes;
    int comp = int(floorf(u0 * matching));
    if (comp > matching - 1) comp = matching - 1;
    // the comp-th present lobe in BxDF order
    int pick = kDzLambertTrans, count = comp;
    bool found = false;
#pragma unroll
    for (int l = kDzDiffuse; l <= kDzLambertTrans; ++l)
        if (!found && dz_has(b, DisneyLobe(l)) && count-- == 0) pick = l, found = true;
    const float ur0 = mn(u0 * matching - comp, kOneMinusEpsilon);
    const F3 wo = to_local(b, woW);
    if (wo.z == 0) return F3{0, 0, 0};
    *pdf = 0;
    F3 wi = F3{0, 0, 0}, f;
    if (pick <= kDzSheen) {  // BxDF::Sample_f, reflection.cpp:378-385
        wi = cosine_sample_hemisphere(ur0, u1);
        if (wo.z < 0) wi.z *= -1;
        *pdf = lambert_pdf(wo, wi);
        f = dz_lobe_f(b, DisneyLobe(pick), wo, wi);
    } else if (pick == kDzMicro) {  // MicrofacetReflection::Sample_f, reflection.cpp:405-417
        const F3 wh = tr_sample_wh(wo, ur0, u1, b.alpha, b.alpha_y);
        wi = -wo + 2 * dot(wo, wh) * wh;
        if (!same_hemisphere(wo, wi))
            f = F3{0, 0, 0};
        else {
            *pdf = tr_pdf(wo, wh, b.alpha, b.alpha_y) / (4 * dot(wo, wh));
            f = dz_micro_f(b, wo, wi);
        }
    } else if (pick == kDzCoat) {  // DisneyClearcoat::Sample_f, disney.cpp:281-303: alpha fixed at .25
        const float alpha2 = .25f * .25f;
        const float cos_t = sqrtf(mx(0.f, (1 - powf(alpha2, 1 - ur0)) / (1 - alpha2)));
        const float sin_t = sqrtf(mx(0.f, 1 - cos_t * cos_t));
        const float phi = 2 * kPi * u1;
        float sp, cp;
        sincos_f(phi, &sp, &cp);
        F3 wh = F3{sin_t * cp, sin_t * sp, cos_t};   // SphericalDirection, geometry.h:1427-1431
        if (!same_hemisphere(wo, wh)) wh = -wh;
        wi = -wo + 2 * dot(wo, wh) * wh;
        if (!same_hemisphere(wo, wi))
            f = F3{0, 0, 0};   // `return Spectrum(0.f)`, *pdf untouched
        else {
            *pdf = dz_coat_pdf(b, wo, wi);
            f = dz_coat_f(b, wo, wi);
        }
    } else if (pick == kDzMicroTrans) {  // MicrofacetTransmission::Sample_f, reflection.cpp:425-433
        const F3 wh = tr_sample_wh(wo, ur0, u1, b.t_ax, b.t_ay);
        const float eta_a = 1.f, eta_b = b.eta;
        const float eta = wo.z > 0 ? (eta_a / eta_b) : (eta_b / eta_a);
        if (!refract_dir(wo, wh, eta, &wi)) return F3{0, 0, 0};  // `return 0`, pdf stays 0
        *pdf = dz_mtrans_pdf(b, wo, wi);
        f = dz_mtrans_f(b, wo, wi);
    } else {  // LambertianTransmission::Sample_f, reflection.cpp:391-398
        wi = cosine_sample_hemisphere(ur0, u1);
        if (wo.z > 0) wi.z *= -1;
        *pdf = ltrans_pdf(wo, wi);
        f = ltrans_f(b);
    }
    if (*pdf == 0) return F3{0, 0, 0};
    *wiW = to_world(b, wi);
    if (matching > 1) {
        *pdf = dz_lobes_pdf(b, pick, wo, wi, *pdf);
        *pdf /= matching;
        const bool reflect = dot(*wiW, b.ng) * dot(woW, b.ng) > 0;
        f = dz_lobes_f(b, reflect, wo, wi);
    }
    if (sampled_transmission) *sampled_transmission = false;   // (read only together with sampled_specular: path.cpp:151)
    return f;
}
