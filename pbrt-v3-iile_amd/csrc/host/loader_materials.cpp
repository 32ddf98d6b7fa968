// loader_materials.cpp — the `Material` / `MakeNamedMaterial` directives. What the loader knows about a material is one row of
// material_rows() and the function that fills its scalars; make_material derives the rest from the row (pbrt_loader.h).
#include "pbrt_loader.h"

namespace iile {

namespace {

// TrowbridgeReitzDistribution::RoughnessToAlpha, microfacet.h:123-128
float roughness_to_alpha(float roughness) {
    roughness = std::max(roughness, 1e-3f);
    const float x = std::log(roughness);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}

// "remaproughness", and the alphas of roughness / roughness_v under it. The reference re-evaluates them per hit (plastic.cpp:61-63,
// uber.cpp:79-84, translucent.cpp:68-70); they are per-material constants, so they are evaluated once here
void remap_alphas(const ParamSet &ps, iile_material *m) {
    m->remap_roughness = ps.one_bool("remaproughness", true) ? 1 : 0;
    m->alpha = m->remap_roughness ? roughness_to_alpha(m->roughness) : m->roughness;
    m->alpha_v = m->remap_roughness ? roughness_to_alpha(m->roughness_v) : m->roughness_v;
}

float eta_or_index(const ParamSet &ps) { return ps.find("eta") ? ps.one_float("eta", 1.5f) : ps.one_float("index", 1.5f); }

void fill_matte(const ParamSet &ps, iile_material *m, iile_disney *) {  // CreateMatteMaterial, matte.cpp:64-71
    m->sigma = clampT(ps.one_float("sigma", 0.f), 0.f, 90.f);  // matte.cpp:56
    if (m->sigma != 0.f) {  // OrenNayar ctor, reflection.h:414-420
        const float sg = radians(m->sigma);
        const float sigma2 = sg * sg;
        m->on_a = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
        m->on_b = 0.45f * sigma2 / (sigma2 + 0.09f);
    }
}

void fill_plastic(const ParamSet &ps, iile_material *m, iile_disney *) {  // CreatePlasticMaterial, plastic.cpp:72-84
    m->roughness = m->roughness_v = ps.one_float("roughness", .1f);
    remap_alphas(ps, m);
}

void fill_uber(const ParamSet &ps, iile_material *m, iile_disney *) {  // CreateUberMaterial, uber.cpp:102-127
    // uber.cpp:73-86: roughu = uroughness or roughness, roughv = vroughness or roughu (numbers here; images: roughness_images)
    m->roughness = ps.one_float("uroughness", ps.one_float("roughness", .1f));
    m->roughness_v = ps.one_float("vroughness", m->roughness);
    m->eta = eta_or_index(ps);
    remap_alphas(ps, m);
}

void fill_mirror(const ParamSet &, iile_material *, iile_disney *) {}  // CreateMirrorMaterial, mirror.cpp:57-63: "Kr" alone

void fill_glass(const ParamSet &ps, iile_material *m, iile_disney *) {  // CreateGlassMaterial, glass.cpp:94-113
    m->eta = eta_or_index(ps);
    // glass.cpp:52-73: urough == vrough == 0 is the smooth dielectric; otherwise MicrofacetReflection + MicrofacetTransmission over
    // one TrowbridgeReitzDistribution(RoughnessToAlpha(urough), ...(vrough))
    m->roughness = ps.one_float("uroughness", 0.f);
    m->roughness_v = ps.one_float("vroughness", 0.f);
    const bool specular = m->roughness == 0.f && m->roughness_v == 0.f;  // `bool isSpecular = urough == 0 && vrough == 0`, glass.cpp:63
    remap_alphas(ps, m);
    if (specular) m->alpha = m->alpha_v = 0.f;
}

void fill_metal(const ParamSet &ps, iile_material *m, iile_disney *) {  // CreateMetalMaterial, metal.cpp:104-127
    // uRough = uRoughness ? uRoughness : roughness, vRough = vRoughness ? vRoughness : roughness (metal.cpp:68-71): each
    // falls back to "roughness" on its own (images: roughness_images)
    const float r = ps.one_float("roughness", .01f);
    m->roughness = ps.one_float("uroughness", r);
    m->roughness_v = ps.one_float("vroughness", r);
    remap_alphas(ps, m);
}

void fill_substrate(const ParamSet &ps, iile_material *m, iile_disney *) {  // CreateSubstrateMaterial, substrate.cpp:81-96
    // "uroughness" / "vroughness", each .1 by default; "roughness" is not looked at
    m->roughness = ps.one_float("uroughness", .1f);
    m->roughness_v = ps.one_float("vroughness", .1f);
    remap_alphas(ps, m);
}

void fill_translucent(const ParamSet &ps, iile_material *m, iile_disney *) {  // CreateTranslucentMaterial, translucent.cpp:82-98
    m->eta = 1.5f;  // translucent.cpp:50
    m->roughness = m->roughness_v = ps.one_float("roughness", .1f);  // TrowbridgeReitzDistribution(rough, rough)
    remap_alphas(ps, m);
}

void fill_disney(const ParamSet &ps, iile_material *m, iile_disney *dz) {  // CreateDisneyMaterial, disney.cpp:590-624
    m->eta = ps.one_float("eta", 1.5f);
    // the roughness as given: DisneyMaterial squares it into the distribution's alphas at the hit and never remaps
    m->roughness = m->roughness_v = m->alpha = m->alpha_v = ps.one_float("roughness", .5f);
    m->remap_roughness = 0;
    dz->metallic = ps.one_float("metallic", 0.f);
    dz->specular_tint = ps.one_float("speculartint", 0.f);
    dz->anisotropic = ps.one_float("anisotropic", 0.f);
    dz->sheen = ps.one_float("sheen", 0.f);
    dz->sheen_tint = ps.one_float("sheentint", .5f);
    dz->clearcoat = ps.one_float("clearcoat", 0.f);
    dz->clearcoat_gloss = ps.one_float("clearcoatgloss", 1.f);
    dz->spec_trans = ps.one_float("spectrans", 0.f);
    dz->flatness = ps.one_float("flatness", 0.f);
    dz->diff_trans = ps.one_float("difftrans", 1.f);
    dz->thin = ps.one_bool("thin", false) ? 1 : 0;
}

#define GREY(x) {x, x, x}

}  // namespace

// The materials, in the order the "is not supported" message names them. A spectrum parameter: name, default, constant, image
// slot, whether "spectrum" / "blackbody" are refused by name. Adding a material is adding a row and its fill function.
const std::vector<MaterialRow> &Loader::material_rows() {
    typedef iile_material M;
    static const std::vector<MaterialRow> rows = {
        {"matte", IILE_MAT_MATTE, {{"Kd", GREY(.5f), &M::kd, &M::kd_tex, false}}, ROUGH_NONE, true, true, fill_matte, nullptr},
        {"plastic", IILE_MAT_PLASTIC, {{"Kd", GREY(.25f), &M::kd, &M::kd_tex, false}, {"Ks", GREY(.25f), &M::ks, &M::ks_tex, false}},
         ROUGH_ONE, true, false, fill_plastic, nullptr},
        {"uber", IILE_MAT_UBER,
         {{"Kd", GREY(.25f), &M::kd, &M::kd_tex, false}, {"Ks", GREY(.25f), &M::ks, &M::ks_tex, false},
          {"Kr", GREY(0.f), &M::kr, &M::kr_tex, false}, {"Kt", GREY(0.f), &M::kt, &M::kt_tex, false},
          {"opacity", GREY(1.f), &M::opacity, &M::opacity_tex, false}},  // GetSpectrumTexture("opacity", 1.f), uber.cpp:117
         ROUGH_UBER, true, false, fill_uber, nullptr},
        {"mirror", IILE_MAT_MIRROR, {{"Kr", GREY(.9f), &M::kr, &M::kr_tex, false}}, ROUGH_NONE, true, false, fill_mirror, nullptr},
        {"glass", IILE_MAT_GLASS, {{"Kr", GREY(1.f), &M::kr, &M::kr_tex, false}, {"Kt", GREY(1.f), &M::kt, &M::kt_tex, false}},
         ROUGH_NUMBERS, false, false, fill_glass, nullptr},
        // "eta" / "k": rgb, color or a constant named texture. The defaults are RGBSpectrum::FromSampled(CopperWavelengths,
        // CopperN / CopperK, CopperSamples) (metal.cpp:108-116), worked out in float64 from the reference's tables and rounded to
        // float (tests/golden/make_copper_fixture.py, copper_fixture.json)
        {"metal", IILE_MAT_METAL,
         {{"eta", {0.199989721f, 0.922085762f, 1.09987628f}, &M::cond_eta, nullptr, true},
          {"k", {3.90463829f, 2.44763327f, 2.13765097f}, &M::cond_k, nullptr, true}},
         ROUGH_METAL, true, false, fill_metal, nullptr},
        {"disney", IILE_MAT_DISNEY, {{"color", GREY(.5f), &M::kd, &M::kd_tex, true}}, ROUGH_ONE, true, false, fill_disney,
         &Loader::refuse_disney_forms},
        {"substrate", IILE_MAT_SUBSTRATE, {{"Kd", GREY(.5f), &M::kd, &M::kd_tex, false}, {"Ks", GREY(.5f), &M::ks, &M::ks_tex, false}},
         ROUGH_SUBSTRATE, true, false, fill_substrate, nullptr},
        {"translucent", IILE_MAT_TRANSLUCENT,
         {{"Kd", GREY(.25f), &M::kd, &M::kd_tex, true}, {"Ks", GREY(.25f), &M::ks, &M::ks_tex, true},
          {"reflect", GREY(.5f), &M::kr, &M::kr_tex, true}, {"transmit", GREY(.5f), &M::kt, &M::kt_tex, true}},
         ROUGH_ONE, true, false, fill_translucent, nullptr},
    };
    return rows;
}
#undef GREY

// The forms of its spectrum parameters that pbrt-v3 takes and this loader does not, refused by name before the textures resolve
bool Loader::refuse_parameter_forms(const MaterialRow &row, const ParamSet &ps) {
    for (const SpectrumParam &sp : row.spectra) {
        const Param *p = ps.find(sp.name);
        if (!p) continue;
        const std::string what = std::string("Material \"") + row.name + "\": parameter \"" + sp.name + "\" given as ";
        const char *taken = sp.image ? "\" is not supported (rgb, color or a texture)" : "\" is not supported (rgb, color or a constant texture)";
        if (sp.refuse_sampled && (p->type == "spectrum" || p->type == "blackbody")) return fail(what + "\"" + p->type + taken);
        const ConstTexture *t = named_texture(p);
        if (!sp.image && t && t->image >= 0) return fail(what + "the image texture \"" + p->strs[0] + taken);
    }
    return !row.refuse || (this->*row.refuse)(ps);
}

// what CreateDisneyMaterial takes and this loader does not
bool Loader::refuse_disney_forms(const ParamSet &ps) {
    // the ten scalar parameters: a number or a constant texture (they ride in iile_disney, one value per material)
    for (const char *param : {"metallic", "eta", "speculartint", "anisotropic", "sheen", "sheentint", "clearcoat", "clearcoatgloss",
                              "spectrans", "flatness", "difftrans"}) {
        const Param *p = ps.find(param);
        const ConstTexture *t = named_texture(p);
        if (t && t->image >= 0)
            return fail(std::string("Material \"disney\": parameter \"") + param + "\" given as the texture \"" + p->strs[0] +
                        "\" is not supported (a number or a constant texture)");
    }
    // "scatterdistance" other than black selects the BSSRDF branch (disney.cpp:515-527): a subsurface walk this renderer lacks.
    // A thin surface never evaluates it (disney.cpp:506-513): there it is ignored, like any parameter that is not read
    if (const Param *p = ps.one_bool("thin", false) ? nullptr : ps.find("scatterdistance")) {
        bool black = p->type == "rgb" || p->type == "color" || p->type == "texture";
        for (double v : p->nums) black = black && v == 0;
        if (p->type == "texture") {
            const ConstTexture *t = named_texture(p);
            black = t && t->image < 0 && t->v[0] == 0 && t->v[1] == 0 && t->v[2] == 0;
        }
        if (!black)
            return fail("Material \"disney\": a \"scatterdistance\" that is not black is not supported (it selects the BSSRDF, which needs a "
                        "subsurface walk)");
    }
    return true;
}

// Float images for the roughness parameters (resolve_textures has made them "roughimage" parameters): which of them the material
// takes, and where each goes. rough_tex_v is -2 where alpha_v follows alpha, -1 where it is the constant, else an image
bool Loader::roughness_images(const MaterialRow &row, const ParamSet &ps, const std::map<std::string, int> &image_of, iile_material *m) {
    const Param *rp = ps.find("roughness"), *up = ps.find("uroughness"), *vp = ps.find("vroughness");
    auto image = [&](const char *name, const Param *p) { return p && p->type == "roughimage" ? image_of.at(name) : -1; };
    const int r = image("roughness", rp), u = image("uroughness", up), v = image("vroughness", vp);
    const bool uv = row.rough == ROUGH_UBER || row.rough == ROUGH_METAL || row.rough == ROUGH_SUBSTRATE;
    if ((r >= 0 && !uv && row.rough != ROUGH_ONE) || ((u >= 0 || v >= 0) && !uv))
        return fail("roughness: a float \"imagemap\" texture is supported on plastic, translucent and disney (\"roughness\"), uber and metal "
                    "(\"roughness\", \"uroughness\", \"vroughness\") and substrate (\"uroughness\", \"vroughness\") only");
    switch (row.rough) {
    case ROUGH_NONE: break;
    case ROUGH_NUMBERS: m->rough_tex_v = -1; break;  // glass.cpp:102-104: u and v, numbers only here
    case ROUGH_ONE: m->rough_tex = r; break;         // "roughness" alone
    case ROUGH_UBER:  // roughu = uroughness ? uroughness : roughness, roughv = vroughness ? vroughness : roughu (uber.cpp:79-86):
                      // "roughness" is not looked at when "uroughness" is there
        m->rough_tex = up ? u : r;
        m->rough_tex_v = vp ? v : -2;
        break;
    case ROUGH_METAL:  // metal.cpp:68-71: each of u and v is its own parameter if given, else "roughness"
        m->rough_tex = up ? u : r;
        m->rough_tex_v = vp ? v : r;
        break;
    case ROUGH_SUBSTRATE:  // substrate ignores "roughness", substrate.cpp:88-91
        m->rough_tex = u;
        m->rough_tex_v = v;
        break;
    }
    return true;
}

bool Loader::make_material(const std::string &name, const ParamSet &ps_in, int *index) {
    const MaterialRow *row = nullptr;
    std::string known;
    for (const MaterialRow &r : material_rows()) {
        if (name == r.name) row = &r;
        known += (known.empty() ? "" : ", ") + std::string(r.name);
    }
    if (row && !refuse_parameter_forms(*row, ps_in)) return false;
    ParamSet ps;
    std::map<std::string, int> image_of;
    if (!resolve_textures(ps_in, row, &ps, &image_of)) return false;
    if (!row) return fail("Material \"" + name + "\" is not supported (" + known + ")");
    auto image = [&](const char *param) {
        auto it = image_of.find(param);
        return it == image_of.end() ? -1 : it->second;
    };
    iile_disney dz;
    std::memset(&dz, 0, sizeof(dz));
    iile_material m;
    std::memset(&m, 0, sizeof(m));
    m.type = row->type;
    m.kd_tex = m.ks_tex = m.kr_tex = m.kt_tex = m.bump_tex = m.rough_tex = m.sigma_tex = m.opacity_tex = -1;
    m.rough_tex_v = -2;  // alpha_v follows alpha
    m.opacity[0] = m.opacity[1] = m.opacity[2] = 1.f;
    // each spectrum parameter: its default, the value given, its image (an image given for a parameter the material does not have
    // is ignored, as a constant would be)
    for (const SpectrumParam &sp : row->spectra) {
        float *value = m.*(sp.value);
        for (int i = 0; i < 3; ++i) value[i] = sp.def[i];
        ps.rgb(sp.name, value);
        if (sp.image) m.*(sp.image) = image(sp.name);
    }
    row->fill(ps, &m, &dz);
    if (const Param *sp = ps.find("sigma"))
        if (sp->type == "sigmaimage") {
            if (!row->sigma) return fail("sigma: a float \"imagemap\" texture is supported on matte only");
            m.sigma_tex = image("sigma");
        }
    if (!roughness_images(*row, ps, image_of, &m)) return false;
    if (const Param *bp = ps.find("bumpmap")) {  // GetFloatTextureOrNull("bumpmap") of every material's Create*
        if (bp->type != "bumpimage" || !row->bump)
            return fail("bumpmap: only a float \"imagemap\" texture on matte / plastic / uber / mirror / metal / substrate / translucent / disney is supported");
        m.bump_tex = image("bumpmap");
    }
    scene_->materials.push_back(m);
    scene_->disney.resize(scene_->materials.size() - 1);
    scene_->disney.push_back(dz);
    *index = int(scene_->materials.size()) - 1;
    return true;
}

int Loader::current_material() {
    if (gs_.material >= 0) return gs_.material;
    if (default_material_ < 0 && !make_material("matte", ParamSet(), &default_material_)) return -1;
    return default_material_;
}

}  // namespace iile
