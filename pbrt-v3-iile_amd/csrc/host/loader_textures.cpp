// loader_textures.cpp — the `Texture` directive (one function per texture class) and how a material's parameters see the
// named textures (pbrt_loader.h).
#include <cstdio>

#include "pbrt_loader.h"

namespace iile {

namespace {

const float kZero[3] = {0, 0, 0}, kOne[3] = {1, 1, 1}, kHalf[3] = {.5f, .5f, .5f};

// TextureParams::FindVector3f (a "vector" / "vector3" parameter of three numbers)
V3 find_vector(const ParamSet &ps, const std::string &name, V3 def) {
    const Param *p = ps.find(name);
    if (p && p->type == "vector" && p->nums.size() == 3) return V3(float(p->nums[0]), float(p->nums[1]), float(p->nums[2]));
    return def;
}

iile_texture blank_texture(int kind) {
    iile_texture pt;
    std::memset(&pt, 0, sizeof(pt));
    pt.kind = kind;
    pt.child[0] = pt.child[1] = pt.child[2] = -1;
    return pt;
}

}  // namespace

// materials/matte.cpp:64-71, plastic.cpp:72-84, microfacet.h:123-128
// value of a float / spectrum parameter that may be given directly or as a reference to a named
// texture (TextureParams::GetFloatTexture / GetSpectrumTexture, paramset.cpp)
bool Loader::tex_value(const ParamSet &ps, const std::string &name, bool want_float, const float def[3], float out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = def[i];
    const Param *p = ps.find(name);
    if (!p) return true;
    if (p->type == "texture") {
        if (p->strs.size() != 1) return fail("bad texture reference for \"" + name + "\"");
        const ConstTexture *t = named_texture(p);
        if (!t || t->is_float != want_float)
            return fail(std::string("Couldn't find ") + (want_float ? "float" : "spectrum") + " texture named \"" +
                        p->strs[0] + "\" for parameter \"" + name + "\"");
        if (t->image >= 0)
            return fail("texture \"" + p->strs[0] + "\": scale / mix of image textures is not supported");
        for (int i = 0; i < 3; ++i) out[i] = t->v[i];
        return true;
    }
    if (want_float) {
        if (p->type == "float" && p->nums.size() == 1) out[0] = out[1] = out[2] = float(p->nums[0]);
    } else
        ps.rgb(name, out);
    return true;
}

// "scale" with exactly one plain spectrum image texture among tex1 / tex2 and a constant for the other
bool Loader::scale_of_image(const ParamSet &ps, ConstTexture *t) {
    const char *names[2] = {"tex1", "tex2"};
    int which = -1;
    for (int k = 0; k < 2; ++k) {
        const ConstTexture *in = named_texture(ps.find(names[k]));
        if (!in) continue;
        if (in->image >= 0 && !in->is_float && scene_->textures[size_t(in->image)].t.kind != IILE_TEX_IMAGE)
            return false;  // a procedural input: a combiner, not this fold
        if (in->image < 0 || in->is_float || in->scaled) continue;
        if (which >= 0) return false;  // two images: not folded
        which = k;
        t->image = in->image;
    }
    if (which < 0) return false;
    ParamSet rest;
    for (const Param &p : ps.params)
        if (p.name != names[which]) rest.params.push_back(p);
    float c[3];
    if (!tex_value(rest, names[1 - which], false, kOne, c)) {
        t->image = -1;
        return false;
    }
    for (int i = 0; i < 3; ++i) t->v[i] = c[i];
    t->scaled = true;
    t->leaf = false;  // a combination (image times factor): a combiner over it would be a third level, and would drop the factor
    return true;
}

// an input of a procedural texture (TextureParams::GetFloatTexture / GetSpectrumTexture): a constant (given directly, a
// constant named texture, or the default) goes to *val with *idx = -1; a named leaf texture gives its index
bool Loader::tex_input(const std::string &tex_name, const ParamSet &ps, const std::string &name, bool want_float, const float def[3],
                       int *idx, float val[3]) {
    *idx = -1;
    const Param *p = ps.find(name);
    const ConstTexture *in = named_texture(p);
    if (in && in->is_float == want_float && in->image >= 0) {
        if (!in->leaf)
            return fail("Texture \"" + tex_name + "\": input \"" + name + "\" is \"" + p->strs[0] +
                        "\", itself a combination of textures; textures nest two levels deep at most");
        *idx = in->image;
        for (int i = 0; i < 3; ++i) val[i] = 0.f;
        return true;
    }
    return tex_value(ps, name, want_float, def, val);
}

// whether one of `inputs` (parameter name, float?) names a texture that is not a constant
bool Loader::has_texture_input(const ParamSet &ps, std::initializer_list<std::pair<const char *, bool>> inputs) const {
    for (const auto &in : inputs) {
        const ConstTexture *t = named_texture(ps.find(in.first));
        if (t && t->is_float == in.second && t->image >= 0) return true;
    }
    return false;
}

// the upper 3 x 4 of an affine matrix (the bottom row (0, 0, 0, 1))
bool Loader::affine_3x4(const Mat4 &m, const std::string &tex_name, float out[12]) {
    if (m.m[3][0] != 0.f || m.m[3][1] != 0.f || m.m[3][2] != 0.f || m.m[3][3] != 1.f)
        return fail("Texture \"" + tex_name + "\": a projective texture transform is not supported");
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) out[4 * r + c] = m.m[r][c];
    return true;
}

// the TextureMapping2D of the 2D classes (checkerboard.cpp:55-76 and the same code in uv.cpp, bilerp.cpp)
bool Loader::mapping_2d(const std::string &tex_name, const ParamSet &ps, iile_texture *t) {
    const std::string type = ps.one_string("mapping", "uv");
    t->su = 1.f, t->sv = 1.f, t->du = 0.f, t->dv = 0.f;
    if (type == "uv") {
        t->mapping = IILE_MAP_UV;
        t->su = ps.one_float("uscale", 1.f);
        t->sv = ps.one_float("vscale", 1.f);
        t->du = ps.one_float("udelta", 0.f);
        t->dv = ps.one_float("vdelta", 0.f);
    } else if (type == "spherical" || type == "cylindrical") {  // Inverse(tex2world): the CTM's inverse
        t->mapping = type == "spherical" ? IILE_MAP_SPHERICAL : IILE_MAP_CYLINDRICAL;
        if (!affine_3x4(ctm().inv, tex_name, t->xf)) return false;
    } else if (type == "planar") {
        t->mapping = IILE_MAP_PLANAR;
        const V3 v1 = find_vector(ps, "v1", V3(1, 0, 0)), v2 = find_vector(ps, "v2", V3(0, 1, 0));
        t->vs[0] = v1.x, t->vs[1] = v1.y, t->vs[2] = v1.z;
        t->vt[0] = v2.x, t->vt[1] = v2.y, t->vt[2] = v2.z;
        t->du = ps.one_float("udelta", 0.f);
        t->dv = ps.one_float("vdelta", 0.f);
    } else {  // Error(...) and a default UVMapping2D
        std::fprintf(stderr, "Error: 2D texture mapping \"%s\" unknown\n", type.c_str());
        t->mapping = IILE_MAP_UV;
    }
    return true;
}

// a procedural entry of HostScene::textures (n_levels = 0, no texels); t becomes a reference to it
void Loader::add_procedural(const iile_texture &pt, bool leaf, ConstTexture *t) {
    HostTexture ht;
    ht.t = pt;
    scene_->textures.push_back(std::move(ht));
    t->image = int(scene_->textures.size()) - 1;
    t->leaf = leaf;
}

bool Loader::make_texture(const std::string &name, const std::string &type, const std::string &cls, const ParamSet &ps) {
    ConstTexture t;
    t.is_float = type == "float";
    if (!t.is_float && type != "spectrum" && type != "color") return fail("Texture type \"" + type + "\" unknown.");
    warn_if_animated("Texture");  // pbrtTexture, api.cpp:1249, 1267: Make*Texture gets curTransform[0]
    bool ok;
    if (cls == "constant")  // CreateConstant*Texture, textures/constant.cpp: "value" default 1
        ok = tex_value(ps, "value", t.is_float, kOne, t.v);
    else if (cls == "scale" || cls == "mix")
        ok = scale_or_mix_texture(name, cls == "mix", ps, &t);
    else if (cls == "checkerboard")
        ok = checkerboard_texture(name, ps, &t);
    else if (cls == "uv")
        ok = uv_texture(name, ps, &t);
    else if (cls == "bilerp")
        ok = bilerp_texture(name, ps, &t);
    else if (cls == "imagemap")
        ok = imagemap_texture(name, ps, &t);
    else if (cls == "fbm" || cls == "wrinkled" || cls == "windy" || cls == "marble" || cls == "dots")
        return fail("Texture class \"" + cls + "\" is not supported (it needs pbrt's noise permutation table)");
    else if (cls == "ptex")
        return fail("Texture class \"ptex\" is not supported (it needs the Ptex library)");
    else
        return fail("Texture class \"" + cls + "\" is not supported (constant, scale, mix, imagemap, checkerboard, uv, bilerp)");
    if (ok) gs_.textures[name] = t;
    return ok;
}

bool Loader::scale_or_mix_texture(const std::string &name, bool mix, const ParamSet &ps, ConstTexture *t) {
    const bool is_float = t->is_float;
    // an image texture times a constant: kept as (image, factor); the product is taken at the hit
    if (!mix && !is_float && scale_of_image(ps, t)) return true;
    // a texture among the inputs: a combiner entry. ScaleTexture / MixTexture over non-constant inputs (scale.cpp:42-53,
    // mix.cpp:42-55) are evaluated at the hit
    if (mix ? has_texture_input(ps, {{"tex1", is_float}, {"tex2", is_float}, {"amount", true}})
            : has_texture_input(ps, {{"tex1", is_float}, {"tex2", is_float}})) {
        iile_texture pt = blank_texture(mix ? IILE_TEX_MIX : IILE_TEX_SCALE);
        if (!tex_input(name, ps, "tex1", is_float, mix ? kZero : kOne, &pt.child[0], pt.cval[0]) ||
            !tex_input(name, ps, "tex2", is_float, kOne, &pt.child[1], pt.cval[1]))
            return false;
        if (mix && !tex_input(name, ps, "amount", true, kHalf, &pt.child[2], pt.cval[2])) return false;
        add_procedural(pt, false, t);
        return true;
    }
    // constant inputs fold, as they always have
    float a[3], b[3], amt[3];
    if (!tex_value(ps, "tex1", is_float, mix ? kZero : kOne, a) || !tex_value(ps, "tex2", is_float, kOne, b)) return false;
    if (!mix) {  // ScaleTexture::Evaluate = tex1 * tex2, textures/scale.h:56-58 (defaults 1, 1)
        for (int i = 0; i < 3; ++i) t->v[i] = a[i] * b[i];
        return true;
    }
    // MixTexture::Evaluate = (1 - amt) * t1 + amt * t2, textures/mix.h:57-61 (0, 1, 0.5)
    if (!tex_value(ps, "amount", true, kHalf, amt)) return false;
    for (int i = 0; i < 3; ++i) t->v[i] = (1 - amt[0]) * a[i] + amt[0] * b[i];
    return true;
}

bool Loader::checkerboard_texture(const std::string &name, const ParamSet &ps, ConstTexture *t) {  // checkerboard.cpp:42-152
    const int dim = ps.one_int("dimension", 2);
    if (dim != 2 && dim != 3) return fail("Texture \"" + name + "\": " + std::to_string(dim) + " dimensional checkerboard texture not supported");
    iile_texture pt = blank_texture(dim == 2 ? IILE_TEX_CHECKER2D : IILE_TEX_CHECKER3D);
    if (!tex_input(name, ps, "tex1", t->is_float, kOne, &pt.child[0], pt.cval[0]) ||
        !tex_input(name, ps, "tex2", t->is_float, kZero, &pt.child[1], pt.cval[1]))
        return false;
    if (dim == 2) {
        if (!mapping_2d(name, ps, &pt)) return false;
        const std::string aa = ps.one_string("aamode", "closedform");
        if (aa == "none")
            pt.aamode = IILE_AA_NONE;
        else {
            if (aa != "closedform")
                std::fprintf(stderr, "Warning: Antialiasing mode \"%s\" not understood by Checkerboard2DTexture; using \"closedform\"\n",
                             aa.c_str());
            pt.aamode = IILE_AA_CLOSEDFORM;
        }
    } else if (!affine_3x4(ctm().m, name, pt.xf))  // IdentityMapping3D(tex2world): tex2world is its WorldToTexture
        return false;
    add_procedural(pt, pt.child[0] < 0 && pt.child[1] < 0, t);
    return true;
}

bool Loader::uv_texture(const std::string &name, const ParamSet &ps, ConstTexture *t) {
    if (t->is_float)  // CreateUVFloatTexture returns no texture (uv.cpp:42-45)
        return fail("Texture \"" + name + "\": class \"uv\" has no float version (a spectrum texture only)");
    iile_texture pt = blank_texture(IILE_TEX_UV);  // CreateUVSpectrumTexture, uv.cpp:47-74
    if (!mapping_2d(name, ps, &pt)) return false;
    add_procedural(pt, true, t);
    return true;
}

// CreateBilerp{Float,Spectrum}Texture, bilerp.cpp:42-103: v00 0, v01 1, v10 0, v11 1
bool Loader::bilerp_texture(const std::string &name, const ParamSet &ps, ConstTexture *t) {
    iile_texture pt = blank_texture(IILE_TEX_BILERP);
    if (!mapping_2d(name, ps, &pt)) return false;
    const char *corner[4] = {"v00", "v01", "v10", "v11"};
    for (int k = 0; k < 4; ++k) {
        const float d = (k & 1) ? 1.f : 0.f;
        float *c = pt.bilerp[k];
        c[0] = c[1] = c[2] = d;
        if (t->is_float)
            c[0] = c[1] = c[2] = ps.one_float(corner[k], d);
        else
            ps.rgb(corner[k], c);
    }
    add_procedural(pt, true, t);
    return true;
}

bool Loader::imagemap_texture(const std::string &name, const ParamSet &ps, ConstTexture *t) {  // textures/imagemap.cpp:148-187
    const std::string mapping = ps.one_string("mapping", "uv");
    if (mapping != "uv") return fail("2D texture mapping \"" + mapping + "\" is not supported (uv only)");
    HostTexture ht;
    std::memset(&ht.t, 0, sizeof(ht.t));
    ht.t.su = ps.one_float("uscale", 1.f);
    ht.t.sv = ps.one_float("vscale", 1.f);
    ht.t.du = ps.one_float("udelta", 0.f);
    ht.t.dv = ps.one_float("vdelta", 0.f);
    ht.t.max_aniso = ps.one_float("maxanisotropy", 8.f);
    ht.t.trilinear = ps.one_bool("trilinear", false) ? 1 : 0;
    const std::string wrap = ps.one_string("wrap", "repeat");
    ht.t.wrap = wrap == "black" ? IILE_WRAP_BLACK : (wrap == "clamp" ? IILE_WRAP_CLAMP : IILE_WRAP_REPEAT);
    const float scale = ps.one_float("scale", 1.f);
    std::string filename = ps.one_string("filename", "");
    if (!filename.empty()) filename = in_search_dir(filename);
    const bool gamma = ps.one_bool("gamma", image_is_8bit(filename));
    std::vector<float> rgb;
    int w = 0, h = 0;
    std::string why;
    if (!read_image(filename, &rgb, &w, &h, &why)) {
        // imagemap.cpp:63-70: Warning + a constant grey 1 x 1 texture
        std::fprintf(stderr, "Warning: %s\nWarning: Creating a constant grey texture to replace \"%s\".\n", why.c_str(),
                     filename.c_str());
        rgb.assign(3, 0.5f);
        w = h = 1;
    }
    if (!build_image_texture(rgb, w, h, scale, gamma, t->is_float, &ht, &why)) return fail("Texture \"" + name + "\": " + why);
    scene_->textures.push_back(std::move(ht));
    t->image = int(scene_->textures.size()) - 1;
    return true;
}

// replaces references to named textures among a material's parameters by their values
// (an image texture stays a reference: `image_of` gets parameter name -> texture index, and the
// parameter a placeholder colour that the material's constant-value checks see as non-black).
// Spectrum images go on Kd, Ks, Kr, Kt and opacity, which every material may be given (one that does not read the parameter
// ignores it), and on the spectrum parameters of `row` that have a slot; `row` is null for a material the loader does not know
bool Loader::resolve_textures(const ParamSet &in, const MaterialRow *row, ParamSet *out, std::map<std::string, int> *image_of) {
    std::string accepted = "Kd, Ks, Kr, Kt, opacity";
    auto common = [](const std::string &n) { return n == "Kd" || n == "Ks" || n == "Kr" || n == "Kt" || n == "opacity"; };
    auto own = [&](const std::string &n) {
        if (row)
            for (const SpectrumParam &sp : row->spectra)
                if (sp.image && n == sp.name) return true;
        return false;
    };
    if (row)
        for (const SpectrumParam &sp : row->spectra)
            if (sp.image && !common(sp.name)) accepted += std::string(", ") + sp.name;
    *out = in;
    for (Param &p : out->params) {
        if (p.type != "texture") continue;
        if (p.strs.size() != 1) return fail("bad texture reference for \"" + p.name + "\"");
        const ConstTexture *t = named_texture(&p);
        if (!t) return fail("Couldn't find texture named \"" + p.strs[0] + "\" for parameter \"" + p.name + "\"");
        if (t->image >= 0 && t->is_float &&
            (p.name == "bumpmap" || p.name == "roughness" || p.name == "uroughness" || p.name == "vroughness" || p.name == "sigma")) {
            (*image_of)[p.name] = t->image;
            p.strs.clear();
            p.type = p.name == "bumpmap" ? "bumpimage" : (p.name == "sigma" ? "sigmaimage" : "roughimage");  // consumed by make_material; no material reads a parameter of these types
            continue;
        }
        if (t->image >= 0) {
            if (t->is_float || (!common(p.name) && !own(p.name)))
                return fail("image texture \"" + p.strs[0] + "\" on parameter \"" + p.name + "\" is not supported (" + accepted + ")");
            (*image_of)[p.name] = t->image;
            p.strs.clear();
            p.type = "color";  // the constant the image's value is multiplied with at the hit (1 unless "scale"d)
            if (t->scaled)
                p.nums = {double(t->v[0]), double(t->v[1]), double(t->v[2])};
            else
                p.nums = {1.0, 1.0, 1.0};
            continue;
        }
        p.strs.clear();
        if (t->is_float) {
            p.type = "float";
            p.nums = {double(t->v[0])};
        } else {
            p.type = "color";
            p.nums = {double(t->v[0]), double(t->v[1]), double(t->v[2])};
        }
    }
    return true;
}

}  // namespace iile
