// pbrt_loader.h — the .pbrt loader's one class, internal to the host library. Its methods are defined by directive:
// pbrt_loader.cpp (the token loop, transforms, attribute stack, options block), loader_textures.cpp, loader_materials.cpp,
// loader_lights.cpp, loader_shapes.cpp. The way in is load_pbrt_file (host_scene.h).
#pragma once
#include <cstdio>
#include <map>

#include "host_scene.h"
#include "pbrt_params.h"

namespace iile {

// A named texture, folded to its value: only textures that are constant over the surface are
// supported ("constant", and "scale" / "mix" of such), so evaluating one at a hit is the same as
// evaluating it once here (textures/constant.h, scale.h, mix.h).
struct ConstTexture {
    bool is_float = true;
    float v[3] = {0, 0, 0};
    int image = -1;  // an "imagemap" spectrum texture: index into HostScene::textures (not constant: kept by reference)
    bool scaled = false;  // a "scale" of that image with a constant: v is the constant factor
    // `image` is a texture of any kind (iile_texture::kind). leaf: an image, uv, bilerp or checkerboard of constants, which a
    // combiner may take as an input; a combiner (and an (image, factor) pair) is not one
    bool leaf = true;
};
struct GraphicsState {
    int material = -1;  // index into scene->materials, -1 = default matte
    bool has_area_light = false;
    ParamSet area_light_params;
    bool reverse_orientation = false;
    std::map<std::string, ConstTexture> textures;  // graphicsState.floatTextures / spectrumTextures, api.cpp:1190-1260
};

// The tokens of one file with one token of look-behind. A tokenizer error ends the stream and is kept in *lex_error (the first
// one of the whole load, Include'd files too).
class TokenStream {
  public:
    explicit TokenStream(std::string *lex_error) : lex_error_(lex_error) {}
    bool open(const std::string &path) { return lex_.open(path); }
    Token next();
    void unget(const Token &t) {
        pending_ = t;
        have_pending_ = true;
    }
    bool numbers(int n, float *out);

  private:
    Lexer lex_;
    Token pending_;
    bool have_pending_ = false;
    std::string *lex_error_;
};

// TransformSet (api.cpp:128-157): the current transform at `TransformTimes`' start and at its end
struct XformPair {
    Xform t[2];
    bool animated() const { return differs(t[0].m, t[1].m) || differs(t[0].inv, t[1].inv); }
};

class Loader;

// One spectrum parameter of a material: GetSpectrumTexture(name, def) of its Create*Material
struct SpectrumParam {
    const char *name;
    float def[3];
    float (iile_material::*value)[3];  // where the constant goes (1, or a "scale"'s factor, under an image)
    int32_t iile_material::*image;     // where an image texture on it goes, or null: constants only, an image is refused by name
    bool refuse_sampled;               // given as "spectrum" / "blackbody": refused by name (else ignored, as any type that is not read)
};
// Which of "roughness" / "uroughness" / "vroughness" a material takes as float images, and which hides which. The reference
// differs per material: see Loader::roughness_images
enum RoughnessImages { ROUGH_NONE, ROUGH_NUMBERS, ROUGH_ONE, ROUGH_UBER, ROUGH_METAL, ROUGH_SUBSTRATE };
// Everything the loader knows about one material: a row of Loader::material_rows() (loader_materials.cpp)
struct MaterialRow {
    const char *name;
    int type;  // IILE_MAT_*
    std::vector<SpectrumParam> spectra;
    RoughnessImages rough;
    bool bump;   // takes "bumpmap"
    bool sigma;  // takes "sigma" as a float image
    void (*fill)(const ParamSet &ps, iile_material *m, iile_disney *dz);  // the scalar parameters
    bool (Loader::*refuse)(const ParamSet &ps);                           // further parameter forms refused by name, or null
};

class Loader {
  public:
    Loader(HostScene *s, std::string *err) : scene_(s), err_(err) {}
    bool run(const std::string &path);

  private:
    HostScene *scene_;
    std::string *err_;
    std::string search_dir_;
    XformPair ctms_;
    uint32_t active_bits_ = 3;  // activeTransformBits: bit i set = transform directives act on ctms_.t[i] (`ActiveTransform`)
    std::map<std::string, XformPair> named_cs_;
    GraphicsState gs_;
    std::vector<GraphicsState> gs_stack_;
    std::vector<std::pair<XformPair, uint32_t>> ctm_stack_;  // pushedTransforms with pushedActiveTransformBits
    bool in_world_ = false;
    int default_material_ = -1;
    std::string lex_error_;
    std::map<std::string, int> named_materials_;  // MakeNamedMaterial, api.cpp:1286-1316

    bool fail(const std::string &m) {
        // a tokenizer error ends the token stream; whatever the parser then complains about,
        // the tokenizer's message is the cause (parser.cpp:199-212)
        if (err_) *err_ = lex_error_.empty() ? m : lex_error_;
        return false;
    }
    // The start transform: what everything but the camera is made with (WARN_IF_ANIMATED_TRANSFORM, api.cpp:422-429)
    const Xform &ctm() const { return ctms_.t[0]; }
    // every transform directive acts on the active members only (FOR_ACTIVE_TRANSFORMS, api.cpp:417-421)
    template <typename F>
    void for_active_transforms(F f) {
        for (int i = 0; i < 2; ++i)
            if (active_bits_ & (1u << i)) f(ctms_.t[i]);
    }
    void warn_if_animated(const char *what) const {
        if (ctms_.animated())
            std::fprintf(stderr, "Warning: Animated transformations set; ignoring for \"%s\" and using the start transform only\n", what);
    }
    // ParamSet::FindOneFilename / AbsolutePath: a relative name is relative to the scene file's directory
    std::string in_search_dir(const std::string &name) const { return (!name.empty() && name[0] == '/') ? name : search_dir_ + "/" + name; }
    // the named texture a "texture" parameter refers to, or null (no such parameter, another type, no such texture)
    const ConstTexture *named_texture(const Param *p) const {
        if (!p || p->type != "texture" || p->strs.size() != 1) return nullptr;
        auto it = gs_.textures.find(p->strs[0]);
        return it == gs_.textures.end() ? nullptr : &it->second;
    }

    // pbrt_loader.cpp
    bool parse_file(const std::string &path);
    bool params(TokenStream &ts, ParamSet *ps);
    bool directive(const std::string &d, TokenStream &ts);
    bool attribute_directive(const std::string &d);
    bool transform_directive(const std::string &d, TokenStream &ts);
    bool motion_directive(const std::string &d, TokenStream &ts);
    bool texture_directive(TokenStream &ts);
    bool named_material_directive(const std::string &d, TokenStream &ts);
    bool camera(const std::string &name, const ParamSet &ps);
    bool film(const std::string &name, const ParamSet &ps);
    bool sampler(const std::string &name, const ParamSet &ps);
    bool pixel_filter(const std::string &name, const ParamSet &ps);
    bool integrator(const std::string &name, const ParamSet &ps);
    bool accelerator(const std::string &name, const ParamSet &ps);
    bool area_light_source(const std::string &name, const ParamSet &ps);
    bool material(const std::string &name, const ParamSet &ps) { return make_material(name, ps, &gs_.material); }

    // loader_textures.cpp
    bool tex_value(const ParamSet &ps, const std::string &name, bool want_float, const float def[3], float out[3]);
    bool scale_of_image(const ParamSet &ps, ConstTexture *t);
    bool tex_input(const std::string &tex_name, const ParamSet &ps, const std::string &name, bool want_float, const float def[3],
                   int *idx, float val[3]);
    bool has_texture_input(const ParamSet &ps, std::initializer_list<std::pair<const char *, bool>> inputs) const;
    bool affine_3x4(const Mat4 &m, const std::string &tex_name, float out[12]);
    bool mapping_2d(const std::string &tex_name, const ParamSet &ps, iile_texture *t);
    void add_procedural(const iile_texture &pt, bool leaf, ConstTexture *t);
    bool make_texture(const std::string &name, const std::string &type, const std::string &cls, const ParamSet &ps);
    bool scale_or_mix_texture(const std::string &name, bool mix, const ParamSet &ps, ConstTexture *t);
    bool checkerboard_texture(const std::string &name, const ParamSet &ps, ConstTexture *t);
    bool uv_texture(const std::string &name, const ParamSet &ps, ConstTexture *t);
    bool bilerp_texture(const std::string &name, const ParamSet &ps, ConstTexture *t);
    bool imagemap_texture(const std::string &name, const ParamSet &ps, ConstTexture *t);
    bool resolve_textures(const ParamSet &in, const MaterialRow *row, ParamSet *out, std::map<std::string, int> *image_of);

    // loader_materials.cpp
    static const std::vector<MaterialRow> &material_rows();
    bool make_material(const std::string &name, const ParamSet &ps_in, int *index);
    bool refuse_parameter_forms(const MaterialRow &row, const ParamSet &ps);
    bool refuse_disney_forms(const ParamSet &ps);
    bool roughness_images(const MaterialRow &row, const ParamSet &ps, const std::map<std::string, int> &image_of, iile_material *m);
    int current_material();

    // loader_lights.cpp
    bool light_source(const std::string &name, const ParamSet &ps);
    void point_light(const V3 &from, iile_light *lt);
    void spot_light(const ParamSet &ps, const V3 &from, const V3 &to, iile_light *lt);
    bool infinite_light(const ParamSet &ps, iile_light *lt);
    bool image_light(const std::string &name, const ParamSet &ps, iile_light *lt);
    void distant_light(const V3 &from, const V3 &to, iile_light *lt);
    bool read_light_map(const ParamSet &ps, std::vector<float> *rgb, int *w, int *h) const;
    iile_light diffuse_area_light() const;

    // loader_shapes.cpp
    bool make_shape(const std::string &name, const ParamSet &ps);
    void sphere_shape(const ParamSet &ps, HostPrim *pr);
    bool quadric_shape(const std::string &name, const ParamSet &ps, HostPrim *pr);
    bool mesh_shape(const std::string &name, const ParamSet &ps, const HostPrim &proto);
    bool mesh_source(const std::string &name, const ParamSet &ps, std::vector<int> *indices, std::vector<V3> *P, std::vector<V3> *N,
                     std::vector<float> *uv);
    bool alpha_masks(const ParamSet &ps, int alpha_mask[2]);
    void add_primitive(int light_type, HostPrim *pr);
};

}  // namespace iile
