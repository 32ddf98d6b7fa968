// pbrt_loader.cpp — minimal .pbrt scene-description front end: the token loop, transforms, the attribute stack and the
// options block. Textures, materials, lights and shapes are in loader_*.cpp (pbrt_loader.h).
//
// The reference's parser/API layer (src/core/parser.cpp, api.cpp, paramset.cpp)
// is OUT OF SCOPE as a re-implementation; the GPU box
// only receives this repository, so the path needs its own loader for the
// directives killeroo-class scenes use. What IS in scope is bit-equal scene
// preparation: number parsing through strtol/strtof
// (parser.cpp:258-300), CTM post-multiplication (api.cpp:934-995),
// `Camera` storing Inverse(CTM) (api.cpp:1118-1123), one primitive per
// triangle with the area light attached per shape (api.cpp:1371-1430).
#include <cstdio>

#include "pbrt_loader.h"

namespace iile {

Token TokenStream::next() {
    if (have_pending_) {
        have_pending_ = false;
        return pending_;
    }
    Token t = lex_.next();
    if (t.kind == Token::Error) {
        if (lex_error_->empty()) *lex_error_ = t.text;
        t.kind = Token::End;
    }
    return t;
}

bool TokenStream::numbers(int n, float *out) {
    for (int i = 0; i < n; ++i) {
        Token t = next();
        double v;
        if (t.kind != Token::Word || !parse_number(t.text, &v)) return false;
        out[i] = float(v);
    }
    return true;
}

bool Loader::run(const std::string &path) {
    size_t slash = path.find_last_of('/');
    search_dir_ = (slash == std::string::npos) ? "." : path.substr(0, slash);
    return parse_file(path);
}

bool Loader::parse_file(const std::string &path) {
    TokenStream ts(&lex_error_);
    if (!ts.open(path)) return fail("cannot open scene file " + path);
    while (true) {
        Token t = ts.next();
        if (t.kind == Token::End) {
            if (!lex_error_.empty()) return fail(lex_error_);
            return true;
        }
        if (t.kind != Token::Word) return fail("unexpected token \"" + t.text + "\"");
        if (!directive(t.text, ts)) return false;
    }
}

// parser.cpp:549-700 (parseParams): `"type name" value | [ values ]`
bool Loader::params(TokenStream &ts, ParamSet *ps) {
    while (true) {
        Token t = ts.next();
        if (t.kind != Token::String) {
            ts.unget(t);
            return true;
        }
        Param p;
        std::istringstream decl(t.text);
        decl >> p.type >> p.name;
        if (p.type.empty() || p.name.empty()) return fail("bad parameter declaration \"" + t.text + "\"");
        auto add_value = [&](const Token &v) -> bool {
            if (v.kind == Token::String) {
                p.strs.push_back(v.text);
                return true;
            }
            if (v.kind != Token::Word) return false;
            if (p.type == "bool") {
                p.strs.push_back(v.text);
                return true;
            }
            double d;
            if (!parse_number(v.text, &d)) return false;
            p.nums.push_back(d);
            return true;
        };
        Token v = ts.next();
        if (v.kind == Token::LBracket) {
            while (true) {
                v = ts.next();
                if (v.kind == Token::RBracket) break;
                if (v.kind == Token::End) return fail("premature EOF in parameter list");
                if (!add_value(v)) return fail("bad value for parameter " + p.name);
            }
        } else if (!add_value(v))
            return fail("bad value for parameter " + p.name);
        if (p.type == "point3") p.type = "point";
        if (p.type == "vector3") p.type = "vector";
        if (p.type == "normal3") p.type = "normal";
        ps->params.push_back(std::move(p));
    }
}

bool Loader::directive(const std::string &d, TokenStream &ts) {
    // `Directive "name" parameters`: the options block, and what makes the world's objects
    static const struct {
        const char *word;
        bool (Loader::*make)(const std::string &name, const ParamSet &ps);
    } named[] = {{"Camera", &Loader::camera},
                 {"Film", &Loader::film},
                 {"Sampler", &Loader::sampler},
                 {"Integrator", &Loader::integrator},
                 {"PixelFilter", &Loader::pixel_filter},
                 {"Accelerator", &Loader::accelerator},
                 {"Material", &Loader::material},
                 {"AreaLightSource", &Loader::area_light_source},
                 {"Shape", &Loader::make_shape},
                 {"LightSource", &Loader::light_source}};
    for (const auto &n : named)
        if (d == n.word) {
            Token name = ts.next();
            if (name.kind != Token::String) return fail(d + ": expected quoted name");
            ParamSet ps;
            return params(ts, &ps) && (this->*n.make)(name.text, ps);
        }
    for (const char *word : {"AttributeBegin", "AttributeEnd", "TransformBegin", "TransformEnd", "ReverseOrientation", "WorldBegin", "WorldEnd"})
        if (d == word) return attribute_directive(d);
    for (const char *word : {"Identity", "Translate", "Scale", "Rotate", "LookAt", "Transform", "ConcatTransform", "CoordinateSystem",
                             "CoordSysTransform"})
        if (d == word) return transform_directive(d, ts);
    if (d == "ActiveTransform" || d == "TransformTimes") return motion_directive(d, ts);
    if (d == "Texture") return texture_directive(ts);
    if (d == "MakeNamedMaterial" || d == "NamedMaterial") return named_material_directive(d, ts);
    if (d == "Include") {
        Token n = ts.next();
        if (n.kind != Token::String) return fail("Include: expected filename");
        return parse_file(in_search_dir(n.text));
    }
    return fail("unsupported directive \"" + d + "\"");
}

bool Loader::attribute_directive(const std::string &d) {
    if (d == "AttributeBegin") {
        gs_stack_.push_back(gs_);
        ctm_stack_.push_back({ctms_, active_bits_});
    } else if (d == "AttributeEnd") {
        if (gs_stack_.empty()) return fail("unmatched AttributeEnd");
        gs_ = gs_stack_.back();
        gs_stack_.pop_back();
        ctms_ = ctm_stack_.back().first;
        active_bits_ = ctm_stack_.back().second;
        ctm_stack_.pop_back();
    } else if (d == "TransformBegin") {
        ctm_stack_.push_back({ctms_, active_bits_});
    } else if (d == "TransformEnd") {
        if (ctm_stack_.empty()) return fail("unmatched TransformEnd");
        ctms_ = ctm_stack_.back().first;
        active_bits_ = ctm_stack_.back().second;
        ctm_stack_.pop_back();
    } else if (d == "ReverseOrientation") {
        gs_.reverse_orientation = !gs_.reverse_orientation;
    } else if (d == "WorldBegin") {  // api.cpp:1160-1168
        in_world_ = true;
        ctms_ = XformPair();
        active_bits_ = 3;
        named_cs_["world"] = ctms_;
    } else  // WorldEnd
        in_world_ = false;
    return true;
}

bool Loader::transform_directive(const std::string &d, TokenStream &ts) {
    float f[16];
    if (d == "Identity") {
        for_active_transforms([](Xform &c) { c = Xform(); });
    } else if (d == "Translate") {  // api.cpp:934-942
        if (!ts.numbers(3, f)) return fail("Translate: expected 3 numbers");
        for_active_transforms([&](Xform &c) { c = c * xf_translate(V3(f[0], f[1], f[2])); });
    } else if (d == "Scale") {  // api.cpp:984-991
        if (!ts.numbers(3, f)) return fail("Scale: expected 3 numbers");
        for_active_transforms([&](Xform &c) { c = c * xf_scale(f[0], f[1], f[2]); });
    } else if (d == "Rotate") {  // api.cpp:973-982
        if (!ts.numbers(4, f)) return fail("Rotate: expected 4 numbers");
        for_active_transforms([&](Xform &c) { c = c * xf_rotate(f[0], V3(f[1], f[2], f[3])); });
    } else if (d == "LookAt") {  // api.cpp:993-1007
        if (!ts.numbers(9, f)) return fail("LookAt: expected 9 numbers");
        Xform la;
        xf_lookat(V3(f[0], f[1], f[2]), V3(f[3], f[4], f[5]), V3(f[6], f[7], f[8]), &la);
        for_active_transforms([&](Xform &c) { c = c * la; });
    } else if (d == "Transform" || d == "ConcatTransform") {  // api.cpp:944-971
        Token b = ts.next();
        if (b.kind != Token::LBracket) return fail(d + ": expected [");
        if (!ts.numbers(16, f)) return fail(d + ": expected 16 numbers");
        b = ts.next();
        if (b.kind != Token::RBracket) return fail(d + ": expected ]");
        Xform x(Mat4(f[0], f[4], f[8], f[12], f[1], f[5], f[9], f[13], f[2], f[6], f[10], f[14],
                     f[3], f[7], f[11], f[15]));
        for_active_transforms([&](Xform &c) { c = (d == "Transform") ? x : c * x; });
    } else {  // CoordinateSystem, CoordSysTransform
        Token n = ts.next();
        if (n.kind != Token::String) return fail(d + ": expected name");
        if (d == "CoordinateSystem")
            named_cs_[n.text] = ctms_;  // the whole set, whatever is active (api.cpp:1009-1013)
        else if (named_cs_.count(n.text))
            ctms_ = named_cs_[n.text];
    }
    return true;
}

// `ActiveTransform StartTime | EndTime | All` (api.cpp:1022-1038) and the option `TransformTimes start end` (api.cpp:1040-1047)
bool Loader::motion_directive(const std::string &d, TokenStream &ts) {
    if (d == "ActiveTransform") {
        Token a = ts.next();
        if (a.kind != Token::Word || (a.text != "StartTime" && a.text != "EndTime" && a.text != "All"))
            return fail("ActiveTransform: expected StartTime, EndTime or All, got \"" + a.text + "\"");
        active_bits_ = a.text == "StartTime" ? 1u : (a.text == "EndTime" ? 2u : 3u);
        return true;
    }
    float f[2];
    if (!ts.numbers(2, f)) return fail("TransformTimes: expected 2 numbers");
    if (in_world_) {  // VERIFY_OPTIONS, api.cpp:397-406
        std::fprintf(stderr, "Error: Options cannot be set inside world block; \"TransformTimes\" not allowed.  Ignoring.\n");
        return true;
    }
    scene_->transform_start_time = f[0];
    scene_->transform_end_time = f[1];
    return true;
}

// pbrtTexture, api.cpp:1190-1260: "name" "float|spectrum|color" "class" params
bool Loader::texture_directive(TokenStream &ts) {
    Token n1 = ts.next(), n2 = ts.next(), n3 = ts.next();
    if (n1.kind != Token::String || n2.kind != Token::String || n3.kind != Token::String)
        return fail("Texture: expected \"name\" \"type\" \"class\"");
    ParamSet ps;
    return params(ts, &ps) && make_texture(n1.text, n2.text, n3.text, ps);
}

bool Loader::named_material_directive(const std::string &d, TokenStream &ts) {
    Token n = ts.next();
    if (n.kind != Token::String) return fail(d + ": expected quoted name");
    if (d == "MakeNamedMaterial") {  // api.cpp:1286-1316
        ParamSet ps;
        if (!params(ts, &ps)) return false;
        const std::string type = ps.one_string("type", "");
        if (type.empty()) return fail("MakeNamedMaterial: the \"string type\" parameter is required");
        int idx;
        if (!make_material(type, ps, &idx)) return false;
        named_materials_[n.text] = idx;
    } else {  // NamedMaterial, api.cpp:1318-1336
        auto it = named_materials_.find(n.text);
        if (it == named_materials_.end()) return fail("NamedMaterial \"" + n.text + "\" unknown.");
        gs_.material = it->second;
    }
    return true;
}

// api.cpp:1118-1123, cameras/perspective.cpp:283-330, cameras/environment.cpp:58-101
// (the environment camera reads the common parameters below and drops all but the shutter: finalize.cpp)
bool Loader::camera(const std::string &name, const ParamSet &ps) {
    HostScene &s = *scene_;
    if (name != "perspective" && name != "environment")
        return fail("only the perspective and environment cameras are supported, got " + name);
    s.camera_name = name;
    // CameraToWorld = Inverse(curTransform), both members; the camera is an AnimatedTransform of the two, which moves where they
    // differ (api.cpp:1118-1123, AnimatedTransform::actuallyAnimated, transform.cpp:404)
    XformPair c2w;
    for (int i = 0; i < 2; ++i) c2w.t[i] = inverse(ctms_.t[i]);
    s.camera_to_world = c2w.t[0];
    s.camera_to_world_end = c2w.t[1];
    s.camera_moves = c2w.animated();
    named_cs_["camera"] = c2w;
    s.shutter_open = ps.one_float("shutteropen", 0.f);
    s.shutter_close = ps.one_float("shutterclose", 1.f);
    if (s.shutter_close < s.shutter_open) std::swap(s.shutter_close, s.shutter_open);
    s.lens_radius = ps.one_float("lensradius", 0.f);
    s.focal_distance = ps.one_float("focaldistance", 1e6);
    s.frame_aspect = ps.one_float("frameaspectratio", -1.f);
    const Param *sw = ps.find("screenwindow");
    if (sw && sw->nums.size() == 4) {
        s.has_screen_window = true;
        for (int i = 0; i < 4; ++i) s.screen_window[i] = float(sw->nums[i]);
    }
    s.fov = ps.one_float("fov", 90.);
    float half = ps.one_float("halffov", -1.f);
    if (half > 0.f) s.fov = 2.f * half;
    return true;
}

bool Loader::film(const std::string &name, const ParamSet &ps) {  // film.cpp:259-304
    HostScene &s = *scene_;
    if (name != "image") return fail("only Film \"image\" is supported");
    s.xres = ps.one_int("xresolution", 1280);
    s.yres = ps.one_int("yresolution", 720);
    s.film_filename = ps.one_string("filename", "pbrt.exr");
    const Param *cw = ps.find("cropwindow");
    if (cw && cw->nums.size() == 4) {
        float c[4];
        for (int i = 0; i < 4; ++i) c[i] = float(cw->nums[i]);
        s.crop[0] = clampT(std::min(c[0], c[1]), 0.f, 1.f);
        s.crop[1] = clampT(std::max(c[0], c[1]), 0.f, 1.f);
        s.crop[2] = clampT(std::min(c[2], c[3]), 0.f, 1.f);
        s.crop[3] = clampT(std::max(c[2], c[3]), 0.f, 1.f);
    }
    s.film_scale = ps.one_float("scale", 1.);
    s.film_diagonal = ps.one_float("diagonal", 35.);
    s.max_sample_luminance = ps.one_float("maxsampleluminance", std::numeric_limits<float>::infinity());
    return true;
}

bool Loader::sampler(const std::string &name, const ParamSet &ps) {  // samplers/halton.cpp:129-135, samplers/sobol.cpp:65-71
    HostScene &s = *scene_;
    if (name != "halton" && name != "sobol") return fail("only Sampler \"halton\" and \"sobol\" are supported, got " + name);
    s.sampler_name = name;
    s.spp = ps.one_int("pixelsamples", 16);
    s.sample_at_pixel_center = name == "halton" && ps.one_bool("samplepixelcenter", false);
    return true;
}

// MakeFilter, api.cpp:855-874; Create*Filter in src/filters/*.cpp: "xwidth" / "ywidth" with the class's default, and its own one or
// two parameters (HostScene::filter_p0, filter_p1)
bool Loader::pixel_filter(const std::string &name, const ParamSet &ps) {
    static const struct {
        const char *name;
        float width;
        const char *p0;
        float def0;
        const char *p1;
        float def1;
    } filters[] = {{"box", 0.5f, nullptr, 0.f, nullptr, 0.f},
                   {"gaussian", 2.f, "alpha", 2.f, nullptr, 0.f},
                   {"mitchell", 2.f, "B", 1.f / 3.f, "C", 1.f / 3.f},
                   {"sinc", 4.f, "tau", 3.f, nullptr, 0.f},
                   {"triangle", 2.f, nullptr, 0.f, nullptr, 0.f}};
    HostScene &s = *scene_;
    s.filter_name = name;
    for (const auto &f : filters)
        if (name == f.name) {
            s.filter_rx = ps.one_float("xwidth", f.width);
            s.filter_ry = ps.one_float("ywidth", f.width);
            if (f.p0) s.filter_p0 = ps.one_float(f.p0, f.def0);
            if (f.p1) s.filter_p1 = ps.one_float(f.p1, f.def1);
            return true;
        }
    return fail("Filter \"" + name + "\" unknown.");
}

// integrators/path.cpp:214-231
// "iispt" (CreateIISPTIntegrator, src/integrators/iispt.cpp:790-820) reads the same parameters; which of the two renders
// the frame is the host's choice (iile_host_scene_info::integrator)
// "ambientocclusion" (CreateAOIntegrator, src/integrators/ao.cpp:105-126) reads "pixelbounds" as the path integrator does,
// "cossample" and "nsamples"; RoundCount is the identity for both samplers here (sampler.h:72), so nsamples stands as given
bool Loader::integrator(const std::string &name, const ParamSet &ps) {
    HostScene &s = *scene_;
    if (name != "path" && name != "iispt" && name != "ambientocclusion")
        return fail("only Integrator \"path\" and \"iispt\" and \"ambientocclusion\" are supported, got " + name);
    s.integrator_iispt = name == "iispt";
    s.integrator_ao = name == "ambientocclusion";
    if (s.integrator_ao) {
        s.ao_cossample = ps.one_bool("cossample", true);
        s.ao_nsamples = ps.one_int("nsamples", 64);
        if (s.ao_nsamples < 1) return fail("Integrator \"ambientocclusion\": \"nsamples\" must be at least 1, got " + std::to_string(s.ao_nsamples));
    }
    s.max_depth = ps.one_int("maxdepth", 5);
    s.rr_threshold = ps.one_float("rrthreshold", 1.);
    s.light_strategy = ps.one_string("lightsamplestrategy", "spatial");
    if (s.light_strategy != "spatial" && s.light_strategy != "uniform" && s.light_strategy != "power") {
        // CreateLightSampleDistribution, lightdistrib.cpp:58-63
        std::fprintf(stderr, "Error: Light sample distribution type \"%s\" unknown. Using \"spatial\".\n", s.light_strategy.c_str());
        s.light_strategy = "spatial";
    }
    if (const Param *pb = ps.find("pixelbounds")) {  // path.cpp:216-229
        // (CreateIISPTIntegrator reads it too, iispt.cpp:797-811, but nothing of IISPTIntegrator::Render looks at the member: the
        //  runners get film->GetSampleBounds(), iispt.cpp:395-409 — finalize leaves the sample bounds in place for "iispt")
        if (pb->type != "integer" || pb->nums.size() != 4)
            std::fprintf(stderr, "Error: Expected four values for \"pixelbounds\" parameter. Got %d.\n", int(pb->nums.size()));
        else {
            s.has_pixel_bounds = true;
            for (int i = 0; i < 4; ++i) s.pixel_bounds_given[i] = int(pb->nums[size_t(i)]);
        }
    }
    return true;
}

bool Loader::accelerator(const std::string &name, const ParamSet &ps) {  // accelerators/bvh.cpp:740-760
    HostScene &s = *scene_;
    if (name != "bvh") return fail("only Accelerator \"bvh\" is supported");
    s.accel_split = ps.one_string("splitmethod", "sah");
    if (s.accel_split != "sah" && s.accel_split != "hlbvh" && s.accel_split != "middle" && s.accel_split != "equal") {
        std::fprintf(stderr, "Warning: BVH split method \"%s\" unknown.  Using \"sah\".\n", s.accel_split.c_str());  // bvh.cpp:753-756
        s.accel_split = "sah";
    }
    s.max_node_prims = ps.one_int("maxnodeprims", 4);
    return true;
}

bool Loader::area_light_source(const std::string &name, const ParamSet &ps) {  // api.cpp:1360-1369
    if (name != "area" && name != "diffuse") return fail("unknown area light " + name);
    gs_.has_area_light = true;
    gs_.area_light_params = ps;
    return true;
}

bool load_pbrt_file(const std::string &path, HostScene *scene, std::string *err) {
    Loader l(scene, err);
    return l.run(path);
}

}  // namespace iile
