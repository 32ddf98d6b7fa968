// loader_lights.cpp — the `LightSource` directive, one function per light class, and the DiffuseAreaLight that an
// `AreaLightSource` gives the shapes after it (pbrt_loader.h).
#include <cstdio>

#include "pbrt_loader.h"

namespace iile {

namespace {

// the upper 3 x 3 of a matrix, row-major
void copy_3x3(const Mat4 &m, float out[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = m.m[r][c];
}

void set_pos(const V3 &p, iile_light *lt) {
    lt->pos[0] = p.x;
    lt->pos[1] = p.y;
    lt->pos[2] = p.z;
}

}  // namespace

// pbrtLightSource, api.cpp:1344-1358; MakeLight, api.cpp:770-806
bool Loader::light_source(const std::string &name, const ParamSet &ps) {
    const bool infinite = name == "infinite" || name == "exinfinite", image = name == "projection" || name == "goniometric";
    if (name != "point" && name != "spot" && name != "distant" && !infinite && !image)
        return fail("LightSource \"" + name +
                    "\" is not supported (point, spot, distant, infinite, exinfinite, projection, goniometric; area lights)");
    warn_if_animated("LightSource");  // pbrtLightSource, api.cpp:1346: every light below is made with the start transform
    float I[3] = {1, 1, 1}, sc[3] = {1, 1, 1};
    ps.rgb((name == "distant" || infinite) ? "L" : "I", I);
    ps.rgb("scale", sc);
    auto point_param = [&](const char *pname, V3 def, V3 *out) -> bool {
        *out = def;
        if (const Param *pp = ps.find(pname)) {
            if (pp->type != "point" || pp->nums.size() != 3) return false;
            *out = V3(float(pp->nums[0]), float(pp->nums[1]), float(pp->nums[2]));
        }
        return true;
    };
    V3 from, to;
    if (!point_param("from", V3(0, 0, 0), &from) || !point_param("to", V3(0, 0, 1), &to))
        return fail(name + " light: bad \"from\" / \"to\"");
    iile_light lt;
    std::memset(&lt, 0, sizeof(lt));
    for (int i = 0; i < 3; ++i) lt.lemit[i] = I[i] * sc[i];
    lt.sphere = -1;
    if (name == "point")
        point_light(from, &lt);
    else if (name == "spot")
        spot_light(ps, from, to, &lt);
    else if (name == "distant")
        distant_light(from, to, &lt);
    else if (!(infinite ? infinite_light(ps, &lt) : image_light(name, ps, &lt)))
        return false;
    scene_->lights.push_back(lt);
    return true;
}

void Loader::point_light(const V3 &from, iile_light *lt) {  // CreatePointLight, lights/point.cpp:80-88
    const Xform l2w = xf_translate(from) * ctm();
    lt->type = IILE_LIGHT_POINT;
    set_pos(l2w.point(V3(0, 0, 0)), lt);
}

void Loader::spot_light(const ParamSet &ps, const V3 &from, const V3 &to, iile_light *lt) {  // CreateSpotLight, lights/spot.cpp:104-124
    const float coneangle = ps.one_float("coneangle", 30.f), conedelta = ps.one_float("conedeltaangle", 5.f);
    const V3 dir = normalize(to - from);
    V3 du, dv;  // CoordinateSystem, geometry.h:1020-1028
    if (std::abs(dir.x) > std::abs(dir.y))
        du = div(V3(-dir.z, 0, dir.x), std::sqrt(dir.x * dir.x + dir.z * dir.z));
    else
        du = div(V3(0, dir.z, -dir.y), std::sqrt(dir.y * dir.y + dir.z * dir.z));
    dv = cross(dir, du);
    Mat4 m;
    const float rows[4][4] = {{du.x, du.y, du.z, 0}, {dv.x, dv.y, dv.z, 0}, {dir.x, dir.y, dir.z, 0}, {0, 0, 0, 1}};
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) m.m[r][c] = rows[r][c];
    const Xform dir_to_z(m);
    const Xform l2w = ctm() * xf_translate(from) * inverse(dir_to_z);
    lt->type = IILE_LIGHT_SPOT;
    set_pos(l2w.point(V3(0, 0, 0)), lt);
    copy_3x3(l2w.inv, lt->w2l);                          // WorldToLight = Inverse(LightToWorld)
    lt->cos_total_width = std::cos(radians(coneangle));  // SpotLight ctor, spot.cpp:43-51
    lt->cos_falloff_start = std::cos(radians(coneangle - conedelta));
}

void Loader::distant_light(const V3 &from, const V3 &to, iile_light *lt) {  // CreateDistantLight, lights/distant.cpp:94-102; ctor :43-48
    lt->type = IILE_LIGHT_DISTANT;
    set_pos(normalize(ctm().vector(from - to)), lt);
    // world_radius is set once the scene bounds are known (finalize_scene)
}

// the image "mapname" names, as ReadImage returns it; a name that cannot be read is a warning and no image
bool Loader::read_light_map(const ParamSet &ps, std::vector<float> *rgb, int *w, int *h) const {
    const std::string mapname = ps.one_string("mapname", "");
    if (mapname.empty()) return false;
    std::string why;
    if (read_image(in_search_dir(mapname), rgb, w, h, &why)) return true;
    std::fprintf(stderr, "Warning: %s\n", why.c_str());
    return false;
}

bool Loader::infinite_light(const ParamSet &ps, iile_light *lt) {  // CreateInfiniteLight, lights/infinite.cpp:176-186
    lt->type = IILE_LIGHT_INFINITE;
    lt->n_samples = ps.one_int("samples", ps.one_int("nsamples", 1));  // infinite.cpp:181-182
    copy_3x3(ctm().m, lt->l2w);
    copy_3x3(ctm().inv, lt->w2l);
    // InfiniteAreaLight ctor (infinite.cpp:42-84): Lmap = the environment map times L (one texel of L
    // without a map or when it cannot be read), not flipped; then the sampling distribution
    std::vector<float> rgb;
    int w = 0, h = 0;
    if (read_light_map(ps, &rgb, &w, &h))
        for (size_t i = 0; i < rgb.size(); ++i) rgb[i] *= lt->lemit[i % 3];
    else
        rgb.clear();
    if (rgb.empty()) {
        rgb.assign(lt->lemit, lt->lemit + 3);
        w = h = 1;
    }
    HostTexture ht;
    std::string why;
    if (!build_environment_light(rgb, w, h, &ht, &scene_->env_dist, &lt->dist_w, &lt->dist_h, &lt->dist_offset, &why))
        return fail("infinite light: " + why);
    scene_->textures.push_back(std::move(ht));
    lt->env_tex = int(scene_->textures.size()) - 1;
    // world_radius is set once the scene bounds are known (finalize_scene)
    return true;
}

// CreateProjectionLight (lights/projection.cpp:134-143) and its ctor (:45-75); CreateGoniometricLight
// (lights/goniometric.cpp:86-94) and its ctor (goniometric.h:57-68): the CTM is LightToWorld
bool Loader::image_light(const std::string &name, const ParamSet &ps, iile_light *lt) {
    lt->type = name == "projection" ? IILE_LIGHT_PROJECTION : IILE_LIGHT_GONIOMETRIC;
    set_pos(ctm().point(V3(0, 0, 0)), lt);
    copy_3x3(ctm().inv, lt->w2l);  // WorldToLight = Inverse(LightToWorld)
    // the map as ReadImage returns it (not times I, not flipped), under MIPMap<RGBSpectrum>(resolution, texels)'s
    // defaults; a name that cannot be read is the reference's null map (a warning, no failure)
    lt->env_tex = -1;
    int w = 0, h = 0;
    std::vector<float> rgb;
    if (read_light_map(ps, &rgb, &w, &h)) {
        HostTexture ht;
        std::memset(&ht.t, 0, sizeof(ht.t));  // MIPMap defaults: EWA, maxAniso 8, repeat (mipmap.h:66-67)
        ht.t.wrap = IILE_WRAP_REPEAT;
        ht.t.max_aniso = 8.f;
        ht.t.su = ht.t.sv = 1.f;
        std::string why;
        if (!build_mip_pyramid(rgb, w, h, &ht, &why)) return fail(name + " light: " + why);
        scene_->textures.push_back(std::move(ht));
        lt->env_tex = int(scene_->textures.size()) - 1;
    }
    if (name == "projection") {
        const float fov = ps.one_float("fov", 45.f), hither = 1e-3f;
        const float aspect = lt->env_tex >= 0 ? float(w) / float(h) : 1.f;  // projection.cpp:59-65
        const float sb_aspect[4] = {-aspect, -1, aspect, 1}, sb_tall[4] = {-1, -1 / aspect, 1, 1 / aspect};
        float *sb = lt->l2w + IILE_PROJ_BOUNDS;
        for (int i = 0; i < 4; ++i) sb[i] = aspect > 1 ? sb_aspect[i] : sb_tall[i];
        const Xform proj = xf_perspective(fov, hither, 1e30f);  // hither, yon: projection.cpp:66-68
        lt->l2w[IILE_PROJ_M00] = proj.m.m[0][0];  // (the rest of rows 0, 1 and 3 is 0, 0, 1, 0: iile_scene.h)
        lt->l2w[IILE_PROJ_M11] = proj.m.m[1][1];
        lt->l2w[IILE_PROJ_HITHER] = hither;
        lt->l2w[IILE_PROJ_FOV] = fov;
        const float hh = (sb[0] * sb[0] + sb[1] * sb[1] + 1);
        lt->cos_total_width = 1 / hh;  // projection.cpp:70-74
    }
    return true;
}

// The DiffuseAreaLight of the current AreaLightSource (api.cpp:808-826 MakeAreaLight, lights/diffuse.cpp:125-146): Lemit,
// twosided, nSamples; type IILE_LIGHT_DIFFUSE_AREA and no sphere until the caller sets what its shape needs
iile_light Loader::diffuse_area_light() const {
    float L[3] = {1, 1, 1}, sc[3] = {1, 1, 1};
    gs_.area_light_params.rgb("L", L);
    gs_.area_light_params.rgb("scale", sc);
    iile_light lt;
    std::memset(&lt, 0, sizeof(lt));
    for (int i = 0; i < 3; ++i) lt.lemit[i] = L[i] * sc[i];
    lt.two_sided = gs_.area_light_params.one_bool("twosided", false);
    lt.n_samples = gs_.area_light_params.one_int("samples", gs_.area_light_params.one_int("nsamples", 1));
    lt.sphere = -1;
    return lt;
}

}  // namespace iile
