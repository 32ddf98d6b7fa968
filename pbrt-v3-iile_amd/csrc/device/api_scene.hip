// api_scene.hip — the scene half of libiile_gpu.so's C ABI (include/iile_gpu.h): iile_last_error and the error record,
// the device and stream utilities, and iile_scene_create / iile_scene_destroy: one refusal pass, then one builder per table
// of DScene. The render entry points are in api_render.hip and api_iispt.hip, the kernel-level ones in api_probes.hip.
#include <array>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>

#include "api_common.h"

using namespace iile;

namespace {
thread_local std::string g_err;  // what iile_last_error() returns: the last failure of this thread
}  // namespace
namespace iile {
int api_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return api_fail(IILE_ERR_NO_DEVICE,
                        "no HIP device available: libiile_gpu has no CPU fallback (hipGetDeviceCount: " +
                            std::string(e == hipSuccess ? "0 devices" : hipGetErrorString(e)) + ")");
    return IILE_OK;
}
int check_bvh_nodes(const iile_bvh_node *nodes, int n_nodes, int64_t max_prims, const char *prefix, int *n_interior) {
    *n_interior = 0;
    for (int i = 0; i < n_nodes; ++i) {
        const iile_bvh_node &nd = nodes[i];
        if (nd.nprims > 0) {
            if (nd.offset < 0 || nd.offset + int64_t(nd.nprims) > max_prims) return api_fail(IILE_ERR_ARG, std::string(prefix) + "bad leaf range");
            continue;
        }
        if (i + 1 >= n_nodes || nd.offset <= i || nd.offset >= n_nodes) return api_fail(IILE_ERR_ARG, std::string(prefix) + "bad BVH child index");
        ++*n_interior;
    }
    return IILE_OK;
}
}  // namespace iile
namespace {

template <typename T>
int upload(iile_scene *sc, const T *host, size_t n, const T **dev) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIP_TRY(hipMalloc(&p, bytes));
    sc->allocs.push_back(p);
    if (n) HIP_TRY(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    *dev = static_cast<const T *>(p);
    return IILE_OK;
}

// ---- iile_scene_create: one refusal pass, then one builder per table of DScene; first the translations both apply ------
// The device's copy of a material: texture indices -1 without textures, an opacity texture for uber only, and rough_tex_v
// -2 for a material without a "vroughness" of its own.
DMaterial device_material(const iile_material &m, int n_textures) {
    DMaterial r = DMaterial();
    r.type = m.type;
    for (int c = 0; c < 3; ++c) {
        r.kd[c] = m.kd[c];
        r.ks[c] = m.ks[c];
        r.kr[c] = m.kr[c];
        r.kt[c] = m.kt[c];
        r.cond_eta[c] = m.type == IILE_MAT_METAL ? m.cond_eta[c] : 0.f;
        r.cond_k[c] = m.type == IILE_MAT_METAL ? m.cond_k[c] : 0.f;
        r.opacity[c] = m.type == IILE_MAT_UBER ? m.opacity[c] : 1.f;
    }
    r.alpha = m.alpha;
    const bool uv_rough = m.type == IILE_MAT_METAL || m.type == IILE_MAT_SUBSTRATE;  // "uroughness" and "vroughness" of their own
    r.alpha_y = (m.type == IILE_MAT_GLASS || uv_rough) ? m.alpha_v : (m.type == IILE_MAT_UBER && m.rough_tex_v != -2) ? m.alpha_v : m.alpha;
    const bool oren_nayar = m.type == IILE_MAT_MATTE && m.sigma != 0;
    r.on_a = oren_nayar ? m.on_a : 1.f;
    r.on_b = oren_nayar ? m.on_b : 0.f;
    r.eta = m.eta;
    const bool tex = n_textures > 0;
    r.kd_tex = tex ? m.kd_tex : -1, r.ks_tex = tex ? m.ks_tex : -1, r.kr_tex = tex ? m.kr_tex : -1, r.kt_tex = tex ? m.kt_tex : -1;
    r.opacity_tex = (tex && m.type == IILE_MAT_UBER) ? m.opacity_tex : -1;
    r.rough_tex_v = (m.type == IILE_MAT_UBER || uv_rough) ? ((m.rough_tex_v >= 0 && !tex) ? -1 : m.rough_tex_v) : -2;
    r.bump_tex = tex ? m.bump_tex : -1, r.rough_tex = tex ? m.rough_tex : -1, r.sigma_tex = tex ? m.sigma_tex : -1;
    r.remap_roughness = m.remap_roughness;
    return r;
}
std::array<int, 9> material_textures(const DMaterial &m) {
    return {m.kd_tex, m.ks_tex, m.kr_tex, m.kt_tex, m.bump_tex, m.rough_tex, m.sigma_tex, m.opacity_tex, m.rough_tex_v};
}
// input k of a texture as the device reads it: an image has none
int texture_input(const iile_texture &t, int k) { return t.kind == IILE_TEX_IMAGE ? -1 : t.child[k]; }
// an alpha mask of the primitive can reject a hit (bit 12 of its flag word)
bool prim_masked(const iile_scene_desc &d, int i) {
    return (d.prim_flags[i] & IILE_PRIM_HAS_ALPHA) && d.prim_alpha &&
           (d.prim_alpha[2 * i] != IILE_ALPHA_NONE || d.prim_alpha[2 * i + 1] != IILE_ALPHA_NONE);
}
// SpatialLightDistribution's voxel grid over the scene bounds (lightdistrib.cpp:98-111): up to 64 voxels per axis, cubes along the
// longest one. The bounds are the root node's.
void light_grid(const iile_scene_desc &d, int nv[3]) {
    const float *lo = d.nodes[0].bmin, *hi = d.nodes[0].bmax;
    const float diag[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const int me = (diag[0] > diag[1] && diag[0] > diag[2]) ? 0 : (diag[1] > diag[2] ? 1 : 2);  // MaximumExtent
    const float bmax = diag[me];
    for (int i = 0; i < 3; ++i) nv[i] = std::max(1, int(std::round(diag[i] / bmax * 64)));
}
// The dense table of the spatial strategy, one record of 2 n + 2 floats per voxel, may take this much device memory: 511 lights on
// a full 64^3 grid. A design decision, not a measurement; the reference fills its voxels lazily and has no such limit.
constexpr uint64_t kMaxLightTableBytes = uint64_t(1) << 30;
bool spatial_table(const iile_scene_desc &d) { return d.n_lights > 1 && d.integrator.light_strategy == IILE_LIGHTS_SPATIAL && d.n_nodes > 0; }

int interior_nodes(const iile_scene_desc &d) {
    return int(std::count_if(d.nodes, d.nodes + std::max(d.n_nodes, 0), [](const iile_bvh_node &nd) { return nd.nprims == 0; }));
}

// Interior nodes on the longest path from the root to a leaf of a flattened tree that passed check_bvh_nodes (a parent lies
// before its children: one pass)
int bvh_depth(const iile_bvh_node *nodes, int n_nodes) {
    std::vector<int> level(size_t(std::max(n_nodes, 0)), 0);
    int deepest = 0;
    for (int i = 0; i < n_nodes; ++i) {
        if (nodes[i].nprims > 0)
            deepest = std::max(deepest, level[i]);
        else
            level[i + 1] = level[nodes[i].offset] = level[i] + 1;
    }
    return deepest;
}

// Every refusal of iile_scene_create, in the order it has always made them, before any device call: a malformed
// descriptor is refused on a machine without a GPU too. The builders below assume a descriptor that passed.
int check_scene_desc(const iile_scene_desc &d) {
    // what the device path supports
    if (d.n_prims >= (1 << 24)) return api_fail(IILE_ERR_UNSUPPORTED, "more than 2^24 primitives");
    if (d.n_lights < 0 || (d.n_lights > 0 && !d.lights)) return api_fail(IILE_ERR_ARG, "n_lights without lights");
    // (light_power_all lies behind the members an older caller's descriptor has: not touched unless the lights need it)
    if (d.n_lights > IILE_MAX_LIGHTS && d.integrator.light_strategy == IILE_LIGHTS_POWER && !d.light_power_all)
        return api_fail(IILE_ERR_ARG, "light_power_all is null: the power strategy over more than " + std::to_string(IILE_MAX_LIGHTS) +
                                          " lights reads every light's power there");
    if (d.n_quadrics < 0 || (d.n_quadrics > 0 && !d.quadrics))
        return api_fail(IILE_ERR_UNSUPPORTED, "too many disks and cylinders");
    for (int i = 0; i < d.n_quadrics; ++i)
        if (d.quadrics[i].kind != IILE_QUADRIC_DISK && d.quadrics[i].kind != IILE_QUADRIC_CYLINDER)
            return api_fail(IILE_ERR_UNSUPPORTED, "unsupported quadric kind");
    for (int i = 0; i < d.n_prims; ++i) {  // every primitive names a shape that exists
        const uint32_t f = d.prim_flags[i];
        if ((f & IILE_PRIM_SPHERE) && (f & IILE_PRIM_QUADRIC)) return api_fail(IILE_ERR_ARG, "primitive is both a sphere and a quadric");
        if ((f & IILE_PRIM_SPHERE) && (d.prim_shape[i] < 0 || d.prim_shape[i] >= d.n_spheres))
            return api_fail(IILE_ERR_ARG, "sphere primitive without its sphere");
        if ((f & IILE_PRIM_QUADRIC) && (d.prim_shape[i] < 0 || d.prim_shape[i] >= d.n_quadrics))
            return api_fail(IILE_ERR_ARG, "quadric primitive without its quadric");
    }
    for (int i = 0; i < d.n_lights; ++i) {
        const iile_light &l = d.lights[i];
        if (l.type == IILE_LIGHT_DIFFUSE_AREA) {
            if (l.sphere < 0 || l.sphere >= d.n_spheres) return api_fail(IILE_ERR_ARG, "area light without a sphere");
        } else if (l.type == IILE_LIGHT_AREA_TRIANGLE) {
            if (l.prim < 0 || l.prim >= d.n_prims || (d.prim_flags[l.prim] & (IILE_PRIM_SPHERE | IILE_PRIM_QUADRIC)) || d.prim_light[l.prim] != i)
                return api_fail(IILE_ERR_ARG, "triangle area light without its triangle");
        } else if (l.type == IILE_LIGHT_AREA_QUADRIC) {
            if (l.prim < 0 || l.prim >= d.n_prims || !(d.prim_flags[l.prim] & IILE_PRIM_QUADRIC) || d.prim_light[l.prim] != i)
                return api_fail(IILE_ERR_ARG, "quadric area light without its quadric");
        } else if (!iile_light_is_delta(l.type) && l.type != IILE_LIGHT_INFINITE) {
            return api_fail(IILE_ERR_UNSUPPORTED, "unsupported light type");
        }
    }
    for (int i = 0; i < d.n_materials; ++i)
        if ((d.materials[i].type < IILE_MAT_MATTE || d.materials[i].type > IILE_MAT_SUBSTRATE) && d.materials[i].type != IILE_MAT_TRANSLUCENT &&
            d.materials[i].type != IILE_MAT_DISNEY)
            return api_fail(IILE_ERR_UNSUPPORTED, "unsupported material type");   // (7 and 9 among them)
    // (disney lies behind the members an older caller's descriptor has: not touched unless a material is Disney's)
    for (int i = 0; i < d.n_materials; ++i)
        if (d.materials[i].type == IILE_MAT_DISNEY && !d.disney)
            return api_fail(IILE_ERR_ARG, "disney is null: a Disney material reads its scalar parameters there");
    if (d.halton.n_dims > kMaxHaltonDims) return api_fail(IILE_ERR_UNSUPPORTED, "too many Halton dimensions");
    const int need_dims = 5 + 8 * d.integrator.max_depth + 1;
    if (d.halton.n_dims < need_dims) return api_fail(IILE_ERR_ARG, "Halton table covers too few dimensions for maxdepth");
    if (d.integrator.max_depth > 14) return api_fail(IILE_ERR_UNSUPPORTED, "maxdepth > 14");
    if ((double(d.halton.spp) + 1) * double(d.halton.sample_stride) >= 4294967296.0)
        return api_fail(IILE_ERR_UNSUPPORTED, "Halton index exceeds 32 bits (pixelsamples too large)");
    if (!(d.film.filter_rx > 0) || !(d.film.filter_ry > 0) || d.film.filter_rx > 16 || d.film.filter_ry > 16)
        return api_fail(IILE_ERR_UNSUPPORTED, "pixel filter radius must lie in (0, 16]");
    if (!d.film_filter_wide && (d.film.filter_rx != 0.5f || d.film.filter_ry != 0.5f))
        return api_fail(IILE_ERR_ARG, "film_filter_wide must be set for any filter but the box of radius 0.5");
    // the references between the tables
    int n_interior = 0;
    if (const int rc = check_bvh_nodes(d.nodes, d.n_nodes, d.n_prims, "", &n_interior)) return rc;
    if (spatial_table(d)) {
        int nv[3];
        light_grid(d, nv);
        const uint64_t bytes = uint64_t(nv[0]) * uint64_t(nv[1]) * uint64_t(nv[2]) * (2 * uint64_t(d.n_lights) + 2) * sizeof(float);
        if (bytes > kMaxLightTableBytes)
            return api_fail(IILE_ERR_UNSUPPORTED,
                            std::to_string(d.n_lights) + " lights: the spatial light distribution's table over " + std::to_string(nv[0]) + " x " +
                                std::to_string(nv[1]) + " x " + std::to_string(nv[2]) + " voxels would take " + std::to_string(bytes >> 20) +
                                " MiB (at most " + std::to_string(kMaxLightTableBytes >> 20) +
                                "); \"lightsamplestrategy\" \"power\" or \"uniform\" renders the scene");
    }
    // a lane's traversal stack holds a tree of traversal_limits().max_bvh_depth levels (dtrav.h: kMaxBvhDepth); a deeper one could
    // write past the lane's HBM column into its neighbours'
    const int depth = bvh_depth(d.nodes, d.n_nodes), max_depth = traversal_limits().max_bvh_depth;
    if (depth > max_depth)
        return api_fail(IILE_ERR_UNSUPPORTED, "BVH depth " + std::to_string(depth) + " exceeds the traversal stack's limit of " +
                                                  std::to_string(max_depth) + " levels");
    for (int i = 0; i < d.n_prims; ++i)
        if ((d.prim_flags[i] & IILE_PRIM_SPHERE) && d.prim_light[i] >= 0 && d.lights[d.prim_light[i]].sphere != d.prim_shape[i])
            return api_fail(IILE_ERR_ARG, "light / sphere cross reference is inconsistent");
    bool masked = false;
    for (int i = 0; i < d.n_prims && !masked; ++i) masked = prim_masked(d, i);
    for (int i = 0; masked && i < d.n_prims; ++i)
        for (int m : {d.prim_alpha[2 * i], d.prim_alpha[2 * i + 1]})
            if (m >= d.n_textures || m < IILE_ALPHA_ZERO) return api_fail(IILE_ERR_ARG, "alpha mask refers to a texture that does not exist");
            else if (m >= 0 && d.textures[m].kind != IILE_TEX_IMAGE)  // (the traversal kernels look up images only)
                return api_fail(IILE_ERR_ARG, "alpha mask refers to a procedural texture");
    for (int i = 0; i < d.n_materials; ++i)
        for (int t : material_textures(device_material(d.materials[i], d.n_textures)))
            if (t >= d.n_textures) return api_fail(IILE_ERR_ARG, "material refers to a texture that does not exist");
    for (int i = 0; i < d.n_textures; ++i) {
        const iile_texture &t = d.textures[i];
        if (t.kind < IILE_TEX_IMAGE || t.kind > IILE_TEX_BILERP) return api_fail(IILE_ERR_ARG, "texture of an unknown kind");
        if ((t.kind == IILE_TEX_IMAGE && (t.n_levels < 1 || t.n_levels > kMaxTexLevels)) || (t.kind != IILE_TEX_IMAGE && t.n_levels != 0))
            return api_fail(IILE_ERR_ARG, "texture with a bad level count");
        // a combiner's input is a leaf (an image, uv, bilerp, or a checkerboard of constants): the device evaluates two levels
        // and does not recurse
        for (int k = 0; k < 3; ++k) {
            const int c = texture_input(t, k);
            if (c < -1 || c >= d.n_textures) return api_fail(IILE_ERR_ARG, "texture input out of range");
            if (c < 0) continue;
            const iile_texture &ct = d.textures[c];
            const bool leaf = ct.kind == IILE_TEX_IMAGE || ct.kind == IILE_TEX_UV || ct.kind == IILE_TEX_BILERP ||
                              ((ct.kind == IILE_TEX_CHECKER2D || ct.kind == IILE_TEX_CHECKER3D) && ct.child[0] < 0 && ct.child[1] < 0);
            if (!leaf) return api_fail(IILE_ERR_ARG, "texture input that is not a leaf (textures nest two levels deep at most)");
        }
        for (int l = 0; l < t.n_levels; ++l)
            if (t.level_offset[l] < 0 || t.level_offset[l] + int64_t(t.level_w[l]) * t.level_h[l] > d.n_texels)
                return api_fail(IILE_ERR_ARG, "texture level outside the texel array");
    }
    for (int i = 0; i < d.n_lights; ++i) {
        const iile_light &il = d.lights[i];
        if (il.type == IILE_LIGHT_INFINITE &&
            (il.env_tex < 0 || il.env_tex >= d.n_textures || d.textures[il.env_tex].kind != IILE_TEX_IMAGE || il.dist_w < 1 || il.dist_h < 1 ||
             il.dist_offset < 0 || il.dist_offset + int64_t(2 * il.dist_w + 2) * il.dist_h + 2 * il.dist_h + 2 > d.n_env_dist))
            return api_fail(IILE_ERR_ARG, "infinite light: bad environment map / distribution reference");
        // (the lookups of delta_light_li and of the light probe rely on this)
        if ((il.type == IILE_LIGHT_PROJECTION || il.type == IILE_LIGHT_GONIOMETRIC) && il.env_tex != -1 &&
            (il.env_tex < 0 || il.env_tex >= d.n_textures || d.textures[il.env_tex].kind != IILE_TEX_IMAGE))
            return api_fail(IILE_ERR_ARG, "projection / goniometric light: its map is not an image texture of the scene");
    }
    const iile_sobol &sb = d.sobol;
    if (sb.enabled && (sb.n_dims < need_dims || sb.n_dims > 256 || !sb.matrices32 || sb.log2_resolution < 1 || sb.log2_resolution > 16 ||
                       sb.resolution != (1 << sb.log2_resolution) || (uint64_t(sb.spp) << (2 * sb.log2_resolution)) > (uint64_t(1) << 32)))
        return api_fail(IILE_ERR_ARG, "iile_sobol: bad dimension count / resolution, or sample indices beyond 32 bits");
    if (sb.enabled && (sb.resolution < d.film.samp_x1 - d.film.samp_x0 || sb.resolution < d.film.samp_y1 - d.film.samp_y0))
        return api_fail(IILE_ERR_ARG, "iile_sobol: resolution smaller than the sample bounds");
    // an all-zero raster_to_camera stands for the environment camera (iile_camera, iile_scene.h) only together with the rest of
    // its encoding: a zeroed struct, or a perspective camera that lost its matrix, is neither camera
    const iile_camera &cam = d.camera;
    if (iile_camera_kind(&cam) == IILE_CAMERA_ENVIRONMENT) {
        const float dphi = cam.dx_camera[IILE_ENVCAM_PHI], dtheta = cam.dy_camera[IILE_ENVCAM_THETA];
        // (the steps are a tag the device does not compute with — it follows environment.cpp from the film's resolution — so a
        // producer that rounds them another way is not refused: a few ulps of slack, 1e-6 relative)
        const auto near = [](float v, float want) { return std::isfinite(v) && v > 0 && std::abs(v - want) <= 1e-6f * want; };
        const bool steps = d.film.xres > 0 && d.film.yres > 0 && near(dphi, 2 * kPi / float(d.film.xres)) &&
                           near(dtheta, kPi / float(d.film.yres)) && cam.dx_camera[1] == 0 && cam.dx_camera[2] == 0 &&
                           cam.dy_camera[0] == 0 && cam.dy_camera[2] == 0;
        if (!steps || cam.lens_radius != 0)
            return api_fail(IILE_ERR_ARG, "environment camera: a zero raster_to_camera needs lens_radius 0 and the angle steps 2 pi / xres, pi / yres");
    }
    return IILE_OK;
}

// Bits 5..7 of a primitive's flag word: the material type (3 for a mirror and anything past uber), +4 for a sphere or a
// quadric; 7 becomes 6.
uint32_t shading_class(int material_type, bool shape) {
    const uint32_t cls = uint32_t(material_type < 0 || material_type > 3 ? 3 : material_type) | (shape ? 4u : 0u);
    return cls == 7u ? 6u : cls;
}

// The kernel-selection flags of DScene, which builds of the kernels the scene needs (kernels*.hip launchers), from the
// descriptor alone; boxes_nested is pack_wide_records' to decide (build_bvh).
void set_kernel_flags(const iile_scene_desc &d, DScene &S) {
    for (int i = 0; i < d.n_prims; ++i)
        if (prim_masked(d, i)) S.has_alpha = 1;
    S.rare_prims = (S.has_alpha || d.n_quadrics > 0 || d.n_spheres > kFewSpheres) ? 1 : 0;
    for (int i = 0; i < d.n_materials; ++i) {
        const iile_material &m = d.materials[i];
        if (m.type == IILE_MAT_GLASS) S.has_glass = 1;
        if (m.type == IILE_MAT_UBER) {
            // uber.cpp:53-61, 94-99: a SpecularTransmission lobe exists if 1 - opacity or opacity x Kt is not black (an image for Kt: may be)
            bool trans = (m.kt_tex >= 0 || m.opacity_tex >= 0) && d.n_textures > 0;
            for (int c = 0; c < 3; ++c) {
                const float op = m.opacity[c] > 0.f ? m.opacity[c] : 0.f;
                trans = trans || (-op + 1.f) > 0.f || op * (m.kt[c] > 0.f ? m.kt[c] : 0.f) != 0.f;
            }
            if (trans) S.has_glass = 1, S.has_uber_trans = 1;   // (etaScale is tracked: path.cpp:151-157)
        }
        for (int t : material_textures(device_material(m, d.n_textures)))
            if (t >= 0) S.textured_materials = 1;
        if (m.type != IILE_MAT_MATTE && m.type != IILE_MAT_PLASTIC && m.type != IILE_MAT_METAL && m.type != IILE_MAT_SUBSTRATE &&
            m.type != IILE_MAT_TRANSLUCENT && m.type != IILE_MAT_DISNEY)
            S.has_specular = 1;   // (metal and substrate: one glossy reflection lobe each, metal.cpp:79, substrate.cpp:62; translucent:
                                  //  diffuse and glossy lobes only, translucent.cpp:62-78; Disney: likewise, disney.cpp:505-587)
        if (m.type == IILE_MAT_DISNEY) S.disney_build = 1;
        if ((m.type != IILE_MAT_MATTE && m.type != IILE_MAT_PLASTIC) || (m.type == IILE_MAT_MATTE && m.sigma != 0))
            S.extended_features = 1;
    }
    // the Disney builds for any scene: the identity tests' switch (their other materials must render what the ordinary builds render)
    if (std::getenv("IILE_DISNEY_BUILD")) S.disney_build = 1;
    if (S.disney_build) S.extended_features = 1;
    S.all_lights_infinite = d.n_lights > 0 ? 1 : 0;
    for (int i = 0; i < d.n_lights; ++i)
        if (d.lights[i].type == IILE_LIGHT_INFINITE) S.has_infinite = 1;
        else S.all_lights_infinite = 0;
    // (quadrics: the plain build leaves quadric hits out, shape_hit_interaction<.., QUAD = false>)
    if (d.n_lights > 1 || (d.n_lights == 1 && d.lights[0].type != IILE_LIGHT_DIFFUSE_AREA) || S.has_infinite || d.n_quadrics > 0)
        S.extended_features = 1;
}

// A device allocation of the scene's (iile_scene_destroy frees it).
template <typename T>
int scene_alloc(iile_scene *sc, size_t bytes, T **out, const char *what) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return api_fail(IILE_ERR_HIP, what);
    sc->allocs.push_back(p);
    *out = static_cast<T *>(p);
    return IILE_OK;
}

// The builders: each fills its part of sc->ds (uploading into sc->allocs) from a checked descriptor, in this order.
// BVH: the depth-first LinearBVHNode array (bvh.cpp:640-658) is re-packed on the device (bvh_build.hip,
// pack_wide_records) into the two-wide records {children[0] box, children[1] box, refs, axis} of the instrumented kernels
// and the four-wide records of dtrav.h trav_interior4. A reference is the interior record index, or ~firstPrimitive for a
// leaf child.
int build_bvh(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    const int n = d.n_nodes, n_interior = interior_nodes(d);
    S.n_nodes = n;
    const iile_bvh_node *d_nodes = nullptr;
    int rc = upload(sc, d.nodes, size_t(std::max(n, 0)), &d_nodes);
    float4 *wide = nullptr, *wide4 = nullptr;
    const char *oom = "out of device memory for the BVH records";
    if (!rc) rc = scene_alloc(sc, 4 * size_t(std::max(n_interior, 1)) * sizeof(float4), &wide, oom);
    if (!rc) rc = scene_alloc(sc, 8 * size_t(std::max(n_interior, 1)) * sizeof(float4), &wide4, oom);
    if (rc) return rc;
    // The four-wide step never tests the two children themselves; that is exact because a child's box lies inside
    // its parent's (Union in recursiveBuild is exact). pack_wide_records verifies it for the tree we were handed; a
    // tree that violates it is traversed with binary steps only.
    S.boxes_nested = 1;
    // (where the records sit in memory is free — a reference is a record slot — and worth nothing: depth-first rank 476.2 ms,
    // scattered 476.0 on the room, profiles/r04_ab_traversal_scheduling.txt)
    rc = pack_wide_records(d_nodes, n, n_interior, wide, wide4, &S.boxes_nested, nullptr);
    if (rc) return rc;
    // the four-wide step addresses its records with 32-bit byte offsets and gives two bits of every ref to a split axis:
    // leaf refs ~prim must survive the shift
    if (n_interior >= (1 << 25) || (kRefShift && d.n_prims >= (1 << 28))) S.boxes_nested = 0;
    S.wide = wide;
    S.wide4 = wide4;
    if (n > 0) {
        std::memcpy(S.root_box, d.nodes[0].bmin, sizeof(d.nodes[0].bmin));
        std::memcpy(S.root_box + 3, d.nodes[0].bmax, sizeof(d.nodes[0].bmax));
        S.root_ref = d.nodes[0].nprims == 0 ? 0 : ~d.nodes[0].offset;  // the root is interior rank 0
    }
    return IILE_OK;
}

// The top of the four-wide tree, breadth first, for the traversal kernels' LDS copies (dtrav.h, load_wide4): the
// records are read back once, the references among the chosen ones become kTopFlag | slot, each copy keeps its own
// record index (the binary fallback step needs it) in the word behind its axes.
int build_top4(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    const int n_interior = interior_nodes(d);
    S.root_ref_top = S.root_ref;
    const int want_top = kMaxTop;
    if (n_interior == 0 || !S.boxes_nested || want_top <= 0 || S.root_ref < 0) return IILE_OK;
    std::vector<float4> all(8 * size_t(n_interior));
    if (hipMemcpy(all.data(), S.wide4, all.size() * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess)
        return api_fail(IILE_ERR_HIP, "reading back the BVH records failed");
    std::vector<int> order;       // record index per slot
    std::map<int, int> slot_of;   // record index -> slot
    order.push_back(S.root_ref);
    slot_of[S.root_ref] = 0;
    for (size_t at = 0; at < order.size() && int(order.size()) < want_top; ++at) {
        const float4 refs = all[8 * size_t(order[at]) + 6];
        const float rf[4] = {refs.x, refs.y, refs.z, refs.w};
        for (int j = 0; j < 4 && int(order.size()) < want_top; ++j) {
            int r;
            std::memcpy(&r, &rf[j], sizeof(r));
            r >>= kRefShift;  // (the low bits are a split axis)
            // (an empty slot — the second one of a leaf child — holds no box: its planes are +-inf and its ref is unused)
            const float bmin_x = (&all[8 * size_t(order[at]) + 0].x)[j];
            if (r < 0 || r >= n_interior || !(bmin_x < std::numeric_limits<float>::infinity()) || slot_of.count(r)) continue;
            slot_of[r] = int(order.size());
            order.push_back(r);
        }
    }
    std::vector<float4> top(8 * order.size());
    for (size_t sl = 0; sl < order.size(); ++sl) {
        for (int q = 0; q < 8; ++q) top[8 * sl + q] = all[8 * size_t(order[sl]) + q];
        float *refs = &top[8 * sl + 6].x;
        for (int j = 0; j < 4; ++j) {
            int raw;
            std::memcpy(&raw, &refs[j], sizeof(raw));
            const int r = raw >> kRefShift;
            const float bmin_x = (&top[8 * sl + 0].x)[j];
            if (r >= 0 && r < n_interior && bmin_x < std::numeric_limits<float>::infinity() && slot_of.count(r)) {
                const int tagged = int(uint32_t(kTopFlag | slot_of[r]) << kRefShift) | (raw & ((1 << kRefShift) - 1));
                std::memcpy(&refs[j], &tagged, sizeof(raw));
            }
        }
        std::memcpy(&top[8 * sl + 7].y, &order[sl], sizeof(int));
    }
    const int rc = upload(sc, top.data(), top.size(), &S.top4);
    if (rc) return rc;
    S.n_top = int(order.size());
    S.root_ref_top = kTopFlag | 0;
    return IILE_OK;
}

// Primitives: gathered into 48-byte vertex records + normal / uv records.
int build_prims(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    const size_t n = size_t(d.n_prims);
    S.n_prims = d.n_prims;
    std::vector<uint32_t> last_in_leaf(n, 0);
    for (int i = 0; i < d.n_nodes; ++i)
        if (d.nodes[i].nprims > 0) last_in_leaf[size_t(d.nodes[i].offset) + d.nodes[i].nprims - 1] = 16u;
    std::vector<float4> verts(3 * n + 3), norms(3 * n);  // one pad record, flagged last-in-leaf
    std::vector<float2> uvs(3 * n);
    for (size_t i = 0; i < n; ++i) {
        const float *p = d.tri_p + 9 * i, *nn = d.tri_n + 9 * i, *uv = d.tri_uv + 6 * i;
        // flag word: bits 0..3 iile_scene.h (bit 0 set for a sphere AND for a quadric: not a triangle, the shape is
        // told by prim_shape), bit 4 last primitive of its leaf, bits 5..7 shading class, bit 8 an area light (which one: the
        // third word; bits 9..11 stay clear, hit_tag in dtrav.h carries bits 5..11 along), bit 12 alpha-masked
        const uint32_t f = d.prim_flags[i];
        const bool quadric = (f & IILE_PRIM_QUADRIC) != 0;
        const int mt = d.prim_material[i] >= 0 ? d.materials[d.prim_material[i]].type : 3;
        uint32_t w[3] = {(f & 15u) | (quadric ? 1u : 0u) | (prim_masked(d, int(i)) ? 4096u : 0u) | last_in_leaf[i] |
                             shading_class(mt, (f & IILE_PRIM_SPHERE) || quadric) << 5 | (d.prim_light[i] >= 0 ? 256u : 0u),
                         uint32_t(d.prim_material[i]), uint32_t(d.prim_light[i])};
        for (int k = 0; k < 3; ++k) {
            float wf;
            std::memcpy(&wf, &w[k], 4);
            verts[3 * i + k] = make_float4(p[3 * k], p[3 * k + 1], p[3 * k + 2], wf);
            norms[3 * i + k] = make_float4(nn[3 * k], nn[3 * k + 1], nn[3 * k + 2], 0.f);
            uvs[3 * i + k] = make_float2(uv[2 * k], uv[2 * k + 1]);
        }
    }
    const uint32_t last = 16u;
    float lf;
    std::memcpy(&lf, &last, 4);
    verts[3 * n] = verts[3 * n + 1] = verts[3 * n + 2] = make_float4(0, 0, 0, lf);
    int rc = upload(sc, verts.data(), verts.size(), &S.tri_verts);
    if (!rc) rc = upload(sc, norms.data(), norms.size(), &S.tri_norms);
    if (!rc) rc = upload(sc, uvs.data(), uvs.size(), &S.tri_uv);
    if (rc) return rc;
    // a quadric primitive's shape is ~(its quadric index) on the device: the sign tells the shape's kind (dtrav.h)
    std::vector<int> shape(d.prim_shape, d.prim_shape + n);
    sc->prim_is_shape.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (d.prim_flags[i] & IILE_PRIM_QUADRIC) shape[i] = ~shape[i];
        sc->prim_is_shape[i] = (d.prim_flags[i] & (IILE_PRIM_SPHERE | IILE_PRIM_QUADRIC)) ? 1 : 0;
    }
    rc = upload(sc, shape.data(), shape.size(), &S.prim_shape);
    if (rc) return rc;
    if (!S.has_alpha) return IILE_OK;
    std::vector<int2> masks(n);
    for (size_t i = 0; i < n; ++i) masks[i] = make_int2(d.prim_alpha[2 * i], d.prim_alpha[2 * i + 1]);
    return upload(sc, masks.data(), masks.size(), &S.prim_alpha);
}

int build_shapes(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    S.n_spheres = d.n_spheres, S.n_quadrics = d.n_quadrics;
    std::vector<DSphere> sp(d.n_spheres);
    for (int i = 0; i < d.n_spheres; ++i) {
        const iile_sphere &s = d.spheres[i];
        std::memcpy(sp[i].o2w.m, s.o2w, 64);
        std::memcpy(sp[i].o2w_inv.m, s.o2w_inv, 64);
        sp[i].radius = s.radius, sp[i].zmin = s.zmin, sp[i].zmax = s.zmax;
        sp[i].theta_min = s.theta_min, sp[i].theta_max = s.theta_max, sp[i].phi_max = s.phi_max;
        sp[i].reverse_orientation = s.reverse_orientation, sp[i].swaps_handedness = s.swaps_handedness;
        // xf_point(o2w, (0, 0, 0)) (dmath.h), operation by operation: products with zero included, the division by w as
        // a multiplication with its reciprocal (this file is compiled without contraction or fast math, host side too)
        const float *m = s.o2w;
        const float zero = 0.f;
        float c[4];
        for (int r = 0; r < 4; ++r) c[r] = m[4 * r] * zero + m[4 * r + 1] * zero + m[4 * r + 2] * zero + m[4 * r + 3];
        if (c[3] != 1) {
            const float inv = 1.f / c[3];
            for (int r = 0; r < 3; ++r) c[r] = c[r] * inv;
        }
        for (int r = 0; r < 3; ++r) sp[i].center[r] = c[r];
        sp[i].pad_ = 0.f;
    }
    const int rc = upload(sc, sp.data(), sp.size(), &S.spheres);
    if (rc) return rc;
    std::vector<DQuadric> qs(d.n_quadrics);
    for (int i = 0; i < d.n_quadrics; ++i) {
        const iile_quadric &q = d.quadrics[i];
        std::memcpy(qs[i].o2w.m, q.o2w, 64);
        std::memcpy(qs[i].o2w_inv.m, q.o2w_inv, 64);
        qs[i].kind = q.kind, qs[i].radius = q.radius, qs[i].inner_radius = q.inner_radius, qs[i].height = q.height;
        qs[i].zmin = q.zmin, qs[i].zmax = q.zmax, qs[i].phi_max = q.phi_max;
        qs[i].reverse_orientation = q.reverse_orientation, qs[i].swaps_handedness = q.swaps_handedness;
    }
    return upload(sc, qs.data(), qs.size(), &S.quadrics);
}

int build_materials(iile_scene *sc, const iile_scene_desc &d) {
    sc->ds.n_materials = d.n_materials;
    std::vector<DMaterial> mats(d.n_materials);
    bool disney = false;
    for (int i = 0; i < d.n_materials; ++i) {
        mats[i] = device_material(d.materials[i], d.n_textures);
        disney = disney || d.materials[i].type == IILE_MAT_DISNEY;
    }
    if (!disney) return upload(sc, mats.data(), mats.size(), &sc->ds.materials);
    // (this function is the only place that sets DScene::materials: disney_table's reading past the array rests on that)
    // the Disney materials' side table right behind the materials, entry for entry (disney_table, dscene.h; read at a hit on a
    // Disney material only: make_bsdf_at, dbsdf.h)
    static_assert(sizeof(DMaterial) % alignof(iile_disney) == 0, "the table behind the materials is aligned");
    const size_t mat_bytes = mats.size() * sizeof(DMaterial), dz_bytes = size_t(d.n_materials) * sizeof(iile_disney);
    std::vector<unsigned char> blob(mat_bytes + dz_bytes);
    std::memcpy(blob.data(), mats.data(), mat_bytes);
    std::memcpy(blob.data() + mat_bytes, d.disney, dz_bytes);
    const unsigned char *dev = nullptr;
    if (const int rc = upload(sc, blob.data(), blob.size(), &dev)) return rc;
    sc->ds.materials = reinterpret_cast<const DMaterial *>(dev);
    return IILE_OK;
}

// Textures: the host-built pyramids of the images, texels widened to float4 (one 16-byte load each); the procedural
// ones' fields.
int build_textures(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    S.n_textures = d.n_textures;
    if (d.n_textures <= 0) return IILE_OK;
    std::vector<DTexture> tx(d.n_textures);
    for (int i = 0; i < d.n_textures; ++i) {
        const iile_texture &t = d.textures[i];
        tx[i].kind = t.kind, tx[i].mapping = t.mapping, tx[i].aamode = t.aamode;
        std::memcpy(tx[i].vs, t.vs, sizeof(t.vs));
        std::memcpy(tx[i].vt, t.vt, sizeof(t.vt));
        std::memcpy(tx[i].xf, t.xf, sizeof(t.xf));
        std::memcpy(tx[i].cval, t.cval, sizeof(t.cval));
        std::memcpy(tx[i].bilerp, t.bilerp, sizeof(t.bilerp));
        for (int k = 0; k < 3; ++k) tx[i].child[k] = texture_input(t, k);
        tx[i].n_levels = t.n_levels, tx[i].wrap = t.wrap, tx[i].trilinear = t.trilinear, tx[i].max_aniso = t.max_aniso;
        tx[i].su = t.su, tx[i].sv = t.sv, tx[i].du = t.du, tx[i].dv = t.dv;
        for (int l = 0; l < kMaxTexLevels; ++l) {
            tx[i].level_w[l] = l < t.n_levels ? t.level_w[l] : 1;
            tx[i].level_h[l] = l < t.n_levels ? t.level_h[l] : 1;
            tx[i].level_offset[l] = l < t.n_levels ? t.level_offset[l] : 0;
        }
    }
    std::vector<float4> tex4(size_t(d.n_texels));
    for (int64_t i = 0; i < d.n_texels; ++i)
        tex4[size_t(i)] = make_float4(d.texels[3 * i], d.texels[3 * i + 1], d.texels[3 * i + 2], 0.f);
    int rc = upload(sc, tx.data(), tx.size(), &S.textures);
    if (!rc) rc = upload(sc, tex4.data(), tex4.size(), &S.texels);
    if (!rc) rc = upload(sc, d.ewa_lut, size_t(IILE_EWA_LUT_SIZE), &S.ewa_lut);
    return rc;
}

int build_lights(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    S.n_lights = d.n_lights;
    sc->light_samples.resize(size_t(d.n_lights));
    for (int i = 0; i < d.n_lights; ++i) sc->light_samples[size_t(i)] = std::max(1, int(d.lights[i].n_samples));
    for (int i = 0; i < d.n_lights; ++i) sc->light_types.push_back(d.lights[i].type);
    std::vector<DLight> lts(d.n_lights);
    for (int i = 0; i < d.n_lights; ++i) {
        const iile_light &l = d.lights[i];
        std::memcpy(lts[i].lemit, l.lemit, sizeof(l.lemit)), std::memcpy(lts[i].pos, l.pos, sizeof(l.pos));
        std::memcpy(lts[i].w2l, l.w2l, sizeof(l.w2l)), std::memcpy(lts[i].l2w, l.l2w, sizeof(l.l2w));
        lts[i].two_sided = l.two_sided, lts[i].sphere = l.sphere, lts[i].type = l.type, lts[i].prim = l.prim;
        lts[i].quadric = l.type == IILE_LIGHT_AREA_QUADRIC ? d.prim_shape[l.prim] : -1;
        lts[i].cos_total_width = l.cos_total_width, lts[i].cos_falloff_start = l.cos_falloff_start, lts[i].world_radius = l.world_radius;
        lts[i].env_tex = l.env_tex, lts[i].dist_w = l.dist_w, lts[i].dist_h = l.dist_h, lts[i].dist_offset = l.dist_offset;
    }
    int rc = upload(sc, lts.data(), lts.size(), &S.lights);
    if (!rc) rc = upload(sc, d.env_dist, size_t(d.n_env_dist), &S.env_dist);
    return rc;
}

// HaltonSampler::GetIndexForSample's per-pixel offset (halton.cpp:96-122) depends only on the pixel modulo
// kMaxResolution = 128: tabulated once (integer arithmetic, exact)
std::vector<uint32_t> halton_pixel_offsets(const int32_t *scales, const int32_t *exps, int32_t stride, const int32_t *mult_inv) {
    static_assert(kPixelOffsets == 128 * 128, "camera_motion (dscene.h) lies behind exactly these offsets");
    std::vector<uint32_t> offs(kPixelOffsets, 0u);
    if (stride <= 1) return offs;
    for (int pmy = 0; pmy < 128; ++pmy)
        for (int pmx = 0; pmx < 128; ++pmx) {
            uint32_t inv = uint32_t(pmx), idx0 = 0, idx1 = 0;  // InverseRadicalInverse<2>, <3>
            for (int i = 0; i < exps[0]; ++i) {
                idx0 = idx0 * 2 + (inv & 1);
                inv >>= 1;
            }
            inv = uint32_t(pmy);
            for (int i = 0; i < exps[1]; ++i) {
                idx1 = idx1 * 3 + inv % 3;
                inv /= 3;
            }
            const unsigned long long off =
                (unsigned long long)idx0 * (unsigned long long)(stride / scales[0]) * (unsigned long long)mult_inv[0] +
                (unsigned long long)idx1 * (unsigned long long)(stride / scales[1]) * (unsigned long long)mult_inv[1];
            offs[pmy * 128 + pmx] = uint32_t(off % (unsigned long long)stride);
        }
    return offs;
}

// Halton: permutations + per-dimension constants, the pixel offsets; the IISPT probe pass's own film and sampler
// (iile_probe_setup).
int build_halton(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    const iile_halton &h = d.halton;
    std::vector<DHaltonDim> dims(h.n_dims);
    for (int i = 0; i < h.n_dims; ++i) {
        const uint32_t base = uint32_t(h.primes[i]);
        dims[i].base = base;
        dims[i].perm_offset = uint32_t(h.prime_sums[i]);
        const float inv_base = 1.f / float(int(base));
        dims[i].inv_base = inv_base;
        dims[i].perm0_term = inv_base * h.perms[h.prime_sums[i]] / (1 - inv_base);
        dims[i].base_d = double(base);
        dims[i].inv_base_d = 1.0 / double(base);
    }
    int rc = upload(sc, h.perms, size_t(h.n_perms), &S.perms);
    if (!rc) rc = upload(sc, dims.data(), dims.size(), &S.hdims);
    if (rc) return rc;
    S.n_hdims = h.n_dims, S.n_perms = h.n_perms, S.sample_stride = h.sample_stride, S.sample_center = h.sample_at_pixel_center;
    S.base_scale0 = h.base_scales[0], S.base_scale1 = h.base_scales[1], S.base_exp0 = h.base_exponents[0], S.base_exp1 = h.base_exponents[1];
    S.mult_inv0 = h.mult_inverse[0], S.mult_inv1 = h.mult_inverse[1];
    sc->spp = h.spp;
    std::vector<uint32_t> offs = halton_pixel_offsets(h.base_scales, h.base_exponents, h.sample_stride, h.mult_inverse);
    offs.resize(size_t(kPixelOffsets) + (sizeof(DCameraMotion) + 3) / 4, 0u);  // room for a moving camera's record (camera_motion, dscene.h)
    sc->probe = d.probe;
    if (d.probe.hemi_size > 0 && d.probe.sample_stride > 0) {
        const std::vector<uint32_t> poffs =
            halton_pixel_offsets(d.probe.base_scales, d.probe.base_exponents, d.probe.sample_stride, d.probe.mult_inverse);
        rc = upload(sc, poffs.data(), poffs.size(), &sc->probe_pixel_offsets);
        if (!rc) rc = upload(sc, d.probe.filter_table, size_t(256), &sc->probe_filter_table);
        if (rc) return rc;
    }
    return upload(sc, offs.data(), offs.size(), &S.pixel_offsets);
}

// SobolSampler in place of the Halton sampler (iile_sobol): matrices [n_dims][32], then vdc[32], vdc_inv[32]; and the
// same columns as XOR tables per byte of the index
int build_sobol(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    const iile_sobol &sb = d.sobol;
    if (!sb.enabled) return IILE_OK;
    std::vector<uint32_t> tab(size_t(sb.n_dims) * 32 + 64);
    std::memcpy(tab.data(), sb.matrices32, size_t(sb.n_dims) * 32 * sizeof(uint32_t));
    std::memcpy(tab.data() + size_t(sb.n_dims) * 32, sb.vdc, 32 * sizeof(uint32_t));
    std::memcpy(tab.data() + size_t(sb.n_dims) * 32 + 32, sb.vdc_inv, 32 * sizeof(uint32_t));
    int rc = upload(sc, tab.data(), tab.size(), &S.sobol_mat);
    if (rc) return rc;
    S.sobol_vdc = S.sobol_mat + size_t(sb.n_dims) * 32;
    auto byte_tables = [](const uint32_t *cols, int n_cols, uint32_t *out) {  // out[4][256]
        for (int q = 0; q < 4; ++q)
            for (int v = 0; v < 256; ++v) {
                uint32_t x = 0;
                for (int j = 0; j < 8; ++j)
                    if (((v >> j) & 1) && 8 * q + j < n_cols) x ^= cols[8 * q + j];
                out[q * 256 + v] = x;
            }
    };
    std::vector<uint32_t> bt(size_t(sb.n_dims) * 1024 + 2048);
    for (int dd = 0; dd < sb.n_dims; ++dd) byte_tables(sb.matrices32 + size_t(dd) * 32, 32, bt.data() + size_t(dd) * 1024);
    const int m2 = 2 * sb.log2_resolution;
    byte_tables(sb.vdc, 32 - m2, bt.data() + size_t(sb.n_dims) * 1024);          // bits of the sample number k
    byte_tables(sb.vdc_inv, m2, bt.data() + size_t(sb.n_dims) * 1024 + 1024);    // bits of the pixel word b
    rc = upload(sc, bt.data(), bt.size(), &S.sobol_bt);
    if (rc) return rc;
    S.sobol_vdc_bt = S.sobol_bt + size_t(sb.n_dims) * 1024;
    S.sobol = 1, S.sobol_log2res = sb.log2_resolution, S.sobol_res = sb.resolution, S.sobol_dims = sb.n_dims;
    sc->spp = sb.spp;
    return IILE_OK;
}

int build_camera_film(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    std::memcpy(S.raster_to_camera.m, d.camera.raster_to_camera, 64);
    std::memcpy(S.camera_to_world.m, d.camera.camera_to_world, 64);
    S.lens_radius = d.camera.lens_radius, S.focal_distance = d.camera.focal_distance;
    S.env_camera = iile_camera_kind(&d.camera) == IILE_CAMERA_ENVIRONMENT ? 1 : 0;
    std::memcpy(S.dx_camera, d.camera.dx_camera, sizeof(S.dx_camera));
    std::memcpy(S.dy_camera, d.camera.dy_camera, sizeof(S.dy_camera));
    S.diff_scale = 1 / std::sqrt(float(d.halton.spp));  // integrator.cpp:284-285
    S.filter_wide = d.film_filter_wide;
    const int rc = upload(sc, d.film_filter_table, size_t(256), &S.filter_table);
    if (rc) return rc;
    const iile_film_desc &f = d.film;
    S.xres = f.xres, S.yres = f.yres;
    S.crop_x0 = f.crop_x0, S.crop_y0 = f.crop_y0, S.crop_x1 = f.crop_x1, S.crop_y1 = f.crop_y1;
    S.samp_x0 = f.samp_x0, S.samp_y0 = f.samp_y0, S.samp_x1 = f.samp_x1, S.samp_y1 = f.samp_y1;
    // "pixelbounds" (iile_integrator::pixel_bounds; all zero = not given, as a caller that never heard of the field leaves it)
    const int32_t *pb = d.integrator.pixel_bounds;
    const bool given = pb[0] != 0 || pb[1] != 0 || pb[2] != 0 || pb[3] != 0;
    S.pb_x0 = given ? std::max(pb[0], f.samp_x0) : f.samp_x0, S.pb_y0 = given ? std::max(pb[1], f.samp_y0) : f.samp_y0;
    S.pb_x1 = given ? std::min(pb[2], f.samp_x1) : f.samp_x1, S.pb_y1 = given ? std::min(pb[3], f.samp_y1) : f.samp_y1;
    S.pb_set = (S.pb_x0 != f.samp_x0 || S.pb_y0 != f.samp_y0 || S.pb_x1 != f.samp_x1 || S.pb_y1 != f.samp_y1) ? 1 : 0;
    S.filter_rx = f.filter_rx, S.filter_ry = f.filter_ry, S.max_sample_luminance = f.max_sample_luminance;
    S.max_depth = d.integrator.max_depth, S.rr_threshold = d.integrator.rr_threshold;
    sc->max_depth = d.integrator.max_depth;
    sc->shutter[0] = d.camera.shutter_open, sc->shutter[1] = d.camera.shutter_close;
    return IILE_OK;
}

// What a render needs besides the scene: the traversal stacks' spill buffers, the NEE stream and its events, the timing
// events and the flagged-sample records.
int build_runtime(iile_scene *sc, const iile_scene_desc &) {
    int rc = scene_alloc(sc, size_t(max_traversal_threads(sc->n_cus)) * sizeof(int), &sc->spill, "hipMalloc(spill) failed");
    if (!rc) rc = scene_alloc(sc, size_t(max_traversal_threads(sc->n_cus)) * sizeof(int), &sc->spill_nee, "hipMalloc(spill) failed");
    if (!rc) rc = scene_alloc(sc, 256 + size_t(kMaxFlagged) * 6 * sizeof(float), &sc->flag_count, "hipMalloc(flag records) failed");
    if (rc) return rc;
    sc->flag_rec = reinterpret_cast<float *>(reinterpret_cast<char *>(sc->flag_count) + 256);
    if (hipStreamCreateWithFlags(&sc->nee_stream, hipStreamNonBlocking) != hipSuccess) return api_fail(IILE_ERR_HIP, "hipStreamCreate failed");
    for (int i = 0; i < 16; ++i)
        if (hipEventCreateWithFlags(&sc->ev_shade[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&sc->ev_nee[i], hipEventDisableTiming) != hipSuccess)
            return api_fail(IILE_ERR_HIP, "hipEventCreate failed");
    if (hipEventCreate(&sc->ev_begin) != hipSuccess || hipEventCreate(&sc->ev_end) != hipSuccess) return api_fail(IILE_ERR_HIP, "hipEventCreate failed");
    return IILE_OK;
}

// More than one light: tabulate the spatial light distribution (lightdistrib.cpp:91-299) for every voxel of its grid
// (light_grid). A Distribution1D over the n lights is a record func[n] | cdf[n + 1] | funcInt.
int build_light_distribution(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    S.light_nv[0] = S.light_nv[1] = S.light_nv[2] = 1;
    const int n = d.n_lights;
    const size_t stride = light_record_floats(n);
    if (n > 1 && d.integrator.light_strategy != IILE_LIGHTS_SPATIAL) {
        // UniformLightDistribution / PowerLightDistribution (lightdistrib.cpp:65-82, integrator.cpp:217-225): one
        // Distribution1D for every point — a grid of a single voxel, built here (sampling.h:57-69)
        std::vector<float> tab(stride, 0.f);
        // (the first IILE_MAX_LIGHTS powers have always been the integrator's; a descriptor with no more lights may end before light_power_all)
        const float *power = n > IILE_MAX_LIGHTS ? d.light_power_all : d.integrator.light_power;
        float *func = tab.data(), *cdf = tab.data() + n;
        for (int i = 0; i < n; ++i) func[i] = d.integrator.light_strategy == IILE_LIGHTS_UNIFORM ? 1.f : power[i];
        cdf[0] = 0;
        for (int i = 1; i < n + 1; ++i) cdf[i] = cdf[i - 1] + func[i - 1] / n;
        const float func_int = cdf[n];
        if (func_int == 0)
            for (int i = 1; i < n + 1; ++i) cdf[i] = float(i) / float(n);
        else
            for (int i = 1; i < n + 1; ++i) cdf[i] /= func_int;
        tab[2 * size_t(n) + 1] = func_int;
        return upload(sc, tab.data(), tab.size(), &S.light_dist);
    }
    if (!spatial_table(d)) return IILE_OK;
    light_grid(d, S.light_nv);
    // RadicalInverse(0..4, i), i < 128 (lowdiscrepancy.cpp:389-444): bases 2, 3, 5, 7, 11
    std::vector<float> samples(128 * 5);
    const int bases[5] = {2, 3, 5, 7, 11};
    for (int i = 0; i < 128; ++i)
        for (int b = 0; b < 5; ++b) {
            if (b == 0) {
                uint64_t v = uint64_t(i), r = 0;  // ReverseBits64(a) * 0x1p-64
                for (int k = 0; k < 64; ++k) r |= ((v >> k) & 1ull) << (63 - k);
                samples[5 * i] = float(double(r) * 0x1p-64);
                continue;
            }
            const float inv_base = 1.f / float(bases[b]);
            uint64_t a = uint64_t(i), rev = 0;
            float inv_base_n = 1;
            while (a) {
                const uint64_t next = a / uint64_t(bases[b]);
                rev = rev * uint64_t(bases[b]) + (a - next * uint64_t(bases[b]));
                inv_base_n *= inv_base;
                a = next;
            }
            samples[5 * i + b] = std::min(float(rev) * inv_base_n, 0x1.fffffep-1f);
        }
    const float *dsamples = nullptr;
    float *dist = nullptr;
    const size_t n_vox = size_t(S.light_nv[0]) * S.light_nv[1] * S.light_nv[2];
    int rc = upload(sc, samples.data(), samples.size(), &dsamples);
    if (!rc) rc = scene_alloc(sc, n_vox * stride * sizeof(float), &dist, "hipMalloc(light distributions) failed");
    if (rc) return rc;
    S.light_dist = dist;
    LaunchCfg cfg{sc->n_cus, nullptr, false};
    launch_light_distributions(S, dsamples, dist, cfg);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return api_fail(IILE_ERR_HIP, "light distribution kernel failed");
    return IILE_OK;
}

// The Halton sampler's values for the whole frame (DScene::stab_*): a sample's index is offset(pixel mod 128) + k * stride, so
// a frame of any size draws from 128 * 128 * spp distinct samples, and everything they depend on — permutations, bases, stride,
// spp, maxdepth, samplepixelcenter — is fixed here. One kernel fills the table with the digit chains' own floats. No table:
// Sobol' (its sampler is four table lookups already), maxdepth 0, a table over the budget, IILE_NO_SAMPLE_TABLE set.
int build_sample_table(iile_scene *sc, const iile_scene_desc &d) {
    DScene &S = sc->ds;
    clear_sample_table(&S);
    sc->sample_table_bytes = 0;
    const int64_t spp = d.halton.spp;
    if (S.sobol || S.max_depth <= 0 || spp <= 0 || S.sample_stride <= 0 || std::getenv("IILE_NO_SAMPLE_TABLE")) return IILE_OK;
    if (5 + 7 * int64_t(S.max_depth) >= int64_t(S.n_hdims)) return IILE_OK;  // the last record's last dimension: 12 + 7 (maxdepth - 1)
    const bool lens = S.lens_radius > 0;
    // (a moving camera's time column, 4 bytes a slot more, is counted when the motion arrives: iile_scene_set_camera_motion)
    const uint64_t per_slot = uint64_t(32) * uint64_t(S.max_depth) + (lens ? 16 : 8);
    if (uint64_t(spp) > sample_table_budget() / (uint64_t(16384) * per_slot)) return IILE_OK;
    const uint64_t slots = uint64_t(16384) * uint64_t(spp);  // (< 2^32: the budget is far below 2^32 slots of 40 bytes or more)
    if (slots >= (uint64_t(1) << 32)) return IILE_OK;
    const auto t0 = std::chrono::steady_clock::now();
    S.stab_slots = uint32_t(slots), S.stab_spp = uint32_t(spp);
    if (spp > 1) {
        // slot / spp as div_magic wants it (Granlund-Montgomery, round-up form): l = ceil(log2 spp), magic = floor(2^32 (2^l - spp) / spp) + 1
        int l = 0;
        while ((uint64_t(1) << l) < uint64_t(spp)) ++l;
        S.stab_spp_magic = uint32_t((((uint64_t(1) << l) - uint64_t(spp)) << 32) / uint64_t(spp) + 1);
        S.stab_spp_shift = uint32_t(l - 1);
    }
    // one allocation, carved cam | lens | shade. The table only saves work: where the device has no room for it the scene does
    // without, as it does over the budget (a 2.6 GiB table beside a nearly full card must not fail the scene)
    float2 *cam = nullptr, *lens_part = nullptr;
    float4 *shade = nullptr;
    auto layout = [&](Carver c) {
        cam = c.take<float2>(slots);
        if (lens) lens_part = c.take<float2>(slots);
        shade = c.take<float4>(slots * uint64_t(S.max_depth) * 2);
        return c.used;
    };
    void *block = nullptr;
    if (hipMalloc(&block, layout(Carver())) != hipSuccess) {
        (void)hipGetLastError();  // (the failure is answered here)
        clear_sample_table(&S);
        return IILE_OK;
    }
    sc->allocs.push_back(block);
    sc->stab_block = block;
    layout(Carver(block));
    launch_sample_table(S, cam, lens_part, shade, LaunchCfg{sc->n_cus, nullptr, false});
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return api_fail(IILE_ERR_HIP, "sample table kernel failed");
    S.stab_cam = cam, S.stab_lens = lens_part, S.stab_shade = shade;
    sc->sample_table_bytes = slots * per_slot;
    if (std::getenv("IILE_TIMING"))
        fprintf(stderr, "iile timing: sample table of %.1f MiB built in %.3f s\n", double(sc->sample_table_bytes) / 1048576.0,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return IILE_OK;
}

}  // namespace

namespace iile {
namespace {
uint64_t g_table_budget_override = 0;  // iile_test_sample_table_budget
}
uint64_t sample_table_budget() { return g_table_budget_override ? g_table_budget_override : kSampleTableBudget; }
void set_sample_table_budget(uint64_t bytes) { g_table_budget_override = bytes; }
}  // namespace iile

extern "C" {

const char *iile_last_error(void) { return g_err.c_str(); }

int iile_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int iile_device_select(int32_t device) {
    int rc = ensure_device();
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    return IILE_OK;
}
int iile_device_alloc(uint64_t bytes, void **out_dev) {
    if (!out_dev) return api_fail(IILE_ERR_ARG, "iile_device_alloc: null argument");
    int rc = ensure_device();
    if (rc) return rc;
    HIP_TRY(hipMalloc(out_dev, std::max<size_t>(size_t(bytes), 1)));
    return IILE_OK;
}
void iile_device_free(void *dev) {
    if (dev) (void)hipFree(dev);
}
int iile_device_download(void *dst_host, const void *src_dev, uint64_t bytes, void *stream) {
    if (!dst_host || !src_dev) return api_fail(IILE_ERR_ARG, "iile_device_download: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(dst_host, src_dev, size_t(bytes), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IILE_OK;
}

int iile_device_upload(void *dst_dev, const void *src_host, uint64_t bytes, void *stream) {
    if (!dst_dev || !src_host) return api_fail(IILE_ERR_ARG, "iile_device_upload: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(dst_dev, src_host, size_t(bytes), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the host buffer may be reused on return)
    return IILE_OK;
}
// A stream of the caller's own for hosts built without hipcc (the C++ IISPT host runs its whole indirect pass on one): a
// non-blocking stream, i.e. one that does not synchronise with the null stream.
int iile_stream_create(void **out_stream) {
    if (!out_stream) return api_fail(IILE_ERR_ARG, "iile_stream_create: null argument");
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out_stream = s;
    return IILE_OK;
}
int iile_stream_wait(void *stream) {
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return IILE_OK;
}
void iile_stream_destroy(void *stream) {
    if (stream) (void)hipStreamDestroy(static_cast<hipStream_t>(stream));
}
int iile_device_zero(void *dev, uint64_t bytes, void *stream) {
    if (!dev) return api_fail(IILE_ERR_ARG, "iile_device_zero: null argument");
    HIP_TRY(hipMemsetAsync(dev, 0, size_t(bytes), static_cast<hipStream_t>(stream)));
    return IILE_OK;
}

// the k* codes the kernels read are the IILE_* codes of the headers
static_assert(kLightDiffuseArea == IILE_LIGHT_DIFFUSE_AREA && kLightPoint == IILE_LIGHT_POINT &&
                  kLightSpot == IILE_LIGHT_SPOT && kLightDistant == IILE_LIGHT_DISTANT &&
                  kLightAreaTriangle == IILE_LIGHT_AREA_TRIANGLE && kLightInfinite == IILE_LIGHT_INFINITE &&
                  kLightAreaQuadric == IILE_LIGHT_AREA_QUADRIC && kLightProjection == IILE_LIGHT_PROJECTION &&
                  kLightGoniometric == IILE_LIGHT_GONIOMETRIC,
              "light type codes");
static_assert(kQuadricDisk == IILE_QUADRIC_DISK && kQuadricCylinder == IILE_QUADRIC_CYLINDER, "quadric kind codes");
static_assert(kMatMatte == IILE_MAT_MATTE && kMatPlastic == IILE_MAT_PLASTIC && kMatUber == IILE_MAT_UBER &&
                  kMatMirror == IILE_MAT_MIRROR && kMatGlass == IILE_MAT_GLASS && kMatMetal == IILE_MAT_METAL &&
                  kMatSubstrate == IILE_MAT_SUBSTRATE && kMatTranslucent == IILE_MAT_TRANSLUCENT && kMatDisney == IILE_MAT_DISNEY,
              "material type codes");
static_assert(kShapeHitFloats == IILE_SHAPE_HIT_FLOATS, "shape hit record");
static_assert(kTexImage == IILE_TEX_IMAGE && kTexScale == IILE_TEX_SCALE && kTexMix == IILE_TEX_MIX && kTexChecker2D == IILE_TEX_CHECKER2D &&
                  kTexChecker3D == IILE_TEX_CHECKER3D && kTexUV == IILE_TEX_UV && kTexBilerp == IILE_TEX_BILERP && kMapUV == IILE_MAP_UV &&
                  kMapSpherical == IILE_MAP_SPHERICAL && kMapCylindrical == IILE_MAP_CYLINDRICAL && kMapPlanar == IILE_MAP_PLANAR &&
                  kAAClosedForm == IILE_AA_CLOSEDFORM && kAANone == IILE_AA_NONE,
              "texture kinds");
int iile_scene_create(const iile_scene_desc *d, iile_scene **out) {
    if (!d || !out) return api_fail(IILE_ERR_ARG, "iile_scene_create: null argument");
    int rc = check_scene_desc(*d);
    if (!rc) rc = ensure_device();
    if (rc) return rc;
    iile_scene *sc = new iile_scene;
    std::memset(&sc->ds, 0, sizeof(sc->ds));
    std::memset(&sc->pb, 0, sizeof(sc->pb));
    std::memset(&sc->fb, 0, sizeof(sc->fb));
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
        sc->n_cus = prop.multiProcessorCount;
    set_kernel_flags(*d, sc->ds);
    // (in this order: build_top4 reads back what build_bvh packed, the light distribution kernel reads the whole scene, the sample
    //  table needs the sampler, the lens and maxdepth)
    for (auto build : {build_bvh, build_top4, build_prims, build_shapes, build_materials, build_textures, build_lights, build_halton,
                       build_sobol, build_camera_film, build_runtime, build_light_distribution, build_sample_table}) {
        rc = build(sc, *d);
        if (rc) {
            iile_scene_destroy(sc);
            return rc;
        }
    }
    *out = sc;
    return IILE_OK;
}

// The camera of the scene moves from now on (iile_camera_motion, iile_scene.h): every camera ray of iile_render, iile_render_ao and
// the kernel-level probes goes through the transform interpolated at its own time. Checked first, without a device call; then
// one record goes to HBM and, where the scene has a sample table, the table's time column — unless the table with that column no
// longer fits its byte budget, or the device has no room for the column: the scene then gives the table up and renders by the
// digit chains.
int iile_scene_set_camera_motion(iile_scene *sc, const iile_camera_motion *mo) {
    if (!sc || !mo) return api_fail(IILE_ERR_ARG, "iile_scene_set_camera_motion: null argument");
    if (sc->camera_moves) return api_fail(IILE_ERR_ARG, "iile_scene_set_camera_motion: the scene's camera has a motion already");
    auto finite = [](const float *v, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(v[i])) return false;
        return true;
    };
    if (!finite(&mo->start_time, 1) || !finite(&mo->end_time, 1) || !finite(mo->camera_to_world_end, 16) || !finite(&mo->T[0][0], 6) ||
        !finite(&mo->R[0][0], 8) || !finite(&mo->S[0][0], 32))
        return api_fail(IILE_ERR_ARG, "iile_scene_set_camera_motion: a non-finite entry in the camera motion");
    if (mo->end_time < mo->start_time) return api_fail(IILE_ERR_ARG, "iile_scene_set_camera_motion: the motion ends before it starts (TransformTimes)");
    int rc = ensure_device();
    if (rc) return rc;
    DScene &S = sc->ds;
    DCameraMotion dm;
    std::memset(&dm, 0, sizeof(dm));
    dm.c2w_start = S.camera_to_world;
    std::memcpy(dm.c2w_end.m, mo->camera_to_world_end, 64);
    dm.start_time = mo->start_time, dm.end_time = mo->end_time;
    dm.shutter_open = sc->shutter[0], dm.shutter_close = sc->shutter[1];
    std::memcpy(dm.T, mo->T, sizeof(dm.T));
    std::memcpy(dm.R, mo->R, sizeof(dm.R));
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) dm.S[k][3 * i + j] = mo->S[k][4 * i + j];
    if (S.stab_cam) {
        const uint64_t slots = S.stab_slots;
        void *time = nullptr;
        if (sc->sample_table_bytes + 4 * slots <= sample_table_budget() && hipMalloc(&time, size_t(slots) * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();  // (the failure is answered here)
            time = nullptr;
        }
        if (!time) {
            // over the budget with its time column, or no room on the device for it: no table (build_sample_table's rules)
            for (void *&p : sc->allocs)
                if (p == sc->stab_block) p = nullptr;
            HIP_TRY(hipFree(sc->stab_block));
            sc->stab_block = nullptr;
            clear_sample_table(&S);
            sc->sample_table_bytes = 0;
        } else {
            sc->allocs.push_back(time);
            launch_sample_table_time(S, static_cast<float *>(time), LaunchCfg{sc->n_cus, nullptr, false});  // (reads no motion record)
            if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return api_fail(IILE_ERR_HIP, "sample table time kernel failed");
            dm.stab_time = static_cast<float *>(time);
            sc->sample_table_bytes += 4 * slots;
        }
    }
    HIP_TRY(hipMemcpy(const_cast<DCameraMotion *>(camera_motion(S)), &dm, sizeof(dm), hipMemcpyHostToDevice));
    sc->camera_moves = true;
    return IILE_OK;
}

void iile_scene_destroy(iile_scene *sc) {
    if (!sc) return;
    for (void *p : sc->allocs) (void)hipFree(p);
    if (sc->nee_stream) (void)hipStreamDestroy(sc->nee_stream);
    for (int i = 0; i < 16; ++i) {
        if (sc->ev_shade[i]) (void)hipEventDestroy(sc->ev_shade[i]);
        if (sc->ev_nee[i]) (void)hipEventDestroy(sc->ev_nee[i]);
    }
    for (EventPair &e : sc->events) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    if (sc->ev_begin) (void)hipEventDestroy(sc->ev_begin);
    if (sc->ev_end) (void)hipEventDestroy(sc->ev_end);
    delete sc;   // (the grow-only blocks free themselves: DevBlock)
}
}  // extern "C"
