// api_iispt.hip — the IISPT half of the C ABI (include/iile_gpu.h): the direct pass (kernels_direct.hip), the probe pass
// (hemispheric cameras through run_pass, api_render.hip), the runner's slices (iispt.hip: hemi points, gather) and the film
// monitor's add / merge.
#include <cmath>
#include <cstring>

#include "api_common.h"

using namespace iile;

extern "C" {
// ---- IISPT direct pass (kernels_direct.hip) -------------------------------------
// IISPT is built around one camera — the probe gather makes "the" main camera ray (iispt.hip), the reference's reference mode fixes
// time = 0 — so every entry point of it refuses a scene whose camera moves, before any launch
static int refuse_moving_camera(const char *who) {
    return api_fail(IILE_ERR_UNSUPPORTED, std::string(who) + ": the scene has a moving camera (iile_scene_set_camera_motion); the IISPT passes render a static camera only");
}

int iile_render_direct(iile_scene *sc, const iile_direct_params *prm, double *film_rgbw) {
    if (!sc || !prm || !film_rgbw || prm->n_passes < 0 || prm->first_pass < 0) return api_fail(IILE_ERR_ARG, "iile_render_direct: bad argument");
    if (sc->camera_moves) return refuse_moving_camera("iile_render_direct");
    int rc = ensure_device();
    if (rc) return rc;
    DScene S = sc->ds;
    // reflected rays carry differentials in textured scenes (SpecularReflect, directprogressiveintegrator.cpp:165-184), built from the
    // hit's dpdu / dpdv and shading.dndu / dndv (triangles: triangle_interaction; spheres, quadrics: shape_hit_interaction<true>)
    const bool reflect_diffs = S.textured_materials && S.has_specular;
    if (S.filter_wide) return api_fail(IILE_ERR_UNSUPPORTED, "iile_render_direct: the direct pass is defined for the one-pixel box film");
    // ("pixelbounds" belongs to the path integrator: the IISPT runner hands DirectProgressiveIntegrator the film's bounds, iisptrenderrunner.cpp:608-613)
    S.pb_x0 = S.samp_x0, S.pb_y0 = S.samp_y0, S.pb_x1 = S.samp_x1, S.pb_y1 = S.samp_y1, S.pb_set = 0;
    // Glass: DirectProgressiveIntegrator::Li builds its BSDF with allowMultipleLobes = false (interaction.h:130-133), GlassMaterial
    // then adds a SpecularReflection and a SpecularTransmission lobe (glass.cpp:62-90) and both recursions fire — Li is a tree,
    // walked depth first by one thread per pixel (k_direct_tree) instead of the wavefront below.
    const bool tree = S.has_glass != 0;
    S.diff_scale = 0.25f;  // ScaleDifferentials(1 / sqrt(16)): the RandomSampler's samples per pixel
    hipStream_t stream = static_cast<hipStream_t>(prm->stream);
    LaunchCfg cfg{sc->n_cus, stream, false};
    PassDesc P;
    rc = frame_pass(sc, S, 0, 1, stream, &P);
    if (rc) return rc;
    P.slot0 = 0;
    P.n_pass_tiles = P.n_owned_tiles;
    P.k0 = 0;
    // One launch renders `batch` passes of the frame at once: path id = (pixel slot, pass of the batch) — the "sample of the pixel"
    // coordinate of the path tracer's enumeration (path_pixel). A pass of one sample per pixel leaves most of a persistent
    // traversal grid without a second ray (2 M paths over 393 k lanes); four at a time run at the path integrator's rates. Each
    // pass keeps its own seed and its own records; the fold adds a pixel's passes in pass order. Glass (one thread per pixel
    // walking a tree) stays at one pass per launch.
    int total_samples_pre = 0;
    for (int l = 0; l < std::max(S.n_lights, 0); ++l) total_samples_pre += sc->light_samples[size_t(l)];
    const uint64_t pixels64 = uint64_t(P.n_owned_tiles) * 256;
    int batch = (S.has_glass != 0) ? 1 : std::max(1, std::min(prm->n_passes, 4));
    while (batch > 1 && pixels64 * uint64_t(batch) * uint64_t(std::max(total_samples_pre, 1)) > 100000000ull) --batch;   // NEE records per level (8 passes at a time measured no faster than 4)
    P.kc = batch;
    const uint64_t n_paths64 = pixels64 * uint64_t(batch);
    if (n_paths64 > kMaxPassPaths) return api_fail(IILE_ERR_UNSUPPORTED, "iile_render_direct: frame too large for one pass");
    P.n_paths = uint32_t(n_paths64);
    const uint32_t fw = uint32_t(S.crop_x1 - S.crop_x0), fh = uint32_t(S.crop_y1 - S.crop_y0);
    const size_t film_bytes = size_t(fw) * fh * 4 * sizeof(double);
    if (P.n_paths == 0 || fw == 0 || fh == 0) return IILE_OK;
    // k_direct_shade appends one NEE record (and at most one MIS ray) per LIGHT and hit (UniformSampleAllLights), where the path
    // integrator's k_shade appends one per hit: the record planes are sized for paths x lights (a workspace sized for the
    // paths alone overflowed from 4 lights on at 1080p; found by the round-3 advisor)
    // UniformSampleAllLights takes Light::nSamples samples of every light (directprogressiveintegrator.cpp:9-18, integrator.cpp:54-83)
    const int n_lights = std::max(S.n_lights, 0), n_arrays = 5 * n_lights * 2;
    const std::vector<int> &nsamples = sc->light_samples;
    const int total_samples = total_samples_pre;
    P.direct_total_samples = total_samples;
    if (total_samples > 64)
        return api_fail(IILE_ERR_UNSUPPORTED, "iile_render_direct: " + std::to_string(total_samples) + " light samples per vertex (the lights' nsamples summed; at most 64)");
    const uint64_t n_records64 = n_paths64 * uint64_t(std::max(total_samples, 1));
    if (n_records64 > 400000000ull)
        return api_fail(IILE_ERR_UNSUPPORTED, "iile_render_direct: pixels x light samples = " + std::to_string(n_records64) + " NEE records per level exceed one pass");
    rc = ensure_workspace(sc, tree ? 1024u : uint32_t(n_records64));  // (the per-pixel tree walk queues nothing)
    if (rc) return rc;
    sc->pb.nray_out = nullptr;
    sc->pb.flag_count = nullptr;
    // E, F (5 levels) and D (5 levels x light samples) of every path, the PCG jump table, the film
    const size_t np = P.n_paths, vec = sizeof(float4);
    const int levels = S.has_specular ? 5 : 1;  // Li recurses through specular lobes only (the pass loop below stops likewise)
    P.direct_levels = levels;
    const size_t d_recs = tree ? 1 : std::max<size_t>(size_t(levels) * size_t(total_samples) * np, 1), ef_recs = tree ? 1 : size_t(levels) * np;
    const size_t def_bytes = (d_recs + 2 * ef_recs) * vec;
    const size_t jump_bytes = (size_t(n_arrays) + 1) * 2 * sizeof(unsigned long long);
    const bool with_rd = reflect_diffs && !tree;
    float4 *D = nullptr, *RD = nullptr;
    unsigned long long *jump_dev = nullptr;
    int *nsamples_dev = nullptr;
    double *film_dev = film_rgbw;
    auto layout = [&](Carver c) {
        D = c.take<float4>(d_recs + 2 * ef_recs);   // D, E, F: one range, cleared by one memset per launch
        if (with_rd) RD = c.take<float4>(4 * np);
        jump_dev = c.take<unsigned long long>((size_t(n_arrays) + 1) * 2);
        nsamples_dev = c.take<int>(size_t(n_lights));
        if (!prm->film_on_device) film_dev = c.take<double>(size_t(fw) * fh * 4);
        return c.used;
    };
    DevBlock block;   // this call's own: the per-vertex records are freed on return
    const std::string oom = "out of device memory for the direct pass (" + std::to_string(def_bytes >> 20) + " MiB of per-vertex records)";
    if ((rc = block.reserve(layout(Carver()), 0, oom.c_str()))) return rc;
    layout(Carver(block.p));
    float4 *E = D + d_recs, *F = E + ef_recs;
    {   // the stream at every array's first entry: array i (of light (i / 2) % n_lights) holds 16 x nSamples entries of two
        // floats (RandomSampler::StartPixel, random.cpp:62-72; Request2DArray(nLightSamples[j]) twice per level and light)
        std::vector<unsigned long long> jump(size_t(n_arrays + 1) * 2);
        const unsigned long long a = 0x5851f42d4c957f2dULL;
        unsigned long long A = 1, G = 0;
        for (int i = 0; i <= n_arrays; ++i) {
            jump[2 * size_t(i)] = A;
            jump[2 * size_t(i) + 1] = G;
            const int draws = i < n_arrays ? 32 * nsamples[size_t((i / 2) % std::max(n_lights, 1))] : 0;
            for (int s = 0; s < draws; ++s) {  // one more draw: state' = a state + inc
                G = G * a + 1;
                A = A * a;
            }
        }
        HIP_TRY(hipMemcpyAsync(jump_dev, jump.data(), jump_bytes, hipMemcpyHostToDevice, stream));
        if (n_lights > 0) HIP_TRY(hipMemcpyAsync(nsamples_dev, nsamples.data(), size_t(n_lights) * sizeof(int), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));  // (the vector dies with this scope)
    }
    if (!prm->accumulate) HIP_TRY(hipMemsetAsync(film_dev, 0, film_bytes, stream));
    else if (!prm->film_on_device) HIP_TRY(hipMemcpyAsync(film_dev, film_rgbw, film_bytes, hipMemcpyHostToDevice, stream));
    PassBuffers B = sc->pb;
    B.L = D;
    B.dir_E = E;
    B.dir_F = F;
    B.dir_RD = RD;
    B.dir_paths = P.n_paths;
    B.spill = sc->spill;
    P.direct_arrays = n_arrays;
    P.direct_jump = jump_dev;
    P.direct_nsamples = nsamples_dev;
    for (int i = 0; i < prm->n_passes; i += batch) {
        const int nb = std::min(batch, prm->n_passes - i);   // (the last launch may hold fewer passes: same buffers, fewer paths)
        P.kc = nb;
        P.n_paths = uint32_t(pixels64 * uint64_t(nb));
        B.dir_paths = P.n_paths;
        P.direct_seed = uint32_t(6284 + 17 * (prm->first_pass + i));
        if (tree) {
            launch_direct_tree(S, P, B, film_dev, cfg);
            HIP_TRY(hipGetLastError());
            continue;
        }
        HIP_TRY(hipMemsetAsync(B.counts, 0, kCntWords * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(D, 0, def_bytes, stream));
        launch_direct_generate(S, P, B, cfg);
        for (int d = 0; d < 5; ++d) {
            launch_extend(S, P, B, d, B.queue_cap, cfg);
            if (S.has_infinite) launch_direct_miss(S, B, d, B.queue_cap, cfg);
            launch_direct_shade(S, P, B, d, B.queue_cap, cfg);
            launch_mis(S, B, d, B.queue_cap, cfg);
            launch_mis_lit(S, B, d, B.queue_cap, cfg);
            launch_shadow(S, B, d, B.queue_cap, cfg);
            if (!S.has_specular) break;  // no mirror lobe anywhere: Li never recurses
        }
        launch_direct_fold(S, P, B, film_dev, cfg);
        HIP_TRY(hipGetLastError());
    }
    if (!prm->film_on_device) HIP_TRY(hipMemcpyAsync(film_rgbw, film_dev, film_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the per-vertex records are freed on return
    return IILE_OK;
}

// ---- IISPT probe pass ---------------------------------------------------------
namespace {
// Inverse(Matrix4x4), transform.cpp:82-141 (Gauss-Jordan, full pivoting; the pivot reciprocal is a double divide)
bool invert4(const float in[16], float out[16]) {
    int indxc[4], indxr[4];
    int ipiv[4] = {0, 0, 0, 0};
    float a[4][4];
    std::memcpy(a, in, sizeof(a));
    for (int i = 0; i < 4; i++) {
        int irow = 0, icol = 0;
        float big = 0.f;
        for (int j = 0; j < 4; j++) {
            if (ipiv[j] == 1) continue;
            for (int k = 0; k < 4; k++) {
                if (ipiv[k] == 0) {
                    if (std::abs(a[j][k]) >= big) {
                        big = std::abs(a[j][k]);
                        irow = j;
                        icol = k;
                    }
                } else if (ipiv[k] > 1)
                    return false;
            }
        }
        ++ipiv[icol];
        if (irow != icol)
            for (int k = 0; k < 4; ++k) std::swap(a[irow][k], a[icol][k]);
        indxr[i] = irow;
        indxc[i] = icol;
        if (a[icol][icol] == 0.f) return false;
        const float pivinv = float(1. / double(a[icol][icol]));
        a[icol][icol] = 1.f;
        for (int j = 0; j < 4; j++) a[icol][j] *= pivinv;
        for (int j = 0; j < 4; j++) {
            if (j == icol) continue;
            const float save = a[j][icol];
            a[j][icol] = 0;
            for (int k = 0; k < 4; k++) a[j][k] -= a[icol][k] * save;
        }
    }
    for (int j = 3; j >= 0; j--)
        if (indxr[j] != indxc[j])
            for (int k = 0; k < 4; k++) std::swap(a[k][indxr[j]], a[k][indxc[j]]);
    std::memcpy(out, a, sizeof(a));
    return true;
}
struct H3 {
    float x, y, z;
};
H3 h_normalize(H3 v) {  // Vector3::operator/ multiplies by the float reciprocal (geometry.h:242-246)
    const float inv = 1.f / std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
    return H3{v.x * inv, v.y * inv, v.z * inv};
}
H3 h_cross(H3 a, H3 b) {  // geometry.h:957-963: in double
    const double ax = a.x, ay = a.y, az = a.z, bx = b.x, by = b.y, bz = b.z;
    return H3{float((ay * bz) - (az * by)), float((az * bx) - (ax * bz)), float((ax * by) - (ay * bx))};
}
// CreateHemisphericCamera (hemispheric.cpp:109-160) over LookAt (transform.cpp:203-236)
bool make_probe_camera(const float *pos, const float *dir, DProbeCam *cam) {
    const H3 up = (dir[0] == 0.0 && dir[1] == 0.0) ? H3{0.f, 1.f, 0.f} : H3{0.f, 0.f, 1.f};
    const H3 look = H3{pos[0] + dir[0], pos[1] + dir[1], pos[2] + dir[2]};
    const H3 d = h_normalize(H3{look.x - pos[0], look.y - pos[1], look.z - pos[2]});
    const H3 c = h_cross(h_normalize(up), d);
    if (std::sqrt(c.x * c.x + c.y * c.y + c.z * c.z) == 0) return false;
    const H3 right = h_normalize(c);
    const H3 new_up = h_cross(d, right);
    const float m[16] = {right.x, new_up.x, d.x, pos[0], right.y, new_up.y, d.y, pos[1], right.z, new_up.z, d.z, pos[2], 0.f, 0.f, 0.f, 1.f};
    std::memcpy(cam->c2w.m, m, sizeof(m));
    float inv[16], minv[16];
    if (!invert4(m, inv) || !invert4(inv, minv)) return false;
    for (int r = 0; r < 3; ++r)
        for (int cidx = 0; cidx < 3; ++cidx) cam->nrm[3 * r + cidx] = minv[4 * cidx + r];  // transpose of mInv
    return true;
}
// the probe's film and sampler in place of the frame's, `max_depth` in place of the integrator's; diff_scale: ScaleDifferentials(1 / sqrt(samples per pixel))
DScene probe_scene(const iile_scene *sc, int max_depth, float diff_scale) {
    const iile_probe_setup &pr = sc->probe;
    DScene S = sc->ds;
    const iile_film_desc &f = pr.film;
    S.probe_mode = 1;
    S.xres = f.xres, S.yres = f.yres;
    S.crop_x0 = f.crop_x0, S.crop_y0 = f.crop_y0, S.crop_x1 = f.crop_x1, S.crop_y1 = f.crop_y1;
    S.samp_x0 = f.samp_x0, S.samp_y0 = f.samp_y0, S.samp_x1 = f.samp_x1, S.samp_y1 = f.samp_y1;
    S.filter_rx = f.filter_rx, S.filter_ry = f.filter_ry;
    S.max_sample_luminance = f.max_sample_luminance;
    S.filter_wide = 1;
    S.filter_table = sc->probe_filter_table;
    S.pixel_offsets = sc->probe_pixel_offsets;
    clear_sample_table(&S);  // the frame sampler's table: the probes' sampler has other offsets and another stride
    S.base_scale0 = pr.base_scales[0], S.base_scale1 = pr.base_scales[1];
    S.base_exp0 = pr.base_exponents[0], S.base_exp1 = pr.base_exponents[1];
    S.sample_stride = pr.sample_stride;
    S.mult_inv0 = pr.mult_inverse[0], S.mult_inv1 = pr.mult_inverse[1];
    S.max_depth = max_depth;
    S.sample_center = 0;  // the probes' own sampler: HaltonSampler(1, sampleBounds)
    S.sobol = 0;
    S.lens_radius = 0;
    S.diff_scale = diff_scale;
    return S;
}
}  // namespace

int iile_render_probes(iile_scene *sc, int32_t n_probes, const float *pos3, const float *dir3, float *intensity_rgb, float *normals_xyz,
                       float *distance, int32_t outputs_on_device, iile_stats *stats, void *stream_arg) {
    if (!sc || n_probes < 0 || !pos3 || !dir3 || !intensity_rgb || !normals_xyz || !distance)
        return api_fail(IILE_ERR_ARG, "iile_render_probes: null argument");
    if (sc->camera_moves) return refuse_moving_camera("iile_render_probes");
    int rc = ensure_device();
    if (rc) return rc;
    const iile_probe_setup &pr = sc->probe;
    if (pr.hemi_size <= 0 || !sc->probe_pixel_offsets) return api_fail(IILE_ERR_ARG, "iile_render_probes: the scene has no probe setup");
    if (pr.max_depth > 14) return api_fail(IILE_ERR_UNSUPPORTED, "probe maxdepth > 14");
    iile_stats st;
    std::memset(&st, 0, sizeof(st));
    if (n_probes == 0) {
        if (stats) *stats = st;
        return IILE_OK;
    }
    const DScene S = probe_scene(sc, pr.max_depth, 1.f);  // ScaleDifferentials(1 / sqrt(1 sample per pixel))
    const iile_film_desc &f = pr.film;
    const int need_dims = 5 + 8 * (pr.max_depth + 1) + 2;
    if (S.n_hdims < need_dims) return api_fail(IILE_ERR_ARG, "Halton table covers too few dimensions for the probe depth");

    hipStream_t stream = static_cast<hipStream_t>(stream_arg);
    PassDesc P;
    rc = frame_pass(sc, S, 0, 1, stream, &P);   // (n_owned_tiles is per batch, below)
    if (rc) return rc;
    P.probe_mode = 1;
    // path slots cover the film's pixel bounds only (no samples are taken elsewhere): 16 x 16 storage tiles over them
    P.probe_stx = (f.crop_x1 - f.crop_x0 + 15) / 16;
    P.probe_tiles = P.probe_stx * ((f.crop_y1 - f.crop_y0 + 15) / 16);
    P.k0 = 0;
    P.kc = 1;
    const uint32_t per_pixels = uint32_t(f.crop_x1 - f.crop_x0) * uint32_t(f.crop_y1 - f.crop_y0);
    const uint64_t slots_per_probe = uint64_t(P.probe_tiles) * 256;
    // probes per pass: bounded by the workspace budget like iile_render's passes
    const uint64_t max_paths = path_budget(430.0);
    const int batch = int(std::max<uint64_t>(1, std::min<uint64_t>(uint64_t(n_probes), max_paths / slots_per_probe)));

    std::vector<DProbeCam> cams;
    cams.resize(size_t(n_probes));
    for (int i = 0; i < n_probes; ++i)
        if (!make_probe_camera(pos3 + 3 * size_t(i), dir3 + 3 * size_t(i), &cams[size_t(i)]))
            return api_fail(IILE_ERR_ARG, "iile_render_probes: degenerate probe direction (probe " + std::to_string(i) + ")");

    LaunchCfg cfg{sc->n_cus, stream, false};
    const uint64_t batch_paths = uint64_t(batch) * slots_per_probe;
    rc = ensure_workspace(sc, uint32_t(batch_paths));
    if (rc) return rc;
    rc = ensure_film(sc, uint32_t(uint64_t(batch) * P.probe_tiles), uint32_t(uint64_t(batch) * per_pixels), batch_paths);
    if (rc) return rc;
    // cameras + aux + device-side outputs of one batch
    DProbeCam *d_cams = nullptr;
    float *d_int = nullptr, *d_nrm = nullptr, *d_dist = nullptr;
    auto layout = [&](Carver c) {
        d_cams = c.take<DProbeCam>(size_t(batch));
        sc->pb.aux = c.take<float4>(size_t(batch_paths));
        d_int = c.take<float>(size_t(batch) * per_pixels * 3);
        d_nrm = c.take<float>(size_t(batch) * per_pixels * 3);
        d_dist = c.take<float>(size_t(batch) * per_pixels);
        return c.used;
    };
    if ((rc = sc->probe_block.reserve(layout(Carver())))) return rc;
    layout(Carver(sc->probe_block.p));
    sc->pb.nray_out = nullptr;
    sc->events_used = 0;
    HIP_TRY(hipEventRecord(sc->ev_begin, stream));
    for (int first = 0; first < n_probes; first += batch) {
        const int nb = std::min(batch, n_probes - first);
        HIP_TRY(hipMemcpyAsync(d_cams, cams.data() + first, size_t(nb) * sizeof(DProbeCam), hipMemcpyHostToDevice, stream));
        P.probe_cams = d_cams;
        P.n_owned_tiles = nb * P.probe_tiles;
        P.n_paths = uint32_t(uint64_t(nb) * slots_per_probe);
        rc = run_pass(sc, S, pr.max_depth, P, cfg, false);
        if (rc) return rc;
        const size_t px = size_t(nb) * per_pixels, off = size_t(first) * per_pixels;
        // the images stay in HBM for whatever consumes them next (the network), or go through the batch's device block
        float *o_int = outputs_on_device ? intensity_rgb + 3 * off : d_int, *o_nrm = outputs_on_device ? normals_xyz + 3 * off : d_nrm;
        float *o_dist = outputs_on_device ? distance + off : d_dist;
        if (!launch_probe_film(S, P, sc->pb, nb, o_int, o_nrm, o_dist, cfg)) {
            launch_film_store(S, P, sc->pb, sc->fb, 0, 1, cfg);
            launch_film_gather(S, P, sc->fb, 1, cfg);
            launch_probe_finish(S, P, sc->pb, sc->fb, nb, o_int, o_nrm, o_dist, cfg);
        }
        HIP_TRY(hipGetLastError());
        if (!outputs_on_device) {
            HIP_TRY(hipMemcpyAsync(intensity_rgb + 3 * off, d_int, px * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(normals_xyz + 3 * off, d_nrm, px * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(distance + off, d_dist, px * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        st.n_passes++;
        st.n_paths += uint64_t(nb) * per_pixels;
    }
    HIP_TRY(hipEventRecord(sc->ev_end, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, sc->ev_begin, sc->ev_end));
    st.ms_total = ms;
    st.workspace_bytes = sc->ws_block.cap;
    sc->pb.aux = nullptr;
    if (stats) *stats = st;
    return IILE_OK;
}

// ---- IISPT reference mode: many samples per probe pixel, the reference points ------------
int iile_render_probes_reference(iile_scene *sc, int32_t n_probes, const float *pos3, const float *dir3, const iile_probe_ref_params *prm,
                                 float *intensity_rgb, float *weight_sum, float *normals_xyz, float *distance, iile_stats *stats) {
    if (!sc || n_probes < 0 || !pos3 || !dir3 || !prm || !intensity_rgb) return api_fail(IILE_ERR_ARG, "iile_render_probes_reference: null argument");
    if (sc->camera_moves) return refuse_moving_camera("iile_render_probes_reference");
    if (prm->n_samples < 1) return api_fail(IILE_ERR_ARG, "iile_render_probes_reference: n_samples < 1");
    if (prm->first_sample < 0) return api_fail(IILE_ERR_ARG, "iile_render_probes_reference: first_sample < 0");
    if (prm->max_depth < 1 || prm->max_depth > 14) return api_fail(IILE_ERR_ARG, "iile_render_probes_reference: max_depth outside 1 .. 14");
    if ((normals_xyz == nullptr) != (distance == nullptr))
        return api_fail(IILE_ERR_ARG, "iile_render_probes_reference: normals_xyz and distance come together or not at all");
    int rc = ensure_device();
    if (rc) return rc;
    const iile_probe_setup &pr = sc->probe;
    if (pr.hemi_size <= 0 || !sc->probe_pixel_offsets) return api_fail(IILE_ERR_ARG, "iile_render_probes_reference: the scene has no probe setup");
    const int spp_total = prm->spp_total > 0 ? prm->spp_total : prm->n_samples;
    const DScene S = probe_scene(sc, prm->max_depth, 1.f / std::sqrt(float(spp_total)));
    const iile_film_desc &f = pr.film;
    const int need_dims = 5 + 8 * (prm->max_depth + 1) + 2;
    if (S.n_hdims < need_dims)
        return api_fail(IILE_ERR_ARG, "Halton table covers " + std::to_string(S.n_hdims) + " dimensions, probe depth " + std::to_string(prm->max_depth) + " needs " +
                                          std::to_string(need_dims) + " (the table follows the scene's maxdepth)");
    // GetIndexForSample(k) = the pixel's first index (< sample_stride) + k sample_stride, a 32-bit number on the device
    if ((uint64_t(prm->first_sample) + uint64_t(prm->n_samples)) * uint64_t(std::max(S.sample_stride, 1)) > 0x100000000ull)
        return api_fail(IILE_ERR_UNSUPPORTED, "iile_render_probes_reference: sample " + std::to_string(int64_t(prm->first_sample) + prm->n_samples - 1) +
                                                  " of a probe pixel has a Halton index beyond 32 bits");
    const int n_ord = probe_film_tiles(S);
    if (n_ord == 0) return api_fail(IILE_ERR_UNSUPPORTED, "iile_render_probes_reference: the accumulating probe film holds films of at most 1024 pixels");
    iile_stats st;
    std::memset(&st, 0, sizeof(st));
    if (n_probes == 0) {
        if (stats) *stats = st;
        return IILE_OK;
    }
    hipStream_t stream = static_cast<hipStream_t>(prm->stream);
    PassDesc P;
    rc = frame_pass(sc, S, 0, 1, stream, &P);
    if (rc) return rc;
    P.probe_mode = 1;
    P.probe_stx = (f.crop_x1 - f.crop_x0 + 15) / 16;
    P.probe_tiles = P.probe_stx * ((f.crop_y1 - f.crop_y0 + 15) / 16);
    const uint32_t per_pixels = uint32_t(f.crop_x1 - f.crop_x0) * uint32_t(f.crop_y1 - f.crop_y0);
    const uint64_t slots_per_probe = uint64_t(P.probe_tiles) * 256;
    // One set of launches renders `group` samples of `batch` probes: path id = (probe, pixel, sample of the group), as iile_render_direct
    // groups passes — one sample of a few probes leaves most of a persistent traversal grid idle. Both are cut from the workspace
    // budget (and from 2^24 paths: beyond that nothing of a launch's fixed cost is left to spread), never from n_samples.
    const uint64_t max_paths = std::min<uint64_t>(path_budget(430.0), uint64_t(1) << 24);
    const int batch = int(std::max<uint64_t>(1, std::min<uint64_t>(uint64_t(n_probes), max_paths / slots_per_probe)));
    int group = int(std::max<uint64_t>(1, std::min<uint64_t>(uint64_t(prm->n_samples), max_paths / (uint64_t(batch) * slots_per_probe))));
    if (sc->probe_ref_group_override) group = int(std::min<uint32_t>(sc->probe_ref_group_override, uint32_t(prm->n_samples)));   // iile_test_probe_ref_group
    const uint64_t batch_paths = uint64_t(batch) * slots_per_probe * uint64_t(group);
    if (batch_paths > kMaxPassPaths) return api_fail(IILE_ERR_UNSUPPORTED, "iile_render_probes_reference: one set of launches would hold more than 200 000 000 paths");

    std::vector<DProbeCam> cams(static_cast<size_t>(n_probes));
    for (int i = 0; i < n_probes; ++i)
        if (!make_probe_camera(pos3 + 3 * size_t(i), dir3 + 3 * size_t(i), &cams[size_t(i)]))
            return api_fail(IILE_ERR_ARG, "iile_render_probes_reference: degenerate probe direction (probe " + std::to_string(i) + ")");

    LaunchCfg cfg{sc->n_cus, stream, false};
    rc = ensure_workspace(sc, uint32_t(batch_paths));
    if (rc) return rc;
    const bool on_device = prm->outputs_on_device != 0, want_aux = normals_xyz != nullptr;
    DProbeCam *d_cams = nullptr;
    float4 *d_acc = nullptr;
    float *d_int = nullptr, *d_w = nullptr, *d_nrm = nullptr, *d_dist = nullptr;
    const size_t acc_records = size_t(batch) * size_t(n_ord) * per_pixels;
    auto layout = [&](Carver c) {
        d_cams = c.take<DProbeCam>(size_t(batch));
        sc->pb.aux = c.take<float4>(size_t(batch_paths));
        d_acc = c.take<float4>(acc_records);
        if (!on_device) {
            d_int = c.take<float>(size_t(batch) * per_pixels * 3);
            d_w = c.take<float>(size_t(batch) * per_pixels);
            d_nrm = c.take<float>(size_t(batch) * per_pixels * 3);
            d_dist = c.take<float>(size_t(batch) * per_pixels);
        }
        return c.used;
    };
    if ((rc = sc->probe_block.reserve(layout(Carver())))) return rc;
    layout(Carver(sc->probe_block.p));
    struct AuxGuard {  // (error returns below must not leave the scene pointing into the block)
        PassBuffers *pb;
        ~AuxGuard() { pb->aux = nullptr; }
    } aux_guard{&sc->pb};
    sc->pb.nray_out = nullptr;
    sc->events_used = 0;
    HIP_TRY(hipEventRecord(sc->ev_begin, stream));
    HIP_TRY(hipMemsetAsync(sc->pb.counters, 0, sizeof(DCounters), stream));
    for (int first = 0; first < n_probes; first += batch) {
        const int nb = std::min(batch, n_probes - first);
        HIP_TRY(hipMemcpyAsync(d_cams, cams.data() + first, size_t(nb) * sizeof(DProbeCam), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(d_acc, 0, size_t(nb) * size_t(n_ord) * per_pixels * sizeof(float4), stream));
        P.probe_cams = d_cams;
        P.n_owned_tiles = nb * P.probe_tiles;
        const size_t px = size_t(nb) * per_pixels, off = size_t(first) * per_pixels;
        float *o_int = on_device ? intensity_rgb + 3 * off : d_int;
        float *o_w = weight_sum ? (on_device ? weight_sum + off : d_w) : nullptr;
        float *o_nrm = want_aux ? (on_device ? normals_xyz + 3 * off : d_nrm) : nullptr, *o_dist = want_aux ? (on_device ? distance + off : d_dist) : nullptr;
        for (int g0 = 0; g0 < prm->n_samples; g0 += group) {
            P.k0 = prm->first_sample + g0;
            P.kc = std::min(group, prm->n_samples - g0);
            P.n_paths = uint32_t(uint64_t(nb) * slots_per_probe * uint64_t(P.kc));
            rc = run_pass(sc, S, prm->max_depth, P, cfg, false);
            if (rc) return rc;
            // (normals and distances: the first hits of sample first_sample, path 0 of every pixel of the first group)
            launch_probe_film_add(S, P, sc->pb, nb, d_acc, n_ord, g0 == 0 ? o_nrm : nullptr, g0 == 0 ? o_dist : nullptr, cfg);
            HIP_TRY(hipGetLastError());
            st.n_passes++;
            st.n_paths += uint64_t(nb) * per_pixels * uint64_t(P.kc);
        }
        launch_probe_film_resolve(S, P, nb, d_acc, n_ord, o_int, o_w, cfg);
        HIP_TRY(hipGetLastError());
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(intensity_rgb + 3 * off, d_int, px * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
            if (weight_sum) HIP_TRY(hipMemcpyAsync(weight_sum + off, d_w, px * sizeof(float), hipMemcpyDeviceToHost, stream));
            if (want_aux) {
                HIP_TRY(hipMemcpyAsync(normals_xyz + 3 * off, d_nrm, px * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipMemcpyAsync(distance + off, d_dist, px * sizeof(float), hipMemcpyDeviceToHost, stream));
            }
        }
        HIP_TRY(hipStreamSynchronize(stream));   // (the next batch reuses the cameras, the sums and the staging images)
    }
    HIP_TRY(hipEventRecord(sc->ev_end, stream));
    DCounters c;
    HIP_TRY(hipMemcpyAsync(&c, sc->pb.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, sc->ev_begin, sc->ev_end));
    st.ms_total = ms;
    st.mis_rays_traced = c.mis_traced, st.ext_rays_traced = c.ext_traced;
    st.workspace_bytes = sc->ws_block.cap;
    if (stats) *stats = st;
    return IILE_OK;
}

int iile_test_probe_ref_group(iile_scene *sc, uint32_t samples_per_group) {
    if (!sc) return api_fail(IILE_ERR_ARG, "iile_test_probe_ref_group: null scene");
    sc->probe_ref_group_override = samples_per_group;
    return IILE_OK;
}

int iile_reference_points(iile_scene *sc, int32_t n, const float *pfilm2, uint8_t *valid, float *pos3, float *dir3) {
    if (!sc || n < 0 || !pfilm2 || !valid || !pos3 || !dir3) return api_fail(IILE_ERR_ARG, "iile_reference_points: bad argument");
    if (sc->camera_moves) return refuse_moving_camera("iile_reference_points");
    int rc = ensure_device();
    if (rc) return rc;
    if (n == 0) return IILE_OK;
    DevBuf<float> dpf, dpos, ddir;
    DevBuf<float4> dro, drd, dh;
    DevBuf<uint8_t> dv;
    const size_t m = size_t(n);
    if ((rc = dpf.put(pfilm2, 2 * m)) || (rc = dro.alloc(m)) || (rc = drd.alloc(m)) || (rc = dh.alloc(2 * m)) || (rc = dv.alloc(m)) || (rc = dpos.alloc(3 * m)) ||
        (rc = ddir.alloc(3 * m)))
        return rc;
    DScene S = sc->ds;
    S.diff_scale = 1.f;  // ray.ScaleDifferentials(1), iispt.cpp:517
    const LaunchCfg cfg{sc->n_cus, nullptr, false};
    launch_reference_rays(S, n, dpf.p, dro.p, drd.p, cfg);
    launch_trace(S, n, dro.p, drd.p, dh.p, 0, nullptr, sc->spill, cfg);
    launch_reference_points(S, n, dro.p, drd.p, dh.p, dv.p, dpos.p, ddir.p, cfg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = dv.get(valid, m)) || (rc = dpos.get(pos3, 3 * m)) || (rc = ddir.get(dir3, 3 * m))) return rc;
    return IILE_OK;
}

// ---- the IISPT runner's gather ----------------------------------------------------
namespace {
int iispt_check(iile_scene *sc, const iile_iispt_task *t, int *nx, int *ny) {
    if (!sc || !t) return api_fail(IILE_ERR_ARG, "iile_iispt: null argument");
    int rc = ensure_device();
    if (rc) return rc;
    if (t->x1 <= t->x0 || t->y1 <= t->y0 || t->tilesize < 1) return api_fail(IILE_ERR_ARG, "iile_iispt: empty task or tilesize < 1");
    if (sc->ds.sobol) return api_fail(IILE_ERR_UNSUPPORTED, "iile_iispt: the runner's camera samples need the scene's Halton sampler");
    if (sc->probe.hemi_size != 32) return api_fail(IILE_ERR_UNSUPPORTED, "iile_iispt: the gather is built for 32 x 32 hemispheres (iisptHemiSize)");
    *nx = iile_iispt_grid_count(t->x0, t->x1, t->tilesize);
    *ny = iile_iispt_grid_count(t->y0, t->y1, t->tilesize);
    if (uint64_t(t->counter_base) + uint64_t(*nx) * uint64_t(*ny) + uint64_t(t->x1 - t->x0) * uint64_t(t->y1 - t->y0) >= 0x7fffffffull)
        return api_fail(IILE_ERR_UNSUPPORTED, "iile_iispt: the sampler's pixel counter would pass INT_MAX");
    return IILE_OK;
}

// The items of a task in HBM: hemi points first, then (with_pixels) the film pixels. Everything a call needs on the device is
// carved from the scene's scratch block (grown on demand, kept): the runner makes hundreds of calls per frame.
// Reserve once per use (may reallocate — after the stream has drained — : nothing of an earlier use is live), then carve.
int scratch_reserve(iile_scene *sc, size_t bytes, hipStream_t stream) {
    if (sc->scratch.holds(bytes)) return IILE_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    return sc->scratch.reserve(bytes, std::max<size_t>(2 * bytes, size_t(1) << 20));
}
constexpr int kIisptMaxJobs = 1024;  // tasks per launch (blockIdx.y); longer batches run in slices
// The traversal kernel of a slice runs max(tasks, ~6 blocks per CU) blocks and every block owns a column of the stack spill
// array, which is sized for 8 blocks per CU (max_traversal_threads): a slice never holds more tasks than that.
int iispt_slice_jobs(const iile_scene *sc) { return std::max(1, std::min(kIisptMaxJobs, sc->n_cus * 8)); }

// A slice of a batch laid out in the scratch block: per task its items (five float4 planes and the Halton indices, task after
// task), the job array the kernels read, one counter of items still on a specular chain.
struct IisptSlice {
    std::vector<IisptJob> jobs;
    std::vector<size_t> hemi_off, pix_off;  // per task: first hemi point / first film pixel of the slice's concatenated arrays
    size_t n_hemi = 0, n_pix = 0, n_items = 0;
    int max_items = 0, max_hemi = 0, max_pix = 0;
    float4 *planes = nullptr;  // in the scratch block (carve_slice)
    IisptJob *d_jobs = nullptr;
    uint32_t *n_active = nullptr;
};
int plan_slice(iile_scene *sc, const iile_iispt_task *tasks, int n_tasks, bool with_pixels, IisptSlice *sl) {
    sl->jobs.resize(size_t(n_tasks));
    sl->hemi_off.resize(size_t(n_tasks));
    sl->pix_off.resize(size_t(n_tasks));
    for (int k = 0; k < n_tasks; ++k) {
        int nx = 0, ny = 0;
        const int rc = iispt_check(sc, &tasks[k], &nx, &ny);
        if (rc) return rc;
        IisptJob &J = sl->jobs[size_t(k)];
        std::memset(&J, 0, sizeof(J));
        J.T = tasks[k];
        J.ny = ny;
        const size_t nh = size_t(nx) * ny, np = with_pixels ? size_t(tasks[k].x1 - tasks[k].x0) * size_t(tasks[k].y1 - tasks[k].y0) : 0;
        J.I.n_hemi = int(nh), J.I.n_items = int(nh + np), J.I.nx = nx;
        sl->hemi_off[size_t(k)] = sl->n_hemi, sl->pix_off[size_t(k)] = sl->n_pix;
        sl->n_hemi += nh, sl->n_pix += np, sl->n_items += nh + np;
        sl->max_items = std::max(sl->max_items, int(nh + np)), sl->max_hemi = std::max(sl->max_hemi, int(nh)), sl->max_pix = std::max(sl->max_pix, int(np));
    }
    if (sl->n_items >= 0x7fffffffull) return api_fail(IILE_ERR_UNSUPPORTED, "iile_iispt: more than 2^31 items in one slice of a batch");
    return IILE_OK;
}
// the slice's own ranges of a layout: the item planes, the indices behind 64 words of counters, the job array
void carve_slice(Carver &c, IisptSlice *sl) {
    sl->planes = c.take<float4>(5 * sl->n_items);
    sl->n_active = c.take<uint32_t>(sl->n_items + 64);
    sl->d_jobs = c.take<IisptJob>(sl->jobs.size());
}
// point every job at its part of the carved planes
void point_jobs(IisptSlice *sl) {
    float4 *planes = sl->planes;
    uint32_t *words = sl->n_active;
    size_t first = 0;
    for (IisptJob &J : sl->jobs) {
        const size_t n = sl->n_items;
        J.I.ro = planes + first, J.I.rd = planes + n + first, J.I.beta = planes + 2 * n + first, J.I.hit = planes + 3 * n + first, J.I.pf = planes + 4 * n + first;
        J.I.idx = words + 64 + first;
        J.I.n_active = words;
        first += size_t(J.I.n_items);
    }
}

int hemi_points_slice(iile_scene *sc, const iile_iispt_task *tasks, int n_tasks, uint8_t *valid, float *pos3, float *dir3, hipStream_t s) {
    IisptSlice sl;
    int rc = plan_slice(sc, tasks, n_tasks, false, &sl);
    if (rc) return rc;
    const size_t n = sl.n_hemi;
    uint8_t *dv = nullptr;
    float *dp = nullptr, *dd = nullptr;
    auto layout = [&](Carver c) {
        carve_slice(c, &sl);
        dv = c.take<uint8_t>(n);
        dp = c.take<float>(3 * n), dd = c.take<float>(3 * n);
        return c.used;
    };
    if ((rc = scratch_reserve(sc, layout(Carver()), s))) return rc;
    layout(Carver(sc->scratch.p));
    point_jobs(&sl);
    for (size_t k = 0; k < sl.jobs.size(); ++k)
        sl.jobs[k].valid = dv + sl.hemi_off[k], sl.jobs[k].pos3 = dp + 3 * sl.hemi_off[k], sl.jobs[k].dir3 = dd + 3 * sl.hemi_off[k];
    // (everything in the caller's stream's order: the copy follows whatever that stream did with the block last, the kernels follow it)
    HIP_TRY(hipMemcpyAsync(sl.d_jobs, sl.jobs.data(), sl.jobs.size() * sizeof(IisptJob), hipMemcpyHostToDevice, s));
    DScene S = sc->ds;
    S.diff_scale = 1.f;  // r.ScaleDifferentials(1.0), iisptrenderrunner.cpp:272
    LaunchCfg cfg{sc->n_cus, s, false};
    if ((rc = launch_iispt_first_hits(S, sl.d_jobs, n_tasks, sl.max_items, sl.n_active, sc->spill, cfg))) return rc;
    launch_iispt_hemi_out(S, sl.d_jobs, n_tasks, sl.max_hemi, cfg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(valid, dv, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(pos3, dp, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(dir3, dd, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the results are for the host, and `sl` dies with this call)
    return IILE_OK;
}

int gather_slice(iile_scene *sc, const iile_iispt_task *tasks, int n_tasks, const uint8_t *valid, const float *pos3, const float *dir3,
                 const float *nn_films, int32_t nn_on_device, float *out_rgbw, int32_t out_on_device, hipStream_t s) {
    IisptSlice sl;
    int rc = plan_slice(sc, tasks, n_tasks, true, &sl);
    if (rc) return rc;
    const size_t n = sl.n_hemi, n_pix = sl.n_pix;
    const int hemi = sc->probe.hemi_size;
    // the hemi points' cameras: CreateHemisphericCamera (hemispheric.cpp:109-160) — CameraToWorld from LookAt, WorldToCamera
    // its numerical inverse, the look direction and origin as given
    std::vector<DHemiCam> cams(n);
    for (size_t k = 0; k < n; ++k) {
        DHemiCam &hc = cams[k];
        std::memset(&hc, 0, sizeof(hc));
        if (!valid[k]) continue;
        DProbeCam pc;
        float inv[16];
        if (!make_probe_camera(pos3 + 3 * k, dir3 + 3 * k, &pc) || !invert4(pc.c2w.m, inv))
            return api_fail(IILE_ERR_ARG, "iile_iispt_gather: degenerate hemi point direction (hemi point " + std::to_string(k) + " of the slice)");
        hc.c2w = pc.c2w;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) hc.w2c[3 * r + c] = inv[4 * r + c];
        for (int c = 0; c < 3; ++c) hc.look[c] = dir3[3 * k + c], hc.origin[c] = pos3[3 * k + c];
        hc.valid = 1;
    }
    std::vector<float> jac(static_cast<size_t>(hemi), 0.f);  // IntensityFilm::get_camera_coord_jacobian, intensityfilm.cpp:60-66
    for (int y = 0; y < hemi; ++y) {
        const float abs_vertical_value = float(y) / hemi;
        const float polar_vertical_value = float(M_PI * abs_vertical_value);
        jac[size_t(y)] = std::sin(polar_vertical_value);  // sin(Float): the float overload (sinf), as in the reference
    }
    const size_t per_hemi = size_t(hemi) * hemi * 3, nn_floats = n * per_hemi;
    DHemiCam *dc = nullptr;
    float *dj = nullptr, *dnn = nullptr;
    float4 *out_dev = reinterpret_cast<float4 *>(out_rgbw);
    auto layout = [&](Carver c) {
        carve_slice(c, &sl);
        dc = c.take<DHemiCam>(n);
        dj = c.take<float>(jac.size());
        if (!nn_on_device) dnn = c.take<float>(nn_floats);
        if (!out_on_device) out_dev = c.take<float4>(n_pix);
        return c.used;
    };
    if ((rc = scratch_reserve(sc, layout(Carver()), s))) return rc;
    layout(Carver(sc->scratch.p));
    point_jobs(&sl);
    const float *nn_dev = nn_on_device ? nn_films : dnn;
    for (size_t k = 0; k < sl.jobs.size(); ++k)
        sl.jobs[k].cams = dc + sl.hemi_off[k], sl.jobs[k].nn_films = nn_dev + sl.hemi_off[k] * per_hemi, sl.jobs[k].out = out_dev + sl.pix_off[k];
    // (copies from these short-lived host vectors, in the caller's stream's order: they follow whatever that stream did with the block
    // last — and the network's kernels that wrote nn_films, when the caller queued them on the same stream)
    HIP_TRY(hipMemcpyAsync(sl.d_jobs, sl.jobs.data(), sl.jobs.size() * sizeof(IisptJob), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dc, cams.data(), n * sizeof(DHemiCam), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dj, jac.data(), jac.size() * sizeof(float), hipMemcpyHostToDevice, s));
    if (dnn) HIP_TRY(hipMemcpyAsync(dnn, nn_films, nn_floats * sizeof(float), hipMemcpyHostToDevice, s));
    DScene S = sc->ds;
    S.diff_scale = 1.f;
    LaunchCfg cfg{sc->n_cus, s, false};
    // (waits on the stream between its rounds, also where it fails: the vectors above are consumed)
    if ((rc = launch_iispt_first_hits(S, sl.d_jobs, n_tasks, sl.max_items, sl.n_active, sc->spill, cfg))) return rc;
    launch_iispt_gather(S, sl.d_jobs, n_tasks, sl.max_pix, dj, cfg);
    HIP_TRY(hipGetLastError());
    // Results on the device: the kernels are in the stream's order and the call returns (the caller's next use of the output, on that
    // stream or one that synchronises with it, follows them). Results for the host: the copy waits.
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(out_rgbw, out_dev, n_pix * sizeof(float4), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return IILE_OK;
}
}  // namespace

int iile_iispt_hemi_points_batch(iile_scene *sc, const iile_iispt_task *tasks, int32_t n_tasks, uint8_t *valid, float *pos3, float *dir3, void *stream) {
    if (!sc || !tasks || n_tasks < 1) return api_fail(IILE_ERR_ARG, "iile_iispt_hemi_points: no task");
    if (sc->camera_moves) return refuse_moving_camera("iile_iispt_hemi_points");
    if (!valid || !pos3 || !dir3) return api_fail(IILE_ERR_ARG, "iile_iispt_hemi_points: null output");
    size_t first = 0;
    const int slice = iispt_slice_jobs(sc);
    for (int k0 = 0; k0 < n_tasks; k0 += slice) {
        const int nk = std::min(slice, n_tasks - k0);
        const int rc = hemi_points_slice(sc, tasks + k0, nk, valid + first, pos3 + 3 * first, dir3 + 3 * first, static_cast<hipStream_t>(stream));
        if (rc) return rc;
        for (int k = k0; k < k0 + nk; ++k)
            first += size_t(iile_iispt_grid_count(tasks[k].x0, tasks[k].x1, tasks[k].tilesize)) * size_t(iile_iispt_grid_count(tasks[k].y0, tasks[k].y1, tasks[k].tilesize));
    }
    return IILE_OK;
}
int iile_iispt_hemi_points(iile_scene *sc, const iile_iispt_task *t, uint8_t *valid, float *pos3, float *dir3) {
    return iile_iispt_hemi_points_batch(sc, t, 1, valid, pos3, dir3, nullptr);
}

int iile_iispt_gather_batch(iile_scene *sc, const iile_iispt_task *tasks, int32_t n_tasks, const uint8_t *valid, const float *pos3, const float *dir3,
                            const float *nn_films, int32_t nn_on_device, float *out_rgbw, int32_t out_on_device, void *stream) {
    if (!sc || !tasks || n_tasks < 1) return api_fail(IILE_ERR_ARG, "iile_iispt_gather: no task");
    if (sc->camera_moves) return refuse_moving_camera("iile_iispt_gather");
    if (!valid || !pos3 || !dir3 || !nn_films || !out_rgbw) return api_fail(IILE_ERR_ARG, "iile_iispt_gather: null argument");
    const size_t per_hemi = size_t(sc->probe.hemi_size) * sc->probe.hemi_size * 3;
    size_t first_h = 0, first_p = 0;
    const int slice = iispt_slice_jobs(sc);
    for (int k0 = 0; k0 < n_tasks; k0 += slice) {
        const int nk = std::min(slice, n_tasks - k0);
        const int rc = gather_slice(sc, tasks + k0, nk, valid + first_h, pos3 + 3 * first_h, dir3 + 3 * first_h, nn_films + first_h * per_hemi, nn_on_device,
                                    out_rgbw + 4 * first_p, out_on_device, static_cast<hipStream_t>(stream));
        if (rc) return rc;
        for (int k = k0; k < k0 + nk; ++k) {
            first_h += size_t(iile_iispt_grid_count(tasks[k].x0, tasks[k].x1, tasks[k].tilesize)) * size_t(iile_iispt_grid_count(tasks[k].y0, tasks[k].y1, tasks[k].tilesize));
            first_p += size_t(tasks[k].x1 - tasks[k].x0) * size_t(tasks[k].y1 - tasks[k].y0);
        }
    }
    return IILE_OK;
}
int iile_iispt_film_add(iile_scene *sc, const iile_iispt_task *tasks, int32_t n_tasks, const float *out_rgbw_dev, double *film_rgbw_dev,
                        int32_t film_w, int32_t film_h, void *stream) {
    if (!sc || !tasks || n_tasks < 1 || !out_rgbw_dev || !film_rgbw_dev || film_w < 1 || film_h < 1)
        return api_fail(IILE_ERR_ARG, "iile_iispt_film_add: bad argument");
    if (sc->camera_moves) return refuse_moving_camera("iile_iispt_film_add");
    if (n_tasks > 65535) return api_fail(IILE_ERR_UNSUPPORTED, "iile_iispt_film_add: more than 65535 tasks in one call");
    std::vector<int4> rects(static_cast<size_t>(n_tasks));
    std::vector<uint32_t> first(static_cast<size_t>(n_tasks));
    uint64_t at = 0;
    int max_pixels = 1;
    for (int k = 0; k < n_tasks; ++k) {
        const iile_iispt_task &t = tasks[k];
        if (t.x0 < 0 || t.y0 < 0 || t.x1 > film_w || t.y1 > film_h || t.x1 <= t.x0 || t.y1 <= t.y0)
            return api_fail(IILE_ERR_ARG, "iile_iispt_film_add: a task lies outside the film");
        rects[size_t(k)] = make_int4(t.x0, t.y0, t.x1, t.y1);
        first[size_t(k)] = uint32_t(at);
        const uint64_t n = uint64_t(t.x1 - t.x0) * uint64_t(t.y1 - t.y0);
        at += n;
        max_pixels = std::max<int>(max_pixels, int(std::min<uint64_t>(n, 1u << 30)));
    }
    if (at >= 0xffffffffull) return api_fail(IILE_ERR_UNSUPPORTED, "iile_iispt_film_add: more than 2^32 pixels in one call");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int4 *d_rects = nullptr;
    uint32_t *d_first = nullptr;
    auto layout = [&](Carver c) {
        d_rects = c.take<int4>(size_t(n_tasks));
        d_first = c.take<uint32_t>(size_t(n_tasks));
        return c.used;
    };
    const size_t bytes = layout(Carver());
    if (!sc->film_add_block.holds(bytes)) {   // a table of its own (the scene's shared scratch may still be read by the gather's kernels)
        HIP_TRY(hipStreamSynchronize(s));
        if (const int rc = sc->film_add_block.reserve(bytes, 2 * bytes)) return rc;
    }
    layout(Carver(sc->film_add_block.p));
    HIP_TRY(hipMemcpyAsync(d_rects, rects.data(), rects.size() * sizeof(int4), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_first, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the vectors die with this call; the kernels before have to finish anyway)
    launch_iispt_film_add(d_rects, d_first, n_tasks, max_pixels, reinterpret_cast<const float4 *>(out_rgbw_dev), film_rgbw_dev, film_w, s);
    HIP_TRY(hipGetLastError());
    return IILE_OK;
}

int iile_iispt_film_merge(const double *direct_rgbw_dev, const double *indirect_rgbw_dev, int64_t n_pixels, float *rgb_dev, void *stream) {
    if (!direct_rgbw_dev || !indirect_rgbw_dev || !rgb_dev || n_pixels < 0) return api_fail(IILE_ERR_ARG, "iile_iispt_film_merge: bad argument");
    int rc = ensure_device();
    if (rc) return rc;
    if (n_pixels == 0) return IILE_OK;
    launch_iispt_film_merge(direct_rgbw_dev, indirect_rgbw_dev, rgb_dev, (long long)n_pixels, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return IILE_OK;
}

int iile_iispt_gather(iile_scene *sc, const iile_iispt_task *t, const uint8_t *valid, const float *pos3, const float *dir3, const float *nn_films,
                      int32_t nn_on_device, float *out_rgbw, int32_t out_on_device) {
    return iile_iispt_gather_batch(sc, t, 1, valid, pos3, dir3, nn_films, nn_on_device, out_rgbw, out_on_device, nullptr);
}

}  // extern "C"
