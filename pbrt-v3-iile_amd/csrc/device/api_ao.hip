// api_ao.hip — the ambient occlusion integrator's part of the C ABI (include/iile_gpu.h): the occlusion-ray block, run_pass_ao (the
// schedule of kernels_ao.hip around the path integrator's k_generate / k_extend), iile_render_ao (render_frame of api_render.hip
// with that pass), and the probes iile_ao_array_samples / iile_ao_li_samples.
#include <cmath>
#include <cstring>

#include "api_common.h"

using namespace iile;

namespace {

constexpr int kMaxAoSamples = 1 << 20;
constexpr uint64_t kMaxAoRays = uint64_t(1) << 31;   // rays of one pass: ray numbers and the feed's cursor are 32-bit words
// per occlusion ray: origin and direction records, the term, the visibility byte
constexpr double kAoBytesPerRay = 2 * sizeof(float4) + sizeof(float) + 1;

// What can be said of the arguments without looking into the scene (so: before the device check)
int check_ao_params(const iile_ao_params *ao, const char *who) {
    if (ao->n_samples < 1) return api_fail(IILE_ERR_ARG, std::string(who) + ": n_samples < 1");
    if (ao->n_samples > kMaxAoSamples) return api_fail(IILE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^20 occlusion samples per camera sample");
    return IILE_OK;
}
// The 2D array takes dimensions 5 and 6 of the samples 0 .. k_end * n_samples - 1 of a pixel: the sampler's tables must cover them
// and the indices must stay 32-bit words, as iile_scene_create checks for the pixel samples themselves
int check_ao_sampler(const iile_scene *sc, int n_samples, int64_t k_end, const char *who) {
    const DScene &S = sc->ds;
    if ((S.sobol ? S.sobol_dims : S.n_hdims) < 7) return api_fail(IILE_ERR_ARG, std::string(who) + ": the sampler's tables cover fewer than 7 dimensions");
    const double n_array = double(k_end) * double(n_samples);
    if (S.sobol) {
        if (n_array * std::ldexp(1.0, 2 * S.sobol_log2res) > 4294967296.0)
            return api_fail(IILE_ERR_UNSUPPORTED, std::string(who) + ": iile_sobol: sample indices beyond 32 bits (pixelsamples x nsamples too large)");
    } else if ((n_array + 1) * double(S.sample_stride) >= 4294967296.0) {
        return api_fail(IILE_ERR_UNSUPPORTED, std::string(who) + ": Halton index exceeds 32 bits (pixelsamples x nsamples too large)");
    }
    return IILE_OK;
}

int ensure_ao(iile_scene *sc, uint32_t n_paths, AoBuffers *A) {
    const size_t max_rays = size_t(n_paths) * size_t(A->n_samples);
    auto layout = [&](Carver c) {
        A->ray_o = c.take<float4>(max_rays);
        A->ray_d = c.take<float4>(max_rays);
        A->term = c.take<float>(max_rays);
        A->vis = c.take<uint8_t>(max_rays);
        A->hit_pid = c.take<uint32_t>(n_paths);
        return c.used;
    };
    if (const int rc = sc->ao_block.reserve(layout(Carver()), 0, "out of device memory for the occlusion rays of an ambient occlusion pass")) return rc;
    layout(Carver(sc->ao_block.p));
    return IILE_OK;
}

// Enqueue one pass of AOIntegrator::Li on cfg.stream: camera rays and their closest hits as the path integrator's bounce 0 (no ray
// is made inside k_extend: ao_rays reads the camera ray back from queue 0), then the three kernels of kernels_ao.hip.
int run_pass_ao(iile_scene *sc, const DScene &S_in, const PassDesc &P_in, const LaunchCfg &cfg, const AoBuffers &A) {
    PassBuffers &B = sc->pb;
    PassDesc P = P_in;
    P.gen_fused = 0;
    P.skip_last_bounce = 0;
    DScene S = S_in;
    clear_sample_table(&S);   // (a path-integrator scene rendered here may carry one; the array's samples lie outside it anyway)
    HIP_TRY(hipMemsetAsync(B.counts, 0, kCntWords * sizeof(uint32_t), cfg.stream));
    launch_generate(S, P, B, cfg);
    launch_extend(S, P, B, 0, B.queue_cap, cfg);
    launch_ao_rays(S, P, B, A, cfg);
    launch_ao_occlude(S, B, A, uint32_t(std::min<uint64_t>(uint64_t(P.n_paths) * uint64_t(A.n_samples), kMaxAoRays)), cfg);
    launch_ao_fold(P, B, A, cfg);
    HIP_TRY(hipGetLastError());
    return IILE_OK;
}

}  // namespace

extern "C" {

int iile_render_ao(iile_scene *sc, const iile_ao_params *ao, const iile_render_params *prm, float *film_xyzw, iile_stats *stats) {
    if (!sc || !ao || !prm || !film_xyzw) return api_fail(IILE_ERR_ARG, "iile_render_ao: null argument");
    int rc = check_ao_params(ao, "iile_render_ao");
    if (rc) return rc;
    rc = ensure_device();
    if (rc) return rc;
    rc = check_ao_sampler(sc, ao->n_samples, prm->k_end > 0 ? prm->k_end : sc->spp, "iile_render_ao");
    if (rc) return rc;
    AoBuffers A = {};
    A.n_samples = ao->n_samples;
    A.cos_sample = ao->cos_sample != 0;
    // a pass is sized so that its paths x nSamples rays fit the workspace budget beside the path workspace (~410 B per path)
    const FrameIntegrator fi = {410.0 + 4.0 + kAoBytesPerRay * double(ao->n_samples), kMaxAoRays / uint64_t(ao->n_samples),
                                "the occlusion rays of one 16 x 16 tile exceed 2^31: split the sample range",
                                [](iile_scene *s, uint32_t n_paths, void *ctx) { return ensure_ao(s, n_paths, static_cast<AoBuffers *>(ctx)); },
                                [](iile_scene *s, const DScene &S, const PassDesc &P, const LaunchCfg &cfg, bool, bool, void *ctx) {
                                    return run_pass_ao(s, S, P, cfg, *static_cast<const AoBuffers *>(ctx));
                                },
                                &A};
    return render_frame(sc, prm, film_xyzw, stats, fi);
}

int iile_ao_array_samples(iile_scene *sc, int32_t n_samples, int32_t n, const int32_t *px, const int32_t *py, const int32_t *k, const int32_t *j,
                          float *out2) {
    if (!sc || n < 0 || !px || !py || !k || !j || !out2) return api_fail(IILE_ERR_ARG, "iile_ao_array_samples: bad argument");
    const iile_ao_params ao = {n_samples, 1};
    int rc = check_ao_params(&ao, "iile_ao_array_samples");
    if (rc) return rc;
    int64_t k_end = 0;
    for (int i = 0; i < n; ++i) {
        if (k[i] < 0 || j[i] < 0 || j[i] >= n_samples) return api_fail(IILE_ERR_ARG, "iile_ao_array_samples: k < 0, or j outside [0, n_samples)");
        k_end = std::max<int64_t>(k_end, int64_t(k[i]) + 1);
    }
    rc = ensure_device();
    if (rc) return rc;
    rc = check_ao_sampler(sc, n_samples, k_end, "iile_ao_array_samples");
    if (rc) return rc;
    DevBuf<int> dx, dy, dk, dj;
    DevBuf<float> dout;
    if ((rc = dx.put(px, n)) || (rc = dy.put(py, n)) || (rc = dk.put(k, n)) || (rc = dj.put(j, n)) || (rc = dout.alloc(2 * size_t(n)))) return rc;
    if (n) launch_ao_array_probe(sc->ds, n_samples, n, dx.p, dy.p, dk.p, dj.p, dout.p, LaunchCfg{sc->n_cus, nullptr, false});
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return dout.get(out2, 2 * size_t(n));
}

int iile_ao_li_samples(iile_scene *sc, const iile_ao_params *ao, int32_t n, const int32_t *px, const int32_t *py, const int32_t *k, float *L1,
                       int32_t *nrays2) {
    if (!sc || !ao || n <= 0 || !px || !py || !k || !L1) return api_fail(IILE_ERR_ARG, "iile_ao_li_samples: bad argument");
    int rc = check_ao_params(ao, "iile_ao_li_samples");
    if (rc) return rc;
    if (uint64_t(n) * uint64_t(ao->n_samples) > kMaxAoRays) return api_fail(IILE_ERR_UNSUPPORTED, "iile_ao_li_samples: more than 2^31 occlusion rays in one call");
    int64_t k_end = 0;
    for (int i = 0; i < n; ++i) {
        if (k[i] < 0) return api_fail(IILE_ERR_ARG, "iile_ao_li_samples: k < 0");
        k_end = std::max<int64_t>(k_end, int64_t(k[i]) + 1);
    }
    rc = ensure_device();
    if (rc) return rc;
    rc = check_ao_sampler(sc, ao->n_samples, k_end, "iile_ao_li_samples");
    if (rc) return rc;
    DevBuf<int> dx, dy, dk;
    DevBuf<uint32_t> dn;
    if ((rc = dx.put(px, n)) || (rc = dy.put(py, n)) || (rc = dk.put(k, n)) || (rc = dn.alloc(2 * size_t(n)))) return rc;
    rc = ensure_workspace(sc, uint32_t(n));
    if (rc) return rc;
    AoBuffers A = {};
    A.n_samples = ao->n_samples;
    A.cos_sample = ao->cos_sample != 0;
    rc = ensure_ao(sc, uint32_t(n), &A);
    if (rc) return rc;
    PassDesc P;
    std::memset(&P, 0, sizeof(P));
    P.n_tiles_x = P.n_tiles_y = 1;
    P.tile_nranks = 1;
    P.kc = 1;
    P.n_paths = uint32_t(n);
    P.list_px = dx.p, P.list_py = dy.p, P.list_k = dk.p;
    LaunchCfg cfg{sc->n_cus, nullptr, true};
    cfg.camera_moves = sc->camera_moves;
    HIP_TRY(hipMemset(sc->pb.counters, 0, sizeof(DCounters)));
    sc->pb.nray_out = dn.p;
    sc->pb.flag_count = nullptr;
    rc = run_pass_ao(sc, sc->ds, P, cfg, A);
    sc->pb.nray_out = nullptr;
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float4> L(n);
    HIP_TRY(hipMemcpy(L.data(), sc->pb.L, size_t(n) * sizeof(float4), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        // guards of SamplerIntegrator::Render (integrator.cpp:293-314); L is the same in every channel, y = (the weights' sum) * L
        const float r = L[i].x, g = L[i].y, b = L[i].z;
        const float y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
        L1[i] = (std::isnan(r) || y < -1e-5 || std::isinf(y)) ? 0.f : r;
    }
    if (nrays2) {
        std::vector<uint32_t> nr(2 * size_t(n));
        if ((rc = dn.get(nr.data(), nr.size()))) return rc;
        for (size_t i = 0; i < nr.size(); ++i) nrays2[i] = int32_t(nr[i]);
    }
    return IILE_OK;
}

}  // extern "C"
