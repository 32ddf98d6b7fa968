// api_probes.hip — the kernel-level entry points of the C ABI (include/iile_gpu.h): single kernels and device functions
// run on arrays of the caller's, for the parity tests. All of them work on the null stream (iile_light_choose: on the caller's) and return with the device
// drained.
#include <cstring>

#include "api_common.h"

using namespace iile;

namespace {
LaunchCfg probe_cfg(const iile_scene *sc, bool count_stats = false) {
    LaunchCfg cfg{sc->n_cus, nullptr, count_stats};
    cfg.camera_moves = sc->camera_moves;
    return cfg;
}
// The tail of every entry point here: the launch's error, the device drained, the (first) result downloaded.
template <typename T>
int finish(DevBuf<T> &dev, T *host, size_t n) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return dev.get(host, n);
}

int trace_common(iile_scene *sc, int32_t n, const float *o3, const float *d3, const float *tmax, int any,
                 std::vector<float4> *hits, iile_stats *stats) {
    if (!sc || n < 0 || !o3 || !d3 || !tmax) return api_fail(IILE_ERR_ARG, "iile_trace: bad argument");
    int rc = ensure_device();
    if (rc) return rc;
    std::vector<float4> ro(n), rd(n);
    for (int i = 0; i < n; ++i) {
        ro[i] = make_float4(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2], 0);
        rd[i] = make_float4(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2], tmax[i]);
    }
    DevBuf<float4> dro, drd, dh;
    DevBuf<DCounters> dc;
    if ((rc = dro.put(ro.data(), size_t(n))) || (rc = drd.put(rd.data(), size_t(n))) || (rc = dh.alloc(2 * size_t(n))) || (rc = dc.alloc(1))) return rc;
    HIP_TRY(hipMemset(dc.p, 0, sizeof(DCounters)));
    if (n) launch_trace(sc->ds, n, dro.p, drd.p, dh.p, any, dc.p, sc->spill, probe_cfg(sc, stats != nullptr));
    hits->resize(2 * size_t(n));
    if ((rc = finish(dh, hits->data(), hits->size()))) return rc;
    if (stats) {
        DCounters c;
        if ((rc = dc.get(&c, 1))) return rc;
        std::memset(stats, 0, sizeof(*stats));
        copy_counters(c, stats);
    }
    return IILE_OK;
}

int bsdf_probe(iile_scene *sc, int32_t n, int32_t mat, const float *wo3, const float *in, size_t in_stride,
               int sample, float *out, size_t out_stride, const float *ng3 = nullptr) {
    if (!sc || n < 0 || !wo3 || !in || !out || mat < 0 || mat >= sc->ds.n_materials)
        return api_fail(IILE_ERR_ARG, "iile_bsdf: bad argument");
    const float up[3] = {0.f, 0.f, 1.f};
    if (!ng3) ng3 = up;
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> dwo, din, dout;
    if ((rc = dwo.put(wo3, 3 * size_t(n))) || (rc = din.put(in, in_stride * size_t(n))) ||
        (rc = dout.alloc(out_stride * size_t(n))))
        return rc;
    if (n) launch_bsdf_probe(sc->ds, n, mat, dwo.p, din.p, sample, dout.p, ng3, probe_cfg(sc));
    return finish(dout, out, out_stride * size_t(n));
}
}  // namespace

extern "C" {

int iile_trace_closest(iile_scene *sc, int32_t n, const float *o3, const float *d3, const float *tmax, int32_t *prim,
                       float *tb, iile_stats *stats) {
    if (!prim || !tb) return api_fail(IILE_ERR_ARG, "iile_trace_closest: null output");
    std::vector<float4> hits;
    int rc = trace_common(sc, n, o3, d3, tmax, 0, &hits, stats);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        uint32_t u;
        std::memcpy(&u, &hits[2 * i].x, 4);
        prim[i] = int32_t(u);
        tb[4 * i] = hits[2 * i].y;
        tb[4 * i + 1] = hits[2 * i + 1].x;
        tb[4 * i + 2] = hits[2 * i + 1].y;
        tb[4 * i + 3] = hits[2 * i + 1].z;
    }
    return IILE_OK;
}

int iile_trace_any(iile_scene *sc, int32_t n, const float *o3, const float *d3, const float *tmax, int32_t *hit,
                   iile_stats *stats) {
    if (!hit) return api_fail(IILE_ERR_ARG, "iile_trace_any: null output");
    std::vector<float4> hits;
    int rc = trace_common(sc, n, o3, d3, tmax, 1, &hits, stats);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        uint32_t u;
        std::memcpy(&u, &hits[2 * i].x, 4);
        hit[i] = int32_t(u);
    }
    return IILE_OK;
}

int iile_halton_samples(iile_scene *sc, int32_t n, const int32_t *px, const int32_t *py, const int32_t *k,
                        int32_t dim0, int32_t ndims, float *out, uint32_t *index_out) {
    if (!sc || n < 0 || !px || !py || !k || !out || ndims <= 0 || dim0 < 0 || dim0 + ndims > (sc->ds.sobol ? sc->ds.sobol_dims : sc->ds.n_hdims))
        return api_fail(IILE_ERR_ARG, "iile_halton_samples: bad argument");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<int> dx, dy, dk;
    DevBuf<float> dout;
    DevBuf<uint32_t> dindex;
    if ((rc = dx.put(px, n)) || (rc = dy.put(py, n)) || (rc = dk.put(k, n)) || (rc = dout.alloc(size_t(n) * ndims)) ||
        (rc = dindex.alloc(n)))
        return rc;
    if (n) launch_halton(sc->ds, n, dx.p, dy.p, dk.p, dim0, ndims, dout.p, dindex.p, probe_cfg(sc));
    if ((rc = finish(dout, out, size_t(n) * ndims))) return rc;
    if (index_out && (rc = dindex.get(index_out, n))) return rc;
    return IILE_OK;
}

int iile_sample_table_records(iile_scene *sc, int32_t n, const int32_t *px, const int32_t *py, const int32_t *k, const int32_t *bounce,
                              float *out8) {
    if (!sc || n < 0 || !px || !py || !k || !bounce || !out8) return api_fail(IILE_ERR_ARG, "iile_sample_table_records: bad argument");
    if (!sc->ds.stab_shade) return api_fail(IILE_ERR_ARG, "iile_sample_table_records: the scene has no sample table");
    for (int i = 0; i < n; ++i)
        if (k[i] < 0 || uint32_t(k[i]) >= sc->ds.stab_spp || bounce[i] >= sc->ds.max_depth)
            return api_fail(IILE_ERR_ARG, "iile_sample_table_records: sample or bounce outside the table");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<int> dx, dy, dk, db;
    DevBuf<float> dout;
    if ((rc = dx.put(px, n)) || (rc = dy.put(py, n)) || (rc = dk.put(k, n)) || (rc = db.put(bounce, n)) || (rc = dout.alloc(size_t(n) * 8))) return rc;
    if (n) launch_sample_table_read(sc->ds, n, dx.p, dy.p, dk.p, db.p, dout.p, probe_cfg(sc));
    return finish(dout, out8, size_t(n) * 8);
}
uint64_t iile_sample_table_budget(void) { return sample_table_budget(); }
void iile_test_sample_table_budget(uint64_t bytes) { set_sample_table_budget(bytes); }
uint64_t iile_sample_table_bytes(const iile_scene *sc) { return sc ? sc->sample_table_bytes : 0; }

int iile_camera_rays(iile_scene *sc, int32_t n, const float *pfilm2, const float *plens2, float *o3, float *d3) {
    if (!sc || n < 0 || !pfilm2 || !o3 || !d3) return api_fail(IILE_ERR_ARG, "iile_camera_rays: bad argument");
    return iile_camera_rays_at(sc, n, pfilm2, plens2, 0.f, o3, d3);
}
int iile_camera_rays_at(iile_scene *sc, int32_t n, const float *pfilm2, const float *plens2, float time, float *o3, float *d3) {
    if (!sc || n < 0 || !pfilm2 || !o3 || !d3) return api_fail(IILE_ERR_ARG, "iile_camera_rays_at: bad argument");
    if (!(time == time)) return api_fail(IILE_ERR_ARG, "iile_camera_rays_at: the time is not a number");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> df, dl, dox, ddx;
    if ((rc = df.put(pfilm2, 2 * size_t(n))) || (rc = dox.alloc(3 * size_t(n))) || (rc = ddx.alloc(3 * size_t(n))))
        return rc;
    if (plens2 && (rc = dl.put(plens2, 2 * size_t(n)))) return rc;
    if (n) launch_camera(sc->ds, n, df.p, plens2 ? dl.p : nullptr, time, dox.p, ddx.p, probe_cfg(sc));
    if ((rc = finish(dox, o3, 3 * size_t(n))) || (rc = ddx.get(d3, 3 * size_t(n)))) return rc;
    return IILE_OK;
}

int iile_bsdf_eval(iile_scene *sc, int32_t n, int32_t mat, const float *wo3, const float *wi3, float *out4) {
    return bsdf_probe(sc, n, mat, wo3, wi3, 3, 0, out4, 4);
}
int iile_bsdf_sample(iile_scene *sc, int32_t n, int32_t mat, const float *wo3, const float *u2, float *out7) {
    return bsdf_probe(sc, n, mat, wo3, u2, 2, 1, out7, 7);
}
int iile_bsdf_eval_ng(iile_scene *sc, int32_t n, int32_t mat, const float *ng3, const float *wo3, const float *wi3, float *out4) {
    if (!ng3) return api_fail(IILE_ERR_ARG, "iile_bsdf_eval_ng: null normal");
    return bsdf_probe(sc, n, mat, wo3, wi3, 3, 0, out4, 4, ng3);
}
int iile_bsdf_sample_ng(iile_scene *sc, int32_t n, int32_t mat, const float *ng3, const float *wo3, const float *u2, float *out7) {
    if (!ng3) return api_fail(IILE_ERR_ARG, "iile_bsdf_sample_ng: null normal");
    return bsdf_probe(sc, n, mat, wo3, u2, 2, 1, out7, 7, ng3);
}

int iile_bsdf_sample_specular(iile_scene *sc, int32_t n, int32_t mat, const float *wo3, const float *u2, float *out9) {
    return bsdf_probe(sc, n, mat, wo3, u2, 2, 2, out9, 9);
}

int iile_light_sample_li(iile_scene *sc, int32_t light, int32_t n, const float *p3, float *out7) {
    if (!sc || n < 0 || !p3 || !out7 || light < 0 || light >= sc->ds.n_lights)
        return api_fail(IILE_ERR_ARG, "iile_light_sample_li: bad argument");
    if (!iile_light_is_delta(sc->light_types[size_t(light)])) return api_fail(IILE_ERR_ARG, "iile_light_sample_li: not a delta light");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> dp, dout;
    if ((rc = dp.put(p3, 3 * size_t(n))) || (rc = dout.alloc(7 * size_t(n)))) return rc;
    if (n) launch_light_probe(sc->ds, n, light, dp.p, dout.p, probe_cfg(sc));
    return finish(dout, out7, 7 * size_t(n));
}

// the lights iile_light_sample_at and iile_light_pdf_at take: the sampled ones
static bool light_is_sampled(int type) {
    return type == IILE_LIGHT_DIFFUSE_AREA || type == IILE_LIGHT_AREA_TRIANGLE || type == IILE_LIGHT_AREA_QUADRIC || type == IILE_LIGHT_INFINITE;
}

int iile_light_sample_at(iile_scene *sc, int32_t light, int32_t n, const float *ref_p3, const float *ref_n3, const float *u2, float *out13) {
    if (!sc || n < 0 || !ref_p3 || !ref_n3 || !u2 || !out13 || light < 0 || light >= sc->ds.n_lights)
        return api_fail(IILE_ERR_ARG, "iile_light_sample_at: bad argument");
    if (!light_is_sampled(sc->light_types[size_t(light)])) return api_fail(IILE_ERR_ARG, "iile_light_sample_at: not an area or infinite light");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> dp, dn, du, dout;
    if ((rc = dp.put(ref_p3, 3 * size_t(n))) || (rc = dn.put(ref_n3, 3 * size_t(n))) || (rc = du.put(u2, 2 * size_t(n))) ||
        (rc = dout.alloc(13 * size_t(n))))
        return rc;
    if (n) launch_light_sample_probe(sc->ds, n, light, dp.p, dn.p, du.p, dout.p, probe_cfg(sc));
    return finish(dout, out13, 13 * size_t(n));
}

int iile_light_pdf_at(iile_scene *sc, int32_t light, int32_t n, const float *ref_p3, const float *ref_n3, const float *wi3, float *out_pdf) {
    if (!sc || n < 0 || !ref_p3 || !ref_n3 || !wi3 || !out_pdf || light < 0 || light >= sc->ds.n_lights)
        return api_fail(IILE_ERR_ARG, "iile_light_pdf_at: bad argument");
    if (!light_is_sampled(sc->light_types[size_t(light)])) return api_fail(IILE_ERR_ARG, "iile_light_pdf_at: not an area or infinite light");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> dp, dn, dw, dout;
    if ((rc = dp.put(ref_p3, 3 * size_t(n))) || (rc = dn.put(ref_n3, 3 * size_t(n))) || (rc = dw.put(wi3, 3 * size_t(n))) ||
        (rc = dout.alloc(size_t(n))))
        return rc;
    if (n) launch_light_pdf_probe(sc->ds, n, light, dp.p, dn.p, dw.p, dout.p, probe_cfg(sc));
    return finish(dout, out_pdf, size_t(n));
}

int iile_light_le(iile_scene *sc, int32_t light, int32_t n, const float *d3, float *out3) {
    if (!sc || n < 0 || !d3 || !out3 || light < 0 || light >= sc->ds.n_lights) return api_fail(IILE_ERR_ARG, "iile_light_le: bad argument");
    if (sc->light_types[size_t(light)] != IILE_LIGHT_INFINITE) return api_fail(IILE_ERR_ARG, "iile_light_le: not an infinite light");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> dd, dout;
    if ((rc = dd.put(d3, 3 * size_t(n))) || (rc = dout.alloc(3 * size_t(n)))) return rc;
    if (n) launch_light_le_probe(sc->ds, n, light, dd.p, dout.p, probe_cfg(sc));
    return finish(dout, out3, 3 * size_t(n));
}

int iile_light_choose(iile_scene *sc, int32_t n, const float *p3, const float *u, int32_t *out_light, float *out_pdf, void *stream) {
    if (!sc || n < 0 || !p3 || !u || !out_light || !out_pdf) return api_fail(IILE_ERR_ARG, "iile_light_choose: bad argument");
    if (sc->ds.n_lights < 1) return api_fail(IILE_ERR_ARG, "iile_light_choose: the scene has no light");
    int rc = ensure_device();
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevBuf<float> dp, du, dpdf;
    DevBuf<int> dl;
    if ((rc = dp.alloc(3 * size_t(n))) || (rc = du.alloc(size_t(n))) || (rc = dl.alloc(size_t(n))) || (rc = dpdf.alloc(size_t(n)))) return rc;
    if (n == 0) return IILE_OK;
    HIP_TRY(hipMemcpyAsync(dp.p, p3, 3 * size_t(n) * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(du.p, u, size_t(n) * sizeof(float), hipMemcpyHostToDevice, s));
    LaunchCfg cfg = probe_cfg(sc);
    cfg.stream = s;
    launch_light_choose(sc->ds, n, dp.p, du.p, dl.p, dpdf.p, cfg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_light, dl.p, size_t(n) * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_pdf, dpdf.p, size_t(n) * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IILE_OK;
}

int iile_texture_eval(iile_scene *sc, int32_t tex, int32_t n, const float *uv2, const float *duv4, float *rgb3) {
    if (!sc || n < 0 || !uv2 || !duv4 || !rgb3 || tex < 0 || tex >= sc->ds.n_textures)
        return api_fail(IILE_ERR_ARG, "iile_texture_eval: bad argument");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> duv, dd, dout;
    if ((rc = duv.put(uv2, 2 * size_t(n))) || (rc = dd.put(duv4, 4 * size_t(n))) || (rc = dout.alloc(3 * size_t(n)))) return rc;
    if (n) launch_texture_probe(sc->ds, n, tex, duv.p, dd.p, nullptr, dout.p, probe_cfg(sc));
    return finish(dout, rgb3, 3 * size_t(n));
}

int iile_texture_eval_p(iile_scene *sc, int32_t tex, int32_t n, const float *uv2, const float *duv4, const float *pdp9, float *rgb3) {
    if (!sc || n < 0 || !uv2 || !duv4 || !pdp9 || !rgb3 || tex < 0 || tex >= sc->ds.n_textures)
        return api_fail(IILE_ERR_ARG, "iile_texture_eval_p: bad argument");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> duv, dd, dp, dout;
    if ((rc = duv.put(uv2, 2 * size_t(n))) || (rc = dd.put(duv4, 4 * size_t(n))) || (rc = dp.put(pdp9, 9 * size_t(n))) ||
        (rc = dout.alloc(3 * size_t(n))))
        return rc;
    if (n) launch_texture_probe(sc->ds, n, tex, duv.p, dd.p, dp.p, dout.p, probe_cfg(sc));
    return finish(dout, rgb3, 3 * size_t(n));
}

int iile_shape_hit_attributes(iile_scene *sc, int32_t n, const float *o3, const float *d3, const int32_t *prim, float *out) {
    if (!sc || n < 0 || !o3 || !d3 || !prim || !out) return api_fail(IILE_ERR_ARG, "iile_shape_hit_attributes: bad argument");
    for (int32_t i = 0; i < n; ++i)  // sphere and quadric primitives only: their flag word has bit 0 (api_scene.hip, the vertex records)
        if (prim[i] < 0 || prim[i] >= sc->ds.n_prims || !(sc->prim_is_shape[size_t(prim[i])]))
            return api_fail(IILE_ERR_ARG, "iile_shape_hit_attributes: a primitive is not a sphere or a quadric");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> dox, ddx, dout;
    DevBuf<int> dp;
    if ((rc = dox.put(o3, 3 * size_t(n))) || (rc = ddx.put(d3, 3 * size_t(n))) || (rc = dp.put(prim, size_t(n))) ||
        (rc = dout.alloc(size_t(kShapeHitFloats) * size_t(n))))
        return rc;
    if (n) launch_shape_hit_probe(sc->ds, n, dox.p, ddx.p, dp.p, dout.p, probe_cfg(sc));
    return finish(dout, out, size_t(kShapeHitFloats) * size_t(n));
}

int iile_trig_probe(int32_t n, const float *x, float *out3) {
    if (n < 0 || !x || !out3) return api_fail(IILE_ERR_ARG, "iile_trig_probe: bad argument");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<float> dx, dout;
    if ((rc = dx.put(x, n)) || (rc = dout.alloc(3 * size_t(n)))) return rc;
    if (n) launch_trig_probe(n, dx.p, dout.p, LaunchCfg{256, nullptr, false});
    return finish(dout, out3, 3 * size_t(n));
}

}  // extern "C"
