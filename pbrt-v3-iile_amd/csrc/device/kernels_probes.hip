// kernels_probes.hip — kernel-level probes for the parity tests, each with its launcher: one device function of the path for n
// independent inputs. (The probes of the traversal, the sample table and the AO arrays live beside the kernels they test.)
#include "kcommon.h"

namespace iile {

DEV void put3(float *out, F3 v) { out[0] = v.x, out[1] = v.y, out[2] = v.z; }

__global__ void k_halton(DScene S, int n, const int *px, const int *py, const int *k, int dim0, int ndims, float *out,
                         uint32_t *index_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t idx = sample_index(S, px[i], py[i], uint32_t(k[i]));
    if (index_out) index_out[i] = idx;
    for (int d = 0; d < ndims; ++d) out[size_t(i) * ndims + d] = sample_dimension(S, idx, dim0 + d, px[i], py[i]);
}
void launch_halton(const DScene &S, int n, const int *px, const int *py, const int *k, int dim0, int ndims,
                   float *out, uint32_t *index_out, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_halton, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, px, py, k, dim0, ndims, out,
                       index_out);
}
__global__ void k_camera(DScene S, int n, const float *pfilm, const float *plens, float *o, float *d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 ro, rd;
    float tm;
    camera_ray(S, pfilm[2 * i], pfilm[2 * i + 1], plens ? plens[2 * i] : 0.f, plens ? plens[2 * i + 1] : 0.f, &ro, &rd,
               &tm);
    put3(o + 3 * i, ro);
    put3(d + 3 * i, rd);
}
// the same for a moving camera (camera_motion, dscene.h) at ray time `time` (not a time sample: the shutter does not enter)
__global__ void k_camera_at(DScene S, int n, const float *pfilm, const float *plens, float time, float *o, float *d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 ro, rd;
    float tm;
    camera_ray<true, true>(S, pfilm[2 * i], pfilm[2 * i + 1], plens ? plens[2 * i] : 0.f, plens ? plens[2 * i + 1] : 0.f, &ro, &rd, &tm, 0.f, time);
    put3(o + 3 * i, ro);
    put3(d + 3 * i, rd);
}
void launch_camera(const DScene &S, int n, const float *pfilm, const float *plens, float time, float *o, float *d,
                   const LaunchCfg &cfg) {
    if (cfg.camera_moves)
        hipLaunchKernelGGL(k_camera_at, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, pfilm, plens, time, o, d);
    else
        hipLaunchKernelGGL(k_camera, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, pfilm, plens, o, d);
}
// BSDF in a canonical frame (ns = +z, ss = +x; the geometric normal ng, +z unless a test tilts it). sample == 0: out = {f.xyz, pdf}
// for (wo, wi); sample == 1: out = {wi.xyz, f.xyz, pdf} for (wo, u); sample == 2: the same sample with the specular lobes allowed
// (BSDF_ALL), out = {wi.xyz, f.xyz, pdf, sampled_specular, sampled_transmission}, the two flags as 0 or 1.
// DIS: the scene's Disney build (DScene::disney_build).
template <bool DIS>
__global__ void k_bsdf_probe(DScene S, int n, int mat, const float *wo, const float *wi_or_u, int sample, float *out, float ngx,
                             float ngy, float ngz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Isect is;
    is.sn = F3{0, 0, 1};
    is.n = F3{ngx, ngy, ngz};
    is.sdpdu = F3{1, 0, 0};
    is.p = is.perr = is.wo = F3{0, 0, 0};
    auto b = make_bsdf_at<true, DIS>(S, mat, S.materials[mat], is);
    b.ss = F3{1, 0, 0};
    b.ts = cross(b.ns, b.ss);
    const F3 w = F3{wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]};
    if (!sample) {
        const F3 wi = F3{wi_or_u[3 * i], wi_or_u[3 * i + 1], wi_or_u[3 * i + 2]};
        const F3 f = bsdf_f(b, w, wi);
        put3(out + 4 * i, f);
        out[4 * i + 3] = bsdf_pdf(b, w, wi);
    } else if (sample == 2) {
        F3 wi = F3{0, 0, 0};
        float pdf = 0;
        bool spec = false, trans = false;
        const F3 f = bsdf_sample_f(b, w, &wi, wi_or_u[2 * i], wi_or_u[2 * i + 1], &pdf, true, &spec, &trans);
        put3(out + 9 * i, wi);
        put3(out + 9 * i + 3, f);
        out[9 * i + 6] = pdf;
        out[9 * i + 7] = spec ? 1.f : 0.f;
        out[9 * i + 8] = trans ? 1.f : 0.f;
    } else {
        F3 wi = F3{0, 0, 0};
        float pdf = 0;
        const F3 f = bsdf_sample_f(b, w, &wi, wi_or_u[2 * i], wi_or_u[2 * i + 1], &pdf);
        put3(out + 7 * i, wi);
        put3(out + 7 * i + 3, f);
        out[7 * i + 6] = pdf;
    }
}
void launch_bsdf_probe(const DScene &S, int n, int mat, const float *wo, const float *wi_or_u, int sample,
                       float *out, const float ng[3], const LaunchCfg &cfg) {
    if (S.disney_build)
        hipLaunchKernelGGL(k_bsdf_probe<true>, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, mat, wo, wi_or_u, sample, out, ng[0], ng[1],
                           ng[2]);
    else
        hipLaunchKernelGGL(k_bsdf_probe<false>, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, mat, wo, wi_or_u, sample, out, ng[0], ng[1],
                           ng[2]);
}
__global__ void k_trig_probe(int n, const float *x, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s, c;
    sincos_f(x[i], &s, &c);
    out[3 * i] = s;
    out[3 * i + 1] = c;
    out[3 * i + 2] = acos_f(clampf(x[i], -1.f, 1.f));
}
void launch_trig_probe(int n, const float *x, float *out, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_trig_probe, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, n, x, out);
}
// Texture::Evaluate for given (u, v) and differentials and, if pdp is not null, p, dpdx and dpdy (9 floats per point; else
// zero) (test probe)
__global__ void k_texture_probe(DScene S, int n, int tex, const float *uv, const float *duv, const float *pdp, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    TexCtx c = TexCtx{uv[2 * i], uv[2 * i + 1], TexDiff{duv[4 * i], duv[4 * i + 1], duv[4 * i + 2], duv[4 * i + 3]}, F3{0, 0, 0},
                      F3{0, 0, 0}, F3{0, 0, 0}};
    if (pdp) {
        const float *q = pdp + 9 * size_t(i);
        c.p = F3{q[0], q[1], q[2]}, c.dpdx = F3{q[3], q[4], q[5]}, c.dpdy = F3{q[6], q[7], q[8]};
    }
    put3(out + 3 * i, tex_evaluate(S, tex, c));
}
void launch_texture_probe(const DScene &S, int n, int tex, const float *uv, const float *duv, const float *pdp, float *out,
                          const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_texture_probe, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, tex, uv, duv, pdp, out);
}
// The SurfaceInteraction of a sphere or quadric hit (shape_hit_interaction<DIFFS = true>) for ray i and the primitive its closest
// hit found (the caller checked that it is not a triangle): kShapeHitFloats floats per ray, see iile_shape_hit_attributes
__global__ void k_shape_hit_probe(DScene S, int n, const float *o, const float *d, const int *prim, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Isect is;
    shape_hit_interaction<true>(S, S.prim_shape[prim[i]], F3{o[3 * i], o[3 * i + 1], o[3 * i + 2]}, F3{d[3 * i], d[3 * i + 1], d[3 * i + 2]},
                                &is);
    const F3 v[8] = {is.p, is.n, is.sn, is.dpdu, is.dpdv, is.dndu, is.dndv, is.wo};
    float *r = out + size_t(kShapeHitFloats) * i;
    for (int k = 0; k < 8; ++k) r[3 * k] = v[k].x, r[3 * k + 1] = v[k].y, r[3 * k + 2] = v[k].z;
    r[24] = is.u;
    r[25] = is.v;
    r[26] = is.flip ? 1.f : 0.f;
    r[27] = 0.f;
}
void launch_shape_hit_probe(const DScene &S, int n, const float *o, const float *d, const int *prim, float *out, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_shape_hit_probe, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, o, d, prim, out);
}
// Light::Sample_Li of delta light `light` at point i (an Interaction without normal or error bounds): {wi, Li, pdf} (test probe;
// the caller checked that the light is a delta light, iile_scene_create that its map is a texture of the scene)
__global__ void k_light_probe(DScene S, int n, int light, const float *p, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F3 wi, target;
    const F3 Li = delta_light_li(S, S.lights[light], F3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}, &wi, &target);
    float *r = out + 7 * size_t(i);
    r[0] = wi.x, r[1] = wi.y, r[2] = wi.z;
    r[3] = Li.x, r[4] = Li.y, r[5] = Li.z;
    r[6] = 1.f;
}
void launch_light_probe(const DScene &S, int n, int light, const float *p, float *out, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_light_probe, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, light, p, out);
}
// Light::Sample_Li of area light (sphere, triangle, quadric) or infinite light `light` for reference point i, an Interaction with
// normal ref_n (zero: a point without a surface) and no error bounds, and the 2D sample u: {wi, Li, pdf, p_light, n_light} (test
// probe; the caller checked the light's type). An area light: shape_sample, then the wi, pdf == 0 and L steps of
// DiffuseAreaLight::Sample_Li as estimate_direct_request has them. The infinite light: p_light is the shadow ray's target, n_light 0.
__global__ void k_light_sample_probe(DScene S, int n, int light, const float *p, const float *nrm, const float *u, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DLight &lt = S.lights[light];
    Isect ref;
    ref.p = F3{p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    ref.perr = F3{0, 0, 0};
    ref.n = F3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
    F3 wi = F3{0, 0, 0}, Li = F3{0, 0, 0}, pl = F3{0, 0, 0}, nl = F3{0, 0, 0};
    float pdf = 0;
    if (lt.type == kLightInfinite) {
        Li = inf_sample_li(S, lt, ref.p, u[2 * i], u[2 * i + 1], &wi, &pdf, &pl);
    } else {
        const LightSample ps = shape_sample(S, lt, ref, u[2 * i], u[2 * i + 1], &pdf);
        pl = ps.p, nl = ps.n;
        if (pdf == 0 || length_sq(ps.p - ref.p) == 0) {
            pdf = 0;
        } else {
            wi = normalize(ps.p - ref.p);
            Li = area_light_L(lt, ps.n, -wi);
        }
    }
    float *r = out + 13 * size_t(i);
    r[0] = wi.x, r[1] = wi.y, r[2] = wi.z;
    r[3] = Li.x, r[4] = Li.y, r[5] = Li.z;
    r[6] = pdf;
    r[7] = pl.x, r[8] = pl.y, r[9] = pl.z;
    r[10] = nl.x, r[11] = nl.y, r[12] = nl.z;
}
void launch_light_sample_probe(const DScene &S, int n, int light, const float *p, const float *nrm, const float *u, float *out, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_light_sample_probe, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, light, p, nrm, u, out);
}
// Light::Pdf_Li of the same lights for reference point i and direction wi: shape_pdf or inf_pdf_li (test probe)
__global__ void k_light_pdf_probe(DScene S, int n, int light, const float *p, const float *nrm, const float *w, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DLight &lt = S.lights[light];
    const F3 wi = F3{w[3 * i], w[3 * i + 1], w[3 * i + 2]};
    if (lt.type == kLightInfinite) {
        out[i] = inf_pdf_li(S, lt, wi);
        return;
    }
    Isect ref;
    ref.p = F3{p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    ref.perr = F3{0, 0, 0};
    ref.n = F3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
    unsigned long long n_tests = 0, n_hits = 0;
    out[i] = shape_pdf(S, lt, ref, wi, &n_tests, &n_hits);
}
void launch_light_pdf_probe(const DScene &S, int n, int light, const float *p, const float *nrm, const float *w, float *out, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_light_pdf_probe, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, light, p, nrm, w, out);
}
// InfiniteAreaLight::Le of infinite light `light` for the direction d of an escaped ray (test probe)
__global__ void k_light_le_probe(DScene S, int n, int light, const float *d, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F3 L = inf_le(S, S.lights[light], F3{d[3 * i], d[3 * i + 1], d[3 * i + 2]});
    put3(out + 3 * i, L);
}
void launch_light_le_probe(const DScene &S, int n, int light, const float *d, float *out, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_light_le_probe, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, light, d, out);
}
// the light k_shade samples at point p with the 1D sample u, and the pdf of that choice (UniformSampleOneLight, integrator.cpp:85-106)
__global__ void k_light_choose(DScene S, int n, const float *p, const float *u, int *light, float *pdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int li = 0;
    float sel = 1.f;
    if (S.n_lights > 1) li = sample_light(S, F3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}, u[i], &sel);
    light[i] = li;
    pdf[i] = sel;
}
void launch_light_choose(const DScene &S, int n, const float *p, const float *u, int *light, float *pdf, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_light_choose, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n, p, u, light, pdf);
}

}  // namespace iile
