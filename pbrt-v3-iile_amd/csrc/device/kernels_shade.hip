// kernels_shade.hip — k_shade: one bounce of PathIntegrator::Li for every hit of a bounce (pipeline overview in
// kernels.hip), and the tabulation of the spatial light distribution it samples from.
#include <cstdlib>
#include <type_traits>

#include "kcommon.h"

namespace iile {

// ---------------------------------------------------------------------------
// SpatialLightDistribution (core/lightdistrib.cpp:91-299): with more than one light the path
// integrator picks the light to sample from a per-voxel distribution. The reference fills a
// hash table lazily; a voxel's distribution is a pure function of its index, so all of them are
// tabulated once at scene creation (k_light_contrib, k_light_cdf) and looked up densely (sample_light, dlight.h).
// Light::Sample_Li at an Interaction without normal or error bounds (lightdistrib.cpp:258-262)
DEV F3 sample_li_plain(const DScene &S, const DLight &lt, F3 po, float u0, float u1, float *pdf) {
    *pdf = 1;
    if (lt.type == kLightInfinite) {
        F3 wi, target;
        return inf_sample_li(S, lt, po, u0, u1, &wi, pdf, &target);
    }
    if (iile_light_is_delta(lt.type)) {
        F3 wi, target;
        return delta_light_li(S, lt, po, &wi, &target);
    }
    Isect ref;  // DiffuseAreaLight::Sample_Li, lights/diffuse.cpp:68-81
    ref.p = po;
    ref.perr = F3{0, 0, 0};
    ref.n = F3{0, 0, 0};
    const LightSample ps = shape_sample(S, lt, ref, u0, u1, pdf);
    if (*pdf == 0 || length_sq(ps.p - po) == 0) {
        *pdf = 0;
        return F3{0, 0, 0};
    }
    const F3 wi = normalize(ps.p - po);
    return area_light_L(lt, ps.n, -wi);
}
DEV float lerp_f(float t, float a, float b) { return (1 - t) * a + t * b; }  // pbrt.h:414
#ifndef IILE_SHADE_MOTION_TU
// SpatialLightDistribution::ComputeDistribution (lightdistrib.cpp:228-299) in two kernels over the table of `stride` = 2 n + 2
// floats per voxel. samples: RadicalInverse(0..4, i) for i < 128 (host table).
// k_light_contrib: one thread per (voxel, light) — blockIdx.y is the light, so a wavefront's lanes share it and sample_li_plain's
// switch on the light's type is wave-uniform. Its 128 samples in order; the sum goes to the record's func[light] slot.
__global__ __launch_bounds__(128) void k_light_contrib(DScene S, const float *samples, float *out, uint32_t stride) {
    const int nv0 = S.light_nv[0], nv1 = S.light_nv[1], nv2 = S.light_nv[2];
    const int v = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (v >= nv0 * nv1 * nv2 || j >= S.n_lights) return;
    const int pi2 = v % nv2, pi1 = (v / nv2) % nv1, pi0 = v / (nv2 * nv1);
    const F3 bmin = F3{S.root_box[0], S.root_box[1], S.root_box[2]}, bmax = F3{S.root_box[3], S.root_box[4], S.root_box[5]};
    const F3 p0 = F3{float(pi0) / float(nv0), float(pi1) / float(nv1), float(pi2) / float(nv2)};
    const F3 p1 = F3{float(pi0 + 1) / float(nv0), float(pi1 + 1) / float(nv1), float(pi2 + 1) / float(nv2)};
    const F3 vmin = F3{lerp_f(p0.x, bmin.x, bmax.x), lerp_f(p0.y, bmin.y, bmax.y), lerp_f(p0.z, bmin.z, bmax.z)};
    const F3 vmax = F3{lerp_f(p1.x, bmin.x, bmax.x), lerp_f(p1.y, bmin.y, bmax.y), lerp_f(p1.z, bmin.z, bmax.z)};
    const DLight &lt = S.lights[j];
    float contrib = 0;
    for (int i = 0; i < 128; ++i) {
        const float *t = samples + 5 * i;
        const F3 po = F3{lerp_f(t[0], vmin.x, vmax.x), lerp_f(t[1], vmin.y, vmax.y), lerp_f(t[2], vmin.z, vmax.z)};
        float pdf;
        const F3 Li = sample_li_plain(S, lt, po, t[3], t[4], &pdf);
        if (pdf > 0) contrib += lum_y(Li) / pdf;
    }
    out[size_t(v) * stride + size_t(j)] = contrib;
}
// k_light_cdf: one thread per voxel turns the contributions k_light_contrib left in func[] into the Distribution1D — the sum in
// light order, the floor of a thousandth of the average, the running cdf and its normalisation (sampling.h:57-69).
__global__ __launch_bounds__(128) void k_light_cdf(DScene S, float *out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= S.light_nv[0] * S.light_nv[1] * S.light_nv[2]) return;
    const int n = S.n_lights;
    float *d = out + size_t(v) * light_record_floats(n);
    float sum = 0;
    for (int j = 0; j < n; ++j) sum = sum + d[j];
    const float avg = sum / float(128 * n);
    const float min_contrib = (avg > 0) ? float(.001 * double(avg)) : 1.f;
    float cdf = 0;
    d[n] = 0;
    for (int j = 0; j < n; ++j) {
        const float f = mx(d[j], min_contrib);
        d[j] = f;
        cdf = cdf + f / float(n);
        d[n + 1 + j] = cdf;
    }
    const float func_int = cdf;
    d[2 * n + 1] = func_int;
    for (int i = 1; i < n + 1; ++i) {
        if (func_int == 0)
            d[n + i] = float(i) / float(n);
        else
            d[n + i] = d[n + i] / func_int;
    }
}

// ---------------------------------------------------------------------------
// The sample table (DScene::stab_*): every Halton sample of the frame, tabulated at scene creation. A frame evaluates each
// radical inverse once per pixel that shares the index — ~127 times at 1080p; the table holds the float the digit chains give,
// made by those chains themselves. One thread per (slot, plane): blockIdx.y = 0 the camera part, 1 + b the record of bounce b.
__global__ __launch_bounds__(256) void k_sample_table(DScene S, float2 *cam, float2 *lens, float4 *shade) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= S.stab_slots) return;
    const uint32_t idx = slot_halton_index(S, slot);
    if (blockIdx.y == 0) {
        cam[slot] = make_float2(sample_dimension(S, idx, 0), sample_dimension(S, idx, 1));
        if (lens) lens[slot] = make_float2(sample_dimension(S, idx, 3), sample_dimension(S, idx, 4));
        return;
    }
    const int b = int(blockIdx.y) - 1, d0 = 5 + 7 * b;
    float r[8];
    for (int i = 0; i < 8; ++i) r[i] = sample_dimension_hi(S, S.perms, idx, d0 + i);
    float4 *rec = shade + (size_t(b) * S.stab_slots + slot) * 2;
    rec[0] = make_float4(r[0], r[1], r[2], r[3]);
    rec[1] = make_float4(r[4], r[5], r[6], r[7]);
}
// the table's time column for a moving camera (DCameraMotion::stab_time): dimension 2 of every slot
__global__ __launch_bounds__(256) void k_sample_table_time(DScene S, float *time) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= S.stab_slots) return;
    time[slot] = sample_dimension(S, slot_halton_index(S, slot), 2);
}
// test probe: the table's entries for sample k[i] of pixel (px[i], py[i]); bounce[i] >= 0: the eight dimensions of that bounce's
// record, bounce[i] < 0: the camera part {u0, u1, l0, l1, 0, 0, 0, 0} (l0 = l1 = 0 without a lens part)
__global__ void k_sample_table_read(DScene S, int n, const int *px, const int *py, const int *k, const int *bounce, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = sample_slot(S, px[i], py[i], uint32_t(k[i]));
    float4 a = make_float4(0, 0, 0, 0), b = make_float4(0, 0, 0, 0);
    if (bounce[i] < 0) {
        const float2 c = S.stab_cam[slot];
        a.x = c.x, a.y = c.y;
        if (S.stab_lens) a.z = S.stab_lens[slot].x, a.w = S.stab_lens[slot].y;
    } else {
        const float4 *rec = S.stab_shade + (size_t(bounce[i]) * S.stab_slots + slot) * 2;
        a = rec[0], b = rec[1];
    }
    reinterpret_cast<float4 *>(out)[2 * size_t(i)] = a;
    reinterpret_cast<float4 *>(out)[2 * size_t(i) + 1] = b;
}
#endif  // !IILE_SHADE_MOTION_TU

// shade: one bounce of PathIntegrator::Li (path.cpp:81-191) for every hit of the
// queue that extend just resolved.
// Waves per SIMD = resident blocks per CU. The plain and the extended builds run at 4 (<= 128 VGPRs, ~10 spilled to scratch
// outside the hot sections: killeroo 18.3 -> 17.2 ms, the closed room 53.5 -> 50.1 ms against 3 waves, profiles/r03_ab_shade_4_waves.txt
// — at the 168 VGPRs the kernel wanted before its uniform table reads became scalar loads, 4 waves lost: 23.6 vs 22.0 ms);
// the textured build is better off at 3 (<= 168 VGPRs; 50.2 vs 52.8 ms at 4).
// TEX: some material takes a parameter from an image texture (implies EXT)
#ifndef IILE_SHADE_WAVES
#define IILE_SHADE_WAVES 4
#endif
#ifndef IILE_SHADE_WAVES_TEX
#define IILE_SHADE_WAVES_TEX 3
#endif
#ifndef IILE_SHADE_WAVES_DISNEY
#define IILE_SHADE_WAVES_DISNEY 2
#endif
constexpr int shade_waves(bool tex, bool disney = false) { return disney ? IILE_SHADE_WAVES_DISNEY : (tex ? IILE_SHADE_WAVES_TEX : IILE_SHADE_WAVES); }
// TAB: the scene has a sample table (DScene::stab_*; never an instrumented build, never Sobol'). A wavefront whose valid lanes all
//   sit at dimension 5 + 7 bounce — every one unless a specular-only vertex or a roulette draw made its lanes disagree — reads its
//   vertex's eight samples as one 32-byte record; `hidx` is then the sample slot, not the Halton index. The other wavefronts run
//   the per-lane digit chains over the permutations in HBM: this build stages nothing in LDS and has no barrier.
#ifndef IILE_SHADE_TAB_REREAD
#define IILE_SHADE_TAB_REREAD 0  // 1: the continuation reads its samples from the record again instead of keeping them in registers
#endif
// DIS: the scene has a Disney material (DScene::disney_build): the vertex's BSDF is a DisneyBsdf (dbsdf.h), always in the textured
//   flavour. The instrumented build includes it.
// MOT: the scene's camera moves (LaunchCfg::camera_moves) and some material reads a texture: the camera differentials rebuilt at the first
//   vertex go through the transform at the ray's time. Three builds only — the instrumented one and the two Disney builds, which
//   shade every material — so that no build of a scene whose camera stands still carries any of it. They are compiled in a
//   translation unit of their own, kernels_shade_motion.hip, which includes this file with IILE_SHADE_MOTION_TU set: it takes
//   the kernel template and its helpers from here, leaves out every other kernel and launcher, and defines launch_shade_motion.
template <bool COUNT, bool EXT, bool TEX, bool TAB = false, bool DIS = false, bool MOT = false>
__global__ __launch_bounds__(kBlock, shade_waves(TEX, DIS)) void k_shade(DScene S, PassDesc P, PassBuffers B, int bounce, uint32_t plane) {
    static_assert(!(TAB && COUNT), "the instrumented build keeps the digit chains");
    static_assert(!DIS || (EXT && TEX && !COUNT), "the Disney builds are textured ones");
    static_assert(!MOT || (TEX && (DIS || COUNT)), "the moving camera's builds are the instrumented one and the Disney builds");
    constexpr bool DZ = DIS || COUNT;
    typename std::conditional<TAB, const uint16_t *, lds_u16 *>::type s_perms;
    if constexpr (TAB) {
        s_perms = S.perms;
    } else {
        // digit permutations of the Halton sampler staged in LDS (dynamic shared memory)
        extern __shared__ __attribute__((aligned(16))) uint16_t s_perms_raw[];
        if (S.sobol) {
            // SobolSampler: four byte-table lookups per dimension, read through the caches (DScene::sobol_bt) — nothing staged
        } else {
            for (int i = threadIdx.x; i < S.n_perms; i += kBlock) s_perms_raw[i] = S.perms[i];
        }
        __syncthreads();
        s_perms = (lds_u16 *)s_perms_raw;
    }
    const uint32_t count = B.counts[kCntShade + bounce];
    const float4 *ro = B.ray_o[bounce & 1], *rd = B.ray_d[bounce & 1];
    float4 *no = B.ray_o[(bounce + 1) & 1], *nd = B.ray_d[(bounce + 1) & 1];
    const float4 *rs = B.ray_s[bounce & 1];
    float4 *ns = B.ray_s[(bounce + 1) & 1];
    unsigned long long n_nee = 0, n_term = 0, n_pdf_tests = 0, n_pdf_hits = 0;
    // diagnostic build only: wave cycles per section of a round, summed per wavefront, added to DCounters::path_length[0..7]
    // at the end: 0 regroup, 1 loads + Halton, 2 interaction + BSDF, 3 EstimateDirect, 4 end of section A,
    // 5 record stores, 6 continuation, 7 next-ray store
    DiagSums<IILE_SWITCH(IILE_SHADE_STAMPS) && !COUNT, 8> stamps;
    WaveOut ray_out{0, 0}, nee_out{0, 0}, mis_out{0, 0};
    auto pad_ray = [&](uint32_t sl) { no[sl] = make_float4(0, 0, 0, b2f(kInvalid)); };
    auto pad_nee = [&](uint32_t sl) { B.nee[plane + sl] = B.nee[4 * plane + sl] = make_float4(0, 0, 0, b2f(kInvalid)); };
    auto pad_mis = [&](uint32_t sl) { B.nee[2 * plane + sl] = make_float4(0, 0, 0, b2f(kInvalid)); };
    __shared__ uint32_t s_entry[kWavesPerBlock][kShadeChunk];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *const head = &B.counts[kCntShdHead + bounce];
    for (;;) {
        // chunks are drawn dynamically: a chunk of glossy hits costs several matte ones
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(head, uint32_t(kShadeChunk));
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= count) break;
        // Each wavefront takes kShadeChunk consecutive hits and regroups them by shading class
        // (material type, sphere) so that its rounds below run one code path each: past the
        // first bounce neighbouring queue entries hit unrelated materials (VALU lane
        // utilisation 39% -> 60% at bounce 1). The hits stay inside their chunk, so the queues
        // written here keep their locality. Wave-local counting sort: no block barrier.
        uint32_t ent[kShadeChunk / 64];
#pragma unroll
        for (int j = 0; j < kShadeChunk / 64; ++j) {
            const uint32_t qi = base + uint32_t(j) * 64u + uint32_t(lane);
            ent[j] = qi < count ? B.shade_q[qi] : kInvalid;
        }
        uint32_t run = 0;
        for (uint32_t c = 0; c < 8; ++c) {
#pragma unroll
            for (int j = 0; j < kShadeChunk / 64; ++j) {
                const bool is_c = (ent[j] == kInvalid ? 7u : ent[j] >> kSlotBits) == c;
                const uint64_t m = __ballot(is_c);
                if (is_c)
                    s_entry[wave][run + __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u))] = ent[j];
                run += uint32_t(__popcll(m));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        stamps.mark(0);
      for (int round = 0; round < kShadeChunk / 64; ++round) {
        const uint32_t mine = s_entry[wave][round * 64 + lane];
        const bool valid = mine != kInvalid;
        if (__ballot(valid) == 0) break;  // padding sorts last
        const uint32_t slot = mine & ((1u << kSlotBits) - 1u);
        // The loop body is two converged sections, each ending in a queue append, so that the
        // NEE record's ~20 registers are dead before the continuation is sampled:
        //   A: interaction, Le, BSDF, both halves of EstimateDirect  -> NEE record
        //   B: next direction, throughput, Russian roulette          -> next ray
        bool surface = false;  // a hit that still scatters (bounces < maxDepth)
        bool alive = false, returned_early = false;
        uint32_t pid = 0, hidx = 0;  // hidx: the sample's Halton (Sobol') index; TAB: its slot in the sample table
        int dim = 0;
        // TAB: this wavefront's vertices take their samples from the table, here their record (dimensions 5 + 7 bounce ..)
        bool tab_wave = false;
        float4 rec_a = make_float4(0, 0, 0, 0), rec_b = make_float4(0, 0, 0, 0);
        auto chain_index = [&]() { return TAB ? slot_halton_index(S, hidx) : hidx; };  // what the digit chains start from
        Isect is;
        typename bsdf_of<DZ>::type bsdf;
        F3 beta = F3{0, 0, 0}, ray_d = F3{0, 0, 1};
        uint32_t state_next = 0;
        {
            bool emit_nee = false;
            F3 so = F3{0, 0, 0}, sd = F3{0, 0, 1}, mo = F3{0, 0, 0}, md = F3{0, 0, 1};
            F3 A = F3{0, 0, 0}, Bc = F3{0, 0, 0};
            uint32_t nee_flags = 0, nee_light = 0;
            float light_sel_pdf = 1.f;  // lightPdf of UniformSampleOneLight: Ld is divided by it
            if (valid) {
                float4 o4, d4;
                uint32_t fused_hidx = 0;
                const float4 h4 = B.hits[slot];
                if (bounce == 0 && P.gen_fused) {
                    // the camera ray again, as the first k_extend made it (queue 0 is dense: slot == path id)
                    const float4 cpf = B.beta[slot];  // pFilm and the Halton index, left by k_extend
                    fused_hidx = f2b(cpf.z);
                    float cl0 = 0, cl1 = 0;
                    if (S.lens_radius > 0) {
                        if (TAB) {
                            const float2 cl = S.stab_lens[fused_hidx];
                            cl0 = cl.x, cl1 = cl.y;
                        } else {
                            cl0 = sample_dimension(S, s_perms, fused_hidx, 3);
                            cl1 = sample_dimension(S, s_perms, fused_hidx, 4);
                        }
                    }
                    F3 co, cd;
                    float ctm;
                    camera_ray<false>(S, cpf.x, cpf.y, cl0, cl1, &co, &cd, &ctm, opaque_zero());  // (gen_fused: never an environment camera)
                    o4 = make_float4(co.x, co.y, co.z, b2f(slot));
                    d4 = make_float4(cd.x, cd.y, cd.z, ctm);
                } else {
                    o4 = ro[slot];
                    d4 = rd[slot];
                }
                pid = f2b(o4.w);
                // a path arrives at its first vertex with beta = 1 at sampler dimension 5 (after
                // the camera sample): k_generate does not spend 16 B per path on saying so
                // from bounce 1 on the path's state arrived with its ray (PassBuffers::ray_s; dimension | specularBounce << 16 in
                // the direction record's .w)
                const float4 beta4 = bounce == 0 ? make_float4(1, 1, 1, 0) : rs[slot];
                const uint32_t state_w = bounce == 0 ? 5u : f2b(d4.w);
                beta = F3{beta4.x, beta4.y, beta4.z};
                dim = int(state_w & 0xffffu);
                const bool prev_specular = EXT && (state_w >> 16) != 0;  // specularBounce of path.cpp:150
                hidx = bounce == 0 ? ((P.gen_fused) ? fused_hidx : B.hindex[pid]) : f2b(beta4.w);
                // The four samples of EstimateDirect (dims dim+1 .. dim+4; dim itself is the
                // 1D sample SampleDiscrete consumes), drawn here while few registers are live.
                // Every path of a bounce normally sits at the same dimension.
                float u_nee[4] = {0, 0, 0, 0};
                if (bounce < S.max_depth) {
                    const int dim_u = __builtin_amdgcn_readfirstlane(dim);
                    const bool dim_uniform = __ballot(dim != dim_u) == 0;
                    if (TAB) {
                        tab_wave = dim_uniform && dim_u == 5 + 7 * bounce;
                        if (tab_wave) {
                            const float4 *rec = S.stab_shade + (size_t(bounce) * S.stab_slots + hidx) * 2;
                            rec_a = rec[0];
                            rec_b = rec[1];
                            u_nee[0] = rec_a.y, u_nee[1] = rec_a.z, u_nee[2] = rec_a.w, u_nee[3] = rec_b.x;
                        } else {
                            sample_dimensions_n<4>(S, s_perms, dim_u + 1, false, dim + 1, chain_index(), u_nee);
                        }
                    } else {
                        sample_dimensions_n<4>(S, s_perms, dim_u + 1, dim_uniform, dim + 1, hidx, u_nee);
                    }
                }
                stamps.mark(1);
                const int prim = int(f2b(h4.x));
                const F3 ray_o = F3{o4.x, o4.y, o4.z};
                ray_d = F3{d4.x, d4.y, d4.z};
                float4 v0 = S.tri_verts[3 * size_t(prim)];
                float4 v1 = S.tri_verts[3 * size_t(prim) + 1];
                float4 v2 = S.tri_verts[3 * size_t(prim) + 2];
                keep_whole(v0, v1, v2);  // three 16-byte loads (not three of 12 bytes and three of 4)
                const uint32_t flags = f2b(v0.w);
                const int material = int(f2b(v1.w)), light = int(f2b(v2.w));
                if (flags & 1u) {
                    // the closest hit was a sphere or a quadric: redo its (deterministic) root
                    // selection to recover the object-space ray and refined hit point
                    shape_hit_interaction<TEX, EXT>(S, S.prim_shape[prim], ray_o, ray_d, &is);   // (TEX: with (u, v), dp/du, dp/dv and dn/du, dn/dv for the texture lookups and Material::Bump)
                } else {
                    triangle_interaction(S, prim, flags, F3{v0.x, v0.y, v0.z}, F3{v1.x, v1.y, v1.z},
                                         F3{v2.x, v2.y, v2.z}, ray_d, h4.y, h4.z, h4.w, &is);
                }
                if (EXT && S.probe_mode && bounce == 0) {  // IISPTdIntegrator::Li, iispt_d.cpp:96-108
                    const F3 cv = is.p - ray_o;
                    const DProbeCam &cam = P.probe_cams[(pid / uint32_t(P.kc)) / (256u * uint32_t(P.probe_tiles))];
                    B.aux[pid] = make_float4(cam.nrm[0] * is.n.x + cam.nrm[1] * is.n.y + cam.nrm[2] * is.n.z,
                                             cam.nrm[3] * is.n.x + cam.nrm[4] * is.n.y + cam.nrm[5] * is.n.z,
                                             cam.nrm[6] * is.n.x + cam.nrm[7] * is.n.y + cam.nrm[8] * is.n.z, sqrtf(dot(cv, cv)));
                }
                // emitted light at the first vertex and after a specular bounce (path.cpp:91-101); the probe
                // integrator leaves out the camera ray's own vertex (iispt_d.cpp:116-123)
                if (((bounce == 0 && !(EXT && S.probe_mode)) || prev_specular) && light >= 0) {
                    const float4 L4 = B.L[pid];
                    const F3 L = F3{L4.x, L4.y, L4.z} + beta * area_light_L(S.lights[light], is.n, -ray_d);
                    B.L[pid] = make_float4(L.x, L.y, L.z, 0);
                }
                if (bounce < S.max_depth) {
                    surface = true;
                    if (TEX && S.textured_materials) {
                        // isect.ComputeScatteringFunctions(ray, ...): ComputeDifferentials (interaction.cpp:95-149)
                        // then the material's Texture::Evaluate calls. Only the camera ray carries differentials
                        // (path.cpp:159 spawns plain Rays); its auxiliary rays are a function of the camera
                        // sample, rebuilt here from the path's pixel instead of travelling with the ray.
                        const DMaterial &m0 = S.materials[material];
                        if (m0.kd_tex >= 0 || m0.ks_tex >= 0 || m0.kr_tex >= 0 || m0.kt_tex >= 0 || m0.bump_tex >= 0 || m0.rough_tex >= 0 || m0.sigma_tex >= 0 || m0.opacity_tex >= 0 || m0.rough_tex_v >= 0) {
                            TexDiff td = TexDiff{0, 0, 0, 0};
                            F3 dpdx = F3{0, 0, 0}, dpdy = F3{0, 0, 0};
                            if (bounce == 0) {
                                int px = 0, py = 0;
                                uint32_t kk = 0;
                                path_pixel(S, P, pid, &px, &py, &kk);
                                float u0, u1, l0 = 0, l1 = 0, time = 0;
                                if (TAB) {
                                    const float2 cu = S.stab_cam[hidx];
                                    u0 = cu.x, u1 = cu.y;
                                    if (S.lens_radius > 0) {
                                        const float2 cl = S.stab_lens[hidx];
                                        l0 = cl.x, l1 = cl.y;
                                    }
                                    if (MOT) time = camera_ray_time(S, camera_motion(S)->stab_time[hidx]);
                                } else {
                                    u0 = sample_dimension(S, s_perms, hidx, 0, px, py), u1 = sample_dimension(S, s_perms, hidx, 1, px, py);
                                    if (S.lens_radius > 0) {
                                        l0 = sample_dimension(S, s_perms, hidx, 3);
                                        l1 = sample_dimension(S, s_perms, hidx, 4);
                                    }
                                    if (MOT) time = camera_ray_time(S, sample_dimension(S, s_perms, hidx, 2));  // the time k_generate drew
                                }
                                const RayDiff rdiff =
                                    S.probe_mode ? probe_differentials(S, P.probe_cams[(pid / uint32_t(P.kc)) / (256u * uint32_t(P.probe_tiles))],
                                                                       float(px) + u0, float(py) + u1, ray_o, ray_d)
                                                 : camera_differentials<MOT>(S, float(px) + u0, float(py) + u1, l0, l1, ray_o, ray_d, time);
                                td = compute_differentials(is, rdiff, &dpdx, &dpdy);
                            }
                            if (m0.bump_tex >= 0) bump(S, m0.bump_tex, td, dpdx, dpdy, &is);  // `if (bumpMap) Bump(bumpMap, si)` comes first
                            const DMaterial mm = textured_material(S, m0, is, td, dpdx, dpdy);
                            bsdf = make_bsdf_at<EXT, DZ>(S, material, mm, is);
                        } else {
                            bsdf = make_bsdf_at<EXT, DZ>(S, material, m0, is);
                        }
                    } else {
                        bsdf = make_bsdf_at<EXT, DZ>(S, material, S.materials[material], is);
                    }
                    stamps.mark(2);
                    if (n_nonspec(bsdf) > 0) {  // NumComponents(BSDF_ALL & ~BSDF_SPECULAR) > 0, path.cpp:118
                        ++n_nee;
                        // UniformSampleOneLight (integrator.cpp:85-106). One light: it is chosen with pdf 1
                        // (SampleDiscrete still consumes a 1D sample). Several: through the voxel's
                        // distribution of the spatial light distribution (lightdistrib.cpp:134-226,
                        // tabulated at scene creation); a zero pdf returns before any further sample.
                        int li = 0;
                        if (EXT && S.n_lights > 1) {
                            float ul;
                            if (TAB && tab_wave)
                                ul = rec_a.x;
                            else
                                ul = sample_dimension_hi(S, s_perms, chain_index(), dim);
                            li = sample_light(S, is.p, ul, &light_sel_pdf);
                        }
                        if (S.n_lights > 0) ++dim;
                        if (S.n_lights > 0 && light_sel_pdf != 0) {
                            // (the plain build has one light, an emitting sphere: both wave-uniform, see uniform_sphere)
                            DLight lt_u;
                            DSphere lsp_u;
                            if (!EXT) {
                                lt_u = uniform_entry(S.lights, 0);
                                lsp_u = uniform_entry(S.spheres, lt_u.sphere);
                            }
                            const DLight &lt = EXT ? S.lights[li] : lt_u;
                            const DSphere &lsp = EXT ? S.spheres[lt.sphere] : lsp_u;
                            dim += 4;  // uLight and uScattering, drawn for every kind of light
                            nee_flags = estimate_direct_request<EXT, COUNT>(S, lt, &lsp, is, bsdf, u_nee[0], u_nee[1], u_nee[2], u_nee[3], so, sd,
                                                                            A, mo, md, Bc, &n_pdf_tests, &n_pdf_hits);
                            stamps.mark(3);
                            nee_light = uint32_t(li);
                            // a record with neither ray adds nothing to L; only the instrumented build needs it (zero_radiance)
                            emit_nee = COUNT || nee_flags != 0;
                        }
                    }
                }
            }
            stamps.mark(4);
            const uint32_t eslot = out_take(nee_out, &B.counts[kCntNee + bounce], emit_nee, pad_nee);
            // the MIS rays go to a dense queue of their own (planes 2 and 3): most records have none
            const bool emit_mis = emit_nee && (nee_flags & NEE_HAS_MIS) != 0;
            const uint32_t mslot = out_take(mis_out, &B.counts[kCntMis + bounce], emit_mis, pad_mis);
            if (emit_nee) {
                B.nee[eslot] = make_float4(so.x, so.y, so.z, light_sel_pdf);
                B.nee[plane + eslot] = make_float4(sd.x, sd.y, sd.z, b2f(nee_flags));
                if (nee_flags & NEE_HAS_MIS) {
                    // the general record: k_shadow forms beta * (([unoccluded] A + [MIS ray lit] B) / lightPdf) once it knows both
                    B.nee[4 * plane + eslot] = make_float4(A.x, A.y, A.z, b2f(pid));
                    B.nee[5 * plane + eslot] = make_float4(Bc.x, Bc.y, Bc.z, b2f(nee_light));
                    B.nee[6 * plane + eslot] = make_float4(beta.x, beta.y, beta.z, b2f(pid));  // beta before this bounce
                } else {
                    // 98 % of the records have no MIS ray: what k_shadow would compute for "unoccluded" is known here — the same
                    // operations in the same order, beta * ((0 + A) / lightPdf) (x / 1 is x: skipped where every lane's is 1) —
                    // so the record carries that product and no throughput plane (16 B less written and read per record)
                    const F3 Ld = F3{0, 0, 0} + A;
                    const F3 pre = (__ballot(light_sel_pdf != 1.f) == 0) ? beta * Ld : beta * sdiv(Ld, light_sel_pdf);
                    B.nee[4 * plane + eslot] = make_float4(pre.x, pre.y, pre.z, b2f(pid));
                }
            }
            if (emit_mis) {
                B.nee[2 * plane + mslot] = make_float4(mo.x, mo.y, mo.z, b2f(eslot));  // + the record it belongs to
                B.nee[3 * plane + mslot] = make_float4(md.x, md.y, md.z, b2f(nee_light));
            }
        }
        stamps.mark(5);
        F3 next_o = F3{0, 0, 0}, next_d = F3{0, 0, 1};
        if (P.skip_last_bounce == 2 && bounce + 1 >= S.max_depth) surface = false;  // the next vertex could add nothing: see PassDesc
        if (surface) {
            // next direction (path.cpp:133-156)
            float u_bsdf[2], ur_tab = 0;
            if (TAB && tab_wave) {
                const int off = dim - (5 + 7 * bounce);
                if (IILE_SHADE_TAB_REREAD) {
                    const float *rf = reinterpret_cast<const float *>(S.stab_shade + (size_t(bounce) * S.stab_slots + hidx) * 2) + off;
                    u_bsdf[0] = rf[0], u_bsdf[1] = rf[1];
                    if (bounce > 3) ur_tab = rf[2];
                } else {
                    record_continuation(rec_a, rec_b, off, &u_bsdf[0], &u_bsdf[1], &ur_tab);
                }
            } else {
                const int dim_u = __builtin_amdgcn_readfirstlane(dim);
                sample_dimensions_n<2>(S, s_perms, dim_u, !TAB && __ballot(dim != dim_u) == 0, dim, chain_index(), u_bsdf);
            }
            const float u0 = u_bsdf[0], u1 = u_bsdf[1];
            dim += 2;
            float pdf = 0;
            F3 wi = F3{0, 0, 0};
            bool sampled_specular = false, sampled_transmission = false;
            const F3 f = bsdf_sample_f(bsdf, -ray_d, &wi, u0, u1, &pdf, EXT, &sampled_specular, &sampled_transmission);
            // etaScale (path.cpp:81, 151-157): a path state of its own, touched only in scenes with glass
            float eta_scale = 1.f;
            if (EXT && S.has_glass && bounce > 0) eta_scale = B.eta_scale[pid];
            if (!(is_black(f) || pdf == 0.f)) {
                beta = beta * sdiv(f * absdot(wi, is.sn), pdf);
                const float by = lum_y(beta);
                if (by < 0.f || is_nan(by)) {
                    returned_early = true;  // `return L` (path.cpp:143-145)
                } else {
                    next_o = offset_ray_origin(is.p, is.perr, is.n, wi);
                    next_d = wi;
                    alive = true;
                    if (sampled_specular && sampled_transmission) {
                        const float eta = bsdf.path_eta;   // BSDF::eta
                        eta_scale *= (dot(-ray_d, is.n) > 0) ? (eta * eta) : 1 / (eta * eta);
                    }
                    // Russian roulette on rrBeta = beta * etaScale (path.cpp:182-190)
                    const F3 rr_beta = beta * eta_scale;
                    const float mc = max3(rr_beta.x, rr_beta.y, rr_beta.z);
                    if (mc < S.rr_threshold && bounce > 3) {
                        const float q = mx(.05f, 1 - mc);
                        float ur;
                        if (TAB && tab_wave)
                            ur = ur_tab;
                        else
                            ur = sample_dimension_hi(S, s_perms, chain_index(), dim);
                        ++dim;
                        if (ur < q)
                            alive = false;
                        else
                            beta = sdiv(beta, 1 - q);
                    }
                }
            }
            // last shaded vertex: only a specular continuation can still pick up emitted light (PassDesc::skip_last_bounce)
            if (EXT && P.skip_last_bounce == 1 && bounce + 1 >= S.max_depth && !sampled_specular) alive = false;
            if (EXT && alive && S.has_glass) B.eta_scale[pid] = eta_scale;
            // sampler dimension | specularBounce << 16
            state_next = uint32_t(dim) | (sampled_specular ? 0x10000u : 0u);  // sampler dimension | specularBounce << 16
        }
        // ReportValue(pathLength, bounces): a path that ends in this iteration leaves the
        // loop with bounces == bounce (not counted on the early `return L`)
        if (COUNT && valid && !alive && !returned_early) ++n_term;
        stamps.mark(6);
        const uint32_t nslot = out_take(ray_out, &B.counts[kCntRay + bounce + 1], alive, pad_ray);
        if (alive) {
            no[nslot] = make_float4(next_o.x, next_o.y, next_o.z, b2f(pid));
            nd[nslot] = make_float4(next_d.x, next_d.y, next_d.z, b2f(state_next));
            ns[nslot] = make_float4(beta.x, beta.y, beta.z, b2f(hidx));
        }
        stamps.mark(7);
      }
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites s_entry
    }
    out_flush(ray_out, pad_ray);
    out_flush(nee_out, pad_nee);
    out_flush(mis_out, pad_mis);
    stamps.flush(B.counters, 0);
    if (COUNT) {
        flush_counter(&B.counters->nee_evals, n_nee);
        flush_counter(&B.counters->path_length[bounce < 7 ? bounce : 7], n_term);
        flush_counter(&B.counters->tri_tests, n_pdf_tests);  // Triangle::Intersect calls of Shape::Pdf
        flush_counter(&B.counters->tri_hits, n_pdf_hits);
    }
}


// ---------------------------------------------------------------------------
// launchers
#ifdef IILE_SHADE_MOTION_TU
// a moving camera whose differentials are read (some material is textured, or the instrumented build runs): the Disney builds,
// which shade every material, with the sample table or without
void launch_shade_motion(const DScene &S, const PassDesc &P, const PassBuffers &B, int bounce, uint32_t max_rays, const LaunchCfg &cfg) {
    const dim3 grid(grid_blocks(max_rays, cfg.n_cus, shade_waves(true, !cfg.count_stats)));
    const size_t perm_bytes = S.sobol ? size_t(16) : (size_t(S.n_perms) * sizeof(uint16_t) + 15) & ~size_t(15);
    if (cfg.count_stats)
        hipLaunchKernelGGL((k_shade<true, true, true, false, false, true>), grid, dim3(kBlock), perm_bytes, cfg.stream, S, P, B, bounce, B.queue_cap);
    else if (S.stab_shade)
        hipLaunchKernelGGL((k_shade<false, true, true, true, true, true>), grid, dim3(kBlock), 0, cfg.stream, S, P, B, bounce, B.queue_cap);
    else
        hipLaunchKernelGGL((k_shade<false, true, true, false, true, true>), grid, dim3(kBlock), perm_bytes, cfg.stream, S, P, B, bounce, B.queue_cap);
}
#else
void launch_shade(const DScene &S, const PassDesc &P, const PassBuffers &B, int bounce, uint32_t max_rays, const LaunchCfg &cfg) {
    // as many blocks as are resident at the build's waves per SIMD: the static split has no tail
    const bool tex_build = cfg.count_stats || S.textured_materials || S.probe_mode;
    if (cfg.camera_moves && tex_build && !S.probe_mode) return launch_shade_motion(S, P, B, bounce, max_rays, cfg);
    const bool dis_build = S.disney_build && !cfg.count_stats;
    const dim3 grid(grid_blocks(max_rays, cfg.n_cus, shade_waves(tex_build, dis_build)));
    const size_t perm_bytes = S.sobol ? size_t(16) : (size_t(S.n_perms) * sizeof(uint16_t) + 15) & ~size_t(15);
    if (dis_build) {
        // a scene with a Disney material: the one Disney build, with the sample table or without
        if (S.stab_shade)
            hipLaunchKernelGGL((k_shade<false, true, true, true, true>), grid, dim3(kBlock), 0, cfg.stream, S, P, B, bounce, B.queue_cap);
        else
            hipLaunchKernelGGL((k_shade<false, true, true, false, true>), grid, dim3(kBlock), perm_bytes, cfg.stream, S, P, B, bounce, B.queue_cap);
    } else if (S.stab_shade && !cfg.count_stats) {
        // the scene has a sample table: the builds that read it (no permutations in LDS, no dynamic shared memory)
        if (S.textured_materials)  // (a probe pass never carries a table)
            hipLaunchKernelGGL((k_shade<false, true, true, true>), grid, dim3(kBlock), 0, cfg.stream, S, P, B, bounce, B.queue_cap);
        else if (S.extended_features)
            hipLaunchKernelGGL((k_shade<false, true, false, true>), grid, dim3(kBlock), 0, cfg.stream, S, P, B, bounce, B.queue_cap);
        else
            hipLaunchKernelGGL((k_shade<false, false, false, true>), grid, dim3(kBlock), 0, cfg.stream, S, P, B, bounce, B.queue_cap);
    } else if (cfg.count_stats)
        hipLaunchKernelGGL((k_shade<true, true, true>), grid, dim3(kBlock), perm_bytes, cfg.stream, S, P, B, bounce, B.queue_cap);
    else
        // Scenes of killeroo-simple's kind (one emitting sphere, matte / plastic only) run a build of the
        // kernel without the code for the wider feature set: it costs them registers otherwise (+0.7 ms);
        // likewise image textures have their own build
        if (S.textured_materials || S.probe_mode)
            hipLaunchKernelGGL((k_shade<false, true, true>), grid, dim3(kBlock), perm_bytes, cfg.stream, S, P, B, bounce, B.queue_cap);
        else if (S.extended_features)
            hipLaunchKernelGGL((k_shade<false, true, false>), grid, dim3(kBlock), perm_bytes, cfg.stream, S, P, B, bounce, B.queue_cap);
        else
            hipLaunchKernelGGL((k_shade<false, false, false>), grid, dim3(kBlock), perm_bytes, cfg.stream, S, P, B, bounce, B.queue_cap);
}
void launch_sample_table(const DScene &S, float2 *cam, float2 *lens, float4 *shade, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_sample_table, dim3((S.stab_slots + 255) / 256, 1 + S.max_depth), dim3(256), 0, cfg.stream, S, cam, lens, shade);
}
void launch_sample_table_time(const DScene &S, float *time, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_sample_table_time, dim3((S.stab_slots + 255) / 256), dim3(256), 0, cfg.stream, S, time);
}
void launch_sample_table_read(const DScene &S, int n, const int *px, const int *py, const int *k, const int *bounce, float *out, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_sample_table_read, dim3((n + 127) / 128), dim3(128), 0, cfg.stream, S, n, px, py, k, bounce, out);
}
void launch_light_distributions(const DScene &S, const float *samples, float *out, const LaunchCfg &cfg) {
    const int n = S.light_nv[0] * S.light_nv[1] * S.light_nv[2];
    // (lights ride in the grid's y: at most 65535 of them; the table's byte cap admits far fewer on any grid of more than 64 voxels,
    //  and the loop covers the flat grids)
    for (int l0 = 0; l0 < S.n_lights; l0 += 32768) {
        DScene part = S;
        part.lights = S.lights + l0;
        part.n_lights = std::min(S.n_lights - l0, 32768);
        hipLaunchKernelGGL(k_light_contrib, dim3((n + 127) / 128, part.n_lights), dim3(128), 0, cfg.stream, part, samples, out + l0,
                           light_record_floats(S.n_lights));
    }
    hipLaunchKernelGGL(k_light_cdf, dim3((n + 127) / 128), dim3(128), 0, cfg.stream, S, out);
}

#endif  // IILE_SHADE_MOTION_TU

}  // namespace iile
