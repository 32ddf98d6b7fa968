// kernels.hip — the wavefront path tracer's pipeline and its three kernels outside traversal, shading and film: generate, miss, mis_lit.
//
// Pipeline per pass (one pass = owned tiles x a chunk of sample indices):
//   generate -> [ extend -> shade -> mis -> mis_lit -> shadow ] x (maxDepth + 1) -> film_accumulate
// and, after the last pass, film_resolve.
//
//   generate  HaltonSampler + PerspectiveCamera::GenerateRayDifferential; fills ray queue 0
//   extend    BVHAccel::Intersect over a ray queue (closest hit), LDS traversal stacks
//   shade     the body of PathIntegrator::Li for one bounce: interaction, Le, BSDF, light
//             sampling + BSDF sampling of EstimateDirect (emits one NEE record holding a
//             shadow ray and an MIS ray), next direction, Russian roulette; compacts the
//             surviving paths into the next ray queue with ballot + one atomic per wavefront
//   shadow    BVHAccel::IntersectP for the shadow ray of each NEE record
//   mis       BVHAccel::Intersect for the MIS ray of each NEE record
//   shadow    BVHAccel::IntersectP for its shadow ray; L += beta * Ld
//
// All kernels are persistent grid-stride loops that read their queue length
// from device memory, so a whole pass is enqueued without host synchronisation.
// 64-lane wavefronts throughout: ballots are 64-bit, lane = threadIdx.x & 63.
#include "kcommon.h"

namespace iile {

// ---------------------------------------------------------------------------
// MOT: the build for a moving camera (camera_motion, dscene.h): dimension 2 of the camera sample is the ray's time
template <bool MOT>
__global__ __launch_bounds__(kBlock) void k_generate(DScene S, PassDesc P, PassBuffers B, int count_stats) {
    unsigned long long n_cam = 0;
    for (uint32_t base = blockIdx.x * kBlock; base < P.n_paths; base += gridDim.x * kBlock) {
        const uint32_t pid = base + threadIdx.x;
        bool valid = pid < P.n_paths;
        int px = 0, py = 0;
        uint32_t k = 0;
        if (valid) valid = path_pixel(S, P, pid, &px, &py, &k);
        F3 o = F3{0, 0, 0}, d = F3{0, 0, 1};
        float tmax = 0;
        if (valid) {
            // Sampler::GetCameraSample (sampler.cpp:46-52): dims 0,1 film, 2 time, 3,4 lens
            // (with a sample table — DScene::stab_cam — read from it; idx is then the sample's slot, as the table build of k_shade wants)
            uint32_t idx;
            // (dimension 2 is read for a moving camera alone; the table then has a time column)
            float u0, u1, l0 = 0, l1 = 0, time = 0;
            if (S.stab_cam) {
                idx = sample_slot(S, px, py, k);
                const float2 cu = S.stab_cam[idx];
                u0 = cu.x, u1 = cu.y;
                if (S.lens_radius > 0) {
                    const float2 cl = S.stab_lens[idx];
                    l0 = cl.x, l1 = cl.y;
                }
                if (MOT) time = camera_ray_time(S, camera_motion(S)->stab_time[idx]);
            } else {
                idx = sample_index(S, px, py, k);
                u0 = sample_dimension(S, idx, 0, px, py), u1 = sample_dimension(S, idx, 1, px, py);
                if (S.lens_radius > 0) {
                    l0 = sample_dimension(S, idx, 3);
                    l1 = sample_dimension(S, idx, 4);
                }
                if (MOT) time = camera_ray_time(S, sample_dimension(S, idx, 2));
            }
            if (P.probe_mode) {
                const uint32_t probe = (pid / uint32_t(P.kc)) / (256u * uint32_t(P.probe_tiles));
                probe_ray(S, P.probe_cams[probe], float(px) + u0, float(py) + u1, &o, &d, &tmax);
                B.aux[pid] = make_float4(0, 0, 0, -1.f);  // no intersection: normal 0, NO_INTERSECTION_DISTANCE
            } else
                camera_ray<true, MOT>(S, float(px) + u0, float(py) + u1, l0, l1, &o, &d, &tmax, 0.f, time);
            if (!P.list_px && !P.probe_mode) flag_whole_film_position(B, pid, px, py, k, float(px) + u0, float(py) + u1, u0, u1);
            B.hindex[pid] = idx;
            B.L[pid] = make_float4(0, 0, 0, 0);
            if (B.nray_out) {
                B.nray_out[2 * pid] = 0;
                B.nray_out[2 * pid + 1] = 0;
            }
            ++n_cam;
        } else if (pid < P.n_paths) {
            B.L[pid] = make_float4(0, 0, 0, 0);
        }
        // queue 0 is dense (slot == pid); pixel slots outside the sample bounds are INVALID records
        if (pid < P.n_paths) {
            B.ray_o[0][pid] = make_float4(o.x, o.y, o.z, b2f(valid ? pid : kInvalid));
            B.ray_d[0][pid] = make_float4(d.x, d.y, d.z, tmax);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) B.counts[kCntRay] = P.n_paths;
    if (count_stats) flush_counter(&B.counters->camera_rays, n_cam);
}

// miss: a ray that left the scene at the first vertex or after a specular bounce picks up the
// infinite lights' radiance (path.cpp:91-99). Only launched for scenes that have one: a pass over
// the hit records of the bounce, so the traversal kernels stay as they are.
__global__ __launch_bounds__(kBlock) void k_miss(DScene S, PassBuffers B, int bounce) {
    const uint32_t count = B.counts[kCntRay + bounce];
    const float4 *ro = B.ray_o[bounce & 1], *rd = B.ray_d[bounce & 1];
    for (uint32_t slot = blockIdx.x * kBlock + threadIdx.x; slot < count; slot += gridDim.x * kBlock) {
        const float4 h4 = B.hits[slot];
        if (int(f2b(h4.x)) >= 0) continue;
        const uint32_t pid = f2b(ro[slot].w);
        if (pid == kInvalid) continue;
        const float4 d4 = rd[slot];
        // (path state rides with the ray from bounce 1 on: throughput in ray_s, specularBounce in the direction record's .w)
        const float4 beta4 = bounce == 0 ? make_float4(1, 1, 1, b2f(5u)) : B.ray_s[bounce & 1][slot];
        const uint32_t state_w = bounce == 0 ? 5u : f2b(d4.w);
        if (!((bounce == 0 && !S.probe_mode) || (bounce != 0 && (state_w >> 16) != 0))) continue;  // iispt_d.cpp:124-131
        const F3 beta = F3{beta4.x, beta4.y, beta4.z}, d = F3{d4.x, d4.y, d4.z};
        const float4 L4 = B.L[pid];
        F3 L = F3{L4.x, L4.y, L4.z};
        for (int l = 0; l < S.n_lights; ++l)
            if (S.lights[l].type == kLightInfinite) L = L + beta * inf_le(S, S.lights[l], d);
        B.L[pid] = make_float4(L.x, L.y, L.z, 0);
    }
}

// mis_lit: k_mis leaves, per record, whether its MIS ray ended on an emitting primitive (1, the hit in
// mis_hit), escaped (255) or neither (0). This pass over that byte plane turns it into "the ray reached the *sampled* light,
// on its emitting side" (`lightIsect.primitive->GetAreaLight() == &light`, then
// SurfaceInteraction::Le -> DiffuseAreaLight::L; integrator.cpp:205-209). Only the rare records
// whose ray did end on an emitter are looked at any further.
__global__ __launch_bounds__(kBlock) void k_mis_lit(DScene S, PassBuffers B, int bounce, uint32_t plane) {
    const uint32_t count = B.counts[kCntMis + bounce];
    for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < count; q += gridDim.x * kBlock) {
        const float4 n2 = B.nee[2 * size_t(plane) + q];
        const uint32_t e = f2b(n2.w);  // the NEE record of this MIS ray
        if (e == kInvalid) continue;
        const uint32_t mis = B.nee_mis[e];
        if (mis == 0) continue;
        const float4 n3 = B.nee[3 * size_t(plane) + q];
        const int li = int(f2b(n3.w));
        bool lit = false;
        if (mis == 255u) {
            lit = S.lights[li].type == kLightInfinite;  // `else Li = light.Le(ray)`, integrator.cpp:209-210
        } else {
            const float4 h4 = B.mis_hit[e];  // left by k_mis
            const int prim = int(f2b(h4.x));
            // which light the primitive is: the third word of its vertex record (the flag word says only that it is one)
            if (int(f2b(S.tri_verts[3 * size_t(prim) + 2].w)) == li)
                lit = mis_ray_lit(S, li, prim, h4.y, h4.z, h4.w, F3{n2.x, n2.y, n2.z}, F3{n3.x, n3.y, n3.z});
        }
        B.nee_mis[e] = lit ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------
// launchers
void launch_generate(const DScene &S, const PassDesc &P, const PassBuffers &B, const LaunchCfg &cfg) {
    if (cfg.camera_moves && !P.probe_mode)
        hipLaunchKernelGGL(k_generate<true>, dim3(grid_blocks(P.n_paths, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, B,
                           cfg.count_stats ? 1 : 0);
    else
        hipLaunchKernelGGL(k_generate<false>, dim3(grid_blocks(P.n_paths, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, B,
                           cfg.count_stats ? 1 : 0);
}
void launch_miss(const DScene &S, const PassBuffers &B, int bounce, uint32_t max_rays, const LaunchCfg &cfg) {
    const dim3 grid(grid_blocks(max_rays, cfg.n_cus, 8));
    hipLaunchKernelGGL(k_miss, grid, dim3(kBlock), 0, cfg.stream, S, B, bounce);
}
void launch_mis_lit(const DScene &S, const PassBuffers &B, int bounce, uint32_t max_rays, const LaunchCfg &cfg) {
    const dim3 grid(grid_blocks(max_rays, cfg.n_cus, 8));
    hipLaunchKernelGGL(k_mis_lit, grid, dim3(kBlock), 0, cfg.stream, S, B, bounce, B.queue_cap);
}

}  // namespace iile
