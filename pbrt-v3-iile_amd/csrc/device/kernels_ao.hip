// kernels_ao.hip — the ambient occlusion integrator (AOIntegrator::Li, src/integrators/ao.cpp:57-103) on the wavefront pipeline.
//
// Pipeline per pass:  generate -> extend (bounce 0) -> ao_rays -> ao_occlude -> ao_fold -> the film kernels of iile_render
//   generate, extend   as the path integrator runs them: the camera rays and their closest hits (kernels.hip, kernels_trav.hip)
//   ao_rays            per hit the frame of ao.cpp:77-79 from the geometric interaction, then the nSamples rays of the sampler's
//                      2D array (dpath.h: sample_array_2d), queued path-major: ray = hit * nSamples + j, so a wavefront's lanes
//                      share one or a few origins
//   ao_occlude         BVHAccel::IntersectP over that queue — the shared wave step of dtrav.h, any-hit, as k_shadow is built
//                      from it — one visibility byte per ray
//   ao_fold            per hit, L = the sum over j = 0 .. nSamples - 1, in that order, of the unoccluded rays' terms: one thread
//                      owns one path, so there is no float atomic and the film does not depend on pass sizes
// The null-BSDF retry of ao.cpp:69-73 is left out: the loader knows no "none" material, so ComputeScatteringFunctions always
// yields a BSDF and the branch is dead. The interaction is read for its geometry alone: no material, no light.
#include "kcommon.h"

namespace iile {

namespace {
// a hit's record in LDS between the two halves of k_ao_rays: p, pError, isect.n, s, t, n (face-forwarded), then px, py, k
constexpr int kAoFrameWords = 21;  // (odd: neighbouring records start on different banks)
}  // namespace

__global__ __launch_bounds__(kBlock) void k_ao_rays(DScene S, PassDesc P, PassBuffers B, AoBuffers A) {
    __shared__ float frames[kWavesPerBlock][64 * kAoFrameWords];
    float *wf = frames[threadIdx.x >> 6];
    const uint32_t count = B.counts[kCntShade];  // the shade queue of bounce 0: reserved slots, the unused ones INVALID
    const uint32_t n_s = uint32_t(A.n_samples);
    const float4 *ro = B.ray_o[0], *rd = B.ray_d[0];
    // (whole blocks step together: the two barriers below are reached by every thread the same number of times)
    for (uint32_t base = blockIdx.x * kBlock; base < count; base += gridDim.x * kBlock) {
        const uint32_t e = base + threadIdx.x;
        const uint32_t entry = e < count ? B.shade_q[e] : kInvalid;
        const bool valid = entry != kInvalid;
        // the wavefront's hits take consecutive hit numbers: one atomic per wavefront
        const unsigned long long mask = __ballot(valid);
        const uint32_t n_valid = uint32_t(__popcll(mask)), rank = lanes_below(mask);
        uint32_t h0 = 0;
        if (n_valid) {
            const int leader = __ffsll((long long)mask) - 1;
            if (lane_id() == leader) h0 = atomicAdd(&B.counts[kCntAoHits], n_valid);
            h0 = __shfl(h0, leader);
        }
        if (valid) {
            const uint32_t slot = entry & ((1u << kSlotBits) - 1u);
            const float4 o4 = ro[slot], d4 = rd[slot], h4 = B.hits[slot];
            const uint32_t pid = f2b(o4.w);
            const int prim = int(f2b(h4.x));
            const F3 ray_o = F3{o4.x, o4.y, o4.z}, ray_d = F3{d4.x, d4.y, d4.z};
            const float4 v0 = S.tri_verts[3 * size_t(prim)], v1 = S.tri_verts[3 * size_t(prim) + 1], v2 = S.tri_verts[3 * size_t(prim) + 2];
            const uint32_t flags = f2b(v0.w);
            Isect is;
            if (flags & 1u)  // a sphere, a disk or a cylinder, with its geometric dp/du (DIFFS)
                shape_hit_interaction<true>(S, S.prim_shape[prim], ray_o, ray_d, &is);
            else
                triangle_interaction(S, prim, flags, F3{v0.x, v0.y, v0.z}, F3{v1.x, v1.y, v1.z}, F3{v2.x, v2.y, v2.z}, ray_d, h4.y, h4.z, h4.w, &is);
            // "Compute coordinate frame based on true geometry, not shading geometry" (ao.cpp:75-79): isect.n and isect.dpdu, not
            // shading.n / shading.dpdu. t is Cross(isect.n, s) with the normal that is NOT face-forwarded, while wi is built on the
            // face-forwarded one: where the ray meets the back of a surface the frame (s, t, n) is left-handed. The reference has it
            // that way — the map stays a hemisphere about n — and it is reproduced.
            const F3 n = faceforward(is.n, -ray_d);
            const F3 s = normalize(is.dpdu);
            const F3 t = cross(is.n, s);
            int px = 0, py = 0;
            uint32_t k = 0;
            path_pixel(S, P, pid, &px, &py, &k);
            float *f = wf + rank * kAoFrameWords;
            f[0] = is.p.x, f[1] = is.p.y, f[2] = is.p.z;
            f[3] = is.perr.x, f[4] = is.perr.y, f[5] = is.perr.z;
            f[6] = is.n.x, f[7] = is.n.y, f[8] = is.n.z;
            f[9] = s.x, f[10] = s.y, f[11] = s.z;
            f[12] = t.x, f[13] = t.y, f[14] = t.z;
            f[15] = n.x, f[16] = n.y, f[17] = n.z;
            f[18] = b2f(uint32_t(px)), f[19] = b2f(uint32_t(py)), f[20] = b2f(k);
            A.hit_pid[h0 + rank] = pid;
        }
        __syncthreads();
        // the wavefront's n_valid * nSamples rays, consecutive lanes -> consecutive rays of (mostly) one hit
        const uint32_t n_rays = n_valid * n_s;
        for (uint32_t r = uint32_t(lane_id()); r < n_rays; r += 64u) {
            const uint32_t local = r / n_s, j = r - local * n_s;
            const float *f = wf + local * kAoFrameWords;
            const F3 p = F3{f[0], f[1], f[2]}, perr = F3{f[3], f[4], f[5]}, ng = F3{f[6], f[7], f[8]};
            const F3 s = F3{f[9], f[10], f[11]}, t = F3{f[12], f[13], f[14]}, n = F3{f[15], f[16], f[17]};
            const int px = int(f2b(f[18])), py = int(f2b(f[19]));
            const uint32_t k = f2b(f[20]);
            float u0, u1;
            sample_array_2d(S, px, py, k, n_s, j, 5, &u0, &u1);  // `sampler.Get2DArray(nSamples)[j]`: the integrator's only array
            F3 wl;
            float pdf;
            if (A.cos_sample) {
                wl = cosine_sample_hemisphere(u0, u1);
                pdf = fabsf(wl.z) * kInvPi;  // CosineHemispherePdf(std::abs(wi.z)), sampling.h:165
            } else {
                wl = uniform_sample_hemisphere(u0, u1);
                pdf = kInv2Pi;  // UniformHemispherePdf()
            }
            // "Transform wi from local frame to world space." (ao.cpp:93-96)
            const F3 wi = F3{s.x * wl.x + t.x * wl.y + n.x * wl.z, s.y * wl.x + t.y * wl.y + n.y * wl.z, s.z * wl.x + t.z * wl.y + n.z * wl.z};
            const F3 o = offset_ray_origin(p, perr, ng, wi);  // isect.SpawnRay(wi), interaction.h:72-75
            const size_t ray = size_t(h0) * n_s + r;
            A.ray_o[ray] = make_float4(o.x, o.y, o.z, 0.f);
            A.ray_d[ray] = make_float4(wi.x, wi.y, wi.z, IILE_INF);
            A.term[ray] = dot(wi, n) / (pdf * float(A.n_samples));  // `L += Dot(wi, n) / (pdf * nSamples)`, ao.cpp:99
        }
        __syncthreads();
    }
}

// BVHAccel::IntersectP for every ray of the pass (`scene.IntersectP(isect.SpawnRay(wi))`, ao.cpp:98): k_shadow's loop without its
// NEE record — a lane that finishes stores one byte.
template <bool COUNT, bool ALPHA>
__global__ __launch_bounds__(kTravBlock, IILE_TRAV_WAVES) void k_ao_occlude(DScene S, PassBuffers B, AoBuffers A) {
    const StackRef sr = trav_block_begin<COUNT, kTravBlock>(S, B.spill);
    const uint32_t count = B.counts[kCntAoHits] * uint32_t(A.n_samples);  // (< 2^32: the pass was sized so)
    uint32_t *head = &B.counts[kCntAoHead];
    TraceStats st = {0, 0, 0, 0};
    unsigned long long n_rays = 0;
    WaveFeed feed{0, 0, count == 0};
    Trav t;  // (an idle lane)
    bool active = false, occluded = false;
    uint32_t r = 0;
    while (true) {
        const unsigned long long idle_mask = __ballot(!active);
        if (refill_due(idle_mask, feed, kRefillIdle)) {
            uint32_t r_new;
            if (feed_take(feed, head, count, !active, &r_new, [&](uint32_t first) {
                    warm_plane(A.ray_o, first, count);
                    warm_plane(A.ray_d, first, count);
                })) {
                r = r_new;
                const float4 o4 = A.ray_o[r], d4 = A.ray_d[r];
                trav_begin<COUNT>(S, t, F3{o4.x, o4.y, o4.z}, F3{d4.x, d4.y, d4.z}, d4.w, &st, sr.root);
                active = true;
                occluded = false;
                ++n_rays;
            }
        }
        if (__ballot(active) == 0) {
            if (feed.exhausted) break;
            continue;
        }
        const WaveStep ws = trav_wave_step<COUNT, ALPHA, true>(S, active, t, sr, &st, true, &A.ray_d[r]);
        if (ws.hit) occluded = true;
        if (active && !t.have) {
            A.vis[r] = occluded ? 0 : 1;
            active = false;
        }
    }
    if (COUNT) {
        flush_counter(&B.counters->shadow_rays, n_rays);
        flush_counter(&B.counters->nodes_any, st.nodes);
        flush_counter(&B.counters->any_tri_tests, st.tris);
        flush_counter(&B.counters->tri_tests, st.tris);
        flush_counter(&B.counters->tri_hits, st.tri_hits);
        flush_counter(&B.counters->sphere_tests, st.spheres);
    }
}

// `for (int i = 0; i < nSamples; ++i) if (!scene.IntersectP(..)) L += ..` (ao.cpp:82-100): one thread per hit adds its rays' terms
// in i order; L is a Spectrum built from one Float, the same in every channel. A camera ray that found nothing keeps the L = 0
// k_generate gave it.
__global__ __launch_bounds__(kBlock) void k_ao_fold(PassBuffers B, AoBuffers A) {
    const uint32_t n_hits = B.counts[kCntAoHits], n_s = uint32_t(A.n_samples);
    for (uint32_t h = blockIdx.x * kBlock + threadIdx.x; h < n_hits; h += gridDim.x * kBlock) {
        const size_t first = size_t(h) * n_s;
        float L = 0.f;
        for (uint32_t j = 0; j < n_s; ++j)
            if (A.vis[first + j]) L += A.term[first + j];
        const uint32_t pid = A.hit_pid[h];
        B.L[pid] = make_float4(L, L, L, 0.f);
        if (B.nray_out) B.nray_out[2 * pid + 1] = n_s;
    }
}

// kernel-level probe: entry j[i] of the 2D array of pixel sample k[i]
__global__ void k_ao_array_probe(DScene S, int n_samples, int n, const int *px, const int *py, const int *k, const int *j, float *out2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sample_array_2d(S, px[i], py[i], uint32_t(k[i]), uint32_t(n_samples), uint32_t(j[i]), 5, &out2[2 * i], &out2[2 * i + 1]);
}

// ---------------------------------------------------------------------------
// launchers
void launch_ao_rays(const DScene &S, const PassDesc &P, const PassBuffers &B, const AoBuffers &A, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_ao_rays, dim3(grid_blocks(B.queue_cap, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, B, A);
}
void launch_ao_occlude(const DScene &S, const PassBuffers &B, const AoBuffers &A, uint32_t max_rays, const LaunchCfg &cfg) {
    // (count_stats: the instrumented build, always with ALPHA; rare_prims: the ALPHA build — as launch_shadow)
    using K = void (*)(DScene, PassBuffers, AoBuffers);
    const K k = cfg.count_stats ? k_ao_occlude<true, true> : S.rare_prims ? k_ao_occlude<false, true> : k_ao_occlude<false, false>;
    const int per_cu256 = cfg.trav_blocks_per_cu > 0 ? cfg.trav_blocks_per_cu : default_trav_blocks_per_cu();
    const dim3 grid(grid_blocks(max_rays, cfg.n_cus, std::max(1, per_cu256 * kBlock / kTravBlock), kTravBlock));
    hipLaunchKernelGGL(k, grid, dim3(kTravBlock), 0, cfg.stream, S, B, A);
}
void launch_ao_fold(const PassDesc &P, const PassBuffers &B, const AoBuffers &A, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_ao_fold, dim3(grid_blocks(P.n_paths, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, B, A);
}
void launch_ao_array_probe(const DScene &S, int n_samples, int n, const int *px, const int *py, const int *k, const int *j, float *out2,
                           const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_ao_array_probe, dim3((n + 255) / 256), dim3(256), 0, cfg.stream, S, n_samples, n, px, py, k, j, out2);
}

}  // namespace iile
