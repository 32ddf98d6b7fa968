// api_render.hip — the path integrator's half of the C ABI (include/iile_gpu.h): the wavefront workspace and the film
// blocks, the set-up of a frame's passes, run_pass (the schedule of the kernels in kernels*.hip), render_frame
// (SamplerIntegrator::Render around an integrator's pass: iile_render here, iile_render_ao in api_ao.hip), iile_render,
// iile_render_status and iile_li_samples.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_common.h"

using namespace iile;

namespace {

int get_events(iile_scene *sc, int kind, EventPair **out) {
    if (sc->events_used == sc->events.size()) {
        EventPair ep;
        HIP_TRY(hipEventCreate(&ep.a));
        HIP_TRY(hipEventCreate(&ep.b));
        sc->events.push_back(ep);
    }
    *out = &sc->events[sc->events_used++];
    (*out)->kind = kind;
    return IILE_OK;
}

// fn's launches between two events of `kind` on `stream` (collect_times adds them up) when the render is timed
template <typename Fn>
int timed_step(iile_scene *sc, bool timed, hipStream_t stream, int kind, Fn &&fn) {
    EventPair *ep = nullptr;
    if (timed) {
        int rc = get_events(sc, kind, &ep);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ep->a, stream));
    }
    fn();
    if (timed) HIP_TRY(hipEventRecord(ep->b, stream));
    return IILE_OK;
}

// The rank's share of SamplerIntegrator::Render's tile grid (iile_tile_owner, iile_scene.h) as two tables in HBM:
// slot -> tile (tile index order) and tile -> slot. One rank owning everything needs none (slot == tile).
int ensure_tile_map(iile_scene *sc, PassDesc *P, hipStream_t stream) {
    const int ntx = P->n_tiles_x, nty = P->n_tiles_y, n_tiles = ntx * nty, rank = P->tile_rank, nranks = P->tile_nranks;
    P->tile_of_slot = P->slot_of_tile = nullptr;
    if (nranks <= 1) {
        sc->tile_of_slot.clear();
        sc->slot_of_tile.clear();
        sc->map_key[3] = 0;
        P->n_owned_tiles = n_tiles;
        return IILE_OK;
    }
    const int key[4] = {ntx, nty, rank, nranks};
    const bool changed = std::memcmp(key, sc->map_key, sizeof(key)) != 0 || sc->slot_of_tile.size() != size_t(n_tiles);
    if (changed) {
        sc->tile_of_slot.clear();
        sc->slot_of_tile.assign(size_t(n_tiles), -1);
        for (int t = 0; t < n_tiles; ++t)
            if (iile_tile_owner(t % ntx, t / ntx, nranks) == rank) {
                sc->slot_of_tile[size_t(t)] = int(sc->tile_of_slot.size());
                sc->tile_of_slot.push_back(t);
            }
    }
    int *d_tile_of_slot = nullptr, *d_slot_of_tile = nullptr;
    auto tables = [&](Carver c) {
        d_tile_of_slot = c.take<int>(sc->tile_of_slot.size());
        d_slot_of_tile = c.take<int>(sc->slot_of_tile.size());
        return c.used;
    };
    if (const int rc = sc->tile_tables.reserve(tables(Carver()))) return rc;   // (holds unless the sharding changed)
    tables(Carver(sc->tile_tables.p));
    if (changed) {  // synchronous copies from pageable vectors: a few KB, once per change of the sharding
        HIP_TRY(hipStreamSynchronize(stream));
        if (!sc->tile_of_slot.empty())
            HIP_TRY(hipMemcpy(d_tile_of_slot, sc->tile_of_slot.data(), sc->tile_of_slot.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_slot_of_tile, sc->slot_of_tile.data(), sc->slot_of_tile.size() * sizeof(int), hipMemcpyHostToDevice));
        std::memcpy(sc->map_key, key, sizeof(key));
    }
    P->n_owned_tiles = int(sc->tile_of_slot.size());
    P->tile_of_slot = d_tile_of_slot;
    P->slot_of_tile = d_slot_of_tile;
    return IILE_OK;
}

// Room for the exact film finish (kernels_film.hip), sized from the frame: a flagged camera sample reaches at most three more
// pixels (hits), every hit becomes at most one tile sum (entries, kept for the whole render). paths_per_pass / samples_in_render
// bound the flagged samples of a pass / of the render; the flagged list itself holds kMaxFlagged records per pass.
int ensure_patch(iile_scene *sc, uint64_t paths_per_pass, uint64_t samples_in_render) {
    PatchDev &D = sc->patch;
    uint64_t want_hits = 3 * std::min<uint64_t>(kMaxFlagged, paths_per_pass);
    uint64_t want_entries = 3 * std::min<uint64_t>(kMaxFlagged, samples_in_render);
    want_hits = std::max<uint64_t>(want_hits, 4096);
    want_entries = std::max<uint64_t>(want_entries, 4096);
    if (sc->patch_cap_override) want_hits = want_entries = sc->patch_cap_override;   // iile_test_patch_capacity
    if (sc->patch_block.p && want_hits == D.cap_hits && want_entries == D.cap_entries) return IILE_OK;
    if (sc->patch_block.p && !sc->patch_cap_override && want_hits <= D.cap_hits && want_entries <= D.cap_entries) return IILE_OK;
    HIP_TRY(sc->patch_block.release());   // (a forced capacity is met exactly: the block may shrink)
    D.cap_hits = uint32_t(want_hits);
    D.cap_entries = uint32_t(want_entries);
    uint32_t table = 1024;
    while (table < 2 * D.cap_entries) table <<= 1;
    D.table_mask = table - 1;
    auto layout = [&](Carver c) {
        D.counters = c.take<uint32_t>(64);
        D.hits = c.take<uint4>(D.cap_hits);
        D.keys = c.take<uint32_t>(2 * size_t(table));   // keys, then heads: one range, cleared by one memset of 0xff (iile_render)
        D.ent_a = c.take<uint4>(D.cap_entries);
        D.ent_b = c.take<float4>(D.cap_entries);
        return c.used;
    };
    if (const int rc = sc->patch_block.reserve(layout(Carver()), 0, "out of device memory for the exact film finish")) return rc;
    layout(Carver(sc->patch_block.p));
    D.heads = D.keys + table;
    return IILE_OK;
}

// The exact film finish reports running out of room through patch.counters[2]; a render that returns before its stream has
// drained (film on the device, no statistics) cannot look. Whoever waits next does: iile_render_status, or the next iile_render.
int check_pending_overflow(iile_scene *sc) {
    if (!sc->overflow_unchecked || !sc->patch_block.p) return IILE_OK;
    HIP_TRY(hipStreamSynchronize(sc->overflow_stream));
    uint32_t pc[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(pc, sc->patch.counters, sizeof(pc), hipMemcpyDeviceToHost));
    sc->overflow_unchecked = false;
    if (pc[2] != 0)
        return api_fail(IILE_ERR_UNSUPPORTED, "the exact film finish of the previous asynchronous iile_render ran out of room (camera samples with whole-number "
                                          "film positions: more than 2^20 in one pass, or more pixel hits / tile sums than the frame was sized for): "
                                          "that film is wrong");
    return IILE_OK;
}

int collect_times(iile_scene *sc, iile_stats *st) {
    for (size_t i = 0; i < sc->events_used; ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc->events[i].a, sc->events[i].b));
        switch (sc->events[i].kind) {
        case 0: st->ms_generate += ms; break;
        case 1: st->ms_extend += ms; st->n_extend_launches++; break;
        case 2: st->ms_shade += ms; st->n_shade_launches++; break;
        case 3: st->ms_connect += ms; st->ms_shadow += ms; st->n_connect_launches++; break;
        case 5: st->ms_connect += ms; st->ms_mis += ms; break;
        case 6: st->ms_connect += ms; st->ms_resolve += ms; break;
        default: st->ms_film += ms; break;
        }
    }
    return IILE_OK;
}
}  // namespace

namespace iile {

int ensure_workspace(iile_scene *sc, uint32_t n_paths) {
    if (n_paths <= sc->ws_paths) return IILE_OK;
    sc->ws_paths = 0;
    const size_t n = n_paths;
    const size_t cap = queue_capacity(n_paths, sc->n_cus);
    PassBuffers &B = sc->pb;
    // per path: L, beta (float4), hindex, eta_scale; per queue slot: ray_o[2], ray_d[2], ray_s[2], hits, 2 x {nee[7], mis_hit}
    // (float4), shade_q, 2 x nee_mis
    auto layout = [&](Carver c) {
        B.L = c.take<float4>(n);
        B.beta = c.take<float4>(n);
        for (float4 **q : {&B.ray_o[0], &B.ray_o[1], &B.ray_d[0], &B.ray_d[1], &B.ray_s[0], &B.ray_s[1], &B.hits}) *q = c.take<float4>(cap);
        B.nee = c.take<float4>(7 * cap);
        B.mis_hit = c.take<float4>(cap);
        B.nee_alt = c.take<float4>(7 * cap);
        B.mis_hit_alt = c.take<float4>(cap);
        B.nee_mis_alt = c.take<uint8_t>(cap);
        B.hindex = c.take<uint32_t>(n);
        B.eta_scale = c.take<float>(n);
        B.shade_q = c.take<uint32_t>(cap);
        B.nee_mis = c.take<uint8_t>(cap);
        B.counts = c.take<uint32_t>(kCntWords);
        B.counters = c.take<DCounters>(1);
        return c.used;
    };
    const size_t bytes = layout(Carver());
    const auto t_alloc = std::chrono::steady_clock::now();
    if (const int rc = sc->ws_block.reserve(bytes)) return rc;
    if (std::getenv("IILE_TIMING"))   // (a fresh process's large allocation can wait seconds for memory another process has just freed)
        fprintf(stderr, "iile timing: workspace of %.1f GiB for %u paths allocated in %.3f s\n", double(bytes) / 1073741824.0, n_paths,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t_alloc).count());
    layout(Carver(sc->ws_block.p));
    B.queue_cap = uint32_t(cap);
    B.nray_out = nullptr;
    B.spill = sc->spill;
    sc->ws_paths = n_paths;
    return IILE_OK;
}

int ensure_film(iile_scene *sc, uint32_t n_tiles, uint32_t n_pixels, uint64_t n_wide) {
    if (n_wide > sc->film_wide) {  // the frame's samples for a wide pixel filter: 24 B each
        sc->film_wide = 0;
        auto wide = [&](Carver c) {
            sc->fb.wide_L = c.take<float4>(n_wide);
            sc->fb.wide_pf = c.take<float2>(n_wide);
            return c.used;
        };
        if (const int rc = sc->wide_block.reserve(wide(Carver()), 0, "out of device memory for the sample store of a wide pixel filter (24 B per camera sample)"))
            return rc;
        wide(Carver(sc->wide_block.p));
        sc->film_wide = n_wide;
    }
    if (n_tiles <= sc->film_tiles && n_pixels <= sc->film_pixels) return IILE_OK;
    n_tiles = std::max(n_tiles, sc->film_tiles);
    n_pixels = std::max(n_pixels, sc->film_pixels);
    sc->film_tiles = sc->film_pixels = 0;
    auto film = [&](Carver c) {
        // the two tile planes are one range: k0_rgbv starts film_tiles * 256 records behind tile_rgbw
        sc->fb.tile_rgbw = c.take<float4>(2 * size_t(n_tiles) * 256);
        sc->fb.film_xyzw = c.take<float4>(n_pixels);
        return c.used;
    };
    if (const int rc = sc->film_block.reserve(film(Carver()))) return rc;
    film(Carver(sc->film_block.p));
    sc->fb.k0_rgbv = sc->fb.tile_rgbw + size_t(n_tiles) * 256;
    sc->film_tiles = n_tiles;
    sc->film_pixels = n_pixels;
    return IILE_OK;
}

int frame_pass(iile_scene *sc, const DScene &S, int rank, int nranks, hipStream_t stream, PassDesc *P) {
    std::memset(P, 0, sizeof(*P));
    P->n_tiles_x = (S.samp_x1 - S.samp_x0 + 15) / 16;
    P->n_tiles_y = (S.samp_y1 - S.samp_y0 + 15) / 16;
    P->tile_rank = rank, P->tile_nranks = nranks;
    return ensure_tile_map(sc, P, stream);
}

uint64_t path_budget(double bytes_per_path) {
    double budget_mb = 65536;  // 64 GiB of the 288 GB: one pass covers 1080p x 64 spp
    if (const char *e = std::getenv("IILE_WORKSPACE_MB")) budget_mb = std::max(64.0, atof(e));
    return std::min<uint64_t>(uint64_t(budget_mb * 1048576.0 / bytes_per_path), kMaxPassPaths);
}

void copy_counters(const DCounters &c, iile_stats *st) {
    st->camera_rays = c.camera_rays;
    st->closest_rays = c.closest_rays;
    st->shadow_rays = c.shadow_rays;
    st->nodes_closest = c.nodes_closest;
    st->nodes_any = c.nodes_any;
    st->tri_tests = c.tri_tests;
    st->tri_hits = c.tri_hits;
    st->sphere_tests = c.sphere_tests;
    st->nee_evals = c.nee_evals;
    st->zero_radiance = c.zero_radiance;
    for (int i = 0; i < 8; ++i) st->path_length[i] = c.path_length[i];
    st->ext_rays = c.ext_rays;
    st->ext_nodes = c.ext_nodes;
    st->ext_tri_tests = c.ext_tri_tests;
    st->ext_sphere_tests = c.ext_sphere_tests;
    st->any_tri_tests = c.any_tri_tests;
    st->mis_rays_traced = c.mis_traced;
    st->ext_rays_traced = c.ext_traced;
}

// Enqueue one wavefront pass on cfg.stream.
int run_pass(iile_scene *sc, const DScene &S_in, int max_depth, const PassDesc &P_in, const LaunchCfg &cfg, bool timed, bool one_stream) {
    PassBuffers &B = sc->pb;
    PassDesc P = P_in;
    // The scene's sample table serves the plain frame passes: the instrumented pass, listed samples and samples past the
    // scene's own spp keep the digit chains (a probe pass's copy of the scene arrives without the table).
    DScene S = S_in;
    if (cfg.count_stats || P.list_px || S.probe_mode || P.k0 < 0 || uint64_t(P.k0) + uint64_t(P.kc) > uint64_t(S.stab_spp) || max_depth > S.max_depth)
        clear_sample_table(&S);
    // camera rays made inside the first extend / shade (see PassDesc::gen_fused) where nothing else reads queue 0
    P.gen_fused = !cfg.count_stats && !P.list_px && !S.has_infinite && !S.probe_mode && !B.nray_out && !S.env_camera && !cfg.camera_moves;  // (camera_ray<false>)
    HIP_TRY(hipMemsetAsync(B.counts, 0, kCntWords * sizeof(uint32_t), cfg.stream));
    auto timed_launch_on = [&](hipStream_t stream, int kind, auto &&fn) -> int { return timed_step(sc, timed, stream, kind, fn); };
    auto timed_launch = [&](int kind, auto &&fn) -> int { return timed_launch_on(cfg.stream, kind, fn); };
    // Two streams: the shadow / MIS rays of bounce b and the extension rays of bounce b + 1 both hang on k_shade of bounce
    // b and on nothing else of each other (k_shadow accumulates into L, k_extend reads the ray queue), so they run side
    // by side and each fills the idle compute units of the other's tail; k_shade of bounce b + 1 waits for both (it
    // overwrites the NEE records, and may add emitted light to L after the NEE contribution of bounce b as path.cpp
    // does). Not with infinite lights (k_miss adds to L between the two) and not in the instrumented pass.
    const bool two_streams = sc->nee_stream && !one_stream && !cfg.count_stats && !S.has_infinite && max_depth < 15;
    // Without specular lobes k_shade touches L at bounce 0 only, and with the NEE arrays doubled (even / odd bounces) it
    // need not wait for k_shadow of the bounce before: the NEE stream then trails the main one by up to a bounce.
    const bool nee_doubled = two_streams && !S.has_specular && B.nee_alt;
    LaunchCfg cfg_nee = cfg;
    if (two_streams) cfg_nee.stream = sc->nee_stream;
    auto buffers_of = [&](int bounce, bool nee_side) {
        PassBuffers X = B;
        if (nee_doubled && (bounce & 1)) X.nee = B.nee_alt, X.mis_hit = B.mis_hit_alt, X.nee_mis = B.nee_mis_alt;
        if (two_streams && nee_side) X.spill = sc->spill_nee;
        return X;
    };
    int rc = IILE_OK;
    if (P.gen_fused) {
        // no k_generate: queue 0 is the dense range of path ids (and the first k_extend zeroes each path's L)
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&B.counts[0]), int(P.n_paths), 1, cfg.stream));
    } else {
        rc = timed_launch(0, [&] { launch_generate(S, P, B, cfg); });
        if (rc) return rc;
    }
    // bounces 0 .. maxDepth: the path loop exits at `bounces >= maxDepth` after
    // intersecting (path.cpp:104), so maxDepth + 1 extend launches are needed — to reproduce the reference's ray count.
    // The radiance does not need the last of them unless a specular bounce or an infinite light can add emitted light
    // at that vertex (path.cpp:91-101): the uninstrumented pass of a scene with neither leaves the bounce out.
    // With specular lobes (or an infinite light) around, the rays that leave the last shaded vertex through a specular
    // lobe are the only ones whose intersection can still add something: the others are dropped there (1); without
    // either, the whole bounce is (2).
    P.skip_last_bounce = 0;
    if (!cfg.count_stats && max_depth >= 1 && !S.probe_mode && !B.nray_out)
        P.skip_last_bounce = S.has_specular ? 1 : 2;
    const int last_bounce = (P.skip_last_bounce == 2) ? max_depth - 1 : max_depth;
    for (int b = 0; b <= last_bounce; ++b) {
        rc = timed_launch(1, [&] { launch_extend(S, P, B, b, B.queue_cap, cfg); });
        if (rc) return rc;
        if (S.has_infinite) {  // escaped rays see the infinite lights (path.cpp:97-99)
            rc = timed_launch(6, [&] { launch_miss(S, B, b, B.queue_cap, cfg); });
            if (rc) return rc;
        }
        if (two_streams && !nee_doubled && b > 0) HIP_TRY(hipStreamWaitEvent(cfg.stream, sc->ev_nee[b - 1], 0));
        if (nee_doubled && b > 1) HIP_TRY(hipStreamWaitEvent(cfg.stream, sc->ev_nee[b - 2], 0));  // its records are overwritten now
        const PassBuffers B_shade = buffers_of(b, false), B_nee = buffers_of(b, true);
        rc = timed_launch(2, [&] { launch_shade(S, P, B_shade, b, B.queue_cap, cfg); });
        if (rc) return rc;
        if (b < max_depth) {
            if (two_streams) {
                HIP_TRY(hipEventRecord(sc->ev_shade[b], cfg.stream));
                HIP_TRY(hipStreamWaitEvent(cfg_nee.stream, sc->ev_shade[b], 0));
            }
            // MIS rays first: the shadow kernel finishes each record (L += beta * Ld)
            rc = timed_launch_on(cfg_nee.stream, 5, [&] { launch_mis(S, B_nee, b, B.queue_cap, cfg_nee); });
            if (rc) return rc;
            rc = timed_launch_on(cfg_nee.stream, 6, [&] { launch_mis_lit(S, B_nee, b, B.queue_cap, cfg_nee); });
            if (rc) return rc;
            rc = timed_launch_on(cfg_nee.stream, 3, [&] { launch_shadow(S, B_nee, b, B.queue_cap, cfg_nee); });
            if (rc) return rc;
            if (two_streams) HIP_TRY(hipEventRecord(sc->ev_nee[b], cfg_nee.stream));
        }
    }
    if (two_streams && max_depth > 0) HIP_TRY(hipStreamWaitEvent(cfg.stream, sc->ev_nee[max_depth - 1], 0));
    HIP_TRY(hipGetLastError());
    return IILE_OK;
}

// SamplerIntegrator::Render (integrator.cpp:227-331) around the Li of `fi`: the tile loop over the rank's share, pixel bounds,
// radiance guards, the film with its filter tables and the exact finish. iile_render and iile_render_ao are this with their own pass.
int render_frame(iile_scene *sc, const iile_render_params *prm, float *film_xyzw, iile_stats *stats, const FrameIntegrator &fi) {
    int rc = check_pending_overflow(sc);   // of an earlier render that returned before its stream had drained
    if (rc) return rc;
    const DScene &S = sc->ds;
    int k_begin = prm->k_begin, k_end = prm->k_end;
    if (k_end <= 0) {
        k_begin = 0;
        k_end = sc->spp;
    }
    if (k_begin < 0 || k_begin >= k_end) return api_fail(IILE_ERR_ARG, "iile_render: empty sample range");
    int rank = prm->tile_rank, nranks = prm->tile_nranks;
    if (nranks <= 0) {
        rank = 0;
        nranks = 1;
    }
    if (rank < 0 || rank >= nranks) return api_fail(IILE_ERR_ARG, "iile_render: tile_rank out of range");
    hipStream_t stream = static_cast<hipStream_t>(prm->stream);
    LaunchCfg cfg{sc->n_cus, stream, prm->collect_stats != 0};
    cfg.camera_moves = sc->camera_moves;
    const bool timed = prm->time_kernels != 0;

    PassDesc P;
    rc = frame_pass(sc, S, rank, nranks, stream, &P);
    if (rc) return rc;
    const uint64_t pix_slots = uint64_t(P.n_owned_tiles) * 256;
    const int n_samples = k_end - k_begin;
    // A pass renders all samples of a range of owned tiles; the range is bounded by the workspace budget (~410 B per
    // path incl. queue padding). `spp_per_pass` (tests) asks for passes of about that many samples per pixel's worth
    // of paths: n_owned_tiles * spp_per_pass / n_samples tiles each.
    uint64_t max_paths = std::min<uint64_t>(path_budget(fi.bytes_per_path), fi.max_pass_paths);
    if (prm->spp_per_pass > 0) max_paths = std::min<uint64_t>(max_paths, std::max<uint64_t>(1, pix_slots * uint64_t(prm->spp_per_pass)));
    const uint64_t paths_per_tile = uint64_t(256) * uint64_t(n_samples);
    if (paths_per_tile > kMaxPassPaths) return api_fail(IILE_ERR_UNSUPPORTED, "more than 781 250 samples per pixel in one render: split the sample range");
    if (paths_per_tile > fi.max_pass_paths) return api_fail(IILE_ERR_UNSUPPORTED, fi.too_many);
    const int tiles_per_pass = int(std::max<uint64_t>(1, std::min<uint64_t>(uint64_t(std::max(P.n_owned_tiles, 1)), max_paths / paths_per_tile)));
    const uint32_t fw = uint32_t(S.crop_x1 - S.crop_x0), fh = uint32_t(S.crop_y1 - S.crop_y0);

    if (pix_slots) {
        rc = ensure_workspace(sc, uint32_t(uint64_t(tiles_per_pass) * paths_per_tile));
        if (rc) return rc;
        if (fi.reserve && (rc = fi.reserve(sc, uint32_t(uint64_t(tiles_per_pass) * paths_per_tile), fi.ctx))) return rc;
    }
    rc = ensure_film(sc, uint32_t(P.n_owned_tiles), fw * fh, S.filter_wide ? pix_slots * uint64_t(n_samples) : 0);
    if (rc) return rc;
    sc->pb.nray_out = nullptr;
    sc->events_used = 0;
    iile_stats st;
    std::memset(&st, 0, sizeof(st));
    // whole-number film positions are listed for the one-pixel box film (the sample store of wider filters handles them).
    // Their exact finish runs on the device, on this stream, without a host wait (kernels_film.hip "exact film finish").
    if (!S.filter_wide) {
        rc = ensure_patch(sc, uint64_t(tiles_per_pass) * paths_per_tile, uint64_t(P.n_owned_tiles) * paths_per_tile);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(sc->patch.counters, 0, 16, stream));
    }
    const size_t patch_table_bytes = (size_t(sc->patch.table_mask) + 1) * 8;  // keys, then heads: one memset of 0xff
    sc->pb.flag_count = S.filter_wide ? nullptr : sc->flag_count;
    sc->pb.flag_rec = sc->flag_rec;
    struct FlagGuard {  // error returns below must not leave the list armed for the kernel-level entry points
        PassBuffers *pb;
        ~FlagGuard() { pb->flag_count = nullptr; }
    } flag_guard{&sc->pb};

    HIP_TRY(hipEventRecord(sc->ev_begin, stream));
    if (pix_slots) HIP_TRY(hipMemsetAsync(sc->pb.counters, 0, sizeof(DCounters), stream));
    // (the two planes are sized for the largest share this scene has rendered: k0_rgbv starts film_tiles * 256 records behind tile_rgbw,
    //  not pix_slots — each is cleared where it lies; a pixel outside "pixelbounds" keeps these zeros)
    if (pix_slots) HIP_TRY(hipMemsetAsync(sc->fb.tile_rgbw, 0, size_t(pix_slots) * sizeof(float4), stream));
    if (pix_slots) HIP_TRY(hipMemsetAsync(sc->fb.k0_rgbv, 0, size_t(pix_slots) * sizeof(float4), stream));
    P.k0 = k_begin;
    P.kc = n_samples;
    for (int slot0 = 0; slot0 < P.n_owned_tiles; slot0 += tiles_per_pass) {
        P.slot0 = slot0;
        P.n_pass_tiles = std::min(tiles_per_pass, P.n_owned_tiles - slot0);
        P.n_paths = uint32_t(uint64_t(P.n_pass_tiles) * paths_per_tile);
        if (sc->pb.flag_count) HIP_TRY(hipMemsetAsync(sc->flag_count, 0, sizeof(uint32_t), stream));
        rc = fi.run(sc, S, P, cfg, timed, prm->time_kernels == 2, fi.ctx);
        if (rc) return rc;
        rc = timed_step(sc, timed, stream, 4, [&] {
            if (S.filter_wide)
                launch_film_store(S, P, sc->pb, sc->fb, k_begin, n_samples, cfg);
            else
                launch_film_accumulate(S, P, sc->pb, sc->fb, cfg);
        });
        if (rc) return rc;
        if (sc->pb.flag_count) {
            // this pass's flagged samples -> exact FilmTile sums (entries) for the pixels they reach
            HIP_TRY(hipMemsetAsync(sc->patch.counters, 0, sizeof(uint32_t), stream));  // hits are per pass; entries add up
            HIP_TRY(hipMemsetAsync(sc->patch.keys, 0xff, patch_table_bytes, stream));
            launch_patch_pass(S, P, sc->pb, sc->fb, sc->patch, cfg);
        }
        st.n_passes++;
        st.n_paths += P.n_paths;
    }
    FilmBuffers F = sc->fb;
    if (prm->film_on_device) F.film_xyzw = reinterpret_cast<float4 *>(film_xyzw);
    if (S.filter_wide) {
        rc = timed_step(sc, timed, stream, 4, [&] { launch_film_gather(S, P, F, n_samples, cfg); });  // counted with the film kernels (ms_film)
        if (rc) return rc;
    } else {
        launch_film_resolve(S, P, F, cfg);
        HIP_TRY(hipGetLastError());
        if (sc->pb.flag_count && pix_slots) {
            HIP_TRY(hipMemsetAsync(sc->patch.keys, 0xff, patch_table_bytes, stream));
            launch_patch_merge(S, P, F, sc->patch, cfg);
            HIP_TRY(hipGetLastError());
        }
    }
    sc->pb.flag_count = nullptr;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc->ev_end, stream));
    if (!prm->film_on_device) {
        HIP_TRY(hipMemcpyAsync(film_xyzw, F.film_xyzw, size_t(fw) * fh * sizeof(float4), hipMemcpyDeviceToHost, stream));
    }
    // The film is complete once the stream drains. Statistics need the drain; a device-resident film without stats
    // stays asynchronous on `stream` past the last pass (the exact film finish waits for each pass on that stream, and
    // only on it: nothing here touches the null stream or synchronises the device).
    if (!(stats || !prm->film_on_device) && pix_slots && !S.filter_wide) {
        sc->overflow_unchecked = true;   // nobody waits here: iile_render_status / the next iile_render reads the error word
        sc->overflow_stream = stream;
    }
    if (stats || !prm->film_on_device) {
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev_begin, sc->ev_end));
        st.ms_total = ms;
        if (timed) {
            rc = collect_times(sc, &st);
            if (rc) return rc;
        }
        if (pix_slots && !S.filter_wide) {  // did the exact film finish run out of room? (checked wherever the host waits anyway)
            uint32_t pc[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpyAsync(pc, sc->patch.counters, sizeof(pc), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (pc[2] != 0)
                return api_fail(IILE_ERR_UNSUPPORTED, "the exact film finish ran out of room (camera samples with whole-number film positions: more than "
                                                  "2^20 in one pass, or more pixel hits / tile sums than the frame was sized for)");
        }
        if (pix_slots) {
            DCounters c;
            HIP_TRY(hipMemcpyAsync(&c, sc->pb.counters, sizeof(c), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (prm->collect_stats)
                copy_counters(c, &st);
            else
                st.mis_rays_traced = c.mis_traced, st.ext_rays_traced = c.ext_traced;
#if defined(IILE_SHADE_STAMPS) || defined(IILE_TRAV_STAMPS) || defined(IILE_SHADOW_STAMPS) || defined(IILE_TRAV_ITERSTATS)
            // diagnostic builds (tools/shade_stamps.py, tools/trav_stamps.py): per-section wave cycles ride out in the path-length histogram
            if (!prm->collect_stats)
                for (int i = 0; i < 8; ++i) st.path_length[i] = c.path_length[i];
#endif
        }
        st.workspace_bytes = sc->ws_block.cap;
        if (stats) *stats = st;
    }
    return IILE_OK;
}
}  // namespace iile

extern "C" {
int iile_render(iile_scene *sc, const iile_render_params *prm, float *film_xyzw, iile_stats *stats) {
    if (!sc || !prm || !film_xyzw) return api_fail(IILE_ERR_ARG, "iile_render: null argument");
    const int rc = ensure_device();
    if (rc) return rc;
    // PathIntegrator::Li: ~410 B of workspace per path incl. queue padding
    static const FrameIntegrator path = {410.0, kMaxPassPaths, "", nullptr,
                                         [](iile_scene *s, const DScene &S, const PassDesc &P, const LaunchCfg &cfg, bool timed, bool one_stream, void *) {
                                             return run_pass(s, S, s->max_depth, P, cfg, timed, one_stream);
                                         },
                                         nullptr};
    return render_frame(sc, prm, film_xyzw, stats, path);
}
int iile_render_status(iile_scene *sc, void *stream) {
    if (!sc) return api_fail(IILE_ERR_ARG, "iile_render_status: null scene");
    int rc = ensure_device();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return check_pending_overflow(sc);
}

int iile_test_patch_capacity(iile_scene *sc, uint32_t capacity) {
    if (!sc) return api_fail(IILE_ERR_ARG, "iile_test_patch_capacity: null scene");
    sc->patch_cap_override = capacity;
    return IILE_OK;
}

int iile_li_samples(iile_scene *sc, int32_t n, const int32_t *px, const int32_t *py, const int32_t *k, float *L3,
                    int32_t *nrays2) {
    if (!sc || n <= 0 || !px || !py || !k || !L3) return api_fail(IILE_ERR_ARG, "iile_li_samples: bad argument");
    int rc = ensure_device();
    if (rc) return rc;
    DevBuf<int> dx, dy, dk;
    DevBuf<uint32_t> dn;
    if ((rc = dx.put(px, n)) || (rc = dy.put(py, n)) || (rc = dk.put(k, n)) || (rc = dn.alloc(2 * size_t(n)))) return rc;
    rc = ensure_workspace(sc, uint32_t(n));
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
    sc->events_used = 0;
    rc = run_pass(sc, sc->ds, sc->max_depth, P, cfg, false);
    sc->pb.nray_out = nullptr;
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float4> L(n);
    HIP_TRY(hipMemcpy(L.data(), sc->pb.L, size_t(n) * sizeof(float4), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        // guards of SamplerIntegrator::Render (integrator.cpp:293-314)
        float r = L[i].x, g = L[i].y, b = L[i].z;
        float y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
        if (std::isnan(r) || std::isnan(g) || std::isnan(b) || y < -1e-5 || std::isinf(y)) r = g = b = 0.f;
        L3[3 * i] = r;
        L3[3 * i + 1] = g;
        L3[3 * i + 2] = b;
    }
    if (nrays2) {
        std::vector<uint32_t> nr(2 * size_t(n));
        if ((rc = dn.get(nr.data(), nr.size()))) return rc;
        for (size_t i = 0; i < nr.size(); ++i) nrays2[i] = int32_t(nr[i]);
    }
    return IILE_OK;
}

}  // extern "C"
