// kernels_film.hip — the film kernels and their launchers (the steps they share: dfilm.h).
//   the one-pixel box film   k_film_accumulate per pass, k_film_resolve after the last one
//   filters wider than that  k_film_store per pass, k_film_gather after the last one
//   the probe films          k_probe_film (k_film_store + k_film_gather + k_probe_finish for films that fit LDS),
//                            k_probe_film_add / k_probe_film_resolve (the accumulating film of the reference mode)
//   the exact film finish    k_patch_hits, k_patch_dests, k_patch_index, k_patch_merge (samples at whole-number film positions)
#include "dfilm.h"

namespace iile {

// film_accumulate: one thread per owned pixel adds this pass's samples, in
// sample order, to the pixel's RGB contribSum (FilmTile::AddSample, film.h:153-193
// with the box filter: weight 1 for the pixel containing pFilm).
__global__ __launch_bounds__(kBlock) void k_film_accumulate(DScene S, PassDesc P, PassBuffers B, FilmBuffers F) {
    const uint32_t n_pix = uint32_t(P.n_pass_tiles) * 256u;
    for (uint32_t lpt = blockIdx.x * kBlock + threadIdx.x; lpt < n_pix; lpt += gridDim.x * kBlock) {
        int px, py;
        uint32_t k;
        const uint32_t pid0 = lpt * uint32_t(P.kc);
        if (!path_pixel(S, P, pid0, &px, &py, &k)) continue;
        const uint32_t pt = uint32_t(P.slot0) * 256u + lpt;  // the pixel's slot among all owned tiles
        float4 acc = F.tile_rgbw[pt];
        // A lane's samples are consecutive in memory (1 KB apart from its neighbour's at 64 spp):
        // eight loads = one whole 128-byte line are issued together, then summed in sample order.
        for (int k8 = 0; k8 < P.kc; k8 += 8) {
            float4 Lb[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) Lb[j] = B.L[pid0 + uint32_t(k8 + j < P.kc ? k8 + j : k8)];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int kk = k8 + j;
                if (kk >= P.kc) break;
                const F3 L = guard_radiance(S, F3{Lb[j].x, Lb[j].y, Lb[j].z});
                acc.x += L.x, acc.y += L.y, acc.z += L.z;
                acc.w += 1.f;
                if (P.k0 + kk == 0) {
                    // a sample whose fractional film offset is exactly 0 also lands in the
                    // left / upper neighbour (support ceil(pd-.5) .. floor(pd+.5))
                    const uint32_t idx = sample_index(S, px, py, 0u);  // (= the index its camera ray was made with)
                    uint32_t mask = 0;
                    if (sample_dimension(S, idx, 0, px, py) == 0.f) mask |= 1u;
                    if (sample_dimension(S, idx, 1, px, py) == 0.f) mask |= 2u;
                    F.k0_rgbv[pt] = make_float4(L.x, L.y, L.z, b2f(mask));
                }
            }
        }
        F.tile_rgbw[pt] = acc;
    }
}

// Filters wider than a pixel (gaussian, mitchell, sinc, triangle, larger boxes). A pixel then sums samples of
// neighbouring pixels and tiles, in the order FilmTile::AddSample / MergeFilmTile give: inside a tile in pixel
// (row-major) then sample order, tiles in index order. The neighbouring pixels may belong to tiles of another pass, so
// the frame's samples are kept — k_film_store, 24 B each — and summed once at the end by a gather per film pixel
// (k_film_gather over dfilm.h's film_gather_pixel).
__global__ __launch_bounds__(kBlock) void k_film_store(DScene S, PassDesc P, PassBuffers B, FilmBuffers F, int k_begin, int n_samples) {
    for (uint32_t pid = blockIdx.x * kBlock + threadIdx.x; pid < P.n_paths; pid += gridDim.x * kBlock) {
        int px, py;
        uint32_t k;
        if (!path_pixel(S, P, pid, &px, &py, &k)) continue;
        const float4 L4 = B.L[pid];
        const F3 L = guard_radiance(S, F3{L4.x, L4.y, L4.z});
        // [tile slot][k][pixel of the tile]: the gather's lanes (neighbouring film pixels) read neighbouring records
        const uint32_t pt = uint32_t(P.slot0) * 256u + pid / uint32_t(P.kc);
        const size_t at = (size_t(pt >> 8) * size_t(n_samples) + size_t(int(k) - k_begin)) * 256u + size_t(pt & 255u);
        F.wide_L[at] = make_float4(L.x, L.y, L.z, 0.f);
        F.wide_pf[at] = sample_film_position(S, px, py, k);
    }
}

__global__ __launch_bounds__(kBlock) void k_film_gather(DScene S, PassDesc P, FilmBuffers F, int n_samples) {
    __shared__ float s_table[256];
    for (int j = threadIdx.x; j < 256; j += kBlock) s_table[j] = S.filter_table[j];
    __syncthreads();
    const int fw = S.crop_x1 - S.crop_x0, fh = S.crop_y1 - S.crop_y0;
    const uint32_t per = uint32_t(fw) * uint32_t(fh);
    const uint32_t n = per * (P.probe_mode ? uint32_t(P.n_owned_tiles / P.probe_tiles) : 1u);  // one film per probe
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t probe = i / per, loc = i % per;
        const int x = S.crop_x0 + int(loc % uint32_t(fw)), y = S.crop_y0 + int(loc / uint32_t(fw));
        F.film_xyzw[i] = film_gather_pixel(S, P, F, s_table, x, y, n_samples, [&](int qx, int qy, size_t row, float2 *pf, float4 *L) {
            const size_t at = P.probe_mode ? probe_record(S, P, probe, qx, qy) : row + size_t(qx);
            *pf = F.wide_pf[at];
            *L = F.wide_L[at];
        });
    }
}

// film_resolve: Film::MergeFilmTile (film.cpp:135-148) as a gather. For film
// pixel Q the contributions are grouped by the tile whose FilmTile holds them
// (Q's own tile, then the tiles right / below / diagonal whose k=0 samples
// splat onto Q), each group summed in RGB in pixel order, converted to XYZ and
// added in tile-index order.
__global__ __launch_bounds__(kBlock) void k_film_resolve(DScene S, PassDesc P, FilmBuffers F) {
    const int fw = S.crop_x1 - S.crop_x0, fh = S.crop_y1 - S.crop_y0;
    const uint32_t n = uint32_t(fw) * uint32_t(fh);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int qx = S.crop_x0 + int(i % uint32_t(fw)), qy = S.crop_y0 + int(i / uint32_t(fw));
        float4 out = make_float4(0, 0, 0, 0);
        const int lx = qx - S.samp_x0, ly = qy - S.samp_y0;
        const bool q_in = lx >= 0 && ly >= 0 && qx < S.samp_x1 && qy < S.samp_y1;
        const int tx0 = lx >= 0 ? lx / kTile : -1, ty0 = ly >= 0 ? ly / kTile : -1;
        const int tx1 = (lx + 1) >= 0 ? (lx + 1) / kTile : -1, ty1 = (ly + 1) >= 0 ? (ly + 1) / kTile : -1;
        // sources: S1 = (qx+1, qy) needs mask bit0; S2 = (qx, qy+1) bit1; S3 = (qx+1, qy+1) both
        auto source = [&](int sx, int sy, int tx, int ty, uint32_t need, float *r, float *g, float *b, float *w) {
            if (sx >= S.samp_x1 || sy >= S.samp_y1 || sx < S.samp_x0 || sy < S.samp_y0) return;
            uint32_t slot;
            if (!tile_owned(P, tx, ty, &slot)) return;
            const float4 v = F.k0_rgbv[slot * 256u + uint32_t(pixel_of_tile(S, sx, sy, tx, ty))];
            if ((f2b(v.w) & need) != need) return;
            *r += v.x, *g += v.y, *b += v.z;
            *w += 1.f;
        };
        // group 0: Q's own tile
        {
            uint32_t slot;
            float r = 0, g = 0, b = 0, w = 0;
            bool any = false;
            if (q_in && tile_owned(P, tx0, ty0, &slot)) {
                const float4 own = F.tile_rgbw[slot * 256u + uint32_t(pixel_of_tile(S, qx, qy, tx0, ty0))];
                r = own.x, g = own.y, b = own.z, w = own.w;
                any = true;
                if (tx1 == tx0) source(qx + 1, qy, tx0, ty0, 1u, &r, &g, &b, &w);
                if (ty1 == ty0) source(qx, qy + 1, tx0, ty0, 2u, &r, &g, &b, &w);
                if (tx1 == tx0 && ty1 == ty0) source(qx + 1, qy + 1, tx0, ty0, 3u, &r, &g, &b, &w);
            }
            if (any) add_xyz(&out, r, g, b, w);
        }
        // group 1: tile to the right in the same tile row
        if (tx1 != tx0 && ty0 >= 0) {
            float r = 0, g = 0, b = 0, w = 0;
            source(qx + 1, qy, tx1, ty0, 1u, &r, &g, &b, &w);
            if (ty1 == ty0) source(qx + 1, qy + 1, tx1, ty0, 3u, &r, &g, &b, &w);
            if (w > 0) add_xyz(&out, r, g, b, w);
        }
        // group 2: tile below in the same tile column
        if (ty1 != ty0 && tx0 >= 0) {
            float r = 0, g = 0, b = 0, w = 0;
            source(qx, qy + 1, tx0, ty1, 2u, &r, &g, &b, &w);
            if (tx1 == tx0) source(qx + 1, qy + 1, tx0, ty1, 3u, &r, &g, &b, &w);
            if (w > 0) add_xyz(&out, r, g, b, w);
        }
        // group 3: diagonal tile
        if (tx1 != tx0 && ty1 != ty0) {
            float r = 0, g = 0, b = 0, w = 0;
            source(qx + 1, qy + 1, tx1, ty1, 3u, &r, &g, &b, &w);
            if (w > 0) add_xyz(&out, r, g, b, w);
        }
        F.film_xyzw[i] = out;
    }
}

// ---------------------------------------------------------------------------
// The probe films. What their kernels share: the first hit's camera-space normal and distance of pixel (x, y) of probe `probe`,
// left in B.aux by the path kernels for the pixel's first sample of the launches, into pixel i of the two images
DEV void write_first_hit(const DScene &S, const PassDesc &P, const PassBuffers &B, uint32_t probe, int x, int y, size_t i, float *normals, float *distance) {
    const float4 a = B.aux[probe_record(S, P, probe, x, y) * size_t(P.kc)];
    normals[3 * i] = a.x, normals[3 * i + 1] = a.y, normals[3 * i + 2] = a.z;
    distance[i] = a.w;
}
// k_film_store into LDS: sample kk (of the launches' kc per pixel; the pixel's sample number k) of every pixel of the probe's film —
// guarded radiance, film position — at [y][x] of s_L / s_pf, by the whole block
DEV void stage_probe_film(const DScene &S, const PassDesc &P, const PassBuffers &B, uint32_t probe, int kc, int kk, uint32_t k, float2 *s_pf, float4 *s_L) {
    const int fw = S.crop_x1 - S.crop_x0, fh = S.crop_y1 - S.crop_y0;
    const int per = fw * fh;
    for (int j = threadIdx.x; j < per; j += kBlock) {
        const int x = S.crop_x0 + j % fw, y = S.crop_y0 + j / fw;
        const float4 L4 = B.L[probe_record(S, P, probe, x, y) * size_t(kc) + size_t(kk)];
        const F3 L = guard_radiance(S, F3{L4.x, L4.y, L4.z});
        s_L[j] = make_float4(L.x, L.y, L.z, 0.f);
        s_pf[j] = sample_film_position(S, x, y, k);
    }
}
// ... and film_gather_pixel's reader of it
struct StagedFilm {
    const float2 *s_pf;
    const float4 *s_L;
    int x0, y0, fw;
    DEV void operator()(int qx, int qy, size_t, float2 *pf, float4 *L) const {
        const int at = (qy - y0) * fw + (qx - x0);
        *pf = s_pf[at];
        *L = s_L[at];
    }
};

// Probe pass: film + aux images of every probe. Film::to_rgb_array on the gathered {X, Y, Z, w},
// and the first hits' normals / distances picked from the paths (1 spp): outputs [probe][y][x].
__global__ __launch_bounds__(kBlock) void k_probe_finish(DScene S, PassDesc P, PassBuffers B, FilmBuffers F, int n_probes, float *intensity,
                                                         float *normals, float *distance) {
    const int fw = S.crop_x1 - S.crop_x0, fh = S.crop_y1 - S.crop_y0;
    const uint32_t per = uint32_t(fw) * uint32_t(fh), n = per * uint32_t(n_probes);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        film_pixel_rgb(F.film_xyzw[i], intensity + 3 * size_t(i));
        const uint32_t probe = i / per, loc = i % per;
        const int x = S.crop_x0 + int(loc % uint32_t(fw)), y = S.crop_y0 + int(loc / uint32_t(fw));
        write_first_hit(S, P, B, probe, x, y, size_t(i), normals, distance);
    }
}

// The probe pass's film in one kernel (k_film_store + k_film_gather + k_probe_finish for films of at most kProbeFilmMax pixels, the
// IISPT network's 32 x 32): a block takes a probe, keeps the film's samples — guarded radiance, film position — in LDS, and
// every thread gathers its pixels from there (each sample is read by up to 36 pixels) and writes the three images.
constexpr int kProbeFilmMax = 1024;
__global__ __launch_bounds__(kBlock) void k_probe_film(DScene S, PassDesc P, PassBuffers B, int n_probes, float *intensity, float *normals, float *distance) {
    __shared__ float s_table[256];
    __shared__ float2 s_pf[kProbeFilmMax];
    __shared__ float4 s_L[kProbeFilmMax];
    for (int j = threadIdx.x; j < 256; j += kBlock) s_table[j] = S.filter_table[j];
    const int fw = S.crop_x1 - S.crop_x0, fh = S.crop_y1 - S.crop_y0;
    const int per = fw * fh;
    FilmBuffers none = {};
    for (uint32_t probe = blockIdx.x; probe < uint32_t(n_probes); probe += gridDim.x) {
        __syncthreads();   // (the table; the previous probe's gathers)
        stage_probe_film(S, P, B, probe, 1, 0, 0u, s_pf, s_L);   // (launch_probe_film: one sample per pixel, sample 0)
        __syncthreads();
        for (int j = threadIdx.x; j < per; j += kBlock) {
            const int x = S.crop_x0 + j % fw, y = S.crop_y0 + j / fw;
            const float4 px = film_gather_pixel(S, P, none, s_table, x, y, 1, StagedFilm{s_pf, s_L, S.crop_x0, S.crop_y0, fw});
            const size_t i = size_t(probe) * size_t(per) + size_t(j);
            film_pixel_rgb(px, intensity + 3 * i);  // k_probe_finish
            write_first_hit(S, P, B, probe, x, y, i, normals, distance);
        }
    }
}

// The accumulating probe film (iile_render_probes_reference: many samples per probe pixel behind the probe's filter). Per probe pixel
// and per tile its samples can come from, {sum of w L, sum of w} in HBM: acc[(probe * n_ord + ordinal) * per + pixel]. k_probe_film_add
// adds the P.kc samples of one set of launches to it: a block takes a probe and, sample after sample, keeps that sample's film — guarded
// radiance, film position — in LDS as k_probe_film does, and every thread adds it to its pixels' sums through film_gather_pixel. A sum
// grows in the order (sample, then pixel row by row), one addition at a time on the stored value, so it is the same number however the
// samples are cut into sets of launches; with one sample it is k_probe_film's. normals / distance (null: not wanted): the first hits of
// sample P.k0, as k_probe_film picks them.
struct ProbeTileSums {
    float4 *acc;     // the pixel's record of tile 0
    size_t stride;   // records between two tiles of a pixel
    bool write;
    DEV void load(int ordinal, float *r, float *g, float *b, float *w) const {
        const float4 v = acc[size_t(ordinal) * stride];
        *r = v.x, *g = v.y, *b = v.z, *w = v.w;
    }
    DEV void store(int ordinal, float r, float g, float b, float w) const {
        if (write) acc[size_t(ordinal) * stride] = make_float4(r, g, b, w);
    }
};
__global__ __launch_bounds__(kBlock) void k_probe_film_add(DScene S, PassDesc P, PassBuffers B, int n_probes, float4 *acc, int n_ord, float *normals,
                                                           float *distance) {
    __shared__ float s_table[256];
    __shared__ float2 s_pf[kProbeFilmMax];
    __shared__ float4 s_L[kProbeFilmMax];
    for (int j = threadIdx.x; j < 256; j += kBlock) s_table[j] = S.filter_table[j];
    const int fw = S.crop_x1 - S.crop_x0, fh = S.crop_y1 - S.crop_y0;
    const int per = fw * fh;
    FilmBuffers none = {};
    for (uint32_t probe = blockIdx.x; probe < uint32_t(n_probes); probe += gridDim.x) {
        for (int kk = 0; kk < P.kc; ++kk) {
            __syncthreads();   // (the table; the previous sample's gathers)
            stage_probe_film(S, P, B, probe, P.kc, kk, uint32_t(P.k0) + uint32_t(kk), s_pf, s_L);
            __syncthreads();
            for (int j = threadIdx.x; j < per; j += kBlock) {
                const int x = S.crop_x0 + j % fw, y = S.crop_y0 + j / fw;
                const ProbeTileSums sums{acc + size_t(probe) * size_t(n_ord) * size_t(per) + size_t(j), size_t(per), true};
                film_gather_pixel(S, P, none, s_table, x, y, 1, StagedFilm{s_pf, s_L, S.crop_x0, S.crop_y0, fw}, sums);
            }
        }
        if (normals)
            for (int j = threadIdx.x; j < per; j += kBlock)
                write_first_hit(S, P, B, probe, S.crop_x0 + j % fw, S.crop_y0 + j / fw, size_t(probe) * size_t(per) + size_t(j), normals, distance);
    }
}
// ... and its end: the tiles' sums of a pixel merged as Film::MergeFilmTile merges FilmTiles (a gather that adds no sample), then
// Film::to_rgb_array as k_probe_finish; weight_sum (null: not wanted): the pixel's filterWeightSum.
__global__ __launch_bounds__(kBlock) void k_probe_film_resolve(DScene S, PassDesc P, int n_probes, float4 *acc, int n_ord, float *intensity, float *weight_sum) {
    __shared__ float s_table[256];
    for (int j = threadIdx.x; j < 256; j += kBlock) s_table[j] = S.filter_table[j];
    __syncthreads();
    const int fw = S.crop_x1 - S.crop_x0, fh = S.crop_y1 - S.crop_y0;
    const uint32_t per = uint32_t(fw) * uint32_t(fh), n = per * uint32_t(n_probes);
    FilmBuffers none = {};
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t probe = i / per, loc = i % per;
        const int x = S.crop_x0 + int(loc % uint32_t(fw)), y = S.crop_y0 + int(loc / uint32_t(fw));
        const ProbeTileSums sums{acc + size_t(probe) * size_t(n_ord) * size_t(per) + size_t(loc), size_t(per), false};
        const float4 px = film_gather_pixel(S, P, none, s_table, x, y, 0, [](int, int, size_t, float2 *, float4 *) {}, sums);
        film_pixel_rgb(px, intensity + 3 * size_t(i));
        if (weight_sum) weight_sum[i] = px.w;
    }
}

// ---------------------------------------------------------------------------
// Exact film finish on the device, for the one-pixel box film. k_film_accumulate / k_film_resolve give every pixel the sum
// of its own samples (plus the k = 0 zero-offset splats): all there is unless a sample's film position is a whole number,
// when FilmTile::AddSample (film.h:159-188) also adds it to a neighbouring pixel, in sample order inside its tile. The
// generation code lists those samples (rare: ~1e-4 of them where pixel coordinates pass 1024); every pixel they touch is
// recomputed the way the reference sums it, per contributing tile and tiles in index order, by four small kernels that never
// leave the stream:
//   k_patch_hits    every flagged sample (kcommon.h flag_whole_film_position) -> one hit record per OTHER pixel it lands in
//                   (FilmTile::AddSample's support, film.h:159-166, clipped to its tile's FilmTile bounds, film.cpp:92-103),
//                   linked into the list of its destination through a hash table over film indices
//   k_patch_dests   the thread that finds its hit at the head of a destination's list walks that list in GENERATION order
//                   (tile, pixel of the tile, sample: the order in which one thread of the reference would have added them)
//                   and forms, per contributing tile, the exact FilmTile sum for that pixel -> an entry
//   k_patch_index / k_patch_merge   after k_film_resolve: per film pixel with an entry that the resolve kernel cannot have
//                   placed, the tiles' sums (and the pixel's own tile sum if no entry covers it) converted to XYZ and added
//                   in tile index order (Film::MergeFilmTile, film.cpp:135-148: the reference merges tiles in completion
//                   order, the oracle and this in index order, so that the sum does not depend on scheduling)
// Lists are short (a sample lands in at most three other pixels, a pixel is reached by a handful): they are walked by repeated
// selection of the next key instead of being sorted, which needs no bound on their length.
namespace {
struct FlagRec {
    int px, py, k, tile, pix;
    float pfx, pfy;
    uint32_t pid;
    bool plain_k0;
};
DEV FlagRec flag_decode(const DScene &S, int ntx, const float *flag_rec, uint32_t i) {
    const float *r = flag_rec + 6 * size_t(i);
    const uint32_t u2 = f2b(r[2]);
    FlagRec f;
    f.px = int(f2b(r[0])), f.py = int(f2b(r[1])), f.k = int(u2 & 0x3fffffffu);
    f.pfx = r[3], f.pfy = r[4];
    f.pid = f2b(r[5]);
    tile_of_pixel(S, f.px, f.py, ntx, &f.tile, &f.pix);
    const bool zero_x = (u2 >> 30) & 1u, zero_y = (u2 >> 31) & 1u;
    const bool whole_x = f.pfx == float(f.px) || f.pfx == float(f.px + 1), whole_y = f.pfy == float(f.py) || f.pfy == float(f.py + 1);
    f.plain_k0 = f.k == 0 && (!whole_x || zero_x) && (!whole_y || zero_y);  // k_film_resolve places these by itself
    return f;
}
DEV unsigned long long gen_key(const FlagRec &f) {
    return (static_cast<unsigned long long>(uint32_t(f.tile)) << 40) | (static_cast<unsigned long long>(uint32_t(f.pix)) << 32) |
           static_cast<unsigned long long>(uint32_t(f.k));
}
DEV uint32_t patch_hash(uint32_t key) { return key * 2654435761u; }
// claim (or find) the table slot of `key`; kPatchNil when the table is full
DEV uint32_t patch_slot(const PatchDev &D, uint32_t key, bool insert) {
    uint32_t s = patch_hash(key) & D.table_mask;
    for (uint32_t probe = 0; probe <= D.table_mask; ++probe, s = (s + 1) & D.table_mask) {
        const uint32_t seen = insert ? atomicCAS(&D.keys[s], kPatchNil, key) : D.keys[s];
        if (seen == key || (insert && seen == kPatchNil)) return s;
        if (!insert && seen == kPatchNil) return kPatchNil;
    }
    return kPatchNil;
}
}  // namespace

__global__ __launch_bounds__(kBlock) void k_patch_hits(DScene S, int ntx, PatchDev D, const uint32_t *flag_count, const float *flag_rec) {
    uint32_t n_flag = *flag_count;
    if (n_flag > kMaxFlagged) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&D.counters[2], 1u);
        n_flag = kMaxFlagged;
    }
    const int fw = S.crop_x1 - S.crop_x0;
    const float r = 0.5f;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_flag; i += gridDim.x * kBlock) {
        const FlagRec f = flag_decode(S, ntx, flag_rec, i);
        const FilmTileBounds t = film_tile_bounds(S, f.tile % ntx, f.tile / ntx, r, r);
        const float dxf = f.pfx - 0.5f, dyf = f.pfy - 0.5f;
        const int ax0 = support_lo(dxf, r, t.fx0), ax1 = support_hi(dxf, r, t.fx1);
        const int ay0 = support_lo(dyf, r, t.fy0), ay1 = support_hi(dyf, r, t.fy1);
        for (int y = ay0; y < ay1; ++y)
            for (int x = ax0; x < ax1; ++x) {
                if (x == f.px && y == f.py) continue;
                const uint32_t dest = uint32_t(y - S.crop_y0) * uint32_t(fw) + uint32_t(x - S.crop_x0);
                const uint32_t h = atomicAdd(&D.counters[0], 1u);
                if (h >= D.cap_hits) {
                    atomicOr(&D.counters[2], 1u);
                    continue;
                }
                const uint32_t s = patch_slot(D, dest, true);
                if (s == kPatchNil) {
                    atomicOr(&D.counters[2], 2u);
                    D.hits[h] = make_uint4(dest, i, kPatchNil, 1u);  // (never a list head: no thread processes it)
                    continue;
                }
                const uint32_t before = atomicExch(&D.heads[s], h);
                D.hits[h] = make_uint4(dest, i, before, 0u);
            }
    }
}

__global__ __launch_bounds__(kBlock) void k_patch_dests(DScene S, PassDesc P, PassBuffers B, FilmBuffers F, PatchDev D, int whole_frame) {
    const uint32_t n_hits = min(D.counters[0], D.cap_hits);
    const int ntx = P.n_tiles_x, fw = S.crop_x1 - S.crop_x0;
    for (uint32_t h0 = blockIdx.x * kBlock + threadIdx.x; h0 < n_hits; h0 += gridDim.x * kBlock) {
        const uint4 me = D.hits[h0];
        if (me.w != 0u) continue;
        const uint32_t slot_t = patch_slot(D, me.x, false);
        if (slot_t == kPatchNil || D.heads[slot_t] != h0) continue;  // one thread per destination: the head of its list
        // the destination pixel
        const uint32_t film_index = me.x;
        const int qx = S.crop_x0 + int(film_index % uint32_t(fw)), qy = S.crop_y0 + int(film_index / uint32_t(fw));
        int d_tile = -1, d_pix = 0;
        bool own_in_pass = false;
        uint32_t own_slot = 0;
        if (in_sample_bounds(S, qx, qy)) {
            tile_of_pixel(S, qx, qy, ntx, &d_tile, &d_pix);
            const int slot = tile_slot(P, d_tile);
            if (slot >= 0) {
                own_in_pass = slot >= P.slot0 && slot < P.slot0 + P.n_pass_tiles;
                own_slot = uint32_t(slot) * 256u + uint32_t(d_pix);
            }
        }
        bool all_plain = true, need_own = false;
        for (uint32_t h = h0; h != kPatchNil; h = D.hits[h].z) {
            const FlagRec f = flag_decode(S, ntx, B.flag_rec, D.hits[h].y);
            all_plain = all_plain && f.plain_k0;
            if (own_in_pass && f.tile == d_tile && f.pix < d_pix) need_own = true;
        }
        // a destination outside the integrator's pixel bounds took no samples of its own ("pixelbounds"): nothing to put in order, and
        // its slot of tile_rgbw holds the zeros it was cleared to
        if (!(qx >= S.pb_x0 && qx < S.pb_x1 && qy >= S.pb_y0 && qy < S.pb_y1)) need_own = false;
        // the pass is the whole frame: a pixel reached only by samples k_film_resolve places itself needs nothing
        if (whole_frame && all_plain) continue;
        float rr = 0, gg = 0, bb = 0, ww = 0;
        auto add = [&](uint32_t pid) {
            const float4 v = B.L[pid];
            const F3 c = guard_radiance(S, F3{v.x, v.y, v.z});
            rr += c.x * 1.f * 1.f;
            gg += c.y * 1.f * 1.f;
            bb += c.z * 1.f * 1.f;
            ww += 1.f;
        };
        auto add_own_samples = [&]() {  // (need_own: the pixel's own samples between the earlier and the later pixels' ones)
            const uint32_t first = (own_slot - uint32_t(P.slot0) * 256u) * uint32_t(P.kc);
            for (int k = 0; k < P.kc; ++k) add(first + uint32_t(k));
        };
        int cur_tile = -1;
        bool nonplain = false, own_run = false, own_done = false;
        auto emit = [&]() {
            if (own_run && need_own && !own_done) add_own_samples();
            const uint32_t e = atomicAdd(&D.counters[1], 1u);
            if (e >= D.cap_entries) {
                atomicOr(&D.counters[2], 1u);
                return;
            }
            D.ent_a[e] = make_uint4(film_index, uint32_t(cur_tile), nonplain ? 1u : 0u, kPatchNil);
            D.ent_b[e] = make_float4(rr, gg, bb, ww);
        };
        unsigned long long prev = 0;
        bool have_prev = false;
        for (;;) {
            // the next hit in generation order
            uint32_t best = kPatchNil;
            unsigned long long best_key = ~0ull;
            for (uint32_t h = h0; h != kPatchNil; h = D.hits[h].z) {
                const unsigned long long key = gen_key(flag_decode(S, ntx, B.flag_rec, D.hits[h].y));
                if ((!have_prev || key > prev) && key < best_key) best = h, best_key = key;
            }
            if (best == kPatchNil) break;
            prev = best_key, have_prev = true;
            const FlagRec f = flag_decode(S, ntx, B.flag_rec, D.hits[best].y);
            if (f.tile != cur_tile) {
                if (cur_tile >= 0) emit();
                cur_tile = f.tile;
                rr = gg = bb = ww = 0.f;
                nonplain = false;
                own_run = own_in_pass && f.tile == d_tile;
                own_done = false;
                if (own_run && !need_own) {  // the finished sum of its own samples (k_film_accumulate), the later pixels' ones follow
                    const float4 own = F.tile_rgbw[own_slot];
                    rr = own.x, gg = own.y, bb = own.z, ww = own.w;
                }
            }
            if (own_run && need_own && !own_done && f.pix > d_pix) {
                add_own_samples();
                own_done = true;
            }
            add(f.pid);
            nonplain = nonplain || !f.plain_k0;
        }
        if (cur_tile >= 0) emit();
    }
}

__global__ __launch_bounds__(kBlock) void k_patch_index(PatchDev D) {
    const uint32_t n = min(D.counters[1], D.cap_entries);
    for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
        const uint32_t s = patch_slot(D, D.ent_a[e].x, true);
        if (s == kPatchNil) {
            atomicOr(&D.counters[2], 2u);
            continue;
        }
        D.ent_a[e].w = atomicExch(&D.heads[s], e);
    }
}

__global__ __launch_bounds__(kBlock) void k_patch_merge(DScene S, PassDesc P, FilmBuffers F, PatchDev D) {
    const uint32_t n = min(D.counters[1], D.cap_entries);
    const int ntx = P.n_tiles_x, fw = S.crop_x1 - S.crop_x0;
    for (uint32_t e0 = blockIdx.x * kBlock + threadIdx.x; e0 < n; e0 += gridDim.x * kBlock) {
        const uint32_t film_index = D.ent_a[e0].x;
        const uint32_t slot_t = patch_slot(D, film_index, false);
        if (slot_t == kPatchNil || D.heads[slot_t] != e0) continue;  // one thread per film pixel
        bool nonplain = false;
        for (uint32_t e = e0; e != kPatchNil; e = D.ent_a[e].w) nonplain = nonplain || D.ent_a[e].z != 0u;
        if (!nonplain) continue;  // k_film_resolve has placed everything that reaches this pixel
        // the pixel's own tile, if it is owned and no entry covers it: its finished sum takes its place in tile order
        const int qx = S.crop_x0 + int(film_index % uint32_t(fw)), qy = S.crop_y0 + int(film_index / uint32_t(fw));
        int own_tile = -1;
        float4 own = make_float4(0, 0, 0, 0);
        if (in_sample_bounds(S, qx, qy)) {
            int q_tile, q_pix;
            tile_of_pixel(S, qx, qy, ntx, &q_tile, &q_pix);
            bool covered = false;
            for (uint32_t e = e0; e != kPatchNil; e = D.ent_a[e].w) covered = covered || int(D.ent_a[e].y) == q_tile;
            const int slot = tile_slot(P, q_tile);
            if (!covered && slot >= 0) {
                own_tile = q_tile;
                own = F.tile_rgbw[uint32_t(slot) * 256u + uint32_t(q_pix)];
            }
        }
        float4 o = make_float4(0, 0, 0, 0);
        bool own_added = own_tile < 0;
        int prev_tile = -1;
        for (;;) {
            uint32_t best = kPatchNil;
            int best_tile = 0x7fffffff;
            for (uint32_t e = e0; e != kPatchNil; e = D.ent_a[e].w) {
                const int t = int(D.ent_a[e].y);
                if (t > prev_tile && t < best_tile) best = e, best_tile = t;
            }
            if (best == kPatchNil) break;
            prev_tile = best_tile;
            if (!own_added && own_tile < best_tile) {
                add_xyz(&o, own.x, own.y, own.z, own.w);
                own_added = true;
            }
            const float4 v = D.ent_b[best];
            add_xyz(&o, v.x, v.y, v.z, v.w);
        }
        if (!own_added) add_xyz(&o, own.x, own.y, own.z, own.w);
        F.film_xyzw[film_index] = o;
    }
}

// ---------------------------------------------------------------------------
// launchers
static uint32_t film_pixels(const DScene &S) { return uint32_t(S.crop_x1 - S.crop_x0) * uint32_t(S.crop_y1 - S.crop_y0); }
void launch_film_accumulate(const DScene &S, const PassDesc &P, const PassBuffers &B, const FilmBuffers &F, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_film_accumulate, dim3(grid_blocks(uint32_t(P.n_pass_tiles) * 256u, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, B, F);
}
void launch_film_store(const DScene &S, const PassDesc &P, const PassBuffers &B, const FilmBuffers &F, int k_begin, int n_samples, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_film_store, dim3(grid_blocks(P.n_paths, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, B, F, k_begin, n_samples);
}
void launch_film_gather(const DScene &S, const PassDesc &P, const FilmBuffers &F, int n_samples, const LaunchCfg &cfg) {
    const uint32_t n = film_pixels(S) * (P.probe_mode ? uint32_t(P.n_owned_tiles / P.probe_tiles) : 1u);
    hipLaunchKernelGGL(k_film_gather, dim3(grid_blocks(n, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, F, n_samples);
}
void launch_film_resolve(const DScene &S, const PassDesc &P, const FilmBuffers &F, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_film_resolve, dim3(grid_blocks(film_pixels(S), cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, F);
}
void launch_probe_finish(const DScene &S, const PassDesc &P, const PassBuffers &B, const FilmBuffers &F, int n_probes, float *intensity, float *normals,
                         float *distance, const LaunchCfg &cfg) {
    const uint32_t n = film_pixels(S) * uint32_t(n_probes);
    hipLaunchKernelGGL(k_probe_finish, dim3(grid_blocks(n, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, B, F, n_probes, intensity, normals, distance);
}
bool launch_probe_film(const DScene &S, const PassDesc &P, const PassBuffers &B, int n_probes, float *intensity, float *normals, float *distance,
                       const LaunchCfg &cfg) {
    if (film_pixels(S) > uint32_t(kProbeFilmMax) || P.kc != 1) return false;   // (larger probe films: the three general kernels)
    hipLaunchKernelGGL(k_probe_film, dim3(unsigned(std::min(n_probes, cfg.n_cus * 8))), dim3(kBlock), 0, cfg.stream, S, P, B, n_probes, intensity, normals,
                       distance);
    return true;
}
int probe_film_tiles(const DScene &S) {
    if (film_pixels(S) > uint32_t(kProbeFilmMax)) return 0;
    // a pixel gathers from 2 ceil(r + 0.5) + 1 sample pixels along an axis (film_gather_pixel), n pixels lie in at most (n - 2) / 16 + 2 tiles
    const int ax = (2 * int(ceilf(S.filter_rx + 0.5f)) - 1) / kTile + 2, ay = (2 * int(ceilf(S.filter_ry + 0.5f)) - 1) / kTile + 2;
    return ax * ay;
}
void launch_probe_film_add(const DScene &S, const PassDesc &P, const PassBuffers &B, int n_probes, float4 *acc, int n_ord, float *normals, float *distance,
                           const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_probe_film_add, dim3(unsigned(std::min(n_probes, cfg.n_cus * 8))), dim3(kBlock), 0, cfg.stream, S, P, B, n_probes, acc, n_ord, normals,
                       distance);
}
void launch_probe_film_resolve(const DScene &S, const PassDesc &P, int n_probes, float4 *acc, int n_ord, float *intensity, float *weight_sum, const LaunchCfg &cfg) {
    const uint32_t n = film_pixels(S) * uint32_t(n_probes);
    hipLaunchKernelGGL(k_probe_film_resolve, dim3(grid_blocks(n, cfg.n_cus, 8)), dim3(kBlock), 0, cfg.stream, S, P, n_probes, acc, n_ord, intensity, weight_sum);
}
void launch_patch_pass(const DScene &S, const PassDesc &P, const PassBuffers &B, const FilmBuffers &F, const PatchDev &D, const LaunchCfg &cfg) {
    // (the table is cleared by the caller: two hipMemsetAsync of 0xff)
    const int whole_frame = P.n_pass_tiles == P.n_owned_tiles ? 1 : 0;
    hipLaunchKernelGGL(k_patch_hits, dim3(64), dim3(kBlock), 0, cfg.stream, S, P.n_tiles_x, D, B.flag_count, B.flag_rec);
    hipLaunchKernelGGL(k_patch_dests, dim3(128), dim3(kBlock), 0, cfg.stream, S, P, B, F, D, whole_frame);
}
void launch_patch_merge(const DScene &S, const PassDesc &P, const FilmBuffers &F, const PatchDev &D, const LaunchCfg &cfg) {
    hipLaunchKernelGGL(k_patch_index, dim3(64), dim3(kBlock), 0, cfg.stream, D);
    hipLaunchKernelGGL(k_patch_merge, dim3(128), dim3(kBlock), 0, cfg.stream, S, P, F, D);
}

}  // namespace iile
