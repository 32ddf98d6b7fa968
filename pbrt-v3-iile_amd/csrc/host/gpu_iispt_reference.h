// gpu_iispt_reference.h — the IISPT integrator's reference mode for C++ hosts (`pbrt --reference=N`): the training sets of
// IISPTNet, written against the C ABI only (include/iile_host.h, include/iile_gpu.h).
//
//   reference                                                        here
//   PbrtOptions.referenceTiles / referencePixelSamples /             ReferenceOptions (--reference= / --reference_samples= / --reference_resume=,
//     referenceResume (src/core/pbrt.h:172-175, main/pbrt.cpp:154-166) same spellings and defaults)
//   IISPTIntegrator::render_reference (iispt.cpp:456-526)            ReferenceGrid (the pixels, ref_idx from 1, $IISPT_REFERENCE_CONTROL_MOD / _MATCH)
//   generate_reference_name, exec_if_not_exists,                     ReferencePixel::File, ReferenceGrid's pending flags
//     exec_if_one_not_exists (iispt.cpp:82-168)
//   IISPTIntegrator::Li_reference (iispt.cpp:650-744)                iile_reference_points + iile_render_probes_reference, batches of hemispheres
//   write_info_file (iispt.cpp:314-339)                              WriteReferenceInfo
//   IISPTdIntegrator::save_reference / save_reference_camera_only    WriteReferencePfm: d and p through Film::WriteImage -> WriteImagePFM
//     (iispt_d.cpp:464-478)                                            (imageio.cpp: scanlines bottom to top), z and n through ImageFilm::write of
//                                                                      films filled by set_camera_coord (imagefilm.cpp:26-81: row height - 1 - y) —
//                                                                      all four files hold raster row (height - 1 - j) as their row j
//
// The reference renders one hemisphere at a time on the CPU, every sample a RandomSampler's; here the pending hemispheres are rendered in
// batches, sample k of a probe pixel being sample k of the probe's Halton sampler (iile_render_probes_reference). The probe depth is
// IISPTdIntegrator's own, 3: CreateIISPTdIntegrator(dcamera, 13) passes 13 as the sampler's seed (iispt_d.cpp:501-529).
#pragma once
#include <sys/stat.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "gpu_integrator.h"

namespace iile {

struct ReferenceOptions {
    int tiles = -1;       // PbrtOptions.referenceTiles (--reference=N); <= 0: no reference mode
    int samples = 4096;   // PbrtOptions.referencePixelSamples (--reference_samples=S)
    int resume = 1;       // PbrtOptions.referenceResume (--reference_resume=0|1)
    int rank = 0, nranks = 1;   // --gpurank R/N: this process renders the pixels of its list whose position is R modulo N
    int devices = 1;            // --gpus N: N devices of this process, a host thread each, the list dealt the same way among them
    int max_probes = 256;       // hemispheres per batch (their images come back to the host and are written before the next batch)
    std::string directory = "out/";   // IISPT_REFERENCE_DIRECTORY (iispt_d.h:56)
};
constexpr int kReferenceDepth = 3;   // IISPTdIntegrator's maxDepth (iispt_d.cpp:505)

struct ReferencePixel {
    int ref_idx, x, y;
    bool one_pending, p_pending;   // the 1-sample group {d, z, n} (exec_if_one_not_exists) / the many-sample p (exec_if_not_exists)
    std::string File(const std::string &dir, const char *kind) const {   // generate_reference_name
        return dir + kind + "_" + std::to_string(x) + "_" + std::to_string(y) + ".pfm";
    }
};

inline bool reference_file_exists(const std::string &name) {
    FILE *fp = fopen(name.c_str(), "rb");
    if (fp) fclose(fp);
    return fp != nullptr;
}

// render_reference's loop over the film's sample extent: the pixels of THIS process ($IISPT_REFERENCE_CONTROL_MOD / _MATCH, then the
// --gpurank share) and what is left to render for each. false (message in *err): nothing is to be rendered.
inline bool ReferenceGrid(const iile_film_desc *f, const ReferenceOptions &opt, std::vector<ReferencePixel> *out, std::string *err) {
    const int ext_x = f->samp_x1 - f->samp_x0, ext_y = f->samp_y1 - f->samp_y0;   // camera->film->GetSampleBounds().Diagonal()
    const int step_x = ext_x / opt.tiles, step_y = ext_y / opt.tiles;
    if (step_x == 0 || step_y == 0) {
        *err = "Reference tile interval too small. Image resolution could be too small or reference tiles too many";
        return false;
    }
    int mod = 1, match = 0;
    if (const char *e = std::getenv("IISPT_REFERENCE_CONTROL_MOD")) mod = std::atoi(e);
    if (const char *e = std::getenv("IISPT_REFERENCE_CONTROL_MATCH")) match = std::atoi(e);
    if (mod < 1) {
        *err = "IISPT_REFERENCE_CONTROL_MOD wants a number >= 1";
        return false;
    }
    int ref_idx = 0;
    size_t mine = 0;
    for (int y = 0; y < ext_y; y += step_y)
        for (int x = 0; x < ext_x; x += step_x) {
            ref_idx++;
            if ((ref_idx % mod) != match) continue;   // "This pixel is not a job of the current process"
            if (int(mine++ % size_t(opt.nranks)) != opt.rank) continue;
            ReferencePixel p = {ref_idx, x, y, true, true};
            if (opt.resume != 0) {
                p.one_pending = !reference_file_exists(p.File(opt.directory, "d")) || !reference_file_exists(p.File(opt.directory, "z")) ||
                                !reference_file_exists(p.File(opt.directory, "n"));
                p.p_pending = !reference_file_exists(p.File(opt.directory, "p"));
            }
            out->push_back(p);
        }
    return true;
}

// --reference-list: the grid as this process would render it, one pixel per line, no device touched
inline void PrintReferenceGrid(const std::vector<ReferencePixel> &grid, const ReferenceOptions &opt) {
    for (const ReferencePixel &p : grid)
        printf("%d %d %d %s %s %s %s %s %s\n", p.ref_idx, p.x, p.y, p.File(opt.directory, "d").c_str(), p.File(opt.directory, "z").c_str(),
               p.File(opt.directory, "n").c_str(), p.File(opt.directory, "p").c_str(), p.one_pending ? "pending" : "present", p.p_pending ? "pending" : "present");
}

// `rows` raster rows of `width` pixels, `channels` floats each (1: "Pf", 3: "PF"), little endian, file row j = raster row rows - 1 - j
inline bool WriteReferencePfm(const std::string &path, const float *data, int width, int rows, int channels) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) {
        fprintf(stderr, "Error: reference mode: cannot open %s: %s\n", path.c_str(), strerror(errno));
        return false;
    }
    fprintf(fp, "%s\n%d %d\n-1.0\n", channels == 1 ? "Pf" : "PF", width, rows);
    const size_t row = size_t(width) * size_t(channels);
    bool ok = true;
    for (int y = rows - 1; y >= 0 && ok; --y) ok = fwrite(data + size_t(y) * row, sizeof(float), row, fp) == row;
    ok = (fclose(fp) == 0) && ok;
    if (!ok) fprintf(stderr, "Error: reference mode: short write to %s\n", path.c_str());
    return ok;
}

// write_info_file: the two normalisation constants the training scripts fill in later (rapidjson prints the doubles as 0.0)
inline bool WriteReferenceInfo(const std::string &path) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) {
        fprintf(stderr, "Error: reference mode: cannot open %s: %s\n", path.c_str(), strerror(errno));
        return false;
    }
    fputs("{\"normalization_intensity\":0.0,\"normalization_distance\":0.0}", fp);
    return fclose(fp) == 0;
}

// The directory exists (made if need be) and takes a file: checked before any device is touched
inline bool PrepareReferenceDirectory(const std::string &dir) {
    std::string d = dir;
    while (d.size() > 1 && d.back() == '/') d.pop_back();
    if (mkdir(d.c_str(), 0777) != 0 && errno != EEXIST) {
        fprintf(stderr, "Error: reference mode: cannot create directory %s: %s\n", d.c_str(), strerror(errno));
        return false;
    }
    const std::string probe = dir + ".iile_write_test";
    FILE *fp = fopen(probe.c_str(), "wb");
    if (!fp) {
        fprintf(stderr, "Error: reference mode: cannot write into directory %s: %s\n", d.c_str(), strerror(errno));
        return false;
    }
    fclose(fp);
    remove(probe.c_str());
    return true;
}

class GpuIisptReference {
  public:
    explicit GpuIisptReference(ReferenceOptions opt) : opt_(std::move(opt)) {}

    struct Stats {
        long long pixels = 0, no_hit = 0, one_sample_sets = 0, reference_hemispheres = 0;
        double ms = 0;
    } stats;

    // the pixels of `grid` (ReferenceGrid) that still have files to write, on opt.devices devices of this process
    bool Render(const Scene &scene, const std::vector<ReferencePixel> &grid) {
        if (!scene.ok()) return false;
        if (scene.desc()->probe.hemi_size <= 0) return Fail("the scene has no probe setup");
        std::vector<ReferencePixel> todo;
        for (const ReferencePixel &p : grid)
            if (p.one_pending || p.p_pending) todo.push_back(p);
        if (todo.empty()) return true;
        const int n_dev = std::max(1, opt_.devices);
        if (n_dev == 1) return RenderShare(scene, todo, 0, 1, -1, &stats);
        if (n_dev > iile_device_count()) return Fail("--gpus asks for more devices than are visible");
        std::vector<Stats> st(static_cast<size_t>(n_dev));
        std::vector<char> ok(static_cast<size_t>(n_dev), 0);
        std::vector<std::thread> threads;
        for (int r = 0; r < n_dev; ++r)
            threads.emplace_back([&, r]() { ok[size_t(r)] = RenderShare(scene, todo, r, n_dev, r, &st[size_t(r)]) ? 1 : 0; });
        for (std::thread &t : threads) t.join();
        bool all = true;
        for (int r = 0; r < n_dev; ++r) {
            all = all && ok[size_t(r)] != 0;
            stats.pixels += st[size_t(r)].pixels, stats.no_hit += st[size_t(r)].no_hit, stats.one_sample_sets += st[size_t(r)].one_sample_sets;
            stats.reference_hemispheres += st[size_t(r)].reference_hemispheres, stats.ms = std::max(stats.ms, st[size_t(r)].ms);
        }
        return all;
    }

  private:
    static bool Fail(const char *msg) {
        fprintf(stderr, "Error: reference mode: %s\n", msg);
        return false;
    }
    // pixels share, share + of, ... of `todo` on one device (device < 0: the process's current one)
    bool RenderShare(const Scene &scene, const std::vector<ReferencePixel> &todo, int share, int of, int device, Stats *st) const {
        if (device >= 0 && iile_device_select(device) != IILE_OK) return Fail(iile_last_error());
        iile_scene *gpu = nullptr;
        if (iile_scene_create(scene.desc(), &gpu) != IILE_OK) return Fail(iile_last_error());
        std::vector<ReferencePixel> mine;
        for (size_t i = size_t(share); i < todo.size(); i += size_t(of)) mine.push_back(todo[i]);
        bool ok = true;
        for (size_t first = 0; first < mine.size() && ok; first += size_t(opt_.max_probes))
            ok = RenderBatch(gpu, scene.desc()->probe.hemi_size, mine.data() + first, std::min(mine.size() - first, size_t(opt_.max_probes)), st);
        iile_scene_destroy(gpu);
        return ok;
    }
    // Li_reference for n pixels: the points, the 1-sample rasters of those that want them, the many-sample raster of those that want it
    bool RenderBatch(iile_scene *gpu, int hemi, const ReferencePixel *px, size_t n, Stats *st) const {
        std::vector<float> pfilm(2 * n), pos(3 * n), dir(3 * n);
        std::vector<uint8_t> valid(n);
        for (size_t i = 0; i < n; ++i) pfilm[2 * i] = float(px[i].x), pfilm[2 * i + 1] = float(px[i].y);   // current_sample.pFilm = Point2f(px_x, px_y)
        if (iile_reference_points(gpu, int32_t(n), pfilm.data(), valid.data(), pos.data(), dir.data()) != IILE_OK) return Fail(iile_last_error());
        st->pixels += (long long)n;
        const size_t img = size_t(hemi) * size_t(hemi);
        std::vector<float> inten, nrm, dist, cpos, cdir;
        std::vector<size_t> who;
        // the hemispheres of the pixels that hit something and want group `many` (false: d, z, n; true: p)
        auto select = [&](bool many) {
            who.clear(), cpos.clear(), cdir.clear();
            for (size_t i = 0; i < n; ++i)
                if (valid[i] && (many ? px[i].p_pending : px[i].one_pending)) {
                    who.push_back(i);
                    cpos.insert(cpos.end(), &pos[3 * i], &pos[3 * i] + 3);
                    cdir.insert(cdir.end(), &dir[3 * i], &dir[3 * i] + 3);
                }
            inten.resize(who.size() * img * 3);
        };
        for (size_t i = 0; i < n; ++i)
            if (!valid[i]) st->no_hit++;   // "No intersection": no files
        iile_probe_ref_params prm = {};
        prm.max_depth = kReferenceDepth;
        iile_stats gs;
        select(false);
        if (!who.empty()) {
            nrm.resize(who.size() * img * 3), dist.resize(who.size() * img);
            prm.n_samples = 1;
            if (iile_render_probes_reference(gpu, int32_t(who.size()), cpos.data(), cdir.data(), &prm, inten.data(), nullptr, nrm.data(), dist.data(), &gs) != IILE_OK)
                return Fail(iile_last_error());
            st->ms += gs.ms_total;
            for (size_t j = 0; j < who.size(); ++j) {
                const ReferencePixel &p = px[who[j]];
                if (!WriteReferencePfm(p.File(opt_.directory, "d"), &inten[j * img * 3], hemi, hemi, 3) ||
                    !WriteReferencePfm(p.File(opt_.directory, "z"), &dist[j * img], hemi, hemi, 1) ||
                    !WriteReferencePfm(p.File(opt_.directory, "n"), &nrm[j * img * 3], hemi, hemi, 3))
                    return false;
            }
            st->one_sample_sets += (long long)who.size();
        }
        select(true);
        if (!who.empty()) {
            prm.n_samples = opt_.samples;
            if (iile_render_probes_reference(gpu, int32_t(who.size()), cpos.data(), cdir.data(), &prm, inten.data(), nullptr, nullptr, nullptr, &gs) != IILE_OK)
                return Fail(iile_last_error());
            st->ms += gs.ms_total;
            for (size_t j = 0; j < who.size(); ++j)
                if (!WriteReferencePfm(px[who[j]].File(opt_.directory, "p"), &inten[j * img * 3], hemi, hemi, 3)) return false;
            st->reference_hemispheres += (long long)who.size();
        }
        return true;
    }

    ReferenceOptions opt_;
};

}  // namespace iile
