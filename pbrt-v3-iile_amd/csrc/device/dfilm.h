// dfilm.h — the film's device functions, each one a step of the reference's film said once: the radiance guards of
// SamplerIntegrator::Render, a camera sample's film position, the tiles of the sample bounds and their FilmTiles,
// FilmTile::AddSample's support, the gather of one film pixel, RGB <-> XYZ and Film::to_rgb_array. For kernels_film.hip and, the
// guards into its double film, kernels_direct.hip. Every float expression stands as the kernels spelled it out before.
#pragma once
#include "kcommon.h"

namespace iile {

// ---- a sample's radiance and film position ----
// the radiance guards of SamplerIntegrator::Render (integrator.cpp:293-314): NaN, negative luminance, infinite luminance
DEV F3 radiance_guards(F3 L) {
    const float y = lum_y(L);
    if (is_nan(L.x) || is_nan(L.y) || is_nan(L.z))
        L = F3{0, 0, 0};
    else if (double(y) < -1e-5)
        L = F3{0, 0, 0};
    else if (is_inf(y))
        L = F3{0, 0, 0};
    return L;
}
// ... and the luminance clamp of FilmTile::AddSample (film.h:157-158)
DEV F3 guard_radiance(const DScene &S, F3 L) {
    L = radiance_guards(L);
    const float y2 = lum_y(L);
    if (y2 > S.max_sample_luminance) L = L * (S.max_sample_luminance / y2);
    return L;
}
// the direct pass's film: guarded, unclamped radiance of one camera sample added to pixel (px, py)'s double {r, g, b, samples}
DEV void direct_film_add(double *film_rgbw, const DScene &S, int px, int py, F3 L) {
    L = radiance_guards(L);
    const int fw = S.crop_x1 - S.crop_x0;
    double *out = film_rgbw + 4 * (size_t(py - S.crop_y0) * fw + (px - S.crop_x0));
    out[0] += double(L.x), out[1] += double(L.y), out[2] += double(L.z);
    out[3] += 1.0;
}
// pFilm of sample k of pixel (px, py): the pixel plus the first two dimensions of Sampler::GetCameraSample (sampler.cpp:46-52)
DEV float2 sample_film_position(const DScene &S, int px, int py, uint32_t k) {
    const uint32_t idx = sample_index(S, px, py, k);  // (= the index its camera ray was made with)
    return make_float2(float(px) + sample_dimension(S, idx, 0, px, py), float(py) + sample_dimension(S, idx, 1, px, py));
}

// ---- the 16 x 16 sample tiles of SamplerIntegrator::Render (integrator.cpp:235-237) and their FilmTiles ----
// slot of tile t among the rank's tiles (negative: another rank's)
DEV int tile_slot(const PassDesc &P, int t) { return P.slot_of_tile ? P.slot_of_tile[t] : t; }
DEV bool tile_owned(const PassDesc &P, int tx, int ty, uint32_t *slot) {
    if (tx < 0 || ty < 0 || tx >= P.n_tiles_x || ty >= P.n_tiles_y) return false;
    const int s = tile_slot(P, ty * P.n_tiles_x + tx);
    if (s < 0) return false;
    *slot = uint32_t(s);
    return true;
}
// pixel (x, y) of tile (tx, ty), row by row
DEV int pixel_of_tile(const DScene &S, int x, int y, int tx, int ty) {
    return (y - S.samp_y0 - ty * kTile) * kTile + (x - S.samp_x0 - tx * kTile);
}
DEV bool in_sample_bounds(const DScene &S, int x, int y) { return x >= S.samp_x0 && x < S.samp_x1 && y >= S.samp_y0 && y < S.samp_y1; }
// tile (of ntx per row) and pixel of the tile of a film pixel (x, y) inside the sample bounds
DEV void tile_of_pixel(const DScene &S, int x, int y, int ntx, int *tile, int *pix) {
    const int tx = (x - S.samp_x0) / kTile, ty = (y - S.samp_y0) / kTile;
    *pix = pixel_of_tile(S, x, y, tx, ty);
    *tile = ty * ntx + tx;
}
// The samples [sx0, sx1) x [sy0, sy1) of tile (tx, ty) and the pixels [fx0, fx1) x [fy0, fy1) of its FilmTile behind a filter of
// radius (rx, ry) (Film::GetFilmTile, film.cpp:92-103)
struct FilmTileBounds {
    int sx0, sy0, sx1, sy1;
    int fx0, fy0, fx1, fy1;
    DEV bool holds(int x, int y) const { return !(x < fx0 || x >= fx1 || y < fy0 || y >= fy1); }
};
DEV FilmTileBounds film_tile_bounds(const DScene &S, int tx, int ty, float rx, float ry) {
    FilmTileBounds t;
    t.sx0 = S.samp_x0 + tx * kTile, t.sy0 = S.samp_y0 + ty * kTile;
    t.sx1 = min(t.sx0 + kTile, S.samp_x1), t.sy1 = min(t.sy0 + kTile, S.samp_y1);
    t.fx0 = max(int(ceilf(float(t.sx0) - 0.5f - rx)), S.crop_x0), t.fx1 = min(int(floorf(float(t.sx1) - 0.5f + rx)) + 1, S.crop_x1);
    t.fy0 = max(int(ceilf(float(t.sy0) - 0.5f - ry)), S.crop_y0), t.fy1 = min(int(floorf(float(t.sy1) - 0.5f + ry)) + 1, S.crop_y1);
    return t;
}
// FilmTile::AddSample's support along one axis (film.h:159-166): a sample at the discrete film position d = pFilm - 0.5 reaches the
// pixels [support_lo, support_hi) of a FilmTile whose pixels are [f0, f1) behind a filter of radius r (one bound per call: a
// gather asking whether one pixel is reached stops at the first bound that says no; profiles/film_kernels_resources.txt)
DEV int support_lo(float d, float r, int f0) { return max(int(ceilf(d - r)), f0); }
DEV int support_hi(float d, float r, int f1) { return min(int(floorf(d + r)) + 1, f1); }

// ---- colour ----
DEV void add_xyz(float4 *out, float r, float g, float b, float w) {  // RGBToXYZ, spectrum.h:62-66
    out->x += 0.412453f * r + 0.357580f * g + 0.180423f * b;
    out->y += 0.212671f * r + 0.715160f * g + 0.072169f * b;
    out->z += 0.019334f * r + 0.119193f * g + 0.950227f * b;
    out->w += w;
}
// Film::to_rgb_array (film.cpp:187-225) for one pixel {X, Y, Z, filterWeightSum}: XYZToRGB, the division by the weight sum,
// no negative values, then the (zero) splat and the scale of 1, into the image's three floats of the pixel
DEV void film_pixel_rgb(float4 px, float rgb[3]) {
    float v[3];
    v[0] = 3.240479f * px.x - 1.537150f * px.y - 0.498535f * px.z;  // XYZToRGB, spectrum.h:56-60
    v[1] = -0.969256f * px.x + 1.875991f * px.y + 0.041556f * px.z;
    v[2] = 0.055648f * px.x - 0.204043f * px.y + 1.057311f * px.z;
    if (px.w != 0) {
        const float inv_wt = 1.f / px.w;
        for (int c = 0; c < 3; ++c) v[c] = mx(0.f, v[c] * inv_wt);
    }
    for (int c = 0; c < 3; ++c) rgb[c] = (v[c] + 0.f) * 1.f;
}

// ---- the gather ----
// One film pixel of the gather: the sum over the tiles whose FilmTile holds (x, y), in tile index order, of the samples
// FilmTile::AddSample would have added to it, in pixel then sample order. rec1(qx, qy, row): the record {film position, radiance} of
// sample pixel (qx, qy) when there is one sample per pixel; the several-samples form reads F directly.
// sums(ordinal): the running {r, g, b, w} of the pixel's tile number `ordinal` (counted row by row over the tiles its samples can come
// from) in an accumulating film — loaded before the tile's samples are added, stored after; the plain gather starts every tile at zero.
struct NoTileSums {
    DEV void load(int, float *, float *, float *, float *) const {}
    DEV void store(int, float, float, float, float) const {}
};
template <typename Rec1, typename Sums = NoTileSums>
DEV float4 film_gather_pixel(const DScene &S, const PassDesc &P, const FilmBuffers &F, const float *s_table, int x, int y, int n_samples, Rec1 rec1,
                             Sums sums = Sums()) {
    const float rx = S.filter_rx, ry = S.filter_ry;
    const float inv_rx = 1 / rx, inv_ry = 1 / ry;  // Filter::invRadius
    // sample pixels that can reach (x, y): |q + u - 0.5 - x| <= r with u in [0, 1), i.e. x - r - 0.5 < q <= x + r + 0.5
    // (floor / ceil keep a pixel of slack on either side against the rounding of the sums in AddSample)
    // (a probe's RenderView takes no samples outside the film's pixel bounds: those records do not exist)
    // (the path pass takes none outside the integrator's pixel bounds — the sample bounds unless "pixelbounds" was given)
    const int lo_x = P.probe_mode ? S.crop_x0 : S.pb_x0, hi_x = P.probe_mode ? S.crop_x1 : S.pb_x1;
    const int lo_y = P.probe_mode ? S.crop_y0 : S.pb_y0, hi_y = P.probe_mode ? S.crop_y1 : S.pb_y1;
    const int qx0 = max(int(floorf(float(x) - rx - 0.5f)), lo_x), qx1 = min(int(ceilf(float(x) + rx + 0.5f)), hi_x - 1);
    const int qy0 = max(int(floorf(float(y) - ry - 0.5f)), lo_y), qy1 = min(int(ceilf(float(y) + ry + 0.5f)), hi_y - 1);
    float4 out = make_float4(0, 0, 0, 0);
    if (qx0 <= qx1 && qy0 <= qy1) {
        const int tx0 = (qx0 - S.samp_x0) / kTile, tx1 = (qx1 - S.samp_x0) / kTile;
        const int ty0 = (qy0 - S.samp_y0) / kTile, ty1 = (qy1 - S.samp_y0) / kTile;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) {  // tile index order
                uint32_t slot = 0;  // (probe pass: the tiles here are the reference's, the records are found per pixel)
                if (!P.probe_mode && !tile_owned(P, tx, ty, &slot)) continue;
                const FilmTileBounds t = film_tile_bounds(S, tx, ty, rx, ry);
                if (!t.holds(x, y)) continue;  // the tile's FilmTile must hold (x, y)
                float r = 0, g = 0, b = 0, w = 0;
                const int ordinal = (ty - ty0) * (tx1 - tx0 + 1) + (tx - tx0);
                sums.load(ordinal, &r, &g, &b, &w);
                // FilmTile::AddSample's support test and table lookup for this pixel (film.h:159-188)
                auto add_sample = [&](float2 pf, float4 L) {
                    const float dxf = pf.x - 0.5f, dyf = pf.y - 0.5f;
                    const bool in = x >= support_lo(dxf, rx, t.fx0) && x < support_hi(dxf, rx, t.fx1) &&
                                    y >= support_lo(dyf, ry, t.fy0) && y < support_hi(dyf, ry, t.fy1);
                    if (in) {
                        const float ffx = fabsf((float(x) - dxf) * inv_rx * 16.f), ffy = fabsf((float(y) - dyf) * inv_ry * 16.f);
                        const int ifx = min(int(floorf(ffx)), 15), ify = min(int(floorf(ffy)), 15);
                        const float fwt = s_table[ify * 16 + ifx];
                        r += L.x * 1.f * fwt;
                        g += L.y * 1.f * fwt;
                        b += L.z * 1.f * fwt;
                        w += fwt;
                    }
                };
                const int xa = max(qx0, t.sx0), xb = min(qx1, t.sx1 - 1);
                for (int qy = max(qy0, t.sy0); qy <= min(qy1, t.sy1 - 1); ++qy) {
                    const size_t row = size_t(slot) * size_t(n_samples) * 256u + size_t((qy - t.sy0) * kTile - t.sx0);
                    if (n_samples == 1) {
                        // one sample per pixel (the probe pass): four neighbouring pixels' records in flight
                        for (int q4 = xa; q4 <= xb; q4 += 4) {
                            float2 pfb[4];
                            float4 Lb[4];
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) rec1(q4 + jj <= xb ? q4 + jj : q4, qy, row, &pfb[jj], &Lb[jj]);
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj)
                                if (q4 + jj <= xb) add_sample(pfb[jj], Lb[jj]);
                        }
                        continue;
                    }
                    for (int qx = xa; qx <= xb; ++qx) {
                        const size_t base = row + size_t(qx);
                        for (int k4 = 0; k4 < n_samples; k4 += 4) {
                            // four records in flight, then summed in sample order
                            float2 pfb[4];
                            float4 Lb[4];
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) {
                                const size_t at = base + size_t(k4 + jj < n_samples ? k4 + jj : k4) * 256u;
                                pfb[jj] = F.wide_pf[at];
                                Lb[jj] = F.wide_L[at];
                            }
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj)
                                if (k4 + jj < n_samples) add_sample(pfb[jj], Lb[jj]);
                        }
                    }
                }
                sums.store(ordinal, r, g, b, w);
                add_xyz(&out, r, g, b, w);
            }
    }
    return out;
}

}  // namespace iile
