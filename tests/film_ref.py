"""The film, from a camera sample's radiance to a pixel, restated in float64 from the reference alone.

  Filters      BoxFilter, TriangleFilter, GaussianFilter, MitchellFilter, LanczosSincFilter ::Evaluate and the parameter
               defaults of their Create functions (filters/box.cpp:41-47, triangle.cpp:41-51, gaussian.cpp:41-51 with
               gaussian.h:50-65, mitchell.cpp:41-52 with mitchell.h:50-63, sinc.cpp:41-50 with sinc.h:50-63)
  Table        Film::filterTable: entry [y][x] = Evaluate((x + .5) rx / 16, (y + .5) ry / 16) (core/film.cpp:65-74)
  Bounds       croppedPixelBounds = Ceil(resolution * cropwindow) (film.cpp:55-59), Film::GetSampleBounds (film.cpp:77-83),
               the path integrator's "pixelbounds" intersected with the sample bounds (integrators/path.cpp:216-229),
               SamplerIntegrator::Render's 16 x 16 sample tiles (core/integrator.cpp:227-255), Film::GetFilmTile's pixel
               bounds of a tile (film.cpp:92-103), the pixels that take samples (integrator.cpp:272)
  Guards       NaN, y < -1e-5, infinite y: black (integrator.cpp:293-314); y = RGBSpectrum::y (core/spectrum.h:463-466)
  AddSample    FilmTile::AddSample (core/film.h:153-193): the luminance clamp, pFilm - 0.5, Ceil / Floor + 1 clipped to the
               tile's pixel bounds, ifx / ify, the weight, contribSum and filterWeightSum
  Merge        Film::MergeFilmTile (film.cpp:135-148): RGBToXYZ (spectrum.h:62-66) per tile pixel, tiles summed
  Image        Film::to_rgb_array (film.cpp:187-225): XYZToRGB (spectrum.h:56-60), division by the weight sum, max(0, .),
               "scale" (the splat terms are zero: nothing here splats)

INPUTS. Per sample: the pixel it belongs to, its film position pFilm = pixel + (u0, u1) as the float32 pair the reference
forms (CameraSample::pFilm), and the radiance Li returned (float32 RGB). The filter's parameters, the resolution, the crop
window and the two film numbers are float32 / integer scene data held exactly. Everything after that is float64.
(The probes the tests take Li from return it after the guards; guard() is applied all the same and changes nothing then.)

u = 2^-24, one float32 rounding. Constants written with an f suffix in the reference (the colour matrices, YWeight, Pi) are
the float32 values, held exactly.

THE TABLE'S BAND (table_band): what a float32 evaluation of a table entry may differ by from the float64 one, per filter and
per entry, absolute. A coordinate p = (i + .5) r / 16 is two roundings: |dp| <= 2 u p. A product of two per-axis factors a, b
with bands ea, eb carries a eb + b ea + ea eb + u |a b|.
  box          1: exact.
  triangle     a = max(0, r - |p|): ea = 2 u p + u |r - p|.
  gaussian     a = max(0, exp(-alpha p^2) - exp(-alpha r^2)). The argument alpha p^2 is two products of a p with 2 u: 6 u
               relative; expf is taken within 2 u relative of the true exponential of its float32 argument; the constant's
               argument alpha r^2 carries 2 u relative (r is exact). With E = exp(-alpha p^2), V = exp(-alpha r^2):
               ea = E (6 u alpha p^2 + 2 u) + V (2 u alpha r^2 + 2 u) + u |E - V|. Near the support's edge E - V cancels: the
               band is absolute, so it stays of the size u V while the entry goes to zero.
  mitchell     x = |2 p / r| with p (2 u), 1 / r (u) and the product (u): 4 u relative. The cubic c3 x^3 + c2 x^2 + c1 x + c0
               times 1/6: a coefficient is at most three float32 operations on B, C (3 u of its absolute terms' sum, written
               |c_i| below for that sum), x^i is i products of an x with 4 u (5 i u relative), the sum is three additions
               (3 u of the absolute sum), the constant 1.f / 6.f and the last product 2 u:
               ea = u [sum_i |c_i| x^i (3 + 5 i) + 3 sum_i |c_i| x^i] / 6 + 2 u |a|. At the zero crossing of the outer cubic
               the absolute sum stays of order 10 while a vanishes: again an absolute band.
  sinc         a = Sinc(p) Sinc(p / tau) inside |p| <= r. Sinc(x) = sin(t) / t, t = Pi x: x carries k u relative (k = 2 for p,
               k = 4 for p / tau), Pi one u, the product one: dt = (k + 2) u t; sinf within 2 u relative of the true sine of
               its float32 argument; the quotient is one rounding and t's relative error again:
               es = (dt + 2 u |sin t|) / t + (k + 3) u |sin t / t| = about (2 k + 4) u absolute near a zero of a lobe, where
               the value itself vanishes. x < 1e-5 returns 1 exactly (no table coordinate comes that close to 0).
The host's table is asserted to lie within table_band of table().

THE FILM'S BAND. The reference adds, per tile pixel, the terms L_c w_i one after the other (film.h:189-190): each product is one
rounding, a sequential sum of n terms of absolute sum S is within (n - 1) u S: n u S_c, S_c = sum_i |w_i| |L_c,i|. A clamped
sample's L is first scaled by max / y: y is five roundings on non-negative terms, the quotient one, the product one: 7 u more on
its terms. RGBToXYZ is three products and two additions per output: 3 u of sum_c M_Xc S_c. Film::MergeFilmTile adds the tiles'
values: with T tiles reaching a pixel, T u more. And a table entry the reference evaluated in float32 differs from the truth's by
at most table_band: D_c = sum_i table_band[cell_i] |L_c,i|. So for X, Y, Z and the weight
    band_X = u (n + T + 10) sum_c M_Xc S_c + sum_c M_Xc D_c         band_w = u (n + T) sum_i |w_i| + sum_i table_band[cell_i]
with n the number of samples that reach the pixel (over all tiles: larger than any one tile's count) and T the number of tiles
whose pixel bounds hold it. Nothing in it is measured on an implementation.

THE FLAGS. Some decisions are discrete: whether a pixel lies inside a sample's support (Ceil(pd - r), Floor(pd + r) + 1, the
tile's bounds likewise), which table cell it reads (Floor(|(x - pd) invRadius 16|)), and whether a sample is clamped (y > max).
Film.accumulate takes each of them twice: from the float64 value of the expression (exact for these inputs up to 2^-53) and from
its float32 value computed with the reference's operations in the reference's order - a float32 value that lies within its own
rounding of an integer (or of the threshold) is exactly one for which the two disagree. Where they disagree for a (sample,
pixel) pair, the pair is flagged and the truth keeps both candidates: the film of the float64 decisions (value) and the film of
the float32 decisions (value32), both summed in float64 with the truth's table. A pixel's band widens by |value - value32| (slack).
No pixel is left out. The tests hold the share of flagged pairs to FLAG_CAP and the slack to SLACK_CAP of the pixel's value
(the absolute sums S above, through the matrix), as conditions on the cases.

FLOAT32 MODE. accumulate_float32 evaluates every step in single precision in the reference's order: tiles in index order, pixels
of a tile row by row, a pixel's samples in order, the support row by row; one float32 accumulator per tile pixel and channel,
RGBToXYZ in float32 left to right, tiles added in index order; the table is table(np.float32). It is what the reference's own
arithmetic gives up to libm, and it must lie inside the bands and the caps before any implementation is asked.
"""
import re
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
FLAG_CAP = 0.01   # share of flagged (sample, pixel) pairs a case may have
SLACK_CAP = 0.01  # |value - value32| a pixel may have, as a fraction of its absolute sums
TILE = 16         # integrator.cpp:234
TABLE = 16        # Film::filterTableWidth, film.h:71

_f = lambda *v: np.array(v, np.float32).astype(np.float64)  # noqa: E731  (float literals with an f suffix, held exactly)
RGB_TO_XYZ = np.stack([_f(0.412453, 0.357580, 0.180423), _f(0.212671, 0.715160, 0.072169), _f(0.019334, 0.119193, 0.950227)])
XYZ_TO_RGB = np.stack([_f(3.240479, -1.537150, -0.498535), _f(-0.969256, 1.875991, 0.041556), _f(0.055648, -0.204043, 1.057311)])
Y_WEIGHT = _f(0.212671, 0.715160, 0.072169)
PI32 = float(np.float32(3.14159265358979323846))

Filter = namedtuple("Filter", "kind rx ry alpha B C tau")


def parse_pixel_filter(line):
    """The Filter of a `PixelFilter "kind" "float name" [v] ...` line with the defaults of the reference's Create functions
    (api.cpp's default is the box filter); every number is the float32 the parser stores."""
    kind = re.search(r'PixelFilter\s+"(\w+)"', line).group(1) if line.strip() else "box"
    given = {m.group(1): float(np.float32(float(m.group(2)))) for m in re.finditer(r'"float (\w+)"\s*\[\s*([-+.\deE]+)\s*\]', line)}
    third = float(np.float32(1.0) / np.float32(3.0))
    w = {"box": 0.5, "triangle": 2.0, "gaussian": 2.0, "mitchell": 2.0, "sinc": 4.0}[kind]
    return Filter(kind, given.get("xwidth", w), given.get("ywidth", w), given.get("alpha", 2.0), given.get("B", third),
                  given.get("C", third), given.get("tau", 3.0))


def _axis(flt, r, i, dtype):
    """(factor, band) of one axis at the table coordinates p = (i + .5) r / 16 (film.cpp:70-71), for the separable filters."""
    T = dtype
    p = (i.astype(T) + T(0.5)) * T(r) / T(TABLE)
    if flt.kind == "box":
        return np.ones_like(p), np.zeros(len(p))
    if flt.kind == "triangle":  # triangle.cpp:41-44
        a = np.maximum(T(0), T(r) - np.abs(p))
        return a, 2 * U * p + U * np.abs(r - p)
    if flt.kind == "gaussian":  # gaussian.h:53-54, 63-65
        al = T(flt.alpha)
        E, V = np.exp(-al * p * p), np.exp(-al * T(r) * T(r))
        a = np.maximum(T(0), (E - V).astype(T))
        return a, E * (6 * U * flt.alpha * p * p + 2 * U) + V * (2 * U * flt.alpha * r * r + 2 * U) + U * np.abs(E - V)
    if flt.kind == "mitchell":  # mitchell.h:53-63, mitchell.cpp:41-43
        B, C = T(flt.B), T(flt.C)
        x = np.abs(T(2) * (p * (T(1) / T(r))))
        outer = ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) * (T(1) / T(6))
        inner = ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) * (T(1) / T(6))
        a = np.where(x > 1, outer, inner)
        b, c = abs(flt.B), abs(flt.C)
        co = np.where((x > 1)[:, None], [8 * b + 24 * c, 12 * b + 48 * c, 6 * b + 30 * c, b + 6 * c], [6 + 2 * b, 0, 18 + 12 * b + 6 * c, 12 + 9 * b + 6 * c])
        terms = co * np.abs(x.astype(np.float64))[:, None] ** np.arange(4)
        return a, U * ((terms * (3 + 5 * np.arange(4))).sum(1) + 3 * terms.sum(1)) / 6 + 2 * U * np.abs(a)
    if flt.kind == "sinc":  # sinc.h:53-63, sinc.cpp:41-43
        pi = T(PI32) if T is np.float32 else T(np.pi)

        def sinc(x, k):
            t = pi * x
            s = np.sin(t) / t
            return np.where(x < 1e-5, T(1), s), ((k + 2) * U * t + 2 * U * np.abs(np.sin(t))) / t + (k + 3) * U * np.abs(s)
        x = np.abs(p)
        s1, e1 = sinc(x, 2)
        s2, e2 = sinc(x / T(flt.tau), 4)
        a = np.where(x > r, T(0), s1 * s2)
        return a, np.abs(s1) * e2 + np.abs(s2) * e1 + e1 * e2 + U * np.abs(a)
    raise ValueError(flt.kind)


def table(flt, dtype=np.float64):
    """Film::filterTable as a (16, 16) array [y][x] of `dtype`, every operation in `dtype`."""
    i = np.arange(TABLE)
    ax, _ = _axis(flt, flt.rx, i, dtype)
    ay, _ = _axis(flt, flt.ry, i, dtype)
    return (ay[:, None] * ax[None, :]).astype(dtype)


def table_band(flt):
    """What a float32 evaluation of table(flt) may differ by, (16, 16), absolute (the module's docstring)."""
    if flt.kind == "box":  # Evaluate returns 1: no operation at all
        return np.zeros((TABLE, TABLE))
    i = np.arange(TABLE)
    ax, ex = _axis(flt, flt.rx, i, np.float64)
    ay, ey = _axis(flt, flt.ry, i, np.float64)
    ax, ay = np.abs(ax), np.abs(ay)
    return ay[:, None] * ex[None, :] + ey[:, None] * ax[None, :] + ey[:, None] * ex[None, :] + U * ay[:, None] * ax[None, :]


def guard(L):
    """SamplerIntegrator::Render's three guards (integrator.cpp:293-314) on (n, 3) radiance: a copy, black where one applies."""
    L = np.array(L, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = L @ Y_WEIGHT
    bad = np.isnan(L).any(1) | (y < -1e-5) | np.isinf(y)
    L[bad] = 0
    return L


FilmValue = namedtuple("FilmValue", "value value32 band slack scale n_pairs n_flagged n_clamped n_unclamped")


class Film:
    """The film of one scene: Film's constructor, GetSampleBounds, the integrator's pixel bounds and the tiles."""

    def __init__(self, xres, yres, flt, crop=(0, 1, 0, 1), pixel_bounds=None, scale=1.0, max_sample_luminance=np.inf):
        self.flt, self.scale, self.max_lum = flt, float(np.float32(scale)), float(np.float32(max_sample_luminance))
        c = [float(np.float32(v)) for v in crop]  # CreateFilm, film.cpp:286-294: {x0, x1, y0, y1}, sorted and clamped
        cx0, cx1 = np.clip([min(c[0], c[1]), max(c[0], c[1])], 0, 1)
        cy0, cy1 = np.clip([min(c[2], c[3]), max(c[2], c[3])], 0, 1)
        ceil = lambda v: int(np.ceil(v))  # noqa: E731
        self.crop = (ceil(xres * cx0), ceil(yres * cy0), ceil(xres * cx1), ceil(yres * cy1))  # x0, y0, x1, y1 (film.cpp:55-59)
        x0, y0, x1, y1 = self.crop
        self.samp = (int(np.floor(x0 + 0.5 - flt.rx)), int(np.floor(y0 + 0.5 - flt.ry)),
                     ceil(x1 - 0.5 + flt.rx), ceil(y1 - 0.5 + flt.ry))  # film.cpp:77-83
        pb = self.samp
        if pixel_bounds is not None:  # path.cpp:216-229: {x0, x1, y0, y1}
            q = pixel_bounds
            pb = (max(pb[0], q[0]), max(pb[1], q[2]), min(pb[2], q[1]), min(pb[3], q[3]))
        self.pixel_bounds = pb
        self.ntx = (self.samp[2] - self.samp[0] + TILE - 1) // TILE  # integrator.cpp:232-237
        self.nty = (self.samp[3] - self.samp[1] + TILE - 1) // TILE
        self.table = table(flt)
        self.table_band = table_band(flt)

    @property
    def shape(self):
        return (self.crop[3] - self.crop[1], self.crop[2] - self.crop[0])

    def sample_pixels(self):
        """(px, py) of every pixel that takes samples (integrator.cpp:262-273), in raster order."""
        s, b = self.samp, self.pixel_bounds
        x0, y0 = max(s[0], b[0]), max(s[1], b[1])
        ys, xs = np.mgrid[y0:max(y0, min(s[3], b[3])), x0:max(x0, min(s[2], b[2]))]
        return xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)

    def tile_of(self, px, py):
        """(tx, ty) of the sample tile a pixel lies in."""
        return (np.asarray(px) - self.samp[0]) // TILE, (np.asarray(py) - self.samp[1]) // TILE

    def _tile_pixel_bounds(self, tx, ty, T):
        """Film::GetFilmTile (film.cpp:92-103) for tiles (tx, ty), every operation in T: x0, y0, x1, y1 arrays."""
        out = []
        for t, s0, s1, r, c0, c1 in ((tx, self.samp[0], self.samp[2], self.flt.rx, self.crop[0], self.crop[2]),
                                     (ty, self.samp[1], self.samp[3], self.flt.ry, self.crop[1], self.crop[3])):
            lo = s0 + np.asarray(t) * TILE
            hi = np.minimum(lo + TILE, s1)
            p0 = np.ceil(lo.astype(T) - T(0.5) - T(r)).astype(np.int64)
            p1 = np.floor(hi.astype(T) - T(0.5) + T(r)).astype(np.int64) + 1
            out.append((np.maximum(p0, c0), np.minimum(p1, c1)))
        return out[0][0], out[1][0], out[0][1], out[1][1]

    def _support(self, pfilm, tx, ty, T):
        """film.h:159-164 in T: pd (n, 2), p0x, p0y, p1x, p1y clipped to the tile's pixel bounds."""
        pd = pfilm.astype(T) - T(0.5)
        bx0, by0, bx1, by1 = self._tile_pixel_bounds(tx, ty, T)
        r = (T(self.flt.rx), T(self.flt.ry))
        p0x = np.maximum(np.ceil(pd[:, 0] - r[0]).astype(np.int64), bx0)
        p0y = np.maximum(np.ceil(pd[:, 1] - r[1]).astype(np.int64), by0)
        p1x = np.minimum(np.floor(pd[:, 0] + r[0]).astype(np.int64) + 1, bx1)
        p1y = np.minimum(np.floor(pd[:, 1] + r[1]).astype(np.int64) + 1, by1)
        return pd, p0x, p0y, p1x, p1y

    def _cell(self, x, pd, r, T):
        """film.h:171-173 in T. The float64 value divides by the radius: invRadius is a float32 rounding of the reference's own."""
        d = x.astype(T) - pd
        f = np.abs(d * (T(1) / T(r)) * T(TABLE)) if T is np.float32 else np.abs(d / r * TABLE)
        return np.minimum(np.floor(f).astype(np.int64), TABLE - 1)

    def _clamp(self, L, T):
        """film.h:156-157 in T: (L scaled where y > max, clamped?)."""
        L = L.astype(T)
        y = T(Y_WEIGHT[0]) * L[:, 0] + T(Y_WEIGHT[1]) * L[:, 1] + T(Y_WEIGHT[2]) * L[:, 2]
        hit = y > T(self.max_lum)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(hit, T(self.max_lum) / np.where(hit, y, T(1)), T(1)).astype(T)
        return L * s[:, None], hit

    def accumulate(self, px, py, pfilm, L, owned=None):
        """The {X, Y, Z, weight} film of the samples (pixel (px, py), film position pfilm (n, 2) float32, radiance L (n, 3)
        float32) as a FilmValue of (h, w, 4) float64 arrays. owned: a (nty, ntx) mask of the tiles whose samples count."""
        px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
        pfilm = np.ascontiguousarray(pfilm, np.float32)
        assert pfilm.dtype == np.float32 and len(px) == len(py) == len(pfilm) == len(L)
        tx, ty = self.tile_of(px, py)
        if owned is not None:
            keep = np.asarray(owned, bool)[ty, tx]
            px, py, pfilm, L, tx, ty = px[keep], py[keep], pfilm[keep], np.asarray(L)[keep], tx[keep], ty[keep]
        Lg = guard(L)
        L64, hit64 = self._clamp(Lg, np.float64)
        L32, hit32 = self._clamp(Lg, np.float32)  # only its decision is used
        Lalt = np.where((hit32 != hit64)[:, None], np.where(hit32[:, None], L32.astype(np.float64), Lg), L64)
        h, w = self.shape
        P = h * w
        cx0, cy0 = self.crop[0], self.crop[1]
        s64 = self._support(pfilm, tx, ty, np.float64)
        s32 = self._support(pfilm, tx, ty, np.float32)
        bx = np.minimum(s64[1], s32[1])
        by = np.minimum(s64[2], s32[2])
        nx = int(max(0, (np.maximum(s64[3], s32[3]) - bx).max(initial=0)))
        ny = int(max(0, (np.maximum(s64[4], s32[4]) - by).max(initial=0)))
        acc = {k: np.zeros((P, 4)) for k in ("a", "b", "abs", "tab")}
        count = np.zeros(P)
        n_pairs = n_flagged = 0
        tab, tband = self.table.ravel(), self.table_band.ravel()
        absL = np.abs(L64)

        def add(dst, idx, w_, Lc):
            for c in range(3):
                dst[:, c] += np.bincount(idx, weights=w_ * Lc[:, c], minlength=P)
            dst[:, 3] += np.bincount(idx, weights=w_, minlength=P)

        for jy in range(ny):
            y = by + jy
            iy64, iy32 = self._cell(y, s64[0][:, 1], self.flt.ry, np.float64), self._cell(y, s32[0][:, 1], self.flt.ry, np.float32)
            in_y64, in_y32 = (y >= s64[2]) & (y < s64[4]), (y >= s32[2]) & (y < s32[4])
            for jx in range(nx):
                x = bx + jx
                in64 = in_y64 & (x >= s64[1]) & (x < s64[3])
                in32 = in_y32 & (x >= s32[1]) & (x < s32[3])
                either = in64 | in32
                if not either.any():
                    continue
                c64 = iy64 * TABLE + self._cell(x, s64[0][:, 0], self.flt.rx, np.float64)
                c32 = iy32 * TABLE + self._cell(x, s32[0][:, 0], self.flt.rx, np.float32)
                n_pairs += int(either.sum())
                flagged = int(((in64 != in32) | (either & ((c64 != c32) | (hit64 != hit32)))).sum())
                n_flagged += flagged
                pix = (y - cy0) * w + (x - cx0)
                m = in64
                one = np.zeros((P, 4))
                add(one, pix[m], tab[c64[m]], L64[m])
                acc["a"] += one
                add(acc["abs"], pix[m], np.abs(tab[c64[m]]), absL[m])
                if tband.any():
                    add(acc["tab"], pix[m], tband[c64[m]], absL[m])
                count += np.bincount(pix[m], minlength=P)
                if flagged:
                    m = in32
                    add(acc["b"], pix[m], tab[c32[m]], Lalt[m])
                else:  # the float32 decisions are the float64 ones at this offset
                    acc["b"] += one
        tiles = np.zeros((h, w))  # T: the tiles whose pixel bounds hold a pixel
        tys, txs = np.mgrid[0:self.nty, 0:self.ntx]
        for x0, y0, x1, y1 in zip(*self._tile_pixel_bounds(txs.ravel(), tys.ravel(), np.float64)):
            tiles[max(0, y0 - cy0):max(0, y1 - cy0), max(0, x0 - cx0):max(0, x1 - cx0)] += 1
        M4 = np.zeros((4, 4))
        M4[:3, :3], M4[3, 3] = RGB_TO_XYZ, 1
        to = lambda a: (a @ M4.T).reshape(h, w, 4)  # noqa: E731  MergeFilmTile: linear, so the tiles' order does not matter here
        n = count.reshape(h, w, 1)
        T = tiles[..., None]
        scale = to(acc["abs"])
        band = U * (n + T + np.array([10, 10, 10, 0])) * scale + to(acc["tab"])
        value, value32 = to(acc["a"]), to(acc["b"])
        return FilmValue(value, value32, band, np.abs(value - value32), scale, n_pairs, n_flagged, int(hit64.sum()), int((~hit64).sum()))

    def accumulate_float32(self, px, py, pfilm, L, owned=None):
        """The same film, every step in float32 in the reference's order (the module's docstring): (h, w, 4) float32. The
        samples are given pixel by pixel in raster order, a pixel's samples in order."""
        T = np.float32
        px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
        pfilm = np.ascontiguousarray(pfilm, np.float32)
        tx, ty = self.tile_of(px, py)
        tile = ty * self.ntx + tx
        order = np.lexsort((np.arange(len(px)), px, py, tile))  # tile, then the pixels of the tile row by row, then as given
        if owned is not None:
            order = order[np.asarray(owned, bool)[ty[order], tx[order]]]
        px, py, pfilm, tx, ty, tile = px[order], py[order], pfilm[order], tx[order], ty[order], tile[order]
        Lc, _ = self._clamp(guard(np.asarray(L)[order]).astype(T), T)
        pd, p0x, p0y, p1x, p1y = self._support(pfilm, tx, ty, T)
        nx, ny = int(max(0, (p1x - p0x).max(initial=0))), int(max(0, (p1y - p0y).max(initial=0)))
        tab = table(self.flt, T).ravel()
        # every (sample, pixel) pair, in the order AddSample visits them: sample-major, then y, then x
        sid, dst, wgt = [], [], []
        for jy in range(ny):
            y = p0y + jy
            iy = self._cell(y, pd[:, 1], self.flt.ry, T)
            for jx in range(nx):
                x = p0x + jx
                m = (y < p1y) & (x < p1x)
                if not m.any():
                    continue
                ix = self._cell(x, pd[:, 0], self.flt.rx, T)
                sid.append(np.flatnonzero(m) * (nx * ny) + jy * nx + jx)
                dst.append(np.stack([tile[m], y[m], x[m]], 1))
                wgt.append(tab[iy[m] * TABLE + ix[m]])
        h, w = self.shape
        film = np.zeros((h * w, 4), T)
        if not sid:
            return film.reshape(h, w, 4)
        sid, dst, wgt = np.concatenate(sid), np.concatenate(dst), np.concatenate(wgt)
        o = np.argsort(sid, kind="stable")
        sample, dst, wgt = sid[o] // (nx * ny), dst[o], wgt[o]
        # one accumulator per (tile, pixel): np.add.at adds in the order of the index array, in float32
        key = (dst[:, 0] * h + (dst[:, 1] - self.crop[1])) * w + (dst[:, 2] - self.crop[0])
        uniq, slot = np.unique(key, return_inverse=True)
        tp = np.zeros((len(uniq), 4), T)
        contrib = np.empty((len(sample), 4), T)
        contrib[:, :3] = Lc[sample] * T(1) * wgt[:, None]
        contrib[:, 3] = wgt
        np.add.at(tp, slot, contrib)
        M = RGB_TO_XYZ.astype(T)
        xyz = np.stack([M[i, 0] * tp[:, 0] + M[i, 1] * tp[:, 1] + M[i, 2] * tp[:, 2] for i in range(3)] + [tp[:, 3]], 1).astype(T)
        np.add.at(film, uniq % (h * w), xyz)  # uniq is sorted by tile first: the tiles are merged in index order
        return film.reshape(h, w, 4)

    def to_rgb(self, film, dtype=np.float64):
        """Film::to_rgb_array (film.cpp:187-225) of an (h, w, 4) film: (rgb, band), band = 6 u scale sum_c |M_rc| |xyz_c| / |w|
        (three products and two additions: 3 u of the absolute sum; 1 / w, the product with it and with scale: 3 u more)."""
        f = np.asarray(film, dtype)
        M = XYZ_TO_RGB.astype(dtype)
        rgb = f[..., :3] @ M.T
        w = f[..., 3:4]
        live = w != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            rgb = np.where(live, np.maximum(0, rgb * (1 / np.where(live, w, 1))), rgb)
            mag = np.abs(f[..., :3].astype(np.float64)) @ np.abs(XYZ_TO_RGB).T / np.where(live, np.abs(w), 1)
        return rgb * dtype(self.scale), 6 * U * self.scale * mag


def compare(got, want):
    """(worst distance as a fraction of band + slack, per-pixel fraction array) of an (h, w, 4) film against a FilmValue; a pixel
    whose band is zero must be matched exactly (fraction 0 or inf)."""
    d = np.abs(np.asarray(got, np.float64) - want.value)
    tol = want.band + want.slack
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(d == 0, 0.0, d / tol)
    return float(frac.max(initial=0)), frac


def caps(want):
    """(share of flagged pairs, worst slack as a fraction of the pixel's absolute sums): both are held to the caps."""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(want.slack == 0, 0.0, want.slack / want.scale)
    return want.n_flagged / max(1, want.n_pairs), float(s.max(initial=0))
