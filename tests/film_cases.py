"""Scenes, cases and comparisons for the film's float64 truth (film_ref.py), shared by test_film_truth.py (the oracle, on the
CPU) and test_gpu_film_truth.py (the device).

The content can see a wrong weight: a small emitter of saturated radiance (4, .5, .1) in front of differently coloured matte
walls under a point light, black background beside them, at maxdepth 1 - neighbouring samples differ by more than an order of
magnitude and per channel, so a pixel's value depends on which weight each neighbour's sample was given and on every entry of
the colour matrices. (In a furnace, or on grey, it depends on neither.) The box room adds a frame with texture-free but busy
content at a size of several tiles in both axes."""
from collections import namedtuple

import numpy as np

import film_ref as FR
from boxroom import boxroom_pbrt
from test_oracle_pins import FILTERS

MAX_LUM = 0.5  # between the walls' luminance (below 0.35) and the emitter's (1.21)

_COLOUR = '''LookAt 0 -6 1   0 0 1   0 0 1
Camera "perspective" "float fov" [32]
Film "image" "integer xresolution" [%d] "integer yresolution" [%d]%s
%s
Sampler "halton" "integer pixelsamples" [%d]%s
Integrator "path" "integer maxdepth" [1]%s
WorldBegin
LightSource "point" "color I" [30 24 18] "point from" [1 -3 3.5]
AttributeBegin
  Material "matte" "color Kd" [.8 .1 .1]
  Shape "trianglemesh" "point P" [ -2.2 3 -1   3 3 -1   3 3 2.6   -2.2 3 2.6 ] "integer indices" [ 0 1 2   0 2 3 ]
AttributeEnd
AttributeBegin
  Material "matte" "color Kd" [.1 .7 .2]
  Shape "trianglemesh" "point P" [ -4 -2 -1   3 -2 -1   3 3 -1   -4 3 -1 ] "integer indices" [ 0 1 2   0 2 3 ]
AttributeEnd
AttributeBegin
  Material "matte" "color Kd" [.1 .2 .9]
  Shape "trianglemesh" "point P" [ -2.2 -2 -1   -2.2 3 -1   -2.2 3 2.2   -2.2 -2 2.2 ] "integer indices" [ 0 1 2   0 2 3 ]
AttributeEnd
AttributeBegin
  Material "matte" "color Kd" [0 0 0]
  AreaLightSource "diffuse" "color L" [4 .5 .1] "bool twosided" ["true"]
  Shape "trianglemesh" "point P" [ -.7 1 .6   .5 1 .6   .5 1 1.5   -.7 1 1.5 ] "integer indices" [ 0 1 2   0 2 3 ]
AttributeEnd
WorldEnd
'''

Case = namedtuple("Case", "name content xres yres spp filter film sampler_opts integrator sobol crop pixel_bounds scale max_lum")


def _case(name, content, xres, yres, spp, filt, crop=None, pixel_bounds=None, scale=None, max_lum=None, center=False, sobol=False):
    film = ""
    if crop is not None:
        film += ' "float cropwindow" [%s]' % " ".join("%.9g" % v for v in crop)
    if scale is not None:
        film += ' "float scale" [%.9g]' % scale
    if max_lum is not None:
        film += ' "float maxsampleluminance" [%.9g]' % max_lum
    integ = ' "integer pixelbounds" [%d %d %d %d]' % tuple(pixel_bounds) if pixel_bounds is not None else ""
    return Case(name, content, xres, yres, spp, filt, film, ' "bool samplepixelcenter" ["true"]' if center else "", integ, sobol,
                crop or (0, 1, 0, 1), pixel_bounds, scale if scale is not None else 1.0, max_lum if max_lum is not None else np.inf)


def _fname(i):
    return "f%d-%s" % (i, FILTERS[i].split('"')[1])


CASES = [_case("small-" + _fname(i), "colour", 12, 10, 4, FILTERS[i]) for i in range(9)]           # border-dominated
CASES += [_case("tiles-" + _fname(i), "colour", 40, 24, 3, FILTERS[i]) for i in range(9)]          # several tiles, ragged last tile
CASES += [_case("room-" + _fname(i), "room", 96, 64, 4, FILTERS[i]) for i in (0, 2, 4, 6, 8)]      # one per filter class
for _i in (1, 8):
    CASES.append(_case("crop-in-tile-" + _fname(_i), "colour", 40, 24, 3, FILTERS[_i], crop=(0.375, 0.5625, 0.25, 0.5625)))
for _i in (3, 7):
    CASES.append(_case("crop-ragged-" + _fname(_i), "colour", 40, 24, 3, FILTERS[_i], crop=(0.25, 0.75, 0.2, 0.9)))
for _i in (0, 8):
    CASES.append(_case("pixelbounds-" + _fname(_i), "colour", 40, 24, 3, FILTERS[_i], pixel_bounds=(5, 30, 3, 19)))
for _i in (0, 2, 6, 8):  # whole-number pd with a whole-number radius: |x - pd| = r, the table index is 16 before its clamp
    CASES.append(_case("pixelcenter-" + _fname(_i), "colour", 40, 24, 3, FILTERS[_i], center=True))
CASES.append(_case("scale-" + _fname(4), "colour", 40, 24, 3, FILTERS[4], scale=2.5))
for _i in (2, 8):
    CASES.append(_case("maxlum-" + _fname(_i), "colour", 40, 24, 3, FILTERS[_i], max_lum=MAX_LUM))
for _i in (0, 8):
    CASES.append(_case("sobol-" + _fname(_i), "colour", 40, 24, 4, FILTERS[_i], sobol=True))
BY_NAME = {c.name: c for c in CASES}
WIDE = [c.name for c in CASES if c.filter != FILTERS[8]]  # the store + gather film path
BOX = [c.name for c in CASES if c.filter == FILTERS[8]]   # the box fast path with the exact finish


def scene_text(case):
    if case.content == "colour":
        return _COLOUR % (case.xres, case.yres, case.film, case.filter, case.spp, case.sampler_opts, case.integrator)
    text = boxroom_pbrt(xres=case.xres, yres=case.yres, spp=case.spp, ico_levels=2, n_blobs=5, wall_n=6, maxdepth=3)
    assert not (case.film or case.sampler_opts or case.integrator)
    return text.replace('Sampler "halton"', case.filter + '\nSampler "halton"', 1)


def load(binding, directory, case):
    """(HostScene, film_ref.Film) of a case; the scene file is written into `directory`."""
    path = directory / (case.name + ".pbrt")
    path.write_text(scene_text(case))
    host = binding.HostScene(path=str(path), **({"sampler": "sobol"} if case.sobol else {}))
    truth = FR.Film(case.xres, case.yres, FR.parse_pixel_filter(case.filter), crop=case.crop, pixel_bounds=case.pixel_bounds,
                    scale=case.scale, max_sample_luminance=case.max_lum)
    return host, truth


def check_bounds(host, truth):
    """The truth's cropped pixel bounds, sample bounds, radii and pixel bounds are the loaded scene's."""
    f = host.film
    assert (f.crop_x0, f.crop_y0, f.crop_x1, f.crop_y1) == truth.crop
    assert (f.samp_x0, f.samp_y0, f.samp_x1, f.samp_y1) == truth.samp
    assert (f.filter_rx, f.filter_ry) == (truth.flt.rx, truth.flt.ry)
    assert tuple(host.scene_desc().integrator.pixel_bounds) == truth.pixel_bounds
    assert f.scale == np.float32(truth.scale) and f.max_sample_luminance == np.float32(truth.max_lum)


def sample_list(truth, k_begin, k_end):
    """(px, py, k) of every sample of the pixels that take samples: pixel by pixel in raster order, k in order."""
    px, py = truth.sample_pixels()
    n = k_end - k_begin
    return np.repeat(px, n), np.repeat(py, n), np.tile(np.arange(k_begin, k_end, dtype=np.int32), len(px))


def pfilm_of(px, py, u):
    """CameraSample::pFilm = (Point2f)pixel + Get2D() (sampler.cpp:46-52), in float32."""
    return np.stack([px.astype(np.float32) + u[:, 0].astype(np.float32), py.astype(np.float32) + u[:, 1].astype(np.float32)], 1)


def oracle_inputs(oracle, host, truth, k_begin, k_end):
    """(px, py, pfilm, L) per sample from the oracle's probes: Oracle.li, sample_index and dimensions 0 and 1."""
    px, py, k = sample_list(truth, k_begin, k_end)
    u = np.empty((len(px), 2), np.float32)
    for i in range(len(px)):
        idx = oracle.sample_index(host, px[i], py[i], k[i])
        u[i] = oracle.sample_dimension(host, idx, 0, px[i], py[i]), oracle.sample_dimension(host, idx, 1, px[i], py[i])
    L, _ = oracle.li(host, px, py, k)
    return px, py, pfilm_of(px, py, u), L


def device_inputs(gpu, truth, k_begin, k_end):
    """The same from the device's probes: GpuScene.li_samples and halton_samples(.., 0, 2)."""
    px, py, k = sample_list(truth, k_begin, k_end)
    u, _ = gpu.halton_samples(px, py, k, 0, 2)
    L, _ = gpu.li_samples(px, py, k)
    return px, py, pfilm_of(px, py, u), L


def owned_tiles(oracle, truth, rank, nranks):
    """(nty, ntx) mask of the tiles of shard `rank`, from Oracle.tile_owner."""
    return np.array([[oracle.tile_owner(tx, ty, nranks) == rank for tx in range(truth.ntx)] for ty in range(truth.nty)], bool).reshape(
        truth.nty, truth.ntx)


def check_caps(name, want):
    """The two conditions on a case: flagged pairs at most FLAG_CAP of all, slack at most SLACK_CAP of the pixel's value."""
    share, slack = FR.caps(want)
    assert share <= FR.FLAG_CAP, (name, share)
    assert slack <= FR.SLACK_CAP, (name, slack)
    return share, slack


def check_film(name, film, want):
    """`film` lies within the truth's band (+ the flagged pairs' slack) at every pixel and channel; returns the worst distance as
    a fraction of it."""
    assert film.shape == want.value.shape, name
    worst, frac = FR.compare(film, want)
    bad = int((frac > 1).any(axis=2).sum())
    assert bad == 0, f"{name}: {bad} of {frac.shape[0] * frac.shape[1]} pixels outside the band, worst {worst:.3g} of it"
    return worst
