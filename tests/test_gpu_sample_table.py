"""The sample table (DScene::stab_*, built at iile_scene_create): every Halton sample a frame can draw, tabulated per
(pixel mod 128, k). The table changes where the samples come from and nothing else, so every check here is bitwise:

* its entries against iile_halton_samples (the digit chains) for the same pixel, sample and dimensions;
* films of one scene file rendered by two handles of one process, one created with IILE_NO_SAMPLE_TABLE set;
* a scene over the byte budget (lowered through the test probe) has no table and renders the same film;
* the probe pass, whose sampler is not the frame's, is untouched by a table.

Scenes: killeroo-simple and tests/boxroom.py at 160 x 136 or less (wider and taller than 128, so pixel classes wrap) and
3 - 4 spp."""
import numpy as np
import pytest

import boxroom

pytestmark = pytest.mark.gpu

W, H = 160, 136


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {a.size} words differ"


def _table_bytes(spp, maxdepth, lens=False):
    return 16384 * spp * (32 * maxdepth + (16 if lens else 8))


@pytest.fixture(scope="module")
def scenes(binding, tmp_path_factory):
    d = tmp_path_factory.mktemp("sample_table")

    def room(name, edit=(), **kw):
        kw.setdefault("xres", 96)
        kw.setdefault("yres", 80)
        kw.setdefault("spp", 4)
        text = boxroom.boxroom_pbrt(ico_levels=1, n_blobs=5, wall_n=4, **kw)
        for old, new in edit:
            assert old in text
            text = text.replace(old, new, 1)
        p = d / (name + ".pbrt")
        p.write_text(text)
        return binding.HostScene(path=str(p))

    gauss = ("WorldBegin", 'PixelFilter "gaussian" "float xwidth" [2.5] "float ywidth" [2.5]\nWorldBegin')
    crop = ('"integer yresolution"', '"float cropwindow" [.25 .75 .25 .75] "integer yresolution"')
    lens = ('"float fov" [55]', '"float fov" [55] "float lensradius" [.15] "float focaldistance" [9]')
    center = ('"integer pixelsamples" [4]', '"integer pixelsamples" [4] "bool samplepixelcenter" ["true"]')
    return {
        # the entries test: 160 x 136 at 3 spp, maxdepth 5; a 5 x 5 gaussian filter puts sample-bound pixels at negative
        # coordinates, the crop window starts the sample bounds at pixel (38, 32)
        "wide": room("wide", [gauss], xres=W, yres=H, spp=3),
        "crop": room("crop", [gauss, crop], xres=W, yres=H, spp=3),
        "lens3": room("lens3", [lens], xres=W, yres=H, spp=3),
        # the film tests
        "killeroo": binding.HostScene(xres=W, yres=H, spp=4),
        "all": room("all", materials="all"),
        "dim8": room("dim8", maxdepth=8),
        "lens": room("lens", [lens]),
        "center": room("center", [center]),
        "textured": room("textured", textures=str(d / "tex")),
        "plain": room("plain", xres=64, yres=48),
        # an infinite light: no camera rays made inside k_extend, so k_generate reads the camera part and leaves the slot in hindex
        "sky": room("sky", [lens], light="sky"),
        "sobol": binding.HostScene(path=str(d / "plain.pbrt"), sampler="sobol"),
    }


def _pair(binding, monkeypatch, scene):
    """Two handles of one scene: with the table, and created under IILE_NO_SAMPLE_TABLE."""
    monkeypatch.delenv("IILE_NO_SAMPLE_TABLE", raising=False)
    on = binding.GpuScene(scene)
    monkeypatch.setenv("IILE_NO_SAMPLE_TABLE", "1")
    off = binding.GpuScene(scene)
    monkeypatch.delenv("IILE_NO_SAMPLE_TABLE")
    return on, off


@pytest.mark.parametrize("name", ["wide", "crop", "lens3"])
def test_table_entries_are_the_chains_values(binding, scenes, name):
    """Every k, every bounce and the camera part of the table against iile_halton_samples, bit for bit."""
    scene = scenes[name]
    spp, depth = 3, 5
    assert scene.info["spp"] == spp and scene.info["max_depth"] == depth
    gpu = binding.GpuScene(scene)
    pixels = [(0, 0), (127, 127), (128, 128), (159, 135),
              (38, 32),                 # first sample-bound pixel of the cropped, filtered film
              (-2, -2), (-1, 130)]      # sample-bound pixels of the 5 x 5 filter left of / above the film
    px = np.array([p[0] for p in pixels for _ in range(spp)], np.int32)
    py = np.array([p[1] for p in pixels for _ in range(spp)], np.int32)
    k = np.array([kk for _ in pixels for kk in range(spp)], np.int32)
    for b in range(depth):
        want, _ = gpu.halton_samples(px, py, k, 5 + 7 * b, 8)
        got = gpu.sample_table_records(px, py, k, np.full(len(px), b, np.int32))
        _same(got, want, f"{name}: records of bounce {b}")
    cam = gpu.sample_table_records(px, py, k, np.full(len(px), -1, np.int32))
    want01, _ = gpu.halton_samples(px, py, k, 0, 2)
    _same(cam[:, :2], want01, f"{name}: film dimensions")
    if name == "lens3":
        want34, _ = gpu.halton_samples(px, py, k, 3, 2)
        _same(cam[:, 2:4], want34, f"{name}: lens dimensions")
    else:
        assert not cam[:, 2:].any()
    st = gpu.render(k_begin=0, k_end=1)[1]
    assert st["sample_table_bytes"] == _table_bytes(spp, depth, lens=(name == "lens3"))


FILMS = [("killeroo", {}), ("all", {}), ("dim8", {}), ("lens", {}), ("center", {}), ("textured", {}), ("sky", {}),
         ("plain", {"spp_per_pass": 1}), ("plain", {"tile_rank": 1, "tile_nranks": 2})]


@pytest.mark.parametrize("name,kw", FILMS, ids=[n + "".join("-" + k for k in kw) for n, kw in FILMS])
def test_film_with_table_equals_film_by_chains(binding, scenes, monkeypatch, name, kw):
    """all: mirror and glass leave a wavefront's lanes at different dimensions (the per-lane chains of the table build);
    dim8: the roulette draws of bounces > 3 do; lens / center: the camera part in the camera-ray k_extend and the first k_shade;
    textured: in the textured k_shade's differentials; sky (an infinite light and an open lens): in k_generate, which runs in place
    of the camera-ray k_extend there and hands k_shade the slot through PassBuffers::hindex."""
    scene = scenes[name]
    on, off = _pair(binding, monkeypatch, scene)
    film_on, st_on = on.render(**kw)
    film_off, st_off = off.render(**kw)
    assert st_on["sample_table_bytes"] == _table_bytes(scene.info["spp"], scene.info["max_depth"], lens=(name in ("lens", "sky")))
    assert st_off["sample_table_bytes"] == 0
    if "spp_per_pass" in kw:
        assert st_on["n_passes"] > 1
    assert film_on[..., :3].any()
    _same(film_on, film_off, f"{name} {kw}")
    # ... and a part of the sample range, which the table serves by the same slots
    _same(on.render(k_begin=1, k_end=3, **kw)[0], off.render(k_begin=1, k_end=3, **kw)[0], f"{name} {kw}, samples [1, 3)")


def test_sobol_scene_has_no_table(binding, scenes, monkeypatch):
    on, off = _pair(binding, monkeypatch, scenes["sobol"])
    film_on, st_on = on.render()
    film_off, st_off = off.render()
    assert st_on["sample_table_bytes"] == 0 and st_off["sample_table_bytes"] == 0
    _same(film_on, film_off, "sobol")


def test_scene_over_the_budget_renders_by_the_chains(binding, scenes):
    """The budget is 4 GiB (kSampleTableBudget); the test probe iile_test_sample_table_budget puts it one byte under the 10.5 MiB
    table of the 64 x 48 room at 4 spp and maxdepth 5, then exactly at it."""
    assert binding.sample_table_budget() == 4 << 30
    scene = scenes["plain"]
    want_bytes = _table_bytes(4, 5)
    with_table = binding.GpuScene(scene)
    try:
        binding.set_test_sample_table_budget(want_bytes - 1)
        assert binding.sample_table_budget() == want_bytes - 1
        over = binding.GpuScene(scene)
        binding.set_test_sample_table_budget(want_bytes)   # ... and a budget that just holds it
        under = binding.GpuScene(scene)
    finally:
        binding.set_test_sample_table_budget(0)
    assert binding.sample_table_budget() == 4 << 30
    film, st = with_table.render()
    film_over, st_over = over.render()
    film_under, st_under = under.render()
    assert st["sample_table_bytes"] == want_bytes and st_under["sample_table_bytes"] == want_bytes
    assert st_over["sample_table_bytes"] == 0
    with pytest.raises(RuntimeError, match="no sample table"):
        over.sample_table_records([0], [0], [0], [0])
    _same(film_over, film, "over the budget")
    _same(film_under, film, "under the budget")


def test_probe_pass_is_untouched_by_the_table(binding, scenes, monkeypatch):
    pos = np.array([[0, 0, 0.5], [1, -2, 1], [-2, 1, 0]], np.float32)
    direction = np.array([[0, 0, 1], [0.3, 1, 0.2], [1, 0, 0]], np.float32)
    on, off = _pair(binding, monkeypatch, scenes["plain"])
    film_on, film_off = on.render()[0], off.render()[0]
    _same(film_on, film_off, "frame")
    for a, b, what in zip(on.render_probes(pos, direction)[:3], off.render_probes(pos, direction)[:3], ("intensity", "normals", "distance")):
        _same(a, b, "probes: " + what)
    _same(on.render()[0], film_on, "frame again after the probe pass")
