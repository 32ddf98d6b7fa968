"""A moving camera on the device (GPU): the rays of `iile_camera_rays_at` against the float64 restatement of camera_motion_ref.py;
a closed shutter against the static camera, bit for bit, through `iile_render` and `iile_render_ao`, over plain and over textured
materials (the camera ray's differentials); texture filtering at an interior time and under an open shutter; the blur of an edge in
closed form; the refusals; and `iile_pbrt` on the closed-form scene."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import camera_motion_cases as CC

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
EXE = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _load(binding, tmp_path, text, name):
    path = tmp_path / name
    path.write_text(text)
    host = binding.HostScene(path=str(path))
    return str(path), host, binding.GpuScene(host)


# ---- 1. the rays against the truth --------------------------------------------------------------------------------------------------
# The worst distance of the float32 restatement of the same operation sequence (camera_motion_ref with ft = float32: Decompose,
# Interpolate, GenerateRay, Transform(Ray)) from the float64 one over every case below — five motions, three cameras, two time
# sets, nine times, 64 film points: 6.71e-7 for an origin component, 6.96e-7 for a direction component (the scale change, whose
# directions are up to 2 long). The device's sincos / acos and the order of its sums differ: it gets four times that.
F32_WORST_ORIGIN, F32_WORST_DIRECTION = 6.71e-7, 6.96e-7
ORIGIN_BAR, DIRECTION_BAR = 4 * F32_WORST_ORIGIN, 4 * F32_WORST_DIRECTION


@pytest.mark.parametrize("camera", list(CC.CAMERAS))
@pytest.mark.parametrize("motion", list(CC.MOTIONS))
def test_rays_match_restatement(binding, tmp_path, motion, camera):
    """Bars: origin 2.68e-6, direction 2.78e-6 (4 x the float32 restatement's own distance from float64, measured on these cases).
    At and beyond the two ends of the motion the rays are those of the static scene at that transform, bit for bit."""
    pfilm, plens = CC.film_points(10 * list(CC.MOTIONS).index(motion) + list(CC.CAMERAS).index(camera))
    lens = plens if camera == "perspective_lens" else None
    _, _, gpu_start = _load(binding, tmp_path, CC.ray_scene_text(motion, camera, "times_0_1", moving=False), "start.pbrt")
    _, _, gpu_end = _load(binding, tmp_path, CC.ray_scene_text(motion, camera, "times_0_1", moving=False, at_end=True), "end.pbrt")
    static = {"start": gpu_start.camera_rays(pfilm, plens=lens), "end": gpu_end.camera_rays(pfilm, plens=lens)}
    # (a static camera reads no time)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(static["start"], gpu_start.camera_rays_at(pfilm, 0.5, plens=lens)))
    gpu_start.close(), gpu_end.close()
    assert not np.array_equal(_bits(static["start"][0]), _bits(static["end"][0])) or not np.array_equal(_bits(static["start"][1]), _bits(static["end"][1]))
    worst_o = worst_d = own_o = own_d = 0.0
    for time_set, ((t0, t1), times) in CC.TIME_SETS.items():
        _, host, gpu = _load(binding, tmp_path, CC.ray_scene_text(motion, camera, time_set), time_set + ".pbrt")
        want = CC.restated_rays(host, camera, time_set, pfilm, plens, np.float64)
        own = CC.restated_rays(host, camera, time_set, pfilm, plens, np.float32)
        assert len(times) == 9 and sum(t0 < t < t1 for t in times) == 5
        for t, (wo, wd), (fo, fd) in zip(times, want, own):
            o, d = gpu.camera_rays_at(pfilm, t, plens=lens)
            assert np.isfinite(o).all() and np.isfinite(d).all()
            worst_o, worst_d = max(worst_o, np.abs(o - wo).max()), max(worst_d, np.abs(d - wd).max())
            own_o, own_d = max(own_o, np.abs(fo - wo).max()), max(own_d, np.abs(fd - wd).max())
            if t <= t0 or t >= t1:
                so, sd = static["start" if t <= t0 else "end"]
                assert np.array_equal(_bits(o), _bits(so)) and np.array_equal(_bits(d), _bits(sd)), (time_set, t)
        if time_set == "times_0_1":  # iile_camera_rays keeps its meaning: the rays at time 0
            o0, d0 = gpu.camera_rays(pfilm, plens=lens)
            assert np.array_equal(_bits(o0), _bits(static["start"][0])) and np.array_equal(_bits(d0), _bits(static["start"][1]))
        gpu.close()
    print(f"{motion} / {camera}: device origin {worst_o:.3e} (bar {ORIGIN_BAR:.3e}), direction {worst_d:.3e} (bar {DIRECTION_BAR:.3e}); "
          f"float32 restatement origin {own_o:.3e}, direction {own_d:.3e}")
    assert own_o <= F32_WORST_ORIGIN * 1.001 and own_d <= F32_WORST_DIRECTION * 1.001   # the measured values stand
    assert worst_o <= ORIGIN_BAR and worst_d <= DIRECTION_BAR


# ---- 2. a closed shutter is a static camera, bit for bit ----------------------------------------------------------------------------
# a lit box of quads seen from inside: an emitting quad overhead, matte walls (16 x 16, 4 spp, maxdepth 3)
def _quad(p):
    return f'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [{" ".join(str(v) for v in p)}]\n'


BOX = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [4 4 4]\n' + _quad([-1, 2.9, -1, 1, 2.9, -1, 1, 2.9, 1, -1, 2.9, 1]) + 'AttributeEnd\n'
       'Material "matte" "rgb Kd" [0.6 0.5 0.4]\n' +
       _quad([-4, -1, -4, 4, -1, -4, 4, -1, 4, -4, -1, 4]) + _quad([-4, 3, -4, 4, 3, -4, 4, 3, 4, -4, 3, 4]) +
       _quad([-4, -1, -4, -4, 3, -4, -4, 3, 4, -4, -1, 4]) + _quad([4, -1, -4, 4, 3, -4, 4, 3, 4, 4, -1, 4]) +
       _quad([-4, -1, -4, 4, -1, -4, 4, 3, -4, -4, 3, -4]) + _quad([-4, -1, 4, 4, -1, 4, 4, 3, 4, -4, 3, 4]))
# the same without its lid and two of its walls, for the ambient occlusion integrator: inside the closed box every occlusion ray hits
OPEN_BOX = ('Material "matte"\n' + _quad([-4, -1, -4, 4, -1, -4, 4, -1, 4, -4, -1, 4]) + _quad([-4, -1, 4, 4, -1, 4, 4, 3, 4, -4, 3, 4]) +
            _quad([-4, -1, -4, -4, 3, -4, -4, 3, 4, -4, -1, 4]) + 'Translate 0.5 0 1\nShape "sphere" "float radius" [0.8]\n')
BOX_BASE = "LookAt 0.5 0.2 -3  0 1 0  0 1 0"
BOX_MOTION = "Translate 0.7 0.1 -0.4\nRotate 25 0.2 1 0.1"
BOX_CAMERAS = {
    "perspective_lens": 'Camera "perspective" "float fov" [60] "float lensradius" [0.05] "float focaldistance" [3] %s',
    "environment": 'Camera "environment" %s',
}


def _box_pair(binding, tmp_path, camera, sampler, shutter, integrator='Integrator "path" "integer maxdepth" [3]', world=BOX):
    """(moving scene, the static scene at the transform the closed shutter stands at), both with the same Camera line."""
    cam = BOX_CAMERAS[camera] % f'"float shutteropen" [{shutter}] "float shutterclose" [{shutter}]'
    smp = f'Sampler "{sampler}" "integer pixelsamples" [4]'
    kw = dict(camera=cam, sampler=smp, world=world, integrator=integrator)
    moving = _load(binding, tmp_path, CC.scene_text(CC.camera_block(BOX_MOTION, BOX_BASE), **kw), "moving.pbrt")
    static = _load(binding, tmp_path, CC.scene_text(BOX_BASE + ("\n" + BOX_MOTION if shutter == 1 else ""), **kw), "static.pbrt")
    assert moving[1].camera_motion is not None and static[1].camera_motion is None
    return moving, static


@pytest.mark.parametrize("table", ["table", "no_table"])
@pytest.mark.parametrize("sampler", ["halton", "sobol"])
@pytest.mark.parametrize("camera", list(BOX_CAMERAS))
def test_closed_shutter_is_a_static_camera(binding, tmp_path, camera, sampler, table):
    for shutter in (0, 1):
        binding.set_test_sample_table_budget(1 if table == "no_table" else 0)
        try:
            (_, _, moving), (_, _, static) = _box_pair(binding, tmp_path, camera, sampler, shutter)
        finally:
            binding.set_test_sample_table_budget(0)
        film_m, st_m = moving.render()
        film_s, st_s = static.render()
        counted_m, _ = moving.render(collect_stats=True)
        moving.close(), static.close()
        has_table = table == "table" and sampler == "halton"
        assert (st_m["sample_table_bytes"] > 0) == has_table and (st_s["sample_table_bytes"] > 0) == has_table
        if has_table:  # the time column: one float per slot
            assert st_m["sample_table_bytes"] - st_s["sample_table_bytes"] == 4 * 128 * 128 * 4
        assert film_s[..., :3].max() > 0 and len(np.unique(film_s.reshape(-1, 4), axis=0)) > 100
        assert np.array_equal(_bits(film_m), _bits(film_s)), (camera, sampler, table, shutter)
        assert np.array_equal(_bits(counted_m), _bits(film_s))


@pytest.mark.parametrize("sampler", ["halton", "sobol"])
@pytest.mark.parametrize("camera", list(BOX_CAMERAS))
def test_closed_shutter_is_a_static_camera_ao(binding, tmp_path, camera, sampler):
    for shutter in (0, 1):
        (_, _, moving), (_, _, static) = _box_pair(binding, tmp_path, camera, sampler, shutter,
                                                  integrator='Integrator "ambientocclusion" "integer nsamples" [8]', world=OPEN_BOX)
        film_m, _ = moving.render_ao()
        film_s, _ = static.render_ao()
        moving.close(), static.close()
        assert film_s[..., :3].max() > 0 and len(np.unique(film_s.reshape(-1, 4), axis=0)) > 20   # (not a blank image; the sky is)
        assert np.array_equal(_bits(film_m), _bits(film_s)), (camera, sampler, shutter)


def test_an_open_shutter_moves_the_image(binding, tmp_path):
    """The closed-shutter equalities above are not those of a motion nobody reads."""
    cam = BOX_CAMERAS["perspective_lens"] % ""
    kw = dict(camera=cam, world=BOX)
    _, _, moving = _load(binding, tmp_path, CC.scene_text(CC.camera_block(BOX_MOTION, BOX_BASE), **kw), "moving.pbrt")
    _, _, static = _load(binding, tmp_path, CC.scene_text(BOX_BASE, **kw), "static.pbrt")
    film_m, film_s = moving.render()[0], static.render()[0]
    moving.close(), static.close()
    assert not np.array_equal(_bits(film_m), _bits(film_s))


# ---- 2b. textured materials: the camera ray's differentials (k_shade rebuilds them from the camera sample, time included) -------------
def _write_pfm(path, rows):
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


def _quad_uv(p):
    return _quad(p)[:-1] + ' "float uv" [0 0 1 0 1 1 0 1]\n'


def _tex_box(tmp_path, disney):
    """The box with a checkerboard floor (closed-form antialiasing), an image on the far wall (EWA), a bump-mapped left wall and,
    `disney`, a Disney right wall with an image for its colour: every one of them filtered by the camera ray's differentials."""
    rng = np.random.default_rng(7)
    _write_pfm(tmp_path / "img.pfm", rng.uniform(0.05, 0.95, (32, 32, 3)).astype(np.float32))
    _write_pfm(tmp_path / "bmp.pfm", np.repeat(rng.uniform(0, 0.3, (16, 16, 1)).astype(np.float32), 3, axis=2))
    right = 'Material "disney" "texture color" "img" "float roughness" [0.4] "float sheen" [0.5]\n' if disney else 'Material "matte" "rgb Kd" [0.4 0.5 0.6]\n'
    return ('Texture "chk" "spectrum" "checkerboard" "float uscale" [6] "float vscale" [6]\n'
            'Texture "img" "spectrum" "imagemap" "string filename" ["img.pfm"]\n'
            'Texture "bmp" "float" "imagemap" "string filename" ["bmp.pfm"]\n'
            'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [4 4 4]\n' + _quad([-1, 2.9, -1, 1, 2.9, -1, 1, 2.9, 1, -1, 2.9, 1]) + 'AttributeEnd\n'
            'Material "matte" "texture Kd" "chk"\n' + _quad_uv([-4, -1, -4, 4, -1, -4, 4, -1, 4, -4, -1, 4]) +
            'Material "matte" "texture Kd" "img"\n' + _quad_uv([-4, -1, 4, 4, -1, 4, 4, 3, 4, -4, 3, 4]) +
            'Material "matte" "rgb Kd" [0.6 0.5 0.4] "texture bumpmap" "bmp"\n' + _quad_uv([-4, -1, -4, -4, 3, -4, -4, 3, 4, -4, -1, 4]) +
            right + _quad_uv([4, -1, -4, 4, 3, -4, 4, 3, 4, 4, -1, 4]) +
            'Material "matte" "rgb Kd" [0.6 0.5 0.4]\n' + _quad([-4, 3, -4, 4, 3, -4, 4, 3, 4, -4, 3, 4]) + _quad([-4, -1, -4, 4, -1, -4, 4, 3, -4, -4, 3, -4]))


@pytest.mark.parametrize("world", ["textured", "textured_disney"])
@pytest.mark.parametrize("sampling", ["halton_table", "halton_no_table", "sobol"])
@pytest.mark.parametrize("camera", list(BOX_CAMERAS))
def test_closed_shutter_is_a_static_camera_textured(binding, tmp_path, camera, sampling, world):
    """The camera differentials of a moving camera, at the two ends of its motion: the film of a scene whose materials read
    textures (image, checkerboard, bump map) equals the static scene's bit for bit, through the builds with and without the sample
    table, Sobol', and the instrumented build. Without a Disney material the static scene runs the textured build and the moving one
    the Disney build, which shades every material."""
    sampler = "sobol" if sampling == "sobol" else "halton"
    tex = _tex_box(tmp_path, world == "textured_disney")
    for shutter in (0, 1):
        binding.set_test_sample_table_budget(1 if sampling == "halton_no_table" else 0)
        try:
            (_, _, moving), (_, host_s, static) = _box_pair(binding, tmp_path, camera, sampler, shutter, world=tex)
        finally:
            binding.set_test_sample_table_budget(0)
        film_m, st_m = moving.render()
        film_s, st_s = static.render()
        counted_m, _ = moving.render(collect_stats=True)
        moving.close(), static.close()
        assert (st_m["sample_table_bytes"] > 0) == (sampling == "halton_table") == (st_s["sample_table_bytes"] > 0)
        assert host_s.scene_desc().n_textures >= 3 and film_s[..., :3].max() > 0
        assert np.array_equal(_bits(film_m), _bits(film_s)), (camera, sampling, world, shutter)
        assert np.array_equal(_bits(counted_m), _bits(film_s)), (camera, sampling, world, shutter)


@pytest.mark.parametrize("camera", list(BOX_CAMERAS))
def test_time_column_over_the_budget_gives_the_table_up(binding, tmp_path, camera):
    """A table that fits its budget alone and not with the time column: the static scene keeps it, the moving one drops it
    (iile_scene_set_camera_motion) and renders the same film by the digit chains."""
    slots = 128 * 128 * 4
    (_, _, probe), (_, _, other) = _box_pair(binding, tmp_path, camera, "halton", 0)
    table = probe.render()[1]["sample_table_bytes"] - 4 * slots
    probe.close(), other.close()
    assert table > 0
    binding.set_test_sample_table_budget(table + 2 * slots)   # between the table and the table with 4 bytes a slot more
    try:
        (_, _, moving), (_, _, static) = _box_pair(binding, tmp_path, camera, "halton", 0)
    finally:
        binding.set_test_sample_table_budget(0)
    film_m, st_m = moving.render()
    film_s, st_s = static.render()
    moving.close(), static.close()
    assert st_s["sample_table_bytes"] == table and st_m["sample_table_bytes"] == 0
    assert np.array_equal(_bits(film_m), _bits(film_s))


# A camera at the origin that looks down +z and only translates: Decompose leaves R = S = identity and the quaternion (0, 0, 0, 1)
# exactly, so the transform composed at an interior time is Translate(lerp T) to the bit, sums of products with exact 0 and 1; and
# lerp T = (1 - 0.5) * 0 + 0.5 * -4 = -2 exactly.
NOISE_WALL = ('LightSource "distant" "point from" [0 0 0] "point to" [0 0 1] "rgb L" [3 3 3]\n'
              'Texture "img" "spectrum" "imagemap" "string filename" ["img.pfm"] %s\nMaterial "matte" "texture Kd" "img"\n'
              'Shape "trianglemesh" "integer indices" [0 2 1 0 3 2] "point P" [%s] "float uv" [0 0 1 0 1 1 0 1]\n')


def _wall_scene(before, shutter, wall, options=""):
    cam = f'Camera "perspective" "float fov" [60] "float shutteropen" [{shutter[0]}] "float shutterclose" [{shutter[1]}]'
    return CC.scene_text(before, camera=cam, integrator='Integrator "path" "integer maxdepth" [1]', world=NOISE_WALL % (options, wall))


def test_interior_time_filters_as_the_static_camera_there(binding, tmp_path):
    """A camera that backs away from a wall of fine noise, z = 0 to z = -4, the shutter standing at time 0.5: through the composed
    transform, ray and differentials alike, the film is that of the static camera at z = -2, bit for bit; and the texture is
    filtered more the later the time (the wall fills every frame: the spread of its pixels falls from time 0 over 0.5 to 1)."""
    _write_pfm(tmp_path / "img.pfm", np.random.default_rng(3).uniform(0, 1, (64, 64, 3)).astype(np.float32))
    wall = "-8 -8 3  8 -8 3  8 8 3  -8 8 3"
    films = {}
    for t in (0, 0.5, 1):
        _, host, gpu = _load(binding, tmp_path, _wall_scene(CC.camera_block("Translate 0 0 4", "Identity"), (t, t), wall), "moving.pbrt")
        assert host.camera_motion is not None
        films[t] = gpu.render()[0]
        gpu.close()
    _, host, gpu = _load(binding, tmp_path, _wall_scene("Translate 0 0 2", (0.5, 0.5), wall), "static.pbrt")
    assert host.camera_motion is None
    static = gpu.render()[0]
    gpu.close()
    assert np.array_equal(_bits(films[0.5]), _bits(static))
    spread = {t: float((f[..., 1] / f[..., 3]).std()) for t, f in films.items()}
    print("spread of the wall's pixels at time 0, 0.5, 1:", spread)
    assert spread[0] > spread[0.5] > spread[1] > 0


def test_open_shutter_along_the_stripes_changes_nothing(binding, tmp_path):
    """An open shutter, every sample at a time of its own: the camera slides 3 along x past a wall whose image has one column
    (stripes along x, trilinear filtering: the filter width is the longer differential) under a distant light. Nothing a sample
    computes depends on the camera's x but the hit point's x, so the film is the static camera's up to rounding: differentials
    taken at another time than the ray's would put the auxiliary rays up to 3 to the side, a footprint of the whole image.
    Bar 1e-4 of a film of about 1: the rays' directions and y, z are the same bits; the hit's y carries the rounding of a
    barycentric sum of coordinates up to 16 (a few 16 * 2^-24 = 1e-6 each, say 1e-5), 1e-5 / 24 of v, 3e-5 of a texel of the 64,
    so 3e-5 of the texel range 1 in Kd, the same again for the filter width, times L / pi = 0.95."""
    rng = np.random.default_rng(5)
    _write_pfm(tmp_path / "img.pfm", np.repeat(rng.uniform(0, 1, (64, 1, 1)).astype(np.float32), 3, axis=2))
    wall = "-16 -12 3  16 -12 3  16 12 3  -16 12 3"
    opts = '"bool trilinear" "true"'
    _, host, gpu = _load(binding, tmp_path, _wall_scene(CC.camera_block("Translate -3 0 0", "Identity"), (0, 1), wall, opts), "moving.pbrt")
    assert host.camera_motion is not None
    film_m = gpu.render()[0]
    gpu.close()
    _, _, gpu = _load(binding, tmp_path, _wall_scene("Identity", (0, 1), wall, opts), "static.pbrt")
    film_s = gpu.render()[0]
    gpu.close()
    err = float(np.abs(film_m[..., :3] / film_m[..., 3:] - film_s[..., :3] / film_s[..., 3:]).max())
    rows = (film_s[..., 1] / film_s[..., 3]).mean(axis=1)
    print(f"open shutter along the stripes: worst difference {err:.3e} (bar 1e-4), spread of the rows {rows.std():.3e}")
    assert rows.std() > 0.02   # the stripes are seen
    assert err <= 1e-4


# ---- 3. the blur in closed form -----------------------------------------------------------------------------------------------------
LE, D, SPP = 2.0, 5.0, 125
# a one-sided emitter in the plane z = 1 over x <= 0, facing the camera (-z), wide in y
EDGE = (f'AreaLightSource "diffuse" "rgb L" [{LE} {LE} {LE}]\n'
        'Shape "trianglemesh" "integer indices" [0 2 1 0 3 2] "point P" [-400 -400 1  0 -400 1  0 400 1  -400 400 1]\n')


def _edge_scene():
    """The camera at the origin looks down +z and moves by D along +x over [0, 1] (its CTM, world to camera, by -D); shutter 0 .. 1."""
    return CC.scene_text(CC.camera_block(f"Translate {-D} 0 0", "Identity"), camera='Camera "perspective" "float fov" [60]', xres=32, yres=4,
                         sampler=f'Sampler "halton" "integer pixelsamples" [{SPP}] "bool samplepixelcenter" "true"',
                         integrator='Integrator "path" "integer maxdepth" [1]', filt='PixelFilter "box" "float xwidth" [0.5] "float ywidth" [0.5]',
                         world=EDGE)


def _edge_expectation(host):
    """Le * clamp(-s / D, 0, 1) per pixel, s = d.x / d.z of the pixel centre's camera-space ray (RasterToCamera in float64)."""
    r2c = np.array(host.camera()[1].raster_to_camera, np.float64).reshape(4, 4)
    px, py = np.meshgrid(np.arange(32) + 0.5, np.arange(4) + 0.5)
    p = np.stack([px, py, np.zeros_like(px), np.ones_like(px)], -1) @ r2c.T
    s = p[..., 0] / p[..., 2]
    frac = -s / D
    return LE * np.clip(frac, 0, 1), (frac > 0) & (frac < 1)


# A pixel's 125 consecutive samples put exactly one time sample in each 1/125 bin of dimension 2 (base 5; the sample stride is
# coprime to 5), so the count of samples that see the emitter is within one of 125 * fraction: Le / 125. Float32: the film's
# weighted sum of 125 values (125 * 2^-24 = 7.5e-6 relative) and, for an RGB image, the XYZ -> RGB matrix, which is not the inverse
# of RGBToXYZ to 4e-6: together 1.2e-5 * Le at the most.
EDGE_BAR = LE / SPP + 1.2e-5 * LE


def _check_ramp(rgb, host):
    want, inside = _edge_expectation(host)
    assert inside.sum() >= 40 and inside.any(axis=0).sum() >= 10   # at least ten pixel columns strictly inside the ramp
    err = np.abs(rgb - want[..., None]).max()
    print(f"closed-form blur: worst error {err:.4e}, bar {EDGE_BAR:.4e} (Le / {SPP} = {LE / SPP:.4e})")
    ramp = rgb[inside]
    assert (ramp > 0).all() and (ramp < LE).all()
    assert (want[~inside] == 0).all() and np.abs(rgb[~inside]).max() <= EDGE_BAR   # right of the edge: nothing, at any time
    assert err <= EDGE_BAR


def test_blur_of_an_edge_in_closed_form(binding, tmp_path):
    _, host, gpu = _load(binding, tmp_path, _edge_scene(), "edge.pbrt")
    assert host.scene_desc().halton.sample_stride % 5 != 0
    film, _ = gpu.render()
    gpu.close()
    assert (film[..., 3] == SPP).all()   # the box filter of one pixel: every sample of a pixel lands in it, with weight 1
    _check_ramp(host.film_to_rgb(film).astype(np.float64), host)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_iispt_entry_points_refuse_a_moving_camera(binding, tmp_path):
    _, host, gpu = _load(binding, tmp_path, CC.scene_text(CC.camera_block(BOX_MOTION, BOX_BASE), world=BOX, spp=1), "moving.pbrt")
    task = binding.IisptTask(0, 0, 16, 16, 8, 0, 1)
    nx, ny = task.grid()
    valid, pos, dr = np.ones((ny, nx), np.uint8), np.zeros((ny, nx, 3), np.float32), np.zeros((ny, nx, 3), np.float32)
    dr[..., 1] = 1
    nn = np.zeros((ny, nx, 32, 32, 3), np.float32)
    one = np.zeros((1, 3), np.float32)
    up = np.array([[0, 1, 0]], np.float32)
    calls = {
        "iile_render_direct": lambda: gpu.render_direct(1),
        "iile_iispt_hemi_points": lambda: gpu.iispt_hemi_points(task),
        "iile_iispt_hemi_points_batch": lambda: gpu.iispt_hemi_points_batch([task]),
        "iile_iispt_gather": lambda: gpu.iispt_gather(task, valid, pos, dr, nn_films=nn),
        "iile_iispt_gather_batch": lambda: gpu.iispt_gather_batch([task], valid.reshape(-1), pos.reshape(-1, 3), dr.reshape(-1, 3),
                                                                   nn_films=nn.reshape(-1, 32, 32, 3)),
        "iile_iispt_film_add": lambda: gpu.iispt_film_add([task], 256, 256),   # (never dereferenced: the refusal comes first)
        "iile_reference_points": lambda: gpu.reference_points(np.array([[8.5, 8.5]], np.float32)),
        "iile_render_probes": lambda: gpu.render_probes(one, up),
        "iile_render_probes_reference": lambda: gpu.render_probes_reference(one, up, 2),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError) as e:
            call()
        msg = str(e.value)
        assert f"({binding.ERR_UNSUPPORTED})" in msg and "moving camera" in msg, (name, msg)
    film, _ = gpu.render()   # the scene itself is fine
    gpu.close()
    assert film[..., :3].max() > 0


def test_set_camera_motion_rejects_bad_arguments(binding, tmp_path):
    _, host, _gpu = _load(binding, tmp_path, CC.scene_text(CC.camera_block(BOX_MOTION, BOX_BASE), world=BOX), "moving.pbrt")
    _gpu.close()
    good = host.camera_motion
    path = tmp_path / "static.pbrt"
    path.write_text(CC.scene_text(BOX_BASE, world=BOX))
    static_host = binding.HostScene(path=str(path))
    lib = binding.gpu_lib()

    def attempt(motion):
        gpu = binding.GpuScene(static_host)   # (a static scene: GpuScene sets no motion itself)
        rc = gpu.set_camera_motion(motion)
        msg = lib.iile_last_error().decode()
        film = gpu.render()[0] if rc else None   # a refused motion leaves the scene what it was
        gpu.close()
        return rc, msg, film

    def altered(change):
        m = binding.CameraMotion.from_buffer_copy(bytes(good))
        change(m)
        return m

    gpu = binding.GpuScene(static_host)
    plain = gpu.render()[0]
    gpu.close()
    cases = {
        "null": (None, "null argument"),
        "nan_time": (altered(lambda m: setattr(m, "start_time", float("nan"))), "non-finite"),
        "inf_matrix": (altered(lambda m: m.camera_to_world_end.__setitem__(3, float("inf"))), "non-finite"),
        "nan_quaternion": (altered(lambda m: m.R[1].__setitem__(2, float("nan"))), "non-finite"),
        "inf_scale": (altered(lambda m: m.S[0].__setitem__(5, float("-inf"))), "non-finite"),
        "nan_translation": (altered(lambda m: m.T[1].__setitem__(0, float("nan"))), "non-finite"),
        "end_before_start": (altered(lambda m: (setattr(m, "start_time", 1.0), setattr(m, "end_time", 0.5))), "ends before it starts"),
    }
    for name, (motion, word) in cases.items():
        rc, msg, film = attempt(motion)
        assert rc == binding.ERR_ARG and word in msg, (name, rc, msg)
        assert np.array_equal(_bits(film), _bits(plain)), name
    # a good motion is taken once
    gpu = binding.GpuScene(static_host)
    assert gpu.set_camera_motion(good) == 0
    assert gpu.set_camera_motion(good) == binding.ERR_ARG and "already" in lib.iile_last_error().decode()
    moved = gpu.render()[0]
    gpu.close()
    assert not np.array_equal(_bits(moved), _bits(plain))


class _Broken:
    """A host scene whose environment-camera descriptor fails the camera checks of iile_scene_create, and its motion."""

    def __init__(self, binding, host, motion):
        self._desc = binding.SceneDesc.from_buffer_copy(ctypes.string_at(host.desc, ctypes.sizeof(binding.SceneDesc)))
        self._desc.camera.lens_radius = 0.25   # an environment camera has no lens: "a zero raster_to_camera needs lens_radius 0 ..."
        self.desc = ctypes.cast(ctypes.pointer(self._desc), ctypes.c_void_p)
        self.camera_motion = motion
        self.keep = host


def test_motion_does_not_get_past_the_camera_checks(binding, tmp_path):
    """A motion travels beside the descriptor: an environment-camera descriptor that fails iile_scene_create's camera checks is
    refused there, before any motion could be attached to it."""
    path = tmp_path / "env.pbrt"
    path.write_text(CC.scene_text(CC.camera_block(BOX_MOTION, BOX_BASE), camera='Camera "environment"', world=BOX))
    host = binding.HostScene(path=str(path))
    assert host.camera()[0] == binding.CAMERA_ENVIRONMENT and host.camera_motion is not None
    with pytest.raises(RuntimeError, match="iile_scene_create failed.*environment camera"):
        binding.GpuScene(_Broken(binding, host, host.camera_motion))
    binding.GpuScene(host).close()   # the descriptor as the host made it, and its motion, are fine


# ---- 5. the command line ------------------------------------------------------------------------------------------------------------
def _run(*args, ok=True):
    p = subprocess.run([EXE, *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stdout
    return p.stdout


def test_cli_renders_the_closed_form_scene(binding, tmp_path):
    path, host, gpu = _load(binding, tmp_path, _edge_scene(), "edge.pbrt")
    gpu.close()
    out = tmp_path / "edge.pfm"
    _run(path, "--outfile", out)
    raw = out.read_bytes()
    head = b"PF\n32 4\n-1.0\n"
    assert raw.startswith(head)
    rgb = np.frombuffer(raw[len(head):], "<f4").reshape(4, 32, 3)[::-1]
    _check_ramp(rgb.astype(np.float64), host)
    allp = tmp_path / "all.pfm"
    _run(path, "--outfile", allp, "--gpus", "1")   # every device of --gpus N gets the motion
    assert allp.read_bytes() == raw


def test_cli_refuses_the_iispt_modes(binding, tmp_path):
    path = tmp_path / "edge.pbrt"
    path.write_text(_edge_scene())
    for args in (["--integrator", "iispt"], ["--reference=2"]):
        text = _run(path, "--outfile", tmp_path / "x.pfm", *args, ok=False)
        assert "moving camera" in text, text
