"""`Camera "environment"` through the loader and the refusal pass of iile_scene_create, without a GPU: the encoding of the camera
in iile_camera (include/iile_scene.h), the parameters CreateEnvironmentCamera reads and drops (src/cameras/environment.cpp:58-101),
the cameras that stay refused, and the perspective camera's descriptor left as it was."""
import ctypes

import numpy as np
import pytest

import envcamera_ref as EC

c_i32, c_u32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
ERR_ARG = 1
REFUSAL = "environment camera: a zero raster_to_camera needs lens_radius 0 and the angle steps 2 pi / xres, pi / yres"
PI = np.float32(3.14159265358979323846)


def scene_text(camera='Camera "environment"', before="", xres=32, yres=16, spp=4, integrator='Integrator "path" "integer maxdepth" [3]',
               sampler=None, world=None):
    world = world if world is not None else ('LightSource "point" "rgb I" [1 1 1] "point from" [0 0 3]\nMaterial "matte"\n'
                                             'Shape "sphere" "float radius" [5]\n')
    sampler = sampler or f'Sampler "halton" "integer pixelsamples" [{spp}]'
    return (f'{before}\n{camera}\nFilm "image" "integer xresolution" [{xres}] "integer yresolution" [{yres}] "string filename" "env.exr"\n'
            f'PixelFilter "box"\n{sampler}\n{integrator}\nWorldBegin\n{world}WorldEnd\n')


def load(binding, tmp_path, name="env.pbrt", **kw):
    path = tmp_path / name
    path.write_text(scene_text(**kw))
    return binding.HostScene(path=str(path))


def _f32s(a):
    return np.array(list(a), np.float32)


def test_environment_camera_loads_without_a_lens(binding, tmp_path):
    """The kind, the zero matrix, the two angle steps as the host rounds them in float, and no lens whatever the file says
    ("lensradius", "focaldistance", "frameaspectratio" and "screenwindow" are read and dropped, environment.cpp:69-98)."""
    for extra in ("", ' "float lensradius" [0.2] "float focaldistance" [3] "float frameaspectratio" [1.5] "float screenwindow" [-2 2 -1 1]'):
        host = load(binding, tmp_path, camera='Camera "environment"' + extra, xres=48, yres=20)
        kind, cam = host.camera()
        assert kind == binding.CAMERA_ENVIRONMENT
        assert not _f32s(cam.raster_to_camera).any()
        assert cam.lens_radius == 0 and cam.focal_distance == 0
        assert _f32s(cam.dx_camera).tolist() == [np.float32(2) * PI / np.float32(48), 0, 0]
        assert _f32s(cam.dy_camera).tolist() == [0, PI / np.float32(20), 0]
        assert (cam.shutter_open, cam.shutter_close) == (0, 1)
        assert host.info["xres"] == 48 and host.info["yres"] == 20


def test_angle_steps_follow_the_resolution_override(binding, tmp_path):
    path = tmp_path / "o.pbrt"
    path.write_text(scene_text())
    _, cam = binding.HostScene(path=str(path), xres=10, yres=6).camera()
    assert cam.dx_camera[0] == np.float32(2) * PI / np.float32(10) and cam.dy_camera[1] == PI / np.float32(6)


def test_camera_to_world_is_the_inverse_ctm(binding, tmp_path):
    before = "LookAt 1 2 3  0 0.5 0  0 0 1\nScale -1 1 1"
    _, cam = load(binding, tmp_path, before=before).camera()
    want = EC.camera_to_world(np.linalg.inv(EC.look_at([1, 2, 3], [0, 0.5, 0], [0, 0, 1])), EC.scale(-1, 1, 1))
    assert np.allclose(_f32s(cam.camera_to_world).reshape(4, 4), want, rtol=0, atol=1e-5)


def test_reversed_shutter_is_swapped(binding, tmp_path):
    _, cam = load(binding, tmp_path, camera='Camera "environment" "float shutteropen" [0.75] "float shutterclose" [0.25]').camera()
    assert (cam.shutter_open, cam.shutter_close) == (0.25, 0.75)


def test_named_coordinate_system_camera(binding, tmp_path):
    """named_cs_["camera"] as for the perspective camera: a light placed in camera space sits at the camera's position."""
    world = ('AttributeBegin\nCoordSysTransform "camera"\nLightSource "point" "rgb I" [1 1 1]\nAttributeEnd\nMaterial "matte"\n'
             'Shape "sphere" "float radius" [5]\n')
    host = load(binding, tmp_path, before="LookAt 1 2 3  0 0 0  0 0 1", world=world)
    assert np.allclose(list(host.light(0).pos), [1, 2, 3], atol=1e-5)


@pytest.mark.parametrize("name", ["realistic", "orthographic"])
def test_other_cameras_stay_refused_by_name(binding, tmp_path, name):
    with pytest.raises(RuntimeError, match=f"perspective and environment cameras are supported, got {name}"):
        load(binding, tmp_path, camera=f'Camera "{name}"')


def test_iispt_and_sobol_scenes_load(binding, tmp_path):
    host = load(binding, tmp_path, integrator='Integrator "iispt"', spp=1)
    assert host.info["integrator"] == 1 and host.camera()[0] == binding.CAMERA_ENVIRONMENT
    host = load(binding, tmp_path, sampler='Sampler "sobol" "integer pixelsamples" [4]')
    assert host.camera()[0] == binding.CAMERA_ENVIRONMENT


# ---- the perspective camera's descriptor is what it was -----------------------------------------------------------------------------
# scenes/killeroo-simple.pbrt (700 x 700) as the commit before the environment camera wrote it, as the floats' bit patterns
KILLEROO_RASTER_TO_CAMERA = [981769544, 0, 0, 3199553288, 0, 3129253192, 0, 1052069640, 0, 0, 0, 1065353216, 0, 0, 3267886973, 1120403456]
KILLEROO_DX_CAMERA = [925482752, 0, 0]
KILLEROO_DY_CAMERA = [0, 3072966400, 0]
KILLEROO_CAMERA_TO_WORLD = [3164757924, 3198696973, 3211901732, 1137073677, 3212833569, 1003845368, 1016683120, 1113269518, 0, 1064421197,
                            3198699139, 1106247680, 0, 0, 0, 1065353216]


def test_perspective_descriptor_of_the_stock_scene_is_unchanged(binding):
    kind, cam = binding.HostScene().camera()
    assert kind == binding.CAMERA_PERSPECTIVE
    bits = lambda a: _f32s(a).view(np.uint32).tolist()
    assert bits(cam.raster_to_camera) == KILLEROO_RASTER_TO_CAMERA
    assert bits(cam.dx_camera) == KILLEROO_DX_CAMERA and bits(cam.dy_camera) == KILLEROO_DY_CAMERA
    assert bits(cam.camera_to_world) == KILLEROO_CAMERA_TO_WORLD
    assert cam.lens_radius == 0 and cam.focal_distance == 1e6 and (cam.shutter_open, cam.shutter_close) == (0, 1)


# ---- the refusal pass: a test-only view of the whole iile_scene_desc, as test_scene_refusals.py builds its own --------------------
class Camera(ctypes.Structure):
    _fields_ = [("raster_to_camera", c_f32 * 16), ("camera_to_world", c_f32 * 16), ("lens_radius", c_f32), ("focal_distance", c_f32),
                ("shutter_open", c_f32), ("shutter_close", c_f32), ("dx_camera", c_f32 * 3), ("dy_camera", c_f32 * 3)]


class Film(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in "xres yres crop_x0 crop_y0 crop_x1 crop_y1 samp_x0 samp_y0 samp_x1 samp_y1".split()
                ] + [(n, c_f32) for n in "filter_rx filter_ry scale max_sample_luminance".split()]


class Halton(ctypes.Structure):
    _fields_ = [("spp", c_i32), ("base_scales", c_i32 * 2), ("base_exponents", c_i32 * 2), ("sample_stride", c_i32),
                ("mult_inverse", c_i32 * 2), ("n_dims", c_i32), ("perms", c_vp), ("primes", c_vp), ("prime_sums", c_vp),
                ("n_perms", c_i32), ("sample_at_pixel_center", c_i32)]


class Integrator(ctypes.Structure):
    _fields_ = [("max_depth", c_i32), ("rr_threshold", c_f32), ("light_strategy", c_i32), ("light_power", c_f32 * 8),
                ("pixel_bounds", c_i32 * 4)]


class ProbeSetup(ctypes.Structure):
    _fields_ = [("hemi_size", c_i32), ("max_depth", c_i32), ("film", Film), ("filter_table", c_f32 * 256), ("base_scales", c_i32 * 2),
                ("base_exponents", c_i32 * 2), ("sample_stride", c_i32), ("mult_inverse", c_i32 * 2)]


class Sobol(ctypes.Structure):
    _fields_ = [("enabled", c_i32), ("spp", c_i32), ("resolution", c_i32), ("log2_resolution", c_i32), ("n_dims", c_i32),
                ("matrices32", c_vp), ("vdc", c_u32 * 32), ("vdc_inv", c_u32 * 32)]


class SceneDesc(ctypes.Structure):
    _fields_ = [("n_nodes", c_i32), ("nodes", c_vp), ("n_prims", c_i32), ("prim_flags", c_vp), ("prim_material", c_vp),
                ("prim_light", c_vp), ("prim_shape", c_vp), ("tri_p", c_vp), ("tri_n", c_vp), ("tri_uv", c_vp), ("prim_alpha", c_vp),
                ("n_spheres", c_i32), ("spheres", c_vp), ("n_materials", c_i32), ("materials", c_vp), ("n_lights", c_i32),
                ("lights", c_vp), ("n_env_dist", c_i64), ("env_dist", c_vp), ("n_textures", c_i32), ("textures", c_vp),
                ("n_texels", c_i64), ("texels", c_vp), ("ewa_lut", c_f32 * 128), ("film_filter_wide", c_i32),
                ("film_filter_table", c_f32 * 256), ("camera", Camera), ("film", Film), ("halton", Halton),
                ("integrator", Integrator), ("probe", ProbeSetup), ("sobol", Sobol), ("n_quadrics", c_i32), ("quadrics", c_vp)]


class Desc:
    """A copy of a loaded scene's descriptor (the loaded scene itself stays as it was)."""

    def __init__(self, binding, host):
        self.binding, self.host = binding, host
        self.d = SceneDesc.from_buffer_copy(ctypes.string_at(host.desc, ctypes.sizeof(SceneDesc)))

    def create(self):
        lib = self.binding.gpu_lib()
        out = c_vp()
        rc = lib.iile_scene_create(ctypes.addressof(self.d), ctypes.byref(out))
        if rc == 0:
            lib.iile_scene_destroy(out)
        return rc, lib.iile_last_error().decode()


def test_camera_struct_keeps_its_layout(binding):
    assert ctypes.sizeof(Camera) == 168 == ctypes.sizeof(binding.Camera)
    assert [(n, t._length_ if hasattr(t, "_length_") else 1) for n, t in Camera._fields_] == \
           [(n, t._length_ if hasattr(t, "_length_") else 1) for n, t in binding.Camera._fields_]


DAMAGE = {
    "lens": lambda c: setattr(c, "lens_radius", 0.2),
    "zero_steps": lambda c: (c.dx_camera.__setitem__(0, 0.0), c.dy_camera.__setitem__(1, 0.0)),
    "negative_step": lambda c: c.dx_camera.__setitem__(0, -c.dx_camera[0]),
    "nan_step": lambda c: c.dy_camera.__setitem__(1, float("nan")),
    "infinite_step": lambda c: c.dx_camera.__setitem__(0, float("inf")),
    "steps_of_another_film": lambda c: c.dx_camera.__setitem__(0, c.dx_camera[0] * 2),
    "stray_entry": lambda c: c.dy_camera.__setitem__(0, 1.0),
}


@pytest.mark.parametrize("how", list(DAMAGE))
def test_half_formed_environment_camera_is_refused(binding, tmp_path, how):
    desc = Desc(binding, load(binding, tmp_path))
    DAMAGE[how](desc.d.camera)
    assert desc.create() == (ERR_ARG, REFUSAL)


def test_steps_rounded_another_way_are_not_refused(binding, tmp_path):
    """The two steps are a tag the device does not compute with: a producer whose float rounding differs by an ulp passes the
    camera check (what stops the call after it, on a machine without a GPU, is the missing device)."""
    desc = Desc(binding, load(binding, tmp_path))
    cam = desc.d.camera
    cam.dx_camera[0] = np.nextafter(np.float32(cam.dx_camera[0]), np.float32(4))
    cam.dy_camera[1] = np.nextafter(np.float32(cam.dy_camera[1]), np.float32(0))
    assert desc.create()[1] != REFUSAL


def test_degenerate_screenwindow_is_dropped(binding, tmp_path):
    """CreateEnvironmentCamera reads "screenwindow" and drops it: a window of no extent, which no perspective camera could use,
    loads and leaves the descriptor of the camera without one."""
    plain = load(binding, tmp_path).camera()[1]
    odd = load(binding, tmp_path, camera='Camera "environment" "float screenwindow" [1 1 2 2] "float frameaspectratio" [0]').camera()[1]
    assert bytes(plain) == bytes(odd)


def test_perspective_camera_that_lost_its_matrix_is_refused(binding, tmp_path):
    """An all-zero raster_to_camera is never a perspective camera's: with dxCamera / dyCamera in the two vectors it is refused,
    not rendered as a panorama."""
    desc = Desc(binding, load(binding, tmp_path, camera='Camera "perspective" "float fov" [40]'))
    assert any(desc.d.camera.raster_to_camera)
    ctypes.memset(ctypes.addressof(desc.d.camera), 0, 64)
    assert desc.create() == (ERR_ARG, REFUSAL)
    ctypes.memset(ctypes.addressof(desc.d.camera), 0, ctypes.sizeof(Camera))  # a camera nobody filled in
    assert desc.create() == (ERR_ARG, REFUSAL)
