"""iile_scene_create refuses a malformed or unsupported descriptor before it touches a device: the same code and message on
a machine without a GPU as on one with, in the order the checks have always been made. Each test edits a copy of a loaded
scene's descriptor (the loaded scene itself stays as it was) and expects one refusal."""
import ctypes

import numpy as np
import pytest

c_i32, c_u32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
ERR_ARG, ERR_UNSUPPORTED = 1, 4
LIGHT_POINT, LIGHT_AREA_TRIANGLE, LIGHT_INFINITE = 1, 4, 5
PRIM_SPHERE, PRIM_HAS_ALPHA, PRIM_QUADRIC = 1, 16, 32
TEX_SCALE = 1


# ---- a test-only view of the whole iile_scene_desc (include/iile_scene.h) ----------------------------------------------------
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


class BvhNode(ctypes.Structure):
    _fields_ = [("bmin", c_f32 * 3), ("bmax", c_f32 * 3), ("offset", c_i32), ("nprims", ctypes.c_uint16), ("axis", ctypes.c_uint8),
                ("pad", ctypes.c_uint8)]


class Desc:
    """A copy of a loaded scene's descriptor; table() swaps one of its arrays for an editable copy."""

    def __init__(self, binding, host):
        self.binding, self.host = binding, host
        self.d = SceneDesc.from_buffer_copy(ctypes.string_at(host.desc, ctypes.sizeof(SceneDesc)))
        self._keep = []

    def table(self, name, ctype, n):
        a = (ctype * max(n, 1))()
        if n and getattr(self.d, name):  # (a null array, prim_alpha without masks: zeros)
            ctypes.memmove(a, getattr(self.d, name), n * ctypes.sizeof(ctype))
        self._keep.append(a)
        setattr(self.d, name, ctypes.addressof(a))
        return a

    def create(self):
        lib = self.binding.gpu_lib()
        out = c_vp()
        rc = lib.iile_scene_create(ctypes.addressof(self.d), ctypes.byref(out))
        if rc == 0:
            lib.iile_scene_destroy(out)
        return rc, lib.iile_last_error().decode()


# ---- one small scene with every kind of table the checks look at -----------------------------------------------------------
def _scene_text(depth=5, pixel_filter=""):
    tri = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-1 2 0  1 2 0  0 3 0]'
    quad = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 1  1 -1 1  1 1 1  -1 1 1] "float uv" [0 0 1 0 1 1 0 1]'
    return f"""LookAt 0 0 -5  0 0 0  0 1 0
Camera "perspective" "float fov" [60]
Film "image" "integer xresolution" [32] "integer yresolution" [32] "string filename" "refusals.exr"
{pixel_filter}
Sampler "halton" "integer pixelsamples" [4]
Integrator "path" "integer maxdepth" [{depth}]
WorldBegin
LightSource "point" "rgb I" [1 1 1] "point from" [0 0 -3]
Texture "ia" "spectrum" "imagemap" "string filename" ["a.pfm"]
Material "matte" "texture Kd" "ia"
{quad}
AttributeBegin
AreaLightSource "diffuse" "rgb L" [1 1 1]
Translate 0 0 2
Shape "sphere" "float radius" [0.5]
AttributeEnd
AttributeBegin
AreaLightSource "diffuse" "rgb L" [1 1 1]
{tri}
AttributeEnd
AttributeBegin
Translate 0 -2 0
Shape "disk" "float radius" [1]
AttributeEnd
WorldEnd
"""


def _host(binding, tmp_path, sampler=None, **kw):
    with open(tmp_path / "a.pfm", "wb") as f:
        f.write(b"PF\n2 2\n-1.0\n" + np.full((2, 2, 3), 0.5, "<f4").tobytes())
    path = tmp_path / "refusals.pbrt"
    path.write_text(_scene_text(**kw))
    return binding.HostScene(path=str(path), sampler=sampler)


@pytest.fixture
def desc(binding, tmp_path):
    return Desc(binding, _host(binding, tmp_path))


def _prims(desc, mask):
    flags = np.ctypeslib.as_array(desc.table("prim_flags", c_u32, desc.d.n_prims))
    return flags, [i for i in range(desc.d.n_prims) if flags[i] & mask == mask]


def _light_of_type(desc, lights, light_type):
    return next(i for i in range(desc.d.n_lights) if lights[i].type == light_type)


def test_maxdepth_15_from_the_scene_file(binding, tmp_path):
    """The loader sizes the Halton table for maxdepth 15 at more dimensions than the device keeps: that check comes first."""
    host = _host(binding, tmp_path, depth=15)
    assert host.info["max_depth"] == 15
    assert Desc(binding, host).create() == (ERR_UNSUPPORTED, "too many Halton dimensions")


def test_maxdepth_above_14(desc):
    desc.d.integrator.max_depth = 15
    desc.d.halton.n_dims = 128  # (enough dimensions for maxdepth 15)
    assert desc.create() == (ERR_UNSUPPORTED, "maxdepth > 14")


def test_halton_table_too_short_for_maxdepth(desc):
    desc.d.halton.n_dims = 5 + 8 * desc.d.integrator.max_depth
    assert desc.create() == (ERR_ARG, "Halton table covers too few dimensions for maxdepth")


def test_filter_radius_above_16(binding, tmp_path):
    host = _host(binding, tmp_path, pixel_filter='PixelFilter "box" "float xwidth" [20]')
    assert Desc(binding, host).create() == (ERR_UNSUPPORTED, "pixel filter radius must lie in (0, 16]")


def test_bad_bvh_leaf_range(desc):
    nodes = desc.table("nodes", BvhNode, desc.d.n_nodes)
    leaf = next(i for i in range(desc.d.n_nodes) if nodes[i].nprims > 0)
    nodes[leaf].offset = desc.d.n_prims
    assert desc.create() == (ERR_ARG, "bad leaf range")


def test_bad_bvh_child_index(desc):
    nodes = desc.table("nodes", BvhNode, desc.d.n_nodes)
    assert nodes[0].nprims == 0
    nodes[0].offset = 0
    assert desc.create() == (ERR_ARG, "bad BVH child index")


def test_sphere_primitive_without_its_sphere(desc):
    _, spheres = _prims(desc, PRIM_SPHERE)
    shape = desc.table("prim_shape", c_i32, desc.d.n_prims)
    shape[spheres[0]] = desc.d.n_spheres
    assert desc.create() == (ERR_ARG, "sphere primitive without its sphere")


def test_unsupported_quadric_kind(binding, desc):
    desc.table("quadrics", binding.Quadric, desc.d.n_quadrics)[0].kind = 2
    assert desc.create() == (ERR_UNSUPPORTED, "unsupported quadric kind")


def test_quadric_primitive_without_its_quadric(desc):
    _, quadrics = _prims(desc, PRIM_QUADRIC)
    shape = desc.table("prim_shape", c_i32, desc.d.n_prims)
    shape[quadrics[0]] = -1
    assert desc.create() == (ERR_ARG, "quadric primitive without its quadric")


def test_triangle_area_light_whose_primitive_does_not_point_back(binding, desc):
    lights = desc.table("lights", binding.Light, desc.d.n_lights)
    light = lights[_light_of_type(desc, lights, LIGHT_AREA_TRIANGLE)]
    desc.table("prim_light", c_i32, desc.d.n_prims)[light.prim] = -1
    assert desc.create() == (ERR_ARG, "triangle area light without its triangle")


def test_unsupported_material_type(binding, desc):
    desc.table("materials", binding.Material, desc.d.n_materials)[0].type = 7
    assert desc.create() == (ERR_UNSUPPORTED, "unsupported material type")


def test_material_texture_index_out_of_range(binding, desc):
    mats = desc.table("materials", binding.Material, desc.d.n_materials)
    mats[0].ks_tex = desc.d.n_textures
    assert desc.create() == (ERR_ARG, "material refers to a texture that does not exist")


def test_material_texture_indices_are_checked_as_clamped(binding, desc):
    """Without textures every index becomes -1, and a non-uber material's opacity texture is ignored: neither is refused (the
    first refusal is a later check's)."""
    mats = desc.table("materials", binding.Material, desc.d.n_materials)
    mats[0].opacity_tex = 5
    desc.d.sobol.enabled = 1  # (a Sobol' table of no dimensions: refused last)
    assert desc.create()[1].startswith("iile_sobol: bad dimension count")
    mats[0].opacity_tex, mats[0].kd_tex = -1, 5
    desc.d.n_textures = 0
    assert desc.create()[1].startswith("iile_sobol: bad dimension count")


def test_alpha_mask_without_its_texture(desc):
    flags, _ = _prims(desc, 0)
    flags[0] |= PRIM_HAS_ALPHA
    alpha = desc.table("prim_alpha", c_i32, 2 * desc.d.n_prims)
    for i in range(2 * desc.d.n_prims):
        alpha[i] = -1
    alpha[1] = desc.d.n_textures
    assert desc.create() == (ERR_ARG, "alpha mask refers to a texture that does not exist")


def test_texture_input_that_is_not_a_leaf(binding, desc):
    tex = desc.table("textures", binding.Texture, 2)  # two scale textures, the first one over the second
    desc.d.n_textures = 2
    tex[0].kind = tex[1].kind = TEX_SCALE
    tex[0].n_levels = tex[1].n_levels = 0
    tex[0].child[:] = [1, -1, -1]
    tex[1].child[:] = [-1, -1, -1]
    assert desc.create() == (ERR_ARG, "texture input that is not a leaf (textures nest two levels deep at most)")
    tex[0].child[:] = [2, -1, -1]
    assert desc.create() == (ERR_ARG, "texture input out of range")


def test_bad_infinite_light_table(binding, desc):
    lights = desc.table("lights", binding.Light, desc.d.n_lights)
    point = lights[_light_of_type(desc, lights, LIGHT_POINT)]
    point.type, point.env_tex, point.dist_w, point.dist_h, point.dist_offset = LIGHT_INFINITE, 0, 2, 2, 0
    assert desc.create() == (ERR_ARG, "infinite light: bad environment map / distribution reference")  # (no env_dist)


def test_sobol_resolution(binding, tmp_path):
    desc = Desc(binding, _host(binding, tmp_path, sampler="sobol"))
    sb = desc.d.sobol
    assert sb.enabled == 1 and sb.resolution == 32 and sb.log2_resolution == 5
    sb.resolution = 24
    assert desc.create() == (ERR_ARG, "iile_sobol: bad dimension count / resolution, or sample indices beyond 32 bits")
    sb.resolution, sb.log2_resolution = 16, 4
    assert desc.create() == (ERR_ARG, "iile_sobol: resolution smaller than the sample bounds")


def _chain_scene(binding, tmp_path, depth):
    """A scene whose tree is a left-leaning chain of `depth` interior nodes over depth + 1 unit boxes, handed in through the
    bvh_build hook: node i's first child is node i + 1, its second the leaf 2 * depth - i."""
    proto = ctypes.CFUNCTYPE(ctypes.c_int, c_i32, c_vp, c_i32, c_vp, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_vp)
    n_prims = depth + 1

    def chain(n, bounds6, max_prims, nodes_out, n_nodes, order, stats):
        assert n == n_prims
        b = np.ctypeslib.as_array(ctypes.cast(bounds6, ctypes.POINTER(c_f32)), (n, 6))
        nodes = ctypes.cast(nodes_out, ctypes.POINTER(BvhNode))
        for i in range(depth):      # interior node i holds primitives 0 .. depth - i
            nodes[i].bmin[:] = b[:depth - i + 1, :3].min(0).tolist()
            nodes[i].bmax[:] = b[:depth - i + 1, 3:].max(0).tolist()
            nodes[i].offset, nodes[i].nprims, nodes[i].axis, nodes[i].pad = 2 * depth - i, 0, 0, 0
        for j in range(n):          # leaf of primitive j: node `depth` for j = 0, else node depth + j
            leaf = nodes[depth + j]
            leaf.bmin[:], leaf.bmax[:] = b[j, :3].tolist(), b[j, 3:].tolist()
            leaf.offset, leaf.nprims, leaf.axis, leaf.pad = j, 1, 0, 0
            order[j] = j
        n_nodes[0] = 2 * depth + 1
        return 0

    tris = " ".join("%d 0 0  %d 1 0  %d 1 1" % (j, j + 1, j + 1) for j in range(n_prims))   # one triangle per unit box along x
    text = f"""LookAt 0 0 -5  0 0 0  0 1 0
Camera "perspective" "float fov" [60]
Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "chain.exr"
Sampler "halton" "integer pixelsamples" [1]
Accelerator "bvh" "string splitmethod" ["hlbvh"] "integer maxnodeprims" [1]
WorldBegin
Material "matte"
Shape "trianglemesh" "point P" [ {tris} ] "integer indices" [ {" ".join(str(i) for i in range(3 * n_prims))} ]
WorldEnd
"""
    path = tmp_path / f"chain{depth}.pbrt"
    path.write_text(text)
    host = binding.HostScene(path=str(path), bvh_on_device=proto(chain))
    assert host.info["n_nodes"] == 2 * depth + 1 and host.info["n_interior_nodes"] == depth
    return host


def test_bvh_deeper_than_the_traversal_stack(binding, tmp_path):
    """A tree one level deeper than the traversal stack is sure to hold (iile_traversal_limits: the reference's own 64) is refused,
    naming the depth; nothing is ever traced on it."""
    limit = binding.traversal_limits()["max_bvh_depth"]
    desc = Desc(binding, _chain_scene(binding, tmp_path, limit + 1))
    assert desc.create() == (ERR_UNSUPPORTED, f"BVH depth {limit + 1} exceeds the traversal stack's limit of {limit} levels")


def test_bvh_exactly_as_deep_as_the_limit_is_accepted(binding, tmp_path):
    """A chain of exactly the limit's depth passes every refusal (the first one left is a later check's, as in
    test_material_texture_indices_are_checked_as_clamped); it is not traced either."""
    limit = binding.traversal_limits()["max_bvh_depth"]
    desc = Desc(binding, _chain_scene(binding, tmp_path, limit))
    desc.d.sobol.enabled = 1  # (a Sobol' table of no dimensions: refused last)
    assert desc.create()[1].startswith("iile_sobol: bad dimension count")
    if binding.device_count() > 0:
        desc.d.sobol.enabled = 0
        assert desc.create()[0] == 0
