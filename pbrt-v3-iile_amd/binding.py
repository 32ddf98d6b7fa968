"""ctypes bindings over the two C-ABI libraries of the path.

    libiile_host.so  scene preparation + film finalisation   (include/iile_host.h)
    libiile_gpu.so   gfx950 wavefront path tracer            (include/iile_gpu.h)
    libiile_dist.so  the multi-GPU film merge over RCCL      (include/iile_dist.h)

Python is plumbing only (tests, bench.py, __graft_entry__): every number comes
out of the HIP kernels. There is no CPU fallback here — if libiile_gpu.so is
missing or no GPU is visible, the calls raise.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
REPO_ROOT = os.path.dirname(_HERE)
DEFAULT_SCENE = os.path.join(REPO_ROOT, "scenes", "killeroo-simple.pbrt")

c_i32, c_u32, c_u64, c_f32, c_f64 = (ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float,
                                     ctypes.c_double)
c_vp = ctypes.c_void_p


class HostOverrides(ctypes.Structure):
    _fields_ = [("xres", c_i32), ("yres", c_i32), ("spp", c_i32), ("max_depth", c_i32), ("sampler", c_i32),
                ("accel_split", c_i32), ("bvh_build", c_vp), ("quick_render", c_i32)]


SAMPLERS = {None: 0, "": 0, "halton": 1, "sobol": 2}  # IILE_SAMPLER_* of include/iile_host.h
SPLITS = {None: 0, "": 0, "sah": 1, "hlbvh": 2, "middle": 3, "equal": 4}  # IILE_SPLIT_*


class HostSceneInfo(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("n_prims n_triangles n_spheres n_meshes n_nodes n_interior_nodes "
                                      "n_leaf_nodes n_materials n_lights xres yres spp max_depth probe_hemi_size integrator").split()]


class Camera(ctypes.Structure):
    """iile_camera (include/iile_scene.h). An environment camera keeps a zero raster_to_camera and the angle steps
    2 pi / xres, pi / yres in dx_camera[0], dy_camera[1] (IILE_ENVCAM_*)."""
    _fields_ = [("raster_to_camera", c_f32 * 16), ("camera_to_world", c_f32 * 16), ("lens_radius", c_f32), ("focal_distance", c_f32),
                ("shutter_open", c_f32), ("shutter_close", c_f32), ("dx_camera", c_f32 * 3), ("dy_camera", c_f32 * 3)]


CAMERA_PERSPECTIVE, CAMERA_ENVIRONMENT = range(2)  # IILE_CAMERA_* of include/iile_scene.h
ERR_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_TIMEOUT = range(1, 6)  # IILE_ERR_* of include/iile_gpu.h


class FilmDesc(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in "xres yres crop_x0 crop_y0 crop_x1 crop_y1 samp_x0 samp_y0 samp_x1 samp_y1".split()
                ] + [(n, c_f32) for n in "filter_rx filter_ry scale max_sample_luminance".split()]


class Texture(ctypes.Structure):
    """iile_texture (include/iile_scene.h)."""
    _fields_ = [("n_levels", c_i32), ("wrap", c_i32), ("trilinear", c_i32), ("max_aniso", c_f32), ("su", c_f32),
                ("sv", c_f32), ("du", c_f32), ("dv", c_f32), ("level_w", c_i32 * 16), ("level_h", c_i32 * 16),
                ("level_offset", ctypes.c_int64 * 16),
                # procedural textures (all zero for an image): appended, include/iile_scene.h
                ("kind", c_i32), ("mapping", c_i32), ("vs", c_f32 * 3), ("vt", c_f32 * 3), ("xf", c_f32 * 12), ("child", c_i32 * 3),
                ("cval", (c_f32 * 3) * 3), ("aamode", c_i32), ("bilerp", (c_f32 * 3) * 4)]


# iile_texture::kind, ::mapping, ::aamode
TEX_IMAGE, TEX_SCALE, TEX_MIX, TEX_CHECKER2D, TEX_CHECKER3D, TEX_UV, TEX_BILERP = range(7)
MAP_UV, MAP_SPHERICAL, MAP_CYLINDRICAL, MAP_PLANAR = range(4)
AA_CLOSEDFORM, AA_NONE = range(2)


class Light(ctypes.Structure):
    """iile_light (include/iile_scene.h)."""
    _fields_ = [("lemit", c_f32 * 3), ("two_sided", c_i32), ("sphere", c_i32), ("type", c_i32), ("pos", c_f32 * 3), ("w2l", c_f32 * 9),
                ("cos_total_width", c_f32), ("cos_falloff_start", c_f32), ("world_radius", c_f32), ("prim", c_i32), ("n_samples", c_i32),
                ("l2w", c_f32 * 9), ("env_tex", c_i32), ("dist_w", c_i32), ("dist_h", c_i32), ("dist_offset", ctypes.c_int64)]

    def projection(self):
        """What a projection light keeps in l2w (IILE_PROJ_*, include/iile_scene.h): m[0][0] and m[1][1] of lightProjection, hither,
        fov and screenBounds {pMin.x, pMin.y, pMax.x, pMax.y}."""
        v = list(self.l2w)
        return {"m00": v[0], "m11": v[1], "hither": v[2], "fov": v[3], "screen_bounds": v[4:8]}


# iile_light::type
(LIGHT_DIFFUSE_AREA, LIGHT_POINT, LIGHT_SPOT, LIGHT_DISTANT, LIGHT_AREA_TRIANGLE, LIGHT_INFINITE, LIGHT_AREA_QUADRIC, LIGHT_PROJECTION,
 LIGHT_GONIOMETRIC) = range(9)


class RenderParams(ctypes.Structure):
    _fields_ = [("k_begin", c_i32), ("k_end", c_i32), ("tile_rank", c_i32), ("tile_nranks", c_i32),
                ("spp_per_pass", c_i32), ("collect_stats", c_i32), ("time_kernels", c_i32),
                ("film_on_device", c_i32), ("stream", c_vp)]


class AoParams(ctypes.Structure):
    """iile_ao_params (include/iile_scene.h): "nsamples" and "cossample" of Integrator "ambientocclusion"."""
    _fields_ = [("n_samples", c_i32), ("cos_sample", c_i32)]


INTEGRATOR_PATH, INTEGRATOR_IISPT, INTEGRATOR_AO = range(3)  # iile_host_scene_info::integrator


class CameraMotion(ctypes.Structure):
    """iile_camera_motion (include/iile_scene.h): a moving camera's AnimatedTransform."""
    _fields_ = [("start_time", c_f32), ("end_time", c_f32), ("camera_to_world_end", c_f32 * 16), ("T", (c_f32 * 3) * 2),
                ("R", (c_f32 * 4) * 2), ("S", (c_f32 * 16) * 2), ("has_rotation", c_i32)]


class IisptTask(ctypes.Structure):
    """iile_iispt_task (include/iile_scene.h): one task of the IISPT render runner."""
    _fields_ = [("x0", c_i32), ("y0", c_i32), ("x1", c_i32), ("y1", c_i32), ("tilesize", c_i32), ("counter_base", c_u32),
                ("rng_seed", c_u64)]

    def grid(self):
        def count(a0, a1, ts):
            n, t = 1, a0
            while t != a1 - 1:
                t = min(t + ts, a1 - 1)
                n += 1
            return n
        return count(self.x0, self.x1, self.tilesize), count(self.y0, self.y1, self.tilesize)


# iile_bvh_node (include/iile_scene.h): LinearBVHNode
BVH_NODE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("offset", "<i4"), ("nprims", "<u2"), ("axis", "u1"), ("pad", "u1")])


class BvhBuildStats(ctypes.Structure):
    _fields_ = [(n, c_f32) for n in "ms_total ms_morton ms_sort ms_treelets ms_upper ms_flatten ms_download".split()] + [
        (n, c_i32) for n in "n_treelets n_nodes n_interior n_leaf".split()]


class SceneDescHead(ctypes.Structure):
    """The first members of iile_scene_desc (include/iile_scene.h): the flattened BVH and the primitives in BVH order."""
    _fields_ = [("n_nodes", c_i32), ("nodes", c_vp), ("n_prims", c_i32), ("prim_flags", c_vp), ("prim_material", c_vp),
                ("prim_light", c_vp), ("prim_shape", c_vp), ("tri_p", c_vp)]


class _Halton(ctypes.Structure):
    _fields_ = [("spp", c_i32), ("base_scales", c_i32 * 2), ("base_exponents", c_i32 * 2), ("sample_stride", c_i32),
                ("mult_inverse", c_i32 * 2), ("n_dims", c_i32), ("perms", c_vp), ("primes", c_vp), ("prime_sums", c_vp),
                ("n_perms", c_i32), ("sample_at_pixel_center", c_i32)]


class Integrator(ctypes.Structure):
    """iile_integrator (include/iile_scene.h); light_power holds the first MAX_LIGHTS lights' power."""
    _fields_ = [("max_depth", c_i32), ("rr_threshold", c_f32), ("light_strategy", c_i32), ("light_power", c_f32 * 8),
                ("pixel_bounds", c_i32 * 4)]


class _ProbeSetup(ctypes.Structure):
    _fields_ = [("hemi_size", c_i32), ("max_depth", c_i32), ("film", FilmDesc), ("filter_table", c_f32 * 256), ("base_scales", c_i32 * 2),
                ("base_exponents", c_i32 * 2), ("sample_stride", c_i32), ("mult_inverse", c_i32 * 2)]


class _Sobol(ctypes.Structure):
    _fields_ = [("enabled", c_i32), ("spp", c_i32), ("resolution", c_i32), ("log2_resolution", c_i32), ("n_dims", c_i32),
                ("matrices32", c_vp), ("vdc", c_u32 * 32), ("vdc_inv", c_u32 * 32)]


class SceneDesc(ctypes.Structure):
    """The whole iile_scene_desc (include/iile_scene.h), light_power_all and disney at its end."""
    _fields_ = SceneDescHead._fields_ + [
        ("tri_n", c_vp), ("tri_uv", c_vp), ("prim_alpha", c_vp), ("n_spheres", c_i32), ("spheres", c_vp), ("n_materials", c_i32),
        ("materials", c_vp), ("n_lights", c_i32), ("lights", c_vp), ("n_env_dist", ctypes.c_int64), ("env_dist", c_vp),
        ("n_textures", c_i32), ("textures", c_vp), ("n_texels", ctypes.c_int64), ("texels", c_vp), ("ewa_lut", c_f32 * 128),
        ("film_filter_wide", c_i32), ("film_filter_table", c_f32 * 256), ("camera", Camera), ("film", FilmDesc), ("halton", _Halton),
        ("integrator", Integrator), ("probe", _ProbeSetup), ("sobol", _Sobol), ("n_quadrics", c_i32), ("quadrics", c_vp),
        ("light_power_all", c_vp), ("disney", c_vp)]


MAX_LIGHTS = 8  # IILE_MAX_LIGHTS: the length of iile_integrator::light_power, not a limit on the lights of a scene


class Quadric(ctypes.Structure):
    """iile_quadric (include/iile_scene.h): a disk or a cylinder."""
    _fields_ = [("o2w", c_f32 * 16), ("o2w_inv", c_f32 * 16), ("kind", c_i32), ("radius", c_f32), ("inner_radius", c_f32),
                ("height", c_f32), ("zmin", c_f32), ("zmax", c_f32), ("phi_max", c_f32), ("reverse_orientation", c_i32),
                ("swaps_handedness", c_i32)]


class Material(ctypes.Structure):
    """iile_material (include/iile_scene.h)."""
    _fields_ = [("type", c_i32), ("kd", c_f32 * 3), ("ks", c_f32 * 3), ("sigma", c_f32), ("roughness", c_f32), ("alpha", c_f32),
                ("remap_roughness", c_i32), ("eta", c_f32), ("kr", c_f32 * 3), ("kt", c_f32 * 3), ("on_a", c_f32), ("on_b", c_f32),
                ("kd_tex", c_i32), ("ks_tex", c_i32), ("kr_tex", c_i32), ("kt_tex", c_i32), ("bump_tex", c_i32), ("rough_tex", c_i32),
                ("sigma_tex", c_i32), ("opacity", c_f32 * 3), ("roughness_v", c_f32), ("alpha_v", c_f32), ("opacity_tex", c_i32),
                ("rough_tex_v", c_i32), ("cond_eta", c_f32 * 3), ("cond_k", c_f32 * 3)]


MAT_MATTE, MAT_PLASTIC, MAT_UBER, MAT_MIRROR, MAT_GLASS, MAT_METAL, MAT_SUBSTRATE = range(7)
MAT_TRANSLUCENT = 8  # (7 is not a material type)
MAT_DISNEY = 10  # (9, like 7, is not a material type)


class Disney(ctypes.Structure):
    """iile_disney (include/iile_scene.h): the scalar parameters of a Disney material, iile_scene_desc::disney[material]."""
    _fields_ = [(n, c_f32) for n in ("metallic specular_tint anisotropic sheen sheen_tint clearcoat clearcoat_gloss spec_trans "
                                     "flatness diff_trans").split()] + [("thin", c_i32), ("pad_", c_i32)]
QUADRIC_DISK, QUADRIC_CYLINDER = 0, 1
PRIM_SPHERE, PRIM_FLIP, PRIM_QUADRIC = 1, 8, 32
LIGHT_AREA_QUADRIC = 6


class GpuStats(ctypes.Structure):
    _fields_ = [(n, c_u64) for n in ("camera_rays closest_rays shadow_rays nodes_closest nodes_any tri_tests "
                                     "tri_hits sphere_tests nee_evals zero_radiance").split()] + [
        ("path_length", c_u64 * 8),
        ("ms_total", c_f64), ("ms_generate", c_f64), ("ms_extend", c_f64), ("ms_shade", c_f64),
        ("ms_connect", c_f64), ("ms_film", c_f64),
        ("n_extend_launches", c_i32), ("n_connect_launches", c_i32), ("n_shade_launches", c_i32),
        ("n_passes", c_i32), ("n_paths", c_u64), ("workspace_bytes", c_u64),
        ("ext_rays", c_u64), ("ext_nodes", c_u64), ("ext_tri_tests", c_u64), ("ext_sphere_tests", c_u64),
        ("any_tri_tests", c_u64), ("ms_shadow", c_f64), ("ms_mis", c_f64), ("ms_resolve", c_f64),
        ("mis_rays_traced", c_u64), ("ext_rays_traced", c_u64)]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if name == "path_length" else v
        return d


# every symbol the headers declare; checked by tests/test_abi.py
HOST_SYMBOLS = ["iile_host_load_pbrt", "iile_host_scene_desc", "iile_host_scene_film", "iile_host_scene_get_info",
                "iile_host_scene_free", "iile_host_film_to_rgb", "iile_host_write_pfm", "iile_host_last_error", "iile_host_read_image",
                "iile_host_scene_texture", "iile_host_scene_texture_level", "iile_host_scene_filter_table",
                "iile_host_sobol_matrices", "iile_host_sobol_vdc", "iile_host_write_exr", "iile_host_write_image",
                "iile_host_scene_film_filename", "iile_host_scene_light", "iile_host_scene_quadric_count", "iile_host_scene_quadric",
                "iile_host_scene_material", "iile_host_scene_camera", "iile_host_scene_ao", "iile_host_scene_camera_motion"]
class NetWeights(ctypes.Structure):
    """iile_iispt_net_weights (include/iile_gpu.h)."""
    _fields_ = [("conv_weight", c_vp * 15), ("conv_bias", c_vp * 15), ("bn_weight", c_vp * 5), ("bn_bias", c_vp * 5),
                ("bn_mean", c_vp * 5), ("bn_var", c_vp * 5), ("bn_eps", c_f32)]


class ProbeRefParams(ctypes.Structure):  # iile_probe_ref_params
    _fields_ = [("max_depth", c_i32), ("first_sample", c_i32), ("n_samples", c_i32), ("spp_total", c_i32), ("outputs_on_device", c_i32),
                ("stream", c_vp)]


class DirectParams(ctypes.Structure):  # iile_direct_params
    _fields_ = [("n_passes", ctypes.c_int32), ("first_pass", ctypes.c_int32), ("accumulate", ctypes.c_int32), ("film_on_device", ctypes.c_int32),
                ("stream", ctypes.c_void_p)]


GPU_SYMBOLS = ["iile_device_count", "iile_last_error", "iile_scene_create", "iile_scene_destroy", "iile_render",
               "iile_scene_set_camera_motion", "iile_camera_rays_at",
               "iile_render_ao", "iile_ao_array_samples", "iile_ao_li_samples",
               "iile_trace_closest", "iile_trace_any", "iile_shape_hit_attributes", "iile_halton_samples", "iile_sample_table_records", "iile_sample_table_budget", "iile_test_sample_table_budget", "iile_sample_table_bytes", "iile_camera_rays", "iile_li_samples",
               "iile_bsdf_eval", "iile_bsdf_sample", "iile_bsdf_eval_ng", "iile_bsdf_sample_ng", "iile_bsdf_sample_specular", "iile_trig_probe", "iile_texture_eval", "iile_texture_eval_p", "iile_light_sample_li", "iile_light_sample_at", "iile_light_pdf_at", "iile_light_le", "iile_light_choose", "iile_render_probes",
               "iile_render_probes_reference", "iile_test_probe_ref_group", "iile_reference_points",
               "iile_device_select", "iile_device_alloc", "iile_device_free", "iile_device_download", "iile_device_upload", "iile_device_zero",
               "iile_stream_create", "iile_stream_wait", "iile_stream_destroy",
               "iile_iispt_film_add", "iile_iispt_film_merge",
               "iile_iispt_hemi_points", "iile_iispt_gather", "iile_iispt_hemi_points_batch", "iile_iispt_gather_batch", "iile_bvh_build_hlbvh", "iile_bvh_pack_probe", "iile_render_direct",
               "iile_wide_ref_shift", "iile_traversal_limits", "iile_render_status", "iile_test_patch_capacity", "iile_iispt_net_create", "iile_iispt_net_load", "iile_iispt_net_forward", "iile_iispt_net_predict", "iile_iispt_net_destroy"]
DIST_SYMBOLS = ["iile_dist_unique_id", "iile_dist_create", "iile_dist_create_deadline", "iile_dist_abort", "iile_dist_wait", "iile_dist_destroy", "iile_dist_rank", "iile_dist_size", "iile_dist_ranks_seen",
                "iile_dist_film_reduce", "iile_dist_monitor_reduce", "iile_dist_barrier", "iile_dist_sum_u64", "iile_dist_max_f64",
                "iile_dist_rendezvous_file", "iile_dist_rendezvous_file_token", "iile_dist_rendezvous_done", "iile_dist_all_ok",
                "iile_dist_last_error"]
DIST_ID_BYTES = 128

_host = None
_gpu = None
_dist = None


def host_lib():
    global _host
    if _host is None:
        path = os.path.join(LIB_DIR, "libiile_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (make -C pbrt-v3-iile_amd/csrc host)")
        lib = ctypes.CDLL(path)
        lib.iile_host_last_error.restype = ctypes.c_char_p
        lib.iile_host_load_pbrt.argtypes = [ctypes.c_char_p, ctypes.POINTER(HostOverrides), ctypes.POINTER(c_vp)]
        lib.iile_host_scene_desc.restype = c_vp
        lib.iile_host_scene_desc.argtypes = [c_vp]
        lib.iile_host_scene_film.restype = ctypes.POINTER(FilmDesc)
        lib.iile_host_scene_film.argtypes = [c_vp]
        lib.iile_host_scene_get_info.argtypes = [c_vp, ctypes.POINTER(HostSceneInfo)]
        lib.iile_host_scene_ao.argtypes = [c_vp, ctypes.POINTER(AoParams)]
        lib.iile_host_scene_free.argtypes = [c_vp]
        lib.iile_host_scene_free.restype = None
        lib.iile_host_scene_quadric_count.argtypes = [c_vp]
        lib.iile_host_scene_quadric_count.restype = c_i32
        lib.iile_host_scene_quadric.argtypes = [c_vp, c_i32, ctypes.POINTER(Quadric)]
        lib.iile_host_scene_material.argtypes = [c_vp, c_i32, ctypes.POINTER(Material)]
        lib.iile_host_scene_camera.argtypes = [c_vp, ctypes.POINTER(Camera)]
        lib.iile_host_scene_camera_motion.argtypes = [c_vp, ctypes.POINTER(CameraMotion)]
        lib.iile_host_film_to_rgb.argtypes = [ctypes.POINTER(FilmDesc), c_vp, c_vp]
        lib.iile_host_write_pfm.argtypes = [ctypes.c_char_p, c_vp, c_i32, c_i32]
        lib.iile_host_read_image.argtypes = [ctypes.c_char_p, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_vp]
        lib.iile_host_write_exr.argtypes = [ctypes.c_char_p, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32]
        lib.iile_host_write_image.argtypes = [ctypes.c_char_p, ctypes.POINTER(FilmDesc), c_vp]
        lib.iile_host_scene_film_filename.argtypes = [c_vp]
        lib.iile_host_scene_film_filename.restype = ctypes.c_char_p
        lib.iile_host_scene_texture.argtypes = [c_vp, c_i32, ctypes.POINTER(Texture)]
        lib.iile_host_scene_texture_level.argtypes = [c_vp, c_i32, c_i32, c_vp]
        lib.iile_host_scene_filter_table.argtypes = [c_vp, c_vp]
        lib.iile_host_sobol_matrices.argtypes = [c_i32, c_vp, c_vp]
        lib.iile_host_sobol_vdc.argtypes = [c_i32, c_vp, c_vp]
        _host = lib
    return _host


def sobol_matrices(n_dims):
    """(SobolMatrices32, SobolMatrices64) as the host builds them: (n_dims, 52) uint32 / uint64."""
    m32 = np.zeros((n_dims, 52), np.uint32)
    m64 = np.zeros((n_dims, 52), np.uint64)
    if host_lib().iile_host_sobol_matrices(int(n_dims), m32.ctypes.data, m64.ctypes.data) != 0:
        raise RuntimeError(host_lib().iile_host_last_error().decode())
    return m32, m64


def sobol_vdc(log2_resolution):
    """(VdCSobolMatrices[m - 1], VdCSobolMatricesInv[m - 1]) as the host builds them: 52 uint64 each."""
    vdc = np.zeros(52, np.uint64)
    inv = np.zeros(52, np.uint64)
    if host_lib().iile_host_sobol_vdc(int(log2_resolution), vdc.ctypes.data, inv.ctypes.data) != 0:
        raise RuntimeError(host_lib().iile_host_last_error().decode())
    return vdc, inv


def read_image(path):
    """ReadImage for .pfm / .png / .tga: (H, W, 3) float32, row 0 = top scanline."""
    lib = host_lib()
    w, h = c_i32(), c_i32()
    if lib.iile_host_read_image(os.fsencode(path), ctypes.byref(w), ctypes.byref(h), None) != 0:
        raise RuntimeError(lib.iile_host_last_error().decode())
    rgb = np.empty((h.value, w.value, 3), np.float32)
    if lib.iile_host_read_image(os.fsencode(path), ctypes.byref(w), ctypes.byref(h), rgb.ctypes.data) != 0:
        raise RuntimeError(lib.iile_host_last_error().decode())
    return rgb


def write_exr(path, rgb, origin=(0, 0), display=None):
    """WriteImageEXR: (H, W, 3) float32 (row 0 = top scanline) as a half-float RGB OpenEXR file; `origin` = (x0, y0) of
    the data window, `display` = (total_w, total_h) of the display window (default: the image itself)."""
    rgb = _f32(rgb)
    h, w = rgb.shape[:2]
    x0, y0 = origin
    tw, th = display if display else (x0 + w, y0 + h)
    if host_lib().iile_host_write_exr(os.fsencode(path), rgb.ctypes.data, x0, y0, x0 + w, y0 + h, tw, th) != 0:
        raise RuntimeError(host_lib().iile_host_last_error().decode())


def gpu_lib():
    """The HIP library. Fails loudly when it has not been built."""
    global _gpu
    if _gpu is None:
        # IILE_GPU_LIB selects an alternative build of the same library (kernel A/B experiments)
        path = os.environ.get("IILE_GPU_LIB") or os.path.join(LIB_DIR, "libiile_gpu.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: the HIP extension was not built; there is no CPU fallback "
                               "(run __graft_entry__.build())")
        lib = ctypes.CDLL(path)
        lib.iile_last_error.restype = ctypes.c_char_p
        lib.iile_scene_create.argtypes = [c_vp, ctypes.POINTER(c_vp)]
        lib.iile_scene_destroy.argtypes = [c_vp]
        lib.iile_scene_destroy.restype = None
        lib.iile_render.argtypes = [c_vp, ctypes.POINTER(RenderParams), c_vp, ctypes.POINTER(GpuStats)]
        lib.iile_render_ao.argtypes = [c_vp, ctypes.POINTER(AoParams), ctypes.POINTER(RenderParams), c_vp, ctypes.POINTER(GpuStats)]
        lib.iile_ao_array_samples.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]
        lib.iile_ao_li_samples.argtypes = [c_vp, ctypes.POINTER(AoParams), c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]
        lib.iile_trace_closest.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(GpuStats)]
        lib.iile_trace_any.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(GpuStats)]
        lib.iile_halton_samples.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]
        lib.iile_camera_rays.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]
        lib.iile_camera_rays_at.argtypes = [c_vp, c_i32, c_vp, c_vp, c_f32, c_vp, c_vp]
        lib.iile_scene_set_camera_motion.argtypes = [c_vp, ctypes.POINTER(CameraMotion)]
        lib.iile_li_samples.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]
        lib.iile_bsdf_eval.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]
        lib.iile_texture_eval.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]
        lib.iile_light_sample_li.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp]
        lib.iile_light_sample_at.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]
        lib.iile_light_pdf_at.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]
        lib.iile_light_le.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp]
        lib.iile_light_choose.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]
        lib.iile_texture_eval_p.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]
        lib.iile_render_probes.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, ctypes.POINTER(GpuStats), c_vp]
        lib.iile_render_probes_reference.argtypes = [c_vp, c_i32, c_vp, c_vp, ctypes.POINTER(ProbeRefParams), c_vp, c_vp, c_vp, c_vp,
                                                     ctypes.POINTER(GpuStats)]
        lib.iile_test_probe_ref_group.argtypes = [c_vp, c_u32]
        lib.iile_reference_points.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]
        lib.iile_bsdf_sample.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]
        lib.iile_bsdf_eval_ng.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]
        lib.iile_bsdf_sample_ng.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]
        lib.iile_bsdf_sample_specular.argtypes = [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]
        lib.iile_trig_probe.argtypes = [c_i32, c_vp, c_vp]
        lib.iile_iispt_hemi_points.argtypes = [c_vp, ctypes.POINTER(IisptTask), c_vp, c_vp, c_vp]
        lib.iile_iispt_gather.argtypes = [c_vp, ctypes.POINTER(IisptTask), c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32]
        lib.iile_iispt_hemi_points_batch.argtypes = [c_vp, ctypes.POINTER(IisptTask), c_i32, c_vp, c_vp, c_vp, c_vp]
        lib.iile_iispt_gather_batch.argtypes = [c_vp, ctypes.POINTER(IisptTask), c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i32, c_vp]
        lib.iile_bvh_build_hlbvh.argtypes = [c_i32, c_vp, c_i32, c_vp, ctypes.POINTER(c_i32), c_vp, ctypes.POINTER(BvhBuildStats)]
        lib.iile_bvh_pack_probe.argtypes = [c_i32, c_vp, c_i32, c_vp, c_vp, ctypes.POINTER(c_i32)]
        lib.iile_render_status.argtypes = [c_vp, c_vp]
        lib.iile_traversal_limits.argtypes = [ctypes.POINTER(c_i32)]
        lib.iile_traversal_limits.restype = None
        lib.iile_test_patch_capacity.argtypes = [c_vp, c_u32]
        lib.iile_sample_table_budget.argtypes = []
        lib.iile_sample_table_budget.restype = c_u64
        lib.iile_test_sample_table_budget.argtypes = [c_u64]
        lib.iile_test_sample_table_budget.restype = None
        lib.iile_sample_table_bytes.argtypes = [c_vp]
        lib.iile_sample_table_bytes.restype = c_u64
        lib.iile_iispt_net_create.argtypes = [ctypes.POINTER(NetWeights), ctypes.POINTER(c_vp)]
        lib.iile_iispt_net_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(c_vp)]
        lib.iile_iispt_net_forward.argtypes = [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_i32]
        lib.iile_iispt_net_predict.argtypes = [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]
        lib.iile_iispt_film_add.argtypes = [c_vp, ctypes.POINTER(IisptTask), c_i32, c_vp, c_vp, c_i32, c_i32, c_vp]
        lib.iile_iispt_film_merge.argtypes = [c_vp, c_vp, ctypes.c_int64, c_vp, c_vp]
        lib.iile_device_upload.argtypes = [c_vp, c_vp, ctypes.c_uint64, c_vp]
        lib.iile_device_zero.argtypes = [c_vp, ctypes.c_uint64, c_vp]
        lib.iile_iispt_net_destroy.argtypes = [c_vp]
        lib.iile_iispt_net_destroy.restype = None
        _gpu = lib
    return _gpu


def dist_lib():
    """The RCCL film-merge library (needs librccl; loads without a GPU)."""
    global _dist
    if _dist is None:
        path = os.path.join(LIB_DIR, "libiile_dist.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (make -C pbrt-v3-iile_amd/csrc dist)")
        lib = ctypes.CDLL(path)
        lib.iile_dist_last_error.restype = ctypes.c_char_p
        lib.iile_dist_unique_id.argtypes = [c_vp]
        lib.iile_dist_create.argtypes = [c_vp, c_i32, c_i32, ctypes.POINTER(c_vp)]
        lib.iile_dist_create_deadline.argtypes = [c_vp, c_i32, c_i32, ctypes.c_double, ctypes.POINTER(c_vp)]
        lib.iile_dist_wait.argtypes = [c_vp, c_vp]
        lib.iile_dist_abort.argtypes = [c_vp]
        lib.iile_dist_abort.restype = None
        lib.iile_dist_destroy.argtypes = [c_vp]
        lib.iile_dist_destroy.restype = None
        lib.iile_dist_rank.argtypes = [c_vp]
        lib.iile_dist_size.argtypes = [c_vp]
        lib.iile_dist_film_reduce.argtypes = [c_vp, c_vp, ctypes.c_int64, c_i32, c_vp]
        lib.iile_dist_barrier.argtypes = [c_vp, c_vp]
        lib.iile_dist_sum_u64.argtypes = [c_vp, c_vp, c_i32]
        lib.iile_dist_max_f64.argtypes = [c_vp, c_vp, c_i32]
        lib.iile_dist_rendezvous_file.argtypes = [ctypes.c_char_p, c_i32, c_vp, c_i32]
        lib.iile_dist_rendezvous_file_token.argtypes = [ctypes.c_char_p, c_i32, ctypes.c_uint64, c_vp, c_i32]
        lib.iile_dist_rendezvous_done.argtypes = [c_vp, ctypes.c_char_p]
        lib.iile_dist_all_ok.argtypes = [c_vp, c_i32, ctypes.POINTER(c_i32)]
        _dist = lib
    return _dist


class Dist:
    """One rank of the film-merge communicator (include/iile_dist.h)."""

    @staticmethod
    def unique_id():
        buf = (ctypes.c_uint8 * DIST_ID_BYTES)()
        lib = dist_lib()
        if lib.iile_dist_unique_id(buf) != 0:
            raise RuntimeError(f"iile_dist_unique_id failed: {lib.iile_dist_last_error().decode()}")
        return bytes(buf)

    def __init__(self, unique_id, rank, nranks, timeout_s=None):
        """timeout_s: None -> iile_dist_create (RCCL's blocking set-up: a launcher owns the job's tear-down); a number ->
        iile_dist_create_deadline (non-blocking set-up polled against that deadline, which then bounds every wait on the communicator)."""
        lib = dist_lib()
        self._c = c_vp()
        buf = (ctypes.c_uint8 * DIST_ID_BYTES).from_buffer_copy(unique_id)
        if timeout_s is None:
            rc, what = lib.iile_dist_create(buf, int(rank), int(nranks), ctypes.byref(self._c)), "iile_dist_create"
        else:
            rc, what = lib.iile_dist_create_deadline(buf, int(rank), int(nranks), float(timeout_s), ctypes.byref(self._c)), "iile_dist_create_deadline"
        if rc != 0:
            err = RuntimeError(f"{what} failed ({rc}): {lib.iile_dist_last_error().decode()}")
            err.code = rc
            raise err
        self.rank, self.size = int(rank), int(nranks)
        lib.iile_dist_ranks_seen.restype = ctypes.c_int
        lib.iile_dist_ranks_seen.argtypes = [c_vp]
        self.ranks_seen = int(lib.iile_dist_ranks_seen(self._c))  # ncclCommCount

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {dist_lib().iile_dist_last_error().decode()}")

    def film_reduce(self, film_device_ptr, n_pixels, root=0, stream=None):
        self._check(dist_lib().iile_dist_film_reduce(self._c, c_vp(int(film_device_ptr)), int(n_pixels), int(root),
                                                     c_vp(stream) if stream else None), "iile_dist_film_reduce")

    def barrier(self, stream=None):
        self._check(dist_lib().iile_dist_barrier(self._c, c_vp(stream) if stream else None), "iile_dist_barrier")

    def wait(self, stream=None):
        """iile_dist_wait: what was queued on `stream` (the film merge) has finished, or the communicator's deadline has passed."""
        self._check(dist_lib().iile_dist_wait(self._c, c_vp(stream) if stream else None), "iile_dist_wait")

    def all_ok(self, ok):
        out = c_i32(0)
        self._check(dist_lib().iile_dist_all_ok(self._c, 1 if ok else 0, ctypes.byref(out)), "iile_dist_all_ok")
        return bool(out.value)

    def abort(self):
        if self._c:
            dist_lib().iile_dist_abort(self._c)
            self._c = c_vp()

    def sum_u64(self, values):
        a = np.ascontiguousarray(values, dtype=np.uint64).copy()
        self._check(dist_lib().iile_dist_sum_u64(self._c, a.ctypes.data, len(a)), "iile_dist_sum_u64")
        return a

    def max_f64(self, values):
        a = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._check(dist_lib().iile_dist_max_f64(self._c, a.ctypes.data, len(a)), "iile_dist_max_f64")
        return a

    def close(self):
        if self._c:
            dist_lib().iile_dist_destroy(self._c)
            self._c = c_vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class HostScene:
    """Scene loaded and flattened by libiile_host (ParseFile + MakeScene in the reference)."""

    def __init__(self, path=DEFAULT_SCENE, xres=0, yres=0, spp=0, max_depth=0, sampler=None, accel_split=None, bvh_on_device=False,
                 quick=False):
        """sampler: None keeps the scene file's; "sobol" is what the fork's path integrator renders with under
        IILE_PATH_SAMPLES_OVERRIDE (src/integrators/path.cpp:202-212). accel_split: BVHAccel's "splitmethod" in place of
        the file's. bvh_on_device: split method "hlbvh" is built by libiile_gpu's iile_bvh_build_hlbvh,
        plugged into the host loader as its bvh_build hook."""
        lib = host_lib()
        self._h = c_vp()
        hook = None
        if bvh_on_device is True:
            hook = ctypes.cast(gpu_lib().iile_bvh_build_hlbvh, c_vp)
        elif bvh_on_device:  # any other builder with iile_host_overrides::bvh_build's signature (a ctypes function object)
            hook = ctypes.cast(bvh_on_device, c_vp)
        ov = HostOverrides(int(xres), int(yres), int(spp), int(max_depth), SAMPLERS[sampler], SPLITS[accel_split], hook, int(bool(quick)))
        rc = lib.iile_host_load_pbrt(os.fsencode(path), ctypes.byref(ov), ctypes.byref(self._h))
        if rc != 0:
            raise RuntimeError(f"iile_host_load_pbrt({path}) failed: {lib.iile_host_last_error().decode()}")
        self.desc = lib.iile_host_scene_desc(self._h)
        self._film = lib.iile_host_scene_film(self._h)
        self.film = self._film.contents
        info = HostSceneInfo()
        lib.iile_host_scene_get_info(self._h, ctypes.byref(info))
        self.info = {n: getattr(info, n) for n, _ in HostSceneInfo._fields_}

    @property
    def film_shape(self):
        f = self.film
        return (f.crop_y1 - f.crop_y0, f.crop_x1 - f.crop_x0)

    @property
    def ao(self):
        """{"nsamples", "cossample"} of an Integrator "ambientocclusion" scene (iile_host_scene_ao); None for any other."""
        if self.info["integrator"] != INTEGRATOR_AO:
            return None
        p = AoParams()
        if host_lib().iile_host_scene_ao(self._h, ctypes.byref(p)) != 0:
            raise RuntimeError(f"iile_host_scene_ao failed: {host_lib().iile_host_last_error().decode()}")
        return {"nsamples": int(p.n_samples), "cossample": bool(p.cos_sample)}

    @property
    def camera_motion(self):
        """The CameraMotion of a scene whose camera moves (iile_host_scene_camera_motion); None for a static camera."""
        m = CameraMotion()
        rc = host_lib().iile_host_scene_camera_motion(self._h, ctypes.byref(m))
        if rc == 2:  # the camera does not move
            return None
        if rc != 0:
            raise RuntimeError(f"iile_host_scene_camera_motion failed: {host_lib().iile_host_last_error().decode()}")
        return m

    def bvh(self):
        """(flattened nodes as a BVH_NODE array, triangle vertices (n_prims, 9) in BVH order, prim_shape (n_prims,)): copies."""
        head = ctypes.cast(self.desc, ctypes.POINTER(SceneDescHead)).contents
        nodes = np.frombuffer(ctypes.string_at(head.nodes, head.n_nodes * BVH_NODE.itemsize), dtype=BVH_NODE).copy()
        tri_p = np.frombuffer(ctypes.string_at(head.tri_p, head.n_prims * 36), dtype=np.float32).reshape(-1, 9).copy()
        shape = np.frombuffer(ctypes.string_at(head.prim_shape, head.n_prims * 4), dtype=np.int32).copy()
        return nodes, tri_p, shape

    def film_to_rgb(self, film_xyzw):
        """Film::to_rgb_array on a (H, W, 4) {X,Y,Z,weight} film."""
        h, w = self.film_shape
        film = _f32(film_xyzw).reshape(h, w, 4)
        rgb = np.empty((h, w, 3), np.float32)
        rc = host_lib().iile_host_film_to_rgb(self._film, film.ctypes.data, rgb.ctypes.data)
        if rc != 0:
            raise RuntimeError(host_lib().iile_host_last_error().decode())
        return rgb

    def filter_table(self):
        """(Film::filterTable as a (16, 16) array [y][x], wide?)"""
        t = np.empty((16, 16), np.float32)
        wide = host_lib().iile_host_scene_filter_table(self._h, t.ctypes.data)
        return t, bool(wide)

    def light(self, index):
        """iile_light number `index` of the scene (a copy)."""
        lt = Light()
        if host_lib().iile_host_scene_light(self._h, int(index), ctypes.byref(lt)) != 0:
            raise RuntimeError(host_lib().iile_host_last_error().decode())
        return lt

    def scene_desc(self):
        """The scene's iile_scene_desc as a SceneDesc (a copy of the struct; its pointers are the scene's own tables)."""
        return SceneDesc.from_buffer_copy(ctypes.string_at(self.desc, ctypes.sizeof(SceneDesc)))

    @property
    def light_count(self):
        return int(self.scene_desc().n_lights)

    def light_power_all(self):
        """iile_scene_desc::light_power_all: Power().y() of every light (a copy); its first MAX_LIGHTS entries are also
        iile_integrator::light_power."""
        d = self.scene_desc()
        if not d.light_power_all:
            raise RuntimeError("the scene's descriptor has no light_power_all")
        return np.frombuffer(ctypes.string_at(d.light_power_all, d.n_lights * 4), dtype=np.float32).copy()

    def prim_light(self):
        """iile_scene_desc::prim_light, in BVH order (a copy): the light a primitive is, or -1."""
        head = ctypes.cast(self.desc, ctypes.POINTER(SceneDescHead)).contents
        return np.frombuffer(ctypes.string_at(head.prim_light, head.n_prims * 4), dtype=np.int32).copy()

    def camera(self):
        """(CAMERA_PERSPECTIVE or CAMERA_ENVIRONMENT, the scene's iile_camera as a copy)."""
        cam = Camera()
        kind = host_lib().iile_host_scene_camera(self._h, ctypes.byref(cam))
        if kind < 0:
            raise RuntimeError(host_lib().iile_host_last_error().decode())
        return int(kind), cam

    @property
    def quadric_count(self):
        """Disks and cylinders of the scene (not among info["n_triangles"])."""
        return int(host_lib().iile_host_scene_quadric_count(self._h))

    def quadric(self, index):
        """iile_quadric number `index` of the scene (a copy)."""
        q = Quadric()
        if host_lib().iile_host_scene_quadric(self._h, int(index), ctypes.byref(q)) != 0:
            raise RuntimeError(host_lib().iile_host_last_error().decode())
        return q

    def material(self, index):
        """iile_material number `index` of the scene (a copy; info["n_materials"] of them)."""
        m = Material()
        if host_lib().iile_host_scene_material(self._h, int(index), ctypes.byref(m)) != 0:
            raise RuntimeError(host_lib().iile_host_last_error().decode())
        return m

    def disney(self, index):
        """iile_disney number `index` of the scene (a copy): the scalar parameters of material `index`, a Disney material."""
        d = self.scene_desc()
        if not 0 <= int(index) < d.n_materials or self.material(index).type != MAT_DISNEY:
            raise RuntimeError("HostScene.disney: material %d is not a Disney material" % int(index))
        if not d.disney:
            raise RuntimeError("the scene's descriptor has no disney table")
        size = ctypes.sizeof(Disney)
        return Disney.from_buffer_copy(ctypes.string_at(d.disney + int(index) * size, size))

    def prim_flags(self):
        """iile_scene_desc::prim_flags, in BVH order (a copy)."""
        head = ctypes.cast(self.desc, ctypes.POINTER(SceneDescHead)).contents
        return np.frombuffer(ctypes.string_at(head.prim_flags, head.n_prims * 4), dtype=np.uint32).copy()

    def texture(self, index):
        """(iile_texture, [level arrays (h, w, 3), row 0 = bottom scanline]) of image texture `index`."""
        lib = host_lib()
        t = Texture()
        if lib.iile_host_scene_texture(self._h, index, ctypes.byref(t)) != 0:
            raise RuntimeError(lib.iile_host_last_error().decode())
        levels = []
        for l in range(t.n_levels):
            a = np.empty((t.level_h[l], t.level_w[l], 3), np.float32)
            lib.iile_host_scene_texture_level(self._h, index, l, a.ctypes.data)
            levels.append(a)
        return t, levels

    def procedural_texture(self, index):
        """The fields of texture `index` as a dict: kind, mapping and its data, inputs (-1: the constant), aamode, bilerp corners.
        An image entry has kind TEX_IMAGE and zeros elsewhere."""
        t, _ = self.texture(index)
        return {"kind": t.kind, "mapping": t.mapping, "n_levels": t.n_levels, "su": t.su, "sv": t.sv, "du": t.du, "dv": t.dv,
                "vs": list(t.vs), "vt": list(t.vt), "xf": np.array(list(t.xf), np.float32).reshape(3, 4),
                "child": list(t.child), "cval": np.array([list(r) for r in t.cval], np.float32), "aamode": t.aamode,
                "bilerp": np.array([list(r) for r in t.bilerp], np.float32)}

    @property
    def film_filename(self):
        """The scene file's Film "filename"."""
        return host_lib().iile_host_scene_film_filename(self._h).decode()

    def write_image(self, path, rgb):
        """Film::WriteImage: .exr (data window = the cropped pixel bounds) or .pfm by the extension."""
        rgb = _f32(rgb)
        if host_lib().iile_host_write_image(os.fsencode(path), self._film, rgb.ctypes.data) != 0:
            raise RuntimeError(host_lib().iile_host_last_error().decode())

    def write_pfm(self, path, rgb):
        rgb = _f32(rgb)
        rc = host_lib().iile_host_write_pfm(os.fsencode(path), rgb.ctypes.data, rgb.shape[1], rgb.shape[0])
        if rc != 0:
            raise RuntimeError(host_lib().iile_host_last_error().decode())

    def close(self):
        if self._h:
            host_lib().iile_host_scene_free(self._h)
            self._h = c_vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sample_table_budget():
    """iile_sample_table_budget: bytes the next GpuScene's table of Halton samples may take (a larger one is not built)."""
    return int(gpu_lib().iile_sample_table_budget())


def set_test_sample_table_budget(nbytes):
    """iile_test_sample_table_budget: the budget of the scenes this process creates next; 0: the constant again."""
    gpu_lib().iile_test_sample_table_budget(int(nbytes))


class GpuScene:
    """Device-resident scene + wavefront integrator (libiile_gpu)."""

    def __init__(self, host_scene):
        lib = gpu_lib()
        self.host = host_scene
        self._s = c_vp()
        rc = lib.iile_scene_create(host_scene.desc, ctypes.byref(self._s))
        if rc != 0:
            raise RuntimeError(f"iile_scene_create failed ({rc}): {lib.iile_last_error().decode()}")
        motion = getattr(host_scene, "camera_motion", None)
        if motion is not None:  # a moving camera travels beside the descriptor (iile_scene_set_camera_motion)
            rc = lib.iile_scene_set_camera_motion(self._s, ctypes.byref(motion))
            if rc != 0:
                msg = lib.iile_last_error().decode()
                lib.iile_scene_destroy(self._s)
                self._s = c_vp()
                raise RuntimeError(f"iile_scene_set_camera_motion failed ({rc}): {msg}")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {gpu_lib().iile_last_error().decode()}")

    def render(self, k_begin=0, k_end=0, tile_rank=0, tile_nranks=1, spp_per_pass=0, collect_stats=False,
               time_kernels=False, film_device_ptr=None, stream=None, want_stats=True):
        """SamplerIntegrator::Render. Returns (film, stats): film is a (H, W, 4) float32
        array, or None when `film_device_ptr` (a raw device pointer) receives it."""
        prm = RenderParams(int(k_begin), int(k_end), int(tile_rank), int(tile_nranks), int(spp_per_pass),
                           int(bool(collect_stats)), int(time_kernels), int(film_device_ptr is not None),
                           c_vp(stream) if stream else None)
        st = GpuStats()
        if film_device_ptr is not None:
            film, ptr = None, c_vp(int(film_device_ptr))
        else:
            h, w = self.host.film_shape
            film = np.zeros((h, w, 4), np.float32)
            ptr = film.ctypes.data
        rc = gpu_lib().iile_render(self._s, ctypes.byref(prm), ptr, ctypes.byref(st) if want_stats else None)
        self._check(rc, "iile_render")
        if not want_stats:
            return film, None
        d = st.as_dict()
        d["sample_table_bytes"] = int(gpu_lib().iile_sample_table_bytes(self._s))  # (not a field of iile_stats: its layout is pinned)
        return film, d

    def _ao_params(self, nsamples, cossample):
        ao = self.host.ao or {"nsamples": 64, "cossample": True}  # CreateAOIntegrator's defaults for a scene of another integrator
        return AoParams(int(ao["nsamples"] if nsamples is None else nsamples), int(bool(ao["cossample"] if cossample is None else cossample)))

    def render_ao(self, nsamples=None, cossample=None, k_begin=0, k_end=0, tile_rank=0, tile_nranks=1, spp_per_pass=0, collect_stats=False,
                  film_device_ptr=None, stream=None, want_stats=True):
        """iile_render_ao: SamplerIntegrator::Render with AOIntegrator::Li. nsamples / cossample: None takes the scene file's
        (HostScene.ao). Returns (film, stats) as render()."""
        ao = self._ao_params(nsamples, cossample)
        prm = RenderParams(int(k_begin), int(k_end), int(tile_rank), int(tile_nranks), int(spp_per_pass), int(bool(collect_stats)), 0,
                           int(film_device_ptr is not None), c_vp(stream) if stream else None)
        st = GpuStats()
        if film_device_ptr is not None:
            film, ptr = None, c_vp(int(film_device_ptr))
        else:
            h, w = self.host.film_shape
            film = np.zeros((h, w, 4), np.float32)
            ptr = film.ctypes.data
        rc = gpu_lib().iile_render_ao(self._s, ctypes.byref(ao), ctypes.byref(prm), ptr, ctypes.byref(st) if want_stats else None)
        self._check(rc, "iile_render_ao")
        return film, (st.as_dict() if want_stats else None)

    def ao_array_samples(self, nsamples, px, py, k, j):
        """iile_ao_array_samples: (n, 2) float32, entry j[i] of the 2D array of `nsamples` entries for pixel sample k[i] of pixel i."""
        px, py, k, j = _i32(px), _i32(py), _i32(k), _i32(j)
        out = np.empty((len(px), 2), np.float32)
        self._check(gpu_lib().iile_ao_array_samples(self._s, int(nsamples), len(px), px.ctypes.data, py.ctypes.data, k.ctypes.data, j.ctypes.data,
                                                    out.ctypes.data), "iile_ao_array_samples")
        return out

    def ao_li_samples(self, px, py, k, nsamples=None, cossample=None):
        """iile_ao_li_samples: (L (n,) float32 after the guards, nrays (n, 2) int32 {closest, occlusion}) of individual camera samples."""
        ao = self._ao_params(nsamples, cossample)
        px, py, k = _i32(px), _i32(py), _i32(k)
        n = len(px)
        L = np.empty(n, np.float32)
        nr = np.empty((n, 2), np.int32)
        self._check(gpu_lib().iile_ao_li_samples(self._s, ctypes.byref(ao), n, px.ctypes.data, py.ctypes.data, k.ctypes.data, L.ctypes.data,
                                                 nr.ctypes.data), "iile_ao_li_samples")
        return L, nr

    def render_status(self, stream=None):
        """iile_render_status: waits for `stream`; raises if the last asynchronous render's exact film finish overflowed."""
        self._check(gpu_lib().iile_render_status(self._s, c_vp(stream) if stream else None), "iile_render_status")

    def test_patch_capacity(self, capacity):
        self._check(gpu_lib().iile_test_patch_capacity(self._s, int(capacity)), "iile_test_patch_capacity")

    def trace_closest(self, o, d, tmax, instrumented=True):
        """instrumented=False runs the traversal of the uninstrumented render kernels."""
        o, d, tmax = _f32(o), _f32(d), _f32(tmax)
        n = len(tmax)
        prim = np.empty(n, np.int32)
        tb = np.empty((n, 4), np.float32)
        st = GpuStats()
        self._check(gpu_lib().iile_trace_closest(self._s, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data,
                                                 prim.ctypes.data, tb.ctypes.data,
                                                 ctypes.byref(st) if instrumented else None), "iile_trace_closest")
        return prim, tb, st.as_dict()

    def shape_hit_attributes(self, o, d, prim):
        """The SurfaceInteraction of each ray's closest hit on a sphere or a quadric (prim: from trace_closest): a dict of world-space
        (n, 3) arrays p, n, sn, dpdu, dpdv, dndu, dndv, wo and (n,) arrays u, v, flip (iile_shape_hit_attributes)."""
        o, d, prim = _f32(o).reshape(-1, 3), _f32(d).reshape(-1, 3), _i32(prim)
        out = np.empty((len(prim), 28), np.float32)
        f = gpu_lib().iile_shape_hit_attributes
        f.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]
        self._check(f(self._s, len(prim), o.ctypes.data, d.ctypes.data, prim.ctypes.data, out.ctypes.data), "iile_shape_hit_attributes")
        r = {k: out[:, 3 * i:3 * i + 3] for i, k in enumerate(("p", "n", "sn", "dpdu", "dpdv", "dndu", "dndv", "wo"))}
        r.update(u=out[:, 24], v=out[:, 25], flip=out[:, 26] != 0)
        return r

    def trace_any(self, o, d, tmax, instrumented=True):
        o, d, tmax = _f32(o), _f32(d), _f32(tmax)
        n = len(tmax)
        hit = np.empty(n, np.int32)
        st = GpuStats()
        self._check(gpu_lib().iile_trace_any(self._s, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data,
                                             hit.ctypes.data, ctypes.byref(st) if instrumented else None),
                    "iile_trace_any")
        return hit, st.as_dict()

    def halton_samples(self, px, py, k, dim0, ndims):
        px, py, k = _i32(px), _i32(py), _i32(k)
        n = len(px)
        out = np.empty((n, ndims), np.float32)
        idx = np.empty(n, np.uint32)
        self._check(gpu_lib().iile_halton_samples(self._s, n, px.ctypes.data, py.ctypes.data, k.ctypes.data, dim0,
                                                  ndims, out.ctypes.data, idx.ctypes.data), "iile_halton_samples")
        return out, idx

    def sample_table_records(self, px, py, k, bounce):
        """iile_sample_table_records: (n, 8) float32, the sample table's record of bounce[i] (dimensions 5 + 7 bounce ..) or, for
        bounce[i] < 0, its camera part {dim 0, 1, 3, 4, 0, 0, 0, 0}, of sample k[i] of pixel (px[i], py[i])."""
        px, py, k, bounce = _i32(px), _i32(py), _i32(k), _i32(bounce)
        out = np.empty((len(px), 8), np.float32)
        f = gpu_lib().iile_sample_table_records
        f.argtypes = [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]
        self._check(f(self._s, len(px), px.ctypes.data, py.ctypes.data, k.ctypes.data, bounce.ctypes.data, out.ctypes.data),
                    "iile_sample_table_records")
        return out

    def camera_rays(self, pfilm, plens=None):
        pfilm = _f32(pfilm)
        n = len(pfilm)
        o = np.empty((n, 3), np.float32)
        d = np.empty((n, 3), np.float32)
        pl = _f32(plens) if plens is not None else None
        self._check(gpu_lib().iile_camera_rays(self._s, n, pfilm.ctypes.data, pl.ctypes.data if pl is not None else None,
                                               o.ctypes.data, d.ctypes.data), "iile_camera_rays")
        return o, d

    def camera_rays_at(self, pfilm, time, plens=None):
        """iile_camera_rays_at: the camera rays at ray time `time` (read by a moving camera alone)."""
        pfilm = _f32(pfilm)
        n = len(pfilm)
        o = np.empty((n, 3), np.float32)
        d = np.empty((n, 3), np.float32)
        pl = _f32(plens) if plens is not None else None
        self._check(gpu_lib().iile_camera_rays_at(self._s, n, pfilm.ctypes.data, pl.ctypes.data if pl is not None else None,
                                                  c_f32(time), o.ctypes.data, d.ctypes.data), "iile_camera_rays_at")
        return o, d

    def set_camera_motion(self, motion):
        """iile_scene_set_camera_motion with a CameraMotion (or None: the null argument); returns the call's code."""
        return gpu_lib().iile_scene_set_camera_motion(self._s, ctypes.byref(motion) if motion is not None else None)

    def li_samples(self, px, py, k):
        px, py, k = _i32(px), _i32(py), _i32(k)
        n = len(px)
        L = np.empty((n, 3), np.float32)
        nr = np.empty((n, 2), np.int32)
        self._check(gpu_lib().iile_li_samples(self._s, n, px.ctypes.data, py.ctypes.data, k.ctypes.data, L.ctypes.data,
                                              nr.ctypes.data), "iile_li_samples")
        return L, nr

    def bsdf_eval(self, mat, wo, wi):
        wo, wi = _f32(wo), _f32(wi)
        out = np.empty((len(wo), 4), np.float32)
        self._check(gpu_lib().iile_bsdf_eval(self._s, len(wo), mat, wo.ctypes.data, wi.ctypes.data, out.ctypes.data),
                    "iile_bsdf_eval")
        return out

    def light_sample_li(self, light, p):
        """Light::Sample_Li of delta light `light` (point, spot, distant, projection, goniometric) at the (n, 3) points p, with no
        surface in between: (n, 7) {wi.xyz, Li.rgb, pdf}."""
        p = _f32(p).reshape(-1, 3)
        out = np.empty((len(p), 7), np.float32)
        self._check(gpu_lib().iile_light_sample_li(self._s, int(light), len(p), p.ctypes.data, out.ctypes.data), "iile_light_sample_li")
        return out

    def light_sample_at(self, light, ref_p, ref_n, u):
        """Light::Sample_Li of area or infinite light `light` at the (n, 3) reference points ref_p with normals ref_n (zero: no
        surface) and the (n, 2) samples u: (n, 13) {wi.xyz, Li.rgb, pdf, p_light.xyz, n_light.xyz}."""
        ref_p, ref_n, u = _f32(ref_p).reshape(-1, 3), _f32(ref_n).reshape(-1, 3), _f32(u).reshape(-1, 2)
        assert len(ref_p) == len(ref_n) == len(u)
        out = np.empty((len(ref_p), 13), np.float32)
        self._check(gpu_lib().iile_light_sample_at(self._s, int(light), len(ref_p), ref_p.ctypes.data, ref_n.ctypes.data, u.ctypes.data,
                                                   out.ctypes.data), "iile_light_sample_at")
        return out

    def light_pdf_at(self, light, ref_p, ref_n, wi):
        """Light::Pdf_Li of area or infinite light `light` for the (n, 3) reference points, normals and directions wi: (n,)."""
        ref_p, ref_n, wi = _f32(ref_p).reshape(-1, 3), _f32(ref_n).reshape(-1, 3), _f32(wi).reshape(-1, 3)
        assert len(ref_p) == len(ref_n) == len(wi)
        out = np.empty(len(ref_p), np.float32)
        self._check(gpu_lib().iile_light_pdf_at(self._s, int(light), len(ref_p), ref_p.ctypes.data, ref_n.ctypes.data, wi.ctypes.data,
                                                out.ctypes.data), "iile_light_pdf_at")
        return out

    def light_le(self, light, d):
        """InfiniteAreaLight::Le of infinite light `light` for the (n, 3) directions d of escaped rays: (n, 3)."""
        d = _f32(d).reshape(-1, 3)
        out = np.empty((len(d), 3), np.float32)
        self._check(gpu_lib().iile_light_le(self._s, int(light), len(d), d.ctypes.data, out.ctypes.data), "iile_light_le")
        return out

    def light_choose(self, p, u, stream=None):
        """The light UniformSampleOneLight samples at the (n, 3) points p with the 1D samples u, under the scene's light strategy:
        (light (n,) int32, pdf (n,) float32). One light: light 0 with pdf 1."""
        p, u = _f32(p).reshape(-1, 3), _f32(u).reshape(-1)
        light, pdf = np.empty(len(u), np.int32), np.empty(len(u), np.float32)
        self._check(gpu_lib().iile_light_choose(self._s, len(u), p.ctypes.data, u.ctypes.data, light.ctypes.data, pdf.ctypes.data,
                                                c_vp(stream) if stream else None), "iile_light_choose")
        return light, pdf

    def render_probes(self, pos, direction, hemi=None, device_out=None, stream=None):
        """IISPT probe pass: (n, 3) origins and directions -> intensity (n, hemi, hemi, 3), camera-space normals
        (n, hemi, hemi, 3), distances (n, hemi, hemi), [y][x] in raster order; plus the stats dict. hemi is the
        scene's probe film size (iile_scene_desc::probe.hemi_size through iile_host_scene_get_info); passing another
        value is an error. device_out: three device pointers (ints), each with room for n * hemi * hemi pixels, to
        write the images to instead (they then stay in HBM). stream: the HIP stream the pass is queued on (None: the null stream)."""
        pos, direction = _f32(pos).reshape(-1, 3), _f32(direction).reshape(-1, 3)
        n = len(pos)
        scene_hemi = int(self.host.info["probe_hemi_size"])
        if hemi is not None and int(hemi) != scene_hemi:
            raise ValueError(f"render_probes: the scene's probe films are {scene_hemi} x {scene_hemi}, not {hemi}")
        hemi = scene_hemi
        st = GpuStats()
        if device_out is not None:
            self._check(gpu_lib().iile_render_probes(self._s, n, pos.ctypes.data, direction.ctypes.data, device_out[0], device_out[1],
                                                     device_out[2], 1, ctypes.byref(st), stream), "iile_render_probes")
            return None, None, None, st.as_dict()
        inten = np.zeros((n, hemi, hemi, 3), np.float32)
        nrm = np.zeros((n, hemi, hemi, 3), np.float32)
        dist = np.zeros((n, hemi, hemi), np.float32)
        self._check(gpu_lib().iile_render_probes(self._s, n, pos.ctypes.data, direction.ctypes.data, inten.ctypes.data,
                                                 nrm.ctypes.data, dist.ctypes.data, 0, ctypes.byref(st), stream), "iile_render_probes")
        return inten, nrm, dist, st.as_dict()

    def render_probes_reference(self, pos, direction, spp, max_depth=3, first_sample=0, spp_total=0, stream=None):
        """The reference mode's probe pass (iile_render_probes_reference): samples [first_sample, first_sample + spp) of every probe pixel
        behind the probe's filter. Returns (intensity (n, hemi, hemi, 3), weight_sum (n, hemi, hemi), normals (n, hemi, hemi, 3), distance
        (n, hemi, hemi), stats); normals / distance are those of sample first_sample. Two ranges of one probe merge as
        sum(intensity_i * weight_i) / sum(weight_i). max_depth: 3 is IISPTdIntegrator's own, what the reference mode renders with.
        spp_total: the samples per pixel of the whole image the range belongs to (ray differentials); 0: spp."""
        pos, direction = _f32(pos).reshape(-1, 3), _f32(direction).reshape(-1, 3)
        n = len(pos)
        hemi = int(self.host.info["probe_hemi_size"])
        prm = ProbeRefParams(int(max_depth), int(first_sample), int(spp), int(spp_total), 0, c_vp(stream) if stream else None)
        inten = np.zeros((n, hemi, hemi, 3), np.float32)
        wsum = np.zeros((n, hemi, hemi), np.float32)
        nrm = np.zeros((n, hemi, hemi, 3), np.float32)
        dist = np.zeros((n, hemi, hemi), np.float32)
        st = GpuStats()
        self._check(gpu_lib().iile_render_probes_reference(self._s, n, pos.ctypes.data, direction.ctypes.data, ctypes.byref(prm), inten.ctypes.data,
                                                           wsum.ctypes.data, nrm.ctypes.data, dist.ctypes.data, ctypes.byref(st)),
                    "iile_render_probes_reference")
        return inten, wsum, nrm, dist, st.as_dict()

    def test_probe_ref_group(self, samples_per_group):
        """Force the samples per set of launches of render_probes_reference (0: sized from the workspace budget again)."""
        self._check(gpu_lib().iile_test_probe_ref_group(self._s, int(samples_per_group)), "iile_test_probe_ref_group")

    def reference_points(self, pfilm):
        """The reference mode's points (iile_reference_points) for (n, 2) film positions: (valid (n,) uint8, aux ray origins (n, 3),
        directions (n, 3)) on the camera rays' closest hits; no specular chain is followed."""
        pfilm = _f32(pfilm).reshape(-1, 2)
        n = len(pfilm)
        valid = np.zeros(n, np.uint8)
        pos = np.zeros((n, 3), np.float32)
        dr = np.zeros((n, 3), np.float32)
        self._check(gpu_lib().iile_reference_points(self._s, n, pfilm.ctypes.data, valid.ctypes.data, pos.ctypes.data, dr.ctypes.data),
                    "iile_reference_points")
        return valid, pos, dr

    def iispt_hemi_points(self, task):
        """The hemi points of an IISPT task: (valid (ny, nx) uint8, aux ray origins (ny, nx, 3), directions (ny, nx, 3))."""
        nx, ny = task.grid()
        valid = np.zeros((ny, nx), np.uint8)
        pos = np.zeros((ny, nx, 3), np.float32)
        dr = np.zeros((ny, nx, 3), np.float32)
        self._check(gpu_lib().iile_iispt_hemi_points(self._s, ctypes.byref(task), valid.ctypes.data, pos.ctypes.data, dr.ctypes.data),
                    "iile_iispt_hemi_points")
        return valid, pos, dr

    def iispt_gather(self, task, valid, pos, direction, nn_films=None, nn_device_ptr=None, out_device_ptr=None):
        """The runner's per-pixel loop over the predicted hemispheres nn_films (ny, nx, 32, 32, 3) -> (h, w, 4)
        {f_beta * L, weight}; nn_device_ptr / out_device_ptr: raw device pointers instead of host arrays."""
        valid, pos, direction = np.ascontiguousarray(valid, np.uint8), _f32(pos), _f32(direction)
        h, w = task.y1 - task.y0, task.x1 - task.x0
        out = None if out_device_ptr is not None else np.zeros((h, w, 4), np.float32)
        nn = _f32(nn_films) if nn_device_ptr is None else None
        self._check(gpu_lib().iile_iispt_gather(self._s, ctypes.byref(task), valid.ctypes.data, pos.ctypes.data, direction.ctypes.data,
                                                nn.ctypes.data if nn is not None else c_vp(int(nn_device_ptr)), int(nn is None),
                                                out.ctypes.data if out is not None else c_vp(int(out_device_ptr)), int(out is None)),
                    "iile_iispt_gather")
        return out

    def iispt_hemi_points_batch(self, tasks, stream=None):
        """iile_iispt_hemi_points_batch: the hemi points of several tasks from one set of launches — (valid (n,), origins (n, 3),
        directions (n, 3)) with the tasks' hemi points one task after the other, each in its own row-by-row order. stream: the HIP
        stream the call's copies and kernels are queued on (None: the null stream)."""
        arr = (IisptTask * len(tasks))(*tasks)
        n = sum(t.grid()[0] * t.grid()[1] for t in tasks)
        valid, pos, dr = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        self._check(gpu_lib().iile_iispt_hemi_points_batch(self._s, arr, len(tasks), valid.ctypes.data, pos.ctypes.data, dr.ctypes.data, stream),
                    "iile_iispt_hemi_points_batch")
        return valid, pos, dr

    def iispt_gather_batch(self, tasks, valid, pos, direction, nn_films=None, nn_device_ptr=None, out_device_ptr=None, stream=None):
        """iile_iispt_gather_batch: the per-pixel loop of several tasks from one set of launches. valid / pos / direction / nn_films
        (n_hemi, 32, 32, 3) as iispt_hemi_points_batch orders them; the result is (n_pixels, 4), the tasks' pixels one task after the
        other, row-major inside a task (None when written to out_device_ptr).
        With out_device_ptr the call returns once its kernels are queued on `stream` (None: the null stream, which is PyTorch's
        default stream); they read the scene's shared scratch block: keep a scene's IISPT calls on one stream."""
        arr = (IisptTask * len(tasks))(*tasks)
        valid, pos, direction = np.ascontiguousarray(valid, np.uint8), _f32(pos), _f32(direction)
        n_pix = sum((t.x1 - t.x0) * (t.y1 - t.y0) for t in tasks)
        out = None if out_device_ptr is not None else np.zeros((n_pix, 4), np.float32)
        nn = _f32(nn_films) if nn_device_ptr is None else None
        self._check(gpu_lib().iile_iispt_gather_batch(self._s, arr, len(tasks), valid.ctypes.data, pos.ctypes.data, direction.ctypes.data,
                                                      nn.ctypes.data if nn is not None else c_vp(int(nn_device_ptr)), int(nn is None),
                                                      out.ctypes.data if out is not None else c_vp(int(out_device_ptr)), int(out is None), stream),
                    "iile_iispt_gather_batch")
        return out

    def iispt_film_add(self, tasks, out_device_ptr, film_device_ptr, stream=None):
        """iile_iispt_film_add: IisptFilmMonitor::add_n_samples for every pixel of the (non-overlapping) tasks, whose gathered
        {f_beta * L, weight} lie at out_device_ptr, into the (h, w, 4) float64 monitor at film_device_ptr."""
        h, w = self.host.film_shape
        arr = (IisptTask * len(tasks))(*tasks)
        self._check(gpu_lib().iile_iispt_film_add(self._s, arr, len(tasks), c_vp(int(out_device_ptr)), c_vp(int(film_device_ptr)), w, h,
                                                  c_vp(stream) if stream else None), "iile_iispt_film_add")

    def render_direct(self, n_passes, first_pass=0, film_device_ptr=None, accumulate=False, stream=None):
        """The IISPT direct pass (iile_render_direct): the direct film monitor {sum r, g, b, weight} as (h, w, 4) float64, or
        accumulated into device memory at film_device_ptr (returns None)."""
        h, w = self.host.film_shape
        out = None if film_device_ptr is not None else np.zeros((h, w, 4), np.float64)
        prm = DirectParams(int(n_passes), int(first_pass), int(bool(accumulate)), int(out is None), c_vp(stream) if stream else None)
        f = gpu_lib().iile_render_direct
        f.argtypes = [c_vp, ctypes.POINTER(DirectParams), c_vp]
        self._check(f(self._s, ctypes.byref(prm), out.ctypes.data if out is not None else c_vp(int(film_device_ptr))), "iile_render_direct")
        return out

    def texture_eval(self, tex, uv, duv):
        """ImageTexture::Evaluate at (n, 2) uv with (n, 4) differentials {dudx, dvdx, dudy, dvdy} -> (n, 3) RGB."""
        uv, duv = _f32(uv), _f32(duv)
        out = np.empty((len(uv), 3), np.float32)
        self._check(gpu_lib().iile_texture_eval(self._s, tex, len(uv), uv.ctypes.data, duv.ctypes.data, out.ctypes.data),
                    "iile_texture_eval")
        return out

    def texture_eval_p(self, tex, uv, duv, p, dpdx, dpdy):
        """Texture::Evaluate of any texture at (n, 2) uv, (n, 4) {dudx, dvdx, dudy, dvdy}, (n, 3) p, dpdx, dpdy -> (n, 3)."""
        uv, duv = _f32(uv), _f32(duv)
        pdp = np.ascontiguousarray(np.concatenate([_f32(p), _f32(dpdx), _f32(dpdy)], axis=1), np.float32)
        out = np.empty((len(uv), 3), np.float32)
        self._check(gpu_lib().iile_texture_eval_p(self._s, tex, len(uv), uv.ctypes.data, duv.ctypes.data, pdp.ctypes.data,
                                                  out.ctypes.data), "iile_texture_eval_p")
        return out

    def bsdf_sample(self, mat, wo, u):
        wo, u = _f32(wo), _f32(u)
        out = np.empty((len(wo), 7), np.float32)
        self._check(gpu_lib().iile_bsdf_sample(self._s, len(wo), mat, wo.ctypes.data, u.ctypes.data, out.ctypes.data),
                    "iile_bsdf_sample")
        return out

    def bsdf_eval_ng(self, mat, ng, wo, wi):
        """bsdf_eval with the geometric normal ng (3,) in place of +z (the shading normal stays +z)."""
        ng, wo, wi = _f32(ng).reshape(3), _f32(wo), _f32(wi)
        out = np.empty((len(wo), 4), np.float32)
        self._check(gpu_lib().iile_bsdf_eval_ng(self._s, len(wo), mat, ng.ctypes.data, wo.ctypes.data, wi.ctypes.data, out.ctypes.data),
                    "iile_bsdf_eval_ng")
        return out

    def bsdf_sample_ng(self, mat, ng, wo, u):
        """bsdf_sample with the geometric normal ng (3,) in place of +z (the shading normal stays +z)."""
        ng, wo, u = _f32(ng).reshape(3), _f32(wo), _f32(u)
        out = np.empty((len(wo), 7), np.float32)
        self._check(gpu_lib().iile_bsdf_sample_ng(self._s, len(wo), mat, ng.ctypes.data, wo.ctypes.data, u.ctypes.data, out.ctypes.data),
                    "iile_bsdf_sample_ng")
        return out

    def bsdf_sample_specular(self, mat, wo, u):
        """bsdf_sample with the specular lobes allowed: {wi (3), f (3), pdf, sampled_specular, sampled_transmission} per (wo, u)."""
        wo, u = _f32(wo), _f32(u)
        out = np.empty((len(wo), 9), np.float32)
        self._check(gpu_lib().iile_bsdf_sample_specular(self._s, len(wo), mat, wo.ctypes.data, u.ctypes.data, out.ctypes.data),
                    "iile_bsdf_sample_specular")
        return out

    def close(self):
        if self._s:
            gpu_lib().iile_scene_destroy(self._s)
            self._s = c_vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the reference's state_dict names in forward order (ml/iispt_net.py:27-88): the 15 convolutions, the 5 BatchNorm2d
NET_CONVS = ("encoder0.0", "encoder0.2", "encoder1.1", "encoder1.4", "encoder2.1", "encoder2.4", "encoder3.1", "encoder3.4",
             "decoder0.0", "decoder0.3", "decoder1.0", "decoder1.3", "decoder2.0", "decoder2.2", "decoder2.4")
NET_BNS = ("encoder1.3", "encoder2.3", "encoder3.3", "decoder0.2", "decoder1.2")


def save_net_weights(state_dict, path, bn_eps=1e-5):
    """The flat file iile_iispt_net_load reads (and `iile_pbrt --iisptNet=`): "IILENET1", eps, the tensors of a state_dict of
    IISPTNet in iile_iispt_net_weights' order, float32."""
    def arr(name):
        t = state_dict[name]
        return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
    with open(path, "wb") as f:
        f.write(b"IILENET1")
        f.write(np.float32(bn_eps).tobytes())
        for k in NET_CONVS:
            f.write(arr(k + ".weight").tobytes())
            f.write(arr(k + ".bias").tobytes())
        for k in NET_BNS:
            for q in ("weight", "bias", "running_mean", "running_var"):
                f.write(arr(k + "." + q).tobytes())


def iispt_film_merge(direct_ptr, indirect_ptr, n_pixels, rgb_ptr, stream=None):
    """iile_iispt_film_merge: the two monitors normalised and added -> float RGB (device pointers)."""
    lib = gpu_lib()
    rc = lib.iile_iispt_film_merge(c_vp(int(direct_ptr)), c_vp(int(indirect_ptr)), int(n_pixels), c_vp(int(rgb_ptr)), c_vp(stream) if stream else None)
    if rc != 0:
        raise RuntimeError(f"iile_iispt_film_merge failed ({rc}): {lib.iile_last_error().decode()}")


class GpuNet:
    """The IISPT network on the device (iile_iispt_net_*): built from a state_dict with the reference's entry names
    (numpy arrays or torch tensors), run on device pointers."""

    def __init__(self, state_dict=None, bn_eps=1e-5, path=None):
        self._lib = gpu_lib()
        self._h = c_vp()
        if path is not None:   # an IILENET1 file (save_net_weights)
            rc = self._lib.iile_iispt_net_load(os.fsencode(path), ctypes.byref(self._h))
            if rc != 0:
                raise RuntimeError(f"iile_iispt_net_load failed ({rc}): {self._lib.iile_last_error().decode()}")
            return
        keep = []

        def arr(name):
            t = state_dict[name]
            a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
            keep.append(a)
            return a.ctypes.data

        w = NetWeights()
        for i, k in enumerate(NET_CONVS):
            w.conv_weight[i], w.conv_bias[i] = arr(k + ".weight"), arr(k + ".bias")
        for i, k in enumerate(NET_BNS):
            w.bn_weight[i], w.bn_bias[i] = arr(k + ".weight"), arr(k + ".bias")
            w.bn_mean[i], w.bn_var[i] = arr(k + ".running_mean"), arr(k + ".running_var")
        w.bn_eps = bn_eps
        rc = self._lib.iile_iispt_net_create(ctypes.byref(w), ctypes.byref(self._h))
        if rc != 0:
            raise RuntimeError(f"iile_iispt_net_create failed ({rc}): {self._lib.iile_last_error().decode()}")

    def forward(self, in_ptr, out_ptr, n, max_batch=0, stream=None, layer_out_ptr=None, layer=0):
        """(n, 7, 32, 32) -> (n, 3, 32, 32), device pointers; queued on `stream`."""
        rc = self._lib.iile_iispt_net_forward(self._h, in_ptr, out_ptr, int(n), int(max_batch), stream, layer_out_ptr, int(layer))
        if rc != 0:
            raise RuntimeError(f"iile_iispt_net_forward failed ({rc}): {self._lib.iile_last_error().decode()}")

    def predict(self, intensity_ptr, normals_ptr, distance_ptr, pred_ptr, n, film_rows=False, max_batch=0, stream=None, slot_ptr=None):
        """normalizeMapsDownstream -> network -> transformMapsUpstream over n rendered probes (device pointers; raster order in,
        (n, 32, 32, 3) out: ImageFilm row order when film_rows, else raster). slot_ptr: n int32 on the device — probe i's image goes to
        image slot[i] of pred_ptr."""
        rc = self._lib.iile_iispt_net_predict(self._h, intensity_ptr, normals_ptr, distance_ptr, pred_ptr, slot_ptr, int(n), int(bool(film_rows)),
                                              int(max_batch), stream)
        if rc != 0:
            raise RuntimeError(f"iile_iispt_net_predict failed ({rc}): {self._lib.iile_last_error().decode()}")

    def close(self):
        if self._h:
            self._lib.iile_iispt_net_destroy(self._h)
            self._h = c_vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bvh_build_hlbvh(bounds6, max_prims_in_node=4):
    """BVHAccel's HLBVH build + flattening on the device: (nodes as a BVH_NODE array, order (n,) int32, stats dict)."""
    b = _f32(bounds6).reshape(-1, 6)
    n = len(b)
    nodes = np.zeros(max(2 * n, 1), dtype=BVH_NODE)
    order = np.zeros(max(n, 1), dtype=np.int32)
    n_nodes = c_i32(0)
    st = BvhBuildStats()
    rc = gpu_lib().iile_bvh_build_hlbvh(n, b.ctypes.data, int(max_prims_in_node), nodes.ctypes.data, ctypes.byref(n_nodes), order.ctypes.data,
                                        ctypes.byref(st))
    if rc != 0:
        raise RuntimeError(f"iile_bvh_build_hlbvh failed ({rc}): {gpu_lib().iile_last_error().decode()}")
    return nodes[:n_nodes.value].copy(), order[:n].copy(), {k: getattr(st, k) for k, _ in BvhBuildStats._fields_}


def bvh_pack_probe(nodes):
    """The traversal records iile_scene_create packs on the device for a flattened tree: (wide (ni, 16) float32,
    wide4 (ni, 32) float32, nested bool)."""
    nodes = np.ascontiguousarray(nodes, dtype=BVH_NODE)
    ni = int((nodes["nprims"] == 0).sum())
    wide = np.zeros((max(ni, 1), 16), np.float32)
    wide4 = np.zeros((max(ni, 1), 32), np.float32)
    nested = c_i32(0)
    rc = gpu_lib().iile_bvh_pack_probe(len(nodes), nodes.ctypes.data, ni, wide.ctypes.data, wide4.ctypes.data, ctypes.byref(nested))
    if rc != 0:
        raise RuntimeError(f"iile_bvh_pack_probe failed ({rc}): {gpu_lib().iile_last_error().decode()}")
    return wide[:ni], wide4[:ni], bool(nested.value)


def traversal_limits():
    """iile_traversal_limits: what this build's traversal kernels were compiled with, as a dict: lds_stack (IILE_LDS_STACK),
    top_records (IILE_TOP_RECORDS), max_bvh_depth (the deepest tree iile_scene_create accepts). Needs no GPU."""
    out = (c_i32 * 3)()
    gpu_lib().iile_traversal_limits(out)
    return {"lds_stack": int(out[0]), "top_records": int(out[1]), "max_bvh_depth": int(out[2])}


def trig_probe(x):
    x = _f32(x)
    out = np.empty((len(x), 3), np.float32)
    rc = gpu_lib().iile_trig_probe(len(x), x.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"iile_trig_probe failed ({rc}): {gpu_lib().iile_last_error().decode()}")
    return out


def device_count():
    return int(gpu_lib().iile_device_count())
