"""Integrator "ambientocclusion" in the loader and the host library (no GPU): CreateAOIntegrator's parameters (pbrt-v3
src/integrators/ao.cpp:105-126), how such a scene is finalised, and the new entry points of the two libraries."""
import ctypes

import pytest

import ao_ref

BODY = ao_ref.truth_body()
LIGHT = 'LightSource "point" "point from" [0 3 0]\n'


def _host(binding, tmp_path, name="s.pbrt", body=BODY, load=None, **kw):
    return binding.HostScene(path=ao_ref.write_scene(tmp_path, body, name=name, **kw), **(load or {}))


def test_defaults(binding, tmp_path):
    host = _host(binding, tmp_path)
    assert host.ao == {"nsamples": 64, "cossample": True}
    assert host.info["integrator"] == binding.INTEGRATOR_AO == 2 and host.info["max_depth"] == 0
    assert host.scene_desc().integrator.max_depth == 0


def test_parameters_given(binding, tmp_path):
    host = _host(binding, tmp_path, nsamples=7, cossample=False)
    assert host.ao == {"nsamples": 7, "cossample": False}
    # a "maxdepth" on the line (CreateAOIntegrator does not read it) and the max_depth override change nothing: Li follows no path
    host = _host(binding, tmp_path, name="d.pbrt", nsamples=3, params=' "integer maxdepth" [9]', load=dict(max_depth=4))
    assert host.ao["nsamples"] == 3 and host.info["max_depth"] == 0


def test_quick_override(binding, tmp_path):
    host = _host(binding, tmp_path, w=64, h=32, spp=8, nsamples=16, load=dict(quick=True))
    assert host.ao == {"nsamples": 1, "cossample": True}   # `if (PbrtOptions.quickRender) nSamples = 1;`
    assert (host.info["xres"], host.info["yres"], host.info["spp"]) == (16, 8, 1)


def test_pixelbounds(binding, tmp_path):
    host = _host(binding, tmp_path, params=' "integer pixelbounds" [3 9 -2 5]')
    assert list(host.scene_desc().integrator.pixel_bounds) == [3, 0, 9, 5]   # clipped to the sample bounds, as the path integrator's
    host = _host(binding, tmp_path, name="n.pbrt")
    assert list(host.scene_desc().integrator.pixel_bounds) == [0, 0, 16, 16]


def test_nsamples_below_one_is_refused(binding, tmp_path):
    for n in (0, -3):
        with pytest.raises(RuntimeError, match="nsamples"):
            _host(binding, tmp_path, name=f"bad{n}.pbrt", nsamples=n)


def test_halton_tables_cover_the_array(binding, tmp_path):
    d = _host(binding, tmp_path).scene_desc()
    assert d.halton.n_dims >= 7   # the array takes dimensions 5 and 6
    d = _host(binding, tmp_path, name="sobol.pbrt", sampler="sobol").scene_desc()
    assert d.sobol.enabled and d.sobol.n_dims >= 7


def test_lights_do_not_matter(binding, tmp_path):
    assert _host(binding, tmp_path).info["n_lights"] == 0   # a scene with no light loads
    many = _host(binding, tmp_path, name="lit.pbrt", body=LIGHT + LIGHT + BODY)
    assert many.info["n_lights"] == 2 and many.ao["nsamples"] == 64
    assert many.scene_desc().integrator.light_strategy == 1   # uniform: no spatial light distribution is built for an AO scene


def test_other_scenes_have_no_ao(binding, tmp_path):
    host = _host(binding, tmp_path, integrator="path")
    assert host.ao is None and host.info["integrator"] == 0 and host.info["max_depth"] == 5
    p = binding.AoParams()
    assert binding.host_lib().iile_host_scene_ao(host._h, ctypes.byref(p)) != 0
    assert b"ambientocclusion" in binding.host_lib().iile_host_last_error()
    assert binding.host_lib().iile_host_scene_ao(None, ctypes.byref(p)) != 0


@pytest.mark.parametrize("name", ["whitted", "directlighting", "volpath", "bdpt", "mlt", "sppm"])
def test_other_integrators_stay_refused(binding, tmp_path, name):
    with pytest.raises(RuntimeError, match='only Integrator "path" and "iispt"'):
        _host(binding, tmp_path, integrator=name)


def test_symbols_and_struct(binding):
    assert ctypes.sizeof(binding.AoParams) == 8 and ctypes.sizeof(binding.HostSceneInfo) == 15 * 4
    assert binding.host_lib().iile_host_scene_ao is not None
    for name in ("iile_render_ao", "iile_ao_array_samples", "iile_ao_li_samples"):
        assert getattr(binding.gpu_lib(), name) is not None


def test_arguments_are_checked_before_the_device(binding):
    lib = binding.gpu_lib()
    scene = ctypes.create_string_buffer(64)   # never looked into: every check below comes first
    film = (ctypes.c_float * 4)()
    prm = binding.RenderParams()
    one = (ctypes.c_int32 * 1)(0)
    ok, zero = binding.AoParams(4, 1), binding.AoParams(0, 1)
    assert lib.iile_render_ao(None, ctypes.byref(ok), ctypes.byref(prm), film, None) == 1
    assert lib.iile_render_ao(scene, None, ctypes.byref(prm), film, None) == 1 and lib.iile_render_ao(scene, ctypes.byref(ok), None, film, None) == 1
    assert lib.iile_render_ao(scene, ctypes.byref(ok), ctypes.byref(prm), None, None) == 1
    assert lib.iile_render_ao(scene, ctypes.byref(zero), ctypes.byref(prm), film, None) == 1 and b"n_samples < 1" in lib.iile_last_error()
    assert lib.iile_ao_array_samples(scene, 0, 1, one, one, one, one, film) == 1
    assert lib.iile_ao_array_samples(scene, 4, 1, one, one, one, (ctypes.c_int32 * 1)(4), film) == 1   # j outside [0, n)
    assert lib.iile_ao_array_samples(scene, 4, 1, one, one, one, one, None) == 1
    assert lib.iile_ao_li_samples(scene, ctypes.byref(zero), 1, one, one, one, film, None) == 1
    assert lib.iile_ao_li_samples(scene, ctypes.byref(ok), 1, one, one, (ctypes.c_int32 * 1)(-1), film, None) == 1


def test_no_cpu_path(binding):
    if binding.device_count() > 0:
        pytest.skip("a GPU is visible")
    lib = binding.gpu_lib()
    scene = ctypes.create_string_buffer(64)
    film = (ctypes.c_float * 4)()
    prm = binding.RenderParams()
    one = (ctypes.c_int32 * 1)(0)
    ok = binding.AoParams(4, 1)
    for rc in (lib.iile_render_ao(scene, ctypes.byref(ok), ctypes.byref(prm), film, None),
               lib.iile_ao_array_samples(scene, 4, 1, one, one, one, one, film),
               lib.iile_ao_li_samples(scene, ctypes.byref(ok), 1, one, one, one, film, None)):
        assert rc == 2 and b"no HIP device" in lib.iile_last_error()   # IILE_ERR_NO_DEVICE
