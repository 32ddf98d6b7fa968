"""The projection and goniometric lights on the host (no GPU): what the loader makes of `LightSource "projection"` and
`LightSource "goniometric"` (type, position, intensity, frustum, the map's pyramid), their Power() under the power light
strategy, and what iile_scene_create refuses about them before it touches a device. Held to the float64 restatement of
imagelight_ref.py. The scene builders here are shared with test_gpu_image_lights.py."""
import ctypes

import numpy as np
import pytest

import imagelight_ref as IL
from quadric_ref import rotate, translate
from test_scene_refusals import ERR_ARG, Desc

LIGHT_POINT, LIGHT_PROJECTION, LIGHT_GONIOMETRIC = 1, 7, 8
TEX_IMAGE = 0
PLANE = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-50 -50 0  50 -50 0  50 50 0  -50 50 0] "float uv" [0 0 1 0 1 1 0 1]\n'
# (width, height) of the maps the tests write: not square, no symmetry
MAP_SIZES = {"wide": (48, 32), "tall": (24, 40), "gonio": (64, 32), "wide_small": (12, 8), "gonio_small": (16, 8)}
# the CTM every test light is declared under, as .pbrt text and as the matrix it makes (LightToWorld)
CTM_TEXT = "Translate 0.5 -0.25 2\nRotate 155 1 0 0\nRotate 25 0 0 1\nRotate 15 0 1 0\n"
CTM = translate(0.5, -0.25, 2) @ rotate(155, (1, 0, 0)) @ rotate(25, (0, 0, 1)) @ rotate(15, (0, 1, 0))
INTENSITY, SCALE = np.array([20.0, 15.0, 10.0]), np.array([0.5, 2.0, 1.5])


def write_pfm(path, rows):
    """rows[0] is the file's first row of data: the image's BOTTOM scanline."""
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


def write_map(tmp_path, which, seed=1):
    """Writes <which>.pfm, random texels in [0.2, 1]; returns the image as ReadImage returns it (row 0 = the top scanline)."""
    w, h = MAP_SIZES[which]
    rows = (0.2 + 0.8 * np.random.default_rng(seed + sorted(MAP_SIZES).index(which)).random((h, w, 3))).astype(np.float32)
    write_pfm(tmp_path / f"{which}.pfm", rows)
    return rows[::-1].astype(np.float64)


def light_text(kind, mapname=None, fov=None, ctm=CTM_TEXT, intensity=INTENSITY, scale=SCALE):
    params = f'"rgb I" [{intensity[0]} {intensity[1]} {intensity[2]}]'
    if scale is not None:
        params += f' "rgb scale" [{scale[0]} {scale[1]} {scale[2]}]'
    if fov is not None:
        params += f' "float fov" [{fov}]'
    if mapname is not None:
        params += f' "string mapname" "{mapname}"'
    return f'AttributeBegin\n{ctm}LightSource "{kind}" {params}\nAttributeEnd\n'


def scene_text(body, w=16, h=16, spp=1, depth=1, fov=30, eye="0 -3 2", look="0 0 0", up="0 0 1", integrator="path", strategy=None,
               center=False):
    strat = f' "string lightsamplestrategy" "{strategy}"' if strategy else ""
    return (f'LookAt {eye}  {look}  {up}\nCamera "perspective" "float fov" [{fov}]\n'
            f'Film "image" "integer xresolution" [{w}] "integer yresolution" [{h}] "string filename" "lights.exr"\nPixelFilter "box"\n'
            f'Sampler "halton" "integer pixelsamples" [{spp}] "bool samplepixelcenter" "{"true" if center else "false"}"\n'
            f'Integrator "{integrator}" "integer maxdepth" [{depth}]{strat}\nWorldBegin\n' + body + "WorldEnd\n")


def write_scene(tmp_path, body, name="lights.pbrt", **kw):
    p = tmp_path / name
    p.write_text(scene_text(body, **kw))
    return str(p)


def restated(kind, image=None, fov=45.0, ctm=CTM, intensity=INTENSITY, scale=SCALE):
    i = np.float32(intensity) * np.float32(1 if scale is None else scale)  # I * scale, in float as the loader multiplies
    if kind == "projection":
        return IL.ProjectionLight(ctm, i.astype(np.float64), fov, image)
    return IL.GoniometricLight(ctm, i.astype(np.float64), image)


def _only_light(binding, tmp_path, text, **kw):
    host = binding.HostScene(path=write_scene(tmp_path, text + 'Material "matte"\n' + PLANE, **kw))
    assert host.info["n_lights"] == 1
    return host, host.light(0)


def _check_common(lt, ref, type_code):
    assert lt.type == type_code and lt.sphere == -1
    assert np.allclose(list(lt.pos), ref.p_light, rtol=1e-6, atol=1e-6)
    assert np.array_equal(np.array(list(lt.lemit), np.float32), (np.float32(INTENSITY) * np.float32(SCALE)))
    assert np.allclose(np.array(list(lt.w2l)).reshape(3, 3), ref.w2l[:3, :3], atol=1e-6)


def _check_pyramid(host, lt, ref):
    t, levels = host.texture(lt.env_tex)
    h, w, _ = ref.image.shape
    assert t.kind == TEX_IMAGE and t.wrap == 0 and t.trilinear == 0
    assert levels[0].shape == (IL._round_up_pow2(h), IL._round_up_pow2(w), 3) and t.n_levels == len(ref.mip.levels)
    if levels[0].shape == ref.image.shape:  # powers of two: level 0 is the file's texels, not times I, not flipped
        assert np.array_equal(levels[0], ref.image.astype(np.float32))
    for got, want in zip(levels, ref.mip.levels):  # (else resampled as MIPMap's constructor does, then the box pyramid)
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("which, bounds", [("wide", (-1.5, -1, 1.5, 1)), ("tall", (-1, -1 / 0.6, 1, 1 / 0.6)), (None, (-1, -1, 1, 1))])
def test_projection_light_loads(binding, tmp_path, which, bounds):
    image = write_map(tmp_path, which) if which else None
    host, lt = _only_light(binding, tmp_path, light_text("projection", f"{which}.pfm" if which else None))
    ref = restated("projection", image)
    _check_common(lt, ref, LIGHT_PROJECTION)
    pr = lt.projection()
    assert pr["fov"] == 45 and pr["hither"] == np.float32(1e-3) and ctypes.sizeof(lt) == 152
    assert np.allclose(pr["screen_bounds"], bounds, rtol=1e-6) and np.allclose(ref.screen_bounds, bounds)
    h = np.float32(bounds[0]) ** 2 + np.float32(bounds[1]) ** 2 + 1
    assert np.isclose(lt.cos_total_width, 1 / h, rtol=1e-6) and np.isclose(ref.cos_total_width, 1 / h, rtol=1e-6)
    assert np.allclose([pr["m00"], pr["m11"]], [ref.proj[0, 0], ref.proj[1, 1]], rtol=1e-6)
    assert np.array_equal(ref.proj[[0, 1, 3]] != 0, [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]) and ref.proj[3, 2] == 1
    if which:
        _check_pyramid(host, lt, ref)
    else:
        assert lt.env_tex == -1


def test_projection_light_fov_parameter(binding, tmp_path):
    host, lt = _only_light(binding, tmp_path, light_text("projection", fov=70))
    pr = lt.projection()
    assert pr["fov"] == 70
    assert np.allclose([pr["m00"], pr["m11"]], [1 / np.tan(np.radians(35.0))] * 2, rtol=1e-6)


@pytest.mark.parametrize("which", ["gonio", "tall", None])
def test_goniometric_light_loads(binding, tmp_path, which):
    image = write_map(tmp_path, which) if which else None
    host, lt = _only_light(binding, tmp_path, light_text("goniometric", f"{which}.pfm" if which else None))
    ref = restated("goniometric", image)
    _check_common(lt, ref, LIGHT_GONIOMETRIC)
    if which:
        _check_pyramid(host, lt, ref)
    else:
        assert lt.env_tex == -1


@pytest.mark.parametrize("kind", ["projection", "goniometric"])
def test_unreadable_map_is_no_map(binding, tmp_path, kind, capfd):
    """ReadImage fails with a warning and returns no texels: the light is built without its map."""
    (tmp_path / "broken.pfm").write_bytes(b"not an image")
    for mapname in ("missing.pfm", "broken.pfm"):
        capfd.readouterr()
        host, lt = _only_light(binding, tmp_path, light_text(kind, mapname))
        assert lt.env_tex == -1 and lt.type in (LIGHT_PROJECTION, LIGHT_GONIOMETRIC)
        assert "Warning" in capfd.readouterr().err
    if kind == "projection":
        assert np.allclose(lt.projection()["screen_bounds"], (-1, -1, 1, 1))


def _three_lights(tmp_path, **kw):
    wide, gonio = write_map(tmp_path, "wide"), write_map(tmp_path, "gonio")
    body = ('LightSource "point" "rgb I" [3 3 3] "point from" [1 1 2]\n' + light_text("projection", "wide.pfm", fov=60) +
            light_text("goniometric", "gonio.pfm", ctm="Translate -1 0.5 1.5\nRotate 40 0 1 1\n") +
            light_text("projection", None) + light_text("goniometric", None) + 'Material "matte"\n' + PLANE)
    refs = [None, restated("projection", wide, fov=60.0),
            restated("goniometric", gonio, ctm=translate(-1, 0.5, 1.5) @ rotate(40, (0, 1, 1))), restated("projection"), restated("goniometric")]
    return write_scene(tmp_path, body, **kw), refs


def test_light_power_matches_restatement(binding, tmp_path):
    path, refs = _three_lights(tmp_path, strategy="power")
    host = binding.HostScene(path=path)
    desc = Desc(binding, host)
    power = list(desc.d.integrator.light_power)
    assert desc.d.integrator.light_strategy == 2 and desc.d.n_lights == 5
    assert np.isclose(power[0], IL.luminance(4 * np.pi * np.full(3, 3.0)), rtol=1e-5)
    for i in range(1, 5):
        assert np.isclose(power[i], IL.luminance(refs[i].power()), rtol=1e-5), (i, power[i], IL.luminance(refs[i].power()))
    assert all(p == 0 for p in power[5:])


@pytest.mark.parametrize("kind", [LIGHT_PROJECTION, LIGHT_GONIOMETRIC])
def test_bad_map_reference_is_refused(binding, tmp_path, kind):
    """env_tex of the new lights is -1 or an image texture of the scene; anything else is refused before a device is touched."""
    write_map(tmp_path, "wide"), write_map(tmp_path, "gonio")
    body = ('Texture "chk" "spectrum" "checkerboard" "float uscale" [4] "float vscale" [4]\n' +
            light_text("projection", "wide.pfm") + light_text("goniometric", "gonio.pfm") + 'Material "matte" "texture Kd" "chk"\n' + PLANE)
    host = binding.HostScene(path=write_scene(tmp_path, body))
    message = "projection / goniometric light: its map is not an image texture of the scene"
    n_tex = Desc(binding, host).d.n_textures
    procedural = next(i for i in range(n_tex) if host.texture(i)[0].kind != TEX_IMAGE)
    for bad in (n_tex, -2, procedural):
        desc = Desc(binding, host)
        lights = desc.table("lights", binding.Light, desc.d.n_lights)
        light = next(l for l in lights if l.type == kind)
        assert host.texture(light.env_tex)[0].kind == TEX_IMAGE
        light.env_tex = bad
        assert desc.create() == (ERR_ARG, message)
    desc = Desc(binding, host)  # a point light's env_tex is nobody's business
    lights = desc.table("lights", binding.Light, desc.d.n_lights)
    for l in lights:
        if l.type == kind:
            l.type = LIGHT_POINT
            l.env_tex = n_tex
    desc.d.sobol.enabled = 1  # (a Sobol' table of no dimensions: refused last, still without a device)
    assert desc.create()[1].startswith("iile_sobol: bad dimension count")


def test_unknown_light_name_is_still_refused(binding, tmp_path):
    path = write_scene(tmp_path, 'LightSource "laser" "rgb I" [1 1 1]\nMaterial "matte"\n' + PLANE)
    with pytest.raises(RuntimeError) as e:
        binding.HostScene(path=path)
    msg = str(e.value)
    assert 'LightSource "laser" is not supported' in msg
    for name in ("point", "spot", "distant", "infinite", "exinfinite", "projection", "goniometric"):
        assert name in msg
