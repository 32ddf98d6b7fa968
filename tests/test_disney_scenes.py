"""The Disney material through the loader and the descriptor check (CPU): CreateDisneyMaterial (materials/disney.cpp:590-624) with
its defaults, every parameter, constant textures folded into values, image and procedural textures on "color" and "roughness", bump
maps and named materials; the parameter forms refused by name; type 10 accepted by iile_scene_create's refusal pass, and refused
without its side table; 9, the value older callers knew as unused, stays refused."""
import ctypes

import numpy as np
import pytest

from quadric_ref import write_scene
from test_metal_substrate_scenes import QUAD, _textures, _v
from test_scene_refusals import ERR_ARG, ERR_UNSUPPORTED, SceneDesc, _host
from test_translucent_scenes import _f32, _procedural

SCALARS = ("metallic", "specular_tint", "anisotropic", "sheen", "sheen_tint", "clearcoat", "clearcoat_gloss", "spec_trans", "flatness",
           "diff_trans")
DEFAULTS = dict(metallic=0, specular_tint=0, anisotropic=0, sheen=0, sheen_tint=.5, clearcoat=0, clearcoat_gloss=1, spec_trans=0,
                flatness=0, diff_trans=1, thin=0)
# pbrt's parameter name of each scalar field
PBRT = dict(metallic="metallic", specular_tint="speculartint", anisotropic="anisotropic", sheen="sheen", sheen_tint="sheentint",
            clearcoat="clearcoat", clearcoat_gloss="clearcoatgloss", spec_trans="spectrans", flatness="flatness", diff_trans="difftrans")


def _disney(binding, tmp_path, line, pre=""):
    """(iile_material, iile_disney) of the one material of a scene whose only shape uses `line`."""
    s = binding.HostScene(path=write_scene(tmp_path, pre + line + "\n" + QUAD))
    assert s.info["n_materials"] == 1
    return s.material(0), s.disney(0)


def _scalars(dz):
    return {n: float(getattr(dz, n)) for n in SCALARS} | {"thin": int(dz.thin)}


def _untouched(m):
    """The fields Disney does not use hold what they hold for a material that never set them."""
    assert (m.ks_tex, m.kr_tex, m.kt_tex, m.sigma_tex, m.opacity_tex) == (-1,) * 5 and m.rough_tex_v == -2
    assert _v(m.ks) == [0, 0, 0] and _v(m.kr) == [0, 0, 0] and _v(m.kt) == [0, 0, 0]
    assert _v(m.opacity) == [1, 1, 1] and _v(m.cond_eta) == [0, 0, 0] and _v(m.cond_k) == [0, 0, 0]
    assert m.sigma == 0 and m.on_a == 0 and m.on_b == 0 and m.remap_roughness == 0


def test_defaults(binding, tmp_path):
    m, dz = _disney(binding, tmp_path, 'Material "disney"')
    assert m.type == binding.MAT_DISNEY == 10
    assert _v(m.kd) == [0.5] * 3 and m.eta == 1.5
    assert m.roughness == 0.5 and m.alpha == 0.5 and m.roughness_v == 0.5 and m.alpha_v == 0.5  # the raw roughness: never remapped
    assert (m.kd_tex, m.rough_tex, m.bump_tex) == (-1, -1, -1)
    _untouched(m)
    assert _scalars(dz) == {k: float(np.float32(v)) if k != "thin" else v for k, v in DEFAULTS.items()}


def test_every_parameter(binding, tmp_path):
    vals = dict(metallic=.1, specular_tint=.2, anisotropic=.3, sheen=.4, sheen_tint=.6, clearcoat=.7, clearcoat_gloss=.8, spec_trans=.9,
                flatness=.15, diff_trans=.25)
    line = ('Material "disney" "rgb color" [0.1 0.2 0.3] "float eta" [1.3] "float roughness" [0.35] "bool thin" "true" ' +
            " ".join(f'"float {PBRT[k]}" [{v}]' for k, v in vals.items()) + ' "rgb scatterdistance" [0 0 0]')
    m, dz = _disney(binding, tmp_path, line)
    assert _v(m.kd) == _f32(.1, .2, .3) and m.eta == float(np.float32(1.3))
    assert m.roughness == m.alpha == m.alpha_v == float(np.float32(.35)) and m.remap_roughness == 0
    _untouched(m)
    assert _scalars(dz) == {k: float(np.float32(v)) for k, v in vals.items()} | {"thin": 1}


def test_color_as_color_type(binding, tmp_path):
    m, _ = _disney(binding, tmp_path, 'Material "disney" "color color" [0.9 0.8 0.7]')
    assert _v(m.kd) == _f32(.9, .8, .7)


def test_parameters_pbrt_disney_does_not_read_are_ignored(binding, tmp_path):
    """Kd, Ks, Kr, index, remaproughness and opacity are not Disney's (disney.cpp:590-624): as with any unknown parameter, ignored."""
    m, dz = _disney(binding, tmp_path, 'Material "disney" "rgb Kd" [0.1 0.1 0.1] "rgb Ks" [0.2 0.2 0.2] "rgb Kr" [1 1 1] "float index" [2] '
                                       '"bool remaproughness" "true" "rgb opacity" [0.5 0.5 0.5] "float sigma" [20]')
    assert _v(m.kd) == [0.5] * 3 and m.eta == 1.5 and m.alpha == 0.5 and m.remap_roughness == 0
    _untouched(m)
    assert _scalars(dz)["metallic"] == 0


def test_constant_textures_are_their_values(binding, tmp_path):
    pre = (_textures(tmp_path) + 'Texture "k7" "float" "constant" "float value" [0.7]\n'
                                 'Texture "k2" "float" "scale" "float tex1" [0.5] "float tex2" [0.4]\n'
                                 'Texture "black" "spectrum" "constant" "rgb value" [0 0 0]\n')
    line = ('Material "disney" "texture color" "konst" "texture roughness" "k2" "texture eta" "k7" "texture scatterdistance" "black" ' +
            " ".join(f'"texture {PBRT[k]}" "k7"' for k in SCALARS))
    m, dz = _disney(binding, tmp_path, line, pre=pre)
    assert m.kd_tex == -1 and m.rough_tex == -1
    assert _v(m.kd) == _f32(.3, .4, .5) and m.eta == float(np.float32(.7))
    assert m.alpha == pytest.approx(0.2, rel=1e-6) and m.alpha_v == m.alpha
    assert all(float(getattr(dz, k)) == float(np.float32(.7)) for k in SCALARS)


@pytest.mark.parametrize("tex", ["col", "ck", "bl"])
def test_color_texture(binding, tmp_path, tex):
    """An image or a procedural texture on "color": the texture, its constant 1."""
    m, _ = _disney(binding, tmp_path, f'Material "disney" "texture color" "{tex}"', pre=_procedural(tmp_path))
    assert m.kd_tex >= 0 and _v(m.kd) == [1, 1, 1] and m.rough_tex == -1
    _untouched(m)


@pytest.mark.parametrize("tex", ["flt", "fck"])
def test_roughness_texture_and_bump(binding, tmp_path, tex):
    m, _ = _disney(binding, tmp_path, f'Material "disney" "texture roughness" "{tex}" "texture bumpmap" "flt2"', pre=_procedural(tmp_path))
    assert m.rough_tex >= 0 and m.rough_tex_v == -2 and m.remap_roughness == 0
    assert m.bump_tex >= 0 and m.bump_tex != m.rough_tex and m.kd_tex == -1


def test_named_materials(binding, tmp_path):
    body = (_textures(tmp_path) +
            'MakeNamedMaterial "car" "string type" "disney" "rgb color" [0.6 0.1 0.1] "float clearcoat" [1] "float metallic" [0.5]\n'
            'MakeNamedMaterial "leaf" "string type" "disney" "texture color" "col" "bool thin" "true" "float difftrans" [1.5]\n'
            'AttributeBegin\nNamedMaterial "car"\n' + QUAD + 'AttributeEnd\n'
            'AttributeBegin\nNamedMaterial "leaf"\nTranslate 0 0 1\n' + QUAD + 'AttributeEnd\n'
            'AttributeBegin\nMaterial "matte"\nTranslate 0 0 2\n' + QUAD + 'AttributeEnd\n')
    s = binding.HostScene(path=write_scene(tmp_path, body))
    mats = [s.material(i) for i in range(s.info["n_materials"])]
    dis = [i for i, m in enumerate(mats) if m.type == binding.MAT_DISNEY]
    assert len(dis) == 2 and len(mats) == 3
    car = next(i for i in dis if mats[i].kd_tex == -1)
    leaf = next(i for i in dis if mats[i].kd_tex >= 0)
    assert _v(mats[car].kd) == _f32(.6, .1, .1) and s.disney(car).clearcoat == 1 and s.disney(car).metallic == 0.5 and s.disney(car).thin == 0
    assert s.disney(leaf).thin == 1 and s.disney(leaf).diff_trans == 1.5
    matte = next(i for i, m in enumerate(mats) if m.type == binding.MAT_MATTE)
    with pytest.raises(RuntimeError, match="not a Disney material"):
        s.disney(matte)
    assert s.scene_desc().disney  # the side table is there, one entry per material


def test_scene_without_disney_has_no_side_table(binding, tmp_path):
    s = binding.HostScene(path=write_scene(tmp_path, 'Material "matte"\n' + QUAD))
    assert not s.scene_desc().disney


@pytest.mark.parametrize("param", ["metallic", "eta", "speculartint", "anisotropic", "sheen", "sheentint", "clearcoat", "clearcoatgloss",
                                   "spectrans", "flatness", "difftrans"])
@pytest.mark.parametrize("tex", ["flt", "fck"])
def test_refuses_textures_on_the_scalars(binding, tmp_path, param, tex):
    with pytest.raises(RuntimeError) as e:
        _disney(binding, tmp_path, f'Material "disney" "texture {param}" "{tex}"', pre=_procedural(tmp_path))
    assert (f'Material "disney": parameter "{param}" given as the texture "{tex}" is not supported (a number or a constant texture)'
            in str(e.value)), str(e.value)


@pytest.mark.parametrize("value", ['"rgb scatterdistance" [0.1 0 0]', '"color scatterdistance" [1 1 1]', '"texture scatterdistance" "konst"',
                                   '"texture scatterdistance" "col"', '"spectrum scatterdistance" [300 1 800 1]'])
def test_refuses_scatterdistance(binding, tmp_path, value):
    with pytest.raises(RuntimeError, match='Material "disney": a "scatterdistance" that is not black is not supported'):
        _disney(binding, tmp_path, 'Material "disney" ' + value, pre=_textures(tmp_path))


def test_thin_ignores_scatterdistance(binding, tmp_path):
    """A thin surface never evaluates "scatterdistance" (disney.cpp:506-513): ignored there, like any parameter that is not read."""
    m, dz = _disney(binding, tmp_path, 'Material "disney" "bool thin" "true" "rgb scatterdistance" [1 0.5 0.25]')
    assert m.type == binding.MAT_DISNEY and dz.thin == 1
    with pytest.raises(RuntimeError, match='a "scatterdistance" that is not black'):
        _disney(binding, tmp_path, 'Material "disney" "bool thin" "false" "rgb scatterdistance" [1 0.5 0.25]')


def test_named_disney_refuses_scatterdistance(binding, tmp_path):
    body = 'MakeNamedMaterial "skin" "string type" "disney" "rgb scatterdistance" [1 0.5 0.25]\nNamedMaterial "skin"\n' + QUAD
    with pytest.raises(RuntimeError, match='Material "disney": a "scatterdistance" that is not black'):
        binding.HostScene(path=write_scene(tmp_path, body))


@pytest.mark.parametrize("value", ['"spectrum color" [300 0.2 800 0.6]', '"blackbody color" [5500 1]'])
def test_refuses_spectral_color(binding, tmp_path, value):
    with pytest.raises(RuntimeError, match='Material "disney": parameter "color" given as "(spectrum|blackbody)" is not supported'):
        _disney(binding, tmp_path, 'Material "disney" ' + value)


@pytest.mark.parametrize("line, words", [
    ('Material "disney" "texture color" "flt"', 'image texture "flt" on parameter "color"'),          # a float texture for a spectrum
    ('Material "disney" "texture roughness" "col"', 'image texture "col" on parameter "roughness"'),  # and the other way round
    ('Material "disney" "texture bumpmap" "col"', "bumpmap"),
])
def test_refuses_mistyped_textures(binding, tmp_path, line, words):
    with pytest.raises(RuntimeError) as e:
        _disney(binding, tmp_path, line, pre=_procedural(tmp_path))
    assert words in str(e.value), str(e.value)


def test_color_texture_stays_refused_elsewhere(binding, tmp_path):
    """Only Disney reads "color": on any other material an image there is refused as before."""
    with pytest.raises(RuntimeError, match='image texture "col" on parameter "color" is not supported'):
        binding.HostScene(path=write_scene(tmp_path, _textures(tmp_path) + 'Material "matte" "texture color" "col"\n' + QUAD))


def test_unsupported_material_message_names_disney(binding, tmp_path):
    with pytest.raises(RuntimeError, match=r'Material "hair" is not supported \(.*disney.*substrate, translucent\)'):
        binding.HostScene(path=write_scene(tmp_path, 'Material "hair"\n' + QUAD))


# ---- iile_scene_create's refusal pass ---------------------------------------------------------------------------------------
class DisneyDesc(ctypes.Structure):
    """iile_scene_desc through its last member: test_scene_refusals' view, then light_power_all and disney."""
    _fields_ = SceneDesc._fields_ + [("light_power_all", ctypes.c_void_p), ("disney", ctypes.c_void_p)]


def _create(binding, d):
    lib = binding.gpu_lib()
    out = ctypes.c_void_p()
    rc = lib.iile_scene_create(ctypes.addressof(d), ctypes.byref(out))
    if rc == 0:
        lib.iile_scene_destroy(out)
    return rc, lib.iile_last_error().decode()


def _desc_with_disney_type(binding, tmp_path):
    host = _host(binding, tmp_path)
    d = DisneyDesc.from_buffer_copy(ctypes.string_at(host.desc, ctypes.sizeof(DisneyDesc)))
    assert ctypes.sizeof(DisneyDesc) == ctypes.sizeof(binding.SceneDesc) and not d.disney
    mats = (binding.Material * d.n_materials)()
    ctypes.memmove(mats, d.materials, ctypes.sizeof(mats))
    mats[0].type = binding.MAT_DISNEY
    d.materials = ctypes.addressof(mats)
    d.halton.n_dims = 1 << 20  # the check behind the materials': no device is touched
    return host, d, mats


def test_descriptor_type_10_passes_the_refusal_pass(binding, tmp_path):
    """Type 10 with its side table gets past the material checks to the next one (a Halton table made too wide here)."""
    host, d, mats = _desc_with_disney_type(binding, tmp_path)
    table = (binding.Disney * d.n_materials)()
    d.disney = ctypes.addressof(table)
    assert _create(binding, d) == (ERR_UNSUPPORTED, "too many Halton dimensions")
    for t in (7, 9, 11, -1):
        mats[0].type = t
        assert _create(binding, d) == (ERR_UNSUPPORTED, "unsupported material type"), t


def test_descriptor_type_10_without_its_table(binding, tmp_path):
    host, d, mats = _desc_with_disney_type(binding, tmp_path)
    rc, msg = _create(binding, d)
    assert rc == ERR_ARG and msg.startswith("disney is null")
    # an unsupported type anywhere among the materials is still reported first
    mats2 = (binding.Material * (d.n_materials + 1))()
    ctypes.memmove(mats2, mats, ctypes.sizeof(mats))
    mats2[d.n_materials] = mats[0]
    mats2[d.n_materials].type = 7
    d.materials, d.n_materials = ctypes.addressof(mats2), d.n_materials + 1
    assert _create(binding, d) == (ERR_UNSUPPORTED, "unsupported material type")


def test_shorter_descriptor_without_disney_still_passes(binding, tmp_path):
    """A descriptor that ends before `disney` (test_scene_refusals' view) is read as before while no material is Disney's."""
    host = _host(binding, tmp_path)
    d = SceneDesc.from_buffer_copy(ctypes.string_at(host.desc, ctypes.sizeof(SceneDesc)))
    d.halton.n_dims = 1 << 20
    assert _create(binding, d) == (ERR_UNSUPPORTED, "too many Halton dimensions")
