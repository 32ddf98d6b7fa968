"""The translucent material through the loader and the descriptor check (CPU): CreateTranslucentMaterial
(materials/translucent.cpp:82-98) with its defaults, every parameter, textures on each of them, bump maps and named materials;
the parameter forms refused by name; type 8 accepted by iile_scene_create's refusal pass; the oracle refusing the material."""
import numpy as np
import pytest

import oracle_binding as ob
from quadric_ref import write_scene
from test_metal_substrate_scenes import QUAD, _material, _textures, _v, roughness_to_alpha
from test_scene_refusals import ERR_UNSUPPORTED, Desc, _host


def _f32(*v):
    return [float(np.float32(x)) for x in v]


def _procedural(tmp_path):
    return _textures(tmp_path) + ('Texture "ck" "spectrum" "checkerboard" "float uscale" [4] "float vscale" [4]\n'
                                  'Texture "fck" "float" "checkerboard" "float tex1" [0.1] "float tex2" [0.4]\n'
                                  'Texture "bl" "spectrum" "bilerp" "rgb v00" [0 0 0] "rgb v11" [1 1 1]\n')


def test_defaults(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "translucent"')
    assert m.type == binding.MAT_TRANSLUCENT == 8
    assert _v(m.kd) == _f32(.25, .25, .25) and _v(m.ks) == _f32(.25, .25, .25)
    assert _v(m.kr) == [0.5] * 3 and _v(m.kt) == [0.5] * 3  # reflect, transmit
    assert m.eta == 1.5 and m.remap_roughness == 1
    assert m.roughness == pytest.approx(0.1) and m.roughness_v == m.roughness
    assert m.alpha == roughness_to_alpha(0.1) and m.alpha_v == m.alpha
    assert (m.kd_tex, m.ks_tex, m.kr_tex, m.kt_tex, m.rough_tex, m.bump_tex, m.sigma_tex, m.opacity_tex) == (-1,) * 8
    assert m.rough_tex_v == -2  # alpha_v follows alpha
    assert _v(m.opacity) == [1, 1, 1] and _v(m.cond_eta) == [0, 0, 0] and _v(m.cond_k) == [0, 0, 0]
    assert m.sigma == 0 and m.on_a == 0 and m.on_b == 0


def test_every_parameter(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "translucent" "rgb Kd" [0.1 0.2 0.3] "color Ks" [0.4 0.5 0.6] '
                                     '"rgb reflect" [0.7 0.8 0.9] "rgb transmit" [0.3 0.2 0.1] "float roughness" [0.35]')
    assert _v(m.kd) == _f32(.1, .2, .3) and _v(m.ks) == _f32(.4, .5, .6)
    assert _v(m.kr) == _f32(.7, .8, .9) and _v(m.kt) == _f32(.3, .2, .1)
    assert m.alpha == roughness_to_alpha(0.35) and m.alpha_v == m.alpha and m.eta == 1.5


def test_parameters_pbrt_translucent_does_not_read_are_ignored(binding, tmp_path):
    """Kr, Kt, eta, uroughness and opacity are not translucent's (translucent.cpp:82-98): as with any unknown parameter, ignored."""
    m = _material(binding, tmp_path, 'Material "translucent" "rgb Kr" [0.1 0.1 0.1] "rgb Kt" [0.2 0.2 0.2] "float eta" [2] '
                                     '"float uroughness" [0.5] "rgb opacity" [0.5 0.5 0.5]')
    assert _v(m.kr) == [0.5] * 3 and _v(m.kt) == [0.5] * 3 and m.eta == 1.5
    assert m.alpha == roughness_to_alpha(0.1) and _v(m.opacity) == [1, 1, 1]


def test_without_remap(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "translucent" "bool remaproughness" "false" "float roughness" [0.2]')
    assert m.remap_roughness == 0 and m.alpha == pytest.approx(0.2) and m.alpha_v == m.alpha
    m = _material(binding, tmp_path, 'Material "translucent" "bool remaproughness" "false" "float roughness" [0]')
    assert m.alpha == 0.0 and m.alpha_v == 0.0


@pytest.mark.parametrize("tex", ["col", "ck", "bl"])
def test_spectrum_textures_on_each_parameter(binding, tmp_path, tex):
    """Image and procedural textures on Kd, Ks, reflect and transmit: each parameter its texture, its constant 1."""
    pre = _procedural(tmp_path)
    for param, field in (("Kd", "kd"), ("Ks", "ks"), ("reflect", "kr"), ("transmit", "kt")):
        m = _material(binding, tmp_path, f'Material "translucent" "texture {param}" "{tex}"', pre=pre)
        assert getattr(m, field + "_tex") >= 0, param
        assert _v(getattr(m, field)) == [1, 1, 1], param
        others = [f for f in ("kd", "ks", "kr", "kt") if f != field]
        assert all(getattr(m, f + "_tex") == -1 for f in others), param


def test_all_four_textured(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "translucent" "texture Kd" "col" "texture Ks" "ck" "texture reflect" "bl" '
                                     '"texture transmit" "col"', pre=_procedural(tmp_path))
    assert min(m.kd_tex, m.ks_tex, m.kr_tex, m.kt_tex) >= 0
    assert m.kd_tex == m.kt_tex and len({m.kd_tex, m.ks_tex, m.kr_tex}) == 3


def test_constant_textures_are_their_values(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "translucent" "texture reflect" "konst" "texture transmit" "konst"', pre=_textures(tmp_path))
    assert m.kr_tex == -1 and m.kt_tex == -1
    assert _v(m.kr) == _f32(.3, .4, .5) and _v(m.kt) == _f32(.3, .4, .5)


@pytest.mark.parametrize("tex", ["flt", "fck"])
def test_roughness_texture_and_bump(binding, tmp_path, tex):
    m = _material(binding, tmp_path, f'Material "translucent" "texture roughness" "{tex}" "texture bumpmap" "flt2"', pre=_procedural(tmp_path))
    assert m.rough_tex >= 0 and m.rough_tex_v == -2 and m.bump_tex >= 0 and m.bump_tex != m.rough_tex


def test_reflect_and_transmit_textures_stay_refused_elsewhere(binding, tmp_path):
    """Only translucent reads "reflect" / "transmit": on any other material an image there is refused as before."""
    with pytest.raises(RuntimeError, match='image texture "col" on parameter "reflect" is not supported'):
        _material(binding, tmp_path, 'Material "matte" "texture reflect" "col"', pre=_textures(tmp_path))


def test_named_materials(binding, tmp_path):
    body = (_textures(tmp_path) +
            'MakeNamedMaterial "leaf" "string type" "translucent" "rgb Kd" [0.1 0.6 0.1] "rgb transmit" [0.8 0.8 0.8]\n'
            'MakeNamedMaterial "paper" "string type" "translucent" "texture reflect" "col" "float roughness" [0.3]\n'
            'AttributeBegin\nNamedMaterial "leaf"\n' + QUAD + 'AttributeEnd\n'
            'AttributeBegin\nNamedMaterial "paper"\nTranslate 0 0 1\n' + QUAD + 'AttributeEnd\n')
    s = binding.HostScene(path=write_scene(tmp_path, body))
    mats = [s.material(i) for i in range(s.info["n_materials"])]
    tr = [m for m in mats if m.type == binding.MAT_TRANSLUCENT]
    assert len(tr) == 2
    leaf = next(m for m in tr if m.kr_tex == -1)
    paper = next(m for m in tr if m.kr_tex >= 0)
    assert _v(leaf.kd) == _f32(.1, .6, .1) and _v(leaf.kt) == _f32(.8, .8, .8) and _v(leaf.kr) == [0.5] * 3
    assert paper.alpha == roughness_to_alpha(0.3)


@pytest.mark.parametrize("param", ["Kd", "Ks", "reflect", "transmit"])
@pytest.mark.parametrize("value", ['"spectrum {p}" [300 0.2 800 0.6]', '"spectrum {p}" "leaf.spd"', '"blackbody {p}" [5500 1]'])
def test_refuses_spectral_values(binding, tmp_path, param, value):
    with pytest.raises(RuntimeError, match=f'Material "translucent": parameter "{param}" given as "(spectrum|blackbody)" is not supported'):
        _material(binding, tmp_path, 'Material "translucent" ' + value.format(p=param))


def test_named_translucent_refuses_spectrum(binding, tmp_path):
    body = 'MakeNamedMaterial "t" "string type" "translucent" "spectrum transmit" [300 1 800 2]\nNamedMaterial "t"\n' + QUAD
    with pytest.raises(RuntimeError, match='Material "translucent": parameter "transmit" given as "spectrum"'):
        binding.HostScene(path=write_scene(tmp_path, body))


@pytest.mark.parametrize("line, words", [
    ('Material "translucent" "texture Kd" "flt"', 'image texture "flt" on parameter "Kd"'),          # a float texture for a spectrum
    ('Material "translucent" "texture roughness" "col"', 'image texture "col" on parameter "roughness"'),  # and the other way round
    ('Material "translucent" "texture uroughness" "flt"', "roughness"),                             # translucent is isotropic
    ('Material "translucent" "texture bumpmap" "col"', "bumpmap"),
])
def test_refuses_mistyped_textures(binding, tmp_path, line, words):
    with pytest.raises(RuntimeError) as e:
        _material(binding, tmp_path, line, pre=_procedural(tmp_path))
    assert words in str(e.value), str(e.value)


def test_unsupported_material_message_names_translucent(binding, tmp_path):
    with pytest.raises(RuntimeError, match=r'Material "hair" is not supported \(.*substrate, translucent\)'):
        _material(binding, tmp_path, 'Material "hair"')


def test_descriptor_type_8_passes_the_refusal_pass(binding, tmp_path):
    """Type 8 gets past the material check to the next one (a Halton table made too wide here, so that no device is touched);
    7 and 9 are refused there."""
    desc = Desc(binding, _host(binding, tmp_path))
    desc.d.halton.n_dims = 1 << 20
    mats = desc.table("materials", binding.Material, desc.d.n_materials)
    mats[0].type = 8
    assert desc.create() == (ERR_UNSUPPORTED, "too many Halton dimensions")
    for t in (7, 9, -1):
        mats[0].type = t
        assert desc.create() == (ERR_UNSUPPORTED, "unsupported material type"), t


def test_oracle_refuses_translucent(binding, oracle, tmp_path):
    body = 'LightSource "point" "rgb I" [1 1 1] "point from" [0 0 3]\nMaterial "translucent"\n' + QUAD
    host = binding.HostScene(path=write_scene(tmp_path, body, w=8, h=8, spp=1, depth=2))
    for entry, call in {"render": lambda: oracle.render(host, threads=1), "li": lambda: oracle.li(host, [4], [4], [0]),
                        "iispt_direct": lambda: oracle.iispt_direct(host, 1, threads=1)}.items():
        with pytest.raises(ob.OracleUnsupported) as e:
            call()
        assert e.value.code == 3000 + binding.MAT_TRANSLUCENT, entry
