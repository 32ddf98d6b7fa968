"""Metal and substrate materials through the loader (CPU): CreateMetalMaterial (materials/metal.cpp:104-127) and
CreateSubstrateMaterial (materials/substrate.cpp:81-96) with their defaults, roughness fallbacks, textures, bump maps and named
materials, and the parameter forms the device path refuses by name."""
import json
import os

import numpy as np
import pytest

from quadric_ref import write_scene

HERE = os.path.dirname(os.path.abspath(__file__))
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0  1 -1 0  1 1 0  -1 1 0] "float uv" [0 0 1 0 1 1 0 1]\n'


def roughness_to_alpha(r):
    """TrowbridgeReitzDistribution::RoughnessToAlpha, microfacet.h:123-128, in float32 as the loader does it."""
    r = np.float32(max(np.float32(r), np.float32(1e-3)))
    x = np.float32(np.log(r))
    c = [np.float32(v) for v in (1.62142, 0.819955, 0.1734, 0.0171201, 0.000640711)]
    return float(c[0] + c[1] * x + c[2] * x * x + c[3] * x * x * x + c[4] * x * x * x * x)


def _write_pfm(path, rows):
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


def _textures(tmp_path):
    _write_pfm(tmp_path / "c.pfm", np.full((4, 4, 3), 0.5, np.float32))
    _write_pfm(tmp_path / "f.pfm", np.full((4, 4, 3), 0.25, np.float32))
    return ('Texture "col" "spectrum" "imagemap" "string filename" ["c.pfm"]\n'
            'Texture "flt" "float" "imagemap" "string filename" ["f.pfm"]\n'
            'Texture "flt2" "float" "imagemap" "string filename" ["f.pfm"]\n'
            'Texture "konst" "spectrum" "constant" "rgb value" [0.3 0.4 0.5]\n')


def _material(binding, tmp_path, line, pre=""):
    """The one material of a scene whose only shape uses `line`."""
    s = binding.HostScene(path=write_scene(tmp_path, pre + line + "\n" + QUAD))
    assert s.info["n_materials"] == 1
    return s.material(0)


def _v(a):
    return [float(x) for x in a]


def test_copper_default_equals_fixture(binding, tmp_path):
    """The loader's copper is RGBSpectrum::FromSampled of CopperN / CopperK (metal.cpp:108-116), as the fixture replays it."""
    fx = json.load(open(os.path.join(HERE, "golden", "copper_fixture.json")))
    m = _material(binding, tmp_path, 'Material "metal"')
    assert m.type == binding.MAT_METAL
    assert _v(m.cond_eta) == [float(np.float32(v)) for v in fx["eta"]]
    assert _v(m.cond_k) == [float(np.float32(v)) for v in fx["k"]]


def test_metal_defaults(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "metal"')
    assert m.remap_roughness == 1
    assert m.roughness == pytest.approx(0.01) and m.roughness_v == pytest.approx(0.01)
    assert m.alpha == roughness_to_alpha(0.01) and m.alpha_v == roughness_to_alpha(0.01)
    assert (m.rough_tex, m.rough_tex_v, m.bump_tex, m.kd_tex, m.ks_tex) == (-1, -1, -1, -1, -1)
    assert _v(m.kd) == [0, 0, 0]


def test_metal_eta_and_k(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "metal" "rgb eta" [0.2 0.4 1.5] "color k" [3.9 2.4 1.9]')
    assert _v(m.cond_eta) == [float(np.float32(v)) for v in (0.2, 0.4, 1.5)]
    assert _v(m.cond_k) == [float(np.float32(v)) for v in (3.9, 2.4, 1.9)]
    # a constant named texture is its value
    m = _material(binding, tmp_path, 'Material "metal" "texture eta" "konst"', pre=_textures(tmp_path))
    assert _v(m.cond_eta) == [float(np.float32(v)) for v in (0.3, 0.4, 0.5)]


@pytest.mark.parametrize("params, u, v", [
    ('"float roughness" [0.3]', 0.3, 0.3),
    ('"float uroughness" [0.2]', 0.2, 0.01),                       # vRough falls back to roughness (0.01), not to uroughness
    ('"float vroughness" [0.4]', 0.01, 0.4),
    ('"float roughness" [0.3] "float uroughness" [0.2]', 0.2, 0.3),  # each of u and v falls back on its own
    ('"float roughness" [0.3] "float vroughness" [0.4]', 0.3, 0.4),
    ('"float roughness" [0.3] "float uroughness" [0.1] "float vroughness" [0.5]', 0.1, 0.5),
])
def test_metal_roughness_fallbacks(binding, tmp_path, params, u, v):
    """uRough = uRoughness ? uRoughness : roughness; vRough = vRoughness ? vRoughness : roughness (metal.cpp:68-71)."""
    m = _material(binding, tmp_path, 'Material "metal" ' + params)
    assert (m.roughness, m.roughness_v) == (pytest.approx(u), pytest.approx(v))
    assert m.alpha == roughness_to_alpha(u) and m.alpha_v == roughness_to_alpha(v)
    assert m.rough_tex_v == -1  # the constant alpha_v, never uber's "same as u" code (-2)


def test_metal_without_remap(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "metal" "bool remaproughness" "false" "float uroughness" [0.2] "float vroughness" [0.05]')
    assert m.remap_roughness == 0
    assert m.alpha == pytest.approx(0.2) and m.alpha_v == pytest.approx(0.05)
    m = _material(binding, tmp_path, 'Material "metal" "bool remaproughness" "false" "float roughness" [0]')
    assert m.alpha == 0.0 and m.alpha_v == 0.0


def test_metal_roughness_textures_and_bump(binding, tmp_path):
    pre = _textures(tmp_path)
    m = _material(binding, tmp_path, 'Material "metal" "texture roughness" "flt" "texture bumpmap" "flt2"', pre=pre)
    assert m.rough_tex >= 0 and m.rough_tex_v == m.rough_tex and m.bump_tex >= 0 and m.bump_tex != m.rough_tex
    # u from its own image, v from "roughness" (a number)
    m = _material(binding, tmp_path, 'Material "metal" "float roughness" [0.3] "texture uroughness" "flt"', pre=pre)
    assert m.rough_tex >= 0 and m.rough_tex_v == -1 and m.alpha_v == roughness_to_alpha(0.3)
    # v from its own image, u from the "roughness" image
    m = _material(binding, tmp_path, 'Material "metal" "texture roughness" "flt" "texture vroughness" "flt2"', pre=pre)
    assert m.rough_tex >= 0 and m.rough_tex_v >= 0 and m.rough_tex != m.rough_tex_v


def test_substrate_defaults(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "substrate"')
    assert m.type == binding.MAT_SUBSTRATE
    assert _v(m.kd) == [0.5] * 3 and _v(m.ks) == [0.5] * 3
    assert m.remap_roughness == 1
    assert m.alpha == roughness_to_alpha(0.1) and m.alpha_v == roughness_to_alpha(0.1)
    assert (m.kd_tex, m.ks_tex, m.rough_tex, m.rough_tex_v, m.bump_tex) == (-1,) * 5
    assert _v(m.cond_eta) == [0, 0, 0] and _v(m.cond_k) == [0, 0, 0]


def test_substrate_parameters(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "substrate" "rgb Kd" [0.1 0.2 0.3] "rgb Ks" [0.04 0.05 0.06] '
                                     '"float uroughness" [0.02] "float vroughness" [0.3]')
    assert _v(m.kd) == [float(np.float32(v)) for v in (0.1, 0.2, 0.3)]
    assert _v(m.ks) == [float(np.float32(v)) for v in (0.04, 0.05, 0.06)]
    assert m.alpha == roughness_to_alpha(0.02) and m.alpha_v == roughness_to_alpha(0.3)
    m = _material(binding, tmp_path, 'Material "substrate" "bool remaproughness" "false" "float uroughness" [0.02]')
    assert m.alpha == pytest.approx(0.02) and m.alpha_v == pytest.approx(0.1)


def test_substrate_ignores_roughness(binding, tmp_path):
    """CreateSubstrateMaterial reads "uroughness" and "vroughness" only (substrate.cpp:88-91)."""
    m = _material(binding, tmp_path, 'Material "substrate" "float roughness" [0.5]')
    assert m.alpha == roughness_to_alpha(0.1) and m.alpha_v == roughness_to_alpha(0.1)
    m = _material(binding, tmp_path, 'Material "substrate" "texture roughness" "flt"', pre=_textures(tmp_path))
    assert m.rough_tex == -1 and m.rough_tex_v == -1


def test_substrate_textures_and_bump(binding, tmp_path):
    m = _material(binding, tmp_path, 'Material "substrate" "texture Kd" "col" "texture Ks" "col" "texture uroughness" "flt" '
                                     '"texture vroughness" "flt2" "texture bumpmap" "flt"', pre=_textures(tmp_path))
    assert m.kd_tex >= 0 and m.ks_tex == m.kd_tex
    assert m.rough_tex >= 0 and m.rough_tex_v >= 0 and m.bump_tex >= 0
    assert _v(m.kd) == [1, 1, 1] and _v(m.ks) == [1, 1, 1]  # the constant the image is multiplied with


def test_named_materials(binding, tmp_path):
    body = ('MakeNamedMaterial "cu" "string type" "metal" "float roughness" [0.2]\n'
            'MakeNamedMaterial "sub" "string type" "substrate" "rgb Kd" [0.7 0.1 0.1]\n'
            'AttributeBegin\nNamedMaterial "cu"\n' + QUAD + 'AttributeEnd\n'
            'AttributeBegin\nNamedMaterial "sub"\nTranslate 0 0 1\n' + QUAD + 'AttributeEnd\n')
    s = binding.HostScene(path=write_scene(tmp_path, body))
    mats = [s.material(i) for i in range(s.info["n_materials"])]
    types = sorted(m.type for m in mats)
    assert binding.MAT_METAL in types and binding.MAT_SUBSTRATE in types
    cu = next(m for m in mats if m.type == binding.MAT_METAL)
    sub = next(m for m in mats if m.type == binding.MAT_SUBSTRATE)
    assert cu.alpha == roughness_to_alpha(0.2) and cu.alpha_v == roughness_to_alpha(0.2)
    assert _v(sub.kd) == [float(np.float32(v)) for v in (0.7, 0.1, 0.1)]


def test_material_index_out_of_range(binding, tmp_path):
    s = binding.HostScene(path=write_scene(tmp_path, 'Material "metal"\n' + QUAD))
    with pytest.raises(RuntimeError, match="out of range"):
        s.material(1)


@pytest.mark.parametrize("param", ["eta", "k"])
@pytest.mark.parametrize("value", ['"spectrum {p}" [300 1.2 800 0.2]', '"spectrum {p}" "Cu.{p}.spd"', '"blackbody {p}" [5500 1]'])
def test_metal_refuses_spectral_values(binding, tmp_path, param, value):
    """A spectrum or blackbody value would otherwise be ignored and the metal come out as copper."""
    with pytest.raises(RuntimeError, match=f'Material "metal": parameter "{param}" given as "(spectrum|blackbody)" is not supported'):
        _material(binding, tmp_path, 'Material "metal" ' + value.format(p=param))


@pytest.mark.parametrize("param", ["eta", "k"])
def test_metal_refuses_image_textures(binding, tmp_path, param):
    with pytest.raises(RuntimeError, match=f'Material "metal": parameter "{param}" given as the image texture "col" is not supported'):
        _material(binding, tmp_path, f'Material "metal" "texture {param}" "col"', pre=_textures(tmp_path))


def test_named_metal_refuses_spectrum(binding, tmp_path):
    body = 'MakeNamedMaterial "cu" "string type" "metal" "spectrum k" [300 1 800 2]\nNamedMaterial "cu"\n' + QUAD
    with pytest.raises(RuntimeError, match='Material "metal": parameter "k" given as "spectrum"'):
        binding.HostScene(path=write_scene(tmp_path, body))
