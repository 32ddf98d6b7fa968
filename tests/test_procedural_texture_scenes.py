"""Procedural textures and texture mappings through the loader (CPU): checkerboard (dimension 2 and 3), uv, bilerp, scale and mix
over non-constant inputs, under the uv, spherical, cylindrical and planar mappings, with the parameters and defaults of
src/textures/*.cpp; the folding of constant subtrees; and what stays refused, by name."""
import numpy as np
import pytest

from quadric_ref import write_scene

QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0  1 -1 0  1 1 0  -1 1 0] "float uv" [0 0 1 0 1 1 0 1]\n'


def _write_pfm(path, rows):
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


def _images(tmp_path):
    _write_pfm(tmp_path / "a.pfm", np.full((4, 4, 3), 0.5, np.float32))
    _write_pfm(tmp_path / "b.pfm", np.full((4, 4, 3), 0.25, np.float32))
    return ('Texture "ia" "spectrum" "imagemap" "string filename" ["a.pfm"]\n'
            'Texture "ib" "spectrum" "imagemap" "string filename" ["b.pfm"]\n'
            'Texture "fa" "float" "imagemap" "string filename" ["a.pfm"]\n')


def _scene(binding, tmp_path, body):
    return binding.HostScene(path=write_scene(tmp_path, body + QUAD))


def _textures(host):
    out = []
    while True:
        try:
            out.append(host.procedural_texture(len(out)))
        except RuntimeError:
            return out


def _kd(binding, tmp_path, tex, pre=""):
    """The procedural texture the one material's Kd refers to, with all textures of the scene."""
    host = _scene(binding, tmp_path, pre + tex + '\nMaterial "matte" "texture Kd" "t"\n')
    m = host.material(0)
    assert m.kd_tex >= 0 and list(m.kd) == [1, 1, 1]
    texs = _textures(host)
    return texs[m.kd_tex], texs


def _refused(binding, tmp_path, body, *words):
    with pytest.raises(RuntimeError) as e:
        _scene(binding, tmp_path, body)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_checkerboard_2d_defaults(binding, tmp_path):
    t, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "checkerboard"')
    assert t["kind"] == binding.TEX_CHECKER2D and t["n_levels"] == 0
    assert t["mapping"] == binding.MAP_UV and (t["su"], t["sv"], t["du"], t["dv"]) == (1, 1, 0, 0)
    assert t["aamode"] == binding.AA_CLOSEDFORM
    assert t["child"] == [-1, -1, -1]
    assert t["cval"][0].tolist() == [1, 1, 1] and t["cval"][1].tolist() == [0, 0, 0]  # tex1 1, tex2 0 (checkerboard.cpp:49-50)


def test_checkerboard_2d_parameters(binding, tmp_path):
    t, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "checkerboard" "string aamode" "none" "float uscale" [4] "float vscale" [8] '
                                  '"float udelta" [0.5] "float vdelta" [0.25] "rgb tex1" [0.1 0.2 0.3] "rgb tex2" [0.7 0.8 0.9]')
    assert t["aamode"] == binding.AA_NONE
    assert (t["su"], t["sv"], t["du"], t["dv"]) == (4, 8, 0.5, 0.25)
    assert np.array_equal(t["cval"][:2], np.float32([[0.1, 0.2, 0.3], [0.7, 0.8, 0.9]]))


def test_checkerboard_unknown_aamode_is_closed_form(binding, tmp_path, capfd):
    t, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "checkerboard" "string aamode" "supersample"')
    assert t["aamode"] == binding.AA_CLOSEDFORM
    assert "not understood by Checkerboard2DTexture" in capfd.readouterr().err


def test_checkerboard_bad_dimension_refused(binding, tmp_path):
    _refused(binding, tmp_path, 'Texture "t" "spectrum" "checkerboard" "integer dimension" [4]\n', "4 dimensional checkerboard")


def test_checkerboard_3d_uses_tex2world_itself(binding, tmp_path):
    """CreateCheckerboard*Texture hands tex2world to IdentityMapping3D as its WorldToTexture (checkerboard.cpp:91, 149)."""
    t, _ = _kd(binding, tmp_path, 'TransformBegin\nTranslate 1 2 3\nScale 2 2 2\n'
                                  'Texture "t" "spectrum" "checkerboard" "integer dimension" [3]\nTransformEnd\n')
    assert t["kind"] == binding.TEX_CHECKER3D
    assert np.array_equal(t["xf"], np.float32([[2, 0, 0, 1], [0, 2, 0, 2], [0, 0, 2, 3]]))


@pytest.mark.parametrize("mapping", ["spherical", "cylindrical"])
def test_spherical_cylindrical_use_the_inverse(binding, tmp_path, mapping):
    t, _ = _kd(binding, tmp_path, f'TransformBegin\nTranslate 1 2 3\nScale 2 2 2\n'
                                  f'Texture "t" "spectrum" "checkerboard" "string mapping" "{mapping}"\nTransformEnd\n')
    assert t["mapping"] == (binding.MAP_SPHERICAL if mapping == "spherical" else binding.MAP_CYLINDRICAL)
    assert np.allclose(t["xf"], np.float32([[.5, 0, 0, -.5], [0, .5, 0, -1], [0, 0, .5, -1.5]]), rtol=0, atol=1e-7)


def test_planar_mapping(binding, tmp_path):
    t, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "uv" "string mapping" "planar" "vector v1" [0 1 0] "vector v2" [0 0 2] '
                                  '"float udelta" [0.5] "float vdelta" [-1]')
    assert t["kind"] == binding.TEX_UV and t["mapping"] == binding.MAP_PLANAR
    assert t["vs"] == [0, 1, 0] and t["vt"] == [0, 0, 2] and (t["du"], t["dv"]) == (0.5, -1)
    d, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "uv" "string mapping" "planar"')
    assert d["vs"] == [1, 0, 0] and d["vt"] == [0, 1, 0] and (d["du"], d["dv"]) == (0, 0)


def test_unknown_mapping_is_uv(binding, tmp_path, capfd):
    t, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "uv" "string mapping" "cubic"')
    assert t["mapping"] == binding.MAP_UV and (t["su"], t["sv"]) == (1, 1)
    assert '2D texture mapping "cubic" unknown' in capfd.readouterr().err


def test_uv_float_refused(binding, tmp_path):
    _refused(binding, tmp_path, 'Texture "t" "float" "uv"\n', '"t"', '"uv" has no float version')


def test_bilerp_spectrum_defaults_and_values(binding, tmp_path):
    t, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "bilerp"')
    assert t["kind"] == binding.TEX_BILERP
    assert t["bilerp"].tolist() == [[0] * 3, [1] * 3, [0] * 3, [1] * 3]  # v00 0, v01 1, v10 0, v11 1
    t, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "bilerp" "rgb v00" [1 0 0] "rgb v01" [0 1 0] "rgb v10" [0 0 1] '
                                  '"rgb v11" [.5 .5 .5] "string mapping" "cylindrical"')
    assert t["bilerp"].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, .5]] and t["mapping"] == binding.MAP_CYLINDRICAL


def test_float_bilerp_as_roughness(binding, tmp_path):
    host = _scene(binding, tmp_path, 'Texture "r" "float" "bilerp" "float v00" [0.1] "float v11" [0.4]\n'
                                     'Material "plastic" "texture roughness" "r"\n')
    m = host.material(0)
    t = _textures(host)[m.rough_tex]
    assert t["kind"] == binding.TEX_BILERP
    assert np.allclose(t["bilerp"], np.float32([[.1] * 3, [1] * 3, [0] * 3, [.4] * 3]))


def test_scale_of_two_images(binding, tmp_path):
    t, texs = _kd(binding, tmp_path, 'Texture "t" "spectrum" "scale" "texture tex1" "ia" "texture tex2" "ib"', pre=_images(tmp_path))
    assert t["kind"] == binding.TEX_SCALE and t["n_levels"] == 0
    assert [texs[c]["kind"] for c in t["child"][:2]] == [binding.TEX_IMAGE] * 2 and t["child"][2] == -1


def test_mix_with_texture_amount(binding, tmp_path):
    t, texs = _kd(binding, tmp_path, 'Texture "amt" "float" "checkerboard" "string mapping" "planar"\n'
                                     'Texture "t" "spectrum" "mix" "texture tex1" "ia" "rgb tex2" [0 1 0] "texture amount" "amt"',
                  pre=_images(tmp_path))
    assert t["kind"] == binding.TEX_MIX
    assert t["child"][1] == -1 and t["cval"][1].tolist() == [0, 1, 0]
    assert texs[t["child"][0]]["kind"] == binding.TEX_IMAGE and texs[t["child"][2]]["kind"] == binding.TEX_CHECKER2D


def test_mix_defaults_with_one_texture(binding, tmp_path):
    t, _ = _kd(binding, tmp_path, 'Texture "t" "spectrum" "mix" "texture tex2" "ia"', pre=_images(tmp_path))
    assert t["child"][0] == -1 and t["cval"][0].tolist() == [0, 0, 0]  # tex1 0, amount 0.5 (mix.cpp:45-53)
    assert t["child"][2] == -1 and t["cval"][2].tolist() == [.5, .5, .5]


def test_checkerboard_of_images_is_a_combiner(binding, tmp_path):
    t, texs = _kd(binding, tmp_path, 'Texture "t" "spectrum" "checkerboard" "texture tex1" "ia" "texture tex2" "ib" '
                                     '"string aamode" "none"', pre=_images(tmp_path))
    assert t["kind"] == binding.TEX_CHECKER2D and [texs[c]["kind"] for c in t["child"][:2]] == [binding.TEX_IMAGE] * 2


def test_constant_subtrees_fold(binding, tmp_path):
    """Constants keep folding as before: no texture entry, the value in the material."""
    host = _scene(binding, tmp_path, 'Texture "c" "spectrum" "constant" "rgb value" [0.2 0.4 0.8]\n'
                                     'Texture "t" "spectrum" "mix" "texture tex1" "c" "rgb tex2" [1 1 1] "float amount" [0.5]\n'
                                     'Material "matte" "texture Kd" "t"\n')
    m = host.material(0)
    assert m.kd_tex == -1 and np.allclose(list(m.kd), [0.6, 0.7, 0.9])
    assert _textures(host) == []


def test_scale_of_image_keeps_its_form(binding, tmp_path):
    """A scale of one image by a constant stays (image, factor), and the image entry's appended fields are all zero."""
    host = _scene(binding, tmp_path, _images(tmp_path) + 'Texture "t" "spectrum" "scale" "texture tex1" "ia" "rgb tex2" [0.5 1 2]\n'
                                                         'Material "matte" "texture Kd" "t"\n')
    m = host.material(0)
    texs = _textures(host)
    assert list(m.kd) == [0.5, 1, 2] and texs[m.kd_tex]["kind"] == binding.TEX_IMAGE
    for t in texs:
        assert t["kind"] == binding.TEX_IMAGE and t["n_levels"] > 0 and t["mapping"] == 0 and t["aamode"] == 0
        assert t["child"] == [0, 0, 0] and not t["xf"].any() and not t["cval"].any() and not t["bilerp"].any()
        assert t["vs"] == [0, 0, 0] and t["vt"] == [0, 0, 0]


def test_deeper_tree_refused_with_its_name(binding, tmp_path):
    _refused(binding, tmp_path, _images(tmp_path) + 'Texture "inner" "spectrum" "scale" "texture tex1" "ia" "texture tex2" "ib"\n'
                                                     'Texture "outer" "spectrum" "mix" "texture tex1" "inner" "texture tex2" "ib"\n',
             '"outer"', '"inner"', "two levels")


def test_checkerboard_of_a_combiner_refused(binding, tmp_path):
    _refused(binding, tmp_path, _images(tmp_path) + 'Texture "ck" "spectrum" "checkerboard" "texture tex1" "ia"\n'
                                                     'Texture "top" "spectrum" "scale" "texture tex1" "ck" "texture tex2" "ib"\n',
             '"top"', '"ck"')


@pytest.mark.parametrize("top", [
    'Texture "top" "spectrum" "mix" "texture tex1" "s" "texture tex2" "ib"',
    'Texture "top" "spectrum" "mix" "texture tex1" "s" "rgb tex2" [0 0 0] "float amount" [0.3]',
    'Texture "top" "spectrum" "checkerboard" "texture tex1" "s" "texture tex2" "ib"',
    'Texture "top" "spectrum" "checkerboard" "texture tex1" "s"',
    'Texture "top" "spectrum" "scale" "texture tex1" "s" "texture tex2" "ib"',
])
def test_combiner_over_a_scaled_image_refused(binding, tmp_path, top):
    """A scale of one image by a constant is kept as (image, factor): a combination, not a leaf. A combiner over it is a third
    level and is refused with both textures named (taking its image alone would drop the factor)."""
    body = _images(tmp_path) + 'Texture "s" "spectrum" "scale" "texture tex1" "ia" "rgb tex2" [0.5 0.5 0.5]\n' + top + '\n'
    _refused(binding, tmp_path, body, '"top"', '"s"', "two levels")


def test_scaled_image_still_a_material_input(binding, tmp_path):
    """The (image, factor) pair itself keeps working as a material input, factor included."""
    host = _scene(binding, tmp_path, _images(tmp_path) + 'Texture "s" "spectrum" "scale" "texture tex1" "ia" "rgb tex2" [0.5 0.5 0.5]\n'
                                                         'Material "matte" "texture Kd" "s"\n')
    m = host.material(0)
    assert m.kd_tex >= 0 and list(m.kd) == [0.5, 0.5, 0.5]


@pytest.mark.parametrize("cls", ["fbm", "wrinkled", "windy", "marble", "dots"])
def test_noise_classes_refused(binding, tmp_path, cls):
    _refused(binding, tmp_path, f'Texture "t" "float" "{cls}"\n', f'"{cls}"', "noise permutation table")


def test_ptex_refused(binding, tmp_path):
    _refused(binding, tmp_path, 'Texture "t" "spectrum" "ptex" "string filename" "x.ptx"\n', '"ptex"', "Ptex library")


@pytest.mark.parametrize("param", ["alpha", "shadowalpha"])
def test_procedural_alpha_refused(binding, tmp_path, param):
    body = ('Texture "ck" "float" "checkerboard"\n'
            f'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 1 1 0] "texture {param}" "ck"\n')
    _refused(binding, tmp_path, body, '"ck"', f'"{param}"')


def test_procedural_metal_eta_refused(binding, tmp_path):
    _refused(binding, tmp_path, 'Texture "e" "spectrum" "checkerboard"\nMaterial "metal" "texture eta" "e"\n', '"eta"')


def test_every_parameter_takes_a_procedural_texture(binding, tmp_path):
    host = _scene(binding, tmp_path, 'Texture "c" "spectrum" "checkerboard"\nTexture "f" "float" "bilerp"\n'
                                     'Material "uber" "texture Kd" "c" "texture Ks" "c" "texture Kr" "c" "texture Kt" "c" '
                                     '"texture opacity" "c" "texture bumpmap" "f" "texture uroughness" "f" "texture vroughness" "f"\n'
                                     'Shape "sphere"\nMaterial "matte" "texture sigma" "f"\n')
    u, m = host.material(0), host.material(1)
    for k in ("kd_tex", "ks_tex", "kr_tex", "kt_tex", "opacity_tex", "bump_tex", "rough_tex", "rough_tex_v"):
        assert getattr(u, k) >= 0, k
    assert m.sigma_tex >= 0
