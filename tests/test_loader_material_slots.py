"""Which texture slot of iile_material each material parameter feeds, held from the outside (CPU): every material of the loader,
every spectrum parameter, the roughness parameters, "bumpmap" and "sigma", one image texture at a time. The tables below are
written by hand from the reference's Create*Material functions (the lines cited beside each row), not read from the library:
a parameter a material looks up with GetSpectrumTexture / GetFloatTexture takes the image, a parameter it never looks up does
not see it."""
import numpy as np
import pytest

from quadric_ref import write_scene
from test_metal_substrate_scenes import QUAD, _write_pfm

SLOTS = ("kd_tex", "ks_tex", "kr_tex", "kt_tex", "opacity_tex", "rough_tex", "rough_tex_v", "bump_tex", "sigma_tex")

# spectrum parameter -> slot, from each material's GetSpectrumTexture calls
SPECTRUM = {
    "matte": {"Kd": "kd_tex"},                                                                  # matte.cpp:66
    "plastic": {"Kd": "kd_tex", "Ks": "ks_tex"},                                                # plastic.cpp:74-76
    "uber": {"Kd": "kd_tex", "Ks": "ks_tex", "Kr": "kr_tex", "Kt": "kt_tex", "opacity": "opacity_tex"},  # uber.cpp:105-111, 121
    "mirror": {"Kr": "kr_tex"},                                                                 # mirror.cpp:60
    "glass": {"Kr": "kr_tex", "Kt": "kt_tex"},                                                  # glass.cpp:96-98
    "metal": {},                                                                                # metal.cpp:119-122: eta, k (no slot: constants only)
    "substrate": {"Kd": "kd_tex", "Ks": "ks_tex"},                                              # substrate.cpp:69-71
    "translucent": {"Kd": "kd_tex", "Ks": "ks_tex", "reflect": "kr_tex", "transmit": "kt_tex"},  # translucent.cpp:84-90
    "disney": {"color": "kd_tex"},                                                              # disney.cpp:592
}
MATERIALS = tuple(SPECTRUM)
COMMON = ("Kd", "Ks", "Kr", "Kt", "opacity")   # an image on one of these that the material does not read is ignored
OWN = ("reflect", "transmit", "color")         # an image on one of these is taken by its own material only, refused elsewhere
REFUSAL_LIST = {"translucent": "(Kd, Ks, Kr, Kt, opacity, reflect, transmit)", "disney": "(Kd, Ks, Kr, Kt, opacity, color)"}

# rough_tex_v without a "vroughness": -2 where alpha_v follows alpha (one roughness, or uber's roughv = roughu, uber.cpp:83-86),
# -1 where v is a parameter of its own (glass.cpp:102-104, metal.cpp:124-128, substrate.cpp:73-75)
V_DEFAULT = {m: -1 if m in ("glass", "metal", "substrate") else -2 for m in MATERIALS}

# float image on a roughness parameter -> (rough_tex, rough_tex_v); "I" is the image, None a refusal
ROUGH_REFUSED = {"roughness": None, "uroughness": None, "vroughness": None}
ONE_ROUGHNESS = {"roughness": ("I", -2), "uroughness": None, "vroughness": None}
ROUGH = {
    "matte": ROUGH_REFUSED,          # matte.cpp:66-69 reads none
    "mirror": ROUGH_REFUSED,         # mirror.cpp:60-62 reads none
    "glass": ROUGH_REFUSED,          # glass.cpp:102-104 reads u and v; this renderer takes numbers only there
    "plastic": ONE_ROUGHNESS,        # plastic.cpp:78
    "translucent": ONE_ROUGHNESS,    # translucent.cpp:92
    "disney": ONE_ROUGHNESS,         # disney.cpp:597
    # uber.cpp:113-117 with uber.cpp:79-86: roughu = uroughness or roughness, roughv = vroughness or roughu
    "uber": {"roughness": ("I", -2), "uroughness": ("I", -2), "vroughness": (-1, "I")},
    # metal.cpp:124-128 with metal.cpp:68-71: each of u and v is its own parameter, or "roughness"
    "metal": {"roughness": ("I", "I"), "uroughness": ("I", -1), "vroughness": (-1, "I")},
    # substrate.cpp:73-75: "roughness" is never looked up
    "substrate": {"roughness": (-1, -1), "uroughness": ("I", -1), "vroughness": (-1, "I")},
}
ROUGH_MESSAGE = "roughness: a float \"imagemap\" texture is supported on"

# four image textures, so that every index asked for below is a different one and none is 0
INDEX = {"col": 1, "flt": 2, "flt2": 3}


@pytest.fixture(scope="module")
def pre(tmp_path_factory):
    d = tmp_path_factory.mktemp("slots")
    _write_pfm(d / "c.pfm", np.full((2, 2, 3), 0.5, np.float32))
    return d, ('Texture "pad" "spectrum" "imagemap" "string filename" ["c.pfm"]\n'
               'Texture "col" "spectrum" "imagemap" "string filename" ["c.pfm"]\n'
               'Texture "flt" "float" "imagemap" "string filename" ["c.pfm"]\n'
               'Texture "flt2" "float" "imagemap" "string filename" ["c.pfm"]\n')


def _slots(binding, pre, line):
    d, text = pre
    s = binding.HostScene(path=write_scene(d, text + line + "\n" + QUAD))
    assert s.info["n_materials"] == 1
    m = s.material(0)
    return {f: getattr(m, f) for f in SLOTS}


def _defaults(material):
    return {f: (V_DEFAULT[material] if f == "rough_tex_v" else -1) for f in SLOTS}


@pytest.mark.parametrize("material", MATERIALS)
def test_spectrum_parameters(binding, pre, material):
    """An image on each spectrum parameter in turn: the parameter's own slot gets the texture's index and nothing else moves; a
    parameter the material lacks is ignored (Kd .. opacity) or refused by name (reflect, transmit, color)."""
    assert _slots(binding, pre, f'Material "{material}"') == _defaults(material)
    for param in COMMON + OWN:
        line = f'Material "{material}" "texture {param}" "col"'
        slot = SPECTRUM[material].get(param)
        if slot is None and param in OWN:
            listed = REFUSAL_LIST.get(material, "(Kd, Ks, Kr, Kt, opacity)")
            with pytest.raises(RuntimeError) as e:
                _slots(binding, pre, line)
            assert str(e.value).endswith(f'image texture "col" on parameter "{param}" is not supported {listed}'), (param, str(e.value))
            continue
        want = _defaults(material)
        if slot is not None:
            want[slot] = INDEX["col"]
        assert _slots(binding, pre, line) == want, param


@pytest.mark.parametrize("param", ["eta", "k"])
def test_metal_spectra_take_no_image(binding, pre, param):
    with pytest.raises(RuntimeError, match=f'Material "metal": parameter "{param}" given as the image texture "col" is not supported'):
        _slots(binding, pre, f'Material "metal" "texture {param}" "col"')


@pytest.mark.parametrize("material", MATERIALS)
def test_roughness_images(binding, pre, material):
    for param, want_uv in ROUGH[material].items():
        line = f'Material "{material}" "texture {param}" "flt"'
        if want_uv is None:
            with pytest.raises(RuntimeError) as e:
                _slots(binding, pre, line)
            assert ROUGH_MESSAGE in str(e.value), (param, str(e.value))
            continue
        want = _defaults(material)
        want["rough_tex"], want["rough_tex_v"] = (INDEX["flt"] if v == "I" else v for v in want_uv)
        assert _slots(binding, pre, line) == want, param


def test_roughness_parameters_that_hide_one_another(binding, pre):
    """uber: "uroughness" hides "roughness", "vroughness" defaults to u (uber.cpp:79-86); metal: u and v fall back to "roughness"
    each on its own (metal.cpp:68-71)."""
    img, img2 = INDEX["flt"], INDEX["flt2"]

    def uv(line):
        s = _slots(binding, pre, line)
        return s["rough_tex"], s["rough_tex_v"]
    assert uv('Material "uber" "texture roughness" "flt" "float uroughness" [0.2]') == (-1, -2)
    assert uv('Material "uber" "texture roughness" "flt" "texture uroughness" "flt2"') == (img2, -2)
    assert uv('Material "uber" "texture roughness" "flt" "float vroughness" [0.2]') == (img, -1)
    assert uv('Material "uber" "texture roughness" "flt" "texture vroughness" "flt2"') == (img, img2)
    assert uv('Material "metal" "texture roughness" "flt" "float uroughness" [0.2]') == (-1, img)
    assert uv('Material "metal" "texture roughness" "flt" "float vroughness" [0.2]') == (img, -1)
    assert uv('Material "metal" "texture roughness" "flt" "texture uroughness" "flt2"') == (img2, img)
    assert uv('Material "metal" "float roughness" [0.3] "texture vroughness" "flt2"') == (-1, img2)
    assert uv('Material "substrate" "texture uroughness" "flt" "texture vroughness" "flt2"') == (img, img2)


@pytest.mark.parametrize("material", MATERIALS)
def test_bumpmap_and_sigma(binding, pre, material):
    """GetFloatTextureOrNull("bumpmap") of every Create*Material (matte.cpp:69 .. disney.cpp:619); glass's is not carried by this
    renderer. "sigma" is matte's alone (matte.cpp:67)."""
    line = f'Material "{material}" "texture bumpmap" "flt2"'
    if material == "glass":
        with pytest.raises(RuntimeError, match="bumpmap: only a float \"imagemap\" texture on matte / plastic"):
            _slots(binding, pre, line)
    else:
        want = _defaults(material)
        want["bump_tex"] = INDEX["flt2"]
        assert _slots(binding, pre, line) == want
    line = f'Material "{material}" "texture sigma" "flt"'
    if material == "matte":
        want = _defaults(material)
        want["sigma_tex"] = INDEX["flt"]
        assert _slots(binding, pre, line) == want
    else:
        with pytest.raises(RuntimeError, match="sigma: a float \"imagemap\" texture is supported on matte only"):
            _slots(binding, pre, line)
