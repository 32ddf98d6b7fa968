"""The CPU oracle on the features added after image textures (CPU, no GPU).

1. Refusal: a scene with a feature the oracle does not restate (disks and cylinders, procedural textures, mappings other than uv)
   is refused by every entry point that reads it, with an exception that names the feature, instead of being read through the
   wrong arrays. This list shrinks as features are restated.
2. Metal and substrate, restated in oracle_path.cpp from metal.cpp, substrate.cpp and reflection.cpp, pinned to the float64
   restatement of microfacet_ref.py: f, pdf, sampled directions, a tilted geometric normal, and the alpha-0 metal.
Both run in libm trig mode, the reference's own behaviour.
3. Sample_f with the specular lobes allowed (oracle_bsdf_sample_specular): which lobe each u0 takes, the two flags, the exits
   with pdf 0, and plastic against the existing mode. It runs in portable trig mode, the mode test_gpu_oracle_features.py holds
   the device to it in, over the same inputs."""
import numpy as np
import pytest

import microfacet_ref as R
import oracle_binding as ob
from quadric_ref import write_scene
from test_gpu_metal_substrate import CASES, PLANE, _direction_pairs, _sphere_dirs

LIBM = ob.TRIG_LIBM
LIGHT = 'LightSource "point" "rgb I" [1 1 1] "point from" [0 0 5]\n'
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0  1 -1 0  1 1 0  -1 1 0] "float uv" [0 0 1 0 1 1 0 1]\n'


def _write_pfm(path, rows):
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


IMAGES = ('Texture "ia" "spectrum" "imagemap" "string filename" ["a.pfm"]\n'
          'Texture "ib" "spectrum" "imagemap" "string filename" ["b.pfm"]\n')
# (scene body, the feature named by the exception, whether it is a texture feature: oracle.texture_eval refuses it too)
UNSUPPORTED = {
    "disk": ('Shape "disk" "float radius" [2]\n', "quadric", False),
    "cylinder": ('AttributeBegin\nTranslate 0 0 1\nShape "cylinder" "float radius" [0.5] "float zmin" [-1] "float zmax" [1]\nAttributeEnd\n',
                 "quadric", False),
    "disk_light": ('AttributeBegin\nTranslate 0 0 3\nAreaLightSource "diffuse" "rgb L" [4 4 4]\nShape "disk" "float radius" [0.5]\nAttributeEnd\n',
                   "quadric", False),
    "checkerboard_2d": ('Texture "t" "spectrum" "checkerboard" "float uscale" [4] "float vscale" [4]\n', "checkerboard (2D)", True),
    "checkerboard_3d": ('Texture "t" "spectrum" "checkerboard" "integer dimension" [3]\n', "checkerboard (3D)", True),
    "uv": ('Texture "t" "spectrum" "uv"\n', "uv", True),
    "bilerp": ('Texture "t" "spectrum" "bilerp" "rgb v00" [1 0 0] "rgb v11" [0 0 1]\n', "bilerp", True),
    "scale": (IMAGES + 'Texture "t" "spectrum" "scale" "texture tex1" "ia" "texture tex2" "ib"\n', "scale", True),
    "mix": (IMAGES + 'Texture "t" "spectrum" "mix" "texture tex1" "ia" "texture tex2" "ib" "float amount" [0.3]\n', "mix", True),
    # (the loader gives the 2D mappings to procedural textures only: a mapping is named before the texture's kind)
    "spherical": ('Texture "t" "spectrum" "checkerboard" "string mapping" "spherical"\n', "spherical", True),
    "cylindrical": ('Texture "t" "spectrum" "checkerboard" "string mapping" "cylindrical"\n', "cylindrical", True),
    "planar": ('Texture "t" "spectrum" "checkerboard" "string mapping" "planar" "vector v1" [1 0 0] "vector v2" [0 1 0]\n', "planar", True),
}


def _unsupported_scene(binding, tmp_path, name):
    body, feature, is_tex = UNSUPPORTED[name]
    _write_pfm(tmp_path / "a.pfm", np.full((4, 4, 3), 0.5, np.float32))
    _write_pfm(tmp_path / "b.pfm", np.full((4, 4, 3), 0.25, np.float32))
    mat = 'Material "matte" "texture Kd" "t"\n' if is_tex else 'Material "matte"\n'
    host = binding.HostScene(path=write_scene(tmp_path, body + mat + QUAD + LIGHT, w=8, h=8, spp=1, depth=2))
    return host, feature, is_tex


@pytest.mark.parametrize("name", list(UNSUPPORTED))
def test_oracle_refuses_what_it_does_not_restate(binding, oracle, tmp_path, name):
    host, feature, is_tex = _unsupported_scene(binding, tmp_path, name)
    calls = {"render": lambda: oracle.render(host, threads=1),
             "li": lambda: oracle.li(host, [4], [4], [0]),
             "iispt_direct": lambda: oracle.iispt_direct(host, 1, threads=1),
             "render_probe": lambda: oracle.render_probe(host, [0, 0, -4], [0, 0, 1]),
             "camera_hit_differentials": lambda: oracle.camera_hit_differentials(host, 4.0, 4.0)}
    if is_tex:
        calls["texture_eval"] = lambda: oracle.texture_eval(host, host.material(0).kd_tex, [[0.5, 0.5]], [[0.01, 0, 0, 0.01]])
    else:
        calls["hit_geometry"] = lambda: oracle.hit_geometry(host, [0, 0, -4], [0, 0, 1])
        calls["intersect"] = lambda: oracle.intersect(host, [[0, 0, -4]], [[0, 0, 1]], [np.inf])
        calls["intersect_p"] = lambda: oracle.intersect_p(host, [[0, 0, -4]], [[0, 0, 1]], [np.inf])
    for entry, call in calls.items():
        with pytest.raises(ob.OracleUnsupported) as e:
            call()
        assert feature in e.value.feature and feature in str(e.value), (entry, str(e.value))


def test_restated_materials_are_not_refused(binding, oracle, tmp_path):
    for i, (line, _) in enumerate(CASES.values()):
        host = binding.HostScene(path=write_scene(tmp_path, line + "\n" + QUAD + LIGHT, name=f"m{i}.pbrt", w=8, h=8, spp=1, depth=2))
        film, _ = oracle.render(host, threads=1)
        assert np.isfinite(film).all() and film[..., 3].min() > 0


# ---- metal and substrate against microfacet_ref.py ------------------------------------------------------------------------------
# Tolerances, measured over these catalogues: the oracle is float32 in the reference's operation order, the restatement float64.
# f and pdf (eval and at the sampled directions) agree to a relative error of 9e-6 at the 99.9th percentile and 1.8e-5 at worst
# (copper's default alpha, 0.01 remapped); asserted: 2e-5 and 5e-5. The sampled directions go through TrowbridgeReitzSample11's
# inversion, which amplifies one float rounding: 3e-4 at the 99.9th percentile (copper, alpha 0.4 / 0.15), asserted 1e-3; and 99%
# within 1e-4.
N = 20_000


def _probe_host(binding, tmp_path, case):
    line, mk = CASES[case]
    return binding.HostScene(path=write_scene(tmp_path, line + "\n" + PLANE + LIGHT, depth=1)), mk()


def _rel(got, want, scale):
    return np.abs(got - want) / (np.abs(want) + 1e-6 * scale)


@pytest.mark.parametrize("case", list(CASES))
def test_bsdf_eval_matches_restatement(binding, oracle, tmp_path, case):
    host, ref = _probe_host(binding, tmp_path, case)
    wo, wi = _direction_pairs(np.random.default_rng(list(CASES).index(case)), N)
    out = oracle.bsdf_eval(host, 0, wo, wi, trig_mode=LIBM).astype(np.float64)
    f, pdf = ref.f(wo.astype(np.float64), wi.astype(np.float64)), ref.pdf(wo.astype(np.float64), wi.astype(np.float64))
    assert (f.max(axis=1) > 0).mean() > 0.3
    ef, ep = _rel(out[:, :3], f, np.abs(f).max()), _rel(out[:, 3], pdf, pdf.max())
    assert np.quantile(ef, 0.999) < 2e-5 and np.quantile(ep, 0.999) < 2e-5, (np.quantile(ef, 0.999), np.quantile(ep, 0.999))
    assert ef.max() < 5e-5 and ep.max() < 5e-5, (ef.max(), ep.max())
    # the batch pdf is the same function
    assert np.array_equal(oracle.bsdf_pdf_batch(host, 0, wo[0], wi[:2000]),
                          oracle.bsdf_eval(host, 0, np.repeat(wo[:1], 2000, 0), wi[:2000], trig_mode=LIBM)[:, 3])


@pytest.mark.parametrize("case", list(CASES))
def test_bsdf_sample_matches_restatement(binding, oracle, tmp_path, case):
    host, ref = _probe_host(binding, tmp_path, case)
    rng = np.random.default_rng(100 + list(CASES).index(case))
    wo = _sphere_dirs(rng, 2 * N)
    wo = wo[np.abs(wo[:, 2]) > 0.05][:N].astype(np.float32)
    u = rng.random((len(wo), 2)).astype(np.float32)
    out = oracle.bsdf_sample(host, 0, wo, u, trig_mode=LIBM).astype(np.float64)
    wi_r, f_r, pdf_r = ref.sample(wo.astype(np.float64), u[:, 0].astype(np.float64), u[:, 1].astype(np.float64))
    wi, f, pdf = out[:, :3], out[:, 3:6], out[:, 6]
    assert ((pdf > 0) != (pdf_r > 0)).mean() < 1e-3  # a direction right at the horizon may fall either way
    sel = (pdf > 0) & (pdf_r > 0) & (np.abs(wi_r[:, 2]) > 0.05)
    assert sel.mean() > 0.7
    dist = np.linalg.norm(wi[sel] - wi_r[sel], axis=1)
    assert np.quantile(dist, 0.999) < 1e-3 and (dist < 1e-4).mean() > 0.99, (np.quantile(dist, 0.999), (dist < 1e-4).mean())
    fd, pd = ref.f(wo[sel].astype(np.float64), wi[sel]), ref.pdf(wo[sel].astype(np.float64), wi[sel])
    ef, ep = _rel(f[sel], fd, np.abs(fd).max()), _rel(pdf[sel], pd, pd.max())
    assert np.quantile(ef, 0.999) < 2e-5 and np.quantile(ep, 0.999) < 2e-5, (np.quantile(ef, 0.999), np.quantile(ep, 0.999))
    assert ef.max() < 5e-5 and ep.max() < 5e-5, (ef.max(), ep.max())
    # the batch sampler draws the same directions and pdfs
    wib, pdfb = oracle.bsdf_sample_batch(host, 0, wo[0], u[:2000])
    one = oracle.bsdf_sample(host, 0, np.repeat(wo[:1], 2000, 0), u[:2000], trig_mode=LIBM)
    assert np.array_equal(wib[one[:, 6] > 0], one[one[:, 6] > 0, :3])


@pytest.mark.parametrize("case", ["gold_iso", "aluminium_aniso", "substrate_default"])
def test_bsdf_with_tilted_geometric_normal(binding, oracle, tmp_path, case):
    """A one-lobe BSDF's Sample_f returns the lobe's f even where wi is below the geometric plane (reflection.cpp:772-780 recomputes f,
    with the reflect test against ng, only when more than one BxDF matches); BSDF::f tests against ng always (reflection.cpp:686-699)."""
    host, ref = _probe_host(binding, tmp_path, case)
    t = np.radians(35)
    ng = np.array([np.sin(t), 0, np.cos(t)], np.float32)
    rng = np.random.default_rng(21)
    z, phi = rng.uniform(0.1, 0.5, N), rng.uniform(-0.7, 0.7, N)
    wo = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1).astype(np.float32)
    out = oracle.bsdf_sample(host, 0, wo, rng.random((N, 2)).astype(np.float32), trig_mode=LIBM, ng=ng).astype(np.float64)
    wi, f, pdf = out[:, :3], out[:, 3:6], out[:, 6]
    below = (pdf > 0) & (wi[:, 2] > 0.05) & (wi @ ng < -0.02)
    above = (pdf > 0) & (wi[:, 2] > 0.05) & (wi @ ng > 0.02)
    assert below.sum() > 100 and above.sum() > 100, (below.sum(), above.sum())
    wo64 = wo.astype(np.float64)
    for sel in (below, above):
        fr = ref.f(wo64[sel], wi[sel])
        assert (fr.max(axis=1) > 0).all()
        assert _rel(f[sel], fr, np.abs(fr).max()).max() < 5e-5
    ev = oracle.bsdf_eval(host, 0, wo[below], wi[below].astype(np.float32), trig_mode=LIBM, ng=ng)
    assert (ev[:, :3] == 0).all() and (ev[:, 3] > 0).all()


def test_metal_alpha_zero(binding, oracle, tmp_path):
    """roughness 0 without remapping: TrowbridgeReitz with alpha 0, whose D is 0 / 0 off the normal. Whatever the reference computes
    there, the restatement computes the same: NaN or 0 at the same places, never a finite value that differs."""
    host = binding.HostScene(path=write_scene(tmp_path, 'Material "metal" "bool remaproughness" "false" "float roughness" [0]\n' + PLANE + LIGHT,
                                              depth=1))
    ref = R.Metal([float(np.float32(v)) for v in (0.199989721, 0.922085762, 1.09987628)],
                  [float(np.float32(v)) for v in (3.90463829, 2.44763327, 2.13765097)], 0.0, 0.0)
    wo, wi = _direction_pairs(np.random.default_rng(5), 2000)
    out = oracle.bsdf_eval(host, 0, wo, wi, trig_mode=LIBM).astype(np.float64)
    with np.errstate(all="ignore"):
        f = ref.f(wo.astype(np.float64), wi.astype(np.float64))
    fin = np.isfinite(f) & np.isfinite(out[:, :3])
    assert np.array_equal(np.isnan(out[:, :3]), np.isnan(f))
    assert np.allclose(out[:, :3][fin], f[fin], rtol=5e-5, atol=0)


# ---- Sample_f with the specular lobes allowed ---------------------------------------------------------------------------------------
# (material line, the lobes of its BSDF in BxDF order). R: specular reflection, T: specular transmission, F: FresnelSpecular
# (reflection or transmission by the Fresnel term), g: a lobe that is not specular
SPECULAR_CASES = {
    "mirror": ('Material "mirror" "rgb Kr" [.9 .8 .7]', "R"),
    "glass": ('Material "glass" "rgb Kr" [.9 .8 .7] "rgb Kt" [.6 .7 .8] "float index" [1.5]', "F"),
    "glass_r_black": ('Material "glass" "rgb Kr" [0 0 0] "rgb Kt" [.6 .7 .8] "float index" [1.5]', "F"),
    "uber_kr_only": ('Material "uber" "rgb Kd" [0 0 0] "rgb Ks" [0 0 0] "rgb Kr" [.8 .7 .6]', "R"),
    "uber_five_lobes": ('Material "uber" "rgb Kd" [.3 .4 .5] "rgb Ks" [.4 .3 .2] "rgb Kr" [.5 .6 .7] "rgb Kt" [.7 .6 .5] '
                        '"rgb opacity" [.4 .4 .4] "float index" [1.4]', "TggRT"),
    "plastic": ('Material "plastic"', "gg"),
}
N_SPECULAR = 4000
U0_TOP = np.float32(float.fromhex("0x1.fffffep-1"))


def lobe_boundaries():
    """every k / matching that u0 can meet with one to five lobes, the float just below each, and the largest float below 1"""
    ks = sorted({float(np.float32(k) / np.float32(m)) for m in range(1, 6) for k in range(m)})
    below = [float(np.nextafter(np.float32(v), np.float32(0))) for v in ks if v > 0]
    return np.array(sorted(set(ks + below + [float(U0_TOP)])), np.float32)


def specular_probe_inputs(case):
    """(wo, u) of one case: wo on both sides of the surface, a fifth of them grazing (|wo.z| < 0.02: total internal reflection, and
    wo.z == 0 itself, Sample_f's first exit); u0 from lobe_boundaries() for the first half — one boundary per five consecutive
    directions, one of them grazing, the list tiled over the half, so every boundary meets grazing and other directions whatever
    the seed —, uniform for the rest."""
    rng = np.random.default_rng(4100 + sorted(SPECULAR_CASES).index(case))
    n = N_SPECULAR
    wo = _sphere_dirs(rng, n)
    grazing = np.arange(n) % 5 == 0
    phi = rng.random(n) * 2 * np.pi
    z = rng.uniform(-0.02, 0.02, n)
    z[:50] = 0
    flat = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    wo = np.where(grazing[:, None], flat, wo).astype(np.float32)
    u = rng.random((n, 2)).astype(np.float32)
    b = lobe_boundaries()
    u[:n // 2, 0] = b[(np.arange(n // 2) // 5) % len(b)]
    assert np.abs(wo[grazing, 2]).max() < 0.02 and (wo[:, 2] > 0.02).sum() > n // 4 and (wo[:, 2] < -0.02).sum() > n // 4
    assert set(b.tolist()) <= set(u[grazing, 0].tolist()) and set(b.tolist()) <= set(u[~grazing, 0].tolist())
    return wo, u


@pytest.mark.parametrize("case", list(SPECULAR_CASES))
def test_bsdf_sample_specular_lobes_and_flags(binding, oracle, tmp_path, case):
    """The oracle's Sample_f with BSDF_ALL. Bit for bit: the lobe u0 picks (comp = min(floor(u0 n), n - 1), in float as the
    reference multiplies) decides the two flags; a specular reflection is wo mirrored, with pdf 1 (mirror, uber) or the Fresnel
    term (glass); plastic, without a specular lobe, gives what the existing mode gives; wo.z == 0 leaves everything zero; and where
    pdf is 0 (total internal reflection in uber's Kt lobe) f and both flags are 0."""
    line, lobes = SPECULAR_CASES[case]
    host = binding.HostScene(path=write_scene(tmp_path, line + "\n" + PLANE + LIGHT, depth=1))
    wo, u = specular_probe_inputs(case)
    out = oracle.bsdf_sample_specular(host, 0, wo, u, trig_mode=ob.TRIG_PORTABLE)
    wi, f, pdf, spec, trans = out[:, :3], out[:, 3:6], out[:, 6], out[:, 7], out[:, 8]
    assert set(np.unique(out[:, 7:]).tolist()) <= {0.0, 1.0}
    zero = wo[:, 2] == 0
    assert zero.sum() == 10 and not out[zero].any()
    dead = pdf == 0
    assert not f[dead].any() and not spec[dead].any() and not trans[dead].any()
    n = len(lobes)
    comp = np.minimum(np.floor(u[:, 0] * np.float32(n)).astype(int), n - 1)
    picked = np.array(list(lobes))[comp]
    live = ~dead
    assert (spec[live] == (picked[live] != "g")).all()
    assert (trans[live & (picked == "T")] == 1).all() and (trans[live & (picked == "R")] == 0).all()
    assert (trans[live & (picked == "g")] == 0).all()
    refl = live & (spec == 1) & (trans == 0)
    assert np.array_equal(wi[refl].view(np.uint32), (wo[refl] * np.float32([-1, -1, 1])).view(np.uint32))
    thru = live & (trans == 1)
    assert (wi[thru, 2] * wo[thru, 2] < 0).all()
    if lobes == "F":
        assert refl.any() and thru.any()   # both halves (under total internal reflection the Fresnel term is 1: it reflects)
        assert not dead[~zero].any()
        assert ((pdf[live] > 0) & (pdf[live] <= 1)).all()
        if case == "glass_r_black":
            assert not f[refl].any() and f[thru].all(axis=1).all()
    elif lobes == "R":
        assert refl.sum() == live.sum() == (~zero).sum() and (pdf[live] == 1).all()
    elif case == "uber_five_lobes":
        for k in range(n):   # every lobe taken, on both sides of the surface
            assert (live & (comp == k) & (wo[:, 2] > 0)).any() and (live & (comp == k) & (wo[:, 2] < 0)).any(), k
        assert (pdf[live & (picked != "g")] == np.float32(1) / np.float32(5)).all()
        tir = dead & ~zero & (comp == 4)
        assert tir.any() and (wo[tir, 2] < 0).all()   # total internal reflection: the Kt lobe, from inside only
    else:
        plain = oracle.bsdf_sample(host, 0, wo, u, trig_mode=ob.TRIG_PORTABLE)
        assert np.array_equal(out[:, 3:7].view(np.uint32), plain[:, 3:].view(np.uint32)) and not out[:, 7:].any()
        ok = plain[:, 6] > 0
        assert np.array_equal(wi[ok].view(np.uint32), plain[ok, :3].view(np.uint32))
