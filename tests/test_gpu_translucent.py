"""The translucent material on the device (GPU): the BSDF probes held to the float64 restatement of translucent_ref.py (f, pdf and
sampled directions with wo on both sides, a tilted geometric normal, a chi-square test of the sampling over the whole sphere);
bit-for-bit identities with uber and rough glass on every render path; a point light in front of and behind a plane through the
path integrator and the IISPT direct pass; a furnace; and the smaller cases (no lobes, bump and texture identities, alpha 0, the
IISPT frame and the C++ host)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

import microfacet_ref as R
import translucent_ref as T
from quadric_ref import write_scene
from test_gpu_metal_substrate import PLANE, _close, _probe_scene, _render, _sphere_dirs, _write_pfm

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
N_DIRS = 100_000


def _a(r, remap=True):
    return float(np.float32(R.roughness_to_alpha(r))) if remap else float(np.float32(r))


def _f32(v):
    return [float(np.float32(x)) for x in v]


# (material line, restated BSDF)
CASES = {
    "default": ('Material "translucent"', lambda: T.Translucent(_f32([.25] * 3), _f32([.25] * 3), [.5] * 3, [.5] * 3, _a(.1))),
    "kd_rt": ('Material "translucent" "rgb Kd" [0.6 0.6 0.6] "rgb Ks" [0 0 0] "rgb reflect" [0.4 0.4 0.4] "rgb transmit" [0.6 0.6 0.6]',
              lambda: T.Translucent(_f32([.6] * 3), [0] * 3, _f32([.4] * 3), _f32([.6] * 3), _a(.1))),
    "transmit_only": ('Material "translucent" "rgb reflect" [0 0 0] "rgb transmit" [0.9 0.9 0.9] "float roughness" [0.2]',
                      lambda: T.Translucent(_f32([.25] * 3), _f32([.25] * 3), [0] * 3, _f32([.9] * 3), _a(.2))),
    "reflect_only": ('Material "translucent" "rgb reflect" [0.8 0.8 0.8] "rgb transmit" [0 0 0] "float roughness" [0.05]',
                     lambda: T.Translucent(_f32([.25] * 3), _f32([.25] * 3), _f32([.8] * 3), [0] * 3, _a(.05))),
    "coloured": ('Material "translucent" "rgb Kd" [0.1 0.7 0.2] "rgb Ks" [0.3 0.2 0.1] "rgb reflect" [0.9 0.5 0.2] '
                 '"rgb transmit" [0.2 0.6 0.8] "float roughness" [0.3]',
                 lambda: T.Translucent(_f32([.1, .7, .2]), _f32([.3, .2, .1]), _f32([.9, .5, .2]), _f32([.2, .6, .8]), _a(.3))),
    "noremap": ('Material "translucent" "bool remaproughness" "false" "float roughness" [0.3] "rgb Ks" [0.5 0.5 0.5]',
                lambda: T.Translucent(_f32([.25] * 3), [.5] * 3, [.5] * 3, [.5] * 3, _a(.3, False))),
}
TILT = np.array([np.sin(np.radians(35)), 0, np.cos(np.radians(35))])


def _direction_pairs(rng, n):
    """wo on both sides; wi uniform on the sphere for a third of the pairs, near wo's mirror direction (the glossy reflection) for
    another, near -wo (the transmitted peak) for the last; all at least 0.05 off the surface."""
    wo = _sphere_dirs(rng, 3 * n)
    wo = wo[np.abs(wo[:, 2]) > 0.05][:n]
    jitter = 0.3 * rng.normal(size=(n, 3)) * rng.random((n, 1))
    mirror, through = wo * np.array([-1, -1, 1]) + jitter, -wo + jitter
    k = np.arange(n) % 3
    wi = np.where((k == 0)[:, None], _sphere_dirs(rng, n), np.where((k == 1)[:, None], mirror, through))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    keep = np.abs(wi[:, 2]) > 0.05
    return wo[keep].astype(np.float32), wi[keep].astype(np.float32)


# ---- BSDF probes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tilted", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_bsdf_eval_matches_restatement(binding, tmp_path, case, tilted):
    line, mk = CASES[case]
    host, gpu = _probe_scene(binding, tmp_path, line)
    ref = mk()
    wo, wi = _direction_pairs(np.random.default_rng(list(CASES).index(case)), N_DIRS)
    ng = TILT if tilted else np.array([0.0, 0, 1])
    out = (gpu.bsdf_eval_ng(0, ng, wo, wi) if tilted else gpu.bsdf_eval(0, wo, wi)).astype(np.float64)
    wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
    f, pdf = ref.f(wo64, wi64, ng.astype(np.float32).astype(np.float64)), ref.pdf(wo64, wi64)
    assert np.isfinite(out).all()
    scale_f, scale_p = np.abs(f).max(), np.abs(pdf).max()
    ok_f = _close(out[:, :3], f, 1e-4, 1e-7 * scale_f).all(axis=1)
    ok_p = _close(out[:, 3], pdf, 1e-4, 1e-7 * scale_p)
    assert (f.max(axis=1) > 0).mean() > 0.3 and (pdf > 0).mean() > 0.3
    assert ok_f.mean() > 0.9995 and ok_p.mean() > 0.9995, (ok_f.mean(), ok_p.mean())
    assert _close(out[:, :3], f, 2e-3, 1e-6 * scale_f).all() and _close(out[:, 3], pdf, 2e-3, 1e-6 * scale_p).all()
    gpu.close()


@pytest.mark.parametrize("tilted", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_bsdf_sample_matches_restatement(binding, tmp_path, case, tilted):
    line, mk = CASES[case]
    host, gpu = _probe_scene(binding, tmp_path, line)
    ref = mk()
    rng = np.random.default_rng(100 + list(CASES).index(case))
    wo = _sphere_dirs(rng, 2 * N_DIRS)
    wo = wo[np.abs(wo[:, 2]) > 0.05][:N_DIRS].astype(np.float32)
    u = rng.random((len(wo), 2)).astype(np.float32)
    ng = TILT if tilted else np.array([0.0, 0, 1])
    out = (gpu.bsdf_sample_ng(0, ng, wo, u) if tilted else gpu.bsdf_sample(0, wo, u)).astype(np.float64)
    ng64 = ng.astype(np.float32).astype(np.float64)
    wo64 = wo.astype(np.float64)
    wi_r, f_r, pdf_r = ref.sample(wo64, u[:, 0].astype(np.float64), u[:, 1].astype(np.float64), ng64)
    wi, f, pdf = out[:, :3], out[:, 3:6], out[:, 6]
    both = (pdf > 0) & (pdf_r > 0)
    assert both.sum() > 0.5 * len(wo)
    assert ((pdf > 0) != (pdf_r > 0)).mean() < 1e-3  # a direction right at the horizon or a refraction at its critical angle
    assert (wi[both, 2] * wo64[both, 2] < 0).mean() > 0.1 or case == "reflect_only"
    sel = both & (np.abs(wi_r[:, 2]) > 0.05)
    same_dir = np.linalg.norm(wi[sel] - wi_r[sel], axis=1) < 1e-3
    assert same_dir.mean() > 0.999, same_dir.mean()
    # f (BSDF::f's rule: every case has more than one lobe) and pdf at the device's own direction, restated
    fd, pd = ref.f(wo64[sel], wi[sel], ng64), ref.pdf(wo64[sel], wi[sel])
    ok = _close(f[sel], fd, 1e-3, 1e-6 * np.abs(fd).max()).all(axis=1) & _close(pdf[sel], pd, 1e-3, 1e-6 * pd.max())
    assert ok.mean() > 0.999, ok.mean()
    gpu.close()


def _hist(wi, nt, nphi):
    """Counts over nt x nphi (cos theta, phi) bins of the whole sphere."""
    ti = np.clip(((wi[:, 2] + 1) / 2 * nt).astype(int), 0, nt - 1)
    pi = np.minimum(((np.arctan2(wi[:, 1], wi[:, 0]) % (2 * np.pi)) / (2 * np.pi) * nphi).astype(int), nphi - 1)
    return np.bincount(ti * nphi + pi, minlength=nt * nphi).astype(np.float64)


def _chi2_pval(obs, exp):
    """Pearson's test of counts against expected counts; bins expected to hold fewer than 5 are pooled."""
    small = exp < 5
    obs, exp = np.append(obs[~small], obs[small].sum()), np.append(exp[~small], exp[small].sum())
    keep = exp > 0
    return stats.chi2.sf((((obs - exp) ** 2)[keep] / exp[keep]).sum(), keep.sum() - 1)


def _two_sample_pval(a, b):
    """The two-sample chi-square test of two histograms (bins holding fewer than 10 of both pooled)."""
    small = (a + b) < 10
    a, b = np.append(a[~small], a[small].sum()), np.append(b[~small], b[small].sum())
    keep = (a + b) > 0
    na, nb = a.sum(), b.sum()
    chi2 = ((np.sqrt(nb / na) * a - np.sqrt(na / nb) * b) ** 2 / (a + b))[keep].sum()
    return stats.chi2.sf(chi2, keep.sum() - 1)


@pytest.mark.parametrize("case, wo", [("default", (0.3, 0.2, 0.93)), ("kd_rt", (0.5, -0.5, -0.707)),
                                      ("transmit_only", (-0.6, 0.1, -0.79)), ("reflect_only", (0.4, -0.3, 0.87)),
                                      ("coloured", (0.8, 0.1, 0.59)), ("noremap", (0.2, 0.6, -0.77))])
def test_bsdf_sample_chi_square(binding, tmp_path, case, wo):
    """bsdf_sample's directions over 32 x 32 (cos theta, phi) bins of the whole sphere, with the samples that come back with pdf 0 as
    one more bin, against (1) the directions the float64 restatement samples (a two-sample test) and (2) where the material has no
    MicrofacetTransmission lobe, the counts bsdf_pdf (the device's) predicts, integrated by an 8 x 8 midpoint rule per bin. (The
    reference's MicrofacetTransmission::Pdf, reflection.cpp:435-447, also covers directions behind the microfacet that its Sample_f
    never yields, so its Pdf is not the density of its samples: tests/test_oracle_pins.py::test_bsdf_sampling_chi_square.)"""
    line, mk = CASES[case]
    ref = mk()
    host, gpu = _probe_scene(binding, tmp_path, line)
    n, nt, nphi, sub = 200_000, 32, 32, 8
    wo = np.array(wo, np.float64)
    wo /= np.linalg.norm(wo)
    rng = np.random.default_rng(11)
    wo32 = np.repeat(wo[None].astype(np.float32), n, 0)
    out = gpu.bsdf_sample(0, wo32, rng.random((n, 2)).astype(np.float32)).astype(np.float64)
    ok = out[:, 6] > 0
    assert ok.mean() > 0.5
    observed = np.append(_hist(out[ok, :3], nt, nphi), (~ok).sum())
    wi_r, _, pdf_r = ref.sample(wo32.astype(np.float64), rng.random(n), rng.random(n))
    restated = np.append(_hist(wi_r[pdf_r > 0], nt, nphi), (pdf_r == 0).sum())
    p2 = _two_sample_pval(observed, restated)
    assert p2 > 1e-4, p2
    if "micro_t" not in ref.lobes:
        c = -1 + 2 * (np.arange(nt * sub) + 0.5) / (nt * sub)
        p = ((np.arange(nphi * sub) + 0.5) / (nphi * sub)) * 2 * np.pi
        C, P = np.meshgrid(c, p, indexing="ij")
        s = np.sqrt(1 - C * C)
        dirs = np.stack([s * np.cos(P), s * np.sin(P), C], -1).reshape(-1, 3)
        pdf = gpu.bsdf_eval(0, np.repeat(wo[None].astype(np.float32), len(dirs), 0), dirs.astype(np.float32))[:, 3].astype(np.float64)
        dw = (2.0 / (nt * sub)) * (2 * np.pi / (nphi * sub))
        expected = (pdf.reshape(nt, sub, nphi, sub) * dw).sum(axis=(1, 3)).reshape(-1) * n
        expected = np.append(expected, max(n - expected.sum(), 0.0))
        p1 = _chi2_pval(observed, expected)
        assert p1 > 1e-4, p1
    gpu.close()


# ---- identities with uber and rough glass, bit for bit -------------------------------------------------------------------------
# (translucent, the material it must equal) over a plain and an image-textured variant
IDENTITIES = {
    "uber": ('Material "translucent" {kd} "rgb Ks" [0.3 0.3 0.3] "float roughness" [0.15] "rgb reflect" [1 1 1] "rgb transmit" [0 0 0]',
             'Material "uber" {kd} "rgb Ks" [0.3 0.3 0.3] "float roughness" [0.15] "rgb Kr" [0 0 0] "rgb Kt" [0 0 0] "float eta" [1.5]'),
    "glass_rt": ('Material "translucent" "rgb Kd" [0 0 0] {ks} "float roughness" [0.15] "rgb reflect" [1 1 1] "rgb transmit" [1 1 1]',
                 'Material "glass" {kr} {kt} "float uroughness" [0.15] "float vroughness" [0.15] "float eta" [1.5]'),
    "glass_t": ('Material "translucent" "rgb Kd" [0 0 0] {ks} "float roughness" [0.15] "rgb reflect" [0 0 0] "rgb transmit" [1 1 1]',
                'Material "glass" "rgb Kr" [0 0 0] {kt} "float uroughness" [0.15] "float vroughness" [0.15] "float eta" [1.5]'),
}
PLAIN = {"kd": '"rgb Kd" [0.5 0.3 0.2]', "ks": '"rgb Ks" [0.8 0.7 0.6]', "kr": '"rgb Kr" [0.8 0.7 0.6]', "kt": '"rgb Kt" [0.8 0.7 0.6]'}
TEXTURED = {"kd": '"texture Kd" "img"', "ks": '"texture Ks" "img"', "kr": '"texture Kr" "img"', "kt": '"texture Kt" "img"'}
ROOM = ('LightSource "point" "rgb I" [10 10 10] "point from" [0.3 -0.5 1.5]\nLightSource "infinite" "rgb L" [0.2 0.2 0.3]\n'
        'AttributeBegin\n{mat}\n' + PLANE + 'AttributeEnd\n'
        'AttributeBegin\n{mat}\nTranslate 0 0 0.6\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n'
        'AttributeBegin\nMaterial "matte" "rgb Kd" [0.6 0.3 0.2]\nTranslate 1.2 0.5 0.4\nShape "sphere" "float radius" [0.4]\nAttributeEnd\n')
COUNTERS = ("camera_rays closest_rays shadow_rays nodes_closest nodes_any tri_tests tri_hits sphere_tests nee_evals zero_radiance "
            "path_length n_paths ext_rays ext_nodes ext_tri_tests ext_sphere_tests any_tri_tests mis_rays_traced ext_rays_traced").split()


def _room_scene(tmp_path, mat, name, integrator="path", spp=2, depth=4, w=32, h=32):
    rng = np.random.default_rng(7)
    _write_pfm(tmp_path / "img.pfm", (0.2 + 0.8 * rng.random((32, 32, 3))).astype(np.float32))
    body = 'Texture "img" "spectrum" "imagemap" "string filename" ["img.pfm"]\n' + ROOM.format(mat=mat)
    return write_scene(tmp_path, body, name=name, w=w, h=h, spp=spp, depth=depth, fov=50, eye="0 -4 2", look="0 0 0.3", up="0 0 1",
                       integrator=integrator)


def _identity_pair(tmp_path, which, variant, **kw):
    fill = TEXTURED if variant == "textured" else PLAIN
    return [_room_scene(tmp_path, IDENTITIES[which][k].format(**fill), f"{which}_{variant}_{k}.pbrt", **kw) for k in (0, 1)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _counters(st):
    return {k: st[k] for k in COUNTERS}


@pytest.mark.parametrize("variant", ["plain", "textured"])
@pytest.mark.parametrize("which", list(IDENTITIES))
@pytest.mark.parametrize("collect", [False, True])
def test_identity_path_integrator(binding, tmp_path, which, variant, collect):
    out = []
    for path in _identity_pair(tmp_path, which, variant):
        host = binding.HostScene(path=path)
        gpu = binding.GpuScene(host)
        out.append(gpu.render(collect_stats=collect))
        gpu.close()
    (fa, sa), (fb, sb) = out
    assert fa.max() > 0 and np.array_equal(_bits(fa), _bits(fb))
    if collect:
        assert _counters(sa) == _counters(sb)


@pytest.mark.parametrize("variant", ["plain", "textured"])
@pytest.mark.parametrize("which", list(IDENTITIES))
def test_identity_direct_pass(binding, tmp_path, which, variant):
    films = []
    for path in _identity_pair(tmp_path, which, variant, integrator="iispt"):
        gpu = binding.GpuScene(binding.HostScene(path=path))
        films.append(gpu.render_direct(4))
        gpu.close()
    assert films[0].max() > 0 and np.array_equal(films[0], films[1])


@pytest.mark.parametrize("variant", ["plain", "textured"])
@pytest.mark.parametrize("which", list(IDENTITIES))
def test_identity_probe_pass(binding, tmp_path, which, variant):
    pos = np.array([[0, -1, 0.01], [0.5, -0.5, 0.3], [0, -0.5, 0.6], [0.2, 0.2, 1.5]])
    dirs = np.array([[0, 0, 1], [0, -0.6, 0.8], [0, -1, 0], [0, 0, -1]])
    out = []
    for path in _identity_pair(tmp_path, which, variant, integrator="iispt"):
        gpu = binding.GpuScene(binding.HostScene(path=path))
        out.append(gpu.render_probes(pos, dirs))
        gpu.close()
    a, b = out
    assert a[0].max() > 0
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(_bits(x), _bits(y))
    assert _counters(a[3]) == _counters(b[3])


def _iispt_modules():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    sys.path.insert(0, REPO)
    nn_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_nn")
    frame_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_frame")
    import iispt_torch_reference as ref_mod
    return torch, nn_mod, frame_mod, ref_mod


def _iispt_image(binding, path, n_tasks=4, n_direct=4):
    torch, nn_mod, frame_mod, ref_mod = _iispt_modules()
    torch.manual_seed(5)
    gpu = binding.GpuScene(binding.HostScene(path=path))
    frame = frame_mod.IisptFrame(binding, gpu, nn_mod.IisptPipeline(gpu, net=ref_mod.IISPTNet().eval()))
    frame.run_batched(n_tasks, radius_start=8.0)
    frame.run_direct(n_direct)
    torch.cuda.synchronize()
    assert frame.stats["probes"] > 0
    img = frame.image().cpu().numpy()
    gpu.close()
    return img


@pytest.mark.parametrize("variant", ["plain", "textured"])
@pytest.mark.parametrize("which", list(IDENTITIES))
def test_identity_iispt_frame(binding, tmp_path, which, variant):
    """The IISPT frame: the probe pass, the network, the gather and the direct pass."""
    _iispt_modules()
    a, b = [_iispt_image(binding, p) for p in _identity_pair(tmp_path, which, variant, integrator="iispt", spp=1)]
    assert a.max() > 0 and np.array_equal(_bits(a), _bits(b))


# ---- a point light in front of the plane and behind it -------------------------------------------------------------------------
RES, FOV, EYE, INTENSITY = 16, 30, np.array([0.0, -3.0, 2.0]), np.array([20.0, 15.0, 10.0])
LIGHTS = {"front": np.array([0.8, 1.0, 3.0]), "behind": np.array([0.8, 1.0, -3.0])}


def _lit_plane(tmp_path, line, light, integrator="path", spp=1, center=True, name="lit.pbrt", extra=""):
    hdr = (f'LookAt {EYE[0]} {EYE[1]} {EYE[2]}  0 0 0  0 0 1\nCamera "perspective" "float fov" [{FOV}]\n'
           f'Film "image" "integer xresolution" [{RES}] "integer yresolution" [{RES}] "string filename" "lit.exr"\nPixelFilter "box"\n'
           f'Sampler "halton" "integer pixelsamples" [{spp}] "bool samplepixelcenter" "{"true" if center else "false"}"\n'
           f'Integrator "{integrator}" "integer maxdepth" [1]\nWorldBegin\n')
    body = (f'LightSource "point" "rgb I" [{INTENSITY[0]} {INTENSITY[1]} {INTENSITY[2]}] "point from" [{light[0]} {light[1]} {light[2]}]\n'
            + extra + line + "\n" + PLANE + "WorldEnd\n")
    p = tmp_path / name
    p.write_text(hdr + body)
    return str(p)


def _point_light_radiance(ref, light, o, d):
    """f(wo, wi) I |cos theta_i| / r^2 at the z = 0 plane point each camera ray (o, d) reaches, in float64 (the plane's shading
    frame: n = ng = +z, ss = +x)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    t = -o[:, 2] / d[:, 2]
    p = o + t[:, None] * d
    wo = -d / np.linalg.norm(d, axis=1, keepdims=True)
    to_l = light[None, :] - p
    r2 = (to_l ** 2).sum(1)
    wi = to_l / np.sqrt(r2)[:, None]
    return T.radiance_point_light(ref, wo, wi, INTENSITY, r2)


@pytest.mark.parametrize("case, side", [(c, s) for c in ("default", "kd_rt", "coloured") for s in LIGHTS] +
                         [("transmit_only", "behind"), ("reflect_only", "front")])
def test_point_light_path_integrator(binding, tmp_path, case, side):
    line, mk = CASES[case]
    gpu = binding.GpuScene(binding.HostScene(path=_lit_plane(tmp_path, line, LIGHTS[side])))
    px, py = np.meshgrid(np.arange(RES), np.arange(RES))
    px, py = px.reshape(-1), py.reshape(-1)
    L, _ = gpu.li_samples(px, py, np.zeros_like(px))
    o, d = gpu.camera_rays(np.stack([px + 0.5, py + 0.5], 1))
    want = _point_light_radiance(mk(), LIGHTS[side], o, d)
    assert want.max() > 0
    assert np.allclose(L, want, rtol=1e-3, atol=1e-6 * want.max()), np.abs(L - want).max()
    gpu.close()


@pytest.mark.parametrize("side", list(LIGHTS))
@pytest.mark.parametrize("case", ["default", "kd_rt"])
def test_point_light_direct_pass(binding, tmp_path, case, side):
    """The IISPT direct pass over 64 jittered passes, each pixel against the restated radiance averaged over an 8 x 8 grid inside
    it; tolerances as in the metal / substrate test."""
    line, mk = CASES[case]
    gpu = binding.GpuScene(binding.HostScene(path=_lit_plane(tmp_path, line, LIGHTS[side], integrator="iispt", center=False,
                                                             name="lit_iispt.pbrt")))
    mon = gpu.render_direct(64)
    img = mon[..., :3] / mon[..., 3:4]
    sub = (np.arange(8) + 0.5) / 8
    gx, gy = np.meshgrid(np.arange(RES)[:, None] + sub[None, :], np.arange(RES)[:, None] + sub[None, :])
    o, d = gpu.camera_rays(np.stack([gx.reshape(-1), gy.reshape(-1)], 1))
    want = _point_light_radiance(mk(), LIGHTS[side], o, d).reshape(RES, 8, RES, 8, 3).mean(axis=(1, 3))
    assert np.isfinite(img).all()
    assert np.allclose(img, want, rtol=5e-2, atol=1e-3 * want.max()), np.abs(img / want - 1).max()
    assert abs(img.mean() / want.mean() - 1) < 1e-2, img.mean() / want.mean()
    gpu.close()


# ---- furnace ------------------------------------------------------------------------------------------------------------------
FURNACE = ('LightSource "infinite" "rgb L" [1 1 1]\n'
           'Material "translucent" "rgb Kd" [1 1 1] "rgb Ks" [0 0 0] "rgb reflect" [0.5 0.5 0.5] "rgb transmit" [0.5 0.5 0.5]\n'
           'Shape "sphere" "float radius" [1]\n')


def test_furnace_path_integrator(binding, tmp_path):
    """A closed sphere that scatters all it receives (reflect + transmit = Kd = 1), under L = 1 from every direction, at maxdepth
    14: every pixel that sees only the sphere sees 1 (what leaks past the last bounce is below 1e-4)."""
    w = 24
    path = write_scene(tmp_path, FURNACE, w=w, h=w, spp=256, depth=14, fov=30, eye="0 -4 0", look="0 0 0", up="0 0 1")
    host = binding.HostScene(path=path)
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    rgb = host.film_to_rgb(film).astype(np.float64)
    # pixels whose four corners all look at the sphere (closest approach of the ray to the centre below 0.98)
    cx, cy = np.meshgrid(np.arange(w + 1), np.arange(w + 1))
    o, d = gpu.camera_rays(np.stack([cx.reshape(-1), cy.reshape(-1)], 1).astype(np.float64))
    gpu.close()
    o, d = o.astype(np.float64), d.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    miss = np.linalg.norm(o - (o * d).sum(1)[:, None] * d, axis=1).reshape(w + 1, w + 1)
    inside = (miss[:-1, :-1] < .98) & (miss[1:, :-1] < .98) & (miss[:-1, 1:] < .98) & (miss[1:, 1:] < .98)
    assert inside.sum() > 150
    assert np.isfinite(rgb).all()
    mean = rgb[inside].mean(0)
    assert np.all(np.abs(mean - 1) < 1e-2), mean
    assert np.all(np.abs(rgb[inside].mean(1) - 1) < 0.25)


def test_furnace_probe_pass(binding, tmp_path):
    """Probes on the furnace sphere. Facing out along the normal (as IISPT places them), every direction escapes at once, and the
    probe pass adds no infinite light at its first bounce (iispt_d.cpp:115-133): 0. Facing in, each hemisphere sees the inside of
    the sphere: light comes in through LambertianTransmission only, 1/2 at every vertex (the light sample and the BSDF sample under
    MIS), and half the continuations leave the sphere, so the probe pass's three vertices (maxdepth 3, iispt_d.cpp:135-136) see
    1/2 + 1/4 + 1/8 = 7/8 in expectation; each hemisphere's mean is held to that."""
    path = write_scene(tmp_path, FURNACE, w=8, h=8, spp=1, depth=14, fov=30, eye="0 -4 0", look="0 0 0", up="0 0 1", integrator="iispt")
    gpu = binding.GpuScene(binding.HostScene(path=path))
    n = np.array([[0, -1, 0], [0.6, -0.8, 0], [0, 0, 1], [-0.48, 0.6, -0.64]], np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out_i, _, out_d, _ = gpu.render_probes(1.001 * n, n)
    in_i, _, in_d, _ = gpu.render_probes(0.999 * n, -n)
    gpu.close()
    assert np.isfinite(out_i).all() and np.isfinite(in_i).all()
    assert (out_i == 0).all()
    means = in_i.astype(np.float64).mean(axis=(1, 2))
    assert np.all(np.abs(means / 0.875 - 1) < 2e-2), means


# ---- smaller cases ------------------------------------------------------------------------------------------------------------
BEHIND = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [5 5 5]\nTranslate 0 0.2 -1\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n')


def test_no_lobes_renders_black_and_occludes(binding, tmp_path):
    """reflect = transmit = 0: the BSDF exists with no lobe (translucent.cpp:53-55 returns after allocating it), so the plane is
    black and opaque, not skipped as an interface would be: the area light and the point light behind it stay hidden."""
    films = {}
    for name, line in (("none", 'Material "translucent" "rgb reflect" [0 0 0] "rgb transmit" [0 0 0]'), ("default", CASES["default"][0])):
        path = _lit_plane(tmp_path, line, LIGHTS["behind"], spp=4, center=False, name=f"{name}.pbrt", extra=BEHIND)
        path_text = open(path).read().replace('"integer maxdepth" [1]', '"integer maxdepth" [5]')
        open(path, "w").write(path_text)
        films[name] = _render(binding, path)
    assert np.isfinite(films["none"]).all() and (films["none"] == 0).all()
    assert films["default"].max() > 0  # the same scene with light passing through the plane


@pytest.mark.parametrize("case", ["default", "coloured"])
def test_zero_bump_map_equals_plain(binding, tmp_path, case):
    _write_pfm(tmp_path / "zero.pfm", np.zeros((4, 4, 3), np.float32))
    tex = 'Texture "zero" "float" "imagemap" "string filename" ["zero.pfm"]\n'
    line = CASES[case][0]
    for side in LIGHTS:
        a = _render(binding, _lit_plane(tmp_path, line, LIGHTS[side], spp=4, center=False, name="plain.pbrt"))
        b = _render(binding, _lit_plane(tmp_path, tex + line + ' "texture bumpmap" "zero"', LIGHTS[side], spp=4, center=False, name="bump.pbrt"))
        assert a.max() > 0
        assert np.allclose(a, b, rtol=1e-4, atol=1e-6 * a.max()), (side, np.abs(a - b).max())


@pytest.mark.parametrize("plain, textured", [
    ('Material "translucent" "rgb reflect" [0.5 0.5 0.5]', 'Material "translucent" "texture reflect" "half"'),
    ('Material "translucent" "rgb transmit" [0.5 0.5 0.5]', 'Material "translucent" "texture transmit" "half"'),
    ('Material "translucent" "float roughness" [0.25]', 'Material "translucent" "texture roughness" "quarter"'),
])
def test_constant_image_texture_equals_constant(binding, tmp_path, plain, textured):
    _write_pfm(tmp_path / "half.pfm", np.full((8, 8, 3), 0.5, np.float32))
    _write_pfm(tmp_path / "quarter.pfm", np.full((8, 8, 3), 0.25, np.float32))
    tex = ('Texture "half" "spectrum" "imagemap" "string filename" ["half.pfm"]\n'
           'Texture "quarter" "float" "imagemap" "string filename" ["quarter.pfm"]\n')
    for side in LIGHTS:
        a = _render(binding, _lit_plane(tmp_path, plain, LIGHTS[side], spp=4, center=False, name="plain.pbrt"))
        b = _render(binding, _lit_plane(tmp_path, tex + textured, LIGHTS[side], spp=4, center=False, name="textured.pbrt"))
        assert a.max() > 0
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6 * a.max()), (side, np.abs(a - b).max())


def _leaf_room(integrator="path", spp=4):
    mat = 'Material "translucent" "rgb Kd" [0.2 0.6 0.1] "rgb Ks" [0.1 0.1 0.1] "rgb reflect" [0.4 0.4 0.4] "rgb transmit" [0.6 0.6 0.6]'
    body = ('LightSource "point" "rgb I" [10 10 10] "point from" [0 0 -1.5]\nLightSource "infinite" "rgb L" [0.2 0.2 0.3]\n'
            'AttributeBegin\n' + mat + '\n' + PLANE + 'AttributeEnd\n'
            'AttributeBegin\nMaterial "matte" "rgb Kd" [0.6 0.3 0.2]\nTranslate 0 0 0.6\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n'
            'AttributeBegin\n' + mat + '\nTranslate 1.2 0.5 0.4\nShape "sphere" "float radius" [0.4]\nAttributeEnd\n')
    return dict(body=body, w=32, h=32, spp=spp, depth=3, fov=50, eye="0 -4 2", look="0 0 0.3", up="0 0 1", integrator=integrator)


def test_alpha_zero_renders_finite(binding, tmp_path):
    """roughness 0 without remapping is alpha 0: the microfacet terms come out as 0 / 0, and the render loop's radiance guards drop
    those samples; the Lambertian lobes still light the film."""
    kw = _leaf_room()
    kw["body"] = kw["body"].replace('"rgb Ks" [0.1 0.1 0.1]', '"rgb Ks" [0.1 0.1 0.1] "bool remaproughness" "false" "float roughness" [0]')
    host = binding.HostScene(path=write_scene(tmp_path, kw.pop("body"), **kw))
    assert any(host.material(i).alpha == 0 for i in range(host.info["n_materials"]))
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    gpu.close()
    rgb = host.film_to_rgb(film)
    assert np.isfinite(film).all() and np.isfinite(rgb).all() and rgb.max() > 0


def test_iispt_frame_is_finite_and_repeatable(binding, tmp_path):
    _iispt_modules()
    kw = _leaf_room(integrator="iispt", spp=1)
    path = write_scene(tmp_path, kw.pop("body"), **kw)
    a, b = _iispt_image(binding, path, n_direct=8), _iispt_image(binding, path, n_direct=8)
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(_bits(a), _bits(b))


def test_cli_renders_the_binding_film(binding, tmp_path):
    """`iile_pbrt` (GpuPathIntegrator) renders the translucent scene to the film the Python binding does, bit for bit."""
    kw = _leaf_room()
    path = write_scene(tmp_path, kw.pop("body"), **kw)
    out = tmp_path / "cli.pfm"
    exe = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
    p = subprocess.run([exe, path, "--outfile", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    raw = out.read_bytes()
    head = b"PF\n32 32\n-1.0\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], "<f4").reshape(32, 32, 3)[::-1]
    want = _render(binding, path).astype(np.float32)
    assert want.max() > 0 and (img.view(np.uint32) == want.view(np.uint32)).all()


def test_cli_iispt_integrator_writes_the_python_frames_image(binding, tmp_path):
    """`iile_pbrt` with `Integrator "iispt"` renders the translucent scene to the images the Python frame makes with the same
    network, schedule and direct passes: merged, indirect and direct, bit for bit."""
    torch, nn_mod, frame_mod, ref_mod = _iispt_modules()
    n_tasks, n_direct = 4, 2
    kw = _leaf_room(integrator="iispt", spp=1)
    path = write_scene(tmp_path, kw.pop("body"), **kw)
    torch.manual_seed(3)
    module = ref_mod.IISPTNet().eval()
    net_file = tmp_path / "net.iilenet"
    binding.save_net_weights(module.state_dict(), str(net_file), bn_eps=module.encoder1[3].eps)
    out, ind, direct = tmp_path / "frame.pfm", tmp_path / "indirect.pfm", tmp_path / "direct.pfm"
    exe = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
    env = dict(os.environ, IISPT_SCHEDULE_RADIUS_START="8")
    p = subprocess.run([exe, path, f"--iisptNet={net_file}", f"--iileIndirect={n_tasks}", f"--iileDirect={n_direct}", "--outfile", str(out),
                        f"--iisptIndirectOut={ind}", f"--iisptDirectOut={direct}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stdout
    host = binding.HostScene(path=path)
    gpu = binding.GpuScene(host)
    frame = frame_mod.IisptFrame(binding, gpu, nn_mod.IisptPipeline(gpu, net=module))
    frame.run_batched(n_tasks, radius_start=8.0)
    frame.run_direct(n_direct)
    torch.cuda.synchronize()
    head = b"PF\n32 32\n-1.0\n"
    for f, want, name in ((out, frame.image(), "merged"), (ind, frame.indirect_image(), "indirect"), (direct, frame.direct_image(), "direct")):
        raw = f.read_bytes()
        assert raw.startswith(head), name
        got = np.frombuffer(raw[len(head):], "<f4").reshape(32, 32, 3)[::-1]
        want = want.cpu().numpy()
        assert float(want.max()) > 0 and np.isfinite(want).all(), name
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    gpu.close()
