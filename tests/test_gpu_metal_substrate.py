"""Metal and substrate on the device (GPU), held to the float64 restatement of microfacet_ref.py: the kernel-level BSDF probes
(f, pdf, sampled directions, a chi-square test of the sampling against the pdf), direct lighting under a point light through the
path integrator and the IISPT direct pass, both halves of MIS under a uniform infinite light, image textures and bump maps, the
probe pass and the IISPT frame, the C++ host, and the alpha-0 metal."""
import json
import os
import subprocess

import numpy as np
import pytest
from scipy import stats

import microfacet_ref as R
from quadric_ref import write_scene

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
COPPER = json.load(open(os.path.join(REPO, "tests", "golden", "copper_fixture.json")))
N_DIRS = 100_000
PLANE = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-50 -50 0  50 -50 0  50 50 0  -50 50 0] "float uv" [0 0 1 0 1 1 0 1]\n'

# (material line, restated BSDF); the alphas as the loader computes them (float32), the restatement in float64
def _a(r, remap=True):
    return float(np.float32(R.roughness_to_alpha(r))) if remap else float(np.float32(r))


def _f32(v):
    return [float(np.float32(x)) for x in v]


GOLD = ([0.143, 0.374, 1.442], [3.983, 2.385, 1.603])
ALUMINIUM = ([1.657, 0.880, 0.521], [9.224, 6.270, 4.837])
CASES = {
    "copper_default": ('Material "metal"', lambda: R.Metal(COPPER["eta"], COPPER["k"], _a(.01), _a(.01))),
    "gold_iso": ('Material "metal" "rgb eta" [%g %g %g] "rgb k" [%g %g %g] "float roughness" [0.2]' % (*GOLD[0], *GOLD[1]),
                 lambda: R.Metal(_f32(GOLD[0]), _f32(GOLD[1]), _a(.2), _a(.2))),
    "aluminium_aniso": ('Material "metal" "rgb eta" [%g %g %g] "rgb k" [%g %g %g] "float uroughness" [0.05] "float vroughness" [0.3]'
                        % (*ALUMINIUM[0], *ALUMINIUM[1]), lambda: R.Metal(_f32(ALUMINIUM[0]), _f32(ALUMINIUM[1]), _a(.05), _a(.3))),
    "gold_noremap_aniso": ('Material "metal" "rgb eta" [%g %g %g] "rgb k" [%g %g %g] "bool remaproughness" "false" '
                           '"float uroughness" [0.4] "float vroughness" [0.15]' % (*GOLD[0], *GOLD[1]),
                           lambda: R.Metal(_f32(GOLD[0]), _f32(GOLD[1]), _a(.4, False), _a(.15, False))),
    "substrate_default": ('Material "substrate"', lambda: R.Substrate([.5] * 3, [.5] * 3, _a(.1), _a(.1))),
    "substrate_red_aniso": ('Material "substrate" "rgb Kd" [0.7 0.1 0.05] "rgb Ks" [0.04 0.04 0.04] "float uroughness" [0.02] '
                            '"float vroughness" [0.3]', lambda: R.Substrate(_f32([.7, .1, .05]), _f32([.04] * 3), _a(.02), _a(.3))),
    "substrate_noremap": ('Material "substrate" "rgb Kd" [0.2 0.5 0.3] "rgb Ks" [0.3 0.2 0.1] "bool remaproughness" "false" '
                          '"float uroughness" [0.25] "float vroughness" [0.25]',
                          lambda: R.Substrate(_f32([.2, .5, .3]), _f32([.3, .2, .1]), .25, .25)),
}


def _probe_scene(binding, tmp_path, line):
    host = binding.HostScene(path=write_scene(tmp_path, line + "\n" + PLANE + 'LightSource "point" "rgb I" [1 1 1] "point from" [0 0 5]\n',
                                              depth=1))
    return host, binding.GpuScene(host)


def _sphere_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _direction_pairs(rng, n):
    """wo anywhere; wi uniform on the sphere for half the pairs, near wo's mirror direction for the other half (the glossy peak);
    both at least GRAZING off the surface."""
    wo = _sphere_dirs(rng, 3 * n)
    wo = wo[np.abs(wo[:, 2]) > 0.05][:n]
    mirror = wo * np.array([-1, -1, 1])
    near = mirror + 0.3 * rng.normal(size=(n, 3)) * rng.random((n, 1))
    near /= np.linalg.norm(near, axis=1, keepdims=True)
    wi = np.where((np.arange(n) % 2 == 0)[:, None], _sphere_dirs(rng, n), near)
    keep = np.abs(wi[:, 2]) > 0.05
    return wo[keep].astype(np.float32), wi[keep].astype(np.float32)


def _close(got, want, rtol, floor):
    """|got - want| <= rtol |want| + floor, elementwise."""
    return np.abs(got - want) <= rtol * np.abs(want) + floor


@pytest.mark.parametrize("case", list(CASES))
def test_bsdf_eval_matches_restatement(binding, tmp_path, case):
    line, mk = CASES[case]
    host, gpu = _probe_scene(binding, tmp_path, line)
    ref = mk()
    wo, wi = _direction_pairs(np.random.default_rng(list(CASES).index(case)), N_DIRS)
    out = gpu.bsdf_eval(0, wo, wi).astype(np.float64)
    wo64, wi64 = wo.astype(np.float64), wi.astype(np.float64)
    f, pdf = ref.f(wo64, wi64), ref.pdf(wo64, wi64)
    assert np.isfinite(out).all()
    scale_f, scale_p = np.abs(f).max(), np.abs(pdf).max()
    ok_f = _close(out[:, :3], f, 1e-4, 1e-7 * scale_f).all(axis=1)
    ok_p = _close(out[:, 3], pdf, 1e-4, 1e-7 * scale_p)
    assert (f.max(axis=1) > 0).mean() > 0.3  # most pairs are in the lobe's hemisphere, many near its peak
    assert ok_f.mean() > 0.9995 and ok_p.mean() > 0.9995, (ok_f.mean(), ok_p.mean())
    assert _close(out[:, :3], f, 2e-3, 1e-6 * scale_f).all() and _close(out[:, 3], pdf, 2e-3, 1e-6 * scale_p).all()
    gpu.close()


@pytest.mark.parametrize("case", list(CASES))
def test_bsdf_sample_matches_restatement(binding, tmp_path, case):
    line, mk = CASES[case]
    host, gpu = _probe_scene(binding, tmp_path, line)
    ref = mk()
    rng = np.random.default_rng(100 + list(CASES).index(case))
    wo = _sphere_dirs(rng, 2 * N_DIRS)
    wo = wo[np.abs(wo[:, 2]) > 0.05][:N_DIRS].astype(np.float32)
    u = rng.random((len(wo), 2)).astype(np.float32)
    out = gpu.bsdf_sample(0, wo, u).astype(np.float64)
    wi_r, f_r, pdf_r = ref.sample(wo.astype(np.float64), u[:, 0].astype(np.float64), u[:, 1].astype(np.float64))
    wi, f, pdf = out[:, :3], out[:, 3:6], out[:, 6]
    both = (pdf > 0) & (pdf_r > 0)
    assert both.sum() > 0.7 * len(wo)
    assert ((pdf > 0) != (pdf_r > 0)).mean() < 1e-3  # a direction right at the horizon may fall either way
    sel = both & (np.abs(wi_r[:, 2]) > 0.05)
    same_dir = np.linalg.norm(wi[sel] - wi_r[sel], axis=1) < 1e-3
    assert same_dir.mean() > 0.999, same_dir.mean()
    # f and pdf at the device's own direction, restated
    fd, pd = ref.f(wo[sel].astype(np.float64), wi[sel]), ref.pdf(wo[sel].astype(np.float64), wi[sel])
    ok = _close(f[sel], fd, 1e-3, 1e-6 * np.abs(fd).max()).all(axis=1) & _close(pdf[sel], pd, 1e-3, 1e-6 * pd.max())
    assert ok.mean() > 0.999, ok.mean()
    gpu.close()


@pytest.mark.parametrize("case, wo", [("gold_iso", (0.3, 0.2, 0.93)), ("gold_noremap_aniso", (0.6, -0.3, 0.74)),
                                      ("substrate_default", (0.5, 0.5, 0.707)), ("substrate_noremap", (-0.8, 0.1, 0.59))])
def test_bsdf_sample_chi_square(binding, tmp_path, case, wo):
    """bsdf_sample's directions against the expected counts from bsdf_pdf (the device's), integrated over 16 x 32 (cos theta, phi)
    bins of the upper hemisphere by an 8 x 8 midpoint rule; bins expected to hold fewer than 5 samples are pooled, and the samples
    that come back with pdf 0 are one more bin."""
    line, _ = CASES[case]
    host, gpu = _probe_scene(binding, tmp_path, line)
    n, nt, nphi, sub = 200_000, 16, 32, 8
    wo = np.array(wo, np.float64)
    wo /= np.linalg.norm(wo)
    rng = np.random.default_rng(11)
    out = gpu.bsdf_sample(0, np.repeat(wo[None].astype(np.float32), n, 0), rng.random((n, 2)).astype(np.float32)).astype(np.float64)
    ok = out[:, 6] > 0
    wi = out[ok, :3]
    assert (wi[:, 2] > 0).all()
    ti = np.minimum((wi[:, 2] * nt).astype(int), nt - 1)
    pi = np.minimum(((np.arctan2(wi[:, 1], wi[:, 0]) % (2 * np.pi)) / (2 * np.pi) * nphi).astype(int), nphi - 1)
    observed = np.bincount(ti * nphi + pi, minlength=nt * nphi).astype(np.float64)
    c = ((np.arange(nt * sub) + 0.5) / (nt * sub))
    p = ((np.arange(nphi * sub) + 0.5) / (nphi * sub)) * 2 * np.pi
    C, P = np.meshgrid(c, p, indexing="ij")
    s = np.sqrt(1 - C * C)
    dirs = np.stack([s * np.cos(P), s * np.sin(P), C], -1).reshape(-1, 3)
    pdf = gpu.bsdf_eval(0, np.repeat(wo[None].astype(np.float32), len(dirs), 0), dirs.astype(np.float32))[:, 3].astype(np.float64)
    dw = (1.0 / (nt * sub)) * (2 * np.pi / (nphi * sub))
    expected = (pdf.reshape(nt, sub, nphi, sub) * dw).sum(axis=(1, 3)).reshape(-1) * n
    observed = np.append(observed, (~ok).sum())
    expected = np.append(expected, max(n - expected.sum(), 0.0))
    small = expected < 5
    obs = np.append(observed[~small], observed[small].sum())
    exp = np.append(expected[~small], expected[small].sum())
    keep = exp > 0
    chi2 = (((obs - exp) ** 2)[keep] / exp[keep]).sum()
    pval = stats.chi2.sf(chi2, keep.sum() - 1)
    assert pval > 1e-4, (chi2, keep.sum(), pval)
    gpu.close()


@pytest.mark.parametrize("case", ["gold_iso", "aluminium_aniso", "substrate_default"])
def test_bsdf_sample_with_tilted_geometric_normal(binding, tmp_path, case):
    """Where the geometric normal differs from the shading one (a bump map, a mesh's "normal N"), BSDF::Sample_f of a one-lobe BSDF
    returns the lobe's own f: reflection.cpp:772-780 recomputes f, with its reflect test against ng, only when more than one BxDF
    matches. BSDF::f applies the test always (reflection.cpp:686-699). So for a sampled direction above the shading plane and below
    the geometric one, bsdf_sample gives the restated lobe f and bsdf_eval gives 0 (the pdf is the lobe's in both)."""
    line, mk = CASES[case]
    host, gpu = _probe_scene(binding, tmp_path, line)
    ref = mk()
    t = np.radians(35)
    ng = np.array([np.sin(t), 0, np.cos(t)])
    rng = np.random.default_rng(21)
    n = N_DIRS
    z = rng.uniform(0.1, 0.5, n)
    phi = rng.uniform(-0.7, 0.7, n)
    wo = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1).astype(np.float32)
    out = gpu.bsdf_sample_ng(0, ng, wo, rng.random((n, 2)).astype(np.float32)).astype(np.float64)
    wi, f, pdf = out[:, :3], out[:, 3:6], out[:, 6]
    wo64 = wo.astype(np.float64)
    below = (pdf > 0) & (wi[:, 2] > 0.05) & (wi @ ng < -0.02)
    above = (pdf > 0) & (wi[:, 2] > 0.05) & (wi @ ng > 0.02)
    assert below.sum() > 500 and above.sum() > 500, (below.sum(), above.sum())
    for sel in (below, above):
        fr = ref.f(wo64[sel], wi[sel])
        assert (fr.max(axis=1) > 0).all()
        ok = _close(f[sel], fr, 1e-3, 1e-6 * np.abs(fr).max()).all(axis=1) & _close(pdf[sel], ref.pdf(wo64[sel], wi[sel]), 1e-3, 0)
        assert ok.mean() > 0.999, ok.mean()
    ev = gpu.bsdf_eval_ng(0, ng, wo[below], wi[below].astype(np.float32)).astype(np.float64)
    assert (ev[:, :3] == 0).all()
    assert _close(ev[:, 3], ref.pdf(wo64[below], wi[below].astype(np.float32).astype(np.float64)), 1e-3, 0).mean() > 0.999
    gpu.close()


# ---- direct lighting ------------------------------------------------------------------------------------------------------------
RES, FOV, EYE, LIGHT, INTENSITY = 16, 30, np.array([0.0, -3.0, 2.0]), np.array([0.8, 1.0, 3.0]), np.array([20.0, 15.0, 10.0])
LIT_CASES = ["gold_iso", "aluminium_aniso", "substrate_default", "substrate_red_aniso"]


def _lit_plane(tmp_path, line, integrator="path", spp=1, center=True, name="lit.pbrt"):
    hdr = (f'LookAt {EYE[0]} {EYE[1]} {EYE[2]}  0 0 0  0 0 1\nCamera "perspective" "float fov" [{FOV}]\n'
           f'Film "image" "integer xresolution" [{RES}] "integer yresolution" [{RES}] "string filename" "lit.exr"\nPixelFilter "box"\n'
           f'Sampler "halton" "integer pixelsamples" [{spp}] "bool samplepixelcenter" "{"true" if center else "false"}"\n'
           f'Integrator "{integrator}" "integer maxdepth" [1]\nWorldBegin\n')
    body = (f'LightSource "point" "rgb I" [{INTENSITY[0]} {INTENSITY[1]} {INTENSITY[2]}] "point from" [{LIGHT[0]} {LIGHT[1]} {LIGHT[2]}]\n'
            + line + "\n" + PLANE + "WorldEnd\n")
    p = tmp_path / name
    p.write_text(hdr + body)
    return str(p)


def _point_light_radiance(ref, o, d):
    """f(wo, wi) I |cos theta_i| / r^2 at the z = 0 plane point each camera ray (o, d) reaches, in float64. The plane's shading
    frame: n = +z, ss = dp/du = +x."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    t = -o[:, 2] / d[:, 2]
    p = o + t[:, None] * d
    wo = -d / np.linalg.norm(d, axis=1, keepdims=True)
    to_l = LIGHT[None, :] - p
    r2 = (to_l ** 2).sum(1)
    wi = to_l / np.sqrt(r2)[:, None]
    return ref.f(wo, wi) * INTENSITY[None, :] * np.abs(wi[:, 2:3]) / r2[:, None]


@pytest.mark.parametrize("case", LIT_CASES)
def test_point_light_path_integrator(binding, tmp_path, case):
    line, mk = CASES[case]
    host = binding.HostScene(path=_lit_plane(tmp_path, line))
    gpu = binding.GpuScene(host)
    px, py = np.meshgrid(np.arange(RES), np.arange(RES))
    px, py = px.reshape(-1), py.reshape(-1)
    L, _ = gpu.li_samples(px, py, np.zeros_like(px))
    o, d = gpu.camera_rays(np.stack([px + 0.5, py + 0.5], 1))
    want = _point_light_radiance(mk(), o, d)
    assert want.max() > 0
    assert np.allclose(L, want, rtol=1e-3, atol=1e-6 * want.max()), np.abs(L - want).max()
    gpu.close()


@pytest.mark.parametrize("case", ["gold_iso", "gold_noremap_aniso", "substrate_default", "substrate_noremap"])
def test_point_light_direct_pass(binding, tmp_path, case):
    """The IISPT direct pass (UniformSampleAllLights at the camera vertex) over 64 jittered passes: each pixel against the
    restated radiance averaged over an 8 x 8 grid inside it (the materials with the broader lobes: a narrow highlight varies across
    a pixel more than 64 jittered samples resolve to this tolerance; the direct film's pixel is a filtered, jittered estimate, so a
    pixel may sit a few percent off the box average where the radiance curves, while the image mean stays within 1 %)."""
    line, mk = CASES[case]
    host = binding.HostScene(path=_lit_plane(tmp_path, line, integrator="iispt", center=False, name="lit_iispt.pbrt"))
    gpu = binding.GpuScene(host)
    mon = gpu.render_direct(64)
    img = mon[..., :3] / mon[..., 3:4]
    sub = (np.arange(8) + 0.5) / 8
    gx, gy = np.meshgrid(np.arange(RES)[:, None] + sub[None, :], np.arange(RES)[:, None] + sub[None, :])
    o, d = gpu.camera_rays(np.stack([gx.reshape(-1), gy.reshape(-1)], 1))
    want = _point_light_radiance(mk(), o, d).reshape(RES, 8, RES, 8, 3).mean(axis=(1, 3))
    assert np.isfinite(img).all()
    assert np.allclose(img, want, rtol=5e-2, atol=1e-3 * want.max()), np.abs(img / want - 1).max()
    assert abs(img.mean() / want.mean() - 1) < 1e-2, img.mean() / want.mean()
    gpu.close()


# ---- both halves of MIS under a uniform infinite light ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["gold_iso", "aluminium_aniso", "substrate_default", "substrate_red_aniso"])
def test_infinite_light_albedo(binding, tmp_path, case):
    """A plane under an infinite light of L = 1 at maxdepth 1: each pixel sees the directional albedo rho(wo) of the plane point its
    centre looks at — light sampling and BSDF sampling both contribute (EstimateDirect's two halves). Four pixels of a 3 x 3 frame
    (wo from about 12 to 50 degrees above the plane, at different azimuths); the mean over 1024 samples of each is held to the
    restated albedo (importance-sampled quadrature) within 5 combined standard errors."""
    line, mk = CASES[case]
    hdr = ('LookAt 0 -3 2  0 0 0  0 0 1\nCamera "perspective" "float fov" [40]\n'
           'Film "image" "integer xresolution" [3] "integer yresolution" [3] "string filename" "inf.exr"\n'
           'Sampler "halton" "integer pixelsamples" [1024] "bool samplepixelcenter" "true"\nIntegrator "path" "integer maxdepth" [1]\n'
           'WorldBegin\nLightSource "infinite" "rgb L" [1 1 1]\n')
    p = tmp_path / "inf.pbrt"
    p.write_text(hdr + line + "\n" + PLANE + "WorldEnd\n")
    host = binding.HostScene(path=str(p))
    gpu = binding.GpuScene(host)
    k = np.arange(1024)
    wos = []
    for px, py in ((1, 1), (0, 0), (2, 0), (2, 2)):
        L, _ = gpu.li_samples(np.full_like(k, px), np.full_like(k, py), k)
        o, d = gpu.camera_rays(np.array([[px + 0.5, py + 0.5]]))
        wo = -d[0].astype(np.float64) / np.linalg.norm(d[0])
        wos.append(wo)
        want, want_se = R.directional_albedo(mk(), wo)
        L = L.astype(np.float64)
        got, got_se = L.mean(0), L.std(0) / np.sqrt(len(L))
        assert (np.abs(got - want) < 5 * np.hypot(got_se, want_se) + 1e-4).all(), ((px, py), got, want, got_se, want_se)
    assert np.ptp([w[2] for w in wos]) > 0.3  # the pixels' wo differ
    gpu.close()


# ---- textures and bump maps -------------------------------------------------------------------------------------------------
def _write_pfm(path, rows):
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


def _render(binding, path):
    host = binding.HostScene(path=path)
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    gpu.close()
    return host.film_to_rgb(film).astype(np.float64)


def test_textured_materials_render_finite(binding, tmp_path):
    rng = np.random.default_rng(3)
    _write_pfm(tmp_path / "kd.pfm", rng.random((16, 16, 3)).astype(np.float32))
    _write_pfm(tmp_path / "ks.pfm", 0.2 * rng.random((16, 16, 3)).astype(np.float32))
    _write_pfm(tmp_path / "rough.pfm", (0.05 + 0.4 * rng.random((16, 16, 3))).astype(np.float32))
    tex = ('Texture "kd" "spectrum" "imagemap" "string filename" ["kd.pfm"]\nTexture "ks" "spectrum" "imagemap" "string filename" ["ks.pfm"]\n'
           'Texture "rough" "float" "imagemap" "string filename" ["rough.pfm"]\n')
    for i, line in enumerate(['Material "substrate" "texture Kd" "kd" "texture Ks" "ks"',
                              'Material "metal" "texture roughness" "rough"',
                              'Material "metal" "texture uroughness" "rough" "float vroughness" [0.1]',
                              'Material "substrate" "texture uroughness" "rough" "texture vroughness" "rough"']):
        rgb = _render(binding, _lit_plane(tmp_path, tex + line, spp=4, center=False, name=f"tex{i}.pbrt"))
        assert np.isfinite(rgb).all() and rgb.max() > 0, line


@pytest.mark.parametrize("plain, textured", [
    ('Material "substrate" "rgb Kd" [0.5 0.5 0.5] "rgb Ks" [0.5 0.5 0.5]', 'Material "substrate" "texture Kd" "half" "texture Ks" "half"'),
    ('Material "metal" "float roughness" [0.25]', 'Material "metal" "texture roughness" "quarter"'),
    ('Material "substrate" "float uroughness" [0.25] "float vroughness" [0.25]', 'Material "substrate" "texture uroughness" "quarter" "texture vroughness" "quarter"'),
])
def test_constant_image_texture_equals_constant(binding, tmp_path, plain, textured):
    _write_pfm(tmp_path / "half.pfm", np.full((8, 8, 3), 0.5, np.float32))
    _write_pfm(tmp_path / "quarter.pfm", np.full((8, 8, 3), 0.25, np.float32))
    tex = ('Texture "half" "spectrum" "imagemap" "string filename" ["half.pfm"]\n'
           'Texture "quarter" "float" "imagemap" "string filename" ["quarter.pfm"]\n')
    a = _render(binding, _lit_plane(tmp_path, plain, spp=4, center=False, name="plain.pbrt"))
    b = _render(binding, _lit_plane(tmp_path, tex + textured, spp=4, center=False, name="textured.pbrt"))
    assert a.max() > 0
    assert np.allclose(a, b, rtol=1e-5, atol=1e-6 * a.max()), np.abs(a - b).max()


@pytest.mark.parametrize("line", ['Material "metal" "float roughness" [0.2]', 'Material "substrate"'])
def test_zero_bump_map_equals_plain(binding, tmp_path, line):
    _write_pfm(tmp_path / "zero.pfm", np.zeros((4, 4, 3), np.float32))
    tex = 'Texture "zero" "float" "imagemap" "string filename" ["zero.pfm"]\n'
    a = _render(binding, _lit_plane(tmp_path, line, spp=4, center=False, name="plain.pbrt"))
    b = _render(binding, _lit_plane(tmp_path, tex + line + ' "texture bumpmap" "zero"', spp=4, center=False, name="bump.pbrt"))
    assert a.max() > 0
    assert np.allclose(a, b, rtol=1e-4, atol=1e-6 * a.max()), np.abs(a - b).max()


# ---- probe pass, IISPT frame, C++ host ---------------------------------------------------------------------------------------
def _room(integrator="path", spp=4, depth=3, w=32, h=32):
    body = ('LightSource "point" "rgb I" [10 10 10] "point from" [0 0 1.5]\nLightSource "infinite" "rgb L" [0.2 0.2 0.3]\n'
            'AttributeBegin\nMaterial "metal" "float uroughness" [0.1] "float vroughness" [0.3]\n' + PLANE + 'AttributeEnd\n'
            'AttributeBegin\nMaterial "substrate" "rgb Kd" [0.6 0.3 0.2]\nTranslate 0 0 0.6\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n'
            'AttributeBegin\nMaterial "metal" "rgb eta" [0.143 0.374 1.442] "rgb k" [3.983 2.385 1.603] "float roughness" [0.05]\n'
            'Translate 1.2 0.5 0.4\nShape "sphere" "float radius" [0.4]\nAttributeEnd\n')
    return dict(body=body, w=w, h=h, spp=spp, depth=depth, fov=50, eye="0 -4 2", look="0 0 0.3", up="0 0 1", integrator=integrator)


def test_probe_pass_is_finite_and_repeatable(binding, tmp_path):
    kw = _room(integrator="iispt")
    host = binding.HostScene(path=write_scene(tmp_path, kw.pop("body"), **kw))
    gpu = binding.GpuScene(host)
    pos, dirs = np.array([[0, -1, 0.01], [0.5, -0.5, 0.3]]), np.array([[0, 0, 1], [0, -0.6, 0.8]])
    a = gpu.render_probes(pos, dirs)
    b = gpu.render_probes(pos, dirs)
    for x, y in zip(a[:3], b[:3]):
        assert np.isfinite(x).all() and np.array_equal(x, y)
    assert a[0].max() > 0
    gpu.close()


def test_iispt_frame_is_finite_and_repeatable(binding, tmp_path):
    import importlib
    import sys
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    sys.path.insert(0, REPO)
    nn_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_nn")
    frame_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_frame")
    import iispt_torch_reference as ref_mod
    kw = _room(integrator="iispt", spp=1)
    host = binding.HostScene(path=write_scene(tmp_path, kw.pop("body"), **kw))
    images = []
    for _ in range(2):
        torch.manual_seed(5)
        gpu = binding.GpuScene(host)
        frame = frame_mod.IisptFrame(binding, gpu, nn_mod.IisptPipeline(gpu, net=ref_mod.IISPTNet().eval()))
        frame.run_batched(4, radius_start=8.0)
        frame.run_direct(8)
        torch.cuda.synchronize()
        assert frame.stats["probes"] > 0
        images.append(frame.image().cpu().numpy())
        gpu.close()
    assert np.isfinite(images[0]).all() and images[0].max() > 0
    assert np.array_equal(images[0], images[1])


def test_path_render_is_finite_and_repeatable(binding, tmp_path):
    kw = _room()
    path = write_scene(tmp_path, kw.pop("body"), **kw)
    a, b = _render(binding, path), _render(binding, path)
    assert np.isfinite(a).all() and a.max() > 0 and np.array_equal(a, b)


def test_cli_renders_the_binding_film(binding, tmp_path):
    """`iile_pbrt` (GpuPathIntegrator) renders the metal / substrate scene to the film the Python binding does, bit for bit."""
    kw = _room()
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
    assert (img.view(np.uint32) == want.view(np.uint32)).all()


def test_cli_iispt_integrator_writes_the_python_frames_image(binding, tmp_path):
    """`iile_pbrt` with the scene's `Integrator "iispt"` (GpuIisptIntegrator) renders the metal / substrate scene to the images the
    Python frame makes with the same network, schedule and direct passes: merged, indirect and direct, bit for bit."""
    import importlib
    import sys
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    sys.path.insert(0, REPO)
    nn_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_nn")
    frame_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_frame")
    import iispt_torch_reference as ref_mod
    n_tasks, n_direct = 4, 2
    kw = _room(integrator="iispt", spp=1)
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
    assert host.info["integrator"] == 1
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


def test_metal_alpha_zero_renders_finite(binding, tmp_path):
    """roughness 0 without remapping is alpha 0: the reference's arithmetic gives NaN there (D and the pdf are 0 / 0), and the
    render loop's radiance guards drop those samples; the film stays finite."""
    kw = _room()
    kw["body"] = kw["body"].replace('Material "metal" "float uroughness" [0.1] "float vroughness" [0.3]',
                                    'Material "metal" "bool remaproughness" "false" "float roughness" [0]')
    host = binding.HostScene(path=write_scene(tmp_path, kw.pop("body"), **kw))
    assert any(host.material(i).alpha == 0 for i in range(host.info["n_materials"]))
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    gpu.close()
    rgb = host.film_to_rgb(film)
    assert np.isfinite(film).all() and np.isfinite(rgb).all() and rgb.max() > 0
