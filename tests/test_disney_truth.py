"""disney_ref.py, the numpy restatement of pbrt-v3's Disney material, checked for itself (CPU): each lobe's sampling density
integrates to the share of samples its Sample_f yields a direction for (1 for the cosine lobes), histograms of `sample` agree with
`sampling_density` (chi-square), the reflection lobes are reciprocal, the lobe lists are the material's, and the float32 mode stays
inside the device bands of test_gpu_disney.py with a factor 4 to spare on the very direction sets the GPU tests use."""
import numpy as np
import pytest

import disney_ref as D
from test_gpu_metal_substrate import _sphere_dirs
from test_gpu_translucent import N_DIRS, _chi2_pval, _direction_pairs, _hist

CASES = D.CASES
WO = {"default": (0.3, 0.2, 0.93), "metal": (0.5, -0.5, -0.707), "coated": (0.8, 0.1, 0.59), "glassy": (-0.6, 0.1, -0.79),
      "all_trans": (0.4, -0.3, 0.87), "thin_default": (0.2, 0.6, -0.77), "thin_all": (0.3, -0.2, 0.93), "rough1": (0.7, 0.2, 0.68),
      "black": (0.1, 0.1, 0.99), "gloss0": (-0.5, 0.4, 0.77)}


def test_lobe_lists():
    """The BxDFs each case's material adds, in order: no is-black test anywhere (a thin surface of flatness 0 carries its FakeSS lobe,
    a black colour every lobe), eight at the most."""
    want = {"default": "diffuse retro micro", "metal": "micro", "coated": "diffuse retro sheen micro coat",
            "glassy": "diffuse retro micro mtrans", "all_trans": "micro mtrans", "thin_default": "diffuse fakess retro micro ltrans",
            "thin_all": "diffuse fakess retro sheen micro coat mtrans ltrans", "rough0": "diffuse retro micro",
            "rough1": "diffuse retro micro", "black": "diffuse retro micro", "gloss0": "diffuse retro micro coat"}
    for case, lobes in want.items():
        b = D.Disney(**CASES[case])
        assert b.lobes == lobes.split(), case
    assert D.Disney(**CASES["thin_all"]).lobes == list(D.LOBES)
    assert not D.Disney(**CASES["thin_default"]).coef["fakess"].any()
    assert D.Disney(**CASES["rough0"]).ax == 0.001 and D.Disney(**CASES["black"]).cspec0[0] == pytest.approx(0.04)


def _sphere_grid(nt, nphi):
    c = -1 + 2 * (np.arange(nt) + 0.5) / nt
    p = ((np.arange(nphi) + 0.5) / nphi) * 2 * np.pi
    C, P = np.meshgrid(c, p, indexing="ij")
    s = np.sqrt(1 - C * C)
    return np.stack([s * np.cos(P), s * np.sin(P), C], -1).reshape(-1, 3), (2.0 / nt) * (2 * np.pi / nphi)


@pytest.mark.parametrize("case", [c for c in CASES if c != "rough0"])
def test_lobe_densities_integrate_to_the_yield(case):
    """Per lobe: the integral of its sampling density over the sphere (midpoint rule) is the share of its samples that come back
    with a direction — 1 for the cosine lobes and the clearcoat seen from above, less where a reflected direction leaves the
    hemisphere or a refraction is total. (rough0's microfacet peak is 0.001 wide: no grid resolves it; its sampling is held to
    the restatement's own float32 mode below and to the device's in test_gpu_disney.)"""
    b = D.Disney(**CASES[case])
    wo = np.array(WO[case], np.float64)
    wo /= np.linalg.norm(wo)
    dirs, dw = _sphere_grid(1024, 2048)
    n = 400_000
    rng = np.random.default_rng(5)
    won = np.repeat(wo[None], n, 0)
    for lobe in b.lobes:
        integral = (b.lobe_density(lobe, np.repeat(wo[None], len(dirs), 0), dirs) * dw).sum()
        _, p = b.sample_lobe(lobe, won, rng.random(n), rng.random(n))
        share = (p > 0).mean()
        if lobe in D.COSINE_LOBES or lobe == "ltrans":
            assert share == 1 and integral == pytest.approx(1, abs=2e-3), (lobe, integral)
        else:
            assert integral == pytest.approx(share, abs=4 * np.sqrt(share * (1 - share) / n) + 5e-3), (lobe, integral, share)
            assert share > 0.5, (lobe, share)


@pytest.mark.parametrize("case", ["default", "metal", "coated", "glassy", "all_trans", "thin_default", "thin_all", "rough1", "gloss0"])
def test_sample_histogram_matches_sampling_density(case):
    """BSDF::Sample_f's directions over 32 x 32 bins of the whole sphere, the samples with pdf 0 one more bin, against the counts
    sampling_density predicts (8 x 8 midpoint rule per bin): the thresholds of test_gpu_translucent.test_bsdf_sample_chi_square."""
    b = D.Disney(**CASES[case])
    n, nt, nphi, sub = 200_000, 32, 32, 8
    wo = np.array(WO[case], np.float64)
    wo /= np.linalg.norm(wo)
    rng = np.random.default_rng(11)
    wi, _, pdf = b.sample(np.repeat(wo[None], n, 0), rng.random(n), rng.random(n))
    ok = pdf > 0
    assert ok.mean() > 0.5
    observed = np.append(_hist(wi[ok], nt, nphi), (~ok).sum())
    dirs, dw = _sphere_grid(nt * sub, nphi * sub)
    dens = b.sampling_density(np.repeat(wo[None], len(dirs), 0), dirs)
    expected = (dens.reshape(nt, sub, nphi, sub) * dw).sum(axis=(1, 3)).reshape(-1) * n
    expected = np.append(expected, max(n - expected.sum(), 0.0))
    p = _chi2_pval(observed, expected)
    assert p > 1e-4, p


@pytest.mark.parametrize("case", list(CASES))
def test_reflection_lobes_are_reciprocal(case):
    """f(wo, wi) = f(wi, wo) for the six reflection lobes (the microfacet lobe's Fresnel term takes Dot(wi, wh) = Dot(wo, wh))."""
    b = D.Disney(**CASES[case])
    rng = np.random.default_rng(3)
    wo, wi = _sphere_dirs(rng, 20_000), _sphere_dirs(rng, 20_000)
    wi[:, 2] = np.abs(wi[:, 2]) * np.sign(wo[:, 2])
    keep = (np.abs(wo[:, 2]) > 0.05) & (np.abs(wi[:, 2]) > 0.05)
    wo, wi = wo[keep], wi[keep]
    for lobe in b.lobes:
        if lobe in D.REFLECTION_LOBES:
            a, c = b._f(lobe, wo, wi), b._f(lobe, wi, wo)
            assert np.allclose(a, c, rtol=1e-9, atol=1e-12 * np.abs(a).max()), lobe


def test_pdf_is_the_average_of_the_lobes_and_counts_the_cosine_once_per_lobe():
    b = D.Disney(**CASES["thin_all"])
    wo = np.array([[0.3, 0.1, 0.95]])
    wo /= np.linalg.norm(wo)
    wi = np.array([[-0.2, 0.4, 0.89]])
    wi /= np.linalg.norm(wi)
    cosine = abs(wi[0, 2]) / np.pi
    rest = b._pdf("micro", wo, wi)[0] + b._pdf("coat", wo, wi)[0]
    assert b.pdf(wo, wi)[0] == pytest.approx((4 * cosine + rest) / 8, rel=1e-12)
    assert b.pdf(wo, -wi)[0] == pytest.approx((b._pdf("mtrans", wo, -wi)[0] + cosine) / 8, rel=1e-12)


def test_path_ref_lobes():
    """lobes(dt) hands path_ref.BSDF scalar BxDFs that give the vectorised class's values, and a DisneyMaterial its statement."""
    import path_ref
    params = CASES["thin_all"]
    lobes, eta = D.lobes(np.float64, **params)
    assert eta == 1 and [lb.name for lb in lobes] == list(D.LOBES)
    ns, ss = np.array([0, 0, 1.0]), np.array([1.0, 0, 0])
    bsdf = path_ref.BSDF(lobes, ns, ns, ss, eta)
    b = D.Disney(**params)
    rng = np.random.default_rng(2)
    for _ in range(50):
        wo = _sphere_dirs(rng, 1)[0]
        u = rng.random(2).astype(np.float32).astype(np.float64)
        ctx = path_ref.Ctx(np.float64)
        wi, f, pdf, _ = bsdf.sample_f(wo, u, ctx, True)
        wi_v, f_v, pdf_v = b.sample(wo[None], u[0:1], u[1:2])
        assert pdf == pytest.approx(pdf_v[0], rel=1e-12)
        if pdf > 0:
            assert np.allclose(wi, wi_v[0], atol=1e-12) and np.allclose(f, f_v[0], rtol=1e-10)
            assert np.allclose(bsdf.f(wo, wi, ctx), b.f(wo[None], wi[None])[0], rtol=1e-10)
            assert bsdf.pdf(wo, wi, ctx) == pytest.approx(b.pdf(wo[None], wi[None])[0], rel=1e-10)
    m = D.DisneyMaterial(color=(.2, .5, .7), thin=True, clearcoat=.6)
    assert m.text() == 'Material "disney" "rgb color" [0.2 0.5 0.7] "bool thin" "true" "float clearcoat" [0.6]\n'
    assert [lb.name for lb in m.lobes(np.float32)[0]] == ["diffuse", "fakess", "retro", "micro", "coat", "ltrans"]


# ---- the float32 mode inside the device bands -------------------------------------------------------------------------------------
def float32_band_units(case):
    """f then pdf: (inner, outer) units outside disney_ref.peak_mask, (inner, outer) inside it — the float32 mode's worst error against
    the float64 mode in units of the device bands, on the eval test's direction pairs of test_gpu_disney (same generator and seed)."""
    p = CASES[case]
    b64, b32 = D.Disney(**p), D.Disney(dtype=np.float32, **p)
    wo, wi = _direction_pairs(np.random.default_rng(list(CASES).index(case)), N_DIRS)
    mask = D.peak_mask(b64, wo, wi)
    return D.band_units(b32.f(wo, wi), b64.f(wo, wi), mask) + D.band_units(b32.pdf(wo, wi), b64.pdf(wo, wi), mask)


@pytest.mark.parametrize("case", list(CASES))
def test_float32_mode_stays_inside_the_device_bands(case):
    """With a factor 4 to spare: the evidence that the bands of test_gpu_disney.py are wide enough for the formulas as such. Outside
    disney_ref.peak_mask (the pairs at the clearcoat's GTR1 peak, or at the peak of a microfacet lobe at the 0.001 clamp) the
    project's bands hold for every case. Inside it a band is 4 x the float32 mode's measured error where that exceeds a quarter of
    the project's (disney_ref.MEASURED, factor()), and this test holds the float32 mode to a quarter of the band in use."""
    units = float32_band_units(case)
    print(case, units)
    m = D.MEASURED[case]
    for i in (0, 1, 4, 5):
        assert units[i] <= 0.25, (case, "outside the mask", units)
    for i in (2, 3, 6, 7):
        assert units[i] <= D.factor(m[i]) / 4, (case, "inside the mask", units)
    if case not in ("coated", "thin_all", "rough0"):
        assert all(D.factor(m[i]) == 1 for i in (2, 3, 6, 7)), case


def float32_sampling_figures(case):
    """(share of samples with pdf > 0 in both modes, share disagreeing on pdf > 0, share of directions further than 1e-3 apart among
    the samples of disney_ref.azimuth_conditioned) of the float32 mode against the float64 one, on test_gpu_disney's wo and u of the sample
    test (the same generator and seed)."""
    p = CASES[case]
    b64, b32 = D.Disney(**p), D.Disney(dtype=np.float32, **p)
    rng = np.random.default_rng(100 + list(CASES).index(case))
    wo = _sphere_dirs(rng, 2 * N_DIRS)
    wo = wo[np.abs(wo[:, 2]) > 0.05][:N_DIRS].astype(np.float32)
    u = rng.random((len(wo), 2)).astype(np.float32)
    wi64, _, p64 = b64.sample(wo, u[:, 0], u[:, 1])
    wi32, _, p32 = b32.sample(wo, u[:, 0], u[:, 1])
    both = (p64 > 0) & (p32 > 0)
    sel = both & (np.abs(wi64[:, 2]) > 0.05) & D.azimuth_conditioned(b64, wo, u[:, 0])
    far = np.linalg.norm(wi32[sel].astype(np.float64) - wi64[sel], axis=1) >= 1e-3
    return float(both.mean()), float(((p64 > 0) != (p32 > 0)).mean()), float(far.mean())


@pytest.mark.parametrize("case", list(CASES))
def test_float32_sampling_agrees_with_float64(case):
    """The sample test's caps for the float32 mode against the float64 one, with a factor 4 to spare: more than half the samples
    with pdf > 0 in both, fewer than 1e-3 / 4 disagreeing on pdf > 0, directions further than 1e-3 apart for fewer than 1e-3 / 4 of
    the samples of disney_ref.azimuth_conditioned (those whose direction float32 can resolve at all: a bound worked out from wo, u0
    and the alphas alone; all but 6.6 % of rough0's samples and 0.15 % of any other case's)."""
    both, disagree, far = float32_sampling_figures(case)
    print(case, both, disagree, far)
    assert both > 0.5
    assert disagree < 1e-3 / 4
    assert far < 1e-3 / 4
    rng = np.random.default_rng(0)
    share = D.azimuth_conditioned(D.Disney(**CASES[case]), _sphere_dirs(rng, 100_000), rng.random(100_000)).mean()
    print(case, "azimuth_conditioned share", share)
    assert share > (0.93 if case == "rough0" else 0.998), share


# ---- the path cases' truth (disney_path_cases.py) --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["disney_room", "disney_thin"])
def test_path_cases_truth(binding, oracle, tmp_path_factory, name):
    """The float64 truth of the two Disney path cases on the CPU alone: the oracle's sample_index / sample_dimension / camera_rays
    accept a descriptor that holds Disney materials (they read its sampler and camera only), at least 0.9 of the samples are kept,
    nearly all are lit, and the float32 mode's distance B is the one MEASURED records (the device's band is 4 B S)."""
    import disney_path_cases as DPC
    host, px, py, k, tr, _ = DPC.case_truth(binding, oracle, tmp_path_factory, name)
    assert any(host.material(i).type == binding.MAT_DISNEY for i in range(host.info["n_materials"]))
    assert len(px) == 256 and tr.kept.mean() >= 0.9 and np.isfinite(tr.L).all()
    assert (tr.L.max(1) > 0).mean() > 0.9 and tr.nverts.mean() > 3
    B, t32 = DPC.float32_distance(name, binding, oracle, tmp_path_factory)
    kept_share, B_recorded = DPC.MEASURED[name]
    assert abs(tr.kept.mean() - kept_share) < 1e-3 and B <= 1.05 * B_recorded and B >= B_recorded / 2, (tr.kept.mean(), B)
