"""The sampled lights held to the float64 truth of lightsample_ref.py without a GPU: the Distribution2D tables the host builds
for the infinite light; the oracle's shape_sample / shape_pdf / inf_sample_li / inf_pdf_li / inf_le through oracle_light_sample_at,
oracle_light_pdf_at and oracle_light_le (portable trigonometry, as the device evaluates them); the float32 restatement of the truth
against its float64 one, for every case the GPU tests use (the quadric ones too, which the oracle refuses); and properties that
do not depend on how the formulas were read: Pdf of what Sample returned, the solid angle, the normalisation of the infinite
light's pdf. Cases, samples and comparisons are lightsample_cases.py's, shared with test_gpu_light_sampling_truth.py."""
import numpy as np
import pytest

import lightsample_cases as C
import lightsample_ref as LS
from lightsample_cases import AREA, ZERO, _area_case, _packed, _pdf_directions, scenes  # noqa: F401  (scenes: the fixture)

U = LS.U


# ---- the host's tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", C.MAPS)
def test_host_tables_match_the_truth(scenes, which):
    """HostScene's env_dist against Table.build(scalar_image(MipMap of the same image file times L)): every row's func, cdf and
    funcInt, the marginal's, dist_w, dist_h and the layout, within lightsample_ref.table_bands."""
    host, light = scenes("infinite", f"{which}_z")
    got, want = light.table, light.own
    h0, w0 = light.mip.levels[0].shape[:2]
    assert (got.w, got.h) == (2 * w0, 2 * h0) == (want.w, want.h)
    assert got.flat.dtype == np.float32 and np.isfinite(got.flat).all()
    band = LS.table_bands(light.mip, light.img)
    worst = {}
    for name in ("func", "cdf", "func_int", "mfunc", "mcdf", "mfunc_int"):
        g, w, b = np.asarray(getattr(got, name), np.float64), np.asarray(getattr(want, name)), band[name]
        worst[name] = float(np.where(g == w, 0.0, np.abs(g - w) / np.maximum(b, 1e-300)).max())
    print(f"{which}: worst distance as a fraction of the band {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert (got.cdf[:, 0] == 0).all() and (got.cdf[:, -1] == 1).all() and got.mcdf[0] == 0 and got.mcdf[-1] == 1
    assert (np.diff(got.cdf, axis=1) >= 0).all() and (np.diff(got.mcdf) >= 0).all()
    if which == "black":  # funcInt == 0: cdf[i] = i / n, exactly
        assert (got.func == 0).all() and (got.func_int == 0).all() and got.mfunc_int == 0
        assert np.array_equal(got.cdf, np.broadcast_to(np.arange(got.w + 1, dtype=np.float32) / np.float32(got.w), got.cdf.shape))
        assert np.array_equal(got.mcdf, np.arange(got.h + 1, dtype=np.float32) / np.float32(got.h))
    else:
        assert got.mfunc_int > 0
    if which == "spike16x8":  # the black rows at the poles and the black column at the seam reach the table as flat stretches
        assert (got.func_int[[0, -1]] == 0).all() and (got.func[:, 0] < 1e-3 * got.func.max()).all()
    if which == "odd5x3":
        assert (w0, h0) == (8, 4)
    level = len(light.mip.levels) - 1 + np.log2(0.5 / min(got.w, got.h))  # Lookup(st, fwidth)'s level: above 0 for the 16 x 2 map only
    assert (level > 0) == (which == "wide16x2")


# ---- the oracle, function by function --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, case", AREA)
def test_oracle_area_light_matches_the_truth(scenes, oracle, kind, case):
    host, light, sets = _area_case(scenes, kind, case)
    for name, p, u in sets:
        want = light.sample_li(p.astype(np.float64), u)
        fig = C.check_area_sample(name, oracle.light_sample_at(host, 0, p, ZERO(p), u), want)
        wi = _pdf_directions(light, p, want, 5)
        figp = C.check_area_pdf(name, oracle.light_pdf_at(host, 0, p, ZERO(p), wi), light.pdf_li(p.astype(np.float64), wi.astype(np.float64)))
        print(f"oracle {name}: Sample_Li {fig}; Pdf_Li {figp}")
    if kind == "triangle":  # the reference point at p0 with u = (0, x): wi has no length; pdf 0 and black radiance, exactly
        out = oracle.light_sample_at(host, 0, p[:16], ZERO(p[:16]), u[:16])
        assert (u[:16, 0] == 0).all() and (out[:, 0:7] == 0).all() and np.array_equal(out[:, 7:10], p[:16])


@pytest.mark.parametrize("case", C.INFINITE)
def test_oracle_infinite_light_matches_the_truth(scenes, oracle, case):
    host, light = scenes("infinite", case)
    p, u = C.infinite_samples(light, 6)
    fig = C.check_infinite_sample(case, oracle.light_sample_at(host, 0, p, ZERO(p), u), light.sample_li(p.astype(np.float64), u))
    d = C.infinite_directions(light, 7)
    # +z and -z of the light are reached exactly under the rotation about z only: there sin theta == 0 and the pdf is exactly 0. Under
    # "tilt" WorldToLight of the float32 pole direction misses the pole by a rounding: those two directions are flagged (the band
    # of their cell reaches across the pole's row) and held by the candidate-cell check of check_infinite_pdf alone.
    if case.endswith("_z"):
        poles = d[-66:-64]
        assert np.array_equal(poles.astype(np.float64) @ light.w2l.T, [[0, 0, 1], [0, 0, -1]])
        assert (oracle.light_pdf_at(host, 0, poles, poles, poles) == 0).all()
    figp = C.check_infinite_pdf(case, oracle.light_pdf_at(host, 0, d, d, d), light.pdf_li(d.astype(np.float64)))
    figl = C.check_infinite_le(case, oracle.light_le(host, 0, d), light.le(d.astype(np.float64)))
    print(f"oracle {case}: Sample_Li {fig}; Pdf_Li {figp}; Le {figl}")


def test_oracle_refuses_what_it_does_not_restate(scenes, oracle):
    from oracle_binding import OracleUnsupported
    host, _ = scenes("quadric", "disk")
    p = np.zeros((1, 3), np.float32)
    with pytest.raises(OracleUnsupported):
        oracle.light_sample_at(host, 0, p, p, p[:, :2])
    with pytest.raises(OracleUnsupported):
        oracle.light_pdf_at(host, 0, p, p, p + 1)
    host, _ = scenes("sphere", "sphere")
    for call in (lambda: oracle.light_le(host, 0, p + 1), lambda: oracle.light_sample_at(host, 1, p, p, p[:, :2]),
                 lambda: oracle.light_pdf_at(host, -1, p, p, p + 1)):
        with pytest.raises(RuntimeError):
            call()


# ---- the bands and the caps, with the float32 restatement alone --------------------------------------------------------------------
@pytest.mark.parametrize("kind, case", AREA + [("quadric", c) for c in C.QUADRICS])
def test_float32_restatement_keeps_the_bands_and_caps_area(scenes, kind, case):
    host, light, sets = _area_case(scenes, kind, case)
    for name, p, u in sets:
        want = light.sample_li(p.astype(np.float64), u)
        fig = C.check_area_sample(name, _packed(light.sample_li(p, u, np.float32)), want)
        wi = _pdf_directions(light, p, want, 5)
        figp = C.check_area_pdf(name, light.pdf_li(p, wi, np.float32).pdf, light.pdf_li(p.astype(np.float64), wi.astype(np.float64)))
        print(f"float32 {name}: Sample_Li {fig}; Pdf_Li {figp}")


@pytest.mark.parametrize("case", C.INFINITE)
def test_float32_restatement_keeps_the_bands_and_caps_infinite(scenes, case):
    host, light = scenes("infinite", case)
    p, u = C.infinite_samples(light, 6)
    w32 = light.sample_li(p, u, np.float32)
    got = np.concatenate([w32.wi, w32.Li, w32.pdf[:, None], w32.target, np.zeros((len(u), 3))], 1)
    fig = C.check_infinite_sample(case, got, light.sample_li(p.astype(np.float64), u))
    d = C.infinite_directions(light, 7)
    figp = C.check_infinite_pdf(case, light.pdf_li(d, np.float32).pdf, light.pdf_li(d.astype(np.float64)))
    figl = C.check_infinite_le(case, light.le(d, np.float32).L, light.le(d.astype(np.float64)))
    print(f"float32 {case}: Sample_Li {fig}; Pdf_Li {figp}; Le {figl}")


# ---- properties that do not depend on our reading of the formulas ------------------------------------------------------------------
@pytest.mark.parametrize("kind, case", AREA)
def test_pdf_of_the_sampled_direction_is_the_sampled_pdf(scenes, oracle, kind, case):
    """Pdf_Li(ref, wi) of the wi Sample_Li returned equals the pdf it returned, within the two bands (samples flagged at an edge,
    or whose pdf has no band, are skipped; the caps on those hold in the tests above)."""
    host, light, sets = _area_case(scenes, kind, case)
    for name, p, u in sets:
        out = oracle.light_sample_at(host, 0, p, ZERO(p), u)
        live = out[:, 6] > 0
        wi = np.where(live[:, None], out[:, 0:3], np.float32([0, 0, 1]))
        pdf = oracle.light_pdf_at(host, 0, p, ZERO(p), wi).astype(np.float64)
        want, wantp = light.sample_li(p.astype(np.float64), u), light.pdf_li(p.astype(np.float64), wi.astype(np.float64))
        k = live & ~wantp.edge_flag & np.isfinite(wantp.band_pdf_rel) & np.isfinite(want.band_pdf_rel) & (wantp.pdf > 0)
        # (a partial sphere seen from inside: Sample draws over the whole sphere, and a point on the part that zmin, zmax and phimax
        #  cut away has Pdf = 0, as a point in a disk's hole has)
        assert k.mean() > (0.4 if name == "sphere_partial/inside" else 0.9)
        band = (want.band_pdf_rel[k] + wantp.band_pdf_rel[k]) * out[k, 6]
        frac = np.abs(pdf[k] - out[k, 6]) / band
        print(f"{name}: Pdf of the sampled direction, worst distance as a fraction of the two bands {frac.max():.3f}")
        assert (frac <= 1).all()


@pytest.mark.parametrize("case", C.QUADRICS)
def test_quadric_pdf_of_the_sampled_direction(scenes, case):
    """The same property on the truth itself (the oracle has no quadrics; the device is asked in the GPU test). The disk with a
    hole is the stated exception: Sample draws over the whole disk, and a point sampled in the hole or beyond phimax has Pdf = 0."""
    host, light, sets = _area_case(scenes, "quadric", case)
    _, p, u = sets[0]
    p = p.astype(np.float64)
    want = light.sample_li(p, u)
    live = want.pdf > 0
    wantp = light.pdf_li(p, np.where(live[:, None], want.wi, [0, 0, 1.0]))
    k = live & ~wantp.edge_flag
    if case == "disk":
        po = (want.p - light.shape.m[:3, 3]) @ light.shape.inv[:3, :3].T
        r = np.hypot(po[:, 0], po[:, 1])
        phi = np.mod(np.arctan2(po[:, 1], po[:, 0]), 2 * np.pi)
        hole = (r < light.shape.shape.inner) | (phi > light.shape.shape.phimax)
        assert 0.2 < hole.mean() < 0.5 and (wantp.pdf[k & hole] == 0).all()
        k &= ~hole
    else:  # the ray towards a point on a cylinder may meet the cylinder's other side first
        k &= np.abs(wantp.pdf - want.pdf) <= 1e-3 * want.pdf
        assert k.mean() > 0.4
    # (Sample goes through ObjectToWorld, Pdf's ray through WorldToObject: two float32 matrices that invert each other to 1e-7)
    k &= np.abs(want.cos) > 0.1
    assert k.sum() > 1000 and (np.abs(wantp.pdf[k] - want.pdf[k]) <= 1e-4 * want.pdf[k]).all()


def test_solid_angle_sphere(scenes, oracle):
    """The mean of 1 / pdf over u is the solid angle: the cap 2 Pi (1 - cosThetaMax) of a sphere seen from outside (every sample
    carries the same pdf), 4 Pi of the sphere around a point 0 or 0.5 r from its centre (five standard errors of the truth's own float64 samples)."""
    host, light = scenes("sphere", "sphere_two_sided")
    for q in (1.05, 2.0, 10.0):
        p, u, _ = C.sphere_points(light, (q,), 11, n=4000)
        pdf = oracle.light_sample_at(host, 0, p, ZERO(p), u)[:, 6].astype(np.float64)
        omega = light.shape.solid_angle(p.astype(np.float64))
        band = light.sample_li(p.astype(np.float64), u).band_pdf_rel
        assert (np.abs(1 / pdf - omega) <= band * omega).all()
    for q in (0.0, 0.5):  # (from 0.99 r the estimator's variance is too large to be measured from its own samples)
        p, u, _ = C.sphere_points(light, (q,), 12, n=20000)
        p[:] = p[0]
        pdf = oracle.light_sample_at(host, 0, p, ZERO(p), u)[:, 6].astype(np.float64)
        truth = 1 / light.sample_li(p.astype(np.float64), u).pdf
        se = truth.std(ddof=1) / np.sqrt(len(truth))
        print(f"sphere from d / r = {q}: mean 1 / pdf {np.mean(1 / pdf):.5f}, 4 Pi {4 * np.pi:.5f}, standard error {se:.5f}")
        assert abs(np.mean(1 / pdf) - 4 * np.pi) <= 5 * se + 1e-4


@pytest.mark.parametrize("case", ["tri", "tri_sliver", "tri_far", "tri_normals"])
def test_solid_angle_triangle(scenes, oracle, case):
    """Van Oosterom and Strackee's closed form against the mean of 1 / pdf, five standard errors of the truth's own samples."""
    host, light = scenes("triangle", case)
    pts, _ = C.triangle_points(light, 13)
    rng = np.random.default_rng(14)
    for i in (20, 21, 120, 121):  # two in front, two behind
        p = np.repeat(pts[i:i + 1], 20000, 0)
        u = rng.random((20000, 2)).astype(np.float32)
        pdf = oracle.light_sample_at(host, 0, p, ZERO(p), u)[:, 6].astype(np.float64)
        truth = 1 / light.sample_li(p.astype(np.float64), u).pdf
        se = truth.std(ddof=1) / np.sqrt(len(truth))
        omega = light.shape.solid_angle(p[:1].astype(np.float64))[0]
        print(f"{case} point {i}: mean 1 / pdf {np.mean(1 / pdf):.6f}, closed form {omega:.6f}, standard error {se:.6f}")
        assert (pdf > 0).all() and abs(np.mean(1 / pdf) - omega) <= 5 * se


@pytest.mark.parametrize("case", [c for c in C.INFINITE if not c.startswith("black")])
def test_infinite_pdf_integrates_to_one(scenes, oracle, case):
    """A quadrature of inf_pdf_li over the sphere of directions is 1: the pdf is constant over a cell of the table divided by sin
    theta, so a 4 x 4 midpoint rule per cell (no point on a cell border) of pdf sin theta is exact up to the pdf's own band."""
    host, light = scenes("infinite", case)
    t, k = light.table, 4
    th = (np.arange(t.h * k) + 0.5) * np.pi / (t.h * k)
    ph = (np.arange(t.w * k) + 0.5) * 2 * np.pi / (t.w * k)
    T, P = np.meshgrid(th, ph, indexing="ij")
    wl = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    d = (wl @ light.l2w.T).astype(np.float32)
    pdf = oracle.light_pdf_at(host, 0, d, d, d).astype(np.float64)
    want = light.pdf_li(d.astype(np.float64))
    assert not want.cell_flag.any()
    cell = (np.pi / (t.h * k)) * (2 * np.pi / (t.w * k))
    total = (pdf * np.sin(T).reshape(-1)).sum() * cell
    slack = (want.band_pdf_rel * want.pdf * np.sin(T).reshape(-1)).sum() * cell + 1e-6  # (the midpoint rule of sin theta / sin theta: exact)
    print(f"{case}: integral of the pdf {total:.7f} (band {slack:.2e})")
    assert abs(total - 1) <= slack
