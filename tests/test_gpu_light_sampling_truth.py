"""The sampled lights on the device (GPU), function by function through the probes iile_light_sample_at, iile_light_pdf_at and
iile_light_le (which call the dlight.h functions the render kernels call), held to the float64 truth of lightsample_ref.py within
its bands and caps and, where the oracle has the function, to the oracle bit for bit. Cases, samples and comparisons are
lightsample_cases.py's, shared with test_light_sampling_truth.py, which checks on the CPU that every case keeps inside the bands
and the caps. One end-to-end check of the lines of estimate_direct_request that join them, against a closed form."""
import numpy as np
import pytest

import lightsample_cases as C
import lightsample_ref as LS
from test_image_light_scenes import write_scene
from lightsample_cases import AREA, ZERO, _area_case, _pdf_directions, scenes  # noqa: F401  (scenes: the fixture)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def devices(binding, scenes):
    """gpu(kind, case) -> (HostScene, truth light, GpuScene), each device scene created once and closed at the end."""
    cache = {}

    def gpu(kind, case):
        if (kind, case) not in cache:
            host, light = scenes(kind, case)
            cache[kind, case] = (host, light, binding.GpuScene(host))
        return cache[kind, case]
    yield gpu
    for _, _, g in cache.values():
        g.close()


@pytest.mark.parametrize("kind, case", AREA + [("quadric", c) for c in C.QUADRICS])
def test_device_area_light_matches_the_truth(devices, scenes, oracle, kind, case):
    """Sample_Li (wi, Li, pdf, the sampled point and its normal) and Pdf_Li of a sphere, triangle, disk or cylinder emitter
    within the truth's bands and caps; sphere and triangle also bit for bit the oracle's; and Pdf_Li of the direction Sample_Li
    returned against the pdf it returned, within the two bands."""
    host, light, gpu = devices(kind, case)
    _, _, sets = _area_case(scenes, kind, case)
    for name, p, u in sets:
        want = light.sample_li(p.astype(np.float64), u)
        out = gpu.light_sample_at(0, p, ZERO(p), u)
        fig = C.check_area_sample(name, out, want)
        wi = _pdf_directions(light, p, want, 5)
        pdf = gpu.light_pdf_at(0, p, ZERO(p), wi)
        figp = C.check_area_pdf(name, pdf, light.pdf_li(p.astype(np.float64), wi.astype(np.float64)))
        print(f"device {name}: Sample_Li {fig}; Pdf_Li {figp}")
        if kind != "quadric":
            assert np.array_equal(_bits(out), _bits(oracle.light_sample_at(host, 0, p, ZERO(p), u))), name
            assert np.array_equal(_bits(pdf), _bits(oracle.light_pdf_at(host, 0, p, ZERO(p), wi))), name
        # a normal on the reference point changes nothing: pError = 0, so no ray origin is offset
        nrm = C._dirs(np.random.default_rng(8), len(p)).astype(np.float32)
        assert np.array_equal(_bits(gpu.light_sample_at(0, p, nrm, u)), _bits(out)), name
        # consistency: Pdf of the sampled direction
        live = out[:, 6] > 0
        back = gpu.light_pdf_at(0, p, ZERO(p), np.where(live[:, None], out[:, 0:3], np.float32([0, 0, 1]))).astype(np.float64)
        wantp = light.pdf_li(p.astype(np.float64), np.where(live[:, None], out[:, 0:3], np.float32([0, 0, 1])).astype(np.float64))
        k = live & ~wantp.edge_flag & np.isfinite(wantp.band_pdf_rel) & np.isfinite(want.band_pdf_rel) & (wantp.pdf > 0)
        if kind == "quadric":  # a cylinder's other side may come first along the ray: there the two are different points
            k &= np.abs(wantp.pdf - want.pdf) <= 1e-3 * want.pdf
        assert k.sum() > 1000
        frac = np.abs(back[k] - out[k, 6]) / ((want.band_pdf_rel[k] + wantp.band_pdf_rel[k]) * out[k, 6])
        print(f"device {name}: Pdf of the sampled direction, worst distance as a fraction of the two bands {frac.max():.3f}")
        assert (frac <= 1).all(), name
    if kind == "triangle":  # the reference point at p0 with u = (0, x): wi has no length; pdf 0 and black radiance, exactly
        assert (u[:16, 0] == 0).all() and (out[:16, 0:7] == 0).all() and np.array_equal(out[:16, 7:10], p[:16])
    if case == "disk":  # Sample ignores innerradius and phimax: points in the hole are sampled, and their Pdf is 0
        po = (out[:, 7:10].astype(np.float64) - light.shape.m[:3, 3]) @ light.shape.inv[:3, :3].T
        r, phi = np.hypot(po[:, 0], po[:, 1]), np.mod(np.arctan2(po[:, 1], po[:, 0]), 2 * np.pi)
        hole = ((r < 0.29) | (phi > light.shape.shape.phimax + 0.01)) & live
        assert hole.mean() > 0.2 and (back[hole & ~wantp.edge_flag] == 0).all()


def test_device_sphere_far_away_is_the_oracles(devices, oracle):
    """d / r = 1000: 1 - cosThetaMax is 5e-7, of which float32 keeps about three bits (the band k u / (1 - cosThetaMax) is 0.18 of
    the pdf there, by the reference's own arithmetic): no comparison with the truth says anything, so the device is held to the
    oracle alone, bit for bit."""
    host, light, gpu = devices("sphere", "sphere")
    p, u, _ = C.sphere_points(light, (1000.0,), 9, n=4000)
    out = gpu.light_sample_at(0, p, ZERO(p), u)
    assert np.isfinite(out).all() and (out[:, 6] > 0).all()
    assert np.array_equal(_bits(out), _bits(oracle.light_sample_at(host, 0, p, ZERO(p), u)))
    wi = out[:, 0:3]
    assert np.array_equal(_bits(gpu.light_pdf_at(0, p, ZERO(p), wi)), _bits(oracle.light_pdf_at(host, 0, p, ZERO(p), wi)))
    assert light.sample_li(p.astype(np.float64), u).band_pdf_rel.min() > 0.1


@pytest.mark.parametrize("case", C.INFINITE)
def test_device_infinite_light_matches_the_truth(devices, oracle, case):
    """Sample_Li (nothing left out: the direction pins (d0, d1), the pdf pins the row and the column), Pdf_Li (the cell index
    flagged within its band) and Le, within the truth's bands; all three bit for bit the oracle's."""
    host, light, gpu = devices("infinite", case)
    p, u = C.infinite_samples(light, 6)
    out = gpu.light_sample_at(0, p, ZERO(p), u)
    fig = C.check_infinite_sample(case, out, light.sample_li(p.astype(np.float64), u))
    d = C.infinite_directions(light, 7)
    pdf, le = gpu.light_pdf_at(0, d, d, d), gpu.light_le(0, d)
    # +z and -z of the light are reached exactly under the rotation about z only: there sin theta == 0 and the pdf is exactly 0. Under
    # "tilt" WorldToLight of the float32 pole direction misses the pole by a rounding: those two directions are flagged (the band
    # of their cell reaches across the pole's row) and held by the candidate-cell check of check_infinite_pdf alone.
    if case.endswith("_z"):
        assert np.array_equal(d[-66:-64].astype(np.float64) @ light.w2l.T, [[0, 0, 1], [0, 0, -1]]) and (pdf[-66:-64] == 0).all()
    figp = C.check_infinite_pdf(case, pdf, light.pdf_li(d.astype(np.float64)))
    figl = C.check_infinite_le(case, le, light.le(d.astype(np.float64)))
    print(f"device {case}: Sample_Li {fig}; Pdf_Li {figp}; Le {figl}")
    assert np.array_equal(_bits(out), _bits(oracle.light_sample_at(host, 0, p, ZERO(p), u)))
    assert np.array_equal(_bits(pdf), _bits(oracle.light_pdf_at(host, 0, d, d, d)))
    assert np.array_equal(_bits(le), _bits(oracle.light_le(host, 0, d)))


def test_probes_refuse_other_lights_and_bad_arguments(binding, tmp_path):
    body = ('LightSource "point" "rgb I" [1 2 3] "point from" [0 0 2]\nLightSource "infinite" "rgb L" [1 1 1]\nMaterial "matte"\n' + C.FLOOR)
    gpu = binding.GpuScene(binding.HostScene(path=write_scene(tmp_path, body)))
    p = np.array([[0, 0, 1], [0.6, 0, 0.8]], np.float32)
    assert np.allclose(gpu.light_le(1, p), 1) and gpu.light_sample_at(1, p, p, p[:, :2]).shape == (2, 13) and gpu.light_pdf_at(1, p, p, p).shape == (2,)
    for light in (0, 2, -1):  # a delta light, and no light at all
        for call, name in ((lambda: gpu.light_sample_at(light, p, p, p[:, :2]), "iile_light_sample_at"),
                           (lambda: gpu.light_pdf_at(light, p, p, p), "iile_light_pdf_at"), (lambda: gpu.light_le(light, p), "iile_light_le")):
            with pytest.raises(RuntimeError, match=name):
                call()
    gpu.close()
    body = C.sphere_scene("sphere").split("WorldBegin\n", 1)[1].rsplit("WorldEnd", 1)[0]
    gpu = binding.GpuScene(binding.HostScene(path=write_scene(tmp_path, body, name="area.pbrt")))
    with pytest.raises(RuntimeError, match="iile_light_le"):  # Le is the infinite light's alone
        gpu.light_le(0, p)
    gpu.close()


# ---- the joining lines of estimate_direct_request, once, against a closed form ------------------------------------------------------
KD, L_SPHERE, R_SPHERE, CENTRE = 0.5, np.array([30.0, 20.0, 10.0]), 0.5, np.array([0.25, 0.5, 2.0])
SPP = 1024


def _closed_form_scene(tmp_path, integrator):
    body = (f'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [{L_SPHERE[0]} {L_SPHERE[1]} {L_SPHERE[2]}]\n'
            f'Translate {CENTRE[0]} {CENTRE[1]} {CENTRE[2]}\nShape "sphere" "float radius" [{R_SPHERE}]\nAttributeEnd\n'
            'Material "matte"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-50 -50 0  50 -50 0  50 50 0  -50 50 0]\n')
    # a camera far away with a very narrow view: a pixel covers 0.01 of the plane, over which the radiance changes by 1e-4 of itself
    return write_scene(tmp_path, body, name=f"closed_{integrator}.pbrt", w=2, h=2, spp=SPP, depth=1, fov=0.1, eye="1.5 -9 6", look="1.5 0.8 0",
                       integrator=integrator, center=False)


def _closed_form(gpu):
    """Kd L (r / d)^2 cos(theta) of the fully visible sphere at the plane point each of the four pixels sees (its centre), and
    the light-sampling estimator's standard error there for SPP samples, from the truth's own float64 samples."""
    o, d = gpu.camera_rays(np.array([[0.5, 0.5], [1.5, 0.5], [0.5, 1.5], [1.5, 1.5]]))
    o, d = o.astype(np.float64), d.astype(np.float64)
    x = o + (-o[:, 2] / d[:, 2])[:, None] * d
    to = CENTRE[None, :] - x
    dist = np.linalg.norm(to, axis=1)
    assert (np.degrees(np.arcsin(R_SPHERE / dist)) < np.degrees(np.arcsin(to[:, 2] / dist))).all()  # wholly above the horizon
    want = KD * L_SPHERE[None, :] * ((R_SPHERE / dist) ** 2 * to[:, 2] / dist)[:, None]
    light = LS.AreaLight(LS.Sphere(np.block([[np.eye(3), CENTRE[:, None]], [np.zeros((1, 3)), 1]]),
                                   np.block([[np.eye(3), -CENTRE[:, None]], [np.zeros((1, 3)), 1]]), R_SPHERE), L_SPHERE)
    rng = np.random.default_rng(10)
    se = np.zeros(4)
    for i in range(4):
        s = light.sample_li(np.repeat(x[i:i + 1], 20000, 0), rng.random((20000, 2)))
        v = (KD / np.pi) * s.Li[:, 0] * np.maximum(s.wi[:, 2], 0) / s.pdf
        assert abs(v.mean() / want[i, 0] - 1) < 5 * v.std() / np.sqrt(len(v)) / want[i, 0] + 1e-12  # the estimator means the closed form
        se[i] = v.std(ddof=1) / np.sqrt(SPP) / want[i, 0]
    assert (se <= 0.01).all(), se
    return want, se


def test_sphere_light_over_a_plane_is_the_closed_form(binding, tmp_path):
    """A fully visible sphere light over a matte plane at maxdepth 1, through the path integrator and the IISPT direct pass: four
    pixels against Kd L (r / d)^2 cos(theta), within five standard errors of the truth's own light-sampling estimator."""
    host = binding.HostScene(path=_closed_form_scene(tmp_path, "path"))
    gpu = binding.GpuScene(host)
    want, se = _closed_form(gpu)
    rgb = host.film_to_rgb(gpu.render()[0]).astype(np.float64).reshape(4, 3)
    gpu.close()
    host = binding.HostScene(path=_closed_form_scene(tmp_path, "iispt"))
    gpu = binding.GpuScene(host)
    mon = gpu.render_direct(SPP)
    gpu.close()
    direct = (mon[..., :3] / mon[..., 3:4]).reshape(4, 3)
    for name, got in (("path", rgb), ("direct pass", direct)):
        dev = np.abs(got / want - 1).max(axis=1)
        print(f"{name}: |film / closed form - 1| per pixel {dev}, standard error {se}")
        assert np.isfinite(got).all() and (dev <= 5 * se).all(), (name, dev, se)


def test_black_infinite_light_leaves_the_film_finite(binding, oracle, tmp_path):
    """An infinite light of no radiance beside a point light: Distribution2D::Pdf is 0 / 0 for it in the reference, whose
    EstimateDirect then drops the term because Le is black; inf_pdf_li returns 0 instead, on the device and in the oracle, and the
    film is the oracle's bit for bit, finite, and lit by the point light."""
    import oracle_binding
    body = ('LightSource "infinite" "rgb L" [0 0 0]\nLightSource "point" "rgb I" [8 6 4] "point from" [0.5 -1 3]\n'
            'Material "matte"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-5 -5 0  5 -5 0  5 5 0  -5 5 0]\n'
            'AttributeBegin\nMaterial "plastic"\nTranslate 0 0 0.6\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n')
    host = binding.HostScene(path=write_scene(tmp_path, body, name="black.pbrt", w=16, h=16, spp=4, depth=3, strategy="uniform"))
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    gpu.close()
    ref, _ = oracle.render(host, trig_mode=oracle_binding.TRIG_PORTABLE)
    assert np.isfinite(film).all() and film[..., :3].max() > 0
    assert np.array_equal(_bits(film), _bits(ref))
