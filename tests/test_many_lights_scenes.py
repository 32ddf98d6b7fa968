"""More than eight lights, without a GPU: what the loader hands over for an emissive mesh (every triangle a light, the powers of all
of them in light_power_all), what iile_scene_create's refusal pass says to such scenes before it touches a device, and the
restatement of lightdistrib_ref.py held against itself in float32 — the scenes of test_gpu_many_lights.py must leave a float32
evaluation inside the bands before a device is asked."""
import ctypes

import numpy as np
import pytest

import lightdistrib_ref as LD
import many_lights_scenes as MS

ERR_ARG, ERR_NO_DEVICE, ERR_UNSUPPORTED = 1, 2, 4
LIGHT_POINT, LIGHT_AREA_TRIANGLE = 1, 4


def _mesh_scene(tmp_path, strategy="power"):
    """A 5 x 2 panel (20 emitting triangles) between three point lights: 23 lights."""
    pts, idx = MS.panel_mesh(5, 2)
    points = [([-1, -1, 2], [1, 2, 3]), ([1, 0.5, 1], [0.5, 0.25, 2]), ([0, 1, 2.5], [3, 3, 3])]
    body = (MS.point_light(*points[0]) + MS.point_light(*points[1]) + MS.emitter(pts, idx, MS.PANEL_L) + MS.point_light(*points[2]) +
            'Material "matte"\n' + MS.quad(MS.PANEL_FLOOR))
    tris = [LD.Tri(*(pts[i] for i in idx[3 * t:3 * t + 3]), MS.PANEL_L) for t in range(20)]
    lights = [LD.Point(*points[0]), LD.Point(*points[1])] + tris + [LD.Point(*points[2])]
    return MS.write(tmp_path, body, strategy=strategy), lights


def test_emissive_mesh_loads_as_one_light_per_triangle(binding, tmp_path):
    path, lights = _mesh_scene(tmp_path)
    host = binding.HostScene(path=path)
    assert host.info["n_lights"] == 23 and host.light_count == 23
    power = host.light_power_all()
    want = np.array([lt.power() for lt in lights])
    assert power.dtype == np.float32 and power.shape == (23,)
    assert np.allclose(power, want, rtol=2e-6, atol=0), np.abs(power / want - 1).max()
    d = host.scene_desc()
    assert np.array_equal(power[:binding.MAX_LIGHTS], np.array(list(d.integrator.light_power), np.float32))
    # the lights stand in the order the scene declares them; every triangle and its light name each other
    prim_light = host.prim_light()
    _, tri_p, _ = host.bvh()
    seen = set()
    for i, lt in enumerate(lights):
        got = host.light(i)
        if isinstance(lt, LD.Point):
            assert got.type == LIGHT_POINT and np.array_equal(np.array(list(got.pos)), np.float32(lt.pos))
            continue
        assert got.type == LIGHT_AREA_TRIANGLE and 0 <= got.prim < len(prim_light) and prim_light[got.prim] == i
        assert np.array_equal(tri_p[got.prim].reshape(3, 3), np.float32(lt.p))
        seen.add(got.prim)
    assert len(seen) == 20 and sorted(np.flatnonzero(prim_light >= 0)) == sorted(seen)


def test_two_light_scene_has_all_powers_too(binding, tmp_path):
    body = MS.point_light([0, 0, 2], [1, 2, 3]) + MS.point_light([1, 0, 2], [2, 2, 2]) + 'Material "matte"\n' + MS.quad(MS.PANEL_FLOOR)
    host = binding.HostScene(path=MS.write(tmp_path, body))
    power = host.light_power_all()
    want = [LD.Point([0, 0, 2], [1, 2, 3]).power(), LD.Point([1, 0, 2], [2, 2, 2]).power()]
    assert np.allclose(power, want, rtol=2e-6, atol=0)
    assert np.array_equal(power, np.array(list(host.scene_desc().integrator.light_power), np.float32)[:2])


def _create(binding, desc):
    lib = binding.gpu_lib()
    out = ctypes.c_void_p()
    rc = lib.iile_scene_create(ctypes.addressof(desc), ctypes.byref(out))
    if rc == 0:
        lib.iile_scene_destroy(out)
    return rc, lib.iile_last_error().decode()


def _passes_the_refusals(rc):
    return rc in (0, ERR_NO_DEVICE)  # (without a device, what follows the refusal pass is "no HIP device")


def test_more_than_eight_lights_pass_the_refusals(binding, tmp_path):
    for strategy in ("spatial", "power", "uniform"):
        host = binding.HostScene(path=_mesh_scene(tmp_path, strategy)[0])
        rc, msg = _create(binding, host.scene_desc())
        assert _passes_the_refusals(rc), (strategy, rc, msg)


def test_power_strategy_needs_every_power(binding, tmp_path):
    host = binding.HostScene(path=_mesh_scene(tmp_path, "power")[0])
    d = host.scene_desc()
    d.light_power_all = None
    rc, msg = _create(binding, d)
    assert rc == ERR_ARG and "light_power_all" in msg, (rc, msg)
    for strategy in ("spatial", "uniform"):  # neither reads the powers
        host = binding.HostScene(path=_mesh_scene(tmp_path, strategy)[0])  # (alive while its tables are read)
        d = host.scene_desc()
        d.light_power_all = None
        assert _passes_the_refusals(_create(binding, d)[0]), strategy


def test_spatial_table_cap(binding, tmp_path):
    """1 100 emitting triangles in a cubic room: the spatial table would take 64^3 x 2 202 floats. Refused before any device call,
    with the way out in the message; the power strategy takes the scene; 511 lights are the most a full grid admits."""
    host = binding.HostScene(path=MS.room_with_panel(tmp_path, 25, 22, "spatial", "cap_spatial.pbrt"))
    assert host.info["n_lights"] == 1100
    rc, msg = _create(binding, host.scene_desc())
    assert rc == ERR_UNSUPPORTED, (rc, msg)
    assert "1100 lights" in msg and "64 x 64 x 64" in msg and "2202 MiB" in msg and '"power"' in msg and '"uniform"' in msg, msg
    host = binding.HostScene(path=MS.room_with_panel(tmp_path, 25, 22, "power", "cap_power.pbrt"))
    assert _passes_the_refusals(_create(binding, host.scene_desc())[0])
    body_511 = MS.point_light([0, 0, 1], [1, 1, 1])
    for n_tri, ok in ((510, True), (512, False)):  # + the point light below: 511 and 513 lights
        nx = n_tri // 2
        path = MS.room_with_panel(tmp_path, nx, 1, "spatial", f"cap_{n_tri}.pbrt")
        text = open(path).read().replace("WorldBegin\n", "WorldBegin\n" + body_511)
        open(path, "w").write(text)
        host = binding.HostScene(path=path)
        assert host.info["n_lights"] == n_tri + 1
        rc, msg = _create(binding, host.scene_desc())
        assert _passes_the_refusals(rc) == ok, (n_tri, rc, msg)


# ---- the restatement against itself ---------------------------------------------------------------------------------------------
MIXED = [(9, 11), (17, 12), (40, 13)]  # (lights, seed): the scenes of test_gpu_many_lights.py


def check_choice(scene, strategy, p, u, light, pdf, label):
    """What test_gpu_many_lights.py asks of iile_light_choose, asked of any evaluation: the pdf of the light it chose inside the
    truth's band for that light everywhere; the truth's light wherever u is not within the band of a cdf step; at most 2 % such
    lookups. Returns the share of undecided lookups and the largest share of a pdf band in use."""
    want, pdfs, undecided, bands = scene.choose(strategy, p, u)
    n = len(scene.lights)
    assert ((light >= 0) & (light < n)).all(), label
    rows = np.arange(len(u))
    truth_pdf, band = pdfs[rows, light], bands[rows, light]
    used = np.abs(pdf.astype(np.float64) - truth_pdf) / (band * truth_pdf)
    share = undecided.mean()
    print(f"{label}: undecided {share:.5f}, indices differing {np.mean(light != want):.5f}, pdf band in use {used.max():.3f}, "
          f"largest relative pdf band {band.max():.3e}")
    assert share <= 0.02, (label, share)
    assert (used <= 1).all(), (label, used.max())
    assert (light == want)[~undecided].all(), (label, np.flatnonzero((light != want) & ~undecided)[:5])
    return share, used.max()


@pytest.mark.parametrize("n, seed", MIXED)
@pytest.mark.parametrize("strategy", ["spatial", "power", "uniform"])
def test_float32_evaluation_stays_inside_the_bands(tmp_path, n, seed, strategy):
    """Measured (undecided share / pdf band in use): see DESIGN.md section 4.2, "Many lights"."""
    _, lights = MS.mixed_lights(n, seed)
    scene = LD.Scene(lights, *MS.BOUNDS)
    p, u, _ = MS.lookups(scene, 10000, seed)
    light, pdfs, _, _ = scene.choose(strategy, p, u, dtype=np.float32)
    check_choice(scene, strategy, p, u, light, pdfs[np.arange(len(u)), light], f"float32 on the CPU, {n} lights, {strategy}")


def test_restatement_basics():
    assert float(LD.radical_inverse(0, 5)) == 0.625
    assert float(LD.radical_inverse(0, 1)) == 0.5 and abs(float(LD.radical_inverse(1, 1)) - 1 / 3) < 1e-7 and abs(float(LD.radical_inverse(1, 5)) - (2 / 3 + 1 / 9)) < 1e-7
    scene = LD.Scene([LD.Point([0, 0, 1], [1, 1, 1]), LD.Point([1, 0, 1], [3, 3, 3])], *MS.BOUNDS)
    assert list(scene.nv) == [64, 64, 48]
    func, cdf, func_int, _, _ = scene.fixed("power")
    assert np.allclose(cdf, [0, 0.25, 1]) and np.isclose(func_int, func.mean())
    off, pdf = LD.sample_discrete(cdf, func, func_int, np.array([0.0, 0.2499, 0.25, 0.999]))
    assert list(off) == [0, 0, 1, 1] and np.allclose(pdf, [0.25, 0.25, 0.75, 0.75])
    # a unit square seen from a point on its axis at distance h: E = 4 atan-form; against the known value for h = 0.5
    sq = [[-0.5, -0.5, 0.5], [0.5, -0.5, 0.5], [0.5, 0.5, 0.5], [-0.5, 0.5, 0.5]]
    a = 0.5 / np.sqrt(0.5)
    assert np.isclose(LD.rect_irradiance(sq, [0, 0, 0], np.array([0, 0, 1.0])), 4 * a * np.arctan(a), rtol=1e-12)
