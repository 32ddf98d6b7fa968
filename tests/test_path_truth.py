"""PathIntegrator::Li held to path_ref.py's float64 truth, vertex by vertex, on the scenes of path_cases.py: the truth against the
closed forms it can reach, its own caps, and the CPU oracle against it. No GPU.

The oracle's C ABI returns, per sample, L and the numbers of scene.Intersect and IntersectP calls ({regular, shadow}), not the vertex
count or the sampler dimension; the truth counts the same two calls as the reference makes them, and they are compared exactly:
a vertex more or less, a shadow or MIS ray traced or skipped changes them, and a dimension taken or skipped out of the reference's
order changes every later sample value, hence L far outside the band.

What path_ref.measure() printed is in path_ref's docstring; the oracle's worst distance in units of the band 4 B S is, per case,
between 0.165 (specular) and 0.910 (normals_quad_light_uniform), and 0.25 exactly where the oracle's float32 result on the sample
that sets B is the float32 mode's own to the last digit.

Mutations of oracle/oracle_path.cpp (a scratch copy, built outside the tree) and the first test here that fails for each: see
DESIGN.md section 2, "PathIntegrator::Li against a float64 truth".
"""
import numpy as np
import pytest

import path_cases
import path_ref as PR

CASES = list(path_cases.CASES)
KEPT_CAP = 0.9   # a cap on the truth alone, not a measurement: a case that misses it changes its scene


@pytest.fixture(scope="module")
def truth(binding, oracle, tmp_path_factory):
    return lambda name: PR.case_truth(binding, oracle, tmp_path_factory, name)


@pytest.mark.parametrize("name", CASES)
def test_case_is_small_and_live(truth, name):
    """At most 64 triangles, 16 x 16 pixels, 4 spp; kept >= 0.9; the branches the case is for are taken, on the truth alone."""
    host, px, py, k, tr, (scene, *_) = truth(name)
    assert len(scene.P) <= 64 and host.info["xres"] <= 16 and host.info["yres"] <= 16 and host.info["spp"] == 4
    assert len(px) == host.info["xres"] * host.info["yres"] * 4
    assert host.info["n_triangles"] == len(scene.P) and host.light_count == len(scene.lights) and host.info["max_depth"] == scene.max_depth
    print(f"{name}: kept {tr.kept.mean():.4f}, stats {tr.stats}, first flags by line {tr.why}")
    assert tr.kept.mean() >= KEPT_CAP, (name, tr.kept.mean(), tr.why)
    for what in path_cases.LIVE.get(name, ()):
        assert tr.stats.get(what, 0) > 0, (name, what, tr.stats)
    assert np.isclose(tr.kept.mean(), PR.MEASURED[name][0], atol=5e-5), name


def test_roulette_sides(truth):
    """rrthreshold 0 never enters the roulette and its paths run to maxdepth; 1 and 10 enter it from bounce 4 on."""
    tr0, tr1, tr10 = (truth(n)[4] for n in ("plain_room_rr0", "plain_room_d8", "plain_room_rr10"))
    assert not tr0.stats.get("rr_survived") and not tr0.stats.get("rr_died")
    assert tr0.nverts.max() == 9 and tr1.nverts.max() <= 9 and tr1.nverts.mean() < tr0.nverts.mean()
    assert tr10.stats["rr_died"] > 0 and tr10.stats["rr_survived"] > 0
    # the draw is taken only inside the test: without it the deepest path ends 8 x 7 dimensions behind the camera sample's five
    assert tr0.dim.max() == 5 + 8 * 7 and tr1.dim.max() > 5 + 8 * 7


def test_depth_0_and_1(truth):
    """maxdepth 0: Le at bounce 0 only, one ray, no sampler dimension taken; maxdepth 1: at most two vertices, Le never added twice."""
    _, _, _, _, tr, (scene, *_) = truth("plain_room_d0")
    L = scene.sphere["L"].astype(np.float64)
    assert (tr.n_regular == 1).all() and (tr.n_shadow == 0).all() and (tr.dim == 5).all()
    on = tr.L.any(1)
    assert 0 < on.sum() < len(on) and (tr.L[on] == L).all()
    tr1 = truth("plain_room_d1")[4]
    assert tr1.nverts.max() == 2 and (tr1.dim <= 12).all()
    assert (tr1.L[on] >= L).all() and np.array_equal(on, (tr1.L >= L).all(1))   # the sphere seen directly, plus what it reflects


def test_closed_white_box_at_depth_0():
    """A closed white matte box with an emitting quad, maxdepth 0: L is the emitter's radiance where the camera sees its front,
    0 elsewhere, exactly."""
    b = path_cases.Builder()
    white = path_cases.M("matte", Kd=(1, 1, 1))
    path_cases.room(b, (-2, 0, -2), (2, 3, 2), white)
    b.quad(path_cases.BLACK, (-1, 2.5, -1), (1, 2.5, -1), (1, 2.5, 1), (-1, 2.5, 1), emit=(3.0, 2.0, 1.0))   # faces down
    scene, _, _ = b.finish("0 1 -1.5", "0 2.5 0", 60, 0)
    rng = np.random.default_rng(7)
    n = 64
    o = np.tile(np.array([0, 1, -1.5], np.float32), (n, 1))
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tr = PR.li(scene, o, d, lambda i, dim: np.float32(0.5))
    t = (2.5 - 1) / d[:, 1].astype(np.float64)
    x, z = t * d[:, 0], -1.5 + t * d[:, 2]
    sees = (d[:, 1] > 0) & (np.abs(x) < 1) & (np.abs(z) < 1)
    assert 0 < sees.sum() < n
    assert (tr.L[sees] == np.array([3.0, 2.0, 1.0])).all() and not tr.L[~sees].any() and (tr.dim == 5).all()


def test_sphere_light_irradiance():
    """plain_room at maxdepth 1 with black walls and a matte floor: the mean of Li over the sampler's values at one floor point is
    Kd / Pi x the closed-form irradiance of a sphere of radiance L wholly above the horizon, L Pi (r / d)^2 cos(theta) (the one
    test_light_sampling_truth.py's solid angles integrate to). Both halves of EstimateDirect enter: each alone falls short."""
    scene, _, _ = path_cases.plain_room(1, black_walls=True)
    rng = np.random.default_rng(11)
    n = 600
    p = np.array([-0.75, -1.0, 1.5])
    eye = np.array([0.25, 1.5, 5.5])
    d = (p - eye) / np.linalg.norm(p - eye)
    u = rng.random((n, 16)).astype(np.float32)
    tr = PR.li(scene, np.tile(eye.astype(np.float32), (n, 1)), np.tile(d.astype(np.float32), (n, 1)), lambda i, dim: u[i, dim])
    c, r, L = scene.sphere["center"].astype(np.float64), float(scene.sphere["radius"]), scene.sphere["L"].astype(np.float64)
    w = c - p
    dist = np.linalg.norm(w)
    want = 0.5 / np.pi * L * np.pi * (r / dist) ** 2 * (w[1] / dist)
    mean, se = tr.L.mean(0), tr.L.std(0, ddof=1) / np.sqrt(n)
    print("sphere irradiance: mean", mean, "closed form", want, "standard error", se)
    assert (np.abs(mean - want) <= 5 * se).all() and (se < 0.05 * want).all()
    assert tr.stats["bsdf_half"] > 0 and (tr.n_shadow > 0).any()


@pytest.mark.parametrize("name", CASES)
def test_float32_mode_gives_the_band(binding, oracle, tmp_path_factory, truth, name):
    """B of the case, from the truth's own float32 mode against its float64 mode over the kept samples: what path_ref.MEASURED
    records, and what the band of the oracle and of the device is four times."""
    tr = truth(name)[4]
    B, t32 = PR.float32_distance(name, binding, oracle, tmp_path_factory)
    print(f"{name}: B {B:.3e} (recorded {PR.MEASURED[name][1]:.3e})")
    assert np.isfinite(t32.L).all() and (t32.L >= 0).all()
    assert np.array_equal(t32.n_regular, tr.n_regular) and np.array_equal(t32.n_shadow, tr.n_shadow) and np.array_equal(t32.dim, tr.dim)
    assert np.isclose(B, PR.MEASURED[name][1], rtol=2e-3, atol=1e-12), name


@pytest.mark.parametrize("name", CASES)
def test_oracle_li_matches_truth(oracle, truth, name):
    """Oracle.li against the truth: finite and non-negative everywhere; over the kept samples within 4 B S of the float64 L, with
    the reference's own numbers of Intersect and IntersectP calls."""
    host, px, py, k, tr, _ = truth(name)
    L, nr = oracle.li(host, px, py, k)
    assert np.isfinite(L).all() and (L >= 0).all() and np.isfinite(tr.L).all() and (tr.L >= 0).all()
    kept = tr.kept
    band = 4 * PR.MEASURED[name][1]
    rel = PR.rel_distance(L, tr)
    worst = int(np.argmax(np.where(kept, rel, -1)))
    print(f"{name}: oracle worst distance {rel[worst]:.3e} of S at sample {worst}, {rel[worst] / band if band else 0:.3f} of the band")
    assert np.array_equal(nr[kept, 0], tr.n_regular[kept]), (name, "scene.Intersect calls")
    assert np.array_equal(nr[kept, 1], tr.n_shadow[kept]), (name, "scene.IntersectP calls")
    assert (rel[kept] <= band).all(), (name, worst, rel[worst], band, L[worst], tr.L[worst])
