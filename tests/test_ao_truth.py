"""The float64 truth of the ambient occlusion integrator (ao_ref.py) against its closed forms, and the share of camera samples it
keeps on the scenes the GPU test uses (no GPU)."""
import numpy as np
import pytest

import ao_ref


def _quad_tris(half, y):
    a, b, c, d = (-half, y, -half), (half, y, -half), (half, y, half), (-half, y, half)
    return [a + b + c, a + c + d]


def _disk_tris(r, y, n=128):
    """A regular n-gon of the disk's area (so that its form factor is the disk's to the fourth order of 2 pi / n)."""
    rp = r / np.sqrt(np.sin(2 * np.pi / n) / (2 * np.pi / n))
    ang = 2 * np.pi * np.arange(n + 1) / n
    return [(0.0, y, 0.0, rp * np.cos(ang[i]), y, rp * np.sin(ang[i]), rp * np.cos(ang[i + 1]), y, rp * np.sin(ang[i + 1])) for i in range(n)]


def _down_rays(points):
    p = np.asarray(points, np.float64)
    return p + np.array([0, 5.0, 0]), np.broadcast_to(np.array([0, -1.0, 0]), p.shape).copy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_open_plane_is_pi(dtype):
    tri = np.array(_quad_tris(50, 0.0))
    rng = np.random.default_rng(5)
    o, d = _down_rays(np.column_stack([rng.uniform(-3, 3, 64), np.zeros(64), rng.uniform(-3, 3, 64)]))
    tr = ao_ref.li(tri, np.zeros(2, np.uint32), o, d, rng.uniform(0, 1, (64, 16, 2)), True, dtype)
    assert tr.hit.all() and tr.kept.mean() > 0.9
    assert np.abs(tr.L.astype(np.float64) - ao_ref.unoccluded()).max() < (1e-12 if dtype is np.float64 else ao_ref.BAND)
    # the sky: rays that miss return 0, and so does a ray turned away
    sky = ao_ref.li(tri, np.zeros(2, np.uint32), o, -d, rng.uniform(0, 1, (64, 16, 2)), True, dtype)
    assert not sky.hit.any() and (sky.L == 0).all()


@pytest.mark.parametrize("cossample", [True, False])
def test_disk_over_a_plane(cossample):
    h, r, n_s = 1.0, 0.6, 4096
    tri = np.array(_quad_tris(50, 0.0) + _disk_tris(r, h))
    rho = np.array([0.0, 0.3, 0.6, 0.9, 1.5, 2.5])
    pts = np.column_stack([rho, np.zeros(len(rho)), np.full(len(rho), 1e-3)])
    o = pts + np.array([6.0, 3.0, 0.0])   # seen from the side, above the plane: the camera rays pass clear of the disk
    d = pts - o
    rng = np.random.default_rng(11 + cossample)
    tr = ao_ref.li(tri, np.zeros(len(tri), np.uint32), o, d, rng.uniform(0, 1, (len(rho), n_s, 2)), cossample)
    assert tr.hit.all() and (tr.prim < 2).all()
    want = ao_ref.under_disk(h, np.hypot(pts[:, 0], pts[:, 2]), r)
    # per-ray terms lie in [0, pi] (cosine) or [0, 2 pi] (uniform): se of the mean of n_s of them
    se = (np.pi if cossample else 2 * np.pi) / 2 / np.sqrt(n_s)
    assert np.abs(tr.L - want).max() < 5 * se, (tr.L, want)
    assert abs((tr.L - want).mean()) < 5 * se / np.sqrt(len(rho)) + 1e-3
    assert tr.L[0] < tr.L[-1] and want[0] < 0.75 * np.pi < want[-1]   # (the factor matters: under the axis a quarter is hidden)


def test_reversed_orientation_keeps_the_hemisphere():
    """t is Cross(isect.n, s) with the normal that is not face-forwarded: flipping the surface's orientation mirrors the frame about
    s, and every wi stays in the hemisphere about the face-forwarded normal (so an open plane is pi either way)."""
    tri = np.array(_quad_tris(50, 0.0))
    o, d = _down_rays([[0.3, 0, 0.2]])
    u = np.random.default_rng(2).uniform(0, 1, (1, 16, 2))
    a = ao_ref.li(tri, np.zeros(2, np.uint32), o, d, u, True)
    b = ao_ref.li(tri, np.full(2, 8, np.uint32), o, d, u, True)
    assert abs(a.L[0] - np.pi) < 1e-12 and abs(b.L[0] - np.pi) < 1e-12
    P = tri.reshape(-1, 9)
    fa, fb = ao_ref.frames(P, np.zeros(2, np.uint32), np.array([0]), d, np.float64), ao_ref.frames(P, np.full(2, 8, np.uint32), np.array([0]), d, np.float64)
    assert np.allclose(fa[3], fb[3]) and np.allclose(fa[1], fb[1]) and np.allclose(fa[2], -fb[2])   # nf and s equal, t mirrored


@pytest.mark.parametrize("case", range(len(ao_ref.cases())), ids=[c[0] for c in ao_ref.cases()])
def test_kept_share_of_the_gpu_scenes(binding, oracle, tmp_path_factory, case):
    host, px, py, k, tr, _ = ao_ref.case_truth(binding, oracle, tmp_path_factory, case)
    assert len(px) == 16 * 16 * 2
    assert tr.kept.mean() >= 0.9, tr.kept.mean()
    assert 0.3 < tr.hit.mean() < 0.7
    hit = tr.hit & tr.kept
    # the scene occludes: some samples see the whole hemisphere, some lose part of it, none gains
    full = ao_ref.unoccluded() if ao_ref.cases()[case][1]["cossample"] else None
    if full is not None:
        assert (tr.L[hit] <= full + 1e-9).all() and (tr.L[hit] > full - 1e-9).any() and (tr.L[hit] < 0.8 * full).any()
    assert abs(tr.kept.mean() - ao_ref.MEASURED[ao_ref.cases()[case][0]][0]) < 5e-4
