"""IISPT reference mode on the device: the many-sample probe pass (iile_render_probes_reference), the reference points
(iile_reference_points) and `iile_pbrt --reference=N` end to end. 32 x 32 hemispheres, at most 8 probes and 16 samples per test (one
test: 256 samples on 2 probes), on the small box room of boxroom.py and the closed can of quadric_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import boxroom
from quadric_ref import write_scene

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")

# four probes in the box room: under the light looking at it, on the floor, on the left wall, on the back wall
ROOM_POS = np.array([[1.5, -2, 3], [0, 0, -2.99], [-9.99, 0, 2], [0, 9.99, 2]], np.float32)
ROOM_DIR = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, -1, 0]], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def room_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("refmode") / "room.pbrt"
    p.write_text(boxroom.boxroom_pbrt(xres=32, yres=32, spp=1, ico_levels=2, n_blobs=4, wall_n=4))
    return str(p)


@pytest.fixture(scope="module")
def room(binding, room_file):
    host = binding.HostScene(path=room_file)
    gpu = binding.GpuScene(host)
    yield host, gpu
    gpu.close()
    host.close()


@pytest.fixture(scope="module")
def room16(room):
    """16 samples of the four probes in one call: shared, never written to."""
    return room[1].render_probes_reference(ROOM_POS, ROOM_DIR, 16)


def test_one_sample_is_the_probe_pass(room):
    _, gpu = room
    inten, nrm, dist, _ = gpu.render_probes(ROOM_POS, ROOM_DIR)
    i1, w1, n1, d1, st = gpu.render_probes_reference(ROOM_POS, ROOM_DIR, 1, max_depth=3, first_sample=0)
    assert inten.max() > 1 and (d1[0] > 0).any()   # (the first probe sees the light)
    assert np.array_equal(bits(i1), bits(inten)) and np.array_equal(bits(n1), bits(nrm)) and np.array_equal(bits(d1), bits(dist))
    assert (w1 > 0).all() and st["n_paths"] == 4 * 32 * 32


def test_repeatable_and_free_of_the_grouping(room, room16):
    _, gpu = room
    again = gpu.render_probes_reference(ROOM_POS, ROOM_DIR, 16)
    for a, b in zip(room16[:4], again[:4]):
        assert np.array_equal(bits(a), bits(b))
    assert room16[4]["n_passes"] == 1   # (all 16 samples in one set of launches)
    try:
        for group in (1, 5):   # one sample per set of launches; sets of 5, 5, 5, 1
            gpu.test_probe_ref_group(group)
            cut = gpu.render_probes_reference(ROOM_POS, ROOM_DIR, 16)
            assert cut[4]["n_passes"] == -(-16 // group)
            for a, b in zip(room16[:4], cut[:4]):
                assert np.array_equal(bits(a), bits(b)), group
    finally:
        gpu.test_probe_ref_group(0)


def test_sample_ranges_merge(room, room16):
    """c = samples [0, 16), a = [0, 8), b = [8, 16): c.I = (a.I a.W + b.I b.W) / (a.W + b.W), c.W = a.W + b.W. Every term is non-negative
    (Gaussian weights, radiance), so a float32 sum of at most about 16 x 25 of them is good to a few 1e-6 relative: rtol 1e-5."""
    _, gpu = room
    # (spp_total = 16: the three calls are ranges of one 16-sample image)
    ai, aw = gpu.render_probes_reference(ROOM_POS, ROOM_DIR, 8, first_sample=0, spp_total=16)[:2]
    bi, bw = gpu.render_probes_reference(ROOM_POS, ROOM_DIR, 8, first_sample=8, spp_total=16)[:2]
    ci, cw = room16[:2]
    aw64, bw64 = aw.astype(np.float64), bw.astype(np.float64)
    wsum = aw64 + bw64
    seen = wsum > 0
    assert (~seen).mean() < 0.01
    merged = (ai.astype(np.float64) * aw64[..., None] + bi.astype(np.float64) * bw64[..., None])[seen] / wsum[seen][:, None]
    rel_i = np.abs(ci[seen] - merged) / np.maximum(np.abs(merged), 1e-300)
    rel_w = np.abs(cw[seen] - wsum[seen]) / wsum[seen]
    print("merge: max relative error, intensity %.3g (where merged > 0), weight %.3g" % (rel_i[merged > 0].max(), rel_w.max()))
    np.testing.assert_allclose(cw[seen], wsum[seen], rtol=1e-5, atol=0)
    np.testing.assert_allclose(ci[seen], merged, rtol=1e-5, atol=0)
    assert not np.array_equal(bits(ai), bits(bi))


def _can(le, kd, depth):
    """The closed can of test_gpu_quadrics.py: two-sided emitting matte walls around the camera."""
    mat = f'Material "matte" "rgb Kd" [{kd} {kd} {kd}]\nAreaLightSource "diffuse" "rgb L" [{le} {le} {le}] "bool twosided" "true"\n'
    body = (mat + 'Shape "cylinder" "float radius" [1] "float zmin" [-1.05] "float zmax" [1.05]\n'
            'Shape "disk" "float height" [-1] "float radius" [1.05]\n'
            'Shape "disk" "float height" [1] "float radius" [1.05]\n')
    return dict(body=body, w=24, h=24, spp=16, depth=depth, fov=90, eye="0 0 0", look="0.3 0.2 1")


def test_furnace_at_depth(binding, tmp_path):
    """Probes inside the can: the camera ray's own vertex is left out (iispt_d.cpp:116-123), so a probe pixel sees
    L (a + a^2 + ... + a^maxdepth) — thirteen terms at max_depth 13, three at 3: the call's depth is the one that is used."""
    le, kd = 0.8, 0.6
    kw = _can(le, kd, 13)   # (the host sizes the Halton table from the scene's maxdepth)
    host = binding.HostScene(path=write_scene(tmp_path, kw.pop("body"), **kw))
    gpu = binding.GpuScene(host)
    pos, dirs = np.array([[0.1, -0.2, 0.3], [0, 0, -0.5]]), np.array([[0, 0, 1], [0.6, 0.8, 0]])
    for depth in (13, 3):
        inten, _, _, dist, _ = gpu.render_probes_reference(pos, dirs, 16, max_depth=depth)
        v = inten[..., 0].astype(np.float64)
        seen = dist > 0
        assert seen.mean() > 0.5
        want = le * sum(kd ** k for k in range(1, depth + 1))
        se = v[seen].std() / np.sqrt(seen.sum())
        print("furnace depth %d: mean %.6f want %.6f se %.3g" % (depth, v[seen].mean(), want, se))
        assert abs(v[seen].mean() - want) < 5 * se + 1e-4, (depth, v[seen].mean(), want, se)
    gpu.close()
    host.close()


def test_samples_differ_and_converge(room):
    _, gpu = room
    pos, dirs = ROOM_POS[1:3], ROOM_DIR[1:3]
    s0 = gpu.render_probes_reference(pos, dirs, 1, first_sample=0)[0]
    s1 = gpu.render_probes_reference(pos, dirs, 1, first_sample=1)[0]
    assert not np.array_equal(bits(s0), bits(s1))
    i16 = gpu.render_probes_reference(pos, dirs, 16)[0].astype(np.float64)
    i256 = gpu.render_probes_reference(pos, dirs, 256)[0].astype(np.float64)
    e1, e16 = (s0 - i256).std(), (i16 - i256).std()
    print("std of (1 - 256 samples) %.4g, of (16 - 256 samples) %.4g" % (e1, e16))
    assert e16 < 0.5 * e1   # (a quarter is expected; a half is what "every sample is sample 0" cannot reach)


def _check_points(host, gpu, pfilm):
    """valid == the camera ray hit; dir == +-n, against the ray; pos within 1e-3 of the hit point, on dir's side of it."""
    valid, pos, dr = gpu.reference_points(pfilm)
    o, d = gpu.camera_rays(pfilm)
    prim, tb, _ = gpu.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    hit = prim >= 0
    assert np.array_equal(valid != 0, hit)
    assert (pos[~hit] == 0).all() and (dr[~hit] == 0).all()
    _, tri_p, _ = host.bvh()
    flags = host.prim_flags()
    is_shape = (flags[np.maximum(prim, 0)] & 1) != 0
    n = np.zeros((len(o), 3))
    p = np.zeros((len(o), 3))
    t = hit & ~is_shape
    v = tri_p[prim[t]].astype(np.float64).reshape(-1, 3, 3)
    n[t] = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    p[t] = (tb[t][:, 1:4, None].astype(np.float64) * v).sum(axis=1)   # b0 v0 + b1 v1 + b2 v2
    s = hit & is_shape
    if s.any():
        a = gpu.shape_hit_attributes(o[s], d[s], prim[s])
        n[s], p[s] = a["n"], a["p"]
    n[hit] /= np.linalg.norm(n[hit], axis=1)[:, None]
    dd, dp = dr[hit].astype(np.float64), pos[hit].astype(np.float64)
    along = (dd * n[hit]).sum(axis=1)
    assert np.allclose(np.abs(along), 1, atol=1e-5) and np.allclose(dd, n[hit] * np.sign(along)[:, None], atol=1e-5)
    assert ((dd * d[hit]).sum(axis=1) <= 0).all()
    assert (np.linalg.norm(dp - p[hit], axis=1) < 1e-3).all()
    assert (((dp - p[hit]) * dd).sum(axis=1) >= 0).all()
    return valid, pos, dr, prim, s


def test_reference_points(binding, room, tmp_path):
    host, gpu = room
    rng = np.random.default_rng(7)
    pfilm = np.concatenate([rng.uniform(0, 32, (190, 2)), np.array([[x, y] for x in (0, 8, 16, 24, 31) for y in (0, 31)], float)]).astype(np.float32)
    assert len(pfilm) == 200
    valid, *_ = _check_points(host, gpu, pfilm)
    assert valid.sum() >= 150
    # a mirror in view: a 2 x 2 mirror at z = 0 facing the camera at z = -5, a matte wall behind the camera at z = -8 that the
    # reflection would reach, a matte sphere beside the mirror, nothing elsewhere
    body = ('Material "mirror"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0  1 -1 0  1 1 0  -1 1 0]\n'
            'Material "matte"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-20 -20 -8  20 -20 -8  20 20 -8  -20 20 -8]\n'
            'AttributeBegin\nTranslate 2 0 0\nShape "sphere" "float radius" [0.7]\nAttributeEnd\n'
            'LightSource "point" "point from" [0 0 -4]\n')
    mh = binding.HostScene(path=write_scene(tmp_path, body, w=32, h=32, spp=1, fov=60, eye="0 0 -5", look="0 0 0"))
    mg = binding.GpuScene(mh)
    grid = np.array([[x + 0.5, y + 0.5] for y in range(0, 32, 2) for x in range(0, 32, 2)], np.float32)
    valid, pos, dr, prim, on_shape = _check_points(mh, mg, grid)
    centre = (np.abs(grid - 16) < 3).all(axis=1)   # |x|, |y| < 0.55 on the mirror's plane: well inside the mirror
    assert centre.sum() >= 9 and valid[centre].all()
    assert np.allclose(pos[centre][:, 2], 0, atol=1e-3) and (pos[centre][:, 2] <= 0).all()   # on the mirror, not on the wall behind the camera
    assert np.allclose(dr[centre], [0, 0, -1], atol=1e-6)
    assert on_shape.any() and (~valid.astype(bool)).any()   # the sphere is hit; rays beside both leave the scene
    mg.close()
    mh.close()


def read_pfm(path):
    """A PFM of the reference mode as raster rows: the file's row j is raster row height - 1 - j."""
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = (int(x) for x in f.readline().split())
        assert float(f.readline()) < 0   # little endian
        c = {b"PF": 3, b"Pf": 1}[kind]
        a = np.frombuffer(f.read(), np.float32)
    assert a.size == w * h * c
    a = a.reshape(h, w, c)[::-1]
    return a[..., 0] if c == 1 else a


def test_cli_end_to_end(room, room_file, tmp_path):
    _, gpu = room
    env = {k: v for k, v in os.environ.items() if not k.startswith("IISPT_REFERENCE_CONTROL")}
    cmd = [EXE, room_file, "--reference=3", "--reference_samples=8"]
    p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    grid = [(x, y) for y in range(0, 32, 10) for x in range(0, 32, 10)]   # interval 32 / 3 = 10; 30 < 32 lets a fourth row and column in
    valid, pos, dr = gpu.reference_points(np.array(grid, np.float32))
    assert valid.sum() >= 12
    out = tmp_path / "out"
    names = {f"{k}_{x}_{y}.pfm" for (x, y), v in zip(grid, valid) if v for k in "dznp"} | {"train.json"}
    assert set(os.listdir(out)) == names
    assert (out / "train.json").read_text() == '{"normalization_intensity":0.0,"normalization_distance":0.0}'
    sel = valid != 0
    d1, _, n1, z1, _ = gpu.render_probes_reference(pos[sel], dr[sel], 1, max_depth=3)
    p8 = gpu.render_probes_reference(pos[sel], dr[sel], 8, max_depth=3)[0]
    for j, (x, y) in enumerate([g for g, v in zip(grid, valid) if v]):
        for kind, want in (("d", d1[j]), ("n", n1[j]), ("z", z1[j]), ("p", p8[j])):
            got = read_pfm(out / f"{kind}_{x}_{y}.pfm")
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (kind, x, y)
    # resume (the default): a second run rewrites nothing; with one p gone, that file alone comes back
    stamps = {n: os.stat(out / n).st_mtime_ns for n in names}
    for n in names:
        os.utime(out / n, ns=(1_000_000_000, 1_000_000_000))   # (so that a rewrite shows whatever the clock's resolution)
    p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert all(os.stat(out / n).st_mtime_ns == 1_000_000_000 for n in names), stamps
    x, y = next(g for g, v in zip(grid, valid) if v)
    gone = f"p_{x}_{y}.pfm"
    before = (out / gone).read_bytes()
    os.remove(out / gone)
    p = subprocess.run(cmd, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert (out / gone).read_bytes() == before
    assert all(os.stat(out / n).st_mtime_ns == 1_000_000_000 for n in names if n != gone)
    assert os.stat(out / gone).st_mtime_ns != 1_000_000_000
