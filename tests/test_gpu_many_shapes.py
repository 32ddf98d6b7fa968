"""More than 8 spheres, 64 materials and 1 024 quadrics on the device (GPU). A scene with more than 8 spheres runs the rare
(ALPHA) builds of the traversal kernels, whose leaf step tests shapes in two turns at the most: the wavefront's first shape from
SGPRs, then every remaining lane its own shape in one pass. Both turns call the same sphere_test / quadric_test, so every film,
ray and counter here is held to the CPU oracle bit for bit where the oracle loads the scene, and to the float64 restatement of
quadric_ref.py where it does not (disks and cylinders)."""
import os
import subprocess

import numpy as np
import pytest

import many_shapes_scenes as MS
from quadric_ref import Cylinder, Disk
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
# every counter of iile_stats the oracle keeps, device name -> oracle name
COUNTERS = (("camera_rays", "camera_rays"), ("closest_rays", "regular_rays"), ("shadow_rays", "shadow_rays"), ("tri_tests", "tri_tests"),
            ("tri_hits", "tri_hits"), ("sphere_tests", "sphere_tests"), ("nodes_closest", "nodes_closest"), ("nodes_any", "nodes_any"),
            ("nee_evals", "nee_evals"), ("zero_radiance", "zero_radiance"), ("path_length", "path_length"))
INF = np.float32(np.inf)


# ---- 1. films ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [None, "sobol"], ids=["halton", "sobol"])
@pytest.mark.parametrize("room", ["72", "9", "8"])
def test_room_film_bitwise(binding, oracle, tmp_path, room, sampler):
    """32 x 32, 4 spp, maxdepth 5: 72 spheres / 73 materials, 9 spheres (the first count the rare builds take) and 8 (the common
    builds still). Instrumented kernels with every counter, then the plain kernels."""
    a, b, c = {"72": MS.ROOM_72, "9": MS.ROOM_9, "8": MS.ROOM_8}[room]
    host = binding.HostScene(path=MS.room_file(tmp_path, a, b, c), sampler=sampler)
    assert host.info["n_spheres"] == a * b * c == int(room) and host.info["n_materials"] == a * b * c + 1
    gpu = binding.GpuScene(host)
    film, st = gpu.render(collect_stats=True)
    ref, ost = oracle.render(host)
    assert float(host.film_to_rgb(ref).mean()) > 1e-3 and ost["sphere_tests"] > 1000
    assert_bitwise(film, ref, f"room of {room} spheres: film, instrumented kernels")
    for k_dev, k_ref in COUNTERS:
        assert st[k_dev] == ost[k_ref], (k_dev, st[k_dev], ost[k_ref])
    plain, _ = gpu.render()
    assert_bitwise(plain, ref, f"room of {room} spheres: film, plain kernels")
    gpu.close()


# ---- 2. rays against the oracle -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud(binding, tmp_path_factory):
    body, centres = MS.cloud(256)
    host = binding.HostScene(path=MS.write(tmp_path_factory.mktemp("cloud"), body, name="cloud.pbrt"))
    assert host.info["n_spheres"] == 256 and host.info["n_triangles"] == 2
    gpu = binding.GpuScene(host)
    yield host, gpu, centres
    gpu.close()


def _cloud_rays(order, centres):
    rng = np.random.default_rng(11)
    if order == "different":   # ray i at sphere i: 64 distinct shapes in a wavefront
        return MS.aimed_rays(centres, rng, 0.06)
    if order == "same":        # 64 consecutive rays at one sphere
        return MS.aimed_rays(np.repeat(centres[[5, 77, 130, 255]], 64, axis=0), rng, 0.06)
    # a shuffle of sphere hits, floor hits between the spheres, and rays that leave upwards
    o, d = MS.aimed_rays(centres, rng, 0.06)
    kind = rng.integers(0, 3, len(o))
    floor = kind == 1
    tgt = np.concatenate([rng.uniform(-3, 3, (len(o), 2)), np.zeros((len(o), 1))], axis=1)
    o[floor] = (tgt[floor] + [0.05, 0.05, 0.1]).astype(np.float32)
    d[floor] = np.float32([0.0, 0.0, -1.0])
    d[kind == 2] *= np.float32(-1)
    perm = rng.permutation(len(o))
    return o[perm], d[perm]


@pytest.mark.parametrize("order", ["different", "same", "shuffled"])
def test_cloud_rays_bitwise(binding, cloud, oracle, order):
    """256 rays against 256 spheres over a floor; prim, (t, b0, b1, b2) and the any-hit answer of every ray, both kernel builds."""
    host, gpu, centres = cloud
    o, d = _cloud_rays(order, centres)
    assert len(o) == 256
    for tmax in (np.full(256, INF, np.float32), np.full(256, 6.05, np.float32)):
        rprim, rtb = oracle.intersect(host, o, d, tmax)
        rhit = oracle.intersect_p(host, o, d, tmax)
        if order == "shuffled" and np.isinf(tmax[0]):
            flags = host.prim_flags()
            on_sphere = (rprim >= 0) & ((flags[np.maximum(rprim, 0)] & binding.PRIM_SPHERE) != 0)
            assert on_sphere.sum() > 40 and ((rprim >= 0) & ~on_sphere).sum() > 40 and (rprim < 0).sum() > 40
        elif np.isinf(tmax[0]):
            assert (rprim >= 0).all() and len(np.unique(rprim)) >= (4 if order == "same" else 200)
        for instrumented in (True, False):
            prim, tb, _ = gpu.trace_closest(o, d, tmax, instrumented=instrumented)
            assert np.array_equal(prim, rprim), (order, instrumented, np.flatnonzero(prim != rprim)[:5])
            assert_bitwise(tb, rtb, f"cloud, {order}, instrumented {instrumented}: (t, b0, b1, b2)")
            hit, _ = gpu.trace_any(o, d, tmax, instrumented=instrumented)
            assert np.array_equal(hit, rhit), (order, instrumented)


# ---- 3. spheres, disks and cylinders in one wavefront ---------------------------------------------------------------------------------
def _shape_of_prim(binding, host, shapes):
    """Per primitive (BVH order): its index among `shapes` (declaration order)."""
    flags, (_, _, prim_shape) = host.prim_flags(), host.bvh()
    spheres = [i for i, s in enumerate(shapes) if isinstance(s, MS.Sphere)]
    quadrics = [i for i, s in enumerate(shapes) if isinstance(s, (Disk, Cylinder))]
    out = np.full(len(flags), -1)
    for p in range(len(flags)):
        if flags[p] & binding.PRIM_QUADRIC:
            out[p] = quadrics[prim_shape[p]]
        elif flags[p] & binding.PRIM_SPHERE:
            out[p] = spheres[prim_shape[p]]
    assert (out >= 0).all() and sorted(out) == list(range(len(shapes)))
    return out


def _check_against_restatement(binding, host, gpu, shapes, o, d, what):
    """Grouped order (64 consecutive rays at one shape) and a shuffle agree ray by ray, bit for bit; primitive and t meet the
    restatement on every ray it decides, and it decides at least 98 % of them."""
    n = len(o)
    tmax = np.full(n, INF, np.float32)
    nearest, want, certain, steep = MS.nearest_of(shapes, o, d)
    print(f"{what}: the restatement decides {certain.mean():.4f} of {n} rays, {np.isfinite(want).mean():.3f} of them hits")
    assert certain.mean() >= 0.98 and np.isfinite(want[certain]).mean() > 0.5
    perm = np.random.default_rng(17).permutation(n)
    of_prim = _shape_of_prim(binding, host, shapes)
    for instrumented in (False, True):
        prim, tb, _ = gpu.trace_closest(o, d, tmax, instrumented=instrumented)
        prim_s, tb_s, _ = gpu.trace_closest(o[perm], d[perm], tmax, instrumented=instrumented)
        assert np.array_equal(prim_s, prim[perm]) and np.array_equal(tb_s.view(np.uint32), tb[perm].view(np.uint32)), what
        hit_a, _ = gpu.trace_any(o, d, tmax, instrumented=instrumented)
        hit_s, _ = gpu.trace_any(o[perm], d[perm], tmax, instrumented=instrumented)
        assert np.array_equal(hit_s, hit_a[perm]) and np.array_equal(hit_a != 0, prim >= 0), what
        hit = prim >= 0
        assert (hit[certain] == np.isfinite(want[certain])).all(), (what, np.flatnonzero(certain & (hit != np.isfinite(want)))[:5])
        both = certain & hit
        assert (of_prim[prim[both]] == nearest[both]).all(), what
        assert np.allclose(tb[both & steep, 0], want[both & steep], rtol=1e-5, atol=0), what
    return prim, tb, certain & steep


def test_mixed_kinds_in_one_wave(binding, tmp_path):
    body, shapes = MS.mixed_kinds(12)
    host = binding.HostScene(path=MS.write(tmp_path, body, name="mixed_kinds.pbrt"))
    assert host.info["n_spheres"] == 12 and host.quadric_count == 24 and host.info["n_prims"] == 36
    gpu = binding.GpuScene(host)
    centres = np.array([s.c if isinstance(s, MS.Sphere) else s.m[:3, 3] for s in shapes])
    o, d = MS.aimed_rays(np.repeat(centres, 64, axis=0), np.random.default_rng(21), 0.3)
    prim, tb, steep = _check_against_restatement(binding, host, gpu, shapes, o, d, "12 spheres, 12 disks, 12 cylinders")
    # the hit point of iile_shape_hit_attributes (refined onto the surface, a few float32 roundings off it) against the ray at the
    # traced t, whatever the primitive's kind. The traced t may be off by the 1e-5 of itself admitted above, and moves o + t d by
    # as much (|d| = 1); evaluating o + t d in float32 adds an ulp of each term: 4 x 2^-24 of the largest coordinate
    sel = np.flatnonzero((prim >= 0) & steep)[::7]
    assert len(sel) > 100 and len(np.unique(prim[sel])) >= 30
    attr = gpu.shape_hit_attributes(o[sel], d[sel], prim[sel])
    on_ray = o[sel].astype(np.float64) + d[sel].astype(np.float64) * tb[sel, :1].astype(np.float64)
    off = np.abs(attr["p"] - on_ray).max(axis=1)
    bound = 1e-5 * tb[sel, 0] + 4 * 2.0 ** -24 * np.abs(o[sel]).max(axis=1)
    print(f"hit attributes: largest share of the bound in use {(off / bound).max():.3f}")
    assert (off <= bound).all(), (off / bound).max()
    gpu.close()


def test_field_of_1025_disks(binding, tmp_path):
    body, disks = MS.disk_field(1025)
    host = binding.HostScene(path=MS.write(tmp_path, body, name="disks_1025.pbrt"))
    assert host.quadric_count == 1025
    gpu = binding.GpuScene(host)
    centres = np.array([s.m[:3, 3] for s in disks])
    pick = np.random.default_rng(22).permutation(1025)[:32]
    pick[0] = 1024  # (the one disk past the old limit)
    o, d = MS.aimed_rays(np.repeat(centres[pick], 64, axis=0), np.random.default_rng(23), 0.09)
    _check_against_restatement(binding, host, gpu, disks, o, d, "1 025 disks")
    gpu.close()


# ---- 4. IISPT ---------------------------------------------------------------------------------------------------------------------
def test_iispt_direct_and_probe_bitwise(binding, oracle, tmp_path):
    host = binding.HostScene(path=MS.room_file(tmp_path, *MS.ROOM_72, w=16, h=16))
    gpu = binding.GpuScene(host)
    assert np.array_equal(gpu.render_direct(2).view(np.uint64), oracle.iispt_direct(host, 2).view(np.uint64))
    pos, direction = np.float32([[0.1, -2.0, 1.4]]), np.float32([[0.1, 1.0, 0.2]])
    inten, nrm, dist, _ = gpu.render_probes(pos, direction)
    oi, on, od = oracle.render_probe(host, pos[0], direction[0])
    assert oi.max() > 0 and (od > 0).mean() > 0.5
    assert_bitwise(inten[0], oi, "probe intensity")
    assert_bitwise(nrm[0], on, "probe normals")
    assert_bitwise(dist[0], od, "probe distances")
    gpu.close()


# ---- 5. the C++ host ----------------------------------------------------------------------------------------------------------------
def test_cli_renders_the_binding_film(binding, tmp_path):
    """`iile_pbrt` renders the 72-sphere file to the film the binding renders: the half-float EXR of the same RGB, bit for bit."""
    path = MS.room_file(tmp_path, *MS.ROOM_72)
    out = tmp_path / "cli.exr"
    p = subprocess.run([EXE, path, "--outfile", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    img = binding.read_image(str(out))
    host = binding.HostScene(path=path)
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    gpu.close()
    want = host.film_to_rgb(film).astype(np.float16).astype(np.float32)
    assert want.max() > 0
    assert_bitwise(img, want, "CLI image through OpenEXR")
