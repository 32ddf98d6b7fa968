"""The device traversal kernels against the tree-free ground truth of trace_ref.py, on the cases of trace_scenes.py (the smallest
trees at which the LDS copy of the tree's top, the ring-to-HBM stack and the persistent waves' refill can go wrong), and bit for
bit against the oracle as the other parity tests have it. instrumented=True runs the binary steps, False the four-wide steps with
the LDS top: the kernels the renders run."""
import numpy as np
import pytest

import trace_ref
import trace_scenes as ts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def limits(binding):
    return binding.traversal_limits()


def _bits(prim, tb):
    return np.concatenate([np.asarray(prim, np.int32)[:, None].view(np.uint32), np.ascontiguousarray(tb, np.float32).view(np.uint32)], 1)


def _check_device(binding, oracle, c, scene, what):
    """trace_closest / trace_any of both kernel builds on the case's rays: the ground truth's answers on the decided rays, the oracle's bits on all."""
    gpu = binding.GpuScene(scene)
    tri_p = scene.bvh()[1]
    rprim, rtb = oracle.intersect(scene, c.o, c.d, c.tmax)
    rany = oracle.intersect_p(scene, c.o, c.d, c.tmax)
    for instrumented in (True, False):
        w = f"{what}, instrumented={instrumented}"
        prim, tb, _ = gpu.trace_closest(c.o, c.d, c.tmax, instrumented=instrumented)
        ts.check_closest(c, tri_p, prim, tb[:, 0], f"trace_closest, {w}")
        hit, _ = gpu.trace_any(c.o, c.d, c.tmax, instrumented=instrumented)
        ts.check_any(c, hit, f"trace_any, {w}")
        diff = (_bits(prim, tb) != _bits(rprim, rtb)).any(1)
        assert not diff.any(), f"{w}: {int(diff.sum())} closest hits differ from the oracle's bits, first ray {int(np.nonzero(diff)[0][0])}"
        assert np.array_equal(hit, rany), f"{w}: any-hit differs from the oracle on {int((hit != rany).sum())} rays"
    return gpu


@pytest.mark.parametrize("k", ts.TINY_SIZES)
def test_tiny_trees(binding, oracle, tmp_path, k):
    """Every builder (the device's HLBVH among them) x maxnodeprims {1, 4, 255} over k random triangles: trees without an interior
    node, with fewer interior records than the LDS top holds, with exactly as many, with more."""
    c = ts.case("tiny", k)
    for method, max_prims, on_device in ts.builders("tiny", with_device=True):
        scene = ts.load(binding, tmp_path, f"tiny{k}", c.tris, method, max_prims, bvh_on_device=on_device)
        _check_device(binding, oracle, c, scene, f"tiny({k}) {method}{' on the device' if on_device else ''} maxnodeprims {max_prims}")


def test_slivers(binding, oracle, tmp_path):
    c = ts.case("slivers")
    for method, max_prims, on_device in ts.builders("slivers", with_device=True):
        scene = ts.load(binding, tmp_path, "slivers", c.tris, method, max_prims, bvh_on_device=on_device)
        _check_device(binding, oracle, c, scene, f"slivers {method}{' on the device' if on_device else ''}")


def test_nest(binding, oracle, tmp_path, limits):
    """The deep chains: test_trace_ground_truth.py::test_nest_against_brute_force_and_spills asserts that these rays evict, pop from
    HBM and evict again in the "middle" tree."""
    c = ts.case("nest", ts.nest_frames(limits))
    for method, max_prims, on_device in ts.builders("nest", with_device=True):
        scene = ts.load(binding, tmp_path, "nest", c.tris, method, max_prims, bvh_on_device=on_device)
        assert trace_ref.tree_shape(scene.bvh()[0])[1] <= limits["max_bvh_depth"] - 8
        _check_device(binding, oracle, c, scene, f"nest {method}{' on the device' if on_device else ''}")


def test_ray_counts_around_a_wavefront_and_a_full_grid(binding, tmp_path):
    """tiny(64) with 0, 1, 63 ... 257 rays and with more rays than a full grid of persistent waves holds at once (they must refill):
    every ray is checked against the brute force."""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    tris = ts.tiny(64)
    scene = ts.load(binding, tmp_path, "tiny64", tris, "sah", 4)
    gpu = binding.GpuScene(scene)
    tri_p = scene.bvh()[1]
    for n in (0, 1, 63, 64, 65, 255, 256, 257, n_cus * 8 * 256 + 65):
        c = ts.Case("tiny", tris, n, 5000 + n % 1000) if n else None
        for instrumented in (True, False):
            if n == 0:
                empty = np.zeros((0, 3), np.float32)
                prim, tb, _ = gpu.trace_closest(empty, empty, np.zeros(0, np.float32), instrumented=instrumented)
                hit, _ = gpu.trace_any(empty, empty, np.zeros(0, np.float32), instrumented=instrumented)
                assert len(prim) == 0 and len(hit) == 0
                continue
            prim, tb, _ = gpu.trace_closest(c.o, c.d, c.tmax, instrumented=instrumented)
            ts.check_closest(c, tri_p, prim, tb[:, 0], f"{n} rays, instrumented={instrumented}")
            hit, _ = gpu.trace_any(c.o, c.d, c.tmax, instrumented=instrumented)
            ts.check_any(c, hit, f"{n} rays (any), instrumented={instrumented}")
            if n > 256:
                assert c.truth.decided.mean() >= 0.97 and (c.truth.hit & c.truth.decided).mean() >= 0.05


def test_lane_independence_on_nest(binding, tmp_path, limits):
    """64 copies of the deepest-stack ray among shallow rays and misses, in several interleavings: every copy returns the bits of the
    ray traced alone (a stack column that leaks into its neighbour, or a wrong ring slot, would show here)."""
    lds = limits["lds_stack"]
    c = ts.case("nest", ts.nest_frames(limits))
    scene = ts.load(binding, tmp_path, "nest", c.tris, "middle", 4)
    nodes, tri_p, _ = scene.bvh()
    prof = trace_ref.stack_profile(nodes, tri_p, c.o, c.d, c.tmax, lds)
    ok = c.truth.decided
    deep = int(np.argmax(np.where(ok & c.truth.hit, prof["peak"], -1)))
    assert prof["peak"][deep] > 2 * lds
    shallow = np.nonzero(ok & (prof["peak"] <= 2))[0]
    assert len(shallow) >= 64 and (~c.truth.hit[shallow]).any()
    gpu = binding.GpuScene(scene)
    rng = np.random.default_rng(9)
    lane = np.arange(64)
    patterns = {"every lane": lambda w, l: w == 0, "lane 0": lambda w, l: l == 0, "lane 63": lambda w, l: l == 63,
                "alternating": lambda w, l: (w < 2) & (l % 2 == 0)}
    for instrumented in (True, False):
        p1, tb1, _ = gpu.trace_closest(c.o[[deep]], c.d[[deep]], c.tmax[[deep]], instrumented=instrumented)
        h1, _ = gpu.trace_any(c.o[[deep]], c.d[[deep]], c.tmax[[deep]], instrumented=instrumented)
        assert p1[0] >= 0
        for name, is_deep in patterns.items():
            w, l = np.repeat(np.arange(64), 64), np.tile(lane, 64)
            mask = is_deep(w, l)
            assert mask.sum() == 64
            idx = np.where(mask, deep, rng.choice(shallow, len(mask)))
            prim, tb, _ = gpu.trace_closest(c.o[idx], c.d[idx], c.tmax[idx], instrumented=instrumented)
            same = (_bits(prim[mask], tb[mask]) == _bits(p1, tb1)).all(1)
            assert same.all(), f"{name}, instrumented={instrumented}: {int((~same).sum())} of 64 copies differ from the ray traced alone"
            ts.check_closest(ts_subset(c, idx), tri_p, prim, tb[:, 0], f"lane independence, {name}")
            hit, _ = gpu.trace_any(c.o[idx], c.d[idx], c.tmax[idx], instrumented=instrumented)
            assert (hit[mask] == h1[0]).all(), (name, instrumented)


class ts_subset:
    """A case's rays idx with their truth (no new brute force)."""

    def __init__(self, c, idx):
        self.o, self.d, self.tmax, self.original = c.o[idx], c.d[idx], c.tmax[idx], c.original
        self.truth = trace_ref.Truth(len(idx), c.truth.ties.shape[1])
        for f in ("t_min", "ties", "edge", "cos", "at_tmax", "at_zero"):
            setattr(self.truth, f, getattr(c.truth, f)[idx])


def test_nest_render_matches_oracle(binding, oracle, tmp_path, limits):
    """The deep tree through k_extend, k_shadow and k_mis (their own copies of the loop): 32 x 32, 4 spp, depth 3, a point light."""
    c = ts.case("nest", ts.nest_frames(limits))
    h = ts.NEST_HEIGHT
    scene = ts.load(binding, tmp_path, "nest_render", c.tris, "middle", 4, light=("%g %g %g" % ((h * h,) * 3), "%g %g %g" % (0.1 * h, 0.05 * h, 1.5 * h)),
                    look="%g %g %g  0 0 0  0 1 0" % (0.05 * h, 0.02 * h, 2.0 * h))
    assert trace_ref.tree_shape(scene.bvh()[0])[1] >= 3 * limits["lds_stack"]
    film, _ = binding.GpuScene(scene).render()
    ref, _ = oracle.render(scene)
    assert np.array_equal(film.view(np.uint32), ref.view(np.uint32)), f"{int((film != ref).any(2).sum())} pixels differ"
    assert (film[..., :3] > 0).any(2).mean() > 0.05   # the frames are lit and seen
