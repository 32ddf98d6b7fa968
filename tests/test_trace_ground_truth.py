"""The host builders' trees and the oracle's walk against a ground truth that reads no tree (trace_ref.py: every ray against every
triangle, float64), on the cases of trace_scenes.py. The oracle is bitwise what the device kernels compute (test_gpu_parity.py), so
what holds here is what test_gpu_trace_ground_truth.py then asks of the device.

Measured (python tests/trace_scenes.py; trace_ref.py's docstring says how): worst relative t error of the oracle 2.73e-5 (slivers),
BAND 1.1e-4 (4 x); EPS 2e-6; GRAZE 0.01. Decided / hit-among-decided shares per case, asserted below at >= 97 % and >= 5 %:
tiny(1) 100 % / 16.0 % (the fewest hits), tiny(85) and tiny(86) 99.90 % (the fewest decided) / 54.5 % and 51.6 %, every other tiny(k)
between those; slivers 99.78 % / 65.6 %; nest(40) 97.88 % / 26.8 %. Tree depths of nest(40): middle 44 (peak stack 42, 1091 rays
above two rings, 213 that evict again after a pop from HBM), sah 25, hlbvh 12, equal 10 — "equal" halves the primitives and does not
chain, so the depth window is asserted for "middle"."""
import numpy as np
import pytest

import trace_ref
import trace_scenes as ts

MIN_DECIDED, MIN_HIT = 0.97, 0.05


@pytest.fixture(scope="module")
def limits(binding):
    return binding.traversal_limits()


def _check_scene(c, scene, oracle, what, limits, sim_rays):
    nodes, tri_p, _ = scene.bvh()
    prim, tb = oracle.intersect(scene, c.o, c.d, c.tmax)
    ts.check_closest(c, tri_p, prim, tb[:, 0], f"oracle.intersect, {what}")
    ts.check_any(c, oracle.intersect_p(scene, c.o, c.d, c.tmax), f"oracle.intersect_p, {what}")
    # the tree itself, walked in float64: the same closest hit as without a tree, and a stack no deeper than the tree
    n_interior, depth = trace_ref.tree_shape(nodes)
    sel = slice(0, sim_rays)
    prof = trace_ref.stack_profile(nodes, tri_p, c.o[sel], c.d[sel], c.tmax[sel], limits["lds_stack"])
    assert prof["peak"].max() <= depth, (what, int(prof["peak"].max()), depth)
    want = c.truth.t_min[sel]
    with np.errstate(invalid="ignore"):
        same = (prof["t"] == want) | (np.abs(prof["t"] - want) <= 1e-12 * np.abs(want))
    assert same.all(), f"{what}: the float64 walk of the tree finds another closest hit than brute force on {int((~same).sum())} rays"
    return n_interior, depth, prof


def _check_shares(c, what):
    decided, hit = c.shares()
    print(f"{what}: decided {decided:.4f}, hits among decided {hit:.4f}")
    assert decided >= MIN_DECIDED and hit >= MIN_HIT, (what, decided, hit)


@pytest.mark.parametrize("k", ts.TINY_SIZES)
def test_tiny_trees_against_brute_force(binding, oracle, tmp_path, limits, k):
    """k random triangles, every host builder x maxnodeprims {1, 4, 255}: the oracle's closest hit and any-hit answers are the
    brute-force ones on every decided ray."""
    c = ts.case("tiny", k)
    _check_shares(c, f"tiny({k})")
    for method, max_prims, _ in ts.builders("tiny", with_device=False):
        scene = ts.load(binding, tmp_path, f"tiny{k}", c.tris, method, max_prims)
        _check_scene(c, scene, oracle, f"tiny({k}) {method} maxnodeprims {max_prims}", limits, sim_rays=256)


def test_tiny_sizes_straddle_the_lds_top(binding, tmp_path, limits):
    """The sizes give trees with no interior node, with fewer interior records than the kernels keep in LDS, with exactly as many and
    with more (maxnodeprims 1: k - 1 interior nodes)."""
    counts = set()
    for k in ts.TINY_SIZES:
        for method in ts.HOST_METHODS:
            scene = ts.load(binding, tmp_path, f"tiny{k}", ts.case("tiny", k).tris, method, 1)
            counts.add(trace_ref.tree_shape(scene.bvh()[0])[0])
    top = limits["top_records"]
    assert 0 in counts and top in counts and top + 1 in counts and top - 1 in counts, (sorted(counts), top)
    assert any(0 < n < top - 1 for n in counts) and any(n > 3 * top for n in counts), (sorted(counts), top)


def test_slivers_against_brute_force(binding, oracle, tmp_path, limits):
    """2000 long thin triangles through one region: boxes overlap, nearly every level defers a child."""
    c = ts.case("slivers")
    _check_shares(c, "slivers")
    peaks = []
    for method, max_prims, _ in ts.builders("slivers", with_device=False):
        scene = ts.load(binding, tmp_path, "slivers", c.tris, method, max_prims)
        _, depth, prof = _check_scene(c, scene, oracle, f"slivers {method}", limits, sim_rays=1024)
        peaks.append((method, depth, int(prof["peak"].max())))
    print("slivers (method, depth, peak stack):", peaks)
    assert max(p[2] for p in peaks) > limits["lds_stack"], peaks  # the stack stress reaches the eviction path


def test_nest_against_brute_force_and_spills(binding, oracle, tmp_path, limits):
    """Two chains of frames: the "middle" tree is deep enough for three rings of stack and stays eight levels under the guard's limit;
    more than a thousand rays peak above two rings, and some climb past a ring, come back from the evicted levels and evict again."""
    lds, max_depth = limits["lds_stack"], limits["max_bvh_depth"]
    m = ts.nest_frames(limits)
    c = ts.case("nest", m)
    _check_shares(c, f"nest({m})")
    shapes = {}
    for method, max_prims, _ in ts.builders("nest", with_device=False):
        scene = ts.load(binding, tmp_path, "nest", c.tris, method, max_prims)
        _, depth, prof = _check_scene(c, scene, oracle, f"nest({m}) {method}", limits, sim_rays=len(c.tmax))
        shapes[method] = (depth, int(prof["peak"].max()), int((prof["peak"] > 2 * lds).sum()), int((prof["again"] > 0).sum()))
        assert depth <= max_depth - 8, (method, depth)
    print(f"nest({m}) (depth, peak, rays above two rings, rays that evict again after a pop from HBM):", shapes)
    depth, peak, deep, again = shapes["middle"]
    assert 3 * lds <= depth <= max_depth - 8, shapes
    assert deep > 1000 and again > 0, shapes
