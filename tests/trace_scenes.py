"""Scenes and rays for the tree-free traversal tests (trace_ref.py is their ground truth): the smallest trees at which each piece of
the device-only traversal machinery can go wrong. Deterministic: geometry from seeded numpy generators, floats written with %.9g
so that strtof reads back exactly the float32 values generated here. Every scene is one `trianglemesh` with Material "matte".

    tiny(k)       k random triangles in a unit box: trees with no interior node, fewer / as many / more interior records than the
                  traversal kernels keep in LDS
    slivers(n)    long thin triangles through a common region: most boxes overlap, a ray defers a child at almost every level
    nest(m)       two cones of m square frames each, every frame (8 triangles) the previous one scaled by RATIO about the cone's
                  apex, side by side along x. "middle" peels one frame per level, so each cone is a chain about m deep ("sah" about
                  half that; "equal" and "hlbvh" stay shallow).
                  One cone is what the stack's depth needs; the second is there so that one ray can climb a deep chain, unwind
                  and climb another (eviction, the pop that comes back from HBM, eviction again).
"""
import os

import numpy as np

TINY_SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 21, 22, 23, 64, 85, 86)
HOST_METHODS = ("sah", "middle", "equal", "hlbvh")
MAX_NODE_PRIMS = (1, 4, 255)

# ---- geometry --------------------------------------------------------------------------------------------------------------


def tiny(k, seed=100):
    rng = np.random.default_rng(seed + k)
    return rng.uniform(0, 1, (k, 9)).astype(np.float32)


def slivers(n=2000, seed=7):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.normal(size=(n, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    c = rng.uniform(-0.15, 0.15, (n, 3))
    length, width = rng.uniform(0.6, 1.0, (n, 1)), rng.uniform(0.01, 0.03, (n, 1))
    return np.concatenate([c - length * u, c + length * u + width * v, c + length * u - width * v], 1).astype(np.float32)


# (the smallest frame of a 40-frame cone is 1.5e-9 across: the triangle test multiplies three lengths, which must stay float32 normals)
NEST_RATIO, NEST_HALF, NEST_HEIGHT, NEST_HOLE, NEST_TWIN_X, NEST_TILT = 0.48, 1000.0, 4000.0, 0.6, 16000.0, 0.02


def _frame(half, z, hole):
    """A square frame at height z: the square of half-width `half` without the square of half-width hole * half, 8 triangles,
    tilted a little so that no triangle lies in a plane of the scene's box (an axis-aligned ray inside such a plane is undecided)."""
    a, b = half, half * hole
    outer = [(-a, -a), (a, -a), (a, a), (-a, a)]
    inner = [(-b, -b), (b, -b), (b, b), (-b, b)]
    tris = []
    for i in range(4):
        j = (i + 1) % 4
        tris.append([*outer[i], z, *outer[j], z, *inner[j], z])
        tris.append([*outer[i], z, *inner[j], z, *inner[i], z])
    f = np.array(tris, np.float64)
    f[:, 2::3] *= 1 + NEST_TILT * (f[:, 0::3] + 0.5 * f[:, 1::3]) / half
    return f


def nest(m):
    """Frame i of a cone: half-width NEST_HALF * RATIO^i at height NEST_HEIGHT * RATIO^i above the apex; apexes at the origin and at
    (NEST_TWIN_X, 0, 0). The cones open towards +z: the z extent of the centroids is the largest, so the builders split along z."""
    tris = []
    for x0 in (0.0, NEST_TWIN_X):
        for i in range(m):
            f = _frame(NEST_HALF * NEST_RATIO ** i, NEST_HEIGHT * NEST_RATIO ** i, NEST_HOLE)
            f[:, 0::3] += x0
            tris.append(f)
    return np.concatenate(tris).astype(np.float32)


# ---- scene files -----------------------------------------------------------------------------------------------------------
def _fmt(a):
    return " ".join("%.9g" % x for x in np.asarray(a, np.float32).ravel())


def scene_text(tris, method="sah", max_node_prims=4, light=None, res=32, spp=4, depth=3, look=None):
    n = len(tris)
    look = look or "0.5 0.5 -4  0.5 0.5 0.5  0 1 0"
    return f"""LookAt {look}
Camera "perspective" "float fov" [50]
Film "image" "integer xresolution" [{res}] "integer yresolution" [{res}] "string filename" "trace.exr"
Sampler "halton" "integer pixelsamples" [{spp}]
Integrator "path" "integer maxdepth" [{depth}]
Accelerator "bvh" "string splitmethod" ["{method}"] "integer maxnodeprims" [{max_node_prims}]
WorldBegin
{'LightSource "point" "rgb I" [%s] "point from" [%s]' % light if light else ''}
Material "matte" "rgb Kd" [0.6 0.6 0.6]
Shape "trianglemesh" "point P" [ {_fmt(tris)} ]
  "integer indices" [ {" ".join(str(i) for i in range(3 * n))} ]
WorldEnd
"""


def load(binding, directory, name, tris, method, max_node_prims=4, bvh_on_device=False, **kw):
    path = os.path.join(str(directory), f"{name}_{method}_{max_node_prims}.pbrt")
    with open(path, "w") as f:
        f.write(scene_text(tris, method, max_node_prims, **kw))
    return binding.HostScene(path=path, bvh_on_device=bvh_on_device)


# ---- rays ------------------------------------------------------------------------------------------------------------------
def _aimed(rng, n, centre, radius, spread):
    """Origins on a sphere around `centre`, aimed at points within `spread` of it."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = centre + radius * v
    tgt = centre + rng.uniform(-spread, spread, (n, 3))
    return o, tgt - o


def degenerate_rays(rng, n, lo, hi):
    """test_gpu_parity._degenerate_rays for a scene with the bounds [lo, hi]: directions with zero and negative-zero components,
    origins exactly on the planes of the scene's box."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    o = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n, 3))
    d = rng.uniform(-1, 1, (n, 3))
    for i in range(n):
        k = int(rng.integers(0, 8))
        zero = lambda: 0.0 if rng.random() < .5 else -0.0
        if k < 6:  # on a plane of the box, travelling inside it
            ax = k % 3
            o[i, ax] = (lo, hi)[k // 3][ax]
            d[i, ax] = zero()
        elif k == 6:
            d[i, rng.integers(0, 3)] = zero()
        else:  # axis aligned, towards the box
            ax = int(rng.integers(0, 3))
            o[i] = rng.uniform(lo, hi)
            o[i, ax] = lo[ax] - 0.5 * ext[ax]
            d[i] = [zero(), zero(), zero()]
            d[i, ax] = 1.0
    return o, d


def nest_axis_rays(rng, n, j_max, x0=0.0):
    """Rays from inside a cone, below frame j < j_max, towards +z: they enter the box of every chain node above frame j and defer a
    frame at each of those levels. Slopes up to the cone's own: below NEST_HOLE of it a ray passes every hole."""
    j = rng.integers(0, j_max, n)
    z0 = 0.75 * NEST_HEIGHT * NEST_RATIO ** j
    slope = rng.uniform(-1, 1, (n, 2)) * (NEST_HALF / NEST_HEIGHT) * 1.1
    o = np.stack([x0 + slope[:, 0] * z0, slope[:, 1] * z0, z0], 1)
    d = np.stack([slope[:, 0], slope[:, 1], np.ones(n)], 1)
    return o, d


# float32 resolves 6e-8 of a coordinate: around the second cone's apex at x = NEST_TWIN_X nothing below 1e-3 is told apart, so rays
# that are to be decided there stay above frame NEST_TWIN_LEVELS (0.14 across); the first cone's apex is the origin, resolved to the end
NEST_TWIN_LEVELS = 14


def nest_cross_rays(rng, n, m):
    """Rays along +x from just outside the first cone's tip, at a small height, rising to frame 12 .. 14 of the second cone: down one
    chain, back up, and down the other for more levels than the LDS ring holds."""
    zeta = NEST_HEIGHT * NEST_RATIO ** rng.uniform(14, m - 1, n)
    rise = NEST_HEIGHT * NEST_RATIO ** rng.uniform(12, NEST_TWIN_LEVELS, n)
    o = np.stack([-8 * zeta, zeta * rng.uniform(-0.1, 0.1, n), zeta], 1)
    d = np.stack([np.ones(n), rise * rng.uniform(-0.1, 0.1, n) / NEST_TWIN_X, rise / NEST_TWIN_X], 1)
    return o, d


def nest_through_rays(rng, n, m):
    """Rays from under the first cone's tip towards the annulus of one of the second cone's four largest frames: they descend the
    first chain for some 35 levels, miss every frame of it, and hit what the walk deferred first of all, at the root. A stack that
    loses its oldest evicted level misses that hit."""
    eps = NEST_HALF * NEST_RATIO ** (m - 1)
    o = np.stack([-2 * eps * rng.uniform(0.5, 1, n), eps * rng.uniform(-0.1, 0.1, n), -0.5 * eps * rng.uniform(0.5, 1, n)], 1)
    half = NEST_HALF * NEST_RATIO ** rng.integers(0, 4, n)
    u = rng.uniform(NEST_HOLE + 0.1, 0.9, n) * rng.choice([-1.0, 1.0], n) * half
    v = rng.uniform(-0.5, 0.5, n) * half
    tgt = np.stack([NEST_TWIN_X + u, v, half * NEST_HEIGHT / NEST_HALF * (1 + NEST_TILT * (u + 0.5 * v) / half)], 1)
    return o, tgt - o


def rays_for(case, tris, n, seed, m=None):
    """(o, d, tmax) float32: the case's own rays, then an eighth (nest: a sixteenth) of degenerate directions; tmax infinite (finite_tmax draws the rest)."""
    rng = np.random.default_rng(seed)
    P = np.asarray(tris, np.float64).reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    centre, size = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) or 1.0
    n_deg = n // (16 if case == "nest" else 8)   # (on nest a sixth of them passes a cone's tip closer than float32 resolves: undecided)
    n_own = n - n_deg
    if case == "nest":
        a, b, c = n_own // 2, n_own // 8, n_own // 16
        parts = [nest_axis_rays(rng, a, m), nest_axis_rays(rng, b, NEST_TWIN_LEVELS, NEST_TWIN_X), nest_cross_rays(rng, c, m),
                 nest_through_rays(rng, b, m),
                 _aimed(rng, n_own - a - 2 * b - c, np.array([0.0, 0.0, 1.0]) * NEST_HALF, 6.0 * NEST_HALF, 1.5 * NEST_HALF)]
        o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    elif case == "slivers":
        o, d = _aimed(rng, n_own, centre, 2.0, 0.25)
    else:
        o, d = _aimed(rng, n_own, centre, 1.5 * size, 0.5 * size / 1.7)
    o2, d2 = degenerate_rays(rng, n_deg, lo, hi)
    o, d = np.concatenate([o, o2]).astype(np.float32), np.concatenate([d, d2]).astype(np.float32)
    return o, d, np.full(len(o), np.inf, np.float32)


def finite_tmax(rng, t_min, extent):
    """Half of the rays get a finite tmax drawn around the truth's t (both t < tmax and t > tmax occur); misses get one of the scene's size."""
    n = len(t_min)
    tmax = np.full(n, np.inf, np.float32)
    pick = rng.random(n) < 0.5
    base = np.where(np.isfinite(t_min), t_min, extent)
    tmax[pick] = (base * rng.choice([0.5, 0.9, 0.999, 1.001, 1.1, 2.0], n))[pick].astype(np.float32)
    return tmax


# ---- cases: geometry, rays and their ground truth, computed once and shared --------------------------------------------------
N_RAYS = {"tiny": 2048, "slivers": 4096, "nest": 4096}
_cases = {}


class Case:
    def __init__(self, kind, tris, n_rays, seed, m=None):
        import trace_ref
        self.kind, self.tris, self.m = kind, tris, m
        P = tris.astype(np.float64).reshape(-1, 3)
        self.lo, self.hi = P.min(0), P.max(0)
        self.extent = float(np.linalg.norm(self.hi - self.lo))
        self.o, self.d, inf = rays_for(kind, tris, n_rays, seed, m)
        first = trace_ref.brute_force(tris, self.o, self.d, inf)
        self.tmax = finite_tmax(np.random.default_rng(seed + 1), first.t_min, self.extent)
        self.truth = trace_ref.brute_force(tris, self.o, self.d, self.tmax)
        self._index = {row.tobytes(): i for i, row in enumerate(tris)}
        assert len(self._index) == len(tris)

    def original(self, tri_p, prim):
        """A scene's primitive numbers (BVH order, -1 = miss) as numbers of self.tris, found by the vertices themselves."""
        perm = np.array([self._index[row.tobytes()] for row in np.ascontiguousarray(tri_p, np.float32)], np.int64)
        assert sorted(perm) == list(range(len(self.tris))), "the scene's triangles are not the case's: one was dropped, doubled or changed"
        prim = np.asarray(prim)
        return np.where(prim >= 0, perm[np.maximum(prim, 0)], -1)

    def shares(self):
        dec = self.truth.decided
        return float(dec.mean()), float((self.truth.hit & dec).sum() / max(int(dec.sum()), 1))


def nest_frames(limits):
    """Frames per cone so that the "middle" chain (one frame per level, the root's split between the cones, two or three levels inside
    a frame) lands in the middle of [3 * lds_stack, max_bvh_depth - 8]."""
    return (3 * limits["lds_stack"] + limits["max_bvh_depth"] - 8) // 2 - 4


def case(kind, k=None, limits=None):
    key = (kind, k)
    if key not in _cases:
        if kind == "tiny":
            _cases[key] = Case("tiny", tiny(k), N_RAYS["tiny"], 1000 + k)
        elif kind == "slivers":
            _cases[key] = Case("slivers", slivers(2000), N_RAYS["slivers"], 2000)
        else:
            _cases[key] = Case("nest", nest(k), N_RAYS["nest"], 3000, m=k)
    return _cases[key]


def check_closest(c, tri_p, prim, t, what):
    """The closest-hit assertions on the decided rays: misses exactly where the truth misses, the primitive in the tie set, t in the band."""
    import trace_ref
    bad = trace_ref.disagreements(c.truth, c.original(tri_p, prim), t)
    if len(bad):
        i = int(bad[0])
        got = int(c.original(tri_p, prim)[i])
        raise AssertionError(f"{what}: {len(bad)} decided rays disagree with the ground truth; ray {i}: o {c.o[i]} d {c.d[i]} tmax {c.tmax[i]} "
                             f"got prim {got} t {t[i]!r}, truth t {c.truth.t_min[i]!r} ties {np.nonzero(c.truth.ties[i])[0].tolist()}")


def check_any(c, hit, what):
    import trace_ref
    bad = trace_ref.any_disagreements(c.truth, hit)
    assert len(bad) == 0, f"{what}: {len(bad)} decided rays disagree with the ground truth, first ray {int(bad[0])}: got {int(hit[bad[0]])}"


def builders(kind, with_device):
    """(split method, maxnodeprims, bvh_on_device) per scene of a case: tiny takes the whole product; slivers and nest the methods at 4."""
    prims = MAX_NODE_PRIMS if kind == "tiny" else (4,)
    out = [(m, p, False) for m in HOST_METHODS for p in prims]
    if with_device:
        out += [("hlbvh", p, True) for p in prims]
    return out


def calibrate():
    """Prints what trace_ref.py's BAND, EPS and GRAZE are taken from: the oracle (host builders, every case) against the brute force."""
    import sys
    import tempfile
    import trace_ref
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    from conftest import load_binding
    import oracle_binding
    binding, oracle = load_binding(), oracle_binding.Oracle()
    limits = binding.traversal_limits()
    names = [("tiny", k) for k in TINY_SIZES] + [("slivers", None), ("nest", nest_frames(limits))]
    # the same cases with many more rays (one builder: the triangle test, not the tree, decides what happens at an edge)
    m = nest_frames(limits)
    big = [Case("tiny", tiny(64), 1 << 17, 91), Case("tiny", tiny(86), 1 << 17, 92), Case("slivers", slivers(2000), 1 << 15, 93),
           Case("nest", nest(m), 1 << 16, 94, m=m)]
    eps_grid = [0.0] + [m * 10.0 ** e for e in range(-10, -3) for m in (1, 2, 5)]
    graze_grid = [0.0] + [10.0 ** e for e in range(-7, -1)]
    worst, runs = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for kind, k, c in [(kind, k, case(kind, k)) for kind, k in names] + [(c.kind, "big", c) for c in big]:
            for method, max_prims, _ in (builders(kind, with_device=False) if k != "big" else [("sah", 4, False)]):
                scene = load(binding, tmp, kind, c.tris, method, max_prims)
                tri_p = scene.bvh()[1]
                prim, tb = oracle.intersect(scene, c.o, c.d, c.tmax)
                t64, cs = trace_ref.t_of(tri_p, c.o, c.d, prim)
                c.truth.eps, c.truth.graze = 1e-3, 1e-2   # generous: the band is measured away from edges and grazing hits
                ok = (prim >= 0) & c.truth.decided
                rel = np.abs(tb[:, 0].astype(np.float64) - t64)[ok] / t64[ok]
                worst[kind] = max(worst.get(kind, 0.0), float(rel.max()) if len(rel) else 0.0)
                runs.append((c, c.original(tri_p, prim), tb[:, 0].astype(np.float64), oracle.intersect_p(scene, c.o, c.d, c.tmax), f"{kind} {k} {method} {max_prims}"))
    print("worst relative t error of the oracle per kind:", worst, "-> BAND", 4 * max(worst.values()), "(in use:", trace_ref.BAND, ")")

    def clean(eps, graze):
        for c, prim, t, anyhit, what in runs:
            c.truth.eps, c.truth.graze = eps, graze
            if len(trace_ref.disagreements(c.truth, prim, t)) or len(trace_ref.any_disagreements(c.truth, anyhit)):
                return what
        return None
    for graze in graze_grid:
        first = next((e for e in eps_grid if clean(e, graze) is None), None)
        print(f"GRAZE {graze:g}: smallest EPS of the grid without a disagreement: {first}" + ("" if first is not None else f" (last offender: {clean(eps_grid[-1], graze)})"))
    for c, *_ in runs:
        c.truth.eps, c.truth.graze = trace_ref.EPS, trace_ref.GRAZE
    done = set()
    for c, _, _, _, what in runs:
        if id(c) not in done:
            done.add(id(c))
            print(what.rsplit(" ", 2)[0], "decided %.4f, hits among decided %.4f" % c.shares())


if __name__ == "__main__":
    calibrate()
