"""Brute-force float64 ground truth for ray / triangle-soup queries: no tree is read.

Input: the triangles `HostScene.bvh()` returns (`tri_p`, (n_prims, 9) float32, BVH order) and rays (o, d, tmax). Every ray
is tested against every triangle with Moller-Trumbore in float64 (the float32 inputs are exact in float64, so the only
error here is float64's own rounding, nine orders of magnitude below the float32 walk it judges).

`brute_force` returns a `Truth`:

    t_min    (n,)   the nearest hit distance with 0 < t <= tmax, inf on a miss
    ties     (n, n_prims) bool: the triangles hit at t <= t_min (1 + BAND); a float32 walk may return any of them
             (coincident and abutting triangles are legitimate ties)
    decided  (n,)   False where float32 may legitimately answer differently. With "near" meaning a triangle whose plane the ray
                    meets between just behind the origin and min(t_min, tmax) (1 + BAND):
                      * the ray passes within EPS of an edge of a near triangle. The margin is in barycentric units times what
                        one such unit subtends from the origin (the triangle's smallest altitude over its farthest vertex's
                        distance): float32 resolves 6e-8 of a coordinate, so a ray is told apart from an edge by angle, and a
                        plain barycentric margin would call a 1e-7-wide triangle seen from 20000 away decided;
                      * it hits a near triangle at |d.n| / (|d| |n|) < GRAZE;
                      * it hits a triangle at a t within BAND of tmax;
                      * it hits a triangle at |t| <= T_SMALL x the distance of the triangle's farthest vertex (Triangle::Intersect's
                        `t <= deltaT` rejection, triangle.cpp:262-284, decides those; deltaT scales with that distance, and a
                        multiple of the whole scene's extent would call every ray near the small end of nest() undecided).

The numbers, measured by `python tests/trace_scenes.py` (calibrate(): oracle.intersect, which is bitwise the device walk and is not
the code under test, against this module over every case of trace_scenes.py with the four host builders, and over tiny(64),
tiny(86), slivers and nest with 131072, 131072, 32768 and 65536 rays):

    BAND     4 x the worst relative difference |t_oracle - t_float64| / t_float64 of the oracle's own primitive over decided hits
             with |cos| >= 0.01. Measured worst: 2.73e-5 (slivers; 6.8e-6 on tiny, 2.5e-7 on nest), so BAND = 1.1e-4.
    EPS      2e-6: the smallest value of the grid 0, 1e-10, 2e-10, 5e-10, 1e-9, ... for which the oracle agrees with the truth on
             every decided ray of every case (the next smaller, 1e-6, leaves disagreements).
    GRAZE    0.01: the bound above, within which the band was measured. On the calibration sample the oracle agrees for every
             GRAZE of the grid 0, 1e-7, ... 1e-2 at that EPS, but only the t of hits with |cos| >= 0.01 is known to lie in the
             band: the 524 353 rays of the ray-count case on tiny(64) hold a hit at |cos| = 1.4e-4 whose float32 t is off by
             1.7e-4 (the oracle and the device alike), while down to |cos| = 1e-3 the worst stays 2.2e-5. The exclusion costs
             5e-5 of the rays.
    T_SMALL  1e-4: not measured. deltaT is some tens of gamma(5) = 3e-7 times the products of the triangle's translated
             coordinates over the determinant, about 1e-5 of the distance of its farthest vertex; ten times that. Random origins
             fall that close to a surface about once in 10^4 rays, so the exclusion costs nothing.
"""
import numpy as np

BAND = 1.1e-4
EPS = 2e-6
GRAZE = 0.01
T_SMALL = 1e-4
# what calibrate() printed (worst relative t error; smallest passing EPS; smallest passing GRAZE at that EPS)
MEASURED = {"t_rel_worst": 2.73e-5, "eps_min": 2e-6, "graze_min": 0.0, "graze_of_band": 0.01}

_PAIRS_PER_CHUNK = 1 << 21  # ray x triangle pairs per chunk: a dozen float64 temporaries of that size, some 200 MB


class Truth:
    def __init__(self, n, n_tri):
        self.t_min = np.full(n, np.inf)
        self.ties = np.zeros((n, n_tri), bool)
        self.edge = np.full(n, np.inf)     # smallest |min(b0, b1, b2)| x (the triangle's smallest altitude / its distance) over the near triangles
        self.cos = np.full(n, np.inf)      # smallest |cos(d, n)| over the near triangles the ray hits (0: in the plane of a parallel one)
        self.at_tmax = np.zeros(n, bool)   # hits a triangle within BAND of tmax
        self.at_zero = np.zeros(n, bool)   # hits a triangle at |t| <= T_SMALL x its farthest vertex's distance
        self.eps, self.graze = EPS, GRAZE

    @property
    def hit(self):
        return np.isfinite(self.t_min)

    @property
    def decided(self):
        return (self.edge > self.eps) & (self.cos >= self.graze) & ~self.at_tmax & ~self.at_zero

    def any_hit(self):
        """BVHAccel::IntersectP: some triangle at t < tmax."""
        return self.hit


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def _mt(P, o, d):
    """Moller-Trumbore for every (ray, triangle) pair: (t, b0, b1, b2, |cos|, the origin's distance from the plane over `scale`,
    parallel to a triangle of non-zero area?, scale: the distance of the triangle's farthest vertex, in units of t), each (n, T); rays
    parallel to a triangle's plane get t = inf and barycentrics -1."""
    p0, e1, e2 = P[:, 0:3], P[:, 3:6] - P[:, 0:3], P[:, 6:9] - P[:, 0:3]
    nx, ny, nz = _cross(e1[:, 0], e1[:, 1], e1[:, 2], e2[:, 0], e2[:, 1], e2[:, 2])
    nlen = np.sqrt(nx * nx + ny * ny + nz * nz)
    dx, dy, dz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    dlen = np.sqrt(dx * dx + dy * dy + dz * dz)
    px, py, pz = _cross(dx, dy, dz, e2[None, :, 0], e2[None, :, 1], e2[None, :, 2])
    det = e1[None, :, 0] * px + e1[None, :, 1] * py + e1[None, :, 2] * pz     # = -d.n
    tx, ty, tz = o[:, 0:1] - p0[None, :, 0], o[:, 1:2] - p0[None, :, 1], o[:, 2:3] - p0[None, :, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        cosn = np.abs(det) / (dlen * nlen[None, :])          # nan for a degenerate triangle or a zero direction
        parallel = ~(np.abs(det) > 0) | ~np.isfinite(cosn)
        inv = np.where(parallel, 0.0, 1.0 / np.where(parallel, 1.0, det))
        u = (tx * px + ty * py + tz * pz) * inv
        qx, qy, qz = _cross(tx, ty, tz, e1[None, :, 0], e1[None, :, 1], e1[None, :, 2])
        v = (dx * qx + dy * qy + dz * qz) * inv
        t = (e2[None, :, 0] * qx + e2[None, :, 1] * qy + e2[None, :, 2] * qz) * inv
        plane = np.abs(tx * nx[None, :] + ty * ny[None, :] + tz * nz[None, :]) / np.where(nlen > 0, nlen, 1.0)[None, :]
        # the triangle as the ray sees it: its farthest vertex from the origin, in units of t (what deltaT scales with)
        scale = np.sqrt(tx * tx + ty * ty + tz * tz)
        for k in (3, 6):
            ax, ay, az = P[None, :, k] - o[:, 0:1], P[None, :, k + 1] - o[:, 1:2], P[None, :, k + 2] - o[:, 2:3]
            scale = np.maximum(scale, np.sqrt(ax * ax + ay * ay + az * az))
        plane_rel = plane / np.where(scale > 0, scale, 1.0)
        # the triangle's smallest altitude over that distance: what one unit of barycentric coordinate subtends from the origin
        e3 = e2 - e1
        longest = np.sqrt(np.maximum(np.maximum((e1 * e1).sum(1), (e2 * e2).sum(1)), (e3 * e3).sum(1)))
        subtends = (nlen / np.where(longest > 0, longest, 1.0))[None, :] / np.where(scale > 0, scale, 1.0)
        scale = scale / np.where(dlen > 0, dlen, 1.0)
    t = np.where(parallel, np.inf, t)
    u = np.where(parallel, -1.0, u)
    v = np.where(parallel, -1.0, v)
    return t, 1.0 - u - v, u, v, np.where(parallel, 0.0, cosn), plane_rel, parallel & (nlen > 0)[None, :], scale, subtends


def brute_force(tri_p, o, d, tmax, band=BAND, t_small=T_SMALL):
    P = np.asarray(tri_p, np.float64).reshape(-1, 9)
    o, d, tmax = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3), np.asarray(tmax, np.float64).ravel()
    n, T = len(tmax), len(P)
    tr = Truth(n, T)
    if n == 0 or T == 0:
        return tr
    step = max(1, _PAIRS_PER_CHUNK // T)
    for a in range(0, n, step):
        s = slice(a, min(a + step, n))
        t, b0, b1, b2, cosn, plane, parallel, scale, subtends = _mt(P, o[s], d[s])
        tm = tmax[s][:, None]
        m = np.minimum(np.minimum(b0, b1), b2)
        inside = m >= 0
        hit = inside & (t > 0) & (t <= tm)
        t_min = np.where(hit, t, np.inf).min(1)
        lim = np.minimum(t_min[:, None], tm) * (1 + band)
        near = (t >= -t_small * scale) & (t <= lim)
        tr.t_min[s] = t_min
        tr.ties[s] = hit & (t <= t_min[:, None] * (1 + band))
        tr.edge[s] = np.where(near, np.abs(m) * subtends, np.inf).min(1)
        in_plane = parallel & (plane <= 1e-6)
        tr.cos[s] = np.minimum(np.where(near & inside, cosn, np.inf).min(1), np.where(in_plane.any(1), 0.0, np.inf))
        with np.errstate(invalid="ignore"):
            tr.at_tmax[s] = (inside & np.isfinite(tm) & (np.abs(t - tm) <= band * tm)).any(1)
        tr.at_zero[s] = (inside & (np.abs(t) <= t_small * scale)).any(1)
    return tr


def _mt_rows(T9, o, d):
    """Ray i against triangle T9[i] alone: (t, hit-side test min(b0, b1, b2) >= 0, |cos|); t = inf where parallel."""
    p0, e1, e2 = T9[:, 0:3], T9[:, 3:6] - T9[:, 0:3], T9[:, 6:9] - T9[:, 0:3]
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(1)
    tv = o - p0
    qv = np.cross(tv, e1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cosn = np.abs(det) / (np.linalg.norm(d, axis=1) * np.linalg.norm(np.cross(e1, e2), axis=1))
        par = ~(np.abs(det) > 0) | ~np.isfinite(cosn)
        inv = np.where(par, 0.0, 1.0 / np.where(par, 1.0, det))
    u, v, t = (tv * pv).sum(1) * inv, (d * qv).sum(1) * inv, (e2 * qv).sum(1) * inv
    inside = ~par & (np.minimum(np.minimum(u, v), 1.0 - u - v) >= 0)
    return np.where(par, np.inf, t), inside, np.where(par, 0.0, cosn)


def t_of(tri_p, o, d, prim):
    """float64 t of ray i against triangle prim[i] alone (nan where prim[i] < 0), and |cos| there."""
    P = np.asarray(tri_p, np.float64).reshape(-1, 9)
    o, d, prim = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3), np.asarray(prim)
    t, cs = np.full(len(o), np.nan), np.full(len(o), np.nan)
    i = np.nonzero(prim >= 0)[0]
    t[i], _, cs[i] = _mt_rows(P[prim[i]], o[i], d[i])
    return t, cs


def disagreements(tr, prim, t, eps=None, graze=None, band=BAND):
    """Indices of the decided rays on which a closest-hit answer (prim, t) contradicts the truth: a miss where the truth hits or the
    reverse, a primitive outside the tie set, a t outside the band."""
    if eps is not None:
        tr.eps = eps
    if graze is not None:
        tr.graze = graze
    prim, t = np.asarray(prim), np.asarray(t, np.float64)
    got = prim >= 0
    bad = got != tr.hit
    both = got & tr.hit
    idx = np.nonzero(both)[0]
    bad[idx] |= ~tr.ties[idx, prim[idx]]
    bad[idx] |= np.abs(t[idx] - tr.t_min[idx]) > band * tr.t_min[idx]
    return np.nonzero(bad & tr.decided)[0]


def any_disagreements(tr, hit):
    """Indices of the decided rays on which an any-hit answer contradicts the truth."""
    return np.nonzero(((np.asarray(hit) != 0) != tr.any_hit()) & tr.decided)[0]


# ---- a float64 walk of a flattened tree that records the stack, as the device keeps it -------------------------------------
def stack_profile(nodes, tri_p, o, d, tmax, lds_levels):
    """BVHAccel::Intersect's walk (bvh.cpp:662-700) in float64, all rays in step, with the stack kept as the instrumented device walk
    keeps it: one entry per interior node entered, the newest `lds_levels` entries in a ring and older ones evicted (dtrav.h:
    stack_push, trav_pop). Per ray: peak (the largest stack size), evictions, hbm_pops (pops that had to come back from evicted
    levels), again (evictions after such a pop), and t (the closest hit, inf on a miss)."""
    P = np.asarray(tri_p, np.float64).reshape(-1, 9)
    bmin, bmax = nodes["bmin"].astype(np.float64), nodes["bmax"].astype(np.float64)
    off, npr, axis = nodes["offset"].astype(np.int64), nodes["nprims"].astype(np.int64), nodes["axis"].astype(np.int64)
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    tm = np.asarray(tmax, np.float64).ravel().copy()
    n = len(tm)
    with np.errstate(divide="ignore"):
        inv = 1.0 / d
    neg = inv < 0
    rows = np.arange(n)
    cur, sp, lo = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    stack = np.zeros((n, len(nodes) + 1), np.int64)
    out = {k: np.zeros(n, np.int64) for k in ("peak", "evictions", "hbm_pops", "again")}
    active = np.full(n, len(nodes) > 0)
    found = np.zeros(n, bool)
    while active.any():
        i = rows[active]
        c = cur[i]
        with np.errstate(invalid="ignore", over="ignore"):
            t0 = (np.where(neg[i], bmax[c], bmin[c]) - o[i]) * inv[i]
            t1 = (np.where(neg[i], bmin[c], bmax[c]) - o[i]) * inv[i]
        tn, tf = np.nan_to_num(t0, nan=-np.inf).max(1), np.nan_to_num(t1, nan=np.inf).min(1)
        ok = (tn <= tf) & (tf > 0) & (tn < tm[i])
        leaf = npr[c] > 0
        li, lc = i[ok & leaf], c[ok & leaf]
        for k in range(int(npr[lc].max()) if len(li) else 0):
            m = npr[lc] > k
            r = li[m]
            t, inside, _ = _mt_rows(P[off[lc[m]] + k], o[r], d[r])
            good = inside & (t > 0) & (t <= tm[r])
            tm[r[good]] = t[good]
            found[r[good]] = True
        down = ok & ~leaf
        ii, ic = i[down], c[down]
        second = neg[ii, axis[ic]]
        full = sp[ii] - lo[ii] == lds_levels
        lo[ii[full]] += 1
        out["evictions"][ii[full]] += 1
        out["again"][ii[full]] += out["hbm_pops"][ii[full]] > 0
        stack[ii, sp[ii]] = np.where(second, ic + 1, off[ic])
        sp[ii] += 1
        out["peak"][ii] = np.maximum(out["peak"][ii], sp[ii])
        cur[ii] = np.where(second, off[ic], ic + 1)
        pi = i[~down]
        done = sp[pi] == 0
        active[pi[done]] = False
        pi = pi[~done]
        sp[pi] -= 1
        cur[pi] = stack[pi, sp[pi]]
        back = sp[pi] < lo[pi]
        lo[pi[back]] = sp[pi[back]]
        out["hbm_pops"][pi[back]] += 1
    out["t"] = np.where(found, tm, np.inf)
    return out


def tree_shape(nodes):
    """(number of interior nodes, binary depth: the largest number of interior nodes on a path from the root to a leaf)."""
    n = len(nodes)
    depth = np.zeros(n, np.int32)
    best = 0
    for i in range(n):  # depth-first layout: a parent comes before its children
        if nodes["nprims"][i] == 0:
            depth[i + 1] = depth[nodes["offset"][i]] = depth[i] + 1
        else:
            best = max(best, int(depth[i]))
    return int((nodes["nprims"] == 0).sum()), best
