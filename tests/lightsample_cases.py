"""The cases test_light_sampling_truth.py (oracle, no GPU) and test_gpu_light_sampling_truth.py (device) share: small .pbrt
scenes with one sampled light each, the float64 truth of lightsample_ref.py built from what the loader made of the scene
(matrices, vertices, radiance and the infinite light's tables are float32 DATA; every formula is the truth's own), seeded
reference points, directions and samples with the edge inputs appended, and the comparisons within the truth's bands and caps.

N = 2 * 10^4 samples per case. The common edge inputs of u: u0, u1 in {0, 2^-24, 0.5, 1 - 2^-24}, all sixteen pairs."""
import ctypes

import numpy as np
import pytest

import lightsample_ref as LS
import quadric_ref as Q
from test_image_light_scenes import write_pfm

N = 20_000
CAP = 0.01  # at most 1 % of a case's samples may be left out of a comparison, for each of the three discrete decisions
EDGE_U = np.array([[a, b] for a in (0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24) for b in (0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24)], np.float32)
PRIM_HAS_NORMALS, PRIM_FLIP = 2, 8

HEAD = ('LookAt 0 -6 3  0 0 0.5  0 0 1\nCamera "perspective" "float fov" [40]\n'
        'Film "image" "integer xresolution" [8] "integer yresolution" [8] "string filename" "ls.exr"\nPixelFilter "box"\n'
        'Sampler "halton" "integer pixelsamples" [1]\nIntegrator "path" "integer maxdepth" [1]\nWorldBegin\nMaterial "matte"\n')
FLOOR = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-3 -3 -1  3 -3 -1  0 3 -1]\n'


class SphereStruct(ctypes.Structure):  # iile_sphere, include/iile_scene.h
    _fields_ = [("o2w", ctypes.c_float * 16), ("o2w_inv", ctypes.c_float * 16), ("radius", ctypes.c_float), ("zmin", ctypes.c_float),
                ("zmax", ctypes.c_float), ("theta_min", ctypes.c_float), ("theta_max", ctypes.c_float), ("phi_max", ctypes.c_float),
                ("reverse_orientation", ctypes.c_int32), ("swaps_handedness", ctypes.c_int32)]


def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _with_edges(rng, n):
    """n seeded samples in [0, 1), the sixteen edge pairs at the end (float32)."""
    return np.concatenate([rng.random((n - len(EDGE_U), 2)).astype(np.float32), EDGE_U])


# ---- sphere lights --------------------------------------------------------------------------------------------------------------
SPHERE_CTM = "Translate 1 -2 0.5\nRotate 35 1 2 3\n"
SPHERES = {  # extra directives, shape parameters, twosided
    "sphere": ("", "", False),
    "sphere_two_sided": ("", "", True),
    "sphere_reversed": ("ReverseOrientation\n", "", False),
    "sphere_partial": ("", ' "float zmin" [-0.3] "float zmax" [0.4] "float phimax" [250]', True),
}
SPHERE_PARAMS = {"sphere_partial": dict(zmin=-0.3, zmax=0.4, phimax=250.0)}
RATIOS_OUT, RATIOS_IN = (1.001, 1.05, 2.0, 10.0, 100.0), (0.0, 0.5, 0.99)
SPHERE_L = (3.0, 2.0, 1.5)


def sphere_scene(case):
    extra, params, two = SPHERES[case]
    return (HEAD + f'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [{SPHERE_L[0]} {SPHERE_L[1]} {SPHERE_L[2]}] "bool twosided" "{"true" if two else "false"}"\n'
            + SPHERE_CTM + extra + f'Shape "sphere" "float radius" [0.5]{params}\nAttributeEnd\n' + FLOOR + "WorldEnd\n")


def sphere_truth(host, case):
    d = host.scene_desc()
    assert d.n_spheres == 1 and d.n_lights == 1
    sp = SphereStruct.from_buffer_copy(ctypes.string_at(d.spheres, ctypes.sizeof(SphereStruct)))
    want = Q.translate(1, -2, 0.5) @ Q.rotate(35, (1, 2, 3))
    assert np.allclose(np.array(list(sp.o2w)).reshape(4, 4), want, atol=1e-6)
    assert np.allclose(np.array(list(sp.o2w_inv)).reshape(4, 4), np.linalg.inv(want), atol=1e-6)
    lt = host.light(0)
    assert lt.type == 0 and lt.sphere == 0 and bool(lt.two_sided) == SPHERES[case][2] and list(lt.lemit) == list(np.float32(SPHERE_L))
    assert bool(sp.reverse_orientation) == (case == "sphere_reversed") and sp.radius == 0.5
    shape = LS.Sphere(list(sp.o2w), list(sp.o2w_inv), 0.5, reverse=case == "sphere_reversed", **SPHERE_PARAMS.get(case, {}))
    assert (np.float32(shape.zmin), np.float32(shape.zmax), np.float32(shape.phimax)) == (sp.zmin, sp.zmax, sp.phi_max)
    return LS.AreaLight(shape, SPHERE_L, SPHERES[case][2])


def sphere_points(light, ratios, seed, n=N):
    """Reference points at the distances ratios * r from the centre in seeded directions (float32; pushed outwards by 2e-6 so that
    the float32 point keeps its nominal side of 1.001), each ratio with n / len(ratios) samples, the sixteen edge pairs among them.
    -> (p, u, ratio of every point)."""
    rng = np.random.default_rng(seed)
    s, per = light.shape, n // len(ratios)
    p, u, rat = [], [], []
    for q in ratios:
        d = _dirs(rng, per)
        p.append((s.pc[None, :] + q * (1 + 2e-6) * s.radius * d).astype(np.float32))
        u.append(_with_edges(rng, per))
        rat.append(np.full(per, q))
    p, u, rat = np.concatenate(p), np.concatenate(u), np.concatenate(rat)
    inside, margin = s.inside(p.astype(np.float64))
    assert (margin >= 1e-3).all() and (inside == (rat < 1)).all()  # the inside / outside switch gets no allowance
    return p, u, rat


# ---- triangle lights ------------------------------------------------------------------------------------------------------------
TRI_L = (2.0, 4.0, 1.0)
_c, _s = np.sqrt(1 - 0.05 ** 2), 0.05
TRIANGLES = {  # vertices, normals (or None), extra directives, twosided
    "tri": ([[-0.5, -0.4, 1.0], [0.7, -0.3, 1.2], [0.1, 0.8, 0.9]], None, "", False),
    "tri_two_sided": ([[-0.5, -0.4, 1.0], [0.7, -0.3, 1.2], [0.1, 0.8, 0.9]], None, "", True),
    "tri_sliver": ([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [float(np.float32(_c)), float(np.float32(_s)), 1.0]], None, "", True),
    "tri_far": ([[1000.0, 1000.25, 999.5], [1001.0, 1000.0, 999.75], [1000.25, 1001.0, 1000.0]], None, "", False),
    "tri_normals": ([[-0.5, -0.4, 1.0], [0.7, -0.3, 1.2], [0.1, 0.8, 0.9]], [[0.1, 0.2, -1.0], [-0.2, 0.1, -1.0], [0.0, -0.1, -1.0]], "", False),
    "tri_reversed": ([[-0.5, -0.4, 1.0], [0.7, -0.3, 1.2], [0.1, 0.8, 0.9]], None, "ReverseOrientation\n", False),
}


def triangle_scene(case):
    v, nrm, extra, two = TRIANGLES[case]
    flat = lambda a: " ".join(repr(float(x)) for row in a for x in row)
    normals = f' "normal N" [{flat(nrm)}]' if nrm else ""
    return (HEAD + f'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [{TRI_L[0]} {TRI_L[1]} {TRI_L[2]}] "bool twosided" "{"true" if two else "false"}"\n'
            + extra + f'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [{flat(v)}]{normals}\nAttributeEnd\n'
            + (FLOOR if case != "tri_far" else "") + "WorldEnd\n")


def triangle_truth(host, case):
    v, nrm, extra, two = TRIANGLES[case]
    d = host.scene_desc()
    assert d.n_lights == 1
    lt = host.light(0)
    assert lt.type == 4 and bool(lt.two_sided) == two
    _, tri_p, _ = host.bvh()
    flags = host.prim_flags()
    got = tri_p[lt.prim].reshape(3, 3)
    assert np.array_equal(got, np.array(v, np.float32))  # declared under the identity: the file's vertices themselves
    assert bool(flags[lt.prim] & PRIM_HAS_NORMALS) == (nrm is not None) and bool(flags[lt.prim] & PRIM_FLIP) == bool(extra)
    normals = None
    if nrm is not None:
        normals = np.frombuffer(ctypes.string_at(d.tri_n + 36 * lt.prim, 36), np.float32).reshape(3, 3)
        assert np.array_equal(normals, np.array(nrm, np.float32))
    shape = LS.Triangle(*got, normals=normals, flip=bool(extra))
    if nrm is not None:  # Faceforward is decided clearly: the vertex normals point against the face normal
        face = np.cross(shape.v[1] - shape.v[0], shape.v[2] - shape.v[0])
        assert all(np.dot(face / np.linalg.norm(face), n) < -0.5 for n in shape.nrm)
    if case == "tri_sliver":
        assert abs(shape.sin_gamma - 0.05) < 1e-6
    return LS.AreaLight(shape, TRI_L, two)


def triangle_points(light, seed, n=N):
    """99 of 200 points in front of the triangle, 99 behind it (0.3 to 3 of its size away, over its whole neighbourhood), one
    10^-3 of its size off its plane on either side (above the triangle and beside it: 200 points of 2 * 10^4; there the pdf grows as
    1 / |cos| and a barycentric coordinate of Shape::Pdf's hit is known to a few per cent only, so most of what lies near an edge
    is flagged: more such points and the flags alone would pass the 1 % cap), and 16 at p0 itself with u = (0, x). -> (p, u)"""
    rng = np.random.default_rng(seed)
    t = light.shape
    p0, p1, p2 = t.v
    nrm = np.cross(p1 - p0, p2 - p0)
    size = np.sqrt(np.linalg.norm(nrm))
    nrm = nrm / np.linalg.norm(nrm)
    b = rng.uniform(-0.5, 1.5, (n, 2))
    base = p0 + b[:, :1] * (p1 - p0) + b[:, 1:] * (p2 - p0)
    k = np.arange(n) % 200
    h = np.where(k < 99, 1.0, np.where(k < 198, -1.0, np.where(k == 198, 1e-3, -1e-3))) * size * np.where(k < 198, 10 ** rng.uniform(-0.5, 0.5, n), 1.0)
    p = (base + h[:, None] * nrm).astype(np.float32)
    u = _with_edges(rng, n)
    p[:16] = np.float32(p0)
    u[:16, 0] = 0
    return p, u


# ---- quadric lights -------------------------------------------------------------------------------------------------------------
QUADRIC_L = (1.0, 2.0, 3.0)
QUADRIC_CTM = "Translate 0.5 0.25 1\nRotate 40 1 1 0\nScale 1.5 1 0.75\n"
QUADRICS = {
    "disk": ('Shape "disk" "float radius" [1] "float innerradius" [0.3] "float phimax" [270] "float height" [0.25]', False),
    "cylinder": ('Shape "cylinder" "float radius" [0.5] "float zmin" [-0.5] "float zmax" [0.75] "float phimax" [200]', True),
}


def quadric_scene(case):
    shape, two = QUADRICS[case]
    return (HEAD + f'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [{QUADRIC_L[0]} {QUADRIC_L[1]} {QUADRIC_L[2]}] "bool twosided" "{"true" if two else "false"}"\n'
            + QUADRIC_CTM + shape + "\nAttributeEnd\n" + FLOOR + "WorldEnd\n")


def quadric_truth(host, case):
    assert host.quadric_count == 1 and host.light_count == 1
    q, lt = host.quadric(0), host.light(0)
    assert lt.type == 6 and bool(lt.two_sided) == QUADRICS[case][1]
    want = Q.translate(0.5, 0.25, 1) @ Q.rotate(40, (1, 1, 0)) @ Q.scale(1.5, 1, 0.75)
    m, inv = np.array(list(q.o2w)).reshape(4, 4), np.array(list(q.o2w_inv)).reshape(4, 4)
    assert np.allclose(m, want, atol=1e-6) and np.allclose(inv, np.linalg.inv(want), atol=1e-6)
    if case == "disk":
        shape = Q.Disk(m, height=0.25, radius=1.0, inner=0.3, phimax=270.0)
        assert (q.radius, q.inner_radius, q.height) == (1.0, np.float32(0.3), 0.25)
        shape.inner = float(np.float32(0.3))
    else:
        shape = Q.Cylinder(m, radius=0.5, zmin=-0.5, zmax=0.75, phimax=200.0)
        assert (q.radius, q.zmin, q.zmax) == (0.5, -0.5, 0.75)
    shape.phimax = float(q.phi_max)
    assert abs(q.phi_max - np.radians(270.0 if case == "disk" else 200.0)) < 1e-6
    return LS.AreaLight(LS.Quadric(shape, m, inv, reverse=False), QUADRIC_L, QUADRICS[case][1])


def quadric_points(light, seed, n=N):
    """Points on both sides of the emitter, 0.3 to 5 away from its origin. -> (p, u)"""
    rng = np.random.default_rng(seed)
    p = (light.shape.m[:3, 3][None, :] + _dirs(rng, n) * 10 ** rng.uniform(-0.5, 0.7, (n, 1))).astype(np.float32)
    return p, _with_edges(rng, n)


# ---- the infinite light -----------------------------------------------------------------------------------------------------------
INF_L = (0.75, 1.25, 0.5)
ROTATIONS = {"z": ("Rotate 30 0 0 1\n", Q.rotate(30, (0, 0, 1))), "tilt": ("Rotate 40 1 2 0.5\n", Q.rotate(40, (1, 2, 0.5)))}
MAPS = ("none", "noise4x2", "odd5x3", "spike16x8", "black", "wide16x2")
INFINITE = [f"{m}_{r}" for m in MAPS for r in ROTATIONS]


def map_rows(which):
    """The file's rows, bottom scanline first (float32), or None."""
    rng = np.random.default_rng(MAPS.index(which))
    if which == "none":
        return None
    if which == "noise4x2":
        return (0.1 + rng.random((2, 4, 3))).astype(np.float32)
    if which == "odd5x3":
        return (0.1 + rng.random((3, 5, 3))).astype(np.float32)
    if which == "black":
        return np.zeros((2, 4, 3), np.float32)
    if which == "wide16x2":  # eight times as wide as high: the one shape here whose scalar image is filtered above level 0 (level 1)
        return (0.1 + rng.random((2, 16, 3))).astype(np.float32)
    rows = (0.1 + rng.random((8, 16, 3))).astype(np.float32)
    rows[5, 11] *= 1000  # one texel x 1000
    rows[0], rows[7] = 0, 0  # all-black rows at both poles
    rows[:, 0] = 0  # an all-black column at the seam
    return rows


def infinite_scene(case, tmp_path):
    which, rot = case.rsplit("_", 1)
    rows = map_rows(which)
    name = ""
    if rows is not None:
        write_pfm(tmp_path / f"{which}.pfm", rows)
        name = f' "string mapname" "{which}.pfm"'
    return (HEAD + f'AttributeBegin\n{ROTATIONS[rot][0]}LightSource "infinite" "rgb L" [{INF_L[0]} {INF_L[1]} {INF_L[2]}]{name}\nAttributeEnd\n'
            + FLOOR + "WorldEnd\n")


def host_table(host, lt):
    d = host.scene_desc()
    flat = np.frombuffer(ctypes.string_at(d.env_dist, 4 * d.n_env_dist), np.float32).copy()
    w, h = lt.dist_w, lt.dist_h
    n = (2 * w + 2) * h + 2 * h + 2
    assert lt.dist_offset == 0 and d.n_env_dist == n  # the layout: 2 w + 2 floats per row, the marginal last
    return LS.Table(flat, w, h)


def infinite_truth(host, case):
    which, rot = case.rsplit("_", 1)
    assert host.light_count == 1
    lt = host.light(0)
    assert lt.type == 5 and list(lt.lemit) == list(np.float32(INF_L))
    l2w, w2l = np.array(list(lt.l2w)).reshape(3, 3), np.array(list(lt.w2l)).reshape(3, 3)
    assert np.allclose(l2w, ROTATIONS[rot][1][:3, :3], atol=1e-6) and np.allclose(w2l, ROTATIONS[rot][1][:3, :3].T, atol=1e-6)
    rows = map_rows(which)
    image = None if rows is None else rows[::-1]
    return LS.InfiniteLight(image, INF_L, l2w, w2l, table=host_table(host, lt), world_radius=lt.world_radius)


def infinite_samples(light, seed, n=N):
    """Seeded u with the sixteen edge pairs, plus u0 and u1 set exactly to entries of the host's cdf rows (every entry of the
    marginal and of three rows) and to the float32 values one ulp either side of them."""
    rng = np.random.default_rng(seed)
    t = light.table
    entries = np.unique(np.concatenate([t.mcdf] + [t.cdf[r] for r in sorted({0, t.h // 2, t.h - 1})]).astype(np.float32))
    near = np.unique(np.clip(np.concatenate([entries, np.nextafter(entries, np.float32(-1)), np.nextafter(entries, np.float32(2))]), 0,
                             np.float32(1) - np.float32(2.0 ** -24)).astype(np.float32))
    other = rng.random(len(near)).astype(np.float32)
    special = np.concatenate([np.stack([near, other], 1), np.stack([other, near], 1), np.stack([near, rng.permutation(near)], 1)])
    u = _with_edges(rng, n)
    u[16:16 + len(special)] = special[:n - 32]
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    return p, u


def infinite_directions(light, seed, n=N):
    """Seeded unit directions (float32), then +z and -z of the light (in world space through l2w, float32), then directions
    with |y| <= 10^-7 and x > 0 in light space on either side of the seam."""
    rng = np.random.default_rng(seed)
    d = _dirs(rng, n)
    m = 64
    y = np.concatenate([rng.uniform(-1e-7, 1e-7, m - 3), [0.0, 1e-7, -1e-7]])
    th = np.arccos(rng.uniform(-0.95, 0.95, m))
    seam = np.stack([np.sin(th), y, np.cos(th)], 1)
    special = np.concatenate([[[0, 0, 1.0], [0, 0, -1.0]], seam]) @ light.l2w.T
    d[-len(special):] = special
    return d.astype(np.float32)


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)


def _frac(got, want, band):
    """|got - want| / band per sample (per coordinate for vectors, the largest); 0 where got equals want, band or no band. A
    float32 +inf stands for any value above the largest float32: it is no difference where the band reaches above that."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        bb = np.asarray(band, np.float64)
        same = (got == want) | (np.isposinf(got) & (want + (bb[..., None] if want.ndim == 2 and bb.ndim == 1 else bb) > FLT_MAX))
        diff = np.where(same, 0.0, np.abs(got - want))
    if diff.ndim == 2:
        diff = diff.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(diff == 0, 0.0, diff / band)
    return f


def check_area_sample(name, got, want):
    """got: (n, 13) {wi, Li, pdf, p, n} of a probe; want: AreaLight.sample_li's record. Returns the measured figures."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), name
    dead = np.asarray(want.pdf) == 0
    fig = {}
    fig["p"] = _frac(got[:, 7:10], want.p, want.band_p).max()
    fig["n"] = _frac(got[:, 10:13], want.n, want.band_n).max()
    live = ~dead
    fig["wi"] = _frac(got[live, 0:3], want.wi[live], want.band_wi[live]).max() if live.any() else 0.0
    cond = live & np.isfinite(want.band_pdf_rel)
    fig["pdf"] = _frac(got[cond, 6], want.pdf[cond], want.band_pdf_rel[cond] * np.abs(want.pdf[cond])).max() if cond.any() else 0.0
    out = want.side_flag | (live & ~cond)  # samples in the band of the side test (a cosine within its band of 0)
    fig["side_left_out"] = out.mean()
    assert fig["side_left_out"] <= CAP, (name, fig)
    # a dead sample (zero-length wi, or an infinite pdf) is dead on both sides, exactly; unless the truth's own cosine is in its band of 0
    assert (got[dead & ~out, 6] == 0).all() and (got[dead & ~out, 0:6] == 0).all(), name
    assert (got[cond, 6] > 0).all(), name
    keep = ~out
    assert np.array_equal(got[keep, 3:6], np.asarray(want.Li, np.float64)[keep]), name  # Lemit or black, exactly
    for k in ("p", "n", "wi", "pdf"):
        assert fig[k] <= 1.0, (name, k, fig)
    return fig


def check_area_pdf(name, got, want):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), name
    flag = want.edge_flag | ~np.isfinite(want.band_pdf_rel)
    fig = {"edge_left_out": flag.mean()}
    assert fig["edge_left_out"] <= CAP, (name, fig)
    k = ~flag
    miss = k & (np.asarray(want.pdf) == 0)
    assert (got[miss] == 0).all(), name
    hit = k & (np.asarray(want.pdf) > 0)
    fig["pdf"] = _frac(got[hit], want.pdf[hit], want.band_pdf_rel[hit] * want.pdf[hit]).max() if hit.any() else 0.0
    fig["hits"] = hit.mean()
    assert fig["pdf"] <= 1.0, (name, fig)
    return fig


def check_infinite_sample(name, got, want):
    """Sample_Li of the infinite light gets no allowance: nothing is left out. The direction within band_wi pins (d0, d1) to
    136 u, the pdf within its band pins func[col] / funcInt of the row and func[row] / funcInt of the marginal."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(np.delete(got, 6, axis=1)).all() and not np.isnan(got[:, 6]).any(), name
    dead = want.dead | (np.asarray(want.pdf) == 0)
    assert (got[want.dead] == 0).all(), name
    assert (got[dead, 6] == 0).all(), name
    live = ~want.dead
    fig = {"dead": dead.mean()}
    if live.any():
        fig["wi"] = _frac(got[live, 0:3], want.wi[live], want.band_wi[live]).max()
        fig["target"] = _frac(got[live, 7:10], want.target[live], want.band_target[live]).max()
        fig["L"] = _frac(got[live, 3:6], want.Li[live], want.band_L[live]).max()
        pos = ~dead
        fig["pdf"] = _frac(got[pos, 6], want.pdf[pos], want.band_pdf_rel[pos] * want.pdf[pos]).max() if pos.any() else 0.0
        assert (got[live, 10:13] == 0).all(), name
        for k in ("wi", "target", "L", "pdf"):
            assert fig[k] <= 1.0, (name, k, fig)
    return fig


def check_infinite_pdf(name, got, want):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), name
    fig = {"cell_left_out": want.cell_flag.mean()}
    assert fig["cell_left_out"] <= CAP, (name, fig)
    k = ~want.cell_flag
    zero = k & (np.asarray(want.pdf) == 0)
    assert (got[zero] == 0).all(), name
    pos = k & (np.asarray(want.pdf) != 0)
    fig["pdf"] = _frac(got[pos], want.pdf[pos], want.band_pdf_rel[pos] * np.abs(want.pdf[pos])).max() if pos.any() else 0.0
    assert fig["pdf"] <= 1.0, (name, fig)
    # a flagged direction: the pdf of one of the cells within the band of its (p0 w, p1 h), within the band of the pdf
    f = want.cell_flag
    near = np.abs(got[f, None] - want.pdf_alt[f]) <= want.band_pdf_rel[f, None] * np.abs(want.pdf_alt[f]) + 1e-300
    assert near.any(axis=1).all(), (name, got[f][~near.any(axis=1)][:4], want.pdf_alt[f][~near.any(axis=1)][:4])
    return fig


def check_infinite_le(name, got, want):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), name
    fig = {"L": _frac(got, want.L, want.band_L).max()}
    assert fig["L"] <= 1.0, (name, fig)
    return fig


# ---- what the two test files share ------------------------------------------------------------------------------------------------
AREA = [("sphere", c) for c in SPHERES] + [("triangle", c) for c in TRIANGLES]
ZERO = np.zeros_like  # the reference Interaction's normal: none


@pytest.fixture(scope="module")
def scenes(binding, tmp_path_factory):
    """load(kind, case) -> (HostScene, truth light), each scene written and loaded once."""
    root, cache = tmp_path_factory.mktemp("lightsample"), {}
    text = {"sphere": sphere_scene, "triangle": triangle_scene, "quadric": quadric_scene}
    truth = {"sphere": sphere_truth, "triangle": triangle_truth, "quadric": quadric_truth, "infinite": infinite_truth}

    def load(kind, case):
        if (kind, case) not in cache:
            body = infinite_scene(case, root) if kind == "infinite" else text[kind](case)
            path = root / f"{case}.pbrt"
            path.write_text(body)
            host = binding.HostScene(path=str(path))
            cache[kind, case] = (host, truth[kind](host, case))
        return cache[kind, case]
    return load


def _packed(w):
    return np.concatenate([w.wi, w.Li, w.pdf[:, None], w.p, w.n], 1)


def _pdf_directions(light, p, want, seed):
    """Pdf's directions for an area light: what Sample returned (a dead sample: a seeded direction instead), then for a triangle
    n / 4 seeded directions (most of which miss) and 48 aimed just inside and just outside each edge."""
    rng = np.random.default_rng(seed)
    wi = np.where((np.asarray(want.pdf) == 0)[:, None], _dirs(rng, len(p)), want.wi)
    if isinstance(light.shape, LS.Triangle):
        n = len(p)
        wi[n // 2:n // 2 + n // 4] = _dirs(rng, n // 4)
        v = light.shape.v
        k = 0
        for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            for off in (1e-7, -1e-7, 1e-3, -1e-3):  # the first two lie within the band of the edge: the flags' business
                for t in (0.2, 0.5, 0.7, 0.9):
                    q = v[a] + t * (v[b] - v[a]) + off * (v[c] - v[a])
                    i = n - 1 - 16 - k  # (not the sixteen at p0 at the front, whose directions would have no length)
                    wi[i] = q - p[i]
                    wi[i] /= np.linalg.norm(wi[i])
                    k += 1
    return wi.astype(np.float32)


def _area_case(scenes, kind, case):
    host, light = scenes(kind, case)
    if kind == "sphere":
        sets = [(f"{case}/outside",) + sphere_points(light, RATIOS_OUT, 1)[:2], (f"{case}/inside",) + sphere_points(light, RATIOS_IN, 2)[:2]]
    elif kind == "triangle":
        sets = [(case,) + triangle_points(light, 3)]
    else:
        sets = [(case,) + quadric_points(light, 4)]
    return host, light, sets
