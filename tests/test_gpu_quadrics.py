"""Disks and cylinders on the device (GPU): the traversal's Disk / Cylinder::Intersect(P) against the float64 restatement of
quadric_ref.py, the closed-can furnace (path integrator and probe pass: the shapes' Sample / Pdf through NEE and MIS), the
irradiance under a disk light (path integrator and the IISPT direct pass), and the C++ host."""
import os
import subprocess

import numpy as np
import pytest

from quadric_ref import GRAZING, Cylinder, Disk, decided, disk_irradiance_factor, matrix_text, rotate, scale, translate, write_scene

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = 100_000


def _rays(rng, center, extent, n=N_RAYS):
    """Rays from a sphere of radius 4 * extent around `center` towards points of the box around it."""
    u = rng.normal(size=(n, 3))
    o = center + 4 * extent * u / np.linalg.norm(u, axis=1, keepdims=True)
    target = center + extent * rng.uniform(-1, 1, size=(n, 3))
    d = target - o
    return o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


CASES = [
    ("disk", 'Shape "disk" "float height" [0.2] "float radius" [1.2]', lambda m: Disk(m, 0.2, 1.2)),
    ("disk_partial", 'Shape "disk" "float height" [-0.3] "float radius" [1] "float innerradius" [0.4] "float phimax" [250]',
     lambda m: Disk(m, -0.3, 1.0, 0.4, 250)),
    ("cylinder", 'Shape "cylinder" "float radius" [0.7] "float zmin" [-1] "float zmax" [1.5]', lambda m: Cylinder(m, 0.7, -1, 1.5)),
    ("cylinder_partial", 'Shape "cylinder" "float radius" [0.9] "float zmin" [-0.5] "float zmax" [0.8] "float phimax" [200]',
     lambda m: Cylinder(m, 0.9, -0.5, 0.8, 200)),
]
XFORMS = [translate(0.5, -0.25, 1) @ rotate(30, (1, 1, 0)) @ scale(1.5, 0.75, 1.25), rotate(-110, (0.2, 1, 0.4))]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
@pytest.mark.parametrize("xf", range(len(XFORMS)))
def test_trace_matches_restatement(binding, tmp_path, case, xf):
    name, line, make = CASES[case]
    m = XFORMS[xf]
    host = binding.HostScene(path=write_scene(tmp_path, 'Material "matte"\nAttributeBegin\n' + matrix_text(m) + "\n" + line + "\nAttributeEnd\n"))
    assert host.quadric_count == 1
    gpu = binding.GpuScene(host)
    rng = np.random.default_rng(1234 + 10 * case + xf)
    o, d = _rays(rng, m[:3, 3], 1.5)
    tmax = np.full(len(o), np.inf, np.float32)
    tmax[::3] = rng.uniform(1, 8, size=len(tmax[::3]))
    want, certain, cos = decided(make(m), o.astype(np.float64), d.astype(np.float64), tmax.astype(np.float64), 1e-4)
    near_tmax = np.isfinite(want) & (np.abs(np.where(np.isfinite(want), want, 0) - tmax) < 1e-4 * np.maximum(1, tmax))
    certain &= ~near_tmax
    assert certain.mean() > 0.97 and np.isfinite(want[certain]).mean() > 0.05
    for instrumented in (True, False):
        prim, tb, st = gpu.trace_closest(o, d, tmax, instrumented=instrumented)
        hit = prim >= 0
        assert (hit[certain] == np.isfinite(want[certain])).all(), (name, np.flatnonzero(certain & (hit != np.isfinite(want)))[:5])
        both = certain & hit & (cos > GRAZING)
        assert both.sum() > 1000 and np.allclose(tb[both, 0], want[both], rtol=1e-5, atol=0), np.abs(tb[both, 0] / want[both] - 1).max()
        if instrumented:
            assert st["sphere_tests"] > 0  # quadric tests are counted with the sphere tests
        any_hit, _ = gpu.trace_any(o, d, tmax, instrumented=instrumented)
        assert ((any_hit != 0)[certain] == np.isfinite(want[certain])).all()
    gpu.close()


MIXED = """Material "matte"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -1.5 -3  3 -1.5 -3  3 -1.5 3  -3 -1.5 3]
AttributeBegin
Translate -1 0.5 0.5
Shape "sphere" "float radius" [0.6]
AttributeEnd
AttributeBegin
{d0}
Shape "disk" "float radius" [1.1] "float innerradius" [0.3]
AttributeEnd
AttributeBegin
{d1}
Shape "disk" "float height" [0.4] "float radius" [0.8] "float phimax" [300]
AttributeEnd
AttributeBegin
{c0}
Shape "cylinder" "float radius" [0.5] "float zmin" [-1] "float zmax" [1]
AttributeEnd
AttributeBegin
{c1}
Shape "cylinder" "float radius" [0.35] "float zmin" [0] "float zmax" [2] "float phimax" [180]
AttributeEnd
"""
MIXED_XF = dict(d0=translate(0.5, 0, 0) @ rotate(70, (1, 0, 0)), d1=translate(-0.5, 1, -1) @ rotate(20, (0, 1, 1)),
                c0=translate(1, 0, 0.5) @ rotate(90, (1, 0, 0)), c1=translate(-0.3, -1, 1) @ rotate(-30, (0, 0, 1)) @ scale(1, 1.5, 1))


def _mixed_restated():
    return [Disk(MIXED_XF["d0"], 0, 1.1, 0.3), Disk(MIXED_XF["d1"], 0.4, 0.8, 0, 300), Cylinder(MIXED_XF["c0"], 0.5, -1, 1),
            Cylinder(MIXED_XF["c1"], 0.35, 0, 2, 180)]


def _sphere_t(o, d, c, r):
    oc = o - c
    b = np.sum(oc * d, axis=1)
    cc = np.sum(oc * oc, axis=1) - r * r
    disc = b * b - cc
    s = np.sqrt(np.maximum(disc, 0))
    t0, t1 = -b - s, -b + s
    t = np.where(t0 > 0, t0, np.where(t1 > 0, t1, np.inf))
    return np.where(disc >= 0, t, np.inf), np.abs(disc) < 1e-3, np.sqrt(np.maximum(disc, 0)) / r


def _plane_t(o, d, y, half):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (y - o[:, 1]) / d[:, 1]
    p = o + d * t[:, None]
    ok = (t > 0) & (np.abs(p[:, 0]) <= half) & (np.abs(p[:, 2]) <= half)
    edge = np.abs(np.abs(p[:, 0]) - half) < 1e-3
    edge |= np.abs(np.abs(p[:, 2]) - half) < 1e-3
    return np.where(ok, t, np.inf), edge & np.isfinite(t)


def _mixed_scene(binding, tmp_path, **kw):
    body = MIXED.format(**{k: matrix_text(v) for k, v in MIXED_XF.items()})
    return binding.HostScene(path=write_scene(tmp_path, body, name="mixed.pbrt"), **kw)


def test_mixed_bvh_returns_the_nearest_primitive(binding, tmp_path):
    host = _mixed_scene(binding, tmp_path)
    assert host.quadric_count == 4 and host.info["n_spheres"] == 1 and host.info["n_triangles"] == 2
    flags = host.prim_flags()
    _, _, shape = host.bvh()
    gpu = binding.GpuScene(host)
    rng = np.random.default_rng(77)
    o, d = _rays(rng, np.zeros(3), 2.0)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    inf = np.full(len(o), np.inf)
    ts, coss, certain = [], [], np.ones(len(o), bool)
    for q in _mixed_restated():
        t, c, cos = decided(q, o64, d64, inf, 1e-4)
        ts.append(t)
        coss.append(cos)
        certain &= c
    t, edge, cos = _sphere_t(o64, d64, np.array([-1, 0.5, 0.5]), 0.6)
    ts.append(t)
    coss.append(cos)
    certain &= ~edge
    t, edge = _plane_t(o64, d64, -1.5, 3.0)
    ts.append(t)
    coss.append(np.abs(d64[:, 1]))
    certain &= ~edge
    ts = np.stack(ts)  # rows: 4 quadrics (in scene order), sphere, plane
    order = np.sort(ts, axis=0)
    with np.errstate(invalid="ignore"):  # (inf - inf where a ray hits nothing)
        certain &= ~(np.isfinite(order[0]) & (order[1] - order[0] < 1e-4 * np.maximum(order[0], 1)))
    nearest = np.argmin(ts, axis=0)
    want = order[0]
    steep = np.take_along_axis(np.stack(coss), nearest[None], axis=0)[0] > GRAZING
    assert certain.mean() > 0.95
    prim, tb, _ = gpu.trace_closest(o, d, np.full(len(o), np.inf, np.float32), instrumented=False)
    hit = prim >= 0
    assert (hit[certain] == np.isfinite(want[certain])).all()
    both = certain & hit
    assert np.allclose(tb[both & steep, 0], want[both & steep], rtol=1e-5, atol=0)
    # the primitive is the restatement's nearest: its kind, and for the quadrics which one
    pf, ps = flags[prim[both]], shape[prim[both]]
    kind = np.where(pf & binding.PRIM_QUADRIC, ps, np.where(pf & binding.PRIM_SPHERE, 4, 5))
    assert (kind == nearest[both]).all()
    # the device-built tree (HLBVH on the GPU) finds the same hits, t bit for bit
    dev_host = _mixed_scene(binding, tmp_path, accel_split="hlbvh", bvh_on_device=True)
    dev = binding.GpuScene(dev_host)
    prim2, tb2, _ = dev.trace_closest(o, d, np.full(len(o), np.inf, np.float32), instrumented=False)
    assert ((prim2 >= 0) == hit).all() and (tb2[hit, 0].view(np.uint32) == tb[hit, 0].view(np.uint32)).all()
    gpu.close()
    dev.close()


def _can(le, kd, depth, integrator="path", w=24, h=24, spp=16):
    """A closed can of two-sided emitting matte walls around the camera: a cylinder of radius 1 and two caps slightly larger than
    it, the wall slightly longer than the caps are apart (no seam to leak through)."""
    mat = f'Material "matte" "rgb Kd" [{kd} {kd} {kd}]\nAreaLightSource "diffuse" "rgb L" [{le} {le} {le}] "bool twosided" "true"\n'
    body = (mat + 'Shape "cylinder" "float radius" [1] "float zmin" [-1.05] "float zmax" [1.05]\n'
            'Shape "disk" "float height" [-1] "float radius" [1.05]\n'
            'Shape "disk" "float height" [1] "float radius" [1.05]\n')
    return dict(body=body, w=w, h=h, spp=spp, depth=depth, fov=90, eye="0 0 0", look="0.3 0.2 1", integrator=integrator)


@pytest.mark.parametrize("depth,kd", [(1, 0.5), (3, 0.7)])
def test_closed_can_furnace(binding, tmp_path, depth, kd):
    le = 0.8
    kw = _can(le, kd, depth)
    host = binding.HostScene(path=write_scene(tmp_path, kw.pop("body"), **kw))
    assert host.info["n_lights"] == 3 and host.quadric_count == 3
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    rgb = host.film_to_rgb(film)[..., 0].astype(np.float64)
    want = le * sum(kd ** k for k in range(depth + 1))
    se = rgb.std() / np.sqrt(rgb.size)
    assert abs(rgb.mean() - want) < 5 * se + 1e-4, (rgb.mean(), want, se)
    gpu.close()


def test_closed_can_furnace_probe(binding, tmp_path):
    """The probe pass (IISPTdIntegrator::Li, maxdepth 3) from inside the can: the camera ray's own vertex is left out
    (iispt_d.cpp:116-123), so each probe pixel sees L (a + a^2 + a^3)."""
    le, kd = 0.8, 0.6
    kw = _can(le, kd, 3)
    host = binding.HostScene(path=write_scene(tmp_path, kw.pop("body"), **kw))
    gpu = binding.GpuScene(host)
    inten, _, dist, _ = gpu.render_probes(np.array([[0.1, -0.2, 0.3], [0, 0, -0.5]]), np.array([[0, 0, 1], [0.6, 0.8, 0]]))
    v = inten[..., 0].astype(np.float64)
    seen = dist > 0
    assert seen.mean() > 0.5
    want = le * (kd + kd ** 2 + kd ** 3)
    se = v[seen].std() / np.sqrt(seen.sum())
    assert abs(v[seen].mean() - want) < 5 * se + 1e-4, (v[seen].mean(), want, se)
    gpu.close()


H_LIGHT, R_LIGHT, CAM_H, RES, FOV = 1.0, 0.6, 4.0, 48, 60


def _disk_light_scene(tmp_path, reverse=False, integrator="path", spp=64, swap=True):
    """A one-sided disk light over a matte plane (Kd 0.5), the camera above looking down. (The reference's disk has its hit
    normal along -z and its sampled normal along +z in object space, disk.cpp:78-80 and :133. swap: under a handedness-swapping
    Scale 1 1 -1 both come out facing down, and the light is the same from both halves of MIS; without it (a plain rotation) the
    sampled normal faces down and the hit normal up, so only light sampling sees the light, and with ReverseOrientation only
    BSDF sampling: test_one_sided_disk_light_halves.)"""
    xf = "Rotate -90 1 0 0\nScale 1 1 -1" if swap else "Rotate 90 1 0 0"
    body = f"""Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-20 0 -20  20 0 -20  20 0 20  -20 0 20]
AttributeBegin
Translate 0 {H_LIGHT} 0
{xf}
{"ReverseOrientation" if reverse else ""}
AreaLightSource "diffuse" "rgb L" [2 2 2]
Shape "disk" "float radius" [{R_LIGHT}]
AttributeEnd
"""
    return write_scene(tmp_path, body, name=f"disklight_{int(reverse)}_{int(swap)}_{integrator}.pbrt", w=RES, h=RES, spp=spp, depth=1,
                       fov=FOV, eye=f"0 {CAM_H} 0", look="0 0 0", up="0 0 1", integrator=integrator)


def _pixel_rho(fn=None, res=RES, fov=FOV, cam_h=CAM_H):
    """Distance from the axis of the plane point each pixel sees (camera cam_h above the plane, looking down the axis),
    averaged over an 8 x 8 grid inside the pixel (the box filter), and fn(rho) averaged the same way (default: the
    analytic Kd L F(h, rho) under the disk light)."""
    if fn is None:
        fn = lambda r: 0.5 * 2 * disk_irradiance_factor(H_LIGHT, r, R_LIGHT)
    t = np.tan(np.radians(fov / 2))
    sub = (np.arange(8) + 0.5) / 8
    px = (np.arange(res)[:, None] + sub[None, :]).reshape(-1)
    s = (-1 + 2 * px / res) * t * cam_h
    x, z = np.meshgrid(s, s)
    rho = np.hypot(x, z)
    f = fn(rho)
    return rho.reshape(res, 8, res, 8).mean(axis=(1, 3)), f.reshape(res, 8, res, 8).mean(axis=(1, 3))


def _check_irradiance(img, fn=None, bands=None):
    rho, want = _pixel_rho(fn)
    sil = R_LIGHT * CAM_H / (CAM_H - H_LIGHT)  # the disk's silhouette on the plane
    for lo, hi in bands or ((sil + 0.1, 1.2), (1.2, 1.6), (1.6, 2.2)):
        sel = (rho > lo) & (rho < hi)
        ratio = img[sel] / want[sel]
        se = ratio.std() / np.sqrt(sel.sum())
        assert sel.sum() > 50 and abs(ratio.mean() - 1) < 5 * se + 0.01, (lo, hi, ratio.mean(), se)


def test_disk_light_irradiance(binding, tmp_path):
    host = binding.HostScene(path=_disk_light_scene(tmp_path))
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    _check_irradiance(host.film_to_rgb(film)[..., 1].astype(np.float64))
    gpu.close()
    # flipped with ReverseOrientation, the disk emits upwards: the plane is black
    host = binding.HostScene(path=_disk_light_scene(tmp_path, reverse=True))
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    img = host.film_to_rgb(film)[..., 1]
    rho, _ = _pixel_rho()
    assert (img[rho > R_LIGHT * CAM_H / (CAM_H - H_LIGHT) + 0.1] == 0).all()
    gpu.close()


def test_disk_light_irradiance_direct_pass(binding, tmp_path):
    host = binding.HostScene(path=_disk_light_scene(tmp_path, integrator="iispt", spp=1))
    gpu = binding.GpuScene(host)
    mon = gpu.render_direct(48)
    _check_irradiance(mon[..., 1] / mon[..., 3])
    gpu.close()


def test_cli_renders_the_binding_film(binding, tmp_path):
    """`iile_pbrt` (GpuPathIntegrator) renders a quadric scene to the film the Python binding does, bit for bit."""
    path = _disk_light_scene(tmp_path, spp=4)
    out = tmp_path / "cli.pfm"
    exe = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
    p = subprocess.run([exe, path, "--outfile", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    raw = out.read_bytes()
    head = f"PF\n{RES} {RES}\n-1.0\n".encode()
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], "<f4").reshape(RES, RES, 3)[::-1]
    host = binding.HostScene(path=path)
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    assert (img.view(np.uint32) == host.film_to_rgb(film).view(np.uint32)).all()
    gpu.close()


# ---- one-sided lights without a handedness swap --------------------------------------------------------------------------------
def _disk_halves(rho, nee):
    """What each half of EstimateDirect brings a plane point rho off the axis under the facing disk light (Kd L = 1), by quadrature
    over the disk: Kd / pi L integral of cos cos' / d^2 times the power heuristic's weight of that half, light sampling's pdf being
    d^2 / (cos' A) (uniform over the disk's area) and BSDF sampling's cos / pi."""
    rho = np.asarray(rho, float)
    flat = rho.reshape(-1)
    table_rho = np.linspace(0, flat.max() + 1e-6, 256)
    nr, nphi = 200, 256
    rr = (np.arange(nr) + 0.5) / nr * R_LIGHT
    ph = (np.arange(nphi) + 0.5) / nphi * 2 * np.pi
    r2, p2 = np.meshgrid(rr, ph, indexing="ij")
    da = (R_LIGHT / nr) * (2 * np.pi / nphi) * r2
    area = np.pi * R_LIGHT ** 2
    vals = []
    for q in table_rho:
        d2 = H_LIGHT ** 2 + q * q + r2 * r2 - 2 * q * r2 * np.cos(p2)
        cos = H_LIGHT / np.sqrt(d2)
        pl, pb = d2 / (cos * area), cos / np.pi
        w = pl * pl / (pl * pl + pb * pb) if nee else pb * pb / (pl * pl + pb * pb)
        vals.append(np.sum(cos * cos / d2 * w * da) / np.pi)
    return np.interp(flat, table_rho, vals).reshape(rho.shape)


def test_one_sided_disk_light_halves(binding, tmp_path):
    """A one-sided disk light under a plain rotation (no handedness swap): Disk::Sample's normal faces the plane and the hit's
    normal faces away, so the plane gets light sampling's MIS-weighted half only; with ReverseOrientation, BSDF sampling's half
    only. Each matches its quadrature, and the two add up to the disk's analytic irradiance."""
    halves = []
    for reverse, nee in ((False, True), (True, False)):
        host = binding.HostScene(path=_disk_light_scene(tmp_path, reverse=reverse, swap=False))
        gpu = binding.GpuScene(host)
        film, _ = gpu.render()
        img = host.film_to_rgb(film)[..., 1].astype(np.float64)
        _check_irradiance(img, lambda r, nee=nee: _disk_halves(r, nee))
        halves.append(img)
        gpu.close()
    _check_irradiance(halves[0] + halves[1])


def test_one_sided_cylinder_light(binding, tmp_path):
    """An open can whose wall (radius 1, height 1.5, no handedness swap) is a one-sided light facing inwards (ReverseOrientation):
    a point of the matte floor rho off the axis sees the wall wherever it does not see the opening, so its radiance is
    Kd L (1 - F(1.5, rho, 1)), F the view factor of the opening (the disk formula). Light sampling and BSDF sampling both see the
    wall's inner side: the cylinder's sampled and hit normals agree."""
    hc, cam = 1.5, 1.4
    body = """AttributeBegin
Material "matte" "rgb Kd" [0 0 0]
ReverseOrientation
AreaLightSource "diffuse" "rgb L" [2 2 2]
Shape "cylinder" "float radius" [1] "float zmin" [-0.05] "float zmax" [1.5]
AttributeEnd
Material "matte" "rgb Kd" [0.5 0.5 0.5]
Shape "disk" "float radius" [1.05]
"""
    path = write_scene(tmp_path, body, name="can_light.pbrt", w=RES, h=RES, spp=64, depth=1, fov=FOV, eye=f"0 0 {cam}", look="0 0 0",
                       up="0 1 0")
    host = binding.HostScene(path=path)
    assert host.light(0).type == binding.LIGHT_AREA_QUADRIC and not host.light(0).two_sided
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    img = host.film_to_rgb(film)[..., 1].astype(np.float64)
    rho, want = _pixel_rho(lambda r: 0.5 * 2 * (1 - disk_irradiance_factor(hc, r, 1.0)), cam_h=cam)
    for lo, hi in ((0, 0.4), (0.4, 0.7), (0.7, 0.9)):
        sel = (rho > lo) & (rho < hi)
        ratio = img[sel] / want[sel]
        se = ratio.std() / np.sqrt(sel.sum())
        assert sel.sum() > 50 and abs(ratio.mean() - 1) < 5 * se + 0.01, (lo, hi, ratio.mean(), se)
    gpu.close()


# ---- hit attributes, textures, bump maps ---------------------------------------------------------------------------------------
def _xf_normal(m, v):
    return v @ np.linalg.inv(m)[:3, :3]  # (M^-1)^T v, row by row


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


ATTR_CASES = [("disk", CASES[1][1], CASES[1][2]), ("cylinder", CASES[3][1], CASES[3][2])]


@pytest.mark.parametrize("case", range(len(ATTR_CASES)), ids=[c[0] for c in ATTR_CASES])
@pytest.mark.parametrize("orient", ["plain", "reverse", "swap"])
def test_hit_attributes_match_restatement(binding, tmp_path, case, orient):
    """(u, v), dp/du, dp/dv, dn/du, dn/dv, the normals and `flip` of quadric hits (shape_hit_interaction<DIFFS = true>: what
    textures, Material::Bump and the direct pass's differentials read) against disk.cpp:73-92 / cylinder.cpp:105-139 restated."""
    name, line, make = ATTR_CASES[case]
    m = XFORMS[0] @ (scale(1, 1, -1) if orient == "swap" else np.eye(4))
    rev = orient == "reverse"
    text = 'Material "matte"\nAttributeBegin\n' + matrix_text(m) + ("\nReverseOrientation\n" if rev else "\n") + line + "\nAttributeEnd\n"
    host = binding.HostScene(path=write_scene(tmp_path, text))
    gpu = binding.GpuScene(host)
    shape = make(m)
    rng = np.random.default_rng(99 + case)
    o, d = _rays(rng, m[:3, 3], 1.5, n=20000)
    want_t, certain, cos = decided(shape, o.astype(np.float64), d.astype(np.float64), np.full(len(o), np.inf), 1e-3)
    prim, tb, _ = gpu.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    sel = certain & (prim >= 0) & np.isfinite(want_t) & (cos > GRAZING)
    _, p, _ = shape.intersect(o[sel].astype(np.float64), d[sel].astype(np.float64), np.full(sel.sum(), np.inf))
    if name == "disk":
        sel_far = np.hypot(p[:, 0], p[:, 1]) > 0.5  # (u = phi / phiMax is ill-conditioned near the centre)
    else:
        sel_far = np.ones(len(p), bool)
    idx = np.flatnonzero(sel)[sel_far]
    p = p[sel_far]
    assert len(idx) > 1000
    a = gpu.shape_hit_attributes(o[idx], d[idx], prim[idx])
    phi = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2 * np.pi)
    zero = np.zeros(len(p))
    dpdu = np.stack([-shape.phimax * p[:, 1], shape.phimax * p[:, 0], zero], 1)
    if name == "disk":
        r = np.hypot(p[:, 0], p[:, 1])
        u, v = phi / shape.phimax, 1 - (r - shape.inner) / (shape.radius - shape.inner)
        dpdv = np.stack([p[:, 0], p[:, 1], zero], 1) * ((shape.radius - shape.inner) / r)[:, None]
        dndu = dndv = np.zeros_like(dpdu)
    else:
        u, v = phi / shape.phimax, (p[:, 2] - shape.zmin) / (shape.zmax - shape.zmin)
        dpdv = np.stack([zero, zero, zero + (shape.zmax - shape.zmin)], 1)
        dndu, dndv = dpdu / shape.radius, np.zeros_like(dpdu)  # -e / E dp/du with e = N . d2P/du2 = -phiMax^2 r, E = phiMax^2 r^2
    flip = rev ^ (orient == "swap")
    n = _unit(np.cross(dpdu, dpdv)) * (-1 if flip else 1)
    world = lambda vec: vec @ m[:3, :3].T
    tol = dict(rtol=1e-4, atol=1e-4)
    assert (a["flip"] == flip).all()
    assert np.allclose(a["u"], u, **tol) and np.allclose(a["v"], v, **tol), (np.abs(a["u"] - u).max(), np.abs(a["v"] - v).max())
    assert np.allclose(a["p"], o[idx] + d[idx] * tb[idx, :1], rtol=1e-5, atol=1e-5)
    # (the derivatives are evaluated at the device's float32 hit point and the restatement's float64 one: they differ by ~1e-5
    # of the shape's size, scaled by phiMax and the transform; a swapped or mis-signed derivative is off by its own size)
    for k, want in (("dpdu", world(dpdu)), ("dpdv", world(dpdv)), ("dndu", _xf_normal(m, dndu)), ("dndv", _xf_normal(m, dndv))):
        scl = max(np.abs(want).max(), np.abs(world(dpdu)).max() / shape.radius)
        assert np.allclose(a[k], want, rtol=0, atol=1e-4 * scl), (k, np.abs(a[k] - want).max(), scl)
    nw = _unit(_xf_normal(m, n))  # (a cylinder's normal follows the hit point: the same float32 / float64 difference as above)
    assert np.allclose(a["n"], nw, atol=2e-4), np.abs(a["n"] - nw).max()
    assert np.allclose(a["sn"], nw, atol=2e-4)  # no bump map: the shading normal is the geometric one
    gpu.close()


BLOCK_COLORS = np.array([[0.8, 0.1, 0.1], [0.1, 0.8, 0.1], [0.1, 0.1, 0.8], [0.8, 0.8, 0.1]], np.float32)


def _write_pfm(path, rows):
    """rows[r, c]: RGB texel r of the FILE (a PFM's first row is the image's bottom scanline)."""
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


def _blocks_texture(tmp_path):
    """16 x 16 texels in 2 x 2 blocks of 8 x 8: texel (s, t) of ImageTexture (t = 0 at the bottom, imagemap.cpp:67-74) has the
    colour of block (floor(2 s), floor(2 t))."""
    rows = np.zeros((16, 16, 3), np.float32)
    for bt in range(2):
        for bs in range(2):
            rows[8 * bt:8 * bt + 8, 8 * bs:8 * bs + 8] = BLOCK_COLORS[2 * bt + bs]
    _write_pfm(tmp_path / "blocks.pfm", rows)
    _write_pfm(tmp_path / "zero.pfm", np.zeros((4, 4, 3), np.float32))


def _textured_scene(tmp_path, shape_line, xform, bump=False, name="tex.pbrt"):
    """A matte shape with the block texture as Kd under a constant infinite light (L = 1) at maxdepth 1: nothing shadows the
    hemisphere a visible point faces, so a pixel's expected value is its texel."""
    body = f"""LightSource "infinite" "rgb L" [1 1 1]
Texture "blocks" "spectrum" "imagemap" "string filename" ["blocks.pfm"]
Texture "zero" "float" "imagemap" "string filename" ["zero.pfm"]
AttributeBegin
{xform}
Material "matte" "texture Kd" "blocks" {'"texture bumpmap" "zero"' if bump else ''}
{shape_line}
AttributeEnd
"""
    return write_scene(tmp_path, body, name=name, w=64, h=64, spp=128, depth=1, fov=50, eye="0 0 -4", look="0 0 0", up="0 1 0")


TEX_CASES = [("disk", 'Shape "disk" "float radius" [1.4]', "Rotate 180 0 1 0", lambda m: Disk(m, 0, 1.4)),
             ("cylinder", 'Shape "cylinder" "float radius" [1] "float zmin" [-1.2] "float zmax" [1.2]', "Rotate -90 1 0 0",
              lambda m: Cylinder(m, 1.0, -1.2, 1.2))]


@pytest.mark.parametrize("case", range(len(TEX_CASES)), ids=[c[0] for c in TEX_CASES])
def test_image_texture_on_quadrics(binding, tmp_path, case):
    """A textured disk seen head-on and a textured cylinder seen from the side: every pixel well inside a block of the texture
    (by the restatement's (u, v) of the ray through the pixel centre) shows that block's colour."""
    name, line, xform, make = TEX_CASES[case]
    _blocks_texture(tmp_path)
    m = rotate(180, (0, 1, 0)) if name == "disk" else rotate(-90, (1, 0, 0))
    host = binding.HostScene(path=_textured_scene(tmp_path, line, xform))
    gpu = binding.GpuScene(host)
    film, _ = gpu.render()
    img = host.film_to_rgb(film).reshape(-1, 3)
    py, px = np.mgrid[0:64, 0:64]
    o, d = gpu.camera_rays(np.stack([px.reshape(-1) + 0.5, py.reshape(-1) + 0.5], 1))
    shape = make(m)
    t, p, cos = shape.intersect(o.astype(np.float64), d.astype(np.float64), np.full(len(o), np.inf))
    phi = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2 * np.pi)
    if name == "disk":
        s_, t_ = phi / shape.phimax, 1 - np.hypot(p[:, 0], p[:, 1]) / shape.radius
        inner = t_ < 0.8  # (u = phi / phiMax changes fast near the centre: the filter's footprint spans blocks there)
    else:
        s_, t_ = phi / shape.phimax, (p[:, 2] - shape.zmin) / (shape.zmax - shape.zmin)
        inner = cos > 0.5
    margin = 0.08
    away = lambda c: (np.abs(c - 0.5) > margin) & (c > margin) & (c < 1 - margin)
    sel = np.isfinite(t) & inner & away(s_) & away(t_)
    assert sel.sum() > 100, sel.sum()
    block = 2 * (t_[sel] >= 0.5).astype(int) + (s_[sel] >= 0.5).astype(int)
    got = np.argmin(((img[sel][:, None, :] - BLOCK_COLORS[None]) ** 2).sum(-1), axis=1)
    assert (got == block).mean() > 0.99, ((got == block).mean(), np.bincount(block, minlength=4))
    for b in np.unique(block):
        mean = img[sel][block == b].mean(axis=0)
        assert np.allclose(mean, BLOCK_COLORS[b], atol=0.03), (b, mean)
    # a bump map that displaces nothing: Material::Bump rebuilds shading.n as Normalize(Cross(dpdu, dpdv)) (material.cpp:72-86),
    # where the interaction's normal was normalised once in object space and once after the transform — the two agree to
    # rounding, not always bit for bit (as in the reference) — so the films agree to rounding
    host_b = binding.HostScene(path=_textured_scene(tmp_path, line, xform, bump=True, name="tex_bump.pbrt"))
    gpu_b = binding.GpuScene(host_b)
    film_b, _ = gpu_b.render()
    img_b = host_b.film_to_rgb(film_b).reshape(-1, 3)
    assert np.isfinite(img_b).all()
    assert np.allclose(img_b, img, rtol=1e-3, atol=1e-4), np.abs(img_b - img).max()
    gpu.close()
    gpu_b.close()


def test_iispt_frame_on_a_quadric_scene(binding, tmp_path):
    """The IISPT frame (iispt_frame.py: hemi points, probe pass, network, gather, direct passes, merge) completes on the disk-light
    scene, and its direct part is the disk's analytic irradiance."""
    import importlib
    import sys
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    sys.path.insert(0, REPO)
    nn_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_nn")
    frame_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_frame")
    import iispt_torch_reference as ref_mod
    torch.manual_seed(5)
    host = binding.HostScene(path=_disk_light_scene(tmp_path, integrator="iispt", spp=1))
    gpu = binding.GpuScene(host)
    frame = frame_mod.IisptFrame(binding, gpu, nn_mod.IisptPipeline(gpu, net=ref_mod.IISPTNet().eval()))
    frame.run_batched(6, radius_start=8.0)
    frame.run_direct(48)
    torch.cuda.synchronize()
    assert frame.stats["tasks"] == 6 and frame.stats["probes"] > 0
    assert np.isfinite(frame.image().cpu().numpy()).all()
    _check_irradiance(frame.direct_image().cpu().numpy()[..., 1].astype(np.float64))
    gpu.close()
