"""The projection and goniometric lights on the device (GPU), held to the float64 restatement of imagelight_ref.py: the light
alone through the `light_sample_li` probe; bit-for-bit identities with a point light on every render path; each light through
a matte plane under the path integrator and the IISPT direct pass; an occluder; the three light strategies; the probe pass,
the gather and the IISPT frame; and the C++ host."""
import os
import subprocess

import numpy as np
import pytest

import imagelight_ref as IL
from quadric_ref import rotate, translate
from test_gpu_translucent import _bits, _counters, _iispt_image, _iispt_modules
from test_image_light_scenes import PLANE, light_text, restated, write_map, write_scene

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
N_POINTS = 100_000
KD = 0.5  # Material "matte"'s default Kd


def _close(got, want, rtol, floor):
    return np.abs(got - want) <= rtol * np.abs(want) + floor


def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ---- the light alone ------------------------------------------------------------------------------------------------------------
def _place(ref, rng, d_light):
    """Points at the light-space directions d_light from the light, at distances over three decades, as the float32 the probe
    takes."""
    r = 10 ** rng.uniform(-2, 1, len(d_light))
    return (ref.p_light[None, :] + r[:, None] * (d_light @ ref.l2w[:3, :3].T)).astype(np.float32)


def projection_points(ref, rng, n=N_POINTS):
    """Three quarters aimed at and around the projection window (15 % of those from behind the light), a quarter anywhere on
    the sphere; by construction none projects into the band between 0.98 and 1.02 of screenBounds, none has wl.z within 1 % of
    hither."""
    m = 2 * n
    k = 1 / np.tan(np.radians(ref.fov) / 2)
    bx, by = ref.screen_bounds[2], ref.screen_bounds[3]
    q = rng.uniform(-1.25, 1.25, (m, 2)) * np.array([bx, by])
    aimed = np.stack([q[:, 0] / k, q[:, 1] / k, np.ones(m)], 1) * np.where(rng.random(m) < 0.15, -1.0, 1.0)[:, None]
    d = np.where((np.arange(m) % 4 == 3)[:, None], _dirs(rng, m), aimed / np.linalg.norm(aimed, axis=1, keepdims=True))
    rel = np.maximum(np.abs(k * d[:, 0] / d[:, 2]) / bx, np.abs(k * d[:, 1] / d[:, 2]) / by)
    keep = ((rel < 0.975) | (rel > 1.025)) & (np.abs(d[:, 2] / IL.HITHER - 1) > 0.02)
    return _place(ref, rng, d[keep][:n])


def goniometric_points(ref, rng, n=N_POINTS):
    """Anywhere on the sphere, plus 0.5 % within 0.01 .. 0.05 of each pole of theta (the light's +y and -y) and 1 % within 0.01
    of the phi seam, on both sides of it."""
    d = _dirs(rng, n)
    n_pole, n_seam = n // 200, n // 100
    theta = np.concatenate([rng.uniform(0.01, 0.05, n_pole), np.pi - rng.uniform(0.01, 0.05, n_pole), np.arccos(rng.uniform(-1, 1, n_seam))])
    phi = np.concatenate([rng.uniform(0, 2 * np.pi, 2 * n_pole), rng.uniform(-0.01, 0.01, n_seam)])
    wp = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], 1)
    d[:len(wp)] = wp[:, [0, 2, 1]]  # Scale() swaps y and z before it takes the angles
    return _place(ref, rng, d)


CASES = {  # kind, map, fov
    "projection_wide": ("projection", "wide", None), "projection_tall": ("projection", "tall", 70.0),
    "projection_nomap": ("projection", None, None), "goniometric": ("goniometric", "gonio", None),
    "goniometric_tall": ("goniometric", "tall", None), "goniometric_nomap": ("goniometric", None, None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_light_sample_li_matches_restatement(binding, tmp_path, case):
    kind, which, fov = CASES[case]
    image = write_map(tmp_path, which) if which else None
    host = binding.HostScene(path=write_scene(tmp_path, light_text(kind, f"{which}.pfm" if which else None, fov=fov) + 'Material "matte"\n' + PLANE))
    gpu = binding.GpuScene(host)
    ref = restated(kind, image, fov=fov or 45.0)
    rng = np.random.default_rng(list(CASES).index(case))
    p = projection_points(ref, rng) if kind == "projection" else goniometric_points(ref, rng)
    assert len(p) == N_POINTS
    out = gpu.light_sample_li(0, p).astype(np.float64)
    gpu.close()
    wi, want, pdf = ref.sample_li(p.astype(np.float64))
    # the point set is what the docstrings above say, checked on the float32 points with the restatement alone
    r = np.linalg.norm(p.astype(np.float64) - ref.p_light, axis=1)
    assert r.min() < 0.02 and r.max() > 5
    if kind == "projection":
        z, q = ref.project(-wi)
        front = z > 0
        rel = np.maximum(np.abs(q[:, 0]) / ref.screen_bounds[2], np.abs(q[:, 1]) / ref.screen_bounds[3])
        assert ((rel[front] < 0.98) | (rel[front] > 1.02)).all() and (np.abs(z / IL.HITHER - 1) > 0.01).all()
        lit = want.max(axis=1) > 0
        assert lit.mean() > 1 / 3 and (~lit).mean() > 1 / 3, lit.mean()
        assert (~front).mean() > 0.1
    else:
        theta, phi = ref.angles(-wi)
        quadrant = (phi // (np.pi / 2)).astype(int)
        assert all((quadrant == k).mean() > 0.2 for k in range(4))
        assert (theta < 0.05).sum() > 100 and (theta > np.pi - 0.05).sum() > 100
        assert (phi < 0.01).sum() > 100 and (phi > 2 * np.pi - 0.01).sum() > 100
        assert (want > 0).all()
    assert np.isfinite(out).all()
    assert (out[:, 6] == 1).all() and (pdf == 1).all()
    assert np.abs(out[:, :3] - wi).max() < 1e-6
    scale = np.abs(want).max()
    ok = _close(out[:, 3:6], want, 1e-4, 1e-7 * scale).all(axis=1)
    worst = np.abs(out[:, 3:6] - want) / (np.abs(want) + 1e-6 * scale / 2e-3)
    print(f"{case}: inside the narrow band {ok.mean():.6f}, worst relative error {worst.max():.3e}")
    assert ok.mean() >= 0.9995, ok.mean()
    assert _close(out[:, 3:6], want, 2e-3, 1e-6 * scale).all()


def test_light_sample_li_refuses_other_lights(binding, tmp_path):
    body = ('LightSource "point" "rgb I" [1 2 3] "point from" [0 0 2]\nLightSource "infinite" "rgb L" [1 1 1]\nMaterial "matte"\n' + PLANE)
    gpu = binding.GpuScene(binding.HostScene(path=write_scene(tmp_path, body)))
    out = gpu.light_sample_li(0, np.array([[0, 0, 0], [1, 0, 2]], np.float32))
    assert np.allclose(out, [[0, 0, 1, .25, .5, .75, 1], [-1, 0, 0, 1, 2, 3, 1]])
    for light in (1, 2, -1):
        with pytest.raises(RuntimeError):
            gpu.light_sample_li(light, np.zeros((1, 3), np.float32))
    gpu.close()


# ---- identities with a point light, bit for bit ----------------------------------------------------------------------------------
ROOM = ('LightSource "infinite" "rgb L" [0.2 0.2 0.3]\nMaterial "matte" "rgb Kd" [0.5 0.4 0.3]\n' + PLANE +
        'AttributeBegin\nMaterial "plastic"\nTranslate 0 0 0.6\nShape "sphere" "float radius" [0.5]\nAttributeEnd\n'
        'AttributeBegin\nMaterial "matte" "rgb Kd" [0.6 0.3 0.2]\nTranslate 1.2 0.5 0.4\nShape "sphere" "float radius" [0.4]\nAttributeEnd\n')
ROOM_VIEW = dict(w=32, h=32, fov=50, eye="0 -4 2", look="0 0 0.3", up="0 0 1")


def _room_pair(tmp_path, **kw):
    """The room under a goniometric light without a map, and under the point light with the same I, scale and transform."""
    opts = dict(ROOM_VIEW, spp=2, depth=4)
    opts.update(kw)
    return [write_scene(tmp_path, light_text(kind) + ROOM, name=f"{kind}.pbrt", **opts) for kind in ("goniometric", "point")]


@pytest.mark.parametrize("collect", [False, True])
def test_goniometric_without_map_is_a_point_light_path_integrator(binding, tmp_path, collect):
    out = []
    for path in _room_pair(tmp_path):
        gpu = binding.GpuScene(binding.HostScene(path=path))
        out.append(gpu.render(collect_stats=collect))
        gpu.close()
    (fa, sa), (fb, sb) = out
    assert fa.max() > 0 and np.array_equal(_bits(fa), _bits(fb))
    if collect:
        assert _counters(sa) == _counters(sb)


def test_goniometric_without_map_is_a_point_light_direct_and_probe_passes(binding, tmp_path):
    pos = np.array([[0, -1, 0.01], [0.5, -0.5, 0.3], [0, -0.5, 0.6], [0.2, 0.2, 1.5]])
    dirs = np.array([[0, 0, 1], [0, -0.6, 0.8], [0, -1, 0], [0, 0, -1]])
    films, probes = [], []
    for path in _room_pair(tmp_path, integrator="iispt"):
        gpu = binding.GpuScene(binding.HostScene(path=path))
        films.append(gpu.render_direct(4))
        probes.append(gpu.render_probes(pos, dirs))
        gpu.close()
    assert films[0].max() > 0 and np.array_equal(films[0], films[1])
    a, b = probes
    assert a[0].max() > 0
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(_bits(x), _bits(y))
    assert _counters(a[3]) == _counters(b[3])


def test_goniometric_without_map_is_a_point_light_iispt_frame(binding, tmp_path):
    _iispt_modules()
    a, b = [_iispt_image(binding, p) for p in _room_pair(tmp_path, integrator="iispt", spp=1)]
    assert a.max() > 0 and np.array_equal(_bits(a), _bits(b))


SMALL_QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-0.4 -0.4 0  0.4 -0.4 0  0.4 0.4 0  -0.4 0.4 0]\n'
ABOVE = "Translate 0.1 -0.05 2.5\nRotate 180 1 0 0\nRotate 30 0 0 1\n"  # looking straight down: the quad lies inside 0.9 of the window


@pytest.mark.parametrize("integrator", ["path", "iispt"])
def test_projection_without_map_is_a_point_light_inside_its_frustum(binding, tmp_path, integrator):
    ref = restated("projection", ctm=translate(0.1, -0.05, 2.5) @ rotate(180, (1, 0, 0)) @ rotate(30, (0, 0, 1)))
    corners = np.array([[x, y, 0.0] for x in (-.4, .4) for y in (-.4, .4)])
    z, q = ref.project(corners - ref.p_light)
    assert (z > 0.5).all() and (np.abs(q) < 0.9).all()  # (screenBounds is [-1, 1]^2 without a map)
    out = []
    for kind in ("projection", "point"):
        path = write_scene(tmp_path, light_text(kind, ctm=ABOVE) + 'Material "matte"\n' + SMALL_QUAD, name=f"{kind}.pbrt", w=32, h=32, spp=4,
                           depth=1, integrator=integrator)
        gpu = binding.GpuScene(binding.HostScene(path=path))
        out.append([gpu.render_direct(4)] if integrator == "iispt" else
                   [x for collect in (False, True) for x in gpu.render(collect_stats=collect)])
        gpu.close()
    a, b = out
    if integrator == "iispt":
        assert a[0].max() > 0 and np.array_equal(a[0], b[0])
    else:
        assert a[0].max() > 0 and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2]))
        assert _counters(a[3]) == _counters(b[3])


# ---- through a surface ------------------------------------------------------------------------------------------------------------
RES = 16
# The light far from the plane and the maps small: the direct pass is held per pixel to 5 % after 64 jittered samples, so what a
# pixel sees of the map must be nearly flat. From 9.5 away a pixel of this view (0.12 x 0.22 on the plane) spans about 0.06
# of a texel of either map, over which a texel of 0.2 beside one of 1 changes by a quarter of its value at most: a standard
# deviation of 7 % for one sample, 0.9 % for the mean of 64, 3 % at 3.5 sigma (768 pixel channels). The projector's window
# (fov 100) is turned so that its edge runs through the view.
SURFACE_CTM_TEXT = "Translate 1 2 9\nRotate 215 1 0 0\nRotate 10 0 0 1\n"
SURFACE_CTM = translate(1, 2, 9) @ rotate(215, (1, 0, 0)) @ rotate(10, (0, 0, 1))
SURFACE = {"projection": ("projection", "wide_small", 100.0), "goniometric": ("goniometric", "gonio_small", None)}


def _surface_scene(binding, tmp_path, kind, which, fov, extra="", **kw):
    image = write_map(tmp_path, which)
    opts = dict(w=RES, h=RES, depth=1, fov=30, center=True)
    opts.update(kw)
    path = write_scene(tmp_path, light_text(kind, f"{which}.pfm", ctm=SURFACE_CTM_TEXT, fov=fov, intensity=(400, 300, 200)) + extra +
                       'Material "matte"\n' + PLANE, **opts)
    return path, restated(kind, image, ctm=SURFACE_CTM, fov=fov or 45.0, intensity=(400, 300, 200))


def _plane_radiance(ref, o, d):
    """f I factor(-wi) |cos theta_i| / r^2 of the matte plane z = 0 where each camera ray (o, d) reaches it, and that point."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    p = o + (-o[:, 2] / d[:, 2])[:, None] * d
    wi, li, _ = ref.sample_li(p)
    return (KD / np.pi) * li * np.abs(wi[:, 2:3]), p


def _sub_pixel(gpu, ref):
    """The restated radiance at the 8 x 8 sub-pixel grid of every pixel, (RES, RES, 64, 3), and whether a pixel is wholly lit or
    wholly dark: its 64 sub-samples and its four corners all lit or all dark. (The lit part of the plane is convex and its
    edges are straight, in the image too: a pixel whose corners are all lit is lit all over, and an edge that cuts into a
    pixel takes a corner with it. The direct pass jitters over the whole pixel, also outside the grid's outermost points.)"""
    sub = (np.arange(8) + 0.5) / 8
    gx, gy = np.meshgrid(np.arange(RES)[:, None] + sub[None, :], np.arange(RES)[:, None] + sub[None, :])
    o, d = gpu.camera_rays(np.stack([gx.reshape(-1), gy.reshape(-1)], 1))
    want = _plane_radiance(ref, o, d)[0].reshape(RES, 8, RES, 8, 3).transpose(0, 2, 1, 3, 4).reshape(RES, RES, 64, 3)
    cx, cy = np.meshgrid(np.arange(RES + 1), np.arange(RES + 1))
    o, d = gpu.camera_rays(np.stack([cx.reshape(-1), cy.reshape(-1)], 1).astype(np.float64))
    corner = (_plane_radiance(ref, o, d)[0].max(axis=1) > 0).reshape(RES + 1, RES + 1)
    corners = np.stack([corner[:-1, :-1], corner[1:, :-1], corner[:-1, 1:], corner[1:, 1:]], 2)
    lit = np.concatenate([want.max(axis=3) > 0, corners], 2)
    return want, lit.all(axis=2) | (~lit).all(axis=2)


@pytest.mark.parametrize("case", list(SURFACE))
def test_lit_plane_path_integrator(binding, tmp_path, case):
    """Every pixel's centre sample; for the projector, the pixels that are wholly lit or wholly dark (0.934 of them, 0.61 of those lit)."""
    path, ref = _surface_scene(binding, tmp_path, *SURFACE[case])
    gpu = binding.GpuScene(binding.HostScene(path=path))
    px, py = np.meshgrid(np.arange(RES), np.arange(RES))
    px, py = px.reshape(-1), py.reshape(-1)
    L, _ = gpu.li_samples(px, py, np.zeros_like(px))
    o, d = gpu.camera_rays(np.stack([px + 0.5, py + 0.5], 1))
    want, _ = _plane_radiance(ref, o, d)
    keep = _sub_pixel(gpu, ref)[1].reshape(-1)
    gpu.close()
    print(f"{case}: share of pixels kept {keep.mean():.3f}, lit {(want.max(axis=1) > 0).mean():.3f}")
    assert keep.mean() > 0.5 and want.max() > 0
    assert (want[keep].max(axis=1) > 0).mean() > 0.25
    if case == "goniometric":
        assert keep.all()
    else:
        assert not keep.all() and (want[keep].max(axis=1) == 0).any()
    assert np.allclose(L[keep], want[keep], rtol=1e-3, atol=1e-6 * want.max()), np.abs(L[keep] - want[keep]).max()


@pytest.mark.parametrize("case", list(SURFACE))
def test_lit_plane_direct_pass(binding, tmp_path, case):
    """The IISPT direct pass over 64 jittered passes, each wholly lit or wholly dark pixel against the restated radiance averaged
    over its 8 x 8 grid, and the mean of the whole film (the pixels the frustum edge crosses among them). Measured: the worst
    kept pixel uses 0.39 (projection) and 0.19 (goniometric) of the band; film mean / restated mean 0.99969 and 1.00000."""
    path, ref = _surface_scene(binding, tmp_path, *SURFACE[case], integrator="iispt", center=False)
    gpu = binding.GpuScene(binding.HostScene(path=path))
    mon = gpu.render_direct(64)
    img = mon[..., :3] / mon[..., 3:4]
    want_sub, keep = _sub_pixel(gpu, ref)
    gpu.close()
    want = want_sub.mean(axis=2)
    print(f"{case}: share of pixels kept {keep.mean():.3f}; film mean / restated mean {img.mean() / want.mean():.5f}; "
          f"worst excess over the band, in units of it {(np.abs(img[keep] - want[keep]) / (5e-2 * np.abs(want[keep]) + 1e-3 * want.max())).max():.3f}")
    assert keep.mean() > 0.5 and np.isfinite(img).all()
    assert np.allclose(img[keep], want[keep], rtol=5e-2, atol=1e-3 * want.max()), np.abs(img[keep] - want[keep]).max()
    assert abs(img.mean() / want.mean() - 1) < 1e-2, img.mean() / want.mean()


# ---- an occluder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(SURFACE))
def test_sphere_casts_a_shadow(binding, tmp_path, case):
    """A sphere between the light and the plane: the shadow ray ends at pLight, so plane points behind the sphere are exactly
    black at maxdepth 1 and those clear of it are what they are without the sphere."""
    centre, radius = np.array([0.3, 0.4, 1.5]), 0.3
    ball = f'AttributeBegin\nTranslate {centre[0]} {centre[1]} {centre[2]}\nShape "sphere" "float radius" [{radius}]\nAttributeEnd\n'
    path, ref = _surface_scene(binding, tmp_path, *SURFACE[case], extra='Material "matte"\n' + ball)
    gpu = binding.GpuScene(binding.HostScene(path=path))
    px, py = np.meshgrid(np.arange(RES), np.arange(RES))
    px, py = px.reshape(-1), py.reshape(-1)
    L, _ = gpu.li_samples(px, py, np.zeros_like(px))
    o, d = gpu.camera_rays(np.stack([px + 0.5, py + 0.5], 1))
    gpu.close()
    want, p = _plane_radiance(ref, o, d)

    def miss_distance(a, b):  # distance from the sphere's centre to the segment a -> b
        ab = b - a
        t = np.clip(((centre - a) * ab).sum(1) / (ab * ab).sum(1), 0, 1)
        return np.linalg.norm(a + t[:, None] * ab - centre, axis=1)

    seen = miss_distance(o.astype(np.float64), p) > 1.1 * radius  # the camera sees the plane, not the sphere
    to_light = miss_distance(p, np.broadcast_to(ref.p_light, p.shape))
    shadow, clear = seen & (to_light < 0.9 * radius), seen & (to_light > 1.1 * radius)
    assert shadow.sum() >= 4 and clear.sum() > 100 and want[shadow].max() > 0
    assert (L[shadow] == 0).all()
    assert np.allclose(L[clear], want[clear], rtol=1e-3, atol=1e-6 * want.max())


# ---- light choice ---------------------------------------------------------------------------------------------------------------
def _three_light_room(tmp_path, strategy, spp=64, integrator="path", name=None, depth=3):
    write_map(tmp_path, "wide"), write_map(tmp_path, "gonio")
    body = ('LightSource "point" "rgb I" [6 6 6] "point from" [-1.5 -1 2]\n' +
            light_text("projection", "wide.pfm", fov=70, ctm="Translate 0.5 -0.5 2.5\nRotate 165 1 0 0\nRotate 10 0 0 1\n") +
            light_text("goniometric", "gonio.pfm", ctm="Translate 1 0.8 1.6\nRotate 40 0 1 1\n", intensity=(4, 4, 4)) +
            ROOM.split("\n", 1)[1])
    return write_scene(tmp_path, body, name=name or f"{strategy}.pbrt", spp=spp, depth=depth, strategy=strategy, integrator=integrator,
                       **ROOM_VIEW)


def test_light_strategies_agree(binding, tmp_path):
    """A room under a point, a projection and a goniometric light at 64 spp: the spatial, power and uniform strategies agree
    in the film's mean within four standard deviations of the uniform render's mean, measured over its 64 single-sample films
    Measured: film means 0.13693 (spatial), 0.13689 (power), 0.13692 (uniform); the standard deviation of the uniform mean is
    3.0e-4, 0.22 % of it."""
    means, sigma = {}, None
    for strategy in ("spatial", "power", "uniform"):
        host = binding.HostScene(path=_three_light_room(tmp_path, strategy))
        gpu = binding.GpuScene(host)
        film, _ = gpu.render()
        rgb = host.film_to_rgb(film).astype(np.float64)
        assert np.isfinite(rgb).all() and (rgb.reshape(-1, 3).max(axis=1) > 0).mean() > 0.9
        means[strategy] = rgb.mean()
        if strategy == "uniform":
            px, py = np.meshgrid(np.arange(32), np.arange(32))
            px, py = px.reshape(-1), py.reshape(-1)
            singles = np.array([gpu.li_samples(px, py, np.full_like(px, k))[0].astype(np.float64).mean() for k in range(64)])
            sigma = singles.std(ddof=1) / np.sqrt(64)
            assert abs(singles.mean() / means["uniform"] - 1) < 1e-3
        gpu.close()
    print(f"film means {means}; standard deviation of the uniform mean {sigma:.6f} ({sigma / means['uniform']:.5f} of it)")
    for a in ("spatial", "power"):
        assert abs(means[a] - means["uniform"]) <= 4 * sigma, (a, means, sigma)
    assert abs(means["spatial"] - means["power"]) <= 4 * sigma, (means, sigma)


# ---- IISPT ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, which", [("projection", "wide"), ("goniometric", "gonio")])
def test_iispt_passes_are_finite_and_repeatable(binding, tmp_path, kind, which):
    """The probe pass twice; the frame (probes, the random-weight network, the gather, the direct pass) twice."""
    _iispt_modules()
    write_map(tmp_path, which)
    path = write_scene(tmp_path, light_text(kind, f"{which}.pfm", ctm=SURFACE_CTM_TEXT, fov=80 if kind == "projection" else None) + ROOM,
                       spp=1, depth=3, integrator="iispt", **ROOM_VIEW)
    pos = np.array([[0, -1, 0.01], [0.5, -0.5, 0.3], [0, -0.5, 0.6], [0.2, 0.2, 1.5]])
    dirs = np.array([[0, 0, 1], [0, -0.6, 0.8], [0, -1, 0], [0, 0, -1]])
    gpu = binding.GpuScene(binding.HostScene(path=path))
    a, b = gpu.render_probes(pos, dirs), gpu.render_probes(pos, dirs)
    gpu.close()
    assert a[0].max() > 0
    for x, y in zip(a[:3], b[:3]):
        assert np.isfinite(x).all() and np.array_equal(_bits(x), _bits(y))
    fa, fb = _iispt_image(binding, path, n_direct=8), _iispt_image(binding, path, n_direct=8)
    assert np.isfinite(fa).all() and fa.max() > 0 and (fa >= 0).all()
    assert np.array_equal(_bits(fa), _bits(fb))


# ---- the C++ host ---------------------------------------------------------------------------------------------------------------
def test_cli_renders_the_binding_film(binding, tmp_path):
    path = _three_light_room(tmp_path, "spatial", spp=4, name="cli.pbrt")
    out = tmp_path / "cli.pfm"
    exe = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
    p = subprocess.run([exe, path, "--outfile", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    raw = out.read_bytes()
    head = b"PF\n32 32\n-1.0\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], "<f4").reshape(32, 32, 3)[::-1]
    host = binding.HostScene(path=path)
    gpu = binding.GpuScene(host)
    want = host.film_to_rgb(gpu.render()[0]).astype(np.float32)
    gpu.close()
    assert want.max() > 0 and (img.view(np.uint32) == want.view(np.uint32)).all()


def test_cli_iispt_integrator_writes_the_python_frames_image(binding, tmp_path):
    torch, nn_mod, frame_mod, ref_mod = _iispt_modules()
    n_tasks, n_direct = 4, 2
    path = _three_light_room(tmp_path, None, spp=1, integrator="iispt", name="cli_iispt.pbrt")
    torch.manual_seed(3)
    module = ref_mod.IISPTNet().eval()
    net_file = tmp_path / "net.iilenet"
    binding.save_net_weights(module.state_dict(), str(net_file), bn_eps=module.encoder1[3].eps)
    out, ind, direct = tmp_path / "frame.pfm", tmp_path / "indirect.pfm", tmp_path / "direct.pfm"
    exe = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
    env = dict(os.environ, IISPT_SCHEDULE_RADIUS_START="8")
    p = subprocess.run([exe, path, f"--iisptNet={net_file}", f"--iileIndirect={n_tasks}", f"--iileDirect={n_direct}", "--outfile", str(out),
                        f"--iisptIndirectOut={ind}", f"--iisptDirectOut={direct}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stdout
    gpu = binding.GpuScene(binding.HostScene(path=path))
    frame = frame_mod.IisptFrame(binding, gpu, nn_mod.IisptPipeline(gpu, net=module))
    frame.run_batched(n_tasks, radius_start=8.0)
    frame.run_direct(n_direct)
    torch.cuda.synchronize()
    head = b"PF\n32 32\n-1.0\n"
    for f, want, name in ((out, frame.image(), "merged"), (ind, frame.indirect_image(), "indirect"), (direct, frame.direct_image(), "direct")):
        raw = f.read_bytes()
        assert raw.startswith(head), name
        got = np.frombuffer(raw[len(head):], "<f4").reshape(32, 32, 3)[::-1]
        want = want.cpu().numpy()
        assert float(want.max()) > 0 and np.isfinite(want).all(), name
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    gpu.close()
