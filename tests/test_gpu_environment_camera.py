"""`Camera "environment"` on the device (GPU), held to the float64 restatement of envcamera_ref.py: the rays alone through the
`camera_rays` probe; a constant sky and a lat-long environment map seen through the path integrator, `li_samples` and the IISPT
direct pass; the ray differentials through a closed-form-filtered checkerboard; the IISPT hemi points and frame; and the C++
host, alone and sharded, against the Python binding bit for bit."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import envcamera_ref as EC
import imagelight_ref as IL
import texture_ref as T

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
EXE = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
SWAP_TEXT = "Transform [1 0 0 0  0 0 1 0  0 1 0 0  0 0 0 1]"  # the camera's y-up frame onto the lights' z-up one
# No ray can hit a triangle of no area (its edge functions are all zero, triangle.cpp:227-262), and the loader refuses a scene
# without primitives: this one stands in for "no geometry".
NOTHING = 'Material "matte"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 -900  0 0 -900  0 0 -900]\n'
CENTER = 'Sampler "halton" "integer pixelsamples" [1] "bool samplepixelcenter" "true"'


def scene_text(camera='Camera "environment"', before="", xres=32, yres=16, spp=4, integrator='Integrator "path" "integer maxdepth" [3]',
               sampler=None, world=None):
    world = world if world is not None else ('LightSource "point" "rgb I" [1 1 1] "point from" [0 0 3]\nMaterial "matte"\n'
                                             'Shape "sphere" "float radius" [5]\n')
    sampler = sampler or f'Sampler "halton" "integer pixelsamples" [{spp}]'
    return (f'{before}\n{camera}\nFilm "image" "integer xresolution" [{xres}] "integer yresolution" [{yres}] "string filename" "env.exr"\n'
            f'PixelFilter "box"\n{sampler}\n{integrator}\nWorldBegin\n{world}WorldEnd\n')


def write_pfm(path, rows):
    """rows[0] is the file's first row of data: the image's BOTTOM scanline."""
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _iispt_modules():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    sys.path.insert(0, REPO)
    nn_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_nn")
    frame_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_frame")
    import iispt_torch_reference as ref_mod
    return torch, nn_mod, frame_mod, ref_mod


def _scene(binding, tmp_path, name="env.pbrt", **kw):
    path = tmp_path / name
    path.write_text(scene_text(**kw))
    host = binding.HostScene(path=str(path))
    return str(path), host, binding.GpuScene(host)


def _centres(xres, yres):
    px, py = np.meshgrid(np.arange(xres), np.arange(yres))
    return px.reshape(-1), py.reshape(-1)


# ---- 1. the rays ------------------------------------------------------------------------------------------------------------------
# Worst absolute error of a direction component against the restatement, measured on an MI355X over the three transforms
# below: 3.86e-7 (an origin component: 1.19e-7), about what rounding phi, up to 2 pi, to a float costs. The bar is four times
# that, for a libm that rounds differently; it may not pass 1e-4.
WORST_MEASURED = 3.86e-7
RAY_BAR = 4 * WORST_MEASURED
assert RAY_BAR <= 1e-4
RAY_CASES = {
    "identity": ("", []),
    "look_at": ("LookAt 1 2 3  0 0.5 0  0.1 0 1", [np.linalg.inv(EC.look_at([1, 2, 3], [0, 0.5, 0], [0.1, 0, 1]))]),
    "swaps_handedness": ("LookAt -2 1 0.5  0 0 0  0 0 1\nScale -1 1 1",
                         [np.linalg.inv(EC.look_at([-2, 1, 0.5], [0, 0, 0], [0, 0, 1])), EC.scale(-1, 1, 1)]),
}


def _film_points(xres, yres, rng):
    """Every pixel centre, then 256 points of the sample bounds [0, xres] x [0, yres] (the box filter of radius 0.5): 32 within 1e-3
    of each pole (pFilm.y at 0 and at yres, the two bounds themselves among them), 32 on each side of the seam (pFilm.x at 0 and
    at xres exactly), the rest anywhere."""
    px, py = _centres(xres, yres)
    p = rng.uniform(0, 1, (256, 2)) * np.array([xres, yres])
    p[:32, 1] = rng.uniform(0, 1e-3, 32)
    p[32:64, 1] = yres - rng.uniform(0, 1e-3, 32)
    p[0, 1], p[32, 1] = 0.0, yres
    p[64:96, 0] = 0.0
    p[96:128, 0] = xres
    return np.concatenate([np.stack([px + 0.5, py + 0.5], 1), p]).astype(np.float32)


@pytest.mark.parametrize("case", list(RAY_CASES))
def test_rays_match_restatement(binding, tmp_path, case):
    """Measured worst errors of a direction component (MI355X): identity 3.86e-7, look_at 3.29e-7, swaps_handedness 3.05e-7; of an
    origin component 0, 1.19e-7, 1.18e-7."""
    text, factors = RAY_CASES[case]
    xres, yres = 16, 8
    _, host, gpu = _scene(binding, tmp_path, before=text, xres=xres, yres=yres)
    pfilm = _film_points(xres, yres, np.random.default_rng(list(RAY_CASES).index(case)))
    assert len(pfilm) == xres * yres + 256
    assert (pfilm[:, 1] < 1e-3).sum() >= 32 and (pfilm[:, 1] > yres - 1e-3).sum() >= 32
    assert (pfilm[:, 0] == 0).sum() >= 32 and (pfilm[:, 0] == xres).sum() >= 32
    o, d = gpu.camera_rays(pfilm)
    o_lens, d_lens = gpu.camera_rays(pfilm, plens=np.random.default_rng(9).random((len(pfilm), 2)))  # plens is ignored
    gpu.close()
    c2w = EC.camera_to_world(*factors)
    assert (np.linalg.det(c2w[:3, :3]) < 0) == (case == "swaps_handedness")
    want_o, want_d = EC.generate_ray(c2w, pfilm.astype(np.float64), xres, yres)
    err_d, err_o = np.abs(d - want_d).max(), np.abs(o - want_o).max()
    print(f"{case}: worst direction error {err_d:.3e}, worst origin error {err_o:.3e} (bar {RAY_BAR:.3e})")
    assert np.array_equal(_bits(o), _bits(o_lens)) and np.array_equal(_bits(d), _bits(d_lens))
    assert np.isfinite(o).all() and np.isfinite(d).all()
    assert err_d <= RAY_BAR
    # the origin is a point of magnitude |translation|: the same bar, relative to it
    assert err_o <= RAY_BAR * max(1.0, np.abs(c2w[:3, 3]).max())
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6


# ---- 2. a constant sky ------------------------------------------------------------------------------------------------------------
SKY = np.array([0.25, 0.5, 1.0])
RGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])  # spectrum.h:62-66


@pytest.mark.parametrize("sampler", ["halton", "sobol"])
def test_constant_sky_path_integrator(binding, tmp_path, sampler):
    """Every camera sample carries L, so a pixel — a weighted mean of equal values — does: through `li_samples` as RGB, and on the
    film, which keeps XYZ, as RGBToXYZ(L). (Film's own XYZ -> RGB matrix is not the inverse of RGBToXYZ to 1e-6: 4.0e-6 in R for
    this L. The film is therefore compared where it is kept, not after `film_to_rgb`.)"""
    world = f'LightSource "infinite" "rgb L" [{SKY[0]} {SKY[1]} {SKY[2]}]\n' + NOTHING
    _, host, gpu = _scene(binding, tmp_path, before=SWAP_TEXT, world=world, sampler=f'Sampler "{sampler}" "integer pixelsamples" [4]')
    film, _ = gpu.render()
    px, py = _centres(32, 16)
    L = np.concatenate([gpu.li_samples(px, py, np.full_like(px, k))[0] for k in range(4)]) if sampler == "halton" else None
    gpu.close()
    # (a sample whose film position is a whole number also counts for the pixel before it: some weights are 5)
    assert film.shape == (16, 32, 4) and (film[..., 3] >= 4).all()
    xyz = film[..., :3].astype(np.float64) / film[..., 3:]
    assert np.abs(xyz / (RGB_TO_XYZ @ SKY) - 1).max() <= 1e-6
    if L is not None:
        assert np.abs(L / SKY - 1).max() <= 1e-6
    assert np.allclose(host.film_to_rgb(film), SKY, rtol=1e-5, atol=0)


def test_constant_sky_direct_pass(binding, tmp_path):
    world = f'LightSource "infinite" "rgb L" [{SKY[0]} {SKY[1]} {SKY[2]}]\n' + NOTHING
    _, host, gpu = _scene(binding, tmp_path, before=SWAP_TEXT, world=world, integrator='Integrator "iispt"', spp=1)
    mon = gpu.render_direct(1)
    gpu.close()
    assert mon.shape == (16, 32, 4) and (mon[..., 3] > 0).all()
    assert np.abs(mon[..., :3] / mon[..., 3:] / SKY - 1).max() <= 1e-6


# ---- 3. a lat-long map seen through the lat-long camera -----------------------------------------------------------------------------
def infinite_le(image, light_to_world, d):
    """InfiniteAreaLight::Le (src/lights/infinite.cpp:97-104): Lmap->Lookup((SphericalPhi(w) / 2 Pi, SphericalTheta(w) / Pi)) at
    w = Normalize(WorldToLight(ray.d)); `image` is Lmap's finest level as ReadImage returns it (row 0 = the top scanline)."""
    w = np.asarray(d, np.float64) @ np.linalg.inv(np.asarray(light_to_world, np.float64))[:3, :3].T
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    theta = np.arccos(np.clip(w[:, 2], -1, 1))
    phi = np.arctan2(w[:, 1], w[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    return IL.MipMap(image).lookup(np.stack([phi / (2 * np.pi), theta / np.pi], 1))


@pytest.mark.parametrize("turned", [False, True])
def test_lat_long_map_comes_back_texel_for_texel(binding, tmp_path, turned):
    """With the camera's y-up frame taken to the light's z-up one, the camera's (phi, theta) of a pixel centre are the light's
    (s, t) of a texel centre: the film is the map (infinite.cpp:97-104 does not flip it). With `Rotate 90 0 1 0` after it the
    camera looks along other axes of the map, and the film is the restatement's bilinear lookup there: a swapped or mirrored
    axis would show."""
    xres, yres = 16, 8
    rows = (0.2 + 0.8 * np.random.default_rng(5).random((yres, xres, 3))).astype(np.float32)
    write_pfm(tmp_path / "sky.pfm", rows)
    image = rows[::-1].astype(np.float64)
    world = 'LightSource "infinite" "string mapname" "sky.pfm"\n' + NOTHING
    before = SWAP_TEXT + ("\nRotate 90 0 1 0" if turned else "")
    _, host, gpu = _scene(binding, tmp_path, before=before, world=world, xres=xres, yres=yres, sampler=CENTER)
    film, _ = gpu.render()
    gpu.close()
    got = host.film_to_rgb(film).astype(np.float64).reshape(-1, 3)
    px, py = _centres(xres, yres)
    c2w = EC.camera_to_world(EC.SWAP_YZ, *([EC.rotate(90, (0, 1, 0))] if turned else []))
    _, d = EC.generate_ray(c2w, np.stack([px + 0.5, py + 0.5], 1), xres, yres)
    want = infinite_le(image, np.eye(4), d)
    # straight, the restated rays land on texel centres and the lookup is the map itself; turned, it is no shift of the map
    shift = np.abs(want.reshape(yres, xres, 3)[None] - np.stack([np.roll(image, s, axis=1) for s in range(xres)])).max(axis=(1, 2, 3))
    assert (shift[0] < 1e-9) if not turned else (shift.min() > 0.05)
    scale = np.abs(want).max()
    assert (np.abs(got - want) <= 2e-3 * np.abs(want) + 1e-6 * scale).all(), np.abs(got - want).max()  # test_gpu_image_lights.py's band for its lookups


# ---- 4. the differentials -----------------------------------------------------------------------------------------------------------
ROOM_HALF, ROOM_H = 4.0, 1.0
LIGHT, INTENSITY = np.array([0.3, 0.2, 0.4]), np.array([20.0, 15.0, 10.0])
CHECKS = 8.0  # "uscale" / "vscale": the floor carries 8 x 8 checks of 1 x 1 world unit


def _room_text():
    a, h = ROOM_HALF, ROOM_H
    quad = lambda p: f'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [{" ".join(str(v) for v in p)}] "float uv" [0 0 1 0 1 1 0 1]\n'
    floor = quad([-a, -a, -h, a, -a, -h, a, a, -h, -a, a, -h])
    others = "".join(quad(p) for p in ([-a, -a, h, a, -a, h, a, a, h, -a, a, h], [-a, -a, -h, a, -a, -h, a, -a, h, -a, -a, h],
                                      [-a, a, -h, a, a, -h, a, a, h, -a, a, h], [-a, -a, -h, -a, a, -h, -a, a, h, -a, -a, h],
                                      [a, -a, -h, a, a, -h, a, a, h, a, -a, h]))
    return (f'LightSource "point" "rgb I" [{INTENSITY[0]} {INTENSITY[1]} {INTENSITY[2]}] "point from" [{LIGHT[0]} {LIGHT[1]} {LIGHT[2]}]\n'
            f'Texture "K" "spectrum" "checkerboard" "string aamode" "closedform" "float uscale" [{CHECKS}] "float vscale" [{CHECKS}] '
            '"rgb tex1" [0.9 0.6 0.3] "rgb tex2" [0.1 0.2 0.4]\n'
            'Material "matte" "texture Kd" "K"\n' + floor + 'Material "matte" "rgb Kd" [0.5 0.5 0.5]\n' + others)


def _room_hits(o, d):
    """(t, which) of the nearest wall of the room for rays from inside it: which 0 = the floor, 1 the ceiling, 2 .. 5 the walls."""
    planes = [(2, -ROOM_H), (2, ROOM_H), (1, -ROOM_HALF), (1, ROOM_HALF), (0, -ROOM_HALF), (0, ROOM_HALF)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ts = np.stack([(c - o[:, ax]) / d[:, ax] for ax, c in planes], 1)
    ts = np.where(ts > 0, ts, np.inf)
    return ts.min(1), ts.argmin(1)


def test_differentials_filter_a_checkerboard(binding, tmp_path):
    """The camera at the centre of an 8 x 8 x 2 room, 1 spp at the pixel centres, maxdepth 1, a point light: Lambertian
    Kd(p) / pi * I |cos| / r^2 at the point each pixel sees, Kd of the floor from the closed-form box filter of texture_ref.py over
    the footprint that ComputeDifferentials (interaction.cpp:95-149) makes of the restated camera differentials. Footprints run from
    a fiftieth of a check below the camera to more than a check at the far floor (the filter's `ds > 1` branch)."""
    xres, yres = 32, 16
    _, host, gpu = _scene(binding, tmp_path, before=SWAP_TEXT, world=_room_text(), xres=xres, yres=yres, sampler=CENTER,
                          integrator='Integrator "path" "integer maxdepth" [1]')
    px, py = _centres(xres, yres)
    L, _ = gpu.li_samples(px, py, np.zeros_like(px))
    gpu.close()
    o, d, rxo, rxd, ryo, ryd = EC.differentials(EC.camera_to_world(EC.SWAP_YZ), np.stack([px + 0.5, py + 0.5], 1), xres, yres, spp=1)
    t, which = _room_hits(o, d)
    p = o + t[:, None] * d
    # no pixel centre looks at an edge of the room: which quad it sees does not hang on rounding
    near_edge = np.sort(np.stack([ROOM_H - np.abs(p[:, 2]), ROOM_HALF - np.abs(p[:, 1]), ROOM_HALF - np.abs(p[:, 0])], 1), 1)[:, 1]
    assert near_edge.min() > 0.05
    floor = which == 0
    assert floor.sum() >= 0.25 * len(p)
    # ComputeDifferentials on the floor (n = (0, 0, 1), dpdu = (8, 0, 0), dpdv = (0, 8, 0): the 2 x 2 system is diagonal)
    n = np.array([0.0, 0.0, 1.0])
    tx = -((rxo @ n) - (p @ n)) / (rxd @ n)
    ty = -((ryo @ n) - (p @ n)) / (ryd @ n)
    dpdx, dpdy = rxo + tx[:, None] * rxd - p, ryo + ty[:, None] * ryd - p
    side = 2 * ROOM_HALF
    uv = (p[:, :2] + ROOM_HALF) / side
    duv = np.stack([dpdx[:, 0] / side, dpdx[:, 1] / side, dpdy[:, 0] / side, dpdy[:, 1] / side], 1)
    tex = host.procedural_texture(0)
    assert tex["kind"] == T.TEX_CHECKER2D and tex["aamode"] == T.AA_CLOSEDFORM
    args = (uv[floor].astype(np.float32), duv[floor].astype(np.float32), p[floor].astype(np.float32), dpdx[floor].astype(np.float32),
            dpdy[floor].astype(np.float32))
    kd = np.full((len(p), 3), 0.5)
    kd[floor] = np.maximum(T.evaluate([tex], 0, *args).astype(np.float64), 0)
    sel, _, _ = T.checker(tex, *args)
    ds = CHECKS * np.maximum(np.abs(duv[floor][:, 0]), np.abs(duv[floor][:, 2]))
    assert (sel == 2).mean() > 0.25 and (sel != 2).any() and ds.max() > 1 and ds.min() < 0.1  # blended, pure and `ds > 1` pixels
    ok = np.ones(len(p), bool)
    ok[floor] = T.edge_distance(tex, *args) >= 1e-4
    assert ok.mean() >= 0.95, ok.mean()  # (of the restatement alone)
    to_l = LIGHT[None, :] - p
    r2 = (to_l ** 2).sum(1)
    normal_axis = np.array([2, 2, 1, 1, 0, 0])[which]
    cos = np.abs(to_l[np.arange(len(p)), normal_axis]) / np.sqrt(r2)
    want = kd / np.pi * INTENSITY[None, :] * (cos / r2)[:, None]
    # and the filter matters: the unfiltered checkerboard is not the film
    plain = dict(tex, aamode=T.AA_NONE)
    want_plain = want.copy()
    want_plain[floor] = (np.maximum(T.evaluate([plain], 0, *args).astype(np.float64), 0) / np.pi * INTENSITY[None, :] * (cos / r2)[floor][:, None])
    assert not np.allclose(want_plain[ok], want[ok], rtol=5e-2, atol=0)
    worst = (np.abs(L[ok] - want[ok]) / (np.abs(want[ok]) + 1e-5 * want.max() / 2e-3)).max()
    print(f"differentials: {ok.sum()} of {len(p)} pixels held, {floor.sum()} on the floor, worst relative error {worst:.3e}")
    assert np.allclose(L[ok], want[ok], rtol=2e-3, atol=1e-5 * want.max()), np.abs(L[ok] - want[ok]).max()  # test_gpu_procedural_textures.py's


# ---- 5. IISPT ------------------------------------------------------------------------------------------------------------------------
SPHERE_ROOM = 'LightSource "point" "rgb I" [30 30 30] "point from" [0 0 3]\nMaterial "matte" "rgb Kd" [0.6 0.5 0.4]\nShape "sphere" "float radius" [5]\n'


def test_iispt_hemi_points_lie_where_the_camera_looks(binding, tmp_path):
    xres, yres, ts = 32, 16, 3
    _, host, gpu = _scene(binding, tmp_path, before=SWAP_TEXT, world=SPHERE_ROOM, xres=xres, yres=yres, sampler=CENTER,
                          integrator='Integrator "iispt"')
    task = binding.IisptTask(0, 0, xres, yres, ts, 0, 1)
    valid, pos, _ = gpu.iispt_hemi_points(task)
    gpu.close()
    nx, ny = task.grid()
    assert (nx, ny) == (12, 6) and valid.shape == (ny, nx) and valid.all()
    gx = np.minimum(np.arange(nx) * ts, xres - 1)
    gy = np.minimum(np.arange(ny) * ts, yres - 1)
    pf = np.stack(np.meshgrid(gx + 0.5, gy + 0.5), -1).reshape(-1, 2)
    _, d = EC.generate_ray(EC.camera_to_world(EC.SWAP_YZ), pf, xres, yres)
    pos = pos.reshape(-1, 3).astype(np.float64)
    r = np.linalg.norm(pos, axis=1)
    assert np.abs(r - 5).max() < 1e-3
    # (the spawned ray's offset runs along the normal, which is radial here)
    assert np.abs(pos / r[:, None] - d).max() <= RAY_BAR + 1e-4


def test_iispt_frame_is_finite_and_lit(binding, tmp_path):
    """The whole frame (hemi points, probe pass, the network with the recipe weights of tests/golden/iispt_net_fixture.npz,
    gather, direct pass): finite, and its direct film is not black. Nothing is held about the network."""
    torch, nn_mod, frame_mod, ref_mod = _iispt_modules()
    import iispt_net_recipe as recipe
    net = ref_mod.IISPTNet()
    recipe.fill_state_dict(net)
    _, host, gpu = _scene(binding, tmp_path, before=SWAP_TEXT, world=SPHERE_ROOM, spp=1, integrator='Integrator "iispt"')
    frame = frame_mod.IisptFrame(binding, gpu, nn_mod.IisptPipeline(gpu, net=net.eval()))
    frame.run_batched(2, radius_start=8.0)
    frame.run_direct(2)
    torch.cuda.synchronize()
    assert frame.stats["probes"] > 0
    img, direct = frame.image().cpu().numpy(), frame.direct_image().cpu().numpy()
    gpu.close()
    assert img.shape == (16, 32, 3) and np.isfinite(img).all() and np.isfinite(direct).all()
    assert (direct.max(axis=2) > 0).all()  # the point light reaches the whole sphere from inside


# ---- 6. the render paths agree, bit for bit -------------------------------------------------------------------------------------------
def _read_pfm(path, w, h):
    raw = path.read_bytes()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], "<f4").reshape(h, w, 3)[::-1]


def _run(*args, timeout=300, env=None):
    p = subprocess.run([EXE, *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, p.stdout
    return p


def test_cli_and_shards_render_the_binding_film(binding, tmp_path):
    """`iile_pbrt scene.pbrt` writes the Python binding's film; `--gpurank 0/1` and `--gpus 1` (the communicator branch) write the
    plain CLI's file; two tile shards of the binding add up to its whole film."""
    world = 'LightSource "infinite" "rgb L" [0.2 0.2 0.3]\n' + SPHERE_ROOM.replace('Shape "sphere" "float radius" [5]', 'Translate 0 3 0\nShape "sphere" "float radius" [1.5]')
    path, host, gpu = _scene(binding, tmp_path, before="LookAt 0.5 0 0.2  0 1 0  0 0 1", world=world, spp=4)
    film, _ = gpu.render()
    parts = [gpu.render(tile_rank=r, tile_nranks=2)[0] for r in range(2)]
    gpu.close()
    want = host.film_to_rgb(film).astype(np.float32)
    assert want.max() > 0 and len(np.unique(want.reshape(-1, 3), axis=0)) > 10
    assert all(p[..., 3].max() > 0 for p in parts) and np.array_equal(_bits(parts[0] + parts[1]), _bits(film))
    plain, ranked, allp, rv = tmp_path / "plain.pfm", tmp_path / "ranked.pfm", tmp_path / "all.pfm", tmp_path / "rendezvous"
    _run(path, "--outfile", plain)
    assert np.array_equal(_bits(_read_pfm(plain, 32, 16)), _bits(want))
    _run(path, "--outfile", ranked, "--gpurank", "0/1", "--rendezvous", rv, "--job", "78")
    _run(path, "--outfile", allp, "--gpus", "1")
    assert ranked.read_bytes() == plain.read_bytes() == allp.read_bytes()


def test_cli_iispt_writes_the_python_frames_image(binding, tmp_path):
    torch, nn_mod, frame_mod, ref_mod = _iispt_modules()
    torch.manual_seed(3)
    module = ref_mod.IISPTNet().eval()
    net_file = tmp_path / "net.iilenet"
    binding.save_net_weights(module.state_dict(), str(net_file), bn_eps=module.encoder1[3].eps)
    path, host, gpu = _scene(binding, tmp_path, before=SWAP_TEXT, world=SPHERE_ROOM, spp=1, integrator='Integrator "iispt"')
    out = tmp_path / "frame.pfm"
    _run(path, f"--iisptNet={net_file}", "--iileIndirect=2", "--iileDirect=2", "--outfile", out, timeout=600,
         env=dict(os.environ, IISPT_SCHEDULE_RADIUS_START="8"))
    frame = frame_mod.IisptFrame(binding, gpu, nn_mod.IisptPipeline(gpu, net=module))
    frame.run_batched(2, radius_start=8.0)
    frame.run_direct(2)
    torch.cuda.synchronize()
    want = frame.image().cpu().numpy()
    gpu.close()
    assert float(want.max()) > 0 and np.isfinite(want).all()
    assert np.array_equal(_bits(_read_pfm(out, 32, 16)), _bits(want))
