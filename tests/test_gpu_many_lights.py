"""More than eight lights on the device (GPU): the light the path integrator chooses and its pdf against the float64 restatement
of lightdistrib_ref.py under all three strategies; black lights added to a scene change nothing, bit for bit; a tessellated
emitter lights a floor as the closed form says; the primitive flag word with many lights beside an alpha mask; the IISPT direct
pass, the frame and the C++ host; the spatial table's cap. No scene here goes to the CPU oracle (its arrays hold eight lights)."""
import os
import subprocess

import numpy as np
import pytest

import lightdistrib_ref as LD
import many_lights_scenes as MS
from test_gpu_translucent import _bits, _counters, _iispt_image, _iispt_modules
from test_many_lights_scenes import MIXED, check_choice

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
EXE = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")


def _gpu(binding, path):
    host = binding.HostScene(path=path)
    return host, binding.GpuScene(host)


# ---- 1. the choice against the truth ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, seed", MIXED)
@pytest.mark.parametrize("strategy", ["spatial", "power", "uniform"])
def test_light_choice_matches_restatement(binding, tmp_path, n, seed, strategy):
    """10^4 lookups (400 voxels of the 64 x 64 x 48 grid, the eight corner voxels entered from outside the bounds). Measured shares:
    DESIGN.md section 4.2, "Many lights"."""
    path, scene = MS.mixed_scene(tmp_path, n, seed, strategy)
    p, u, vox = MS.lookups(scene, 10000, seed)
    assert len(u) == 10000 and list(scene.nv) == [64, 64, 48]
    inside = ((p >= scene.bmin) & (p <= scene.bmax)).all(axis=1)
    assert (~inside).sum() == 200 and np.array_equal(scene.voxel_of(p).reshape(-1, 25, 3)[:, 0], vox)
    # the scene keeps a float32 evaluation inside the bands: asked of the CPU before the device
    light32, pdfs32, _, _ = scene.choose(strategy, p, u, dtype=np.float32)
    check_choice(scene, strategy, p, u, light32, pdfs32[np.arange(len(u)), light32], f"float32 on the CPU, {n} lights, {strategy}")
    host, gpu = _gpu(binding, path)
    assert host.info["n_lights"] == n
    light, pdf = gpu.light_choose(p, u)
    gpu.close()
    check_choice(scene, strategy, p, u, light, pdf, f"device, {n} lights, {strategy}")
    assert len(np.unique(light)) >= min(n, 9) - 1  # (a choice among the lights, not one of them)


def test_one_light_is_chosen_with_pdf_one(binding, tmp_path):
    body = MS.point_light([0, 0, 2], [1, 1, 1]) + MS.SHELL
    _, gpu = _gpu(binding, MS.write(tmp_path, body))
    light, pdf = gpu.light_choose(np.array([[0, 0, 1], [5, 5, 5]], np.float32), np.array([0.1, 0.9], np.float32))
    gpu.close()
    assert list(light) == [0, 0] and list(pdf) == [1, 1]


# ---- 2. black lights change nothing under the power strategy ------------------------------------------------------------------------
def _with_black(n, seed, where):
    """The mixed scene of n lights, and the same with n more point lights of I = 0: ahead of them, behind them, or one after each.
    n and 2 n differ by a power of two, so every cdf value and every pdf is the same float; FindInterval never lands on a flat step."""
    rng = np.random.default_rng(seed)
    lights, _ = MS.mixed_light_chunks(n, seed)
    black = [MS.point_light(rng.uniform([-1.5, -1.5, 0.5], [1.5, 1.5, 2.5]), [0, 0, 0]) for _ in range(n)]
    if where == "none":
        parts = lights
    elif where == "first":
        parts = black + lights
    elif where == "last":
        parts = lights + black
    else:
        parts = [x for pair in zip(lights, black) for x in pair]
    return "".join(parts)


@pytest.mark.parametrize("n", [8, 5, 20])
def test_black_lights_change_nothing_under_power(binding, tmp_path, n):
    """Film and every counter of iile_render (both builds), and the probe pass, bit for bit: 8 lights against 16, 5 against 10, 20
    against 40."""
    mirror = 'AttributeBegin\nMaterial "mirror"\nTranslate 0.8 0.3 0.5\nShape "sphere" "float radius" [0.45]\nAttributeEnd\n'
    pos = np.array([[0, -1, 0.01], [0.5, -0.5, 0.3], [1.9, 1.9, 1.5]])
    dirs = np.array([[0, 0, 1], [0, -0.6, 0.8], [-0.6, -0.8, 0]])
    out = {}
    for where in ("none", "first", "last", "interleaved"):
        path = MS.write(tmp_path, _with_black(n, 20 + n, where) + MS.SHELL + mirror, name=f"black_{where}.pbrt", strategy="power", w=48, h=32, spp=4)
        host, gpu = _gpu(binding, path)
        assert host.info["n_lights"] == (n if where == "none" else 2 * n)
        plain, _ = gpu.render()
        counted, st = gpu.render(collect_stats=True)
        probes = gpu.render_probes(pos, dirs)
        gpu.close()
        out[where] = (plain, counted, _counters(st), probes)
    base = out["none"]
    assert base[0].max() > 0 and np.isfinite(base[0]).all() and base[2]["shadow_rays"] > 0 and base[3][0].max() > 0
    for where in ("first", "last", "interleaved"):
        got = out[where]
        assert np.array_equal(_bits(got[0]), _bits(base[0])) and np.array_equal(_bits(got[1]), _bits(base[1])), where
        assert got[2] == base[2], where
        for a, b in zip(got[3][:3], base[3][:3]):
            assert np.array_equal(_bits(a), _bits(b)), where
        assert _counters(got[3][3]) == _counters(base[3][3]), where


# ---- 3. tessellation does not change the light --------------------------------------------------------------------------------------
FAR_BLACK = MS.spot_light([40, 30, 20], [0, 0, 0], [0, 0, 0]) + MS.point_light([-30, 40, 25], [0, 0, 0])


@pytest.mark.parametrize("strategy", ["spatial", "power", "uniform"])
@pytest.mark.parametrize("case", ["2_triangles", "32_triangles", "32_triangles_and_black_lights"])
def test_tessellated_panel_lights_the_floor_as_the_closed_form(binding, tmp_path, case, strategy):
    """A 1.6 x 1.0 emitter 1.5 above a matte floor, 64 spp, maxdepth 1. Measured means and errors: DESIGN.md section 4.2, "Many lights"."""
    nx, ny = (1, 1) if case == "2_triangles" else (4, 4)
    extra = FAR_BLACK if case.endswith("black_lights") else ""
    host, gpu = _gpu(binding, MS.panel_scene(tmp_path, nx, ny, strategy, extra=extra))
    assert host.info["n_lights"] == 2 * nx * ny + (2 if extra else 0)
    film, _ = gpu.render()
    gpu.close()
    MS.patch_check(host.film_to_rgb(film), label=f"{case}, {strategy}")


# ---- 4. the flag word -----------------------------------------------------------------------------------------------------------------
def _flag_scene(tmp_path, emit, name):
    """Sixteen point lights, then a quad that is lights 16 and 17 (or no light), over a floor; an invisible quad ("float alpha" [0])
    hangs between the floor and the emitter, so the ALPHA builds of the traversal kernels run and every ray below passes through it."""
    rng = np.random.default_rng(4)
    body = "".join(MS.point_light(rng.uniform([-1, -1, 2.2], [1, 1, 2.8]), [0.02, 0.02, 0.02]) for _ in range(16))
    pts = [[-0.5, -0.5, 2], [-0.5, 0.5, 2], [0.5, 0.5, 2], [0.5, -0.5, 2]]  # facing down
    quad = MS.mesh(pts, [0, 1, 2, 0, 2, 3])
    body += ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [8 8 8]\n' + quad + "AttributeEnd\n") if emit else ('Material "matte"\n' + quad)
    body += 'Material "matte" "rgb Kd" [0.5 0.5 0.5]\n' + MS.quad(MS.PANEL_FLOOR)
    body += MS.mesh([[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], [0, 1, 2, 0, 2, 3], ' "float alpha" [0]')
    return MS.write(tmp_path, body, name=name, strategy="spatial", spp=16, **MS.PATCH_VIEW)


def test_flag_word_with_many_lights_and_an_alpha_mask(binding, tmp_path):
    rng = np.random.default_rng(5)
    n = 512
    o = rng.uniform([-0.45, -0.45, 0.05], [0.45, 0.45, 0.5], (n, 3)).astype(np.float32)
    target = rng.uniform([-0.45, -0.45, 2], [0.45, 0.45, 2], (n, 3))
    d = (target - o).astype(np.float32)
    tmax = np.full(n, np.inf, np.float32)
    out = {}
    for emit in (True, False):
        host, gpu = _gpu(binding, _flag_scene(tmp_path, emit, f"flags_{int(emit)}.pbrt"))
        assert host.info["n_lights"] == (18 if emit else 16)
        if emit:
            assert sorted(host.prim_light()[host.prim_light() >= 0]) == [16, 17]
        res = []
        for instrumented in (False, True):
            prim, tb, _ = gpu.trace_closest(o, d, tmax, instrumented=instrumented)
            hit, _ = gpu.trace_any(o, d, np.full(n, 2.0, np.float32), instrumented=instrumented)
            res.append((prim, tb, hit))
        film, _ = gpu.render()
        out[emit] = (res, host.film_to_rgb(film), host.prim_light())
        gpu.close()
    for (prim_e, tb_e, hit_e), (prim_m, tb_m, hit_m) in zip(out[True][0], out[False][0]):
        assert (prim_e >= 0).all() and (out[True][2][prim_e] >= 16).all()  # every ray ends on the emitter, through the invisible quad
        assert np.array_equal(prim_e, prim_m) and np.array_equal(_bits(tb_e), _bits(tb_m))
        assert (hit_e != 0).all() and np.array_equal(hit_e, hit_m)
    lit, dark = out[True][1], out[False][1]
    assert lit[12:20, 12:20].min() > 10 * dark.max() and lit[12:20, 12:20].min() > 0.2  # Kd / Pi x 8 x E = 0.29 under the centre


# ---- 5. the IISPT direct pass -------------------------------------------------------------------------------------------------------
def _plane_points(binding, gpu, w, h, offsets):
    """Where the camera rays through the film positions (pixel + offset) meet the plane z = 0, in float64: (len(offsets), h, w, 3)."""
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    out = []
    for ox, oy in offsets:
        o, d = gpu.camera_rays(np.stack([px.reshape(-1) + ox, py.reshape(-1) + oy], 1).astype(np.float32))
        o, d = o.astype(np.float64), d.astype(np.float64)
        t = -o[:, 2] / d[:, 2]
        out.append((o + t[:, None] * d).reshape(h, w, 3))
    return np.array(out)


def _point_lights_over_plane(n, seed):
    rng = np.random.default_rng(seed)
    pos = np.float32(rng.uniform([-1.5, -1.5, 1.0], [1.5, 1.5, 2.5], (n, 3)))
    rgb = np.float32(rng.uniform(0.5, 2.0, (n, 3)))
    return pos, rgb, "".join(MS.point_light(p, c) for p, c in zip(pos, rgb))


def test_direct_pass_sums_sixteen_point_lights(binding, tmp_path):
    """16 passes of jittered samples per pixel against the float64 sum of the sixteen inverse-square terms at the pixel's centre;
    the band is the largest deviation of that sum from its centre value over a 5 x 5 grid on the pixel's footprint, and 1e-5 of
    the value for the float32 arithmetic."""
    pos, rgb, text = _point_lights_over_plane(16, 7)
    w, h = 24, 16
    body = text + f'Material "matte" "rgb Kd" [{MS.KD} {MS.KD} {MS.KD}]\n' + MS.quad(MS.WIDE_FLOOR)
    host, gpu = _gpu(binding, MS.write(tmp_path, body, integrator="iispt", w=w, h=h, spp=1, depth=1, eye="0 -4 3", look="0 0 0", fov=30))
    mon = gpu.render_direct(16)
    grid = [(x, y) for y in np.linspace(0, 1, 5) for x in np.linspace(0, 1, 5)]
    pts = _plane_points(binding, gpu, w, h, [(0.5, 0.5)] + grid)
    gpu.close()
    assert (mon[..., 3] == 16).all()
    img = mon[..., :3] / mon[..., 3:4]

    def radiance(x):
        v = pos.astype(np.float64)[None, None] - x[:, :, None, :]
        d2 = (v * v).sum(-1)
        return (MS.KD / np.pi * rgb.astype(np.float64)[None, None] * (v[..., 2] / np.sqrt(d2) / d2)[..., None]).sum(axis=2)

    want = radiance(pts[0])
    band = np.max([np.abs(radiance(x) - want) for x in pts[1:]], axis=0) + 1e-5 * want
    used = np.abs(img - want) / band
    print(f"direct pass, 16 lights: largest share of the band in use {used.max():.3f}; band / value up to {(band / want).max():.4f}")
    assert want.min() > 0 and (used <= 1).all(), used.max()


def test_direct_pass_takes_64_lights_and_refuses_65(binding, tmp_path):
    for n in (64, 65):
        _, _, text = _point_lights_over_plane(n, 8)
        body = text + 'Material "matte"\n' + MS.quad(MS.WIDE_FLOOR)
        host, gpu = _gpu(binding, MS.write(tmp_path, body, name=f"direct_{n}.pbrt", integrator="iispt", w=16, h=16, spp=1, depth=1, eye="0 -4 3", look="0 0 0"))
        if n == 64:
            mon = gpu.render_direct(1)
            assert np.isfinite(mon).all() and (mon[..., :3].min(axis=2) > 0).all()
        else:
            with pytest.raises(RuntimeError, match=r"65 light samples per vertex \(the lights' nsamples summed; at most 64\)"):
                gpu.render_direct(1)
        gpu.close()


def test_direct_pass_with_a_mirror_is_repeatable(binding, tmp_path):
    text, _ = MS.mixed_lights(12, 31)
    mirror = 'AttributeBegin\nMaterial "mirror"\nTranslate 0.5 0 0.6\nShape "sphere" "float radius" [0.6]\nAttributeEnd\n'
    host, gpu = _gpu(binding, MS.write(tmp_path, text + MS.SHELL + mirror, integrator="iispt", spp=1))
    a, b = gpu.render_direct(4), gpu.render_direct(4)
    gpu.close()
    assert a[..., :3].max() > 0 and np.isfinite(a).all() and np.array_equal(a, b)


# ---- 6. the IISPT frame and the C++ host ----------------------------------------------------------------------------------------------
def test_iispt_frame_with_twelve_lights_is_repeatable(binding, tmp_path):
    _iispt_modules()
    text, _ = MS.mixed_lights(12, 32)
    path = MS.write(tmp_path, text + MS.SHELL, integrator="iispt", spp=1, w=32, h=32)
    a, b = _iispt_image(binding, path), _iispt_image(binding, path)
    assert np.isfinite(a).all() and a.max() > 0 and np.array_equal(_bits(a), _bits(b))


def _mesh_room(tmp_path, integrator, name):
    pts, idx = MS.panel_mesh(4, 3)  # 24 emitting triangles
    body = MS.emitter(pts + np.array([0, 0, 1.0]), idx, MS.PANEL_L) + MS.SHELL
    return MS.write(tmp_path, body, name=name, integrator=integrator, spp=4 if integrator == "path" else 1, w=32, h=32)


def _read_pfm(path, w=32, h=32):
    raw = open(path, "rb").read()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], "<f4").reshape(h, w, 3)[::-1]


def test_cli_renders_an_emissive_mesh_under_both_integrators(binding, tmp_path):
    path = _mesh_room(tmp_path, "path", "cli_path.pbrt")
    out = tmp_path / "cli_path.pfm"
    p = subprocess.run([EXE, path, "--outfile", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    img = _read_pfm(out)
    host, gpu = _gpu(binding, path)
    assert host.info["n_lights"] == 24
    want = host.film_to_rgb(gpu.render()[0]).astype(np.float32)
    gpu.close()
    assert np.isfinite(img).all() and want.max() > 0 and np.array_equal(_bits(img), _bits(want))
    torch, _, _, ref_mod = _iispt_modules()
    torch.manual_seed(3)
    module = ref_mod.IISPTNet().eval()
    net_file = tmp_path / "net.iilenet"
    binding.save_net_weights(module.state_dict(), str(net_file), bn_eps=module.encoder1[3].eps)
    out = tmp_path / "cli_iispt.pfm"
    p = subprocess.run([EXE, _mesh_room(tmp_path, "iispt", "cli_iispt.pbrt"), f"--iisptNet={net_file}", "--iileIndirect=4", "--iileDirect=2",
                        "--outfile", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600,
                       env=dict(os.environ, IISPT_SCHEDULE_RADIUS_START="8"))
    assert p.returncode == 0, p.stdout
    img = _read_pfm(out)
    assert np.isfinite(img).all() and img.max() > 0


# ---- 7. the spatial table's cap -------------------------------------------------------------------------------------------------------
def test_spatial_table_cap_on_the_device(binding, tmp_path):
    """1 100 emitting triangles in a cubic room: refused under "spatial", rendered under "power" (its floor patch as the closed form
    says); 511 lights, the most the full grid admits, are tabulated."""
    host = binding.HostScene(path=MS.room_with_panel(tmp_path, 25, 22, "spatial", "cap_spatial.pbrt"))
    with pytest.raises(RuntimeError, match="1100 lights.*2202 MiB") as e:
        binding.GpuScene(host)
    assert '"power"' in str(e.value) and '"power"' in binding.gpu_lib().iile_last_error().decode()
    host, gpu = _gpu(binding, MS.room_with_panel(tmp_path, 25, 22, "power", "cap_power.pbrt", spp=64, **MS.PATCH_VIEW))
    assert host.info["n_lights"] == 1100
    film, _ = gpu.render()
    gpu.close()
    MS.patch_check(host.film_to_rgb(film), lift=MS.ROOM_LIFT, label="1100 triangles, power")
    path = MS.room_with_panel(tmp_path, 255, 1, "spatial", "cap_511.pbrt")
    text = open(path).read().replace("WorldBegin\n", "WorldBegin\n" + MS.point_light([0, 0, 1], [1, 1, 1]))
    open(path, "w").write(text)
    host, gpu = _gpu(binding, path)
    assert host.info["n_lights"] == 511
    p = np.array([[0, 0, 0.5], [1.5, 1.5, 3.9], [-9, -9, -9]], np.float32)
    light, pdf = gpu.light_choose(p, np.array([0.3, 0.6, 0.9], np.float32))
    gpu.close()
    assert ((light >= 0) & (light < 511)).all() and (pdf > 0).all() and (pdf <= 1).all()
