"""Metal and substrate on the device held bit for bit to the CPU oracle (GPU), which restates them from metal.cpp, substrate.cpp and
reflection.cpp (tests/test_oracle_features.py pins that restatement to microfacet_ref.py): the BSDF probes over the catalogue of
test_gpu_metal_substrate.py, with and without a tilted geometric normal; per-sample Li; whole films of box rooms with metal and
substrate blobs (constant, anisotropic, unremapped, image-textured and bump-mapped) with both kernel builds, counters included; the
IISPT direct pass, probe pass and gather on the same rooms; and a film under the Sobol' sampler."""
import numpy as np
import pytest

import boxroom
from test_gpu_metal_substrate import CASES, PLANE, _direction_pairs, _sphere_dirs
from test_gpu_parity import assert_bitwise
from test_oracle_features import SPECULAR_CASES, specular_probe_inputs
from quadric_ref import write_scene

pytestmark = pytest.mark.gpu

LIGHT = 'LightSource "point" "rgb I" [1 1 1] "point from" [0 0 5]\n'
N = 4000
COUNTERS = (("closest_rays", "regular_rays"), ("shadow_rays", "shadow_rays"), ("tri_tests", "tri_tests"), ("nodes_closest", "nodes_closest"),
            ("nodes_any", "nodes_any"), ("nee_evals", "nee_evals"), ("zero_radiance", "zero_radiance"), ("path_length", "path_length"))


@pytest.mark.parametrize("case", list(CASES) + ["metal_alpha_zero"])
def test_bsdf_probes_bitwise(binding, oracle, tmp_path, case):
    line = CASES[case][0] if case in CASES else 'Material "metal" "bool remaproughness" "false" "float roughness" [0]'
    host = binding.HostScene(path=write_scene(tmp_path, line + "\n" + PLANE + LIGHT, depth=1))
    gpu = binding.GpuScene(host)
    rng = np.random.default_rng(300 + len(case))
    wo, wi = _direction_pairs(rng, N)
    assert_bitwise(gpu.bsdf_eval(0, wo, wi), oracle.bsdf_eval(host, 0, wo, wi), f"{case}: bsdf_eval")
    wos = _sphere_dirs(rng, 2 * N)
    wos = wos[np.abs(wos[:, 2]) > 0.02][:N].astype(np.float32)
    u = rng.random((len(wos), 2)).astype(np.float32)
    u[:64, 0] = np.float32(0.5)           # substrate's switch between its two sampling halves
    u[64:128, 0] = np.float32(float.fromhex("0x1.fffffep-1"))
    dev, ref = gpu.bsdf_sample(0, wos, u), oracle.bsdf_sample(host, 0, wos, u)
    assert_bitwise(dev[:, 3:], ref[:, 3:], f"{case}: bsdf_sample f, pdf")
    ok = ref[:, 6] > 0
    assert ok.mean() > 0.5 or case not in CASES  # (alpha 0: D is 0 / 0 at the sampled half vector, the pdf NaN)
    assert_bitwise(dev[ok, :3], ref[ok, :3], f"{case}: bsdf_sample wi")
    t = np.radians(35)
    ng = np.array([np.sin(t), 0, np.cos(t)], np.float32)
    assert_bitwise(gpu.bsdf_eval_ng(0, ng, wo, wi), oracle.bsdf_eval(host, 0, wo, wi, ng=ng), f"{case}: bsdf_eval_ng")
    dev, ref = gpu.bsdf_sample_ng(0, ng, wos, u), oracle.bsdf_sample(host, 0, wos, u, ng=ng)
    assert_bitwise(dev[:, 3:], ref[:, 3:], f"{case}: bsdf_sample_ng f, pdf")
    ok = ref[:, 6] > 0
    assert_bitwise(dev[ok, :3], ref[ok, :3], f"{case}: bsdf_sample_ng wi")
    gpu.close()


@pytest.mark.parametrize("case", list(SPECULAR_CASES))
def test_bsdf_probe_with_specular_lobes_bitwise(binding, oracle, tmp_path, case):
    """bsdf_sample_f with allow_specular, as the path's bounce calls it: the pass-through, specular reflection, specular
    transmission and FresnelSpecular lobes, which bsdf_sample never reaches. f, pdf and the two flags everywhere, wi where a
    direction was sampled; plastic, which has no specular lobe, gives what bsdf_sample gives."""
    host = binding.HostScene(path=write_scene(tmp_path, SPECULAR_CASES[case][0] + "\n" + PLANE + LIGHT, depth=1))
    gpu = binding.GpuScene(host)
    wo, u = specular_probe_inputs(case)
    dev, ref = gpu.bsdf_sample_specular(0, wo, u), oracle.bsdf_sample_specular(host, 0, wo, u)
    assert_bitwise(dev[:, 3:], ref[:, 3:], f"{case}: bsdf_sample_specular f, pdf, flags")
    ok = ref[:, 6] > 0
    assert ok.mean() > 0.5
    assert_bitwise(dev[ok, :3], ref[ok, :3], f"{case}: bsdf_sample_specular wi")
    if case == "plastic":
        plain = gpu.bsdf_sample(0, wo, u)
        assert_bitwise(dev[:, 3:7], plain[:, 3:], "plastic: bsdf_sample_specular against bsdf_sample")
        assert_bitwise(dev[ok, :3], plain[ok, :3], "plastic: wi against bsdf_sample")
    gpu.close()


def _room(binding, tmp_path, seed, light, textured):
    path = tmp_path / f"room_metal_{seed}_{light}_{int(textured)}.pbrt"
    path.write_text(boxroom.boxroom_pbrt(xres=64, yres=48, spp=3, ico_levels=3, n_blobs=12, wall_n=12, seed=seed, maxdepth=6, light=light,
                                         materials="metal", textures=str(tmp_path / "img") if textured else None))
    return binding.HostScene(path=str(path))


ROOMS = [(1, "multi", False), (2, "area", True), (3, "quad", True), (4, "spot", False)]


@pytest.mark.parametrize("seed,light,textured", ROOMS)
def test_metal_rooms_bitwise(binding, oracle, tmp_path, seed, light, textured):
    """Box rooms whose blobs are metal and substrate: per-sample Li, then film and every counter bitwise with the instrumented kernels,
    and the film with the plain kernels over two passes."""
    scene = _room(binding, tmp_path, seed, light, textured)
    gpu = binding.GpuScene(scene)
    rng = np.random.default_rng(seed)
    h, w = scene.film_shape
    px, py, k = rng.integers(0, w, 512), rng.integers(0, h, 512), rng.integers(0, 3, 512)
    L, nr = gpu.li_samples(px, py, k)
    rL, rnr = oracle.li(scene, px, py, k)
    assert_bitwise(L, rL, f"room {seed}: Li per sample")
    assert np.array_equal(nr, rnr)
    film, st = gpu.render(collect_stats=True)
    ref, ost = oracle.render(scene)
    assert float(scene.film_to_rgb(ref).mean()) > 1e-3
    assert_bitwise(film, ref, f"room {seed} / {light}: film")
    for k_dev, k_ref in COUNTERS:
        assert st[k_dev] == ost[k_ref], k_dev
    plain, _ = gpu.render(spp_per_pass=2)
    assert_bitwise(plain, ref, f"room {seed} / {light}: film, uninstrumented kernels, two passes")
    gpu.close()


@pytest.mark.parametrize("seed,light,textured", ROOMS[:2])
def test_metal_rooms_iispt_paths_bitwise(binding, oracle, tmp_path, seed, light, textured):
    """The IISPT direct pass, the probe pass and the gather on the same rooms."""
    torch = pytest.importorskip("torch")
    scene = _room(binding, tmp_path, seed, light, textured)
    gpu = binding.GpuScene(scene)
    assert np.array_equal(gpu.render_direct(2).view(np.uint64), oracle.iispt_direct(scene, 2).view(np.uint64))
    rng = np.random.default_rng(seed)
    pos = rng.uniform((-8, -8, -2), (8, 8, 8), (4, 3)).astype(np.float32)
    d = rng.standard_normal((4, 3)).astype(np.float32)
    inten, nrm, dist, _ = gpu.render_probes(pos, d)
    for i in range(len(pos)):
        oi, on, od = oracle.render_probe(scene, pos[i], d[i])
        assert_bitwise(inten[i], oi, f"room {seed}: probe {i} intensity")
        assert_bitwise(nrm[i], on, f"room {seed}: probe {i} normals")
        assert_bitwise(dist[i], od, f"room {seed}: probe {i} distances")
    h, w = scene.film_shape
    task = binding.IisptTask(0, 0, w, h, 12, 40, 2024)
    valid, hp, hd = gpu.iispt_hemi_points(task)
    rv, rp, rd = oracle.iispt_hemi_points(scene, task)
    assert np.array_equal(valid, rv) and valid.any()
    assert_bitwise(hp, rp, "hemi point positions")
    assert_bitwise(hd, rd, "hemi point directions")
    nn = rng.uniform(0.0, 1.5, valid.shape + (32, 32, 3)).astype(np.float32)
    nn_t = torch.from_numpy(nn).cuda()
    out_t = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    gpu.iispt_gather(task, valid, hp, hd, nn_device_ptr=nn_t.data_ptr(), out_device_ptr=out_t.data_ptr())
    torch.cuda.synchronize()
    out = out_t.cpu().numpy()
    ref = oracle.iispt_gather(scene, task, valid, hp, hd, nn)
    assert_bitwise(out, ref, f"room {seed}: gather")
    assert (ref[..., 3] == 0.5).mean() > 0.5
    gpu.close()


def test_metal_room_sobol_bitwise(binding, oracle, tmp_path):
    path = tmp_path / "room_metal_sobol.pbrt"
    path.write_text(boxroom.boxroom_pbrt(xres=48, yres=32, spp=4, ico_levels=3, n_blobs=12, wall_n=12, seed=5, maxdepth=5, light="multi",
                                         materials="metal", textures=str(tmp_path / "img")))
    scene = binding.HostScene(path=str(path), sampler="sobol")
    gpu = binding.GpuScene(scene)
    film, st = gpu.render(collect_stats=True)
    ref, ost = oracle.render(scene)
    assert float(scene.film_to_rgb(ref).mean()) > 1e-3
    assert_bitwise(film, ref, "Sobol' film")
    for k_dev, k_ref in COUNTERS:
        assert st[k_dev] == ost[k_ref], k_dev
    gpu.close()
