"""IISPT reference mode without a device: the grid `iile_pbrt --reference=N --reference-list` enumerates (render_reference's loop,
src/integrators/iispt.cpp:468-505), the $IISPT_REFERENCE_CONTROL_MOD / _MATCH split, the resume logic of exec_if_not_exists /
exec_if_one_not_exists (iispt.cpp:142-168), the errors that need no device, and the C entry point's argument checks."""
import ctypes
import os
import subprocess

import pytest

from quadric_ref import write_scene

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
BODY = 'Material "matte"\nShape "sphere" "float radius" [1]\n'
W, H, TILES = 40, 30, 4


def run(scene, *args, cwd, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("IISPT_REFERENCE_CONTROL")}
    e.update(env or {})
    return subprocess.run([EXE, scene, *args], cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def listing(scene, *args, cwd, env=None):
    p = run(scene, f"--reference={TILES}", "--reference-list", *args, cwd=cwd, env=env)
    assert p.returncode == 0, p.stderr
    rows = []
    for line in p.stdout.splitlines():
        f = line.split()
        rows.append(dict(idx=int(f[0]), x=int(f[1]), y=int(f[2]), files=f[3:7], one=f[7], p=f[8]))
    return rows


def expected_grid(w, h, tiles):
    """iispt.cpp:471-472 and :498-499 restated: the interval is extent / tiles (integer), the loops run `px < extent` — so an extent that
    is no multiple of the interval lets one more row or column in — and ref_idx counts every pixel from 1."""
    ix, iy = w // tiles, h // tiles
    out, idx = [], 0
    px_y = 0
    while px_y < h:
        px_x = 0
        while px_x < w:
            idx += 1
            out.append((idx, px_x, px_y))
            px_x += ix
        px_y += iy
    return out


@pytest.fixture
def scene(binding, tmp_path):
    return write_scene(tmp_path, BODY, w=W, h=H, spp=1)


def test_reference_list_enumerates_the_grid(scene, tmp_path):
    rows = listing(scene, cwd=tmp_path)
    want = expected_grid(W, H, TILES)
    assert [x for _, x, _ in want[:4]] == [0, 10, 20, 30] and sorted({y for _, _, y in want}) == [0, 7, 14, 21, 28]  # (a fifth row: 30 = 4 * 7 + 2)
    assert len(want) == 20 and want[0][0] == 1
    assert [(r["idx"], r["x"], r["y"]) for r in rows] == want
    r = rows[6]
    assert r["files"] == [f"out/{k}_{r['x']}_{r['y']}.pfm" for k in "dznp"]   # generate_reference_name
    assert all(r["one"] == "pending" and r["p"] == "pending" for r in rows)
    assert not (tmp_path / "out").exists()   # listing touches nothing


def test_control_mod_match_partition_the_grid(scene, tmp_path):
    whole = [r["idx"] for r in listing(scene, cwd=tmp_path)]
    parts = [[r["idx"] for r in listing(scene, cwd=tmp_path, env={"IISPT_REFERENCE_CONTROL_MOD": "3", "IISPT_REFERENCE_CONTROL_MATCH": str(m)})]
             for m in range(3)]
    for m, part in enumerate(parts):
        assert part and all(i % 3 == m for i in part)   # `(ref_idx % reference_control_mod) != reference_control_match` skips
    assert sorted(sum(parts, [])) == whole and len(set(sum(parts, []))) == len(whole)


def test_gpurank_deals_the_list_by_position(scene, tmp_path):
    whole = [r["idx"] for r in listing(scene, cwd=tmp_path)]
    shares = [[r["idx"] for r in listing(scene, "--gpurank", f"{k}/3", cwd=tmp_path)] for k in range(3)]
    assert shares == [whole[k::3] for k in range(3)]


def test_resume_marks_what_is_on_disk(scene, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    for k in "dznp":
        (out / f"{k}_10_7.pfm").write_bytes(b"x")      # complete
    for k in "dnp":
        (out / f"{k}_20_14.pfm").write_bytes(b"x")     # z alone is missing
    (out / "p_0_0.pfm").write_bytes(b"x")              # p alone is there
    by_px = {(r["x"], r["y"]): (r["one"], r["p"]) for r in listing(scene, cwd=tmp_path)}
    assert by_px[(10, 7)] == ("present", "present")
    assert by_px[(20, 14)] == ("pending", "present")   # the 1-sample group only (exec_if_one_not_exists)
    assert by_px[(0, 0)] == ("pending", "present")
    assert by_px[(30, 21)] == ("pending", "pending")
    off = {(r["x"], r["y"]): (r["one"], r["p"]) for r in listing(scene, "--reference_resume=0", cwd=tmp_path)}
    assert set(off.values()) == {("pending", "pending")}   # referenceResume == 0: everything is rendered again


def test_too_many_tiles_is_an_error_before_anything_is_made(scene, tmp_path):
    p = run(scene, "--reference=31", cwd=tmp_path)   # 30 / 31 == 0
    assert p.returncode != 0
    assert "Reference tile interval too small. Image resolution could be too small or reference tiles too many" in p.stderr
    assert not (tmp_path / "out").exists()


def test_reference_refuses_the_frame_flags_and_an_unwritable_directory(scene, tmp_path):
    p = run(scene, "--reference=4", "--iisptNet=weights.bin", cwd=tmp_path)
    assert p.returncode != 0 and "--iisptNet" in p.stderr and "no HIP device" not in p.stderr
    assert not (tmp_path / "out").exists()
    (tmp_path / "out").write_text("a file where the directory should be")
    p = run(scene, "--reference=4", cwd=tmp_path)
    assert p.returncode != 0 and "out" in p.stderr and "no HIP device" not in p.stderr
    p = run(scene, "--reference-list", cwd=tmp_path)
    assert p.returncode != 0 and "--reference=N" in p.stderr


def test_entry_point_checks_its_arguments(binding):
    lib = binding.gpu_lib()
    for name in ("iile_render_probes_reference", "iile_test_probe_ref_group", "iile_reference_points"):
        assert getattr(lib, name) is not None
    assert ctypes.sizeof(binding.ProbeRefParams) == 5 * 4 + 4 + 8
    scene = ctypes.create_string_buffer(64)   # never looked into: every check below comes first
    xyz = (ctypes.c_float * 3)(0, 0, 1)
    img = (ctypes.c_float * (32 * 32 * 3))()
    call = lambda prm, sc=scene, out=img: lib.iile_render_probes_reference(sc, 1, xyz, xyz, prm, out, None, None, None, None)
    ok = binding.ProbeRefParams(3, 0, 4, 0, 0, None)
    assert call(None) == 1 and b"null argument" in lib.iile_last_error()   # IILE_ERR_ARG
    assert call(ctypes.byref(ok), sc=None) == 1 and call(ctypes.byref(ok), out=None) == 1
    assert call(ctypes.byref(binding.ProbeRefParams(3, 0, 0, 0, 0, None))) == 1 and b"n_samples < 1" in lib.iile_last_error()
    assert call(ctypes.byref(binding.ProbeRefParams(0, 0, 4, 0, 0, None))) == 1 and b"max_depth" in lib.iile_last_error()
    assert call(ctypes.byref(binding.ProbeRefParams(15, 0, 4, 0, 0, None))) == 1
    assert call(ctypes.byref(binding.ProbeRefParams(3, -1, 4, 0, 0, None))) == 1
    assert lib.iile_reference_points(scene, 1, None, None, None, None) == 1
    assert lib.iile_test_probe_ref_group(None, 1) == 1


def test_reference_mode_has_no_cpu_path(binding):
    if binding.device_count() > 0:
        pytest.skip("a GPU is visible")
    lib = binding.gpu_lib()
    scene = ctypes.create_string_buffer(64)
    xyz = (ctypes.c_float * 3)(0, 0, 1)
    img = (ctypes.c_float * (32 * 32 * 3))()
    prm = binding.ProbeRefParams(3, 0, 4, 0, 0, None)
    assert lib.iile_render_probes_reference(scene, 1, xyz, xyz, ctypes.byref(prm), img, None, None, None, None) == 2   # IILE_ERR_NO_DEVICE
    assert b"no HIP device" in lib.iile_last_error()
    valid = (ctypes.c_uint8 * 1)()
    assert lib.iile_reference_points(scene, 1, xyz, valid, xyz, xyz) == 2 and b"no HIP device" in lib.iile_last_error()
