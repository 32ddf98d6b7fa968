"""Throughput of the IISPT reference mode's many-sample probe pass (iile_render_probes_reference): N hemispheres of 32 x 32 pixels x S
samples on the box room (tests/boxroom.py, the 36 k-triangle default), placed on the reference mode's own points (a grid of film pixels,
iile_reference_points), at the reference mode's depth 3. Prints one JSON line: hemispheres per second, probe samples per second and
the closest-hit rays the pass traced per second (extension + MIS rays; shadow rays are not counted by the uninstrumented kernels).
usage: python tools/reference_bench.py [n_probes=64] [samples=4096] [repeats=3] [out.json]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import __graft_entry__ as ge  # noqa: E402
import boxroom  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_path = sys.argv[4] if len(sys.argv) > 4 else None
b = ge._load_binding()
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "room.pbrt")
    open(path, "w").write(boxroom.boxroom_pbrt(xres=256, yres=256, spp=1))
    host = b.HostScene(path=path)
gpu = b.GpuScene(host)
side = int(np.ceil(np.sqrt(n * 1.2)))
grid = np.array([[(x + 0.5) * 256 / side, (y + 0.5) * 256 / side] for y in range(side) for x in range(side)], np.float32)
valid, pos, dr = gpu.reference_points(grid)
pos, dr = pos[valid != 0][:n], dr[valid != 0][:n]
n = len(pos)
gpu.render_probes_reference(pos[:1], dr[:1], 1)  # (the first launch of every kernel)
runs = []
for _ in range(reps):
    t0 = time.time()
    st = gpu.render_probes_reference(pos, dr, spp)[4]
    wall = time.time() - t0
    rays = st["ext_rays_traced"] + st["mis_rays_traced"]
    runs.append({"wall_ms": round(wall * 1e3, 1), "device_ms": round(st["ms_total"], 1), "launch_sets": st["n_passes"],
                 "closest_hit_rays": rays, "workspace_MiB": st["workspace_bytes"] >> 20})
best = min(runs, key=lambda r: r["device_ms"])
line = {"scene": "boxroom 256x256 default", "hemispheres": n, "hemi": 32, "samples": spp, "max_depth": 3,
        "hemispheres_per_s": round(n / (best["device_ms"] * 1e-3), 2), "probe_samples_per_s": round(n * 1024 * spp / (best["device_ms"] * 1e-3)),
        "closest_hit_rays_per_s": round(best["closest_hit_rays"] / (best["device_ms"] * 1e-3)), "runs": runs}
print(json.dumps(line))
if out_path:
    open(out_path, "w").write(json.dumps(line, indent=1) + "\n")
