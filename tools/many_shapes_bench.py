"""Render time of scenes of many small shapes (960 x 540, 16 spp, maxdepth 5), where the traversal's leaf step tests a different
sphere, disk or cylinder in every lane of a wavefront:
  hall    60 cylinder columns with disk caps between a floor and a ceiling (hall_tess: the columns as triangles)
  field   32 x 32 = 1 024 small cylinders on a floor
  cloud   4 096 spheres over a floor (cloud_tess: every sphere an icosphere of 320 triangles)
Prints one JSON line per scene: the device time of each of `repeats` renders after one warm-up render, their median, the
scene's counts and a checksum of the film (two builds that render the same film print the same one). IILE_GPU_LIB selects
another build of libiile_gpu.so (binding.py): a build from before the tables were sized by the scene renders hall and field, and
refuses the cloud. Measured: profiles/many_shapes_ab.txt.
usage: python tools/many_shapes_bench.py [scene[,scene...]=hall,field,cloud] [repeats=5] [out.jsonl]"""
import json
import os
import sys
import tempfile
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as ge  # noqa: E402

HEADER = """LookAt {eye}  {look}  0 0 1
Camera "perspective" "float fov" [{fov}]
Film "image" "integer xresolution" [960] "integer yresolution" [540] "string filename" "many_shapes.exr"
PixelFilter "box"
Sampler "halton" "integer pixelsamples" [16]
Integrator "path" "integer maxdepth" [5]
WorldBegin
"""


def num(values):
    return " ".join(f"{np.float32(v):.9g}" for v in np.ravel(values))


def mesh(points, indices):
    return f'Shape "trianglemesh" "integer indices" [{" ".join(str(int(i)) for i in np.ravel(indices))}] "point P" [{num(points)}]\n'


def quad(x0, y0, x1, y1, z, up=True):
    pts = [[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]]
    return mesh(pts if up else pts[::-1], [0, 1, 2, 0, 2, 3])


def column_mesh(x, y, radius, z0, z1, segments):
    """A capped cylinder as triangles: `segments` wall quads (two triangles each) and two fans."""
    a = np.arange(segments) * 2 * np.pi / segments
    ring = np.stack([x + radius * np.cos(a), y + radius * np.sin(a)], 1)
    pts = np.concatenate([np.c_[ring, np.full(segments, z0)], np.c_[ring, np.full(segments, z1)], [[x, y, z0], [x, y, z1]]])
    idx = []
    for i in range(segments):
        j = (i + 1) % segments
        idx += [i, j, segments + j, i, segments + j, segments + i, 2 * segments, j, i, 2 * segments + 1, segments + i, segments + j]
    return mesh(pts, idx)


def icosphere(level):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f)


LIGHT = 'LightSource "point" "rgb I" [{i} {i} {i}] "point from" [{p}]\n'
MATTE = 'Material "matte" "rgb Kd" [{} {} {}]\n'


def hall(tessellated=False):
    body = LIGHT.format(i=60, p="0 -1 5.5") + LIGHT.format(i=40, p="3 9 5.5") + MATTE.format(0.6, 0.6, 0.6)
    body += quad(-8, -4, 8, 24, 0) + quad(-8, -4, 8, 24, 6, up=False) + MATTE.format(0.7, 0.6, 0.5)
    for row in range(10):
        for col in range(6):
            x, y = (col - 2.5) * 2.4, row * 2.4
            if tessellated:   # 60 x 4 704 triangles
                body += column_mesh(x, y, 0.35, 0.0, 5.0, 1176)
            else:
                body += (f'AttributeBegin\nTranslate {x:.9g} {y:.9g} 0\nShape "cylinder" "float radius" [0.35] "float zmin" [0] "float zmax" [5]\n'
                         'Shape "disk" "float radius" [0.35] "float height" [5]\nShape "disk" "float radius" [0.35] "float height" [0]\nAttributeEnd\n')
    return HEADER.format(eye="0.4 -3.5 1.7", look="0 8 2.2", fov=60) + body + "WorldEnd\n"


def field():
    body = LIGHT.format(i=80, p="0 0 6") + MATTE.format(0.6, 0.6, 0.6) + quad(-7, -7, 7, 7, 0) + MATTE.format(0.5, 0.6, 0.7)
    rng = np.random.default_rng(1)
    for j in range(32):
        for i in range(32):
            x, y = (i - 15.5) * 0.4, (j - 15.5) * 0.4
            body += (f'AttributeBegin\nTranslate {x:.9g} {y:.9g} 0\nRotate {rng.uniform(-20, 20):.9g} 1 0 0\nRotate {rng.uniform(-20, 20):.9g} 0 1 0\n'
                     f'Shape "cylinder" "float radius" [0.08] "float zmin" [0] "float zmax" [{rng.uniform(0.3, 0.9):.9g}]\nAttributeEnd\n')
    return HEADER.format(eye="0 -9 5", look="0 0 0.2", fov=50) + body + "WorldEnd\n"


def cloud(tessellated=False):
    body = LIGHT.format(i=80, p="0 -2 7") + MATTE.format(0.6, 0.6, 0.6) + quad(-6, -6, 6, 6, 0) + MATTE.format(0.7, 0.5, 0.4)
    rng = np.random.default_rng(2)
    centres = rng.uniform([-4, -4, 0.2], [4, 4, 4], (4096, 3))
    if tessellated:   # (one mesh of 4 096 x 320 triangles)
        v, f = icosphere(2)
        body += mesh(np.concatenate([v * 0.09 + c for c in centres]), np.concatenate([f + len(v) * i for i in range(len(centres))]))
    else:
        for c in centres:
            body += f'AttributeBegin\nTranslate {c[0]:.9g} {c[1]:.9g} {c[2]:.9g}\nShape "sphere" "float radius" [0.09]\nAttributeEnd\n'
    return HEADER.format(eye="0 -11 4", look="0 0 1.8", fov=50) + body + "WorldEnd\n"


SCENES = {"hall": hall, "hall_tess": lambda: hall(True), "field": field, "cloud": cloud, "cloud_tess": lambda: cloud(True)}


def main():
    names = (sys.argv[1] if len(sys.argv) > 1 else "hall,field,cloud").split(",")
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    b = ge._load_binding()
    if b.device_count() < 1:
        raise SystemExit("many_shapes_bench: no HIP device visible")
    for name in names:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, name + ".pbrt")
            open(path, "w").write(SCENES[name]())
            host = b.HostScene(path=path)
        line = {"scene": name, "gpu_lib": os.environ.get("IILE_GPU_LIB", "in-tree build"), "n_triangles": host.info["n_triangles"],
                "n_spheres": host.info["n_spheres"], "n_quadrics": host.quadric_count}
        try:
            gpu = b.GpuScene(host)
        except RuntimeError as e:
            line["refused"] = str(e)
        else:
            film, _ = gpu.render()  # (the first launch of every kernel)
            ms = [gpu.render()[1]["ms_total"] for _ in range(repeats)]
            line.update(ms=[round(m, 3) for m in ms], median_ms=round(float(np.median(ms)), 3),
                        film_mean=float(host.film_to_rgb(film).mean(dtype=np.float64)), film_crc32=zlib.crc32(film.tobytes()))
            gpu.close()
        print(json.dumps(line), flush=True)
        if out_path:
            open(out_path, "a").write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
