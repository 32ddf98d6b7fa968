"""The smallest scenes at which each branch of the IISPT render runner is live, for iispt_ref.py: every case is at most 64 triangles
on a 16 x 16 film, its tasks at most about 150 film pixels, hemi = 32 (fixed by the product). build() returns the truth's own
description of the scene (path_ref.Scene through path_cases.Builder, never the loader's tables) and the .pbrt text of the same numbers.

  room      a matte and plastic box room; task 12 x 10, tilesize 5: the last column (x = 11) is clamped at x1 - 1 behind x = 10, the
            last row (y = 9) is one short of a tile
  offset    the same room, a task strictly inside the film (x0 = 3, y0 = 2), tilesize 7, counter_base 777; and a one-pixel task, whose
            four neighbours are one hemi point
  specular  a mirror quad and a glass slab before matte walls (chains of 1 to 3 bounces, beta != 1), an uber pane (a multi-lobe
            Sample_f, the pass-through lobe in the chain), a black emitter in view and the pane's and the glass's zero-pdf samples (the black exit)
  missing   a floor and a back wall, open to every side: hemi points without a vertex beside pixels with one
  folded    a faceted ridge with per-vertex normals seen from above, the task's four hemi points on horizontal plates over it: the
            pixels' geometric normals are 19 to 30 degrees off their hemi points'; row 0 and column 0 of the hemispheres stay lit
  up_rule   a wall in the plane z = 0 seen along -z: hemi-point normals exactly (0, 0, 1), the other branch of the camera's `up`

Synthetic hemispheres: uniform in [0, 3) from a seeded generator, a tenth of the texels black, and (but for `folded`) camera row 0
and column 0 black: iispt_ref's docstring, "the hazard of row 0 and column 0". In these axis-aligned scenes the same hazard has two more
forms, met the same way: row 16 and column 16 (theta = Pi / 2, phi = Pi / 2) lie exactly in the horizon of a pixel on a plane at right
angles to its hemi point's (a floor pixel under a wall's hemi point), and the four texels (1 | 31, 1 | 31) have cos = sin^2(Pi / 32) =
0.0096, inside path_ref's GRAZE of 0.01. `folded` keeps all of them lit. Its normals are in general position, where a light sample's
direction falls inside GRAZE of the shading or of the geometric normal's plane with probability 0.01 each: 16 samples a pixel would
drop 16 x 2 x 0.01 = 0.3 of the pixels whatever the geometry. (Measured with 0.3 of the texels lit: 0.16 of the pixels, the
texel grid being denser than uniform near the poles.) Only lit texels reach BSDF::f, so `folded` has 0.9 of its texels black rather
than a tenth, row 0 and column 0 excepted, of which half are lit (column 0 is horizontal, and a fifth of it grazes the facets); and its facets are matte, so that no microfacet sample adds
grazing directions of its own.
"""
import numpy as np

import path_cases as PC
from path_cases import M

HEMI = 32


def _finish(b, eye, look, fov=45):
    return b.finish(eye, look, fov, 5, res=16)


def _emitter(b, y=3.9):
    b.quad(PC.BLACK, (-0.5, y, -0.5), (0.5, y, -0.5), (0.5, y, 0.5), (-0.5, y, 0.5), emit=(8.0, 8.0, 7.0))


def room():
    b = PC.Builder()
    PC.room(b, (-3, 0, -7), (3, 4, 3), M("matte", Kd=(0.6, 0.6, 0.5)), floor=M("plastic", Kd=(0.3, 0.3, 0.35), Ks=(0.4, 0.4, 0.4), roughness=0.15),
            back=M("matte", Kd=(0.3, 0.5, 0.7), sigma=20))
    _emitter(b)
    return _finish(b, "0.5 2.75 -6.5", "0 1 0.5")


def specular():
    b = PC.Builder()
    (x0, y0, z0), (x1, y1, z1) = (-3, 0, -7), (3, 4, 3)
    walls = M("matte", Kd=(0.6, 0.6, 0.6))
    # the room without its ceiling: rays that leave upwards find no surface
    b.quad(M("plastic", Kd=(0.4, 0.4, 0.4), Ks=(0.3, 0.3, 0.3), roughness=0.2), (x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0))
    b.quad(walls, (x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1))
    b.quad(walls, (x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0))
    b.quad(walls, (x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1))
    b.quad(walls, (x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0))
    glass = M("glass", index=1.5)
    b.quad(glass, (-1.5, 0.25, -1.0), (-1.5, 1.75, -1.0), (-0.25, 1.75, -1.0), (-0.25, 0.25, -1.0))
    b.quad(glass, (-1.5, 0.25, -0.5), (-0.25, 0.25, -0.5), (-0.25, 1.75, -0.5), (-1.5, 1.75, -0.5))
    b.quad(M("mirror", Kr=(0.9, 0.8, 0.7)), (0.25, 0.1, 1.5), (0.25, 2.1, 1.5), (2.25, 2.1, 0.5), (2.25, 0.1, 0.5))
    b.quad(M("uber", Kd=(0.5, 0.3, 0.3), Ks=(0.3, 0.3, 0.3), roughness=0.1, opacity=0.4), (0.25, 0.25, -1.25), (0.25, 1.75, -1.25), (1.5, 1.75, -1.25), (1.5, 0.25, -1.25))
    b.quad(PC.BLACK, (-1.0, 2.0, 2.5), (-1.0, 3.5, 2.5), (1.0, 3.5, 2.5), (1.0, 2.0, 2.5), emit=(10.0, 10.0, 8.0))
    return _finish(b, "0 1.5 -6", "0 1.25 0", 40)


def missing():
    b = PC.Builder()
    b.quad(M("plastic", Kd=(0.4, 0.4, 0.45), Ks=(0.3, 0.3, 0.3), roughness=0.2), (-2, 0, -4), (-2, 0, 3), (2, 0, 3), (2, 0, -4))
    b.quad(M("matte", Kd=(0.6, 0.5, 0.4)), (-2, 0, 3), (-2, 3.2, 3), (2, 3.2, 3), (2, 0, 3))
    b.quad(PC.BLACK, (-4.0, 6, -0.5), (-3.5, 6, -0.5), (-3.5, 6, 0.5), (-4.0, 6, 0.5), emit=(8.0, 8.0, 7.0))   # out of view
    return _finish(b, "0 2 -6", "0 1 0")


FOLDED_TASK = (1, 2, 13, 13, 12, 300, 17)


def _pinhole(eye, look, fov, res, px, py):
    """The direction through the centre of raster pixel (px, py) of a square perspective film under LookAt(eye, look, (0, 1, 0))."""
    eye, look = np.asarray(eye, np.float64), np.asarray(look, np.float64)
    d = (look - eye) / np.linalg.norm(look - eye)
    right = np.cross([0, 1, 0], d)
    right /= np.linalg.norm(right)
    up = np.cross(d, right)
    t = np.tan(np.radians(fov) / 2)
    return d + right * t * ((px + 0.5) / res * 2 - 1) + up * t * (1 - (py + 0.5) / res * 2)


def folded():
    b = PC.Builder()
    PC.room(b, (-6, -1, -6), (6, 9, 6), M("matte", Kd=(0.6, 0.6, 0.5)))
    rough = M("matte", Kd=(0.7, 0.5, 0.4), sigma=20)
    smooth = M("matte", Kd=(0.3, 0.4, 0.5))
    # seen from above: a ridge of six facets under the whole film, 19 to 30 degrees off the horizontal, per-vertex normals tilted a
    # further 10 to 20 degrees; the task's four hemi points (its corners: tilesize 12) lie on small horizontal plates above the ridge,
    # so a pixel of the ridge never shares a plane with a hemi point
    # (the facets slope along z: the poles of a plate's hemisphere, +-z, where its texels crowd, stay 19 degrees or more off every facet)
    xs = [-3.9, -2.6, -1.3, 0.0, 1.3, 2.6, 3.9]   # the facets' z
    ys = [0.0, 0.75, 1.25, 1.7, 1.25, 0.75, 0.0]
    offs = [(0.2, 0.15), (-0.25, 0.2), (0.3, -0.2), (-0.15, -0.3)]
    for k in range(6):
        face = [(-4.5, ys[k], xs[k]), (-4.5, ys[k + 1], xs[k + 1]), (4.5, ys[k + 1] + 0.6, xs[k + 1]), (4.5, ys[k] + 0.6, xs[k])]
        b.mesh(rough if k % 2 == 0 else smooth, face, [0, 1, 2, 0, 2, 3], normals=PC._tilted(face, offs[k % 4:] + offs[:k % 4]))
    eye, look, fov = (0.3, 8.0, -1.5), (0.0, 0.0, 0.0), 38
    x0, y0, x1, y1 = FOLDED_TASK[:4]
    for px, py in ((x0, y0), (x1 - 1, y0), (x0, y1 - 1), (x1 - 1, y1 - 1)):
        d = _pinhole(eye, look, fov, 16, px, py)
        c = np.asarray(eye) + d * ((3.5 - eye[1]) / d[1])
        cx, cz, r = float(np.float32(c[0])), float(np.float32(c[2])), 0.2
        b.quad(M("matte", Kd=(0.5, 0.5, 0.5)), (cx - r, 3.5, cz - r), (cx - r, 3.5, cz + r), (cx + r, 3.5, cz + r), (cx + r, 3.5, cz - r))
    b.quad(PC.BLACK, (-0.5, 8.9, 3.5), (0.5, 8.9, 3.5), (0.5, 8.9, 4.5), (-0.5, 8.9, 4.5), emit=(8.0, 8.0, 7.0))
    return _finish(b, "0.3 8 -1.5", "0 0 0", fov)


def up_rule():
    b = PC.Builder()
    b.quad(M("matte", Kd=(0.6, 0.5, 0.4)), (-5, -5, 0), (-5, 5, 0), (0.25, 5, 0), (0.25, -5, 0))
    b.quad(M("plastic", Kd=(0.3, 0.4, 0.5), Ks=(0.3, 0.3, 0.3), roughness=0.2), (0.25, -5, 0), (0.25, 5, 0), (5, 5, 0), (5, -5, 0))
    b.quad(PC.BLACK, (-9.0, 6, -0.5), (-8.5, 6, -0.5), (-8.5, 6, 0.5), (-9.0, 6, 0.5), emit=(8.0, 8.0, 7.0))   # out of view
    return _finish(b, "0.4 0.3 6", "0 0 0")


# tasks: (x0, y0, x1, y1, tilesize, counter_base, rng_seed)
CASES = {
    "room": dict(build=room, tasks=[(0, 0, 12, 10, 5, 0, 99)], nn_seed=3),
    "offset": dict(build=room, tasks=[(3, 2, 14, 13, 7, 777, 2024), (9, 6, 10, 7, 7, 5000, 5)], nn_seed=5),
    "specular": dict(build=specular, tasks=[(2, 3, 14, 14, 5, 40, 7)], nn_seed=7),
    "missing": dict(build=missing, tasks=[(4, 0, 14, 11, 5, 12, 31)], nn_seed=11),
    "folded": dict(build=folded, tasks=[FOLDED_TASK], nn_seed=13, lit_edges=True, black=0.9),
    "up_rule": dict(build=up_rule, tasks=[(2, 2, 13, 12, 5, 64, 23)], nn_seed=17),
}

# what each case is for: counts of the truth's stats that must not be zero, on the truth alone
LIVE = {
    "room": ("exit_vertex", "mis_light", "mis_bsdf", "bsdf_outside", "distinct_weights", "multi_lobe"),
    "offset": ("exit_vertex", "mis_light", "mis_bsdf", "distinct_weights"),
    "specular": ("exit_vertex", "exit_black", "chain_vertex", "missing_drew", "multi_lobe"),
    "missing": ("exit_none", "missing_drew", "mis_light", "mis_bsdf"),
    "folded": ("distinct_weights", "mis_light", "mis_bsdf", "bsdf_outside"),
    "up_rule": ("exit_vertex", "mis_light", "mis_bsdf", "multi_lobe"),
}


def hemispheres(case, k, grid):
    """The synthetic predictions of task k: (ny, nx, hemi, hemi, 3) float32, image row 0 first (camera row y is image row hemi - 1 - y)."""
    rng = np.random.default_rng(case["nn_seed"] + 1000 * k)
    nn = rng.uniform(0.0, 3.0, tuple(grid) + (HEMI, HEMI, 3)).astype(np.float32)
    lit = nn.copy()
    nn[rng.uniform(size=nn.shape[:4]) < case.get("black", 0.1)] = 0
    if case.get("lit_edges"):
        half = rng.uniform(size=nn.shape[:4]) < 0.5                                  # camera row 0 and column 0: every other texel lit
        lit[half] = 0
        nn[:, :, HEMI - 1], nn[:, :, :, 0] = lit[:, :, HEMI - 1], lit[:, :, :, 0]
    else:
        rows = lambda y: nn[:, :, HEMI - 1 - y]
        rows(0)[...] = 0                    # camera row y = 0
        nn[:, :, :, 0, :] = 0               # camera column x = 0
        rows(HEMI // 2)[...] = 0            # theta = Pi / 2 and phi = Pi / 2: the horizon of the planes at right angles
        nn[:, :, :, HEMI // 2, :] = 0
        for y in (1, HEMI - 1):             # sin^2(Pi / 32) = 0.0096 < GRAZE
            for x in (1, HEMI - 1):
                rows(y)[:, :, x] = 0
    return nn


# The probe cameras whose first-hit channels are held to the truth (iispt_ref.probe_first_hits): (position, direction) per scene, three
# or four at once: one along +z (the other branch of `up`), one oblique, one looking into a corner; distinct positions, so that a
# probe's normals and distances cannot come from its neighbour's camera.
PROBES = {
    "room": ([(0.5, 1.5, -2.0), (-1.0, 1.0, 0.25), (1.5, 0.75, 1.25), (-0.75, 2.5, -4.0)],
             [(0.0, 0.0, 1.0), (1.0, 0.5, 0.3), (1.0, -1.0, 1.0), (-0.3, -1.0, 0.2)]),
    "up_rule": ([(0.3, -0.2, -0.5), (-1.0, 0.5, -0.75), (0.6, 0.4, 0.7)],
                [(0.0, 0.0, 1.0), (0.5, 0.3, 1.0), (0.0, 0.0, -1.0)]),
}
PROBE_SHARE = 0.6   # a condition on the truth alone: the pixels whose whole footprint lies on one planar face, per probe
