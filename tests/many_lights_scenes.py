"""Scenes of more than eight lights, as .pbrt text and as the restatement's own description (lightdistrib_ref.py), for
test_many_lights_scenes.py (no GPU) and test_gpu_many_lights.py. Every number is written with nine digits, so the loader reads
the float32 the restatement holds."""
import numpy as np

import lightdistrib_ref as LD


def num(values):
    return " ".join(f"{np.float32(v):.9g}" for v in np.ravel(values))


def header(w=32, h=24, spp=4, depth=3, fov=50, eye="0 -5.5 2.6", look="0 0 0.8", up="0 0 1", integrator="path", strategy=None, center=False,
           name="many.exr"):
    strat = f' "string lightsamplestrategy" "{strategy}"' if strategy else ""
    return (f'LookAt {eye}  {look}  {up}\nCamera "perspective" "float fov" [{fov}]\n'
            f'Film "image" "integer xresolution" [{w}] "integer yresolution" [{h}] "string filename" "{name}"\nPixelFilter "box"\n'
            f'Sampler "halton" "integer pixelsamples" [{spp}] "bool samplepixelcenter" "{"true" if center else "false"}"\n'
            f'Integrator "{integrator}" "integer maxdepth" [{depth}]{strat}\nWorldBegin\n')


def write(tmp_path, body, name="many.pbrt", **kw):
    p = tmp_path / name
    p.write_text(header(**kw) + body + "WorldEnd\n")
    return str(p)


def mesh(points, indices, extra=""):
    return f'Shape "trianglemesh" "integer indices" [{" ".join(str(int(i)) for i in np.ravel(indices))}] "point P" [{num(points)}]{extra}\n'


def quad(corners):
    return mesh(corners, [0, 1, 2, 0, 2, 3])


def point_light(pos, intensity):
    return f'LightSource "point" "rgb I" [{num(intensity)}] "point from" [{num(pos)}]\n'


def spot_light(pos, to, intensity, cone=30.0, delta=5.0):
    return (f'LightSource "spot" "rgb I" [{num(intensity)}] "point from" [{num(pos)}] "point to" [{num(to)}] '
            f'"float coneangle" [{num([cone])}] "float conedeltaangle" [{num([delta])}]\n')


def emitter(points, indices, L, two_sided=False):
    side = ' "bool twosided" "true"' if two_sided else ""
    return f'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [{num(L)}]{side}\n' + mesh(points, indices) + "AttributeEnd\n"


# the shell every mixed scene stands in: a floor and a back wall; with the emitters inside, the world bound is BOUNDS
FLOOR = [[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]]
WALL = [[-2, 2, 0], [2, 2, 0], [2, 2, 3], [-2, 2, 3]]
BOUNDS = ([-2, -2, 0], [2, 2, 3])
SHELL = 'Material "matte" "rgb Kd" [0.6 0.6 0.6]\n' + quad(FLOOR) + quad(WALL)


def mixed_lights(n, seed):
    """n lights, in turn a point light, a spot light aimed at the floor, a one-sided triangle facing mostly down and a two-sided
    one, all well inside BOUNDS -> (.pbrt text, [restated lights]) in declaration order."""
    chunks, lights = mixed_light_chunks(n, seed)
    return "".join(chunks), lights


def mixed_light_chunks(n, seed):
    """mixed_lights with the text as one piece per light."""
    rng = np.random.default_rng(seed)
    text, lights = [], []
    for i in range(n):
        pos = np.float32(rng.uniform([-1.7, -1.7, 0.6], [1.7, 1.7, 2.7]))
        rgb = np.float32(rng.uniform(0.5, 4.0, 3))
        kind = i % 4
        if kind == 0:
            text.append(point_light(pos, rgb))
            lights.append(LD.Point(pos, rgb))
        elif kind == 1:
            to = np.float32([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 0.0])
            text.append(spot_light(pos, to, 4 * rgb))
            lights.append(LD.Spot(pos, to, 4 * rgb))
        else:
            a, b = rng.uniform(-0.25, 0.25, 3), rng.uniform(-0.25, 0.25, 3)
            while np.linalg.norm(np.cross(a, b)) < 0.3 * np.linalg.norm(a) * np.linalg.norm(b) or min(np.linalg.norm(a), np.linalg.norm(b)) < 0.1:
                a, b = rng.uniform(-0.25, 0.25, 3), rng.uniform(-0.25, 0.25, 3)  # (no slivers: lightdistrib_ref.py's band for the normal)
            tri = np.float32([pos, pos + a, pos + b])
            if np.cross(tri[1] - tri[0], tri[2] - tri[0])[2] > 0:  # face down
                tri = tri[[0, 2, 1]]
            text.append(emitter(tri, [0, 1, 2], 20 * rgb, two_sided=kind == 3))
            lights.append(LD.Tri(tri[0], tri[1], tri[2], 20 * rgb, two_sided=kind == 3))
    return text, lights


def mixed_scene(tmp_path, n, seed, strategy, name=None, **kw):
    text, lights = mixed_lights(n, seed)
    path = write(tmp_path, text + SHELL, name=name or f"mixed_{n}_{strategy}.pbrt", strategy=strategy, **kw)
    return path, LD.Scene(lights, *BOUNDS)


def lookups(scene, m, seed):
    """m points and samples for choose(): 25 points in each of m / 25 voxels — among them the grid's eight corner voxels, entered from
    points OUTSIDE the bounds (Lookup clamps them) — each strictly inside its voxel (a tenth of a voxel from its faces, so that no
    rounding of Offset() moves it next door). float32, as the device takes them."""
    rng = np.random.default_rng(seed)
    nv = scene.nv
    n_vox = m // 25
    vox = np.stack([rng.integers(0, nv[k], n_vox) for k in range(3)], 1)
    corners = np.array([[x, y, z] for x in (0, nv[0] - 1) for y in (0, nv[1] - 1) for z in (0, nv[2] - 1)])
    vox[:8] = corners
    frac = rng.uniform(0.1, 0.9, (n_vox, 25, 3))
    g = (vox[:, None, :] + frac) / nv  # position in the bounds, in [0, 1]^3
    g[:8] = np.where(corners[:, None, :] == 0, -rng.uniform(0.05, 0.5, (8, 25, 3)), 1 + rng.uniform(0.05, 0.5, (8, 25, 3)))
    p = (scene.bmin + g.reshape(-1, 3) * (scene.bmax - scene.bmin)).astype(np.float32)
    u = rng.random(len(p)).astype(np.float32)
    u[u >= 1] = np.float32(0.5)
    return p, u, vox


# ---- a rectangular emitter over a floor, tessellated or not --------------------------------------------------------------------
PANEL = np.array([[-0.8, -0.5, 1.5], [0.8, -0.5, 1.5], [0.8, 0.5, 1.5], [-0.8, 0.5, 1.5]])  # facing down when wound 0 3 2 1
PANEL_L = np.array([6.0, 5.0, 4.0])
PANEL_FLOOR = [[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0]]
KD = 0.5
WIDE_FLOOR = [[-50, -50, 0], [50, -50, 0], [50, 50, 0], [-50, 50, 0]]  # wider than any view of the direct-pass tests


def panel_mesh(nx, ny):
    """The panel as nx x ny cells of two triangles, wound to face the floor."""
    xs, ys = np.linspace(PANEL[0, 0], PANEL[1, 0], nx + 1), np.linspace(PANEL[0, 1], PANEL[2, 1], ny + 1)
    pts = np.array([[x, y, PANEL[0, 2]] for y in ys for x in xs])
    idx = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            idx += [a, d, c, a, c, b]
    return pts, idx


def panel_scene(tmp_path, nx, ny, strategy, extra="", name=None, spp=64, **kw):
    pts, idx = panel_mesh(nx, ny)
    body = extra + emitter(pts, idx, PANEL_L) + f'Material "matte" "rgb Kd" [{KD} {KD} {KD}]\n' + quad(PANEL_FLOOR)
    view = dict(PATCH_VIEW, spp=spp)
    view.update(kw)
    return write(tmp_path, body, name=name or f"panel_{nx}x{ny}_{strategy}.pbrt", strategy=strategy, **view)


def panel_radiance(p=(0.0, 0.0, 0.0), lift=0.0):
    """What the floor at p reflects towards any direction: Kd / Pi x L x the closed-form irradiance of the rectangle (`lift` higher)."""
    return KD / np.pi * PANEL_L * LD.rect_irradiance(PANEL + np.array([0, 0, lift]), p, np.array([0.0, 0.0, 1.0]))


ROOM_LIFT = 2.0


def room_with_panel(tmp_path, nx, ny, strategy, name, **view):
    """A cubic room of side 4 (the full 64^3 grid), open towards -y, with an nx x ny panel of emitting triangles ROOM_LIFT higher
    than PANEL, under its ceiling."""
    pts, idx = panel_mesh(nx, ny)
    pts = pts + np.array([0, 0, ROOM_LIFT])
    lo, hi = -2.0, 2.0
    walls = [[[lo, lo, 0], [hi, lo, 0], [hi, hi, 0], [lo, hi, 0]], [[lo, lo, 4], [hi, lo, 4], [hi, hi, 4], [lo, hi, 4]],
             [[lo, hi, 0], [hi, hi, 0], [hi, hi, 4], [lo, hi, 4]], [[lo, lo, 0], [lo, hi, 0], [lo, hi, 4], [lo, lo, 4]],
             [[hi, lo, 0], [hi, hi, 0], [hi, hi, 4], [hi, lo, 4]]]
    body = emitter(pts, idx, PANEL_L) + f'Material "matte" "rgb Kd" [{KD} {KD} {KD}]\n' + "".join(quad(w) for w in walls)
    kw = dict(eye="0 -1.9 2", look="0 0 1.5")
    kw.update(view)
    return write(tmp_path, body, name=name, strategy=strategy, **kw)


PATCH_VIEW = dict(w=32, h=32, fov=4, eye="0 0 1.2", look="0 0 0", up="0 1 0", depth=1)  # straight down at the floor under the panel's centre


def patch_check(rgb, lift=0.0, label=""):
    """The mean of the film's central 8 x 8 pixels (PATCH_VIEW: 21 mm of floor around the origin) against the closed form, within four
    standard errors of that mean as the pixels' spread estimates it -> (mean, closed form, standard error), per channel."""
    half = 1.2 * np.tan(np.radians(2.0)) * 8 / 32  # the patch's half-width on the floor
    centre, corner = panel_radiance((0, 0, 0), lift), panel_radiance((half, half, 0), lift)
    assert np.abs(corner / centre - 1).max() < 1e-3  # the closed form varies by less than 0.1 % across the patch
    # (the closed form at the 64 pixel centres, averaged: film x and y run along the floor's x and y, up to signs the panel does not see)
    at = (np.arange(12, 20) + 0.5 - 16) / 16 * 1.2 * np.tan(np.radians(2.0))
    want = np.mean([panel_radiance((x, y, 0), lift) for y in at for x in at], axis=0)
    patch = np.asarray(rgb, np.float64)[12:20, 12:20].reshape(-1, 3)
    mean, se = patch.mean(axis=0), patch.std(axis=0, ddof=1) / np.sqrt(len(patch))
    print(f"{label}: patch mean {mean}, closed form {want}, standard error {se}, off by {np.abs(mean - want) / se} of it")
    assert (se > 0).all() and (np.abs(mean - want) <= 4 * se).all(), (label, mean, want, se)
    return mean, want, se
