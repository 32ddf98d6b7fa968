"""Scenes of more spheres, materials and quadrics than the device once took (8, 64 and 1 024), as .pbrt text, for
test_many_shapes_scenes.py (no GPU) and test_gpu_many_shapes.py. Every sphere has a `Material` directive of its own with a
parameter no other material has, so a wrong material index changes the film and is read back from the host's table."""
import numpy as np

import quadric_ref as Q

KINDS = ("matte", "plastic", "mirror", "glass", "metal", "uber", "substrate")  # the cycle of the spheres' materials
RADIUS = 0.3


def header(w=32, h=32, spp=4, depth=5, fov=55, eye="0 -5.6 2.2", look="0 0 1.9", up="0 0 1", integrator="path", name="shapes.exr"):
    return (f'LookAt {eye}  {look}  {up}\nCamera "perspective" "float fov" [{fov}]\n'
            f'Film "image" "integer xresolution" [{w}] "integer yresolution" [{h}] "string filename" "{name}"\nPixelFilter "box"\n'
            f'Sampler "halton" "integer pixelsamples" [{spp}]\nIntegrator "{integrator}" "integer maxdepth" [{depth}]\nWorldBegin\n')


def write(tmp_path, body, name="shapes.pbrt", **kw):
    p = tmp_path / name
    p.write_text(header(**kw) + body + "WorldEnd\n")
    return str(p)


def mesh(points, indices):
    pts = " ".join(f"{np.float32(v):.9g}" for v in np.ravel(points))
    return f'Shape "trianglemesh" "integer indices" [{" ".join(str(int(i)) for i in np.ravel(indices))}] "point P" [{pts}]\n'


def quad(corners):
    return mesh(corners, [0, 1, 2, 0, 2, 3])


def tint(j):
    """Material j's own value in (0.2, 0.8), exact in float32 and different for every j < 600."""
    return np.float32((128 + j) / 1024.0)


def material(j):
    """-> (the `Material` line of sphere j, the iile_material field that holds its own value, that value): Kd where the
    type has one, else the type's reflectance (mirror, glass: Kr; metal: k)."""
    kind, t = KINDS[j % len(KINDS)], tint(j)
    v = f"{t:.9g}"
    if kind == "matte":
        return f'Material "matte" "rgb Kd" [{v} 0.5 0.4]\n', "kd", t
    if kind == "plastic":
        return f'Material "plastic" "rgb Kd" [{v} 0.3 0.5] "rgb Ks" [0.3 0.3 0.3] "float roughness" [0.2]\n', "kd", t
    if kind == "mirror":
        return f'Material "mirror" "rgb Kr" [{v} 0.8 0.8]\n', "kr", t
    if kind == "glass":
        return f'Material "glass" "rgb Kr" [{v} 0.9 0.9] "rgb Kt" [0.9 0.9 0.9] "float index" [1.4]\n', "kr", t
    if kind == "metal":
        return f'Material "metal" "rgb eta" [0.2 0.9 1.1] "rgb k" [{v} 2.4 2.1] "float roughness" [0.1]\n', "cond_k", t
    if kind == "uber":
        return f'Material "uber" "rgb Kd" [{v} 0.4 0.3] "rgb Ks" [0.2 0.2 0.2] "rgb Kr" [0.1 0.1 0.1] "float roughness" [0.15]\n', "kd", t
    return f'Material "substrate" "rgb Kd" [{v} 0.4 0.4] "rgb Ks" [0.1 0.1 0.1] "float uroughness" [0.1] "float vroughness" [0.2]\n', "kd", t


def grid_centres(a, b, c, count=None, pitch=0.7, z0=0.5):
    """The first `count` cells (all by default) of an a x b x c grid of sphere centres, `pitch` apart, centred over the origin,
    the lowest layer at height z0: x fastest."""
    out = [((i - (a - 1) / 2) * pitch, (j - (b - 1) / 2) * pitch, z0 + k * pitch) for k in range(c) for j in range(b) for i in range(a)]
    return np.array(out[:count if count is not None else len(out)])


def sphere_block(j, centre):
    """Sphere j of a room: its own material; every fifth one partial; every seventh under a rotation, every eleventh under a
    non-uniform scale; spheres 1, 4 and 8 emit."""
    line, _, _ = material(j)
    xf = f"Translate {centre[0]:.9g} {centre[1]:.9g} {centre[2]:.9g}\n"
    if j % 7 == 3:
        xf += f"Rotate {25 + 10 * (j % 5)} 1 0.5 0.25\n"
    if j % 11 == 6:
        xf += "Scale 1 0.7 0.85\n"
    part = ' "float zmax" [0.18] "float phimax" [250]' if j % 5 == 2 else ""
    emit = f'AreaLightSource "diffuse" "rgb L" [{3 + j % 3} 3 2]\n' if j in (1, 4, 8) else ""
    return f'AttributeBegin\n{line}{emit}{xf}Shape "sphere" "float radius" [{RADIUS}]{part}\nAttributeEnd\n'


def room_shell(half, height):
    lo, hi = -half, half
    walls = [[[lo, lo, 0], [hi, lo, 0], [hi, hi, 0], [lo, hi, 0]], [[lo, lo, height], [lo, hi, height], [hi, hi, height], [hi, lo, height]],
             [[lo, hi, 0], [hi, hi, 0], [hi, hi, height], [lo, hi, height]], [[lo, lo, 0], [lo, hi, 0], [lo, hi, height], [lo, lo, height]],
             [[hi, lo, 0], [hi, hi, 0], [hi, hi, height], [hi, lo, height]]]
    return 'Material "matte" "rgb Kd" [0.6 0.6 0.6]\n' + "".join(quad(w) for w in walls)


def sphere_room(a, b, c, count=None, extra_materials=0):
    """A box room open towards the camera, a point light under its ceiling, and a grid of spheres: material 0 is the room's,
    material j + 1 sphere j's; then `extra_materials` more, one small matte triangle on the floor each -> .pbrt body."""
    centres = grid_centres(a, b, c, count)
    half = max(a, b) * 0.35 + 0.8
    height = 0.5 + c * 0.7 + 0.8
    body = f'LightSource "point" "rgb I" [12 12 12] "point from" [0.2 {-half + 0.4:.9g} {height - 0.3:.9g}]\n' + room_shell(half, height)
    body += "".join(sphere_block(j, p) for j, p in enumerate(centres))
    for e in range(extra_materials):
        x = -half + 0.1 + 0.05 * e
        body += f'Material "matte" "rgb Kd" [{tint(len(centres) + e):.9g} 0.2 0.2]\n' + mesh([[x, -half, 0.01], [x + 0.04, -half, 0.01], [x, -half + 0.3, 0.01]], [0, 1, 2])
    return body


def room_file(tmp_path, a, b, c, count=None, name=None, extra_materials=0, **kw):
    n = len(grid_centres(a, b, c, count))
    return write(tmp_path, sphere_room(a, b, c, count, extra_materials), name=name or f"room_{n}_{extra_materials}.pbrt", **kw)


ROOM_72 = (6, 4, 3)  # 72 spheres, 73 materials
ROOM_9 = (3, 3, 1)   # the first count over the common build's
ROOM_8 = (4, 2, 1)   # still the common build


# ---- a cloud of spheres over a triangle floor (ray tests) ----------------------------------------------------------------------------
def cloud(n=256, seed=3):
    """n spheres of radius 0.12 on a jittered 16 x 16 lattice over a floor of two triangles -> (.pbrt body, centres (n, 3))."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n]
    centres = np.float32(np.concatenate([(ij - (side - 1) / 2) * 0.4 + rng.uniform(-0.05, 0.05, (n, 2)), rng.uniform(0.3, 1.2, (n, 1))], axis=1))
    s = side * 0.2 + 1
    body = 'Material "matte"\n' + quad([[-s, -s, 0], [s, -s, 0], [s, s, 0], [-s, s, 0]])
    for p in centres:
        body += f'AttributeBegin\nTranslate {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\nShape "sphere" "float radius" [0.12]\nAttributeEnd\n'
    return body, centres


# ---- spheres, disks and cylinders side by side -----------------------------------------------------------------------------------------
def _xf(rng, centre):
    axis = rng.normal(size=3)
    return Q.translate(*centre) @ Q.rotate(rng.uniform(0, 360), axis)


class Sphere:
    """A full sphere restated in float64: intersect() -> (t or inf, near-tangent?, |cos| between the ray and the normal)."""

    def __init__(self, centre, radius):
        self.c, self.r = np.asarray(centre, np.float64), float(radius)

    def intersect(self, o, d):
        oc = o - self.c
        b = np.sum(oc * d, axis=1)
        disc = b * b - (np.sum(oc * oc, axis=1) - self.r * self.r)
        s = np.sqrt(np.maximum(disc, 0))
        t0, t1 = -b - s, -b + s
        t = np.where(t0 > 0, t0, np.where(t1 > 0, t1, np.inf))
        return np.where(disc >= 0, t, np.inf), np.abs(disc) < 1e-3, s / self.r


def mixed_kinds(n_each=12, seed=5):
    """n_each spheres (radius 0.3), disks and cylinders in turn on a lattice 1.2 apart, no floor -> (.pbrt body, the shapes
    restated, in declaration order: Sphere, quadric_ref.Disk, quadric_ref.Cylinder, ...)."""
    rng = np.random.default_rng(seed)
    n = 3 * n_each
    side = int(np.ceil(np.sqrt(n)))
    cells = [((i - (side - 1) / 2) * 1.2, (j - (side - 1) / 2) * 1.2, 0.0) for j in range(side) for i in range(side)][:n]
    body, shapes = 'Material "matte"\n', []
    for idx, cell in enumerate(cells):
        kind = idx % 3
        centre = np.float32(np.array(cell) + np.array([0, 0, rng.uniform(-0.3, 0.3)])).astype(np.float64)
        if kind == 0:
            body += f'AttributeBegin\nTranslate {centre[0]:.9g} {centre[1]:.9g} {centre[2]:.9g}\nShape "sphere" "float radius" [0.3]\nAttributeEnd\n'
            shapes.append(Sphere(centre, np.float32(0.3)))
            continue
        m = _xf(rng, centre)
        m = np.array([[float(f"{v:.9g}") for v in row] for row in m])
        if kind == 1:
            inner, phimax = (0.1, 300.0) if idx % 2 else (0.0, 360.0)
            body += (f'AttributeBegin\n{Q.matrix_text(m)}\nShape "disk" "float radius" [0.4] "float innerradius" [{inner}] '
                     f'"float phimax" [{phimax}]\nAttributeEnd\n')
            shapes.append(Q.Disk(m, 0.0, 0.4, inner, phimax))
        else:
            phimax = 270.0 if idx % 2 else 360.0
            body += (f'AttributeBegin\n{Q.matrix_text(m)}\nShape "cylinder" "float radius" [0.25] "float zmin" [-0.3] "float zmax" [0.3] '
                     f'"float phimax" [{phimax}]\nAttributeEnd\n')
            shapes.append(Q.Cylinder(m, 0.25, -0.3, 0.3, phimax))
    return body, shapes


def nearest_of(shapes, o, d, eps=1e-4):
    """What the restatement says of float32 rays (o, d) against `shapes`: (index of the nearest shape hit, its t or inf, decided?,
    steep?). A ray is undecided within eps of an edge of any shape (quadric_ref.decided), near-tangent to a sphere, or where its two
    nearest hits lie within 1e-4 of each other; steep: |cos| at the nearest hit above quadric_ref.GRAZING (t is compared there)."""
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    inf = np.full(len(o64), np.inf)
    ts, coss, certain = [], [], np.ones(len(o64), bool)
    for s in shapes:
        if isinstance(s, Sphere):
            t, edge, cos = s.intersect(o64, d64)
            certain &= ~edge
        else:
            t, c, cos = Q.decided(s, o64, d64, inf, eps)
            certain &= c
        ts.append(t)
        coss.append(cos)
    ts = np.stack(ts)
    two = np.partition(ts, 1, axis=0)[:2] if len(shapes) > 1 else np.stack([ts[0], inf])
    with np.errstate(invalid="ignore"):  # (inf - inf where a ray hits nothing)
        certain &= ~(np.isfinite(two[0]) & (two[1] - two[0] < 1e-4 * np.maximum(two[0], 1)))
    nearest = np.argmin(ts, axis=0)
    with np.errstate(invalid="ignore"):
        steep = np.take_along_axis(np.stack(coss), nearest[None], axis=0)[0] > Q.GRAZING
    return nearest, two[0], certain, steep


def disk_field(n=1025, seed=6):
    """n disks of radius 0.1 on a lattice 33 wide and 0.3 apart, each tilted by up to 35 degrees -> (.pbrt body, [Disk...])."""
    rng = np.random.default_rng(seed)
    side = 33
    body, disks = 'Material "matte"\n', []
    for idx in range(n):
        i, j = idx % side, idx // side
        m = Q.translate((i - 16) * 0.3, (j - 16) * 0.3, 0.0) @ Q.rotate(rng.uniform(-35, 35), (rng.uniform(-1, 1), rng.uniform(-1, 1), 0.01))
        m = np.array([[float(f"{v:.9g}") for v in row] for row in m])
        body += f'AttributeBegin\n{Q.matrix_text(m)}\nShape "disk" "float radius" [0.1]\nAttributeEnd\n'
        disks.append(Q.Disk(m, 0.0, 0.1))
    return body, disks


def aimed_rays(targets, rng, spread, height=6.0):
    """One ray per target from a point `height` above it (jittered sideways) towards the target offset by up to `spread`: float32
    (o, d), d normalised."""
    targets = np.asarray(targets, np.float64)
    n = len(targets)
    o = targets + np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), np.full((n, 1), height)], axis=1)
    aim = targets + rng.uniform(-spread, spread, (n, 3))
    d = aim - o
    return o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
