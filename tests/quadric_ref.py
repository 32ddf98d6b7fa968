"""Disks and cylinders restated in float64 numpy (shapes/disk.cpp, shapes/cylinder.cpp of pbrt-v3), and small .pbrt scenes
built around them, for test_quadric_scenes.py and test_gpu_quadrics.py. The CPU oracle has no quadrics, so these are the
independent statement the device is held to."""
import numpy as np

HEADER = """LookAt {eye} {look} {up}
Camera "perspective" "float fov" [{fov}]
Film "image" "integer xresolution" [{w}] "integer yresolution" [{h}] "string filename" "quadrics.exr"
Sampler "halton" "integer pixelsamples" [{spp}]
Integrator "{integrator}" "integer maxdepth" [{depth}]
WorldBegin
"""


def scene_text(body, w=32, h=32, spp=4, depth=5, fov=60, eye="0 0 -5", look="0 0 0", up="0 1 0", integrator="path"):
    return HEADER.format(eye=eye, look=look, up=up, fov=fov, w=w, h=h, spp=spp, depth=depth, integrator=integrator) + body + "\nWorldEnd\n"


def write_scene(tmp_path, body, name="scene.pbrt", **kw):
    p = tmp_path / name
    p.write_text(scene_text(body, **kw))
    return str(p)


# ---- transforms (row-major 4x4, as iile_quadric::o2w) ----------------------------------------------------------------------
def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def scale(x, y, z):
    return np.diag([x, y, z, 1.0])


def rotate(deg, axis):
    """Rotate(theta, axis), transform.cpp:117-143."""
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    s, c = np.sin(np.radians(deg)), np.cos(np.radians(deg))
    m = np.eye(4)
    m[0, :3] = (a[0] * a[0] + (1 - a[0] * a[0]) * c, a[0] * a[1] * (1 - c) - a[2] * s, a[0] * a[2] * (1 - c) + a[1] * s)
    m[1, :3] = (a[0] * a[1] * (1 - c) + a[2] * s, a[1] * a[1] + (1 - a[1] * a[1]) * c, a[1] * a[2] * (1 - c) - a[0] * s)
    m[2, :3] = (a[0] * a[2] * (1 - c) - a[1] * s, a[1] * a[2] * (1 - c) + a[0] * s, a[2] * a[2] + (1 - a[2] * a[2]) * c)
    return m


def bound_corners(lo, hi):
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], float)


def world_bound(m, lo, hi):
    """Transform::operator()(Bounds3f), transform.cpp:219-231: the box around the eight transformed corners."""
    c = bound_corners(lo, hi) @ m[:3, :3].T + m[:3, 3]
    return c.min(axis=0), c.max(axis=0)


# ---- shapes ------------------------------------------------------------------------------------------------------------------
class Disk:
    def __init__(self, m, height=0.0, radius=1.0, inner=0.0, phimax=360.0):
        self.m, self.inv = np.asarray(m, float), np.linalg.inv(np.asarray(m, float))
        self.height, self.radius, self.inner, self.phimax = height, radius, inner, np.radians(np.clip(phimax, 0, 360))

    def params(self, grow):
        """The same disk grown (grow > 0) or shrunk at every edge by `grow` (object units)."""
        d = Disk(self.m, self.height, self.radius + grow, max(self.inner - grow, 0.0), 0.0)
        d.phimax = self.phimax + grow / max(self.radius, 1e-9) if self.phimax < 2 * np.pi else self.phimax
        return d

    def intersect(self, o, d, tmax):
        """t of Disk::Intersect per ray (inf = miss), the object-space hit point (disk.cpp:48-92) and |cos| between the ray and
        the surface normal there."""
        oo, dd = o @ self.inv[:3, :3].T + self.inv[:3, 3], d @ self.inv[:3, :3].T
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (self.height - oo[:, 2]) / dd[:, 2]
        p = oo + dd * t[:, None]
        r2 = p[:, 0] ** 2 + p[:, 1] ** 2
        phi = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2 * np.pi)
        ok = (dd[:, 2] != 0) & (t > 0) & (t < tmax) & (r2 <= self.radius ** 2) & (r2 >= self.inner ** 2) & (phi <= self.phimax)
        p[:, 2] = self.height
        return np.where(ok, t, np.inf), p, np.abs(dd[:, 2]) / np.linalg.norm(dd, axis=1)

    def object_bound(self):
        return (-self.radius, -self.radius, self.height), (self.radius, self.radius, self.height)


class Cylinder:
    def __init__(self, m, radius=1.0, zmin=-1.0, zmax=1.0, phimax=360.0):
        self.m, self.inv = np.asarray(m, float), np.linalg.inv(np.asarray(m, float))
        self.radius, self.zmin, self.zmax = radius, min(zmin, zmax), max(zmin, zmax)
        self.phimax = np.radians(np.clip(phimax, 0, 360))

    def params(self, grow):
        c = Cylinder(self.m, self.radius + grow, self.zmin - grow, self.zmax + grow, 0.0)
        c.phimax = self.phimax + grow / max(self.radius, 1e-9) if self.phimax < 2 * np.pi else self.phimax
        return c

    def intersect(self, o, d, tmax):
        """t of Cylinder::Intersect per ray (inf = miss), the object-space hit point (cylinder.cpp:48-103) and |cos| between the
        ray and the surface normal there."""
        oo, dd = o @ self.inv[:3, :3].T + self.inv[:3, 3], d @ self.inv[:3, :3].T
        a = dd[:, 0] ** 2 + dd[:, 1] ** 2
        b = 2 * (dd[:, 0] * oo[:, 0] + dd[:, 1] * oo[:, 1])
        c = oo[:, 0] ** 2 + oo[:, 1] ** 2 - self.radius ** 2
        disc = b * b - 4 * a * c
        sq = np.sqrt(np.maximum(disc, 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(b < 0, -0.5 * (b - sq), -0.5 * (b + sq))
            t0, t1 = q / a, c / q
        t0, t1 = np.minimum(t0, t1), np.maximum(t0, t1)
        valid = (disc >= 0) & (a > 0)

        def at(t):
            p = oo + dd * t[:, None]
            s = self.radius / np.hypot(p[:, 0], p[:, 1])
            p[:, 0] *= s
            p[:, 1] *= s
            phi = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2 * np.pi)
            inside = (p[:, 2] >= self.zmin) & (p[:, 2] <= self.zmax) & (phi <= self.phimax)
            return p, inside

        with np.errstate(invalid="ignore"):
            p0, in0 = at(t0)
            p1, in1 = at(t1)
        use0 = valid & (t0 > 0) & (t0 <= tmax) & in0
        use1 = valid & ~use0 & (t1 > 0) & (t1 <= tmax) & in1
        t = np.where(use0, t0, np.where(use1, t1, np.inf))
        p = np.where(use0[:, None], p0, p1)
        with np.errstate(invalid="ignore"):
            cos = np.abs(dd[:, 0] * p[:, 0] + dd[:, 1] * p[:, 1]) / (np.linalg.norm(dd, axis=1) * self.radius)
        return t, p, cos

    def object_bound(self):
        return (-self.radius, -self.radius, self.zmin), (self.radius, self.radius, self.zmax)


GRAZING = 0.25  # |cos| between ray and normal below which t is not compared: the float32 roots lose digits as the ray turns tangent


def decided(shape, o, d, tmax, eps):
    """(t, certain, cos): the restated hit, whether the shape grown and shrunk by eps at every edge agrees on hit or miss (rays
    near an edge, or grazing a cylinder, are left undecided), and |cos| between the ray and the normal at the hit."""
    t, _, cos = shape.intersect(o, d, tmax)
    ti, _, _ = shape.params(-eps).intersect(o, d, tmax)
    to, _, _ = shape.params(eps).intersect(o, d, tmax)
    return t, np.isfinite(ti) == np.isfinite(to), cos


def matrix_text(m):
    """A pbrt "Transform" directive for row-major m (pbrt reads the transpose, column-major)."""
    return "Transform [" + " ".join(f"{v:.9g}" for v in np.asarray(m, float).T.reshape(-1)) + "]"


def disk_irradiance_factor(h, rho, r):
    """Irradiance / (pi L) at a point on a plane a height h below a facing disk of radius r, rho off its axis:
    1/2 [1 - (h^2 + rho^2 - r^2) / sqrt((h^2 + rho^2 + r^2)^2 - 4 r^2 rho^2)]."""
    a = h * h + rho * rho
    return 0.5 * (1 - (a - r * r) / np.sqrt((a + r * r) ** 2 - 4 * r * r * rho * rho))
