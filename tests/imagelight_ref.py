"""The projection and goniometric lights of pbrt-v3 (src/lights/projection.cpp, src/lights/goniometric.{h,cpp}) restated in
float64 numpy, vectorised over points; the MIPMap they look their image up in (src/core/mipmap.h: the Lanczos resampling
to powers of two, the box-filtered pyramid, the bilinear `triangle` with repeat wrap, `Lookup(st, width)`) is mipmap_ref.py's.

The CPU oracle has neither light and the reference cannot be built here, so this is the independent statement the loader and
the device are held to (test_image_light_scenes.py, test_gpu_image_lights.py). An image is an (h, w, 3) array as ReadImage
returns it: row 0 is the TOP scanline, and neither light flips it."""
import numpy as np

# the MIPMap of src/core/mipmap.h and its resampling helpers live in mipmap_ref.py, with all three wrap modes and EWA
from mipmap_ref import MipMap, _round_up_pow2  # noqa: F401  (_round_up_pow2: test_image_light_scenes.py sizes level 0 with it)

HITHER = float(np.float32(1e-3))
YON = float(np.float32(1e30))


# ---- the lights -------------------------------------------------------------------------------------------------------------
def perspective(fov, n=HITHER, f=YON):
    """Perspective(fov, n, f), src/core/transform.cpp:303-311."""
    persp = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, f / (f - n), -f * n / (f - n)], [0, 0, 1, 0]], np.float64)
    inv_tan = 1.0 / np.tan(np.radians(fov) / 2)
    return np.diag([inv_tan, inv_tan, 1.0, 1.0]) @ persp


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class _ImagePointLight:
    """What the two lights share: pLight, WorldToLight, I (times scale) and the optional map; Sample_Li of both is
    I * <factor>(-wi) / DistanceSquared(pLight, p) with wi = Normalize(pLight - p) and pdf 1."""

    def __init__(self, light_to_world, intensity, image=None):
        self.l2w = np.asarray(light_to_world, np.float64)
        self.w2l = np.linalg.inv(self.l2w)
        self.p_light = self.l2w[:3, 3] / self.l2w[3, 3]
        self.I = np.asarray(intensity, np.float64)
        self.image = None if image is None else np.asarray(image, np.float64)
        self.mip = None if image is None else MipMap(self.image)

    def world_to_light(self, w):
        return np.asarray(w, np.float64) @ self.w2l[:3, :3].T

    def factor(self, w):
        raise NotImplementedError

    def sample_li(self, p):
        """(wi, Li, pdf) at the (n, 3) points p."""
        d = self.p_light[None, :] - np.asarray(p, np.float64)
        r2 = (d * d).sum(1)
        wi = d / np.sqrt(r2)[:, None]
        return wi, self.I[None, :] * self.factor(-wi) / r2[:, None], np.ones(len(d))


class ProjectionLight(_ImagePointLight):
    def __init__(self, light_to_world, intensity, fov=45.0, image=None):
        super().__init__(light_to_world, intensity, image)
        aspect = 1.0 if image is None else self.image.shape[1] / self.image.shape[0]  # projection.cpp:59-65
        self.screen_bounds = np.array([-aspect, -1, aspect, 1] if aspect > 1 else [-1, -1 / aspect, 1, 1 / aspect], np.float64)
        self.fov = float(fov)
        self.proj = perspective(self.fov)
        h = self.screen_bounds[0] ** 2 + self.screen_bounds[1] ** 2 + 1  # :70-74
        self.cos_total_width = 1 / h

    def project(self, w):
        """(wl.z, the projected point (x, y)) of world direction w: what Projection() tests against hither and screenBounds."""
        wl = self.world_to_light(w)
        hom = wl @ self.proj[:, :3].T + self.proj[:, 3][None, :]
        return wl[:, 2], hom[:, :2] / hom[:, 3:4]

    def projection(self, w):
        """ProjectionLight::Projection(w), projection.cpp:88-99."""
        z, p = self.project(w)
        x0, y0, x1, y1 = self.screen_bounds
        with np.errstate(invalid="ignore", divide="ignore"):
            lit = (z >= HITHER) & (p[:, 0] >= x0) & (p[:, 0] <= x1) & (p[:, 1] >= y0) & (p[:, 1] <= y1)
        out = np.zeros((len(z), 3))
        if self.mip is None:
            out[lit] = 1.0
        else:
            st = (p[lit] - np.array([x0, y0])) / np.array([x1 - x0, y1 - y0])  # Bounds2f::Offset
            out[lit] = self.mip.lookup(st)
        return out

    factor = projection

    def power(self):
        """ProjectionLight::Power, projection.cpp:101-107."""
        centre = np.ones(3) if self.mip is None else self.mip.lookup(np.array([0.5, 0.5]), 0.5)
        return centre * self.I * 2 * np.pi * (1 - self.cos_total_width)


class GoniometricLight(_ImagePointLight):
    def angles(self, w):
        """(theta, phi) of Scale(w): of Normalize(WorldToLight(w)) with y and z swapped (goniometric.h:70-73)."""
        wp = _normalize(self.world_to_light(w))[:, [0, 2, 1]]
        theta = np.arccos(np.clip(wp[:, 2], -1, 1))
        phi = np.arctan2(wp[:, 1], wp[:, 0])
        return theta, np.where(phi < 0, phi + 2 * np.pi, phi)

    def scale(self, w):
        """GonioPhotometricLight::Scale(w), goniometric.h:69-77."""
        if self.mip is None:
            return np.ones((len(w), 3))
        theta, phi = self.angles(w)
        return self.mip.lookup(np.stack([phi / (2 * np.pi), theta / np.pi], 1))

    factor = scale

    def power(self):
        """GonioPhotometricLight::Power, goniometric.cpp:55-59."""
        centre = np.ones(3) if self.mip is None else self.mip.lookup(np.array([0.5, 0.5]), 0.5)
        return 4 * np.pi * self.I * centre


def luminance(rgb):
    """RGBSpectrum::y()."""
    rgb = np.asarray(rgb, np.float64)
    return 0.212671 * rgb[..., 0] + 0.715160 * rgb[..., 1] + 0.072169 * rgb[..., 2]
