"""The environment camera of pbrt-v3 restated in float64 numpy, vectorised over film points: EnvironmentCamera::GenerateRay
(src/cameras/environment.cpp:43-56) with Transform::operator()(Ray) (src/core/transform.h:251-264), and the ray differentials
the camera inherits from its base class, Camera::GenerateRayDifferential (src/core/camera.cpp:60-96), with the render loop's
ScaleDifferentials(1 / sqrt(spp)).

The CPU oracle knows only the perspective camera, so this is the independent statement the loader and the device are held to
(test_environment_camera_scenes.py, test_gpu_environment_camera.py). Transforms are 4 x 4 arrays, m[r][c]."""
import numpy as np

GAMMA3 = 3 * 2.0 ** -24 / (1 - 3 * 2.0 ** -24)  # gamma(3) of core/pbrt.h: the error bound of a transformed point
EPS = float(np.float32(0.05))                   # the film shift of Camera::GenerateRayDifferential


# ---- the transforms a scene file states before `Camera` (core/transform.cpp) ---------------------------------------------------
def look_at(eye, look, up):
    """LookAt's camera-to-world matrix (transform.cpp:262-301); the directive multiplies the CTM by its inverse."""
    eye, look, up = (np.asarray(v, np.float64) for v in (eye, look, up))
    d = (look - eye) / np.linalg.norm(look - eye)
    right = np.cross(up / np.linalg.norm(up), d)
    right /= np.linalg.norm(right)
    new_up = np.cross(d, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, new_up, d, eye
    return m


def rotate(deg, axis):
    """Rotate(theta, axis), transform.cpp:223-260."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    s, c = np.sin(np.radians(deg)), np.cos(np.radians(deg))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = c * np.eye(3) + s * k + (1 - c) * np.outer(a, a)
    return m


def scale(x, y, z):
    return np.diag([float(x), float(y), float(z), 1.0])


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = x, y, z
    return m


SWAP_YZ = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)  # `Transform [1 0 0 0  0 0 1 0  0 1 0 0  0 0 0 1]`


def camera_to_world(*ctm_factors):
    """CameraToWorld = Inverse(CTM) (api.cpp:1118-1123) of the directives before `Camera`, each given as the matrix the directive
    multiplies the CTM by, in file order (for LookAt that is the inverse of look_at())."""
    ctm = np.eye(4)
    for m in ctm_factors:
        ctm = ctm @ np.asarray(m, np.float64)
    return np.linalg.inv(ctm)


# ---- the camera ------------------------------------------------------------------------------------------------------------------
def direction(pfilm, xres, yres):
    """The camera-space direction of environment.cpp:47-50 (not normalised there; its length is 1 up to rounding)."""
    pfilm = np.asarray(pfilm, np.float64)
    theta = np.pi * pfilm[:, 1] / yres
    phi = 2 * np.pi * pfilm[:, 0] / xres
    return np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], 1)


def generate_ray(c2w, pfilm, xres, yres):
    """(o, d) in world space: Ray((0, 0, 0), dir) through CameraToWorld. Transform::operator()(Ray) moves the origin along d by
    the error bound of the transformed point, dt = Dot(Abs(d), oError) / LengthSquared(d), oError = gamma(3) * |translation| for
    the point (0, 0, 0) (transform.h:233-264)."""
    c2w = np.asarray(c2w, np.float64)
    d = direction(pfilm, xres, yres) @ c2w[:3, :3].T
    o = np.broadcast_to(c2w[:3, 3], d.shape).copy()
    o_err = GAMMA3 * np.abs(c2w[:3, 3])
    len2 = (d * d).sum(1)
    dt = np.where(len2 > 0, (np.abs(d) @ o_err) / np.where(len2 > 0, len2, 1), 0.0)
    return o + d * dt[:, None], d


def differentials(c2w, pfilm, xres, yres, spp=1):
    """(o, d, rx_o, rx_d, ry_o, ry_d): the rays through pFilm + (0.05, 0) and pFilm + (0, 0.05), differenced (camera.cpp:65-91;
    every weight is 1, so the -0.05 retry never runs), then ScaleDifferentials(1 / sqrt(spp)) (integrator.cpp:284-285,
    geometry.h:908-913)."""
    pfilm = np.asarray(pfilm, np.float64)
    o, d = generate_ray(c2w, pfilm, xres, yres)
    xo, xd = generate_ray(c2w, pfilm + np.array([EPS, 0.0]), xres, yres)
    yo, yd = generate_ray(c2w, pfilm + np.array([0.0, EPS]), xres, yres)
    s = 1 / np.sqrt(float(np.float32(spp)))
    rxo, rxd = o + (xo - o) / EPS, d + (xd - d) / EPS
    ryo, ryd = o + (yo - o) / EPS, d + (yd - d) / EPS
    return o, d, o + (rxo - o) * s, d + (rxd - d) * s, o + (ryo - o) * s, d + (ryd - d) * s
