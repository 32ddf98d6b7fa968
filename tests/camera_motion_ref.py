"""A moving camera, restated in numpy from the reference's text: AnimatedTransform's constructor, Decompose and Interpolate
(src/core/transform.cpp:396-411, 1103-1169), Quaternion(Transform), ToTransform and Slerp (src/core/quaternion.cpp:41-104), and
GenerateRay of the perspective and the environment camera (src/cameras/perspective.cpp:100-122, environment.cpp:43-56) with
Transform::operator()(Ray) (src/core/transform.h:251-264).

Every function takes the float type `ft` it computes in. np.float64 is the truth the tests hold the host and the device to;
np.float32 is the same operation sequence in the precision the product computes in, whose distance from the truth is the
measured rounding band of the tests (test_camera_motion_scenes.py, test_gpu_camera_motion.py). Nothing here is taken from the
device or host code."""
import numpy as np

GAMMA3 = 3 * 2.0 ** -24 / (1 - 3 * 2.0 ** -24)  # gamma(3), core/pbrt.h: the error bound of a transformed point


# ---- the transforms a scene file spells (core/transform.cpp:146-242), float64: they make the tests' inputs ----
def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m


def scale(x, y, z):
    return np.diag([float(x), float(y), float(z), 1.0])


def rotate(deg, axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    s, c = np.sin(np.radians(deg)), np.cos(np.radians(deg))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = c * np.eye(3) + s * k + (1 - c) * np.outer(a, a)
    return m


def look_at(eye, look, up):
    eye, look, up = (np.asarray(v, np.float64) for v in (eye, look, up))
    d = (look - eye) / np.linalg.norm(look - eye)
    right = np.cross(up / np.linalg.norm(up), d)
    right /= np.linalg.norm(right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(d, right), d, eye
    return np.linalg.inv(c2w)


def camera_to_world(*ctm_factors):
    """Inverse(CTM), the CTM being the product of the file's directives in order (api.cpp:934-995, 1118-1123)."""
    ctm = np.eye(4)
    for f in ctm_factors:
        ctm = ctm @ f
    return np.linalg.inv(ctm)


# ---- AnimatedTransform ----
def quaternion_of(m, ft):
    """Quaternion(const Transform &): {x, y, z, w}."""
    m = np.asarray(m, ft)
    one, half, two = ft(1), ft(0.5), ft(2)
    q = np.zeros(4, ft)
    trace = m[0, 0] + m[1, 1] + m[2, 2]
    if trace > 0:
        s = np.sqrt(trace + one)
        q[3] = s / two
        s = half / s
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s
    else:
        nxt = [1, 2, 0]
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = nxt[i]
        k = nxt[j]
        s = np.sqrt((m[i, i] - (m[j, j] + m[k, k])) + one)
        q[i] = s * half
        if s != 0:
            s = half / s
        q[3] = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
    return q


def decompose(m, ft):
    """AnimatedTransform::Decompose: (T, R as {x, y, z, w}, S 4 x 4, the rotation matrix the iteration ended on)."""
    m = np.asarray(m, ft)
    T = m[:3, 3].copy()
    M = m.copy()
    M[:3, 3] = 0
    M[3, :3] = 0
    M[3, 3] = 1
    R = M.copy()
    count = 0
    while True:
        Rit = np.linalg.inv(R.T).astype(ft)
        Rnext = (ft(0.5) * (R + Rit)).astype(ft)
        norm = np.abs(R[:3, :3] - Rnext[:3, :3]).sum(1).max()
        R = Rnext
        count += 1
        if not (count < 100 and norm > 1e-4):
            break
    S = (np.linalg.inv(R).astype(ft) @ M).astype(ft)
    return T, quaternion_of(R, ft), S, R


def polar_truth(m):
    """The polar decomposition itself, by SVD in float64: M = R S with R the nearest rotation (det M > 0 for every camera here)."""
    m = np.asarray(m, np.float64)
    u, _, vt = np.linalg.svd(m[:3, :3])
    R = np.eye(4)
    R[:3, :3] = u @ vt
    M = m.copy()
    M[:3, 3] = 0
    return m[:3, 3].copy(), quaternion_of(R, np.float64), np.linalg.inv(R) @ M


class Animated:
    """AnimatedTransform(start, start_time, end, end_time) of two camera-to-world matrices."""

    def __init__(self, start, end, start_time=0.0, end_time=1.0, ft=np.float64):
        self.ft = ft
        self.m = [np.asarray(start, ft), np.asarray(end, ft)]
        self.t0, self.t1 = ft(start_time), ft(end_time)
        self.animated = not np.array_equal(self.m[0], self.m[1])
        if not self.animated:
            return
        d = [decompose(x, ft) for x in self.m]
        self.T = [d[0][0], d[1][0]]
        self.R = [d[0][1], d[1][1]]
        self.S = [d[0][2], d[1][2]]
        if qdot(self.R[0], self.R[1]) < 0:
            self.R[1] = -self.R[1]
        self.has_rotation = bool(qdot(self.R[0], self.R[1]) < ft(0.9995))

    def interpolate(self, time):
        """AnimatedTransform::Interpolate: the matrix of the transform at `time`."""
        ft = self.ft
        time = ft(time)
        if not self.animated or time <= self.t0:
            return self.m[0]
        if time >= self.t1:
            return self.m[1]
        dt = (time - self.t0) / (self.t1 - self.t0)
        one = ft(1)
        trans = (one - dt) * self.T[0] + dt * self.T[1]
        q = slerp(dt, self.R[0], self.R[1], ft)
        sc = np.eye(4, dtype=ft)
        sc[:3, :3] = (one - dt) * self.S[0][:3, :3] + dt * self.S[1][:3, :3]
        tm = np.eye(4, dtype=ft)
        tm[:3, 3] = trans
        return ((tm @ quaternion_matrix(q, ft)).astype(ft) @ sc).astype(ft)


def qdot(a, b):
    return (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) + a[3] * b[3]


def qnormalize(q, ft):
    return (q / np.sqrt(qdot(q, q))).astype(ft)


def slerp(t, q1, q2, ft):
    cos_theta = qdot(q1, q2)
    one = ft(1)
    if cos_theta > ft(0.9995):
        return qnormalize((one - t) * q1 + t * q2, ft)
    theta = np.arccos(np.clip(cos_theta, -one, one))
    thetap = theta * t
    qperp = qnormalize(q2 - q1 * cos_theta, ft)
    return (q1 * np.cos(thetap) + qperp * np.sin(thetap)).astype(ft)


def quaternion_matrix(q, ft):
    """Quaternion::ToTransform().m — the transpose of the matrix the method writes out."""
    x, y, z, w = (ft(v) for v in q)
    one, two = ft(1), ft(2)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, x * w, y * w, z * w
    m = np.eye(4, dtype=ft)
    m[0, :3] = [one - two * (yy + zz), two * (xy - wz), two * (xz + wy)]
    m[1, :3] = [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)]
    m[2, :3] = [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]
    return m


# ---- the two cameras ----
def concentric_sample_disk(u, ft):
    u = np.asarray(u, ft)
    o = ft(2) * u - ft(1)
    ox, oy = o[:, 0], o[:, 1]
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, ox, oy)
        theta = np.where(first, ft(np.pi / 4) * (oy / ox), ft(np.pi / 2) - ft(np.pi / 4) * (ox / oy))
    zero = (ox == 0) & (oy == 0)
    theta = np.where(zero, ft(0), theta).astype(ft)
    r = np.where(zero, ft(0), r).astype(ft)
    return np.stack([r * np.cos(theta), r * np.sin(theta)], 1).astype(ft)


def _normalize(v):
    return v / np.sqrt((v * v).sum(1))[:, None]


def camera_space_ray(kind, pfilm, plens, raster_to_camera, lens_radius, focal_distance, xres, yres, ft):
    """(o, d) in camera space. kind: "perspective" or "environment"."""
    pfilm = np.asarray(pfilm, ft)
    n = len(pfilm)
    o = np.zeros((n, 3), ft)
    if kind == "environment":
        theta = ft(np.pi) * pfilm[:, 1] / ft(yres)
        phi = ft(2) * ft(np.pi) * pfilm[:, 0] / ft(xres)
        return o, np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], 1).astype(ft)
    r2c = np.asarray(raster_to_camera, ft).reshape(4, 4)
    p = np.concatenate([pfilm, np.zeros((n, 1), ft), np.ones((n, 1), ft)], 1) @ r2c.T
    pcam = p[:, :3] / p[:, 3:4]
    d = _normalize(pcam).astype(ft)
    if lens_radius > 0:
        plens_c = ft(lens_radius) * concentric_sample_disk(plens, ft)
        t = ft(focal_distance) / d[:, 2]
        pfocus = d * t[:, None]
        o = np.concatenate([plens_c, np.zeros((n, 1), ft)], 1).astype(ft)
        d = _normalize(pfocus - o).astype(ft)
    return o, d


def transform_ray(m, o, d, ft):
    """Transform::operator()(Ray): the origin with its error bound, moved along d by Dot(Abs(d), oError) / LengthSquared(d)."""
    m = np.asarray(m, ft)
    A, t = m[:3, :3], m[:3, 3]
    ow = o @ A.T + t
    o_err = ft(GAMMA3) * (np.abs(o[:, None, :] * A[None, :, :]).sum(2) + np.abs(t))
    dw = (d @ A.T).astype(ft)
    len2 = (dw * dw).sum(1)
    dt = np.where(len2 > 0, (np.abs(dw) * o_err).sum(1) / np.where(len2 > 0, len2, 1), 0)
    return (ow + dw * dt[:, None]).astype(ft), dw


def generate_ray(anim, time, kind, pfilm, plens=None, raster_to_camera=None, lens_radius=0.0, focal_distance=0.0, xres=1, yres=1):
    """GenerateRay at ray time `time` (what Lerp(sample.time, shutterOpen, shutterClose) gave): (o, d) in world space."""
    ft = anim.ft
    o, d = camera_space_ray(kind, pfilm, plens, raster_to_camera, lens_radius, focal_distance, xres, yres, ft)
    return transform_ray(anim.interpolate(time), o, d, ft)
