"""pbrt-v3's image-texture path restated in float64 numpy, from the pixel to the texel: MIPMap (src/core/mipmap.h: the Lanczos
resampling to powers of two under the three wrap modes, the box pyramid, Texel, triangle, Lookup(st, width), EWA and
Lookup(st, dst0, dst1)), ImageTexture::Evaluate over UVMapping2D (src/textures/imagemap.h, src/core/texture.cpp) and, for a
planar uv-mapped quad, the perspective camera's GenerateRayDifferential with ScaleDifferentials and
SurfaceInteraction::ComputeDifferentials (src/cameras/perspective.cpp, src/core/camera.cpp, src/core/interaction.cpp).

Numpy only: no oracle, no host library, no device. It is written from the reference's sources, so that the oracle's tex_*
functions and the device's dtex.h, which restate each other operation for operation, are both held to a third statement.

An image is an (h, w, 3) array whose row index is t and whose column index is s; which scanline is row 0 is the caller's
business (ImageTexture flips the file's rows, the image lights do not).

EWA reads its Gaussian at int(r2 * 128): the one place where a float32 evaluation may legitimately land on another value than
this float64 one. `MipMap.lookup_diff` and `evaluate` therefore return (value, slack): slack bounds what the float32 rounding
of r2 can move the value by through that step (see MipMap._ewa). Everything else is continuous in the inputs, with one
exception of measure zero: under `black` wrap the trilinear Lookup jumps from `triangle` on the 1 x 1 level to its texel where
the level n - 1 + log2(2 * width) rounds up to n - 1 in float32 only (2 * width within about 1e-7 below 1), which random
differentials do not hit."""
import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32
WRAPS = {0: "repeat", 1: "black", 2: "clamp", "repeat": "repeat", "black": "black", "clamp": "clamp"}  # IILE_WRAP_* or the name
LUT_SIZE = 128


def ulp32(x):
    """The spacing of float32 at |x|."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---- the constructor ----------------------------------------------------------------------------------------------------------
def _round_up_pow2(v):
    return 1 << (int(v) - 1).bit_length()


def _lanczos(x, tau=2.0):
    """Lanczos(x, tau), src/core/texture.cpp:254-262."""
    x = np.abs(x)
    xs = np.where(x < 1e-5, 1.0, x) * np.pi
    val = np.sin(xs * tau) / (xs * tau) * (np.sin(xs) / xs)
    return np.where(x < 1e-5, 1.0, np.where(x > 1.0, 0.0, val))


def _resample_weights(old, new):
    """MIPMap::resampleWeights (mipmap.h:78-97): (first texel, four normalised weights) per new texel."""
    center = (np.arange(new) + 0.5) * old / new
    first = np.floor(center - 2.0 + 0.5).astype(int)
    pos = first[:, None] + np.arange(4)[None, :] + 0.5
    w = _lanczos((pos - center[:, None]) / 2.0)
    return first, w / w.sum(1, keepdims=True)


def _wrap_index(i, n, wrap):
    """(index into [0, n), weight 1 or 0) of tap i under the wrap mode: repeat wraps, clamp clamps, black drops."""
    if wrap == "repeat":
        return i % n, np.ones(i.shape)
    if wrap == "clamp":
        return np.clip(i, 0, n - 1), np.ones(i.shape)
    return np.clip(i, 0, n - 1), ((i >= 0) & (i < n)).astype(np.float64)


def resample_pow2(img, wrap="repeat"):
    """The constructor's resampling of an image whose sides are not both powers of two (mipmap.h:126-183): the s-pass, then
    the t-pass, each tap indexed through the wrap mode (a dropped tap of `black` is not renormalised), then the clamp to [0, inf)."""
    wrap = WRAPS[wrap]
    img = np.asarray(img, np.float64)
    h, w, _ = img.shape
    wp, hp = _round_up_pow2(w), _round_up_pow2(h)
    if (wp, hp) == (w, h):
        return img
    first, wt = _resample_weights(w, wp)
    cols, keep = _wrap_index(first[:, None] + np.arange(4)[None, :], w, wrap)
    tmp = (img[:, cols, :] * (wt * keep)[None, :, :, None]).sum(2)  # (h, wp, 3)
    first, wt = _resample_weights(h, hp)
    rows, keep = _wrap_index(first[:, None] + np.arange(4)[None, :], h, wrap)
    out = (tmp[rows, :, :] * (wt * keep)[:, :, None, None]).sum(1)  # (hp, wp, 3)
    return np.maximum(out, 0.0)


def weight_lut():
    """MIPMap::weightLut (mipmap.h:209-216): exp(-2 r2) - exp(-2) at r2 = i / 127."""
    r2 = np.arange(LUT_SIZE) / (LUT_SIZE - 1.0)
    return np.exp(-2.0 * r2) - np.exp(-2.0)


class MipMap:
    """MIPMap<RGBSpectrum>(resolution, texels, doTrilinear, maxAnisotropy, wrapMode); the defaults are the reference's."""

    def __init__(self, img, wrap="repeat", trilinear=False, max_aniso=8.0):
        self.wrap = WRAPS[wrap]
        self.trilinear = bool(trilinear)
        self.max_aniso = float(max_aniso)
        self.lut = weight_lut()
        level = resample_pow2(img, self.wrap)
        self.levels = [level]
        while max(level.shape[:2]) > 1:  # mipmap.h:185-207; a side that has reached 1 stays 1
            h, w, _ = level.shape
            nh, nw = max(1, h // 2), max(1, w // 2)
            t, s = np.arange(nh)[:, None], np.arange(nw)[None, :]
            k = len(self.levels) - 1
            level = 0.25 * (self.texel(k, 2 * s, 2 * t) + self.texel(k, 2 * s + 1, 2 * t) + self.texel(k, 2 * s, 2 * t + 1) +
                            self.texel(k, 2 * s + 1, 2 * t + 1))
            self.levels.append(level)

    def texel(self, level, s, t):
        """MIPMap::Texel (mipmap.h:220-242)."""
        a = self.levels[level]
        h, w, _ = a.shape
        s, t = np.broadcast_arrays(np.asarray(s), np.asarray(t))
        if self.wrap == "repeat":
            return a[t % h, s % w]
        if self.wrap == "clamp":
            return a[np.clip(t, 0, h - 1), np.clip(s, 0, w - 1)]
        inside = (s >= 0) & (s < w) & (t >= 0) & (t < h)
        return a[np.clip(t, 0, h - 1), np.clip(s, 0, w - 1)] * inside[..., None]

    def triangle(self, level, st):
        """MIPMap::triangle (mipmap.h:263-274)."""
        level = min(max(level, 0), len(self.levels) - 1)
        h, w, _ = self.levels[level].shape
        s, t = st[..., 0] * w - 0.5, st[..., 1] * h - 0.5
        s0, t0 = np.floor(s).astype(int), np.floor(t).astype(int)
        ds, dt = (s - s0)[..., None], (t - t0)[..., None]
        return ((1 - ds) * (1 - dt) * self.texel(level, s0, t0) + (1 - ds) * dt * self.texel(level, s0, t0 + 1) +
                ds * (1 - dt) * self.texel(level, s0 + 1, t0) + ds * dt * self.texel(level, s0 + 1, t0 + 1))

    def lookup(self, st, width=0.0):
        """MIPMap::Lookup(st, width) (mipmap.h:244-261); width a scalar or one per lookup."""
        st = np.asarray(st, np.float64)
        n = len(self.levels)
        width = np.broadcast_to(np.asarray(width, np.float64), st.shape[:-1])
        level = n - 1 + np.log2(np.maximum(width, 1e-8))
        out = np.empty(st.shape[:-1] + (3,))
        low, top = level < 0, level >= n - 1
        if low.any():
            out[low] = self.triangle(0, st[low])
        if top.any():
            out[top] = self.texel(n - 1, 0, 0)
        il = np.floor(level).astype(int)
        for k in range(n - 1):
            m = ~low & ~top & (il == k)
            if m.any():
                delta = (level[m] - k)[..., None]
                out[m] = (1 - delta) * self.triangle(k, st[m]) + delta * self.triangle(k + 1, st[m])
        return out

    # -- EWA ----------------------------------------------------------------------------------------------------------------
    def _ewa(self, level, st, d0, d1, st_err, d_rel):
        """MIPMap::EWA (mipmap.h:305-353) for the (m, 2) lookups st, d0, d1 at one level -> (value (m, 3), slack (m,)).

        The loop runs over the bounding box of the largest footprint, each lookup masked to its own box.

        slack: r2 = A ss^2 + B ss tt + C tt^2 is evaluated in float32 by the code under test; a texel whose r2 * 128 lies within
        that evaluation's rounding of an integer k may be given lut[k - 1] or lut[k]. The rounding is bounded from the
        operations, with u = 2^-24, first order:
          d = dst * res (1 rounding); A' = d0t^2 + d1t^2 + 1 and C' likewise: sums of positive terms, (1 + 2) + 1 + 1 = 5 u
          relative; B' = -2 (d0s d0t + d1s d1t): 3 u per product and 1 for the sum, 4 u of |d0s d0t| + |d1s d1t| (it may
          cancel, so the bound is on the absolute values: `Babs`); F = A' C' - B'^2 / 4: 11 u of A' C' and 10 u of Babs^2 / 4,
          then the subtraction and the reciprocal, 12 u (A' C' + Babs^2 / 4) / F relative to F (`rel_f`), which scales r2 as a
          whole; A = A' / F: 1 more; A ss ss, B ss tt, C tt tt: 2 each, the two additions 2: 10 u of each term's magnitude
          (`quad`). ss = is - s with s = st * res - 0.5: 2 roundings, u (|st res| + |s|) absolute, and st = su * u + du adds
          u (|su u| + |st|) res when the mapping is not the identity (`st_err`, in units of st); it enters r2 through its
          gradient (2 A ss + B tt, B ss + 2 C tt).
        d_rel: a relative uncertainty of the differentials themselves (0 when they are exact inputs), which moves every term
        of A', B', C' but the + 1 by 2 d_rel."""
        m = len(st)
        n = len(self.levels)
        if level >= n:
            return np.broadcast_to(self.texel(n - 1, 0, 0), (m, 3)).copy(), np.zeros(m)
        h, w, _ = self.levels[level].shape
        s, t = st[:, 0] * w - 0.5, st[:, 1] * h - 0.5
        s_err = U32 * (np.abs(st[:, 0] * w) + np.abs(s)) + st_err[:, 0] * w
        t_err = U32 * (np.abs(st[:, 1] * h) + np.abs(t)) + st_err[:, 1] * h
        d0s, d0t, d1s, d1t = d0[:, 0] * w, d0[:, 1] * h, d1[:, 0] * w, d1[:, 1] * h
        A = d0t * d0t + d1t * d1t + 1
        B = -2 * (d0s * d0t + d1s * d1t)
        Babs = 2 * (np.abs(d0s * d0t) + np.abs(d1s * d1t))
        C = d0s * d0s + d1s * d1s + 1
        F = A * C - B * B * 0.25
        rel_f = (12 * U32 + 4 * d_rel) * (A * C + Babs * Babs * 0.25) / F
        term = 10 * U32 + 2 * d_rel
        A, B, C, Babs = A / F, B / F, C / F, Babs / F
        det = -B * B + 4 * A * C
        u_sqrt, v_sqrt = np.sqrt(det * C), np.sqrt(A * det)
        s0, s1 = np.ceil(s - 2 / det * u_sqrt).astype(int), np.floor(s + 2 / det * u_sqrt).astype(int)
        t0, t1 = np.ceil(t - 2 / det * v_sqrt).astype(int), np.floor(t + 2 / det * v_sqrt).astype(int)
        # lookups with small boxes and with large ones are scanned apart, so that the many small do not idle through the large scan
        size = np.maximum(s1 - s0, t1 - t0) + 1
        value, slack = np.zeros((m, 3)), np.zeros(m)
        lo = 0
        for hi in (3, 6, 12, 24, int(size.max())):
            sel = np.nonzero((size > lo) & (size <= hi))[0]
            lo = hi
            if len(sel) == 0:
                continue
            value[sel], slack[sel] = self._ewa_scan(level, s[sel], t[sel], A[sel], B[sel], C[sel], Babs[sel], s0[sel], s1[sel],
                                                    t0[sel], t1[sel], s_err[sel], t_err[sel], rel_f[sel], term)
        return value, slack

    def _ewa_scan(self, level, s, t, A, B, C, Babs, s0, s1, t0, t1, s_err, t_err, rel_f, term):
        m = len(s)
        total, wsum = np.zeros((m, 3)), np.zeros(m)
        near_i, near_tex, near_step = [], [], []
        for jt in range(int((t1 - t0).max()) + 1):
            it = t0 + jt
            tt = it - t
            for js in range(int((s1 - s0).max()) + 1):
                i_s = s0 + js
                ss = i_s - s
                r2 = A * ss * ss + B * ss * tt + C * tt * tt
                box = (i_s <= s1) & (it <= t1)
                inside = box & (r2 < 1)
                x = r2 * LUT_SIZE
                eps = term * (A * ss * ss + Babs * np.abs(ss * tt) + C * tt * tt) + rel_f * r2 + \
                    np.abs(2 * A * ss + B * tt) * s_err + np.abs(B * ss + 2 * C * tt) * t_err
                k = np.rint(x)
                near = box & (np.abs(x - k) <= LUT_SIZE * eps) & (k >= 1) & (k <= LUT_SIZE - 1)
                if not (inside.any() or near.any()):
                    continue
                tex = self.texel(level, i_s, it)
                wgt = np.where(inside, self.lut[np.minimum(x.astype(int), LUT_SIZE - 1) * inside], 0.0)
                total += tex * wgt[:, None]
                wsum += wgt
                if near.any():
                    j = np.nonzero(near)[0]
                    kk = k[j].astype(int)
                    near_i.append(j)
                    near_tex.append(tex[j])
                    near_step.append(np.abs(self.lut[kk - 1] - self.lut[kk]))
        value = total / wsum[:, None]
        slack = np.zeros(m)
        if near_i:
            j, tex, step = np.concatenate(near_i), np.concatenate(near_tex), np.concatenate(near_step)
            np.add.at(slack, j, step * np.abs(tex - value[j]).max(1) / wsum[j])
        return value, slack

    def lookup_diff(self, st, dst0, dst1, st_err=None, d_rel=0.0):
        """MIPMap::Lookup(st, dst0, dst1) (mipmap.h:276-303) -> (value (n, 3), slack (n,)); see _ewa for the slack and for
        st_err ((n, 2), the absolute rounding st arrives with) and d_rel."""
        st, d0, d1 = (np.array(a, np.float64).reshape(-1, 2) for a in (st, dst0, dst1))
        m = len(st)
        st_err = np.zeros((m, 2)) if st_err is None else np.asarray(st_err, np.float64)
        if self.trilinear:
            width = np.maximum(np.abs(d0).max(1), np.abs(d1).max(1))
            return self.lookup(st, 2 * width), np.zeros(m)
        swap = (d0 * d0).sum(1) < (d1 * d1).sum(1)
        d0[swap], d1[swap] = d1[swap], d0[swap].copy()
        major, minor = np.sqrt((d0 * d0).sum(1)), np.sqrt((d1 * d1).sum(1))
        clamp = (minor * self.max_aniso < major) & (minor > 0)
        scale = np.where(clamp, major / np.where(clamp, minor * self.max_aniso, 1.0), 1.0)
        d1 = d1 * scale[:, None]
        minor = minor * scale
        value, slack = np.zeros((m, 3)), np.zeros(m)
        flat = minor == 0
        if flat.any():
            value[flat] = self.triangle(0, st[flat])
        n = len(self.levels)
        with np.errstate(divide="ignore"):
            lod = np.maximum(0.0, n - 1.0 + np.log2(minor))
        lod[flat] = 0
        ilod = np.floor(lod).astype(int)
        frac = lod - ilod
        for k in np.unique(np.minimum(ilod[~flat], n)):
            sel = np.nonzero(~flat & (np.minimum(ilod, n) == k))[0]
            f = frac[sel]
            a, sa = self._ewa(k, st[sel], d0[sel], d1[sel], st_err[sel], d_rel)
            b, sb = self._ewa(k + 1, st[sel], d0[sel], d1[sel], st_err[sel], d_rel)
            value[sel] = (1 - f)[:, None] * a + f[:, None] * b
            slack[sel] = (1 - f) * sa + f * sb
        return value, slack


# ---- ImageTexture::Evaluate -----------------------------------------------------------------------------------------------------
def evaluate(tex, uv, duv, uv_err=0.0, d_rel=0.0):
    """ImageTexture<RGBSpectrum, Spectrum>::Evaluate (imagemap.h:87-94) over UVMapping2D::Map (texture.cpp:93-99):
    st = (su u + du, sv v + dv), dstdx = (su dudx, sv dvdx), dstdy = (su dudy, sv dvdy), then MIPMap::Lookup(st, dstdx, dstdy).

    tex: the pair HostScene.texture(i) returns, (record with wrap, trilinear, max_aniso, su, sv, du, dv; level arrays), of which
    the record and level 0 are used: the pyramid above it is rebuilt here. uv (n, 2), duv (n, 4) = {dudx, dvdx, dudy, dvdy}.
    uv_err, d_rel: how uncertain (u, v) (absolute) and the differentials (relative) are, when they are computed and not given;
    they only widen the band of the slack. Returns (value (n, 3), slack (n,))."""
    rec, levels = tex
    mip = MipMap(np.asarray(levels[0], np.float64), wrap=rec.wrap, trilinear=rec.trilinear, max_aniso=rec.max_aniso)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    duv = np.asarray(duv, np.float64).reshape(-1, 4)
    sc, off = np.array([rec.su, rec.sv], np.float64), np.array([rec.du, rec.dv], np.float64)
    st = uv * sc + off
    identity = (sc == 1).all() and (off == 0).all()
    st_err = (0.0 if identity else U32 * (np.abs(uv * sc) + np.abs(st))) + uv_err * np.abs(sc) * np.ones_like(st)
    return mip.lookup_diff(st, duv[:, 0:2] * sc, duv[:, 2:4] * sc, st_err=st_err, d_rel=d_rel)


def texel_coordinates(tex, uv):
    """(|s|, |t|) of the lookups on level 0: st * resolution - 0.5, whose float32 rounding the bilinear weights carry."""
    rec, levels = tex
    h, w, _ = levels[0].shape
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    return np.abs((uv[:, 0] * rec.su + rec.du) * w - 0.5), np.abs((uv[:, 1] * rec.sv + rec.dv) * h - 0.5)


# ---- from the pixel to (u, v) and its differentials -----------------------------------------------------------------------------
def _look_at(pos, look, up):
    """The camera-to-world matrix of LookAt (transform.cpp:244-274)."""
    pos, look, up = (np.asarray(a, np.float64) for a in (pos, look, up))
    d = (look - pos) / np.linalg.norm(look - pos)
    right = np.cross(up / np.linalg.norm(up), d)
    right /= np.linalg.norm(right)
    new_up = np.cross(d, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, new_up, d, pos
    return m


def _perspective(fov, n, f):
    """Perspective(fov, n, f), transform.cpp:303-311."""
    persp = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, f / (f - n), -f * n / (f - n)], [0, 0, 1, 0]], np.float64)
    inv_tan = 1.0 / np.tan(np.radians(fov) / 2)
    return np.diag([inv_tan, inv_tan, 1.0, 1.0]) @ persp


def _apply_point(m, p):
    q = p @ m[:3, :3].T + m[:3, 3]
    wq = p @ m[3, :3] + m[3, 3]
    return q / wq[..., None]


class PerspectiveCamera:
    """PerspectiveCamera with a pinhole and the default screen window (api.cpp:  [-frame, frame] x [-1, 1] for a wide film,
    [-1, 1] x [-1 / frame, 1 / frame] for a tall one), camera.h:100-118 and perspective.cpp:50-63."""

    def __init__(self, xres, yres, fov, pos=(0, 0, 0), look=(0, 0, 1), up=(0, 1, 0)):
        frame = xres / yres
        x0, x1, y0, y1 = (-frame, frame, -1.0, 1.0) if frame > 1 else (-1.0, 1.0, -1 / frame, 1 / frame)
        translate = np.eye(4)
        translate[:3, 3] = [-x0, -y1, 0]
        screen_to_raster = np.diag([xres, yres, 1.0, 1.0]) @ np.diag([1 / (x1 - x0), 1 / (y0 - y1), 1.0, 1.0]) @ translate
        self.raster_to_camera = np.linalg.inv(_perspective(fov, 1e-2, 1000.0)) @ np.linalg.inv(screen_to_raster)
        origin = _apply_point(self.raster_to_camera, np.zeros(3))
        self.dx_camera = _apply_point(self.raster_to_camera, np.array([1.0, 0, 0])) - origin
        self.dy_camera = _apply_point(self.raster_to_camera, np.array([0, 1.0, 0])) - origin
        self.c2w = _look_at(pos, look, up)

    def ray_differential(self, pfilm, spp):
        """GenerateRayDifferential (perspective.cpp:124-185, no lens) and ScaleDifferentials(1 / sqrt(spp)) (camera.h / ray
        differentials, geometry.h:913-918; SamplerIntegrator::Render, integrator.cpp:284-285): (o, d, rxd, ryd) in world
        space; the auxiliary origins are o."""
        pfilm = np.asarray(pfilm, np.float64).reshape(-1, 2)
        pc = _apply_point(self.raster_to_camera, np.concatenate([pfilm, np.zeros((len(pfilm), 1))], 1))
        unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
        d, rxd, ryd = unit(pc), unit(pc + self.dx_camera), unit(pc + self.dy_camera)
        s = 1.0 / np.sqrt(spp)
        rxd, ryd = d + (rxd - d) * s, d + (ryd - d) * s
        rot = self.c2w[:3, :3].T
        return self.c2w[:3, 3].copy(), d @ rot, rxd @ rot, ryd @ rot


def hit_differentials(camera, spp, quad, pfilm):
    """Where the camera ray through film position pfilm (n, 2) meets the planar quad, and SurfaceInteraction::ComputeDifferentials
    there (interaction.cpp:103-149), by geometry: the main ray and the two auxiliary rays are intersected with the plane of the
    triangle hit, and the triangle's own affine (u, v) is differenced. The reference solves the same two equations per
    differential through two of the three coordinates, chosen by the normal's dominant axis; any choice has this solution.

    quad: (4, 3) corners with uv (0,0), (1,0), (1,1), (0,1), split as the triangles (0, 1, 2) and (0, 2, 3).
    Returns (hit (n,) bool, out (n, 6) = {u, v, dudx, dvdx, dudy, dvdy}, p (n, 3), dpdx (n, 3), dpdy (n, 3)); hit is false
    where (u, v) leaves [0, 1]^2 ("miss")."""
    quad = np.asarray(quad, np.float64)
    o, d, rxd, ryd = camera.ray_differential(pfilm, spp)
    n_rays = len(d)
    res = {}
    for name, (i, j, k), uvs in (("lower", (0, 1, 2), ((0, 0), (1, 0), (1, 1))), ("upper", (0, 2, 3), ((0, 0), (1, 1), (0, 1)))):
        p0, e1, e2 = quad[i], quad[j] - quad[i], quad[k] - quad[i]
        nrm = np.cross(e1, e2)
        uv0, duv1, duv2 = (np.asarray(uvs[0], np.float64), np.subtract(uvs[1], uvs[0]).astype(np.float64),
                           np.subtract(uvs[2], uvs[0]).astype(np.float64))
        gram = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])

        def meet(direction):
            t = ((p0 - o) @ nrm) / (direction @ nrm)
            p = o + t[:, None] * direction
            b = np.linalg.solve(gram, np.stack([(p - p0) @ e1, (p - p0) @ e2]))  # barycentrics along e1, e2
            return p, uv0 + b[0][:, None] * duv1 + b[1][:, None] * duv2, t
        p, uv, t = meet(d)
        px, uvx, _ = meet(rxd)
        py, uvy, _ = meet(ryd)
        res[name] = (p, uv, uvx - uv, uvy - uv, px - p, py - p, t)
    lower = res["lower"][1][:, 0] >= res["lower"][1][:, 1]  # v <= u: the triangle (0, 1, 2)
    pick = lambda a, b: np.where(lower.reshape((n_rays,) + (1,) * (a.ndim - 1)), a, b)
    p, uv, dx, dy, dpdx, dpdy, t = (pick(a, b) for a, b in zip(res["lower"], res["upper"]))
    hit = (uv >= 0).all(1) & (uv <= 1).all(1) & (t > 0)
    return hit, np.concatenate([uv, dx, dy], 1), p, dpdx, dpdy
