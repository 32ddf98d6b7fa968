"""A float32 restatement of pbrt-v3's procedural textures and 2D / 3D texture mappings (src/core/texture.cpp, src/textures/
checkerboard.h, uv.h, bilerp.h, scale.h, mix.h), vectorised over points, in the reference's order of operations.

Every operation rounds to float32 as the reference's Float arithmetic does (the library is built with -ffp-contract=off, so no
product is fused into a sum). The transcendental functions are the exception: acos and atan2 are taken in float64 and rounded,
as the device's portable versions do; a result may then differ from the device's by an ulp or so of the angle.

A texture is the dict of `HostScene.procedural_texture`; `images` maps a texture index to a callable (u, v) -> (n, 3) for the
image leaves a test uses (the restatement does not refilter MIP maps)."""
import numpy as np

F = np.float32
PI, INV_PI, INV_2PI = F(3.14159265358979323846), F(0.31830988618379067154), F(0.15915494309189533577)
TEX_IMAGE, TEX_SCALE, TEX_MIX, TEX_CHECKER2D, TEX_CHECKER3D, TEX_UV, TEX_BILERP = range(7)
MAP_UV, MAP_SPHERICAL, MAP_CYLINDRICAL, MAP_PLANAR = range(4)
AA_CLOSEDFORM, AA_NONE = range(2)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def dot3(a, b):
    """Dot(a, b) = a.x * b.x + a.y * b.y + a.z * b.z, summed left to right."""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def xf_point(xf, p):
    """Transform::operator()(Point3f) of an affine 3 x 4 (transform.h:217-232)."""
    xf = f32(xf)
    return np.stack([((xf[r, 0] * p[:, 0] + xf[r, 1] * p[:, 1]) + xf[r, 2] * p[:, 2]) + xf[r, 3] for r in range(3)], 1)


def normalize(v):
    """Normalize: v / Length(v), the division taken as a multiplication by 1 / Length (Vector3::operator/)."""
    inv = F(1) / np.sqrt(dot3(v, v))
    return v * inv[:, None]


def sphere(xf, p):
    """SphericalMapping2D::sphere (texture.cpp:119-123)."""
    vec = normalize(xf_point(xf, p))
    theta = np.arccos(np.clip(vec[:, 2], F(-1), F(1)).astype(np.float64)).astype(np.float32)
    phi = np.arctan2(vec[:, 1].astype(np.float64), vec[:, 0].astype(np.float64)).astype(np.float32)
    phi = np.where(phi < 0, phi + F(2) * PI, phi)
    return theta * INV_PI, phi * INV_2PI


def cylinder(xf, p):
    """CylindricalMapping2D::cylinder (texture.h:92-95)."""
    vec = normalize(xf_point(xf, p))
    phi = np.arctan2(vec[:, 1].astype(np.float64), vec[:, 0].astype(np.float64)).astype(np.float32)
    return (PI + phi) * INV_2PI, vec[:, 2]


def wrap_dt(d):
    """The discontinuity fix-up of the spherical and cylindrical mappings' dt (texture.cpp:108-116, 133-141)."""
    return np.where(d > F(.5), F(1) - d, np.where(d < F(-.5), -(d + F(1)), d))


def map2d(t, uv, duv, p, dpdx, dpdy):
    """TextureMapping2D::Map: (s, t, dsdx, dtdx, dsdy, dtdy)."""
    uv, duv, p, dpdx, dpdy = f32(uv), f32(duv), f32(p), f32(dpdx), f32(dpdy)
    m = t["mapping"]
    if m == MAP_UV:  # UVMapping2D::Map, texture.cpp:93-99
        su, sv, du, dv = F(t["su"]), F(t["sv"]), F(t["du"]), F(t["dv"])
        return (su * uv[:, 0] + du, sv * uv[:, 1] + dv, su * duv[:, 0], sv * duv[:, 1], su * duv[:, 2], sv * duv[:, 3])
    if m == MAP_PLANAR:  # PlanarMapping2D::Map, texture.cpp:147-153
        vs, vt = np.broadcast_to(f32(t["vs"]), p.shape), np.broadcast_to(f32(t["vt"]), p.shape)
        return (F(t["du"]) + dot3(p, vs), F(t["dv"]) + dot3(p, vt), dot3(dpdx, vs), dot3(dpdx, vt), dot3(dpdy, vs), dot3(dpdy, vt))
    fn, delta = (sphere, F(.1)) if m == MAP_SPHERICAL else (cylinder, F(.01))
    s, tt = fn(t["xf"], p)
    sx, tx = fn(t["xf"], p + delta * dpdx)
    sy, ty = fn(t["xf"], p + delta * dpdy)
    inv = F(1) / delta  # Vector2f::operator/
    return s, tt, (sx - s) * inv, wrap_dt((tx - tt) * inv), (sy - s) * inv, wrap_dt((ty - tt) * inv)


def _parity(*floors):
    """(int)floor(a) + (int)floor(b) [+ ...] % 2 == 0, with C++'s % (negative for a negative odd sum): 0 selects tex1."""
    total = sum(np.floor(f).astype(np.int64) for f in floors)
    return np.where(np.fmod(total, 2) == 0, 0, 1)


def checker(t, uv, duv, p, dpdx, dpdy):
    """Checkerboard{2D,3D}Texture::Evaluate short of the lookups: (sel, area2, inside). sel 0 / 1: tex1 / tex2 alone; sel 2: the
    closed-form blend (1 - area2) * tex1 + area2 * tex2. inside: where the result is a pure selection."""
    if t["kind"] == TEX_CHECKER3D:  # IdentityMapping3D(tex2world): tex2world is the WorldToTexture (checkerboard.cpp:91, 149)
        q = xf_point(t["xf"], f32(p))
        sel = _parity(q[:, 0], q[:, 1], q[:, 2])
        return sel, np.zeros(len(sel), np.float32), np.ones(len(sel), bool)
    s, tt, dsdx, dtdx, dsdy, dtdy = map2d(t, uv, duv, p, dpdx, dpdy)
    sel = _parity(s, tt)
    if t["aamode"] == AA_NONE:
        return sel, np.zeros(len(sel), np.float32), np.ones(len(sel), bool)
    ds, dt = np.maximum(np.abs(dsdx), np.abs(dsdy)), np.maximum(np.abs(dtdx), np.abs(dtdy))
    s0, s1, t0, t1 = s - ds, s + ds, tt - dt, tt + dt
    inside = (np.floor(s0) == np.floor(s1)) & (np.floor(t0) == np.floor(t1))

    def bump_int(x):
        h = x / F(2)
        fl = np.floor(h).astype(np.int64).astype(np.float32)
        return fl + F(2) * np.maximum(h - fl - F(.5), F(0))

    with np.errstate(divide="ignore", invalid="ignore"):
        sint = (bump_int(s1) - bump_int(s0)) / (F(2) * ds)
        tint = (bump_int(t1) - bump_int(t0)) / (F(2) * dt)
    area2 = sint + tint - F(2) * sint * tint
    area2 = np.where((ds > 1) | (dt > 1), F(.5), area2).astype(np.float32)
    return np.where(inside, sel, 2), area2, inside


def blend(a2, a, b):
    a2 = a2[:, None]
    return (F(1) - a2) * a + a2 * b


def evaluate(textures, idx, uv, duv, p, dpdx, dpdy, images=None):
    """Texture::Evaluate of texture idx (of any kind) -> (n, 3) float32."""
    t = textures[idx]
    n = len(uv)
    k = t["kind"]
    args = (uv, duv, p, dpdx, dpdy)
    if k == TEX_IMAGE:
        return f32(images[idx](uv, duv))
    if k == TEX_UV:  # UVTexture, uv.h:54-60
        s, tt = map2d(t, *args)[:2]
        return np.stack([s - np.floor(s), tt - np.floor(tt), np.zeros(n, np.float32)], 1)
    if k == TEX_BILERP:  # BilerpTexture, bilerp.h:56-62
        s, tt = map2d(t, *args)[:2]
        c = f32(t["bilerp"])
        w = [(F(1) - s) * (F(1) - tt), (F(1) - s) * tt, s * (F(1) - tt), s * tt]
        return ((w[0][:, None] * c[0] + w[1][:, None] * c[1]) + w[2][:, None] * c[2]) + w[3][:, None] * c[3]

    def inp(j):
        if t["child"][j] < 0:
            return np.broadcast_to(f32(t["cval"][j]), (n, 3))
        return evaluate(textures, t["child"][j], *args, images=images)

    if k == TEX_SCALE:  # ScaleTexture, scale.h:56-58
        return inp(0) * inp(1)
    if k == TEX_MIX:  # MixTexture, mix.h:57-61
        a, b, amt = inp(0), inp(1), inp(2)[:, :1]
        return (F(1) - amt) * a + amt * b
    sel, a2, _ = checker(t, *args)
    a, b = inp(0), inp(1)
    out = blend(a2, a, b)
    out = np.where((sel == 0)[:, None], a, np.where((sel == 1)[:, None], b, out))
    return out.astype(np.float32)


def edge_distance(t, uv, duv, p, dpdx, dpdy):
    """How far each point lies from a check edge (in the texture's own (s, t) or 3D units), or from the mapping's seam: points closer
    than a test's margin are left out where a one-ulp difference of the mapping could flip the selection."""
    if t["kind"] == TEX_CHECKER3D:
        q = xf_point(t["xf"], f32(p)).astype(np.float64)
        return np.min(np.abs(q - np.round(q)), axis=1)
    s, tt, dsdx, dtdx, dsdy, dtdy = [np.asarray(x, np.float64) for x in map2d(t, uv, duv, p, dpdx, dpdy)]
    d = np.minimum(np.abs(s - np.round(s)), np.abs(tt - np.round(tt)))
    if t["kind"] == TEX_CHECKER2D and t["aamode"] == AA_CLOSEDFORM:
        ds, dt = np.maximum(np.abs(dsdx), np.abs(dsdy)), np.maximum(np.abs(dtdx), np.abs(dtdy))
        for c, w in ((s, ds), (tt, dt)):  # the filter box's sides
            d = np.minimum(d, np.minimum(np.abs(c - w - np.round(c - w)), np.abs(c + w - np.round(c + w))))
    return d
