"""The smallest scenes at which each branch of PathIntegrator::Li is live, for path_ref.py: every case is at most 64 triangles,
16 x 16 pixels and 4 spp (1024 camera samples); the deep ones are 8 x 8 or 12 x 12, so that a case's truth takes a few seconds.
build(name) returns the truth's own description of the scene (path_ref.Scene, built from the numbers below and never from the
loader's tables), the .pbrt text of the same numbers, and the image files the text names.

  plain_room          a matte and plastic box room closed around the camera, one emitting sphere: the only material and light set of
                      the plain (EXT = false) build. _d8: maxdepth 8, rrthreshold 1 (roulette entered from bounce 4); _rr0 / _rr10:
                      both sides of mc < rrThreshold; _d0 / _d1: the break, and Le at bounce 0 only
  normals_quad_light  an emissive quad (two triangle lights) with a smaller one under it, a folded mesh whose `normal N` tilts 20-30 degrees off the faces (one
                      half under ReverseOrientation) in matte sigma 20, a plastic floor of roughness 0.05; maxdepth 6; _uniform /
                      _power / _spatial, and _sobol
  delta_lights        point, spot and distant light on matte and plastic, maxdepth 3; _uniform / _power
  specular            a glass slab (two parallel quads, index 1.5), a mirror quad and an uber pane of opacity 0.4 between the camera,
                      a quad emitter and a matte floor; maxdepth 8
  infinite            an infinite light with lightsample_cases' noise4x2 map over a matte and a plastic quad; maxdepth 4
"""
import numpy as np

import lightdistrib_ref as LD
import lightsample_ref as LS
import path_ref as PR

W = H = 16
SPP = 4


class Builder:
    def __init__(self):
        self.tris, self.normals, self.flip, self.tri_mat, self.mats, self.lights, self.body = [], [], [], [], [], [], []
        self.sphere, self.files = None, {}

    def mesh(self, mat, pts, idx, normals=None, reverse=False, emit=None):
        """A trianglemesh of material `mat` (a path_ref.Material); emit: the radiance of an AreaLightSource "diffuse"."""
        pts = np.asarray(pts, np.float32)
        self.mats.append(mat)
        f = lambda a: " ".join(f"{float(v):.9g}" for v in np.asarray(a, np.float32).ravel())
        t = "AttributeBegin\n" + mat.text()
        if reverse:
            t += "ReverseOrientation\n"
        if emit is not None:
            t += f'AreaLightSource "diffuse" "rgb L" [{f(emit)}]\n'
        t += f'Shape "trianglemesh" "integer indices" [{" ".join(map(str, idx))}] "point P" [{f(pts)}]'
        if normals is not None:
            normals = np.asarray(normals, np.float32)
            t += f' "normal N" [{f(normals)}]'
        self.body.append(t + "\nAttributeEnd\n")
        for a, b, c in np.asarray(idx).reshape(-1, 3):
            if emit is not None:
                self.lights.append(("tri", len(self.tris), np.asarray(emit, np.float32)))
            self.tris.append(np.concatenate([pts[a], pts[b], pts[c]]))
            self.normals.append(np.full(9, np.nan, np.float32) if normals is None else np.concatenate([normals[a], normals[b], normals[c]]))
            self.flip.append(reverse)
            self.tri_mat.append(len(self.mats) - 1)

    def quad(self, mat, p0, p1, p2, p3, **kw):
        self.mesh(mat, [p0, p1, p2, p3], [0, 1, 2, 0, 2, 3], **kw)

    def emitting_sphere(self, mat, center, radius, L):
        self.mats.append(mat)
        self.sphere = dict(center=np.asarray(center, np.float32), radius=np.float32(radius), mat=len(self.mats) - 1, L=np.asarray(L, np.float32))
        self.lights.append(("sphere",))
        c = self.sphere["center"]
        self.body.append(f'AttributeBegin\n{mat.text()}Translate {c[0]:g} {c[1]:g} {c[2]:g}\nAreaLightSource "diffuse" "rgb L" [{L[0]:g} {L[1]:g} {L[2]:g}]\n'
                         f'Shape "sphere" "float radius" [{radius:g}]\nAttributeEnd\n')

    def light(self, kind, **kw):
        self.lights.append((kind, kw))
        v = lambda a: " ".join(f"{x:g}" for x in a)
        if kind == "point":
            t = f'LightSource "point" "point from" [{v(kw["pos"])}] "rgb I" [{v(kw["I"])}]\n'
        elif kind == "spot":
            t = (f'LightSource "spot" "point from" [{v(kw["pos"])}] "point to" [{v(kw["to"])}] "rgb I" [{v(kw["I"])}] '
                 f'"float coneangle" [{kw["cone"]:g}] "float conedeltaangle" [{kw["delta"]:g}]\n')
        elif kind == "distant":
            t = f'LightSource "distant" "point from" [{v(kw["frm"])}] "point to" [{v(kw["to"])}] "rgb L" [{v(kw["L"])}]\n'
        else:
            import lightsample_cases as LC
            self.files[kw["map"] + ".pfm"] = LC.map_rows(kw["map"])
            t = f'AttributeBegin\n{LC.ROTATIONS[kw["rot"]][0]}LightSource "infinite" "rgb L" [{v(kw["L"])}] "string mapname" "{kw["map"]}.pfm"\nAttributeEnd\n'
        self.body.append(t)

    def finish(self, eye, look, fov, max_depth, rr=1.0, strategy="spatial", sampler="halton", res=W):
        head = (f'LookAt {eye}  {look}  0 1 0\nCamera "perspective" "float fov" [{fov}]\n'
                f'Film "image" "integer xresolution" [{res}] "integer yresolution" [{res}] "string filename" "path.pfm"\n'
                f'Sampler "{sampler}" "integer pixelsamples" [{SPP}]\n'
                f'Integrator "path" "integer maxdepth" [{max_depth}] "float rrthreshold" [{rr:g}] "string lightsamplestrategy" "{strategy}"\nWorldBegin\n')
        geo = PR.Scene(self.tris, self.normals, self.flip, self.tri_mat, self.mats, self.sphere, [], max_depth)
        radius = geo.world_radius()
        lights = []
        for spec in self.lights:
            if spec[0] == "tri":
                T = geo.P[spec[1]]
                nrm = None if np.isnan(geo.N[spec[1], 0]) else geo.N[spec[1]].reshape(3, 3)
                ls = LS.AreaLight(LS.Triangle(T[0:3], T[3:6], T[6:9], nrm, bool(geo.flip[spec[1]])), spec[2])
                lights.append(PR.AreaLight(ls, spec[1], LD.Tri(T[0:3], T[3:6], T[6:9], spec[2])))
            elif spec[0] == "sphere":
                s = self.sphere
                m = np.eye(4)
                m[:3, 3] = s["center"]
                inv = np.eye(4)
                inv[:3, 3] = -s["center"].astype(np.float64)
                lights.append(PR.AreaLight(LS.AreaLight(LS.Sphere(m, inv, s["radius"]), s["L"]), PR.SPHERE, PR.SpherePower(s["radius"], s["L"])))
            elif spec[0] == "point":
                lights.append(PR.PointLight(spec[1]["pos"], spec[1]["I"]))
            elif spec[0] == "spot":
                lights.append(PR.SpotLight(spec[1]["pos"], spec[1]["to"], spec[1]["I"], spec[1]["cone"], spec[1]["delta"]))
            elif spec[0] == "distant":
                lights.append(PR.DistantLight(spec[1]["frm"], spec[1]["to"], spec[1]["L"], radius))
            else:
                import lightsample_cases as LC
                kw = spec[1]
                rot = LC.ROTATIONS[kw["rot"]][1][:3, :3].astype(np.float32)
                inv = np.linalg.inv(rot.astype(np.float64)).astype(np.float32)
                lights.append(PR.InfiniteLight(LS.InfiniteLight(LC.map_rows(kw["map"])[::-1], kw["L"], rot, inv, world_radius=radius)))
        scene = PR.Scene(self.tris, self.normals, self.flip, self.tri_mat, self.mats, self.sphere, lights, max_depth, rr, strategy)
        return scene, head + "".join(self.body) + "WorldEnd\n", self.files


M = PR.Material
# An emitting quad reflects nothing: from a point of a flat emitter every sample of it, or of its coplanar other half, lies in the
# point's own tangent plane, where the side test of L and |cos| = 0 are undecided in any arithmetic.
BLACK = M("matte", Kd=(0, 0, 0))


def room(b, lo, hi, walls, floor=None, back=None):
    """The six quads of a box closed around the camera: `walls` everywhere but where floor / back (the +z wall) give their own."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    b.quad(floor or walls, (x0, y0, z0), (x0, y0, z1), (x1, y0, z1), (x1, y0, z0))
    b.quad(walls, (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1))
    b.quad(back or walls, (x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1))
    b.quad(walls, (x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0))
    b.quad(walls, (x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1))
    b.quad(walls, (x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0))


def plain_room(max_depth, rr=1.0, black_walls=False):
    b = Builder()
    x0, x1, y0, y1, z0, z1 = -2, 2, -1, 3, -3, 6
    white, red, green = M("matte", Kd=(0.7, 0.7, 0.7)), M("matte", Kd=(0.65, 0.2, 0.15)), M("matte", Kd=(0.2, 0.6, 0.25))
    floor = M("plastic", Kd=(0.5, 0.5, 0.55), Ks=(0.3, 0.3, 0.3), roughness=0.2)
    if black_walls:   # for the closed form: a matte floor under the sphere, nothing else reflects
        white = red = green = BLACK
        floor = M("matte", Kd=(0.5, 0.5, 0.5))
    b.quad(floor, (x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1))
    b.quad(white, (x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0))
    b.quad(white, (x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0))
    b.quad(white, (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))
    b.quad(red, (x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0))
    b.quad(green, (x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1))
    b.emitting_sphere(M("matte", Kd=(0.5, 0.5, 0.5)), (0.5, 1.25, 0.0), 0.5, (12.0, 11.0, 9.0))
    return b.finish("0.25 1.5 5.5", "0.1 0.75 0", 50, max_depth, rr, res=8 if max_depth > 1 else W)


def _tilted(face, offsets):
    """Per-vertex normals of a flat face: its unit normal plus tangent offsets of length tan(20 .. 30 degrees)."""
    p = np.asarray(face, np.float64)
    n = np.cross(p[0] - p[2], p[1] - p[2])
    n /= np.linalg.norm(n)
    t1 = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
    t2 = np.cross(n, t1)
    out = [n + a * t1 + c * t2 for a, c in offsets]
    return [v / np.linalg.norm(v) for v in out]


def normals_quad_light(strategy, sampler="halton"):
    b = Builder()
    room(b, (-3, 0, -7), (3, 4, 3), M("matte", Kd=(0.6, 0.6, 0.5)), floor=M("plastic", Kd=(0.3, 0.3, 0.35), Ks=(0.5, 0.5, 0.5), roughness=0.05))
    rough = M("matte", Kd=(0.7, 0.5, 0.4), sigma=20)
    left = [(-1.75, 0, -1), (-1.75, 0, 1.5), (0, 1.25, 1.5), (0, 1.25, -1)]
    right = [(0, 1.25, -1), (0, 1.25, 1.5), (1.75, 0, 1.5), (1.75, 0, -1)]
    offs = [(0.36, 0.2), (-0.3, 0.4), (0.45, -0.3), (-0.2, -0.5)]   # lengths 0.41 .. 0.54: 22 .. 28 degrees
    b.mesh(rough, left, [0, 1, 2, 0, 2, 3], normals=_tilted(left, offs))
    b.mesh(rough, right, [0, 1, 2, 0, 2, 3], normals=_tilted(right, offs[::-1]), reverse=True)
    b.quad(BLACK, (-1, 3.5, -0.5), (1, 3.5, -0.5), (1, 3.5, 1.5), (-1, 3.5, 1.5), emit=(10.0, 9.0, 8.0))
    # a second emitter under the first: a BSDF-half ray aimed at the upper one may end on the lower, which then adds nothing (under
    # uniform and power only: the spatial distribution's cdf steps carry wide bands, and four lights' would cost the kept share)
    if strategy != "spatial":
        b.quad(BLACK, (-0.5, 3.0, 0), (0.5, 3.0, 0), (0.5, 3.0, 1), (-0.5, 3.0, 1), emit=(6.0, 6.0, 8.0))
    return b.finish("0.5 2.75 -6.5", "0 1 0.5", 45, 6, strategy=strategy, sampler=sampler, res=8)


def delta_lights(strategy):
    b = Builder()
    room(b, (-3, 0, -7), (3, 4, 3), M("matte", Kd=(0.6, 0.5, 0.5)), floor=M("plastic", Kd=(0.4, 0.4, 0.4), Ks=(0.4, 0.4, 0.4), roughness=0.15))
    lo, hi = (-0.5, 0, -0.25), (0.75, 1.25, 1.0)
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    idx = [0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 3, 7, 6, 3, 6, 2, 0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5]
    b.mesh(M("matte", Kd=(0.3, 0.5, 0.7)), c, idx)
    b.light("point", pos=(-1.5, 2.5, -1.0), I=(6.0, 5.0, 4.0))
    b.light("spot", pos=(2.0, 3.0, -1.5), to=(0.5, 0.0, 0.5), I=(20.0, 20.0, 25.0), cone=30.0, delta=8.0)
    b.light("distant", frm=(-1.0, 3.0, -2.0), to=(0.0, 0.0, 0.0), L=(0.75, 0.75, 0.5))
    return b.finish("0.5 3 -6.5", "0 0.5 0.5", 45, 3, strategy=strategy, res=12)


def specular():
    b = Builder()
    room(b, (-3, 0, -7), (3, 4, 3), M("matte", Kd=(0.6, 0.6, 0.6)))
    glass = M("glass", index=1.5)
    # the slab: two parallel quads 0.5 apart, normals outwards; its open sides let floor light in at steep angles (total internal reflection)
    b.quad(glass, (-1.5, 0.25, -1.0), (-1.5, 1.75, -1.0), (-0.25, 1.75, -1.0), (-0.25, 0.25, -1.0))
    b.quad(glass, (-1.5, 0.25, -0.5), (-0.25, 0.25, -0.5), (-0.25, 1.75, -0.5), (-1.5, 1.75, -0.5))
    b.quad(M("mirror", Kr=(0.9, 0.9, 0.9)), (0.25, 0.1, 1.5), (0.25, 2.1, 1.5), (2.25, 2.1, 0.5), (2.25, 0.1, 0.5))
    b.quad(M("uber", Kd=(0.5, 0.3, 0.3), Ks=(0.3, 0.3, 0.3), roughness=0.1, opacity=0.4), (0.25, 0.25, -1.25), (0.25, 1.75, -1.25), (1.5, 1.75, -1.25), (1.5, 0.25, -1.25))
    b.quad(BLACK, (-1.0, 0.5, 2.5), (-1.0, 2.5, 2.5), (1.0, 2.5, 2.5), (1.0, 0.5, 2.5), emit=(10.0, 10.0, 8.0))
    return b.finish("0 1.5 -6", "0 1 0", 40, 8, res=8)


def infinite():
    b = Builder()
    b.quad(M("matte", Kd=(0.6, 0.5, 0.4)), (-3, 0, -3), (-3, 0, 3), (0, 0, 3), (0, 0, -3))
    b.quad(M("plastic", Kd=(0.3, 0.3, 0.3), Ks=(0.5, 0.5, 0.5), roughness=0.1), (0, 0, -3), (0, 0, 3), (3, 0.75, 3), (3, 0.75, -3))
    b.light("infinite", map="noise4x2", rot="z", L=(0.75, 1.25, 0.5))
    return b.finish("0 3 -7", "0 -0.5 0", 45, 4)


CASES = {
    "plain_room_d8": lambda: plain_room(8), "plain_room_rr0": lambda: plain_room(8, 0.0), "plain_room_rr10": lambda: plain_room(8, 10.0),
    "plain_room_d0": lambda: plain_room(0), "plain_room_d1": lambda: plain_room(1),
    "normals_quad_light_uniform": lambda: normals_quad_light("uniform"), "normals_quad_light_power": lambda: normals_quad_light("power"),
    "normals_quad_light_spatial": lambda: normals_quad_light("spatial"), "normals_quad_light_sobol": lambda: normals_quad_light("spatial", "sobol"),
    "delta_lights_uniform": lambda: delta_lights("uniform"), "delta_lights_power": lambda: delta_lights("power"),
    "specular": specular, "infinite": infinite,
}

# what each case is for: the counts of PathTruth.stats that must not be zero on the truth alone
LIVE = {
    "plain_room_d8": ("rr_survived", "rr_died", "bsdf_half"), "plain_room_rr10": ("rr_survived", "rr_died"),
    "normals_quad_light_uniform": ("bsdf_half", "ns_ng_disagree", "other_emitter"), "normals_quad_light_power": ("bsdf_half", "ns_ng_disagree", "other_emitter"),
    "normals_quad_light_spatial": ("bsdf_half", "ns_ng_disagree"), "normals_quad_light_sobol": ("bsdf_half", "ns_ng_disagree"),
    "specular": ("specular_emitter", "eta_scale", "tir", "pass_through"), "infinite": ("bsdf_half", "escaped_le"),
}


def build(name):
    """(path_ref.Scene, .pbrt text, {file name: rows (bottom scanline first)} of the images the text names)."""
    return CASES[name]()
