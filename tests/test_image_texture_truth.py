"""The ImageTexture path of the host and of the CPU oracle against mipmap_ref.py's float64 statement of the reference: the MIP
pyramid the host builds, the oracle's filtered lookups (EWA, trilinear, bilinear; repeat / clamp / black; the UV mapping),
the oracle's camera-ray differentials on tilted quads of every dominant normal axis, and the per-sample radiance of a textured
quad. test_gpu_image_texture_truth.py holds the device to the same truths and shares the configurations defined here.

Each test prints the distances it measured before it asserts (pytest -s shows them)."""
import zlib

import numpy as np
import pytest

import mipmap_ref as MR

# ---- images and texture configurations ------------------------------------------------------------------------------------------
IMAGES = {"12x5": (12, 5), "8x16": (8, 16), "5x1": (5, 1), "1x1": (1, 1)}  # width x height: two, no, one non-power-of-two sides
OPTIONS = {"ewa": '',
           "clamp": ' "string wrap" ["clamp"]',
           "black": ' "string wrap" ["black"]',
           "trilinear": ' "bool trilinear" ["true"]',
           "trilinear-black": ' "bool trilinear" ["true"] "string wrap" ["black"]',
           "aniso2-mapped": ' "float maxanisotropy" [2] "float uscale" [3] "float vdelta" [.3]',
           "aniso1": ' "float maxanisotropy" [1]'}
CONFIGS = [(i, o) for i in IMAGES for o in OPTIONS]
N_LOOKUPS = 2000


def image(name):
    """rand^2 * 3, (h, w, 3), row index = t: dark texels next to bright ones, so that Lanczos' negative lobes reach the clamp to >= 0."""
    w, h = IMAGES[name]
    rng = np.random.default_rng(1000 + 17 * w + h)
    return (rng.random((h, w, 3)) ** 2 * 3).astype(np.float32)


def write_pfm(path, img):
    """A PFM's scanlines run bottom-up and ImageTexture puts the bottom scanline at t = 0: img's row index is t."""
    path.write_bytes(b"PF\n%d %d\n-1.0\n" % (img.shape[1], img.shape[0]) + np.ascontiguousarray(img, "<f4").tobytes())


FACING = np.array([[-1, -1, 5], [1, -1, 5], [1, 1, 5], [-1, 1, 5]], np.float32)


def quad_scene(directory, binding, image_name, options, quad=FACING, xres=64, yres=48, spp=4, fov=40):
    """A uv-mapped quad (corners in uv order (0,0), (1,0), (1,1), (0,1)) with `matte` Kd read from the image texture, seen by a
    perspective camera at the origin looking down +z, lit by a point light at the camera."""
    write_pfm(directory / f"{image_name}.pfm", image(image_name))
    pts = " ".join("%.9g" % float(x) for x in np.asarray(quad, np.float32).ravel())
    path = directory / f"{image_name}-{zlib.crc32(repr((options, pts, xres, yres, spp, fov)).encode()):08x}.pbrt"
    path.write_text(
        'LookAt 0 0 0  0 0 1  0 1 0\nCamera "perspective" "float fov" [%g]\n'
        'Film "image" "integer xresolution" [%d] "integer yresolution" [%d]\nSampler "halton" "integer pixelsamples" [%d]\n'
        'WorldBegin\nLightSource "point" "point from" [0 0 0]\n'
        'Texture "t" "spectrum" "imagemap" "string filename" ["%s.pfm"]%s\nMaterial "matte" "texture Kd" ["t"]\n'
        'Shape "trianglemesh" "point P" [%s] "integer indices" [0 1 2 0 2 3] "float uv" [0 0 1 0 1 1 0 1]\nWorldEnd\n'
        % (fov, xres, yres, spp, image_name, options, pts))
    return binding.HostScene(path=str(path))


def lookup_inputs(seed, n=N_LOOKUPS):
    """Lookups drawn as test_gpu_parity.py::test_image_textures_bitwise draws them; non-zero differentials are kept at 1e-12 or
    more in magnitude, so that their squares stay normal in float32 and `minor == 0` is decided alike in float32 and float64."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1.5, 2.5, (n, 2)).astype(np.float32)
    duv = (rng.standard_normal((n, 4)) * 10.0 ** rng.uniform(-5, 0.3, (n, 1))).astype(np.float32)
    tiny = (duv != 0) & (np.abs(duv) < 1e-12)
    duv[tiny] = np.copysign(np.float32(1e-12), duv[tiny])
    duv[::5] = 0            # no differentials: bilinear at level 0
    duv[1::9, 2:] = 0       # a degenerate ellipse (minor axis 0)
    duv[2::13, :2] *= 50    # anisotropy beyond maxanisotropy
    return uv, duv


class LookupCase:
    """One (image, options) configuration: its scene, its lookups, the truth and the tolerance per lookup."""

    def __init__(self, directory, binding, image_name, option_name, n=N_LOOKUPS):
        self.name = f"{image_name} {option_name}"
        self.scene = quad_scene(directory, binding, image_name, OPTIONS[option_name])
        self.tex = self.scene.texture(0)
        self.uv, self.duv = lookup_inputs(CONFIGS.index((image_name, option_name)), n)
        self.want, self.slack = MR.evaluate(self.tex, self.uv, self.duv)
        self.scale = float(self.tex[1][0].max())
        s, t = MR.texel_coordinates(self.tex, self.uv)
        # the bilinear / EWA weights carry the float32 rounding of st * res - 0.5; 2^-20 for the sums that follow
        self.tol = self.scale * (4 * MR.ulp32(1 + np.maximum(s, t)) + 2.0 ** -20) + self.slack

    def check_slack_cap(self):
        """Slack on at most 2 % of the lookups and at most 1 % of scale; a slack under 1e-12 of scale (texels that equal the
        value but for rounding, as on a 1 x 1 image) is none."""
        share, worst = float((self.slack > 1e-12 * self.scale).mean()), float(self.slack.max())
        assert share <= 0.02 and worst <= 0.01 * self.scale, f"{self.name}: slack on {share:.2%} of lookups, largest {worst / self.scale:.2%} of scale"
        return share, worst / self.scale

    def check(self, got, who):
        """Every lookup of `got` (the first len(got) lookups) within its tolerance of the truth; returns the largest distance
        outside the slack, in units of scale."""
        n = len(got)
        err = np.abs(np.asarray(got, np.float64) - self.want[:n]).max(1)
        assert np.isfinite(err).all(), f"{who}, {self.name}: non-finite values"
        bad = np.nonzero(err > self.tol[:n])[0]
        assert len(bad) == 0, (f"{who}, {self.name}: {len(bad)} of {len(err)} lookups off the float64 truth, worst {err[bad].max() / self.scale:.3g} "
                               f"of scale at lookup {bad[np.argmax(err[bad])]} (tolerance there {self.tol[bad[np.argmax(err[bad])]] / self.scale:.3g})")
        return float(np.maximum(err - self.slack[:n], 0).max() / self.scale)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("image_texture_truth")


# ---- the pyramid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", ["repeat", "clamp", "black"])
@pytest.mark.parametrize("image_name", list(IMAGES))
def test_host_pyramid_against_the_float64_constructor(binding, workdir, image_name, wrap):
    """MIPMap's constructor (mipmap.h:116-218) on non-constant images: every level the host builds is the float64 statement's
    to 16 * 2^-24 of the level's maximum (two normalised four-tap sums and the box average: about ten float32 roundings).
    Measured: at most 1.9e-7 of the maximum (12x5, repeat). The images are dark next to bright, so where the image is resampled
    the clamp to >= 0 is at work: the truth's level 0 has zeros the raw image has not."""
    img = image(image_name)
    scene = quad_scene(workdir, binding, image_name, ' "string wrap" ["%s"]' % wrap)
    rec, levels = scene.texture(0)
    truth = MR.MipMap(img, wrap=wrap).levels
    assert MR.WRAPS[rec.wrap] == wrap
    assert [l.shape for l in levels] == [l.shape for l in truth]
    assert truth[-1].shape[:2] == (1, 1)
    w, h = IMAGES[image_name]
    if image_name == "12x5":
        assert (img > 0).all() and (truth[0] == 0).any(), "the clamp to >= 0 is not exercised"
        assert [l.shape[:2] for l in truth] == [(8, 16), (4, 8), (2, 4), (1, 2), (1, 1)]
    if image_name == "5x1":
        assert [l.shape[:2] for l in truth] == [(1, 8), (1, 4), (1, 2), (1, 1)]
    worst = 0.0
    for k, (got, want) in enumerate(zip(levels, truth)):
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst = max(worst, err / want.max())
        assert err <= 16 * 2.0 ** -24 * want.max(), f"{image_name} {wrap} level {k}: {err / want.max():.3g} of the maximum"
    print(f"pyramid {image_name} {wrap}: largest level distance {worst:.3g} of the level maximum")


# ---- the lookups ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_name,option_name", CONFIGS)
def test_oracle_lookups_against_the_float64_truth(binding, oracle, workdir, image_name, option_name):
    """oracle.texture_eval against ImageTexture::Evaluate in float64, 2000 lookups per configuration, each within
    scale * (4 ulp32(1 + max(|s|, |t|)) + 2^-20) + slack of the truth (about 3e-5 * scale at |s| <= 120). Measured: at most
    8.1e-7 of scale plain and 2.7e-6 with `uscale 3`, slack on at most 0.55 % of a configuration's lookups and 0.36 % of scale; one wrong index, sign, axis or level moves values by 1e-3 to 1."""
    case = LookupCase(workdir, binding, image_name, option_name)
    share, worst = case.check_slack_cap()
    dist = case.check(oracle.texture_eval(case.scene, 0, case.uv, case.duv), "oracle")
    print(f"lookups {case.name}: oracle to truth {dist:.3g} of scale; slack on {share:.2%} of lookups, largest {worst:.3g} of scale")


# ---- the differentials ------------------------------------------------------------------------------------------------------------
CENTRE, HALF = np.array([0.1, -0.05, 5.0]), 1.5
FILM = dict(xres=64, yres=48, spp=4, fov=40)
NORMALS = {"facing": (0, 0, -1), "tilted-z": (0.3, -0.4, -0.85), "x": (0.97, 0, 0.26), "x-near-y": (-0.72, -0.6, 0.34),
           "y": (0.25, 0.9, -0.36),
           # normals with no z at all, seen from the side: here the x and y branches of the dominant-axis choice cannot be traded
           # for the z branch, whose two equations (through x and y) are then singular; with n.z = 0.26 they are merely four times
           # worse conditioned, which stays inside the bound
           "x-no-z": (0.8, 0.6, 0), "y-no-z": (0.5, 0.85, 0)}
CENTRES = {"x-no-z": (1.2, -0.05, 3.5), "y-no-z": (0.1, 1.0, 3.5)}  # off the axis, or they would be seen edge-on
DOMINANT = {"facing": 2, "tilted-z": 2, "x": 0, "x-near-y": 0, "y": 1, "x-no-z": 0, "y-no-z": 1}


def tilted_quad(name, spin=0.4):
    """The four corners (float32) of a square of half-side HALF around CENTRE (or CENTRES[name]) with the normal NORMALS[name],
    turned in its plane by `spin`."""
    centre = np.asarray(CENTRES.get(name, CENTRE), np.float64)
    n = np.asarray(NORMALS[name], np.float64)
    n /= np.linalg.norm(n)
    a = np.cross(n, [0.0, 1.0, 0.0] if abs(n[1]) < 0.9 else [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    e1, e2 = np.cos(spin) * a + np.sin(spin) * b, -np.sin(spin) * a + np.cos(spin) * b
    return np.array([centre + HALF * (sx * e1 + sy * e2) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]).astype(np.float32)


def dominant_axis(quad):
    q = np.asarray(quad, np.float64)
    return int(np.argmax(np.abs(np.cross(q[1] - q[0], q[2] - q[0]))))


@pytest.mark.parametrize("name", list(NORMALS))
def test_oracle_differentials_against_geometry(binding, oracle, workdir, name):
    """oracle.camera_hit_differentials (GenerateRayDifferential, ScaleDifferentials(1 / sqrt(spp)), ComputeDifferentials) on a
    non-square film, on quads whose normal is dominant in z, in x (one close to the x / y tie) and in y, and on two whose
    normal has no z component (where taking the z branch for the x or the y branch is singular, not just less accurate):
    (u, v) within 4 ulp32 of 1; the four differentials, relative to the largest of them, within
    8 ulp32(max |p|) / max(|dpdx|, |dpdy|), which is the cancellation of px - p (about 1e-4 here; measured at most 1.8e-5, and
    3.5e-7 on (u, v)); a miss exactly where the truth's (u, v) leaves the unit square, but for a band of 1e-4 at its edge."""
    quad = tilted_quad(name)
    assert dominant_axis(quad) == DOMINANT[name]
    scene = quad_scene(workdir, binding, "12x5", "", quad=quad, **FILM)
    camera = MR.PerspectiveCamera(FILM["xres"], FILM["yres"], FILM["fov"])
    rng = np.random.default_rng(300 + list(NORMALS).index(name))
    pfilm = (rng.random((400, 2)) * [FILM["xres"], FILM["yres"]]).astype(np.float32)
    hit, want, p, dpdx, dpdy = MR.hit_differentials(camera, FILM["spp"], quad, pfilm)
    edge = (np.abs(want[:, :2]) < 1e-4).any(1) | (np.abs(want[:, :2] - 1) < 1e-4).any(1)
    assert edge.mean() <= 0.01
    n_hit, worst_uv, worst_d = 0, 0.0, 0.0
    for i in range(len(pfilm)):
        got = oracle.camera_hit_differentials(scene, float(pfilm[i, 0]), float(pfilm[i, 1]))
        if edge[i]:
            continue
        assert (got is not None) == bool(hit[i]), f"{name}: film position {pfilm[i]} hit / miss disagrees, truth (u, v) = {want[i, :2]}"
        if got is None:
            continue
        n_hit += 1
        got = got.astype(np.float64)
        e_uv = np.abs(got[:2] - want[i, :2]).max()
        e_d = np.abs(got[2:] - want[i, 2:]).max() / np.abs(want[i, 2:]).max()
        bound = 8 * MR.ulp32(np.abs(p[i]).max()) / max(np.linalg.norm(dpdx[i]), np.linalg.norm(dpdy[i]))
        worst_uv, worst_d = max(worst_uv, e_uv), max(worst_d, e_d)
        assert e_uv <= 4 * MR.ulp32(1.0), f"{name}: (u, v) at {pfilm[i]} off by {e_uv:.3g}"
        assert e_d <= bound, f"{name}: differentials at {pfilm[i]} off by {e_d:.3g} of the largest (bound {bound:.3g}): {got[2:]} vs {want[i, 2:]}"
    assert n_hit >= 50, f"{name}: only {n_hit} of 400 film positions hit the quad"
    print(f"differentials {name}: {n_hit} hits; (u, v) {worst_uv:.3g}; differentials {worst_d:.3g} of the largest; {int(edge.sum())} skipped at the edge")


# ---- from the pixel: per-sample radiance of a textured quad ---------------------------------------------------------------------
LI_CASES = [(axis, filt) for axis in ("tilted-z", "x", "y") for filt in ("ewa", "trilinear")]
LI_WINDOW = (24, 40, 18, 30)  # x0, x1, y0, y1: 16 x 12 pixels around the film's centre
LI_MEASURED = 3.6e-6  # of scale: the largest oracle-to-truth distance test_oracle_li_per_sample_against_the_truth measured
LI_BOUND = 4 * LI_MEASURED
LI_CAP = 2e-3
# The lookup tests cap the share of lookups with slack at 2 %; that cannot hold here, where the band on r2 carries the 2e-5 of
# the computed differentials and 4 ulp32 of (u, v): it averages 7e-5 on r2 (4e-6 sufficed for given differentials), so one
# texel lies within it of one of the 128 steps with probability 2 * 128 * 7e-5 = 1.8 %, and a footprint holds 6.4 to 8.1 texels
# over its two levels: 11 to 15 % if the texels fell independently. Measured: 5.6 to 6.5 %. The cap is 10 %: half as much again
# as measured, and under what the band allows at worst, so a band widened further fails here.
LI_SLACK_SHARE_CAP = 0.10
LI_SLACK_CAP = 0.01  # of scale, as for the lookups


class LiCase:
    """One textured quad seen from the pixel: the scene and the (px, py, k) of every sample of the window."""

    def __init__(self, directory, binding, axis, filt):
        self.name = f"{axis} {filt}"
        self.quad = tilted_quad(axis)
        self.scene = quad_scene(directory, binding, "12x5", OPTIONS[filt], quad=self.quad, **FILM)
        x0, x1, y0, y1 = LI_WINDOW
        ys, xs, ks = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), np.arange(FILM["spp"]), indexing="ij")
        self.px, self.py, self.k = (a.ravel().astype(np.int32) for a in (xs, ys, ks))

    def truth(self, film_positions):
        """(hit, (u, v) (n, 2), Li (n, 3), scale per sample (n,), slack (n,)): Li = Kd / pi * I / r^2 * |cos theta| with I = 1 and
        the light at the camera; a single planar quad receives no indirect light. scale is the largest texel's Li there. The
        slack's band is widened by what the float32 hit and its differentials carry: 4 ulp32 of (u, v) and 2e-5 relative of
        the differentials."""
        camera = MR.PerspectiveCamera(FILM["xres"], FILM["yres"], FILM["fov"])
        hit, uvd, p, _, _ = MR.hit_differentials(camera, FILM["spp"], self.quad, film_positions)
        tex = self.scene.texture(0)
        kd, slack = MR.evaluate(tex, uvd[:, :2], uvd[:, 2:], uv_err=4 * MR.ulp32(1.0), d_rel=2e-5)
        q = self.quad.astype(np.float64)
        n = np.cross(q[1] - q[0], q[2] - q[0])
        n /= np.linalg.norm(n)
        r2 = (p * p).sum(1)
        geom = np.abs(p @ n) / np.sqrt(r2) / r2 / np.pi
        li = kd * geom[:, None]
        li[~hit] = 0
        return hit, uvd[:, :2], li, geom * float(tex[1][0].max()), geom * slack

    def distance(self, got, film_positions):
        """got: per-sample Li at film_positions (n, 2), the film positions of (px, py, k). Returns (the largest |got - truth|
        outside the slack in units of the sample's scale, number of hits, share of them with slack, largest slack in units of
        scale), after asserting the slack's caps (LI_SLACK_SHARE_CAP, LI_SLACK_CAP): the slack is part of the tolerance, so
        whoever compares against this truth is held to them. Samples within 1e-4 of the quad's edge in (u, v) may hit or
        miss and are left out."""
        hit, uv, li, scale, slack = self.truth(film_positions)
        edge = (np.abs(uv) < 1e-4).any(1) | (np.abs(uv - 1) < 1e-4).any(1)
        got = np.asarray(got, np.float64)
        assert (got[~hit & ~edge] == 0).all(), f"{self.name}: radiance where the truth misses the quad"
        use = hit & ~edge
        assert use.sum() >= 200, f"{self.name}: only {int(use.sum())} samples of the window hit the quad"
        assert (got[use] > 0).any(1).mean() > 0.9
        rel_slack = slack[use] / scale[use]
        share, worst = float((rel_slack > 1e-12).mean()), float(rel_slack.max())
        assert share <= LI_SLACK_SHARE_CAP and worst <= LI_SLACK_CAP, \
            f"{self.name}: slack on {share:.2%} of samples, largest {worst:.2%} of scale: the ambiguity band is too wide"
        err = np.abs(got[use] - li[use]).max(1)
        return float((np.maximum(err - slack[use], 0) / scale[use]).max()), int(use.sum()), share, worst


def oracle_film_positions(oracle, scene, px, py, k):
    """(px, py) + the Halton sampler's dimensions 0 and 1, as the camera sample is drawn."""
    out = np.empty((len(px), 2), np.float32)
    for i in range(len(px)):
        idx = oracle.halton_index(scene, int(px[i]), int(py[i]), int(k[i]))
        out[i] = (np.float32(px[i]) + np.float32(oracle.halton_sample(scene, idx, 0)),
                  np.float32(py[i]) + np.float32(oracle.halton_sample(scene, idx, 1)))
    return out


@pytest.mark.parametrize("axis,filt", LI_CASES)
def test_oracle_li_per_sample_against_the_truth(binding, oracle, workdir, axis, filt):
    """The oracle's per-sample Li of a textured tilted quad against the truth built from the pixel: film position ->
    hit_differentials -> evaluate -> Kd / pi * I / r^2 * |cos|. How far the smooth part of the lookup moves with the 2e-5
    relative error of float32 differentials has no closed form, so it is measured here, where the oracle stands in for the
    device: the largest distance outside the slack over the six cases is 3.6e-6 of scale (LI_MEASURED; trilinear on the
    y-dominant quad; EWA stays under 2.3e-6), with slack on 5.6 to 6.5 % of the EWA samples and at most 0.31 % of scale, both
    capped (LI_SLACK_SHARE_CAP, where it is said why that is 10 % and not the lookups' 2 %); the bound asserted here and
    on the device is 4 x that (other seeds and configurations), and must stay under 2e-3 of scale, beyond which a wrong
    weight index or a lost `+ 1` would pass."""
    assert 0 < LI_BOUND <= LI_CAP
    case = LiCase(workdir, binding, axis, filt)
    pfilm = oracle_film_positions(oracle, case.scene, case.px, case.py, case.k)
    L, _ = oracle.li(case.scene, case.px, case.py, case.k)
    dist, n, share, worst = case.distance(L, pfilm)
    print(f"Li {case.name}: oracle to truth {dist:.3g} of scale over {n} samples; slack on {share:.2%}, largest {worst:.3g} of scale")
    assert dist <= LI_BOUND, f"{case.name}: {dist:.3g} of scale"
