"""Procedural textures on the device: the texture probe against tests/texture_ref.py (a float32 restatement of src/core/texture.cpp
and src/textures/*.h), film identities that must hold bit for bit on every render path, point-light radiance on a textured quad, a
planar-mapped bump map, and a float bilerp as plastic roughness."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import texture_ref as T
from quadric_ref import write_scene

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0  1 -1 0  1 1 0  -1 1 0] "float uv" [0 0 1 0 1 1 0 1]\n'
N = 100_000
# Points closer than this to a check edge or a mapping seam (in the texture's (s, t) or 3D units, and for the closed form also
# the filter box's sides) are left out of the comparison: there a one-ulp difference of the angle of a spherical or cylindrical
# mapping may flip the selection.
MARGIN = 1e-4
XF = "Translate 0.3 -0.2 0.1\nRotate 30 1 1 0\nScale 0.5 0.7 0.5\n"

# name -> Texture directive (after the transform XF): every class x mapping x aamode the device implements
LEAVES = {}
for _m, _extra in (("uv", '"float uscale" [3] "float vscale" [2] "float udelta" [0.25] "float vdelta" [-0.5]'),
                   ("spherical", ""), ("cylindrical", ""),
                   ("planar", '"vector v1" [1 0.5 0] "vector v2" [0 0.25 1] "float udelta" [0.1] "float vdelta" [0.2]')):
    for _aa in ("none", "closedform"):
        LEAVES[f"ck_{_m}_{_aa}"] = (f'"spectrum" "checkerboard" "string mapping" "{_m}" {_extra} "string aamode" "{_aa}" '
                                    '"rgb tex1" [0.9 0.6 0.3] "rgb tex2" [0.1 0.2 0.4]')
    LEAVES[f"uv_{_m}"] = f'"spectrum" "uv" "string mapping" "{_m}" {_extra}'
    LEAVES[f"bl_{_m}"] = f'"spectrum" "bilerp" "string mapping" "{_m}" {_extra} "rgb v00" [0.1 0.2 0.3] "rgb v10" [0.9 0.1 0.5] "rgb v11" [0.4 0.4 0.8]'
    LEAVES[f"fbl_{_m}"] = f'"float" "bilerp" "string mapping" "{_m}" {_extra} "float v00" [0.2] "float v11" [0.7]'
LEAVES["ck3d"] = '"spectrum" "checkerboard" "integer dimension" [3] "rgb tex1" [0.9 0.6 0.3] "rgb tex2" [0.1 0.2 0.4]'
LEAVES["fck_planar"] = '"float" "checkerboard" "string mapping" "planar" "float tex1" [0.25] "float tex2" [0.75]'
COMBINERS = {
    "scale_bl_uv": '"spectrum" "scale" "texture tex1" "bl_planar" "texture tex2" "uv_uv"',
    "mix_amount_tex": '"spectrum" "mix" "texture tex1" "uv_cylindrical" "texture tex2" "bl_uv" "texture amount" "fck_planar"',
    "mix_amount_bilerp": '"spectrum" "mix" "texture tex1" "ck_uv_none" "texture tex2" "bl_spherical" "texture amount" "fbl_planar"',
    "ck_of_leaves_none": '"spectrum" "checkerboard" "string mapping" "planar" "string aamode" "none" "texture tex1" "uv_uv" "texture tex2" "bl_planar"',
    "ck_of_leaves_closed": '"spectrum" "checkerboard" "string aamode" "closedform" "texture tex1" "uv_planar" "texture tex2" "rgb tex2" [0.5 0.5 0.5]',
    "ck3d_of_leaves": '"spectrum" "checkerboard" "integer dimension" [3] "texture tex1" "bl_cylindrical" "texture tex2" "uv_uv"',
    "fscale": '"float" "scale" "texture tex1" "fbl_uv" "texture tex2" "fck_planar"',
}
COMBINERS["ck_of_leaves_closed"] = COMBINERS["ck_of_leaves_closed"].replace(' "texture tex2" "rgb tex2"', ' "rgb tex2"')


@pytest.fixture(scope="module")
def catalogue(binding, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("catalogue")
    body = "TransformBegin\n" + XF
    names = []
    for name, decl in list(LEAVES.items()) + list(COMBINERS.items()):
        body += f'Texture "{name}" {decl}\n'
        names.append(name)
    body += 'TransformEnd\nMaterial "matte" "texture Kd" "scale_bl_uv"\nLightSource "point" "rgb I" [1 1 1] "point from" [0 0 3]\n' + QUAD
    host = binding.HostScene(path=write_scene(tmp, body))
    gpu = binding.GpuScene(host)
    texs = [host.procedural_texture(i) for i in range(len(names))]  # every declaration above makes one entry, in order
    yield dict(zip(names, range(len(names)))), texs, gpu
    gpu.close()


def _points(seed):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-3, 3, (N, 2)).astype(np.float32)
    duv = (rng.normal(0, 0.05, (N, 4)) * rng.uniform(0, 1, (N, 1)) ** 3).astype(np.float32)
    p = rng.uniform(-2, 2, (N, 3)).astype(np.float32)
    dpdx = (rng.normal(0, 0.05, (N, 3)) * rng.uniform(0, 1, (N, 1)) ** 3).astype(np.float32)
    dpdy = (rng.normal(0, 0.05, (N, 3)) * rng.uniform(0, 1, (N, 1)) ** 3).astype(np.float32)
    return uv, duv, p, dpdx, dpdy


def _far_from_edges(texs, t, args):
    """True where the point is MARGIN or more from every check edge / seam of t and of the checkerboards among its inputs."""
    ok = np.ones(N, bool)
    for u in [t] + [texs[c] for c in t["child"] if c >= 0 and t["kind"] != T.TEX_IMAGE]:
        if u["kind"] in (T.TEX_CHECKER2D, T.TEX_CHECKER3D) or u["mapping"] in (T.MAP_SPHERICAL, T.MAP_CYLINDRICAL):
            ok &= T.edge_distance(u, *args) >= MARGIN
    return ok


def _pure_selection(texs, t, args):
    """Where the result is a pure selection among constants: a checkerboard of constants with aamode none, a 3D checkerboard, or
    a closed form whose filter box stays inside one check."""
    if t["kind"] not in (T.TEX_CHECKER2D, T.TEX_CHECKER3D) or any(c >= 0 for c in t["child"][:2]):
        return np.zeros(N, bool)
    return T.checker(t, *args)[2]


@pytest.mark.parametrize("name", list(LEAVES) + list(COMBINERS))
def test_probe_matches_restatement(catalogue, name):
    idx, texs, gpu = catalogue
    t = texs[idx[name]]
    args = _points(idx[name])
    got = gpu.texture_eval_p(idx[name], *args)
    want = T.evaluate(texs, idx[name], *args)
    ok = _far_from_edges(texs, t, args)
    assert ok.mean() > 0.9, ok.mean()
    pure = _pure_selection(texs, t, args) & ok
    if pure.any():  # a selection: bit for bit
        assert np.array_equal(got[pure].view(np.uint32), want[pure].view(np.uint32)), name
    rest = ok & ~pure
    trig = t["mapping"] in (T.MAP_SPHERICAL, T.MAP_CYLINDRICAL) or any(
        texs[c]["mapping"] in (T.MAP_SPHERICAL, T.MAP_CYLINDRICAL) for c in t["child"] if c >= 0)
    if not trig:  # the same float32 operations in the same order: bit for bit as well
        assert np.array_equal(got[rest].view(np.uint32), want[rest].view(np.uint32)), (name, np.abs(got[rest] - want[rest]).max())
    elif rest.any():  # acos / atan2 may differ by an ulp of the angle; the closed form's finite differences amplify it by 1 / delta
        closed = t["kind"] == T.TEX_CHECKER2D and t["aamode"] == T.AA_CLOSEDFORM
        atol = 1e-3 if closed else 4e-7
        err = np.abs(got[rest].astype(np.float64) - want[rest])
        assert np.all(err <= atol + 4 * 1.2e-7 * np.abs(want[rest])), (name, err.max())
        assert np.mean(err == 0) > 0.9, (name, np.mean(err == 0))


def test_probe_image_path_unchanged(binding, tmp_path):
    """iile_texture_eval and the new probe agree bit for bit on an image (the image path takes the same instructions)."""
    rng = np.random.default_rng(1)
    _write_pfm(tmp_path / "a.pfm", rng.random((16, 16, 3)).astype(np.float32))
    host = binding.HostScene(path=write_scene(tmp_path, 'Texture "a" "spectrum" "imagemap" "string filename" ["a.pfm"]\n'
                                                        'Material "matte" "texture Kd" "a"\nLightSource "point" "point from" [0 0 3]\n' + QUAD))
    gpu = binding.GpuScene(host)
    uv, duv, p, dpdx, dpdy = _points(2)
    a = gpu.texture_eval(0, uv, duv)
    b = gpu.texture_eval_p(0, uv, duv, p, dpdx, dpdy)
    gpu.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))



IMAGE_COMBINERS = {
    "scale_images": '"spectrum" "scale" "texture tex1" "ia" "texture tex2" "ib"',
    "mix_images_bilerp_amount": '"spectrum" "mix" "texture tex1" "ia" "texture tex2" "ib" "texture amount" "fbl"',
    "mix_image_float_image_amount": '"spectrum" "mix" "texture tex1" "ia" "rgb tex2" [0.2 0.9 0.4] "texture amount" "fa"',
    "ck_image_bilerp_none": '"spectrum" "checkerboard" "string aamode" "none" "float uscale" [4] "float vscale" [3] "texture tex1" "ia" "texture tex2" "bl"',
    "ck_images_closed": '"spectrum" "checkerboard" "string mapping" "planar" "texture tex1" "ia" "texture tex2" "ib"',
    "ck3d_image_const": '"spectrum" "checkerboard" "integer dimension" [3] "texture tex1" "ib" "rgb tex2" [0.3 0.3 0.3]',
    "fscale_image_ck": '"float" "scale" "texture tex1" "fa" "texture tex2" "fck"',
}


@pytest.fixture(scope="module")
def image_catalogue(binding, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("image_catalogue")
    rng = np.random.default_rng(11)
    for n in ("ia", "ib", "fa"):
        _write_pfm(tmp / f"{n}.pfm", rng.random((16, 16, 3)).astype(np.float32))
    decls = [("ia", '"spectrum" "imagemap" "string filename" ["ia.pfm"]'), ("ib", '"spectrum" "imagemap" "string filename" ["ib.pfm"]'),
             ("fa", '"float" "imagemap" "string filename" ["fa.pfm"]'),
             ("fbl", '"float" "bilerp" "string mapping" "planar" "float v00" [0.1] "float v11" [0.9]'),
             ("bl", '"spectrum" "bilerp" "rgb v00" [0.1 0.2 0.3] "rgb v10" [0.9 0.1 0.5] "rgb v11" [0.4 0.4 0.8]'),
             ("fck", '"float" "checkerboard" "string mapping" "planar" "float tex1" [0.25] "float tex2" [0.75]')]
    decls += list(IMAGE_COMBINERS.items())
    body = "TransformBegin\n" + XF + "".join(f'Texture "{n}" {d}\n' for n, d in decls) + "TransformEnd\n"
    body += 'Material "matte" "texture Kd" "scale_images"\nLightSource "point" "rgb I" [1 1 1] "point from" [0 0 3]\n' + QUAD
    host = binding.HostScene(path=write_scene(tmp, body))
    gpu = binding.GpuScene(host)
    texs = [host.procedural_texture(i) for i in range(len(decls))]  # every declaration above makes one entry, in order
    assert [t["kind"] for t in texs[:3]] == [T.TEX_IMAGE] * 3
    # the image leaves' values: ImageTexture::Evaluate through iile_texture_eval, the image path as it was before this change
    images = {i: (lambda uv, duv, i=i: gpu.texture_eval(i, uv, duv)) for i in range(3)}
    yield {n: i for i, (n, _) in enumerate(decls)}, texs, images, gpu
    gpu.close()


@pytest.mark.parametrize("name", list(IMAGE_COMBINERS))
def test_probe_image_leaves_in_combiners(image_catalogue, name):
    """Combiners over image leaves against the restatement, the image leaves looked up through the unchanged image path: no
    spherical or cylindrical mapping here, so the same float32 operations in the same order, bit for bit (points within MARGIN of
    a check edge left out)."""
    idx, texs, images, gpu = image_catalogue
    t = texs[idx[name]]
    args = _points(100 + idx[name])
    got = gpu.texture_eval_p(idx[name], *args)
    want = T.evaluate(texs, idx[name], *args, images=images)
    ok = _far_from_edges(texs, t, args)
    assert ok.mean() > 0.9, ok.mean()
    assert want[ok].max() > 0
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (name, np.abs(got[ok] - want[ok]).max())

# ---- film identities ------------------------------------------------------------------------------------------------------------
def _write_pfm(path, rows):
    h, w, _ = rows.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


ROOM = ('LightSource "point" "rgb I" [8 8 8] "point from" [0.3 -0.5 1.5]\nLightSource "infinite" "rgb L" [0.1 0.1 0.15]\n'
        'AttributeBegin\nMaterial "matte" "texture Kd" "KD"\n'
        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -3 0  3 -3 0  3 3 0  -3 3 0] "float uv" [0 0 2 0 2 2 0 2]\n'
        'AttributeEnd\nAttributeBegin\nMaterial "plastic" "texture Kd" "KD" "float roughness" [0.2]\nTranslate 0 0 0.6\n'
        'Shape "sphere" "float radius" [0.5]\nAttributeEnd\n')
IDENTITIES = {
    "image": 'Texture "KD" "spectrum" "scale" "texture tex1" "ia" "rgb tex2" [1 1 1]\n',
    "checker_same_image": 'Texture "KD" "spectrum" "checkerboard" "string aamode" "none" "texture tex1" "ia" "texture tex2" "ia"\n',
    "mix_amount_0": 'Texture "KD" "spectrum" "mix" "texture tex1" "ia" "texture tex2" "ib" "float amount" [0]\n',
}


def _identity_scene(tmp_path, which, integrator="path", spp=2):
    rng = np.random.default_rng(7)
    _write_pfm(tmp_path / "ia.pfm", rng.random((32, 32, 3)).astype(np.float32))
    _write_pfm(tmp_path / "ib.pfm", rng.random((32, 32, 3)).astype(np.float32))
    body = ('Texture "ia" "spectrum" "imagemap" "string filename" ["ia.pfm"]\nTexture "ib" "spectrum" "imagemap" "string filename" ["ib.pfm"]\n'
            + IDENTITIES[which] + ROOM)
    return write_scene(tmp_path, body, name=f"{which}_{integrator}.pbrt", w=32, h=32, spp=spp, depth=3, fov=50, eye="0 -4 2",
                       look="0 0 0.3", up="0 0 1", integrator=integrator)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("which", ["checker_same_image", "mix_amount_0"])
@pytest.mark.parametrize("stats", [False, True])
def test_identity_path_integrator(binding, tmp_path, which, stats):
    """The path integrator: the textured build, and the build that also counts statistics."""
    films = []
    for w in ("image", which):
        host = binding.HostScene(path=_identity_scene(tmp_path, w))
        gpu = binding.GpuScene(host)
        film, _ = gpu.render(collect_stats=stats)
        gpu.close()
        films.append(film)
    assert films[0].max() > 0 and np.array_equal(_bits(films[0]), _bits(films[1]))


@pytest.mark.parametrize("which", ["checker_same_image", "mix_amount_0"])
def test_identity_direct_pass(binding, tmp_path, which):
    films = []
    for w in ("image", which):
        host = binding.HostScene(path=_identity_scene(tmp_path, w, integrator="iispt"))
        gpu = binding.GpuScene(host)
        films.append(gpu.render_direct(4))
        gpu.close()
    assert films[0].max() > 0 and np.array_equal(films[0], films[1])


@pytest.mark.parametrize("which", ["checker_same_image", "mix_amount_0"])
def test_identity_iispt_frame(binding, tmp_path, which):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    sys.path.insert(0, REPO)
    nn_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_nn")
    frame_mod = importlib.import_module("pbrt-v3-iile_amd.iispt_frame")
    import iispt_torch_reference as ref_mod
    images = []
    for w in ("image", which):
        host = binding.HostScene(path=_identity_scene(tmp_path, w, integrator="iispt", spp=1))
        torch.manual_seed(5)
        gpu = binding.GpuScene(host)
        frame = frame_mod.IisptFrame(binding, gpu, nn_mod.IisptPipeline(gpu, net=ref_mod.IISPTNet().eval()))
        frame.run_batched(4, radius_start=8.0)
        frame.run_direct(4)
        torch.cuda.synchronize()
        images.append(frame.image().cpu().numpy())
        gpu.close()
    assert images[0].max() > 0 and np.array_equal(_bits(images[0]), _bits(images[1]))


@pytest.mark.parametrize("which", ["checker_same_image", "mix_amount_0"])
@pytest.mark.parametrize("integrator", ["path", "iispt"])
def test_identity_cli(binding, tmp_path, which, integrator):
    """`iile_pbrt` under both integrators (iispt: with a fixed random network)."""
    exe = os.path.join(REPO, "pbrt-v3-iile_amd", "lib", "iile_pbrt")
    extra = []
    if integrator == "iispt":
        torch = pytest.importorskip("torch")
        import iispt_torch_reference as ref_mod
        torch.manual_seed(3)
        module = ref_mod.IISPTNet().eval()
        net_file = tmp_path / "net.iilenet"
        binding.save_net_weights(module.state_dict(), str(net_file), bn_eps=module.encoder1[3].eps)
        extra = [f"--iisptNet={net_file}", "--iileIndirect=2", "--iileDirect=2"]
    out = []
    for w in ("image", which):
        path = _identity_scene(tmp_path, w, integrator=integrator, spp=1)
        f = tmp_path / f"{w}_{integrator}.pfm"
        env = dict(os.environ, IISPT_SCHEDULE_RADIUS_START="8")
        p = subprocess.run([exe, path, "--outfile", str(f)] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=600, env=env)
        assert p.returncode == 0, p.stdout
        out.append(f.read_bytes())
    assert out[0] == out[1]


# ---- radiance on a lit quad -----------------------------------------------------------------------------------------------------
RES, EYE, LIGHT, INTENSITY = 16, np.array([0.0, -3.0, 2.0]), np.array([0.8, 1.0, 3.0]), np.array([20.0, 15.0, 10.0])
PLANE = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-4 -4 0  4 -4 0  4 4 0  -4 4 0] "float uv" [0 0 1 0 1 1 0 1]\n'


def _lit(tmp_path, body, name):
    hdr = (f'LookAt {EYE[0]} {EYE[1]} {EYE[2]}  0 0 0  0 0 1\nCamera "perspective" "float fov" [30]\n'
           f'Film "image" "integer xresolution" [{RES}] "integer yresolution" [{RES}] "string filename" "lit.exr"\nPixelFilter "box"\n'
           'Sampler "halton" "integer pixelsamples" [1] "bool samplepixelcenter" "true"\nIntegrator "path" "integer maxdepth" [1]\nWorldBegin\n')
    p = tmp_path / name
    p.write_text(hdr + f'LightSource "point" "rgb I" [{INTENSITY[0]} {INTENSITY[1]} {INTENSITY[2]}] "point from" [{LIGHT[0]} {LIGHT[1]} {LIGHT[2]}]\n'
                 + body + PLANE + "WorldEnd\n")
    return str(p)


def _hits(gpu):
    px, py = np.meshgrid(np.arange(RES), np.arange(RES))
    px, py = px.reshape(-1), py.reshape(-1)
    L, _ = gpu.li_samples(px, py, np.zeros_like(px))
    o, d = gpu.camera_rays(np.stack([px + 0.5, py + 0.5], 1))
    o, d = o.astype(np.float64), d.astype(np.float64)
    p = o + (-o[:, 2] / d[:, 2])[:, None] * d
    to_l = LIGHT[None, :] - p
    r2 = (to_l ** 2).sum(1)
    wi = to_l / np.sqrt(r2)[:, None]
    return L, p, wi, r2


@pytest.mark.parametrize("tex", ["ck_uv_none", "ck_spherical_none", "ck_cylindrical_none", "ck_planar_none", "ck3d",
                                 "uv_uv", "uv_spherical", "uv_cylindrical", "uv_planar", "bl_uv", "bl_spherical", "bl_cylindrical", "bl_planar"])
def test_point_light_matte_quad(binding, tmp_path, tex):
    """Lambertian Kd(p) / pi * I |cos| / r^2 at the quad point each pixel centre sees, Kd from the restatement."""
    body = "TransformBegin\n" + XF + f'Texture "K" {LEAVES[tex]}\nTransformEnd\nMaterial "matte" "texture Kd" "K"\n'
    host = binding.HostScene(path=_lit(tmp_path, body, f"{tex}.pbrt"))
    gpu = binding.GpuScene(host)
    L, p, wi, r2 = _hits(gpu)
    gpu.close()
    t = host.procedural_texture(0)
    n = len(p)
    pf = p.astype(np.float32)
    uv = ((pf[:, :2] + np.float32(4)) / np.float32(8)).astype(np.float32)
    z3, z4 = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
    kd = np.maximum(T.evaluate([t], 0, uv, z4, pf, z3, z3).astype(np.float64), 0)  # Kd->Evaluate(*si).Clamp(), matte.cpp:54
    want = kd / np.pi * INTENSITY[None, :] * np.abs(wi[:, 2:3]) / r2[:, None]
    ok = T.edge_distance(t, uv, z4, pf, z3, z3) >= 1e-3 if (t["kind"] != T.TEX_BILERP or t["mapping"] != T.MAP_UV) else np.ones(n, bool)
    assert ok.mean() > 0.8 and want[ok].max() > 0
    assert np.allclose(L[ok], want[ok], rtol=2e-3, atol=1e-5 * want.max()), np.abs(L[ok] - want[ok]).max()


def test_bump_planar_shifts_p(binding, tmp_path):
    """A planar-mapped float bilerp displacement d = s = x (v10 = v11 = 1): Material::Bump evaluates it at p + du * dpdu, so
    d(u + du) - d(u) = 8 du: dpdu' = dpdu + 8 n = (8, 0, 8), and the shading normal tilts to (-1, 0, 1) / sqrt 2 (dpdu = (8, 0, 0),
    dpdv = (0, 8, 0)). Were p not shifted, the displacement would not change with u and the normal would stay (0, 0, 1)."""
    body = ('Texture "d" "float" "bilerp" "string mapping" "planar" "float v00" [0] "float v01" [0] "float v10" [1] "float v11" [1]\n'
            'Material "matte" "rgb Kd" [0.5 0.5 0.5] "texture bumpmap" "d"\n')
    host = binding.HostScene(path=_lit(tmp_path, body, "bump.pbrt"))
    gpu = binding.GpuScene(host)
    L, p, wi, r2 = _hits(gpu)
    gpu.close()
    ns = np.array([-1.0, 0.0, 1.0]) / np.sqrt(2.0)
    want = 0.5 / np.pi * INTENSITY[None, :] * np.abs(wi @ ns)[:, None] / r2[:, None]
    flat = 0.5 / np.pi * INTENSITY[None, :] * np.abs(wi[:, 2:3]) / r2[:, None]
    assert not np.allclose(want, flat, rtol=1e-2)
    assert np.allclose(L, want, rtol=2e-3, atol=1e-5 * want.max()), np.abs(L - want).max()


def test_float_bilerp_as_plastic_roughness(binding, tmp_path):
    """A constant-valued float bilerp as "roughness" renders the film of the constant roughness (to float rounding of the alpha the
    device computes at the hit), and a varying one renders finite."""
    def render(body, name):
        host = binding.HostScene(path=_lit(tmp_path, body, name))
        gpu = binding.GpuScene(host)
        film, _ = gpu.render()
        gpu.close()
        return host.film_to_rgb(film).astype(np.float64)
    a = render('Material "plastic" "float roughness" [0.3]\n', "plain.pbrt")
    b = render('Texture "r" "float" "bilerp" "float v00" [0.3] "float v01" [0.3] "float v10" [0.3] "float v11" [0.3]\n'
               'Material "plastic" "texture roughness" "r"\n', "bl.pbrt")
    c = render('Texture "r" "float" "bilerp" "string mapping" "planar" "float v00" [0.05] "float v11" [0.5]\n'
               'Material "plastic" "texture roughness" "r"\n', "blv.pbrt")
    assert a.max() > 0 and np.allclose(a, b, rtol=1e-5, atol=1e-6 * a.max()), np.abs(a - b).max()
    assert np.isfinite(c).all() and c.max() > 0 and not np.allclose(a, c, rtol=1e-3)
