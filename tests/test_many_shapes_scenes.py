"""More than 8 spheres, 64 materials and 1 024 disks or cylinders on the host (no GPU): the loader's counts and material indices,
and iile_scene_create's refusal pass, which takes such descriptors on a machine without a device (the idiom of
test_scene_refusals.py: a Sobol' table of no dimensions is refused last, so that message means every earlier check passed)."""
import numpy as np
import pytest

import many_shapes_scenes as MS
from test_scene_refusals import Desc

# (a, b, c, count): spheres; the room's own material comes on top
ROOMS = {"9_spheres": (3, 3, 1, None), "72_spheres": MS.ROOM_72 + (None,), "65_materials": (4, 4, 4, None), "300_materials": (7, 7, 7, 299)}


def _room(binding, tmp_path, key):
    a, b, c, count = ROOMS[key]
    return binding.HostScene(path=MS.room_file(tmp_path, a, b, c, count))


@pytest.mark.parametrize("key", list(ROOMS))
def test_counts_and_material_indices(binding, tmp_path, key):
    a, b, c, count = ROOMS[key]
    n = count if count is not None else a * b * c
    assert n + 1 == {"9_spheres": 10, "72_spheres": 73, "65_materials": 65, "300_materials": 300}[key]
    host = _room(binding, tmp_path, key)
    assert host.info["n_spheres"] == n and host.info["n_materials"] == n + 1 and host.info["n_triangles"] == 10
    assert host.info["n_lights"] == 1 + sum(1 for j in (1, 4, 8) if j < n)
    d = host.scene_desc()
    assert d.n_spheres == n and d.n_materials == n + 1 and d.n_prims == n + 10
    import ctypes
    prim_material = np.frombuffer(ctypes.string_at(d.prim_material, d.n_prims * 4), dtype=np.int32)
    flags, (_, _, shape) = host.prim_flags(), host.bvh()
    is_sphere = (flags & binding.PRIM_SPHERE) != 0
    assert is_sphere.sum() == n and sorted(shape[is_sphere]) == list(range(n))
    assert (prim_material[~is_sphere] == 0).all()
    # sphere j was declared j-th, under the (j + 1)-th Material directive, whose own value no other material has
    assert np.array_equal(prim_material[is_sphere], shape[is_sphere] + 1)
    kinds = dict(matte=binding.MAT_MATTE, plastic=binding.MAT_PLASTIC, mirror=binding.MAT_MIRROR, glass=binding.MAT_GLASS,
                 metal=binding.MAT_METAL, uber=binding.MAT_UBER, substrate=binding.MAT_SUBSTRATE)
    seen = set()
    for j in range(n):
        _, field, value = MS.material(j)
        m = host.material(j + 1)
        assert m.type == kinds[MS.KINDS[j % len(MS.KINDS)]], j
        assert np.float32(getattr(m, field)[0]) == value, (j, field)
        seen.add(float(value))
    assert len(seen) == n and tuple(host.material(0).kd) == tuple(np.float32([0.6, 0.6, 0.6]))


def _passes_the_refusal_pass(binding, host):
    desc = Desc(binding, host)
    desc.d.sobol.enabled = 1  # (a Sobol' table of no dimensions: refused last)
    rc, msg = desc.create()
    assert rc != 0 and msg.startswith("iile_sobol: bad dimension count"), msg


@pytest.mark.parametrize("key", list(ROOMS))
def test_refusal_pass_takes_many_spheres_and_materials(binding, tmp_path, key):
    _passes_the_refusal_pass(binding, _room(binding, tmp_path, key))


def test_refusal_pass_takes_8_spheres_and_64_materials(binding, tmp_path):
    """The most the device took before: accepted then and now."""
    host = binding.HostScene(path=MS.room_file(tmp_path, *MS.ROOM_8, extra_materials=55))
    assert host.info["n_spheres"] == 8 and host.info["n_materials"] == 64 and host.info["n_triangles"] == 65
    assert tuple(host.material(63).kd)[0] == MS.tint(8 + 54)
    _passes_the_refusal_pass(binding, host)


def test_1025_disks_load_and_pass(binding, tmp_path):
    body, disks = MS.disk_field(1025)
    host = binding.HostScene(path=MS.write(tmp_path, body, name="disks_1025.pbrt"))
    assert len(disks) == 1025 and host.quadric_count == 1025 and host.info["n_prims"] == 1025
    assert host.quadric(1024).kind == binding.QUADRIC_DISK and host.quadric(1024).radius == np.float32(0.1)
    _passes_the_refusal_pass(binding, host)
