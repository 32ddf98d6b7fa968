"""Disks and cylinders through the loader (CPU): Shape "disk" / "cylinder" with their parameters and the constructors' clamps
(shapes/disk.cpp:140-150, shapes/cylinder.cpp:223-233), their world bounds in the BVH, area lights on them, orientation flags."""
import numpy as np
import pytest

from quadric_ref import Cylinder, Disk, matrix_text, rotate, scale, translate, world_bound, write_scene

MATTE = 'Material "matte" "rgb Kd" [0.5 0.5 0.5]\n'


def _only_quadric(binding, tmp_path, shape_line, xform=""):
    path = write_scene(tmp_path, MATTE + "AttributeBegin\n" + xform + "\n" + shape_line + "\nAttributeEnd\n")
    return binding.HostScene(path=path)


def test_disk_and_cylinder_defaults(binding, tmp_path):
    s = _only_quadric(binding, tmp_path, 'Shape "disk"')
    assert s.quadric_count == 1 and s.info["n_prims"] == 1 and s.info["n_triangles"] == 0 and s.info["n_spheres"] == 0
    q = s.quadric(0)
    assert q.kind == binding.QUADRIC_DISK
    assert (q.height, q.radius, q.inner_radius) == (0.0, 1.0, 0.0)
    assert q.phi_max == pytest.approx(2 * np.pi, rel=1e-6)
    s = _only_quadric(binding, tmp_path, 'Shape "cylinder"')
    q = s.quadric(0)
    assert q.kind == binding.QUADRIC_CYLINDER
    assert (q.radius, q.zmin, q.zmax) == (1.0, -1.0, 1.0)
    assert q.phi_max == pytest.approx(2 * np.pi, rel=1e-6)
    assert s.prim_flags()[0] & binding.PRIM_QUADRIC and not s.prim_flags()[0] & binding.PRIM_SPHERE


def test_explicit_parameters_and_clamps(binding, tmp_path):
    s = _only_quadric(binding, tmp_path, 'Shape "disk" "float height" [0.25] "float radius" [2] "float innerradius" [0.5] '
                                         '"float phimax" [400]')
    q = s.quadric(0)
    assert (q.height, q.radius, q.inner_radius) == (0.25, 2.0, 0.5)
    assert q.phi_max == pytest.approx(2 * np.pi, rel=1e-6)  # Radians(Clamp(phimax, 0, 360))
    s = _only_quadric(binding, tmp_path, 'Shape "cylinder" "float radius" [0.5] "float zmin" [3] "float zmax" [-2] "float phimax" [90]')
    q = s.quadric(0)
    assert (q.radius, q.zmin, q.zmax) == (0.5, -2.0, 3.0)  # zMin / zMax ordered
    assert q.phi_max == pytest.approx(np.pi / 2, rel=1e-6)


def test_counts_in_a_mixed_scene(binding, tmp_path):
    body = MATTE + """Shape "sphere" "float radius" [0.3]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -1 -3  3 -1 -3  3 -1 3  -3 -1 3]
AttributeBegin
Translate 1 0 0
Shape "disk"
Shape "cylinder" "float radius" [0.2]
Shape "disk" "float height" [1]
AttributeEnd
"""
    s = binding.HostScene(path=write_scene(tmp_path, body))
    assert s.quadric_count == 3 and s.info["n_spheres"] == 1 and s.info["n_triangles"] == 2 and s.info["n_prims"] == 6
    flags = s.prim_flags()
    _, _, shape = s.bvh()
    quad = (flags & binding.PRIM_QUADRIC) != 0
    assert quad.sum() == 3 and sorted(shape[quad]) == [0, 1, 2]
    assert ((flags & binding.PRIM_SPHERE) != 0).sum() == 1


@pytest.mark.parametrize("xform", [np.eye(4), translate(1, -2, 3) @ rotate(37, (1, 2, 0.5)) @ scale(2, 0.5, 1.5),
                                   rotate(-75, (0, 1, 1)) @ scale(1, 3, 0.25)])
def test_root_bounds_are_the_transformed_object_bounds(binding, tmp_path, xform):
    for line, shape in (('Shape "disk" "float height" [0.5] "float radius" [1.5] "float innerradius" [0.5] "float phimax" [120]',
                         Disk(xform, 0.5, 1.5, 0.5, 120)),
                        ('Shape "cylinder" "float radius" [0.75] "float zmin" [-0.5] "float zmax" [2]', Cylinder(xform, 0.75, -0.5, 2))):
        s = _only_quadric(binding, tmp_path, line, matrix_text(xform))
        nodes, _, _ = s.bvh()
        lo, hi = world_bound(xform, *shape.object_bound())
        tol = 1e-5 * (1 + np.abs(np.concatenate([lo, hi])).max())
        assert np.allclose(nodes[0]["bmin"], lo, atol=tol) and np.allclose(nodes[0]["bmax"], hi, atol=tol), (line, nodes[0], lo, hi)


def test_area_lights_on_quadrics(binding, tmp_path):
    body = MATTE + """AttributeBegin
AreaLightSource "diffuse" "rgb L" [2 3 4] "rgb scale" [0.5 0.5 0.5] "bool twosided" "true" "integer samples" [4]
Shape "disk" "float radius" [0.5]
AttributeEnd
AttributeBegin
AreaLightSource "diffuse" "rgb L" [1 1 1]
Shape "cylinder" "float radius" [0.25]
AttributeEnd
Shape "sphere" "float radius" [0.1]
"""
    s = binding.HostScene(path=write_scene(tmp_path, body))
    assert s.info["n_lights"] == 2
    flags = s.prim_flags()
    _, _, shape = s.bvh()
    for i, (two_sided, n_samples, lemit, kind) in enumerate(((1, 4, (1.0, 1.5, 2.0), binding.QUADRIC_DISK),
                                                              (0, 1, (1.0, 1.0, 1.0), binding.QUADRIC_CYLINDER))):
        lt = s.light(i)
        assert lt.type == binding.LIGHT_AREA_QUADRIC and lt.sphere == -1
        assert (lt.two_sided, lt.n_samples, tuple(lt.lemit)) == (two_sided, n_samples, lemit)
        assert 0 <= lt.prim < s.info["n_prims"] and flags[lt.prim] & binding.PRIM_QUADRIC
        assert s.quadric(int(shape[lt.prim])).kind == kind


def test_orientation_flags(binding, tmp_path):
    s = _only_quadric(binding, tmp_path, 'ReverseOrientation\nShape "disk"')
    q = s.quadric(0)
    assert (q.reverse_orientation, q.swaps_handedness) == (1, 0) and s.prim_flags()[0] & binding.PRIM_FLIP
    s = _only_quadric(binding, tmp_path, 'Shape "cylinder"', "Scale 1 1 -1")
    q = s.quadric(0)
    assert (q.reverse_orientation, q.swaps_handedness) == (0, 1) and s.prim_flags()[0] & binding.PRIM_FLIP
    s = _only_quadric(binding, tmp_path, 'ReverseOrientation\nShape "cylinder"', "Scale 1 1 -1")
    q = s.quadric(0)
    assert (q.reverse_orientation, q.swaps_handedness) == (1, 1) and not s.prim_flags()[0] & binding.PRIM_FLIP
    s = _only_quadric(binding, tmp_path, 'Shape "disk"', "Rotate 180 1 0 0")
    assert (s.quadric(0).reverse_orientation, s.quadric(0).swaps_handedness) == (0, 0)


@pytest.mark.parametrize("name", ["cone", "paraboloid", "hyperboloid", "curve", "heightfield", "nurbs"])
def test_other_quadrics_still_refused(binding, tmp_path, name):
    with pytest.raises(RuntimeError, match=f'Shape "{name}" is not supported .*disk, cylinder'):
        _only_quadric(binding, tmp_path, f'Shape "{name}"')
