"""`ActiveTransform` / `TransformTimes` and the moving camera in the scene loader (CPU): which transform the directives move, what
the attribute stack and the named coordinate systems keep, what a light, a texture and a shape under an animated transform get,
and the decomposition the host hands the device, held to the float64 polar decomposition of camera_motion_ref.py."""
import ctypes

import numpy as np
import pytest

import camera_motion_cases as CC
import camera_motion_ref as CM

WARNING = 'Animated transformations set; ignoring for "%s" and using the start transform only'
POINT_LIGHT = 'LightSource "point" "rgb I" [1 1 1] "point from" [0 0 0]\n'


def load(binding, tmp_path, text, name="motion.pbrt"):
    path = tmp_path / name
    path.write_text(text)
    return binding.HostScene(path=str(path))


def _bits(a):
    return np.ascontiguousarray(np.array(a, np.float32)).view(np.uint32)


def _c2w(host):
    return _bits(host.camera()[1].camera_to_world)


def _masked(struct):
    """The bytes of a ctypes struct with every pointer member zeroed (two loads of one file keep their tables at different addresses)."""
    raw = bytearray(ctypes.string_at(ctypes.addressof(struct), ctypes.sizeof(struct)))

    def walk(tp, base):
        for name, ft in tp._fields_:
            off = base + getattr(tp, name).offset
            if isinstance(ft, type) and issubclass(ft, ctypes.Structure):
                walk(ft, off)
            elif isinstance(ft, type) and issubclass(ft, ctypes.Array) and issubclass(ft._type_, ctypes.Structure):
                for i in range(ft._length_):
                    walk(ft._type_, off + i * ctypes.sizeof(ft._type_))
            elif ft is ctypes.c_void_p or (isinstance(ft, type) and issubclass(ft, ctypes._Pointer)):
                raw[off:off + ctypes.sizeof(ft)] = bytes(ctypes.sizeof(ft))
    walk(type(struct), 0)
    return bytes(raw)


# ---- directive semantics ------------------------------------------------------------------------------------------------------------
def test_end_time_directives_move_the_end_transform_alone(binding, tmp_path):
    moving = load(binding, tmp_path, CC.scene_text(CC.camera_block("Translate 0.5 -0.25 1")), "moving.pbrt")
    start = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT), "start.pbrt")
    end = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT + "\nTranslate 0.5 -0.25 1"), "end.pbrt")
    mo = moving.camera_motion
    assert mo is not None and start.camera_motion is None and end.camera_motion is None
    assert np.array_equal(_c2w(moving), _c2w(start))
    assert np.array_equal(_bits(mo.camera_to_world_end), _c2w(end))
    assert not np.array_equal(_c2w(start), _c2w(end))
    assert (mo.start_time, mo.end_time) == (0.0, 1.0)
    # everything else of the descriptor is the start scene's
    assert _masked(moving.scene_desc()) == _masked(start.scene_desc())


def test_start_time_directives_move_the_start_transform_alone(binding, tmp_path):
    text = f"{CC.BASE_TEXT}\nActiveTransform StartTime\nRotate 30 0 1 0\nActiveTransform All\n"
    moving = load(binding, tmp_path, CC.scene_text(text), "moving.pbrt")
    start = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT + "\nRotate 30 0 1 0"), "start.pbrt")
    end = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT), "end.pbrt")
    assert np.array_equal(_c2w(moving), _c2w(start))
    assert np.array_equal(_bits(moving.camera_motion.camera_to_world_end), _c2w(end))


def test_transform_times(binding, tmp_path, capfd):
    moving = load(binding, tmp_path, CC.scene_text("TransformTimes 0.25 0.75\n" + CC.camera_block("Translate 1 0 0")))
    mo = moving.camera_motion
    assert (mo.start_time, mo.end_time) == (0.25, 0.75)
    # an option: inside the world block it is an error message and ignored (VERIFY_OPTIONS)
    capfd.readouterr()
    inside = load(binding, tmp_path, CC.scene_text(CC.camera_block("Translate 1 0 0"), world="TransformTimes 0.5 0.6\n" + CC.NOTHING), "inside.pbrt")
    err = capfd.readouterr().err
    assert 'Options cannot be set inside world block; "TransformTimes" not allowed.  Ignoring.' in err
    mo = inside.camera_motion
    assert (mo.start_time, mo.end_time) == (0.0, 1.0)


def test_attribute_end_restores_the_active_transforms(binding, tmp_path, capfd):
    """Inside the attribute block the Translate moves the end transform alone; after AttributeEnd both are back and both move: the
    light sits under a transform that is not animated, where the same file without the ActiveTransform line puts it."""
    world = "AttributeBegin\n%sTranslate 5 0 0\nAttributeEnd\nTranslate 1 2 3\n" + POINT_LIGHT + CC.NOTHING
    capfd.readouterr()
    with_bits = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT, world=world % "ActiveTransform EndTime\n"), "a.pbrt")
    err = capfd.readouterr().err
    without = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT, world=world % ""), "b.pbrt")
    assert "Animated transformations" not in err
    assert bytes(with_bits.light(0)) == bytes(without.light(0))
    assert list(with_bits.light(0).pos) == [1.0, 2.0, 3.0]
    # TransformBegin / TransformEnd keep them likewise
    world = "TransformBegin\nActiveTransform EndTime\nTranslate 5 0 0\nTransformEnd\nTranslate 1 2 3\n" + POINT_LIGHT + CC.NOTHING
    capfd.readouterr()
    tb = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT, world=world), "c.pbrt")
    assert "Animated transformations" not in capfd.readouterr().err
    assert bytes(tb.light(0)) == bytes(without.light(0))


def test_coord_sys_transform_restores_a_pair(binding, tmp_path, capfd):
    """`CoordSysTransform "camera"` brings both camera transforms back: the light under it is under an animated transform, warns,
    and sits where the start transform puts it — the camera's start position."""
    world = 'CoordSysTransform "camera"\n' + POINT_LIGHT + "Identity\n" + CC.NOTHING   # (no shape may stand under a moving transform)
    capfd.readouterr()
    moving = load(binding, tmp_path, CC.scene_text(CC.camera_block("Translate 0.5 -0.25 1"), world=world), "moving.pbrt")
    err = capfd.readouterr().err
    static = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT, world=world), "static.pbrt")
    assert WARNING % "LightSource" in err
    assert "Animated transformations" not in capfd.readouterr().err
    assert bytes(moving.light(0)) == bytes(static.light(0))
    assert np.allclose(list(moving.light(0).pos), [1, 2, 3], atol=1e-5)
    # a coordinate system named inside the world keeps its pair too
    world = ('ActiveTransform EndTime\nTranslate 0 9 0\nActiveTransform All\nCoordinateSystem "rig"\nIdentity\nCoordSysTransform "rig"\n'
             + POINT_LIGHT + "Identity\n" + CC.NOTHING)
    capfd.readouterr()
    rig = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT, world=world), "rig.pbrt")
    assert WARNING % "LightSource" in capfd.readouterr().err
    assert list(rig.light(0).pos) == [0.0, 0.0, 0.0]


def test_equal_transforms_are_a_static_scene(binding, tmp_path):
    """Both transforms spelled one after the other, with the same directives: no motion, and the descriptor of the same file
    without the ActiveTransform lines, byte for byte."""
    lines = ["ActiveTransform EndTime", "Identity", CC.BASE_TEXT, "Translate 1 0 0", "ActiveTransform StartTime", "Identity", CC.BASE_TEXT,
             "Translate 1 0 0", "ActiveTransform All", "Scale 1 1 1"]
    spelled = load(binding, tmp_path, CC.scene_text("\n".join(lines)), "spelled.pbrt")
    plain = load(binding, tmp_path, CC.scene_text("\n".join(ln for ln in lines if not ln.startswith("ActiveTransform"))), "plain.pbrt")
    assert spelled.camera_motion is None and plain.camera_motion is None
    assert _masked(spelled.scene_desc()) == _masked(plain.scene_desc())
    assert bytes(spelled.camera()[1]) == bytes(plain.camera()[1])
    rc = binding.host_lib().iile_host_scene_camera_motion(spelled._h, ctypes.byref(binding.CameraMotion()))
    assert rc == 2 and b"does not move" in binding.host_lib().iile_host_last_error()


# ---- warnings and refusals ----------------------------------------------------------------------------------------------------------
ANIMATED_WORLD = "ActiveTransform EndTime\nTranslate 0 0 7\nActiveTransform All\n"


def test_light_and_texture_under_an_animated_transform_keep_the_start_transform(binding, tmp_path, capfd):
    tex = 'Texture "chk" "spectrum" "checkerboard" "integer dimension" [3]\n'
    capfd.readouterr()
    moving = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT, world="Translate 1 2 3\n" + ANIMATED_WORLD + POINT_LIGHT + tex +
                                                   'AttributeBegin\nIdentity\nMaterial "matte" "texture Kd" "chk"\nShape "sphere"\nAttributeEnd\n'),
                  "moving.pbrt")
    err = capfd.readouterr().err
    static = load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT, world="Translate 1 2 3\n" + POINT_LIGHT + tex +
                                                   'AttributeBegin\nIdentity\nMaterial "matte" "texture Kd" "chk"\nShape "sphere"\nAttributeEnd\n'),
                  "static.pbrt")
    assert WARNING % "LightSource" in err and WARNING % "Texture" in err
    assert "Animated transformations" not in capfd.readouterr().err
    assert bytes(moving.light(0)) == bytes(static.light(0)) and list(moving.light(0).pos) == [1.0, 2.0, 3.0]
    n = moving.scene_desc().n_textures
    assert n == static.scene_desc().n_textures and n >= 1
    for i in range(n):
        assert _masked(moving.texture(i)[0]) == _masked(static.texture(i)[0])
    assert moving.camera_motion is None   # the camera itself stands still


@pytest.mark.parametrize("before,shape,rest", [("", "sphere", ""),
                                               ("", "trianglemesh", ' "integer indices" [0 1 2] "point P" [0 0 0  1 0 0  0 1 0]'),
                                               ('AreaLightSource "diffuse" "rgb L" [1 1 1]\n', "disk", "")])
def test_shape_under_an_animated_transform_is_refused_by_name(binding, tmp_path, before, shape, rest):
    with pytest.raises(RuntimeError) as e:
        load(binding, tmp_path, CC.scene_text(CC.BASE_TEXT, world=f'{ANIMATED_WORLD}{before}Shape "{shape}"{rest}\n'))
    msg = str(e.value)
    assert f'Shape "{shape}"' in msg and "camera motion only" in msg
    assert ("AreaLightSource" in msg) == bool(before)


def test_active_transform_wants_one_of_three_words(binding, tmp_path):
    with pytest.raises(RuntimeError, match="ActiveTransform: expected StartTime, EndTime or All"):
        load(binding, tmp_path, CC.scene_text("ActiveTransform Middle\n"))


# ---- the decomposition --------------------------------------------------------------------------------------------------------------
# Worst distance of the float32 restatement (camera_motion_ref.Animated(ft=float32)) from the float64 polar decomposition (numpy
# SVD) over the five motions, start and end: T 0 (it is a copy of the matrix's column), R 2.46e-8, S 8.31e-8. The host's own sums
# may be ordered differently: it gets four times that. (Measured on the same cases, the host: T 0, R 2.46e-8, S 1.36e-7.)
F32_WORST = {"T": 0.0, "R": 2.46e-8, "S": 8.31e-8}


@pytest.mark.parametrize("name", list(CC.MOTIONS))
def test_decomposition_against_the_polar_decomposition(binding, tmp_path, name):
    """T, R (with R[1] negated where Dot(R[0], R[1]) < 0) and S of both transforms against the SVD's, in float64, of the very
    matrices the host decomposed. Band: 4 x F32_WORST, the float32 restatement's own distance measured on these five cases."""
    host = load(binding, tmp_path, CC.scene_text(CC.camera_block(CC.MOTIONS[name][0])))
    mo = host.camera_motion
    assert mo is not None
    ms = [np.array(host.camera()[1].camera_to_world, np.float32).reshape(4, 4), np.array(mo.camera_to_world_end, np.float32).reshape(4, 4)]
    # the matrices are the directives' own
    for got, want in zip(ms, CC.start_end_matrices(name)):
        assert np.abs(got - want).max() < 2e-6
    truth = [CM.polar_truth(m.astype(np.float64)) for m in ms]
    q = [truth[0][1], truth[1][1]]
    flipped = CM.qdot(q[0], q[1]) < 0
    if flipped:
        q[1] = -q[1]
    assert flipped == (name == "rotate_200_flip")
    f32 = CM.Animated(ms[0], ms[1], ft=np.float32)
    for i in range(2):
        got = {"T": np.array(mo.T[i]), "R": np.array(mo.R[i]), "S": np.array(mo.S[i]).reshape(4, 4)}
        want = {"T": truth[i][0], "R": q[i], "S": truth[i][2]}
        mine = {"T": f32.T[i], "R": f32.R[i], "S": f32.S[i]}
        for key in "TRS":
            err = np.abs(got[key].astype(np.float64) - want[key]).max()
            own = np.abs(mine[key].astype(np.float64) - want[key]).max()
            print(f"{name}[{i}] {key}: host {err:.3e}, float32 restatement {own:.3e}, band {4 * F32_WORST[key]:.3e}")
            assert own <= F32_WORST[key] * 1.001   # the measured value stands
            assert err <= 4 * F32_WORST[key]
        assert np.array_equal(got["S"][3], [0, 0, 0, 1]) and np.array_equal(got["S"][:3, 3], [0, 0, 0])
    dot = CM.qdot(np.array(mo.R[0], np.float64), np.array(mo.R[1], np.float64))
    assert dot >= 0 and mo.has_rotation == int(dot < 0.9995)
    assert (dot > 0.9995) == (name in ("translation", "rotate_1_lerp"))
