"""The moving-camera scenes the CPU and the GPU tests share: five motions of a camera, as scene-file text and as float64 matrices."""
import numpy as np

import camera_motion_ref as CM

BASE_TEXT = "LookAt 1 2 3  0 0.5 0  0 1 0"
BASE = [CM.look_at([1, 2, 3], [0, 0.5, 0], [0, 1, 0])]
# name: (the directives that act on the end transform alone, the same as matrices)
MOTIONS = {
    "translation": ("Translate 0.5 -0.25 1", [CM.translate(0.5, -0.25, 1)]),
    "rotate_90_oblique": ("Rotate 90 1 2 3", [CM.rotate(90, [1, 2, 3])]),
    "rotate_200_flip": ("Rotate 200 0.3 1 -0.2", [CM.rotate(200, [0.3, 1, -0.2])]),  # Dot(R[0], R[1]) < 0: R[1] is negated
    "rotate_1_lerp": ("Rotate 1 0 1 0.5", [CM.rotate(1, [0, 1, 0.5])]),               # Dot > 0.9995: Slerp's normalised lerp
    "scale_change": ("Rotate 30 0 0 1\nScale 1 2 0.5", [CM.rotate(30, [0, 0, 1]), CM.scale(1, 2, 0.5)]),
}
# No ray can hit a triangle of no area, and the loader refuses a scene without primitives: this one stands in for "no geometry"
NOTHING = 'Material "matte"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 -900  0 0 -900  0 0 -900]\n'


def camera_block(end_text, base_text=BASE_TEXT):
    """The CTM of a camera that moves from `base_text` to `base_text` followed by `end_text`."""
    return f"{base_text}\nActiveTransform EndTime\n{end_text}\nActiveTransform All\n"


def scene_text(before, camera='Camera "perspective" "float fov" [40]', xres=16, yres=16, spp=4, world=None, sampler=None,
               integrator='Integrator "path" "integer maxdepth" [3]', filt='PixelFilter "box"'):
    world = world if world is not None else NOTHING
    sampler = sampler or f'Sampler "halton" "integer pixelsamples" [{spp}]'
    return (f'{before}\n{camera}\nFilm "image" "integer xresolution" [{xres}] "integer yresolution" [{yres}] "string filename" "motion.exr"\n'
            f'{filt}\n{sampler}\n{integrator}\nWorldBegin\n{world}WorldEnd\n')


def start_end_matrices(name):
    """(camera_to_world at the start, at the end) of motion `name`, float64, from the directives' own matrices."""
    return CM.camera_to_world(*BASE), CM.camera_to_world(*BASE, *MOTIONS[name][1])


# ---- the ray cases (test_gpu_camera_motion.py): camera kinds, times, and the two restatements ----
CAMERAS = {
    "perspective": 'Camera "perspective" "float fov" [40]',
    "perspective_lens": 'Camera "perspective" "float fov" [40] "float lensradius" [0.1] "float focaldistance" [3]',
    "environment": 'Camera "environment"',
}
# (TransformTimes, the ray times): below the start, at it, five interior values, at the end, above it
TIME_SETS = {
    "times_0_1": ((0.0, 1.0), [-0.5, 0.0, 0.1, 0.3, 0.5, 0.77, 0.9, 1.0, 1.5]),
    "times_025_075": ((0.25, 0.75), [0.1, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.9]),
}
XRES, YRES = 16, 8


def film_points(seed):
    """64 points of the sample bounds [0, xres] x [0, yres], the four corners among them."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, (64, 2)) * np.array([XRES, YRES])
    p[:4] = [[0, 0], [XRES, 0], [0, YRES], [XRES, YRES]]
    return p.astype(np.float32), rng.uniform(0, 1, (64, 2)).astype(np.float32)


def ray_scene_text(motion, camera, time_set, moving=True, at_end=False):
    """The scene of a ray case; moving = False: the static scene whose camera stands at the start (at_end: the end) transform."""
    (t0, t1), _ = TIME_SETS[time_set]
    if moving:
        before = f"TransformTimes {t0} {t1}\n" + camera_block(MOTIONS[motion][0])
    else:
        before = BASE_TEXT + ("\n" + MOTIONS[motion][0] if at_end else "")
    return scene_text(before, camera=CAMERAS[camera], xres=XRES, yres=YRES)


def restated_rays(host, camera, time_set, pfilm, plens, ft):
    """The rays of every time of the set from the host's two float32 matrices and camera, restated in `ft`: [(o, d)] per time."""
    kind, cam = host.camera()
    mo = host.camera_motion
    (t0, t1), times = TIME_SETS[time_set]
    assert (mo.start_time, mo.end_time) == (np.float32(t0), np.float32(t1))
    start = np.array(cam.camera_to_world, np.float32).reshape(4, 4)
    end = np.array(mo.camera_to_world_end, np.float32).reshape(4, 4)
    anim = CM.Animated(start, end, mo.start_time, mo.end_time, ft=ft)
    out = []
    for t in times:
        out.append(CM.generate_ray(anim, np.float32(t), "environment" if camera == "environment" else "perspective", pfilm, plens,
                                   raster_to_camera=np.array(cam.raster_to_camera, np.float32), lens_radius=cam.lens_radius,
                                   focal_distance=cam.focal_distance, xres=XRES, yres=YRES))
    return out
