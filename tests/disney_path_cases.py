"""Two small scenes at which PathIntegrator::Li runs through Disney BSDFs, for path_ref.py's float64 truth (test_gpu_disney.py holds
the device to it): the builder, the room and the truth machinery are path_cases' and path_ref's, the materials disney_ref's
DisneyMaterial (its lobes plug into path_ref.BSDF unchanged).

  disney_room   a small closed room, 16 x 16 x 1 spp, one quad area light under the ceiling, maxdepth 5: walls `default`, floor
                `coated`, back wall `metal` (test_gpu_disney's cases)
  disney_thin   a thin Disney sheet (`thin_all`) between the camera and the lights, a point light and a quad area light behind it,
                matte walls, maxdepth 5: light reaches the camera side only through the sheet's two transmission lobes

The oracle has no Disney material, but its sampler and camera read only the descriptor's sampler and camera: path_ref.frame_inputs
takes the sample values and camera rays of these scenes from it as for every other case (test_disney_truth.test_path_cases_truth checks
that on the CPU).

MEASURED: per case (kept share, B), B = the worst |L32 - L64| / S of path_ref's float32 mode over the kept samples, as
`python tests/disney_path_cases.py` printed them. The device's band is 4 B S."""
import numpy as np

import disney_ref as D
import path_cases as PC
import path_ref as PR

DM = D.DisneyMaterial
M = PR.Material
SPP = 1


def _finish(b, *a, **kw):
    scene, text, files = b.finish(*a, **kw)
    return scene, text.replace(f'"integer pixelsamples" [{PC.SPP}]', f'"integer pixelsamples" [{SPP}]'), files


def disney_room():
    b = PC.Builder()
    PC.room(b, (-2, 0, -4), (2, 3, 2), DM(**D.CASES["default"]), floor=DM(**D.CASES["coated"]), back=DM(**D.CASES["metal"]))
    b.quad(PC.BLACK, (-0.75, 2.75, -1.5), (0.75, 2.75, -1.5), (0.75, 2.75, 0.0), (-0.75, 2.75, 0.0), emit=(12.0, 11.0, 9.0))
    return _finish(b, "0.25 1.5 -3.5", "0 1 0.5", 55, 5)


def disney_thin():
    b = PC.Builder()
    PC.room(b, (-2, 0, -4), (2, 3, 3), M("matte", Kd=(0.6, 0.55, 0.5)))
    b.quad(DM(**D.CASES["thin_all"]), (-1.75, 0.2, 0.0), (-1.75, 2.8, 0.0), (1.75, 2.8, 0.0), (1.75, 0.2, 0.0))
    b.quad(PC.BLACK, (-0.75, 0.75, 2.5), (-0.75, 2.25, 2.5), (0.75, 2.25, 2.5), (0.75, 0.75, 2.5), emit=(10.0, 10.0, 8.0))
    b.light("point", pos=(0.5, 1.0, 1.5), I=(8.0, 7.0, 6.0))
    return _finish(b, "0 1.5 -3.5", "0 1.4 0", 50, 5, strategy="uniform")


CASES = {"disney_room": disney_room, "disney_thin": disney_thin}

# what measure() printed: per case (kept share, B)
MEASURED = {
    "disney_room": (0.9453, 1.816e-04),   # 256 samples, 4.32 vertices; lit 1.00; {'rr_survived': 6, 'rr_died': 171, 'bsdf_half': 8}; dropped at {335: 7, 892: 5, 776: 1, 699: 1}
    "disney_thin": (0.9961, 1.901e-05),   # 256 samples, 4.66 vertices; lit 0.99; {'rr_survived': 7, 'rr_died': 206, 'bsdf_half': 1}; dropped at {776: 1}
}

_CACHE = {}


def case_truth(binding, oracle, tmp_path_factory, name):
    """(host, px, py, k, PathTruth, (scene, o, d, value)) of a case, computed once per session (as path_ref.case_truth)."""
    if name not in _CACHE:
        scene, text, files = CASES[name]()
        assert not files
        root = tmp_path_factory.mktemp("disney_path")
        p = root / (name + ".pbrt")
        p.write_text(text)
        host = binding.HostScene(path=str(p))
        host.scene_path = str(p)
        px, py, k, o, d, value = PR.frame_inputs(oracle, host)
        _CACHE[name] = (host, px, py, k, PR.li(scene, o, d, value), (scene, o, d, value))
    return _CACHE[name]


def float32_distance(name, binding, oracle, tmp_path_factory):
    """(B of the case, the float32 PathTruth): path_ref.float32_distance over this module's cases."""
    _, _, _, _, tr, (scene, o, d, value) = case_truth(binding, oracle, tmp_path_factory, name)
    t32 = PR.li(scene, o, d, value, np.float32, tr.logs)
    return float(PR.rel_distance(t32.L, tr)[tr.kept].max()), t32


def measure():
    import pathlib
    import sys
    import tempfile
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
    import conftest
    import oracle_binding
    import __graft_entry__ as ge
    ge.build_if_needed()
    binding, oracle = conftest.load_binding(), oracle_binding.Oracle()

    class Factory:
        def mktemp(self, name):
            return pathlib.Path(tempfile.mkdtemp(prefix=name))
    for name in CASES:
        host, px, py, k, tr, _ = case_truth(binding, oracle, Factory(), name)
        B, t32 = float32_distance(name, binding, oracle, Factory())
        live = {k_: int(v) for k_, v in tr.stats.items() if v}
        print(f'    "{name}": ({tr.kept.mean():.4f}, {B:.3e}),   # {len(px)} samples, {tr.nverts.mean():.2f} vertices; lit {(tr.L.max(1) > 0).mean():.2f}; '
              f'{live}; dropped at {dict(sorted(tr.why.items(), key=lambda kv: -kv[1])[:4])}')


if __name__ == "__main__":
    measure()
