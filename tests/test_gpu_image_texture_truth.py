"""The device's ImageTexture path against mipmap_ref.py's float64 statement of the reference, on the configurations of
test_image_texture_truth.py: filtered lookups through the texture probe, and the per-sample radiance of a textured tilted quad
from the pixel on. Each comparison with the truth is paired with the bitwise one against the oracle, which these small
pyramids (a 1 x 1 image: ilod + 1 == n_levels on every lookup; a 5 x 1 image: levels of height 1) had not seen."""
import numpy as np
import pytest

import test_image_texture_truth as T
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_image_texture_truth")


@pytest.fixture(scope="module")
def lookup_case(binding, workdir):
    """The (image, options) configuration with its truth, computed once."""
    made = {}

    def get(image_name, option_name):
        if (image_name, option_name) not in made:
            case = T.LookupCase(workdir, binding, image_name, option_name)
            made[image_name, option_name] = (case, binding.GpuScene(case.scene))
        return made[image_name, option_name]
    return get


@pytest.mark.parametrize("image_name,option_name", T.CONFIGS)
def test_device_lookups_against_the_float64_truth(lookup_case, oracle, image_name, option_name):
    """gpu.texture_eval within scale * (4 ulp32(1 + max(|s|, |t|)) + 2^-20) + slack of ImageTexture::Evaluate in float64 on each
    of 2000 lookups, and bit for bit the oracle's on the same inputs."""
    case, gpu = lookup_case(image_name, option_name)
    case.check_slack_cap()
    got = gpu.texture_eval(0, case.uv, case.duv)
    dist = case.check(got, "device")
    print(f"lookups {case.name}: device to truth {dist:.3g} of scale")
    assert_bitwise(got, oracle.texture_eval(case.scene, 0, case.uv, case.duv), f"{case.name} lookups")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_device_lookup_counts_at_the_ends_of_the_probe_grid(lookup_case, oracle, n):
    """Lookup counts around the wave and the block size of the probe's grid (2000 is the other tests'): the first n lookups."""
    case, gpu = lookup_case("12x5", "ewa")
    got = gpu.texture_eval(0, case.uv[:n], case.duv[:n])
    assert got.shape == (n, 3)
    case.check(got, f"device, {n} lookups")
    assert_bitwise(got, oracle.texture_eval(case.scene, 0, case.uv[:n], case.duv[:n]), f"{n} lookups")


@pytest.mark.parametrize("axis,filt", T.LI_CASES)
def test_device_li_per_sample_against_the_truth(binding, oracle, workdir, axis, filt):
    """gpu.li_samples on a textured quad tilted to each dominant normal axis, EWA and trilinear, for every (pixel, sample) of a
    16 x 12 window: against film position (the Halton sampler's dimensions 0 and 1, an input here) -> hit_differentials ->
    evaluate -> Kd / pi * I / r^2 * |cos|, within 4 x the distance the oracle was measured at on the CPU (T.LI_MEASURED,
    T.LI_BOUND; under the 2e-3 cap) plus the slack, which `distance` holds to the same caps as on the CPU (at most 10 % of the
    samples, at most 1 % of scale), so that the device's film positions cannot bring a wider slack than was measured; and bit
    for bit the oracle's per-sample Li."""
    assert 0 < T.LI_BOUND <= T.LI_CAP
    case = T.LiCase(workdir, binding, axis, filt)
    gpu = binding.GpuScene(case.scene)
    samples, _ = gpu.halton_samples(case.px, case.py, case.k, 0, 2)
    pfilm = np.stack([case.px.astype(np.float32) + samples[:, 0], case.py.astype(np.float32) + samples[:, 1]], 1)
    L, nr = gpu.li_samples(case.px, case.py, case.k)
    dist, n, share, worst = case.distance(L, pfilm)
    print(f"Li {case.name}: device to truth {dist:.3g} of scale over {n} samples; slack on {share:.2%}, largest {worst:.3g} of scale")
    assert dist <= T.LI_BOUND, f"{case.name}: {dist:.3g} of scale"
    rL, rnr = oracle.li(case.scene, case.px, case.py, case.k)
    assert np.array_equal(nr, rnr), "per-sample ray counts differ"
    assert_bitwise(L, rL, f"{case.name} per-sample radiance")
