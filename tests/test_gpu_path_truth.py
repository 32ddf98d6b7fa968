"""The device's PathIntegrator::Li against path_ref.py's float64 truth, on the scenes of path_cases.py (test_path_truth.py holds the
CPU oracle to the same truth). Per case:

  * GpuScene.li_samples (the listed-sample pass: the instrumented wavefront kernels over the digit chains) equals Oracle.li bit for
    bit, L and ray counts, and lies within the band 4 B S of the truth over the kept samples;
  * the frame through render() equals Oracle.render bit for bit, at the case's own size and at 40 x 24 (six sample tiles, so that
    spp_per_pass has something to split): with the plain kernels, with the instrumented ones, split by spp_per_pass, and from a
    handle created under IILE_NO_SAMPLE_TABLE: the frame runs the sample table, skip_last_bounce and the
    NEE record without a MIS ray, which the per-sample pass does not.

The frames tie those paths to the oracle; the per-sample check ties the oracle, and the device with it, to the truth."""
import numpy as np
import pytest

import path_cases
import path_ref as PR

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(path_cases.CASES))
def test_device_li_and_frames(binding, oracle, tmp_path_factory, monkeypatch, name):
    host, px, py, k, tr, _ = PR.case_truth(binding, oracle, tmp_path_factory, name)
    monkeypatch.delenv("IILE_NO_SAMPLE_TABLE", raising=False)
    gpu = binding.GpuScene(host)
    L, nr = gpu.li_samples(px, py, k)
    L_o, nr_o = oracle.li(host, px, py, k)
    assert np.array_equal(_bits(L), _bits(L_o)), (name, "li_samples against Oracle.li")
    assert np.array_equal(nr, nr_o), (name, "ray counts")
    assert np.isfinite(L).all() and (L >= 0).all()
    kept, band = tr.kept, 4 * PR.MEASURED[name][1]
    rel = PR.rel_distance(L, tr)
    worst = int(np.argmax(np.where(kept, rel, -1)))
    print(f"{name}: device worst distance {rel[worst]:.3e} of S at sample {worst}, {rel[worst] / band if band else 0:.3f} of the band")
    assert np.array_equal(nr[kept, 0], tr.n_regular[kept]) and np.array_equal(nr[kept, 1], tr.n_shadow[kept]), name
    assert (rel[kept] <= band).all(), (name, worst, rel[worst], band)
    ref, _ = oracle.render(host)
    film, _ = gpu.render()
    assert np.array_equal(_bits(film), _bits(ref)), (name, "the case's own frame")
    # a pass is made of whole 16 x 16 sample tiles, so the split needs a frame of several: the same scene at 40 x 24
    wide = binding.HostScene(path=host.scene_path, xres=40, yres=24)
    gpu = binding.GpuScene(wide)
    ref, _ = oracle.render(wide)
    assert ref[..., :3].any()
    film, st = gpu.render()
    assert np.array_equal(_bits(film), _bits(ref)), (name, "plain kernels")
    inst, _ = gpu.render(collect_stats=True)
    assert np.array_equal(_bits(inst), _bits(ref)), (name, "instrumented kernels")
    split, st = gpu.render(spp_per_pass=1)
    assert st["n_passes"] > 1
    assert np.array_equal(_bits(split), _bits(ref)), (name, "spp_per_pass 1")
    monkeypatch.setenv("IILE_NO_SAMPLE_TABLE", "1")
    chains = binding.GpuScene(wide)
    monkeypatch.delenv("IILE_NO_SAMPLE_TABLE")
    by_chains, st = chains.render()
    assert st["sample_table_bytes"] == 0
    assert np.array_equal(_bits(by_chains), _bits(ref)), (name, "without the sample table")
