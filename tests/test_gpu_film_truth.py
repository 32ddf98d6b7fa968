"""The film on the device (GPU): iile_render's {X, Y, Z, weight} film held to the float64 truth of film_ref.py within its bands and
caps, over film_cases.py's cases (shared with test_film_truth.py, which holds the oracle, the host's table and the host's image
conversion to the same truth on the CPU). The per-sample inputs are the device's own probes - GpuScene.li_samples and
halton_samples(px, py, k, 0, 2) - and are the oracle's bit for bit, as are the films: a disagreement with the truth then lies
in the film kernels and not in Li.

Both film paths, by name:
  the box fast path   k_film_accumulate + k_film_resolve with the exact finish (k_patch_*) for whole-number film positions:
                      every case under PixelFilter "box" of radius 0.5, and the 1900 x 24 x 48 strip
  store + gather      k_film_store + k_film_gather / film_gather_pixel + k_film_resolve: every case under a wide filter
each in one pass, with spp_per_pass splitting it, with the instrumented kernels (collect_stats), shard by shard and on a sample
sub-range. guard_radiance's clamp is the maxlum cases'."""
import numpy as np
import pytest

import film_cases as C
import film_ref as FR
from test_oracle_pins import FILTERS

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return tmp_path_factory.mktemp("film_gpu")


def _hold(name, binding, oracle, host, truth, spp, splits, input_check):
    """One scene through every way of rendering it; returns the figures. input_check(px, py, k, pfilm, L): the inputs against
    the oracle's."""
    gpu = binding.GpuScene(host)
    try:
        px, py, pfilm, L = C.device_inputs(gpu, truth, 0, spp)
        _, _, k = C.sample_list(truth, 0, spp)
        input_check(px, py, k, pfilm, L)
        want = truth.accumulate(px, py, pfilm, L)
        share, slack = C.check_caps(name, want)
        ref, _ = oracle.render(host)
        film, st = gpu.render()
        assert st["n_passes"] == 1, name
        figures = [C.check_film(name + ", one pass", film, want)]
        assert np.array_equal(_bits(film), _bits(ref)), name
        for s in splits:
            figures.append(C.check_film(f"{name}, spp_per_pass {s}", gpu.render(spp_per_pass=s)[0], want))
        inst, st = gpu.render(collect_stats=True)
        figures.append(C.check_film(name + ", instrumented kernels", inst, want))
        assert np.array_equal(_bits(inst), _bits(ref)), name
        for rank in range(2):
            owned = C.owned_tiles(oracle, truth, rank, 2)
            part = truth.accumulate(px, py, pfilm, L, owned=owned)
            C.check_caps(name, part)
            figures.append(C.check_film(f"{name}, shard {rank} of 2", gpu.render(tile_rank=rank, tile_nranks=2, spp_per_pass=splits[0] * rank)[0], part))
        m = k >= 1
        sub = truth.accumulate(px[m], py[m], pfilm[m], L[m])
        C.check_caps(name, sub)
        figures.append(C.check_film(f"{name}, samples 1..{spp}", gpu.render(k_begin=1, k_end=spp)[0], sub))
        print(f"device {name}: worst distance {max(figures):.3f} of the band over {len(figures)} renders; {want.n_pairs} pairs, "
              f"flagged share {share:.2e}, slack {slack:.2e}; {want.n_clamped} samples clamped")
        return want
    finally:
        gpu.close()


def _case(name, binding, oracle, directory):
    case = C.BY_NAME[name]
    host, truth = C.load(binding, directory, case)
    C.check_bounds(host, truth)
    spp = host.info["spp"]

    def input_check(px, py, k, pfilm, L):
        opx, opy, opfilm, oL = C.oracle_inputs(oracle, host, truth, 0, spp)
        assert np.array_equal(px, opx) and np.array_equal(py, opy)
        assert np.array_equal(_bits(pfilm), _bits(opfilm)), name
        assert np.array_equal(_bits(L), _bits(oL)), name
    want = _hold(name, binding, oracle, host, truth, spp, (1, 2), input_check)
    if np.isfinite(case.max_lum):
        assert want.n_clamped > 40 and want.n_unclamped > 40
    return host, want


@pytest.mark.parametrize("name", C.BOX)
def test_box_fast_path_matches_the_truth(binding, oracle, directory, name):
    """The box fast path with the exact finish (this module's docstring), every way of rendering."""
    host, _ = _case(name, binding, oracle, directory)
    assert not host.filter_table()[1]


@pytest.mark.parametrize("name", C.WIDE)
def test_store_and_gather_path_matches_the_truth(binding, oracle, directory, name):
    """The store + gather path of the wide filters (this module's docstring), every way of rendering."""
    host, _ = _case(name, binding, oracle, directory)
    assert host.filter_table()[1]


def test_box_exact_finish_on_the_whole_number_strip_matches_the_truth(binding, oracle):
    """The strip of test_whole_number_film_positions_bitwise (killeroo-simple, 1900 x 24 at 48 samples): a film position that is a
    whole number also reaches the pixel before it, and the box fast path then needs its exact finish (k_patch_*) - the left
    neighbour's sum takes a sample of a pixel whose own samples come later in the tile. The truth takes the float32 positions as
    its input and sums exactly. In this strip the whole-number positions are the Halton points' exact zeros, also past x = 1024
    where a float32 position keeps 13 bits of the offset (no position rounds up to the next pixel at 48 samples: counted, not
    required). The inputs are held to the oracle's on every whole-number position and on a random three thousand of the rest."""
    host = binding.HostScene(xres=1900, yres=24, spp=48)
    truth = FR.Film(1900, 24, FR.parse_pixel_filter(FILTERS[8]))
    C.check_bounds(host, truth)
    seen = {}

    def input_check(px, py, k, pfilm, L):
        whole = (pfilm == np.floor(pfilm)).any(axis=1)
        up = (pfilm[:, 0] == px + 1) | (pfilm[:, 1] == py + 1)  # rounded up: the sample left its own pixel
        seen.update(whole=int(whole.sum()), up=int(up.sum()), beyond=int((whole & (px >= 1100)).sum()))
        sel = np.flatnonzero(whole | (np.random.default_rng(3).random(len(px)) < 3000 / len(px)))
        idx = [oracle.sample_index(host, px[i], py[i], k[i]) for i in sel]
        u = np.array([[oracle.sample_dimension(host, j, d, px[i], py[i]) for d in (0, 1)] for i, j in zip(sel, idx)], np.float32)
        assert np.array_equal(_bits(pfilm[sel]), _bits(C.pfilm_of(px[sel], py[sel], u)))
        assert np.array_equal(_bits(L[sel]), _bits(oracle.li(host, px[sel], py[sel], k[sel])[0]))
    want = _hold("strip", binding, oracle, host, truth, 48, (10, 24), input_check)
    print(f"device strip: whole-number film positions {seen}")
    assert seen["whole"] > 100 and seen["beyond"] > 20, seen
    assert (want.value[..., 3] > 48).sum() > 100 and (want.value[..., 3] > 48)[:, 1100:].sum() > 20
