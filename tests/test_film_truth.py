"""The film on the CPU: the oracle's film (oracle_render), the host's filter table and the host's image conversion
(HostScene.film_to_rgb) held to the float64 truth of film_ref.py within its bands and caps, over film_cases.py's cases: all nine
pixel filters at a border-dominated size and at a size of several ragged tiles, the box room, crop windows, pixelbounds,
samplepixelcenter, scale, maxsampleluminance, Halton and Sobol'. The per-sample inputs (film position, radiance) are the
oracle's own probes, so a disagreement lies in the film. The truth's float32 mode is held to the truth as well - and, where the
float32 table is the host's bit for bit (no exp or sin in it), it is the oracle's film bit for bit.

Measured on the oracle (worst distance as a fraction of band + slack, per case family; printed by every test): small 0.15,
tiles 0.16, room 0.20, crop 0.16, pixelbounds 0.16, pixelcenter 0.22, scale 0.05, maxlum 0.16, sobol 0.17; sample sub-ranges
and shards 0.22; film_to_rgb 0.50 of its own band; flagged pairs 0 of 4.0 million, slack 0 (a constructed input exercises
the flags: test_flagged_pairs_keep_both_candidates)."""
import numpy as np
import pytest

import film_cases as C
import film_ref as FR
from test_oracle_pins import FILTERS

NAMES = [c.name for c in C.CASES]


@pytest.fixture(scope="module")
def loaded(binding, oracle, tmp_path_factory):
    """get(name) -> dict(case, host, truth, px, py, k, pfilm, L, want): each case loaded, probed and summed once, left unchanged."""
    cache, directory = {}, tmp_path_factory.mktemp("film")

    def get(name):
        if name not in cache:
            case = C.BY_NAME[name]
            host, truth = C.load(binding, directory, case)
            spp = host.info["spp"]
            px, py, pfilm, L = C.oracle_inputs(oracle, host, truth, 0, spp)
            _, _, k = C.sample_list(truth, 0, spp)
            for a in (px, py, k, pfilm, L):
                a.setflags(write=False)
            cache[name] = dict(case=case, host=host, truth=truth, spp=spp, px=px, py=py, k=k, pfilm=pfilm, L=L,
                               want=truth.accumulate(px, py, pfilm, L))
        return cache[name]
    return get


@pytest.mark.parametrize("line", FILTERS)
def test_host_filter_table_lies_within_the_float32_band(binding, tmp_path, line):
    """Film::filterTable as the host builds it against the truth's own, computed from the filters' formulas: within table_band, the
    derived float32 evaluation error of an entry. So does the truth's float32 table. The band is a small fraction of the
    table's largest entry - it cannot hide a wrong cell - and zero for box and exact-arithmetic entries."""
    case = C._case("table", "colour", 12, 10, 1, line)
    host, truth = C.load(binding, tmp_path, case)
    tab, wide = host.filter_table()
    assert wide == (line != FILTERS[8])
    band = truth.table_band
    assert band.max() <= 1e-4 * np.abs(truth.table).max(), band.max()
    for name, t in (("host", tab), ("float32 mode", FR.table(truth.flt, np.float32))):
        d = np.abs(t.astype(np.float64) - truth.table)
        frac = np.where(d == 0, 0.0, d / np.where(band == 0, 1e-300, band))
        print(f"{line}: {name} table, worst distance {frac.max():.3f} of the band (band at most {band.max():.2e}, table at most {np.abs(truth.table).max():.3f})")
        assert (d <= band).all(), (line, name, frac.max())
    # [y][x], y with ry: under anisotropic radii the table is not symmetric (Mitchell's is: it is evaluated at p / radius)
    if truth.flt.rx != truth.flt.ry and truth.flt.kind not in ("box", "mitchell"):
        assert np.abs(truth.table - truth.table.T).max() > 100 * band.max()


@pytest.mark.parametrize("name", NAMES)
def test_case_bounds_and_caps(loaded, name):
    """The truth's cropped pixel bounds, sample bounds and pixel bounds are scene.film's; the case keeps inside the two caps
    (flagged pairs, slack); a maxsampleluminance case has samples of both classes, the clamped ones well above the limit."""
    c = loaded(name)
    C.check_bounds(c["host"], c["truth"])
    share, slack = C.check_caps(name, c["want"])
    print(f"{name}: {c['want'].n_pairs} pairs, flagged share {share:.2e} (cap {FR.FLAG_CAP}), slack {slack:.2e} (cap {FR.SLACK_CAP})")
    assert c["want"].n_pairs > 0
    y = c["L"].astype(np.float64) @ FR.Y_WEIGHT
    if np.isfinite(c["case"].max_lum):
        assert c["want"].n_clamped > 40 and c["want"].n_unclamped > 40
        assert (y > 2 * c["case"].max_lum).sum() > 40  # the inputs themselves are not clamped: the film does that
        assert ((y > 0) & (y < c["case"].max_lum)).sum() > 40
    else:
        assert c["want"].n_clamped == 0
    if c["case"].content == "colour" and c["case"].crop == (0, 1, 0, 1) and c["case"].pixel_bounds is None:
        L = c["L"]  # what the content promises: saturated emitter samples beside dim ones of other hues
        assert ((L[:, 0] > 3.9) & (L[:, 2] < 0.2)).sum() > 10 and ((L[:, 2] > 2 * L[:, 0]) & (L[:, 2] > 0.01)).sum() > 10
        assert ((L[:, 1] > 2 * L[:, 0]) & (L[:, 1] > 0.01)).sum() > 10 and (y == 0).sum() > 10


@pytest.mark.parametrize("name", NAMES)
def test_oracle_film_matches_the_truth(loaded, oracle, name):
    """oracle_render's {X, Y, Z, weight} film against the truth at every pixel and channel. The weight plane is the sum of the
    weights; under the 0.5 box, away from whole-number film positions, that is exactly the samples per pixel."""
    c = loaded(name)
    film, _ = oracle.render(c["host"])
    worst = C.check_film(name, film, c["want"])
    print(f"{name}: oracle film, worst distance {worst:.3f} of the band")
    if c["case"].filter == FILTERS[8] and c["case"].pixel_bounds is None:
        # a whole-number coordinate (the Halton and Sobol' points have many exact zeros) also reaches the pixel before it
        wx, wy = (c["pfilm"] == np.floor(c["pfilm"])).T
        expect = np.full(film.shape[:2], float(c["spp"]))
        x, y = c["px"] - c["truth"].crop[0], c["py"] - c["truth"].crop[1]
        for m, dx, dy in ((wx, 1, 0), (wy, 0, 1), (wx & wy, 1, 1)):
            m = m & (x - dx >= 0) & (y - dy >= 0) & (x < film.shape[1]) & (y < film.shape[0])
            np.add.at(expect, (y[m] - dy, x[m] - dx), 1)
        assert (expect == c["spp"]).mean() > 0.3 and ((expect > c["spp"]).sum() > 3 or c["case"].sampler_opts)
        assert (c["want"].value[..., 3] == expect).all() and (film[..., 3] == expect).all()
        assert (c["want"].band[..., 3] > 0).all()  # ... which the band would not have demanded


@pytest.mark.parametrize("name", NAMES)
def test_oracle_sample_ranges_and_tile_shards_match_the_truth(loaded, oracle, name):
    """A k_begin / k_end sub-range sums only those samples; a tile_rank / tile_nranks shard only the samples of its own tiles
    (Oracle.tile_owner) - into whatever pixels their supports reach, neighbouring tiles' included."""
    c = loaded(name)
    truth, spp = c["truth"], c["spp"]
    figures = []
    for kb, ke in ((1, spp), (0, 1)):
        m = (c["k"] >= kb) & (c["k"] < ke)
        want = truth.accumulate(c["px"][m], c["py"][m], c["pfilm"][m], c["L"][m])
        C.check_caps(name, want)
        figures.append(C.check_film(f"{name} k {kb}..{ke}", oracle.render(c["host"], k_begin=kb, k_end=ke)[0], want))
    nranks = 3 if c["case"].content == "room" else 2
    total = 0
    for rank in range(nranks):
        owned = C.owned_tiles(oracle, truth, rank, nranks)
        total += owned.sum()
        want = truth.accumulate(c["px"], c["py"], c["pfilm"], c["L"], owned=owned)
        C.check_caps(name, want)
        figures.append(C.check_film(f"{name} shard {rank} of {nranks}", oracle.render(c["host"], tile_rank=rank, tile_nranks=nranks)[0], want))
    assert total == truth.ntx * truth.nty
    print(f"{name}: sub-ranges and shards, worst distance {max(figures):.3f} of the band")


@pytest.mark.parametrize("name", NAMES)
def test_float32_mode_matches_the_truth(loaded, oracle, name):
    """The truth's float32 mode (the reference's operations in the reference's order) lies inside the truth's bands. Where its
    float32 table is the host's bit for bit, its film is the oracle's bit for bit: two restatements written apart agree on every
    operation and on their order."""
    c = loaded(name)
    f32 = c["truth"].accumulate_float32(c["px"], c["py"], c["pfilm"], c["L"])
    worst = C.check_film(name + " float32 mode", f32, c["want"])
    print(f"{name}: float32 mode, worst distance {worst:.3f} of the band")
    tab, _ = c["host"].filter_table()
    if np.array_equal(tab.view(np.uint32), FR.table(c["truth"].flt, np.float32).view(np.uint32)):
        film, _ = oracle.render(c["host"])
        assert np.array_equal(f32.view(np.uint32), film.view(np.uint32)), name
        owned = C.owned_tiles(oracle, c["truth"], 1, 2)
        part = c["truth"].accumulate_float32(c["px"], c["py"], c["pfilm"], c["L"], owned=owned)
        assert np.array_equal(part.view(np.uint32), oracle.render(c["host"], tile_rank=1, tile_nranks=2)[0].view(np.uint32)), name
    else:
        assert c["truth"].flt.kind in ("gaussian", "sinc")  # the tables differ by libm's exp and sin only


def _check_rgb(name, host, truth, film):
    want, band = truth.to_rgb(film)
    got = host.film_to_rgb(film).astype(np.float64)
    d = np.abs(got - want)
    assert (d <= band).all(), (name, float(np.where(d == 0, 0, d / np.where(band == 0, 1e-300, band)).max()))
    f32, _ = truth.to_rgb(film, np.float32)
    assert (np.abs(f32 - want) <= band).all(), name
    return float(np.where(d == 0, 0, d / np.where(band == 0, 1e-300, band)).max()), want


@pytest.mark.parametrize("name", NAMES)
def test_film_to_rgb_matches_the_truth(loaded, oracle, name):
    """HostScene.film_to_rgb (Film::WriteImage's conversion) of the oracle's film against the truth's conversion of the same film:
    XYZ to RGB, the division by the weight sum, max(0, .), scale. The scale case also against the unscaled conversion; the sinc
    and Mitchell cases have pixels whose sum is negative (a negative lobe over the emitter), which max(0, .) must catch."""
    c = loaded(name)
    film, _ = oracle.render(c["host"])
    worst, want = _check_rgb(name, c["host"], c["truth"], film)
    print(f"{name}: film_to_rgb, worst distance {worst:.3f} of the band")
    raw = film[..., :3].astype(np.float64) @ FR.XYZ_TO_RGB.T
    if c["case"].scale != 1.0:
        assert c["truth"].scale == 2.5 and want.max() > 1
        unscaled = FR.Film(c["case"].xres, c["case"].yres, c["truth"].flt).to_rgb(film)[0]
        assert np.allclose(want, 2.5 * unscaled, rtol=1e-12, atol=0)
    if c["truth"].flt.kind in ("sinc", "mitchell") and c["case"].crop == (0, 1, 0, 1) and c["case"].pixel_bounds is None:
        neg = (raw < -1e-3) & (film[..., 3:4] > 0)
        assert neg.sum() >= 3, name
        assert (want[neg] == 0).all()


def test_film_to_rgb_on_a_synthetic_film(binding, tmp_path):
    """The conversion alone, on a film no render gives: negative sums, negative and zero weight sums (a zero weight leaves
    the pixel undivided and unclamped, film.cpp:200), with scale 2.5."""
    case = C._case("synthetic", "colour", 40, 24, 1, FILTERS[8], scale=2.5)
    host, truth = C.load(binding, tmp_path, case)
    rng = np.random.default_rng(11)
    film = rng.normal(0, 2, (24, 40, 4)).astype(np.float32)
    film[..., 3] = rng.uniform(0.2, 5, (24, 40)).astype(np.float32) * rng.choice([1, 1, 1, -1], (24, 40))
    film[::5, ::3, 3] = 0
    worst, want = _check_rgb("synthetic", host, truth, film)
    print(f"synthetic film: film_to_rgb, worst distance {worst:.3f} of the band")
    zero = film[..., 3] == 0
    assert (want[zero] < 0).any() and (want[~zero] >= 0).all() and (want[~zero] == 0).any()


def test_flagged_pairs_keep_both_candidates():
    """The flags, on an input made for them (no case of film_cases.py has one): under a filter of radius 4, pFilm.x = 5.5 - 2^-21
    gives pd + r = 9 - 2^-21, which float32 rounds to 9 (a tie, to even): Floor + 1 takes pixel column 9 in float32 and leaves it out
    in float64. The truth flags those pairs, keeps both films, widens the band by their difference, accepts either and nothing
    further away; and such an input breaks the share cap, as a condition on a case must."""
    truth = FR.Film(40, 24, FR.parse_pixel_filter(FILTERS[4]))
    pfilm = np.array([[np.float32(5.5) - np.float32(2.0 ** -21), 6.3]], np.float32)
    assert float(pfilm[0, 0]) == 5.5 - 2.0 ** -21
    want = truth.accumulate([5], [6], pfilm, np.array([[4, .5, .1]], np.float32))
    rows = np.flatnonzero(want.slack[:, 9, 3])
    assert want.n_flagged == len(rows) >= 8 and (want.slack[:, :9] == 0).all() and (want.slack[:, 10:] == 0).all()
    assert (want.value[rows, 9] == 0).all() and (want.value32[rows, 9, 3] != 0).all()
    for film in (want.value, want.value32):
        assert FR.compare(film, want)[0] <= 1
    assert FR.compare(want.value32 + 2.001 * (want.value32 - want.value), want)[0] > 1
    with pytest.raises(AssertionError):
        C.check_caps("flagged", want)
