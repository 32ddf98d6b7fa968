"""The IISPT render runner held to iispt_ref.py's float64 truth, hemi point to film pixel, on the scenes of iispt_cases.py: the truth's
generator against PCG32's published values, its own caps, and the CPU oracle against it (test_gpu_iispt_truth.py holds the device
to the same truth). No GPU.

Per case: Oracle.iispt_hemi_points has the truth's `valid`, positions within the float32 error bound of the hit (iispt_ref.
hemi_point_bound) on the normal's side, directions within DIR_BAND of the unit normal; Oracle.iispt_gather lies within 4 B S of the
truth over the kept pixels, with the truth's weight channel exactly (0 or 0.5) and zeros where the runner records nothing;
Oracle.iispt_merge is the float64 monitors' merge to one float32 rounding.

What iispt_ref.measure() printed is iispt_ref.MEASURED; the oracle's worst distance in units of the band is, per case, between 0.20
(offset) and 0.60 (specular).

Mutations of oracle/oracle_path.cpp (a scratch copy, built outside the tree) and what fails for each: DESIGN.md section 2, "The IISPT
gather is held to a float64 truth".
"""
import numpy as np
import pytest

import iispt_cases
import iispt_ref as IR

CASES = list(iispt_cases.CASES)
KEPT_CAP = 0.9     # a cap on the truth alone, not a measurement: a case that misses it changes its inputs
KEPT_MIN = 50
DIR_BAND = 64 * IR.U   # a unit normal from a float32 cross product of two edges and its normalisation: some ten roundings a component


@pytest.fixture(scope="module")
def truth(binding, oracle, tmp_path_factory):
    return lambda name: IR.case_truth(binding, oracle, tmp_path_factory, name)


def test_pcg32_known_answers():
    """The PCG32 demo's published values (pcg32_srandom(42, 54): pcg-random.org's pcg32-demo) pin the step, the output function and
    the seeding of rng.h:142-156, which differs from the demo only in its initial state; UniformFloat and UniformUInt32(b) on top."""
    g = IR.Pcg32(54, initstate=42)
    assert [g.u32() for _ in range(6)] == [0xa15c02b7, 0x7b47f409, 0xba1d3330, 0x83d2f293, 0xbfa4784b, 0xcbed606e]
    a, b = IR.Pcg32(7), IR.Pcg32(7)
    for _ in range(64):
        u = a.u32()
        f = b.uniform_float()
        assert f.dtype == np.float32 and 0 <= f < 1 and f == min(np.float32(1) - np.float32(2.0 ** -24), np.float32(np.float32(u) * np.float32(2.0 ** -32)))
    a, b = IR.Pcg32(9), IR.Pcg32(9)
    assert [a.uniform_u32(32) for _ in range(32)] == [b.u32() % 32 for _ in range(32)]   # 2^32 mod 32 = 0: nothing is rejected
    c = IR.Pcg32(11)
    assert all(c.uniform_u32(3) < 3 for _ in range(64))
    assert IR.Pcg32(0).u32() != IR.Pcg32(1).u32()


def test_hemi_grid_and_neighbours(binding):
    """iisptrenderrunner.cpp:381-410 and :434-464 on the truth's own Task, against the ABI's count."""
    for (a1, ts, want) in ((96, 10, [0, 10, 20, 30, 40, 50, 60, 70, 80, 90, 95]), (81, 10, [0, 10, 20, 30, 40, 50, 60, 70, 80]), (5, 10, [0, 4]), (1, 3, [0])):
        t = IR.Task(0, 0, a1, a1, ts, 0, 0)
        assert t.hemi_xs() == want and t.hemi_ys() == want
        assert binding.IisptTask(0, 0, a1, a1, ts, 0, 0).grid() == (len(want), len(want))
    t = IR.Task(3, 2, 14, 13, 7, 0, 0)
    assert t.hemi_xs() == [3, 10, 13] and t.hemi_ys() == [2, 9, 12]
    assert t.neighbours(3, 2) == [(3, 2), (10, 9), (10, 2), (3, 9)]            # S, E, R, B
    assert t.neighbours(12, 11) == [(10, 9), (13, 12), (13, 9), (10, 12)]      # the clamp at x1 - 1, y1 - 1
    assert t.neighbours(13, 12) == [(10, 9), (13, 12), (13, 9), (10, 12)]
    assert IR.Task(9, 6, 10, 7, 7, 0, 0).neighbours(9, 6) == [(9, 6)] * 4


@pytest.mark.parametrize("name", CASES)
def test_case_is_small_and_live(truth, name):
    """At most 64 triangles and about 150 film pixels a task; kept >= 0.9 of the pixels with a vertex and >= 50 pixels; the branches
    the case is for are taken: on the truth alone."""
    c = truth(name)
    assert len(c.scene.P) <= 64 and c.host.info["n_triangles"] == len(c.scene.P)
    for task, *_ in c.tasks:
        assert (task.x1 - task.x0) * (task.y1 - task.y0) <= 160 and task.x1 <= c.host.info["xres"] and task.y1 <= c.host.info["yres"]
    share, kept, est, stats = IR.summary(c)
    why = [t[5].why for t in c.tasks]
    print(f"{name}: kept {share:.4f} ({kept} pixels), {est:.1f} estimates per pixel, stats {stats}, first flags by line {why}")
    assert share >= KEPT_CAP and kept >= KEPT_MIN, (name, share, kept, why)
    for what in iispt_cases.LIVE[name]:
        assert stats.get(what, 0) > 0, (name, what, stats)
    assert np.isclose(share, IR.MEASURED[name][0], atol=5e-5) and kept == IR.MEASURED[name][1], name


def test_what_the_cases_are_for(truth):
    """offset: a rectangle strictly inside the film and a one-pixel task; missing: pixels with one to three missing neighbours that
    still count their draws; folded: nine pixels in ten at least 10 degrees off every one of their hemi points; up_rule: normals
    exactly along z; specular: chains with beta != 1."""
    c = truth("offset")
    (t0, *_), (t1, _, _, (v1, _, _), _, g1) = c.tasks
    assert t0.x0 > 0 and t0.y0 > 0 and t0.counter_base > 0 and t0.x1 < c.host.info["xres"]
    assert (t1.x1 - t1.x0, t1.y1 - t1.y0) == (1, 1) and v1.shape == (1, 1) and g1.has.all() and g1.kept.all()
    c = truth("missing")
    task, _, _, (valid, _, _), _, g = c.tasks[0]
    xs, ys = task.hemi_xs(), task.hemi_ys()
    n_missing = np.array([[sum(1 - int(valid[ys.index(qy), xs.index(qx)]) for qx, qy in task.neighbours(fx, fy)) for fx in range(task.x0, task.x1)]
                          for fy in range(task.y0, task.y1)])
    assert {1, 2, 3} <= set(n_missing[g.has].tolist())
    assert (g.taken[g.has & (n_missing > 0)] > g.n_est[g.has & (n_missing > 0)]).any()
    g = truth("folded").tasks[0][5]
    a = g.angle[g.has]
    assert (a >= 10).mean() >= 0.9 and np.nanmax(a) <= 40
    _, _, _, (valid, _, dr), _, _ = truth("up_rule").tasks[0]
    assert valid.all() and (dr[..., :2] == 0).all() and (np.abs(dr[..., 2]) == 1).all()
    g = truth("specular").tasks[0][5]
    m = g.has & g.kept
    assert {0, 1, 2, 3} <= set(g.chain[m].tolist()) and (g.chain[m] > 0).sum() >= 10
    assert (g.out[..., :3][m & (g.chain > 0)] > 0).any()   # beta != 1 reaches the record


@pytest.mark.parametrize("name", CASES)
def test_oracle_hemi_points_match_truth(truth, name):
    c = truth(name)
    for task, _, ht, (valid, pos, dr), _, _ in c.tasks:
        k = ht.kept
        assert np.array_equal(valid[k], ht.valid[k]), name
        v = k & (ht.valid == 1)
        off = pos.astype(np.float64) - ht.pos
        dist = np.linalg.norm(off, axis=-1)
        assert (dist[v] <= ht.bound[v]).all(), (name, dist[v].max(), ht.bound[v])
        assert ((off * ht.dir).sum(-1)[v] >= -ht.bound[v]).all(), (name, "the aux ray starts on the normal's side")
        assert (np.abs(dr.astype(np.float64) - ht.dir)[v] <= DIR_BAND).all(), (name, np.abs(dr - ht.dir)[v].max())
        assert not pos[valid == 0].any() and not dr[valid == 0].any()


@pytest.mark.parametrize("name", CASES)
def test_float32_mode_gives_the_band(truth, oracle, name):
    """B of the case, from the truth's own float32 mode against its float64 mode over the kept pixels: what iispt_ref.MEASURED
    records, and what the band of the oracle and of the device is four times."""
    B = IR.float32_distance(truth(name), oracle)
    print(f"{name}: B {B:.3e} (recorded {IR.MEASURED[name][2]:.3e})")
    assert np.isclose(B, IR.MEASURED[name][2], rtol=2e-3, atol=1e-12), name


def check_gather(name, task, out, gt, who):
    """`out` (h, w, 4) against the truth of one task; returns the worst share of the band."""
    band = 4 * IR.MEASURED[name][2]
    out = np.asarray(out).reshape(gt.out.shape)
    assert np.isfinite(out).all() and (out[..., :3] >= 0).all()
    m = gt.kept
    assert np.array_equal(out[..., 3][m], gt.out[..., 3][m]), (name, who, "the weight channel: 0 or 0.5")
    assert not out[m & ~gt.has].any(), (name, who, "nothing is recorded without a vertex")
    m = gt.kept & gt.has
    rel = np.where(m, IR.rel_distance(out, gt), -1)
    worst = np.unravel_index(int(np.argmax(rel)), rel.shape)
    share = float(rel[worst]) / band
    print(f"{name}: {who} worst distance {rel[worst]:.3e} of S at pixel {worst}, {share:.3f} of the band")
    assert (rel[m] <= band).all(), (name, who, worst, rel[worst], band, out[worst], gt.out[worst])
    return share


@pytest.mark.parametrize("name", CASES)
def test_oracle_gather_matches_truth(truth, oracle, name):
    c = truth(name)
    for task, btask, _, (valid, pos, dr), nn, gt in c.tasks:
        check_gather(name, task, oracle.iispt_gather(c.host, btask, valid, pos, dr, nn), gt, "oracle")


def test_the_band_sees_a_wrong_input(truth, oracle):
    """The truth's inputs mutated: the oracle given the hemispheres upside down, mirrored, or its neighbours' images R and B swapped
    leaves the band on most pixels; another seed or sampler counter likewise."""
    c = truth("room")
    task, btask, _, (valid, pos, dr), nn, gt = c.tasks[0]
    band, m = 4 * IR.MEASURED["room"][2], gt.kept & gt.has
    outside = lambda out: float((IR.rel_distance(out, gt)[m] > band).mean())
    assert outside(oracle.iispt_gather(c.host, btask, valid, pos, dr, nn[:, :, ::-1])) > 0.9
    assert outside(oracle.iispt_gather(c.host, btask, valid, pos, dr, nn[:, :, :, ::-1])) > 0.9
    assert outside(oracle.iispt_gather(c.host, btask, valid, pos, dr, nn[:, ::-1])) > 0.9
    other = type(btask)(*(task.args()[:6] + (task.rng_seed + 1,)))
    assert outside(oracle.iispt_gather(c.host, other, valid, pos, dr, nn)) > 0.9


def monitors(c, outs, seed=3):
    """(direct monitor, indirect monitor, their float64 merge): a seeded direct monitor (weights 0, 1 or 16) and the float64
    add_n_samples of the case's tasks."""
    h, w = c.host.film_shape
    rng = np.random.default_rng(seed)
    direct = np.zeros((h, w, 4))
    direct[..., 3] = rng.choice([0.0, 1.0, 16.0], size=(h, w))
    direct[..., :3] = rng.uniform(0, 40, (h, w, 3)) * (direct[..., 3:] > 0)
    indirect = np.zeros((h, w, 4))
    for (task, *_), out in zip(c.tasks, outs):
        IR.film_add(indirect, task, out)
    return direct, indirect, IR.film_merge(direct, indirect)


def test_oracle_merge_matches_the_float64_monitors(truth, oracle):
    c = truth("offset")
    outs = [oracle.iispt_gather(c.host, btask, v, p, d, nn) for _, btask, _, (v, p, d), nn, _ in c.tasks]
    direct, indirect, want = monitors(c, outs)
    assert (indirect[..., 3] == 0.5).sum() > 100 and (indirect[..., 3] == 1.0).sum() == 1   # the one-pixel task lies inside the other: two records
    got = oracle.iispt_merge(direct, indirect)
    assert np.array_equal(got, want.astype(np.float32))   # the sums are double: one float32 rounding


PROBE_RUNS = [("room", 32), ("room", 40), ("up_rule", 32)]   # 40: more than one 16 x 16 storage tile a row, the device's general film path


@pytest.mark.parametrize("name,hemi", PROBE_RUNS)
def test_oracle_probe_first_hits(binding, oracle, tmp_path_factory, name, hemi):
    """Oracle.render_probe's distance and normal films against iispt_ref.probe_first_hits: wherever a probe pixel's whole footprint
    lies on one planar face, at least 0.6 of every probe's film. (Intensity is PathIntegrator::Li's integrand, held to path_ref.)"""
    host, pos, dr, truths = IR.probe_truths(binding, oracle, tmp_path_factory, name, hemi)
    assert 3 <= len(pos) <= 4 and len({tuple(p) for p in pos.tolist()}) == len(pos)
    assert any(d[0] == 0 and d[1] == 0 for d in dr) and any(d[0] != 0 or d[1] != 0 for d in dr)   # both branches of `up`
    films = []
    for i, tr in enumerate(truths):
        assert tr.ok.mean() >= iispt_cases.PROBE_SHARE, (name, i, tr.ok.mean())
        _, nrm, dist = oracle.render_probe(host, pos[i], dr[i], hemi=hemi)
        films.append((nrm, dist))
        share = IR.check_probe(tr, nrm, dist, (name, hemi, "oracle, probe", i))
        print(f"{name} at {hemi}: probe {i} checked on {share:.3f} of its film")
    # the check sees a neighbour's camera, and (in the room: a plane seen head-on is the same upside down) a film upside down
    with pytest.raises(AssertionError):
        IR.check_probe(truths[0], *films[1], "probe 1's films as probe 0's")
    if name == "room":
        with pytest.raises(AssertionError):
            IR.check_probe(truths[0], films[0][0][::-1], films[0][1][::-1], "rows reversed")
        with pytest.raises(AssertionError):
            IR.check_probe(truths[0], films[0][0].transpose(1, 0, 2), films[0][1].T, "x and y swapped")
