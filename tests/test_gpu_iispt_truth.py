"""The device's IISPT render runner against iispt_ref.py's float64 truth, on the scenes of iispt_cases.py (test_iispt_truth.py holds
the CPU oracle to the same truth). Per case:

  * GpuScene.iispt_hemi_points and iispt_gather equal the oracle's bit for bit, as test_iispt_gather.py has it on its own scenes;
  * independently, the device's hemi points have the truth's `valid`, positions within the float32 error bound of the hit and
    directions within DIR_BAND of the unit normal, and its gather lies within the band 4 B S of the truth over the kept pixels, with
    the truth's weight channel exactly.

`offset`, with its one-pixel task, also goes through iispt_gather_batch, iispt_film_add into a zeroed double monitor and
iispt_film_merge, against the float64 monitors: the sums are double, so the add is held exactly and the merge to one float32
rounding.

The probe cameras' first-hit channels: render_probes takes the three or four probes of iispt_cases.PROBES at once; each probe's
normals and distances equal Oracle.render_probe's bit for bit and, independently, satisfy iispt_ref.probe_first_hits wherever a
pixel's whole footprint lies on one planar face, at 32 x 32 and at 40 x 40 (more than one 16 x 16 storage tile a row)."""
import numpy as np
import pytest

import iispt_cases
import iispt_ref as IR
from test_iispt_truth import DIR_BAND, PROBE_RUNS, check_gather, monitors

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (a == b)).all()


@pytest.mark.parametrize("name", list(iispt_cases.CASES))
def test_device_hemi_points_and_gather(binding, oracle, tmp_path_factory, name):
    c = IR.case_truth(binding, oracle, tmp_path_factory, name)
    gpu = binding.GpuScene(c.host)
    for task, btask, ht, (ov, op, od), nn, gt in c.tasks:
        valid, pos, dr = gpu.iispt_hemi_points(btask)
        assert np.array_equal(valid, ov) and _bits_equal(pos, op) and _bits_equal(dr, od), (name, "hemi points against the oracle")
        k = ht.kept
        assert np.array_equal(valid[k], ht.valid[k]), name
        v = k & (ht.valid == 1)
        off = pos.astype(np.float64) - ht.pos
        assert (np.linalg.norm(off, axis=-1)[v] <= ht.bound[v]).all() and ((off * ht.dir).sum(-1)[v] >= -ht.bound[v]).all(), name
        assert (np.abs(dr.astype(np.float64) - ht.dir)[v] <= DIR_BAND).all(), name
        out = gpu.iispt_gather(btask, valid, pos, dr, nn)
        ref = oracle.iispt_gather(c.host, btask, ov, op, od, nn)
        assert _bits_equal(out, ref), (name, "gather against the oracle")
        check_gather(name, task, out, gt, "device")


def test_offset_through_the_batch_and_the_film_monitors(binding, oracle, tmp_path_factory):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    c = IR.case_truth(binding, oracle, tmp_path_factory, "offset")
    gpu = binding.GpuScene(c.host)
    btasks = [t[1] for t in c.tasks]
    valid, pos, dr = gpu.iispt_hemi_points_batch(btasks)
    assert np.array_equal(valid, np.concatenate([t[3][0].reshape(-1) for t in c.tasks]))
    assert _bits_equal(pos, np.concatenate([t[3][1].reshape(-1, 3) for t in c.tasks]))
    assert _bits_equal(dr, np.concatenate([t[3][2].reshape(-1, 3) for t in c.tasks]))
    nn = np.concatenate([t[4].reshape(-1, IR.HEMI, IR.HEMI, 3) for t in c.tasks])
    out = gpu.iispt_gather_batch(btasks, valid, pos, dr, nn)
    first, outs = 0, []
    for task, btask, _, (ov, op, od), tnn, gt in c.tasks:
        n = (task.x1 - task.x0) * (task.y1 - task.y0)
        outs.append(out[first:first + n].reshape(gt.out.shape))
        assert _bits_equal(outs[-1], oracle.iispt_gather(c.host, btask, ov, op, od, tnn))
        check_gather("offset", task, outs[-1], gt, "device, batched")
        first += n
    assert first == len(out)
    # the film monitors: the one-pixel task lies inside the other, so the two are added by two calls (one call's tasks never overlap)
    direct, indirect, merged = monitors(c, outs)
    h, w = c.host.film_shape
    film = torch.zeros((h, w, 4), dtype=torch.float64, device="cuda")
    for btask, o in zip(btasks, outs):
        o_t = torch.from_numpy(np.ascontiguousarray(o, np.float32)).cuda()
        gpu.iispt_film_add([btask], o_t.data_ptr(), film.data_ptr())
        torch.cuda.synchronize()
    assert np.array_equal(film.cpu().numpy(), indirect), "add_n_samples: double sums of float values, exactly"
    assert (indirect[..., 3] == 1.0).sum() == 1
    direct_t = torch.from_numpy(direct).cuda()
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    binding.iispt_film_merge(direct_t.data_ptr(), film.data_ptr(), h * w, rgb.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(rgb.cpu().numpy(), merged.astype(np.float32)), "merge_into + to_intensity_film: one float32 rounding"


@pytest.mark.parametrize("name,hemi", PROBE_RUNS)
def test_device_probe_first_hits(binding, oracle, tmp_path_factory, name, hemi):
    host, pos, dr, truths = IR.probe_truths(binding, oracle, tmp_path_factory, name, hemi)
    gpu = binding.GpuScene(host)
    inten, nrm, dist, st = gpu.render_probes(pos, dr)
    assert nrm.shape == (len(pos), hemi, hemi, 3) and st["n_paths"] == len(pos) * hemi * hemi
    for i, tr in enumerate(truths):
        oi, on, od = oracle.render_probe(host, pos[i], dr[i], hemi=hemi)
        assert _bits_equal(inten[i], oi) and _bits_equal(nrm[i], on) and _bits_equal(dist[i], od), (name, hemi, "probe", i, "against the oracle")
        share = IR.check_probe(tr, nrm[i], dist[i], (name, hemi, "device, probe", i))
        print(f"{name} at {hemi}: device probe {i} checked on {share:.3f} of its film")
