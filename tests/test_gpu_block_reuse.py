"""A scene handle keeps eight grow-only device blocks (path workspace, film planes, wide-filter store, probe block, exact
film finish, tile tables, IISPT scratch, film_add table; api_common.h DevBlock / Carver). Most tests make a fresh handle
per case and never walk the paths on which a block regrows, a pointer into a freed block could survive, or a carving
moves. Every case here holds a result of a long-lived handle to the same call on a fresh handle, bit for bit.

Scenes: tests/boxroom.py at 32 x 32 (four 16 x 16 tiles, so more than one block and more than one tile per rank); `strip`
is a 32 x 32 crop window past pixel 1024 of a 2048 x 2048 frame, where film positions round to whole numbers as in
test_whole_number_film_positions_bitwise (the oracle counts 53 pixels that take a neighbour's sample at 16 spp)."""
import numpy as np
import pytest

import boxroom

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    u = np.uint64 if a.dtype.itemsize == 8 else (np.uint32 if a.dtype.itemsize == 4 else np.uint8)
    bad = int((a.view(u) != b.view(u)).sum())
    assert bad == 0, f"{what}: {bad} words differ"


@pytest.fixture(scope="module")
def rooms(binding, tmp_path_factory):
    """The scenes of this module, made once: plain (box film), wide (gaussian pixel filter), mirror (mirror and uber blobs)."""
    d = tmp_path_factory.mktemp("block_reuse")

    def room(name, extra="", res=32, spp=4, crop="", **kw):
        text = boxroom.boxroom_pbrt(xres=res, yres=res, spp=spp, ico_levels=1, n_blobs=3, wall_n=4, **kw)
        if extra:
            text = text.replace("WorldBegin", extra + "\nWorldBegin", 1)
        if crop:
            assert '"integer yresolution"' in text
            text = text.replace('"integer yresolution"', crop + ' "integer yresolution"', 1)
        p = d / (name + ".pbrt")
        p.write_text(text)
        return binding.HostScene(path=str(p))

    a, b = 1100 / 2048, 1132 / 2048
    return {"plain": room("plain"), "wide": room("wide", 'PixelFilter "gaussian"'), "mirror": room("mirror", materials="mixed"),
            "strip": room("strip", res=2048, spp=16, crop='"float cropwindow" [%r %r %r %r]' % (a, b, a, b))}


def _walk(binding, scene, calls, what):
    """Each call on one long-lived handle and on a handle of its own; returns the long-lived handle's results."""
    gpu = binding.GpuScene(scene)
    got = []
    for i, call in enumerate(calls):
        r = call(gpu)
        twin = call(binding.GpuScene(scene))
        for j, (a, b) in enumerate(zip(r, twin)):
            _same(a, b, f"{what}, call {i}, output {j}")
        got.append(r)
    return got


def _render(**kw):
    return lambda gpu: (gpu.render(**kw)[0],)


PROBE_POS = np.array([[0, 0, 0.5], [1, -2, 1], [-2, 1, 0]], np.float32)
PROBE_DIR = np.array([[0, 0, 1], [0.3, 1, 0.2], [1, 0, 0]], np.float32)


def _probes(n):
    return lambda gpu: gpu.render_probes(PROBE_POS[:n], PROBE_DIR[:n])[:3]


@pytest.mark.parametrize("spp_per_pass", [0, 1])
def test_path_workspace_grows_then_is_reused(binding, rooms, spp_per_pass):
    """Samples [0, 1), then [0, 4) (the workspace grows), then [0, 1) again in the larger workspace; with spp_per_pass = 1 the
    four-sample render makes four passes through one workspace."""
    ranges = ((0, 1), (0, 4), (0, 1))
    got = _walk(binding, rooms["plain"], [_render(k_begin=a, k_end=b, spp_per_pass=spp_per_pass) for a, b in ranges], "workspace")
    _same(got[2][0], got[0][0], "third render against the first")
    assert not np.array_equal(got[1][0], got[0][0])


def test_tile_tables(binding, rooms):
    shards = ((0, 1), (0, 2), (1, 2), (0, 1))
    got = _walk(binding, rooms["plain"], [_render(tile_rank=r, tile_nranks=n) for r, n in shards], "tile tables")
    _same(got[3][0], got[0][0], "one rank again")


def test_wide_filter_store_shared_with_the_probe_pass(binding, rooms):
    got = _walk(binding, rooms["wide"], [_render(k_begin=0, k_end=1), _render(k_begin=0, k_end=2), _probes(2), _render(k_begin=0, k_end=2)],
                "wide store")
    _same(got[3][0], got[1][0], "the frame again after the probe pass")


def test_probe_block(binding, rooms):
    got = _walk(binding, rooms["plain"], [_probes(1), _probes(3), _probes(1)], "probe block")
    for a, b in zip(got[2], got[0]):
        _same(a, b, "one probe again")


def test_exact_film_finish_after_a_regrow(binding, rooms):
    """The exact finish's block (hits, keys and heads, entries) after a smaller render, after iile_test_patch_capacity forced it to
    another size, and over four passes; on a film whose samples do land on whole-number positions, so that the finish has hits to
    chain and entries to merge: pixels whose weight exceeds their own 16 samples."""
    assert rooms["strip"].film_shape == (32, 32)

    def forced(gpu):
        gpu.test_patch_capacity(8192)
        return (gpu.render()[0],)
    got = _walk(binding, rooms["strip"], [_render(k_begin=0, k_end=1), _render(), forced, _render(spp_per_pass=4)], "exact finish")
    assert (got[1][0][..., 3] > 16).sum() > 20   # samples that also landed in a neighbouring pixel
    _same(got[2][0], got[1][0], "forced capacity")
    _same(got[3][0], got[2][0], "four passes")


@pytest.mark.parametrize("room", ["plain", "mirror"])
def test_direct_pass_between_path_renders(binding, rooms, room):
    """The direct pass carves the path workspace its own way (NEE records per light sample); mirror: five levels of D / E / F."""
    direct = lambda gpu: (gpu.render_direct(2),)
    got = _walk(binding, rooms[room], [_render(), direct, _render(), direct], "direct " + room)
    _same(got[2][0], got[0][0], "path render again")
    _same(got[3][0], got[1][0], "direct pass again")


def test_direct_pass_accumulates_on_a_used_handle(binding, rooms):
    import torch

    def two_calls(gpu):
        film = torch.zeros((32, 32, 4), dtype=torch.float64, device="cuda")
        gpu.render_direct(1, film_device_ptr=film.data_ptr())
        gpu.render_direct(1, first_pass=1, film_device_ptr=film.data_ptr(), accumulate=True)
        torch.cuda.synchronize()
        return (film.cpu().numpy(),)
    got = _walk(binding, rooms["mirror"], [_render(), two_calls, two_calls], "direct accumulate")
    _same(got[2][0], got[1][0], "accumulated passes again")


@pytest.mark.parametrize("nn_on_device", [False, True])
def test_iispt_scratch(binding, rooms, nn_on_device):
    """One task, then three of different sizes (the scratch block grows), then the one task again."""
    import torch
    T = binding.IisptTask
    one, three = [T(0, 0, 8, 8, 4, 0, 1)], [T(0, 0, 32, 32, 8, 100, 2), T(4, 4, 20, 12, 3, 2000, 3), T(30, 30, 31, 31, 5, 4000, 4)]

    def batch(tasks):
        def call(gpu):
            valid, pos, dr = gpu.iispt_hemi_points_batch(tasks)
            nn = np.random.default_rng(len(valid)).uniform(0.0, 3.0, (len(valid), 32, 32, 3)).astype(np.float32)
            if nn_on_device:
                t = torch.from_numpy(nn).cuda()
                out = gpu.iispt_gather_batch(tasks, valid, pos, dr, nn_device_ptr=t.data_ptr())
            else:
                out = gpu.iispt_gather_batch(tasks, valid, pos, dr, nn)
            return valid, pos, dr, out
        return call
    got = _walk(binding, rooms["plain"], [batch(one), batch(three), batch(one)], "iispt scratch")
    for a, b in zip(got[2], got[0]):
        _same(a, b, "one task again")


def test_film_add_table(binding, rooms):
    import torch
    T = binding.IisptTask
    five = [T(0, 0, 16, 16, 4, 0, 0), T(16, 0, 32, 7, 4, 0, 0), T(16, 7, 32, 16, 4, 0, 0), T(0, 16, 31, 32, 4, 0, 0), T(31, 16, 32, 32, 4, 0, 0)]

    def add(tasks):
        def call(gpu):
            n_pix = sum((t.x1 - t.x0) * (t.y1 - t.y0) for t in tasks)
            out = torch.from_numpy(np.random.default_rng(n_pix).uniform(0, 2, (n_pix, 4)).astype(np.float32)).cuda()
            film = torch.ones((32, 32, 4), dtype=torch.float64, device="cuda")
            gpu.iispt_film_add(tasks, out.data_ptr(), film.data_ptr())
            torch.cuda.synchronize()
            return (film.cpu().numpy(),)
        return call
    got = _walk(binding, rooms["plain"], [add(five[:1]), add(five), add(five[:1])], "film_add")
    _same(got[2][0], got[0][0], "one task again")
