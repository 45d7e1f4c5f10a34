"""The lean render loop's per-item tables: the plan's item table (one entry per 64-pixel work item, built on the host beside the tile
table) and the two pixel-coordinate tables (filled on the device by get_coordsf itself).

CPU: the item table's decode gives, lane for lane, the pixel and the dense-payload offset of the tile arithmetic it replaces
(work_to_pixel), and both cover a plan's pixels exactly once.  GPU: the coordinate tables hold get_coordsf's bits, and a batch of 32
frames -- the path that splits a ticket into frame and item with a multiplier -- equals the frames rendered alone."""
import ctypes as C

import numpy as np
import pytest

from helpers import product_camera_lights
from glome_amd import _lib as L
from glome_amd import api, dist, scenes

# (width, height, blocksize of the params, blocksize override of the plan, tile_first, tile_stride)
PLANS = {
    "work_tiles_64_at_1920x1080": (1920, 1080, 65, 64, 0, 1),          # the whole-frame plan of the flagship: every item an 8x8 block
    "reference_tiles_65_with_leftover_strips": (1920, 1080, 65, 0, 0, 1),  # 65 = 8 * 8 + 1: a column and a row of leftovers per tile
    "sides_no_multiple_of_8_tiles_64": (191, 97, 65, 64, 0, 1),
    "sides_no_multiple_of_8_tiles_65": (191, 97, 65, 0, 0, 1),
    "dense_shard_stride_3_first_1_tiles_64": (1920, 1080, 64, 0, 1, 3),
    "dense_shard_stride_3_first_1_tiles_65": (333, 197, 65, 0, 1, 3),
}


def _layout(lib, P, first, stride, override, which):
    n = lib.glome_items_layout(C.byref(P), first, stride, override, which, None, 0)
    assert n >= 0
    out = np.full((max(n, 1), 64, 4), -7, dtype=np.int32)
    assert lib.glome_items_layout(C.byref(P), first, stride, override, which, out.ctypes.data_as(L.c_ip), n) == n
    return out[:n]


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_item_table_decode_equals_work_to_pixel_lane_for_lane(built, plan):
    w, h, bs, override, first, stride = PLANS[plan]
    lib = L.load()
    P = api.render_params(width=w, height=h, blocksize=bs, tile_first=first, tile_stride=stride)
    ref = _layout(lib, P, first, stride, override, 0)
    tab = _layout(lib, P, first, stride, override, 1)
    assert ref.shape == tab.shape and ref.shape[0] > 0
    assert np.array_equal(ref, tab), np.argwhere(ref != tab)[:8]
    # ... and what both say is a plan: every pixel of the owned tiles once, the dense offsets a permutation of the payload
    Pt = api.render_params(width=w, height=h, blocksize=override or bs, tile_first=first, tile_stride=stride)
    lay = dist.owned_layout(Pt, first, stride)
    owned = np.zeros((h, w), dtype=np.int32)
    off = np.full((h, w), -1, dtype=np.int32)  # a pixel's place in the dense payload: tiles in owned order, row major inside a tile
    npx = 0
    for x, y, tw, th, base in lay:
        owned[y:y + th, x:x + tw] += 1
        off[y:y + th, x:x + tw] = base + np.arange(tw * th, dtype=np.int32).reshape(th, tw)
        npx += tw * th
    valid = tab[..., 0] == 1
    assert int(valid.sum()) == npx
    seen = np.zeros((h, w), dtype=np.int32)
    np.add.at(seen, (tab[..., 2][valid], tab[..., 1][valid]), 1)
    assert np.array_equal(seen, owned)
    assert np.array_equal(tab[..., 3][valid], off[tab[..., 2][valid], tab[..., 1][valid]])
    if plan == "work_tiles_64_at_1920x1080":
        assert valid.all() and len(tab) == 32400


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1920, 1080), (191, 97)])
def test_coordinate_tables_hold_get_coordsf_bit_for_bit(gpu_ctx, w, h):
    got = [np.zeros(w, dtype=np.float32), np.zeros(h, dtype=np.float32)]
    ref = [np.ones(w, dtype=np.float32), np.ones(h, dtype=np.float32)]
    for arr, direct in ((got, 0), (ref, 1)):
        rc = gpu_ctx.lib.glome_ctx_coord_tables(gpu_ctx.h, w, h, arr[0].ctypes.data_as(L.c_fp), arr[1].ctypes.data_as(L.c_fp), direct)
        assert rc == 0, gpu_ctx.err()
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    # what get_coordsf is (Glome.hs:119-140): correctly rounded quotients, so the centre column of an even width is exactly 0
    x = np.arange(w, dtype=np.float32)
    q = (x.astype(np.float64) / np.float64(w)).astype(np.float32)
    aspect = np.float32(np.float64(np.float32(w)) / np.float64(np.float32(h)))
    assert np.allclose(got[0], (q.astype(np.float64) * 2 - 1) * aspect, rtol=0, atol=4e-7 * float(aspect))
    if w % 2 == 0:
        assert got[0][w // 2] == 0.0
    y = np.arange(h, dtype=np.float32)
    assert np.allclose(got[1], -((y.astype(np.float64) / h) * 2 - 1), rtol=0, atol=4e-7)


@pytest.mark.gpu
def test_batch_of_32_frames_equals_the_frames_alone_with_padding_chunks(gpu_ctx):
    """333 x 97 in 64 x 64 work tiles: an item count that is no multiple of a chunk of 64, so every frame's last chunk ends in padding
    tickets; the tiles of the right column and the bottom row have leftover strips."""
    import torch
    sd = scenes.s3(224)
    b = api.Builder()
    nm, _ = sd.replay(b)
    sc = gpu_ctx.commit(b, nm[sd.root])
    try:
        w, h, nframes = 333, 97, 32
        dev = torch.device("cuda:0")
        _, lights = product_camera_lights(sd)
        la = (L.Light * len(lights))(*lights)
        pos, at, up, ang = sd.cam
        views = [api.camera((pos[0] + 0.17 * f, pos[1] + 0.04 * (f % 5), pos[2] - 0.08 * f), at, up, ang) for f in range(nframes)]
        cams = (L.Camera * nframes)(*views)
        P = api.render_params(width=w, height=h, maxdepth=1)
        n_items = gpu_ctx.lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)
        assert n_items % 64 != 0  # padding tickets at the end of every frame's last chunk
        px = torch.zeros((nframes, h, w), dtype=torch.int32, device=dev)
        assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, nframes, la, len(lights), C.byref(P), C.c_void_p(px.data_ptr()), h * w, None) == 0, gpu_ctx.err()
        gpu_ctx.synchronize()
        got = px.cpu().numpy().view(np.uint32)
        one = torch.zeros((h, w), dtype=torch.int32, device=dev)
        for f in range(nframes):
            one.zero_()
            sc.render_dev(views[f], lights, P, None, one.data_ptr(), want_stats=False)
            gpu_ctx.synchronize()
            alone = one.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[f], alone), f
            assert alone.any(), f  # (the view sees the terrain: the comparison is of pictures, not of two empty frames)
    finally:
        sc.release()
