"""GPU suite (-m gpu): the production walks start at the ray's origin (bih_clip_root_at_origin, glome_amd/csrc/rt_device.hpp) and the cull pass
of the flagship launch decides with the same clipped interval (cull_kernels.hpp).  Neither the faithful instance (faithful=1) nor the
counting one (count_work=1) is clipped: every frame and every stream here must equal theirs bit for bit.

Frames: 200 x 136 over the terrain s3(32), maxdepth 1 -- the size at which tests/test_cull_pass.py has the flagship instance chosen (asserted
here too): 425 work items.  Streams: glome_trace_batch on two ladders of tests/ladder.py (along +x and -x: with the four tilt signs, all
eight octants), whose deep rays start inside the ladder's bounds; tests/test_origin_clip_host.py models that they still hold 16 pending
entries under the clipped interval."""
import ctypes as C

import numpy as np
import pytest

import ladder
from helpers import product_camera_lights
from glome_amd import _lib as L
from glome_amd import api, scenes

pytestmark = pytest.mark.gpu

W, H = 200, 136
RAY_KEYS = ("rays_primary", "rays_shadow", "rays_secondary")
HIT_KEYS = ("t", "prim", "n", "tex", "rgba", "depth")


def _params(**kw):
    return api.render_params(width=W, height=H, maxdepth=1, **kw)


def _last_cull(ctx):
    live, total = C.c_int64(-1), C.c_int64(-1)
    assert ctx.lib.glome_ctx_last_cull(ctx.h, C.byref(live), C.byref(total)) == 0, ctx.err()
    return live.value, total.value


def _two_rows(lib, builder, root, P, items):
    """two_rows of the launch's instance (glome_kernel_choice over the commit's own traits): 1 = the flagship"""
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(builder.h, root, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    row = np.array([list(t[:8]) + [P.mode, P.faithful, P.count_work, P.maxdepth, P.tile_stride, items]], dtype=np.int64)
    out = np.zeros((1, 4), dtype=np.int32)
    assert lib.glome_kernel_choice(1, row.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == 1
    return int(out[0, 2])


VIEWS = {
    "inside": lambda: api.camera((0.0, 0.5, 0.0), (5.0, 0.3, 5.0), (0.0, 1.0, 0.0), 45.0),  # the camera inside the root box: primary rays start inside too
    "bench": lambda: api.camera(*scenes.CUST_CAM),
    # above the terrain (its box ends at y = 1.55), looking straight up: every ray's BACKWARD extension enters the box through its top
    "up": lambda: api.camera_from_vectors((0.0, 6.0, 0.0), (0, 1, 0), (0, 0, 1), (1, 0, 0)),
}


@pytest.fixture(scope="module")
def terrain(gpu_ctx):
    sd = scenes.s3(32)
    b = api.Builder()
    nm, _ = sd.replay(b)
    sc = gpu_ctx.commit(b, nm[sd.root])
    items = int(gpu_ctx.lib.glome_items_layout(C.byref(_params()), 0, 1, 64, 1, None, 0))
    assert items == 425
    assert _two_rows(gpu_ctx.lib, b, nm[sd.root], _params(), items) == 1, "the flagship instance is not chosen at this size"
    assert _two_rows(gpu_ctx.lib, b, nm[sd.root], _params(faithful=1), items) == 0 and _two_rows(gpu_ctx.lib, b, nm[sd.root], _params(count_work=1), items) == 0
    lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
    yield gpu_ctx, sc, lights, items
    sc.release()


@pytest.mark.parametrize("view", ["inside", "bench", "up"])
def test_frames_equal_the_unclipped_instances(terrain, view):
    ctx, sc, lights, items = terrain
    cam = VIEWS[view]()
    img, packed, st = sc.render(cam, lights, _params())
    live, total = _last_cull(ctx)
    assert total == items
    for kw in ({"faithful": 1}, {"count_work": 1}, {"faithful": 1, "count_work": 1}):
        rimg, rpacked, rst = sc.render(cam, lights, _params(**kw))
        assert np.array_equal(img.view(np.uint32), rimg.view(np.uint32)), (view, kw, np.argwhere(img.view(np.uint32) != rimg.view(np.uint32))[:8])
        assert np.array_equal(packed, rpacked), (view, kw)
        assert [st[k] for k in RAY_KEYS] == [rst[k] for k in RAY_KEYS], (view, kw)
    assert st["rays_primary"] == W * H
    hit = img[..., 4] < 1.0e6
    if view == "up":
        # nothing of the terrain is in the frame, and no item is queued: the unclipped entry test let every one of them through
        # (tests/test_cull_pass.py's "down" view is this camera turned over)
        assert not hit.any() and st["rays_shadow"] == 0
        assert live == 0
    else:
        assert hit.any() and st["rays_shadow"] > 0
        assert 0 < live <= total
        blocks = hit.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))  # (the plan's items are the frame's aligned 8 x 8 blocks)
        assert live >= int(blocks.sum())


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              np.ascontiguousarray(b[k]).view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in HIT_KEYS)


@pytest.mark.parametrize("v", [(0, 1), (0, -1)], ids=["x+", "x-"])
def test_streams_from_inside_the_ladder(gpu_ctx, v):
    """glome_trace_batch, the early-out instance (the hand-written walk, closest hit and any hit: the shadow rays of the hits) against the
    faithful one, bit for bit, on rays that start inside the bounds: the deep stream (from the heavy end: 16 pending entries), the mixed
    stream (eight octants, lanes that run the comb backwards), and both again from the MIDDLE of the comb, forwards and backwards -- half
    of the tree lies behind such an origin."""
    lad = ladder.Ladder(*v)
    b = api.Builder()
    nm, _ = lad.sd.replay(b)
    sc = gpu_ctx.commit(b, nm[lad.sd.root])
    try:
        _, lights = product_camera_lights(lad.sd)
        do, dd, _ = lad.deep_set()
        mo, md, _ = lad.mixed_set()
        ro, rd = np.concatenate([do, mo]), np.concatenate([dd, md])
        u0, du = lad.local(ro)[:, 0], lad.local(rd)[:, 0]
        s = np.where(du > 0, (ladder.rung_u(8) * 1.3 - u0) / du, 0.0)  # the forward lanes moved to between rungs 8 and 7; the others stay
        mid = (ro.astype(np.float64) + s[:, None] * rd.astype(np.float64)).astype(np.float32)
        lo, hi = np.asarray(b.bound(nm[lad.bih_id])[:3]), np.asarray(b.bound(nm[lad.bih_id])[3:])
        # the deep stream starts inside the bounds; of the origins moved to the middle of the comb a third and more are still inside its thin
        # cross-section (a ray aimed at a near rung has left it by then: those start outside, beside the comb)
        assert np.all((do >= lo) & (do <= hi)) and np.all(du[:len(do)] > 0) and int(np.all((mid >= lo) & (mid <= hi), axis=1).sum()) >= 256
        octs, shadows = set(), 0
        for name, o, d in (("as drawn", ro, rd), ("from the middle", mid, rd), ("from the middle, backwards", mid, -rd)):
            octs |= set(((d[:, 0] > 0) * 1 + (d[:, 1] > 0) * 2 + (d[:, 2] > 0) * 4).tolist())
            r = sc.trace(o, d, lights, params=api.trace_params(maxdepth=3), want_hit=True)
            f = sc.trace(o, d, lights, params=api.trace_params(maxdepth=3, faithful=1), want_hit=True)
            bad = np.flatnonzero((r["t"].view(np.uint32) != f["t"].view(np.uint32)) | (r["prim"] != f["prim"]) | np.any(r["rgba"].view(np.uint32) != f["rgba"].view(np.uint32), axis=1))
            assert _same_bits(r, f), (name, bad[:16], len(bad))
            assert [r["stats"][k] for k in RAY_KEYS] == [f["stats"][k] for k in RAY_KEYS], name
            assert (r["t"] >= 0).sum() >= 64, name
            shadows += r["stats"]["rays_shadow"]
        assert shadows >= 64  # both modes walked: the hits' shadow rays leave from inside the bounds, in the any-hit mode
        assert octs == set(range(8))
    finally:
        sc.release()
