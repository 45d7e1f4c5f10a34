"""The cull pass of a flagship launch (glome_amd/csrc/cull_kernels.hpp): work items whose rays all miss the scene's root bounds are
finished before the render kernel and never queued; the live ones become the slot's ticket list.

Every comparison is with the same view rendered with faithful=1: the every-class instance, which has no cull pass and which the
project already holds bit-identical to the flagship.  The frame is 200 x 136 over the terrain s3(N=32) -- the flagship instance is
chosen at this size (asserted through glome_kernel_choice) --, maxdepth 1, one light: 25 x 17 = 425 work items of 8 x 8 pixels in
64 x 64 work tiles with an 8-pixel column and row of tiles at the right and the bottom, seven chunks of 64 the last of which is
partly filled.
"""
import ctypes as C
import math

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

W, H = 200, 136
POS = scenes.CUST_CAM[0]


def _views():
    """name -> glome_camera.  The terrain's box is x, z in [-10, 10], y in about [-1.5, 1.55]."""
    roll = math.radians(30.0)
    return {
        "horizon": api.camera(*scenes.CUST_CAM),                                             # the horizon through the middle of the frame
        # looking away, from high above: the terrain behind and below the camera.  The walk's entry test does not clip an interval at
        # t = 0, so a ray whose backward extension crosses the box "enters" it (and then hits nothing); from y = 40 no line does: live == 0
        "away": api.camera((POS[0], 40.0, POS[2]), (POS[0], 44.0, POS[2] + 15.0), (0.0, 1.0, 0.0), 45.0),
        "down": api.camera_from_vectors((0.0, 6.0, 0.0), (0, -1, 0), (0, 0, -1), (1, 0, 0)),  # every ray enters the box through its top: live == total
        "inside": api.camera((0.0, 0.5, 0.0), (5.0, 0.3, 5.0), (0.0, 1.0, 0.0), 45.0),        # the camera inside the root box
        # an axis-aligned camera on an even width: the centre column's rays have an exactly zero x component, and the slab test misses for them
        "axis_aligned": api.camera_from_vectors((0.0, 3.0, 15.0), (0, 0, -1), (0, 1, 0), (1, 0, 0)),
        "rolled_30": api.camera(scenes.CUST_CAM[0], scenes.CUST_CAM[1], (math.sin(roll), math.cos(roll), 0.0), 45.0),  # the silhouette crosses chunk corners diagonally
    }


def _two_terrains():
    """two root entries: the terrain and a copy 20 units further along x, each a triangle BIH of its own"""
    sd = SceneDesc()
    mat = scenes.matte(sd, (0.8, 0.5, 0.4))
    t = scenes.heightfield_triangles(32)
    t2 = t.copy()
    t2[:, 0::3] += 20.0
    sd.set_root(sd.group([sd.tex(sd.bih(sd.triangles_bulk(t)), mat), sd.tex(sd.bih(sd.triangles_bulk(t2)), mat)]))
    scenes._common(sd, 1)
    return sd


def _choice(lib, builder, root, P, items):
    """two_rows of the launch's instance (glome_kernel_choice over the commit's own traits): 1 = the flagship"""
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(builder.h, root, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    row = np.array([list(t[:8]) + [P.mode, P.faithful, P.count_work, P.maxdepth, P.tile_stride, items]], dtype=np.int64)
    out = np.zeros((1, 4), dtype=np.int32)
    assert lib.glome_kernel_choice(1, row.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == 1
    return int(out[0, 2])


def _params(**kw):
    return api.render_params(width=W, height=H, maxdepth=1, **kw)


def _last_cull(ctx):
    live, total = C.c_int64(-1), C.c_int64(-1)
    assert ctx.lib.glome_ctx_last_cull(ctx.h, C.byref(live), C.byref(total)) == 0, ctx.err()
    return live.value, total.value


class _Case:
    """a committed scene, its lights, and the faithful reference of every (view, fog) asked for, rendered once"""

    def __init__(self, ctx, sd):
        self.ctx = ctx
        b = api.Builder()
        nm, _ = sd.replay(b)
        self.sc = ctx.commit(b, nm[sd.root])
        self.lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
        self.views = _views()
        self.items = int(ctx.lib.glome_items_layout(C.byref(_params()), 0, 1, 64, 1, None, 0))
        assert self.items == 425
        assert _choice(ctx.lib, b, nm[sd.root], _params(), self.items) == 1, "the flagship instance is not chosen at this size"
        assert _choice(ctx.lib, b, nm[sd.root], _params(faithful=1), self.items) == 0
        self._ref = {}

    def ref(self, view, fog=0):
        if (view, fog) not in self._ref:
            img, packed, st = self.sc.render(self.views[view], self.lights, _params(faithful=1, fog=fog))
            img.setflags(write=False); packed.setflags(write=False)
            self._ref[(view, fog)] = (img, packed, st)
        return self._ref[(view, fog)]


@pytest.fixture(scope="module")
def terrain(gpu_ctx):
    c = _Case(gpu_ctx, scenes.s3(32))
    yield c
    c.sc.release()


@pytest.fixture(scope="module")
def two_terrains(gpu_ctx):
    c = _Case(gpu_ctx, _two_terrains())
    yield c
    c.sc.release()


def _hit(img):
    """pixels with a finite depth: a miss stores the reference's `infinity`, 1e6 (Vec.hs:14)"""
    return img[..., 4] < 1.0e6


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_view(case, view):
    for fog in (0, 1):
        ref_img, ref_packed, ref_st = case.ref(view, fog)
        img, packed, st = case.sc.render(case.views[view], case.lights, _params(fog=fog))
        assert _same_bits(img, ref_img), (view, fog, np.argwhere(img.view(np.uint32) != ref_img.view(np.uint32))[:8])
        if fog == 0:
            assert np.array_equal(packed, ref_packed), (view, np.argwhere(packed != ref_packed)[:8])
        # the counters: every pixel's primary ray is counted, by the cull pass or by the render kernel; the shadow rays are the hits'
        assert st["rays_primary"] == W * H, (view, fog)
        assert st["rays_shadow"] == ref_st["rays_shadow"], (view, fog)


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["horizon", "away", "down", "inside", "axis_aligned", "rolled_30"])
def test_frames_byte_identical_to_the_faithful_render(terrain, view):
    """packed, out5 and out5 with fog, and the ray counters of the launch"""
    _check_view(terrain, view)
    img = terrain.ref(view)[0]
    if view == "away":
        assert not _hit(img).any()   # (nothing of the terrain in the frame)
    else:
        assert _hit(img).any()       # (the comparison is of pictures)
    if view == "axis_aligned":
        assert not _hit(img)[:, W // 2].any() and _hit(img)[:, W // 2 - 1].any()  # the centre column is empty in the reference too


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["horizon", "away", "rolled_30"])
def test_several_root_entries(two_terrains, view):
    """Two terrains side by side: a root list of two triangle BIHs selects the flagship instance (asserted by the fixture), and an item is
    dead only when its rays miss both."""
    _check_view(two_terrains, view)
    if view == "horizon":
        live2, total2 = _last_cull(two_terrains.ctx)
        assert total2 == two_terrains.items and 0 < live2 < total2


@pytest.mark.gpu
def test_last_cull_reports_what_was_queued(terrain):
    ctx, sc = terrain.ctx, terrain.sc
    for view in ("away", "down", "horizon"):
        sc.render(terrain.views[view], terrain.lights, _params())
        live, total = _last_cull(ctx)
        assert total == terrain.items
        if view == "away":
            assert live == 0
        elif view == "down":
            assert live == total
        else:
            assert 0 < live < total
            hit = _hit(terrain.ref(view)[0])
            blocks = hit.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))  # (the plan's items are the frame's aligned 8 x 8 blocks)
            assert live >= int(blocks.sum())


@pytest.mark.gpu
def test_batch_of_five_frames_with_empty_frames_between(terrain):
    """horizon, away, down, horizon, away in one launch: the interleaved order, chunk by chunk through the frames, with frames that queue nothing"""
    import torch
    ctx, sc = terrain.ctx, terrain.sc
    names = ["horizon", "away", "down", "horizon", "away"]
    dev = torch.device("cuda:0")
    cams = (L.Camera * len(names))(*[terrain.views[n] for n in names])
    la = (L.Light * len(terrain.lights))(*terrain.lights)
    P = _params()
    px = torch.full((len(names), H, W), 0x55555555, dtype=torch.int32, device=dev)
    st = L.Stats()
    assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, len(names), la, len(terrain.lights), C.byref(P), C.c_void_p(px.data_ptr()), H * W, C.byref(st)) == 0, ctx.err()
    got = px.cpu().numpy().view(np.uint32)
    live, total = _last_cull(ctx)
    assert total == len(names) * terrain.items
    one = torch.zeros((H, W), dtype=torch.int32, device=dev)
    lives = {}
    for f, n in enumerate(names):
        one.fill_(0x55555555)
        sc.render_dev(terrain.views[n], terrain.lights, P, None, one.data_ptr(), want_stats=False)
        ctx.synchronize()
        lives[n] = _last_cull(ctx)[0]
        assert np.array_equal(got[f], one.cpu().numpy().view(np.uint32)), (f, n)
        assert np.array_equal(got[f], terrain.ref(n)[1]), (f, n)
    assert live == sum(lives[n] for n in names)
    assert st.rays_primary == W * H * len(names)
    assert st.rays_shadow == sum(terrain.ref(n)[2]["rays_shadow"] for n in names)


@pytest.mark.gpu
def test_back_to_back_launches_on_one_slot(terrain):
    """An all-sky launch, then a horizon launch, nothing in between: the queue heads, the dry mask and the list length are left ready by
    the first launch's own waves and cull pass."""
    import torch
    ctx, sc = terrain.ctx, terrain.sc
    dev = torch.device("cuda:0")
    P = _params()
    a = torch.full((H, W), 0x55555555, dtype=torch.int32, device=dev)
    b = torch.full((H, W), 0x55555555, dtype=torch.int32, device=dev)
    c = torch.full((H, W), 0x55555555, dtype=torch.int32, device=dev)
    sc.render_dev(terrain.views["away"], terrain.lights, P, None, a.data_ptr(), want_stats=False)
    sc.render_dev(terrain.views["horizon"], terrain.lights, P, None, b.data_ptr(), want_stats=False)
    sc.render_dev(terrain.views["away"], terrain.lights, P, None, c.data_ptr(), want_stats=False)
    ctx.synchronize()
    assert np.array_equal(a.cpu().numpy().view(np.uint32), terrain.ref("away")[1])
    assert np.array_equal(b.cpu().numpy().view(np.uint32), terrain.ref("horizon")[1])
    assert np.array_equal(c.cpu().numpy().view(np.uint32), terrain.ref("away")[1])
    assert _last_cull(ctx) == (0, terrain.items)


@pytest.mark.gpu
def test_a_ranks_shard_dense_packed_payload(gpu_ctx):
    """tile_stride=2 with a dense packed payload.  choose_render takes the flagship for a shard from 48,000 work items on: 3072 x 2048 in
    65 x 65 tiles, every second one, is 50,672 -- and these tiles have leftover strips, whose items the cull pass decodes through the
    tile table."""
    import torch
    sd = scenes.s3(32)
    b = api.Builder()
    nm, _ = sd.replay(b)
    sc = gpu_ctx.commit(b, nm[sd.root])
    try:
        lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
        la = (L.Light * len(lights))(*lights)
        cam = api.camera(*scenes.CUST_CAM)
        out = {}
        for faithful in (0, 1):
            P = api.render_params(width=3072, height=2048, maxdepth=1, tile_first=0, tile_stride=2, faithful=faithful)
            items = int(gpu_ctx.lib.glome_items_layout(C.byref(P), 0, 2, 0, 1, None, 0))
            assert _choice(gpu_ctx.lib, b, nm[sd.root], P, items) == 1 - faithful
            npx = int(gpu_ctx.lib.glome_tiles_payload_floats(C.byref(P), 0, 2)) // 5
            buf = torch.full((npx,), 0x55555555, dtype=torch.int32, device=torch.device("cuda:0"))
            assert sc.lib.glome_render_tiles_packed_dev(sc.h, C.byref(cam), la, len(lights), C.byref(P), C.c_void_p(buf.data_ptr()), None) == 0, gpu_ctx.err()
            gpu_ctx.synchronize()
            out[faithful] = buf.cpu().numpy().view(np.uint32)
            if not faithful:
                live, total = _last_cull(gpu_ctx)
                assert total == items and 0 < live < total
        assert np.array_equal(out[0], out[1]), np.argwhere(out[0] != out[1])[:8]
        assert out[1].any()
    finally:
        sc.release()
