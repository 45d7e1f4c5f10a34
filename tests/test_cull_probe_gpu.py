"""The probe phase of the cull pass (glome_amd/csrc/cull_kernels.hpp): one ray of every work item -- lane 36 of its 64, the pixel at
(4, 4) of an 8 x 8 block -- proves the item live, and only the items whose probe ray misses are tested with all their rays.  A probe
can go wrong where the full test cannot: at the silhouette of the root bounds, where the probe ray misses and a neighbour enters; on
the degenerate centre column; in a leftover strip whose probe lane lies past its end; with several root entries; and with the chunks
of several frames in one launch.

test_cull_pass.py's setting: the terrain s3(N=32) at 200 x 136 (425 work items, seven chunks), one light, maxdepth 1; the flagship
instance is asserted through glome_kernel_choice and every frame is compared bit for bit with the faithful=1 render of the same view
(the every-class instance, which has no cull pass).

Which rays enter the root bounds is also worked out here, in float64 from the frame's rays (api.frame_rays) and the bounds of the
triangles, with a margin of 1e-3 in t on either side (the rays are the kernels' to an ulp, the frame's t values are of order 10): a
ray that enters the triangles' own bounds by the margin enters on the device, whose boxes are those bounds padded by 1e-4 a level, and
one that misses the bounds padded by 1e-3 by the margin misses there.  That shows that a view holds the items it is
meant to hold, and bounds `live` from below by the blocks that hold an entering ray -- more than the frame can show, since a ray may
enter the bounds and hit nothing.
"""
import ctypes as C
import math

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

W, H = 200, 136
PROBE_X, PROBE_Y = 4, 4  # lane 36 of an 8 x 8 block
MARGIN = 1.0e-3  # in t
PAD = 1.0e-3     # in space: ten times the pad the scene's boxes carry (bbpts' delta, 1e-4 per level)


def _rotated(cam, pitch=0.0, roll=0.0):
    """`cam` pitched (about its right vector, radians, up positive) and then rolled (about its new forward vector)"""
    f, u, r = (np.array(list(v), np.float64) for v in (cam.fwd, cam.up, cam.right))
    f, u = f * math.cos(pitch) + u * (np.linalg.norm(f) / np.linalg.norm(u)) * math.sin(pitch), u * math.cos(pitch) - f * (np.linalg.norm(u) / np.linalg.norm(f)) * math.sin(pitch)
    u, r = u * math.cos(roll) + r * (np.linalg.norm(u) / np.linalg.norm(r)) * math.sin(roll), r * math.cos(roll) - u * (np.linalg.norm(r) / np.linalg.norm(u)) * math.sin(roll)
    return api.camera_from_vectors(list(cam.pos), f, u, r)


def _bounds(tris):
    p = np.asarray(tris, np.float64).reshape(-1, 3)
    return p.min(axis=0), p.max(axis=0)


def _enters(cam, lo, hi, w=W, h=H):
    """(enters, misses): (h, w) masks of the rays that enter the box [lo, hi] in front of the camera by MARGIN, and that miss it by
    MARGIN.  A ray with a zero direction component is in neither."""
    o, d = api.frame_rays(cam, w, h)
    o, d = o.astype(np.float64), d.astype(np.float64)
    known = (np.abs(d) > 1e-9).all(axis=1)

    def interval(pad):
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - pad - o) / d, (hi + pad - o) / d
        return np.maximum(np.minimum(t0, t1).max(axis=1), 0.0), np.maximum(t0, t1).min(axis=1)
    near, far = interval(0.0)
    near_p, far_p = interval(PAD)
    return (known & (near < far - MARGIN)).reshape(h, w), (known & (near_p > far_p + MARGIN)).reshape(h, w)


def _blocks(mask):
    """(H, W) pixels -> (H / 8, W / 8): the plan's items are the frame's aligned 8 x 8 blocks"""
    return mask.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))


def _probe(mask):
    return mask[PROBE_Y::8, PROBE_X::8]


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


def _hit(img):
    """pixels with a finite depth: a miss stores the reference's `infinity`, 1e6 (Vec.hs:14)"""
    return img[..., 4] < 1.0e6


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


class _Case:
    """a committed scene with its lights and the boxes of its root entries; the flagship instance is asserted"""

    def __init__(self, ctx, sd, boxes):
        self.ctx, self.boxes = ctx, boxes
        b = api.Builder()
        nm, _ = sd.replay(b)
        self.sc = ctx.commit(b, nm[sd.root])
        self.lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
        self.items = int(ctx.lib.glome_items_layout(C.byref(_params()), 0, 1, 64, 1, None, 0))
        assert self.items == (W // 8) * (H // 8)
        assert _choice(ctx.lib, b, nm[sd.root], _params(), self.items) == 1, "the flagship instance is not chosen at this size"
        assert _choice(ctx.lib, b, nm[sd.root], _params(faithful=1), self.items) == 0

    def check(self, cam):
        """the flagship frame of `cam` against the faithful one, bit for bit; -> (faithful image, live): live is bounded from below by the
        blocks that hold a hit pixel and by those that hold a ray entering a root box, from above by those no ray of which misses all"""
        ref_img, ref_packed, ref_st = self.sc.render(cam, self.lights, _params(faithful=1))
        img, packed, st = self.sc.render(cam, self.lights, _params())
        live, total = _last_cull(self.ctx)
        assert _same_bits(img, ref_img), np.argwhere(img.view(np.uint32) != ref_img.view(np.uint32))[:8]
        assert np.array_equal(packed, ref_packed), np.argwhere(packed != ref_packed)[:8]
        assert st["rays_primary"] == W * H
        assert st["rays_shadow"] == ref_st["rays_shadow"]
        assert total == self.items
        assert live >= int(_blocks(_hit(ref_img)).sum())
        enters, misses = self.enters(cam)
        assert int(_blocks(enters).sum()) <= live <= int(_blocks(~misses).sum())
        return ref_img, live

    def enters(self, cam):
        """a ray enters if it enters any entry's box, and misses if it misses every one"""
        per = [_enters(cam, lo, hi) for lo, hi in self.boxes]
        return np.any([e for e, _ in per], axis=0), np.all([m for _, m in per], axis=0)


def _two_terrains():
    """test_cull_pass.py's: the terrain and a copy 20 units further along x, each a triangle BIH of its own -- two root entries"""
    sd = SceneDesc()
    mat = scenes.matte(sd, (0.8, 0.5, 0.4))
    t = scenes.heightfield_triangles(32)
    t2 = t.copy()
    t2[:, 0::3] += 20.0
    sd.set_root(sd.group([sd.tex(sd.bih(sd.triangles_bulk(t)), mat), sd.tex(sd.bih(sd.triangles_bulk(t2)), mat)]))
    scenes._common(sd, 1)
    return sd, [_bounds(t), _bounds(t2)]


@pytest.fixture(scope="module")
def terrain(gpu_ctx):
    c = _Case(gpu_ctx, scenes.s3(32), [_bounds(scenes.heightfield_triangles(32))])
    yield c
    c.sc.release()


@pytest.fixture(scope="module")
def two_terrains(gpu_ctx):
    sd, boxes = _two_terrains()
    c = _Case(gpu_ctx, sd, boxes)
    yield c
    c.sc.release()


ROW = math.atan(2.0 / H * math.tan(math.radians(22.5)))  # a pitch of one pixel row at the frame's centre (yc runs over [-1, 1] in H rows; |up| / |fwd| = tan(45 / 2))


def _pitched(k, roll_deg):
    return _rotated(api.camera(*scenes.CUST_CAM), pitch=k * ROW, roll=math.radians(roll_deg))


@pytest.mark.gpu
@pytest.mark.parametrize("roll_deg", [0, 30])
def test_silhouette_at_every_offset_inside_a_block(terrain, roll_deg):
    """The camera pitched by 0..7 pixel rows: the far edge of the root box -- the straight line above which every ray misses -- falls on
    each of the eight rows of the blocks it crosses, and with a roll of 30 degrees it crosses their columns too.  The items on it whose
    probe ray misses while another ray enters must stay live."""
    rows = set()
    for k in range(8):
        cam = _pitched(k, roll_deg)
        enters, misses = terrain.enters(cam)
        on_edge = _blocks(enters) & _probe(misses)
        assert on_edge.any(), (k, "no item whose probe ray misses while another ray of it enters")
        _, live = terrain.check(cam)
        assert 0 < live < terrain.items
        if roll_deg == 0:
            # the first row of the frame's centre columns with an entering ray: it moves down a row per step
            rows.add(int(np.argmax(enters[:, W // 2 - 3])) % 8)
    if roll_deg == 0:
        assert rows == set(range(8)), rows


@pytest.mark.gpu
def test_the_probe_pixel_on_the_degenerate_column(terrain):
    """An axis-aligned camera on an even width: the rays of column W / 2 have an exactly zero x component and the slab test misses for
    them by construction.  W / 2 = 100 = 12 * 8 + 4 is the probe lane's column: the probe of every item of that column of blocks misses,
    and those over the terrain are live by their other rays."""
    assert (W // 2) % 8 == PROBE_X
    cam = api.camera_from_vectors((0.0, 3.0, 15.0), (0, 0, -1), (0, 1, 0), (1, 0, 0))
    _, d = api.frame_rays(cam, W, H)
    assert (d.reshape(H, W, 3)[:, W // 2, 0] == 0).all()
    img, live = terrain.check(cam)
    hit = _hit(img)
    assert not hit[:, W // 2].any() and hit[:, W // 2 - 1].any()  # the centre column is empty in the reference too
    assert _blocks(hit)[:, (W // 2) // 8].any()                     # ... and its blocks are not
    assert 0 < live < terrain.items


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["second_only", "edge_of_the_first"])
def test_two_root_entries(two_terrains, view):
    """second_only: from in front of the copy, probe rays that miss the first terrain's box and enter the second's.  edge_of_the_first: the
    copy out of the frame on the right, the first terrain's silhouette in it -- probe rays that miss both boxes while another ray of the
    item enters the first."""
    c = two_terrains
    if view == "second_only":
        cam = api.camera((22.0, 4.3, 15.0), (22.0, 2.0, 0.0), (0.0, 1.0, 0.0), 45.0)
    else:
        cam = _rotated(api.camera((-12.0, 4.3, 15.0), (-12.0, 2.0, 0.0), (0.0, 1.0, 0.0), 45.0), pitch=3 * ROW, roll=math.radians(10.0))
    (e1, m1), (e2, m2) = (_enters(cam, lo, hi) for lo, hi in c.boxes)
    if view == "second_only":
        assert (_probe(m1) & _probe(e2)).any()
    else:
        assert (_probe(m1 & m2) & _blocks(e1)).any()
    _, live = c.check(cam)
    assert 0 < live < c.items


@pytest.mark.gpu
def test_leftover_strips_of_a_ranks_dense_payload(gpu_ctx):
    """The second of two ranks, 65 x 65 tiles, a dense packed payload (3072 x 2048: a shard takes the flagship from 48,000 work items
    on).  A 65 x 65 tile has 129 leftover pixels, packed 64 to an item: the third such item holds one pixel, and the strip items of the
    tiles at the frame's right and bottom end early too -- their probe lane lies past their end, and lane 0 probes."""
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
        for faithful in (1, 0):
            P = api.render_params(width=3072, height=2048, maxdepth=1, tile_first=1, tile_stride=2, faithful=faithful)
            items = int(gpu_ctx.lib.glome_items_layout(C.byref(P), 1, 2, 0, 1, None, 0))
            assert _choice(gpu_ctx.lib, b, nm[sd.root], P, items) == 1 - faithful
            npx = int(gpu_ctx.lib.glome_tiles_payload_floats(C.byref(P), 1, 2)) // 5
            buf = torch.full((npx,), 0x55555555, dtype=torch.int32, device=torch.device("cuda:0"))
            assert sc.lib.glome_render_tiles_packed_dev(sc.h, C.byref(cam), la, len(lights), C.byref(P), C.c_void_p(buf.data_ptr()), None) == 0, gpu_ctx.err()
            gpu_ctx.synchronize()
            out[faithful] = buf.cpu().numpy().view(np.uint32)
            if not faithful:
                live, total = _last_cull(gpu_ctx)
                assert total == items and 0 < live < total
        assert np.array_equal(out[0], out[1]), np.argwhere(out[0] != out[1])[:8]
        assert out[1].any() and not (out[0] == 0x55555555).any()  # a picture, and every pixel of the payload written
    finally:
        sc.release()


@pytest.mark.gpu
@pytest.mark.parametrize("nframes", [5, 32])
def test_batches_of_different_views(terrain, nframes):
    """Frames of different views in one launch -- the pitched and rolled silhouettes, the view from above (all live), and the view away
    from the terrain (nothing live) between them: a block's probe runs with its chunk's frame's camera.  Each frame equals that view
    rendered alone, and the launch's live count is the sum of the single launches'."""
    import torch
    ctx, sc = terrain.ctx, terrain.sc
    pos = scenes.CUST_CAM[0]
    away = api.camera((pos[0], 40.0, pos[2]), (pos[0], 44.0, pos[2] + 15.0), (0.0, 1.0, 0.0), 45.0)
    down = api.camera_from_vectors((0.0, 6.0, 0.0), (0, -1, 0), (0, 0, -1), (1, 0, 0))
    views = []
    for f in range(nframes):
        views.append(away if f % 4 == 1 else (down if f % 8 == 6 else _pitched(f % 8, 30 * (f % 3 == 0) + f)))
    dev = torch.device("cuda:0")
    cams = (L.Camera * nframes)(*views)
    la = (L.Light * len(terrain.lights))(*terrain.lights)
    P = _params()
    px = torch.full((nframes, H, W), 0x55555555, dtype=torch.int32, device=dev)
    st = L.Stats()
    assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, nframes, la, len(terrain.lights), C.byref(P), C.c_void_p(px.data_ptr()), H * W, C.byref(st)) == 0, ctx.err()
    got = px.cpu().numpy().view(np.uint32)
    live, total = _last_cull(ctx)
    assert total == nframes * terrain.items
    one = torch.zeros((H, W), dtype=torch.int32, device=dev)
    lives = []
    for f, cam in enumerate(views):
        one.fill_(0x55555555)
        sc.render_dev(cam, terrain.lights, P, None, one.data_ptr(), want_stats=False)
        ctx.synchronize()
        lives.append(_last_cull(ctx)[0])
        assert np.array_equal(got[f], one.cpu().numpy().view(np.uint32)), f
        assert np.array_equal(got[f], sc.render(cam, terrain.lights, _params(faithful=1))[1]), f
    assert lives[1] == 0 and 0 < lives[0] < terrain.items and (nframes < 7 or lives[6] == terrain.items)
    assert live == sum(lives)
    assert st.rays_primary == W * H * nframes
