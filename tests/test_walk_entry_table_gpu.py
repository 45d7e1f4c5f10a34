"""GPU suite (-m gpu): the kernels that read the walk-entry table (glome_amd/csrc/rt_types.h DScene::walk) against the kernels that do not.

The flagship render instance and its cull pass take a root entry's flags and header index from one record of the table (rt_device.hpp
closest_flat / occluded_flat with TABLE, cull_kernels.hpp lane_enters); every other instance reads `entries` and `recs` -- the two two-row
sampler instances among them, which rely on the same admission rule (every root entry a triangle bih) and are held here as well.  The
same view under faithful=1 runs the every-class instance (the sampler: its three-row instance), so a frame of the one must equal the frame
of the other bit for bit -- the comparison of tests/test_flagship_shading_gpu.py, whose `_choice` and `_same_bits` are used here; every
case asserts through glome_kernel_choice that its launch gets the two-row instance and its reference does not.

Scenes.  The two-row rule admits a scene only when its deepest tree fills the hand-written walk's stack (instances.hpp use_two_rows:
stack_cap == kAsmLdsCap), so every scene holds the terrain of scenes.s3(32) as one entry -- a real walk -- and beside it bihs of 4
triangles (a root that is a single leaf, tested regardless of its interval) and of 16 to 64 (a shallow walk): one bih; three bihs; a
NoShadow and an OnlyShadow entry; bihs under one and two Tex levels next to a bare one; an entry that is not visible.  Frames 24 x 16
and 72 x 40 (the sampler's 65-pixel tiles leave strips in the second), and 75 x 43, which has a leftover strip in renderTile's
64 x 64 work tiles as well.  A one-frame launch and a three-frame batch.  Then the same after every update call a committed triangle bih
has -- bih_update, bih_update_f32, bih_update_indexed; bih_refit is refused for such a tree, which holds no object to refit from, and
must leave the scene as it was -- which is what would catch a table word that an update rewrites.

The cull pass (glome_ctx_last_cull): `total` is the launch's item count, `live` lies between the items that hold a pixel with a hit,
counted here from the reference frame, and `total`; and `live` is the number the parent of this change queued for the same launch
(LIVE below: recorded once from a build of the parent commit, the same on both).

The two-row sampler is two instances of one source: four waves per SIMD, and five for a tree of more than 500,000 nodes
(instances.hpp choose_sampler).  The second gets the NoShadow / OnlyShadow scene over a terrain of 576 x 576 cells, whose tree has about
530,000 nodes (the host builder makes it in under a second); each case asserts the waves of the instance it is given.
"""
import ctypes as C

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc
from test_flagship_shading_gpu import _choice, _same_bits

pytestmark = pytest.mark.gpu

FRAMES = [(24, 16), (72, 40), (75, 43)]
N = 32
BIG = 576  # the terrain whose tree has more than 500,000 nodes


def _terrain(sd, n=N):
    return sd.bih(sd.triangles_bulk(scenes.heightfield_triangles(n).copy()))


def _patch(n, dx=0.0, dy=0.0, dz=0.0, seed=1):
    """n small triangles scattered over a 3 x 3 patch a little above the ground"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.5, 1.5, (n, 1, 3)) * np.array([1, 0.1, 1]) + rng.uniform(-0.4, 0.4, (n, 3, 3))
    p += np.array([dx, 2.0 + dy, dz])
    return p.reshape(n, 9)


def _small(sd, n, **kw):
    return sd.bih(sd.triangles_bulk(_patch(n, **kw)))


def _one():
    sd = SceneDesc()
    sd.bihs = {"terrain": _terrain(sd)}
    sd.set_root(sd.tex(sd.bihs["terrain"], scenes.matte(sd, (0.8, 0.5, 0.4))))
    return sd


def _three():
    sd = SceneDesc()
    m1, m2 = scenes.matte(sd, (0.8, 0.5, 0.4)), scenes.matte(sd, (0.2, 0.7, 0.3))
    sd.bihs = {"terrain": _terrain(sd), "leaf": _small(sd, 4, dx=-2.0), "walk": _small(sd, 64, dx=2.0, dz=1.0, seed=2)}
    sd.set_root(sd.group([sd.tex(sd.bihs["terrain"], m1), sd.tex(sd.bihs["leaf"], m2), sd.tex(sd.bihs["walk"], m2)]))
    return sd


class _Direct(api.Builder):
    """a builder that takes a scene function's calls itself: a terrain of BIG x BIG cells without a SceneDesc's copy of it"""
    def set_root(self, root):
        self.root = root


def _flags(n=N, sd=None):
    """the terrain; a bih under NoShadow (seen, casts nothing); a bih above both under OnlyShadow (not visible, shades what lies under it)"""
    sd = sd or SceneDesc()
    m1, m2 = scenes.matte(sd, (0.8, 0.5, 0.4)), scenes.matte(sd, (0.2, 0.7, 0.3))
    sd.bihs = {"terrain": _terrain(sd, n), "leaf": _small(sd, 4, dx=-1.0), "walk": _small(sd, 64, dy=1.5, seed=3)}
    sd.set_root(sd.group([sd.tex(sd.bihs["terrain"], m1), sd.noshadow(sd.tex(sd.bihs["leaf"], m2)), sd.onlyshadow(sd.tex(sd.bihs["walk"], m1))]))
    return sd


def _texed():
    """two Tex levels over the terrain, one over a small walk, none over a root leaf (its hits: the transparent pixel with a finite depth)"""
    sd = SceneDesc()
    inner = sd.material_surface((0.8, 0.5, 0.4), 0.5, 0.2, 1, 0, 0)
    outer = sd.material_surface((0.1, 0.6, 0.9), 1, 0.3, 0.7, 0, 0)
    sd.bihs = {"terrain": _terrain(sd), "leaf": _small(sd, 4, dx=1.5), "walk": _small(sd, 16, dx=-1.5, seed=4)}
    sd.set_root(sd.group([sd.tex(sd.tex(sd.bihs["terrain"], inner), outer), sd.bihs["leaf"], sd.tex(sd.bihs["walk"], outer)]))
    return sd


SCENES = {"one_bih": _one, "three_bihs": _three, "noshadow_and_onlyshadow": _flags, "tex_levels_and_a_bare_bih": _texed}

# live items of the one-frame launch, view -> per frame of FRAMES: what the parent commit's cull pass queued (see the docstring).  One
# table for the four scenes: the parent queued the same items for each (the terrain, which all four hold, is what these views see).
LIVE = {"horizon": [3, 27, 32], "down": [6, 45, 51]}


def _views():
    return {"horizon": api.camera(*scenes.CUST_CAM),
            "down": api.camera_from_vectors((0.0, 6.0, 0.0), (0, -1, 0), (0, 0, -1), (1, 0, 0))}


def _params(w, h, **kw):
    return api.render_params(width=w, height=h, maxdepth=1, **kw)


def _last_cull(ctx):
    live, total = C.c_int64(-1), C.c_int64(-1)
    assert ctx.lib.glome_ctx_last_cull(ctx.h, C.byref(live), C.byref(total)) == 0, ctx.err()
    return live.value, total.value


def _items(lib, P):
    """the lanes of the work items of renderTile's plan (64 x 64 work tiles): [items, 64, (valid, x, y, offset)]"""
    n = int(lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0))
    out = np.zeros((n, 64, 4), np.int32)
    assert lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, out.ctypes.data_as(L.c_ip), n) == n
    return out


class Committed:
    def __init__(self, ctx, name, make=None):
        sd = (make or SCENES[name])()
        self.name, self.ctx = name, ctx
        if isinstance(sd, _Direct):
            self.b, self.root, self.bihs, sd = sd, sd.root, sd.bihs, SceneDesc()
            scenes._common(sd, 1)
        else:
            scenes._common(sd, 1)
            self.b = api.Builder()
            nm, _ = sd.replay(self.b)
            self.root, self.bihs = nm[sd.root], {k: nm[v] for k, v in sd.bihs.items()}
        self.sc = ctx.commit(self.b, self.root)
        self.lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]

    def check_choice(self, mode):
        lib = self.ctx.lib
        kind, inst, two = _choice(lib, self.b, self.root, _params(24, 16, mode=mode))
        assert (kind, two) == (mode, 1) and (inst >> 3) & 1 == 1, "the two-row instance is not chosen for this scene"
        assert _choice(lib, self.b, self.root, _params(24, 16, mode=mode, faithful=1))[2] == 0

    def compare(self, frames=FRAMES, live_of=None):
        """every view and frame: the flagship launch against the every-class one, and the cull pass's counts (live_of: view -> the
        parent's live counts per frame of FRAMES, for the scene as committed)"""
        hits = 0
        for view, cam in _views().items():
            for fi, (w, h) in enumerate(frames):
                for fog in ((0, 1) if (w, h) == FRAMES[1] else (0,)):
                    ref, ref_packed, ref_st = self.sc.render(cam, self.lights, _params(w, h, faithful=1, fog=fog))
                    img, packed, st = self.sc.render(cam, self.lights, _params(w, h, fog=fog))
                    live, total = _last_cull(self.ctx)
                    where = (self.name, view, w, h, fog)
                    assert _same_bits(img, ref), (where, np.argwhere(img.view(np.uint32) != ref.view(np.uint32))[:8])
                    assert np.array_equal(packed, ref_packed), where
                    assert st["rays_primary"] == w * h and st["rays_shadow"] == ref_st["rays_shadow"], (where, st, ref_st)
                    lanes = _items(self.ctx.lib, _params(w, h))
                    hit = (ref[..., 4] < 1.0e6)[lanes[..., 2], lanes[..., 1]] & (lanes[..., 0] != 0)
                    assert total == len(lanes) and int(hit.any(axis=1).sum()) <= live <= total, (where, live, total, int(hit.any(axis=1).sum()))
                    if fog == 0:
                        hits += int(hit.sum())
                        if live_of is not None:
                            assert live == live_of[view][fi], (where, live, live_of[view][fi])
        return hits


@pytest.fixture(scope="module")
def committed(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Committed(gpu_ctx, name)
        return cache[name]
    yield get
    for c in cache.values():
        c.sc.release()


@pytest.mark.parametrize("name", list(SCENES))
def test_flagship_frames_equal_the_every_class_frames(committed, name):
    c = committed(name)
    c.check_choice(0)
    assert c.compare(live_of=LIVE) > 1000, name  # pictures, not skies


def _sampler_equals_the_three_row_sampler(c, waves):
    """mode 1 against mode 1 faithful=1 on every view, 24 x 16 and 72 x 40; `waves`: the waves per SIMD the two-row instance is compiled for"""
    c.check_choice(1)
    inst = _choice(c.ctx.lib, c.b, c.root, _params(24, 16, mode=1))[1]
    assert (inst >> 4) & 15 == waves, (c.name, inst)
    hits = 0
    for view, cam in _views().items():
        for w, h in FRAMES[:2]:
            ref, _, ref_st = c.sc.render(cam, c.lights, _params(w, h, mode=1, faithful=1), want_packed=False)
            img, _, st = c.sc.render(cam, c.lights, _params(w, h, mode=1), want_packed=False)
            assert _same_bits(img, ref), (c.name, view, w, h, np.argwhere(img.view(np.uint32) != ref.view(np.uint32))[:8])
            assert st["rays_primary"] == ref_st["rays_primary"] and st["rays_shadow"] == ref_st["rays_shadow"], (c.name, view, w, h, st, ref_st)
            hits += int((ref[..., 4] < 1.0e6).sum())
    assert hits > 1000, (c.name, hits)  # pictures, not skies


@pytest.mark.parametrize("name", ["three_bihs", "noshadow_and_onlyshadow"])
def test_two_row_sampler_equals_the_three_row_sampler(committed, name):
    _sampler_equals_the_three_row_sampler(committed(name), 4)


def test_the_five_wave_two_row_sampler_equals_the_three_row_sampler(gpu_ctx):
    """a tree of more than 500,000 nodes gets the two-row sampler compiled for five waves per SIMD (instances.hpp choose_sampler): the
    terrain at BIG x BIG cells (about 0.8 nodes per triangle: 530,000), with the NoShadow and the OnlyShadow bih beside it"""
    c = Committed(gpu_ctx, "noshadow_and_onlyshadow_big", lambda: _flags(BIG, _Direct()))
    try:
        _sampler_equals_the_three_row_sampler(c, 5)
    finally:
        c.sc.release()


@pytest.mark.parametrize("name", ["three_bihs", "noshadow_and_onlyshadow", "tex_levels_and_a_bare_bih"])
def test_a_three_frame_batch_equals_three_every_class_frames(committed, name):
    import torch
    c = committed(name)
    pos = scenes.CUST_CAM[0]
    cams = list(_views().values()) + [api.camera((pos[0], 40.0, pos[2]), (pos[0], 44.0, pos[2] + 15.0), (0.0, 1.0, 0.0), 45.0)]  # the third sees sky alone
    ca, la = (L.Camera * 3)(*cams), (L.Light * max(1, len(c.lights)))(*c.lights)
    for w, h in FRAMES[1:]:
        P = _params(w, h)
        px = torch.full((3, h, w), 0x55555555, dtype=torch.int32, device=torch.device("cuda:0"))
        assert c.sc.lib.glome_render_packed_batch_dev(c.sc.h, ca, 3, la, len(c.lights), C.byref(P), C.c_void_p(px.data_ptr()), h * w, None) == 0, c.ctx.err()
        c.ctx.synchronize()
        got = px.cpu().numpy().view(np.uint32)
        live, total = _last_cull(c.ctx)
        n_items = len(_items(c.ctx.lib, P))
        assert total == 3 * n_items and 0 < live <= 2 * n_items, (name, w, h, live, total)
        for f, cam in enumerate(cams):
            assert np.array_equal(got[f], c.sc.render(cam, c.lights, _params(w, h, faithful=1))[1]), (name, w, h, f)


def test_frames_stay_equal_after_every_update_of_a_committed_triangle_bih(gpu_ctx):
    c = Committed(gpu_ctx, "noshadow_and_onlyshadow")
    try:
        c.check_choice(0)
        frames = FRAMES[1:]
        before = c.sc.render(_views()["down"], c.lights, _params(72, 40, faithful=1))[0]
        walk = _patch(64, dx=0.6, dy=1.2, seed=5)
        c.sc.bih_update(c.bihs["walk"], walk)
        assert c.compare(frames) > 500
        after = c.sc.render(_views()["down"], c.lights, _params(72, 40, faithful=1))[0]
        assert not _same_bits(before, after), "the update changed nothing that the view sees"
        c.sc.bih_update_f32(c.bihs["leaf"], _patch(4, dx=-0.5, dy=0.3, seed=6).astype(np.float32))
        assert c.compare(frames) > 500
        terrain = scenes.heightfield_triangles(N).copy()
        terrain[:, 1::3] *= 1.25  # a higher terrain: its root box changes, and with it what the cull pass and the walks read from bihhdr
        c.sc.bih_update_indexed(c.bihs["terrain"], terrain.reshape(-1, 3), np.arange(3 * len(terrain), dtype=np.int32).reshape(-1, 3))
        assert c.compare(frames) > 500
        for t in c.bihs.values():  # a tree of triangles holds no object to refit from: refused, nested updates on or off, and nothing changes
            with pytest.raises(api.GlomeError):
                c.sc.bih_refit(t)
        c.sc.nested_updates(True)
        with pytest.raises(api.GlomeError):
            c.sc.bih_refit(c.bihs["walk"])
        assert c.compare(frames) > 500
    finally:
        c.sc.release()
