"""GPU suite (-m gpu): the pair test of the hand-written packet walk that leaves when no ray passes b1, and its hit update that is skipped when
nobody hit (GLOME_PKW_PAIR_B1 / _VOTE / _REST, GLOME_PKW_SKIP_1; glome_amd/csrc/bih_packet_asm.hpp), on packets composed lane by lane through
glome_trace_batch.

The packets: tests/pair_exit_model.py's two text trees, whose leaves hold exactly 1, 2, 3 and 5 triangles (every lane of a packet aimed at one
triangle of a leaf, at two, or beside them: per octant one packet of each kind; the mirror image sends the shadow packets the other way along
x), and the 6 x 6 x 6 lattice and the 16 x 16 heightfield of tests/test_packet_walk_streams_gpu.py.  tests/test_pair_exit_model_host.py
asserts, without a GPU, that they reach every path through the pair test in the closest-hit and in the any-hit mode: a test left on the first
pair of a leaf of 1, 2, 3 and 5 triangles, left on the first pair and hit on the second, A kept alone, B kept alone, both kept, a kept lane
that fails the chain, the update skipped on A and taken on B and the reverse -- and that the text trees get the 12-entry stack and the
instance that inlines the walk.

Every packet is compared bit for bit with the faithful instance (and with glome_rayint_batch) and, ray by ray, with the fp64 oracle: hit or
miss and the primitive on every ray, depth inside 1e-4, colour inside the project's 1e-4 gate (the rays are aimed clear of every edge and
the materials are matte), the oracle's ray counts.  Then three frames of 100 x 76 of each text tree through the two-row flagship against the
every-class kernel, one frame per launch and the three as one batch."""
import ctypes as C

import numpy as np
import pytest

import pair_exit_model as X
import packet_walk_scenes as PS
import test_packet_walk_streams_gpu as S
from helpers import oracle_for, product_camera_lights
from test_packet_walk_edges import RAY_KEYS, both_instances, oracle_rows
from test_kernel_choice import export_choice as render_choice, instance_name as render_instance_name
from glome_amd import _lib as L
from glome_amd import api

pytestmark = pytest.mark.gpu

FRAME_W, FRAME_H = 100, 76


class CommittedLeaves:
    """a text tree on the GPU, its fp64 oracle (over the same triangles in the oracle's own tree) and the id maps back to the SceneDesc"""

    def __init__(self, ctx, sign):
        self.lv = lv = X.Leaves(sign)
        self.b = api.Builder()
        self.root, items = lv.load(self.b)
        self.sc = ctx.commit(self.b, self.root)
        self.cam, self.lights = product_camera_lights(lv.sd)
        self.o, om, _ = oracle_for(lv.sd)
        self.oroot = om[lv.sd.root]
        self.sd_of_prod = np.full(max(items) + 2, -1)
        self.sd_of_prod[np.asarray(items) - 1] = lv.tri_ids  # (a hit names the Triangle inside its Tex: the node made just before it)
        self.sd_of_oracle = np.full(max(om) + 2, -1); self.sd_of_oracle[np.asarray(om)] = np.arange(len(om))


@pytest.fixture(scope="module")
def leaves(gpu_ctx):
    cache = {}

    def get(sign):
        if sign not in cache:
            cache[sign] = CommittedLeaves(gpu_ctx, sign)
        return cache[sign]
    yield get
    for c in cache.values():
        c.sc.release()


@pytest.mark.parametrize("sign", [1, -1], ids=["x+", "x-"])
def test_packets_on_leaves_of_1_2_3_and_5_triangles(leaves, sign):
    """all eight octants (a packet per octant and kind), the closest-hit walk on the primary rays and the any-hit walk on their shadow rays"""
    c = leaves(sign)
    hits = shadows = 0
    for name, (ro, rd) in c.lv.streams().items():
        r = both_instances(c, ro, rd)
        levels = S.check_rows(c, "leaves x%s %s" % ("+-"[sign < 0], name), r, oracle_rows(c, ro, rd))
        assert np.all(c.sd_of_prod[r["prim"][r["prim"] >= 0]] >= 0)
        hits += levels["hits"]; shadows += r["stats"]["rays_shadow"]
        if name.startswith("beside"):
            assert levels["hits"] < levels["rays"] // 2  # most of these rays pass beside every triangle
    assert hits > 3000 and shadows > 3000, (hits, shadows)


@pytest.mark.parametrize("make, lights", [(PS.Lattice, 2), (PS.Field, 1)], ids=["lattice", "heightfield"])
def test_packets_on_the_lattice_and_the_heightfield(gpu_ctx, make, lights):
    """the streams of tests/test_packet_walk_streams_gpu.py, by its own check: leaves of one and two triangles in trees the builder made"""
    S.test_packets_on_a_lattice_and_a_heightfield(gpu_ctx, make, lights)


@pytest.mark.parametrize("sign", [1, -1], ids=["x+", "x-"])
def test_three_frames_through_the_flagship_instance(leaves, sign):
    """the scene's camera (from the lit side, along the leaves), one from the dark side and one from above at a slant: the two-row flagship against
    the every-class kernel, out5 and packed, one frame per launch and the three as one batch"""
    import torch
    c = leaves(sign)
    w, h = FRAME_W, FRAME_H
    lib = L.load()
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(c.b.h, c.root, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    P = api.render_params(width=w, height=h, maxdepth=3)
    items = lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)
    kind, inst, two_rows, cap = render_choice(lib, [list(t[:8]) + [0, 0, 0, 3, 1, items]])[0].tolist()
    print("frame instance:", render_instance_name(kind, inst), "two_rows", two_rows, "items", items)
    assert two_rows == 1
    mx = (lambda x: x) if sign > 0 else (lambda x: 8.0 - x)
    cams = [c.cam, api.camera((mx(15.0), 0.2, 5.5), (mx(1.0), 0.5, 3.5), (0.0, 1.0, 0.0), 24.0), api.camera((mx(-3.0), 5.0, -4.0), (mx(6.0), 0.4, 5.0), (0.0, 1.0, 0.0), 28.0)]
    refs, seen = [], []
    for cam in cams:
        img, packed, st = c.sc.render(cam, c.lights, P)
        imf, packedf, stf = c.sc.render(cam, c.lights, api.render_params(width=w, height=h, maxdepth=3, faithful=1))
        assert np.array_equal(img.view(np.uint32), imf.view(np.uint32)) and np.array_equal(packed, packedf)
        assert [st[k] for k in RAY_KEYS] == [stf[k] for k in RAY_KEYS]
        refs.append(packedf); seen.append(float((imf[..., 4] < 1e6).mean()))
    assert all(0.02 < x < 0.9 for x in seen), seen  # (every view sees triangles and sky)
    ca, la = (L.Camera * 3)(*cams), (L.Light * max(1, len(c.lights)))(*c.lights)
    px = torch.full((3, h, w), 0x55555555, dtype=torch.int32, device=torch.device("cuda:0"))
    assert c.sc.lib.glome_render_packed_batch_dev(c.sc.h, ca, 3, la, len(c.lights), C.byref(P), C.c_void_p(px.data_ptr()), h * w, None) == 0, c.sc.ctx.err()
    c.sc.ctx.synchronize()
    got = px.cpu().numpy()
    for f in range(3):
        assert np.array_equal(got[f].view(np.uint32), np.asarray(refs[f]).view(np.uint32)), f
