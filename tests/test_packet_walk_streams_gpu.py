"""GPU suite (-m gpu): the far-only step, the per-site dispatches, the one-test pop, the one-instruction push and B's record index of the
hand-written packet walk (bih_walk_asm, glome_amd/csrc/bih_packet_asm.hpp) on packets composed lane by lane through glome_trace_batch, as
tests/test_packet_walk_edges.py does for the overflow paths.

The packets are tests/packet_walk_scenes.py's; tests/test_packet_walk_model_host.py asserts, without a GPU, that their far-only steps come in
both register sets, on every axis in every octant, at stack pointers 0, CAP - 1, CAP and beyond, with a leaf and with a branch as the far
child, with a far mask that is a strict subset, with a NaN `near` lane, in the any-hit mode with lanes already occluded, directly after a pop
and directly after a re-entry from a C++ step; that they take every dispatch the block contains -- by site (after a both, near-only or
far-only step on each axis in each register set, after a pop, at the root, after a re-entry from a C++ step), target kind and mode, but for
the classes it lists as unreachable --; that they pop at stack pointers CAP - 1, CAP and CAP + 1, end every walk by a pop on the empty stack
(after a rejected entry among others), and hit the B half of pair records in leaves of 2, 3 and 5 triangles.  Scenes: the six ladders of
tests/ladder.py (walked from the heavy end, from inside the comb both ways, from the far end; their trimming branches have one empty child and
give far-only steps under 8 to 15 pending entries), a 6 x 6 x 6 lattice of small triangles whose tree changes axis in every order (two
lights: the shadow packets run two ways), and a heightfield of 16 x 16 cells under one light with the two outliers that give it the 12-entry
stack the walk is compiled for.  That the lattice and the heightfield reach the hand-written walk is asserted from the commit's own traits in
tests/test_packet_walk_model_host.py::test_the_scenes_reach_the_hand_written_walk (tests/test_packet_model.py's way).

Every packet is compared bit for bit with the faithful instance (and with glome_rayint_batch) and, ray by ray, with the fp64 oracle: hit or
miss and the primitive on every ray, depth inside 1e-4, colour inside the project's 1e-4 gate on every ray -- the rays are drawn clear of
every edge, their shadow rays too, and the materials are matte (the caps of tests/test_packet_walk_edges.py are 0 for the same reason); the
oracle's ray counts.  Then small frames (the ladder's 100 x 76) through the two-row flagship against the every-class kernel, out5 and
packed, one frame per launch and three as one batch."""
import ctypes as C

import numpy as np
import pytest

import ladder
import packet_walk_model as PM
import packet_walk_scenes as PS
from helpers import oracle_for, product_camera_lights
from test_packet_walk_edges import RAY_KEYS, Committed, both_instances, oracle_rows, rgbad
from test_kernel_choice import export_choice as render_choice, instance_name as render_instance_name
from glome_amd import _lib as L
from glome_amd import api
from oracle import np_scene as NS

pytestmark = pytest.mark.gpu

IDS = ["%s%s" % ("xyz"[a], "+" if s > 0 else "-") for a, s in ladder.CONFIGS]


def check_rows(c, name, r, ref):
    got = rgbad(r).astype(np.float64)
    rows = ref["rows"]
    hit_g, hit_r = got[:, 4] < 1e6, rows[:, 4] < 1e6
    prim_g = np.where(r["prim"] >= 0, c.sd_of_prod[r["prim"]], -1)
    away = ladder.colour_away(got, rows)
    both = hit_g & hit_r
    drel = np.abs(got[both, 4] - rows[both, 4]) / np.maximum(1.0, rows[both, 4])
    levels = {"rays": len(got), "hits": int(hit_r.sum()), "away": int(away.sum()), "flips": int((hit_g != hit_r).sum()), "other_prim": int((prim_g != ref["prim"]).sum()),
              "depth": int((drel > 1e-4).sum())}
    print("far_only_vs_oracle", name, levels, {k: r["stats"][k] for k in RAY_KEYS})
    assert np.array_equal(hit_g, r["t"] >= 0)
    assert levels["flips"] == 0 and levels["other_prim"] == 0, (name, levels, np.flatnonzero(prim_g != ref["prim"])[:16])
    assert levels["depth"] == 0 and levels["away"] == 0, (name, levels, np.flatnonzero(away)[:16])
    assert {k: r["stats"][k] for k in RAY_KEYS} == ref["counts"], name
    return levels


@pytest.fixture(scope="module")
def committed(gpu_ctx):
    cache = {}

    def get(v):
        if v not in cache:
            cache[v] = Committed(gpu_ctx, v)
        return cache[v]
    yield get
    for c in cache.values():
        c.sc.release()


@pytest.mark.parametrize("v", ladder.CONFIGS, ids=IDS)
def test_packets_on_the_ladder(committed, v):
    c = committed(v + (False,))
    sc, nm = NS.load(c.lad.sd)
    streams = PS.ladder_streams(c.lad, PM.device_bounds(sc.nodes[nm[c.lad.bih_id]].bb)[1][2])
    hits = 0
    for name, (ro, rd) in streams.items():
        r = both_instances(c, ro, rd)
        hits += check_rows(c, IDS[ladder.CONFIGS.index(v)] + " " + name, r, oracle_rows(c, ro, rd))["hits"]
        if name == "nan":  # the lane whose interval starts at NaN meets nothing, and its neighbours are what they are without it
            assert r["t"][17] == -1 and r["prim"][17] == -1
            keep = np.arange(64) != 17
            base = both_instances(c, streams["comb"][0][:64], streams["comb"][1][:64])
            assert all(np.array_equal(r[k][keep], base[k][keep]) for k in ("t", "prim", "rgba", "depth"))
    assert hits > 1000


class CommittedScene:
    """a Field or a Lattice on the GPU, its fp64 oracle and the id maps back to the SceneDesc (tests/test_packet_walk_edges.py's Committed, of a scene given)"""

    def __init__(self, ctx, field):
        self.field = field
        sd = self.field.sd
        self.b = api.Builder()
        self.nm, _ = sd.replay(self.b)
        self.sc = ctx.commit(self.b, self.nm[sd.root])
        self.cam, self.lights = product_camera_lights(sd)
        self.o, om, _ = oracle_for(sd)
        self.oroot = om[sd.root]
        self.sd_of_prod = np.full(max(self.nm) + 2, -1); self.sd_of_prod[np.asarray(self.nm)] = np.arange(len(self.nm))
        self.sd_of_oracle = np.full(max(om) + 2, -1); self.sd_of_oracle[np.asarray(om)] = np.arange(len(om))


@pytest.mark.parametrize("make, lights", [(PS.Lattice, 2), (PS.Field, 1)], ids=["lattice", "heightfield"])
def test_packets_on_a_lattice_and_a_heightfield(gpu_ctx, make, lights):
    c = CommittedScene(gpu_ctx, make())
    try:
        assert len(c.lights) == lights
        hits = 0
        for name, (ro, rd) in c.field.streams().items():
            r = both_instances(c, ro, rd)
            hits += check_rows(c, ("field " if make is PS.Field else "lattice ") + name, r, oracle_rows(c, ro, rd))["hits"]
        assert hits > 400
    finally:
        c.sc.release()


@pytest.mark.parametrize("n, rungs", [(1, (9, 4)), (4, (9, 4)), (2, (12, 6)), (5, (12, 6))], ids=[IDS[1], IDS[4], IDS[2], IDS[5]])
def test_three_frames_through_the_flagship_instance(committed, n, rungs):
    """the ladder's frame of 100 x 76 and two more views from inside the comb (between rungs, where every item's walk starts with far-only steps
    past the rungs behind the camera): the two-row flagship against the every-class kernel, out5 and packed, one frame per launch and the
    three as one batch"""
    import torch
    c = committed(ladder.CONFIGS[n] + (False,))
    lad = c.lad
    w, h = ladder.FRAME_W, ladder.FRAME_H
    lib = L.load()
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(c.b.h, c.nm[lad.sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    P = api.render_params(width=w, height=h, maxdepth=3)
    items = lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)
    kind, inst, two_rows, cap = render_choice(lib, [list(t[:8]) + [0, 0, 0, 3, 1, items]])[0].tolist()
    print("frame instance:", render_instance_name(kind, inst), "two_rows", two_rows, "items", items)
    assert two_rows == 1
    up = [0.0, 0.0, 0.0]; up[(lad.axis + 1) % 3] = 1.0
    look = ladder.to_world((ladder.L, 0.7e-6 * ladder.L, 0.4e-6 * ladder.L), lad.axis, lad.sign)
    cams = [c.cam] + [api.camera(ladder.to_world((1.4 * ladder.rung_u(j), 0.0, 0.0), lad.axis, lad.sign), look, tuple(up), ladder.FRAME_ANGLE) for j in rungs]
    refs, seen = [], []
    for cam in cams:
        img, packed, st = c.sc.render(cam, c.lights, P)
        imf, packedf, stf = c.sc.render(cam, c.lights, api.render_params(width=w, height=h, maxdepth=3, faithful=1))
        assert np.array_equal(img.view(np.uint32), imf.view(np.uint32)) and np.array_equal(packed, packedf)
        assert [st[k] for k in RAY_KEYS] == [stf[k] for k in RAY_KEYS]
        refs.append(packedf); seen.append(float((imf[..., 4] < 1e6).mean()))
    assert 0.05 < seen[0] < 0.9 and all(x > 0 for x in seen), seen  # (some pixels see a rung, the ones around the axis see none)
    ca, la = (L.Camera * 3)(*cams), (L.Light * max(1, len(c.lights)))(*c.lights)
    px = torch.full((3, h, w), 0x55555555, dtype=torch.int32, device=torch.device("cuda:0"))
    assert c.sc.lib.glome_render_packed_batch_dev(c.sc.h, ca, 3, la, len(c.lights), C.byref(P), C.c_void_p(px.data_ptr()), h * w, None) == 0, c.sc.ctx.err()
    c.sc.ctx.synchronize()
    got = px.cpu().numpy()
    for f in range(3):
        assert np.array_equal(got[f].view(np.uint32), np.asarray(refs[f]).view(np.uint32)), f
