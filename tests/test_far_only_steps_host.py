"""What the packets of tests/test_far_only_steps_gpu.py make the hand-written packet walk do, step by step -- asserted without a GPU.

Since the votes of its branch step were reordered (GLOME_PKW_STEP, glome_amd/csrc/bih_packet_asm.hpp) the walk pushes only when both
children are entered; a far child entered alone is a step of its own kind: no capacity test, no stack traffic, its node fetched into the
register set the step ran in.  That path can only run on a GPU, so a GPU test of it is worth what its inputs reach.  tests/far_only_model.py
restates the step's control flow for the 64 lanes of a wave and reports every step's kind and state; here the streams of the GPU test
-- the six ladders of tests/ladder.py walked from the heavy end, from inside the comb both ways and from the far end, their shadow packets,
a packet with a NaN `near` lane, and a heightfield of 16 x 16 cells -- are held to CONDITIONS: every class below is reached by a far-only
step at least once (an empty class fails), and the model's pushes and pops beyond the LDS part of the stack are packet_model.walk_packet's.

Reached on this tree (printed by the tests): far-only steps in both register sets; on each split axis in each of the eight octants, in mode 1
and in mode 2; at stack pointers 0 .. 15 (0, CAP - 1 = 11, CAP = 12 and 13 .. 15 among them); with a leaf and with a branch as the far child;
with a far mask that is a strict subset of the node's lanes; with a NaN `near` lane (the root step of that lane's walk); in mode 2 with 2 .. 45
lanes occluded; directly after a pop inside the block and directly after a re-entry from a C++ step."""
import collections
import ctypes as C

import numpy as np
import pytest

import far_only_model as FM
import ladder
import packet_model as PM
from test_trace_choice import export_choice, instance_name
from glome_amd import _lib as L
from glome_amd import api
from oracle import np_scene as NS

CAP = FM.CAP
EVERY = {(o, a) for o in range(8) for a in range(3)}


class LadderCase:
    def __init__(self, axis, sign):
        self.lad = ladder.Ladder(axis, sign)
        sc, nm = NS.load(self.lad.sd)
        self.bih = sc.nodes[nm[self.lad.bih_id]]
        self.streams = FM.ladder_streams(self.lad, FM.device_bounds(self.bih.bb)[1][2])


@pytest.fixture(scope="module")
def ladders(built):
    return [LadderCase(*v) for v in ladder.CONFIGS]


@pytest.fixture(scope="module")
def field(built):
    f = FM.Field()
    sc, nm = NS.load(f.sd)
    return f, sc.nodes[nm[f.bih_id]], f.streams()


def _shadow_stream(c, o, d):
    """the shadow rays of a stream of primary rays that all end on the screen (ladder.shadow_rays), from the model's own hit distances"""
    prim = FM.stream_steps(c.bih, o, d, 1e6, 1)
    t = np.concatenate([r["t"] for r in prim])
    assert np.all(t > 0)
    return ladder.shadow_rays(c.lad, o, d, t)


def _far(res):
    return [s for r in res for s in r["steps"] if s.kind == "far"]


def _same_as_packet_model(bih, o, d, dist, mode):
    """without the origin clip the restated steps give packet_model.walk_packet's walk: the same pushes and pops beyond the LDS part, depth and
    per-lane results; and the clip changes no lane's result"""
    pm = PM.walk_stream(bih, o, d, dist, mode)
    plain = FM.stream_steps(bih, o, d, dist, mode, origin_clip=False)
    clip = FM.stream_steps(bih, o, d, dist, mode)
    for a, b, c in zip(pm, plain, clip):
        assert (a["pushes_over"], a["pops_over"], a["max_depth"]) == (b["pushes_over"], b["pops_over"], b["max_depth"])
        assert sum(s.kind == "both" and s.where == "cpp" for s in b["steps"]) == a["pushes_over"]
        assert np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["prim"], c["prim"])
        if mode == 1:
            assert np.array_equal(a["t"], b["t"]) and np.array_equal(a["t"], c["t"])
        else:
            assert np.array_equal(a["occluded"], b["occluded"]) and np.array_equal(a["occluded"], c["occluded"])
    return clip


def test_the_scenes_reach_the_hand_written_walk(ladders, field):
    """a 12-entry LDS stack with overflow columns and the instances that inline bih_walk_asm: the ladders (tests/test_packet_model.py asserts the
    same of them) and the heightfield"""
    lib = L.load()
    for sd in [c.lad.sd for c in ladders[:1]] + [field[0].sd]:
        b = api.Builder()
        nmap, _ = sd.replay(b)
        t = np.zeros(11, dtype=np.int64)
        assert lib.glome_sb_scene_traits(b.h, nmap[sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        tier, cls_mask, sec, nested, refract, pk_all, stack_cap = (int(x) for x in t[:7])
        assert (tier, pk_all, stack_cap, cls_mask) == (0, 1, CAP, 1)
        assert instance_name(int(export_choice(lib, [list(t[:8]) + [0, 0, 3]])[0, 0])) == "k_trace_batch_flat<false,false,false,TRI,1>"


def test_every_class_of_far_only_step_is_reached(ladders, field):
    far = {1: [], 2: []}
    per_stream = collections.Counter()
    for c in ladders:
        for name, (o, d) in c.streams.items():
            res = FM.stream_steps(c.bih, o, d, 1e6, 1) if name == "nan" else _same_as_packet_model(c.bih, o, d, 1e6, 1)
            far[1] += _far(res); per_stream[name] += len(_far(res))
        so, sd_, sl = _shadow_stream(c, *c.streams["screen"])
        res = _same_as_packet_model(c.bih, so, sd_, sl, 2)
        far[2] += _far(res); per_stream["screen's shadow rays"] += len(_far(res))
    f, bih, streams = field
    for name, (o, d) in streams.items():
        res = _same_as_packet_model(bih, o, d, 1e6, 1)
        far[1] += _far(res); per_stream["field " + name] += len(_far(res))
    both = far[1] + far[2]
    print("far-only steps per stream:", dict(per_stream))
    print("stack pointers:", sorted({s.sp for s in both}), "lanes occluded (mode 2):", sorted({s.occluded for s in far[2]}))
    print("after:", dict(collections.Counter(s.after for s in both)), "sets:", dict(collections.Counter(s.set for s in both)))
    assert all(s.where == "asm" for s in both)  # no far-only step is handed to C++, whatever the stack holds
    assert {s.set for s in both} == {"A", "B"}
    for mode in (1, 2):
        assert {(s.octant, s.axis) for s in far[mode]} == EVERY, (mode, sorted(EVERY - {(s.octant, s.axis) for s in far[mode]}))
        assert {(s.axis, s.fwd) for s in far[mode]} == {(a, w) for a in range(3) for w in (False, True)}
    sps = {s.sp for s in both}
    assert {0, CAP - 1, CAP} <= sps and max(sps) > CAP, sorted(sps)
    assert {s.fc_leaf for s in both} == {False, True}
    assert any(s.far_subset for s in both)
    assert any(s.nan_near for s in both)
    assert any(s.occluded > 0 for s in far[2]) and all(s.occluded == 0 for s in far[1])
    assert {"pop", "reentry", "step", "root"} <= {s.after for s in both}
    # ... and the far-only steps under a full LDS part come in both sets and after both kinds of fetch
    deep = [s for s in both if s.sp >= CAP]
    assert {s.set for s in deep} == {"A", "B"} and {"reentry", "step"} <= {s.after for s in deep}


def test_the_nan_lane_is_one(ladders):
    """the lane composed into the "nan" packets has a NaN root interval start on the device's bounds, walks alone (its octant differs from its
    neighbours'), takes its root step as a far-only step and meets nothing"""
    for c in ladders:
        if c.lad.axis == 2:
            assert "nan" not in c.streams
            continue
        o, d = c.streams["nan"]
        with np.errstate(divide="ignore", invalid="ignore"):
            near, far = PM.root_interval(FM.device_bounds(c.bih.bb), o.astype(np.float64), d.astype(np.float64), np.full(len(o), 1e6))
        assert np.flatnonzero(np.isnan(near)).tolist() == [17] and far[17] > 0
        r = FM.walk_steps(c.bih, o[17:18], d[17:18], 1e6, 1)
        assert r["steps"][0].kind == "far" and r["steps"][0].nan_near and r["steps"][0].sp == 0 and all(s.kind != "near" and s.kind != "both" for s in r["steps"])
        assert r["prim"][0] == -1
