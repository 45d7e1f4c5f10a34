"""What the packets of tests/test_packet_walk_streams_gpu.py make the hand-written packet walk (GLOME_PKW_ASM,
glome_amd/csrc/bih_packet_asm.hpp) do, step by step and block by block -- asserted without a GPU.

The walk's far-only step (a far child entered alone: no capacity test, no stack traffic, its node fetched into the register set the step ran
in), its per-site dispatches (GLOME_PKW_AFTER_X / _Y / _Z / _POP, GLOME_PKW_AT_ROOT: a different piece of code at every site, with its own
test order), its pop that tests the stack pointer once and B's record index made on the lanes run only on a GPU, so a GPU test of them is
worth what its inputs reach.  tests/packet_walk_model.py restates the walk for the 64 lanes of a wave and reports every event; here the
streams of the GPU test -- the six ladders of tests/ladder.py walked from the heavy end, from inside the comb both ways and from the far end,
a packet with a NaN `near` lane, a heightfield of 16 x 16 cells and a 6 x 6 x 6 lattice whose tree changes axis in every order, each with the
shadow packets the product makes of them -- are held to CONDITIONS: every class below is reached at least once (an empty class fails), but
for the dispatch classes listed in `unreachable` with their reasons.

The model itself is held, on every lane of every stream, to np_scene's own per-ray walk of the same tree, and to a record of what the three
models it replaced said of the same streams (tests/golden/packet_walk_record.json; tests/golden/make_packet_walk_record.py says how it was made).

Reached on this tree (printed by the tests): far-only steps in both register sets; on each split axis in each of the eight octants, in mode 1
and in mode 2; at stack pointers 0 .. 15 (0, CAP - 1 = 11, CAP = 12 and 13 .. 15 among them); with a leaf and with a branch as the far child;
with a far mask that is a strict subset of the node's lanes; with a NaN `near` lane (the root step of that lane's walk); in mode 2 with 2 .. 45
lanes occluded; directly after a pop inside the block and directly after a re-entry from a C++ step."""
import collections
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import packet_walk_model as PM
from test_trace_choice import export_choice, instance_name
from glome_amd import _lib as L
from glome_amd import api

_spec = importlib.util.spec_from_file_location("make_packet_walk_record", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_packet_walk_record.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

CAP = PM.LDS_CAP
EVERY = {(o, a) for o in range(8) for a in range(3)}
LADDER_SHADOW = "screen's shadow rays by ladder.shadow_rays"


@pytest.fixture(scope="module")
def scenes_(built):
    """the six ladders, the field and the lattice, each with its tree and its primary streams"""
    return REC.all_scenes()


@pytest.fixture(scope="module")
def walked(scenes_):
    """Everything the record holds, walked ONCE: (scene name, stream, mode, origin clip) -> (the rays as [(o, d, limit)], the packets' walks); and the
    record made of those walks' three views.  Shared, never written to."""
    walks = {}

    def views(s, stream, mode, clip, chunks):
        w = [r for o, d, lim in chunks for r in PM.stream(s.bih, o, d, lim, mode, origin_clip=clip)]
        walks[(s.name, stream, mode, clip)] = (chunks, w)
        return None if clip else [PM.as_packet(r) for r in w], [PM.as_steps(r) for r in w], [PM.as_events(r) for r in w]
    return walks, REC.record(scenes_, views)


def _steps(walked, s, stream, mode):
    return [PM.as_steps(r) for r in walked[0][(s.name, stream, mode, True)][1]]


def _events_of(scenes_, walked):
    """(scene, stream name, mode, the production walk's events per packet): the primary packets and the shadow packets made of them"""
    for s in scenes_:
        for name in s.streams:
            for stream, mode in ((name, 1), (name + "'s shadow rays", 2)):
                if (s.name, stream, mode, True) in walked[0]:
                    yield s, stream, mode, [PM.as_events(r) for r in walked[0][(s.name, stream, mode, True)][1]]


@pytest.fixture(scope="module")
def events(scenes_, walked):
    """every event of every packet, per mode: computed once, shared, never written to"""
    ev = {1: [], 2: []}
    per = collections.Counter()
    for s, name, mode, res in _events_of(scenes_, walked):
        for r in res:
            ev[mode] += r["events"]
        per[s.name.split()[0] + " " + name] += sum(isinstance(e, PM.Dispatch) for r in res for e in r["events"])
    print("dispatches per stream:", dict(per))
    return {m: tuple(v) for m, v in ev.items()}


def test_the_scenes_reach_the_hand_written_walk(scenes_):
    """a 12-entry LDS stack with overflow columns and the instances that inline bih_walk_asm, by the commit's own traits (tests/test_packet_model.py's
    way): one ladder (that test asserts it of all), the heightfield with its two outliers and the lattice with its outliers"""
    lib = L.load()
    for s in (scenes_[0], scenes_[-2], scenes_[-1]):
        sd = s.holder.sd
        b = api.Builder()
        nmap, _ = sd.replay(b)
        t = np.zeros(11, dtype=np.int64)
        assert lib.glome_sb_scene_traits(b.h, nmap[sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        tier, cls_mask, sec, nested, refract, pk_all, stack_cap = (int(x) for x in t[:7])
        assert (tier, pk_all, stack_cap, cls_mask) == (0, 1, CAP, 1), s.name
        assert instance_name(int(export_choice(lib, [list(t[:8]) + [0, 0, 3]])[0, 0])) == "k_trace_batch_flat<false,false,false,TRI,1>"


# ---------------------------------------------------------------- the model against np_scene's own walk, and against the record
def test_every_lane_is_np_scenes_own_answer(scenes_, walked):
    """On every lane of every stream the model's primitive is the one np_scene's own per-ray walk of the same tree reports (Bih.rayint: recursive,
    the reference's interval), and in mode 2 `occluded` is its shadow answer (Bih.shadow) -- with the origin clip and, where the stream is walked
    without it, without.  The streams are drawn clear of every edge: no lane is left out."""
    by_name = {s.name: s for s in scenes_}
    want, lanes = {}, 0
    for (scene, stream, mode, clip), (chunks, w) in walked[0].items():
        bih = by_name[scene].bih
        if (scene, stream) not in want:
            rays = [(tuple(map(float, o)), tuple(map(float, d)), float(lim)) for co, cd, cl in chunks
                    for o, d, lim in zip(np.asarray(co, np.float64), np.asarray(cd, np.float64), np.broadcast_to(np.asarray(cl, np.float64), (len(co),)))]
            if mode == 1:
                hits = [bih.rayint(o, d, lim, ()) for o, d, lim in rays]
                want[(scene, stream)] = np.array([-1 if h is None else h[4] for h in hits])
            else:
                want[(scene, stream)] = np.array([bih.shadow(o, d, lim) for o, d, lim in rays])
        got = np.concatenate([r["prim"] if mode == 1 else r["occluded"] for r in w])
        assert np.array_equal(got, want[(scene, stream)]), (scene, stream, mode, clip, np.flatnonzero(got != want[(scene, stream)])[:16])
        if mode == 2:
            assert all(np.array_equal(r["prim"] >= 0, r["occluded"]) for r in w)
        lanes += len(got)
    print("lanes held to np_scene:", lanes, "in", len(walked[0]), "walked streams")
    assert {k[3] for k in walked[0]} == {True, False} and {k[2] for k in walked[0]} == {1, 2}


def test_the_model_says_what_the_three_models_it_replaced_said(walked):
    """tests/golden/packet_walk_record.json, made with the three models' walk_stream, stream_steps and stream_events on the commit that had them,
    against the same record made of this model's three views: key by key, the readable totals first"""
    with open(REC.RECORD) as f:
        text = f.read()
    want, got = json.loads(text), json.loads(REC.dumps(walked[1]))
    assert list(got) == list(want)
    for k in want:
        assert got[k]["totals"] == want[k]["totals"], k
    for k in want:
        assert got[k] == want[k], k
    assert REC.dumps(walked[1]) == text


# ---------------------------------------------------------------- the far-only step
def _far(res):
    return [s for r in res for s in r["steps"] if s.kind == "far"]


def test_every_class_of_far_only_step_is_reached(scenes_, walked):
    far = {1: [], 2: []}
    per_stream = collections.Counter()
    for c in scenes_[:6]:
        for name in c.streams:
            res = _steps(walked, c, name, 1)
            far[1] += _far(res); per_stream[name] += len(_far(res))
        res = _steps(walked, c, LADDER_SHADOW, 2)
        far[2] += _far(res); per_stream["screen's shadow rays"] += len(_far(res))
    for name in scenes_[-2].streams:
        res = _steps(walked, scenes_[-2], name, 1)
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


def test_the_steps_pushes_and_pops_beyond_the_lds_part_are_the_blocks_exits(walked):
    """a both-step handed to C++ is one push beyond the LDS part and one exit with status 1, in every packet, with the origin clip and without"""
    for key, (chunks, w) in walked[0].items():
        for r in w:
            a, b, c = PM.as_packet(r), PM.as_steps(r), PM.as_events(r)
            assert sum(s.kind == "both" and s.where == "cpp" for s in b["steps"]) == a["pushes_over"] == b["pushes_over"] == c["exits_push"], key
            assert a["pops_over"] == b["pops_over"] == c["exits_pop"] == sum(isinstance(e, PM.Pop) and e.outcome == "over" for e in c["events"]), key
            assert max([s.sp + 1 for s in b["steps"] if s.kind == "both"], default=0) == a["max_depth"], key


def test_the_nan_lane_is_one(scenes_):
    """the lane composed into the "nan" packets has a NaN root interval start on the device's bounds, walks alone (its octant differs from its
    neighbours'), takes its root step as a far-only step and meets nothing"""
    for c in scenes_[:6]:
        if c.holder.axis == 2:
            assert "nan" not in c.streams
            continue
        o, d = c.streams["nan"]
        with np.errstate(divide="ignore", invalid="ignore"):
            near, far = PM.root_interval(PM.device_bounds(c.bih.bb), o.astype(np.float64), d.astype(np.float64), np.full(len(o), 1e6))
        assert np.flatnonzero(np.isnan(near)).tolist() == [17] and far[17] > 0
        r = PM.walk_steps(c.bih, o[17:18], d[17:18], 1e6, 1)
        assert r["steps"][0].kind == "far" and r["steps"][0].nan_near and r["steps"][0].sp == 0 and all(s.kind != "near" and s.kind != "both" for s in r["steps"])
        assert r["prim"][0] == -1


# ---------------------------------------------------------------- the dispatches
# The classes no packet can reach, with their reasons.  A class: (site, axis of the step left, register set of the dispatching code, target, mode).
def unreachable(cls):
    site, axis, rset, target, mode = cls
    if site in ("pop", "root", "reentry") and rset == "B":
        return "a pop, the root and a re-entry fetch the node into set A (L_node2 and the pop's own fetch): their dispatch has no set B form"
    if site == "root" and target == 3:
        return "a tree whose root is a leaf never reaches the walk: bih_tri_wave tests a one-leaf tree per lane"
    return None


def test_every_dispatch_class_is_reached(events):
    every = {(k, a, s, t, m) for (k, a, s) in PM.STEP_SITES for t in PM.TARGETS for m in (1, 2)}
    every |= {(k, None, s, t, m) for k in ("pop", "root", "reentry") for s in "AB" for t in PM.TARGETS for m in (1, 2)}
    seen = collections.Counter((e.site, e.axis, e.set, e.target, e.mode) for m in (1, 2) for e in events[m] if isinstance(e, PM.Dispatch))
    assert set(seen) <= every
    listed = {c for c in every if unreachable(c)}
    assert not (set(seen) & listed), sorted(set(seen) & listed, key=str)
    missing = sorted(every - listed - set(seen), key=str)
    print("classes:", len(every), "listed as unreachable:", len(listed), "reached:", len(seen), "fewest packets' dispatches in a class:", min(seen.values()))
    # a fresh walk starts at the tree's root, whose kind is the tree's: the scenes' roots split every axis between them
    assert not missing, missing


# ---------------------------------------------------------------- the pop
def _pops(ev):
    return [e for e in ev if isinstance(e, PM.Pop)]


def test_the_pop_cases_are_reached(events):
    for mode in (1, 2):
        ev = events[mode]
        pops = _pops(ev)
        # every walk ends by a pop on an empty stack: the block's only way to status 0
        exits = [e for e in ev if isinstance(e, PM.Exit)]
        assert sum(p.outcome == "empty" for p in pops) == sum(e.status == 0 for e in exits) > 0
        assert all(e.sp == 0 and e.lanes == 0 for e in exits if e.status == 0)
        by_sp = collections.Counter((p.sp, p.outcome) for p in pops)
        print("mode", mode, "pops by (sp before, outcome):", dict(sorted(by_sp.items())))
        # the last entry of the LDS part, the first beyond it (sp = CAP: m0 = CAP - 1 passes the one compare) and the next (m0 = CAP: handed to C++)
        assert by_sp[(CAP - 1, "taken")] and by_sp[(CAP, "taken")] and by_sp[(CAP + 1, "over")]
        assert all(p.outcome == "over" for p in pops if p.sp > CAP) and not any(p.outcome == "over" for p in pops if p.sp <= CAP)
        # a popped entry that the filter rejects, directly followed by the empty stack
        assert any(a.outcome == "rejected" and a.sp == 1 and b.outcome == "empty" for a, b in zip(pops, pops[1:]))
        # entries of the block: fresh (phase 0, sp 0), after a C++ push (phase 0, sp > CAP), after a C++ pop that some lane wants (phase 0, sp >= CAP)
        # and after one that nobody wants (phase 1, sp >= CAP: the block pops first)
        entries = collections.Counter((e.phase, min(e.sp, CAP + 1)) for e in ev if isinstance(e, PM.Entry))
        print("mode", mode, "entries by (phase, min(sp, CAP + 1)):", dict(sorted(entries.items())))
        assert entries[(0, 0)] and entries[(0, CAP)] and entries[(0, CAP + 1)] and entries[(1, CAP)]
        # AN ENTRY WITH phase = 1 AND sp = 0 CANNOT OCCUR: bih_tri_packet_hw sets phase 1 only after a pop from the overflow columns, which leaves
        # sp >= CAP.  The block's answer to it (status 0, am = 0, sp = 0) is held by test_phase_1_on_an_empty_stack_is_the_end on the model of the pop.
        assert not any(isinstance(e, PM.Entry) and e.phase == 1 and e.sp < CAP for e in ev)


def parents_pop(m0, cap=CAP):
    """the pop's head before it tested once: s_sub_u32 m0, m0, 1; s_cbranch_scc1 L_empty (SCC = the borrow); s_cmp_ge_u32 m0, cap; s_cbranch_scc1 L_popslow"""
    borrow = m0 == 0
    m0 = (m0 - 1) & PM.U32
    if borrow:
        return "empty", 0
    if m0 >= cap:
        return "over", m0 + 1
    return "lds", m0


def test_one_compare_is_the_parents_two():
    for cap in (1, CAP, 255):
        for m0 in list(range(0, cap + 40)) + [2 ** 31 - 1, 2 ** 31, PM.U32 - 1]:
            assert PM.pop_fold(m0, cap) == parents_pop(m0, cap), (cap, m0)
    assert PM.pop_fold(0) == ("empty", 0) and PM.pop_fold(1) == ("lds", 0) and PM.pop_fold(CAP) == ("lds", CAP - 1) and PM.pop_fold(CAP + 1) == ("over", CAP + 1)
    # (m0 - 1 is 0xffffffff for m0 = 0 alone: the two forms differ on no value at all)
    assert PM.pop_fold(PM.U32) == ("over", PM.U32) == parents_pop(PM.U32)


def test_phase_1_on_an_empty_stack_is_the_end(scenes_):
    s = scenes_[-1]
    o, d = (a[:64].astype(np.float64) for a in s.streams["outside"])
    for mode in (1, 2):
        ev = []
        w = PM._Walk(s.bih, o, d, 1.0 / d, 7, np.ones(64, bool), np.zeros(64), np.full(64, 1e6), mode, np.full(64, PM.NO_BEST), np.full(64, -1, np.int64), np.zeros(64, bool), ev)
        assert w.block(1, False) == 0 and w.sp == 0 and not w.am.any()
        assert ev == [PM.Entry(1, 0, mode), PM.Pop(0, "empty", mode)]


def test_the_model_has_the_walks_stack_pointer_status_and_final_am(scenes_, walked):
    """on every packet: the stack pointer is 0 at every end, one exit with status 0 per walk and none after it, exits with 1 and 3 only beyond the
    LDS part, and no lane left at the end"""
    packets = over = 0
    for s, name, mode, res in _events_of(scenes_, walked):
        for r in res:
            exits = [e for e in r["events"] if isinstance(e, PM.Exit)]
            walks = sum(isinstance(e, PM.Entry) and e.phase == 0 and e.sp == 0 for e in r["events"])
            done = [e for e in exits if e.status == 0]
            assert len(done) == walks and all(e.sp == 0 and e.lanes == 0 for e in done)
            assert all(e.sp >= CAP and e.lanes > 0 for e in exits if e.status == 1) and all(e.sp > CAP for e in exits if e.status == 3)
            assert {e.status for e in exits} <= {0, 1, 3} and exits[-1].status == 0
            packets += 1; over += r["exits_pop"]
    print("packets:", packets, "exits with status 3:", over)
    assert packets > 200 and over > 100


# ---------------------------------------------------------------- the leaf
def test_the_leaf_cases_are_reached(events):
    """leaves of 1, 2, 3 and 5 triangles, and hits on the B half of a pair record (odd items: their record index is the A half's plus one), the B
    half of a leaf's LAST record among them; a leaf of odd size ends with a record whose B half is computed and ignored, so its last item is an A"""
    for mode in (1, 2):
        leaves = [e for e in events[mode] if isinstance(e, PM.Leaf)]
        hits = collections.defaultdict(set)
        for e in leaves:
            hits[e.size] |= e.hits
        print("mode", mode, "items hit by leaf size:", {k: sorted(v) for k, v in sorted(hits.items())})
        assert {1, 2, 3, 5} <= set(hits)
        assert 0 in hits[1] and 1 in hits[2] and {1, 2} <= hits[3] and 1 in hits[5]
        assert any(s % 2 == 0 and s - 1 in h for s, h in hits.items())  # the B half of the last record
