"""What the packets of tests/test_dispatch_sites_gpu.py make the hand-written packet walk do at its dispatches, pops and leaves -- asserted
without a GPU.

Since round 12 the branch on a reference's two low bits (GLOME_PKW_AFTER_X / _Y / _Z / _POP, GLOME_PKW_AT_ROOT, bih_packet_asm.hpp) is a
different piece of code at every site, with its own test order; the pop tests the stack pointer once; B's record index is made on the
lanes.  Those paths run only on a GPU, so the GPU test is worth what its packets reach.  tests/dispatch_model.py runs the walk block by
block and records every dispatch by (site, axis and register set of the step it leaves, target kind, mode); here the GPU test's packets --
the six ladders' streams of tests/far_only_model.py, its 16 x 16 heightfield, and a 6 x 6 x 6 lattice whose tree changes axis in every
order, each with the shadow packets the product makes of them -- are held to: EVERY class is reached, but for the ones listed in
UNREACHABLE with their reasons."""
import collections
import ctypes as C

import numpy as np
import pytest

import dispatch_model as DM
import far_only_model as FM
import ladder
import packet_model as PM
from test_trace_choice import export_choice, instance_name
from glome_amd import _lib as L
from glome_amd import api
from oracle import np_scene as NS

CAP = DM.CAP


class Scene:
    """a scene of the GPU test: its tree, its primary streams and the shadow packets made of them"""

    def __init__(self, name, holder, bih, streams):
        self.name, self.holder, self.bih, self.streams = name, DM.with_uids(holder, bih), bih, streams

    def events(self):
        """(stream name, mode, the stream's modelled packets).  The primary packets without the origin clip are packet_model.walk_packet's walk; the
        production walk (with it) gives every lane the same result."""
        for name, (o, d) in self.streams.items():
            res = DM.stream_events(self.bih, o, d, 1e6, 1)
            if name != "nan":  # (packet_model takes no direction component of 0)
                for a, b, c in zip(PM.walk_stream(self.bih, o, d, 1e6, 1), DM.stream_events(self.bih, o, d, 1e6, 1, origin_clip=False), res):
                    assert (a["pushes_over"], a["pops_over"], a["max_depth"]) == (b["exits_push"], b["exits_pop"], b["max_depth"])
                    assert np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["prim"], c["prim"]) and np.array_equal(a["t"], c["t"])
            yield name, 1, res
            if name == "nan":
                continue
            sh = []
            for so, sd_, sl in DM.shadow_stream(self.holder, o, d, res):
                a, b = PM.walk_packet(self.bih, so, sd_, sl, 2), DM.walk_events(self.bih, so, sd_, sl, 2, origin_clip=False)
                assert (a["pushes_over"], a["pops_over"], a["max_depth"]) == (b["exits_push"], b["exits_pop"], b["max_depth"]) and np.array_equal(a["occluded"], b["occluded"])
                sh.append(DM.walk_events(self.bih, so, sd_, sl, 2))
                assert np.array_equal(a["occluded"], sh[-1]["occluded"])
            yield name + "'s shadow rays", 2, sh


@pytest.fixture(scope="module")
def scenes_(built):
    out = []
    for v in ladder.CONFIGS:
        lad = ladder.Ladder(*v)
        sc, nm = NS.load(lad.sd)
        bih = sc.nodes[nm[lad.bih_id]]
        out.append(Scene("ladder %s%s" % ("xyz"[v[0]], "+-"[v[1] < 0]), lad, bih, FM.ladder_streams(lad, FM.device_bounds(bih.bb)[1][2])))
    f = FM.Field()
    sc, nm = NS.load(f.sd)
    out.append(Scene("field", f, sc.nodes[nm[f.bih_id]], f.streams()))
    lat = DM.Lattice()
    out.append(Scene("lattice", lat, lat.bih, lat.streams()))
    return out


@pytest.fixture(scope="module")
def events(scenes_):
    """every event of every packet, per mode: computed once, shared, never written to"""
    ev = {1: [], 2: []}
    per = collections.Counter()
    for s in scenes_:
        for name, mode, res in s.events():
            for r in res:
                ev[mode] += r["events"]
            per[s.name.split()[0] + " " + name] += sum(isinstance(e, DM.Dispatch) for r in res for e in r["events"])
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


# The classes no packet can reach, with their reasons.  A class: (site, axis of the step left, register set of the dispatching code, target, mode).
def unreachable(cls):
    site, axis, rset, target, mode = cls
    if site in ("pop", "root", "reentry") and rset == "B":
        return "a pop, the root and a re-entry fetch the node into set A (L_node2 and the pop's own fetch): their dispatch has no set B form"
    if site == "root" and target == 3:
        return "a tree whose root is a leaf never reaches the walk: bih_tri_wave tests a one-leaf tree per lane"
    return None


def test_every_dispatch_class_is_reached(events):
    every = {(k, a, s, t, m) for (k, a, s) in DM.STEP_SITES for t in DM.TARGETS for m in (1, 2)}
    every |= {(k, None, s, t, m) for k in ("pop", "root", "reentry") for s in "AB" for t in DM.TARGETS for m in (1, 2)}
    seen = collections.Counter((e.site, e.axis, e.set, e.target, e.mode) for m in (1, 2) for e in events[m] if isinstance(e, DM.Dispatch))
    assert set(seen) <= every
    listed = {c for c in every if unreachable(c)}
    assert not (set(seen) & listed), sorted(set(seen) & listed, key=str)
    missing = sorted(every - listed - set(seen), key=str)
    print("classes:", len(every), "listed as unreachable:", len(listed), "reached:", len(seen), "fewest packets' dispatches in a class:", min(seen.values()))
    # a fresh walk starts at the tree's root, whose kind is the tree's: the scenes' roots split every axis between them
    assert not missing, missing


def _pops(ev):
    return [e for e in ev if isinstance(e, DM.Pop)]


def test_the_pop_cases_are_reached(events):
    for mode in (1, 2):
        ev = events[mode]
        pops = _pops(ev)
        # every walk ends by a pop on an empty stack: the block's only way to status 0
        exits = [e for e in ev if isinstance(e, DM.Exit)]
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
        entries = collections.Counter((e.phase, min(e.sp, CAP + 1)) for e in ev if isinstance(e, DM.Entry))
        print("mode", mode, "entries by (phase, min(sp, CAP + 1)):", dict(sorted(entries.items())))
        assert entries[(0, 0)] and entries[(0, CAP)] and entries[(0, CAP + 1)] and entries[(1, CAP)]
        # AN ENTRY WITH phase = 1 AND sp = 0 CANNOT OCCUR: bih_tri_packet_hw sets phase 1 only after a pop from the overflow columns, which leaves
        # sp >= CAP.  The block's answer to it (status 0, am = 0, sp = 0) is held by tests/test_pop_fold_host.py on the model of the pop.
        assert not any(isinstance(e, DM.Entry) and e.phase == 1 and e.sp < CAP for e in ev)


def test_the_leaf_cases_are_reached(events):
    """leaves of 1, 2, 3 and 5 triangles, and hits on the B half of a pair record (odd items: their record index is the A half's plus one), the B
    half of a leaf's LAST record among them; a leaf of odd size ends with a record whose B half is computed and ignored, so its last item is an A"""
    for mode in (1, 2):
        leaves = [e for e in events[mode] if isinstance(e, DM.Leaf)]
        hits = collections.defaultdict(set)
        for e in leaves:
            hits[e.size] |= e.hits
        print("mode", mode, "items hit by leaf size:", {k: sorted(v) for k, v in sorted(hits.items())})
        assert {1, 2, 3, 5} <= set(hits)
        assert 0 in hits[1] and 1 in hits[2] and {1, 2} <= hits[3] and 1 in hits[5]
        assert any(s % 2 == 0 and s - 1 in h for s, h in hits.items())  # the B half of the last record
