"""What the inputs of tests/test_packet_walk_edges.py reach -- asserted without a GPU.

The hand-written packet walk (bih_walk_asm, glome_amd/csrc/bih_packet_asm.hpp) runs only on a GPU, only for a scene whose stack has exactly
kAsmLdsCap LDS entries, and takes its rare paths -- a push or pop beyond those entries, the dump block, the C++ step, re-entry -- only for a
packet that holds more than twelve pending far children.  A GPU test of those paths that a shallow scene or a narrow packet quietly turns into
a test of the C++ walk passes for nothing; so the conditions are stated here, on the ladder scenes and ray streams of tests/ladder.py:

  * the commit's own rules (glome_sb_scene_traits, glome_trace_kernel_choice) send every ladder to the instances that call the walk;
  * tests/packet_walk_model.py walks the tree the product builds (compared through the `show` text);
  * every deep packet, closest-hit and shadow, is modelled at stack depth >= 15 with pushes and pops beyond entry 12, in each of the 8
    octants over combs split on each of the 3 axes; the leaves they test hold 1 .. 9 and 13 triangles; a packet first-hits >= 10 rungs
    while >= 4 of its lanes miss everything; an octant held by one lane of a wave is walked alone and deep;
  * the oracle computing in fp32 agrees with the oracle computing in fp64 on the primitive of every ray (so the GPU test may ask for the
    oracle's primitive on every ray, nothing left out), and its colours stay inside the caps ladder.AWAY_FP32 records;
  * the model itself agrees with the oracle on every lane, and three mutants of it (a lost mask word, an ignored pair half, a dropped clip beyond
    the LDS part) do not: the inputs can tell."""
import collections
import ctypes as C

import numpy as np
import pytest

import ladder
import packet_walk_model as PM
import showfmt
from helpers import oracle_for
from test_trace_choice import export_choice, instance_name
from glome_amd import _lib as L
from glome_amd import api
from oracle import np_scene as NS

VARIANTS = [(a, s, False) for a, s in ladder.CONFIGS] + [(0, 1, True), (2, -1, True)]
IDS = ["%s%s%s" % ("xyz"[a], "+" if s > 0 else "-", "-mirror" if m else "") for a, s, m in VARIANTS]


class Case:
    """a ladder, np_scene's copy of it (the model's tree) and the two oracles"""

    def __init__(self, axis, sign, mirror):
        self.lad = ladder.Ladder(axis, sign, mirror)
        self.sc, self.nm = NS.load(self.lad.sd)
        self.bih = self.sc.nodes[self.nm[self.lad.bih_id]]
        self.sd_of_uid = {self.nm[i]: i for i in range(len(self.nm))}  # np_scene uid -> SceneDesc id
        self._o = {}

    def oracle(self, use_float):
        if use_float not in self._o:
            o, om, _ = oracle_for(self.lad.sd, use_float=use_float)
            self._o[use_float] = (o, om[self.lad.sd.root], {om[i]: i for i in range(len(om))})
        return self._o[use_float]

    def model_prims(self, res):
        """SceneDesc ids of the per-lane hits of a modelled stream (-1: none)"""
        return np.array([self.sd_of_uid[p] if p >= 0 else -1 for r in res for p in r["prim"]])


@pytest.fixture(scope="module")
def cases(built):
    cache = {}

    def get(v):
        if v not in cache:
            cache[v] = Case(*v)
        return cache[v]
    return get


# ---------------------------------------------------------------- 1. the commit's rules send the ladder to the hand-written walk
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_ladder_reaches_the_hand_written_walk(cases, v):
    """bih_tri_wave takes bih_walk_asm when stk.cap == kAsmLdsCap, the tree has the walk's node form, the stack has a dump block (the flat
    tier's launches give it one: ensure_overflow) and the instance is neither faithful nor counting."""
    lad = cases(v).lad
    lib = L.load()
    b = api.Builder()
    nmap, _ = lad.sd.replay(b)
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(b.h, nmap[lad.sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    tier, cls_mask, sec, nested, refract, pk_all, stack_cap, n_bih_nodes, ovf_cap = (int(x) for x in t[:9])
    assert (tier, pk_all, stack_cap) == (0, 1, PM.LDS_CAP) and ovf_cap > 0
    assert stack_cap + ovf_cap >= ladder.COMB_DEPTH + 1  # (the comb's pending entries have somewhere to go)
    assert (cls_mask, sec, nested, refract) == (1, int(v[2]), 0, 0)  # one triangle BIH; the mirror variant has a secondary material
    full = "true" if v[2] else "false"
    for faithful, want in ((0, "k_trace_batch_flat<false,false,%s,TRI,1>" % full), (1, "k_trace_batch_flat<true,true,%s,EVERY,1>" % full)):
        inst = export_choice(lib, [list(t[:8]) + [faithful, 0, 3]])[0, 0]
        assert instance_name(int(inst)) == want


# ---------------------------------------------------------------- 2. the model walks the product's tree
def _np_preorder(node, out):
    if node[0] == "leaf":
        out.append(("leaf", [tuple(map(tuple, PM._tri(s).p)) for s in node[1]]))
    else:
        out.append(("branch", node[1], node[2], node[3]))
        _np_preorder(node[4], out); _np_preorder(node[5], out)
    return out


def _show_preorder(n, out):
    if n[0] == "BihLeaf":
        out.append(("leaf", [tuple(tuple(v[1:]) for v in tri[1:]) for item in n[1] for tri in showfmt.walk(item) if tri[0] == "Triangle"]))
    else:
        out.append(("branch", n[1], n[2], n[3]))
        _show_preorder(n[4], out); _show_preorder(n[5], out)
    return out


@pytest.mark.parametrize("v", VARIANTS[:6], ids=IDS[:6])
def test_model_tree_is_the_products_tree(cases, v):
    """split planes, axes and the triangles of every leaf in order: np_scene's build_rec against the host builder's, through `show`"""
    c = cases(v)
    b = api.Builder()
    nmap, _ = c.lad.sd.replay(b)
    bihs = [x for x in showfmt.walk(showfmt.parse(b.show(nmap[c.lad.sd.root]))) if x[0] == "Bih"]
    assert len(bihs) == 1
    got, want = _show_preorder(bihs[0][2], []), _np_preorder(c.bih.root, [])
    assert got == want
    assert bihs[0][1] == ("Bbox", ("Vec",) + tuple(c.bih.bb[0]), ("Vec",) + tuple(c.bih.bb[1]))
    sizes = sorted(len(x[1]) for x in want if x[0] == "leaf" and x[1])
    assert sizes == sorted(ladder.CLUSTER[:-2] + [3]) and set(range(1, 10)) <= set(sizes) and max(sizes) >= 13
    assert ladder.COMB_DEPTH <= PM.tree_depth(c.bih.root) < 32  # (deeper than kFlatStack and the scene falls to the generic tier)


# ---------------------------------------------------------------- 3. what the packets make the walk do
def _shadow_packets(c):
    """the shadow packets of the screen stream, modelled: its primary rays hit the screen (modelled too), the hits' shadow rays walk in mode 2"""
    o, d, lanes = c.lad.shadow_set()
    prim = PM.walk_stream(c.bih, o, d, 1e6, 1)
    assert np.all(c.model_prims(prim) == c.lad.screen_id)
    t = np.concatenate([r["t"] for r in prim])
    so, sd_, sl = ladder.shadow_rays(c.lad, o, d, t)
    return prim, PM.walk_stream(c.bih, so, sd_, sl, 2), lanes


def test_deep_packets_overflow_the_lds_stack_in_every_octant_on_every_axis(cases):
    seen = {1: set(), 2: set()}
    sizes = {1: collections.Counter(), 2: collections.Counter()}
    for v in VARIANTS[:6]:
        c = cases(v)
        lad = c.lad
        o, d, tilt = lad.deep_set()
        res = PM.walk_stream(c.bih, o, d, 1e6, 1)
        prims = c.model_prims(res).reshape(-1, 64)
        for r, (sv, sw), p in zip(res, tilt, prims):
            (w,) = r["walks"]  # one octant, one walk
            assert (w.octant, w.lanes) == (lad.octant(1, sv, sw), 64)
            assert w.max_depth >= 15 and w.pushes_over >= 1 and w.pops_over >= 1, w
            assert set(w.axes) == {lad.axis}  # every push of the comb is on the ladder's axis
            seen[1].add((w.octant, lad.axis)); sizes[1].update(w.leaf_sizes)
            rungs = {lad.rung_of[x] for x in p if x >= 0 and x != lad.screen_id}
            assert len(rungs) >= 10 and int((p < 0).sum()) >= 4, (len(rungs), int((p < 0).sum()))
        prim, shadow, lanes = _shadow_packets(c)
        for k, r in enumerate(shadow):
            quads = sorted(set(lanes[64 * k:64 * k + 64]))
            assert sorted(w.octant for w in r["walks"]) == sorted(lad.octant(1, -qv, -qw) for qv, qw in quads)
            for w in r["walks"]:
                assert w.max_depth >= 15 and w.pushes_over >= 1 and w.pops_over >= 1, w
                seen[2].add((w.octant, lad.axis)); sizes[2].update(w.leaf_sizes)
            assert 0 < r["occluded"].sum() < 64  # both outcomes in every packet ...
        assert 0.2 <= np.concatenate([r["occluded"] for r in shadow]).mean() <= 0.8  # ... and both common over the stream (the oracle's own share: section 4)
    every = {(o, a) for o in range(8) for a in range(3)}
    assert seen[1] == every and seen[2] == every
    for mode in (1, 2):
        assert set(range(1, 10)) <= set(sizes[mode]) and max(sizes[mode]) >= 13, sizes[mode]


def test_mixed_packets_are_what_they_say(cases):
    for v in VARIANTS[:6]:
        c = cases(v)
        o, d, what = c.lad.mixed_set()
        res = dict(zip(what, PM.walk_stream(c.bih, o, d, 1e6, 1)))
        deep = lambda w: w.max_depth >= 15 and w.pushes_over >= 1 and w.pops_over >= 1
        assert [w.lanes for w in res["2 octants, alternating lanes"]["walks"]] == [32, 32] and all(map(deep, res["2 octants, alternating lanes"]["walks"]))
        assert [w.lanes for w in res["4 octants, 16 lanes each"]["walks"]] == [16] * 4 and all(map(deep, res["4 octants, 16 lanes each"]["walks"]))
        for name in ("8 octants", "8 octants, uneven"):
            ws = res[name]["walks"]
            assert sorted(w.octant for w in ws) == list(range(8)) and sum(w.lanes for w in ws) == 64
            assert sum(map(deep, ws)) >= 3 and sum(w.max_depth <= 2 for w in ws) == 4  # the four octants that run the comb backwards hold an entry or two
        for lane in (0, 31, 32, 63):
            ws = res["single lane %d" % lane]["walks"]
            assert sorted(w.lanes for w in ws) == [1, 63] and all(map(deep, ws))
            assert [w.lanes for w in ws] == ([1, 63] if lane == 0 else [63, 1])  # (the walks are made lowest lane first)
        ws = res["four single deep lanes among shallow ones"]["walks"]
        assert [w.lanes for w in ws] == [4, 60] and deep(ws[0]) and ws[1].max_depth <= 2
        (w,) = res["deep lanes between lanes that miss the bounds"]["walks"]
        assert w.lanes == 32 and deep(w)
        ws = res["4 octants between lanes that miss the bounds"]["walks"]
        assert len(ws) == 4 and sum(w.lanes for w in ws) == 22 and any(map(deep, ws))
        (w,) = res["eight deep lanes in the high half only"]["walks"]
        assert w.lanes == 8 and deep(w)


def test_the_frame_along_the_ladder_is_deep(cases):
    """the frame of the GPU suite, cut into the work items of its launch (glome_items_layout: the whole-frame plan of 64 x 64 work tiles, 8 x 8
    blocks and the 64-pixel strips of the ragged edges): no ray is parallel to an axis, most items run the whole comb, some hold more than one
    octant (the axis runs through the frame), and some pixels see a rung"""
    from helpers import product_camera_lights
    lib = L.load()
    w, h = ladder.FRAME_W, ladder.FRAME_H
    P = api.render_params(width=w, height=h, maxdepth=3)
    n = lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)
    items = np.full((n, 64, 4), -7, dtype=np.int32)
    assert lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, items.ctypes.data_as(L.c_ip), n) == n
    assert int((items[..., 0] == 1).sum()) == w * h
    for v in (VARIANTS[0], VARIANTS[5]):
        c = cases(v)
        cam, _ = product_camera_lights(c.lad.sd)
        o, d = api.frame_rays(cam, w, h)
        assert np.all(d != 0)
        o, d = o.reshape(h, w, 3), d.reshape(h, w, 3)
        deep = walks = hits = 0
        for it in items:
            lanes = it[it[:, 0] == 1]
            r = PM.walk_packet(c.bih, o[lanes[:, 2], lanes[:, 1]], d[lanes[:, 2], lanes[:, 1]], 1e6, 1)
            deep += r["max_depth"] >= 15 and r["pushes_over"] >= 1 and r["pops_over"] >= 1
            walks = max(walks, len(r["walks"])); hits += int((r["prim"] >= 0).sum())
        assert deep >= n // 2 and walks >= 2 and 0.05 < hits / (w * h) < 0.9, (deep, n, walks, hits)


# ---------------------------------------------------------------- 4. the oracle in fp32 and in fp64: the same primitive for every ray
def _streams(lad):
    return {"deep": lad.deep_set()[:2], "shadow": lad.shadow_set()[:2], "mixed": lad.mixed_set()[:2]}


@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_fp32_and_fp64_oracles_agree_on_every_ray(cases, v):
    """The margins of tests/ladder.py (Ladder.clear) are wide enough: the oracle computing in fp32 reports the fp64 oracle's primitive for every
    ray of every stream, traces the same number of rays, keeps every depth inside 1e-4, and its colours leave the 1e-4 gate on no more rays than
    ladder.AWAY_FP32 records (the GPU tests allow twice that) -- under 1 % of any stream."""
    c = cases(v)
    o64, r64, inv64 = c.oracle(False)
    o32, r32, inv32 = c.oracle(True)
    for name, (ro, rd) in _streams(c.lad).items():
        a, b = (o.rayint(r, ro.astype(np.float64), rd.astype(np.float64)) for o, r in ((o64, r64), (o32, r32)))
        pa = np.array([inv64[p] if p >= 0 else -1 for p in a["prim"]]); pb = np.array([inv32[p] if p >= 0 else -1 for p in b["prim"]])
        assert np.array_equal(pa, pb), (name, np.flatnonzero(pa != pb))
        assert np.array_equal(a["t"] >= 0, b["t"] >= 0)
        ref, c64 = ladder.oracle_trace(o64, ro, rd, 3)
        got, c32 = ladder.oracle_trace(o32, ro, rd, 3)
        assert c64 == c32, (name, c64, c32)
        hit = ref[:, 4] < 1e6
        assert np.array_equal(hit, a["t"] >= 0) and np.all(np.abs(got[hit, 4] - ref[hit, 4]) <= 1e-4 * np.maximum(1.0, ref[hit, 4]))
        away = int(ladder.colour_away(got, ref).sum())
        print("fp32 oracle", IDS[VARIANTS.index(v)], name, "rays", len(ro), "away", away, "counts", c64)
        cap = ladder.AWAY_FP32[("mirror" if v[2] else "plain", name)]
        assert away <= cap and 2 * cap <= 0.01 * len(ro), (name, away, cap)
        if name == "shadow":  # both outcomes are common among the shadow rays that leave the screen
            so, sd_, sl = ladder.shadow_rays(c.lad, ro, rd, a["t"])
            occluded = o64.shadow(r64, so, sd_, sl).mean()
            assert c64["rays_shadow"] == len(ro) and 0.2 <= occluded <= 0.8, occluded


# ---------------------------------------------------------------- 5. the model agrees with the oracle; its mutants do not
@pytest.mark.parametrize("v", [VARIANTS[0], VARIANTS[3], VARIANTS[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_model_finds_the_oracles_primitives_and_its_mutants_do_not(cases, v):
    """The model's per-lane hit is the fp64 oracle's on every ray of the deep and the mixed stream -- duplicates included: the later item of a tie.
    The model's three mutants (packet_walk_model.MUTANTS: an entry beyond the LDS part that loses the high word of its lane mask, the B half of every
    pair of a leaf ignored, the early-out's clip dropped at pops from beyond the LDS part under the hand-written walk's own acceptance, t <= far
    alone) each get rays of the deep stream wrong: the streams can tell.  These are mutants of the MODEL: the hand-written walk cannot run without a GPU and the
    host build's wave is one lane; what the like changes do to the host-compiled C++ walk is recorded in DESIGN.md 4.1c."""
    c = cases(v)
    o64, r64, inv64 = c.oracle(False)
    want = {}
    for name in ("deep", "mixed"):
        ro, rd = _streams(c.lad)[name]
        a = o64.rayint(r64, ro.astype(np.float64), rd.astype(np.float64))
        want[name] = np.array([inv64[p] if p >= 0 else -1 for p in a["prim"]])
        assert np.array_equal(c.model_prims(PM.walk_stream(c.bih, ro, rd, 1e6, 1)), want[name]), name
    ro, rd = _streams(c.lad)["deep"]
    for mutant in PM.MUTANTS:
        got = c.model_prims(PM.walk_stream(c.bih, ro, rd, 1e6, 1, mutant))
        wrong = int((got != want["deep"]).sum())
        print("mutant", mutant, "wrong rays", wrong, "of", len(ro))
        assert wrong >= 8, (mutant, wrong)
