"""What the inputs of tests/test_mesh_packet_walk_edges.py reach -- asserted without a GPU.

The Mesh packet walk (mesh_closest_wave, glome_amd/csrc/rt_device.hpp) runs only on a GPU, only in the non-faithful, non-counting MESH
instances, and takes its rare paths -- a node visited in three passes, a push or a pop in the global overflow columns, both at once -- only
for a packet whose lanes disagree about a node's order while more than twelve entries are pending.  A GPU test of those paths that a
shallow scene or a coherent packet quietly turns into a test of the common path passes for nothing; so the conditions are stated here, on
the scenes and ray streams of tests/mesh_ladder.py:

  * the commit's own rules (glome_sb_scene_traits, glome_trace_kernel_choice, glome_kernel_choice) send every variant to the instances that
    call the walk, with a 12-entry LDS stack and overflow columns for two entries more than the model ever holds;
  * tests/mesh_packet_model.py walks the tree the product builds (compared through the `show` text): depth 24, leaves of 1 .. 9, 13, 15 and
    20 triangles;
  * every deep packet is modelled at 27 or 28 entries (at least 20 asserted), with 75 .. 117 pushes and as many pops beyond entry 12, three
    passes at 20 .. 35 nodes met with the LDS part full (at least 8 asserted), a leaf of 15 or 20 triangles tested, 29 or more different rungs
    and patch cells first hit and 5 lanes that miss -- on all six axis and sign variants;
  * the oracle computing in fp32 agrees with the oracle computing in fp64 on the primitive, the texture and the ray counts of every ray,
    and its colours stay inside the caps mesh_ladder.AWAY_FP32 records (0);
  * the model itself finds the fp64 oracle's hit on every lane -- the mesh (the second of the twin), the distance and the material, which
    among exact duplicates tells which one was kept -- and three mutants of it (the third pass dropped, an overflow entry that loses the
    intervals of lanes 32 .. 63, the later-left lanes' interval taken from the right child) do not: the inputs can tell."""
import collections
import ctypes as C

import numpy as np
import pytest

import ladder
import mesh_ladder as ML
import mesh_packet_model as MM
from helpers import oracle_for, product_camera_lights
from test_kernel_choice import export_choice as render_choice, instance_name as render_instance_name
from test_mesh_refit_host import box, mesh_of, shape
from test_trace_choice import CLS_MESH, export_choice, instance_name
from glome_amd import _lib as L
from glome_amd import api
from oracle import np_scene as NS

VARIANTS, IDS = ML.VARIANTS, ML.IDS
PLAIN = VARIANTS[:6]


class Case:
    """a mesh ladder, np_scene's copy of it (the model's trees), its streams, their modelled walks and the two oracles"""

    def __init__(self, v):
        self.lad = ML.MeshLadder(*v)
        self.sc, self.nm = NS.load(self.lad.sd)
        self.meshes = [self.sc.nodes[self.nm[i]] for i in self.lad.mesh_ids]
        self.streams = self.lad.streams()
        self.what = self.lad.mixed_set()[2]
        self.model = {name: MM.walk_stream(self.meshes, o, d) for name, (o, d) in self.streams.items()}
        self._o = {}

    def oracle(self, use_float):
        """(oracle, its root, oracle uid -> SceneDesc id, SceneDesc material -> oracle material)"""
        if use_float not in self._o:
            o, om, mm = oracle_for(self.lad.sd, use_float=use_float)
            self._o[use_float] = (o, om[self.lad.sd.root], {om[i]: i for i in range(len(om))}, mm)
        return self._o[use_float]

    def lanes(self, res):
        """per lane of a modelled stream: the SceneDesc id of the mesh hit (-1: none), the distance, the SceneDesc material of the triangle"""
        tri = np.concatenate([r["tri"] for r in res]); which = np.concatenate([r["which"] for r in res])
        mesh = np.where(which >= 0, np.asarray(self.lad.mesh_ids)[np.maximum(which, 0)], -1)
        mat = np.where(tri >= 0, np.asarray(self.lad.mats)[self.lad.tris[np.maximum(tri, 0), 6]], -1)
        return mesh, np.concatenate([r["t"] for r in res]), mat, tri

    def oracle_lanes(self, ro, rd, use_float=False):
        """the same of the oracle's rayint"""
        o, root, inv, mm = self.oracle(use_float)
        a = o.rayint(root, ro.astype(np.float64), rd.astype(np.float64))
        hit = a["prim"] >= 0
        assert np.array_equal(hit, a["t"] >= 0) and np.all(a["ntex"][hit] == 1)
        mat_of = {m: i for i, m in enumerate(mm)}
        return np.array([inv[p] if p >= 0 else -1 for p in a["prim"]]), a["t"], np.array([mat_of[x] if h else -1 for x, h in zip(a["tex"][:, 0], hit)])


@pytest.fixture(scope="module")
def cases(built):
    cache = {}

    def get(v):
        if v not in cache:
            cache[v] = Case(v)
        return cache[v]
    return get


def _traits(lib, lad):
    b = api.Builder()
    nmap, _ = lad.sd.replay(b)
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(b.h, nmap[lad.sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return b, nmap, t


def _frame_items(lib):
    w, h = ML.FRAME_W, ML.FRAME_H
    P = api.render_params(width=w, height=h, maxdepth=3)
    n = lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)
    items = np.full((n, 64, 4), -7, dtype=np.int32)
    assert lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, items.ctypes.data_as(L.c_ip), n) == n
    assert int((items[..., 0] == 1).sum()) == w * h
    return items


# ---------------------------------------------------------------- 1. the commit's rules send the mesh ladder to the packet walk
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_mesh_ladder_reaches_the_packet_walk(cases, v):
    """closest_flat calls mesh_closest_wave in the WAVE instances that are neither faithful nor counting (rt_device.hpp); the walk's `err` exit is
    sp + 2 > stack_cap + ovf_cap, which commit sizes as min(kFlatStackMesh, 2 * depth): two entries more than the model ever holds."""
    c = cases(v)
    lib = L.load()
    _, _, t = _traits(lib, c.lad)
    tier, cls_mask, sec, nested, refract, pk_all, stack_cap, n_bih_nodes, ovf_cap, _, n_mesh_nodes = (int(x) for x in t)
    assert (tier, cls_mask, stack_cap) == (0, CLS_MESH, MM.LDS_CAP) and n_mesh_nodes > 0
    assert (sec, nested, refract) == (int(c.lad.mirror), 0, 0)
    max_sp = max(r["max_sp"] for res in c.model.values() for r in res)
    print("stack", IDS[VARIANTS.index(v)], "cap", stack_cap, "+", ovf_cap, "model's largest sp", max_sp, "mesh nodes", n_mesh_nodes)
    assert stack_cap + ovf_cap >= max_sp + 2
    full = "true" if c.lad.mirror else "false"
    for faithful, want in ((0, "k_trace_batch_flat<false,false,%s,MESH,1>" % full), (1, "k_trace_batch_flat<true,true,%s,EVERY,1>" % full)):
        assert instance_name(int(export_choice(lib, [list(t[:8]) + [faithful, 0, 3]])[0, 0])) == want
    items = len(_frame_items(lib))
    for faithful, want in ((0, "k_render_flat<false,false,%s,MESH,1,false>" % full), (1, "k_render_flat<true,true,%s,EVERY,1,false>" % full)):
        kind, inst, two_rows, cap = render_choice(lib, [list(t[:8]) + [0, faithful, 0, 3, 1, items]])[0].tolist()
        assert (render_instance_name(kind, inst), two_rows) == (want, 0)


# ---------------------------------------------------------------- 2. the model walks the product's tree
def _np_shape(node):
    return ("Leaf", tuple(node[1])) if node[0] == "leaf" else ("Branch", _np_shape(node[3]), _np_shape(node[4]))


def _boxes(bvh, out, np_form):
    if bvh[0] in ("Leaf", "leaf"):
        return out
    out += [np.concatenate(bvh[1]), np.concatenate(bvh[2])] if np_form else [box(bvh[1]), box(bvh[2])]
    _boxes(bvh[3], out, np_form); _boxes(bvh[4], out, np_form)
    return out


@pytest.mark.parametrize("v", VARIANTS[:6] + VARIANTS[8:9], ids=IDS[:6] + IDS[8:9])
def test_model_tree_is_the_products_tree(cases, v):
    """leaf lists in order, nesting and every box: np_scene's build_tree against the host builder's, through `show`; the tree is deeper than the LDS
    part of the stack and shallower than kFlatStack (a deeper one sends the scene to the generic tier); the leaf sizes of mesh_ladder are there"""
    c = cases(v)
    b, nmap, _ = _traits(L.load(), c.lad)
    for mid, mesh in zip(c.lad.mesh_ids, c.meshes):
        got = mesh_of(b.show(nmap[mid]))
        assert shape(got[4]) == _np_shape(mesh.bvh)
        assert np.array_equal(np.array(_boxes(got[4], [], False)), np.array(_boxes(mesh.bvh, [], True)))
        assert np.array_equal(box(got[3]), np.concatenate(mesh.bb))
        assert len(got[2]) == len(mesh.tris) == len(c.lad.tris)
    sizes = sorted(len(x) for x in MM.leaves(c.meshes[0].bvh))
    depth = MM.tree_depth(c.meshes[0].bvh)
    print("tree", IDS[VARIANTS.index(v)], "depth", depth, "leaf sizes", sizes)
    assert set(range(1, 10)) | {13, 15, 20} <= set(sizes) and min(sizes) >= 1
    assert MM.LDS_CAP < depth < 32
    for j, ndup in ML.DUPLICATES.items():  # the duplicates: the same three vertex indices, first in their leaf or last
        (leaf,) = [x for x in MM.leaves(c.meshes[0].bvh) if c.lad.rung_ids[j][0] in x]
        assert leaf == c.lad.rung_ids[j]
        dup = leaf[-ndup:] if j in ML.DUP_AT_END else leaf[:ndup]
        assert len({tuple(c.lad.tris[t, :3]) for t in dup}) == 1 and len({tuple(c.lad.tris[t, :3]) for t in leaf}) == len(leaf) - ndup + 1


# ---------------------------------------------------------------- 3. what the packets make the walk do
def _report(tag, r):
    print(tag, "sp", r["max_sp"], "pushes/pops beyond %d:" % MM.LDS_CAP, r["pushes_over"], r["pops_over"], "three-pass nodes", r["three_pass"],
          "with sp >= %d:" % MM.LDS_CAP, r["three_pass_over"], "leaves", dict(sorted(r["leaf_sizes"].items())))


def test_deep_packets_take_three_passes_beyond_the_lds_stack_on_every_axis(cases):
    sizes = collections.Counter()
    for v in PLAIN:
        c = cases(v)
        o, d = c.streams["deep"]
        assert np.all(c.lad.local(d)[:, 0] > 0)  # forward
        tilt = (c.lad.local(d)[:, 1] > 0) * 1 + (c.lad.local(d)[:, 2] > 0) * 2
        for k, r in enumerate(c.model["deep"]):
            _report("deep %s packet %d" % (IDS[VARIANTS.index(v)], k), r)
            assert r["max_sp"] >= 20 and r["pushes_over"] >= 1 and r["pops_over"] >= 1, r
            assert r["three_pass_over"] >= 8 and max(r["leaf_sizes"]) >= 15, r
            places = {c.lad.place_of(t) for t in r["tri"] if t >= 0}
            assert len(places) >= 8 and int((r["tri"] < 0).sum()) >= 4, (len(places), r["tri"])
            assert any(p[0] == "rung" for p in places) and any(p[0] == "cell" for p in places)  # some lanes go on through the holes to the rungs
            assert set(tilt[64 * k:64 * k + 64]) == {0, 1, 2, 3}  # the four tilt-sign quadrants in every packet
            sizes.update(r["leaf_sizes"])
    assert set(range(1, 10)) | {13, 15, 20} <= set(sizes), sizes


def test_mixed_packets_are_what_they_say(cases):
    for v in PLAIN:
        c = cases(v)
        lad, mesh = c.lad, c.meshes[0]
        o, d = c.streams["mixed"]
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        fwd = lad.local(d)[:, 0] > 0
        near, far = MM.clip(o64, 1.0 / d64, mesh.bb)
        enters = ~((near > far) | (far < 0))
        inside = np.all((o64 > np.asarray(mesh.bb[0])) & (o64 < np.asarray(mesh.bb[1])), axis=1)
        res = dict(zip(c.what, c.model["mixed"]))
        at = {name: slice(64 * k, 64 * k + 64) for k, name in enumerate(c.what)}
        odd = np.arange(64) % 2 == 1
        deep = lambda r: r["max_sp"] >= 20 and r["pushes_over"] >= 1 and r["pops_over"] >= 1 and r["three_pass_over"] >= 8
        for name, r in res.items():
            _report("mixed %s %s:" % (IDS[VARIANTS.index(v)], name), r)
        name = "forward and reverse lanes alternating"
        assert np.array_equal(fwd[at[name]], odd) and enters[at[name]].all() and deep(res[name])
        for lane in (0, 31, 32, 63):
            name = "one reverse lane at %d" % lane
            assert np.array_equal(~fwd[at[name]], np.arange(64) == lane) and enters[at[name]].all() and deep(res[name]) and res[name]["tri"][lane] >= 0
        name = "deep lanes between lanes that miss the bounds"
        assert np.array_equal(enters[at[name]], odd) and np.all(res[name]["tri"][~odd] < 0) and deep(res[name])
        name = "eight deep lanes in the high half only"
        high = (np.arange(64) >= 32) & (np.arange(64) < 40)
        assert np.array_equal(enters[at[name]], high) and np.all(res[name]["tri"][~high] < 0) and (res[name]["tri"][high] >= 0).sum() >= 6
        assert res[name]["max_sp"] > MM.LDS_CAP and res[name]["pushes_over"] >= 1 and res[name]["pops_over"] >= 1  # (eight lanes alone still overflow)
        name = "lanes that start inside the box"
        gaps = np.floor(np.log2(ladder.rung_u(0) / lad.local(o)[at[name], 0]))  # between which two rungs a lane starts
        assert inside[at[name]].all() and not inside[at["forward and reverse lanes alternating"]][odd].any() and len(set(gaps)) >= 12
        assert 16 <= fwd[at[name]].sum() <= 48 and deep(res[name])


def test_the_frame_along_the_comb_is_deep(cases):
    """the frame of the GPU suite, cut into the work items of its launch (glome_items_layout: 8 x 8 blocks and the 64-pixel strips of the ragged
    edges): no ray is parallel to an axis, and most items -- here all of them -- push and pop beyond the LDS part of the stack; between 5 % and
    90 % of the pixels hit"""
    items = _frame_items(L.load())
    w, h = ML.FRAME_W, ML.FRAME_H
    for v in (VARIANTS[0], VARIANTS[5]):
        c = cases(v)
        cam, _ = product_camera_lights(c.lad.sd)
        o, d = api.frame_rays(cam, w, h)
        assert np.all(d != 0)
        o, d = o.reshape(h, w, 3), d.reshape(h, w, 3)
        over = three = hits = 0
        for it in items:
            lanes = it[it[:, 0] == 1]
            r = MM.walk_packet(c.meshes[0], o[lanes[:, 2], lanes[:, 1]], d[lanes[:, 2], lanes[:, 1]])
            over += r["pushes_over"] >= 1 and r["pops_over"] >= 1
            three += r["three_pass_over"] >= 1; hits += int((r["tri"] >= 0).sum())
        print("frame", IDS[VARIANTS.index(v)], "items", len(items), "beyond the LDS part", over, "three passes there", three, "hit share", hits / (w * h))
        assert over > len(items) // 2 and three >= 1 and 0.05 < hits / (w * h) < 0.9, (over, len(items), three, hits)


# ---------------------------------------------------------------- 4. the oracle in fp32 and in fp64: the same hit for every ray
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_fp32_and_fp64_oracles_agree_on_every_ray(cases, v):
    """The margins of Ladder.clear are wide enough for the mesh ladder too: the oracle computing in fp32 reports the fp64 oracle's primitive and
    texture for every ray of the deep and the mixed stream, traces the same number of rays, keeps every depth inside 1e-4, and its colours leave
    the 1e-4 gate on no more rays than mesh_ladder.AWAY_FP32 records (the GPU tests allow twice that) -- under 1 % of either stream.  A Mesh
    casts no shadow: every hit on a Surface material sends one shadow ray, which comes back lit."""
    c = cases(v)
    o64, o32 = c.oracle(False)[0], c.oracle(True)[0]
    for name, (ro, rd) in c.streams.items():
        pa, ta, ma = c.oracle_lanes(ro, rd, False)
        pb, tb, mb = c.oracle_lanes(ro, rd, True)
        assert np.array_equal(pa, pb) and np.array_equal(ma, mb), (name, np.flatnonzero((pa != pb) | (ma != mb)))
        assert set(pa) == {-1, c.lad.mesh_ids[-1]}  # (the twin: every hit is the second mesh's)
        ref, c64 = ladder.oracle_trace(o64, ro, rd, 3)
        got, c32 = ladder.oracle_trace(o32, ro, rd, 3)
        assert c64 == c32 and c64["rays_primary"] == len(ro), (name, c64, c32)
        hit = ref[:, 4] < 1e6
        assert np.array_equal(hit, pa >= 0) and np.all(np.abs(got[hit, 4] - ref[hit, 4]) <= 1e-4 * np.maximum(1.0, ref[hit, 4]))
        if c.lad.mirror:
            assert c64["rays_secondary"] >= int((ma == c.lad.mats[1]).sum()) > 0.2 * len(ro)
        else:
            assert c64["rays_secondary"] == 0 and c64["rays_shadow"] == int(hit.sum())
        away = int(ladder.colour_away(got, ref).sum())
        print("fp32 oracle", IDS[VARIANTS.index(v)], name, "rays", len(ro), "hits", int(hit.sum()), "away", away, "counts", c64)
        cap = ML.AWAY_FP32[(c.lad.kind, name)]
        assert away <= cap and 2 * cap <= 0.01 * len(ro), (name, away, cap)


# ---------------------------------------------------------------- 5. the model agrees with the oracle; its mutants do not
@pytest.mark.parametrize("v", [VARIANTS[0], VARIANTS[3], VARIANTS[4], VARIANTS[8]], ids=[IDS[0], IDS[3], IDS[4], IDS[8]])
def test_model_finds_the_oracles_hits_and_its_mutants_do_not(cases, v):
    """The model's per-lane hit is the fp64 oracle's on every ray of the deep and the mixed stream: the mesh (of the twin the second: an exact tie,
    which nearest gives to the later operand), the distance to 1e-12 and the material -- the duplicates of a cluster alternate between the two
    materials, so the material says that the LAST of them was kept.  The model's three mutants (mesh_packet_model.MUTANTS) each get rays of the
    deep stream wrong: the streams can tell.  These are mutants of the MODEL: the packet walk cannot run without a GPU and the host build's wave
    is one lane; what the like changes do to the kernel's source is recorded in DESIGN.md."""
    c = cases(v)
    want = {}
    for name, (ro, rd) in c.streams.items():
        want[name] = c.oracle_lanes(ro, rd)
        mesh, t, mat, _ = c.lanes(c.model[name])
        hit = mesh >= 0
        assert np.array_equal(mesh, want[name][0]) and np.array_equal(mat, want[name][2]), name
        assert np.all(np.abs(t - want[name][1])[hit] <= 1e-12 * np.maximum(1.0, t[hit])), name
    dup = [t for j in ML.DUPLICATES for t in c.lad.rung_ids[j]]
    assert np.isin(c.lanes(c.model["deep"])[3], dup).sum() >= 20  # (ties inside a leaf are among the first hits)
    ro, rd = c.streams["deep"]
    for mutant in MM.MUTANTS:
        mesh, t, mat, _ = c.lanes(MM.walk_stream(c.meshes, ro, rd, mutant=mutant))
        wrong = int(((mesh != want["deep"][0]) | (mat != want["deep"][2]) | (np.abs(t - want["deep"][1]) > 1e-12 * np.maximum(1.0, np.abs(t)))).sum())
        print("mutant", mutant, "wrong rays", wrong, "of", len(ro))
        assert wrong >= 8, (mutant, wrong)
