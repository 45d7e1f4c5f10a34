"""The tree builders at their edges, without a GPU: tests/tree_build_model.py (the level-by-level build of bih_build_device.hpp
restated in fp64) against the host builders (Graph::BihBuild, Graph::MeshBuild) and the oracle's `bih` on every case of
tests/tree_build_cases.py, bit for bit; what each case reaches; the pool bounds of the device builder; and the inputs on which
the reference's build_rec does not terminate, which glome_sb_bih refuses with a status."""
import os
import re

import numpy as np
import pytest

import showfmt
import tree_build_cases as TC
import tree_build_model as M
from helpers import ROOT, O
from glome_amd import _lib as L
from glome_amd import api

BUILDS = [c for c in TC.CASES if c.refusal is None]
REFUSALS = [c for c in TC.CASES if c.refusal is not None]
STATUS = {"E_SCENE": L.E_SCENE, "E_LIMIT": L.E_LIMIT, "E_INVALID": L.E_INVALID}
KINDS = {"leaf_size", "leaf_cost", "pick_x", "pick_y", "pick_z", "pick_b", "chain_differs", "tie", "tie_xy", "empty_side",
         "wave_uniform", "wave_mixed", "wave_first_inactive", "wave_tail", "wave_leaf_and_active", "wave_uniform_first_inactive", "wave_uniform_leaf_and_active",
         "seg_straddles_1024", "seg_starts_on_1024", "over_4n_nodes", "over_512_levels", "depth_at_limit", "depth_over_limit"}
_models = {}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def item_boxes(b, ids):
    bx = np.array([b.bound(i) for i in ids]).reshape(-1, 6)
    return bx[:, :3], bx[:, 3:]


def model_of(case):
    """the model's tree of a case (or the Loop it raised), made once"""
    if case.name not in _models:
        try:
            if case.kind == "bih":
                b = api.Builder()
                _models[case.name] = M.build_bih(*item_boxes(b, case.make(b)))
            else:
                V, T = case.make()
                _models[case.name] = M.build_mesh(V, T)
        except M.Loop as e:
            _models[case.name] = e
    return _models[case.name]


def assert_bih_is_model(b, node, ids, T):
    ls, rs, ax, nl, items = b.bih_dump(node)
    assert np.array_equal(ax, T.axis) and np.array_equal(nl, T.nleaf)
    assert np.array_equal(bits(ls), bits(T.lsplit)) and np.array_equal(bits(rs), bits(T.rsplit))
    assert np.array_equal(items, np.asarray(ids)[T.items])
    assert np.array_equal(bits(b.bound(node)), bits(T.bound))


def shown_mesh(text):
    """the `show` text of a Mesh as (bound, the preorder of its BVH in the model's form)"""
    si = showfmt.parse(text)
    assert si[0] == "SI" and si[1][0] == "Mesh"
    _, _, _, bbox, bvh = si[1]
    vec = lambda v: np.array(v[1:], np.float64)
    box = lambda bb: (vec(bb[1]), vec(bb[2]))
    pre, stack = [], [bvh]
    while stack:
        nd = stack.pop()
        if nd[0] == "Leaf":
            pre.append(("Leaf", list(nd[1])))
        else:
            pre.append(("Branch",) + box(nd[1]) + box(nd[2]))
            stack += [nd[4], nd[3]]
    return np.concatenate(box(bbox)), pre


def assert_mesh_is_model(b, node, T):
    bound, pre = shown_mesh(b.show(node))
    assert len(pre) == len(T.preorder)
    for got, want in zip(pre, T.preorder):
        assert got[0] == want[0]
        if got[0] == "Leaf":
            assert got[1] == want[1]
        else:
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got[1:], want[1:])), (got, want)
    assert np.array_equal(bits(bound), bits(T.bound)) and np.array_equal(bits(b.bound(node)), bits(T.bound))
    branches = sum(1 for p in T.preorder if p[0] == "Branch")
    assert b.primcount(node) == (T.n, 0, branches)  # Mesh.hs:201-205


def assert_reaches(case, T):
    for want in case.reaches:
        if want.startswith("root:"):
            assert want[5:] in T.record["nodes"][0], (case, want, T.record["nodes"][0])
        else:
            assert want in T.reached, (case, want, sorted(T.reached))


@pytest.mark.parametrize("case", BUILDS, ids=repr)
def test_model_is_the_host_builders_tree(built, case):
    """every case that builds: the model's tree is the host builder's, bit for bit; the case went where it was written to go; and the
    tree fits the device builder's pools (bihdev::kNodeCap, kAccCap)"""
    T = model_of(case)
    b = api.Builder()
    if case.kind == "bih":
        ids = case.make(b)
        assert_bih_is_model(b, b.bih(ids), ids, T)
    else:
        V, Tr = case.make()
        assert_mesh_is_model(b, b.mesh(V, np.zeros((0, 3)), Tr, []), T)
    assert_reaches(case, T)
    assert T.n_nodes <= M.node_cap(T.n) and T.widest <= M.acc_cap(T.n), (T.n, T.n_nodes, T.widest)


@pytest.mark.parametrize("case", [c for c in BUILDS if c.kind == "bih" and c.oracle], ids=repr)
def test_model_is_the_oracles_bih(built, case):
    """the same tree from the oracle's restatement of Bih.hs (its own recursion, its own bounds)"""
    T = model_of(case)
    o = O.Oracle()
    ids = case.make(o)
    ls, rs, ax, nl, items = o.bih_dump(o.bih(ids))
    assert np.array_equal(ax, T.axis) and np.array_equal(nl, T.nleaf)
    assert np.array_equal(bits(ls), bits(T.lsplit)) and np.array_equal(bits(rs), bits(T.rsplit))
    assert np.array_equal(items, np.asarray(ids)[T.items])
    assert np.array_equal(bits(o.bound(o.bih(ids))), bits(T.bound))


def test_the_table_reaches_every_kind_of_record(built):
    seen = set()
    for case in BUILDS:
        seen |= model_of(case).reached
    assert KINDS <= seen, sorted(KINDS - seen)
    assert seen <= KINDS, sorted(seen - KINDS)  # a kind the model records and this list forgot


def test_pool_sizes_and_level_limit_are_the_device_builders(built):
    """the model's copies of kNodeCap, kAccCap and kMaxLevels are what bih_build_device.hpp compiles, and glome_hip.h states the limit"""
    src = open(os.path.join(ROOT, "glome_amd", "csrc", "bih_build_device.hpp")).read()
    assert re.search(r"kNodeCap\(long long n\) \{ return 14 \* n \+ 16; \}", src) and M.node_cap(7) == 14 * 7 + 16
    assert re.search(r"kAccCap\(long long n\) \{ return n \+ n / 3 \+ 2; \}", src) and M.acc_cap(7) == 7 + 7 // 3 + 2
    assert int(re.search(r"constexpr int kMaxLevels = (\d+);", src).group(1)) == M.MAX_LEVELS
    hdr = open(os.path.join(ROOT, "include", "glome_hip.h")).read()
    assert ("%d levels" % M.MAX_LEVELS) in hdr


@pytest.mark.parametrize("case", REFUSALS, ids=repr)
def test_refusals_are_statuses_and_leave_the_builder_usable(built, case):
    """glome_sb_bih / glome_sb_mesh on the inputs they must refuse: the status and message, no node added, and the next build on the same builder is
    right.  The loops (four points, boxes without surface, areas that underflow, a vertex at infinity) ended the process by stack exhaustion
    before."""
    b = api.Builder()
    if case.refusal in (TC.LOOP, TC.MESH_LOOP):
        assert isinstance(model_of(case), M.Loop)
    if case.kind == "bih":
        arr, p = L.ivec(case.make(b))
        call = lambda: b.lib.glome_sb_bih(b.h, p, len(arr))
    else:
        V, Tr = case.make()
        call = lambda: b.lib.glome_sb_mesh(b.h, V.ctypes.data_as(L.c_dp), len(V), None, 0, Tr.ctypes.data_as(L.c_ip), len(Tr), None, 0)
    before = b.sphere((0.0, 0.0, 0.0), 1.0)
    assert call() == STATUS[case.refusal[0]]
    assert re.search(case.refusal[1], b.lib.glome_sb_last_error(b.h).decode())
    assert b.sphere((0.0, 0.0, 0.0), 1.0) == before + 1  # the refused bih left no node behind
    ids = TC.ORDINARY.make(b)
    assert_bih_is_model(b, b.bih(ids), ids, model_of(TC.ORDINARY))


def test_four_points_through_nff_text(built):
    """glome_sb_load_nff builds its `bih` through the same constructor"""
    text = "b 0.1 0.1 0.1\nv\nfrom 0 0 -5\nat 0 0 0\nup 0 1 0\nangle 40\nhither 1\nresolution 8 8\nl 0 5 -5\nf 1 1 1 1 0 0 0 0\n" + "".join("s %d 0 0 0\n" % i for i in range(4))
    b = api.Builder()
    with pytest.raises(api.GlomeError, match=r"does not terminate.*status -2"):
        b.load_nff(text)
    root = b.load_nff(text.replace("s 3 0 0 0\n", ""))[0]  # three of them build
    assert b.primcount(root)[0] == 3
