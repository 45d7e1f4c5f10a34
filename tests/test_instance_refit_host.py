"""glome_sb_instance_set_transforms: new matrices for Instances, and the bihs that hold them as items refitted, on the host builder (no
GPU).  This call is the specification the device path (glome_scene_instance_update, test_instance_update_gpu.py) is held against; here
it is held against its own definitions computed in NumPy, against a builder made fresh at the new pose, and against the fp64 oracle."""
import numpy as np
import pytest

import bihs_refit as BR
import instances_refit as IR
import parity
from helpers import HostSim, product_camera_lights
from glome_amd import _lib as L
from glome_amd import api

DELTA = 1e-4   # kDelta, Vec.hs:40
INF = 1e6      # kInfinity, Vec.hs:14
WITH_BIH = ["grove", "mixed", "mixed_nested"]


def dump(b, node):
    return [np.asarray(x).tolist() for x in b.bih_dump(node)]


def check_planes(b, T):
    """every branch's lsplit / rsplit equals, exactly, the builder's definition over glome_sb_bound of the items below it: the max (min)
    of the items' box hi (lo) on the node's axis from -(+)infinity, plus (minus) delta.  Returns the number of planes compared."""
    box = {}
    n = 0
    for k in T.branches():
        ax = int(T.axis[k])
        for side, items in ((0, T.items[T.left[k]]), (1, T.items[T.right[k]])):
            for i in items:
                if i not in box:
                    box[i] = b.bound(i)
            if side == 0:
                want = max([-INF] + [box[i][3 + ax] for i in items]) + DELTA
                assert T.ls[k] == want, (k, T.ls[k], want)
            else:
                want = min([INF] + [box[i][ax] for i in items]) - DELTA
                assert T.rs[k] == want, (k, T.rs[k], want)
            n += 1
    return n


def joined_bound(b, items):
    boxes = np.array([b.bound(i) for i in items])
    return np.concatenate([np.minimum(INF, boxes[:, :3].min(axis=0)), np.maximum(-INF, boxes[:, 3:].max(axis=0))])


@pytest.mark.parametrize("name", WITH_BIH + ["oak"])
def test_the_same_matrices_change_nothing(built, name):
    B = IR.build_oak() if name == "oak" else IR.build(name)
    before = dump(B.b, B.bih), B.b.show(B.root), B.b.bound(B.bih).tolist()
    B.b.instance_set_transforms(*IR.original_matrices(B))
    assert (dump(B.b, B.bih), B.b.show(B.root), B.b.bound(B.bih).tolist()) == before


@pytest.mark.parametrize("pose", IR.POSES)
@pytest.mark.parametrize("name", WITH_BIH + ["oak"])
def test_refit_planes_are_the_definitions_over_the_items_bounds(built, name, pose):
    B = IR.build_oak() if name == "oak" else IR.build(name)
    before = BR.Tree(B.b, B.bih)
    box0 = B.b.bound(B.bih).copy()
    t0 = BR.traits(B.b, B.root)
    n0 = check_planes(B.b, before)  # the planes of the tree as built are the same definitions
    B.b.instance_set_transforms(*IR.moved_matrices(B, pose))
    T = BR.Tree(B.b, B.bih)
    assert T.shape() == before.shape()
    assert check_planes(B.b, T) == n0 == 2 * len(T.branches())
    assert (np.asarray(T.ls) != np.asarray(before.ls)).any() and (np.asarray(T.rs) != np.asarray(before.rs)).any()
    assert np.array_equal(B.b.bound(B.bih), joined_bound(B.b, T.items[0]))
    span0, span = box0[3:] - box0[:3], B.b.bound(B.bih)[3:] - B.b.bound(B.bih)[:3]
    if name in ("grove", "oak"):  # every item moves: "grow" enlarges the root box, "shrink" shrinks it
        assert (span[[0, 2]] > span0[[0, 2]]).all() if pose == "grow" else (span[[0, 2]] < span0[[0, 2]]).all()
    assert BR.traits(B.b, B.root) == t0


def test_only_the_named_items_and_the_bihs_that_hold_them_change(built):
    B = IR.build("grove")
    T0 = BR.Tree(B.b, B.bih)
    sizes = [int(T0.nleaf[k]) for k in T0.leaves()]  # the grove has the leaves its case is about: the count escape, the empty leaf
    assert max(sizes) >= 7 and min(sizes) == 0 and len(B.ids) == 40 and len(T0.items[0]) == 40 and all(IR.is_instance(B.b, i) for i in B.ids)
    three = [2, 17, 33]
    ids, M = IR.moved_matrices(B, "grow", three)
    others = [i for k, i in enumerate(B.ids) if k not in three]
    before = {i: B.b.show(i) for i in others}
    B.b.instance_set_transforms(ids, M)
    assert {i: B.b.show(i) for i in others} == before
    T = BR.Tree(B.b, B.bih)
    check_planes(B.b, T)
    assert np.array_equal(B.b.bound(B.bih), joined_bound(B.b, T.items[0]))
    for i, m in zip(ids, M):
        assert np.array_equal(IR.xf_of(B.b, i), m)


@pytest.mark.parametrize("name", WITH_BIH)
def test_there_and_back_gives_the_original_text(built, name):
    B = IR.build(name)
    orig = B.b.show(B.root), dump(B.b, B.bih)
    back = IR.original_matrices(B)
    B.b.instance_set_transforms(*IR.moved_matrices(B, "grow"))
    assert B.b.show(B.root) != orig[0]
    B.b.instance_set_transforms(*back)
    assert (B.b.show(B.root), dump(B.b, B.bih)) == orig


def test_an_instance_outside_any_bih_is_a_matrix_and_nothing_else(built):
    for name in ("flat3", "shared", "subtrees"):
        B = IR.build(name)
        B.b.instance_set_transforms(*IR.moved_matrices(B, "grow"))
        F = IR.build(name, "grow")
        assert B.b.show(B.root) == F.b.show(F.root), name


def test_a_bih_that_holds_the_instance_deeper_keeps_its_planes(built):
    """the header's statement: only a bih that holds the Instance AS AN ITEM is refitted"""
    B = IR.build("mixed")
    outer = B.b.bih([B.bih, B.b.sphere((9.0, 1.0, 0.0), 0.5)])           # a bih above the refitted one
    deeper = B.b.bih([B.b.group([B.ids[0], B.b.sphere((0.0, 5.0, 0.0), 0.3)]), B.b.sphere((0.0, 9.0, 0.0), 0.5)])  # the Instance inside an item
    kept = dump(B.b, outer), B.b.bound(outer).tolist(), dump(B.b, deeper), B.b.bound(deeper).tolist()
    inner = dump(B.b, B.bih)
    B.b.instance_set_transforms(*IR.moved_matrices(B, "grow"))
    assert (dump(B.b, outer), B.b.bound(outer).tolist(), dump(B.b, deeper), B.b.bound(deeper).tolist()) == kept
    assert dump(B.b, B.bih) != inner


@pytest.mark.parametrize("name,pose", [("grove", "grow"), ("grove", "shrink"), ("mixed_nested", "grow")])
def test_refitted_builder_renders_what_a_fresh_build_renders(built, name, pose):
    """through the host build of the device headers: bit-equal frames when the fresh build picks the same tree; else both within the scene
    class's gate against the fp64 oracle of the scene at the pose"""
    B = IR.build(name)
    B.b.instance_set_transforms(*IR.moved_matrices(B, pose))
    F = IR.build(name, pose)
    cam, lights = product_camera_lights(F.sd)
    frames = []
    for X in (B, F):
        hs = HostSim(X.b, X.root)
        frames.append(hs.render(cam, lights, 96, 54, 2))
    if dump(B.b, B.bih) == dump(F.b, F.bih):
        assert np.array_equal(frames[0][0], frames[1][0], equal_nan=True)
    for img, cnt in frames:
        parity.check_image(img, [int(x) for x in cnt], F.sd, 96, 54, 2)
    hs = HostSim(F.b, F.root)  # (the rays' check maps primitive ids through the pose description's node map: the fresh builder's)
    parity.check_rays(lambda o, d: hs.rayint(o, d), lambda o, d, t: hs.shadow(o, d, t), hs.inside, F.sd, F.nm, n=6000)


@pytest.mark.parametrize("pose", IR.POSES)
def test_swayed_oak_against_the_oracle(built, pose):
    """the oak with every item turned about its own base: the refitted builder against the oracle of the oak written out at the pose"""
    B = IR.build_oak()
    E0 = IR.Built(IR.oak_explicit())
    # the written-out oak is scenes.oak's: same items in the same order, equal to rounding
    assert len(E0.ids) == len(B.ids) == 63
    for i, j in zip(B.ids, E0.ids):
        assert np.allclose(B.b.bound(i), E0.b.bound(j), rtol=0, atol=1e-12)
    B.b.instance_set_transforms(*IR.moved_matrices(B, pose))
    E = IR.Built(IR.oak_explicit(pose))
    for i, j in zip(B.ids, E.b.bih_items(E.bih)):
        assert np.allclose(B.b.bound(i), E.b.bound(j), rtol=0, atol=1e-9)
    cam, lights = product_camera_lights(E.sd)
    hs = HostSim(B.b, B.root)
    img, cnt = hs.render(cam, lights, 96, 54, 2)
    parity.check_image(img, [int(x) for x in cnt], E.sd, 96, 54, 2)
    # the rays, under parity.py's bounds, of the refitted builder and of the builder made fresh at the pose: the setup the GPU test of the
    # update uses is within the gate before any update is involved
    IR.check_oak_rays(lambda o, d: hs.rayint(o, d), lambda o, d, t: hs.shadow(o, d, t), E)
    hf = HostSim(E.b, E.root)
    IR.check_oak_rays(lambda o, d: hf.rayint(o, d), lambda o, d, t: hf.shadow(o, d, t), E)


def test_a_tree_read_from_a_show_text_is_handled(built):
    B = IR.build("grove")
    b2 = api.Builder()
    t2, _ = b2.load_show(B.b.show(B.bih), default_material=b2.material_surface((0.5, 0.5, 0.5), 1, 0.2, 0.8, 0, 0))
    items2 = [i for i in b2.bih_items(t2)]
    # the read tree's items in preorder are the built tree's leaf items in preorder; peel the wrappers to the Instances
    T = BR.Tree(B.b, B.bih)
    pre = [i for k in T.leaves() for i in T.items[k]]
    assert len(items2) == len(pre) == 40

    inst2 = [IR.peel(b2, i) for i in items2]
    inst1 = [IR.peel(B.b, i) for i in pre]
    assert sorted(inst1) == sorted(B.ids)
    order = {i: k for k, i in enumerate(B.ids)}
    ids, M = IR.moved_matrices(B, "grow")
    B.b.instance_set_transforms(ids, M)
    b2.instance_set_transforms(inst2, M[[order[i] for i in inst1]])
    assert b2.show(t2) == B.b.show(B.bih)


def test_refusals_leave_everything_untouched(built):
    B = IR.build("grove")
    b = B.b
    ids, M = IR.moved_matrices(B, "grow")
    orig = dump(b, B.bih), b.show(B.root)
    nan = M.copy(); nan[3, 7] = np.nan
    inf = M.copy(); inf[5, 20] = np.inf
    corrupt = M.copy(); corrupt[4, :12] *= 2.0   # forward * inverse is no identity: check_xfm, Vec.hs:466-477
    ball = b.sphere((0.0, 6.0, 0.0), 1.0)
    for args, status, msg in (((ids[:-1] + [ball], M), -1, rf"node {ball} is a Sphere, not an Instance"),
                              ((ids[:-1] + [B.bih], M), -1, rf"node {B.bih} is a Bih"),
                              ((ids[:-1] + [ids[0]], M), -1, rf"node {ids[0]} is named more than once"),
                              ((ids[:-1] + [10 ** 6], M), -1, r"no node 1000000"),
                              ((ids, nan), -1, rf"node {ids[3]} is not finite"),
                              ((ids, inf), -1, rf"node {ids[5]} is not finite"),
                              ((ids, corrupt), -2, rf"node {ids[4]}: corrupt matrix")):
        with pytest.raises(api.GlomeError, match=msg + rf".*status {status}"):
            b.instance_set_transforms(*args)
        assert (dump(b, B.bih), b.show(B.root)) == orig, msg
    with pytest.raises(api.GlomeError, match="ids but"):
        b.instance_set_transforms(ids, M[:-1])
    lib = L.load()
    i32, pi = L.ivec(ids)
    assert lib.glome_sb_instance_set_transforms(b.h, pi, None, len(ids)) == L.E_INVALID  # null arrays, which the Python wrapper cannot express
    assert lib.glome_sb_instance_set_transforms(b.h, None, M.ctypes.data_as(L.c_dp), len(ids)) == L.E_INVALID
    assert lib.glome_sb_instance_set_transforms(b.h, pi, M.ctypes.data_as(L.c_dp), -1) == L.E_INVALID
    assert (dump(b, B.bih), b.show(B.root)) == orig
    assert lib.glome_sb_instance_set_transforms(b.h, None, None, 0) == 0  # nothing named: nothing done
    assert (dump(b, B.bih), b.show(B.root)) == orig
    b.instance_set_transforms(ids, M)  # and the valid call still works
    assert b.show(B.root) != orig[1]


def test_scene_desc_records_the_call(built):
    """SceneDesc.instance_set_transforms replays into the builder in its place"""
    fx = IR.grove()
    B0 = IR.Built(fx)
    ids, M = IR.moved_matrices(B0, "shrink")
    back = {v: k for k, v in enumerate(B0.nm)}
    fx.sd.instance_set_transforms([back[i] for i in ids], M)
    B1 = IR.Built(fx)
    B0.b.instance_set_transforms(ids, M)
    assert B1.b.show(B1.root) == B0.b.show(B0.root)


def test_a_box_that_reaches_infinity_is_refused_as_the_constructor_refuses_it(built):
    b = api.Builder()
    pl, tree = IR.plane_bih(b)
    orig = dump(b, tree), b.show(tree)
    with pytest.raises(api.GlomeError, match=rf"bih {tree}: bih: infinite bounding box.*status -2"):
        b.instance_set_transforms([pl], api.translate((1e-4, 0, 0)).reshape(1, 24))
    assert (dump(b, tree), b.show(tree)) == orig
    b.instance_set_transforms([pl], api.translate((0.5, 0, 0)).reshape(1, 24))
    assert b.show(tree) != orig[1]
