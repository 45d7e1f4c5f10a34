"""glome_sb_bih_refit and glome_sb_bihs_above: objects that lie under a bih move, and the bihs above them are refitted inner trees first,
on the host builder (no GPU).  The sequence -- mesh_set_vertices / bih_set_triangles / instance_set_transforms, then bih_refit of every
bih above -- is the specification the device path (glome_scene_bih_refit, test_nested_update_gpu.py) is held against; here it is held
against its own definitions computed in NumPy, against a builder made fresh at the new pose, and against the fp64 oracle."""
import numpy as np
import pytest

import bihs_refit as BR
import instances_refit as IR
import nested_refit as NR
import parity
from helpers import HostSim, product_camera_lights
from glome_amd import _lib as L
from glome_amd import api
from test_instance_refit_host import check_planes, dump, joined_bound


def refitted(B):
    """the builder ids of every bih of the fixture that a move of its movables refits"""
    return sorted(set(B.bihs.values()))


def state(B):
    return {t: (dump(B.b, t), B.b.bound(t).tolist()) for t in refitted(B)}


@pytest.mark.parametrize("name", NR.ALL)
def test_bihs_above_names_the_trees_in_an_order_they_can_be_refitted_in(built, name):
    B = NR.get(name)
    for k, (kind, node, _) in enumerate(B.movable):
        got = B.b.bihs_above(B.root, node)
        assert sorted(got) == sorted(B.above[k]), (name, k, got)
        if name in ("chain", "oak_in_scene"):
            assert got == B.above[k]  # the inner tree before the root
    # a bih as an object: the trees above IT
    if "inner" in B.bihs:
        assert B.b.bihs_above(B.root, B.bihs["inner"]) == [B.bihs["root"]]
    assert B.b.bihs_above(B.root, B.bihs.get("root", B.bihs.get("o1"))) == []


def test_bihs_above_of_objects_with_no_bih_above_is_empty(built):
    for fx in (IR.build("subtrees"), IR.build("flat3")):
        for i in fx.ids:
            assert fx.b.bihs_above(fx.root, i) == []
    B = IR.build("grove")  # Instances that are items of a bih below a group: that bih, and nothing above it
    assert B.b.bihs_above(B.root, B.ids[0]) == [B.bih] and B.b.bihs_above(B.root, B.bih) == []
    with pytest.raises(api.GlomeError, match=r"is not a Mesh, a triangle bih, an Instance or a refittable bih.*status -1"):
        B.b.bihs_above(B.root, B.b.sphere((0, 0, 0), 1.0))


@pytest.mark.parametrize("shape", sorted(NR.REFUSED))
def test_refused_shapes_name_the_node_in_the_way(built, shape):
    b = api.Builder()
    root, node, msg = NR.REFUSED[shape](b)
    with pytest.raises(api.GlomeError, match=msg + r".*status -1"):
        b.bihs_above(root, node)


def test_an_instance_that_is_an_item_twice_and_a_triangle_outside_its_bih_are_refused(built):
    b = api.Builder()
    x = b.transform(b.sphere((0.0, 0.0, 0.0), 0.4), [api.translate((0.5, 1.0, 0.0))])
    t1 = b.bih([x, b.sphere((3.0, 1.0, 0.0), 0.5), b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 3.0), 0.5)])
    t2 = b.bih([x, b.sphere((6.0, 1.0, 0.0), 0.5), b.sphere((-6.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 6.0), 0.5)])
    with pytest.raises(api.GlomeError, match=rf"instance {x} is an item of a bih more than once"):
        b.bihs_above(b.group([t1, t2]), x)
    tris = b.triangles_bulk(NR.tris9())
    t = b.bih(tris)
    outer = b.bih([t, b.sphere((3.0, 1.0, -3.0), 0.5), b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 3.0), 0.5)])
    with pytest.raises(api.GlomeError, match=rf"triangle {tris[4]} of bih {t} is also part of the scene outside that bih"):
        b.bihs_above(b.group([outer, tris[4]]), t)


@pytest.mark.parametrize("pose", NR.POSES)
@pytest.mark.parametrize("name", NR.ALL)
def test_refit_planes_are_the_definitions_over_the_items_bounds(built, name, pose):
    B = NR.get(name)
    trees = refitted(B)
    before = {t: BR.Tree(B.b, t) for t in trees}
    s0 = state(B)
    t0 = BR.traits(B.b, B.root)
    n0 = {t: check_planes(B.b, before[t]) for t in trees}  # the planes of the trees as built are the same definitions
    NR.host_sequence(B, NR.moves(B, pose))
    for t in trees:
        T = BR.Tree(B.b, t)
        assert T.shape() == before[t].shape()
        assert check_planes(B.b, T) == n0[t] == 2 * len(T.branches())
        assert np.array_equal(B.b.bound(t), joined_bound(B.b, T.items[0]))
    s1 = state(B)
    assert all(s1[t] != s0[t] for t in trees), "every refitted tree's planes or box move with the pose"
    assert BR.traits(B.b, B.root) == t0


def test_an_empty_tree_and_a_tree_of_one_leaf(built):
    b = api.Builder()
    tri = b.bih(b.triangles_bulk(NR.tris9()[:2]))
    leaf = b.bih([tri, b.sphere((0.0, 1.0, 0.0), 0.5)])  # two items: one leaf, no branch
    assert BR.Tree(b, leaf).n == 1
    b.bih_set_triangles(tri, NR.pose_points(NR.tris9()[:2].reshape(-1, 3), "grow").reshape(-1, 9))
    assert b.bihs_above(leaf, tri) == [leaf]
    old = b.bound(leaf).copy()
    b.bih_refit(leaf)
    assert np.array_equal(b.bound(leaf), joined_bound(b, b.bih_items(leaf))) and not np.array_equal(b.bound(leaf), old)
    void = b.bih([])  # bih [] = Void
    with pytest.raises(api.GlomeError, match=rf"bih_refit: node {void} is a Void, not a Bih.*status -1"):
        b.bih_refit(void)
    with pytest.raises(api.GlomeError, match=r"is a Sphere, not a Bih.*status -1"):
        b.bih_refit(b.sphere((0, 0, 0), 1.0))


@pytest.mark.parametrize("name", sorted(NR.FIXTURES))
def test_everything_not_above_the_moved_object_is_unchanged(built, name):
    B = NR.build(name)
    calls = NR.moves(B, "grow", [0])
    moved_ids = set(calls[0][1]) if calls[0][0] == "inst" else {calls[0][1]}
    above = set(B.b.bihs_above(B.root, NR.node_of(calls[0])))

    def depends(i):  # does node i's text hold a moved object or a refitted tree?  (ids below it: the builder makes a node after its children)
        return i in moved_ids or i in above
    texts = {i: B.b.show(i) for i in B.nm if not depends(i)}
    moved_text = {i: B.b.show(i) for i in moved_ids}
    NR.host_sequence(B, calls)
    changed = [i for i in texts if B.b.show(i) != texts[i]]
    # whatever changed holds a moved object (its text contains the moved object's NEW text) or is part of one (a moved bih's triangle)
    core = lambda i: B.b.show(i).removeprefix("SI ")
    for i in changed:
        assert any(core(m) in core(i) or core(i) in core(m) for m in moved_ids), (name, i)
    assert all(B.b.show(m) != moved_text[m] for m in moved_ids)
    others = [k for k in range(len(B.movable)) if k != 0 and B.movable[k][0] != "inst"]
    for k in others:  # the other movables keep their text
        assert B.b.show(B.movable[k][1]) == texts[B.movable[k][1]]


# how many of a fixture's refitted trees the builder, given the scene at the pose, splits as it split the scene as built: those are compared
# plane by plane.  Pinned, so that a fixture that drifts cannot leave the comparison empty without this test saying so.  (What does not
# depend on the split -- every tree's box and every item's bound -- is compared for every tree.)
ALIKE = {("chain", "grow"): 1, ("chain", "shrink"): 2, ("mesh_shared", "grow"): 0, ("mesh_shared", "shrink"): 0, ("nff_like", "grow"): 1,
         ("nff_like", "shrink"): 0, ("two_parents", "grow"): 1, ("two_parents", "shrink"): 2}


@pytest.mark.parametrize("pose", NR.POSES)
@pytest.mark.parametrize("name", sorted(NR.FIXTURES))
def test_refitted_builder_equals_a_fresh_build_where_the_trees_agree(built, name, pose):
    B = NR.build(name)
    NR.host_sequence(B, NR.moves(B, pose))
    F = NR.build(name, pose)
    same = 0
    for key in B.bihs:
        tb, tf = B.bihs[key], F.bihs[key]
        # whatever the split: the tree's box is the join of its items' bounds, and item k of one is item k of the other
        assert np.array_equal(B.b.bound(tb), F.b.bound(tf)), (name, key)
        ib, jf = B.b.bih_items(tb), F.b.bih_items(tf)
        assert len(ib) == len(jf) and all(np.array_equal(B.b.bound(i), F.b.bound(j)) for i, j in zip(ib, jf)), (name, key)
        a, f = BR.Tree(B.b, tb), BR.Tree(F.b, tf)
        if [len(x) for x in a.shape()[2]] != [len(x) for x in f.shape()[2]] or list(a.axis) != list(f.axis):
            continue  # the fresh build split this tree differently: no node to compare with a node
        same += 1
        assert np.array_equal(a.ls, f.ls) and np.array_equal(a.rs, f.rs), (name, key)
    assert same == ALIKE[(name, pose)], (name, pose, same)
    if same == len(B.bihs) and not F.fx.inserted:
        assert B.b.show(B.root) == F.b.show(F.root)


@pytest.mark.parametrize("name", NR.ALL)
def test_a_refit_with_nothing_moved_changes_nothing(built, name):
    B = NR.get(name)
    before = state(B), B.b.show(B.root)
    for k in range(len(B.movable)):
        for t in B.b.bihs_above(B.root, B.movable[k][1]):
            B.b.bih_refit(t)
        if name == "oak_in_scene" and k >= 2:
            break
    assert (state(B), B.b.show(B.root)) == before


@pytest.mark.parametrize("name", ["chain", "oak_in_scene"])
def test_the_outer_tree_before_the_inner_does_not_match_the_definitions(built, name):
    """the order matters: the root refitted while the inner tree still has its old box keeps planes that are not the definitions"""
    B = NR.get(name)
    inner, root = B.bihs["inner"], B.bihs["root"]
    ids = [node for kind, node, _ in B.movable]
    M = np.stack([api.compose([IR.xf_of(B.b, node), IR.sway(base, k, "grow")]) for k, (_, node, base) in enumerate(B.movable)])
    B.b.instance_set_transforms(ids, M)   # refits `inner`, the tree that holds them, as the call always has; the root keeps its planes
    stale = BR.Tree(B.b, root)
    try:
        check_planes(B.b, stale)
        planes_match = True
    except AssertionError:
        planes_match = False
    assert not (planes_match and np.array_equal(B.b.bound(root), joined_bound(B.b, stale.items[0]))), "the root is stale until it is refitted"
    B.b.bih_refit(root)
    T = BR.Tree(B.b, root)
    check_planes(B.b, T)
    assert np.array_equal(B.b.bound(root), joined_bound(B.b, T.items[0]))


def test_the_order_matters_for_two_trees_above_a_triangle_bih(built):
    """nff_like with one more level: root -> middle -> triangle bih; the root refitted before the middle is NOT the definitions"""
    b = api.Builder()
    t = b.bih(b.triangles_bulk(NR.tris9()))
    mid = b.bih([t, b.sphere((2.0, 1.0, -1.0), 0.5), b.sphere((4.0, 2.0, 2.0), 0.4), b.sphere((2.0, 3.0, 3.0), 0.3)])
    root = b.bih([mid, b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, -4.0), 0.5), b.sphere((0.0, 5.0, 0.0), 0.5)])
    assert b.bihs_above(root, t) == [mid, root]
    b.bih_set_triangles(t, NR.pose_points(NR.tris9().reshape(-1, 3), "grow").reshape(-1, 9))
    b.bih_refit(root)   # too early: `mid` still has its old box
    b.bih_refit(mid)
    assert not np.array_equal(b.bound(root), joined_bound(b, b.bih_items(root)))
    b.bih_refit(root)
    assert np.array_equal(b.bound(root), joined_bound(b, b.bih_items(root)))
    check_planes(b, BR.Tree(b, root))


def test_a_joined_box_that_reaches_infinity_is_refused_as_the_constructor_refuses_it(built):
    b = api.Builder()
    pts = NR.tris9()
    t = b.bih(b.triangles_bulk(pts))
    root = b.bih([t, b.sphere((3.0, 1.0, -2.0), 0.5), b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 3.0), 0.5)])
    far = pts.copy(); far[0, 0] = 1e6 - 1e-4   # its padded box reaches +1e6 exactly
    b.bih_set_triangles(t, far)
    assert b.bound(t)[3] == 1e6
    orig = dump(b, root), b.bound(root).tolist()
    with pytest.raises(api.GlomeError, match=rf"bih_refit: bih {root}: bih: infinite bounding box.*status -2"):
        b.bih_refit(root)
    assert (dump(b, root), b.bound(root).tolist()) == orig
    b.bih_set_triangles(t, pts)
    b.bih_refit(root)
    assert (dump(b, root), b.bound(root).tolist()) == orig


@pytest.mark.parametrize("name,pose", [("nff_like", "grow"), ("mesh_shared", "shrink"), ("two_parents", "grow"), ("chain", "grow")])
def test_refitted_builder_against_the_oracle(built, name, pose):
    """the refitted builder's scene through the host build of the device headers, within parity.py's bounds of the fp64 oracle of the
    scene built fresh at the pose"""
    B = NR.build(name)
    NR.host_sequence(B, NR.moves(B, pose))
    F = NR.build(name, pose)
    cam, lights = product_camera_lights(F.sd)
    hs = HostSim(B.b, B.root)
    img, cnt = hs.render(cam, lights, 96, 54, 2)
    parity.check_image(img, [int(x) for x in cnt], F.sd, 96, 54, 2)
    parity.check_rays(lambda o, d: hs.rayint(o, d), lambda o, d, t: hs.shadow(o, d, t), hs.inside, F.sd, IR.node_map_at_pose(B, F), n=6000)


def test_the_symbols_are_bound(built):
    lib = L.load()
    for name in ("glome_sb_bih_refit", "glome_sb_bihs_above", "glome_scene_nested_updates", "glome_scene_bih_refit", "glome_scene_bih_refit_dev", "glome_scene_bihs_above",
                 "glome_scene_stale_bihs"):
        assert hasattr(lib, name)
