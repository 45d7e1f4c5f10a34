"""glome_sb_bih_resplit: the tree built again in place, and glome_sb_bih_layout: what a commit lays out for it -- on the host builder (no
GPU).  The re-split is held against the constructor itself: after the call the node is the tree glome_sb_bih builds over the same items
in update order.  Fixtures and poses are bihs_refit's and spheres_refit's; SH and the growth and depth poses are bihs_resplit's."""
import numpy as np
import pytest

import bihs_refit as BR
import bihs_resplit as RS
import parity
import spheres_refit as SR
import tree_build_cases as TC
from helpers import HostSim, product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api


def dump(b, node):
    return [np.asarray(x).tolist() for x in b.bih_dump(node)]


def state(b, node):
    return dump(b, node), b.show(node), b.bound(node).tolist(), b.bih_items(node)


def tri_bih(P):
    b = api.Builder()
    return b, b.bih(b.triangles_bulk(P))


def assert_is_the_constructors_tree(b, node):
    """the node against a fresh glome_sb_bih over its items in update order: node for node, bit for bit, same box"""
    fresh = b.bih(b.bih_items(node))
    assert dump(b, node) == dump(b, fresh)
    assert b.show(node) == b.show(fresh)
    assert b.bound(node).tolist() == b.bound(fresh).tolist()
    return fresh


@pytest.mark.parametrize("which", ["V1", "V2", "SH"])
@pytest.mark.parametrize("name", ["three", "mixed", "s3_20", "wide"])
def test_resplit_gives_the_tree_the_constructor_builds(built, name, which):
    sd, b, nm, tree = BR.build(name)
    items = b.bih_items(tree)
    refitted_from = BR.Tree(b, tree).shape()
    b.bih_set_triangles(tree, RS.triangles(name, which))
    assert BR.Tree(b, tree).shape() == refitted_from  # (set_triangles keeps what the builder decided ...)
    b.bih_resplit(tree)
    assert_is_the_constructors_tree(b, tree)
    assert b.bih_items(tree) == items  # the update order is the same before and after
    if which == "SH" and name != "three":  # (... and the re-split decides again: the shuffled pose leaves no leaf list as it was)
        assert BR.Tree(b, tree).shape() != refitted_from
    # the scene above sees the new tree under the old id
    assert b.show(tree) in b.show(nm[sd.root])


def test_resplit_of_the_pose_it_was_built_for_changes_nothing(built):
    sd, b, nm, tree = BR.build("mixed")
    before = state(b, tree)
    b.bih_resplit(tree)
    assert state(b, tree) == before


@pytest.mark.parametrize("which", ["V1", "SH"])
def test_resplit_of_a_sphere_bih(built, which):
    B = SR.build("cloud")
    items = B.b.bih_items(B.tree)
    B.b.bih_set_spheres(B.tree, RS.spheres("cloud", which))
    B.b.bih_resplit(B.tree)
    assert_is_the_constructors_tree(B.b, B.tree)
    assert B.b.bih_items(B.tree) == items


def test_resplit_of_a_tree_read_from_show_text_keeps_its_preorder_update_order(built):
    sd, b, nm, tree = BR.build("mixed")
    b2 = api.Builder()
    t2, _ = b2.load_show(b.show(tree))
    items = b2.bih_items(t2)  # the leaf items in preorder: the read tree records no order of its own
    T2 = BR.Tree(b2, t2)
    assert items == [i for k in T2.leaves() for i in T2.items[k]]
    P = RS.triangles("mixed", "SH")
    b2.bih_set_triangles(t2, P)
    b2.bih_resplit(t2)
    # the preorder of the NEW tree is another one: the order was recorded before the tree went
    T2 = BR.Tree(b2, t2)
    assert [i for k in T2.leaves() for i in T2.items[k]] != items
    assert b2.bih_items(t2) == items
    assert_is_the_constructors_tree(b2, t2)
    # item k still means the same item: a second pose lands on the same triangles
    P1 = RS.triangles("mixed", "V1")
    b2.bih_set_triangles(t2, P1)
    fresh = b2.bih(b2.triangles_bulk(P1))
    b2.bih_refit(t2)
    assert np.array_equal(b2.bound(t2), b2.bound(fresh))


def test_any_bih_is_legal(built):
    """a bih of boxes, a sphere and an Instance: no update call serves it, the re-split does (and changes nothing: nothing moved)"""
    b = api.Builder()
    items = [b.box((float(i), 0.0, 0.0), (i + 0.5, 0.5 + 0.1 * i, 0.5)) for i in range(7)] + [b.sphere((3.0, 4.0, 0.0), 1.0)]
    items.append(b.transform(b.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), [api.translate((0.0, 5.0, 2.0))]))
    t = b.bih(items)
    before = state(b, t)
    b.bih_resplit(t)
    assert state(b, t) == before
    # ... and after an Instance of it has moved, it is the constructor's tree for the new place
    b.instance_set_transforms([items[-1]], [api.translate((9.0, -5.0, 2.0))])
    b.bih_resplit(t)
    assert_is_the_constructors_tree(b, t)
    assert state(b, t)[0] != before[0]


def test_refusals_leave_the_node_untouched(built):
    lib = L.load()
    # build_rec's fixed point (tree_build_cases bih_four_points): four points on a line, which no constructor accepts -- a tree read
    # from a text holds them
    assert TC.BY_NAME["bih_four_points"].refusal == TC.LOOP
    b = api.Builder()
    good = b.bih([b.sphere((float(i), 0.0, 0.0), 0.25) for i in range(4)])
    b2 = api.Builder()
    t2, _ = b2.load_show(b.show(good).replace("0.25", "0.0"))
    assert [b2.bound(i).tolist() for i in b2.bih_items(t2)] == [[float(i), 0.0, 0.0] * 2 for i in range(4)]
    with pytest.raises(api.GlomeError, match=TC.LOOP[1]):  # the constructor's own refusal of these items
        b2.bih(b2.bih_items(t2))
    before = state(b2, t2)
    with pytest.raises(api.GlomeError, match=TC.LOOP[1] + r".*status -2"):
        b2.bih_resplit(t2)
    assert state(b2, t2) == before
    # an infinite box: an item that is a plane, again through a text (glome_sb_bih refuses the list)
    b3 = api.Builder()
    t3 = b3.bih([b3.sphere((float(i), 0.0, 0.0), 0.25) for i in range(4)])
    text = b3.show(t3)
    b4 = api.Builder()
    plane = b4.show(b4.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    ball = "SI Sphere (Vec 3.0 0.0 0.0) 0.25 4.0"
    assert ball in text and plane.startswith("SI ")
    t4, _ = b4.load_show(text.replace(ball, plane))
    with pytest.raises(api.GlomeError, match=r"bih: infinite bounding box.*status -2"):
        b4.bih(b4.bih_items(t4))
    before = state(b4, t4)
    with pytest.raises(api.GlomeError, match=r"bih: infinite bounding box.*status -2"):
        b4.bih_resplit(t4)
    assert state(b4, t4) == before
    # not a Bih, and no such node
    sd, b5, nm, tree = BR.build("mixed")
    before = state(b5, tree)
    for node, what in ((nm[sd.root], "Tex"), (nm[0], "Triangle")):
        with pytest.raises(api.GlomeError, match=rf"is a {what}, not a Bih.*status -1"):
            b5.bih_resplit(node)
        with pytest.raises(api.GlomeError, match=rf"is a {what}, not a Bih.*status -1"):
            b5.bih_layout(node)
    assert lib.glome_sb_bih_resplit(b5.h, 10 ** 6) == L.E_INVALID and lib.glome_sb_bih_layout(b5.h, 10 ** 6, None) == L.E_INVALID
    assert state(b5, tree) == before
    # a bih that is not a leaf bih has no layout of this kind
    mixed_items = b5.bih([nm[0], nm[1], b5.sphere((0.0, 9.0, 0.0), 1.0), nm[2]])
    with pytest.raises(api.GlomeError, match=r"not a leaf bih.*status -1"):
        b5.bih_layout(mixed_items)


def layout_from_the_dump(b, node):
    """what the layout must say, counted from the tree itself: a record per leaf item, a pair record per two triangles of a leaf, the
    deepest node's level; and the least the slots can be -- a slot per branch and per leaf of 7 or more items (treelet padding adds)"""
    T = BR.Tree(b, node)
    leaves = [T.nleaf[k] for k in T.leaves()]
    return {"records": sum(leaves), "pairs": sum((c + 1) // 2 for c in leaves), "depth": max(T.depth) + 1,
            "min_slots": len(T.branches()) + sum(1 for c in leaves if c > 6)}


@pytest.mark.parametrize("name", ["three", "mixed", "s3_20"])
def test_layout_is_what_a_commit_of_the_lone_tree_lays_out(built, name):
    sd, b, nm, tree = BR.build(name, wrap="root")
    lay = b.bih_layout(tree)
    want = layout_from_the_dump(b, tree)
    assert (lay["records"], lay["pairs"], lay["depth"]) == (want["records"], want["pairs"], want["depth"])
    assert want["min_slots"] <= lay["slots"] <= 4 * want["min_slots"]  # (a treelet holds a node at least and skips three slots at most)
    tr = BR.traits(b, tree)
    assert tr[7] == max(lay["slots"], 1)  # n_bih_nodes: the lone tree's slots (a tree of no slot keeps the pool's one padding entry)
    info = HostSim(b, tree).info()
    assert info["max_bih_depth"] == lay["depth"] and info["n_recs"] == lay["records"] + 2  # (its items' records, the bih's and the root's)
    # the same counts under wrappers and beside other trees: only the bases differ
    sd2, b2, nm2, tree2 = BR.build(name, wrap="instances")
    assert b2.bih_layout(tree2) == lay


def test_layout_of_a_sphere_bih_has_no_pair_records(built):
    B = SR.build("cluster", wrap="root")
    lay = B.b.bih_layout(B.tree)
    want = layout_from_the_dump(B.b, B.tree)
    assert (lay["records"], lay["pairs"], lay["depth"]) == (want["records"], 0, want["depth"]) and lay["slots"] >= want["min_slots"]
    assert BR.traits(B.b, B.tree)[7] == max(lay["slots"], 1)


def test_growth_and_shrink(built):
    """one item list, two poses: piled (A) the builder cannot split, apart (B) it splits to leaves of one to three -- B needs more node
    slots AND more pair records than A, so A -> B outgrows what a commit of A laid out, and B -> A fits into what B's did"""
    A, Bp = RS.pose_piled(), RS.pose_apart()
    b, t = tri_bih(A)
    la = b.bih_layout(t)
    b.bih_set_triangles(t, Bp)
    assert b.bih_layout(t) == la  # a refit lays out what was there
    b.bih_resplit(t)
    lb = b.bih_layout(t)
    assert lb["slots"] > la["slots"] and lb["pairs"] > la["pairs"], (la, lb)
    assert lb["records"] == la["records"] == RS.GROW_N
    bf, tf = tri_bih(Bp)
    assert bf.bih_layout(tf) == lb
    b.bih_set_triangles(t, A)
    b.bih_resplit(t)
    assert b.bih_layout(t) == la  # and back


def test_a_resplit_may_be_deeper_than_anything_the_first_pose_needed(built):
    comb, flat = RS.comb_and_flat()
    b, t = tri_bih(flat)
    stack_cap = BR.traits(b, t)[6]
    assert b.bih_layout(t)["depth"] <= stack_cap
    b.bih_set_triangles(t, comb)
    assert b.bih_layout(t)["depth"] <= stack_cap  # (refitted: as shallow as it was)
    b.bih_resplit(t)
    depth = b.bih_layout(t)["depth"]
    assert depth > stack_cap, (depth, stack_cap)
    tr = BR.traits(b, t)
    assert tr[6] + tr[8] >= depth - 1 and tr[8] > 0  # the commit's stack: LDS entries, and now overflow entries beyond them
    assert_is_the_constructors_tree(b, t)


@pytest.mark.parametrize("name", ["mixed", "s3_20"])
def test_a_shuffled_pose_costs_more_refitted_than_resplit(built, name):
    """SH on random rays: the refitted tree and the re-split tree answer alike, and the refitted one visits strictly more nodes and tests
    strictly more triangles.  The counters are those of the product's own traversal compiled for the host (tests/hostsim, its faithful
    walk): the fp64 oracle builds every bih itself and so cannot hold a refitted tree; it is held against the re-split scene below."""
    sd, b, nm, tree = BR.build(name, wrap="root")
    b.bih_set_triangles(tree, RS.triangles(name, "SH"))
    o, d = random_rays(4000, 5)
    refit = HostSim(b, tree).rayint(o, d, analysis=1)
    b.bih_resplit(tree)
    split = HostSim(b, tree).rayint(o, d, analysis=1)
    assert (refit["t"] >= 0).mean() > 0.3
    assert np.array_equal(refit["t"], split["t"]) and np.array_equal(refit["prim"], split["prim"])
    nodes_r, _, prims_r = (int(x) for x in refit["counters"])
    nodes_s, _, prims_s = (int(x) for x in split["counters"])
    print(f"{name} SH: refitted {nodes_r} nodes {prims_r} triangle tests, re-split {nodes_s} nodes {prims_s} triangle tests")
    assert nodes_r > nodes_s and prims_r > prims_s, "the pose does not degrade the tree: it is the wrong pose"


def test_resplit_builder_against_the_oracle(built):
    """the spec sequence's scene through the host-compiled device code, against the fp64 oracle loaded with a description made from the
    shuffled triangles (which builds the same tree from them)"""
    sd0, b, nm, tree = BR.build("mixed")
    P = RS.triangles("mixed", "SH")
    b.bih_set_triangles(tree, P)
    b.bih_resplit(tree)
    sd = BR.SceneDesc(round32=False)
    mat = BR.scenes.matte(sd, (0.8, 0.5, 0.4))
    sd.set_root(sd.tex(sd.bih(sd.triangles_bulk(P)), mat))  # (the op list of bihs_refit.scene_desc(.., wrap="tex"): nm maps its ids too)
    for pos, col in BR.scenes.LIGHTS[:2]:
        sd.add_light(pos, col)
    sd.set_camera(*BR.MR.camera_for("V1"))
    hs = HostSim(b, nm[sd.root])
    parity.check_rays(lambda o, d: hs.rayint(o, d), lambda o, d, t: hs.shadow(o, d, t), hs.inside, sd, nm, n=4000)
    cam, lights = product_camera_lights(sd)
    img, cnt = hs.render(cam, lights, 96, 54, 2)
    parity.check_image(img, [int(x) for x in cnt], sd, 96, 54, 2)
