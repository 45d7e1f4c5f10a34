"""glome_sb_bih_set_spheres: same tree, new centres and radii, on the host builder (no GPU).  This call is the specification the device
path (glome_scene_sphere_bih_update, test_sphere_bih_update_gpu.py) is held against; here it is held against NumPy and the fp64 oracle."""
import numpy as np
import pytest

import parity
import spheres_refit as SR
from helpers import HostSim, product_camera_lights
from glome_amd import _lib as L
from glome_amd import api

DELTA = 1e-4   # kDelta, Vec.hs:40
INF = 1e6      # kInfinity, Vec.hs:14


def dump(b, node):
    return [np.asarray(x).tolist() for x in b.bih_dump(node)]


def check_planes(T, lo, hi):
    """every branch's lsplit / rsplit equals, exactly, the builder's definition over the items below it, in float64: the max (min) of the
    items' box hi (lo) on the node's axis plus (minus) delta; lo / hi: item id -> its box.  The side of an empty subtree is not compared
    (the flattener overrides it).  Returns the number of planes compared."""
    n = 0
    for k in T.branches():
        ax = T.axis[k]
        below_l, below_r = T.items[T.left[k]], T.items[T.right[k]]
        if below_l:
            want = max(-INF, max(hi[i][ax] for i in below_l)) + DELTA
            assert T.ls[k] == want, (k, T.ls[k], want)
            n += 1
        if below_r:
            want = min(INF, min(lo[i][ax] for i in below_r)) - DELTA
            assert T.rs[k] == want, (k, T.rs[k], want)
            n += 1
    return n


def sphere_boxes(items, S):
    """a Sphere's box is c - r / c + r, no pad (Sphere.hs:78-81)"""
    return {it: S[k, :3] - S[k, 3] for k, it in enumerate(items)}, {it: S[k, :3] + S[k, 3] for k, it in enumerate(items)}


def bound_of(S):
    return np.concatenate([(S[:, :3] - S[:, 3:]).min(axis=0), (S[:, :3] + S[:, 3:]).max(axis=0)])


@pytest.mark.parametrize("wrap", SR.WRAPS)
@pytest.mark.parametrize("name", ["three", "cluster", "cloud"])
def test_fixtures_are_what_they_are_described_as(built, name, wrap):
    B = SR.build(name, "V0", wrap)
    SR.check_fixture(name, wrap, B)
    items = B.b.bih_items(B.tree)
    assert len(items) == len(B.balls) == len(SR.BIHS[name]())  # update order = the order `bih` was given: sphere k under item k
    S1 = SR.spheres(name, "V1")
    assert (S1[:, 3] > 0).all() and S1[0, 0] - S1[0, 3] == 0.0 and np.float64(np.float32(S1[1, 1])) != S1[1, 1]


def test_the_wide_fixture_is_the_smallest_of_its_kind(built):
    B = SR.build("wide")
    SR.check_fixture("wide", "tex", B)
    B1 = SR.build_lattice(SR.WIDE_N - 1)
    assert max(SR.Tree(B1.b, B1.tree).level_widths()) <= SR.MERGE_BLOCK


@pytest.mark.parametrize("name,wrap,which", [(n, "tex", w) for n in ("three", "cluster", "cloud") for w in ("V1", "V2")] + [("cluster", wrap, "V1") for wrap in ("root", "instances", "bound")]
                         + [("wide", "tex", "V1")])
def test_the_refitted_fixtures_show_their_spheres_to_rays_and_pixels(built, name, wrap, which):
    """what test_sphere_bih_update_gpu.py asserts of its comparisons, checked here on the host-compiled device code: at least 20 of the
    tests' rays and 20 pixels of the tests' frame meet a sphere of the bih"""
    B = SR.build(name, "V0", wrap)
    B.b.bih_set_spheres(B.tree, SR.spheres(name, which))
    rays, pixels = SR.sees_spheres(HostSim(B.b, B.root), B, which, api.camera(*SR.MR.camera_for(which)), 131, 66)
    assert rays >= 20 and pixels >= 20, (rays, pixels)


@pytest.mark.parametrize("name", ["three", "cluster", "cloud"])
def test_same_spheres_change_nothing(built, name):
    B = SR.build(name)
    before = dump(B.b, B.tree), B.b.show(B.tree), B.b.bound(B.tree).tolist()
    B.b.bih_set_spheres(B.tree, SR.spheres(name, "V0"))
    assert (dump(B.b, B.tree), B.b.show(B.tree), B.b.bound(B.tree).tolist()) == before


@pytest.mark.parametrize("which", ["V1", "V2"])
@pytest.mark.parametrize("name", ["cluster", "cloud"])
def test_refit_planes_are_the_definitions_over_the_new_spheres(built, name, which):
    B = SR.build(name)
    b, tree = B.b, B.tree
    before = SR.Tree(b, tree)
    t0 = SR.traits(b, B.root)
    S = SR.spheres(name, which)
    b.bih_set_spheres(tree, S)
    T = SR.Tree(b, tree)
    assert T.shape() == before.shape()
    n = check_planes(T, *sphere_boxes(b.bih_items(tree), S))
    assert n >= len(T.branches())
    assert np.array_equal(b.bound(tree), bound_of(S))
    assert SR.traits(b, B.root) == t0
    # the planes of the tree as built are the same definitions over the spheres it was built from
    assert check_planes(before, *sphere_boxes(b.bih_items(tree), SR.spheres(name, "V0"))) == n
    # and the Sphere nodes themselves moved: a later commit, `show` and `bound` see them
    assert np.array_equal(np.array([b.bound(s) for s in B.balls]), np.concatenate([S[:, :3] - S[:, 3:], S[:, :3] + S[:, 3:]], axis=1))


def test_a_tree_read_from_show_text_is_updated_in_preorder(built):
    B = SR.build("cluster", wrap="root")
    b, tree = B.b, B.tree
    b2 = api.Builder()
    t2, _ = b2.load_show(b.show(tree), default_material=b2.material_surface((0.8, 0.5, 0.4), 1, 0.2, 1, 0, 0))  # (every item is a `Tex`: the text carries no material)
    items = b2.bih_items(t2)
    T2 = SR.Tree(b2, t2)
    assert items == [i for k in T2.leaves() for i in T2.items[k]]
    # item k of the read tree is the sphere the first builder calls by its k-th preorder id
    order = {it: k for k, it in enumerate(b.bih_items(tree))}
    T = SR.Tree(b, tree)
    perm = [order[i] for k in T.leaves() for i in T.items[k]]
    assert perm != sorted(perm)
    S = SR.spheres("cluster", "V1")
    b.bih_set_spheres(tree, S)
    b2.bih_set_spheres(t2, S[perm])
    assert b2.show(t2) == b.show(tree)


def test_there_and_back_gives_the_original_text(built):
    B = SR.build("cluster")
    orig = B.b.show(B.tree)
    B.b.bih_set_spheres(B.tree, SR.spheres("cluster", "V1"))
    assert B.b.show(B.tree) != orig
    B.b.bih_set_spheres(B.tree, SR.spheres("cluster", "V0"))
    assert B.b.show(B.tree) == orig


@pytest.mark.parametrize("which", ["V1"])
def test_refitted_builder_against_the_oracle(built, which):
    """the refitted bih through the host-compiled device code, against the fp64 oracle loaded with a description made from the new spheres
    (parity.check_rays aims its rays at the origin's neighbourhood: V1's, not the far-away V2's)"""
    B = SR.build("cloud")
    B.b.bih_set_spheres(B.tree, SR.spheres("cloud", which))
    sd, _, _ = SR.scene_desc("cloud", which)  # (same op list as B.sd: B.nm maps its ids too)
    hs = HostSim(B.b, B.root)
    parity.check_rays(lambda o, d: hs.rayint(o, d), lambda o, d, t: hs.shadow(o, d, t), hs.inside, sd, B.nm, n=6000)
    cam, lights = product_camera_lights(sd)
    img, cnt = hs.render(cam, lights, 96, 54, 2)
    parity.check_image(img, [int(x) for x in cnt], sd, 96, 54, 2)


def test_refusals_leave_the_tree_untouched(built):
    B = SR.build("cluster")
    b, tree = B.b, B.tree
    S = SR.spheres("cluster", "V1")
    orig = dump(b, tree), b.show(tree)

    def variant(row, col, value):
        X = S.copy(); X[row, col] = value
        return X
    for args, what, msg in (((tree, S[:-1]), "too few", r"has 40 items, not 39"), ((tree, np.concatenate([S, S[:1]])), "too many", r"has 40 items, not 41"),
                            ((tree, variant(17, 1, np.nan)), "a NaN", r"a value is not finite"), ((tree, variant(3, 0, np.inf)), "an infinity", r"a value is not finite"),
                            ((tree, variant(5, 3, -np.inf)), "an infinite radius", r"a value is not finite"),
                            ((tree, variant(11, 3, 0.0)), "radius 0", r"radius of item 11 is not positive"), ((tree, variant(39, 3, -0.5)), "a negative radius", r"radius of item 39 is not positive"),
                            ((B.root, S), "a group", r"is a List, not a Bih"), ((B.balls[0], S), "a sphere", r"is a Sphere, not a Bih"), ((10 ** 6, S), "no such node", r"")):
        with pytest.raises(api.GlomeError, match=msg + r".*status -1"):
            b.bih_set_spheres(*args)
        assert (dump(b, tree), b.show(tree)) == orig, what
    lib = L.load()
    assert lib.glome_sb_bih_set_spheres(b.h, tree, None, len(S)) == L.E_INVALID  # a null array, which the Python wrapper cannot express
    assert b"null" in lib.glome_sb_last_error(b.h) and (dump(b, tree), b.show(tree)) == orig
    # an item that is not a plain sphere is named; the same Sphere node twice among the items
    tri = b.triangle((0.0, 5.0, 0.0), (1.0, 5.0, 0.0), (0.0, 6.0, 0.5))
    with_tri = b.bih(B.balls[:2] + [tri] + B.balls[2:5])
    twice = b.bih(B.balls[:5] + [b.tex(B.balls[1], 0)])
    for node, rows, msg in ((with_tri, 6, rf"item 2 \(node {tri}\) is a Triangle, not a plain Sphere"), (twice, 6, rf"sphere {B.balls[1]} is an item of the bih more than once")):
        before = dump(b, node), b.show(node)
        with pytest.raises(api.GlomeError, match=msg + r".*status -1"):
            b.bih_set_spheres(node, S[:rows])
        assert (dump(b, node), b.show(node)) == before
    assert (dump(b, tree), b.show(tree)) == orig
    b.bih_set_spheres(tree, S)  # and the valid call still works
    assert b.show(tree) != orig[1]


@pytest.mark.parametrize("how", ["direct", "instanced"])
def test_bihs_above_a_sphere_bih_and_the_nested_refit_on_the_host(built, how):
    """bihs_above gives the chain for a sphere bih under two bihs; bih_set_spheres, then bih_refit of each tree above, inner first, leaves
    every tree with the planes its definitions give over its items' new bounds, and with the box a fresh build of the moved scene has"""
    B = SR.build_nested("cluster", "V0", how)
    b = B.b
    assert b.bihs_above(B.root, B.tree) == [B.mid, B.top]
    with pytest.raises(api.GlomeError, match=r"is not a Mesh, a triangle bih, an Instance or a refittable bih.*status -1"):
        b.bihs_above(B.root, B.balls[0])
    shapes = [SR.Tree(b, t).shape() for t in (B.tree, B.mid, B.top)]
    S = SR.spheres("cluster", "V1")
    b.bih_set_spheres(B.tree, S)
    stale = SR.Tree(b, B.mid)
    for t in b.bihs_above(B.root, B.tree):
        b.bih_refit(t)
    assert [SR.Tree(b, t).shape() for t in (B.tree, B.mid, B.top)] == shapes
    moved = 0
    for t in (B.mid, B.top):
        T = SR.Tree(b, t)
        boxes = {i: b.bound(i) for i in b.bih_items(t)}
        assert check_planes(T, {i: x[:3] for i, x in boxes.items()}, {i: x[3:] for i, x in boxes.items()}) >= len(T.branches())
        if t == B.mid:
            moved = int(np.sum(np.asarray(T.ls) != np.asarray(stale.ls)) + np.sum(np.asarray(T.rs) != np.asarray(stale.rs)))
    assert moved > 0, "the refit of mid must have had something to do"
    fresh = SR.build_nested("cluster", "V1", how)
    for mine, theirs in ((B.tree, fresh.tree), (B.mid, fresh.mid), (B.top, fresh.top)):
        assert np.array_equal(b.bound(mine), fresh.b.bound(theirs))
    if how == "direct":
        assert np.array_equal(b.bound(B.tree), bound_of(S))
    rays, pixels = SR.sees_spheres(HostSim(b, B.root), B, "V1", api.camera(*SR.MR.camera_for("V1")), 131, 66)  # (what the GPU test of this fixture asserts)
    assert rays >= 20 and pixels >= 20, (rays, pixels)
