"""The scenes, poses and helpers of the Instance update tests (test_instance_refit_host.py, test_instance_update_gpu.py) -- test
infrastructure.  Constants are float64 throughout (SceneDesc(round32=False)): the update's arithmetic is fp64 and is held to the bit.

A fixture is built at a POSE.  Pose None is the scene as it is committed; at any other pose every movable Instance k is wrapped in one
more `transform` by extra(k, pose) -- which the builder folds into the Instance (Solid.hs:494-496), so the scene built fresh at a pose
holds, at the same place, an Instance whose matrix is compose([old matrix, extra]).  moved_matrices() computes exactly that product
for the update calls, so for these fixtures the builder after instance_set_transforms and the builder made fresh at the pose agree to
the bit wherever the fresh build picks the same trees."""
import re

import numpy as np

import bihs_refit as BR
import meshes_refit as MR
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

POSES = ("grow", "shrink")


def xf_of(builder, node):
    """the 24 doubles of Instance `node`, read from the builder's own `show` text (exact: GHC's show round-trips a Double); the node's
    own Xfm is the last one of its text"""
    text = builder.show(node)
    assert text.startswith(("SI Instance", "Instance")), text[:40]
    nums = re.findall(r"-?\d+\.\d+(?:e-?\d+)?", text[text.rindex("(Xfm (Matrix "):])
    assert len(nums) == 24, nums
    return np.array([float(x) for x in nums], dtype=np.float64)


def is_instance(builder, node):
    return builder.show(node).startswith(("SI Instance", "Instance"))


def sway(base, k, pose):
    """the pose's extra transform of movable k: a rotation of a few degrees about an axis through `base` (the item's own origin in
    the world) and a step away from (grow) or towards (shrink) the y axis"""
    rng = np.random.default_rng(1000 + k)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    ang = api.deg(float(rng.uniform(2.0, 6.0))) * (1 if pose == "grow" else -1)
    b = np.round(np.asarray(base, dtype=np.float64), 6)
    out = np.array([b[0], 0.0, b[2]])
    step = out * (0.25 if pose == "grow" else -0.2) + np.array([0.0, 0.3 if pose == "grow" else -0.1, 0.0])
    return api.compose([api.translate(tuple(-b)), api.rotate(tuple(float(x) for x in ax), ang), api.translate(tuple(b + step))])


class Fixture:
    """sd, and the SceneDesc ids of: the movable Instances in order, the bih that holds them (or None)"""

    def __init__(self, pose):
        self.sd = SceneDesc(round32=False)
        self.pose = pose
        self.movable = []   # SceneDesc ids of the Instances an update names (pose None), in order
        self.bases = []     # their origins in the world: what sway() turns about
        self.bih = None
        self.inserted = []  # at a pose: the SceneDesc ids of the transforms the pose added, one per movable

    def mv(self, node, base):
        """register `node`, an Instance, as movable k; at a pose, the Instance moved"""
        k = len(self.movable)
        self.bases.append(tuple(float(x) for x in base))
        if self.pose is not None:
            node = self.sd.transform(node, [sway(base, k, self.pose)])
            self.inserted.append(node)
        self.movable.append(node)
        return node

    def finish(self, root, cam):
        sd = self.sd
        sd.set_root(root)
        for pos, col in scenes.LIGHTS[:2]:
            sd.add_light(pos, col)
        sd.set_camera(*cam)
        return self


CAM = ((1.0, 6.0, 13.0), (0.0, 2.0, 0.0), (0.0, 1.0, 0.0), 55.0)


def _floor(sd):
    return sd.tex(sd.plane((0, 0, 0), (0, 1, 0)), scenes.matte(sd, (0.1, 0.7, 0.3)))


def flat3(pose=None):
    """(a) a root group of three Instances, one of them a cone's, no bih: the flat tier, xfm slots only"""
    f = Fixture(pose); sd = f.sd
    m = scenes.materials(sd)
    c = f.mv(sd.cone((-3.0, 0.5, 0.0), 0.9, (-2.5, 3.5, 0.5), 0.2), (-3.0, 0.5, 0.0))
    e = f.mv(sd.transform(sd.sphere((0, 0, 0), 1.0), [api.scale((1.5, 0.7, 1.0)), api.rotate((0, 0, 1), 0.4), api.translate((0.5, 2.0, 0.0))]), (0.5, 2.0, 0.0))
    d = f.mv(sd.transform(sd.difference(sd.box((-1, 0, -1), (1, 2, 1)), sd.sphere((0, 2, 0), 0.9)), [api.rotate((0, 1, 0), 0.6), api.translate((3.5, 0.2, -1.0))]), (3.5, 0.2, -1.0))
    return f.finish(sd.group([_floor(sd), sd.tex(c, m["shiny_red"]), sd.tex(e, m["shiny_white"]), sd.tex(d, scenes.matte(sd, (0.3, 0.4, 0.9)))]), CAM)


def shared(pose=None):
    """(b) one Instance held by two groups, one of them inside an Instance of its own: whatever holds it moves"""
    f = Fixture(pose); sd = f.sd
    m = scenes.materials(sd)
    inst = f.mv(sd.transform(sd.tex(sd.box((-0.5, 0, -0.5), (0.5, 1.5, 0.5)), m["shiny_red"]), [api.rotate((0, 1, 0), 0.3), api.translate((-1.0, 0.5, 0.0))]), (-1.0, 0.5, 0.0))
    g2 = sd.group([inst, sd.tex(sd.sphere((1.0, 1.0, 1.0), 0.6), m["shiny_white"])])
    far = sd.transform(g2, [api.rotate((0, 1, 0), 1.1), api.translate((3.5, 0.0, -2.0))])
    return f.finish(sd.group([_floor(sd), inst, sd.sphere((-3.5, 1.0, 1.0), 0.8), far]), CAM)


def subtrees(pose=None):
    """(c) an Instance of a small mesh and one of a small triangle bih: one update moves the whole subtree under it"""
    f = Fixture(pose); sd = f.sd
    mat = scenes.matte(sd, (0.8, 0.5, 0.4))
    V, N, T = MR.mixed_mesh()
    T = T.copy(); T[:, 6] = -1
    mesh = sd.tex(sd.mesh(V, N, T, []), mat)
    tree = sd.tex(sd.bih(sd.triangles_bulk(BR.triangles("mixed"))), scenes.matte(sd, (0.3, 0.5, 0.9)))
    a = f.mv(sd.transform(mesh, [api.scale((0.3, 0.3, 0.3)), api.translate((-3.0, 1.0, 0.0))]), (-3.0, 1.0, 0.0))
    b = f.mv(sd.transform(tree, [api.scale((0.3, 0.3, 0.3)), api.rotate((0, 1, 0), 0.5), api.translate((3.0, 1.5, -1.0))]), (3.0, 1.5, -1.0))
    return f.finish(sd.group([_floor(sd), a, b]), CAM)


def grove_items(f, n=40, seed=5):
    """about forty cylinders, cones and scaled spheres, every one an Instance, in the manner of zoo.grove; eight of them piled nearly on
    top of each other (a leaf the builder cannot split: the count escape)"""
    sd = f.sd
    m = scenes.materials(sd)
    mats = [m["shiny_red"], m["shiny_white"], scenes.matte(sd, (0.2, 0.5, 0.9)), scenes.matte(sd, (0.9, 0.8, 0.2))]
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k < 8:  # the pile
            pos = (0.001 * k, 2.0 + 0.001 * k, -0.001 * k)
            sc = (2.5, 0.5, 2.5)
        else:
            ang, rad = rng.uniform(0, 2 * np.pi), 4.5 * np.sqrt(rng.uniform(0.05, 1.0))
            pos = (float(rad * np.cos(ang)), float(rng.uniform(1.6, 4.2)), float(rad * np.sin(ang)))
            sc = tuple(float(x) for x in rng.uniform(0.3, 0.9, 3))
        kind = 0 if k < 8 else k % 4
        if kind == 0:
            it = sd.tex(f.mv(sd.transform(sd.sphere((0, 0, 0), 0.8), [api.scale(sc), api.translate(pos)]), pos), mats[k % 4])       # Tex above the Instance: an ellipsoid
        elif kind == 1:
            it = f.mv(sd.cone(pos, 0.35, (pos[0] + 0.3, pos[1] + 0.9, pos[2] - 0.2), 0.1), pos)                                       # `cone` itself
        elif kind == 2:
            it = f.mv(sd.transform(sd.tex(sd.cylinder((0, 0, 0), (0, 1.2, 0), 0.4), mats[k % 4]), [api.scale(sc), api.translate(pos)]), pos)  # Tex below it
        else:
            it = sd.noshadow(sd.tex(f.mv(sd.transform(sd.cone((0, 0, 0), 0.5, (0, 1.0, 0), 0.0), [api.scale(sc), api.translate(pos)]), pos), mats[k % 4]))
        out.append(it)
    return out


def grove(pose=None):
    """(d) a bih of forty Instances of one primitive each: class BC_CSG, walked in place by the interpreter's packet service"""
    f = Fixture(pose); sd = f.sd
    f.bih = sd.bih(grove_items(f))
    f.finish(sd.group([_floor(sd), f.bih]), ((0.5, 4.0, 9.5), (0.0, 2.0, 0.0), (0, 1, 0), 60))
    # zoo.grove's gates, for zoo.grove's reasons (quadrics under non-uniform scales: tests/zoo.py)
    sd.pixel_outlier_max, sd.rel_outlier_max, sd.pixel_mean_max = 6e-3, 2.5e-2, 2e-4
    return f


def _mixed_bih(f):
    sd = f.sd
    m = scenes.materials(sd)
    static = [sd.tex(sd.box((-4.0, 0.2, -3.0), (-3.0, 1.2, -2.0)), m["shiny_red"]), sd.tex(sd.sphere((3.5, 1.0, 2.5), 0.8), m["shiny_white"]),
              sd.tex(sd.difference(sd.box((-0.5, 0.2, 2.5), (0.8, 1.5, 3.8)), sd.sphere((0.8, 1.5, 3.8), 0.7)), scenes.matte(sd, (0.9, 0.8, 0.2)))]
    moving = []
    for k, pos in enumerate([(-2.0, 1.0, 0.5), (0.0, 2.5, -1.0), (2.0, 1.2, 0.0), (-1.0, 3.0, 2.0), (1.5, 3.2, -2.5)]):
        g = sd.group([sd.box((-0.4, 0, -0.4), (0.4, 0.5, 0.4)), sd.tex(sd.sphere((0, 0.8, 0), 0.35), m["shiny_red"]), sd.cylinder((0, 0.5, 0), (0, 1.4, 0), 0.12)])
        moving.append(f.mv(sd.transform(sd.tex(g, scenes.matte(sd, (0.2, 0.5, 0.9))), [api.rotate((1, 0, 0), 0.2 * k), api.translate(pos)]), pos))
    return sd.bih(static + moving)


def mixed(pose=None):
    """(e) a bih of static items that are no Instances (a box, a sphere, a Difference) and Instances of groups: class BC_GENERIC"""
    f = Fixture(pose)
    f.bih = _mixed_bih(f)
    return f.finish(f.sd.group([_floor(f.sd), f.bih]), CAM)


def mixed_nested(pose=None):
    """(f) that bih under an outer Instance and under a Bound: not at the root"""
    f = Fixture(pose); sd = f.sd
    f.bih = _mixed_bih(f)
    inner = sd.transform(f.bih, [api.rotate((0, 1, 0), 0.4), api.translate((0.5, 0.0, -1.0))])
    return f.finish(sd.group([_floor(sd), sd.bound_object(sd.sphere((0.0, 2.0, 0.0), 30.0), inner)]), CAM)


OAK_AGE = 6.9  # (leaves 0.9 across before the branches' scalings: they cover the twig ends and the joints below them, where coincident cone
                # ends make an fp32 ray report the other surface -- at 6.4 the host build of the FRESH oak has 3-6 of 9,000-13,000 hits beyond
                # parity.py's 1e-4, over its OUTLIER_MAX; at 6.9 none to two of 16,000-23,000)
OAK_CAM = ((0.5, 3.0, 5.5), (0.0, 2.2, 0.0), (0.0, 1.0, 0.0), 55.0)


def oak(pose=None):
    """(g) scenes.oak at a small age (31 cones, 32 spheres), alone and close up.  Its items are made inside the backend (flatten_transform),
    so a SceneDesc cannot name them: the update tests take them from Builder.bih_items, and the scene at a pose is oak_explicit."""
    assert pose is None
    f = Fixture(None); sd = f.sd
    top = scenes.oak(sd, OAK_AGE, 42)
    f.bih = top - 2  # tag (tex (bih_tolist ...)): scenes.oak's last three nodes (build_oak asserts that it is the Bih)
    return f.finish(top, OAK_CAM)


def oak_explicit(pose=None):
    """The same oak with every item written out -- flatten_transform done here: item = transform(cone or leaf, the chain of its
    ancestors' transforms) -- in scenes.oak's item order, so that item k can be moved by the pose.  The matrices are the same products
    associated differently: equal to rounding, which test_instance_refit_host.py checks on the items' bounds."""
    f = Fixture(pose); sd = f.sd
    year, season = int(np.floor(OAK_AGE)), OAK_AGE - int(np.floor(OAK_AGE))
    thickness, minbranch, maxbranch = 0.03, api.deg(10), api.deg(25)
    leaf_mat = scenes.matte(sd, (0.2, 1, 0.4))
    items = []

    def place(node, chain):
        M = api.compose(chain) if chain else api.compose([api.translate((0, 0, 0))])
        items.append(f.mv(sd.transform(node, [M]), (M[3], M[7], M[11])))

    def tree(n_, r, chain):
        if n_ == 0:
            return
        if n_ == 1:
            place(sd.tex(sd.sphere((0, 0, 0), season), leaf_mat), chain)
            return
        nf = float(n_)
        rng1, rng2 = r.split()
        rng3, rng4 = rng1.split()
        r1, rng5 = rng4.randomR(0.0, 0.5)
        r2, rng6 = rng5.randomR(minbranch, maxbranch)
        r3, _ = rng6.randomR(0.8, 0.95)
        seglen, branchang, scaling = 0.5 + r1, r2, r3
        place(sd.cone((0, 0, 0), thickness * nf, (0, seglen, 0), thickness * (nf - 1) * scaling), chain)
        for sub, ang in ((rng2, branchang), (rng3, -branchang)):
            tree(n_ - 1, sub, [api.scale((scaling, scaling, scaling)), api.rotate((0, 0, 1), ang), api.rotate((0, 1, 0), api.deg(30)), api.translate((0, seglen, 0))] + chain)

    tree(year, scenes._Draws(42), [])
    f.bih = sd.bih(items)
    f.finish(sd.tag(sd.tex(f.bih, scenes.matte(sd, (0.8, 0.5, 0.4))), "tree"), OAK_CAM)
    # scenes.testscene's gates for the oak, for its reasons (coincident joints, twig-end spheres: glome_amd/scenes.py)
    sd.rel_outlier_max, sd.same_prim_min, sd.pixel_outlier_max, sd.pixel_mean_max = 2.0e-2, 0.95, 6e-3, 4e-4
    return f


FIXTURES = {"flat3": flat3, "shared": shared, "subtrees": subtrees, "grove": grove, "mixed": mixed, "mixed_nested": mixed_nested}


class Built:
    """a fixture replayed into a product builder: ids are builder ids"""

    def __init__(self, fx):
        self.fx, self.sd = fx, fx.sd
        self.b = api.Builder()
        self.nm, _ = fx.sd.replay(self.b)
        self.root = self.nm[fx.sd.root]
        self.bih = None if fx.bih is None else self.nm[fx.bih]
        self.ids = [self.nm[k] for k in fx.movable]
        self.bases = list(fx.bases)


def build(name, pose=None):
    return Built(FIXTURES[name](pose))


def build_oak():
    """scenes.oak committed as it is: the movable Instances are the bih's items, their bases the origins their matrices map to"""
    B = Built(oak())
    assert B.b.show(B.bih).startswith(("SI Bih", "Bih")), B.b.show(B.bih)[:40]
    B.ids = B.b.bih_items(B.bih)
    assert all(is_instance(B.b, i) for i in B.ids)
    B.bases = [tuple(xf_of(B.b, i)[[3, 7, 11]]) for i in B.ids]
    return B


def moved_matrices(B, pose, which=None):
    """(ids, n x 24 matrices) of movables `which` (default: all) at `pose`: compose([the builder's own matrix, the pose's extra]) --
    what `transform` of the Instance by the extra makes"""
    which = range(len(B.ids)) if which is None else which
    ids = [B.ids[k] for k in which]
    return ids, np.stack([api.compose([xf_of(B.b, B.ids[k]), sway(B.bases[k], k, pose)]) for k in which])


def original_matrices(B, which=None):
    which = range(len(B.ids)) if which is None else which
    return [B.ids[k] for k in which], np.stack([xf_of(B.b, B.ids[k]) for k in which])


def node_map_at_pose(A, F):
    """For the parity checks of a scene UPDATED to a pose: the node map that takes the ids of F's description (the fixture built fresh at
    the pose, which the oracle is loaded with) to the ids of builder A (the fixture as committed).  F's description is A's with one
    transform added per movable, which is no primitive and so is never reported: it maps to no node (-1)."""
    base = iter(A.nm)
    added = set(F.fx.inserted)
    return [-1 if j in added else next(base) for j in range(F.sd.n_nodes)]


def plane_bih(b):
    """a bih that holds an Instance of a plane: `bound` of a plane is the reference's "everything", +-1e6, and a shift by delta puts a
    corner's padded coordinate on -1e6 exactly ((-1e6 + 1e-4) - 1e-4 == -1e6 in float64): the box `bih` itself refuses"""
    pl = b.transform(b.plane((0, 0, 0), (0, 1, 0)), [api.rotate((0, 1, 0), 0.3)])
    tree = b.bih([pl, b.sphere((0, 1, 0), 1.0), b.sphere((3, 1, 0), 1.0), b.sphere((0, 1, 3), 1.0)])
    return pl, tree


def peel(builder, node):
    """the Instance under the Tex / NoShadow / OnlyShadow wrappers of `node`, in a builder where a wrapper is made right after the node it
    wraps (the `show` reader and these fixtures): each step is checked on the texts"""
    while not is_instance(builder, node):
        outer, inner = builder.show(node), builder.show(node - 1)
        assert outer.startswith(("SI Tex", "Tex", "SI NoShadow", "NoShadow", "SI OnlyShadow", "OnlyShadow")) and inner.removeprefix("SI ") in outer, (node, outer[:60])
        node -= 1
    return node


OAK_RAYS = dict(n=40000, seed=11, center=(0.0, 2.2, 0.0), radius=4.0, spread=1.5)  # close up: half of them hit the tree


def check_oak_rays(rayint, shadow, F):
    """parity.check_rays for the oak at a pose, F the oak written out at that pose (what the oracle is loaded with): its hit / miss, distance
    and shadow checks under parity.py's own bounds.  Its comparison of primitive ids is left out: the committed oak's items are made
    inside the builder (flatten_transform) and have no ids in common with the written-out oak's.  Returns the levels."""
    import parity
    from helpers import random_rays
    o, om, _ = parity.oracle_for(F.sd)
    ro, rd = random_rays(OAK_RAYS["n"], OAK_RAYS["seed"], center=OAK_RAYS["center"], radius=OAK_RAYS["radius"], spread=OAK_RAYS["spread"])
    ref = o.rayint(om[F.sd.root], ro.astype(np.float64), rd.astype(np.float64))
    mism, emax, err = parity.compare_hits(rayint(ro, rd)["t"], ref["t"])
    lv = {"hits": int(err.size), "mismatch": mism, "t_outliers": float(np.mean(err > parity.T_RTOL)), "t_err_max": emax}
    print("oak rays:", lv)
    assert err.size >= 10000, lv
    assert mism <= parity.MISMATCH_MAX, lv
    assert lv["t_outliers"] <= parity.OUTLIER_MAX, lv
    tm = np.random.default_rng(OAK_RAYS["seed"] + 1).uniform(1, 30, size=len(ro)).astype(np.float32)
    so = o.shadow(om[F.sd.root], ro.astype(np.float64), rd.astype(np.float64), tm.astype(np.float64))
    lv["shadow_mismatch"] = float(np.mean(so != shadow(ro, rd, tm)))
    assert lv["shadow_mismatch"] <= parity.MISMATCH_MAX, lv
    return lv
