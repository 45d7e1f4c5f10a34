"""The sphere bihs, poses and scene descriptions of the sphere bih refit tests (test_sphere_bih_refit_host.py,
test_sphere_bih_update_gpu.py) -- test infrastructure, after bihs_refit.py.  Centres and radii are float64 throughout
(SceneDesc(round32=False)): the update's arithmetic is fp64 and is held to the bit.  A bih is an n x 4 array, cx cy cz r per sphere; sphere k
is item k of the bih (the order `bih` is given)."""
import numpy as np

import bihs_refit as BR
import meshes_refit as MR
from host_shade import primary_rays
from helpers import random_rays
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

MERGE_BLOCK = BR.MERGE_BLOCK  # bih_update_kernels.hpp kMergeBlock: the widest tree level the merged launch takes
WIDE_N = 85                   # the smallest lattice(N) with a level of more branch nodes than that (test_sphere_bih_refit_host.py asserts it)

Tree, traits = BR.Tree, BR.traits


def three_spheres():
    """a bih whose root is a leaf: no branch, no level launch"""
    return np.array([(-2.0, 1.0, 0.0, 0.8), (1.5, 1.5, -1.0, 1.0), (0.5, 3.0, 1.5, 0.6)])


def cluster_spheres():
    """31 scattered spheres and nine with one centre and different radii, which the builder cannot split: a leaf of nine (the 7+-item slot
    form of child_box) beside small and empty leaves; 40 spheres"""
    rng = np.random.default_rng(5)
    c = rng.uniform((-6.0, 0.4, -6.0), (6.0, 4.0, 6.0), size=(31, 3))
    r = rng.uniform(0.25, 0.6, size=(31, 1))
    same = np.array([(0.5, 2.0, 0.25, 0.3 + 0.05 * k) for k in range(9)])
    return np.concatenate([np.concatenate([c, r], axis=1), same])


def cloud_spheres():
    """300 seeded spheres: more than 64 (the folds cross a wave) and more than 256 (the bound kernels run a second block)"""
    rng = np.random.default_rng(9)
    c = rng.uniform((-6.0, 0.3, -6.0), (6.0, 4.5, 6.0), size=(300, 3))
    return np.concatenate([c, rng.uniform(0.1, 0.35, size=(300, 1))], axis=1)


def lattice(N):
    """N x N spheres on a plane lattice over [-6, 6]^2, a little height from an integer hash"""
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    h = ((i * 73856093) ^ (j * 19349663)) & 1023
    step = 12.0 / N
    return np.stack([i * step - 6.0 + step / 2, 1.0 + h / 1024.0, j * step - 6.0 + step / 2, np.full(i.shape, 0.35 * step)], axis=-1).reshape(-1, 4)


BIHS = {"three": three_spheres, "cluster": cluster_spheres, "cloud": cloud_spheres, "wide": lambda: lattice(WIDE_N)}
WRAPS = ("tex", "root", "instances", "bound")


def pose(S0, which):
    """V0: as built.  V1: centres displaced by a smooth seeded field plus jitter, radii scaled 0.5 - 1.5x per sphere; sphere 0 is then put
    where c == r on x (c - r is exactly 0, the one place a fold's order could show a zero's sign) and sphere 1 at a y of 0.1 (whose fp32
    rounding differs from the fp64 value).  V2: meshes_refit's similarity, radii scaled alike."""
    S0 = np.asarray(S0, dtype=np.float64)
    if which == "V0":
        return S0.copy()
    if which == "V2":
        return np.concatenate([S0[:, :3] * MR.V2_SCALE + MR.V2_SHIFT, S0[:, 3:] * MR.V2_SCALE], axis=1)
    if which != "V1":
        raise KeyError(which)
    rng = np.random.default_rng(13)
    c0 = S0[:, :3]
    d = np.stack([0.25 * np.sin(0.7 * c0[:, 2] + 0.3), 0.3 * np.sin(0.5 * c0[:, 0]) * np.cos(0.4 * c0[:, 2]), 0.2 * np.cos(0.6 * c0[:, 0])], 1)
    c = c0 + d + rng.uniform(-0.05, 0.05, c0.shape)
    r = S0[:, 3] * rng.uniform(0.5, 1.5, len(S0))
    c[0, 0] = r[0]
    c[1, 1] = 0.1
    S = np.concatenate([c, r[:, None]], axis=1)
    assert S[0, 0] - S[0, 3] == 0.0 and np.float64(np.float32(S[1, 1])) != S[1, 1]
    return S


def spheres(name, which="V0"):
    return pose(BIHS[name](), which)


def scene_desc_of(S, which="V0", wrap="tex"):
    """A SceneDesc over spheres S (already posed), the SceneDesc id of the bih node and the ids of the Sphere nodes, in item order.
      tex        scenes.s1's form: group [tex plane, bih [tex (sphere ..) mat ...]]
      root       the bih alone
      instances  two `transform`s of the one bih in a group (the generic tier)
      bound      the bih as the second operand of a Bound whose bounding solid is a large sphere"""
    sd = SceneDesc(round32=False)
    m = scenes.materials(sd)
    mats = [m["shiny_white"], m["shiny_red"], scenes.matte(sd, (0.5, 0.0, 1.0))]
    balls = [sd.sphere(tuple(float(x) for x in s[:3]), float(s[3])) for s in S]
    tree = sd.bih([sd.tex(b, mats[k % 3]) for k, b in enumerate(balls)])
    if wrap == "tex":
        root = sd.group([sd.tex(sd.plane((0, 0, 0), (0, 1, 0)), scenes.matte(sd, (0.0, 0.8, 0.3))), tree])
    elif wrap == "root":
        root = tree
    elif wrap == "instances":
        root = sd.group([sd.transform(tree, [api.translate((-4.0, 0.0, 0.0))]), sd.transform(tree, [api.rotate((0.0, 1.0, 0.0), 0.5), api.translate((5.0, 1.0, -3.0))])])
    elif wrap == "bound":
        root = sd.bound_object(sd.sphere((0.0, 0.0, 0.0), 400.0), tree)
    else:
        raise KeyError(wrap)
    sd.set_root(root)
    for pos, col in scenes.LIGHTS[:2]:
        sd.add_light(pos, col)
    sd.set_camera(*MR.camera_for(which))
    return sd, tree, balls


def scene_desc(name, which="V0", wrap="tex"):
    return scene_desc_of(spheres(name, which), which, wrap)


class Built:
    """a description replayed into a product builder: ids are builder ids"""

    def __init__(self, sd, tree, balls):
        self.sd = sd
        self.b = api.Builder()
        self.nm, _ = sd.replay(self.b)
        self.root, self.tree = self.nm[sd.root], self.nm[tree]
        self.balls = [self.nm[k] for k in balls]


def build(name, which="V0", wrap="tex"):
    return Built(*scene_desc(name, which, wrap))


def build_lattice(N):
    return Built(*scene_desc_of(lattice(N)))


def nested_desc(S, how="direct"):
    """The sphere bih under two bihs, on a floor: `mid` holds it as a direct item (how = "direct") or as `transform (tex bih)`, an instanced
    item (how = "instanced"), beside three static solids; `top` holds `mid` beside three more.  Returns (sd, tree, balls, mid, top)."""
    sd = SceneDesc(round32=False)
    m = scenes.materials(sd)
    mats = [m["shiny_white"], m["shiny_red"], scenes.matte(sd, (0.5, 0.0, 1.0))]
    balls = [sd.sphere(tuple(float(x) for x in s[:3]), float(s[3])) for s in S]
    tree = sd.bih([sd.tex(b, mats[k % 3]) for k, b in enumerate(balls)])
    item = tree if how == "direct" else sd.transform(sd.tex(tree, mats[1]), [api.rotate((0.0, 1.0, 0.0), 0.4), api.translate((0.5, 0.25, -1.0))])
    mid = sd.bih([item, sd.sphere((8.0, 1.0, 2.0), 0.7), sd.box((-9.0, 0.1, -3.0), (-8.0, 1.5, -2.0)), sd.sphere((7.5, 3.0, -4.0), 0.5)])
    top = sd.bih([mid, sd.tex(sd.box((-3.0, 5.5, -1.0), (-2.0, 6.5, 0.0)), m["shiny_white"]), sd.sphere((3.0, 6.0, 1.0), 0.6), sd.sphere((0.0, 1.0, 9.0), 0.8)])
    sd.set_root(sd.group([sd.tex(sd.plane((0, 0, 0), (0, 1, 0)), scenes.matte(sd, (0.0, 0.8, 0.3))), top]))
    for pos, col in scenes.LIGHTS[:2]:
        sd.add_light(pos, col)
    sd.set_camera(*scenes.CUST_CAM)
    return sd, tree, balls, mid, top


def build_nested(name, which="V0", how="direct"):
    sd, tree, balls, mid, top = nested_desc(spheres(name, which), how)
    B = Built(sd, tree, balls)
    B.mid, B.top = B.nm[mid], B.nm[top]
    return B


def check_fixture(name, wrap, B):
    """each fixture still is what it is described as: its tree's shape, and per wrap the tier and the bih's class"""
    T = Tree(B.b, B.tree)
    tr = traits(B.b, B.root)
    leaf_sizes = sorted(T.nleaf[k] for k in T.leaves())
    widths = T.level_widths()
    if name == "three":
        assert T.n == 1 and leaf_sizes == [3]
    elif name == "cluster":
        assert len(T.items[0]) == 40 and leaf_sizes[-1] >= 7 and leaf_sizes[0] == 0, leaf_sizes  # the slot form of a leaf, and an empty leaf
    elif name == "cloud":
        assert len(T.items[0]) == 300 and len(widths) > 3
    elif name == "wide":
        assert max(widths) > MERGE_BLOCK and widths[0] == 1, widths
    # the flat tier with the sphere bih as a root entry (rt_types.h CLS_BIH_SPHERE = 2; the plane: CLS_PRIMS = 16), or -- Instances, a Bound -- the
    # generic tier, whose packet service walks the tree
    assert (tr[0], tr[1]) == {"tex": (0, 18), "root": (0, 2), "instances": (1, 31), "bound": (1, 31)}[wrap], (wrap, tr)
    assert B.b.show(B.tree).startswith(("SI Bih", "Bih"))
    return T, tr


def sees_spheres(backend, B, which, cam, w, h):
    """(random rays of the tests that hit a sphere of the bih, pixels of a w x h frame whose primary ray does): what a comparison of two
    scenes' answers can tell apart.  backend: anything with rayint(o, d) -- helpers.HostSim, api.Scene."""
    ro, rd = rays_for(which)
    ids = np.asarray(B.balls)
    hit = backend.rayint(ro, rd)
    po, pd = primary_rays(cam, w, h)
    pix = backend.rayint(po, pd)
    return int(np.isin(hit["prim"][hit["t"] >= 0], ids).sum()), int(np.isin(pix["prim"][pix["t"] >= 0], ids).sum())


def rays_for(which, n=4000):
    """the tests' random rays: about the scene, following V2's similarity"""
    k = MR.V2_SCALE if which == "V2" else 1.0
    shift = MR.V2_SHIFT if which == "V2" else np.zeros(3)
    return random_rays(n, 23, center=tuple(np.array((0, 1.5, 0)) * k + shift), radius=13 * k, spread=7 * k)
