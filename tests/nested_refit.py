"""The scenes, poses and helpers of the nested refit tests (test_nested_refit_host.py, test_nested_update_gpu.py) -- test infrastructure.
Objects that lie UNDER a bih move -- a triangle bih, a mesh, Instances -- and the bihs above them are refitted, inner trees first.
Constants are float64 throughout (SceneDesc(round32=False)): the arithmetic is fp64 and is held to the bit.  No coordinate is chosen so
that a padded value p -+ 1e-4 is zero: the sign of a zero is the one thing a fold's order could show (item_bih_update_kernels.hpp).

A fixture is built at a POSE in the manner of instances_refit.py: pose None is the scene as committed, "grow" / "shrink" the scene with
every movable moved.  A movable is ("bih", node, n x 9 triangles), ("mesh", node, vertices) or ("inst", node, base): `moves(B, pose)`
gives, for a fixture built at pose None, the update calls that take it to the pose."""
import numpy as np

import instances_refit as IR
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

POSES = ("grow", "shrink")
CAM = ((1.0, 6.0, 13.0), (0.0, 2.0, 0.0), (0.0, 1.0, 0.0), 55.0)


def pose_points(P, pose, k=0):
    """points P (n x 3) at a pose: scaled about their (rounded) centre and shifted, so the object's bound grows or shrinks AND moves"""
    P = np.asarray(P, dtype=np.float64)
    if pose is None:
        return P.copy()
    c = np.round(P.mean(axis=0), 3)
    s, shift = (1.3, np.array([0.4, 0.3, -0.25])) if pose == "grow" else (0.8, np.array([-0.15, 0.1, 0.2]))
    return (P - c) * s + c + shift * (1 + 0.5 * k)


def tris70():
    """70 triangles about (-3, 1.5, 0): 61 of a small heightfield and a pile of nine nearly coincident ones -- a leaf of seven or more
    (the count escape in child_box) -- in a tree with the packet form"""
    hf = scenes.heightfield_triangles(6)[:61].reshape(-1, 3) * np.array([0.25, 0.6, 0.25]) + np.array([-3.0, 1.5, 0.0])
    pile = []
    for k in range(9):
        y = 2.6 + 1e-3 * k
        pile.append((-4.5 + 1e-3 * k, y, -1.5, -1.5, y, -1.5 - 1e-3 * k, -3.0, y + 5e-4 * k, 1.5))
    return np.concatenate([hf.reshape(-1, 9), np.array(pile)])


def tris9():
    """nine triangles about (3, 1, 1): an odd last pair"""
    return (scenes.heightfield_triangles(3)[:9].reshape(-1, 3) * np.array([0.2, 0.5, 0.2]) + np.array([3.0, 1.0, 1.0])).reshape(-1, 9)


def patch_mesh():
    """the grid patch of meshes_refit.py at N = 4 (32 triangles), scaled down to about two units across, untextured triangles"""
    import meshes_refit as MR
    N = 4
    V = scenes.heightfield_vertices(N).reshape(-1, 3) * np.array([0.1, 0.4, 0.1]) + np.array([0.0, 1.0, 0.0])
    tris = np.full((2 * N * N, 8), -1, dtype=np.int32)
    tris[:, :3] = MR._grid_tris(N)
    return V, np.zeros((0, 3)), tris


class Fixture:
    def __init__(self, pose):
        self.sd = SceneDesc(round32=False)
        self.pose = pose
        self.movable = []   # (kind, SceneDesc node, data at pose None)
        self.bihs = {}      # name -> SceneDesc node of a bih that is refitted
        self.above = {}     # index of a movable -> the names of the bihs above it, in a valid refit order
        self.inserted = []  # at a pose: the transforms the pose added (instances_refit.node_map_at_pose)
        self.named = {}     # name -> SceneDesc node of anything else a test wants to find

    def tri_bih(self, P0):
        k = len(self.movable)
        node = self.sd.bih(self.sd.triangles_bulk(pose_points(P0.reshape(-1, 3), self.pose, k).reshape(-1, 9)))
        self.movable.append(("bih", node, P0))
        return node

    def mesh(self, V0, N0, T):
        k = len(self.movable)
        node = self.sd.mesh(pose_points(V0, self.pose, k), N0, T, [])
        self.movable.append(("mesh", node, V0))
        return node

    def inst(self, node, base):
        k = len(self.movable)
        if self.pose is not None:
            node = self.sd.transform(node, [IR.sway(base, k, self.pose)])
            self.inserted.append(node)
        self.movable.append(("inst", node, tuple(float(x) for x in base)))
        return node

    def finish(self, root, cam=CAM):
        self.sd.set_root(root)
        for pos, col in scenes.LIGHTS[:2]:
            self.sd.add_light(pos, col)
        self.sd.set_camera(*cam)
        return self


def _floor(sd):
    return sd.tex(sd.plane((0, 0, 0), (0, 1, 0)), scenes.matte(sd, (0.1, 0.7, 0.3)))


def nff_like(pose=None):
    """what glome_sb_load_nff returns: root bih [tex (bih 70 triangles), tex (bih 9 triangles), 3 spheres]"""
    f = Fixture(pose); sd = f.sd
    m = scenes.materials(sd)
    a = sd.tex(f.tri_bih(tris70()), scenes.matte(sd, (0.8, 0.5, 0.4)))
    b = sd.tex(f.tri_bih(tris9()), scenes.matte(sd, (0.3, 0.5, 0.9)))
    balls = [sd.tex(sd.sphere(c, r), m["shiny_red"]) for c, r in (((0.0, 0.8, -2.0), 0.8), ((1.0, 3.5, 0.5), 0.5), ((-1.0, 0.6, 3.0), 0.6))]
    f.bihs["root"] = sd.bih([a, b] + balls)
    f.above = {0: ["root"], 1: ["root"]}
    return f.finish(f.bihs["root"])


def mesh_shared(pose=None):
    """root bih of 70 static spheres (more than 64 items: the box fold crosses a wave), a small mesh as a direct item, and the same mesh
    under two different transforms: direct and instanced rows from one bound.  The tree stands on a floor plane in a root group, as the
    fixtures of instances_refit.py do: parity.py's bounds are FRACTIONS of the rays that hit, measured on scenes most of its rays hit,
    and without a floor a tenth of them hit this scene at all -- then the one ray in 20,000 that slips through a seam of the mesh in fp32
    (the scene built FRESH at a pose has it too, in the host build: 1 of 2,157 hits) is already over the bound of 2 in 10,000."""
    f = Fixture(pose); sd = f.sd
    m = scenes.materials(sd)
    rng = np.random.default_rng(3)
    balls = []
    for k in range(70):
        ang, rad = rng.uniform(0, 2 * np.pi), rng.uniform(3.0, 6.0)
        balls.append(sd.tex(sd.sphere((float(rad * np.cos(ang)), float(rng.uniform(0.3, 4.0)), float(rad * np.sin(ang))), float(rng.uniform(0.15, 0.35))), m["shiny_white"]))
    me = f.mesh(*patch_mesh())
    direct = sd.tex(me, scenes.matte(sd, (0.8, 0.5, 0.4)))
    i1 = sd.transform(sd.tex(me, m["shiny_red"]), [api.rotate((0, 1, 0), 0.7), api.translate((-2.0, 0.5, 1.0))])
    f.named["i2"] = sd.transform(me, [api.scale((0.8, 1.2, 0.8)), api.rotate((0, 0, 1), 0.2), api.translate((2.0, 1.0, -1.0))])
    i2 = sd.tex(f.named["i2"], scenes.matte(sd, (0.2, 0.5, 0.9)))
    f.named["i1"] = i1
    f.bihs["root"] = sd.bih(balls + [direct, i1, i2])
    f.above = {0: ["root"]}
    return f.finish(sd.group([_floor(sd), f.bihs["root"]]))


def two_parents(pose=None):
    """one triangle bih as an item of two different outer bihs under a group (one of them holds it through an Instance)"""
    f = Fixture(pose); sd = f.sd
    m = scenes.materials(sd)
    t = f.tri_bih(tris9())
    item = sd.tex(t, scenes.matte(sd, (0.3, 0.5, 0.9)))
    f.bihs["o1"] = sd.bih([item, sd.sphere((1.0, 1.0, -1.0), 0.5), sd.sphere((4.5, 2.0, 2.0), 0.4), sd.sphere((2.0, 3.0, 3.0), 0.3), sd.box((4.0, 0.1, -1.0), (5.0, 1.0, 0.0))])
    far = sd.transform(item, [api.rotate((0, 1, 0), 1.0), api.translate((-5.0, 0.5, -1.0))])
    f.bihs["o2"] = sd.bih([far, sd.tex(sd.sphere((-2.0, 1.0, 2.0), 0.6), m["shiny_red"]), sd.sphere((-4.0, 3.0, 0.0), 0.4), sd.sphere((-1.5, 2.5, -2.0), 0.3)])
    f.above = {0: ["o1", "o2"]}
    return f.finish(sd.group([_floor(sd), f.bihs["o1"], f.bihs["o2"]]))  # (on a floor, for mesh_shared's reason: 2,300 of 20,000 rays hit the trees)


def chain(pose=None):
    """three levels written out, what oak_in_scene is with items a description can name: Instances of a cone, an ellipsoid and a cylinder
    as items of an inner bih with a static box, `transform (tag (tex inner))` an item of the root bih beside a box and two spheres"""
    f = Fixture(pose); sd = f.sd
    m = scenes.materials(sd)
    a = f.inst(sd.cone((-0.8, 0.2, 0.0), 0.4, (-0.6, 1.4, 0.2), 0.1), (-0.8, 0.2, 0.0))
    b = sd.tex(f.inst(sd.transform(sd.sphere((0, 0, 0), 0.5), [api.scale((1.2, 0.6, 0.9)), api.translate((0.6, 0.9, 0.3))]), (0.6, 0.9, 0.3)), m["shiny_red"])
    c = f.inst(sd.transform(sd.cylinder((0, 0, 0), (0, 0.9, 0), 0.2), [api.rotate((1, 0, 0), 0.3), api.translate((0.1, 0.3, -0.9))]), (0.1, 0.3, -0.9))
    f.bihs["inner"] = sd.bih([a, b, c, sd.box((-0.3, 0.0, 0.6), (0.3, 0.5, 1.1)), sd.sphere((0.9, 0.3, -0.6), 0.25)])
    placed = sd.transform(sd.tag(sd.tex(f.bihs["inner"], scenes.matte(sd, (0.8, 0.5, 0.4))), "tree"), [api.rotate((0, 1, 0), 0.5), api.translate((0.5, 0.5, 0.0))])
    f.bihs["root"] = sd.bih([placed, sd.tex(sd.box((-4.0, 0.0, -2.0), (-3.0, 1.0, -1.0)), m["shiny_white"]), sd.sphere((3.5, 1.0, 1.0), 0.8), sd.sphere((-2.0, 2.5, 2.0), 0.5)])
    f.above = {0: ["inner", "root"], 1: ["inner", "root"], 2: ["inner", "root"]}
    return f.finish(sd.group([_floor(sd), f.bihs["root"]]))  # (on a floor, for mesh_shared's reason: 844 of 20,000 rays hit the trees)


FIXTURES = {"nff_like": nff_like, "mesh_shared": mesh_shared, "two_parents": two_parents, "chain": chain}


class Built:
    """a fixture replayed into a product builder: ids are builder ids"""

    def __init__(self, fx):
        self.fx, self.sd = fx, fx.sd
        self.b = api.Builder()
        self.nm, _ = fx.sd.replay(self.b)
        self.root = self.nm[fx.sd.root]
        self.bihs = {k: self.nm[v] for k, v in fx.bihs.items()}
        self.named = {k: self.nm[v] for k, v in fx.named.items()}
        self.movable = [(kind, self.nm[node], data) for kind, node, data in fx.movable]
        self.above = {k: [self.bihs[n] for n in names] for k, names in fx.above.items()}


def build(name, pose=None):
    return Built(FIXTURES[name](pose))


def oak_in_scene():
    """instances_refit.oak's small oak as `transform (tag (tex oak))` inside a root bih with a box and two spheres: Instance item -> inner
    bih -> wrappers -> Instance -> root bih.  The oak's items are made inside the builder, so the movables come from Builder.bih_items."""
    f = Fixture(None); sd = f.sd
    m = scenes.materials(sd)
    top = scenes.oak(sd, IR.OAK_AGE, 42)
    f.bihs["inner"] = top - 2
    placed = sd.transform(top, [api.rotate((0, 1, 0), 0.4), api.translate((0.3, 0.0, -0.5))])
    f.bihs["root"] = sd.bih([placed, sd.tex(sd.box((-3.0, 0.0, -1.0), (-2.2, 0.8, -0.2)), m["shiny_white"]), sd.sphere((2.5, 0.8, 0.5), 0.7), sd.sphere((-1.5, 3.5, 1.0), 0.4)])
    f.finish(f.bihs["root"], IR.OAK_CAM)
    B = Built(f)
    assert B.b.show(B.bihs["inner"]).startswith(("SI Bih", "Bih")), B.b.show(B.bihs["inner"])[:40]
    twigs = B.b.bih_items(B.bihs["inner"])
    assert all(IR.is_instance(B.b, i) for i in twigs)
    B.movable = [("inst", i, tuple(IR.xf_of(B.b, i)[[3, 7, 11]])) for i in twigs]
    B.above = {k: [B.bihs["inner"], B.bihs["root"]] for k in range(len(twigs))}
    return B


def get(name):
    return oak_in_scene() if name == "oak_in_scene" else build(name)


ALL = sorted(FIXTURES) + ["oak_in_scene"]


def moves(B, pose, which=None):
    """the update calls that take B (built at pose None, its builder untouched so far) to `pose`: a list of (kind, id(s), array) -- one
    per moved mesh / triangle bih, and ONE for all the moved Instances together -- and per call the index of a movable it moves"""
    which = range(len(B.movable)) if which is None else which
    out, ids, M, first = [], [], [], None
    for k in which:
        kind, node, data = B.movable[k]
        if kind == "inst":
            ids.append(node); M.append(api.compose([IR.xf_of(B.b, node), IR.sway(data, k, pose)]))
            first = k if first is None else first
        else:
            out.append((kind, node, pose_points(data.reshape(-1, 3), pose, k).reshape(data.shape), k))
    if ids:
        out.append(("inst", ids, np.stack(M), first))
    return out


def original(B, which=None):
    """the calls that take B back: the data it was built with"""
    which = range(len(B.movable)) if which is None else which
    out, ids, M, first = [], [], [], None
    for k in which:
        kind, node, data = B.movable[k]
        if kind == "inst":
            ids.append(node); M.append(IR.xf_of(B.b, node)); first = k if first is None else first
        else:
            out.append((kind, node, data.copy(), k))
    if ids:
        out.append(("inst", ids, np.stack(M), first))
    return out


def apply_host(b, call):
    kind, node, data, _ = call
    if kind == "mesh":
        b.mesh_set_vertices(node, data)
    elif kind == "bih":
        b.bih_set_triangles(node, data)
    else:
        b.instance_set_transforms(node, data)


def apply_scene(sc, call):
    """the same call on a committed scene (host forms); returns the device milliseconds"""
    kind, node, data, _ = call
    if kind == "mesh":
        return sc.mesh_update(node, data)
    if kind == "bih":
        return sc.bih_update(node, data)
    return sc.instance_update(node, data)


def node_of(call):
    """a node the call moves (for bihs_above: every node of one call has the same trees above it in these fixtures)"""
    return call[1][0] if call[0] == "inst" else call[1]


def host_sequence(B, calls):
    """the specification: each update, then bih_refit of every bih above it, inner trees first"""
    for call in calls:
        apply_host(B.b, call)
        for t in B.b.bihs_above(B.root, node_of(call)):
            B.b.bih_refit(t)


# ---- refused shapes: (builder, root, node, the message's pattern) ----
def refused_mesh_in_group(b):
    V, N, T = patch_mesh()
    me = b.mesh(V, N, T, [])
    g = b.group([me, b.sphere((0.0, 3.0, 0.0), 0.4)])
    root = b.bih([g, b.sphere((3.0, 1.0, 0.0), 0.5), b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 3.0), 0.5)])
    return root, me, rf"mesh {me} lies inside an item of bih {root} under List {g}"


def refused_bih_under_difference(b):
    t = b.bih(b.triangles_bulk(tris9()))
    d = b.difference(t, b.sphere((3.0, 1.0, 1.0), 0.3))
    root = b.bih([d, b.sphere((3.0, 1.0, -2.0), 0.5), b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 3.0), 0.5)])
    return root, t, rf"bih {t} lies inside an item of bih {root} under Difference {d}"


def refused_instance_under_instance(b):
    x = b.transform(b.sphere((0.0, 0.0, 0.0), 0.4), [api.scale((1.0, 0.5, 1.0)), api.translate((0.5, 1.0, 0.0))])
    g = b.group([x, b.sphere((0.0, 2.0, 0.0), 0.3)])
    outer_inst = b.transform(g, [api.rotate((0, 1, 0), 0.3), api.translate((1.0, 0.0, 0.0))])
    inner = b.bih([outer_inst, b.sphere((3.0, 1.0, 0.0), 0.5), b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 3.0), 0.5)])
    root = b.bih([inner, b.sphere((6.0, 1.0, 0.0), 0.5), b.sphere((-6.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 6.0), 0.5)])
    return root, x, rf"instance {x} lies inside an item of bih {inner} under Instance {outer_inst}"


REFUSED = {"mesh_in_group": refused_mesh_in_group, "bih_under_difference": refused_bih_under_difference, "instance_under_instance": refused_instance_under_instance}
