"""The triangle bihs, deformations and scene descriptions of the bih refit tests (test_bih_refit_host.py, test_bih_update_gpu.py) -- test
infrastructure.  Vertices are float64 throughout (SceneDesc(round32=False)): the update's arithmetic is fp64 and is held to the bit.  The
deformations are meshes_refit.deform's, applied to the triangles' 3 n vertices."""
import ctypes as C

import numpy as np

import meshes_refit as MR
from glome_amd import _lib as L
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

MERGE_BLOCK = 1024  # bih_update_kernels.hpp kMergeBlock: the widest tree level the merged launch (GLOME_DEBUG_BIH_UPDATE_MERGED) takes
WIDE_N = 56         # the smallest s3(N) with a level of more branch nodes than that (test_bih_refit_host.py asserts it, and that WIDE_N - 1 has none)


def three_triangles():
    """a bih whose root is a leaf: no branch, no level launch, an odd pair"""
    return np.array([(-3.0, 0.5, -1.0, 3.5, 0.25, -2.0, 0.5, 4.0, 1.5), (-2.0, 0.0, 2.0, 4.0, 0.5, 2.5, 1.0, 3.0, -3.0), (-4.0, 1.0, 0.0, -1.0, 3.5, 0.5, -2.5, 0.5, 3.0)])


def mixed_triangles():
    """scenes.heightfield_triangles(12) -- 288 triangles -- and a pile of nine large, nearly coincident triangles (meshes_refit.mixed_mesh's
    pile formula) that the builder cannot split: a leaf of nine (the 7+-item slot form, an odd count of pairs) beside leaves of two and
    empty leaves (infinite planes); 297 triangles, no multiple of 64"""
    pile = []
    for k in range(9):
        y = 2.5 + 1e-3 * k
        pile.append((-9.0 + 1e-3 * k, y, -9.0, 9.0, y, -9.0 - 1e-3 * k, 0.0, y + 5e-4 * k, 9.0))
    return np.concatenate([scenes.heightfield_triangles(12), np.array(pile)])


BIHS = {"three": three_triangles, "mixed": mixed_triangles, "s3_20": lambda: scenes.heightfield_triangles(20), "wide": lambda: scenes.heightfield_triangles(WIDE_N)}
WRAPS = ("root", "tex", "instances", "bound")


def triangles(name, which="V0"):
    """the n x 9 array of bih `name` deformed by `which` (meshes_refit.deform over its 3 n vertices)"""
    P0 = BIHS[name]()
    return MR.deform(P0.reshape(-1, 3), which)[0].reshape(-1, 9)


def scene_desc(name, which="V0", wrap="tex"):
    """A SceneDesc of bih `name` with triangles `which`, and the SceneDesc id of the bih node.
      root       the bare bih is the scene
      tex        `tex (bih (map triangle ...)) matte`: the flagship's form, scenes.s3's
      instances  two Instances of the one textured bih
      bound      the textured bih as the second operand of a Bound whose bounding solid is a large sphere"""
    sd = SceneDesc(round32=False)
    mat = scenes.matte(sd, (0.8, 0.5, 0.4))
    tree = sd.bih(sd.triangles_bulk(triangles(name, which)))
    if wrap == "root":
        root = tree
    elif wrap == "tex":
        root = sd.tex(tree, mat)
    elif wrap == "instances":
        t = sd.tex(tree, mat)
        root = sd.group([sd.transform(t, [api.translate((-4.0, 0.0, 0.0))]), sd.transform(t, [api.rotate((0.0, 1.0, 0.0), 0.5), api.translate((5.0, 1.0, -3.0))])])
    elif wrap == "bound":
        root = sd.bound_object(sd.sphere((0.0, 0.0, 0.0), 400.0), sd.tex(tree, mat))
    else:
        raise KeyError(wrap)
    sd.set_root(root)
    for pos, col in scenes.LIGHTS[:2]:
        sd.add_light(pos, col)
    sd.set_camera(*MR.camera_for(which))
    return sd, tree


def build(name, which="V0", wrap="tex"):
    """(sd, builder, node map, bih node) of bih `name` built with triangles `which`"""
    sd, tree = scene_desc(name, which, wrap)
    b = api.Builder()
    nm, _ = sd.replay(b)
    return sd, b, nm, nm[tree]


def build_n(N):
    """(sd, builder, node map, bih node) of `tex (bih ...)` over scenes.heightfield_triangles(N)"""
    sd = SceneDesc(round32=False)
    mat = scenes.matte(sd, (0.8, 0.5, 0.4))
    tree = sd.bih(sd.triangles_bulk(scenes.heightfield_triangles(N)))
    sd.set_root(sd.tex(tree, mat))
    b = api.Builder()
    nm, _ = sd.replay(b)
    return sd, b, nm, nm[tree]


class Tree:
    """a bih as glome_sb_bih_dump gives it: preorder arrays, and per node the items below it"""

    def __init__(self, builder, node):
        self.ls, self.rs, self.axis, self.nleaf, prims = builder.bih_dump(node)
        self.n = len(self.axis)
        self.left, self.right, self.items = [-1] * self.n, [-1] * self.n, [None] * self.n
        self.depth = [0] * self.n
        at, k = 0, 0
        stack = []  # (node, children still to come)
        for k in range(self.n):
            while stack and stack[-1][1] == 0:
                stack.pop()
            if stack:
                p, left_to_come = stack[-1]
                (self.left if left_to_come == 2 else self.right)[p] = k
                stack[-1] = (p, left_to_come - 1)
                self.depth[k] = self.depth[p] + 1
            if self.axis[k] < 0:
                self.items[k] = [int(x) for x in prims[at:at + self.nleaf[k]]]
                at += self.nleaf[k]
            else:
                stack.append((k, 2))
        for k in range(self.n - 1, -1, -1):
            if self.axis[k] >= 0:
                self.items[k] = self.items[self.left[k]] + self.items[self.right[k]]

    def branches(self):
        return [k for k in range(self.n) if self.axis[k] >= 0]

    def leaves(self):
        return [k for k in range(self.n) if self.axis[k] < 0]

    def level_widths(self):
        """branch nodes per tree level"""
        w = {}
        for k in self.branches():
            w[self.depth[k]] = w.get(self.depth[k], 0) + 1
        return [w[d] for d in sorted(w)]

    def shape(self):
        """what a refit must leave alone: axes, leaf counts, leaf items"""
        return list(self.axis), list(self.nleaf), [self.items[k] for k in self.leaves()]


def traits(builder, root):
    """glome_sb_scene_traits: tier, cls_mask, ..., pk_all, stack_cap, n_bih_nodes, ovf_cap, pk_generic_cap, n_mesh_nodes"""
    t = np.zeros(11, dtype=np.int64)
    assert L.load().glome_sb_scene_traits(builder.h, int(root), t.ctypes.data_as(C.POINTER(C.c_int64))) == 0, builder.lib.glome_sb_last_error(builder.h)
    return [int(x) for x in t]


def two_rows(builder, root, width, height, mode):
    """1 when a whole-frame launch of the scene takes the flagship instance / the two-row sampler (glome_kernel_choice over the commit's own traits)"""
    lib = L.load()
    P = api.render_params(width=width, height=height, mode=mode, maxdepth=2)
    items = lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)
    row = np.array([traits(builder, root)[:8] + [P.mode, P.faithful, P.count_work, P.maxdepth, P.tile_stride, items]], dtype=np.int64)
    out = np.zeros((1, 4), dtype=np.int32)
    assert lib.glome_kernel_choice(1, row.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == 1
    return int(out[0, 2])


def check_fixture(name, builder, root, tree_node):
    """each fixture still is what it is described as: a fixture that drifts would stop testing its case"""
    T = Tree(builder, tree_node)
    tr = traits(builder, root)
    widths = T.level_widths()
    leaf_sizes = sorted(T.nleaf[k] for k in T.leaves())
    if name == "three":
        assert T.n == 1 and leaf_sizes == [3]
    elif name == "mixed":
        assert T.n == 337 and leaf_sizes == [0] * 24 + [2] * 144 + [9], (T.n, leaf_sizes)
        assert len(T.items[0]) == 297 and 297 % 64
    elif name == "s3_20":
        assert len(T.items[0]) == 800
        assert (tr[0], tr[5], tr[6], tr[8]) == (0, 1, 12, 1), tr  # tier 0, pk_all, stack_cap 12, ovf_cap 1
        assert two_rows(builder, root, 131, 66, 0) == 1 and two_rows(builder, root, 131, 66, 1) == 1
    elif name == "wide":
        assert max(widths) > MERGE_BLOCK and widths[0] == 1, widths
        wide = [w > MERGE_BLOCK for w in widths]
        assert not wide[0] and not wide[-1]  # a launch of its own between the narrow levels below it and the merged run above it
    return T, tr
