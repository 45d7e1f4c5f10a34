"""The meshes, deformations and scene descriptions of the mesh refit tests (test_mesh_refit_host.py, test_mesh_update_gpu.py) -- test
infrastructure.  Vertices are float64 throughout (SceneDesc(round32=False)): the update's arithmetic is fp64 and is held to the bit."""
import numpy as np

from glome_amd import scenes
from glome_amd.scene import SceneDesc

FAR_VERTEX = (14.0, 9.0, -13.0)  # referenced by no triangle: it moves the mesh's own box and nothing else


def _grid_tris(N, first=0):
    idx = first + np.arange((N + 1) * (N + 1)).reshape(N + 1, N + 1)
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    return np.stack([np.stack([a, b, c], -1), np.stack([c, b, d], -1)], axis=2).reshape(-1, 3)


def mixed_mesh():
    """(verts, norms, tris): scenes.heightfield_vertices(12) -- 288 triangles, several tree levels, no multiple of 64 --, a pile of 20
    large, nearly coincident triangles that build_tree cannot split (a leaf whose count saturates the reference's four bits), one
    vertex no triangle refers to, vertex normals on every other heightfield triangle and none elsewhere, two textures."""
    N = 12
    hf = scenes.heightfield_vertices(N).reshape(-1, 3)
    pile = []
    for k in range(20):
        y = 2.5 + 1e-3 * k
        pile += [(-9.0 + 1e-3 * k, y, -9.0), (9.0, y, -9.0 - 1e-3 * k), (0.0, y + 5e-4 * k, 9.0)]
    V = np.concatenate([hf, np.array(pile), np.array([FAR_VERTEX])])
    ht = _grid_tris(N)
    pt = len(hf) + np.arange(60).reshape(20, 3)
    tris = np.full((len(ht) + 20, 8), -1, dtype=np.int32)
    tris[:len(ht), :3] = ht
    tris[len(ht):, :3] = pt
    tris[:, 6] = np.arange(len(tris)) % 2
    # one normal per heightfield vertex (leaning with the vertex's position, unit length)
    n = np.stack([0.2 * np.sin(hf[:, 0]), np.ones(len(hf)), 0.2 * np.cos(hf[:, 2])], 1)
    norms = n / np.linalg.norm(n, axis=1, keepdims=True)
    with_n = np.arange(len(ht))[::2]
    tris[with_n, 3:6] = ht[with_n]
    return V, norms, tris


def one_triangle_mesh():
    """a mesh whose root is a leaf: no branch node, so no level launch"""
    V = np.array([(-3.0, 0.5, -1.0), (3.5, 0.25, -2.0), (0.5, 4.0, 1.5)])
    tris = np.full((1, 8), -1, dtype=np.int32)
    tris[0, :3] = (0, 1, 2)
    tris[0, 6] = 0
    return V, np.zeros((0, 3)), tris


def s3_mesh():
    """the vertex arrays of scenes.s3(24, as_mesh=True): 1,152 triangles"""
    N = 24
    V = scenes.heightfield_vertices(N).reshape(-1, 3)
    tris = np.full((2 * N * N, 8), -1, dtype=np.int32)
    tris[:, :3] = _grid_tris(N)
    tris[:, 6] = 0
    return V, np.zeros((0, 3)), tris


MESHES = {"mixed": mixed_mesh, "one": one_triangle_mesh, "s3": s3_mesh}
V2_SCALE, V2_SHIFT = 3.0, np.array([40.0, 6.0, -30.0])


def deform(V0, which, norms0=None):
    """V1: a smooth displacement of a few tenths plus per-vertex jitter.  V2: V0 scaled by 3 and translated -- the box's centre moves
    by more than the box's diagonal.  The normals (when given) are turned a little and renormalised for V1, kept for V2."""
    if which == "V0":
        V, n = V0.copy(), norms0
    elif which == "V1":
        rng = np.random.default_rng(7)
        d = np.stack([0.25 * np.sin(0.7 * V0[:, 2] + 0.3), 0.3 * np.sin(0.5 * V0[:, 0]) * np.cos(0.4 * V0[:, 2]), 0.2 * np.cos(0.6 * V0[:, 0])], 1)
        V = V0 + d + rng.uniform(-0.02, 0.02, V0.shape)
        n = norms0
        if norms0 is not None and len(norms0):
            n = norms0 + 0.1 * np.stack([np.cos(V0[:len(norms0), 2]), np.zeros(len(norms0)), np.sin(V0[:len(norms0), 0])], 1)
            n = n / np.linalg.norm(n, axis=1, keepdims=True)
    elif which == "V2":
        V, n = V0 * V2_SCALE + V2_SHIFT, norms0
    else:
        raise KeyError(which)
    return V, (np.zeros((0, 3)) if n is None else n)


def camera_for(which):
    """the camera follows V2's similarity, so its frame shows what V0's shows"""
    pos, at, up, angle = scenes.CUST_CAM
    if which == "V2":
        pos = tuple(np.array(pos) * V2_SCALE + V2_SHIFT)
        at = tuple(np.array(at) * V2_SCALE + V2_SHIFT)
    return pos, at, up, angle


WRAPS = ("root", "tex", "instances", "bound")


def scene_desc(mesh, which="V0", wrap="root"):
    """A SceneDesc of mesh `mesh` with vertices `which`, and the SceneDesc id of the mesh node.
      root       the mesh is the scene
      tex        under a Tex
      instances  two Instances of the one mesh node
      bound      the second operand of a Bound whose bounding solid is a large sphere"""
    from glome_amd import api
    V0, n0, tris = MESHES[mesh]()
    V, n = deform(V0, which, n0)
    sd = SceneDesc(round32=False)
    mats = [scenes.matte(sd, (0.8, 0.5, 0.4)), sd.material_surface((0.2, 0.4, 1.0), 1, 0.2, 0.8, 0.4, 10)]
    me = sd.mesh(V, n, tris, mats)
    if wrap == "root":
        root = me
    elif wrap == "tex":
        root = sd.tex(me, sd.material_surface((0.1, 0.9, 0.2), 1, 0.2, 0.8, 0.4, 10))
    elif wrap == "instances":
        root = sd.group([sd.transform(me, [api.translate((-4.0, 0.0, 0.0))]), sd.transform(me, [api.rotate((0.0, 1.0, 0.0), 0.5), api.translate((5.0, 1.0, -3.0))])])
    elif wrap == "bound":
        root = sd.bound_object(sd.sphere((0.0, 0.0, 0.0), 400.0), me)
    else:
        raise KeyError(wrap)
    sd.set_root(root)
    for pos, col in scenes.LIGHTS[:2]:
        sd.add_light(pos, col)
    sd.set_camera(*camera_for(which))
    return sd, me


def holed_builder(builder, which="V0"):
    """The one mesh here that only a `show` text can make: s3(4)'s 32 triangles under a root whose LEFT child is an empty leaf (build_tree
    never leaves one; a tree read with load_show may).  Returns (mesh node, V0): the text is the builder's own dump of the mesh with the
    BVH wrapped, read back with load_show and given vertices `which`."""
    N = 4
    V0 = scenes.heightfield_vertices(N).reshape(-1, 3)
    tris = np.full((2 * N * N, 8), -1, dtype=np.int32)
    tris[:, :3] = _grid_tris(N)
    tris[:, 6] = 0
    mat = builder.material_surface((0.8, 0.5, 0.4), 1, 0.2, 1, 0, 0)
    text = builder.show(builder.mesh(V0, np.zeros((0, 3)), tris, [mat]))
    at = text.index("] Bbox {") + 2
    cut = text.index("}", at) + 1
    bbox, bvh = text[at:cut], text[cut + 1:]
    empty = "Bbox {p1 = Vec 1000000.0 1000000.0 1000000.0, p2 = Vec (-1000000.0) (-1000000.0) (-1000000.0)}"
    me, _ = builder.load_show(text[:cut] + " Branch (" + empty + ") (" + bbox + ") (Leaf []) (" + bvh + ")", default_material=mat)
    builder.mesh_set_vertices(me, deform(V0, which)[0])
    return me, V0


def arrays(mesh, which):
    V0, n0, _ = MESHES[mesh]()
    return deform(V0, which, n0)


def leaf_sizes(bvh):
    """sizes of the leaves of a parsed `show` BVH (showfmt.parse), preorder"""
    if bvh[0] == "Leaf":
        return [len(bvh[1])]
    return leaf_sizes(bvh[3]) + leaf_sizes(bvh[4])
