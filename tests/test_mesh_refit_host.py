"""glome_sb_mesh_set_vertices: same tree, new vertices, on the host builder (no GPU).  This call is the specification the device
path (glome_scene_mesh_update, test_mesh_update_gpu.py) is held against; here it is held against NumPy and the fp64 oracle."""
import numpy as np
import pytest

import meshes_refit as MR
import parity
import showfmt
from helpers import HostSim, product_camera_lights
from glome_amd import _lib as L
from glome_amd import api

DELTA = 1e-4  # kDelta, Vec.hs:40


def build(mesh, which="V0", wrap="root"):
    sd, me = MR.scene_desc(mesh, which, wrap)
    b = api.Builder()
    nm, _ = sd.replay(b)
    return sd, b, nm, nm[me]


def mesh_of(text):
    v = showfmt.parse(text)
    assert v[0] == "SI" and v[1][0] == "Mesh"
    return v[1]


def shape(bvh):
    """the tree without its boxes: leaf lists and nesting"""
    return ("Leaf", tuple(bvh[1])) if bvh[0] == "Leaf" else ("Branch", shape(bvh[3]), shape(bvh[4]))


def box(bb):
    assert bb[0] == "Bbox"
    return np.array(bb[1][1:] + bb[2][1:], dtype=np.float64)


def tris_below(bvh):
    return list(bvh[1]) if bvh[0] == "Leaf" else tris_below(bvh[3]) + tris_below(bvh[4])


def box_over(V, idx):
    """min / max of v -+ delta over vertices idx, in float64: box_of_points"""
    p = V[np.asarray(idx, dtype=np.int64)]
    return np.concatenate([(p - DELTA).min(axis=0), (p + DELTA).max(axis=0)])


def check_boxes(bvh, V, tris):
    """every branch box equals, exactly, the box over the vertices of the triangles below it; returns the number of branches"""
    if bvh[0] == "Leaf":
        return 0
    for bb, child in ((bvh[1], bvh[3]), (bvh[2], bvh[4])):
        below = tris_below(child)
        assert below, "the test meshes have no empty leaf"
        want = box_over(V, tris[below, :3].ravel())
        assert np.array_equal(box(bb), want), (box(bb), want)
    return 1 + check_boxes(bvh[3], V, tris) + check_boxes(bvh[4], V, tris)


@pytest.mark.parametrize("mesh", sorted(MR.MESHES))
def test_same_vertices_change_nothing(built, mesh):
    sd, b, nm, me = build(mesh)
    before = b.show(me), b.bound(me).tolist(), b.primcount(me)
    V0, n0 = MR.arrays(mesh, "V0")
    b.mesh_set_vertices(me, V0, n0)
    assert (b.show(me), b.bound(me).tolist(), b.primcount(me)) == before


def test_the_mixed_mesh_has_a_saturated_leaf(built):
    """a leaf of 15 or more triangles: the count of its reference saturates, the true one is read from mtrimeta"""
    sd, b, nm, me = build("mixed")
    sizes = MR.leaf_sizes(mesh_of(b.show(me))[4])
    assert max(sizes) >= 15 and len(sizes) > 64, sizes


@pytest.mark.parametrize("mesh", sorted(MR.MESHES))
def test_refit_boxes_are_the_unions_of_the_new_vertices(built, mesh):
    sd, b, nm, me = build(mesh)
    orig, count = mesh_of(b.show(me)), b.primcount(me)
    V1, n1 = MR.arrays(mesh, "V1")
    tris = MR.MESHES[mesh]()[2]
    b.mesh_set_vertices(me, V1, n1)
    got = mesh_of(b.show(me))
    assert shape(got[4]) == shape(orig[4])  # leaf lists and tree shape
    assert got[2] == orig[2]                # the triangles
    assert np.array_equal(np.array([v[1:] for v in got[1]], dtype=np.float64), V1)  # the vertices, digit for digit
    nb = check_boxes(got[4], V1, tris)
    assert nb == (0 if mesh == "one" else len(MR.leaf_sizes(got[4])) - 1)
    assert np.array_equal(box(got[3]), box_over(V1, np.arange(len(V1))))  # over ALL vertices, the unreferenced one included
    if mesh == "mixed":
        assert box(got[3])[3] > V1[:-1, 0].max() + 1, "the unreferenced vertex must widen the mesh's box"
    # bound: that of a mesh built fresh from V1
    _, b1, _, me1 = build(mesh, "V1")
    assert np.array_equal(b.bound(me), b1.bound(me1))
    assert b.primcount(me) == count


def test_an_empty_leaf_keeps_the_empty_box(built):
    """a tree read from a `show` text may hold an empty leaf: its box is box_empty, what MeshBuild::join gives for no triangle"""
    b = api.Builder()
    me, V0 = MR.holed_builder(b)
    V1 = MR.deform(V0, "V1")[0]
    b.mesh_set_vertices(me, V1)
    got = mesh_of(b.show(me))
    assert got[4][0] == "Branch" and got[4][3] == ("Leaf", [])
    assert box(got[4][1]).tolist() == [1e6] * 3 + [-1e6] * 3
    assert np.array_equal(box(got[4][2]), box_over(V1, np.arange(len(V1))))  # (every vertex of this mesh is referenced)
    HostSim(b, me)  # and it flattens


def test_there_and_back_gives_the_original_text(built):
    sd, b, nm, me = build("mixed")
    orig = b.show(me)
    b.mesh_set_vertices(me, *MR.arrays("mixed", "V1"))
    assert b.show(me) != orig
    b.mesh_set_vertices(me, *MR.arrays("mixed", "V0"))
    assert b.show(me) == orig


@pytest.mark.parametrize("which", ["V1", "V2"])
def test_refitted_builder_against_the_oracle(built, which):
    """the refitted mesh through the host-compiled device code, against the fp64 oracle loaded with a description made from the new vertices"""
    sd0, b, nm, me = build("mixed")
    b.mesh_set_vertices(me, *MR.arrays("mixed", which))
    sd, _ = MR.scene_desc("mixed", which)  # (same op list as sd0: nm maps its ids too)
    hs = HostSim(b, nm[sd.root])
    parity.check_rays(lambda o, d: hs.rayint(o, d), lambda o, d, t: hs.shadow(o, d, t), hs.inside, sd, nm, n=6000)
    cam, lights = product_camera_lights(sd)
    img, cnt = hs.render(cam, lights, 96, 54, 2)
    parity.check_image(img, [int(x) for x in cnt], sd, 96, 54, 2)


def test_refusals_leave_the_mesh_untouched(built):
    sd, b, nm, me = build("mixed", wrap="tex")
    V1, n1 = MR.arrays("mixed", "V1")
    orig = b.show(me)
    nan = V1.copy(); nan[17, 1] = np.nan
    inf_n = n1.copy(); inf_n[3, 0] = np.inf
    for args, what in (((me, V1[:-1], n1), "wrong nv"), ((me, V1, n1[:-1]), "wrong nn"), ((me, V1, None), "no normals"), ((me, nan, n1), "a NaN"),
                       ((me, V1, inf_n), "an infinite normal"), ((nm[sd.root], V1, n1), "a Tex node"), ((10 ** 6, V1, n1), "no such node")):
        with pytest.raises(api.GlomeError, match=r"status -1"):
            b.mesh_set_vertices(*args)
        assert b.show(me) == orig, what
    # NULL norms with nn > 0, which the Python wrapper cannot express
    lib = L.load()
    v = np.ascontiguousarray(V1)
    assert lib.glome_sb_mesh_set_vertices(b.h, me, v.ctypes.data_as(L.c_dp), len(v), None, len(n1)) == L.E_INVALID
    assert b"normal" in lib.glome_sb_last_error(b.h) and b.show(me) == orig
    b.mesh_set_vertices(me, V1, n1)  # and the valid call still works
    assert b.show(me) != orig
