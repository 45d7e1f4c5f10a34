"""The fp32 and indexed update calls on the GPU: glome_scene_bih_update_indexed / _f32, glome_scene_mesh_update_f32 and
glome_scene_sphere_bih_update_f32, each in its host and its _dev form.  The contract: a new call leaves the committed scene bit for bit as
the existing fp64 call leaves it when given the widened and gathered array.  fp32 -> fp64 is exact, so nothing here has a tolerance:
everything two scenes answer is compared bit for bit (NaNs as equal), with the helpers of the fp64 calls' own tests.  Poses are rounded
to fp32 and widened back (update_sources.r32) so that both calls see the same doubles; the tests stay away from fp32 subnormals, which
the library may read as zero.  What a reference scene answers is computed once per (fixture, pose) and shared."""
import numpy as np
import pytest

import bihs_refit as BR
import meshes_refit as MR
import nested_refit as NR
import spheres_refit as SR
import test_bih_update_gpu as TB
import test_mesh_update_gpu as TM
import test_nested_update_gpu as TN
import test_sphere_bih_update_gpu as TS
import update_sources as US
from helpers import product_camera_lights
from glome_amd import _lib as L
from glome_amd import api
from update_answers import assert_same

pytestmark = pytest.mark.gpu

_reference = {}


def torch_dev(*arrays):
    """the arrays as CUDA tensors of their own dtypes, complete before the context's stream reads them"""
    import torch
    out = [torch.tensor(np.ascontiguousarray(a), device=torch.device("cuda:0")) for a in arrays]
    torch.cuda.synchronize()
    return out


def sees(says):
    return (says["t"] >= 0).sum() >= 20 and (says["frame0"][..., 4] < 1e6).sum() >= 20


# ---- triangle bihs ----
def tri_pose(name, which):
    return US.r32(BR.triangles(name, which))


def tri_reference(ctx, name, which):
    """what scene B answers: a second commit of the same builder, updated through the existing fp64 call with the widened array"""
    key = ("tri", name, which)
    if key not in _reference:
        _, sc, tree, _, lights = TB.make(ctx, name)
        assert sc.bih_update(tree, tri_pose(name, which)) > 0
        _reference[key] = TB.answers(sc, api.camera(*MR.camera_for(which)), lights, which)
        sc.release()
    return _reference[key]


def tri_update(ctx, sc, tree, P, kind, form, decoys=True):
    """P through one of the new calls: kind = indexed64 / indexed32 / dense32, form = host / dev"""
    if kind == "dense32":
        arrays = (P.astype(np.float32),)
        call = sc.bih_update_f32
    else:
        verts, idx = US.pool(P, decoys)
        arrays = (verts.astype(np.float32) if kind == "indexed32" else verts, idx)
        assert arrays[0].astype(np.float64)[idx].reshape(-1, 9).tobytes() == P.tobytes()
        call = sc.bih_update_indexed
    if form == "dev":
        tensors = torch_dev(*arrays)
        assert call(tree, *tensors) is None
        assert sc.lib.glome_ctx_synchronize(ctx.h) == 0, ctx.err()
    else:
        assert call(tree, *arrays) > 0


TRI_CASES = [(n, "V1") for n in ("three", "mixed", "s3_20", "wide")] + [("mixed", "V2"), ("s3_20", "V2")]


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", ["indexed64", "indexed32", "dense32"])
@pytest.mark.parametrize("name,which", TRI_CASES)
def test_a_triangle_bih_update_equals_the_fp64_call_on_the_widened_gathered_array(gpu_ctx, name, which, kind, form):
    _, sc, tree, _, lights = TB.make(gpu_ctx, name)
    tri_update(gpu_ctx, sc, tree, tri_pose(name, which), kind, form)
    says = TB.answers(sc, api.camera(*MR.camera_for(which)), lights, which)
    sc.release()
    assert sees(says), "the rays and the frame must see the triangles"
    assert_same(says, tri_reference(gpu_ctx, name, which), f"{name} {which} through {kind}, {form} form")


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("name", ["mixed", "s3_20"])
def test_unreferenced_vertices_take_no_part(gpu_ctx, name, form):
    """the shuffled pool with a far vertex and a NaN vertex no item names, against the pool without them: a bound folded over the vertex
    array instead of over the items would differ (the far vertex) or raise the error word (the NaN)"""
    P = tri_pose(name, "V1")
    verts, idx = US.pool(P, decoys=True)
    assert np.isnan(verts).any() and np.nanmax(np.abs(verts)) >= 3.0e4
    says = []
    for decoys in (True, False):
        _, sc, tree, cam, lights = TB.make(gpu_ctx, name)
        tri_update(gpu_ctx, sc, tree, P, "indexed32", form, decoys)
        assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0
        says.append(TB.answers(sc, cam, lights, "V1"))
        sc.release()
    assert sees(says[0])
    assert_same(says[0], says[1], f"{name}: with and without decoys")
    assert_same(says[0], tri_reference(gpu_ctx, name, "V1"), f"{name}: with decoys")


@pytest.mark.parametrize("what", ["index_nv", "index_minus_one", "referenced_inf"])
def test_bad_input_is_found_on_the_device_and_a_valid_update_mends_the_scene(gpu_ctx, what):
    """An index outside [0, nv) and a referenced vertex that is not finite raise the updates' error word: the next synchronize returns
    GLOME_E_INVALID.  Neither is a fault: IndexedPts::load (update_common.hpp) replaces a bad index by 0 BEFORE it loads, and nv > 0 is
    checked on the host, so every load is inside the vertex array."""
    P = tri_pose("mixed", "V1")
    verts, idx = US.pool(P)
    v32, bad_idx = verts.astype(np.float32), idx.copy()
    if what == "index_nv":
        bad_idx[100, 1] = len(verts)
    elif what == "index_minus_one":
        bad_idx[296, 2] = -1
    else:
        v32[idx[40, 0], 1] = np.inf
    _, sc, tree, cam, lights = TB.make(gpu_ctx, "mixed")
    tv, ti = torch_dev(v32, bad_idx)
    assert sc.bih_update_indexed(tree, tv, ti) is None
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID
    assert "not finite" in gpu_ctx.err() and ("vertex index" in gpu_ctx.err()) and "glome_scene_bih_update_indexed_dev" in gpu_ctx.err()
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0  # (the word is cleared where it is read)
    tri_update(gpu_ctx, sc, tree, P, "indexed32", "dev")
    says = TB.answers(sc, cam, lights, "V1")
    sc.release()
    assert_same(says, tri_reference(gpu_ctx, "mixed", "V1"), f"a valid update after {what}")


def test_the_host_forms_refuse_before_anything_is_launched(gpu_ctx):
    P = tri_pose("mixed", "V1")
    verts, idx = US.pool(P)
    v32 = verts.astype(np.float32)
    nv, n = len(verts), len(idx)
    _, sc, tree, cam, lights = TB.make(gpu_ctx, "mixed")
    before = TB.frames(sc, cam, lights)
    bad = idx.copy(); bad[17, 1] = -1
    with pytest.raises(api.GlomeError, match=r"item 17 has vertex index -1.*status -1"):
        sc.bih_update_indexed(tree, v32, bad)
    bad = idx.copy(); bad[200, 2] = nv
    with pytest.raises(api.GlomeError, match=rf"item 200 has vertex index {nv}.*status -1"):
        sc.bih_update_indexed(tree, verts, bad)
    bad = idx.copy(); bad[5, 0] = int(np.flatnonzero(np.isnan(verts[:, 0]))[0])  # the NaN vertex, referenced now
    with pytest.raises(api.GlomeError, match=r"not finite.*status -1"):
        sc.bih_update_indexed(tree, v32, bad)
    with pytest.raises(api.GlomeError, match=rf"the bih has {n} items, not {n - 1}.*status -1"):
        sc.bih_update_indexed(tree, v32, idx[:-1])
    with pytest.raises(api.GlomeError, match=rf"the bih has {n} items, not {n - 1}.*status -1"):
        sc.bih_update_f32(tree, P[:-1])
    nan = P.copy(); nan[5, 2] = np.nan
    with pytest.raises(api.GlomeError, match=r"not finite.*status -1"):
        sc.bih_update_f32(tree, nan)
    lib, ip = sc.lib, idx.ctypes.data_as(L.c_ip)
    assert lib.glome_scene_bih_update_indexed(sc.h, tree, v32.ctypes.data, 1, 0, ip, n, None) == L.E_INVALID      # no vertices, n items
    assert lib.glome_scene_bih_update_indexed(sc.h, tree, v32.ctypes.data, 2, nv, ip, n, None) == L.E_INVALID     # no such dtype
    assert lib.glome_scene_bih_update_indexed(sc.h, tree, None, 1, nv, ip, n, None) == L.E_INVALID
    assert lib.glome_scene_bih_update_indexed(sc.h, tree, v32.ctypes.data, 1, nv, None, n, None) == L.E_INVALID
    # the _dev form refuses the same before it looks at a pointer (these are host pointers)
    assert lib.glome_scene_bih_update_indexed_dev(sc.h, tree, v32.ctypes.data, 1, 0, idx.ctypes.data, n) == L.E_INVALID
    assert lib.glome_scene_bih_update_indexed_dev(sc.h, tree, v32.ctypes.data, 1, nv, idx.ctypes.data, n - 1) == L.E_INVALID
    assert lib.glome_scene_bih_update_indexed_dev(sc.h, tree, v32.ctypes.data, 7, nv, idx.ctypes.data, n) == L.E_INVALID
    assert lib.glome_scene_bih_update_f32_dev(sc.h, tree, None, n) == L.E_INVALID
    import torch
    t64 = torch.zeros(9 * n, dtype=torch.float64, device="cuda:0")
    with pytest.raises(api.GlomeError, match=r"bih_update_f32: pts9 must be a contiguous CUDA torch.float32 tensor"):
        sc.bih_update_f32(tree, t64)
    with pytest.raises(api.GlomeError, match=r"bih_update: pts9 must be a contiguous CUDA torch.float64 tensor"):
        sc.bih_update(tree, t64.float())  # the existing call still refuses float32
    gpu_ctx.synchronize()
    assert_same(TB.frames(sc, cam, lights), before, "the refusals")
    sc.release()


def test_an_fp64_update_after_a_new_form_update_still_equals_its_commit(gpu_ctx):
    """the forms of one object share its workspace and tables: the old path is left as it was"""
    b, sc, tree, _, lights = TB.make(gpu_ctx, "mixed")
    tri_update(gpu_ctx, sc, tree, tri_pose("mixed", "V1"), "indexed32", "dev")
    tri_update(gpu_ctx, sc, tree, tri_pose("mixed", "V1"), "dense32", "host")
    P2 = BR.triangles("mixed", "V2")  # (not rounded: the fp64 call's own pose)
    assert sc.bih_update(tree, P2) > 0
    cam = api.camera(*MR.camera_for("V2"))
    says = TB.answers(sc, cam, lights, "V2")
    sc.release()
    b2, root2, tree2, _, _ = TB.build("mixed")
    b2.bih_set_triangles(tree2, P2)
    ref = gpu_ctx.commit(b2, root2)
    want = TB.answers(ref, cam, lights, "V2")
    ref.release()
    assert sees(says)
    assert_same(says, want, "fp64 V2 after the new forms' V1")


# ---- meshes ----
def mesh_pose(mesh, which):
    V, n = MR.arrays(mesh, which)
    return US.r32(V), US.r32(n)


def mesh_reference(ctx, mesh, which):
    key = ("mesh", mesh, which)
    if key not in _reference:
        _, sc, me, _, lights = TM.make(ctx, mesh)
        V, n = mesh_pose(mesh, which)
        assert sc.mesh_update(me, V, n) > 0
        _reference[key] = TM.answers(sc, api.camera(*MR.camera_for(which)), lights, which)
        sc.release()
    return _reference[key]


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("mesh,which", [("mixed", "V1"), ("mixed", "V2"), ("one", "V1"), ("s3", "V1")])  # (mixed: with normals and an unreferenced vertex)
def test_a_mesh_update_from_fp32_equals_the_fp64_call_on_the_widened_arrays(gpu_ctx, mesh, which, form):
    _, sc, me, _, lights = TM.make(gpu_ctx, mesh)
    V, n = mesh_pose(mesh, which)
    assert (len(n) > 0) == (mesh == "mixed")
    V32, n32 = V.astype(np.float32), n.astype(np.float32)
    if form == "dev":
        tensors = torch_dev(V32, n32) if len(n32) else torch_dev(V32) + [None]
        assert sc.mesh_update_f32(me, *tensors) is None
        assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0, gpu_ctx.err()
    else:
        assert sc.mesh_update_f32(me, V32, n32 if len(n32) else None) > 0
    says = TM.answers(sc, api.camera(*MR.camera_for(which)), lights, which)
    sc.release()
    assert sees(says), "the rays and the frame must see the mesh"
    assert_same(says, mesh_reference(gpu_ctx, mesh, which), f"mesh {mesh} {which}, {form} form")


# ---- sphere bihs ----
def sphere_reference(ctx, name, which):
    key = ("sph", name, which)
    if key not in _reference:
        B = SR.build(name)
        sc = ctx.commit(B.b, B.root)
        assert sc.sphere_bih_update(B.tree, US.r32(SR.spheres(name, which))) > 0
        cam, lights = TS.cam_lights(B, which)
        _reference[key] = TS.answers(sc, cam, lights, which)
        sc.release()
    return _reference[key]


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("name,which", [("three", "V1"), ("cluster", "V1"), ("cloud", "V1"), ("cloud", "V2")])
def test_a_sphere_bih_update_from_two_fp32_streams_equals_the_fp64_call(gpu_ctx, name, which, form):
    A = SR.build(name)
    sc = gpu_ctx.commit(A.b, A.root)
    cam, lights = TS.cam_lights(A, which)
    S = SR.spheres(name, which).astype(np.float32)
    centres, radii = np.ascontiguousarray(S[:, :3]), np.ascontiguousarray(S[:, 3])
    if form == "dev":
        assert sc.sphere_bih_update_f32(A.tree, *torch_dev(centres, radii)) is None
        assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0, gpu_ctx.err()
    else:
        assert sc.sphere_bih_update_f32(A.tree, centres, radii) > 0
    says = TS.answers(sc, cam, lights, which)
    rays, pixels = SR.sees_spheres(sc, A, which, cam, TS.W, TS.H)
    sc.release()
    assert rays >= 20 and pixels >= 20, "the rays and the frame must see the spheres"
    assert_same(says, sphere_reference(gpu_ctx, name, which), f"spheres {name} {which}, {form} form")


def test_a_bad_sphere_through_the_fp32_forms(gpu_ctx):
    A = SR.build("cluster")
    sc = gpu_ctx.commit(A.b, A.root)
    cam, lights = TS.cam_lights(A)
    S = SR.spheres("cluster", "V1").astype(np.float32)
    centres, radii = np.ascontiguousarray(S[:, :3]), np.ascontiguousarray(S[:, 3])
    before = TS.frames(sc, cam, lights)
    zero = radii.copy(); zero[7] = 0.0
    with pytest.raises(api.GlomeError, match=r"radius of item 7 is not positive.*status -1"):
        sc.sphere_bih_update_f32(A.tree, centres, zero)
    inf = centres.copy(); inf[3, 1] = np.inf
    with pytest.raises(api.GlomeError, match=r"not finite.*status -1"):
        sc.sphere_bih_update_f32(A.tree, inf, radii)
    with pytest.raises(api.GlomeError, match=r"the bih has 40 items, not 39.*status -1"):
        sc.sphere_bih_update_f32(A.tree, centres[:-1], radii[:-1])
    assert sc.lib.glome_scene_sphere_bih_update_f32_dev(sc.h, A.tree, centres.ctypes.data, None, len(radii)) == L.E_INVALID
    assert_same(TS.frames(sc, cam, lights), before, "the refusals")
    assert sc.sphere_bih_update_f32(A.tree, *torch_dev(centres, zero)) is None  # found on the device
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID and "radius that is not positive" in gpu_ctx.err()
    assert sc.sphere_bih_update_f32(A.tree, *torch_dev(centres, radii)) is None
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0
    says = TS.answers(sc, cam, lights, "V1")
    sc.release()
    assert_same(says, sphere_reference(gpu_ctx, "cluster", "V1"), "a valid update after a refused one")


# ---- under bihs: the same fp64 bound in the bounds table, the same trees stale ----
def nested_new_form(sc, call, dev):
    """one of nested_refit's calls through the new forms: a triangle bih indexed from fp32, a mesh from fp32"""
    kind, node, data, _ = call
    if kind == "bih":
        verts, idx = US.pool(data)
        arrays, fn = (verts.astype(np.float32), idx), sc.bih_update_indexed
    else:
        arrays, fn = (data.astype(np.float32),), sc.mesh_update_f32
    if dev:
        assert fn(node, *torch_dev(*arrays)) is None
    else:
        assert fn(node, *arrays) > 0


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("name", ["nff_like", "mesh_shared"])  # triangle bihs under a bih; a mesh under a bih, direct and instanced
def test_under_bihs_the_new_forms_do_what_the_fp64_forms_do(gpu_ctx, name, dev):
    A = NR.get(name)
    cam, lights = product_camera_lights(A.sd)
    center = (0.0, 1.5, 0.0)
    calls = [(kind, node, US.r32(data), k) for kind, node, data, k in NR.moves(A, "grow")]
    assert calls and all(c[0] in ("bih", "mesh") for c in calls)
    says, stale = [], []
    for new_form in (True, False):
        B = NR.get(name)
        sc = gpu_ctx.commit(B.b, B.root)
        sc.nested_updates(True)
        before = TN.answers(sc, cam, lights, center)
        marks = []
        for call in calls:
            if new_form:
                nested_new_form(sc, call, dev)
            else:
                assert NR.apply_scene(sc, call) > 0
            marks.append(sc.stale_bihs())
            assert set(sc.bihs_above(NR.node_of(call))) <= set(marks[-1]) and marks[-1]
            sc.refit_above(NR.node_of(call), dev=dev)
            assert sc.stale_bihs() == []
        assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0, gpu_ctx.err()
        says.append(TN.answers(sc, cam, lights, center))
        stale.append(marks)
        assert not np.array_equal(says[-1]["frame0"], before["frame0"]), "the update must show"
        sc.release()
    assert stale[0] == stale[1]
    assert sees(says[0]), "the rays and the frame must see the scene"
    assert_same(says[0], says[1], f"{name}: new forms against fp64 forms, refitted")
