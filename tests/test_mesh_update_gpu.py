"""glome_scene_mesh_update: new vertices for a committed Mesh, its BVH refitted on the GPU.  The contract: after an update the committed
scene is bit for bit the scene a commit after glome_sb_mesh_set_vertices (test_mesh_refit_host.py) would have made -- so everything the
two scenes answer is compared bit for bit (NaNs as equal), and the updated scene is held against the fp64 oracle besides."""
import ctypes as C

import numpy as np
import pytest

import meshes_refit as MR
import parity
import update_answers as UA
from helpers import product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api
from update_answers import assert_same, frames

pytestmark = pytest.mark.gpu

W, H = UA.SIZE


def build(mesh, which="V0", wrap="root"):
    """(builder, root, mesh node, cam, lights) of mesh `mesh` built with vertices `which`"""
    if mesh == "holed":
        b = api.Builder()
        me, _ = MR.holed_builder(b, which)
        sd, _ = MR.scene_desc("one", which)
        root = me
    else:
        sd, m = MR.scene_desc(mesh, which, wrap)
        b = api.Builder()
        nm, _ = sd.replay(b)
        me, root = nm[m], nm[sd.root]
    cam, lights = product_camera_lights(sd)
    return b, root, me, cam, lights


def make(ctx, mesh, which="V0", wrap="root"):
    """the same, committed: (builder, scene, mesh node, cam, lights)"""
    b, root, me, cam, lights = build(mesh, which, wrap)
    return b, ctx.commit(b, root), me, cam, lights


def new_arrays(mesh, which):
    if mesh == "holed":
        return MR.deform(MR.holed_builder(api.Builder())[1], which)
    return MR.arrays(mesh, which)


def answers(sc, cam, lights, which):
    """update_answers.answers on the pose's rays"""
    k = MR.V2_SCALE if which == "V2" else 1.0
    shift = MR.V2_SHIFT if which == "V2" else np.zeros(3)
    rays = random_rays(4000, 23, center=tuple(np.array((0, 1.5, 0)) * k + shift), radius=13 * k, spread=7 * k)
    return UA.answers(sc, cam, lights, rays, k, shift)


CASES = [(m, "root", w) for m in ("mixed", "one", "s3") for w in ("V1", "V2")] + [("holed", "root", "V1")] + [("mixed", wrap, "V1") for wrap in ("tex", "instances", "bound")]


@pytest.mark.parametrize("mesh,wrap,which", CASES)
def test_update_equals_the_commit_of_the_refitted_builder(gpu_ctx, mesh, wrap, which):
    _, a, me, cam, lights = make(gpu_ctx, mesh, "V0", wrap)
    V, n = new_arrays(mesh, which)
    ms = a.mesh_update(me, V, n)
    assert ms > 0
    a_says = answers(a, cam, lights, which)
    a.release()
    # scene B: the builder refitted first, then committed
    b, root, me_b, _, _ = build(mesh, "V0", wrap)
    b.mesh_set_vertices(me_b, V, n)
    sc_b = gpu_ctx.commit(b, root)
    b_says = answers(sc_b, cam, lights, which)
    sc_b.release()
    assert (a_says["t"] >= 0).sum() >= 20 and (a_says["frame0"][..., 4] < 1e6).sum() >= 20, "the rays and the frame must see the mesh"
    assert_same(a_says, b_says, f"{mesh} under {wrap}, {which}")


def test_there_and_back_renders_the_never_updated_frame(gpu_ctx):
    _, sc, me, cam, lights = make(gpu_ctx, "mixed")
    before = frames(sc, cam, lights)
    sc.mesh_update(me, *MR.arrays("mixed", "V1"))
    moved = frames(sc, cam, lights)
    assert not np.array_equal(moved["frame0"], before["frame0"])
    sc.mesh_update(me, *MR.arrays("mixed", "V0"))
    assert_same(frames(sc, cam, lights), before, "V0 -> V1 -> V0")
    sc.release()


@pytest.mark.parametrize("which", ["V1", "V2"])
def test_updated_scene_against_the_oracle(gpu_ctx, which):
    sd0, m = MR.scene_desc("mixed")
    b = api.Builder()
    nm, _ = sd0.replay(b)
    sc = gpu_ctx.commit(b, nm[sd0.root])
    sc.mesh_update(nm[m], *MR.arrays("mixed", which))
    sd, _ = MR.scene_desc("mixed", which)  # what the oracle is loaded with: a description made from the new vertices
    parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, sd, nm, n=20000)
    cam, lights = product_camera_lights(sd)
    img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=2))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, W, H, 2)
    sc.release()


def test_device_form_is_ordered_by_the_stream(gpu_ctx):
    """three updates from CUDA tensors, each followed by a render into a buffer of its own, nothing synchronised in between"""
    import torch
    cam = api.camera((-30.0, 40.0, 60.0), (25.0, 4.0, -20.0), (0.0, 1.0, 0.0), 60.0)  # sees the mesh at V0, V1 and V2
    _, sc, me, _, lights = make(gpu_ctx, "mixed")
    P = api.render_params(width=W, height=H, maxdepth=2)
    dev = torch.device("cuda:0")
    order = ("V1", "V2", "V0")
    tensors = [[torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev) for x in MR.arrays("mixed", w)] for w in order]
    bufs = [torch.zeros(H * W * 5, dtype=torch.float32, device=dev) for _ in order]
    sc.render_dev(cam, lights, P, bufs[0].data_ptr(), want_stats=False)  # (the frame size's tables are made at its first render, which waits for them)
    gpu_ctx.synchronize()
    bufs[0].zero_()
    torch.cuda.synchronize()
    for (v, n), out in zip(tensors, bufs):
        assert sc.mesh_update(me, v, n) is None
        sc.render_dev(cam, lights, P, out.data_ptr(), want_stats=False)
    gpu_ctx.synchronize()
    got = [o.cpu().numpy().reshape(H, W, 5) for o in bufs]
    sc.release()
    for w, img in zip(order, got):
        _, ref, me_r, _, _ = make(gpu_ctx, "mixed")
        ref.mesh_update(me_r, *MR.arrays("mixed", w))  # the host form
        want, _, _ = ref.render(cam, lights, P, want_packed=False)
        ref.release()
        assert (want[..., 4] < 1e6).mean() > 0.01, w
        assert np.array_equal(img, want, equal_nan=True), w
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])


def test_refusals_leave_the_scene_as_it_was(gpu_ctx):
    V1, n1 = MR.arrays("mixed", "V1")
    # a mesh that is an item of a bih: the tree's planes and root box were built from the mesh's bound
    sd, m = MR.scene_desc("mixed")
    b = api.Builder()
    nm, _ = sd.replay(b)
    ball = b.sphere((0.0, 6.0, 0.0), 1.0)
    tree = b.bih([nm[m], ball])
    cam, lights = product_camera_lights(sd)
    sc = gpu_ctx.commit(b, tree)
    before = frames(sc, cam, lights)
    with pytest.raises(api.GlomeError, match=rf"inside bih {tree}.*status -1"):
        sc.mesh_update(nm[m], V1, n1)
    assert_same(frames(sc, cam, lights), before, "a mesh under a bih")
    sc.release()
    # the same mesh, also reachable past the bih: still refused (any path)
    sc = gpu_ctx.commit(b, b.group([tree, nm[m]]))
    with pytest.raises(api.GlomeError, match=r"inside bih"):
        sc.mesh_update(nm[m], V1, n1)
    sc.release()
    # wrong counts, an id of another kind, an id of no node: refused by both forms
    root = b.group([nm[m], ball])
    sc = gpu_ctx.commit(b, root)
    before = frames(sc, cam, lights)
    for args, what in (((nm[m], V1[:-1], n1), "wrong nv"), ((nm[m], V1, n1[:-1]), "wrong nn"), ((nm[m], V1, None), "no normals"), ((ball, V1, n1), "a sphere"),
                       ((root, V1, n1), "a list"), ((10 ** 6, V1, n1), "no such node")):
        with pytest.raises(api.GlomeError, match=r"status -1"):
            sc.mesh_update(*args)
        assert_same(frames(sc, cam, lights), before, what)
    nan = V1.copy(); nan[5, 2] = np.nan
    with pytest.raises(api.GlomeError, match=r"not finite.*status -1"):
        sc.mesh_update(nm[m], nan, n1)  # the host form checks on the host
    assert_same(frames(sc, cam, lights), before, "a NaN through the host form")
    v = np.ascontiguousarray(V1)
    assert sc.lib.glome_scene_mesh_update_dev(sc.h, nm[m], C.c_void_p(v.ctypes.data), len(v) - 1, None, len(n1)) == L.E_INVALID  # (refused before the pointer is looked at)
    assert sc.lib.glome_scene_mesh_update_dev(sc.h, nm[m], C.c_void_p(v.ctypes.data), len(v), None, len(n1)) == L.E_INVALID
    gpu_ctx.synchronize()
    assert_same(frames(sc, cam, lights), before, "the device form's refusals")
    sc.release()


def test_a_vertex_that_is_not_finite_is_reported_at_the_next_synchronize(gpu_ctx):
    import torch
    _, sc, me, cam, lights = make(gpu_ctx, "mixed")
    V1, n1 = MR.arrays("mixed", "V1")
    dev = torch.device("cuda:0")
    bad = V1.copy(); bad[100, 0] = np.nan
    tb, tv, tn = (torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev) for x in (bad, V1, n1))
    torch.cuda.synchronize()
    sc.mesh_update(me, tb, tn)
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID
    assert "not finite" in gpu_ctx.err()
    sc.mesh_update(me, tv, tn)  # a valid update: the scene is specified again
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0
    got = frames(sc, cam, lights)
    sc.release()
    _, ref, me_r, _, _ = make(gpu_ctx, "mixed")
    ref.mesh_update(me_r, V1, n1)
    assert_same(got, frames(ref, cam, lights), "a valid update after a refused one")
    ref.release()
