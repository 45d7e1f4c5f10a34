"""glome_scene_bih_update: new triangles for a committed triangle bih, its planes refitted on the GPU.  The contract: after an update the
committed scene is bit for bit the scene a commit after glome_sb_bih_set_triangles (test_bih_refit_host.py) would have made -- so
everything the two scenes answer is compared bit for bit (NaNs as equal), and the updated scene is held against the fp64 oracle besides.
One thing is left out, in the one case where it was seen to matter: the normal of a ray that MISSES a scene whose root is a Bound.  A miss
has no normal (glome_hip.h); what the call stores there is whatever the traversal left behind, and under a Bound it differs between two
commits of one and the same builder, no update involved (measured on `mixed` under the Bound: 273 of 1,183 misses, no hit among them;
DESIGN.md 4.7).  Everywhere else the normals are compared raw, misses included."""
import ctypes as C

import numpy as np
import pytest

import bihs_refit as BR
import meshes_refit as MR
import parity
import update_answers as UA
from helpers import product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api
from update_answers import assert_same, frames

pytestmark = pytest.mark.gpu

W, H = UA.SIZE


def build(name, which="V0", wrap="tex"):
    """(builder, root, bih node, cam, lights) of bih `name` built with triangles `which`"""
    sd, b, nm, tree = BR.build(name, which, wrap)
    cam, lights = product_camera_lights(sd)
    return b, nm[sd.root], tree, cam, lights


def make(ctx, name, which="V0", wrap="tex"):
    """the same, committed: (builder, scene, bih node, cam, lights)"""
    b, root, tree, cam, lights = build(name, which, wrap)
    return b, ctx.commit(b, root), tree, cam, lights


def answers(sc, cam, lights, which, hits_only_normals=False):
    """update_answers.answers on the pose's rays (hits_only_normals: the Bound case, see the top of the file)"""
    k = MR.V2_SCALE if which == "V2" else 1.0
    shift = MR.V2_SHIFT if which == "V2" else np.zeros(3)
    rays = random_rays(4000, 23, center=tuple(np.array((0, 1.5, 0)) * k + shift), radius=13 * k, spread=7 * k)
    return UA.answers(sc, cam, lights, rays, k, shift, hits_only_normals)


CASES = [(n, "tex", w) for n in ("three", "mixed", "s3_20", "wide") for w in ("V1", "V2")] + [("mixed", wrap, "V1") for wrap in ("root", "instances", "bound")]


@pytest.mark.parametrize("merged", [False, True], ids=["per_level", "merged"])
@pytest.mark.parametrize("name,wrap,which", CASES)
def test_update_equals_the_commit_of_the_refitted_builder(gpu_ctx, monkeypatch, name, wrap, which, merged):
    """both forms of the level pass: a launch per level (the default), and every run of narrow levels in one single-block launch"""
    if merged:
        monkeypatch.setenv("GLOME_DEBUG_BIH_UPDATE_MERGED", "1")
    b0, root0, tree, _, lights = build(name, "V0", wrap)
    _, tr = BR.check_fixture(name, b0, root0, tree)
    a = gpu_ctx.commit(b0, root0)
    cam = api.camera(*MR.camera_for(which))  # (the camera follows V2's similarity)
    if wrap == "instances":
        assert tr[0] == 1, "two Instances of a bih are the generic tier's"
    P = BR.triangles(name, which)
    ms = a.bih_update(tree, P)
    assert ms > 0
    a_says = answers(a, cam, lights, which, wrap == "bound")
    a.release()
    # scene B: the builder refitted first, then committed
    b, root, tree_b, _, _ = build(name, "V0", wrap)
    b.bih_set_triangles(tree_b, P)
    sc_b = gpu_ctx.commit(b, root)
    b_says = answers(sc_b, cam, lights, which, wrap == "bound")
    sc_b.release()
    assert (a_says["t"] >= 0).sum() >= 20 and (a_says["frame0"][..., 4] < 1e6).sum() >= 20, "the rays and the frame must see the triangles"
    assert_same(a_says, b_says, f"{name} under {wrap}, {which}")


def test_a_tree_read_from_a_show_text_is_updated_in_preorder(gpu_ctx):
    """a bih made by glome_sb_load_show keeps no list it was built from: item k is its k-th leaf item in preorder, on the device as on the host"""
    sd, b0, nm, tree0 = BR.build("mixed", "V0", "root")
    cam, lights = product_camera_lights(sd)
    T = BR.Tree(b0, tree0)
    index = {it: k for k, it in enumerate(b0.bih_items(tree0))}
    perm = [index[i] for k in T.leaves() for i in T.items[k]]  # the read tree's item k is the built tree's item perm[k]
    assert perm != sorted(perm)
    text = b0.show(tree0)
    P = BR.triangles("mixed", "V1")[perm]
    says = []
    for refit_first in (False, True):
        b = api.Builder()
        tree, _ = b.load_show(text)
        assert len(b.bih_items(tree)) == len(perm)
        if refit_first:
            b.bih_set_triangles(tree, P)
        sc = gpu_ctx.commit(b, tree)
        if not refit_first:
            assert sc.bih_update(tree, P) > 0
        says.append(answers(sc, cam, lights, "V1"))
        sc.release()
    assert (says[0]["t"] >= 0).sum() >= 20
    assert_same(says[0], says[1], "a bih read from a show text")
    # and it is the scene the built tree gives with the same triangles
    _, sc, tree_r, _, _ = make(gpu_ctx, "mixed", "V0", "root")
    sc.bih_update(tree_r, BR.triangles("mixed", "V1"))
    ref = answers(sc, cam, lights, "V1")
    sc.release()
    for key in ("frame0", "t", "shadow", "inside"):  # (prim ids are the other builder's)
        assert np.array_equal(np.asarray(says[0][key]), np.asarray(ref[key]), equal_nan=True), key


def test_there_and_back_renders_the_never_updated_frame(gpu_ctx):
    _, sc, tree, cam, lights = make(gpu_ctx, "mixed")
    before = frames(sc, cam, lights)
    sc.bih_update(tree, BR.triangles("mixed", "V1"))
    moved = frames(sc, cam, lights)
    assert not np.array_equal(moved["frame0"], before["frame0"])
    sc.bih_update(tree, BR.triangles("mixed", "V0"))
    assert_same(frames(sc, cam, lights), before, "V0 -> V1 -> V0")
    sc.release()


@pytest.mark.parametrize("which", ["V1", "V2"])
def test_updated_scene_against_the_oracle(gpu_ctx, which):
    sd0, b, nm, tree = BR.build("mixed")
    sc = gpu_ctx.commit(b, nm[sd0.root])
    sc.bih_update(tree, BR.triangles("mixed", which))
    sd, _ = BR.scene_desc("mixed", which)  # what the oracle is loaded with: a description made from the new triangles
    parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, sd, nm, n=20000)
    cam, lights = product_camera_lights(sd)
    img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=2))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, W, H, 2)
    sc.release()


def test_device_form_is_ordered_by_the_stream(gpu_ctx):
    """three updates from CUDA tensors, each followed by a render into a buffer of its own, nothing synchronised in between"""
    import torch
    cam = api.camera((-30.0, 40.0, 60.0), (25.0, 4.0, -20.0), (0.0, 1.0, 0.0), 60.0)  # sees the triangles at V0, V1 and V2
    _, sc, tree, _, lights = make(gpu_ctx, "mixed")
    P = api.render_params(width=W, height=H, maxdepth=2)
    dev = torch.device("cuda:0")
    order = ("V1", "V2", "V0")
    tensors = [torch.tensor(np.ascontiguousarray(BR.triangles("mixed", w)), dtype=torch.float64, device=dev) for w in order]
    bufs = [torch.zeros(H * W * 5, dtype=torch.float32, device=dev) for _ in order]
    sc.render_dev(cam, lights, P, bufs[0].data_ptr(), want_stats=False)  # (the frame size's tables are made at its first render, which waits for them)
    gpu_ctx.synchronize()
    bufs[0].zero_()
    torch.cuda.synchronize()
    for t, out in zip(tensors, bufs):
        assert sc.bih_update(tree, t) is None
        sc.render_dev(cam, lights, P, out.data_ptr(), want_stats=False)
    gpu_ctx.synchronize()
    got = [o.cpu().numpy().reshape(H, W, 5) for o in bufs]
    sc.release()
    for w, img in zip(order, got):
        _, ref, tree_r, _, _ = make(gpu_ctx, "mixed")
        ref.bih_update(tree_r, BR.triangles("mixed", w))  # the host form
        want, _, _ = ref.render(cam, lights, P, want_packed=False)
        ref.release()
        assert (want[..., 4] < 1e6).mean() > 0.01, w
        assert np.array_equal(img, want, equal_nan=True), w
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])


def test_refusals_leave_the_scene_as_it_was(gpu_ctx):
    P = BR.triangles("mixed", "V1")
    sd, b, nm, tree = BR.build("mixed", wrap="root")
    cam, lights = product_camera_lights(sd)
    tris = [nm[k] for k in range(len(P))]
    ball = b.sphere((0.0, 6.0, 0.0), 1.0)
    # a triangle bih that is an item of another bih: that tree's planes and root box were built from this one's bound
    outer = b.bih([tree, ball])
    sc = gpu_ctx.commit(b, outer)
    before = frames(sc, cam, lights)
    with pytest.raises(api.GlomeError, match=rf"bih {tree} lies inside bih {outer}.*status -1"):
        sc.bih_update(tree, P)
    with pytest.raises(api.GlomeError, match=rf"node {outer} is not a bih of plain triangles.*status -1"):
        sc.bih_update(outer, P[:2])
    assert_same(frames(sc, cam, lights), before, "a bih under a bih")
    sc.release()
    # a bih holding a sphere
    with_ball = b.bih(tris[:40] + [ball])
    sc = gpu_ctx.commit(b, with_ball)
    before = frames(sc, cam, lights)
    with pytest.raises(api.GlomeError, match=r"not a bih of plain triangles.*status -1"):
        sc.bih_update(with_ball, P[:41])
    assert_same(frames(sc, cam, lights), before, "a bih holding a sphere")
    sc.release()
    # a bih whose triangle is also in a group beside it: the device could not move that other copy
    sc = gpu_ctx.commit(b, b.group([tree, tris[7]]))
    before = frames(sc, cam, lights)
    with pytest.raises(api.GlomeError, match=rf"triangle {tris[7]} of bih {tree} is also part of the scene outside.*status -1"):
        sc.bih_update(tree, P)
    assert_same(frames(sc, cam, lights), before, "a triangle beside its bih")
    sc.release()
    # wrong counts, an id of another kind, an id of no node: refused by both forms
    root = b.group([tree, ball])
    sc = gpu_ctx.commit(b, root)
    before = frames(sc, cam, lights)
    for args, what in (((tree, P[:-1]), "too few"), ((tree, np.concatenate([P, P[:1]])), "too many"), ((ball, P), "a sphere"), ((root, P), "a list"), ((tris[0], P), "a triangle"),
                       ((10 ** 6, P), "no such node")):
        with pytest.raises(api.GlomeError, match=r"status -1"):
            sc.bih_update(*args)
        assert_same(frames(sc, cam, lights), before, what)
    nan = P.copy(); nan[5, 2] = np.nan
    with pytest.raises(api.GlomeError, match=r"not finite.*status -1"):
        sc.bih_update(tree, nan)  # the host form checks on the host
    assert_same(frames(sc, cam, lights), before, "a NaN through the host form")
    v = np.ascontiguousarray(P)
    assert sc.lib.glome_scene_bih_update_dev(sc.h, tree, C.c_void_p(v.ctypes.data), len(v) - 1) == L.E_INVALID  # (a host pointer: refused before the pointer is looked at)
    assert sc.lib.glome_scene_bih_update_dev(sc.h, tree, None, len(v)) == L.E_INVALID
    assert sc.lib.glome_scene_bih_update(sc.h, tree, None, len(v), None) == L.E_INVALID
    gpu_ctx.synchronize()
    assert_same(frames(sc, cam, lights), before, "the device form's refusals")
    sc.bih_update(tree, P)  # and the valid call still works
    assert not np.array_equal(frames(sc, cam, lights)["frame0"], before["frame0"])
    sc.release()


def test_a_coordinate_that_is_not_finite_is_reported_at_the_next_synchronize(gpu_ctx):
    import torch
    _, sc, tree, cam, lights = make(gpu_ctx, "mixed")
    P = BR.triangles("mixed", "V1")
    dev = torch.device("cuda:0")
    bad = P.copy(); bad[100, 3] = np.nan
    tb, tv = (torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev) for x in (bad, P))
    torch.cuda.synchronize()
    sc.bih_update(tree, tb)
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID
    assert "not finite" in gpu_ctx.err()
    sc.bih_update(tree, tv)  # a valid update: the scene is specified again
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0
    got = frames(sc, cam, lights)
    sc.release()
    b, root, tree_r, _, _ = build("mixed")
    b.bih_set_triangles(tree_r, P)
    ref = gpu_ctx.commit(b, root)
    assert_same(got, frames(ref, cam, lights), "a valid update after a refused one")
    ref.release()
