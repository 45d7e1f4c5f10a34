"""glome_scene_sphere_bih_update: new centres and radii for a committed sphere bih, its planes refitted on the GPU.  The contract: after an
update the committed scene is bit for bit the scene a commit after glome_sb_bih_set_spheres (test_sphere_bih_refit_host.py) would have
made -- so everything the two scenes answer is compared bit for bit (NaNs as equal), and the updated scene is held against the fp64 oracle
besides.  As in test_bih_update_gpu.py the normal of a ray that MISSES a scene whose root is a Bound is left out: a miss has no normal
(glome_hip.h), and under a Bound what is stored there differs between two commits of one builder."""
import ctypes as C

import numpy as np
import pytest

import parity
import spheres_refit as SR
import update_answers as UA
from helpers import product_camera_lights
from glome_amd import _lib as L
from glome_amd import api
from update_answers import assert_same, frames

pytestmark = pytest.mark.gpu

W, H = UA.SIZE


def answers(sc, cam, lights, which, hits_only_normals=False):
    """update_answers.answers on the pose's rays (hits_only_normals: the Bound case, see the top of the file)"""
    k = SR.MR.V2_SCALE if which == "V2" else 1.0
    shift = SR.MR.V2_SHIFT if which == "V2" else np.zeros(3)
    return UA.answers(sc, cam, lights, SR.rays_for(which), k, shift, hits_only_normals)


def cam_lights(B, which="V0"):
    _, lights = product_camera_lights(B.sd)
    return api.camera(*SR.MR.camera_for(which)), lights  # (the camera follows V2's similarity)


CASES = [(n, "tex", w, False) for n in ("three", "cluster", "cloud") for w in ("V1", "V2")] + [("cluster", wrap, "V1", False) for wrap in ("root", "instances", "bound")] + [("wide", "tex", "V1", True)]


@pytest.mark.parametrize("name,wrap,which,merged", CASES)
def test_update_equals_the_commit_of_the_refitted_builder(gpu_ctx, monkeypatch, name, wrap, which, merged):
    """a launch per level (the default) and, for the tree with a level wider than one block, every run of narrow levels in one
    single-block launch with the wide level between them on its own"""
    if merged:
        monkeypatch.setenv("GLOME_DEBUG_BIH_UPDATE_MERGED", "1")
    A = SR.build(name, "V0", wrap)
    SR.check_fixture(name, wrap, A)
    a = gpu_ctx.commit(A.b, A.root)
    cam, lights = cam_lights(A, which)
    S = SR.spheres(name, which)
    ms = a.sphere_bih_update(A.tree, S)
    assert ms > 0
    a_says = answers(a, cam, lights, which, wrap == "bound")
    rays, pixels = SR.sees_spheres(a, A, which, cam, W, H)
    a.release()
    # scene B: the builder refitted first, then committed
    B = SR.build(name, "V0", wrap)
    B.b.bih_set_spheres(B.tree, S)
    sc_b = gpu_ctx.commit(B.b, B.root)
    b_says = answers(sc_b, cam, lights, which, wrap == "bound")
    sc_b.release()
    assert rays >= 20 and pixels >= 20, "the rays and the frame must see the spheres"
    assert_same(a_says, b_says, f"{name} under {wrap}, {which}")


def test_there_and_back_renders_the_never_updated_frame(gpu_ctx):
    """and an update with the spheres the scene was committed with changes no frame"""
    A = SR.build("cluster")
    cam, lights = cam_lights(A)
    sc = gpu_ctx.commit(A.b, A.root)
    before = frames(sc, cam, lights)
    sc.sphere_bih_update(A.tree, SR.spheres("cluster", "V0"))
    assert_same(frames(sc, cam, lights), before, "V0 -> V0")
    sc.sphere_bih_update(A.tree, SR.spheres("cluster", "V1"))
    moved = frames(sc, cam, lights)
    assert not np.array_equal(moved["frame0"], before["frame0"])
    sc.sphere_bih_update(A.tree, SR.spheres("cluster", "V0"))
    assert_same(frames(sc, cam, lights), before, "V0 -> V1 -> V0")
    sc.release()


def test_updated_scene_against_the_oracle(gpu_ctx):
    """(parity.check_rays aims at the origin's neighbourhood: V1's, not the far-away V2's)"""
    A = SR.build("cloud")
    sc = gpu_ctx.commit(A.b, A.root)
    sc.sphere_bih_update(A.tree, SR.spheres("cloud", "V1"))
    sd, _, _ = SR.scene_desc("cloud", "V1")  # what the oracle is loaded with: a description made from the new spheres
    parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, sd, A.nm, n=20000)
    cam, lights = product_camera_lights(sd)
    img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=2))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, W, H, 2)
    sc.release()


def test_device_form_is_ordered_by_the_stream(gpu_ctx):
    """three updates from CUDA tensors, each followed by a render into a buffer of its own, nothing synchronised in between"""
    import torch
    cam = api.camera((-30.0, 40.0, 60.0), (25.0, 4.0, -20.0), (0.0, 1.0, 0.0), 60.0)  # sees the spheres at V0, V1 and V2
    A = SR.build("cluster")
    _, lights = cam_lights(A)
    sc = gpu_ctx.commit(A.b, A.root)
    P = api.render_params(width=W, height=H, maxdepth=2)
    dev = torch.device("cuda:0")
    order = ("V1", "V2", "V0")
    tensors = [torch.tensor(np.ascontiguousarray(SR.spheres("cluster", w)), dtype=torch.float64, device=dev) for w in order]
    bufs = [torch.zeros(H * W * 5, dtype=torch.float32, device=dev) for _ in order]
    sc.render_dev(cam, lights, P, bufs[0].data_ptr(), want_stats=False)  # (the frame size's tables are made at its first render, which waits for them)
    gpu_ctx.synchronize()
    bufs[0].zero_()
    torch.cuda.synchronize()
    for t, out in zip(tensors, bufs):
        assert sc.sphere_bih_update(A.tree, t) is None
        sc.render_dev(cam, lights, P, out.data_ptr(), want_stats=False)
    gpu_ctx.synchronize()
    got = [o.cpu().numpy().reshape(H, W, 5) for o in bufs]
    sc.release()
    for w, img in zip(order, got):
        R = SR.build("cluster")
        ref = gpu_ctx.commit(R.b, R.root)
        ref.sphere_bih_update(R.tree, SR.spheres("cluster", w))  # the host form
        want, _, _ = ref.render(cam, lights, P, want_packed=False)
        ref.release()
        assert np.array_equal(img, want, equal_nan=True), w
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])


@pytest.mark.parametrize("how", ["direct", "instanced"])
def test_a_sphere_bih_under_two_bihs(gpu_ctx, how):
    """switch off: refused, the trees above named; switch on: the update leaves the trees above stale, they are refitted inner tree first,
    and the scene is the commit of the builder after bih_set_spheres + bih_refit(mid) + bih_refit(top), bit for bit"""
    A = SR.build_nested("cluster", "V0", how)
    cam, lights = cam_lights(A)
    S = SR.spheres("cluster", "V1")
    sc = gpu_ctx.commit(A.b, A.root)
    before = frames(sc, cam, lights)
    with pytest.raises(api.GlomeError, match=rf"bih {A.tree} lies inside bih {A.top}.*status -1"):
        sc.sphere_bih_update(A.tree, S)
    assert_same(frames(sc, cam, lights), before, "refused with the switch off")
    sc.nested_updates(True)
    assert sc.bihs_above(A.tree) == [A.mid, A.top] and sc.stale_bihs() == []
    assert sc.sphere_bih_update(A.tree, S) > 0
    assert sc.stale_bihs() == [A.mid, A.top]
    with pytest.raises(api.GlomeError, match=rf"refit bih {A.mid} first.*status -1"):
        sc.bih_refit(A.top)
    for t in sc.bihs_above(A.tree):
        assert sc.bih_refit(t) > 0
    assert sc.stale_bihs() == []
    a_says = answers(sc, cam, lights, "V1")
    rays, pixels = SR.sees_spheres(sc, A, "V1", cam, W, H)
    sc.release()
    B = SR.build_nested("cluster", "V0", how)
    B.b.bih_set_spheres(B.tree, S)
    B.b.bih_refit(B.mid)
    B.b.bih_refit(B.top)
    sc_b = gpu_ctx.commit(B.b, B.root)
    b_says = answers(sc_b, cam, lights, "V1")
    sc_b.release()
    assert rays >= 20 and pixels >= 20
    assert_same(a_says, b_says, f"a sphere bih under two bihs, {how}")


def test_refusals_leave_the_scene_as_it_was(gpu_ctx):
    S = SR.spheres("cluster", "V1")
    A = SR.build("cluster", wrap="root")
    b, tree = A.b, A.tree
    cam, lights = cam_lights(A)
    # a sphere of the bih that is also in a group beside it: the device could not move that other record
    sc = gpu_ctx.commit(b, b.group([tree, A.balls[7]]))
    before = frames(sc, cam, lights)
    with pytest.raises(api.GlomeError, match=rf"sphere {A.balls[7]} of bih {tree} is also part of the scene outside.*status -1"):
        sc.sphere_bih_update(tree, S)
    assert_same(frames(sc, cam, lights), before, "a sphere beside its bih")
    sc.release()
    # a bih that holds one Sphere node under two items: two records, which one row could not name
    twice = b.bih(A.balls[:5] + [b.tex(A.balls[1], 0)])
    sc = gpu_ctx.commit(b, twice)
    before = frames(sc, cam, lights)
    with pytest.raises(api.GlomeError, match=rf"bih {twice} holds sphere {A.balls[1]} more than once.*status -1"):
        sc.sphere_bih_update(twice, S[:6])
    assert_same(frames(sc, cam, lights), before, "a sphere twice in its bih")
    sc.release()
    # wrong counts, ids of other kinds, an id of no node, bad values: refused by the host form
    tris = b.bih([b.triangle((0.0, 5.0, 0.0), (1.0, 5.0, 0.0), (0.0, 6.0, 0.5)), b.triangle((2.0, 5.0, 0.0), (3.0, 5.0, 0.0), (2.0, 6.0, 0.5))])
    root = b.group([tree, tris])
    sc = gpu_ctx.commit(b, root)
    before = frames(sc, cam, lights)

    def variant(row, col, value):
        X = S.copy(); X[row, col] = value
        return X
    for args, what, msg in (((tree, S[:-1]), "too few", r"has 40 items, not 39"), ((tree, np.concatenate([S, S[:1]])), "too many", r"has 40 items, not 41"),
                            ((tris, S[:2]), "a triangle bih", rf"node {tris} is not a bih of plain spheres of this scene"), ((A.balls[0], S), "a sphere", r"not a bih of plain spheres"),
                            ((root, S), "a list", r"not a bih of plain spheres"), ((10 ** 6, S), "no such node", r"not a bih of plain spheres"),
                            ((tree, variant(5, 2, np.nan)), "a NaN", r"a value is not finite"), ((tree, variant(6, 3, 0.0)), "radius 0", r"radius of item 6 is not positive"),
                            ((tree, variant(7, 3, -1.0)), "a negative radius", r"radius of item 7 is not positive")):
        with pytest.raises(api.GlomeError, match=msg + r".*status -1"):
            sc.sphere_bih_update(*args)
        assert_same(frames(sc, cam, lights), before, what)
    with pytest.raises(api.GlomeError, match=r"not a bih of plain triangles.*status -1"):
        sc.bih_update(tree, np.zeros((40, 9)))  # and the triangle update keeps refusing a sphere bih
    v = np.ascontiguousarray(S)
    assert sc.lib.glome_scene_sphere_bih_update_dev(sc.h, tree, C.c_void_p(v.ctypes.data), len(v) - 1) == L.E_INVALID  # (a host pointer: refused before the pointer is looked at)
    assert sc.lib.glome_scene_sphere_bih_update_dev(sc.h, tree, None, len(v)) == L.E_INVALID
    assert sc.lib.glome_scene_sphere_bih_update(sc.h, tree, None, len(v), None) == L.E_INVALID
    gpu_ctx.synchronize()
    assert_same(frames(sc, cam, lights), before, "the raw forms' refusals")
    sc.sphere_bih_update(tree, S)  # and the valid call still works
    assert not np.array_equal(frames(sc, cam, lights)["frame0"], before["frame0"])
    sc.release()


@pytest.mark.parametrize("what", ["nan", "radius0"])
def test_a_bad_value_through_the_device_form_is_reported_at_the_next_synchronize(gpu_ctx, what):
    """an error return, not a fault: every store of the update is to an index below its table's count, whatever the values"""
    import torch
    A = SR.build("cluster")
    cam, lights = cam_lights(A)
    sc = gpu_ctx.commit(A.b, A.root)
    S = SR.spheres("cluster", "V1")
    dev = torch.device("cuda:0")
    bad = S.copy()
    if what == "nan":
        bad[20, 1] = np.nan
    else:
        bad[33, 3] = 0.0
    tb, tv = (torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev) for x in (bad, S))
    torch.cuda.synchronize()
    sc.sphere_bih_update(A.tree, tb)
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID
    assert "glome_scene_sphere_bih_update" in gpu_ctx.err()
    sc.sphere_bih_update(A.tree, tv)  # a valid update: the scene is specified again
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0
    got = frames(sc, cam, lights)
    sc.release()
    B = SR.build("cluster")
    B.b.bih_set_spheres(B.tree, S)
    ref = gpu_ctx.commit(B.b, B.root)
    assert_same(got, frames(ref, cam, lights), "a valid update after a refused one")
    ref.release()
