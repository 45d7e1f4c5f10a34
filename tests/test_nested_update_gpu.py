"""glome_scene_nested_updates / glome_scene_bih_refit: objects that lie under a bih are updated on the GPU and the bihs above them
refitted there, one call per tree, inner trees first.  The contract: after the last refit the committed scene is bit for bit the scene a
commit would have made after the builder's own sequence (test_nested_refit_host.py) -- so everything the two scenes answer is compared
bit for bit (NaNs as equal): frames in both render modes, the three per-ray seams on rays aimed at the moved objects, and the trace
seam's per-ray work records, which count the nodes a ray enters and so catch a plane that is merely conservative.  The normal of a ray
that misses is left out, as in test_instance_update_gpu.py and for its reason."""
import numpy as np
import pytest

import instances_refit as IR
import nested_refit as NR
import parity
import update_answers as UA
from helpers import product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api, scenes
from update_answers import assert_same

pytestmark = pytest.mark.gpu

W, H = 64, 48
N_RAYS = 3000
CENTER = {"oak_in_scene": (0.3, 2.2, -0.5)}


def frames(sc, cam, lights):
    return UA.frames(sc, cam, lights, (W, H))


def answers(sc, cam, lights, center):
    ro, rd = random_rays(N_RAYS, 23, center=center, radius=10, spread=4)
    out = frames(sc, cam, lights)
    hit = sc.rayint(ro, rd)
    out.update({"t": hit["t"], "prim": hit["prim"], "tex8": hit["tex"], "n": np.where(hit["t"][:, None] >= 0, hit["n"], 0)})
    out["shadow"] = sc.shadow(ro, rd, np.random.default_rng(24).uniform(1, 30, size=len(ro)).astype(np.float32))
    pts = np.random.default_rng(25).uniform(-4, 4, size=(N_RAYS, 3)) + np.asarray(center)
    out["inside"] = sc.inside(pts.astype(np.float32))
    rn = rd / np.linalg.norm(rd, axis=1, keepdims=True)
    out["work"] = sc.trace_work(ro, rn.astype(np.float32), lights, params=api.trace_params(maxdepth=2))["work"]
    return out


def which_of(name):
    return [5, 40, 62] if name == "oak_in_scene" else None


def committed_after(ctx, A, name, poses, cam, lights, center):
    """scene B: a builder made as the fixture is, the host sequence for every pose, then committed; what it answers.  The poses' calls
    are taken from A, the untouched builder of the same fixture (same ids): a pose is a move of the scene AS BUILT."""
    B = NR.get(name)
    for pose in poses:
        NR.host_sequence(B, NR.moves(A, pose, which_of(name)))
    sc = ctx.commit(B.b, B.root)
    says = answers(sc, cam, lights, center)
    sc.release()
    return says


def update_and_refit(sc, A, calls, dev_refit=False):
    """each update, then the refits in bihs_above order; checks the stale marks on the way"""
    for call in calls:
        assert NR.apply_scene(sc, call) > 0
        above = sc.bihs_above(NR.node_of(call))
        holder = above[:1] if call[0] == "inst" else []   # an Instance update refits the tree that holds the Instances itself
        stale = sc.stale_bihs()
        assert set(above) - set(holder) <= set(stale), (above, stale)
        for t in above:
            n0 = len(sc.stale_bihs())
            if dev_refit:
                sc.bih_refit_dev(t)
            else:
                assert sc.bih_refit(t) > 0
            assert len(sc.stale_bihs()) == n0 - (1 if t in stale else 0) and t not in sc.stale_bihs()
    assert sc.stale_bihs() == []


@pytest.mark.parametrize("dev_refit", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("name", NR.ALL)
def test_update_and_refits_equal_the_commit_of_the_refitted_builder(gpu_ctx, name, dev_refit):
    A = NR.get(name)
    cam, lights = product_camera_lights(A.sd)
    center = CENTER.get(name, (0.0, 1.5, 0.0))
    sc = gpu_ctx.commit(A.b, A.root)
    sc.nested_updates(True)
    before = answers(sc, cam, lights, center)
    done = []
    for pose in NR.POSES:
        # (every pose is taken from the builder as it was built: scene A's builder is never touched)
        update_and_refit(sc, A, NR.moves(A, pose, which_of(name)), dev_refit)
        gpu_ctx.synchronize()
        done.append(pose)
        a_says = answers(sc, cam, lights, center)
        b_says = committed_after(gpu_ctx, A, name, done, cam, lights, center)
        assert (a_says["t"] >= 0).sum() >= 20 and (a_says["frame0"][..., 4] < 1e6).sum() >= 20, "the rays and the frame must see the scene"
        assert not np.array_equal(a_says["frame0"], before["frame0"]), "the update must show"
        assert_same(a_says, b_says, f"{name} after {done}")
    sc.release()


@pytest.mark.parametrize("name,pose", [("nff_like", "grow"), ("mesh_shared", "shrink"), ("two_parents", "grow"), ("chain", "grow")])
def test_updated_scene_against_the_oracle(gpu_ctx, name, pose):
    A = NR.build(name)
    sc = gpu_ctx.commit(A.b, A.root)
    sc.nested_updates(True)
    update_and_refit(sc, A, NR.moves(A, pose))
    F = NR.build(name, pose)
    cam, lights = product_camera_lights(F.sd)
    img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=2))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), F.sd, W, H, 2)
    parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, F.sd, IR.node_map_at_pose(A, F), n=20000)
    sc.release()


@pytest.mark.parametrize("name", ["nff_like", "mesh_shared", "chain"])
def test_there_and_back_renders_the_never_updated_frame(gpu_ctx, name):
    A = NR.build(name)
    cam, lights = product_camera_lights(A.sd)
    sc = gpu_ctx.commit(A.b, A.root)
    sc.nested_updates(True)
    before = frames(sc, cam, lights)
    update_and_refit(sc, A, NR.moves(A, "grow"))
    assert not np.array_equal(frames(sc, cam, lights)["frame0"], before["frame0"])
    update_and_refit(sc, A, NR.original(A))
    assert_same(frames(sc, cam, lights), before, "there and back")
    sc.nested_updates(False)  # nothing is stale: allowed
    assert_same(frames(sc, cam, lights), before, "the switch itself changes nothing")
    sc.release()


def test_an_instance_moved_with_the_switch_off_is_refitted_with_its_new_matrix(gpu_ctx):
    """An Instance over the mesh is an item of one bih: it can be updated with the switch OFF, before the scene has any nested state.  A
    refit after a later mesh update must make that item's box from the NEW matrix.  Through the description's ids (scene.commit_desc):
    the Instance update with the switch off, the switch on, the mesh update, refit_above -- against the fresh commit of the builder."""
    from glome_amd.scene import commit_desc
    fx = NR.mesh_shared()
    cam, lights = product_camera_lights(fx.sd)
    D = commit_desc(gpu_ctx, fx.sd, nested=False)
    sc = D.scene
    before = answers(sc, cam, lights, (0.0, 1.5, 0.0))
    insts = [fx.named["i1"], fx.named["i2"]]
    M = np.stack([api.compose([IR.xf_of(D.builder, D.nmap[i]), api.rotate((0, 1, 0), 0.5), api.translate((0.6, 0.4, -0.8))]) for i in insts])
    kind, me, V0 = fx.movable[0]
    V1 = NR.pose_points(V0, "grow")
    assert D.instance_update(insts, M) > 0          # switch off: accepted as it always was (one bih above, the Instance is the item)
    with pytest.raises(api.GlomeError, match=r"mesh update refused.*status -1"):
        D.mesh_update(me, V1)
    sc.nested_updates(True)
    assert D.bihs_above(me) == [fx.bihs["root"]] == D.bihs_above(insts[0]) and D.stale_bihs() == []
    assert D.mesh_update(me, V1) > 0
    assert D.stale_bihs() == [fx.bihs["root"]]
    assert D.refit_above(me) > 0 and D.stale_bihs() == []
    got = answers(sc, cam, lights, (0.0, 1.5, 0.0))
    D.release()
    B = NR.Built(NR.mesh_shared())
    B.b.instance_set_transforms([B.nm[i] for i in insts], M)
    B.b.mesh_set_vertices(B.nm[me], V1)
    B.b.bih_refit(B.bihs["root"])
    ref = gpu_ctx.commit(B.b, B.root)
    want = answers(ref, cam, lights, (0.0, 1.5, 0.0))
    ref.release()
    assert not np.array_equal(got["frame0"], before["frame0"])
    assert_same(got, want, "Instances moved with the switch off, then the mesh and the refit")


def test_refusals_leave_the_scene_untouched(gpu_ctx):
    A = NR.build("chain")
    cam, lights = product_camera_lights(A.sd)
    inner, root = A.bihs["inner"], A.bihs["root"]
    sc = gpu_ctx.commit(A.b, A.root)
    before = frames(sc, cam, lights)
    (call,) = NR.moves(A, "grow")
    # the switch is off: the Instance update's own refusal, unchanged, and no refit
    with pytest.raises(api.GlomeError, match=rf"instance {call[1][0]} lies under bih {inner} inside bih {root}.*status -1"):
        NR.apply_scene(sc, call)
    with pytest.raises(api.GlomeError, match=r"bih refit refused: nested updates are off.*status -1"):
        sc.bih_refit(root)
    assert_same(frames(sc, cam, lights), before, "refusals with the switch off")
    sc.nested_updates(True)
    with pytest.raises(api.GlomeError, match=r"is not a bih of this scene that holds.*status -1"):
        sc.bih_refit(call[1][0])
    assert_same(frames(sc, cam, lights), before, "a refit of something that is no bih")
    sc.release()
    # a tree below is stale: the triangle bih under two trees
    b = api.Builder()
    t = b.bih(b.triangles_bulk(NR.tris9()))
    mid = b.bih([t, b.sphere((2.0, 1.0, -1.0), 0.5), b.sphere((4.0, 2.0, 2.0), 0.4), b.sphere((2.0, 3.0, 3.0), 0.3)])
    top = b.bih([mid, b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, -4.0), 0.5), b.sphere((0.0, 5.0, 0.0), 0.5)])
    sc = gpu_ctx.commit(b, top)
    sc.nested_updates(True)
    assert sc.bihs_above(t) == [mid, top] and sc.stale_bihs() == []
    sc.bih_update(t, NR.pose_points(NR.tris9().reshape(-1, 3), "grow").reshape(-1, 9))
    assert sc.stale_bihs() == [mid, top]
    moved = frames(sc, cam, lights)   # rendering while stale is allowed: unspecified, in bounds
    with pytest.raises(api.GlomeError, match=rf"bih {mid} below bih {top} is stale: refit bih {mid} first.*status -1"):
        sc.bih_refit(top)
    with pytest.raises(api.GlomeError, match=rf"bih {mid} is stale.*status -1"):
        sc.nested_updates(False)
    assert sc.stale_bihs() == [mid, top]
    assert_same(frames(sc, cam, lights), moved, "the refused refit and the refused switch")
    assert sc.refit_above(t) > 0 and sc.stale_bihs() == []
    got = frames(sc, cam, lights)
    sc.release()
    b.bih_set_triangles(t, NR.pose_points(NR.tris9().reshape(-1, 3), "grow").reshape(-1, 9))
    b.bih_refit(mid); b.bih_refit(top)
    ref = gpu_ctx.commit(b, top)
    assert_same(got, frames(ref, cam, lights), "two trees above a triangle bih")
    ref.release()


def test_with_the_switch_off_the_three_updates_refuse_what_they_refused(gpu_ctx):
    for name, k, msg in (("nff_like", 0, r"bih update refused: bih {node} lies inside bih {root}, whose planes and root box were built from its bound"),
                         ("mesh_shared", 0, r"mesh update refused: mesh {node} lies inside bih {root}, whose planes and root box were built from the mesh's bound"),
                         ("chain", 0, r"instance update refused: instance {node} lies under bih {inner} inside bih {root}")):
        A = NR.build(name)
        sc = gpu_ctx.commit(A.b, A.root)
        call = [c for c in NR.moves(A, "grow") if c[3] == k][0]
        with pytest.raises(api.GlomeError, match=msg.format(node=NR.node_of(call), root=A.bihs["root"], inner=A.bihs.get("inner")) + r".*status -1"):
            NR.apply_scene(sc, call)
        sc.release()


def test_device_forms_are_ordered_by_the_stream(gpu_ctx):
    """update, refit and render enqueued on one stream with no synchronize in between"""
    import torch
    A = NR.build("nff_like")
    cam, lights = product_camera_lights(A.sd)
    sc = gpu_ctx.commit(A.b, A.root)
    sc.nested_updates(True)
    P = api.render_params(width=W, height=H, maxdepth=2)
    dev = torch.device("cuda:0")
    calls = NR.moves(A, "grow")
    tensors = [torch.tensor(np.ascontiguousarray(c[2]), dtype=torch.float64, device=dev) for c in calls]
    bufs = [torch.zeros(H * W * 5, dtype=torch.float32, device=dev) for _ in range(2)]
    sc.render_dev(cam, lights, P, bufs[0].data_ptr(), want_stats=False)  # (the frame size's tables are made at its first render, which waits for them)
    sc.bih_refit(A.bihs["root"])                                         # (and the tree's workspace at its first refit)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    sc.render_dev(cam, lights, P, bufs[0].data_ptr(), want_stats=False)
    for c, t in zip(calls, tensors):
        assert sc.bih_update(c[1], t) is None
    sc.bih_refit_dev(A.bihs["root"])
    sc.render_dev(cam, lights, P, bufs[1].data_ptr(), want_stats=False)
    gpu_ctx.synchronize()
    got = [o.cpu().numpy().reshape(H, W, 5) for o in bufs]
    sc.release()
    for k, poses in enumerate(([], ["grow"])):
        R = NR.build("nff_like")
        for pose in poses:
            NR.host_sequence(R, NR.moves(R, pose))
        ref = gpu_ctx.commit(R.b, R.root)
        want, _, _ = ref.render(cam, lights, P, want_packed=False)
        ref.release()
        assert np.array_equal(got[k], want, equal_nan=True), k
    assert not np.array_equal(got[0], got[1])


def test_a_joined_box_that_reaches_infinity_is_reported_at_the_next_synchronize(gpu_ctx):
    """finite arithmetic: a coordinate whose padded value is exactly 1e6, the box `bih` refuses; a valid update and refit repair the scene"""
    b = api.Builder()
    pts = NR.tris9()
    t = b.bih(b.triangles_bulk(pts))
    root = b.bih([t, b.sphere((3.0, 1.0, -2.0), 0.5), b.sphere((-3.0, 1.0, 0.0), 0.5), b.sphere((0.0, 1.0, 3.0), 0.5)])
    cam, lights = api.camera((1.0, 6.0, 13.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 55.0), [api.light(p, c) for p, c in scenes.LIGHTS[:1]]
    sc = gpu_ctx.commit(b, root)
    sc.nested_updates(True)
    before = frames(sc, cam, lights)
    far = pts.copy(); far[0, 0] = 1e6 - 1e-4
    # (the update itself reports it too: the triangle bih's own joined box reaches 1e6)
    with pytest.raises(api.GlomeError, match=r"reaches infinity"):
        sc.bih_update(t, far)
    sc.bih_refit_dev(root)
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID
    assert "glome_scene_bih_refit" in gpu_ctx.err() and "reaches infinity" in gpu_ctx.err() and "glome_scene_instance_update" in gpu_ctx.err()
    sc.bih_update(t, pts)
    sc.bih_refit_dev(root)
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0
    assert_same(frames(sc, cam, lights), before, "a valid update and refit after an infinite box")
    sc.release()


def test_three_twigs_of_the_oak_in_the_default_scene(gpu_ctx):
    """GlomeView's default scene: three of the oak's 2,047 twigs moved, the oak's bih and the root refitted"""
    sd = scenes.testscene(2)
    b = api.Builder()
    nm, _ = sd.replay(b)
    root = nm[sd.root]
    cam, lights = product_camera_lights(sd)
    oak = b.bih_items(root)[4]
    oak_bih = oak - 3   # transform (tag (tex (bih ...)))
    assert b.show(oak_bih).startswith(("SI Bih", "Bih"))
    twigs = b.bih_items(oak_bih)
    ids = [twigs[k] for k in (3, 900, 2046)]
    M = np.stack([api.compose([IR.xf_of(b, i), api.rotate((0, 1, 0), api.deg(8)), api.translate((0.05, 0.1, -0.05))]) for i in ids])
    sc = gpu_ctx.commit(b, root)
    before = frames(sc, cam, lights)
    sc.nested_updates(True)
    assert sc.bihs_above(ids[0]) == [oak_bih, root] == b.bihs_above(root, ids[0])
    assert sc.instance_update(ids, M) > 0
    assert sc.stale_bihs() == [root]
    assert sc.refit_above(ids[0]) > 0 and sc.stale_bihs() == []
    got = frames(sc, cam, lights)
    sc.release()
    b.instance_set_transforms(ids, M)
    b.bih_refit(oak_bih); b.bih_refit(root)
    ref = gpu_ctx.commit(b, root)
    assert_same(got, frames(ref, cam, lights), "three twigs moved")
    ref.release()
    assert not np.array_equal(got["packed0"], before["packed0"]) or not np.array_equal(got["frame0"], before["frame0"])
