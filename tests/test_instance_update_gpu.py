"""glome_scene_instance_update: new matrices for committed Instances, the bih that holds them as items refitted on the GPU.  The contract:
after an update the committed scene is bit for bit the scene a commit after glome_sb_instance_set_transforms (test_instance_refit_host.py)
would have made -- so everything the two scenes answer is compared bit for bit (NaNs as equal), and the updated scene is held against the
fp64 oracle of the scene built fresh at the new pose besides.  The normal of a ray that misses is left out, as in test_bih_update_gpu.py
and for its reason: a miss has no normal (glome_hip.h), and under a Bound what is stored there differs between two commits of one
builder."""
import ctypes as C

import numpy as np
import pytest

import bihs_refit as BR
import instances_refit as IR
import parity
import update_answers as UA
from helpers import product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api, scenes
from update_answers import assert_same

pytestmark = pytest.mark.gpu

W, H = 64, 48
N_RAYS = 3000


def frames(sc, cam, lights):
    return UA.frames(sc, cam, lights, (W, H))


def answers(sc, cam, lights, center=(0.0, 2.0, 0.0)):
    """everything a scene answers: a frame in both render modes (rgbad and packed) and the three per-ray seams"""
    ro, rd = random_rays(N_RAYS, 23, center=center, radius=12, spread=5)
    out = frames(sc, cam, lights)
    hit = sc.rayint(ro, rd)
    out.update({"t": hit["t"], "prim": hit["prim"], "tex8": hit["tex"], "n": np.where(hit["t"][:, None] >= 0, hit["n"], 0)})
    out["shadow"] = sc.shadow(ro, rd, np.random.default_rng(24).uniform(1, 30, size=len(ro)).astype(np.float32))
    pts = np.random.default_rng(25).uniform(-5, 5, size=(N_RAYS, 3)) + np.asarray(center)
    out["inside"] = sc.inside(pts.astype(np.float32))
    return out


def get(name):
    return IR.build_oak() if name == "oak" else IR.build(name)


def committed_after(ctx, name, steps, cam, lights, center):
    """scene B: a builder made as the fixture is, instance_set_transforms for every step, then committed; what it answers"""
    B = get(name)
    for ids, M in steps:
        B.b.instance_set_transforms(ids, M)
    sc = ctx.commit(B.b, B.root)
    says = answers(sc, cam, lights, center)
    sc.release()
    return says


# (name, the steps: (pose, which movables or None for all) -- each step is an update of scene A and a commit of scene B)
THREE = [2, 17, 33]
CASES = {
    "a_flat3": ("flat3", [("grow", None), ("shrink", [1])]),
    "b_shared": ("shared", [("grow", None)]),
    "c_subtrees": ("subtrees", [("grow", None), ("shrink", [1])]),
    "d_grove": ("grove", [("grow", None), ("shrink", None), ("grow", THREE)]),
    "e_mixed": ("mixed", [("grow", None), ("shrink", [0, 3])]),
    "f_mixed_nested": ("mixed_nested", [("grow", None), ("shrink", None)]),
    "g_oak": ("oak", [("grow", None), ("shrink", [5, 40, 62])]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_update_equals_the_commit_of_the_refitted_builder(gpu_ctx, case):
    name, steps = CASES[case]
    A = get(name)
    cam, lights = product_camera_lights(A.sd)
    center = (0.0, 2.2, 0.0)
    tr = BR.traits(A.b, A.root)
    if name == "flat3":
        assert tr[0] == 0, "three Instances over primitives and CSG are the flat tier's"
    if name == "grove":
        T = BR.Tree(A.b, A.bih)
        sizes = [int(T.nleaf[k]) for k in T.leaves()]
        assert max(sizes) >= 7 and min(sizes) == 0, sizes  # the count escape, the -+inf planes
    sc = gpu_ctx.commit(A.b, A.root)
    before = answers(sc, cam, lights, center)
    done = []
    for pose, which in steps:
        # (every pose is taken from the builder as it was built: scene A's builder is never touched)
        ids, M = IR.moved_matrices(A, pose, which)
        ms = sc.instance_update(ids, M)
        assert ms > 0
        done.append((ids, M))
        a_says = answers(sc, cam, lights, center)
        b_says = committed_after(gpu_ctx, name, done, cam, lights, center)
        assert (a_says["t"] >= 0).sum() >= 20 and (a_says["frame0"][..., 4] < 1e6).sum() >= 20, "the rays and the frame must see the scene"
        assert not np.array_equal(a_says["frame0"], before["frame0"]), "the update must show"
        assert_same(a_says, b_says, f"{case} after {len(done)} update(s)")
    sc.release()


@pytest.mark.parametrize("name,pose", [("grove", "grow"), ("grove", "shrink"), ("oak", "grow"), ("oak", "shrink")])
def test_updated_scene_against_the_oracle(gpu_ctx, name, pose):
    """the updated scene against the fp64 oracle of the scene built fresh at the pose, under the gates the scene's class states
    (zoo.grove's, scenes.testscene's for the oak; instances_refit.py) -- poses for which the host build of the fresh scene is itself
    within the gate (test_instance_refit_host.py)"""
    A = get(name)
    sc = gpu_ctx.commit(A.b, A.root)
    sc.instance_update(*IR.moved_matrices(A, pose))
    F = IR.Built(IR.oak_explicit(pose)) if name == "oak" else IR.build(name, pose)
    cam, lights = product_camera_lights(F.sd)
    img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=2))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), F.sd, W, H, 2)
    if name == "grove":  # (F's description is A's plus the pose's transforms: primitive ids compare through node_map_at_pose)
        parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, F.sd, IR.node_map_at_pose(A, F), n=20000)
    else:
        # (the ids of the oak's items have no common map: parity.check_rays' other checks, under its own bounds -- instances_refit.py; the
        # host build of the scene made fresh at the pose passes the same check in test_instance_refit_host.py)
        IR.check_oak_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), F)
    sc.release()


@pytest.mark.parametrize("name", ["grove", "mixed_nested", "flat3"])
def test_there_and_back_renders_the_never_updated_frame(gpu_ctx, name):
    A = get(name)
    cam, lights = product_camera_lights(A.sd)
    sc = gpu_ctx.commit(A.b, A.root)
    before = frames(sc, cam, lights)
    sc.instance_update(*IR.moved_matrices(A, "grow"))
    moved = frames(sc, cam, lights)
    assert not np.array_equal(moved["frame0"], before["frame0"])
    sc.instance_update(*IR.original_matrices(A))
    assert_same(frames(sc, cam, lights), before, "there and back")
    sc.release()


def test_device_form_is_ordered_by_the_stream(gpu_ctx):
    """render, update, render on one stream, nothing synchronised in between: the frames of the two poses"""
    import torch
    A = get("grove")
    cam, lights = product_camera_lights(A.sd)
    sc = gpu_ctx.commit(A.b, A.root)
    P = api.render_params(width=W, height=H, maxdepth=2)
    dev = torch.device("cuda:0")
    poses = ("grow", "shrink")
    moves = [IR.moved_matrices(A, p) for p in poses]
    tensors = [torch.tensor(np.ascontiguousarray(M), dtype=torch.float64, device=dev) for _, M in moves]
    bufs = [torch.zeros(H * W * 5, dtype=torch.float32, device=dev) for _ in range(3)]
    sc.render_dev(cam, lights, P, bufs[0].data_ptr(), want_stats=False)  # (the frame size's tables are made at its first render, which waits for them)
    gpu_ctx.synchronize()
    bufs[0].zero_()
    torch.cuda.synchronize()
    gpu_ctx.lib.glome_ctx_timing_begin(gpu_ctx.h, 16)
    sc.render_dev(cam, lights, P, bufs[0].data_ptr(), want_stats=False)
    for (ids, _), t, out in zip(moves, tensors, bufs[1:]):
        assert sc.instance_update_dev(ids, t) is None
        sc.render_dev(cam, lights, P, out.data_ptr(), want_stats=False)
    ms = np.zeros(16, np.float32)
    n_timed = gpu_ctx.lib.glome_ctx_timing_end(gpu_ctx.h, ms.ctypes.data_as(L.c_fp), 16)
    assert n_timed == 5 and (ms[:5] > 0).all(), (n_timed, ms)  # three renders, and one event pair per update
    gpu_ctx.synchronize()
    got = [o.cpu().numpy().reshape(H, W, 5) for o in bufs]
    sc.release()
    for k, steps in enumerate(([], moves[:1], moves)):
        R = get("grove")
        for ids, M in steps:
            R.b.instance_set_transforms(ids, M)
        ref = gpu_ctx.commit(R.b, R.root)
        want, _, _ = ref.render(cam, lights, P, want_packed=False)
        ref.release()
        assert np.array_equal(got[k], want, equal_nan=True), k
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


def refused(sc, ids, M, msg, cam, lights, before, what):
    with pytest.raises(api.GlomeError, match=msg + r".*status -1"):
        sc.instance_update(ids, M)
    assert_same(frames(sc, cam, lights), before, what)


def test_refusals_leave_the_scene_as_it_was(gpu_ctx):
    A = get("mixed")
    b = A.b
    cam, lights = product_camera_lights(A.sd)
    ids, M = IR.moved_matrices(A, "grow")
    ball = b.sphere((0.0, 6.0, 0.0), 1.0)
    # an Instance inside an item of a bih (the item is a group), and one with two bihs above it
    loose = b.transform(b.sphere((0.0, 0.0, 0.0), 0.5), [api.translate((5.0, 1.0, 0.0))])
    holder = b.bih([b.group([loose, b.sphere((5.0, 2.0, 0.0), 0.3)]), ball, b.sphere((6.0, 1.0, 1.0), 0.4), b.sphere((4.0, 1.0, -1.0), 0.4)])
    outer = b.bih([A.bih, holder])
    sc = gpu_ctx.commit(b, outer)
    before = frames(sc, cam, lights)
    one = IR.xf_of(b, loose).reshape(1, 24)
    refused(sc, [loose], one, rf"instance {loose} lies under bih {holder} inside bih {outer}", cam, lights, before, "two bihs above (inside an item)")
    refused(sc, ids[:1], M[:1], rf"instance {ids[0]} lies under bih {A.bih} inside bih {outer}", cam, lights, before, "two bihs above")
    sc.release()
    sc = gpu_ctx.commit(b, b.group([holder, A.bih]))
    before = frames(sc, cam, lights)
    refused(sc, [loose], one, rf"instance {loose} lies inside an item of bih {holder} rather than being the item", cam, lights, before, "inside an item")
    # ids: not an Instance, not of this scene, twice; counts and pointers; a matrix that fails check_xfm or is not finite (the host form)
    stranger = b.transform(b.sphere((0.0, 0.0, 0.0), 0.5), [api.translate((1.0, 1.0, 0.0))])  # made after the commit: not of this scene
    refused(sc, [ball], one, rf"node {ball} is not an Instance of this scene", cam, lights, before, "a sphere")
    refused(sc, [A.bih], one, rf"node {A.bih} is not an Instance of this scene", cam, lights, before, "a bih")
    refused(sc, [stranger], one, rf"node {stranger} is not an Instance of this scene", cam, lights, before, "an Instance of no scene")
    refused(sc, [10 ** 6], one, r"node 1000000 is not an Instance of this scene", cam, lights, before, "no such node")
    refused(sc, ids[:2] + ids[:1], M[:3], rf"node {ids[0]} is named more than once", cam, lights, before, "an id twice")
    corrupt = M.copy(); corrupt[2, :12] *= 2.0
    refused(sc, ids, corrupt, rf"node {ids[2]}: corrupt matrix", cam, lights, before, "a matrix that fails check_xfm")
    nan = M.copy(); nan[1, 5] = np.nan
    refused(sc, ids, nan, rf"node {ids[1]} is not finite", cam, lights, before, "a NaN through the host form")
    i32, pi = L.ivec(ids)
    m = np.ascontiguousarray(M)
    for form, args in ((sc.lib.glome_scene_instance_update, (None,)), (sc.lib.glome_scene_instance_update_dev, ())):
        assert form(sc.h, pi, None, len(ids), *args) == L.E_INVALID
        assert form(sc.h, None, m.ctypes.data_as(L.c_dp) if args else C.c_void_p(m.ctypes.data), len(ids), *args) == L.E_INVALID
        assert form(sc.h, pi, m.ctypes.data_as(L.c_dp) if args else C.c_void_p(m.ctypes.data), -1, *args) == L.E_INVALID
        assert "bad count or null array" in gpu_ctx.err()
    _, pball = L.ivec([ball])
    assert sc.lib.glome_scene_instance_update_dev(sc.h, pball, C.c_void_p(m.ctypes.data), 1) == L.E_INVALID  # (a host pointer: refused before the pointer is looked at)
    gpu_ctx.synchronize()
    assert_same(frames(sc, cam, lights), before, "the refusals of both forms")
    sc.instance_update(ids, M)  # and the valid call still works
    assert not np.array_equal(frames(sc, cam, lights)["frame0"], before["frame0"])
    sc.release()


def test_refusals_and_the_door_of_the_default_scene(gpu_ctx):
    """GlomeView's default scene, whose root is itself a bih: the oak's items have two bihs above them, the chessboard's Instance lies
    inside an item (a Difference); the door, the glass and the whole oak are items of the root bih and move"""
    sd = scenes.testscene(2)
    b = api.Builder()
    nm, _ = sd.replay(b)
    root = nm[sd.root]
    cam, lights = product_camera_lights(sd)
    board, _, _, cone, oak, hollow, door, glass = b.bih_items(root)
    oak_bih, board_inst = oak - 3, board - 3   # transform (tag (tex (bih ...))); difference (transform board) (tex sphere)
    assert b.show(oak_bih).startswith(("SI Bih", "Bih"))
    twigs = b.bih_items(oak_bih)
    assert len(twigs) == 2047 and all(IR.is_instance(b, i) for i in (twigs[0], twigs[-1], board_inst, cone, oak, door, glass))
    sc = gpu_ctx.commit(b, root)
    before = frames(sc, cam, lights)
    refused(sc, twigs[:1], IR.xf_of(b, twigs[0]).reshape(1, 24), rf"instance {twigs[0]} lies under bih {oak_bih} inside bih {root}", cam, lights, before, "an oak item")
    refused(sc, [board_inst], IR.xf_of(b, board_inst).reshape(1, 24), rf"instance {board_inst} lies inside an item of bih {root}", cam, lights, before, "the board's Instance")
    ids = [door, glass, oak]
    M = np.stack([api.compose([IR.xf_of(b, i), api.rotate((0, 1, 0), api.deg(5)), api.translate((0.3, 0.1, -0.2))]) for i in ids])
    assert sc.instance_update(ids, M) > 0
    got = frames(sc, cam, lights)
    sc.release()
    assert not np.array_equal(got["frame0"], before["frame0"])
    b.instance_set_transforms(ids, M)
    ref = gpu_ctx.commit(b, root)
    assert_same(got, frames(ref, cam, lights), "the door, the glass and the oak moved")
    ref.release()


def test_a_matrix_that_is_not_finite_is_reported_at_the_next_synchronize(gpu_ctx):
    import torch
    A = get("grove")
    cam, lights = product_camera_lights(A.sd)
    sc = gpu_ctx.commit(A.b, A.root)
    ids, M = IR.moved_matrices(A, "grow")
    bad = M.copy(); bad[7, 3] = np.nan
    dev = torch.device("cuda:0")
    tb, tv = (torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev) for x in (bad, M))
    torch.cuda.synchronize()
    sc.instance_update_dev(ids, tb)
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID
    assert "not finite" in gpu_ctx.err() and "glome_scene_instance_update" in gpu_ctx.err() and "glome_scene_bih_update" in gpu_ctx.err() and "mesh update" in gpu_ctx.err()
    sc.instance_update_dev(ids, tv)  # a valid update: the scene is specified again
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0
    got = frames(sc, cam, lights)
    sc.release()
    R = get("grove")
    R.b.instance_set_transforms(ids, M)
    ref = gpu_ctx.commit(R.b, R.root)
    assert_same(got, frames(ref, cam, lights), "a valid update after a refused one")
    ref.release()


def test_an_item_box_that_reaches_infinity(gpu_ctx):
    """the host form refuses it as `bih` does; the device form raises the bad-input bit, and a valid update repairs the scene"""
    import torch
    b = api.Builder()
    pl, tree = IR.plane_bih(b)
    cam, lights = api.camera((1.0, 6.0, 13.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 55.0), [api.light(p, c) for p, c in scenes.LIGHTS[:1]]
    sc = gpu_ctx.commit(b, tree)
    before = frames(sc, cam, lights)
    bad, good = api.translate((1e-4, 0, 0)).reshape(1, 24), api.translate((0.0, 0.5, 0.0)).reshape(1, 24)
    with pytest.raises(api.GlomeError, match=rf"node {pl} in bih {tree}: bih: infinite bounding box.*status -2"):
        sc.instance_update([pl], bad)
    assert_same(frames(sc, cam, lights), before, "an infinite box through the host form")
    tb, tg = (torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda:0") for x in (bad, good))
    torch.cuda.synchronize()
    sc.instance_update_dev([pl], tb)
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID and "reaches infinity" in gpu_ctx.err()
    sc.instance_update_dev([pl], tg)
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0
    got = frames(sc, cam, lights)
    sc.release()
    b.instance_set_transforms([pl], good)
    ref = gpu_ctx.commit(b, tree)
    assert_same(got, frames(ref, cam, lights), "a valid update after an infinite box")
    ref.release()
    assert not np.array_equal(got["frame0"], before["frame0"])
