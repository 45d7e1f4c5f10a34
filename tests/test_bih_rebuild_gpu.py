"""glome_scene_bih_rebuild / _indexed / glome_scene_sphere_bih_rebuild: a committed triangle or sphere bih re-split on the GPU, in place.
The contract: after a rebuild the committed scene is bit for bit the scene a commit would have made after the builder's own sequence
(test_bih_resplit_host.py): set_triangles / set_spheres, bih_resplit, bih_refit of the bihs above -- so everything the two scenes answer
is compared bit for bit (update_answers.assert_same, no allowance), the work counters of a counting frame included.  The normal of a
ray that misses a scene under a Bound is left out, for test_bih_update_gpu.py's reason."""
import numpy as np
import pytest

import bihs_refit as BR
import bihs_resplit as RS
import meshes_refit as MR
import nested_refit as NR
import parity
import spheres_refit as SR
import update_answers as UA
from helpers import product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api
from update_answers import assert_same, frames

pytestmark = pytest.mark.gpu

W, H = 128, 96


def build(name, wrap="tex"):
    sd, b, nm, tree = BR.build(name, "V0", wrap)
    cam, lights = product_camera_lights(sd)
    return b, nm[sd.root], tree, cam, lights


def work(sc, cam, lights):
    """(bih_nodes, prim_tests) of a counting frame, faithful and production"""
    out = []
    for faithful in (1, 0):
        _, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=2, faithful=faithful, count_work=1))
        out.append((int(st["bih_nodes"]), int(st["prim_tests"])))
    return out


def answers(sc, cam, lights, which="V1", hits_only_normals=False):
    k = MR.V2_SCALE if which == "V2" else 1.0
    shift = MR.V2_SHIFT if which == "V2" else np.zeros(3)
    rays = random_rays(3000, 23, center=tuple(np.array((0, 1.5, 0)) * k + shift), radius=13 * k, spread=7 * k)
    out = UA.answers(sc, cam, lights, rays, k, shift, hits_only_normals, size=(W, H))
    out["work"] = np.array(work(sc, cam, lights))
    return out


def spec_commit(ctx, name, wrap, P):
    """the commit after the spec sequence: set_triangles, bih_resplit"""
    b, root, tree, _, _ = build(name, wrap)
    b.bih_set_triangles(tree, P)
    b.bih_resplit(tree)
    return b, ctx.commit(b, root), tree


CASES = [(n, "tex", w) for n in ("three", "mixed", "s3_20", "wide") for w in ("V1", "V2", "SH")] + [("mixed", wrap, "V1") for wrap in ("root", "instances", "bound")]


@pytest.mark.parametrize("name,wrap,which", CASES)
def test_rebuild_equals_the_commit_after_the_spec_sequence(gpu_ctx, name, wrap, which):
    b0, root0, tree, _, lights = build(name, wrap)
    a = gpu_ctx.commit(b0, root0)
    cam = api.camera(*MR.camera_for(which))
    P = RS.triangles(name, which)
    assert a.bih_rebuild(tree, P) > 0
    a_says = answers(a, cam, lights, which, wrap == "bound")
    a_lay, a_info = a.bih_layout(tree), a.info()
    a.release()
    b, sc_b, tree_b = spec_commit(gpu_ctx, name, wrap, P)
    b_says = answers(sc_b, cam, lights, which, wrap == "bound")
    b_lay, b_info = sc_b.bih_layout(tree_b), sc_b.info()
    sc_b.release()
    assert (a_says["t"] >= 0).sum() >= 20 and (a_says["frame0"][..., 4] < 1e6).sum() >= 20, "the rays and the frame must see the triangles"
    assert_same(a_says, b_says, f"{name} under {wrap}, {which}")
    assert [a_lay[k] for k in ("slots", "pairs", "records", "depth")] == [b_lay[k] for k in ("slots", "pairs", "records", "depth")]
    assert a_lay["depth"] == b.bih_layout(tree_b)["depth"] and a_info["max_bih_depth"] == b_info["max_bih_depth"]


def test_rebuild_costs_what_the_fresh_commit_costs_and_less_than_the_refit(gpu_ctx):
    b0, root0, tree, cam, lights = build("s3_20")
    P = RS.triangles("s3_20", "SH")
    a = gpu_ctx.commit(b0, root0)
    a.bih_update(tree, P)
    refit = work(a, cam, lights)
    a.bih_rebuild(tree, P)
    rebuilt = work(a, cam, lights)
    a.release()
    _, sc_b, _ = spec_commit(gpu_ctx, "s3_20", "tex", P)
    fresh = work(sc_b, cam, lights)
    sc_b.release()
    print("s3_20 SH (bih_nodes, prim_tests), faithful then production: refit", refit, "rebuilt", rebuilt, "fresh", fresh)
    assert rebuilt == fresh
    for (n_r, p_r), (n_s, p_s) in zip(refit, rebuilt):
        assert n_s < n_r and p_s < p_r


def lone(ctx, P):
    b = api.Builder()
    t = b.bih(b.triangles_bulk(P))
    return b, ctx.commit(b, t), t


GROW_CAM = ((20.0, 30.0, 60.0), (30.0, 1.0, 0.0), (0.0, 1.0, 0.0), 70.0)


def grow_answers(sc):
    cam = api.camera(*GROW_CAM)
    lights = [api.light((30.0, 60.0, 40.0), (1.0, 1.0, 1.0), 1e6, True)]
    # rays aimed at the triangles of either pose, from all around each
    rng = np.random.default_rng(7)
    c = np.concatenate([RS.pose_piled().reshape(-1, 3, 3).mean(axis=1), RS.pose_apart().reshape(-1, 3, 3).mean(axis=1)])
    c = np.repeat(c, 25, axis=0) + rng.uniform(-0.05, 0.05, (25 * len(c), 3))
    v = rng.normal(size=c.shape); v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = (c + 12.0 * v).astype(np.float32)
    d = (c - o); d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32); d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    rays = (o, d)
    out = UA.answers(sc, cam, lights, rays, size=(W, H))
    out["work"] = np.array(work(sc, cam, lights))
    return out


def test_growth_takes_new_segments_and_shrink_reuses_them(gpu_ctx):
    A, B = RS.pose_piled(), RS.pose_apart()
    _, sc, t = lone(gpu_ctx, A)
    la = sc.bih_layout(t)
    assert (la["slot_cap"], la["pair_cap"]) == (max(la["slots"], 1), la["pairs"])
    sc.bih_rebuild(t, B)
    lb = sc.bih_layout(t)
    assert lb["slots"] > la["slot_cap"] and lb["pairs"] > la["pair_cap"], (la, lb)
    assert (lb["slot_cap"], lb["pair_cap"]) == (lb["slots"], lb["pairs"]) and sc.info()["n_bih_nodes"] > la["slot_cap"]
    grown = grow_answers(sc)
    _, fresh_sc, _ = lone(gpu_ctx, B)
    fresh = grow_answers(fresh_sc)
    fresh_sc.release()
    assert (grown["t"] >= 0).sum() >= 20
    assert_same(grown, fresh, "A -> B, grown")
    # B -> A: the tree fits into what it has
    sc.bih_rebuild(t, A)
    lc = sc.bih_layout(t)
    assert (lc["slot_cap"], lc["pair_cap"]) == (lb["slot_cap"], lb["pair_cap"]) and (lc["slots"], lc["pairs"]) == (la["slots"], la["pairs"])
    _, fresh_sc, _ = lone(gpu_ctx, A)
    assert_same(grow_answers(sc), grow_answers(fresh_sc), "B -> A, in place")
    fresh_sc.release()
    # and B again: in place now
    sc.bih_rebuild(t, B)
    assert sc.bih_layout(t) == lb
    assert_same(grow_answers(sc), grown, "A -> B -> A -> B")
    sc.release()


def test_a_rebuilt_tree_may_be_deeper_than_anything_the_commit_saw(gpu_ctx):
    import ladder
    comb, flat = RS.comb_and_flat()
    lad = ladder.Ladder()
    cam, lights = product_camera_lights(lad.sd)
    b, sc, t = lone(gpu_ctx, flat)
    shallow = sc.info()["max_bih_depth"]
    sc.bih_rebuild(t, comb)
    assert sc.info()["max_bih_depth"] > max(shallow, 12)  # (beyond the LDS part of the stack: overflow entries now)
    bf, fresh_sc, tf = lone(gpu_ctx, comb)
    assert sc.info()["max_bih_depth"] == fresh_sc.info()["max_bih_depth"] == bf.bih_layout(tf)["depth"]
    rng = np.random.default_rng(3)  # rays up and down the comb, inside its cross-section
    o = np.concatenate([np.full((2000, 1), -1.0), rng.uniform(-0.6 * ladder.W, 0.6 * ladder.W, (2000, 2))], axis=1)
    d = np.concatenate([np.ones((2000, 1)), rng.uniform(-2e-6, 2e-6, (2000, 2))], axis=1)
    o[1000:, 0], d[1000:, 0] = ladder.L + 1.0, -1.0
    o, d = ladder._f32_rays(o, d)
    says = []
    for s in (sc, fresh_sc):
        out = {}
        for faithful in (1, 0):
            img, packed, st = s.render(cam, lights, api.render_params(width=ladder.FRAME_W, height=ladder.FRAME_H, maxdepth=2, faithful=faithful, count_work=1))
            out[f"frame{faithful}"], out[f"packed{faithful}"] = img, packed
            out[f"work{faithful}"] = np.array([int(st["bih_nodes"]), int(st["prim_tests"])])
        hit = s.rayint(o, d)
        out.update({"t": hit["t"], "prim": hit["prim"], "n": np.where(hit["t"][:, None] >= 0, hit["n"], 0)})
        says.append(out)
        s.release()
    assert (says[0]["frame1"][..., 4] < 1e6).sum() >= 20
    assert_same(says[0], says[1], "the comb after a flat commit")


def test_round_trip_renders_the_never_touched_frames(gpu_ctx):
    b, root, tree, cam, lights = build("mixed")
    sc = gpu_ctx.commit(b, root)
    before = frames(sc, cam, lights)
    sc.bih_rebuild(tree, RS.triangles("mixed", "V1"))
    assert not np.array_equal(frames(sc, cam, lights)["frame0"], before["frame0"])
    sc.bih_rebuild(tree, RS.triangles("mixed", "V0"))
    assert_same(frames(sc, cam, lights), before, "V0 -> rebuild(V1) -> rebuild(V0)")
    sc.release()


def test_update_after_rebuild(gpu_ctx):
    b0, root0, tree, cam, lights = build("mixed")
    sc = gpu_ctx.commit(b0, root0)
    sc.bih_rebuild(tree, RS.triangles("mixed", "SH"))
    sc.bih_update(tree, RS.triangles("mixed", "V1"))
    got = answers(sc, cam, lights)
    sc.release()
    b, root, t, _, _ = build("mixed")
    b.bih_set_triangles(t, RS.triangles("mixed", "SH"))
    b.bih_resplit(t)
    b.bih_set_triangles(t, RS.triangles("mixed", "V1"))
    ref_sc = gpu_ctx.commit(b, root)
    assert_same(got, answers(ref_sc, cam, lights), "rebuild(SH), update(V1)")
    ref_sc.release()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_indexed_form(gpu_ctx, dtype):
    """a vertex array with unreferenced vertices that are not finite, and a table that visits the vertices in another order"""
    P = RS.triangles("mixed", "SH")
    rng = np.random.default_rng(3)
    V = P.reshape(-1, 3).astype(dtype)
    order = rng.permutation(len(V))
    verts = np.concatenate([V[order], np.full((2, 3), np.nan, dtype)])
    idx = np.argsort(order).astype(np.int32).reshape(-1, 3)
    assert np.array_equal(verts[idx.reshape(-1)].reshape(-1, 9), P.astype(dtype))
    b0, root0, tree, cam, lights = build("mixed")
    sc = gpu_ctx.commit(b0, root0)
    assert sc.bih_rebuild_indexed(tree, verts, idx) > 0
    got = answers(sc, cam, lights)
    sc.release()
    _, ref_sc, _ = spec_commit(gpu_ctx, "mixed", "tex", P.astype(dtype).astype(np.float64))
    assert_same(got, answers(ref_sc, cam, lights), f"indexed, {np.dtype(dtype).name}")
    ref_sc.release()


@pytest.mark.parametrize("which", ["V1", "SH"])
def test_a_sphere_bih(gpu_ctx, which):
    B0 = SR.build("cloud")
    cam, lights = product_camera_lights(B0.sd)
    S = RS.spheres("cloud", which)
    sc = gpu_ctx.commit(B0.b, B0.root)
    assert sc.sphere_bih_rebuild(B0.tree, S) > 0
    got = answers(sc, cam, lights)
    lay = sc.bih_layout(B0.tree)
    sc.release()
    B = SR.build("cloud")
    B.b.bih_set_spheres(B.tree, S)
    B.b.bih_resplit(B.tree)
    ref_sc = gpu_ctx.commit(B.b, B.root)
    assert (got["t"] >= 0).sum() >= 20
    assert_same(got, answers(ref_sc, cam, lights), f"sphere bih, {which}")
    assert lay["pairs"] == 0 and lay["depth"] == B.b.bih_layout(B.tree)["depth"]
    ref_sc.release()


def test_a_tree_read_from_a_show_text(gpu_ctx):
    sd, b0, nm, tree0 = BR.build("mixed", "V0", "root")
    cam, lights = product_camera_lights(sd)
    text = b0.show(tree0)
    P = RS.triangles("mixed", "SH")
    says = []
    for on_host in (False, True):
        b = api.Builder()
        tree, _ = b.load_show(text)
        if on_host:
            b.bih_set_triangles(tree, P)
            b.bih_resplit(tree)
        sc = gpu_ctx.commit(b, tree)
        if not on_host:
            sc.bih_rebuild(tree, P)
        says.append(answers(sc, cam, lights))
        sc.release()
    assert (says[0]["t"] >= 0).sum() >= 20
    assert_same(says[0], says[1], "a bih read from a show text")


def test_the_device_form_and_a_render_on_the_same_stream(gpu_ctx):
    import torch
    b0, root0, tree, cam, lights = build("mixed")
    P = RS.triangles("mixed", "SH")
    sc = gpu_ctx.commit(b0, root0)
    t = torch.from_numpy(P).cuda()
    assert sc.bih_rebuild(tree, t) > 0
    got = frames(sc, cam, lights)  # (no synchronisation of the caller's in between)
    v = torch.from_numpy(P.reshape(-1, 3)).cuda()
    i = torch.arange(len(P) * 3, dtype=torch.int32).reshape(-1, 3).cuda()
    assert sc.bih_rebuild_indexed(tree, v, i) > 0
    again = frames(sc, cam, lights)
    sc.release()
    _, ref_sc, _ = spec_commit(gpu_ctx, "mixed", "tex", P)
    ref = frames(ref_sc, cam, lights)
    ref_sc.release()
    assert_same(got, ref, "the device form")
    assert_same(again, ref, "the indexed device form")


def test_nested_a_triangle_bih_under_an_outer_bih(gpu_ctx):
    def scene():
        b = api.Builder()
        t = b.bih(b.triangles_bulk(NR.tris9()))
        top = b.bih([t, b.sphere((2.0, 1.0, -1.0), 0.5), b.sphere((4.0, 2.0, 2.0), 0.4), b.sphere((2.0, 3.0, 3.0), 0.3)])
        return b, t, top
    P = RS.shuffled(NR.pose_points(NR.tris9().reshape(-1, 3), "grow").reshape(-1, 9))
    cam = api.camera(*MR.camera_for("V1"))
    lights = [api.light((10.0, 20.0, 10.0), (1.0, 1.0, 1.0), 1e6, True)]
    b, t, top = scene()
    sc = gpu_ctx.commit(b, top)
    with pytest.raises(api.GlomeError, match=r"bih rebuild refused:.*status -1"):  # the plain rule, the update's
        sc.bih_rebuild(t, P)
    sc.nested_updates(True)
    sc.bih_rebuild(t, P)
    assert sc.stale_bihs() == [top]
    assert sc.refit_above(t) > 0 and sc.stale_bihs() == []
    rays = random_rays(3000, 23, center=(0, 1.5, 0), radius=13, spread=7)
    got = UA.answers(sc, cam, lights, rays, hits_only_normals=True, size=(W, H))  # (a miss has no normal: what is stored there is the traversal's leftovers)
    sc.release()
    b2, t2, top2 = scene()
    b2.bih_set_triangles(t2, P)
    b2.bih_resplit(t2)
    b2.bih_refit(top2)
    ref_sc = gpu_ctx.commit(b2, top2)
    assert (got["t"] >= 0).sum() >= 20
    assert_same(got, UA.answers(ref_sc, cam, lights, rays, hits_only_normals=True, size=(W, H)), "nested")
    ref_sc.release()


def test_refusals_leave_the_scene_untouched(gpu_ctx):
    import torch
    lib = L.load()
    b, root, tree, cam, lights = build("mixed")
    sc = gpu_ctx.commit(b, root)
    before = frames(sc, cam, lights)
    lay = sc.bih_layout(tree)
    P = RS.triangles("mixed", "SH")
    nan = P.copy(); nan[17, 4] = np.nan
    V = P.reshape(-1, 3)
    idx = np.arange(len(V), dtype=np.int32).reshape(-1, 3)
    bad = idx.copy(); bad[5, 1] = len(V)
    unchanged = lambda what: (assert_same(frames(sc, cam, lights), before, what), sc.bih_layout(tree) == lay or pytest.fail(what))
    with pytest.raises(api.GlomeError, match=r"is not a bih of plain spheres.*status -1"):
        sc.sphere_bih_rebuild(tree, np.ones((len(P), 4)))
    unchanged("a wrong class")
    with pytest.raises(api.GlomeError, match=rf"the bih has {len(P)} items, not {len(P) - 1}.*status -1"):
        sc.bih_rebuild(tree, P[:-1])
    unchanged("a count mismatch")
    with pytest.raises(api.GlomeError, match=r"not finite.*status -1"):
        sc.bih_rebuild(tree, nan)
    unchanged("a NaN, host form")
    with pytest.raises(api.GlomeError, match=r"not finite.*status -1"):
        sc.bih_rebuild(tree, torch.from_numpy(nan).cuda())
    unchanged("a NaN, device form")
    with pytest.raises(api.GlomeError, match=rf"item 5 has vertex index {len(V)}.*status -1"):
        sc.bih_rebuild_indexed(tree, V, bad)
    unchanged("a bad index, host form")
    with pytest.raises(api.GlomeError, match=r"vertex index outside.*status -1"):
        sc.bih_rebuild_indexed(tree, torch.from_numpy(V.copy()).cuda(), torch.from_numpy(bad).cuda())
    unchanged("a bad index, device form")
    sc.ctx.synchronize()  # (the refused device forms left nothing in the context's error word)
    assert lib.glome_scene_bih_rebuild(sc.h, tree, None, len(P), None) == L.E_INVALID
    unchanged("a null array")
    sc.release()
    # the loop input: build_rec's fixed point needs a box without surface, which a padded triangle never has -- spheres of one centre line
    # and an underflowing radius have it
    S4 = SR.build("cluster")
    cam, lights = product_camera_lights(S4.sd)
    sc = gpu_ctx.commit(S4.b, S4.root)
    before = frames(sc, cam, lights)
    n = len(SR.spheres("cluster"))
    tiny = np.ones((n, 4)); tiny[:, 0] = 1.0 + np.arange(n); tiny[:, 3] = 5e-324  # (c - r == c == c + r: every box a point)
    with pytest.raises(api.GlomeError, match=r"build_rec .* does not terminate.*status -2"):
        sc.sphere_bih_rebuild(S4.tree, tiny)
    assert_same(frames(sc, cam, lights), before, "the loop input")
    with pytest.raises(api.GlomeError, match=r"build_rec .* does not terminate.*status -2"):  # the constructor says the same of it
        b4 = api.Builder()
        b4.bih([b4.sphere((1.0 + k, 1.0, 1.0), 5e-324) for k in range(n)])
    sc.release()


def test_oracle(gpu_ctx):
    b0, root0, tree, _, _ = build("mixed")
    sc = gpu_ctx.commit(b0, root0)
    sc.bih_rebuild(tree, RS.triangles("mixed", "V1"))
    sd, _ = BR.scene_desc("mixed", "V1")
    _, _, nm, _ = BR.build("mixed")
    parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, sd, nm, n=6000)
    cam, lights = product_camera_lights(sd)
    img, packed, st = sc.render(cam, lights, api.render_params(width=96, height=54, maxdepth=2))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 96, 54, 2)
    sc.release()
