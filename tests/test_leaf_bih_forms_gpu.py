"""GPU suite (-m gpu): the ten update and six rebuild entry points of a committed leaf bih -- glome_scene_bih_update / _f32 / _indexed,
glome_scene_sphere_bih_update / _f32, glome_scene_bih_rebuild / _indexed, glome_scene_sphere_bih_rebuild, each with its _dev twin -- as
plumbing, at the C ABI: the order in which they refuse and the full text of each refusal, what a refused call does to *gpu_ms and to the
scene, that the host form and the device form of a call leave the same scene bit for bit, and an update's workspace across a rebuild that
outgrows it.  What the calls compute is held elsewhere (test_bih_update_gpu.py, test_sphere_bih_update_gpu.py, test_update_sources_gpu.py,
test_bih_rebuild_gpu.py).

Scenes: bihs_refit's "mixed" (297 triangles) under a Tex, spheres_refit's "cluster" (40 spheres), the 41-triangle lone bih of
bihs_resplit's two poses, and each class once under an outer bih.  Frames are 128 x 96.  Every refusal here is decided on the host or by
the rebuild's own flag word: none faults the device, and none is an update's deferred report of a bad value."""
import ctypes as C

import numpy as np
import pytest

import bihs_refit as BR
import bihs_resplit as RS
import spheres_refit as SR
import update_answers as UA
from helpers import product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api
from update_answers import assert_same, frames

pytestmark = pytest.mark.gpu

W, H = 128, 96
SENTINEL = -7.5
SUFFIX = {"dense64": "", "dense32": "_f32", "indexed": "_indexed", "sph64": "", "sph32": "_f32"}


class EP:
    """an entry point: the class of bih it is for, the form of its source, update or rebuild, host or device form"""

    def __init__(self, form, rebuild, host):
        self.form, self.rebuild, self.host = form, rebuild, host
        self.sphere = form.startswith("sph")
        self.word = "sphere" if self.sphere else "triangle"
        self.name = ("sphere_" if self.sphere else "") + "bih_" + ("rebuild" if rebuild else "update") + SUFFIX[form] + ("" if host else "_dev")
        self.what = ("sphere " if self.sphere else "") + ("bih rebuild" if rebuild else "bih update")
        self.has_ms = host or rebuild

    def __repr__(self):
        return self.name


UPDATES = [EP(f, False, h) for f in SUFFIX for h in (True, False)]
REBUILDS = [EP(f, True, h) for f in ("dense64", "indexed", "sph64") for h in (True, False)]
ALL = UPDATES + REBUILDS
assert len(UPDATES) == 10 and len(REBUILDS) == 6 and len({e.name for e in ALL}) == 16


def source(form, V):
    """the arguments of a call between the bih's id and the item count, as NumPy arrays: V is n x 9 (triangles) or n x 4 (spheres), float64"""
    V = np.ascontiguousarray(V, dtype=np.float64)
    if form in ("dense64", "sph64"):
        return [V.copy()]
    if form == "dense32":
        return [V.astype(np.float32)]
    if form == "indexed":
        return [V.reshape(-1, 3).copy(), L.F64, 3 * len(V), np.arange(3 * len(V), dtype=np.int32).reshape(-1, 3)]
    return [np.ascontiguousarray(V[:, :3], dtype=np.float32), np.ascontiguousarray(V[:, 3], dtype=np.float32)]


def call(ep, h, bih_id, src, n, ms=SENTINEL):
    """the C call: arrays go as they are to a host form and as CUDA tensors to a device form.  Returns (status, *gpu_ms afterwards or None)"""
    import torch
    fn = getattr(L.load(), "glome_scene_" + ep.name)
    held = [torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) and not ep.host else a for a in src]
    args = []
    for k, a in enumerate(held + [int(n)]):
        if isinstance(a, np.ndarray):
            a = a.ctypes.data_as(fn.argtypes[2 + k])
        elif hasattr(a, "data_ptr"):
            a = C.c_void_p(a.data_ptr())
        args.append(a)
    out = C.c_float(ms)
    rc = fn(h, int(bih_id), *args, *([C.byref(out)] if ep.has_ms else []))
    if not ep.host:
        torch.cuda.synchronize()  # (the tensors outlive what read them)
    return rc, (out.value if ep.has_ms else None)


class Held:
    """a committed scene, its leaf bih, and what it answered at commit"""

    def __init__(self, ctx, b, root, tree, cam, lights, V0, above=None):
        self.ctx, self.b, self.tree, self.cam, self.lights, self.V0, self.above = ctx, b, tree, cam, lights, V0, above
        self.n = len(V0)
        self.sc = ctx.commit(b, root)
        self.frames0, self.layout0 = frames(self.sc, cam, lights, (W, H)), self.sc.bih_layout(tree)

    def unchanged(self, what):
        assert self.sc.bih_layout(self.tree) == self.layout0, what
        assert_same(frames(self.sc, self.cam, self.lights, (W, H)), self.frames0, what)


def tri_scene(ctx):
    sd, b, nm, tree = BR.build("mixed", "V0", "tex")
    return Held(ctx, b, nm[sd.root], tree, *product_camera_lights(sd), BR.triangles("mixed", "V0"))


def sph_scene(ctx):
    B = SR.build("cluster")
    return Held(ctx, B.b, B.root, B.tree, *product_camera_lights(B.sd), SR.spheres("cluster"))


GROW_CAM = ((20.0, 30.0, 60.0), (30.0, 1.0, 0.0), (0.0, 1.0, 0.0), 70.0)
GROW_LIGHTS = [((30.0, 60.0, 40.0), (1.0, 1.0, 1.0), 1e6, True)]


def two_level(P):
    """test_bih_rebuild_gpu.py's nested scene over the triangles P: the triangle bih beside three spheres under an outer bih"""
    b = api.Builder()
    t = b.bih(b.triangles_bulk(P))
    top = b.bih([t, b.sphere((2.0, 1.0, -1.0), 0.5), b.sphere((4.0, 2.0, 2.0), 0.4), b.sphere((2.0, 3.0, 3.0), 0.3)])
    return b, t, top


def nested_tri_scene(ctx):
    b, t, top = two_level(RS.pose_piled())
    return Held(ctx, b, top, t, api.camera(*GROW_CAM), [api.light(*l) for l in GROW_LIGHTS], RS.pose_piled(), above=top)


def nested_sph_scene(ctx):
    B = SR.build_nested("cluster")
    return Held(ctx, B.b, B.root, B.tree, *product_camera_lights(B.sd), SR.spheres("cluster"), above=B.top)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """the scenes the refusals are tried on: none of them ever changes"""
    w = {False: tri_scene(gpu_ctx), True: sph_scene(gpu_ctx), ("nested", False): nested_tri_scene(gpu_ctx), ("nested", True): nested_sph_scene(gpu_ctx)}
    yield w
    for s in w.values():
        s.sc.release()


# ---------------------------------------------------------------- 1. the order of the refusals, their texts, *gpu_ms, the scene
def refused(ep, S, src, n, text, status=L.E_INVALID, ms_after=None, bih_id=None):
    """the call is refused with exactly `text`; *gpu_ms afterwards is ms_after (default: zeroed by a host form, kept by a device form);
    the scene is as it was"""
    rc, ms = call(ep, S.sc.h, S.tree if bih_id is None else bih_id, src, n)
    assert (rc, S.ctx.err()) == (status, text), (ep, rc, S.ctx.err())
    if ep.has_ms:
        want = ms_after if ms_after is not None else (0.0 if ep.host else SENTINEL)
        assert ms == want, (ep, text, ms)
    S.unchanged(f"{ep.name}: {text}")


@pytest.mark.parametrize("ep", ALL, ids=repr)
def test_what_both_forms_refuse_in_order(world, ep):
    S, other, nest = world[ep.sphere], world[not ep.sphere], world[("nested", ep.sphere)]
    good = lambda of=S: source(ep.form, of.V0)
    null_items = lambda src: src[:3] + [None] if ep.form == "indexed" else [None] + src[1:]
    # a null scene before everything, and *gpu_ms is not touched
    rc, ms = call(ep, None, other.tree, null_items(good()), S.n - 1)
    assert rc == L.E_INVALID and ms in (None, SENTINEL)
    # the class before the count: the other scene's bih, and a count that is not its own
    assert other.n != S.n - 1
    refused(ep, other, good(), S.n - 1, f"{ep.what}: node {other.tree} is not a bih of plain {ep.word}s of this scene")
    refused(ep, S, good(), S.n, f"{ep.what}: node {S.tree + 1000} is not a bih of plain {ep.word}s of this scene", bih_id=S.tree + 1000)
    # the count before the null item array
    refused(ep, S, null_items(good()), S.n - 1, f"{ep.what}: the bih has {S.n} items, not {S.n - 1}")
    # the null item array before the plain rule (the nested scene, its switch off), and the plain rule before what follows
    rule = f"{ep.what} refused: bih {nest.tree} lies inside bih {nest.above}, whose planes and root box were built from its bound"
    refused(ep, nest, null_items(good(nest)), nest.n, f"{ep.what}: null {ep.word} array")
    refused(ep, S, null_items(good()), S.n, f"{ep.what}: null {ep.word} array")
    src = good(nest)
    if ep.form == "indexed":
        src[1] = 7
    elif ep.form == "sph32":
        src[1] = None
    elif ep.host or ep.rebuild:
        src[0][3, 1] = np.nan  # (a host form's validation, a rebuild's flag word; an update's device form would report it later: it gets good values)
    refused(ep, nest, src, nest.n, rule)
    if ep.form == "sph32":  # the radii after the rule, before the values
        src = good()
        src[0][2, 0] = np.nan
        refused(ep, S, [src[0], None], S.n, f"{ep.what}: null radius array")
    if ep.form == "indexed":  # dtype, then the vertex array, then the count of vertices, then the values
        src = good()
        src[1], src[2] = 7, -1
        refused(ep, S, src, S.n, f"{ep.what}: dtype 7 is neither GLOME_F64 nor GLOME_F32")
        src = good()
        src[2] = -1  # (every index lies outside it, too)
        refused(ep, S, src, S.n, f"{ep.what}: null vertex array")
        src = good()
        src[0] = None
        refused(ep, S, src, S.n, f"{ep.what}: null vertex array")
        src = good()
        src[0], src[2] = None, 0
        refused(ep, S, src, S.n, f"{ep.what}: {S.n} items index an array of no vertices")
    S.ctx.synchronize()  # (no refusal left anything in the context's error word)


@pytest.mark.parametrize("ep", [e for e in ALL if e.host], ids=repr)
def test_a_host_form_refuses_the_first_bad_value(world, ep):
    S = world[ep.sphere]
    V = S.V0
    if ep.form in ("dense64", "dense32"):
        src = source(ep.form, V)
        src[0][17, 4], src[0][3, 0] = np.nan, np.inf
        refused(ep, S, src, S.n, f"{ep.what}: a vertex coordinate is not finite")
    elif ep.form == "indexed":
        for dtype, code in ((np.float64, L.F64), (np.float32, L.F32)):
            src = source(ep.form, V)
            src[0], src[1] = np.concatenate([src[0].astype(dtype), np.full((1, 3), np.nan, dtype)]), code  # (an unreferenced vertex may be anything)
            src[2] += 1
            nv = src[2]
            src[3][5, 1] = nv  # item 5: outside; item 7: a vertex that is not finite
            src[0][21, 2] = np.inf
            assert src[3][7, 0] == 21
            refused(ep, S, src, S.n, f"{ep.what}: item 5 has vertex index {nv}, outside [0, {nv})")
            src[3][5, 1], src[3][9, 2] = 16, -1
            refused(ep, S, src, S.n, f"{ep.what}: a vertex coordinate is not finite (vertex 21, of item 7)")
            src[0][21, 2] = 0.0
            refused(ep, S, src, S.n, f"{ep.what}: item 9 has vertex index -1, outside [0, {nv})")
    elif ep.form == "sph64":
        src = source(ep.form, V)
        src[0][0, 3], src[0][5, 1] = 0.0, np.nan  # every value is looked at before any radius
        refused(ep, S, src, S.n, f"{ep.what}: a value is not finite")
        src[0][5, 1] = 1.0
        src[0][3, 3] = -1.0
        refused(ep, S, src, S.n, f"{ep.what}: radius of item 0 is not positive")
        src[0][0, 3] = 1.0
        refused(ep, S, src, S.n, f"{ep.what}: radius of item 3 is not positive")
    else:
        src = source(ep.form, V)
        src[1][0], src[1][2] = 0.0, np.inf
        refused(ep, S, src, S.n, f"{ep.what}: a value is not finite")
        src[1][2] = 1.0
        src[0][39, 2] = np.nan
        refused(ep, S, src, S.n, f"{ep.what}: a value is not finite")
        src[0][39, 2] = 1.0
        refused(ep, S, src, S.n, f"{ep.what}: radius of item 0 is not positive")
        src[1][0], src[1][3] = 1.0, -2.0
        refused(ep, S, src, S.n, f"{ep.what}: radius of item 3 is not positive")


@pytest.mark.parametrize("ep", [e for e in REBUILDS if not e.host], ids=repr)
def test_a_rebuild_device_form_refuses_by_its_flag_word(world, ep):
    """after every host-side refusal; *gpu_ms has been zeroed by then"""
    S = world[ep.sphere]
    V = RS.spheres("cluster", "SH") if ep.sphere else RS.triangles("mixed", "SH")
    if ep.form == "dense64":
        src = source(ep.form, V)
        src[0][17, 4] = np.nan
        refused(ep, S, src, S.n - 1, f"{ep.what}: the bih has {S.n} items, not {S.n - 1}")
        refused(ep, S, src, S.n, f"{ep.what}: a vertex coordinate is not finite", ms_after=0.0)
    elif ep.form == "indexed":
        src = source(ep.form, V)
        src[0][21, 2] = np.nan
        bad_dtype = list(src)
        bad_dtype[1] = 7
        refused(ep, S, bad_dtype, S.n, f"{ep.what}: dtype 7 is neither GLOME_F64 nor GLOME_F32")
        refused(ep, S, src, S.n, f"{ep.what}: a vertex coordinate is not finite", ms_after=0.0)
        src[3][5, 1] = src[2]  # an index outside the array is told before a value that is not finite, wherever either is
        refused(ep, S, src, S.n, f"{ep.what}: an item has a vertex index outside the vertex array", ms_after=0.0)
        src[3][5, 1], src[3][2, 0] = 16, -1
        refused(ep, S, src, S.n, f"{ep.what}: an item has a vertex index outside the vertex array", ms_after=0.0)
    else:
        src = source(ep.form, V)
        src[0][5, 1] = np.nan
        refused(ep, S, src, S.n, f"{ep.what}: a value is not finite or a radius is not positive", ms_after=0.0)
        src = source(ep.form, V)
        src[0][3, 3] = 0.0
        refused(ep, S, src, S.n, f"{ep.what}: a value is not finite or a radius is not positive", ms_after=0.0)
    S.ctx.synchronize()


# ---------------------------------------------------------------- 2. host form against device form
RAYS = random_rays(1000, 23, center=(0, 1.5, 0), radius=13, spread=7)


@pytest.mark.parametrize("form,rebuild", [(f, False) for f in SUFFIX] + [(f, True) for f in ("dense64", "indexed", "sph64")], ids=lambda v: {True: "rebuild", False: "update"}.get(v, v))
def test_host_form_and_device_form_leave_the_same_scene(gpu_ctx, form, rebuild):
    sphere = form.startswith("sph")
    which = "SH" if rebuild else "V1"
    V = RS.spheres("cluster", which) if sphere else RS.triangles("mixed", which)
    src = source(form, V)
    if form == "indexed":  # float32 vertices, in another order than the table visits them
        order = np.random.default_rng(3).permutation(len(src[0]))
        src = [src[0].astype(np.float32)[order], L.F32, src[2], np.argsort(order).astype(np.int32).reshape(-1, 3)]
    says, lays = [], []
    for host in (True, False):
        ep = EP(form, rebuild, host)
        S = (sph_scene if sphere else tri_scene)(gpu_ctx)
        rc, ms = call(ep, S.sc.h, S.tree, src, S.n)
        assert rc == 0, (ep, gpu_ctx.err())
        assert ms is None or ms > 0
        gpu_ctx.synchronize()
        says.append(UA.answers(S.sc, S.cam, S.lights, RAYS, size=(W, H)))
        lays.append(S.sc.bih_layout(S.tree))
        assert not np.array_equal(says[-1]["frame0"], S.frames0["frame0"]), "the call must show in the frame"
        S.sc.release()
    assert (says[0]["t"] >= 0).sum() >= 20
    assert_same(says[0], says[1], f"{form}, {'rebuild' if rebuild else 'update'}: host form, device form")
    assert lays[0] == lays[1]


# ---------------------------------------------------------------- 3. an update's workspace across a rebuild that outgrows it
def aimed_answers(sc, hits_only_normals=False):
    """rays aimed at the triangles of either pose of the lone bih, from all around each; the frame from GROW_CAM"""
    rng = np.random.default_rng(7)
    c = np.concatenate([RS.pose_piled().reshape(-1, 3, 3).mean(axis=1), RS.pose_apart().reshape(-1, 3, 3).mean(axis=1)])
    c = np.repeat(c, 25, axis=0) + rng.uniform(-0.05, 0.05, (25 * len(c), 3))
    v = rng.normal(size=c.shape); v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = (c + 12.0 * v).astype(np.float32)
    d = c - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return UA.answers(sc, api.camera(*GROW_CAM), [api.light(*l) for l in GROW_LIGHTS], (o, d), hits_only_normals=hits_only_normals, size=(W, H))


def test_the_update_after_a_rebuild_that_outgrew_its_workspace(gpu_ctx):
    """bih_update(A) allocates the workspace for A's tree; bih_rebuild(B) grows the tree, so the workspace goes; bih_update(B) makes a larger one"""
    A, B = RS.pose_piled(), RS.pose_apart()
    b = api.Builder()
    t = b.bih(b.triangles_bulk(A))
    sc = gpu_ctx.commit(b, t)
    la = sc.bih_layout(t)
    assert sc.bih_update(t, A) > 0
    assert sc.bih_rebuild(t, B) > 0
    lb = sc.bih_layout(t)
    assert lb["slots"] > la["slots"] and lb["records"] == la["records"], (la, lb)
    assert sc.bih_update(t, B) > 0
    got = aimed_answers(sc)
    sc.release()
    b = api.Builder()
    t = b.bih(b.triangles_bulk(B))
    fresh = gpu_ctx.commit(b, t)
    want = aimed_answers(fresh)
    fresh.release()
    assert (got["t"] >= 0).sum() >= 20
    assert_same(got, want, "update(A), rebuild(B), update(B) against a commit of B")


def test_the_same_under_an_outer_bih_with_nested_updates(gpu_ctx):
    A, B = RS.pose_piled(), RS.pose_apart()
    b, t, top = two_level(A)
    sc = gpu_ctx.commit(b, top)
    sc.nested_updates(True)
    la = sc.bih_layout(t)
    assert sc.bih_update(t, A) > 0
    assert sc.bih_rebuild(t, B) > 0
    lb = sc.bih_layout(t)
    assert lb["slots"] > la["slots"], (la, lb)
    assert sc.bih_update(t, B) > 0
    assert sc.stale_bihs() == [top]
    assert sc.refit_above(t) > 0 and sc.stale_bihs() == []
    got = aimed_answers(sc, hits_only_normals=True)  # (a miss has no normal: what is stored there is the traversal's leftovers)
    sc.release()
    b2, t2, top2 = two_level(A)
    b2.bih_set_triangles(t2, B)
    b2.bih_resplit(t2)
    b2.bih_refit(top2)
    ref = gpu_ctx.commit(b2, top2)
    want = aimed_answers(ref, hits_only_normals=True)
    ref.release()
    assert (got["t"] >= 0).sum() >= 20
    assert_same(got, want, "nested: update(A), rebuild(B), update(B), refit above")
