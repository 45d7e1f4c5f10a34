"""glome_scene_instance_update_from: the Instance update from poses, forward matrices and pairs, fp64 or fp32, strided, after a base
matrix or not, in its host and its _dev form.  The contract: the call leaves the committed scene bit for bit as the EXISTING
glome_scene_instance_update leaves it when given the 24-double table the host functions (glome_xfm_from_pose, glome_xfm_from_forward,
glome_xfm_mult: test_xfm_sources_host.py) yield for the widened items.  fp32 -> fp64 is exact, so nothing here has a tolerance:
everything two scenes answer is compared bit for bit (NaNs as equal).  Items are rounded to fp32 and widened back so that every dtype
sees the same doubles, and stay away from fp32 subnormals.  What a reference scene answers is computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest

import instances_refit as IR
import nested_refit as NR
import test_instance_update_gpu as TI
import test_nested_update_gpu as TN
import update_sources as US
from helpers import product_camera_lights
from glome_amd import _lib as L
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc
from update_answers import assert_same

pytestmark = pytest.mark.gpu

CENTER = (0.0, 2.2, 0.0)
WIDTH = {"pair": 24, "forward": 12, "pose": 8}
PADDED = {"pair": 29, "forward": 16, "pose": 11}   # forward: a row-major [n, 4, 4] tensor
_reference = {}


# ---- fixtures: (builder, root, the ids an update names, where they stand, the bih that holds them) ----
class Oak2047:
    """scenes.oak at age 11.4, alone: 2,047 Instances (cones, and spheres under a Tex) under one bih -- 31 full 64-lane items and a
    63-lane tail"""

    def __init__(self):
        self.sd = SceneDesc(round32=False)
        top = scenes.oak(self.sd, 11.4, 42)
        self.sd.set_root(top)
        for pos, col in scenes.LIGHTS[:2]:
            self.sd.add_light(pos, col)
        self.sd.set_camera((1.0, 5.0, 9.0), (0.0, 3.5, 0.0), (0.0, 1.0, 0.0), 55.0)
        self.b = api.Builder()
        nm, _ = self.sd.replay(self.b)
        self.root, self.bih = nm[top], nm[top - 2]
        self.ids = self.b.bih_items(self.bih)
        assert len(self.ids) == 2047 and all(IR.is_instance(self.b, i) for i in (self.ids[0], self.ids[1023], self.ids[-1]))
        self.bases = [tuple(self.b.instance_transform(i)[[3, 7, 11]]) for i in self.ids]


def get(name):
    return Oak2047() if name == "oak2047" else TI.get(name)


def center_of(name):
    return (0.0, 3.5, 0.0) if name == "oak2047" else CENTER


# ---- the items of a case, and the table the host functions give for them ----
def small_pose(rng):
    """a sway applied AFTER a base: a turn of a few degrees about an axis near y through the world's origin, a short step, a scale near 1"""
    ax = rng.normal(size=3) * 0.2 + np.array([0.0, 1.0, 0.0])
    half = np.deg2rad(rng.uniform(2.0, 5.0)) / 2
    q = np.concatenate([np.sin(half) * ax / np.linalg.norm(ax), [np.cos(half)]]) * rng.uniform(0.5, 2.0)   # not unit: the library normalises
    return np.concatenate([rng.uniform(-0.15, 0.15, 3), q, [rng.uniform(0.9, 1.1)]])


def own_pose(rng, at):
    """a pose that REPLACES an Instance's matrix: it stands where the Instance stood, turned at random, at a scale of its own"""
    q = rng.normal(size=4)
    return np.concatenate([np.asarray(at) + rng.uniform(-0.2, 0.2, 3), q / np.linalg.norm(q) * rng.uniform(0.5, 2.0), [rng.uniform(0.5, 0.9)]])


def items_of(A, form, with_base, which=None, seed=0):
    """(ids, data [n, width] of float64 values every one of which is an fp32 value, base [n, 24] or None, table [n, 24]): the source of a
    case and what the host functions make of it -- the specification"""
    which = list(range(len(A.ids))) if which is None else list(which)
    ids = [A.ids[k] for k in which]
    rng = np.random.default_rng(4000 + seed)
    base = np.stack([A.b.instance_transform(i) for i in ids]) if with_base else None
    if with_base:
        poses = US.r32(np.stack([small_pose(rng) for _ in ids]))
    elif form == "pose":
        poses = US.r32(np.stack([own_pose(rng, A.bases[k]) for k in which]))
    if with_base or form == "pose":
        full = np.stack([api.xfm_from_pose(p[:3], p[3:7], p[7]) for p in poses])
    else:  # the fixture's own "grow" pose: the Instance's matrix with its sway
        full = IR.moved_matrices(A, "grow", which)[1]
    data = poses if form == "pose" else US.r32(full[:, :12]) if form == "forward" else US.r32(full)
    item = {"pose": lambda v: api.xfm_from_pose(v[:3], v[3:7], v[7]), "forward": api.xfm_from_forward, "pair": lambda v: v.copy()}[form]
    table = np.stack([item(v) for v in data])
    if with_base:
        table = np.stack([api.xfm_mult(t, b) for t, b in zip(table, base)])
    return ids, data, base, table


def laid_out(data, form, dtype, padded):
    """the items as the caller holds them: dense, or inside a wider array whose other values are NaN and 3e38 alternately (for a forward
    matrix the fourth row of a [n, 4, 4] array).  Returns (the array to hand over -- a view of the wide one --, the wide array)."""
    n, w = data.shape
    if not padded:
        a = np.ascontiguousarray(data.astype(dtype))
        return a, a
    wide = np.empty((n, PADDED[form]), dtype=dtype)
    wide[:] = np.where(np.arange(wide.size).reshape(wide.shape) % 2 == 0, np.nan, 3e38).astype(dtype)
    wide[:, :w] = data
    assert wide[:, :w].astype(np.float64).tobytes() == data.tobytes() and not np.isfinite(wide[:, w:]).all()
    return (wide.reshape(n, 4, 4) if form == "forward" else wide[:, :w]), wide


def update_from(ctx, sc, ids, data, base, form, dtype, way, padded, sync=True):
    """the items through the new call: way = host / dev"""
    view, wide = laid_out(data, form, np.float32 if dtype == "f32" else np.float64, padded)
    if way == "host":
        ms = sc.instance_update_from(ids, view, form, base=base)
        assert ms > 0
        return ms
    import torch
    t = torch.tensor(wide, device=torch.device("cuda:0"))
    if padded:
        t = t.reshape(len(ids), 4, 4) if form == "forward" else t[:, :WIDTH[form]]
        assert t.stride(0) == PADDED[form]
    tb = None if base is None else torch.tensor(np.ascontiguousarray(base), dtype=torch.float64, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    assert sc.instance_update_from(ids, t, form, base=tb) is None
    if sync:
        assert sc.lib.glome_ctx_synchronize(ctx.h) == 0, ctx.err()
    return t, tb


def reference(ctx, name, key, ids, table, nested=False):
    """what scene B answers: a second commit of the same fixture, updated through the EXISTING call with the host functions' table"""
    key = (name, nested) + key
    if key not in _reference:
        A = get(name)
        cam, lights = product_camera_lights(A.sd)
        sc = ctx.commit(A.b, A.root)
        if nested:
            sc.nested_updates(True)
        before = TI.frames(sc, cam, lights)
        assert sc.instance_update(ids, table) > 0
        if nested:
            sc.refit_above(ids[0])
            assert sc.stale_bihs() == []
        says = TI.answers(sc, cam, lights, center_of(name))
        sc.release()
        assert not np.array_equal(says["frame0"], before["frame0"]), "the update must show"
        assert (says["t"] >= 0).sum() >= 20 and (says["frame0"][..., 4] < 1e6).sum() >= 20, "the rays and the frame must see the scene"
        _reference[key] = says
    return _reference[key]


THREE = [2, 17, 33]
GROVE_FULL = [("grove", None, form, dtype, way, padded, False) for form in ("pair", "forward", "pose") for dtype in ("f32", "f64") for way in ("host", "dev") for padded in (False, True)]
# (fixture, which movables, form, dtype, way, padded, with a base)
CASES = GROVE_FULL + [
    ("grove", None, "pose", "f32", "dev", False, True), ("grove", None, "pose", "f64", "host", True, True),
    ("grove", None, "forward", "f32", "host", False, True), ("grove", None, "forward", "f64", "dev", True, True),
    ("grove", None, "pair", "f32", "dev", True, True), ("grove", None, "pair", "f64", "host", False, True),
    # 3 of 40: fewer than a 64-lane item, and the named rows' indices are not the items'
    ("grove", THREE, "pose", "f32", "dev", True, False), ("grove", THREE, "pose", "f64", "host", False, True),
    ("grove", THREE, "forward", "f32", "host", True, False), ("grove", THREE, "forward", "f64", "dev", False, False),
    ("grove", THREE, "pair", "f32", "dev", False, True), ("grove", THREE, "pair", "f64", "host", True, False),
    # no bih: slot writes only
    ("flat3", None, "pose", "f32", "dev", False, False), ("flat3", None, "pose", "f64", "host", True, True),
    ("flat3", None, "forward", "f32", "host", True, False), ("flat3", None, "forward", "f64", "dev", False, False),
    ("flat3", None, "pair", "f32", "dev", True, False), ("flat3", None, "pair", "f64", "host", False, True),
    # 2,047 Instances, cones and spheres moved rigidly from where they were built: base = each Instance's own committed matrix
    ("oak2047", None, "pose", "f32", "dev", False, True), ("oak2047", None, "pose", "f32", "host", True, True), ("oak2047", None, "forward", "f64", "dev", True, True),
]


def case_id(c):
    name, which, form, dtype, way, padded, with_base = c
    return "-".join([name + ("3" if which else ""), form, dtype, way, "padded" if padded else "dense", "base" if with_base else "nobase"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_an_update_from_a_source_equals_the_existing_call_on_the_host_functions_table(gpu_ctx, case):
    name, which, form, dtype, way, padded, with_base = case
    A = get(name)
    cam, lights = product_camera_lights(A.sd)
    ids, data, base, table = items_of(A, form, with_base, which)
    sc = gpu_ctx.commit(A.b, A.root)
    held = update_from(gpu_ctx, sc, ids, data, base, form, dtype, way, padded)
    says = TI.answers(sc, cam, lights, center_of(name))
    sc.release()
    del held
    assert_same(says, reference(gpu_ctx, name, (form, with_base, tuple(which or ())), ids, table), case_id(case))


def test_pair_f64_dense_without_a_base_is_the_existing_call(gpu_ctx):
    """the delegation: the layout the existing call takes goes to that call, table and all"""
    A = get("grove")
    cam, lights = product_camera_lights(A.sd)
    ids, M = IR.moved_matrices(A, "shrink")   # (not rounded: the existing call's own doubles)
    says = []
    for new in (True, False):
        sc = gpu_ctx.commit(A.b, A.root)
        assert (sc.instance_update_from(ids, M, "pair") if new else sc.instance_update(ids, M)) > 0
        says.append(TI.answers(sc, cam, lights, CENTER))
        sc.release()
    assert_same(says[0], says[1], "PAIR / F64 / dense / no base")


@pytest.mark.parametrize("way", ["host", "dev"])
@pytest.mark.parametrize("form,dtype,padded", [("pose", "f32", True), ("forward", "f64", False), ("pair", "f32", False)])
def test_under_nested_updates_the_tables_keep_the_converted_matrices(gpu_ctx, form, dtype, padded, way):
    """mixed_nested with the switch on, then bih_refit of the trees above: what the existing call and the same refits give"""
    A = get("mixed_nested")
    cam, lights = product_camera_lights(A.sd)
    ids, data, base, table = items_of(A, form, form == "pose")
    sc = gpu_ctx.commit(A.b, A.root)
    sc.nested_updates(True)
    held = update_from(gpu_ctx, sc, ids, data, base, form, dtype, way, padded, sync=False)
    assert sc.bihs_above(ids[0]) == [A.bih]
    sc.refit_above(ids[0], dev=way == "dev")
    assert sc.stale_bihs() == [] and sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0, gpu_ctx.err()
    says = TI.answers(sc, cam, lights, CENTER)
    sc.release()
    del held
    assert_same(says, reference(gpu_ctx, "mixed_nested", (form, form == "pose", ()), ids, table, nested=True), f"mixed_nested {form} {dtype} {way}")


@pytest.mark.parametrize("way", ["host", "dev"])
def test_a_refit_after_a_mesh_update_reads_the_converted_matrix(gpu_ctx, way):
    """mesh_shared: two Instances of one mesh are items of the root bih.  They are moved by poses after their own matrices with the switch
    on, then the mesh is updated and the tree refitted: the instanced items' boxes are made from the matrices the TREE'S TABLE keeps,
    which must be the converted ones.  Against the same sequence through the existing call."""
    fx = NR.mesh_shared()
    cam, lights = product_camera_lights(fx.sd)
    _, me, V0 = fx.movable[0]
    V1 = NR.pose_points(V0, "grow")
    says = []
    for new in (True, False):
        B = NR.Built(NR.mesh_shared())
        ids = [B.nm[fx.named["i1"]], B.nm[fx.named["i2"]]]
        rng = np.random.default_rng(77)
        poses = US.r32(np.stack([small_pose(rng) for _ in ids]))
        base = np.stack([B.b.instance_transform(i) for i in ids])
        table = np.stack([api.xfm_mult(api.xfm_from_pose(p[:3], p[3:7], p[7]), b) for p, b in zip(poses, base)])
        sc = gpu_ctx.commit(B.b, B.root)
        sc.nested_updates(True)
        before = TN.frames(sc, cam, lights)
        if new:
            held = update_from(gpu_ctx, sc, ids, poses, base, "pose", "f32", way, True, sync=False)
        else:
            assert sc.instance_update(ids, table) > 0
        sc.refit_above(ids[0])
        assert sc.mesh_update(B.nm[me], V1) > 0
        assert sc.stale_bihs() == [B.bihs["root"]]
        assert sc.refit_above(B.nm[me]) > 0 and sc.stale_bihs() == []
        says.append(TN.answers(sc, cam, lights, (0.0, 1.5, 0.0)))
        assert not np.array_equal(says[-1]["frame0"], before["frame0"]), "the update must show"
        sc.release()
    assert (says[0]["t"] >= 0).sum() >= 20
    assert_same(says[0], says[1], "poses after a base, the mesh, the refit")


def test_a_call_between_timing_begin_and_end_reports_one_launch(gpu_ctx):
    import torch
    A = get("grove")
    ids, data, base, table = items_of(A, "pose", True)
    sc = gpu_ctx.commit(A.b, A.root)
    t = torch.tensor(data.astype(np.float32), device="cuda:0")
    tb = torch.tensor(base, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    sc.instance_update_from(ids, t, "pose", base=tb)   # (the first update of the tree allocates its workspace)
    gpu_ctx.synchronize()
    ms = np.zeros(8, np.float32)
    gpu_ctx.lib.glome_ctx_timing_begin(gpu_ctx.h, 8)
    sc.instance_update_from(ids, t, "pose", base=tb)
    assert gpu_ctx.lib.glome_ctx_timing_end(gpu_ctx.h, ms.ctypes.data_as(L.c_fp), 8) == 1 and ms[0] > 0, ms
    gpu_ctx.lib.glome_ctx_timing_begin(gpu_ctx.h, 8)
    sc.instance_update_from(ids, t, "pose", base=tb)
    sc.instance_update_from(ids[:3], t[:3], "pose")
    assert gpu_ctx.lib.glome_ctx_timing_end(gpu_ctx.h, ms.ctypes.data_as(L.c_fp), 8) == 2 and (ms[:2] > 0).all(), ms
    gpu_ctx.synchronize()
    sc.release()


def test_there_and_back_renders_the_never_updated_frame(gpu_ctx):
    """poses that replace the matrices, then PAIR with the committed matrices -- strided, so through the table, not the delegation"""
    A = get("grove")
    cam, lights = product_camera_lights(A.sd)
    sc = gpu_ctx.commit(A.b, A.root)
    before = TI.frames(sc, cam, lights)
    ids, data, _, _ = items_of(A, "pose", False)
    update_from(gpu_ctx, sc, ids, data, None, "pose", "f32", "host", False)
    assert not np.array_equal(TI.frames(sc, cam, lights)["frame0"], before["frame0"])
    own = np.stack([A.b.instance_transform(i) for i in ids])
    assert own.tobytes() == IR.original_matrices(A)[1].tobytes()
    held = update_from(gpu_ctx, sc, ids, own, None, "pair", "f64", "dev", True)
    assert_same(TI.frames(sc, cam, lights), before, "there and back")
    del held
    sc.release()


# ---- bad input ----
def spoiled(A, what):
    """(form, data, k, status of the host form, what its message says) -- item k of an otherwise valid source spoiled"""
    form = "forward" if what == "singular" else "pair" if what == "nan_pair" else "pose"
    ids, data, base, table = items_of(A, form, False)
    bad = data.copy()
    k = 7
    if what == "zero_quaternion":
        bad[k, 3:7] = 0.0
    elif what == "zero_scale":
        bad[k, 7] = 0.0
    elif what == "negative_scale":
        bad[k, 7] = -0.5
    elif what == "singular":
        bad[k, 8:11] = bad[k, 4:7]   # two equal rows: every cofactor product cancels exactly, det = 0
    elif what == "nan_pose":
        bad[k, 1] = np.nan
    else:
        bad[k, 17] = np.nan
    msg = {"zero_quaternion": "quaternion has length 0", "zero_scale": "scale is not positive", "negative_scale": "scale is not positive",
           "singular": "forward matrix is singular", "nan_pose": "is not finite", "nan_pair": "is not finite"}[what]
    return form, ids, data, bad, k, (L.E_SCENE if what == "singular" else L.E_INVALID), msg, table


BAD = ["zero_quaternion", "zero_scale", "negative_scale", "singular", "nan_pose", "nan_pair"]


@pytest.mark.parametrize("what", BAD)
def test_bad_items_through_the_host_form_leave_the_scene_as_it_was(gpu_ctx, what):
    A = get("grove")
    cam, lights = product_camera_lights(A.sd)
    form, ids, data, bad, k, status, msg, _ = spoiled(A, what)
    sc = gpu_ctx.commit(A.b, A.root)
    before = TI.frames(sc, cam, lights)
    for dtype in (np.float32, np.float64):
        with pytest.raises(api.GlomeError, match=rf"node {ids[k]}\b.*{msg}.*status {status}|{msg}.*node {ids[k]}\b.*status {status}"):
            sc.instance_update_from(ids, bad.astype(dtype), form)
    assert_same(TI.frames(sc, cam, lights), before, f"{what} through the host form")
    sc.release()


@pytest.mark.parametrize("what", BAD)
def test_bad_items_are_found_on_the_device_and_a_valid_update_mends_the_scene(gpu_ctx, what):
    """Every one of these only raises the sticky error word: the conversion reads its own item and writes its own row whatever the values
    are, and no index anywhere depends on a value."""
    import torch
    A = get("grove")
    cam, lights = product_camera_lights(A.sd)
    form, ids, data, bad, k, _, _, table = spoiled(A, what)
    sc = gpu_ctx.commit(A.b, A.root)
    tb, tg = (torch.tensor(x.astype(np.float32), device="cuda:0") for x in (bad, data))
    torch.cuda.synchronize()
    assert sc.instance_update_from(ids, tb, form) is None
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == L.E_INVALID
    assert "glome_scene_instance_update_from_dev" in gpu_ctx.err() and "glome_scene_instance_update," in gpu_ctx.err()
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0  # (the word is cleared where it is read)
    assert sc.instance_update_from(ids, tg, form) is None
    assert sc.lib.glome_ctx_synchronize(gpu_ctx.h) == 0, gpu_ctx.err()
    says = TI.answers(sc, cam, lights, CENTER)
    sc.release()
    assert_same(says, reference(gpu_ctx, "grove", (form, False, ()), ids, table), f"a valid update after {what}")


def test_both_forms_refuse_a_bad_source_before_anything_is_launched(gpu_ctx):
    A = get("grove")
    cam, lights = product_camera_lights(A.sd)
    ids, data, base, table = items_of(A, "pose", False)
    sc = gpu_ctx.commit(A.b, A.root)
    before = TI.frames(sc, cam, lights)
    lib = sc.lib
    _, pi = L.ivec(ids)
    d32 = np.ascontiguousarray(data.astype(np.float32))
    n = len(ids)

    def src(**kw):
        s = L.XfmSource()
        s.data, s.base, s.dtype, s.form, s.stride = d32.ctypes.data, None, L.F32, L.XFM_POSE, 0
        for key, v in kw.items():
            setattr(s, key, v)
        return s

    def both(s, pids=pi, count=n):
        ps = None if s is None else C.byref(s)
        # (the _dev form is handed host pointers: it refuses before it looks at one)
        return lib.glome_scene_instance_update_from(sc.h, pids, ps, count, None), lib.glome_scene_instance_update_from_dev(sc.h, pids, ps, count)

    for s, why in ((None, "null array"), (src(data=None), "null array"), (src(form=3), "form 3 is none of"), (src(form=-1), "form -1 is none of"),
                   (src(dtype=2), "dtype 2 is neither"), (src(stride=-8), "stride -8 is negative"), (src(stride=7), "stride 7 is less than the form's 8"),
                   (src(form=L.XFM_FORWARD, stride=11), "stride 11 is less than the form's 12"), (src(form=L.XFM_PAIR, stride=23), "stride 23 is less than the form's 24")):
        for rc in both(s):
            assert rc == L.E_INVALID and why in gpu_ctx.err(), (why, rc, gpu_ctx.err())
    # what the existing call refuses stays refused, with its messages
    assert both(src(), pids=None) == (L.E_INVALID, L.E_INVALID) and "bad count or null array" in gpu_ctx.err()
    assert both(src(), count=-1) == (L.E_INVALID, L.E_INVALID)
    twice = ids[:2] + ids[:1]
    _, p2 = L.ivec(twice)
    assert both(src(), pids=p2, count=3) == (L.E_INVALID, L.E_INVALID) and f"node {ids[0]} is named more than once" in gpu_ctx.err()
    _, pb = L.ivec([A.bih])
    assert both(src(), pids=pb, count=1) == (L.E_INVALID, L.E_INVALID) and f"node {A.bih} is not an Instance of this scene" in gpu_ctx.err()
    assert both(src(), count=0) == (0, 0) and both(None, count=0) == (0, 0)   # nothing named: nothing to refuse
    # a converted matrix that fails check_xfm, and a count that does not match, through the Python side
    corrupt = US.r32(IR.moved_matrices(A, "grow")[1]); corrupt[2, :12] *= 2.0
    with pytest.raises(api.GlomeError, match=rf"node {ids[2]}: corrupt matrix.*status -1"):
        sc.instance_update_from(ids, corrupt.astype(np.float32), "pair")
    with pytest.raises(api.GlomeError, match=rf"{n} ids but {n - 1} items"):
        sc.instance_update_from(ids, data[:-1], "pose")
    with pytest.raises(api.GlomeError, match=r"form 'euler' is none of"):
        sc.instance_update_from(ids, data, "euler")
    import torch
    with pytest.raises(api.GlomeError, match=r"data must be a CUDA torch.float32 or torch.float64 tensor"):
        sc.instance_update_from(ids, torch.zeros(n, 8, dtype=torch.float16, device="cuda:0"), "pose")
    with pytest.raises(api.GlomeError, match=r"inner dimensions of data must be contiguous"):
        sc.instance_update_from(ids, torch.zeros(n, 16, dtype=torch.float32, device="cuda:0")[:, ::2], "pose")
    gpu_ctx.synchronize()
    assert_same(TI.frames(sc, cam, lights), before, "the refusals of both forms")
    sc.release()


def test_an_item_box_that_reaches_infinity_through_a_pose(gpu_ctx):
    """the checks of the existing host form run on the CONVERTED matrix: a plane's Instance shifted by delta is `bih`'s own refusal"""
    b = api.Builder()
    pl, tree = IR.plane_bih(b)
    sc = gpu_ctx.commit(b, tree)
    bad = np.array([[1e-4, 0, 0, 0, 0, 0, 1, 1]], dtype=np.float64)
    assert api.xfm_from_pose(bad[0, :3], bad[0, 3:7], 1.0).tobytes() == api.translate((1e-4, 0, 0)).tobytes()
    with pytest.raises(api.GlomeError, match=rf"node {pl} in bih {tree}: bih: infinite bounding box.*status -2"):
        sc.instance_update_from([pl], bad, "pose")
    sc.release()
