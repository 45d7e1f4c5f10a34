"""Which kernel instance a trace launch gets (glome_amd/csrc/instances.hpp choose_trace), seen through the host-only export
glome_trace_kernel_choice -- no GPU is touched.

The rule is choose_render's without the two-row instance; here it is stated a second time, independently, in numpy, and the export
must agree with it on every point of the grid of scene traits tests/test_kernel_choice.py uses, times faithful, count_work and
maxdepth.  The second test pins the instances of five scenes; its table doubles as documentation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import zoo
from glome_amd import _lib as L
from glome_amd import api, scenes

CLS_BIH_TRI, CLS_BIH_SPHERE, CLS_BIH_SIMPLE, CLS_MESH, CLS_PRIMS, CLS_ALL, CLS_CSG, CLS_EVERY = 1, 2, 4, 8, 16, 31, 32, 63  # rt_types.h
ASM_LDS_CAP = 12  # kAsmLdsCap
CSG_LB = 2        # GLOME_CSG_LB
COLS = ("tier", "cls_mask", "sec", "nested", "refract", "pk_all", "stack_cap", "n_bih_nodes", "faithful", "count_work", "maxdepth")


def flat_key(F, Cn, U, cls, lb):  # render_flat_key with TWO_ROWS = false
    return (F * 1) | (Cn * 2) | (U * 4) | (lb << 4) | (cls << 8)


def rule(g):
    """g: dict of int64 arrays (COLS) -> (instance, lb, wave slots per CU): section "the trace seam" of DESIGN.md"""
    m, depth = g["cls_mask"], g["maxdepth"]
    sec, nested, refract = (g[k] != 0 for k in ("sec", "nested", "refract"))
    # the smallest class that covers the scene's entry classes
    with_csg = np.where((m & ~(CLS_CSG | CLS_PRIMS)) == 0, CLS_CSG | CLS_PRIMS, CLS_EVERY)
    without = np.where((m & ~CLS_BIH_TRI) == 0, CLS_BIH_TRI,
                       np.where((m & ~(CLS_BIH_SPHERE | CLS_PRIMS)) == 0, CLS_BIH_SPHERE | CLS_PRIMS, np.where((m & ~CLS_MESH) == 0, CLS_MESH, CLS_ALL)))
    cls = np.where((m & CLS_CSG) != 0, with_csg, without)
    faithful = (g["faithful"] != 0) | (refract & (depth > 1))  # asked for, or a Refract material traced deeper than the primary ray
    count = (g["count_work"] != 0) | faithful
    full = nested | (sec & (depth > 1))
    lb_cls = np.where(cls == CLS_EVERY, 2, np.where(cls == (CLS_CSG | CLS_PRIMS), CSG_LB, 1))
    key = np.select([faithful, count], [flat_key(1, 1, full, CLS_EVERY, 1), flat_key(0, 1, full, CLS_EVERY, 1)], default=flat_key(0, 0, full, cls, lb_cls))
    lb = np.where(faithful | count, 1, lb_cls)
    generic = g["tier"] != 0
    return np.where(generic, np.where(g["count_work"] != 0, -1, -2), key), np.where(generic, 2, lb), np.full(m.shape, 32)


def export_choice(lib, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.full((rows.shape[0], 3), -99, dtype=np.int32)
    assert lib.glome_trace_kernel_choice(rows.shape[0], rows.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == rows.shape[0]
    return out


def test_trace_choice_equals_the_rule_on_the_whole_grid(built):
    lib = L.load()
    axes = [(0, 1), range(64), (0, 1), (0, 1), (0, 1), (0, 1), (ASM_LDS_CAP, 8), (500000, 500001), (0, 1), (0, 1), (1, 2)]
    rows = np.array(list(itertools.product(*axes)), dtype=np.int64)
    assert rows.shape == (2 * 64 * 16 * 2 * 2 * 2 * 2 * 2, 11)
    got = export_choice(lib, rows)
    g = {k: rows[:, i] for i, k in enumerate(COLS)}
    for name, want, col in zip(("instance", "lb", "wave cap"), rule(g), range(3)):
        bad = np.flatnonzero(got[:, col] != want)
        assert bad.size == 0, (name, bad.size, [dict(zip(COLS, rows[i].tolist())) for i in bad[:4]], got[bad[:4]].tolist(), want[bad[:4]].tolist())
    flat = got[:, 0] >= 0
    assert np.array_equal(~flat, g["tier"] != 0)         # generic exactly when the scene is on the generic tier
    assert flat.any() and not np.any(got[flat, 0] & 8)   # bit 3, TWO_ROWS: never
    assert set(np.unique(got[~flat, 0])) == {-1, -2}
    assert lib.glome_trace_kernel_choice(1, None, None) == L.E_INVALID
    assert lib.glome_trace_kernel_choice(0, None, None) == 0


CLS_NAMES = {CLS_BIH_TRI: "TRI", CLS_BIH_SPHERE | CLS_PRIMS: "SPHERE|PRIMS", CLS_MESH: "MESH", CLS_ALL: "ALL", CLS_CSG | CLS_PRIMS: "CSG|PRIMS", CLS_EVERY: "EVERY"}


def instance_name(inst):
    if inst < 0:
        return "k_trace_batch_generic" + ("<counting>" if inst == -1 else "<lean>")
    F, Cn, U, two, lb, cls = inst & 1, (inst >> 1) & 1, (inst >> 2) & 1, (inst >> 3) & 1, (inst >> 4) & 15, CLS_NAMES[inst >> 8]
    assert not two
    b = lambda x: "true" if x else "false"
    return f"k_trace_batch_flat<{b(F)},{b(Cn)},{b(U)},{cls},{lb}>"  # <FAITHFUL, COUNT, FULL, CLS, LB>


# (scene, faithful, count_work, maxdepth) -> instance.  S1: a plane and a sphere BIH, some spheres mirrors -- full from maxdepth 2; S3: one triangle BIH -- the class
# instance, one wave per SIMD asked of the allocator, NOT the frame's two-row flagship; S4: CSG items and primitives with a Reflect material,
# full from maxdepth 2; materials: a Refract material, so the reference's own traversal from maxdepth 2 (and nested materials: full at any
# depth); testscene: the generic tier.
TRACE_INSTANCES = {
    ("S1", 0, 0, 1): "k_trace_batch_flat<false,false,false,SPHERE|PRIMS,1>",
    ("S1", 0, 0, 3): "k_trace_batch_flat<false,false,true,SPHERE|PRIMS,1>",
    ("S1", 0, 1, 1): "k_trace_batch_flat<false,true,false,EVERY,1>",
    ("S1", 1, 0, 3): "k_trace_batch_flat<true,true,true,EVERY,1>",
    ("S3", 0, 0, 3): "k_trace_batch_flat<false,false,false,TRI,1>",
    ("S4", 0, 0, 1): "k_trace_batch_flat<false,false,false,CSG|PRIMS,2>",
    ("S4", 0, 0, 3): "k_trace_batch_flat<false,false,true,CSG|PRIMS,2>",
    ("materials", 0, 0, 3): "k_trace_batch_flat<true,true,true,EVERY,1>",
    ("materials", 0, 1, 1): "k_trace_batch_flat<false,true,true,EVERY,1>",
    ("testscene", 0, 0, 3): "k_trace_batch_generic<lean>",
    ("testscene", 1, 1, 3): "k_trace_batch_generic<counting>",
}
MAKE = {"S1": lambda: scenes.s1(nlights=2), "S3": lambda: scenes.s3(24), "S4": scenes.s4, "materials": zoo.materials, "testscene": lambda: zoo.testscene(2)}


@pytest.fixture(scope="module")
def traits(built):
    """glome_sb_scene_traits: the commit's own rules, no device"""
    lib = L.load()
    out = {}
    for name, make in MAKE.items():
        sd = make()
        b = api.Builder()
        nmap, _ = sd.replay(b)
        t = np.zeros(11, dtype=np.int64)
        assert lib.glome_sb_scene_traits(b.h, nmap[sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        out[name] = t
    return out


@pytest.mark.parametrize("scene,faithful,count_work,maxdepth", sorted(TRACE_INSTANCES))
def test_scene_gets_its_trace_instance(traits, scene, faithful, count_work, maxdepth):
    row = list(traits[scene][:8]) + [faithful, count_work, maxdepth]
    inst, lb, cap = export_choice(L.load(), [row])[0].tolist()
    assert instance_name(inst) == TRACE_INSTANCES[(scene, faithful, count_work, maxdepth)], dict(zip(COLS, row))
    assert cap == 32 and lb == (2 if inst < 0 else (inst >> 4) & 15)
