"""Which kernel instance a launch gets (glome_amd/csrc/instances.hpp choose_render / choose_sampler), seen through the host-only
export glome_kernel_choice -- no GPU is touched.

The rules were spread over the device file before it was split.  Here they are stated a second time, independently, in numpy:
transcribed from glome_amd/csrc/glome_device.hip of commit 7405391 (the last one that had that file) --
    scene_class      lines 1324-1328        use_two_rows    lines 1330-1337
    launch_render    lines 1339-1360        the sampler's branch of render_impl, lines 1445-1470
    the wave caps of the two grids: lines 1453 and 1476
and the export must agree with them exactly on every point of the grid of inputs those rules look at (524,288 cases).  The second
test pins which instance each bench configuration gets; its table doubles as documentation."""
import ctypes as C
import itertools

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes

CLS_BIH_TRI, CLS_BIH_SPHERE, CLS_BIH_SIMPLE, CLS_MESH, CLS_PRIMS, CLS_ALL, CLS_CSG, CLS_EVERY = 1, 2, 4, 8, 16, 31, 32, 63  # rt_device.hpp:1370 there
ASM_LDS_CAP = 12  # kAsmLdsCap = GLOME_LDS_STACK, rt_device.hpp:743-746 there
FLAG_LB, CSG_LB = 6, 2  # GLOME_FLAG_LB, GLOME_CSG_LB: lines 709-714
COLS = ("tier", "cls_mask", "sec", "nested", "refract", "pk_all", "stack_cap", "n_bih_nodes", "mode", "faithful", "count_work", "maxdepth", "tile_stride", "items")


def render_key(F, Cn, U, cls, lb, two):  # render_flat_key, line 716
    return (F * 1) | (Cn * 2) | (U * 4) | (two * 8) | (lb << 4) | (cls << 8)


def ss_key(U, cls, lb, two, F):  # ss_flat_key, line 717
    return (F * 1) | (U * 4) | (two * 8) | (lb << 4) | (cls << 8)


def parent_choice(g):
    """g: dict of int64 arrays (COLS) -> (instance, two_rows, wave cap), the parent's rules"""
    m, tier, depth = g["cls_mask"], g["tier"], g["maxdepth"]
    sec, nested, refract, pk_all = (g[k] != 0 for k in ("sec", "nested", "refract", "pk_all"))
    faithful_p, count_p = g["faithful"] != 0, g["count_work"] != 0
    # scene_class (1324-1328)
    with_csg = np.where((m & ~(CLS_CSG | CLS_PRIMS)) == 0, CLS_CSG | CLS_PRIMS, CLS_EVERY)
    without = np.where((m & ~CLS_BIH_TRI) == 0, CLS_BIH_TRI,
                       np.where((m & ~(CLS_BIH_SPHERE | CLS_PRIMS)) == 0, CLS_BIH_SPHERE | CLS_PRIMS, np.where((m & ~CLS_MESH) == 0, CLS_MESH, CLS_ALL)))
    cls = np.where((m & CLS_CSG) != 0, with_csg, without)

    def use_two_rows(items):  # 1330-1337
        small_shard = (g["tile_stride"] != 1) & (items < 48000)
        out = (tier != 0) | faithful_p | count_p | sec | nested | (g["stack_cap"] != ASM_LDS_CAP) | ~pk_all
        return ~small_shard & ~out & (cls == CLS_BIH_TRI)

    full = nested | (sec & (depth > 1))  # 1349, 1447
    generic = np.where(count_p, -1, -2)  # 1347, 1469: launch_*_generic counts, *_generic_lean does not
    # ---- renderTile: launch_render (1339-1360), grid cap (1476)
    two_r = use_two_rows(g["items"])  # (1352, 1474: the launch's item count)
    faithful = faithful_p | ((tier == 0) & refract & (depth > 1))  # 1341, 1346
    count = count_p | faithful
    lb = np.where(cls == CLS_EVERY, 2, np.where(cls == (CLS_CSG | CLS_PRIMS), CSG_LB, 1))  # 1357
    key_r = np.select([two_r, faithful, count],
                      [render_key(0, 0, 0, CLS_BIH_TRI, FLAG_LB, 1), render_key(1, 1, full, CLS_EVERY, 1, 0), render_key(0, 1, full, CLS_EVERY, 1, 0)],
                      default=render_key(0, 0, full, cls, lb, 0))  # 1352-1358
    cap_r = np.where(two_r, 4 * FLAG_LB, 32)  # 1476
    # ---- renderTileSubsample: the sampler's branch (1445-1470), grid cap (1453)
    two_s = use_two_rows(np.int64(0xffffffff)) & (cls == CLS_BIH_TRI)  # 1445: no item count
    tri = (tier == 0) & ((m & ~CLS_BIH_TRI) == 0)  # 1448
    big_tree = g["n_bih_nodes"] > 500000  # 1450
    refr = refract & (depth > 1)  # 1458
    key_s = np.select([two_s, tri & ~full, tri & ~refr, full & refr],
                      [ss_key(0, CLS_BIH_TRI, np.where(big_tree, 5, 4), 1, 0), ss_key(0, CLS_BIH_TRI, 1, 0, 0), ss_key(1, CLS_BIH_TRI, 1, 0, 0), ss_key(1, CLS_EVERY, 1, 0, 1)],
                      default=ss_key(full, np.where(cls == (CLS_CSG | CLS_PRIMS), CLS_CSG | CLS_PRIMS, CLS_EVERY), 2, 0, 0))  # 1463-1468
    cap_s = np.where(two_s, np.where(big_tree, 20, 16), 32)  # 1453
    sampler = g["mode"] == 1
    instance = np.where(tier != 0, generic, np.where(sampler, key_s, key_r))
    return instance, np.where(sampler, two_s, two_r), np.where(sampler, cap_s, cap_r)


def export_choice(lib, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.full((rows.shape[0], 4), -99, dtype=np.int32)
    assert lib.glome_kernel_choice(rows.shape[0], rows.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == rows.shape[0]
    return out


def test_choice_equals_the_parents_rules_on_the_whole_grid(built):
    lib = L.load()
    axes = [(0, 1), range(64), (0, 1), (0, 1), (0, 1), (0, 1), (ASM_LDS_CAP, 8), (500000, 500001), (0, 1), (0, 1), (0, 1), (1, 2), (1, 8), (47999, 48000)]
    rows = np.array(list(itertools.product(*axes)), dtype=np.int64)
    assert rows.shape == (2 * 64 * 16 * 2 * 2 * 2 * 2 * 2 * 2 * 2 * 2, 14)
    got = export_choice(lib, rows)
    instance, two_rows, cap = parent_choice({k: rows[:, i] for i, k in enumerate(COLS)})
    assert np.array_equal(got[:, 0], rows[:, 8])  # the kind is the mode
    for name, want, col in (("instance", instance, 1), ("two_rows", two_rows.astype(np.int64), 2), ("wave cap", cap, 3)):
        bad = np.flatnonzero(got[:, col] != want)
        assert bad.size == 0, (name, bad.size, [dict(zip(COLS, rows[i].tolist())) for i in bad[:4]], got[bad[:4]].tolist(), want[bad[:4]].tolist())
    assert lib.glome_kernel_choice(1, None, None) == L.E_INVALID


CLS_NAMES = {CLS_BIH_TRI: "TRI", CLS_BIH_SPHERE | CLS_PRIMS: "SPHERE|PRIMS", CLS_MESH: "MESH", CLS_ALL: "ALL", CLS_CSG | CLS_PRIMS: "CSG|PRIMS", CLS_EVERY: "EVERY"}


def instance_name(kind, inst):
    if inst < 0:
        return ("k_ss_frame_generic" if kind else "k_render_generic") + ("<counting>" if inst == -1 else "<lean>")
    F, Cn, U, two, lb, cls = inst & 1, (inst >> 1) & 1, (inst >> 2) & 1, (inst >> 3) & 1, (inst >> 4) & 15, CLS_NAMES[inst >> 8]
    b = lambda x: "true" if x else "false"
    if kind:
        return f"k_ss_frame_flat<{b(U)},{cls},{lb},{b(two)},{b(F)}>"  # <FULL, CLS, LB, TWO_ROWS, FAITHFUL>
    return f"k_render_flat<{b(F)},{b(Cn)},{b(U)},{cls},{lb},{b(two)}>"  # <FAITHFUL, COUNT, FULL, CLS, LB, TWO_ROWS>


# What each bench configuration (glome_amd/scenes.py CONFIGS; bench.py renders the whole frame: tile_stride 1, neither faithful nor
# counting) is launched with: (instance, two stack rows, wave slots per CU).  Read off the parent's rules (the lines cited at the top)
# for the traits the commit derives for each scene -- S3 / S5: one triangle BIH, all materials Surface, a tree no deeper than the LDS
# stack, so the two-row instances (the sampler's by tree size: S5 has over 500,000 nodes); S3mesh: class MESH; S1 / S2: a plane and a sphere
# BIH; S4: CSG items and primitives with a Reflect material at maxdepth 3, so the full instances; TS: the generic tier.
BENCH_INSTANCES = {
    ("S1", 0): ("k_render_flat<false,false,false,SPHERE|PRIMS,1,false>", 0, 32),
    ("S1", 1): ("k_ss_frame_flat<false,EVERY,2,false,false>", 0, 32),
    ("S2", 0): ("k_render_flat<false,false,false,SPHERE|PRIMS,1,false>", 0, 32),
    ("S2", 1): ("k_ss_frame_flat<false,EVERY,2,false,false>", 0, 32),
    ("S3", 0): ("k_render_flat<false,false,false,TRI,6,true>", 1, 24),
    ("S3", 1): ("k_ss_frame_flat<false,TRI,4,true,false>", 1, 16),
    ("S3mesh", 0): ("k_render_flat<false,false,false,MESH,1,false>", 0, 32),
    ("S3mesh", 1): ("k_ss_frame_flat<false,EVERY,2,false,false>", 0, 32),
    ("S4", 0): ("k_render_flat<false,false,true,CSG|PRIMS,2,false>", 0, 32),
    ("S4", 1): ("k_ss_frame_flat<true,CSG|PRIMS,2,false,false>", 0, 32),
    ("S5", 0): ("k_render_flat<false,false,false,TRI,6,true>", 1, 24),
    ("S5", 1): ("k_ss_frame_flat<false,TRI,5,true,false>", 1, 20),
    ("TS", 0): ("k_render_generic<lean>", 0, 32),
    ("TS", 1): ("k_ss_frame_generic<lean>", 0, 32),
}


@pytest.fixture(scope="module")
def bench_traits(built):
    """the traits of every bench scene, committed through the host builder (glome_sb_scene_traits: the commit's own rules, no device)"""
    lib = L.load()
    out = {}
    for name in sorted({k[0] for k in BENCH_INSTANCES}):
        sd = scenes.CONFIGS[name]["make"]()
        b = api.Builder()
        nmap, _ = sd.replay(b)
        t = np.zeros(11, dtype=np.int64)
        assert lib.glome_sb_scene_traits(b.h, nmap[sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        out[name] = t
    return out


@pytest.mark.parametrize("scene,mode", sorted(BENCH_INSTANCES))
def test_bench_configuration_gets_its_instance(bench_traits, scene, mode):
    lib = L.load()
    cfg = scenes.CONFIGS[scene]
    P = api.render_params(width=cfg["width"], height=cfg["height"], maxdepth=cfg["maxdepth"], mode=mode)
    items = lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)  # (the whole-frame plan of renderTile: 64 x 64 work tiles)
    row = list(bench_traits[scene][:8]) + [mode, 0, 0, cfg["maxdepth"], 1, items]
    kind, inst, two_rows, cap = export_choice(lib, [row])[0].tolist()
    assert kind == mode
    assert (instance_name(kind, inst), two_rows, cap) == BENCH_INSTANCES[(scene, mode)], dict(zip(COLS, row))
