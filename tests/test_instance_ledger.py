"""The ledger of kernel instances (tests/instance_ledger.py) holds what it says, checked without a GPU:

  - every row's launch gets the instance the row names (the commit's own traits through glome_sb_scene_traits, the frame's item count
    through glome_items_layout, the choice through glome_kernel_choice / glome_trace_kernel_choice);
  - the rows name every instance the rules can choose over the grids of tests/test_kernel_choice.py and tests/test_trace_choice.py, and
    those are exactly as many as glome_amd/csrc/instances.hpp lists -- a listed instance the rules can never name is a dead compile, an
    instance without a row is a kernel no test launches;
  - the scenes made for the ledger are worth a launch: at a row's frame most pixels hit, a maxdepth 3 frame has secondary rays, and the
    oracle computing in fp32 stays within half of every cap of tests/parity.py, so a device frame has room under the caps as they are."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import instance_ledger as ledger
import parity
import test_kernel_choice as render_choice
import test_trace_choice as trace_choice
from helpers import compare_images, oracle_for
from glome_amd import _lib as L
from glome_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [r.id for r in ledger.LAUNCHES]


def test_row_ids_are_unique_and_frames_are_the_kinds():
    assert len(set(IDS)) == len(IDS)
    for r in ledger.LAUNCHES:
        assert (r.width, r.height) == ledger.FRAME[r.kind] and r.kind in ledger.FRAME and r.maxdepth in (1, 3), r.id
    # the one row no GPU test launches, and the scene it names
    assert [r.id for r in ledger.LAUNCHES if not r.gpu] == ["sampler-S5-d1"]
    assert [r.instance for r in ledger.LAUNCHES if not r.gpu] == ["k_ss_frame_flat<false,TRI,5,true,false>"]


@pytest.fixture(scope="module")
def traits(built):
    """glome_sb_scene_traits of a row's scene (the commit's own rules, no device), once per scene"""
    lib = L.load()
    cache = {}

    def get(row):
        if row.make not in cache:
            sd = row.make()
            b = api.Builder()
            nmap, _ = sd.replay(b)
            t = np.zeros(11, dtype=np.int64)
            assert lib.glome_sb_scene_traits(b.h, nmap[sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
            cache[row.make] = t
        return cache[row.make]
    return get


def chosen_instance(lib, t, row):
    if row.kind == ledger.TRACE:
        inst, _, _ = trace_choice.export_choice(lib, [list(t[:8]) + [row.faithful, row.count_work, row.maxdepth]])[0].tolist()
        return trace_choice.instance_name(inst)
    mode = 1 if row.kind == ledger.SAMPLER else 0
    P = api.render_params(width=row.width, height=row.height, maxdepth=row.maxdepth, mode=mode)
    items = lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)  # (the whole-frame plan of renderTile: 64 x 64 work tiles)
    kind, inst, _, _ = render_choice.export_choice(lib, [list(t[:8]) + [mode, row.faithful, row.count_work, row.maxdepth, 1, items]])[0].tolist()
    assert kind == mode
    return render_choice.instance_name(kind, inst)


@pytest.mark.parametrize("row", ledger.LAUNCHES, ids=IDS)
def test_row_gets_the_instance_it_names(traits, row):
    t = traits(row)
    assert chosen_instance(L.load(), t, row) == row.instance, dict(zip(render_choice.COLS[:8], t[:8].tolist()))


def test_new_scenes_have_the_traits_they_were_made_for(traits):
    """tier, cls_mask, sec, nested, refract (and the LDS stack of the two triangle trees) as the scenes' docstrings state"""
    want = {"mirror_tri": dict(tier=0, cls_mask=1, sec=1, nested=0, refract=0, stack_cap=12), "mirror_mesh": dict(tier=0, cls_mask=8, sec=1, nested=0, refract=0),
            "every_class": dict(tier=0, cls_mask=35, sec=1, nested=0, refract=0)}
    for name in ledger.NEW_SCENES:
        row = next(r for r in ledger.LAUNCHES if ledger.scene_name(r) == name)
        got = dict(zip(render_choice.COLS[:8], traits(row)[:8].tolist()))
        assert {k: got[k] for k in want[name]} == want[name], (name, got)


# ---------------------------------------------------------------- completeness
def rule_names():
    """every instance name the rules produce over the two grids: (render, sampler, trace) sets, generic ones included"""
    lib = L.load()
    axes = [(0, 1), range(64), (0, 1), (0, 1), (0, 1), (0, 1), (render_choice.ASM_LDS_CAP, 8), (500000, 500001), (0, 1), (0, 1), (0, 1), (1, 2), (1, 8), (47999, 48000)]
    rows = np.array(list(itertools.product(*axes)), dtype=np.int64)
    assert rows.shape[0] == 524288
    got = render_choice.export_choice(lib, rows)
    pairs = np.unique(got[:, :2], axis=0)
    render = {render_choice.instance_name(k, i) for k, i in pairs.tolist() if k == 0}
    sampler = {render_choice.instance_name(k, i) for k, i in pairs.tolist() if k == 1}
    rows = np.array(list(itertools.product(*(axes[:8] + [(0, 1), (0, 1), (1, 2)]))), dtype=np.int64)
    trace = {trace_choice.instance_name(i) for i in np.unique(trace_choice.export_choice(lib, rows)[:, 0]).tolist()}
    return render, sampler, trace


def listed_counts():
    """the `X(` entries of the GLOME_*_FLAT_P* lists of instances.hpp, by kind -- counted in the text"""
    with open(os.path.join(ROOT, "glome_amd", "csrc", "instances.hpp")) as f:
        text = f.read()
    counts, lists = {"RENDER": 0, "SS": 0, "TRACE": 0}, 0
    for m in re.finditer(r"^#define GLOME_(RENDER|SS|TRACE)_FLAT_P\d+\(X\)((?:.*\\\n)*.*)$", text, re.M):
        body = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
        counts[m.group(1)] += len(re.findall(r"\bX\(", body))
        lists += 1
    return counts, lists


def test_the_rows_name_every_instance_and_every_listed_instance_can_be_named(built):
    render, sampler, trace = rule_names()
    flat = lambda names: {n for n in names if "_flat<" in n}
    assert (len(flat(render)), len(flat(sampler)), len(flat(trace))) == (17, 9, 16)
    for names, kind in ((render, "render"), (sampler, "ss_frame"), (trace, "trace_batch")):
        assert names - flat(names) == {"k_%s_generic<lean>" % kind, "k_%s_generic<counting>" % kind}
    counts, lists = listed_counts()
    assert lists == 9 and counts == {"RENDER": 17, "SS": 9, "TRACE": 16}, (lists, counts)  # listed = nameable: no dead compile
    for names, kind in ((render, ledger.RENDER), (sampler, ledger.SAMPLER), (trace, ledger.TRACE)):
        rows = {r.instance for r in ledger.LAUNCHES if r.kind == kind}
        assert rows == names, (kind, "without a row:", sorted(names - rows), "no such instance:", sorted(rows - names))
    assert len({r.instance for r in ledger.LAUNCHES}) == 48


# ---------------------------------------------------------------- the new scenes are worth a launch
NEW_ROWS = [r for r in ledger.LAUNCHES if ledger.scene_name(r) in ledger.NEW_SCENES]


@pytest.fixture(scope="module")
def oracle_frames(built):
    """the fp64 and the fp32 oracle's frame of a new scene, once per (scene, mode, maxdepth, frame)"""
    cache = {}

    def get(row):
        mode = 1 if row.kind == ledger.SAMPLER else 0
        key = (row.make, mode, row.maxdepth, row.width, row.height)
        if key not in cache:
            sd = row.make()
            out = []
            for use_float in (False, True):
                o, _, _ = oracle_for(sd, use_float=use_float)
                img, _, rc = o.render(row.width, row.height, mode=mode, maxdepth=row.maxdepth, want_packed=False)
                out.append((img, rc))
            cache[key] = out
        return cache[key]
    return get


@pytest.mark.parametrize("row", NEW_ROWS, ids=[r.id for r in NEW_ROWS])
def test_new_scene_conditions(oracle_frames, row):
    """Stated by the oracle alone.  At the row's frame at least half of the pixels hit (the sampler's frame: of the pixels, traced or
    blended); a maxdepth 3 frame traces at least a tenth as many secondary rays as primary ones; and the fp32 oracle's frame is within
    HALF of each cap the GPU test holds the device to (parity.PIXEL_OUTLIER_MAX, REL_PIXEL_OUTLIER_MAX, SUBSAMPLE_OUTLIER_MAX)."""
    (ref, rc), (f32, _) = oracle_frames(row)
    hit = float(np.mean(ref[..., 4] < 1e6))
    c = compare_images(f32, ref)
    print("new_scene_conditions", row.id, {"hit": hit, "primary": rc["rays_primary"], "secondary": rc["rays_secondary"], "frac_over": c["frac_over"], "rel_frac_over": c["rel_frac_over"]})
    assert hit >= 0.5, hit
    if row.maxdepth == 3:
        assert rc["rays_secondary"] >= rc["rays_primary"] / 10, rc
    assert c["frac_over"] <= 0.5 * (parity.SUBSAMPLE_OUTLIER_MAX if row.kind == ledger.SAMPLER else parity.PIXEL_OUTLIER_MAX), c
    assert c["rel_frac_over"] <= 0.5 * parity.REL_PIXEL_OUTLIER_MAX, c


@pytest.mark.parametrize("name", ledger.NEW_SCENES)
def test_new_scene_mirrors_show_the_scene(built, name):
    """A mirror that shows the sky alone makes a secondary ray that wrongly misses everything look right.  In the 320 x 180 frame the
    bounces of maxdepth 3 change at least one pixel in a hundred from the maxdepth 1 frame (by more than 1e-3: a hundred times the
    colour gate), i.e. over 500 reflected rays end on a surface.  (Oracle, fp64: 2.7 % on mirror_tri, 10 % on mirror_mesh, 7 % on
    every_class; the heightfields of the first two are bent into bowls for this -- left flat, none of their mirrors showed anything.)"""
    o, _, _ = oracle_for(ledger.SCENES[name]())
    w, h = ledger.FRAME[ledger.RENDER]
    one, _, _ = o.render(w, h, maxdepth=1, want_packed=False)
    three, _, _ = o.render(w, h, maxdepth=3, want_packed=False)
    changed = float(np.mean(np.any(np.abs(one[..., :3] - three[..., :3]) > 1e-3, axis=-1)))
    print("bounces change", name, changed)
    assert changed >= 0.01, changed
