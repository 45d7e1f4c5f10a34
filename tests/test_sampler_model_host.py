"""CPU suite: the host build's adaptive sampler (hostsim_render_subsample, over the device headers' pass helpers) against
tests/sampler_model.py fed from the host build's own renderTile frame at twice the size -- every bit of every pixel, and the
traced count.  The same backend makes both, so no tolerance and no outlier share is in play.  Then what the case table as a whole
reaches, from the model's own counters, and the table's conditions: no undecided candidate, a smallest margin of four bands."""
import functools
import json
import os

import numpy as np
import pytest

import sampler_model as M
from helpers import HostSim, product_camera_lights
from glome_amd import api
from sampler_cases import BATCH, CASES, GENERIC, SCENES, SINGLE, case_id, views

MIN_MARGIN = 4 * M.BAND  # 6.1e-5


@functools.lru_cache(maxsize=None)
def host_scene(name):
    sd = SCENES[name]()
    b = api.Builder()
    nm, _ = sd.replay(b)
    hs = HostSim(b, nm[sd.root])
    assert hs.info()["tier"] == (1 if name in GENERIC else 0), (name, hs.info())
    return sd, b, hs


@functools.lru_cache(maxsize=None)
def run_case(c):
    """[(model result, host frame, host counters)] per view of the case"""
    sd, b, hs = host_scene(c.scene)
    _, lights = product_camera_lights(sd)
    thr = c.thresholds or M.DEFAULT_THRESHOLDS
    out = []
    for cam in views(c, sd):
        R2, _ = hs.render(cam, lights, 2 * c.w, 2 * c.h, c.maxdepth)
        res = M.model(R2, c.w, c.h, c.blocksize, thr)
        img, cnt = hs.render_subsample(cam, lights, c.w, c.h, c.maxdepth, c.blocksize, thr)
        out.append((res, img, cnt))
    return out


def _log(c, f, res):
    path = os.environ.get("GLOME_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"check": "sampler_model_host", "case": case_id(c), "view": f, "tested": res.tested[1:], "traced": res.traced[1:],
                                 "undecided": res.undecided, "margin": res.margin, "margin_at": res.margin_at}) + "\n")


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_model_equals_the_host_build(built, c):
    for f, (res, img, cnt) in enumerate(run_case(c)):
        _log(c, f, res)
        print(case_id(c), "view", f, "tested", res.tested[1:], "traced", res.traced[1:], "undecided", res.undecided, "margin", res.margin, res.margin_at)
        d = M.first_difference(res, img)
        assert d is None, d
        assert sum(res.traced) == int(cnt[0]), (res.traced, cnt)
        assert np.array_equal(M.pack(img), res.packed)
        # the conditions on the table (on the host build's samples)
        assert res.undecided == 0, (res.undecided, res.margin, res.margin_at)
        assert res.margin >= MIN_MARGIN, (res.margin, res.margin_at)


def test_generic_scene_through_the_generic_tier_and_flat_scene_through_both(built):
    """tier = 1 forces the interpreter: the generic scene's own tier (asserted above) and, for a flat-tier scene, a second backend
    whose frames the model must predict from that backend's own doubled frame."""
    for c in (next(c for c in SINGLE if c.scene in GENERIC), next(c for c in SINGLE if c.scene == "materials")):
        sd, b, hs = host_scene(c.scene)
        cam, lights = product_camera_lights(sd)
        R2, _ = hs.render(cam, lights, 2 * c.w, 2 * c.h, c.maxdepth, tier=1)
        res = M.model(R2, c.w, c.h, c.blocksize, c.thresholds or M.DEFAULT_THRESHOLDS)
        img, cnt = hs.render_subsample(cam, lights, c.w, c.h, c.maxdepth, c.blocksize, c.thresholds or M.DEFAULT_THRESHOLDS, tier=1)
        d = M.first_difference(res, img)
        assert d is None, d
        assert sum(res.traced) == int(cnt[0])


def test_the_table_reaches_what_it_is_there_for(built):
    single = [(c, run_case(c)[0][0]) for c in SINGLE]
    # both outcomes of decide in each of passes 2-5, in every case large enough to have them and over the table
    for p in range(2, 6):
        assert any(r.traced[p] > 0 and r.traced[p] < r.tested[p] for _, r in single), p
        assert sum(r.traced[p] for _, r in single) > 50 and sum(r.tested[p] - r.traced[p] for _, r in single) > 50, p
    # all four forms of the last blend, in one frame and over the table
    assert any(all(r.forms[k] > 0 for k in M.BLEND_FORMS) for _, r in single)
    # a neighbour read outside the tile on each of the four sides
    for side in ("left", "right", "top", "bottom"):
        assert any(r.outside[side] > 0 for _, r in single), side
    # tiles clipped on the right, at the bottom and at both (blocksize 65)
    shapes = {(tw, th) for c, r in single if c.blocksize == 65 for (_, _, tw, th) in r.tiles}
    assert any(tw < 65 and th == 65 for tw, th in shapes) and any(tw == 65 and th < 65 for tw, th in shapes) and any(tw < 65 and th < 65 for tw, th in shapes)
    # a last tile 1 pixel wide, one 1 pixel high, a 2-pixel one; a 1x1 frame; 7x5 and 65x65 frames
    assert any(tw == 1 and th > 1 for tw, th in shapes) and any(th == 1 and tw > 1 for tw, th in shapes)
    assert any(tw == 2 or th == 2 for tw, th in shapes)
    sizes = {(c.w, c.h) for c in SINGLE}
    assert {(1, 1), (7, 5), (65, 65)} <= sizes
    # at least 2x2 full tiles in one frame
    assert any(len({xt for (xt, yt, tw, th) in r.tiles if (tw, th) == (65, 65)}) >= 2 and len({yt for (xt, yt, tw, th) in r.tiles if (tw, th) == (65, 65)}) >= 2
               for c, r in single if c.blocksize == 65)
    assert {65, 16, 7, 1} <= {c.blocksize for c in SINGLE}
    assert any(c.thresholds is not None and tuple(c.thresholds) != M.DEFAULT_THRESHOLDS for c in SINGLE)
    # the scenes: the triangle walk (lean), secondary rays, CSG, a mesh, the generic tier
    assert {"S3small", "materials", "S4", "mesh"} <= {c.scene for c in SINGLE} and any(c.scene in GENERIC for c in SINGLE)
    # frames per launch: 1, 2, 3, 8 on a flat-tier scene, 1, 3, 12 on the generic one
    assert {2, 3, 8} <= {c.nframes for c in BATCH if c.scene not in GENERIC} and {3, 12} <= {c.nframes for c in BATCH if c.scene in GENERIC}
    # the views of a batch are different frames
    for c in BATCH:
        rs = run_case(c)
        assert any(not np.array_equal(rs[0][0].packed, r[0].packed) for r in rs[1:]), case_id(c)
