"""GPU suite (-m gpu): ss_frame_loop and its item, region, block and lane arithmetic (render_kernels.hpp) against
tests/sampler_model.py, bit for bit.  The model is fed from the GPU's own renderTile frame at twice the size, which holds every
sample the sampler may take (sampler_model.py), so what is compared is the sampler alone: no tolerance, no share of outliers, and
rays_primary to the ray.  One device operation is not correctly rounded, the quotient in ccmp; each case asserts on the GPU's own
samples that no contrast lies within the band of a threshold (sampler_model.BAND), so that bit decides nothing."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sampler_model as M
from helpers import product_camera_lights
from glome_amd import _lib as L
from glome_amd import api
from sampler_cases import BATCH, GENERIC, SCENES, SINGLE, case_id, views

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def committed(gpu_ctx):
    made = {}

    def get(name):
        if name not in made:
            sd = SCENES[name]()
            b = api.Builder()
            nm, _ = sd.replay(b)
            sc = gpu_ctx.commit(b, nm[sd.root])
            assert sc.info()["tier"] == (1 if name in GENERIC else 0), (name, sc.info())
            made[name] = (sd, b, sc)
        return made[name]
    yield get
    for _, _, sc in made.values():
        sc.release()


def _log(c, f, res):
    path = os.environ.get("GLOME_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"check": "sampler_model_gpu", "case": case_id(c), "view": f, "tested": res.tested[1:], "traced": res.traced[1:],
                                 "undecided": res.undecided, "margin": res.margin, "margin_at": res.margin_at}) + "\n")


def _model_of(sc, cam, lights, c, f=0):
    """the model of view `cam` from the GPU's own mode 0 frame at 2W x 2H, after asserting that it has no undecided candidate"""
    R2, _, _ = sc.render(cam, lights, api.render_params(width=2 * c.w, height=2 * c.h, maxdepth=c.maxdepth, fog=0), want_packed=False)
    res = M.model(R2, c.w, c.h, c.blocksize, c.thresholds or M.DEFAULT_THRESHOLDS)
    _log(c, f, res)
    print(case_id(c), "view", f, "tested", res.tested[1:], "traced", res.traced[1:], "undecided", res.undecided, "margin", res.margin, res.margin_at)
    assert res.undecided == 0, (res.undecided, res.margin, res.margin_at)  # (the case's inputs are at fault then: another size or threshold set)
    return res


def _params(c):
    return api.render_params(width=c.w, height=c.h, mode=1, maxdepth=c.maxdepth, blocksize=c.blocksize, thresholds=c.thresholds)


@pytest.mark.parametrize("c", SINGLE, ids=case_id)
def test_sampler_frame_equals_the_model(gpu_ctx, committed, c):
    sd, b, sc = committed(c.scene)
    cam, lights = product_camera_lights(sd)
    res = _model_of(sc, cam, lights, c)
    for rep in range(2):
        img, packed, st = sc.render(cam, lights, _params(c), init=np.full((c.h, c.w, 5), np.nan, np.float32))
        d = M.first_difference(res, img)  # (every bit: a pixel that kept its NaN differs too)
        assert d is None, d
        assert np.array_equal(packed, res.packed)
        assert st["rays_primary"] == sum(res.traced), (st["rays_primary"], res.traced)


@pytest.mark.parametrize("c", BATCH, ids=case_id)
def test_sampler_batch_equals_the_model_of_every_view(gpu_ctx, committed, c):
    """glome_render_packed_batch_dev in mode 1: the region shape follows the frames of the launch, so the same pixels come from other
    items, blocks and packets.  Each frame's packed pixels against the model of that view's own doubled frame."""
    import torch
    sd, b, sc = committed(c.scene)
    _, lights = product_camera_lights(sd)
    vs = views(c, sd)
    want = [_model_of(sc, v, lights, c, f).packed for f, v in enumerate(vs)]
    assert any(not np.array_equal(want[0], w) for w in want[1:])
    P = _params(c)
    px = torch.full((c.nframes, c.h, c.w), -1, dtype=torch.int32, device=torch.device("cuda:0"))
    cams = (L.Camera * c.nframes)(*vs)
    la = (L.Light * max(1, len(lights)))(*lights)
    for rep in range(2):
        assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, c.nframes, la, len(lights), C.byref(P), C.c_void_p(px.data_ptr()), c.h * c.w, None) == 0, gpu_ctx.err()
        gpu_ctx.synchronize()
        got = px.cpu().numpy().view(np.uint32)
        for f in range(c.nframes):
            bad = np.argwhere(got[f] != want[f])
            assert len(bad) == 0, (rep, f, len(bad), "first (y, x):", bad[0].tolist(), hex(int(got[f][tuple(bad[0])])), hex(int(want[f][tuple(bad[0])])))
        px.fill_(-1)
