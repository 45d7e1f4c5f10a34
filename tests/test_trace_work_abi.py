"""CPU suite: the ABI of the per-ray work records (glome_trace_work_batch) -- the symbols the built library exports and the binding
binds --, api.frame_rays against its defining formula, and INTEGRATION.md's foreign imports against the library's exports."""
import os
import re
import subprocess

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exported(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_the_library_exports_and_the_binding_binds_the_work_symbols(exported):
    names = ("glome_work_words", "glome_trace_work_batch", "glome_trace_work_batch_dev")
    assert all(n in exported for n in names), [n for n in names if n not in exported]
    lib = L.load()
    declared = {name for name, _, _ in L.SYMBOLS}
    assert all(n in declared and getattr(lib, n).argtypes is not None for n in names)
    assert lib.glome_work_words() == 8
    assert len(lib.glome_trace_work_batch.argtypes) == len(lib.glome_trace_work_batch_dev.argtypes) == 15
    assert (api.WORK_BIH_NODES, api.WORK_MESH_NODES, api.WORK_PRIM_TESTS, api.WORK_RAYS_SHADOW, api.WORK_RAYS_SECONDARY,
            api.WORK_PRIMARY_BIH_NODES, api.WORK_PRIMARY_MESH_NODES, api.WORK_PRIMARY_PRIM_TESTS) == tuple(range(8))


@pytest.mark.parametrize("w,h", [(7, 5), (64, 36)])
def test_frame_rays_are_the_reference_formula_rounded_as_stated(built, w, h):
    """get_coordsf / get_rayint (Glome.hs:27-33, 119-140) in float64, rounded to float32, renormalised in float64, rounded again"""
    cam = api.camera(*scenes.s1().cam)
    o, d = api.frame_rays(cam, w, h)
    assert o.shape == d.shape == (w * h, 3) and o.dtype == d.dtype == np.float32
    assert np.array_equal(o, np.broadcast_to(np.array(list(cam.pos), np.float32), (w * h, 3)))
    assert np.abs((d.astype(np.float64) ** 2).sum(1) - 1).max() <= 1e-6
    pos, fwd, up, right = (np.array(list(v), np.float64) for v in (cam.pos, cam.fwd, cam.up, cam.right))
    want = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            xc = ((x / w) * 2 - 1) * (w / h)
            yc = -((y / h) * 2 - 1)
            v = fwd + right * (-xc) + up * yc
            v32 = (v / np.sqrt((v * v).sum())).astype(np.float32)
            v64 = v32.astype(np.float64)
            want[y, x] = (v64 / np.sqrt((v64 * v64).sum())).astype(np.float32)
    assert np.array_equal(d.view(np.uint32), want.reshape(-1, 3).view(np.uint32))
    assert len(np.unique(d, axis=0)) == w * h  # (every pixel its own ray, row major: x runs fastest)
    assert d[1, 0] != d[0, 0] and d[w, 1] != d[0, 1]


def test_every_foreign_import_of_the_integration_guide_is_an_exported_symbol(exported):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    names = re.findall(r'foreign import ccall\s+(?:safe|unsafe)?\s*"&?(\w+)"', text)
    assert len(names) > 60 and "glome_trace_work_batch" in names and "glome_trace_work_batch_dev" in names and "glome_work_words" in names
    missing = sorted({n for n in names if n not in exported})
    assert not missing, missing
    assert "glome_ctx_error" not in text  # (there is no such function: glome_last_error)
