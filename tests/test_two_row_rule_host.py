"""CPU suite: the admission rule of the two-row kernels, material kind by material kind.

The two-row instances -- the flagship render instance and the two two-row sampler instances -- are compiled with TIER::SURFACE_ONLY
(glome_amd/csrc/render_kernels.hpp FlatTier): they shade every hit as a Surface and never read a material's kind (rt_device.hpp
trace_primary, postshade_lean).  That is sound only while the rule that admits a scene to them (instances.hpp use_two_rows over
capi_shared.hpp commit_rules) refuses every scene that holds a material of another kind.  Here: one scene per kind -- a textured
triangle bih, which alone is a flagship scene -- through the commit's own traits (glome_sb_scene_traits) and the launch's own choice
(glome_kernel_choice), for renderTile and for the adaptive sampler, at maxdepth 1 (where a lean kernel is legal for a Reflect or a
Refract material, so only the two-row rule stands between the scene and a Surface-only kernel) and at maxdepth 3.
"""
import ctypes as C

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

ITEMS = 425  # the work items of the 200 x 136 frame of tests/test_cull_pass.py; the rule looks at them only under a tile stride


def _scene(kind):
    """`tex (bih triangles) m`, m of the kind asked for; the other kinds' children are Surfaces"""
    sd = SceneDesc()
    a = scenes.matte(sd, (0.8, 0.5, 0.4))
    tris = sd.bih(sd.triangles_bulk(scenes.heightfield_triangles(32)))
    if kind == "surface":
        m = a
    elif kind == "reflect":
        m = sd.material_reflect(0.8)
    elif kind == "refract":
        m = sd.material_refract(0.1, 0.9, 1.5)
    elif kind == "layers":
        m = sd.material_layers([a, scenes.matte(sd, (0.1, 0.2, 0.3))])
    elif kind == "blend":
        m = sd.material_blend(a, scenes.matte(sd, (0.1, 0.2, 0.3)), 0.25)
    elif kind == "warp":
        frame = sd.tex(sd.sphere((0.0, 0.0, 3.0), 1.0), a)
        m = sd.material_warp(frame, None, [], api.translate((0.0, 100.0, 0.0)))
    else:
        raise KeyError(kind)
    sd.set_root(sd.tex(tris, m))
    scenes._common(sd, 1)
    return sd


def _choices(kind):
    """(mode, maxdepth) -> the four outputs of glome_kernel_choice for the scene of that kind"""
    lib = L.load()
    sd = _scene(kind)
    b = api.Builder()
    nm, _ = sd.replay(b)
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(b.h, nm[sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    keys = [(mode, md) for mode in (0, 1) for md in (1, 3)]
    rows = np.array([list(t[:8]) + [mode, 0, 0, md, 1, ITEMS] for mode, md in keys], dtype=np.int64)
    out = np.zeros((len(keys), 4), dtype=np.int32)
    assert lib.glome_kernel_choice(len(keys), rows.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == len(keys)
    return t, {k: out[i].tolist() for i, k in enumerate(keys)}


def test_a_scene_of_surfaces_is_admitted(built):
    """the control: without it the refusals below could come from the geometry"""
    t, ch = _choices("surface")
    assert (t[0], t[2], t[3], t[4]) == (0, 0, 0, 0) and t[5] == 1
    for (mode, md), (kind, inst, two_rows, _) in ch.items():
        assert kind == mode and two_rows == 1 and inst >= 0 and (inst >> 3) & 1 == 1, (mode, md, inst)
        assert (inst >> 2) & 1 == 0  # (a lean instance: SURFACE_ONLY is never set on a full one)


@pytest.mark.parametrize("kind", ["reflect", "refract", "layers", "blend", "warp"])
def test_any_other_material_kind_is_refused(built, kind):
    t, ch = _choices(kind)
    assert t[2] == 1 or t[3] == 1, "commit_rules classifies the kind as neither secondary nor nested"
    assert t[2] == (kind in ("reflect", "refract", "warp")) and t[3] == (kind in ("layers", "blend")) and t[4] == (kind == "refract")
    for (mode, md), (_, inst, two_rows, _) in ch.items():
        assert two_rows == 0, (kind, mode, md)
        assert inst < 0 or (inst >> 3) & 1 == 0, (kind, mode, md, inst)  # (the TWO_ROWS bit of a flat-tier key; negative: the generic tier)
