"""The two-row kernels shade every hit as a Surface (TIER::SURFACE_ONLY, glome_amd/csrc/render_kernels.hpp FlatTier): trace_primary asks
no material whether it is one, postshade_lean dispatches on no kind and tests no `lc.done`.  What those kernels still do per hit -- the
tex-stack loop, the opacity early-out, the light loops of preshade_wave and surface_shade -- case by case, bit for bit against the same
view under faithful=1: the every-class instance, which reads every material's kind and shares none of the compiled-out code.

As tests/test_cull_pass.py: the terrain of scenes.s3(32), 200 x 136, 425 work items; every case asserts through glome_kernel_choice that
its launch gets the flagship instance and its reference does not.  One case goes through the adaptive sampler as well: the two-row
sampler instance against the three-row one (mode 1 with faithful=1 selects it).
"""
import ctypes as C

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

W, H = 200, 136
ITEMS = 425
N = 32


def _terrain(sd, dx=0.0, dy=0.0):
    t = scenes.heightfield_triangles(N).copy()
    t[:, 0::3] += dx
    t[:, 1::3] += dy
    return sd.bih(sd.triangles_bulk(t))


def _one(mat_of):
    sd = SceneDesc()
    sd.set_root(mat_of(sd, _terrain(sd)))
    scenes._common(sd, 1)
    return sd


def _stacked(translucent):
    """tex (tex terrain inner) outer.  The stack is walked innermost first (rt_types.h TexStack): with a translucent inner material the
    loop takes its second iteration and folds the outer one under it; with an opaque inner one it ends at the opacity test."""
    def f(sd, node):
        inner = sd.material_surface((0.8, 0.5, 0.4), 0.5 if translucent in ("inner", "both") else 1, 0.2, 1, 0, 0)
        outer = sd.material_surface((0.1, 0.6, 0.9), 0.25 if translucent in ("outer", "both") else 1, 0.3, 0.7, 0, 0)
        return sd.tex(sd.tex(node, inner), outer)
    return _one(f)


def _bare():
    """a textured terrain and, a little higher and to the side so that the two interpenetrate, one without any Tex: its hits have an empty
    texture stack (id == 0), the transparent black pixel with a finite depth, and no shadow ray"""
    sd = SceneDesc()
    sd.set_root(sd.group([sd.tex(_terrain(sd), scenes.matte(sd, (0.8, 0.5, 0.4))), _terrain(sd, 6.0, 0.4)]))
    scenes._common(sd, 1)
    return sd


def _shiny():
    return _one(lambda sd, node: sd.tex(node, sd.material_surface((1, 1, 1), 1, 0.2, 0.8, 0.4, 10)))  # ks > delta: the powf branch


def _two_lights():
    """one light that casts no shadows and one whose radius ends inside the terrain (llen > rad for the far part of it)"""
    sd = _one(lambda sd, node: sd.tex(node, sd.material_surface((1, 1, 1), 1, 0.2, 0.8, 0.4, 10)))
    sd.lights = []
    sd.add_light(scenes.LIGHTS[0][0], scenes.LIGHTS[0][1], shadow=False)
    sd.add_light(scenes.LIGHTS[1][0], scenes.LIGHTS[1][1], rad=9.0, shadow=True)
    return sd


def _no_lights():
    sd = _one(lambda sd, node: sd.tex(node, scenes.matte(sd, (0.8, 0.5, 0.4))))
    sd.lights = []
    return sd


def _flags():
    """three root entries: the terrain; a raised copy under NoShadow (seen, casts nothing); a copy high above under OnlyShadow (unseen,
    shades what lies under it)"""
    sd = SceneDesc()
    mat = scenes.matte(sd, (0.8, 0.5, 0.4))
    mat2 = scenes.matte(sd, (0.2, 0.7, 0.3))
    sd.set_root(sd.group([sd.tex(_terrain(sd), mat), sd.noshadow(sd.tex(_terrain(sd, 6.0, 0.4), mat2)), sd.onlyshadow(sd.tex(_terrain(sd, -4.0, 3.0), mat))]))
    scenes._common(sd, 1)
    return sd


def _two_terrains():
    """the scene of tests/test_cull_pass.py: two root entries, the terrain and a copy 20 units along x"""
    sd = SceneDesc()
    mat = scenes.matte(sd, (0.8, 0.5, 0.4))
    sd.set_root(sd.group([sd.tex(_terrain(sd), mat), sd.tex(_terrain(sd, 20.0), mat)]))
    scenes._common(sd, 1)
    return sd


CASES = {
    "stacked_outer_translucent": lambda: _stacked("outer"),
    "stacked_inner_translucent": lambda: _stacked("inner"),
    "stacked_both_translucent": lambda: _stacked("both"),
    "bare_bih_beside_a_textured_one": _bare,
    "shiny": _shiny,
    "two_lights_one_shadowless_one_short": _two_lights,
    "no_lights": _no_lights,
    "noshadow_and_onlyshadow_entries": _flags,
    "two_terrains": _two_terrains,
}


def _views():
    return {"horizon": api.camera(*scenes.CUST_CAM),
            "down": api.camera_from_vectors((0.0, 6.0, 0.0), (0, -1, 0), (0, 0, -1), (1, 0, 0))}


def _params(**kw):
    return api.render_params(width=W, height=H, maxdepth=1, **kw)


def _choice(lib, builder, root, P):
    """(kind, instance key, two_rows) of the launch (glome_kernel_choice over the commit's own traits)"""
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(builder.h, root, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    row = np.array([list(t[:8]) + [P.mode, P.faithful, P.count_work, P.maxdepth, P.tile_stride, ITEMS]], dtype=np.int64)
    out = np.zeros((1, 4), dtype=np.int32)
    assert lib.glome_kernel_choice(1, row.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == 1
    return int(out[0, 0]), int(out[0, 1]), int(out[0, 2])


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _commit(ctx, sd):
    b = api.Builder()
    nm, _ = sd.replay(b)
    assert int(ctx.lib.glome_items_layout(C.byref(_params()), 0, 1, 64, 1, None, 0)) == ITEMS
    return b, nm[sd.root], ctx.commit(b, nm[sd.root]), [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_flagship_frame_equals_the_faithful_one_bit_for_bit(gpu_ctx, case):
    sd = CASES[case]()
    b, root, sc, lights = _commit(gpu_ctx, sd)
    try:
        kind, inst, two = _choice(gpu_ctx.lib, b, root, _params())
        assert (kind, two) == (0, 1) and (inst >> 3) & 1 == 1, "the flagship instance is not chosen for this case"
        assert _choice(gpu_ctx.lib, b, root, _params(faithful=1))[2] == 0
        seen = np.zeros((0, 5), np.float32)
        for view, cam in _views().items():
            for fog in (0, 1):
                ref, ref_packed, ref_st = sc.render(cam, lights, _params(faithful=1, fog=fog))
                img, packed, st = sc.render(cam, lights, _params(fog=fog))
                assert _same_bits(img, ref), (case, view, fog, np.argwhere(img.view(np.uint32) != ref.view(np.uint32))[:8])
                assert np.array_equal(packed, ref_packed), (case, view, fog)
                assert st["rays_primary"] == W * H and st["rays_shadow"] == ref_st["rays_shadow"], (case, view, fog, st, ref_st)
                if fog == 0:
                    seen = np.concatenate([seen, ref.reshape(-1, 5)])
                    shadow_rays = ref_st["rays_shadow"]
        # the comparison is of pictures, and of the branch the case is named after (all read from the REFERENCE frames)
        hit = seen[seen[:, 4] < 1.0e6]
        assert len(hit) > 2000, case
        if case == "stacked_outer_translucent":     # the inner material is opaque: its alpha alone, the outer colour never folded in
            assert (hit[:, 3] == 1).all()
        elif case in ("stacked_inner_translucent", "stacked_both_translucent"):  # 0.5, then the outer material's share under it
            want = np.float32(0.5) + (np.float32(1) - np.float32(0.5)) * np.float32(1 if case == "stacked_inner_translucent" else 0.25)
            assert (hit[:, 3] == want).all(), (case, np.unique(hit[:, 3]), want)
        elif case == "bare_bih_beside_a_textured_one":
            blank = (hit[:, :4] == 0).all(axis=1)
            assert 500 < blank.sum() < len(hit) - 500, (case, int(blank.sum()), len(hit))
        elif case == "no_lights":
            assert shadow_rays == 0 and len(np.unique(hit[:, :3], axis=0)) == 1  # ambient alone
        elif case == "two_lights_one_shadowless_one_short":
            assert 0 < shadow_rays < len(hit) // 2  # the short light's rays only, and only where it reaches
    finally:
        sc.release()


@pytest.mark.gpu
def test_two_row_sampler_equals_the_three_row_sampler(gpu_ctx):
    """mode 1 over the two-light scene with stacked translucent materials: the two-row sampler instance against the sampler's three-row
    instance of the triangle class, which reads every material's kind"""
    sd = _stacked("both")
    sd.lights = []
    sd.add_light(scenes.LIGHTS[0][0], scenes.LIGHTS[0][1], shadow=False)
    sd.add_light(scenes.LIGHTS[1][0], scenes.LIGHTS[1][1], rad=9.0, shadow=True)
    b, root, sc, lights = _commit(gpu_ctx, sd)
    try:
        kind, inst, two = _choice(gpu_ctx.lib, b, root, _params(mode=1))
        assert (kind, two) == (1, 1) and (inst >> 3) & 1 == 1, "the two-row sampler instance is not chosen"
        kind, inst, two = _choice(gpu_ctx.lib, b, root, _params(mode=1, faithful=1))
        assert (kind, two) == (1, 0) and inst >= 0 and (inst >> 3) & 1 == 0
        for view, cam in _views().items():
            ref, _, ref_st = sc.render(cam, lights, _params(mode=1, faithful=1), want_packed=False)
            img, _, st = sc.render(cam, lights, _params(mode=1), want_packed=False)
            assert _same_bits(img, ref), (view, np.argwhere(img.view(np.uint32) != ref.view(np.uint32))[:8])
            assert (ref[..., 4] < 1.0e6).sum() > 1000
            assert st["rays_primary"] == ref_st["rays_primary"] and st["rays_shadow"] == ref_st["rays_shadow"], (view, st, ref_st)
    finally:
        sc.release()
