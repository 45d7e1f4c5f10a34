"""CPU suite: the walk-entry table (glome_amd/csrc/rt_types.h DScene::walk, flatten.hpp emit_walk).

The two-row kernels and their cull pass read a root entry's flags, header index and tex prefix from one 16-byte record of the table
where every other instance reads `entries[e]` and then `recs[entries[e].x]`.  Here the table the flattener leaves is held, word for
word, against what those loops read from the other pools (rt_device.hpp closest_flat / occluded_flat, the branch without TABLE):

    walk[e] = (entries[e].z, recs[entries[e].x].y, entries[e].y, recs[entries[e].x].x)

for every entry, on crafted scenes, and again after each host update call that exists for a triangle bih.  The header a record points
to must be a triangle tree's wherever the two-row rule admits the scene (the readers take that for granted: capi_shared.hpp
commit_rules).  The pools come from tests/walk_table/walk_table_dump.cpp, which runs the product's flattener as a commit does and is
built here into a temporary directory.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RF_KINDMASK, RF_NOVIS, RF_NOSHADOW, R_BIH, BC_TRI = 0xFF, 1 << 8, 1 << 9, 15, 1
ENTRIES, RECS, BIHHDR, WALK, INFO = range(5)


@pytest.fixture(scope="module")
def dump(built, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("walk_table") / "libwalk_table_dump.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "walk_table", "walk_table_dump.cpp")])
    lib = C.CDLL(so)
    lib.walk_table_dump.restype = C.c_int
    lib.walk_table_dump.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int]

    def pools(b, root):
        out = {}
        for what in (ENTRIES, RECS, BIHHDR, WALK, INFO):
            n = lib.walk_table_dump(C.c_void_p(b.h), int(root), what, None, 0)
            assert n >= 0, "the flattener refused the scene"
            a = np.zeros(max(1, n), np.uint32)
            assert lib.walk_table_dump(C.c_void_p(b.h), int(root), what, a.ctypes.data_as(C.POINTER(C.c_uint32)), n) == n
            out[what] = a[:n].reshape(-1, 4) if what != INFO else a[:n]
        return out
    return pools


def _tris(n, dx=0.0, dy=0.0, seed=1):
    """n small triangles scattered over a 4 x 4 patch"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-2, 2, (n, 1, 3)) * np.array([1, 0.2, 1]) + rng.uniform(-0.3, 0.3, (n, 3, 3))
    p[..., 0] += dx
    p[..., 1] += dy
    return p.reshape(n, 9)


def _terrain(b, dx=0.0):
    t = scenes.heightfield_triangles(32).copy()
    t[:, 0::3] += dx
    return b.bih(b.triangles_bulk(t))


def _matte(b, rgb=(0.8, 0.5, 0.4)):
    return b.material_surface(rgb, 1, 0.2, 0.8, 0, 0)


def _two_rows(b, root):
    """does the launch of a 1920 x 1080 renderTile frame of this scene get the flagship instance?"""
    lib = L.load()
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(b.h, root, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    row = np.array([list(t[:8]) + [0, 0, 0, 1, 1, 32400]], dtype=np.int64)
    out = np.zeros((1, 4), dtype=np.int32)
    assert lib.glome_kernel_choice(1, row.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == 1
    return bool(out[0, 2])


def _check(pools, b, root, n_entries, flags=None, tex_ids=None):
    """the table against the parent's reads, for every entry; returns the table"""
    P = pools(b, root)
    ent, recs, hdr, walk = P[ENTRIES], P[RECS], P[BIHHDR], P[WALK]
    assert len(walk) == len(ent) and (P[INFO][0] != 0 or P[INFO][1] == len(ent) == n_entries), (len(walk), len(ent), P[INFO], n_entries)
    for e in range(len(ent)):
        rec = recs[ent[e, 0]]
        assert walk[e].tolist() == [ent[e, 2], rec[1], ent[e, 1], rec[0]], (e, walk[e], ent[e], rec)
    if _two_rows(b, root):  # what the readers do not look at: every entry a bih, every header a triangle tree's
        assert P[INFO][0] == 0
        for e in range(len(ent)):
            assert walk[e, 3] & RF_KINDMASK == R_BIH and hdr[3 * walk[e, 1] + 1, 3] == BC_TRI, (e, walk[e])
    if flags is not None:
        assert [int(w) & (RF_NOVIS | RF_NOSHADOW) for w in walk[:, 0]] == flags
    if tex_ids is not None:
        assert [int(w) for w in walk[:, 2]] == tex_ids
    return walk


def test_one_triangle_bih(dump):
    for n in (4, 64):
        b = api.Builder()
        root = b.tex(b.bih(b.triangles_bulk(_tris(n))), _matte(b))
        _check(dump, b, root, 1, flags=[0])
    b = api.Builder()
    root = b.tex(_terrain(b), _matte(b))
    assert _two_rows(b, root)
    _check(dump, b, root, 1, flags=[0])


def test_noshadow_and_onlyshadow_entries(dump):
    b = api.Builder()
    m = _matte(b)
    root = b.group([b.tex(_terrain(b), m), b.noshadow(b.tex(b.bih(b.triangles_bulk(_tris(4, 6.0, 0.4))), m)), b.onlyshadow(b.tex(b.bih(b.triangles_bulk(_tris(64, -4.0, 3.0))), m))])
    assert _two_rows(b, root)
    _check(dump, b, root, 3, flags=[0, RF_NOSHADOW, RF_NOVIS], tex_ids=[m + 1] * 3)


def test_a_bih_under_tex_levels_and_an_entry_that_is_not_visible(dump):
    b = api.Builder()
    m1, m2 = _matte(b), _matte(b, (0.1, 0.6, 0.9))
    # two Tex levels: the inner id in front (flatten.hpp collect_entries); a bare bih: no prefix; an OnlyShadow entry is not visible
    root = b.group([b.tex(b.tex(_terrain(b), m1), m2), b.bih(b.triangles_bulk(_tris(16, 5.0))), b.onlyshadow(b.tex(b.bih(b.triangles_bulk(_tris(8, 0.0, 3.0))), m2))])
    assert _two_rows(b, root)
    _check(dump, b, root, 3, flags=[0, 0, RF_NOVIS], tex_ids=[((m2 + 1) << 16) | (m1 + 1), 0, m2 + 1])


def test_the_table_after_each_host_update_of_a_triangle_bih(dump):
    b = api.Builder()
    m = _matte(b)
    small = b.bih(b.triangles_bulk(_tris(64, 6.0, 0.4)))
    root = b.group([b.tex(_terrain(b), m), b.noshadow(b.tex(small, m))])
    before = _check(dump, b, root, 2, flags=[0, RF_NOSHADOW]).copy()
    new = _tris(64, 6.5, 0.6, seed=2)
    b.bih_set_triangles(small, new)
    assert np.array_equal(_check(dump, b, root, 2, flags=[0, RF_NOSHADOW]), before)  # (same slots: an update moves no record)
    b.bih_set_triangles_indexed(small, _tris(64, 7.0, 0.2, seed=3).reshape(-1, 3), np.arange(192, dtype=np.int32).reshape(-1, 3))
    assert np.array_equal(_check(dump, b, root, 2, flags=[0, RF_NOSHADOW]), before)
    assert _two_rows(b, root)


def test_a_nested_refit_and_a_refused_scene_get_a_table_too(dump):
    """a triangle bih under another bih: the scene renders on the generic tier, which has no root program -- the table is the padding
    entry's record and nothing reads it; after new triangles below and a refit of the tree above it is what it was"""
    b = api.Builder()
    m = _matte(b)
    inner = b.bih(b.triangles_bulk(_tris(16)))
    outer = b.bih([b.tex(inner, m), b.sphere((5, 0, 0), 1.0)])
    assert not _two_rows(b, outer)
    before = _check(dump, b, outer, 0).copy()
    assert len(before) == 1
    b.bih_set_triangles(inner, _tris(16, 0.5, seed=4))
    for t in b.bihs_above(outer, inner):
        b.bih_refit(t)
    assert np.array_equal(_check(dump, b, outer, 0), before)
    # refused by the rule for its material, on the flat tier: a table all the same, the same words
    b2 = api.Builder()
    root = b2.tex(_terrain(b2), b2.material_reflect(0.5))
    assert not _two_rows(b2, root)
    _check(dump, b2, root, 1, flags=[0])


def _traits(b, root):
    t = np.zeros(11, dtype=np.int64)
    assert L.load().glome_sb_scene_traits(b.h, root, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return t


def test_an_entry_that_is_no_bih_keeps_a_scene_off_the_table_readers(dump):
    """The readers walk every entry as a triangle bih, and the guarantee is made at commit (capi_shared.hpp commit_rules clears the trait
    pk_all).  A lone triangle beside the terrain is refused by its class already, as it was before the table.  The one scene of class
    CLS_BIH_TRI with an entry that is no bih is the scene without entries -- Void and wrappers of it give the root program nothing, and the
    device gets a padding entry whose record is no bih: its class mask is empty, which scene_class takes for the triangle class, and only
    commit_rules' look at the records clears pk_all for it.  (Its shallow stack refuses it as well; so the trait itself is asserted, and
    the rule is asked again with the stack the two-row kernels want.)"""
    b = api.Builder()
    m = _matte(b)
    root = b.group([b.tex(_terrain(b), m), b.tex(b.triangle((0, 3, 0), (1, 3, 0), (0, 3, 1)), m)])
    assert _traits(b, root)[1] & 16 and not _two_rows(b, root)  # (CLS_PRIMS)
    _check(dump, b, root, 2)

    b = api.Builder()
    terrain = b.tex(_terrain(b), _matte(b))
    assert _traits(b, terrain)[5] == 1 and _two_rows(b, terrain)
    for root in (b.group([]), b.noshadow(b.tex(b.group([]), _matte(b)))):
        P = dump(b, root)
        assert P[INFO].tolist() == [0, 1] and len(P[WALK]) == 1 and P[WALK][0, 3] & RF_KINDMASK != R_BIH, (P[INFO], P[WALK])
        _check(dump, b, root, 1)
        t = _traits(b, root)
        assert (t[0], t[1], t[5]) == (0, 0, 0), t  # flat tier, no class bit -- and pk_all cleared
        row = np.array([list(t[:6]) + [_traits(b, terrain)[6], t[7], 0, 0, 0, 1, 1, 32400]], dtype=np.int64)
        out = np.zeros((1, 4), dtype=np.int32)
        assert L.load().glome_kernel_choice(1, row.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == 1
        assert out[0, 2] == 0
        row[0, 5] = 1  # (the same scene with the trait as the flattener alone leaves it: admitted -- the line is what refuses it)
        assert L.load().glome_kernel_choice(1, row.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(L.c_ip)) == 1
        assert out[0, 2] == 1
