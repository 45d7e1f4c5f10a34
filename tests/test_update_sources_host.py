"""The fp32 and indexed update calls, the part that needs no GPU: the nine symbols, and glome_sb_bih_set_triangles_indexed -- the
specification of glome_scene_bih_update_indexed -- held to glome_sb_bih_set_triangles of the gathered array on a shuffled vertex pool
with two decoys no item references, one far outside the scene and one NaN (update_sources.pool)."""
import os
import re
import subprocess

import numpy as np
import pytest

import bihs_refit as BR
import update_sources as US
from glome_amd import _lib as L
from glome_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["glome_sb_bih_set_triangles_indexed", "glome_scene_bih_update_indexed", "glome_scene_bih_update_indexed_dev", "glome_scene_bih_update_f32",
       "glome_scene_bih_update_f32_dev", "glome_scene_mesh_update_f32", "glome_scene_mesh_update_f32_dev", "glome_scene_sphere_bih_update_f32",
       "glome_scene_sphere_bih_update_f32_dev"]


def test_the_nine_symbols_are_declared_exported_bound_and_imported(built):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "glome_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(glome_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "glome_amd", "libglome_hip.so")]).decode()
    exported = set(re.findall(r" T (glome_[a-z0-9_]+)", out))
    bound = {s[0] for s in L.SYMBOLS}
    imported = set(re.findall(r'foreign import ccall\s+(?:safe|unsafe)?\s*"&?(\w+)"', open(os.path.join(ROOT, "INTEGRATION.md")).read()))
    lib = L.load()
    for name in NEW:
        assert name in declared and name in exported and name in bound and name in imported, name
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"enum\s*\{\s*GLOME_F64\s*=\s*0\s*,\s*GLOME_F32\s*=\s*1\s*\}", hdr)


def described(b, tree):
    """what the builder says of a tree: its text, its bound, its dump"""
    return b.show(tree), b.bound(tree), b.bih_dump(tree)


def assert_described_alike(x, y, what):
    assert x[0] == y[0], what
    assert np.array_equal(x[1], y[1]), what
    assert len(x[2]) == len(y[2]) and all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x[2], y[2])), what


@pytest.mark.parametrize("name", ["three", "mixed", "s3_20", "wide"])
def test_the_indexed_builder_call_is_the_dense_one_of_the_gathered_array(built, name):
    P = BR.triangles(name, "V1")
    verts, idx = US.pool(P)
    assert np.isnan(verts).any() and np.nanmax(np.abs(verts)) >= 3.0e4 and len(verts) <= 3 * len(P) + 2
    _, b_ix, _, tree_ix = BR.build(name)
    before = described(b_ix, tree_ix)
    b_ix.bih_set_triangles_indexed(tree_ix, verts, idx)
    _, b_dense, _, tree_dense = BR.build(name)
    b_dense.bih_set_triangles(tree_dense, verts[idx].reshape(-1, 9))
    after = described(b_ix, tree_ix)
    assert_described_alike(after, described(b_dense, tree_dense), name)
    assert after[0] != before[0] and not np.array_equal(after[1], before[1]), "the new triangles must show"
    assert np.abs(after[1]).max() < 1.0e3, "the far decoy is referenced by no item: it is no part of the tree's box"


def test_the_indexed_builder_call_refuses_and_leaves_the_tree_untouched(built):
    P = BR.triangles("mixed", "V1")
    verts, idx = US.pool(P)
    nv, n = len(verts), len(idx)
    _, b, _, tree = BR.build("mixed")
    before = described(b, tree)
    nan_at = int(np.flatnonzero(np.isnan(verts[:, 0]))[0])

    def with_index(item, corner, value):
        bad = idx.copy()
        bad[item, corner] = value
        return bad

    for bad_idx, count, pattern in ((with_index(17, 1, -1), n, r"item 17 has vertex index -1"), (with_index(200, 2, nv), n, rf"item 200 has vertex index {nv}"),
                                    (with_index(5, 0, nan_at), n, r"not finite"), (idx[:-1], n - 1, rf"the bih has {n} items, not {n - 1}"),
                                    (np.concatenate([idx, idx[:1]]), n + 1, rf"the bih has {n} items, not {n + 1}")):
        assert len(bad_idx) == count
        with pytest.raises(api.GlomeError, match=pattern + r".*status -1"):
            b.bih_set_triangles_indexed(tree, verts, bad_idx)
        assert_described_alike(described(b, tree), before, pattern)
    lib = L.load()
    assert lib.glome_sb_bih_set_triangles_indexed(b.h, tree, None, nv, idx.ctypes.data_as(L.c_ip), n) == L.E_INVALID
    assert lib.glome_sb_bih_set_triangles_indexed(b.h, tree, verts.ctypes.data_as(L.c_dp), nv, None, n) == L.E_INVALID
    assert_described_alike(described(b, tree), before, "null arrays")
    b.bih_set_triangles_indexed(tree, verts, idx)  # and the valid call still works
    assert described(b, tree)[0] != before[0]


class NotOnTheGpu:
    """what the device forms' check reads of a torch tensor: here one of fp64 in host memory, nine values"""
    is_cuda, dtype = False, "torch.float64"

    def data_ptr(self):
        return 0

    def is_contiguous(self):
        return True

    def numel(self):
        return 9


def test_the_fp64_device_forms_refuse_a_tensor_in_the_words_they_always_had(built):
    """the three messages as the methods spelled them before they shared _dev_arg; the check comes before the library is called"""
    sc, t = api.Scene(type("NoContext", (), {"lib": L.load()})(), None), NotOnTheGpu()
    for call, msg in [(lambda: sc.mesh_update(1, t), "mesh_update: verts must be a contiguous CUDA torch.float64 tensor of 3 values per row"),
                      (lambda: sc.bih_update(1, t), "bih_update: pts9 must be a contiguous CUDA torch.float64 tensor of 9 values per row"),
                      (lambda: sc.sphere_bih_update(1, t), "sphere_bih_update: c3r must be a contiguous CUDA torch.float64 tensor of 4 values per row")]:
        with pytest.raises(api.GlomeError) as e:
            call()
        assert str(e.value) == msg
