"""The device tree builders (glome_sb_bih_dev, glome_sb_mesh_dev; bih_build_device.hpp) held to the host builders on every case of
tests/tree_build_cases.py, bit for bit and with no allowance -- the wave reductions, the scan and scatter at segment boundaries on
and beside 64, 256 and 1024, the pools, the level limit -- plus the refusals as statuses and the one size that reaches the carry
loop of the scan's second stage.  tests/test_tree_build_model_host.py shows, without a GPU, that each case goes where it says."""
import ctypes as C
import re
import time

import numpy as np
import pytest

import tree_build_cases as TC
from glome_amd import _lib as L
from glome_amd import api

pytestmark = pytest.mark.gpu

BUILDS = [c for c in TC.CASES if c.dev_refusal is None]
REFUSALS = [c for c in TC.CASES if c.dev_refusal is not None]
STATUS = {"E_SCENE": L.E_SCENE, "E_LIMIT": L.E_LIMIT, "E_INVALID": L.E_INVALID}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def assert_same_bih(b, host, dev):
    dh, dd = b.bih_dump(host), b.bih_dump(dev)
    assert np.array_equal(bits(dh[0]), bits(dd[0])) and np.array_equal(bits(dh[1]), bits(dd[1]))  # split planes
    assert np.array_equal(dh[2], dd[2]) and np.array_equal(dh[3], dd[3]) and np.array_equal(dh[4], dd[4])  # axes, leaf sizes, leaf items in order
    assert np.array_equal(bits(b.bound(host)), bits(b.bound(dev)))


@pytest.mark.parametrize("case", BUILDS, ids=repr)
def test_device_built_tree_is_the_host_builders(gpu_ctx, case):
    b = api.Builder()
    if case.kind == "bih":
        ids = case.make(b)
        host = b.bih(ids)
        dev, _ = gpu_ctx.bih(b, ids)
        assert_same_bih(b, host, dev)
    else:
        V, T = case.make()
        none = np.zeros((0, 3))
        host = b.mesh(V, none, T, [])
        dev, _ = gpu_ctx.mesh(b, V, none, T, [])
        assert b.show(host) == b.show(dev)  # every box of the BVH and every leaf's triangle list
        assert np.array_equal(bits(b.bound(host)), bits(b.bound(dev))) and b.primcount(host) == b.primcount(dev)


@pytest.mark.parametrize("case", REFUSALS, ids=repr)
def test_refusals_are_statuses_and_the_context_works_on(gpu_ctx, case):
    """The status and message of the host builder where it refuses too (the fixed points of build_rec end as a finite loop's status, not
    at a stack's end), the level limit where only the device has one; no node is added; the next build on the same context and builder
    is the host's tree."""
    b = api.Builder()
    ms = C.c_float(0)
    if case.kind == "bih":
        arr, p = L.ivec(case.make(b))
        host_call = lambda: b.lib.glome_sb_bih(b.h, p, len(arr))
        dev_call = lambda: gpu_ctx.lib.glome_sb_bih_dev(gpu_ctx.h, b.h, p, len(arr), C.byref(ms))
    else:
        V, T = case.make()
        mesh_args = (V.ctypes.data_as(L.c_dp), len(V), None, 0, T.ctypes.data_as(L.c_ip), len(T), None, 0)
        host_call = lambda: b.lib.glome_sb_mesh(b.h, *mesh_args)
        dev_call = lambda: gpu_ctx.lib.glome_sb_mesh_dev(gpu_ctx.h, b.h, *mesh_args, C.byref(ms))
    if case.refusal is not None:
        assert host_call() == STATUS[case.refusal[0]]
        host_message = b.lib.glome_sb_last_error(b.h).decode()
    before = b.sphere((0.0, 0.0, 0.0), 1.0)
    rc = dev_call()
    assert rc == STATUS[case.dev_refusal[0]], gpu_ctx.err()
    assert re.search(case.dev_refusal[1], gpu_ctx.err())
    if case.refusal is not None:
        assert gpu_ctx.err() == host_message
    else:
        assert host_call() >= 0  # the host builder has no level limit
        before += 1
    assert b.sphere((0.0, 0.0, 0.0), 1.0) == before + 1  # the refused call left no node behind
    ids = TC.ORDINARY.make(b)
    host = b.bih(ids)
    dev, _ = gpu_ctx.bih(b, ids)
    assert_same_bih(b, host, dev)


def test_the_carry_loop_of_the_scans_second_stage(gpu_ctx):
    """n = 1024 * 1024 + 1025 items make 1026 block sums: the one block of k_bb_scan_sums goes round twice and carries the first
    round's total into the second.  Nothing smaller reaches that loop.  Triangles on a jittered dyadic grid (multiples of 1/1024)."""
    n = 1024 * 1024 + 1025
    rng = np.random.default_rng(5)
    i = np.arange(n)
    p0 = np.stack([(i % 1025).astype(np.float64), np.zeros(n), (i // 1025).astype(np.float64)], 1) + rng.integers(0, 512, size=(n, 3)) / 1024
    p1 = p0 + np.array([0.5, 0.0, 0.0]) + rng.integers(0, 256, size=(n, 3)) / 1024
    p2 = p0 + np.array([0.0, 0.0, 0.5]) + rng.integers(0, 256, size=(n, 3)) / 1024
    b = api.Builder()
    ids = b.triangles_bulk(np.concatenate([p0, p1, p2], 1))
    t0 = time.perf_counter()
    host = b.bih(ids)
    t1 = time.perf_counter()
    dev, ms = gpu_ctx.bih(b, ids)
    t2 = time.perf_counter()
    print(f"bih of {n} triangles: host {t1 - t0:.2f} s; device {ms:.1f} ms on the GPU, {t2 - t1:.2f} s wall with bounds, upload and read-back")
    assert_same_bih(b, host, dev)
