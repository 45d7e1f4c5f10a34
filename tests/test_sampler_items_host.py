"""CPU suite: the adaptive sampler's item plan -- which (region, block, lane) of a pass stands for which pixel of a tile.  The
kernel's own functions (ss_plan, ss_regions_per_tile, ss_region_blocks, ss_block_pixel; rt_device.hpp) are walked on the host
the way ss_frame_loop walks them (tests/hostsim: hostsim_ss_items) for every blocksize, every clipped tile and every region shape
the runtime can pick.  The lanes with dx < tw and dy < th must be exactly the pixels the reference's pass visits
(Glome.hs:241-302), each once; passes 1-4 together must cover the tile exactly once; ss_plan must count the regions."""
import ctypes as C

import numpy as np
import pytest

from helpers import hostsim_lib

TH = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def reference_pass(p):
    """the pixels of a 65 x 65 tile that the reference's pass p visits, as [dy, dx] (a smaller tile visits the same, clipped)"""
    m = np.zeros((65, 65), bool)
    if p in (1, 2):  # forM_ [xtmin, xtmin+2 ..] / [ytmin, ytmin+2 ..], mod (dx + dy) 4 == 0 / 2   (Glome.hs:241-243, 251-253)
        for x in range(0, 65, 2):
            for y in range(0, 65, 2):
                m[y, x] = (x + y) % 4 == (0 if p == 1 else 2)
    elif p == 3:     # [xtmin+1, xtmin+3 ..] x [ytmin+1, ytmin+3 ..]   (:272-273)
        m[1::2, 1::2] = True
    elif p == 4:     # mod (dx + dy) 2 == 1   (:283-285)
        for x in range(65):
            for y in range(65):
                m[y, x] = (x + y) % 2 == 1
    else:            # every pixel (:301-302)
        m[:] = True
    return m


@pytest.fixture(scope="module")
def lib(built):
    lib = hostsim_lib()
    lib.hostsim_ss_items.restype = C.c_longlong
    return lib


def region_shapes(lib):
    """{name: (rw[8], rh[8])} indexed by pass: what render_impl (runtime.hip) picks by the tier and the frames of a launch"""
    out = {}
    for size in (0, 1, 2):  # the flat tier: one or two frames, three to seven, eight or more
        rw, rh = [0] * 8, [0] * 8
        for p in range(1, 6):
            a, b = C.c_int(), C.c_int()
            lib.hostsim_ss_region_shape(p, size, C.byref(a), C.byref(b))
            rw[p], rh[p] = a.value, b.value
        out[f"flat{size}"] = (rw, rh)
    out["generic_1x1"] = ([0, 1, 1, 1, 1, 1, 0, 0], [0, 1, 1, 1, 1, 1, 0, 0])     # a frame or two
    out["generic_2x1"] = ([0, 1, 1, 2, 2, 2, 0, 0], [0, 1, 1, 1, 1, 1, 0, 0])     # three to eleven frames: two blocks from pass 3
    out["generic_twelve"] = ([0, 1, 2, 2, 2, 3, 0, 0], [0, 1, 1, 2, 2, 3, 0, 0])  # twelve frames or more
    return out


def walk(lib, p, bs, tw, th, shape, ntiles=1, nframes=1, want_items=False):
    rw, rh = (C.c_int * 8)(*shape[0]), (C.c_int * 8)(*shape[1])
    cover = np.zeros((5 if p == 0 else 1, 65, 65), np.uint16)
    plan = np.zeros(21, np.uint32)
    cap = 1 << 16
    items = np.zeros((cap, 5), np.int32) if want_items else None
    n = lib.hostsim_ss_items(p, bs, tw, th, rw, rh, ntiles, nframes, items.ctypes.data_as(C.POINTER(C.c_int)) if want_items else None, C.c_longlong(cap if want_items else 0),
                             cover.ctypes.data_as(C.POINTER(C.c_ushort)), plan.ctypes.data_as(C.POINTER(C.c_uint)))
    assert n >= 0, (n, p, bs, tw, th)
    P = {"per_tile": plan[0:6], "nrx": plan[6:12], "first": plan[12:19], "tiles_per_head": int(plan[19]), "heads": int(plan[20])}
    if want_items:
        assert n <= cap
        items = items[:n]
    return n, cover, P, items


def test_every_lane_of_every_region_is_a_candidate_of_its_pass_once(lib):
    want = np.stack([reference_pass(p) for p in range(1, 6)]).astype(np.uint16)
    assert np.array_equal(want[:4].sum(0), np.ones((65, 65)))  # (the reference's passes 1-4 visit every pixel once)
    shapes = region_shapes(lib)
    checked = 0
    for name, shape in shapes.items():
        for bs in range(1, 66):
            for th in sorted({t for t in TH if t <= bs} | {bs}):
                for tw in range(1, bs + 1):
                    n, cover, P, _ = walk(lib, 0, bs, tw, th, shape)
                    inside = np.zeros((65, 65), np.uint16); inside[:th, :tw] = 1
                    if not np.array_equal(cover, want * inside):
                        p = next(p for p in range(1, 6) if not np.array_equal(cover[p - 1], want[p - 1] * inside))
                        bad = np.argwhere(cover[p - 1] != want[p - 1] * inside)
                        raise AssertionError(f"{name} blocksize {bs} tile {tw}x{th} pass {p}: pixel dx={bad[0][1]} dy={bad[0][0]} came up {cover[p - 1][tuple(bad[0])]} times, "
                                             f"the reference visits it {int((want[p - 1] * inside)[tuple(bad[0])])} times ({len(bad)} pixels differ)")
                    assert np.array_equal(cover[:4].sum(0), inside)  # passes 1-4: the tile, once
                    checked += 1
    assert checked > 6 * 15000


@pytest.mark.parametrize("bs,tw,th", [(65, 65, 65), (65, 1, 65), (65, 65, 1), (65, 33, 17), (16, 16, 16), (16, 9, 2), (7, 7, 7), (1, 1, 1), (33, 32, 33)])
def test_the_item_list_is_what_the_cover_counts(lib, bs, tw, th):
    """the list of (region, block, lane, dx, dy) behind the counts: no triple twice, regions below ss_plan's per_tile, a lane's pixel
    fits the 8 + 8 bits of the kernel's need list, and the pixels inside the tile are the cover"""
    for name, shape in region_shapes(lib).items():
        for p in range(1, 6):
            n, cover, P, items = walk(lib, p, bs, tw, th, shape, want_items=True)
            assert n % 64 == 0 and len(items) == n
            r, b, lane, dx, dy = items.T
            assert len({(int(a), int(c), int(d)) for a, c, d in zip(r, b, lane)}) == n
            assert n == 0 or (r.max() < P["per_tile"][p] and lane.max() == 63 and b.max() < shape[0][p] * shape[1][p])
            inside = (dx < tw) & (dy < th)
            assert (dx >= 0).all() and (dy >= 0).all() and (dx[inside] < 256).all() and (dy[inside] < 256).all()
            got = np.zeros((65, 65), np.uint16)
            np.add.at(got, (dy[inside], dx[inside]), 1)
            assert np.array_equal(got, cover[0]), (name, p)
            assert inside.sum() == (reference_pass(p)[:th, :tw]).sum()


def test_ss_plan_counts_the_items(lib):
    """first[] and per_tile[]: per pass per_tile regions for each of the tiles_per_head tiles of a head's sequence, passes in order; the
    plan's regions are laid out for a full tile and reach every block of it"""
    for name, shape in region_shapes(lib).items():
        for bs in (1, 7, 16, 33, 64, 65):
            for ntiles, nframes in ((1, 1), (6, 1), (9, 3), (4, 12), (17, 8)):
                _, _, P, _ = walk(lib, 1, bs, bs, bs, shape, ntiles, nframes)
                assert P["heads"] == 8 and P["tiles_per_head"] == (ntiles * nframes + 7) // 8
                assert P["tiles_per_head"] * P["heads"] >= ntiles * nframes
                assert P["first"][1] == 0
                for p, (bw, bh) in zip(range(1, 6), ((32, 16), (32, 16), (16, 16), (16, 8), (8, 8))):
                    rw, rh = shape[0][p], shape[1][p]
                    nrx, nry = -(-bs // (bw * rw)), -(-bs // (bh * rh))
                    assert P["nrx"][p] == nrx and P["per_tile"][p] == nrx * nry, (name, bs, p)
                    assert P["first"][p + 1] - P["first"][p] == P["per_tile"][p] * P["tiles_per_head"]
