"""GPU suite (-m gpu): the hand-written packet walk of a triangle BIH (bih_walk_asm, glome_amd/csrc/bih_packet_asm.hpp, driven by
bih_tri_packet_hw in rt_device.hpp) on ray packets composed lane by lane -- through glome_trace_batch, whose work item is 64 consecutive
rays of the caller's stream, one per lane.

The scenes are the ladders of tests/ladder.py (69 triangles: a comb of 16 branches with a leaf per rung, leaves of 1 .. 9 and 13
triangles, exact duplicates; six copies: along x, y and z, both ways, and a variant whose rungs are mirrors).  tests/test_packet_model.py
asserts, without a GPU, that they reach what this suite is about: the commit gives them a 12-entry LDS stack with overflow columns and the
instances that call the walk; every "deep" packet here holds 16 pending entries -- four pushes and four pops beyond the LDS part, each a
hand-off PKW_PUSH_OVERFLOW / PKW_POP_OVERFLOW through the dump block, a C++ step and a re-entry with sp > 0 -- in every octant, on every
split axis, in the closest-hit mode and in the any-hit mode (the shadow rays that leave the screen for the light beyond the far end).

Expected values: the fp64 oracle, one 1 x 1 frame per ray (ladder.oracle_trace), and the faithful instance (trace_params(faithful=1): the
reference's own per-lane traversal), which the early-out instances must equal bit for bit.

Colour caps.  The rays are drawn clear of every edge, their shadow rays and reflected rays too (Ladder.clear), and the materials are
matte; the oracle computing in fp32 moves the colour of NO ray of any stream beyond the 1e-4 gate (ladder.AWAY_FP32: 0 of 512 deep, 0 of
384 screen, 0 of 768 mixed rays, on all eight ladders), and agrees with the fp64 oracle on the primitive of every ray.  The cap asserted
here is twice the fp32 oracle's count, as tests/test_trace_batch.py does: 0.  The GPU's own counts on an MI355X are 0 as well: no ray beyond
the gate, no flip, no other primitive, no depth beyond 1e-4, on every stream of every ladder.  The frame's instance on that GPU: the two-row flagship,
k_render_flat<false,false,false,TRI,6,true>, 119 work items."""
import ctypes as C

import numpy as np
import pytest

import ladder
from helpers import oracle_for, product_camera_lights
from test_kernel_choice import export_choice as render_choice, instance_name as render_instance_name
from glome_amd import _lib as L
from glome_amd import api

pytestmark = pytest.mark.gpu

VARIANTS = [(a, s, False) for a, s in ladder.CONFIGS] + [(0, 1, True), (2, -1, True)]
IDS = ["%s%s%s" % ("xyz"[a], "+" if s > 0 else "-", "-mirror" if m else "") for a, s, m in VARIANTS]
MISS = np.array([0, 0, 0, 0, 1e6], np.float32)


class Committed:
    """a ladder on the GPU, its fp64 oracle and the id maps back to the SceneDesc"""

    def __init__(self, ctx, v):
        self.lad = ladder.Ladder(*v)
        self.variant = "mirror" if v[2] else "plain"
        sd = self.lad.sd
        self.b = api.Builder()
        self.nm, _ = sd.replay(self.b)
        self.sc = ctx.commit(self.b, self.nm[sd.root])
        self.cam, self.lights = product_camera_lights(sd)
        self.o, om, _ = oracle_for(sd)
        self.oroot = om[sd.root]
        self.sd_of_prod = np.full(max(self.nm) + 2, -1); self.sd_of_prod[np.asarray(self.nm)] = np.arange(len(self.nm))
        self.sd_of_oracle = np.full(max(om) + 2, -1); self.sd_of_oracle[np.asarray(om)] = np.arange(len(om))
        self._deep = None

    def deep(self):
        """the deep stream, its two traces and its oracle rows: made once, shared, never written to"""
        if self._deep is None:
            ro, rd, _ = self.lad.deep_set()
            r = both_instances(self, ro, rd)
            ref = oracle_rows(self, ro, rd)
            for a in [ro, rd] + [x for x in list(r.values()) + list(ref.values()) if isinstance(x, np.ndarray)]:
                a.setflags(write=False)
            self._deep = (ro, rd, r, ref)
        return self._deep


@pytest.fixture(scope="module")
def committed(gpu_ctx):
    cache = {}

    def get(v):
        if v not in cache:
            cache[v] = Committed(gpu_ctx, v)
        return cache[v]
    yield get
    for c in cache.values():
        c.sc.release()


def rgbad(r):
    return np.concatenate([r["rgba"], r["depth"][:, None]], axis=1)


HIT_KEYS = ("t", "prim", "n", "tex", "rgba", "depth")
RAY_KEYS = ("rays_primary", "rays_shadow", "rays_secondary")


def same_bits(a, b):
    """bit for bit (array_equal on the words, so that -0.0 and 0.0, or two NaNs, are not taken for each other)"""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              np.ascontiguousarray(b[k]).view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in HIT_KEYS)


def both_instances(c, ro, rd, tmax=None):
    """the stream through the early-out instance (the hand-written walk) and through the faithful one: the same bits in t, prim, normal, tex and
    (r, g, b, a, depth), the same ray counts; and t / prim / normal / tex are glome_rayint_batch's.  Returns the early-out instance's result."""
    r = c.sc.trace(ro, rd, c.lights, tmax=tmax, params=api.trace_params(maxdepth=3), want_hit=True)
    f = c.sc.trace(ro, rd, c.lights, tmax=tmax, params=api.trace_params(maxdepth=3, faithful=1), want_hit=True)
    bad = np.flatnonzero(~np.all(rgbad(r).view(np.uint32) == rgbad(f).view(np.uint32), axis=1) | (r["prim"] != f["prim"]) | (r["t"].view(np.uint32) != f["t"].view(np.uint32)))
    assert same_bits(r, f), ("rays that differ from the faithful instance", bad[:16], len(bad))
    assert [r["stats"][k] for k in RAY_KEYS] == [f["stats"][k] for k in RAY_KEYS] and r["stats"]["rays_primary"] == len(ro)
    ri = c.sc.rayint(ro, rd) if tmax is None else c.sc.rayint(ro, rd, tmax)
    assert all(np.array_equal(r[k], ri[k]) for k in ("prim", "tex")) and all(np.array_equal(r[k].view(np.uint32), ri[k].view(np.uint32)) for k in ("t", "n"))
    return r


def oracle_rows(c, ro, rd):
    rows, counts = ladder.oracle_trace(c.o, ro, rd, 3)
    hit = c.o.rayint(c.oroot, ro.astype(np.float64), rd.astype(np.float64))
    return {"rows": rows, "counts": counts, "prim": np.where(hit["prim"] >= 0, c.sd_of_oracle[hit["prim"]], -1), "t": hit["t"]}


def check_against_oracle(c, name, r, ref):
    """hit / miss and the primitive on EVERY ray (for a cluster of exact duplicates: the one the oracle's `nearest` fold reports); depth inside
    1e-4; colour inside 1e-4 on all but at most twice the rays the fp32 oracle itself moves; the oracle's ray counts"""
    got = rgbad(r).astype(np.float64)
    rows = ref["rows"]
    hit_g, hit_r = got[:, 4] < 1e6, rows[:, 4] < 1e6
    prim_g = np.where(r["prim"] >= 0, c.sd_of_prod[r["prim"]], -1)
    away = ladder.colour_away(got, rows)
    both = hit_g & hit_r
    drel = np.abs(got[both, 4] - rows[both, 4]) / np.maximum(1.0, rows[both, 4])
    levels = {"rays": len(got), "away": int(away.sum()), "flips": int((hit_g != hit_r).sum()), "other_prim": int((prim_g != ref["prim"]).sum()), "depth": int((drel > 1e-4).sum())}
    print("packet_walk_vs_oracle", "xyz"[c.lad.axis] + "+-"[c.lad.sign < 0], c.variant, name, levels, {k: r["stats"][k] for k in RAY_KEYS})
    assert np.array_equal(hit_g, r["t"] >= 0)
    assert levels["flips"] == 0 and levels["other_prim"] == 0, (levels, np.flatnonzero(prim_g != ref["prim"])[:16])
    assert levels["depth"] == 0, levels
    assert levels["away"] <= 2 * ladder.AWAY_FP32[(c.variant, name)], (levels, np.flatnonzero(away)[:16])
    assert {k: r["stats"][k] for k in RAY_KEYS} == ref["counts"]


# ---------------------------------------------------------------- 1. single-octant deep packets, twice
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_deep_packets_of_one_octant(committed, v):
    """Two packets per pair of tilt signs: with the six ladders every octant over every split axis.  Every lane's walk holds 16 pending entries;
    the lanes of a packet first meet 11 or more different rungs, five miss everything.  Traced a second time, the stream gives the same bits
    (the overflow path's one recorded fault showed as pixels that changed from run to run)."""
    c = committed(v)
    ro, rd, r, ref = c.deep()
    check_against_oracle(c, "deep", r, ref)
    dup = [t for j in ladder.DUPLICATES for t in c.lad.rung_ids[j]]
    assert np.isin(ref["prim"], dup).sum() >= 20  # (ties inside a leaf are among the first hits)
    again = c.sc.trace(ro, rd, c.lights, params=api.trace_params(maxdepth=3), want_hit=True)
    assert same_bits(r, again)


# ---------------------------------------------------------------- 2. shadow packets: the any-hit mode with a deep stack
@pytest.mark.parametrize("v", VARIANTS[:6], ids=IDS[:6])
def test_shadow_packets_that_run_the_whole_comb(committed, v):
    """Primary rays at the screen; the shadow rays of their hits leave for the light beyond the far end: one packet per quadrant of the screen
    (one octant each), one of two quadrants, one of four.  Between 20 % and 80 % of them meet a rung."""
    c = committed(v)
    ro, rd, _ = c.lad.shadow_set()
    r = both_instances(c, ro, rd)
    ref = oracle_rows(c, ro, rd)
    assert np.all(ref["prim"] == c.lad.screen_id) and ref["counts"]["rays_shadow"] == len(ro)
    so, sd_, sl = ladder.shadow_rays(c.lad, ro, rd, ref["t"])
    occluded = c.o.shadow(c.oroot, so, sd_, sl)
    assert 0.2 <= occluded.mean() <= 0.8, occluded.mean()
    check_against_oracle(c, "shadow", r, ref)
    # the product's own any-hit seam on the same shadow rays (they are clear of every edge: exact)
    so32, sd32 = ladder._f32_rays(so, sd_)
    assert np.array_equal(c.sc.shadow(so32, sd32, sl.astype(np.float32)), occluded)


# ---------------------------------------------------------------- 3. mixed packets
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_mixed_packets(committed, v):
    """Packets of 2, 4 and 8 octants; an octant held by one lane -- lane 0, 31, 32, 63: the ends of the wave and the seam of the two halves of a
    lane mask --; deep lanes between lanes that miss the tree's bounds; deep lanes in the high half of the wave only."""
    c = committed(v)
    ro, rd, what = c.lad.mixed_set()
    r = both_instances(c, ro, rd)
    check_against_oracle(c, "mixed", r, oracle_rows(c, ro, rd))


# ---------------------------------------------------------------- 4. tails and order
def _trace_into_sentinels(c, ro, rd, n):
    """the first n rays through the C ABI into buffers one row longer than n, pre-filled with a sentinel (tests/test_trace_batch.py)"""
    params = api.trace_params(maxdepth=3)
    cols = [np.ascontiguousarray(a[:n]) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
    out = np.full((n + 1, 5), -7.5, np.float32)
    t = np.full(n + 1, -7.5, np.float32); prim = np.full(n + 1, -77, np.int32)
    nx, ny, nz = (np.full(n + 1, -7.5, np.float32) for _ in range(3))
    tex = np.full((n + 1, 8), -77, np.int32)
    la = (L.Light * max(1, len(c.lights)))(*c.lights)
    st = L.Stats()
    rc = c.sc.lib.glome_trace_batch(c.sc.h, n, *[a.ctypes.data_as(L.c_fp) for a in cols], None, la, len(c.lights), C.byref(params), out.ctypes.data_as(L.c_fp),
                                    t.ctypes.data_as(L.c_fp), prim.ctypes.data_as(L.c_ip), nx.ctypes.data_as(L.c_fp), ny.ctypes.data_as(L.c_fp), nz.ctypes.data_as(L.c_fp),
                                    tex.ctypes.data_as(L.c_ip), C.byref(st))
    return rc, {"rgba": out[:, :4], "depth": out[:, 4], "t": t, "prim": prim, "n": np.stack([nx, ny, nz], 1), "tex": tex}, st


@pytest.mark.parametrize("v", [VARIANTS[1], VARIANTS[6]], ids=[IDS[1], IDS[6]])
def test_tails_and_order_on_the_ladder(committed, v):
    """A lane's result depends neither on how many lanes of its wave hold a ray nor on its place in the stream: the first n rays of the deep
    stream (a lone ray, a wave less one, a wave, a wave and one, three waves and 37) give the first n rows of the whole stream's result bit for
    bit, nothing is written past row n, and a permutation of the rays -- which deals every packet lanes of all four tilt octants -- gives the
    permuted rows."""
    c = committed(v)
    ro, rd, base, _ = c.deep()
    for n in (1, 63, 64, 65, 64 * 3 + 37):
        rc, got, st = _trace_into_sentinels(c, ro, rd, n)
        assert rc == 0, c.sc.ctx.err()
        assert same_bits({k: got[k][:n] for k in HIT_KEYS}, {k: base[k][:n] for k in HIT_KEYS}), n
        assert np.all(got["rgba"][n] == -7.5) and got["depth"][n] == -7.5 and got["t"][n] == -7.5 and got["prim"][n] == -77 and np.all(got["n"][n] == -7.5) and np.all(got["tex"][n] == -77), n
        assert (st.rays_primary, st.n_pixels, st.n_tiles) == (n, n, (n + 63) // 64)
    perm = np.random.default_rng(3).permutation(len(ro))
    r = c.sc.trace(ro[perm], rd[perm], c.lights, params=api.trace_params(maxdepth=3), want_hit=True)
    assert same_bits(r, {k: base[k][perm] for k in HIT_KEYS})


# ---------------------------------------------------------------- 5. a tmax per lane
@pytest.mark.parametrize("v", [VARIANTS[3], VARIANTS[4]], ids=[IDS[3], IDS[4]])
def test_a_tmax_per_lane(committed, v):
    """The deep stream with a limit of its own on every lane: cut before the first rung -- a miss; cut between two rungs (a rung per lane, at three
    quarters of its place along the axis: clear of the rung before it, which ends at half) -- the uncut row where the uncut hit lies inside, a
    miss otherwise; cut far beyond the last rung -- the uncut rows.  With tmax exactly a hit's own t the answer is compared with the faithful
    instance alone."""
    c = committed(v)
    lad = c.lad
    ro, rd, base, ref = c.deep()
    n = len(ro)
    u0, du = lad.local(ro)[:, 0], lad.local(rd)[:, 0]
    miss = lambda r, m: np.all(rgbad(r)[m] == MISS) and np.all(r["prim"][m] == -1) and np.all(r["t"][m] == -1)
    # before the first rung (the nearest stands at rung_u(NLEV - 1) less its thickness; the rays start at 0.3 .. 0.5 of that)
    short = both_instances(c, ro, rd, tmax=((0.55 * ladder.rung_u(ladder.NLEV - 1) - u0) / du).astype(np.float32))
    assert miss(short, np.ones(n, bool))
    # between two rungs
    j = np.random.default_rng(5).integers(0, ladder.NLEV - 2, n)
    cut = ((0.75 * ladder.rung_u(0) / 2.0 ** j - u0) / du)
    assert np.all(np.abs(ref["t"] - cut)[ref["t"] >= 0] > 1e-3 * cut[ref["t"] >= 0])  # (no ray's hit is anywhere near its cut)
    mid = both_instances(c, ro, rd, tmax=cut.astype(np.float32))
    inside = (ref["t"] >= 0) & (ref["t"] < cut)
    assert 0.2 < inside.mean() < 0.8
    assert same_bits({k: mid[k][inside] for k in HIT_KEYS}, {k: base[k][inside] for k in HIT_KEYS}) and miss(mid, ~inside)
    # far beyond the last rung
    far = both_instances(c, ro, rd, tmax=np.full(n, 5.0 * ladder.L, np.float32))
    assert same_bits(far, base)
    # exactly the hit's t
    hit = base["t"] >= 0
    both_instances(c, ro[hit], rd[hit], tmax=base["t"][hit])


# ---------------------------------------------------------------- 6. a frame
@pytest.mark.parametrize("v", [VARIANTS[0], VARIANTS[5]], ids=[IDS[0], IDS[5]])
def test_a_frame_along_the_ladder(committed, v):
    """glome_render of the ladder from its heavy end, through an angle so narrow that every 8 x 8 block of the frame runs the whole comb (modelled
    in tests/test_packet_model.py): the frame equals the faithful instance's bit for bit, out5 and packed.  The instance is the two-row flagship
    (printed, and asserted: the scene is one triangle BIH with Surface materials and a 12-entry stack, the launch the whole frame), so its cull
    pass and the overflow of its two-row stack are on the path too."""
    c = committed(v)
    w, h = ladder.FRAME_W, ladder.FRAME_H
    lib = L.load()
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(c.b.h, c.nm[c.lad.sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    P = api.render_params(width=w, height=h, maxdepth=3)
    items = lib.glome_items_layout(C.byref(P), 0, 1, 64, 1, None, 0)
    kind, inst, two_rows, cap = render_choice(lib, [list(t[:8]) + [0, 0, 0, 3, 1, items]])[0].tolist()
    print("frame instance:", render_instance_name(kind, inst), "two_rows", two_rows, "items", items)
    assert two_rows == 1
    img, packed, st = c.sc.render(c.cam, c.lights, P)
    imf, packedf, stf = c.sc.render(c.cam, c.lights, api.render_params(width=w, height=h, maxdepth=3, faithful=1))
    assert np.array_equal(img.view(np.uint32), imf.view(np.uint32)) and np.array_equal(packed, packedf)
    assert [st[k] for k in RAY_KEYS] == [stf[k] for k in RAY_KEYS]
    hit = img[..., 4] < 1e6
    assert 0.05 < hit.mean() < 0.9, hit.mean()  # (some pixels see a rung, the ones around the axis see none)
