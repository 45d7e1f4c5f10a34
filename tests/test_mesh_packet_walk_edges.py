"""GPU suite (-m gpu): the packet walk of a Mesh BVH (mesh_closest_wave, glome_amd/csrc/rt_device.hpp; its stack LaneStackCols; the tie rule
of closest_flat's root list) on ray packets composed lane by lane -- through glome_trace_batch, whose work item is 64 consecutive rays of the
caller's stream, one per lane.

The scenes are the mesh ladders of tests/mesh_ladder.py (157 triangles: a comb with a leaf per rung, leaves of 1 .. 9, 13, 15 and 20
triangles, exact duplicates, and under the comb a 6 x 6 patch with holes, split across the other two axes; ten copies: along x, y and z,
both ways, two whose second material is a mirror, two whose root is a group of the mesh twice).  tests/test_mesh_packet_model.py asserts,
without a GPU, that they reach what this suite is about: the commit gives them a 12-entry LDS stack with 38 overflow entries and the MESH
instances; every "deep" packet here holds 27 or 28 entries, pushes and pops 75 .. 117 times beyond the LDS part, and visits 20 .. 35 nodes in
all three passes while the LDS part is full, on every axis, both ways.

Expected values: the fp64 oracle, one 1 x 1 frame per ray (ladder.oracle_trace), and the faithful instance (trace_params(faithful=1): the
per-lane mesh_closest), which the early-out instances must equal bit for bit.

Colour caps.  The deep and the mixed stream are drawn clear of every edge, their reflected rays too (Ladder.clear); a Mesh casts no shadow and
the materials are matte; the oracle computing in fp32 moves the colour of NO ray of either stream beyond the 1e-4 gate
(mesh_ladder.AWAY_FP32: 0 of 512 deep, 0 of 512 mixed rays, on all ten variants), and agrees with the fp64 oracle on the primitive and the
material of every ray.  The cap asserted here is twice the fp32 oracle's count, as tests/test_trace_batch.py does: 0.

The GPU's own counts on an MI355X are 0 as well, on each of the ten variants and both streams: no ray beyond the gate, no flip, no other
primitive, no other material, no depth beyond 1e-4; the ray counts are the oracle's (deep: 512 + 472 shadow, the mirrors 512 + 228 + 245
and 512 + 223 + 249 secondary; mixed: 512 + 397, the mirrors 512 + 189 + 209 and 512 + 195 + 203).  Census of the edges stream (808 rays
at shared edges and vertices, not asserted): 622 .. 649 hit; 333 .. 352 report another triangle than the fp64 oracle's or flip -- as expected
of rays that fp32 rounding puts to either side of an edge -- and every one of them equals the faithful instance.  The frame: 360 + 300 shadow
rays, 83 % of the pixels hit."""
import numpy as np
import pytest

import ladder
import mesh_ladder as ML
from helpers import oracle_for, product_camera_lights
from test_packet_walk_edges import HIT_KEYS, MISS, RAY_KEYS, _trace_into_sentinels, both_instances, oracle_rows, rgbad, same_bits
from glome_amd import api

pytestmark = pytest.mark.gpu

VARIANTS, IDS = ML.VARIANTS, ML.IDS
DELTA = 1e-4  # kDelta, Vec.hs:40: what pads every box of a Mesh


class Committed:
    """a mesh ladder on the GPU, its fp64 oracle and the id maps back to the SceneDesc"""

    def __init__(self, ctx, v):
        self.lad = ML.MeshLadder(*v)
        self.name = IDS[VARIANTS.index(v)]
        sd = self.lad.sd
        self.b = api.Builder()
        self.nm, self.mm = sd.replay(self.b)
        self.sc = ctx.commit(self.b, self.nm[sd.root])
        self.cam, self.lights = product_camera_lights(sd)
        self.o, om, self.omm = oracle_for(sd)
        self.oroot = om[sd.root]
        self.sd_of_prod = np.full(max(self.nm) + 2, -1); self.sd_of_prod[np.asarray(self.nm)] = np.arange(len(self.nm))
        self.sd_of_oracle = np.full(max(om) + 2, -1); self.sd_of_oracle[np.asarray(om)] = np.arange(len(om))
        self._deep = None

    def oracle_rows(self, ro, rd):
        """ladder.oracle_trace's rows and counts, the oracle's rayint: the SceneDesc id of the mesh hit, t, and the PRODUCT's id of the hit's material"""
        ref = oracle_rows(self, ro, rd)
        a = self.o.rayint(self.oroot, ro.astype(np.float64), rd.astype(np.float64))
        prod_of_oracle = {om: pm for om, pm in zip(self.omm, self.mm)}
        ref["mat"] = np.array([prod_of_oracle[x] if p >= 0 else -1 for x, p in zip(a["tex"][:, 0], a["prim"])])
        ref["n"] = a["n"]
        return ref

    def deep(self):
        """the deep stream, its two traces and its oracle rows: made once, shared, never written to"""
        if self._deep is None:
            ro, rd = self.lad.deep_set()
            r = both_instances(self, ro, rd)
            ref = self.oracle_rows(ro, rd)
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


def check_against_oracle(c, name, r, ref):
    """hit / miss, the primitive (the mesh; of the twin the second) and the material (among exact duplicates: that of the one `nearest` keeps) on
    EVERY ray; depth inside 1e-4; colour inside 1e-4 on all but at most twice the rays the fp32 oracle itself moves; the oracle's ray counts"""
    got = rgbad(r).astype(np.float64)
    rows = ref["rows"]
    hit_g, hit_r = got[:, 4] < 1e6, rows[:, 4] < 1e6
    prim_g = np.where(r["prim"] >= 0, c.sd_of_prod[r["prim"]], -1)
    away = ladder.colour_away(got, rows)
    both = hit_g & hit_r
    drel = np.abs(got[both, 4] - rows[both, 4]) / np.maximum(1.0, rows[both, 4])
    levels = {"rays": len(got), "away": int(away.sum()), "flips": int((hit_g != hit_r).sum()), "other_prim": int((prim_g != ref["prim"]).sum()),
              "other_material": int((np.where(hit_g, r["tex"][:, 0], -1) != ref["mat"]).sum()), "depth": int((drel > 1e-4).sum())}
    print("mesh_packet_walk_vs_oracle", c.name, name, levels, {k: r["stats"][k] for k in RAY_KEYS})
    assert np.array_equal(hit_g, r["t"] >= 0)
    assert levels["flips"] == 0 and levels["other_prim"] == 0 and levels["other_material"] == 0, (levels, np.flatnonzero(prim_g != ref["prim"])[:16])
    assert set(ref["prim"]) == {-1, c.lad.mesh_ids[-1]}
    assert levels["depth"] == 0, levels
    assert levels["away"] <= 2 * ML.AWAY_FP32[(c.lad.kind, name)], (levels, np.flatnonzero(away)[:16])
    assert {k: r["stats"][k] for k in RAY_KEYS} == ref["counts"]
    if not c.lad.mirror:  # a Mesh casts no shadow: one shadow ray per hit, every one of them lit
        assert ref["counts"]["rays_shadow"] == int(hit_r.sum()) and ref["counts"]["rays_secondary"] == 0


# ---------------------------------------------------------------- 1. deep packets, twice; mixed packets
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_deep_packets_of_four_tilt_quadrants(committed, v):
    """Eight forward packets from in front of the patch, the four tilt-sign quadrants in each: 27 or 28 entries pending, three passes at 20 .. 35
    nodes beyond the LDS part (tests/test_mesh_packet_model.py).  The early-out instance equals the faithful one bit for bit and
    glome_rayint_batch in t, prim, n and tex (both_instances); every ray is the oracle's.  Traced a second time, the stream gives the same bits."""
    c = committed(v)
    ro, rd, r, ref = c.deep()
    check_against_oracle(c, "deep", r, ref)
    again = c.sc.trace(ro, rd, c.lights, params=api.trace_params(maxdepth=3), want_hit=True)
    assert same_bits(r, again)


@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_mixed_packets(committed, v):
    """Forward and reverse lanes alternating; one reverse lane at lane 0, 31, 32, 63 -- the ends of the wave and the seam of the two halves of a
    lane mask -- among forward ones; deep lanes between lanes that miss the mesh's bounds; eight deep lanes in the high half of the wave only;
    lanes that start inside the mesh's box all along the comb."""
    c = committed(v)
    ro, rd, what = c.lad.mixed_set()
    r = both_instances(c, ro, rd)
    check_against_oracle(c, "mixed", r, c.oracle_rows(ro, rd))


# ---------------------------------------------------------------- 2. rays AT shared edges and vertices
@pytest.mark.parametrize("v", [VARIANTS[0], VARIANTS[3], VARIANTS[4], VARIANTS[7], VARIANTS[8]], ids=[IDS[0], IDS[3], IDS[4], IDS[7], IDS[8]])
def test_rays_at_shared_edges_and_vertices(committed, v):
    """Rays aimed exactly at the patch's shared vertices and edge middles: which of the triangles that meet there reports the hit depends on the
    order a lane visits the two children of a node in -- what the three passes are for.  Held to the faithful instance and to
    glome_rayint_batch, bit for bit; how many rays differ from the fp64 oracle (hit or miss, or a normal more than 1e-3 away: another triangle)
    is printed, not asserted."""
    c = committed(v)
    ro, rd = c.lad.edges_set()
    assert np.all(rd != 0)
    r = both_instances(c, ro, rd)
    a = c.o.rayint(c.oroot, ro.astype(np.float64), rd.astype(np.float64))
    hit_g, hit_r = r["t"] >= 0, a["t"] >= 0
    other = (hit_g != hit_r) | (hit_g & hit_r & (np.abs(r["n"].astype(np.float64) - a["n"]).max(axis=1) > 1e-3))
    print("mesh_packet_walk_edges_census", c.name, "rays", len(ro), "hits", int(hit_g.sum()), "another triangle than the fp64 oracle's, or a flip:", int(other.sum()))
    assert hit_g.mean() > 0.5


# ---------------------------------------------------------------- 3. tails and order
@pytest.mark.parametrize("v", [VARIANTS[1], VARIANTS[6], VARIANTS[9]], ids=[IDS[1], IDS[6], IDS[9]])
def test_tails_and_order_on_the_mesh_ladder(committed, v):
    """A lane's result depends neither on how many lanes of its wave hold a ray nor on its place in the stream: the first n rays of the deep
    stream (a lone ray, a wave less one, a wave, a wave and one, three waves and 37) give the first n rows of the whole stream's result bit for
    bit, nothing is written past row n, and a seeded permutation of the rays gives the permuted rows."""
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


# ---------------------------------------------------------------- 4. a tmax per lane
@pytest.mark.parametrize("v", [VARIANTS[3], VARIANTS[4], VARIANTS[8]], ids=[IDS[3], IDS[4], IDS[8]])
def test_a_tmax_per_lane(committed, v):
    """The deep stream with a limit of its own on every lane, each case bit for bit the faithful instance's (both_instances): cut before the patch
    -- a miss; cut between two rungs; cut far beyond the last rung -- the uncut rows; tmax exactly a hit's own t -- the faithful instance alone.

    Between two rungs a Mesh does NOT simply drop what lies beyond the cut: a box is entered when its near is within `depth`, and its leaves test
    with the box interval's far (Mesh.hs:163, 198; quirk Q12).  The cut of lane i is the plane at three quarters of rung j_i's place along the
    axis, j_i <= 14: every box face across the axis is a rung's or the patch's, padded by delta, and none of them is nearer to such a plane than
    a tenth of its distance (asserted); so no box straddles a cut, and the oracle's rayint with that tmax -- the primitive, hit or miss -- is
    asserted on every ray whose uncut hit is not near its cut (asserted to be all of them)."""
    c = committed(v)
    lad = c.lad
    ro, rd, base, ref = c.deep()
    n = len(ro)
    u0, du = lad.local(ro)[:, 0], lad.local(rd)[:, 0]
    miss = lambda r, m: np.all(rgbad(r)[m] == MISS) and np.all(r["prim"][m] == -1) and np.all(r["t"][m] == -1)
    # before the patch (the rays start 0.3 .. 0.5 of the nearest rung's place in front of it; the mesh's box begins delta in front of it)
    short = both_instances(c, ro, rd, tmax=((-2.0 * DELTA - u0) / du).astype(np.float32))
    assert miss(short, np.ones(n, bool))
    # between two rungs
    j = np.random.default_rng(5).integers(0, 15, n)
    cut_u = 0.75 * ladder.rung_u(0) / 2.0 ** j
    faces = np.array([f for k in range(ladder.NLEV) for f in (ladder.rung_u(k) - ladder.THICK - DELTA, ladder.rung_u(k) + DELTA)] + [-DELTA, ML.RELIEF + DELTA])
    assert np.all(np.abs(faces[None, :] - cut_u[:, None]) > 0.1 * cut_u[:, None])  # (no cut is anywhere near a box face ...)
    cut = (cut_u - u0) / du
    assert np.all(np.abs(ref["t"] - cut)[ref["t"] >= 0] > 1e-3 * cut[ref["t"] >= 0])  # (... or near its ray's hit)
    mid = both_instances(c, ro, rd, tmax=cut.astype(np.float32))
    a = c.o.rayint(c.oroot, ro.astype(np.float64), rd.astype(np.float64), cut.astype(np.float32).astype(np.float64))
    want = np.where(a["prim"] >= 0, c.sd_of_oracle[a["prim"]], -1)
    assert np.array_equal(np.where(mid["prim"] >= 0, c.sd_of_prod[mid["prim"]], -1), want) and np.array_equal(mid["t"] >= 0, a["t"] >= 0)
    inside = (ref["t"] >= 0) & (ref["t"] < cut)
    assert np.array_equal(inside, a["t"] >= 0) and 0.2 < inside.mean() < 0.8  # (with no box astride a cut, Q12 changes nothing here)
    assert same_bits({k: mid[k][inside] for k in HIT_KEYS}, {k: base[k][inside] for k in HIT_KEYS}) and miss(mid, ~inside)
    # far beyond the last rung
    far = both_instances(c, ro, rd, tmax=np.full(n, 5.0 * ladder.L, np.float32))
    assert same_bits(far, base)
    # exactly the hit's t
    hit = base["t"] >= 0
    both_instances(c, ro[hit], rd[hit], tmax=base["t"][hit])


# ---------------------------------------------------------------- 5. a frame
@pytest.mark.parametrize("v", [VARIANTS[0], VARIANTS[5]], ids=[IDS[0], IDS[5]])
def test_a_frame_along_the_comb(committed, v):
    """glome_render of the mesh ladder from in front of the patch through the ladder's narrow angle, so far back that the small frame spans the
    cross-section: every work item of it pushes and pops beyond the LDS part of the stack and some take three passes there (modelled, and the
    instance k_render_flat<false,false,false,MESH,1,false> asserted, in tests/test_mesh_packet_model.py).  The frame equals the faithful
    instance's bit for bit, out5 and packed, with the same ray counts; between 5 % and 90 % of the pixels hit."""
    c = committed(v)
    w, h = ML.FRAME_W, ML.FRAME_H
    img, packed, st = c.sc.render(c.cam, c.lights, api.render_params(width=w, height=h, maxdepth=3))
    imf, packedf, stf = c.sc.render(c.cam, c.lights, api.render_params(width=w, height=h, maxdepth=3, faithful=1))
    assert np.array_equal(img.view(np.uint32), imf.view(np.uint32)) and np.array_equal(packed, packedf)
    assert [st[k] for k in RAY_KEYS] == [stf[k] for k in RAY_KEYS] and st["rays_primary"] == w * h
    hit = img[..., 4] < 1e6
    print("mesh_packet_walk_frame", c.name, "hit share", hit.mean(), {k: st[k] for k in RAY_KEYS})
    assert 0.05 < hit.mean() < 0.9, hit.mean()
