"""The pair test that leaves when no ray passes b1 (GLOME_PKW_PAIR_B1 / _VOTE / _REST, glome_amd/csrc/bih_packet_asm.hpp), without a GPU.

1. tests/pair_exit_model.py's fp32 restatement of the reordered test and its vote is held to tri_test's accept / reject (the device code compiled
   for the host, tests/hostsim) on crafted rays: b1 exactly 0 and exactly 1 (through an edge, through a vertex), one ulp above 1, the smallest
   negative normal, a subnormal that the kernels flush, a zero divisor with a zero numerator (b1 = NaN) and with a non-zero one (b1 = +-inf); as
   the A half of a pair record and as its B half.  The vote never drops a ray tri_test accepts -- on those, and on random rays around a triangle.
   The triangle lies in z = 0 with e1 = x and e2 = y and the crafted rays run down z from height 1, tilted by 2^-10, so b1, b2 and t = 1 are exact,
   and the divisor is 1: its reciprocal is exact on the host, in numpy and in v_rcp_f32 alike.
2. The vote on b1 alone: which fp32 values stay and which go, at every boundary the header's soundness argument names.
3. What the packets of tests/test_pair_exit_gpu.py reach, by tests/pair_exit_model.py's walk: every path through the pair test, in both modes."""
import collections
import ctypes as C

import numpy as np
import pytest

import pair_exit_model as X
import packet_walk_model as PM
import packet_walk_scenes as PS
from helpers import HostSim
from test_trace_choice import export_choice, instance_name
from glome_amd import _lib as L
from glome_amd import api

F = np.float32
T0 = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
OTHER = ((50.0, 50.0, 7.0), (51.0, 50.0, 7.0), (50.0, 51.0, 7.0))  # the other half of the pair record: nowhere near the rays, in another plane
ULP1 = float(np.nextafter(F(1), F(2)))
E = 2.0 ** -10  # the rays' tilt (the host build takes no direction component of +0): b1 = o.x + E, b2 = o.y + E, every operation exact
DOWN, ALONG = (E, E, -1.0), (1.0, E, -0.0)
TINY, SUB = float(X.FLT_MIN), 1e-40


def at(b1, b2):
    return (b1 - E, b2 - E, 1.0)


# name: (origin, direction, tri_test accepts, the vote keeps -- None where it may do either)
CRAFTED = {
    "b1 = 0, through the edge p1 p3": (at(0.0, 0.5), DOWN, True, True),
    "b1 = 0, through the vertex p1": (at(0.0, 0.0), DOWN, True, True),
    "b1 = 1, through the vertex p2": (at(1.0, 0.0), DOWN, True, True),
    "b1 + b2 = 1, through the edge p2 p3": (at(0.5, 0.5), DOWN, True, True),
    "b1 one ulp above 1": (at(ULP1, 0.0), DOWN, False, False),
    # from o.x = 0 with d.x = b1: D . s1 = 0 * 1 + 1 * d.x
    "b1 the smallest negative normal": ((0.0, 0.25 - E, 1.0), (-TINY, E, -1.0), False, None),
    "b1 a positive subnormal": ((0.0, 0.25 - E, 1.0), (SUB, E, -1.0), True, True),
    "b1 a negative subnormal": ((0.0, 0.25 - E, 1.0), (-SUB, E, -1.0), None, True),  # (the kernels flush it to zero and accept; the host build keeps it and rejects)
    "zero divisor, zero numerator": ((-1.0, 0.5, 0.0), ALONG, False, True),   # in the triangle's plane: b1 = 0 * inf = NaN stays in the vote, the chain's divisor test rejects
    "zero divisor, non-zero numerator": ((-1.0, 0.5, 1.0), ALONG, False, False),  # parallel to it, 1 above: b1 = 1 * inf
}


@pytest.fixture(scope="module")
def leaves_of_two(built):
    """two one-leaf trees: T0 as the A half of its pair record, and as the B half"""
    out = {}
    for half, tris in (("A", (T0, OTHER)), ("B", (OTHER, T0))):
        b = api.Builder()
        m = b.material_surface((1, 1, 1), 1, 0.2, 0.8, 0, 0)
        root = b.bih([b.tex(b.triangle(*t), m) for t in tris])
        out[half] = HostSim(b, root)
    return out


@pytest.mark.parametrize("half", ["A", "B"])
def test_crafted_rays_against_tri_test(leaves_of_two, half):
    hs = leaves_of_two[half]
    o = np.array([c[0] for c in CRAFTED.values()], F); d = np.array([c[1] for c in CRAFTED.values()], F)
    host = hs.rayint(o, d, 1e6, analysis=1)["t"] >= 0  # (the faithful per-ray code: tri_test on every triangle of the leaf)
    assert np.array_equal(host, hs.rayint(o, d, 1e6)["t"] >= 0)
    m = X.pair_test32(T0, o, d, 1e6)
    other = X.pair_test32(OTHER, o, d, 1e6)
    assert not other["accept"].any() and not other["keep"].any()  # the other half never keeps the pair alive: what is seen is T0's vote
    for k, (name, (_, _, accepts, keeps)) in enumerate(CRAFTED.items()):
        print(half, name, "b1", m["b1"][k], "h", m["h"][k], "keep", bool(m["keep"][k]), "model", bool(m["accept"][k]), "tri_test", bool(host[k]))
        if accepts is not None:
            assert bool(host[k]) == accepts and bool(m["accept"][k]) == accepts, name
        if keeps is not None:
            assert bool(m["keep"][k]) == keeps, name
        assert m["keep"][k] or not (host[k] or m["accept"][k]), name  # never drops what is accepted
    assert np.isnan(m["b1"][list(CRAFTED).index("zero divisor, zero numerator")]) and np.isinf(m["b1"][list(CRAFTED).index("zero divisor, non-zero numerator")])
    b1 = dict(zip(CRAFTED, m["b1"]))
    assert b1["b1 a negative subnormal"] == 0 and b1["b1 a positive subnormal"] == 0 and b1["b1 the smallest negative normal"] == -F(TINY)
    assert b1["b1 one ulp above 1"] == F(ULP1) and b1["b1 = 1, through the vertex p2"] == 1 and b1["b1 = 0, through the vertex p1"] == 0


@pytest.mark.parametrize("half", ["A", "B"])
def test_the_vote_never_drops_a_ray_tri_test_accepts(leaves_of_two, half):
    """20,000 rays at points in and closely around T0 -- a third of them aimed exactly at the line b1 = 0 or b1 = 1 -- from origins all around it"""
    rng = np.random.default_rng(5)
    n = 20000
    b1 = rng.uniform(-0.2, 1.2, n); b2 = rng.uniform(-0.2, 1.2, n)
    k = np.arange(n) % 6
    b1 = np.where(k == 0, 0.0, np.where(k == 1, 1.0, b1)); b2 = np.where(k == 2, 0.0, b2)
    p = np.stack([b1, b2, np.zeros(n)], 1).astype(F)
    o = (p + rng.uniform(-3, 3, (n, 3)) * np.array((1.0, 1.0, 2.0))).astype(F)
    d = (p - o).astype(F)
    host = leaves_of_two[half].rayint(o, d, 1e6, analysis=1)["t"] >= 0
    m = X.pair_test32(T0, o, d, 1e6)
    # the host build has no fma, the kernels and the model have: on a ray aimed exactly at the line b1 = 0 or b1 = 1 the two round b1 to
    # different sides.  The vote and the chain of the kernel read the SAME b1, so the model's vote is held to the model's chain on every ray,
    # and to the host's tri_test on the rays whose exact b1 is 1e-6 or more away from both lines
    tri = collections.namedtuple("T", "p")(T0)
    exact = X._b1(tri, o.astype(np.float64), d.astype(np.float64))
    clear = (np.abs(exact) > 1e-6) & (np.abs(exact - 1) > 1e-6)
    print("accepted by tri_test:", int(host.sum()), "by the model's chain:", int(m["accept"].sum()), "kept by the vote:", int(m["keep"].sum()), "of", n, "; on a line:", int((~clear).sum()))
    assert 3000 < host.sum() < 12000 and m["keep"].sum() < 0.9 * n and (~clear).sum() > n // 4  # not vacuous: many rays are accepted, the vote drops rays, many lie on a line
    assert not (m["accept"] & ~m["keep"]).any()
    assert not (host & ~m["keep"] & clear).any()


def test_the_vote_on_b1_alone():
    one, half = F(1), F(0.5)
    keep = lambda v: X.vote32(np.asarray(v, F))[1]
    up = lambda x: np.nextafter(F(x), F(np.inf)); dn = lambda x: np.nextafter(F(x), F(-np.inf))
    stays = [0.0, -0.0, X.FLT_MIN, 1e-40, -1e-40, dn(0.25), 0.25, up(0.25), dn(half), half, up(half), dn(one), one, np.nan, -F(2.0) ** -25, -X.FLT_MIN]
    goes = [up(one), 1.5, 2.0, 3e38, np.inf, up(-F(2.0) ** -24), -F(2.0) ** -24, -0.25, -1.0, -3e38, -np.inf]
    assert keep(stays).all(), np.asarray(stays)[~keep(stays)]
    assert not keep(goes).any(), np.asarray(goes)[keep(goes)]
    # every fp32 number of [0, 1] in a sample of two million, and the whole binades at both ends
    rng = np.random.default_rng(1)
    bits = rng.integers(0, int(one.view(np.uint32)) + 1, 2_000_000, dtype=np.uint32)
    assert keep(bits.view(F)).all()
    top = np.arange(int(half.view(np.uint32)), int(one.view(np.uint32)) + 1, dtype=np.uint32).view(F)
    h, k = X.vote32(top)
    assert k.all() and np.array_equal(h.astype(np.float64), top.astype(np.float64) - 0.5)  # exact there (Sterbenz)
    low = np.arange(int(F(X.FLT_MIN).view(np.uint32)), int(F(X.FLT_MIN).view(np.uint32)) + (1 << 23), dtype=np.uint32).view(F)
    h, k = X.vote32(low)
    assert k.all() and np.all(h == F(-0.5))


# ---------------------------------------------------------------- what the GPU test's packets reach
def _scenes():
    lat = PS.Lattice()
    f = PS.Field()
    from oracle import np_scene as NS
    sc, nm = NS.load(f.sd)
    return [("leaves +", X.Leaves(1), None), ("leaves -", X.Leaves(-1), None), ("lattice", PS.with_uids(lat, lat.bih), lat.bih),
            ("field", PS.with_uids(f, sc.nodes[nm[f.bih_id]]), sc.nodes[nm[f.bih_id]])]


@pytest.fixture(scope="module")
def reached():
    """scene name -> Counter of (mode, path) over the packets of every stream and of the shadow packets the product makes of them; and the
    octants of the walks of the two text trees per mode.  Walked once, shared."""
    out, octants = {}, {1: set(), 2: set()}
    for name, s, bih in _scenes():
        bih = bih or s.bih
        got = collections.Counter()
        for _, (ro, rd) in s.streams().items():
            res = X.stream(bih, ro, rd, 1e6, 1)
            shadow = [r for so, sdv, sl in PS.shadow_stream(s, ro, rd, res) for r in X.stream(bih, so, sdv, sl, 2)]
            for r in res + shadow:
                got.update(X.paths(r["events"]))
                if name.startswith("leaves"):
                    for w in r["walks"]:
                        octants[w[3][0].mode].add(w[0])
        out[name] = got
    return out, octants


def test_the_text_trees_hold_what_they_say_and_reach_the_hand_written_walk(built):
    lib = L.load()
    for sign in (1, -1):
        lv = X.Leaves(sign)
        assert sorted(len(x) for x in PM.leaves(lv.bih.root) if x) == [1, 2, 3, 5]
        b = api.Builder()
        root, items = lv.load(b)
        assert b.show(root) == lv.text and len(items) == 11
        t = np.zeros(11, dtype=np.int64)
        assert lib.glome_sb_scene_traits(b.h, root, t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        tier, cls_mask, sec, nested, refract, pk_all, stack_cap = (int(x) for x in t[:7])
        assert (tier, pk_all, stack_cap, cls_mask) == (0, 1, PM.LDS_CAP, 1)
        assert instance_name(int(export_choice(lib, [list(t[:8]) + [0, 0, 3]])[0, 0])) == "k_trace_batch_flat<false,false,false,TRI,1>"
        # the model's tree is the product's: the host build of the device code gives the model's hit or miss on every ray of every stream
        hs = HostSim(b, root)
        for name, (ro, rd) in lv.streams().items():
            prim = np.concatenate([r["prim"] for r in X.stream(lv.bih, ro, rd, 1e6, 1)])
            got = hs.rayint(ro, rd)
            assert np.array_equal(prim >= 0, got["t"] >= 0), name
            want = np.where(prim >= 0, np.asarray(items)[np.maximum(prim, 0)] - 1, -1)  # (a hit names the Triangle inside its Tex: the node made just before it)
            assert np.array_equal(got["prim"], want), name


@pytest.mark.parametrize("mode", [1, 2])
def test_the_packets_reach_every_path(reached, mode):
    got, octants = reached
    for name, c in got.items():
        print(name, "mode", mode, {p: c[(mode, p)] for p in X.PATHS})
    for sign in ("leaves +", "leaves -"):  # each text tree alone reaches every path
        assert all(got[sign][(mode, p)] > 0 for p in X.PATHS), [p for p in X.PATHS if not got[sign][(mode, p)]]
    assert octants[mode] == set(range(8)), octants[mode]
    # the lattice and the heightfield add leaves of one and two triangles in trees the builder made; what they reach is printed above
    every = sum(got.values(), collections.Counter())
    assert all(every[(mode, p)] > 0 for p in X.PATHS)
    assert sum(got["lattice"][(mode, p)] + got["field"][(mode, p)] for p in X.PATHS[:2]) > 0  # (they do leave early)
