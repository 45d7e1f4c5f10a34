"""The pair test of the hand-written packet walk since it leaves early (TEST INFRASTRUCTURE, no GPU): GLOME_PKW_PAIR_B1 / _VOTE / _REST and the
two chains of glome_amd/csrc/bih_packet_asm.hpp, restated three ways.

  pair_test32   the arithmetic in fp32, operation for operation in the block's order (fma where the block has one, denormals flushed on the
                way in and on the way out, as the kernels are built), for the two triangles of a pair record and any number of rays: b1, the
                vote's h and its answer, and the chain's accept / reject.  The reciprocal is numpy's correctly rounded one: the tests that hold it
                to tri_test choose divisors whose reciprocal is exact.
  PairWalk      tests/packet_walk_model.py's walk (float64, 64 lanes) with a leaf that is tested pair record by pair record and says of every
                pair test which PATH it takes: left after b1 or run through; which halves keep a lane; which halves some lane hits; whether a kept
                lane then fails its chain.  Everything else is the model's own code.  The vote here is the exact one (0 <= b1 <= 1, a NaN stays);
                the block's keeps b1 in [-2^-25, 0) as well, which no ray of the tests' streams comes near.
  Leaves        a scene whose tree is given as TEXT (glome_sb_load_show), so that its leaves hold exactly 1, 2, 3 and 5 triangles: four
                clusters in planes x = 1, 3, 5, 7, the triangles of a cluster side by side along z with e1 along z -- b1 of a ray is its z within
                the triangle's strip, so a packet aimed at one triangle has b1 out of range for every other one of the leaf -- under a comb of
                three branches on x and nine trimming branches (one empty child each, on all three axes) that make the tree the 12 levels deep
                the hand-written walk is compiled for.  One light far out on the side the triangles face: a shadow ray runs back through the
                leaves in front of its hit, almost along x.  sign = -1 is the mirror image (x -> 8 - x), walked the other way."""
import collections

import numpy as np

import packet_walk_model as PM
from glome_amd import scenes
from glome_amd.scene import SceneDesc
from oracle import np_scene as NS

F = np.float32
FLT_MIN = np.finfo(np.float32).tiny


# ---------------------------------------------------------------- the arithmetic in fp32
def ftz(x):
    x = np.asarray(x, F)
    return np.where(np.abs(x) < FLT_MIN, np.copysign(F(0), x), x).astype(F)


def _mul(a, b):
    return ftz(ftz(a) * ftz(b))


def _add(a, b):
    return ftz(ftz(a) + ftz(b))


def _fma(a, b, c):
    """round(a * b + c) once: the product of two fp32 numbers is exact in float64"""
    return ftz((ftz(a).astype(np.float64) * ftz(b).astype(np.float64) + ftz(c).astype(np.float64)).astype(F))


def vote32(b1):
    """GLOME_PKW_PAIR_VOTE on one half: h = b1 - 0.5; the lane stays unless |h| > 0.5 holds (ordered: a NaN stays)"""
    with np.errstate(invalid="ignore"):
        h = _add(b1, F(-0.5))
        return h, ~(np.abs(h) > F(0.5))


def pair_test32(tri, o, d, far):
    """tri: 3 x 3 (p1, p2, p3) of ONE half (the halves of a pair are independent elements of the packed instructions); o, d: n x 3; far: n.
    Returns a dict of per-ray arrays: b1, h, keep (the vote), accept (the chain: divisor != 0, 0 <= min3(b1, b2, t), max(b1, b1 + b2) <= 1, t <= far), t"""
    tri = np.asarray(tri, F); o = np.asarray(o, F).reshape(-1, 3); d = np.asarray(d, F).reshape(-1, 3)
    far = np.broadcast_to(np.asarray(far, F), (len(o),))
    p1, e1, e2 = tri[0], ftz(tri[1] - tri[0]), ftz(tri[2] - tri[0])  # (the triangle record holds p1, e1, e2)
    ox, oy, oz = o.T; dx, dy, dz = d.T
    with np.errstate(all="ignore"):
        # part one
        Dx, Dy, Dz = _add(ox, -p1[0]), _add(oy, -p1[1]), _add(oz, -p1[2])
        s1y = _fma(dz, e2[0], -_mul(dx, e2[2])); s1x = _fma(dy, e2[2], -_mul(dz, e2[1])); s1z = _fma(dx, e2[1], -_mul(dy, e2[0]))
        div = _fma(s1z, e1[2], _fma(s1x, e1[0], _mul(s1y, e1[1])))
        num = _fma(Dz, s1z, _fma(Dx, s1x, _mul(Dy, s1y)))
        inv = ftz(F(1.0) / ftz(div))
        b1 = _mul(num, inv)
        h, keep = vote32(b1)
        # part two
        nz = div != 0
        s2y = _fma(Dz, e1[0], -_mul(Dx, e1[2])); s2x = _fma(Dy, e1[2], -_mul(Dz, e1[1])); s2z = _fma(Dx, e1[1], -_mul(Dy, e1[0]))
        b2 = _mul(_fma(dz, s2z, _fma(dx, s2x, _mul(dy, s2y))), inv)
        t = _mul(_fma(s2z, e2[2], _fma(s2x, e2[0], _mul(s2y, e2[1]))), inv)
        lo = np.fmin(np.fmin(b1, b2), t)          # v_min3_f32 drops a NaN
        hi = np.fmax(b1, _add(b1, b2))            # v_max_f32 too
        accept = nz & ~(F(0) > lo) & ~(F(1) < hi) & ~(t > far)
    return {"b1": b1, "h": h, "keep": keep, "accept": accept, "t": t, "div": div}


# ---------------------------------------------------------------- the walk, pair test by pair test
Pair = collections.namedtuple("Pair", "leaf_size index left kept hits chain_fail mode")
# leaf_size: triangles in the leaf; index: which pair record of the leaf; left: no lane kept for A or B, the test ends after b1; kept / hits:
# frozensets of "A" / "B" -- the halves with a lane the vote keeps / some lane accepts as a hit (B of a leaf's odd last triangle is A again and
# is not listed); chain_fail: a lane the vote kept for a half then fails that half's chain


def _b1(tr, o, d):
    p1, p2, p3 = (np.asarray(q, np.float64) for q in tr.p)
    e1, e2 = p2 - p1, p3 - p1
    s1 = np.cross(d, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.einsum("ij,ij->i", o - p1, s1) * (1.0 / (s1 @ e1))


class PairWalk(PM._Walk):
    def leaf(self):
        items, hits_all = self.node[1], set()
        for p in range(0, len(items), 2):
            halves = [("A", p)] + ([("B", p + 1)] if p + 1 < len(items) else [])
            am0 = self.am.copy()
            kept, hit_by, fail = {}, {}, False
            for name, k in halves:
                with np.errstate(invalid="ignore"):
                    b1 = _b1(PM._tri(items[k]), self.o, self.d)
                    kept[name] = am0 & ~((b1 < 0) | (b1 > 1))
            left = not any(v.any() for v in kept.values())
            for name, k in halves:  # (the model's own leaf, triangle by triangle)
                tr = PM._tri(items[k])
                at_half = self.am.copy()  # (mode 2: the lanes A occluded are gone when B's chain runs)
                hit, t = PM.tri_hits(tr.p, self.o, self.d, self.far)
                hit &= self.am
                if self.mode == 2:
                    self.occ |= hit; self.prim[hit] = tr.uid; self.am = self.am & ~hit
                    acc = hit
                else:
                    acc = hit & ~(self.best_t < t)
                    self.best_t[:] = np.where(acc, t, self.best_t); self.prim[acc] = tr.uid
                    self.far = np.where(acc & (self.far > t), t, self.far)
                assert not (acc & ~kept[name]).any(), "the vote dropped a lane that hits"
                hit_by[name] = acc
                fail = fail or bool((kept[name] & at_half & ~acc).any())
                if acc.any():
                    hits_all.add(k)
            assert not (left and hits_all & {p, p + 1})
            self.ev.append(Pair(len(items), p // 2, left, frozenset(n for n, v in kept.items() if v.any()), frozenset(n for n, v in hit_by.items() if v.any()), fail and not left, self.mode))
            if self.mode == 2 and not self.am.any():
                break  # (every lane of the leaf is occluded: the block goes to the pops)
        self.ev.append(PM.Leaf(len(items), frozenset(hits_all), self.mode))


def walk(bih, o, d, dist, mode):
    """PM.walk (the production walk: origin clip) with the leaf above"""
    saved = PM._Walk
    PM._Walk = PairWalk
    try:
        return PM.walk(bih, o, d, dist, mode, origin_clip=True)
    finally:
        PM._Walk = saved


def stream(bih, o, d, dist, mode):
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    dist = np.broadcast_to(np.asarray(dist, np.float64), (len(o),))
    return [walk(bih, o[i:i + 64], d[i:i + 64], dist[i:i + 64], mode) for i in range(0, len(o), 64)]


def paths(events):
    """the classes of the issue, of one packet's events: a set of (mode, name)"""
    out = set()
    seen_left_first = {}
    for e in events:
        if not isinstance(e, Pair):
            continue
        m = e.mode
        if e.index == 0:
            seen_left_first[m] = e.left
            if e.left:
                out.add((m, "leave on the first pair of a leaf of %d" % e.leaf_size))
        elif e.index == 1 and seen_left_first.get(m) and e.hits:
            out.add((m, "leave on the first pair and hit on the second"))
        if not e.left:
            out.add((m, {frozenset("A"): "A kept alone", frozenset("B"): "B kept alone", frozenset("AB"): "both kept"}[e.kept]))
            if e.chain_fail:
                out.add((m, "a kept lane fails the chain"))
            if e.leaf_size - 2 * e.index >= 2:
                if e.hits == frozenset("B"):
                    out.add((m, "update skipped on A and taken on B"))
                if e.hits == frozenset("A"):
                    out.add((m, "update taken on A and skipped on B"))
    return out


PATHS = (["leave on the first pair of a leaf of %d" % n for n in (1, 2, 3, 5)] +
         ["leave on the first pair and hit on the second", "A kept alone", "B kept alone", "both kept", "a kept lane fails the chain",
          "update skipped on A and taken on B", "update taken on A and skipped on B"])


# ---------------------------------------------------------------- leaves of exactly 1, 2, 3 and 5 triangles: a tree given as text
SIZES = (1, 2, 3, 5)
LEAF_X = (1.0, 3.0, 5.0, 7.0)
LIGHT = (-100.0, 0.5, 4.5)


def _num(x):
    """a number as Haskell's show prints it (values here are multiples of 1/8 between 1/8 and 100 in size, or 0)"""
    s = repr(float(x))
    assert "e" not in s and (x == 0 or 0.1 <= abs(x) < 1e7)
    return "(%s)" % s if x < 0 else s


def _vec(p):
    return "Vec %s %s %s" % tuple(_num(x) for x in p)


class Leaves:
    mirror = False

    def __init__(self, sign=1):
        self.sign = sign
        X = (lambda x: x) if sign > 0 else (lambda x: 8.0 - x)
        self.tris, self.leaf_of = [], []
        for k, (n, x) in enumerate(zip(SIZES, LEAF_X)):
            for i in range(n):
                z = 2.0 * i
                if sign > 0:   # e1 = +z, e2 = +y: the normal points to -x, where the light is
                    t = ((x, 0.0, z), (x, 0.0, z + 1.0), (x, 1.0, z))
                else:          # mirrored: e1 = +z, e2 = -y from y = 1: the normal points to +x
                    t = ((X(x), 1.0, z), (X(x), 1.0, z + 1.0), (X(x), 0.0, z))
                self.tris.append(t); self.leaf_of.append(k)
        self.first = [int(np.flatnonzero(np.array(self.leaf_of) == k)[0]) for k in range(4)]
        self.light = (X(LIGHT[0]),) + LIGHT[1:]
        # ---- the SceneDesc: what the oracle renders (its own tree over the same triangles) and where lights and materials come from
        sd = self.sd = SceneDesc()
        self.mat = scenes.matte(sd, (0.8, 0.5, 0.4))
        self.tri_ids = [sd.triangle(*t) for t in self.tris]
        self.bih_id = sd.bih([sd.tex(t, self.mat) for t in self.tri_ids])
        sd.set_root(self.bih_id)
        sd.add_light(self.light, (9000.0, 9000.0, 9000.0))
        sd.set_camera((X(-6.0), 0.6, 4.3), (X(7.0), 0.45, 4.4), (0.0, 1.0, 0.0), 22.0)
        # ---- the tree: as text for the product, as np_scene nodes for the model
        solids = []
        for u, t in enumerate(self.tris):
            s = NS.Tex(NS.Triangle(*t), None); s.s.uid = u
            solids.append(s)
        leaf = lambda k: ("leaf", [solids[self.first[k] + i] for i in range(SIZES[k])])
        node = leaf(3)
        # nine trimming branches above the leaf of five, innermost first: (axis, plane, which side is empty) -- x planes in ladder coordinates
        trims = [(1, -0.5, "L"), (2, 9.5, "R"), (0, 6.5, "L"), (1, 1.5, "R"), (2, -0.5, "L"), (0, 7.5, "R"), (1, -0.25, "L"), (2, 9.25, "R"), (1, 1.25, "R")]
        for axis, plane, side in trims:
            if axis == 0 and sign < 0:
                plane, side = 8.0 - plane, "R" if side == "L" else "L"
            node = ("branch", plane, plane, axis, ("leaf", []), node) if side == "L" else ("branch", plane, plane, axis, node, ("leaf", []))
        for k, plane in ((2, 6.0), (1, 4.0), (0, 2.0)):  # the comb on x
            node = ("branch", plane, plane, 0, leaf(k), node) if sign > 0 else ("branch", 8.0 - plane, 8.0 - plane, 0, node, leaf(k))
        lo, hi = (0.5, -0.5, -0.5), (7.5, 1.5, 9.5)
        self.bih = collections.namedtuple("TextBih", "bb root")((lo, hi), node)
        assert PM.tree_depth(node) == PM.LDS_CAP
        self.pts_of_uid = {u: np.asarray(t, np.float64) for u, t in enumerate(self.tris)}

        def show(n):
            if n[0] == "leaf":
                return "BihLeaf [%s]" % ",".join("SI Tex SI Triangle (%s) (%s) (%s) Texture" % tuple(_vec(p) for p in PM._tri(s).p) for s in n[1])
            return "BihBranch %s %s %d (%s) (%s)" % (_num(n[1]), _num(n[2]), n[3], show(n[4]), show(n[5]))
        self.text = "SI Bih {bihbb = Bbox {p1 = %s, p2 = %s}, bihroot = %s}" % (_vec(lo), _vec(hi), show(node))

    def load(self, builder):
        """the tree in a product builder: (root node, the builder's item ids in the order of self.tris)"""
        nm, mm = self.sd.replay(builder)  # (for the material; the description's own bih stays unused)
        root, ntex = builder.load_show(self.text, default_material=mm[self.mat])
        assert ntex == len(self.tris)
        items = builder.bih_items(root)  # (in the tree's preorder: the order of the text)
        order = [PM._tri(s).uid for leaf in PM.leaves(self.bih.root) for s in leaf]
        assert len(items) == len(order)
        return root, [items[order.index(u)] for u in range(len(order))]

    # ---- the packets
    def point(self, tri, b1, b2):
        p = np.asarray(self.tris[tri], np.float64)
        return p[0] + b1 * (p[1] - p[0]) + b2 * (p[2] - p[0])

    def streams(self):
        """name -> (o, d), fp32: per octant one packet of 64 lanes of every kind below, every lane aimed at a point given by (triangle, b1, b2) --
        inside a triangle with both coordinates and their sum clear of the edges, or beside one -- from 4 to 9 away along x on either side, tilted
        across x by 2 to 7 hundredths.  A ray may meet another leaf's triangle first: the oracle says what it hits, the model which paths it takes."""
        rng = np.random.default_rng(13 + (self.sign < 0))
        F0 = self.first
        # (every other lane in the half of the triangle beyond the light's height: the shadow rays of a packet run up and run down)
        inside = lambda t: (lambda i: (t, rng.uniform(0.25, 0.4), rng.uniform(0.25, 0.4)) if i % 4 < 2 else (t, rng.uniform(0.15, 0.25), rng.uniform(0.55, 0.65)))
        kinds = {
            "leaf2 A": inside(F0[1]), "leaf2 B": inside(F0[1] + 1), "leaf2 A and B": lambda i: inside(F0[1] + i % 2)(i),
            "leaf3 third": inside(F0[2] + 2), "leaf5 fifth": inside(F0[3] + 4), "leaf5 A": inside(F0[3]), "leaf5 B": inside(F0[3] + 1),
            "leaf5 A and B": lambda i: inside(F0[3] + i % 2)(i), "leaf5 third": inside(F0[3] + 2), "leaf1": inside(F0[0]),
            "beside in z": lambda i: (F0[i % 4], rng.uniform(-0.45, -0.25), rng.uniform(0.25, 0.4)),   # b1 < 0 in every triangle of every leaf
            "beside in y": lambda i: (F0[i % 4] + (i // 4) % SIZES[i % 4], rng.uniform(0.25, 0.4), rng.uniform(1.2, 1.4)),  # b1 in range, b2 > 1
        }
        out = {}
        for name, make in kinds.items():
            os_, ds = [], []
            for octant in range(8):
                s = np.array([1.0 if octant >> a & 1 else -1.0 for a in range(3)])
                for i in range(64):
                    p = self.point(*make(i))
                    v = s * np.array((rng.uniform(4.0, 9.0), 0.0, 0.0))
                    v[1], v[2] = s[1] * abs(v[0]) * rng.uniform(0.02, 0.07), s[2] * abs(v[0]) * rng.uniform(0.02, 0.07)
                    os_.append(p - v); ds.append(v)
            o, d = np.array(os_), np.array(ds)
            d = d / np.linalg.norm(d, axis=1, keepdims=True)
            o32, d32 = o.astype(np.float32), d.astype(np.float32)
            d32 = (d32 / np.linalg.norm(d32.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
            assert np.all(d32 != 0)
            out[name] = (o32, d32)
        return out
