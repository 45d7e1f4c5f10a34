"""The "ladder": an adversarial triangle BIH for the packet walk, and the ray packets aimed at it (TEST INFRASTRUCTURE;
tests/test_packet_model.py states what they reach, tests/test_packet_walk_edges.py traces them on the GPU).

Along its axis u the ladder has a HEAVY end at 0 and a far end at L = 250.  A "screen" triangle stands at 0, rungs stand at
u_j = 0.75 L / 2^j, j = 0 .. NLEV - 1 (a rung is THICK deep and ends at u_j): build_rec (Bih.hs:211-285) splits a box at its middle, so
every level of the tree peels the one rung of the far half off to the right and keeps the rest on the left -- a comb of NLEV - 2 = 16
branches on u with a leaf per rung (the last leaf holds the screen and the two nearest rungs; a cluster's leaf hangs under a few more
branches that trim its box, each with one empty child).  A ray that travels from the heavy end towards the far end enters the left
(near) child at every level and leaves the right one pending: 16 stack entries by the time it reaches the bottom, four of them beyond
the 12 the LDS part of the stack holds.  The same ray travelling the other way holds one.

The cross-section is the square |v|, |w| <= W = 0.001, of the size of the smallest rung spacing (a wider one and the builder starts to
split across the axis at the heavy end).  A rung covers a rectangle of it, centred 0.45 W off the axis at an angle that turns by the
golden angle from rung to rung, so the rays of a packet first meet many different rungs, and the corners of the square and the axis
meet none.  A rung is a CLUSTER of k triangles that share one bounding box exactly (each touches its six faces), so that no split
separates them and their leaf holds k items: k = 1 .. 9 and 13 occur (the six far rungs, 6 to 190 along the axis, are single
triangles: that far away fp32 cannot tell the members of a cluster apart).  Some clusters hold EXACT DUPLICATES, at the front of the
leaf or at its end: ties inside a leaf.  The light sits on the axis beyond the far end, so shadow rays that leave the screen run the
whole comb; some meet a rung, some do not.  The materials are matte.

Ladder(axis, sign) puts u on x, y or z, pointing towards + or - (the mirrored copy): with the signs of the rays' small tilts across the
axis that gives packets of all eight octants over combs split on each of the three axes.  Ladder(mirror=True) gives the rungs a
Reflect material: secondary rays re-enter the walk from inside the comb.

The rays are drawn in float64 from seeded generators and kept only when plain geometry (Ladder.clear: every ray against every triangle,
nothing of the code under test) finds them WELL CLEAR of every edge -- the ray itself, the shadow ray that leaves its hit, a mirror's
reflected ray and what follows it -- so that hit or miss and the primitive are decided by margins fp32 cannot blur.  No ray is
degenerate: every direction has three non-zero components, and no origin lies on a split plane."""
import math

import numpy as np

from glome_amd import scenes
from glome_amd.scene import SceneDesc

L = 250.0
NLEV = 18
W = 0.001
THICK = 0.5 * W       # a rung's extent along the axis (the members of a cluster differ by fractions of it: enough for fp32 to tell them apart 12 away)
RUNG_OFF, RUNG_HALF = 0.45, 0.24  # a rung's rectangle: its centre's distance from the axis and its half-width, in units of W
LIGHT_U = 275.0
CLUSTER = [1, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 3, 1, 1]  # triangles per rung, far end first
DUPLICATES = {7: 2, 9: 3, 11: 7, 14: 4, 15: 3}                     # rung -> how many of its triangles are one and the same triangle ...
DUP_AT_END = {9, 14}                                               # ... the leaf's first ones, or (these rungs) its last ones
GOLDEN = math.pi * (3.0 - math.sqrt(5.0))
FRAME_ANGLE, FRAME_W, FRAME_H = 0.003, 100, 76  # the frame of the GPU suite: 8 x 8 pixel blocks, ragged at two edges
COMB_DEPTH = NLEV - 2  # stack entries a ray holds that runs the comb from the heavy end


def rung_u(j):
    return 0.75 * L / 2 ** j


def rung_rect(j):
    """(v0, v1, w0, w1) of rung j's rectangle in the cross-section: inside |v|, |w| <= 0.7 W"""
    a = j * GOLDEN
    cv, cw = RUNG_OFF * W * math.cos(a), RUNG_OFF * W * math.sin(a)
    return cv - RUNG_HALF * W, cv + RUNG_HALF * W, cw - RUNG_HALF * W, cw + RUNG_HALF * W


def rung_triangles(j, k=None, ndup=None, dup_at_end=None):
    """the cluster of rung j in ladder coordinates: k triangles (P1, P2_i, P3_i) that each touch the six faces of the box
    [u - THICK, u] x [v0, v1] x [w0, w1] -- P1 its low corner, P2_i on the far face's v1 edge, P3_i on the w1 face -- facing the far end.
    k, ndup, dup_at_end: the ladder's own tables (CLUSTER, DUPLICATES, DUP_AT_END) unless given (tests/mesh_ladder.py has its own)"""
    k, u = CLUSTER[j] if k is None else k, rung_u(j)
    v0, v1, w0, w1 = rung_rect(j)
    ndup = DUPLICATES.get(j, 1) if ndup is None else ndup
    dup_at_end = j in DUP_AT_END if dup_at_end is None else dup_at_end
    tris = []
    for i in range(k):
        m = min(i, k - ndup) if dup_at_end else max(0, i - (ndup - 1))  # which member of the cluster triangle i is
        a, b, c = 0.27 * (m % 3), 0.05 + 0.22 * (m % 5), 0.13 * (m % 4)
        tris.append(((u - THICK, v0, w0), (u, v1, w0 + a * (w1 - w0)), (u - (1 - b) * THICK, v0 + c * (v1 - v0), w1)))
    return tris


def to_world(p, axis, sign):
    """ladder coordinates (u, v, w) -> world: u on `axis` (times sign), v and w on the two axes that follow it"""
    q = [0.0, 0.0, 0.0]
    q[axis], q[(axis + 1) % 3], q[(axis + 2) % 3] = sign * p[0], p[1], p[2]
    return tuple(q)


def _f32_rays(o, d):
    """rounded to fp32 and renormalised, as helpers.random_rays does"""
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = o.astype(np.float32); d = d.astype(np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    assert np.all(d != 0)
    return o, d


class Ladder:
    """sd: the SceneDesc; rung_ids[j]: the SceneDesc ids of rung j's triangles (the Triangle nodes inside their Tex); screen_id; bih_id"""

    def __init__(self, axis=0, sign=1, mirror=False):
        self.axis, self.sign, self.mirror = axis, sign, mirror
        sd = self.sd = SceneDesc()
        # (only the materials it uses: an unused Reflect would send the plain ladder to the FULL instance)
        m_screen = scenes.matte(sd, (0.8, 0.5, 0.4))
        # (matte: a ray that runs the comb looks almost straight at the light, and Blinn's half vector of two opposite directions is all rounding)
        m_rung = sd.material_reflect(0.8) if mirror else scenes.matte(sd, (1, 1, 1))  # TestScene.hs:243, 236-237
        m_rung2 = m_rung if mirror else scenes.matte(sd, (1, 0, 0))
        items = []
        self.rung_ids, self.tri_pts = [], {}
        for j in range(NLEV):
            ids = []
            for i, t in enumerate(rung_triangles(j)):
                ids.append(self._triangle(t))
                items.append(sd.tex(ids[-1], m_rung if (j + i) % 2 == 0 else m_rung2))
            self.rung_ids.append(ids)
        # the screen: one triangle over the whole cross-section, its normal towards the light
        self.screen_id = self._triangle(((0.0, -3.2 * W, -1.6 * W), (0.0, 3.2 * W, -1.6 * W), (0.0, 0.0, 3.2 * W)))
        items.append(sd.tex(self.screen_id, m_screen))
        self.bih_id = sd.bih(items)
        sd.set_root(self.bih_id)
        sd.add_light(to_world((LIGHT_U, 0.0, 0.0), axis, sign), (4.0e5 * (L / 1000.0) ** 2, 3.6e5 * (L / 1000.0) ** 2, 3.2e5 * (L / 1000.0) ** 2))
        # the frame's camera: on the axis between the screen and the nearest rung, looking along the ladder through an angle so narrow that the
        # frame's rays stay inside the comb to its far end (FRAME_ANGLE degrees), aimed a hair off the axis so that no ray is parallel to it
        up = [0.0, 0.0, 0.0]; up[(axis + 1) % 3] = 1.0
        sd.set_camera(to_world((0.4 * rung_u(NLEV - 1), 0.0, 0.0), axis, sign), to_world((L, 0.7e-6 * L, 0.4e-6 * L), axis, sign), tuple(up), FRAME_ANGLE)
        self.rung_of = {t: j for j, ids in enumerate(self.rung_ids) for t in ids}
        self.targets = [t for j in range(NLEV) for t in self.rung_ids[j]]  # every rung triangle, far end first
        self.tri_ids = self.targets + [self.screen_id]
        P = np.stack([self.tri_pts[t] for t in self.tri_ids]).reshape(len(self.tri_ids), 9)
        self.same_as = np.all(P[:, None, :] == P[None, :, :], axis=2)  # exact duplicates

    def _triangle(self, t):
        pts = [to_world(p, self.axis, self.sign) for p in t]
        if self.sign < 0:
            pts = [pts[0], pts[2], pts[1]]  # (a mirror image turns the winding: turned back, the triangle keeps facing the light)
        tid = self.sd.triangle(*pts)
        self.tri_pts[tid] = np.asarray(self.sd.ops[-1][2], np.float64)  # (as rounded to fp32)
        return tid

    def world(self, p):
        p = np.asarray(p, np.float64).reshape(-1, 3)
        q = np.zeros_like(p)
        q[:, self.axis], q[:, (self.axis + 1) % 3], q[:, (self.axis + 2) % 3] = self.sign * p[:, 0], p[:, 1], p[:, 2]
        return q

    def local(self, q):
        q = np.asarray(q, np.float64).reshape(-1, 3)
        return np.stack([self.sign * q[:, self.axis], q[:, (self.axis + 1) % 3], q[:, (self.axis + 2) % 3]], 1)

    def octant(self, su, sv, sw):
        """the walk's octant number (bit k: the rays run towards +axis k) of ladder-coordinate direction signs"""
        return ((1 << self.axis) if su * self.sign > 0 else 0) | ((1 << (self.axis + 1) % 3) if sv > 0 else 0) | ((1 << (self.axis + 2) % 3) if sw > 0 else 0)

    # ---- is a ray well clear of every edge?  (plain geometry in float64; nothing of the code under test)
    def _all_hits(self, o, d):
        """Triangle.hs:45-73 without its cut-offs, every ray against every triangle: b1, b2, t as (rays x triangles)"""
        P = np.stack([self.tri_pts[t] for t in self.tri_ids])
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        s1 = np.cross(d[:, None, :], e2[None])
        inv = 1.0 / np.einsum("rtk,tk->rt", s1, e1)
        dd = o[:, None, :] - P[None, :, 0]
        b1 = np.einsum("rtk,rtk->rt", dd, s1) * inv
        s2 = np.cross(dd, e1[None])
        b2 = np.einsum("rk,rtk->rt", d, s2) * inv
        return b1, b2, np.einsum("tk,rtk->rt", e2, s2) * inv

    def clear(self, o, d, limit=None, any_hit=False, margin=0.03):
        """per ray (float64, world): it meets no triangle within `margin` (in barycentric units) of an edge before what it hits, and the nearest hit
        is nearer than every other (exact duplicates apart) by more than fp32 can blur.  any_hit (a shadow ray as far as `limit`): it meets a
        triangle well inside, or comes near none.  Also returns the nearest hit: triangle index (-1: none) and distance."""
        b1, b2, t = self._all_hits(o, d)
        lim = np.full(len(o), 1e6) if limit is None else np.asarray(limit, np.float64)
        ahead = (t > 0) & (t < lim[:, None])
        inside = ahead & (b1 > margin) & (b2 > margin) & (b1 + b2 < 1 - margin)
        near = ahead & (b1 > -margin) & (b2 > -margin) & (b1 + b2 < 1 + margin) & ~inside
        tin = np.where(inside, t, np.inf)
        k = tin.argmin(axis=1)
        tbest = tin[np.arange(len(o)), k]
        if any_hit:
            return np.isfinite(tbest) | ~near.any(axis=1), np.where(np.isfinite(tbest), k, -1), tbest
        gap = 2e-6 * np.maximum(1.0, np.where(np.isfinite(tbest), tbest, 1.0))
        same = self.same_as[k]  # (rays x triangles): the triangles that ARE triangle k
        rival = inside & ~same & (t < (tbest + gap)[:, None])
        graze = near & (t < (tbest + gap)[:, None])
        return ~(rival.any(axis=1) | graze.any(axis=1)), np.where(np.isfinite(tbest), k, -1), tbest

    def clear_with_shadow(self, o32, d32, depth=3):
        """the rays as traced (fp32 values): clear themselves, and so are the rays that leave their hit -- the shadow ray of a hit on a Surface
        material (Shader.hs:65-80), the reflected ray of a hit on a mirror (Shader.hs:124-131) and what follows it, `depth` levels in all"""
        return self._clear_chain(o32.astype(np.float64), d32.astype(np.float64), depth)

    def _clear_chain(self, o, d, depth):
        ok, k, t = self.clear(o, d)
        hit = k >= 0
        if not hit.any():
            return ok
        P = np.stack([self.tri_pts[i] for i in self.tri_ids])[k[hit]]
        nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        pos = o[hit] + t[hit][:, None] * d[hit]
        mirror = (k[hit] != len(self.tri_ids) - 1) if self.mirror else np.zeros(len(pos), bool)
        lv = np.array(self.sd.lights[0][0]) - pos
        ll = np.linalg.norm(lv, axis=1)
        lit = np.einsum("ij,ij->i", lv, nrm) >= 0
        sok = self.clear(pos + 1e-4 * nrm, lv / ll[:, None], ll - 2e-4, any_hit=True)[0] | ~lit | mirror
        if mirror.any() and depth > 1:
            dm = d[hit][mirror]
            out = dm - 2.0 * np.einsum("ij,ij->i", dm, nrm[mirror])[:, None] * nrm[mirror]
            sok[mirror] &= self._clear_chain(pos[mirror] + 1e-4 * out, out, depth - 1)
        ok[np.flatnonzero(hit)] &= sok
        return ok

    # ---- ray generators: ladder coordinates in float64, then world, then fp32.  A lane is drawn again until it is clear of every edge.
    def _draw(self, n, seed, one):
        rng = np.random.default_rng(seed)
        o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
        todo = np.arange(n)
        for _ in range(200):
            if not len(todo):
                return o, d
            od = np.array([one(i, rng) for i in todo])
            oo, dd = _f32_rays(self.world(od[:, 0]), self.world(od[:, 1] - od[:, 0]))
            ok = self.clear_with_shadow(oo, dd)
            o[todo[ok]], d[todo[ok]] = oo[ok], dd[ok]
            todo = todo[~ok]
        raise AssertionError("no clear ray found for lanes %s" % todo)

    def deep_lanes(self, sv, sw, n, first, seed):
        """n rays that run the comb from the heavy end with tilt signs (sv, sw) across the axis: from the corner of the cross-section opposite
        to (sv, sw), between the screen and the nearest rung, each at an interior point of a rung triangle -- the triangles in turn, starting with
        number `first` -- and every 13th well clear of every rung (it stays in the corner, which no rung covers)."""
        def one(i, rng):
            o = np.array((rung_u(NLEV - 1) * rng.uniform(0.3, 0.5), -sv * W * rng.uniform(0.86, 0.9), -sw * W * rng.uniform(0.86, 0.9)))
            if (first + i) % 13 == 5:
                return o, np.array((1.5 * L, o[1] + sv * W * rng.uniform(0.002, 0.008), o[2] + sw * W * rng.uniform(0.002, 0.008)))
            b1 = rng.uniform(0.15, 0.55); b2 = rng.uniform(0.15, 0.85 - b1)
            p = self.local(self.tri_pts[self.targets[(first + i) % len(self.targets)]])
            return o, p[0] + b1 * (p[1] - p[0]) + b2 * (p[2] - p[0])
        return self._draw(n, seed, one)

    def reverse_lanes(self, sv, sw, n, first, seed):
        """n rays that run towards the heavy end (the shallow direction: one pending entry), at the back of rungs 2 .. 5 (single triangles 6 to
        47 along the axis, met from a third as far again: where delta, which lifts the shadow ray off the hit, is many ulps)"""
        def one(i, rng):
            if self.mirror:  # (these come from beyond the far end, stay in the corner and end on the screen)
                o = np.array((rng.uniform(1.2 * L, 1.3 * L), -sv * W * rng.uniform(0.86, 0.9), -sw * W * rng.uniform(0.86, 0.9)))
                return o, np.array((0.0, o[1] + sv * W * rng.uniform(0.002, 0.008), o[2] + sw * W * rng.uniform(0.002, 0.008)))
            j = 2 + (first + i) % 4
            o = np.array((rung_u(j) * rng.uniform(1.25, 1.4), -sv * W * rng.uniform(0.86, 0.9), -sw * W * rng.uniform(0.86, 0.9)))
            b1 = rng.uniform(0.2, 0.4); b2 = rng.uniform(0.2, 0.4)
            p = self.local(self.tri_pts[self.rung_ids[j][0]])
            return o, p[0] + b1 * (p[1] - p[0]) + b2 * (p[2] - p[0])
        return self._draw(n, seed, one)

    def outside_lanes(self, sv, sw, n, seed):
        """n rays that miss the tree's bounds: they start beside the ladder and leave it"""
        def one(i, rng):
            o = np.array((rng.uniform(0.5, 8.0), sv * rng.uniform(1.0, 2.0), sw * rng.uniform(1.0, 2.0)))
            return o, o + np.array((1.0, sv * rng.uniform(0.05, 0.1), sw * rng.uniform(0.05, 0.1)))
        return self._draw(n, seed, one)

    def screen_lanes(self, quadrants, seed):
        """one ray per entry (qv, qw) of `quadrants`: from behind the screen at a point of its quadrant (qv, qw) of the cross-section.  The shadow
        ray of that hit leaves the screen towards the light on the axis -- tilt signs (-qv, -qw) -- and runs the whole comb."""
        def one(i, rng):
            qv, qw = quadrants[i]
            s = np.array((0.0, qv * W * rng.uniform(0.05, 0.8), qw * W * rng.uniform(0.05, 0.8)))
            d = np.array((1.0, -qv * rng.uniform(1e-4, 3e-4), -qw * rng.uniform(1e-4, 3e-4)))
            return s - 0.003 * L * d, s
        return self._draw(len(quadrants), seed, one)

    # ---- the streams the tests share (64 consecutive rays are one packet)
    def deep_set(self):
        """two packets per tilt-sign pair: every rung triangle is aimed at in each pair.  Returns o, d and per packet its (sv, sw)."""
        os_, ds, tilt = [], [], []
        for k, (sv, sw) in enumerate([(1, 1), (-1, 1), (1, -1), (-1, -1)]):
            for half in range(2):
                o, d = self.deep_lanes(sv, sw, 64, 64 * half + 5 * k, 100 + 10 * k + half)
                os_.append(o); ds.append(d); tilt.append((sv, sw))
        return np.concatenate(os_), np.concatenate(ds), tilt

    def shadow_set(self):
        """primary rays at the screen whose shadow rays form deep packets: one packet per quadrant, then one of two, one of four"""
        quads = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
        lanes = []
        for q in quads:
            lanes += [q] * 64
        lanes += [quads[i % 2] for i in range(64)] + [quads[i % 4] for i in range(64)]
        o, d = self.screen_lanes(lanes, 7)
        return o, d, lanes

    def mixed_set(self):
        """packets composed lane by lane.  Returns o, d and a description per packet."""
        T = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
        packets, what = [], []

        def compose(parts, name):
            """parts: per lane (kind, sv, sw)"""
            o = np.zeros((64, 3), np.float32); d = np.zeros((64, 3), np.float32)
            groups = {}
            for lane, key in enumerate(parts):
                groups.setdefault(key, []).append(lane)
            for g, (key, lanes) in enumerate(sorted(groups.items())):
                kind, sv, sw = key
                seed = 1000 + 97 * len(packets) + g
                if kind == "deep": oo, dd = self.deep_lanes(sv, sw, len(lanes), 7 * len(packets) + g, seed)
                elif kind == "far": oo, dd = self.deep_lanes(sv, sw, len(lanes), len(packets) % 3, seed)  # at the far rungs: each lane alone holds the whole comb pending
                elif kind == "rev": oo, dd = self.reverse_lanes(sv, sw, len(lanes), 7 * len(packets) + g, seed)
                else: oo, dd = self.outside_lanes(sv, sw, len(lanes), seed)
                o[lanes], d[lanes] = oo, dd
            packets.append((o, d)); what.append(name)

        compose([("deep",) + T[i % 2] for i in range(64)], "2 octants, alternating lanes")
        compose([("deep",) + T[(i // 16) % 4] for i in range(64)], "4 octants, 16 lanes each")
        compose([("deep",) + T[i % 4] if i % 8 < 4 else ("rev",) + T[i % 4] for i in range(64)], "8 octants")
        compose([("deep",) + T[(i * 7 // 3) % 4] if i % 3 else ("rev",) + T[(i // 3) % 4] for i in range(64)], "8 octants, uneven")
        for lane in (0, 31, 32, 63):  # an octant held by one lane: at the ends of the wave and on the seam of the two mask halves
            compose([("far", -1, 1) if i == lane else ("deep", 1, 1) for i in range(64)], "single lane %d" % lane)
        compose([("far", 1, -1) if i in (0, 31, 32, 63) else ("rev", -1, -1) for i in range(64)], "four single deep lanes among shallow ones")
        compose([("deep", 1, 1) if i % 2 else ("out", 1, 1) for i in range(64)], "deep lanes between lanes that miss the bounds")
        compose([("deep",) + T[i % 4] if i % 3 == 0 else ("out",) + T[(i + 1) % 4] for i in range(64)], "4 octants between lanes that miss the bounds")
        compose([("deep", -1, -1) if 32 <= i < 40 else ("out", -1, 1) for i in range(64)], "eight deep lanes in the high half only")
        return np.concatenate([p[0] for p in packets]), np.concatenate([p[1] for p in packets]), what


def shadow_rays(lad, o, d, t):
    """mpreshade's shadow rays (Shader.hs:65-80) of primary rays that hit the screen at distance t: from the hit point, lifted off the
    screen by delta along its normal, towards the light, as far as the light less two deltas"""
    p = np.asarray(o, np.float64) + np.asarray(t, np.float64)[:, None] * np.asarray(d, np.float64)
    nrm = np.array(to_world((1.0, 0.0, 0.0), lad.axis, lad.sign))
    lv = np.array(lad.sd.lights[0][0]) - p
    ll = np.linalg.norm(lv, axis=1)
    return p + 1e-4 * nrm, lv / ll[:, None], ll - 2e-4


def oracle_trace(o, ro, rd, maxdepth):
    """(n x 5 (r, g, b, a, depth), ray counts) from the oracle: one 1 x 1 frame per ray, whose camera (pos = o, fwd = d, up = right = 0) traces
    exactly `Ray o (vnorm d)` to infinity with the scene's lights (tests/test_trace_batch.py)"""
    out = np.zeros((len(ro), 5))
    counts = {"rays_primary": 0, "rays_shadow": 0, "rays_secondary": 0}
    for i in range(len(ro)):
        o.set_camera_vectors(ro[i].astype(np.float64), rd[i].astype(np.float64), [0, 0, 0], [0, 0, 0])
        img, _, rc = o.render(1, 1, maxdepth=maxdepth, want_packed=False)
        out[i] = img[0, 0]
        for k in counts:
            counts[k] += rc[k]
    return out, counts


def colour_away(got, ref):
    """per ray: is a colour channel farther than the project's 1e-4 gate from the reference's (tests/test_trace_batch.py)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return (np.abs(got[:, :4] - ref[:, :4]) / np.maximum(1.0, np.abs(ref[:, :4]))).max(axis=1) > 1e-4


CONFIGS = [(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]  # (axis, sign) of the six ladders

# Rays whose colour the oracle ITSELF moves by more than the 1e-4 gate when it computes in fp32 instead of fp64 -- the worst count over the
# ladders, per material variant and stream (tests/test_packet_model.py measures them).  None: every shadow and reflected ray is clear of
# the edges by construction (Ladder.clear) and the materials are matte.  The GPU tests allow twice these, as tests/test_trace_batch.py does.
AWAY_FP32 = {("plain", "deep"): 0, ("plain", "shadow"): 0, ("plain", "mixed"): 0, ("mirror", "deep"): 0, ("mirror", "shadow"): 0, ("mirror", "mixed"): 0}
