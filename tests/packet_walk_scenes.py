"""The scenes and ray packets of tests/test_packet_walk_model_host.py / tests/test_packet_walk_streams_gpu.py (TEST INFRASTRUCTURE, no GPU):
the streams of the six ladders of tests/ladder.py, a heightfield of 16 x 16 cells and a 6 x 6 x 6 lattice whose tree changes axis in every
order, and the shadow packets the product makes of a stream.  tests/packet_walk_model.py says what they make the hand-written packet walk do."""
import numpy as np

import ladder
import packet_walk_model as PM
from glome_amd import scenes
from glome_amd.scene import SceneDesc

# ---------------------------------------------------------------- the ladder's packets
TILTS = [(1, 1), (-1, 1), (1, -1), (-1, -1)]


def comb_lanes(lad, sv, sw, n, seed, back):
    """n rays that start INSIDE the comb, in the corner of the cross-section opposite to their tilt, between two rungs (a place per lane, from
    the heavy end to the far end), and run towards the far end (back = False: aimed at an interior point of a rung triangle ahead) or towards the
    heavy end (back = True: they end on the screen or on the back of a rung)."""
    def one(i, rng):
        j = 1 + (i * 5 + seed) % (ladder.NLEV - 2)  # between rung j and rung j - 1
        u = ladder.rung_u(j) * rng.uniform(1.2, 1.7)
        o = np.array((u, -sv * ladder.W * rng.uniform(0.86, 0.9), -sw * ladder.W * rng.uniform(0.86, 0.9)))
        if back:
            return o, np.array((-0.2 * ladder.L, o[1] + sv * ladder.W * rng.uniform(0.2, 1.6), o[2] + sw * ladder.W * rng.uniform(0.2, 1.6)))
        if i % 7 == 3:  # stays in the corner: meets nothing
            return o, np.array((1.5 * ladder.L, o[1] + sv * ladder.W * rng.uniform(0.002, 0.008), o[2] + sw * ladder.W * rng.uniform(0.002, 0.008)))
        ahead = [t for k in range(j) for t in lad.rung_ids[k]]
        p = lad.local(lad.tri_pts[ahead[(i * 3 + seed) % len(ahead)]])
        b1 = rng.uniform(0.15, 0.55); b2 = rng.uniform(0.15, 0.85 - b1)
        return o, p[0] + b1 * (p[1] - p[0]) + b2 * (p[2] - p[0])
    return lad._draw(n, seed, one)


def nan_lane(lad, hi_z):
    """One ray whose root interval starts at NaN: its z direction component is -0 and its origin lies exactly on the upper z face of the tree's
    bounds (hi_z: the bounds are the triangles' with a margin, so the face lies above the screen triangle's highest corner), half a cross-section
    beside the axis: it runs along the comb on the face and meets nothing.  Only for a ladder whose axis is not z."""
    assert lad.axis != 2 and hi_z > max(float(p[:, 2].max()) for p in lad.tri_pts.values()) and float(np.float32(hi_z)) == hi_z
    other = 1 - lad.axis  # the cross-section's axis that is not z
    ou = np.zeros(3); ou[lad.axis] = lad.sign * 0.4 * ladder.rung_u(ladder.NLEV - 1); ou[other] = 0.5 * ladder.W; ou[2] = hi_z
    du = np.zeros(3); du[lad.axis] = lad.sign * 1.0; du[other] = 1e-7; du[2] = -0.0
    o = ou.astype(np.float32); dd = du.astype(np.float32)
    dd = (dd / np.linalg.norm(dd.astype(np.float64))).astype(np.float32)
    assert o[2] == np.float32(hi_z) and dd[2] == 0 and np.signbit(dd[2])
    return o, dd


def ladder_streams(lad, hi_z):
    """name -> (o, d): packets of 64 consecutive rays.  "deep": tests/ladder.py's, from the heavy end (16 pending entries); "comb": from inside
    the comb towards the far end; "back": from inside the comb towards the heavy end; "far_end": tests/ladder.py's reverse lanes, from beyond the
    rungs they aim at; "screen": rays at the screen whose shadow rays run the whole comb (mode 2); on the ladders along x and y, "nan": a "comb"
    packet whose lane 17 is nan_lane (hi_z: the upper z face of the tree's bounds on the device, device_bounds)."""
    out = {"deep": lad.deep_set()[:2]}
    for name, back in (("comb", False), ("back", True)):
        parts = [comb_lanes(lad, sv, sw, 64, 300 + 10 * k + back, back) for k, (sv, sw) in enumerate(TILTS)]
        out[name] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    parts = [lad.reverse_lanes(sv, sw, 64, k, 340 + k) for k, (sv, sw) in enumerate(TILTS)]
    out["far_end"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    out["screen"] = lad.shadow_set()[:2]
    if lad.axis != 2:
        o, d = (a[:64].copy() for a in out["comb"])
        o[17], d[17] = nan_lane(lad, hi_z)
        out["nan"] = (o, d)
    return out


def draw(scene, make, n):
    """n rays (o, d), lane i from make(i) = (origin, target), each drawn again until it is clear of every edge, its shadow rays too"""
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    todo = np.arange(n)
    for _ in range(200):
        if not len(todo):
            return o, d
        od = np.array([make(i) for i in todo])
        oo, dd = ladder._f32_rays(od[:, 0], od[:, 1] - od[:, 0])
        ok = scene.clear_with_shadow(oo, dd)
        o[todo[ok]], d[todo[ok]] = oo[ok], dd[ok]
        todo = todo[~ok]
    raise AssertionError("no clear ray found for lanes %s" % todo)


# ---------------------------------------------------------------- a heightfield of 16 x 16 cells under one light
FIELD_N = 16


class Field:
    """scenes.s3(16)'s heightfield: 512 triangles in one BIH under one light -- and two small triangles far outside it (60 along x, 400 along
    -z).  The field alone is 10 levels deep, the commit would give it a 10-entry stack, and a walk of it would never be the hand-written one
    (bih_tri_wave takes bih_walk_asm for a stack of exactly kAsmLdsCap LDS entries); each outlier puts a trimming branch above the field, which
    makes 12.  No ray of the streams goes anywhere near them.  Borrows tests/ladder.py's plain-geometry test of a ray's clearance from every edge."""
    mirror = False
    _all_hits, clear, _clear_chain, clear_with_shadow = ladder.Ladder._all_hits, ladder.Ladder.clear, ladder.Ladder._clear_chain, ladder.Ladder.clear_with_shadow
    OUTLIERS = [[60.0, 0.5, 0.0, 60.0, 0.5, 0.5, 60.5, 0.6, 0.0], [0.0, 0.5, -400.0, 0.0, 0.5, -399.5, 0.5, 0.6, -400.0]]

    def __init__(self):
        sd = self.sd = SceneDesc()
        mat = scenes.matte(sd, (0.8, 0.5, 0.4))
        T = np.concatenate([scenes.heightfield_triangles(FIELD_N), np.array(self.OUTLIERS)])
        self.bih_id = sd.bih(sd.triangles_bulk(T))
        sd.set_root(sd.tex(self.bih_id, mat))
        scenes._common(sd, 1)
        T = T.astype(np.float32).astype(np.float64).reshape(-1, 3, 3)
        self.tri_ids = list(range(len(T)))
        self.tri_pts = {i: T[i] for i in self.tri_ids}
        self.same_as = np.eye(len(T), dtype=bool)
        self.nfield = len(T) - len(self.OUTLIERS)

    def streams(self):
        """name -> (o, d).  "above": one packet per octant -- the origins high above one quarter of the field (or low beside it, for the rays that
        run upwards), each aimed at an interior point of a triangle, every seventh past the field --; "mixed": two packets that hold lanes of every
        octant; "low": four packets from just above the surface inside the field, one per horizontal quadrant of directions, almost level"""
        rng = np.random.default_rng(16)
        T = np.stack([self.tri_pts[i] for i in self.tri_ids])

        def inside(k):
            b1 = rng.uniform(0.2, 0.5); b2 = rng.uniform(0.2, 0.7 - b1)
            return T[k, 0] + b1 * (T[k, 1] - T[k, 0]) + b2 * (T[k, 2] - T[k, 0])

        def above(octant):
            sx, sy, sz = (1 if octant & 1 else -1), (1 if octant & 2 else -1), (1 if octant & 4 else -1)

            def make(i):
                p = inside(int(rng.integers(self.nfield)))
                if i % 7 == 3:
                    p = np.array((sx * 30.0, sy * 3.0, sz * 30.0)) * rng.uniform(0.8, 1.2, 3)
                # the origin lies against the direction signs: above the field for the rays that run downwards, below its rim for the others
                o = p - np.array((sx * rng.uniform(3.0, 14.0), sy * rng.uniform(2.0, 9.0), sz * rng.uniform(3.0, 14.0)))
                return o, p
            return make

        out = {}
        parts = [draw(self, above(k), 64) for k in range(8)]
        out["above"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        parts = [draw(self, lambda i: above((i + s) % 8)(i), 64) for s in (0, 3)]
        out["mixed"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))

        def low(sx, sz):
            def make(i):
                q = inside(int(rng.integers(self.nfield)))
                o = q + np.array((0.0, rng.uniform(0.05, 0.4), 0.0))
                return o, o + np.array((sx * rng.uniform(0.3, 1.0), rng.uniform(-0.08, 0.05), sz * rng.uniform(0.3, 1.0)))
            return make
        parts = [draw(self, low(sx, sz), 64) for sx in (1, -1) for sz in (1, -1)]
        out["low"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        return out


# ---------------------------------------------------------------- a lattice of small triangles whose tree changes axis in every order
LATTICE_N = 6


class Lattice(Field):
    """6 x 6 x 6 small triangles on a lattice whose pitch differs per axis and per slab (so the longest axis of a node's bounds, which the
    builder splits, changes in every order on the way down: x after x, z after z and y after y among them), in one BIH under one light, with
    far outliers that each put a trimming branch above it until the tree is 12 levels deep: the stack the hand-written walk is compiled for
    (Field does the same with two).  No ray of the streams goes anywhere near the outliers.  TWO lights, on opposite sides: the shadow packets
    of one light all run one way, and which register set a node of the tree is walked in would never change."""
    LIGHT2 = (120.0, -90.0, -60.0)
    FAR = [(900.0, 0.0, 0.0), (0.0, 0.0, -5000.0), (0.0, 30000.0, 0.0), (-2.0e5, 0.0, 0.0), (0.0, 0.0, 1.2e6), (0.0, -7.0e6, 0.0)]

    def __init__(self, depth=PM.LDS_CAP):
        from oracle import np_scene as NS
        rng = np.random.default_rng(66)
        # pitches: x grows, y shrinks, z alternates -- the extents of the sub-boxes are ordered differently in different corners
        gx = np.cumsum([0.0, 0.5, 0.7, 1.0, 1.5, 2.3]); gy = np.cumsum([0.0, 1.9, 1.3, 0.9, 0.6, 0.4]); gz = np.cumsum([0.0, 0.6, 1.6, 0.6, 1.6, 0.6])
        tris = []
        for x in gx:
            for y in gy:
                for z in gz:
                    p = np.array((x, y, z)) + rng.uniform(-0.03, 0.03, 3)
                    a, b = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
                    a *= 0.16 / np.linalg.norm(a); b -= a * (a @ b) / (a @ a); b *= 0.16 / np.linalg.norm(b)
                    tris.append(np.concatenate([p, p + a, p + b]))
        for nout in range(len(self.FAR) + 1):
            T = np.array(tris + [np.concatenate([np.array(c), np.array(c) + (0.0, 0.3, 0.0), np.array(c) + (0.3, 0.0, 0.3)]) for c in self.FAR[:nout]])
            sd = SceneDesc()
            mat = scenes.matte(sd, (0.8, 0.5, 0.4))
            bih_id = sd.bih(sd.triangles_bulk(T))
            sd.set_root(sd.tex(bih_id, mat))
            scenes._common(sd, 1)
            sd.add_light(self.LIGHT2, sd.lights[0][1])
            sc, nm = NS.load(sd)
            if PM.tree_depth(sc.nodes[nm[bih_id]].root) >= depth:
                break
        self.sd, self.bih_id, self.bih = sd, bih_id, sc.nodes[nm[bih_id]]
        assert PM.tree_depth(self.bih.root) == depth, PM.tree_depth(self.bih.root)
        T = T.astype(np.float32).astype(np.float64).reshape(-1, 3, 3)
        self.tri_ids = list(range(len(T)))
        self.tri_pts = {i: T[i] for i in self.tri_ids}
        self.same_as = np.eye(len(T), dtype=bool)
        self.nfield = len(tris)
        self.lo, self.hi = T[:self.nfield].reshape(-1, 3).min(0), T[:self.nfield].reshape(-1, 3).max(0)

    def clear_with_shadow(self, o32, d32, depth=3):
        """tests/ladder.py's test of a ray's clearance from every edge, and of its shadow rays' towards EVERY light (matte: nothing is reflected)"""
        o, d = o32.astype(np.float64), d32.astype(np.float64)
        ok, k, t = self.clear(o, d)
        hit = k >= 0
        if hit.any():
            P = np.stack([self.tri_pts[i] for i in self.tri_ids])[k[hit]]
            nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            pos = o[hit] + t[hit][:, None] * d[hit]
            for light in self.sd.lights:
                lv = np.array(light[0]) - pos
                ll = np.linalg.norm(lv, axis=1)
                lit = np.einsum("ij,ij->i", lv, nrm) >= 0
                ok[np.flatnonzero(hit)] &= self.clear(pos + 1e-4 * nrm, lv / ll[:, None], ll - 2e-4, any_hit=True)[0] | ~lit
        return ok

    def streams(self):
        """name -> (o, d).  "outside": one packet per octant from outside the lattice, each lane aimed at an interior point of a triangle, every
        seventh past everything; "inside": eight packets from points between the triangles, aimed the same way; "mixed": four packets of every octant"""
        rng = np.random.default_rng(67)
        T = np.stack([self.tri_pts[i] for i in self.tri_ids])
        centre, size = 0.5 * (self.lo + self.hi), self.hi - self.lo

        def inside(k):
            b1 = rng.uniform(0.2, 0.5); b2 = rng.uniform(0.2, 0.7 - b1)
            return T[k, 0] + b1 * (T[k, 1] - T[k, 0]) + b2 * (T[k, 2] - T[k, 0])

        def outside(octant):
            s = np.array([1 if octant >> a & 1 else -1 for a in range(3)])

            def make(i):
                p = inside(int(rng.integers(self.nfield)))
                if i % 7 == 3:
                    p = centre + s * size * rng.uniform(0.8, 1.2, 3)
                return centre - s * size * rng.uniform(0.7, 1.6, 3), p
            return make

        def between(i):
            o = self.lo + size * rng.uniform(0.05, 0.95, 3)
            return o, inside(int(rng.integers(self.nfield)))

        out = {}
        parts = [draw(self, outside(k), 64) for k in range(8)]
        out["outside"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        out["inside"] = draw(self, between, 512)
        out["mixed"] = draw(self, lambda i: outside((i + i // 64) % 8)(i), 256)
        return out


def shadow_stream(scene, o, d, res):
    """the shadow packets the product makes of a stream of primary rays (mpreshade, Shader.hs:65-80; tests/ladder.py's _clear_chain restates it
    the same way): per packet of 64, and per light, the lanes that hit a triangle facing it, from the hit point lifted 1e-4 along the normal, as far as
    the light less two deltas.  res: the stream's modelled closest hits (mode 1).  Returns a list of (o, d, limit) per packet."""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out = []
    for i, r in enumerate(res):
        sl = slice(64 * i, 64 * i + len(r["prim"]))
        hit = r["prim"] >= 0
        if not hit.any():
            continue
        # the model's t is along the direction as given: the streams' directions are unit vectors in fp32, the difference is below what a class needs
        P = np.stack([scene.pts_of_uid[u] for u in r["prim"][hit]])
        nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        pos = o[sl][hit] + r["t"][hit][:, None] * np.asarray(d[sl][hit])
        for light in scene.sd.lights:  # one shadow packet per light
            lv = np.array(light[0], np.float64) - pos
            ll = np.linalg.norm(lv, axis=1)
            lit = np.einsum("ij,ij->i", lv, nrm) >= 0
            if lit.any():
                out.append(((pos + 1e-4 * nrm)[lit], (lv / ll[:, None])[lit], (ll - 2e-4)[lit]))
    return out


def with_uids(scene, bih):
    """scene.pts_of_uid: np_scene uid of a triangle of `bih` -> its corners (for shadow_stream)"""
    scene.pts_of_uid = {PM._tri(s).uid: np.asarray(PM._tri(s).p, np.float64) for leaf in PM.leaves(bih.root) for s in leaf}
    return scene
