"""The hand-written packet walk (GLOME_PKW_ASM, glome_amd/csrc/bih_packet_asm.hpp) restated BLOCK BY BLOCK for the 64 lanes of a wave (TEST
INFRASTRUCTURE, no GPU), and the scenes and ray packets of tests/test_dispatch_sites_host.py / _gpu.py and tests/test_pop_fold_host.py.

tests/packet_model.py says what a packet makes the walk do as a whole, tests/far_only_model.py what every branch step is.  This module
runs the walk the way bih_tri_packet_hw (rt_device.hpp) does: a loop around the block, which is entered with (phase, ref, am, sp), leaves
with a status (0 done, 1 a push beyond the LDS part, 3 a pop from beyond it) and is re-entered after the C++ step.  Inside the block it
follows the labels:

  dispatch   the branch on a reference's two low bits.  Since round 12 every SITE has its own form, so every site is recorded: after a
             both / near-only / far-only step on each axis in the register set the step ran in, after a pop (always set A), at the root
             (L_node at the first entry) and after a re-entry from a C++ step (L_node again: phase 0, the entries read back)
  pop        as the block takes it since round 12: m0 = m0 - 1 in 32 unsigned bits, ONE compare m0 >= CAP (an empty stack leaves
             0xffffffff and so goes the same way as an entry beyond the LDS part), and only the slow label tells the two apart
  leaf       which items of a leaf some lane accepts as a hit: item 2 p + 1 is the B half of pair record p, whose record index the
             block makes with v_add_u32 from the A half's

origin_clip as in far_only_model: True is the production walk, False is packet_model's interval (for the comparison with it)."""
import collections

import numpy as np

import far_only_model as FM
import ladder
import packet_model as PM
from glome_amd import scenes
from glome_amd.scene import SceneDesc

CAP = PM.LDS_CAP
U32 = 0xFFFFFFFF

Entry = collections.namedtuple("Entry", "phase sp mode")
Dispatch = collections.namedtuple("Dispatch", "site axis set target mode")  # axis, set: of the step left (None, "A" for pop / root / reentry)
Pop = collections.namedtuple("Pop", "sp outcome mode")  # sp before the pop; outcome: taken / rejected / empty / over (handed to C++)
Leaf = collections.namedtuple("Leaf", "size hits mode")  # hits: the item indices within the leaf that some lane accepted
Exit = collections.namedtuple("Exit", "status sp lanes mode")

STEP_SITES = [(k, a, s) for k in ("both", "near", "far") for a in range(3) for s in "AB"]
TARGETS = (0, 1, 2, 3)  # a branch along x / y / z, a leaf


def pop_fold(m0, cap=CAP):
    """L_pop's first three instructions and L_popslow's first two, on the stack pointer alone: s_sub_u32 m0, m0, 1; s_cmp_ge_u32 m0, cap;
    s_cbranch_scc1 L_popslow -- and there s_cmp_eq_u32 m0, -1; s_cbranch_scc1 L_empty; s_add_u32 m0, m0, 1.  Returns (where, m0): "lds" with
    the entry's index, "empty" with 0 (L_empty's s_mov_b32 m0, 0), or "over" with the stack pointer as it was (status 3)."""
    assert 0 <= m0 <= U32
    m0 = (m0 - 1) & U32
    if m0 >= cap:  # unsigned
        if m0 == U32:
            return "empty", 0
        return "over", (m0 + 1) & U32
    return "lds", m0


def _kind(node):
    return 3 if node[0] == "leaf" else node[3]


class _Walk:
    """one walk of one octant: the state bih_tri_packet_hw keeps between two entries of the block"""

    def __init__(self, bih, o, d, rcp, fwdbits, am, near, far, mode, best_t, prim, occ, ev):
        self.o, self.d, self.rcp, self.fwdbits, self.mode, self.ev = o, d, rcp, fwdbits, mode, ev
        self.node, self.am, self.near, self.far = bih.root, am, near, far
        self.best_t, self.prim, self.occ = best_t, prim, occ
        self.stack, self.sp, self.max_depth = [], 0, 0

    def votes(self):
        _, lsplit, rsplit, axis, left, right = self.node
        with np.errstate(invalid="ignore"):
            dl, dr = (lsplit - self.o[:, axis]) * self.rcp[:, axis], (rsplit - self.o[:, axis]) * self.rcp[:, axis]
            fwd = (self.fwdbits >> axis) & 1
            c1, c2 = (left, right) if fwd else (right, left)
            t1, t2 = (dl, dr) if fwd else (dr, dl)
            vf = self.am & (t2 < self.far) & (not FM._empty(c2))
            vn = self.am & (self.near < t1) & (not FM._empty(c1))
            f1, n2 = np.minimum(t1, self.far), np.maximum(t2, self.near)
        return axis, c1, c2, vn, vf, f1, n2

    def filter(self, entry):
        """a popped entry: the lanes that still want it"""
        self.node, am, self.near, self.far = entry
        if self.mode == 1:
            self.far = np.where(self.far > self.best_t, self.best_t, self.far)
            am = am & ~(self.near > self.far)
        else:
            am = am & ~self.occ
        self.am = am
        return am.any()

    def leaf(self):
        hits = set()
        for k, s in enumerate(self.node[1]):
            tr = PM._tri(s)
            hit, t = PM.tri_hits(tr.p, self.o, self.d, self.far)
            hit &= self.am
            if self.mode == 2:
                self.occ |= hit; self.prim[hit] = tr.uid; self.am = self.am & ~hit
                acc = hit
            else:
                acc = hit & ~(self.best_t < t)
                self.best_t[:] = np.where(acc, t, self.best_t); self.prim[acc] = tr.uid
                self.far = np.where(acc & (self.far > t), t, self.far)
            if acc.any():
                hits.add(k)
        self.ev.append(Leaf(len(self.node[1]), frozenset(hits), self.mode))

    def block(self, phase, first):
        """GLOME_PKW_ASM from its first instruction to L_end: returns the status"""
        ev, mode = self.ev, self.mode
        m0 = self.sp
        ev.append(Entry(phase, self.sp, mode))
        state = "pop" if phase else "dispatch"
        site, cur = (("root" if first else "reentry"), None, "A"), "A"  # (site, axis, set of the dispatching code), the set the node arrives in
        while True:
            if state == "dispatch":
                ev.append(Dispatch(site[0], site[1], site[2], _kind(self.node), mode))
                state = "leaf" if self.node[0] == "leaf" else "step"
            elif state == "step":
                axis, c1, c2, vn, vf, f1, n2 = self.votes()
                other = "B" if cur == "A" else "A"
                if vf.any() and vn.any():
                    if m0 >= CAP:  # L_slow: the C++ step takes this node
                        self.sp = m0
                        return 1
                    assert len(self.stack) == m0
                    self.stack.append((c2, vf, n2, self.far.copy())); m0 += 1
                    self.max_depth = max(self.max_depth, m0)
                    kind = "both"
                else:
                    kind = "far" if vf.any() else ("near" if vn.any() else "neither")
                if kind == "neither":
                    state = "pop"
                    continue
                site = (kind, axis, cur)
                if kind == "far":
                    self.node, self.am, self.near = c2, vf, np.where(vf, n2, self.near)
                else:
                    self.node, self.am, self.far = c1, vn, np.where(vn, f1, self.far)
                    cur = other
                state = "dispatch"
            elif state == "leaf":
                self.leaf()
                state = "pop"
            else:  # L_pop
                where, m0 = pop_fold(m0)  # the one compare; L_popslow tells the two cases apart
                if where == "empty":
                    ev.append(Pop(0, "empty", mode))
                    self.sp = 0; self.am = np.zeros(len(self.o), bool)
                    return 0
                if where == "over":
                    ev.append(Pop(m0, "over", mode))
                    self.sp = m0
                    return 3
                assert len(self.stack) == m0 + 1
                if self.filter(self.stack.pop()):
                    ev.append(Pop(m0 + 1, "taken", mode))
                    site, cur = ("pop", None, "A"), "A"
                    state = "dispatch"
                else:
                    ev.append(Pop(m0 + 1, "rejected", mode))

    def run(self):
        """bih_tri_packet_hw's loop"""
        phase, first = 0, True
        while True:
            st = self.block(phase, first)
            first = False
            self.ev.append(Exit(st, self.sp, int(self.am.sum()), self.mode))
            if st == 0:
                return
            if st == 1:  # one branch step of bih_tri_packet; its push goes to the overflow columns
                axis, c1, c2, vn, vf, f1, n2 = self.votes()
                assert vn.any() and vf.any() and len(self.stack) == self.sp
                self.stack.append((c2, vf, n2, self.far.copy())); self.sp += 1
                self.max_depth = max(self.max_depth, self.sp)
                self.node, self.am, self.far = c1, vn, np.where(vn, f1, self.far)
                phase = 0
            else:
                assert len(self.stack) == self.sp
                self.sp -= 1
                phase = 0 if self.filter(self.stack.pop()) else 1


def walk_events(bih, o, d, dist, mode, origin_clip=True):
    """One packet, as packet_model.walk_packet takes it.  Returns a dict: events (every Entry, Dispatch, Pop, Leaf and Exit of every walk, in order),
    exits_push / exits_pop (block exits with status 1 / 3), max_depth, prim / t / occluded per lane."""
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    assert 1 <= n <= 64 and mode in (1, 2) and bih.root[0] == "branch"
    dist = np.broadcast_to(np.asarray(dist, np.float64), (n,))
    with np.errstate(divide="ignore", invalid="ignore"):
        rcp = 1.0 / d
        near0, far0 = PM.root_interval(FM.device_bounds(bih.bb) if origin_clip else bih.bb, o, d, dist)
    if origin_clip:
        near0 = np.where(-FM.FLT_MIN > near0, -FM.FLT_MIN, near0)
    octant = (rcp[:, 0] > 0) * 1 + (rcp[:, 1] > 0) * 2 + (rcp[:, 2] > 0) * 4
    todo = ~(near0 > far0)
    best_t = np.full(n, PM.NO_BEST); prim = np.full(n, -1, np.int64); occ = np.zeros(n, bool)
    ev, max_depth = [], 0
    while todo.any():
        fwdbits = int(octant[np.flatnonzero(todo)[0]])
        am = todo & (octant == fwdbits)
        todo &= ~am
        w = _Walk(bih, o, d, rcp, fwdbits, am, near0.copy(), far0.copy(), mode, best_t, prim, occ, ev)
        w.run()
        assert not w.stack
        max_depth = max(max_depth, w.max_depth)
    return {"events": ev, "exits_push": sum(isinstance(e, Exit) and e.status == 1 for e in ev), "exits_pop": sum(isinstance(e, Exit) and e.status == 3 for e in ev),
            "max_depth": max_depth, "prim": prim, "t": np.where(prim >= 0, best_t, -1.0) if mode == 1 else None, "occluded": occ if mode == 2 else None}


def stream_events(bih, o, d, dist, mode, origin_clip=True):
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    dist = np.broadcast_to(np.asarray(dist, np.float64), (len(o),))
    return [walk_events(bih, o[i:i + 64], d[i:i + 64], dist[i:i + 64], mode, origin_clip) for i in range(0, len(o), 64)]


def shadow_stream(scene, o, d, res):
    """the shadow packets the product makes of a stream of primary rays (mpreshade, Shader.hs:65-80; tests/ladder.py's _clear_chain restates it
    the same way): per packet of 64, and per light, the lanes that hit a triangle facing it, from the hit point lifted 1e-4 along the normal, as far as
    the light less two deltas.  res: the stream's modelled closest hits (stream_events, mode 1).  Returns a list of (o, d, limit) per packet."""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out = []
    for i, r in enumerate(res):
        sl = slice(64 * i, 64 * i + len(r["prim"]))
        hit = r["prim"] >= 0
        if not hit.any():
            continue
        # packet_model's t is along the direction as given: the streams' directions are unit vectors in fp32, the difference is below what a class needs
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


# ---------------------------------------------------------------- a lattice of small triangles whose tree changes axis in every order
LATTICE_N = 6


class Lattice(FM.Field):
    """6 x 6 x 6 small triangles on a lattice whose pitch differs per axis and per slab (so the longest axis of a node's bounds, which the
    builder splits, changes in every order on the way down: x after x, z after z and y after y among them), in one BIH under one light, with
    far outliers that each put a trimming branch above it until the tree is 12 levels deep: the stack the hand-written walk is compiled for
    (tests/far_only_model.py's Field does the same with two).  No ray of the streams goes anywhere near the outliers.  TWO lights, on opposite
    sides: the shadow packets of one light all run one way, and which register set a node of the tree is walked in would never change."""
    LIGHT2 = (120.0, -90.0, -60.0)
    FAR = [(900.0, 0.0, 0.0), (0.0, 0.0, -5000.0), (0.0, 30000.0, 0.0), (-2.0e5, 0.0, 0.0), (0.0, 0.0, 1.2e6), (0.0, -7.0e6, 0.0)]

    def __init__(self, depth=CAP):
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

        def draw(make, n):
            o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
            todo = np.arange(n)
            for _ in range(200):
                if not len(todo):
                    return o, d
                od = np.array([make(i) for i in todo])
                oo, dd = ladder._f32_rays(od[:, 0], od[:, 1] - od[:, 0])
                ok = self.clear_with_shadow(oo, dd)
                o[todo[ok]], d[todo[ok]] = oo[ok], dd[ok]
                todo = todo[~ok]
            raise AssertionError("no clear ray found for lanes %s" % todo)

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
        parts = [draw(outside(k), 64) for k in range(8)]
        out["outside"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        out["inside"] = draw(between, 512)
        out["mixed"] = draw(lambda i: outside((i + i // 64) % 8)(i), 256)
        return out


def with_uids(scene, bih):
    """scene.pts_of_uid: np_scene uid of a triangle of `bih` -> its corners (for shadow_stream)"""
    scene.pts_of_uid = {PM._tri(s).uid: np.asarray(PM._tri(s).p, np.float64) for leaf in PM.leaves(bih.root) for s in leaf}
    return scene
