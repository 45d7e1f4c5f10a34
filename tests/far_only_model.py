"""The branch step of the hand-written packet walk (GLOME_PKW_STEP, glome_amd/csrc/bih_packet_asm.hpp) restated step by step for the
64 lanes of a wave (TEST INFRASTRUCTURE, no GPU), and the ray packets of tests/test_far_only_steps_host.py / _gpu.py.

tests/packet_model.py says what a packet makes the walk do as a whole.  This module says what every single branch step is, as the block
takes it since the votes were reordered:

  far vote empty                     "near" (the lanes of the near child go on) or "neither" (a pop follows)
  far vote not empty, near vote too  "both": the one step that pushes -- inside the block below the LDS part's capacity, else handed to
                                     the C++ step (where = "cpp"), which pushes to the overflow columns; the walk re-enters afterwards
  far vote not empty, near empty     "far": the far child alone.  Nothing is pushed, whatever the stack holds; its node is fetched into the
                                     register set the step ran in

and, per step, what the block's state is: the stack pointer, the register set the node is in (A after every fetch that was not
prefetched: the root, a pop, a re-entry; the other set after a "near" or "both" step, the same set after a "far" step), the axis and
the direction, whether the far child is a leaf, whether its lanes are a strict subset of the node's, whether one of them carries a NaN
`near`, how many lanes are occluded already (mode 2), and what came directly before the step.

origin_clip: the production walks start at the ray's origin (bih_clip_root_at_origin); packet_model.walk_packet restates the
reference's interval, so the comparison with it is made without the clip.  Unlike packet_model this walk takes a direction component
of +-0: bbclip_ub then gives a NaN `near` for an origin exactly on the upper z face of the bounds (gmax3f keeps a NaN third operand)."""
import collections

import numpy as np

import ladder
import packet_model as PM
from glome_amd import scenes
from glome_amd.scene import SceneDesc

CAP = PM.LDS_CAP
FLT_MIN = float(np.finfo(np.float32).tiny)

Step = collections.namedtuple("Step", "kind where sp set axis fwd octant fc_leaf far_subset nan_near mode occluded after")


def _empty(c):
    return c[0] == "leaf" and not c[1]


def device_bounds(bb):
    """the tree's bounds as the device holds them (flatten.hpp: the lower corner rounded down to fp32, the upper one rounded up)"""
    lo, hi = np.asarray(bb[0], np.float64), np.asarray(bb[1], np.float64)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32.astype(np.float64) > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32)
    hi32 = np.where(hi32.astype(np.float64) < hi, np.nextafter(hi32, np.float32(np.inf)), hi32)
    return lo32.astype(np.float64), hi32.astype(np.float64)


def walk_steps(bih, o, d, dist, mode, origin_clip=True):
    """One packet, as packet_model.walk_packet takes it.  Returns a dict: steps (every branch step of every walk, in order), pushes_over (pushes
    at stack entry >= CAP: the C++ steps), pops_over, max_depth, prim / t / occluded per lane.  origin_clip = True is the production walk: the
    root interval over the device's bounds, clipped at the origin; False is packet_model's."""
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    assert 1 <= n <= 64 and mode in (1, 2) and bih.root[0] == "branch"
    dist = np.broadcast_to(np.asarray(dist, np.float64), (n,))
    with np.errstate(divide="ignore", invalid="ignore"):
        rcp = 1.0 / d
        near0, far0 = PM.root_interval(device_bounds(bih.bb) if origin_clip else bih.bb, o, d, dist)
    if origin_clip:
        near0 = np.where(-FLT_MIN > near0, -FLT_MIN, near0)  # gmaxf(-FLT_MIN, near): a NaN near stays
    octant = (rcp[:, 0] > 0) * 1 + (rcp[:, 1] > 0) * 2 + (rcp[:, 2] > 0) * 4
    todo = ~(near0 > far0)
    best_t = np.full(n, PM.NO_BEST); prim = np.full(n, -1, np.int64); occ = np.zeros(n, bool)
    steps = []
    max_depth = pushes_over = pops_over = 0
    while todo.any():
        fwdbits = int(octant[np.flatnonzero(todo)[0]])
        am = todo & (octant == fwdbits)
        todo &= ~am
        near, far = near0.copy(), far0.copy()
        node, stack = bih.root, []
        rset, after = "A", "root"
        while True:
            while node[0] == "branch":
                _, lsplit, rsplit, axis, left, right = node
                with np.errstate(invalid="ignore"):
                    dl, dr = (lsplit - o[:, axis]) * rcp[:, axis], (rsplit - o[:, axis]) * rcp[:, axis]
                    fwd = (fwdbits >> axis) & 1
                    c1, c2 = (left, right) if fwd else (right, left)
                    t1, t2 = (dl, dr) if fwd else (dr, dl)
                    vf = am & (t2 < far) & (not _empty(c2))    # the far vote (VCC)
                    vn = am & (near < t1) & (not _empty(c1))   # the near vote (s[K28:K29] / v_cmpx)
                    f1, n2 = np.minimum(t1, far), np.maximum(t2, near)  # (v_maximum3: NaN when an operand is)
                sp = len(stack)
                kind = ("both" if vn.any() else "far") if vf.any() else ("near" if vn.any() else "neither")
                where = "cpp" if kind == "both" and sp >= CAP else "asm"
                steps.append(Step(kind, where, sp, rset, axis, bool(fwd), fwdbits, c2[0] == "leaf", bool(vf.any() and (am & ~vf).any()),
                                  bool((vf & np.isnan(near)).any()), mode, int(occ.sum()), after))
                if kind == "both":
                    pushes_over += sp >= CAP
                    stack.append((c2, vf, n2, far.copy()))
                    max_depth = max(max_depth, len(stack))
                if kind in ("both", "near"):
                    node, am, far = c1, vn, np.where(vn, f1, far)
                    rset = "B" if rset == "A" else "A"
                else:
                    node, am, near = c2, vf, np.where(vf, n2, near)  # ("neither": am becomes empty)
                after = "step"
                if where == "cpp":
                    rset, after = "A", "reentry"  # phase 0: L_node fetches into set A
                if not am.any():
                    break
            if am.any():
                for s in node[1]:
                    tr = PM._tri(s)
                    hit, t = PM.tri_hits(tr.p, o, d, far)
                    hit &= am
                    if mode == 2:
                        occ |= hit; prim[hit] = tr.uid; am = am & ~hit
                    else:
                        acc = hit & ~(best_t < t)
                        best_t = np.where(acc, t, best_t); prim[acc] = tr.uid
                        far = np.where(acc & (far > t), t, far)
            am = np.zeros(n, bool)
            while stack and not am.any():
                over = len(stack) - 1 >= CAP
                pops_over += over
                node, am, near, far = stack.pop()
                if mode == 1:
                    far = np.where(far > best_t, best_t, far)
                    am = am & ~(near > far)
                else:
                    am = am & ~occ
                rset, after = "A", ("reentry" if over else "pop")
            if not am.any():
                break
    return {"steps": steps, "pushes_over": int(pushes_over), "pops_over": int(pops_over), "max_depth": max_depth, "prim": prim,
            "t": np.where(prim >= 0, best_t, -1.0) if mode == 1 else None, "occluded": occ if mode == 2 else None}


def stream_steps(bih, o, d, dist, mode, origin_clip=True):
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    dist = np.broadcast_to(np.asarray(dist, np.float64), (len(o),))
    return [walk_steps(bih, o[i:i + 64], d[i:i + 64], dist[i:i + 64], mode, origin_clip) for i in range(0, len(o), 64)]


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
        parts = [draw(above(k), 64) for k in range(8)]
        out["above"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        parts = [draw(lambda i: above((i + s) % 8)(i), 64) for s in (0, 3)]
        out["mixed"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))

        def low(sx, sz):
            def make(i):
                q = inside(int(rng.integers(self.nfield)))
                o = q + np.array((0.0, rng.uniform(0.05, 0.4), 0.0))
                return o, o + np.array((sx * rng.uniform(0.3, 1.0), rng.uniform(-0.08, 0.05), sz * rng.uniform(0.3, 1.0)))
            return make
        parts = [draw(low(sx, sz), 64) for sx in (1, -1) for sz in (1, -1)]
        out["low"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
        return out
