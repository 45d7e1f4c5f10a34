"""Lattice rays: every Solid's edge branches held to the oracle, case by case.

A plain module (no GPU, no fixtures) shared by tests/test_lattice_host.py and tests/test_lattice_gpu.py:

  OBJECTS   small solids whose parameters are dyadic and of magnitude at most 4, written as SceneDesc fragments;
  ROUTES    the ways an object is placed in a scene, each named after the device code it is meant to reach
            (tests/test_lattice_host.py asserts from the commit's own traits that it does);
  rays      LATTICE rays -- origins on the half-integer lattice of [-4, 4]^3, direction components from {+0, -0, +-0.5, +-1, +-2},
            tmax a multiple of 0.5 -- and AIMED families, one generator per primitive kind, each naming the branch it is aimed at.
            Every ray carries a label; the arrays are float32 and nothing renormalises them, so signed zeros reach the device bit for bit.
            An aimed family comes twice: as written, and with its directions normalised in fp32 (label + "/unit"); a family about an
            exact equality has no twin, and runs where the arithmetic is exact on the device (DESIGN.md 4.9 says which runs where).
            Where it is not, the pair also gets lattice rays with origins off the lattice (`lattice+`, N_PLAIN_INEXACT below).

A case is one ray of one object on one route, through the three seams rayint, shadow and inside.  evaluate() computes it three ways
on the CPU -- the fp64 oracle, the oracle in float, the host build of the device headers -- and marks the AGREEMENT SET: the cases on
which all three decide alike (hit / miss, primitive, texture stack, shadow, inside), give depths within parity.T_RTOL, and none gives
the ray up (the oracle's `diverged` flag, the host build's limit status).  Inside that set a backend is held on EVERY case, with no
outlier fraction (check_backend); outside it nothing is asserted and the counts go to profiles/lattice_agreement.txt."""
import functools
from collections import namedtuple

import numpy as np

import parity
from helpers import HostSim, O
from glome_amd import api
from glome_amd.scene import SceneDesc
from oracle import np_scene as NS

N_LATTICE = 8000     # lattice rays per object and route (with the aimed families: well under 20,000)
# Where the arithmetic is inexact whatever the ray (has_instance, inexact: 63 of the 93 pairs) the half-integer lattice is kept, and
# rounding_stable judges every ray of it; what it moves out there, measured with 8,000 plain rays per pair: up to 7.4 % of them (plane
# on generic: origins in the plane), 5.7 % (the Mesh), 2-3.4 % (CSG solids, boxes and discs below an Instance, the triangle bih), that is
# two to seven times the cap on its own.  The cap is a share of the pair's cases, so such a pair gets MORE cases: 3,000 rays of the plain
# lattice, every one judged, and 9,000 whose origins are moved off it by (1, 3, 5) / 64 (`lattice+`), which meet no plane and no edge
# exactly and still carry the signed zeros, the origins inside, the axis-parallel and the non-unit directions.  Both kinds keep their
# own labels and so their own floor of 32.
N_PLAIN_INEXACT, N_LATTICE_INEXACT = 3000, 12000
NORMAL_TOL = 2e-3    # parity.check_rays' normal tolerance, with its allowance set to zero
MAX_OUTSIDE = 0.02   # at most this share of an object-and-route's cases may lie outside the agreement set
MIN_PER_LABEL = 32   # and every label keeps at least this many inside it

DIR_VALUES = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], np.float32)
AXES = np.eye(3, dtype=np.float32)

Family = namedtuple("Family", "label o d tmax expect")  # expect: what the fp64 oracle must answer (hit, n, inside, t, nan, prim); {} = nothing stated
Obj = namedtuple("Obj", "name build families routes")    # build(sd) -> (node, {name: node} of the parts a family's `prim` names)


def f32(x):
    return np.asarray(x, np.float32)


def _fam(label, o, d, tmax, **expect):
    o = f32(o).reshape(-1, 3); d = f32(d).reshape(-1, 3)
    assert len(o) == len(d) and len(o) >= MIN_PER_LABEL + 8, (label, len(o))
    return Family(label, o, d, np.ascontiguousarray(np.broadcast_to(f32(tmax), (len(o),))), expect)


def axis_dir(a, s, mag=1.0):
    """+-mag along axis a, the other two components -0: a +0 component misses every box and every bih (Q1), a -0 does not"""
    v = np.full(3, -0.0); v[a] = s * mag
    return v


def apply_linear(A, v):
    """A v for a matrix with one non-zero entry per row (a permutation with scales): a product, never a sum, so a zero keeps its sign"""
    A = np.asarray(A, np.float64); v = np.asarray(v, np.float64).reshape(-1, 3)
    assert np.all((A != 0).sum(1) == 1) and np.all((A != 0).sum(0) == 1), A
    return np.stack([v[:, int(np.flatnonzero(A[i])[0])] * A[i, int(np.flatnonzero(A[i])[0])] for i in range(3)], 1)


def ulp_step(x, k):
    """x moved k fp32 steps (k = +-1)"""
    return np.nextafter(f32(x), f32(np.inf if k > 0 else -np.inf))


def with_tmax_edges(label, o, d, t, **expect):
    """tmax == t exactly (a hit: the tests reject `t > tmax`), and tmax one fp32 step either side of it"""
    t = f32(t)
    return [_fam(label + ":tmax==t", o, d, t, hit=True, t=t, exact_only=True, **expect),
            _fam(label + ":tmax-ulp", o, d, ulp_step(t, -1), hit=False, exact_only=True),
            _fam(label + ":tmax+ulp", o, d, ulp_step(t, +1), hit=True, t=t, exact_only=True, **expect)]


def _signs(v):
    """v with every combination of signs of its non-zero components"""
    out = {tuple(v)}
    for k in range(3):
        out |= {tuple(-x if j == k else x for j, x in enumerate(w)) for w in out}
    return sorted(out)


def _perms(v):
    a, b, c = v
    return sorted({(a, b, c), (a, c, b), (b, a, c), (b, c, a), (c, a, b), (c, b, a)})


# ---------------------------------------------------------------------------------------------------------------- sphere
def sphere_families(c, r, tag="sphere"):
    """c dyadic, r a dyadic multiple of 2.5, so that (0.6 r, 0.8 r, 0) is a dyadic point ON the sphere"""
    c = np.asarray(c, np.float64)
    fams = []
    on = [p for q in _perms((0.6 * r, 0.8 * r, 0.0)) + _perms((r, 0.0, 0.0)) for p in _signs(q)]  # lattice points ON the sphere
    # tangent: an axis direction (unit length as written) at distance r from the centre; disc == 0 and `disc < 0` is false
    o, d, t = [], [], []
    for a in range(3):
        for b in range(3):
            if b == a: continue
            for s in (-1.0, 1.0):
                for k in (2.0, 2.5, 3.0, 3.5, 4.0 - abs(c).max()):
                    for sa in (-1.0, 1.0):
                        p = np.zeros(3); p[b] = s * r; p[a] = -sa * k
                        o.append(c + p); d.append(axis_dir(a, sa)); t.append(k)
    fams.append(_fam(tag + ":tangent", o, d, 8.0, hit=True, t=t, exact_only=True))
    # through lattice points of the sphere along an axis: sqrt(disc) is exact
    o, d, t = [], [], []
    for p in on:
        for a in range(3):
            if p[a] == 0: continue
            for k in (1.0, 1.5):
                s = np.sign(p[a])
                q = np.array(p); q[a] += s * k
                o.append(c + q); d.append(axis_dir(a, -s)); t.append(k)
    fams += with_tmax_edges(tag, o, d, t)
    # hitdist == 0: the origin ON the sphere, leaving along an axis (`v + d` is 0, and `hitdist < 0` is false)
    o, d = [], []
    for p in on:
        for a in range(3):
            if p[a] != 0: o.append(c + np.array(p)); d.append(axis_dir(a, np.sign(p[a])))
    fams.append(_fam(tag + ":hitdist==0", o, d, 4.0, hit=True, t=np.zeros(len(o)), exact_only=True))
    # origin inside: the `v + d` root; shadow_sphere's early-out says no shadow here for v <= 0 (Q4)
    o, d = [], []
    for p in on:
        for a in range(3):
            for s in (-1.0, 1.0):
                v = axis_dir(a, s, 2.0); v[(a + 1) % 3] = 0.5
                o.append(c + 0.5 * np.array(p)); d.append(v)
    fams.append(_fam(tag + ":inside", o, d, 8.0, inside=True, **({"hit": True} if tag == "sphere" else {})))
    return fams


# ---------------------------------------------------------------------------------------------------------------- box
def box_families(lo, hi, tag="box"):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    mid = (lo + hi) / 2
    fams = []
    nz = -0.0
    # Q1: an axis ray through the box; the other two components +0 miss, -0 hit
    o, dp, dm, t = [], [], [], []
    for a in range(3):
        for s in (-1.0, 1.0):
            for k in (0.5, 1.0, 1.5, 2.0):
                for off in ((0, 0), (0.25, 0.25), (-0.25, 0.25), (0.25, -0.25)):
                    p = mid.copy(); p[(a + 1) % 3] += off[0]; p[(a + 2) % 3] += off[1]
                    p[a] = (lo[a] - k) if s > 0 else (hi[a] + k)
                    for mag in (1.0, 2.0):
                        o.append(p); t.append(k / mag)
                        v = np.zeros(3); v[a] = s * mag; dp.append(v.copy())
                        v[(a + 1) % 3] = nz; v[(a + 2) % 3] = nz; dm.append(v)
    fams.append(_fam(tag + ":dir+0", o, dp, 8.0, hit=False))
    n_axis = [-np.sign(v[np.flatnonzero(v)[0]]) * AXES[np.flatnonzero(v)[0]] for v in dm]
    fams.append(_fam(tag + ":dir-0", o, dm, 8.0, hit=True, t=t, n=n_axis))
    fams += with_tmax_edges(tag, o, dm, t)
    # origin on a face, moving along it with a zero component across it: 0 * inf in the slab
    o, d = [], []
    for a in range(3):
        for face in (lo[a], hi[a]):
            for z in (0.0, nz):
                for b in ((a + 1) % 3, (a + 2) % 3):
                    for s in (-1.0, 1.0):
                        for off in (0.0, 0.25):
                            p = mid.copy(); p[a] = face; p[b] += off
                            v = np.full(3, -0.5); v[a] = z; v[b] = s
                            o.append(p); d.append(v)
    fams.append(_fam(tag + ":face-origin-zero", o, d, 8.0, exact_only=True))
    # origin on a face, going in: lastin == 0, the entry hit at t == 0 with that face's normal
    o, d, n = [], [], []
    for a in range(3):
        for face, s in ((lo[a], 1.0), (hi[a], -1.0)):
            for v1 in (-0.5, 0.5):
                for v2 in (-0.5, 0.5):
                    for mag in (1.0, 2.0):
                        p = mid.copy(); p[a] = face
                        v = np.zeros(3); v[a] = s * mag; v[(a + 1) % 3] = v1; v[(a + 2) % 3] = v2
                        o.append(p); d.append(v); n.append(-s * AXES[a])
    fams.append(_fam(tag + ":face-origin-in", o, d, 8.0, hit=True, t=np.zeros(len(o)), n=n, exact_only=True))
    # origin inside: the exit hit and its normal
    o, d = [], []
    for v in _signs((1.0, 0.5, 2.0)) + _signs((0.5, 2.0, 1.0)) + _signs((2.0, 1.0, 0.5)):
        for off in (0.0, 0.25):
            o.append(mid + off); d.append(v)
    fams.append(_fam(tag + ":inside", o, d, 8.0, hit=True, inside=True))
    # onto an edge and onto a corner: equal slab entries, the normal goes to the first axis of the chain (Q6)
    for what, comps in (("edge", 2), ("corner", 3)):
        o, d, n = [], [], []
        for a in range(3):  # the axis the edge runs along (a corner: ignored)
            for sg in _signs((1.0, 1.0, 1.0)):
                for k in (1.0, 1.5, 2.0):
                    for mag in (0.5, 1.0):
                        v = -np.array(sg) * mag
                        tgt = np.where(np.array(sg) > 0, hi, lo).astype(np.float64)
                        if comps == 2:
                            tgt[a] = mid[a]; v[a] = -0.25 * sg[a] * mag
                        p = tgt - v * (k / mag)
                        first = min(j for j in range(3) if comps == 3 or j != a)
                        o.append(p); d.append(v); n.append(sg[first] * AXES[first])
        fams.append(_fam(tag + ":" + what, o, d, 8.0, hit=True, n=n, exact_only=True))
    return fams


# ---------------------------------------------------------------------------------------------------------------- cylinder / cone
def frame_of(p1, p2):
    """the frame the reference gives a cylinder / cone from p1 to p2 (Cone.hs:41-67: orth, xyz_to_uvw, translate): local -> world"""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    ln = float(np.linalg.norm(p2 - p1))
    ax1 = (p2 - p1) / ln
    ax2, ax3 = NS.orth(tuple(ax1))
    M = np.stack([np.array(ax2), np.array(ax3), ax1], 1)
    assert np.all(np.isin(np.abs(M), (0.0, 1.0))), "an axis-aligned quadric: the frame is a signed permutation"
    return M, p1, ln


def _to_world(M, T, fams):
    out = []
    for f in fams:
        e = dict(f.expect)
        if "n" in e: e["n"] = apply_linear(M, e["n"])
        out.append(Family(f.label, f32(apply_linear(M, f.o) + T), f32(apply_linear(M, f.d)), f.tmax, e))
    return out


def quadric_families(tag, r, h, r_top, height):
    """canonical frame: axis +z, base radius r at z = 0, top radius r_top at z = h (a cylinder: r_top == r; height: the cone's apex)"""
    cone = r_top != r
    fams = []
    ring = [(r, 0.0), (0.0, r), (-r, 0.0), (0.0, -r), (0.6 * r, 0.8 * r), (-0.8 * r, 0.6 * r), (0.8 * r, -0.6 * r), (-0.6 * r, -0.8 * r)]
    zs = (0.0, -0.0)
    # parallel to the axis at radius below r, equal to r and above r, from below and from above: a == 0 for a cylinder
    # (a cone has no `r==`: there the ray grazes the base's rim, and which side of `pos.z > clip1` it lands on is the last bit of a division;
    # its `r<` stays inside the top radius as well)
    for what, f in ((("r<", 0.25), ("r>", 1.25)) if cone else (("r<", 0.5), ("r==", 1.0), ("r>", 1.25))):
        o, d = [], []
        for (x, y) in ring:
            for z0, s in ((-1.0, 1.0), (-0.5, 1.0), (h + 1.0, -1.0), (h + 0.5, -1.0), (0.25 * h, 1.0), (0.25 * h, -1.0)):
                for zz in zs:
                    o.append((x * f, y * f, z0)); d.append((zz, zz, s * 2.0))
        fams.append(_fam("%s:axis-parallel:%s" % (tag, what), o, d, 8.0))
    # onto the bottom cap from below, onto the top cap from above.  The side's roots come first (Cone.hs:104-139, 155-200): the origin lies
    # outside the solid's extension beyond the cap, so the first root is where the ray enters that extension, outside the slab, and the cap
    # is asked; tmax stays beyond that root, which would reject the ray before the cap is looked at (an answer that depends on tmax, Q7).
    rt = r_top if cone else r
    for what, z0, s, rr, n in (("cap-below", -1.0, 1.0, r, (0, 0, -1.0)), ("cap-above", h + 1.0, -1.0, rt, (0, 0, 1.0))):
        if rr == 0: continue
        o, d, t = [], [], []
        for (x, y) in ring:
            for f in (0.0, 0.25, 0.5, 0.75):
                for mag in (1.0, 2.0):
                    ox, oy, tx, ty = x * 1.5 * rr / r, y * 1.5 * rr / r, x * f * rr / r, y * f * rr / r  # from 1.5 radii out, at a point of the cap
                    o.append((ox, oy, z0)); d.append(((tx - ox) * mag, (ty - oy) * mag, s * mag)); t.append(1.0 / mag)
        fams.append(_fam("%s:%s" % (tag, what), o, d, 8.0, hit=True, n=[n] * len(o), t=t))
    # Q7: a steep ray from inside misses both caps (`dz > 0 && oz < h1`, `oz > h2`); so does one that starts ON a cap's plane
    o, d = [], []
    for (x, y) in ring:
        for f in (0.0, 0.125, 0.25):
            for s in ((-1.0, -2.0) if cone else (-1.0, 1.0)):  # (up a cone the side comes first: a hit)
                for z0 in (0.25 * h, 0.5 * h):
                    o.append((x * f * rt / r, y * f * rt / r, z0)); d.append((0.25, -0.25, s * 2.0))  # (the side's root lies outside the slab and below tmax: the caps decide)
    fams.append(_fam(tag + ":q7-miss-from-inside", o, d, 8.0, hit=False))
    o, d = [], []
    for (x, y) in ring:
        for f in (0.0, 0.125, 0.25):
            for mag in (1.0, 2.0):
                for z0, s in ((0.0, 1.0), (h, -1.0)):
                    if z0 == h and rt == 0: continue
                    o.append((x * f * rt / r, y * f * rt / r, z0)); d.append((0.25 / mag, -0.25 / mag, s * 2.0))
    fams.append(_fam(tag + ":origin-on-cap-plane", o, d, 8.0, **({} if cone else {"hit": False})))  # `oz < h1` and `oz > h2` are strict; up a cone the side answers
    # origin inside, across the axis: the `t0 < 0` root
    o, d = [], []
    for (x, y) in ring:
        for z0 in (0.25 * h, 0.5 * h):
            for f in (0.0, 0.25):
                for s in (-1.0, 1.0):
                    o.append((x * f * rt / r, y * f * rt / r, z0)); d.append((s * 1.0, s * 0.5, 0.0625))
    fams.append(_fam(tag + ":inside", o, d, 8.0, hit=True, inside=True))
    if not cone:
        # tangent to the side, across the axis: disc == 0.  With a unit axis direction the Instance above divides by a length of exactly 1,
        # a == 1, and the decision is `disc < 0` on exact operands; only the depth c / qq is a division the device approximates, and the
        # depth is held to T_RTOL.  So the DECISION is exact on the device too (device_exact), and the family is kept for a quadric.
        o, d, t = [], [], []
        for a, b in ((0, 1), (1, 0)):
            for sb in (-1.0, 1.0):
                for sa in (-1.0, 1.0):
                    for k in (2.0, 2.5, 3.0, 3.5):
                        for z0 in (0.25 * h, 0.5 * h, 0.75 * h):
                            p = np.zeros(3); p[a] = -sa * k; p[b] = sb * r; p[2] = z0
                            o.append(p); d.append(axis_dir(a, sa)); t.append(k)
        fams.append(_fam(tag + ":tangent", o, d, 8.0, hit=True, exact_only=True, device_exact=True))
    # What a quadric has NOT, on any route, and why (an equality that hangs on a division cannot be held: rounding_stable moves it out):
    #   `tmax == t` and one step either side of it, on the side or on a cap -- the near root is c / qq, a division of exact values that the
    #     device approximates (no correctly rounded division there), so t lands a step beside tmax by chance; and a cap's answer depends on
    #     tmax beyond its own depth (Q7), so no tmax equals it;
    #   a cone's `through-apex` -- at the apex disc is 0 and both roots are (height - oz) / dz, a division again, and `pos.z < clip2` asks
    #     whether it came out a step short of the apex;
    #   a cone's axis-parallel `r==` -- the ray grazes the base's rim, the same question asked of `pos.z > clip1`.
    # The plain primitives have their `tmax == t` families on the routes that keep the arithmetic exact.
    return fams


# ---------------------------------------------------------------------------------------------------------------- disc / plane / triangle
def disc_families(pos, axis, r, tag="disc"):
    """a disc at pos, normal +axis"""
    pos = np.asarray(pos, np.float64)
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3
    ring = [(r, 0.0), (0.0, r), (-r, 0.0), (0.0, -r), (0.6 * r, 0.8 * r), (-0.8 * r, 0.6 * r), (0.8 * r, -0.6 * r), (-0.6 * r, -0.8 * r)]
    fams = []
    for what, f, hit in (("rim", 1.0, True), ("inside-rim", 0.5, True), ("outside-rim", 1.25, False)):  # on the rim `off . off > r2` is false: a hit
        o, d, t = [], [], []
        for (x, y) in ring:
            for s in (-1.0, 1.0):
                for k in (0.5, 1.0, 2.0):
                    v = np.zeros(3); v[a] = -s; v[b] = 0.25; v[c] = -0.5
                    tgt = pos.copy(); tgt[b] += x * f; tgt[c] += y * f
                    o.append(tgt - v * k); d.append(v); t.append(k)
        fams.append(_fam("%s:%s" % (tag, what), o, d, 8.0, hit=hit, **({"exact_only": True} if what == "rim" else {}), **({"t": t, "n": [AXES[a]] * len(o)} if hit else {})))
        if what == "inside-rim": fams += with_tmax_edges(tag, o, d, t)
    # Q2: a ray IN the disc's plane: -(0 / 0) is NaN, passes every comparison and is a hit at depth NaN
    o, d = [], []
    for (x, y) in ring:
        for f in (0.0, 0.5, 1.25, 2.0):
            for z in (0.0, -0.0):
                p = pos.copy(); p[b] += x * f; p[c] += y * f
                v = np.zeros(3); v[a] = z; v[b] = 1.0; v[c] = -0.5
                o.append(p); d.append(v)
    fams.append(_fam(tag + ":in-plane-nan", o, d, 8.0, hit=True, nan=True, exact_only=True))
    # parallel to the plane beside it: -(c / 0) is an infinity of either sign, a miss both ways
    o2 = [np.asarray(p) + AXES[a] * s for p, s in zip(o, [0.5, -0.5] * (len(o) // 2))]
    fams.append(_fam(tag + ":parallel-off-plane", o2, d, 8.0, hit=False))
    return fams


def plane_families(pt, axis, tag="plane"):
    """a plane through pt, normal +axis"""
    pt = np.asarray(pt, np.float64)
    a, b, c = axis, (axis + 1) % 3, (axis + 2) % 3
    grid = [(x, y) for x in (-3.0, -1.5, 0.0, 0.5, 2.0, 3.5) for y in (-2.5, 0.0, 1.0, 3.0)]
    fams = []
    o, d, t = [], [], []
    for (x, y) in grid:
        for s in (-1.0, 1.0):
            for k in (0.5, 2.0):
                v = np.zeros(3); v[a] = -s; v[b] = 0.5; v[c] = -0.25
                tgt = pt.copy(); tgt[b] = x; tgt[c] = y
                o.append(tgt - v * k); d.append(v); t.append(k)
    fams.append(_fam(tag + ":both-sides", o, d, 8.0, hit=True, t=t, n=[AXES[a]] * len(o)))
    fams += with_tmax_edges(tag, o, d, t)
    o, dz, dn, away = [], [], [], []
    for (x, y) in grid:
        for z in (0.0, -0.0):
            p = pt.copy(); p[b] = x; p[c] = y
            v = np.zeros(3); v[a] = z; v[b] = 1.0; v[c] = -0.5
            o.append(p); dz.append(v)
            w = v.copy(); w[a] = 1.0 if z == 0 and not np.signbit(z) else -1.0; away.append(w)
    fams.append(_fam(tag + ":in-plane-nan", o, dz, 8.0, hit=True, nan=True, exact_only=True))   # Q2
    fams.append(_fam(tag + ":origin-on-plane", o, away, 8.0, hit=True, t=np.zeros(len(o)), exact_only=True))  # -(0 / x) is a zero of either sign: not < 0
    o2 = [np.asarray(p) + AXES[a] * s for p, s in zip(o, [0.5, -1.5] * (len(o) // 2))]
    fams.append(_fam(tag + ":parallel-off-plane", o2, dz, 8.0, hit=False))
    return fams


def triangle_families(p1, p2, p3, tag="tri"):
    """a triangle in a plane of constant z (dyadic vertices); aimed at its edges, its vertices and its interior from both sides"""
    p1, p2, p3 = (np.asarray(p, np.float64) for p in (p1, p2, p3))
    assert p1[2] == p2[2] == p3[2]
    pts = {"vertex": [p1, p2, p3], "edge": [(p1 + p2) / 2, (p2 + p3) / 2, (p1 + p3) / 2, p1 * 0.75 + p2 * 0.25, p2 * 0.25 + p3 * 0.75, p1 * 0.25 + p3 * 0.75],
           "interior": [(p1 + p2) / 4 + p3 / 2, p1 / 2 + (p2 + p3) / 4, p1 / 4 + p2 / 2 + p3 / 4]}
    dirs = [(vx, vy, s) for s in (-1.0, 1.0) for vx in (0.0, -0.0, 0.5) for vy in (0.0, -0.5)]
    fams = []
    for what, targets in pts.items():
        o, d, t = [], [], []
        for tgt in targets:
            for v in dirs:
                for k in (0.5, 1.0, 2.0):
                    for mag in (1.0, 2.0):
                        if what != "edge" and mag == 2.0 and k == 2.0: continue
                        v_ = np.array(v) * mag
                        o.append(tgt - np.array(v) * k); d.append(v_); t.append(k / mag)
        # a barycentric coordinate that is exactly 0, or a sum that is exactly 1, is inside (`b1 < 0`, `b1 + b2 > 1`): the lattice keeps them exact
        fams.append(_fam("%s:%s" % (tag, what), o, d, 8.0, hit=True, t=t, **({} if what == "interior" else {"exact_only": True})))
        if what == "interior": fams += with_tmax_edges(tag, o, d, t)
    o, d = [], []
    for tgt in pts["interior"] + pts["edge"]:
        for v in ((1.0, 0.5, 0.0), (-1.0, 0.5, -0.0), (0.5, -2.0, 0.0), (2.0, 1.0, -0.0)):
            for k in (0.0, 1.0):
                o.append(tgt - np.array(v) * k); d.append(v)
    fams.append(_fam(tag + ":in-plane", o, d, 8.0, hit=False, exact_only=True))  # divisor == 0: a miss, no NaN hit (Q5)
    return fams


# ---------------------------------------------------------------------------------------------------------------- objects
def _mat(sd, k):
    return sd.material_surface((0.25 * (k + 1), 0.5, 0.75), 1, 0.25, 0.75, 0, 0)


SPHERE = ((0.0, 0.0, 0.0), 2.5)
BOX = ((-1.0, -1.5, -2.0), (1.5, 1.0, 2.0))
CYL_Z = ((0.0, 0.0, -1.0), (0.0, 0.0, 3.0), 1.25)
CYL_Y = ((0.5, -2.0, 0.0), (0.5, 2.0, 0.0), 1.25)
CONE_Z = ((0.0, 0.0, -2.0), 2.5, (0.0, 0.0, 2.0), 1.25)   # kept between radius 2.5 and radius 1.25: the apex would be at z = 6
CONE_Y = ((0.0, -2.0, 0.5), 2.5, (0.0, 2.0, 0.5), 0.0)     # ends in a point
DISC = ((0.0, 0.0, 0.5), 2, 2.5)                            # position, normal axis, radius
PLANE = ((0.0, 0.5, 0.0), 1)
TRI = ((-2.0, -1.0, 0.5), (2.0, -1.0, 0.5), (0.0, 3.0, 0.5))
TIE = ((0.0, 0.0, 0.5), (0.5, 0.0, 0.5))                    # two coplanar discs of radius 2.5: every ray meets both at one depth


def _quadric(spec, cone):
    p1, p2 = (spec[0], spec[2]) if cone else (spec[0], spec[1])
    M, T, ln = frame_of(p1, p2)
    r = spec[1] if cone else spec[2]
    r_top = spec[3] if cone else r
    height = r * ln / (r - r_top) if cone else 0.0
    return M, T, quadric_families("cone" if cone else "cyl", r, ln, r_top, height)


def _q_fams(spec, cone, tag):
    M, T, fams = _quadric(spec, cone)
    return [f._replace(label=tag + f.label[f.label.index(":"):]) for f in _to_world(M, T, fams)]


def _csg_families(tag, targets):
    """rays aimed at dyadic points of a CSG solid's surface or of the cut, from outside and from inside"""
    o, d = [], []
    for tgt in targets:
        for v in _signs((0.5, 1.0, 2.0)) + _signs((1.0, -0.0, 0.0)) + _signs((0.0, 2.0, -0.0)) + _signs((-0.0, 0.0, 0.5)):
            for k in (1.0, 2.0):
                o.append(np.asarray(tgt, np.float64) - np.array(v) * k); d.append(v)
    return [_fam(tag + ":aimed", o, d, 8.0)]


def _tie_families():
    f = disc_families(TIE[0], 2, 2.5, tag="tie")
    both = [x for x in f if x.label in ("tie:inside-rim",)]  # rays that meet both discs (the second is half a unit along x: the inner ring is inside it too)
    return [Family("tie:nearest-takes-the-later", x.o, x.d, x.tmax, dict(x.expect, prim="second")) for x in both] + f[1:4]


def _no_expect(fams):
    """the same rays with nothing stated about the answers (the object is not the plain primitive the family was written for)"""
    return [f._replace(expect={"exact_only": True} if f.expect.get("exact_only") else {}) for f in fams]


def _objects():
    def sphere(sd): return sd.sphere(*SPHERE), {}
    def box(sd): return sd.box(*BOX), {}
    def cyl_z(sd): return sd.cylinder(*CYL_Z), {}
    def cyl_y(sd): return sd.cylinder(*CYL_Y), {}
    def cone_z(sd): return sd.cone(*CONE_Z), {}
    def cone_y(sd): return sd.cone(*CONE_Y), {}
    def disc(sd): return sd.disc(DISC[0], AXES[DISC[1]], DISC[2]), {}
    def plane(sd): return sd.plane(PLANE[0], AXES[PLANE[1]]), {}
    def triangle(sd): return sd.triangle(*TRI), {}
    def trianglenorm(sd): return sd.trianglenorm(*TRI, (0.0, 0.0, 1.0), (0.5, 0.0, 1.0), (0.0, -0.5, 1.0)), {}
    def difference(sd): return sd.difference(sd.sphere(*SPHERE), sd.sphere((0.0, 0.0, 2.0), 1.5)), {}

    def difference_retexture(sd):
        return sd.difference_retexture(sd.tex(sd.sphere(*SPHERE), _mat(sd, 0)), sd.tex(sd.box((0.0, -1.0, -1.0), (3.0, 1.0, 1.0)), _mat(sd, 1))), {}

    def intersection3(sd):  # the solid of the issue's crash ray
        return sd.intersection([sd.sphere((0.0, 0.0, 0.0), 2.0), sd.box((-1.0, -1.0, -3.0), (1.0, 1.0, 3.0)), sd.plane_offset((0.0, 1.0, 0.0), 0.5)]), {}

    def intersection7(sd):  # a sphere cut by six planes: a cube with rounded corners
        planes = [sd.plane_offset(tuple(float(s) * AXES[a]), 1.25) for a in range(3) for s in (1, -1)]  # (off the lattice: intersection3 has the origins ON a face)
        return sd.intersection([sd.sphere((0.0, 0.0, 0.0), 2.0)] + planes), {}

    def bound(sd): return sd.bound_object(sd.sphere((0.0, 0.0, 0.0), 3.0), sd.box(*BOX)), {}
    def innerbound(sd): return sd.innerbound(sd.sphere((0.0, 0.0, 0.0), 3.0), sd.box(*BOX)), {}
    def noshadow(sd): return sd.noshadow(sd.sphere(*SPHERE)), {}
    def onlyshadow(sd): return sd.onlyshadow(sd.box(*BOX)), {}

    def tie(sd):
        a, b = sd.disc(TIE[0], AXES[2], 2.5), sd.disc(TIE[1], AXES[2], 2.5)
        return sd.group([a, b]), {"second": b}

    def spheres(sd):  # a bih of spheres only
        cs = [SPHERE[0] + (1.25,), (2.5, 2.5, -2.5, 0.625), (-3.0, 1.0, 2.0, 0.5), (-2.0, -3.0, -1.0, 1.0), (3.0, -2.0, 1.5, 0.75), (0.5, 3.0, 3.0, 0.5), (-3.5, 3.5, -3.5, 0.25)]
        return sd.bih([sd.sphere(c[:3], c[3]) for c in cs]), {}

    simple = ("alone", "list", "bih_simple", "instance", "instance_bih", "generic")
    composite = ("alone", "list", "instance", "instance_bih", "generic")
    return [
        Obj("sphere", sphere, lambda: sphere_families(*SPHERE), simple),
        Obj("box", box, lambda: box_families(*BOX), simple),
        Obj("cyl_z", cyl_z, lambda: _q_fams(CYL_Z, False, "cyl_z"), composite),
        Obj("cyl_y", cyl_y, lambda: _q_fams(CYL_Y, False, "cyl_y"), composite),
        Obj("cone_z", cone_z, lambda: _q_fams(CONE_Z, True, "cone_z"), composite),
        Obj("cone_y", cone_y, lambda: _q_fams(CONE_Y, True, "cone_y"), composite),
        Obj("disc", disc, lambda: disc_families(*DISC), simple),
        Obj("plane", plane, lambda: plane_families(*PLANE), ("alone", "list", "instance", "generic")),  # (unbounded: no bih holds it)
        # (a transformed triangle is a new triangle, Triangle.hs: no Instance is made, so no `instance` route holds one)
        Obj("triangle", triangle, lambda: triangle_families(*TRI), ("alone", "list", "bih_simple", "generic", "bih_tri", "mesh")),
        Obj("trianglenorm", trianglenorm, lambda: triangle_families(*TRI, tag="trin"), ("alone", "list", "bih_simple", "generic")),
        Obj("difference", difference, lambda: _csg_families("diff", [(0.0, 0.0, 0.5), (0.0, 0.0, -2.5), (1.5, 0.0, 2.0), (0.0, 1.5, 2.0), (2.5, 0.0, 0.0)]), composite),
        Obj("difference_retexture", difference_retexture, lambda: _csg_families("diffre", [(0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (2.5, 0.0, 0.0), (-2.5, 0.0, 0.0), (1.0, -1.0, 0.5)]), composite),
        # (with the box's own face-origin family: origins on its faces with a zero component across, the class of the ray whose advance is NaN)
        Obj("intersection3", intersection3, lambda: _csg_families("isect3", [(1.0, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, -1.0, 1.0), (-1.0, 0.5, 1.0), (0.0, 0.0, 2.0)]) +
            [f._replace(expect={}) for f in box_families((-1.0, -1.0, -3.0), (1.0, 1.0, 3.0), tag="isect3:box") if f.label.endswith("face-origin-zero")], composite),
        Obj("intersection7", intersection7, lambda: _csg_families("isect7", [(1.0, 0.0, 0.0), (0.0, -1.0, 0.5), (1.0, 1.0, 0.0), (0.0, 0.0, -1.0), (0.5, 1.0, 0.5)]), composite),
        # (a Bound always leaves the flat tier: each of its routes is the interpreter's)
        Obj("bound", bound, lambda: _no_expect(box_families(*BOX, tag="bound")), ("alone", "list", "instance")),
        Obj("innerbound", innerbound, lambda: _no_expect(box_families(*BOX, tag="inner")), ("alone", "list", "instance")),
        Obj("noshadow", noshadow, lambda: sphere_families(*SPHERE, tag="noshadow"), simple),
        Obj("onlyshadow", onlyshadow, lambda: _no_expect(box_families(*BOX, tag="onlyshadow")), simple),
        Obj("tie", tie, _tie_families, ("alone", "list")),
        Obj("spheres", spheres, lambda: sphere_families(SPHERE[0], 1.25, tag="spheres"), ("bih_sphere",)),
    ]


OBJECTS = {o.name: o for o in _objects()}

# ---------------------------------------------------------------------------------------------------------------- routes
# name -> (tier, bits of the commit's cls_mask that must be set, bits that must not be): rt_types.h CLS_*
CLS_BIH_TRI, CLS_BIH_SPHERE, CLS_BIH_SIMPLE, CLS_MESH, CLS_PRIMS, CLS_CSG = 1, 2, 4, 8, 16, 32
FAR = ((3.5, 3.5, -3.5), 0.25)  # the small far sphere beside a list item
# exact matrices: an axis permutation through xyz_to_uvw, a scale by 2 / 0.5 per axis, a dyadic translation
XFM_INSTANCE = lambda: [api.xyz_to_uvw((0, 1, 0), (0, 0, 1), (1, 0, 0)), api.scale((2.0, 0.5, 1.0)), api.translate((0.5, -0.25, 0.25))]
XFM_GENERIC = lambda: [api.translate((0.25, 0.5, -0.5))]


def _matrix(xfms):
    """the composed 3 x 4 forward matrix of a list of transforms (exact: every entry dyadic)"""
    m = np.asarray(api.compose(xfms), np.float64).ravel()[:12].reshape(3, 4)
    assert np.array_equal(m * 64, np.round(m * 64)), m
    return m


def _fillers(sd):
    """simple primitives far in the corners: with the object they make a bih of mixed simple primitives"""
    return [sd.sphere((-3.5, -3.5, 3.5), 0.25), sd.box((3.0, -4.0, -4.0), (3.5, -3.5, -3.5)), sd.triangle((-4.0, 3.0, 3.5), (-3.0, 3.0, 3.5), (-3.5, 4.0, 3.5)),
            sd.disc((3.5, 3.5, 3.5), (0.0, 1.0, 0.0), 0.25)]


def _tri_set():
    """the triangles of the bih_tri / mesh routes: TRI first, ALONE -- no other triangle shares a vertex or an edge with it or lies in its
    plane, so a ray aimed at TRI's edge or vertex meets TRI only, whose divisor is a power of two (-16 dz): the equality families stay exact
    in the tree as they are on the triangle alone.  Around it a fan of dyadic triangles below and three above, sharing edges among themselves."""
    v = [TRI[0], TRI[1], TRI[2], (-3.0, -3.0, -1.0), (3.0, -3.0, -1.5), (3.0, 3.0, -1.0), (-3.0, 3.0, -2.0), (0.0, 0.0, -3.0), (-3.5, 0.0, 2.0), (3.5, 0.5, 2.5), (0.0, -3.5, 3.0),
         (-3.5, -3.5, 2.5), (3.5, -3.0, 2.0), (0.5, 3.5, 3.0)]
    idx = [(0, 1, 2), (3, 4, 7), (4, 5, 7), (5, 6, 7), (6, 3, 7), (8, 11, 10), (10, 12, 9), (9, 13, 8), (3, 4, 10), (5, 6, 9), (6, 8, 3), (4, 9, 5)]
    assert not any(set(t) & {0, 1, 2} for t in idx[1:])
    return np.array(v, np.float64), idx


def build_scene(name, route):
    """(SceneDesc, the object's node, its named parts, the 3 x 4 matrix that places the object's own frame in the scene)"""
    obj = OBJECTS[name]
    assert route in obj.routes, (name, route)
    sd = SceneDesc()
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    M = eye
    if route in ("bih_tri", "mesh"):
        v, idx = _tri_set()
        if route == "bih_tri":
            ids = [sd.triangle(*(tuple(v[i]) for i in t)) for t in idx]
            node, root = ids[0], sd.bih(ids)
        else:
            node = root = sd.mesh(v, [], [list(t) + [-1] * 5 for t in idx], [])
        parts = {}
    else:
        node, parts = obj.build(sd)
        far = lambda: sd.sphere(*FAR)
        if route in ("alone", "bih_sphere"): root = node
        elif route == "list": root = sd.group([node, far()])
        elif route == "bih_simple": root = sd.bih([node] + _fillers(sd))
        elif route == "instance":
            M = _matrix(XFM_INSTANCE()); root = sd.group([sd.transform(node, XFM_INSTANCE()), far()])
        elif route == "instance_bih":
            M = _matrix(XFM_INSTANCE()); root = sd.bih([sd.transform(node, XFM_INSTANCE())] + _fillers(sd))
        elif route == "generic":
            M = _matrix(XFM_GENERIC()); root = sd.group([sd.transform(sd.group([node, far()]), XFM_GENERIC()), sd.sphere((-3.5, 3.5, -3.5), 0.25)])
        else: raise KeyError(route)
    sd.set_root(root)
    sd.set_camera((0.0, 0.0, -8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0)
    return sd, node, parts, M


def route_traits(name, route):
    """what the commit's own traits must say for this object on this route (checked by tests/test_lattice_host.py): the tier, bits of
    cls_mask that must be set and bits that must be clear, and the class of the trace instance a production launch at maxdepth 1 gets"""
    simple = "bih_simple" in OBJECTS[name].routes or name in ("plane", "tie")
    bihs = CLS_BIH_TRI | CLS_BIH_SPHERE | CLS_BIH_SIMPLE | CLS_MESH
    if route == "generic" or name in ("bound", "innerbound"): return dict(tier=1, trace="k_trace_batch_generic<lean>")
    if route in ("alone", "list"):
        if simple: return dict(tier=0, has=CLS_PRIMS, hasnot=bihs | CLS_CSG, trace="k_trace_batch_flat<false,false,false,SPHERE|PRIMS,1>")
        return dict(tier=0, has=CLS_CSG, hasnot=bihs, trace="k_trace_batch_flat<false,false,false,CSG|PRIMS,2>")
    return {"bih_simple": dict(tier=0, has=CLS_BIH_SIMPLE, hasnot=63 & ~CLS_BIH_SIMPLE, trace="k_trace_batch_flat<false,false,false,ALL,1>"),
            "instance": dict(tier=0, has=CLS_CSG, hasnot=bihs, trace="k_trace_batch_flat<false,false,false,CSG|PRIMS,2>"),
            "instance_bih": dict(tier=0, has=CLS_CSG, hasnot=bihs | CLS_PRIMS, trace="k_trace_batch_flat<false,false,false,CSG|PRIMS,2>"),
            "bih_sphere": dict(tier=0, has=CLS_BIH_SPHERE, hasnot=63 & ~CLS_BIH_SPHERE, trace="k_trace_batch_flat<false,false,false,SPHERE|PRIMS,1>"),
            "bih_tri": dict(tier=0, has=CLS_BIH_TRI, hasnot=63 & ~CLS_BIH_TRI, trace="k_trace_batch_flat<false,false,false,TRI,1>"),
            "mesh": dict(tier=0, has=CLS_MESH, hasnot=63 & ~CLS_MESH, trace="k_trace_batch_flat<false,false,false,MESH,1>")}[route]


CASES = [(o.name, r) for o in OBJECTS.values() for r in o.routes]


# ---------------------------------------------------------------------------------------------------------------- rays
OFF_LATTICE = (1.0 / 64, 3.0 / 64, 5.0 / 64)


def lattice_rays(n, seed, n_plain=None):
    """n rays: the first n_plain (all of them by default) with origins on the half-integer lattice, the others (labels `lattice+`) with
    the origins moved off it by (1, 3, 5) / 64, which no plane of any object contains and from which no slope of {1/4 .. 4} leads to an edge."""
    n_plain = n if n_plain is None else n_plain
    rng = np.random.default_rng(seed)
    o = rng.integers(-8, 9, size=(n, 3)) * 0.5
    o[n_plain:] += np.array(OFF_LATTICE)
    o = o.astype(np.float32)
    d = DIR_VALUES[rng.integers(0, len(DIR_VALUES), size=(n, 3))]
    zero = np.all(d == 0, axis=1)
    d[zero, 0] = np.float32(1.0)  # (the zero vector is left out)
    tmax = (rng.integers(1, 17, size=n) * 0.5).astype(np.float32)
    nzero = (d == 0).sum(1)
    labels = np.array(["lattice:%d-zero-components" % k for k in range(3)] + ["lattice+:%d-zero-components" % k for k in range(3)])[nzero + 3 * (np.arange(n) >= n_plain)]
    return o, d, tmax, labels


def split_plane_family(sd, node):
    """origins ON the split planes of a bih's first branches, with a zero component across the plane"""
    o_, om, _ = O.load_scene(sd)
    ls, rs, ax, nl, _ = o_.bih_dump(om[node])
    o, d = [], []
    for k in np.flatnonzero(ax >= 0)[:4]:
        for split in (ls[k], rs[k]):
            a = int(ax[k])
            for z in (0.0, -0.0):
                for u in (-2.0, -0.5, 0.0, 1.0):
                    for v in ((1.0, 0.5), (-1.0, 2.0), (0.5, -1.0)):
                        p = np.full(3, u); p[a] = split
                        w = np.zeros(3); w[a] = z; w[(a + 1) % 3] = v[0]; w[(a + 2) % 3] = v[1]
                        o.append(p); d.append(w)
    return _fam("bih:origin-on-split-plane", o, d, 8.0)


QUADRICS = ("cyl_z", "cyl_y", "cone_z", "cone_y")
# objects whose own arithmetic is inexact whatever the ray: a quadric divides twice by computed values (`qq / a`, `c / qq`) and takes a root; a CSG
# solid advances by delta = 1e-4, which is no dyadic number, and asks its parts about the advanced ray
INEXACT = QUADRICS + ("difference", "difference_retexture", "intersection3", "intersection7")
ULPS = 4  # the size of the nudges of rounding_stable, in fp32 steps


def inexact(name, route):
    """is the arithmetic inexact whatever the ray?  In the objects of INEXACT; and in the trees of many triangles (bih_tri, mesh), whose
    triangles beside TRI divide by divisors that are no powers of two (`1.0f / divisor`, tri_test: v_rcp_f32 on the device), so that which
    of two triangles that share an edge answers a ray through that edge is the last bit of a reciprocal"""
    return name in INEXACT or route in ("bih_tri", "mesh")


def has_instance(name, route):
    """does a ray meet an Instance on the way to the object?  Instance (Solid.hs:388-403) hands the solid below it the direction divided by
    its length: a sqrt and a division, v_sqrt_f32 and v_rcp_f32 on the device, exact only where the length is exactly 1"""
    return route in ("instance", "instance_bih", "generic") or name in QUADRICS


def exact_rays(name, route, d, A):
    """the rays whose arithmetic is exact on the device as on the host: every direction component a zero or a power of two, so that
    v_rcp_f32 of it is exact -- and, below an Instance, a direction that is a unit axis vector in the Instance's frame, so that the length
    it divides by is exactly 1.  Every other case hangs on how an inexact reciprocal or square root rounds: see rounding_stable."""
    d = np.asarray(d, np.float64)
    m, _ = np.frexp(np.abs(d))
    dyadic = np.all((d == 0) | (m == 0.5), axis=1)
    if not has_instance(name, route): return dyadic
    local = apply_linear(np.linalg.inv(A), d)
    return dyadic & ((local != 0).sum(1) == 1) & (np.abs(local).max(1) == 1.0)


def bounds_face_family(sd, node):
    """origins ON a face of a bih's bounds with a -0 component across it: bbclip_ub's `near` is 0 * -inf = NaN (Q1), and a ray whose near is
    NaN enters no near child on its whole way down (`fmax t2 near` keeps the NaN, Bih.hs:332-368) -- in every walk, the packet walks included.
    The other two coordinates are off the lattice by 3 / 64 and 5 / 64, so that no ray meets an edge of an item exactly: the family is about
    the NaN, which is exact on every route."""
    o_, om, _ = O.load_scene(sd)
    bb = o_.bound(om[node])
    lo, hi = bb[:3], bb[3:]
    o, d = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for face in (lo[a], hi[a]):
            for fu in (0.25, 0.625):
                for fv in (0.375, 0.75):
                    for v in ((1.0, 0.5), (-1.0, 2.0), (0.5, -1.0), (-2.0, -0.5)):
                        p = np.zeros(3); p[a] = face
                        p[b] = np.round((lo[b] + fu * (hi[b] - lo[b])) * 2) / 2 + 3.0 / 64; p[c] = np.round((lo[c] + fv * (hi[c] - lo[c])) * 2) / 2 + 5.0 / 64
                        w = np.zeros(3); w[a] = -0.0; w[b] = v[0]; w[c] = v[1]
                        o.append(p); d.append(w)
    return _fam("bih:origin-on-bounds-face", o, d, 8.0, exact_only=True)


Rays = namedtuple("Rays", "o d tmax labels exact trusted expect")  # exact: the ray is as written (not renormalised); trusted: of a family whose arithmetic is exact by construction; expect: [(label, slice, dict)]


@functools.lru_cache(maxsize=None)
def rays_for(name, route):
    """the rays of an object on a route, in the scene's frame: the lattice, then every aimed family as written and normalised in fp32"""
    sd, node, parts, M = build_scene(name, route)
    fams = list(OBJECTS[name].families())
    if route in ("bih_simple", "instance_bih", "bih_sphere", "bih_tri"):
        root_bih = sd.root
        fams.append(split_plane_family(sd, root_bih))
        fams.append(bounds_face_family(sd, root_bih))
    if has_instance(name, route) or inexact(name, route):
        lo, ld, lt, ll = lattice_rays(N_LATTICE_INEXACT, seed=sum(map(ord, name)), n_plain=N_PLAIN_INEXACT)
    else:
        lo, ld, lt, ll = lattice_rays(N_LATTICE, seed=sum(map(ord, name)))
    os_, ds_, ts_, labels, exact, trusted, expect = [lo], [ld], [lt], [ll], [np.ones(len(lo), bool)], [np.zeros(len(lo), bool)], []
    at = len(lo)
    A, T = M[:, :3], M[:, 3]
    for f in fams:
        own = f.label.startswith("bih:")  # (already in the scene's frame, and about the tree, not about what is in it)
        o = f.o if own else f32(apply_linear(A, f.o) + T)
        d = f.d if own else f32(apply_linear(A, f.d))
        assert own or (np.array_equal(o.astype(np.float64), apply_linear(A, f.o) + T) and np.array_equal(np.signbit(d), np.signbit(apply_linear(A, f.d)))), "the route's matrix keeps the lattice exact"
        tmax_f = f.tmax
        if f.expect.get("exact_only") and name in INEXACT and not f.expect.get("device_exact"): continue
        if f.expect.get("exact_only") and has_instance(name, route) and not own:
            # a family aimed at an exact equality keeps the rays whose arithmetic stays exact below the Instance; where too few do, this
            # route has no such family (the other routes of the object have it)
            ok = exact_rays(name, route, d, A)
            if ok.sum() < MIN_PER_LABEL + 8: continue
            o, d, tmax_f = o[ok], d[ok], f.tmax[ok]
            f = f._replace(expect={k: (np.asarray(v)[ok] if k in ("t", "n") else v) for k, v in f.expect.items()})
        ln = np.sqrt((d.astype(np.float64) ** 2).sum(1))
        du = f32(d / ln[:, None]); du = f32(du / np.sqrt((du.astype(np.float64) ** 2).sum(1))[:, None])
        du = np.where(d == 0, d, du)  # (a signed zero stays the zero it was)
        e = dict(f.expect)
        if "n" in e:
            nn = apply_linear(np.linalg.inv(A).T, e["n"])  # normals go with the inverse transpose
            e["n"] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
        # (a family aimed at an exact equality -- exact_only -- has no normalised twin: normalising breaks the equality it is about)
        for lab, dd, tt, ex in ((f.label, d, tmax_f, True), (f.label + "/unit", du, f32(tmax_f.astype(np.float64) * ln), False))[:1 if e.get("exact_only") else 2]:
            os_.append(o); ds_.append(dd); ts_.append(tt); labels.append(np.full(len(o), lab)); exact.append(np.full(len(o), ex)); trusted.append(np.full(len(o), bool(e.get("exact_only"))))
            expect.append((lab, slice(at, at + len(o)), e, ex))
            at += len(o)
    r = Rays(np.ascontiguousarray(np.concatenate(os_)), np.ascontiguousarray(np.concatenate(ds_)), np.concatenate(ts_), np.concatenate(labels), np.concatenate(exact), np.concatenate(trusted), expect)
    assert r.o.dtype == np.float32 and r.d.dtype == np.float32 and len(r.o) <= 20000, (name, route, len(r.o))
    return r


def unit_length(d):
    """rt_device.hpp unit_length, in fp32 like the device"""
    d = f32(d)
    dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return (dd > np.float32(0.99999)) & (dd < np.float32(1.00001))


# ---------------------------------------------------------------------------------------------------------------- evaluation
def _ids(pr, back):
    """a backend's primitive ids as description ids (-1 a miss, -2 a primitive made inside the backend)"""
    inv = np.full(max(max(back) + 2, int(pr.max()) + 2), -2); inv[np.asarray(back)] = np.arange(len(back))
    return np.where(pr < 0, -1, inv[np.maximum(pr, 0)])


def hit_of(t):
    return ~(np.asarray(t) < 0)  # (a miss is -1; a NaN depth is a hit, Q2)


def hostsim_answers(hs, o, d, tmax):
    """the host build's rayint and shadow ray by ray where a batch reports a limit (one status per batch): (rayint dict, shadow, over_limit)"""
    n = len(o)
    over = np.zeros(n, bool)
    ri = {"t": np.full(n, -1, np.float32), "prim": np.full(n, -1, np.int32), "n": np.zeros((n, 3), np.float32), "tex": np.full((n, 8), -1, np.int32)}
    sh = np.zeros(n, bool)

    def run(idx):
        try:
            r = hs.rayint(o[idx], d[idx], tmax[idx]); s = hs.shadow(o[idx], d[idx], tmax[idx])
        except RuntimeError:
            if len(idx) == 1: over[idx] = True; return
            run(idx[:len(idx) // 2]); run(idx[len(idx) // 2:]); return
        for k in ri: ri[k][idx] = r[k]
        sh[idx] = s
    for a in range(0, n, 512):  # (a ray over the limit costs 2^20 advances each time it is run: small batches keep the halving short)
        run(np.arange(a, min(n, a + 512)))
    return ri, sh, over


def rounding_stable(hs, nm, o, d, tmax, base, base_shadow, keep_axis=None):
    """Section "what the tests find" of the issue, the third kind: a case whose decision hangs on how an inexact operation rounds -- a
    division or a square root of values that are exact on the lattice, which the device approximates (v_rcp_f32, v_sqrt_f32, and a * b + c
    contracted) and the host rounds correctly -- is held by the three CPU evaluations only by luck.  Such a case is moved out of the agreement
    set by a rule, not by a list: the host build must decide alike -- hit / miss, primitive, face (the normal), shadow -- on twelve nudged
    copies of the ray: every direction component and tmax moved by ULPS fp32 steps, every origin coordinate by ULPS steps of the scene's
    size (4), signs drawn from a fixed seed.  A zero direction component stays the zero it is.  keep_axis: the origin coordinate left alone --
    along a quadric's axis, where the cap tests `oz < h1` and `oz > h2` read the origin itself and are exact.  Returns the stable rays."""
    stable = np.ones(len(o), bool)
    e = np.float32(ULPS * 2.0 ** -23)
    rng = np.random.default_rng(20261019)
    bh, bid, bn = hit_of(base["t"]), _ids(base["prim"], nm), base["n"].astype(np.float64)
    for _ in range(12):
        so, sd, st = (f32(rng.choice([-1.0, 1.0], size=sh)) for sh in ((len(o), 3), (len(o), 3), (len(o),)))
        if keep_axis is not None: so[:, keep_axis] = 0
        oo, dd, tt = f32(o + so * e * np.float32(4)), f32(d * (np.float32(1) + e * sd)), f32(tmax * (np.float32(1) + e * st))
        r, sh, over = hostsim_answers(hs, oo, dd, tt)
        with np.errstate(invalid="ignore"):
            face = ~(np.abs(r["n"].astype(np.float64) - bn).max(axis=1) > NORMAL_TOL) | ~bh
        stable &= ~over & (hit_of(r["t"]) == bh) & (_ids(r["prim"], nm) == bid) & (sh == base_shadow) & face
    return stable


Eval = namedtuple("Eval", "key rays sd nm ref f32_ hs hs_shadow hs_inside ref_shadow ref_inside prim_ref agree flagged why")


@functools.lru_cache(maxsize=None)
def evaluate(name, route):
    """the three CPU evaluations of every case of an object on a route, and the agreement set"""
    rays = rays_for(name, route)
    sd, node, parts, M = build_scene(name, route)
    o, d, tm = rays.o, rays.d, rays.tmax
    o64, d64, t64 = o.astype(np.float64), d.astype(np.float64), tm.astype(np.float64)
    res = []
    for fl in (False, True):
        orc, om, _ = O.load_scene(sd, use_float=fl)
        r = orc.rayint(om[sd.root], o64, d64, t64)
        r["shadow"] = orc.shadow(om[sd.root], o64, d64, t64); r["diverged"] = r["diverged"] | orc.last_diverged
        r["inside"] = orc.inside(om[sd.root], o64)
        r["id"] = _ids(r["prim"], om)
        res.append(r)
    ref, r32 = res
    flagged = ref["diverged"] | r32["diverged"]
    b = api.Builder()
    nm, _ = sd.replay(b)
    hs = HostSim(b, nm[sd.root])
    keep = np.flatnonzero(~flagged)  # (a ray the oracle gave up takes the runaway path of the device headers: test_lattice_host runs a handful of them, once)
    hri, hsh, over = hostsim_answers(hs, o[keep], d[keep], tm[keep])
    n = len(o)
    h = {"t": np.full(n, -1, np.float32), "prim": np.full(n, -1, np.int32), "n": np.zeros((n, 3), np.float32), "tex": np.full((n, 8), -1, np.int32)}
    for k in h: h[k][keep] = hri[k]
    hshadow = np.zeros(n, bool); hshadow[keep] = hsh
    flagged = flagged.copy(); flagged[keep] |= over
    hinside = hs.inside(o)
    h["id"] = _ids(h["prim"], nm)
    why = {}
    agree = ~flagged
    why["flagged"] = flagged
    # trusted as exact: the families written to be, and on an object whose own arithmetic is exact the rays that stay exact on this route
    sure = rays.trusted | (exact_rays(name, route, d, M[:, :3]) & (not inexact(name, route)))
    fragile = np.flatnonzero(~sure & ~flagged)
    unstable = np.zeros(n, bool)
    if len(fragile):
        axis = None
        if name in QUADRICS:  # the quadric's axis in this scene: y or z in its own frame, then through the route's matrix
            ax = np.zeros(3); ax[1 if name.endswith("_y") else 2] = 1.0
            axis = int(np.flatnonzero(apply_linear(M[:, :3], ax)[0])[0])
        unstable[fragile] = ~rounding_stable(hs, nm, o[fragile], d[fragile], tm[fragile], {k: v[fragile] for k, v in h.items()}, hshadow[fragile], axis)
    for key, bad in (("hit/miss", (hit_of(ref["t"]) != hit_of(r32["t"])) | (hit_of(ref["t"]) != hit_of(h["t"]))),
                     ("primitive", (ref["id"] != r32["id"]) | (ref["id"] != h["id"])),
                     ("texture", np.any(ref["tex"] != r32["tex"], axis=1) | np.any(ref["tex"] != h["tex"], axis=1)),
                     ("shadow", (ref["shadow"] != r32["shadow"]) | (ref["shadow"] != hshadow)),
                     ("inside", (ref["inside"] != r32["inside"]) | (ref["inside"] != hinside)),
                     ("depth", ~depth_ok(r32["t"], ref["t"]) | ~depth_ok(h["t"], ref["t"])),
                     # stricter than the decisions alone: a ray onto the rim between a cap and the side hits at one depth whichever of the two
                     # answers, and which one does hangs on the last bit of sqrt(disc) -- the three must name one face
                     ("normal", ~normal_ok(r32["n"], ref)),
                     ("rounding", unstable)):
        why[key] = bad & agree
        agree = agree & ~bad
    return Eval((name, route), rays, sd, nm, ref, r32, h, hshadow, hinside, ref["shadow"], ref["inside"], ref["id"], agree, flagged, why)


def depth_ok(t, ref):
    """both miss, both NaN (Q2: a decision), or within parity.T_RTOL of the fp64 depth"""
    t, ref = np.asarray(t, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        close = np.abs(t - ref) <= parity.T_RTOL * np.maximum(1.0, np.abs(ref))
    return np.where(np.isnan(ref) | np.isnan(t), np.isnan(ref) & np.isnan(t), close | ((ref < 0) & (t < 0)))


def normal_ok(n, ref):
    """within NORMAL_TOL of the fp64 normal wherever the fp64 oracle hits with a finite normal"""
    hit = hit_of(ref["t"]) & np.all(np.isfinite(ref["n"]), axis=1)
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(n, np.float64) - ref["n"]).max(axis=1)
    return ~hit | (err <= NORMAL_TOL)


def check_backend(ev, got, shadow=None, inside=None, nm=None, what="", sel=None):
    """EVERY case of the agreement set (of `sel`, an index array into the rays, when the backend was given a subset): the oracle's
    decision, the fp64 depth within T_RTOL (NaN where the oracle's is NaN), the normal within NORMAL_TOL.  Returns the number held."""
    sel = np.arange(len(ev.agree)) if sel is None else np.asarray(sel)
    a = ev.agree[sel]
    ref = ev.ref
    lab = ev.rays.labels[sel]

    def none(bad, msg):
        bad = bad & a
        assert not bad.any(), "%s %s: %d cases of the agreement set, e.g. %s" % (what, msg, int(bad.sum()), [
            (str(lab[i]), ev.rays.o[sel[i]].tolist(), ev.rays.d[sel[i]].tolist(), float(ev.rays.tmax[sel[i]]), float(got["t"][i]), float(ref["t"][sel[i]])) for i in np.flatnonzero(bad)[:4]])
    none(hit_of(got["t"]) != hit_of(ref["t"][sel]), "hit / miss")
    none(~depth_ok(got["t"], ref["t"][sel]), "depth")
    none(_ids(got["prim"], ev.nm if nm is None else nm) != ev.prim_ref[sel], "primitive")
    none(np.any(got["tex"] != ref["tex"][sel], axis=1), "texture stack")
    hit = hit_of(ref["t"][sel]) & np.all(np.isfinite(ref["n"][sel]), axis=1)
    with np.errstate(invalid="ignore"):
        nerr = np.abs(got["n"].astype(np.float64) - ref["n"][sel]).max(axis=1)
    none(hit & ~(nerr <= NORMAL_TOL), "normal")
    if shadow is not None: none(np.asarray(shadow) != ev.ref_shadow[sel], "shadow")
    if inside is not None: none(np.asarray(inside) != ev.ref_inside[sel], "inside")
    return int(a.sum())
