"""Frame towers: scenes that hold the generic tier's frame memory to the estimate commit makes of it (TEST INFRASTRUCTURE).

A plain module (no GPU, no fixtures) shared by tests/test_frame_words_host.py and tests/test_frame_words_gpu.py.

A TOWER is L levels of one composite KIND over one BOTTOM.  A level pairs the kind with a list -- `group [kind(x), side_k]`, x the levels
below -- so that every level has an object of its own beside the way down (side_k, a small sphere), and the builder has no two lists to
merge.  Everything is dyadic, as in tests/lattice.py: centres on multiples of 1 / 4, radii powers of two, the only transform a translation
by 2^-7 along z (up on even levels, down on odd ones), rays along z or a hair off it.  So every decision is far from its edge, and the families' depths are short sums.

  KINDS     xform        group [transform x]                         an Instance frame and a list frame per level
            inst2        transform (transform x)                     Instance on Instance: one Instance to the builder, which composes them (not in KINDS)
            innerbound   innerbound x (sphere 3)                     IB_R live over the way down
            bound_prim   bound_object (sphere 3.5) x                 the Bound frame is gone when x runs
            bound_comp   bound_object (group [sphere 3.5, far]) x    the same with `inside` and `shadow` of the bounding solid over frames
            bound_deep   bound_object x (sphere 1)                   the tower IS the bounding solid: BOUND_R / BOUND_S live over a deep shadow call
            diff         difference x (group [far, far])             a Difference frame per level, no advance
            diff_retex   difference_retexture x (group [far, far])
            isect        intersection [x, group [sphere 3.5, far]]   an Intersection frame per level, no advance
            bih          bih [x, group .., group ..]                 a bih of three composite items
            warp_frame, warp_scene   a disc before a group [transform] tower, textured with a Warp material whose frame / scene is the tower:
                                     the root is shallow, the tower is reached from the shader alone (the trace route, maxdepth >= 2)
  BOTTOMS   sphere, sphere_bih, tri_bih, inst_bih (a bih of Instances of primitives), mesh, prim_diff and prim_isect (a Difference / an Intersection of two primitives, answered in place),
            combD (a bih of composites whose tree is a comb D branches deep -- group [sphere 1, far] at the origin and D teeth group [sphere,
            sphere] at z = 8, 16, .. 8 * 2^(D-1): the builder splits a box at its middle, so every branch peels the farthest tooth off; a ray
            up the axis enters the near child and leaves the far one pending at every branch, D entries of 3 words when it calls the item at
            the origin -- tests/ladder.py's tree with composite items),
            and the ADVANCE FAMILIES:
            carve        difference (group [sphere 1, far]) (group of 48 spheres of radius 1 / 64, 1 / 16 apart on the axis before the sphere):
                         a ray along the axis advances twice per carving sphere ahead of it (to its near face, then out of it), once for one
                         it starts at the centre of
            chain        intersection of 12 children group [sphere (0, 0, k / 8) 3, far]: a ray along the axis from outside them all advances
                         through every child but the last -- 11 advance frames and one frame more behind the first child it leaves
            carve_face   `carve` with one more carving sphere, of radius 1 / 4 on the carved sphere's near face: every ray ends on the CARVED face
                         (one advance more, to that sphere's near face), where the Difference asks `inside` of both operands and get_metainfo of
                         the carved solid (vm_inside, vm_meta) above all its advances
            carve_mesh   difference (sphere 1) (a Mesh of 48 triangles across the axis, 1 / 16 apart): a primitive and a Mesh are answered with no
                         frame of their own, so what stops a ray of this family at the brim is the advance's own check and nothing else; one
                         advance per triangle ahead (a Mesh has no inside)
            chain2       intersection [group [sphere 1, the 48 small spheres of `carve`], group [sphere 2, far]]: two advances per small sphere
                         ahead of the ray (from its near face, where the ray is outside the second child; and out of it, where the second child
                         is missed within its depth), one for a sphere it starts at the centre of -- the Intersection's advance family
            chain_in     the same children at (0, 0, -k / 8): a ray from inside them all leaves them last child first, and every child but
                         the last puts a frame on the chain with NO advance -- what commit can count
  ROUTES    rays()       one batch per tower: down the axis to the bottom, to every level's side object, misses at the top -- dealt out so that
                         neighbours in the batch (the lanes of a wave) stand at different stack heights; the same origins are `inside` points
"""
import functools
import re
from collections import namedtuple

import numpy as np

import parity
from helpers import HostSim, O, vm_consts
from glome_amd import api
from glome_amd.scene import SceneDesc

STEP = 2.0 ** -7
KINDS = ("xform", "innerbound", "bound_prim", "bound_comp", "bound_deep", "diff", "diff_retex", "isect", "bih")
BOTTOMS = ("sphere", "sphere_bih", "tri_bih", "inst_bih", "mesh", "prim_diff", "prim_isect")
# a group [transform] tower that only a Warp material refers to (Shader.hs:157-175: a hit on the material traces its frame through the hit's own
# ray, then its scene through the warped ray from the hit point): commit estimates such roots apart from the scene's (flatten.hpp bind_warps)
WARP_KINDS = ("warp_frame", "warp_scene")
WARP_LIGHTS = [((0.0, 7.0, -8.0), (1.0, 1.0, 1.0))]
FAMILIES = ("carve", "carve_face", "carve_mesh", "chain", "chain2", "chain_in")
FAR_A, FAR_B = ((0.0, 6.0, 0.0), 0.25), ((0.0, -6.0, 0.0), 0.25)
N_CARVE, CARVE_Z0, CARVE_PITCH, CARVE_R = 48, -6.0, 1.0 / 16, 1.0 / 64
N_CHAIN = 12
Z_START = -8.0
# where the towers' rays go down: odd sixteenths, beside the axis and every other multiple of 1 / 8 -- a ray along z that lies IN a split plane or
# a box face of a bottom's tree misses it in the reference too (0 * inf), and those planes are all multiples of 1 / 8; the families' rays keep the axis
BOTTOM_XY = (0.3125, 0.1875)


def _side_sites():
    """where the levels' side objects stand: the points of the 1 / 4 grid between radius 1.5 and 3 of the axis (inside every bounding
    sphere of a Bound level, beside the bottom), nearest first"""
    g = np.arange(-12, 13) * 0.25
    pts = [(float(x), float(y)) for x in g for y in g if 1.5 ** 2 <= x * x + y * y <= 3.0 ** 2]
    return sorted(pts, key=lambda p: (p[0] * p[0] + p[1] * p[1], p))


SIDES = _side_sites()
SIDE_R = 1.0 / 16


def zdir(s=1.0):
    """+-z with the other two components -0 (a +0 component misses every box and every bih, lattice.axis_dir)"""
    return np.array([-0.0, -0.0, s], np.float32)


def tilted():
    """the direction of the towers' rays: a hair off +z, unit length in fp32.  (Under an Instance an axis direction's -0 components come out of
    the matrix product as +0, and such a ray misses every box and every bih in the reference too, Q1; the families' rays, which meet neither,
    keep the axis.)  Over the 8 units to the objects it drifts 1 / 64 sideways: a quarter of a side object's radius."""
    v = np.array([2.0 ** -9, 2.0 ** -10, 1.0], np.float64)
    v = (v / np.linalg.norm(v)).astype(np.float32)
    return (v / np.float32(np.linalg.norm(v.astype(np.float64)))).astype(np.float32)


def bottom(sd, name):
    """the bottom's node; a ray down the tower from z = -8 meets it, the origin lies inside it where it has an inside"""
    far = lambda: sd.sphere(*FAR_A)
    if name == "sphere":
        return sd.sphere((0.0, 0.0, 0.0), 1.0)
    if name == "sphere_bih":
        return sd.bih([sd.sphere((0.0, 0.0, 0.0), 1.0)] + [sd.sphere((0.5 * i - 1.0, 0.5 * j - 1.0, 1.5 + 0.25 * ((i + j) % 3)), 0.125) for i in range(5) for j in range(5)])
    if name == "tri_bih":
        t = [((-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (0.0, 1.0, 0.0))]
        t += [((0.5 * i - 1.0, 0.5 * j - 1.0, 1.0 + 0.25 * ((i + j) % 3)), (0.5 * i - 0.75, 0.5 * j - 1.0, 1.0), (0.5 * i - 1.0, 0.5 * j - 0.75, 1.25)) for i in range(5) for j in range(5)]
        return sd.bih([sd.triangle(*p) for p in t])
    if name == "inst_bih":
        unit = sd.sphere((0.0, 0.0, 0.0), 0.5)
        return sd.bih([sd.transform(unit, [api.scale((2.0, 2.0, 2.0))])] +
                      [sd.transform(unit, [api.scale((0.25, 0.25, 0.25)), api.translate((0.5 * i - 1.0, 0.5 * j - 1.0, 1.5))]) for i in range(4) for j in range(4)])
    if name == "mesh":
        v = [(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (0.0, 1.0, 0.0), (-1.0, -1.0, 0.5), (1.0, -1.0, 0.5), (0.0, 1.0, 0.75), (1.0, 1.0, 1.0), (-1.0, 1.0, 1.0)]
        idx = [(0, 1, 2), (3, 4, 5), (5, 6, 7), (3, 5, 7)]
        return sd.mesh(np.array(v, np.float64), [], [list(t) + [-1] * 5 for t in idx], [])
    if name == "prim_isect":  # (a cube cut from a sphere: answered in place by csg_isect, like prim_diff by csg_diff -- no frame word)
        return sd.intersection([sd.sphere((0.0, 0.0, 0.0), 1.0), sd.box((-0.75, -0.75, -0.75), (0.75, 0.75, 0.75))])
    if name == "prim_diff":
        return sd.difference(sd.sphere((0.0, 0.0, 0.0), 1.0), sd.sphere((0.0, 0.0, -1.0), 0.5))
    if name in ("carve", "carve_face"):
        carving = [sd.sphere((0.0, 0.0, CARVE_Z0 + j * CARVE_PITCH), CARVE_R) for j in range(N_CARVE)]
        if name == "carve_face": carving.append(sd.sphere((0.0, 0.0, -1.0), 0.25))  # (carves the face the rays arrive at)
        return sd.difference(sd.group([sd.sphere((0.0, 0.0, 0.0), 1.0), far()]), sd.group(carving))
    if name == "chain":
        return sd.intersection([sd.group([sd.sphere((0.0, 0.0, k / 8.0), 3.0), sd.sphere((0.0, 6.0 + 0.5 * k, 0.0), 0.125)]) for k in range(N_CHAIN)])
    if name.startswith("comb"):
        core = sd.group([sd.sphere((0.0, 0.0, 0.0), 1.0), far()])
        teeth = [sd.group([sd.sphere((0.0, 0.0, 8.0 * 2 ** j), 0.5), sd.sphere((1.0, 0.0, 8.0 * 2 ** j), 0.5)]) for j in range(int(name[4:]))]
        return sd.bih([core] + teeth)
    if name == "carve_mesh":
        z = [CARVE_Z0 + j * CARVE_PITCH for j in range(N_CARVE)]
        v = [p for zj in z for p in ((-1.0, -1.0, zj), (1.0, -1.0, zj), (0.0, 1.0, zj))]
        return sd.difference(sd.sphere((0.0, 0.0, 0.0), 1.0), sd.mesh(np.array(v, np.float64), [], [[3 * j, 3 * j + 1, 3 * j + 2] + [-1] * 5 for j in range(N_CARVE)], []))
    if name == "chain2":
        dots = [sd.sphere((0.0, 0.0, CARVE_Z0 + j * CARVE_PITCH), CARVE_R) for j in range(N_CARVE)]
        return sd.intersection([sd.group([sd.sphere((0.0, 0.0, 0.0), 1.0)] + dots), sd.group([sd.sphere((0.0, 0.0, 0.0), 2.0), far()])])
    if name == "chain_in":
        return sd.intersection([sd.group([sd.sphere((0.0, 0.0, -k / 8.0), 3.0), sd.sphere((0.0, 6.0 + 0.5 * k, 0.0), 0.125)]) for k in range(N_CHAIN)])
    raise KeyError(name)


def level(sd, kind, x, k):
    """level k (0: the one above the bottom) of a tower of `kind` over x"""
    sx, sy = SIDES[k]
    side = sd.sphere((sx, sy, 0.0), SIDE_R)
    two = lambda: sd.group([sd.sphere(*FAR_A), sd.sphere(*FAR_B)])
    if kind == "bound_deep":  # the tower is the bounding solid, the side object what it bounds: the way down is a shadow call
        return sd.bound_object(sd.group([x, side]), sd.sphere((0.0, 0.0, 0.0), 1.0))
    if kind == "bih":
        return sd.bih([sd.group([x, side]), sd.group([sd.sphere((0.0, 5.0, 4.0), 0.25), sd.sphere((0.0, 5.0, 5.0), 0.25)]),
                       sd.group([sd.sphere((0.0, -5.0, 4.0), 0.25), sd.sphere((0.0, -5.0, 5.0), 0.25)])])
    core = {"xform": lambda: sd.transform(x, [api.translate((0.0, 0.0, STEP if k % 2 == 0 else -STEP))]),
            "inst2": lambda: sd.transform(sd.transform(x, [api.translate((0.0, 0.0, STEP))]), [api.translate((0.0, 0.0, -STEP))]),
            "innerbound": lambda: sd.innerbound(x, sd.sphere((0.0, 0.0, 0.0), 3.0)),
            "bound_prim": lambda: sd.bound_object(sd.sphere((0.0, 0.0, 0.0), 3.5), x),
            "bound_comp": lambda: sd.bound_object(sd.group([sd.sphere((0.0, 0.0, 0.0), 3.5), sd.sphere(*FAR_A)]), x),
            "diff": lambda: sd.difference(x, two()),
            "diff_retex": lambda: sd.difference_retexture(x, two()),
            "isect": lambda: sd.intersection([x, sd.group([sd.sphere((0.0, 0.0, 0.0), 3.5), sd.sphere(*FAR_A)])])}[kind]()
    return sd.group([core, side])


Tower = namedtuple("Tower", "sd kind bottom levels shift")  # shift: the bottom's displacement along z in the scene (an odd number of xform levels: STEP)


def tower(kind, bot, levels, xfill=0, ibfill=0):
    """`levels` levels of `kind` over `bot`; above them the FILLER of a brim scene (brim): xfill levels of group [transform], the tight kind
    with the smallest step that keeps every answer, then ibfill bare `innerbound x (sphere 3)`, 4 words each and the smallest step the
    builder offers (under one, every ray that meets the sphere of radius 3 answers its near face)"""
    assert levels + xfill <= len(SIDES)
    sd = SceneDesc()
    x = bottom(sd, bot)
    base = "xform" if kind in WARP_KINDS else kind
    ups = 0
    for k in range(levels + xfill):
        kd = base if k < levels else "xform"
        x = level(sd, kd, x, k)
        if kd == "xform": ups += 1 if k % 2 == 0 else -1
    for _ in range(ibfill):
        x = sd.innerbound(x, sd.sphere((0.0, 0.0, 0.0), 3.0))
    if kind in WARP_KINDS:  # the tower is no part of the root: a Warp material on a disc before it traces it, as its frame or as its scene
        small = sd.sphere(*FAR_B)
        xfm = api.compose([api.translate((0.0, 0.0, STEP))])
        warp = sd.material_warp(x, small, WARP_LIGHTS, xfm) if kind == "warp_frame" else sd.material_warp(small, x, WARP_LIGHTS, xfm)
        x = sd.group([sd.tex(sd.disc((0.0, 0.0, -4.0), (0.0, 0.0, -1.0), 3.5), warp), sd.sphere(*FAR_A)])
    sd.set_root(x)
    sd.set_camera((0.0, 0.0, -8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0)
    sd.add_light((0.0, 7.0, -8.0), (1.0, 1.0, 1.0))
    return Tower(sd, kind, bot, levels + xfill, STEP * ups)


# ------------------------------------------------------------------------------------------------------------------- commit and estimate
class Refused(Exception):
    def __init__(self, msg):
        Exception.__init__(self, msg)
        m = re.search(r"\((\d+) of (\d+) words\)", msg)
        self.words, self.limit = (int(m.group(1)), int(m.group(2))) if m else (None, None)


def commit_host(sd):
    """(HostSim, builder, node map) of a description; Refused, with the count of the message, where commit refuses it"""
    b = api.Builder()
    nm, _ = sd.replay(b)
    try:
        return HostSim(b, nm[sd.root]), b, nm
    except RuntimeError as e:
        raise Refused(str(e))


def estimate(sd):
    """the frame words commit estimates for a ray of the scene: FlatScene::vm_words where commit accepts, the refusal's own count where not"""
    try:
        return commit_host(sd)[0].vm_words()[0]
    except Refused as r:
        assert r.words is not None, str(r)
        return r.words


@functools.lru_cache(maxsize=None)
def brim(kind, bot):
    """(levels of `kind`, group [transform] fillers, innerbound fillers) of the tallest tower over `bot` that commit accepts, found by asking
    the estimate: as many levels of the kind as fit, then as many of each filler as still fit.  The accepted scene ends within one
    innerbound frame of kVmWords; one more innerbound (next_up) is refused."""
    limit = commit_host(tower(kind, bot, 1).sd)[0].vm_words()[1]
    e1, e2 = estimate(tower(kind, bot, 1).sd), estimate(tower(kind, bot, 2).sd)
    n = max(1, (limit - e1) // (e2 - e1) + 1)
    while estimate(tower(kind, bot, n + 1).sd) <= limit: n += 1
    while estimate(tower(kind, bot, n).sd) > limit: n -= 1
    xf = 0
    while estimate(tower(kind, bot, n, xf + 1).sd) <= limit: xf += 1
    ib = 0
    while estimate(tower(kind, bot, n, xf, ib + 1).sd) <= limit: ib += 1
    return n, xf, ib


def next_up(kind, bot):
    n, xf, ib = brim(kind, bot)
    return n, xf, ib + 1


# ------------------------------------------------------------------------------------------------------------------------------- rays
Rays = namedtuple("Rays", "o d tmax labels level")  # level: the level whose side object the ray is aimed at (-1: the bottom, -2: a miss at the top)


def rays(tw, n_min=192):
    """the tower's mixed batch: bottom, side objects from the deepest level up, misses -- round robin, so that the 64 lanes of every wave stand
    at different stack heights; at least n_min rays (more than two waves)"""
    sides = list(range(tw.levels))
    if len(sides) > 40:  # a tall tower: the 20 deepest, the 10 highest, and every fourth between
        sides = sorted(set(sides[:20] + sides[-10:] + sides[20:-10:4]))
    o, lab, lev = [], [], []
    reps = max(1, -(-n_min // (len(sides) + 2)))
    for rep in range(reps):
        dz = -0.125 * (rep % 48)  # (the same ray from a little further away: another depth, the same frames)
        o.append((BOTTOM_XY[0], BOTTOM_XY[1], Z_START + dz)); lab.append("bottom"); lev.append(-1)
        for k in sides:
            o.append((SIDES[k][0], SIDES[k][1], Z_START + dz)); lab.append("side"); lev.append(k)
        o.append((0.0, 7.5, Z_START + dz)); lab.append("miss"); lev.append(-2)
    o = np.array(o, np.float32)
    d = np.tile(tilted(), (len(o), 1))
    return Rays(o, d, np.full(len(o), 64.0, np.float32), np.array(lab), np.array(lev))


def inside_points(tw):
    """points for `inside`: the centre (inside the bottom where it has an inside), every side object's centre, points outside everything"""
    p = [(0.0, 0.0, tw.shift), (0.0, 0.0, tw.shift + 0.5), (0.0, 7.5, 0.0), (4.0, 4.0, 4.0)] + [(SIDES[k][0], SIDES[k][1], 0.0) for k in range(tw.levels)]
    return np.array(p, np.float32)


def carve_rays(shift=0.0):
    """rays along the axis into the carving spheres of `carve`: (origins, directions, tmax, advances) -- advances 2 m for a ray that starts
    half way before the m-th sphere from the end, 2 m - 1 for one that starts at its centre: every count from 0 to 2 N_CARVE"""
    o, adv = [], []
    for j in range(N_CARVE + 1):  # spheres j .. N_CARVE - 1 lie ahead
        o.append((0.0, 0.0, CARVE_Z0 + j * CARVE_PITCH - CARVE_PITCH / 2 + shift)); adv.append(2 * (N_CARVE - j))
        if j < N_CARVE:
            o.append((0.0, 0.0, CARVE_Z0 + j * CARVE_PITCH + shift)); adv.append(2 * (N_CARVE - j) - 1)
    o = np.array(o, np.float32)
    return o, np.tile(zdir(), (len(o), 1)), np.full(len(o), 64.0, np.float32), np.array(adv)


def carve_face_rays(shift=0.0):
    o, d, tm, adv = carve_rays(shift)
    return o, d, tm, adv + 1


def carve_mesh_rays(shift=0.0):
    """rays a hair off the axis (tilted: the Mesh's boxes want no zero component) that start half way before the triangle j of `carve_mesh`:
    (origins, directions, tmax, advances = the triangles ahead)"""
    o = np.array([(0.0, 0.0, CARVE_Z0 + j * CARVE_PITCH - CARVE_PITCH / 2 + shift) for j in range(N_CARVE + 1)], np.float32)
    return o, np.tile(tilted(), (len(o), 1)), np.full(len(o), 64.0, np.float32), np.array([N_CARVE - j for j in range(N_CARVE + 1)])


def chain_rays(shift=0.0):
    """rays along the axis into `chain`, from outside all its spheres and from inside the first m < 12 of them (origins at z = -3 + m / 8 - 1 / 16):
    (origins, directions, tmax, advances) -- one advance per child the ray starts outside of but the last, whose hit is the answer"""
    ms = [0] + list(range(N_CHAIN))
    o = [(0.0, 0.0, Z_START + shift)] + [(0.0, 0.0, -3.0 + m / 8.0 - 1.0 / 16 + shift) for m in ms[1:]]
    o = np.array(o, np.float32)
    return o, np.tile(zdir(), (len(o), 1)), np.full(len(o), 64.0, np.float32), np.array([max(0, N_CHAIN - 1 - m) for m in ms])


def chain_in_rays(shift=0.0):
    """rays along the axis from z = -2, inside all the spheres of `chain_in`, which they leave at depth 5 - k / 8: with tmax = 5 - j / 8 the
    first j children answer a miss (no frame), every later one but the last a frame: (origins, directions, tmax, frames without an advance)"""
    tm = np.array([64.0] + [5.0 - j / 8.0 for j in range(N_CHAIN)], np.float32)
    o = np.tile(np.array([0.0, 0.0, -2.0 + shift], np.float32), (len(tm), 1))
    return o, np.tile(zdir(), (len(o), 1)), tm, np.array([N_CHAIN - 1] + [N_CHAIN - 1 - j for j in range(N_CHAIN)])


# -------------------------------------------------------------------------------------------------------------------------- the oracle
def oracle_answers(sd, o, d, tmax):
    """the fp64 oracle on the rays: depth (-1 a miss), shadow, inside of the origins, and the rays it gave up"""
    orc, om, _ = O.load_scene(sd, use_float=False)
    o64, d64, t64 = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(tmax, np.float64)
    r = orc.rayint(om[sd.root], o64, d64, t64)
    sh = orc.shadow(om[sd.root], o64, d64, t64)
    div = r["diverged"] | orc.last_diverged
    return {"t": r["t"], "shadow": sh, "inside": orc.inside(om[sd.root], o64), "diverged": div, "prim": r["prim"], "nm": om}


def depth_ok(t, ref):
    """lattice.depth_ok for finite depths: both miss, or within parity.T_RTOL of the fp64 depth"""
    t, ref = np.asarray(t, np.float64), np.asarray(ref, np.float64)
    return np.where((ref < 0) | (t < 0), (ref < 0) & (t < 0), np.abs(t - ref) <= parity.T_RTOL * np.maximum(1.0, np.abs(ref)))


# ------------------------------------------------------------------------------------------------------------------- what the tests share
K = vm_consts()
LIGHTS = [((0.0, 7.0, -8.0), (1.0, 1.0, 1.0), 1000000.0, True)]
BRIMS = [(k, "sphere") for k in KINDS] + [("xform", b) for b in BOTTOMS[1:] + ("comb5",) + FAMILIES] + [("warp_frame", "sphere"), ("warp_scene", "tri_bih")]  # the brim scenes: every kind, every bottom, every family
FAMILY_RAYS = {"carve": carve_rays, "carve_face": carve_face_rays, "carve_mesh": carve_mesh_rays, "chain": chain_rays, "chain2": carve_rays, "chain_in": chain_in_rays}
# the steps the estimate allows a family's ray: advances of a Difference, advances of an Intersection, children a ray leaves (all counted at commit)
ALLOWANCE = {"carve": K["kCsgMaxAdvance"], "carve_face": K["kCsgMaxAdvance"], "carve_mesh": K["kCsgMaxAdvance"], "chain": K["kVmIsectChain"], "chain2": K["kVmIsectChain"], "chain_in": N_CHAIN - 1}
OVER_FROM_AFAR = ("carve", "carve_face", "carve_mesh", "chain", "chain2")  # bottoms that a ray down the tower from z = -8 advances through beyond the allowance: the family's own rays cover them


def family(bot, levels):
    """(tower of group [transform] levels over the family, its HostSim, its estimate, origins, directions, tmax, steps per ray)"""
    tw = tower("xform", bot, levels)
    hs = commit_host(tw.sd)[0]
    o, d, tm, cnt = FAMILY_RAYS[bot](tw.shift)
    return tw, hs, hs.vm_words()[0], o, d, tm, cnt


def brim_batch(kind, bot):
    """the brim scene and its rays within the allowances: the tower's mixed batch and, over a family, the family's own rays"""
    tw = tower(kind, bot, *brim(kind, bot))
    r = rays(tw)
    keep = r.labels != "bottom" if bot in OVER_FROM_AFAR else np.ones(len(r.o), bool)
    r = Rays(r.o[keep], r.d[keep], r.tmax[keep], r.labels[keep], r.level[keep])
    if bot in FAMILIES:
        fo, fd, ftm, cnt = FAMILY_RAYS[bot](tw.shift)
        sel = cnt <= ALLOWANCE[bot]
        r = Rays(np.concatenate([r.o, fo[sel]]), np.concatenate([r.d, fd[sel]]), np.concatenate([r.tmax, ftm[sel]]), np.concatenate([r.labels, np.full(sel.sum(), "family")]),
                 np.concatenate([r.level, np.full(sel.sum(), -1)]))
    return tw, r
