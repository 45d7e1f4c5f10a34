"""Shading cases: every branch of trace / mpreshade / mpostshade, the colour algebra and the solid textures, reached by a ray built for it.

A plain module (no GPU, no fixtures) shared by tests/test_shading_host.py and tests/test_shading_gpu.py, in the style of tests/lattice.py:

  FAMILIES  light, surface, texfold, reflect, refract, blend, tx, warp: each a scene of TILES -- squares of two triangles, 32 x 32, 64 apart
            along z, floors at y = 0 (ceilings, slab faces and occluders at other heights) -- every tile under the material (or stack of
            materials) of one branch, and BATCHES: a light list, a maxdepth and the rays of one launch, every ray with a label
            `family/branch`.  A batch holds several labels under ONE light list and rays that miss, so that dealt out label by label
            (interleave) a wave holds lanes in different states: check_mixing asserts it from what the oracle answers.  Every parameter is dyadic (the two heights beside kDel apart: they are about kDel), the rays go straight
            down onto dyadic points, so hit point, normal and lvec are exact on every backend; the oblique rays of refract/critical are
            the exception and say so.
  ROUTES    prims (the tiles as a list of primitives: the flat tier, lean or full as the materials ask), prims_full (the same scene with an
            unreachable Reflect and an unreachable Blend in the material table: the full instance, whatever the maxdepth), bih_tri (one
            triangle bih: the hand-written walk), mesh (one Mesh: mesh_closest_wave), generic (the tiles below a Bound: the interpreter,
            which has ONE shading instance -- full, with the per-lane preshade and light_set).  A route holds the families it can:
            a triangle bih has one texture for all its triangles, a Mesh one material per triangle and no wrapper objects.

A case is one ray of one batch.  evaluate() computes it by the fp64 oracle and by the oracle in float and marks the AGREEMENT SET: the cases
on which the two give one decision (hit / miss, the shadow rays and the secondary rays the ray spawned), colours within COLOUR_TOL and
depths within parity.T_RTOL.  Inside it a backend -- the host build of the device headers (hostsim_trace: the full tier, the lean tier where
the product would launch one, the faithful traversal), the GPU -- is held on EVERY case (check_backend); NaN equals NaN."""
import functools
from collections import namedtuple

import numpy as np

import parity
from helpers import O
from glome_amd import api
from glome_amd.scene import SceneDesc

MAX_OUTSIDE = 0.02    # at most this share of a family-and-route's cases may lie outside the agreement set (lattice.MAX_OUTSIDE)
MIN_PER_LABEL = 32    # and every label keeps at least this many inside it (lattice.MIN_PER_LABEL)
COLOUR_TOL = 1e-4     # of max(1, |ref|): the project's gate (north_star, tests/parity.py)
KDEL = float(np.float32(0.0001))  # rt_device.hpp kDel, Vec.hs:40
K_MAX_MAT_NEST = 4    # rt_types.h kMaxMatNest
MISS_DEPTH = 1e6

f32 = lambda x: np.asarray(x, np.float32)
TINY = float(np.float32(2.0 ** -126))  # the smallest normal fp32: the device build flushes denormals, so the fp32 step beside 0 that every backend can hold
DOWN = (-0.0, -1.0, -0.0)              # (a +0 component misses every bih, Q1; a -0 does not)
HALF = 16.0
GRID = [(float(dx), dz + 0.5) for dx in range(-3, 4) for dz in range(-3, 4)]  # 49 dyadic points of a tile, none on its diagonal (x == z)
HEIGHTS = [0.25 * k for k in range(1, 41)]                                    # 40 heights to start from above one point

Batch = namedtuple("Batch", "lights maxdepth o d labels expect")  # expect: {label: {"shadow": n, "secondary": n, "hit": bool}} what the fp64 oracle must answer
Case = namedtuple("Case", "family route")


def ulp(x, k):
    return float(np.nextafter(np.float32(x), np.float32(np.inf if k > 0 else -np.inf)))


def light(pos, color=(16.0, 16.0, 16.0), rad=1000000.0, shadow=True):
    return (tuple(float(v) for v in pos), tuple(float(v) for v in color), float(rad), bool(shadow))


def cz(j):
    return 64.0 * j


# ---------------------------------------------------------------------------------------------------------------- the floor of a route
class Floor:
    """the tiles of one family on one route.  tile(): a square of two triangles centred at (0, y, z) whose normal looks up (or down),
    under a stack of materials (the first is the innermost Tex: the head the fold starts with, Trace.hs:67-80)"""

    def __init__(self, route, sd=None):
        self.route, self.sd = route, SceneDesc() if sd is None else sd
        self.items, self.tris, self.tri_mat = [], [], []
        self.one_mat = route == "bih_tri"            # one texture for every triangle
        self.stacks = route in ("prims", "prims_full", "generic")   # a tile can carry a stack of materials
        self.deep_stacks = route == "generic"        # of more than two (the flat tier's root program holds two Tex levels above an entry)
        self.wrappers = self.stacks                  # and stand below a NoShadow / OnlyShadow
        self.normals = route in ("prims", "prims_full", "generic", "mesh")  # shading normals (trianglenorm, Mesh vertex normals)
        self.norms = []

    def tile(self, z, stack, y=0.0, up=True, half=HALF, wrap=None, normal=None):
        a, b, c, d = (-half, y, z - half), (-half, y, z + half), (half, y, z + half), (half, y, z - half)
        tris = [(a, b, c), (a, c, d)] if up else [(a, c, b), (a, d, c)]
        if self.route in ("bih_tri", "mesh"):
            assert len(stack) == 1 and wrap is None, "one material per triangle, no wrappers"
            self.tris += tris; self.tri_mat += [stack[0]] * 2; self.norms += [normal] * 2
            return
        sd = self.sd
        nodes = [sd.triangle(*t) if normal is None else sd.trianglenorm(*t, normal, normal, normal) for t in tris]
        for m in stack:
            nodes = [sd.tex(n, m) for n in nodes]
        node = sd.group(nodes)
        if wrap == "noshadow": node = sd.noshadow(node)
        if wrap == "onlyshadow": node = sd.onlyshadow(node)
        self.items.append(node)

    def finish(self):
        sd = self.sd
        if self.route == "prims_full":  # unreachable: no tile carries them, the commit's traits still see them
            sd.material_blend(sd.material_reflect(0.5), sd.material_surface((0.5, 0.5, 0.5), 1, 0.5, 0.5, 0, 0), 0.5)
        if self.route == "bih_tri":
            assert len(set(self.tri_mat)) == 1
            root = sd.tex(sd.bih([sd.triangle(*t) for t in self.tris]), self.tri_mat[0])
        elif self.route == "mesh":
            v = np.array([p for t in self.tris for p in t], np.float64)
            t = np.full((len(self.tris), 8), -1, np.int32)
            t[:, :3] = np.arange(3 * len(self.tris)).reshape(-1, 3)
            mats = sorted(set(self.tri_mat))
            t[:, 6] = [mats.index(m) for m in self.tri_mat]
            nrm = np.zeros((0, 3))
            if any(n is not None for n in self.norms):
                nrm = np.array([n for n in self.norms if n is not None], np.float64)
                k = 0
                for i, n in enumerate(self.norms):
                    if n is not None: t[i, 3:6] = k; k += 1
            root = sd.mesh(v, nrm, t, mats)
        elif self.route == "generic":
            root = sd.bound_object(sd.sphere((0.0, 0.0, 0.0), 32768.0), sd.group(self.items))
        else:
            root = sd.group(self.items)
        sd.set_root(root)
        sd.set_camera((0.0, 8.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 45.0)
        return sd


def down(z, pts=GRID, heights=(3.0,), y=0.0):
    """rays straight down onto the points (dx, dz) of the tile at z, one per height above y"""
    o = [(dx, y + h, z + dz) for (dx, dz) in pts for h in heights]
    return o, [DOWN] * len(o)


class Batches:
    """collects the batches of a family: add(label, o, d) to the batch in progress, close(lights, maxdepth) to finish it"""

    def __init__(self):
        self.out, self.o, self.d, self.lab, self.expect = [], [], [], [], {}

    def add(self, label, od, **expect):
        o, d = od
        assert len(o) >= MIN_PER_LABEL + 3, (label, len(o))
        self.o += list(o); self.d += list(d); self.lab += [label] * len(o)
        if expect: self.expect[label] = expect

    def close(self, lights, maxdepth=3):
        # every batch holds primary rays that miss: beside the tiles, which are 32 wide
        self.add(self.lab[0].split("/")[0] + "/miss", down(cz(0), [(dx + 100.0, dz) for (dx, dz) in GRID]), shadow=0, secondary=0, hit=False)
        o, d = f32(self.o).reshape(-1, 3), f32(self.d).reshape(-1, 3)
        assert len(np.unique(np.hstack([o, d]).view(np.uint32), axis=0)) == len(o), "a ray is repeated"
        self.out.append(Batch(list(lights), maxdepth, o, d, np.array(self.lab), dict(self.expect)))
        self.o, self.d, self.lab, self.expect = [], [], [], {}


def base_surface(sd, k=0, alpha=1.0):
    return sd.material_surface((0.5, 0.25 + 0.125 * (k % 5), 0.75 - 0.125 * (k % 3)), alpha, 0.25, 0.5, 0.25, 2.0)


def tile_light(z):
    return light((5.0, 4.0, z + 3.0))


# ---------------------------------------------------------------------------------------------------------------- light list (mpreshade)
def fam_light(F):
    """Every batch shares ONE light list among tiles in different states -- and rays that miss -- so that, dealt out label by label, a wave
    holds lanes on either side of the branch the batch is about (preshade_wave's per-lane `lit` and its partial-mask occluded_wave).
    Tiles: 0, 10 open floors; 1 below a ceiling; 2, 3, 6, 7 below the occluders of the kDel margin; 4, 5 below a NoShadow and an OnlyShadow
    ceiling; 8 a floor raised to y = 1, 9 to y = 2, -1 one lowered to y = -1.  Lights are kept to their tile by `rad` where a batch says so."""
    sd, B = F.sd, Batches()
    m = base_surface(sd)
    F.tile(cz(0), [m]); F.tile(cz(10), [m])
    F.tile(cz(1), [m]); F.tile(cz(1), [m], y=2.0, up=False)
    F.tile(cz(8), [m], y=1.0); F.tile(cz(9), [m], y=2.0); F.tile(cz(-1), [m], y=-1.0)
    if F.wrappers:
        F.tile(cz(4), [m]); F.tile(cz(4), [m], y=2.0, up=False, wrap="noshadow")
        F.tile(cz(5), [m]); F.tile(cz(5), [m], y=2.0, up=False, wrap="onlyshadow")
    # the light above the tangent plane of the hit, in it and below it by one step: `vdot(lvec, n) < 0` is false IN the plane, so the shadow
    # ray is spawned there too and adds nothing -- only the count tells (both oracles: 1, 1, 0).  Beside it in the wave: the lowered floor,
    # which the light is above, and the raised one, which it is behind
    for what, y, ns in (("above", TINY, 1), ("in", 0.0, 1), ("below", -TINY, 0)):
        B.add("light/tangent-" + what, down(cz(0)), shadow=ns, secondary=0, hit=True)
        B.add("light/tangent-%s:lowered-floor" % what, down(cz(-1), y=-1.0), shadow=1, secondary=0, hit=True)
        B.add("light/tangent-%s:raised-floor" % what, down(cz(8), y=1.0), shadow=0, secondary=0, hit=True)
        B.close([light((20.0, y, 3.0))], 3)
    # llen == rad: lvec = (0, 4, +-3) and (+-3, 4, 0), rad = 5; `llen > rad` is false at equality.  Beside them points nearer and farther
    pts = [(5.0, 2.0), (5.0, 8.0), (2.0, 5.0), (8.0, 5.0)]
    near = [(float(dx), dz + 0.5) for dx in (3, 4, 5, 6, 7) for dz in (3, 4, 5, 6)]    # (5 - x)^2 + (5 - z)^2 <= 6.25 < 9
    far = [(float(dx), dz + 0.5) for dx in (-2, -1, 0, 1) for dz in (-3, -2, -1, 0)]   # (5 - x)^2 >= 16 > 9
    for what, rad, ns in (("==", 5.0, 1), ("-ulp", ulp(5.0, -1), 0), ("+ulp", ulp(5.0, +1), 1)):
        B.add("light/rad" + what, down(cz(0), pts, HEIGHTS[1:21:2] + [0.625]), shadow=ns, secondary=0)  # (11 heights: 44 rays)
        B.add("light/rad%s:nearer" % what, down(cz(0), near, (3.0, 2.5)), shadow=1, secondary=0)
        B.add("light/rad%s:farther" % what, down(cz(0), far, (3.0, 2.5, 3.5)), shadow=0, secondary=0)
        B.close([light((5.0, 4.0, 5.0), rad=rad)], 3)
    B.add("light/none", down(cz(0)), shadow=0, secondary=0)
    B.add("light/none:below-ceiling", down(cz(1), heights=(1.0,)), shadow=0, secondary=0)
    B.close([], 3)
    # sixteen lights, each kept to one tile by its radius, so every tile sees another mask: the first alone, the sixteenth alone (the mask's
    # bit 15), the odd ones from 1 to 13, and -- below the ceiling, every one occluded -- the even ones from 2 to 14
    over = {0: (0, 0.0), 15: (10, 0.0)}
    over.update({i: (9, 2.0) for i in range(1, 15, 2)}); over.update({i: (1, 0.0) for i in range(2, 15, 2)})
    B.add("light/16-first", down(cz(0)), shadow=1, secondary=0)
    B.add("light/16-sixteenth", down(cz(10)), shadow=1, secondary=0)
    B.add("light/16-alternating", down(cz(9), y=2.0), shadow=7, secondary=0)
    B.add("light/16-alternating:occluded", down(cz(1), heights=(1.0,)), shadow=7, secondary=0)
    B.close([light((i - 7.5, over[i][1] + 4.0, cz(over[i][0]) + 2.0), color=(2.0 + i, 4.0, 18.0 - i), rad=24.0) for i in range(16)], 3)
    # the light AT the hit point: llen == 0, ldir = 0 * inf = NaN (which adds nothing: isNaN -> 0).  Beside those lanes: other points of the
    # tile, in whose plane that light lies, and the lowered floor, from which the tile hides it; a second light reaches them all
    B.add("light/llen==0", down(cz(0), [(1.0, 0.5)], HEIGHTS))
    B.add("light/llen==0:same-tile", down(cz(0), [p for p in GRID if p != (1.0, 0.5)]), shadow=2, secondary=0, hit=True)
    B.add("light/llen==0:lowered-floor", down(cz(-1), y=-1.0), shadow=2, secondary=0, hit=True)
    B.close([light((1.0, 0.0, 0.5)), tile_light(cz(0))], 3)
    # one list -- a light high above every tile (its shadow rays are all but vertical: each meets what stands over its own tile), a
    # shadowless one beside it, and one in the plane of the raised floor -- over tiles in every state: open, below a ceiling (occluded; the
    # shadowless light costs no ray and shines through), below a NoShadow ceiling (lit) and an OnlyShadow one (occluded; the primary ray
    # passes it), the floor the third light is in the plane of, and the higher one it is behind.  (A Mesh casts no shadow at all, Mesh.hs:210
    # `shadow s r d = False`: on the mesh route every occluder label is lit, in the oracle as in the product, and the labels keep the count.)
    high = [light((5.0, 4096.0, cz(5)), color=(2.0 ** 26,) * 3), light((-5.0, 4096.0, cz(5)), color=(2.0 ** 25, 2.0 ** 24, 2.0 ** 23), shadow=False),
            light((20.0, 1.0, cz(8) + 3.0))]  # (so bright for their height: 2^26 / 4096^2 = 4)
    B.add("light/lit", down(cz(0)), shadow=2, secondary=0)
    B.add("light/occluded", down(cz(1), heights=(1.0,)), shadow=2, secondary=0)
    B.add("light/in-plane-of-raised-floor", down(cz(8), y=1.0), shadow=2, secondary=0)
    B.add("light/behind-higher-floor", down(cz(9), y=2.0), shadow=1, secondary=0)
    if F.wrappers:
        B.add("light/noshadow-occluder", down(cz(4), heights=(1.0,)), shadow=2, secondary=0)
        B.add("light/onlyshadow-occluder", down(cz(5)), shadow=2, secondary=0, hit=True)  # (from above it: the primary ray does not see it)
    B.close(high, 3)
    B.add("light/shadowless-behind-occluder", down(cz(1), heights=(1.0,)), shadow=0, secondary=0)
    B.add("light/shadowless:open", down(cz(0)), shadow=0, secondary=0)
    B.close([light((5.0, 4.0, cz(1) + 3.0), shadow=False)], 3)
    # a vertical shadow ray of length llen = 1 is tested to llen - 2 kDel from p + kDel n: an occluder at llen - 0.5 kDel is inside the
    # margin and does not occlude, one at llen - 1.5 kDel does.  (That shadow ray is (a - a, 1, b - b) = (+0, 1, +0), which misses every bih
    # and Mesh box (Q1): in a tree neither occluder shadows, and the oracle says so too.)  The same margin on a slanted shadow ray, no
    # component zero: lvec = (2, 3, 6), llen = 7; the ray starts kDel above the floor and meets a plane at height h after (h - kDel) * 7 / 3.
    # All four in one batch, each light kept to its tile by its radius: lit and occluded lanes at the margin in one wave
    lights = []
    for j, what, f in ((2, "inside-margin", 0.5), (3, "outside-margin", 1.5)):
        F.tile(cz(j), [m]); F.tile(cz(j), [m], y=float(np.float32(1.0 - f * KDEL)), up=False)
        B.add("light/" + what, down(cz(j), [(1.0, 0.5)], [k / 64.0 for k in range(1, 41)]), shadow=1, secondary=0)
        lights.append(light((1.0, 1.0, cz(j) + 0.5), color=(1.0, 0.5, 0.25), rad=2.0))
    for j, what, f in ((6, "inside-margin:slanted", 1.5), (7, "outside-margin:slanted", 2.5)):
        h = float(np.float32(KDEL + (7.0 - f * KDEL) * 3.0 / 7.0))
        F.tile(cz(j), [m]); F.tile(cz(j), [m], y=h, up=False)
        B.add("light/" + what, down(cz(j), [(1.0, 0.5)], [k / 16.0 for k in range(1, 41)]), shadow=1, secondary=0)
        lights.append(light((3.0, 3.0, cz(j) + 6.5), color=(32.0, 16.0, 8.0), rad=8.0))
    B.close(lights, 3)
    return B.out, dict(secondary=False, nested=False, refract=False)


# ---------------------------------------------------------------------------------------------------------------- Surface (Shader.hs:90-105)
def fam_surface(F):
    sd, B = F.sd, Batches()
    col = (0.5, 0.25, 0.75)
    # ks beside kDel (`ks <= kDel`: no blinn term): kd = 0 and a light of their own bright enough that the term, ks * blinn * colour / llen^2, shows
    # where it is wrongly taken or left (2^-13 * 0.8 * 4096 / 34: 1e-2).  kDel itself is float32(0.0001), which fp64 too sees as <= 0.0001
    variants = [("ks=0", (col, 1, 0.25, 0.0, 0.0, 2.0)), ("ks=2^-14", (col, 1, 0.25, 0.0, 2.0 ** -14, 2.0)), ("ks=kDel", (col, 1, 0.25, 0.0, KDEL, 2.0)),
                ("ks=2^-13", (col, 1, 0.25, 0.0, 2.0 ** -13, 2.0))]
    variants += [("shine=%g" % s, (col, 1, 0.25, 0.5, 0.5, s)) for s in (0.0, 1.0, 2.0, 2.5, 64.0)]
    variants += [("alpha=%g" % a, (col, a, 0.25, 0.5, 0.25, 2.0)) for a in (0.0, 0.5, 1.0)]
    variants += [("kd=0", (col, 1, 0.25, 0.0, 0.5, 2.0))]
    for j, (what, args) in enumerate(variants):
        F.tile(cz(j), [sd.material_surface(*args)])
        B.add("surface/" + what, down(cz(j)), secondary=0, hit=True)
    j0 = len(variants)
    if F.normals:
        # a shading normal that faces away from the eye while the light is in front of it: half . n < 0, and pow of a negative base is NaN
        # with a fractional shine (isNaN -> 0), negative with an odd one, positive with an even one.  n = (0.5, -1, 0) / |.|: the eye
        # (0, 1, 0) is behind it, the light at (+16, 1, .) before it
        n = np.array([0.5, -1.0, 0.0]); n = tuple((n / np.linalg.norm(n)).tolist())
        for k, s in enumerate((2.5, 3.0, 2.0)):
            F.tile(cz(j0 + k), [sd.material_surface(col, 1, 0.25, 0.5, 0.5, s)], normal=n)
            B.add("surface/half.n<0:shine=%g" % s, down(cz(j0 + k)), secondary=0, hit=True)
    if F.stacks:
        # the fold's `acc.a + kDel >= 1` in a scene of Surfaces alone (the lean kernels' copy, shade_hit_lean): below the top a Surface whose
        # ambient colour is 4096, so that what the fold lets through past an alpha of 1 - 2^-13 (1.2e-4 of it) shows, and nothing past
        # float32(1 - kDel) + one step, where a + kDel is exactly 1 in fp32 (texfold has the same pair over a mirror: the full kernels' copy)
        glare = sd.material_surface((4096.0, 4096.0, 4096.0), 1, 1.0, 0.0, 0.0, 0.0)
        for k, (what, a) in enumerate((("1-2^-13", 1 - 2.0 ** -13), ("1-kDel+ulp", ulp(np.float32(1.0) - np.float32(KDEL), +1)))):
            F.tile(cz(j0 + 3 + k), [sd.material_surface(col, a, 0.25, 0.5, 0.25, 2.0), glare])
            B.add("surface/fold:alpha=" + what, down(cz(j0 + 3 + k)), secondary=0, hit=True)
    bright = [light((5.0, 4.0, cz(j) + 3.0), color=(4096.0, 4096.0, 4096.0)) for j in range(4)]
    lights = bright + [tile_light(cz(j)) for j in (4, 7, 10, 12)]
    # (shadowless: p + kDel n lies below the tile for such a normal, and the tile itself would shadow the light)
    if F.normals: lights += [light((16.0, 1.0, cz(j0 + k) + 0.25), color=(256.0, 256.0, 256.0), shadow=False) for k in range(3)]
    B.close(lights, 3)
    return B.out, dict(secondary=False, nested=False, refract=False)


# ---------------------------------------------------------------------------------------------------------------- the Tex fold (Trace.hs:67-80)
def fam_texfold(F):
    sd, B = F.sd, Batches()
    solid, mirror = base_surface(sd, 1), sd.material_reflect(1.0)
    veil = [base_surface(sd, k + 2, alpha=0.25 + 0.0625 * k) for k in range(7)]
    for j, n in enumerate((1, 2, 8) if F.deep_stacks else (1, 2)):
        F.tile(cz(j), veil[:n - 1] + [solid] if n > 1 else [veil[0]])
        B.add("texfold/stack-%d" % n, down(cz(j)), secondary=0, hit=True)
    # `acc.a + kDel >= 1`: an alpha of 1 - 2^-13 is not yet opaque (the fold goes on to the mirror below it: one secondary ray), 1 - 2^-14 is
    # and the equality itself: with a = float32(1 - kDel) + one step, a + kDel rounds to exactly 1 in fp32 and is 1 + 4e-8 in fp64 -- opaque
    # on every backend, by `>=` alone in fp32 (float32(1 - kDel) itself is opaque in fp32 and not in fp64: no case)
    a_eq = ulp(np.float32(1.0) - np.float32(KDEL), +1)
    assert np.float32(a_eq) + np.float32(KDEL) == np.float32(1.0) and a_eq + 0.0001 >= 1.0
    for j, what, a, ns in ((3, "1-2^-13", 1 - 2.0 ** -13, 1), (4, "1-2^-14", 1 - 2.0 ** -14, 0), (6, "1-kDel+ulp", a_eq, 0)):
        F.tile(cz(j), [base_surface(sd, 3, alpha=a), mirror]); F.tile(cz(j), [solid], y=6.0, up=False)
        B.add("texfold/alpha=" + what, down(cz(j)), shadow=7 + 7 * ns, secondary=ns, hit=True)  # (seven lights on the tile, and on the ceiling the mirror shows)
    # (and the same fold below a ceiling lower than every light: the lights are behind it, the mirror shows it unlit)
    F.tile(cz(7), [base_surface(sd, 3, alpha=1 - 2.0 ** -13), mirror]); F.tile(cz(7), [solid], y=3.0, up=False)
    B.add("texfold/alpha=1-2^-13:unlit-ceiling", down(cz(7), heights=(2.0,)), shadow=7, secondary=1, hit=True)
    F.tile(cz(5), [base_surface(sd, 4, alpha=0.0), solid])
    B.add("texfold/alpha=0-top", down(cz(5)), secondary=0, hit=True)
    B.close([tile_light(cz(j)) for j in range(7)], 3)
    return B.out, dict(secondary=True, nested=False, refract=False)


# ---------------------------------------------------------------------------------------------------------------- Reflect (Shader.hs:107-118)
def fam_reflect(F):
    sd, B = F.sd, Batches()
    solid = base_surface(sd, 1)
    for j, (refl, ns) in enumerate(((-0.5, 0), (0.0, 0), (0.5, 1), (1.0, 1))):
        F.tile(cz(j), [sd.material_reflect(refl)]); F.tile(cz(j), [solid], y=6.0, up=False)
        # (the one light reaches the ceiling over refl = 0.5 alone, by its radius: the ceiling refl = 1 shows is unlit, and costs no shadow ray)
        B.add("reflect/refl=%g" % refl, down(cz(j)), shadow=1 if j == 2 else 0, secondary=ns, hit=True)
    B.close([light((5.0, 2.0, cz(2) + 3.0), rad=16.0)], 3)
    # the ladder: two facing mirrors at normal incidence; a ray spawns maxdepth - 1 secondary rays (the last Reflect finds recurs - 1 <= 0)
    mirror = sd.material_reflect(1.0)
    F.tile(cz(4), [mirror]); F.tile(cz(4), [mirror], y=4.0, up=False)
    # and one whose upper mirror is a strip: a ray leaning along x (direction (-0.6, -0.8, -0) rounded to fp32, not an equality) leaves the
    # corridor after a few bounces
    F.tile(cz(5), [mirror], half=HALF); F.tile(cz(5) , [mirror], y=4.0, up=False, half=8.0)
    lean = f32([-0.6, -0.8, -0.0]); lean = f32(lean / np.sqrt((lean.astype(np.float64) ** 2).sum()))
    for md in range(1, 9):
        B.add("reflect/ladder:maxdepth=%d" % md, down(cz(4)), shadow=0, secondary=md - 1, hit=True)
        o = [(dx + 6.0, 3.0, cz(5) + dz) for (dx, dz) in GRID]
        B.add("reflect/ladder-leaves:maxdepth=%d" % md, (o, [tuple(lean.tolist())] * len(o)), shadow=0, hit=True)
        B.close([light((5.0, 2.0, cz(4) + 3.0))], md)
    if F.stacks:
        # a Reflect over a Surface: the fold goes on below the mirror's alpha, and the light list is forced late -- in a lean kernel by the
        # per-lane preshade of postshade_lean, not by the wave's eager one.  The light lies in the tangent plane: the count tells.
        F.tile(cz(6), [sd.material_reflect(0.5), solid])
        for md in (1, 3):
            B.add("reflect/over-surface:tangent-light:maxdepth=%d" % md, down(cz(6)), shadow=1, secondary=min(md - 1, 1), hit=True)
            B.add("reflect/over-surface:beside-it-a-mirror:maxdepth=%d" % md, down(cz(3)), secondary=min(md - 1, 1), hit=True)
            B.close([light((20.0, 0.0, cz(6) + 3.0))], md)
    return B.out, dict(secondary=True, nested=False, refract=False)


# ---------------------------------------------------------------------------------------------------------------- Refract (Shader.hs:120-155)
REFRACT_PAIRS = ((0.0, 0.0), (0.25, 0.0), (0.0, 0.5), (0.25, 0.5))


def fam_refract(F):
    sd, B = F.sd, Batches()
    solid = base_surface(sd, 1)
    tiles = [(rr, ior) for ior in (1.5, 1.0, 0.5) for rr in REFRACT_PAIRS]
    for j, ((refl, refr), ior) in enumerate(tiles):  # a slab: its upper face looks up, its lower face down (the two arms of `vdot(n, -d) > 0`), a floor below
        g = sd.material_refract(refl, refr, ior)
        F.tile(cz(j), [g]); F.tile(cz(j), [g], y=-1.0, up=False); F.tile(cz(j), [solid], y=-3.0)
    lights = [light((5.0, -1.5, cz(j) + 3.0)) for j in range(len(tiles))] + [light((0.0, 8.0, cz(5)))]
    for md in (1, 2, 3, 8):
        for j, ((refl, refr), ior) in enumerate(tiles):
            B.add("refract/refl=%g,refr=%g,ior=%g:maxdepth=%d" % (refl, refr, ior, md), down(cz(j)), hit=True)
        B.close(lights, md)
    # around the critical angle: eta * sin = 1.  The exact angle has no dyadic case (eta^2 (1 - c1^2) = 1 has none); sin = 1 / eta +- 2^-10
    # and +- 2^-6 are decided alike by every backend (the directions are rounded to fp32 and renormalised: no equality here)
    lean = f32([0.6, -0.8, -0.0]); lean = f32(lean / np.sqrt((lean.astype(np.float64) ** 2).sum()))
    # (at maxdepth 1 too: the lean kernel's restatement -- both children are traceMiss, and total internal reflection leaves alpha = refr)
    for md in (1, 3):
        for rr in REFRACT_PAIRS:
            jc = tiles.index((rr, 1.5))
            for what, ds in (("+2^-10", 2.0 ** -10), ("-2^-10", -2.0 ** -10), ("+2^-6", 2.0 ** -6), ("-2^-6", -2.0 ** -6)):
                s = 1.0 / 1.5 + ds
                d = f32([s, -np.sqrt(1 - s * s), -0.0]); d = f32(d / np.sqrt((d.astype(np.float64) ** 2).sum()))
                o = [tuple((np.array([dx, 0.0, cz(jc) + dz]) - d.astype(np.float64) * 4.0).tolist()) for (dx, dz) in GRID]
                name = "refract/critical:sin=1/eta%s:maxdepth=%d" % (what, md) + ("" if rr == (0.25, 0.5) else ":refl=%g,refr=%g" % rr)
                B.add(name, (o, [tuple(d.tolist())] * len(o)), secondary=(0 if md == 1 else (1 if ds > 0 else None)) if rr == (0.25, 0.5) else None, hit=True)
        B.close(lights, md)
    # an oblique ray through every slab (direction (0.6, -0.8, -0) rounded to fp32: no equality): it leaves through the lower face with
    # eta = 1 / ior and c1 != -1, the second arm of `vdot(n, -d) > 0` away from normal incidence
    for md in (3, 8):
        for j, ((refl, refr), ior) in enumerate(tiles):
            o = [tuple((np.array([dx, 0.0, cz(j) + dz]) - lean.astype(np.float64) * 2.5).tolist()) for (dx, dz) in GRID]
            B.add("refract/oblique:refl=%g,refr=%g,ior=%g:maxdepth=%d" % (refl, refr, ior, md), (o, [tuple(lean.tolist())] * len(o)), hit=True)
        B.close(lights, md)
    return B.out, dict(secondary=True, nested=False, refract=True)


# ---------------------------------------------------------------------------------------------------------------- Blend / AdditiveLayers
def fam_blend(F):
    sd, B = F.sd, Batches()
    a, b = base_surface(sd, 1), base_surface(sd, 2)
    tiles = [("blend/w=%g" % w, sd.material_blend(a, b, w)) for w in (0.0, 0.5, 1.0)]
    tiles += [("layers/0", sd.material_layers([]))]
    tiles += [("layers/1:alpha=%g" % al, sd.material_layers([base_surface(sd, 3, alpha=al)])) for al in (0.0, 0.5, 1.0, 1.5)]  # aclamp: both arms
    tiles += [("layers/3:alphas=0.5,1.5,0", sd.material_layers([base_surface(sd, 1, alpha=0.5), base_surface(sd, 2, alpha=1.5), base_surface(sd, 3, alpha=0.0)]))]
    m = a
    for depth in range(1, K_MAX_MAT_NEST + 1):  # Blend of AdditiveLayers of Blend ...: kMaxMatNest levels
        m = sd.material_blend(m, b, 0.25) if depth % 2 else sd.material_layers([m, base_surface(sd, depth, alpha=0.5)])
        tiles.append(("nest/%d" % depth, m))
    # a Blend whose first child is a Reflect: the light list is forced by the SECOND child, after a secondary trace has returned
    tiles.append(("blend/reflect-then-surface", sd.material_blend(sd.material_reflect(0.5), a, 0.5)))
    for j, (what, m) in enumerate(tiles):
        F.tile(cz(j), [m])
        B.add(what if what.startswith("blend/") else "blend/" + what, down(cz(j)), hit=True)
    F.tile(cz(len(tiles) - 1), [b], y=6.0, up=False)
    # (the same Blend below a ceiling lower than every light: the lights are behind it, the Reflect child shows it unlit)
    F.tile(cz(len(tiles)), [tiles[-1][1]]); F.tile(cz(len(tiles)), [b], y=3.0, up=False)
    B.add("blend/reflect-then-surface:unlit-ceiling", down(cz(len(tiles)), heights=(2.0,)), hit=True)
    B.close([tile_light(cz(j)) for j in range(0, len(tiles), 2)][:8], 3)
    return B.out, dict(secondary=True, nested=True, refract=False)


# ---------------------------------------------------------------------------------------------------------------- solid textures (tx_weight)
def fam_tx(F):
    sd, B = F.sd, Batches()
    a, b = base_surface(sd, 1), base_surface(sd, 2)
    fns = {"square": api.WEIGHT_STRIPE_SQUARE, "triangle": api.WEIGHT_STRIPE_TRIANGLE, "sine": api.WEIGHT_STRIPE_SINE}
    dzs = [dz + 0.5 for dz in range(-8, 8)]  # 16 z offsets

    def at(z, xs, dzs_=dzs, hs=(3.0, 2.5, 3.5)):
        return down(z, [(x, dz) for x in xs for dz in dzs_ if x != dz], hs)
    # the stripes run along x: pos . axis == x exactly
    for j, (name, fn) in enumerate(fns.items()):
        F.tile(cz(j), [sd.material_blend_fn(a, b, fn, [1.0, 0.0, 0.0])])
    z = cz(0)
    B.add("tx/square:k", at(z, [1.0, 2.0, 5.0]), hit=True)
    B.add("tx/square:k+0.5", at(z, [0.5, 2.5, 7.5]), hit=True)        # `offset < 0.5` is false AT 0.5: weight 1
    B.add("tx/square:k+0.5-ulp", at(z, [ulp(0.5, -1), ulp(2.5, -1), ulp(7.5, -1)]), hit=True)
    B.add("tx/square:k+0.5+ulp", at(z, [ulp(0.5, 1), ulp(2.5, 1), ulp(7.5, 1)]), hit=True)
    B.add("tx/square:k-ulp", at(z, [ulp(1.0, -1), ulp(2.0, -1), ulp(5.0, -1)]), hit=True)
    B.add("tx/square:k+ulp", at(z, [ulp(1.0, 1), ulp(2.0, 1), ulp(5.0, 1)]), hit=True)
    B.add("tx/square:-0.5", at(z, [-0.5]), hit=True)
    B.add("tx/square:-k", at(z, [-1.0, -4.0]), hit=True)
    z = cz(1)
    for fr in (0.0, 0.25, 0.5, 0.75):
        B.add("tx/triangle:%g" % fr, at(z, [fr, 3.0 + fr]), hit=True)
    B.add("tx/triangle:negative", at(z, [-0.25, -2.5, -3.75]), hit=True)
    z = cz(2)
    for q in (0.0, 0.25, 0.5, 0.75):
        B.add("tx/sine:%g" % q, at(z, [q, 2.0 + q, -1.0 + q]), hit=True)
    # Perlin with scale * pos on the integer lattice: every knot's distance vector has a zero weight or a zero dot, the weight is exactly 0.5
    F.tile(cz(3), [sd.material_blend_fn(a, b, api.WEIGHT_PERLIN, [1.0])])
    z = cz(3)
    B.add("tx/perlin:lattice", down(z, [(float(x), float(dz)) for x in range(-4, 5) for dz in range(-4, 5) if x != dz]), hit=True)
    B.add("tx/perlin:cell-centres", down(z, [(x + 0.5, dz + 0.5) for x in range(-4, 4) for dz in range(-4, 4) if x != dz]), hit=True)
    F.tile(8192.0, [sd.material_blend_fn(a, b, api.WEIGHT_PERLIN, [1.0])], half=2048.0)
    B.add("tx/perlin:+-1000", down(8192.0, [(sx * (1000.0 + x), sz * 1000.0 + dz + 0.5) for sx in (-1, 1) for sz in (-1, 1) for x in range(3) for dz in range(3)]), hit=True)
    B.close([tile_light(cz(j)) for j in range(4)] + [light((0.0, 512.0, 8192.0), color=(2.0 ** 20,) * 3)], 3)
    return B.out, dict(secondary=False, nested=True, refract=False)


# ---------------------------------------------------------------------------------------------------------------- Warp (Shader.hs:157-175)
WARP_SHIFT = 4096.0


def fam_warp(F):
    """every tile of the floor carries ONE Warp material.  Its frame -- a group of tiles 2 below the floor, traced through the hit's own ray,
    which starts 3 above the floor: depth 5 -- and its other scene -- tiles WARP_SHIFT along z, traced through the warped ray from the hit
    point up to the frame's depth -- are nodes outside the root; which of them a tile has below it decides the branch."""
    assert F.route == "generic"
    sd, B = F.sd, Batches()
    fcol, scol = base_surface(sd, 1), base_surface(sd, 3)
    variants = [("tie", 2.0, 5.0), ("other-nearer", 2.0, 4.5), ("frame-nearer", 2.0, 5.5), ("both-miss", None, None), ("frame-misses", None, 5.0), ("other-misses", 2.0, None)]
    frame, other = Floor("generic", sd), Floor("generic", sd)
    for j, (what, yf, yo) in enumerate(variants):
        if yf is not None: frame.tile(cz(j), [fcol], y=-yf)
        if yo is not None: other.tile(cz(j) + WARP_SHIFT, [scol], y=-yo)
    own = [light((5.0, 4.0, cz(j) + WARP_SHIFT + 3.0)) for j in (0, 2, 4)]  # the Warp's own light list: three lights; the call's has two
    warp = sd.material_warp(sd.group(frame.items), sd.group(other.items), own, api.compose([api.translate((0.0, 0.0, WARP_SHIFT))]))
    for j in range(len(variants)):
        F.tile(cz(j), [warp])
    call = [light((5.0, -1.0, cz(j) + 3.0)) for j in (1, 4)]
    for md in (1, 2, 3):
        for j, (what, yf, yo) in enumerate(variants):
            ns = 0 if md == 1 else (1 if yf is not None else 0) * 2 + (1 if (yo is not None and not (yf is not None and yo > 5.0)) else 0) * 3
            B.add("warp/%s:maxdepth=%d" % (what, md), down(cz(j)), hit=True, secondary=0 if md == 1 else 2, shadow=ns)
        B.close(call, md)
    return B.out, dict(secondary=True, nested=False, refract=False)


FAMILIES = {"warp": fam_warp, "light": fam_light, "surface": fam_surface, "texfold": fam_texfold, "reflect": fam_reflect, "refract": fam_refract, "blend": fam_blend, "tx": fam_tx}
# which family runs where: a triangle bih carries one texture, so it holds the light list alone; a Mesh one material per
# triangle, so no texture stacks
ROUTES = {"light": ("prims", "prims_full", "bih_tri", "mesh", "generic"),
          "surface": ("prims", "prims_full", "mesh", "generic"),
          "texfold": ("prims", "prims_full", "generic"),
          "reflect": ("prims", "prims_full", "mesh", "generic"),
          "refract": ("prims", "mesh", "generic"),
          "blend": ("prims", "mesh", "generic"),
          "tx": ("prims", "mesh", "generic"),
          "warp": ("generic",)}  # (a Warp material traces other roots than the scene's: the commit puts such a scene on the generic tier)
CASES = [Case(f, r) for f in FAMILIES for r in ROUTES[f]]
# labels about an exact equality: they keep ALL their cases inside the agreement set
EQUALITY = ("light/tangent-", "light/rad", "tx/square:k+0.5", "tx/perlin:lattice", "surface/ks=", "surface/fold:", "texfold/alpha=1-", "light/inside-margin", "light/outside-margin",
            "reflect/ladder:", "reflect/over-surface", "warp/tie")

Scene = namedtuple("Scene", "sd batches traits")


@functools.lru_cache(maxsize=None)
def build(family, route):
    F = Floor(route)
    batches, traits = FAMILIES[family](F)
    return Scene(F.finish(), batches, traits)


CLS_OF = {"prims": ("SPHERE|PRIMS", 1), "prims_full": ("SPHERE|PRIMS", 1), "bih_tri": ("TRI", 1), "mesh": ("MESH", 1)}


def instance_name(family, route, maxdepth, faithful=False, count=False):
    """the trace instance a launch of this family on this route must get, stated from what the family's materials are (not from the
    commit's traits): lean where no secondary trace can do work and nothing nests; the reference's own traversal under a Refract traced
    deeper than the primary ray"""
    t = build(family, route).traits
    if route == "generic": return "k_trace_batch_generic<%s>" % ("counting" if count else "lean")
    full = route == "prims_full" or t["nested"] or (t["secondary"] and maxdepth > 1)
    faithful = faithful or (t["refract"] and maxdepth > 1)
    b = lambda x: "true" if x else "false"
    cls, lb = ("EVERY", 1) if (faithful or count) else CLS_OF[route]
    return "k_trace_batch_flat<%s,%s,%s,%s,%d>" % (b(faithful), b(faithful or count), b(full), cls, lb)


def lean_legal(family, route, maxdepth):
    """does a launch get a lean kernel (trace_primary -> shade_hit_lean)?  The generic tier has none."""
    t = build(family, route).traits
    return route not in ("generic", "prims_full") and not t["nested"] and not (t["secondary"] and maxdepth > 1)


# ---------------------------------------------------------------------------------------------------------------- evaluation
def lights_of(b):
    return [api.light(p, c, r, s) for (p, c, r, s) in b.lights]


def oracle_trace(orc, b):
    """n x 7 (r, g, b, a, depth, shadow rays, secondary rays) from an oracle, one 1 x 1 frame per ray (tests/test_trace_batch.py oracle_trace)"""
    orc.clear_lights()
    for (p, c, r, s) in b.lights:
        lt = api.light(p, c, r, s)  # (the fp32 fields the product gets)
        orc.add_light(list(lt.pos), list(lt.color), lt.rad, bool(lt.shadow))
    out = np.zeros((len(b.o), 7))
    for i in range(len(b.o)):
        # (up = right = -0: get_rayint adds right * -xc and up * yc to fwd, and -0 + +0 would turn a direction's -0 into the +0 that misses every bih, Q1)
        orc.set_camera_vectors(b.o[i].astype(np.float64), b.d[i].astype(np.float64), [-0.0] * 3, [-0.0] * 3)
        img, _, cnt = orc.render(1, 1, maxdepth=b.maxdepth, want_packed=False)
        out[i, :5] = img[0, 0]; out[i, 5] = cnt["rays_shadow"]; out[i, 6] = cnt["rays_secondary"]
    return out


def hostsim_trace(hs, b, full=1, faithful=0, tier=-1):
    """n x 7 from the host build of the device headers (helpers.HostSim.trace)"""
    out, cnt = hs.trace(b.o, b.d, b.lights, b.maxdepth, full, faithful, tier)
    return np.hstack([out.astype(np.float64), cnt.astype(np.float64)])


def same_decision(a, b):
    """hit / miss and both counts"""
    return ((a[:, 4] < MISS_DEPTH) == (b[:, 4] < MISS_DEPTH)) & (a[:, 5] == b[:, 5]) & (a[:, 6] == b[:, 6])


def colour_err(a, ref):
    """the worst channel's |a - ref| / max(1, |ref|) per ray; NaN where both are NaN counts as equal, where one is as infinite"""
    with np.errstate(invalid="ignore"):
        e = np.abs(a[:, :4] - ref[:, :4]) / np.maximum(1.0, np.abs(ref[:, :4]))
    both, one = np.isnan(a[:, :4]) & np.isnan(ref[:, :4]), np.isnan(a[:, :4]) != np.isnan(ref[:, :4])
    return np.where(both, 0.0, np.where(one, np.inf, e)).max(axis=1)


def depth_ok(a, ref):
    hit = ref[:, 4] < MISS_DEPTH
    return ~hit | (np.abs(a[:, 4] - ref[:, 4]) <= parity.T_RTOL * np.maximum(1.0, np.abs(ref[:, 4])))


Eval = namedtuple("Eval", "case scene labels batch_of ref f32_ agree why")


@functools.lru_cache(maxsize=None)
def evaluate(family, route):
    """the two oracles on every case of a family on a route, and the agreement set"""
    sc = build(family, route)
    o64, _, _ = O.load_scene(sc.sd)
    o32, _, _ = O.load_scene(sc.sd, use_float=True)
    ref = np.vstack([oracle_trace(o64, b) for b in sc.batches])
    r32 = np.vstack([oracle_trace(o32, b) for b in sc.batches])
    labels = np.concatenate([b.labels for b in sc.batches])
    batch_of = np.concatenate([np.full(len(b.o), k) for k, b in enumerate(sc.batches)])
    why = {"decision": ~same_decision(r32, ref)}
    why["colour"] = ~why["decision"] & ~(colour_err(r32, ref) <= COLOUR_TOL)
    why["depth"] = ~why["decision"] & ~why["colour"] & ~depth_ok(r32, ref)
    agree = ~(why["decision"] | why["colour"] | why["depth"])
    for a in (ref, r32, labels, batch_of, agree): a.setflags(write=False)
    return Eval(Case(family, route), sc, labels, batch_of, ref, r32, agree, why)


def check_backend(ev, got, what, sel=None):
    """EVERY case of the agreement set (of `sel`, indices into the cases): the oracle's decision and both per-ray counts exactly, every
    colour channel and alpha within COLOUR_TOL, the depth within parity.T_RTOL.  No allowance.  Returns (cases held, worst colour error)."""
    sel = np.arange(len(ev.agree)) if sel is None else np.asarray(sel)
    a, ref, lab = ev.agree[sel], ev.ref[sel], ev.labels[sel]

    def none(bad, msg):
        bad = bad & a
        assert not bad.any(), "%s/%s %s, %s: %d cases of the agreement set, e.g. %s" % (ev.case.family, ev.case.route, what, msg, int(bad.sum()), [
            (str(lab[i]), got[i].tolist(), ref[i].tolist()) for i in np.flatnonzero(bad)[:3]])
    none((got[:, 4] < MISS_DEPTH) != (ref[:, 4] < MISS_DEPTH), "hit / miss")
    none(got[:, 5] != ref[:, 5], "shadow rays")
    none(got[:, 6] != ref[:, 6], "secondary rays")
    e = colour_err(got, ref)
    none(~(e <= COLOUR_TOL), "colour")
    none(~depth_ok(got, ref), "depth")
    return int(a.sum()), float(e[a].max()) if a.any() else 0.0


def interleave(labels):
    """a permutation that deals the cases of a batch out label by label: neighbours in a wave then sit in different branches"""
    order = np.argsort(labels, kind="stable")
    _, start, count = np.unique(labels[order], return_index=True, return_counts=True)
    rank = np.concatenate([np.arange(c) for c in count])
    lab_ix = np.concatenate([np.full(c, k) for k, c in enumerate(count)])
    return order[np.lexsort((lab_ix, rank))]


WAVE = 64


def check_mixing(ev):
    """The interleaved order is no copy of the sorted one, and its waves are mixed in STATE, not in name alone.  Every batch holds more
    than one wave's worth of rays under at least two labels; its interleaved order is not the identity; its first wave holds every label
    (up to 64) and so a primary miss beside hits.  Over the family, some wave holds hits whose shadow counts differ, and -- where the
    family spawns secondary rays -- hits whose secondary counts differ.  Returns the permutations, one per batch."""
    perms, shadow_mixed, secondary_mixed = [], False, False
    for k, bt in enumerate(ev.scene.batches):
        p = interleave(bt.labels)
        names = np.unique(bt.labels)
        assert len(p) > WAVE and len(names) >= 2, (ev.case, k, len(p), names.tolist())
        assert not np.array_equal(p, np.arange(len(p))), (ev.case, k, "the interleaved order is the sorted one")
        first = bt.labels[p][:WAVE]
        assert len(np.unique(first)) == min(len(names), WAVE), (ev.case, k)
        ref = ev.ref[ev.batch_of == k][p]
        hit = ref[:WAVE, 4] < MISS_DEPTH
        assert hit.any() and not hit.all(), (ev.case, k, "no wave holds a miss beside a hit")
        for w in range(0, len(p), WAVE):
            lanes = ref[w:w + WAVE][ref[w:w + WAVE, 4] < MISS_DEPTH]  # (the lanes that hit: a miss spawns nothing)
            shadow_mixed |= len(np.unique(lanes[:, 5])) > 1
            secondary_mixed |= len(np.unique(lanes[:, 6])) > 1
        perms.append(p)
    # (surface and tx: every tile is an opaque Surface, or a Blend of two, under one light list that reaches them all -- one count)
    assert shadow_mixed or ev.case.family in ("surface", "tx"), (ev.case, "no wave holds hits with different shadow counts")
    # (warp: a Warp hit traces its two scenes whatever they hold -- two secondary rays below maxdepth 1, none at it)
    assert secondary_mixed or not ev.ref[:, 6].any() or ev.case.family == "warp", (ev.case, "no wave holds hits with different secondary counts")
    return perms
