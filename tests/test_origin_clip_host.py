"""The production walks of a triangle or sphere BIH start at the ray's origin (bih_clip_root_at_origin, glome_amd/csrc/rt_device.hpp):
near = max(near, -FLT_MIN) after the root interval is formed.  The reference does not clip, and neither do the faithful and the counting
instances; this file holds the clipped walks to them on rays for which the clip matters -- rays that start INSIDE the tree's bounds --
through tests/hostsim (no GPU): the production tier is `analysis = 0`, the faithful counting tier `analysis = 1`, each per lane and (+ 2)
through the wave entry bih_tri_wave -- for the closest-hit walks (hostsim_rayint).  hostsim_shadow has the per-lane any-hit walk only
(bih_tri<2>): the clipped any-hit WAVE walk, bih_tri_wave<2, false, *, true> with the hand-written walk or the C++ packet walk under it, is
not reached on the host; tests/test_origin_clip_gpu.py covers it (the shadow rays of a frame's and of a stream's hits).

Occlusion.  hostsim_shadow runs the production any-hit walk; the unclipped any-hit walk it is compared with is the generic tier's over the
same flattened scene (tier = 1: vm_occluded<true>, a counting instance, whose BIH walks are not clipped), and, for triangles, the faithful
closest-hit walk asked for a hit up to the same limit (tri_test accepts the same hits in both modes; sphere_shadow and sphere_test differ
by design, Sphere.hs:51-71).

Scenes: the terrain scenes.s3(32) (2,048 triangles) and a soup of 300 spheres (zoo.soup).  Every set of rays is made once per scene and
shared."""
import numpy as np
import pytest

import zoo
from helpers import HostSim
from glome_amd import api, scenes

KDEL = 1.0e-4  # Vec.hs:40


def _bih_ids(sd, nm):
    """builder ids of the SceneDesc's bih nodes, in the order they were made (tests/test_hostsim_parity.py)"""
    nid, out = 0, []
    for kind, name, args in sd.ops:
        if kind == "N":
            nid += args[0].shape[0]
        elif kind == "n":
            if name == "bih":
                out.append(nm[nid])
            nid += 1
    return out


def _unit32(d):
    d = np.asarray(d, np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


SIGNS = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float32)


class Case:
    def __init__(self, sd, seed):
        self.sd = sd
        self.b = api.Builder()
        self.nm, _ = sd.replay(self.b)
        self.hs = HostSim(self.b, self.nm[sd.root])
        assert self.hs.info()["tier"] == 0
        (self.bih,) = _bih_ids(sd, self.nm)
        bb = self.b.bound(self.bih)
        self.lo, self.hi = bb[:3], bb[3:]
        self.ls, self.rs, self.ax, self.nl, _ = self.b.bih_dump(self.bih)
        self.light = np.array(sd.lights[0][0], np.float64)
        rng = np.random.default_rng(seed)
        # ---- a few thousand random rays from inside the bounds
        o = rng.uniform(self.lo, self.hi, (3000, 3)).astype(np.float32)
        d = _unit32(rng.normal(size=(3000, 3)))
        # ---- rays pointing straight out of the bounds: away from its centre, and along the axes (two components exactly zero, both signs of zero)
        oc = rng.uniform(self.lo, self.hi, (600, 3)).astype(np.float32)
        dc = _unit32(oc.astype(np.float64) - 0.5 * (self.lo + self.hi))
        oa = rng.uniform(self.lo, self.hi, (48, 3)).astype(np.float32)
        da = np.zeros((48, 3), np.float32)
        for i in range(48):
            da[i] = [0.0 if (i // 12) % 2 == 0 else -0.0] * 3
            da[i, i % 3] = 1.0 if (i // 3) % 2 == 0 else -1.0
        self.o = np.concatenate([o, oc, oa]); self.d = np.concatenate([d, dc, da])
        inside = np.all((self.o >= self.lo) & (self.o <= self.hi), axis=1)
        assert inside.all()
        # ---- shadow rays from actual hit points towards the light: primary rays of the scene's camera, lifted off the hit by delta along the normal
        cam = api.camera(*sd.cam)
        po, pd = api.frame_rays(cam, 96, 54)
        h = self.hs.rayint(po, pd)
        hit = h["t"] >= 0
        assert hit.sum() > 500
        p = po[hit].astype(np.float64) + h["t"][hit, None].astype(np.float64) * pd[hit].astype(np.float64)
        n = h["n"][hit].astype(np.float64)
        # (towards the scene's light, and towards a second one low over the horizon: on the small terrain nothing stands in the way of the first)
        sets = []
        for light in (self.light, self.light * np.array([1.0, 0.08, 1.0])):
            lv = light - p
            nn = np.where((np.einsum("ij,ij->i", lv, n) < 0)[:, None], -n, n)
            ll = np.linalg.norm(lv, axis=1)
            sets.append(((p + KDEL * nn).astype(np.float32), _unit32(lv), (ll - 2 * KDEL).astype(np.float32)))
        self.so, self.sd_, self.sl = (np.concatenate([a[k] for a in sets]) for k in range(3))
        for a in (self.o, self.d, self.so, self.sd_, self.sl):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def terrain(built):
    return Case(scenes.s3(32), 21)


@pytest.fixture(scope="module")
def spheres(built):
    return Case(zoo.soup(300, seed=5, spheres=True, floor=False), 22)


def _same_hits(a, b):
    return (np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32)) and np.array_equal(a["prim"], b["prim"])
            and np.array_equal(a["n"].view(np.uint32), b["n"].view(np.uint32)))


def _check_closest(hs, o, d, tmax=1e6):
    """hit, primitive and the bits of t (and of the normal): the production tier == the faithful tier, per lane and through the wave entry"""
    ref = hs.rayint(o, d, tmax, analysis=1)
    for analysis in (0, 2, 3):
        got = hs.rayint(o, d, tmax, analysis=analysis)
        bad = np.flatnonzero((got["t"].view(np.uint32) != ref["t"].view(np.uint32)) | (got["prim"] != ref["prim"]))
        assert _same_hits(got, ref), (analysis, bad[:8], len(bad))
    return ref


def _check_occlusion(c, o, d, tmax):
    got = c.hs.shadow(o, d, tmax)
    ref = c.hs.shadow(o, d, tmax, tier=1)  # the generic tier's any-hit walk: not clipped
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]
    return got


@pytest.mark.parametrize("which", ["terrain", "spheres"])
def test_rays_from_inside_the_bounds(request, which):
    c = request.getfixturevalue(which)
    ref = _check_closest(c.hs, c.o, c.d)
    assert 0.05 < (ref["t"] >= 0).mean() < 0.95  # both outcomes are common
    rng = np.random.default_rng(4)
    tm = rng.uniform(0.05, 12.0, len(c.o)).astype(np.float32)
    _check_closest(c.hs, c.o, c.d, tm)  # a limit of its own on every ray
    occ = _check_occlusion(c, c.o, c.d, tm)
    assert 0.02 < occ.mean() < 0.98
    if which == "terrain":  # tri_test accepts the same hits in both modes: occluded == the faithful closest-hit walk finds something up to the limit
        assert np.array_equal(occ, c.hs.rayint(c.o, c.d, tm, analysis=1)["t"] >= 0)


@pytest.mark.parametrize("which", ["terrain", "spheres"])
def test_shadow_rays_from_hit_points(request, which):
    c = request.getfixturevalue(which)
    assert np.all((c.so >= c.lo) & (c.so <= c.hi))  # they start inside the bounds
    occ = _check_occlusion(c, c.so, c.sd_, c.sl)
    assert 0 < occ.sum() < len(occ)
    _check_closest(c.hs, c.so, c.sd_, c.sl)
    if which == "terrain":
        assert np.array_equal(occ, c.hs.rayint(c.so, c.sd_, c.sl, analysis=1)["t"] >= 0)


# The faithful counting tier counts the reference's interval, clipped nowhere: bih_nodes and prim_tests of the rays above, computed once with
# the library as it was before the production walks were clipped (per lane and through the wave entry: the same numbers).
PARENT_COUNTS = {
    "terrain": {"inside": (120626, 32018), "shadow": (195919, 57973)},
    "spheres": {"inside": (87536, 69833), "shadow": (57002, 45362)},
}


@pytest.mark.parametrize("which", ["terrain", "spheres"])
def test_the_counting_tier_still_counts_the_reference_interval(request, which):
    c = request.getfixturevalue(which)
    for analysis in (1, 3):
        cnt = c.hs.rayint(c.o, c.d, analysis=analysis)["counters"]
        assert (int(cnt[0]), int(cnt[2])) == PARENT_COUNTS[which]["inside"], analysis
        cnt = c.hs.rayint(c.so, c.sd_, c.sl, analysis=analysis)["counters"]
        assert (int(cnt[0]), int(cnt[2])) == PARENT_COUNTS[which]["shadow"], analysis


def _directions(extra):
    """each direction of `extra` and a diagonal, with every pattern of signs: all eight octants"""
    base = np.concatenate([np.asarray(extra, np.float64).reshape(-1, 3), [[1.0, 1.0, 1.0], [0.3, 0.9, 0.2]]])
    base = np.abs(base) + 1e-3  # (no zero component: the sign patterns are eight different octants)
    return _unit32((base[:, None, :] * SIGNS[None].astype(np.float64)).reshape(-1, 3))


def test_origins_exactly_on_a_triangle(terrain):
    """Terrain vertices: o - p1 = 0, so the triangle is hit at t = 0 exactly.  From each, rays along the triangle's normal, along its two edges
    (in the surface) and two diagonals, each with every pattern of signs, and the four exact directions.  The expected answer is the faithful
    tier's; many of these rays do hit at t = 0 there."""
    c = terrain
    T = scenes.heightfield_triangles(32).astype(np.float32)
    rng = np.random.default_rng(8)
    os_, ds = [], []
    for k in rng.choice(len(T), 160, replace=False):
        p1, p2, p3 = T[k, 0:3], T[k, 3:6], T[k, 6:9]
        nrm = np.cross((p2 - p1).astype(np.float64), (p3 - p1).astype(np.float64))
        dirs = _directions([nrm, p2 - p1, p3 - p1])
        dirs = np.concatenate([dirs, _unit32([nrm, -nrm, (p2 - p1).astype(np.float64), (p3 - p1).astype(np.float64)])])  # and the exact ones
        os_.append(np.repeat(p1[None], len(dirs), 0)); ds.append(dirs)
    o, d = np.concatenate(os_), np.concatenate(ds)
    ref = _check_closest(c.hs, o, d)
    assert int((ref["t"] == 0).sum()) >= 100, int((ref["t"] == 0).sum())  # not vacuous: the faithful tier hits at t = 0
    occ = _check_occlusion(c, o, d, np.float32(30.0))
    assert np.array_equal(occ, c.hs.rayint(o, d, 30.0, analysis=1)["t"] >= 0)
    assert occ.sum() >= 100


def test_origins_exactly_on_a_split_plane_of_the_terrain(terrain):
    """The planes of the tree (glome_sb_bih_dump; the builder sets them two deltas off the grid lines) as the walk reads them, in fp32: the origin
    has exactly that coordinate -- the distance to the plane is +-0, the child's interval ends or begins at the origin -- and lies on the
    terrain's surface there (to rounding), or just above it.  The rays leave along the axis, along the surface and diagonally, with every pattern
    of signs.  Some hit within a few ulps of the origin in the faithful tier -- not at t = 0 exactly: the builder's planes stand off their
    items, so no item of a child touches the plane that ends it.  The exact case, t == 0 in a child whose interval ends at +-0, is the next
    test's (a tree given as text), and test_a_sphere_through_an_origin_on_the_plane_that_ends_its_child's for spheres."""
    c = terrain
    V = scenes.heightfield_vertices(32)
    rng = np.random.default_rng(10)
    os_, ds = [], []
    idx = np.flatnonzero((c.ax == 0) | (c.ax == 2))
    for k in rng.choice(idx, 80, replace=False):
        a = int(c.ax[k])
        for plane in (np.float32(c.ls[k]), np.float32(c.rs[k])):
            if not abs(plane) < 9.9:
                continue
            for lift in (0.0, 1e-3):
                q = rng.uniform(-9.9, 9.9, 3)
                q[a] = float(plane)
                # the height of the surface at (x, z): the cell's two triangles (scenes.heightfield_triangles)
                fi, fj = (q[0] + 10.0) * 32 / 20.0, (q[2] + 10.0) * 32 / 20.0
                i, j = int(fi), int(fj)
                u, w = fi - i, fj - j
                ya, yb, yc, yd = V[i, j, 1], V[i, j + 1, 1], V[i + 1, j, 1], V[i + 1, j + 1, 1]
                q[1] = (ya + u * (yc - ya) + w * (yb - ya) if u + w <= 1 else yd + (1 - u) * (yb - yd) + (1 - w) * (yc - yd)) + lift
                o = q.astype(np.float32)
                assert o[a] == plane
                e = np.zeros(3); e[a] = 1.0
                dirs = _directions([e, [1.0, 0.0, 1.0]])
                os_.append(np.repeat(o[None], len(dirs), 0)); ds.append(dirs)
    o, d = np.concatenate(os_), np.concatenate(ds)
    ref = _check_closest(c.hs, o, d)
    assert int(((ref["t"] >= 0) & (ref["t"] < 1e-5)).sum()) >= 20  # not vacuous: hits at the origin itself
    occ = _check_occlusion(c, o, d, np.float32(30.0))
    assert np.array_equal(occ, c.hs.rayint(o, d, 30.0, analysis=1)["t"] >= 0)


def test_a_triangle_through_an_origin_on_the_plane_that_ends_its_child(built):
    """The case that rules out clipping at 0 itself.  A tree given as text (glome_sb_load_show takes it as printed; the builder's own planes
    stand two deltas off its items): the left child's triangle reaches its plane x = 1 exactly, at its vertex (1, 0, 0); so does the right
    child's, at (1, 5, 5).  A ray that leaves such a vertex AWAY from the child has that child as its near child, with an interval that ends at
    +-0: the reference enters it (near < 0 < +-0 there) and hits the triangle at t = 0.  With near = -FLT_MIN the walk still does; with
    near = 0 it would not, and the ray would miss."""
    text = ("SI Bih {bihbb = Bbox {p1 = Vec (-1.0e-4) (-1.0e-4) (-1.0e-4), p2 = Vec 2.0001 6.0001 6.0001}, bihroot = BihBranch 1.0 1.0 0 "
            "(BihLeaf [SI Triangle (Vec 1.0 0.0 0.0) (Vec 0.0 1.0 0.0) (Vec 0.0 0.0 1.0)]) "
            "(BihLeaf [SI Triangle (Vec 1.0 5.0 5.0) (Vec 2.0 6.0 5.0) (Vec 2.0 5.0 6.0)])}")
    b = api.Builder()
    m = b.material_surface((1, 1, 1), 1, 0.2, 0.8, 0, 0)
    root, _ = b.load_show(text, default_material=m)
    assert b.show(root) == text
    hs = HostSim(b, root)
    dirs = _directions([[1.0, 0.0, 0.0], [3.0, 1.0, 2.0]])
    for vertex, away in (((1.0, 0.0, 0.0), 1.0), ((1.0, 5.0, 5.0), -1.0)):
        o = np.repeat(np.float32([vertex]), len(dirs), 0)
        ref = _check_closest(hs, o, dirs)
        leaving = dirs[:, 0] * away > 0  # the vertex's own child is the near child, and ends at the origin
        assert leaving.sum() == len(dirs) // 2 and np.all(ref["t"][leaving] == 0), ref["t"][leaving]  # not vacuous: hit at t = 0 in the faithful tier
        occ = hs.shadow(o, dirs, np.float32(30.0))
        assert np.array_equal(occ, hs.shadow(o, dirs, np.float32(30.0), tier=1)) and np.array_equal(occ, hs.rayint(o, dirs, 30.0, analysis=1)["t"] >= 0)
        assert occ[leaving].all()


def test_origins_on_split_planes_and_on_spheres_of_the_sphere_tree(spheres):
    """The builder's sphere tree.  (a) Origins with one coordinate exactly a split plane of the tree (the distance to that plane is +-0), anywhere
    in the bounds otherwise -- the builder's planes stand two deltas off the spheres, so no such origin lies on a sphere.  (b) Origins on a
    sphere's surface, to rounding: its six extreme points c +- r e_a, rays leaving outwards, along the surface and inwards.  Rays along the
    axis, diagonal, with every pattern of signs.  Neither gives a hit at t == 0 in a child that ends at the origin -- that takes a plane that
    touches its sphere: the next test."""
    c = spheres
    branch = c.ax >= 0
    rng = np.random.default_rng(9)
    lo, hi = c.lo, c.hi
    os_, ds = [], []
    idx = rng.choice(np.flatnonzero(branch), 120, replace=False)
    for k in idx:
        a = int(c.ax[k])
        for plane in (np.float32(c.ls[k]), np.float32(c.rs[k])):
            if not np.isfinite(plane):
                continue
            o = rng.uniform(lo, hi).astype(np.float32)
            o[a] = plane  # exactly on the plane; the other coordinates anywhere in the bounds
            e = np.zeros(3); e[a] = 1.0
            dirs = _directions([e])
            os_.append(np.repeat(o[None], len(dirs), 0)); ds.append(dirs)
    o, d = np.concatenate(os_), np.concatenate(ds)
    ref = _check_closest(c.hs, o, d)
    assert (ref["t"] >= 0).sum() >= 100
    _check_occlusion(c, o, d, np.float32(30.0))
    # (b) on the spheres
    sph = np.array([list(op[2][0]) + [op[2][1]] for op in c.sd.ops if op[0] == "n" and op[1] == "sphere"], np.float64)
    assert len(sph) == 300
    os_, ds = [], []
    for k in rng.choice(len(sph), 60, replace=False):
        for a in range(3):
            for sg in (1.0, -1.0):
                e = np.zeros(3); e[a] = sg
                o = (sph[k, :3] + sph[k, 3] * e).astype(np.float32)
                dirs = _directions([e])
                os_.append(np.repeat(o[None], len(dirs), 0)); ds.append(dirs)
    o, d = np.concatenate(os_), np.concatenate(ds)
    ref = _check_closest(c.hs, o, d)
    assert int(((ref["t"] >= 0) & (ref["t"] < 1e-5)).sum()) >= 100  # hits at the origin itself, to rounding
    _check_occlusion(c, o, d, np.float32(30.0))


def test_a_sphere_through_an_origin_on_the_plane_that_ends_its_child(built):
    """The sphere form (sphere_test, LEAFK = 1) of the case that rules out clipping at 0.  A tree given as text: the left child's unit sphere
    around the origin of the axes touches its plane x = 1 at (1, 0, 0), the right child's around (2, 5, 5) touches the same plane at (1, 5, 5).
    A ray that leaves the touching point AWAY from the sphere has the sphere's child as its near child, with an interval that ends at +-0;
    rayint_sphere's far root v + sqrt(disc) is then 0 up to rounding, and for many directions exactly 0: the reference hits the sphere at t = 0
    there.  The expected answer is the faithful tier's, and it must contain such hits.  (The any-hit form cannot: sphere_shadow rejects a
    sphere whose centre lies behind the ray, v > 0 fails, and with v > 0 both roots are positive -- no accepted distance is 0; the booleans are
    compared all the same.)"""
    text = ("SI Bih {bihbb = Bbox {p1 = Vec (-1.0) (-1.0) (-1.0), p2 = Vec 3.0 6.0 6.0}, bihroot = BihBranch 1.0 1.0 0 "
            "(BihLeaf [SI Sphere (Vec 0.0 0.0 0.0) 1.0 1.0]) (BihLeaf [SI Sphere (Vec 2.0 5.0 5.0) 1.0 1.0])}")
    b = api.Builder()
    m = b.material_surface((1, 1, 1), 1, 0.2, 0.8, 0, 0)
    root, _ = b.load_show(text, default_material=m)
    assert b.show(root) == text
    hs = HostSim(b, root)
    rng = np.random.default_rng(14)
    dirs = _unit32(rng.normal(size=(4000, 3)))
    dirs = dirs[np.all(dirs != 0, axis=1)]
    for point, away in (((1.0, 0.0, 0.0), 1.0), ((1.0, 5.0, 5.0), -1.0)):
        o = np.repeat(np.float32([point]), len(dirs), 0)
        ref = _check_closest(hs, o, dirs)
        leaving = dirs[:, 0] * away > 0  # the touching sphere's child is the near child, and ends at the origin
        at0 = leaving & (ref["t"] == 0)
        assert at0.sum() >= 100, int(at0.sum())  # not vacuous: hits at t = 0 exactly in the faithful tier, in the child that ends there
        occ = hs.shadow(o, dirs, np.float32(30.0))
        assert np.array_equal(occ, hs.shadow(o, dirs, np.float32(30.0), tier=1))


def test_one_leaf_trees_are_tested_regardless(built):
    """A tree that is one leaf is tested whatever its interval (Bih.hs:339) -- also by the clipped walks: origin outside the bounds, ray pointing
    away; and the documented Refract case, a direction that is not unit length at a sphere, for which rayint_sphere reports hits where the line
    misses the sphere (Shader.hs:141, Sphere.hs:20-41)."""
    for item in ("sphere", "triangle"):
        sd = zoo.SceneDesc()
        mat = scenes.matte(sd, (0.7, 0.6, 0.5))
        prim = sd.sphere((0.0, 1.0, 0.0), 0.5) if item == "sphere" else sd.triangle((-1.0, 0.5, 0.0), (1.0, 0.5, 0.0), (0.0, 1.5, 0.2))
        sd.set_root(sd.tex(sd.bih([prim]), mat))
        scenes._common(sd, 1)
        b = api.Builder()
        nm, _ = sd.replay(b)
        (bih,) = _bih_ids(sd, nm)
        assert len(b.bih_dump(bih)[3]) == 1  # a single node: the root leaf
        hs = HostSim(b, nm[sd.root])
        rng = np.random.default_rng(12)
        o = (np.array([0.0, 1.0, 0.0]) + _unit32(rng.normal(size=(400, 3))) * rng.uniform(0.8, 4.0, (400, 1))).astype(np.float32)
        away = _unit32(o.astype(np.float64) - np.array([0.0, 1.0, 0.0]))
        towards = -away
        scale = rng.uniform(0.3, 3.0, (400, 1)).astype(np.float32)
        for d in (away, towards, away * scale, towards * scale):  # (a non-unit ray through rayint goes to the faithful instance, as in the product)
            ref = _check_closest(hs, o, d)
            got = hs.shadow(o, d, np.float32(50.0))
            assert np.array_equal(got, hs.shadow(o, d, np.float32(50.0), tier=1))
        assert (hs.rayint(o, towards, analysis=1)["t"] >= 0).any()
        if item == "sphere":
            # the Refract case: a direction that is not unit length, on a line that passes the sphere (and its box) at 1.5 radii -- with |d| = 1 a
            # miss, with |d| = 3 rayint_sphere's formula reports a hit, in the faithful tier and in the production any-hit walk alike
            cen = np.array([0.0, 1.0, 0.0])
            side = np.cross(away.astype(np.float64), rng.normal(size=(400, 3)))
            side /= np.linalg.norm(side, axis=1, keepdims=True)
            past = _unit32(cen + 0.75 * side - o.astype(np.float64))
            assert not (hs.rayint(o, past, analysis=1)["t"] >= 0).any()
            long_d = past * np.float32(3.0)
            f = _check_closest(hs, o, long_d)
            assert (f["t"] >= 0).sum() >= 100, int((f["t"] >= 0).sum())  # the case exists
            occ = hs.shadow(o, long_d, np.float32(50.0))
            assert np.array_equal(occ, hs.shadow(o, long_d, np.float32(50.0), tier=1))


def test_the_deep_streams_of_the_ladder_keep_their_overflow(built):
    """tests/test_packet_walk_edges.py reaches the overflow path of the hand-written walk with streams that hold 16 pending entries.  Their rays
    start INSIDE the ladder's bounds (between the screen and the nearest rung; the shadow rays on the screen) and run towards the far end: the
    pending entries are far children AHEAD of the origin.  Modelled (tests/packet_walk_model.py, origin_clip) with the root interval clipped as the production
    walk now clips it: the same depth, pushes and pops beyond the LDS part as with the reference interval, in every packet."""
    import ladder
    import packet_walk_model as PM
    from oracle import np_scene as NS
    for v in ((0, 1), (1, -1)):
        lad = ladder.Ladder(*v)
        sc, nm = NS.load(lad.sd)
        bih = sc.nodes[nm[lad.bih_id]]
        o, d, _ = lad.deep_set()
        lo, hi = np.asarray(bih.bb[0]), np.asarray(bih.bb[1])
        assert np.all((o >= lo) & (o <= hi))  # the deep streams start inside the root box
        ref = PM.walk_stream(bih, o, d, 1e6, 1)
        t = np.concatenate([r["t"] for r in PM.walk_stream(bih, *lad.shadow_set()[:2], 1e6, 1)])
        so, sd_, sl = ladder.shadow_rays(lad, *lad.shadow_set()[:2], t)
        assert np.all((so >= lo) & (so <= hi))
        sref = PM.walk_stream(bih, so, sd_, sl, 2)
        got = PM.walk_stream(bih, o, d, 1e6, 1, origin_clip=True)
        sgot = PM.walk_stream(bih, so, sd_, sl, 2, origin_clip=True)
        for a, b in list(zip(ref, got)) + list(zip(sref, sgot)):
            assert [(w.octant, w.lanes, w.max_depth, w.pushes_over, w.pops_over) for w in a["walks"]] == [(w.octant, w.lanes, w.max_depth, w.pushes_over, w.pops_over) for w in b["walks"]]
            assert all(w.max_depth >= 15 and w.pushes_over >= 1 and w.pops_over >= 1 for w in b["walks"])
            assert np.array_equal(a["prim"], b["prim"])
