"""GPU suite (-m gpu): lattice rays (tests/lattice.py) through the C ABI, case by case.

For every object on every route that can hold it, one scene is committed and the same rays go through glome_rayint_batch,
glome_shadow_batch, glome_inside_batch and glome_trace_batch with want_hit (no lights, maxdepth 1: the wave-wide instances -- the packet
walks, closest_flat<WAVE>, the interpreter's packet service), with faithful = 0 and with faithful = 1.  On the agreement set of the three
CPU evaluations (lattice.evaluate) the device gives the oracle's decision on EVERY case: hit / miss, primitive, texture stack, shadow,
inside, the depth within parity.T_RTOL of the fp64 depth (NaN where the oracle's is NaN, Q2), the normal within 2e-3.  There is no outlier
fraction.  The two trace launches agree bit for bit, and an object's routes agree with each other in every decision.

Not the same rays in both trace launches: the production trace (faithful = 0) refuses a direction that is not unit length (kErrNonUnit),
so it gets the unit-length subset only -- the lattice's unit axis rays and the normalised twins of the aimed families.  The wave-wide
production instances therefore see none of the aimed families as written with non-unit directions, and none of the lattice's directions
with a component of 0.5 or 2 or with two non-zero components; those go through the faithful launch and the three batch seams.

A ray the CPU stage flagged -- the oracle gave it up as diverged, or the host build of the device headers reported a limit -- is in no GPU
batch: the device's loop is the header the host build ran, and a lane that spins 2^20 times on a shared machine adds no information."""
import numpy as np
import pytest

import lattice as LT
from glome_amd import api

pytestmark = pytest.mark.gpu

DECISIONS = ("hit", "id", "shadow", "inside")


def run_route(ctx, name, route):
    """commit, launch, check, release: returns (evaluation, the device's decisions on every ray it was given, the indices it was given)"""
    ev = LT.evaluate(name, route)
    rays = ev.rays
    sel = np.flatnonzero(~ev.flagged)
    assert not ev.flagged[sel].any() and not np.any(ev.agree & ev.flagged)  # no GPU batch holds a flagged ray
    assert len(sel) >= 0.98 * len(ev.flagged)
    o, d, tm = rays.o[sel], rays.d[sel], rays.tmax[sel]
    assert o.dtype == np.float32 and d.dtype == np.float32 and np.signbit(d[d == 0]).any()
    b = api.Builder()
    nm, _ = ev.sd.replay(b)
    sc = ctx.commit(b, nm[ev.sd.root])
    try:
        assert sc.info()["tier"] == LT.route_traits(name, route)["tier"]
        what = "%s on %s: " % (name, route)
        got = sc.rayint(o, d, tm)
        shadow = sc.shadow(o, d, tm)
        inside = sc.inside(o)
        held = LT.check_backend(ev, got, shadow, inside, nm=nm, what=what + "rayint / shadow / inside", sel=sel)
        assert held == int(ev.agree.sum())
        faithful = sc.trace(o, d, [], tmax=tm, params=api.trace_params(maxdepth=1, faithful=1), want_hit=True)
        LT.check_backend(ev, faithful, nm=nm, what=what + "trace, faithful", sel=sel)
        unit = np.flatnonzero(LT.unit_length(d))  # (a production trace takes unit directions only: the lattice's axis rays and the normalised twins)
        assert len(unit) >= 256
        lean = sc.trace(o[unit], d[unit], [], tmax=tm[unit], params=api.trace_params(maxdepth=1), want_hit=True)
        LT.check_backend(ev, lean, nm=nm, what=what + "trace", sel=sel[unit])
        a = ev.agree[sel[unit]]
        for k in ("t", "prim", "n", "tex"):
            x, y = np.ascontiguousarray(lean[k][a]), np.ascontiguousarray(faithful[k][unit][a])
            same = np.array_equal(x.view(np.uint32), y.view(np.uint32)) if x.dtype == np.float32 else np.array_equal(x, y)
            assert same, what + "the production trace and the faithful one differ in " + k
    finally:
        sc.release()
    n = len(ev.flagged)
    dec = {"hit": np.zeros(n, bool), "id": np.full(n, -3), "shadow": np.zeros(n, bool), "inside": np.zeros(n, bool)}
    dec["hit"][sel] = LT.hit_of(got["t"]); dec["id"][sel] = LT._ids(got["prim"], nm); dec["shadow"][sel] = shadow; dec["inside"][sel] = inside
    return ev, dec


def comparable(ev_a, ev_b):
    """pairs (index in a, index in b) of rays that are one ray in both routes' scenes: the k-th ray of a label both routes have in equal
    number (a route may leave a family out, or keep a part of it) -- where neither route moves the object the rays must be equal bit for
    bit (the lattice is shifted on some routes), else they are the aimed families as written, which were moved with the object"""
    ia, ib = [], []
    for lab in np.unique(ev_a.rays.labels):
        a, b = np.flatnonzero(ev_a.rays.labels == lab), np.flatnonzero(ev_b.rays.labels == lab)
        if len(a) != len(b): continue
        same = np.all(ev_a.rays.o[a] == ev_b.rays.o[b], axis=1) & np.all(ev_a.rays.d[a] == ev_b.rays.d[b], axis=1)
        moved = np.full(len(a), not lab.startswith(("lattice", "bih:"))) & ev_a.rays.exact[a] & ev_b.rays.exact[b]
        ia.append(a[same | moved]); ib.append(b[same | moved])
    return np.concatenate(ia), np.concatenate(ib)


@pytest.mark.parametrize("name", sorted(LT.OBJECTS))
def test_every_case_of_the_agreement_set(gpu_ctx, name):
    obj = LT.OBJECTS[name]
    done = {}
    for route in obj.routes:
        done[route] = run_route(gpu_ctx, name, route)
    ev_a, dec_a = done[obj.routes[0]]
    ref_a = {"hit": LT.hit_of(ev_a.ref["t"]), "id": ev_a.prim_ref, "shadow": ev_a.ref_shadow, "inside": ev_a.ref_inside}
    for route in obj.routes[1:]:
        if route in ("bih_tri", "mesh"): continue  # (another scene: the triangle among eleven others, numbered differently)
        ev_b, dec_b = done[route]
        ref_b = {"hit": LT.hit_of(ev_b.ref["t"]), "id": ev_b.prim_ref, "shadow": ev_b.ref_shadow, "inside": ev_b.ref_inside}
        ia, ib = comparable(ev_a, ev_b)
        m = ev_a.agree[ia] & ev_b.agree[ib]
        for k in DECISIONS:  # where the fp64 oracle answers one thing on both routes (beside the object a route has others, which a ray may meet first)
            m = m & (ref_a[k][ia] == ref_b[k][ib])
        assert m.sum() >= LT.MIN_PER_LABEL, (route, int(m.sum()))  # (not vacuous: as many as a label must keep)
        for k in DECISIONS:
            assert np.array_equal(dec_a[k][ia][m], dec_b[k][ib][m]), "%s: %s and %s disagree in %s" % (name, obj.routes[0], route, k)
