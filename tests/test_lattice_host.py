"""CPU suite: lattice rays (tests/lattice.py) through the host build of the device headers, case by case.

  - every route is what it claims to be: the tier, the entry classes and the trace instance come from the commit's own traits
    (HostSim.info, glome_sb_scene_traits, glome_trace_kernel_choice), so a route that falls back to another kernel class fails here;
  - every aimed family reaches its branch: its label is checked against what the fp64 oracle answers;
  - the agreement set cannot hide a failure: per object and route at most 2 % of the cases lie outside it and every label keeps at least 32
    cases inside it;
  - inside the set the host build is held on every case, normals included (lattice.check_backend), also in its faithful traversal;
  - the runaway contract: a ray the bounded oracle gives up as diverged ends in a limit status, not in an answer.

The counts outside the set, per object, route and label, are in profiles/lattice_agreement.txt, which a test holds to what is computed."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import lattice as LT
import test_trace_choice as trace_choice
from helpers import HostSim
from glome_amd import _lib as L
from glome_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "lattice_agreement.txt")
IDS = ["%s-%s" % c for c in LT.CASES]


def test_the_table_holds_the_objects_and_routes_it_should():
    assert {"sphere", "box", "cyl_z", "cyl_y", "cone_z", "cone_y", "disc", "plane", "triangle", "difference", "intersection3", "trianglenorm", "difference_retexture",
            "bound", "innerbound", "noshadow", "onlyshadow", "intersection7"} <= set(LT.OBJECTS)
    routes = {r for _, r in LT.CASES}
    assert routes == {"alone", "list", "bih_simple", "instance", "instance_bih", "generic", "bih_sphere", "bih_tri", "mesh"}
    assert len(set(LT.CASES)) == len(LT.CASES)


@pytest.mark.parametrize("name,route", LT.CASES, ids=IDS)
def test_route_is_what_it_claims(built, name, route):
    sd, node, parts, M = LT.build_scene(name, route)
    b = api.Builder()
    nm, _ = sd.replay(b)
    want = LT.route_traits(name, route)
    assert HostSim(b, nm[sd.root]).info()["tier"] == want["tier"]
    lib = L.load()
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(b.h, nm[sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    assert t[0] == want["tier"]
    if want["tier"] == 0:
        assert (t[1] & want["has"]) == want["has"] and (t[1] & want["hasnot"]) == 0, (int(t[1]), want)
    inst, _, _ = trace_choice.export_choice(lib, [list(t[:8]) + [0, 0, 1]])[0].tolist()
    assert trace_choice.instance_name(inst) == want["trace"], dict(zip(trace_choice.COLS, t[:8].tolist()))
    inst, _, _ = trace_choice.export_choice(lib, [list(t[:8]) + [1, 0, 1]])[0].tolist()  # the faithful launch of the GPU suite
    assert trace_choice.instance_name(inst) == ("k_trace_batch_flat<true,true,false,EVERY,1>" if want["tier"] == 0 else "k_trace_batch_generic<lean>")


def check_labels(ev):
    """every aimed family against what the fp64 oracle answers: a generator that does not reach its branch fails here.  Where a family
    states the decision, the host build gives it on EVERY ray of the family, flagged ones apart: the agreement set is made with the host
    build's own answers, so a branch it gets wrong would otherwise only shrink the set."""
    ref = ev.ref
    for lab, sl, e, exact in ev.rays.expect:
        hit = LT.hit_of(ref["t"][sl])
        if "hit" in e:
            assert np.all(hit == e["hit"]), (lab, "hit", int(hit.sum()), len(hit))
            ok = ~ev.flagged[sl]
            assert np.all(LT.hit_of(ev.hs["t"][sl])[ok] == e["hit"]), (lab, "the host build's hit / miss", int(LT.hit_of(ev.hs["t"][sl])[ok].sum()), int(ok.sum()))
            if e.get("nan"):
                assert np.all(np.isnan(ev.hs["t"][sl][ok])), (lab, "the host build's NaN depth")
        if "inside" in e:
            assert np.all(ev.hs_inside[sl] == e["inside"]), (lab, "the host build's inside")
        if e.get("nan"):
            assert np.all(np.isnan(ref["t"][sl])), (lab, "a NaN depth (Q2)")
        if "t" in e and exact:
            assert np.allclose(ref["t"][sl], np.asarray(e["t"], np.float64), rtol=0, atol=1e-12), (lab, "depth")
        if "n" in e and e.get("hit"):
            assert np.abs(ref["n"][sl] - e["n"]).max() <= 1e-12, (lab, "normal")
        if "inside" in e:
            assert np.all(ev.ref_inside[sl] == e["inside"]), (lab, "inside")
        if "prim" in e:
            sd, node, parts, M = LT.build_scene(*ev.key)
            assert np.all(ev.prim_ref[sl] == parts[e["prim"]]), (lab, "primitive")


@pytest.mark.parametrize("name,route", LT.CASES, ids=IDS)
def test_cases_agree_and_the_host_build_holds_every_one(built, name, route):
    ev = LT.evaluate(name, route)
    n = len(ev.agree)
    assert n <= 20000
    assert not np.any(ev.agree & ev.flagged)
    outside = 1.0 - ev.agree.mean()
    assert outside <= LT.MAX_OUTSIDE, (outside, {k: int(v.sum()) for k, v in ev.why.items()})
    for lab in np.unique(ev.rays.labels):
        kept = int((ev.agree & (ev.rays.labels == lab)).sum())
        assert kept >= LT.MIN_PER_LABEL, (lab, kept)
    if route == LT.OBJECTS[name].routes[0]:  # the labels speak of the object in its own frame, alone
        check_labels(ev)
    held = LT.check_backend(ev, ev.hs, ev.hs_shadow, ev.hs_inside, what="host build")
    assert held == int(ev.agree.sum()) >= 0.98 * n
    # signed zeros are in the arrays the backends get
    z = ev.rays.d == 0
    assert np.signbit(ev.rays.d[z]).any() and (~np.signbit(ev.rays.d[z])).any()
    if LT.route_traits(name, route)["tier"] == 0:  # the reference's own traversal (what a faithful launch runs) decides alike
        b = api.Builder()
        nm, _ = ev.sd.replay(b)
        hs = HostSim(b, nm[ev.sd.root])
        sel = np.flatnonzero(~ev.flagged)
        f = hs.rayint(ev.rays.o[sel], ev.rays.d[sel], ev.rays.tmax[sel], analysis=1)
        LT.check_backend(ev, f, nm=nm, what="host build, faithful", sel=sel)


def profile_text():
    lines = ["# cases outside the agreement set of tests/lattice.py, per object and route, then per label (labels with none are left out)",
             "# written by tests/test_lattice_host.py::test_profile_of_the_agreement_set; columns: cases, held, outside, flagged (diverged / over a limit), and the rays of the half-integer lattice outside"]
    for name, route in LT.CASES:
        ev = LT.evaluate(name, route)
        plain = np.char.startswith(ev.rays.labels.astype(str), "lattice:")
        lines.append("%-22s %-13s %6d %6d %5d %5d   plain lattice %4d of %5d" % (name, route, len(ev.agree), int(ev.agree.sum()), int((~ev.agree).sum()), int(ev.flagged.sum()),
                                                                          int((~ev.agree & plain).sum()), int(plain.sum())))
        labs, cnt = np.unique(ev.rays.labels[~ev.agree], return_counts=True)
        for l, c in zip(labs, cnt):
            lines.append("    %-44s %5d of %5d" % (l, c, int((ev.rays.labels == l).sum())))
    return "\n".join(lines) + "\n"


def test_profile_of_the_agreement_set(built):
    """The committed profile is what the checks compute (square roots and divisions are correctly rounded on every host, so the figures
    do not depend on the machine).  GLOME_LATTICE_WRITE=1 writes it anew instead."""
    text = profile_text()
    if os.environ.get("GLOME_LATTICE_WRITE"):
        with open(PROFILE, "w") as f:
            f.write(text)
    with open(PROFILE) as f:
        old = f.read()
    assert old == text, "profiles/lattice_agreement.txt is stale: run this test with GLOME_LATTICE_WRITE=1 and commit the file"
    total = sum(len(LT.evaluate(*c).agree) for c in LT.CASES)
    held = sum(int(LT.evaluate(*c).agree.sum()) for c in LT.CASES)
    assert held >= 0.98 * total


RUNAWAY = {  # origins ON a face of a box with a zero direction component across it: 0 * inf = NaN in the slab, and the advance never moves
    "intersection3": [((-1.0, 2.5, 1.0), (-0.0, -2.0, -2.0), 7.5),   # the ray that used to end the oracle's process
                      ((-1.0, 1.0, 0.5), (-0.0, 0.0, 0.5), 6.5), ((-1.0, -1.0, 1.5), (-0.0, 0.5, -1.0), 5.5)],
    "difference_retexture": [((1.0, -1.0, 1.0), (1.0, -0.5, -0.0), 5.0), ((0.0, 2.0, 1.5), (-0.0, -0.5, -1.0), 5.0)],
}


def test_a_diverged_ray_ends_in_a_limit_status_on_the_host_build(built):
    """Rays the bounded oracle gives up (rayint_advance nests past kAdvanceNesting: an advance that is NaN never moves the ray) run the device
    headers' own loop to kCsgRunaway = 2^20 advances and end the batch with the limit status -- not an endless loop, not an answer.  A
    handful of rays: each costs 2^20 advances per seam (some 50 ms on the host).  On the host build only: no GPU test runs such a ray."""
    from helpers import O
    t0 = time.time()
    ran = 0
    for name, rays in RUNAWAY.items():
        sd, node, parts, M = LT.build_scene(name, "alone")
        o, d, tm = (np.array([r[k] for r in rays], np.float32) for k in range(3))
        for fl in (False, True):
            orc, om, _ = O.load_scene(sd, use_float=fl)
            r = orc.rayint(om[sd.root], o.astype(np.float64), d.astype(np.float64), tm.astype(np.float64))
            assert r["diverged"].all() and np.all(r["t"] == -1), (name, fl)
            orc.shadow(om[sd.root], o.astype(np.float64), d.astype(np.float64), tm.astype(np.float64))
            assert orc.last_diverged.all(), (name, fl)
        b = api.Builder()
        nm, _ = sd.replay(b)
        hs = HostSim(b, nm[sd.root])
        assert hs.info()["tier"] == 0
        for i in range(len(rays)):
            with pytest.raises(RuntimeError, match="rc=-2"):
                hs.rayint(o[i:i + 1], d[i:i + 1], tm[i:i + 1])
            with pytest.raises(RuntimeError, match="rc=-2"):
                hs.shadow(o[i:i + 1], d[i:i + 1], tm[i:i + 1])
            ran += 1
        assert hs.rayint([[3.5, 3.5, 3.75]], [[1.0, 0.0, 0.0]], 1.0)["t"][0] == -1  # the status is the batch's: the next batch is clean
        _, _, over = LT.hostsim_answers(hs, o, d, tm)  # and the CPU stage of the lattice finds each of them in a batch
        assert over.all()
    assert ran == 5 and time.time() - t0 < 10.0
