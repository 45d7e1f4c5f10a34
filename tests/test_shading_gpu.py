"""GPU suite (-m gpu): shading cases (tests/shading_cases.py) through the C ABI, case by case.

For every family on every route that can hold it one scene is committed, and every batch -- a light list, a maxdepth, its rays -- goes through
glome_trace_batch (the class instance the scene gets: lean or full, or the faithful one under a Refract), through glome_trace_work_batch
(the counting instance, whose words 3 and 4 are the shadow and secondary rays each ray spawned) and through glome_trace_batch with
faithful = 1.  On the agreement set of the two oracles (shading_cases.evaluate) the device answers EVERY case as the fp64 oracle does:
hit / miss and both per-ray counts exactly, every colour channel and alpha within 1e-4 of max(1, |ref|), the depth within parity.T_RTOL,
NaN where the oracle's is NaN.  There is no outlier allowance.

Cross-checks, bit for bit: the production trace and the faithful one (every direction here is unit length); a batch sorted by label, so
that waves are uniform, and dealt out label by label, so that the 64 lanes of a wave sit in different states of shade_vm -- miss, lit,
occluded, a light behind or out of reach, other masks of sixteen lights, other depths of the ladder (shading_cases.check_mixing asserts
that the waves are mixed in what the oracle answers, not in name alone, and that the order is no copy of the sorted one); and the lean
instance against the full one -- the library has no switch for that, so the twin is the same scene with an unreachable Reflect and an
unreachable Blend in its material table (route prims_full).

GLOME_SHADING_GPU_PROFILE=<file> appends the worst deviation inside the set per family and route (the `gpu` lines of
profiles/shading_agreement.txt)."""
import os

import numpy as np
import pytest

import shading_cases as SC
from glome_amd import api

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(sc, bt, perm=None, faithful=0):
    """(n x 5 float32 of the trace launch, n x 5 of the work launch, n x 2 counts), rows in the batch's own order"""
    o, d = (bt.o, bt.d) if perm is None else (bt.o[perm], bt.d[perm])
    lights = SC.lights_of(bt)
    P = api.trace_params(maxdepth=bt.maxdepth, faithful=faithful)
    r = sc.trace(o, d, lights, params=P)
    w = sc.trace_work(o, d, lights, params=P)
    assert r["stats"]["rays_primary"] == len(o) and int(w["work"][:, 3].sum()) == w["stats"]["rays_shadow"] and int(w["work"][:, 4].sum()) == w["stats"]["rays_secondary"]
    assert r["stats"]["rays_shadow"] == w["stats"]["rays_shadow"] and r["stats"]["rays_secondary"] == w["stats"]["rays_secondary"]
    out = [np.hstack([r["rgba"], r["depth"][:, None]]), np.hstack([w["rgba"], w["depth"][:, None]]), w["work"][:, 3:5].astype(np.float64)]
    if perm is not None:
        inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
        out = [a[inv] for a in out]
    return out


def run_case(ctx, family, route):
    """commit, launch every batch, check, release: returns (the evaluation, the trace launch's rows, the worst colour deviation inside the set)"""
    ev = SC.evaluate(family, route)
    sd = ev.scene.sd
    b = api.Builder()
    nm, _ = sd.replay(b)
    sc = ctx.commit(b, nm[sd.root])
    # (the library names no instance from a launch: that these launches get the lean, full and faithful instances the families ask for is
    # held on the host, from the commit's own traits, by test_shading_host.py::test_route_is_what_it_claims; here the tier alone)
    rows, worst = [], 0.0
    perms = SC.check_mixing(ev)  # (every batch: more than a wave, not the identity, hits beside misses, counts that differ in a wave)
    try:
        assert sc.info()["tier"] == (1 if route == "generic" else 0)
        for k, bt in enumerate(ev.scene.batches):
            sel = np.flatnonzero(ev.batch_of == k)
            what = "batch %d (maxdepth %d, %d lights)" % (k, bt.maxdepth, len(bt.lights))
            tr, wk, cnt = launch(sc, bt)
            for name, five in (("trace", tr), ("work", wk)):
                held, e = SC.check_backend(ev, np.hstack([five.astype(np.float64), cnt]), "%s, %s" % (name, what), sel)
                print("shading_gpu", family, route, k, name, held, "%.3e" % e)
                worst = max(worst, e)
            assert held == int(ev.agree[sel].sum())
            ftr, fwk, fcnt = launch(sc, bt, faithful=1)
            SC.check_backend(ev, np.hstack([ftr.astype(np.float64), fcnt]), "faithful trace, " + what, sel)
            a = ev.agree[sel]
            assert np.array_equal(bits(ftr[a]), bits(tr[a])) and np.array_equal(fcnt[a], cnt[a]), "%s/%s %s: the production trace and the faithful one differ" % (family, route, what)
            mtr, mwk, mcnt = launch(sc, bt, perm=perms[k])
            assert np.array_equal(bits(mtr), bits(tr)) and np.array_equal(bits(mwk), bits(wk)) and np.array_equal(mcnt, cnt), "%s/%s %s: the two batch orders differ" % (family, route, what)
            rows.append(np.hstack([tr.astype(np.float64), cnt]))
    finally:
        sc.release()
    return ev, np.vstack(rows), worst


@pytest.fixture(scope="module")
def done():
    return {}


@pytest.mark.parametrize("family,route", SC.CASES, ids=["%s-%s" % c for c in SC.CASES])
def test_every_case_of_the_agreement_set(gpu_ctx, done, family, route):
    ev, rows, worst = run_case(gpu_ctx, family, route)
    assert 200 <= len(rows) <= 6000
    done[(family, route)] = rows
    path = os.environ.get("GLOME_SHADING_GPU_PROFILE")
    if path:
        with open(path, "a") as f:
            f.write("gpu %-8s %-10s %5d held   MI355X worst %.3e\n" % (family, route, int(ev.agree.sum()), worst))


@pytest.mark.parametrize("family", [f for f in SC.FAMILIES if "prims_full" in SC.ROUTES[f]])
def test_lean_and_full_instances_agree_bit_for_bit(gpu_ctx, done, family):
    """the same rays, lights and maxdepth on the scene that gets a lean instance and on its twin that gets the full one"""
    lean = done[(family, "prims")] if (family, "prims") in done else run_case(gpu_ctx, family, "prims")[1]
    full = done[(family, "prims_full")] if (family, "prims_full") in done else run_case(gpu_ctx, family, "prims_full")[1]
    ev = SC.evaluate(family, "prims")
    legal = np.array([SC.lean_legal(family, "prims", ev.scene.batches[k].maxdepth) for k in ev.batch_of])
    assert np.array_equal(ev.ref, SC.evaluate(family, "prims_full").ref)  # (one scene to the oracle)
    assert legal.sum() >= SC.MIN_PER_LABEL or family == "texfold"  # (texfold holds a Reflect at maxdepth 3: full on both scenes)
    assert np.array_equal(bits(lean[legal, :5]), bits(full[legal, :5])) and np.array_equal(lean[legal, 5:], full[legal, 5:])
    assert np.array_equal(bits(lean[:, :5]), bits(full[:, :5]))  # (and where both are full: one kernel, one answer)
