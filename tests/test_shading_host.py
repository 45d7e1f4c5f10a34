"""CPU suite: shading cases (tests/shading_cases.py) through the host build of `trace` (tests/hostsim hostsim_trace), case by case.

  - every route is what it claims to be: the tier and the trace instance of every launch come from the commit's own traits
    (glome_sb_scene_traits, glome_trace_kernel_choice) and must be the instance the family's materials ask for -- lean, full, faithful;
  - every label reaches its branch: where a family states the shadow and secondary rays a ray spawns, the fp64 oracle spawns them;
  - the agreement set cannot hide a failure: per family and route at most 2 % of the cases lie outside it, every label keeps at least 32
    cases inside it, and the labels about an exact equality keep ALL theirs;
  - inside the set the host build answers every case as the oracle does -- the full tier, the lean tier wherever the product would launch
    a lean kernel (and hostsim_trace refuses it elsewhere, by the product's own predicate), and the reference's own traversal;
  - the batches are mixed in state: the interleaved order is no copy of the sorted one, a wave holds hits beside misses and lanes whose
    counts differ, and the light family's labels answer as their names say under the one light list they share;
  - lean and full answers are bit-identical wherever both are legal, and a batch's answers do not depend on the order of its rays.

The counts are in profiles/shading_agreement.txt, which a test holds to what is computed."""
import ctypes as C
import os

import numpy as np
import pytest

import shading_cases as SC
import test_trace_choice as trace_choice
from helpers import HostSim
from glome_amd import _lib as L
from glome_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "shading_agreement.txt")
IDS = ["%s-%s" % c for c in SC.CASES]


def host_scene(case):
    sd = SC.build(*case).sd
    b = api.Builder()
    nm, _ = sd.replay(b)
    return b, nm, HostSim(b, nm[sd.root])


def test_the_table_holds_the_families_and_routes_it_should():
    assert set(SC.FAMILIES) == {"light", "surface", "texfold", "reflect", "refract", "blend", "tx", "warp"}
    assert {r for _, r in SC.CASES} == {"prims", "prims_full", "bih_tri", "mesh", "generic"}
    assert all("generic" in SC.ROUTES[f] for f in SC.FAMILIES) and SC.ROUTES["warp"] == ("generic",)
    assert len(set(SC.CASES)) == len(SC.CASES)


@pytest.mark.parametrize("family,route", SC.CASES, ids=IDS)
def test_route_is_what_it_claims(built, family, route):
    b, nm, hs = host_scene((family, route))
    sd = SC.build(family, route).sd
    assert hs.info()["tier"] == (1 if route == "generic" else 0)
    lib = L.load()
    t = np.zeros(11, dtype=np.int64)
    assert lib.glome_sb_scene_traits(b.h, nm[sd.root], t.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    depths = sorted({bt.maxdepth for bt in SC.build(family, route).batches})
    for md in depths:
        for faithful, count in ((0, 0), (1, 0), (0, 1)):  # the trace launch, the faithful one, the work launch of the GPU suite
            inst, _, _ = trace_choice.export_choice(lib, [list(t[:8]) + [faithful, count, md]])[0].tolist()
            assert trace_choice.instance_name(inst) == SC.instance_name(family, route, md, bool(faithful), bool(count)), (md, faithful, count)
    if route == "prims":  # the lean instance is reached where it should be: by the families without secondary materials, and at maxdepth 1
        lean = {md for md in depths if SC.lean_legal(family, route, md)}
        assert lean == {"light": {3}, "surface": {3}, "texfold": set(), "reflect": {1}, "refract": {1}, "blend": set(), "tx": set()}[family]


@pytest.mark.parametrize("family,route", SC.CASES, ids=IDS)
def test_labels_reach_their_branches(built, family, route):
    ev = SC.evaluate(family, route)
    stated = 0
    for k, bt in enumerate(ev.scene.batches):
        ref = ev.ref[ev.batch_of == k]
        for lab, e in bt.expect.items():
            m = bt.labels == lab
            assert m.any()
            if e.get("hit") is not None:
                assert np.all((ref[m, 4] < SC.MISS_DEPTH) == e["hit"]), (lab, "hit")
            for key, col in (("shadow", 5), ("secondary", 6)):
                if e.get(key) is not None:
                    assert np.all(ref[m, col] == e[key]), (lab, key, e[key], np.unique(ref[m, col]).tolist())
                    stated += 1
    assert stated > 0 or family in ("refract", "blend", "tx")
    assert len(np.unique(np.hstack([np.vstack([b.o for b in ev.scene.batches]), np.vstack([b.d for b in ev.scene.batches]), ev.batch_of[:, None].astype(np.float32)]), axis=0)) == len(ev.agree)


def host_answers(case, hs, full, faithful=0, order=None):
    """the host build on every batch (NaN rows where a lean tier is not legal: hostsim_trace must refuse it there)"""
    out = []
    for bt in SC.build(*case).batches:
        if not full and not SC.lean_legal(case[0], case[1], bt.maxdepth):
            with pytest.raises(RuntimeError, match="rc=-3"):
                SC.hostsim_trace(hs, bt, 0, faithful)
            out.append(np.full((len(bt.o), 7), np.nan)); continue
        if order is None:
            out.append(SC.hostsim_trace(hs, bt, full, faithful))
        else:
            p = order(bt.labels)
            got = np.zeros((len(p), 7)); got[p] = SC.hostsim_trace(hs, bt._replace(o=bt.o[p], d=bt.d[p], labels=bt.labels[p]), full, faithful)
            out.append(got)
    return np.vstack(out)


def bits(a):
    return np.ascontiguousarray(a[:, :5], np.float32).view(np.uint32)


@pytest.mark.parametrize("family,route", SC.CASES, ids=IDS)
def test_cases_agree_and_the_host_build_holds_every_one(built, family, route):
    ev = SC.evaluate(family, route)
    n = len(ev.agree)
    assert 200 <= n <= 6000
    outside = 1.0 - ev.agree.mean()
    assert outside <= SC.MAX_OUTSIDE, (outside, {k: int(v.sum()) for k, v in ev.why.items()})
    for lab in np.unique(ev.labels):
        m = ev.labels == lab
        kept = int((ev.agree & m).sum())
        assert kept >= SC.MIN_PER_LABEL, (lab, kept)
        if lab.startswith(SC.EQUALITY):
            assert kept == int(m.sum()), (lab, "an equality label keeps all its cases", kept, int(m.sum()))
    assert any(l.startswith(SC.EQUALITY) for l in np.unique(ev.labels)) or family in ("refract", "blend")
    _, _, hs = host_scene((family, route))
    full = host_answers((family, route), hs, 1)
    held, _ = SC.check_backend(ev, full, "host build, full")
    assert held == int(ev.agree.sum())
    faithful = host_answers((family, route), hs, 1, faithful=1)
    SC.check_backend(ev, faithful, "host build, faithful")
    lean = host_answers((family, route), hs, 0)
    legal = np.flatnonzero(~np.isnan(lean[:, 5]))
    if len(legal):
        SC.check_backend(ev, lean[legal], "host build, lean", legal)
        assert np.array_equal(bits(lean[legal]), bits(full[legal])) and np.array_equal(lean[legal, 5:], full[legal, 5:]), "lean and full differ"
    assert (len(legal) > 0) == any(SC.lean_legal(family, route, bt.maxdepth) for bt in ev.scene.batches)
    perms = SC.check_mixing(ev)
    assert all(np.array_equal(p, SC.interleave(bt.labels)) for p, bt in zip(perms, ev.scene.batches))
    mixed = host_answers((family, route), hs, 1, order=SC.interleave)
    assert np.array_equal(bits(mixed), bits(full)) and np.array_equal(mixed[:, 5:], full[:, 5:]), "a ray's answer depends on its place in the batch"


def test_hostsim_trace_refuses_what_the_product_refuses(built):
    _, _, hs = host_scene(("light", "prims"))
    bt = SC.build("light", "prims").batches[0]
    for md in (0, 9):
        with pytest.raises(RuntimeError, match="rc=-5"):
            SC.hostsim_trace(hs, bt._replace(maxdepth=md))
    with pytest.raises(RuntimeError, match="rc=-4"):  # a direction that is not unit length, without `faithful`
        SC.hostsim_trace(hs, bt._replace(d=bt.d * np.float32(2)))
    SC.hostsim_trace(hs, bt._replace(d=bt.d * np.float32(2)), faithful=1)
    _, _, hg = host_scene(("light", "generic"))
    with pytest.raises(RuntimeError, match="rc=-3"):  # the generic tier has no lean kernel
        SC.hostsim_trace(hg, SC.build("light", "generic").batches[0], full=0)
    with pytest.raises(RuntimeError, match="rc=-1"):  # nor does a generic scene run on the flat tier
        SC.hostsim_trace(hg, SC.build("light", "generic").batches[0], tier=0)


def test_the_light_batches_mix_states_and_not_names_alone(built):
    """one light list over tiles in different states: what the oracle answers differs between the labels of one batch as the labels say"""
    for route in SC.ROUTES["light"]:
        ev = SC.evaluate("light", route)
        red = lambda lab: ev.ref[ev.labels == lab, 0]
        count = lambda lab: set(ev.ref[ev.labels == lab, 5].tolist())
        shadows = route != "mesh"  # (a Mesh casts no shadow)
        assert (red("light/occluded").max() < red("light/lit").min()) == shadows
        assert (red("light/16-alternating:occluded").max() < red("light/16-alternating").min()) == shadows
        assert (red("light/outside-margin:slanted").max() < red("light/inside-margin:slanted").min()) == shadows
        assert (red("light/outside-margin").max() < red("light/inside-margin").min()) == (route in ("prims", "prims_full", "generic"))  # (Q1)
        assert count("light/behind-higher-floor") == {1.0} and count("light/in-plane-of-raised-floor") == {2.0}
        for what in ("==", "-ulp", "+ulp"):
            assert count("light/rad%s:nearer" % what) == {1.0} and count("light/rad%s:farther" % what) == {0.0}
        assert count("light/llen==0") == count("light/llen==0:same-tile") == count("light/llen==0:lowered-floor") == {2.0}
        assert red("light/shadowless-behind-occluder").min() > red("light/none:below-ceiling").max()
        if route in ("prims", "prims_full", "generic"):
            assert red("light/onlyshadow-occluder").max() < red("light/noshadow-occluder").min()
        # all of them in ONE batch each, so in one wave once dealt out
        for group in (("light/lit", "light/occluded", "light/behind-higher-floor", "light/miss"), ("light/rad==", "light/rad==:nearer", "light/rad==:farther"),
                      ("light/16-first", "light/16-sixteenth", "light/16-alternating", "light/16-alternating:occluded"),
                      ("light/inside-margin", "light/outside-margin", "light/inside-margin:slanted", "light/outside-margin:slanted"), ("light/tangent-in", "light/tangent-in:raised-floor")):
            assert any(set(group) <= set(bt.labels.tolist()) for bt in ev.scene.batches), group


def test_interleave_is_a_permutation_that_mixes_labels():
    labels = np.array(["a"] * 5 + ["b"] * 3 + ["c"] * 4)
    p = SC.interleave(labels)
    assert sorted(p.tolist()) == list(range(12))
    assert labels[p][:6].tolist() == ["a", "b", "c", "a", "b", "c"]


def cpu_lines():
    lines = []
    for case in SC.CASES:
        ev = SC.evaluate(*case)
        lines.append("%-8s %-10s %5d %5d   outside: decision %3d colour %3d depth %3d   float oracle worst %.3e" % (
            case.family, case.route, len(ev.agree), int(ev.agree.sum()), int(ev.why["decision"].sum()), int(ev.why["colour"].sum()), int(ev.why["depth"].sum()),
            SC.colour_err(ev.f32_, ev.ref)[ev.agree].max()))
        for lab in np.unique(ev.labels):
            m = ev.labels == lab
            lines.append("    %-52s %4d of %4d" % (lab, int((ev.agree & m).sum()), int(m.sum())))
    return lines


HEADER = ["# the agreement set of tests/shading_cases.py per family and route: cases, cases inside, cases outside by reason, the float oracle's worst colour",
          "# deviation inside the set (|x - ref| / max(1, |ref|)); then per label the cases inside.  Written by tests/test_shading_host.py::test_profile_of_the_agreement_set",
          "# (GLOME_SHADING_WRITE=1).  The lines that start with `gpu` are the MI355X's worst deviation inside the set, from tests/test_shading_gpu.py; the CPU test keeps them."]


def test_profile_of_the_agreement_set(built):
    """The committed profile is what the checks compute.  GLOME_SHADING_WRITE=1 writes the CPU lines anew and keeps the GPU's."""
    lines = cpu_lines()
    old = open(PROFILE).read().splitlines() if os.path.exists(PROFILE) else []
    gpu = [l for l in old if l.startswith("gpu")]
    if os.environ.get("GLOME_SHADING_WRITE"):
        with open(PROFILE, "w") as f:
            f.write("\n".join(HEADER + lines + gpu) + "\n")
        old = open(PROFILE).read().splitlines()
    assert [l for l in old if not l.startswith(("#", "gpu"))] == lines, "profiles/shading_agreement.txt is stale: run this test with GLOME_SHADING_WRITE=1 and commit the file"
    assert {tuple(l.split()[1:3]) for l in gpu} == {tuple(c) for c in SC.CASES}, "a GPU line per family and route"
