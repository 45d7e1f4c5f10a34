"""Writes tests/golden/packet_walk_record.json: what the models of the hand-written packet walk say of every scene and stream of
tests/test_packet_walk_model_host.py (TEST INFRASTRUCTURE, no GPU).

The committed record was made on the commit that still had three models of the walk -- tests/packet_model.py (walk_stream),
tests/far_only_model.py (stream_steps) and tests/dispatch_model.py (stream_events) -- with

    python tests/golden/make_packet_walk_record.py --modules packet_model,far_only_model,dispatch_model

and tests/packet_walk_model.py, which replaced them, gives the same file with no arguments.  The host test regenerates it in memory.

What is walked: the six ladders of tests/ladder.py (ladder_streams), the heightfield (Field) and the lattice (Lattice).  Per scene and stream,
the primary packets in mode 1; the shadow packets shadow_stream makes of them (from the production walk's hits) in mode 2; and for a ladder's
"screen" stream the shadow rays of ladder.shadow_rays as well.  Each with the origin clip and without it, but for the "nan" stream, whose
direction component of 0 the reference interval does not take: with the clip only, and no shadow packets.  walk_stream has the reference
interval alone on that commit, so its view is recorded without the clip only.

Per key "scene | stream | mode | clip": the number of packets, a sha256 of the rays' bytes, readable totals (steps by kind, dispatches by
site, pops by outcome, pushes and pops beyond the LDS part, the deepest stack) and a sha256 of each view over a canonical form: plain ints,
strings and lists, Counters as sorted item lists, per-lane arrays as lists, floats by float.hex."""
import argparse
import collections
import hashlib
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "packet_walk_record.json")
for _p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)


class Scene:
    """a scene of the tests: its tree, its primary streams and who holds its geometry"""

    def __init__(self, name, holder, bih, streams, with_uids):
        self.name, self.holder, self.bih, self.streams = name, with_uids(holder, bih), bih, streams


def all_scenes():
    """the six ladders, the field and the lattice.  (On the commit the record was made on they come from the models' own modules.)"""
    import ladder
    from oracle import np_scene as NS
    if importlib.util.find_spec("packet_walk_scenes"):
        import packet_walk_scenes as F
        from packet_walk_model import device_bounds
        D = F
    else:
        import dispatch_model as D
        import far_only_model as F
        device_bounds = F.device_bounds
    out = []
    for v in ladder.CONFIGS:
        lad = ladder.Ladder(*v)
        sc, nm = NS.load(lad.sd)
        bih = sc.nodes[nm[lad.bih_id]]
        out.append(Scene("ladder %s%s" % ("xyz"[v[0]], "+-"[v[1] < 0]), lad, bih, F.ladder_streams(lad, device_bounds(bih.bb)[1][2]), D.with_uids))
    f = F.Field()
    sc, nm = NS.load(f.sd)
    out.append(Scene("field", f, sc.nodes[nm[f.bih_id]], f.streams(), D.with_uids))
    lat = D.Lattice()
    out.append(Scene("lattice", lat, lat.bih, lat.streams(), D.with_uids))
    for s in out:
        s.shadow_stream = D.shadow_stream
    return out


def module_views(names):
    """views(scene, stream, mode, clip, chunks) from the three stream functions of the named modules.  chunks: [(o, d, limit)], each cut
    into packets of 64 on its own.  Returns the packets' (walk_stream, stream_steps, stream_events) results; the first is None with the clip."""
    pm, fm, dm = (importlib.import_module(n) for n in names)

    def views(scene, stream, mode, clip, chunks):
        packets = None if clip else [r for o, d, lim in chunks for r in pm.walk_stream(scene.bih, o, d, lim, mode)]
        return (packets, [r for o, d, lim in chunks for r in fm.stream_steps(scene.bih, o, d, lim, mode, origin_clip=clip)],
                [r for o, d, lim in chunks for r in dm.stream_events(scene.bih, o, d, lim, mode, origin_clip=clip)])
    return views


def walk_all(scenes, views):
    """yields (scene, stream, mode, clip, chunks, the three views) for everything the record holds"""
    import ladder
    for s in scenes:
        for name, (o, d) in s.streams.items():
            todo = [(name, 1, [(o, d, 1e6)])]
            first = views(s, name, 1, True, todo[0][2])
            if name != "nan":
                todo.append((name + "'s shadow rays", 2, s.shadow_stream(s.holder, o, d, first[2])))
                if name == "screen":  # a ladder's: the primary rays all end on the screen
                    t = np.concatenate([r["t"] for r in first[1]])
                    assert np.all(t > 0)
                    todo.append(("screen's shadow rays by ladder.shadow_rays", 2, [ladder.shadow_rays(s.holder, o, d, t)]))
            for stream, mode, chunks in todo:
                for clip in (True,) if name == "nan" else (True, False):
                    yield s, stream, mode, clip, chunks, first if (stream, clip) == (name, True) else views(s, stream, mode, clip, chunks)


def canon(x):
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    if x is None or isinstance(x, str):
        return x
    if isinstance(x, np.ndarray):
        return [canon(v) for v in x.tolist()]
    if isinstance(x, collections.Counter):
        return [[canon(k), canon(v)] for k, v in sorted(x.items())]
    if isinstance(x, (set, frozenset)):
        return sorted(canon(v) for v in x)
    if isinstance(x, dict):
        return {k: canon(x[k]) for k in sorted(x)}
    if isinstance(x, tuple) and hasattr(x, "_fields"):
        return [type(x).__name__] + [canon(v) for v in x]
    assert isinstance(x, (list, tuple)), type(x)
    return [canon(v) for v in x]


def digest(x):
    return hashlib.sha256(json.dumps(canon(x), separators=(",", ":")).encode()).hexdigest()


def _count(items):
    return {str(k): v for k, v in sorted(collections.Counter(items).items(), key=str)}


def record(scenes, views):
    rec = {}
    for s, stream, mode, clip, chunks, (packets, steps, events) in walk_all(scenes, views):
        rays = hashlib.sha256()
        for o, d, lim in chunks:
            for a in (o, d):
                rays.update(np.ascontiguousarray(a).tobytes())
        ev = [e for r in events for e in r["events"]]
        totals = {"steps": _count(x.kind for r in steps for x in r["steps"]),
                  "dispatches": _count(e.site for e in ev if type(e).__name__ == "Dispatch"),
                  "pops": _count(e.outcome for e in ev if type(e).__name__ == "Pop"),
                  "pushes_over": sum(r["pushes_over"] for r in steps), "pops_over": sum(r["pops_over"] for r in steps),
                  "max_depth": max((r["max_depth"] for r in steps), default=0)}
        rec["%s | %s | mode %d | %s" % (s.name, stream, mode, "clip" if clip else "no clip")] = {
            "packets": len(steps), "rays": rays.hexdigest(), "totals": totals,
            "walk_stream": None if packets is None else digest(packets), "stream_steps": digest(steps), "stream_events": digest(events)}
    return rec


def dumps(rec):
    """one line per key"""
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(canon(v))) for k, v in rec.items()) + "\n}\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--modules", default="packet_walk_model,packet_walk_model,packet_walk_model", help="where walk_stream, stream_steps and stream_events are")
    ap.add_argument("--out", default=RECORD)
    a = ap.parse_args()
    with open(a.out, "w") as f:
        f.write(dumps(record(all_scenes(), module_views(a.modules.split(",")))))
