"""The rate of the update calls by the source they read, on the flagship terrain (S3: 100,352 triangles over 225 x 225
vertices) and on a sphere bih of similar size (a 47^3 lattice: 103,823 spheres), device forms, by the library's own event pairs
(glome_ctx_timing_begin / _end), median of REPS warm updates:
  dense_f64     the existing call: nine fp64 per triangle, cx cy cz r fp64 per sphere
  dense_f32     glome_scene_bih_update_f32_dev; for the spheres glome_scene_sphere_bih_update_f32_dev's two streams
  indexed_f32   glome_scene_bih_update_indexed_dev over the terrain's own 225 x 225 fp32 vertices and its int32 face table
  torch_expand  what a torch host pays to feed the fp64 call instead: the gather + .double() (the cat + .double() for the spheres), by
                torch's events
and dense_f64 of ANOTHER build of the library (the parent commit's, given with --parent-lib: loaded through GLOME_DEBUG_LIB), so that
the existing calls can be held to what they were.  A library is fixed when a process starts, so every measurement runs in a child
process of its own, one at a time; the two libraries alternate, PAIRS pairs, and every figure is reported as min / median / max over
its PAIRS runs: the spread between repeated runs of ONE library is what a difference between the two must exceed to count.
Run from the repository root: python tools/probe/update_sources_rate.py [out.json] [--parent-lib path/to/libglome_hip.so]"""
import json
import os
import subprocess
import sys

REPS, PAIRS = 25, 5


def child():
    import ctypes as C

    sys.path.insert(0, ".")
    import numpy as np
    import torch

    from glome_amd import api, scenes

    new_calls = not os.environ.get("GLOME_DEBUG_LIB")
    ctx = api.Context(0)
    lib = ctx.lib

    def timed(fn):
        for _ in range(3):
            fn()
        ctx.synchronize()
        assert lib.glome_ctx_timing_begin(ctx.h, REPS) == 0
        for _ in range(REPS):
            fn()
        ms = (C.c_float * REPS)()
        assert lib.glome_ctx_timing_end(ctx.h, ms, REPS) == REPS
        ctx.synchronize()
        return float(np.median(np.array(list(ms))))

    def torch_timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        return float(np.median(t))

    dev = torch.device("cuda:0")
    res = {}
    # the terrain as a simulation holds it: every distinct vertex once (fp32), and the face table
    P0 = scenes.heightfield_triangles(224)
    uniq, inv = np.unique(P0.reshape(-1, 3).view(np.int64), axis=0, return_inverse=True)
    V0 = uniq.view(np.float64).reshape(-1, 3)
    idx = np.ascontiguousarray(np.asarray(inv).reshape(-1, 3).astype(np.int32))
    assert len(V0) == 225 * 225 and len(idx) == 100352
    d = np.stack([0.25 * np.sin(0.7 * V0[:, 2] + 0.3), 0.3 * np.sin(0.5 * V0[:, 0]) * np.cos(0.4 * V0[:, 2]), 0.2 * np.cos(0.6 * V0[:, 0])], 1)
    V1 = (V0 + d + np.random.default_rng(7).uniform(-0.02, 0.02, V0.shape)).astype(np.float32)
    b = api.Builder()
    ids = b.triangles_bulk(P0)
    tree = ctx.bih(b, ids)[0]
    sc = ctx.commit(b, b.tex(tree, b.material_surface((0.8, 0.5, 0.4), 1, 0.2, 1, 0, 0)))
    tv, ti = torch.tensor(V1, device=dev), torch.tensor(idx, device=dev)
    expand = lambda: tv[ti.long()].double().reshape(-1, 9)
    t64 = expand().contiguous()
    t32 = t64.float().contiguous()
    torch.cuda.synchronize()
    res["terrain"] = {"triangles": int(len(idx)), "vertices": int(len(V0)), "dense_f64_ms": timed(lambda: sc.bih_update(tree, t64))}
    if new_calls:
        res["terrain"]["dense_f32_ms"] = timed(lambda: sc.bih_update_f32(tree, t32))
        res["terrain"]["indexed_f32_ms"] = timed(lambda: sc.bih_update_indexed(tree, tv, ti))
        res["terrain"]["torch_expand_ms"] = torch_timed(expand)
    sc.release()
    # a sphere bih of similar size
    n = 23
    S0 = np.array([(float(x), float(y), float(z), 0.2) for x in range(-n, n + 1) for y in range(-n, n + 1) for z in range(-n, n + 1)])
    c = S0[:, :3]
    d = np.stack([0.25 * np.sin(0.7 * c[:, 2] + 0.3), 0.3 * np.sin(0.5 * c[:, 0]) * np.cos(0.4 * c[:, 2]), 0.2 * np.cos(0.6 * c[:, 0])], 1)
    S1 = np.concatenate([c + d, S0[:, 3:] * np.random.default_rng(13).uniform(0.5, 1.5, (len(S0), 1))], axis=1).astype(np.float32)
    b = api.Builder()
    tree = b.bih([b.sphere(tuple(s[:3]), float(s[3])) for s in S0])
    sc = ctx.commit(b, tree)
    tc, tr = torch.tensor(np.ascontiguousarray(S1[:, :3]), device=dev), torch.tensor(np.ascontiguousarray(S1[:, 3]), device=dev)
    expand = lambda: torch.cat([tc, tr[:, None]], dim=1).double()
    s64 = expand().contiguous()
    torch.cuda.synchronize()
    res["spheres"] = {"spheres": int(len(S0)), "dense_f64_ms": timed(lambda: sc.sphere_bih_update(tree, s64))}
    if new_calls:
        res["spheres"]["dense_f32_ms"] = timed(lambda: sc.sphere_bih_update_f32(tree, tc, tr))
        res["spheres"]["torch_expand_ms"] = torch_timed(expand)
    sc.release()
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def spread(values):
    v = sorted(values)
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1], "n": len(v)}


def main():
    args = sys.argv[1:]
    parent_lib = None
    if "--parent-lib" in args:
        k = args.index("--parent-lib")
        parent_lib = os.path.abspath(args[k + 1])
        del args[k:k + 2]
    runs = {"this": [], "parent": []}
    for pair in range(PAIRS):
        for which in ("this", "parent"):
            if which == "parent" and not parent_lib:
                continue
            env = {k: v for k, v in os.environ.items() if k != "GLOME_DEBUG_LIB"}
            if which == "parent":
                env["GLOME_DEBUG_LIB"] = parent_lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, stdout=subprocess.PIPE, timeout=240).stdout.decode()
            runs[which].append(json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:]))
            print(pair, which, json.dumps(runs[which][-1]), flush=True)
    res = {"reps_per_median": REPS, "pairs": PAIRS}
    for which, rs in runs.items():
        if not rs:
            continue
        res[which] = {}
        for scene in ("terrain", "spheres"):
            res[which][scene] = {k: (spread([r[scene][k] for r in rs]) if k.endswith("_ms") else rs[0][scene][k]) for k in rs[0][scene]}
    print(json.dumps(res))
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
