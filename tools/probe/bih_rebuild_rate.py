"""The cost of glome_scene_bih_rebuild_dev on S3 (100,352 triangles, 1920 x 1080) and S5 (1,002,528 triangles, 3840 x 2160),
the `tex (bih (map triangle ...))` terrains under the V1 pose of bih_update_rate.py, beside the road it replaces, in ONE run.  Every
timing is host wall clock, the median of REPS with min and max:
  rebuild       glome_scene_bih_rebuild_dev of a device array, the call's whole duration (it returns with the scene complete), and its
                stages by the library's own marks (glome_scene_bih_rebuild_stages): boxes, levels (with the readback), tables (the
                layout on the host), upload, values (the update's kernels and the last wait)
  replaced      the road it replaces: glome_sb_bih_dev of the same triangles plus glome_scene_commit (the triangles already in a builder)
  commit_alone  glome_scene_commit by itself, which since this feature also keeps the per-item record table
  frame         the lone frame after the rebuild against a fresh commit's of the same pose (the layout is the same: a difference beyond the
                spread would be a finding), by the library's event pairs
Run from the repository root: python tools/probe/bih_rebuild_rate.py [out.json]"""
import ctypes as C
import json
import sys
import time

sys.path.insert(0, ".")
import torch

from glome_amd import api, scenes

sys.path.insert(0, "tools/probe")
from bih_update_rate import camera, deform  # noqa: E402

REPS, FRAME_REPS = 5, 25


def stats(v):
    v = sorted(float(x) for x in v)
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}


def one(ctx, name, N, W, H):
    lib = ctx.lib
    P0 = scenes.heightfield_triangles(N)
    P1 = deform(P0, "V1")
    lights = [api.light(p, c) for p, c in scenes.LIGHTS[:1]]
    RP = api.render_params(width=W, height=H, maxdepth=1)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
    cam = camera("V1")

    def commit(P):
        b = api.Builder()
        mat = b.material_surface((0.8, 0.5, 0.4), 1, 0.2, 1, 0, 0)
        ids = b.triangles_bulk(P)
        t0 = time.perf_counter()
        tree = ctx.bih(b, ids)[0]
        root = b.tex(tree, mat)
        t1 = time.perf_counter()
        sc = ctx.commit(b, root)
        t2 = time.perf_counter()
        return sc, tree, (t2 - t0) * 1e3, (t2 - t1) * 1e3

    def frame_ms(sc):
        fn = lambda: sc.render_dev(cam, lights, RP, None, out.data_ptr(), want_stats=False)
        for _ in range(3):
            fn()
        ctx.synchronize()
        assert lib.glome_ctx_timing_begin(ctx.h, FRAME_REPS) == 0
        for _ in range(FRAME_REPS):
            fn()
        ms = (C.c_float * FRAME_REPS)()
        assert lib.glome_ctx_timing_end(ctx.h, ms, FRAME_REPS) == FRAME_REPS
        ctx.synchronize()
        return stats(list(ms))

    res = {"scene": name, "triangles": int(len(P0)), "frame": [W, H]}
    commit(P0)[0].release()  # (warm: the first build pays for the process's first allocations)
    replaced, commits = [], []
    fresh = None
    for _ in range(REPS):
        if fresh is not None:
            fresh.release()
        fresh, _, road, alone = commit(P1)
        replaced.append(road)
        commits.append(alone)
    res["replaced_bih_dev_commit_ms"] = stats(replaced)
    res["commit_alone_ms"] = stats(commits)
    sc, tree, _, _ = commit(P0)
    d = {w: torch.tensor(P, dtype=torch.float64, device="cuda:0") for w, P in (("V0", P0), ("V1", P1))}
    torch.cuda.synchronize()
    sc.bih_rebuild(tree, d["V1"])  # (warm)
    whole, stages = [], []
    for _ in range(REPS):
        sc.bih_rebuild(tree, d["V0"])
        ctx.synchronize()
        t0 = time.perf_counter()
        sc.bih_rebuild(tree, d["V1"])
        whole.append((time.perf_counter() - t0) * 1e3)
        stages.append(sc.bih_rebuild_stages())
    res["rebuild_ms"] = stats(whole)
    res["rebuild_stages_ms"] = {k: stats([s[k] for s in stages]) for k in stages[0]}
    res["layout"] = sc.bih_layout(tree)
    res["frame_after_rebuild_ms"] = frame_ms(sc)
    res["frame_fresh_commit_ms"] = frame_ms(fresh)
    res["replaced_over_rebuild"] = res["replaced_bih_dev_commit_ms"]["median"] / res["rebuild_ms"]["median"]
    sc.release()
    fresh.release()
    return res


def main():
    ctx = api.Context(0)
    res = [one(ctx, "S3", 224, 1920, 1080), one(ctx, "S5", 708, 3840, 2160)]
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
