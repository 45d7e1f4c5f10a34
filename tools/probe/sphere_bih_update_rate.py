"""The rate of glome_scene_sphere_bih_update_dev on S1's tree (scenes.s1 at the benchmark's n: 121 spheres under Tex beside
a plane) and on the 9,261-sphere lattice of GlomeView's default scene (scenes.testscene's, as a scene of its own), beside what it
replaces, timed in the same run:
  update        median of REPS warm device-form updates, by the library's own event pairs (glome_ctx_timing_begin / _end); `spread` is
                the same measurement repeated RUNS times (min, median, max of the medians): what a difference must exceed to count
  merged        the same with every run of narrow levels in one single-block launch (GLOME_DEBUG_BIH_UPDATE_MERGED)
  split         one pair per stage (GLOME_DEBUG_BIH_UPDATE_SPLIT): sphere records, the level launches, the root box
  rebuild       glome_sb_bih over the moved spheres + glome_scene_commit (wall clock, the scene ready to render), RUNS times
  unchanged     whether a frame after an update with the committed spheres equals the frame before it
Run from the repository root: python tools/probe/sphere_bih_update_rate.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from glome_amd import api, scenes

REPS, RUNS = 25, 5


def s1_spheres(n=5):
    return np.array([(float(x), 0.5, float(z), 0.4) for x in range(-n, n + 1) for z in range(-n, n + 1)])


def lattice_spheres(n=10):
    return np.array([(float(x), float(y), float(z), 0.2) for x in range(-n, n + 1) for y in range(-n, n + 1) for z in range(-n, n + 1)])


def moved(S0):
    """a smooth displacement of the centres, radii scaled 0.5 - 1.5x per sphere"""
    c = S0[:, :3]
    d = np.stack([0.25 * np.sin(0.7 * c[:, 2] + 0.3), 0.3 * np.sin(0.5 * c[:, 0]) * np.cos(0.4 * c[:, 2]), 0.2 * np.cos(0.6 * c[:, 0])], 1)
    return np.concatenate([c + d, S0[:, 3:] * np.random.default_rng(13).uniform(0.5, 1.5, (len(S0), 1))], axis=1)


def one(ctx, name, S0, with_plane, W, H, cam):
    lib = ctx.lib
    lights = [api.light(p, c) for p, c in scenes.LIGHTS[:1]]
    RP = api.render_params(width=W, height=H, maxdepth=1)

    def commit(S):
        """(scene, bih node, wall ms of glome_sb_bih + the wrappers + glome_scene_commit); the Sphere nodes are made before the clock starts"""
        b = api.Builder()
        mats = [b.material_surface((1, 1, 1), 1, 0.2, 0.8, 0.4, 10), b.material_surface((1, 0, 0), 1, 0.2, 0.8, 0.4, 10), b.material_surface((0.5, 0, 1), 1, 0.2, 1, 0, 0)]
        items = [b.sphere(tuple(s[:3]), float(s[3])) for s in S]
        if with_plane:
            items = [b.tex(i, mats[k % 3]) for k, i in enumerate(items)]
            plane = b.tex(b.plane((0, 0, 0), (0, 1, 0)), b.material_surface((0, 0.8, 0.3), 1, 0.2, 1, 0, 0))
        t0 = time.perf_counter()
        tree = b.bih(items)
        root = b.group([plane, tree]) if with_plane else tree
        sc = ctx.commit(b, root)
        return sc, tree, (time.perf_counter() - t0) * 1e3

    def timed(fn, pairs=1):
        for _ in range(3):
            fn()
        ctx.synchronize()
        assert lib.glome_ctx_timing_begin(ctx.h, REPS * pairs) == 0
        for _ in range(REPS):
            fn()
        ms = (C.c_float * (REPS * pairs))()
        assert lib.glome_ctx_timing_end(ctx.h, ms, REPS * pairs) == REPS * pairs
        ctx.synchronize()
        return np.median(np.array(list(ms)).reshape(REPS, pairs), axis=0)

    def spread(values):
        v = sorted(values)
        return {"min": v[0], "median": v[len(v) // 2], "max": v[-1], "n": len(v)}

    res = {"scene": name, "spheres": int(len(S0)), "reps_per_median": REPS}
    S1 = moved(S0)
    commit(S0)[0].release()  # (warm: the first commit pays for the process's first allocations)
    sc, tree, _ = commit(S0)
    before, _, _ = sc.render(cam, lights, RP, want_packed=False)
    sc.sphere_bih_update(tree, S0)
    after, _, _ = sc.render(cam, lights, RP, want_packed=False)
    res["unchanged_update_keeps_the_frame"] = bool(np.array_equal(before, after, equal_nan=True))
    dv = torch.tensor(S1, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    upd = lambda: sc.sphere_bih_update(tree, dv)
    res["update_ms"] = spread(float(timed(upd)[0]) for _ in range(RUNS))
    os.environ["GLOME_DEBUG_BIH_UPDATE_MERGED"] = "1"
    res["update_merged_ms"] = spread(float(timed(upd)[0]) for _ in range(RUNS))
    del os.environ["GLOME_DEBUG_BIH_UPDATE_MERGED"]
    os.environ["GLOME_DEBUG_BIH_UPDATE_SPLIT"] = "1"
    rec, lev, bnd = (float(x) for x in timed(upd, pairs=3))
    res["split_ms"] = {"sphere_records": rec, "levels": lev, "root_box": bnd}
    del os.environ["GLOME_DEBUG_BIH_UPDATE_SPLIT"]
    sc.release()
    rebuilds = []
    for _ in range(RUNS):
        fresh, _, ms = commit(S1)
        rebuilds.append(ms)
        fresh.release()
    res["rebuild_and_commit_wall_ms"] = spread(rebuilds)
    res["rebuild_over_update"] = res["rebuild_and_commit_wall_ms"]["median"] / res["update_ms"]["median"]
    return res


def main():
    ctx = api.Context(0)
    res = [one(ctx, "S1 tree (scenes.s1, n = 5)", s1_spheres(5), True, 720, 480, api.camera(*scenes.CUST_CAM)),
           one(ctx, "lattice (21^3, scenes.testscene's)", lattice_spheres(10), False, 720, 480, api.camera((-14.0, 18.0, 40.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0))]
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
