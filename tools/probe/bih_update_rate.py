"""The rate of glome_scene_bih_update_dev on S3 (100,352 triangles, 1920 x 1080) and S5 (1,002,528 triangles, 3840 x 2160),
the `tex (bih (map triangle ...))` terrains, beside what it replaces, timed in the same run:
  update        median of REPS warm device-form updates, by the library's own event pairs (glome_ctx_timing_begin / _end); `spread` is
                the same measurement repeated RUNS times (min, median, max of the medians): what a difference must exceed to count
  merged        the same with every run of narrow levels in one single-block launch (GLOME_DEBUG_BIH_UPDATE_MERGED; the default is a
                launch per level until this comparison says otherwise), repeated as often
  split         one pair per stage (GLOME_DEBUG_BIH_UPDATE_SPLIT): triangle records, the level launches, the root box -- in both forms
  launches      level launches with and without the merged form (from the tree's level widths, glome_sb_bih_dump)
  bih_dev       glome_sb_bih_dev + glome_scene_commit of the same triangles (wall clock, the scene ready to render)
  bih_host      glome_sb_bih + glome_scene_commit
  commit_alone  glome_scene_commit by itself (wall clock), which since this feature also makes the update's tables
  frame         the lone frame the update feeds
  stale         the frame time of the refitted scene against a scene built fresh from the same triangles, for V1 (a smooth displacement
                plus jitter) and V2 (scaled by 3 and translated; the camera follows)
Run from the repository root: python tools/probe/bih_update_rate.py [out.json]"""
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
MERGE_BLOCK = 1024  # bih_update_kernels.hpp kMergeBlock
SHIFT = np.array([40.0, 6.0, -30.0])


def deform(P0, which):
    V0 = P0.reshape(-1, 3)
    if which == "V1":
        d = np.stack([0.25 * np.sin(0.7 * V0[:, 2] + 0.3), 0.3 * np.sin(0.5 * V0[:, 0]) * np.cos(0.4 * V0[:, 2]), 0.2 * np.cos(0.6 * V0[:, 0])], 1)
        return (V0 + d + np.random.default_rng(7).uniform(-0.02, 0.02, V0.shape)).reshape(-1, 9)
    return (V0 * 3.0 + SHIFT).reshape(-1, 9)


def camera(which):
    pos, at, up, angle = scenes.CUST_CAM
    if which == "V2":
        pos, at = tuple(np.array(pos) * 3.0 + SHIFT), tuple(np.array(at) * 3.0 + SHIFT)
    return api.camera(pos, at, up, angle)


def level_widths(builder, node):
    """branch nodes per tree level, from the preorder dump"""
    _, _, axis, _, _ = builder.bih_dump(node)
    widths, stack = {}, []
    for ax in axis:
        while stack and stack[-1][1] == 0:
            stack.pop()
        depth = 0
        if stack:
            depth = stack[-1][0] + 1
            stack[-1][1] -= 1
        if ax >= 0:
            widths[depth] = widths.get(depth, 0) + 1
            stack.append([depth, 2])
    return [widths[d] for d in sorted(widths)]


def merged_launches(widths):
    """launches of the levels, deepest first, when every run of two or more levels of at most MERGE_BLOCK nodes is one launch"""
    n, run = 0, 0
    for w in reversed(widths):
        if w <= MERGE_BLOCK:
            run += 1
        else:
            n += (1 if run else 0) + 1
            run = 0
    return n + (1 if run else 0)


def one(ctx, name, N, W, H):
    lib = ctx.lib
    P0 = scenes.heightfield_triangles(N)
    lights = [api.light(p, c) for p, c in scenes.LIGHTS[:1]]
    RP = api.render_params(width=W, height=H, maxdepth=1)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")

    def commit(P, on_device):
        b = api.Builder()
        mat = b.material_surface((0.8, 0.5, 0.4), 1, 0.2, 1, 0, 0)
        ids = b.triangles_bulk(P)
        t0 = time.perf_counter()
        tree = ctx.bih(b, ids)[0] if on_device else b.bih(ids)
        root = b.tex(tree, mat)
        t1 = time.perf_counter()
        sc = ctx.commit(b, root)
        commit_only.append((time.perf_counter() - t1) * 1e3)
        return sc, tree, (time.perf_counter() - t0) * 1e3, b

    commit_only = []  # glome_scene_commit alone, of every scene made here (it now also makes the update's tables)

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

    def frame_ms(sc, which):
        cam = camera(which)
        return float(timed(lambda: sc.render_dev(cam, lights, RP, None, out.data_ptr(), want_stats=False))[0])

    def spread(fn):
        v = sorted(float(timed(fn)[0]) for _ in range(RUNS))
        return {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}

    res = {"scene": name, "triangles": int(len(P0)), "frame": [W, H]}
    commit(P0, True)[0].release()  # (warm: the first build pays for the process's first allocations)
    sc, tree, res["bih_dev_commit_ms"], b = commit(P0, True)
    res["bih_host_commit_ms"] = commit(P0, False)[2]
    widths = level_widths(b, tree)
    res["levels"] = len(widths)
    res["level_launches"] = {"per_level": len(widths), "merged": merged_launches(widths)}
    res["frame_V0_ms"] = frame_ms(sc, "V0")
    dv = {w: torch.tensor(deform(P0, w), dtype=torch.float64, device="cuda:0") for w in ("V1", "V2")}
    torch.cuda.synchronize()
    upd = lambda: sc.bih_update(tree, dv["V1"])
    res["update_per_level_ms"] = spread(upd)
    os.environ["GLOME_DEBUG_BIH_UPDATE_MERGED"] = "1"
    res["update_ms"] = spread(upd)
    del os.environ["GLOME_DEBUG_BIH_UPDATE_MERGED"]
    os.environ["GLOME_DEBUG_BIH_UPDATE_SPLIT"] = "1"
    for form in ("per_level", "merged"):
        if form == "merged":
            os.environ["GLOME_DEBUG_BIH_UPDATE_MERGED"] = "1"
        tri, lev, bnd = (float(x) for x in timed(upd, pairs=3))
        res["split_" + form + "_ms"] = {"triangle_records": tri, "levels": lev, "root_box": bnd}
    del os.environ["GLOME_DEBUG_BIH_UPDATE_MERGED"], os.environ["GLOME_DEBUG_BIH_UPDATE_SPLIT"]
    for w in ("V1", "V2"):
        sc.bih_update(tree, dv[w])
        ctx.synchronize()
        fresh = commit(deform(P0, w), True)[0]
        res["stale_" + w] = {"refit_frame_ms": frame_ms(sc, w), "fresh_frame_ms": frame_ms(fresh, w)}
        res["stale_" + w]["refit_over_fresh"] = res["stale_" + w]["refit_frame_ms"] / res["stale_" + w]["fresh_frame_ms"]
        fresh.release()
    res["commit_alone_ms"] = {"min": min(commit_only), "median": sorted(commit_only)[len(commit_only) // 2]}
    res["bih_dev_commit_over_update"] = res["bih_dev_commit_ms"] / res["update_per_level_ms"]["median"]
    sc.release()
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
