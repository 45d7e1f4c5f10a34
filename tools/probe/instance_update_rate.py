"""The rate of glome_scene_instance_update_dev beside what it replaces, timed in the same run:
  oak           scenes.oak at age 11.4 alone (2,047 Instance items under one bih, 720 x 480): all items updated, and 16 of them
  default       GlomeView's default scene (scenes.testscene(10), 720 x 480): the door, the glass and the whole-oak Instances, items of
                the root bih, updated
  update        median of REPS warm device-form calls, by the library's own event pairs (glome_ctx_timing_begin / _end); `spread` is the
                same measurement repeated RUNS times (min, median, max of the medians): what a difference must exceed to count
  rebuild       the road an update replaces: the scene made again in a new builder and committed (wall clock, the scene ready to render)
  commit        glome_scene_commit by itself (wall clock), which since this feature also makes the update's tables
  frame         the scene's lone frame, the one an update feeds
Run from the repository root: python tools/probe/instance_update_rate.py [out.json]
With `commit` as the first argument it only times glome_scene_commit on TS and S3 (min and median of five), for a comparison of two
builds of the library through GLOME_DEBUG_LIB: python tools/probe/instance_update_rate.py commit"""
import ctypes as C
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from glome_amd import api, scenes
from glome_amd.scene import SceneDesc

REPS, RUNS = 25, 5
W, H = 720, 480


def timed(ctx, fn):
    lib = ctx.lib
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


def spread(ctx, fn):
    v = sorted(timed(ctx, fn) for _ in range(RUNS))
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}


def built(sd):
    """(builder, root, builder + commit wall-clock parts are the caller's)"""
    b = api.Builder()
    nm, _ = sd.replay(b)
    return b, nm, nm[sd.root]


def matrix_of(b, node):
    """the 24 doubles of an Instance, from the builder's `show` text"""
    import re
    text = b.show(node)
    at = text.rindex("(Xfm (Matrix ")
    nums = re.findall(r"-?\d+\.\d+(?:e-?\d+)?", text[at:])
    return np.array([float(x) for x in nums[:24]])


def scene(ctx, name, make, pick):
    res = {"scene": name, "frame": [W, H]}
    t0 = time.perf_counter()
    sd = make()
    b, nm, root = built(sd)
    t1 = time.perf_counter()
    sc = ctx.commit(b, root)
    t2 = time.perf_counter()
    sc.release()
    walls, commits = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        sd = make()
        b, nm, root = built(sd)
        t1 = time.perf_counter()
        sc = ctx.commit(b, root)
        t2 = time.perf_counter()
        walls.append((t2 - t0) * 1e3); commits.append((t2 - t1) * 1e3)
        sc.release()
    sc = ctx.commit(b, root)
    res["rebuild_and_commit_ms"] = {"min": min(walls), "median": sorted(walls)[2]}
    res["commit_alone_ms"] = {"min": min(commits), "median": sorted(commits)[2]}
    cam = api.camera(*sd.cam)
    lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
    RP = api.render_params(width=W, height=H, maxdepth=3)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
    res["frame_ms"] = spread(ctx, lambda: sc.render_dev(cam, lights, RP, None, out.data_ptr(), want_stats=False))
    for label, ids in pick(b, root).items():
        base = np.stack([matrix_of(b, i) for i in ids])
        sway = api.compose([api.rotate((0, 1, 0), api.deg(3)), api.translate((0.02, 0.0, 0.01))])
        moved = np.stack([api.compose([m, sway]) for m in base])
        t = [torch.tensor(x, dtype=torch.float64, device="cuda:0") for x in (moved, base)]
        torch.cuda.synchronize()
        flip = [0]

        def upd():
            flip[0] ^= 1
            sc.instance_update_dev(ids, t[flip[0]])
        res["update_" + label + "_ms"] = dict(spread(ctx, upd), instances=len(ids))
        sc.instance_update_dev(ids, t[1])
        ctx.synchronize()
        res["frame_over_update_" + label] = res["frame_ms"]["median"] / res["update_" + label + "_ms"]["median"]
        res["commit_over_update_" + label] = res["commit_alone_ms"]["median"] / res["update_" + label + "_ms"]["median"]
    res["frame_after_ms"] = spread(ctx, lambda: sc.render_dev(cam, lights, RP, None, out.data_ptr(), want_stats=False))
    sc.release()
    return res


def oak_alone():
    sd = SceneDesc()
    sd.set_root(scenes.oak(sd, 11.4, 42))
    for pos, col in scenes.LIGHTS[:2]:
        sd.add_light(pos, col)
    sd.set_camera((1.0, 5.0, 9.0), (0.0, 3.5, 0.0), (0.0, 1.0, 0.0), 55.0)
    return sd


def pick_oak(b, root):
    items = b.bih_items(root - 2)  # tag (tex (bih ...))
    assert len(items) == 2047
    return {"all": items, "16": items[100:2020:120]}


def pick_default(b, root):
    items = b.bih_items(root)
    door, glass, oak = items[6], items[7], items[4]
    return {"door_glass_oak": [door, glass, oak]}


def commit_only(ctx):
    res = {}
    for name, make in (("TS", lambda: scenes.testscene(10)), ("S3", lambda: scenes.s3(224))):
        b, nm, root = built(make())
        ctx.commit(b, root).release()
        v = []
        for _ in range(5):
            t0 = time.perf_counter()
            sc = ctx.commit(b, root)
            v.append((time.perf_counter() - t0) * 1e3)
            sc.release()
        res[name] = {"min": min(v), "median": sorted(v)[2]}
    return res


def main():
    ctx = api.Context(0)
    if len(sys.argv) > 1 and sys.argv[1] == "commit":
        print(json.dumps(commit_only(ctx)))
        ctx.close()
        return
    res = [scene(ctx, "oak_11.4", oak_alone, pick_oak), scene(ctx, "default_scene", lambda: scenes.testscene(10), pick_default)]
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
