"""The rate of an update under bihs plus the refits above it (glome_scene_nested_updates, glome_scene_bih_refit_dev)
beside what it replaces, timed in the same run:
  default       GlomeView's default scene (scenes.testscene(10), 720 x 480): 16 of the oak's 2,047 twigs moved (an Instance update, which
                refits the oak's bih), then the root bih refitted
  nff_100k      an NFF-shaped scene: root bih [tex (bih of 100,352 triangles), tex (bih of 9 triangles), 3 spheres]; all triangles of the
                large tree replaced (glome_scene_bih_update_dev), then the root refitted
  update        median of REPS warm sequences update + refits, device forms, by the library's own event pairs (glome_ctx_timing_begin /
                _end: one pair per call, summed per sequence); `spread` is the measurement repeated RUNS times (min, median, max)
  rebuild       the only road without the feature: the builder calls (set_* and bih_refit) plus glome_scene_commit (wall clock)
  frame         the scene's lone frame, the one an update feeds
Run from the repository root: python tools/probe/nested_update_rate.py [out.json]   (default profiles/nested_update_rate.json)"""
import ctypes as C
import json
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools/probe")
import numpy as np
import torch

from glome_amd import api, scenes
from glome_amd.scene import SceneDesc
from instance_update_rate import built, matrix_of

REPS, RUNS = 25, 5
W, H = 720, 480


def timed_seq(ctx, fn, calls):
    """median over REPS of the summed event times of one sequence of `calls` timed library calls"""
    lib = ctx.lib
    for _ in range(3):
        fn()
    ctx.synchronize()
    assert lib.glome_ctx_timing_begin(ctx.h, REPS * calls) == 0
    for _ in range(REPS):
        fn()
    ms = (C.c_float * (REPS * calls))()
    assert lib.glome_ctx_timing_end(ctx.h, ms, REPS * calls) == REPS * calls
    ctx.synchronize()
    return float(np.median(np.array(list(ms)).reshape(REPS, calls).sum(axis=1)))


def spread(ctx, fn, calls=1):
    v = sorted(timed_seq(ctx, fn, calls) for _ in range(RUNS))
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}


def frame_fn(sc, sd):
    cam = api.camera(*sd.cam)
    lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
    RP = api.render_params(width=W, height=H, maxdepth=3)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")
    return lambda: sc.render_dev(cam, lights, RP, None, out.data_ptr(), want_stats=False), out


def wall(fn, n=5):
    v = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t0) * 1e3)
    return {"min": min(v), "median": sorted(v)[n // 2]}


def default_scene(ctx):
    res = {"scene": "default_scene", "frame": [W, H]}
    sd = scenes.testscene(10)
    b, nm, root = built(sd)
    oak = b.bih_items(root)[4]
    oak_bih = oak - 3
    twigs = b.bih_items(oak_bih)
    ids = twigs[100:2020:120]
    base = np.stack([matrix_of(b, i) for i in ids])
    sway = api.compose([api.rotate((0, 1, 0), api.deg(3)), api.translate((0.02, 0.0, 0.01))])
    moved = np.stack([api.compose([m, sway]) for m in base])
    sc = ctx.commit(b, root)
    sc.nested_updates(True)
    frame, keep = frame_fn(sc, sd)
    res["frame_ms"] = spread(ctx, frame)
    t = [torch.tensor(x, dtype=torch.float64, device="cuda:0") for x in (moved, base)]
    torch.cuda.synchronize()
    above = sc.bihs_above(ids[0])
    assert above == [oak_bih, root]
    flip = [0]

    def seq():
        flip[0] ^= 1
        sc.instance_update_dev(ids, t[flip[0]])
        sc.bih_refit_dev(root)   # (the Instance update has refitted the oak's bih itself)
    res["update_and_refits_ms"] = dict(spread(ctx, seq, 2), instances=len(ids), refits=1)
    res["frame_after_ms"] = spread(ctx, frame)
    sc.release()
    flip = [0]

    def rebuild():
        flip[0] ^= 1
        b.instance_set_transforms(ids, (moved, base)[flip[0]])
        b.bih_refit(root)
        ctx.commit(b, root).release()
    res["builder_calls_and_commit_ms"] = wall(rebuild)
    return res


def nff_100k(ctx):
    res = {"scene": "nff_100k", "frame": [W, H]}
    N = 224
    sd = SceneDesc(round32=False)
    P0 = scenes.heightfield_triangles(N)
    big = sd.bih(sd.triangles_bulk(P0))
    small = sd.bih(sd.triangles_bulk(scenes.heightfield_triangles(3)[:9] * 0.1 + 4.0))
    items = [sd.tex(big, scenes.matte(sd, (0.8, 0.5, 0.4))), sd.tex(small, scenes.matte(sd, (0.3, 0.5, 0.9)))]
    items += [sd.sphere(c, 0.8) for c in ((0.0, 4.0, 0.0), (5.0, 3.5, 2.0), (-4.0, 3.0, -3.0))]
    top = sd.bih(items)
    sd.set_root(top)
    for pos, col in scenes.LIGHTS[:2]:
        sd.add_light(pos, col)
    sd.set_camera(*scenes.CUST_CAM)
    b, nm, root = built(sd)
    res["triangles"] = int(P0.shape[0])
    P1 = P0.reshape(-1, 3).copy()
    P1[:, 1] += 0.2 * np.sin(0.5 * P1[:, 0]) * np.cos(0.4 * P1[:, 2])
    P1 = P1.reshape(-1, 9)
    sc = ctx.commit(b, root)
    sc.nested_updates(True)
    frame, keep = frame_fn(sc, sd)
    res["frame_ms"] = spread(ctx, frame)
    t = [torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda:0") for x in (P1, P0)]
    torch.cuda.synchronize()
    assert sc.bihs_above(nm[big]) == [root]
    flip = [0]

    def seq():
        flip[0] ^= 1
        sc.bih_update(nm[big], t[flip[0]])
        sc.bih_refit_dev(root)
    res["update_and_refits_ms"] = dict(spread(ctx, seq, 2), refits=1)
    res["frame_after_ms"] = spread(ctx, frame)
    sc.release()
    flip = [0]

    def rebuild():
        flip[0] ^= 1
        b.bih_set_triangles(nm[big], (P1, P0)[flip[0]])
        b.bih_refit(root)
        ctx.commit(b, root).release()
    res["builder_calls_and_commit_ms"] = wall(rebuild, 3)
    return res


def main():
    ctx = api.Context(0)
    res = [default_scene(ctx), nff_100k(ctx)]
    print(json.dumps(res))
    path = sys.argv[1] if len(sys.argv) > 1 else "profiles/nested_update_rate.json"
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
