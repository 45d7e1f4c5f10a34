"""The rate of glome_scene_mesh_update_dev on S3 as a mesh (100,352 triangles) and on the 1M-triangle mesh, beside what
it replaces, timed in the same run:
  update        median of REPS warm device-form updates, by the library's own event pairs (glome_ctx_timing_begin / _end)
  split         the same with one pair per stage (GLOME_DEBUG_MESH_UPDATE_SPLIT): triangle records, the level launches, the bound
  mesh_dev      glome_sb_mesh_dev + glome_scene_commit of the same arrays (wall clock, the scene ready to render)
  mesh_host     glome_sb_mesh + glome_scene_commit
  stale         the frame time of the refitted scene against a scene committed fresh from the same vertices, for V1 (a smooth
                displacement plus jitter) and V2 (scaled by 3 and translated; the camera follows)
Run from the repository root: python tools/probe/mesh_update_rate.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from glome_amd import _lib as L
from glome_amd import api, scenes

REPS = 25
SHIFT = np.array([40.0, 6.0, -30.0])


def mesh_arrays(N):
    V = scenes.heightfield_vertices(N).reshape(-1, 3)
    idx = np.arange((N + 1) * (N + 1)).reshape(N + 1, N + 1)
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    tris = np.full((2 * N * N, 8), -1, dtype=np.int32)
    tris[:, :3] = np.stack([np.stack([a, b, c], -1), np.stack([c, b, d], -1)], axis=2).reshape(-1, 3)
    tris[:, 6] = 0
    return V, tris


def deform(V0, which):
    if which == "V1":
        d = np.stack([0.25 * np.sin(0.7 * V0[:, 2] + 0.3), 0.3 * np.sin(0.5 * V0[:, 0]) * np.cos(0.4 * V0[:, 2]), 0.2 * np.cos(0.6 * V0[:, 0])], 1)
        return V0 + d + np.random.default_rng(7).uniform(-0.02, 0.02, V0.shape)
    return V0 * 3.0 + SHIFT


def camera(which):
    pos, at, up, angle = scenes.CUST_CAM
    if which == "V2":
        pos, at = tuple(np.array(pos) * 3.0 + SHIFT), tuple(np.array(at) * 3.0 + SHIFT)
    return api.camera(pos, at, up, angle)


def one(ctx, name, N, W, H):
    lib = ctx.lib
    V0, tris = mesh_arrays(N)
    none = np.zeros((0, 3))
    lights = [api.light(p, c) for p, c in scenes.LIGHTS[:1]]
    P = api.render_params(width=W, height=H, maxdepth=1)
    out = torch.zeros(W * H, dtype=torch.int32, device="cuda:0")

    def commit(V, on_device):
        b = api.Builder()
        mat = b.material_surface((0.8, 0.5, 0.4), 1, 0.2, 1, 0, 0)
        t0 = time.perf_counter()
        me = ctx.mesh(b, V, none, tris, [mat])[0] if on_device else b.mesh(V, none, tris, [mat])
        sc = ctx.commit(b, me)
        return sc, me, (time.perf_counter() - t0) * 1e3

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
        return float(timed(lambda: sc.render_dev(cam, lights, P, None, out.data_ptr(), want_stats=False))[0])

    res = {"mesh": name, "triangles": int(len(tris)), "vertices": int(len(V0)), "frame": [W, H]}
    commit(V0, True)[0].release()  # (warm: the first build pays for the process's first allocations)
    sc, me, res["mesh_dev_commit_ms"] = commit(V0, True)
    res["mesh_host_commit_ms"] = commit(V0, False)[2]
    res["level_launches"] = sc.info()["max_mesh_depth"] - 1
    res["frame_V0_ms"] = frame_ms(sc, "V0")
    dv = {w: torch.tensor(deform(V0, w), dtype=torch.float64, device="cuda:0") for w in ("V1", "V2")}
    torch.cuda.synchronize()
    res["update_ms"] = float(timed(lambda: sc.mesh_update(me, dv["V1"]))[0])
    os.environ["GLOME_DEBUG_MESH_UPDATE_SPLIT"] = "1"
    tri, lev, bnd = (float(x) for x in timed(lambda: sc.mesh_update(me, dv["V1"]), pairs=3))
    del os.environ["GLOME_DEBUG_MESH_UPDATE_SPLIT"]
    res["split_ms"] = {"triangle_records": tri, "levels": lev, "bound": bnd}
    res["level_launch_us"] = 1e3 * lev / max(1, res["level_launches"])
    res["levels_share_of_update"] = lev / (tri + lev + bnd)
    for w in ("V1", "V2"):
        sc.mesh_update(me, dv[w])
        ctx.synchronize()
        fresh, _, _ = commit(deform(V0, w), True)
        res["stale_" + w] = {"refit_frame_ms": frame_ms(sc, w), "fresh_frame_ms": frame_ms(fresh, w)}
        res["stale_" + w]["refit_over_fresh"] = res["stale_" + w]["refit_frame_ms"] / res["stale_" + w]["fresh_frame_ms"]
        fresh.release()
    res["mesh_dev_commit_over_update"] = res["mesh_dev_commit_ms"] / res["update_ms"]
    sc.release()
    return res


def main():
    ctx = api.Context(0)
    res = [one(ctx, "S3mesh", 224, 1920, 1080), one(ctx, "S5mesh", 708, 3840, 2160)]
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
