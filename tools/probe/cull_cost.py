"""What does the cull pass cost where nothing can be culled?  Renders the flagship frame (SCENE=S3, 1920 x 1080) in launches of 8 frames,
one launch at a time, from straight above the terrain looking down, so that every work item has a ray that enters the root box
(live == total: the cull pass removes nothing and the render kernel does all the parent's work), then with the scene's own camera.

  python tools/probe/cull_cost.py                                   ms per frame of both views, and what the cull pass found
  GLOME_DEBUG_LIB=<the parent's library> python tools/probe/cull_cost.py      the same launches without a cull pass
  KIND=down rocprofv3 --kernel-trace --stats ... -- python tools/probe/cull_cost.py     k_cull_items' own duration in the kernel statistics

Through the C ABI as glome_amd binds it (include/glome_hip.h); reads nothing but the scene."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GROUP = 8


def main():
    import numpy as np
    import torch
    from glome_amd import _lib as L, api, scenes
    name = os.environ.get("SCENE", "S3")
    cfg = scenes.CONFIGS[name]
    W, H = cfg["width"], cfg["height"]
    P = api.render_params(width=W, height=H, maxdepth=cfg["maxdepth"])
    sd = cfg["make"]()
    b = api.Builder()
    nm, _ = sd.replay(b)
    ctx = api.Context(0)
    sc = ctx.commit(b, nm[sd.root])
    lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
    la = (L.Light * max(1, len(lights)))(*lights)
    cams = {"scene": api.camera(*sd.cam),
            # from y = 4.5 the frame's widest ray meets the box's top (y ~ 1.55) 16 / 9 * 2.95 = 5.3 units from the centre: inside x, z in [-10, 10]
            "down": api.camera_from_vectors((0.0, 4.5, 0.0), (0, -1, 0), (0, 0, -1), (1, 0, 0))}
    buf = torch.zeros((GROUP, H, W), dtype=torch.int32, device=torch.device("cuda:0"))
    reps = int(os.environ.get("REPS", "20"))
    kinds = [k for k in ("down", "scene") if os.environ.get("KIND", "both") in (k, "both")]
    for kind in kinds:
        ca = (L.Camera * GROUP)(*([cams[kind]] * GROUP))
        for i in range(reps + 3):
            if i == 3:
                ctx.lib.glome_ctx_timing_begin(ctx.h, reps)
            assert ctx.lib.glome_render_packed_batch_dev(sc.h, ca, GROUP, la, len(lights), C.byref(P), C.c_void_p(buf.data_ptr()), H * W, None) == 0, ctx.err()
            ctx.synchronize()
        ms = np.zeros(reps, np.float32)
        n = ctx.lib.glome_ctx_timing_end(ctx.h, ms.ctypes.data_as(L.c_fp), reps)
        live, total = C.c_int64(-1), C.c_int64(-1)
        if hasattr(ctx.lib, "glome_ctx_last_cull"):  # (a library from before the cull pass, loaded through GLOME_DEBUG_LIB, has none)
            assert ctx.lib.glome_ctx_last_cull(ctx.h, C.byref(live), C.byref(total)) == 0, ctx.err()
            if kind == "down":
                assert live.value == total.value, "the view from above has dead items"
        med, lo, hi = float(np.median(ms[:n])), float(ms[:n].min()), float(ms[:n].max())
        print(json.dumps({"scene": name, "kind": kind, "frames_per_launch": GROUP, "launches": n, "live": live.value, "total": total.value,
                          "ms_per_frame_median": round(med / GROUP, 4), "ms_per_frame_min": round(lo / GROUP, 4), "ms_per_frame_max": round(hi / GROUP, 4),
                          "launch_ms_median": round(med, 4), "lib": os.environ.get("GLOME_DEBUG_LIB", "in-tree")}), flush=True)
    sc.release()
    ctx.close()


if __name__ == "__main__":
    main()
