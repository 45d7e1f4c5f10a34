"""What does a work item cost before and after its walks?  Renders the flagship frame (SCENE=S3, 1920 x 1080) in launches of 8 frames,
one launch at a time, twice: with the scene's camera, and with the camera turned straight up from above the terrain, so that every ray
misses the scene's root box -- an all-sky frame, whose items walk nothing: its time per item is the fixed price of an item (ticket,
item -> pixel, pixel -> ray, the root box test, the stores).

  python tools/probe/item_overhead.py                       ms per frame and launch time per item, both kinds
  KIND=sky|scene|down python tools/probe/item_overhead.py   one kind only (down: from straight above, every item live): the workload for a counter pass, e.g.
      PMC_SCRIPT=tools/probe/item_overhead.py KIND=sky tools/pmc_pass.sh OUT "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_INSTS_BRANCH"
  python tools/probe/item_overhead.py --pmc OUT/pass1       instructions per item by kind from that pass's counter_collection.csv
  python tools/probe/item_overhead.py --pmc OUT/pass1 --live N     the same per LIVE item: N = live_items_per_launch of a KIND=scene run (what the
      cull pass queued, glome_ctx_last_cull) -- the render kernel's instructions over the items it walks, and k_cull_items' over all items

Through the C ABI as glome_amd binds it (include/glome_hip.h); reads nothing but the scene."""
import collections
import csv
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GROUP = 8


def items_per_frame(P, width, height, blocksize=64):
    """64-pixel work items of a whole frame cut into 64 x 64 work tiles: the plan's own count (glome_items_layout); a library loaded through
    GLOME_DEBUG_LIB that predates that entry gets the same arithmetic (tiles.hpp chunk / tile_waves) from here"""
    from glome_amd import _lib as L
    lib = L.load()
    if hasattr(lib, "glome_items_layout"):
        return int(lib.glome_items_layout(C.byref(P), 0, 1, blocksize, 1, None, 0))

    def chunk(size):
        out, pos = [], 0
        while pos + blocksize < size:
            out.append(blocksize); pos += blocksize
        return out + [size - pos]

    def waves(w, h):
        blocks = (w // 8) * (h // 8)
        return blocks + (w * h - blocks * 64 + 63) // 64
    return sum(waves(w, h) for w in chunk(width) for h in chunk(height))


def summarise_pmc(passdir, items, kernel="k_render", per_launch=None):
    """mean per launch of every counter over the dispatches of `kernel` (run the pass with one KIND), per item: of `items` per frame, or of
    `per_launch` items in the whole launch"""
    per = collections.defaultdict(list)
    for f in sorted(glob.glob(passdir + "/**/*counter_collection.csv", recursive=True)):
        for r in csv.DictReader(open(f)):
            if kernel in r["Kernel_Name"]:
                per[r["Counter_Name"]].append(float(r["Counter_Value"]))
    out = {}
    for c, v in sorted(per.items()):
        out[c] = round(sum(v) / len(v) / (per_launch or items * GROUP), 1)
    out["all"] = round(sum(out.values()), 1)
    out["per_launch"] = round(sum(sum(v) / len(v) for v in per.values()))
    return out


def main():
    import numpy as np
    import torch
    from glome_amd import _lib as L, api, scenes
    name = os.environ.get("SCENE", "S3")
    cfg = scenes.CONFIGS[name]
    W, H = cfg["width"], cfg["height"]
    P = api.render_params(width=W, height=H, maxdepth=cfg["maxdepth"])
    n_items = items_per_frame(P, W, H)
    if "--pmc" in sys.argv:
        passdir = sys.argv[sys.argv.index("--pmc") + 1]
        out = {"pass": passdir, "items_per_frame": n_items, "frames_per_launch": GROUP, "instructions_per_item": summarise_pmc(passdir, n_items)}
        if "--live" in sys.argv:  # a flagship launch: the render kernel walks the live items only, the cull pass looks at every item
            live = int(sys.argv[sys.argv.index("--live") + 1])
            out["live_items_per_launch"] = live
            out["instructions_per_live_item"] = summarise_pmc(passdir, n_items, per_launch=live)
            out["cull_pass_instructions_per_item"] = summarise_pmc(passdir, n_items, kernel="k_cull_items")
        print(json.dumps(out))
        return
    sd = cfg["make"]()
    b = api.Builder()
    nm, _ = sd.replay(b)
    ctx = api.Context(0)
    sc = ctx.commit(b, nm[sd.root])
    lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
    la = (L.Light * max(1, len(lights)))(*lights)
    pos = sd.cam[0]
    cams = {"scene": api.camera(*sd.cam),
            # straight up from above everything: a ray's y component is fwd's 1 whatever the pixel, and the heightfield ends at y = 1.6
            "sky": api.camera_from_vectors((pos[0], max(float(pos[1]), 3.0), pos[2]), (0, 1, 0), (0, 0, 1), (1, 0, 0)),
            # cull_cost.py's view from straight above (KIND=down only): every item live, the cull pass's probe proves them all
            "down": api.camera_from_vectors((0.0, 4.5, 0.0), (0, -1, 0), (0, 0, -1), (1, 0, 0))}
    buf = torch.zeros((GROUP, H, W), dtype=torch.int32, device=torch.device("cuda:0"))
    reps = int(os.environ.get("REPS", "20"))
    kinds = [k for k in ("scene", "sky") if os.environ.get("KIND", "both") in (k, "both")] + (["down"] if os.environ.get("KIND") == "down" else [])
    for kind in kinds:
        ca = (L.Camera * GROUP)(*([cams[kind]] * GROUP))
        for i in range(reps + 3):
            if i == 3:
                ctx.lib.glome_ctx_timing_begin(ctx.h, reps)
            assert ctx.lib.glome_render_packed_batch_dev(sc.h, ca, GROUP, la, len(lights), C.byref(P), C.c_void_p(buf.data_ptr()), H * W, None) == 0, ctx.err()
            ctx.synchronize()
        ms = np.zeros(reps, np.float32)
        n = ctx.lib.glome_ctx_timing_end(ctx.h, ms.ctypes.data_as(L.c_fp), reps)
        frame = buf[GROUP - 1].cpu().numpy()
        hit = float((frame != 0).mean())
        if kind == "sky":
            assert hit == 0.0, "the all-sky camera sees the scene"
        med, lo, hi = float(np.median(ms[:n])), float(ms[:n].min()), float(ms[:n].max())
        live = None  # what the cull pass of the last launch queued (a flagship launch of a library that has the pass)
        if hasattr(ctx.lib, "glome_ctx_last_cull"):
            lv, tot = C.c_int64(-1), C.c_int64(-1)
            if ctx.lib.glome_ctx_last_cull(ctx.h, C.byref(lv), C.byref(tot)) == 0 and tot.value == GROUP * n_items:
                live = lv.value
        print(json.dumps({"scene": name, "kind": kind, "frames_per_launch": GROUP, "items_per_frame": n_items, "launches": n,
                          "ms_per_frame_median": round(med / GROUP, 4), "ms_per_frame_min": round(lo / GROUP, 4), "ms_per_frame_max": round(hi / GROUP, 4),
                          "ns_per_item_of_the_launch": round(med * 1e6 / (GROUP * n_items), 2), "live_items_per_launch": live, "pixels_hit": round(hit, 4), "lib": os.environ.get("GLOME_DEBUG_LIB", "in-tree")}), flush=True)
    sc.release()
    ctx.close()


if __name__ == "__main__":
    main()
