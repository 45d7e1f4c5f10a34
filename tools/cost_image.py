"""Where does a frame spend its work?  The per-ray work records of a frame's primary rays (Scene.cost_image: glome_trace_work_batch over
api.frame_rays), as
  <out>.npy   the records, (height, width, 8) uint32 (the words: include/glome_hip.h GLOME_WORK_*)
  <out>.ppm   the frame tinted as GlomeView's debug view tints it (get_color_debug, Glome.hs:35-41: r + (dbg mod 30) / 60, g + dbg / 1000,
              dbg = word 5, the BIH nodes the primary ray's closest hit entered)
  <out>.txt   a summary per 64-ray work item (words 0..2 summed over the item's rays: median, mean, p99, max, and the item that has the
              max), for the trace seam's items (64 consecutive rays of the row-major stream) and for the render loop's (8 x 8 pixel blocks)

usage: cost_image.py SCENE [WIDTH HEIGHT] [--maxdepth N] [--faithful] [--out PREFIX]
SCENE: S1 .. S5, S3mesh, TS (glome_amd/scenes.py CONFIGS; size and maxdepth default to the config's) or a name of tests/zoo.py."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glome_amd import api, scenes  # noqa: E402


def scene_of(name):
    if name in scenes.CONFIGS:
        cfg = scenes.CONFIGS[name]
        return cfg["make"](), cfg["width"], cfg["height"], cfg["maxdepth"]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import zoo
    if name not in zoo.ALL:
        sys.exit(f"unknown scene {name}: one of {sorted(scenes.CONFIGS)} or {sorted(zoo.ALL)}")
    return zoo.ALL[name](), 320, 180, 3


def item_lines(title, cost, where):
    """cost: work per item; where(i): what to print for item i"""
    i = int(np.argmax(cost))
    return [f"{title}: {cost.size} items",
            f"  work per item (bih_nodes + mesh_nodes + prim_tests of its rays): median {np.median(cost):.0f}  mean {cost.mean():.1f}  "
            f"p99 {np.quantile(cost, 0.99):.0f}  max {cost.max()}",
            f"  the item with the max: {where(i)}  ({cost.max() / max(1.0, cost.mean()):.1f} x the mean)"]


def summary(name, work, maxdepth, faithful, stats):
    h, w, _ = work.shape
    per_ray = work[..., 0:3].astype(np.uint64).sum(-1)
    lines = [f"cost image of {name} at {w} x {h}, maxdepth {maxdepth}, faithful {faithful}",
             f"  launch: kernel {stats['kernel_ms']:.3f} ms, rays {stats['rays_primary']} + {stats['rays_shadow']} shadow + {stats['rays_secondary']} secondary, "
             f"bih_nodes {stats['bih_nodes']}, mesh_nodes {stats['mesh_nodes']}, prim_tests {stats['prim_tests']}",
             f"  per ray: work median {np.median(per_ray):.0f}  mean {per_ray.mean():.1f}  max {per_ray.max()};  "
             f"word 5 (trace_debug's count) median {np.median(work[..., 5]):.0f}  mean {work[..., 5].mean():.1f}  max {work[..., 5].max()}"]
    flat = per_ray.ravel()
    n_items = (flat.size + 63) // 64
    stream = np.zeros(n_items * 64, np.uint64)
    stream[:flat.size] = flat
    lines += item_lines("the trace seam's items (64 consecutive rays, row major)", stream.reshape(n_items, 64).sum(1),
                        lambda i: f"item {i}: rays {64 * i} .. {min(flat.size, 64 * i + 64) - 1}, row {64 * i // w}, columns from {64 * i % w}")
    bw, bh = (w + 7) // 8, (h + 7) // 8
    pad = np.zeros((bh * 8, bw * 8), np.uint64)
    pad[:h, :w] = per_ray
    blocks = pad.reshape(bh, 8, bw, 8).sum(axis=(1, 3))
    lines += item_lines("the render loop's items (8 x 8 pixel blocks)", blocks.ravel(),
                        lambda i: f"block at pixel ({8 * (i % bw)}, {8 * (i // bw)})")
    rows = blocks.sum(1).astype(np.float64)
    band = max(1, bh // 8)
    lines.append("  share of the frame's work by band of block rows, top to bottom: " +
                 "  ".join(f"{rows[k:k + band].sum() / max(1.0, rows.sum()):.3f}" for k in range(0, bh, band)))
    return "\n".join(lines) + "\n"


def tinted_ppm(path, rgba, dbg):
    r = rgba[..., 0] + (dbg % 30) / 60.0
    g = rgba[..., 1] + dbg / 1000.0
    img = np.stack([r, g, rgba[..., 2]], -1)
    img = (np.floor(np.clip(img, 0.0, 1.0 - 1e-4) * 256)).astype(np.uint8)  # (cap1, Glome.hs:98-101)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("size", nargs="*", type=int)
    ap.add_argument("--maxdepth", type=int)
    ap.add_argument("--faithful", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    sd, w, h, md = scene_of(a.scene)
    if len(a.size) == 2:
        w, h = a.size
    elif a.size:
        ap.error("give WIDTH and HEIGHT, or neither")
    md = a.maxdepth or md
    out = a.out or f"cost_image_{a.scene}_{w}x{h}"
    ctx = api.Context(0)
    b = api.Builder()

    class Dev:  # long lists are built on the device (the same tree)
        def __getattr__(self, n): return getattr(b, n)
        def bih(self, ids): return ctx.bih(b, ids)[0] if len(ids) >= 4096 else b.bih(ids)
    nm, _ = sd.replay(Dev())
    sc = ctx.commit(b, nm[sd.root])
    cam = api.camera(*sd.cam)
    lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
    o, d = api.frame_rays(cam, w, h)
    r = sc.trace_work(o, d, lights, params=api.trace_params(maxdepth=md, faithful=int(a.faithful)))
    work = r["work"].reshape(h, w, -1)
    np.save(out + ".npy", work)
    tinted_ppm(out + ".ppm", r["rgba"].reshape(h, w, 4), work[..., 5].astype(np.float64))
    text = summary(a.scene, work, md, int(a.faithful), r["stats"])
    with open(out + ".txt", "w") as f:
        f.write(text)
    print(text, end="")
    sc.release()
    ctx.close()


if __name__ == "__main__":
    main()
