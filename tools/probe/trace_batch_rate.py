"""The rate of the trace seam on the flagship frame: S3 at 1920 x 1080, maxdepth 3, device-resident ray streams.
  (a) glome_trace_batch_dev over the frame's own primary rays in pixel row order
  (b) the same rays under a fixed random permutation
  (c) what a host with its own rays had before: glome_rayint_batch_dev, then one glome_shadow_batch_dev of as many rays
  (d) glome_render_dev of that frame: the ceiling
Warm, median of REPS launches.  (a), (b) and (d) are timed by the library's own event pairs (glome_ctx_timing_begin / _end); the batch
seams of (c) record none, so the context is put on torch's stream and (c) is bracketed by torch events there.
Run from the repository root: python tools/probe/trace_batch_rate.py [out.json]"""
import ctypes as C
import json
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from glome_amd import _lib as L
from glome_amd import api, scenes

REPS, W, H, MAXDEPTH = 25, 1920, 1080, 3


def frame_rays(cam, w, h):  # get_coordsf / get_rayint (Glome.hs:27-33, 119-140) in float64, rounded to unit fp32 directions
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xc, yc = ((x / w) * 2 - 1) * (w / h), -((y / h) * 2 - 1)
    pos, fwd, up, right = (np.array(list(v), np.float64) for v in (cam.pos, cam.fwd, cam.up, cam.right))
    d = fwd + right * (-xc[..., None]) + up * yc[..., None]
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3).astype(np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return np.broadcast_to(pos.astype(np.float32), d.shape).copy(), d


def main():
    sd = scenes.s3(224)
    ctx, b = api.Context(0), api.Builder()

    class Dev:  # (the tree of 100k triangles is built on the device, like bench.py's)
        def __getattr__(self, n): return getattr(b, n)
        def bih(self, ids): return ctx.bih(b, ids)[0] if len(ids) >= 4096 else b.bih(ids)
    nm, _ = sd.replay(Dev())
    sc = ctx.commit(b, nm[sd.root])
    cam = api.camera(*sd.cam)
    lights = [api.light(p, c, r, s) for (p, c, r, s) in sd.lights]
    la = (L.Light * len(lights))(*lights)
    lib, dev, n = sc.lib, torch.device("cuda:0"), W * H
    assert lib.glome_ctx_use_stream(ctx.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    o, d = frame_rays(cam, W, H)
    perm = np.random.default_rng(7).permutation(n)
    cols = lambda o, d: [torch.tensor(np.ascontiguousarray(a), device=dev) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2])]
    rows, shuffled = cols(o, d), cols(o[perm], d[perm])
    tmax = torch.full((n,), 1e6, dtype=torch.float32, device=dev)
    out = torch.zeros((n, 5), dtype=torch.float32, device=dev)
    t = torch.zeros(n, dtype=torch.float32, device=dev)
    prim = torch.zeros(n, dtype=torch.int32, device=dev)
    occ = torch.zeros(n, dtype=torch.uint8, device=dev)
    TP, RP = api.trace_params(maxdepth=MAXDEPTH), api.render_params(width=W, height=H, maxdepth=MAXDEPTH)
    vp = lambda x: C.c_void_p(x.data_ptr())

    def trace(c):
        assert lib.glome_trace_batch_dev(sc.h, n, *[vp(x) for x in c], None, la, len(lights), C.byref(TP), vp(out), None, None, None, None, None, None, None) == 0

    def render():
        assert lib.glome_render_dev(sc.h, C.byref(cam), la, len(lights), C.byref(RP), vp(out), None, None) == 0

    def two_seams():
        assert lib.glome_rayint_batch_dev(sc.h, n, *[vp(x) for x in rows], vp(tmax), vp(t), vp(prim), None, None, None, None) == 0
        assert lib.glome_shadow_batch_dev(sc.h, n, *[vp(x) for x in rows], vp(tmax), vp(occ)) == 0

    def library_timed(fn):
        for _ in range(3):
            fn()
        ctx.synchronize()
        assert lib.glome_ctx_timing_begin(ctx.h, REPS) == 0
        for _ in range(REPS):
            fn()
        ms = (C.c_float * REPS)()
        assert lib.glome_ctx_timing_end(ctx.h, ms, REPS) == REPS
        ctx.synchronize()
        return float(np.median(list(ms)))

    def torch_timed(fn):
        for _ in range(3):
            fn()
        ctx.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
        for e0, e1 in ev:
            e0.record(); fn(); e1.record()
        ctx.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    res = {"scene": "S3", "width": W, "height": H, "maxdepth": MAXDEPTH, "rays": n, "reps": REPS}
    res["render_ms"] = library_timed(render)
    res["trace_rows_ms"] = library_timed(lambda: trace(rows))
    res["trace_rows_ms_torch_events"] = torch_timed(lambda: trace(rows))  # (the same launch under the other clock: what (c) is comparable to)
    res["trace_shuffled_ms"] = library_timed(lambda: trace(shuffled))
    res["rayint_then_shadow_ms"] = torch_timed(two_seams)
    res["trace_rows_over_render"] = res["trace_rows_ms"] / res["render_ms"]
    res["trace_rows_over_two_seams"] = res["trace_rows_ms_torch_events"] / res["rayint_then_shadow_ms"]
    res["trace_shuffled_over_rows"] = res["trace_shuffled_ms"] / res["trace_rows_ms"]
    res["Mrays_per_s_rows"] = n / res["trace_rows_ms"] / 1e3
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    sc.release()
    ctx.close()


if __name__ == "__main__":
    main()
