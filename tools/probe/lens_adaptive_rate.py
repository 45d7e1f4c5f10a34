"""glome_render_lens_adaptive against glome_render_lens on the flagship frame (DESIGN.md 4.7's lens protocol): S3 at 1920 x 1080, thin
lens, jittered, maxdepth 3, device frame pointers, no statistics.
  (a) glome_render_lens_dev at samples = 16: what the adaptive frame is compared against, measured in the same run
  (b) glome_render_lens_adaptive_dev at (base, max) = (4, 16) with the default threshold
Event time: the library's event pairs (glome_ctx_timing_begin / _end), every launch of a frame summed.  Wall time: the host's clock
around the call and a synchronize, because the waits between (b)'s rounds do not show in the event pairs.  Two warm-up frames, median
of 7.  Also: the mean count, the share of pixels per level, the stream waits of a frame (one per round of a pass that reads its list's
length back: every level a pass reaches but max).
Run from the repository root: python tools/probe/lens_adaptive_rate.py [out.json]"""
import ctypes as C
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from glome_amd import api, scenes

W, H, MAXDEPTH, BASE, MAX, WARM, REPS, CAP = 1920, 1080, 3, 4, 16, 2, 7, 512


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
    pos, at = np.array(sd.cam[0], np.float64), np.array(sd.cam[1], np.float64)
    focus = float(np.linalg.norm(at - pos))
    aperture = 0.01 * focus
    lib, dev = sc.lib, torch.device("cuda:0")
    rp = api.raygen_params(width=W, height=H, lens=api.LENS_THIN, samples=MAX, jitter=1, seed=1, aperture=aperture, focus_dist=focus)
    tp, ap = api.trace_params(maxdepth=MAXDEPTH), api.adaptive_params()
    assert (ap.base_samples, MAX) == (BASE, 16)
    frame = torch.zeros((W * H, 5), dtype=torch.float32, device=dev)
    words = torch.zeros((W * H,), dtype=torch.int32, device=dev)
    counts = torch.zeros((W * H,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def fixed():
        sc.render_lens_dev(cam, lights, rp, tp, frame.data_ptr(), words.data_ptr(), want_stats=False)

    def adaptive():
        sc.render_lens_adaptive_dev(cam, lights, rp, ap, tp, frame.data_ptr(), words.data_ptr(), counts.data_ptr(), want_stats=False)

    def measure(fn):
        for _ in range(WARM):
            fn()
        ctx.synchronize()
        ev, wall, launches = [], [], 0
        for _ in range(REPS):
            assert lib.glome_ctx_timing_begin(ctx.h, CAP) == 0
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = (C.c_float * CAP)()
            launches = lib.glome_ctx_timing_end(ctx.h, ms, CAP)
            assert 0 < launches < CAP
            ev.append(float(sum(ms[:launches])))
        return {"event_ms": float(np.median(ev)), "wall_ms": float(np.median(wall)), "launches": int(launches)}, [float(x) for x in ms[:launches]]

    res = {"scene": "S3", "width": W, "height": H, "maxdepth": MAXDEPTH, "lens": "thin", "aperture": aperture, "focus_dist": focus, "jitter": 1,
           "warmup": WARM, "reps": REPS, "base": BASE, "max": MAX, "threshold": ap.threshold,
           "note": "base and threshold are the library's defaults: a first guess, not tuned"}
    res["render_lens_16"], each = measure(fixed)
    res["render_lens_16"]["event_ms_by_stage"] = {k: sum(each[i::3]) for i, k in enumerate(("raygen", "trace", "resolve"))}  # (the last frame's launches)
    st = sc.render_lens_dev(cam, lights, rp, tp, frame.data_ptr(), words.data_ptr())
    res["render_lens_16"]["rays_primary"] = st["rays_primary"]
    res["render_lens_adaptive_4_16"], each = measure(adaptive)
    st = sc.render_lens_adaptive_dev(cam, lights, rp, ap, tp, frame.data_ptr(), words.data_ptr(), counts.data_ptr())
    c = counts.cpu().numpy()
    levels = api.adaptive_levels(BASE, MAX)

    def rounds(per_pass, each):
        """the stream waits of a frame, and its launches' event times summed by (stage, level): a pass runs a round per level it
        reaches, three launches a round"""
        waits, order, by = 0, [], {}
        for p0 in range(0, W * H, per_pass):
            top = int(c[p0:p0 + per_pass].max())
            waits += sum(1 for l in levels[:-1] if l <= top)
            order += [(k, l) for l in levels if l <= top for k in ("raygen", "trace", "fold")]
        assert len(order) == len(each)
        for (k, l), ms in zip(order, each):
            by["%s@%d" % (k, l)] = by.get("%s@%d" % (k, l), 0.0) + ms
        return waits, by

    per_pass = (1 << 22) // MAX
    waits, by = rounds(per_pass, each)
    a = res["render_lens_adaptive_4_16"]
    a["rays_primary"] = st["rays_primary"]
    a["mean_count"] = float(c.mean())
    a["share_per_level"] = {str(l): float((c == l).mean()) for l in levels}
    a["stream_waits_per_frame"] = waits
    a["event_ms_by_stage_and_level"] = by  # (the last frame's launches)
    a["rays_per_level"] = {str(l): int((c >= l).sum()) * (l if l == BASE else l // 2) for l in levels}
    a["passes"] = (W * H + per_pass - 1) // per_pass
    res["adaptive_over_fixed_event"] = a["event_ms"] / res["render_lens_16"]["event_ms"]
    res["adaptive_over_fixed_wall"] = a["wall_ms"] / res["render_lens_16"]["wall_ms"]
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
    sc.release()
    ctx.close()


if __name__ == "__main__":
    main()
