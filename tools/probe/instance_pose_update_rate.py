"""The rate of glome_scene_instance_update_from_dev beside the existing fp64 call, timed in one session on the oak
alone (scenes.oak at age 11.4: 2,047 Instance items under one bih), all items named:
  pair_f64            glome_scene_instance_update_dev: 24 contiguous doubles per Instance, no conversion, no table
  pose_f32            POSE / fp32 dense: the pose replaces the matrix
  pose_f32_base       POSE / fp32 after base = each Instance's own committed matrix (the cylinder / cone case)
  forward_f32_s16     FORWARD / fp32 read out of a row-major [n, 4, 4] tensor
Each figure is the median of REPS warm device-form calls by the library's own event pairs (glome_ctx_timing_begin / _end: one pair per
call, the conversion inside it); `spread` is that measurement repeated RUNS times (min, median, max of the medians): what a difference
must exceed to count.  bytes_read_per_instance: what the call reads of the CALLER'S arrays; the three new forms also write and read
back 192 bytes of table per Instance.
Run from the repository root: python tools/probe/instance_pose_update_rate.py [out.json]"""
import json
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tools/probe")
import numpy as np
import torch

from instance_update_rate import oak_alone, pick_oak, built, spread
from glome_amd import api


def main():
    ctx = api.Context(0)
    b, nm, root = built(oak_alone())
    ids = pick_oak(b, root)["all"]
    sc = ctx.commit(b, root)
    own = np.stack([b.instance_transform(i) for i in ids])
    rng = np.random.default_rng(1)
    dev = torch.device("cuda:0")

    def pose_set(step):
        """a small sway after the base, and the same written out as a pose of its own at the Instance's place"""
        half = np.deg2rad(1.5 + step) / 2
        after = np.tile(np.array([0.02 * step, 0.0, 0.01, 0.0, np.sin(half), 0.0, np.cos(half), 1.0]), (len(ids), 1))
        alone = after.copy()
        alone[:, :3] += own[:, [3, 7, 11]]
        alone[:, 7] = rng.uniform(0.05, 0.1, len(ids))
        return after.astype(np.float32), alone.astype(np.float32)

    sets = [pose_set(0), pose_set(1)]
    pair = [np.stack([api.xfm_mult(api.xfm_from_pose(p[:3], p[3:7], p[7]), m) for p, m in zip(after.astype(np.float64), own)]) for after, _ in sets]
    fwd44 = []
    for M in pair:
        t = np.zeros((len(ids), 4, 4), np.float32)
        t[:, :3, :] = M[:, :12].reshape(-1, 3, 4)
        t[:, 3, 3] = 1.0
        fwd44.append(t)
    t_pair = [torch.tensor(M, dtype=torch.float64, device=dev) for M in pair]
    t_after = [torch.tensor(a, device=dev) for a, _ in sets]
    t_alone = [torch.tensor(a, device=dev) for _, a in sets]
    t_fwd = [torch.tensor(f, device=dev) for f in fwd44]
    t_base = torch.tensor(own, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    flip = [0]

    def alternating(fn):
        def go():
            flip[0] ^= 1
            fn(flip[0])
        return go

    calls = {
        "pair_f64": (192, alternating(lambda k: sc.instance_update_dev(ids, t_pair[k]))),
        "pose_f32": (32, alternating(lambda k: sc.instance_update_from(ids, t_alone[k], "pose"))),
        "pose_f32_base": (32 + 192, alternating(lambda k: sc.instance_update_from(ids, t_after[k], "pose", base=t_base))),
        "forward_f32_s16": (48, alternating(lambda k: sc.instance_update_from(ids, t_fwd[k], "forward"))),
    }
    res = {"scene": "oak_11.4", "instances": len(ids), "form": "_dev", "reps": "median of 25 calls, repeated 5 times"}
    for name, (nbytes, fn) in calls.items():
        res[name] = dict(spread(ctx, fn), bytes_read_per_instance=nbytes)
        assert ctx.lib.glome_ctx_synchronize(ctx.h) == 0, ctx.err()
    res["pair_f64_again"] = dict(spread(ctx, calls["pair_f64"][1]), bytes_read_per_instance=192)  # the first figure once more: the session's drift
    sc.release()
    ctx.close()
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
