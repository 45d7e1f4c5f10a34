"""What the GPU tests of the scene updates compare: everything a committed scene answers, bit for bit (test_mesh_update_gpu.py,
test_bih_update_gpu.py, test_sphere_bih_update_gpu.py in full; the instance, nested and sources files take the frames and the comparison
and ask their own rays).  No test lives here."""
import numpy as np

from glome_amd import api

SIZE = (131, 66)  # an odd frame: tiles cut at both edges


def frames(sc, cam, lights, size=SIZE):
    out = {}
    for mode in (0, 1):
        img, packed, _ = sc.render(cam, lights, api.render_params(width=size[0], height=size[1], mode=mode, maxdepth=2))
        out[f"frame{mode}"], out[f"packed{mode}"] = img, packed
    return out


def answers(sc, cam, lights, rays, k=1.0, shift=np.zeros(3), hits_only_normals=False, size=SIZE):
    """everything a scene answers: the three per-ray seams on `rays` = (origins, directions), a frame in both render modes, the trace
    seam's rows.  k, shift: the similarity the pose applies, which the shadow distances and the inside points follow.
    hits_only_normals: the normal of a miss zeroed -- a miss has no normal (glome_hip.h), and under a Bound what is stored there differs
    between two commits of one builder (test_bih_update_gpu.py)"""
    ro, rd = rays
    out = frames(sc, cam, lights, size)
    hit = sc.rayint(ro, rd)
    out.update({"t": hit["t"], "prim": hit["prim"], "n": hit["n"], "tex8": hit["tex"]})
    out["shadow"] = sc.shadow(ro, rd, np.random.default_rng(24).uniform(1, 30 * k, size=len(ro)).astype(np.float32))
    out["inside"] = sc.inside((np.random.default_rng(25).uniform(-7, 7, size=(4000, 3)) * k + shift).astype(np.float32))
    tr = sc.trace(ro, rd, lights, params=api.trace_params(maxdepth=2), want_hit=True)
    out.update({"trace_" + key: tr[key] for key in ("rgba", "depth", "t", "prim", "n", "tex")})
    if hits_only_normals:
        out["n"] = np.where(hit["t"][:, None] >= 0, hit["n"], 0)
        out["trace_n"] = np.where(np.asarray(tr["t"]).reshape(-1, 1) >= 0, np.asarray(tr["n"]).reshape(len(ro), -1), 0)
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f"{what}: {key} differs in {int(np.sum(x != y))} of {x.size} values"
