"""GPU suite (-m gpu): the frame-memory brim through the C ABI (tests/frame_towers.py; the CPU side is tests/test_frame_words_host.py).

Every accepted brim scene -- the tallest tower of a frame kind that commit accepts, within one InnerBound frame of kVmWords -- answers its
mixed batch through glome_rayint_batch, glome_shadow_batch, glome_inside_batch and glome_trace_batch (production and faithful) with status
0, ray by ray as the fp64 oracle does and in every decision as the host build of the device headers does, and the same with the
interpreter's packet service switched off; the next scene up is refused by glome_scene_commit.  Over the allowance a ray is answered while
the memory lasts, and at the brim the call returns GLOME_E_LIMIT -- a status, with every other ray of the batch answered and the context
fit for the next call.

Against the host build the answers are compared in their decisions, not bit for bit: every tower stands under an Instance, and below an
Instance tests/test_lattice_gpu.py asserts no bit identity with the host build either (the two contract the matrix products differently).
Bit for bit are what the lattice holds so: the production trace against the faithful one, and every answer with the packet service on
against the same with it off."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_towers as FT
from frame_towers import BRIMS, K, LIGHTS, depth_ok, family
from glome_amd import _lib as L
from glome_amd import api

pytestmark = pytest.mark.gpu


def commit(ctx, sd, packets=True):
    b = api.Builder()
    nm, _ = sd.replay(b)
    if not packets:
        os.environ["GLOME_DEBUG_NO_GENERIC_PACKETS"] = "1"
    try:
        return b, nm, ctx.commit(b, nm[sd.root])
    finally:
        os.environ.pop("GLOME_DEBUG_NO_GENERIC_PACKETS", None)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("kind,bot", BRIMS)
def test_every_accepted_brim_scene_answers_with_status_0_as_the_oracle_does(gpu_ctx, kind, bot):
    tw, r = FT.brim_batch(kind, bot)
    o, d, tm = r.o, r.d, r.tmax
    assert len(o) > 128
    hs = FT.commit_host(tw.sd)[0]
    assert K["kVmWords"] - K["kVmIbR"] < hs.vm_words()[0] <= K["kVmWords"]
    ref = FT.oracle_answers(tw.sd, o, d, tm)
    pts = FT.inside_points(tw)
    orc, om, _ = FT.O.load_scene(tw.sd, use_float=False)
    ref_in = orc.inside(om[tw.sd.root], pts.astype(np.float64))
    host = hs.rayint(o, d, tm)
    host_sh, host_in = hs.shadow(o, d, tm), hs.inside(pts)
    host_lit = hs.trace(o, d, LIGHTS, 2, tmax=tm)[0]
    out = []
    for packets in (True, False):
        b, nm, sc = commit(gpu_ctx, tw.sd, packets)
        try:
            assert sc.info()["tier"] == 1
            got = sc.rayint(o, d, tm)  # (a status other than 0 raises)
            sh, ins = sc.shadow(o, d, tm), sc.inside(pts)
            faithful = sc.trace(o, d, [], tmax=tm, params=api.trace_params(maxdepth=1, faithful=1), want_hit=True)
            lean = sc.trace(o, d, [], tmax=tm, params=api.trace_params(maxdepth=1), want_hit=True)
            lit = sc.trace(o, d, [api.light(*l) for l in LIGHTS], tmax=tm, params=api.trace_params(maxdepth=2))
        finally:
            sc.release()
        what = "%s over %s, packets %s: " % (kind, bot, packets)
        for name, t in (("rayint", got["t"]), ("trace, faithful", faithful["t"]), ("trace", lean["t"])):
            assert depth_ok(t, ref["t"]).all(), what + name
            assert np.array_equal(t >= 0, host["t"] >= 0), what + name + " against the host build"
        assert np.array_equal(lit["depth"] < 999999.0, ref["t"] >= 0), what + "trace with a light"
        if kind in FT.WARP_KINDS:  # the tower is reached from the shader alone: the colours are the host build's (rays far from every edge)
            assert np.abs(lit["rgba"].astype(np.float64) - host_lit[:, :4]).max() <= 1e-4, what + "the Warp's colours"
        assert np.array_equal(sh, ref["shadow"]) and np.array_equal(sh, host_sh), what + "shadow"
        assert np.array_equal(ins, ref_in) and np.array_equal(ins, host_in), what + "inside"
        for k in ("t", "prim", "n", "tex"):
            assert same_bits(lean[k], faithful[k]) if lean[k].dtype == np.float32 else np.array_equal(lean[k], faithful[k]), what + "the two traces differ in " + k
        out.append((got, sh, ins, lean, lit))
    (g0, s0, i0, l0, c0), (g1, s1, i1, l1, c1) = out
    assert same_bits(g0["t"], g1["t"]) and np.array_equal(g0["prim"], g1["prim"]) and same_bits(g0["n"], g1["n"])
    assert np.array_equal(s0, s1) and np.array_equal(i0, i1) and same_bits(l0["t"], l1["t"]) and same_bits(c0["rgba"], c1["rgba"])


@pytest.mark.parametrize("kind,bot", [("xform", "sphere"), ("isect", "sphere"), ("xform", "chain_in"), ("warp_frame", "sphere"), ("warp_scene", "tri_bih")])
def test_the_next_scene_up_is_refused_at_commit(gpu_ctx, kind, bot):
    up = FT.tower(kind, bot, *FT.next_up(kind, bot))
    b = api.Builder()
    nm, _ = up.sd.replay(b)
    assert not gpu_ctx.lib.glome_scene_commit(gpu_ctx.h, b.h, int(nm[up.sd.root]))
    msg = gpu_ctx.err()
    assert "frame memory" in msg and "of %d words" % K["kVmWords"] in msg, msg


@pytest.mark.parametrize("kind,bot,mode", [("xform", "sphere_bih", 0), ("xform", "inst_bih", 1), ("diff", "sphere", 0), ("bih", "sphere", 1)])
def test_a_frame_of_a_brim_scene(gpu_ctx, kind, bot, mode):
    """glome_render over a brim scene, renderTile and the adaptive sampler: status 0 at the statistics read, the frame bit for bit the one
    with the packet service off, and the host build's frame but for the odd silhouette pixel (the bound of
    test_gpu_parity.test_gpu_equals_the_host_build_where_boxes_end_on_split_planes, whose frame has seven times the pixels)"""
    from helpers import HostSim, product_camera_lights
    tw = FT.tower(kind, bot, *FT.brim(kind, bot))
    cam, lights = product_camera_lights(tw.sd)
    w, h = (64, 48) if mode == 0 else (65, 48)
    frames = []
    for packets in (True, False):
        b, nm, sc = commit(gpu_ctx, tw.sd, packets)
        try:
            img, _, st = sc.render(cam, lights, api.render_params(width=w, height=h, mode=mode, maxdepth=2), want_packed=False)
            if packets: hs = HostSim(b, nm[tw.sd.root])
        finally:
            sc.release()
        frames.append(img.copy())
    assert same_bits(frames[0], frames[1])
    him = hs.render(cam, lights, w, h, 2)[0] if mode == 0 else hs.render_subsample(cam, lights, w, h, 2)[0]
    e = (np.abs(frames[0][..., :4] - him[..., :4]) / np.maximum(1, np.abs(him[..., :4]))).max(-1)
    assert int((e > 1e-4).sum()) <= 16, int((e > 1e-4).sum())
    assert (frames[0][..., 4] < 999999.0).sum() > w * h // 8  # (the tower fills the middle of the frame)


# ----------------------------------------------------------------------------------------------------------------------------- run-out
def raw_rayint(sc, o, d, tm):
    n, cols = sc._rays(o, d, tm)
    t = np.full(n, -7.5, np.float32); prim = np.zeros(n, np.int32); nx, ny, nz = (np.zeros(n, np.float32) for _ in range(3))
    tex = np.zeros((n, sc.lib.glome_tex_words()), np.int32)
    rc = sc.lib.glome_rayint_batch(sc.h, n, *[c.ctypes.data_as(L.c_fp) for c in cols], t.ctypes.data_as(L.c_fp), prim.ctypes.data_as(L.c_ip), nx.ctypes.data_as(L.c_fp),
                                   ny.ctypes.data_as(L.c_fp), nz.ctypes.data_as(L.c_fp), tex.ctypes.data_as(L.c_ip))
    return rc, sc.ctx.err(), t


def raw_shadow(sc, o, d, tm):
    n, cols = sc._rays(o, d, tm)
    occ = np.full(n, 7, np.uint8)
    rc = sc.lib.glome_shadow_batch(sc.h, n, *[c.ctypes.data_as(L.c_fp) for c in cols], occ.ctypes.data_as(L.c_bp))
    return rc, sc.ctx.err(), occ


def raw_trace(sc, o, d, tm, faithful):
    n, cols = sc._rays(o, d, tm)
    out = np.full((n, 5), -7.5, np.float32)
    P = api.trace_params(maxdepth=1, faithful=faithful)
    la = (L.Light * 1)()
    st = L.Stats()
    rc = sc.lib.glome_trace_batch(sc.h, n, *[c.ctypes.data_as(L.c_fp) for c in cols[:6]], cols[6].ctypes.data_as(L.c_fp), la, 0, C.byref(P), out.ctypes.data_as(L.c_fp),
                                  None, None, None, None, None, None, C.byref(st))
    return rc, sc.ctx.err(), out[:, 4]


@pytest.mark.parametrize("bot", ["carve", "carve_face", "carve_mesh", "chain2"])
def test_over_the_allowance_a_low_tower_answers_as_the_oracle_does(gpu_ctx, bot):
    """the allowance is no cap: 96 advances fit in an empty stack"""
    tw, hs, est, o, d, tm, cnt = family(bot, 2)
    assert cnt.max() > FT.ALLOWANCE[bot]
    ref = FT.oracle_answers(tw.sd, o, d, tm)
    b, nm, sc = commit(gpu_ctx, tw.sd)
    try:
        assert depth_ok(sc.rayint(o, d, tm)["t"], ref["t"]).all() and np.array_equal(sc.shadow(o, d, tm), ref["shadow"])
        assert depth_ok(sc.trace(o, d, [], tmax=tm, params=api.trace_params(maxdepth=1), want_hit=True)["t"], ref["t"]).all()
    finally:
        sc.release()


@pytest.mark.parametrize("kind,bot", [("xform", "carve"), ("xform", "carve_face"), ("xform", "carve_mesh"), ("xform", "chain2"), ("diff", "chain2")])
def test_at_the_brim_a_ray_over_the_allowance_ends_the_call_with_the_limit_status(gpu_ctx, kind, bot):
    """The rays the host build flags (tests/test_frame_words_host.py: the same header, the same guards, canaries intact) make every batch seam
    return GLOME_E_LIMIT with the device-side-limit message.  A host-buffer seam returns it before it copies anything out; through the
    device-pointer seams, where the status comes at glome_ctx_synchronize and the answers lie in the caller's own buffers, the flagged rays
    are answered a miss (or, the one that ends on the last word, the oracle's answer: see the host test) and every other ray of the batch as
    the oracle answers it.  A clean, correct call follows on the same context."""
    import torch
    tw = FT.tower(kind, bot, *FT.brim(kind, bot))
    o, d, tm, cnt = FT.FAMILY_RAYS[bot](tw.shift)
    hs = FT.commit_host(tw.sd)[0]
    flag_r = hs.frame_probe("rayint", o, d, tm)
    flag_s = hs.frame_probe("shadow", o, d, tm)
    assert flag_r["canary"].all() and flag_s["canary"].all() and flag_r["flag"].sum() >= 2
    ref = FT.oracle_answers(tw.sd, o, d, tm)
    fine = np.flatnonzero(~flag_r["flag"] & ~flag_s["flag"])
    assert len(fine) >= 8
    b, nm, sc = commit(gpu_ctx, tw.sd)

    def clean_call(after):
        assert depth_ok(sc.rayint(o[fine], d[fine], tm[fine])["t"], ref["t"][fine]).all(), after + ": the call after"
        assert np.array_equal(sc.shadow(o[fine], d[fine], tm[fine]), ref["shadow"][fine]), after + ": the call after"

    def limit_at_synchronize(what):
        with pytest.raises(api.GlomeError, match="device-side limit"):
            gpu_ctx.synchronize()
        gpu_ctx.synchronize()  # (read and cleared)

    try:
        for name, (rc, msg, t) in (("rayint", raw_rayint(sc, o, d, tm)), ("trace", raw_trace(sc, o, d, tm, 0)), ("trace, faithful", raw_trace(sc, o, d, tm, 1))):
            assert rc == L.E_LIMIT and "device-side limit" in msg, (name, rc, msg)
            clean_call(name)
        rc, msg, occ = raw_shadow(sc, o, d, tm)
        if flag_s["flag"].any():
            assert rc == L.E_LIMIT and "device-side limit" in msg, (rc, msg)
        else:
            assert rc == 0 and np.array_equal(occ != 0, ref["shadow"]), (rc, msg)
        clean_call("shadow")
        # the device-pointer seams
        dev = torch.device("cuda:0")
        cols = [torch.tensor(np.ascontiguousarray(a), device=dev) for a in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2], tm)]
        ptrs = [C.c_void_p(c.data_ptr()) for c in cols]
        t = torch.full((len(o),), -7.5, dtype=torch.float32, device=dev)
        occ = torch.full((len(o),), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert sc.lib.glome_rayint_batch_dev(sc.h, len(o), *ptrs, C.c_void_p(t.data_ptr()), None, None, None, None, None) == 0
        limit_at_synchronize("rayint")
        got = t.cpu().numpy()
        ok = ~flag_r["flag"]
        assert depth_ok(got[ok], ref["t"][ok]).all() and np.all((got[~ok] == -1.0) | depth_ok(got[~ok], ref["t"][~ok])) and (got[~ok] != -1.0).sum() <= (1 if bot == "carve_mesh" else 0) and (got[~ok] == -1.0).sum() >= 2
        assert sc.lib.glome_shadow_batch_dev(sc.h, len(o), *ptrs, C.c_void_p(occ.data_ptr())) == 0
        if flag_s["flag"].any(): limit_at_synchronize("shadow")
        else: gpu_ctx.synchronize()
        got = occ.cpu().numpy()
        assert np.array_equal(got[~flag_s["flag"]] != 0, ref["shadow"][~flag_s["flag"]]) and not got[flag_s["flag"]].any()
        for faithful in (0, 1):
            t.fill_(-7.5)
            rgbad = torch.zeros((len(o), 5), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            sc.trace_dev(len(o), [c.data_ptr() for c in cols], [], api.trace_params(maxdepth=1, faithful=faithful), rgbad.data_ptr(),
                         hit_ptrs=[t.data_ptr(), None, None, None, None, None], want_stats=False)
            limit_at_synchronize("trace")
            got = t.cpu().numpy()
            assert depth_ok(got[ok], ref["t"][ok]).all() and np.all((got[~ok] == -1.0) | depth_ok(got[~ok], ref["t"][~ok])) and (got[~ok] != -1.0).sum() <= (1 if bot == "carve_mesh" else 0) and (got[~ok] == -1.0).sum() >= 2, faithful
        clean_call("the device-pointer seams")
    finally:
        sc.release()


def test_a_frame_whose_rays_run_out_reports_the_limit_at_the_statistics_read(gpu_ctx):
    """a camera that looks down the axis of the brim tower over `carve` through one degree: the rays of the middle of the frame pass
    through all 48 carving spheres.  glome_render returns GLOME_E_LIMIT where it reads the statistics, and the next frame -- from the
    side, where no ray advances -- is clean."""
    from helpers import HostSim, product_camera_lights
    tw = FT.tower("xform", "carve", *FT.brim("xform", "carve"))
    cam = api.camera((0.0, 0.0, -8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0)
    _, lights = product_camera_lights(tw.sd)
    b, nm, sc = commit(gpu_ctx, tw.sd)
    try:
        hs = HostSim(b, nm[tw.sd.root])
        with pytest.raises(RuntimeError, match="rc=-2"):
            hs.render(cam, lights, 32, 24, 1)
        with pytest.raises(api.GlomeError, match=r"device-side limit.*\(status %d\)" % L.E_LIMIT):
            sc.render(cam, lights, api.render_params(width=32, height=24, maxdepth=1), want_packed=False)
        side = api.camera((0.0, 0.0, -8.0), (0.0, 4.0, 0.0), (0.0, 1.0, 0.0), 1.0)
        img, _, st = sc.render(side, lights, api.render_params(width=32, height=24, maxdepth=1), want_packed=False)
        assert st["rays_primary"] == 32 * 24
        him = hs.render(side, lights, 32, 24, 1)[0]
        assert int(((np.abs(img[..., :4] - him[..., :4]) / np.maximum(1, np.abs(him[..., :4]))).max(-1) > 1e-4).sum()) <= 16
    finally:
        sc.release()
