"""GPU suite (-m gpu): the HIP path through the C ABI (include/glome_hip.h) against the oracle on seeded inputs, the
committed golden vectors, and -- at BASELINE.json's full sizes -- size-independent properties."""
import ctypes as C
import os

import numpy as np
import pytest

import parity
import zoo
from helpers import compare_images, oracle_for, product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api, dist, scenes

pytestmark = pytest.mark.gpu

SCENES = dict(zoo.ALL)
SCENES.update({"S1": lambda: scenes.s1(nlights=2), "S3small": lambda: scenes.s3(24), "S3mesh_small": lambda: scenes.s3(24, as_mesh=True), "S4": scenes.s4})


def commit(ctx, sd):
    b = api.Builder()
    nm, _ = sd.replay(b)
    return b, nm, ctx.commit(b, nm[sd.root])


@pytest.fixture(scope="module")
def s3_full(gpu_ctx):
    sd = scenes.s3(224)
    b, nm, sc = commit(gpu_ctx, sd)
    yield sd, sc
    sc.release()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_rayint_shadow_inside_vs_oracle(gpu_ctx, name):
    sd = SCENES[name]()
    b, nm, sc = commit(gpu_ctx, sd)
    parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, sd, nm, n=40000)
    sc.release()


@pytest.mark.parametrize("name", ["flat_mixed", "nested"])
def test_sixteen_lights(gpu_ctx, name):
    # the light list's capacity (kMaxLights): a flat-tier and a generic-tier scene under 16 lights of every kind
    sd = SCENES[name]()
    rng = np.random.default_rng(16)
    sd.lights = []
    for k in range(16):
        sd.add_light((float(rng.uniform(-20, 20)), float(rng.uniform(6, 40)), float(rng.uniform(-5, 40))), tuple(float(x) for x in rng.uniform(5, 60, 3)),
                     rad=float(rng.uniform(25, 60)) if k % 5 == 4 else 1000000.0, shadow=k % 4 != 3)
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    assert len(lights) == 16
    img, _, st = sc.render(cam, lights, api.render_params(width=200, height=120, maxdepth=2), want_packed=False)
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 200, 120, 2)
    sc.release()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_render_vs_oracle(gpu_ctx, name):
    sd = SCENES[name]()
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    img, packed, st = sc.render(cam, lights, api.render_params(width=320, height=180, maxdepth=3))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 320, 180, 3)
    # blitTile / rgbf (Glome.hs:353-358, 107-110): packed pixels follow from the float tuple
    r, g, bl, a = [img[..., k].astype(np.float32) for k in range(4)]
    cap = lambda x: np.where(x >= 1, np.float32(1 - 1e-4), x)
    want = (np.floor(cap(r * a) * 256).astype(np.int64) * 65536 + np.floor(cap(g * a) * 256).astype(np.int64) * 256 + np.floor(cap(bl * a) * 256).astype(np.int64)) & 0xFFFFFFFF
    assert np.mean(packed.astype(np.int64) == want) > 0.9999
    sc.release()


def test_golden_vectors_through_c_abi(gpu_ctx):
    import test_golden as tg
    for name in tg.NAMES:
        mg, g = tg.load_gold(name)
        sd = mg.SCENES[name]()
        b, nm, sc = commit(gpu_ctx, sd)
        ro, rd = mg.golden_inputs()
        cam, lights = product_camera_lights(sd)
        img, _, _ = sc.render(cam, lights, api.render_params(width=g["image"]["w"], height=g["image"]["h"], maxdepth=g["image"]["maxdepth"]))
        tg.compare_backend_to_gold(g, sc.rayint(ro, rd), sc.shadow(ro, rd, np.full(len(ro), g["shadow_tmax"], np.float32)), img, nm,
                                   getattr(sd, "same_prim_min", 0.97), getattr(sd, "normal_atol", 2e-3))
        sc.release()


# ------------------------------------------------------------------ full-size properties (1920x1080, 100k triangles)
def test_full_size_faithful_equals_early_out_and_is_deterministic(s3_full):
    sd, sc = s3_full
    cam, lights = product_camera_lights(sd)
    a, pa, sa = sc.render(cam, lights, api.render_params(width=1920, height=1080, maxdepth=1))
    b, pb, sb = sc.render(cam, lights, api.render_params(width=1920, height=1080, maxdepth=1))
    f, pf, sf = sc.render(cam, lights, api.render_params(width=1920, height=1080, maxdepth=1, faithful=1))
    assert np.array_equal(a, b) and np.array_equal(pa, pb)  # deterministic whatever the work-queue order
    assert np.array_equal(a, f) and np.array_equal(pa, pf)  # ordered early-out picks the same hits as the reference's traversal
    assert sa["rays_primary"] == 1920 * 1080 and (sa["rays_shadow"], sa["rays_secondary"]) == (sf["rays_shadow"], sf["rays_secondary"])
    assert sf["bih_nodes"] > 0 and sa["bih_nodes"] == 0
    hit = a[..., 3] > 0
    assert 0.3 < hit.mean() < 0.7 and np.all(a[..., 4][~hit] == 1e6) and np.all(a[..., :4][~hit] == 0)  # misses are transparent at depth = infinity


def test_full_size_counts_and_pixels_match_oracle_on_a_tile_sample(s3_full):
    """Every 37th 65x65 tile of the 1080p frame (14 tiles, ~59k pixels) rendered by the oracle; the GPU renders the same
    tiles: pixels within tolerance, ray counts equal, faithful node / primitive visit counts equal to the oracle's."""
    sd, sc = s3_full
    cam, lights = product_camera_lights(sd)
    o, om, _ = oracle_for(sd)
    ref, _, rc = o.render(1920, 1080, maxdepth=1, tile_first=3, tile_stride=37, nthreads=8, want_packed=False)
    init = np.zeros((1080, 1920, 5), np.float32)
    img, _, st = sc.render(cam, lights, api.render_params(width=1920, height=1080, maxdepth=1, tile_first=3, tile_stride=37, faithful=1), want_packed=False, init=init)
    owned = np.zeros((1080, 1920), bool)
    for x, y, w, h, _ in dist.owned_layout(api.render_params(width=1920, height=1080), 3, 37):
        owned[y:y + h, x:x + w] = True
    assert owned.sum() == st["n_pixels"] == rc["rays_primary"] == st["rays_primary"]
    assert np.all(img[~owned] == 0)  # tiles this call does not own are left untouched
    e = (np.abs(img[owned][:, :4] - ref[owned][:, :4]) / np.maximum(1, np.abs(ref[owned][:, :4]))).max(-1)
    parity._log("tile_sample_S3", sd, {"frac_over": float(np.mean(e > 1e-4)), "max": float(e.max())})
    assert np.mean(e > 1e-4) <= parity.PIXEL_OUTLIER_MAX
    assert st["rays_shadow"] == rc["rays_shadow"]
    assert abs(st["bih_nodes"] - rc["bih_nodes"]) <= rc["bih_nodes"] // 5000 + 4
    assert abs(st["prim_tests"] - rc["prim_tests"]) <= rc["prim_tests"] // 5000 + 4


def _same(a, b, what):
    """torch.equal with a report: how many elements differ and where the first ones are"""
    import torch
    if torch.equal(a, b):
        return True
    d = (a != b) & ~(torch.isnan(a) & torch.isnan(b)) if a.is_floating_point() else (a != b)
    idx = torch.nonzero(d)[:8].cpu().tolist()
    raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} elements differ, first at {idx}, got {[a[tuple(i)].item() for i in idx[:4]]} want {[b[tuple(i)].item() for i in idx[:4]]}")


@pytest.mark.parametrize("world,pct", [(2, 0), (8, 0), (8, 60), (3, 70)])
def test_full_size_tile_shards_reassemble_bit_exactly(gpu_ctx, s3_full, world, pct):
    """The multi-GPU data path on one GPU: each 'rank' renders its tiles (round robin, or rank 0 with less than a fair share:
    rank0_share_pct) into a dense payload, the payloads are blitted into a frame -- identical to the whole-frame render, bit
    for bit."""
    import torch
    sd, sc = s3_full
    cam, lights = product_camera_lights(sd)
    dev = torch.device("cuda:0")
    P = api.render_params(width=1920, height=1080, maxdepth=1, rank0_share_pct=pct)
    whole = torch.zeros((1080, 1920, 5), dtype=torch.float32, device=dev)
    sc.render_dev(cam, lights, P, whole.data_ptr())
    frame = torch.full((1080, 1920, 5), float("nan"), dtype=torch.float32, device=dev)
    la = (L.Light * len(lights))(*lights)
    tot = 0
    for r in range(world):
        plan = dist.ShardPlan(P, r, world)
        payload = torch.zeros(plan.maxp, dtype=torch.float32, device=dev)
        st = L.Stats()
        assert sc.lib.glome_render_tiles_dev(sc.h, C.byref(cam), la, len(lights), C.byref(plan.P_local), C.c_void_p(payload.data_ptr()), C.byref(st)) == 0
        tot += st.n_pixels
        assert sc.lib.glome_tiles_blit_dev(gpu_ctx.h, C.byref(plan.P), r, world, C.c_void_p(payload.data_ptr()), C.c_void_p(frame.data_ptr()), None) == 0
        # pack(frame-of-this-rank) == payload
        back = torch.zeros(plan.maxp, dtype=torch.float32, device=dev)
        assert sc.lib.glome_tiles_pack_dev(gpu_ctx.h, C.byref(plan.P_local), C.c_void_p(frame.data_ptr()), C.c_void_p(back.data_ptr())) == 0
        gpu_ctx.synchronize()
        _same(back[:plan.sizes[r]], payload[:plan.sizes[r]], f"pack(frame) vs payload of rank {r}")
    gpu_ctx.synchronize()
    assert tot == 1920 * 1080
    _same(frame, whole, "blitted shards vs whole frame")
    # the one-launch blit of all gathered slabs (what rank 0 runs after the gather)
    plans = [dist.ShardPlan(P, r, world) for r in range(world)]
    gathered = torch.zeros((world, plans[0].maxp), dtype=torch.float32, device=dev)
    for r in range(world):
        assert sc.lib.glome_render_tiles_dev(sc.h, C.byref(cam), la, len(lights), C.byref(plans[r].P_local), C.c_void_p(gathered[r].data_ptr()), None) == 0
    frame2 = torch.full((1080, 1920, 5), float("nan"), dtype=torch.float32, device=dev)
    assert sc.lib.glome_tiles_blit_all_dev(gpu_ctx.h, C.byref(P), world, C.c_void_p(gathered.data_ptr()), plans[0].maxp, C.c_void_p(frame2.data_ptr()), None) == 0
    gpu_ctx.synchronize()
    _same(frame2, whole, "one-launch blit vs whole frame")
    # the packed-pixel product: each rank's dense 0x00RRGGBB payload, one blit -> the packed framebuffer of the
    # whole-frame render (float tuple and packed pixel written together), and of a packed-only whole-frame render
    whole_px = torch.zeros((1080, 1920), dtype=torch.int32, device=dev)
    sc.render_dev(cam, lights, P, whole.data_ptr(), whole_px.data_ptr())
    only_px = torch.zeros((1080, 1920), dtype=torch.int32, device=dev)
    sc.render_dev(cam, lights, P, None, only_px.data_ptr())
    plans1 = [dist.ShardPlan(P, r, world, unit=1) for r in range(world)]
    gathered_px = torch.zeros((world, plans1[0].maxp), dtype=torch.int32, device=dev)
    for r in range(world):
        assert sc.lib.glome_render_tiles_packed_dev(sc.h, C.byref(cam), la, len(lights), C.byref(plans1[r].P_local), C.c_void_p(gathered_px[r].data_ptr()), None) == 0
    frame_px = torch.full((1080, 1920), -1, dtype=torch.int32, device=dev)
    assert sc.lib.glome_tiles_blit_all_packed_dev(gpu_ctx.h, C.byref(P), world, C.c_void_p(gathered_px.data_ptr()), plans1[0].maxp, C.c_void_p(frame_px.data_ptr())) == 0
    gpu_ctx.synchronize()
    _same(only_px, whole_px, "packed-only render vs packed of the float render")
    _same(frame_px, whole_px, "packed shards vs whole packed frame")


def test_sharded_frame_pipeline_rehearsal_on_one_gpu(gpu_ctx):
    """The N = 2 frame pipeline (dist.ShardedFrame: lanes, frame groups rendered by one launch each, packed payloads, one
    blit per frame) with both ranks living in this process on one GPU; the collective is replaced by device copies.
    Every frame that comes out equals the single-GPU render of the same view, in order.  Then the one-GPU batch path."""
    import torch
    sd = scenes.s3(64)
    cam0, lights = product_camera_lights(sd)
    dev = torch.device("cuda:0")
    P = api.render_params(width=640, height=360, maxdepth=1)
    ranks = []
    for r in range(2):
        b = api.Builder(); nm, _ = sd.replay(b)
        ctx = gpu_ctx if r == 0 else api.Context(0)
        ranks.append((ctx, ctx.commit(b, nm[sd.root])))
    # a moving camera: frame k looks from a different eye point
    pos, at, up, fov = sd.cam
    cams = [api.camera((pos[0] + 3.0 * k, pos[1] + 1.0 * k, pos[2]), at, up, fov) for k in range(7)]
    sfs = [dist.ShardedFrame(ranks[r][1], P, r, 2, dev, lanes=2, product="packed", group=3) for r in range(2)]
    assert sfs[0].G == 3 and sfs[0].n == 2
    mailbox = []

    class Done:
        def wait(self):
            return True

    def gather1(payload, gathered, async_op=False):
        mailbox.append(payload.clone())
        torch.cuda.current_stream().synchronize()
        return Done()

    def gather0(payload, gathered, async_op=False):
        gathered[0].copy_(payload)
        gathered[1].copy_(mailbox.pop(0))
        return Done()

    sfs[1].plan.gather = gather1
    sfs[0].plan.gather = gather0
    # the synchronous statistics step bench.py starts with: both ranks, one frame, ray counts add up to the frame's
    sts = [sfs[r].step(cams[0], lights, stats=True) for r in (1, 0)]
    assert sum(st["rays_primary"] for st in sts) == 640 * 360 and not mailbox
    for k in range(7):
        for r in (1, 0):
            sfs[r].step(cams[k], lights)
    for r in (1, 0):
        sfs[r].flush()
    torch.cuda.synchronize()
    assert sfs[0].pipe.done == 7 and not mailbox  # (the statistics step goes around the pipeline)

    def single(k):
        want = torch.zeros((360, 640), dtype=torch.int32, device=dev)
        ranks[0][1].render_dev(cams[k], lights, P, None, want.data_ptr())
        gpu_ctx.synchronize()
        return want

    # groups: frames 0-2 on lane 0, 3-5 on lane 1, 6 (a partial group) on lane 0 again
    for k, (lane, g) in {3: (1, 0), 4: (1, 1), 5: (1, 2), 6: (0, 0), 1: (0, 1), 2: (0, 2)}.items():
        assert torch.equal(sfs[0].frames[lane][g], single(k)), k
    assert torch.equal(sfs[0].frame, single(6))
    # one GPU, two frames per launch
    gpu_ctx.lib.glome_ctx_use_slot(gpu_ctx.h, None, 0)
    sf1 = dist.ShardedFrame(ranks[0][1], P, 0, 1, dev, lanes=2, product="packed", group=2)
    for k in range(5):
        sf1.step(cams[k], lights)
    sf1.flush()
    torch.cuda.synchronize()
    for k, (lane, g) in {2: (1, 0), 3: (1, 1), 4: (0, 0), 1: (0, 1)}.items():
        assert torch.equal(sf1.frames[lane][g], single(k)), k
    gpu_ctx.lib.glome_ctx_use_slot(gpu_ctx.h, None, 0)
    ranks[1][1].release(); ranks[0][1].release()


def test_pipeline_through_a_one_rank_rccl_group(gpu_ctx):
    """The frame pipeline with the REAL collective: a child process opens a one-rank RCCL group (backend nccl) and runs
    dist.ShardedFrame's payload -> gather -> blit path through it; every frame equals the direct render."""
    import socket
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_one_rank.py"), str(port)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "rccl one-rank pipeline ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


@pytest.mark.parametrize("name,tier", [("S4", 0), ("csg", 1)])
def test_full_size_csg_vs_oracle_tile_sample(gpu_ctx, name, tier):
    """BASELINE configs[3] at 1920x1080, maxdepth 3: S4 (CSG over primitives: the flat tier's evaluator) and the zoo's CSG
    scene (composites below composites: the generic tier's interpreter), a tile sample against the oracle."""
    sd = SCENES[name]()
    b, nm, sc = commit(gpu_ctx, sd)
    assert sc.info()["tier"] == tier
    cam, lights = product_camera_lights(sd)
    o, om, _ = oracle_for(sd)
    ref, _, rc = o.render(1920, 1080, maxdepth=3, tile_first=5, tile_stride=23, nthreads=8, want_packed=False)
    img, _, st = sc.render(cam, lights, api.render_params(width=1920, height=1080, maxdepth=3, tile_first=5, tile_stride=23), want_packed=False)
    owned = np.zeros((1080, 1920), bool)
    for x, y, w, h, _ in dist.owned_layout(api.render_params(width=1920, height=1080), 5, 23):
        owned[y:y + h, x:x + w] = True
    e = (np.abs(img[owned][:, :4] - ref[owned][:, :4]) / np.maximum(1, np.abs(ref[owned][:, :4]))).max(-1)
    parity._log("tile_sample_S4", sd, {"frac_over": float(np.mean(e > 1e-4)), "max": float(e.max())})
    assert np.mean(e > 1e-4) <= parity.PIXEL_OUTLIER_MAX
    assert st["rays_primary"] == rc["rays_primary"]
    assert abs(st["rays_shadow"] - rc["rays_shadow"]) <= rc["rays_shadow"] // 500 + 8 and abs(st["rays_secondary"] - rc["rays_secondary"]) <= rc["rays_secondary"] // 200 + 8
    sc.release()


def test_limits_lifted_in_round_3(gpu_ctx):
    """maxdepth 8 between two facing mirrors and four levels of nested Blend / AdditiveLayers (zoo.hall_of_mirrors) against the
    oracle, both render modes (until round 3: maxdepth <= 4, nesting <= 2)."""
    sd = zoo.hall_of_mirrors()
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    img, packed, st = sc.render(cam, lights, api.render_params(width=240, height=160, maxdepth=8))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 240, 160, 8)
    assert st["rays_secondary"] > st["rays_primary"] // 4  # (reflections of reflections between the walls)
    img, packed, st = sc.render(cam, lights, api.render_params(width=195, height=130, mode=1, maxdepth=6))
    parity.check_subsample_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 195, 130, 6)
    sc.release()


@pytest.mark.parametrize("gen,seed", [("composites", 14019), ("composites", 14093), ("grove", 14003), ("grove", 14010), ("grove", 14016)])
def test_packet_service_equals_the_per_lane_walk_on_fuzz_scenes(gpu_ctx, gen, seed):
    """The same bit-identity on fuzz scenes under the fuzz soak's rig (a camera inside the scene, lights of finite reach): composites 14019 is
    the scene on which the first form of bih_items_wave -- the nearest item finished by an ordinary call -- came out an ulp of the depth
    away from the per-lane walk on the GPU (the Instance frame's arithmetic and its in-place copy contract differently) and identical on
    the host build; the groves are the soak's three with the most rounding-sensitive pixels."""
    sd = zoo.random_rig(zoo.random_composites(seed) if gen == "composites" else zoo.grove(n=30 + (seed * 37) % 200, seed=seed), seed)
    cam, lights = product_camera_lights(sd)
    out = []
    for off in (False, True):
        if off:
            os.environ["GLOME_DEBUG_NO_GENERIC_PACKETS"] = "1"
        try:
            b, nm, sc = commit(gpu_ctx, sd)
        finally:
            os.environ.pop("GLOME_DEBUG_NO_GENERIC_PACKETS", None)
        assert sc.info()["tier"] == 1
        out.append([sc.render(cam, lights, api.render_params(width=192, height=108, mode=mode, maxdepth=md))[0].copy() for mode, md in ((0, 1), (0, 3), (1, 3))])
        sc.release()
    for a_, b_ in zip(*out):
        assert np.array_equal(a_, b_)


@pytest.mark.parametrize("name", ["nested", "instanced_terrain", "testscene", "grove"])
def test_generic_tier_packet_service_equals_the_per_lane_walk(gpu_ctx, name):
    """Sphere / triangle BIHs inside the generic tier's interpreter, and BIHs whose items are all answered in place (the oak of the default
    scene, 21 levels; zoo.grove: every kind of such item), are walked as wave-wide packets (rt_generic.hpp, vm_run's packet service,
    bih_items_wave).  Committed with GLOME_DEBUG_NO_GENERIC_PACKETS the same scene walks them lane by lane over frames: frames and ray counts must be
    bit-identical in both render modes, the work counters close."""
    sd = zoo.testscene(4) if name == "testscene" else SCENES[name]()
    cam, lights = product_camera_lights(sd)
    out = []
    for off in (False, True):
        if off:
            os.environ["GLOME_DEBUG_NO_GENERIC_PACKETS"] = "1"
        try:
            b, nm, sc = commit(gpu_ctx, sd)
        finally:
            os.environ.pop("GLOME_DEBUG_NO_GENERIC_PACKETS", None)
        assert sc.info()["tier"] == 1
        if name in ("testscene", "grove"): assert sc.info()["max_bih_depth"] <= 24  # (kGenericPacketStack: the service's stack holds these trees)
        frames = []
        for mode, w, h in ((0, 240, 160), (1, 195, 130)):
            img, packed, st = sc.render(cam, lights, api.render_params(width=w, height=h, mode=mode, maxdepth=3, count_work=1))
            frames.append((img.copy(), packed.copy(), {k: st[k] for k in ("rays_primary", "rays_shadow", "rays_secondary", "bih_nodes", "mesh_nodes", "prim_tests")}))
        out.append(frames)
        sc.release()
    for (ia, pa, sa), (ib, pb, sb_) in zip(*out):
        assert np.array_equal(ia, ib) and np.array_equal(pa, pb)
        for k in ("rays_primary", "rays_shadow", "rays_secondary", "mesh_nodes"):
            assert sa[k] == sb_[k], (k, sa, sb_)
        # (work counters: the interpreter's own walk re-tests a popped node against the best hit so far before it counts it, the packet
        # walk counts as rayint_debug does, and a lane that is not in a packet's mask tests no item: a few per cent apart, same hits)
        for k in ("bih_nodes", "prim_tests"):
            assert abs(sa[k] - sb_[k]) <= 0.05 * max(sa[k], sb_[k]), (k, sa, sb_)


@pytest.mark.parametrize("extra", [0, 300])
def test_texture_stacks_of_eight(gpu_ctx, extra):
    """zoo.veils: eight Tex levels (8-bit ids) above a sphere, a Difference, BIH items and a mesh triangle, and four levels in a
    table of more than 254 materials (16-bit ids), against the oracle; a level more than the stack holds is refused at commit."""
    sd = zoo.veils(extra)
    b, nm, sc = commit(gpu_ctx, sd)
    parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, sd, nm, n=20000)
    ro, rd = random_rays(20000, 11, center=(0, 1.5, 0), radius=13, spread=7)
    assert (sc.rayint(ro, rd)["tex"] >= 0).sum(1).max() == (4 if extra else 8)
    cam, lights = product_camera_lights(sd)
    for mode, w, h in ((0, 320, 200), (1, 195, 130)):
        img, packed, st = sc.render(cam, lights, api.render_params(width=w, height=h, mode=mode, maxdepth=3))
        (parity.check_subsample_image if mode else parity.check_image)(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, w, h, 3)
    sc.release()
    over = sd.tex(sd.root, 0)
    b = api.Builder()
    nm, _ = sd.replay(b)
    with pytest.raises(api.GlomeError, match="nested textures"):
        gpu_ctx.commit(b, nm[over])


@pytest.mark.parametrize("name,w,h", [("S1", 720, 480), ("S3small", 131, 66), ("materials", 200, 150), ("S4", 260, 195), ("mesh", 130, 65)])
def test_adaptive_sampler_vs_oracle(gpu_ctx, name, w, h):
    """GLOME_MODE_SUBSAMPLE = renderTileSubsample (Glome.hs:226-323), incl. S1 at BASELINE configs[0..1]'s 720x480."""
    sd = SCENES[name]()
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    img, packed, st = sc.render(cam, lights, api.render_params(width=w, height=h, mode=1, maxdepth=3))
    c, rc = parity.check_subsample_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, w, h, 3)
    assert w * h / 8 <= st["rays_primary"] <= 2 * w * h
    img2, packed2, _ = sc.render(cam, lights, api.render_params(width=w, height=h, mode=1, maxdepth=3))
    assert np.array_equal(img, img2) and np.array_equal(packed, packed2)  # deterministic
    sc.release()


def test_adaptive_sampler_tile_shards_reassemble_bit_exactly(gpu_ctx):
    """The adaptive result depends on tile origin (Q21), so sharding must use whole reference tiles: 3 shards == whole."""
    import torch
    sd = scenes.s1(nlights=1)
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    dev = torch.device("cuda:0")
    P = api.render_params(width=720, height=480, mode=1, maxdepth=1)
    whole = torch.zeros((480, 720, 5), dtype=torch.float32, device=dev)
    sc.render_dev(cam, lights, P, whole.data_ptr())
    frame = torch.full((480, 720, 5), float("nan"), dtype=torch.float32, device=dev)
    la = (L.Light * len(lights))(*lights)
    for r in range(3):
        plan = dist.ShardPlan(P, r, 3)
        payload = torch.zeros(plan.maxp, dtype=torch.float32, device=dev)
        assert sc.lib.glome_render_tiles_dev(sc.h, C.byref(cam), la, len(lights), C.byref(plan.P_local), C.c_void_p(payload.data_ptr()), None) == 0
        assert sc.lib.glome_tiles_blit_dev(gpu_ctx.h, C.byref(plan.P), r, 3, C.c_void_p(payload.data_ptr()), C.c_void_p(frame.data_ptr()), None) == 0
        gpu_ctx.synchronize()  # the context runs on its own stream: finish before torch recycles `payload`
    assert torch.equal(frame, whole)
    # the packed-pixel product in adaptive mode (what `bench.py --mode 1` gathers at N > 1): whole frame and 3 shards
    whole_px = torch.zeros((480, 720), dtype=torch.int32, device=dev)
    sc.render_dev(cam, lights, P, whole.data_ptr(), whole_px.data_ptr())
    only_px = torch.zeros((480, 720), dtype=torch.int32, device=dev)
    sc.render_dev(cam, lights, P, None, only_px.data_ptr())
    plans1 = [dist.ShardPlan(P, r, 3, unit=1) for r in range(3)]
    gathered = torch.zeros((3, plans1[0].maxp), dtype=torch.int32, device=dev)
    for r in range(3):
        assert sc.lib.glome_render_tiles_packed_dev(sc.h, C.byref(cam), la, len(lights), C.byref(plans1[r].P_local), C.c_void_p(gathered[r].data_ptr()), None) == 0
    frame_px = torch.full((480, 720), -1, dtype=torch.int32, device=dev)
    assert sc.lib.glome_tiles_blit_all_packed_dev(gpu_ctx.h, C.byref(P), 3, C.c_void_p(gathered.data_ptr()), plans1[0].maxp, C.c_void_p(frame_px.data_ptr())) == 0
    gpu_ctx.synchronize()
    assert torch.equal(only_px, whole_px) and torch.equal(frame_px, whole_px)
    sc.release()


# ------------------------------------------------------------------ edge cases
def test_edge_cases(gpu_ctx):
    b = api.Builder()
    m = b.material_surface((1, 1, 1), 1, 0.2, 0.8, 0, 0)
    void = b.group([])
    sc = gpu_ctx.commit(b, void)  # empty scene: everything misses
    cam = api.camera((0, 0, -5), (0, 0, 0), (0, 1, 0), 45)
    img, packed, st = sc.render(cam, [api.light((0, 5, 0), (10, 10, 10))], api.render_params(width=7, height=5, maxdepth=3))
    assert np.all(img[..., :4] == 0) and np.all(img[..., 4] == 1e6) and np.all(packed == 0) and st["rays_shadow"] == 0
    assert sc.rayint(np.zeros((0, 3)), np.zeros((0, 3)))["t"].shape == (0,)  # zero rays
    r = sc.rayint([[0, 0, -3]], [[0, 0, 1]])
    assert r["t"][0] == -1 and r["prim"][0] == -1 and np.all(r["tex"][0] == -1)
    sc.release()
    sph = b.sphere((0, 0, 0), 1)
    s = b.tex(sph, m)
    sc = gpu_ctx.commit(b, s)
    for n in (1, 63, 64, 65, 1000):  # ragged batch sizes
        o = np.tile([[0, 0, -3]], (n, 1)); d = np.tile([[0, 0, 1]], (n, 1))
        r = sc.rayint(o, d)
        assert np.allclose(r["t"], 2) and np.all(r["prim"] == sph) and np.all(r["tex"][:, 0] == m) and np.all(r["tex"][:, 1] == -1)
        assert sc.shadow(o, d, 5.0).all() and not sc.shadow(o, d, 1.5).any()
    assert np.array_equal(sc.rayint([[0, 0, -3]], [[0, 0, 1]], 1.5)["t"], [-1])  # beyond tmax (D4)
    for (w, h) in [(1, 1), (7, 5), (65, 65), (66, 131), (130, 64)]:  # frames that are not multiples of 8 or 65
        img, _, st = sc.render(cam, [], api.render_params(width=w, height=h, maxdepth=1), want_packed=False)
        assert st["rays_primary"] == w * h == st["n_pixels"] and np.isfinite(img).all()
    with pytest.raises(api.GlomeError):
        sc.render(cam, [], api.render_params(width=16, height=16, maxdepth=0))
    with pytest.raises(api.GlomeError):
        sc.render(cam, [api.light((0, 1, 0), (1, 1, 1))] * 17, api.render_params(width=16, height=16))
    with pytest.raises(api.GlomeError):
        sc.render(cam, [], api.render_params(width=16, height=16, mode=7))
    for (w, h) in [(1, 1), (7, 5), (65, 65), (66, 131)]:  # adaptive mode on tiny / ragged frames
        img, _, st = sc.render(cam, [], api.render_params(width=w, height=h, mode=1, maxdepth=1), want_packed=False)
        assert np.isfinite(img).all() and st["n_pixels"] == w * h
    sc.release()
    n = b.sphere((0, 0, 0), 1)
    for _ in range(8):
        n = b.group([b.transform(n, [api.translate((0.1, 0, 0))]), b.sphere((9, 9, 9), 0.1)])
    gpu_ctx.commit(b, b.difference(n, b.sphere((0.5, 0, 0), 0.7))).release()  # seventeen composite levels: fine (zoo.deep_nest is rendered by the parity tests)
    for _ in range(60):  # (2,048 frame words since round 4: a group and the Instance inside it take 34)
        n = b.group([b.transform(n, [api.translate((0.1, 0, 0))]), b.sphere((9, 9, 9), 0.1)])
    with pytest.raises(api.GlomeError, match="frame memory"):  # what bounds the nesting: the interpreter's frame words, estimated at commit
        gpu_ctx.commit(b, n)


@pytest.mark.parametrize("seed", [5069, 5059, 3199])
def test_gpu_equals_the_host_build_where_boxes_end_on_split_planes(gpu_ctx, seed):
    """The library against the HOST BUILD of the same device headers (tests/hostsim) on fuzz scenes whose boxes end exactly on
    their leaf's split plane or their tree's bounds: `shadow` of a Box asks `far > d` (Box.hs:56-62), so the leaf's interval
    and the box's slab must be clipped with bit-identical reciprocals (rt_device.hpp dir_rcp).  Before that, the compiler's
    mixed lowering of `1.0f / x` made 99-118 pixels of these frames a whole light too bright and 1 shadow ray in 10,000 miss."""
    from helpers import HostSim, random_rays
    sd = zoo.random_rig(zoo.random_composites(seed), seed)
    b, nm, sc = commit(gpu_ctx, sd)
    hs = HostSim(b, nm[sd.root])
    cam, lights = product_camera_lights(sd)
    img, _, st = sc.render(cam, lights, api.render_params(width=192, height=108, maxdepth=3), want_packed=False)
    him, cnt = hs.render(cam, lights, 192, 108, 3)
    e = (np.abs(img[..., :4] - him[..., :4]) / np.maximum(1, np.abs(him[..., :4]))).max(-1)
    assert int((e > 1e-4).sum()) <= 16, int((e > 1e-4).sum())  # measured 0 / 1 / <= 10: fp32 contraction at silhouettes
    ro, rd = random_rays(100000, seed)
    assert np.array_equal(sc.shadow(ro, rd, 30.0), hs.shadow(ro, rd, 30.0))
    assert np.array_equal(sc.inside(ro), hs.inside(ro))
    sc.release()


def test_gpu_equals_the_host_build_on_a_sweep_of_fuzz_scenes(gpu_ctx):
    """The same comparison over 24 more fuzz scenes of both generators (the three above are the ones a soak once flagged): the
    host build never runs the ballots, the scalar loads or the hand-written walk, and divides exactly where the device takes
    v_rcp_f32 -- so this is where a difference in LOGIC between the two builds of the same headers would show.  Frames within a
    few silhouette pixels, shadow and inside answers equal but for the odd ray an ulp from a surface (tools/probe/
    gpu_vs_hostsim_sweep.py: two shadow rays of 12 million)."""
    from helpers import HostSim, random_rays
    odd = 0
    for seed in range(100, 124):
        sd = zoo.random_rig(zoo.random_composites(seed) if seed % 2 else zoo.random_flat(seed), seed)
        try:
            b, nm, sc = commit(gpu_ctx, sd)
        except api.GlomeError as e:  # (a generator may stack five textures: refused at commit)
            assert "nested textures" in str(e), e
            continue
        hs = HostSim(b, nm[sd.root])
        cam, lights = product_camera_lights(sd)
        img, _, st = sc.render(cam, lights, api.render_params(width=128, height=72, maxdepth=3), want_packed=False)
        him, cnt = hs.render(cam, lights, 128, 72, 3)
        e = (np.abs(img[..., :4] - him[..., :4]) / np.maximum(1, np.abs(him[..., :4]))).max(-1)
        assert int((e > 1e-4).sum()) <= 24, (seed, int((e > 1e-4).sum()))
        ro, rd = random_rays(20000, seed)
        ds = int((sc.shadow(ro, rd, 30.0) != hs.shadow(ro, rd, 30.0)).sum()) + int((sc.inside(ro) != hs.inside(ro)).sum())
        assert ds <= 1, (seed, ds)
        odd += ds
        sc.release()
    assert odd <= 3, odd


def test_device_pointer_seams_match_host_seams(gpu_ctx):
    import torch
    sd = scenes.s1(nlights=1)
    b, nm, sc = commit(gpu_ctx, sd)
    ro, rd = random_rays(10000, 5)
    host = sc.rayint(ro, rd)
    dev = torch.device("cuda:0")
    cols = [torch.tensor(np.ascontiguousarray(a), device=dev) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2], np.full(len(ro), 1e6, np.float32))]
    t = torch.zeros(len(ro), dtype=torch.float32, device=dev)
    prim = torch.zeros(len(ro), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = sc.lib.glome_rayint_batch_dev(sc.h, len(ro), *[C.c_void_p(c.data_ptr()) for c in cols], C.c_void_p(t.data_ptr()), C.c_void_p(prim.data_ptr()), None, None, None, None)
    assert rc == 0
    occ = torch.zeros(len(ro), dtype=torch.uint8, device=dev)
    assert sc.lib.glome_shadow_batch_dev(sc.h, len(ro), *[C.c_void_p(c.data_ptr()) for c in cols], C.c_void_p(occ.data_ptr())) == 0
    gpu_ctx.synchronize()
    assert np.array_equal(t.cpu().numpy(), host["t"]) and np.array_equal(prim.cpu().numpy(), host["prim"])
    assert np.array_equal(occ.cpu().numpy().astype(bool), sc.shadow(ro, rd, 1e6))
    sc.release()


@pytest.mark.gpu
def test_nff_scene_renders_like_the_oracle(gpu_ctx):
    """N2: a scene loaded by glome_sb_load_nff (spheres, cones, polygon fans, three lights) against the oracle fed by the
    independent Python reading of the same text."""
    import nff
    text = nff.balls_nff(3)
    b = api.Builder()
    root, cam_desc, light_descs, bg = b.load_nff(text)
    sc = gpu_ctx.commit(b, root)
    sd, _ = nff.read_nff(text)
    cam, lights = product_camera_lights(sd)
    img, packed, st = sc.render(cam, lights, api.render_params(width=256, height=256, maxdepth=2))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 256, 256, 2)
    sc.release()


def _same_tree(b, a_node, d_node):
    da, dd = b.bih_dump(a_node), b.bih_dump(d_node)
    for k in range(5):  # split planes, axes, leaf sizes, leaf items in order: bit for bit
        assert np.array_equal(da[k], dd[k]), k
    assert np.array_equal(b.bound(a_node), b.bound(d_node))


@pytest.mark.parametrize("kind", ["spheres", "mixed", "duplicates", "tiny"])
def test_device_built_bih_is_the_host_builders_tree(gpu_ctx, kind):
    """N4: glome_sb_bih_dev (four kernels per tree level) against glome_sb_bih (the recursion of Bih.hs:211-285): same
    candidates, same costs, same comparison chain, same stable partitions -- the same tree, leaf order included."""
    rng = np.random.default_rng(17)
    b = api.Builder()
    if kind == "spheres":
        ids = [b.sphere(tuple(rng.uniform(-30, 30, size=3)), float(rng.uniform(0.1, 4))) for _ in range(3000)]
    elif kind == "mixed":  # big and small objects (the fourth candidate: area > 0.4 of the node's), boxes, triangles
        ids = [b.sphere(tuple(rng.uniform(-10, 10, size=3)), float(rng.uniform(0.05, 0.5))) for _ in range(800)]
        ids += [b.box(tuple(rng.uniform(-10, 0, size=3)), tuple(rng.uniform(0, 10, size=3))) for _ in range(6)]
        ids += [b.triangle(*[tuple(rng.uniform(-10, 10, size=3)) for _ in range(3)]) for _ in range(700)]
        ids = [ids[i] for i in rng.permutation(len(ids))]
    elif kind == "duplicates":  # identical boxes: partitions that do not separate, ties everywhere, empty leaves
        ids = [b.sphere((float(i % 5), 0.0, float(i % 3)), 1.0) for i in range(600)]
    else:
        ids = [b.sphere((float(i), 0.0, 0.0), 0.4) for i in range(3)]
    host = b.bih(ids)
    dev, ms = gpu_ctx.bih(b, ids)
    _same_tree(b, host, dev)
    if kind != "tiny":
        assert ms > 0


def test_device_built_bih_of_the_flagship_terrain(gpu_ctx):
    """100,352 triangles (S3's heightfield): the device build gives the host builder's tree and the frame it renders."""
    import time
    sd = scenes.s3(224)
    b = api.Builder()
    nm, _ = sd.replay(b)
    nid, host, ids = 0, None, None  # SceneDesc node ids run over the node ops in order (a bulk op makes many)
    for kind, name, args in sd.ops:
        if kind == "N":
            nid += args[0].shape[0]
        elif kind == "n":
            if name == "bih":
                host, ids = nm[nid], [nm[i] for i in args[0]]
            nid += 1
    assert host is not None and len(ids) == 100352
    t0 = time.perf_counter()
    dev, ms = gpu_ctx.bih(b, ids)
    wall = time.perf_counter() - t0
    _same_tree(b, host, dev)
    print(f"device bih of {len(ids)} triangles: {ms:.2f} ms on the GPU, {wall * 1e3:.0f} ms wall incl. bounds, upload and tree read-back")


@pytest.mark.parametrize("n", [12, 96])
def test_device_built_mesh_bvh_is_the_host_builders_tree(gpu_ctx, n):
    """N4: glome_sb_mesh_dev against glome_sb_mesh (build_tree, Mesh.hs:69-113): the `show` text spells out every box of
    the BVH and every leaf's triangle list -- identical -- and so is the rendered frame."""
    V = scenes.heightfield_vertices(n).reshape(-1, 3) * np.array([0.5, 1.0, 0.5])
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b_, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]
    tri = np.stack([np.stack([a, b_, c], -1), np.stack([c, b_, d], -1)], axis=2).reshape(-1, 3)
    T = np.full((len(tri), 8), -1, np.int32)
    T[:, :3] = tri
    b = api.Builder()
    host = b.mesh(V, np.zeros((0, 3)), T, [])
    dev, ms = gpu_ctx.mesh(b, V, np.zeros((0, 3)), T, [])
    assert b.show(host) == b.show(dev) and ms > 0
    assert b.primcount(host) == b.primcount(dev) and np.array_equal(b.bound(host), b.bound(dev))


@pytest.mark.parametrize("name", ["csg", "materials", "soup"])
def test_scene_read_back_from_show_text_renders_the_same_frame(gpu_ctx, name):
    """N4: a scene written as `show geom` text and read back (trees as printed, materials from the side list) is the same
    scene on the device: the frame is bit-identical, generic and flat tiers."""
    sd = zoo.soup(2500, 5) if name == "soup" else getattr(zoo, name)()
    b, nm, sc = commit(gpu_ctx, sd)
    root = nm[sd.root]
    root2, ntex = b.load_show(b.show(root), b.show_tex_materials(root))
    sc2 = gpu_ctx.commit(b, root2)
    assert sc2.info()["tier"] == sc.info()["tier"]
    cam, lights = product_camera_lights(sd)
    P = api.render_params(width=200, height=144, maxdepth=3)
    img, packed, st = sc.render(cam, lights, P)
    img2, packed2, st2 = sc2.render(cam, lights, P)
    assert np.array_equal(img, img2) and np.array_equal(packed, packed2)
    assert (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]) == (st2["rays_primary"], st2["rays_shadow"], st2["rays_secondary"])
    parity.check_image(img2, (st2["rays_primary"], st2["rays_shadow"], st2["rays_secondary"]), sd, 200, 144, 3)
    sc.release(); sc2.release()


@pytest.mark.parametrize("kind", ["tri_floor", "tri_only", "sphere_floor"])
def test_random_soup_renders_like_the_oracle(gpu_ctx, kind):
    """The packet walk on irregular trees (overlapping items, leaves of more than six, mixed entry lists)."""
    sd = zoo.soup(2500, 5, spheres=kind.startswith("sphere"), floor=kind.endswith("floor"))
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    img, packed, st = sc.render(cam, lights, api.render_params(width=320, height=200, maxdepth=1))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 320, 200, 1)
    f, _, sf = sc.render(cam, lights, api.render_params(width=320, height=200, maxdepth=1, faithful=1))
    assert np.array_equal(img, f)  # early-out packets pick the reference traversal's hits, ties included
    sc.release()


def test_render_tile_fog_term(gpu_ctx):
    """renderTile stores (r + depth/400, g, b, a, depth) (Glome.hs:174, Q20); `fog = 1` reproduces that -- a miss stores
    r = 1e6 / 400 = 2500 with alpha 0 -- and the default (fog = 0) is the get_color tuple before the term."""
    sd = scenes.s1(nlights=1)
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    o, om, _ = oracle_for(sd)
    ref, _, _ = o.render(320, 180, maxdepth=1, fog=1, want_packed=False)
    img, _, _ = sc.render(cam, lights, api.render_params(width=320, height=180, maxdepth=1, fog=1), want_packed=False)
    plain, _, _ = sc.render(cam, lights, api.render_params(width=320, height=180, maxdepth=1), want_packed=False)
    c = parity.compare_images(img, ref)
    assert c["frac_over"] <= parity.PIXEL_OUTLIER_MAX, c
    miss = img[..., 4] == 1e6
    assert miss.any() and (~miss).any() and np.all(img[..., 0][miss] == 2500.0) and np.all(img[..., 3][miss] == 0)
    assert np.array_equal(img[..., 1:], plain[..., 1:])
    # (the device divides through v_rcp_f32: within an ulp or two of the exact quotient)
    assert np.allclose(img[..., 0], plain[..., 0] + plain[..., 4] / np.float32(400), rtol=1e-6, atol=0)
    sc.release()


def test_two_row_packet_kernel_over_a_one_leaf_bih(gpu_ctx):
    """A deep triangle BIH (LDS stack at its 12 entries: the frame runs on the two-row, 24-wave packet instance) next to a
    BIH whose root is a leaf of nine coincident triangles: the one-leaf tree is tested item by item without a push
    (a continuation entry would land on a stack row the two-row instance does not have)."""
    sd = zoo.deep_and_clump()
    b, nm, sc = commit(gpu_ctx, sd)
    assert sc.info()["tier"] == 0 and sc.info()["max_bih_depth"] >= 12
    cam, lights = product_camera_lights(sd)
    img, packed, st = sc.render(cam, lights, api.render_params(width=480, height=270, maxdepth=1))
    f, pf, sf = sc.render(cam, lights, api.render_params(width=480, height=270, maxdepth=1, faithful=1))  # three-row counting instance
    assert np.array_equal(img, f) and np.array_equal(packed, pf)
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 480, 270, 1)
    # the batch path bench.py uses (several frames per launch, packed product)
    import torch
    dev = torch.device("cuda:0")
    P = api.render_params(width=480, height=270, maxdepth=1)
    px = torch.zeros((2, 270, 480), dtype=torch.int32, device=dev)
    cams = (L.Camera * 2)(cam, cam)
    la = (L.Light * len(lights))(*lights)
    assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, 2, la, len(lights), C.byref(P), C.c_void_p(px.data_ptr()), 270 * 480, None) == 0
    gpu_ctx.synchronize()
    got = px.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[0], packed) and np.array_equal(got[1], packed)
    sc.release()


def test_reference_default_scene_with_the_full_lattice(gpu_ctx):
    """GlomeView's default scene (TestScene.hs:183-197 `geom''`, zoo.testscene) at the reference's own sizes -- the lattice of
    21^3 = 9261 spheres under its bih, hollowed out by the sphere of radius 32 the camera stands inside -- against the oracle,
    in renderTile and in renderTileSubsample mode, maxdepth 3 as GlomeView traces it."""
    sd = zoo.testscene(10)
    b, nm, sc = commit(gpu_ctx, sd)
    info = sc.info()
    assert info["tier"] == 1 and info["n_spheres"] >= 9261  # (a Warp material and composites below composites: the interpreter)
    cam, lights = product_camera_lights(sd)
    img, packed, st = sc.render(cam, lights, api.render_params(width=400, height=300, maxdepth=3))
    parity.check_image(img, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 400, 300, 3)
    sub, _, st = sc.render(cam, lights, api.render_params(width=260, height=195, maxdepth=3, mode=1))
    parity.check_subsample_image(sub, (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), sd, 260, 195, 3)
    sc.release()


@pytest.mark.parametrize("nframes,which", [(3, "S3"), (8, "S3"), (16, "S3"), (3, "testscene"), (12, "testscene")])
def test_adaptive_sampler_frame_batches_equal_the_frames_rendered_alone(gpu_ctx, nframes, which):
    """renderTileSubsample over several views in ONE launch (glome_render_packed_batch_dev, mode 1): the sampler then works in
    larger regions per work item (3 frames: medium, 8: a whole tile per pass) -- other packets, the same pixels.  Every frame
    of the batch must equal the frame rendered alone, bit for bit; the frame size leaves clipped tiles on two edges."""
    import torch
    sd = scenes.s3(48) if which == "S3" else zoo.testscene(2)  # (the flat tier's sampler kernel / the generic tier's, with secondary rays)
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    W, H = (531, 397) if which == "S3" else (267, 199)
    P = api.render_params(width=W, height=H, maxdepth=1 if which == "S3" else 3, mode=1)
    views = []
    for f in range(nframes):  # the scene's camera, then the eye moved sideways and up a little
        pos, at, up, angle = sd.cam
        views.append(api.camera([pos[0] + 0.4 * f, pos[1] + 0.1 * f, pos[2]], at, up, angle))
    alone = [sc.render(v, lights, P)[1] for v in views]
    assert any(not np.array_equal(alone[0], a) for a in alone[1:])
    px = torch.zeros((nframes, H, W), dtype=torch.int32, device=torch.device("cuda:0"))
    cams = (L.Camera * nframes)(*views)
    la = (L.Light * len(lights))(*lights)
    for rep in range(2):
        assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, nframes, la, len(lights), C.byref(P), C.c_void_p(px.data_ptr()), H * W, None) == 0, gpu_ctx.err()
        gpu_ctx.synchronize()
        got = px.cpu().numpy().view(np.uint32)
        for f in range(nframes):
            assert np.array_equal(got[f], alone[f]), (rep, f)
        px.zero_()
    sc.release()


# ------------------------------------------------------------------ BASELINE configs[4]: 1M triangles, 3840x2160, adaptive, shards
def _bih_op(sd, nm):
    """(host node, item ids) of the scene's `bih` call: SceneDesc node ids run over the node ops in order (a bulk op makes many)"""
    nid, out = 0, None
    for kind, name, args in sd.ops:
        if kind == "N":
            nid += args[0].shape[0]
        elif kind == "n":
            if name == "bih":
                out = (nm[nid], [nm[i] for i in args[0]])
            nid += 1
    return out


def _owned_mask(w, h, first, stride):
    owned = np.zeros((h, w), bool)
    for x, y, tw, th, _ in dist.owned_layout(api.render_params(width=w, height=h), first, stride):
        owned[y:y + th, x:x + tw] = True
    return owned


@pytest.fixture(scope="module")
def s5_bih(gpu_ctx):
    """S5 = heightfield of 708 x 708 x 2 = 1,002,528 triangles as `bih [triangle ...]`, tree built on the device."""
    sd = scenes.s3(708)
    b = api.Builder()

    class DevBih:
        def __getattr__(self, name):
            return getattr(b, name)

        def bih(self, ids):
            return gpu_ctx.bih(b, ids)[0]
    nm, _ = sd.replay(DevBih())
    sc = gpu_ctx.commit(b, nm[sd.root])
    o, om, _ = oracle_for(sd)  # ~15 s for a million triangles: once per module
    yield sd, sc, o
    sc.release()


def test_s5_device_built_tree_of_a_million_triangles_is_the_host_builders(gpu_ctx):
    sd = scenes.s3(708)
    b = api.Builder()
    nm, _ = sd.replay(b)  # host builder (build_rec, Bih.hs:211-285)
    host, ids = _bih_op(sd, nm)
    assert len(ids) == 1002528
    dev, ms = gpu_ctx.bih(b, ids)
    _same_tree(b, host, dev)
    assert ms > 0


def _whole_frame_check(tag, sd, sc, o, W, H, maxdepth):
    """The PRODUCTION kernels' whole frame against the oracle's whole frame (16 host threads): every pixel, by the absolute metric
    the tile samples use and by the true relative one (|got - ref| / max(|ref|, 1e-3)); gates = measured level x margin
    (profiles/r03_parity_levels.txt)."""
    cam, lights = product_camera_lights(sd)
    ref, _, rc = o.render(W, H, maxdepth=maxdepth, nthreads=16, want_packed=False)
    img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=maxdepth), want_packed=False)
    c = compare_images(img, ref)
    hit_g, hit_r = img[..., 4] < 1e6, ref[..., 4] < 1e6
    c["hit_flip"] = float(np.mean(hit_g != hit_r))
    parity._log("whole_frame_" + tag, sd, c)
    assert st["rays_primary"] == rc["rays_primary"] == W * H
    assert abs(st["rays_shadow"] - rc["rays_shadow"]) <= rc["rays_shadow"] // 2000 + 8, (st, rc)
    assert abs(st["rays_secondary"] - rc["rays_secondary"]) <= rc["rays_secondary"] // 200 + 8, (st, rc)
    assert c["frac_over"] <= parity.PIXEL_OUTLIER_MAX, c          # beyond 1e-4 of max(1, |ref|)
    assert c["rel_frac_over"] <= parity.REL_PIXEL_OUTLIER_MAX, c  # beyond 1e-4 of max(|ref|, 1e-3)
    assert c["hit_flip"] <= 1e-4, c
    return c


def test_whole_frame_s3_1080p_vs_oracle(s3_full):
    sd, sc = s3_full
    o, om, _ = oracle_for(sd)
    _whole_frame_check("S3", sd, sc, o, 1920, 1080, 1)


def test_whole_frame_s4_1080p_vs_oracle(gpu_ctx):
    sd = scenes.s4()
    b, nm, sc = commit(gpu_ctx, sd)
    o, om, _ = oracle_for(sd)
    _whole_frame_check("S4", sd, sc, o, 1920, 1080, 3)
    sc.release()


def test_whole_frame_s5_4k_vs_oracle(s5_bih):
    sd, sc, o = s5_bih
    _whole_frame_check("S5", sd, sc, o, 3840, 2160, 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_s5_4k_tile_sample_vs_oracle(s5_bih, mode):
    """Every 173rd 65x65 tile of the 3840x2160 frame (12 tiles, ~48k pixels) by the oracle and by the GPU, in renderTile mode
    (faithful traversal: ray and node / primitive visit counts equal the oracle's) and in renderTileSubsample mode (whole
    reference tiles, so the sampled tiles are exactly the frame's)."""
    sd, sc, o = s5_bih
    cam, lights = product_camera_lights(sd)
    W, H, first, stride = 3840, 2160, 7, 173
    ref, _, rc = o.render(W, H, mode=mode, maxdepth=1, tile_first=first, tile_stride=stride, nthreads=8, want_packed=False)
    init = np.zeros((H, W, 5), np.float32)
    img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, mode=mode, maxdepth=1, tile_first=first, tile_stride=stride, faithful=1 if mode == 0 else 0),
                           want_packed=False, init=init)
    owned = _owned_mask(W, H, first, stride)
    assert owned.sum() == st["n_pixels"] and np.all(img[~owned] == 0)
    e = (np.abs(img[owned][:, :4] - ref[owned][:, :4]) / np.maximum(1, np.abs(ref[owned][:, :4]))).max(-1)
    parity._log(f"tile_sample_S5_mode{mode}", sd, {"frac_over": float(np.mean(e > 1e-4)), "max": float(e.max())})
    if mode == 0:
        assert np.mean(e > 1e-4) <= parity.PIXEL_OUTLIER_MAX, np.mean(e > 1e-4)
        assert st["rays_primary"] == rc["rays_primary"] == owned.sum() and st["rays_shadow"] == rc["rays_shadow"]
        assert abs(st["bih_nodes"] - rc["bih_nodes"]) <= rc["bih_nodes"] // 5000 + 4
        assert abs(st["prim_tests"] - rc["prim_tests"]) <= rc["prim_tests"] // 5000 + 4
    else:
        assert np.mean(e > 1e-4) <= parity.SUBSAMPLE_OUTLIER_MAX, np.mean(e > 1e-4)
        assert abs(int(st["rays_primary"]) - rc["rays_primary"]) <= max(8, rc["rays_primary"] // 500)
        assert owned.sum() / 8 <= st["rays_primary"] <= 2 * owned.sum()


def test_s5_4k_adaptive_eight_shards_reassemble_bit_exactly(gpu_ctx, s5_bih):
    """configs[4] as stated: 3840x2160, renderTileSubsample, whole 65x65 reference tiles round-robin over 8 ranks -- each
    rank's packed payload, one blit: the packed framebuffer of the single-GPU render, bit for bit."""
    import torch
    sd, sc, _ = s5_bih
    cam, lights = product_camera_lights(sd)
    dev = torch.device("cuda:0")
    W, H, world = 3840, 2160, 8
    P = api.render_params(width=W, height=H, mode=1, maxdepth=1)
    whole_px = torch.zeros((H, W), dtype=torch.int32, device=dev)
    sc.render_dev(cam, lights, P, None, whole_px.data_ptr())
    la = (L.Light * len(lights))(*lights)
    plans = [dist.ShardPlan(P, r, world, unit=1) for r in range(world)]
    gathered = torch.zeros((world, plans[0].maxp), dtype=torch.int32, device=dev)
    tot = 0
    for r in range(world):
        st = L.Stats()
        assert sc.lib.glome_render_tiles_packed_dev(sc.h, C.byref(cam), la, len(lights), C.byref(plans[r].P_local), C.c_void_p(gathered[r].data_ptr()), C.byref(st)) == 0
        tot += st.n_pixels
    frame_px = torch.full((H, W), -1, dtype=torch.int32, device=dev)
    assert sc.lib.glome_tiles_blit_all_packed_dev(gpu_ctx.h, C.byref(P), world, C.c_void_p(gathered.data_ptr()), plans[0].maxp, C.c_void_p(frame_px.data_ptr())) == 0
    gpu_ctx.synchronize()
    assert tot == W * H and torch.equal(frame_px, whole_px)


@pytest.fixture(scope="module")
def s5_mesh(gpu_ctx):
    sd = scenes.s3(708, as_mesh=True)
    b = api.Builder()

    class DevMesh:
        def __getattr__(self, name):
            return getattr(b, name)

        def mesh(self, verts, norms, tris, mats):
            return gpu_ctx.mesh(b, verts, norms, tris, mats)[0]
    nm, _ = sd.replay(DevMesh())
    sc = gpu_ctx.commit(b, nm[sd.root])
    o, om, _ = oracle_for(sd)
    yield sd, sc, o
    sc.release()


def test_mesh_packet_walk_equals_the_per_lane_walk(gpu_ctx, s5_mesh):
    """rayint_mesh for a wave's 64 rays at once (rt_device.hpp mesh_closest_wave: a node's children in up to three passes so that
    every lane keeps its own `lnear < rnear` order, Mesh.hs:178) against the per-lane walk (the faithful instance): the same
    frame bit for bit -- the 100k-triangle mesh at 1080p, the 1M-triangle mesh at 4K, and a small mesh seen from inside its
    bounds with a camera on an axis (lanes that want opposite orders)."""
    cases = [(scenes.s3(224, as_mesh=True), None, 1920, 1080), (None, s5_mesh, 3840, 2160), (scenes.s3(12, as_mesh=True), None, 333, 222)]
    for sd, fix, W, H in cases:
        if fix is not None:
            sd, sc = fix[0], fix[1]
        else:
            b, nm, sc = commit(gpu_ctx, sd)
        cam, lights = product_camera_lights(sd)
        if W == 333:
            cam = api.camera((0.0, 0.4, 0.0), (0.0, 0.0, 5.0), (0, 1, 0), 80)  # inside the height field's box, looking along +z
        a, pa, sa = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=1))
        f, pf, sf = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=1, faithful=1))
        assert np.array_equal(pa, pf) and np.array_equal(a, f), (W, int((pa != pf).sum()))
        assert (sa["rays_primary"], sa["rays_shadow"]) == (sf["rays_primary"], sf["rays_shadow"])
        if fix is None:
            sc.release()


@pytest.mark.parametrize("mode", [0, 1])
def test_s5_as_a_mesh_of_a_million_triangles_4k_tile_sample_vs_oracle(s5_mesh, mode):
    """configs[4] names a Mesh: the same 1,002,528 triangles as `mesh verts [] tris` (rayint_mesh, Mesh.hs:136-198; the BVH of
    build_tree, Mesh.hs:69-113, made on the device), 3840x2160, a tile sample against the oracle in both render modes.  A
    Mesh casts no shadows (Mesh.hs:210), so shadow rays are traced and all come back unoccluded."""
    sd, sc, o = s5_mesh
    assert sc.info()["n_triangles"] == 1002528 and sc.info()["n_mesh_nodes"] > 0
    cam, lights = product_camera_lights(sd)
    W, H, first, stride = 3840, 2160, 11, 173
    ref, _, rc = o.render(W, H, mode=mode, maxdepth=1, tile_first=first, tile_stride=stride, nthreads=8, want_packed=False)
    img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, mode=mode, maxdepth=1, tile_first=first, tile_stride=stride, count_work=1 if mode == 0 else 0),
                           want_packed=False, init=np.zeros((H, W, 5), np.float32))
    owned = _owned_mask(W, H, first, stride)
    e = (np.abs(img[owned][:, :4] - ref[owned][:, :4]) / np.maximum(1, np.abs(ref[owned][:, :4]))).max(-1)
    parity._log(f"tile_sample_S5mesh_mode{mode}", sd, {"frac_over": float(np.mean(e > 1e-4)), "max": float(e.max())})
    assert np.mean(e > 1e-4) <= (parity.PIXEL_OUTLIER_MAX if mode == 0 else parity.SUBSAMPLE_OUTLIER_MAX), np.mean(e > 1e-4)
    if mode == 0:
        assert st["rays_primary"] == rc["rays_primary"] == owned.sum() and st["rays_shadow"] == rc["rays_shadow"]
        # the device walk re-tests a postponed child against the best hit of the whole mesh so far, which is at most the depth
        # the reference clips with (Mesh.hs:178, 190: the first child's result): same hits, a few per cent fewer nodes
        assert 0.95 * rc["mesh_nodes"] <= st["mesh_nodes"] <= rc["mesh_nodes"] + 4, (st["mesh_nodes"], rc["mesh_nodes"])
    else:
        assert abs(int(st["rays_primary"]) - rc["rays_primary"]) <= max(8, rc["rays_primary"] // 500)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_multi_gpu_c_abi_frames_equal_the_single_gpu_frames(gpu_ctx, n):
    """glome_multi_* (SURVEY.md Appendix B's glome_render_multi: the Haskell host's way to several GPUs): n ranks -- here n
    contexts on the one GPU of the box, so the payloads move by peer copy; on distinct devices the same calls go through
    RCCL send / recv -- render their tile shards of a batch of views, rank 0 gathers and blits: every frame equals the
    single-context render bit for bit, in renderTile mode (a batch of three moving views) and in adaptive mode."""
    import torch
    sd = scenes.s3(48)
    dev = torch.device("cuda:0")
    ctxs = [gpu_ctx] + [api.Context(0) for _ in range(n - 1)]
    scs = []
    for c in ctxs:
        b = api.Builder(); nm, _ = sd.replay(b)
        scs.append(c.commit(b, nm[sd.root]))
    pos, at, up, fov = sd.cam
    cams = [api.camera((pos[0] + 2.0 * k, pos[1] + 0.5 * k, pos[2]), at, up, fov) for k in range(3)]
    _, lights = product_camera_lights(sd)
    W, H = 645, 390
    for transport in (None, "direct"):  # the payload / exchange / blit path, and (round 4) every rank storing straight into the frame
      for mode, views in ((0, cams), (1, cams[:1])):
        P = api.render_params(width=W, height=H, mode=mode, maxdepth=1, rank0_share_pct=65 if n == 3 else 0)  # (three ranks: rank 0 with less than a fair share)
        m = api.Multi(scs, P, transport=transport)
        assert m.transport() == ("none" if n == 1 else (transport or "peer-copy"))
        out = torch.full((len(views), H, W), -1, dtype=torch.int32, device=dev)
        for rep in range(2):  # a second call reuses the payload buffers: the first call's copies must have drained
            m.render(views, lights, out.data_ptr())
        m.synchronize()
        for k, cam in enumerate(views):
            want = torch.zeros((H, W), dtype=torch.int32, device=dev)
            scs[0].render_dev(cam, lights, P, None, want.data_ptr())
            gpu_ctx.synchronize()
            assert torch.equal(out[k], want), (mode, transport, k)
        m.close()
    # the one-call host-buffer form
    P = api.render_params(width=W, height=H, maxdepth=1)
    host = np.zeros((H, W), np.uint32)
    arr = (C.c_void_p * n)(*[s.h for s in scs])
    la = (L.Light * len(lights))(*lights)
    assert gpu_ctx.lib.glome_render_multi(arr, n, C.byref(cams[0]), la, len(lights), C.byref(P), host.ctypes.data_as(L.c_up)) == 0
    img, packed, _ = scs[0].render(cams[0], lights, P)
    assert np.array_equal(host, packed)
    for s_ in scs:
        s_.release()
    for c in ctxs[1:]:
        c.close()


@pytest.mark.gpu
def test_rccl_branch_of_the_multi_gpu_entry_with_a_stub_transport():
    """glome_multi_render's RCCL branch (one group of ncclSend / ncclRecv per call, on the ranks' own streams) needs distinct
    devices and so never ran on a one-GPU box.  Here it runs against tests/rcclstub (send / recv pairs = stream-ordered device
    copies; GLOME_DEBUG_RCCL_LIB, GLOME_DEBUG_RCCL_SAME_DEVICE): 2, 3 and 8 ranks, batches of four views and adaptive mode,
    payload buffers reused over three calls -- every frame equals the single-context render bit for bit."""
    import subprocess
    import sys
    if not os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "rcclstub", "librccl_stub.so")):
        pytest.skip("tests/rcclstub did not build")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_stub_multi.py")], capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "rccl stub transport ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


# ------------------------------------------------------------------ edge cases: empty, tiny and ragged inputs, refused parameters
def test_empty_and_tiny_inputs_through_the_c_abi(gpu_ctx):
    """An empty ray batch; a scene that is an empty group (every ray misses: transparent pixels at depth = infinity, Shader.hs:
    186-187); frames smaller than one 8x8 work item and than one tile, in both render modes, against the oracle; a shard that
    owns no tile at all (more ranks than tiles)."""
    from glome_amd.scene import SceneDesc
    sd = scenes.s1(nlights=2)
    b, nm, sc = commit(gpu_ctx, sd)
    none = sc.rayint(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert none["t"].shape == (0,) and sc.shadow(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32)).shape == (0,)
    assert sc.inside(np.zeros((0, 3), np.float32)).shape == (0,)
    cam, lights = product_camera_lights(sd)
    o, om, _ = oracle_for(sd)
    for (w, h) in ((1, 1), (7, 3), (9, 70), (66, 5)):
        for mode in (0, 1):
            img, packed, st = sc.render(cam, lights, api.render_params(width=w, height=h, maxdepth=1, mode=mode))
            ref, _, rc = o.render(w, h, maxdepth=1, mode=mode, want_packed=False)
            e = np.abs(img[..., :4] - ref[..., :4]) / np.maximum(1, np.abs(ref[..., :4]))
            assert e.max() <= 2e-4 and st["rays_primary"] == rc["rays_primary"], (w, h, mode, float(e.max()))
    # a shard with nothing to do: rank 5 of 7 on a one-tile frame
    init = np.full((40, 50, 5), 7.0, np.float32)
    img, _, st = sc.render(cam, lights, api.render_params(width=50, height=40, maxdepth=1, tile_first=5, tile_stride=7), want_packed=False, init=init)
    assert st["n_tiles"] == 0 and st["rays_primary"] == 0 and np.all(img == 7.0)
    sc.release()
    # the empty scene
    ed = SceneDesc()
    ed.set_root(ed.group([]))
    ed.add_light(*scenes.LIGHTS[0]); ed.set_camera(*scenes.CUST_CAM)
    b, nm, sc = commit(gpu_ctx, ed)
    ro, rd = random_rays(500, 3)
    r = sc.rayint(ro, rd)
    assert np.all(r["t"] == -1) and np.all(r["prim"] == -1) and not sc.shadow(ro, rd, np.full(500, 50.0, np.float32)).any() and not sc.inside(ro).any()
    cam, lights = product_camera_lights(ed)
    for mode in (0, 1):
        img, packed, st = sc.render(cam, lights, api.render_params(width=70, height=33, maxdepth=3, mode=mode))
        assert np.all(img[..., :4] == 0) and np.all(img[..., 4] == 1e6) and np.all(packed == 0) and st["rays_shadow"] == 0
    sc.release()


def test_refused_parameters_fail_with_a_status_not_a_frame(gpu_ctx):
    """Out-of-range arguments are refused with a status code and a message (include/glome_hip.h), nothing is rendered."""
    import torch
    sd = scenes.s1(nlights=1)
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    la = (L.Light * len(lights))(*lights)
    buf = torch.zeros((33, 64, 64), dtype=torch.int32, device=torch.device("cuda:0"))
    for kw in (dict(width=0), dict(height=-3), dict(maxdepth=0), dict(maxdepth=9), dict(blocksize=0), dict(tile_stride=0), dict(tile_first=-1), dict(rank0_share_pct=101)):
        P = api.render_params(**{**dict(width=64, height=64, maxdepth=1), **kw})
        rc = sc.lib.glome_render_dev(sc.h, C.byref(cam), la, len(lights), C.byref(P), None, C.c_void_p(buf.data_ptr()), None)
        assert rc in (L.E_INVALID, L.E_LIMIT) and gpu_ctx.err(), kw
    P = api.render_params(width=64, height=64, maxdepth=1)
    cams = (L.Camera * 33)(*[cam] * 33)
    assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, 33, la, len(lights), C.byref(P), C.c_void_p(buf.data_ptr()), 64 * 64, None) == L.E_LIMIT  # 1..32 frames
    assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, 2, la, len(lights), C.byref(P), C.c_void_p(buf.data_ptr()), 0, None) == L.E_INVALID   # frame stride
    too_many = (L.Light * 17)(*[lights[0]] * 17)  # (the light list holds 16)
    assert sc.lib.glome_render_dev(sc.h, C.byref(cam), too_many, 17, C.byref(P), None, C.c_void_p(buf.data_ptr()), None) in (L.E_INVALID, L.E_LIMIT)
    gpu_ctx.synchronize()
    assert int(buf.abs().sum()) == 0
    sc.release()


@pytest.mark.parametrize("gen,seed", [("composites", 0), ("composites", 4), ("composites", 7), ("composites", 23), ("composites", 36), ("composites", 56),
                                      ("flat", 3), ("flat", 12), ("flat", 51), ("flat", 77)])
def test_random_composite_scenes_on_the_gpu(gpu_ctx, gen, seed):
    """The fuzz of tests/test_hostsim_parity.py (zoo.random_composites / zoo.random_flat) through the C ABI, ray batches with
    unit and with non-unit directions (a caller's rays need not be normalised; Refract's are not) and a frame."""
    sd = (zoo.random_composites if gen == "composites" else zoo.random_flat)(seed)
    b, nm, sc = commit(gpu_ctx, sd)
    parity.check_rays(lambda o, d: sc.rayint(o, d), lambda o, d, t: sc.shadow(o, d, t), sc.inside, sd, nm, n=20000)
    o, om, _ = oracle_for(sd)
    ro, rd = random_rays(6000, 3, center=(0, 1.5, 0), radius=13, spread=7)
    rd = (rd * np.random.default_rng(seed).uniform(0.4, 3.0, size=(len(rd), 1))).astype(np.float32)
    got, want = sc.rayint(ro, rd), o.rayint(om[sd.root], ro.astype(np.float64), rd.astype(np.float64))
    assert np.mean((got["t"] >= 0) != (want["t"] >= 0)) <= 5e-4  # (t itself cancels badly in fp32 for such rays and spheres: not compared)
    cam, lights = product_camera_lights(sd)
    W, H = 192, 108
    img, packed, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=3))
    ref, _, rc = o.render(W, H, maxdepth=3, want_packed=False)
    of, _, _ = oracle_for(sd, use_float=True)
    ref32, _, _ = of.render(W, H, maxdepth=3, want_packed=False)
    err = lambda a, r: (np.abs(a[..., :4] - r[..., :4]) / np.maximum(1, np.abs(r[..., :4]))).max(-1)
    both = (err(img, ref) > 1e-4) & (err(img, ref32) > 1e-4)
    assert both.mean() <= 2e-3, (int(both.sum()), np.argwhere(both)[:6].tolist())
    assert st["rays_primary"] == rc["rays_primary"] and abs(st["rays_shadow"] - rc["rays_shadow"]) <= max(8, rc["rays_shadow"] // 100)
    sc.release()


def test_axis_aligned_camera_reproduces_the_centre_column(gpu_ctx):
    """GlomeView's camera looking straight down -z at an even-width frame: the centre column's rays have an x component of
    exactly +0, for which the reference's slab test (bbclip_ub, Vec.hs:743-762; Q1) misses every box and every bih -- (hi - o)
    / 0 = +inf on the entry side -- while spheres, cones and instances are hit as usual.  The reference renders that column
    empty behind boxes and bihs; so must we: the pixel coordinate 96 / 192 has to come out as exactly 0.5 on the device (the
    kernels are built with the fast fp32 division, which is an ulp off), and the direction's zero keeps its sign."""
    from glome_amd.scene import SceneDesc
    W, H = 192, 108
    for kind in ("box", "bih", "sphere", "cone"):
        sd = SceneDesc()
        m = scenes.materials(sd)
        it = {"box": lambda: sd.box((-2, 0.5, -1), (2, 3.5, 1)), "sphere": lambda: sd.sphere((0, 2, 0), 1.5), "cone": lambda: sd.cone((0, 0.5, 0), 1.5, (0, 3.5, 0), 0.2),
              "bih": lambda: sd.bih([sd.sphere((-1.0, 2, 0), 1.2), sd.sphere((1.0, 2, 0), 1.2), sd.sphere((0, 3.5, 0), 0.7)])}[kind]()
        sd.set_root(sd.group([sd.tex(it, m["shiny_red"])]))
        sd.add_light(*scenes.LIGHTS[0]); sd.set_camera((0.0, 2.0, 12.0), (0.0, 2.0, 0.0), (0, 1, 0), 45.0)
        b, nm, sc = commit(gpu_ctx, sd)
        cam, lights = product_camera_lights(sd)
        o, om, _ = oracle_for(sd)
        for mode in (0, 1):
            img, _, st = sc.render(cam, lights, api.render_params(width=W, height=H, maxdepth=1, mode=mode))
            ref, _, rc = o.render(W, H, maxdepth=1, mode=mode, want_packed=False)
            assert np.array_equal(img[..., 3] > 0, ref[..., 3] > 0), (kind, mode)  # the same pixels are covered, column 96 included
            if mode == 0:
                assert (ref[:, 96, 3] > 0).sum() == (0 if kind in ("box", "bih") else (ref[:, 95, 3] > 0).sum())
        sc.release()


def test_default_scene_at_the_reference_window_beyond_rounding(gpu_ctx):
    """GlomeView's default scene WITH the oak at GlomeView's own 720x480 (Glome.hs:112-113), both render modes.  The scene
    states wide bounds against the fp64 oracle (scenes.testscene); what this test adds is the gate that says those pixels are
    ROUNDING (parity.away_beyond_rounding): outside the set of pixels where the oracle itself, computing in fp32 with the eye
    an ulp off, leaves the fp64 frame, the GPU may differ from the fp64 oracle on 5e-4 of the pixels like any other scene."""
    sd = zoo.testscene(10)
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    for mode in (0, 1):
        img, _, st = sc.render(cam, lights, api.render_params(width=720, height=480, maxdepth=3, mode=mode), want_packed=False)
        lv = parity.away_beyond_rounding(img, sd, 720, 480, 3, mode=mode, jitters=12)  # (measured with 8: 4.9e-4 / 6.3e-4; 87 % / 95 % inside)
        assert lv["away_outside_sensitive"] <= (5e-4 if mode == 0 else 1.5e-3), lv
        assert lv["away_inside_sensitive_share"] >= 0.75, lv  # (a random 2-3 % of the frame would hold 2-3 % of them)
        assert lv["away_fp64"] <= (sd.pixel_outlier_max if mode == 0 else sd.subsample_outlier_max), lv
    sc.release()


def test_oak_alone_where_its_twigs_are_not_sub_pixel(gpu_ctx):
    """The oak of TestScene.hs:68-110 by itself over a floor, the camera close enough that a twig is several pixels wide: the
    strict gates of every other scene hold for hit / miss and depth, and the pixels that differ from the fp64 oracle lie where the
    fp32 oracle's do."""
    from glome_amd.scene import SceneDesc
    sd = SceneDesc()
    pl = sd.tex(sd.plane((0, 0, 0), (0, 1, 0)), scenes.matte(sd, (0, 0.8, 0.3)))
    sd.set_root(sd.group([pl, sd.transform(scenes.oak(sd, 8.4, 42), [api.translate((0, 0.01, 0))])]))
    for pos, col in scenes.LIGHTS[:2]:
        sd.add_light(pos, col)
    sd.set_camera((1.5, 3.2, 6.5), (0, 2.6, 0), (0, 1, 0), 45)
    b, nm, sc = commit(gpu_ctx, sd)
    cam, lights = product_camera_lights(sd)
    img, _, st = sc.render(cam, lights, api.render_params(width=480, height=360, maxdepth=2), want_packed=False)
    o, om, _ = oracle_for(sd)
    ref, _, rc = o.render(480, 360, maxdepth=2, want_packed=False)
    hit_g, hit_r = img[..., 4] < 1e6, ref[..., 4] < 1e6
    both = hit_g & hit_r
    assert np.mean(hit_g != hit_r) <= 3e-4
    assert np.mean(np.abs(img[..., 4][both] - ref[..., 4][both]) / np.maximum(1, ref[..., 4][both]) > 1e-4) <= 5e-4
    lv = parity.away_beyond_rounding(img, sd, 480, 360, 2)
    assert lv["away_outside_sensitive"] <= 5e-4, lv
    sc.release()


def test_closure_fallback_host_shading_over_the_batch_seams(gpu_ctx):
    """tests/test_hostsim_parity.py's contract check through the real C ABI: a host that keeps trace / mpreshade / mpostshade for
    its closure textures and calls glome_rayint_batch / glome_shadow_batch reproduces glome_render's frames and ray counts."""
    from test_hostsim_parity import _closure_fallback_checks
    made = []

    def make_backend(sd):
        b, nm, sc = commit(gpu_ctx, sd)
        made.append(sc)
        _, mm = sd.replay(api.Builder())  # (material ids are assigned in call order: the same in every builder)
        return sc, mm

    def render_ref(sc, cam, lights, w, h, md):
        img, _, st = sc.render(cam, lights, api.render_params(width=w, height=h, maxdepth=md), want_packed=False)
        return img, [st["rays_primary"], st["rays_shadow"], st["rays_secondary"]]
    _closure_fallback_checks(make_backend, render_ref, exact=False)
    for sc in made:
        sc.release()


@pytest.mark.parametrize("nframes,w,h", [(32, 200, 120), (5, 333, 97), (32, 1920, 1080)])
def test_renderTile_frame_batches_equal_the_frames_rendered_alone(gpu_ctx, s3_full, nframes, w, h):
    """Up to 32 frames per launch, interleaved in the work queue chunk by chunk (chunk c of every frame, then chunk c + 1 ...;
    render_kernels.hpp render_loop): every frame of a batch -- different views, frame sizes whose item counts are no multiple of a
    chunk -- is, pixel for pixel, the frame rendered alone; through the whole-frame entry and through a rank's dense tile payload."""
    import torch
    sd, sc = s3_full
    dev = torch.device("cuda:0")
    cam, lights = product_camera_lights(sd)
    la = (L.Light * len(lights))(*lights)
    pos, at, up, ang = sd.cam
    views = [api.camera((pos[0] + 0.21 * f, pos[1] + 0.05 * (f % 3), pos[2] - 0.1 * f), at, up, ang) for f in range(nframes)]
    cams = (L.Camera * nframes)(*views)
    P = api.render_params(width=w, height=h, maxdepth=1)
    px = torch.zeros((nframes, h, w), dtype=torch.int32, device=dev)
    assert sc.lib.glome_render_packed_batch_dev(sc.h, cams, nframes, la, len(lights), C.byref(P), C.c_void_p(px.data_ptr()), h * w, None) == 0, gpu_ctx.err()
    gpu_ctx.synchronize()
    got = px.cpu().numpy().view(np.uint32)
    one = torch.zeros((h, w), dtype=torch.int32, device=dev)
    for f in (range(nframes) if w < 1000 else (0, 13, 31)):
        one.zero_()
        sc.render_dev(views[f], lights, P, None, one.data_ptr(), want_stats=False)
        gpu_ctx.synchronize()
        assert np.array_equal(got[f], one.cpu().numpy().view(np.uint32)), f
    if w < 1000:  # a rank's shard (tiles 1, 4, 7 ... of three ranks) of the same frames as a dense payload
        Pl = api.render_params(width=w, height=h, maxdepth=1, tile_first=1, tile_stride=3, blocksize=64)
        n = dist.payload_floats(Pl, 1, 3) // 5
        pay = torch.zeros((nframes, n), dtype=torch.int32, device=dev)
        assert sc.lib.glome_render_tiles_packed_batch_dev(sc.h, cams, nframes, la, len(lights), C.byref(Pl), C.c_void_p(pay.data_ptr()), n, None) == 0, gpu_ctx.err()
        gpu_ctx.synchronize()
        lay = dist.owned_layout(Pl, 1, 3)
        payh = pay.cpu().numpy().view(np.uint32)
        for f in range(nframes):
            assert np.array_equal(payh[f], dist.pack_numpy(got[f], lay)), f


def test_csg_items_of_the_flat_tier_advance_without_a_cap(gpu_ctx):
    """tests/test_hostsim_parity.py's check through the C ABI: the scenes that used to stop a launch with GLOME_E_LIMIT render."""
    from test_hostsim_parity import _many_sided_intersection_scene
    for sd in (zoo.random_rig(zoo.random_flat(12094), 12094), _many_sided_intersection_scene()):
        b, nm, sc = commit(gpu_ctx, sd)
        assert sc.info()["tier"] == 0
        cam, lights = product_camera_lights(sd)
        for mode in (0, 1):
            img, _, st = sc.render(cam, lights, api.render_params(width=192, height=108, maxdepth=3, mode=mode), want_packed=False)  # (raises on a limit)
            o, _, _ = oracle_for(sd)
            o32, _, _ = oracle_for(sd, use_float=True)
            ref, _, rc = o.render(192, 108, maxdepth=3, mode=mode, want_packed=False)
            r32, _, _ = o32.render(192, 108, maxdepth=3, mode=mode, want_packed=False)
            err = lambda a, r: (np.abs(a[..., :4] - r[..., :4]) / np.maximum(1, np.abs(r[..., :4]))).max(-1)
            both = (err(img, ref) > 1e-4) & (err(img, r32) > 1e-4)
            assert both.mean() <= (2e-3 if mode == 0 else 6e-3), (mode, int(both.sum()))
        sc.release()


@pytest.mark.gpu
@pytest.mark.parametrize("ranks,transport,group", [(2, "direct", 4), (3, "direct", 4), (2, "gather", 4), (3, "auto", None), (2, "gather", None)])
def test_one_process_per_gpu_job_rehearsed_on_one_gpu(ranks, transport, group):
    """bench.py --gpus N as the driver launches it -- one process per rank, torch.distributed -- rehearsed on the one GPU of the box
    (--rehearse: gloo instead of RCCL, every rank on device 0).  `direct` (round 4): every rank's kernel stores its tiles straight
    into rank 0's frames, mapped into the other processes through HIP IPC handles (glome_ipc_*); `gather`: payloads to rank 0 and a
    blit.  Either way the last frame rank 0 holds equals the same view rendered whole on its GPU, bit for bit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(ranks), "--rehearse", "--transport", transport, "--scene", "S3", "--steps", "9", "--warmup", "3",
                        "--full", "--no-cpu"] + (["--group", str(group)] if group else []),  # (no --group: bench.py's own rule -- one launch of nine frames when the frames can be mapped)
                       capture_output=True, text=True, timeout=500, env=env, cwd=root)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-2500:])
    line = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == ranks and line["frame_equals_single_gpu_render"] is True, line
    assert line["config"]["transport"].startswith("direct" if transport == "auto" else transport), line["config"]["transport"]
    if group is None:
        assert line["config"]["frames_per_launch"] == (9 if transport == "auto" else 4), line["config"]
