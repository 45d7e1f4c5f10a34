"""GPU suite (-m gpu): glome_render_lens_adaptive.  Every pixel of its three frames -- rgbad, packed, counts -- is held, bit for bit, to
glome_adaptive_fold (the rule on the host, test_lens_adaptive_host.py) of the tuples the stages give by hand at samples = max; and,
without passing through the fold function at all, to the pixels of glome_render_lens at samples = the pixel's own count."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_lens_abi import PINHOLE, THIN, THIN_KW
from test_lens_gpu import DEV, SENT, committed, device_rays, ptrs  # noqa: F401  (committed: the module's scenes, a fixture)
from glome_amd import _lib as L
from glome_amd import api

pytestmark = pytest.mark.gpu

# Chosen once on the GPU so that every level of (2, 8) is some pixel's count in every frame below and neither end holds nine pixels in
# ten: the thin lens of THIN_KW blurs S1's and the zoo's spheres by a few pixels, and the halves of such a pixel differ by a few 1/64.
# Pixels per level at this threshold and seed on an MI355X, S1 / materials:
#   67 x 35 (2, 8) 1765 166 414 / 1894 245 206;  (4, 64) 1777 158 71 51 288 / 1958 209 69 32 77 (the largest share of a level: 0.835)
#   70 x 9  (2, 8)  509  46  75 /  513 47 70;  (4, 64) 515 48 23 6 38 / 515 52 25 13 25;  9 x 7 (2, 8) 32 9 22 (S1)
# (1/32 leaves materials' 67 x 35 at (4, 64) with 0.902 of its pixels at base; 1/128 would do as well as 1/64.)
THRESHOLD = 1.0 / 64
SEED = 5
FRAMES = [(67, 35), (70, 9)]
RULES = [(2, 8), (4, 64)]


def raygen(w, h, samples, lens=THIN, jitter=1, seed=SEED):
    return api.raygen_params(width=w, height=h, lens=lens, samples=samples, jitter=jitter, seed=seed, **(THIN_KW if lens == THIN else {}))


@pytest.fixture(scope="module")
def tuples_of(gpu_ctx, committed):
    """the frame's tuples at samples = max through camera_rays -> trace_dev, made once per (scene, frame, max): [pixels, max, 5] and the
    trace's statistics"""
    cache = {}

    def get(name, w, h, mx):
        key = (name, w, h, mx)
        if key not in cache:
            c = committed(name)
            n = w * h * mx
            rays = device_rays(gpu_ctx, c.cam, raygen(w, h, mx))
            res = torch.zeros((n, 5), dtype=torch.float32, device=DEV)
            torch.cuda.synchronize()
            st = c.sc.trace_dev(n, ptrs(rays) + [None], c.lights, api.trace_params(maxdepth=3), res.data_ptr())
            x = res.cpu().numpy().reshape(w * h, mx, 5)
            x.setflags(write=False)
            cache[key] = (x, st)
        return cache[key]
    return get


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def adaptive(c, w, h, base, mx, thr=THRESHOLD, rpp=0, **kw):
    return c.sc.render_lens_adaptive(c.cam, c.lights, raygen(w, h, mx, **kw), api.adaptive_params(base, thr), api.trace_params(maxdepth=3), rays_per_pass=rpp)


# ---------------------------------------------------------------- 1. the stages
@pytest.mark.parametrize("base,mx", RULES)
@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("name", ["S1", "materials"])
def test_every_pixel_is_the_host_fold_of_its_tuples(committed, tuples_of, name, w, h, base, mx):
    c = committed(name)
    x, _ = tuples_of(name, w, h, mx)
    want_counts, want, want_packed = api.adaptive_fold(x, base, THRESHOLD)
    img, packed, counts, st = adaptive(c, w, h, base, mx)
    levels = api.adaptive_levels(base, mx)
    share = {l: float((counts == l).mean()) for l in levels}
    print(name, (w, h), (base, mx), "share of pixels per level", share)
    assert img.shape == (h, w, 5) and packed.shape == counts.shape == (h, w) and counts.dtype == np.uint8
    assert np.array_equal(counts.ravel(), want_counts)
    assert np.array_equal(bits(img.reshape(-1, 5)), bits(want)) and np.array_equal(packed.ravel(), want_packed)
    if (base, mx) == (2, 8):
        assert all(share[l] > 0 for l in levels), share  # every level of (2, 8) occurs
    assert share[base] <= 0.9 and share[mx] <= 0.9, share
    assert st["rays_primary"] == int(counts.astype(np.int64).sum()) and st["n_pixels"] == w * h and st["kernel_ms"] > 0


# ---------------------------------------------------------------- 2. without the fold function: the fixed frames
@pytest.mark.parametrize("name", ["S1", "materials"])
def test_a_pixel_that_stopped_at_c_is_the_fixed_frame_at_c_samples(committed, name):
    c = committed(name)
    w, h = 67, 35
    for base, mx in RULES:
        img, packed, counts, _ = adaptive(c, w, h, base, mx)
        present = sorted(set(counts.ravel().tolist()))
        assert len(present) >= 2
        for n in present:
            fixed, fixed_packed, _ = c.sc.render_lens(c.cam, c.lights, raygen(w, h, n), api.trace_params(maxdepth=3))
            m = counts == n
            assert np.array_equal(bits(img[m]), bits(fixed[m])) and np.array_equal(packed[m], fixed_packed[m]), (base, mx, n)


# ---------------------------------------------------------------- 3. rays_per_pass
@pytest.mark.parametrize("w,h,rpps", [(67, 35, (0, 800)), (9, 7, (0, 32, 1))])
def test_the_frames_do_not_depend_on_rays_per_pass(committed, w, h, rpps):
    """(2, 8): 800 rays are 100 pixels a pass -- a boundary inside the rows of 67, a last pass of 45; 32 rays are 4 pixels of a row of 9,
    a last pass of 3; 1 ray is a pixel a pass"""
    c = committed("S1")
    got = [adaptive(c, w, h, 2, 8, rpp=rpp) for rpp in rpps]
    img0, packed0, counts0, st0 = got[0]
    assert len(set(counts0.ravel().tolist())) >= 2 and (img0[..., 4] < 1e6).any()
    for img, packed, counts, st in got:
        assert np.array_equal(bits(img), bits(img0)) and np.array_equal(packed, packed0) and np.array_equal(counts, counts0)
        assert st["rays_primary"] == int(counts0.astype(np.int64).sum())
        assert (st["rays_shadow"], st["rays_secondary"]) == (st0["rays_shadow"], st0["rays_secondary"]) and st["n_pixels"] == w * h
    assert st0["rays_shadow"] > 0


# ---------------------------------------------------------------- 4. degenerate rules
def test_degenerate_rules_are_fixed_frames(committed):
    c = committed("S1")
    w, h = 67, 35
    tp = api.trace_params(maxdepth=3)

    def fixed(samples, **kw):
        return c.sc.render_lens(c.cam, c.lights, raygen(w, h, samples, **kw), tp)

    def same(a, f, count):
        return np.array_equal(bits(a[0]), bits(f[0])) and np.array_equal(a[1], f[1]) and np.all(a[2] == count)

    # a pinhole without jitter: every sample of a pixel is the same ray
    assert same(adaptive(c, w, h, 4, 16, lens=PINHOLE, jitter=0), fixed(4, lens=PINHOLE, jitter=0), 4)
    # no threshold at all
    assert same(adaptive(c, w, h, 4, 16, thr=float("inf")), fixed(4), 4)
    # one level
    assert same(adaptive(c, w, h, 16, 16), fixed(16), 16)
    assert same(adaptive(c, w, h, 6, 6, thr=0.0), fixed(6), 6)
    # a 1 x 1 frame
    one = c.sc.render_lens_adaptive(c.cam, c.lights, raygen(1, 1, 8), api.adaptive_params(2, THRESHOLD), tp)
    assert one[0].shape == (1, 1, 5) and int(one[2][0, 0]) in (2, 4, 8) and one[3]["rays_primary"] == int(one[2][0, 0])
    f = c.sc.render_lens(c.cam, c.lights, raygen(1, 1, int(one[2][0, 0])), tp)
    assert np.array_equal(bits(one[0]), bits(f[0])) and np.array_equal(one[1], f[1])


# ---------------------------------------------------------------- 5. the device-pointer form
def test_the_dev_form_on_torch_tensors(gpu_ctx, committed):
    c = committed("materials")
    w, h, base, mx = 70, 9, 2, 8
    n, pad = w * h, 64
    img0, packed0, counts0, st0 = adaptive(c, w, h, base, mx)
    rp, ap, tp = raygen(w, h, mx), api.adaptive_params(base, THRESHOLD), api.trace_params(maxdepth=3)
    frame = torch.empty((n + 2 * pad, 5), dtype=torch.float32, device=DEV)
    words = torch.empty((n + 2 * pad,), dtype=torch.int32, device=DEV)
    cnt = torch.empty((n + 2 * pad,), dtype=torch.uint8, device=DEV)

    def run(want_rgbad=True, want_packed=True, want_counts=True, **kw):
        frame.fill_(SENT); words.fill_(-77); cnt.fill_(211)
        torch.cuda.synchronize()
        st = c.sc.render_lens_adaptive_dev(c.cam, c.lights, rp, ap, tp, frame[pad:].data_ptr() if want_rgbad else None, words[pad:].data_ptr() if want_packed else None,
                                           cnt[pad:].data_ptr() if want_counts else None, **kw)
        gpu_ctx.synchronize()
        f, p, k = frame.cpu().numpy(), words.cpu().numpy(), cnt.cpu().numpy()
        inside = np.zeros(n + 2 * pad, bool); inside[pad:pad + n] = True
        assert np.all(f[~inside] == SENT) and np.all(p[~inside] == -77) and np.all(k[~inside] == 211)  # nothing outside the frames
        return f[inside], p[inside].view(np.uint32), k[inside], st

    f, p, k, st = run()
    assert np.array_equal(bits(f), bits(img0.reshape(-1, 5))) and np.array_equal(p, packed0.ravel()) and np.array_equal(k, counts0.ravel())
    assert (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]) == (st0["rays_primary"], st0["rays_shadow"], st0["rays_secondary"])
    f, p, k, st = run(want_stats=False, rays_per_pass=8 * 100)  # without statistics
    assert st is None
    assert np.array_equal(bits(f), bits(img0.reshape(-1, 5))) and np.array_equal(p, packed0.ravel()) and np.array_equal(k, counts0.ravel())
    f, p, k, _ = run(want_rgbad=False)  # only the packed words (and the counts)
    assert np.all(f == SENT) and np.array_equal(p, packed0.ravel()) and np.array_equal(k, counts0.ravel())
    f, p, k, _ = run(want_packed=False, want_counts=False)
    assert np.array_equal(bits(f), bits(img0.reshape(-1, 5))) and np.all(p.view(np.int32) == -77) and np.all(k == 211)
    # the host form without its optional frames
    img, packed, _, _ = c.sc.render_lens_adaptive(c.cam, c.lights, rp, ap, tp, want_packed=False)
    assert packed is None and np.array_equal(bits(img), bits(img0))


# ---------------------------------------------------------------- 6. refusals
def test_refused_arguments_fail_before_anything_is_launched(gpu_ctx, committed):
    c = committed("S1")
    lib, cam = gpu_ctx.lib, c.cam
    w, h = 67, 35
    la = (L.Light * len(c.lights))(*c.lights)
    tp = api.trace_params()
    good = dict(width=w, height=h, lens=THIN, samples=8, jitter=1, seed=2, **THIN_KW)
    img = np.full((h, w, 5), SENT, np.float32); pk = np.full((h, w), 77, np.uint32); cn = np.full((h, w), 211, np.uint8)
    frame = torch.full((w * h, 5), SENT, dtype=torch.float32, device=DEV)
    words = torch.full((w * h,), -77, dtype=torch.int32, device=DEV)
    cnt = torch.full((w * h,), 211, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    bp = C.POINTER(C.c_uint8)

    def refused(cam_, p, ap, lights=la, nl=len(c.lights), tp_=tp, rpp=0, out=True, status=L.E_INVALID):
        cc = C.byref(cam_) if cam_ is not None else None
        pp = C.byref(p) if p is not None else None
        tt = C.byref(tp_) if tp_ is not None else None
        aa = C.byref(ap) if ap is not None else None
        assert lib.glome_render_lens_adaptive(c.sc.h, cc, pp, lights, nl, tt, aa, rpp, img.ctypes.data_as(L.c_fp) if out else None,
                                              pk.ctypes.data_as(L.c_up) if out else None, cn.ctypes.data_as(bp), None) == status and gpu_ctx.err()
        assert lib.glome_render_lens_adaptive_dev(c.sc.h, cc, pp, lights, nl, tt, aa, rpp, vp(frame) if out else None, vp(words) if out else None, vp(cnt), None) == status

    ok = api.adaptive_params(2, THRESHOLD)
    bad_cam = api.camera_from_vectors(list(cam.pos), list(cam.fwd), list(cam.up), list(cam.right)); bad_cam.fwd[1] = float("inf")
    # what glome_render_lens refuses
    refused(None, api.raygen_params(**good), ok)
    refused(cam, None, ok)
    refused(cam, api.raygen_params(**good), ok, tp_=None)
    refused(cam, api.raygen_params(**good), ok, out=False)
    refused(cam, api.raygen_params(**good), ok, nl=-1)
    refused(cam, api.raygen_params(**good), ok, lights=None, nl=1)
    refused(cam, api.raygen_params(**good), ok, rpp=-1)
    refused(cam, api.raygen_params(**{**good, "samples": 128}), ok)
    refused(cam, api.raygen_params(**{**good, "focus_dist": 0.0}), ok)
    refused(bad_cam, api.raygen_params(**good), ok)
    refused(cam, api.raygen_params(width=65536, height=32768, samples=8), ok)  # 2^31 pixels: not a frame
    refused(cam, api.raygen_params(**good), ok, tp_=api.trace_params(maxdepth=9), status=L.E_LIMIT)
    refused(cam, api.raygen_params(**good), ok, lights=(L.Light * 17)(*([c.lights[0]] * 17)), nl=17, status=L.E_LIMIT)
    # its own
    refused(cam, api.raygen_params(**good), None)
    for base in (0, 1, 3, 6, 16, -2):  # (samples = 8)
        refused(cam, api.raygen_params(**good), api.adaptive_params(base, THRESHOLD))
    refused(cam, api.raygen_params(**{**good, "samples": 12}), api.adaptive_params(4, THRESHOLD))
    refused(cam, api.raygen_params(**{**good, "samples": 1}), api.adaptive_params(2, THRESHOLD))
    for thr in (float("nan"), -1.0, float("-inf")):
        refused(cam, api.raygen_params(**good), api.adaptive_params(2, thr))
    refused(cam, api.raygen_params(width=32768, height=32768, samples=4), api.adaptive_params(2, THRESHOLD))  # 2^32 rays at max
    assert lib.glome_render_lens_adaptive(None, C.byref(cam), C.byref(api.raygen_params(**good)), la, len(c.lights), C.byref(tp), C.byref(ok), 0,
                                          img.ctypes.data_as(L.c_fp), None, None, None) == L.E_INVALID
    # nothing was launched, nothing written
    gpu_ctx.synchronize()
    assert np.all(img == SENT) and np.all(pk == 77) and np.all(cn == 211)
    assert np.all(frame.cpu().numpy() == SENT) and np.all(words.cpu().numpy() == -77) and np.all(cnt.cpu().numpy() == 211)
    # and the scene is as good as before
    img2, _, counts, st = c.sc.render_lens_adaptive(cam, c.lights, api.raygen_params(**good), ok)
    assert st["n_pixels"] == w * h and (img2[..., 4] < 1e6).any() and st["rays_primary"] == int(counts.astype(np.int64).sum())
