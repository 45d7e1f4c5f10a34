"""GPU suite (-m gpu): the trace seam's lens stages -- glome_camera_rays (raygen on the device), glome_resolve_dev (the per-pixel fold of a
trace's results) and glome_render_lens (raygen -> trace -> resolve in bounded passes).  The device rays are held to the float64
restatement of the lens formulas (test_lens_abi.py, which also shows the bounds are within fp32's reach), the resolve to a NumPy float32
restatement bit for bit, the one-call form to its stages bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity
import zoo
from helpers import product_camera_lights
from test_lens_abi import LATLONG, PINHOLE, THIN, THIN_KW, cameras, lens_rays, library_words, scale_of
from glome_amd import _lib as L
from glome_amd import api, scenes

pytestmark = pytest.mark.gpu

SCENES = {"S1": lambda: scenes.s1(nlights=2), "S4": scenes.s4, "nested": zoo.nested, "materials": zoo.materials}
DEV = "cuda:0"


class Committed:
    def __init__(self, ctx, name):
        self.sd = SCENES[name]()
        self.b = api.Builder()
        self.nm, _ = self.sd.replay(self.b)
        self.sc = ctx.commit(self.b, self.nm[self.sd.root])
        self.cam, self.lights = product_camera_lights(self.sd)


@pytest.fixture(scope="module")
def committed(gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Committed(gpu_ctx, name)
        return cache[name]
    yield get
    for c in cache.values():
        c.sc.release()


def ray_buffers(n, fill=0.0):
    t = torch.full((6, max(n, 1)), fill, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    return t


def ptrs(t, offset=0):
    return [t[k].data_ptr() + 4 * offset for k in range(6)]


def device_rays(ctx, cam, params, first=0, n=None):
    """camera_rays_dev into fresh device streams: the 6 x n tensor"""
    n = int(ctx.lib.glome_raygen_count(C.byref(params))) - first if n is None else n
    t = ray_buffers(n)
    ctx.camera_rays_dev(cam, params, first, n, ptrs(t))
    ctx.synchronize()
    return t


def od(t):
    a = t.cpu().numpy()
    return a[:3].T.copy(), a[3:].T.copy()


def unit_rule(d):
    return np.abs((d.astype(np.float64) ** 2).sum(1) - 1).max()


# ---------------------------------------------------------------- 1. pinhole
@pytest.mark.parametrize("cam_name", ["S1", "axis"])
def test_pinhole_rays_are_get_rayint(gpu_ctx, cam_name):
    """67 x 35, one sample, no jitter: 2,345 rays, a last item of 41.  A direction goes through fewer than ten fp32 roundings of quantities
    below 2, 2^-24 relative each: 1e-6 absolute per component against float64."""
    cam = cameras()[cam_name]
    p = api.raygen_params(width=67, height=35)
    o, d = od(device_rays(gpu_ctx, cam, p))
    assert o.shape == d.shape == (2345, 3)
    assert np.array_equal(o.view(np.uint32), np.broadcast_to(np.array(list(cam.pos), np.float32), o.shape).view(np.uint32))
    _, want = lens_rays(cam, 67, 35, PINHOLE)
    e = np.abs(d - want).max()
    print("pinhole", cam_name, "max error", e, "unit", unit_rule(d))
    assert e <= 1e-6
    assert unit_rule(d) <= 1e-5
    ho, hd = gpu_ctx.camera_rays(cam, p)  # the host form: the same rays
    assert np.array_equal(ho, o) and np.array_equal(hd, d)


# ---------------------------------------------------------------- 2. the device's own rays give the oracle frame
@pytest.mark.parametrize("name", ["S1", "S4", "nested"])
def test_device_pinhole_rays_traced_give_the_oracle_frame(gpu_ctx, committed, name):
    """test_frame_rays_traced_as_a_batch_give_the_oracle_frame with the rays made on the device, under the same gates, ray counts included"""
    c = committed(name)
    w, h = 320, 180
    rays = device_rays(gpu_ctx, c.cam, api.raygen_params(width=w, height=h))
    out = torch.zeros((w * h, 5), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    st = c.sc.trace_dev(w * h, ptrs(rays) + [None], c.lights, api.trace_params(maxdepth=3), out.data_ptr())
    assert st["n_pixels"] == w * h and st["n_tiles"] == w * h // 64
    parity.check_image(out.cpu().numpy().reshape(h, w, 5), (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]), c.sd, w, h, 3)


# ---------------------------------------------------------------- 3. thin lens and latitude-longitude
@pytest.mark.parametrize("seed", [1, 0xdeadbeef])
@pytest.mark.parametrize("lens", [THIN, LATLONG])
def test_thin_and_latlong_rays_against_float64(gpu_ctx, committed, lens, seed):
    """33 x 17, five samples, jittered: within 1e-5 * max(1, |pos|, aperture, focus_dist) of the float64 restatement fed the library's own
    sample words; unit length; and legal for a production trace."""
    c = committed("S1")
    kw = THIN_KW if lens == THIN else {}
    p = api.raygen_params(width=33, height=17, lens=lens, samples=5, jitter=1, seed=seed, **kw)
    rays = device_rays(gpu_ctx, c.cam, p)
    o, d = od(rays)
    wo, wd = lens_rays(c.cam, 33, 17, lens, samples=5, jitter=1, seed=seed, words=library_words, **kw)
    bound = 1e-5 * scale_of(c.cam, **kw)
    eo, ed = np.abs(o - wo).max(), np.abs(d - wd).max()
    print("lens", lens, seed, "max error o, d:", eo, ed, "bound", bound, "unit", unit_rule(d))
    assert eo <= bound and ed <= bound
    assert unit_rule(d) <= 1e-5
    if lens == LATLONG:
        assert np.array_equal(o, np.broadcast_to(np.array(list(c.cam.pos), np.float32), o.shape))
    else:
        assert len(np.unique(o, axis=0)) > 2000  # (a lens point per ray)
    n = 33 * 17 * 5
    out = torch.zeros((n, 5), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    st = c.sc.trace_dev(n, ptrs(rays) + [None], c.lights, api.trace_params(maxdepth=3, faithful=0), out.data_ptr())  # (raises on a status)
    assert st["rays_primary"] == n


def test_a_thin_lens_without_aperture_is_the_pinhole(gpu_ctx):
    cam = cameras()["S1"]
    kw = dict(width=33, height=17, samples=5, jitter=1, seed=1)
    _, dp = od(device_rays(gpu_ctx, cam, api.raygen_params(lens=PINHOLE, **kw)))
    ot, dt = od(device_rays(gpu_ctx, cam, api.raygen_params(lens=THIN, aperture=0.0, focus_dist=14.0, **kw)))
    assert np.abs(dp - dt).max() <= 1e-6
    assert np.array_equal(ot, np.broadcast_to(np.array(list(cam.pos), np.float32), ot.shape))


# ---------------------------------------------------------------- 4. ranges and determinism
@pytest.mark.parametrize("lens", [PINHOLE, THIN, LATLONG])
def test_ranges_and_determinism(gpu_ctx, lens):
    cam = cameras()["S1"]
    kw = dict(width=67, height=35, lens=lens, samples=5, **(THIN_KW if lens == THIN else {}))
    p = api.raygen_params(jitter=1, seed=3, **kw)
    n = 67 * 35 * 5
    whole = device_rays(gpu_ctx, cam, p).cpu().numpy()
    parts = ray_buffers(n + 1, fill=-7.5)
    for a, b in ((0, 1000), (1000, 7777), (7777, n)):  # (inside a work item both, 7777 inside a pixel's samples as well)
        gpu_ctx.camera_rays_dev(cam, p, a, b - a, ptrs(parts, a))
    gpu_ctx.synchronize()
    parts = parts.cpu().numpy()
    assert np.array_equal(parts[:, :n].view(np.uint32), whole.view(np.uint32)) and np.all(parts[:, n] == -7.5)
    assert np.array_equal(device_rays(gpu_ctx, cam, p).cpu().numpy().view(np.uint32), whole.view(np.uint32))
    other = device_rays(gpu_ctx, cam, api.raygen_params(jitter=1, seed=4, **kw)).cpu().numpy()
    assert np.mean(np.any(other[3:] != whole[3:], axis=0)) > 0.99
    a = device_rays(gpu_ctx, cam, api.raygen_params(jitter=0, seed=3, **kw)).cpu().numpy()
    b = device_rays(gpu_ctx, cam, api.raygen_params(jitter=0, seed=4, **kw)).cpu().numpy()
    if lens == THIN:
        assert np.any(a != b)  # (the lens point is drawn with or without jitter)
    else:
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(a.reshape(6, -1, 5)[:, :, 0], a.reshape(6, -1, 5)[:, :, 4])  # every sample at the pixel's own coordinates


# ---------------------------------------------------------------- 5. resolve
W, H = 67, 35
SENT = -7.5


@pytest.fixture(scope="module")
def tuples():
    """67 x 35 x 64 random tuples, made once: colours in [0, 2) (beyond cap1), depths a mix of misses (1e6) and finite values"""
    rng = np.random.default_rng(17)
    x = rng.uniform(0, 2, size=(W * H, 64, 5)).astype(np.float32)
    x[..., 4] = np.where(rng.uniform(size=(W * H, 64)) < 0.4, np.float32(1e6), rng.uniform(0.5, 40, size=(W * H, 64)).astype(np.float32))
    x[::29, :, 4] = np.float32(1e6)  # (and pixels every sample of which misses)
    x.setflags(write=False)
    return x


def resolve_np(x):
    """the contract in NumPy float32: sequential sums from sample 0, one correctly rounded division, the least depth; rgbf of the
    premultiplied colour (Glome.hs:98-110)"""
    acc = x[:, 0, :4].copy()
    for s in range(1, x.shape[1]):
        acc = acc + x[:, s, :4]
    assert acc.dtype == np.float32
    out = np.concatenate([acc / np.float32(x.shape[1]), x[:, :, 4].min(axis=1, keepdims=True)], axis=1)
    cap1 = lambda v: np.where(v >= 1, np.float32(1) - np.float32(0.0001), v)
    ch = [np.floor(cap1(out[:, k] * out[:, 3]) * np.float32(256)).astype(np.int64) for k in range(3)]
    packed = ((ch[0] * 65536 + ch[1] * 256 + ch[2]) & 0xffffffff).astype(np.uint32)
    return out, packed


def run_resolve(ctx, x, first, n, want_rgbad=True, want_packed=True):
    """resolve_dev of pixels first .. first + n - 1 into sentinel-filled frames; the input pointer is the range's own first tuple"""
    samples = x.shape[1]
    src = torch.tensor(x, device=DEV)
    frame = torch.full((W * H, 5), SENT, dtype=torch.float32, device=DEV)
    packed = torch.full((W * H,), -77, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.resolve_dev(W, H, samples, first, n, src.data_ptr() + first * samples * 20, frame.data_ptr() if want_rgbad else None, packed.data_ptr() if want_packed else None)
    ctx.synchronize()
    return frame.cpu().numpy(), packed.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("samples", [1, 2, 5, 64])
def test_resolve_is_the_sequential_float32_sum(gpu_ctx, tuples, samples):
    x = np.ascontiguousarray(tuples[:, :samples])
    want, want_packed = resolve_np(x)
    got, packed = run_resolve(gpu_ctx, x, 0, W * H)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, 4], x[:, :, 4].min(axis=1)) and (got[:, 4] == 1e6).any() and (got[:, 4] < 1e6).any()
    assert np.array_equal(packed, want_packed) and (got[:, :3] * got[:, 3:4] >= 1).any()  # (cap1 was exercised)
    if samples == 1:
        assert np.array_equal(got.view(np.uint32), x[:, 0].view(np.uint32))
    # a pixel range writes only its pixels -- through the 16-byte loads (pixel 100's tuples start 16-byte aligned) and without them (101's do not)
    for first, n in ((100, 1001), (101, 1001)):
        got, packed = run_resolve(gpu_ctx, x, first, n)
        inside = np.zeros(W * H, bool); inside[first:first + n] = True
        assert np.array_equal(got[inside].view(np.uint32), want[inside].view(np.uint32)) and np.array_equal(packed[inside], want_packed[inside]), first
        assert np.all(got[~inside] == SENT) and np.all(packed[~inside] == np.uint32(-77 & 0xffffffff)), first
    # either output may be absent
    got, packed = run_resolve(gpu_ctx, x, 0, W * H, want_packed=False)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.all(packed == np.uint32(-77 & 0xffffffff))
    got, packed = run_resolve(gpu_ctx, x, 0, W * H, want_rgbad=False)
    assert np.all(got == SENT) and np.array_equal(packed, want_packed)


# ---------------------------------------------------------------- 6. the packed words are glome_render's
def test_packed_words_are_glome_renders(gpu_ctx, committed):
    c = committed("S1")
    w, h = 128, 72
    img, packed, _ = c.sc.render(c.cam, c.lights, api.render_params(width=w, height=h, maxdepth=3))
    assert len(np.unique(packed)) > 100
    src = torch.tensor(img.reshape(-1, 5), device=DEV)
    frame = torch.full((w * h, 5), SENT, dtype=torch.float32, device=DEV)
    words = torch.full((w * h,), -77, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    gpu_ctx.resolve_dev(w, h, 1, 0, w * h, src.data_ptr(), frame.data_ptr(), words.data_ptr())
    gpu_ctx.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), img.reshape(-1, 5).view(np.uint32))
    assert np.array_equal(words.cpu().numpy().view(np.uint32), packed.ravel())


# ---------------------------------------------------------------- 7. render_lens equals its stages
@pytest.mark.parametrize("name", ["S1", "materials"])
def test_render_lens_equals_its_stages(gpu_ctx, committed, name):
    c = committed(name)
    w, h, samples = 67, 35, 5
    n = w * h * samples
    rp = api.raygen_params(width=w, height=h, lens=THIN, samples=samples, jitter=1, seed=5, **THIN_KW)
    tp = api.trace_params(maxdepth=3)
    img0, packed0, st0 = c.sc.render_lens(c.cam, c.lights, rp, tp, rays_per_pass=0)
    img1, packed1, st1 = c.sc.render_lens(c.cam, c.lights, rp, tp, rays_per_pass=1500)  # 300 pixels a pass: eight passes, the last one short
    # the stages by hand
    rays = device_rays(gpu_ctx, c.cam, rp)
    res = torch.zeros((n, 5), dtype=torch.float32, device=DEV)
    frame = torch.zeros((w * h, 5), dtype=torch.float32, device=DEV)
    words = torch.zeros((w * h,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st2 = c.sc.trace_dev(n, ptrs(rays) + [None], c.lights, tp, res.data_ptr())
    gpu_ctx.resolve_dev(w, h, samples, 0, w * h, res.data_ptr(), frame.data_ptr(), words.data_ptr())
    gpu_ctx.synchronize()
    img2, packed2 = frame.cpu().numpy().reshape(h, w, 5), words.cpu().numpy().view(np.uint32).reshape(h, w)
    assert img0.shape == (h, w, 5) and packed0.shape == (h, w)
    for img, packed in ((img1, packed1), (img2, packed2)):
        assert np.array_equal(img.view(np.uint32), img0.view(np.uint32)) and np.array_equal(packed, packed0)
    hit = img0[..., 4] < 1e6
    assert 0.05 < hit.mean() and len(np.unique(packed0)) > 100  # (a frame, not a blank)
    for st in (st0, st1, st2):
        assert (st["rays_primary"], st["rays_shadow"], st["rays_secondary"]) == (n, st0["rays_shadow"], st0["rays_secondary"])
    assert st0["rays_shadow"] > 0 and (name != "materials" or st0["rays_secondary"] > 0)
    assert st0["n_pixels"] == st1["n_pixels"] == 2345 and st0["kernel_ms"] > 0 and st1["kernel_ms"] > 0
    assert st1["n_tiles"] == 7 * ((1500 + 63) // 64) + (245 * 5 + 63) // 64
    # the device-pointer form, without statistics (asynchronous) and without the float frame
    frame.fill_(SENT); words.fill_(-77)
    torch.cuda.synchronize()
    assert c.sc.render_lens_dev(c.cam, c.lights, rp, tp, frame.data_ptr(), words.data_ptr(), rays_per_pass=4000, want_stats=False) is None
    gpu_ctx.synchronize()
    assert np.array_equal(frame.cpu().numpy().reshape(h, w, 5).view(np.uint32), img0.view(np.uint32))
    assert np.array_equal(words.cpu().numpy().view(np.uint32).reshape(h, w), packed0)
    words.fill_(-77)
    torch.cuda.synchronize()
    st = c.sc.render_lens_dev(c.cam, c.lights, rp, tp, None, words.data_ptr())
    assert np.array_equal(words.cpu().numpy().view(np.uint32).reshape(h, w), packed0) and st["rays_shadow"] == st0["rays_shadow"]
    img, packed, _ = c.sc.render_lens(c.cam, c.lights, rp, tp, want_packed=False)
    assert packed is None and np.array_equal(img.view(np.uint32), img0.view(np.uint32))


# ---------------------------------------------------------------- 8. refusals
def test_refused_arguments_fail_before_anything_is_launched(gpu_ctx, committed):
    c = committed("S1")
    lib, cam = gpu_ctx.lib, c.cam
    fp = lambda a: a.ctypes.data_as(L.c_fp)
    n = 67 * 35 * 5
    good = dict(width=67, height=35, samples=5, jitter=1, seed=2)
    cols = [np.full(n, SENT, np.float32) for _ in range(6)]
    dcols = ray_buffers(n, fill=SENT)

    def rays_refused(cam_, p, first=0, count=n, null=None, status=L.E_INVALID):
        a = [fp(x) for x in cols]
        d = [C.c_void_p(q) for q in ptrs(dcols)]
        if null is not None:
            a[null] = None; d[null] = None
        pp = C.byref(p) if p is not None else None
        cc = C.byref(cam_) if cam_ is not None else None
        assert lib.glome_camera_rays(gpu_ctx.h, cc, pp, first, count, *a) == status and gpu_ctx.err()
        assert lib.glome_camera_rays_dev(gpu_ctx.h, cc, pp, first, count, *d) == status

    bad_cam = api.camera_from_vectors(list(cam.pos), list(cam.fwd), list(cam.up), list(cam.right)); bad_cam.fwd[1] = float("inf")
    flat_cam = api.camera_from_vectors(list(cam.pos), list(cam.fwd), (0, 0, 0), list(cam.right))
    rays_refused(None, api.raygen_params(**good))
    rays_refused(cam, None)
    for k in range(6):
        rays_refused(cam, api.raygen_params(**good), null=k)
    for bad in (dict(width=0), dict(height=0), dict(width=-1), dict(samples=0), dict(samples=65), dict(lens=3), dict(lens=THIN, focus_dist=0.0),
                dict(lens=THIN, focus_dist=-1.0), dict(lens=THIN, aperture=-0.5, focus_dist=1.0), dict(aperture=float("nan")), dict(focus_dist=float("inf")),
                dict(lens=THIN, aperture=float("inf"), focus_dist=2.0)):
        rays_refused(cam, api.raygen_params(**{**good, **bad}), count=1)
    rays_refused(bad_cam, api.raygen_params(**good))
    rays_refused(flat_cam, api.raygen_params(lens=LATLONG, **good))  # (no up to measure the latitude against)
    for first, count in ((-1, 10), (0, n + 1), (n, 1), (5, -1), (n - 3, 4)):
        rays_refused(cam, api.raygen_params(**good), first=first, count=count)
    assert lib.glome_camera_rays(None, C.byref(cam), C.byref(api.raygen_params(**good)), 0, n, *[fp(x) for x in cols]) == L.E_INVALID

    # resolve
    src = torch.zeros((W * H * 5, 5), dtype=torch.float32, device=DEV)
    frame = torch.full((W * H, 5), SENT, dtype=torch.float32, device=DEV)
    words = torch.full((W * H,), -77, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    res = lambda w, h, s, first, count, a, b, d: lib.glome_resolve_dev(gpu_ctx.h, w, h, s, first, count, a, b, d)
    assert res(W, H, 5, 0, W * H, vp(src), None, None) == L.E_INVALID and "rgbad" in gpu_ctx.err()  # both outputs null
    assert res(W, H, 5, 0, W * H, None, vp(frame), vp(words)) == L.E_INVALID
    for w, h, s, first, count in ((0, H, 5, 0, 1), (W, 0, 5, 0, 1), (W, H, 0, 0, 1), (W, H, 65, 0, 1), (W, H, 5, -1, 2), (W, H, 5, 0, W * H + 1), (W, H, 5, W * H, 1), (W, H, 5, 3, -1)):
        assert res(w, h, s, first, count, vp(src), vp(frame), vp(words)) == L.E_INVALID, (w, h, s, first, count)
    assert lib.glome_resolve_dev(None, W, H, 5, 0, 1, vp(src), vp(frame), vp(words)) == L.E_INVALID

    # render_lens: the host form into small sentinel buffers it must not touch, the device form into the frames above
    la = (L.Light * len(c.lights))(*c.lights)
    tp = api.trace_params()
    img = np.full((H, W, 5), SENT, np.float32); pk = np.full((H, W), 77, np.uint32)

    def lens_refused(cam_, p, lights=la, nl=len(c.lights), tp_=tp, rpp=0, out=True, status=L.E_INVALID):
        cc = C.byref(cam_) if cam_ is not None else None
        pp = C.byref(p) if p is not None else None
        tt = C.byref(tp_) if tp_ is not None else None
        assert lib.glome_render_lens(c.sc.h, cc, pp, lights, nl, tt, rpp, fp(img) if out else None, pk.ctypes.data_as(L.c_up) if out else None, None) == status
        assert lib.glome_render_lens_dev(c.sc.h, cc, pp, lights, nl, tt, rpp, vp(frame) if out else None, vp(words) if out else None, None) == status

    lens_refused(None, api.raygen_params(**good))
    lens_refused(cam, None)
    lens_refused(cam, api.raygen_params(**good), tp_=None)
    lens_refused(cam, api.raygen_params(**good), out=False)
    lens_refused(cam, api.raygen_params(**good), nl=-1)
    lens_refused(cam, api.raygen_params(**good), lights=None, nl=1)
    lens_refused(cam, api.raygen_params(**good), rpp=-1)
    lens_refused(cam, api.raygen_params(**{**good, "samples": 65}))
    lens_refused(cam, api.raygen_params(**{**good, "lens": THIN, "focus_dist": 0.0}))
    lens_refused(bad_cam, api.raygen_params(**good))
    lens_refused(cam, api.raygen_params(width=32768, height=32768, samples=4))  # 2^32 rays; the frame itself is within glome_render's limit
    lens_refused(cam, api.raygen_params(width=65536, height=32768))             # 2^31 pixels: not a frame
    lens_refused(cam, api.raygen_params(**good), tp_=api.trace_params(maxdepth=9), status=L.E_LIMIT)
    lens_refused(cam, api.raygen_params(**good), lights=(L.Light * 17)(*([c.lights[0]] * 17)), nl=17, status=L.E_LIMIT)
    assert lib.glome_render_lens(None, C.byref(cam), C.byref(api.raygen_params(**good)), la, len(c.lights), C.byref(tp), 0, fp(img), None, None) == L.E_INVALID

    # nothing was launched, nothing written
    gpu_ctx.synchronize()
    assert all(np.all(x == SENT) for x in cols) and np.all(dcols.cpu().numpy() == SENT)
    assert np.all(frame.cpu().numpy() == SENT) and np.all(words.cpu().numpy() == -77) and np.all(img == SENT) and np.all(pk == 77)
    # and the context is as good as before
    o, d = gpu_ctx.camera_rays(cam, api.raygen_params(**good))
    assert o.shape == (n, 3) and unit_rule(d) <= 1e-5
    assert lib.glome_camera_rays(gpu_ctx.h, C.byref(cam), C.byref(api.raygen_params(**good)), n, 0, *[fp(x) for x in cols]) == 0  # an empty range at the end
    img2, _, st = c.sc.render_lens(cam, c.lights, api.raygen_params(**good))
    assert st["n_pixels"] == 67 * 35 and (img2[..., 4] < 1e6).any()
