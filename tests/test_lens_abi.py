"""CPU suite: the ABI of the trace seam's lens stages (glome_raygen_*, glome_camera_rays, glome_resolve_dev, glome_render_lens) -- the
symbols, the params struct, the ray count, the sample words --, and the restatement the GPU suite (test_lens_gpu.py) checks the device
rays against: the three lenses and the sample words written from their formulas (include/glome_hip.h), in NumPy, for any dtype.
Evaluated in float32 it stays well inside the bounds the GPU suite holds the kernel to: a correct fp32 implementation can meet them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINHOLE, THIN, LATLONG = 0, 1, 2


# ---------------------------------------------------------------- the restatement
def mix(x):
    x = np.asarray(x, np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def sample_words(seed, pixel, s, dim):
    """mix(mix(mix(seed + 0x9e3779b9 * (pixel + 1)) + s) + dim) in uint32 arithmetic, elementwise"""
    seed, pixel, s, dim = (np.asarray(v, np.uint32) for v in (seed, pixel, s, dim))
    with np.errstate(over="ignore"):
        return mix(mix(mix(seed + np.uint32(0x9e3779b9) * (pixel + np.uint32(1))) + s) + dim)


def library_words(seed, pixel, s, dim):
    """the same words from glome_raygen_sample, one call per element"""
    f = L.load().glome_raygen_sample
    pixel, s = np.broadcast_arrays(np.asarray(pixel), np.asarray(s))
    return np.array([f(int(seed), int(p), int(k), int(dim)) for p, k in zip(pixel.ravel(), s.ravel())], np.uint32).reshape(pixel.shape)


def unit(words, dt):
    return (words >> np.uint32(8)).astype(dt) * dt(2.0 ** -24)


def vnorm(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def lens_rays(cam, w, h, lens, samples=1, jitter=0, seed=0, aperture=0.0, focus_dist=1.0, dt=np.float64, words=sample_words, first=0, n=None):
    """(o, d) of rays first .. first + n - 1 of the frame's order (y * w + x) * samples + s, every operation in dtype dt"""
    n = w * h * samples - first if n is None else n
    i = np.arange(first, first + n, dtype=np.int64)
    pixel, s = i // samples, i % samples
    x, y = (pixel % w).astype(dt), (pixel // w).astype(dt)
    if jitter:
        x = x + unit(words(seed, pixel, s, 0), dt)
        y = y + unit(words(seed, pixel, s, 1), dt)
    wf, hf, one, two = dt(w), dt(h), dt(1), dt(2)
    xc = ((x / wf) * two - one) * (wf / hf)
    yc = -((y / hf) * two - one)
    pos, fwd, up, right = (np.array(list(v), dt) for v in (cam.pos, cam.fwd, cam.up, cam.right))
    dp = vnorm(fwd + right * (-xc[:, None]) + up * yc[:, None])
    if lens == PINHOLE:
        return np.broadcast_to(pos, dp.shape).copy(), dp
    fh, rh, uh = vnorm(fwd), vnorm(right), vnorm(up)
    pi = dt(np.pi)
    if lens == THIN:
        u2, u3 = unit(words(seed, pixel, s, 2), dt), unit(words(seed, pixel, s, 3), dt)
        P = pos + dp * (dt(focus_dist) / (dp * fh).sum(-1))[:, None]
        ang = two * pi * u3
        Lp = pos + (dt(aperture) * np.sqrt(u2))[:, None] * (np.cos(ang)[:, None] * rh + np.sin(ang)[:, None] * uh)
        return Lp, vnorm(P - Lp)
    lam = pi * ((x / wf) * two - one)
    beta = (pi / two) * yc
    d = np.cos(beta)[:, None] * (np.cos(lam)[:, None] * fh - np.sin(lam)[:, None] * rh) + np.sin(beta)[:, None] * uh
    return np.broadcast_to(pos, d.shape).copy(), vnorm(d)


def cameras():
    """the GPU suite's two views: S1's camera and an axis-aligned one (fwd = (0, 0, 1))"""
    return {"S1": api.camera(*scenes.s1().cam), "axis": api.camera_from_vectors((0.5, 1.0, -6.0), (0, 0, 1), (0, 0.4, 0), (0.4, 0, 0))}


def scale_of(cam, aperture=0.0, focus_dist=0.0):
    return max(1.0, max(abs(float(v)) for v in cam.pos), aperture, focus_dist)


THIN_KW = dict(aperture=0.3, focus_dist=14.0)  # (the GPU suite's thin lens)


# ---------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib(built):
    return L.load()


def test_the_library_exports_and_the_binding_binds_the_lens_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    names = ("glome_raygen_params_default", "glome_raygen_params_size", "glome_raygen_count", "glome_raygen_sample", "glome_camera_rays_dev", "glome_camera_rays",
             "glome_resolve_dev", "glome_render_lens", "glome_render_lens_dev")
    assert all(n in exported for n in names), [n for n in names if n not in exported]
    declared = {name for name, _, _ in L.SYMBOLS}
    assert all(n in declared and getattr(lib, n).argtypes is not None for n in names)
    assert (api.LENS_PINHOLE, api.LENS_THIN, api.LENS_LATLONG) == (0, 1, 2)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(('"%s"' % n) in text for n in names if n != "glome_raygen_params_size")  # (the guide's foreign imports)


def test_default_params_and_struct_size(lib):
    p = L.RaygenParams()
    C.memset(C.byref(p), 0xff, C.sizeof(p))
    lib.glome_raygen_params_default(C.byref(p))
    assert (p.width, p.height, p.lens, p.samples, p.jitter, p.seed, p.aperture, p.focus_dist) == (720, 480, 0, 1, 0, 0, 0.0, 1.0)
    assert C.sizeof(L.RaygenParams) == lib.glome_raygen_params_size() == 32
    q = api.raygen_params(width=67, height=35, lens=api.LENS_THIN, samples=5, jitter=1, seed=9, aperture=0.25, focus_dist=3.0)
    assert (q.width, q.height, q.lens, q.samples, q.jitter, q.seed, q.aperture, q.focus_dist) == (67, 35, 1, 5, 1, 9, 0.25, 3.0)


def test_raygen_count(lib):
    count = lambda **kw: lib.glome_raygen_count(C.byref(api.raygen_params(**kw)))
    assert count(width=67, height=35, samples=5) == 11725
    assert count(width=67, height=35, samples=64) == 67 * 35 * 64 and count(width=1, height=1) == 1
    for bad in (dict(samples=0), dict(samples=65), dict(width=0), dict(height=0), dict(height=-3), dict(lens=3), dict(lens=-1),
                dict(lens=THIN, focus_dist=0.0), dict(lens=THIN, aperture=-0.1), dict(aperture=float("nan")), dict(focus_dist=float("inf"))):
        assert count(**bad) == L.E_INVALID, bad
    assert lib.glome_raygen_count(None) == L.E_INVALID
    assert count(lens=PINHOLE, focus_dist=-1.0) == 720 * 480  # (the thin lens's fields bind the thin lens only)


def test_sample_words_are_the_stated_mixer(lib):
    rng = np.random.default_rng(5)
    n = 10000
    seed, pixel = rng.integers(0, 2 ** 32, n, dtype=np.uint64), rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    s, dim = rng.integers(0, 64, n, dtype=np.uint64), rng.integers(0, 4, n, dtype=np.uint64)
    seed[:4] = 0xffffffff; pixel[:2] = 2 ** 31 - 1; pixel[2:6] = 2 ** 31 - 1; seed[6] = 0; pixel[6] = 0xffffffff  # wrap-around
    got = np.array([lib.glome_raygen_sample(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(seed, pixel, s, dim)], np.uint32)
    want = sample_words(seed.astype(np.uint32), pixel.astype(np.uint32), s.astype(np.uint32), dim.astype(np.uint32))
    assert np.array_equal(got, want)
    assert api.raygen_sample(int(seed[9]), int(pixel[9]), int(s[9]), int(dim[9])) == int(want[9])
    # one value by hand, in Python integers
    def mix1(x):
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff; x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff; x ^= x >> 16
        return x
    assert lib.glome_raygen_sample(7, 1234, 3, 2) == mix1((mix1((mix1((7 + 0x9e3779b9 * 1235) & 0xffffffff) + 3) & 0xffffffff) + 2) & 0xffffffff)
    u = unit(got, np.float32)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    assert float(unit(np.array([0xffffffff], np.uint32), np.float32)[0]) < 1.0
    u0 = unit(library_words(0, np.arange(65536), 0, 0), np.float64)
    assert abs(u0.mean() - 0.5) <= 0.01, u0.mean()  # (a uniform variable's standard error here is 0.0011)


# ---------------------------------------------------------------- the bounds are reachable in fp32
@pytest.mark.parametrize("cam_name", ["S1", "axis"])
def test_float32_restatement_stays_well_inside_the_gpu_bounds(lib, cam_name):
    """The GPU suite's cameras and sizes: the formulas in float32 against the same in float64, with at least half of each bound to spare."""
    cam = cameras()[cam_name]
    o32, d32 = lens_rays(cam, 67, 35, PINHOLE, dt=np.float32)
    o64, d64 = lens_rays(cam, 67, 35, PINHOLE)
    e = np.abs(d32 - d64).max()
    print("pinhole fp32 error", cam_name, e)
    assert np.array_equal(o32, np.broadcast_to(np.array(list(cam.pos), np.float32), o32.shape)) and e <= 0.5e-6
    assert np.abs((d32.astype(np.float64) ** 2).sum(1) - 1).max() <= 0.5e-5
    for lens in (THIN, LATLONG):
        for seed in (1, 0xdeadbeef):
            kw = dict(samples=5, jitter=1, seed=seed, words=library_words, **(THIN_KW if lens == THIN else {}))
            o32, d32 = lens_rays(cam, 33, 17, lens, dt=np.float32, **kw)
            o64, d64 = lens_rays(cam, 33, 17, lens, **kw)
            bound = 1e-5 * scale_of(cam, **(THIN_KW if lens == THIN else {}))
            eo, ed = np.abs(o32 - o64).max(), np.abs(d32 - d64).max()
            print("lens", lens, cam_name, seed, "fp32 error o, d:", eo, ed, "bound", bound)
            assert eo <= 0.5 * bound and ed <= 0.5 * bound
            assert np.abs((d32.astype(np.float64) ** 2).sum(1) - 1).max() <= 0.5e-5
    # a thin lens without an aperture is the pinhole of the same jitter
    kw = dict(samples=5, jitter=1, seed=1, words=library_words)
    _, dp = lens_rays(cam, 33, 17, PINHOLE, dt=np.float32, **kw)
    _, dt_ = lens_rays(cam, 33, 17, THIN, dt=np.float32, aperture=0.0, focus_dist=14.0, **kw)
    assert np.abs(dp - dt_).max() <= 0.5e-6
