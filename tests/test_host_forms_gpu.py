"""GPU suite (-m gpu): the host-buffer forms of the ray seams and of the frame -- glome_rayint_batch, glome_shadow_batch,
glome_inside_batch, glome_render -- as plumbing: what they refuse before anything is staged, which outputs they write, and that they
answer what their device-pointer forms answer.  What the seams compute is held to the oracle elsewhere (test_gpu_parity.py); the trace
and lens forms have files of their own (test_trace_batch.py, test_trace_work.py, test_lens_gpu.py, test_lens_adaptive_gpu.py).

Scene S1, 65 rays (a full wave and a tail of one) and a 9 x 7 frame.  Every refusal here is decided on the host, before a launch."""
import ctypes as C

import numpy as np
import pytest

from helpers import product_camera_lights, random_rays
from glome_amd import _lib as L
from glome_amd import api, scenes

pytestmark = pytest.mark.gpu

N = 65
F32_SENTINEL, I32_SENTINEL, U8_SENTINEL, PACKED_SENTINEL = np.float32(-7.5), -77, 0xA5, 0xDEADBEEF
W, H, BLOCK = 9, 7, 4


class S1:
    def __init__(self, ctx):
        self.ctx = ctx
        self.sd = scenes.s1(nlights=2)
        self.b = api.Builder()
        nm, _ = self.sd.replay(self.b)
        self.sc = ctx.commit(self.b, nm[self.sd.root])
        self.lib = self.sc.lib
        self.cam, self.lights = product_camera_lights(self.sd)
        ro, rd = random_rays(N, 5)
        self.cols = [np.ascontiguousarray(a) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2], np.full(N, 30.0, np.float32))]
        # points for `inside`: the spheres' centres (x, 0.5, z), and points well above them
        g = np.arange(N, dtype=np.float32)
        self.pts = [np.ascontiguousarray(a) for a in (g % 11 - 5, np.where(g % 2 == 0, 0.5, 3.0).astype(np.float32), (g // 11) % 11 - 5)]
        # the all-outputs runs, made once and never written to
        rc, self.hit = self.rayint(range(6))
        assert rc == 0, ctx.err()
        self.occ = np.full(N + 1, U8_SENTINEL, np.uint8)
        assert self.lib.glome_shadow_batch(self.sc.h, N, *[fp(a) for a in self.cols], bp(self.occ)) == 0, ctx.err()
        self.ins = np.full(N + 1, U8_SENTINEL, np.uint8)
        assert self.lib.glome_inside_batch(self.sc.h, N, *[fp(a) for a in self.pts], bp(self.ins)) == 0, ctx.err()
        for a in self.hit + [self.occ, self.ins]:
            a.setflags(write=False)

    def rayint(self, wanted, cols=None):
        """glome_rayint_batch into sentinel-filled buffers one row longer than N; only the outputs named in `wanted` are passed"""
        out = hit_buffers()
        ptrs = [as_ptr(a) if k in wanted else None for k, a in enumerate(out)]
        cols = self.cols if cols is None else cols
        return self.lib.glome_rayint_batch(self.sc.h, N, *[fp(a) if a is not None else None for a in cols], *ptrs), out


def fp(a):
    return a.ctypes.data_as(L.c_fp)


def bp(a):
    return a.ctypes.data_as(L.c_bp)


def as_ptr(a):
    return a.ctypes.data_as(L.c_ip if a.dtype == np.int32 else L.c_fp)


def hit_buffers():
    """t, prim, nx, ny, nz, tex8: N + 1 rows of sentinels"""
    f = lambda: np.full(N + 1, F32_SENTINEL, np.float32)
    return [f(), np.full(N + 1, I32_SENTINEL, np.int32), f(), f(), f(), np.full((N + 1, 8), I32_SENTINEL, np.int32)]


def untouched(a):
    s = {np.dtype(np.float32): F32_SENTINEL, np.dtype(np.int32): I32_SENTINEL, np.dtype(np.uint8): U8_SENTINEL, np.dtype(np.uint32): PACKED_SENTINEL}[a.dtype]
    return bool(np.all(a == s))


@pytest.fixture(scope="module")
def s1(gpu_ctx):
    c = S1(gpu_ctx)
    yield c
    c.sc.release()


# ---------------------------------------------------------------- 1. null streams, n = 0, a null scene
def test_the_inputs_are_not_trivial(s1):
    t, prim = s1.hit[0][:N], s1.hit[1][:N]
    assert 0 < (t >= 0).sum() < N and np.array_equal(t >= 0, prim >= 0)
    assert 0 < s1.occ[:N].sum() < N and set(np.unique(s1.occ[:N])) == {0, 1}
    assert 0 < s1.ins[:N].sum() < N and set(np.unique(s1.ins[:N])) == {0, 1}
    assert all(untouched(a[N:]) for a in s1.hit + [s1.occ, s1.ins])  # nothing is written past row N


def test_rayint_refuses_a_null_ray_stream(s1):
    for k in range(7):
        cols = list(s1.cols)
        cols[k] = None
        rc, out = s1.rayint(range(6), cols)
        assert rc == L.E_INVALID and "null" in s1.ctx.err(), (k, rc, s1.ctx.err())
        assert all(untouched(a) for a in out), k
    lib = s1.lib
    assert lib.glome_rayint_batch(s1.sc.h, 0, *[None] * 13) == 0
    out = hit_buffers()
    assert lib.glome_rayint_batch(None, N, *[fp(a) for a in s1.cols], *[as_ptr(a) for a in out]) == L.E_INVALID
    assert all(untouched(a) for a in out)
    s1.ctx.synchronize()


def test_shadow_refuses_a_null_stream(s1):
    lib = s1.lib
    for k in range(8):
        occ = np.full(N + 1, U8_SENTINEL, np.uint8)
        args = [fp(a) for a in s1.cols] + [bp(occ)]
        args[k] = None
        rc = lib.glome_shadow_batch(s1.sc.h, N, *args)
        assert rc == L.E_INVALID and "null" in s1.ctx.err(), (k, rc, s1.ctx.err())
        assert untouched(occ), k
    assert lib.glome_shadow_batch(s1.sc.h, 0, *[None] * 8) == 0
    occ = np.full(N + 1, U8_SENTINEL, np.uint8)
    assert lib.glome_shadow_batch(None, N, *[fp(a) for a in s1.cols], bp(occ)) == L.E_INVALID and untouched(occ)
    s1.ctx.synchronize()


def test_inside_refuses_a_null_stream(s1):
    lib = s1.lib
    for k in range(4):
        ins = np.full(N + 1, U8_SENTINEL, np.uint8)
        args = [fp(a) for a in s1.pts] + [bp(ins)]
        args[k] = None
        rc = lib.glome_inside_batch(s1.sc.h, N, *args)
        assert rc == L.E_INVALID and "null" in s1.ctx.err(), (k, rc, s1.ctx.err())
        assert untouched(ins), k
    assert lib.glome_inside_batch(s1.sc.h, 0, None, None, None, None) == 0
    ins = np.full(N + 1, U8_SENTINEL, np.uint8)
    assert lib.glome_inside_batch(None, N, *[fp(a) for a in s1.pts], bp(ins)) == L.E_INVALID and untouched(ins)
    s1.ctx.synchronize()


# ---------------------------------------------------------------- 2. rayint's optional outputs
@pytest.mark.parametrize("k", range(6), ids=["t", "prim", "nx", "ny", "nz", "tex8"])
def test_rayint_with_one_output_alone(s1, k):
    """An output that is not wanted is null: the one that is wanted holds the bits of the all-outputs run, the others are not written."""
    rc, out = s1.rayint([k])
    assert rc == 0, s1.ctx.err()
    assert np.array_equal(out[k], s1.hit[k])  # (row N included: the sentinel)
    assert all(untouched(a) for j, a in enumerate(out) if j != k)


# ---------------------------------------------------------------- 3. the frame's host form
def owned_mask(first, stride):
    """pixels of the tiles (first, stride) owns in renderTiles' order: x chunks outer, y chunks inner, the last chunk the remainder"""
    def chunks(size):
        out, pos = [], 0
        while pos + BLOCK < size:
            out.append((pos, BLOCK)); pos += BLOCK
        return out + [(pos, size - pos)]
    m = np.zeros((H, W), bool)
    k = 0
    for x, w in chunks(W):
        for y, h in chunks(H):
            if k >= first and (k - first) % stride == 0:
                m[y:y + h, x:x + w] = True
            k += 1
    return m


def render_into_sentinels(s1, P, want_rgbad=True, want_packed=True):
    img = np.full((H, W, 5), F32_SENTINEL, np.float32)
    packed = np.full((H, W), PACKED_SENTINEL, np.uint32)
    la = (L.Light * len(s1.lights))(*s1.lights)
    st = L.Stats()
    rc = s1.lib.glome_render(s1.sc.h, C.byref(s1.cam), la, len(s1.lights), C.byref(P), fp(img) if want_rgbad else None,
                             packed.ctypes.data_as(L.c_up) if want_packed else None, C.byref(st))
    return rc, img, packed, st


def test_render_keeps_the_pixels_of_tiles_it_does_not_own(s1):
    rc, full, full_packed, st = render_into_sentinels(s1, api.render_params(width=W, height=H, blocksize=BLOCK, maxdepth=3))
    assert rc == 0 and st.n_pixels == W * H, s1.ctx.err()
    assert not np.any(full == F32_SENTINEL) and not np.any(full_packed == PACKED_SENTINEL)
    mine = owned_mask(1, 2)
    assert 0 < mine.sum() < W * H and np.array_equal(mine | owned_mask(0, 2), np.ones((H, W), bool))
    P = api.render_params(width=W, height=H, blocksize=BLOCK, maxdepth=3, tile_first=1, tile_stride=2)
    rc, img, packed, st = render_into_sentinels(s1, P)
    assert rc == 0 and st.n_pixels == mine.sum() and st.n_tiles == 3, s1.ctx.err()
    assert untouched(img[~mine]) and untouched(packed[~mine])
    assert np.array_equal(img[mine], full[mine]) and np.array_equal(packed[mine], full_packed[mine])
    # packed is optional
    rc, img, packed, _ = render_into_sentinels(s1, P, want_packed=False)
    assert rc == 0, s1.ctx.err()
    assert untouched(img[~mine]) and np.array_equal(img[mine], full[mine]) and untouched(packed)


def test_render_refuses_a_null_framebuffer(s1):
    rc, img, packed, _ = render_into_sentinels(s1, api.render_params(width=W, height=H, blocksize=BLOCK), want_rgbad=False)
    assert rc == L.E_INVALID and "null framebuffer" in s1.ctx.err()
    assert untouched(packed)
    s1.ctx.synchronize()


# ---------------------------------------------------------------- 4. host form against device-pointer form
def test_device_pointer_forms_equal_the_host_forms(s1):
    import torch
    dev = torch.device("cuda:0")
    cols = [torch.tensor(a, device=dev) for a in s1.cols]
    out = [torch.tensor(a, device=dev) for a in hit_buffers()]
    occ = torch.full((N + 1,), U8_SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ptrs = [C.c_void_p(c.data_ptr()) for c in cols]
    assert s1.lib.glome_rayint_batch_dev(s1.sc.h, N, *ptrs, *[C.c_void_p(a.data_ptr()) for a in out]) == 0, s1.ctx.err()
    assert s1.lib.glome_shadow_batch_dev(s1.sc.h, N, *ptrs, C.c_void_p(occ.data_ptr())) == 0, s1.ctx.err()
    s1.ctx.synchronize()
    for got, want in zip(out, s1.hit):
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(occ.cpu().numpy(), s1.occ)
