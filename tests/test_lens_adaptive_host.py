"""CPU suite: the rule of glome_render_lens_adaptive on the host -- glome_adaptive_levels, glome_adaptive_fold, the params struct.
The rule is restated here in NumPy float32 from its text (include/glome_hip.h), by prefix sums instead of the library's streaming fold,
and the library is held to it bit for bit: on random pixels over every legal (base, max) and on crafted dyadic tuples whose sums are
exact, so that the comparison sits exactly on, or one ulp beyond, threshold * h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from glome_amd import _lib as L
from glome_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LEGAL = [(b, b << k) for b in range(2, 65, 2) for k in range(6) if (b << k) <= 64]


@pytest.fixture(scope="module")
def lib(built):
    return L.load()


# ---------------------------------------------------------------- the restatement
def seq_sum(x):
    """fp32 sum along axis 1 in index order, starting from a copy of element 0"""
    acc = x[:, 0].copy()
    for k in range(1, x.shape[1]):
        acc = acc + x[:, k]
    assert acc.dtype == F32
    return acc


def rgbf_np(r, g, b):
    """Glome.hs:98-110 on premultiplied channels: cap1, * 256, floor, to int32 (saturating, 0 for a NaN), a wrapping Word32 sum"""
    def ch(v):
        v = np.where(v >= 1, F32(1) - F32(0.0001), v).astype(F32)
        f = np.floor(v * F32(256))
        i = np.where(np.isnan(f), 0, np.clip(f, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
        return i & 0xffffffff
    return ((ch(r) * 65536 + ch(g) * 256 + ch(b)) & 0xffffffff).astype(np.uint32)


def resolve_np(x):
    """glome_resolve_dev's contract for samples = x.shape[1]: sequential sums, one correctly rounded division, the least depth by
    compare-select; the packed word"""
    mean = seq_sum(x[:, :, :4]) / F32(x.shape[1])
    d = x[:, 0, 4].copy()
    for k in range(1, x.shape[1]):
        d = np.where(x[:, k, 4] < d, x[:, k, 4], d)
    out = np.concatenate([mean, d[:, None]], axis=1).astype(F32)
    return out, rgbf_np(out[:, 0] * out[:, 3], out[:, 1] * out[:, 3], out[:, 2] * out[:, 3])


def model(x, base, thr):
    """the rule for every pixel of x[n, max, 5] at once: (counts, rgbad, packed)"""
    n, mx = x.shape[0], x.shape[1]
    thr = F32(thr)
    counts = np.zeros(n, np.int32)
    out = np.zeros((n, 5), F32)
    packed = np.zeros(n, np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        level = base
        while True:
            h = level // 2
            a = seq_sum(x[:, :h, :4])
            b = seq_sum(x[:, h:level, :4])
            stop = np.all(np.abs(a - b) <= thr * F32(h), axis=1) if level < mx else np.ones(n, bool)
            new = stop & (counts == 0)
            if new.any():
                counts[new] = level
                out[new], packed[new] = resolve_np(x[new][:, :level])
            if level == mx:
                break
            level *= 2
    return counts, out, packed


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check(x, base, thr):
    x = np.ascontiguousarray(x, F32)
    got = api.adaptive_fold(x, base, thr)
    want = model(x, base, thr)
    assert np.array_equal(got[0], want[0]), (base, x.shape[1], thr)
    assert same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]), (base, x.shape[1], thr)
    return got


# ---------------------------------------------------------------- the ABI
NAMES = ("glome_adaptive_params_default", "glome_adaptive_params_size", "glome_adaptive_levels", "glome_adaptive_fold", "glome_render_lens_adaptive",
         "glome_render_lens_adaptive_dev")


def test_the_library_exports_and_the_binding_binds_the_adaptive_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert all(n in exported for n in NAMES), [n for n in NAMES if n not in exported]
    declared = {name for name, _, _ in L.SYMBOLS}
    assert all(n in declared and getattr(lib, n).argtypes is not None for n in NAMES)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(('"%s"' % n) in text for n in NAMES if n != "glome_adaptive_params_size")  # (the guide's foreign imports)


def test_default_params_and_struct_size(lib):
    p = L.AdaptiveParams()
    C.memset(C.byref(p), 0xff, C.sizeof(p))
    lib.glome_adaptive_params_default(C.byref(p))
    assert (p.base_samples, p.threshold) == (4, 1.0 / 64)
    assert C.sizeof(L.AdaptiveParams) == lib.glome_adaptive_params_size() == 8
    lib.glome_adaptive_params_default(None)  # (a null pointer is ignored, like the other defaults)
    q = api.adaptive_params(base_samples=2, threshold=0.5)
    assert (q.base_samples, q.threshold) == (2, 0.5)
    assert (api.adaptive_params().base_samples, api.adaptive_params().threshold) == (4, 1.0 / 64)


# ---------------------------------------------------------------- the levels
def test_the_legal_levels_are_exactly_the_stated_set(lib):
    legal = set(LEGAL)
    assert len(legal) == 63 and (2, 64) in legal and (64, 64) in legal and (6, 48) in legal
    out = (C.c_int32 * 8)()
    for base in range(-2, 66):
        for mx in range(-2, 66):
            n = lib.glome_adaptive_levels(base, mx, out, 8)
            if (base, mx) in legal:
                want = [base << k for k in range(7) if (base << k) <= mx]
                assert n == len(want) <= 6 and list(out[:n]) == want and want[-1] == mx, (base, mx)
                assert api.adaptive_levels(base, mx) == want
            else:
                assert n == L.E_INVALID, (base, mx)
    # a short buffer gets the first levels, the count is the whole list's; no buffer at all asks for the count
    for k in range(8):
        out[k] = -7
    assert lib.glome_adaptive_levels(2, 64, out, 2) == 6 and list(out) == [2, 4, -7, -7, -7, -7, -7, -7]
    assert lib.glome_adaptive_levels(2, 64, None, 0) == 6
    assert lib.glome_adaptive_levels(2, 64, None, 1) == L.E_INVALID and lib.glome_adaptive_levels(2, 64, out, -1) == L.E_INVALID
    with pytest.raises(ValueError):
        api.adaptive_levels(3, 6)


# ---------------------------------------------------------------- random pixels
def random_tuples(rng, n, mx):
    """colours in [0, 2) (beyond cap1) whose samples agree, differ a little or differ a lot, pixel by pixel; depths a mix of misses and hits"""
    centre = rng.uniform(0, 2, size=(n, 1, 4))
    spread = rng.choice([0.0, 1e-3, 0.02, 0.1, 0.5], size=(n, 1, 1))
    x = np.empty((n, mx, 5), F32)
    x[..., :4] = np.abs(centre + spread * rng.normal(size=(n, mx, 4)))
    x[..., 4] = np.where(rng.uniform(size=(n, mx)) < 0.4, 1e6, rng.uniform(0.5, 40, size=(n, mx)))
    return x


def test_fold_equals_the_float32_model_on_random_pixels(lib):
    """64 pixels for each of the 63 legal pairs, at three thresholds: some four thousand pixels a threshold"""
    rng = np.random.default_rng(23)
    seen = set()
    for base, mx in LEGAL:
        x = random_tuples(rng, 64, mx)
        for thr in (1.0 / 64, 0.05, 0.0):
            counts, out, packed = check(x, base, thr)
            seen.update((base, mx, int(c)) for c in counts)
            assert set(counts) <= set(api.adaptive_levels(base, mx))
            # whatever the count, the pixel is the fixed frame's at samples = count
            for c in set(counts):
                m = counts == c
                want, want_packed = resolve_np(x[m][:, :c])
                assert same_bits(out[m], want) and np.array_equal(packed[m], want_packed)
                assert np.array_equal(out[m][:, 4], x[m][:, :c, 4].min(axis=1))
    assert all((2, 64, c) in seen for c in (2, 4, 8, 16, 32, 64))  # every level was somebody's count
    assert all((4, 16, c) in seen for c in (4, 8, 16))


# ---------------------------------------------------------------- crafted tuples: every sum exact
def tuples_of(colours, depth=3.0):
    """[max, 5] from a list of per-sample grey values (all four channels equal)"""
    x = np.zeros((len(colours), 5), F32)
    x[:, :4] = np.asarray(colours, F32)[:, None]
    x[:, 4] = depth
    return x


def fold1(x, base, thr):
    counts, out, packed = check(x[None], base, thr)
    return int(counts[0]), out[0], int(packed[0])


def test_equal_samples_stop_at_base(lib):
    for base, mx in LEGAL:
        c, out, packed = fold1(tuples_of([0.25] * mx), base, 0.0)  # (|A - B| = 0 <= 0 * h)
        assert c == base and np.array_equal(out, np.array([0.25, 0.25, 0.25, 0.25, 3.0], F32)) and packed == 0x101010


def test_a_difference_in_the_second_half_only_continues_one_level(lib):
    # level 4: A = 0.5, B = 1.0, |A - B| = 0.5 > 2 / 64; level 8: A = 1.5 = B; samples 8.. are never looked at
    x = tuples_of([0.25, 0.25, 0.5, 0.5, 0.375, 0.375, 0.375, 0.375] + [7.0] * 8)
    c, out, _ = fold1(x, 4, 1.0 / 64)
    assert c == 8 and out[0] == F32(3.0 / 8)
    # the difference in one channel alone is enough, whichever it is
    for ch in range(4):
        y = tuples_of([0.25] * 16)
        y[3, ch] = 0.75
        assert fold1(y, 4, 1.0 / 64)[0] == 16 and fold1(y, 4, 0.25)[0] == 4  # (|0.5 - 1.0| = 0.5 = 0.25 * 2 at level 4)
    # depth takes no part in the test
    y = tuples_of([0.25] * 16)
    y[:, 4] = np.arange(16, 0, -1)
    c, out, _ = fold1(y, 4, 0.0)
    assert c == 4 and out[4] == 13.0


def test_the_comparison_is_less_or_equal_to_the_ulp(lib):
    thr = F32(1.0 / 64)
    lim = thr * F32(2)  # base 4: h = 2
    on = tuples_of([0, 0, 0, lim] + [0] * 12)
    beyond = tuples_of([0, 0, 0, np.nextafter(lim, F32(1))] + [0] * 12)
    assert fold1(on, 4, thr)[0] == 4
    assert fold1(beyond, 4, thr)[0] > 4
    # the same on the other side (A larger than B), and at the second level (h = 4: threshold * 4)
    assert fold1(tuples_of([0, lim, 0, 0] + [0] * 12), 4, thr)[0] == 4
    assert fold1(tuples_of([0, np.nextafter(lim, F32(1)), 0, 0] + [0] * 12), 4, thr)[0] > 4
    lim4 = thr * F32(4)
    assert fold1(tuples_of([0, 0, 0, 1, 1 + lim4, 0, 0, 0] + [9.0] * 8), 4, thr)[0] == 8
    assert fold1(tuples_of([0, 0, 0, 1, np.nextafter(1 + lim4, F32(2)), 0, 0, 0] + [0.0] * 8), 4, thr)[0] == 16


def test_a_nan_sample_runs_to_max(lib):
    for base, mx in ((2, 64), (4, 16), (6, 24)):
        x = tuples_of([0.25] * mx)
        x[0, 1] = np.nan
        for thr in (0.0, 1.0 / 64, np.inf):
            c, out, packed = fold1(x, base, thr)
            assert c == mx and np.isnan(out[1]) and out[0] == 0.25
            assert packed == 0x100010  # (the NaN channel converts to 0)
    # a NaN the stopped pixel never saw does not matter
    x = tuples_of([0.25] * 16)
    x[5, 2] = np.nan
    assert fold1(x, 4, 1.0 / 64)[0] == 4


def test_base_equal_to_max_and_the_two_ends_of_the_threshold(lib):
    rng = np.random.default_rng(5)
    x = random_tuples(rng, 200, 16)
    x[..., :4] += rng.uniform(0, 0.5, size=(200, 16, 4)).astype(F32)  # (no pixel's samples all alike)
    for thr in (0.0, 1.0 / 64, np.inf):
        counts, out, _ = check(x, 16, thr)  # base == max: the fixed frame
        assert np.all(counts == 16) and same_bits(out, resolve_np(x)[0])
    counts, out, _ = check(x, 4, np.inf)     # every pixel stops at base
    assert np.all(counts == 4) and same_bits(out, resolve_np(x[:, :4])[0])
    counts, _, _ = check(x, 4, 0.0)          # only exact agreement stops a pixel
    assert np.all(counts == 16)
    x[::2] = x[::2, :1]                      # (every sample of every other pixel the same)
    counts, _, _ = check(x, 4, 0.0)
    assert np.all(counts[::2] == 4) and np.all(counts[1::2] == 16)


# ---------------------------------------------------------------- refusals
def test_the_host_functions_refuse_bad_arguments(lib):
    x = np.full((16, 5), 0.25, F32)
    cnt, out, word = C.c_int32(-7), (C.c_float * 5)(*([-7.5] * 5)), C.c_uint32(77)
    fp = x.ctypes.data_as(L.c_fp)
    fold = lambda t=fp, base=4, mx=16, thr=1.0 / 64, c=C.byref(cnt), o=out, w=C.byref(word): lib.glome_adaptive_fold(t, base, mx, thr, c, o, w)
    assert fold(t=None) == L.E_INVALID and fold(c=None) == L.E_INVALID and fold(o=None) == L.E_INVALID and fold(w=None) == L.E_INVALID
    for base, mx in ((0, 16), (3, 12), (4, 12), (4, 2), (-4, 16), (2, 128), (66, 66), (4, 0)):
        assert fold(base=base, mx=mx) == L.E_INVALID, (base, mx)
    for thr in (float("nan"), -1.0, -1e-30, float("-inf")):
        assert fold(thr=thr) == L.E_INVALID, thr
    assert (cnt.value, list(out), word.value) == (-7, [-7.5] * 5, 77)  # nothing was written
    assert fold(thr=float("inf")) == 0 and cnt.value == 4
    assert fold(thr=0.0) == 0 and cnt.value == 4 and list(out) == [0.25] * 5 and word.value == 0x101010
    with pytest.raises(ValueError):
        api.adaptive_fold(x, 4, -1.0)
    with pytest.raises(ValueError):
        api.adaptive_fold(x[:, :4], 4, 0.0)
