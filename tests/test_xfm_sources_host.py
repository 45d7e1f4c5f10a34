"""The host functions that specify glome_scene_instance_update_from: glome_xfm_from_pose, glome_xfm_from_forward, glome_xfm_mult and the
getter glome_sb_instance_transform.  glome_hip.h states their arithmetic operation by operation; this file restates it with scalar
np.float64 operations in the stated order (every one a single round-to-nearest fp64 operation, nothing fused) and holds the library to
it bit for bit.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import instances_refit as IR
from glome_amd import _lib as L
from glome_amd import api

F = np.float64
ONE, TWO = F(1.0), F(2.0)


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


# ---- the restatement ----
def inverse_column(i, t):
    """i[r][3] = -(((i[r][0] tx) + (i[r][1] ty)) + (i[r][2] tz))"""
    return [-(((i[r][0] * t[0]) + (i[r][1] * t[1])) + (i[r][2] * t[2])) for r in range(3)]


def flat(fwd, inv, t, col):
    return np.array([v for r in range(3) for v in (*fwd[r], t[r])] + [v for r in range(3) for v in (*inv[r], col[r])], dtype=np.float64)


def np_from_pose(t, q, s):
    t, (qx, qy, qz, qw), s = [F(v) for v in t], [F(v) for v in q], F(s)
    inv = ONE / np.sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
    x, y, z, w = qx * inv, qy * inv, qz * inv, qw * inv
    xx, yy, zz, xy, xz, yz, xw, yw, zw = x * x, y * y, z * z, x * y, x * z, y * z, x * w, y * w, z * w
    R = [[ONE - TWO * (yy + zz), TWO * (xy - zw), TWO * (xz + yw)],
         [TWO * (xy + zw), ONE - TWO * (xx + zz), TWO * (yz - xw)],
         [TWO * (xz - yw), TWO * (yz + xw), ONE - TWO * (xx + yy)]]
    fwd = [[s * R[r][c] for c in range(3)] for r in range(3)]
    inv3 = [[R[c][r] / s for c in range(3)] for r in range(3)]
    return flat(fwd, inv3, t, inverse_column(inv3, t))


def np_from_forward(m):
    a = [[F(m[4 * r + c]) for c in range(3)] for r in range(3)]
    t = [F(m[4 * r + 3]) for r in range(3)]
    c = [[a[1][1] * a[2][2] - a[1][2] * a[2][1], a[1][2] * a[2][0] - a[1][0] * a[2][2], a[1][0] * a[2][1] - a[1][1] * a[2][0]],
         [a[0][2] * a[2][1] - a[0][1] * a[2][2], a[0][0] * a[2][2] - a[0][2] * a[2][0], a[0][1] * a[2][0] - a[0][0] * a[2][1]],
         [a[0][1] * a[1][2] - a[0][2] * a[1][1], a[0][2] * a[1][0] - a[0][0] * a[1][2], a[0][0] * a[1][1] - a[0][1] * a[1][0]]]
    det = ((a[0][0] * c[0][0]) + (a[0][1] * c[0][1])) + (a[0][2] * c[0][2])
    inv3 = [[c[k][r] / det for k in range(3)] for r in range(3)]
    return flat(a, inv3, t, inverse_column(inv3, t))


def np_mmul(A, B):
    """mmul of host_graph.hpp (mat_mult, Vec.hs:426-443)"""
    A, B = [F(v) for v in A], [F(v) for v in B]
    o = []
    for r in range(3):
        a = A[4 * r:4 * r + 4]
        o += [(a[0] * B[k] + a[1] * B[4 + k]) + a[2] * B[8 + k] for k in range(3)]
        o.append(((a[0] * B[3] + a[1] * B[7]) + a[2] * B[11]) + a[3])
    return o


def np_mult(a, b):
    """a applied after b: Xf{ mmul(a.f, b.f), mmul(b.i, a.i) }"""
    return np.array(np_mmul(a[:12], b[:12]) + np_mmul(b[12:], a[12:]), dtype=np.float64)


# ---- inputs ----
def r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def random_poses(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4)) * rng.uniform(0.2, 5.0, size=(n, 1))  # not unit: the library normalises
    return [(tuple(rng.uniform(-20, 20, 3)), tuple(q[k]), float(rng.uniform(0.2, 4.0))) for k in range(n)]


def random_forwards(n, seed):
    """well conditioned: a rotation times scales in [0.3, 3] times a small shear"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        A = Q @ np.diag(rng.uniform(0.3, 3.0, 3)) @ (np.eye(3) + 0.1 * rng.normal(size=(3, 3)))
        out.append(np.concatenate([A, rng.uniform(-20, 20, (3, 1))], axis=1).ravel())
    return out


FIXED_POSES = [((0, 0, 0), (0, 0, 0, 1), 1.0), ((1.5, -2.0, 0.25), (0, 0, 1, 0), 1.0), ((1.5, -2.0, 0.25), (0, 0, 3, 4), 1.0)] + \
              [((0.3, 4.0, -7.0), q, s) for q in ((0, 0, 1, 0), (0, 0, 3, 4), (0.1, -0.7, 0.2, 0.5)) for s in (1.0, 0.5, 3.0)]
POSES = FIXED_POSES + random_poses(300, 7)
POSES32 = [(tuple(r32(t)), tuple(r32(q)), float(r32(s))) for t, q, s in POSES]
IDENTITY12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
FORWARDS = [IDENTITY12] + random_forwards(300, 8)
FORWARDS32 = [r32(m) for m in FORWARDS]


def passes_check_xfm(x):
    api.compose([x])  # (raises when check_xfm refuses the matrix)
    return True


@pytest.mark.parametrize("poses", [POSES, POSES32], ids=["fp64", "through_fp32"])
def test_from_pose_is_the_stated_arithmetic_to_the_bit(poses):
    for t, q, s in poses:
        got = api.xfm_from_pose(t, q, s)
        assert same_bits(got, np_from_pose(t, q, s)), (t, q, s)
        assert passes_check_xfm(got)
    ident = api.xfm_from_pose((0, 0, 0), (0, 0, 0, 1), 1.0)
    assert np.array_equal(ident[:12], IDENTITY12) and np.array_equal(ident[12:], IDENTITY12)
    # the non-unit quaternion is normalised: (0, 0, 3, 4) / 5 is a rotation about z
    rot = api.xfm_from_pose((0, 0, 0), (0, 0, 3, 4), 1.0)
    assert np.allclose(rot[:12].reshape(3, 4)[:, :3] @ rot[:12].reshape(3, 4)[:, :3].T, np.eye(3), atol=1e-15)
    half = api.xfm_from_pose((0, 0, 0), (0, 0, 1, 0), 0.5)
    assert np.array_equal(half[:12].reshape(3, 4)[:, :3], np.diag([-0.5, -0.5, 0.5])) and np.array_equal(half[12:].reshape(3, 4)[:, :3], np.diag([-2.0, -2.0, 2.0]))


@pytest.mark.parametrize("forwards", [FORWARDS, FORWARDS32], ids=["fp64", "through_fp32"])
def test_from_forward_is_the_stated_arithmetic_to_the_bit(forwards):
    for m in forwards:
        got = api.xfm_from_forward(m)
        assert same_bits(got, np_from_forward(m)), m
        assert same_bits(got[:12], m)
        assert passes_check_xfm(got)
    # the forward matrix of a pose, inverted by cofactors, is a legal Xfm too (what a producer of 3x4 matrices hands over)
    for t, q, s in POSES32[:40]:
        assert passes_check_xfm(api.xfm_from_forward(api.xfm_from_pose(t, q, s)[:12]))


def test_mult_is_mmul_of_both_halves_and_compose_without_its_identity():
    xs = [api.xfm_from_pose(t, q, s) for t, q, s in POSES[:120]] + [api.xfm_from_forward(m) for m in FORWARDS[1:120]]
    with_compose = 0
    for a, b in zip(xs, xs[1:]):
        got = api.xfm_mult(a, b)
        assert same_bits(got, np_mult(a, b))
        if (a != 0).all() and (b != 0).all() and (got != 0).all():  # (compose starts from an identity: equal wherever no zero's sign is at stake)
            assert same_bits(got, api.compose([b, a]))
            with_compose += 1
    assert with_compose >= 100
    # where compose's identity shows: -0 + 0 is +0, so a product that is -0 comes out of compose as +0, and out of mult as it is
    neg = api.xfm_from_pose((0, 0, 0), (0, 0, 1, 0), 1.0)   # a half turn about z: its forward holds -1 and signed zeros
    a = api.xfm_mult(neg, api.translate((0.0, 0.0, 0.0)))
    assert same_bits(a, np_mult(neg, api.translate((0.0, 0.0, 0.0))))
    # out may alias an argument
    lib = L.load()
    x, y = xs[3].copy(), xs[4].copy()
    want = api.xfm_mult(x, y)
    assert lib.glome_xfm_mult(x.ctypes.data_as(L.c_dp), y.ctypes.data_as(L.c_dp), x.ctypes.data_as(L.c_dp)) == 0
    assert same_bits(x, want)


def test_instance_transform_is_the_matrix_the_show_text_prints():
    b = api.Builder()
    ball = b.sphere((0, 0, 0), 1.0)
    tr = b.transform(ball, [api.scale((1.5, 0.7, 1.0)), api.rotate((0, 0, 1), 0.4), api.translate((0.5, 2.0, 0.0))])
    cyl = b.cylinder((0.3, 0.5, -1.0), (1.0, 2.5, 0.5), 0.4)
    cone = b.cone((-3.0, 0.5, 0.0), 0.9, (-2.5, 3.5, 0.5), 0.2)
    for node in (tr, cyl, cone):
        assert IR.is_instance(b, node)
        got = b.instance_transform(node)
        assert same_bits(got, IR.xf_of(b, node)), node
        assert not np.array_equal(got[:12], IDENTITY12)
    # it follows instance_set_transforms
    M = api.compose([IR.xf_of(b, cyl), api.translate((1.0, 0.0, 0.0))])
    b.instance_set_transforms([cyl], M.reshape(1, 24))
    assert same_bits(b.instance_transform(cyl), M)
    # a rigid motion of a cone from where it was built: mult(pose, its own matrix) is a legal Xfm
    moved = api.xfm_mult(api.xfm_from_pose((0.1, 0.2, 0.3), (0.1, 0.0, 0.05, 1.0), 1.0), b.instance_transform(cone))
    assert passes_check_xfm(moved)
    with pytest.raises(api.GlomeError, match=rf"node {ball} is a Sphere, not an Instance.*status -1"):
        b.instance_transform(ball)
    for node in (10 ** 6, -1):
        with pytest.raises(api.GlomeError, match=r"glome_sb_instance_transform: bad node id.*status -1"):
            b.instance_transform(node)
    out = np.zeros(24)
    assert b.lib.glome_sb_instance_transform(b.h, tr, None) == L.E_INVALID
    assert b.lib.glome_sb_instance_transform(None, tr, out.ctypes.data_as(L.c_dp)) == L.E_INVALID


def test_the_host_functions_refuse_what_gives_no_matrix():
    lib = L.load()
    out = np.full(24, 7.0)
    po = out.ctypes.data_as(L.c_dp)

    def pose(t, q, s):
        (_, pt), (_, pq) = L.dvec(t), L.dvec(q)
        return lib.glome_xfm_from_pose(pt, pq, float(s), po)

    def forward(m):
        a, pa = L.dvec(m)
        return lib.glome_xfm_from_forward(pa, po)

    assert pose((0, 0, 0), (0, 0, 0, 0), 1.0) == L.E_INVALID            # q of length 0
    assert pose((0, 0, 0), (0, 0, 0, 1), 0.0) == L.E_INVALID            # s = 0
    assert pose((0, 0, 0), (0, 0, 0, 1), -1.0) == L.E_INVALID           # s < 0
    assert pose((0, np.nan, 0), (0, 0, 0, 1), 1.0) == L.E_INVALID
    assert pose((0, 0, 0), (0, np.inf, 0, 1), 1.0) == L.E_INVALID
    assert pose((0, 0, 0), (0, 0, 0, 1), np.inf) == L.E_INVALID
    singular = IDENTITY12.copy(); singular[8:11] = singular[4:7]         # two equal rows: det = 0
    assert forward(singular) == L.E_SCENE
    assert forward(np.zeros(12)) == L.E_SCENE
    tiny = IDENTITY12.copy(); tiny[[0, 5, 10]] = 1e-160                  # det underflows to 0
    assert forward(tiny) == L.E_SCENE
    bad = IDENTITY12.copy(); bad[3] = np.nan
    assert forward(bad) == L.E_INVALID
    assert np.array_equal(out, np.full(24, 7.0)), "a refusal leaves out untouched"
    assert lib.glome_xfm_from_pose(None, None, 1.0, po) == L.E_INVALID and lib.glome_xfm_from_forward(None, po) == L.E_INVALID
    assert lib.glome_xfm_mult(None, po, po) == L.E_INVALID and lib.glome_xfm_mult(po, po, None) == L.E_INVALID
    with pytest.raises(api.GlomeError, match="quaternion of length 0"):
        api.xfm_from_pose((0, 0, 0), (0, 0, 0, 0))
    with pytest.raises(api.GlomeError, match="singular"):
        api.xfm_from_forward(singular)
    with pytest.raises(api.GlomeError, match="12 values"):
        api.xfm_from_forward(np.zeros(16))


def test_the_source_struct_is_the_one_the_binding_declares():
    lib = L.load()
    assert lib.glome_xfm_source_size() == C.sizeof(L.XfmSource) == 32
    assert (L.XFM_PAIR, L.XFM_FORWARD, L.XFM_POSE) == (0, 1, 2) and (L.F64, L.F32) == (0, 1)
    assert {k: v for k, v in api.XFM_FORMS.items()} == {"pair": (0, 24), "forward": (1, 12), "pose": (2, 8)}
    # the layouts the Python side reads in place, and the ones it copies
    assert api._xfm_stride("t", "pose", (5, 8), (11, 1)) == 11 and api._xfm_stride("t", "pose", (5, 8), (8, 1)) == 8
    assert api._xfm_stride("t", "forward", (5, 4, 4), (16, 4, 1)) == 16 and api._xfm_stride("t", "forward", (5, 3, 4), (12, 4, 1)) == 12
    assert api._xfm_stride("t", "pose", (5, 8), (8, 2)) is None and api._xfm_stride("t", "pose", (5, 8), (4, 1)) is None
    assert api._xfm_stride("t", "pair", (1, 24), (1, 1)) == 0
    with pytest.raises(api.GlomeError, match=r"a pose source is \[n, 8\]"):
        api._xfm_stride("t", "pose", (5, 7), (7, 1))
    with pytest.raises(api.GlomeError, match=r"\[n, 3, 4\] or \[n, 4, 4\]"):
        api._xfm_stride("t", "forward", (5, 16), (16, 1))
