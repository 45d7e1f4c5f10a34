"""The poses of the re-split tests (test_bih_resplit_host.py) beyond bihs_refit's V0 / V1 / V2 -- test infrastructure.  Float64
throughout, like bihs_refit."""
import numpy as np

import bihs_refit as BR
import ladder
import spheres_refit as SR

SH_SEED = 23


def shuffled(P):
    """SH of a pose: the items permuted by a fixed-seed permutation, so that item k sits where item perm[k] sat.  Neighbours in the tree
    are then strangers in space: the topology a refit keeps is as wrong for the pose as a pose can make it."""
    perm = np.random.default_rng(SH_SEED).permutation(len(P))
    assert not np.array_equal(perm, np.arange(len(P))) or len(P) < 2
    return np.ascontiguousarray(P[perm])


def triangles(name, which):
    """bihs_refit.triangles, and SH = V1 shuffled"""
    return shuffled(BR.triangles(name, "V1")) if which == "SH" else BR.triangles(name, which)


def spheres(name, which):
    return shuffled(SR.spheres(name, "V1")) if which == "SH" else SR.spheres(name, which)


# ---- growth and shrink: one item list, two poses ----
GROW_N = 41


def _small_triangle(c, k):
    """a triangle of a few tenths around c, no two alike"""
    x, y, z = c
    return (x - 0.2, y, z - 0.1 - 0.001 * k, x + 0.2, y + 0.01 * k, z - 0.1, x, y + 0.3, z + 0.2)


def pose_piled():
    """A: every triangle nearly where every other is, the pile of bihs_refit.mixed_triangles: the builder cannot split it -- one leaf of
    GROW_N items, one node slot, ceil(GROW_N / 2) pair records"""
    out = []
    for k in range(GROW_N):
        y = 2.5 + 1e-3 * k
        out.append((-9.0 + 1e-3 * k, y, -9.0, 9.0, y, -9.0 - 1e-3 * k, 0.0, y + 5e-4 * k, 9.0))
    return np.array(out)


def pose_apart():
    """B: the triangles well apart on an uneven row: a branch per split and leaves of one, two and three -- more node slots, and, with
    the odd leaves' half-empty pair records, more pair records than the pile's"""
    return np.array([_small_triangle((1.7 * k + 0.4 * (k % 3), 1.0 + 0.05 * (k % 5), 0.3 * (k % 2)), k) for k in range(GROW_N)])


# ---- depth: the ladder's comb against a flat pose of as many triangles ----
def comb_and_flat():
    """(comb, flat): the ladder's triangles in its item order (tests/ladder.py: a comb of NLEV - 2 branches on the axis), and as many
    triangles of a height field, a shallow tree"""
    lad = ladder.Ladder()
    comb = np.stack([np.asarray(lad.tri_pts[t], np.float64).reshape(9) for t in lad.tri_ids])
    from glome_amd import scenes
    N = 1
    while 2 * N * N < len(comb):
        N += 1
    flat = scenes.heightfield_triangles(N)[:len(comb)]
    return comb, np.ascontiguousarray(flat, dtype=np.float64)
