"""A model of the packet walk of a triangle BIH (TEST INFRASTRUCTURE, no GPU): the control flow of bih_tri_wave / bih_tri_packet
(glome_amd/csrc/rt_device.hpp) for the 64 lanes of a wave, restated in float64 over the tree oracle/np_scene.py builds -- which
tests/test_np_crosscheck.py holds equal to the product's.

It computes no expected pixels (those are the fp64 oracle's and the faithful instance's).  It says what a packet of rays makes the walk
DO: how many walks (one per octant present), how deep the stack gets, how many pushes land beyond the LDS part of the stack
(kAsmLdsCap entries, where the hand-written walk hands the step to C++) and how many pops come from there, which leaves are tested -- so
that tests/test_packet_model.py can state, on a machine without a GPU, that the inputs of tests/test_packet_walk_edges.py reach those paths.

The rules restated (rt_device.hpp):
  bih_tri_wave      root interval = bbclip_ub of the tree's bounds, far clipped to the ray's own limit; a lane enters when !(near > far);
                    the lanes are grouped by octant (the signs of 1 / d), lowest lane first, one walk per group
  branch step       dl, dr = (plane - o[axis]) / d[axis]; near child = left when the walk's rays run towards +axis; m1 = lanes with
                    near < t1, m2 = lanes with t2 < far; the far child is pushed (with m2) when m1 and m2 are both non-empty; the walk
                    goes to the near child when m1 is non-empty, else to the far one
  leaf              every triangle in order, tmax = far; mode 1: a hit that is not farther than the best replaces it (ties -> later
                    item) and clips far; mode 2: a hit retires the lane
  pop               until an entry some lane still wants: mode 1 clips far by the best hit and drops the lanes with near > far (the
                    early-out); mode 2 drops the retired lanes
"""
import collections

import numpy as np

from oracle import np_scene as NS

MUTANTS = ("low_mask_word_beyond_lds", "b_half_ignored", "no_clip_beyond_lds")
LDS_CAP = 12  # kAsmLdsCap (rt_types.h): stack entries 0..11 live in LDS, entry 12 and beyond in the overflow columns
NO_BEST = 3.0e38


def _tri(s):
    while isinstance(s, NS.Tex):
        s = s.s
    assert isinstance(s, NS.Triangle), type(s)
    return s


def tri_hits(p, o, d, tmax):
    """tri_core (np_scene / Triangle.hs:45-73) for many rays at once: (hit mask, t)"""
    p1, p2, p3 = (np.asarray(q, np.float64) for q in p)
    e1, e2 = p2 - p1, p3 - p1
    s1 = np.cross(d, e2)
    div = s1 @ e1
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / div
        dd = o - p1
        b1 = np.einsum("ij,ij->i", dd, s1) * inv
        s2 = np.cross(dd, e1)
        b2 = np.einsum("ij,ij->i", d, s2) * inv
        t = (s2 @ e2) * inv
        ok = (div != 0) & ~((b1 < 0) | (b1 > 1)) & ~((b2 < 0) | (b1 + b2 > 1)) & ~((t < 0) | (t > tmax))
    return ok, t


def root_interval(bb, o, d, dist):
    """bih_root_interval: bbclip_ub (Vec.hs:743-762) of the tree's bounds, far clipped to the ray's own limit"""
    lo, hi = np.asarray(bb[0]), np.asarray(bb[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        rcp = 1.0 / d
        pos = d > 0
        tin = np.where(pos, lo - o, hi - o) * rcp
        tout = np.where(pos, hi - o, lo - o) * rcp
    near = NS_fmax3(tin)
    far = NS_fmin3(tout)
    far = np.where(dist > far, far, dist)  # fmin d far
    return near, far


def NS_fmax3(v):  # Vec.hs:62-69, compare-select
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    return np.where(a > b, np.where(a > c, a, c), np.where(b > c, b, c))


def NS_fmin3(v):  # Vec.hs:52-59
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    return np.where(a > b, np.where(b > c, c, b), np.where(a > c, c, a))


def tree_depth(node):
    """stack entries a walk of `node` may need: the number of branches on the longest path (flatten.hpp's BihTree::depth counts the same)"""
    return 0 if node[0] == "leaf" else 1 + max(tree_depth(node[4]), tree_depth(node[5]))


def leaves(node):
    if node[0] == "leaf":
        yield node[1]
    else:
        yield from leaves(node[4])
        yield from leaves(node[5])


Walk = collections.namedtuple("Walk", "octant lanes max_depth pushes_over pops_over leaf_sizes axes")


def walk_packet(bih, o, d, dist, mode, mutant=None):
    """One packet: up to 64 rays (o, d: n x 3; dist: n or a scalar) against the np_scene.Bih `bih`, mode 1 (closest hit, early-out) or 2 (any hit).
    Returns a dict: walks (a Walk per octant present, in the order they are made), max_depth, pushes_over / pops_over (pushes that landed at
    stack entry >= LDS_CAP, pops that came from there), leaf_sizes (a Counter over the leaves tested), prim (per lane: the uid of the triangle
    hit, -1 for none; mode 2: of the occluder found), t (per lane, mode 1) and occluded (per lane, mode 2).
    mutant: None, or one of MUTANTS -- a walk that is wrong on purpose in one place, for the tests to show that their inputs can tell."""
    assert mutant is None or mutant in MUTANTS
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    assert 1 <= n <= 64 and mode in (1, 2) and bih.root[0] == "branch"
    dist = np.broadcast_to(np.asarray(dist, np.float64), (n,))
    assert np.all(d != 0), "the model takes no axis-parallel rays"
    rcp = 1.0 / d
    near0, far0 = root_interval(bih.bb, o, d, dist)
    octant = (rcp[:, 0] > 0) * 1 + (rcp[:, 1] > 0) * 2 + (rcp[:, 2] > 0) * 4
    todo = ~(near0 > far0)  # bih_root_enters
    best_t = np.full(n, NO_BEST); prim = np.full(n, -1, np.int64); occ = np.zeros(n, bool)
    walks = []
    while todo.any():
        fwdbits = int(octant[np.flatnonzero(todo)[0]])
        am = todo & (octant == fwdbits)
        todo &= ~am
        lanes = int(am.sum())
        near, far = near0.copy(), far0.copy()
        node = bih.root
        stack = []
        max_depth = pushes_over = pops_over = 0
        sizes, axes = collections.Counter(), collections.Counter()
        while True:
            while node[0] == "branch":
                _, lsplit, rsplit, axis, left, right = node
                dl, dr = (lsplit - o[:, axis]) * rcp[:, axis], (rsplit - o[:, axis]) * rcp[:, axis]
                fwd = (fwdbits >> axis) & 1
                c1, c2 = (left, right) if fwd else (right, left)
                t1, t2 = (dl, dr) if fwd else (dr, dl)
                # (an empty leaf is never entered: flatten.hpp gives it a plane at -+inf)
                m1 = am & (near < t1) & (not (c1[0] == "leaf" and not c1[1]))
                m2 = am & (t2 < far) & (not (c2[0] == "leaf" and not c2[1]))
                f1, n2 = np.minimum(t1, far), np.maximum(t2, near)
                if m1.any() and m2.any():
                    if len(stack) >= LDS_CAP:
                        pushes_over += 1
                    # (mutant: an entry beyond the LDS part keeps the low word of its lane mask only -- as the dump block would with one store missing)
                    stack.append((c2, m2 & (np.arange(n) < 32) if mutant == "low_mask_word_beyond_lds" and len(stack) >= LDS_CAP else m2, n2, far.copy()))
                    max_depth = max(max_depth, len(stack))
                    axes[axis] += 1
                if m1.any():
                    node, am, far = c1, m1, np.where(m1, f1, far)
                else:
                    node, am, near = c2, m2, np.where(m2, n2, near)
                if not am.any():
                    break
            if am.any():
                sizes[len(node[1])] += 1
                for k, s in enumerate(node[1]):
                    if mutant == "b_half_ignored" and k % 2:  # (mutant: the B half of every pair record of a leaf is never looked at)
                        continue
                    tr = _tri(s)
                    hit, t = tri_hits(tr.p, o, d, far)
                    hit &= am
                    if mode == 2:
                        occ |= hit; prim[hit] = tr.uid; am = am & ~hit
                    else:
                        # (mutant: the hand-written walk's own acceptance, t <= far alone -- right only while far <= best_t, which the clip at a pop keeps)
                        acc = hit if mutant == "no_clip_beyond_lds" else hit & ~(best_t < t)
                        best_t = np.where(acc, t, best_t); prim[acc] = tr.uid
                        far = np.where(acc & (far > t), t, far)
            am = np.zeros(n, bool)
            while stack and not am.any():
                over = len(stack) - 1 >= LDS_CAP
                pops_over += over
                node, am, near, far = stack.pop()
                if mode == 1:
                    if not (over and mutant == "no_clip_beyond_lds"):  # (mutant: a pop from beyond the LDS part keeps the `far` it was pushed with)
                        far = np.where(far > best_t, best_t, far)
                    am = am & ~(near > far)
                else:
                    am = am & ~occ
            if not am.any():
                break
        walks.append(Walk(fwdbits, lanes, max_depth, pushes_over, pops_over, sizes, axes))
    leaf_sizes = collections.Counter()
    for w in walks:
        leaf_sizes.update(w.leaf_sizes)
    return {"walks": walks, "max_depth": max((w.max_depth for w in walks), default=0), "pushes_over": sum(w.pushes_over for w in walks),
            "pops_over": sum(w.pops_over for w in walks), "leaf_sizes": leaf_sizes, "prim": prim, "t": np.where(prim >= 0, best_t, -1.0) if mode == 1 else None,
            "occluded": occ if mode == 2 else None}


def walk_stream(bih, o, d, dist, mode, mutant=None):
    """a stream as glome_trace_batch cuts it: packets of 64 consecutive rays"""
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    dist = np.broadcast_to(np.asarray(dist, np.float64), (len(o),))
    return [walk_packet(bih, o[i:i + 64], d[i:i + 64], dist[i:i + 64], mode, mutant) for i in range(0, len(o), 64)]
