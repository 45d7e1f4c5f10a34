"""A model of the packet walk of a Mesh BVH (TEST INFRASTRUCTURE, no GPU): the control flow of mesh_closest_wave
(glome_amd/csrc/rt_device.hpp) for the 64 lanes of a wave, restated in float64 over the tree oracle/np_scene.py's Mesh.build_tree builds --
which tests/test_mesh_packet_model.py holds equal to the product's.

It computes no expected pixels (those are the fp64 oracle's and the faithful instance's).  It says what a packet of rays makes the walk DO:
how many entries its stack holds at most, how many pushes land beyond the LDS part of the stack (LDS_CAP entries; the rest are the global
overflow columns of LaneStackCols) and how many pops come from there, at how many nodes the packet takes all three passes and how many of
those it meets with the LDS part already full, which leaves it tests -- so that tests/test_mesh_packet_model.py can state, on a machine
without a GPU, that the inputs of tests/test_mesh_packet_walk_edges.py reach those paths.

The rules restated (rt_device.hpp):
  root         interval = bbclip_ub_rcp of the mesh's bounds; a lane enters unless near > far, near > depth or far < 0 (Mesh.hs:141)
  branch       per lane: both child boxes clipped to the lane's interval; its FIRST child is the left one when lnear < rnear (Mesh.hs:178);
               gof / gos: does it enter the first / the second (the second judged with far clipped to the best hit so far).  Four ballots:
               mNL, mNR (lanes that go left / right NOW: their first child, or their second at once when the first is a miss), mLL, mLR
               (lanes that go there LATER).  Passes: left for mNL, right for mNR | mLR, left again for mLL.  With mNL non-empty the walk
               pushes the left child for mLL (if any), THEN the right child for mNR | mLR (if any), and goes left; else it pushes the left
               child for mLL (if any) and goes right.  A lane outside an entry stores the empty interval (+OUT, -OUT).
  leaf         every triangle in order, tmax = min(far, best_t); a hit replaces the best (t <= tmax: ties -> later triangle) and clips tmax
  pop          until an entry some lane still wants: a lane is in unless near > min(far, best_t), near > depth or min(far, best_t) < 0
  root list    (closest_flat) the meshes in order, each walked whole with the same depth; a mesh's hit replaces the best unless best.t < t
"""
import collections

import numpy as np

from packet_walk_model import NS_fmax3, NS_fmin3, tri_hits

MUTANTS = ("no_third_pass", "high_lanes_lost_beyond_lds", "later_left_interval_from_the_right")
LDS_CAP = 12  # kAsmLdsCap (rt_types.h): stack entries 0..11 live in LDS, entry 12 and beyond in the overflow columns
OUT = 3.0e38  # kOut
INF = float("inf")


def clip(o, rcp, bb):
    """bbclip_ub_rcp (Vec.hs:725-741) for many rays at once: branches on the sign of the reciprocal"""
    lo, hi = np.asarray(bb[0], np.float64), np.asarray(bb[1], np.float64)
    pos = rcp > 0
    return NS_fmax3(np.where(pos, lo - o, hi - o) * rcp), NS_fmin3(np.where(pos, hi - o, lo - o) * rcp)


def tree_depth(node):
    """levels of branches on the longest path (flatten.hpp's max_mesh_depth counts the same)"""
    return 0 if node[0] == "leaf" else 1 + max(tree_depth(node[3]), tree_depth(node[4]))


def leaves(node):
    if node[0] == "leaf":
        yield node[1]
    else:
        yield from leaves(node[3])
        yield from leaves(node[4])


def walk_packet(mesh, o, d, depth=1e6, valid=None, mutant=None):
    """One packet: up to 64 rays (o, d: n x 3; depth: n or a scalar; valid: which lanes hold a ray) against the np_scene.Mesh `mesh`.
    Returns a dict: max_sp (the most entries held), pushes_over / pops_over (pushes that landed at entry >= LDS_CAP, pops that came from
    there), three_pass / three_pass_over (nodes at which the packet took all three passes; those of them met with sp >= LDS_CAP),
    leaf_sizes (a Counter over the leaves tested), tri (per lane: the number of the triangle hit, -1 for none) and t (per lane).
    mutant: None, or one of MUTANTS -- a walk that is wrong on purpose in one place, for the tests to show that their inputs can tell."""
    assert mutant is None or mutant in MUTANTS
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    assert 1 <= n <= 64 and np.all(d != 0), "the model takes no axis-parallel rays"
    depth = np.broadcast_to(np.asarray(depth, np.float64), (n,))
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    V = np.asarray(mesh.verts, np.float64)
    rcp = 1.0 / d
    enters = lambda near, far: ~((near > far) | (near > depth) | (far < 0))
    near, far = clip(o, rcp, mesh.bb)
    best_t = np.full(n, INF); best_tri = np.full(n, -1, np.int64)
    res = {"max_sp": 0, "pushes_over": 0, "pops_over": 0, "three_pass": 0, "three_pass_over": 0, "leaf_sizes": collections.Counter()}
    am = valid & enters(near, far)
    node, stack = mesh.bvh, []

    def push(child, m, a, b):
        a, b = np.where(m, a, OUT), np.where(m, b, -OUT)
        if len(stack) >= LDS_CAP:
            res["pushes_over"] += 1
            if mutant == "high_lanes_lost_beyond_lds":  # (mutant: an overflow entry keeps the intervals of lanes 0 .. 31 only)
                hi = np.arange(n) >= 32
                a, b = np.where(hi, OUT, a), np.where(hi, -OUT, b)
        stack.append((child, a, b))
        res["max_sp"] = max(res["max_sp"], len(stack))

    while am.any():
        if node[0] == "leaf":
            res["leaf_sizes"][len(node[1])] += 1
            tmax = np.minimum(far, best_t)
            for ti in node[1]:
                hit, t = tri_hits(V[list(mesh.tris[ti])], o, d, tmax)
                hit &= am
                best_t = np.where(hit, t, best_t); best_tri[hit] = ti; tmax = np.where(hit, t, tmax)
            am = np.zeros(n, bool)
        else:
            _, lbb, rbb, left, right = node
            lnp, lfp = clip(o, rcp, lbb)
            rnp, rfp = clip(o, rcp, rbb)
            lnear, lfar, rnear, rfar = np.maximum(near, lnp), np.minimum(far, lfp), np.maximum(near, rnp), np.minimum(far, rfp)
            lfirst = lnear < rnear
            fnear, ffar = np.where(lfirst, lnear, rnear), np.where(lfirst, lfar, rfar)
            snear, sfar = np.where(lfirst, rnear, lnear), np.where(lfirst, rfar, lfar)
            gof = am & enters(fnear, ffar)
            gos = am & enters(snear, np.minimum(sfar, best_t))
            now_l, now_r = np.where(gof, lfirst, gos & ~lfirst), np.where(gof, ~lfirst, gos & lfirst)
            later_l, later_r = gof & gos & ~lfirst, gof & gos & lfirst
            in_r = now_r | later_r
            if now_l.any() and later_l.any():
                res["three_pass"] += 1
                res["three_pass_over"] += len(stack) >= LDS_CAP
            # (mutant: the later_l lanes' interval stored from the right child's clip)
            ll_near, ll_far = (rnear, rfar) if mutant == "later_left_interval_from_the_right" else (lnear, lfar)
            third = later_l.any() and not (mutant == "no_third_pass" and now_l.any())  # (mutant: the left child is not visited a second time)
            if now_l.any():
                if third: push(left, later_l, ll_near, ll_far)
                if in_r.any(): push(right, in_r, rnear, rfar)
                node, am, near, far = left, now_l, lnear, lfar
            elif in_r.any():
                if third: push(left, later_l, ll_near, ll_far)
                node, am, near, far = right, in_r, rnear, rfar
            else:
                am = np.zeros(n, bool)
        while not am.any() and stack:
            res["pops_over"] += len(stack) - 1 >= LDS_CAP
            node, near, far = stack.pop()
            am = enters(near, np.minimum(far, best_t))
    res["tri"], res["t"] = best_tri, np.where(best_tri >= 0, best_t, -1.0)
    return res


def walk_stream(meshes, o, d, depth=1e6, mutant=None):
    """a stream as glome_trace_batch cuts it: packets of 64 consecutive rays, each walked through every mesh of the root list in order
    (closest_flat).  Returns the packets' records (of the last mesh walked that is; max_sp and the counts are the largest / the sums over
    the meshes) with `which` added: per lane the position in `meshes` of the mesh whose hit is kept, -1 for none."""
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    depth = np.broadcast_to(np.asarray(depth, np.float64), (len(o),))
    out = []
    for i in range(0, len(o), 64):
        n = len(o[i:i + 64])
        best_t = np.zeros(n); tri = np.full(n, -1, np.int64); which = np.full(n, -1, np.int64)
        tot = None
        for k, mesh in enumerate(meshes):
            r = walk_packet(mesh, o[i:i + 64], d[i:i + 64], depth[i:i + 64], None, mutant)
            take = (r["tri"] >= 0) & ((which < 0) | ~(best_t < r["t"]))
            best_t = np.where(take, r["t"], best_t); tri = np.where(take, r["tri"], tri); which = np.where(take, k, which)
            if tot is None:
                tot = r
            else:
                tot["max_sp"] = max(tot["max_sp"], r["max_sp"])
                for key in ("pushes_over", "pops_over", "three_pass", "three_pass_over"):
                    tot[key] += r[key]
                tot["leaf_sizes"].update(r["leaf_sizes"])
        tot["tri"], tot["t"], tot["which"] = tri, np.where(tri >= 0, best_t, -1.0), which
        out.append(tot)
    return out
