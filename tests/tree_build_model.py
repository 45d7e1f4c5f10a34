"""A plain fp64 restatement of the two level-by-level tree builds (glome_amd/csrc/bih_build_device.hpp) -- test infrastructure.

The object array is kept in the device's layout: one contiguous segment per node, a stable partition of every split
segment per level, breadth-first node numbers.  Python floats and numpy float64 are IEEE doubles with round-to-nearest
and no contraction, so every product, sum and comparison below is the one Graph::BihBuild::rec / MeshBuild::rec (and the
reference's build_rec / build_tree) makes, in their order.

build(...) returns a Tree: the preorder arrays of glome_sb_bih_dump (bih) or the preorder Branch / Leaf structure the
`show` text spells out (mesh), and a record of what the build did -- the places where the kernels can go wrong and a
tree alone does not show whether a case went through them:

  per node        leaf_size / leaf_cost; pick_x / pick_y / pick_z / pick_b; chain_differs (costz < costb <= costy with x
                  not strictly cheapest: the bih's written chain takes big/small, the straight one z); tie (two
                  candidates of a split node cost exactly the same), tie_xy; empty_side (the chosen partition sends
                  everything one way)
  per level and   wave_uniform (one active node: the register reduction), wave_mixed (several: the per-lane atomics),
  64-lane wave    wave_first_inactive (lane 0 inactive, a later lane active), wave_tail (active lanes and positions past
                  n), wave_leaf_and_active (positions of a leaf by size beside active ones); wave_uniform_first_inactive
                  and wave_uniform_leaf_and_active where the register reduction meets them
  per level and   seg_straddles_1024 (left-goers on both sides of a multiple of 1024 inside the segment: the block
  split segment   offsets of the second scan stage enter), seg_starts_on_1024 (start > 0 on a multiple of 1024)
  overall         depth (levels), n_nodes, widest (nodes of the widest level); over_4n_nodes (more nodes than the
                  4n + 16 the pool was once guessed at), over_512_levels, depth_at_limit / depth_over_limit (MAX_LEVELS)

A fixed point of build_rec (a chosen partition with an empty side whose other child keeps the box) raises Loop, as
the builders refuse it."""
import numpy as np

DELTA = 0.0001  # Vec.hs:40
INF = 1000000.0  # the reference's `infinity`, Vec.hs:14: box_empty is (INF, -INF), and has a positive area
SCAN_BLOCK = 1024
WAVE = 64
BLOCK = 256
MAX_LEVELS = 2048  # bihdev::kMaxLevels


def node_cap(n):  # bihdev::kNodeCap
    return 14 * n + 16


def acc_cap(n):  # bihdev::kAccCap
    return n + n // 3 + 2


class Loop(Exception):
    pass


def area(lo, hi):
    """bbsa, Vec.hs:694-697, over arrays [..., 3] (Prelude max: `max 0 v` = if 0 <= v then v else 0)"""
    d = hi - lo
    v = 2.0 * ((d[..., 0] * d[..., 1] + d[..., 0] * d[..., 2]) + d[..., 1] * d[..., 2])
    return np.where(0 <= v, v, 0.0)


def fold_join(lo, hi):
    """box_join folded from box_empty over the boxes in order, with the builders' compare-selects (gmin a b = a > b ? b : a,
    gmax a b = a > b ? a : b), so that the sign of a zero comes out as theirs"""
    blo, bhi = [INF] * 3, [-INF] * 3
    for i in range(len(lo)):
        for a in range(3):
            blo[a] = lo[i, a] if blo[a] > lo[i, a] else blo[a]
            bhi[a] = bhi[a] if bhi[a] > hi[i, a] else hi[i, a]
    return np.array(blo), np.array(bhi)


def points_box(p):
    """bbpts, Vec.hs:676-690, of the points p [k, 3]: a right fold with the +-delta pad"""
    lo, hi = p[-1] - DELTA, p[-1] + DELTA
    for q in p[-2::-1]:
        lo = np.where((q - DELTA) > lo, lo, q - DELTA)
        hi = np.where((q + DELTA) > hi, q + DELTA, hi)
    return lo, hi


class Node:
    __slots__ = ("start", "count", "lo", "hi", "leaf", "k", "nleft", "left", "right", "lsplit", "rsplit", "level")


class Tree:
    pass


def _costs(mesh, olo, ohi, omid, oarea, seg, N):
    """the four candidates of node N over its objects `seg` (indices): goes-left masks, costs, split planes / child boxes"""
    sa = float(area(N.lo, N.hi))
    mid = (N.lo + N.hi) * 0.5
    left = [omid[seg, a] < mid[a] for a in range(3)] + [oarea[seg] > sa * 0.4]
    cost, planes, boxes = [], [], []
    for k in range(4):
        ax = 0 if k == 3 else k
        L, R = seg[left[k]], seg[~left[k]]
        nl, nr = float(len(L)), float(len(R))
        if mesh:
            llo = olo[L].min(axis=0) if len(L) else np.full(3, INF)
            lhi = ohi[L].max(axis=0) if len(L) else np.full(3, -INF)
            rlo = olo[R].min(axis=0) if len(R) else np.full(3, INF)
            rhi = ohi[R].max(axis=0) if len(R) else np.full(3, -INF)
            planes.append(None)
        else:
            lmax = float(ohi[L, ax].max()) if len(L) else -INF
            rmin = float(olo[R, ax].min()) if len(R) else INF
            llo, lhi, rlo, rhi = N.lo.copy(), N.hi.copy(), N.lo.copy(), N.hi.copy()
            lhi[ax] = lmax
            rlo[ax] = rmin
            planes.append((lmax, rmin))
        boxes.append((llo, lhi, rlo, rhi))
        cost.append(float((float(area(llo, lhi)) * nl + float(area(rlo, rhi)) * nr) * (1.2 if (k == 3 and not mesh) else 1.1)))
    return sa, left, cost, planes, boxes


def build(olo, ohi, root_lo, root_hi, mesh=False):
    """olo, ohi [n, 3]: the objects' boxes in input order; root_lo, root_hi: the root's box."""
    with np.errstate(all="ignore"):  # infinite vertices: inf - inf and inf * 0 are what the builders compute, too
        return _build(olo, ohi, root_lo, root_hi, mesh)


def _build(olo, ohi, root_lo, root_hi, mesh):
    olo, ohi = np.asarray(olo, np.float64), np.asarray(ohi, np.float64)
    n = len(olo)
    omid = (olo + ohi) * 0.5
    oarea = area(olo, ohi)
    order = np.arange(n)
    nodeof = np.zeros(n, np.int64)
    min_split = 3 if mesh else 4  # a node of fewer objects is a leaf by size
    root = Node()
    root.start, root.count, root.lo, root.hi, root.level = 0, n, np.array(root_lo, np.float64), np.array(root_hi, np.float64), 0
    nodes, counts = [root], [n]
    rec = {"nodes": {}, "waves": {}, "segs": {}}
    reached = set()
    lvl_begin, lvl_end, nlev, widest = 0, 1, 0, 0
    nwaves = ((n + BLOCK - 1) // BLOCK) * (BLOCK // WAVE)
    pos = np.arange(nwaves * WAVE)
    while lvl_begin < lvl_end:
        nlev += 1
        widest = max(widest, lvl_end - lvl_begin)
        # ---- the waves of k_*_accumulate
        nd = np.where(pos < n, np.concatenate([nodeof, np.full(len(pos) - n, -1)]), -1)
        cnt = np.where(nd >= 0, np.array(counts)[nd], 0)
        act = (nd >= 0) & (cnt >= min_split)
        small = (nd >= 0) & (cnt < min_split)
        for w in range(nwaves):
            s = slice(w * WAVE, (w + 1) * WAVE)
            if not act[s].any():
                continue
            kinds = set()
            kinds.add("wave_uniform" if len(set(nd[s][act[s]])) == 1 else "wave_mixed")
            if not act[s][0]:
                kinds.add("wave_first_inactive")
                if "wave_uniform" in kinds:
                    kinds.add("wave_uniform_first_inactive")
            if (w + 1) * WAVE > n:
                kinds.add("wave_tail")
            if small[s].any():
                kinds.add("wave_leaf_and_active")
                if "wave_uniform" in kinds:
                    kinds.add("wave_uniform_leaf_and_active")
            rec["waves"][(nlev - 1, w)] = kinds
            reached |= kinds
        # ---- k_*_decide
        new_order, new_nodeof = order.copy(), np.full(n, -1, np.int64)
        for i in range(lvl_begin, lvl_end):
            N = nodes[i]
            N.leaf, N.k, N.nleft, N.left, N.right, N.lsplit, N.rsplit = True, -1, 0, -1, -1, 0.0, 0.0
            kinds = set()
            rec["nodes"][i] = kinds
            if N.count < min_split:
                kinds.add("leaf_size")
                continue
            seg = order[N.start:N.start + N.count]
            sa, left, cost, planes, boxes = _costs(mesh, olo, ohi, omid, oarea, seg, N)
            orig = sa * float(N.count)
            if orig < cost[0] and orig < cost[1] and orig < cost[2] and orig < cost[3]:
                kinds.add("leaf_cost")
                continue
            x_first = cost[0] < cost[1] and cost[0] < cost[2] and cost[0] < cost[3]
            if x_first:
                k = 0
            elif cost[1] < cost[2] and cost[1] < cost[3]:
                k = 1
            elif (cost[2] < cost[3]) if mesh else (cost[1] < cost[3]):  # the bih as written: `costy < costb`, Bih.hs:283
                k = 2
            else:
                k = 3
            kinds.add("pick_" + "xyzb"[k])
            if not x_first and cost[2] < cost[3] <= cost[1]:
                kinds.add("chain_differs")
                assert k == (2 if mesh else 3)
            if len(set(cost)) < 4:
                kinds.add("tie")
            if cost[0] == cost[1]:
                kinds.add("tie_xy")
            ax = 0 if k == 3 else k
            nleft = int(left[k].sum())
            llo, lhi, rlo, rhi = boxes[k]
            if nleft == 0 or nleft == N.count:
                kinds.add("empty_side")
                if not mesh and ((nleft == 0 and planes[k][1] == N.lo[ax]) or (nleft == N.count and planes[k][0] == N.hi[ax])):
                    raise Loop("node %d of %d objects at level %d" % (i, N.count, nlev - 1))
                same = lambda u, v: bool(np.all((u == v) | ((u != u) & (v != v))))  # Graph::same_bound
                if mesh and ((nleft == 0 and same(rlo, N.lo) and same(rhi, N.hi)) or (nleft == N.count and same(llo, N.lo) and same(lhi, N.hi))):
                    raise Loop("mesh node %d of %d triangles at level %d" % (i, N.count, nlev - 1))
            N.leaf, N.k, N.nleft, N.left, N.right = False, k, nleft, len(nodes), len(nodes) + 1
            if not mesh:
                N.lsplit, N.rsplit = planes[k][0] + DELTA, planes[k][1] - DELTA
            Lc, Rc = Node(), Node()
            Lc.start, Lc.count, Lc.lo, Lc.hi, Lc.level = N.start, nleft, llo, lhi, nlev
            Rc.start, Rc.count, Rc.lo, Rc.hi, Rc.level = N.start + nleft, N.count - nleft, rlo, rhi, nlev
            nodes += [Lc, Rc]
            counts += [Lc.count, Rc.count]
            # ---- the scan and k_bb_scatter: a stable partition of the segment
            m = left[k]
            new_order[N.start:N.start + N.count] = np.concatenate([seg[m], seg[~m]])
            new_nodeof[N.start:N.start + nleft] = N.left
            new_nodeof[N.start + nleft:N.start + N.count] = N.right
            skinds = set()
            first_b, last_b = N.start // SCAN_BLOCK, (N.start + N.count - 1) // SCAN_BLOCK
            if first_b != last_b:
                per_block = [int(m[max(0, b * SCAN_BLOCK - N.start):(b + 1) * SCAN_BLOCK - N.start].sum()) for b in range(first_b, last_b + 1)]
                if per_block[0] > 0 and sum(per_block[1:]) > 0:
                    skinds.add("seg_straddles_1024")
            if N.start > 0 and N.start % SCAN_BLOCK == 0:
                skinds.add("seg_starts_on_1024")
            rec["segs"][(nlev - 1, i)] = skinds
            reached |= skinds
        for i in range(lvl_begin, lvl_end):
            reached |= rec["nodes"][i]
        order, nodeof = new_order, new_nodeof
        lvl_begin, lvl_end = lvl_end, len(nodes)
    T = Tree()
    T.nodes, T.order, T.record, T.reached = nodes, order, rec, reached
    T.depth, T.n_nodes, T.widest, T.n = nlev, len(nodes), widest, n
    reached |= {k for k, hit in (("over_4n_nodes", len(nodes) > 4 * n + 16), ("over_512_levels", nlev > 512), ("depth_at_limit", nlev == MAX_LEVELS),
                                 ("depth_over_limit", nlev > MAX_LEVELS)) if hit}
    _preorder(T, mesh)
    return T


def _preorder(T, mesh):
    """breadth-first numbers -> the preorder of the host builders (left subtree first)"""
    ls, rs, ax, nl, items, pre = [], [], [], [], [], []
    stack = [0]
    while stack:
        N = T.nodes[stack.pop()]
        if N.leaf:
            seg = T.order[N.start:N.start + N.count].tolist()
            ls.append(0.0); rs.append(0.0); ax.append(-1); nl.append(N.count)
            items += seg
            pre.append(("Leaf", seg))
        else:
            ls.append(N.lsplit); rs.append(N.rsplit); ax.append(0 if N.k == 3 else N.k); nl.append(0)
            L, R = T.nodes[N.left], T.nodes[N.right]
            pre.append(("Branch", L.lo, L.hi, R.lo, R.hi))
            stack += [N.right, N.left]
    if mesh:
        T.preorder = pre
    else:
        T.lsplit, T.rsplit = np.array(ls), np.array(rs)
        T.axis, T.nleaf, T.items = np.array(ax, np.int32), np.array(nl, np.int32), np.array(items, np.int64)


def build_bih(olo, ohi):
    """`bih` over objects with these boxes (Bih.hs:309-324): the root's box is their join"""
    olo, ohi = np.asarray(olo, np.float64).reshape(-1, 3), np.asarray(ohi, np.float64).reshape(-1, 3)
    lo, hi = fold_join(olo, ohi)
    T = build(olo, ohi, lo, hi, mesh=False)
    T.bound = np.concatenate([lo, hi])
    return T


def build_mesh(verts, tris):
    """`mesh` (Mesh.hs:50-134): the root's box is over ALL vertices, a triangle's box over its three (each with the pad)"""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    tris = np.asarray(tris).reshape(-1, 8)[:, :3]
    lo, hi = points_box(verts)
    tb = [points_box(verts[t]) for t in tris]
    T = build(np.array([b[0] for b in tb]), np.array([b[1] for b in tb]), lo, hi, mesh=True)
    T.bound = np.concatenate([lo, hi])
    return T
