"""The ONE model of the packet walk of a triangle BIH (TEST INFRASTRUCTURE, no GPU): the hand-written walk (GLOME_PKW_ASM,
glome_amd/csrc/bih_packet_asm.hpp) and the C++ around it (bih_tri_wave / bih_tri_packet_hw / bih_tri_packet, rt_device.hpp) restated for the
64 lanes of a wave, in float64 over the tree oracle/np_scene.py builds -- which tests/test_np_crosscheck.py holds equal to the product's.

It computes no expected pixels (those are the fp64 oracle's and the faithful instance's).  It says what a packet of rays makes the walk DO,
as one list of events per packet, so that the host tests can state, on a machine without a GPU, what the packets of the GPU tests reach.

The walk runs the way bih_tri_packet_hw does: a loop around the block, which is entered with (phase, ref, am, sp), leaves with a status
(0 done, 1 a push beyond the LDS part, 3 a pop from beyond it) and is re-entered after the C++ step.  Inside the block it follows the labels:

  dispatch   the branch on a reference's two low bits.  Every SITE has its own form, so every site is recorded: after a both / near-only /
             far-only step on each axis in the register set the step ran in, after a pop (always set A), at the root (L_node at the first
             entry) and after a re-entry from a C++ step (L_node again: phase 0, the entries read back)
  step       dl, dr = (plane - o[axis]) / d[axis]; near child = left when the walk's rays run towards +axis; the far vote = lanes with
             t2 < far, the near vote = lanes with near < t1 (an empty leaf is never entered: flatten.hpp gives it a plane at -+inf).
               far vote empty                     "near" (the lanes of the near child go on) or "neither" (a pop follows)
               far vote not empty, near vote too  "both": the one step that pushes -- inside the block below the LDS part's capacity, else
                                                  handed to the C++ step (where = "cpp"), which pushes to the overflow columns; the walk
                                                  re-enters afterwards
               far vote not empty, near empty     "far": the far child alone.  Nothing is pushed, whatever the stack holds; its node is
                                                  fetched into the register set the step ran in
             A Step records the block's state: the stack pointer, the register set the node is in (A after every fetch that was not
             prefetched: the root, a pop, a re-entry; the other set after a "near" or "both" step, the same set after a "far" step), the
             axis and the direction, whether the far child is a leaf, whether its lanes are a strict subset of the node's, whether one of
             them carries a NaN `near`, how many lanes are occluded already (mode 2), and what came directly before the step.
  leaf       every triangle in order, tmax = far; mode 1: a hit that is not farther than the best replaces it (ties -> later item) and
             clips far; mode 2: a hit retires the lane.  Recorded: which items some lane accepts as a hit: item 2 p + 1 is the B half of
             pair record p, whose record index the block makes with v_add_u32 from the A half's
  pop        m0 = m0 - 1 in 32 unsigned bits, ONE compare m0 >= CAP (an empty stack leaves 0xffffffff and so goes the same way as an entry
             beyond the LDS part), and only the slow label tells the two apart.  A popped entry is filtered: mode 1 clips far by the best
             hit and drops the lanes with near > far (the early-out); mode 2 drops the retired lanes

bih_tri_wave around it: the root interval = bbclip_ub of the tree's bounds, far clipped to the ray's own limit; a lane enters when
!(near > far); the lanes are grouped by octant (the signs of 1 / d), lowest lane first, one walk per group.

origin_clip = True is the production walk: the root interval over the device's bounds, started at the ray's origin
(bih_clip_root_at_origin); it takes a direction component of +-0: bbclip_ub then gives a NaN `near` for an origin exactly on the upper z face
of the bounds (gmax3f keeps a NaN third operand).  False is the reference's interval, which walk_packet takes for rays with no such component.

walk() makes the events; walk_packet, walk_steps and walk_events are three views of them."""
import collections

import numpy as np

from oracle import np_scene as NS

MUTANTS = ("low_mask_word_beyond_lds", "b_half_ignored", "no_clip_beyond_lds")
LDS_CAP = 12  # kAsmLdsCap (rt_types.h): stack entries 0..11 live in LDS, entry 12 and beyond in the overflow columns
NO_BEST = 3.0e38
FLT_MIN = float(np.finfo(np.float32).tiny)
U32 = 0xFFFFFFFF

Entry = collections.namedtuple("Entry", "phase sp mode")
Dispatch = collections.namedtuple("Dispatch", "site axis set target mode")  # axis, set: of the step left (None, "A" for pop / root / reentry)
Step = collections.namedtuple("Step", "kind where sp set axis fwd octant fc_leaf far_subset nan_near mode occluded after")
Pop = collections.namedtuple("Pop", "sp outcome mode")  # sp before the pop; outcome: taken / rejected / empty / over (handed to C++)
Leaf = collections.namedtuple("Leaf", "size hits mode")  # hits: the item indices within the leaf that some lane accepted
Exit = collections.namedtuple("Exit", "status sp lanes mode")
Walk = collections.namedtuple("Walk", "octant lanes max_depth pushes_over pops_over leaf_sizes axes")

STEP_SITES = [(k, a, s) for k in ("both", "near", "far") for a in range(3) for s in "AB"]
TARGETS = (0, 1, 2, 3)  # a branch along x / y / z, a leaf


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


def device_bounds(bb):
    """the tree's bounds as the device holds them (flatten.hpp: the lower corner rounded down to fp32, the upper one rounded up)"""
    lo, hi = np.asarray(bb[0], np.float64), np.asarray(bb[1], np.float64)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32.astype(np.float64) > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32)
    hi32 = np.where(hi32.astype(np.float64) < hi, np.nextafter(hi32, np.float32(np.inf)), hi32)
    return lo32.astype(np.float64), hi32.astype(np.float64)


def tree_depth(node):
    """stack entries a walk of `node` may need: the number of branches on the longest path (flatten.hpp's BihTree::depth counts the same)"""
    return 0 if node[0] == "leaf" else 1 + max(tree_depth(node[4]), tree_depth(node[5]))


def leaves(node):
    if node[0] == "leaf":
        yield node[1]
    else:
        yield from leaves(node[4])
        yield from leaves(node[5])


def pop_fold(m0, cap=LDS_CAP):
    """L_pop's first three instructions and L_popslow's first two, on the stack pointer alone: s_sub_u32 m0, m0, 1; s_cmp_ge_u32 m0, cap;
    s_cbranch_scc1 L_popslow -- and there s_cmp_eq_u32 m0, -1; s_cbranch_scc1 L_empty; s_add_u32 m0, m0, 1.  Returns (where, m0): "lds" with
    the entry's index, "empty" with 0 (L_empty's s_mov_b32 m0, 0), or "over" with the stack pointer as it was (status 3)."""
    assert 0 <= m0 <= U32
    m0 = (m0 - 1) & U32
    if m0 >= cap:  # unsigned
        if m0 == U32:
            return "empty", 0
        return "over", (m0 + 1) & U32
    return "lds", m0


def _empty(c):
    return c[0] == "leaf" and not c[1]


def _kind(node):
    return 3 if node[0] == "leaf" else node[3]


class _Walk:
    """one walk of one octant: the state bih_tri_packet_hw keeps between two entries of the block"""

    def __init__(self, bih, o, d, rcp, fwdbits, am, near, far, mode, best_t, prim, occ, ev, mutant=None):
        self.o, self.d, self.rcp, self.fwdbits, self.mode, self.ev, self.mutant = o, d, rcp, fwdbits, mode, ev, mutant
        self.node, self.am, self.near, self.far = bih.root, am, near, far
        self.best_t, self.prim, self.occ = best_t, prim, occ
        self.stack, self.sp, self.max_depth = [], 0, 0
        self.handed = None  # the votes of the step the block handed to C++ (status 1)

    def votes(self):
        _, lsplit, rsplit, axis, left, right = self.node
        with np.errstate(invalid="ignore"):
            dl, dr = (lsplit - self.o[:, axis]) * self.rcp[:, axis], (rsplit - self.o[:, axis]) * self.rcp[:, axis]
            fwd = (self.fwdbits >> axis) & 1
            c1, c2 = (left, right) if fwd else (right, left)
            t1, t2 = (dl, dr) if fwd else (dr, dl)
            vf = self.am & (t2 < self.far) & (not _empty(c2))    # the far vote (VCC)
            vn = self.am & (self.near < t1) & (not _empty(c1))   # the near vote (s[K28:K29] / v_cmpx)
            f1, n2 = np.minimum(t1, self.far), np.maximum(t2, self.near)  # (v_maximum3: NaN when an operand is)
        return axis, c1, c2, vn, vf, f1, n2

    def step(self, m0, cur, after):
        """the votes of a branch step and its Step record; where = "cpp" when the block hands the step over"""
        axis, c1, c2, vn, vf, f1, n2 = v = self.votes()
        kind = ("both" if vn.any() else "far") if vf.any() else ("near" if vn.any() else "neither")
        where = "cpp" if kind == "both" and m0 >= LDS_CAP else "asm"
        self.ev.append(Step(kind, where, m0, cur, axis, bool((self.fwdbits >> axis) & 1), self.fwdbits, c2[0] == "leaf", bool(vf.any() and (self.am & ~vf).any()),
                            bool((vf & np.isnan(self.near)).any()), self.mode, int(self.occ.sum()), after))
        return kind, where, v

    def push_and_descend(self, v, over=False):
        """a both-step: the far child is pushed with the far vote, the walk goes to the near child"""
        axis, c1, c2, vn, vf, f1, n2 = v
        if over and self.mutant == "low_mask_word_beyond_lds":  # (an entry beyond the LDS part keeps the low word of its lane mask only -- as the dump block would with one store missing)
            vf = vf & (np.arange(len(vf)) < 32)
        self.stack.append((c2, vf, n2, self.far.copy()))
        self.max_depth = max(self.max_depth, len(self.stack))
        self.node, self.am, self.far = c1, vn, np.where(vn, f1, self.far)

    def filter(self, entry, over=False):
        """a popped entry: the lanes that still want it"""
        self.node, am, self.near, self.far = entry
        if self.mode == 1:
            if not (over and self.mutant == "no_clip_beyond_lds"):  # (mutant: a pop from beyond the LDS part keeps the `far` it was pushed with)
                self.far = np.where(self.far > self.best_t, self.best_t, self.far)
            am = am & ~(self.near > self.far)
        else:
            am = am & ~self.occ
        self.am = am
        return am.any()

    def leaf(self):
        hits = set()
        for k, s in enumerate(self.node[1]):
            if self.mutant == "b_half_ignored" and k % 2:  # (mutant: the B half of every pair record of a leaf is never looked at)
                continue
            tr = _tri(s)
            hit, t = tri_hits(tr.p, self.o, self.d, self.far)
            hit &= self.am
            if self.mode == 2:
                self.occ |= hit; self.prim[hit] = tr.uid; self.am = self.am & ~hit
                acc = hit
            else:
                # (mutant: the hand-written walk's own acceptance, t <= far alone -- right only while far <= best_t, which the clip at a pop keeps)
                acc = hit if self.mutant == "no_clip_beyond_lds" else hit & ~(self.best_t < t)
                self.best_t[:] = np.where(acc, t, self.best_t); self.prim[acc] = tr.uid
                self.far = np.where(acc & (self.far > t), t, self.far)
            if acc.any():
                hits.add(k)
        self.ev.append(Leaf(len(self.node[1]), frozenset(hits), self.mode))

    def block(self, phase, first):
        """GLOME_PKW_ASM from its first instruction to L_end: returns the status"""
        ev, mode = self.ev, self.mode
        m0 = self.sp
        ev.append(Entry(phase, self.sp, mode))
        state = "pop" if phase else "dispatch"
        site, cur = (("root" if first else "reentry"), None, "A"), "A"  # (site, axis, set of the dispatching code), the set the node arrives in
        while True:
            if state == "dispatch":
                ev.append(Dispatch(site[0], site[1], site[2], _kind(self.node), mode))
                state = "leaf" if self.node[0] == "leaf" else "step"
            elif state == "step":
                kind, where, v = self.step(m0, cur, site[0] if site[1] is None else "step")
                if where == "cpp":  # L_slow: the C++ step takes this node
                    self.sp, self.handed = m0, v
                    return 1
                if kind == "neither":
                    state = "pop"
                    continue
                site = (kind, v[0], cur)
                if kind == "far":
                    self.node, self.am, self.near = v[2], v[4], np.where(v[4], v[6], self.near)
                else:
                    if kind == "both":
                        assert len(self.stack) == m0
                        self.push_and_descend(v); m0 += 1
                    else:
                        self.node, self.am, self.far = v[1], v[3], np.where(v[3], v[5], self.far)
                    cur = "B" if cur == "A" else "A"
                state = "dispatch"
            elif state == "leaf":
                self.leaf()
                state = "pop"
            else:  # L_pop
                where, m0 = pop_fold(m0)  # the one compare; L_popslow tells the two cases apart
                if where == "empty":
                    ev.append(Pop(0, "empty", mode))
                    self.sp = 0; self.am = np.zeros(len(self.o), bool)
                    return 0
                if where == "over":
                    ev.append(Pop(m0, "over", mode))
                    self.sp = m0
                    return 3
                assert len(self.stack) == m0 + 1
                if self.filter(self.stack.pop()):
                    ev.append(Pop(m0 + 1, "taken", mode))
                    site, cur = ("pop", None, "A"), "A"
                    state = "dispatch"
                else:
                    ev.append(Pop(m0 + 1, "rejected", mode))

    def run(self):
        """bih_tri_packet_hw's loop"""
        phase, first = 0, True
        while True:
            st = self.block(phase, first)
            first = False
            self.ev.append(Exit(st, self.sp, int(self.am.sum()), self.mode))
            if st == 0:
                return
            assert len(self.stack) == self.sp
            if st == 1:  # one branch step of bih_tri_packet; its push goes to the overflow columns
                self.push_and_descend(self.handed, over=True); self.sp += 1
                phase = 0
            else:
                self.sp -= 1
                phase = 0 if self.filter(self.stack.pop(), over=True) else 1


def walk(bih, o, d, dist, mode, origin_clip=True, mutant=None):
    """One packet: up to 64 rays (o, d: n x 3; dist: n or a scalar) against the np_scene.Bih `bih`, mode 1 (closest hit, early-out) or 2 (any hit).
    Returns a dict: events (every Entry, Dispatch, Step, Pop, Leaf and Exit of every walk, in order), walks ((octant, lanes, deepest stack, its
    events) per octant present, in the order they are made), prim (per lane: the uid of the triangle hit, -1 for none; mode 2: of the occluder
    found), t (per lane, mode 1) and occluded (per lane, mode 2).
    mutant: None, or one of MUTANTS -- a walk that is wrong on purpose in one place, for the tests to show that their inputs can tell."""
    assert mutant is None or mutant in MUTANTS
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    assert 1 <= n <= 64 and mode in (1, 2) and bih.root[0] == "branch"
    dist = np.broadcast_to(np.asarray(dist, np.float64), (n,))
    with np.errstate(divide="ignore", invalid="ignore"):
        rcp = 1.0 / d
        near0, far0 = root_interval(device_bounds(bih.bb) if origin_clip else bih.bb, o, d, dist)
    if origin_clip:
        near0 = np.where(-FLT_MIN > near0, -FLT_MIN, near0)  # gmaxf(-FLT_MIN, near): a NaN near stays
    octant = (rcp[:, 0] > 0) * 1 + (rcp[:, 1] > 0) * 2 + (rcp[:, 2] > 0) * 4
    todo = ~(near0 > far0)  # bih_root_enters
    best_t = np.full(n, NO_BEST); prim = np.full(n, -1, np.int64); occ = np.zeros(n, bool)
    events, walks = [], []
    while todo.any():
        fwdbits = int(octant[np.flatnonzero(todo)[0]])
        am = todo & (octant == fwdbits)
        todo &= ~am
        w = _Walk(bih, o, d, rcp, fwdbits, am, near0.copy(), far0.copy(), mode, best_t, prim, occ, [], mutant)
        w.run()
        assert not w.stack
        walks.append((fwdbits, int(am.sum()), w.max_depth, w.ev))
        events += w.ev
    return {"events": events, "walks": walks, "prim": prim, "t": np.where(prim >= 0, best_t, -1.0) if mode == 1 else None, "occluded": occ if mode == 2 else None}


def _over(ev):
    """(pushes, pops) beyond the LDS part: the block's exits with status 1 and with status 3"""
    return tuple(sum(isinstance(e, Exit) and e.status == st for e in ev) for st in (1, 3))


def _view(r, **kw):
    return dict(kw, max_depth=max((w[2] for w in r["walks"]), default=0), prim=r["prim"], t=r["t"], occluded=r["occluded"])


def as_packet(r):
    """the walks as a whole: walks (a Walk per octant present), max_depth, pushes_over / pops_over (pushes that landed at stack entry >= LDS_CAP,
    pops that came from there), leaf_sizes (a Counter over the leaves tested; Walk.axes: over the axes of the pushes) and the per-lane results"""
    walks = [Walk(octant, lanes, depth, *_over(ev), collections.Counter(e.size for e in ev if isinstance(e, Leaf)),
                  collections.Counter(e.axis for e in ev if isinstance(e, Step) and e.kind == "both")) for octant, lanes, depth, ev in r["walks"]]
    return _view(r, walks=walks, pushes_over=sum(w.pushes_over for w in walks), pops_over=sum(w.pops_over for w in walks),
                 leaf_sizes=sum((w.leaf_sizes for w in walks), collections.Counter()))


def as_steps(r):
    """every branch step of every walk, in order; pushes_over are the C++ steps"""
    return _view(r, steps=[e for e in r["events"] if isinstance(e, Step)], pushes_over=_over(r["events"])[0], pops_over=_over(r["events"])[1])


def as_events(r):
    """every Entry, Dispatch, Pop, Leaf and Exit of every walk, in order; exits_push / exits_pop: block exits with status 1 / 3"""
    return _view(r, events=[e for e in r["events"] if not isinstance(e, Step)], exits_push=_over(r["events"])[0], exits_pop=_over(r["events"])[1])


def walk_packet(bih, o, d, dist, mode, mutant=None, origin_clip=False):
    assert origin_clip or np.all(np.asarray(d) != 0), "the reference interval takes no axis-parallel rays"
    return as_packet(walk(bih, o, d, dist, mode, origin_clip, mutant))


def walk_steps(bih, o, d, dist, mode, origin_clip=True):
    return as_steps(walk(bih, o, d, dist, mode, origin_clip))


def walk_events(bih, o, d, dist, mode, origin_clip=True):
    return as_events(walk(bih, o, d, dist, mode, origin_clip))


def _stream(one):
    def stream(bih, o, d, dist, mode, *a, **kw):
        """a stream as glome_trace_batch cuts it: packets of 64 consecutive rays"""
        o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
        dist = np.broadcast_to(np.asarray(dist, np.float64), (len(o),))
        return [one(bih, o[i:i + 64], d[i:i + 64], dist[i:i + 64], mode, *a, **kw) for i in range(0, len(o), 64)]
    return stream


stream, walk_stream, stream_steps, stream_events = _stream(walk), _stream(walk_packet), _stream(walk_steps), _stream(walk_events)
