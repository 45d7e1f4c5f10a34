"""The "mesh ladder": tests/ladder.py's comb given to `mesh` as indexed vertices, with a grid patch at its heavy end, and the ray packets
aimed at it (TEST INFRASTRUCTURE; tests/test_mesh_packet_model.py states what they reach, tests/test_mesh_packet_walk_edges.py traces
them on the GPU).  It is for the Mesh packet walk (mesh_closest_wave, glome_amd/csrc/rt_device.hpp) what the ladder is for the BIH's.

The rungs stand where the ladder's stand (ladder.rung_u, rung_rect, rung_triangles): build_tree (Mesh.hs:69-113) splits a box at its middle,
so every level peels the rung of the far half off to the right -- a comb with a leaf per rung.  The cross-section is the ladder's squeezed
to a quarter (SQUEEZE; |v|, |w| <= W = 0.00025): build_tree weighs surface areas, and with the ladder's own width it prefers, four levels down,
to split ACROSS the axis whenever two successive far rungs lie on one side of it (depth 17, with the patch beside the comb rather than under
it).  Squeezed, the delta = 1e-4 that pads every box (Vec.hs:676-690) is most of a box's width, a split across the axis saves little, and the
comb is peeled to its end: depth 24, the patch at the bottom.  A Mesh node holds two tight boxes, not two planes: a forward ray leaves a
rung pending only when it meets that rung's box, which, padded, most rays that run the comb do.

The clusters (CLUSTER: triangles that share one bounding box, which no split separates) give leaves of 1 .. 9 and 13 triangles as in the ladder, and one of 15 and one of 20: 15 is the escape value of a leaf reference's four count
bits, the count is then read from mtrimeta[first].z.  Exact duplicates (the same three vertex indices; the two materials alternate, so the
texture of a hit tells which of them was kept) sit at the front of some leaves and at the end of others.

In place of the ladder's screen a PATCH of G x G cells (two triangles each) crosses the section at the heavy end, with a small relief
along the axis: the builder splits it across the other two axes, and a Mesh ray enters the child whose box it meets first, so lanes of
opposite tilt want the two children of such a node in opposite orders -- the three-pass nodes of the walk -- while the comb's entries are
pending beneath.  The four corner cells and four inner ones are holes: lanes that start in a corner pass through to the rungs, or to
nothing.  Every other patch triangle has vertex normals, and the two materials alternate in pairs.

MeshLadder(axis, sign) puts the axis on x, y or z, pointing either way.  kind "mirror": the second material is a Reflect (the FULL MESH
instance; secondary rays re-enter the walk from inside the comb, in waves some of whose lanes hold no ray).  kind "twin": the root is a
group of two meshes built from the same arrays -- two R_MESH root entries, every hit an exact tie between them, which `nearest` gives to
the later operand.

A Mesh casts no shadow (Mesh.hs:210), so a ray's colour depends on its own hit (and, off a mirror, on the hits that follow) only.  The deep
and the mixed stream are drawn clear of every edge with the ladder's own float64 geometry (Ladder.clear); the edges stream is aimed AT
shared edges and vertices of the patch and is held to the faithful instance alone.  No direction has a zero component, no origin lies on a
box face."""
import numpy as np

import ladder
from ladder import L, NLEV, rung_u
from glome_amd import scenes
from glome_amd.scene import SceneDesc, r32

CLUSTER = [1, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 15, 20, 3]  # triangles per rung, far end first
DUPLICATES = {7: 2, 9: 3, 11: 7, 14: 4, 15: 3, 16: 5}               # rung -> how many of its triangles are one and the same triangle ...
DUP_AT_END = {9, 14, 16}                                            # ... the leaf's first ones, or (these rungs) its last ones
SQUEEZE = 0.25                                                      # the cross-section is the ladder's, squeezed (see above)
W = SQUEEZE * ladder.W
G = 6                                                               # the patch: G x G cells over |v|, |w| <= W
HOLES = {(0, 0), (0, G - 1), (G - 1, 0), (G - 1, G - 1), (2, 3), (3, 1), (1, 4), (4, 2)}
RELIEF = 0.2 * W                                                    # the patch's extent along the axis
FRAME_W, FRAME_H, FRAME_BACK = 20, 18, 9.0  # the frame of the GPU suite: from FRAME_BACK in front of the patch ladder.FRAME_ANGLE spans the cross-section
KINDS = ("plain", "mirror", "twin")
T4 = [(1, 1), (-1, 1), (1, -1), (-1, -1)]  # the tilt-sign quadrants


def patch_u(i, j):
    """the relief: where along the axis the patch's vertex (i, j) stands"""
    return RELIEF * ((3 * i + 5 * j) % 7) / 6.0


class MeshLadder(ladder.Ladder):
    """sd: the SceneDesc; mesh_ids: the SceneDesc ids of the mesh (two for the twin); tris: the mesh's n x 8 triangle rows; rung_ids[j]: the
    triangle numbers of rung j; patch_ids: those of the patch, cell_of[t] their cell.  A triangle's number is its row in `tris`."""

    def __init__(self, axis=0, sign=1, kind="plain"):
        assert kind in KINDS
        self.axis, self.sign, self.kind, self.mirror = axis, sign, kind, kind == "mirror"
        vid, verts, rows = {}, [], []

        def vertex(p):
            if p not in vid:
                vid[p] = len(verts); verts.append(p)
            return vid[p]

        def triangle(pa, pb, pc, normals, mat):
            a, b, c = vertex(pa), vertex(pb), vertex(pc)
            if sign < 0:
                b, c = c, b  # (a mirror image turns the winding: turned back, the triangle keeps facing the light)
            rows.append([a, b, c] + ([a, b, c] if normals else [-1, -1, -1]) + [mat, -1])
            return len(rows) - 1

        self.rung_ids = []
        for j in range(NLEV):
            ts = [[(p[0], SQUEEZE * p[1], SQUEEZE * p[2]) for p in t] for t in ladder.rung_triangles(j, CLUSTER[j], DUPLICATES.get(j, 1), j in DUP_AT_END)]
            self.rung_ids.append([triangle(*t, False, (j + i) % 2) for i, t in enumerate(ts)])
        self.patch_ids, self.cell_of = [], {}
        cell = 2.0 * W / G
        pt = lambda i, j: (patch_u(i, j), -W + i * cell, -W + j * cell)
        for i in range(G):
            for j in range(G):
                if (i, j) in HOLES:
                    continue
                for k, t in enumerate(((pt(i, j), pt(i + 1, j), pt(i, j + 1)), (pt(i, j + 1), pt(i + 1, j), pt(i + 1, j + 1)))):
                    n = len(self.patch_ids)
                    self.patch_ids.append(triangle(*t, n % 2 == 0, (n // 2) % 2))
                    self.cell_of[self.patch_ids[-1]] = (i, j)
        # one normal per vertex (used by the patch's smooth triangles only): leaning off the axis with the vertex's place, unit length
        V = np.array(verts)
        nrm = np.stack([np.ones(len(V)), 0.3 * np.sin(2500.0 * V[:, 1] + 1.0), 0.3 * np.cos(1900.0 * V[:, 2])], 1)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        self.tris = np.array(rows, dtype=np.int32)
        self.verts, self.norms = np.array(r32(self.world(V))), np.array(r32(self.world(nrm)))  # (as SceneDesc rounds them)

        sd = self.sd = SceneDesc()
        # (matte, as the ladder's: a ray that runs the comb looks almost straight at the light)
        mats = [scenes.matte(sd, (0.8, 0.5, 0.4)), sd.material_reflect(0.8) if self.mirror else scenes.matte(sd, (0.3, 0.6, 1.0))]
        self.mats = mats
        self.mesh_ids = [sd.mesh(self.verts, self.norms, self.tris, mats) for _ in range(2 if kind == "twin" else 1)]
        sd.set_root(sd.group(self.mesh_ids) if kind == "twin" else self.mesh_ids[0])
        sd.add_light(ladder.to_world((ladder.LIGHT_U, 0.0, 0.0), axis, sign), (4.0e5 * (L / 1000.0) ** 2, 3.6e5 * (L / 1000.0) ** 2, 3.2e5 * (L / 1000.0) ** 2))
        # the frame's camera: on the axis in front of the patch, so far back that the ladder's narrow angle spans the cross-section: every 8 x 8
        # block of the small frame then covers a good part of it, and its rays meet most of the rungs' boxes between them
        up = [0.0, 0.0, 0.0]; up[(axis + 1) % 3] = 1.0
        sd.set_camera(ladder.to_world((-FRAME_BACK, 0.0, 0.0), axis, sign), ladder.to_world((L, 0.7e-6 * L, 0.4e-6 * L), axis, sign), tuple(up), ladder.FRAME_ANGLE)

        # what Ladder.clear reads: the triangles as rounded to fp32, and which of them are one and the same
        self.tri_ids = list(range(len(self.tris)))
        self.tri_pts = {t: self.verts[self.tris[t, :3]] for t in self.tri_ids}
        self.same_as = np.all(self.tris[:, None, :3] == self.tris[None, :, :3], axis=2)
        self.rung_of = {t: j for j, ids in enumerate(self.rung_ids) for t in ids}
        self.is_mirror = (self.tris[:, 6] == 1) if self.mirror else np.zeros(len(self.tris), bool)
        self._turn = {"rung": [0] * NLEV, "patch": 0}  # whose turn it is: the triangles are aimed at in turn

    def place_of(self, t):
        """what a triangle belongs to: ("rung", j) or ("cell", i, j)"""
        return ("rung", self.rung_of[t]) if t in self.rung_of else ("cell",) + self.cell_of[t]

    # ---- is a ray well clear of every edge?  A Mesh casts no shadow: only the ray itself and, off a mirror, what follows it
    def _clear_chain(self, o, d, depth):
        ok, k, t = self.clear(o, d)
        m = (k >= 0) & self.is_mirror[np.maximum(k, 0)]
        if not m.any() or depth <= 1:
            return ok
        o, d, k, t = o[m], d[m], k[m], t[m]
        P = np.stack([self.tri_pts[i] for i in k])
        nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        smooth = self.tris[k, 3] >= 0
        if smooth.any():  # smooth_normal (Triangle.hs:135-139) of the mesh's vertex normals
            b1, b2, _ = self._all_hits(o[smooth], d[smooth])
            r = np.arange(int(smooth.sum()))
            b1, b2 = b1[r, k[smooth]], b2[r, k[smooth]]
            N = self.norms[self.tris[k[smooth], 3:6]]
            n = N[:, 0] * (1 - (b1 + b2))[:, None] + N[:, 1] * b1[:, None] + N[:, 2] * b2[:, None]
            nrm[smooth] = n / np.linalg.norm(n, axis=1, keepdims=True)
        pos = o + t[:, None] * d
        out = d - 2.0 * np.einsum("ij,ij->i", d, nrm)[:, None] * nrm  # Shader.hs:124-131
        ok[np.flatnonzero(m)] &= self._clear_chain(pos + 1e-4 * out, out, depth - 1)
        return ok

    # ---- ray generators (ladder coordinates in float64, then world, then fp32; Ladder._draw draws a lane again until it is clear)
    def _next(self, what, j=None):
        if what == "patch":
            self._turn["patch"] += 1
            return self.patch_ids[(self._turn["patch"] - 1) % len(self.patch_ids)]
        self._turn["rung"][j] += 1
        return self.rung_ids[j][(self._turn["rung"][j] - 1) % len(self.rung_ids[j])]

    def _interior(self, t, rng):
        b1 = rng.uniform(0.15, 0.55); b2 = rng.uniform(0.15, 0.85 - b1)
        p = self.local(self.tri_pts[t])
        return p[0] + b1 * (p[1] - p[0]) + b2 * (p[2] - p[0])

    @staticmethod
    def _corner(sv, sw, rng):
        return -sv * W * rng.uniform(0.86, 0.9), -sw * W * rng.uniform(0.86, 0.9)

    def deep_lanes(self, tilts, seed, rungs=range(NLEV)):
        """one forward lane per entry (sv, sw) of `tilts`: from in front of the patch, in the corner of the cross-section opposite to (sv, sw) -- a
        hole of the patch --, at an interior point of a triangle: the rungs `rungs` in turn (of each its triangles in turn) alternating with the patch's
        triangles in turn; every 13th lane stays in its corner, clear of everything."""
        rungs = list(rungs)
        target = [None if i % 13 == 5 else self._next("patch") if i % 2 else self._next("rung", rungs[(i // 2) % len(rungs)]) for i in range(len(tilts))]

        def one(i, rng):
            sv, sw = tilts[i]
            o = np.array((-rung_u(NLEV - 1) * rng.uniform(0.3, 0.5),) + self._corner(sv, sw, rng))
            if target[i] is None:
                return o, np.array((1.5 * L, o[1] + sv * W * rng.uniform(0.002, 0.008), o[2] + sw * W * rng.uniform(0.002, 0.008)))
            return o, self._interior(target[i], rng)
        return self._draw(len(tilts), seed, one)

    def reverse_lanes(self, tilts, seed):
        """lanes that run towards the heavy end: from beyond one of rungs 2 .. 5 (single triangles) at its face (as Ladder.reverse_lanes; here also
        off a mirror: the reflected ray leaves for the far end)"""
        def one(i, rng):
            sv, sw = tilts[i]
            j = 2 + i % 4
            o = np.array((rung_u(j) * rng.uniform(1.25, 1.4),) + self._corner(sv, sw, rng))
            return o, self._interior(self.rung_ids[j][0], rng)
        return self._draw(len(tilts), seed, one)

    def outside_lanes(self, tilts, seed):
        """lanes that miss the mesh's bounds: they start beside the comb and leave it"""
        def one(i, rng):
            sv, sw = tilts[i]
            o = np.array((rng.uniform(0.5, 8.0), sv * rng.uniform(1.0, 2.0), sw * rng.uniform(1.0, 2.0)))
            return o, o + np.array((1.0, sv * rng.uniform(0.05, 0.1), sw * rng.uniform(0.05, 0.1)))
        return self._draw(len(tilts), seed, one)

    def inside_lanes(self, tilts, seed):
        """lanes that start INSIDE the mesh's box, between rung j and rung j - 1 for j = 17, 16 .. 1 in turn: the even ones forward at a triangle of a
        rung farther on, the odd ones back at a triangle of a nearer rung or of the patch"""
        def one(i, rng):
            sv, sw = tilts[i]
            j = NLEV - 1 - i % (NLEV - 1)  # 17 .. 1
            o = np.array((rung_u(j) * rng.uniform(1.15, 1.45),) + self._corner(sv, sw, rng))
            if i % 2 == 0:
                jj = int(rng.integers(0, j))
            else:
                jj = int(rng.integers(j, NLEV + 3))
            t = self.patch_ids[int(rng.integers(len(self.patch_ids)))] if jj >= NLEV else self.rung_ids[jj][int(rng.integers(len(self.rung_ids[jj])))]
            return o, self._interior(t, rng)
        return self._draw(len(tilts), seed, one)

    # ---- the streams the tests share (64 consecutive rays are one packet)
    def deep_set(self):
        """eight forward packets, each of the four tilt-sign quadrants: dealt lane by lane, in runs of 16, and unevenly.  Returns o, d."""
        self._turn = {"rung": [0] * NLEV, "patch": 0}
        deal = (lambda i: i % 4, lambda i: (i // 16) % 4, lambda i: (i * 7 // 3) % 4)
        parts = [self.deep_lanes([T4[(deal[p % 3](i) + p) % 4] for i in range(64)], 100 + p) for p in range(8)]
        return np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts])

    def mixed_set(self):
        """packets composed lane by lane.  Returns o, d and a description per packet."""
        self._turn = {"rung": [3] * NLEV, "patch": 7}
        packets, what = [], []
        gen = {"deep": self.deep_lanes, "rev": self.reverse_lanes, "out": self.outside_lanes, "in": self.inside_lanes}

        def compose(parts, name):
            """parts: per lane (kind, sv, sw)"""
            o = np.zeros((64, 3), np.float32); d = np.zeros((64, 3), np.float32)
            for g, kind in enumerate(sorted({p[0] for p in parts})):
                lanes = [i for i, p in enumerate(parts) if p[0] == kind]
                o[lanes], d[lanes] = gen[kind]([parts[i][1:] for i in lanes], 1000 + 97 * len(packets) + g)
            packets.append((o, d)); what.append(name)

        compose([("deep",) + T4[i % 4] if i % 2 else ("rev",) + T4[(i // 2) % 4] for i in range(64)], "forward and reverse lanes alternating")
        for lane in (0, 31, 32, 63):  # at the ends of the wave and on the seam of the two halves of a lane mask
            compose([("rev", -1, 1) if i == lane else ("deep",) + T4[i % 4] for i in range(64)], "one reverse lane at %d" % lane)
        compose([("deep",) + T4[i % 4] if i % 2 else ("out",) + T4[(i + 1) % 4] for i in range(64)], "deep lanes between lanes that miss the bounds")
        compose([("deep",) + T4[i % 4] if 32 <= i < 40 else ("out",) + T4[i % 4] for i in range(64)], "eight deep lanes in the high half only")
        compose([("in",) + T4[(i // 2) % 4] for i in range(64)], "lanes that start inside the box")
        return np.concatenate([p[0] for p in packets]), np.concatenate([p[1] for p in packets]), what

    def edges_set(self):
        """rays aimed, in float64, exactly AT the patch's shared vertices and at the middles of its shared edges (those of a cell's diagonal too),
        from the four corners in front of the patch and from four places between the patch and the nearest rung.  Not filtered by `clear`: which of
        the triangles that share the point reports the hit is for the walk's order and fp32 to decide, and the faithful instance is the judge."""
        cell = 2.0 * W / G
        pt = lambda i, j: np.array((patch_u(i, j), -W + i * cell, -W + j * cell))
        at = []
        for i in range(1, G):
            for j in range(1, G):
                at.append(pt(i, j))
        for i in range(G):
            for j in range(G):
                if (i, j) not in HOLES:
                    at += [0.5 * (pt(i + 1, j) + pt(i, j + 1))] + ([0.5 * (pt(i + 1, j) + pt(i + 1, j + 1))] if i + 1 < G else []) + ([0.5 * (pt(i, j + 1) + pt(i + 1, j + 1))] if j + 1 < G else [])
        at = np.array(at)
        rng = np.random.default_rng(11)
        os_, ds = [], []
        for k, (sv, sw) in enumerate(T4 + T4):
            u0 = -rung_u(NLEV - 1) * rng.uniform(0.3, 0.5) if k < 4 else rung_u(NLEV - 1) * rng.uniform(0.35, 0.55)  # (behind the patch: still in front of the nearest rung)
            o = np.array((u0, -sv * W * rng.uniform(0.83, 0.93), -sw * W * rng.uniform(0.83, 0.93)))
            os_.append(np.broadcast_to(o, at.shape)); ds.append(at - o)
        o, d = ladder._f32_rays(self.world(np.concatenate(os_)), self.world(np.concatenate(ds)))
        return o, d

    def streams(self):
        return {"deep": self.deep_set(), "mixed": self.mixed_set()[:2]}


CONFIGS = ladder.CONFIGS
VARIANTS = [(a, s, "plain") for a, s in CONFIGS] + [(0, 1, "mirror"), (2, -1, "mirror"), (1, -1, "twin"), (2, 1, "twin")]
IDS = ["%s%s%s" % ("xyz"[a], "+" if s > 0 else "-", "" if k == "plain" else "-" + k) for a, s, k in VARIANTS]

# Rays whose colour the oracle ITSELF moves by more than the 1e-4 gate when it computes in fp32 instead of fp64 -- the worst count over the
# variants of a kind, per stream (tests/test_mesh_packet_model.py measures them and holds them to this record).  The GPU tests allow twice these.
AWAY_FP32 = {("plain", "deep"): 0, ("plain", "mixed"): 0, ("mirror", "deep"): 0, ("mirror", "mixed"): 0, ("twin", "deep"): 0, ("twin", "mixed"): 0}
