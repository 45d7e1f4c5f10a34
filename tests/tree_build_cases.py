"""The case table of the tree builders (glome_sb_bih / glome_sb_bih_dev, glome_sb_mesh / glome_sb_mesh_dev) -- test infrastructure.

A bih case makes its items through any builder with the constructor methods of api.Builder (the oracle binding has the
same ones) and returns their ids; a mesh case returns (vertices, triangle rows).  Coordinates are dyadic, so that no
outcome hangs on a last-bit cost comparison unless the case is about a tie (a triangle's box carries the +-delta pad,
the same on every corner).  `reaches` names the entries of tree_build_model's record the case exists for; the host
test holds every case to them, and the whole table to every kind.  `refusal` = (status name, message pattern) for the
inputs that must come back as a status; `oracle` = False where the reference's build_rec does not terminate."""
import numpy as np

from glome_amd import api


class Case:
    def __init__(self, name, kind, make, reaches=(), refusal=None, oracle=True, dev_refusal=None):
        self.name, self.kind, self.make, self.reaches = name, kind, make, frozenset(reaches)
        self.refusal, self.oracle = refusal, oracle and refusal is None
        self.dev_refusal = dev_refusal if dev_refusal is not None else refusal  # what the device builder answers, where it differs

    def __repr__(self):
        return self.name


LOOP = ("E_SCENE", "build_rec .* does not terminate")
MESH_LOOP = ("E_SCENE", "build_tree .* does not terminate")
LIMIT = ("E_LIMIT", "deeper than the level limit of 2048")


def _dy(rng, lo, hi, step):
    """a dyadic value in [lo, hi) on a grid of `step`"""
    return lo + step * int(rng.integers(0, int((hi - lo) / step)))


def _small_box(b, rng, x0, x1, size_steps=(1, 2, 4, 8)):
    s = [int(rng.choice(size_steps)) / 64 for _ in range(3)]
    p = [_dy(rng, x0, x1, 1 / 64), _dy(rng, 0.0, 4.0, 1 / 64), _dy(rng, 0.0, 4.0, 1 / 64)]
    return b.box(tuple(p), tuple(p[a] + s[a] for a in range(3)))


# ---- sizes: m items of a cluster at x in [0, 4), then n - m at x in [8, 12): the root splits on x and puts a segment
# boundary at m -- on and beside multiples of 64, 256 and 1024 -- and the levels below split both halves at random places
BIH_SIZES = {1: 0, 2: 1, 3: 1, 4: 2, 5: 2, 63: 32, 64: 32, 65: 64, 255: 65, 256: 63, 257: 256, 1023: 257, 1024: 255, 1025: 1024, 2048: 1025, 2049: 1024}


def sized_bih(n, m):
    def make(b):
        rng = np.random.default_rng(1000 + n)
        return [_small_box(b, rng, 0.0, 4.0) if i < m else _small_box(b, rng, 8.0, 12.0) for i in range(n)]
    return make


def _tri_of_box(lo, hi):
    """three vertices whose box is (lo, hi)"""
    return [(lo[0], lo[1], lo[2]), (hi[0], hi[1], lo[2]), (lo[0], hi[1], hi[2])]


def soup(boxes, unused=()):
    """a mesh of one triangle per box (its own three vertices), then vertices no triangle uses"""
    V, T = [], []
    for lo, hi in boxes:
        T.append([len(V), len(V) + 1, len(V) + 2, -1, -1, -1, -1, -1])
        V += _tri_of_box(lo, hi)
    return np.array(V + list(unused), np.float64).reshape(-1, 3), np.array(T, np.int32).reshape(-1, 8)


def random_boxes(seed, n, big=0, span=4.0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = [int(rng.choice((1, 2, 4, 8))) / 64 * (24 if i < big else 1) for _ in range(3)]
        p = [_dy(rng, 0.0, span, 1 / 64) for _ in range(3)]
        out.append((tuple(p), tuple(p[a] + s[a] for a in range(3))))
    return out


def sized_mesh(nt, m):
    def make():
        rng = np.random.default_rng(2000 + nt)
        boxes = []
        for i in range(nt):
            x0 = 0.0 if (i % 2 == 0 if m is None else i < m) else 8.0  # m = None: alternating, so that the root's left-goers lie on both sides of 1024
            s = [int(rng.choice((1, 2, 4, 8))) / 64 for _ in range(3)]
            p = [_dy(rng, x0, x0 + 4.0, 1 / 64), _dy(rng, 0.0, 4.0, 1 / 64), _dy(rng, 0.0, 4.0, 1 / 64)]
            boxes.append((tuple(p), tuple(p[a] + s[a] for a in range(3))))
        return soup(boxes)
    return make


MESH_SIZES = {3: 1, 4: 2, 5: 2, 64: 31, 65: 64, 1024: 257, 1025: None}


def boxes_bih(boxes):
    return lambda b: [b.box(lo, hi) for lo, hi in boxes]


def nested(n, e0=0):
    """cubes nested at a shared corner, edges 2^(e0 - i): every level but a few peels one cube off (depth about 3n)"""
    return lambda b: [b.box((0.0, 0.0, 0.0), (2.0 ** (e0 - i),) * 3) for i in range(n)]


# boxes on which the written chain of the bih and the straight chain of the mesh part ways at some node of BOTH builders' trees
# (found by a search over random dyadic sets; the host test holds each builder's model to chain_differs on them)
CHAIN_BOXES = random_boxes(404, 16, big=2)


def clusters(axis, seed):
    """two clusters of 20 small boxes, 8 apart along `axis`, interleaved in input order: the root takes that axis"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(40):
        p = [_dy(rng, 0.0, 1.0, 1 / 64) for _ in range(3)]
        p[axis] += 8.0 * (i % 2)
        out.append((tuple(p), tuple(c + 1 / 16 for c in p)))
    return out


def big_over_small():
    """A slab as long as the set and sixteen short ones in its far half, all of one cross-section: every centre lies at or beyond
    the root's midpoint on every axis, so x, y and z separate nothing (1.1 x costorig each, to the bit) and big / small does."""
    return [((0.0, 0.0, 0.0), (16.0, 1.0, 1.0))] + [((8.0 + i / 2, 0.0, 0.0), (8.5 + i / 2, 1.0, 1.0)) for i in range(16)]


def _duplicates(b):
    return [b.sphere((float(i % 5), 0.0, float(i % 3)), 1.0) for i in range(600)]


def _tie_xy(b):  # a 4 x 4 grid of unit cubes in one layer: x and y cost the same to the bit, z separates nothing
    return [b.box((float(i), float(j), 0.0), (i + 0.5, j + 0.5, 0.5)) for i in range(4) for j in range(4)]


def _repeated_id(b):
    ids = boxes_bih(random_boxes(31, 12))(b)
    return ids + [ids[3], ids[3], ids[7]]


def _bih_of_bih(b):
    inner = b.bih(boxes_bih(random_boxes(32, 9))(b))
    return boxes_bih(random_boxes(33, 7))(b) + [inner]


def _instance(b):
    ids = boxes_bih(random_boxes(34, 6))(b)
    return ids + [b.transform(b.sphere((0.0, 0.0, 0.0), 0.5), [api.translate((2.0, 1.0, 0.5))]), b.transform(b.box((0.0, 0.0, 0.0), (0.25, 0.25, 0.25)), [api.translate((1.0, 3.0, 2.0))])]


def _void_item(b):  # Void's box is box_empty: inside out, with a large positive area and its midpoint at the origin
    ids = boxes_bih(random_boxes(35, 8))(b)
    return ids[:4] + [b.group([])] + ids[4:]


def _signed_zeros(b):
    """Boxes that end or begin at x = 0 with either sign of the zero, on both sides of the root's split: the host's fold keeps
    the last of equal maxima (-0.0 here) and the first of equal minima (+0.0), the device's atomic max / min the +0.0 / -0.0 of
    the key order: the two builders hold zeros of opposite signs in both children's boxes."""
    L = [((-1.0 - i / 4, 0.0, 0.0), (z, 0.25, 0.25)) for i, z in enumerate([0.0, -0.0, 0.0, -0.0, -0.0])]
    R = [((z, 0.0, 0.0), (1.0 + i / 4, 0.25, 0.25)) for i, z in enumerate([0.0, -0.0, 0.0, -0.0, 0.0])]
    return boxes_bih(L + R)(b)


def _points(n):
    return lambda b: [b.sphere((float(i), 0.0, 0.0), 0.0) for i in range(n)]


def _flat_boxes(b):  # flat in y and z: the node's box has no surface
    return [b.box((float(i), 0.0, 0.0), (i + 0.5, 0.0, 0.0)) for i in range(4)]


def _infinite_item(b):
    return boxes_bih(random_boxes(36, 5))(b) + [b.plane((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))]


def _bad_id(b):
    return boxes_bih(random_boxes(37, 5))(b) + [123456]


def _coincident_mesh():
    return soup([((0.0, 0.0, 0.0), (1.0, 0.5, 0.25))] * 7)


def _unused_vertices_mesh():
    return soup(random_boxes(41, 24), unused=[(64.0, 64.0, 64.0), (-32.0, 0.0, 0.0)])


def _infinite_vertex_mesh():  # every cost is infinite, big / small is taken and sends everything right: build_tree's fixed point
    V, T = soup(random_boxes(43, 6))
    V[4, 0] = np.inf
    return V, T


def _big_small_mesh():
    return soup(random_boxes(42, 40, big=3))



WAVES = {"wave_uniform", "wave_mixed", "wave_first_inactive", "wave_leaf_and_active", "wave_uniform_first_inactive", "wave_uniform_leaf_and_active"}
CASES = []
for _n, _m in BIH_SIZES.items():
    _r = {"leaf_size"} if _n < 4 else {"root:pick_x", "wave_uniform"}
    if _n >= 63:
        _r |= {"wave_mixed", "wave_first_inactive", "wave_leaf_and_active", "pick_y", "pick_z", "empty_side"}
    if _n >= 255:
        _r |= WAVES
    if _n % 64:
        _r |= {"wave_tail"} if _n >= 4 else set()
    if _n >= 2048:
        _r |= {"seg_straddles_1024"}
    if _n == 2049:
        _r |= {"seg_starts_on_1024"}
    CASES.append(Case("bih_n%d" % _n, "bih", sized_bih(_n, _m), _r))
for _nt, _m in MESH_SIZES.items():
    _r = {"leaf_size", "wave_uniform"}
    if _nt >= 64:
        _r |= {"wave_mixed", "wave_first_inactive", "wave_leaf_and_active", "pick_x", "pick_y", "pick_z"}
    if _nt >= 1024:
        _r |= WAVES
    if _nt % 64:
        _r |= {"wave_tail"}
    if _nt == 1025:
        _r |= {"seg_straddles_1024"}
    CASES.append(Case("mesh_nt%d" % _nt, "mesh", sized_mesh(_nt, _m), _r))

CASES += [
    # decisions
    Case("bih_root_x", "bih", boxes_bih(clusters(0, 50)), {"root:pick_x"}),
    Case("bih_root_y", "bih", boxes_bih(clusters(1, 51)), {"root:pick_y"}),
    Case("bih_root_z", "bih", boxes_bih(clusters(2, 52)), {"root:pick_z"}),
    Case("bih_root_b", "bih", boxes_bih(big_over_small()), {"root:pick_b", "root:tie_xy"}),
    Case("mesh_root_x", "mesh", lambda: soup(clusters(0, 50)), {"root:pick_x"}),
    Case("mesh_root_y", "mesh", lambda: soup(clusters(1, 51)), {"root:pick_y"}),
    Case("mesh_root_z", "mesh", lambda: soup(clusters(2, 52)), {"root:pick_z"}),
    Case("bih_chain", "bih", boxes_bih(CHAIN_BOXES), {"chain_differs", "pick_b"}),
    Case("mesh_chain", "mesh", lambda: soup(CHAIN_BOXES), {"chain_differs", "pick_z"}),
    Case("bih_tie_xy", "bih", _tie_xy, {"root:tie_xy", "root:pick_y", "tie"}),
    Case("bih_duplicates", "bih", _duplicates, {"tie", "leaf_cost", "wave_uniform_first_inactive", "wave_mixed"}),
    Case("mesh_coincident", "mesh", _coincident_mesh, {"root:leaf_cost"}),
    Case("mesh_big_small", "mesh", _big_small_mesh, {"pick_b"}),
    Case("mesh_unused_vertices", "mesh", _unused_vertices_mesh, {"root:empty_side", "root:tie"}),
    # items
    Case("bih_repeated_id", "bih", _repeated_id, {"pick_x"}),
    Case("bih_of_bih", "bih", _bih_of_bih, {"leaf_size"}),
    Case("bih_instance", "bih", _instance, {"leaf_size"}),
    Case("bih_void_item", "bih", _void_item, {"leaf_size"}),
    Case("bih_signed_zeros", "bih", _signed_zeros, {"root:pick_x"}),
    Case("bih_three_points", "bih", _points(3), {"root:leaf_size"}),
    # pools: kNodeCap / kAccCap against the guess they replace (4n + 16 nodes), and kMaxLevels from both sides
    Case("bih_nested_8", "bih", nested(8), {"empty_side"}),
    Case("bih_nested_20", "bih", nested(20), {"empty_side", "over_4n_nodes"}),
    Case("bih_nested_30", "bih", nested(30), {"empty_side", "over_4n_nodes"}),
    Case("bih_nested_100", "bih", nested(100), {"empty_side", "over_4n_nodes"}),
    Case("bih_nested_300", "bih", nested(300), {"empty_side", "over_4n_nodes", "over_512_levels"}),
    Case("bih_depth_at_limit", "bih", nested(686, 300), {"depth_at_limit", "over_4n_nodes"}),
    Case("bih_depth_over_limit", "bih", nested(687, 300), {"depth_over_limit"}, dev_refusal=LIMIT),
    # refusals
    Case("bih_four_points", "bih", _points(4), refusal=LOOP),
    Case("bih_flat_boxes", "bih", _flat_boxes, refusal=LOOP),
    Case("bih_nested_600", "bih", nested(600), refusal=LOOP),
    Case("bih_infinite_item", "bih", _infinite_item, refusal=("E_SCENE", "infinite bounding box")),
    Case("bih_bad_id", "bih", _bad_id, refusal=("E_INVALID", "")),
    Case("mesh_infinite_vertex", "mesh", _infinite_vertex_mesh, refusal=MESH_LOOP),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ORDINARY = BY_NAME["bih_n65"]  # built after every refusal, on the same context and builder
