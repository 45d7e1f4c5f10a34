"""An fp32 model of the adaptive sampler's five passes (renderTileSubsample, Glome.hs:179-323), fed from a renderTile frame.

The pass 1-4 sample of pixel (x, y) of a W x H frame is pixel (2x, 2y) of the plain frame at 2W x 2H: getCoords divides
2x / 2W, which rounds as x / W does, and 2W / 2H as W / H.  The pass 5 sample at (x + .5, y + .5) is pixel (2x + 1, 2y + 1)
of that frame.  So the samples the sampler may take are all in the doubled frame `R2`, and what is left of the sampler -- which
of them it takes, what it averages, what it blends -- is float32 arithmetic on them, written here from the reference in the
shape of oracle/np_scene.py's render_subsample: `chunk` tiles, a blank outside the tile, four neighbour sets, four forms of the
last blend.  Nothing here knows of work items, regions, blocks or lanes.

Every operation is a float32 operation in the reference's order (cCmp, cAvg, cAvg2: left-to-right sums, then * 0.25 or * 0.5).
One operation of the device is not correctly rounded, the quotient in cCmp, so every contrast is evaluated in float64 too (from
the float32 neighbours): a candidate whose float64 contrast lies within BAND * max(1, k) of its threshold is UNDECIDED -- the
model still decides it, in float32, but says how many there were and how close the closest contrast came.  The band: four
rounded differences, four rounded additions, a quotient within 2.5 ulp and the cancelling `- 1` stay under 16 ulp of max(1, k),
about 2e-6; BAND is eight times that.  A case with no undecided candidate has one answer whatever the quotient's last bits."""
import numpy as np

F = np.float32
INF = F(1000000.0)   # Vec.hs:14: the depth of a miss, and of the blank
DELTA = F(0.0001)    # Vec.hs:40
BAND = 2.0 ** -16
DEFAULT_THRESHOLDS = (0.14, 0.15, 0.16, 0.18)  # Glome.hs:221-224

# (a, b, c, d) of a pass as (dx, dy) offsets, Glome.hs:255-258, 274-277, 287-290, 303-306
NEIGHBOURS = {2: ((-2, 0), (0, 2), (2, 0), (0, -2)),
              3: ((-1, -1), (1, -1), (1, 1), (-1, 1)),
              4: ((-1, 0), (0, 1), (1, 0), (0, -1)),
              5: ((0, 0), (0, 1), (1, 1), (1, 0))}
BLEND_FORMS = ("inner", "last_col", "last_row", "corner")


def chunk(size, blocksize):  # Glome.hs:371-377: (start, length), the last tile the remainder
    out, pos = [], 0
    while True:
        if pos + blocksize >= size:
            out.append((pos, size - pos)); return out
        out.append((pos, blocksize)); pos += blocksize


def candidates(p, tw, th):
    """(dy, dx) of the pixels pass p visits in a tw x th tile (Glome.hs:241-243, 251-253, 272-273, 283-285, 301-302)."""
    dy, dx = np.mgrid[0:th, 0:tw]
    if p == 1: m = (dx % 2 == 0) & (dy % 2 == 0) & ((dx + dy) % 4 == 0)
    elif p == 2: m = (dx % 2 == 0) & (dy % 2 == 0) & ((dx + dy) % 4 == 2)
    elif p == 3: m = (dx % 2 == 1) & (dy % 2 == 1)
    elif p == 4: m = (dx + dy) % 2 == 1
    else: m = np.ones((th, tw), bool)
    return dy[m], dx[m]


def _ccmp32(p, q):  # cCmp, Glome.hs:179-189, in float32
    pd, qd = p[..., 4], q[..., 4]
    with np.errstate(divide="ignore", invalid="ignore"):
        md = np.where(pd > qd, pd / qd - F(1), qd / pd - F(1)).astype(F)
    md = np.where((pd == 0) & (qd == 0), F(0), md)
    return np.abs(q[..., 0] - p[..., 0]) + np.abs(q[..., 1] - p[..., 1]) + np.abs(q[..., 2] - p[..., 2]) + np.abs(q[..., 3] - p[..., 3]) + md


def _ccmp64(p, q):  # the same contrast of the same float32 values, in float64
    p, q = p.astype(np.float64), q.astype(np.float64)
    pd, qd = p[..., 4], q[..., 4]
    with np.errstate(divide="ignore", invalid="ignore"):
        md = np.where(pd > qd, pd / qd - 1.0, qd / pd - 1.0)
    md = np.where((pd == 0) & (qd == 0), 0.0, md)
    return np.abs(q[..., 0] - p[..., 0]) + np.abs(q[..., 1] - p[..., 1]) + np.abs(q[..., 2] - p[..., 2]) + np.abs(q[..., 3] - p[..., 3]) + md


def _fmax(a, b): return np.where(a > b, a, b)  # Vec.hs:48-49


def _cavg4(a, b, c, d): return (a + b + c + d) * F(0.25)  # cAvg, Glome.hs:191-197 (numpy adds left to right)


def _cavg2(a, b): return (a + b) * F(0.5)  # cAvg2, Glome.hs:199-205


def pack(img):
    """blitTile's rgbf (r * a) (g * a) (b * a), Glome.hs:107-110, 353-358, in float32; wraps like Word32 arithmetic."""
    img = np.asarray(img, F)
    a = img[..., 3]

    def chan(x):
        x = (x * a).astype(F)
        x = np.where(x >= 1, F(1) - DELTA, x).astype(F)
        return np.floor(x * F(256)).astype(np.int64)
    return ((chan(img[..., 0]) * 65536 + chan(img[..., 1]) * 256 + chan(img[..., 2])) & 0xFFFFFFFF).astype(np.uint32)


class Result:
    """frame [h, w, 5] float32; packed [h, w] uint32; tested[p], traced[p] for p = 1..5 (index 0 unused); after[p]: the working
    buffer of the whole frame after pass p (after[5] is the frame); wrote[h, w]: the pass that wrote a pixel of the working
    buffer; sampled[p][h, w]: candidates of pass p that were traced; contrast[p][h, w]: the float64 contrast a candidate was
    decided by (NaN elsewhere); undecided, margin (the smallest |k64 - thr| of any candidate; inf when none was tested) and
    margin_at (pass, x, y); forms: pixels per form of the last blend; outside: candidates that read a neighbour beyond the
    tile's left / right / top / bottom edge; tiles: (xt, yt, tw, th)."""


def model(R2, w, h, blocksize=65, thresholds=DEFAULT_THRESHOLDS):
    R2 = np.asarray(R2)
    assert R2.dtype == np.float32 and R2.shape == (2 * h, 2 * w, 5), (R2.dtype, R2.shape)
    thr32 = np.asarray(thresholds, F)
    assert thr32.shape == (4,)
    blank = np.array([0, 0, 0, 0, INF], F)
    res = Result()
    res.tested, res.traced = [0] * 6, [0] * 6
    res.after = [None] + [np.tile(blank, (h, w, 1)) for _ in range(5)]
    res.wrote = np.zeros((h, w), np.int8)
    res.sampled = [None] + [np.zeros((h, w), bool) for _ in range(5)]
    res.contrast = [None, None] + [np.full((h, w), np.nan) for _ in range(4)]
    res.undecided, res.margin, res.margin_at = 0, np.inf, None
    res.forms = dict.fromkeys(BLEND_FORMS, 0)
    res.outside = dict.fromkeys(("left", "right", "top", "bottom"), 0)
    res.tiles = []
    for xt, tw in chunk(w, blocksize):
        for yt, th in chunk(h, blocksize):
            res.tiles.append((xt, yt, tw, th))
            # the tile's own buffer inside a border of blanks two pixels wide: getc beyond the tile, Glome.hs:233-235
            v = np.tile(blank, (th + 4, tw + 4, 1))
            for p in range(1, 6):
                dy, dx = candidates(p, tw, th)
                x, y = xt + dx, yt + dy
                off = 1 if p == 5 else 0
                sample = R2[2 * y + off, 2 * x + off]
                res.tested[p] += len(dy)
                if p == 1:  # Glome.hs:241-250: always traced
                    need, col = np.ones(len(dy), bool), sample
                else:
                    n4 = [v[dy + 2 + oy, dx + 2 + ox] for (ox, oy) in NEIGHBOURS[p]]
                    a, b, c, d = n4
                    thr = thr32[p - 2]
                    need = _fmax(_ccmp32(a, c), _ccmp32(b, d)) > thr  # decide, Glome.hs:213-219
                    col = np.where(need[:, None], sample, _cavg4(a, b, c, d)).astype(F)
                    k64 = _fmax(_ccmp64(a, c), _ccmp64(b, d))
                    dist = np.abs(k64 - float(thr))
                    res.undecided += int(np.sum(dist <= BAND * np.maximum(1.0, k64)))
                    res.contrast[p][y, x] = k64
                    if len(dist) and np.nanmin(dist) < res.margin:
                        i = int(np.nanargmin(dist))
                        res.margin, res.margin_at = float(dist[i]), (p, int(x[i]), int(y[i]))
                    for (ox, oy) in NEIGHBOURS[p]:
                        res.outside["left"] += int(np.sum(dx + ox < 0)); res.outside["right"] += int(np.sum(dx + ox >= tw))
                        res.outside["top"] += int(np.sum(dy + oy < 0)); res.outside["bottom"] += int(np.sum(dy + oy >= th))
                res.traced[p] += int(need.sum())
                res.sampled[p][y, x] = need
                if p < 5:
                    v[dy + 2, dx + 2] = col
                    res.wrote[y, x] = p
                    for q in range(p, 5):
                        res.after[q][y, x] = col
                else:  # Glome.hs:309-316
                    lc, lr = dx == tw - 1, dy == th - 1
                    out = _cavg2(col, _cavg4(a, b, c, d))
                    out = np.where((lc & ~lr)[:, None], _cavg2(col, _cavg2(a, b)), out)
                    out = np.where((lr & ~lc)[:, None], _cavg2(col, _cavg2(a, d)), out)
                    out = np.where((lc & lr)[:, None], col, out).astype(F)
                    res.after[5][y, x] = out
                    for name, m in zip(BLEND_FORMS, (~lc & ~lr, lc & ~lr, lr & ~lc, lc & lr)):
                        res.forms[name] += int(m.sum())
    res.frame = res.after[5]
    res.packed = pack(res.frame)
    return res


def bits(img): return np.ascontiguousarray(img, dtype=F).view(np.uint32)


def first_difference(res, got):
    """Where `got` (a frame [h, w, 5]) first leaves the model's frame, and what the model did there: None when they agree on
    every bit.  The frame's pixel comes from pass 5's candidate at that pixel and its neighbours (x, y), (x, y + 1), (x + 1, y + 1),
    (x + 1, y) of the working buffer, each written by one of passes 1-4: the report names them, so that a mismatch points at
    the earliest pass that can have caused it."""
    diff = (bits(got) != bits(res.frame)).any(-1)
    if not diff.any():
        return None
    ys, xs = np.nonzero(diff)
    y, x = int(ys[0]), int(xs[0])
    tile = next(t for t in res.tiles if t[0] <= x < t[0] + t[2] and t[1] <= y < t[1] + t[3])
    lines = [f"{int(diff.sum())} of {diff.size} pixels differ; first at x={x} y={y}, tile x={tile[0]} y={tile[1]} {tile[2]}x{tile[3]}, dx={x - tile[0]} dy={y - tile[1]}",
             f"  model {res.frame[y, x].tolist()}", f"  got   {np.asarray(got)[y, x].tolist()}",
             f"  pass 5: contrast {res.contrast[5][y, x]!r}, traced {bool(res.sampled[5][y, x])}"]
    for (ox, oy) in NEIGHBOURS[5]:
        nx, ny = x + ox, y + oy
        if tile[0] <= nx < tile[0] + tile[2] and tile[1] <= ny < tile[1] + tile[3]:
            p = int(res.wrote[ny, nx])
            k = res.contrast[p][ny, nx] if p >= 2 else None
            lines.append(f"  neighbour x={nx} y={ny}: written by pass {p}, contrast {k!r}, traced {bool(res.sampled[p][ny, nx])}, value {res.after[4][ny, nx].tolist()}")
        else:
            lines.append(f"  neighbour x={nx} y={ny}: outside the tile (blank)")
    return "\n".join(lines)
