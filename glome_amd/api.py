"""Host-side mirror of glome's scene vocabulary over the C ABI (include/glome_hip.h).

Names follow the reference: `sphere`, `triangle`, `box`, `cone`, `cylinder`, `disc`, `plane`, `plane_offset`,
`difference`, `intersection`, `bih`, `mesh`, `group`, `transform`, `tex`, `tag`, `noshadow`, `onlyshadow`,
`bound_object`, `innerbound` (GlomeTrace/Data/Glome/Scene.hs:1-27 re-exports them), `camera` (Scene.hs:48-57),
`light` (Shader.hs:22-23), transforms `translate` / `scale` / `rotate` / `xyz_to_uvw` / `compose` (Vec.hs:461-629).
Errors surface as exceptions the way the reference's constructors `error` out.

All compute goes through the HIP library; nothing here traces rays.
"""
import ctypes as C

import numpy as np

from . import _lib as L


class GlomeError(RuntimeError):
    pass


# what the scene updates take, by numpy dtype: the pointer type of a host form's array, the torch dtype of a device form's tensor
_HOST_PTR = {np.float64: L.c_dp, np.float32: L.c_fp, np.int32: L.c_ip}
_TORCH_NAME = {np.float64: ("torch.float64",), np.float32: ("torch.float32",)}


# ---------------------------------------------------------------- transforms (24 doubles: forward 3x4 + inverse 3x4)
def _xf(fn, *args):
    lib = L.load()
    out = np.zeros(24, dtype=np.float64)
    keep = []
    cargs = []
    for a in args:
        if isinstance(a, (float, int)):
            cargs.append(C.c_double(float(a)))
        else:
            arr, p = L.dvec(a)
            keep.append(arr)
            cargs.append(p)
    rc = getattr(lib, fn)(*cargs, out.ctypes.data_as(L.c_dp))
    if rc != 0:
        raise GlomeError(f"{fn}: invalid transform (reference would `error`, Vec.hs:466-477, 577-622)")
    return out


def translate(v):
    return _xf("glome_xfm_translate", v)


def scale(v):
    return _xf("glome_xfm_scale", v)


def rotate(axis, angle_rad):
    return _xf("glome_xfm_rotate", axis, float(angle_rad))


def xyz_to_uvw(u, v, w):
    return _xf("glome_xfm_xyz_to_uvw", u, v, w)


def compose(xfms):
    lib = L.load()
    arr = np.ascontiguousarray(np.asarray(xfms, dtype=np.float64).reshape(-1, 24))
    out = np.zeros(24, dtype=np.float64)
    if lib.glome_xfm_compose(arr.ctypes.data_as(L.c_dp), arr.shape[0], out.ctypes.data_as(L.c_dp)) != 0:
        raise GlomeError("compose: corrupt matrix")
    return out


def xfm_from_pose(t, q_xyzw, s=1.0):
    """The Xfm of the rigid pose p -> t + s R(q) p (glome_xfm_from_pose): q = (qx, qy, qz, qw), the scalar last, any length but 0; s a
    uniform scale > 0.  The arithmetic is stated in glome_hip.h and is what Scene.instance_update_from computes on the device."""
    lib = L.load()
    (_, pt), (_, pq) = L.dvec(t), L.dvec(q_xyzw)
    out = np.zeros(24, dtype=np.float64)
    rc = lib.glome_xfm_from_pose(pt, pq, float(s), out.ctypes.data_as(L.c_dp))
    if rc != 0:
        raise GlomeError(f"xfm_from_pose: a value that is not finite, a quaternion of length 0 or a scale that is not positive (status {rc})")
    return out


def xfm_from_forward(m):
    """The Xfm of a row-major 3x4 forward matrix, 12 values, its inverse by cofactors (glome_xfm_from_forward)."""
    lib = L.load()
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float64).ravel())
    if a.size != 12:
        raise GlomeError(f"xfm_from_forward: 12 values, not {a.size}")
    out = np.zeros(24, dtype=np.float64)
    rc = lib.glome_xfm_from_forward(a.ctypes.data_as(L.c_dp), out.ctypes.data_as(L.c_dp))
    if rc != 0:
        raise GlomeError(f"xfm_from_forward: {'a singular matrix' if rc == L.E_SCENE else 'a value that is not finite'} (status {rc})")
    return out


def xfm_mult(a, b):
    """a applied after b (glome_xfm_mult): compose([b, a]) without the identity it starts from and without check_xfm."""
    lib = L.load()
    (xa, pa), (xb, pb) = L.dvec(a), L.dvec(b)
    if xa.size != 24 or xb.size != 24:
        raise GlomeError("xfm_mult: two transforms of 24 values")
    out = np.zeros(24, dtype=np.float64)
    if lib.glome_xfm_mult(pa, pb, out.ctypes.data_as(L.c_dp)) != 0:
        raise GlomeError("xfm_mult: invalid arguments")
    return out


XFM_FORMS = {"pair": (L.XFM_PAIR, 24), "forward": (L.XFM_FORWARD, 12), "pose": (L.XFM_POSE, 8)}


def _xfm_stride(call, form, shape, strides):
    """The element stride between the items of an array / tensor of `shape` and element `strides` handed to instance_update_from: [n, w],
    or for "forward" [n, 3, 4] / [n, 4, 4], the inner dimensions contiguous; None when the layout is not one the library reads in place."""
    w = XFM_FORMS[form][1]
    inner = tuple(shape[1:])
    if not (inner == (w,) or (form == "forward" and inner in ((3, 4), (4, 4)))):
        raise GlomeError(f"{call}: a {form} source is [n, {w}]" + (", [n, 3, 4] or [n, 4, 4]" if form == "forward" else "") + f", not {list(shape)}")
    if tuple(strides[1:]) != ((1,) if len(inner) == 1 else (4, 1)):
        return None
    if shape[0] <= 1:
        return 0
    return strides[0] if strides[0] >= w else None


def deg(x):  # Vec.hs:17-18 (note the truncated pi, as written in the reference)
    return (x * 3.1415926535897) / 180


def camera(pos, at, up, angle_deg):
    """camera pos at up angle (Scene.hs:48-57) -> L.Camera (fp32 fields)."""
    lib = L.load()
    cam = L.Camera()
    a, pa = L.dvec(pos)
    b, pb = L.dvec(at)
    c, pc = L.dvec(up)
    lib.glome_camera_lookat(pa, pb, pc, float(angle_deg), C.byref(cam))
    return cam


def camera_from_vectors(pos, fwd, up, right):
    cam = L.Camera()
    for name, v in (("pos", pos), ("fwd", fwd), ("up", up), ("right", right)):
        getattr(cam, name)[:] = [float(x) for x in v]
    return cam


WEIGHT_PERLIN, WEIGHT_STRIPE_SQUARE, WEIGHT_STRIPE_TRIANGLE, WEIGHT_STRIPE_SINE = 1, 2, 3, 4  # GLOME_WEIGHT_*


def light(pos, color, rad=1000000.0, shadow=True):
    """light pos clr = Light pos clr (\\x -> 1/(x*x)) infinity True (Shader.hs:22-23)."""
    li = L.Light()
    li.pos[:] = [float(x) for x in pos]
    li.color[:] = [float(x) for x in color]
    li.rad = float(rad)
    li.shadow = 1 if shadow else 0
    return li


def render_params(width=720, height=480, mode=0, blocksize=65, maxdepth=3, fog=0, tile_first=0, tile_stride=1,
                  faithful=0, count_work=0, thresholds=None, rank0_share_pct=0):
    lib = L.load()
    p = L.RenderParams()
    lib.glome_render_params_default(C.byref(p))
    p.width, p.height, p.mode, p.blocksize, p.maxdepth, p.fog = width, height, mode, blocksize, maxdepth, fog
    p.tile_first, p.tile_stride, p.faithful, p.count_work = tile_first, tile_stride, faithful, count_work
    p.rank0_share_pct = rank0_share_pct
    if thresholds is not None:
        p.thresholds[:] = [float(t) for t in thresholds]
    return p


def frame_rays(cam, w, h):
    """The primary rays of a w x h frame of `cam` (an L.Camera), as (o, d) float32 arrays of w * h rows, row major: get_coordsf and
    get_rayint (Glome.hs:27-33, 119-140) evaluated in float64, rounded to float32 and renormalised -- the render kernels' own rays to an
    ulp.  What Scene.cost_image traces.  The device form is Context.camera_rays / camera_rays_dev (glome_camera_rays: the render
    kernels' own rays bit for bit, three lens models, jitter), and Scene.render_lens a whole frame from them without the rays ever
    leaving the GPU; this host form stays for small streams and as a formula to read."""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xc = ((x / w) * 2 - 1) * (w / h)
    yc = -((y / h) * 2 - 1)
    pos, fwd, up, right = (np.array(list(v), np.float64) for v in (cam.pos, cam.fwd, cam.up, cam.right))
    d = fwd + right * (-xc[..., None]) + up * yc[..., None]
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3).astype(np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    o = np.broadcast_to(pos.astype(np.float32), d.shape).copy()
    return o, d


# a work record's words (GLOME_WORK_*, include/glome_hip.h)
WORK_BIH_NODES, WORK_MESH_NODES, WORK_PRIM_TESTS, WORK_RAYS_SHADOW, WORK_RAYS_SECONDARY = 0, 1, 2, 3, 4
WORK_PRIMARY_BIH_NODES, WORK_PRIMARY_MESH_NODES, WORK_PRIMARY_PRIM_TESTS = 5, 6, 7


def trace_params(maxdepth=3, faithful=0, count_work=0):
    """glome_trace_params: faithful=1 is required when ray directions are not unit length (include/glome_hip.h, the trace seam)."""
    lib = L.load()
    p = L.TraceParams()
    lib.glome_trace_params_default(C.byref(p))
    p.maxdepth, p.faithful, p.count_work = maxdepth, faithful, count_work
    return p


LENS_PINHOLE, LENS_THIN, LENS_LATLONG = 0, 1, 2  # GLOME_LENS_*


def raygen_params(width=720, height=480, lens=LENS_PINHOLE, samples=1, jitter=0, seed=0, aperture=0.0, focus_dist=1.0):
    """glome_raygen_params: the frame, the lens model and the sampling of Context.camera_rays and Scene.render_lens."""
    lib = L.load()
    p = L.RaygenParams()
    lib.glome_raygen_params_default(C.byref(p))
    p.width, p.height, p.lens, p.samples, p.jitter, p.seed = width, height, lens, samples, jitter, seed
    p.aperture, p.focus_dist = float(aperture), float(focus_dist)
    return p


def raygen_sample(seed, pixel, s, dim):
    """The 32-bit word behind sample dimension `dim` of sample s of pixel y * width + x (glome_raygen_sample): u = (word >> 8) * 2^-24."""
    return int(L.load().glome_raygen_sample(seed & 0xffffffff, pixel & 0xffffffff, s & 0xffffffff, dim & 0xffffffff))


def adaptive_params(base_samples=None, threshold=None):
    """glome_adaptive_params of Scene.render_lens_adaptive: the first level and the most the means of a pixel's two halves may differ.
    The defaults (4, 1/64) are the library's first guess, not tuned."""
    p = L.AdaptiveParams()
    L.load().glome_adaptive_params_default(C.byref(p))
    if base_samples is not None:
        p.base_samples = int(base_samples)
    if threshold is not None:
        p.threshold = float(threshold)
    return p


def adaptive_levels(base, max_samples):
    """The levels base, 2 base, .. max_samples of the adaptive rule (glome_adaptive_levels); ValueError when the pair is not legal."""
    out = (C.c_int32 * 8)()
    n = int(L.load().glome_adaptive_levels(int(base), int(max_samples), out, 8))
    if n < 0:
        raise ValueError("adaptive_levels: base must be even and at least 2, max = base * 2^k, at most 64 (got %r, %r)" % (base, max_samples))
    return [int(out[k]) for k in range(n)]


def adaptive_fold(tuples, base, threshold):
    """The adaptive rule on the host (glome_adaptive_fold), pixel by pixel: tuples[n, max, 5] float32 (or [max, 5]) gives
    (counts[n] int32, rgbad[n, 5] float32, packed[n] uint32).  What Scene.render_lens_adaptive computes on the device, bit for bit."""
    lib = L.load()
    x = np.ascontiguousarray(tuples, dtype=np.float32)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.shape[2] != 5:
        raise ValueError("adaptive_fold: tuples must be [n, max, 5]")
    n, mx = x.shape[0], x.shape[1]
    counts, out, packed = np.zeros(n, np.int32), np.zeros((n, 5), np.float32), np.zeros(n, np.uint32)
    px, pc, po, pp = x.ctypes.data, counts.ctypes.data, out.ctypes.data, packed.ctypes.data
    for k in range(n):
        rc = lib.glome_adaptive_fold(C.cast(px + k * mx * 20, L.c_fp), int(base), mx, float(threshold), C.cast(pc + 4 * k, L.c_ip), C.cast(po + 20 * k, L.c_fp),
                                     C.cast(pp + 4 * k, L.c_up))
        if rc:
            raise ValueError("adaptive_fold: refused (base %r, max %r, threshold %r)" % (base, mx, threshold))
    return counts, out, packed


# ---------------------------------------------------------------- scene builder
class Builder:
    """One method per reference constructor; returns integer node / material ids."""

    def __init__(self):
        self.lib = L.load()
        self.h = self.lib.glome_sb_new()

    def __del__(self):
        try:
            if self.h:
                self.lib.glome_sb_free(self.h)
                self.h = None
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            raise GlomeError(f"{what}: {self.lib.glome_sb_last_error(self.h).decode()} (status {rc})")
        return rc

    def _call(self, name, *args):
        keep, cargs = [], []
        for a in args:
            if isinstance(a, float):
                cargs.append(C.c_double(a))
            elif isinstance(a, (int, np.integer)):
                cargs.append(int(a))
            else:
                arr, p = L.dvec(a)
                keep.append(arr)
                cargs.append(p)
        return self._chk(getattr(self.lib, name)(self.h, *cargs), name)

    def sphere(self, c, r): return self._call("glome_sb_sphere", c, float(r))
    def triangle(self, p1, p2, p3): return self._call("glome_sb_triangle", list(p1) + list(p2) + list(p3))
    def trianglenorm(self, p1, p2, p3, n1, n2, n3): return self._call("glome_sb_trianglenorm", list(p1) + list(p2) + list(p3), list(n1) + list(n2) + list(n3))
    def box(self, a, b): return self._call("glome_sb_box", a, b)
    def plane(self, pt, n): return self._call("glome_sb_plane", pt, n)
    def plane_offset(self, n, off): return self._call("glome_sb_plane_offset", n, float(off))
    def disc(self, pos, n, r): return self._call("glome_sb_disc", pos, n, float(r))
    def cylinder(self, p1, p2, r): return self._call("glome_sb_cylinder", p1, p2, float(r))
    def cone(self, p1, r1, p2, r2): return self._call("glome_sb_cone", p1, float(r1), p2, float(r2))

    def _ids(self, name, ids):
        arr, p = L.ivec(ids)
        return self._chk(getattr(self.lib, name)(self.h, p, len(arr)), name)

    def group(self, ids): return self._ids("glome_sb_group", ids)
    def intersection(self, ids): return self._ids("glome_sb_intersection", ids)
    def bih(self, ids): return self._ids("glome_sb_bih", ids)

    def triangles_bulk(self, pts9):
        """n x 9 array -> list of triangle ids (one glome_sb_triangle call each)."""
        pts9 = np.ascontiguousarray(pts9, dtype=np.float64).reshape(-1, 9)
        f = self.lib.glome_sb_triangle
        base = pts9.ctypes.data
        ids = [f(self.h, C.cast(base + 72 * k, L.c_dp)) for k in range(pts9.shape[0])]
        if ids and min(ids) < 0:
            self._chk(min(ids), "glome_sb_triangle")
        return ids

    def transform(self, node, xfms):
        arr = np.ascontiguousarray(np.asarray(xfms, dtype=np.float64).reshape(-1, 24))
        return self._chk(self.lib.glome_sb_transform(self.h, int(node), arr.ctypes.data_as(L.c_dp), arr.shape[0]), "glome_sb_transform")

    def difference(self, a, b): return self._chk(self.lib.glome_sb_difference(self.h, int(a), int(b)), "glome_sb_difference")
    def difference_retexture(self, a, b): return self._chk(self.lib.glome_sb_difference_retexture(self.h, int(a), int(b)), "glome_sb_difference_retexture")

    def mesh(self, verts, norms, tris, mats):
        v = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 3))
        n = np.ascontiguousarray(np.asarray(norms, dtype=np.float64).reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(tris, dtype=np.int32).reshape(-1, 8))
        m = np.ascontiguousarray(np.asarray(mats, dtype=np.int32).ravel())
        return self._chk(self.lib.glome_sb_mesh(self.h, v.ctypes.data_as(L.c_dp), v.shape[0], n.ctypes.data_as(L.c_dp), n.shape[0],
                                                t.ctypes.data_as(L.c_ip), t.shape[0], m.ctypes.data_as(L.c_ip), m.shape[0]), "glome_sb_mesh")

    def mesh_set_vertices(self, node, verts, norms=None):
        """Same tree, new vertices (glome_sb_mesh_set_vertices): the mesh's boxes are made again from `verts`, its topology stays."""
        v = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 3))
        n = None if norms is None else np.ascontiguousarray(np.asarray(norms, dtype=np.float64).reshape(-1, 3))
        self._chk(self.lib.glome_sb_mesh_set_vertices(self.h, int(node), v.ctypes.data_as(L.c_dp), v.shape[0], n.ctypes.data_as(L.c_dp) if n is not None and n.shape[0] else None,
                                                      0 if n is None else n.shape[0]), "glome_sb_mesh_set_vertices")

    def bih_set_triangles(self, node, pts9):
        """Same tree, new triangles (glome_sb_bih_set_triangles): nine values per item in update order (bih_items); the bih's planes and
        box are made again, its topology stays."""
        p = np.ascontiguousarray(np.asarray(pts9, dtype=np.float64).reshape(-1, 9))
        self._chk(self.lib.glome_sb_bih_set_triangles(self.h, int(node), p.ctypes.data_as(L.c_dp) if p.shape[0] else None, p.shape[0]), "glome_sb_bih_set_triangles")

    def bih_set_triangles_indexed(self, node, verts, idx):
        """bih_set_triangles from a vertex array [nv, 3] and an index table [n, 3] of vertex indices per item in update order
        (glome_sb_bih_set_triangles_indexed): only referenced vertices count."""
        v = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 3))
        i = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1, 3))
        self._chk(self.lib.glome_sb_bih_set_triangles_indexed(self.h, int(node), v.ctypes.data_as(L.c_dp) if v.shape[0] else None, v.shape[0],
                                                              i.ctypes.data_as(L.c_ip) if i.shape[0] else None, i.shape[0]), "glome_sb_bih_set_triangles_indexed")

    def bih_set_spheres(self, node, c3r):
        """Same tree, new spheres (glome_sb_bih_set_spheres): four values per item in update order (bih_items), cx cy cz r with r > 0; the
        bih's planes and box are made again, its topology stays."""
        p = np.ascontiguousarray(np.asarray(c3r, dtype=np.float64).reshape(-1, 4))
        self._chk(self.lib.glome_sb_bih_set_spheres(self.h, int(node), p.ctypes.data_as(L.c_dp) if p.shape[0] else None, p.shape[0]), "glome_sb_bih_set_spheres")

    def instance_set_transforms(self, ids, xfms):
        """New matrices for Instances (glome_sb_instance_set_transforms): xfms holds 24 values per id (api.translate / rotate / compose ...);
        every bih that holds one of them as an item has its planes and box made again, its topology stays."""
        i, pi = L.ivec(ids)
        x = np.ascontiguousarray(np.asarray(xfms, dtype=np.float64).reshape(-1, 24))
        if x.shape[0] != len(i):
            raise GlomeError(f"instance_set_transforms: {len(i)} ids but {x.shape[0]} matrices")
        self._chk(self.lib.glome_sb_instance_set_transforms(self.h, pi if len(i) else None, x.ctypes.data_as(L.c_dp) if len(i) else None, len(i)), "glome_sb_instance_set_transforms")

    def instance_transform(self, node):
        """The 24 doubles of Instance `node` as it stands (glome_sb_instance_transform): the placement a `cylinder` or `cone` carries, the
        product a `transform` made.  xfm_mult(motion, this) moves the Instance rigidly."""
        out = np.zeros(24, dtype=np.float64)
        self._chk(self.lib.glome_sb_instance_transform(self.h, int(node), out.ctypes.data_as(L.c_dp)), "glome_sb_instance_transform")
        return out

    def bih_refit(self, node):
        """What `bih` derives from its items' bounds, made again for the tree as it stands (glome_sb_bih_refit): after mesh_set_vertices /
        bih_set_triangles / instance_set_transforms of something below, call it for every bih above, inner trees first (bihs_above)."""
        self._chk(self.lib.glome_sb_bih_refit(self.h, int(node)), "glome_sb_bih_refit")

    def bih_resplit(self, node):
        """The tree built again in place from its items' bounds as they stand (glome_sb_bih_resplit): the tree `bih` makes over
        bih_items(node) in that order, under the old id; the update order stays.  After bih_set_triangles / bih_set_spheres of a pose
        that has degraded the tree; then bih_refit of the bihs above, inner trees first."""
        self._chk(self.lib.glome_sb_bih_resplit(self.h, int(node)), "glome_sb_bih_resplit")

    def bih_layout(self, node):
        """What a commit lays out for a bih of plain triangles or plain spheres (glome_sb_bih_layout): a dict of `slots` (node slots,
        treelet padding included), `pairs` (pair records), `records` and `depth`."""
        out = (C.c_int64 * 4)()
        self._chk(self.lib.glome_sb_bih_layout(self.h, int(node), out), "glome_sb_bih_layout")
        return dict(zip(("slots", "pairs", "records", "depth"), (int(x) for x in out)))

    def bihs_above(self, root, node):
        """the bihs above `node` in the scene under `root`, in an order in which they can be refitted (glome_sb_bihs_above); raises with
        the reason when an update of `node` would be refused even with nested updates on"""
        n = self._chk(self.lib.glome_sb_bihs_above(self.h, int(root), int(node), None, 0), "glome_sb_bihs_above")
        out = np.zeros(max(1, n), np.int32)
        self._chk(self.lib.glome_sb_bihs_above(self.h, int(root), int(node), out.ctypes.data_as(L.c_ip), n), "glome_sb_bihs_above")
        return [int(x) for x in out[:n]]

    def bih_items(self, node):
        """the item ids of a Bih in update order (glome_sb_bih_items)"""
        n = self._chk(self.lib.glome_sb_bih_items(self.h, int(node), None, 0), "glome_sb_bih_items")
        out = np.zeros(max(1, n), np.int32)
        self._chk(self.lib.glome_sb_bih_items(self.h, int(node), out.ctypes.data_as(L.c_ip), n), "glome_sb_bih_items")
        return [int(x) for x in out[:n]]

    def tex(self, node, material): return self._chk(self.lib.glome_sb_tex(self.h, int(node), int(material)), "glome_sb_tex")
    def tag(self, node, _tag=None): return self._chk(self.lib.glome_sb_tag(self.h, int(node)), "glome_sb_tag")
    def noshadow(self, node): return self._chk(self.lib.glome_sb_noshadow(self.h, int(node)), "glome_sb_noshadow")
    def onlyshadow(self, node): return self._chk(self.lib.glome_sb_onlyshadow(self.h, int(node)), "glome_sb_onlyshadow")
    def bound_object(self, a, b): return self._chk(self.lib.glome_sb_bound_object(self.h, int(a), int(b)), "glome_sb_bound_object")
    def innerbound(self, a, b): return self._chk(self.lib.glome_sb_innerbound(self.h, int(a), int(b)), "glome_sb_innerbound")
    def flatten_transform(self, node): return self._chk(self.lib.glome_sb_flatten_transform(self.h, int(node)), "glome_sb_flatten_transform")
    def tolist(self, node): return self._chk(self.lib.glome_sb_tolist(self.h, int(node)), "glome_sb_tolist")

    def list_items(self, node):
        """the [SolidItem] that `tolist node` yields, as node ids"""
        n = self._chk(self.lib.glome_sb_list_items(self.h, int(node), None, 0), "glome_sb_list_items")
        out = np.zeros(max(1, n), np.int32)
        self._chk(self.lib.glome_sb_list_items(self.h, int(node), out.ctypes.data_as(L.c_ip), n), "glome_sb_list_items")
        return [int(x) for x in out[:n]]

    def bih_tolist(self, node): return self.bih(self.list_items(node))  # `bih (tolist node)`, TestScene.hs:109

    def material_surface(self, color, alpha, amb, kd, ks, shine):
        return self._call("glome_sb_material_surface", color, float(alpha), float(amb), float(kd), float(ks), float(shine))
    def material_reflect(self, refl): return self._call("glome_sb_material_reflect", float(refl))
    def material_refract(self, refl, refr, ior): return self._call("glome_sb_material_refract", float(refl), float(refr), float(ior))
    def material_layers(self, mats): return self._ids("glome_sb_material_layers", mats)
    def material_blend(self, a, b, w): return self._chk(self.lib.glome_sb_material_blend(self.h, int(a), int(b), float(w)), "glome_sb_material_blend")

    def load_nff(self, text, max_lights=16):
        """A scene in NFF (Spd.hs:89-254): returns (root node, (from, at, up, angle), [(pos, rgb), ...], background rgb)."""
        cam = (C.c_double * 10)(); lp = (C.c_double * (6 * max_lights))(); nl = C.c_int32(0); bg = (C.c_double * 3)()
        root = self._chk(self.lib.glome_sb_load_nff(self.h, text.encode() if isinstance(text, str) else text, cam, lp, max_lights, C.byref(nl), bg), "glome_sb_load_nff")
        c = list(cam)
        lights = [(tuple(lp[6 * k:6 * k + 3]), tuple(lp[6 * k + 3:6 * k + 6])) for k in range(min(nl.value, max_lights))]
        return root, (tuple(c[0:3]), tuple(c[3:6]), tuple(c[6:9]), c[9]), lights, tuple(bg)

    def show(self, node):
        """Node `node` as the text GlomeView's `show geom` prints (Glome.hs:431; derived Show + Solid.hs:277, Tex.hs:50, Mesh.hs:44)."""
        n = self.lib.glome_sb_show(self.h, int(node), None, 0)
        self._chk(int(n), "glome_sb_show")
        buf = C.create_string_buffer(n + 1)
        self._chk(int(self.lib.glome_sb_show(self.h, int(node), buf, n + 1)), "glome_sb_show")
        return buf.value.decode()

    def show_tex_materials(self, node):
        """Material ids of the Tex constructors of show(node), in reading order (the part the text cannot carry)."""
        n = int(self.lib.glome_sb_show_tex_materials(self.h, int(node), None, 0))
        self._chk(n, "glome_sb_show_tex_materials")
        out = (C.c_int32 * max(1, n))()
        self._chk(int(self.lib.glome_sb_show_tex_materials(self.h, int(node), out, n)), "glome_sb_show_tex_materials")
        return list(out)[:n]

    def load_show(self, text, tex_materials=(), default_material=-1):
        """Read a `show geom` text: returns (root node, number of Tex constructors).  The k-th Tex gets tex_materials[k],
        later ones default_material (textures are closures in the reference and print as "Texture")."""
        mats = (C.c_int32 * max(1, len(tex_materials)))(*[int(m) for m in tex_materials])
        nt = C.c_int32(0)
        root = self._chk(self.lib.glome_sb_load_show(self.h, text.encode() if isinstance(text, str) else text, mats, len(tex_materials), int(default_material), C.byref(nt)),
                         "glome_sb_load_show")
        return root, nt.value

    def material_blend_fn(self, a, b, fn, params):
        """Blend a b (f pos): fn = WEIGHT_PERLIN (params = [scale]) or WEIGHT_STRIPE_* (params = axis), TestScene.hs:214-234."""
        wp = (C.c_double * 4)(*([float(x) for x in params] + [0.0] * (4 - len(params))))
        return self._chk(self.lib.glome_sb_material_blend_fn(self.h, int(a), int(b), int(fn), wp), "glome_sb_material_blend_fn")

    def material_warp(self, frame, scene, lights, xfm):
        """Warp frame scene' lights' xfm (Shader.hs:47-50): scene = a node or None (the root the scene is committed with);
        lights = glome_light structs (api.light); xfm = the 24 doubles of the transform M of the closure
        \\ray hit -> xfm_ray M (Ray (pos hit) (vnorm (dir ray))) (the portal, TestScene.hs:166-172)."""
        la = (L.Light * max(1, len(lights)))(*lights)
        x = np.ascontiguousarray(np.asarray(xfm, dtype=np.float64).ravel())
        return self._chk(self.lib.glome_sb_material_warp(self.h, int(frame), -1 if scene is None else int(scene), la, len(lights), x.ctypes.data_as(L.c_dp)), "glome_sb_material_warp")

    # host-side inspection
    def primcount(self, node):
        out = (C.c_long * 3)()
        self._chk(self.lib.glome_sb_primcount(self.h, int(node), out), "glome_sb_primcount")
        return tuple(out)

    def bound(self, node):
        out = np.zeros(6)
        self._chk(self.lib.glome_sb_bound(self.h, int(node), out.ctypes.data_as(L.c_dp)), "glome_sb_bound")
        return out

    def bih_dump(self, node):
        n = self.lib.glome_sb_bih_dump(self.h, int(node), 0, None, None, None, None, None, 0)
        self._chk(int(n), "glome_sb_bih_dump")
        ls, rs = np.zeros(n), np.zeros(n)
        ax, nl = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        cap = 1 << 24
        lp = np.zeros(cap, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self.lib.glome_sb_bih_dump(self.h, int(node), n, ls.ctypes.data_as(L.c_dp), rs.ctypes.data_as(L.c_dp), ax.ctypes.data_as(ip),
                                   nl.ctypes.data_as(ip), lp.ctypes.data_as(L.c_ip), cap)
        return ls, rs, ax, nl, lp[:int(nl.sum())]


# ---------------------------------------------------------------- device objects
class Context:
    def __init__(self, device=0):
        self.lib = L.load()
        self.h = self.lib.glome_ctx_create(int(device))
        if not self.h:
            raise GlomeError("glome_ctx_create failed: " + self.lib.glome_global_error().decode() + " (no CPU fallback exists)")

    def close(self):
        if self.h:
            self.lib.glome_ctx_destroy(self.h)
            self.h = None

    def err(self):
        return self.lib.glome_last_error(self.h).decode()

    def synchronize(self):
        if self.lib.glome_ctx_synchronize(self.h) != 0:
            raise GlomeError(self.err())

    def device_info(self):
        name = C.create_string_buffer(256)
        cu, ws = C.c_int(), C.c_int()
        self.lib.glome_ctx_device_info(self.h, name, 256, C.byref(cu), C.byref(ws))
        return name.value.decode(), cu.value, ws.value

    def _chk(self, rc, what):
        if rc != 0:
            raise GlomeError(f"{what}: {self.err()} (status {rc})")

    def camera_rays(self, cam, params, first_ray=0, n_rays=None):
        """The rays of `cam` under params' lens, made on the device (glome_camera_rays): (o, d) float32 arrays of n_rays rows, in the
        frame's order (y * width + x) * samples + s; the whole frame by default."""
        n = int(self.lib.glome_raygen_count(C.byref(params))) - first_ray if n_rays is None else int(n_rays)
        cols = [np.zeros(max(n, 0), np.float32) for _ in range(6)]
        self._chk(self.lib.glome_camera_rays(self.h, C.byref(cam), C.byref(params), int(first_ray), n, *[c.ctypes.data_as(L.c_fp) for c in cols]), "glome_camera_rays")
        return np.stack(cols[:3], 1), np.stack(cols[3:], 1)

    def camera_rays_dev(self, cam, params, first_ray, n_rays, ray_ptrs6):
        """Device-pointer raygen: ray_ptrs6 = ox, oy, oz, dx, dy, dz, n_rays floats each; asynchronous on the context's stream."""
        self._chk(self.lib.glome_camera_rays_dev(self.h, C.byref(cam), C.byref(params), int(first_ray), int(n_rays), *[C.c_void_p(p) if p else None for p in ray_ptrs6]),
                  "glome_camera_rays_dev")

    def resolve_dev(self, width, height, samples, first_pixel, n_pixels, samples_ptr, rgbad_ptr=None, packed_ptr=None):
        """Device-pointer resolve: samples_ptr = the n_pixels * samples * 5 floats a trace wrote for the range's rays; rgbad_ptr / packed_ptr
        = whole frames, either may be None / 0; asynchronous on the context's stream."""
        vp = lambda p: C.c_void_p(p) if p else None
        self._chk(self.lib.glome_resolve_dev(self.h, int(width), int(height), int(samples), int(first_pixel), int(n_pixels), vp(samples_ptr), vp(rgbad_ptr), vp(packed_ptr)),
                  "glome_resolve_dev")

    def bih(self, builder, ids):
        """`bih ids` built on this context's GPU (glome_sb_bih_dev): the node glome_sb_bih makes, tree bit for bit.
        Returns (node, device milliseconds)."""
        arr = (C.c_int32 * max(1, len(ids)))(*[int(i) for i in ids])
        ms = C.c_float(0)
        rc = self.lib.glome_sb_bih_dev(self.h, builder.h, arr, len(ids), C.byref(ms))
        if rc < 0:
            raise GlomeError(f"glome_sb_bih_dev: {self.err()} (status {rc})")
        return rc, ms.value

    def mesh(self, builder, verts, norms, tris, mats):
        """`mesh` with its BVH built on this context's GPU (glome_sb_mesh_dev).  Returns (node, device milliseconds)."""
        v = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 3))
        n = np.ascontiguousarray(np.asarray(norms, dtype=np.float64).reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(tris, dtype=np.int32).reshape(-1, 8))
        m = np.ascontiguousarray(np.asarray(mats, dtype=np.int32).ravel())
        ms = C.c_float(0)
        rc = self.lib.glome_sb_mesh_dev(self.h, builder.h, v.ctypes.data_as(L.c_dp), v.shape[0], n.ctypes.data_as(L.c_dp), n.shape[0],
                                        t.ctypes.data_as(L.c_ip), t.shape[0], m.ctypes.data_as(L.c_ip), m.shape[0], C.byref(ms))
        if rc < 0:
            raise GlomeError(f"glome_sb_mesh_dev: {self.err()} (status {rc})")
        return rc, ms.value

    def commit(self, builder, root):
        s = self.lib.glome_scene_commit(self.h, builder.h, int(root))
        if not s:
            raise GlomeError("glome_scene_commit: " + self.err())
        return Scene(self, s)


def _stats_dict(st):
    return {k: getattr(st, k) for k, _ in L.Stats._fields_}


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).ravel())


class Scene:
    def __init__(self, ctx, h):
        self.ctx, self.lib, self.h = ctx, ctx.lib, h

    def release(self):
        if self.h:
            self.lib.glome_scene_release(self.h)
            self.h = None

    def info(self):
        i = L.SceneInfo()
        self.lib.glome_scene_get_info(self.h, C.byref(i))
        return {k: getattr(i, k) for k, _ in L.SceneInfo._fields_}

    def _chk(self, rc, what):
        if rc != 0:
            raise GlomeError(f"{what}: {self.ctx.err()} (status {rc})")

    @staticmethod
    def _dev_arg(t, call, what, dtypes, per_row):
        """(pointer, rows) of a torch tensor handed to a device form, refused in the wording of the fp64 methods"""
        if not hasattr(t, "data_ptr") or not t.is_cuda or str(t.dtype) not in dtypes or not t.is_contiguous() or t.numel() % per_row:
            raise GlomeError(f"{call}: {what} must be a contiguous CUDA {' or '.join(dtypes)} tensor of {per_row} value{'s' if per_row > 1 else ''} per row")
        return (C.c_void_p(t.data_ptr()) if t.numel() else None), t.numel() // per_row

    def _host_update(self, fn, obj_id, arrays, args, ptr=_HOST_PTR):
        """The blocking host form `fn` (the library's function) of an update of object obj_id; returns its device milliseconds.  arrays:
        (values, numpy dtype, values per row) each, made contiguous; None stands for an array that is not given.  args(ptrs, rows) gives
        the C arguments between the object's id and the milliseconds, from the arrays' pointers (None for one of no rows: the count says
        that nothing is read) and row counts.  ptr: the pointer type by dtype."""
        held = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=dt).reshape(-1, w)) for a, dt, w in arrays]
        ptrs = [h.ctypes.data_as(ptr[dt]) if h is not None and h.shape[0] else None for h, (_, dt, _) in zip(held, arrays)]
        ms = C.c_float(0)
        self._chk(fn(self.h, int(obj_id), *args(ptrs, [0 if h is None else h.shape[0] for h in held]), C.byref(ms)), fn.__name__)
        return ms.value

    def mesh_update(self, mesh_id, verts, norms=None):
        """New vertices for a committed Mesh, its BVH refitted on the GPU (glome_scene_mesh_update): the scene a commit after
        Builder.mesh_set_vertices would have made.  NumPy arrays (or anything array-like) take the host form, which returns the device
        milliseconds of the finished update; CUDA torch.float64 tensors take the device form, asynchronous on the context's stream
        (returns None; the tensors must stay alive until it has run)."""
        return self._mesh_update("mesh_update", self.lib.glome_scene_mesh_update, self.lib.glome_scene_mesh_update_dev, np.float64, mesh_id, verts, norms)

    def _mesh_update(self, call, host, dev, dtype, mesh_id, verts, norms):
        """mesh_update / mesh_update_f32: the library's host and device form, arrays and tensors of `dtype`"""
        if hasattr(verts, "data_ptr"):  # torch tensors: the device form
            pv, nv = self._dev_arg(verts, call, "verts", _TORCH_NAME[dtype], 3)
            pn, nn = (None, 0) if norms is None else self._dev_arg(norms, call, "norms", _TORCH_NAME[dtype], 3)
            self._chk(dev(self.h, int(mesh_id), pv, nv, pn, nn), dev.__name__)
            return None
        return self._host_update(host, mesh_id, [(verts, dtype, 3), (norms, dtype, 3)], lambda p, n: (p[0], n[0], p[1], n[1]))

    def bih_update(self, bih_id, pts9):
        """New triangles for a committed triangle bih, its planes refitted on the GPU (glome_scene_bih_update): the scene a commit after
        Builder.bih_set_triangles would have made.  NumPy arrays (or anything array-like) take the host form, which returns the device
        milliseconds of the finished update; a CUDA torch.float64 tensor takes the device form, asynchronous on the context's stream
        (returns None; the tensor must stay alive until it has run)."""
        return self._one_array_update("bih_update", self.lib.glome_scene_bih_update, self.lib.glome_scene_bih_update_dev, np.float64, bih_id, pts9, "pts9", 9)

    def _dev_call(self, dev, bih_id, args, blocking):
        """the device form `dev` of a leaf bih call: an update's is asynchronous and returns None; a rebuild's (blocking) takes the
        milliseconds' address last and returns them"""
        ms = C.c_float(0)
        self._chk(dev(self.h, int(bih_id), *args, *([C.byref(ms)] if blocking else [])), dev.__name__)
        return ms.value if blocking else None

    def _one_array_update(self, call, host, dev, dtype, bih_id, values, what, per_row, blocking=False):
        """the leaf bih updates and rebuilds that take one array of per_row values per item: the library's host and device form.
        blocking: the device form, too, returns the device milliseconds (a rebuild's)"""
        if hasattr(values, "data_ptr"):  # a torch tensor: the device form
            return self._dev_call(dev, bih_id, self._dev_arg(values, call, what, _TORCH_NAME[dtype], per_row), blocking)
        return self._host_update(host, bih_id, [(values, dtype, per_row)], lambda p, n: (p[0], n[0]))

    def _indexed(self, call, host, dev, bih_id, verts, idx, blocking=False):
        """bih_update_indexed / bih_rebuild_indexed: the library's host and device form"""
        if hasattr(verts, "data_ptr") or hasattr(idx, "data_ptr"):  # torch tensors: the device form
            pv, nv = self._dev_arg(verts, call, "verts", ("torch.float32", "torch.float64"), 3)
            pi, n = self._dev_arg(idx, call, "idx", ("torch.int32",), 3)
            dtype = 1 if str(verts.dtype) == "torch.float32" else 0  # GLOME_F32 / GLOME_F64
            return self._dev_call(dev, bih_id, (pv, dtype, nv, pi, n), blocking)
        dtype = 1 if np.asarray(verts).dtype == np.float32 else 0
        return self._host_update(host, bih_id, [(verts, np.float32 if dtype else np.float64, 3), (idx, np.int32, 3)],
                                 lambda p, n: (p[0], dtype, n[0], p[1], n[1]), ptr={np.float32: C.c_void_p, np.float64: C.c_void_p, np.int32: L.c_ip})

    def sphere_bih_update(self, bih_id, c3r):
        """New centres and radii for a committed sphere bih, its planes refitted on the GPU (glome_scene_sphere_bih_update): the scene a
        commit after Builder.bih_set_spheres would have made.  NumPy arrays (or anything array-like) take the host form, which returns the
        device milliseconds of the finished update; a CUDA torch.float64 tensor takes the device form, asynchronous on the context's
        stream (returns None; the tensor must stay alive until it has run)."""
        return self._one_array_update("sphere_bih_update", self.lib.glome_scene_sphere_bih_update, self.lib.glome_scene_sphere_bih_update_dev, np.float64, bih_id, c3r, "c3r", 4)

    def bih_update_indexed(self, bih_id, verts, idx):
        """bih_update from the arrays a simulation holds (glome_scene_bih_update_indexed): vertices [nv, 3], float32 or float64, and an int32
        table [n, 3] of three vertex indices per item in update order.  The scene bih_update gives for the gathered, widened array, bit for
        bit; only referenced vertices count.  NumPy arrays take the host form (a float32 array is staged as float32, anything else as
        float64) and return the device milliseconds; CUDA torch tensors -- float32 or float64 vertices, int32 indices -- take the device
        form, asynchronous on the context's stream (returns None; the tensors must stay alive until it has run)."""
        return self._indexed("bih_update_indexed", self.lib.glome_scene_bih_update_indexed, self.lib.glome_scene_bih_update_indexed_dev, bih_id, verts, idx)

    def bih_rebuild(self, bih_id, pts9):
        """A committed triangle bih re-split in place from new triangles (glome_scene_bih_rebuild): the scene a commit after
        Builder.bih_set_triangles and Builder.bih_resplit would have made.  Arguments as bih_update; NOT asynchronous in either form: returns
        the device milliseconds when the scene is complete."""
        return self._one_array_update("bih_rebuild", self.lib.glome_scene_bih_rebuild, self.lib.glome_scene_bih_rebuild_dev, np.float64, bih_id, pts9, "pts9", 9, blocking=True)

    def sphere_bih_rebuild(self, bih_id, c3r):
        """A committed sphere bih re-split in place from new centres and radii (glome_scene_sphere_bih_rebuild); arguments as
        sphere_bih_update, blocking like bih_rebuild."""
        return self._one_array_update("sphere_bih_rebuild", self.lib.glome_scene_sphere_bih_rebuild, self.lib.glome_scene_sphere_bih_rebuild_dev, np.float64, bih_id, c3r, "c3r", 4, blocking=True)

    def bih_rebuild_indexed(self, bih_id, verts, idx):
        """bih_rebuild from a vertex array [nv, 3], float32 or float64, and an int32 table [n, 3] (glome_scene_bih_rebuild_indexed);
        arguments as bih_update_indexed, blocking like bih_rebuild."""
        return self._indexed("bih_rebuild_indexed", self.lib.glome_scene_bih_rebuild_indexed, self.lib.glome_scene_bih_rebuild_indexed_dev, bih_id, verts, idx, blocking=True)

    def bih_layout(self, bih_id):
        """A committed triangle or sphere bih as it stands (glome_scene_bih_layout): a dict of `slots`, `pairs`, `records`, `depth`, and the
        capacities `slot_cap` and `pair_cap` of its node and pair segments."""
        out = (C.c_int64 * 6)()
        self._chk(self.lib.glome_scene_bih_layout(self.h, int(bih_id), out), "glome_scene_bih_layout")
        return dict(zip(("slots", "pairs", "records", "depth", "slot_cap", "pair_cap"), (int(x) for x in out)))

    def bih_rebuild_stages(self):
        """the last rebuild's host wall-clock milliseconds by stage (glome_scene_bih_rebuild_stages): boxes, levels, tables, upload, values"""
        out = np.zeros(5)
        self._chk(self.lib.glome_scene_bih_rebuild_stages(self.h, out.ctypes.data_as(L.c_dp)), "glome_scene_bih_rebuild_stages")
        return dict(zip(("boxes", "levels", "tables", "upload", "values"), out.tolist()))

    def bih_update_f32(self, bih_id, pts9):
        """bih_update from float32 (glome_scene_bih_update_f32): nine values per item; the scene bih_update gives for the widened array, bit
        for bit.  NumPy arrays take the host form; a CUDA torch.float32 tensor takes the device form (returns None)."""
        return self._one_array_update("bih_update_f32", self.lib.glome_scene_bih_update_f32, self.lib.glome_scene_bih_update_f32_dev, np.float32, bih_id, pts9, "pts9", 9)

    def mesh_update_f32(self, mesh_id, verts, norms=None):
        """mesh_update from float32 (glome_scene_mesh_update_f32): the scene mesh_update gives for the widened arrays, bit for bit.  NumPy
        arrays take the host form; CUDA torch.float32 tensors take the device form (returns None)."""
        return self._mesh_update("mesh_update_f32", self.lib.glome_scene_mesh_update_f32, self.lib.glome_scene_mesh_update_f32_dev, np.float32, mesh_id, verts, norms)

    def sphere_bih_update_f32(self, bih_id, centres, radii):
        """sphere_bih_update from two float32 streams, centres [n, 3] and radii [n], as a particle system holds them
        (glome_scene_sphere_bih_update_f32): the scene sphere_bih_update gives for the widened, interleaved array, bit for bit.  NumPy
        arrays take the host form; CUDA torch.float32 tensors take the device form (returns None)."""
        def same(n, nr):
            if nr != n:
                raise GlomeError(f"sphere_bih_update_f32: {n} centres but {nr} radii")
            return n
        if hasattr(centres, "data_ptr") or hasattr(radii, "data_ptr"):
            pc, n = self._dev_arg(centres, "sphere_bih_update_f32", "centres", ("torch.float32",), 3)
            pr, nr = self._dev_arg(radii, "sphere_bih_update_f32", "radii", ("torch.float32",), 1)
            self._chk(self.lib.glome_scene_sphere_bih_update_f32_dev(self.h, int(bih_id), pc, pr, same(n, nr)), "glome_scene_sphere_bih_update_f32_dev")
            return None
        return self._host_update(self.lib.glome_scene_sphere_bih_update_f32, bih_id, [(centres, np.float32, 3), (radii, np.float32, 1)],
                                 lambda p, n: (p[0], p[1], same(n[0], n[1])))

    def instance_update(self, ids, xfms):
        """New matrices for committed Instances, the bih that holds them refitted on the GPU (glome_scene_instance_update): the scene a
        commit after Builder.instance_set_transforms would have made.  xfms: 24 values per id.  The host form; returns the device
        milliseconds of the finished update."""
        i, pi = L.ivec(ids)
        x = np.ascontiguousarray(np.asarray(xfms, dtype=np.float64).reshape(-1, 24))
        if x.shape[0] != len(i):
            raise GlomeError(f"instance_update: {len(i)} ids but {x.shape[0]} matrices")
        ms = C.c_float(0)
        self._chk(self.lib.glome_scene_instance_update(self.h, pi if len(i) else None, x.ctypes.data_as(L.c_dp) if len(i) else None, len(i), C.byref(ms)), "glome_scene_instance_update")
        return ms.value

    def instance_update_dev(self, ids, tensor):
        """The device form (glome_scene_instance_update_dev): ids a host list, `tensor` a contiguous CUDA torch.float64 tensor of 24 values
        per id; asynchronous on the context's stream (the tensor must stay alive until it has run)."""
        i, pi = L.ivec(ids)
        t = tensor
        if not hasattr(t, "data_ptr") or not t.is_cuda or str(t.dtype) != "torch.float64" or not t.is_contiguous() or t.numel() != 24 * len(i):
            raise GlomeError("instance_update_dev: the matrices must be a contiguous CUDA torch.float64 tensor of 24 values per id")
        self._chk(self.lib.glome_scene_instance_update_dev(self.h, pi if len(i) else None, C.c_void_p(t.data_ptr()) if len(i) else None, len(i)), "glome_scene_instance_update_dev")

    def instance_update_from(self, ids, data, form, base=None):
        """instance_update from what a rigid-body step holds (glome_scene_instance_update_from): form "pose" -- 8 values tx ty tz qx qy qz qw
        s per id --, "forward" -- a row-major 3x4 matrix, [n, 12], [n, 3, 4] or [n, 4, 4] (the fourth row is not read) --, or "pair" -- the
        24 values of instance_update.  The scene instance_update gives for xfm_from_pose / xfm_from_forward of the widened items, bit for
        bit.  base: None, or 24 float64 values per id; the item is then applied after it, xfm_mult(item, base[k]).  The inner dimensions
        must be contiguous; the stride between items is the array's own, so a column slice of a wider state array is read in place, and
        what lies between the items may be anything.  NumPy arrays take the host form (a float32 array is staged as float32, anything else
        as float64) and return the device milliseconds; CUDA torch tensors, float32 or float64 (base: float64, contiguous), take the
        device form, asynchronous on the context's stream (returns None; the tensors must stay alive until it has run)."""
        call = "instance_update_from"
        if form not in XFM_FORMS:
            raise GlomeError(f"{call}: form {form!r} is none of {sorted(XFM_FORMS)}")
        i, pi = L.ivec(ids)
        n = len(i)
        src = L.XfmSource()
        src.form = XFM_FORMS[form][0]
        if hasattr(data, "data_ptr") or hasattr(base, "data_ptr"):  # torch tensors: the device form
            t = data
            if not hasattr(t, "data_ptr") or not t.is_cuda or str(t.dtype) not in ("torch.float32", "torch.float64") or t.dim() < 2:
                raise GlomeError(f"{call}: data must be a CUDA torch.float32 or torch.float64 tensor of one row per id")
            stride = _xfm_stride(call, form, tuple(t.shape), tuple(t.stride()))
            if stride is None:
                raise GlomeError(f"{call}: the inner dimensions of data must be contiguous and its rows must not overlap (strides {tuple(t.stride())})")
            if base is not None:
                if not hasattr(base, "data_ptr") or not base.is_cuda or str(base.dtype) != "torch.float64" or not base.is_contiguous() or base.numel() != 24 * n:
                    raise GlomeError(f"{call}: base must be a contiguous CUDA torch.float64 tensor of 24 values per id")
                src.base = base.data_ptr() if n else None
            if t.shape[0] != n:
                raise GlomeError(f"{call}: {n} ids but {t.shape[0]} items")
            src.data, src.dtype, src.stride = (t.data_ptr() if n else None), (L.F32 if str(t.dtype) == "torch.float32" else L.F64), stride
            self._chk(self.lib.glome_scene_instance_update_from_dev(self.h, pi if n else None, C.byref(src), n), "glome_scene_instance_update_from_dev")
            return None
        a = np.asarray(data)
        a = np.asarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
        if a.ndim < 2:
            a = a.reshape(-1, XFM_FORMS[form][1])
        stride = _xfm_stride(call, form, a.shape, tuple(s // a.itemsize if s % a.itemsize == 0 else -1 for s in a.strides))
        if stride is None:  # (a layout the library does not read in place: a dense copy)
            a = np.ascontiguousarray(a)
            stride = 0
        if a.shape[0] != n:
            raise GlomeError(f"{call}: {n} ids but {a.shape[0]} items")
        held = None
        if base is not None:
            held = np.ascontiguousarray(np.asarray(base, dtype=np.float64).reshape(-1, 24))
            if held.shape[0] != n:
                raise GlomeError(f"{call}: {n} ids but {held.shape[0]} base matrices")
            src.base = held.ctypes.data if n else None
        src.data, src.dtype, src.stride = (a.ctypes.data if n else None), (L.F32 if a.dtype == np.float32 else L.F64), stride
        ms = C.c_float(0)
        self._chk(self.lib.glome_scene_instance_update_from(self.h, pi if n else None, C.byref(src), n, C.byref(ms)), "glome_scene_instance_update_from")
        return ms.value

    def nested_updates(self, on=True):
        """The switch of glome_scene_nested_updates: with it on, the three updates accept objects that lie under bihs, leave the trees above
        them stale, and bih_refit makes those trees again, one call per tree, inner trees first (refit_above does the walk)."""
        self._chk(self.lib.glome_scene_nested_updates(self.h, 1 if on else 0), "glome_scene_nested_updates")

    def bih_refit(self, bih_id):
        """One tree refitted from the current bounds of the objects its items hang on (glome_scene_bih_refit, the host form): returns the
        device milliseconds of the finished refit."""
        ms = C.c_float(0)
        self._chk(self.lib.glome_scene_bih_refit(self.h, int(bih_id), C.byref(ms)), "glome_scene_bih_refit")
        return ms.value

    def bih_refit_dev(self, bih_id):
        """The device form (glome_scene_bih_refit_dev): asynchronous on the context's stream, after the updates enqueued before it."""
        self._chk(self.lib.glome_scene_bih_refit_dev(self.h, int(bih_id)), "glome_scene_bih_refit_dev")

    def _id_list(self, fn, what, *args):
        n = fn(self.h, *args, None, 0)
        if n < 0:
            self._chk(n, what)
        out = np.zeros(max(1, n), np.int32)
        fn(self.h, *args, out.ctypes.data_as(L.c_ip), n)
        return [int(x) for x in out[:n]]

    def bihs_above(self, node):
        """the bihs above `node` in this scene, in an order in which they can be refitted (glome_scene_bihs_above)"""
        return self._id_list(self.lib.glome_scene_bihs_above, "glome_scene_bihs_above", int(node))

    def stale_bihs(self):
        """the bihs an update has left stale, in an order in which they can be refitted (glome_scene_stale_bihs)"""
        return self._id_list(self.lib.glome_scene_stale_bihs, "glome_scene_stale_bihs")

    def refit_above(self, node, dev=False):
        """bih_refit of every bih above `node`, inner trees first; returns the summed device milliseconds (None in the device form)"""
        total = 0.0
        for b in self.bihs_above(node):
            if dev:
                self.bih_refit_dev(b)
            else:
                total += self.bih_refit(b)
        return None if dev else total

    def _rays(self, o, d, tmax):
        o = np.asarray(o, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(d, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        tm = np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,))
        cols = [_f32(o[:, 0]), _f32(o[:, 1]), _f32(o[:, 2]), _f32(d[:, 0]), _f32(d[:, 1]), _f32(d[:, 2]), _f32(tm)]
        return n, cols

    def rayint(self, o, d, tmax=1000000.0):
        """rayint over a batch (Solid.hs:146-151): returns dict t (-1 = miss), prim, n (nx3), tex (nx8: the stack innermost first, -1 padded)."""
        n, cols = self._rays(o, d, tmax)
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32)
        nx = np.zeros(n, np.float32); ny = np.zeros(n, np.float32); nz = np.zeros(n, np.float32)
        tex = np.zeros((n, self.lib.glome_tex_words()), np.int32)  # (8: GLOME_TEX_WORDS of the loaded library)
        self._chk(self.lib.glome_rayint_batch(self.h, n, *[c.ctypes.data_as(L.c_fp) for c in cols], t.ctypes.data_as(L.c_fp),
                                              prim.ctypes.data_as(L.c_ip), nx.ctypes.data_as(L.c_fp), ny.ctypes.data_as(L.c_fp),
                                              nz.ctypes.data_as(L.c_fp), tex.ctypes.data_as(L.c_ip)), "glome_rayint_batch")
        return {"t": t, "prim": prim, "n": np.stack([nx, ny, nz], 1), "tex": tex}

    def shadow(self, o, d, tmax):
        n, cols = self._rays(o, d, tmax)
        occ = np.zeros(n, np.uint8)
        self._chk(self.lib.glome_shadow_batch(self.h, n, *[c.ctypes.data_as(L.c_fp) for c in cols], occ.ctypes.data_as(L.c_bp)), "glome_shadow_batch")
        return occ.astype(bool)

    def inside(self, p):
        p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
        n = p.shape[0]
        ins = np.zeros(n, np.uint8)
        cols = [_f32(p[:, 0]), _f32(p[:, 1]), _f32(p[:, 2])]
        self._chk(self.lib.glome_inside_batch(self.h, n, *[c.ctypes.data_as(L.c_fp) for c in cols], ins.ctypes.data_as(L.c_bp)), "glome_inside_batch")
        return ins.astype(bool)

    def trace(self, o, d, lights, tmax=None, params=None, want_hit=False):
        """Trace.trace over a batch of rays (Trace.hs:59-82): returns dict rgba (nx4), depth (n; 1e6 = miss), stats, and with want_hit
        the trace's own Rayint t, prim, n, tex as `rayint` returns them.  Directions are used as given: unit length, or params.faithful."""
        o = np.asarray(o, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(d, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        cols = [_f32(o[:, 0]), _f32(o[:, 1]), _f32(o[:, 2]), _f32(d[:, 0]), _f32(d[:, 1]), _f32(d[:, 2])]
        tm = None if tmax is None else _f32(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))
        params = trace_params() if params is None else params
        out = np.zeros((n, 5), np.float32)
        hit, hp = {}, [None] * 6
        if want_hit:
            t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32)
            nx = np.zeros(n, np.float32); ny = np.zeros(n, np.float32); nz = np.zeros(n, np.float32)
            tex = np.zeros((n, self.lib.glome_tex_words()), np.int32)
            hp = [t.ctypes.data_as(L.c_fp), prim.ctypes.data_as(L.c_ip), nx.ctypes.data_as(L.c_fp), ny.ctypes.data_as(L.c_fp), nz.ctypes.data_as(L.c_fp),
                  tex.ctypes.data_as(L.c_ip)]
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_trace_batch(self.h, n, *[c.ctypes.data_as(L.c_fp) for c in cols], tm.ctypes.data_as(L.c_fp) if tm is not None else None,
                                             la, len(lights), C.byref(params), out.ctypes.data_as(L.c_fp), *hp, C.byref(st)), "glome_trace_batch")
        if want_hit:
            hit = {"t": t, "prim": prim, "n": np.stack([nx, ny, nz], 1), "tex": tex}
        return {"rgba": out[:, :4], "depth": out[:, 4], "stats": _stats_dict(st), **hit}

    def trace_dev(self, n, ray_ptrs7, lights, params, rgbad_ptr, hit_ptrs=None, want_stats=True):
        """Device-pointer trace: ray_ptrs7 = ox, oy, oz, dx, dy, dz, tmax (tmax may be None / 0); hit_ptrs = t, prim, nx, ny, nz, tex8 (any may be
        None / 0); asynchronous on the context's stream unless want_stats."""
        vp = lambda p: C.c_void_p(p) if p else None
        hit = list(hit_ptrs) if hit_ptrs is not None else [None] * 6
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_trace_batch_dev(self.h, int(n), *[vp(p) for p in ray_ptrs7], la, len(lights), C.byref(params), vp(rgbad_ptr),
                                                 *[vp(p) for p in hit], C.byref(st) if want_stats else None), "glome_trace_batch_dev")
        return _stats_dict(st) if want_stats else None

    def trace_work(self, o, d, lights, tmax=None, params=None):
        """Trace.trace_debug over a batch of rays (Trace.hs:84-109): `trace` with a record of each ray's work.  Returns dict work (n x 8
        uint32, the words WORK_* name), rgba, depth, stats.  params.count_work is implied."""
        o = np.asarray(o, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(d, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        cols = [_f32(o[:, 0]), _f32(o[:, 1]), _f32(o[:, 2]), _f32(d[:, 0]), _f32(d[:, 1]), _f32(d[:, 2])]
        tm = None if tmax is None else _f32(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,)))
        params = trace_params() if params is None else params
        out = np.zeros((n, 5), np.float32)
        work = np.zeros((n, self.lib.glome_work_words()), np.uint32)
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_trace_work_batch(self.h, n, *[c.ctypes.data_as(L.c_fp) for c in cols], tm.ctypes.data_as(L.c_fp) if tm is not None else None,
                                                  la, len(lights), C.byref(params), out.ctypes.data_as(L.c_fp), work.ctypes.data_as(L.c_up), C.byref(st)),
                  "glome_trace_work_batch")
        return {"work": work, "rgba": out[:, :4], "depth": out[:, 4], "stats": _stats_dict(st)}

    def trace_work_dev(self, n, ray_ptrs7, lights, params, work_ptr, rgbad_ptr=None, want_stats=True):
        """Device-pointer trace_work: ray_ptrs7 as trace_dev takes them; work_ptr: n * 8 uint32, 16-byte aligned; rgbad_ptr may be None / 0
        (no colour is stored); asynchronous on the context's stream unless want_stats."""
        vp = lambda p: C.c_void_p(p) if p else None
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_trace_work_batch_dev(self.h, int(n), *[vp(p) for p in ray_ptrs7], la, len(lights), C.byref(params), vp(rgbad_ptr),
                                                      vp(work_ptr), C.byref(st) if want_stats else None), "glome_trace_work_batch_dev")
        return _stats_dict(st) if want_stats else None

    def cost_image(self, cam, lights, width, height, maxdepth=3, faithful=0):
        """A frame's work records, (height, width, 8) uint32: the frame's primary rays (frame_rays) through trace_work.  Word 5 is what
        GlomeView's debug view tints a pixel with (get_color_debug, Glome.hs:35-41)."""
        o, d = frame_rays(cam, width, height)
        r = self.trace_work(o, d, lights, params=trace_params(maxdepth=maxdepth, faithful=faithful))
        return r["work"].reshape(height, width, -1)

    def render_lens(self, cam, lights, raygen, trace=None, rays_per_pass=0, want_packed=True):
        """A frame of `cam` under raygen's lens through the trace seam, rays made and samples resolved on the device (glome_render_lens):
        returns (rgbad[h,w,5] float32, packed[h,w] uint32 or None, stats dict), like render."""
        w, h = raygen.width, raygen.height
        img = np.zeros((max(h, 0), max(w, 0), 5), np.float32)
        packed = np.zeros((max(h, 0), max(w, 0)), np.uint32) if want_packed else None
        trace = trace_params() if trace is None else trace
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_render_lens(self.h, C.byref(cam), C.byref(raygen), la, len(lights), C.byref(trace), int(rays_per_pass), img.ctypes.data_as(L.c_fp),
                                             packed.ctypes.data_as(L.c_up) if want_packed else None, C.byref(st)), "glome_render_lens")
        return img, packed, _stats_dict(st)

    def render_lens_dev(self, cam, lights, raygen, trace, rgbad_ptr, packed_ptr=None, rays_per_pass=0, want_stats=True):
        """Device-pointer render_lens (whole frames; either pointer may be None / 0); asynchronous unless want_stats."""
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_render_lens_dev(self.h, C.byref(cam), C.byref(raygen), la, len(lights), C.byref(trace), int(rays_per_pass),
                                                 C.c_void_p(rgbad_ptr) if rgbad_ptr else None, C.c_void_p(packed_ptr) if packed_ptr else None,
                                                 C.byref(st) if want_stats else None), "glome_render_lens_dev")
        return _stats_dict(st) if want_stats else None

    def render_lens_adaptive(self, cam, lights, raygen, adaptive=None, trace=None, rays_per_pass=0, want_packed=True):
        """render_lens with raygen.samples the most a pixel gets and fewer where the halves of its samples agree
        (glome_render_lens_adaptive): returns (rgbad[h,w,5] float32, packed[h,w] uint32 or None, counts[h,w] uint8, stats dict).  Every
        pixel is adaptive_fold of its samples, bit for bit."""
        w, h = raygen.width, raygen.height
        img = np.zeros((max(h, 0), max(w, 0), 5), np.float32)
        packed = np.zeros((max(h, 0), max(w, 0)), np.uint32) if want_packed else None
        counts = np.zeros((max(h, 0), max(w, 0)), np.uint8)
        trace = trace_params() if trace is None else trace
        adaptive = adaptive_params() if adaptive is None else adaptive
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_render_lens_adaptive(self.h, C.byref(cam), C.byref(raygen), la, len(lights), C.byref(trace), C.byref(adaptive), int(rays_per_pass),
                                                      img.ctypes.data_as(L.c_fp), packed.ctypes.data_as(L.c_up) if want_packed else None,
                                                      counts.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st)), "glome_render_lens_adaptive")
        return img, packed, counts, _stats_dict(st)

    def render_lens_adaptive_dev(self, cam, lights, raygen, adaptive, trace, rgbad_ptr, packed_ptr=None, counts_ptr=None, rays_per_pass=0, want_stats=True):
        """Device-pointer render_lens_adaptive (whole frames; any pointer may be None / 0, rgbad_ptr and packed_ptr not both).  Not
        asynchronous: the call waits for the stream once per round of each pass."""
        vp = lambda p: C.c_void_p(p) if p else None
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_render_lens_adaptive_dev(self.h, C.byref(cam), C.byref(raygen), la, len(lights), C.byref(trace), C.byref(adaptive),
                                                          int(rays_per_pass), vp(rgbad_ptr), vp(packed_ptr), vp(counts_ptr), C.byref(st) if want_stats else None),
                  "glome_render_lens_adaptive_dev")
        return _stats_dict(st) if want_stats else None

    def render(self, cam, lights, params, want_packed=True, init=None):
        """renderTiles (Glome.hs:379-386): returns (rgbad[h,w,5] float32, packed[h,w] uint32 or None, stats dict)."""
        w, h = params.width, params.height
        img = np.zeros((h, w, 5), np.float32) if init is None else np.ascontiguousarray(init, dtype=np.float32)
        packed = np.zeros((h, w), np.uint32) if want_packed else None
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_render(self.h, C.byref(cam), la, len(lights), C.byref(params), img.ctypes.data_as(L.c_fp),
                                        packed.ctypes.data_as(L.c_up) if want_packed else None, C.byref(st)), "glome_render")
        return img, packed, _stats_dict(st)

    def render_dev(self, cam, lights, params, rgbad_ptr, packed_ptr=None, want_stats=True):
        """Device-pointer render (e.g. a torch tensor's data_ptr()); asynchronous unless want_stats."""
        la = (L.Light * max(1, len(lights)))(*lights)
        st = L.Stats()
        self._chk(self.lib.glome_render_dev(self.h, C.byref(cam), la, len(lights), C.byref(params), C.c_void_p(rgbad_ptr) if rgbad_ptr else None,
                                            C.c_void_p(packed_ptr) if packed_ptr else None, C.byref(st) if want_stats else None), "glome_render_dev")
        return _stats_dict(st) if want_stats else None


class Multi:
    """Several GPUs driven by this one process (glome_multi_*): scenes[i] is the scene committed on context i; frames land
    on scenes[0]'s device.  The one-process counterpart of dist.ShardedFrame (one process per GPU)."""

    def __init__(self, scenes, params, use_rccl=True, transport=None):
        """transport: "direct" (ranks store straight into rank 0's framebuffer), "rccl", "peer-copy"; default: rccl when use_rccl else peer-copy"""
        self.lib = scenes[0].lib
        self.scenes = list(scenes)
        arr = (C.c_void_p * len(scenes))(*[s.h for s in scenes])
        code = {"direct": 2, "rccl": 1, "peer-copy": 0}[transport] if transport is not None else (1 if use_rccl else 0)
        self.h = self.lib.glome_multi_create(arr, len(scenes), C.byref(params), code)
        if not self.h:
            raise GlomeError("glome_multi_create: " + self.lib.glome_global_error().decode())
        self.params = params

    def transport(self):
        return self.lib.glome_multi_transport(self.h).decode()

    def render(self, cams, lights, packed_ptr):
        """cams: one glome_camera or a list of up to 32; packed_ptr: device pointer on rank 0's GPU (frames back to back)"""
        cams = list(cams) if isinstance(cams, (list, tuple)) else [cams]
        ca = (L.Camera * len(cams))(*cams)
        la = (L.Light * max(1, len(lights)))(*lights)
        rc = self.lib.glome_multi_render(self.h, ca, len(cams), la, len(lights), C.c_void_p(packed_ptr))
        if rc != 0:
            raise GlomeError(f"glome_multi_render: {self.lib.glome_multi_last_error(self.h).decode()} (status {rc})")

    def synchronize(self):
        rc = self.lib.glome_multi_synchronize(self.h)
        if rc != 0:
            raise GlomeError(f"glome_multi_synchronize: {self.lib.glome_multi_last_error(self.h).decode()} (status {rc})")

    def close(self):
        if self.h:
            self.lib.glome_multi_destroy(self.h)
            self.h = None
