/* glome_hip.h -- C ABI of libglome_hip.so: the MI355X (gfx950) ray-tracing core that replaces
 * glome's per-ray hot path behind glome's own constructor vocabulary.
 *
 * The reference (jimsnow/glome, Haskell) has no FFI boundary of its own; the seams this library
 * sits behind are (paths relative to the reference tree):
 *   - the `Solid` class methods  rayint / shadow / inside   GlomeTrace/Data/Glome/Solid.hs:146-166
 *   - the tile map               renderTiles                 GlomeView/Glome.hs:379-386
 *   - the ray tracer's entry     trace                       GlomeTrace/Data/Glome/Trace.hs:53-82
 *   - the scene constructors     sphere, triangle, box, ...  (cited per function below)
 * Each entry point cites the reference interface it replaces.  INTEGRATION.md shows the Haskell
 * `foreign import ccall` stubs a maintainer would add.
 *
 * Conventions
 *   - Every function returning `int` returns 0 on success, <0 (a glome_status) on error; builder
 *     functions returning int32_t return a node/material id >= 0, or <0 on error.  The message is
 *     read with glome_sb_last_error / glome_last_error.  No C++ exception crosses the boundary.
 *   - Scene constants cross as `double` (glome's `Flt = Double`, Vec.hs:9); the device computes in
 *     fp32.  Ray / hit / framebuffer arrays are caller-owned fp32 SoA buffers, valid for the call.
 *   - `_dev` variants take DEVICE pointers and run asynchronously on the context's HIP stream.
 *   - A glome_ctx owns one device + one stream and is single-threaded; distinct contexts may be
 *     driven from distinct threads.  A glome_scene is immutable after commit, but for the vertices of its
 *     meshes (glome_scene_mesh_update), the items of its triangle and sphere bihs (glome_scene_bih_update,
 *     glome_scene_sphere_bih_update) and those trees' own topology (glome_scene_bih_rebuild), the matrices of its
 *     Instances (glome_scene_instance_update) and the planes of the bihs above them (glome_scene_bih_refit).
 *   - There is NO CPU fallback: every compute entry point fails with GLOME_E_NO_DEVICE when no
 *     gfx950 device is usable.  Builder and flatten-inspection calls are host-only.
 */
#ifndef GLOME_HIP_H
#define GLOME_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct glome_ctx glome_ctx;     /* one GPU + one HIP stream */
typedef struct glome_sb glome_sb;       /* scene builder: the host-side scene graph */
typedef struct glome_scene glome_scene; /* flattened scene resident in HBM */

enum glome_status {
  GLOME_OK = 0,
  GLOME_E_INVALID = -1,   /* bad argument / bad id */
  GLOME_E_SCENE = -2,     /* scene validation failed (infinite bound in bih, corrupt matrix, ...) */
  GLOME_E_NO_DEVICE = -3, /* no usable gfx950 device */
  GLOME_E_HIP = -4,       /* HIP runtime error */
  GLOME_E_LIMIT = -5      /* scene exceeds a device-side limit (texture stack, frame memory, ...) */
};

/* ---- context ---- */
/* The context launches on a stream of its own, created as a blocking stream: it is ordered against the device's default
 * (null) stream in both directions, so buffers a caller prepared there may be handed to the *_dev entry points directly.
 * Work on the caller's own non-blocking streams is the caller's to order (or the stream is given to glome_ctx_use_slot). */
glome_ctx* glome_ctx_create(int device_ordinal); /* NULL on failure; see glome_global_error() */
void glome_ctx_destroy(glome_ctx*);
const char* glome_last_error(const glome_ctx*);
const char* glome_global_error(void);  /* error text when no ctx/sb exists yet */
void* glome_ctx_stream(glome_ctx*);    /* the hipStream_t, for interop */
int glome_ctx_synchronize(glome_ctx*);
/* Run on an external HIP stream (e.g. torch's current stream) instead of the context's own; NULL restores it. */
int glome_ctx_use_stream(glome_ctx*, void* hip_stream);
/* Several frames in flight: a context has 8 launch slots, each with its own work queue, counters and workspaces.  Select
 * (stream, slot) before a launch; launches that may overlap in time must use different slots (and streams). */
int glome_ctx_use_slot(glome_ctx*, void* hip_stream, int slot);
/* Per-launch kernel timing without extra synchronisation: between begin and end every render launch records its own
 * HIP-event pair on the context's stream; end synchronises once and returns the number of launches, writing their
 * durations (ms) to ms_out[0..cap). */
int glome_ctx_timing_begin(glome_ctx*, int max_launches);
/* The same, but only every `stride`-th render launch carries an event pair: event records are extra packets on the
 * launch stream and cost frame rate when a frame is a fraction of a millisecond. */
int glome_ctx_timing_begin_sampled(glome_ctx*, int max_launches, int stride);
int glome_ctx_timing_end(glome_ctx*, float* ms_out, int cap);
/* Waves per CU of the persistent render launches.  0 (default): sized by the launch's work, for several launches in flight
 * on separate slots (each takes a share of the CUs' wave slots); n > 0: n per CU, resources permitting -- what a launch
 * that runs ALONE wants (24 for the packet instances).  The reference has no such knob (GHC's +RTS -N is the nearest). */
int glome_ctx_set_grid_per_cu(glome_ctx*, int waves_per_cu);
int glome_ctx_device_info(glome_ctx*, char* name, int cap, int* cu_count, int* warp_size);

/* ---- transforms: Xfm = forward 3x4 (12 doubles, row major) + inverse 3x4 (12 doubles) ---- */
int glome_xfm_translate(const double v[3], double out[24]);                          /* Vec.hs:564-567 */
int glome_xfm_scale(const double v[3], double out[24]);                              /* Vec.hs:571-574 */
int glome_xfm_rotate(const double axis[3], double angle_rad, double out[24]);        /* Vec.hs:577-598 */
int glome_xfm_xyz_to_uvw(const double u[3], const double v[3], const double w[3], double out[24]); /* Vec.hs:602-622 */
int glome_xfm_compose(const double* xfms /* n*24 */, int n, double out[24]);         /* Vec.hs:461-462 */
/* An Xfm from what a producer of rigid motion holds, and the product of two.  Host only: the specification of
 * glome_scene_instance_update_from, whose device side evaluates the same expressions.  Every operation below is one round-to-nearest
 * fp64 operation, in the order written, sums left to right, and nothing contracts: the results are defined to the bit.
 *   glome_xfm_from_pose(t, q, s): the forward map p -> t + s R(q) p, q = (qx, qy, qz, qw) with the scalar LAST, any length but 0, s a
 *     uniform scale.
 *       inv = 1 / sqrt(((qx qx + qy qy) + qz qz) + qw qw);   x, y, z, w = qx inv, qy inv, qz inv, qw inv
 *       R = [[1 - 2 (yy + zz), 2 (xy - zw), 2 (xz + yw)], [2 (xy + zw), 1 - 2 (xx + zz), 2 (yz - xw)], [2 (xz - yw), 2 (yz + xw), 1 - 2 (xx + yy)]]
 *     (xx = x x and so on, each product made once; the products by 2 are exact).
 *       forward row r: (s R[r][0], s R[r][1], s R[r][2], t[r])
 *       inverse row r: i[r][c] = R[c][r] / s for c < 3 -- a division, not a product by 1 / s --, i[r][3] = -(((i[r][0] tx) + (i[r][1] ty)) + (i[r][2] tz))
 *     GLOME_E_INVALID, out untouched: a value that is not finite, q of length 0 (the sum of squares is 0), s <= 0, a result that is not finite.
 *   glome_xfm_from_forward(m12): m12 a row-major 3x4 forward matrix, A = a[r][c] its 3x3 part, t its column 3.  The forward rows are m12.
 *       c00 = a11 a22 - a12 a21   c01 = a12 a20 - a10 a22   c02 = a10 a21 - a11 a20
 *       c10 = a02 a21 - a01 a22   c11 = a00 a22 - a02 a20   c12 = a01 a20 - a00 a21
 *       c20 = a01 a12 - a02 a11   c21 = a02 a10 - a00 a12   c22 = a00 a11 - a01 a10
 *       det = ((a00 c00) + (a01 c01)) + (a02 c02)
 *       inverse row r: i[r][c] = c[c][r] / det for c < 3 (the transposed cofactor matrix, each entry DIVIDED by det), i[r][3] as for the pose.
 *     GLOME_E_INVALID for a value that is not finite; GLOME_E_SCENE when det is 0 or an entry of the inverse is not finite; out untouched.
 *   glome_xfm_mult(a, b): a applied AFTER b, xfm_mult a b (Vec.hs:447-449): forward = mat_mult a.forward b.forward, inverse = mat_mult
 *     b.inverse a.inverse, mat_mult (Vec.hs:426-443) with every entry ((x0 y0 + x1 y1) + x2 y2) and column 3 (((x0 y0 + x1 y1) + x2 y2) + x3).
 *     It is the step glome_xfm_compose folds from an identity; without the identity it never changes the sign of a zero, and it does not
 *     run check_xfm.  out may be a or b. */
int glome_xfm_from_forward(const double m12[12], double out[24]);
int glome_xfm_from_pose(const double t[3], const double q_xyzw[4], double s, double out[24]);
int glome_xfm_mult(const double a[24], const double b[24], double out[24]);

/* ---- scene builder: one call per reference constructor ---- */
glome_sb* glome_sb_new(void);
void glome_sb_free(glome_sb*);
const char* glome_sb_last_error(const glome_sb*);
int32_t glome_sb_sphere(glome_sb*, const double c[3], double r);                                 /* Sphere.hs:15-17 */
int32_t glome_sb_triangle(glome_sb*, const double p[9]);                                         /* Triangle.hs:18-20 */
int32_t glome_sb_trianglenorm(glome_sb*, const double p[9], const double n[9]);                  /* Triangle.hs:34-35 */
int32_t glome_sb_box(glome_sb*, const double a[3], const double b[3]);                           /* Box.hs:12-15 */
int32_t glome_sb_plane(glome_sb*, const double pt[3], const double n[3]);                        /* Plane.hs:17-20 */
int32_t glome_sb_plane_offset(glome_sb*, const double n[3], double off);                         /* Plane.hs:24-25 */
int32_t glome_sb_disc(glome_sb*, const double pos[3], const double n[3], double r);              /* Cone.hs:29-31 */
int32_t glome_sb_cylinder(glome_sb*, const double p1[3], const double p2[3], double r);          /* Cone.hs:40-48 */
int32_t glome_sb_cone(glome_sb*, const double p1[3], double r1, const double p2[3], double r2);  /* Cone.hs:52-67 */
int32_t glome_sb_group(glome_sb*, const int32_t* ids, int n);                                    /* Solid.hs:293-296 */
int32_t glome_sb_transform(glome_sb*, int32_t id, const double* xfms /* n*24 */, int n);         /* Solid.hs:184,235 */
int32_t glome_sb_difference(glome_sb*, int32_t a, int32_t b);                                    /* Csg.hs:26-27 */
int32_t glome_sb_difference_retexture(glome_sb*, int32_t a, int32_t b);                          /* Csg.hs:29-30: `Difference a b False` -- the surface hollowed out by b keeps b's textures (Csg.hs:42-43) */
int32_t glome_sb_intersection(glome_sb*, const int32_t* ids, int n);                             /* Csg.hs:64-65 */
/* GLOME_E_SCENE, no node added, for an infinite box (Bih.hs:319-322) and for an input on which the reference's build_rec does not
 * terminate: a node of more than three items whose chosen partition leaves one side empty and the other child's box unchanged (a
 * box of zero or underflowing surface area: four points on a line).  glome_sb_mesh refuses build_tree's fixed point (a vertex at
 * infinity) the same way; glome_sb_load_nff / glome_sb_load_show go through the same constructors. */
int32_t glome_sb_bih(glome_sb*, const int32_t* ids, int n);                                      /* Bih.hs:309-324 */
/* tris: 8 ints per triangle = a b c na nb nc tex tag (-1 = none), Mesh.hs:27-29; mats = the mesh's texture vector */
int32_t glome_sb_mesh(glome_sb*, const double* verts, int nv, const double* norms, int nn,
                      const int32_t* tris, int nt, const int32_t* mats, int nm);                 /* Mesh.hs:50-55 */
/* Same tree, new vertices.  mesh_id names a Mesh node, whoever made it (glome_sb_mesh, glome_sb_mesh_dev, glome_sb_load_show); nv and
 * nn are the mesh's own counts; norms may be NULL when nn == 0; every coordinate is finite.  Replaces the mesh's vertex and normal
 * arrays and makes again what `mesh` derives from them: every triangle's box (Mesh.hs:119-121), every branch's two boxes as the true
 * unions of the triangle boxes below them (Mesh.hs:89-96), and the mesh's box over ALL vertices, unreferenced ones included
 * (Mesh.hs:55).  What build_tree decided -- nodes, leaf lists, depth -- stays: no triangle changes leaf, so a tree built for one pose
 * serves the next one less well the further the vertices move (glome_sb_mesh again re-splits).  glome_sb_bound, glome_sb_show and a later
 * commit see the new mesh; a `bih` built over the mesh earlier keeps the planes it was built with.  The reference has no such call
 * (`mesh` is a pure constructor); the result is the Mesh the reference would print for the same tree with the new arrays.  Anything
 * else is GLOME_E_INVALID with a message, and the mesh is left untouched.  Host only; the specification of glome_scene_mesh_update. */
int glome_sb_mesh_set_vertices(glome_sb*, int32_t mesh_id, const double* verts, int nv, const double* norms, int nn);
/* Same tree, new triangles.  bih_id names a Bih node, whoever made it (glome_sb_bih, glome_sb_bih_dev, glome_sb_load_show, glome_sb_load_nff);
 * n is its item count and pts9 holds nine doubles per item, p1 p2 p3, every one finite.  Item k is the k-th id of the list the bih was
 * built from; for a tree read by glome_sb_load_show, the k-th leaf item in preorder (glome_sb_bih_items returns the ids in this order).
 * Every item must be a Triangle under any number of Tex / Tag / NoShadow / OnlyShadow wrappers, and no Triangle node may be an item
 * twice.  Sets the item triangles' vertices (a Triangle node that is also used elsewhere in the builder moves there too) and makes again
 * what `bih` derives from its items' bounds: every branch's lsplit = (max over the left subtree of the items' box hi[axis]) + delta and
 * rsplit = (min over the right subtree of lo[axis]) - delta (Bih.hs:243-250, 285), and the tree's box.  What the builder decided -- nodes,
 * axes, leaf lists, depth -- stays.  The tree stays correct: the traversal enters a child when the ray's interval, which starts from the
 * tree's box, reaches the half-space below lsplit / above rsplit, whichever item sits in which leaf; only its quality degrades the
 * further the triangles move (glome_sb_bih again re-splits).  glome_sb_bound, glome_sb_show, glome_sb_bih_dump and a later commit see the
 * new tree; a `bih` built earlier over this one keeps the planes it was built with.  The reference has no such call (`bih` is a pure
 * constructor); the result is the Bih the reference would print for the same tree with the new triangles.  Anything else is
 * GLOME_E_INVALID with a message (an item that is not a plain triangle is named), and nothing is touched.  Host only; the specification
 * of glome_scene_bih_update. */
int glome_sb_bih_set_triangles(glome_sb*, int32_t bih_id, const double* pts9, int n);
/* The same from a vertex array and an index table, as a simulation holds a mesh: verts holds nv vertices of three doubles, idx3 three
 * vertex indices per item, items in update order.  It is glome_sb_bih_set_triangles of the gathered array, pts9[9 k + 3 c ..] =
 * verts[3 * idx3[3 k + c] ..], and refuses what that call refuses.  Only REFERENCED vertices count: a vertex no item names may be
 * anything, not finite included, and takes no part in the tree's box.  An index outside [0, nv) is GLOME_E_INVALID, the message naming
 * the item, and nothing is touched.  Host only; the specification of glome_scene_bih_update_indexed. */
int glome_sb_bih_set_triangles_indexed(glome_sb*, int32_t bih_id, const double* verts, int nv, const int32_t* idx3, int n);
/* Same tree, new spheres: glome_sb_bih_set_triangles for a bih of spheres.  bih_id names a Bih node, whoever made it; n is its item
 * count and c3r holds four doubles per item in update order (glome_sb_bih_items): cx cy cz r, every one finite, every r > 0.  Every item
 * must be a Sphere under any number of Tex / Tag / NoShadow / OnlyShadow wrappers, and no Sphere node may be an item twice.  Sets the
 * item spheres' centres and radii (a Sphere node that is also used elsewhere in the builder moves there too) and makes again what `bih`
 * derives from its items' bounds, as glome_sb_bih_refit does: a Sphere's box is c - r / c + r with no pad (Sphere.hs:78-81), so lsplit =
 * (max over the left subtree of (c + r)[axis]) + delta, rsplit = (min over the right subtree of (c - r)[axis]) - delta, and the tree's
 * box is [min(c - r), max(c + r)].  What the builder decided -- nodes, axes, leaf lists, depth -- stays, and the tree stays correct for
 * the reason given above.  Why r > 0: c - r and c + r are then never -0 in round-to-nearest, so the min / max folds give the same bits
 * in any order (the device folds in another one); a sphere of radius 0 is nothing anyway.  All or nothing: anything else is
 * GLOME_E_INVALID with a message (an item that is not a plain Sphere is named, and so are a Sphere held twice and the item whose radius
 * is not positive), and nothing is touched.  The reference has no such call; the result is the Bih the reference would print for the
 * same tree with the new spheres.  Host only; the specification of glome_scene_sphere_bih_update. */
int glome_sb_bih_set_spheres(glome_sb*, int32_t bih_id, const double* c3r, int n);
/* the item ids of a Bih in update order: returns their number and fills out[0 .. min(number, cap)) (out may be NULL: count first) */
int32_t glome_sb_bih_items(glome_sb*, int32_t bih_id, int32_t* out, int32_t cap);
/* New matrices for Instances.  Every id names an Instance node, whoever made it -- glome_sb_transform (of anything but a triangle, an
 * Instance or Void, which it rewrites instead), glome_sb_cylinder / _cone (the node they return), glome_sb_flatten_transform, a `show`
 * text --, no id twice; xfms holds 24 doubles per id (forward rows, inverse rows), every one finite, each matrix passing the reference's
 * check_xfm (Vec.hs:466-477).  Sets the nodes' matrices and, for every Bih of the builder that holds one of these Instances AS AN ITEM
 * (under any number of Tex / Tag / NoShadow / OnlyShadow wrappers), makes again what `bih` derives from its items' bounds, exactly as
 * glome_sb_bih_set_triangles does: every branch's planes and the tree's box, an Instance item's box being the eight transformed corners
 * of its child's bound padded by delta (Solid.hs:477-484).  What the builder decided -- nodes, axes, leaf lists, depth -- stays, and the
 * tree stays correct for the reason given above.  A bih that holds the Instance deeper inside an item (in a group, a CSG node, a Bound,
 * under another Instance), and a bih above a refitted bih, keep the planes and box they were built with: an Instance that leaves them is
 * the caller's error.  glome_sb_bound, glome_sb_show, glome_sb_bih_dump and a later commit see the new matrices and trees.  The reference
 * has no such call; the result is what the reference would print for the same trees with the new matrices.  All or nothing: GLOME_E_INVALID
 * (not an Instance, an id twice, a bad count or pointer, an entry that is not finite) or GLOME_E_SCENE (check_xfm fails; a refitted tree's
 * box would be infinite, as glome_sb_bih refuses it) with a message naming the node, and nothing is touched.  Host only; the
 * specification of glome_scene_instance_update. */
int glome_sb_instance_set_transforms(glome_sb*, const int32_t* ids, const double* xfms, int n);
/* The matrix of Instance `id` as it stands, 24 doubles (forward rows, inverse rows): the placement `cylinder` and `cone` gave the node
 * they return, the product `transform` made, what glome_sb_instance_set_transforms last set.  With it a caller moves such an Instance
 * rigidly: glome_xfm_mult(motion, this).  GLOME_E_INVALID for a node that is not an Instance. */
int glome_sb_instance_transform(glome_sb*, int32_t id, double out[24]);
/* What `bih` derives from its items' bounds, made again for the tree as it stands: every branch's planes and the tree's box from
 * glome_sb_bound of the items' current state -- the last step of glome_sb_bih_set_triangles and glome_sb_instance_set_transforms, on its
 * own.  Topology stays.  With it the host spells the nested case: glome_sb_mesh_set_vertices / _bih_set_triangles /
 * _instance_set_transforms, then glome_sb_bih_refit of every bih above the object, inner trees first (glome_sb_bihs_above gives that
 * order).  That sequence is the specification of glome_scene_bih_refit.  GLOME_E_INVALID for an id that is not a Bih; GLOME_E_SCENE with
 * the constructor's "bih: infinite bounding box" when the joined box reaches +-1e6, and nothing is touched then.  Host only. */
int glome_sb_bih_refit(glome_sb*, int32_t bih_id);
/* The tree built again in place, from its items' bounds as they stand: where glome_sb_bih_set_triangles, _set_spheres and _bih_refit keep
 * what the builder decided, this call decides again.  bih_id names a Bih node, whoever made it, of any items (not only triangles or
 * spheres).  The node becomes the tree glome_sb_bih builds over glome_sb_bih_items(bih_id), in that order: node for node and bit for bit,
 * same box (glome_sb_bih_dump and glome_sb_show tell), as if the caller had handed the same ids to the constructor -- but under the old
 * id, so whatever holds the bih (a group, an Instance, a bih above: which keeps the planes it was built with, glome_sb_bih_refit) holds
 * the new tree.  The update order does not change: a tree read by glome_sb_load_show, whose order is its preorder item list, records
 * that list first, so item k of a later _set_triangles names the same item before and after.  Statuses are glome_sb_bih's: GLOME_E_SCENE
 * with the constructor's messages for an infinite box and for an input on which build_rec does not terminate; GLOME_E_INVALID for an id
 * that is not a Bih.  All or nothing: a refused call leaves the node untouched.  The reference has no such call (`bih` is a pure
 * constructor).  Host only.  glome_sb_bih_set_triangles / _set_triangles_indexed / _set_spheres, then this call, then glome_sb_bih_refit
 * of the bihs above, inner trees first, is the sequence a re-split of a deformed tree is specified by. */
int glome_sb_bih_resplit(glome_sb*, int32_t bih_id);
/* What a commit lays out for a bih of plain triangles or of plain spheres (the trees glome_scene_bih_update / _sphere_bih_update serve):
 * out4 = node slots (branches in treelets of four with their padding, and leaves of 7 or more items), pair records of the packet walk
 * (one per two triangles of a leaf; 0 for spheres), records (one per leaf item), and the tree's depth -- of a scene that is only this
 * tree; in a larger scene the counts are the same and only the segments' bases differ.  Runs the flattener, no GPU.  With it a caller
 * sees what a re-split costs in device memory before asking for it.  GLOME_E_INVALID for a node that is not such a bih. */
int glome_sb_bih_layout(glome_sb*, int32_t bih_id, int64_t out4[4]);
/* The bihs above node_id -- a Mesh, a bih of plain triangles or of plain spheres, an Instance, or a bih that holds a Mesh, a Bih or an Instance as an item --
 * in the scene under `root`: every Bih on any path from root (or from a Warp material's frame / scene) down to the node, in an order in
 * which they can be refitted, a tree after every tree below it.  Returns their number (0: none) and fills out[0 .. min(number, cap)).
 * Runs the flattener's marking, no GPU.  GLOME_E_INVALID, the reason in glome_sb_last_error, when an update of the node would be refused
 * even with glome_scene_nested_updates on (the rule is stated there). */
int32_t glome_sb_bihs_above(glome_sb*, int32_t root, int32_t node_id, int32_t* out, int32_t cap);
int32_t glome_sb_tex(glome_sb*, int32_t id, int32_t material);                                   /* Tex.hs:33-34 */
int32_t glome_sb_tag(glome_sb*, int32_t id);                                                     /* Tex.hs:38-39 (tags feed picking only) */
int32_t glome_sb_noshadow(glome_sb*, int32_t id);                                                /* Tex.hs:43 */
int32_t glome_sb_onlyshadow(glome_sb*, int32_t id);                                              /* Tex.hs:48 */
int32_t glome_sb_bound_object(glome_sb*, int32_t bounding, int32_t bounded);                     /* Bound.hs:27-28 */
int32_t glome_sb_innerbound(glome_sb*, int32_t inner, int32_t outer);                            /* Bound.hs:116 */
int32_t glome_sb_flatten_transform(glome_sb*, int32_t id);  /* `SolidItem (flatten_transform s)`, Solid.hs:192,273 */
int32_t glome_sb_tolist(glome_sb*, int32_t id);             /* `tolist`, Solid.hs:177,230: a list node of the flattened items */
/* the [SolidItem] that `tolist id` yields, as node ids: writes up to cap of them and returns their number -- what a host passes
   on to a constructor that takes a list, e.g. TestScene.hs:109's `bih (tolist (SolidItem (flatten_transform tree)))` */
int32_t glome_sb_list_items(glome_sb*, int32_t id, int32_t* out, int32_t cap);
/* A whole scene in the Neutral File Format of Eric Haines' SPD (GlomeTrace/Data/Glome/Spd.hs:89-254): statements v (camera),
 * l (light, colour optional), b (background), f (fill -> Surface clr (1-T) 0 kd ks shine), s (sphere), c (cone), p / pp
 * (polygon / polygon with normals -> a triangle fan); `#` comments.  Returns the root node -- `bih` of one
 * `tex (bih prims) fill` per fill, in the reference's (reversed) order -- and fills camera (from, at, up, angle), up to
 * max_lights lights (position + rgb each; *n_lights = how many the file holds) and the background colour. */
int32_t glome_sb_load_nff(glome_sb*, const char* text, double cam_from_at_up_angle[10], double* light_pos_rgb, int32_t max_lights, int32_t* n_lights,
                          double bg_rgb[3]);

/* The text GlomeView prints for a scene (`show geom`, SDLK_s, Glome.hs:431) as an interchange format: derived `Show` of
 * the solids' constructors (Sphere.hs:11, Triangle.hs:13-14, Box.hs:10, Cone.hs:21-23, Plane.hs:11, Csg.hs:14-15,
 * Bound.hs:20,95, Tex.hs:27-29, Solid.hs:386, Bih.hs:51-57, Vec.hs:105,407-414,646) with the hand-written instances for
 * SolidItem ("SI ...", Solid.hs:277), Texture ("Texture", Solid.hs:101), Tag (Tex.hs:50) and Mesh (Mesh.hs:44).
 * glome_sb_show writes node `id` in that text (returns its length; at most cap-1 characters + NUL go to buf, buf may
 * be NULL to ask for the length).  glome_sb_load_show reads such a text -- e.g. the dump of a real GHC build of
 * TestScene.hs -- into the builder, Bih and Mesh trees exactly as printed, and returns the root.  Materials are closures
 * on the Haskell side and print as "Texture": the k-th `Tex` of the text (reading order) gets tex_materials[k], the
 * rest default_material (-1: fail); *n_tex = how many the text holds.  Tags and mesh vertex normals are not printed by
 * the reference and do not survive (a mesh with normals is refused); `Difference _ _ False` reads as glome_sb_difference_retexture. */
long glome_sb_show(glome_sb*, int32_t id, char* buf, long cap);
/* the material ids of the `Tex` constructors of that text, in reading order (what the text itself cannot carry): returns
 * their number, writes at most cap of them */
long glome_sb_show_tex_materials(glome_sb*, int32_t id, int32_t* mats, long cap);
int32_t glome_sb_load_show(glome_sb*, const char* text, const int32_t* tex_materials, int32_t n_tex_materials, int32_t default_material, int32_t* n_tex);

/* materials (the defunctionalised `Material`, Shader.hs:43-52; a texture is a material id = t_uniform, Shader.hs:55-56) */
int32_t glome_sb_material_surface(glome_sb*, const double color[3], double alpha, double amb, double kd, double ks, double shine);
int32_t glome_sb_material_reflect(glome_sb*, double refl);
int32_t glome_sb_material_refract(glome_sb*, double refl, double refr, double ior);
int32_t glome_sb_material_layers(glome_sb*, const int32_t* mats, int n);
int32_t glome_sb_material_blend(glome_sb*, int32_t a, int32_t b, double weight);
/* A Blend whose weight is a solid texture function of the hit position (GlomeVec/Data/Glome/Texture.hs) -- the
 * defunctionalised form of the closures t_mottled / t_stripe (TestScene.hs:214-234):
 *   GLOME_WEIGHT_PERLIN            weight = perlin (vscale pos params[0])                      (Texture.hs:109-117)
 *   GLOME_WEIGHT_STRIPE_SQUARE / _TRIANGLE / _SINE   weight = wave (vdot pos params[0..2])     (Texture.hs:11-41) */
#define GLOME_WEIGHT_PERLIN 1
#define GLOME_WEIGHT_STRIPE_SQUARE 2
#define GLOME_WEIGHT_STRIPE_TRIANGLE 3
#define GLOME_WEIGHT_STRIPE_SINE 4
int32_t glome_sb_material_blend_fn(glome_sb*, int32_t a, int32_t b, int32_t weight_fn, const double* params4);
/* Warp frame scene' lights' xfm (Shader.hs:47-50, 157-175): a hit on this material traces `frame` with the hit's own ray (the
 * ray as the primitive saw it -- local coordinates inside a `transform`, Solid.hs:388-403) and the other scene with the
 * warped ray, up to the frame's depth, and shows whichever is nearer.  `scene` is a node, or -1 for the root the scene
 * is committed with (the portal of TestScene.hs:152-181 looks into the scene it stands in: in Haskell laziness ties that
 * knot).  `lights` are that scene's lights.  The closure `Ray -> Rayint -> Ray` crosses the ABI as its one shape in the
 * reference, \ray hit -> xfm_ray M (Ray (pos hit) (vnorm (dir ray))) (TestScene.hs:166-172): xfm = M, 24 doubles like
 * every transform here.  Scenes with a Warp material render on the generic tier. */
struct glome_light;
int32_t glome_sb_material_warp(glome_sb*, int32_t frame, int32_t scene, const struct glome_light* lights, int nlights, const double xfm[24]);
/* host-side inspection (no GPU needed) */
int glome_sb_primcount(glome_sb*, int32_t id, long out3[3]);  /* primcount, Solid.hs:197,251 */
int glome_sb_bound(glome_sb*, int32_t id, double out6[6]);    /* bound, Solid.hs:171 */
/* Preorder dump of the BIH built for node `id` (axis = -1 marks a leaf; nleaf = its item count;
 * leaf_prims = builder ids of leaf items in order).  Returns the node count, <0 on error. */
long glome_sb_bih_dump(glome_sb*, int32_t id, long cap, double* lsplit, double* rsplit, int* axis, int* nleaf,
                       int32_t* leaf_prims, long cap_prims);

/* `bih` (Bih.hs:309-324) built on the GPU of `ctx`: the same node as glome_sb_bih over the same ids -- the tree of the
 * reference's build_rec (Bih.hs:211-285), node for node and bit for bit -- made level by level by four kernels per tree
 * level instead of by recursion on the host (100k triangles: see DESIGN.md).  *gpu_ms (may be NULL) = device time of the
 * build.  Needs the HIP half of the library (a context); the host builder stays the default and the checker.
 *   Statuses are glome_sb_bih's (GLOME_E_SCENE with its message for an infinite box and for an input on which build_rec does not
 * terminate, GLOME_E_INVALID for a bad id) and one of its own: a level of the tree costs six launches and a synchronisation, so a
 * tree deeper than 2048 levels is refused with GLOME_E_LIMIT and a message naming the limit (the host builder has none).  The node
 * and accumulator pools are sized from the item count by a bound that holds for every input (bih_build_device.hpp), so nothing
 * else is refused.  A refused call adds no node; the context and the builder work on the next call. */
int32_t glome_sb_bih_dev(glome_ctx*, glome_sb*, const int32_t* ids, int32_t n, float* gpu_ms);

/* `mesh` (Mesh.hs:50-134) with its two-box BVH (build_tree, Mesh.hs:69-113) built on the GPU of `ctx`: arguments and
 * result as glome_sb_mesh, the tree the host builder makes (boxes, leaf order).  Statuses are glome_sb_mesh's (GLOME_E_SCENE
 * with its message for a mesh on which build_tree does not terminate: a vertex at infinity) and the same limit of 2048 levels,
 * refused the same way (GLOME_E_LIMIT, no node added); fewer than three triangles are built on the host. */
int32_t glome_sb_mesh_dev(glome_ctx*, glome_sb*, const double* verts, int nv, const double* norms, int nn, const int32_t* tris, int nt, const int32_t* mats, int nm,
                          float* gpu_ms);

/* ---- commit: validate + flatten to packed SoA pools + upload to HBM ---- */
glome_scene* glome_scene_commit(glome_ctx*, glome_sb*, int32_t root);
void glome_scene_release(glome_scene*);
typedef struct glome_scene_info {
  int32_t tier;            /* 0 = flat fast path (LDS-stack kernels), 1 = generic interpreter */
  int32_t nesting_depth;   /* composite nesting depth of the generic graph */
  int64_t n_records, n_bih_nodes, n_mesh_nodes, n_triangles, n_spheres, n_other_prims, n_xfms, n_materials;
  int32_t max_bih_depth, max_mesh_depth;
  int64_t device_bytes;
} glome_scene_info;
int glome_scene_get_info(const glome_scene*, glome_scene_info* out);

/* ---- animate a committed Mesh: new vertices, its BVH refitted on the GPU ----
 * After an update the committed scene is, bit for bit, the scene glome_scene_commit would have made had glome_sb_mesh_set_vertices
 * been called with the same arrays first: the mesh's triangle records and vertex normals, every box of its BVH, its own box.  The tree's
 * topology stays (see glome_sb_mesh_set_vertices); nothing else of the scene is read or written, and one update moves every Instance
 * of the mesh.  (One deviation from "bit for bit": a component whose fp32 value would be subnormal is stored as zero -- which is how
 * every kernel reads it anyway.)  The builder is not touched: a host that also wants the new mesh there calls both.
 *   mesh_id  the builder id of a Mesh that is part of this scene; nv, nn its own vertex / normal counts; norms NULL when nn == 0.
 *   Refused with GLOME_E_INVALID before anything is launched, the scene untouched: an id that is not a mesh of this scene, a count
 *   mismatch, a missing array, and a mesh with a `bih` above it on any path from the committed root (or from a Warp material's frame
 *   / scene) -- that tree's planes and root box were built from the mesh's bound; the message names the bih.  Every other composite
 *   keeps nothing of its children's bounds, and the bounding solid of a Bound / InnerBound is the caller's own object, as in the
 *   reference: it must still contain the moved mesh.
 * glome_scene_mesh_update takes host arrays, checks that every coordinate is finite, waits for every launch of the context (all
 * slots), stages the arrays, updates and returns when the update is complete; *gpu_ms (may be NULL) = HIP-event time of its kernels.
 * glome_scene_mesh_update_dev takes DEVICE pointers (fp64, 3 per vertex) and is asynchronous on the context's current stream and
 * slot, like glome_rayint_batch_dev: launches enqueued after it on that stream see the new mesh, and the arrays must stay valid until
 * it has run.  Launches still in flight on OTHER slots / streams read the same pools: ordering an update against them is the
 * caller's responsibility (the pools are not double-buffered).  It takes part in glome_ctx_timing_begin / _end (one event pair per
 * update).  A coordinate that is not finite is found on the device: the next glome_ctx_synchronize returns GLOME_E_INVALID, and the
 * mesh is unspecified -- though never out of bounds -- until a valid update (as rgbad is after a failed trace).
 * The first update of a mesh allocates its workspace (32 bytes per triangle), kept until glome_scene_release. */
int glome_scene_mesh_update(glome_scene*, int32_t mesh_id, const double* verts, int nv, const double* norms, int nn, float* gpu_ms);
int glome_scene_mesh_update_dev(glome_scene*, int32_t mesh_id, const double* verts_dev, int nv, const double* norms_dev, int nn);

/* ---- animate a committed triangle bih: new triangles, its planes refitted on the GPU ----
 * A triangle bih is a Bih whose items are all plain Triangles (under Tex / Tag wrappers, at most two Tex levels): the flagship's
 * `tex (bih (map triangle ...))`.  After an update the committed scene is, bit for bit, the scene glome_scene_commit would have made had
 * glome_sb_bih_set_triangles been called with the same array first: the triangle records, the pair records of the packet walk, every
 * branch's two planes in both node pools, the tree's box.  The tree's topology stays (see glome_sb_bih_set_triangles); nothing else of
 * the scene is read or written, and one update moves every Instance of the bih.  (One deviation from "bit for bit", as for the mesh: a
 * component whose fp32 value would be subnormal is stored as zero -- which is how every kernel reads it anyway.)  The builder is not
 * touched: a host that also wants the new tree there calls both.
 *   bih_id  the builder id of a triangle bih that is part of this scene; n its item count; pts9 nine doubles per item in update order.
 *   Refused with GLOME_E_INVALID before anything is launched, the scene untouched: an id that is not a triangle bih of this scene, a
 *   count mismatch, a missing array, a bih with another `bih` above it on any path from the committed root (or from a Warp material's
 *   frame / scene) -- that tree's planes were built from this one's bound; the message names it --, a bih one of whose triangles the
 *   scene also reaches outside it (in a group beside it, say: that copy could not be moved; the message names the triangle), and a bih
 *   that holds a triangle twice.  The bounding solid of a Bound / InnerBound above is the caller's own object, as in the reference: it
 *   must still contain the moved triangles.
 * glome_scene_bih_update takes a host array, checks that every coordinate is finite, waits for every launch of the context (all slots),
 * stages the array, updates and returns when the update is complete; *gpu_ms (may be NULL) = HIP-event time of its kernels.
 * glome_scene_bih_update_dev takes a DEVICE pointer (fp64) and is asynchronous on the context's current stream and slot, like
 * glome_scene_mesh_update_dev: launches enqueued after it on that stream see the new triangles, and the array must stay valid until it
 * has run.  Launches still in flight on OTHER slots / streams read the same pools: ordering an update against them is the caller's
 * responsibility (the pools are not double-buffered).  It takes part in glome_ctx_timing_begin / _end (one event pair per update).  A
 * coordinate that is not finite is found on the device: the next glome_ctx_synchronize returns GLOME_E_INVALID (the error word is the mesh
 * update's: the message names both calls, a context cannot tell which one raised it), and the tree is unspecified -- though never out
 * of bounds -- until a valid update.
 * The first update of a bih allocates its workspace (32 bytes per triangle and per node), kept until glome_scene_release. */
int glome_scene_bih_update(glome_scene*, int32_t bih_id, const double* pts9, int n, float* gpu_ms);
int glome_scene_bih_update_dev(glome_scene*, int32_t bih_id, const double* pts9_dev, int n);

/* ---- animate a committed sphere bih: new centres and radii, its planes refitted on the GPU ----
 * A sphere bih is a Bih whose items are all plain Spheres (under Tex / Tag wrappers, at most two Tex levels): the benchmark scenes'
 * `bih [tex (sphere ..) mat ...]`, a lattice, particles, a point cloud.  After an update the committed scene is, bit for bit, the scene
 * glome_scene_commit would have made had glome_sb_bih_set_spheres been called with the same array first: the sphere records, every
 * branch's two planes, the tree's box.  The tree's topology stays (see glome_sb_bih_set_triangles); nothing else of the scene is read or
 * written, and one update moves every Instance of the bih.  (The other updates' deviation holds: a component whose fp32 value would be
 * subnormal is stored as zero.)  The builder is not touched: a host that also wants the new tree there calls both.
 *   bih_id  the builder id of a sphere bih that is part of this scene; n its item count; c3r four doubles per item in update order
 *           (glome_sb_bih_items): cx cy cz r.
 *   Refused with GLOME_E_INVALID before anything is launched, the scene untouched: an id that is not a sphere bih of this scene, a count
 *   mismatch, a missing array, a bih with another `bih` above it on any path from the committed root (or from a Warp material's frame /
 *   scene) -- the message names it; glome_scene_nested_updates lifts this one --, a bih one of whose spheres the scene also reaches
 *   outside it (in a group beside it, say: that copy has a record of its own, which could not be moved; the message names the sphere),
 *   and a bih that holds a sphere twice.  The bounding solid of a Bound / InnerBound above is the caller's own object: it must still
 *   contain the moved spheres.  glome_scene_bih_update keeps refusing a sphere bih, and this call a triangle bih.
 * glome_scene_sphere_bih_update takes a host array, checks that every value is finite and every radius > 0, waits for every launch of
 * the context (all slots), stages the array, updates and returns when the update is complete; *gpu_ms (may be NULL) = HIP-event time of
 * its kernels.
 * glome_scene_sphere_bih_update_dev takes a DEVICE pointer (fp64) and is asynchronous on the context's current stream and slot, like
 * glome_scene_bih_update_dev: launches enqueued after it on that stream see the new spheres, and the array must stay valid until it has
 * run.  Launches still in flight on OTHER slots / streams read the same pools: ordering an update against them is the caller's
 * responsibility.  It takes part in glome_ctx_timing_begin / _end (one event pair per update).  A value that is not finite or a radius
 * that is not positive is found on the device: the next glome_ctx_synchronize returns GLOME_E_INVALID (the error word is the other
 * updates': the message names this call too), and the tree is unspecified -- though never out of bounds -- until a valid update.
 *   With glome_scene_nested_updates on (below), an accepted update of a sphere bih under bihs also leaves its fp64 bound, min(c - r) /
 * max(c + r) from +-1e6, in the scene's bounds table and marks the trees above stale; glome_scene_bih_refit of those, inner trees first,
 * then gives the scene a commit after glome_sb_bih_set_spheres + glome_sb_bih_refit would give, bit for bit.
 * The first update of a bih allocates its workspace (32 bytes per sphere and per node), kept until glome_scene_release. */
int glome_scene_sphere_bih_update(glome_scene*, int32_t bih_id, const double* c3r, int n, float* gpu_ms);
int glome_scene_sphere_bih_update_dev(glome_scene*, int32_t bih_id, const double* c3r_dev, int n);

/* ---- the three updates above from the arrays a simulation holds: fp32, and a vertex array with an index table ----
 * The calls above take one layout, contiguous fp64 expanded per item.  A producer on the GPU -- a cloth, terrain or skinning step, a
 * particle step -- holds fp32 vertices [nv, 3] with an int32 face table [n, 3], or fp32 positions [n, 3] and radii [n]; these calls read
 * those arrays as they are, so nothing is gathered or widened per frame.  Each leaves the committed scene bit for bit as its fp64 call
 * leaves it when given the WIDENED AND GATHERED array: pts9[9 k + 3 c ..] = (double)verts[3 * idx3[3 k + c] ..], c3r[4 k ..] =
 * ((double)centre, (double)radius).  fp32 -> fp64 is exact, and the kernels are the fp64 calls' own, instantiated for another way to
 * load a point: there is no tolerance.  Everything else of the fp64 call's contract holds word for word -- the refusals before anything
 * is launched, the host form's wait for all slots and its gpu_ms, the _dev form asynchronous on the current stream and slot with one
 * event pair under glome_ctx_timing_begin, the workspace of the first update (the same one: the forms of one object share it), the
 * subnormal-stored-as-zero deviation, and with glome_scene_nested_updates on the same fp64 bound in the bounds table and the same trees
 * marked stale.  An fp32 INPUT that is subnormal may be read as zero.  The host forms stage the caller's arrays as they are.
 *   glome_scene_bih_update_f32 / glome_scene_mesh_update_f32 / glome_scene_sphere_bih_update_f32: the fp64 call with fp32 arrays; the
 *     sphere form takes two streams, centres3 [n, 3] and radii [n].
 *   glome_scene_bih_update_indexed: verts holds nv vertices of three values of `dtype` (GLOME_F64: double, GLOME_F32: float), idx3 three
 *     vertex indices per item, items in update order (glome_sb_bih_items); the specification is glome_sb_bih_set_triangles_indexed.
 *     Only REFERENCED vertices count: the tree's box and its nested fp64 bound are folded over the gathered item vertices, never over
 *     the vertex array, and a vertex no item names may be anything, NaN included (a Mesh keeps its own rule: its box is over ALL
 *     vertices, Mesh.hs:55).  Refused up front as well: a dtype that is neither, a missing array, nv == 0 with n > 0.  The host form
 *     checks every index -- one outside [0, nv) is GLOME_E_INVALID, the message naming the item, the scene untouched -- and finiteness
 *     over the referenced vertices only.  The _dev form (both arrays DEVICE pointers) finds a bad index on the device: the lane raises
 *     the updates' error word and reads vertex 0 instead -- the index is clamped before the load, so nothing is read out of bounds --,
 *     the next glome_ctx_synchronize returns GLOME_E_INVALID, and the tree is unspecified, never out of bounds, until a valid update. */
enum { GLOME_F64 = 0, GLOME_F32 = 1 };
int glome_scene_bih_update_indexed(glome_scene*, int32_t bih_id, const void* verts, int32_t dtype, int nv, const int32_t* idx3, int n, float* gpu_ms);
int glome_scene_bih_update_indexed_dev(glome_scene*, int32_t bih_id, const void* verts_dev, int32_t dtype, int nv, const int32_t* idx3_dev, int n);
int glome_scene_bih_update_f32(glome_scene*, int32_t bih_id, const float* pts9, int n, float* gpu_ms);
int glome_scene_bih_update_f32_dev(glome_scene*, int32_t bih_id, const float* pts9_dev, int n);
int glome_scene_mesh_update_f32(glome_scene*, int32_t mesh_id, const float* verts, int nv, const float* norms, int nn, float* gpu_ms);
int glome_scene_mesh_update_f32_dev(glome_scene*, int32_t mesh_id, const float* verts_dev, int nv, const float* norms_dev, int nn);
int glome_scene_sphere_bih_update_f32(glome_scene*, int32_t bih_id, const float* centres3, const float* radii, int n, float* gpu_ms);
int glome_scene_sphere_bih_update_f32_dev(glome_scene*, int32_t bih_id, const float* centres3_dev, const float* radii_dev, int n);

/* ---- animate committed Instances: new matrices, the bih that holds them refitted on the GPU ----
 * Every `transform` that is not pushed down into a primitive is an Instance: a rigid object, and every `cylinder` and `cone`.  After an
 * update the committed scene is, bit for bit, the scene glome_scene_commit would have made had glome_sb_instance_set_transforms been
 * called with the same ids and matrices first: the six float4 of every xfm slot of every named Instance and, for a bih that holds a
 * named Instance as an item, both planes of every branch and the header's box.  The tree's topology stays; one update moves everything
 * below the Instance (a Mesh or a triangle bih under it keeps its own update call).  (The deviation of the two other updates holds: a
 * component whose fp32 value would be subnormal is stored as zero.)  The builder is not touched: a host that also wants the new
 * matrices there calls both.
 *   ids   n builder ids of Instances that are part of this scene, a HOST array in both forms, no id twice; xfms 24 doubles per id
 *         (forward rows, inverse rows: what glome_xfm_* writes).
 *   Accepted: an Instance anywhere below lists, Instances, CSG, Bound / InnerBound and wrappers with no bih above it -- a write of its
 *   slots and nothing else --, and an Instance that is an item of exactly one bih (under Tex / Tag / shadow wrappers), that bih below
 *   anything but another bih.  The bounding solid of a Bound / InnerBound above is the caller's own object, as in the reference.
 *   Refused with GLOME_E_INVALID before anything is launched, the scene untouched, the message naming the node: an id that is not an
 *   Instance of this scene, an id named twice, a bad count or a null array, in the host form a matrix that is not finite or fails the
 *   reference's check_xfm (forward * inverse = identity), an Instance that lies INSIDE an item of a bih rather than being the item (the
 *   item's box depends on it through a list, CSG, Bound or Instance, which the update does not recompute), an Instance with two or more
 *   bihs above it on any path from the committed root or from a Warp material's frame / scene (the items of the oak inside GlomeView's
 *   default scene, whose root is itself a bih), and one that is an item of a bih more than once.  The host form also refuses, with
 *   GLOME_E_SCENE and the constructor's "bih: infinite bounding box", an item whose new box reaches the reference's infinity (1e6) in a
 *   component; it looks at the named items one by one, where glome_sb_instance_set_transforms looks at the joined box.
 * glome_scene_instance_update takes a host array of matrices, checks it, waits for every launch of the context (all slots), stages it,
 * updates and returns when the update is complete; *gpu_ms (may be NULL) = HIP-event time of its kernels.
 * glome_scene_instance_update_dev takes the matrices as a DEVICE pointer (fp64, 24 per id) and is asynchronous on the context's current
 * stream and slot, like the two other updates: launches enqueued after it on that stream see the new matrices, and the array must stay
 * valid until it has run.  Launches still in flight on OTHER slots / streams read the same pools: ordering an update against them is
 * the caller's responsibility.  It takes part in glome_ctx_timing_begin / _end (one event pair per call).  A matrix entry that is not
 * finite, and an item box that reaches infinity, are found on the device: the next glome_ctx_synchronize returns GLOME_E_INVALID (the
 * error word is the other updates': the message names all three calls), and the named Instances and the bih that holds them are
 * unspecified -- though never out of bounds -- until a valid update.  A matrix that merely fails check_xfm is the caller's error there.
 * The first update that touches a bih allocates its workspace (32 bytes per record the tree spans, per node and per item), kept until
 * glome_scene_release, and gives it the commit-time boxes of all the tree's items; later updates rewrite only the named items' rows, so
 * updating 3 of 2,047 items costs 3 boxes and the plane pass.  That first update is NOT asynchronous, in either form: it allocates and
 * copies the workspace with blocking calls before it enqueues its kernels (once per bih; a host that cannot block mid-stream makes one
 * update with the committed matrices right after the commit).  A call that names more Instances than any before it also waits for the
 * stream once, to grow its table. */
int glome_scene_instance_update(glome_scene*, const int32_t* ids, const double* xfms, int n, float* gpu_ms);
int glome_scene_instance_update_dev(glome_scene*, const int32_t* ids, const double* xfms_dev, int n);

/* ---- the same update from what a rigid-body or skinning step holds: poses, 3x4 / 4x4 forward matrices, fp32, strided ----
 * glome_scene_instance_update takes 24 contiguous doubles per Instance, the inverse included.  These calls read a SOURCE instead: item k
 * of the source is the matrix of ids[k], and the library makes the 24 doubles on the device.  The contract is the other updates': the
 * call leaves the committed scene, bit for bit, as glome_scene_instance_update leaves it when given the table the host functions above
 * (glome_xfm_from_pose, glome_xfm_from_forward, glome_xfm_mult) yield for the widened items.  fp32 -> fp64 is exact and the device
 * evaluates those functions' own expressions with explicit round-to-nearest operations: there is no tolerance.  (An fp32 input that is
 * subnormal may be read as zero, as in the other fp32 forms.)
 *   data    item k starts k * stride ELEMENTS of dtype after data; GLOME_F64 or GLOME_F32.
 *   stride  elements between the starts of two items: 0 = dense (the form's width), otherwise at least the width.  Only the values
 *           [k * stride, k * stride + width) are ever read, k < n: what lies between two items, and after the last one, may be anything,
 *           NaN included, and need not exist after the last item.  All index arithmetic is 64-bit.
 *   form    GLOME_XFM_PAIR: 24 values, forward rows then inverse rows -- the existing layout, now also fp32 and strided.
 *           GLOME_XFM_FORWARD: 12 values, a row-major 3x4 forward matrix (glome_xfm_from_forward); stride 16 reads a row-major 4x4
 *             [n, 4, 4] array, whose fourth row is never read.
 *           GLOME_XFM_POSE: 8 values tx ty tz qx qy qz qw s (glome_xfm_from_pose): the quaternion's scalar last, a uniform scale.
 *   base    NULL, or 24 doubles per id, contiguous (fp64 whatever dtype is): the item is applied AFTER base[k], the result being
 *           glome_xfm_mult(item, base[k]) -- NOT glome_xfm_compose, which starts from an identity and can change the sign of a zero.  With
 *           base[k] = glome_sb_instance_transform of a `cylinder` or `cone`, a pose moves that primitive rigidly from where it was built.
 * ids is a HOST array in both forms, and the struct is host memory read during the call.  Everything glome_scene_instance_update
 * refuses stays refused, with its messages, before anything is launched (what is updatable, an id twice, the nested rule); also
 * GLOME_E_INVALID before anything is launched: a null source or null data with n > 0, an unknown form or dtype, a negative stride, a
 * stride that is neither 0 nor at least the form's width.
 *   glome_scene_instance_update_from: data and base are HOST arrays.  It converts every item on the host first and refuses, the scene
 * untouched and the message naming the node: a value of an item that is not finite, a quaternion of length 0 or s <= 0
 * (GLOME_E_INVALID); a forward matrix whose det is 0 or whose inverse is not finite (GLOME_E_SCENE); then, on the converted matrix,
 * exactly what glome_scene_instance_update checks (an entry that is not finite, check_xfm, an item box that reaches 1e6).  Then it
 * waits for every launch of the context, stages the caller's array AS IT IS -- its own dtype and stride, (n - 1) * stride + width
 * elements -- and base, runs the _dev form and returns when the update is complete; *gpu_ms (may be NULL) = HIP-event time.
 *   glome_scene_instance_update_from_dev: data and base are DEVICE pointers; asynchronous on the current stream and slot like
 * glome_scene_instance_update_dev, whose first-update, workspace and nested-updates behaviour it inherits (with
 * glome_scene_nested_updates on, the trees' tables keep the CONVERTED 24 doubles and the trees above are marked stale).  It takes part
 * in glome_ctx_timing_begin / _end with ONE event pair per call, the conversion inside it.  The same defects are found on the device:
 * a lane whose 24 results are not all finite (a value that is not finite, a singular forward matrix), or whose quaternion has length 0
 * or s <= 0, raises the updates' error word; the next glome_ctx_synchronize returns GLOME_E_INVALID (its message names this call too),
 * and the named Instances and their bih are unspecified, never out of bounds, until a valid update.  A matrix that merely fails
 * check_xfm is the caller's error there, as it is in glome_scene_instance_update_dev.
 *   The conversion writes the 24 doubles into ONE table per scene, which the update's kernels then read as they read a caller's array;
 * a call that names more Instances than any _from call before it waits for the stream once, to grow the table (192 bytes per
 * Instance, kept until glome_scene_release).  So the ordering rule of the Instance updates holds here too and covers the table: two
 * _dev Instance updates of one scene, of either entry, must not run at the same time on different streams / slots; order them on one
 * stream or with events.  PAIR + GLOME_F64 + dense + no base is glome_scene_instance_update_dev itself, with no table. */
enum { GLOME_XFM_PAIR = 0, GLOME_XFM_FORWARD = 1, GLOME_XFM_POSE = 2 };
typedef struct glome_xfm_source {
  const void* data;   /* item k starts k * stride ELEMENTS of dtype after data */
  const double* base; /* NULL, or 24 doubles per id, contiguous: the item is applied AFTER base[k] */
  int32_t dtype;      /* GLOME_F64 / GLOME_F32 */
  int32_t form;       /* GLOME_XFM_* */
  int64_t stride;     /* elements between items; 0 = dense: 24 / 12 / 8 */
} glome_xfm_source;
size_t glome_xfm_source_size(void);
int glome_scene_instance_update_from(glome_scene*, const int32_t* ids, const glome_xfm_source*, int n, float* gpu_ms);
int glome_scene_instance_update_from_dev(glome_scene*, const int32_t* ids, const glome_xfm_source*, int n);

/* ---- update objects under a bih: the chain of bihs above refitted on the GPU, one call per tree ----
 * The three updates above refuse an object as soon as a bih lies above it (a second one for an Instance): that tree's planes and box
 * were built from the object's bound.  glome_scene_nested_updates(scene, 1) lifts that: the updates then accept an object X -- a Mesh, a
 * bih of plain triangles or plain spheres, an Instance that is an item of a bih -- when on EVERY path from the committed root (or a Warp material's frame /
 * scene) down to X every bih B on the path holds, on that path, an item that is LIVE over the next thing down (X, or the next bih): the
 * item, Tex / Tag / NoShadow / OnlyShadow wrappers peeled off, is that thing itself (a direct item) or an Instance whose child, peeled
 * again, is that thing (an instanced item).  For an Instance X its own bih holds X as the item.  Still refused, the message naming the
 * node in the way: a list, a CSG node, a Bound / InnerBound or a second Instance between two trees, an Instance deeper inside an item, a
 * triangle the scene also reaches outside its bih, an Instance that is an item more than once.  One object under several items or
 * several bihs is fine (a mesh instanced five times, a bih shared by two outer trees).  With the switch off -- the default -- every call
 * accepts and refuses exactly what it did, with the same messages.
 *   An accepted update of an object with bihs above it also leaves the object's fp64 bound on the device (Mesh: min(p - delta) / max(p +
 * delta) over all vertices; triangle bih: the same from +-1e6 over all item vertices; a refitted bih: the join of its items' fp64 boxes
 * from +-1e6) and marks every bih above as STALE (glome_scene_stale_bihs; an Instance update refits the bih that holds the Instance itself,
 * so it marks the trees above that one).  The folds are fp64 min / max of finite values, exact in any order; a component that folds to
 * zero is stored as +0 whenever an operand was +0 (p - delta and p + delta never give -0), and a refit stores what it is given.
 * glome_scene_instance_update also stores the named Instances' 24 doubles in a device table the refits read.
 *   glome_scene_bih_refit(scene, B) makes again, for ALL live items of B (not only the changed ones: the simpler choice, an item is 200
 * bytes), the item's plane-form and box-form rows and its fp64 box from the object's bound -- an instanced item's through its matrix,
 * eight corners, glome_scene_instance_update's arithmetic --, then every branch's planes, the header's box and B's own fp64 bound, and
 * clears B's stale mark.  Call it once per tree, inner trees first: the order of glome_scene_bihs_above.  After the last one the scene is,
 * bit for bit, the scene glome_scene_commit would have made after the builder calls glome_sb_bih_refit documents.
 *   Refused with GLOME_E_INVALID before anything is launched: B is not a bih of this scene that holds a Mesh, Bih or Instance item, the
 * switch is off, or a tree below B is stale ("refit bih N first").  Turning the switch off while a tree is stale is refused too.  An item
 * box or joined box that reaches +-1e6 is found on the device and reported by the next glome_ctx_synchronize, through the updates' error
 * word (the message names this call too); the tree is then unspecified, never out of bounds, until a valid update and refit.
 *   glome_scene_bih_refit waits for every launch of the context (all slots) and returns when the refit is complete, *gpu_ms (may be NULL)
 * the HIP-event time of its kernels; glome_scene_bih_refit_dev is asynchronous on the current stream and slot, ordered after the updates
 * enqueued before it, and takes part in glome_ctx_timing_begin / _end (one event pair per call).  Turning the switch on allocates and
 * fills the bounds table, and the first refit or Instance update of a tree allocates and fills its workspace (32 bytes per record the
 * tree spans, per node and per item, and 240 bytes of fp64 per item), both with blocking calls, kept until glome_scene_release.
 *   The _dev forms of two updates of objects under bihs, or of two refits, must not run at the same time on different streams / slots of one
 * scene: a bound's partial boxes pass through one buffer per scene, as an Instance update's rows do.  Order them on one stream, or with
 * events; the host forms wait for every slot and need nothing.
 *   Rendering while a bih is stale is allowed: the picture is unspecified but never out of bounds -- an update writes planes, boxes and
 * records, never a reference.
 * glome_scene_bihs_above: glome_sb_bihs_above for the committed root.  glome_scene_stale_bihs: the stale trees, in an order in which they
 * can be refitted; both return the number and fill out[0 .. min(number, cap)). */
int glome_scene_nested_updates(glome_scene*, int on);              /* default 0 */
int glome_scene_bih_refit(glome_scene*, int32_t bih_id, float* gpu_ms);
int glome_scene_bih_refit_dev(glome_scene*, int32_t bih_id);       /* asynchronous on the current stream / slot */
int32_t glome_scene_bihs_above(const glome_scene*, int32_t node_id, int32_t* out, int32_t cap);
int32_t glome_scene_stale_bihs(const glome_scene*, int32_t* out, int32_t cap);

/* ---- a committed triangle or sphere bih re-split in place ----
 * Where the updates above keep what the builder decided, a rebuild decides again: the committed tree is built again on the GPU from the
 * new items, in place, and everything else of the scene stays.  The arguments are the matching update's -- glome_scene_bih_update,
 * _bih_update_indexed, _sphere_bih_update: the same items in the same update order, the same checks of count and pointers up front, the
 * same rule for a tree under other trees (refused, or, with glome_scene_nested_updates on, accepted: the object's fp64 bound is left in
 * the bounds table and the bihs above are marked stale, glome_scene_bih_refit of them follows), every refusal of the update in the
 * update's words ("bih rebuild: ...").
 *   Contract.  After the call the scene answers every render, sampler, trace and per-ray seam call, bit for bit, work counters bih_nodes
 * and prim_tests included, as a glome_scene_commit of the same builder after glome_sb_bih_set_triangles (_indexed, _set_spheres) with the
 * same array, glome_sb_bih_resplit, and glome_sb_bih_refit of the bihs above, inner trees first.  The tree's own segments of the pools --
 * node slots in both node forms, pair records, triangles or spheres, records -- hold the words that commit uploads, child references
 * shifted by the segment's base.  The updates' fp32 subnormal-as-zero deviation holds.
 *   Sequence, on the current stream and slot: a kernel makes the items' fp64 boxes straight from the caller's arrays (min(p) - delta /
 * max(p) + delta, c - r / c + r: glome_sb_bound's own operations) and validates them; the device builder's level loop (glome_sb_bih_dev)
 * runs over those boxes; the built topology and the object order come back; the host lays the tree out with the commit's own layout
 * function and uploads node words, records in the new leaf order, the pair records' count and index words, the update's tables and the
 * header's words; the update's kernels fill in every value.  NOT asynchronous, in either form: a level costs a synchronisation.  The
 * call waits for every launch of the context (all slots) first and returns when the scene is complete; *gpu_ms (may be NULL) is the
 * HIP-event time from the first kernel to the last.  The _dev forms take DEVICE arrays and differ in nothing else.
 *   All or nothing.  Everything up to the readback writes scratch alone, and every refusal is found by then: GLOME_E_INVALID for a value
 * that is not finite, a radius that is not positive, a vertex index outside [0, nv) (the host forms look before anything is launched and
 * name the item; the _dev forms find it in the box kernel, through a flag of the call's own -- not the context's sticky error word --
 * and report it at once; a bad index is clamped before the load); GLOME_E_SCENE with the constructor's messages for an infinite box and
 * for an input on which build_rec does not terminate; GLOME_E_LIMIT for a tree deeper than the device builder's 2,048 levels.  The scene
 * is then as it was.
 *   Capacity.  A tree's node segment and its pair segment hold what commit gave them (glome_scene_bih_layout: out6 = node slots, pair
 * records, records, depth of the tree as it stands, then the capacities of the two segments).  A rebuilt tree that fits is laid out from
 * the segment's unchanged base; one that does not gets new segments at the line-aligned end of the pools, which are reallocated with a
 * quarter of headroom when they are full; the old segment is abandoned (not reclaimed).  GLOME_E_LIMIT, scene untouched, when the new
 * segments would pass what a child reference or the packet walk's byte offsets can address, when a tree would lose the packet walk's
 * node form (or never had it), and -- in a scene of the flat tier -- when the tree would be deeper than the flat tier's stack (32), where
 * a commit would have taken the generic tier.
 *   Everything commit derives from the trees' depths is derived again: the header's depth word, glome_scene_info's max_bih_depth and
 * n_bih_nodes, the stack entries per lane in LDS and beyond, the generic tier's packet stack, the update's workspace.  A rebuilt tree may
 * be deeper than anything the commit saw.  The walk-entry table and the cull pass name a tree by its header, which does not move. */
int glome_scene_bih_rebuild(glome_scene*, int32_t bih_id, const double* pts9, int n, float* gpu_ms);
int glome_scene_bih_rebuild_dev(glome_scene*, int32_t bih_id, const double* pts9_dev, int n, float* gpu_ms);
int glome_scene_bih_rebuild_indexed(glome_scene*, int32_t bih_id, const void* verts, int32_t dtype, int nv, const int32_t* idx3, int n, float* gpu_ms);
int glome_scene_bih_rebuild_indexed_dev(glome_scene*, int32_t bih_id, const void* verts_dev, int32_t dtype, int nv, const int32_t* idx3_dev, int n, float* gpu_ms);
int glome_scene_sphere_bih_rebuild(glome_scene*, int32_t bih_id, const double* c3r, int n, float* gpu_ms);
int glome_scene_sphere_bih_rebuild_dev(glome_scene*, int32_t bih_id, const double* c3r_dev, int n, float* gpu_ms);
int glome_scene_bih_layout(const glome_scene*, int32_t bih_id, int64_t out6[6]);
/* The last rebuild of the scene by stage, host wall-clock milliseconds: the boxes (kernel, and the wait for the flag and the root's box),
 * the level loop with the readback, the tables on the host, their upload, the update's kernels with the final wait.  Zeros before the
 * first rebuild.  For measurement (tools/probe/bih_rebuild_rate.py). */
int glome_scene_bih_rebuild_stages(const glome_scene*, double out5[5]);

/* ---- per-ray seams (Solid.hs:146-166), host buffers ---- */
/* closest hit: t < 0 marks a miss (RayMiss), and then prim is -1, tex8 all -1 and the normal UNSPECIFIED (whatever the traversal
 * left: it may differ between two commits of one builder); prim = builder id of the primitive hit; tex8 = the hit's
 * texture stack (the ids of glome_sb_material), innermost first, -1 padded: GLOME_TEX_WORDS (8) int32 PER RAY -- the buffer is
 * n * GLOME_TEX_WORDS words (until round 3 it was 4 per ray: a caller built against that header must be rebuilt; glome_tex_words()
 * returns what the loaded library writes, for a binding that wants to check at run time).  Any output pointer may be NULL. */
#define GLOME_TEX_WORDS 8
int glome_tex_words(void);
int glome_rayint_batch(glome_scene*, size_t n, const float* ox, const float* oy, const float* oz, const float* dx,
                       const float* dy, const float* dz, const float* tmax, float* t, int32_t* prim, float* nx,
                       float* ny, float* nz, int32_t* tex8);
int glome_shadow_batch(glome_scene*, size_t n, const float* ox, const float* oy, const float* oz, const float* dx,
                       const float* dy, const float* dz, const float* tmax, uint8_t* occluded);
int glome_inside_batch(glome_scene*, size_t n, const float* px, const float* py, const float* pz, uint8_t* inside);
/* the same on device pointers, asynchronous on the ctx stream */
int glome_rayint_batch_dev(glome_scene*, size_t n, const float* ox, const float* oy, const float* oz, const float* dx,
                           const float* dy, const float* dz, const float* tmax, float* t, int32_t* prim, float* nx,
                           float* ny, float* nz, int32_t* tex8);
int glome_shadow_batch_dev(glome_scene*, size_t n, const float* ox, const float* oy, const float* oz, const float* dx,
                           const float* dy, const float* dz, const float* tmax, uint8_t* occluded);

/* ---- whole-frame seam (renderTiles, Glome.hs:379-386; Scene tuple, TestScene.hs:15) ---- */
typedef struct glome_camera { float pos[3], fwd[3], up[3], right[3]; } glome_camera; /* Scene.hs:35 */
int glome_camera_lookat(const double pos[3], const double at[3], const double up[3], double angle_deg,
                        glome_camera* out); /* camera, Scene.hs:48-57 */
typedef struct glome_light {               /* Light, Shader.hs:13-23; falloff is fixed to 1/d^2 as `light` builds it */
  float pos[3], color[3], rad;
  int32_t shadow;
} glome_light;
enum { GLOME_MODE_TILE = 0 /* renderTile, Glome.hs:162-176 */, GLOME_MODE_SUBSAMPLE = 1 /* renderTileSubsample, :226-323 */ };
typedef struct glome_render_params {
  int32_t width, height;
  int32_t mode;          /* GLOME_MODE_* */
  int32_t blocksize;     /* tile edge, Glome.hs:116 (65) */
  int32_t maxdepth;      /* Glome.hs:25 (3); 1..8 supported */
  int32_t fog;           /* 1: TILE mode stores (r + depth/400, g, b, a, depth) exactly as renderTile does (Glome.hs:174,
                            Q20: a miss stores r = 2500); 0 -- the DEFAULT, a deliberate deviation from renderTile -- stores
                            the tuple get_color returns (Glome.hs:53-55) before that debug term */
  float thresholds[4];   /* Glome.hs:221-224 */
  int32_t tile_first, tile_stride; /* shard: render tiles tile_first, tile_first+tile_stride, ... (x-major order) */
  int32_t faithful;      /* 1: BIH traversal without ordered early-out, exactly as Bih.hs:332-368 visits nodes */
  int32_t count_work;    /* 1: count node visits / primitive tests (slower -- counting kernel instances; implied by faithful).
                            The generic tier always traverses with early-out (a ray that is not unit length excepted). */
  int32_t rank0_share_pct; /* shards of tile_stride ranks: 0 (or 100) = tile k belongs to rank k mod tile_stride; 1..99 = the
                            weight of rank 0, which also receives and blits every frame, in percent of one other rank's: rank
                            0 owns pct / (pct + 100 (tile_stride - 1)) of the tiles, the others split the rest evenly (an
                            evenly interleaved repeating pattern every rank derives from (tile_stride, percentage), every
                            percent a different one; parMap over tiles, Glome.hs:385, has no such notion -- a tile is a tile
                            whoever renders it) */
} glome_render_params;
void glome_render_params_default(glome_render_params*);
typedef struct glome_stats {
  uint64_t rays_primary, rays_shadow, rays_secondary; /* rays actually traversed */
  uint64_t bih_nodes, mesh_nodes, prim_tests;         /* only when count_work */
  float kernel_ms;                                    /* HIP-event time of the render kernel(s) on the ctx stream */
  int32_t n_tiles, n_pixels;
} glome_stats;
/* rgbad: width*height*5 floats (r,g,b,a,depth per pixel, row major; pixels of tiles this call does not own are
 * left untouched); packed: width*height 0x00RRGGBB words as blitTile/rgbf produce (Glome.hs:353-358, 107-110) or NULL. */
int glome_render(glome_scene*, const glome_camera*, const glome_light* lights, int nlights,
                 const glome_render_params*, float* rgbad, uint32_t* packed, glome_stats*);
/* Device-pointer variant.  Asynchronous on the ctx stream unless stats != NULL (then it synchronizes to read
 * the counters and the event timer).  rgbad_dev may be NULL when packed_dev is given: only the displayable pixels are
 * then written (trace and blitTile fused; the float tuple never leaves registers). */
int glome_render_dev(glome_scene*, const glome_camera*, const glome_light* lights, int nlights,
                     const glome_render_params*, float* rgbad_dev, uint32_t* packed_dev, glome_stats*);
/* Render the tiles owned by (params->tile_first, params->tile_stride) straight into a dense tile payload (what a
 * rank sends to the gather): tiles in owned order, row major inside a tile, 5 floats per pixel = the reference's
 * `Tile Rect (UV.Vector TColor)` (Glome.hs:153-154). */
int glome_render_tiles_dev(glome_scene*, const glome_camera*, const glome_light* lights, int nlights,
                           const glome_render_params*, float* payload_dev, glome_stats*);
/* The same render, but only the displayable pixel leaves the kernel: payload_dev receives one packed 0x00RRGGBB word per
 * owned pixel (rgbf of the premultiplied colour -- what blitTile, Glome.hs:353-358, pokes into GlomeView's framebuffer),
 * tiles in owned order, row major inside a tile.  This is the payload of the multi-GPU framebuffer gather (4 bytes per
 * pixel instead of 20).  GLOME_MODE_TILE and GLOME_MODE_SUBSAMPLE alike. */
int glome_render_tiles_packed_dev(glome_scene*, const glome_camera*, const glome_light* lights, int nlights,
                                  const glome_render_params*, uint32_t* payload_dev, glome_stats*);
/* Several independent frames in ONE launch (an animation's next views: same scene and lights, cams[0..nframes), at
 * most 32).  Frame f's pixels land frame_stride_pixels words after frame f-1's: rows of a dense tile payload
 * (..._tiles_packed_batch_dev; stride >= this rank's payload size) or whole packed framebuffers (..._packed_batch_dev;
 * stride >= width*height).  A rank's share of one frame is a few thousand work items -- too little to fill the GPU
 * beyond its slowest item; a batch restores long launches.  Both render modes (the adaptive sampler of a batch of 4 or
 * more frames works in larger regions per work item: fewer, fuller sample packets; the frames are unchanged). */
int glome_render_tiles_packed_batch_dev(glome_scene*, const glome_camera* cams, int nframes, const glome_light* lights, int nlights,
                                        const glome_render_params*, uint32_t* payload_dev, int64_t frame_stride_pixels, glome_stats*);
int glome_render_packed_batch_dev(glome_scene*, const glome_camera* cams, int nframes, const glome_light* lights, int nlights,
                                  const glome_render_params*, uint32_t* packed_dev, int64_t frame_stride_pixels, glome_stats*);
/* ---- the trace seam (Trace.trace, Trace.hs:53-82: "for most applications ... the entry point into the ray tracer") ----
 * For a host with a ray generator of its own (depth of field, a fisheye or stereo camera, a light probe, a sampler other than
 * renderTileSubsample, a picking ray): the device's own trace -- closest hit, the texture stack's fold (Trace.hs:67-80), the materials'
 * shaders with their shadow and secondary rays (Shader.hs:65-189) -- over caller-supplied SoA ray streams, in one launch.  A ray's result
 * is what glome_render computes for a pixel with that primary ray, and does not depend on the rays beside it in the stream. */
typedef struct glome_trace_params {
  int32_t maxdepth;    /* `recurs` of Trace.trace; 1..8, default 3 (Glome.hs:25) */
  int32_t faithful;    /* as glome_render_params.faithful; REQUIRED when directions are not unit length (below) */
  int32_t count_work;  /* as glome_render_params.count_work */
} glome_trace_params;
void glome_trace_params_default(glome_trace_params*);
/* trace lights materialShader root (Ray o d) tmax maxdepth, for n <= 2^31 rays (Trace.hs:59-82, Shader.hs:65-189).
 * rgbad: n*5 floats, (r, g, b, a, depth) per ray -- the tuple glome_render stores per pixel with fog = 0 (depth = ridepth, 1e6 for a
 * miss).  tmax may be NULL (every ray: infinity = 1e6, Vec.hs:14).  t / prim / nx / ny / nz / tex8: the trace's own Rayint
 * (TraceResult's third component, Trace.hs:49-51), laid out exactly as glome_rayint_batch writes them; any of them may be NULL.
 * Directions are used as given: `trace` does not normalise and neither does this.  The production traversal (ordered early-out) is
 * exact for unit-length rays only, so with faithful == 0 every direction must be unit length (|d|^2 within 1e-5 of 1); a launch that
 * meets another one fails with GLOME_E_INVALID -- at once when `stats` is given, else at the next glome_ctx_synchronize -- and its
 * outputs are not to be used.  With faithful == 1 the traversal is the reference's own and any direction is legal.
 * The _dev form takes device pointers and is asynchronous on the context's stream and slot unless stats != NULL; it takes part in
 * glome_ctx_timing_begin / _end like a render launch.  stats: rays_primary = n, shadow and secondary rays as in a render, n_tiles = the
 * 64-ray work items, n_pixels = n. */
int glome_trace_batch(glome_scene*, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                      const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params*,
                      float* rgbad, float* t, int32_t* prim, float* nx, float* ny, float* nz, int32_t* tex8, glome_stats*);
int glome_trace_batch_dev(glome_scene*, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                          const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params*,
                          float* rgbad, float* t, int32_t* prim, float* nx, float* ny, float* nz, int32_t* tex8, glome_stats*);
/* ---- per-ray work records (Trace.trace_debug, Trace.hs:84-109; rayint_debug, Solid.hs:155,205, Bih.hs:376-412) ----
 * glome_trace_batch again, but every ray also leaves a record of the work its trace did: what glome_stats counts for a whole launch,
 * for that ray alone -- GLOME_WORK_WORDS (8) uint32 PER RAY, ray i at work[8 i ..] (glome_work_words() returns what the loaded library
 * writes).  Words 0..2: BIH nodes, Mesh nodes and primitive tests of everything the ray's trace walked -- its closest hit, its shadow
 * rays, its reflection / refraction / Warp rays; words 3, 4: the shadow and secondary rays it spawned; words 5..7: words 0..2 as they
 * stood when the primary ray's closest hit returned, before mpreshade -- word 5 is the Int of trace_debug for a scene without Bound, the
 * number GlomeView tints a pixel with (get_color_debug, Glome.hs:35-41).  Over a launch words 0..4 sum to its glome_stats exactly.
 * The contract is glome_trace_batch's -- validation, the unit-length rule, tmax == NULL, n == 0, the asynchronous _dev form, timing --
 * but: `work` is required, and work_dev must be 16-byte aligned (else GLOME_E_INVALID); rgbad may be NULL, and then no colour is stored;
 * there are no hit streams; count_work is implied (the launch takes the counting kernel instance) and ignored, faithful is honoured.
 * A launch that fails leaves the records unspecified, as it leaves rgbad.  It costs what a count_work launch costs plus 32 bytes
 * stored per ray. */
#define GLOME_WORK_WORDS 8
enum { GLOME_WORK_BIH_NODES = 0, GLOME_WORK_MESH_NODES = 1, GLOME_WORK_PRIM_TESTS = 2, GLOME_WORK_RAYS_SHADOW = 3, GLOME_WORK_RAYS_SECONDARY = 4,
       GLOME_WORK_PRIMARY_BIH_NODES = 5, GLOME_WORK_PRIMARY_MESH_NODES = 6, GLOME_WORK_PRIMARY_PRIM_TESTS = 7 };
int glome_work_words(void);
int glome_trace_work_batch(glome_scene*, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                           const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params*,
                           float* rgbad, uint32_t* work, glome_stats*);
int glome_trace_work_batch_dev(glome_scene*, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                               const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params*,
                               float* rgbad_dev, uint32_t* work_dev, glome_stats*);
/* ---- frames through the trace seam: camera rays made on the device, and the per-pixel resolve of their results ----
 * The two stages a host with a lens of its own needs around glome_trace_batch_dev so that a frame's rays never cross the bus: raygen
 * stands where GlomeView makes a pixel's ray (getCoords / get_coords + get_rayint, Glome.hs:27-33, 119-140), resolve where it averages
 * a pixel's samples and pokes the word into the framebuffer (cAvg + blitTile, Glome.hs:191-197, 353-358).  The reference has one lens,
 * the pinhole of get_rayint; THIN and LATLONG have no counterpart there.
 * A frame's rays are ordered (y * width + x) * samples + s: a pixel's samples are consecutive.
 *   PINHOLE  get_rayint of the pixel's coordinates: with samples = 1, jitter = 0 the rays glome_render traces, bit for bit.
 *   THIN     thin lens: with dp the pinhole direction and f, r, u the camera's fwd, right and up normalised, the ray from the lens point
 *            L = pos + aperture sqrt(u2) (cos(2 pi u3) r + sin(2 pi u3) u) through the focal-plane point P = pos + dp focus_dist / (dp . f).
 *   LATLONG  light probe / panorama: longitude pi (2 (x + jx) / width - 1), latitude (pi / 2) yc (yc: get_coords' y, +1 at the top row);
 *            d = cos(lat) (cos(lon) f - sin(lon) r) + sin(lat) u, o = pos.  Every pixel has a ray.
 * (jx, jy) = (u0, u1) when jitter is set, else 0; every direction is normalised last, so the streams are legal for glome_trace_batch
 * with faithful = 0.  u_dim = (glome_raygen_sample(seed, y * width + x, s, dim) >> 8) * 2^-24, in [0, 1): dims 0, 1 the jitter, 2, 3 the
 * lens point.  With mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32 arithmetic), the word is
 * mix(mix(mix(seed + 0x9e3779b9 * (pixel + 1)) + s) + dim); the device computes the same word. */
enum { GLOME_LENS_PINHOLE = 0, GLOME_LENS_THIN = 1, GLOME_LENS_LATLONG = 2 };
typedef struct glome_raygen_params {
  int32_t width, height;
  int32_t lens;        /* GLOME_LENS_* */
  int32_t samples;     /* per pixel, 1..64 */
  int32_t jitter;      /* 0: every sample at the pixel's own coordinates (getCoords, Glome.hs:119-128); 1: + (u0, u1) in [0,1)^2 */
  uint32_t seed;
  float aperture;      /* THIN: lens radius, scene units (0 = a pinhole's rays up to rounding) */
  float focus_dist;    /* THIN: distance of the focal plane along the normalised fwd, > 0 */
} glome_raygen_params;
void glome_raygen_params_default(glome_raygen_params*);  /* 720x480 (Glome.hs:112-113), PINHOLE, 1 sample, no jitter, seed 0, aperture 0, focus 1 */
size_t glome_raygen_params_size(void);                   /* sizeof(glome_raygen_params) of the loaded library, for a binding to check */
/* Host-only.  What every entry below refuses, as GLOME_E_INVALID: a null pointer, width or height < 1, width * height > 2^30 (the limit
 * of glome_render), samples outside 1..64, an unknown lens, aperture or focus_dist not finite, THIN with focus_dist <= 0 or aperture < 0.
 * glome_raygen_count: width * height * samples, or GLOME_E_INVALID. */
int64_t glome_raygen_count(const glome_raygen_params*);
uint32_t glome_raygen_sample(uint32_t seed, uint32_t pixel, uint32_t s, uint32_t dim);  /* host-only: the word behind u_dim */
/* Rays first_ray .. first_ray + n_rays - 1 of the frame's order into elements 0 .. n_rays - 1 of the six streams.  The range need not be
 * a multiple of 64 nor start at a pixel's first sample; a call makes at most 2^31 rays (what one trace launch takes).  GLOME_E_INVALID,
 * before anything is launched or written: the params as above, a null context, camera or stream, a camera with a component that is not
 * finite, for THIN and LATLONG a fwd, right or up of length 0, a range that is negative or reaches past glome_raygen_count.  n_rays = 0
 * succeeds.  The _dev form is asynchronous on the context's stream and takes part in glome_ctx_timing_begin / _end like a render launch;
 * the host form stages the streams through device memory and is there for tests and small streams. */
int glome_camera_rays_dev(glome_ctx*, const glome_camera*, const glome_raygen_params*, int64_t first_ray, int64_t n_rays,
                          float* ox, float* oy, float* oz, float* dx, float* dy, float* dz);
int glome_camera_rays(glome_ctx*, const glome_camera*, const glome_raygen_params*, int64_t first_ray, int64_t n_rays,
                      float* ox, float* oy, float* oz, float* dx, float* dy, float* dz);
/* Pixels first_pixel .. first_pixel + n_pixels - 1 (row major) of a width x height frame from rgbad_samples, the n_pixels * samples
 * (r, g, b, a, depth) tuples glome_trace_batch wrote for those pixels' rays.  Per pixel r, g, b, a are each summed over s = 0 .. samples - 1
 * in that order -- fp32 additions starting from sample 0 -- and the sum is divided once by (float)samples, correctly rounded; depth is the
 * least of the samples' depths.  The order is part of the contract: a host reproduces the frame bit for bit.  rgbad (width * height * 5) and
 * packed (width * height words) are whole frames, and pixels outside the range are left untouched; packed gets the word glome_render
 * stores for a pixel with that (r, g, b, a) (rgbf of the premultiplied colour); samples = 1 copies the tuples.  Either output may be NULL,
 * not both.  GLOME_E_INVALID: a null context or input, both outputs null, width or height < 1, width * height > 2^30, samples outside
 * 1..64, a range that is negative or reaches past the frame.  Asynchronous; timed like glome_camera_rays_dev. */
int glome_resolve_dev(glome_ctx*, int32_t width, int32_t height, int32_t samples, int64_t first_pixel, int64_t n_pixels,
                      const float* rgbad_samples, float* rgbad, uint32_t* packed);
/* A frame of `cam` under the lens of the raygen params, in one call: for each pass of at most rays_per_pass rays (rounded down to whole
 * pixels, at least one pixel) raygen -> glome_trace_batch_dev -> resolve, all on the scene's context, its current stream and slot.  The
 * pass's rays and results live in a workspace the slot owns and grows on demand: 44 bytes per ray (six streams and the five-float
 * result; tmax is not needed).  rays_per_pass = 0 takes the default, 4M rays = 176 MiB -- a first guess (large enough that a pass fills
 * the GPU many times over, small enough to sit beside a scene), not a measured optimum.  The frame does not depend on rays_per_pass, bit
 * for bit, and equals the three stages called by hand.  rgbad and packed as glome_render's (either may be NULL, not both); faithful and
 * count_work of the trace params are passed through.  stats are summed over the passes, n_pixels = width * height, n_tiles = the trace
 * launches' 64-ray work items, kernel_ms = the HIP-event time of all three stages.  GLOME_E_INVALID, before anything is launched: what
 * glome_camera_rays_dev and glome_resolve_dev refuse, null trace params, bad lights, rays_per_pass < 0, and width * height * samples >
 * 2^31 -- a limit of this entry's bookkeeping, not of its passes, which are far below it; GLOME_E_LIMIT: maxdepth or the light count, as
 * glome_trace_batch.  The host form allocates and copies the frame like glome_render; the _dev form takes device frame pointers and is
 * asynchronous unless stats != NULL (a unit-length refusal cannot occur: raygen normalises). */
int glome_render_lens(glome_scene*, const glome_camera*, const glome_raygen_params*, const glome_light* lights, int nlights,
                      const glome_trace_params*, int64_t rays_per_pass, float* rgbad, uint32_t* packed, glome_stats*);
int glome_render_lens_dev(glome_scene*, const glome_camera*, const glome_raygen_params*, const glome_light* lights, int nlights,
                          const glome_trace_params*, int64_t rays_per_pass, float* rgbad_dev, uint32_t* packed_dev, glome_stats*);

/* ---- Adaptive sampling for lens frames: more samples only where the two halves of a pixel's samples differ.
 * glome_raygen_params.samples is the most a pixel gets (`max`).  Levels are n_0 = base, n_{k+1} = 2 n_k, up to max: base is even and at
 * least 2, max = base * 2^k with k >= 0, max <= 64.  For one pixel with tuples x_s = (r, g, b, a, depth) of samples s = 0 .. max - 1:
 *   S  the running fp32 sum of r, g, b, a: a copy of sample 0, then plain fp32 additions in index order (glome_resolve_dev's sum);
 *   d  the least depth so far (glome_resolve_dev's);
 *   at level n with h = n / 2: A is S as it stood after sample h - 1, B a fresh sum of samples h .. n - 1 (a copy of sample h, then
 *   additions in index order).  The pixel stops at n when fabsf(A_c - B_c) <= threshold * (float)h is true for each of the four channels
 *   -- one fp32 subtraction and one fp32 multiplication, round to nearest, never contracted; in words, the means of the two halves
 *   differ by at most threshold.  A comparison that is false -- one with a NaN too -- continues the pixel; at max it stops whatever the
 *   test says.
 * The result at count = n: r, g, b, a = S_c / (float)n correctly rounded, depth = d, the packed word rgbf(r a, g a, b a): what
 * glome_resolve_dev gives for samples = n, bit for bit.  (The device flushes subnormals like every kernel here; the identity with the
 * host functions holds where none arises.)
 * The defaults -- base 4, threshold 1/64 -- are a first guess, not tuned. */
typedef struct glome_adaptive_params {
  int32_t base_samples;  /* the first level: even, >= 2; raygen samples = base_samples * 2^k */
  float threshold;       /* >= 0; +inf is legal (every pixel stops at base_samples), NaN is not */
} glome_adaptive_params;
void glome_adaptive_params_default(glome_adaptive_params*);  /* base 4, threshold 1/64: a first guess, not tuned */
size_t glome_adaptive_params_size(void);                     /* sizeof(glome_adaptive_params) of the loaded library */
/* Host-only.  The levels of (base, max) into out[0 .. cap), returns how many there are (at most 6; out may be NULL with cap = 0);
 * GLOME_E_INVALID when (base, max) is not as above, or out is NULL with cap > 0. */
int glome_adaptive_levels(int32_t base, int32_t max, int32_t* out, int cap);
/* Host-only.  The rule for one pixel: tuples = max * 5 floats; writes the count, the (r, g, b, a, depth) result and the packed word.
 * GLOME_E_INVALID: a null pointer, a bad (base, max), a threshold that is NaN or negative.  The kernels below compile the same
 * definition of the step (glome_amd/csrc/adaptive_rule.hpp). */
int glome_adaptive_fold(const float* tuples, int32_t base, int32_t max, float threshold, int32_t* count, float rgbad[5], uint32_t* packed);
/* A frame like glome_render_lens's in which every pixel is glome_adaptive_fold of that pixel's max tuples -- the tuples glome_camera_rays
 * -> glome_trace_batch give for it at samples = max -- bit for bit in rgbad, packed and counts, whatever rays_per_pass is.  rgbad and
 * packed are whole frames (either may be NULL, not both); counts, width * height bytes, receives the level each pixel stopped at and may
 * be NULL.  Only the samples a pixel needs are made and traced.  A pass covers max(1, rays_per_pass / max) consecutive pixels
 * (rays_per_pass = 0: glome_render_lens's default) and runs in rounds: round 0 makes and traces samples [0, base) of every pixel of the
 * pass and folds them at level base; round k makes, traces and folds samples [n / 2, n) of the pixels the round before listed; the pass
 * ends when a list is empty or after level max.  The workspace is the slot's, grown on demand: 44 bytes per ray for the most rays a
 * round holds, pixels-per-pass * max(base, max / 2), and per pixel of a pass 20 bytes of state and two list words.
 * NOT asynchronous, in either form: the length of a round's list is read back (4 bytes), so the call waits for its stream once per
 * round of each pass -- the only blocking steps of the _dev form when stats is NULL; with stats every trace launch waits as well.  Every
 * launch takes part in glome_ctx_timing_begin / _end (one event pair each: raygen, trace, fold).  stats are summed over all trace
 * launches: rays_primary equals the sum of the counts, n_pixels = width * height, kernel_ms = the HIP-event time of all stages.
 * GLOME_E_INVALID / GLOME_E_LIMIT before anything is launched, the frames untouched: everything glome_render_lens refuses (with
 * samples = max; width * height * max > 2^31 among it), null adaptive params, what glome_adaptive_levels refuses of (base_samples,
 * samples), a threshold that is NaN or negative. */
int glome_render_lens_adaptive(glome_scene*, const glome_camera*, const glome_raygen_params*, const glome_light* lights, int nlights,
                               const glome_trace_params*, const glome_adaptive_params*, int64_t rays_per_pass,
                               float* rgbad, uint32_t* packed, uint8_t* counts, glome_stats*);
int glome_render_lens_adaptive_dev(glome_scene*, const glome_camera*, const glome_raygen_params*, const glome_light* lights, int nlights,
                                   const glome_trace_params*, const glome_adaptive_params*, int64_t rays_per_pass,
                                   float* rgbad_dev, uint32_t* packed_dev, uint8_t* counts_dev, glome_stats*);

/* Host-only, no device: the kernel instance a trace launch gets (choose_trace, glome_amd/csrc/instances.hpp).  n rows of 11 inputs -- the
 * eight scene traits of glome_sb_scene_traits, then faithful, count_work, maxdepth -- give n rows of 3 outputs: the instance (a flat-tier
 * key with the bits glome_kernel_choice describes, TWO_ROWS never set; -1 / -2: the generic tier's kernel that counts work / does not),
 * LB, and the wave slots per CU.  Returns n, or GLOME_E_INVALID for a null array. */
int64_t glome_trace_kernel_choice(int64_t n, const int64_t* in11, int32_t* out3);

/* ---- the whole-frame seam on several GPUs driven by ONE process (renderTiles' parMap over tiles + blitTile, Glome.hs:379-386) ----
 * scenes[i] = the same scene committed on context i (a context per GPU; rank 0's GPU receives the frame).  Tile k of the
 * frame -- 64x64 work tiles in renderTile mode, the 65x65 reference tiles in adaptive mode (whose pixels depend on the tile
 * map, Q21) -- belongs to rank k mod n, or to the rank the weighted pattern of glome_render_params.rank0_share_pct gives it.
 * A call renders nframes <= 32 views (one in adaptive mode), every rank its tiles of all of them in one launch.  How the pixels
 * reach packed_dev (frame f at f * width * height words) is the TRANSPORT (glome_multi_transport says which was taken):
 *   2 "direct"     every rank's render kernel stores its tiles' packed 0x00RRGGBB pixels straight into packed_dev on rank 0's GPU
 *                  (4 bytes per pixel over xGMI); rank 0's stream waits for the others' launches.  No payload, no exchange, no blit,
 *                  and every rank owns a fair share of the tiles (rank0_share_pct is ignored).  Needs every rank's device to reach rank
 *                  0's memory (the same device, or peer access); asked for and not possible -> "rccl" / "peer-copy" as below.
 *   1 "rccl"       ranks render into packed payloads, which move to rank 0's GPU with RCCL send / recv in one group (librccl.so is
 *                  dlopen'ed; the ranks must sit on distinct devices), and one launch there blits the frames into packed_dev.
 *   0 "peer-copy"  the same with peer copies on rank 0's stream.
 * Asynchronous; glome_multi_synchronize waits for all ranks and reports device-side limits.
 * The RCCL branch needs distinct devices and has not run on real RCCL with more than one rank on this pool (one-GPU boxes): it
 * is exercised against a stand-in transport whose send / recv pairs are stream-ordered device copies (tests/rcclstub). */
/* ---- a framebuffer several processes render into (one process per GPU, glome_amd/dist.py) ----
 * glome_ipc_alloc: device memory on this context's GPU (zeroed) and a 64-byte handle another process passes to glome_ipc_open to
 * map it; a rank then renders its tiles of a frame with glome_render_packed_batch_dev (tile_first / tile_stride set, frame
 * layout) straight into the mapping -- its kernel's stores cross xGMI, nothing is gathered or blitted.  glome_ipc_close: the
 * owner frees, the others unmap.  (HIP IPC; on this driver dmabuf handles: HSA_ENABLE_IPC_MODE_LEGACY=0.) */
int glome_ipc_alloc(glome_ctx*, size_t bytes, void** dev_ptr, unsigned char* handle64);
int glome_ipc_open(glome_ctx*, const unsigned char* handle64, void** dev_ptr);
int glome_ipc_close(glome_ctx*, void* dev_ptr, int owner);
typedef struct glome_multi glome_multi;
glome_multi* glome_multi_create(glome_scene* const* scenes, int n, const glome_render_params*, int transport); /* 0 / 1 / 2 as above; NULL: glome_global_error() */
void glome_multi_destroy(glome_multi*);
int glome_multi_render(glome_multi*, const glome_camera* cams, int nframes, const glome_light* lights, int nlights, uint32_t* packed_dev);
int glome_multi_synchronize(glome_multi*);
const char* glome_multi_transport(const glome_multi*); /* "direct", "rccl", "peer-copy" or "none" (one rank) */
const char* glome_multi_last_error(const glome_multi*);
/* One frame into a host framebuffer (width * height words): create, render, synchronize, copy, destroy. */
int glome_render_multi(glome_scene* const* scenes, int n, const glome_camera*, const glome_light* lights, int nlights,
                       const glome_render_params*, uint32_t* packed);
/* Tile payload transport for multi-GPU sharding (Tile = Rect + pixel vector, Glome.hs:153-154).
 * pack: copy this rank's owned tiles from a full frame into a dense payload (tiles in owned order, row major
 * inside a tile, 5 floats per pixel).  blit: scatter a payload of the tiles owned by (tile_first, tile_stride)
 * back into a full frame (blitTile, Glome.hs:353-358).  glome_tiles_payload_floats gives the payload size. */
int64_t glome_tiles_payload_floats(const glome_render_params*, int tile_first, int tile_stride);
/* Host-only: the tiles owned by (tile_first, tile_stride) in renderTiles' order (Glome.hs:382-384).  Writes 5 ints per
 * tile (x, y, w, h, pixel offset of the tile inside the dense payload) and returns the tile count. */
int glome_tiles_layout(const glome_render_params*, int tile_first, int tile_stride, int32_t* xywh_base, int cap);
/* Host-only: the pixels of the 64-lane work items of that plan (blocksize_override > 0: tiles of that edge instead of the params'), 4 ints
 * per lane: valid, x, y, offset inside the dense payload.  which 0: by the tile arithmetic (work_to_pixel); 1: by the plan's item table, as
 * the lean render loop decodes it.  Writes up to cap_items items and returns the item count. */
int64_t glome_items_layout(const glome_render_params*, int tile_first, int tile_stride, int blocksize_override, int which, int32_t* out, int64_t cap_items);
/* Host-only: which kernel instance a launch gets (the rules of glome_amd/csrc/instances.hpp; no device is touched).  n rows of 14 inputs
 *   tier, cls_mask, has_secondary_mats, has_nested_mats, has_refract, pk_all, stack_cap, n_bih_nodes,   (the scene: glome_sb_scene_traits)
 *   mode, faithful, count_work, maxdepth, tile_stride, items                                            (the params; items: work items of the launch)
 * give n rows of 4 outputs: the kind (0 render kernel, 1 adaptive sampler); the instance -- a flat-tier key, which holds the kernel's
 * template arguments as bits 0 FAITHFUL, 1 COUNT, 2 FULL, 3 TWO_ROWS, 4-7 LB (waves per SIMD), 8-13 CLS (entry classes), or -1 / -2 for
 * the generic tier's kernel that counts work / does not --; two_rows; the wave slots per CU a persistent grid is capped by.
 * Returns n, or GLOME_E_INVALID for a null array or an unknown mode. */
int64_t glome_kernel_choice(int64_t n, const int64_t* in14, int32_t* out4);
/* Host-only: what a commit of `root` would derive for that choice.  out11: the first eight inputs above, then ovf_cap, pk_generic_cap
 * (without the debug switch of the environment) and n_mesh_nodes.  pk_all: every triangle bih of the scene has the hand-written walk's
 * node form and, where triangle bihs are the scene's only entry class, every root entry is a bih. */
int glome_sb_scene_traits(glome_sb*, int32_t root, int64_t* out11);
/* The lean render loop's pixel-coordinate tables of a frame size (xc[width], yc[height]; made on the device, once per context), or with
 * direct != 0 the same values evaluated per pixel by the coordinate function itself. */
int glome_ctx_coord_tables(glome_ctx*, int width, int height, float* xc, float* yc, int direct);
/* What the cull pass of the last flagship launch on the current slot found (the launches glome_kernel_choice reports two_rows for; their
 * work items whose rays all miss the scene's root bounds are finished before the render kernel and never queued): `total` work items of
 * the launch (all its frames), `live` of them queued.  Synchronizes the context's stream.  0 / 0 before the slot's first such launch. */
int glome_ctx_last_cull(glome_ctx*, int64_t* live, int64_t* total);
int glome_tiles_pack_dev(glome_ctx*, const glome_render_params*, const float* rgbad_dev, float* payload_dev);
int glome_tiles_blit_dev(glome_ctx*, const glome_render_params*, int tile_first, int tile_stride,
                         const float* payload_dev, float* rgbad_dev, uint32_t* packed_dev);
/* After the gather: `gathered_dev` holds `world` payload slabs of `stride_floats` floats each (rank r's payload at
 * gathered_dev + r * stride_floats).  One launch blits every rank's tiles into the frame. */
int glome_tiles_blit_all_dev(glome_ctx*, const glome_render_params*, int world, const float* gathered_dev, int64_t stride_floats,
                             float* rgbad_dev, uint32_t* packed_dev);
/* The packed-pixel form: `gathered_dev` holds `world` slabs of `stride_pixels` words (glome_render_tiles_packed_dev
 * payloads); one launch writes every rank's tiles into the packed framebuffer (width*height words). */
int glome_tiles_blit_all_packed_dev(glome_ctx*, const glome_render_params*, int world, const uint32_t* gathered_dev, int64_t stride_pixels,
                                    uint32_t* packed_dev);
/* The same for the nframes frames of a batch in one launch: frame f's payload starts f * payload_frame_stride words into
 * every rank's slab, its framebuffer f * out_frame_stride words after packed_dev. */
int glome_tiles_blit_all_packed_batch_dev(glome_ctx*, const glome_render_params*, int world, const uint32_t* gathered_dev, int64_t stride_pixels,
                                          int nframes, int64_t payload_frame_stride, uint32_t* packed_dev, int64_t out_frame_stride);

#ifdef __cplusplus
}
#endif
#endif /* GLOME_HIP_H */
