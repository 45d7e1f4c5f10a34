// xfm_sources.hpp -- an Instance's 24 doubles (forward rows, inverse rows) from what a producer of rigid motion holds: a forward 3x4
// matrix, or a pose (translation, quaternion, uniform scale); and the product of two such pairs.  The arithmetic of
// glome_xfm_from_forward / _from_pose / _mult and of glome_scene_instance_update_from (include/glome_hip.h states it), written ONCE:
// capi_host.cpp (g++) and runtime.hip (host and device) include this file, and the host functions and the conversion kernel
// (item_bih_update_kernels.hpp: k_xfm_convert) call the same bodies.  Every operation is one round-to-nearest fp64 operation, in the
// order written: on the host a plain fp64 operation inside a function of its own (nothing spans two of them, so nothing contracts), on
// the device __dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn -- as update_common.hpp spells tri_record against
// host_graph.hpp.  No function here reads or writes memory other than its arguments.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GLOME_XFM_FN __host__ __device__ __forceinline__
#else
#define GLOME_XFM_FN inline
#endif

namespace glome {
namespace xfm {

constexpr int kPair = 0, kForward = 1, kPose = 2;  // GLOME_XFM_PAIR / _FORWARD / _POSE
// values per item of a form: 24 / 12 / 8; 0 for a form there is none of
GLOME_XFM_FN int width_of(int form) { return form == kPair ? 24 : form == kForward ? 12 : form == kPose ? 8 : 0; }

#if defined(__HIP_DEVICE_COMPILE__)
GLOME_XFM_FN double add(double a, double b) { return __dadd_rn(a, b); }
GLOME_XFM_FN double sub(double a, double b) { return __dsub_rn(a, b); }
GLOME_XFM_FN double mul(double a, double b) { return __dmul_rn(a, b); }
GLOME_XFM_FN double div(double a, double b) { return __ddiv_rn(a, b); }
GLOME_XFM_FN double root(double a) { return __dsqrt_rn(a); }
GLOME_XFM_FN bool finite(double a) { return isfinite(a); }
#else
GLOME_XFM_FN double add(double a, double b) { return a + b; }
GLOME_XFM_FN double sub(double a, double b) { return a - b; }
GLOME_XFM_FN double mul(double a, double b) { return a * b; }
GLOME_XFM_FN double div(double a, double b) { return a / b; }
GLOME_XFM_FN double root(double a) { return std::sqrt(a); }
GLOME_XFM_FN bool finite(double a) { return std::isfinite(a); }
#endif

// column 3 of the inverse rows from their 3x3 part and the forward translation: i[r][3] = -(((i[r][0] tx) + (i[r][1] ty)) + (i[r][2] tz))
GLOME_XFM_FN void inverse_column(double inv[12], const double t[3]) {
  for (int r = 0; r < 3; r++) inv[4 * r + 3] = -add(add(mul(inv[4 * r], t[0]), mul(inv[4 * r + 1], t[1])), mul(inv[4 * r + 2], t[2]));
}

// POSE: p = tx ty tz qx qy qz qw s, the forward map v -> t + s R(q) v.  False for a quaternion of length 0 or s <= 0 (out is written
// all the same: whatever the expressions give).
GLOME_XFM_FN bool from_pose(const double p[8], double out[24]) {
  const double* t = p;
  const double s = p[7];
  const double len2 = add(add(add(mul(p[3], p[3]), mul(p[4], p[4])), mul(p[5], p[5])), mul(p[6], p[6]));
  const double inv = div(1.0, root(len2));  // normalize, host_graph.hpp
  const double x = mul(p[3], inv), y = mul(p[4], inv), z = mul(p[5], inv), w = mul(p[6], inv);
  const double xx = mul(x, x), yy = mul(y, y), zz = mul(z, z);
  const double xy = mul(x, y), xz = mul(x, z), yz = mul(y, z), xw = mul(x, w), yw = mul(y, w), zw = mul(z, w);
  double R[9];
  R[0] = sub(1.0, mul(2.0, add(yy, zz))); R[1] = mul(2.0, sub(xy, zw));           R[2] = mul(2.0, add(xz, yw));
  R[3] = mul(2.0, add(xy, zw));           R[4] = sub(1.0, mul(2.0, add(xx, zz))); R[5] = mul(2.0, sub(yz, xw));
  R[6] = mul(2.0, sub(xz, yw));           R[7] = mul(2.0, add(yz, xw));           R[8] = sub(1.0, mul(2.0, add(xx, yy)));
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      out[4 * r + c] = mul(s, R[3 * r + c]);
      out[12 + 4 * r + c] = div(R[3 * c + r], s);
    }
    out[4 * r + 3] = t[r];
  }
  inverse_column(out + 12, t);
  return len2 > 0.0 && s > 0.0;
}

// FORWARD: m = a row-major 3x4 forward matrix; the inverse 3x3 is the transposed cofactor matrix, each entry divided by det.  Returns det.
GLOME_XFM_FN double from_forward(const double m[12], double out[24]) {
  const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
  double c[9];  // c[3 r + c]: the cofactor of a[r][c]
  c[0] = sub(mul(a11, a22), mul(a12, a21)); c[1] = sub(mul(a12, a20), mul(a10, a22)); c[2] = sub(mul(a10, a21), mul(a11, a20));
  c[3] = sub(mul(a02, a21), mul(a01, a22)); c[4] = sub(mul(a00, a22), mul(a02, a20)); c[5] = sub(mul(a01, a20), mul(a00, a21));
  c[6] = sub(mul(a01, a12), mul(a02, a11)); c[7] = sub(mul(a02, a10), mul(a00, a12)); c[8] = sub(mul(a00, a11), mul(a01, a10));
  const double det = add(add(mul(a00, c[0]), mul(a01, c[1])), mul(a02, c[2]));
  const double t[3] = {m[3], m[7], m[11]};
  for (int q = 0; q < 12; q++) out[q] = m[q];
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) out[12 + 4 * r + k] = div(c[3 * k + r], det);
  inverse_column(out + 12, t);
  return det;
}

// mmul of host_graph.hpp (mat_mult, Vec.hs:426-443), its sums left to right
GLOME_XFM_FN void mmul34(const double A[12], const double B[12], double o[12]) {
  for (int r = 0; r < 3; r++) {
    const double* a = A + 4 * r;
    for (int k = 0; k < 3; k++) o[4 * r + k] = add(add(mul(a[0], B[k]), mul(a[1], B[4 + k])), mul(a[2], B[8 + k]));
    o[4 * r + 3] = add(add(add(mul(a[0], B[3]), mul(a[1], B[7])), mul(a[2], B[11])), a[3]);
  }
}
// a applied after b: xfm_mult a b (Vec.hs:447-449) = Xf{ mmul(a.f, b.f), mmul(b.i, a.i) }.  out is neither a nor b.
GLOME_XFM_FN void mult(const double a[24], const double b[24], double out[24]) {
  mmul34(a, b, out);
  mmul34(b + 12, a + 12, out + 12);
}

// One item of a source, widened to doubles in v (width_of(form) of them), as 24 doubles; false for what the POSE form refuses.
GLOME_XFM_FN bool convert(int form, const double* v, double out[24]) {
  if (form == kPose) return from_pose(v, out);
  if (form == kForward) { (void)from_forward(v, out); return true; }
  for (int q = 0; q < 24; q++) out[q] = v[q];
  return true;
}

}  // namespace xfm
}  // namespace glome
