// adaptive_rule.hpp -- the rule of glome_render_lens_adaptive (include/glome_hip.h states it), written ONCE: capi_host.cpp (g++) calls
// these bodies for glome_adaptive_fold and glome_adaptive_levels, lens_adaptive_kernels.hpp calls them in the fold kernels, and the two
// must agree to the bit -- as raygen_word (rt_types.h) and xfm_sources.hpp do for their seams.
// A pixel's samples arrive in index order.  Levels are base, 2 base, .. max; at level n, h = n / 2:
//   S   the running fp32 sum of (r, g, b, a): a copy of sample 0, then plain additions -- k_resolve's sum
//   d   the least depth so far, by k_resolve's compare-select
//   A   S as it stood after sample h - 1;  B  a fresh sum of samples h .. n - 1: a copy of sample h, then additions
// and the pixel stops at n when |A_c - B_c| <= threshold * (float)h holds for all four channels (a comparison with a NaN is false: the
// pixel goes on), or when n is the last level.
// Every operation is one round-to-nearest fp32 operation in the order written: on the host a plain operation in a function of its own
// (nothing spans two of them, so nothing contracts), on the device __fadd_rn / __fsub_rn / __fmul_rn; the quotient goes through fp64
// like div_ieee (rt_device.hpp).  No function here reads or writes memory other than its arguments.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GLOME_ADP_FN __host__ __device__ __forceinline__
#else
#define GLOME_ADP_FN inline
#endif

namespace glome {
namespace adaptive {

constexpr int kMaxLevels = 6;  // base >= 2, max <= 64: 2, 4, .. 64

#if defined(__HIP_DEVICE_COMPILE__)
GLOME_ADP_FN float add(float a, float b) { return __fadd_rn(a, b); }
GLOME_ADP_FN float sub(float a, float b) { return __fsub_rn(a, b); }
GLOME_ADP_FN float mul(float a, float b) { return __fmul_rn(a, b); }
GLOME_ADP_FN float mag(float a) { return fabsf(a); }
#else
GLOME_ADP_FN float add(float a, float b) { return a + b; }
GLOME_ADP_FN float sub(float a, float b) { return a - b; }
GLOME_ADP_FN float mul(float a, float b) { return a * b; }
GLOME_ADP_FN float mag(float a) { return std::fabs(a); }
#endif
GLOME_ADP_FN float quot(float a, float b) { return (float)((double)a / (double)b); }  // correctly rounded: 53 >= 2 * 24 + 2 bits

// base even and >= 2, max = base * 2^k <= 64
GLOME_ADP_FN bool legal(int32_t base, int32_t max) {
  if (base < 2 || (base & 1) || max < base || max > 64) return false;
  int32_t n = base;
  while (n < max) n *= 2;
  return n == max;
}

struct Fold {
  float S[4], d;     // what a pixel that goes on keeps between levels: 20 bytes
  float A[4], B[4];  // of the level at hand
};

// Sample s of the pixel, t = its (r, g, b, a, depth), at the level whose half is h.  Sample 0 starts the pixel; sample h takes the
// snapshot and starts B.
GLOME_ADP_FN void take(Fold& F, uint32_t s, uint32_t h, const float* t) {
  if (s == 0) {
    for (int c = 0; c < 4; c++) F.S[c] = t[c];
    F.d = t[4];
    return;
  }
  if (s == h) {
    for (int c = 0; c < 4; c++) { F.A[c] = F.S[c]; F.B[c] = t[c]; }
  } else if (s > h) {
    for (int c = 0; c < 4; c++) F.B[c] = add(F.B[c], t[c]);
  }
  for (int c = 0; c < 4; c++) F.S[c] = add(F.S[c], t[c]);
  F.d = t[4] < F.d ? t[4] : F.d;
}

// After sample 2 h - 1: do the halves agree?
GLOME_ADP_FN bool agrees(const Fold& F, uint32_t h, float threshold) {
  const float lim = mul(threshold, (float)h);
  bool ok = true;
  for (int c = 0; c < 4; c++) ok = (mag(sub(F.A[c], F.B[c])) <= lim) && ok;
  return ok;
}

// The pixel's (r, g, b, a, depth) at count n: k_resolve's for samples = n.
GLOME_ADP_FN void result(const Fold& F, uint32_t n, float out[5]) {
  const float nf = (float)n;
  for (int c = 0; c < 4; c++) out[c] = quot(F.S[c], nf);
  out[4] = F.d;
}

}  // namespace adaptive
}  // namespace glome
