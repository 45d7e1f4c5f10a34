// lens_kernels.hpp -- the two stages around a trace launch that make the trace seam render frames (glome_camera_rays, glome_resolve,
// glome_render_lens): the device code.  Templates only, like trace_kernels.hpp; an instance exists where kernel_parts.hip launches it.
//
//   k_camera_rays<>     a camera's rays under a lens model, straight into the SoA streams glome_trace_batch_dev reads: one lane per ray,
//                       a work item is 64 consecutive rays of the frame's order (y * width + x) * samples + s
//   k_resolve<SB>       `samples` consecutive results per pixel folded into the frame glome_render writes: (r, g, b, a, depth) and the
//                       packed 0x00RRGGBB word; one wave per 64 consecutive pixels, the wave's block staged through LDS SB samples at a time
//
// Both are memory-bound and small beside the trace between them: plain grids, no ticket, no inline assembly.
#pragma once
#include "rt_device.hpp"

// u_dim of (pixel, s): 24 bits of the sample word, in [0, 1) and exact in fp32
GD float raygen_u(const DLensArgs& A, uint32_t pixel, uint32_t s, uint32_t dim) { return (float)(raygen_word(A.seed, pixel, s, dim) >> 8) * 0x1p-24f; }

// t / samples for the lanes of an item.  `samples` is wave-uniform: a power of two is a shift, anything else one 32-bit division.
GD uint32_t div_samples(uint32_t t, uint32_t samples) {
  switch (samples) {
    case 1: return t;
    case 2: return t >> 1;
    case 4: return t >> 2;
    case 8: return t >> 3;
    case 16: return t >> 4;
    case 32: return t >> 5;
    case 64: return t >> 6;
    default: return t / samples;
  }
}

// One ray.  (xf, yf): the pixel's coordinates plus its jitter; xc, yc: get_coordsf's, as every render loop takes them.
//   PINHOLE  primary_ray itself (get_rayint, Glome.hs:27-33): without jitter the render kernels' rays
//   THIN     the pinhole ray's point on the focal plane, seen from a point of the lens disc.  P - L is taken without the detour through
//            pos (P = pos + dp k, L = pos + l: P - L = dp k - l), which keeps the direction's error free of |pos|
//   LATLONG  longitude across the frame's width, latitude by yc: the whole sphere of directions around pos
// Every direction is normalised last: unit length under the trace seam's rule.
GD Ray lens_ray(const DLensArgs& A, uint32_t pixel, uint32_t s) {
  const uint32_t y = pixel / (uint32_t)A.width, x = pixel - y * (uint32_t)A.width;
  float xf = (float)x, yf = (float)y;
  if (A.jitter) { xf = xf + raygen_u(A, pixel, s, 0); yf = yf + raygen_u(A, pixel, s, 1); }
  float xc, yc;
  get_coordsf(A.width, A.height, xf, yf, xc, yc);
  if (A.lens == LENS_PINHOLE) return primary_ray(A.cam, xc, yc);
  const V3 fh = v3(A.fhat[0], A.fhat[1], A.fhat[2]), rh = v3(A.rhat[0], A.rhat[1], A.rhat[2]), uh = v3(A.uhat[0], A.uhat[1], A.uhat[2]);
  Ray r;
  r.o = v3(A.cam.pos[0], A.cam.pos[1], A.cam.pos[2]);
  if (A.lens == LENS_THIN) {
    const V3 dp = primary_ray(A.cam, xc, yc).d;
    const float k = A.focus_dist / vdot(dp, fh);
    float sn, cs;
    sincospif(2.0f * raygen_u(A, pixel, s, 3), &sn, &cs);
    const float rad = A.aperture * sqrtf(raygen_u(A, pixel, s, 2));
    const V3 l = (rh * cs + uh * sn) * rad;
    r.o = r.o + l;
    r.d = vnorm(dp * k - l);
    return r;
  }
  // LATLONG
  float sl, cl, sb, cb;
  sincospif((div_ieee(xf, (float)A.width) * 2) - 1, &sl, &cl);
  sincospif(0.5f * yc, &sb, &cb);
  r.d = vnorm((fh * cl - rh * sl) * cb + uh * sb);
  return r;
}

// Grid-stride over the launch's 64-ray items, like trace_batch_loop; six coalesced stream stores per wave, 256 contiguous bytes each.
// The ray index is first_pixel * samples + first_s + j (j: the ray's offset in the launch, < 2^31): its pixel and sample come from
// t = first_s + j by the one division by `samples`.
template <int = 0>
__global__ void __launch_bounds__(64) k_camera_rays(DLensArgs A) {
  const uint32_t lane = threadIdx.x, samples = (uint32_t)A.samples;
  const uint32_t items = (A.n + 63u) >> 6;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t j = item * 64u + lane;
    if (j >= A.n) continue;
    const uint32_t t = A.first_s + j, q = div_samples(t, samples);
    const Ray r = lens_ray(A, A.first_pixel + q, t - q * samples);
    A.ox[j] = r.o.x; A.oy[j] = r.o.y; A.oz[j] = r.o.z;
    A.dx[j] = r.d.x; A.dy[j] = r.d.y; A.dz[j] = r.d.z;
  }
}

// The resolve.  A wave owns 64 consecutive pixels; their samples are one contiguous block of 64 * samples * 20 bytes, which the wave
// streams in with coalesced loads -- 16 bytes per lane when the whole block goes through LDS at once (samples <= SB) -- instead of every
// lane striding 20 * samples bytes through global memory.  With more than SB samples the block is staged SB samples at a time: 64 runs of
// SB * 20 contiguous bytes, a word per lane.
// In LDS a pixel's run of nb samples starts at pixel * stride, stride = nb * 5 | 1 words: odd, so the 32 lanes of a half-wave, each
// reading word k of its own run, sit on 32 different banks whatever nb is (nb * 5 itself is even for every even nb).
// Each lane then sums its pixel's samples in index order -- r, g, b, a as plain fp32 additions starting from sample 0, the order being
// part of the contract -- and divides once, correctly rounded; depth is the nearest sample's.  samples = 1 copies the tuple.
template <int SB>
__global__ void __launch_bounds__(64) k_resolve(DResolveArgs A) {
  constexpr uint32_t kStrideMax = (uint32_t)SB * 5u + 1u;
  __shared__ float tile[64 * kStrideMax];
  const uint32_t lane = threadIdx.x, samples = (uint32_t)A.samples;
  const uint32_t p0 = blockIdx.x * 64u;
  if (p0 >= A.n_pixels) return;
  const uint32_t np = A.n_pixels - p0 < 64u ? A.n_pixels - p0 : 64u;
  const float* src = A.samples_in + (size_t)p0 * samples * 5;
  float r = 0, g = 0, b = 0, a = 0, d = 0;
  for (uint32_t s0 = 0; s0 < samples; s0 += (uint32_t)SB) {
    const uint32_t nb = samples - s0 < (uint32_t)SB ? samples - s0 : (uint32_t)SB;
    const uint32_t run = nb * 5u, stride = run | 1u, total = np * run;
    // m / run for m < 64 * SB * 5 by multiply-shift (run = 5 nb is never a power of two: ceil(2^20 / run) = 2^20 / run + 1; exact while
    // m * (run - 1) < 2^20)
    static_assert(64u * SB * 5u * (SB * 5u) <= (1u << 20) && SB <= kMaxLensSamples, "k_resolve: the multiply-shift's range");
    const uint32_t magic = (1u << 20) / run + 1u;
    if (s0) __syncthreads();  // (the lanes are done with the block before)
    if (A.vec && nb == samples) {  // the whole block at once: word m of LDS run m / run is word m of the block
      for (uint32_t m = lane * 4u; m < total; m += 256u) {
        if (m + 4u <= total) {
          const float4 v = *reinterpret_cast<const float4*>(src + m);
          const float w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (uint32_t k = 0; k < 4u; k++) { const uint32_t p = ((m + k) * magic) >> 20; tile[p * stride + (m + k - p * run)] = w[k]; }
        } else {
          for (uint32_t k = m; k < total; k++) { const uint32_t p = (k * magic) >> 20; tile[p * stride + (k - p * run)] = src[k]; }
        }
      }
    } else {
      for (uint32_t m = lane; m < total; m += 64u) {
        const uint32_t p = (m * magic) >> 20, k = m - p * run;
        tile[p * stride + k] = src[((size_t)p * samples + s0) * 5 + k];
      }
    }
    __syncthreads();
    if (lane < np) {
      const float* t = tile + lane * stride;
      uint32_t k = 0;
      if (s0 == 0) { r = t[0]; g = t[1]; b = t[2]; a = t[3]; d = t[4]; k = 1; }
      for (; k < nb; k++) {
        const float* e = t + k * 5u;
        r = r + e[0]; g = g + e[1]; b = b + e[2]; a = a + e[3];
        d = e[4] < d ? e[4] : d;
      }
    }
  }
  if (lane >= np) return;
  const float n = (float)samples;  // (x / 1 is x: one sample is copied)
  r = div_ieee(r, n); g = div_ieee(g, n); b = div_ieee(b, n); a = div_ieee(a, n);
  const size_t o = (size_t)A.first_pixel + p0 + lane;
  if (A.rgbad) {
    float* out = A.rgbad + o * 5;
    out[0] = r; out[1] = g; out[2] = b; out[3] = a; out[4] = d;
  }
  if (A.packed) A.packed[o] = rgbf(r * a, g * a, b * a);  // blitTile (Glome.hs:353-358): store_pixel's word
}
