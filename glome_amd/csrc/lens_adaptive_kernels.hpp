// lens_adaptive_kernels.hpp -- the device code of glome_render_lens_adaptive beside lens_kernels.hpp's two stages: a pass runs in rounds,
// one per level of the rule (adaptive_rule.hpp), and a pixel leaves at the level where the two halves of its samples agree.
//
//   k_adaptive_fold<SB, true>    round 0, after k_camera_rays and a trace of samples [0, base) of every pixel of the pass: the step at level
//                                base.  One wave per 64 consecutive pixels, their block staged through LDS as k_resolve stages it
//   k_camera_rays_list<>         round k: samples [n / 2, n) of the pixels the round before listed, through lens_ray itself; an entry's
//                                rays are consecutive, so its results are one contiguous run
//   k_adaptive_fold<SB, false>   round k, after the trace: one wave per 64 consecutive entries, the same staging; B from the new tuples,
//                                S continued with them, the step at level n
//
// A pixel that stops is written to the frames (k_resolve's words for samples = n); one that goes on stores S and d (20 bytes) and is
// appended to the next round's list: one ballot and one atomic add per wave, the lanes placed by their rank in the ballot.  The order of
// a list is whatever the waves' atomics make it; no frame depends on it.  No lane waits for another block.  Streaming kernels: plain
// grids, no ticket, no inline assembly.
#pragma once
#include "adaptive_rule.hpp"
#include "lens_kernels.hpp"

// Grid-stride over the launch's 64-ray items like k_camera_rays.  h is wave-uniform; an entry read from the list is clamped to the pass.
template <int = 0>
__global__ void __launch_bounds__(64) k_camera_rays_list(DLensListArgs A) {
  const DLensArgs& L = A.L;
  const uint32_t lane = threadIdx.x, h = A.h;
  const uint32_t items = (L.n + 63u) >> 6;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t j = item * 64u + lane;
    if (j >= L.n) continue;
    const uint32_t e = div_samples(j, h);
    uint32_t p = A.list[e];
    p = p < A.pass_pixels ? p : A.pass_pixels - 1u;
    const Ray r = lens_ray(L, L.first_pixel + p, h + (j - e * h));
    L.ox[j] = r.o.x; L.oy[j] = r.o.y; L.oz[j] = r.o.z;
    L.dx[j] = r.d.x; L.dy[j] = r.d.y; L.dz[j] = r.d.z;
  }
}

// The fold at one level.  `per` tuples per entry lie in samples_in -- the whole level in round 0, its second half later -- and the wave's
// 64 entries are one contiguous block of 64 * per * 20 bytes, staged as k_resolve stages its block: at once with 16-byte loads when per
// <= SB (the workspace is 256-byte aligned and a wave's block starts a multiple of 1280 bytes in), else SB samples at a time; in LDS an
// entry's run starts at lane * (nb * 5 | 1) words.  Each lane then feeds its tuples to the rule in index order.
template <int SB, bool FIRST>
__global__ void __launch_bounds__(64) k_adaptive_fold(DAdaptFoldArgs A) {
  constexpr uint32_t kStrideMax = (uint32_t)SB * 5u + 1u;
  __shared__ float tile[64 * kStrideMax];
  const uint32_t lane = threadIdx.x, level = (uint32_t)A.level, h = level >> 1;
  const uint32_t per = FIRST ? level : h, s_first = FIRST ? 0u : h;
  const uint32_t e0 = blockIdx.x * 64u;
  if (e0 >= A.n) return;
  const uint32_t ne = A.n - e0 < 64u ? A.n - e0 : 64u;
  const bool active = lane < ne;
  const float* src = A.samples_in + (size_t)e0 * per * 5;
  glome::adaptive::Fold F = {};
  uint32_t entry = e0 + lane;  // round 0: the pixel itself
  if (!FIRST && active) {
    entry = A.list_in[e0 + lane];
    entry = entry < A.pass_pixels ? entry : A.pass_pixels - 1u;
    const float* st = A.state + (size_t)entry * 5;
    F.S[0] = st[0]; F.S[1] = st[1]; F.S[2] = st[2]; F.S[3] = st[3]; F.d = st[4];
  }
  for (uint32_t s0 = 0; s0 < per; s0 += (uint32_t)SB) {
    const uint32_t nb = per - s0 < (uint32_t)SB ? per - s0 : (uint32_t)SB;
    const uint32_t run = nb * 5u, stride = run | 1u, total = ne * run;
    // m / run for m < 64 * SB * 5 by multiply-shift, as in k_resolve
    static_assert(64u * SB * 5u * (SB * 5u) <= (1u << 20) && SB <= kMaxLensSamples, "k_adaptive_fold: the multiply-shift's range");
    const uint32_t magic = (1u << 20) / run + 1u;
    if (s0) __syncthreads();  // (the lanes are done with the block before)
    if (nb == per) {  // the whole block at once: word m of LDS run m / run is word m of the block
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
        tile[p * stride + k] = src[((size_t)p * per + s0) * 5 + k];
      }
    }
    __syncthreads();
    if (active) {
      const float* t = tile + lane * stride;
      for (uint32_t k = 0; k < nb; k++) glome::adaptive::take(F, s_first + s0 + k, h, t + k * 5u);
    }
  }
  const bool stop = active && (A.last != 0 || glome::adaptive::agrees(F, h, A.threshold));
  const bool more = active && !stop;
  if (stop) {
    float px[5];
    glome::adaptive::result(F, level, px);
    const size_t o = (size_t)A.first_pixel + entry;
    if (A.rgbad) {
      float* out = A.rgbad + o * 5;
      out[0] = px[0]; out[1] = px[1]; out[2] = px[2]; out[3] = px[3]; out[4] = px[4];
    }
    if (A.packed) A.packed[o] = rgbf(px[0] * px[3], px[1] * px[3], px[2] * px[3]);  // k_resolve's word
    if (A.counts) A.counts[o] = (uint8_t)level;
  }
  const unsigned long long m = __ballot(more);
  if (m == 0ull) return;  // (wave-uniform)
  uint32_t at = 0;
  if (lane == (uint32_t)__ffsll((long long)m) - 1u) at = atomicAdd(A.counter, (uint32_t)__popcll(m));
  at = (uint32_t)__shfl((int)at, __ffsll((long long)m) - 1, 64);
  if (more) {
    float* st = A.state + (size_t)entry * 5;
    st[0] = F.S[0]; st[1] = F.S[1]; st[2] = F.S[2]; st[3] = F.S[3]; st[4] = F.d;
    const uint32_t slot = at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (slot < A.pass_pixels) A.list_out[slot] = entry;
  }
}
