// cull_kernels.hpp -- the cull pass of a flagship render launch (k_render_flat<..., CLS_BIH_TRI, GLOME_FLAG_LB, true>): one light kernel
// on the launch's stream, in front of the render kernel.
//
// Almost half of the flagship frame's work items hold only rays that miss the root box of the terrain.  Such an item used to take a
// ticket, make its rays, fail bih_tri_wave's entry test and store 64 blank pixels: ~500 instructions and, above all, a turn at a queue
// head.  The cull pass visits every (frame, item) of the launch once -- one block per chunk of kQueueChunk positions of the launch's
// order, a wave per item -- makes the item's rays as the render loop makes them (item table, coordinate tables, the frame's camera,
// primary_ray) and asks, for every root entry, what bih_tri_wave asks before it walks (bih_root_interval / bih_clip_root_at_origin / bih_root_enters: the same
// inline functions, not a restatement).  An item none of whose lanes enters any root is dead: its pixels are stored here, through the
// render loop's own store (store_pixel), and it never reaches the queue.  The live items become the slot's ticket list, in the launch's
// order: every block leaves its chunk's 64-bit live mask in device memory, and the last block to finish scans the masks and writes the
// list and its length (deterministic: no atomic append).  The render kernel's queue then runs over list positions (TicketQueue::
// take_direct).  No margins, no projected boxes: the decision is the walk's own, so the frame is bit-identical.
//
// Included by runtime.hip only (a light kernel of the host runtime).
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_launch.hpp"
#include "rt_device.hpp"
#include "tiles.hpp"

constexpr int kCullThreads = 1024;                                // 16 waves: kQueueChunk / 16 = 4 items of the chunk per wave
constexpr int kCullWaves = kCullThreads / 64, kCullPerWave = (int)kQueueChunk / kCullWaves;
static_assert(kCullWaves * kCullPerWave == (int)kQueueChunk && kQueueChunk == 64, "a chunk's live mask is one 64-bit word, a lane per position");

// Position w of the launch's item order -> frame and item of the frame's plan; false: padding.  The order is render_loop's (render_kernels.hpp),
// which keeps its own decode for the instances without a cull pass: chunk by chunk through the frames when chunks_per_frame != 0, else
// frame after frame.
__device__ __forceinline__ bool queue_position(const DRenderArgs& A, uint32_t w, uint32_t& frame, uint32_t& item) {
  if (A.chunks_per_frame) {
    const uint32_t g = w / kQueueChunk, nf = (uint32_t)A.nframes;
    if (g >= A.chunks_per_frame * nf) return false;  // padding of the last round of chunks
    const uint32_t q = g / nf;
    frame = g - q * nf;
    w = q * kQueueChunk + (w % kQueueChunk);
    if (w >= A.total_waves) return false;            // padding of a frame's last chunk
  } else {
    if (w >= A.total_waves * (uint32_t)A.nframes) return false;  // padding of the last round of chunks
    frame = w / A.total_waves;
    w -= frame * A.total_waves;
  }
  item = w;
  return true;
}

// Does any ray of the wave enter any root entry?  closest_flat<..., CLS_BIH_TRI, WAVE>'s loop over the entries, down to the test
// bih_tri_wave begins with.  d = kInf is the primary ray's tmax for EVERY entry of a dead item: an entry's d is only ever clipped to an
// earlier entry's hit, and a dead item has none.  Wave-uniform answer; every lane calls.
__device__ __forceinline__ bool item_live(const DScene& S, const Ray& r, bool valid) {
  for (uint32_t e = 0; e < S.n_entries; e++) {
    U4 ent = ldu4(S.entries, e);
    ent.x = uni(ent.x); ent.z = uni(ent.z);
    if (ent.z & RF_NOVIS) continue;
    U4 rec = ldu4(S.recs, ent.x);
    rec.x = uni(rec.x); rec.y = uni(rec.y);
    if ((rec.x & RF_KINDMASK) != R_BIH) return true;  // (no such entry in a scene of class CLS_BIH_TRI; live is always right)
    const F4 h0 = ld4u(S.bihhdr, 3 * rec.y), h1 = ld4u(S.bihhdr, 3 * rec.y + 1);
    if (uni(as_u(h0.w)) & BREF_LEAF) return true;     // a root that is a single leaf is tested regardless of its interval (Bih.hs:339)
    float nearv, farv;
    bih_root_interval(r, h0, h1, kInf, nearv, farv);
    bih_clip_root_at_origin(nearv);  // as the launch's walk does (never a faithful or counting instance): bounds that only the line behind the camera crosses are missed
    if (wave_ballot(bih_root_enters(valid, nearv, farv)) != 0) return true;
  }
  return false;
}

// masks: two words per chunk (written and read at agent scope: the blocks run on every XCD); list: room for every item of the launch.
__global__ void __launch_bounds__(kCullThreads) k_cull_items(DRenderArgs, uint32_t* list, uint32_t* masks, uint32_t nchunks) {
  const DRenderArgs& A = kernel_args<DRenderArgs>();
  __shared__ uint32_t s_bits[2], s_last, s_wave[kCullWaves], s_lo[kCullThreads], s_hi[kCullThreads], s_off[kCullThreads];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, g = blockIdx.x;
  if (tid < 2) s_bits[tid] = 0;
  __syncthreads();
  uint32_t dead_px = 0;  // wave-uniform
  for (uint32_t k = 0; k < (uint32_t)kCullPerWave; k++) {
    const uint32_t j = wave * kCullPerWave + k;  // the position inside the chunk
    uint32_t frame, item;
    if (!queue_position(A, g * kQueueChunk + j, frame, item)) continue;
    const DItem it = ld_item_u(A.items, item);
    int px = 0, py = 0;
    size_t dense_off = 0;
    const bool valid = item_pixel(it, A.tiles, (int)lane, px, py, dense_off);
    const float xc = ldf(A.xc_tab, valid ? (uint32_t)px : 0u), yc = ldf(A.yc_tab, valid ? (uint32_t)py : 0u);
    const Ray ray = primary_ray(frame == 0 ? A.cam : A.more_cams[frame - 1], xc, yc);
    if (item_live(A.S, ray, valid)) {
      if (lane == 0) atomicOr(&s_bits[j >> 5], 1u << (j & 31u));
    } else {
      dead_px += (uint32_t)__builtin_popcountll(wave_ballot(valid));
      // mmissshade's transparent pixel, ridepth = infinity.  (The depth is handed over as a value the compiler cannot fold: the fog's
      // quotient is then the division the render loop makes at run time, not a constant rounded at compile time.)
      float depth = kInf;
      asm volatile("" : "+v"(depth));
      if (valid) store_pixel(A, frame, px, py, dense_off, ca(0, 0, 0, 0), depth);
    }
  }
  if (A.want_counters && dead_px && lane == 0) atomicAdd(&A.counters->rays_primary, (unsigned long long)dead_px);
  __syncthreads();
  if (tid == 0) {
    __hip_atomic_store(&masks[2 * g], s_bits[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&masks[2 * g + 1], s_bits[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the mask is in memory before the block counts as done (cdna_hip_programming.md, Guideline 16)
    s_last = atomicAdd(&A.counters->cull_done, 1u) == nchunks - 1u ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;

  // ---- the last block: an exclusive scan over the chunks' live counts, kCullThreads chunks at a time, and the list
  uint32_t running = 0;  // live items of the chunks before `base`
  for (uint32_t base = 0; base < nchunks; base += kCullThreads) {
    const uint32_t c = base + tid;
    uint32_t lo = 0, hi = 0;
    if (c < nchunks) {
      lo = __hip_atomic_load(&masks[2 * c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      hi = __hip_atomic_load(&masks[2 * c + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t cnt = (uint32_t)__builtin_popcount(lo) + (uint32_t)__builtin_popcount(hi);
    uint32_t incl = cnt;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += v; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < (uint32_t)kCullWaves; w++) { const uint32_t v = s_wave[w]; total += v; if (w < wave) before += v; }
    s_lo[tid] = lo; s_hi[tid] = hi; s_off[tid] = running + before + incl - cnt;
    __syncthreads();
    for (uint32_t k = 0; k < 64; k++) {  // wave `wave` writes the entries of chunks base + wave * 64 + k, a lane per position
      const uint32_t i = wave * 64 + k, ck = base + i;
      if (ck >= nchunks) break;
      const unsigned long long m = (unsigned long long)s_lo[i] | ((unsigned long long)s_hi[i] << 32);
      if (m == 0) continue;
      if ((m >> lane) & 1ull) {
        uint32_t frame = 0, item = 0;
        (void)queue_position(A, ck * kQueueChunk + lane, frame, item);  // (a live position is no padding)
        list[s_off[i] + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (frame << kListFrameShift) | item;
      }
    }
    running += total;
    __syncthreads();  // (s_wave, s_lo, s_hi and s_off are rewritten by the next round)
  }
  if (tid == 0) {
    __hip_atomic_store(&A.counters->list_len, running, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&A.counters->cull_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the next launch on the slot needs no reset
  }
}
