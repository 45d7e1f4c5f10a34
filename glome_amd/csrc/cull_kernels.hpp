// cull_kernels.hpp -- the cull pass of a flagship render launch (k_render_flat<..., CLS_BIH_TRI, GLOME_FLAG_LB, true>): one light kernel
// on the launch's stream, in front of the render kernel.
//
// Almost half of the flagship frame's work items hold only rays that miss the root box of the terrain.  Such an item used to take a
// ticket, make its rays, fail bih_tri_wave's entry test and store 64 blank pixels: ~500 instructions and, above all, a turn at a queue
// head.  The cull pass visits every (frame, item) of the launch once -- one block per chunk of kQueueChunk positions of the launch's
// order -- makes the item's rays as the render loop makes them (item table, coordinate tables, the frame's camera, primary_ray) and
// asks, for every root entry, what bih_tri_wave asks before it walks (bih_root_interval / bih_clip_root_at_origin / bih_root_enters: the
// same inline functions, not a restatement).  An item none of whose lanes enters any root is dead: its pixels are stored here, through
// the render loop's own store (store_pixel), and it never reaches the queue.
//
// "Live" needs one ray that enters, "dead" needs all 64 to miss, and calling an item live is always safe (the render kernel makes the
// walk's entry test again).  So a block works in two phases.  The PROBE: one wave, a lane per position of the chunk, makes ONE ray of
// each item -- the item's own ray of lane kCullProbeLane -- and a ballot of lane_enters over them is the chunk's mask of items proven
// live, at a 64th of the price of the full test per item.  The FULL test -- a wave per item, a lane per ray, as the render loop holds
// the item -- then runs only for the positions that are no padding and not proven: the dead items, and the items on the silhouette
// whose probe ray misses.  The probe ray is one of the rays of the full test (same pixel, same tables, same camera, same inline
// functions), so the probe proves live only what the full test finds live, and the list is the one a full test of every item gives.
//
// The live items become the slot's ticket list, in the launch's order: every block leaves its chunk's 64-bit live mask in device
// memory, and the last block to finish scans the masks and writes the list and its length (deterministic: no atomic append; the render
// kernel waits for that one block, so its loop over the chunks holds masks and offsets in registers and waits for nothing).  The
// render kernel's queue then runs over list positions (TicketQueue::take_direct).  No margins, no projected boxes: the decision is the
// walk's own, so the frame is bit-identical.
//
// Included by runtime.hip only (a light kernel of the host runtime).
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_launch.hpp"
#include "rt_device.hpp"
#include "tiles.hpp"

// The block: eight waves, chosen by measurement among 256, 512 and 1,024 threads (DESIGN.md 4.1c has the three shapes' figures).  The
// kernel and the last block's scan derive everything from this one number.
constexpr int kCullThreads = 512;
constexpr int kCullWaves = kCullThreads / 64;
constexpr int kCullProbeLane = 36;  // the pixel at (4, 4) of an 8 x 8 block; lane 0 where a leftover strip ends before it
// the last block's scan takes kScanChunks chunks per round whatever the block: kScanPerThread consecutive chunks per thread
constexpr int kScanChunks = 1024, kScanPerThread = kScanChunks / kCullThreads, kScanPerWave = kScanChunks / kCullWaves;
static_assert(kCullThreads % 64 == 0 && kScanPerThread * kCullThreads == kScanChunks && kQueueChunk == 64, "a chunk's live mask is one 64-bit word, a lane per position");

// Chunk g of the launch's item order -> its frame and the first item of the frame's plan in it.  The order is render_loop's
// (render_kernels.hpp), which keeps its own decode for the instances without a cull pass: chunk by chunk through the frames when
// chunks_per_frame != 0.  A chunk lies in ONE frame: a flagship launch of several frames always has chunks_per_frame != 0 (render_impl
// sets it for every renderTile launch with nframes > 1 and checks it before this kernel), and a launch of one frame is frame 0.
// Position j of the chunk is item first + j; positions from total_waves - first on are the padding of the frame's last chunk.
__device__ __forceinline__ void chunk_position(const DRenderArgs& A, uint32_t g, uint32_t& frame, uint32_t& first) {
  frame = 0;
  if (A.chunks_per_frame) {
    const uint32_t nf = (uint32_t)A.nframes, q = g / nf;
    frame = g - q * nf;
    g = q;
  }
  first = g * kQueueChunk;
}

// an entry of the item table at a per-lane index (the probe; the full test's is wave-uniform: ld_item_u)
__device__ __forceinline__ DItem ld_item(const DItem* p, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return as_global(p)[i];
#else
  return p[i];
#endif
}

// Does this lane's ray enter any root entry?  closest_flat<..., CLS_BIH_TRI, WAVE>'s loop over the entries, down to the test
// bih_tri_wave begins with.  d = kInf is the primary ray's tmax for EVERY entry of a dead item: an entry's d is only ever clipped to an
// earlier entry's hit, and a dead item has none.  The entries are the scene's, the same for every lane, whatever the lanes' rays are:
// 64 rays of one item (item_live) or one ray each of 64 items (the probe).  Two answers are wave-uniform and given to every lane.
__device__ __forceinline__ bool lane_enters(const DScene& S, const Ray& r, bool valid) {
  bool in = false;
  for (uint32_t e = 0; e < S.n_entries; e++) {
    // the entry as the launch's walk reads it: the same record of the walk-entry table, the same words of it (closest_flat, TABLE) -- an
    // entry of a flagship launch's scene is a triangle bih (commit_rules)
    const U4 w = ld_walk_u(S.walk, e);
    if (w.x & RF_NOVIS) continue;
    const F4 h0 = ld4u(S.bihhdr, 3 * w.y), h1 = ld4u(S.bihhdr, 3 * w.y + 1);
    if (uni(as_u(h0.w)) & BREF_LEAF) return true;     // a root that is a single leaf is tested regardless of its interval (Bih.hs:339)
    float nearv, farv;
    bih_root_interval(r, h0, h1, kInf, nearv, farv);
    bih_clip_root_at_origin(nearv);  // as the launch's walk does (never a faithful or counting instance): bounds that only the line behind the camera crosses are missed
    in = in || bih_root_enters(valid, nearv, farv);
  }
  return in;
}
// ... and does any ray of the wave?  Wave-uniform answer; every lane calls.
__device__ __forceinline__ bool item_live(const DScene& S, const Ray& r, bool valid) { return wave_ballot(lane_enters(S, r, valid)) != 0; }

// masks: two words per chunk (written and read at agent scope: the blocks run on every XCD); list: room for every item of the launch.
__global__ void __launch_bounds__(kCullThreads) k_cull_items(DRenderArgs, uint32_t* list, uint32_t* masks, uint32_t nchunks) {
  const DRenderArgs& A = kernel_args<DRenderArgs>();
  __shared__ uint32_t s_bits[2], s_todo[2], s_last, s_wave[kCullWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6), g = blockIdx.x;
  uint32_t frame, first;
  chunk_position(A, g, frame, first);                                          // block constants: no division per item
  const uint32_t npos = min((uint32_t)kQueueChunk, A.total_waves - first);     // positions of the chunk that hold an item (>= 1)
  const DCamera cam = frame == 0 ? A.cam : A.more_cams[frame - 1];             // the chunk's frame's, read once

  // ---- the probe: lane j of the first wave stands for position j
  if (wave == 0) {
    const bool pos = lane < npos;
    const DItem it = ld_item(A.items, first + (pos ? lane : 0u));
    int px = 0, py = 0;
    size_t dense_off = 0;
    // (lane 0 of an item always holds a pixel: a strip's items are as many as its pixels need)
    if (!item_pixel(it, A.tiles, kCullProbeLane, px, py, dense_off)) (void)item_pixel(it, A.tiles, 0, px, py, dense_off);
    const Ray ray = primary_ray(cam, ldf(A.xc_tab, (uint32_t)px), ldf(A.yc_tab, (uint32_t)py));
    const LaneMask proven = wave_ballot(pos && lane_enters(A.S, ray, pos));
    const LaneMask todo = wave_ballot(pos) & ~proven;                          // padding is neither proven nor tested
    if (lane == 0) {
      s_bits[0] = (uint32_t)proven; s_bits[1] = (uint32_t)(proven >> 32);
      s_todo[0] = (uint32_t)todo; s_todo[1] = (uint32_t)(todo >> 32);
    }
  }
  __syncthreads();

  // ---- the full test of what the probe left: the k-th position of `todo` goes to wave k mod kCullWaves, so an all-sky chunk's 64
  // tests and a silhouette chunk's few are shared out evenly
  const LaneMask todo = (LaneMask)uni(s_todo[0]) | ((LaneMask)uni(s_todo[1]) << 32);
  LaneMask mine = wave_ballot(((todo >> lane) & 1ull) != 0 && (uint32_t)__builtin_popcountll(todo & ((1ull << lane) - 1ull)) % (uint32_t)kCullWaves == wave);
  LaneMask found = 0;    // wave-uniform, as mine
  uint32_t dead_px = 0;  // wave-uniform
  for (; mine; mine &= mine - 1ull) {
    const uint32_t j = (uint32_t)__builtin_ctzll(mine);  // the position inside the chunk
    const DItem it = ld_item_u(A.items, first + j);
    int px = 0, py = 0;
    size_t dense_off = 0;
    const bool valid = item_pixel(it, A.tiles, (int)lane, px, py, dense_off);
    const float xc = ldf(A.xc_tab, valid ? (uint32_t)px : 0u), yc = ldf(A.yc_tab, valid ? (uint32_t)py : 0u);
    const Ray ray = primary_ray(cam, xc, yc);
    if (item_live(A.S, ray, valid)) {
      found |= 1ull << j;
    } else {
      dead_px += (uint32_t)__builtin_popcountll(wave_ballot(valid));
      // mmissshade's transparent pixel, ridepth = infinity.  (The depth is handed over as a value the compiler cannot fold: the fog's
      // quotient is then the division the render loop makes at run time, not a constant rounded at compile time.)
      float depth = kInf;
      asm volatile("" : "+v"(depth));
      if (valid) store_pixel(A, frame, px, py, dense_off, ca(0, 0, 0, 0), depth);
    }
  }
  if (found && lane == 0) {  // the chunk's live mask: proven or found live
    if ((uint32_t)found) atomicOr(&s_bits[0], (uint32_t)found);
    if ((uint32_t)(found >> 32)) atomicOr(&s_bits[1], (uint32_t)(found >> 32));
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

  // ---- the last block: an exclusive scan over the chunks' live counts, kScanChunks chunks at a time (thread t: the kScanPerThread
  // chunks from base + t * kScanPerThread on), and the list
  uint32_t running = 0;  // live items of the chunks before `base`
  for (uint32_t base = 0; base < nchunks; base += (uint32_t)kScanChunks) {
    uint32_t lo[kScanPerThread], hi[kScanPerThread], cnt = 0;  // cnt: live items of this thread's chunks
#pragma unroll
    for (int p = 0; p < kScanPerThread; p++) {
      const uint32_t c = base + tid * (uint32_t)kScanPerThread + (uint32_t)p;
      lo[p] = 0; hi[p] = 0;
      if (c < nchunks) {
        lo[p] = __hip_atomic_load(&masks[2 * c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        hi[p] = __hip_atomic_load(&masks[2 * c + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      cnt += (uint32_t)__builtin_popcount(lo[p]) + (uint32_t)__builtin_popcount(hi[p]);
    }
    uint32_t incl = cnt;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += v; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < (uint32_t)kCullWaves; w++) { const uint32_t v = s_wave[w]; total += v; if (w < wave) before += v; }
    uint32_t off[kScanPerThread];  // where the entries of this thread's chunks begin
    off[0] = running + before + incl - cnt;
#pragma unroll
    for (int p = 1; p < kScanPerThread; p++) off[p] = off[p - 1] + (uint32_t)__builtin_popcount(lo[p - 1]) + (uint32_t)__builtin_popcount(hi[p - 1]);
    // The wave writes the entries of its threads' chunks, base + wave * kScanPerWave onwards in order, a lane per position.  A chunk's
    // mask and offset come from the registers of the thread that holds them (v_readlane at a wave-uniform lane: no trip through the
    // LDS, and nothing to wait for between two chunks), and its frame and first item follow from the chunk's before by a step.
    uint32_t ck = base + wave * (uint32_t)kScanPerWave, cframe = 0, cfirst = 0;
    if (ck < nchunks) chunk_position(A, ck, cframe, cfirst);
    cframe = uni(cframe); cfirst = uni(cfirst);
    for (uint32_t l = 0; l < 64u && ck < nchunks; l++) {
#pragma unroll
      for (int p = 0; p < kScanPerThread; p++, ck++) {  // (the masks past the launch's last chunk are zero)
        const unsigned long long m = (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)lo[p], (int)l) | ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)hi[p], (int)l) << 32);
        if (m != 0) {
          const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)off[p], (int)l);
          if ((m >> lane) & 1ull) list[o + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (cframe << kListFrameShift) | (cfirst + lane);
        }
        if (A.chunks_per_frame && ++cframe != (uint32_t)A.nframes) continue;  // the next chunk: the same chunk of the next frame,
        cframe = 0; cfirst += kQueueChunk;                                     // or the next chunk of the first
      }
    }
    running += total;
    __syncthreads();  // (s_wave is rewritten by the next round)
  }
  if (tid == 0) {
    __hip_atomic_store(&A.counters->list_len, running, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&A.counters->cull_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the next launch on the slot needs no reset
  }
}
