// render_kernels.hpp -- the device code of every render, sampler and ray-batch kernel for gfx950: tiers, the work queue, the render
// loop, the adaptive sampler and the batch seams.  Templates only (an instance exists where kernel_parts.hip launches it); the
// non-template generic batch kernels are defined in kernel_parts.hip, the light kernels of the host runtime in runtime.hip.
//
// Kernel catalogue
//   k_render_flat<FAITHFUL,COUNT,FULL,CLS,LB,TWO_ROWS>
//                                       persistent: one wave pulls 64-pixel work items (8x8 blocks of a 65x65
//                                       reference tile, Glome.hs:371-386; up to 32 frames per launch) from a ticket
//                                       queue of eight heads; the wave walks a triangle / sphere BIH once for its 64 rays
//                                       (packet: rt_device.hpp bih_tri_wave; for triangles the hand-written walk of
//                                       bih_packet_asm.hpp) -> shadow rays -> shade; secondary rays re-enter the same walk
//                                       through the shading state machine (shade_vm).  No ray streams in HBM at all.
//   k_render_generic                    same loop over the generic interpreter (rt_generic.hpp: rayint / shadow / inside / get_metainfo of any
//                                       nesting of composites as one loop over explicit frames)
//   k_ss_frame_flat / k_ss_frame_generic  the adaptive sampler (renderTileSubsample, Glome.hs:226-323): five passes per
//                                       tile, one launch per frame or batch of frames
//   k_rayint_batch / k_shadow_batch / k_inside_batch   the `Solid` method seams on SoA ray streams (the generic tier's: kernel_parts.hip)
//   (runtime.hip: k_tiles_pack / k_tiles_blit / k_tiles_blit_packed, Tile payload <-> frame; bih_build_device.hpp: k_bb_* / k_mb_*, the tree builders;
//   cull_kernels.hpp: k_cull_items, the cull pass in front of the flagship instance of k_render_flat, which leaves that launch's ticket list)
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_launch.hpp"
#include "rt_device.hpp"
#include "rt_generic.hpp"

// ------------------------------------------------------------------------------------------------ tiers
// FAITHFUL = the reference's exact node-visit order (no ordered early-out, Bih.hs:332-368); COUNT = node / primitive
// work counters.  They back the `faithful` / `count_work` render params (byte-model measurement, parity tests).
// The production variant traverses with early-out and counts rays only.
template <bool FAITHFUL, bool COUNT_, bool FULL_, int CLS = CLS_ALL, bool SURFACE_ONLY_ = false, bool TABLE_ = false>
struct FlatTier {
  static constexpr bool FULL = FULL_;  // false: lean kernel (no secondary rays, no Blend / Layers)
  // every material of the scene is a Surface: the two-row kernels, whose admission rule (instances.hpp use_two_rows over capi_shared.hpp
  // commit_rules) refuses a scene with any other kind -- shading then reads no material kind and has no per-lane light list (rt_device.hpp
  // trace_primary, postshade_lean)
  static constexpr bool SURFACE_ONLY = SURFACE_ONLY_;
  static_assert(!SURFACE_ONLY_ || !FULL_, "a full kernel shades every material kind");
  // ... and every root entry is a triangle bih (commit_rules), so the wave-wide entry loops of such a kernel may read the walk-entry table
  // (rt_device.hpp closest_flat, TABLE).  The flagship render instance does, as does the cull pass in front of it (cull_kernels.hpp
  // lane_enters).  The two-row samplers do not: they spill already, the table's reads moved their spills, and the five-wave instance lost
  // 4.8 % on the million-triangle scene (0.968 -> 1.015 ms per frame) where the four-wave one gained nothing.
  static constexpr bool TABLE = TABLE_;
  static_assert(!TABLE_ || SURFACE_ONLY_, "the walk-entry table serves kernels whose every root entry is a triangle bih");
  static_assert(!SURFACE_ONLY_ || CLS == CLS_BIH_TRI, "the two-row kernels are instances of the triangle class");
  static constexpr bool COUNT = COUNT_;  // (rt_device.hpp tier_counts: a counting tier counts every ray per lane and keeps the primary ray's snapshot)
  static constexpr bool WARP = false;  // scenes with a Warp material (traces over other roots, Shader.hs:157-175) render on the generic tier
  const DScene& S;
  const DLight* lights;
  int nlights;
  LaneStack stk;
  Cnt cnt;
  unsigned int err = 0;  // a CSG item ran into the advance / frame cap (kernels with CLS_CSG)
  PrimarySnap<COUNT_> snap = {};
  // the same tier over another copy of the launch's arguments (render_loop: the kernarg segment, re-read per work item), and back
  __device__ __forceinline__ FlatTier rebound(const DRenderArgs& A) const { return FlatTier{A.S, A.lights, A.nlights, stk, cnt, err}; }
  __device__ __forceinline__ void absorb(const FlatTier& t) { cnt = t.cnt; err = t.err; }
  __device__ __forceinline__ HitG closest(const Ray& r, float tmax) {
    HitG ch;
    Cand c = closest_flat<FAITHFUL, COUNT, CLS>(S, r, tmax, stk, cnt, true, &ch, &err);
    return finalize_flat<CLS>(S, r, c, &ch);
  }
  __device__ __forceinline__ bool occluded(const Ray& r, float d, uint32_t = 0) { return occluded_flat<COUNT, CLS>(S, r, d, stk, cnt, true, &err); }
  // wave-wide calls (every lane of the wave makes them together; `valid` = the lane holds a ray): triangle and sphere
  // BIHs are walked as packets, by primary, shadow and secondary rays alike
  static constexpr bool PACKETS = (CLS & (CLS_BIH_TRI | CLS_BIH_SPHERE | CLS_MESH)) != 0;
  __device__ __forceinline__ HitG closest_wave(const Ray& r, float tmax, bool valid, uint32_t = 0) {
    if constexpr (PACKETS) {
      HitG ch;
      Cand c = closest_flat<FAITHFUL, COUNT, CLS, true, TABLE>(S, r, tmax, stk, cnt, valid, &ch, &err);
      return valid ? finalize_flat<CLS>(S, r, c, &ch) : hit_miss();
    } else {
      return valid ? closest(r, tmax) : hit_miss();
    }
  }
  __device__ __forceinline__ bool occluded_wave(const Ray& r, float d, bool valid) {
    if constexpr (PACKETS) return occluded_flat<COUNT, CLS, true, TABLE>(S, r, d, stk, cnt, valid, &err);
    else return valid && occluded(r, d);
  }
};
// PKMIN: lanes that must wait before the packet service walks (rt_generic.hpp vm_run).  COUNT: bih_nodes / prim_tests are counted -- asked for by
// glome_render_params.count_work; the instances that do not count are 4 % (renderTile) and 2 % (sampler) faster on GlomeView's default scene
// (profiles/r04_probes/generic_tier_no_count_ab.txt), like the flat tier's lean instances.
template <int PKMIN = kPkMinLanes, bool COUNT_ = true>
struct GenericTierT {
  static constexpr bool FULL = true;
  static constexpr bool COUNT = COUNT_;
  static constexpr bool WARP = true;
  // What the out-of-line interpreter calls take the address of -- counters, error flag, frame memory -- are locals of the kernel,
  // referred to from here, and S refers to the kernel-argument segment itself (kernel_args): this struct then never needs an
  // address, lives in registers, and a pool's base is one scalar load from the argument segment.  (With the members inside the
  // struct and S a reference to the by-value argument, both were kept in scratch: every pool access began with a per-lane flat load
  // of the pool's base pointer from the scratch copy of DScene -- two dependent round trips per primitive test.)
  const DScene& S;
  const DLight* lights;
  int nlights;
  Cnt& cnt;
  unsigned int& err;
  uint32_t* vm;  // the interpreter's frames: one word stack of kVmWords per lane for the whole kernel (scratch)
  LaneStack pk;  // the wave's LDS stack for packet walks of sphere BIHs inside the interpreter (cap 0: the scene has none)
  PrimarySnap<COUNT_> snap = {};
  __device__ __forceinline__ GenericTierT rebound(const DRenderArgs&) const { return *this; }  // (already reads the kernarg segment: kernel_args<>())
  __device__ __forceinline__ void absorb(const GenericTierT&) {}
  // `root`: the record the trace runs over -- the scene's, or the frame / scene of a Warp material
  __device__ __forceinline__ HitG closest(const Ray& r, float tmax, uint32_t root) { return vm_closest<COUNT, PKMIN>(S, cnt, err, vm, pk.cap > 0 ? &pk : (LaneStack*)nullptr, r, tmax, root); }
  __device__ __forceinline__ bool occluded(const Ray& r, float d, uint32_t root) { return vm_occluded<COUNT, PKMIN>(S, cnt, err, vm, pk.cap > 0 ? &pk : (LaneStack*)nullptr, r, d, root); }
  __device__ __forceinline__ HitG closest(const Ray& r, float tmax) { return closest(r, tmax, S.root_rec); }
  __device__ __forceinline__ bool occluded(const Ray& r, float d) { return occluded(r, d, S.root_rec); }
  __device__ __forceinline__ HitG closest_wave(const Ray& r, float tmax, bool valid, uint32_t root) { return valid ? closest(r, tmax, root) : hit_miss(); }
  __device__ __forceinline__ bool occluded_wave(const Ray& r, float d, bool valid) { return valid && occluded(r, d); }
};
using GenericTier = GenericTierT<>;

// LDS carve per wave: three stack rows of cap * 64 words (reference, near, far -- the per-lane traversal's entries), or
// two (near, far) in kernels that only ever run the hand-written packet walk, which keeps its references in registers
template <bool TWO_ROWS = false>
__device__ __forceinline__ LaneStack lane_stack(uint32_t* lds, int cap, uint32_t* ovf_base, int ovf_cap) {
  const int wave = threadIdx.x >> 6;  // (uniform per wave; the flat kernels run one wave per workgroup)
  LaneStack s;
  s.lds = lds + (size_t)wave * cap * 64 * (TWO_ROWS ? 2 : 3);
  s.cap = cap;
  s.has_ref_row = !TWO_ROWS;
  // overflow: one [entry * 3][64] block per wave slot (blockIdx.x * waves_per_block + wave); the block after the last
  // entry is the dump block
  s.ovf_cap = ovf_cap;
  s.ovfb = ovf_base ? ovf_base + ((size_t)(blockIdx.x * (blockDim.x >> 6) + wave) * (ovf_cap + 1) * 3) * 64 : nullptr;
  return s;
}
// the generic tier's packet stack: three rows in LDS, no overflow columns (a tree deeper than `cap` keeps the per-lane walk)
__device__ __forceinline__ LaneStack generic_packet_stack(uint32_t* lds, int cap) {
  return lane_stack<false>(lds, cap, nullptr, 0);  // (ovfb null: no overflow columns and no dump block -- bih_tri_wave then never takes the hand-written walk)
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned int v) {
  unsigned long long s = v;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  return s;
}
__device__ __forceinline__ void flush_counters(DCounters* c, const Cnt& cnt, unsigned int err) {
  unsigned long long a = wave_sum(cnt.primary) + cnt.w_primary, b = wave_sum(cnt.shadow) + cnt.w_shadow, s = wave_sum(cnt.secondary);
  unsigned long long n = wave_sum(cnt.bih), m = wave_sum(cnt.mesh), p = wave_sum(cnt.prim);
  unsigned long long e = wave_sum(err);
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&c->rays_primary, a);
    if (b) atomicAdd(&c->rays_shadow, b);
    if (s) atomicAdd(&c->rays_secondary, s);
    if (n) atomicAdd(&c->bih_nodes, n);
    if (m) atomicAdd(&c->mesh_nodes, m);
    if (p) atomicAdd(&c->prim_tests, p);
    if (e) atomicOr(&c->error, 1u);
  }
}

// work item w -> tile + 64 pixels (tiles.hpp tile_item_pixel).  The adaptive kernels and the round-3 loop; the lean loop reads the
// plan's item table instead (DItem).
__device__ __forceinline__ bool work_to_pixel(const DRenderArgs& A, uint32_t w, int lane, int& px, int& py, size_t& dense_off) {
  int lo = (int)A.tile_lut[w >> 6];  // the tile of item (w & ~63); w's own is that one or one of the next few
  while (lo + 1 < A.ntiles && A.tiles[lo + 1].wave_base <= w) lo++;
  DTile t = A.tiles[lo];
  return tile_item_pixel(t, w - t.wave_base, lane, px, py, dense_off);
}

// The work queue of a render launch.  One ticket counter cannot feed the GPU: a returning atomic on one word completes
// about every 11 ns (MI355X_MICROARCH.md, "dequeue": ~88 per microsecond), a frame of the flagship scene is 32,400 items
// and the 6,144 resident waves get through ~150 of them per microsecond -- the waves queue up behind the counter.
// (Measured with one counter: a launch running alone took 0.39 ms per frame whatever its grid, four launches on four slots
// -- four counters -- 0.226.)  So the queue has kQueueShards heads, each on a cache line of its own; ticket chunk c
// (kQueueChunk consecutive items: one 64x64 work tile) belongs to head c mod kQueueShards, so the order in which the image
// is worked through stays what it was.  A wave starts at the head of its XCD (blocks are dealt round-robin over the XCDs:
// speed only, never correctness) and moves on when a head runs dry.  Heads found dry are published in a mask word that is
// written a handful of times per launch and therefore cheap to read (a load of a head itself would wait behind the
// atomics queued on its line: measured 4x slower), so a wave rarely pays for more than one failed take.  The last wave to
// leave puts everything back to zero: the next launch on the slot needs no reset packet on the stream.
constexpr uint32_t kNoTicket = 0xffffffffu;
// One ticket per atomic.  (Several per atomic while a head is far from empty -- guided self-scheduling -- was measured in round 3:
// batches of 4 or 8 won 0-7 % pipelined and lost 15-30 % on a launch alone, whose last items then run on too few waves.)
// A ticket the atomic returns is handed out at the top of the loop, from inext / cur: returning it on the spot frees two scalar
// registers for the kernel's lifetime and moves the register allocation of every render kernel (tools/kernel_mix.py; a Mesh
// instance 5 -> 4 waves per SIMD), so only the lean loop does that (take_direct).
struct TicketQueue {
  uint32_t shard, dry;
  uint32_t inext = 0, left = 0, cur = 0;  // a ticket in hand: its queue index, 1 while it is unused, the head it came from (lane 0's)
  __device__ __forceinline__ TicketQueue() : shard(blockIdx.x % kQueueShards), dry(0) {}
  // what both takes share: ticket i of head h -> its place in the launch's item order, and the marking of a head found dry
  static __device__ __forceinline__ uint32_t ticket_item(uint32_t i, uint32_t h) { return ((i / kQueueChunk) * kQueueShards + h) * kQueueChunk + (i % kQueueChunk); }
  __device__ __forceinline__ void mark_dry(const DRenderArgs& A) {
    uint32_t d = 0;
    if (LaneStack::lane() == 0) { atomicOr(&A.counters->dry, 1u << shard); d = __hip_atomic_load(&A.counters->dry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    dry |= (1u << shard) | uni(d);
  }
  // Every lane of the wave makes the call; the state is wave-uniform (scalar registers) and only the atomics themselves are lane 0's.
  // (Until round 3 the whole take ran on lane 0 under a branch: its six state words then lived in vector registers for the kernel's lifetime.)
  __device__ __forceinline__ uint32_t take(const DRenderArgs& A) {
    constexpr uint32_t kAll = (1u << kQueueShards) - 1u;
    for (;;) {
      if (left) {
        left--;
        const uint32_t i = inext++;
        if (i < A.shard_cap) return ticket_item(i, cur);
        left = 0;
      }
      if (dry == kAll) return kNoTicket;
      if (!((dry >> shard) & 1u)) {
        uint32_t i = 0;
        if (LaneStack::lane() == 0) i = atomicAdd(&A.counters->heads[shard * kQueueHeadStride], 1u);
        i = uni(i);
        if (i < A.shard_cap) { inext = i; left = 1; cur = shard; continue; }
        mark_dry(A);
      }
      shard = (shard + 1) % kQueueShards;
    }
  }
  // The flagship loop's take: the ticket the atomic returns is handed out on the spot (inext / left / cur are then dead: two scalar registers
  // fewer through both walks of the flagship instance).  Its queue runs over the positions of the launch's ticket list (cull_kernels.hpp):
  // head h's ticket i is position ticket_item(i, h), which grows with i, so the head is dry from the first position at or past the list's
  // length -- a word of device memory the cull pass wrote, read here, beside the atomic, and dead before the walks.
  __device__ __forceinline__ uint32_t take_direct(const DRenderArgs& A) {
    constexpr uint32_t kAll = (1u << kQueueShards) - 1u;
    for (;;) {
      if (dry == kAll) return kNoTicket;
      if (!((dry >> shard) & 1u)) {
        uint32_t i = 0;
        if (LaneStack::lane() == 0) i = atomicAdd(&A.counters->heads[shard * kQueueHeadStride], 1u);
        i = uni(i);
        const uint32_t t = ticket_item(i, shard);
        if (t < ld_word_u(&A.counters->list_len, 0)) return t;
        mark_dry(A);
      }
      shard = (shard + 1) % kQueueShards;
    }
  }
  __device__ __forceinline__ void leave(const DRenderArgs& A) {  // after the wave's last take (every lane calls; lane 0 acts)
    if (LaneStack::lane() != 0) return;
    if (atomicAdd(&A.counters->done, 1u) == gridDim.x - 1u) {  // every other wave has taken its last ticket
      for (uint32_t h = 0; h < kQueueShards; h++) __hip_atomic_store(&A.counters->heads[h * kQueueHeadStride], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&A.counters->dry, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&A.counters->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
};

// LEAN (the flagship instance: every step the hand-written walk's, six waves per SIMD, 80 vector registers): the three measures of
// DESIGN.md 4.1c that take registers out of the walks' way -- arguments re-read per item through an opaque pointer, the ticket taken as
// a scalar, the pixel made a second time after the trace.  They are worth 8-10 % there and COST the other instances, whose C++ walks
// then re-read table pointers inside their loops: the 1M-triangle Mesh 0.797 -> 0.872 ms with all three, 0.84 with any one of them off
// (profiles/r04_probes/mesh_regress_ab.txt); so the other flat-tier instances keep round 3's loop.
// ITEMS (the flagship instance only): round 5's item path -- the plan's item table, the coordinate tables, the multiplier split, the scalar
// camera and the ticket returned by the atomic.  The interpreter's kernel keeps round 4's lean loop: TS measured 0.2 % slower with the
// item path (2.3633 / 2.3649 against the parent's 2.3585-2.3594 ms, profiles/r05_probes/item_path_ab.txt).
template <bool LEAN, bool ITEMS, class TIER>
__device__ __forceinline__ void render_loop(const DRenderArgs& A_, TIER& Tk) {
  TicketQueue Q;
  // The launch's arguments are read where the dispatch put them (the kernarg segment: scalar loads), through a pointer the compiler
  // cannot see through from one work item to the next: what an item derives from them -- (float)width, the reciprocals of the
  // item -> pixel divisions, the table pointers -- is then made afresh per item (tens of instructions in eleven thousand) instead of
  // being hoisted out of the loop and carried, spilled, through both walks.
  const DRenderArgs __attribute__((address_space(4)))* ap_ = (const DRenderArgs __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  for (;;) {
    if constexpr (LEAN) asm volatile("" : "+s"(ap_));
    const DRenderArgs& A = LEAN ? *(const DRenderArgs*)ap_ : A_;
    TIER T = Tk.rebound(A);
    uint32_t w = kNoTicket;
    if constexpr (ITEMS) w = Q.take_direct(A);  // a SCALAR: the frame, the item and the camera the ticket names are then scalar loads, not a lane's
    else if constexpr (LEAN) w = Q.take(A);
    else { if (LaneStack::lane() == 0) w = Q.take(A); w = __shfl(w, 0, 64); }
    if (w == kNoTicket) break;
    uint32_t frame;  // wave-uniform
    if constexpr (ITEMS) {
      // the ticket is a position of the launch's ticket list: the live items in the launch's order, every entry a frame and an item of
      // its plan -- no padding, no division (the cull pass decoded the position: cull_kernels.hpp queue_position)
      const uint32_t e = ld_word_u(A.list, w);
      frame = e >> kListFrameShift;
      w = e & ((1u << kListFrameShift) - 1u);
    } else if (A.chunks_per_frame) {
      // chunk by chunk through all frames: the same 64x64 work tile of every view one after the other (neighbouring views walk the
      // same part of the tree), and what a launch ends with is the last chunks of ALL its frames, not the whole of its last frame
      const uint32_t g = w / kQueueChunk, nf = (uint32_t)A.nframes;
      if (g >= A.chunks_per_frame * nf) continue;  // padding of the last round of chunks
      const uint32_t q = g / nf;
      frame = g - q * nf;
      w = q * kQueueChunk + (w % kQueueChunk);
      if (w >= A.total_waves) continue;            // padding of a frame's last chunk
    } else {
      if (w >= A.total_waves * (uint32_t)A.nframes) continue;  // padding of the last round of chunks
      frame = w / A.total_waves;
      w -= frame * A.total_waves;
    }
    int px = 0, py = 0;
    size_t dense_off = 0;
    bool valid;
    float xc, yc;
    DItem it{};  // the item's entry of the plan's table, four scalars
    if constexpr (ITEMS) {
      it = ld_item_u(A.items, w);
      valid = item_pixel(it, A.tiles, (int)LaneStack::lane(), px, py, dense_off);  // lanes past the end of a leftover strip idle along
      // get_coordsf's values from the two tables k_coord_tables filled with it (three IEEE divisions per lane per item otherwise)
      xc = ldf(A.xc_tab, valid ? (uint32_t)px : 0u); yc = ldf(A.yc_tab, valid ? (uint32_t)py : 0u);
    } else {
      valid = work_to_pixel(A, w, (int)LaneStack::lane(), px, py, dense_off);
      get_coordsf(A.width, A.height, (float)px, (float)py, xc, yc);
    }
    Ray ray;
    if constexpr (ITEMS) {  // the frame's camera: twelve scalars out of the argument segment
      const uint32_t cam_off = frame == 0 ? (uint32_t)offsetof(DRenderArgs, cam) : (uint32_t)offsetof(DRenderArgs, more_cams) + (frame - 1) * (uint32_t)sizeof(DCamera);
      ray = primary_ray(ld_camera_u(ap_, cam_off), xc, yc);
    }
    else ray = primary_ray(frame == 0 ? A.cam : A.more_cams[frame - 1], xc, yc);
    count_wave(T.cnt.primary, T.cnt.w_primary, valid);
    HitG h;
    CA c = trace_primary(T, ray, kInf, A.maxdepth, valid, &h);  // Trace.trace lights shader sld ray infinity maxdepth (Glome.hs:33)
    Tk.absorb(T);  // (counters and the error flag back into the kernel's tier)
    if (!valid) continue;
    // the pixel once more (rather than three registers carried, spilled, through both walks): from the entry's four scalars, which the
    // compiler must take for new values here, or it would keep the first decode's lanes alive instead
    if constexpr (ITEMS) {
      asm volatile("" : "+s"(it.x), "+s"(it.y), "+s"(it.off), "+s"(it.pitch));
      px = 0; py = 0; dense_off = 0;
      (void)item_pixel(it, A.tiles, (int)LaneStack::lane(), px, py, dense_off);
    } else if constexpr (LEAN) { px = 0; py = 0; dense_off = 0; (void)work_to_pixel(A, w, (int)LaneStack::lane(), px, py, dense_off); }
    store_pixel(A, frame, px, py, dense_off, c, h.hit ? h.t : kInf);  // (ridepth)
  }
  Q.leave(A_);
}

// TWO_ROWS: the wave's LDS holds two stack rows per entry instead of three (lane_stack); legal when no lane ever pushes on
// its own -- a lean kernel of a triangle / sphere class over a scene whose materials are all Surface, where every ray of
// the frame goes through the packet walk.  With LB waves per SIMD asked of the register allocator that is 24 waves per
// CU instead of 16.
template <bool FAITHFUL, bool COUNT, bool FULL, int CLS, int LB = 1, bool TWO_ROWS = false>
__global__ void __launch_bounds__(64, LB) k_render_flat(DRenderArgs A, int stack_cap, uint32_t* ovf, int ovf_cap) {
  extern __shared__ uint32_t lds[];
  FlatTier<FAITHFUL, COUNT, FULL, CLS, TWO_ROWS, TWO_ROWS> T{A.S, A.lights, A.nlights, lane_stack<TWO_ROWS>(lds, stack_cap, ovf, ovf_cap), Cnt()};
  render_loop<TWO_ROWS, TWO_ROWS>(A, T);
  if (A.want_counters) flush_counters(A.counters, T.cnt, T.err);
  else if ((CLS & (CLS_CSG | CLS_MESH)) && __builtin_amdgcn_ballot_w64(T.err != 0) && (threadIdx.x & 63) == 0) atomicOr(&A.counters->error, 1u);
}
template <bool COUNT>
__global__ void __launch_bounds__(64, GLOME_GENERIC_LB) k_render_generic(DRenderArgs) {
  const DRenderArgs& A = kernel_args<DRenderArgs>();
  extern __shared__ uint32_t lds[];
  Cnt cnt; unsigned int err = 0; uint32_t vm[kVmWords];
  GenericTierT<1, COUNT> T{A.S, A.lights, A.nlights, cnt, err, vm, generic_packet_stack(lds, (int)A.S.pk_generic_cap)};  // (<1>: this kernel's packet service never waits)
  // (Tried in round 3 and dropped: refilling a lane with the next pixel as soon as its trace is through, with shade_vm as a
  // resumable object.  The object form alone cost S4 0.39 -> 0.50 ms and this tier 4.3 -> 4.85 ms (its state no longer stays in
  // registers), and with refilling the lanes fall out of step, every closest-hit call then runs for a part of the wave, and the frame took 5.8 ms
  // against 4.3: what keeps the lanes idle -- 28 % of the vector lane slots are used -- is the interpreter's own divergence
  // inside a call, not pixels of unequal cost.)
  render_loop<true, false>(A, T);  // (the interpreter, short of registers like the flagship, measures better with the lean loop: TS 2.70 against 2.74 ms)
  if (A.want_counters) flush_counters(A.counters, T.cnt, T.err);
  else if (__builtin_amdgcn_ballot_w64(T.err != 0) && (threadIdx.x & 63) == 0) atomicOr(&A.counters->error, 1u);
}


// ------------------------------------------------------------------------------------------------ adaptive sampler
// renderTileSubsample (Glome.hs:226-323).  The reference runs five passes over each 65x65 tile; a pass looks at
// neighbour contrast (`decide`, Glome.hs:213-219) and either averages or traces a fresh sample.  Here persistent waves
// pull regions of a tile's candidate lattice (ss_block_pixel: blocks of 64 candidates of a pass in a compact pixel area,
// one per lane; a region = a rectangle of blocks, ss_region_shape); a lane takes the contrast test and writes the average when
// that settles it; the candidates that need a sample are compacted over the region (ballot + LDS ring) and traced 64 at a
// time -- neighbours in the image, so the rays are walked as a packet.  A region in which nobody needs a sample traces nothing.
// The working buffer `v` is a dense per-tile array in global memory (tile order, row major inside a tile), so all
// neighbour reads stay inside the tile like the reference's getc (Glome.hs:233-235); `v2` is the output.  A pass reads
// what the previous passes wrote anywhere in the tile: ss_frame_loop below orders the passes per tile.
// channel planes, not 5-float structs: the lanes of a block read neighbouring pixels, so a plane read is (nearly) contiguous
struct SSBuf { float* v; size_t plane; };
__device__ __forceinline__ void out5_store(float* v, size_t i, const TC& c) { float* p = v + i * 5; p[0] = c.r; p[1] = c.g; p[2] = c.b; p[3] = c.a; p[4] = c.d; }
__device__ __forceinline__ size_t ss_out_index(const DRenderArgs& A, const DTile& t, int dx, int dy) {
  return A.dense ? (size_t)t.pix_base + (size_t)dy * t.w + dx : (size_t)(t.y + dy) * A.width + (t.x + dx);
}
__device__ __forceinline__ void ss_write_out(const DRenderArgs& A, size_t frame_off, const DTile& t, int dx, int dy, const TC& c) {
  size_t o = ss_out_index(A, t, dx, dy) + frame_off;
  if (A.out5) out5_store(A.out5, o, c);
  if (A.packed) A.packed[o] = rgbf(c.r * c.a, c.g * c.a, c.b * c.a);
}

// One launch renders the frame: its work items are (pass, tile, region) in pass-major order, and an item of pass p waits
// for the tile's pass p - 1 (a counter per tile and pass) instead of the whole frame's -- no launch boundary between the
// passes, no tail of a short launch five times per frame, and the tiles that are early go on with their next pass while
// the late ones finish the last.
//   Order and progress: the items are dealt to kSSHeads queue heads by tile (tile mod kSSHeads); each head hands its items
//   out in order, so whatever an item waits for (earlier passes of the SAME tile) was handed out before it, to a wave that
//   is running: the oldest unfinished item of a head never waits.
//   Visibility: the working buffer `v` is written by one wave and read by others, on other CUs and XCDs, inside one
//   launch.  Every store to it is an agent-scope (sc1, write-through) store, every load an agent-scope (sc1) load that
//   bypasses the CU's L1; a wave drains its stores (s_waitcnt vmcnt(0)) before it counts its region as done, and polls the
//   counter with an agent-scope load before its first read (cdna_hip_programming.md, Guideline 16: payload and flag
//   both sc1, producer drained).  The pixels of the frame are write-only.
__device__ __forceinline__ float ss_ld(const float* p) { return as_f(__hip_atomic_load((const unsigned int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
__device__ __forceinline__ void ss_st(float* p, float x) { __hip_atomic_store((unsigned int*)p, as_u(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ TC ss_load(const SSBuf& b, size_t i) { const float* p = b.v + i; return tc(ss_ld(p), ss_ld(p + b.plane), ss_ld(p + 2 * b.plane), ss_ld(p + 3 * b.plane), ss_ld(p + 4 * b.plane)); }
__device__ __forceinline__ void ss_store(const SSBuf& b, size_t i, const TC& c) { float* p = b.v + i; ss_st(p, c.r); ss_st(p + b.plane, c.g); ss_st(p + 2 * b.plane, c.b); ss_st(p + 3 * b.plane, c.a); ss_st(p + 4 * b.plane, c.d); }
__device__ __forceinline__ TC ss_getc(const SSBuf& v, const DTile& t, int dx, int dy) {  // getc: outside the tile reads blank
  // (the load is unconditional, from a clamped address, so the twenty loads of a contrast test go out back to back)
  const bool in = dx >= 0 && dx < t.w && dy >= 0 && dy < t.h;
  const TC c = ss_load(v, (size_t)t.pix_base + (in ? (size_t)dy * t.w + dx : (size_t)0));
  return in ? c : tc_blank();
}

template <class TIER>
__device__ __forceinline__ void ss_frame_loop(const DRenderArgs& A, TIER& T) {
  __shared__ uint32_t need_list[256];  // ring of the region's candidates that need a sample: dx | dy << 8 (one wave per block)
  const int lane = threadIdx.x & 63;
  const SSPlan PL = ss_plan(A);
  const uint32_t vtiles = (uint32_t)A.ntiles * (uint32_t)A.nframes;
  uint32_t shard = blockIdx.x % kSSHeads, dry = 0;  // (lane 0's)
  for (;;) {
    // ---- take the next item of a queue head (TicketQueue's scheme, over the frame's own heads)
    uint32_t w = kNoTicket, h = 0;
    if (lane == 0) {
      while (dry != (1u << kSSHeads) - 1u) {
        if (!((dry >> shard) & 1u)) {
          const uint32_t i = atomicAdd(&A.ss_cnt[shard * kSSHeadStride], 1u);
          if (i < PL.first[6]) { w = i; h = shard; break; }
          atomicOr(&A.ss_cnt[kSSHeads * kSSHeadStride], 1u << shard);
          dry |= (1u << shard) | __hip_atomic_load(&A.ss_cnt[kSSHeads * kSSHeadStride], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        shard = (shard + 1) % kSSHeads;
      }
    }
    w = __shfl(w, 0, 64); h = __shfl(h, 0, 64);
    if (w == kNoTicket) break;
    int pass = 1;
    while (w >= PL.first[pass + 1]) pass++;
    const uint32_t j = w - PL.first[pass];
    const uint32_t ti = (j / PL.per_tile[pass]) * kSSHeads + h;  // tile of a frame (ti mod kSSHeads == h): frame-major
    if (ti >= vtiles) continue;                                   // padding of the last round of tiles
    const int r = (int)(j % PL.per_tile[pass]), rx = r % (int)PL.nrx[pass], ry = r / (int)PL.nrx[pass];
    const uint32_t frame = ti / (uint32_t)A.ntiles;
    const DTile t = A.tiles[ti - frame * (uint32_t)A.ntiles];
    const SSBuf v{A.scratch + (size_t)frame * 5 * A.ss_plane, (size_t)A.ss_plane};  // every frame has its own working buffer
    const size_t frame_off = (size_t)frame * A.frame_stride;
    const DCamera& cam = frame == 0 ? A.cam : A.more_cams[frame - 1];
    unsigned int* done = A.ss_done + (size_t)ti * 8;
    if (pass >= 2) {  // the tile's previous pass must be complete (its regions read each other's pixels)
      if (lane == 0) while (__hip_atomic_load(&done[pass - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < PL.per_tile[pass - 1]) __builtin_amdgcn_s_sleep(2);
      __builtin_amdgcn_wave_barrier();
    }
    const float thr = pass >= 2 ? A.thresholds[pass - 2] : 0.0f;
    int ox[4], oy[4];
    ss_neighbours(pass, ox, oy);
    // the region's blocks inside the (possibly clipped) tile (ss_region_blocks, rt_device.hpp)
    int bx0, by0, nbx, nb;
    ss_region_blocks(pass, t.w, t.h, rx, ry, A.ss_rw[pass], A.ss_rh[pass], bx0, by0, nbx, nb);
    // ---- decide block after block; whenever 64 candidates wait for a sample (and at the region's end) they are traced as
    // one packet -- neighbours in the image.  Every pixel of the tile is written by exactly one of the passes 1-4 before a
    // later pass reads it (Glome.hs:241-297), so the blank initial value (:231) is only ever seen outside the tile (getc).
    uint32_t n = 0, hd = 0;  // wave-uniform: candidates listed / traced so far (ring positions)
    int b = 0;
    for (;;) {
      for (; b < nb && n - hd < 64u; b++) {
        const int bx = bx0 + b % nbx, by = by0 + b / nbx;
        int dx, dy;
        ss_block_pixel(pass, bx, by, lane, dx, dy);
        bool need = dx < t.w && dy < t.h;
        if (need && pass >= 2) {
          TC a = ss_getc(v, t, dx + ox[0], dy + oy[0]), bb = ss_getc(v, t, dx + ox[1], dy + oy[1]);
          TC c = ss_getc(v, t, dx + ox[2], dy + oy[2]), d = ss_getc(v, t, dx + ox[3], dy + oy[3]);
          need = gmaxf(ccmp(a, c), ccmp(bb, d)) > thr;  // decide, Glome.hs:215-216
          if (!need) {
            TC avg = cavg4(a, bb, c, d);
            if (pass < 5) ss_store(v, (size_t)t.pix_base + (size_t)dy * t.w + dx, avg);
            else ss_write_out(A, frame_off, t, dx, dy, ss_pass5_blend(avg, a, bb, c, d, dx == t.w - 1, dy == t.h - 1));
          }
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(need);
        if (need) need_list[(n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))) & 255u] = (uint32_t)dx | ((uint32_t)dy << 8);
        n += (uint32_t)__popcll(m);
      }
      if (n == hd) break;  // (b == nb: the region is through)
      __syncthreads();     // one wave per block: makes the list visible across lanes
      const uint32_t cnt = min(64u, n - hd);
      const bool valid = (uint32_t)lane < cnt;
      const uint32_t e = need_list[(hd + (valid ? (uint32_t)lane : 0u)) & 255u];
      hd += cnt;
      const int dx = (int)(e & 255u), dy = (int)(e >> 8);
      const float off = pass == 5 ? 0.5f : 0.0f;  // pass 5 samples between pixels (getCoordsf (x+.5) (y+.5), Glome.hs:307)
      float xc, yc;
      get_coordsf(A.width, A.height, (float)(t.x + dx) + off, (float)(t.y + dy) + off, xc, yc);
      Ray ray = primary_ray(cam, xc, yc);
      if (valid) T.cnt.primary++;
      HitG hh;
      CA col = trace_primary(T, ray, kInf, A.maxdepth, valid, &hh);
      if (valid) {
        TC smp = tc(col.r, col.g, col.b, col.a, hh.hit ? hh.t : kInf);
        if (pass < 5) ss_store(v, (size_t)t.pix_base + (size_t)dy * t.w + dx, smp);
        else {
          TC a = ss_getc(v, t, dx + ox[0], dy + oy[0]), bb = ss_getc(v, t, dx + ox[1], dy + oy[1]);
          TC c = ss_getc(v, t, dx + ox[2], dy + oy[2]), d = ss_getc(v, t, dx + ox[3], dy + oy[3]);
          ss_write_out(A, frame_off, t, dx, dy, ss_pass5_blend(smp, a, bb, c, d, dx == t.w - 1, dy == t.h - 1));
        }
      }
      __syncthreads();  // the entries just read may be overwritten by the blocks that follow
    }
    if (pass < 5) {   // the region's pixels are in memory before it counts as done
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) atomicAdd(&done[pass], 1u);
    }
  }
}
template <bool FULL, int CLS, int LB = 1, bool TWO_ROWS = false, bool FAITHFUL = false>
__global__ void __launch_bounds__(64, LB) k_ss_frame_flat(DRenderArgs A, int stack_cap, uint32_t* ovf, int ovf_cap) {
  extern __shared__ uint32_t lds[];
  FlatTier<FAITHFUL, false, FULL, CLS, TWO_ROWS> T{A.S, A.lights, A.nlights, lane_stack<TWO_ROWS>(lds, stack_cap, ovf, ovf_cap), Cnt()};
  ss_frame_loop(A, T);
  if (A.want_counters) flush_counters(A.counters, T.cnt, T.err);
  else if ((CLS & (CLS_CSG | CLS_MESH)) && __builtin_amdgcn_ballot_w64(T.err != 0) && (threadIdx.x & 63) == 0) atomicOr(&A.counters->error, 1u);
}
template <bool COUNT>
__global__ void __launch_bounds__(64, GLOME_GENERIC_LB) k_ss_frame_generic(DRenderArgs) {
  const DRenderArgs& A = kernel_args<DRenderArgs>();
  extern __shared__ uint32_t lds[];
  Cnt cnt; unsigned int err = 0; uint32_t vm[kVmWords];
  GenericTierT<kPkMinLanes, COUNT> T{A.S, A.lights, A.nlights, cnt, err, vm, generic_packet_stack(lds, (int)A.S.pk_generic_cap)};
  ss_frame_loop(A, T);
  if (A.want_counters) flush_counters(A.counters, T.cnt, T.err);
  else if (__builtin_amdgcn_ballot_w64(T.err != 0) && (threadIdx.x & 63) == 0) atomicOr(&A.counters->error, 1u);
}

// ------------------------------------------------------------------------------------------------ batch seams

__device__ __forceinline__ void store_hit(const HitStream& H, size_t i, const HitG& h, int B) {
  if (H.t) H.t[i] = h.hit ? h.t : -1.0f;
  if (H.prim) H.prim[i] = h.hit ? (int32_t)h.uid : -1;
  if (H.nx) H.nx[i] = h.n.x;
  if (H.ny) H.ny[i] = h.n.y;
  if (H.nz) H.nz[i] = h.n.z;
  if (H.tex8) {
    TexStack ts = h.hit ? h.tex : 0;
    for (int k = 0; k < 8; k++) { H.tex8[8 * i + k] = (int32_t)tex_head(ts, B) - 1; ts = k * B + B < 64 ? ts >> B : 0; }
  }
}
__device__ __forceinline__ Ray load_ray(const RayStream& R, size_t i) {
  Ray r;
  r.o = v3(R.ox[i], R.oy[i], R.oz[i]);
  r.d = v3(R.dx[i], R.dy[i], R.dz[i]);
  return r;
}
template <bool FAITHFUL>
__global__ void __launch_bounds__(64) k_rayint_batch_flat(DScene S, size_t n, RayStream R, HitStream H, int stack_cap, uint32_t* ovf, int ovf_cap, DCounters* c) {
  extern __shared__ uint32_t lds[];
  FlatTier<FAITHFUL, false, false, CLS_EVERY> T{S, nullptr, 0, lane_stack(lds, stack_cap, ovf, ovf_cap), Cnt()};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const Ray r = load_ray(R, i);
    if (FAITHFUL || unit_length(r.d)) { store_hit(H, i, T.closest(r, R.tmax[i]), (int)S.tex_bits); continue; }
    // a caller's ray that is not unit length: the reference's own traversal (rayint_sphere reports hits for such rays that lie
    // outside the sphere's box, so the ordered early-out's pruning is not exact for them)
    HitG ch;
    Cand c = closest_flat<true, false, CLS_EVERY>(S, r, R.tmax[i], T.stk, T.cnt, true, &ch, &T.err);
    store_hit(H, i, finalize_flat<CLS_EVERY>(S, r, c, &ch), (int)S.tex_bits);
  }
  if (T.err) atomicOr(&c->error, 1u);
}
template <int DUMMY = 0>
__global__ void __launch_bounds__(64) k_shadow_batch_flat(DScene S, size_t n, RayStream R, uint8_t* occ, int stack_cap, uint32_t* ovf, int ovf_cap, DCounters* c) {
  extern __shared__ uint32_t lds[];
  FlatTier<false, false, false, CLS_EVERY> T{S, nullptr, 0, lane_stack(lds, stack_cap, ovf, ovf_cap), Cnt()};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    occ[i] = T.occluded(load_ray(R, i), R.tmax[i]) ? 1 : 0;
  if (T.err) atomicOr(&c->error, 1u);
}
