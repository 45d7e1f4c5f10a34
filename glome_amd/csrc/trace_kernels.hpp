// trace_kernels.hpp -- Trace.trace (GlomeTrace/Data/Glome/Trace.hs:59-82) over a caller's SoA ray streams: the device code of the trace
// seam (glome_trace_batch).  Templates only, like render_kernels.hpp; an instance exists where kernel_parts.hip launches it.
//
//   k_trace_batch_flat<FAITHFUL,COUNT,FULL,CLS,LB>   one wave per block; a work item is 64 consecutive rays, one per lane, traced by the
//                                                    render kernels' own trace_primary -- closest hit, shadow and secondary rays walk as a
//                                                    packet where the instance's class has a packet walk
//   k_trace_batch_generic<COUNT>                     the same loop over the generic interpreter
#pragma once
#include "render_kernels.hpp"

// The item loop.  trace_primary is a wave-wide call, so the loop is wave-uniform: every lane of the wave goes through the same items, and a
// lane past the end of the last item makes the call with valid = false -- it loads nothing and stores nothing.
// Items are dealt statically (item = blockIdx.x, += gridDim.x), not by TicketQueue.  The grid is several times the wave slots of the GPU
// (runtime.hip trace_impl), so the dispatcher itself hands blocks to the slots that come free, which balances the launch at the grain of
// a block's few items; a ticket would add an atomic round trip per item, the reset protocol's dependence on the slot's counter block
// between launches, and an item order that means nothing here -- a caller's rays have no image order to keep.
// CHECK: directions are used as given (trace does not normalise); an instance whose traversal is exact for unit rays only refuses the
// others -- the lane sits the item out and the launch reports kErrNonUnit.
template <bool CHECK, class TIER>
__device__ __forceinline__ void trace_batch_loop(const DTraceArgs& A, TIER& T, bool check, unsigned int& bad) {
  const uint32_t lane = LaneStack::lane();
  const uint32_t items = (A.n + 63u) >> 6;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t i = item * 64u + lane;
    bool valid = i < A.n;
    Ray ray;
    ray.o = v3(0, 0, 0); ray.d = v3(0, 0, 1);
    float tmax = kInf;
    if (valid) {  // seven streams, 256 contiguous bytes of each per wave
      ray.o = v3(A.ox[i], A.oy[i], A.oz[i]);
      ray.d = v3(A.dx[i], A.dy[i], A.dz[i]);
      if (A.tmax) tmax = A.tmax[i];
      if (CHECK && check && !unit_length(ray.d)) { bad = 1; valid = false; }
    }
    count_wave(T.cnt.primary, T.cnt.w_primary, valid);
    // a counting instance keeps what this ray's trace adds to the lane's counters (they run on across the items a block takes): the work
    // record.  The primary ray's part is the snapshot trace_primary leaves in the tier's `snap`; a lane it never traces keeps zeros there.
    Cnt c0;
    if constexpr (tier_counts<TIER>::value) { c0 = T.cnt; T.snap.p_bih = c0.bih; T.snap.p_mesh = c0.mesh; T.snap.p_prim = c0.prim; }
    HitG h;
    const CA c = trace_primary(T, ray, tmax, A.maxdepth, valid, &h);
    if (!valid) continue;
    if constexpr (tier_counts<TIER>::value) {
      if (A.work) {  // two 16-byte stores per lane: a wave writes 2 KB contiguously
        const Cnt& c1 = T.cnt;
        uint4* w = reinterpret_cast<uint4*>(A.work + (size_t)i * kWorkWords);
        w[0] = make_uint4(c1.bih - c0.bih, c1.mesh - c0.mesh, c1.prim - c0.prim, c1.shadow - c0.shadow);
        w[1] = make_uint4(c1.secondary - c0.secondary, T.snap.p_bih - c0.bih, T.snap.p_mesh - c0.mesh, T.snap.p_prim - c0.prim);
        if (!A.rgbad) continue;  // (a work launch may leave the colour out; it has no hit streams)
      }
    }
    float* out = A.rgbad + (size_t)i * 5;
    out[0] = c.r; out[1] = c.g; out[2] = c.b; out[3] = c.a; out[4] = h.hit ? h.t : kInf;  // (ridepth: what glome_render stores with fog = 0)
    store_hit(HitStream{A.t, A.prim, A.nx, A.ny, A.nz, A.tex8}, i, h, (int)A.S.tex_bits);
  }
}
// what a trace kernel ends with: the counters when somebody reads them, the error bits always (one atomic per wave that has any)
__device__ __forceinline__ void trace_batch_report(const DTraceArgs& A, const Cnt& cnt, unsigned int err, unsigned int bad) {
  if (A.want_counters) flush_counters(A.counters, cnt, err);
  else if (__builtin_amdgcn_ballot_w64(err != 0) && (threadIdx.x & 63) == 0) atomicOr(&A.counters->error, kErrLimit);
  if (__builtin_amdgcn_ballot_w64(bad != 0) && (threadIdx.x & 63) == 0) atomicOr(&A.counters->error, kErrNonUnit);
}

template <bool FAITHFUL, bool COUNT, bool FULL, int CLS, int LB = 1>
__global__ void __launch_bounds__(64, LB) k_trace_batch_flat(DTraceArgs A, int stack_cap, uint32_t* ovf, int ovf_cap) {
  extern __shared__ uint32_t lds[];
  FlatTier<FAITHFUL, COUNT, FULL, CLS> T{A.S, A.lights, A.nlights, lane_stack(lds, stack_cap, ovf, ovf_cap), Cnt()};
  unsigned int bad = 0;
  trace_batch_loop<!FAITHFUL>(A, T, true, bad);  // (the faithful instance is the reference's own traversal: any direction is legal)
  trace_batch_report(A, T.cnt, T.err, bad);
}
template <bool COUNT>
__global__ void __launch_bounds__(64, GLOME_GENERIC_LB) k_trace_batch_generic(DTraceArgs) {
  const DTraceArgs& A = kernel_args<DTraceArgs>();  // (the kernarg segment itself: see GenericTierT)
  extern __shared__ uint32_t lds[];
  Cnt cnt; unsigned int err = 0, bad = 0; uint32_t vm[kVmWords];
  GenericTierT<1, COUNT> T{A.S, A.lights, A.nlights, cnt, err, vm, generic_packet_stack(lds, (int)A.S.pk_generic_cap)};
  trace_batch_loop<true>(A, T, A.check_unit != 0, bad);  // (one contract on both tiers, though this tier switches its traversal per ray)
  trace_batch_report(A, cnt, err, bad);
}
