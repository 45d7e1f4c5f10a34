// runtime.hip -- the device half of the C ABI (include/glome_hip.h): context, slots, tile and coordinate caches, scene commit / upload,
// the whole-frame render, the per-ray batch seams, tile transport and the multi-GPU driver.  Compiled once.  It launches the render,
// sampler and batch kernels through kernel_launch.hpp (the instances live in kernel_parts.hip, chosen by instances.hpp) and holds
// only the light kernels: the kernel-argument self-test, the coordinate tables, tile transport, the tree builders
// (bih_build_device.hpp), the flagship launch's cull pass (cull_kernels.hpp) and the updates of a committed Mesh (mesh_update_kernels.hpp)
// and of a committed triangle bih (bih_update_kernels.hpp) and sphere bih (sphere_bih_update_kernels.hpp), and of committed Instances'
// matrices and the refit of the bihs above an updated object (item_bih_update_kernels.hpp); what those kernels share is in
// update_common.hpp.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/glome_hip.h"
#include "capi_shared.hpp"
#include "flatten.hpp"
#include "tiles.hpp"
#include "rt_device.hpp"
#include "instances.hpp"
#include "kernel_launch.hpp"
#include "bih_build_device.hpp"
#include "cull_kernels.hpp"
#include "mesh_update_kernels.hpp"
#include "bih_update_kernels.hpp"
#include "item_bih_update_kernels.hpp"
#include "sphere_bih_update_kernels.hpp"
#include "bih_rebuild_kernels.hpp"

using namespace glome;

// ------------------------------------------------------------------------------------------------ light kernels
// what kernel_args assumes, asked of the device: the unnamed first argument read through the kernarg pointer equals the bytes the
// host passed (a second, named copy of them travels as a pointer)
__global__ void k_kernarg_selftest(DRenderArgs, const DRenderArgs* expect, unsigned int* ok) {
  const unsigned char* a = (const unsigned char*)&kernel_args<DRenderArgs>();
  const unsigned char* b = (const unsigned char*)expect;
  unsigned int same = 1;
  for (size_t i = threadIdx.x; i < sizeof(DRenderArgs); i += blockDim.x) same &= a[i] == b[i] ? 1u : 0u;
  if (!same) atomicAnd(ok, 0u);
}
// The lean render loop's pixel coordinates: xc of every column and yc of every row of a width x height frame, made by get_coordsf itself
// (bit-identical by construction; the host would have to reproduce the device's contraction of q * 2 - 1).  xc depends on the column
// only and yc on the row only, so the other coordinate is passed as 0.
__global__ void k_coord_tables(int width, int height, float* xc_tab, float* yc_tab) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  float xc, yc;
  if (i < width) { get_coordsf(width, height, (float)i, 0.0f, xc, yc); xc_tab[i] = xc; }
  if (i < height) { get_coordsf(width, height, 0.0f, (float)i, xc, yc); yc_tab[i] = yc; }
}
// what the tables are checked against (glome_ctx_coord_tables): get_coordsf of whole pixels (i mod width, i mod height), as a render loop calls it
__global__ void k_coords_direct(int width, int height, float* xc_out, float* yc_out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= width && i >= height) return;
  float xc, yc;
  get_coordsf(width, height, (float)(i % width), (float)(i % height), xc, yc);
  if (i < width) xc_out[i] = xc;
  if (i < height) yc_out[i] = yc;
}
// ------------------------------------------------------------------------------------------------ tile transport
__global__ void k_tiles_pack(const DTile* tiles, int ntiles, int width, const float* frame, float* payload) {
  for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
    DTile T = tiles[t];
    int np = T.w * T.h;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < np * 5; i += gridDim.x * blockDim.x) {
      int p = i / 5, k = i - p * 5;
      size_t src = ((size_t)(T.y + p / T.w) * width + (T.x + p % T.w)) * 5 + k;
      payload[(size_t)T.pix_base * 5 + i] = frame[src];
    }
  }
}
__global__ void k_tiles_blit(const DTile* tiles, int ntiles, int width, const float* payload, float* frame, uint32_t* packed) {
  for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
    DTile T = tiles[t];
    int np = T.w * T.h;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < np; p += gridDim.x * blockDim.x) {
      const float* s = payload + ((size_t)T.pix_base + p) * 5;
      size_t o = (size_t)(T.y + p / T.w) * width + (T.x + p % T.w);
      float r = s[0], g = s[1], b = s[2], a = s[3], d = s[4];
      float* dst = frame + o * 5;
      dst[0] = r; dst[1] = g; dst[2] = b; dst[3] = a; dst[4] = d;
      if (packed) packed[o] = rgbf(r * a, g * a, b * a);
    }
  }
}
// blockIdx.z = frame of a group: frame f's payload sits f * payload_frame_stride words into every rank's slab, its
// framebuffer f * out_frame_stride words after the first
__global__ void k_tiles_blit_packed(const DTile* tiles, int ntiles, int width, const uint32_t* payload, uint32_t* packed, size_t payload_frame_stride, size_t out_frame_stride) {
  payload += (size_t)blockIdx.z * payload_frame_stride;
  packed += (size_t)blockIdx.z * out_frame_stride;
  for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
    DTile T = tiles[t];
    int np = T.w * T.h;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < np; p += gridDim.x * blockDim.x)
      packed[(size_t)(T.y + p / T.w) * width + (T.x + p % T.w)] = payload[(size_t)T.pix_base + p];
  }
}

// ================================================================================================ host runtime
static bool launch_render_flat(int key, const FlatLaunch& L, const DRenderArgs& A) {
  return launch_flat_p1(key, L, A) || launch_flat_p2(key, L, A) || launch_flat_p3(key, L, A) || launch_flat_p4(key, L, A);
}
static bool launch_ss_flat(int key, const FlatLaunch& L, const DRenderArgs& A) { return launch_ss_flat_p5(key, L, A) || launch_ss_flat_p9(key, L, A); }
static bool launch_trace_flat(int key, const FlatLaunch& L, const DTraceArgs& A) { return launch_trace_flat_p12(key, L, A) || launch_trace_flat_p13(key, L, A) || launch_trace_flat_p14(key, L, A); }
struct glome_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  // event pool: while timing is on, every render launch records its own (start, stop) pair
  std::vector<hipEvent_t> pool;
  int pool_used = 0;
  bool timing = false;
  int timing_stride = 1, timing_seen = 0;  // every timing_stride-th launch is timed
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev2 = nullptr, ev3 = nullptr;  // glome_render_lens with statistics: its raygen and resolve stages (a trace launch in between records ev0 / ev1)
  hipDeviceProp_t prop;
  // Per-slot launch state, so several frames can be in flight on different streams (their work queues, counters and
  // workspaces must not be shared): slot 0 is the default.
  struct Slot {
    DCounters* d_counters = nullptr;
    uint32_t* d_ovf = nullptr;   // traversal-stack overflow workspace (grown on demand)
    size_t ovf_bytes = 0;
    float* d_scratch = nullptr;  // adaptive sampler working buffer
    size_t scratch_bytes = 0;
    uint32_t* d_list = nullptr;  // the flagship launch's ticket list, then its cull pass's chunk masks (cull_kernels.hpp)
    size_t list_items = 0;       // ... sized for this many work items (ensure_list)
    uint32_t cull_total = 0;     // work items of the slot's last flagship launch (its live ones: DCounters::list_len)
    float* d_lens = nullptr;     // glome_render_lens: a pass's six ray streams, then its n * 5 results (grown on demand)
    size_t lens_bytes = 0;
    uint32_t* d_adapt = nullptr; // glome_render_lens_adaptive: a pass's list lengths, pixel states and two lists (grown on demand)
    size_t adapt_bytes = 0;
    bool launched = false;  // a launch went out on this slot since its error word was last polled
    hipStream_t launched_on = nullptr;  // ... on this stream (a caller's own stream is the caller's to synchronise)
  };
  static constexpr int kSlots = 8;
  Slot slots[kSlots];
  int cur = 0;
  Slot& slot() { return slots[cur]; }
  std::string err;
  int grid_per_cu = 0;  // 0: persistent grids sized by work (tuned for several launches in flight); > 0: this many waves per CU, resources permitting
  // tile tables cached per (w, h, blocksize, first, stride)
  // lut[w >> 6] = the tile that holds work item (w & ~63): the kernel's item -> tile lookup is one table read and a step or two
  // items: the plan's item table (DItem: one entry per work item, read by the lean render loop)
  struct TileTable { std::vector<DTile> host; DTile* dev = nullptr; uint32_t* lut = nullptr; DItem* items = nullptr; uint32_t total_waves = 0; int64_t pixels = 0; };
  std::map<std::vector<int>, TileTable> tile_cache;
  std::map<std::pair<int, int>, float*> coord_cache;  // (width, height) -> xc[width] then yc[height] (k_coord_tables)
};
struct glome_scene {
  glome_ctx* ctx = nullptr;
  int ovf_cap = 0;  // stack entries per lane beyond the LDS part
  DScene dev{};
  std::vector<void*> allocs;
  glome_scene_info info{};
  SceneTraits tr;   // what the choice of a kernel instance looks at (instances.hpp; tr.stack_cap: stack entries per lane in LDS)
  // what glome_scene_mesh_update needs of every Mesh of the scene, by its builder id (flatten.hpp MeshUpdateInfo; the index rows and the
  // level list live on the device, in `allocs`); outside DScene: no render, sampler or trace kernel sees any of it
  struct MeshUpd {
    MeshUpdateInfo info;               // (rows and level_nodes emptied once uploaded)
    const int32_t* d_rows = nullptr;
    const uint32_t* d_levels = nullptr;
    float4* d_ws = nullptr;            // two words per record, then the bound's partial boxes: allocated at the first update
  };
  std::map<int, MeshUpd> meshes;
  // the same for glome_scene_bih_update and glome_scene_sphere_bih_update, of every triangle bih and sphere bih of the scene (flatten.hpp
  // LeafBihUpdateInfo: info.cls tells them apart)
  struct LeafBihUpd {
    LeafBihUpdateInfo info;            // (rows and level_nodes emptied once uploaded)
    const uint32_t* d_rows = nullptr;  // info.row_words words per record
    const uint32_t* d_levels = nullptr;
    const uint32_t* d_level_off = nullptr;
    float4* d_ws = nullptr;            // two words per record, two per node slot, then the bound's partial boxes: allocated at the first update
    // what a rebuild (glome_scene_bih_rebuild) needs beyond an update's tables: per item, in update order, its record as commit emitted it
    // (flags and kind, -, own-texture word, builder id: .y is made again with the leaf order); what the tree's node segment and pair segment
    // hold (slots; pair records), initially their committed size; and what the device tables above and the workspace hold
    std::vector<U4> item_recs;
    uint32_t slot_cap = 0, pair_cap = 0;
    size_t rows_cap = 0, levels_cap = 0, level_off_cap = 0, ws_words = 0;
  };
  std::map<int, LeafBihUpd> leaf_bihs;
  // what commit derived from every bih's depth, kept so that a rebuild can derive it again: per bih header its tree's depth and whether it
  // counts towards max_sphere_bih_depth (flatten.hpp emit_bih); the Meshes' deepest tree; and the pools a rebuild may extend -- entries in
  // use and entries allocated of bihnodes / pknodes, float words of tripairs
  std::vector<int> hdr_depth;
  std::vector<uint8_t> hdr_packet_service;
  int max_mesh_depth = 0;
  size_t bihnodes_used = 0, bihnodes_cap = 0, tripairs_used = 0, tripairs_cap = 0;
  double rebuild_stage_ms[5] = {0, 0, 0, 0, 0};  // the last rebuild's wall-clock by stage (glome_scene_bih_rebuild_stages)
  // and for glome_scene_instance_update: every Instance of the scene by its builder id, and every bih that holds one as an item
  // (flatten.hpp InstanceUpdateInfo, InstBihInfo)
  std::map<int, InstanceUpdateInfo> insts;
  struct InstBih {
    InstBihInfo info;                  // (level_nodes emptied once uploaded; rows once the workspace holds them)
    const uint32_t* d_levels = nullptr;
    const uint32_t* d_rec_off = nullptr;
    const double* d_bounds = nullptr;
    // two words per record of the tree's span (plane-form rows), two per node slot, two per item (box-form rows), then the bound's partial
    // boxes: allocated, and filled with the commit-time rows, at the first update that touches the tree
    float4* d_ws = nullptr;
    // the refit's tables (item_bih_update_kernels.hpp), allocated and filled with the workspace: six doubles of bound(item) per item, then 24
    // doubles of matrix per item (the commit's for an instanced live item, zeros until an update names the item otherwise); the live items
    // as (item, the object's row of the bounds table | kInstancedBit); per item the row of its live child, kNoLive for none
    double* d_box64 = nullptr;
    double* d_xf = nullptr;
    const uint2* d_live_items = nullptr;
    const uint32_t* d_item_live = nullptr;
    uint32_t n_live = 0;
  };
  std::map<int, InstBih> ibihs;
  // glome_scene_nested_updates: the switch; every Mesh, triangle bih, sphere bih and table-holding bih has a row of six doubles in d_live, its fp64
  // bound (live_bound0: the commit's, what the table is filled with when the switch is first turned on); d_live_part: the partial boxes
  // of a bound's first stage; stale: the bihs whose planes and box no longer match an object below them
  bool nested_on = false;
  std::map<int, uint32_t> live_slot;
  std::vector<double> live_bound0;
  double* d_live = nullptr;
  double* d_live_part = nullptr;
  std::set<int> stale;
  // an update's own tables (which matrix goes to which slot / item) travel through pinned buffers, so that the device form stays
  // asynchronous: a small ring, a buffer reused once the copy out of it has run.  The ring protects the PINNED side only: the one device
  // table d_inst_rows is rewritten by every call, which is safe because a call's copy into it is ordered, on the stream, after the
  // kernels of the call before it -- calls on other streams are the caller's to order, as for the pools themselves
  struct RowStage { uint2* h = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; };
  RowStage inst_stage[4];
  int inst_stage_next = 0;
  uint2* d_inst_rows = nullptr;
  size_t inst_rows_cap = 0;
  // glome_scene_instance_update_from: the 24 doubles per named Instance its conversion kernel makes of the caller's source, which the
  // update's kernels then read.  One per scene, grown like d_inst_rows and ordered like it
  double* d_xfm_table = nullptr;
  size_t xfm_table_cap = 0;  // matrices
};

static std::string g_global_error;
#define HIPCHK(ctx, call)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
      return GLOME_E_HIP;                                                                          \
    }                                                                                              \
  } while (0)

static int check_params(glome_ctx* ctx, const glome_render_params* P) {
  if (!P || P->width <= 0 || P->height <= 0 || P->blocksize <= 0 || P->tile_stride <= 0 || P->tile_first < 0 || P->rank0_share_pct < 0 || P->rank0_share_pct > 100) { ctx->err = "bad render params"; return GLOME_E_INVALID; }
  if ((int64_t)P->width * P->height > (1ll << 30)) { ctx->err = "frame too large"; return GLOME_E_INVALID; }
  if (P->maxdepth < 1 || P->maxdepth > kMaxTraceDepth) { ctx->err = "maxdepth must be in 1.." + std::to_string(kMaxTraceDepth); return GLOME_E_LIMIT; }
  return 0;
}
static int get_tiles(glome_ctx* ctx, const glome_render_params* P, int first, int stride, glome_ctx::TileTable** out, int blocksize = 0) {
  if (!blocksize) blocksize = P->blocksize;
  std::vector<int> key{P->width, P->height, blocksize, first, stride, P->rank0_share_pct};
  auto it = ctx->tile_cache.find(key);
  if (it == ctx->tile_cache.end()) {
    glome_ctx::TileTable tt;
    owned_tiles(P->width, P->height, blocksize, first, stride, P->rank0_share_pct, tt.host, tt.total_waves, tt.pixels);
    size_t bytes = std::max<size_t>(1, tt.host.size()) * sizeof(DTile);
    HIPCHK(ctx, hipMalloc((void**)&tt.dev, bytes));
    if (!tt.host.empty()) HIPCHK(ctx, hipMemcpy(tt.dev, tt.host.data(), tt.host.size() * sizeof(DTile), hipMemcpyHostToDevice));
    std::vector<uint32_t> lut((tt.total_waves >> 6) + 1, 0);
    for (size_t k = 0, t = 0; k < lut.size(); k++) {
      while (t + 1 < tt.host.size() && tt.host[t + 1].wave_base <= (uint32_t)(k << 6)) t++;
      lut[k] = (uint32_t)t;
    }
    HIPCHK(ctx, hipMalloc((void**)&tt.lut, lut.size() * sizeof(uint32_t)));
    HIPCHK(ctx, hipMemcpy(tt.lut, lut.data(), lut.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    std::vector<DItem> items;
    build_item_table(tt.host, tt.total_waves, items);
    HIPCHK(ctx, hipMalloc((void**)&tt.items, std::max<size_t>(1, items.size()) * sizeof(DItem)));
    if (!items.empty()) HIPCHK(ctx, hipMemcpy(tt.items, items.data(), items.size() * sizeof(DItem), hipMemcpyHostToDevice));
    it = ctx->tile_cache.emplace(key, std::move(tt)).first;
  }
  *out = &it->second;
  return 0;
}
// xc[width] | yc[height] of a frame size, filled once per context (and complete before this returns: the slots launch on streams of their own)
static int get_coord_tables(glome_ctx* ctx, int width, int height, float** out) {
  auto it = ctx->coord_cache.find({width, height});
  if (it == ctx->coord_cache.end()) {
    float* d = nullptr;
    HIPCHK(ctx, hipMalloc((void**)&d, ((size_t)width + (size_t)height) * sizeof(float)));
    const int n = std::max(width, height);
    hipLaunchKernelGGL(k_coord_tables, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, width, height, d, d + width);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(d); ctx->err = std::string("k_coord_tables: ") + hipGetErrorString(e); return GLOME_E_HIP; }
    it = ctx->coord_cache.emplace(std::make_pair(width, height), d).first;
  }
  *out = it->second;
  return 0;
}
int glome_ctx_coord_tables(glome_ctx* ctx, int width, int height, float* xc, float* yc, int direct) {
  if (!ctx || width <= 0 || height <= 0 || !xc || !yc || (int64_t)width * height > (1ll << 30)) return GLOME_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  float* d = nullptr;
  if (direct) {
    HIPCHK(ctx, hipMalloc((void**)&d, ((size_t)width + (size_t)height) * sizeof(float)));
    const int n = std::max(width, height);
    hipLaunchKernelGGL(k_coords_direct, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, width, height, d, d + width);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(d); ctx->err = std::string("k_coords_direct: ") + hipGetErrorString(e); return GLOME_E_HIP; }
  } else if (int rc = get_coord_tables(ctx, width, height, &d)) return rc;
  hipError_t e = hipMemcpy(xc, d, (size_t)width * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(yc, d + width, (size_t)height * sizeof(float), hipMemcpyDeviceToHost);
  if (direct) (void)hipFree(d);
  if (e != hipSuccess) { ctx->err = std::string("hipMemcpy: ") + hipGetErrorString(e); return GLOME_E_HIP; }
  return 0;
}

template <class T> static int upload(glome_scene* s, const std::vector<T>& v, const T** out) {
  glome_ctx* ctx = s->ctx;
  void* d = nullptr;
  size_t bytes = v.size() * sizeof(T);
  HIPCHK(ctx, hipMalloc(&d, bytes));
  s->allocs.push_back(d);
  HIPCHK(ctx, hipMemcpy(d, v.data(), bytes, hipMemcpyHostToDevice));
  s->info.device_bytes += (int64_t)bytes;
  *out = (const T*)d;
  return 0;
}
static void drop_alloc(glome_scene* s, const void* p) {
  if (!p) return;
  auto it = std::find(s->allocs.begin(), s->allocs.end(), (void*)p);
  if (it != s->allocs.end()) s->allocs.erase(it);
  (void)hipFree((void*)p);
}
// a fresh allocation becomes the scene's in place of what `slot` held, which is freed (no launch reads it: the caller has quiesced)
template <class T> static void adopt(glome_scene* s, const T*& slot, T*& fresh) {
  if (!fresh) return;
  drop_alloc(s, slot);
  s->allocs.push_back(fresh);
  slot = fresh; fresh = nullptr;
}
// The device tables of a leaf bih's update -- rows, level_nodes, level_off (flatten.hpp LeafBihLayout; a tree whose root is a leaf has no
// levels) -- filled from a layout: by commit for the first time, by a rebuild again.  room(): a fresh allocation for every table that
// lacks the room, all of them before anything is copied; fill(): the copies; take(): the fresh ones become the scene's and the
// capacities follow.  Until take() the scene is as it was, and what room() allocated goes with this.
struct LeafTables {
  struct One { const uint32_t*& d; size_t& cap; const std::vector<uint32_t>& v; uint32_t* fresh; };
  One t[3];
  LeafTables(glome_scene::LeafBihUpd& m, const std::vector<uint32_t>& rows, const std::vector<uint32_t>& level_nodes, const std::vector<uint32_t>& level_off)
      : t{{m.d_rows, m.rows_cap, rows, nullptr}, {m.d_levels, m.levels_cap, level_nodes, nullptr}, {m.d_level_off, m.level_off_cap, level_off, nullptr}} {}
  LeafTables(const LeafTables&) = delete;
  ~LeafTables() { for (One& o : t) (void)hipFree(o.fresh); }
  int room(glome_ctx* ctx) {
    for (One& o : t) if (!o.v.empty() && (o.v.size() > o.cap || !o.d)) HIPCHK(ctx, hipMalloc((void**)&o.fresh, o.v.size() * sizeof(uint32_t)));
    return 0;
  }
  int fill(glome_ctx* ctx) {
    for (One& o : t) if (!o.v.empty()) HIPCHK(ctx, hipMemcpy(o.fresh ? o.fresh : (uint32_t*)o.d, o.v.data(), o.v.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
  }
  void take(glome_scene* s) {
    for (One& o : t) if (o.fresh) { o.cap = o.v.size(); adopt(s, o.d, o.fresh); }
  }
};

const char* glome_global_error(void) { return g_global_error.c_str(); }

glome_ctx* glome_ctx_create(int device_ordinal) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) { g_global_error = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"); return nullptr; }
  if (device_ordinal < 0 || device_ordinal >= n) { g_global_error = "device ordinal out of range"; return nullptr; }
  glome_ctx* c = new glome_ctx();
  c->device = device_ordinal;
  auto fail = [&](const char* what, hipError_t err) { g_global_error = std::string(what) + ": " + hipGetErrorString(err); delete c; return (glome_ctx*)nullptr; };
  if ((e = hipSetDevice(device_ordinal)) != hipSuccess) return fail("hipSetDevice", e);
  if ((e = hipGetDeviceProperties(&c->prop, device_ordinal)) != hipSuccess) return fail("hipGetDeviceProperties", e);
  if (std::string(c->prop.gcnArchName).rfind("gfx950", 0) != 0) {
    g_global_error = std::string("device is ") + c->prop.gcnArchName + ", this library is built for gfx950 only";
    delete c;
    return nullptr;
  }
  // The context's own stream is a BLOCKING stream: work a caller put on the device's default stream (filling or allocating
  // the very buffers it hands to a *_dev entry point) is ordered before this context's launches and after them, as with any
  // HIP code that never names a stream.  A caller that wants overlap brings its own streams (glome_ctx_use_slot).
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamDefault)) != hipSuccess) return fail("hipStreamCreate", e);
  c->own_stream = c->stream;
  if ((e = hipEventCreate(&c->ev0)) != hipSuccess) return fail("hipEventCreate", e);
  if ((e = hipEventCreate(&c->ev1)) != hipSuccess) return fail("hipEventCreate", e);
  if ((e = hipEventCreate(&c->ev2)) != hipSuccess || (e = hipEventCreate(&c->ev3)) != hipSuccess) return fail("hipEventCreate", e);
  for (int k = 0; k < glome_ctx::kSlots; k++)
    if ((e = hipMalloc((void**)&c->slots[k].d_counters, sizeof(DCounters))) != hipSuccess || (e = hipMemset(c->slots[k].d_counters, 0, sizeof(DCounters))) != hipSuccess) return fail("hipMalloc", e);
  {  // kernel_args<>()'s assumption about the kernarg segment, checked once per process on the first context
    static std::once_flag once;
    static bool good = true;
    std::call_once(once, [&] {
      DRenderArgs* h = new DRenderArgs;
      unsigned char* hb = (unsigned char*)h;
      for (size_t i = 0; i < sizeof(DRenderArgs); i++) hb[i] = (unsigned char)(i * 131u + 7u);
      DRenderArgs* d = nullptr; unsigned int* ok = nullptr; unsigned int one = 1, got = 0;
      if (hipMalloc((void**)&d, sizeof(DRenderArgs)) == hipSuccess && hipMalloc((void**)&ok, sizeof(unsigned int)) == hipSuccess &&
          hipMemcpy(d, h, sizeof(DRenderArgs), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(ok, &one, sizeof(one), hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(k_kernarg_selftest, dim3(1), dim3(256), 0, c->stream, *h, d, ok);
        if (hipStreamSynchronize(c->stream) == hipSuccess && hipMemcpy(&got, ok, sizeof(got), hipMemcpyDeviceToHost) == hipSuccess) good = got == 1u;
        else good = false;
      } else good = false;
      if (d) (void)hipFree(d);
      if (ok) (void)hipFree(ok);
      delete h;
    });
    if (!good) { g_global_error = "kernel-argument self-test failed: the first by-value kernel argument is not at offset 0 of the kernarg segment in host layout (kernel_args<>)"; glome_ctx_destroy(c); return nullptr; }
  }
  return c;
}
void glome_ctx_destroy(glome_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (auto& kv : c->tile_cache) { if (kv.second.dev) (void)hipFree(kv.second.dev); if (kv.second.lut) (void)hipFree(kv.second.lut); if (kv.second.items) (void)hipFree(kv.second.items); }
  for (auto& kv : c->coord_cache) (void)hipFree(kv.second);
  for (auto& sl : c->slots) {
    if (sl.d_counters) (void)hipFree(sl.d_counters);
    if (sl.d_ovf) (void)hipFree(sl.d_ovf);
    if (sl.d_scratch) (void)hipFree(sl.d_scratch);
    if (sl.d_list) (void)hipFree(sl.d_list);
    if (sl.d_lens) (void)hipFree(sl.d_lens);
    if (sl.d_adapt) (void)hipFree(sl.d_adapt);
  }
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev2) (void)hipEventDestroy(c->ev2);
  if (c->ev3) (void)hipEventDestroy(c->ev3);
  for (hipEvent_t ev : c->pool) (void)hipEventDestroy(ev);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}
const char* glome_last_error(const glome_ctx* c) { return c ? c->err.c_str() : g_global_error.c_str(); }
void* glome_ctx_stream(glome_ctx* c) { return c ? (void*)c->stream : nullptr; }
int glome_ctx_use_stream(glome_ctx* c, void* stream) {
  if (!c) return GLOME_E_INVALID;
  c->stream = stream ? (hipStream_t)stream : c->own_stream;
  return 0;
}
int glome_ctx_use_slot(glome_ctx* c, void* stream, int slot) {
  if (!c || slot < 0 || slot >= glome_ctx::kSlots) return GLOME_E_INVALID;
  c->stream = stream ? (hipStream_t)stream : c->own_stream;
  c->cur = slot;
  // a slot rebound to another stream forgets the one its last launch went to: that handle is the caller's and may be destroyed by
  // now (glome_ctx_synchronize must not query it); the slot's error word is then read without asking whether the old stream is idle
  // -- a word a running kernel ORs into later is reported by the next synchronize
  glome_ctx::Slot& sl = c->slots[slot];
  if (sl.launched && sl.launched_on != c->stream) sl.launched_on = nullptr;
  return 0;
}
int glome_ctx_set_grid_per_cu(glome_ctx* c, int waves_per_cu) {
  if (!c || waves_per_cu < 0 || waves_per_cu > 32) return GLOME_E_INVALID;
  c->grid_per_cu = waves_per_cu;
  return 0;
}
int glome_ctx_last_cull(glome_ctx* c, int64_t* live, int64_t* total) {
  if (!c || !live || !total) return GLOME_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  unsigned int n = 0;
  if (c->slot().cull_total) HIPCHK(c, hipMemcpy(&n, &c->slot().d_counters->list_len, sizeof(n), hipMemcpyDeviceToHost));
  *live = (int64_t)n; *total = (int64_t)c->slot().cull_total;
  return 0;
}
int glome_ctx_timing_begin(glome_ctx* c, int max_launches) {
  if (!c || max_launches <= 0) return GLOME_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  while ((int)c->pool.size() < 2 * max_launches) {
    hipEvent_t ev;
    HIPCHK(c, hipEventCreate(&ev));
    c->pool.push_back(ev);
  }
  c->pool_used = 0;
  c->timing = true;
  c->timing_stride = 1; c->timing_seen = 0;
  return 0;
}
int glome_ctx_timing_begin_sampled(glome_ctx* c, int max_launches, int stride) {
  int rc = glome_ctx_timing_begin(c, max_launches);
  if (rc == 0) c->timing_stride = stride < 1 ? 1 : stride;
  return rc;
}
int glome_ctx_timing_end(glome_ctx* c, float* ms_out, int cap) {
  if (!c) return GLOME_E_INVALID;
  c->timing = false;
  int n = c->pool_used / 2;
  // the pairs were recorded on whichever lane stream launched (up to kSlots of them): wait on each stop event itself
  for (int i = 0; i < n && i < cap; i++) {
    HIPCHK(c, hipEventSynchronize(c->pool[2 * i + 1]));
    HIPCHK(c, hipEventElapsedTime(&ms_out[i], c->pool[2 * i], c->pool[2 * i + 1]));
  }
  return n;
}
static int poll_device_error(glome_ctx* ctx, glome_ctx::Slot& sl);
int glome_ctx_synchronize(glome_ctx* c) {
  if (!c) return GLOME_E_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // limits hit by launches nobody asked statistics of; lanes on the caller's own streams are the caller's to synchronise
  // first (an error raised by a launch still in flight is reported by the next call)
  int rc = 0;
  for (auto& sl : c->slots) {
    if (!sl.launched) continue;
    // a slot bound to a caller's stream (glome_ctx_use_slot) may still be running: its word is read once that stream is idle,
    // by this call or a later one -- never while a kernel could still OR into it
    if (sl.launched_on && sl.launched_on != c->stream && hipStreamQuery(sl.launched_on) == hipErrorNotReady) continue;
    sl.launched = false;
    int r = poll_device_error(c, sl);
    if (r) rc = r;
  }
  return rc;
}
// ---- a framebuffer several PROCESSES render into (one process per GPU: glome_amd/dist.py) ----
// rank 0 allocates the frames and exports a handle; the other ranks open it and hand the pointer to their render calls, whose kernels
// then store their tiles' pixels straight into rank 0's memory over xGMI (hipIpc*: dmabuf handles on this driver).
int glome_ipc_alloc(glome_ctx* c, size_t bytes, void** dev_ptr, unsigned char* handle64) {
  if (!c || !dev_ptr || !handle64 || bytes == 0) return GLOME_E_INVALID;
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "a HIP IPC memory handle is 64 bytes");
  HIPCHK(c, hipSetDevice(c->device));
  void* p = nullptr;
  HIPCHK(c, hipMalloc(&p, bytes));
  hipIpcMemHandle_t h;
  hipError_t e = hipIpcGetMemHandle(&h, p);
  if (e != hipSuccess) { (void)hipFree(p); c->err = std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e); (void)hipGetLastError(); return GLOME_E_HIP; }
  memcpy(handle64, &h, 64);
  HIPCHK(c, hipMemset(p, 0, bytes));
  *dev_ptr = p;
  return 0;
}
int glome_ipc_open(glome_ctx* c, const unsigned char* handle64, void** dev_ptr) {
  if (!c || !dev_ptr || !handle64) return GLOME_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  hipIpcMemHandle_t h;
  memcpy(&h, handle64, 64);
  hipError_t e = hipIpcOpenMemHandle(dev_ptr, h, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) { c->err = std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e); (void)hipGetLastError(); return GLOME_E_HIP; }
  return 0;
}
int glome_ipc_close(glome_ctx* c, void* dev_ptr, int owner) {  // owner: the process that allocated frees, the others close their mapping
  if (!c || !dev_ptr) return GLOME_E_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  if (owner) HIPCHK(c, hipFree(dev_ptr)); else HIPCHK(c, hipIpcCloseMemHandle(dev_ptr));
  return 0;
}
int glome_ctx_device_info(glome_ctx* c, char* name, int cap, int* cu_count, int* warp_size) {
  if (!c) return GLOME_E_INVALID;
  if (name && cap > 0) snprintf(name, cap, "%s (%s)", c->prop.name, c->prop.gcnArchName);
  if (cu_count) *cu_count = c->prop.multiProcessorCount;
  if (warp_size) *warp_size = c->prop.warpSize;
  return 0;
}

// ---- bih, built on the device (bih_build_device.hpp) ----
static int32_t bihdev_status(int rc) {  // a refusal of the level loop as a status of the C ABI
  return rc == bihdev::kRefusedLimit ? GLOME_E_LIMIT : rc == bihdev::kRefusedLoop ? GLOME_E_SCENE : GLOME_E_HIP;
}
int32_t glome_sb_bih_dev(glome_ctx* ctx, glome_sb* sb, const int32_t* ids, int32_t n, float* gpu_ms) {
  if (!ctx || !sb) { g_global_error = "null ctx or builder"; return GLOME_E_INVALID; }
  if (gpu_ms) *gpu_ms = 0;
  try {
    if (n < 0 || (n > 0 && !ids)) throw std::invalid_argument("bad id list");
    Graph& G = sb->graph;
    std::vector<int> v(ids, ids + n);
    if (v.empty()) return G.bih(v);  // bih [] = Void, Bih.hs:309-311
    std::vector<Box3> boxes;
    Box3 bb = box_empty();
    for (int i : v) boxes.push_back(G.bound(i));
    for (auto& b : boxes) bb = box_join(bb, b);
    if (bb.lo.x == -kInfinity || bb.lo.y == -kInfinity || bb.lo.z == -kInfinity || bb.hi.x == kInfinity || bb.hi.y == kInfinity || bb.hi.z == kInfinity)
      throw scene_error("bih: infinite bounding box");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    auto T = std::make_shared<BihTree>();
    std::string err;
    if (const int rc = bihdev::build(boxes, v, bb, *T, ctx->stream, err, gpu_ms)) { ctx->err = sb->err = err; return bihdev_status(rc); }
    T->order = v;
    Node nd; nd.kind = K_BIH; nd.bih = T;
    return G.add(nd);
  } catch (const scene_error& e) { ctx->err = sb->err = e.what(); return GLOME_E_SCENE; }
  catch (const std::exception& e) { ctx->err = sb->err = e.what(); return GLOME_E_INVALID; }
}

int32_t glome_sb_mesh_dev(glome_ctx* ctx, glome_sb* sb, const double* verts, int nv, const double* norms, int nn, const int32_t* tris, int nt, const int32_t* mats, int nm,
                          float* gpu_ms) {
  if (!ctx || !sb) { g_global_error = "null ctx or builder"; return GLOME_E_INVALID; }
  if (gpu_ms) *gpu_ms = 0;
  try {
    if (nv < 0 || nn < 0 || nt < 0 || nm < 0 || (nv && !verts) || (nn && !norms) || (nt && !tris) || (nm && !mats)) throw std::invalid_argument("bad mesh arrays");
    Graph& G = sb->graph;
    std::vector<D3> V, N;
    for (int k = 0; k < nv; k++) V.push_back(D3{verts[3 * k], verts[3 * k + 1], verts[3 * k + 2]});
    for (int k = 0; k < nn; k++) N.push_back(D3{norms[3 * k], norms[3 * k + 1], norms[3 * k + 2]});
    std::vector<MeshTri> T;
    for (int k = 0; k < nt; k++) { const int32_t* t = tris + 8 * k; T.push_back(MeshTri{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]}); }
    std::vector<int> M(mats, mats + nm);
    if (nt < 3) return G.mesh(std::move(V), std::move(N), std::move(T), std::move(M));  // a single leaf (Mesh.hs:70)
    std::vector<Box3> tbb;
    auto D = G.mesh_data(std::move(V), std::move(N), std::move(T), std::move(M), tbb);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string err;
    if (const int rc = bihdev::build_mesh(tbb, *D, ctx->stream, err, gpu_ms)) { ctx->err = sb->err = err; return bihdev_status(rc); }
    return G.mesh_node(D);
  } catch (const scene_error& e) { ctx->err = sb->err = e.what(); return GLOME_E_SCENE; }
  catch (const std::exception& e) { ctx->err = sb->err = e.what(); return GLOME_E_INVALID; }
}

// ---- commit ----
glome_scene* glome_scene_commit(glome_ctx* ctx, glome_sb* sb, int32_t root) {
  if (!ctx || !sb) { g_global_error = "null ctx or builder"; return nullptr; }
  FlatScene F;
  try {
    Flattener fl(sb_graph(sb), F);
    fl.run(root);
  } catch (std::exception& e) { ctx->err = e.what(); return nullptr; }
  (void)hipSetDevice(ctx->device);
  glome_scene* s = new glome_scene();
  s->ctx = ctx;
  int rc = 0;
  DScene& D = s->dev;
  rc |= upload(s, F.recs, &D.recs);
  rc |= upload(s, F.spheres, &D.spheres); rc |= upload(s, F.tris, &D.tris); rc |= upload(s, F.tripairs, &D.tripairs); rc |= upload(s, F.trinorms, &D.trinorms);
  rc |= upload(s, F.boxes, &D.boxes); rc |= upload(s, F.planes, &D.planes); rc |= upload(s, F.discs, &D.discs);
  rc |= upload(s, F.quadrics, &D.quadrics); rc |= upload(s, F.xfms, &D.xfms);
  rc |= upload(s, F.bihhdr, &D.bihhdr); rc |= upload(s, F.bihnodes, &D.bihnodes); rc |= upload(s, F.pknodes, &D.pknodes); D.pknodes_bytes = (uint32_t)(F.pknodes.size() * sizeof(F4));
  rc |= upload(s, F.meshhdr, &D.meshhdr); rc |= upload(s, F.meshnodes, &D.meshnodes); rc |= upload(s, F.mtris, &D.mtris);
  rc |= upload(s, F.mtrimeta, &D.mtrimeta); rc |= upload(s, F.mats, &D.mats); rc |= upload(s, F.wlights, &D.wlights); rc |= upload(s, F.matkids, &D.matkids);
  rc |= upload(s, F.entries, &D.entries); rc |= upload(s, F.walk, &D.walk); D.walk_pad = 0;
  if (rc) { glome_scene_release(s); return nullptr; }
  D.n_entries = F.tier == 0 ? (uint32_t)F.entries.size() : 0;
  D.root_rec = F.root_rec; D.tier = F.tier; D.n_mats = (uint32_t)sb_graph(sb).mats.size(); D.tex_bits = F.tex_bits;
  const CommitRules R = commit_rules(sb_graph(sb), F);  // (instances.hpp scene_caps: entry classes, stack entries, the generic tier's packet stack)
  D.pk_generic_cap = R.caps.pk_generic_cap;
  if (getenv("GLOME_DEBUG_NO_GENERIC_PACKETS")) D.pk_generic_cap = 0;  // (debug switch: every BIH inside the interpreter walked lane by lane -- the test that holds the packet service against it)
  glome_scene_info& I = s->info;
  I.tier = (int32_t)F.tier; I.nesting_depth = F.nesting_depth;
  I.n_records = (int64_t)F.recs.size(); I.n_bih_nodes = (int64_t)F.bihnodes.size(); I.n_mesh_nodes = (int64_t)F.meshnodes.size() / 4;
  I.n_triangles = (int64_t)(F.tris.size() + F.mtris.size()) / 3; I.n_spheres = (int64_t)F.spheres.size();
  I.n_other_prims = F.n_other_prims; I.n_xfms = (int64_t)F.xfms.size() / 6; I.n_materials = D.n_mats;
  I.max_bih_depth = F.max_bih_depth; I.max_mesh_depth = F.max_mesh_depth;
  s->tr = R.traits;
  s->ovf_cap = R.caps.ovf_cap;
  for (MeshUpdateInfo& U : F.mesh_updates) {
    glome_scene::MeshUpd& m = s->meshes[U.node];
    if (upload(s, U.rows, &m.d_rows) || (!U.level_nodes.empty() && upload(s, U.level_nodes, &m.d_levels))) { glome_scene_release(s); return nullptr; }
    U.rows = {}; U.level_nodes = {};
    m.info = std::move(U);
  }
  for (LeafBihUpdateInfo& U : F.leaf_bih_updates) {
    glome_scene::LeafBihUpd& m = s->leaf_bihs[U.node];
    LeafTables tables(m, U.rows, U.level_nodes, U.level_off);
    if (tables.room(ctx) || tables.fill(ctx)) { glome_scene_release(s); return nullptr; }
    tables.take(s);
    s->info.device_bytes += (int64_t)((U.rows.size() + U.level_nodes.size() + U.level_off.size()) * sizeof(uint32_t));
    m.item_recs.assign((size_t)U.n_items, U4{0, 0, 0, 0});
    for (uint32_t j = 0; j < U.n_recs; j++) m.item_recs[U.rows[(size_t)j * U.row_words]] = F.recs[(size_t)U.first_rec + j];
    m.slot_cap = std::max<uint32_t>(U.n_slots, 1u); m.pair_cap = U.n_pair_recs;
    U.rows = {}; U.level_nodes = {};
    m.info = std::move(U);
  }
  for (size_t h = 0; 3 * h + 2 < F.bihhdr.size(); h++) {
    uint32_t w; memcpy(&w, &F.bihhdr[3 * h + 2].w, 4);
    uint32_t cl; memcpy(&cl, &F.bihhdr[3 * h + 1].w, 4);
    s->hdr_depth.push_back((int)(w & ~kBihItemsInPlace));
    s->hdr_packet_service.push_back(cl == BC_SPHERE || cl == BC_TRI || (w & kBihItemsInPlace) != 0);
  }
  s->max_mesh_depth = F.max_mesh_depth;
  s->bihnodes_used = s->bihnodes_cap = F.bihnodes.size(); s->tripairs_used = s->tripairs_cap = F.tripairs.size();
  for (InstBihInfo& B : F.inst_bihs) {
    glome_scene::InstBih& m = s->ibihs[B.node];
    if ((!B.level_nodes.empty() && upload(s, B.level_nodes, &m.d_levels)) || upload(s, B.rec_off, &m.d_rec_off) || upload(s, B.child_bound, &m.d_bounds)) { glome_scene_release(s); return nullptr; }
    B.level_nodes = {};
    m.info = std::move(B);
  }
  for (InstanceUpdateInfo& U : F.inst_updates) { const int node = U.node; s->insts[node] = std::move(U); }
  auto live_row = [&](int node, const double* b6) { s->live_slot[node] = (uint32_t)(s->live_bound0.size() / 6); s->live_bound0.insert(s->live_bound0.end(), b6, b6 + 6); };
  for (auto& m : s->meshes) live_row(m.first, m.second.info.bound6);
  for (auto& m : s->leaf_bihs) live_row(m.first, m.second.info.bound6);
  for (auto& m : s->ibihs) live_row(m.first, m.second.info.bound6);
  return s;
}
void glome_scene_release(glome_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->ctx->device);
  for (void* p : s->allocs) (void)hipFree(p);
  for (auto& st : s->inst_stage) { if (st.h) (void)hipHostFree(st.h); if (st.ev) (void)hipEventDestroy(st.ev); }
  if (s->d_inst_rows) (void)hipFree(s->d_inst_rows);
  if (s->d_xfm_table) (void)hipFree(s->d_xfm_table);
  delete s;
}
int glome_scene_get_info(const glome_scene* s, glome_scene_info* out) {
  if (!s || !out) return GLOME_E_INVALID;
  *out = s->info;
  return 0;
}

// ---- launch helpers ----
// Waves of a persistent launch.  At most what the CU can hold (LDS, register budget); fewer when the launch is small: a wave
// should get ~64 work items, so that its fixed costs (set-up, the counter flush) amortise and several launches in flight
// share the CUs side by side instead of one after the other (measured on the flagship frame, 4 launches of 4 frames in
// flight: 24 waves per CU 0.272 ms, 16: 0.249, 8: 0.239; the 4K / 1M-triangle frame, 4x the items, is best at 24).
// Is anything still running on the streams the context's OTHER slots last launched on?  A launch sized by its work (below) leaves room
// for the launches beside it; one that has the GPU to itself -- a short multi-GPU run is ONE launch of a rank's shard, nothing beside it --
// wants every wave slot: twenty frames of an eighth of the flagship's tiles 0.90 -> 0.66 ms (profiles/r04_probes/short_run_shards.txt).
static bool other_slots_busy(glome_ctx* ctx) {
  for (int k = 0; k < glome_ctx::kSlots; k++) {
    const glome_ctx::Slot& sl = ctx->slots[k];
    if (k == ctx->cur || !sl.launched_on || sl.launched_on == ctx->stream) continue;
    if (hipStreamQuery(sl.launched_on) == hipErrorNotReady) return true;
  }
  (void)hipGetLastError();  // (a query of a finished stream leaves nothing behind; one of a stream its owner has destroyed must not be this call's error)
  return false;
}
static int persistent_grid(glome_ctx* ctx, size_t lds_per_block, uint32_t total_work, int max_per_cu = 32, int min_per_cu = 0) {
  int cus = ctx->prop.multiProcessorCount;
  int per_cu = max_per_cu;  // wave slots per CU the kernel's register budget allows
  if (lds_per_block) per_cu = std::min<int>(per_cu, (int)(160 * 1024 / lds_per_block));
  per_cu = std::max(per_cu, 1);
  if (ctx->grid_per_cu > 0) per_cu = std::min(per_cu, ctx->grid_per_cu);  // glome_ctx_set_grid_per_cu: the caller knows what else runs
  else if (min_per_cu > 0) {  // sized by work: ~64 items per wave (~16 when nothing runs beside the launch), not below min_per_cu waves per CU
    const bool alone = !other_slots_busy(ctx);
    const long per_wave = alone ? 16L : 64L;
    // ... and a large scene's launch that is alone not below 12: one flagship frame takes 0.45 ms with 8 waves per CU, 0.40 with 12, 0.41 with
    // 16, 0.51 with 24; two frames want 16, four and more all 24 (profiles/r04_probes/lone_launch_grid.txt)
    if (alone && min_per_cu >= 8) min_per_cu = 12;
    long want = ((long)total_work + per_wave * cus - 1) / (per_wave * cus);
    per_cu = (int)std::min<long>(per_cu, std::max<long>(min_per_cu, want));
  }
  long g = (long)cus * per_cu;
  return (int)std::max<long>(1, std::min<long>(g, total_work));
}
// The floor of a work-sized grid: a scene with a small tree has cheap work items (tens of traversal steps), and a wave's
// fixed costs then dominate a short launch -- 3 waves per CU (S2, four 720x480 frames per launch: 0.024 ms per frame
// against 0.036 with 8); items of a large scene keep a wave busy for ~0.1 ms each and a short launch wants 8 (a rank's
// shard of the flagship frame: 0.039 ms per frame with 8, 0.048 with 4).
static int grid_floor(const glome_scene* s) { return s->tr.n_bih_nodes + s->tr.n_mesh_nodes < 4096 ? 3 : 8; }
// per wave slot: ovf_cap overflow entries + one more block of [3][64] words, the dump block of bih_walk_asm (LaneStack::dump)
static int ensure_overflow(glome_ctx* ctx, int grid, int waves_per_block, int ovf_cap) {
  size_t need = (size_t)grid * waves_per_block * (ovf_cap + 1) * 3 * 64 * sizeof(uint32_t);
  glome_ctx::Slot& sl = ctx->slot();
  if (need <= sl.ovf_bytes) return 0;
  if (sl.d_ovf) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(sl.d_ovf)); sl.d_ovf = nullptr; sl.ovf_bytes = 0; }
  HIPCHK(ctx, hipMalloc((void**)&sl.d_ovf, need));
  sl.ovf_bytes = need;
  return 0;
}
static int ensure_scratch(glome_ctx* ctx, size_t need) {
  glome_ctx::Slot& sl = ctx->slot();
  if (need <= sl.scratch_bytes) return 0;
  if (sl.d_scratch) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(sl.d_scratch)); sl.d_scratch = nullptr; sl.scratch_bytes = 0; }
  HIPCHK(ctx, hipMalloc((void**)&sl.d_scratch, need));
  sl.scratch_bytes = need;
  return 0;
}
// The ticket list of a flagship launch and, behind it, the two mask words per chunk of its cull pass: room for a launch of kMaxBatchFrames
// frames of the plan (`per_frame` items, chunked per frame), so a slot allocates once per frame size.
static size_t list_chunks(size_t items) { return (items + kQueueChunk - 1) / kQueueChunk + kMaxBatchFrames; }
static int ensure_list(glome_ctx* ctx, uint32_t per_frame) {
  glome_ctx::Slot& sl = ctx->slot();
  const size_t need = (size_t)per_frame * kMaxBatchFrames;
  if (need <= sl.list_items) return 0;
  if (sl.d_list) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(sl.d_list)); sl.d_list = nullptr; sl.list_items = 0; }
  HIPCHK(ctx, hipMalloc((void**)&sl.d_list, (need + 2 * list_chunks(need)) * sizeof(uint32_t)));
  sl.list_items = need;
  return 0;
}
// The device-side error word is sticky: kernels only ever OR into it, the counter reset leaves it alone, and it is read --
// and cleared -- where the host waits anyway (statistics, the host-buffer seams, glome_ctx_synchronize).  So a launch
// that nobody asked statistics of (the pipelined frame path) still reports a CSG-advance or frame-pool limit, at the
// next synchronize.  The caller has synchronised the slot's stream.
// the status and message of a non-zero error word (kErr* bits, rt_types.h)
static int device_error_status(glome_ctx* ctx, unsigned int e) {
  if (e & kErrNonUnit) {  // (only a trace launch sets it)
    ctx->err = "a ray direction is not unit length: set glome_trace_params.faithful to trace such rays (the reference's own traversal)";
    return GLOME_E_INVALID;
  }
  if (e & kErrBadVertex) {  // (only the updates set it; the word does not say which)
    ctx->err = "a mesh update met a vertex coordinate that is not finite: the scene's mesh is unspecified until a valid update"
               " (or a bih update, glome_scene_bih_update: then the bih is; or an Instance update, glome_scene_instance_update, met a matrix"
               " entry that is not finite or a bih item box that reaches infinity: then those Instances and the bih that holds them are; or a"
               " refit, glome_scene_bih_refit, met an item box or joined box that reaches infinity: then that bih and the bihs above it are;"
               " or a sphere bih update, glome_scene_sphere_bih_update, met a value that is not finite or a radius that is not positive: then"
               " that bih is); or an indexed bih update, glome_scene_bih_update_indexed_dev, met a vertex index outside [0, nv), read vertex 0 in"
               " its place, and left that bih unspecified; or an Instance update from a source, glome_scene_instance_update_from_dev, met an"
               " item that gives no finite matrix (a value that is not finite, a quaternion of length 0, a scale that is not positive, a"
               " singular forward matrix): then those Instances and the bih that holds them are unspecified";
    return GLOME_E_INVALID;
  }
  ctx->err = "device-side limit hit (traversal stack or CSG advance cap)";
  return GLOME_E_LIMIT;
}
static int poll_device_error(glome_ctx* ctx, glome_ctx::Slot& sl) {
  unsigned int e = 0;
  unsigned int* d = &sl.d_counters->error;
  HIPCHK(ctx, hipMemcpy(&e, d, sizeof(e), hipMemcpyDeviceToHost));
  if (!e) return 0;
  HIPCHK(ctx, hipMemset(d, 0, sizeof(e)));
  return device_error_status(ctx, e);
}
static int check_device_error(glome_ctx* ctx) { return poll_device_error(ctx, ctx->slot()); }

static int reset_counters(glome_ctx* ctx) {
  HIPCHK(ctx, hipMemsetAsync(ctx->slot().d_counters, 0, offsetof(DCounters, error), ctx->stream));  // not the sticky error word
  return 0;
}

// the (start, stop) events of a launch: the next pair of the pool while timing is on (every timing_stride-th launch; answers true), else the context's own
static bool launch_events(glome_ctx* ctx, hipEvent_t& e0, hipEvent_t& e1) {
  const bool pooled = ctx->timing && (ctx->timing_seen++ % ctx->timing_stride) == 0 && ctx->pool_used + 2 <= (int)ctx->pool.size();
  e0 = pooled ? ctx->pool[ctx->pool_used] : ctx->ev0; e1 = pooled ? ctx->pool[ctx->pool_used + 1] : ctx->ev1;
  if (pooled) ctx->pool_used += 2;
  return pooled;
}
// A light launch between a pair of the pool while timing is on: it takes part in glome_ctx_timing_begin / _end like a render launch.  (The
// caller returns before this for an empty launch: no pair is taken for it.)
template <class Launch> static int timed_launch(glome_ctx* ctx, Launch launch) {
  hipEvent_t e0, e1;
  const bool pooled = ctx->timing && launch_events(ctx, e0, e1);
  if (pooled) HIPCHK(ctx, hipEventRecord(e0, ctx->stream));
  launch();
  HIPCHK(ctx, hipGetLastError());
  if (pooled) HIPCHK(ctx, hipEventRecord(e1, ctx->stream));
  return 0;
}
// a launch nobody waits for: what it ORs into the slot's error word is reported at the next synchronize
static void mark_launched(glome_ctx* ctx) { ctx->slot().launched = true; ctx->slot().launched_on = ctx->stream; }
// the lights of a launch's arguments (DRenderArgs, DTraceArgs; the caller has refused nlights > kMaxLights)
template <class Args> static void fill_lights(Args& A, const glome_light* lights, int nlights) {
  for (int i = 0; i < nlights; i++) {
    memcpy(A.lights[i].pos, lights[i].pos, 12); memcpy(A.lights[i].color, lights[i].color, 12);
    A.lights[i].rad = lights[i].rad; A.lights[i].shadow = lights[i].shadow;
  }
  A.nlights = nlights;
}
// What a launch asked for statistics does once it is on the stream: the wait, the slot's counters into `stats` (n_tiles and n_pixels are
// the caller's), the time between the launch's events if it recorded them, and the error word read and cleared with the counters.
static int read_stats(glome_ctx* ctx, glome_stats* stats, bool timed, hipEvent_t ev_start, hipEvent_t ev_stop) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  DCounters c;
  HIPCHK(ctx, hipMemcpy(&c, ctx->slot().d_counters, sizeof(c), hipMemcpyDeviceToHost));
  stats->rays_primary = c.rays_primary; stats->rays_shadow = c.rays_shadow; stats->rays_secondary = c.rays_secondary;
  stats->bih_nodes = c.bih_nodes; stats->mesh_nodes = c.mesh_nodes; stats->prim_tests = c.prim_tests;
  if (timed) HIPCHK(ctx, hipEventElapsedTime(&stats->kernel_ms, ev_start, ev_stop));
  ctx->slot().launched = false;
  if (c.error) {
    HIPCHK(ctx, hipMemset(&ctx->slot().d_counters->error, 0, sizeof(unsigned int)));
    return device_error_status(ctx, c.error);
  }
  return 0;
}
// the instance instances.hpp chose (choose_render / choose_sampler), on the context's stream and slot (whose overflow workspace the caller has sized: ensure_overflow)
static int launch_chosen(glome_scene* s, const Choice& ch, InstanceKind kind, int grid, size_t lds, const DRenderArgs& A) {
  glome_ctx* ctx = s->ctx;
  hipStream_t st = ctx->stream;
  if (ch.generic) {
    if (kind == KIND_SAMPLER) { if (ch.generic_counts) launch_ss_generic(grid, st, A); else launch_ss_generic_lean(grid, st, A); }
    else { if (ch.generic_counts) launch_render_generic(grid, st, A); else launch_render_generic_lean(grid, st, A); }
  } else {
    const FlatLaunch L{grid, lds, st, s->tr.stack_cap, ctx->slot().d_ovf, s->ovf_cap};
    // (the choice rules only name listed instances -- instances.hpp choices_listed, asserted at compile time: a launcher that does not know the key is a broken build)
    if (kind == KIND_SAMPLER) { if (!launch_ss_flat(ch.key, L, A)) { ctx->err = "no sampler kernel instance for this scene class (build error)"; return GLOME_E_INVALID; } }
    else if (!launch_render_flat(ch.key, L, A)) { ctx->err = "no kernel instance for this scene class (build error)"; return GLOME_E_INVALID; }
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

static int render_impl(glome_scene* s, const glome_camera* cam, const glome_light* lights, int nlights, const glome_render_params* P,
                       float* rgbad_dev, uint32_t* packed_dev, glome_stats* stats, int dense, int nframes = 1, int64_t frame_stride = 0) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (!cam || (!rgbad_dev && !(dense != 1 && packed_dev)) || nlights < 0 || (nlights > 0 && !lights)) { ctx->err = "bad argument"; return GLOME_E_INVALID; }
  if (nlights > kMaxLights) { ctx->err = "too many lights"; return GLOME_E_LIMIT; }
  int rc = check_params(ctx, P);
  if (rc) return rc;
  if (P->mode != GLOME_MODE_TILE && P->mode != GLOME_MODE_SUBSAMPLE) { ctx->err = "unknown render mode"; return GLOME_E_INVALID; }
  if (P->mode == GLOME_MODE_SUBSAMPLE && P->blocksize > 65) { ctx->err = "GLOME_MODE_SUBSAMPLE supports tiles up to 65x65"; return GLOME_E_LIMIT; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  glome_ctx::TileTable* tt;
  // a whole renderTile frame in image layout: the pixels are independent and every tile is owned, so the tile size only
  // decides how the work is cut.  64x64 tiles are all 8x8 blocks -- no thin leftover strips (a 65x65 tile has 129
  // pixels in a column and a row, whose 64-pixel items are the least coherent and slowest of the frame)
  const bool whole = P->mode == GLOME_MODE_TILE && dense == 0 && P->tile_first == 0 && P->tile_stride == 1;
  if ((rc = get_tiles(ctx, P, P->tile_first, P->tile_stride, &tt, whole ? 64 : 0))) return rc;
  DRenderArgs A;
  memset(&A, 0, sizeof(A));
  A.S = s->dev;
  memcpy(&A.cam, cam, sizeof(DCamera));
  if (nframes < 1 || nframes > kMaxBatchFrames) { ctx->err = "a launch carries 1..32 frames"; return GLOME_E_LIMIT; }
  if (nframes > 1 && (frame_stride <= 0 || frame_stride > 0xffffffffll)) { ctx->err = "frame batches: positive frame stride"; return GLOME_E_INVALID; }
  for (int f = 1; f < nframes; f++) memcpy(&A.more_cams[f - 1], cam + f, sizeof(DCamera));
  A.nframes = nframes; A.frame_stride = nframes > 1 ? (uint32_t)frame_stride : 0u;
  fill_lights(A, lights, nlights);
  A.width = P->width; A.height = P->height; A.fog = P->fog; A.maxdepth = P->maxdepth;
  memcpy(A.thresholds, P->thresholds, 16);
  A.tiles = tt->dev; A.tile_lut = tt->lut; A.items = tt->items; A.ntiles = (int)tt->host.size(); A.total_waves = tt->total_waves;
  {
    float* ct = nullptr;
    if ((rc = get_coord_tables(ctx, P->width, P->height, &ct))) return rc;
    A.xc_tab = ct; A.yc_tab = ct + P->width;
  }
  {  // tickets per queue head: the launch's chunks dealt round-robin over the heads, the last round padded
    A.chunks_per_frame = (nframes > 1 && P->mode == GLOME_MODE_TILE) ? (A.total_waves + kQueueChunk - 1) / kQueueChunk : 0u;
    const uint32_t tickets = A.chunks_per_frame ? A.chunks_per_frame * kQueueChunk * (uint32_t)nframes : A.total_waves * (uint32_t)nframes, round = kQueueChunk * kQueueShards;
    A.shard_cap = ((tickets + round - 1) / round) * kQueueChunk;
  }
  // dense 0: full frame (rgbad and / or packed); 1: dense rgbad tile payload; 2: dense packed-pixel tile payload only
  A.out5 = dense == 2 ? nullptr : rgbad_dev; A.packed = dense == 1 ? nullptr : packed_dev; A.counters = ctx->slot().d_counters; A.dense = dense != 0;
  // a plain frame (no statistics wanted, renderTile mode) does not reset the counters -- the queue heads are put back by
  // the last wave of the launch before -- so the frame is a single packet on the stream
  const bool bare = !stats && P->mode == GLOME_MODE_TILE && !P->faithful && !P->count_work;
  if (!bare && (rc = reset_counters(ctx))) return rc;
  A.want_counters = (bare || (P->mode == GLOME_MODE_SUBSAMPLE && !stats)) ? 0 : 1;  // nobody reads them without `stats`
  hipEvent_t ev_start = ctx->ev0, ev_stop = ctx->ev1;
  if (A.ntiles > 0 && P->mode == GLOME_MODE_SUBSAMPLE) {
    // scratch: v (5 float planes over the owned pixels) | queue heads, one per 128-byte line, then the dry mask | one
    // line of pass counters per tile
    size_t npx = (size_t)tt->pixels;
    const size_t ctl_words = (size_t)(kSSHeads + 1) * kSSHeadStride + (size_t)A.ntiles * nframes * 8;
    if ((rc = ensure_scratch(ctx, npx * 5 * nframes * sizeof(float) + ctl_words * sizeof(unsigned int)))) return rc;
    A.scratch = ctx->slot().d_scratch;
    A.ss_cnt = (unsigned int*)(A.scratch + npx * 5 * nframes);
    A.ss_done = A.ss_cnt + (size_t)(kSSHeads + 1) * kSSHeadStride;
    A.ss_plane = (uint32_t)npx;
    A.blocksize = P->blocksize;
    // Region size by the frames of the launch: what hides a tile's chain of five dependent passes is other frames' tiles
    // (profiles/r02_f_ss_regions.log: one frame alone wants the small regions whatever its tile count)
    for (int pass = 1; pass <= 5; pass++) {
      int rw, rh;
      ss_region_shape(pass, nframes >= 8 ? 2 : (nframes >= 3 ? 1 : 0), rw, rh);
      // The generic tier's rays cost fifty times a flat-tier ray and its kernel runs eight waves per CU: parallelism is worth
      // more than shared compaction.  One block per region for a frame alone (GlomeView's default scene: 68.5 -> 37.0 ms), two
      // blocks in passes 3-5 of a batch (12.1 -> 9.1 ms per frame)
      if (s->dev.tier != 0) { rw = (nframes >= 3 && pass >= 3) ? 2 : 1; rh = 1; }
      // ... and once the interpreter's rays had become three times cheaper (round 3) a launch of twelve or more frames wants larger
      // regions in the later passes: 5.8 -> 5.1 ms per frame with 1x1, 2x1, 2x2, 2x2, 3x3 blocks (a launch of eight alone: 7.1 -> 10.2,
      // so those keep the rule above; profiles/r03_probes/generic_tier_sampler_regions.txt)
      if (s->dev.tier != 0 && nframes >= 12) { static const int8_t W[6] = {0, 1, 2, 2, 2, 3}, H[6] = {0, 1, 1, 2, 2, 3}; rw = W[pass]; rh = H[pass]; }
      A.ss_rw[pass] = (int8_t)rw; A.ss_rh[pass] = (int8_t)rh;
    }
    HIPCHK(ctx, hipMemsetAsync(A.ss_cnt, 0, ctl_words * sizeof(unsigned int), ctx->stream));
    launch_events(ctx, ev_start, ev_stop);
    HIPCHK(ctx, hipEventRecord(ev_start, ctx->stream));
    const Choice ch = choose_sampler(s->tr, P->faithful != 0, P->count_work != 0, P->maxdepth, P->tile_stride);
    const size_t lds = ch.generic ? 0 : flat_lds_bytes(s->tr.stack_cap, ch.two_rows);
    const uint32_t items = ss_plan(A).first[6] * kSSHeads;
    // (a wave that is not resident yet holds no item, so the items a running wave waits for are always with running waves)
    // (the sampler's items are long -- a region's contrast tests and one or more packet walks -- so the grid is sized for ~4 per wave)
    int tgrid = persistent_grid(ctx, lds, (uint32_t)std::min<uint64_t>((uint64_t)items * 16, 0x7fffffffu), waves_per_cu(ch), grid_floor(s));
    tgrid = (int)std::min<uint32_t>((uint32_t)tgrid, items);
    if (!ch.generic && (rc = ensure_overflow(ctx, tgrid, 1, s->ovf_cap))) return rc;
    if ((rc = launch_chosen(s, ch, KIND_SAMPLER, tgrid, lds, A))) return rc;
    HIPCHK(ctx, hipEventRecord(ev_stop, ctx->stream));
  } else if (A.ntiles > 0) {
    const uint32_t items = A.total_waves * (uint32_t)nframes;
    const Choice ch = choose_render(s->tr, P->faithful != 0, P->count_work != 0, P->maxdepth, P->tile_stride, items);
    const size_t lds = ch.generic ? 0 : flat_lds_bytes(s->tr.stack_cap, ch.two_rows);
    const int grid = persistent_grid(ctx, lds, items, waves_per_cu(ch), grid_floor(s));
    if (!ch.generic && (rc = ensure_overflow(ctx, grid, 1, s->ovf_cap))) return rc;
    if (ch.two_rows) {  // the flagship instance: its queue runs over the ticket list the cull pass leaves
      if (A.total_waves > (1u << kListFrameShift)) { ctx->err = "frame too large"; return GLOME_E_INVALID; }
      if ((rc = ensure_list(ctx, A.total_waves))) return rc;
      A.list = ctx->slot().d_list;
    }
    const bool pooled = launch_events(ctx, ev_start, ev_stop), timed = stats || pooled;
    if (timed) HIPCHK(ctx, hipEventRecord(ev_start, ctx->stream));
    if (ch.two_rows) {
      // one block per chunk of the launch's item order (padding chunks of the last round of heads hold nothing and are not visited);
      // a chunk lies in one frame, which the block reads once (cull_kernels.hpp chunk_position)
      if (nframes > 1 && !A.chunks_per_frame) { ctx->err = "a flagship launch of several frames is interleaved by chunks"; return GLOME_E_INVALID; }
      const uint32_t nchunks = A.chunks_per_frame ? A.chunks_per_frame * (uint32_t)nframes : (items + kQueueChunk - 1) / kQueueChunk;
      glome_ctx::Slot& sl = ctx->slot();
      hipLaunchKernelGGL(k_cull_items, dim3(nchunks), dim3(kCullThreads), 0, ctx->stream, A, sl.d_list, sl.d_list + sl.list_items, nchunks);
      HIPCHK(ctx, hipGetLastError());
      sl.cull_total = items;
    }
    if ((rc = launch_chosen(s, ch, KIND_RENDER, grid, lds, A))) return rc;
    if (timed) HIPCHK(ctx, hipEventRecord(ev_stop, ctx->stream));
  }
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->n_tiles = A.ntiles; stats->n_pixels = (int32_t)tt->pixels;
    return read_stats(ctx, stats, A.ntiles > 0, ev_start, ev_stop);
  }
  if (A.ntiles > 0) mark_launched(ctx);
  return 0;
}

int glome_render_dev(glome_scene* s, const glome_camera* cam, const glome_light* lights, int nlights, const glome_render_params* P,
                     float* rgbad_dev, uint32_t* packed_dev, glome_stats* stats) {
  return render_impl(s, cam, lights, nlights, P, rgbad_dev, packed_dev, stats, 0);
}
int glome_render_tiles_dev(glome_scene* s, const glome_camera* cam, const glome_light* lights, int nlights, const glome_render_params* P,
                           float* payload_dev, glome_stats* stats) {
  return render_impl(s, cam, lights, nlights, P, payload_dev, nullptr, stats, 1);
}
int glome_render_tiles_packed_dev(glome_scene* s, const glome_camera* cam, const glome_light* lights, int nlights, const glome_render_params* P,
                                  uint32_t* payload_dev, glome_stats* stats) {
  return render_impl(s, cam, lights, nlights, P, nullptr, payload_dev, stats, 2);
}

int glome_render_tiles_packed_batch_dev(glome_scene* s, const glome_camera* cams, int nframes, const glome_light* lights, int nlights,
                                        const glome_render_params* P, uint32_t* payload_dev, int64_t frame_stride_pixels, glome_stats* stats) {
  return render_impl(s, cams, lights, nlights, P, nullptr, payload_dev, stats, 2, nframes, frame_stride_pixels);
}
int glome_render_packed_batch_dev(glome_scene* s, const glome_camera* cams, int nframes, const glome_light* lights, int nlights,
                                  const glome_render_params* P, uint32_t* packed_dev, int64_t frame_stride_pixels, glome_stats* stats) {
  return render_impl(s, cams, lights, nlights, P, nullptr, packed_dev, stats, 0, nframes, frame_stride_pixels);
}

// ---- host-buffer forms: the caller's arrays staged through HBM ----
// in: a device copy of an input (h null: the allocation alone).  out: the device twin of an output, copied back by fetch(); null when h is
// null -- an output the caller does not want.  inout: both.  An allocation or a copy in that fails clears `ok`; an output that is not
// wanted does not.  Everything is freed on every exit.
struct Staging {
  struct Out { void* h; const void* d; size_t bytes; };
  std::vector<void*> bufs;
  std::vector<Out> outs;
  bool ok = true;
  Staging() = default;
  Staging(const Staging&) = delete;
  ~Staging() { for (void* p : bufs) (void)hipFree(p); }
  template <class T> T* in(const T* h, size_t n) {
    T* d = nullptr;
    if (hipMalloc((void**)&d, std::max<size_t>(1, n) * sizeof(T)) != hipSuccess) { ok = false; return nullptr; }
    bufs.push_back(d);
    if (h && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { ok = false; return nullptr; }
    return d;
  }
  template <class T> T* out(T* h, size_t n, bool copy_in = false) {
    T* d = h ? in<T>(copy_in ? h : nullptr, n) : nullptr;
    if (d) outs.push_back({h, d, n * sizeof(T)});
    return d;
  }
  template <class T> T* inout(T* h, size_t n) { return out(h, n, true); }
  // the streams of a ray batch, staged in this order (a braced list); tmax stays null where the call has none
  RayStream rays(const RayStream& h, size_t n) { return {in(h.ox, n), in(h.oy, n), in(h.oz, n), in(h.dx, n), in(h.dy, n), in(h.dz, n), h.tmax ? in(h.tmax, n) : nullptr}; }
  hipError_t fetch() const {
    for (const Out& o : outs)
      if (hipError_t e = hipMemcpy(o.h, o.d, o.bytes, hipMemcpyDeviceToHost)) return e;
    return hipSuccess;
  }
};
// The tail of every host form, its arguments checked and staged: the device form, the wait and the slot's error word where the device form
// has not seen to both itself (it has when it was given `stats`), the outputs back to the caller.
template <class Dev> static int run_staged(glome_ctx* ctx, const Staging& st, bool dev_waited, Dev dev) {
  if (!st.ok) { ctx->err = "staging allocation failed"; return GLOME_E_HIP; }
  if (int rc = dev()) return rc;
  if (!dev_waited) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = check_device_error(ctx)) return rc;
  }
  HIPCHK(ctx, st.fetch());
  return 0;
}

int glome_render(glome_scene* s, const glome_camera* cam, const glome_light* lights, int nlights, const glome_render_params* P, float* rgbad,
                 uint32_t* packed, glome_stats* stats) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  int rc = check_params(ctx, P);
  if (rc) return rc;
  if (!rgbad) { ctx->err = "null framebuffer"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t np = (size_t)P->width * P->height;
  Staging st;
  float* d5 = st.inout(rgbad, np * 5);  // tiles this call does not own keep the caller's values
  uint32_t* dp = st.inout(packed, np);
  glome_stats local;
  return run_staged(ctx, st, true, [&] { return glome_render_dev(s, cam, lights, nlights, P, d5, dp, stats ? stats : &local); });
}

// ---- per-ray seams ----
static int batch_grid(glome_ctx* ctx, size_t n, size_t lds) {
  size_t blocks = (n + 63) / 64;
  return (int)std::max<size_t>(1, std::min<size_t>(blocks, (size_t)persistent_grid(ctx, lds, 0x7fffffff) * 4));
}
// the flat tier's launch of a ray seam: LDS stack, grid, overflow workspace
static int flat_batch_launch(glome_scene* s, size_t n, FlatLaunch& L) {
  glome_ctx* ctx = s->ctx;
  const size_t lds = flat_lds_bytes(s->tr.stack_cap);
  const int grid = batch_grid(ctx, n, lds);
  if (int rc = ensure_overflow(ctx, grid, 1, s->ovf_cap)) return rc;
  L = FlatLaunch{grid, lds, ctx->stream, s->tr.stack_cap, ctx->slot().d_ovf, s->ovf_cap};
  return 0;
}
int glome_rayint_batch_dev(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                           const float* dz, const float* tmax, float* t, int32_t* prim, float* nx, float* ny, float* nz, int32_t* tex8) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (n == 0) return 0;
  if (!ox || !oy || !oz || !dx || !dy || !dz || !tmax) { ctx->err = "null ray stream"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  RayStream R{ox, oy, oz, dx, dy, dz, tmax};
  HitStream H{t, prim, nx, ny, nz, tex8};
  if (s->dev.tier == 0) {
    FlatLaunch L;
    if (int rc = flat_batch_launch(s, n, L)) return rc;
    launch_rayint_batch_flat(L, s->dev, n, R, H, ctx->slot().d_counters);
  } else {
    if (int rc = reset_counters(ctx)) return rc;
    launch_rayint_batch_generic(batch_grid(ctx, n, 0), ctx->stream, s->dev, n, R, H, ctx->slot().d_counters);
  }
  mark_launched(ctx);  // (a limit hit here is this call's to report, at the next synchronize)
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int glome_shadow_batch_dev(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                           const float* dz, const float* tmax, uint8_t* occluded) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (n == 0) return 0;
  if (!ox || !oy || !oz || !dx || !dy || !dz || !tmax || !occluded) { ctx->err = "null stream"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  RayStream R{ox, oy, oz, dx, dy, dz, tmax};
  if (s->dev.tier == 0) {
    FlatLaunch L;
    if (int rc = flat_batch_launch(s, n, L)) return rc;
    launch_shadow_batch_flat(L, s->dev, n, R, occluded, ctx->slot().d_counters);
  } else {
    if (int rc = reset_counters(ctx)) return rc;
    launch_shadow_batch_generic(batch_grid(ctx, n, 0), ctx->stream, s->dev, n, R, occluded, ctx->slot().d_counters);
  }
  mark_launched(ctx);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// the host-buffer forms (Staging, run_staged)
int glome_rayint_batch(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                       const float* dz, const float* tmax, float* t, int32_t* prim, float* nx, float* ny, float* nz, int32_t* tex8) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (n == 0) return 0;
  if (!ox || !oy || !oz || !dx || !dy || !dz || !tmax) { ctx->err = "null ray stream"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staging st;
  const RayStream R = st.rays({ox, oy, oz, dx, dy, dz, tmax}, n);
  const HitStream H{st.out(t, n), st.out(prim, n), st.out(nx, n), st.out(ny, n), st.out(nz, n), st.out(tex8, 8 * n)};
  return run_staged(ctx, st, false, [&] { return glome_rayint_batch_dev(s, n, R.ox, R.oy, R.oz, R.dx, R.dy, R.dz, R.tmax, H.t, H.prim, H.nx, H.ny, H.nz, H.tex8); });
}
int glome_shadow_batch(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                       const float* dz, const float* tmax, uint8_t* occluded) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (n == 0) return 0;
  if (!ox || !oy || !oz || !dx || !dy || !dz || !tmax || !occluded) { ctx->err = "null stream"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staging st;
  const RayStream R = st.rays({ox, oy, oz, dx, dy, dz, tmax}, n);
  uint8_t* docc = st.out(occluded, n);
  return run_staged(ctx, st, false, [&] { return glome_shadow_batch_dev(s, n, R.ox, R.oy, R.oz, R.dx, R.dy, R.dz, R.tmax, docc); });
}
int glome_inside_batch(glome_scene* s, size_t n, const float* px, const float* py, const float* pz, uint8_t* inside) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (n == 0) return 0;
  if (!px || !py || !pz || !inside) { ctx->err = "null stream"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staging st;
  float *dx = st.in(px, n), *dy = st.in(py, n), *dz = st.in(pz, n);
  uint8_t* din = st.out(inside, n);
  return run_staged(ctx, st, false, [&]() -> int {  // (the seam has no device-pointer form: its launch stands here)
    if (int rc = reset_counters(ctx)) return rc;
    launch_inside_batch(batch_grid(ctx, n, 0), ctx->stream, s->dev, n, dx, dy, dz, din, ctx->slot().d_counters);
    HIPCHK(ctx, hipGetLastError());
    return 0;
  });
}

// ---- updates of a committed scene: what the four updates share ----
// every slot of the context may have a launch in flight that reads the pools about to be written
static int quiesce(glome_ctx* ctx) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (auto& sl : ctx->slots)
    if (sl.launched_on && sl.launched_on != ctx->stream) (void)hipStreamSynchronize(sl.launched_on);
  (void)hipGetLastError();  // (a stream its owner has destroyed since must not be this call's error: other_slots_busy)
  return 0;
}
// What a blocking form does once it has quiesced and staged: its device form between the context's event pair, the wait, the error word.
template <class Dev> static int run_blocking(glome_ctx* ctx, float* gpu_ms, Dev dev) {
  if (gpu_ms) HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if (int rc = dev()) return rc;
  if (gpu_ms) HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (gpu_ms) HIPCHK(ctx, hipEventElapsedTime(gpu_ms, ctx->ev0, ctx->ev1));
  return check_device_error(ctx);
}
// The front half of a blocking host form that changes a committed scene.  check(): what both forms of the call refuse.  validate(): what
// the host form alone can see, the values in the caller's arrays.  stage(st) copies the arrays to the device through st.in and returns
// the device form as a callable, which run(dev) is given while the copies live.  Refusals keep this order: check, validation, device
// work.  empty: the call names nothing to change -- once it has passed the check and the validation it is complete.
template <class Check, class Validate, class Stage, class Run> static int staged_front(glome_scene* s, float* gpu_ms, Check check, Validate validate, Stage stage, Run run, bool empty = false) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (gpu_ms) *gpu_ms = 0;
  if (int rc = check()) return rc;
  if (int rc = validate()) return rc;
  if (empty) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = quiesce(ctx)) return rc;
  Staging st;
  auto dev = stage(st);
  if (!st.ok) { ctx->err = "staging allocation failed"; return GLOME_E_HIP; }
  return run(dev);
}
// The frame of the updates' blocking host forms: the front half, then the device form timed and waited for -- the copies stay outside the
// timed span, the device form runs inside it.
template <class Check, class Validate, class Stage> static int blocking_update(glome_scene* s, float* gpu_ms, Check check, Validate validate, Stage stage, bool empty = false) {
  return staged_front(s, gpu_ms, check, validate, stage, [&](auto dev) { return run_blocking(s->ctx, gpu_ms, dev); }, empty);
}
// One event pair per update while timing is on; with the update's split switch (GLOME_DEBUG_MESH_UPDATE_SPLIT,
// GLOME_DEBUG_BIH_UPDATE_SPLIT: tools/probe/*_update_rate.py) one per stage -- records, levels, bound.
struct UpdateSpan {
  glome_ctx* ctx;
  bool split;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  UpdateSpan(glome_ctx* c, const char* split_env) : ctx(c), split(split_env && getenv(split_env) != nullptr) {}
  hipError_t begin() { return ctx->timing && launch_events(ctx, e0, e1) ? hipEventRecord(e0, ctx->stream) : (e1 = nullptr, hipSuccess); }
  hipError_t end() { return e1 ? hipEventRecord(e1, ctx->stream) : hipSuccess; }
  hipError_t stage() {
    if (!split) return hipSuccess;
    const hipError_t e = end();
    return e != hipSuccess ? e : begin();
  }
};
// n lanes, 64 to a block, at most CUs * 128 blocks -- the kernels stride (upd::for_lanes); no launch for no lane
template <class K, class... Args> static void launch_lanes(glome_ctx* ctx, K kernel, uint32_t n, Args... args) {
  if (!n) return;
  const uint32_t max_items = (uint32_t)ctx->prop.multiProcessorCount * 32u * 4u;
  hipLaunchKernelGGL(kernel, dim3(std::min<uint32_t>((n + 63u) >> 6, max_items)), dim3(64), 0, ctx->stream, args...);
}
// an update's workspace, `words` float4, allocated at the object's first update and kept until glome_scene_release
static int ensure_ws(glome_scene* s, float4*& d_ws, size_t words) {
  if (d_ws) return 0;
  void* d = nullptr;
  HIPCHK(s->ctx, hipMalloc(&d, words * sizeof(float4)));
  s->allocs.push_back(d);
  d_ws = (float4*)d;
  return 0;
}
// the answer with the switch off or on (Flattener::mark_updatable, mark_nested), and the refusal's text
static int accepted(glome_scene* s, const char* what, const UpdateAnswer& plain, const NestedAnswer& nested) {
  const UpdateAnswer& A = s->nested_on ? nested : plain;
  if (!A.ok) { s->ctx->err = std::string(what) + " refused: " + A.why_not; return GLOME_E_INVALID; }
  return 0;
}
// The point sources of the updates (update_common.hpp): dense or indexed, fp64 or fp32.
template <class T> static upd::IndexedPts<T> indexed_pts(glome_ctx* ctx, const void* verts_dev, int nv, const int32_t* idx_dev) {
  return upd::IndexedPts<T>{(const T*)verts_dev, idx_dev, (uint32_t)nv, &ctx->slot().d_counters->error};
}
// The spheres' sources (sphere_bih_update_kernels.hpp) yield items; every other source yields points (update_common.hpp).  What an update
// launches for a source is picked by this alone.
template <class Src> constexpr bool kSphereSrc = std::is_same<Src, sphupd::SphPacked64>::value || std::is_same<Src, sphupd::SphSplit32>::value;
// The fp32 box over all points (all spheres) of a source into a header's two box words: partial boxes, then their fold from +-start
// (update_common.hpp).
template <class Src> static void launch_bound32(glome_ctx* ctx, Src src, uint32_t n, float4* part, float start, float4* hdr) {
  const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((n + upd::kBoundBlock - 1) / upd::kBoundBlock, (uint32_t)upd::kBoundMaxBlocks));
  if constexpr (kSphereSrc<Src>) {
    hipLaunchKernelGGL(sphupd::k_sph_bound<Src>, dim3(blocks), dim3(upd::kBoundBlock), 0, ctx->stream, src, n, part);
  } else {
    upd::DBoundArgs<Src> A;
    A.src = src; A.nv = n; A.part = part; A.error = &ctx->slot().d_counters->error;
    hipLaunchKernelGGL(upd::k_points_bound<Src>, dim3(blocks), dim3(upd::kBoundBlock), 0, ctx->stream, A);
  }
  hipLaunchKernelGGL(upd::k_bound_store, dim3(1), dim3(64), 0, ctx->stream, (const float4*)part, blocks, start, hdr);
}
// A bih's planes: a launch of k_bih_level per tree level, deepest first.  merged_off (the triangle bih alone, behind its switch): the
// device copy of level_off, and every run of two or more narrow levels goes to ONE block of k_bih_levels_merged instead.
static void launch_levels(glome_ctx* ctx, const bihupd::DLevelArgs& A, const std::vector<uint32_t>& level_off, const uint32_t* merged_off) {
  const size_t levels = level_off.empty() ? 0 : level_off.size() - 1;
  auto width = [&](size_t l) { return level_off[l + 1] - level_off[l]; };
  for (size_t l = 0; l < levels;) {
    size_t e = l;
    while (merged_off && e < levels && width(e) <= (uint32_t)bihupd::kMergeBlock) e++;
    if (e > l + 1) {  // a run of narrow levels: one block
      hipLaunchKernelGGL(bihupd::k_bih_levels_merged, dim3(1), dim3(bihupd::kMergeBlock), 0, ctx->stream, A, merged_off, (uint32_t)l, (uint32_t)e);
      l = e;
    } else {
      launch_lanes(ctx, bihupd::k_bih_level, width(l), A, level_off[l], width(l));
      l++;
    }
  }
}

// ---- objects under a bih, and the item bihs above them (item_bih_update_kernels.hpp) ----
// An updated object's fp64 bound into its row of the bounds table -- two launches on the current stream -- and the trees above it stale.
// `part`: the kernel that makes the partial boxes of the source (k_nest_points_part, k_nest_spheres_part).
template <class Src> static void nested_points_bound(glome_scene* s, int node, void (*part)(Src, uint32_t, double*), Src src, uint32_t n, double start, const std::vector<int>& above) {
  glome_ctx* ctx = s->ctx;
  const uint32_t blocks = std::min<uint32_t>((n + itemupd::kFoldBlock - 1) / itemupd::kFoldBlock, (uint32_t)itemupd::kPartMaxBlocks);
  if (blocks) hipLaunchKernelGGL(part, dim3(blocks), dim3(itemupd::kFoldBlock), 0, ctx->stream, src, n, s->d_live_part);
  hipLaunchKernelGGL(itemupd::k_nest_fold_store, dim3(1), dim3(itemupd::kFoldBlock), 0, ctx->stream, (const double*)s->d_live_part, blocks, start,
                     s->d_live + 6 * (size_t)s->live_slot.at(node), &ctx->slot().d_counters->error);
  s->stale.insert(above.begin(), above.end());
}
// An item bih's workspace, in float4 from its start: two words per record of the tree's span (plane-form rows), two per node slot, two
// per item (box-form rows), then the bound's partial boxes.
struct TreeWs {
  uint32_t n_items;
  size_t node, box, part, words;
  explicit TreeWs(const InstBihInfo& B)
      : n_items((uint32_t)B.kind.size()), node(2 * (size_t)B.rec_span), box(node + 2 * (size_t)B.n_slots), part(box + 2 * (size_t)n_items), words(part + 2 * (size_t)upd::kBoundMaxBlocks) {}
};
// A tree's workspace and tables, allocated and given the commit-time rows of all its items at the first update or refit that touches it
// (blocking calls: nothing has read them yet, and the launches that follow are ordered after the copies).
static int ensure_tree_ws(glome_scene* s, glome_scene::InstBih& m) {
  glome_ctx* ctx = s->ctx;
  if (m.d_ws) return 0;
  const InstBihInfo& B = m.info;
  const TreeWs W(B);
  const size_t n_items = W.n_items;
  std::vector<float4> init(W.words, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  float4* box = init.data() + W.box;
  for (size_t j = 0; j < n_items; j++) {
    const F4* r = &B.rows[4 * j];
    float4* plane = init.data() + 2 * (size_t)m.info.rec_off[j];
    plane[0] = make_float4(r[0].x, r[0].y, r[0].z, 0.0f); plane[1] = make_float4(r[1].x, r[1].y, r[1].z, 0.0f);
    box[2 * j] = make_float4(r[2].x, r[2].y, r[2].z, 0.0f); box[2 * j + 1] = make_float4(r[3].x, r[3].y, r[3].z, 0.0f);
  }
  std::vector<double> d64(30 * n_items, 0.0);  // box64, then the matrices
  std::copy(B.box64.begin(), B.box64.end(), d64.begin());
  std::vector<uint2> live;
  std::vector<uint32_t> item_live(n_items, itemupd::kNoLive);
  for (size_t j = 0; j < n_items; j++) {
    if (B.xf_at[j] >= 0) std::copy(B.live_xf.begin() + 24 * (ptrdiff_t)B.xf_at[j], B.live_xf.begin() + 24 * (ptrdiff_t)B.xf_at[j] + 24, d64.begin() + 6 * (ptrdiff_t)n_items + 24 * (ptrdiff_t)j);
    if (B.kind[j] != InstBihInfo::kDirectLive && B.kind[j] != InstBihInfo::kInstancedLive) continue;
    const uint32_t row = s->live_slot.at(B.live[j]);
    live.push_back(make_uint2((uint32_t)j, row | (B.kind[j] == InstBihInfo::kInstancedLive ? itemupd::kInstancedBit : 0u)));
    if (B.kind[j] == InstBihInfo::kInstancedLive) item_live[j] = row;
  }
  void *d = nullptr, *d2 = nullptr;
  HIPCHK(ctx, hipMalloc(&d, W.words * sizeof(float4)));
  s->allocs.push_back(d);
  HIPCHK(ctx, hipMemcpy(d, init.data(), W.words * sizeof(float4), hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMalloc(&d2, std::max<size_t>(1, d64.size()) * sizeof(double)));
  s->allocs.push_back(d2);
  if (!d64.empty()) HIPCHK(ctx, hipMemcpy(d2, d64.data(), d64.size() * sizeof(double), hipMemcpyHostToDevice));
  if ((!live.empty() && upload(s, live, &m.d_live_items)) || upload(s, item_live, &m.d_item_live)) return GLOME_E_HIP;
  m.d_box64 = (double*)d2; m.d_xf = (double*)d2 + 6 * n_items; m.n_live = (uint32_t)live.size();
  m.d_ws = (float4*)d;
  m.info.rows = {}; m.info.box64 = {}; m.info.live_xf = {};
  return 0;
}
// An item bih made again from its workspace rows, which the caller has brought up to date: the planes, a launch per tree level over the
// plane-form rows (the triangle bih's own kernel); the header's box, the fold of the box-form rows from box_empty; and -- fold64 -- the
// tree's own fp64 bound, the join of its items' boxes from box_empty, into its row of the bounds table.
static void refit_item_tree(glome_scene* s, int bih_id, glome_scene::InstBih& m, bool fold64) {
  glome_ctx* ctx = s->ctx;
  const InstBihInfo& B = m.info;
  const TreeWs W(B);
  bihupd::DLevelArgs A;
  A.nodes = m.d_levels; A.bihnodes = (float4*)s->dev.bihnodes; A.pknodes = nullptr;
  A.ws_tri = m.d_ws; A.ws_node = m.d_ws + W.node; A.first_rec = B.first_rec; A.first_slot = B.first_slot;
  launch_levels(ctx, A, B.level_off, nullptr);
  float4* part = m.d_ws + W.part;
  const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((W.n_items + 63u) >> 6, (uint32_t)upd::kBoundMaxBlocks));
  hipLaunchKernelGGL(itemupd::k_inst_box_fold, dim3(blocks), dim3(64), 0, ctx->stream, (const float4*)(m.d_ws + W.box), W.n_items, part);
  hipLaunchKernelGGL(upd::k_bound_store, dim3(1), dim3(64), 0, ctx->stream, (const float4*)part, blocks, (float)kInfinity, (float4*)s->dev.bihhdr + 3 * (size_t)B.hdr);
  if (fold64)
    hipLaunchKernelGGL(itemupd::k_nest_fold_store, dim3(1), dim3(itemupd::kFoldBlock), 0, ctx->stream, (const double*)m.d_box64, W.n_items, kInfinity,
                       s->d_live + 6 * (size_t)s->live_slot.at(bih_id), &ctx->slot().d_counters->error);
}

// ---- new vertices for a committed Mesh (mesh_update_kernels.hpp) ----
// what both forms refuse before anything is launched; *out = the mesh's tables
static int mesh_update_check(glome_scene* s, int32_t mesh_id, const void* verts, int nv, const void* norms, int nn, glome_scene::MeshUpd** out) {
  glome_ctx* ctx = s->ctx;
  auto it = s->meshes.find(mesh_id);
  if (it == s->meshes.end()) { ctx->err = "mesh update: node " + std::to_string(mesh_id) + " is not a mesh of this scene"; return GLOME_E_INVALID; }
  const MeshUpdateInfo& U = it->second.info;
  if (nv != U.nv) { ctx->err = "mesh update: the mesh has " + std::to_string(U.nv) + " vertices, not " + std::to_string(nv); return GLOME_E_INVALID; }
  if (nn != U.nn) { ctx->err = "mesh update: the mesh has " + std::to_string(U.nn) + " normals, not " + std::to_string(nn); return GLOME_E_INVALID; }
  if ((nv && !verts) || (nn && !norms)) { ctx->err = "mesh update: null vertex / normal array"; return GLOME_E_INVALID; }
  if (int rc = accepted(s, "mesh update", U.plain, U.nested)) return rc;
  *out = &it->second;
  return 0;
}
// the device form, for arrays of T: the launches, on the current stream
template <class T> static int mesh_update_dev(glome_scene* s, int32_t mesh_id, const T* verts_p, int nv, const T* norms_p, int nn) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  glome_scene::MeshUpd* m = nullptr;
  if (int rc = mesh_update_check(s, mesh_id, verts_p, nv, norms_p, nn, &m)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  using Src = upd::DensePts<T>;
  const Src verts_dev{verts_p}, norms_dev{norms_p};
  const MeshUpdateInfo& U = m->info;
  if (int rc = ensure_ws(s, m->d_ws, 2 * ((size_t)U.n_tris + upd::kBoundMaxBlocks))) return rc;  // a box per record, and the bound's partial boxes
  UpdateSpan span(ctx, "GLOME_DEBUG_MESH_UPDATE_SPLIT");
  HIPCHK(ctx, span.begin());
  {
    meshupd::DTrisArgs<Src> A;
    A.verts = verts_dev; A.norms = norms_dev; A.rows = (const int4*)m->d_rows;
    A.mtris = (float4*)s->dev.mtris + 3 * (size_t)U.first_tri; A.trinorms = (float4*)s->dev.trinorms; A.ws = m->d_ws; A.n = U.n_tris;
    launch_lanes(ctx, meshupd::k_mesh_tris<Src>, U.n_tris, A);
  }
  HIPCHK(ctx, span.stage());
  for (size_t l = 0; l + 1 < U.level_off.size(); l++) {
    meshupd::DLevelArgs A;
    A.nodes = m->d_levels + U.level_off[l]; A.n = U.level_off[l + 1] - U.level_off[l];
    A.meshnodes = (float4*)s->dev.meshnodes; A.mtrimeta = (const uint4*)s->dev.mtrimeta; A.ws = m->d_ws; A.first_tri = U.first_tri;
    launch_lanes(ctx, meshupd::k_mesh_refit_level, A.n, A);
  }
  HIPCHK(ctx, span.stage());
  // box_of_points starts from a vertex (real infinities); a mesh of no vertices keeps box_empty
  if (nv > 0) launch_bound32(ctx, verts_dev, (uint32_t)nv, m->d_ws + 2 * (size_t)U.n_tris, __builtin_huge_valf(), (float4*)s->dev.meshhdr + 2 * (size_t)U.hdr);
  if (s->nested_on && !U.nested.above.empty()) nested_points_bound(s, mesh_id, itemupd::k_nest_points_part<Src>, verts_dev, (uint32_t)nv, nv > 0 ? __builtin_huge_val() : kInfinity, U.nested.above);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, span.end());
  mark_launched(ctx);  // (a vertex that is not finite is reported at the next synchronize)
  return 0;
}
// the host form, for arrays of T: staged as they are
template <class T> static int mesh_update_host(glome_scene* s, int32_t mesh_id, const T* verts, int nv, const T* norms, int nn, float* gpu_ms) {
  glome_scene::MeshUpd* m = nullptr;
  return blocking_update(
      s, gpu_ms, [&] { return mesh_update_check(s, mesh_id, verts, nv, norms, nn, &m); },
      [&]() -> int {
        for (size_t k = 0; k < 3 * (size_t)nv; k++) if (!std::isfinite(verts[k])) { s->ctx->err = "mesh update: a vertex coordinate is not finite"; return GLOME_E_INVALID; }
        for (size_t k = 0; k < 3 * (size_t)nn; k++) if (!std::isfinite(norms[k])) { s->ctx->err = "mesh update: a normal coordinate is not finite"; return GLOME_E_INVALID; }
        return 0;
      },
      [&](Staging& st) {
        T* dv = st.in(verts, 3 * (size_t)nv);
        T* dn = nn ? st.in(norms, 3 * (size_t)nn) : nullptr;
        return [=] { return mesh_update_dev<T>(s, mesh_id, dv, nv, dn, nn); };
      });
}
int glome_scene_mesh_update_dev(glome_scene* s, int32_t mesh_id, const double* verts_dev, int nv, const double* norms_dev, int nn) {
  return mesh_update_dev<double>(s, mesh_id, verts_dev, nv, norms_dev, nn);
}
int glome_scene_mesh_update(glome_scene* s, int32_t mesh_id, const double* verts, int nv, const double* norms, int nn, float* gpu_ms) {
  return mesh_update_host<double>(s, mesh_id, verts, nv, norms, nn, gpu_ms);
}
int glome_scene_mesh_update_f32_dev(glome_scene* s, int32_t mesh_id, const float* verts_dev, int nv, const float* norms_dev, int nn) {
  return mesh_update_dev<float>(s, mesh_id, verts_dev, nv, norms_dev, nn);
}
int glome_scene_mesh_update_f32(glome_scene* s, int32_t mesh_id, const float* verts, int nv, const float* norms, int nn, float* gpu_ms) {
  return mesh_update_host<float>(s, mesh_id, verts, nv, norms, nn, gpu_ms);
}

// ---- new items for a committed leaf bih: triangles (bih_update_kernels.hpp) or spheres (sphere_bih_update_kernels.hpp) ----
// One path serves both classes: the record (LeafBihUpdateInfo) says what differs in the tables, the source type what differs in the kernels.
// The source forms, the two actions on them and the entry points follow the rebuild, below.
// A refusal of one of these calls: the call's name, then why (texts are made by a refusal alone)
static int refuse(glome_ctx* ctx, const char* what, const std::string& why, int rc = GLOME_E_INVALID) {
  ctx->err = std::string(what) + ": " + why;
  return rc;
}
// What both forms of every call refuse before anything is launched; *out = the bih's tables.  cls: the class the call is for; what: the
// call's name in its texts ("bih update", "sphere bih rebuild"); `items`: the array there is one entry per item of.
static int leaf_bih_update_check(glome_scene* s, uint32_t cls, const char* what, int32_t bih_id, const void* items, int n, glome_scene::LeafBihUpd** out) {
  auto refuse = [&](const std::string& why) { return ::refuse(s->ctx, what, why); };
  const char* word = cls == BC_SPHERE ? "sphere" : "triangle";
  auto it = s->leaf_bihs.find(bih_id);
  if (it == s->leaf_bihs.end() || it->second.info.cls != cls) return refuse("node " + std::to_string(bih_id) + " is not a bih of plain " + word + "s of this scene");
  const LeafBihUpdateInfo& U = it->second.info;
  if (n != U.n_items) return refuse("the bih has " + std::to_string(U.n_items) + " items, not " + std::to_string(n));
  if (n && !items) return refuse(std::string("null ") + word + " array");
  if (int rc = accepted(s, what, U.plain, U.nested)) return rc;
  *out = &it->second;
  return 0;
}
// an update's workspace, in words of one float4: a box, two words, per record and per node slot, and the bound's partial boxes
static size_t leaf_ws_words(uint32_t n_recs, uint32_t n_slots) { return 2 * ((size_t)n_recs + n_slots + upd::kBoundMaxBlocks); }
// The launches of an update the checks have accepted, on the current stream.  `src` yields the n items: a point source their 3 n vertices
// (update_common.hpp), a sphere source their spheres (sphere_bih_update_kernels.hpp); every kernel that reads them is its instance for
// that source.  The source's kind picks the records kernel and the two partial-box kernels; all else is one sequence.
template <class Src> static int leaf_bih_update_launch(glome_scene* s, int32_t bih_id, glome_scene::LeafBihUpd* m, Src src, int n) {
  glome_ctx* ctx = s->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const LeafBihUpdateInfo& U = m->info;
  const uint32_t n_src = kSphereSrc<Src> ? (uint32_t)n : 3u * (uint32_t)n;  // what the bounds fold: spheres, or vertices
  const size_t ws_words = leaf_ws_words(U.n_recs, U.n_slots);
  if (int rc = ensure_ws(s, m->d_ws, ws_words)) return rc;
  if (!m->ws_words) m->ws_words = ws_words;  // (what it was allocated with: a rebuild may ask for more)
  // The levels run a launch each: the merged launch of the narrow levels (k_bih_levels_merged) stays behind GLOME_DEBUG_BIH_UPDATE_MERGED
  // until tools/probe/bih_update_rate.py has shown on the hardware that it wins beyond the run-to-run spread
  const bool merged = getenv("GLOME_DEBUG_BIH_UPDATE_MERGED") != nullptr;
  UpdateSpan span(ctx, "GLOME_DEBUG_BIH_UPDATE_SPLIT");
  HIPCHK(ctx, span.begin());
  if constexpr (kSphereSrc<Src>) {
    sphupd::DItemsArgs<Src> A;
    A.src = src; A.rows = m->d_rows; A.spheres = (float4*)s->dev.spheres + (size_t)U.first_prim; A.ws = m->d_ws; A.n = U.n_recs;
    A.error = &ctx->slot().d_counters->error;
    launch_lanes(ctx, sphupd::k_sph_items<Src>, U.n_recs, A);
  } else {
    bihupd::DTrisArgs<Src> A;
    A.src = src; A.rows = (const uint2*)m->d_rows; A.tris = (float4*)s->dev.tris + 3 * (size_t)U.first_prim; A.tripairs = (float*)s->dev.tripairs;
    A.ws = m->d_ws; A.n = U.n_recs;
    launch_lanes(ctx, bihupd::k_bih_tris<Src>, U.n_recs, A);
  }
  HIPCHK(ctx, span.stage());
  {
    bihupd::DLevelArgs A;
    A.nodes = m->d_levels; A.bihnodes = (float4*)s->dev.bihnodes; A.pknodes = U.pk ? (float4*)s->dev.pknodes : nullptr;  // (a sphere tree's walk reads bihnodes alone)
    A.ws_tri = m->d_ws; A.ws_node = m->d_ws + 2 * (size_t)U.n_recs; A.first_rec = U.first_rec; A.first_slot = U.first_slot;
    launch_levels(ctx, A, U.level_off, merged ? m->d_level_off : nullptr);
  }
  HIPCHK(ctx, span.stage());
  // the join of the items' boxes, from box_empty: in fp32 into the header, in fp64 into the bounds table
  launch_bound32(ctx, src, n_src, m->d_ws + 2 * ((size_t)U.n_recs + U.n_slots), (float)kInfinity, (float4*)s->dev.bihhdr + 3 * (size_t)U.hdr);
  if (s->nested_on && !U.nested.above.empty()) {
    if constexpr (kSphereSrc<Src>) nested_points_bound(s, bih_id, sphupd::k_nest_spheres_part<Src>, src, n_src, kInfinity, U.nested.above);
    else nested_points_bound(s, bih_id, itemupd::k_nest_points_part<Src>, src, n_src, kInfinity, U.nested.above);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, span.end());
  mark_launched(ctx);  // (a value that is not finite, a radius that is not positive or an index outside the vertex array is reported at the next synchronize)
  return 0;
}

// ---- a committed leaf bih re-split: the tree built again in place from new items (bih_rebuild_kernels.hpp, bih_build_device.hpp) ----
// glome_sb_bih_set_triangles / _set_spheres, glome_sb_bih_resplit and a commit, without the commit.  boxes and tree write scratch alone;
// plan, the layout function of the commit (flatten.hpp leaf_bih_layout) against the tree's own segments, reads the scene and writes
// nothing; every refusal is found in those three, so a refused call leaves the scene as it was.  apply cannot refuse, and a HIP call
// of its that fails leaves the scene's record with the old tree.  Not asynchronous in either form: a level costs a synchronisation,
// tree and apply wait.
// a pool of the scene's moved to an allocation with room for `cap` elements of T, its first `used` copied (the caller has quiesced: no
// launch reads the old one, which is freed at once, so two copies of one pool are alive at a time).  The pool holds what it held: the
// scene's record, which does not know the new room yet, still describes it.
template <class T> static int pool_grow(glome_scene* s, const T*& d, size_t used, size_t cap) {
  T* nd = nullptr;
  HIPCHK(s->ctx, hipMalloc((void**)&nd, cap * sizeof(T)));
  if (hipMemset(nd, 0, cap * sizeof(T)) != hipSuccess || hipMemcpy(nd, d, used * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) {
    (void)hipFree(nd);
    s->ctx->err = "rebuild: copying a pool failed";
    return GLOME_E_HIP;
  }
  adopt(s, d, nd);
  return 0;
}
// What commit derives from the trees' depths (Flattener::run, scene_caps), derived again from the depths as they now stand
struct DepthRules { int max_bih_depth = 0, max_sphere_bih_depth = 0; SceneCaps caps; };
static DepthRules depth_rules(const glome_scene* s, uint32_t hdr, int depth) {
  DepthRules R;
  for (size_t h = 0; h < s->hdr_depth.size(); h++) {
    const int d = h == hdr ? depth : s->hdr_depth[h];
    R.max_bih_depth = std::max(R.max_bih_depth, d);
    if (s->hdr_packet_service[h]) R.max_sphere_bih_depth = std::max(R.max_sphere_bih_depth, d);
  }
  struct View { uint32_t tier; int max_sphere_bih_depth, max_bih_depth, max_mesh_depth; std::vector<U4> entries, recs; std::vector<F4> bihhdr; } V;
  V.tier = s->dev.tier; V.max_sphere_bih_depth = R.max_sphere_bih_depth; V.max_bih_depth = R.max_bih_depth; V.max_mesh_depth = s->max_mesh_depth;
  R.caps = scene_caps(V);  // (no entries: the class mask, which no depth changes, stays the commit's)
  return R;
}
static unsigned long long host_dkey(double x) {  // bihdev::dkey
  unsigned long long b; memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// boxes: the items' fp64 boxes from the update's source, their join and the validation flag, in scratch
struct RebuildScratch {
  struct RootWords { unsigned long long key[6]; double bound[6]; unsigned int flag, pad; };
  double* box = nullptr;
  RootWords* root = nullptr;
  RootWords rw;  // the host's copy: what goes up, then what comes back
  ~RebuildScratch() { (void)hipFree(box); (void)hipFree(root); }
  // room for n boxes; the root words at the empty box, no flag
  int init(glome_ctx* ctx, int n) {
    HIPCHK(ctx, hipMalloc((void**)&box, sizeof(double) * 6 * (size_t)n));
    HIPCHK(ctx, hipMalloc((void**)&root, sizeof(RootWords)));
    for (int a = 0; a < 3; a++) { rw.key[a] = host_dkey(kInfinity); rw.key[3 + a] = host_dkey(-kInfinity); rw.bound[a] = rw.bound[3 + a] = 0; }
    rw.flag = rw.pad = 0;
    HIPCHK(ctx, hipMemcpyAsync(root, &rw, sizeof(rw), hipMemcpyHostToDevice, ctx->stream));
    return 0;
  }
};
template <class Src> static int rebuild_boxes(glome_ctx* ctx, Src src, int n, const char* what, RebuildScratch& sc, Box3& bb) {
  constexpr bool SPH = kSphereSrc<Src>;
  RebuildScratch::RootWords& rw = sc.rw;
  hipLaunchKernelGGL((bihrebuild::k_item_boxes<Src, SPH>), dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, ctx->stream, src, (uint32_t)n, sc.box, sc.root->key, &sc.root->flag);
  hipLaunchKernelGGL(bihrebuild::k_root_box, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long*)sc.root->key, sc.root->bound);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(&rw, sc.root, sizeof(rw), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (rw.flag & bihrebuild::kBadIndex) return refuse(ctx, what, "an item has a vertex index outside the vertex array");
  if (rw.flag) return refuse(ctx, what, SPH ? "a value is not finite or a radius is not positive" : "a vertex coordinate is not finite");
  bb = Box3{{rw.bound[0], rw.bound[1], rw.bound[2]}, {rw.bound[3], rw.bound[4], rw.bound[5]}};
  if (bb.lo.x == -kInfinity || bb.lo.y == -kInfinity || bb.lo.z == -kInfinity || bb.hi.x == kInfinity || bb.hi.y == kInfinity || bb.hi.z == kInfinity) {
    ctx->err = "bih: infinite bounding box";  // (the constructor's message)
    return GLOME_E_SCENE;
  }
  return 0;
}
// tree: the device builder's level loop over the boxes; the topology and the final object order back.  Items by their index in the update order.
static int rebuild_tree(glome_ctx* ctx, double* box, int n, const Box3& bb, BihTree& T) {
  std::vector<bihdev::DevNode> none;
  std::vector<bihdev::PackedNode> packed;
  std::vector<int> order;
  std::string err;
  if (const int rc = bihdev::levels_dev<false>(box, n, bb, ctx->stream, err, nullptr, none, order, &packed)) { ctx->err = err; return bihdev_status(rc); }
  T.bb = bb;
  bihdev::to_preorder(packed, T,
    [&](BihTree::Node& tn, const bihdev::PackedNode& d) {
      tn.leaf = true; tn.lsplit = tn.rsplit = 0; tn.axis = -1; tn.left = tn.right = -1;
      for (int k = 0; k < d.count; k++) tn.items.push_back(order[(size_t)(d.start + k)]);
    },
    [&](BihTree::Node& tn, const bihdev::PackedNode& d) { tn.leaf = false; tn.lsplit = tn.rsplit = 0; tn.axis = d.axis; tn.left = tn.right = -1; });
  return 0;
}
// plan: what the scene will hold once the tree stands in it.  Where its node segment and its pair segment start -- the tree's own, or,
// for a tree that has outgrown one, a new one at the pool's end --, the pools' entries in use and allocated after that (allocated: the
// scene's own figure while the pool has the room), what the tree's segments hold, the commit's layout against them, and what commit
// derives from the depths.  Every refusal that is not the boxes' or the builder's is made here, of a scene that is not written to; no
// device call.
struct RebuildPlan {
  uint32_t base = 0, slot_cap = 0, pair_cap = 0;
  uint64_t pair_word = 0;
  size_t nodes_used = 0, nodes_cap = 0, pairs_used = 0, pairs_cap = 0;
  LeafBihLayout L;
  DepthRules R;
};
static int rebuild_plan(const glome_scene* s, int32_t bih_id, const glome_scene::LeafBihUpd& m, const BihTree& T, const char* what, RebuildPlan& P) {
  glome_ctx* ctx = s->ctx;
  const LeafBihUpdateInfo& U = m.info;
  if (U.cls == BC_TRI && !U.pk) return refuse(ctx, what, "bih " + std::to_string(bih_id) + " was committed without the packet walk's node form and cannot be rebuilt", GLOME_E_LIMIT);
  std::vector<uint32_t> ident((size_t)U.n_items);
  for (size_t k = 0; k < ident.size(); k++) ident[k] = (uint32_t)k;
  P.base = U.first_slot; P.pair_word = U.first_pair_word; P.nodes_used = s->bihnodes_used; P.pairs_used = s->tripairs_used;
  {
    std::vector<uint32_t> slot;
    const uint32_t need = std::max<uint32_t>(bih_slots(T, slot), 1u);
    uint64_t pairs = 0;
    if (U.cls == BC_TRI) for (const BihTree::Node& bn : T.nodes) pairs += (bn.items.size() + 1) / 2;
    if (need > m.slot_cap) { P.base = (uint32_t)((s->bihnodes_used + 3u) & ~(size_t)3u); P.nodes_used = (size_t)P.base + need; }
    if (pairs > m.pair_cap) { P.pair_word = (s->tripairs_used + 15u) & ~(uint64_t)15u; P.pairs_used = (size_t)(P.pair_word + pairs * kPairWords); }
    if (P.nodes_used >= (1ull << 27) || (uint64_t)P.pairs_used * 4 >= (1ull << 31))
      return refuse(ctx, what, "the rebuilt tree's segments would lie beyond what a reference of the packet walk can address", GLOME_E_LIMIT);
  }
  P.nodes_cap = P.nodes_used > s->bihnodes_cap ? P.nodes_used + P.nodes_used / 4 : s->bihnodes_cap;
  P.pairs_cap = P.pairs_used > s->tripairs_cap ? P.pairs_used + P.pairs_used / 4 : s->tripairs_cap;
  LeafBihLayout& L = P.L;
  try { L = leaf_bih_layout(T, U.cls, ident, P.base, U.first_rec, U.first_prim, P.pair_word); }
  catch (const limit_error& e) { return refuse(ctx, what, e.what(), GLOME_E_LIMIT); }
  if (U.pk && !L.pk) return refuse(ctx, what, "the rebuilt tree would lose the packet walk's node form", GLOME_E_LIMIT);
  if (L.n_recs != U.n_recs) return refuse(ctx, what, "internal: the rebuilt tree holds another number of records", GLOME_E_HIP);
  P.slot_cap = P.base != U.first_slot ? std::max<uint32_t>(L.n_slots, 1u) : m.slot_cap;  // (an outgrown segment is abandoned)
  P.pair_cap = P.pair_word != U.first_pair_word ? L.n_pair_recs : m.pair_cap;
  P.R = depth_rules(s, U.hdr, T.depth);
  if (s->dev.tier == 0 && P.R.max_bih_depth > kFlatStack)
    return refuse(ctx, what, "the rebuilt tree is " + std::to_string(T.depth) + " levels deep, deeper than the flat tier's stack (" + std::to_string(kFlatStack) + "): a commit would take the generic tier", GLOME_E_LIMIT);
  return 0;
}
// apply: the plan carried out.  Every allocation first -- each pool a segment has outgrown moved to a larger one (pool_grow: it holds
// what it held), a fresh table for each that lacks the room --, then the uploads, then the scene's record and what commit derives from
// the depths and the pools' sizes, in one block that no call that can fail interrupts: a failure before it returns with the record, and
// the tables it points to, still the old tree's.
static int rebuild_apply(glome_scene* s, glome_scene::LeafBihUpd* m, const RebuildPlan& P) {
  glome_ctx* ctx = s->ctx;
  DScene& D = s->dev;
  LeafBihUpdateInfo& U = m->info;
  const LeafBihLayout& L = P.L;
  if (P.nodes_cap > s->bihnodes_cap) {
    if (int rc = pool_grow(s, D.bihnodes, s->bihnodes_used, P.nodes_cap)) return rc;
    if (int rc = pool_grow(s, D.pknodes, s->bihnodes_used, P.nodes_cap)) return rc;
  }
  if (P.pairs_cap > s->tripairs_cap)
    if (int rc = pool_grow(s, D.tripairs, s->tripairs_used, P.pairs_cap)) return rc;
  LeafTables tables(*m, L.rows, L.level_nodes, L.level_off);
  if (int rc = tables.room(ctx)) return rc;
  // the node words in both pools (planes zero: the values stage makes them), the records in the new leaf order, the pair records' count
  // and index words; the update's tables; the header's ref[0] and words 2 and 3
  {
    const uint32_t n_slots = std::max<uint32_t>(L.n_slots, 1u);
    std::vector<F4> nodes(n_slots), pk(n_slots, F4{0, 0, 0, 0});
    for (uint32_t q = 0; q < n_slots; q++) {
      nodes[q] = F4{0.0f, 0.0f, as_float_bits(L.node_zw[2 * (size_t)q]), as_float_bits(L.node_zw[2 * (size_t)q + 1])};
      if (L.pk) pk[q] = F4{0.0f, 0.0f, as_float_bits(L.pk_zw[2 * (size_t)q]), as_float_bits(L.pk_zw[2 * (size_t)q + 1])};
    }
    HIPCHK(ctx, hipMemcpy((F4*)D.bihnodes + P.base, nodes.data(), nodes.size() * sizeof(F4), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy((F4*)D.pknodes + P.base, pk.data(), pk.size() * sizeof(F4), hipMemcpyHostToDevice));
    std::vector<U4> recs(L.n_recs);
    for (uint32_t j = 0; j < L.n_recs; j++) { recs[j] = m->item_recs[L.rows[(size_t)j * U.row_words]]; recs[j].y = U.first_prim + j; }
    if (!recs.empty()) HIPCHK(ctx, hipMemcpy((U4*)D.recs + U.first_rec, recs.data(), recs.size() * sizeof(U4), hipMemcpyHostToDevice));
    if (L.n_pair_recs) {
      std::vector<float> pairs((size_t)L.n_pair_recs * kPairWords, 0.0f);
      for (uint32_t q = 0; q < L.n_pair_recs; q++) { pairs[(size_t)q * kPairWords + 18] = as_float_bits(L.pair_words[2 * (size_t)q]); pairs[(size_t)q * kPairWords + 19] = as_float_bits(L.pair_words[2 * (size_t)q + 1]); }
      HIPCHK(ctx, hipMemcpy((float*)D.tripairs + P.pair_word, pairs.data(), pairs.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (int rc = tables.fill(ctx)) return rc;
    F4* hdr = (F4*)D.bihhdr + 3 * (size_t)U.hdr;
    HIPCHK(ctx, hipMemcpy(&hdr[0].w, &L.ref[0], 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(&hdr[2], L.hdr2, 16, hipMemcpyHostToDevice));
  }
  // the record: the pools and tables, the tree's segments, the update's figures, the workspace when the tree has outgrown it (two words
  // per record and per slot: the next update makes a larger one), and everything commit derives from the trees' depths and the pool's size
  if (P.nodes_cap > s->bihnodes_cap) D.pknodes_bytes = (uint32_t)(P.nodes_cap * sizeof(F4));
  tables.take(s);
  s->bihnodes_used = P.nodes_used; s->bihnodes_cap = P.nodes_cap; s->tripairs_used = P.pairs_used; s->tripairs_cap = P.pairs_cap;
  m->slot_cap = P.slot_cap; m->pair_cap = P.pair_cap;
  U.first_slot = P.base; U.n_slots = L.n_slots; U.first_pair_word = P.pair_word; U.n_pair_recs = L.n_pair_recs; U.pk = L.pk; U.depth = L.depth;
  U.level_off = L.level_off;
  if (m->d_ws && leaf_ws_words(U.n_recs, U.n_slots) > m->ws_words) { drop_alloc(s, m->d_ws); m->d_ws = nullptr; m->ws_words = 0; }
  s->hdr_depth[U.hdr] = L.depth;
  s->info.max_bih_depth = P.R.max_bih_depth; s->info.n_bih_nodes = (int64_t)s->bihnodes_used;
  s->tr.stack_cap = P.R.caps.stack_cap; s->tr.n_bih_nodes = (int64_t)s->bihnodes_used; s->ovf_cap = P.R.caps.ovf_cap;
  D.pk_generic_cap = getenv("GLOME_DEBUG_NO_GENERIC_PACKETS") ? 0 : P.R.caps.pk_generic_cap;
  return 0;
}
// The driver: the five stages, the wall clock between them (glome_scene_bih_rebuild_stages), the context's event pair around the device work
template <class Src> static int leaf_bih_rebuild(glome_scene* s, int32_t bih_id, glome_scene::LeafBihUpd* m, Src src, int n, const char* what, float* gpu_ms) {
  glome_ctx* ctx = s->ctx;
  using clock = std::chrono::steady_clock;
  if (gpu_ms) *gpu_ms = 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = quiesce(ctx)) return rc;
  if (n == 0) return 0;
  clock::time_point t[6];
  RebuildScratch sc;
  Box3 bb;
  BihTree T;
  RebuildPlan P;
  t[0] = clock::now();
  if (int rc = sc.init(ctx, n)) return rc;
  if (gpu_ms) HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if (int rc = rebuild_boxes(ctx, src, n, what, sc, bb)) return rc;
  t[1] = clock::now();
  if (int rc = rebuild_tree(ctx, sc.box, n, bb, T)) return rc;
  t[2] = clock::now();
  if (int rc = rebuild_plan(s, bih_id, *m, T, what, P)) return rc;
  t[3] = clock::now();
  if (int rc = rebuild_apply(s, m, P)) return rc;
  t[4] = clock::now();
  if (int rc = leaf_bih_update_launch(s, bih_id, m, src, n)) return rc;  // values: records, pair values, planes, the box, the nested bound -- the update itself, on the same source
  if (gpu_ms) HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (gpu_ms) HIPCHK(ctx, hipEventElapsedTime(gpu_ms, ctx->ev0, ctx->ev1));
  t[5] = clock::now();
  for (int k = 0; k < 5; k++) s->rebuild_stage_ms[k] = std::chrono::duration<double, std::milli>(t[k + 1] - t[k]).count();
  return check_device_error(ctx);
}
int glome_scene_bih_rebuild_stages(const glome_scene* s, double out5[5]) {
  if (!s || !out5) return GLOME_E_INVALID;
  std::copy(s->rebuild_stage_ms, s->rebuild_stage_ms + 5, out5);
  return 0;
}

// ---- the leaf bih calls: four source forms, two actions ----
// A form says in what arrays a call is given its n items: its class; items(), the array there is one entry per item of; check(), what
// both forms of a call refuse beyond leaf_bih_update_check; validate(), what the host form alone can see, the values in the caller's
// arrays; stage(), the form over device copies of the arrays; visit(), the source its kernels read (update_common.hpp,
// sphere_bih_update_kernels.hpp).  Every text takes the call's name.
template <class T> static bool all_finite(const T* v, size_t n) {
  for (size_t k = 0; k < n; k++) if (!std::isfinite(v[k])) return false;
  return true;
}
// triangles, nine values of T each
template <class T> struct DenseTris {
  static constexpr uint32_t cls = BC_TRI;
  const T* pts9; int n;
  const void* items() const { return pts9; }
  int check(glome_ctx*, const char*) const { return 0; }
  int validate(glome_ctx* ctx, const char* what) const { return all_finite(pts9, 9 * (size_t)n) ? 0 : refuse(ctx, what, "a vertex coordinate is not finite"); }
  DenseTris stage(Staging& st) const { return {st.in(pts9, 9 * (size_t)n), n}; }  // (staged as it is)
  template <class F> int visit(glome_ctx*, F f) const { return f(upd::DensePts<T>{pts9}); }
};
// triangles whose vertices are verts[3 * idx3[3 k + c] ..]: a vertex array of `dtype` and an index table, as a simulation holds a mesh
struct IndexedTris {
  static constexpr uint32_t cls = BC_TRI;
  const void* verts; int32_t dtype; int nv; const int32_t* idx3; int n;
  const void* items() const { return idx3; }
  int check(glome_ctx* ctx, const char* what) const {
    if (dtype != GLOME_F64 && dtype != GLOME_F32) return refuse(ctx, what, "dtype " + std::to_string(dtype) + " is neither GLOME_F64 nor GLOME_F32");
    if (nv < 0 || (nv && !verts)) return refuse(ctx, what, "null vertex array");
    if (n > 0 && nv == 0) return refuse(ctx, what, std::to_string(n) + " items index an array of no vertices");
    return 0;
  }
  int validate(glome_ctx* ctx, const char* what) const {
    for (size_t k = 0; k < 3 * (size_t)n; k++) {  // only referenced vertices count: an unreferenced one may be anything
      const int32_t i = idx3[k];
      if (i < 0 || i >= nv) return refuse(ctx, what, "item " + std::to_string(k / 3) + " has vertex index " + std::to_string(i) + ", outside [0, " + std::to_string(nv) + ")");
      if (!(dtype == GLOME_F32 ? all_finite((const float*)verts + 3 * (size_t)i, 3) : all_finite((const double*)verts + 3 * (size_t)i, 3)))
        return refuse(ctx, what, "a vertex coordinate is not finite (vertex " + std::to_string(i) + ", of item " + std::to_string(k / 3) + ")");
    }
    return 0;
  }
  IndexedTris stage(Staging& st) const {  // the caller's arrays as they are: no widened, gathered copy
    const size_t vbytes = 3 * (size_t)nv * (dtype == GLOME_F32 ? sizeof(float) : sizeof(double));
    const char* dv = st.in((const char*)verts, vbytes);
    return {dv, dtype, nv, st.in(idx3, 3 * (size_t)n), n};
  }
  template <class F> int visit(glome_ctx* ctx, F f) const {
    if (dtype == GLOME_F32) return f(indexed_pts<float>(ctx, verts, nv, idx3));
    return f(indexed_pts<double>(ctx, verts, nv, idx3));
  }
};
// what a host form refuses of n spheres' radii, every value having been found finite: the first that is not positive.  radius(k): item k's
template <class Radius> static int positive_radii(glome_ctx* ctx, const char* what, int n, Radius radius) {
  for (size_t k = 0; k < (size_t)n; k++) if (!(radius(k) > 0)) return refuse(ctx, what, "radius of item " + std::to_string(k) + " is not positive");
  return 0;
}
// spheres, fp64 cx cy cz r interleaved
struct PackedSpheres {
  static constexpr uint32_t cls = BC_SPHERE;
  const double* c3r; int n;
  const void* items() const { return c3r; }
  int check(glome_ctx*, const char*) const { return 0; }
  int validate(glome_ctx* ctx, const char* what) const {
    if (!all_finite(c3r, 4 * (size_t)n)) return refuse(ctx, what, "a value is not finite");
    return positive_radii(ctx, what, n, [&](size_t k) { return c3r[4 * k + 3]; });
  }
  PackedSpheres stage(Staging& st) const { return {st.in(c3r, 4 * (size_t)n), n}; }
  template <class F> int visit(glome_ctx*, F f) const { return f(sphupd::SphPacked64{c3r}); }
};
// spheres, fp32 in two streams: centres [n, 3] and radii [n]
struct SplitSpheres {
  static constexpr uint32_t cls = BC_SPHERE;
  const float* centres3; const float* radii; int n;
  const void* items() const { return centres3; }
  int check(glome_ctx* ctx, const char* what) const { return n && !radii ? refuse(ctx, what, "null radius array") : 0; }
  int validate(glome_ctx* ctx, const char* what) const {
    if (!all_finite(centres3, 3 * (size_t)n) || !all_finite(radii, (size_t)n)) return refuse(ctx, what, "a value is not finite");
    return positive_radii(ctx, what, n, [&](size_t k) { return radii[k]; });
  }
  SplitSpheres stage(Staging& st) const { return {st.in(centres3, 3 * (size_t)n), st.in(radii, (size_t)n), n}; }
  template <class F> int visit(glome_ctx*, F f) const { return f(sphupd::SphSplit32{centres3, radii}); }
};
// The actions.  refit: the values made again on the tree as it stands (leaf_bih_update_launch), asynchronous in the device form, timed by
// the event pair and waited for in the host form.  rebuild: the tree first (leaf_bih_rebuild), which times and waits itself in both forms.
enum LeafAct { kRefit, kRebuild };
static const char* leaf_what(uint32_t cls, LeafAct act) {
  return cls == BC_SPHERE ? (act == kRebuild ? "sphere bih rebuild" : "sphere bih update") : (act == kRebuild ? "bih rebuild" : "bih update");
}
template <class Form> static int leaf_form_check(glome_scene* s, const char* what, int32_t bih_id, const Form& f, glome_scene::LeafBihUpd** out) {
  if (int rc = leaf_bih_update_check(s, Form::cls, what, bih_id, f.items(), f.n, out)) return rc;
  return f.check(s->ctx, what);
}
// the device form: the checks, then the action on the caller's device arrays
template <LeafAct A, class Form> static int leaf_bih_dev(glome_scene* s, int32_t bih_id, const Form& f, float* gpu_ms = nullptr) {
  if (!s) return GLOME_E_INVALID;
  const char* what = leaf_what(Form::cls, A);
  glome_scene::LeafBihUpd* m = nullptr;
  if (int rc = leaf_form_check(s, what, bih_id, f, &m)) return rc;
  return f.visit(s->ctx, [&](auto src) {
    if constexpr (A == kRebuild) return leaf_bih_rebuild(s, bih_id, m, src, f.n, what, gpu_ms);
    else return leaf_bih_update_launch(s, bih_id, m, src, f.n);
  });
}
// the host form: the checks, the values in the caller's arrays, then the arrays staged as they are and the device form
template <LeafAct A, class Form> static int leaf_bih_host(glome_scene* s, int32_t bih_id, const Form& f, float* gpu_ms) {
  const char* what = leaf_what(Form::cls, A);
  glome_scene::LeafBihUpd* m = nullptr;
  return staged_front(
      s, gpu_ms, [&] { return leaf_form_check(s, what, bih_id, f, &m); }, [&] { return f.validate(s->ctx, what); },
      [&](Staging& st) {
        const Form d = f.stage(st);
        return [=] { return leaf_bih_dev<A>(s, bih_id, d, gpu_ms); };
      },
      [&](auto dev) { return A == kRebuild ? dev() : run_blocking(s->ctx, gpu_ms, dev); });
}
int glome_scene_bih_update_dev(glome_scene* s, int32_t bih_id, const double* pts9_dev, int n) { return leaf_bih_dev<kRefit>(s, bih_id, DenseTris<double>{pts9_dev, n}); }
int glome_scene_bih_update(glome_scene* s, int32_t bih_id, const double* pts9, int n, float* gpu_ms) { return leaf_bih_host<kRefit>(s, bih_id, DenseTris<double>{pts9, n}, gpu_ms); }
int glome_scene_bih_update_f32_dev(glome_scene* s, int32_t bih_id, const float* pts9_dev, int n) { return leaf_bih_dev<kRefit>(s, bih_id, DenseTris<float>{pts9_dev, n}); }
int glome_scene_bih_update_f32(glome_scene* s, int32_t bih_id, const float* pts9, int n, float* gpu_ms) { return leaf_bih_host<kRefit>(s, bih_id, DenseTris<float>{pts9, n}, gpu_ms); }
int glome_scene_bih_update_indexed_dev(glome_scene* s, int32_t bih_id, const void* verts_dev, int32_t dtype, int nv, const int32_t* idx3_dev, int n) {
  return leaf_bih_dev<kRefit>(s, bih_id, IndexedTris{verts_dev, dtype, nv, idx3_dev, n});
}
int glome_scene_bih_update_indexed(glome_scene* s, int32_t bih_id, const void* verts, int32_t dtype, int nv, const int32_t* idx3, int n, float* gpu_ms) {
  return leaf_bih_host<kRefit>(s, bih_id, IndexedTris{verts, dtype, nv, idx3, n}, gpu_ms);
}
int glome_scene_sphere_bih_update_dev(glome_scene* s, int32_t bih_id, const double* c3r_dev, int n) { return leaf_bih_dev<kRefit>(s, bih_id, PackedSpheres{c3r_dev, n}); }
int glome_scene_sphere_bih_update(glome_scene* s, int32_t bih_id, const double* c3r, int n, float* gpu_ms) { return leaf_bih_host<kRefit>(s, bih_id, PackedSpheres{c3r, n}, gpu_ms); }
int glome_scene_sphere_bih_update_f32_dev(glome_scene* s, int32_t bih_id, const float* centres3_dev, const float* radii_dev, int n) {
  return leaf_bih_dev<kRefit>(s, bih_id, SplitSpheres{centres3_dev, radii_dev, n});
}
int glome_scene_sphere_bih_update_f32(glome_scene* s, int32_t bih_id, const float* centres3, const float* radii, int n, float* gpu_ms) {
  return leaf_bih_host<kRefit>(s, bih_id, SplitSpheres{centres3, radii, n}, gpu_ms);
}
int glome_scene_bih_rebuild_dev(glome_scene* s, int32_t bih_id, const double* pts9_dev, int n, float* gpu_ms) { return leaf_bih_dev<kRebuild>(s, bih_id, DenseTris<double>{pts9_dev, n}, gpu_ms); }
int glome_scene_bih_rebuild(glome_scene* s, int32_t bih_id, const double* pts9, int n, float* gpu_ms) { return leaf_bih_host<kRebuild>(s, bih_id, DenseTris<double>{pts9, n}, gpu_ms); }
int glome_scene_bih_rebuild_indexed_dev(glome_scene* s, int32_t bih_id, const void* verts_dev, int32_t dtype, int nv, const int32_t* idx3_dev, int n, float* gpu_ms) {
  return leaf_bih_dev<kRebuild>(s, bih_id, IndexedTris{verts_dev, dtype, nv, idx3_dev, n}, gpu_ms);
}
int glome_scene_bih_rebuild_indexed(glome_scene* s, int32_t bih_id, const void* verts, int32_t dtype, int nv, const int32_t* idx3, int n, float* gpu_ms) {
  return leaf_bih_host<kRebuild>(s, bih_id, IndexedTris{verts, dtype, nv, idx3, n}, gpu_ms);
}
int glome_scene_sphere_bih_rebuild_dev(glome_scene* s, int32_t bih_id, const double* c3r_dev, int n, float* gpu_ms) { return leaf_bih_dev<kRebuild>(s, bih_id, PackedSpheres{c3r_dev, n}, gpu_ms); }
int glome_scene_sphere_bih_rebuild(glome_scene* s, int32_t bih_id, const double* c3r, int n, float* gpu_ms) { return leaf_bih_host<kRebuild>(s, bih_id, PackedSpheres{c3r, n}, gpu_ms); }
// slots, pair records, records, depth of the tree as it stands, then what its node segment and its pair segment hold
int glome_scene_bih_layout(const glome_scene* s, int32_t bih_id, int64_t out6[6]) {
  if (!s || !out6) return GLOME_E_INVALID;
  auto it = s->leaf_bihs.find(bih_id);
  if (it == s->leaf_bihs.end()) { s->ctx->err = "bih layout: node " + std::to_string(bih_id) + " is not a bih of plain triangles or plain spheres of this scene"; return GLOME_E_INVALID; }
  const LeafBihUpdateInfo& U = it->second.info;
  out6[0] = U.n_slots; out6[1] = U.n_pair_recs; out6[2] = U.n_recs; out6[3] = U.depth; out6[4] = it->second.slot_cap; out6[5] = it->second.pair_cap;
  return 0;
}

// ---- new matrices for committed Instances (item_bih_update_kernels.hpp) ----
// what both forms refuse before anything is launched; out[k] = the tables of ids[k]
static int instance_update_check(glome_scene* s, const int32_t* ids, const void* xfms, int n, std::vector<const InstanceUpdateInfo*>& out) {
  glome_ctx* ctx = s->ctx;
  if (n < 0 || (n && (!ids || !xfms))) { ctx->err = "instance update: bad count or null array"; return GLOME_E_INVALID; }
  out.clear();
  for (int k = 0; k < n; k++) {
    auto it = s->insts.find(ids[k]);
    if (it == s->insts.end()) { ctx->err = "instance update: node " + std::to_string(ids[k]) + " is not an Instance of this scene"; return GLOME_E_INVALID; }
    if (int rc = accepted(s, "instance update", it->second.plain, it->second.nested)) return rc;
    out.push_back(&it->second);
  }
  std::vector<int32_t> sorted(ids, ids + n);
  std::sort(sorted.begin(), sorted.end());
  auto dup = std::adjacent_find(sorted.begin(), sorted.end());
  if (dup != sorted.end()) { ctx->err = "instance update: node " + std::to_string(*dup) + " is named more than once"; return GLOME_E_INVALID; }
  return 0;
}
// The launches of an accepted update of n > 0 Instances U, on the current stream, their matrices 24 doubles each at xfms_dev.  first():
// what the call enqueues inside its event pair before its kernels -- nothing, or the conversion that fills xfms_dev.
template <class First> static int instance_update_launch(glome_scene* s, const std::vector<const InstanceUpdateInfo*>& U, const double* xfms_dev, int n, First first) {
  glome_ctx* ctx = s->ctx;
  hipStream_t st = ctx->stream;
  // this call's rows: (matrix, xfm slot) of every slot, then per bih (matrix, item) of its named items
  std::vector<uint2> rows;
  std::map<int, std::vector<uint2>> per_bih;
  for (int k = 0; k < n; k++) {
    for (uint32_t slot : U[(size_t)k]->slots) rows.push_back(make_uint2((uint32_t)k, slot));
    if (U[(size_t)k]->bih >= 0) per_bih[U[(size_t)k]->bih].push_back(make_uint2((uint32_t)k, U[(size_t)k]->item));
  }
  const uint32_t n_xfm = (uint32_t)rows.size();
  for (auto& pb : per_bih) rows.insert(rows.end(), pb.second.begin(), pb.second.end());
  if (rows.size() > s->inst_rows_cap) {
    if (s->d_inst_rows) { HIPCHK(ctx, hipStreamSynchronize(st)); HIPCHK(ctx, hipFree(s->d_inst_rows)); s->d_inst_rows = nullptr; s->inst_rows_cap = 0; }
    HIPCHK(ctx, hipMalloc((void**)&s->d_inst_rows, rows.size() * sizeof(uint2)));
    s->inst_rows_cap = rows.size();
  }
  glome_scene::RowStage& stage = s->inst_stage[s->inst_stage_next];
  s->inst_stage_next = (s->inst_stage_next + 1) % 4;
  if (stage.pending) { HIPCHK(ctx, hipEventSynchronize(stage.ev)); stage.pending = false; }
  if (rows.size() > stage.cap) {
    if (stage.h) { HIPCHK(ctx, hipHostFree(stage.h)); stage.h = nullptr; stage.cap = 0; }
    HIPCHK(ctx, hipHostMalloc((void**)&stage.h, rows.size() * sizeof(uint2), hipHostMallocDefault));
    stage.cap = rows.size();
  }
  if (!stage.ev) HIPCHK(ctx, hipEventCreateWithFlags(&stage.ev, hipEventDisableTiming));
  std::copy(rows.begin(), rows.end(), stage.h);
  // the workspaces of the bihs this call refits, allocated and given the commit-time rows of all their items at their first update
  for (auto& pb : per_bih) if (int rc = ensure_tree_ws(s, s->ibihs.at(pb.first))) return rc;
  UpdateSpan span(ctx, nullptr);
  HIPCHK(ctx, span.begin());
  first();
  HIPCHK(ctx, hipMemcpyAsync(s->d_inst_rows, stage.h, rows.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipEventRecord(stage.ev, st));
  stage.pending = true;
  unsigned int* err = &ctx->slot().d_counters->error;
  {
    itemupd::DXfmArgs A;
    A.xfms = xfms_dev; A.rows = s->d_inst_rows; A.pool = (float4*)s->dev.xfms; A.n = n_xfm; A.error = err;
    launch_lanes(ctx, itemupd::k_inst_xfm, n_xfm, A);
  }
  uint32_t at = n_xfm;
  for (auto& pb : per_bih) {
    glome_scene::InstBih& m = s->ibihs.at(pb.first);
    const TreeWs W(m.info);
    const uint32_t n_named = (uint32_t)pb.second.size();
    // A tree whose items hang on objects that move keeps its matrices and fp64 boxes ALWAYS, switch on or off, from its first update:
    // a later refit reads an instanced item's matrix from the tree's table, whenever the Instance was last named.  So does any tree
    // while the switch is on (its own fp64 bound feeds the tree above).  k_nest_inst_named<true> takes a live child's bound from the
    // bounds table once that exists, and the commit's before: until the switch has been on no object under a bih can have moved.
    // Every other update runs the instance without the tables (item_bih_update_kernels.hpp: why both exist).
    const bool nested = m.n_live || (s->d_live && s->nested_on);
    itemupd::DNamedArgs A;
    A.xfms = xfms_dev; A.rows = s->d_inst_rows + at; A.child_bounds = m.d_bounds; A.item_live = m.d_item_live; A.bounds = s->d_live; A.xf = m.d_xf; A.rec_off = m.d_rec_off;
    A.ws_plane = m.d_ws; A.ws_box = m.d_ws + W.box; A.box64 = m.d_box64; A.n = n_named; A.error = err;
    launch_lanes(ctx, nested ? itemupd::k_nest_inst_named<true> : itemupd::k_nest_inst_named<false>, n_named, A);
    at += n_named;
    refit_item_tree(s, pb.first, m, nested && s->d_live);  // (the tree's own fp64 bound: the join of its items' boxes from box_empty)
  }
  if (s->nested_on)  // the update has refitted the tree that holds the Instance: the trees above that one are stale
    for (const InstanceUpdateInfo* u : U) for (int a : u->nested.above) if (a != u->bih) s->stale.insert(a);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, span.end());
  mark_launched(ctx);  // (a matrix entry that is not finite is reported at the next synchronize)
  return 0;
}
int glome_scene_instance_update_dev(glome_scene* s, const int32_t* ids, const double* xfms_dev, int n) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  std::vector<const InstanceUpdateInfo*> U;
  if (int rc = instance_update_check(s, ids, xfms_dev, n, U)) return rc;
  if (n == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return instance_update_launch(s, U, xfms_dev, n, [] {});
}
// what the host forms check of the matrix m (24 doubles) they would give Instance `id`, whose tables are u: 0, or the refusal
static int instance_matrix_check(glome_scene* s, int32_t id, const InstanceUpdateInfo* u, const double* m) {
  glome_ctx* ctx = s->ctx;
  for (int q = 0; q < 24; q++) if (!std::isfinite(m[q])) { ctx->err = "instance update: a matrix entry of node " + std::to_string(id) + " is not finite"; return GLOME_E_INVALID; }
  Xf x;
  for (int q = 0; q < 12; q++) { x.f.m[q] = m[q]; x.i.m[q] = m[12 + q]; }
  try { xf_check(x); } catch (const scene_error& e) { ctx->err = "instance update: node " + std::to_string(id) + ": " + e.what(); return GLOME_E_INVALID; }
  if (u->bih < 0) return 0;
  // the item's new box, as `bound` makes it: `bih` refuses one that reaches the reference's infinity
  const double* cb = &s->ibihs.at(u->bih).info.child_bound[6 * (size_t)u->item];
  D3 pts[8];
  int q = 0;
  for (double px : {cb[0], cb[3]}) for (double py : {cb[1], cb[4]}) for (double pz : {cb[2], cb[5]}) pts[q++] = xf_point(x, D3{px, py, pz});
  const Box3 b = box_of_points(pts, 8);
  if (b.lo.x == -kInfinity || b.lo.y == -kInfinity || b.lo.z == -kInfinity || b.hi.x == kInfinity || b.hi.y == kInfinity || b.hi.z == kInfinity) {
    ctx->err = "instance update: node " + std::to_string(id) + " in bih " + std::to_string(u->bih) + ": bih: infinite bounding box";
    return GLOME_E_SCENE;
  }
  return 0;
}
int glome_scene_instance_update(glome_scene* s, const int32_t* ids, const double* xfms, int n, float* gpu_ms) {
  std::vector<const InstanceUpdateInfo*> U;
  auto validate = [&]() -> int {
    for (int k = 0; k < n; k++) if (int rc = instance_matrix_check(s, ids[k], U[(size_t)k], xfms + 24 * (size_t)k)) return rc;
    return 0;
  };
  return blocking_update(s, gpu_ms, [&] { return instance_update_check(s, ids, xfms, n, U); }, validate, [&](Staging& st) {
    double* dx = st.in(xfms, 24 * (size_t)n);
    return [=] { return glome_scene_instance_update_dev(s, ids, dx, n); };
  }, n == 0);
}

// ---- the same from a matrix source: pairs, forward matrices or poses, fp64 or fp32, strided, after a base (xfm_sources.hpp) ----
size_t glome_xfm_source_size(void) { return sizeof(glome_xfm_source); }
static_assert((int)GLOME_XFM_PAIR == xfm::kPair && (int)GLOME_XFM_FORWARD == xfm::kForward && (int)GLOME_XFM_POSE == xfm::kPose, "the header's forms are the kernels' (xfm_sources.hpp)");
// what both forms refuse of the source before anything is launched, once instance_update_check has passed; *stride = elements per item
static int xfm_source_check(glome_scene* s, const glome_xfm_source* src, int n, int64_t* stride) {
  glome_ctx* ctx = s->ctx;
  auto refuse = [&](const std::string& why) { ctx->err = "instance update: " + why; return GLOME_E_INVALID; };
  *stride = 0;
  if (n == 0) return 0;
  if (!src || !src->data) return refuse("bad count or null array");  // (instance_update_check's words for its own null array)
  const int w = xfm::width_of(src->form);
  if (!w) return refuse("form " + std::to_string(src->form) + " is none of GLOME_XFM_PAIR, GLOME_XFM_FORWARD, GLOME_XFM_POSE");
  if (src->dtype != GLOME_F64 && src->dtype != GLOME_F32) return refuse("dtype " + std::to_string(src->dtype) + " is neither GLOME_F64 nor GLOME_F32");
  if (src->stride < 0) return refuse("stride " + std::to_string(src->stride) + " is negative");
  if (src->stride != 0 && src->stride < w) return refuse("stride " + std::to_string(src->stride) + " is less than the form's " + std::to_string(w) + " values");
  *stride = src->stride ? src->stride : w;
  return 0;
}
template <class T, int FORM> static void launch_xfm_convert(glome_scene* s, const glome_xfm_source& src, int64_t stride, int n) {
  using Src = itemupd::XfmSrc<T, FORM>;
  itemupd::DConvertArgs<Src> A;
  A.src = Src{(const T*)src.data, src.base, stride};
  A.table = s->d_xfm_table; A.n = (uint32_t)n; A.error = &s->ctx->slot().d_counters->error;
  launch_lanes(s->ctx, itemupd::k_xfm_convert<Src>, (uint32_t)n, A);
}
int glome_scene_instance_update_from_dev(glome_scene* s, const int32_t* ids, const glome_xfm_source* src_in, int n) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  std::vector<const InstanceUpdateInfo*> U;
  // (the array instance_update_check asks for: a null source is a null array)
  if (int rc = instance_update_check(s, ids, src_in ? src_in->data : nullptr, n, U)) return rc;
  int64_t stride = 0;
  if (int rc = xfm_source_check(s, src_in, n, &stride)) return rc;
  if (n == 0) return 0;
  const glome_xfm_source src = *src_in;
  // the layout the existing call takes: that call, and no table
  if (src.form == GLOME_XFM_PAIR && src.dtype == GLOME_F64 && stride == 24 && !src.base) return glome_scene_instance_update_dev(s, ids, (const double*)src.data, n);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if ((size_t)n > s->xfm_table_cap) {  // (grown like d_inst_rows: the kernels of an earlier call may still read the old one)
    if (s->d_xfm_table) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(s->d_xfm_table)); s->d_xfm_table = nullptr; s->xfm_table_cap = 0; }
    HIPCHK(ctx, hipMalloc((void**)&s->d_xfm_table, 24 * (size_t)n * sizeof(double)));
    s->xfm_table_cap = (size_t)n;
  }
  return instance_update_launch(s, U, s->d_xfm_table, n, [&] {
    const bool f32 = src.dtype == GLOME_F32;
    if (src.form == GLOME_XFM_POSE) f32 ? launch_xfm_convert<float, xfm::kPose>(s, src, stride, n) : launch_xfm_convert<double, xfm::kPose>(s, src, stride, n);
    else if (src.form == GLOME_XFM_FORWARD) f32 ? launch_xfm_convert<float, xfm::kForward>(s, src, stride, n) : launch_xfm_convert<double, xfm::kForward>(s, src, stride, n);
    else f32 ? launch_xfm_convert<float, xfm::kPair>(s, src, stride, n) : launch_xfm_convert<double, xfm::kPair>(s, src, stride, n);
  });
}
int glome_scene_instance_update_from(glome_scene* s, const int32_t* ids, const glome_xfm_source* src, int n, float* gpu_ms) {
  std::vector<const InstanceUpdateInfo*> U;
  int64_t stride = 0;
  auto check = [&]() -> int {
    if (int rc = instance_update_check(s, ids, src ? src->data : nullptr, n, U)) return rc;
    return xfm_source_check(s, src, n, &stride);
  };
  // every item converted on the host, by the device's own expressions (xfm_sources.hpp), and held to what the existing host form checks
  auto validate = [&]() -> int {
    glome_ctx* ctx = s->ctx;
    if (n == 0) return 0;
    const int w = xfm::width_of(src->form);
    for (int k = 0; k < n; k++) {
      const std::string node = "node " + std::to_string(ids[k]);
      double v[24], item[24], m[24];
      for (int q = 0; q < w; q++) {
        const size_t at = (size_t)k * (size_t)stride + (size_t)q;
        v[q] = src->dtype == GLOME_F32 ? (double)((const float*)src->data)[at] : ((const double*)src->data)[at];
        if (!std::isfinite(v[q])) { ctx->err = "instance update: a value of the item of " + node + " is not finite"; return GLOME_E_INVALID; }
      }
      if (src->form == GLOME_XFM_POSE) {
        if (!xfm::from_pose(v, item)) {
          ctx->err = "instance update: " + node + ": " + (v[7] > 0.0 ? "the quaternion has length 0" : "the scale is not positive");
          return GLOME_E_INVALID;
        }
      } else if (src->form == GLOME_XFM_FORWARD) {
        const double det = xfm::from_forward(v, item);
        bool finite = true;
        for (int q = 12; q < 24; q++) finite = finite && std::isfinite(item[q]);
        if (det == 0.0 || !finite) { ctx->err = "instance update: " + node + ": the forward matrix is singular (its determinant is 0 or its inverse is not finite)"; return GLOME_E_SCENE; }
      } else {
        xfm::convert(xfm::kPair, v, item);
      }
      if (src->base) xfm::mult(item, src->base + 24 * (size_t)k, m);
      else std::copy(item, item + 24, m);
      if (int rc = instance_matrix_check(s, ids[k], U[(size_t)k], m)) return rc;
    }
    return 0;
  };
  return blocking_update(s, gpu_ms, check, validate, [&](Staging& st) {
    // the caller's array as it is, in its own dtype and stride (the tail after the last item is not the call's to read)
    const size_t elems = (size_t)(n - 1) * (size_t)stride + (size_t)xfm::width_of(src->form);
    glome_xfm_source d = *src;
    d.data = st.in((const char*)src->data, elems * (src->dtype == GLOME_F32 ? sizeof(float) : sizeof(double)));
    d.base = src->base ? st.in(src->base, 24 * (size_t)n) : nullptr;
    d.stride = stride;
    return [=] { return glome_scene_instance_update_from_dev(s, ids, &d, n); };
  }, n == 0);
}

// ---- the bihs above an updated object, refitted one tree per call (item_bih_update_kernels.hpp) ----
static const NestedAnswer* nested_answer_of(const glome_scene* s, int32_t node) {
  { auto it = s->meshes.find(node); if (it != s->meshes.end()) return &it->second.info.nested; }
  { auto it = s->leaf_bihs.find(node); if (it != s->leaf_bihs.end()) return &it->second.info.nested; }
  { auto it = s->insts.find(node); if (it != s->insts.end()) return &it->second.nested; }
  { auto it = s->ibihs.find(node); if (it != s->ibihs.end()) return &it->second.info.nested; }
  return nullptr;
}
int32_t glome_scene_bihs_above(const glome_scene* s, int32_t node_id, int32_t* out, int32_t cap) {
  if (!s) return GLOME_E_INVALID;
  const NestedAnswer* A = nested_answer_of(s, node_id);
  if (!A) { s->ctx->err = "bihs_above: node " + std::to_string(node_id) + " is not a Mesh, a triangle bih, an Instance or a refittable bih of this scene (nor a sphere bih)"; return GLOME_E_INVALID; }
  if (!A->ok) { s->ctx->err = "bihs_above: " + A->why_not; return GLOME_E_INVALID; }
  for (size_t k = 0; k < A->above.size() && (int32_t)k < cap && out; k++) out[k] = A->above[k];
  return (int32_t)A->above.size();
}
int32_t glome_scene_stale_bihs(const glome_scene* s, int32_t* out, int32_t cap) {
  if (!s) return GLOME_E_INVALID;
  // a tree below another has every tree above that one above itself, and that one: more trees above, so it comes first
  std::vector<int> order(s->stale.begin(), s->stale.end());
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return s->ibihs.at(a).info.nested.above.size() > s->ibihs.at(b).info.nested.above.size(); });
  for (size_t k = 0; k < order.size() && (int32_t)k < cap && out; k++) out[k] = order[k];
  return (int32_t)order.size();
}
int glome_scene_nested_updates(glome_scene* s, int on) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (!on) {
    if (!s->stale.empty()) { ctx->err = "nested updates: bih " + std::to_string(*s->stale.begin()) + " is stale: refit the stale bihs before turning the switch off"; return GLOME_E_INVALID; }
    s->nested_on = false;
    return 0;
  }
  if (!s->d_live) {  // the bounds table with the commit's values, and the partial boxes of a bound's first stage: kept until glome_scene_release
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void *d = nullptr, *p = nullptr;
    HIPCHK(ctx, hipMalloc(&d, std::max<size_t>(6, s->live_bound0.size()) * sizeof(double)));
    s->allocs.push_back(d);
    HIPCHK(ctx, hipMalloc(&p, 6 * (size_t)itemupd::kPartMaxBlocks * sizeof(double)));
    s->allocs.push_back(p);
    if (!s->live_bound0.empty()) HIPCHK(ctx, hipMemcpy(d, s->live_bound0.data(), s->live_bound0.size() * sizeof(double), hipMemcpyHostToDevice));
    s->d_live = (double*)d; s->d_live_part = (double*)p;
  }
  s->nested_on = true;
  return 0;
}
// what both forms refuse before anything is launched
static int bih_refit_check(glome_scene* s, int32_t bih_id, glome_scene::InstBih** out) {
  glome_ctx* ctx = s->ctx;
  auto it = s->ibihs.find(bih_id);
  if (it == s->ibihs.end()) { ctx->err = "bih refit: node " + std::to_string(bih_id) + " is not a bih of this scene that holds a Mesh, a Bih or an Instance as an item"; return GLOME_E_INVALID; }
  if (!s->nested_on) { ctx->err = "bih refit refused: nested updates are off (glome_scene_nested_updates)"; return GLOME_E_INVALID; }
  for (int below : it->second.info.live)
    if (below >= 0 && s->stale.count(below)) { ctx->err = "bih refit refused: bih " + std::to_string(below) + " below bih " + std::to_string(bih_id) + " is stale: refit bih " + std::to_string(below) + " first"; return GLOME_E_INVALID; }
  *out = &it->second;
  return 0;
}
int glome_scene_bih_refit_dev(glome_scene* s, int32_t bih_id) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  glome_scene::InstBih* mp = nullptr;
  if (int rc = bih_refit_check(s, bih_id, &mp)) return rc;
  glome_scene::InstBih& m = *mp;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = ensure_tree_ws(s, m)) return rc;
  const TreeWs W(m.info);
  UpdateSpan span(ctx, nullptr);
  HIPCHK(ctx, span.begin());
  {  // every live item, changed or not: its rows from its object's bound as it stands
    itemupd::DItemsArgs A;
    A.live = m.d_live_items; A.bounds = s->d_live; A.xf = m.d_xf; A.rec_off = m.d_rec_off; A.ws_plane = m.d_ws; A.ws_box = m.d_ws + W.box; A.box64 = m.d_box64; A.n = m.n_live;
    A.error = &ctx->slot().d_counters->error;
    launch_lanes(ctx, itemupd::k_nest_item_rows, m.n_live, A);
  }
  refit_item_tree(s, bih_id, m, true);  // the Instance update's own launches
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, span.end());
  s->stale.erase(bih_id);
  mark_launched(ctx);  // (a box that reaches infinity is reported at the next synchronize)
  return 0;
}
int glome_scene_bih_refit(glome_scene* s, int32_t bih_id, float* gpu_ms) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (gpu_ms) *gpu_ms = 0;
  glome_scene::InstBih* m = nullptr;
  if (int rc = bih_refit_check(s, bih_id, &m)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = quiesce(ctx)) return rc;
  if (int rc = ensure_tree_ws(s, *m)) return rc;  // (outside the timed span)
  return run_blocking(ctx, gpu_ms, [&] { return glome_scene_bih_refit_dev(s, bih_id); });
}

// ---- the trace seam: Trace.trace over a caller's ray streams (trace_kernels.hpp) ----
// the limits of a call that shades, on its lights and its depth (the trace seam, the lens frames)
static int shading_limits(glome_ctx* ctx, int nlights, int maxdepth) {
  if (nlights > kMaxLights) { ctx->err = "too many lights"; return GLOME_E_LIMIT; }
  if (maxdepth < 1 || maxdepth > kMaxTraceDepth) { ctx->err = "maxdepth must be in 1.." + std::to_string(kMaxTraceDepth); return GLOME_E_LIMIT; }
  return 0;
}
// Everything a trace call of n > 0 rays is refused for on its arguments, in one order for both forms: trace_launch asks it first, the host
// forms before they stage anything.  host_form: `work` is the caller's array, nothing the device reads -- its staged twin is a device
// allocation, aligned far beyond 16 bytes.
static int trace_check(glome_ctx* ctx, size_t n, const RayStream& R, const glome_light* lights, int nlights, const glome_trace_params* P,
                       const float* rgbad, bool with_work, const uint32_t* work, bool host_form) {
  if (!R.ox || !R.oy || !R.oz || !R.dx || !R.dy || !R.dz) { ctx->err = "null ray stream"; return GLOME_E_INVALID; }
  if ((!rgbad && !with_work) || !P || nlights < 0 || (nlights > 0 && !lights)) { ctx->err = "bad argument"; return GLOME_E_INVALID; }
  if (with_work && !work) { ctx->err = "null work buffer"; return GLOME_E_INVALID; }
  if (with_work && !host_form && ((uintptr_t)work & 15u)) { ctx->err = "the work buffer must be 16-byte aligned"; return GLOME_E_INVALID; }
  if (int rc = shading_limits(ctx, nlights, P->maxdepth)) return rc;
  if (n > ((size_t)1 << 31)) { ctx->err = "a trace launch carries at most 2^31 rays"; return GLOME_E_LIMIT; }
  return 0;
}
// One launch for both forms.  with_work: glome_trace_work_batch_dev -- `work` receives a record per ray, rgbad may be null, and the launch
// takes the counting instance whatever count_work says; else `work` is null and rgbad is required.
static int trace_launch(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                        const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params* P,
                        float* rgbad, float* t, int32_t* prim, float* nx, float* ny, float* nz, int32_t* tex8, bool with_work, uint32_t* work,
                        glome_stats* stats) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (n == 0) return 0;
  if (int rc = trace_check(ctx, n, {ox, oy, oz, dx, dy, dz, tmax}, lights, nlights, P, rgbad, with_work, work, false)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DTraceArgs A;
  memset(&A, 0, sizeof(A));
  A.S = s->dev;
  fill_lights(A, lights, nlights);
  A.maxdepth = P->maxdepth; A.n = (uint32_t)n;
  A.check_unit = P->faithful ? 0 : 1;
  A.want_counters = stats ? 1 : 0;
  A.ox = ox; A.oy = oy; A.oz = oz; A.dx = dx; A.dy = dy; A.dz = dz; A.tmax = tmax;
  A.rgbad = rgbad; A.t = t; A.prim = prim; A.nx = nx; A.ny = ny; A.nz = nz; A.tex8 = tex8;
  A.work = with_work ? work : nullptr;
  A.counters = ctx->slot().d_counters;
  int rc;
  if (stats && (rc = reset_counters(ctx))) return rc;  // (nobody reads the counters of a launch without `stats`, and a trace launch has no queue heads)
  const uint32_t items = (uint32_t)((n + 63) / 64);
  const Choice ch = choose_trace(s->tr, P->faithful != 0, with_work || P->count_work != 0, P->maxdepth);  // (only the counting instances read A.work)
  const size_t lds = ch.generic ? flat_lds_bytes((int)s->dev.pk_generic_cap) : flat_lds_bytes(s->tr.stack_cap);
  // four blocks per wave slot the kernel can hold: the items are dealt statically, and the dispatcher evens out what they cost (trace_batch_loop)
  const int grid = (int)std::min<uint64_t>(items, (uint64_t)persistent_grid(ctx, lds, 0x7fffffff, waves_per_cu(ch)) * 4);
  if (!ch.generic && (rc = ensure_overflow(ctx, grid, 1, s->ovf_cap))) return rc;
  hipEvent_t ev_start = ctx->ev0, ev_stop = ctx->ev1;
  const bool pooled = launch_events(ctx, ev_start, ev_stop), timed = stats || pooled;
  if (timed) HIPCHK(ctx, hipEventRecord(ev_start, ctx->stream));
  if (ch.generic) { if (ch.generic_counts) launch_trace_generic(grid, ctx->stream, A); else launch_trace_generic_lean(grid, ctx->stream, A); }
  else {
    const FlatLaunch L{grid, lds, ctx->stream, s->tr.stack_cap, ctx->slot().d_ovf, s->ovf_cap};
    // (choose_trace only names listed instances -- instances.hpp choices_listed)
    if (!launch_trace_flat(ch.key, L, A)) { ctx->err = "no trace kernel instance for this scene class (build error)"; return GLOME_E_INVALID; }
  }
  HIPCHK(ctx, hipGetLastError());
  if (timed) HIPCHK(ctx, hipEventRecord(ev_stop, ctx->stream));
  if (!stats) { mark_launched(ctx); return 0; }  // (a refusal or a limit is reported at the next synchronize)
  memset(stats, 0, sizeof(*stats));
  stats->n_tiles = (int32_t)items; stats->n_pixels = (int32_t)std::min<size_t>(n, 0x7fffffff);
  return read_stats(ctx, stats, true, ev_start, ev_stop);
}
int glome_trace_batch_dev(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                          const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params* P,
                          float* rgbad, float* t, int32_t* prim, float* nx, float* ny, float* nz, int32_t* tex8, glome_stats* stats) {
  return trace_launch(s, n, ox, oy, oz, dx, dy, dz, tmax, lights, nlights, P, rgbad, t, prim, nx, ny, nz, tex8, false, nullptr, stats);
}
int glome_trace_work_batch_dev(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                               const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params* P,
                               float* rgbad, uint32_t* work, glome_stats* stats) {
  return trace_launch(s, n, ox, oy, oz, dx, dy, dz, tmax, lights, nlights, P, rgbad, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, work, stats);
}
int glome_trace_work_batch(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                           const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params* P,
                           float* rgbad, uint32_t* work, glome_stats* stats) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (n == 0) return 0;
  if (int rc = trace_check(ctx, n, {ox, oy, oz, dx, dy, dz, tmax}, lights, nlights, P, rgbad, true, work, true)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staging st;
  const RayStream R = st.rays({ox, oy, oz, dx, dy, dz, tmax}, n);
  float* d5 = st.out(rgbad, n * 5);
  uint32_t* dwork = st.out(work, n * kWorkWords);
  glome_stats local;
  return run_staged(ctx, st, true, [&] {
    return glome_trace_work_batch_dev(s, n, R.ox, R.oy, R.oz, R.dx, R.dy, R.dz, R.tmax, lights, nlights, P, d5, dwork, stats ? stats : &local);
  });
}
int glome_trace_batch(glome_scene* s, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                      const float* dz, const float* tmax, const glome_light* lights, int nlights, const glome_trace_params* P,
                      float* rgbad, float* t, int32_t* prim, float* nx, float* ny, float* nz, int32_t* tex8, glome_stats* stats) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  if (n == 0) return 0;
  if (int rc = trace_check(ctx, n, {ox, oy, oz, dx, dy, dz, tmax}, lights, nlights, P, rgbad, false, nullptr, true)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staging st;
  const RayStream R = st.rays({ox, oy, oz, dx, dy, dz, tmax}, n);
  float* d5 = st.out(rgbad, n * 5);
  const HitStream H{st.out(t, n), st.out(prim, n), st.out(nx, n), st.out(ny, n), st.out(nz, n), st.out(tex8, 8 * n)};
  glome_stats local;
  return run_staged(ctx, st, true, [&] {
    return glome_trace_batch_dev(s, n, R.ox, R.oy, R.oz, R.dx, R.dy, R.dz, R.tmax, lights, nlights, P, d5, H.t, H.prim, H.nx, H.ny, H.nz, H.tex8, stats ? stats : &local);
  });
}

// ---- frames through the trace seam: raygen and resolve (lens_kernels.hpp), and the pass loop that chains them around a trace launch ----
// Everything a raygen launch is refused for, decided before anything is launched; fills the launch's arguments but for the streams.
static int lens_args(glome_ctx* ctx, const glome_camera* cam, const glome_raygen_params* P, int64_t first_ray, int64_t n_rays, DLensArgs& A) {
  if (const char* why = raygen_params_error(P)) { ctx->err = why; return GLOME_E_INVALID; }
  if (!cam) { ctx->err = "null camera"; return GLOME_E_INVALID; }
  const float* c = cam->pos;  // (pos, fwd, up, right: twelve floats)
  for (int k = 0; k < 12; k++) if (!std::isfinite(c[k])) { ctx->err = "a camera component is not finite"; return GLOME_E_INVALID; }
  const int64_t total = (int64_t)P->width * P->height * P->samples;
  if (first_ray < 0 || n_rays < 0 || first_ray > total || n_rays > total - first_ray) { ctx->err = "ray range outside the frame"; return GLOME_E_INVALID; }
  if (n_rays > (1ll << 31)) { ctx->err = "a raygen launch makes at most 2^31 rays"; return GLOME_E_INVALID; }
  memset(&A, 0, sizeof(A));
  static_assert(sizeof(DCamera) == sizeof(glome_camera), "glome_camera is DCamera");
  memcpy(&A.cam, cam, sizeof(DCamera));
  const float* axis[3] = {cam->fwd, cam->right, cam->up};
  float* hat[3] = {A.fhat, A.rhat, A.uhat};
  for (int k = 0; k < 3; k++) {
    const double x = axis[k][0], y = axis[k][1], z = axis[k][2], len = std::sqrt(x * x + y * y + z * z);
    if (len > 0) { hat[k][0] = (float)(x / len); hat[k][1] = (float)(y / len); hat[k][2] = (float)(z / len); }
    else if (P->lens != GLOME_LENS_PINHOLE) { ctx->err = "the camera's fwd, right and up must not be zero for this lens"; return GLOME_E_INVALID; }
  }
  A.width = P->width; A.height = P->height; A.lens = P->lens; A.samples = P->samples; A.jitter = P->jitter ? 1 : 0;
  A.seed = P->seed; A.aperture = P->aperture; A.focus_dist = P->focus_dist;
  A.first_pixel = (uint32_t)(first_ray / P->samples); A.first_s = (uint32_t)(first_ray % P->samples);
  A.n = (uint32_t)n_rays;
  return 0;
}
static int resolve_check(glome_ctx* ctx, int32_t width, int32_t height, int32_t samples, int64_t first_pixel, int64_t n_pixels) {
  if (width < 1 || height < 1) { ctx->err = "width and height must be at least 1"; return GLOME_E_INVALID; }
  if ((int64_t)width * height > (1ll << 30)) { ctx->err = "frame too large"; return GLOME_E_INVALID; }
  if (samples < 1 || samples > kMaxLensSamples) { ctx->err = "samples must be in 1..64"; return GLOME_E_INVALID; }
  const int64_t total = (int64_t)width * height;
  if (first_pixel < 0 || n_pixels < 0 || first_pixel > total || n_pixels > total - first_pixel) { ctx->err = "pixel range outside the frame"; return GLOME_E_INVALID; }
  return 0;
}
// the blocks of a raygen launch of n rays: a wave per 64, at most CUs * 128 -- the kernels stride
static int lens_grid(glome_ctx* ctx, uint32_t n) { return (int)std::min<uint32_t>((n + 63u) >> 6, (uint32_t)ctx->prop.multiProcessorCount * 32u * 4u); }
// the two launches (arguments checked; timed_launch: both take part in glome_ctx_timing_begin / _end like a render launch)
static int lens_launch_rays(glome_ctx* ctx, const DLensArgs& A) {
  if (A.n == 0) return 0;
  return timed_launch(ctx, [&] { launch_camera_rays(lens_grid(ctx, A.n), ctx->stream, A); });
}
static int lens_launch_resolve(glome_ctx* ctx, int32_t samples, int64_t first_pixel, int64_t n_pixels, const float* in, float* rgbad, uint32_t* packed) {
  if (n_pixels == 0) return 0;
  DResolveArgs A;
  A.samples_in = in; A.rgbad = rgbad; A.packed = packed;
  A.first_pixel = (uint32_t)first_pixel; A.n_pixels = (uint32_t)n_pixels; A.samples = samples;
  A.vec = ((uintptr_t)in & 15u) == 0 ? 1 : 0;
  return timed_launch(ctx, [&] { launch_resolve((int)((n_pixels + 63) / 64), ctx->stream, A); });  // (a wave per 64 pixels: at most 2^24 blocks)
}
int glome_camera_rays_dev(glome_ctx* ctx, const glome_camera* cam, const glome_raygen_params* P, int64_t first_ray, int64_t n_rays,
                          float* ox, float* oy, float* oz, float* dx, float* dy, float* dz) {
  if (!ctx) return GLOME_E_INVALID;
  DLensArgs A;
  if (int rc = lens_args(ctx, cam, P, first_ray, n_rays, A)) return rc;
  if (!ox || !oy || !oz || !dx || !dy || !dz) { ctx->err = "null ray stream"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  A.ox = ox; A.oy = oy; A.oz = oz; A.dx = dx; A.dy = dy; A.dz = dz;
  return lens_launch_rays(ctx, A);
}
int glome_camera_rays(glome_ctx* ctx, const glome_camera* cam, const glome_raygen_params* P, int64_t first_ray, int64_t n_rays,
                      float* ox, float* oy, float* oz, float* dx, float* dy, float* dz) {
  if (!ctx) return GLOME_E_INVALID;
  DLensArgs A;
  if (int rc = lens_args(ctx, cam, P, first_ray, n_rays, A)) return rc;
  if (!ox || !oy || !oz || !dx || !dy || !dz) { ctx->err = "null ray stream"; return GLOME_E_INVALID; }
  if (n_rays == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Staging st;
  const size_t n = (size_t)n_rays;
  A.ox = st.out(ox, n); A.oy = st.out(oy, n); A.oz = st.out(oz, n); A.dx = st.out(dx, n); A.dy = st.out(dy, n); A.dz = st.out(dz, n);
  return run_staged(ctx, st, true, [&]() -> int {  // (raygen raises nothing in the slot's error word: the wait is all there is to see to)
    if (int rc = lens_launch_rays(ctx, A)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
  });
}
int glome_resolve_dev(glome_ctx* ctx, int32_t width, int32_t height, int32_t samples, int64_t first_pixel, int64_t n_pixels,
                      const float* rgbad_samples, float* rgbad, uint32_t* packed) {
  if (!ctx) return GLOME_E_INVALID;
  if (int rc = resolve_check(ctx, width, height, samples, first_pixel, n_pixels)) return rc;
  if (!rgbad_samples) { ctx->err = "null sample buffer"; return GLOME_E_INVALID; }
  if (!rgbad && !packed) { ctx->err = "a resolve needs a frame to write: rgbad, packed or both"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return lens_launch_resolve(ctx, samples, first_pixel, n_pixels, rgbad_samples, rgbad, packed);
}
// The pass's workspace: six streams of `rays` floats, each starting a multiple of 256 bytes in, then the results.
static size_t lens_stream_floats(size_t rays) { return (rays + 63) & ~(size_t)63; }
static int ensure_lens(glome_ctx* ctx, size_t rays) {
  glome_ctx::Slot& sl = ctx->slot();
  const size_t need = (lens_stream_floats(rays) * 6 + rays * 5) * sizeof(float);
  if (need <= sl.lens_bytes) return 0;
  if (sl.d_lens) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(sl.d_lens)); sl.d_lens = nullptr; sl.lens_bytes = 0; }
  HIPCHK(ctx, hipMalloc((void**)&sl.d_lens, need));
  sl.lens_bytes = need;
  return 0;
}
constexpr int64_t kLensRaysPerPass = 1ll << 22;  // 4M rays, 176 MiB of workspace: a first guess, not a measured optimum (include/glome_hip.h)
// everything glome_render_lens is refused for -- its own arguments, and what a pass's raygen, trace or resolve launch would refuse --
// asked before the first launch and before a frame is allocated; fills the raygen arguments but for the streams and the range
static int render_lens_check(glome_ctx* ctx, const glome_camera* cam, const glome_raygen_params* RP, const glome_light* lights, int nlights,
                             const glome_trace_params* TP, int64_t rays_per_pass, const void* rgbad, const void* packed, DLensArgs& A) {
  if (int rc = lens_args(ctx, cam, RP, 0, 0, A)) return rc;
  if (!rgbad && !packed) { ctx->err = "a frame needs somewhere to go: rgbad, packed or both"; return GLOME_E_INVALID; }
  if (!TP || nlights < 0 || (nlights > 0 && !lights) || rays_per_pass < 0) { ctx->err = "bad argument"; return GLOME_E_INVALID; }
  if ((int64_t)RP->width * RP->height * RP->samples > (1ll << 31)) { ctx->err = "glome_render_lens renders at most 2^31 rays per frame"; return GLOME_E_INVALID; }
  return shading_limits(ctx, nlights, TP->maxdepth);
}
// The workspace of a pass of `rays` rays, carved: the six streams into A, then the results.
static int lens_workspace(glome_ctx* ctx, size_t rays, DLensArgs& A, float** results) {
  if (int rc = ensure_lens(ctx, rays)) return rc;
  const size_t sf = lens_stream_floats(rays);
  float* w = ctx->slot().d_lens;
  A.ox = w; A.oy = w + sf; A.oz = w + 2 * sf; A.dx = w + 3 * sf; A.dy = w + 4 * sf; A.dz = w + 5 * sf;
  *results = w + 6 * sf;
  return 0;
}
// a stage's statistics added to its frame's: the trace launch's own, and the times of the launches before and after it
static void add_stats(glome_stats* sum, const glome_stats& ps, float ms_before, float ms_after) {
  sum->rays_primary += ps.rays_primary; sum->rays_shadow += ps.rays_shadow; sum->rays_secondary += ps.rays_secondary;
  sum->bih_nodes += ps.bih_nodes; sum->mesh_nodes += ps.mesh_nodes; sum->prim_tests += ps.prim_tests;
  sum->kernel_ms += ms_before + ps.kernel_ms + ms_after;
  sum->n_tiles += ps.n_tiles;
}
// One traced stage of a lens frame: produce() launches what puts n rays into the workspace's streams (A), the trace seam turns them into n
// results, consume() launches what takes the results.  With `stats` the two launches are timed between ev2 and ev3 (the trace launch in
// between records ev0 / ev1), the call waits for the stage and adds it to the frame's statistics; without, it waits for nothing.
template <class Produce, class Consume>
static int traced_stage(glome_scene* s, const DLensArgs& A, float* results, size_t n, const glome_light* lights, int nlights, const glome_trace_params* TP,
                        glome_stats* stats, Produce produce, Consume consume) {
  glome_ctx* ctx = s->ctx;
  float ms_produce = 0, ms_consume = 0;
  glome_stats ps;
  if (stats) HIPCHK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  if (int rc = produce()) return rc;
  if (stats) HIPCHK(ctx, hipEventRecord(ctx->ev3, ctx->stream));
  if (int rc = glome_trace_batch_dev(s, n, A.ox, A.oy, A.oz, A.dx, A.dy, A.dz, nullptr, lights, nlights, TP, results, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, stats ? &ps : nullptr)) return rc;
  if (stats) {  // (the trace launch has synchronised the stream: the producer's pair is complete)
    HIPCHK(ctx, hipEventElapsedTime(&ms_produce, ctx->ev2, ctx->ev3));
    HIPCHK(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  }
  if (int rc = consume()) return rc;
  if (stats) {
    HIPCHK(ctx, hipEventRecord(ctx->ev3, ctx->stream));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev3));
    HIPCHK(ctx, hipEventElapsedTime(&ms_consume, ctx->ev2, ctx->ev3));
    add_stats(stats, ps, ms_produce, ms_consume);
  }
  return 0;
}
int glome_render_lens_dev(glome_scene* s, const glome_camera* cam, const glome_raygen_params* RP, const glome_light* lights, int nlights,
                          const glome_trace_params* TP, int64_t rays_per_pass, float* rgbad_dev, uint32_t* packed_dev, glome_stats* stats) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  DLensArgs A;
  if (int rc = render_lens_check(ctx, cam, RP, lights, nlights, TP, rays_per_pass, rgbad_dev, packed_dev, A)) return rc;
  const int64_t pixels = (int64_t)RP->width * RP->height, samples = RP->samples;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t per_pass = std::min<int64_t>(pixels, std::max<int64_t>(1, (rays_per_pass ? rays_per_pass : kLensRaysPerPass) / samples));  // pixels
  float* results;
  if (int rc = lens_workspace(ctx, (size_t)(per_pass * samples), A, &results)) return rc;
  if (stats) memset(stats, 0, sizeof(*stats));
  for (int64_t p0 = 0; p0 < pixels; p0 += per_pass) {
    const int64_t np = std::min(per_pass, pixels - p0), n = np * samples;
    A.first_pixel = (uint32_t)p0; A.first_s = 0; A.n = (uint32_t)n;
    if (int rc = traced_stage(s, A, results, (size_t)n, lights, nlights, TP, stats, [&] { return lens_launch_rays(ctx, A); },
                              [&] { return lens_launch_resolve(ctx, (int32_t)samples, p0, np, results, rgbad_dev, packed_dev); })) return rc;
  }
  if (stats) stats->n_pixels = (int32_t)pixels;
  return 0;
}
int glome_render_lens(glome_scene* s, const glome_camera* cam, const glome_raygen_params* RP, const glome_light* lights, int nlights,
                      const glome_trace_params* TP, int64_t rays_per_pass, float* rgbad, uint32_t* packed, glome_stats* stats) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  DLensArgs A;
  if (int rc = render_lens_check(ctx, cam, RP, lights, nlights, TP, rays_per_pass, rgbad, packed, A)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t np = (size_t)RP->width * RP->height;
  Staging st;
  float* d5 = st.out(rgbad, np * 5);
  uint32_t* dp = st.out(packed, np);
  glome_stats local;
  return run_staged(ctx, st, true, [&] { return glome_render_lens_dev(s, cam, RP, lights, nlights, TP, rays_per_pass, d5, dp, stats ? stats : &local); });
}

// ---- adaptive lens frames: a pass in rounds, one per level of the rule (adaptive_rule.hpp, lens_adaptive_kernels.hpp) ----
// The pass's own workspace beside d_lens: kAdaptCounterWords list lengths (one per round, zeroed once a pass), 20 bytes of state per
// pixel, two lists of a word per pixel.
constexpr size_t kAdaptCounterWords = 16;
static_assert(kAdaptCounterWords >= (size_t)adaptive::kMaxLevels, "a list length per round");
static int ensure_adapt(glome_ctx* ctx, size_t pass_pixels) {
  glome_ctx::Slot& sl = ctx->slot();
  const size_t need = (kAdaptCounterWords + pass_pixels * 7) * sizeof(uint32_t);
  if (need <= sl.adapt_bytes) return 0;
  if (sl.d_adapt) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(sl.d_adapt)); sl.d_adapt = nullptr; sl.adapt_bytes = 0; }
  HIPCHK(ctx, hipMalloc((void**)&sl.d_adapt, need));
  sl.adapt_bytes = need;
  return 0;
}
// everything glome_render_lens_adaptive is refused for, asked before the first launch and before a frame is allocated
static int render_lens_adaptive_check(glome_ctx* ctx, const glome_camera* cam, const glome_raygen_params* RP, const glome_light* lights, int nlights,
                                      const glome_trace_params* TP, const glome_adaptive_params* AP, int64_t rays_per_pass, const void* rgbad,
                                      const void* packed, DLensArgs& A) {
  if (int rc = render_lens_check(ctx, cam, RP, lights, nlights, TP, rays_per_pass, rgbad, packed, A)) return rc;
  if (!AP) { ctx->err = "null adaptive params"; return GLOME_E_INVALID; }
  if (const char* why = adaptive_rule_error(AP->base_samples, RP->samples, AP->threshold)) { ctx->err = why; return GLOME_E_INVALID; }
  return 0;
}
int glome_render_lens_adaptive_dev(glome_scene* s, const glome_camera* cam, const glome_raygen_params* RP, const glome_light* lights, int nlights,
                                   const glome_trace_params* TP, const glome_adaptive_params* AP, int64_t rays_per_pass, float* rgbad_dev,
                                   uint32_t* packed_dev, uint8_t* counts_dev, glome_stats* stats) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  DLensArgs A;
  if (int rc = render_lens_adaptive_check(ctx, cam, RP, lights, nlights, TP, AP, rays_per_pass, rgbad_dev, packed_dev, A)) return rc;
  const int64_t pixels = (int64_t)RP->width * RP->height, max = RP->samples, base = AP->base_samples;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int64_t per_pass = std::min<int64_t>(pixels, std::max<int64_t>(1, (rays_per_pass ? rays_per_pass : kLensRaysPerPass) / max));  // pixels
  const size_t round_rays = (size_t)(per_pass * std::max(base, max / 2));  // the most a round holds: round 0's, or the last round's with every pixel listed
  float* results;
  if (int rc = lens_workspace(ctx, round_rays, A, &results)) return rc;
  if (int rc = ensure_adapt(ctx, (size_t)per_pass)) return rc;
  uint32_t* counters = ctx->slot().d_adapt;
  float* state = reinterpret_cast<float*>(counters + kAdaptCounterWords);
  uint32_t* lists[2] = {counters + kAdaptCounterWords + 5 * per_pass, counters + kAdaptCounterWords + 6 * per_pass};
  if (stats) memset(stats, 0, sizeof(*stats));
  for (int64_t p0 = 0; p0 < pixels; p0 += per_pass) {
    const int64_t np = std::min(per_pass, pixels - p0);
    HIPCHK(ctx, hipMemsetAsync(counters, 0, kAdaptCounterWords * sizeof(uint32_t), ctx->stream));
    uint32_t len = (uint32_t)np;  // entries of the round: the pass's pixels, then the list the round before wrote
    int round = 0;
    for (int64_t level = base;; level *= 2, round++) {
      const int64_t h = level / 2, n = round == 0 ? np * base : (int64_t)len * h;
      const bool last = level == max;
      auto rays = [&]() -> int {
        if (round == 0) {  // samples [0, base) of every pixel of the pass: k_camera_rays's own frame order at samples = base
          A.samples = (int32_t)base; A.first_pixel = (uint32_t)p0; A.first_s = 0; A.n = (uint32_t)n;
          return lens_launch_rays(ctx, A);
        }
        DLensListArgs LA;
        LA.L = A; LA.L.first_pixel = (uint32_t)p0; LA.L.n = (uint32_t)n;
        LA.list = lists[(round - 1) & 1]; LA.pass_pixels = (uint32_t)np; LA.h = (uint32_t)h;
        if (LA.L.n == 0) return 0;
        return timed_launch(ctx, [&] { launch_camera_rays_list(lens_grid(ctx, LA.L.n), ctx->stream, LA); });
      };
      auto fold = [&]() -> int {
        DAdaptFoldArgs F;
        F.samples_in = results; F.rgbad = rgbad_dev; F.packed = packed_dev; F.counts = counts_dev;
        F.state = state; F.list_in = lists[(round - 1) & 1]; F.list_out = lists[round & 1]; F.counter = counters + round;
        F.first_pixel = (uint32_t)p0; F.pass_pixels = (uint32_t)np; F.n = len;
        F.level = (int32_t)level; F.last = last ? 1 : 0; F.threshold = AP->threshold;
        if (F.n == 0) return 0;
        return timed_launch(ctx, [&] { launch_adaptive_fold((int)((F.n + 63u) / 64u), ctx->stream, round == 0, F); });  // (a wave per 64 entries: at most 2^24 blocks)
      };
      if (int rc = traced_stage(s, A, results, (size_t)n, lights, nlights, TP, stats, rays, fold)) return rc;
      if (last) break;
      // the next round's size: 4 bytes and one wait for the stream
      HIPCHK(ctx, hipMemcpyAsync(&len, counters + round, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      if (len > (uint32_t)np) len = (uint32_t)np;  // (the fold writes no list slot beyond the pass)
      if (len == 0) break;
    }
  }
  if (stats) stats->n_pixels = (int32_t)pixels;
  return 0;
}
int glome_render_lens_adaptive(glome_scene* s, const glome_camera* cam, const glome_raygen_params* RP, const glome_light* lights, int nlights,
                               const glome_trace_params* TP, const glome_adaptive_params* AP, int64_t rays_per_pass, float* rgbad, uint32_t* packed,
                               uint8_t* counts, glome_stats* stats) {
  if (!s) return GLOME_E_INVALID;
  glome_ctx* ctx = s->ctx;
  DLensArgs A;
  if (int rc = render_lens_adaptive_check(ctx, cam, RP, lights, nlights, TP, AP, rays_per_pass, rgbad, packed, A)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t np = (size_t)RP->width * RP->height;
  Staging st;
  float* d5 = st.out(rgbad, np * 5);
  uint32_t* dp = st.out(packed, np);
  uint8_t* dc = st.out(counts, np);
  glome_stats local;
  return run_staged(ctx, st, true, [&] { return glome_render_lens_adaptive_dev(s, cam, RP, lights, nlights, TP, AP, rays_per_pass, d5, dp, dc, stats ? stats : &local); });
}

// ---- tile payload transport ----
int64_t glome_tiles_payload_floats(const glome_render_params* P, int tile_first, int tile_stride) {
  if (!P || P->width <= 0 || P->height <= 0 || P->blocksize <= 0 || tile_stride <= 0 || tile_first < 0) return -1;
  std::vector<DTile> t; uint32_t w; int64_t px;
  owned_tiles(P->width, P->height, P->blocksize, tile_first, tile_stride, P->rank0_share_pct, t, w, px);
  return px * 5;
}
int glome_tiles_pack_dev(glome_ctx* ctx, const glome_render_params* P, const float* rgbad_dev, float* payload_dev) {
  if (!ctx) return GLOME_E_INVALID;
  int rc = check_params(ctx, P);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  glome_ctx::TileTable* tt;
  if ((rc = get_tiles(ctx, P, P->tile_first, P->tile_stride, &tt))) return rc;
  if (tt->host.empty()) return 0;
  hipLaunchKernelGGL(k_tiles_pack, dim3(21, std::min<int>((int)tt->host.size(), 1024)), dim3(256), 0, ctx->stream, tt->dev, (int)tt->host.size(), P->width, rgbad_dev, payload_dev);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
// one table over every tile of the frame; pix_base = owner rank's slab offset + the tile's offset inside that rank's payload
static int gathered_table(glome_ctx* ctx, const glome_render_params* P, int world, int64_t stride_pixels, glome_ctx::TileTable** out) {
  std::vector<int> key{P->width, P->height, P->blocksize, -world, (int)stride_pixels, P->rank0_share_pct};
  auto it = ctx->tile_cache.find(key);
  if (it == ctx->tile_cache.end()) {
    glome_ctx::TileTable tt;
    for (int r = 0; r < world; r++) {
      std::vector<DTile> t; uint32_t w; int64_t px;
      owned_tiles(P->width, P->height, P->blocksize, r, world, P->rank0_share_pct, t, w, px);
      if ((int64_t)r * stride_pixels + px > 0xffffffffll) { ctx->err = "gathered payload too large"; return GLOME_E_LIMIT; }
      for (DTile& d : t) { d.pix_base += (uint32_t)(r * stride_pixels); tt.host.push_back(d); }
      tt.pixels += px;
    }
    size_t bytes = std::max<size_t>(1, tt.host.size()) * sizeof(DTile);
    HIPCHK(ctx, hipMalloc((void**)&tt.dev, bytes));
    if (!tt.host.empty()) HIPCHK(ctx, hipMemcpy(tt.dev, tt.host.data(), tt.host.size() * sizeof(DTile), hipMemcpyHostToDevice));
    it = ctx->tile_cache.emplace(key, std::move(tt)).first;
  }
  *out = &it->second;
  return 0;
}
int glome_tiles_blit_all_dev(glome_ctx* ctx, const glome_render_params* P, int world, const float* gathered_dev, int64_t stride_floats,
                             float* rgbad_dev, uint32_t* packed_dev) {
  if (!ctx) return GLOME_E_INVALID;
  int rc = check_params(ctx, P);
  if (rc) return rc;
  if (world <= 0 || stride_floats < 0 || stride_floats % 5 != 0) { ctx->err = "bad world / stride"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  glome_ctx::TileTable* tt;
  if ((rc = gathered_table(ctx, P, world, stride_floats / 5, &tt))) return rc;
  if (tt->host.empty()) return 0;
  hipLaunchKernelGGL(k_tiles_blit, dim3(17, std::min<int>((int)tt->host.size(), 1024)), dim3(256), 0, ctx->stream, tt->dev, (int)tt->host.size(), P->width, gathered_dev, rgbad_dev, packed_dev);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int glome_tiles_blit_all_packed_dev(glome_ctx* ctx, const glome_render_params* P, int world, const uint32_t* gathered_dev, int64_t stride_pixels,
                                    uint32_t* packed_dev) {
  return glome_tiles_blit_all_packed_batch_dev(ctx, P, world, gathered_dev, stride_pixels, 1, 0, packed_dev, 0);
}
int glome_tiles_blit_all_packed_batch_dev(glome_ctx* ctx, const glome_render_params* P, int world, const uint32_t* gathered_dev, int64_t stride_pixels,
                                          int nframes, int64_t payload_frame_stride, uint32_t* packed_dev, int64_t out_frame_stride) {
  if (!ctx) return GLOME_E_INVALID;
  int rc = check_params(ctx, P);
  if (rc) return rc;
  if (world <= 0 || stride_pixels < 0 || !gathered_dev || !packed_dev || nframes < 1 || nframes > kMaxBatchFrames || payload_frame_stride < 0 || out_frame_stride < 0) {
    ctx->err = "bad world / stride / buffer / frame count"; return GLOME_E_INVALID;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  glome_ctx::TileTable* tt;
  if ((rc = gathered_table(ctx, P, world, stride_pixels, &tt))) return rc;
  if (tt->host.empty()) return 0;
  hipLaunchKernelGGL(k_tiles_blit_packed, dim3(17, std::min<int>((int)tt->host.size(), 1024), nframes), dim3(256), 0, ctx->stream, tt->dev, (int)tt->host.size(), P->width, gathered_dev,
                     packed_dev, (size_t)payload_frame_stride, (size_t)out_frame_stride);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int glome_tiles_blit_dev(glome_ctx* ctx, const glome_render_params* P, int tile_first, int tile_stride, const float* payload_dev, float* rgbad_dev, uint32_t* packed_dev) {
  if (!ctx) return GLOME_E_INVALID;
  int rc = check_params(ctx, P);
  if (rc) return rc;
  if (tile_stride <= 0 || tile_first < 0) { ctx->err = "bad tile shard"; return GLOME_E_INVALID; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  glome_ctx::TileTable* tt;
  if ((rc = get_tiles(ctx, P, tile_first, tile_stride, &tt))) return rc;
  if (tt->host.empty()) return 0;
  hipLaunchKernelGGL(k_tiles_blit, dim3(17, std::min<int>((int)tt->host.size(), 1024)), dim3(256), 0, ctx->stream, tt->dev, (int)tt->host.size(), P->width, payload_dev, rgbad_dev, packed_dev);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}


// ================================================================================================ several GPUs, one process
// renderTiles' `runPar $ parMap` over tiles followed by `forM_ tiles (blitTile surf)` (Glome.hs:379-386) across the GPUs of a
// node, for a host that drives all of them from one process (the Haskell host of INTEGRATION.md): scenes[i] is the scene
// committed on context i, tile k of the frame belongs to rank k mod n (or to the rank rank0_share_pct's pattern gives it), a rank renders its tiles of up to 32 frames in one
// launch straight into a packed payload, the payloads travel to rank 0's GPU over xGMI, one launch there blits the frames.
// The exchange is the path's only communication step.  Transport: RCCL send / recv in one group (librccl is opened at run
// time, so the library carries no link-time dependency on it) when the ranks sit on distinct devices; peer copies on rank
// 0's stream (hipMemcpyPeerAsync) when librccl cannot be loaded or two ranks share a device (how the path is tested on a
// one-GPU box).  glome_amd/dist.py is the same data path with one process per GPU and torch.distributed's gather.
#include <dlfcn.h>
namespace {
struct Rccl {  // the five entry points the gather needs, resolved from librccl.so on first use
  typedef void* comm_t;
  int (*CommInitAll)(comm_t*, int, const int*) = nullptr;
  int (*CommDestroy)(comm_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, comm_t, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, comm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
  bool debug_lib = false;  // GLOME_DEBUG_RCCL_LIB named the library: the test stub, not RCCL
  static Rccl& get() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
      void* h = nullptr;
      // GLOME_DEBUG_RCCL_LIB: another library with the same entry points (tests/rcclstub: the RCCL branch exercised on one GPU)
      if (const char* dbg = getenv("GLOME_DEBUG_RCCL_LIB")) { h = dlopen(dbg, RTLD_NOW | RTLD_GLOBAL); r.debug_lib = true; }
      else for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
      if (!h) return;
      r.CommInitAll = (decltype(r.CommInitAll))dlsym(h, "ncclCommInitAll");
      r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
      r.GroupStart = (decltype(r.GroupStart))dlsym(h, "ncclGroupStart");
      r.GroupEnd = (decltype(r.GroupEnd))dlsym(h, "ncclGroupEnd");
      r.Send = (decltype(r.Send))dlsym(h, "ncclSend");
      r.Recv = (decltype(r.Recv))dlsym(h, "ncclRecv");
      r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
      r.ok = r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv;
    });
    return r;
  }
};
constexpr int kNcclUint32 = 3;  // ncclUint32 (nccl.h: ncclInt8 0, ncclUint8 1, ncclInt32 2, ncclUint32 3)
}  // namespace

struct glome_multi {
  int n = 0;
  std::vector<glome_scene*> scenes;
  glome_render_params P{}, P0{};           // the frame (work tiles in renderTile mode); P0 = P with rank 0's shard
  std::vector<glome_render_params> Pl;     // rank i's shard: tiles i, i + n, ...
  int64_t maxp = 0;                        // pixels of the largest shard: a frame's slot in every payload
  std::vector<uint32_t*> payload;          // rank i's payload on device i: kMaxBatchFrames * maxp words (rank 0: its slab of `gathered`)
  uint32_t* gathered = nullptr;            // device 0: n slabs of kMaxBatchFrames * maxp words
  std::vector<hipEvent_t> rendered;        // rank i's launch is done
  hipEvent_t consumed = nullptr;           // rank 0 has taken the payloads of the last call
  bool used = false;
  bool rccl = false;
  bool direct = false;                     // every rank's render kernel stores its pixels straight into packed_dev on rank 0's GPU (peer access)
  std::vector<Rccl::comm_t> comms;
  std::string err;
};
#define MHIP(m, call)                                                                 \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) { (m)->err = std::string(#call) + ": " + hipGetErrorString(e_); return GLOME_E_HIP; } \
  } while (0)

glome_multi* glome_multi_create(glome_scene* const* scenes, int n, const glome_render_params* P, int transport) {
  if (!scenes || n < 1 || n > 64 || !P) { g_global_error = "glome_multi_create: bad argument"; return nullptr; }
  for (int i = 0; i < n; i++) {
    if (!scenes[i]) { g_global_error = "glome_multi_create: null scene"; return nullptr; }
    for (int j = 0; j < i; j++) if (scenes[j]->ctx == scenes[i]->ctx) { g_global_error = "glome_multi_create: every rank needs a context (and scene) of its own"; return nullptr; }
  }
  if (check_params(scenes[0]->ctx, P)) { g_global_error = scenes[0]->ctx->err; return nullptr; }
  glome_multi* m = new glome_multi();
  m->n = n;
  m->scenes.assign(scenes, scenes + n);
  m->P = *P;
  // renderTile's pixels do not depend on the tile map (the adaptive sampler's do, Q21): shard 64x64 work tiles then
  if (P->mode == GLOME_MODE_TILE) m->P.blocksize = 64;
  m->P.tile_first = 0; m->P.tile_stride = 1;
  for (int i = 0; i < n; i++) {
    glome_render_params q = m->P;
    q.tile_first = i; q.tile_stride = n;
    m->Pl.push_back(q);
    m->maxp = std::max<int64_t>(m->maxp, glome_tiles_payload_floats(&q, i, n) / 5);
  }
  m->maxp = std::max<int64_t>(m->maxp, 1);
  auto fail = [&](const std::string& what) { g_global_error = "glome_multi_create: " + what; glome_multi_destroy(m); return (glome_multi*)nullptr; };
  const size_t slab = (size_t)kMaxBatchFrames * (size_t)m->maxp;
  // transport 2 ("direct"): no payloads, no exchange, no blit -- every rank's render kernel writes its tiles' packed pixels where they
  // belong in the caller's framebuffer on rank 0's GPU (4 bytes per pixel over xGMI, a 256-byte store per work item), and rank 0's
  // stream waits for the other ranks' launches.  It needs every rank's device to reach rank 0's memory: the same device, or peer access.
  if (transport == 2 && n > 1) {
    bool can_all = true;
    for (int i = 1; i < n && can_all; i++) {
      if (scenes[i]->ctx->device == scenes[0]->ctx->device) continue;
      int can = 0;
      (void)hipDeviceCanAccessPeer(&can, scenes[i]->ctx->device, scenes[0]->ctx->device);
      if (!can) { can_all = false; break; }
      if (hipSetDevice(scenes[i]->ctx->device) != hipSuccess) { can_all = false; break; }
      hipError_t e = hipDeviceEnablePeerAccess(scenes[0]->ctx->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); can_all = false; }
    }
    m->direct = can_all;
    // nobody receives or blits any more: every rank owns a fair share of the tiles, whatever weight the caller gave rank 0
    if (m->direct) { m->P.rank0_share_pct = 0; for (auto& q : m->Pl) q.rank0_share_pct = 0; }
  }
  const bool use_rccl = transport == 1 || (transport == 2 && !m->direct);
  m->payload.assign(n, nullptr);
  m->rendered.assign(n, nullptr);
  if (!m->direct) {
    if (hipSetDevice(scenes[0]->ctx->device) != hipSuccess || hipMalloc((void**)&m->gathered, slab * n * sizeof(uint32_t)) != hipSuccess) return fail("device allocation failed");
    m->payload[0] = m->gathered;  // rank 0 renders into its own slab
  }
  for (int i = 0; i < n; i++) {
    if (hipSetDevice(scenes[i]->ctx->device) != hipSuccess) return fail("hipSetDevice failed");
    if (!m->direct && i > 0 && hipMalloc((void**)&m->payload[i], slab * sizeof(uint32_t)) != hipSuccess) return fail("device allocation failed");
    if (hipEventCreateWithFlags(&m->rendered[i], hipEventDisableTiming) != hipSuccess) return fail("hipEventCreate failed");
  }
  (void)hipSetDevice(scenes[0]->ctx->device);
  if (hipEventCreateWithFlags(&m->consumed, hipEventDisableTiming) != hipSuccess) return fail("hipEventCreate failed");
  // transport
  bool distinct = true;
  for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) distinct &= scenes[i]->ctx->device != scenes[j]->ctx->device;
  // (GLOME_DEBUG_RCCL_SAME_DEVICE lifts the distinct-device condition -- real RCCL refuses two ranks on one device -- for the
  // stubbed transport of the one-GPU test, and ONLY for it: with the real library loaded the variable is ignored)
  if (m->direct) return m;
  if (use_rccl && n > 1 && (distinct || (Rccl::get().debug_lib && getenv("GLOME_DEBUG_RCCL_SAME_DEVICE"))) && Rccl::get().ok) {
    std::vector<int> devs;
    for (int i = 0; i < n; i++) devs.push_back(scenes[i]->ctx->device);
    m->comms.assign(n, nullptr);
    int rc = Rccl::get().CommInitAll(m->comms.data(), n, devs.data());
    if (rc != 0) return fail(std::string("ncclCommInitAll: ") + (Rccl::get().GetErrorString ? Rccl::get().GetErrorString(rc) : "error"));
    m->rccl = true;
  } else if (n > 1) {
    for (int i = 1; i < n; i++) {  // peer copies into rank 0's GPU: let it see the others' memory where they differ
      if (scenes[i]->ctx->device == scenes[0]->ctx->device) continue;
      int can = 0;
      (void)hipDeviceCanAccessPeer(&can, scenes[0]->ctx->device, scenes[i]->ctx->device);
      if (can) { (void)hipSetDevice(scenes[0]->ctx->device); hipError_t e = hipDeviceEnablePeerAccess(scenes[i]->ctx->device, 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError(); }
    }
  }
  return m;
}
void glome_multi_destroy(glome_multi* m) {
  if (!m) return;
  for (int i = 0; i < m->n; i++) {
    (void)hipSetDevice(m->scenes[i]->ctx->device);
    (void)hipStreamSynchronize(m->scenes[i]->ctx->stream);
    if (i > 0 && i < (int)m->payload.size() && m->payload[i]) (void)hipFree(m->payload[i]);
    if (i < (int)m->rendered.size() && m->rendered[i]) (void)hipEventDestroy(m->rendered[i]);
    if (m->rccl && i < (int)m->comms.size() && m->comms[i]) (void)Rccl::get().CommDestroy(m->comms[i]);
  }
  (void)hipSetDevice(m->scenes[0]->ctx->device);
  if (m->gathered) (void)hipFree(m->gathered);
  if (m->consumed) (void)hipEventDestroy(m->consumed);
  delete m;
}
const char* glome_multi_last_error(const glome_multi* m) { return m ? m->err.c_str() : g_global_error.c_str(); }
const char* glome_multi_transport(const glome_multi* m) { return !m ? "" : (m->n == 1 ? "none" : (m->direct ? "direct" : (m->rccl ? "rccl" : "peer-copy"))); }

int glome_multi_render(glome_multi* m, const glome_camera* cams, int nframes, const glome_light* lights, int nlights, uint32_t* packed_dev) {
  if (!m || !cams || !packed_dev) return GLOME_E_INVALID;
  if (nframes < 1 || nframes > kMaxBatchFrames || (m->P.mode != GLOME_MODE_TILE && nframes != 1)) { m->err = "a call carries 1..32 frames (one in adaptive mode)"; return GLOME_E_LIMIT; }
  const int n = m->n;
  glome_ctx* c0 = m->scenes[0]->ctx;
  const size_t slab = (size_t)kMaxBatchFrames * (size_t)m->maxp;
  if (m->direct) {
    // every rank renders its tiles of the nframes views into the frames themselves (frame layout, its own tiles only); rank 0's stream
    // -- the one the caller orders its reads of packed_dev on -- waits for the others
    const int64_t fs = (int64_t)m->P.width * m->P.height;
    for (int i = n - 1; i >= 0; i--) {  // (rank 0 last: its launch is queued behind nothing of the others)
      glome_ctx* c = m->scenes[i]->ctx;
      MHIP(m, hipSetDevice(c->device));
      int rc = nframes > 1 ? render_impl(m->scenes[i], cams, lights, nlights, &m->Pl[i], nullptr, packed_dev, nullptr, 0, nframes, fs)
                           : render_impl(m->scenes[i], cams, lights, nlights, &m->Pl[i], nullptr, packed_dev, nullptr, 0);
      if (rc) { m->err = "rank " + std::to_string(i) + ": " + c->err; return rc; }
      if (i > 0) MHIP(m, hipEventRecord(m->rendered[i], c->stream));
    }
    MHIP(m, hipSetDevice(c0->device));
    for (int i = 1; i < n; i++) MHIP(m, hipStreamWaitEvent(c0->stream, m->rendered[i], 0));
    m->used = true;
    return 0;
  }
  // every rank renders its tiles of the nframes views into its payload (frame f at f * maxp)
  for (int i = 0; i < n; i++) {
    glome_ctx* c = m->scenes[i]->ctx;
    MHIP(m, hipSetDevice(c->device));
    if (m->used && i > 0 && !m->rccl) MHIP(m, hipStreamWaitEvent(c->stream, m->consumed, 0));  // rank 0 has read this payload's last contents
    int rc = nframes > 1 ? render_impl(m->scenes[i], cams, lights, nlights, &m->Pl[i], nullptr, m->payload[i], nullptr, 2, nframes, m->maxp)
                         : render_impl(m->scenes[i], cams, lights, nlights, &m->Pl[i], nullptr, m->payload[i], nullptr, 2);
    if (rc) { m->err = "rank " + std::to_string(i) + ": " + c->err; return rc; }
    if (i > 0) MHIP(m, hipEventRecord(m->rendered[i], c->stream));
  }
  // the exchange: rank i's payload -> slab i on rank 0's GPU
  const size_t words = (size_t)nframes * (size_t)m->maxp;
  if (n > 1 && m->rccl) {
    Rccl& R = Rccl::get();
    int rc = R.GroupStart();
    // rank i's Send is ordered on ITS stream behind its render and in front of its next one, so a payload is never rewritten
    // before it has left; rank 0's Recvs are ordered on its stream in front of the blit.  (The device of a call's communicator
    // is made current first: RCCL releases before 2.18 want that.)
    hipError_t he = hipSuccess;  // (no early return inside the group: GroupEnd is called whatever happens)
    for (int i = 1; i < n && rc == 0 && he == hipSuccess; i++) {
      if ((he = hipSetDevice(m->scenes[i]->ctx->device)) != hipSuccess) break;
      rc = R.Send(m->payload[i], words, kNcclUint32, 0, m->comms[i], m->scenes[i]->ctx->stream);
      if ((he = hipSetDevice(c0->device)) != hipSuccess) break;
      if (rc == 0) rc = R.Recv(m->gathered + (size_t)i * slab, words, kNcclUint32, i, m->comms[0], c0->stream);
    }
    int rc2 = R.GroupEnd();
    if (he != hipSuccess) { m->err = std::string("hipSetDevice inside the RCCL group: ") + hipGetErrorString(he); return GLOME_E_HIP; }
    if (rc || rc2) { m->err = std::string("RCCL send / recv: ") + (R.GetErrorString ? R.GetErrorString(rc ? rc : rc2) : "error"); return GLOME_E_HIP; }
  } else if (n > 1) {
    MHIP(m, hipSetDevice(c0->device));
    for (int i = 1; i < n; i++) {
      MHIP(m, hipStreamWaitEvent(c0->stream, m->rendered[i], 0));
      MHIP(m, hipMemcpyPeerAsync(m->gathered + (size_t)i * slab, c0->device, m->payload[i], m->scenes[i]->ctx->device, words * sizeof(uint32_t), c0->stream));
    }
    MHIP(m, hipEventRecord(m->consumed, c0->stream));
  }
  m->used = true;
  // blitTile for every tile of every frame, one launch on rank 0
  MHIP(m, hipSetDevice(c0->device));
  int rc = glome_tiles_blit_all_packed_batch_dev(c0, &m->P, n, m->gathered, (int64_t)slab, nframes, m->maxp, packed_dev, (int64_t)m->P.width * m->P.height);
  if (rc) { m->err = c0->err; return rc; }
  return 0;
}
int glome_multi_synchronize(glome_multi* m) {
  if (!m) return GLOME_E_INVALID;
  int rc = 0;
  for (int i = m->n - 1; i >= 0; i--) {
    MHIP(m, hipSetDevice(m->scenes[i]->ctx->device));
    int r = glome_ctx_synchronize(m->scenes[i]->ctx);
    if (r) { m->err = m->scenes[i]->ctx->err; rc = r; }
  }
  return rc;
}
// the one-call form SURVEY.md Appendix B names: host framebuffer out
int glome_render_multi(glome_scene* const* scenes, int n, const glome_camera* cam, const glome_light* lights, int nlights, const glome_render_params* P, uint32_t* packed) {
  if (!packed) { g_global_error = "glome_render_multi: null framebuffer"; return GLOME_E_INVALID; }
  glome_multi* m = glome_multi_create(scenes, n, P, 2);  // direct stores where the GPUs reach each other's memory, else RCCL, else peer copies
  if (!m) return GLOME_E_INVALID;
  uint32_t* d = nullptr;
  const size_t np = (size_t)P->width * P->height;
  int rc = 0;
  if (hipSetDevice(scenes[0]->ctx->device) != hipSuccess || hipMalloc((void**)&d, np * 4) != hipSuccess) rc = GLOME_E_HIP;
  if (!rc) rc = glome_multi_render(m, cam, 1, lights, nlights, d);
  if (!rc) rc = glome_multi_synchronize(m);
  if (!rc && hipMemcpy(packed, d, np * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = GLOME_E_HIP;
  if (rc) g_global_error = std::string("glome_render_multi: ") + m->err;
  if (d) (void)hipFree(d);
  glome_multi_destroy(m);
  return rc;
}
