// walk_table_dump.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_walk_entry_table_host.py builds it into a temporary directory).  Runs the
// product's flattener over a builder's graph, as a commit does, and hands out the pools the walk-entry table is made from and the table
// itself, as 32-bit words.  Nothing in glome_amd includes or loads it.
#include <cstdint>
#include <cstring>
#include <exception>

#include "../../glome_amd/csrc/capi_shared.hpp"

using namespace glome;

extern "C" {
// what: 0 = entries, 1 = recs, 2 = bihhdr, 3 = walk; 4 = {tier, n_entries as a commit sets DScene::n_entries}.  Returns the pool's size in
// words and copies up to cap of them; -1: the flattener refused the scene.
int walk_table_dump(glome_sb* sb, int root, int what, uint32_t* out, int cap) {
  FlatScene F;
  try {
    Flattener fl(sb_graph(sb), F);
    fl.run(root);
  } catch (std::exception&) { return -1; }
  const void* p = nullptr;
  size_t words = 0;
  uint32_t info[2] = {F.tier, F.tier == 0 ? (uint32_t)F.entries.size() : 0u};
  switch (what) {
    case 0: p = F.entries.data(); words = F.entries.size() * 4; break;
    case 1: p = F.recs.data(); words = F.recs.size() * 4; break;
    case 2: p = F.bihhdr.data(); words = F.bihhdr.size() * 4; break;
    case 3: p = F.walk.data(); words = F.walk.size() * 4; break;
    case 4: p = info; words = 2; break;
    default: return -2;
  }
  const size_t n = words < (size_t)cap ? words : (size_t)cap;
  if (out && n) std::memcpy(out, p, n * 4);
  return (int)words;
}
}
