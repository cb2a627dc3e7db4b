// The scratch of one intake call (intake_api.cpp, repair_api.cpp): the sections of a grow-only
// context buffer, laid out per call.  Host only.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "intake.hpp"
#include "shredder.hpp"
#include "wire.hpp"

namespace ag {
namespace host {

constexpr size_t kIntakeMax = size_t{1} << 24;  // datagrams per call, rows per window
constexpr size_t kProofBytes = 32 * ag::kPipeHeight;

// Sections of the scratch buffer, each 256-byte aligned.
struct Carver {
  uint8_t* base;
  size_t used = 0;
  template <typename T>
  T* take(size_t count) {
    T* out = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += (count * sizeof(T) + 255) / 256 * 256;
    return out;
  }
};

struct IntakeScratch {
  ag::ShredColumns cols{};
  uint8_t *wire, *plausible, *roots, *commit, *ok;
  uint32_t *row, *meta, *mlist, *list1, *list2, *counts, *pick, *out;
  size_t zero_bytes, none_bytes;  // [ok, counts] is one zeroed span, [pick .. claim] one of kIntakeNone
  uint32_t *setter, *tstar, *claim;
};

// Lays the sections out from `base` (null: only the size is wanted); returns the bytes used.
inline size_t carve(uint8_t* base, size_t n, size_t nrows, size_t nslots, IntakeScratch* s) {
  Carver c{base};
  s->cols.kind = c.take<uint8_t>(n);
  s->cols.slot = c.take<uint64_t>(n);
  s->cols.slice_index = c.take<uint64_t>(n);
  s->cols.is_last = c.take<uint8_t>(n);
  s->cols.shred_index = c.take<uint32_t>(n);
  s->cols.data = c.take<uint8_t>(n * ag::kPipeMaxShredBytes);
  s->cols.data_stride = ag::kPipeMaxShredBytes;
  s->cols.data_len = c.take<uint32_t>(n);
  s->cols.sig = c.take<uint8_t>(n * 64);
  s->cols.proof = c.take<uint8_t>(n * kProofBytes);
  s->cols.proof_stride = kProofBytes;
  s->cols.height = c.take<uint32_t>(n);
  s->wire = c.take<uint8_t>(n);
  s->plausible = c.take<uint8_t>(n);
  s->roots = c.take<uint8_t>(n * 32);
  s->commit = c.take<uint8_t>(n * ag::kIntakeCommitStride);
  s->row = c.take<uint32_t>(n);
  s->meta = c.take<uint32_t>(n);
  s->mlist = c.take<uint32_t>(n + 1);
  s->list1 = c.take<uint32_t>(std::min(n, nrows));
  s->list2 = c.take<uint32_t>(n);
  s->out = c.take<uint32_t>(2 * nrows);
  size_t at = c.used;
  s->ok = c.take<uint8_t>(n);
  s->counts = c.take<uint32_t>(2);
  s->zero_bytes = c.used - at;
  at = c.used;
  s->pick = c.take<uint32_t>(nrows);
  s->setter = c.take<uint32_t>(nrows);
  s->tstar = c.take<uint32_t>(nslots);
  s->claim = c.take<uint32_t>(ag::kPipeShreds * nrows);
  s->none_bytes = c.used - at;
  return c.used;
}

// The scratch sections into the kernels' parameter block.
inline void bind_scratch(const IntakeScratch& s, IntakeParams* params) {
  IntakeParams& p = *params;
  p.wire = s.wire;
  p.slot = s.cols.slot;
  p.slice_index = s.cols.slice_index;
  p.height = s.cols.height;
  p.row = s.row;
  p.meta = s.meta;
  p.plausible = s.plausible;
  p.roots = s.roots;
  p.commit = s.commit;
  p.ok = s.ok;
  p.list1 = s.list1;
  p.list2 = s.list2;
  p.counts = s.counts;
  p.pick = s.pick;
  p.setter = s.setter;
  p.tstar = s.tstar;
  p.claim = s.claim;
  p.out = s.out;
}

}  // namespace host
}  // namespace ag
