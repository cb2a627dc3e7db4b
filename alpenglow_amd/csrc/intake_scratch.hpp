// What the two intake calls (intake_api.cpp, repair_api.cpp) share on the host: the scratch of
// one call, carved out of the context's d_intake, and the pieces of their chains that read only
// that scratch -- the datagram buffers' argument check, the two memsets, the root derivation's
// and the signature checks' parameters, the read-back.  Both calls end in a stream
// synchronisation, so neither holds the scratch, the staged window or the pinned outputs past its
// return.  Host only.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "ed25519.hpp"
#include "intake.hpp"
#include "merkle.hpp"
#include "rs_ctx.hpp"
#include "shredder.hpp"
#include "wire.hpp"

namespace ag {
namespace host {

constexpr size_t kIntakeMax = size_t{1} << 24;  // datagrams per call, rows per window
constexpr size_t kProofBytes = 32 * ag::kPipeHeight;

// The store's datagram slots and the received datagrams: strides that hold the largest datagram,
// 16-byte aligned rows.
inline bool intake_buffers_ok(const uint8_t* packets, size_t packet_stride, size_t n, const uint8_t* rx,
                              size_t rx_stride) {
  size_t need = 0;
  return !ag_shred_datagram_bytes(AG_RS_MAX_DATA_PER_SHRED, ag::kPipeHeight, &need) && packet_stride >= need &&
         packet_stride % 16 == 0 && reinterpret_cast<uintptr_t>(packets) % 16 == 0 &&
         (n == 0 || (rx_stride >= need && rx_stride % 16 == 0 && reinterpret_cast<uintptr_t>(rx) % 16 == 0));
}

struct IntakeScratch {
  ag::ShredColumns cols{};
  uint8_t *wire, *plausible, *roots, *commit, *ok;
  uint32_t *row, *meta, *mlist, *list1, *list2, *counts, *pick, *out;
  size_t zero_bytes, none_bytes;  // [ok, counts] is one zeroed span, [pick .. claim] one of kIntakeNone
  uint32_t *setter, *tstar, *claim;
  uint8_t* keys;  // repair: the verifying key of each reply's block (32-byte rows)
};

// Lays the sections out from `base` (null: only the size is wanted); returns the bytes used.
inline size_t carve(uint8_t* base, size_t n, size_t nrows, size_t nslots, size_t key_rows, IntakeScratch* s) {
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
  s->keys = c.take<uint8_t>(32 * key_rows);
  return c.used;
}

// One call's scratch: d_intake grown to the layout's size and carved, the pinned staging of the
// per-row outputs grown beside it.
inline int intake_scratch(ag_rs_ctx* c, size_t n, size_t nrows, size_t nslots, size_t key_rows, IntakeScratch* s) {
  int st;
  if ((st = c->d_intake.ensure(carve(nullptr, n, nrows, nslots, key_rows, s), c->stream)) ||
      (st = c->h_intake.ensure(8 * nrows)))
    return st;
  carve(c->d_intake.as<uint8_t>(), n, nrows, nslots, key_rows, s);
  return AG_RS_OK;
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

// The two memsets every call starts with: the ok flags and the list counts to zero, the picks,
// setters, last slices and claims to kIntakeNone.
inline int clear_scratch(const IntakeScratch& s, hipStream_t q) {
  AG_HIP(hipMemsetAsync(s.ok, 0, s.zero_bytes, q));
  AG_HIP(hipMemsetAsync(s.pick, 0xFF, s.none_bytes, q));
  return AG_RS_OK;
}

// The root of every plausible datagram, derived from its parsed payload (a leaf of its own size)
// and path.
inline ag::MerkleVerifyParams root_derivation(const IntakeScratch& s, size_t n) {
  ag::MerkleVerifyParams mv{};
  mv.leaves = s.cols.data;
  mv.leaf_stride = s.cols.data_stride;
  mv.height = ag::kPipeHeight;
  mv.index = s.cols.shred_index;
  mv.proofs = s.cols.proof;
  mv.proofs_stride = kProofBytes;
  mv.n = n;
  mv.roots_out = s.roots;
  mv.active = s.plausible;
  mv.list = s.mlist;
  mv.leaf_sizes = s.cols.data_len;
  mv.size_group = 1;
  return mv;
}

// The signature checks over the datagrams' commitments and parsed signatures into s.ok; the
// caller sets the keys (pks, pk_stride) and, per launch, n and the list.
inline ag::EdVerifyParams commitment_verify(const IntakeScratch& s, const int32_t* base_table) {
  ag::EdVerifyParams ev{};
  ev.msgs = s.commit;
  ev.msg_stride = ag::kIntakeCommitStride;
  ev.msg_len = ag::kSliceCommitmentLen;
  ev.sigs = s.cols.sig;
  ev.sig_stride = 64;
  ev.ok = s.ok;
  ev.base_table = base_table;
  return ev;
}

// The rows' shred sizes and counts (s.out, written by launch_intake_finalize) to the host; ends
// the call: the stream is synchronised.
inline int read_back(ag_rs_ctx* c, const IntakeScratch& s, size_t nrows, uint32_t* shred_bytes_out,
                     uint32_t* counts_out) {
  uint32_t* h = c->h_intake.as<uint32_t>();
  AG_HIP(hipMemcpyAsync(h, s.out, 8 * nrows, hipMemcpyDeviceToHost, c->stream));
  AG_HIP(hipStreamSynchronize(c->stream));
  if (shred_bytes_out) std::memcpy(shred_bytes_out, h, 4 * nrows);
  if (counts_out) std::memcpy(counts_out, h + nrows, 4 * nrows);
  return AG_RS_OK;
}

}  // namespace host
}  // namespace ag
