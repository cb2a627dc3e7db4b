// Host side of ag_repair_intake_batch (include/alpenglow_rs.h section 11): the argument checks,
// the upload of the blocks' slots, the carve-up of the context's repair scratch (intake's layout
// plus a key row per reply) and the fixed chain of launches -- the wire parse (wire.hip), the
// repair kernels (repair.hip), the Merkle root derivation (merkle.hip), at most two Ed25519
// verify launches (ed25519.hip) and the dissemination intake's own setter, claim, route and
// finalize (intake.hip).  Every launch is made whatever the replies hold; ordering is the stream's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/alpenglow_rs.h"
#include "ed25519.hpp"
#include "intake.hpp"
#include "intake_scratch.hpp"
#include "merkle.hpp"
#include "repair.hpp"
#include "rs_ctx.hpp"
#include "shredder.hpp"
#include "wire.hpp"

using namespace ag::host;

int ag_repair_intake_batch(ag_rs_ctx* c, size_t nblocks, const uint64_t* block_slots, const uint8_t* pks,
                           size_t slices_per_block, size_t n, const uint8_t* rx, size_t rx_stride,
                           const uint32_t* rx_lens, const uint32_t* req_block, const uint32_t* req_slice,
                           const uint32_t* req_index, const uint8_t* slice_roots, const uint8_t* have_root,
                           uint8_t* packets, size_t packet_stride, uint32_t* packet_lens, uint8_t* commitments,
                           uint8_t* signatures, uint32_t* shred_bytes, int32_t* last_slice, uint8_t* verdict,
                           uint32_t* shred_bytes_out, uint32_t* counts_out) {
  size_t need = 0;
  if (!c || nblocks == 0 || nblocks >= kIntakeMax || slices_per_block == 0 ||
      slices_per_block > ag::kMaxSlicesPerBlock || nblocks * slices_per_block >= kIntakeMax || n >= kIntakeMax ||
      !block_slots || !pks || !slice_roots || !have_root || !packets || !packet_lens || !commitments || !signatures ||
      !shred_bytes || !last_slice || (n && (!rx || !rx_lens || !req_block || !req_slice || !req_index || !verdict)) ||
      ag_shred_datagram_bytes(AG_RS_MAX_DATA_PER_SHRED, ag::kPipeHeight, &need) || packet_stride < need ||
      packet_stride % 16 || reinterpret_cast<uintptr_t>(packets) % 16 ||
      (n && (rx_stride < need || rx_stride % 16 || reinterpret_cast<uintptr_t>(rx) % 16)))
    return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t nrows = nblocks * slices_per_block;
  if (c->enter()) return AG_RS_ERR_DEVICE;

  int st;
  uint64_t* slots = nullptr;
  if ((st = c->repair_blocks.host(8 * nblocks, &slots))) return st;
  std::memcpy(slots, block_slots, 8 * nblocks);
  if ((st = c->repair_blocks.send(8 * nblocks, c->stream))) return st;
  IntakeScratch s;
  const size_t shared = carve(nullptr, n, nrows, nblocks, &s);  // then the key rows
  if ((st = c->d_repair.ensure(shared + (32 * n + 255) / 256 * 256, c->stream))) return st;
  carve(c->d_repair.as<uint8_t>(), n, nrows, nblocks, &s);
  if ((st = c->h_repair.ensure(8 * nrows))) return st;
  hipStream_t q = c->stream;

  ag::RepairParams p{};
  p.in.n = n;
  p.in.nslots = static_cast<uint32_t>(nblocks);
  p.in.spp = static_cast<uint32_t>(slices_per_block);
  p.in.nrows = static_cast<uint32_t>(nrows);
  p.in.rx = rx;
  p.in.rx_stride = rx_stride;
  p.in.rx_lens = rx_lens;
  p.in.packets = packets;
  p.in.packet_stride = packet_stride;
  p.in.packet_lens = packet_lens;
  p.in.commitments = commitments;
  p.in.shred_bytes = shred_bytes;
  p.in.last_slice = last_slice;
  p.in.verdict = verdict;
  bind_scratch(s, &p.in);
  p.block_slots = c->repair_blocks.dev.as<uint64_t>();
  p.req_block = req_block;
  p.req_slice = req_slice;
  p.req_index = req_index;
  p.pks = pks;
  p.slice_roots = slice_roots;
  p.have_root = have_root;
  p.signatures = signatures;
  p.sig = s.cols.sig;
  p.keys = c->d_repair.as<uint8_t>() + shared;
  p.ok = s.ok;

  AG_HIP(hipMemsetAsync(s.ok, 0, s.zero_bytes, q));
  AG_HIP(hipMemsetAsync(s.pick, 0xFF, s.none_bytes, q));
  if (n) {
    if ((st = ensure_ed_base(c))) return st;
    // parse + key: the replies' fields, then verdicts 1-4 and the request's row
    AG_HIP(ag::launch_shred_deserialize(rx, rx_stride, rx_lens, n, s.cols, s.wire, q));
    AG_HIP(ag::launch_repair_key(p, q));
    // the root of every plausible reply (leaves of their own sizes) against the proved one;
    // only then the rows' picks
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
    AG_HIP(ag::launch_merkle_verify(mv, q));
    AG_HIP(ag::launch_repair_root(p, q));
    AG_HIP(ag::launch_repair_picks(p, q));
    // the picks' signatures, then every reply that is not byte for byte a pair known valid,
    // each under its block's key
    ag::EdVerifyParams ev{};
    ev.pks = p.keys;
    ev.pk_stride = 32;
    ev.msgs = s.commit;
    ev.msg_stride = ag::kIntakeCommitStride;
    ev.msg_len = ag::kSliceCommitmentLen;
    ev.sigs = s.cols.sig;
    ev.sig_stride = 64;
    ev.ok = s.ok;
    ev.base_table = c->d_ed_base.as<int32_t>();
    ev.n = std::min(n, nrows);
    ev.list = s.list1;
    ev.list_count = s.counts;
    AG_HIP(ag::launch_ed25519_verify(ev, q));
    AG_HIP(ag::launch_repair_classify(p, q));
    ev.n = n;
    ev.list = s.list2;
    ev.list_count = s.counts + 1;
    AG_HIP(ag::launch_ed25519_verify(ev, q));
    AG_HIP(ag::launch_intake_setter(p.in, q));
    AG_HIP(ag::launch_repair_accept(p, q));
    // last slice per block, the claim of the datagram slots, the copies: as intake
    AG_HIP(ag::launch_intake_claim(p.in, q));
    AG_HIP(ag::launch_intake_route(p.in, q));
  }
  AG_HIP(ag::launch_repair_signatures(p, q));
  AG_HIP(ag::launch_intake_finalize(p.in, q));
  uint32_t* h = c->h_repair.as<uint32_t>();
  AG_HIP(hipMemcpyAsync(h, s.out, 8 * nrows, hipMemcpyDeviceToHost, q));
  AG_HIP(hipStreamSynchronize(q));
  if (shred_bytes_out) std::memcpy(shred_bytes_out, h, 4 * nrows);
  if (counts_out) std::memcpy(counts_out, h + nrows, 4 * nrows);
  return AG_RS_OK;
}
