// Host side of ag_repair_intake_batch (include/alpenglow_rs.h section 11): the argument checks,
// the upload of the blocks' slots, the carve-up of the context's intake scratch (intake's layout
// plus a key row per reply; intake_scratch.hpp) and the fixed chain of launches -- the wire parse (wire.hip), the
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
  if (!c || nblocks == 0 || nblocks >= kIntakeMax || slices_per_block == 0 ||
      slices_per_block > ag::kMaxSlicesPerBlock || nblocks * slices_per_block >= kIntakeMax || n >= kIntakeMax ||
      !block_slots || !pks || !slice_roots || !have_root || !packets || !packet_lens || !commitments || !signatures ||
      !shred_bytes || !last_slice || (n && (!rx || !rx_lens || !req_block || !req_slice || !req_index || !verdict)) ||
      !intake_buffers_ok(packets, packet_stride, n, rx, rx_stride))
    return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t nrows = nblocks * slices_per_block;
  if (c->enter()) return AG_RS_ERR_DEVICE;

  int st;
  uint64_t* slots = nullptr;
  if ((st = c->intake_win.host(8 * nblocks, &slots))) return st;
  std::memcpy(slots, block_slots, 8 * nblocks);
  if ((st = c->intake_win.send(8 * nblocks, c->stream))) return st;
  IntakeScratch s;
  if ((st = intake_scratch(c, n, nrows, nblocks, n, &s))) return st;  // intake's layout, then a key row per reply
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
  p.block_slots = c->intake_win.dev.as<uint64_t>();
  p.req_block = req_block;
  p.req_slice = req_slice;
  p.req_index = req_index;
  p.pks = pks;
  p.slice_roots = slice_roots;
  p.have_root = have_root;
  p.signatures = signatures;
  p.sig = s.cols.sig;
  p.keys = s.keys;
  p.ok = s.ok;

  if ((st = clear_scratch(s, q))) return st;
  if (n) {
    if ((st = ensure_ed_base(c))) return st;
    // parse + key: the replies' fields, then verdicts 1-4 and the request's row
    AG_HIP(ag::launch_shred_deserialize(rx, rx_stride, rx_lens, n, s.cols, s.wire, q));
    AG_HIP(ag::launch_repair_key(p, q));
    // the root of every plausible reply (leaves of their own sizes) against the proved one;
    // only then the rows' picks
    AG_HIP(ag::launch_merkle_verify(root_derivation(s, n), q));
    AG_HIP(ag::launch_repair_root(p, q));
    AG_HIP(ag::launch_repair_picks(p, q));
    // the picks' signatures, then every reply that is not byte for byte a pair known valid,
    // each under its block's key
    ag::EdVerifyParams ev = commitment_verify(s, c->d_ed_base.as<int32_t>());
    ev.pks = p.keys;
    ev.pk_stride = 32;
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
  return read_back(c, s, nrows, shred_bytes_out, counts_out);
}
