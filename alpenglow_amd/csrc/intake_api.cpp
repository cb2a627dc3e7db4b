// Host side of ag_shredder_intake_batch (include/alpenglow_rs.h section 10): the argument
// checks, the window upload, the carve-up of the context's intake scratch and the fixed chain of
// launches -- the wire parse (wire.hip), the intake kernels (intake.hip), the Merkle root
// derivation (merkle.hip) and at most two Ed25519 verify launches (ed25519.hip).  Every launch
// is made whatever the datagrams hold; ordering is the stream's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "ed25519.hpp"
#include "intake.hpp"
#include "intake_scratch.hpp"
#include "merkle.hpp"
#include "rs_ctx.hpp"
#include "shredder.hpp"
#include "wire.hpp"

using namespace ag::host;

int ag_shredder_intake_batch(ag_rs_ctx* c, size_t nslots, const uint64_t* slot_ids, size_t slices_per_slot, size_t n,
                             const uint8_t* rx, size_t rx_stride, const uint32_t* rx_lens, const uint8_t* pk,
                             uint8_t* packets, size_t packet_stride, uint32_t* packet_lens, uint8_t* commitments,
                             uint32_t* shred_bytes, int32_t* last_slice, uint8_t* verdict, uint32_t* shred_bytes_out,
                             uint32_t* counts_out) {
  if (!c || nslots == 0 || nslots >= kIntakeMax || slices_per_slot == 0 ||
      slices_per_slot > ag::kMaxSlicesPerBlock || nslots * slices_per_slot >= kIntakeMax || n >= kIntakeMax ||
      !slot_ids || !packets || !packet_lens || !commitments || !shred_bytes || !last_slice ||
      (n && (!rx || !rx_lens || !pk || !verdict)) || !intake_buffers_ok(packets, packet_stride, n, rx, rx_stride))
    return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t nrows = nslots * slices_per_slot;
  // the window sorted by slot id (the kernels search it), each id with the caller's index
  std::vector<uint32_t> order(nslots);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return slot_ids[a] < slot_ids[b]; });
  for (size_t i = 1; i < nslots; ++i)
    if (slot_ids[order[i]] == slot_ids[order[i - 1]]) return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;

  int st;
  uint8_t* win = nullptr;
  if ((st = c->intake_win.host(12 * nslots, &win))) return st;
  for (size_t i = 0; i < nslots; ++i) {
    reinterpret_cast<uint64_t*>(win)[i] = slot_ids[order[i]];
    reinterpret_cast<uint32_t*>(win + 8 * nslots)[i] = order[i];
  }
  if ((st = c->intake_win.send(12 * nslots, c->stream))) return st;
  IntakeScratch s;
  if ((st = intake_scratch(c, n, nrows, nslots, 0, &s))) return st;
  hipStream_t q = c->stream;

  ag::IntakeParams p{};
  p.n = n;
  p.nslots = static_cast<uint32_t>(nslots);
  p.spp = static_cast<uint32_t>(slices_per_slot);
  p.nrows = static_cast<uint32_t>(nrows);
  p.win_ids = c->intake_win.dev.as<uint64_t>();
  p.win_w = reinterpret_cast<const uint32_t*>(c->intake_win.dev.as<uint8_t>() + 8 * nslots);
  p.rx = rx;
  p.rx_stride = rx_stride;
  p.rx_lens = rx_lens;
  p.packets = packets;
  p.packet_stride = packet_stride;
  p.packet_lens = packet_lens;
  p.commitments = commitments;
  p.shred_bytes = shred_bytes;
  p.last_slice = last_slice;
  p.verdict = verdict;
  bind_scratch(s, &p);

  if ((st = clear_scratch(s, q))) return st;
  if (n) {
    if ((st = ensure_ed_base(c))) return st;
    // parse + key: the datagrams' fields (payload, signature and path to aligned scratch rows),
    // then verdicts 1-3, the window row and the rows' picks
    AG_HIP(ag::launch_shred_deserialize(rx, rx_stride, rx_lens, n, s.cols, s.wire, q));
    AG_HIP(ag::launch_intake_key(p, q));
    // root and commitment of every plausible datagram (leaves of their own sizes)
    AG_HIP(ag::launch_merkle_verify(root_derivation(s, n), q));
    AG_HIP(ag::launch_intake_commit(p, q));
    // cache resolution: the picks' signatures, then everything not equal to a valid cache
    ag::EdVerifyParams ev = commitment_verify(s, c->d_ed_base.as<int32_t>());
    ev.pks = pk;
    ev.pk_stride = 0;
    ev.n = std::min(n, nrows);
    ev.list = s.list1;
    ev.list_count = s.counts;
    AG_HIP(ag::launch_ed25519_verify(ev, q));
    AG_HIP(ag::launch_intake_classify(p, q));
    ev.n = n;
    ev.list = s.list2;
    ev.list_count = s.counts + 1;
    AG_HIP(ag::launch_ed25519_verify(ev, q));
    AG_HIP(ag::launch_intake_setter(p, q));
    AG_HIP(ag::launch_intake_accept(p, q));
    // last slice per slot, the claim of the datagram slots, the copies
    AG_HIP(ag::launch_intake_claim(p, q));
    AG_HIP(ag::launch_intake_route(p, q));
  }
  AG_HIP(ag::launch_intake_finalize(p, q));
  return read_back(c, s, nrows, shred_bytes_out, counts_out);
}
