// The C ABI of the shred wire format and the slice framing (include/alpenglow_rs.h): argument
// checks and metadata staging in front of the kernels of wire.hip and slice.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/alpenglow_rs.h"
#include "rs_ctx.hpp"
#include "slice.hpp"
#include "wire.hpp"

using namespace ag::host;

// ---- shred wire format ----------------------------------------------------------------

namespace {
bool columns_ok(const ag_shred_columns* c) {
  return c && c->kind && c->slot && c->slice_index && c->is_last && c->shred_index && c->data_len && c->sig &&
         c->height && (c->data || c->data_stride == 0) && (c->proof || c->proof_stride == 0);
}
ag::ShredColumns to_columns(const ag_shred_columns* c) {
  ag::ShredColumns r{};
  r.kind = c->kind;
  r.slot = c->slot;
  r.slice_index = c->slice_index;
  r.is_last = c->is_last;
  r.shred_index = c->shred_index;
  r.data = c->data;
  r.data_stride = c->data_stride;
  r.data_len = c->data_len;
  r.sig = c->sig;
  r.proof = c->proof;
  r.proof_stride = c->proof_stride;
  r.height = c->height;
  return r;
}
}  // namespace

extern "C" {

int ag_shred_deserialize_batch(ag_rs_ctx* c, size_t n, const uint8_t* packets, size_t packet_stride,
                               const uint32_t* packet_lens, const ag_shred_columns* cols, uint8_t* status) {
  if (!c || n >= kMaxSigBatch || (n && (!packets || !packet_lens || !status || !columns_ok(cols))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  return ag::launch_shred_deserialize(packets, packet_stride, packet_lens, n, to_columns(cols), status, c->stream) ==
                 hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_shred_serialize_batch(ag_rs_ctx* c, size_t n, const ag_shred_columns* cols, uint8_t* packets,
                             size_t packet_stride, uint32_t* packet_lens) {
  if (!c || n >= kMaxSigBatch || (n && (!packets || !packet_lens || !columns_ok(cols))))
    return AG_RS_ERR_INVALID_ARGUMENT;
  if (n == 0) return AG_RS_OK;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  return ag::launch_shred_serialize(to_columns(cols), n, packets, packet_stride, packet_lens, c->stream) ==
                 hipSuccess
             ? AG_RS_OK
             : AG_RS_ERR_DEVICE;
}

int ag_shred_datagram_bytes(size_t shred_bytes, size_t proof_len, size_t* out) {
  if (!out || shred_bytes > ag::kMtuBytes || proof_len > ag::kMtuBytes / 32) return AG_RS_ERR_INVALID_ARGUMENT;
  const size_t len = ag::kShredHeadBytes + shred_bytes + 64 + 8 + 32 * proof_len;
  if (len > ag::kMtuBytes) return AG_RS_ERR_INVALID_ARGUMENT;
  *out = len;
  return AG_RS_OK;
}

int ag_slice_frame_batch(ag_rs_ctx* c, size_t nslices, size_t shred_bytes, const uint8_t* parent_flags,
                         const uint8_t* parent_ids, const uint8_t* data, size_t data_stride, const uint32_t* data_lens,
                         uint8_t* codewords, size_t codeword_stride, uint32_t* payload_lens_out) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (!parent_flags || !parent_ids || !data_lens || !codewords || !payload_lens_out || nslices > 0x7FFFFFFFull ||
      shred_bytes == 0 || reinterpret_cast<uintptr_t>(codewords) % 4 || codeword_stride % 4 ||
      (nslices > 1 && codeword_stride < 32 * shred_bytes))
    return AG_RS_ERR_INVALID_ARGUMENT;
  size_t max_len = 0;
  for (size_t b = 0; b < nslices; ++b) {
    if (parent_flags[b] > 1) return AG_RS_ERR_INVALID_ARGUMENT;
    const size_t framed = 1 + (parent_flags[b] ? AG_SLICE_BLOCK_ID_BYTES : 0) + 8 + size_t{data_lens[b]};
    if (framed > AG_SLICE_MAX_DATA || framed >= 32 * shred_bytes) return AG_RS_ERR_TOO_MUCH_DATA;
    max_len = std::max<size_t>(max_len, data_lens[b]);
  }
  if (max_len && (!data || (nslices > 1 && data_stride < max_len))) return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  // metadata: flags | ids | lens, one upload
  const size_t off_ids = (nslices + 15) / 16 * 16, off_lens = off_ids + (nslices * AG_SLICE_BLOCK_ID_BYTES + 15) / 16 * 16;
  const size_t bytes = off_lens + 4 * nslices;
  int st = c->d_slice_meta.ensure(bytes, c->stream);
  if (st) return st;
  std::vector<uint8_t> meta(bytes, 0);
  std::memcpy(meta.data(), parent_flags, nslices);
  std::memcpy(meta.data() + off_ids, parent_ids, nslices * AG_SLICE_BLOCK_ID_BYTES);
  std::memcpy(meta.data() + off_lens, data_lens, 4 * nslices);
  AG_HIP(hipMemcpyAsync(c->d_slice_meta.ptr, meta.data(), bytes, hipMemcpyHostToDevice, c->stream));
  ag::SliceFrameParams p{};
  uint8_t* d = c->d_slice_meta.as<uint8_t>();
  p.parent_flags = d;
  p.parent_ids = d + off_ids;
  p.data_lens = reinterpret_cast<const uint32_t*>(d + off_lens);
  p.data = data;
  p.data_stride = data_stride;
  p.cw = codewords;
  p.cw_stride = codeword_stride;
  p.n = nslices;
  if (ag::launch_slice_frame(p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  AG_HIP(hipStreamSynchronize(c->stream));  // the host metadata buffer goes out of scope
  for (size_t b = 0; b < nslices; ++b)
    payload_lens_out[b] = static_cast<uint32_t>(1 + (parent_flags[b] ? AG_SLICE_BLOCK_ID_BYTES : 0) + 8 + data_lens[b]);
  return AG_RS_OK;
}

int ag_slice_parse_batch(ag_rs_ctx* c, size_t nslices, const uint8_t* codewords, size_t codeword_stride,
                         const int64_t* payload_lens, uint8_t* status, uint8_t* parent_flags, uint8_t* parent_ids,
                         uint32_t* data_offsets, uint32_t* data_lens) {
  if (!c) return AG_RS_ERR_INVALID_ARGUMENT;
  if (nslices == 0) return AG_RS_OK;
  if (!codewords || !payload_lens || !status || !parent_flags || !parent_ids || !data_offsets || !data_lens ||
      nslices > 0x7FFFFFFFull)
    return AG_RS_ERR_INVALID_ARGUMENT;
  for (size_t b = 0; b < nslices; ++b)  // the bytes parsed must lie inside the codeword
    if (nslices > 1 && payload_lens[b] > 0 && static_cast<uint64_t>(payload_lens[b]) > codeword_stride)
      return AG_RS_ERR_INVALID_ARGUMENT;
  if (c->enter()) return AG_RS_ERR_DEVICE;
  // device layout: lens (8n) | status (n) | flags (n) | ids (40n) | offsets (4n) | data lens (4n)
  const size_t o_st = 8 * nslices, o_fl = o_st + nslices, o_id = o_fl + nslices,
               o_off = (o_id + AG_SLICE_BLOCK_ID_BYTES * nslices + 3) / 4 * 4, o_len = o_off + 4 * nslices;
  const size_t bytes = o_len + 4 * nslices;
  int st = c->d_slice_meta.ensure(bytes, c->stream);
  if (st) return st;
  uint8_t* d = c->d_slice_meta.as<uint8_t>();
  AG_HIP(hipMemcpyAsync(d, payload_lens, 8 * nslices, hipMemcpyHostToDevice, c->stream));
  ag::SliceParseParams p{};
  p.cw = codewords;
  p.cw_stride = codeword_stride;
  p.payload_lens = reinterpret_cast<const int64_t*>(d);
  p.status = d + o_st;
  p.parent_flags = d + o_fl;
  p.parent_ids = d + o_id;
  p.data_offsets = reinterpret_cast<uint32_t*>(d + o_off);
  p.data_lens = reinterpret_cast<uint32_t*>(d + o_len);
  p.n = nslices;
  if (ag::launch_slice_parse(p, c->stream) != hipSuccess) return AG_RS_ERR_DEVICE;
  // read back through pinned staging (a pageable destination costs a staged copy: ~0.3 ms more
  // for a 65 536-slice batch)
  if ((st = c->h_slice_meta.ensure(bytes - o_st))) return st;
  const uint8_t* out = c->h_slice_meta.as<uint8_t>();
  AG_HIP(hipMemcpyAsync(c->h_slice_meta.ptr, d + o_st, bytes - o_st, hipMemcpyDeviceToHost, c->stream));
  AG_HIP(hipStreamSynchronize(c->stream));
  std::memcpy(status, out, nslices);
  std::memcpy(parent_flags, out + (o_fl - o_st), nslices);
  std::memcpy(parent_ids, out + (o_id - o_st), AG_SLICE_BLOCK_ID_BYTES * nslices);
  std::memcpy(data_offsets, out + (o_off - o_st), 4 * nslices);
  std::memcpy(data_lens, out + (o_len - o_st), 4 * nslices);
  return AG_RS_OK;
}

}  // extern "C"
