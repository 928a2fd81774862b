// LDS ring layout of paged_attention_v4r_kernel (attention_decode.hip).
//
// A page is 16 tokens x 128 dims of bf16: 4 KiB of K and 4 KiB of V, each 256
// chunks of 16 bytes; chunk (tok, dc) of the page in memory is tok * 16 + dc.
// A ring slot holds one page, K in its first 4 KiB and V in its second. Four
// waves fill a slot half with one direct-to-LDS 16-byte load each: lane i of
// wave w writes LDS chunk w * 64 + i, so where a source chunk lands is chosen
// by which source chunk that lane loads.
//  - V lands as it lies in memory. A wave's PV read (lane -> token vtok +
//    4 * q4, dims 8 * (lane & 15)) is then 16 lanes on 256 contiguous bytes.
//  - K: lane (tok, part) of the QK layout reads the four chunks
//    part * 4 + c of row tok, 64 bytes apart from lane to lane; chunk dc of
//    row tok is therefore stored at dc ^ (tok & 3), which puts the 16 lanes
//    of four consecutive tokens on 16 different 16-byte columns.
// Plain host/device functions so that tests/test_gpu_attention_ring.py can
// check the maps without a GPU (tests/ring_layout_check.cpp).
#pragma once

#ifndef KS_HD
#ifdef __HIPCC__
#define KS_HD __host__ __device__
#else
#define KS_HD
#endif
#endif

namespace ring_layout {

constexpr int CHUNK = 16;             // bytes per lane per load
constexpr int HALF_BYTES = 4096;      // K or V of one page
constexpr int SLOT_BYTES = 2 * HALF_BYTES;
constexpr int ROW_CHUNKS = 16;        // chunks per token row

// where source chunk (tok, dc) of a K page sits in its slot half
KS_HD constexpr int k_lds_chunk(int tok, int dc) {
  return tok * ROW_CHUNKS + (dc ^ (tok & 3));
}

// byte offset in the source page half that lane `lane` of wave `wave` loads;
// it lands at byte (wave * 64 + lane) * CHUNK of the slot half
KS_HD constexpr int k_src_byte(int wave, int lane) {
  const int p = wave * 64 + lane;
  const int tok = p / ROW_CHUNKS;
  return (tok * ROW_CHUNKS + ((p % ROW_CHUNKS) ^ (tok & 3))) * CHUNK;
}
KS_HD constexpr int v_src_byte(int wave, int lane) {
  return (wave * 64 + lane) * CHUNK;
}

// byte offset in the slot's K half of kreg[c] of lane `lane`
// (tok = lane >> 2, part = lane & 3; v4p loads source chunk part * 4 + c)
KS_HD constexpr int k_read_byte(int lane, int c) {
  return k_lds_chunk(lane >> 2, (lane & 3) * 4 + c) * CHUNK;
}
// byte offset in the slot's V half of vreg[q4] of lane `lane`
// (v4p loads row (lane >> 4) + 4 * q4, chunk lane & 15)
KS_HD constexpr int v_read_byte(int lane, int q4) {
  return (((lane >> 4) + 4 * q4) * ROW_CHUNKS + (lane & 15)) * CHUNK;
}

}  // namespace ring_layout
