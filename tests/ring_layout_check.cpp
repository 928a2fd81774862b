// Host program over kserve_amd/ops/csrc/attn_ring_layout.h, the lane maps the
// LDS-ring decode attention kernel is built from. Prints them for
// tests/test_gpu_attention_ring.py and checks them itself, so that a build
// with -fsanitize=address,undefined has something to trip over:
//   K <wave> <lane> <source byte> <LDS byte>     one line per fetching lane
//   V <wave> <lane> <source byte> <LDS byte>
//   k <lane> <c> <LDS byte>                       one line per operand read
//   v <lane> <q4> <LDS byte>
#include <cstdio>
#include <vector>

#include "attn_ring_layout.h"

int main() {
  using namespace ring_layout;
  std::vector<int> k_at(HALF_BYTES, -1), v_at(HALF_BYTES, -1);
  int bad = 0;
  for (int w = 0; w < 4; ++w)
    for (int l = 0; l < 64; ++l) {
      const int dst = (w * 64 + l) * CHUNK;
      const int ks = k_src_byte(w, l), vs = v_src_byte(w, l);
      std::printf("K %d %d %d %d\nV %d %d %d %d\n", w, l, ks, dst, w, l, vs,
                  dst);
      for (int b = 0; b < CHUNK; ++b) {
        bad += k_at.at(dst + b) != -1 || v_at.at(dst + b) != -1;
        bad += ks < 0 || ks + CHUNK > HALF_BYTES;
        bad += vs < 0 || vs + CHUNK > HALF_BYTES;
        k_at.at(dst + b) = ks + b;
        v_at.at(dst + b) = vs + b;
      }
    }
  for (int l = 0; l < 64; ++l)
    for (int c = 0; c < 4; ++c) {
      const int kr = k_read_byte(l, c), vr = v_read_byte(l, c);
      std::printf("k %d %d %d\nv %d %d %d\n", l, c, kr, l, c, vr);
      // v4p: kreg[c] = K[tok = l >> 2][(l & 3) * 32 + c * 8 ..], and
      // vreg[c] = V[(l >> 4) + 4 * c][(l & 15) * 8 ..], 2 bytes an element
      const int k_want = ((l >> 2) * 128 + (l & 3) * 32 + c * 8) * 2;
      const int v_want = (((l >> 4) + 4 * c) * 128 + (l & 15) * 8) * 2;
      for (int b = 0; b < CHUNK; ++b) {
        bad += k_at.at(kr + b) != k_want + b;
        bad += v_at.at(vr + b) != v_want + b;
      }
    }
  std::printf("bad %d\n", bad);
  return bad != 0;
}
