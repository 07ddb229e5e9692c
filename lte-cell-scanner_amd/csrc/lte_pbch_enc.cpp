// lte_pbch_enc.cpp -- the PBCH of one 40 ms period from the fields of a decoded record: the transmit side of decode_mib, for the
// cancellation stage (sic.hip).  36.331 MasterInformationBlock (dl-Bandwidth 3 bits, phich-Duration 1, phich-Resource 2, the
// 8 most significant bits of the SFN, 10 spare), 36.212 5.3.1.1 (CRC16 xor the antenna mask), 5.1.3.1 (tail-biting
// convolutional code, K = 7, G = 133 171 165), 5.1.4.2 (rate matching to 1920 / 1728 bits), 36.211 6.6.1 (scrambling with
// c_init = n_id_cell), 6.6.2 (QPSK).  tests/test_sic_host.py pins it to synth.pbch_symbols, the encoder the decoder's tests use.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "lcs_internal.h"

namespace lcs_tables {

// sfn: any frame of the period (its two low bits are not sent).  out: 960 (normal CP) or 864 (extended) QPSK symbols as
// (re, im) pairs; quarter q of them goes out in the frame with sfn mod 4 == q.  false: a field no MIB can carry.
bool pbch_encode(int n_id_cell, int n_ports, int n_rb_dl, int phich_duration, int phich_resource, int sfn, int cp_type, double *out_re_im) {
  static const int bw[6] = {6, 15, 25, 50, 75, 100};
  int bw_idx = -1;
  for (int i = 0; i < 6; ++i) if (bw[i] == n_rb_dl) bw_idx = i;
  if (bw_idx < 0 || (n_ports != 1 && n_ports != 2 && n_ports != 4) || phich_duration < 1 || phich_duration > 2 || phich_resource < 1 ||
      phich_resource > 4 || n_id_cell < 0 || n_id_cell > 503 || (cp_type != LCS_CP_NORMAL && cp_type != LCS_CP_EXTENDED))
    return false;
  uint8_t c[40];
  std::memset(c, 0, sizeof(c));
  c[0] = (bw_idx >> 2) & 1; c[1] = (bw_idx >> 1) & 1; c[2] = bw_idx & 1;
  c[3] = phich_duration == 2;
  c[4] = ((phich_resource - 1) >> 1) & 1; c[5] = (phich_resource - 1) & 1;
  const int sfn8 = (sfn >> 2) & 0xff;
  for (int i = 0; i < 8; ++i) c[6 + i] = (sfn8 >> (7 - i)) & 1;
  // CRC-16-CCITT over the 24 bits, zero initial state, MSB first; the mask of the port count (36.212 table 5.3.1.1-1)
  unsigned reg = 0;
  for (int i = 0; i < 24; ++i) {
    const unsigned top = ((reg >> 15) & 1u) ^ c[i];
    reg = (reg << 1) & 0xffffu;
    if (top) reg ^= 0x1021u;
  }
  for (int i = 0; i < 16; ++i) {
    uint8_t b = (reg >> (15 - i)) & 1u;
    if (n_ports == 2) b ^= 1;
    else if (n_ports == 4) b ^= (uint8_t)(i & 1);
    c[24 + i] = b;
  }
  // the register starts with the last six bits; bit 6 of `r` is the input, bits 5..0 the six before it, newest first
  static const unsigned G[3] = {0133, 0171, 0165};
  uint8_t d[3][40];
  unsigned state = 0;
  for (int i = 34; i < 40; ++i) state = (state >> 1) | ((unsigned)c[i] << 5);
  for (int k = 0; k < 40; ++k) {
    const unsigned r = ((unsigned)c[k] << 6) | state;
    for (int j = 0; j < 3; ++j) d[j][k] = (uint8_t)(__builtin_popcount(r & G[j]) & 1);
    state = r >> 1;
  }
  // sub-block interleaver: 2 rows of 32 columns, 24 nulls in front, columns permuted, read column by column
  static const int perm[32] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
  int8_t w[3 * 64];
  for (int s = 0; s < 3; ++s)
    for (int col = 0; col < 32; ++col)
      for (int row = 0; row < 2; ++row) {
        const int y = row * 32 + perm[col] - 24;      // index into d, negative: a null
        w[s * 64 + col * 2 + row] = y < 0 ? (int8_t)-1 : (int8_t)d[s][y];
      }
  const int n_e = cp_type == LCS_CP_NORMAL ? 1920 : 1728;
  static thread_local uint8_t e[1920], scr[1920];
  for (int k = 0, j = 0; k < n_e; j = (j + 1) % 192)
    if (w[j] >= 0) e[k++] = (uint8_t)w[j];
  lte_pn((uint32_t)n_id_cell, (uint32_t)n_e, scr);
  const double a = 1.0 / std::sqrt(2.0);      // (1 - 2 b) / sqrt(2), the quotient synth forms: one ulp below sqrt(1 / 2)
  for (int i = 0; i < n_e / 2; ++i) {
    out_re_im[2 * i] = (e[2 * i] ^ scr[2 * i]) ? -a : a;
    out_re_im[2 * i + 1] = (e[2 * i + 1] ^ scr[2 * i + 1]) ? -a : a;
  }
  return true;
}

}  // namespace lcs_tables
