// Host-side calls of the 8-bit channelizer output's two rules (channelizer.h: chan_u8_exponent, chan_u8_code), the very functions
// k_chan_quant_u8 runs on the device.  tests/test_channelizer_u8_host.py compares them with their numpy restatement
// (tests/chan_u8_ref.py).  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/channelizer.h"

extern "C" void chan_u8_host_exponents(const double *P, int n, int *e) {
  for (int i = 0; i < n; ++i) e[i] = chan_u8_exponent(P[i]);
}

extern "C" void chan_u8_host_codes(const float *z, int n, unsigned char *code) {
  for (int i = 0; i < n; ++i) code[i] = (unsigned char)chan_u8_code(z[i]);
}
