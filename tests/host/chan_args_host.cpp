// Host-side call of the channelizer's refusal rules (channelizer.h: chan_refusal), the very routine the three entry points of
// lcs_api.hip go by.  tests/test_channelizer_args_host.py holds the texts.  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/channelizer.h"

// the pointers are only looked at (null, alignment), f_shift is read; decim_form: lcs_channelize's rules (up is taken as 1)
extern "C" const char *chan_args_refusal(int decim_form, unsigned long long d_wide, int fmt, unsigned long long n_in, double fs_in, int up, int down,
                                         const double *f_shift, int n_ch, unsigned long long d_out, unsigned n_out) {
  const ChanCall a = {reinterpret_cast<const void *>(d_wide), fmt, n_in, fs_in, decim_form ? 1 : up, down, f_shift, n_ch, reinterpret_cast<void *>(d_out), n_out};
  return chan_refusal(a, decim_form ? CHAN_DECIM : CHAN_RATE);
}
