// channelizer.h -- the wideband channelizer's launchers (channelizer.hip: integer decimation; channelizer_rate.hip: rational
// rate change up / down).  Its per-context state (parameter and filter-bank buffers, page-locked slots, events) are the
// chan_* / ev_chan* members of the context, shared by both forms.
#pragma once
#include "lcs_internal.h"

void lcs_chan_taps(int decim, double *taps /*[16*decim]*/);      // any decim >= 2
unsigned long long lcs_chan_step(double f_shift, double fs_in);
int lcs_chan_slot(lcs_ctx *c, size_t bytes, int *slot);          // the next page-locked parameter slot, free to be written
int lcs_launch_channelize(lcs_ctx *c, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int decim, const double *f_shift,
                          int n_ch, void *d_out, uint32_t n_out);
int lcs_launch_channelize_rational(lcs_ctx *c, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int up, int down,
                                   const double *f_shift, int n_ch, void *d_out, uint32_t n_out);
int lcs_chan_last_ms(lcs_ctx *c, float *ms);   // HIP-event time of the context's last channelizer launch (either form)

// sample n of a capture of format FMT as (re, im) floats
template <int FMT>
__device__ __forceinline__ float2 chan_sample(const void *x, unsigned long long n) {
  if (FMT == LCS_FMT_C64) return ((const float2 *)x)[n];
  if (FMT == LCS_FMT_IQ_S16) {
    const uint32_t p = ((const uint32_t *)x)[n];
    return make_float2((float)(int)(int16_t)(p & 0xFFFFu) * (1.f / 32768.f), (float)(int)(int16_t)(p >> 16) * (1.f / 32768.f));
  }
  const uint32_t p = ((const uint16_t *)x)[n];
  return make_float2((float)(int)(int8_t)(p & 255u) * (1.f / 128.f), (float)(int)(int8_t)(p >> 8) * (1.f / 128.f));
}
