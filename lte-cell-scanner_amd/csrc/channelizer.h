// channelizer.h -- the wideband channelizer's launchers (channelizer.hip).  Its per-context state (parameter and filter-bank
// buffers, page-locked slots, events) are the chan_* / ev_chan* members of the context.
#pragma once
#include "lcs_internal.h"

void lcs_chan_taps(int decim, double *taps /*[16*decim]*/);
int lcs_launch_channelize(lcs_ctx *c, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int decim, const double *f_shift,
                          int n_ch, void *d_out, uint32_t n_out);
int lcs_chan_last_ms(lcs_ctx *c, float *ms);   // HIP-event time of the context's last lcs_launch_channelize
