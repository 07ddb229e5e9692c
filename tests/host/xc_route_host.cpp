// Host-side call of the PSS correlation's routing rule (xcorr_route.h: xc_route), the very function upload_host_capbuf,
// lcs_batch_enqueue and the streaming chain of lcs_api.hip go by.  The header is all this file includes: it needs neither HIP nor
// a context.  tests/test_xcorr_route_host.py holds the table.  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/xcorr_route.h"

static const char *const kKernelNames[] = {"fp32", "i8", "f16", "single_exact"};
static_assert((int)XcKernel::fp32 == 0 && (int)XcKernel::i8 == 1 && (int)XcKernel::f16 == 2 && (int)XcKernel::single_exact == 3, "kKernelNames");

// caller 0 host / 1 batch / 2 stream; verdict 0 unknown / 1 dongle data / 2 anything else.  out = {int8 set, fp16 set, fp32 tables,
// may_probe, pack_taps}; returns the kernel's name
extern "C" const char *xc_route_call(int caller, int u8, int st_open, int i8_ready, int f16_ready, int n_comb, int verdict, int probe_on,
                                     int probe_fits, int *out) {
  const XcCaller callers[] = {XcCaller::host, XcCaller::batch, XcCaller::stream};
  const XcVerdict verdicts[] = {XcVerdict::unknown, XcVerdict::dongle, XcVerdict::other};
  const XcRoute r = xc_route(XcFacts{callers[caller], u8 != 0, st_open != 0, i8_ready != 0, f16_ready != 0, n_comb, verdicts[verdict],
                                     probe_on != 0, probe_fits != 0});
  out[0] = (r.sets & XC_SET_I8) != 0; out[1] = (r.sets & XC_SET_F16) != 0; out[2] = (r.sets & XC_SET_BTAB) != 0;
  out[3] = r.may_probe; out[4] = r.pack_taps;
  return kKernelNames[(int)r.kernel];
}
extern "C" int xc_route_probe_fits(unsigned long long n_samples, unsigned long long src) { return xc_probe_fits((size_t)n_samples, (uintptr_t)src); }
// out = {tap limit of fp32, i8, f16, single_exact; LCS_I8_OFF, LCS_KP2_MAX, LCS_KP2_UNROLL}
extern "C" void xc_route_limits(int *out) {
  for (int k = 0; k < 4; ++k) out[k] = xc_max_taps((XcKernel)k);
  out[4] = LCS_I8_OFF; out[5] = LCS_KP2_MAX; out[6] = LCS_KP2_UNROLL;
}
