// xcorr_route.h -- which PSS correlation kernel a call takes and which of the kernels' buffer sets it needs: the one rule the callers of
// lcs_launch_xcorr go by (lcs_api.hip: upload_host_capbuf, lcs_batch_enqueue, the streaming chain).  Plain host C++, no HIP and no
// context: tests/test_xcorr_route_host.py walks it over its whole domain.
#pragma once
#include <cstddef>
#include <cstdint>

// what a template group holds: the limit each kernel puts on pack_grid (pss_ref.h)
#define LCS_KP2_MAX 128      // fp32 kernel: tap pairs per (window, group): 137 taps + up to 119 samples of spread
#define LCS_KP2_UNROLL 4
#define LCS_I8_OFF 16        // int8 kernel: a template column's delay inside its group (window-start spread) stays below this
#define LCS_I8_MAX_TAPS (137 + LCS_I8_OFF - 1)

// k_xcorr_mfma_blk / k_xcorr_i8x3 (u8 sources) / k_xcorr_f16x3 (complex<float> batches) / k_single_exact (one combining window: every
// element in the reference's own arithmetic, no operand tables)
enum class XcKernel { fp32, i8, f16, single_exact };
// 137 taps + the window-start spread a group may have.  The fp16 kernel holds 160 taps and shares the int8 kernel's packing.
constexpr int xc_max_taps(XcKernel k) { return k == XcKernel::fp32 ? 2 * (LCS_KP2_MAX - LCS_KP2_UNROLL) : LCS_I8_MAX_TAPS; }

enum class XcCaller { host /* complex<double>: lcs_xcorr_pss, lcs_search_capbuf, lcs_foe_partial */, batch /* lcs_batch_enqueue */, stream };
enum XcSet : unsigned { XC_SET_I8 = 1, XC_SET_F16 = 2, XC_SET_BTAB = 4 };      // the int8 set, the fp16 set, the fp32 kernel's tables
enum class XcVerdict { unknown, dongle, other };      // k_ingest_c128 on a host buffer: every component is (u8 - 127) / 128, or not
struct XcFacts {
  XcCaller caller;
  bool u8;                   // the source is u8 I/Q -- for a batch AFTER the float probe, which turns dongle data into u8
  bool st_open;              // a stream is open: its captured graph holds the workspace's addresses, no set may be allocated
  bool i8_ready, f16_ready;  // the set exists for the current workspace
  int n_comb;                // combining windows
  XcVerdict verdict;         // host caller: unknown until the ingest has run
  bool probe_on, probe_fits; // batch caller: lcs_set_float_batch_probe; xc_probe_fits of the batch
  bool screen_on = false;    // batch caller: lcs_set_batch_screen (the context's default is on)
};
struct XcRoute {
  unsigned sets;             // XcSet bits the caller ensures before it ingests (a stream: at open).  Holding the int8 set, the host caller
                             // ingests with a verdict; holding the fp16 set, the batch caller ingests into fp16 pairs
  bool may_probe;            // a complex<float> batch is probed for dongle data first (the caller keeps the c64_skip countdown)
  XcKernel kernel;
  int pack_taps;             // the tap limit the launch's grid is packed for
  bool screen = false;       // int8 batches of two or more windows: a two-digit pass over every tile, the three-digit kernel over the tiles
                             // whose collapsed power can reach the detection threshold (pss_xcorr_i8.hip, screen_bound.h)
};
inline bool xc_probe_fits(size_t n_samples, uintptr_t src) { return n_samples % 2 == 0 && (src & 15) == 0; }   // k_c64_probe_u8 reads float4

inline XcRoute xc_route(const XcFacts &f) {
  const bool i8_ok = f.i8_ready || !f.st_open, f16_ok = f.f16_ready || !f.st_open;      // the set is there, or may be allocated
  XcRoute r{0, false, XcKernel::fp32, xc_max_taps(XcKernel::i8)};
  if (f.caller == XcCaller::host) {
    // a buffer that is dongle data -- any capture -- takes the int8 kernel, anything else, or a context that cannot have the int8
    // copies, the fp32 one; the grid is packed for the kernel
    if (i8_ok) r.sets = XC_SET_I8;
    if (i8_ok && f.verdict == XcVerdict::dongle) r.kernel = XcKernel::i8;
    r.pack_taps = xc_max_taps(r.kernel);
  } else if (f.caller == XcCaller::batch) {
    // u8: the int8 kernel (refused by lcs_ensure_xc under an open stream without the set).  complex<float>: fp16 hi / lo operands,
    // three products -- or the fp32 kernel, which the int8 packing fits too
    if (f.u8) r.sets = XC_SET_I8, r.kernel = XcKernel::i8;
    else if (f16_ok) r.sets = XC_SET_F16, r.kernel = XcKernel::f16;
    r.may_probe = !f.u8 && f.probe_on && f.probe_fits && i8_ok;
  } else {
    // the fp32 tables exist from the open on: host buffers that are not dongle data take that kernel also while the stream is open
    r.sets = XC_SET_BTAB | (f.u8 ? XC_SET_I8 : 0);
    if (f.u8) r.kernel = XcKernel::i8;
  }
  if (f.n_comb == 1) r.kernel = XcKernel::single_exact;
  r.screen = f.caller == XcCaller::batch && r.kernel == XcKernel::i8 && f.n_comb >= 2 && f.screen_on;
  return r;
}
