// lcs_api.hip -- C ABI (include/lcs.h) over the HIP kernels.  Host-side glue only: workspace
// management, H2D/D2H staging for the host-buffer entry points, launch sequencing.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <chrono>

#include "lcs_internal.h"
#include "channelizer.h"
#include "lte_device.h"
#include "tdd_config.h"
#include "cell_meas.h"
#include "cell_meas_wide.h"
#include "pcfich.h"
#include "pdcch.h"
#include "pdcch_scan.h"
#include "phich.h"
#include "wide_call.h"
#include "pdsch.h"
#include "tfg_layout.h"
#include "pss_ref.h"

namespace {

// Grow the workspace so that n_slots buffers of n_cap samples with n_f hypotheses fit.
int ensure_ws(lcs_ctx *c, int n_slots, uint32_t n_cap, int n_f, bool debug, int G_need = 0) {
  if (G_need <= 0) G_need = (3 * n_f + LCS_TG - 1) / LCS_TG;           // dense packing
  if (n_slots <= c->cap_slots && n_cap <= c->cap_n_cap && n_f <= c->cap_n_f && G_need <= c->cap_G && (!debug || c->cap_debug)) return LCS_OK;
  if (c->st_open) {     // the captured graph of the streaming mode holds the current buffers' addresses
    c->err = "this call needs a larger workspace than the open stream was captured with: lcs_stream_close first";
    return LCS_ERR_BAD_ARG;
  }
  n_slots = std::max(n_slots, c->cap_slots);
  n_cap = std::max(n_cap, c->cap_n_cap);
  n_f = std::max(n_f, c->cap_n_f);
  debug = debug || c->cap_debug;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t S = n_slots, NE = 3 * LCS_N_IDX;
  const int G = std::max(std::max(G_need, c->cap_G), (3 * n_f + LCS_TG - 1) / LCS_TG);
  int rc;
  c->xcb = XcBufs();        // the correlation kernels' sets were sized for the old workspace: gone, allocated again on first use (lcs_ensure_xc)
  // the per-hypothesis / per-group tables (fset .. kp2, single, sref) are sized for the largest grid seen; every call lays its
  // own grid out with its own strides n_f and G (k_prep_tables rebuilds them per call)
  if ((rc = c->cap32.alloc(c, S * n_cap)) || (rc = c->cap64.alloc(c, (size_t)n_cap)) || (rc = c->params_ws.alloc(c, S)) ||
      (rc = c->fset_ws.alloc(c, (size_t)n_f)) || (rc = c->tmpl.alloc(c, S * n_f * 3 * 137)) || (rc = c->start.alloc(c, S * LCS_NW_MAX * n_f)) ||
      (rc = c->smin.alloc(c, S * LCS_NW_MAX * G)) || (rc = c->kp2.alloc(c, S * LCS_NW_MAX * G)) ||
      (rc = c->single.alloc(c, S * G * LCS_N_IDX * LCS_TG)) || (rc = c->sref.alloc(c, NE * n_f)) || (rc = c->sp.alloc(c, S * LCS_NW_MAX * LCS_N_IDX)) ||
      (rc = c->pow_.alloc(c, S * NE)) || (rc = c->work.alloc(c, S * NE)) || (rc = c->frq.alloc(c, S * NE)) || (rc = c->fix_list.alloc(c, S * NE)) ||
      (rc = c->n_fix.alloc(c, 4)) || (rc = c->second32.alloc(c, S * NE)) || (rc = c->spinc.alloc(c, S * LCS_N_IDX)) ||
      (rc = c->zth.alloc(c, S * LCS_N_IDX)) || (rc = c->peaks.alloc(c, S * LCS_MAXP)) || (rc = c->npeaks.alloc(c, S)) ||
      (debug && (rc = c->incoh.alloc(c, S * NE * n_f))))
    return rc;
  c->foe_ready = false;      // (a pending lcs_foe_partial result lived in the buffers just replaced)
  c->batch = BatchRecord();  // ... and so did the last batch: its record points into them (lcs_batch_collect / _readback then refuse)
  c->screen_pending = false;
  c->cap_slots = n_slots;
  c->cap_n_cap = n_cap;
  c->cap_n_f = n_f;
  c->cap_G = G;
  c->cap_debug = debug;
  return LCS_OK;
}

// Buffers of the per-cell stages, allocated on first use for c->max_work cells (~6 MB each: 3 GB at the default 512) and
// again when the limit was raised since (lcs_set_max_cells_in_flight, or by itself after a batch that carried more cells).
int alloc_percell(lcs_ctx *c, size_t W) {
  int rc;
  const size_t GRID = (size_t)LCS_TFG_ROWS * LCS_TFG_NSC;
  c->percell_ready = false;      // until every buffer exists: a failure part-way leaves a context that allocates again, not one
  c->percell_cap = 0;            // that runs kernels on a null pointer
  if ((rc = c->work_items.alloc(c, W)) || (rc = c->n_work.alloc(c, 4)) || (rc = c->tfg.alloc(c, W * GRID)) || (rc = c->tfg_comp.alloc(c, W * GRID)) ||
      (rc = c->ce.alloc(c, W * 4 * GRID)) || (rc = c->tfg_desc.alloc(c, W * (size_t)LCS_TFG_DESC_BYTES)) || (rc = c->tfg_ts.alloc(c, W * LCS_TFG_ROWS)) ||
      (rc = c->tfg_ts_comp.alloc(c, W * LCS_TFG_ROWS)) || (rc = c->cell_scratch.alloc(c, W * LCS_CELL_SCRATCH)) || (rc = c->cells_out.alloc(c, W)) ||
      (rc = c->d_dbg.alloc(c, 2048)))
    return rc;
  c->percell_ready = true;
  c->percell_cap = (int)W;
  return LCS_OK;
}
int ensure_percell(lcs_ctx *c) {
  if (c->percell_ready && c->max_work <= c->percell_cap) return LCS_OK;
  if (c->st_open && c->percell_ready) return LCS_OK;      // the open stream's graph holds these addresses: keep what it was captured with
  const int prev = c->percell_ready ? c->percell_cap : 0;
  if (c->percell_ready) HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t W = (size_t)std::max(c->max_work, prev);
  int rc = alloc_percell(c, W);
  if (rc != LCS_OK && prev > 0 && W > (size_t)prev) {
    // growing failed (6 MB per cell: 512 -> 1024 cells asks for 3 GB more): back to the capacity that worked, and the limit stays
    // there -- more rounds per batch instead of a failed batch
    (void)hipGetLastError();
    c->max_work = prev;
    c->max_work_pinned = true;
    rc = alloc_percell(c, (size_t)prev);
  }
  return rc;
}

// Device block the results of a batch are compacted into (k_pack_results) and its page-locked mirror, sized for the worst case
// of n_buf buffers (every buffer LCS_MAXP records): allocated when a larger batch arrives, never inside lcs_batch_collect.
int ensure_res_pack(lcs_ctx *c, int n_buf) {
  const size_t need = lcs_pack_rec_offset(n_buf) + (size_t)n_buf * LCS_MAXP * sizeof(lcs_cell);
  if (need <= c->res_pack.capacity() && need <= c->h_res.capacity()) return LCS_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (the streaming mode's graph does not reference this block: it may grow under an open stream)
  c->res_pack.reset();      // both go before either comes back, as ever
  c->h_res.reset();
  int rc;
  if ((rc = c->res_pack.alloc(c, need)) || (rc = c->h_res.alloc(c, need))) return rc;
  return LCS_OK;
}

const double kPeakThresh = std::pow(10.0, -12.0 / 10.0);                  // peak_search: udb10(-12.0), what lies below this fraction of a found peak is cleared (ref src/searcher.cpp:501)

// lcs_set_float_batch_probe: is a batch of complex<float> buffers dongle data -- every component exactly (u8 - 127) / 128 (ref
// src/capbuf.cpp:172-181)?  One pass: per component dongle_component_f32 (lte_device.h) decides on the exact product x * 128 and
// names the byte it came from; a component that does not compare equal to one of the 256 values -- one ulp beside one, tiny, NaN,
// infinite -- clears the flag.  The bytes are then handed to the u8 route unchanged (int8 copies, int8 correlation kernel, the
// fp64 stages on the int8 pairs): the same numbers, the faster kernel.
__global__ __launch_bounds__(256) void k_c64_probe_u8(const float *__restrict__ src, size_t n_comp, uint8_t *__restrict__ dst, int *__restrict__ flag) {
  bool ok = true;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n_comp; i += (size_t)gridDim.x * blockDim.x * 4) {
    const float4 x = *reinterpret_cast<const float4 *>(src + i);      // (n_comp = 2 n_cap n_buf is a multiple of 4 for the batch shapes the library takes: checked by the caller)
    const float v[4] = {x.x, x.y, x.z, x.w};
    uchar4 b;
    unsigned char *pb = reinterpret_cast<unsigned char *>(&b);
#pragma unroll
    for (int q = 0; q < 4; ++q) ok = dongle_component_f32(v[q], pb + q) && ok;
    *reinterpret_cast<uchar4 *>(dst + i) = b;
  }
  if (__any(!ok) && (threadIdx.x & 63) == 0) atomicAnd(flag, 0);
}
// The probe of one batch: one pass + one small read-back -- the host waits for it, while the other contexts' kernels keep the GPU busy,
// before it knows which kernels to queue.  c->last_c64_routed: the batch is dongle data and takes the u8 route with the bytes in c->c64_u8.
int probe_c64_batch(lcs_ctx *c, bool may_probe, const void *d_capbufs, size_t n_comp) {
  c->last_c64_routed = false;
  if (!may_probe) return LCS_OK;
  if (c->c64_skip > 0) { --c->c64_skip; return LCS_OK; }
  if (n_comp > c->c64_u8.capacity()) HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = c->c64_u8.reserve(c, n_comp);
  if (rc) return rc;
  int flag = 1;
  HIPCHK(c, hipMemcpyAsync(c->d_flag, &flag, sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_c64_probe_u8, dim3(2048), dim3(256), 0, c->stream, (const float *)d_capbufs, n_comp, c->c64_u8, c->d_flag);
  HIPCHK(c, hipMemcpyAsync(&flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (flag) c->last_c64_routed = true;
  else c->c64_skip = 15;      // a float front end: the next batches are not probed (one in sixteen is)
  return LCS_OK;
}

// The one place a Launch is built: n_buf buffers of n_cap samples that the fp64 stages read from `src`, parameters and hypotheses in
// the workspace's arrays, 64 workgroups per work-list axis.  The entry point then sets what differs for its call.  Two things a
// context with an OPEN STREAM hands to every launch made on it, not only to the stream's own chain: everything runs on one
// stream, and k_gather_work leaves out the identities on the stream's tracked list.
Launch make_launch(const lcs_ctx *c, int n_buf, uint32_t n_cap, const CapSrc &src) {
  Launch L;
  L.n_buf = n_buf;
  L.n_cap = n_cap;
  L.src = src;
  L.params = c->params_ws;
  L.fset = c->fset_ws;
  L.round_cells = std::min(c->max_work, c->percell_cap);
  L.single_stream = c->st_open;
  L.duplex = c->duplex;
  L.foe_unwrap = c->foe_unwrap;
  L.tdd_config = (c->tdd_config && c->duplex == LCS_DUPLEX_TDD) ? 1 : 0;
  L.cell_meas = c->cell_meas;
  if (c->st_open) { L.tracked = c->st_dtracked; L.n_tracked = c->st_dntracked; }
  return L;
}

// What xc_route (xcorr_route.h) asks about a context; the caller adds what it knows of its call.
XcFacts route_facts(const lcs_ctx *c, XcCaller caller, bool u8, int n_comb) {
  return XcFacts{caller, u8, c->st_open, c->xcb.i8.ready, c->xcb.f16.ready, n_comb, XcVerdict::unknown, c->c64_probe, false};
}

// complex<double> host buffer -> device (cap64, slot 0) and xc_route's choice of the correlation kernel, once the ingest has
// said whether the buffer is dongle data.  *out: the launch to correlate with (geometry, kernel, source).
int upload_host_capbuf(lcs_ctx *c, const double *capbuf, uint32_t n_cap, const double *f_search_set, int n_f, int ds, double fc_req,
                       double fc_prog, double fs_prog, bool debug, Launch *out) {
  const XcGeom geo32 = pack_grid(n_cap, n_f, ds, f_search_set, &fc_req, &fc_prog, 1, fs_prog, xc_max_taps(XcKernel::fp32));
  const XcGeom geo8 = pack_grid(n_cap, n_f, ds, f_search_set, &fc_req, &fc_prog, 1, fs_prog, xc_max_taps(XcKernel::i8));
  int rc;
  c->foe_ready = false;      // slot 0 is overwritten: a pending lcs_foe_partial result is gone (lcs_foe_partial sets it again)
  if ((rc = ensure_ws(c, 1, n_cap, n_f, debug, std::max(geo32.G, geo8.G)))) return rc;
  XcFacts facts = route_facts(c, XcCaller::host, false, geo8.n_comb);
  const unsigned sets = xc_route(facts).sets;
  if ((rc = lcs_ensure_xc(c, sets))) return rc;
  c->h_params = SlotParams{fc_req, fc_prog, fs_prog};
  HIPCHK(c, hipMemcpyAsync(c->cap64, capbuf, sizeof(double2) * n_cap, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->fset_ws, f_search_set, sizeof(double) * n_f, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->params_ws, &c->h_params, sizeof(SlotParams), hipMemcpyHostToDevice, c->stream));
  bool exact = false;
  CapSrc src;
  if (sets & XC_SET_I8) { if ((rc = lcs_launch_ingest_c128(c, n_cap, &exact, &src))) return rc; }
  else if ((rc = lcs_launch_ingest(c, nullptr, LCS_FMT_C128, 1, n_cap, &src))) return rc;
  facts.verdict = exact ? XcVerdict::dongle : XcVerdict::other;
  const XcRoute r = xc_route(facts);
  *out = make_launch(c, 1, n_cap, src);
  out->geo = r.pack_taps == xc_max_taps(XcKernel::i8) ? geo8 : geo32;
  out->xc = r.kernel;
  return LCS_OK;
}

// The workspace of the stage entry points that take no capture buffer (a fresh context: the kernels read the slot's parameter record).
int ensure_stage_ws(lcs_ctx *c, int n_f = 1) { return ensure_ws(c, 1, std::max<uint32_t>(c->cap_n_cap, 153600), n_f, false); }

// The per-peak chain of a launch: sss_detect + pss_sss_foe on every peak (with the first round), then per round of L.round_cells
// cells the work list, the grids, the frequency / timing correction and the MIB.  Rounds [r0, r1).
// With L.tdd_config (lcs_set_tdd_config in LCS_DUPLEX_TDD) every round also estimates the uplink-downlink configuration of its cells
// (k_tdd_config, on the raw grid) into c->tdd_info, a table beside the peak table (SideTable: the first round's call sets every
// record of it to LCS_TDD_NOT_ESTIMATED, all 32-bit words -2: lcs_last_tdd_info reads the integer fields only of such a record).
// With L.cell_meas (lcs_set_cell_meas) every round measures its cells as well (k_cell_meas, behind k_tdd_config, whose record of the
// cell names the subframes to measure where there is one) into c->cell_meas_tab, a table made and kept in the same way.
int launch_per_peak(lcs_ctx *c, const Launch &L, int r0, int r1) {
  int rc;
  if (r0 == 0) {
    c->fused_n_buf = L.n_buf;
    if ((rc = c->tdd_info.begin(c, L.n_buf, L.tdd_config != 0)) || (rc = c->cell_meas_tab.begin(c, L.n_buf, L.cell_meas != 0))) return rc;
  }
  const int meas_mask = L.duplex == LCS_DUPLEX_TDD ? 0x021 : 0x3ff;      // TDD: subframes 0 and 5 are downlink in every configuration
  if (r0 == 0 && (rc = lcs_launch_sss_foe(c, L, 3.0 /* THRESH2_N_SIGMA, ref src/CellSearch.cpp:528 */, nullptr))) return rc;
  for (int r = r0; r < r1; ++r)
    if ((rc = lcs_launch_gather_work(c, L, r * L.round_cells)) || (rc = lcs_launch_tfg(c, L, true)) || (rc = lcs_launch_tfoec(c, L, false)) ||
        (rc = lcs_launch_mib(c, L, true)) || (L.tdd_config && (rc = lcs_launch_tdd_config(c, L, c->tdd_info.get(), false))) ||
        (L.cell_meas && (rc = lcs_launch_cell_meas(c, L, L.tdd_config ? c->tdd_info.get() : nullptr, c->cell_meas_tab.get(), meas_mask, false))))
      return rc;
  return LCS_OK;
}

// The peak table of slot 0, read back (one synchronisation): *np entries, of which tmp holds the first LCS_MAXP.
int read_peak_table(lcs_ctx *c, std::vector<lcs_cell> &tmp, int *np) {
  tmp.resize(LCS_MAXP);
  HIPCHK(c, hipMemcpyAsync(tmp.data(), c->peaks, sizeof(lcs_cell) * LCS_MAXP, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(np, c->npeaks, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

// ... and handed out after the fused chain: `peaks` gets the peak_search view of every record (PSS fields only), `cells` the
// decoded ones.  With `order` (lcs_foe_finish) a peak won by another rank's hypothesis -- the fused peak search marks it in
// `reserved` -- has no `ind` here and is nobody's cell on this rank; order[k] is the peak index of cells[k].
int read_cells_and_peaks(lcs_ctx *c, lcs_cell *cells, int32_t *order, int max_cells, int *n_cells, lcs_cell *peaks, int max_peaks, int *n_peaks) {
  std::vector<lcs_cell> tmp;
  int np = 0, rc;
  if ((rc = read_peak_table(c, tmp, &np))) return rc;
  if (np > LCS_MAXP) { np = LCS_MAXP; rc = LCS_ERR_OVERFLOW; }
  int n = 0;
  for (int i = 0; i < np; ++i) {
    const bool mine = !order || tmp[i].reserved == 0;
    if (peaks && i < max_peaks) {
      lcs_cell pk;
      lcs_cell_init(&pk);
      pk.fc_requested = tmp[i].fc_requested; pk.fc_programmed = tmp[i].fc_programmed; pk.pss_pow = tmp[i].pss_pow;
      pk.ind = mine ? tmp[i].ind : -1; pk.freq = tmp[i].freq; pk.n_id_2 = tmp[i].n_id_2;
      if (order) pk.reserved = tmp[i].reserved;
      peaks[i] = pk;
    }
    if (!mine || tmp[i].n_id_1 == -1 || tmp[i].n_rb_dl == -1) continue;
    if (n < max_cells) { cells[n] = tmp[i]; if (order) order[n] = i; } else rc = LCS_ERR_OVERFLOW;
    ++n;
  }
  if (n_peaks) *n_peaks = np;
  *n_cells = n;
  if (rc) c->err = "more results than the output arrays hold";
  return rc;
}

// A mode of a context that is 0 or 1 and that an open stream holds (lcs_set_foe_unwrap, lcs_set_tdd_config, lcs_set_cell_meas);
// `held`: the refusal of a change under an open stream
int set_mode(lcs_ctx *c, int lcs_ctx::*mode, int on, const char *name, const char *held) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (on != 0 && on != 1) { c->err = std::string(name) + " is neither 0 nor 1"; return LCS_ERR_BAD_ARG; }
  if (c->st_open && on != c->*mode) { c->err = held; return LCS_ERR_BAD_ARG; }
  c->*mode = on;
  return LCS_OK;
}
int get_mode(const lcs_ctx *c, int lcs_ctx::*mode, int *on) {
  if (!c || !on) return LCS_ERR_BAD_ARG;
  *on = c->*mode;
  return LCS_OK;
}

int check_common(lcs_ctx *c, uint32_t n_cap, int n_f) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (n_f < 1 || n_f > LCS_NF_LIMIT) { c->err = "n_f out of range (1..1024)"; return LCS_ERR_BAD_ARG; }
  if (n_cap < 136 + 137 + 9600 + 100) { c->err = "capture buffer shorter than one 5 ms window"; return LCS_ERR_BAD_ARG; }
  if ((n_cap - 136 - 100) / 9600 > LCS_NW_MAX) { c->err = "capture buffer longer than 16 combining windows"; return LCS_ERR_BAD_ARG; }
  return LCS_OK;
}

}  // namespace

extern "C" {

const char *lcs_version(void) { return "lcs_amd 0.1 (gfx950)"; }

void lcs_cell_init(lcs_cell *c) {
  c->fc_requested = NAN; c->fc_programmed = NAN; c->pss_pow = NAN; c->freq = NAN; c->frame_start = NAN;
  c->freq_fine = NAN; c->freq_superfine = NAN; c->ind = -1; c->n_id_2 = -1; c->n_id_1 = -1;
  c->cp_type = LCS_CP_UNKNOWN; c->n_ports = -1; c->n_rb_dl = -1; c->phich_duration = 0; c->phich_resource = 0;
  c->sfn = -1; c->reserved = 0;
}

int lcs_create(int device, lcs_ctx **out) {
  if (!out) return LCS_ERR_BAD_ARG;
  *out = nullptr;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return LCS_ERR_NO_DEVICE;
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return LCS_ERR_NO_DEVICE; }
  if (device >= n_dev) return LCS_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return LCS_ERR_NO_DEVICE;
  lcs_ctx *c = new lcs_ctx();
  c->device = device;
  // Two streams per context: the correlation kernel goes to a LOW-priority stream, everything
  // else (small, latency-bound kernels) to a HIGH-priority one, so that when two contexts are
  // used round-robin the tail of batch i is not starved by the correlation of batch i+1.
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  bool ok_streams = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_greatest) == hipSuccess;
  ok_streams = ok_streams && hipStreamCreateWithPriority(&c->stream_xc, hipStreamNonBlocking, prio_least) == hipSuccess;
  if (!ok_streams) { lcs_destroy(c); return LCS_ERR_HIP; }
  // events between streams of ONE device (and the two that time the correlation): no system-scope fence -- its cache
  // write-back and invalidation at every record is paid by the kernels that follow (results reach the host through
  // hipMemcpyAsync / stream synchronisation, which fence on their own)
  (void)hipEventCreateWithFlags(&c->ev_xc0, LCS_EVENT_NOFENCE);
  (void)hipEventCreateWithFlags(&c->ev_xc1, LCS_EVENT_NOFENCE);
  (void)hipEventCreateWithFlags(&c->ev_pre, hipEventDisableTiming | LCS_EVENT_NOFENCE);
  (void)hipEventCreateWithFlags(&c->ev_post, hipEventDisableTiming | LCS_EVENT_NOFENCE);
  // constant tables
  std::vector<double> td(3 * 137 * 2), fd(3 * 62 * 2);
  for (int t = 0; t < 3; ++t) { lcs_tables::pss_td(t, &td[t * 137 * 2]); lcs_tables::pss_fd(t, &fd[t * 62 * 2]); }
  std::vector<int8_t> sss(168 * 3 * 2 * 62);
  for (int n1 = 0; n1 < 168; ++n1)
    for (int n2 = 0; n2 < 3; ++n2)
      for (int s = 0; s < 2; ++s) {
        int32_t tmp[62];
        lcs_tables::sss_fd(n1, n2, s * 10, tmp);
        for (int i = 0; i < 62; ++i) sss[((n1 * 3 + n2) * 2 + s) * 62 + i] = (int8_t)tmp[i];
      }
  std::vector<uint8_t> scr(504 * 1920);
  for (int id = 0; id < 504; ++id) lcs_tables::lte_pn((uint32_t)id, 1920, &scr[(size_t)id * 1920]);
  std::vector<int16_t> derm(2 * 120 * 16, (int16_t)-1);
  for (int v = 0; v < 2; ++v)                              // 0: normal CP (1920 bits), 1: extended CP (1728)
    if (!lcs_tables::pbch_derm_inv(v ? 1728 : 1920, &derm[(size_t)v * 120 * 16])) { lcs_destroy(c); return LCS_ERR_HIP; }
  uint32_t pn_jump[32];
  lcs_tables::pn_jump_table(1600 + 2 * (110 - 6), pn_jump);
  bool ok = c->d_pss_td.alloc(c, td.size() / 2) == LCS_OK &&
            c->d_flag.alloc(c, 1) == LCS_OK &&
            c->d_pn_jump.alloc(c, 32) == LCS_OK &&
            hipMemcpy(c->d_pn_jump, pn_jump, sizeof(pn_jump), hipMemcpyHostToDevice) == hipSuccess &&
            c->d_pss_fd.alloc(c, fd.size() / 2) == LCS_OK &&
            c->d_sss_fd.alloc(c, sss.size()) == LCS_OK &&
            c->d_pbch_scr.alloc(c, scr.size()) == LCS_OK &&
            c->d_derm_inv.alloc(c, derm.size()) == LCS_OK &&
            hipMemcpy(c->d_derm_inv, derm.data(), derm.size() * sizeof(int16_t), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(c->d_pss_td, td.data(), td.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(c->d_pss_fd, fd.data(), fd.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(c->d_sss_fd, sss.data(), sss.size(), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(c->d_pbch_scr, scr.data(), scr.size(), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { lcs_destroy(c); return LCS_ERR_HIP; }
  *out = c;
  return LCS_OK;
}

// The order of a context's end (lcs_internal.h, at lcs_ctx): this body, then the members -- the owners free their memory --, then
// the base with the events and the streams.
lcs_ctx::~lcs_ctx() {
  (void)hipSetDevice(device);
  if (st_open) (void)lcs_stream_close(this);      // graphs first
  if (stream) (void)hipStreamSynchronize(stream);
  if (stream_xc) (void)hipStreamSynchronize(stream_xc);
}

lcs_ctx_queues::~lcs_ctx_queues() {
  for (hipEvent_t e : {ev_stage[0], ev_stage[1], ev_chan_slot[0], ev_chan_slot[1], ev_chan0, ev_chan1, ev_xc0, ev_xc1, ev_pre, ev_post})
    if (e) (void)hipEventDestroy(e);
  if (stream) (void)hipStreamDestroy(stream);
  if (stream_xc) (void)hipStreamDestroy(stream_xc);
}

void lcs_destroy(lcs_ctx *c) { delete c; }

const char *lcs_last_error(const lcs_ctx *c) { return c ? c->err.c_str() : "null context"; }

int lcs_set_float_batch_probe(lcs_ctx *c, int on) {
  if (!c) return LCS_ERR_BAD_ARG;
  c->c64_probe = on != 0;
  c->c64_skip = 0;
  return LCS_OK;
}

int lcs_set_batch_screen(lcs_ctx *c, int on) {
  if (!c) return LCS_ERR_BAD_ARG;
  c->batch_screen = on != 0;
  c->screen_skip = 0;
  return LCS_OK;
}
int lcs_get_batch_screen(const lcs_ctx *c, int *on) {
  if (!c || !on) return LCS_ERR_BAD_ARG;
  *on = c->batch_screen ? 1 : 0;
  return LCS_OK;
}
// From the header the last lcs_batch_collect brought over (k_pack_results copies the screen's counters into it)
int lcs_last_screen_stats(lcs_ctx *c, int stats[4]) {
  if (!c || !stats || !c->h_res || c->batch.l.n_buf <= 0) return LCS_ERR_BAD_ARG;
  const int *hdr = reinterpret_cast<const int *>(c->h_res.get());
  const Launch &L = c->batch.l;
  stats[0] = L.screen ? hdr[2] : 0;
  stats[1] = L.screen ? L.n_buf * LCS_I8_TILES : 0;
  stats[2] = L.screen ? hdr[2] * L.geo.G : 0;
  stats[3] = L.screen ? hdr[3] >> 16 : 0;
  return LCS_OK;
}

int lcs_set_duplex(lcs_ctx *c, int duplex) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (duplex != LCS_DUPLEX_FDD && duplex != LCS_DUPLEX_TDD) { c->err = "duplex is neither LCS_DUPLEX_FDD nor LCS_DUPLEX_TDD"; return LCS_ERR_BAD_ARG; }
  if (c->st_open && duplex != c->duplex) {
    c->err = "the open stream's captured graph holds the duplex mode it was opened with: lcs_stream_close first";
    return LCS_ERR_BAD_ARG;
  }
  c->duplex = duplex;
  return LCS_OK;
}
int lcs_get_duplex(const lcs_ctx *c, int *duplex) { return get_mode(c, &lcs_ctx::duplex, duplex); }

int lcs_set_foe_unwrap(lcs_ctx *c, int on) {
  return set_mode(c, &lcs_ctx::foe_unwrap, on, "foe_unwrap",
                  "the open stream's captured graph holds the foe_unwrap mode it was opened with: lcs_stream_close first");
}
int lcs_get_foe_unwrap(const lcs_ctx *c, int *on) { return get_mode(c, &lcs_ctx::foe_unwrap, on); }

int lcs_set_tdd_config(lcs_ctx *c, int on) {
  return set_mode(c, &lcs_ctx::tdd_config, on, "tdd_config",
                  "the streaming mode does not carry the uplink-downlink estimate: the tdd_config mode cannot change under an open stream, lcs_stream_close first");
}
int lcs_get_tdd_config(const lcs_ctx *c, int *on) { return get_mode(c, &lcs_ctx::tdd_config, on); }

int lcs_set_cell_meas(lcs_ctx *c, int on) {
  return set_mode(c, &lcs_ctx::cell_meas, on, "cell_meas",
                  "the streaming mode does not carry the cell measurement: the cell_meas mode cannot change under an open stream, lcs_stream_close first");
}
int lcs_get_cell_meas(const lcs_ctx *c, int *on) { return get_mode(c, &lcs_ctx::cell_meas, on); }
int lcs_tdd_dl_mask(int ul_dl_config) { return meas_tdd_dl_mask(ul_dl_config); }

// The side tables of the last fused call (SideTable::read_last): k_tdd_config's estimates and k_cell_meas's measurements
int lcs_last_tdd_info(lcs_ctx *c, lcs_tdd_info *info, int max_cells_per_buf) {
  if (!c || max_cells_per_buf < 0 || (!info && max_cells_per_buf > 0)) return LCS_ERR_BAD_ARG;
  if (c->fused_n_buf <= 0) { c->err = "lcs_last_tdd_info needs lcs_search_capbuf or a batch on this context first"; return LCS_ERR_BAD_ARG; }
  lcs_tdd_info none;
  tdd_info_clear(&none, LCS_TDD_NOT_ESTIMATED);
  return c->tdd_info.read_last(c, c->fused_n_buf, none, &lcs_tdd_info::ul_dl_config, info, max_cells_per_buf);
}
int lcs_last_cell_meas(lcs_ctx *c, lcs_meas_info *info, int max_cells_per_buf) {
  if (!c || max_cells_per_buf < 0 || (!info && max_cells_per_buf > 0)) return LCS_ERR_BAD_ARG;
  if (c->fused_n_buf <= 0) { c->err = "lcs_last_cell_meas needs lcs_search_capbuf or a batch on this context first"; return LCS_ERR_BAD_ARG; }
  lcs_meas_info none;
  meas_clear(&none, LCS_MEAS_NOT_MEASURED);
  return c->cell_meas_tab.read_last(c, c->fused_n_buf, none, &lcs_meas_info::status, info, max_cells_per_buf);
}

int lcs_set_max_cells_in_flight(lcs_ctx *c, int n) {
  if (!c || n < 1) return LCS_ERR_BAD_ARG;
  c->max_work = std::min(n, (int)LCS_MAX_WORK);
  c->max_work_pinned = true;          // the limit no longer grows by itself
  return LCS_OK;
}

void *lcs_stream(lcs_ctx *c) { return c ? (void *)c->stream : nullptr; }

int lcs_sync(lcs_ctx *c) {
  if (!c) return LCS_ERR_BAD_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

// ------------------------------------------------------------------------- xcorr_pss
int lcs_xcorr_pss(lcs_ctx *c, const double *capbuf, uint32_t n_cap, const double *f_search_set, uint16_t n_f,
                  uint8_t ds_comb_arm, double fc_req, double fc_prog, double fs_prog, double *pow_, int32_t *frq,
                  float *single, float *incoh, double *sp_incoherent, float *xc, double *sp, uint16_t *n_comb_xc,
                  uint16_t *n_comb_sp) {
  int rc = check_common(c, n_cap, n_f);
  if (rc) return rc;
  if (!capbuf || !f_search_set || !pow_ || !frq || !single || !sp_incoherent) { c->err = "null argument"; return LCS_ERR_BAD_ARG; }
  if (ds_comb_arm > 8) { c->err = "ds_comb_arm > 8 is not supported (the reference uses 2)"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  const bool debug = incoh != nullptr;
  Launch L;
  if ((rc = upload_host_capbuf(c, capbuf, n_cap, f_search_set, n_f, ds_comb_arm, fc_req, fc_prog, fs_prog, debug, &L))) return rc;
  if ((rc = lcs_launch_xcorr(c, L, incoh != nullptr, false))) return rc;
  if ((rc = lcs_launch_single_layout(c, L, 0, c->sref, 1))) return rc;
  const size_t NE = 3 * LCS_N_IDX;
  HIPCHK(c, hipMemcpyAsync(pow_, c->pow_, sizeof(double) * NE, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(frq, c->frq, sizeof(int) * NE, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(single, c->sref, sizeof(float) * NE * n_f, hipMemcpyDeviceToHost, c->stream));
  if (incoh) HIPCHK(c, hipMemcpyAsync(incoh, c->incoh, sizeof(float) * NE * n_f, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(sp_incoherent, c->spinc, sizeof(double) * LCS_N_IDX, hipMemcpyDeviceToHost, c->stream));
  const int ncsp = (int)((n_cap - 136 - 137) / 9600);
  if (sp) HIPCHK(c, hipMemcpyAsync(sp, c->sp, sizeof(double) * ncsp * LCS_N_IDX, hipMemcpyDeviceToHost, c->stream));
  if (xc) {
    const size_t n = 3 * (size_t)(n_cap - 136) * n_f;
    if ((rc = c->xc.reserve(c, n))) return rc;
    if ((rc = lcs_launch_xc_debug(c, L))) return rc;
    HIPCHK(c, hipMemcpyAsync(xc, c->xc, sizeof(float2) * n, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_comb_xc) *n_comb_xc = (uint16_t)L.geo.n_comb;
  if (n_comb_sp) *n_comb_sp = (uint16_t)ncsp;
  return LCS_OK;
}

// ------------------------------------------------------------------------ peak_search
int lcs_peak_search(lcs_ctx *c, const double *pow_, const int32_t *frq, const double *Z_th1, const double *f_search_set,
                    uint16_t n_f, double fc_req, double fc_prog, const float *single, uint8_t ds_comb_arm,
                    lcs_cell *cells, int max_cells, int *n_cells) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (n_f < 1 || n_f > LCS_NF_LIMIT) { c->err = "n_f out of range (1..1024)"; return LCS_ERR_BAD_ARG; }
  if (!pow_ || !frq || !Z_th1 || !f_search_set || !single || !n_cells || (max_cells > 0 && !cells)) { c->err = "null argument"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_stage_ws(c, n_f))) return rc;
  const size_t NE = 3 * LCS_N_IDX;
  SlotParams p{fc_req, fc_prog, 0.0};
  HIPCHK(c, hipMemcpyAsync(c->pow_, pow_, sizeof(double) * NE, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->frq, frq, sizeof(int) * NE, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->zth, Z_th1, sizeof(double) * LCS_N_IDX, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->fset_ws, f_search_set, sizeof(double) * n_f, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->sref, single, sizeof(float) * NE * n_f, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->params_ws, &p, sizeof(p), hipMemcpyHostToDevice, c->stream));
  Launch L = make_launch(c, 1, 153600, CapSrc{});
  L.geo = make_geo(153600, n_f, ds_comb_arm);
  if ((rc = lcs_launch_single_layout(c, L, 0, c->sref, 0))) return rc;
  if ((rc = lcs_launch_peak_search(c, L, kPeakThresh, false))) return rc;
  std::vector<lcs_cell> tmp;
  int n = 0;
  if ((rc = read_peak_table(c, tmp, &n))) return rc;
  *n_cells = n;
  const int lim = std::min(std::min(n, max_cells), (int)LCS_MAXP);
  for (int i = 0; i < lim; ++i) cells[i] = tmp[i];
  if (n > lim) { c->err = "more peaks than the output array (or LCS_MAXP) holds"; return LCS_ERR_OVERFLOW; }
  return LCS_OK;
}

// ------------------------------------------------------------------- batched chain
int lcs_batch_enqueue(lcs_ctx *c, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap, const double *f_search_set,
                      uint16_t n_f, const double *fc_requested, const double *fc_programmed, double fs_programmed,
                      int stage_mask) {
  int rc = check_common(c, n_cap, n_f);
  if (rc) return rc;
  if (!d_capbufs || !f_search_set || !fc_requested || !fc_programmed || n_buf < 1) { c->err = "bad argument"; return LCS_ERR_BAD_ARG; }
  if (fmt != LCS_FMT_C64 && fmt != LCS_FMT_IQ_U8) { c->err = "unknown capture format"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  c->foe_ready = false;      // the batch overwrites the buffers a pending lcs_foe_partial left for lcs_foe_finish
  c->fused_n_buf = n_buf;      // lcs_last_tdd_info, lcs_last_cell_meas: this batch's tables (launch_per_peak makes them, if the batch gets that far and the mode is on)
  (void)c->tdd_info.begin(c, n_buf, false);
  (void)c->cell_meas_tab.begin(c, n_buf, false);
  // pack: 137 taps + window-start spread <= 152 inside every template group, the int8 kernel's limit, whatever kernel follows (the
  // fp16 kernel holds 160 taps, the fp32 kernel more); pack_grid thins the groups of a grid that is too sparse for that
  const XcGeom geo = pack_grid(n_cap, n_f, 2 /* DS_COMB_ARM, ref src/CellSearch.cpp:484 */, f_search_set, fc_requested, fc_programmed,
                               n_buf, fs_programmed, xc_max_taps(XcKernel::i8));
  if ((rc = ensure_ws(c, n_buf, n_cap, n_f, false, geo.G))) return rc;
  if ((rc = ensure_res_pack(c, n_buf))) return rc;
  if ((rc = c->h_pinned.reserve(c, sizeof(SlotParams) * n_buf + sizeof(double) * n_f))) return rc;
  SlotParams *hp = reinterpret_cast<SlotParams *>(c->h_pinned.get());
  double *hf = (double *)(hp + n_buf);
  for (int i = 0; i < n_buf; ++i) hp[i] = SlotParams{fc_requested[i], fc_programmed[i], fs_programmed};
  std::memcpy(hf, f_search_set, sizeof(double) * n_f);
  HIPCHK(c, hipMemcpyAsync(c->params_ws, hp, sizeof(SlotParams) * n_buf, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->fset_ws, hf, sizeof(double) * n_f, hipMemcpyHostToDevice, c->stream));
  // route: a complex<float> batch that the probe finds to be dongle data becomes the u8 batch it came from
  XcFacts facts = route_facts(c, XcCaller::batch, fmt == LCS_FMT_IQ_U8, geo.n_comb);
  facts.probe_fits = xc_probe_fits((size_t)n_buf * n_cap, reinterpret_cast<uintptr_t>(d_capbufs));
  if ((rc = probe_c64_batch(c, xc_route(facts).may_probe, d_capbufs, (size_t)2 * n_cap * n_buf))) return rc;
  const int fmt_in = fmt;      // what the caller handed over: the hint bookkeeping goes by it
  if (c->last_c64_routed) { d_capbufs = c->c64_u8; fmt = LCS_FMT_IQ_U8; facts.u8 = true; }
  // the screen pays while few tiles are flagged: after a batch that flagged many (lcs_batch_collect) the next LCS_SCREEN_SKIP batches that
  // would be screened run the three-digit kernel alone -- the records are the same either way, so a wrong guess costs time only
  // (under an open stream the screen's work list could not be allocated: such batches run unscreened)
  facts.screen_on = c->batch_screen && c->screen_skip == 0 && !c->st_open;
  const XcRoute r = xc_route(facts);
  if (c->batch_screen && c->screen_skip > 0 && r.kernel == XcKernel::i8) --c->screen_skip;
  if ((rc = lcs_ensure_xc(c, r.sets))) return rc;
  // ingest: int8 copies of a u8 source (the fp64 stages read them), fp16 hi / lo pairs of a complex<float> one that holds the fp16 set
  CapSrc src;
  if (r.sets & XC_SET_F16) { if ((rc = lcs_launch_ingest_f16(c, d_capbufs, n_buf, n_cap, &src))) return rc; }
  else if ((rc = lcs_launch_ingest(c, d_capbufs, fmt, n_buf, n_cap, &src))) return rc;
  Launch L = make_launch(c, n_buf, n_cap, src);
  L.geo = geo;
  L.xc = r.kernel;
  L.screen = r.screen;
  L.needed_rows_only = true;
  L.tfoec_parts = 2;
  if ((rc = lcs_launch_xcorr(c, L, false, true))) return rc;
  if ((rc = lcs_launch_peak_search(c, L, kPeakThresh, true))) return rc;
  int rounds = 0;
  if (stage_mask & 2) {
    // The per-cell stages hold max_work cells at a time, in rounds.  Round 4: the batch before is the predictor for how many
    // rounds to enqueue and how wide the per-cell grids are.  A busy band carries 4-5 cells per buffer past SSS: with the
    // rounds and grids sized for one cell per buffer, every such batch needed a second round launched from
    // lcs_batch_collect (a host round trip in the middle of the pipeline) and every workgroup walked ~8 cells one after
    // the other.  A wrong guess costs time only: the kernels loop over whatever the list holds, and collect launches the
    // missing rounds, so no batch overflows and sparse batches pay for no empty rounds.  The hint was measured on a batch
    // of hint_n_buf buffers of one format and stage mask: it is scaled to this batch's size and forgotten when the shape changed.
    int hint = 0;
    if (c->hint_n_buf > 0 && c->hint_fmt == fmt_in && c->hint_stage == stage_mask)
      hint = (int)std::min<long long>((long long)c->work_hint * n_buf / c->hint_n_buf, (long long)n_buf * LCS_MAXP);
    // a batch that carried more cells than a round holds: the limit doubles (up to LCS_MAX_WORK) unless the caller pinned it
    if (!c->max_work_pinned && !c->st_open && hint > c->max_work && c->max_work < LCS_MAX_WORK)
      c->max_work = std::min<int>(LCS_MAX_WORK, 2 * c->max_work);
    if ((rc = ensure_percell(c))) return rc;
    L.round_cells = std::min(c->max_work, c->percell_cap);      // fixed for this batch
    L.grid_items = std::min(L.round_cells, std::max(64, std::max(n_buf / 2, hint + hint / 8)));
    const int expect = std::max(n_buf, hint + hint / 4);
    rounds = std::min(8, (expect + L.round_cells - 1) / L.round_cells);
    if ((rc = launch_per_peak(c, L, 0, rounds))) return rc;
  }
  if ((rc = lcs_launch_pack_results(c, L, (stage_mask & 2) != 0))) return rc;
  c->batch = BatchRecord{L, stage_mask, fmt_in, rounds};
  return LCS_OK;
}

// Round 5: the results arrive compacted (k_pack_results at the end of the enqueued chain).  ONE copy of the header, the
// per-buffer counts and as many records as the previous batch returned (+ 25 %) into page-locked memory owned by the
// context, one synchronisation; a second copy only when the batch returned more.  No allocation, no pageable staging
// (rounds 1-4 copied n_buf x 64 records, 786 KB per 128-buffer batch, into a vector built inside the call).
int lcs_batch_collect(lcs_ctx *c, lcs_cell *cells, int max_cells_per_buf, int *n_cells) {
  if (!c || !n_cells || c->batch.l.n_buf <= 0 || max_cells_per_buf < 0 || (!cells && max_cells_per_buf > 0)) return LCS_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  BatchRecord &batch = c->batch;
  const Launch &L = batch.l;
  const int nb = L.n_buf;
  const bool full = (batch.stage_mask & 2) != 0;
  const size_t rec_off = lcs_pack_rec_offset(nb);
  const int *hdr = reinterpret_cast<const int *>(c->h_res.get());
  const int *cnt = hdr + 8;
  const lcs_cell *rec = reinterpret_cast<const lcs_cell *>(c->h_res + rec_off);
  int rc = LCS_OK;
  double host_us = 0;                                   // host time of this call outside the wait for the GPU (lcs_last_collect_host_us)
  auto t_sync_done = std::chrono::steady_clock::now();
  for (int pass = 0;; ++pass) {
    const size_t first = std::min<size_t>((size_t)nb * LCS_MAXP, (size_t)std::max(nb / 2, c->collect_hint + c->collect_hint / 4 + 8));
    const auto t_a = std::chrono::steady_clock::now();
    HIPCHK(c, hipMemcpyAsync(c->h_res, c->res_pack, rec_off + first * sizeof(lcs_cell), hipMemcpyDeviceToHost, c->stream));
    const auto t_b = std::chrono::steady_clock::now();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t_sync_done = std::chrono::steady_clock::now();
    host_us += std::chrono::duration<double, std::micro>(t_b - t_a).count();
    const int work_total = hdr[5];
    if (full && pass == 0) { c->work_hint = work_total; c->hint_n_buf = nb; c->hint_fmt = batch.fmt; c->hint_stage = batch.stage_mask; }
    if (full && pass == 0 && work_total > batch.cell_rounds * L.round_cells) {
      // more cells passed SSS than the enqueued rounds decode: run the remaining rounds now, as the batch was enqueued (rare: the
      // first dense batch)
      const int rounds = (work_total + L.round_cells - 1) / L.round_cells;
      if ((rc = launch_per_peak(c, L, batch.cell_rounds, rounds))) return rc;
      batch.cell_rounds = rounds;
      if ((rc = lcs_launch_pack_results(c, L, true))) return rc;
      continue;
    }
    if (L.screen && !batch.list_ops_counted) {      // the three-digit launch over the flagged tiles: counted once its size is known
      c->last_xc_ops += lcs_i8_list_ops(L.geo, hdr[2], hdr[3] & 0xFFFF);
      batch.list_ops_counted = true;
      if (LCS_SCREEN_DENSE * hdr[2] > nb * LCS_I8_TILES) c->screen_skip = LCS_SCREEN_SKIP;
    }
    const int total = hdr[0];
    if ((size_t)total > first) {
      HIPCHK(c, hipMemcpyAsync(c->h_res + rec_off + first * sizeof(lcs_cell), c->res_pack + rec_off + first * sizeof(lcs_cell),
                               ((size_t)total - first) * sizeof(lcs_cell), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->collect_hint = total;
    break;
  }
  if (hdr[1]) rc = LCS_ERR_OVERFLOW;          // a buffer with more than LCS_MAXP peaks: only with non-positive thresholds (lcs.h)
  size_t at = 0;
  for (int b = 0; b < nb; ++b) {
    const int n = cnt[b];
    const int take = std::min(n, max_cells_per_buf);
    if (take > 0) std::memcpy(cells + (size_t)b * max_cells_per_buf, rec + at, (size_t)take * sizeof(lcs_cell));
    if (n > max_cells_per_buf) rc = LCS_ERR_OVERFLOW;
    at += (size_t)n;
    n_cells[b] = n;
  }
  if (batch.l.src.c32) batch.l.src.c32 = c->cap32;      // complex<float> batches were read in place: the caller's buffers are no longer referenced
  c->last_collect_host_us = host_us + std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_sync_done).count();
  if (rc) c->err = "more results than the output array holds";
  return rc;
}

int lcs_last_batch_stats(lcs_ctx *c, int stats[8]) {
  if (!c || !stats || !c->h_res || c->batch.l.n_buf <= 0) return LCS_ERR_BAD_ARG;
  std::memcpy(stats, c->h_res, 8 * sizeof(int));      // the header lcs_batch_collect brought over (k_pack_results)
  return LCS_OK;
}

int lcs_last_collect_host_us(lcs_ctx *c, double *us) {
  if (!c || !us) return LCS_ERR_BAD_ARG;
  *us = c->last_collect_host_us;
  return LCS_OK;
}

int lcs_search_batch_dev(lcs_ctx *c, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap, const double *f_search_set,
                         uint16_t n_f, const double *fc_requested, const double *fc_programmed, double fs_programmed,
                         int stage_mask, lcs_cell *cells, int max_cells_per_buf, int *n_cells) {
  int rc = lcs_batch_enqueue(c, d_capbufs, fmt, n_buf, n_cap, f_search_set, n_f, fc_requested, fc_programmed,
                             fs_programmed, stage_mask);
  if (rc) return rc;
  return lcs_batch_collect(c, cells, max_cells_per_buf, n_cells);
}

// ---- host-fed batches ---------------------------------------------------------------------------------------------
// What a caller holding recorded capbuf_NNNN.it files or dongle bytes uses (the carrier loop of src/CellSearch.cpp:471-569
// with the captures in host memory).  The H2D copy is asynchronous on the context's stream: with two or three contexts
// used round-robin (enqueue batch i + 1, then collect batch i) the PCIe transfer of one batch runs under the kernels of
// the previous one.  That needs page-locked source memory: buffers from lcs_host_alloc are DMA'd in place; any other
// pointer is staged through two pinned 4 MB slots owned by the context (CPU memcpy of chunk k + 1 under the DMA of
// chunk k -- correct for every pointer, but then the CPU copy, ~10 GB/s, is what bounds the transfer).
int lcs_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int lcs_host_alloc(lcs_ctx *c, size_t bytes, void **out) {
  if (!c || !out) return LCS_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return LCS_OK;
}

int lcs_host_free(lcs_ctx *c, void *p) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (p) HIPCHK(c, hipHostFree(p));
  return LCS_OK;
}

// Device memory for callers without a HIP toolchain of their own (the host tools are plain g++): buffers they hand to the
// device-resident entry points (lcs_batch_enqueue, lcs_track_block with td_on_device, lcs_track_stream_block).
int lcs_device_alloc(lcs_ctx *c, size_t bytes, void **out) {
  if (!c || !out) return LCS_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMalloc(out, bytes ? bytes : 1));
  return LCS_OK;
}

int lcs_device_free(lcs_ctx *c, void *p) {
  if (!c) return LCS_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (p) HIPCHK(c, hipFree(p));
  return LCS_OK;
}

int lcs_device_upload(lcs_ctx *c, void *d_dst, const void *h_src, size_t bytes) {
  if (!c || !d_dst || !h_src) return LCS_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
  return LCS_OK;
}

int lcs_batch_enqueue_host(lcs_ctx *c, const void *h_capbufs, int fmt, int n_buf, uint32_t n_cap, const double *f_search_set,
                           uint16_t n_f, const double *fc_requested, const double *fc_programmed, double fs_programmed,
                           int stage_mask) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (!h_capbufs || n_buf < 1 || (fmt != LCS_FMT_C64 && fmt != LCS_FMT_IQ_U8)) { c->err = "bad argument"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)n_buf * n_cap * (fmt == LCS_FMT_IQ_U8 ? 2 : sizeof(float2));
  if (bytes > c->h2d.capacity()) {
    if (c->st_open) { c->err = "lcs_stream_close first"; return LCS_ERR_BAD_ARG; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc;
    if ((rc = c->h2d.reserve(c, bytes))) return rc;
  }
  hipPointerAttribute_t at;
  const bool locked = hipPointerGetAttributes(&at, h_capbufs) == hipSuccess && at.type == hipMemoryTypeHost;
  (void)hipGetLastError();        // an ordinary malloc'ed pointer makes the query fail: not an error here
  if (locked) {
    HIPCHK(c, hipMemcpyAsync(c->h2d, h_capbufs, bytes, hipMemcpyHostToDevice, c->stream));
  } else {
    constexpr size_t CH = (size_t)4 << 20;
    for (int k = 0; k < 2; ++k)
      if (!c->h_stage[k]) {
        int rc;
        if ((rc = c->h_stage[k].alloc(c, CH))) return rc;
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_stage[k], hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->ev_stage[k], c->stream));
      }
    int k = 0;
    for (size_t off = 0; off < bytes; off += CH, k ^= 1) {
      const size_t n = std::min(CH, bytes - off);
      HIPCHK(c, hipEventSynchronize(c->ev_stage[k]));          // the DMA that last read this slot is done
      std::memcpy(c->h_stage[k], (const char *)h_capbufs + off, n);
      HIPCHK(c, hipMemcpyAsync(c->h2d + off, c->h_stage[k], n, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipEventRecord(c->ev_stage[k], c->stream));
    }
  }
  return lcs_batch_enqueue(c, c->h2d, fmt, n_buf, n_cap, f_search_set, n_f, fc_requested, fc_programmed, fs_programmed, stage_mask);
}

int lcs_search_batch_host(lcs_ctx *c, const void *h_capbufs, int fmt, int n_buf, uint32_t n_cap, const double *f_search_set,
                          uint16_t n_f, const double *fc_requested, const double *fc_programmed, double fs_programmed,
                          int stage_mask, lcs_cell *cells, int max_cells_per_buf, int *n_cells) {
  const int rc = lcs_batch_enqueue_host(c, h_capbufs, fmt, n_buf, n_cap, f_search_set, n_f, fc_requested, fc_programmed,
                                        fs_programmed, stage_mask);
  if (rc) return rc;
  return lcs_batch_collect(c, cells, max_cells_per_buf, n_cells);
}

// Debug readback: the xcorr_pss outputs of buffer `buf` of the last batch, in the reference's layouts.
int lcs_batch_readback(lcs_ctx *c, int buf, float *single, double *pow_, int32_t *frq, double *sp_incoherent, double *z_th1) {
  if (!c || buf < 0 || buf >= c->batch.l.n_buf) { if (c) c->err = "no such buffer in the last batch"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  const XcGeom &geo = c->batch.l.geo;
  const size_t NE = 3 * LCS_N_IDX;
  int rc;
  if ((rc = lcs_launch_xcorr_complete(c, c->batch.l))) return rc;      // a screened batch: the arrays become the exact path's first
  if (single) {
    if ((rc = lcs_launch_single_layout(c, c->batch.l, buf, c->sref, 1))) return rc;
    HIPCHK(c, hipMemcpyAsync(single, c->sref, sizeof(float) * NE * geo.n_f, hipMemcpyDeviceToHost, c->stream));
  }
  if (pow_) HIPCHK(c, hipMemcpyAsync(pow_, c->pow_ + (size_t)buf * NE, sizeof(double) * NE, hipMemcpyDeviceToHost, c->stream));
  if (frq) HIPCHK(c, hipMemcpyAsync(frq, c->frq + (size_t)buf * NE, sizeof(int) * NE, hipMemcpyDeviceToHost, c->stream));
  if (sp_incoherent) HIPCHK(c, hipMemcpyAsync(sp_incoherent, c->spinc + (size_t)buf * LCS_N_IDX, sizeof(double) * LCS_N_IDX, hipMemcpyDeviceToHost, c->stream));
  if (z_th1) HIPCHK(c, hipMemcpyAsync(z_th1, c->zth + (size_t)buf * LCS_N_IDX, sizeof(double) * LCS_N_IDX, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

// ---------------------------------------------------------- single-cell stage entry points
namespace {
int upload_cap_and_params(lcs_ctx *c, const double *capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog, Launch *out) {
  int rc;
  if (!capbuf || n_cap < 128) { c->err = "bad capture buffer"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_ws(c, 1, n_cap, std::max(1, c->cap_n_f), false))) return rc;
  c->h_params = SlotParams{fc_req, fc_prog, fs_prog};      // outlives the asynchronous copy (the callers synchronise later)
  HIPCHK(c, hipMemcpyAsync(c->cap64, capbuf, sizeof(double2) * n_cap, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->params_ws, &c->h_params, sizeof(SlotParams), hipMemcpyHostToDevice, c->stream));
  *out = make_launch(c, 1, n_cap, CapSrc{nullptr, c->cap64, nullptr, n_cap});      // the stages read the fp64 copy itself
  return LCS_OK;
}
int put_single_work_item(lcs_ctx *c, const lcs_cell *cell, int n_ofdm) {
  int rc;
  if ((rc = ensure_percell(c))) return rc;
  const WorkItem wi{0, 0};
  const int nw[4] = {1, 1, 0, 0};      // one cell taken of one; no re-detections
  const double hdr[3] = {(double)n_ofdm, 0.0, 0.0};
  HIPCHK(c, hipMemcpyAsync(c->work_items, &wi, sizeof(wi), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->n_work, nw, sizeof(nw), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->cells_out, cell, sizeof(lcs_cell), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->cell_scratch, hdr, sizeof(hdr), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the sources above are stack variables
  return LCS_OK;
}
int n_ofdm_for(const lcs_cell *cell) {
  return cell->cp_type == LCS_CP_NORMAL ? 854 : (cell->cp_type == LCS_CP_EXTENDED ? 732 : -1);
}
// a cell with n_id_1 in 0 .. 167, n_id_2 in 0 .. 2 and a known cp_type
bool cell_identified(const lcs_cell *cell) { return wide_cell_identified(cell); }
// What the stages that take the caller's grid share: the workspace, the one-cell work list, the grid in `dst` (c->tfg: in the
// chain's raw grid's place, c->tfg_comp: in the compensated one's) and the cell's RS_DL table (k_cell_prep).  *L: the launch of
// the stage's own kernels.
int stage_grid(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, DevBuf<double2> lcs_ctx::*dst, Launch *L) {
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_stage_ws(c))) return rc;
  if ((rc = put_single_work_item(c, cell, n_ofdm))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->*dst, tfg, sizeof(double2) * n_ofdm * LCS_TFG_NSC, hipMemcpyHostToDevice, c->stream));
  *L = make_launch(c, 1, 0, CapSrc{});
  return lcs_launch_rs_build(c, *L);
}
// lcs_tdd_config and lcs_cell_meas, which take a raw grid of two frames .. LCS_TFG_MAX_OFDM rows and leave one record: what they
// refuse alike, under the stage's own name ...
int record_stage_check(lcs_ctx *c, const char *who, const lcs_cell *cell, int n_ofdm) {
  const char *what = nullptr;
  if (!cell_identified(cell)) what = " needs a cell with n_id_1, n_id_2 and a known cp_type";
  else if (n_ofdm < 2 * 20 * (n_ofdm_for(cell) == 854 ? 7 : 6)) what = " needs at least two frames of the grid (280 OFDM symbols with the normal CP, 240 with the extended)";
  else if (n_ofdm > LCS_TFG_MAX_OFDM) what = " takes at most LCS_TFG_MAX_OFDM (854) OFDM symbols";
  if (!what) return LCS_OK;
  c->err = std::string(who) + what;
  return LCS_ERR_BAD_ARG;
}
// ... and how their record comes back: the kernel writes it into the debug block (the fused calls' tables stay what they are)
int read_dbg_record(lcs_ctx *c, void *out, size_t bytes) {
  HIPCHK(c, hipMemcpyAsync(out, c->d_dbg, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}
}  // namespace

int lcs_sss_detect(lcs_ctx *c, const lcs_cell *cell, const double *capbuf, uint32_t n_cap, double thresh2_n_sigma,
                   double fc_req, double fc_prog, double fs_prog, lcs_cell *cell_out, double *h1_np, double *h2_np,
                   double *h1_nrm, double *h2_nrm, double *h1_ext, double *h2_ext, double *ll_nrm, double *ll_ext) {
  if (!c || !cell || !cell_out) return LCS_ERR_BAD_ARG;
  if (cell->n_id_2 < 0 || cell->n_id_2 > 2) { c->err = "cell.n_id_2 must be 0..2"; return LCS_ERR_BAD_ARG; }
  int rc;
  Launch L;
  if ((rc = upload_cap_and_params(c, capbuf, n_cap, fc_req, fc_prog, fs_prog, &L))) return rc;
  if ((rc = ensure_percell(c))) return rc;
  const int one = 1;
  HIPCHK(c, hipMemcpyAsync(c->peaks, cell, sizeof(lcs_cell), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->npeaks, &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_dbg, 0, sizeof(double) * 2048, c->stream));
  if ((rc = lcs_launch_sss_only(c, L, thresh2_n_sigma, c->d_dbg))) return rc;
  std::vector<double> dbg(1292);
  HIPCHK(c, hipMemcpyAsync(cell_out, c->peaks, sizeof(lcs_cell), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(dbg.data(), c->d_dbg, sizeof(double) * dbg.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h1_np) std::memcpy(h1_np, &dbg[0], 62 * sizeof(double));
  if (h2_np) std::memcpy(h2_np, &dbg[62], 62 * sizeof(double));
  if (h1_nrm) std::memcpy(h1_nrm, &dbg[124], 124 * sizeof(double));
  if (h2_nrm) std::memcpy(h2_nrm, &dbg[248], 124 * sizeof(double));
  if (h1_ext) std::memcpy(h1_ext, &dbg[372], 124 * sizeof(double));
  if (h2_ext) std::memcpy(h2_ext, &dbg[496], 124 * sizeof(double));
  if (ll_nrm) std::memcpy(ll_nrm, &dbg[620], 336 * sizeof(double));
  if (ll_ext) std::memcpy(ll_ext, &dbg[956], 336 * sizeof(double));
  return LCS_OK;
}

int lcs_pss_sss_foe(lcs_ctx *c, const lcs_cell *cell_in, const double *capbuf, uint32_t n_cap, double fc_req,
                    double fc_prog, double fs_prog, lcs_cell *cell_out) {
  if (!c || !cell_in || !cell_out) return LCS_ERR_BAD_ARG;
  if (!cell_identified(cell_in)) {
    c->err = "pss_sss_foe needs a cell with n_id_1, n_id_2 and a known cp_type";   // the reference throws (src/searcher.cpp:786)
    return LCS_ERR_BAD_ARG;
  }
  int rc;
  Launch L;
  if ((rc = upload_cap_and_params(c, capbuf, n_cap, fc_req, fc_prog, fs_prog, &L))) return rc;
  const int one = 1;
  HIPCHK(c, hipMemcpyAsync(c->peaks, cell_in, sizeof(lcs_cell), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->npeaks, &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
  if ((rc = lcs_launch_foe_only(c, L))) return rc;
  HIPCHK(c, hipMemcpyAsync(cell_out, c->peaks, sizeof(lcs_cell), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

// The coarse estimate alone: the work list and k_foe_fin_unwrap in its read-back form -- no native estimate, no write to the record.
int lcs_pss_foe_coarse(lcs_ctx *c, const lcs_cell *cell, const double *capbuf, uint32_t n_cap, double fc_req, double fc_prog,
                       double fs_prog, double *f_coarse, double *c_re_im, int *n_occ) {
  if (!c || !cell || !f_coarse) return LCS_ERR_BAD_ARG;
  if (!cell_identified(cell)) {
    c->err = "pss_foe_coarse needs a cell with n_id_1, n_id_2 and a known cp_type";      // as lcs_pss_sss_foe: it shares its geometry
    return LCS_ERR_BAD_ARG;
  }
  int rc;
  Launch L;
  if ((rc = upload_cap_and_params(c, capbuf, n_cap, fc_req, fc_prog, fs_prog, &L))) return rc;
  if ((rc = c->foe_coarse.reserve(c, 4))) return rc;
  const int one = 1;
  double out[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(c->peaks, cell, sizeof(lcs_cell), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->npeaks, &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
  if ((rc = lcs_launch_foe_coarse(c, L, c->foe_coarse))) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c->foe_coarse, sizeof(out), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *f_coarse = out[0];
  if (c_re_im) { c_re_im[0] = out[1]; c_re_im[1] = out[2]; }
  if (n_occ) *n_occ = (int)out[3];
  return LCS_OK;
}

int lcs_extract_tfg(lcs_ctx *c, const lcs_cell *cell, const double *capbuf, uint32_t n_cap, double fc_req,
                    double fc_prog, double fs_prog, double *tfg, double *tfg_timestamp, int *n_ofdm) {
  if (!c || !cell || !tfg || !tfg_timestamp || !n_ofdm) return LCS_ERR_BAD_ARG;
  const int no = n_ofdm_for(cell);
  if (no < 0) { c->err = "extract_tfg needs a known cp_type"; return LCS_ERR_BAD_ARG; }   // ref :883 throws
  int rc;
  Launch L;
  if ((rc = upload_cap_and_params(c, capbuf, n_cap, fc_req, fc_prog, fs_prog, &L))) return rc;
  if ((rc = put_single_work_item(c, cell, no))) return rc;
  if ((rc = lcs_launch_tfg(c, L, false))) return rc;
  double oob = 0;
  HIPCHK(c, hipMemcpyAsync(tfg, c->tfg, sizeof(double2) * no * LCS_TFG_NSC, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tfg_timestamp, c->tfg_ts, sizeof(double) * no, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&oob, c->cell_scratch + 2, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_ofdm = no;
  if (oob != 0.0) { c->err = "a DFT window falls outside the capture buffer (the reference would read out of bounds)"; return LCS_ERR_BAD_ARG; }
  return LCS_OK;
}

int lcs_tfoec(lcs_ctx *c, const lcs_cell *cell, const double *tfg, const double *tfg_timestamp, int n_ofdm,
              double fc_req, double fc_prog, double *tfg_comp, double *tfg_comp_timestamp, lcs_cell *cell_out) {
  if (!c || !cell || !tfg || !tfg_timestamp || !tfg_comp || !tfg_comp_timestamp || !cell_out) return LCS_ERR_BAD_ARG;
  if (n_ofdm_for(cell) < 0 || n_ofdm < 14 || n_ofdm > LCS_TFG_MAX_OFDM || cell->n_id_1 < 0 || cell->n_id_2 < 0) {
    c->err = "tfoec needs a detected cell and 14..854 OFDM symbols";
    return LCS_ERR_BAD_ARG;
  }
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_stage_ws(c))) return rc;
  SlotParams p{fc_req, fc_prog, 0.0};
  HIPCHK(c, hipMemcpyAsync(c->params_ws, &p, sizeof(p), hipMemcpyHostToDevice, c->stream));
  if ((rc = put_single_work_item(c, cell, n_ofdm))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->tfg, tfg, sizeof(double2) * n_ofdm * LCS_TFG_NSC, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->tfg_ts, tfg_timestamp, sizeof(double) * n_ofdm, hipMemcpyHostToDevice, c->stream));
  const Launch L = make_launch(c, 1, 0, CapSrc{});
  if ((rc = lcs_launch_rs_build(c, L))) return rc;
  if ((rc = lcs_launch_tfoec(c, L, true))) return rc;
  HIPCHK(c, hipMemcpyAsync(tfg_comp, c->tfg_comp, sizeof(double2) * n_ofdm * LCS_TFG_NSC, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tfg_comp_timestamp, c->tfg_ts_comp, sizeof(double) * n_ofdm, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cell_out, c->cells_out, sizeof(lcs_cell), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

int lcs_decode_mib(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, lcs_cell *cell_out) {
  if (!c || !cell || !tfg || !cell_out) return LCS_ERR_BAD_ARG;
  const int need = n_ofdm_for(cell);
  if (need < 0 || n_ofdm != need || cell->n_id_1 < 0 || cell->n_id_2 < 0) {
    c->err = "decode_mib needs a detected cell and its full 854/732-symbol grid";
    return LCS_ERR_BAD_ARG;
  }
  int rc;
  Launch L;
  if ((rc = stage_grid(c, cell, tfg, n_ofdm, &lcs_ctx::tfg_comp, &L))) return rc;
  L.needed_rows_only = true;      // decode_mib reads the channel estimate on PBCH rows only
  if ((rc = lcs_launch_mib(c, L, false))) return rc;
  HIPCHK(c, hipMemcpyAsync(cell_out, c->cells_out, sizeof(lcs_cell), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

// The soft values of one forced PBCH candidate (for tests): staged exactly as lcs_decode_mib, so the channel estimate is the
// PBCH-rows-only form that decode_mib reads; k_pbch_soft leaves the values in the debug block.
int lcs_pbch_soft(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int frame_timing_guess, int n_ports,
                  double *e_est, double *d_est, uint64_t *bits40, int *crc_ok) {
  if (!c || !cell || !tfg || !e_est || !d_est || !bits40 || !crc_ok) return LCS_ERR_BAD_ARG;
  const int need = n_ofdm_for(cell);
  if (need < 0 || n_ofdm != need || cell->n_id_1 < 0 || cell->n_id_2 < 0) {
    c->err = "pbch_soft needs a detected cell and its full 854/732-symbol grid";
    return LCS_ERR_BAD_ARG;
  }
  if (frame_timing_guess < 0 || frame_timing_guess > 3 || (n_ports != 1 && n_ports != 2 && n_ports != 4)) {
    c->err = "pbch_soft needs a frame_timing_guess of 0 .. 3 and n_ports of 1, 2 or 4";
    return LCS_ERR_BAD_ARG;
  }
  int rc;
  Launch L;
  if ((rc = stage_grid(c, cell, tfg, n_ofdm, &lcs_ctx::tfg_comp, &L))) return rc;
  L.needed_rows_only = true;      // as lcs_decode_mib
  if ((rc = lcs_launch_pbch_soft(c, L, frame_timing_guess, n_ports, c->d_dbg))) return rc;
  std::vector<double> dbg(2048);
  if ((rc = read_dbg_record(c, dbg.data(), sizeof(double) * dbg.size()))) return rc;
  int at_d, at_bits, at_ok;
  lcs_pbch_soft_layout(&at_d, &at_bits, &at_ok);
  const int m_bit = need == 854 ? 1920 : 1728;
  std::memcpy(e_est, &dbg[0], sizeof(double) * m_bit);
  std::memcpy(d_est, &dbg[at_d], sizeof(double) * 120);
  std::memcpy(bits40, &dbg[at_bits], sizeof(uint64_t));
  *crc_ok = dbg[at_ok] != 0.0;
  return LCS_OK;
}

// The uplink-downlink configuration as a stage (tdd_config.h): the caller's grid takes the place of the chain's raw one, k_cell_prep
// builds RS_DL, k_tdd_config writes its record into the debug block.
int lcs_tdd_config(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, lcs_tdd_info *out) {
  if (!c || !cell || !tfg || !out) return LCS_ERR_BAD_ARG;
  int rc;
  Launch L;
  if ((rc = record_stage_check(c, "tdd_config", cell, n_ofdm)) || (rc = stage_grid(c, cell, tfg, n_ofdm, &lcs_ctx::tfg, &L))) return rc;
  static_assert(sizeof(lcs_tdd_info) <= 2048 * sizeof(double), "the debug block holds a record");
  if ((rc = lcs_launch_tdd_config(c, L, reinterpret_cast<lcs_tdd_info *>(c->d_dbg.get()), true))) return rc;
  return read_dbg_record(c, out, sizeof(*out));
}

// RSRP, RSSI, RSRQ and the noise power as a stage (cell_meas.h), as lcs_tdd_config
int lcs_cell_meas(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int dl_mask, lcs_meas_info *out) {
  if (!c || !cell || !tfg || !out) return LCS_ERR_BAD_ARG;
  int rc;
  Launch L;
  if ((rc = record_stage_check(c, "cell_meas", cell, n_ofdm))) return rc;
  if (!meas_mask_ok(dl_mask)) { c->err = "cell_meas needs a dl_mask with at least one of the bits 0 .. 9 and none above"; return LCS_ERR_BAD_ARG; }
  if ((rc = stage_grid(c, cell, tfg, n_ofdm, &lcs_ctx::tfg, &L))) return rc;
  static_assert(sizeof(lcs_meas_info) <= 2048 * sizeof(double), "the debug block holds a record");
  if ((rc = lcs_launch_cell_meas(c, L, nullptr, reinterpret_cast<lcs_meas_info *>(c->d_dbg.get()), dl_mask, true))) return rc;
  return read_dbg_record(c, out, sizeof(*out));
}

// ---- the stages on the full-bandwidth grid (tfg_wide.hip, cell_meas_wide.h, pcfich.hip, pdcch.hip, pdcch_scan.hip, phich.hip,
// pdsch.hip; what they refuse and plan alike: wide_call.h).  They touch the context's stream, the blocks of c->meas_wide and their own
// and nothing else: no workspace, no mode, no table of a fused call -- so they run beside an open stream as well.
namespace {
int wide_refused(lcs_ctx *c, const char *who, const char *what) {
  c->err = std::string(who) + ": " + what;
  return LCS_ERR_BAD_ARG;
}
// where a call's grid comes from: complex<float> samples on the device, of which the rows it needs are transformed, or the whole grid
// [n_ofdm][12 n_rb] from the host
struct WideSource {
  bool samples;
  const void *d_capbuf; uint32_t n_cap; double fc_req, fc_prog, fs_prog; int n_fft;
  const double *tfg;
};
WideSource wide_samples(const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog, int n_fft) {
  return WideSource{true, d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft, nullptr};
}
WideSource wide_host_grid(const double *tfg) { return WideSource{false, nullptr, 0, 0.0, 0.0, 0.0, 0, tfg}; }
// what wide_begin leaves for the plan and for wide_fill_grid.  Of samples: ts[t] = the ideal location of row t, kk = the frequency
// correction's phase step in half turns per sample (fshift, ref dsp.h:40-53); ideal[0 .. n_ideal - 1]: the locations of the rows a
// transform is asked for.  The plan of a stage: need, first, rows and n_sf as wide_plan_rows gives them.
struct WideCall {
  int n_symb = 0;
  bool samples = false, device_set = false;
  std::vector<double> ts, gathered;
  double kk = 0.0;
  const double *ideal = nullptr;
  size_t n_ideal = 0;
  int n_sf = 0, need[PCF_MAX_SF], first[PCF_MAX_SF], rows[4 * PCF_MAX_SF];
  // need -> first, rows, n_sf; of samples also the locations of the planned rows (one block for the list, one for the locations)
  void plan(int n_ofdm, int keep, int rec) {
    std::vector<int> list;
    if (samples) {
      size_t n = 0;
      for (int g = 0; g < pcf_n_sf(n_ofdm, n_symb); ++g) n += (size_t)need[g];
      list.reserve(n);
    }
    n_sf = wide_plan_rows(n_symb, n_ofdm, keep, rec, need, rows, first, samples ? &list : nullptr);
    gathered.resize(list.size());
    for (size_t i = 0; i < list.size(); ++i) gathered[i] = ts[(size_t)list[i]];
    ideal = gathered.data(); n_ideal = gathered.size();
  }
};
// What the sample entries refuse alike, then extract_tfg's walk (ref src/searcher.cpp:875-920) with the caller's rate
int wide_rows(lcs_ctx *c, const char *who, const lcs_cell *cell, const WideSource &s, int n_rb, int n_ofdm, WideCall *w) {
  const char *what;
  if (!cell || !s.d_capbuf) return wide_refused(c, who, "a null pointer");
  if (reinterpret_cast<uintptr_t>(s.d_capbuf) & 7) return wide_refused(c, who, "d_capbuf is not aligned to a complex<float>");
  if (measw_log2r(s.n_fft) < 0) return wide_refused(c, who, "n_fft is not 128, 256, 512, 1024 or 2048");
  if (!(fabs(s.fs_prog / (15000.0 * s.n_fft) - 1.0) < 1e-3)) return wide_refused(c, who, "fs_programmed is not 15 kHz x n_fft to within 1e-3");
  if (!measw_rb_ok(s.n_fft, n_rb)) return wide_refused(c, who, "n_rb is outside 6 .. {6, 15, 25, 50, 100} for n_fft = 128 {1, 2, 4, 8, 16}");
  if ((what = wide_refuse_cell(cell))) return wide_refused(c, who, what);
  const int n_symb = w->n_symb = cell->cp_type == LCS_CP_NORMAL ? 7 : 6;
  if ((what = wide_refuse_n_ofdm(n_ofdm, n_symb))) return wide_refused(c, who, what);
  const double fs_prog = s.fs_prog, k_factor = (s.fc_req - cell->freq_fine) / s.fc_prog;
  double loc;
  if (cell->cp_type == LCS_CP_NORMAL) loc = cell->frame_start + 10 * 16 / FS_LTE * fs_prog * k_factor;
  else loc = cell->frame_start + 32 * 16 / FS_LTE * fs_prog * k_factor;
  if (loc - .01 * fs_prog * k_factor > -0.5) loc = loc - .01 * fs_prog * k_factor;
  const double inc_ext = (128 + 32) * 16 / FS_LTE * fs_prog * k_factor;
  const double inc_10 = (128 + 10) * 16 / FS_LTE * fs_prog * k_factor;
  const double inc_9 = (128 + 9) * 16 / FS_LTE * fs_prog * k_factor;
  w->ts.resize((size_t)n_ofdm);
  int sym_num = 0;
  for (int t = 0; t < n_ofdm; ++t) {
    w->ts[t] = loc;
    if (n_symb == 6) loc += inc_ext;
    else { loc += (sym_num == 6) ? inc_10 : inc_9; sym_num = (sym_num + 1) % 7; }
  }
  w->kk = (-cell->freq_fine) / ((fs_prog * k_factor) / 2);
  if (!std::isfinite(w->ts[0]) || !std::isfinite(w->ts[(size_t)n_ofdm - 1]) || !std::isfinite(w->kk))
    return wide_refused(c, who, "the cell's frame_start / freq_fine and the frequencies give no finite positions");
  return LCS_OK;
}
// The refusals every entry point shares, in one order for both sources: the record `out`, the source's own, the cell, n_ofdm; then
// the mask (dl_mask null: the entry takes none) and, for the stages that decode (lte_rb), the bandwidth.  Nothing is launched.
int wide_begin(lcs_ctx *c, const char *who, const WideSource &s, const lcs_cell *cell, const void *out, int n_rb, int n_ofdm, const int *dl_mask, bool lte_rb,
               WideCall *w) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (!out) return wide_refused(c, who, "a null pointer");
  const char *what;
  int rc;
  w->samples = s.samples;
  if (s.samples) {
    if ((rc = wide_rows(c, who, cell, s, n_rb, n_ofdm, w))) return rc;
  } else {
    if (!cell || !s.tfg) return wide_refused(c, who, "a null pointer");
    if ((what = wide_refuse_cell(cell))) return wide_refused(c, who, what);
    w->n_symb = cell->cp_type == LCS_CP_NORMAL ? 7 : 6;
    if ((what = wide_refuse_n_ofdm(n_ofdm, w->n_symb))) return wide_refused(c, who, what);
  }
  if (dl_mask && (what = wide_refuse_mask(*dl_mask))) return wide_refused(c, who, what);
  if (lte_rb && (what = wide_refuse_rb(cell->n_rb_dl, n_rb))) return wide_refused(c, who, what);
  static_assert(122 * 7 <= LCS_TFG_MAX_OFDM && 61 <= PCF_MAX_SF, "the subframes of 122 slots fit the records");
  return LCS_OK;
}
// The rows of the call into c->meas_wide.grid.  Samples: the rows at w.ideal, which must all lie inside the capture -- the locations
// grow, so the first and the last decide -- (none: nothing to transform); a host grid: all of it.
int wide_fill_grid(lcs_ctx *c, const char *who, const WideSource &s, const WideCall &w, int n_rb, int n_ofdm) {
  if (s.samples && w.n_ideal) {
    if (rint(w.ideal[0]) < 0.0) return wide_refused(c, who, "the first requested row starts before sample 0 of the capture");
    if (rint(w.ideal[w.n_ideal - 1]) + (double)s.n_fft > (double)s.n_cap)
      return wide_refused(c, who, "the capture does not hold the last requested row (round_i(location) + n_fft > n_cap)");
  }
  if (!w.device_set) HIPCHK(c, hipSetDevice(c->device));      // (the PHICH has set it for its tables)
  if (!s.samples) return lcs_pcfich_stage_grid(c, s.tfg, (size_t)n_ofdm * 12 * n_rb);
  if (!w.n_ideal) return LCS_OK;
  return lcs_launch_tfg_wide(c, static_cast<const float2 *>(s.d_capbuf), s.n_cap, w.ideal, (int)w.n_ideal, w.kk, s.n_fft, n_rb);
}
// how a stage's record comes back
int wide_read_record(lcs_ctx *c, void *out, const void *d_rec, size_t bytes) {
  HIPCHK(c, hipMemcpyAsync(out, d_rec, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}
}  // namespace

int lcs_extract_tfg_wide(lcs_ctx *c, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog,
                         int n_fft, int n_rb, int n_ofdm, double *tfg, double *timestamp) {
  static const char who[] = "lcs_extract_tfg_wide";
  const WideSource src = wide_samples(d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft);
  WideCall w;
  int rc;
  if ((rc = wide_begin(c, who, src, cell, tfg, n_rb, n_ofdm, nullptr, false, &w))) return rc;
  w.ideal = w.ts.data(); w.n_ideal = w.ts.size();      // every row
  if ((rc = wide_fill_grid(c, who, src, w, n_rb, n_ofdm))) return rc;
  HIPCHK(c, hipMemcpyAsync(tfg, c->meas_wide.grid, sizeof(double2) * (size_t)n_ofdm * 12 * n_rb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (timestamp) std::memcpy(timestamp, w.ts.data(), sizeof(double) * (size_t)n_ofdm);
  return LCS_OK;
}

int lcs_cell_meas_wide(lcs_ctx *c, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog,
                       int n_fft, int n_rb, int n_ofdm, int dl_mask, lcs_meas_wide_info *out) {
  static const char who[] = "lcs_cell_meas_wide";
  const WideSource src = wide_samples(d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft);
  WideCall w;
  int rc;
  if ((rc = wide_begin(c, who, src, cell, out, n_rb, n_ofdm, &dl_mask, false, &w))) return rc;
  // port 0's reference rows only: reference row q is row q of the device's grid
  const int n_q = tdd_n_ref_rows(n_ofdm, w.n_symb);
  static_assert(2 * 122 <= TC_MAX_Q, "the reference rows of 122 slots fit the per-row table");
  w.gathered.resize((size_t)n_q);
  for (int q = 0; q < n_q; ++q) w.gathered[q] = w.ts[(size_t)tdd_grid_row(q, w.n_symb)];
  w.ideal = w.gathered.data(); w.n_ideal = w.gathered.size();
  if ((rc = wide_fill_grid(c, who, src, w, n_rb, n_ofdm))) return rc;
  if ((rc = lcs_launch_cell_meas_wide(c, *cell, n_q, n_fft, n_rb, dl_mask))) return rc;
  return wide_read_record(c, out, c->meas_wide.rec.get(), sizeof(*out));
}

// ---- the PCFICH on that grid (pcfich.hip, pcfich.h).  Every stage below is one function over a WideSource -- begin, resolve, plan,
// fill, launch, read -- and two entry points that name the source.
namespace {
int pcfich_call(lcs_ctx *c, const char *who, const WideSource &src, const lcs_cell *cell, int n_rb, int n_ofdm, int dl_mask, lcs_pcfich_info *out) {
  WideCall w;
  int rc;
  if ((rc = wide_begin(c, who, src, cell, out, n_rb, n_ofdm, &dl_mask, true, &w))) return rc;
  pcfich_need(w.n_symb, n_ofdm, pcf_ports(cell->n_ports), dl_mask, w.need);
  w.plan(n_ofdm, 2, 2);
  if ((rc = wide_fill_grid(c, who, src, w, n_rb, n_ofdm))) return rc;
  if ((rc = lcs_launch_pcfich(c, *cell, w.rows, w.n_sf, n_rb, dl_mask))) return rc;
  return wide_read_record(c, out, c->meas_wide.pcf_rec.get(), sizeof(*out));
}
}  // namespace

int lcs_pcfich_wide(lcs_ctx *c, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog,
                    int n_fft, int n_rb, int n_ofdm, int dl_mask, lcs_pcfich_info *out) {
  return pcfich_call(c, "lcs_pcfich_wide", wide_samples(d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft), cell, n_rb, n_ofdm, dl_mask, out);
}
int lcs_pcfich(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int n_rb, int dl_mask, lcs_pcfich_info *out) {
  return pcfich_call(c, "lcs_pcfich", wide_host_grid(tfg), cell, n_rb, n_ofdm, dl_mask, out);
}

// ---- the PDCCH common search space on that grid (pdcch.hip, pdcch.h)
namespace {
// what cfg and the cell say together, or the refusal
int pdcch_resolve(lcs_ctx *c, const char *who, const lcs_cell *cell, int n_rb, const lcs_pdcch_cfg *cfg, PdcchPlan *p) {
  if (!cfg) return wide_refused(c, who, "a null pointer");
  const char *sizes = nullptr;
  p->n_sizes = cfg->n_sizes;
  p->size[0] = p->size[1] = 0;
  if (cfg->n_sizes < 1 || cfg->n_sizes > LCS_PDCCH_MAX_SIZES) sizes = "n_sizes is outside 1 .. 2";
  for (int i = 0; !sizes && i < cfg->n_sizes; ++i) {
    if (cfg->size[i] < 8 || cfg->size[i] > 48) sizes = "a payload size is outside 8 .. 48";
    p->size[i] = cfg->size[i];
  }
  const char *what = wide_resolve_shared(cell->phich_duration, cell->phich_resource, cfg->phich_duration, cfg->phich_resource, cfg->phich_mi, cfg->rnti_mask,
                                         cfg->cfi_force, n_rb, sizes, &p->sh);
  return what ? wide_refused(c, who, what) : LCS_OK;
}
int pdcch_call(lcs_ctx *c, const char *who, const WideSource &src, const lcs_cell *cell, int n_rb, int n_ofdm, int dl_mask, const lcs_pdcch_cfg *cfg, lcs_pdcch_info *out) {
  WideCall w;
  PdcchPlan plan;
  int rc;
  if ((rc = wide_begin(c, who, src, cell, out, n_rb, n_ofdm, &dl_mask, true, &w)) || (rc = pdcch_resolve(c, who, cell, n_rb, cfg, &plan))) return rc;
  pdcch_need(w.n_symb, n_ofdm, n_rb, dl_mask, plan.sh, w.need);
  w.plan(n_ofdm, 4, 4);
  if ((rc = wide_fill_grid(c, who, src, w, n_rb, n_ofdm))) return rc;
  if ((rc = lcs_launch_pdcch(c, *cell, w.rows, w.n_sf, n_rb, dl_mask, plan))) return rc;
  return wide_read_record(c, out, c->pdcch.rec.get(), sizeof(*out));
}
}  // namespace

int lcs_pdcch_wide(lcs_ctx *c, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog,
                   int n_fft, int n_rb, int n_ofdm, int dl_mask, const lcs_pdcch_cfg *cfg, lcs_pdcch_info *out) {
  return pdcch_call(c, "lcs_pdcch_wide", wide_samples(d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft), cell, n_rb, n_ofdm, dl_mask, cfg, out);
}
int lcs_pdcch(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int n_rb, int dl_mask, const lcs_pdcch_cfg *cfg, lcs_pdcch_info *out) {
  return pdcch_call(c, "lcs_pdcch", wide_host_grid(tfg), cell, n_rb, n_ofdm, dl_mask, cfg, out);
}

// ---- the blind search of every CCE on that grid (pdcch_scan.hip, pdcch_scan.h)
namespace {
// the refusals on the fields the configurations share, then this stage's own
int pdcch_scan_resolve(lcs_ctx *c, const char *who, const lcs_cell *cell, int n_rb, const lcs_pdcch_scan_cfg *cfg, PdcchScanPlan *p) {
  if (!cfg) return wide_refused(c, who, "a null pointer");
  const char *what = wide_resolve_shared(cell->phich_duration, cell->phich_resource, cfg->phich_duration, cfg->phich_resource, cfg->phich_mi, cfg->rnti_mask,
                                         cfg->cfi_force, n_rb, nullptr, &p->sh);
  if (what) return wide_refused(c, who, what);
  if (cfg->n_sizes < 1 || cfg->n_sizes > LCS_PDCCH_SCAN_MAX_SIZES) return wide_refused(c, who, "n_sizes is outside 1 .. 6");
  for (int i = 0; i < LCS_PDCCH_SCAN_MAX_SIZES; ++i) p->size[i] = 0;
  for (int i = 0; i < cfg->n_sizes; ++i) {
    if (cfg->size[i] < 8 || cfg->size[i] > 64) return wide_refused(c, who, "a payload size is outside 8 .. 64");
    p->size[i] = cfg->size[i];
  }
  if (cfg->min_repeat < 1) return wide_refused(c, who, "min_repeat is below 1");
  if (!(cfg->min_quality >= 0.0 && cfg->min_quality <= 1.0)) return wide_refused(c, who, "min_quality is outside 0 .. 1");
  if (cfg->reserved[0] || cfg->reserved[1]) return wide_refused(c, who, "a reserved field is not zero");
  p->n_sizes = cfg->n_sizes; p->min_repeat = cfg->min_repeat; p->min_quality = cfg->min_quality;
  return LCS_OK;
}
int pdcch_scan_call(lcs_ctx *c, const char *who, const WideSource &src, const lcs_cell *cell, int n_rb, int n_ofdm, int dl_mask, const lcs_pdcch_scan_cfg *cfg,
                    lcs_pdcch_scan_info *out) {
  WideCall w;
  PdcchScanPlan plan;
  int rc;
  if ((rc = wide_begin(c, who, src, cell, out, n_rb, n_ofdm, &dl_mask, true, &w)) || (rc = pdcch_scan_resolve(c, who, cell, n_rb, cfg, &plan))) return rc;
  pdcch_need(w.n_symb, n_ofdm, n_rb, dl_mask, plan.sh, w.need);
  w.plan(n_ofdm, 4, 4);
  if ((rc = wide_fill_grid(c, who, src, w, n_rb, n_ofdm))) return rc;
  if ((rc = lcs_launch_pdcch_scan(c, *cell, w.rows, w.n_sf, n_rb, dl_mask, plan))) return rc;
  lcs_ctx::PdcchScan &p = c->pdcch_scan;
  if ((rc = wide_read_record(c, out, p.rec.get(), sizeof(*out)))) return rc;
  for (int g = 0; g < w.n_sf; ++g) p.last_n_cand[g] = out->sf[g].n_cand;
  p.last_n_sizes = plan.n_sizes;
  p.last_n_sf = w.n_sf;
  return LCS_OK;
}
}  // namespace

int lcs_pdcch_scan_wide(lcs_ctx *c, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog,
                        int n_fft, int n_rb, int n_ofdm, int dl_mask, const lcs_pdcch_scan_cfg *cfg, lcs_pdcch_scan_info *out) {
  return pdcch_scan_call(c, "lcs_pdcch_scan_wide", wide_samples(d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft), cell, n_rb, n_ofdm, dl_mask, cfg, out);
}
int lcs_pdcch_scan(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int n_rb, int dl_mask, const lcs_pdcch_scan_cfg *cfg, lcs_pdcch_scan_info *out) {
  return pdcch_scan_call(c, "lcs_pdcch_scan", wide_host_grid(tfg), cell, n_rb, n_ofdm, dl_mask, cfg, out);
}

int lcs_pdcch_scan_decodes(lcs_ctx *c, int g, lcs_pdcch_scan_dec *out, int cap) {
  if (!c) return LCS_ERR_BAD_ARG;
  static const char who[] = "lcs_pdcch_scan_decodes";
  lcs_ctx::PdcchScan &p = c->pdcch_scan;
  if (!out) return wide_refused(c, who, "a null pointer");
  if (p.last_n_sf == 0) return wide_refused(c, who, "the context has run no scan");
  if (g < 0 || g >= p.last_n_sf) return wide_refused(c, who, "g is outside the subframes of the last scan");
  const int n_cand = p.last_n_cand[g], n = n_cand * p.last_n_sizes;
  if (cap < n) return wide_refused(c, who, "cap is below n_cand * n_sizes of that subframe");
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  p.h_tab.resize((size_t)PSC_MAX_CAND * PSC_SIZES);
  HIPCHK(c, hipMemcpyAsync(p.h_tab.data(), p.tab.get() + (size_t)g * PSC_MAX_CAND * PSC_SIZES, sizeof(lcs_pdcch_scan_dec) * (size_t)n_cand * PSC_SIZES,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n_cand; ++i)
    for (int si = 0; si < p.last_n_sizes; ++si) out[i * p.last_n_sizes + si] = p.h_tab[(size_t)i * PSC_SIZES + si];
  return n;
}

// ---- the PHICH on that grid (phich.hip, phich.h): blocks of its own
namespace {
// what cfg (or its absence) and the cell say together, or the refusal
int phich_resolve(lcs_ctx *c, const char *who, const lcs_cell *cell, int n_rb, const lcs_phich_cfg *cfg, PhichPlan *p) {
  p->min_amp = cfg ? cfg->min_amp : LCS_PHICH_MIN_AMP;
  p->min_sigma = cfg ? cfg->min_sigma : LCS_PHICH_MIN_SIGMA;
  const char *what = wide_resolve_shared(cell->phich_duration, cell->phich_resource, cfg ? cfg->phich_duration : 0, cfg ? cfg->phich_resource : 0,
                                         cfg ? cfg->phich_mi : nullptr, 0, 0, n_rb, nullptr, &p->sh);
  if (what) return wide_refused(c, who, what);
  if (!(p->min_amp >= 0.0) || !std::isfinite(p->min_amp)) return wide_refused(c, who, "min_amp is negative or not finite");
  if (!(p->min_sigma >= 0.0) || !std::isfinite(p->min_sigma)) return wide_refused(c, who, "min_sigma is negative or not finite");
  if (cfg && (cfg->reserved[0] || cfg->reserved[1])) return wide_refused(c, who, "a reserved field is not zero");
  return LCS_OK;
}
int phich_call(lcs_ctx *c, const char *who, const WideSource &src, const lcs_cell *cell, int n_rb, int n_ofdm, int dl_mask, const lcs_phich_cfg *cfg, lcs_phich_info *out) {
  WideCall w;
  PhichPlan plan;
  int rc;
  if ((rc = wide_begin(c, who, src, cell, out, n_rb, n_ofdm, &dl_mask, true, &w)) || (rc = phich_resolve(c, who, cell, n_rb, cfg, &plan))) return rc;
  // the tables before the plan: a subframe whose map is refused is not read
  HIPCHK(c, hipSetDevice(c->device));
  w.device_set = true;
  if ((rc = lcs_phich_tables(c, *cell, n_rb, plan))) return rc;
  const int units[3] = {lcs_phich_map_units(c, 0), lcs_phich_map_units(c, 1), lcs_phich_map_units(c, 2)};
  phich_need(w.n_symb, n_ofdm, pcf_ports(cell->n_ports), dl_mask, plan.sh, units, w.need);
  w.plan(n_ofdm, 3, 3);
  if ((rc = wide_fill_grid(c, who, src, w, n_rb, n_ofdm))) return rc;
  if ((rc = lcs_launch_phich(c, *cell, w.rows, w.n_sf, n_rb, dl_mask, plan))) return rc;
  lcs_ctx::Phich &p = c->phich;
  p.last_n_sf = 0;
  if ((rc = wide_read_record(c, out, p.rec.get(), sizeof(*out)))) return rc;
  for (int g = 0; g < w.n_sf; ++g) p.last_n_unit[g] = out->sf[g].n_unit;
  p.last_n_sf = w.n_sf;
  return LCS_OK;
}
}  // namespace

int lcs_phich_wide(lcs_ctx *c, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog,
                   int n_fft, int n_rb, int n_ofdm, int dl_mask, const lcs_phich_cfg *cfg, lcs_phich_info *out) {
  return phich_call(c, "lcs_phich_wide", wide_samples(d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft), cell, n_rb, n_ofdm, dl_mask, cfg, out);
}
int lcs_phich(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int n_rb, int dl_mask, const lcs_phich_cfg *cfg, lcs_phich_info *out) {
  return phich_call(c, "lcs_phich", wide_host_grid(tfg), cell, n_rb, n_ofdm, dl_mask, cfg, out);
}

int lcs_phich_values(lcs_ctx *c, int g, double *out, int cap) {
  if (!c) return LCS_ERR_BAD_ARG;
  static const char who[] = "lcs_phich_values";
  lcs_ctx::Phich &p = c->phich;
  if (!out) return wide_refused(c, who, "a null pointer");
  if (p.last_n_sf == 0) return wide_refused(c, who, "the context has run no PHICH call");
  if (g < 0 || g >= p.last_n_sf) return wide_refused(c, who, "g is outside the subframes of the last call");
  const int n = p.last_n_unit[g] > 0 ? 8 * p.last_n_unit[g] : 0;
  if (cap < n) return wide_refused(c, who, "cap is below n_group * n_seq of that subframe");
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  p.h_tab.resize((size_t)LCS_PHICH_MAX_ENTRIES);
  HIPCHK(c, hipMemcpyAsync(p.h_tab.data(), p.tab.get() + (size_t)g * LCS_PHICH_MAX_ENTRIES, sizeof(lcs_ctx::PhichEntry) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) out[i] = p.h_tab[(size_t)i].value;
  return n;
}

// ---- the PDSCH behind the grants of that search space (pdsch.hip, pdsch.h)
namespace {
int pdsch_resolve(lcs_ctx *c, const char *who, const PdcchPlan &plan, const lcs_pdsch_cfg *pc, int n_ofdm, int n_symb, int n_rb, PdschPlan *p) {
  static const lcs_pdsch_cfg zero = {};
  if (!pc) pc = &zero;
  if (pc->max_iter < 0 || pc->max_iter > 16) return wide_refused(c, who, "max_iter is outside 1 .. 16 (0: 8)");
  if (pc->rnti_mask < 0 || pc->rnti_mask > 7) return wide_refused(c, who, "the PDSCH rnti_mask is outside 0 .. 7");
  if (pc->i_1a < 0 || pc->i_1a >= plan.n_sizes) return wide_refused(c, who, "i_1a is outside the PDCCH configuration's sizes");
  if (pc->n_forced < 0 || pc->n_forced > LCS_PDSCH_MAX_FORCED) return wide_refused(c, who, "n_forced is outside 0 .. 4");
  p->i_1a = pc->i_1a; p->max_iter = pc->max_iter ? pc->max_iter : 8; p->rnti_mask = pc->rnti_mask ? pc->rnti_mask : 7; p->n_forced = pc->n_forced;
  p->tdd = plan.sh.tdd;
  const lcs_pdsch_alloc_cfg &al = c->pdsch.alloc;           // lcs_set_pdsch_alloc: the launch takes it as an argument
  if ((al.flags & 2) && plan.n_sizes < 2) return wide_refused(c, who, "format 1C is followed (lcs_set_pdsch_alloc) but the PDCCH configuration has one size");
  if ((al.flags & 2) && plan.size[1 - pc->i_1a] != (n_rb >= 50 ? 1 : 0) + pds_1c_riv_bits(n_rb) + 5)
    return wide_refused(c, who, "format 1C is followed (lcs_set_pdsch_alloc) but the PDCCH configuration's other size is not format 1C's for this bandwidth");
  p->alloc_flags = al.flags; p->sfn0 = al.sfn0; p->si_window = al.si_window;
  const int n_sf = pcf_n_sf(n_ofdm, n_symb);
  for (int f = 0; f < LCS_PDSCH_MAX_FORCED; ++f) {
    p->forced[f] = pc->forced[f];
    if (f >= pc->n_forced) continue;
    const lcs_pdsch_grant &g = pc->forced[f];
    if (g.subframe < 0 || g.subframe >= n_sf) return wide_refused(c, who, "a forced grant lies outside the grid's subframes");
    if (g.rb_start < 0 || g.n_prb < 1 || g.rb_start > n_rb - g.n_prb) return wide_refused(c, who, "a forced grant lies outside the grid's resource blocks");
    if (g.rnti < 1 || g.rnti > 65535) return wide_refused(c, who, "a forced grant's rnti is outside 1 .. 65535");
    if (g.rv < 0 || g.rv > 3) return wide_refused(c, who, "a forced grant's rv is outside 0 .. 3");
    if (g.tbs < 1 || g.tbs > PDS_MAX_K - 24) return wide_refused(c, who, "a forced grant's tbs is outside 1 .. 2216");
    int same = 0;
    for (int u = 0; u < f; ++u) same += pc->forced[u].subframe == g.subframe;
    if (same >= PDS_GRANTS) return wide_refused(c, who, "more than two forced grants in one subframe");
  }
  return LCS_OK;
}
// the combining's configuration (null: defaults)
int pdsch_comb_resolve(lcs_ctx *c, const char *who, const lcs_pdsch_comb_cfg *cc, PdschCombPlan *p) {
  static const lcs_pdsch_comb_cfg zero = {};
  if (!cc) cc = &zero;
  if (cc->si_window < 0 || cc->si_window > 61) return wide_refused(c, who, "si_window is outside 0 .. 61");
  if (cc->no_sib1 < 0 || cc->no_sib1 > 1) return wide_refused(c, who, "no_sib1 is outside 0 .. 1");
  p->si_window = cc->si_window; p->no_sib1 = cc->no_sib1;
  return LCS_OK;
}
// the four entry points: with comb_out the redundancy versions are combined behind the decode
int pdsch_call(lcs_ctx *c, const char *who, const WideSource &src, const lcs_cell *cell, int n_rb, int n_ofdm, int dl_mask, const lcs_pdcch_cfg *cfg,
               const lcs_pdsch_cfg *pdsch_cfg, lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out, const lcs_pdsch_comb_cfg *comb_cfg, lcs_pdsch_comb_info *comb_out) {
  WideCall w;
  PdcchPlan plan;
  PdschPlan ps;
  PdschCombPlan cp = {0, 0};
  int rc;
  if ((rc = wide_begin(c, who, src, cell, out, n_rb, n_ofdm, &dl_mask, true, &w)) || (rc = pdcch_resolve(c, who, cell, n_rb, cfg, &plan))) return rc;
  if ((rc = pdsch_resolve(c, who, plan, pdsch_cfg, n_ofdm, w.n_symb, n_rb, &ps))) return rc;
  if (comb_out && (rc = pdsch_comb_resolve(c, who, comb_cfg, &cp))) return rc;
  int sfrow[PCF_MAX_SF];
  pdsch_need(w.n_symb, n_ofdm, n_rb, dl_mask, plan.sh, w.need);
  w.plan(n_ofdm, 4, pdc_n_ctrl_max(n_rb));
  pdsch_sfrow(w.n_symb, w.n_sf, w.need, w.first, sfrow);
  if ((rc = wide_fill_grid(c, who, src, w, n_rb, n_ofdm))) return rc;
  if ((rc = lcs_launch_pdsch(c, *cell, w.rows, sfrow, w.n_sf, n_rb, dl_mask, plan, ps, comb_out ? &cp : nullptr))) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c->pdsch.rec, sizeof(lcs_pdsch_info), hipMemcpyDeviceToHost, c->stream));
  if (comb_out) HIPCHK(c, hipMemcpyAsync(comb_out, c->pdsch.crec, sizeof(lcs_pdsch_comb_info), hipMemcpyDeviceToHost, c->stream));
  if (pdcch_out) HIPCHK(c, hipMemcpyAsync(pdcch_out, c->pdsch.pdc.rec, sizeof(lcs_pdcch_info), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}
}  // namespace

int lcs_pdsch_wide(lcs_ctx *c, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog,
                   int n_fft, int n_rb, int n_ofdm, int dl_mask, const lcs_pdcch_cfg *cfg, const lcs_pdsch_cfg *pdsch_cfg, lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out) {
  if (!c) return LCS_ERR_BAD_ARG;
  return pdsch_call(c, "lcs_pdsch_wide", wide_samples(d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft), cell, n_rb, n_ofdm, dl_mask, cfg, pdsch_cfg, out, pdcch_out, nullptr, nullptr);
}
int lcs_pdsch_comb_wide(lcs_ctx *c, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap, double fc_req, double fc_prog, double fs_prog,
                        int n_fft, int n_rb, int n_ofdm, int dl_mask, const lcs_pdcch_cfg *cfg, const lcs_pdsch_cfg *pdsch_cfg, lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out,
                        const lcs_pdsch_comb_cfg *comb_cfg, lcs_pdsch_comb_info *comb_out) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (!comb_out) return wide_refused(c, "lcs_pdsch_comb_wide", "a null pointer");
  return pdsch_call(c, "lcs_pdsch_comb_wide", wide_samples(d_capbuf, n_cap, fc_req, fc_prog, fs_prog, n_fft), cell, n_rb, n_ofdm, dl_mask, cfg, pdsch_cfg, out, pdcch_out,
                    comb_cfg, comb_out);
}
int lcs_pdsch(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int n_rb, int dl_mask, const lcs_pdcch_cfg *cfg, const lcs_pdsch_cfg *pdsch_cfg,
              lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out) {
  if (!c) return LCS_ERR_BAD_ARG;
  return pdsch_call(c, "lcs_pdsch", wide_host_grid(tfg), cell, n_rb, n_ofdm, dl_mask, cfg, pdsch_cfg, out, pdcch_out, nullptr, nullptr);
}
int lcs_pdsch_comb(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int n_rb, int dl_mask, const lcs_pdcch_cfg *cfg, const lcs_pdsch_cfg *pdsch_cfg,
                   lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out, const lcs_pdsch_comb_cfg *comb_cfg, lcs_pdsch_comb_info *comb_out) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (!comb_out) return wide_refused(c, "lcs_pdsch_comb", "a null pointer");
  return pdsch_call(c, "lcs_pdsch_comb", wide_host_grid(tfg), cell, n_rb, n_ofdm, dl_mask, cfg, pdsch_cfg, out, pdcch_out, comb_cfg, comb_out);
}


int lcs_pdsch_last_soft(lcs_ctx *c, int subframe, int which, double *llr_out, int n) {
  if (!c) return LCS_ERR_BAD_ARG;
  static const char who[] = "lcs_pdsch_last_soft";
  if (!llr_out) return wide_refused(c, who, "a null pointer");
  const lcs_ctx::Pdsch &p = c->pdsch;
  if (subframe < 0 || subframe >= p.last_n_sf || which < 0 || which >= PDS_GRANTS || n < 0 || (size_t)n > p.last_stride)
    return wide_refused(c, who, "no such grant slot of the last call, or more soft bits than a slot holds");
  HIPCHK(c, hipSetDevice(c->device));
  // the slot's job as the plan left it: only a grant that was followed has soft bits of this call, G of them
  PdsJob job;
  HIPCHK(c, hipMemcpyAsync(&job, reinterpret_cast<const PdsJob *>(p.job.get()) + (PDS_GRANTS * subframe + which), sizeof(job), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (job.status != LCS_PDSCH_FOLLOW || n > job.G) return wide_refused(c, who, "that grant slot was not followed in the last call, or holds fewer soft bits");
  HIPCHK(c, hipMemcpyAsync(llr_out, p.llr.get() + (size_t)(PDS_GRANTS * subframe + which) * p.last_stride, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

int lcs_set_pdsch_alloc(lcs_ctx *c, const lcs_pdsch_alloc_cfg *cfg) {
  if (!c) return LCS_ERR_BAD_ARG;
  static const char who[] = "lcs_set_pdsch_alloc";
  static const lcs_pdsch_alloc_cfg zero = {0, 0, 0, 0};
  if (!cfg) cfg = &zero;
  if (cfg->flags < 0 || cfg->flags > 3) return wide_refused(c, who, "flags is outside 0 .. 3");
  if (cfg->sfn0 < -1 || cfg->sfn0 > 1023) return wide_refused(c, who, "sfn0 is outside -1 .. 1023");
  if (cfg->si_window < 0 || cfg->si_window > 61) return wide_refused(c, who, "si_window is outside 0 .. 61");
  if (cfg->reserved != 0) return wide_refused(c, who, "a non-zero reserved field");
  c->pdsch.alloc = *cfg;
  return LCS_OK;
}

int lcs_pdsch_last_alloc(lcs_ctx *c, int block_index, lcs_pdsch_alloc *out) {
  if (!c) return LCS_ERR_BAD_ARG;
  static const char who[] = "lcs_pdsch_last_alloc";
  if (!out) return wide_refused(c, who, "a null pointer");
  const lcs_ctx::Pdsch &p = c->pdsch;
  if (block_index < 0 || block_index >= LCS_PDSCH_MAX_BLOCKS || p.last_n_sf <= 0) return wide_refused(c, who, "no such block of the last call");
  HIPCHK(c, hipSetDevice(c->device));
  // the grant slots as the plan left them: block i of the record is the i-th slot that holds a grant (k_pdsch_fin).  A diagnostic
  // query, not a hot path: every call copies the whole job array and one block back and waits for the stream twice
  std::vector<PdsJob> jobs((size_t)PDS_GRANTS * p.last_n_sf);
  HIPCHK(c, hipMemcpyAsync(jobs.data(), p.job.get(), sizeof(PdsJob) * jobs.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int slot = -1, n = 0;
  for (size_t i = 0; i < jobs.size() && slot < 0; ++i)
    if (jobs[i].status != 0 && n++ == block_index) slot = (int)i;
  if (slot < 0) return wide_refused(c, who, "no such block of the last call");
  lcs_pdsch_block b;
  HIPCHK(c, hipMemcpyAsync(&b, p.blk.get() + slot, sizeof(b), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  pds_alloc_of(p.last_n_rb, b, jobs[(size_t)slot].reserved, out);
  return LCS_OK;
}

int lcs_turbo_decode(lcs_ctx *c, const double *d, int K, int F, int max_iter, uint8_t *bits_out, int *n_iter_out, int *crc_ok_out) {
  if (!c) return LCS_ERR_BAD_ARG;
  static const char who[] = "lcs_turbo_decode";
  if (!d || !bits_out || !n_iter_out || !crc_ok_out) return wide_refused(c, who, "a null pointer");
  if (pds_k_index(K) < 0) return wide_refused(c, who, "K is not one of the 127 turbo block sizes up to 2240");
  if (F < 0 || F >= K) return wide_refused(c, who, "F is outside 0 .. K - 1");
  if (max_iter < 0 || max_iter > 16) return wide_refused(c, who, "max_iter is outside 1 .. 16 (0: 8)");
  int rc, res[2];
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = lcs_launch_turbo(c, d, K, F, max_iter ? max_iter : 8))) return rc;
  HIPCHK(c, hipMemcpyAsync(res, c->pdsch.res, sizeof(res), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(bits_out, c->pdsch.hard, (size_t)K, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (res[1] != LCS_PDSCH_OK && res[1] != LCS_PDSCH_CRC) std::memset(bits_out, 0, (size_t)K);
  *n_iter_out = res[0];
  *crc_ok_out = res[1] == LCS_PDSCH_OK;
  return LCS_OK;
}

// chan_est of decode_mib as a stage of its own (ref src/searcher.cpp:1369-1477, ce_interp_hex :1223-1362): the channel
// estimate of one antenna port on the whole grid and its noise power -- an internal function of the reference, exported
// so that the tests can pin it to the oracle directly rather than through the decoded MIB.
int lcs_chan_est(lcs_ctx *c, const lcs_cell *cell, const double *tfg, int n_ofdm, int port, double *ce_tfg, double *np_out) {
  if (!c || !cell || !tfg || !ce_tfg || !np_out) return LCS_ERR_BAD_ARG;
  const int need = n_ofdm_for(cell);
  if (need < 0 || n_ofdm != need || cell->n_id_1 < 0 || cell->n_id_2 < 0 || port < 0 || port > 3) {
    c->err = "chan_est needs a detected cell, its full 854/732-symbol grid and a port 0..3";
    return LCS_ERR_BAD_ARG;
  }
  int rc;
  Launch L;
  if ((rc = stage_grid(c, cell, tfg, n_ofdm, &lcs_ctx::tfg_comp, &L))) return rc;
  if ((rc = lcs_launch_chan_est(c, L))) return rc;
  int first, per_port, n_rs_at;
  lcs_chan_est_np_layout(&first, &per_port, &n_rs_at);
  std::vector<double> sc(LCS_CELL_SCRATCH);
  HIPCHK(c, hipMemcpyAsync(ce_tfg, c->ce + (size_t)port * LCS_TFG_ROWS * LCS_TFG_NSC, sizeof(double2) * n_ofdm * LCS_TFG_NSC, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(sc.data(), c->cell_scratch, sizeof(double) * LCS_CELL_SCRATCH, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double s = 0;
  for (int q = 0; q < per_port; ++q) s += sc[first + port * per_port + q];      // chunk partials, in chunk order (tfg_mib.hip np_from_partials)
  *np_out = s / (sc[n_rs_at + port] * 12);
  return LCS_OK;
}

// One host buffer through the whole chain (ref src/CellSearch.cpp:484-558).
int lcs_search_capbuf(lcs_ctx *c, const double *capbuf, uint32_t n_cap, const double *f_search_set, uint16_t n_f,
                      double fc_req, double fc_prog, double fs_prog, lcs_cell *cells, int max_cells, int *n_cells,
                      lcs_cell *peaks, int max_peaks, int *n_peaks) {
  int rc = check_common(c, n_cap, n_f);
  if (rc) return rc;
  if (!capbuf || !f_search_set || !n_cells || (max_cells > 0 && !cells)) { c->err = "null argument"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_percell(c))) return rc;      // before the Launch is built: it takes the cells per round from the per-cell buffers' capacity
  Launch L;
  if ((rc = upload_host_capbuf(c, capbuf, n_cap, f_search_set, n_f, 2, fc_req, fc_prog, fs_prog, false, &L))) return rc;
  L.repair = FrqRepair::peaks_only;      // no array leaves this call: the peak list is what has to be exact
  L.needed_rows_only = true;
  if ((rc = lcs_launch_xcorr(c, L, false, false))) return rc;
  if ((rc = lcs_launch_peak_search(c, L, kPeakThresh, true))) return rc;
  if ((rc = launch_per_peak(c, L, 0, 1))) return rc;
  return read_cells_and_peaks(c, cells, nullptr, max_cells, n_cells, peaks, max_peaks, n_peaks);
}

// ------------------------------------------------------------------- successive cancellation (sic.hip; the rule: sic.h)
static int sic_check(lcs_ctx *c, int fmt, int n_buf, uint32_t n_cap, int mask) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (mask <= 0 || (mask & ~LCS_SIC_ALL)) { c->err = "lcs_sic: mask selects no component (LCS_SIC_PSS | _SSS | _CRS | _PBCH)"; return LCS_ERR_BAD_ARG; }
  if (fmt != LCS_FMT_C64 && fmt != LCS_FMT_IQ_U8) { c->err = "lcs_sic: captures are LCS_FMT_C64 or LCS_FMT_IQ_U8"; return LCS_ERR_BAD_ARG; }
  if (n_buf < 1 || n_cap < 9600 || n_cap > 268800) { c->err = "lcs_sic: n_buf >= 1, 9600 <= n_cap <= 268800 (the per-cell PBCH table holds 16 frames)"; return LCS_ERR_BAD_ARG; }
  return LCS_OK;
}

int lcs_sic_cancel_cfg_dev(lcs_ctx *c, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap, const lcs_cell *cells, const int *n_cells_per_buf,
                           int max_cells_per_buf, const int32_t *ul_dl_config, const double *fc_requested, const double *fc_programmed,
                           double fs_programmed, int mask, void *d_residual_c64, lcs_sic_info *info) {
  int rc = sic_check(c, fmt, n_buf, n_cap, mask);
  if (rc) return rc;
  if (!d_capbufs || !cells || !n_cells_per_buf || !fc_requested || !fc_programmed || !d_residual_c64 || max_cells_per_buf < 1) { c->err = "null argument"; return LCS_ERR_BAD_ARG; }
  for (int b = 0; b < n_buf; ++b)
    if (n_cells_per_buf[b] < 0 || n_cells_per_buf[b] > max_cells_per_buf) { c->err = "lcs_sic_cancel_dev: n_cells_per_buf beyond max_cells_per_buf"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  return lcs_launch_sic(c, d_capbufs, fmt, n_buf, n_cap, cells, n_cells_per_buf, max_cells_per_buf, fc_requested, fc_programmed, fs_programmed,
                        mask, c->duplex, nullptr, ul_dl_config, static_cast<float2 *>(d_residual_c64), info);
}

int lcs_sic_cancel_dev(lcs_ctx *c, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap, const lcs_cell *cells, const int *n_cells_per_buf,
                       int max_cells_per_buf, const double *fc_requested, const double *fc_programmed, double fs_programmed, int mask,
                       void *d_residual_c64, lcs_sic_info *info) {
  return lcs_sic_cancel_cfg_dev(c, d_capbufs, fmt, n_buf, n_cap, cells, n_cells_per_buf, max_cells_per_buf, nullptr, fc_requested, fc_programmed,
                                fs_programmed, mask, d_residual_c64, info);
}

// The side tables of the fused call that has just returned (n buffers), as lcs_last_tdd_info / lcs_last_cell_meas lay them out; a mode
// that is off leaves its sentinel everywhere.
static int sic_read_side(lcs_ctx *c, int n, int max_cells, std::vector<lcs_tdd_info> *tdd, std::vector<lcs_meas_info> *meas) {
  lcs_tdd_info t0{}; t0.ul_dl_config = t0.dwpts_rs_rows = LCS_TDD_NOT_ESTIMATED;
  lcs_meas_info m0{}; meas_clear(&m0, LCS_MEAS_NOT_MEASURED);
  tdd->assign((size_t)n * max_cells, t0);
  meas->assign((size_t)n * max_cells, m0);
  int rc;
  if (c->tdd_config && c->duplex == LCS_DUPLEX_TDD && (rc = lcs_last_tdd_info(c, tdd->data(), max_cells)) && rc != LCS_ERR_OVERFLOW) return rc;
  if (c->cell_meas && (rc = lcs_last_cell_meas(c, meas->data(), max_cells)) && rc != LCS_ERR_OVERFLOW) return rc;
  return LCS_OK;
}

// Rounds 1 .. max_rounds - 1 behind a round 0 whose records the caller holds in cells / n_cells.
static int sic_rounds(lcs_ctx *c, const void *d_cap, int fmt, int n_buf, uint32_t n_cap, const double *f_search_set, uint16_t n_f,
                      const double *fc_req, const double *fc_prog, double fs_prog, lcs_cell *cells, int max_cells, int *n_cells, int max_rounds,
                      int mask, int32_t *round_of_cell, lcs_sic_info *info) {
  int *st = c->sic.stats;
  st[0] = 1; st[1] = st[2] = st[3] = 0;
  int overflow = LCS_OK;
  if (round_of_cell) std::fill(round_of_cell, round_of_cell + (size_t)n_buf * max_cells, 0);
  lcs_sic_info none{};
  none.ul_dl_config = LCS_TDD_NOT_ESTIMATED;
  if (info) std::fill(info, info + (size_t)n_buf * max_cells, none);
  std::vector<int> held(n_buf), active;
  for (int b = 0; b < n_buf; ++b) { held[b] = std::min(n_cells[b], max_cells); if (held[b] > 0) active.push_back(b); }
  // round 0's side tables belong to the caller's buffers as they are; later rounds' records are put in their cells' places
  std::vector<lcs_tdd_info> &all_tdd = c->sic.h_tdd;
  std::vector<lcs_meas_info> &all_meas = c->sic.h_meas;
  c->sic.h_n_buf = n_buf; c->sic.h_max_cells = max_cells;
  int rc0 = sic_read_side(c, n_buf, max_cells, &all_tdd, &all_meas);
  if (rc0) return rc0;
  for (int round = 1; round < max_rounds && !active.empty(); ++round) {
    const int na = (int)active.size();
    std::vector<lcs_cell> known((size_t)na * max_cells), found((size_t)na * max_cells);
    std::vector<lcs_sic_info> inf((size_t)na * max_cells);
    std::vector<int> nk(na), nf(na);
    std::vector<int32_t> cfg((size_t)na * max_cells, LCS_TDD_NOT_ESTIMATED);
    std::vector<lcs_tdd_info> r_tdd;
    std::vector<lcs_meas_info> r_meas;
    std::vector<double> fr(na), fp(na);
    for (int a = 0; a < na; ++a) {
      const int b = active[a];
      nk[a] = held[b]; fr[a] = fc_req[b]; fp[a] = fc_prog[b];
      std::copy(cells + (size_t)b * max_cells, cells + (size_t)b * max_cells + held[b], known.begin() + (size_t)a * max_cells);
      for (int i = 0; i < held[b]; ++i) cfg[(size_t)a * max_cells + i] = all_tdd[(size_t)b * max_cells + i].ul_dl_config;
    }
    int rc = c->sic.res.reserve(c, (size_t)na * n_cap);
    if (rc) return rc;
    if ((rc = lcs_launch_sic(c, d_cap, fmt, na, n_cap, known.data(), nk.data(), max_cells, fr.data(), fp.data(), fs_prog, mask, c->duplex,
                             active.data(), cfg.data(), c->sic.res, inf.data())))
      return rc;
    ++st[1];
    rc = lcs_search_batch_dev(c, c->sic.res, LCS_FMT_C64, na, n_cap, f_search_set, n_f, fr.data(), fp.data(), fs_prog, LCS_STAGE_FULL, found.data(),
                              max_cells, nf.data());
    if (rc && rc != LCS_ERR_OVERFLOW) return rc;
    ++st[0];
    if ((rc = sic_read_side(c, na, max_cells, &r_tdd, &r_meas))) return rc;
    std::vector<int> next;
    for (int a = 0; a < na; ++a) {
      const int b = active[a];
      lcs_cell *mine = cells + (size_t)b * max_cells;
      // the n_dup counts live in the caller's array across rounds; everything else of the record is this round's
      for (int i = 0; i < held[b] && info; ++i) { const int32_t dup = info[(size_t)b * max_cells + i].n_dup; info[(size_t)b * max_cells + i] = inf[(size_t)a * max_cells + i]; info[(size_t)b * max_cells + i].n_dup = dup; }
      int added = 0;
      const int before = held[b];
      for (int i = 0; i < std::min(nf[a], max_cells); ++i) {
        const lcs_cell &f = found[(size_t)a * max_cells + i];
        int listed = -1;
        for (int k = 0; k < held[b]; ++k)
          if (mine[k].n_id_1 == f.n_id_1 && mine[k].n_id_2 == f.n_id_2) listed = k;
        if (listed >= 0) { ++st[3]; if (info) ++info[(size_t)b * max_cells + listed].n_dup; continue; }
        if (held[b] >= max_cells) { overflow = LCS_ERR_OVERFLOW; continue; }
        if (round_of_cell) round_of_cell[(size_t)b * max_cells + held[b]] = round;
        all_tdd[(size_t)b * max_cells + held[b]] = r_tdd[(size_t)a * max_cells + i];
        all_meas[(size_t)b * max_cells + held[b]] = r_meas[(size_t)a * max_cells + i];
        mine[held[b]++] = f;
        ++added; ++st[2];
      }
      n_cells[b] = std::max(n_cells[b], before) + added;
      if (added) next.push_back(b);
    }
    active.swap(next);
  }
  if (overflow) c->err = "more results than the output array holds";
  return overflow;
}

int lcs_search_capbuf_sic(lcs_ctx *c, const double *capbuf, uint32_t n_cap, const double *f_search_set, uint16_t n_f, double fc_req,
                          double fc_prog, double fs_prog, lcs_cell *cells, int max_cells, int *n_cells, lcs_cell *peaks, int max_peaks,
                          int *n_peaks, int max_rounds, int mask, int32_t *round_of_cell, lcs_sic_info *info) {
  int rc = sic_check(c, LCS_FMT_C64, 1, n_cap, mask);
  if (rc) return rc;
  if (max_rounds < 1 || max_rounds > LCS_SIC_MAX_ROUNDS || max_cells < 1) { c->err = "lcs_search_capbuf_sic: max_rounds 1 .. 4, max_cells >= 1"; return LCS_ERR_BAD_ARG; }
  rc = lcs_search_capbuf(c, capbuf, n_cap, f_search_set, n_f, fc_req, fc_prog, fs_prog, cells, max_cells, n_cells, peaks, max_peaks, n_peaks);
  if (rc) return rc;
  if (max_rounds > 1 && *n_cells > 0) {      // the capture as complex<float> (exact for dongle data) for the cancellation to read
    std::vector<float2> h(n_cap);
    for (uint32_t i = 0; i < n_cap; ++i) h[i] = make_float2((float)capbuf[2 * i], (float)capbuf[2 * i + 1]);
    if ((rc = c->sic.cap.reserve(c, n_cap))) return rc;
    HIPCHK(c, hipMemcpy(c->sic.cap.get(), h.data(), (size_t)n_cap * sizeof(float2), hipMemcpyHostToDevice));
  }
  return sic_rounds(c, c->sic.cap, LCS_FMT_C64, 1, n_cap, f_search_set, n_f, &fc_req, &fc_prog, fs_prog, cells, max_cells, n_cells, max_rounds, mask,
                    round_of_cell, info);
}

int lcs_search_batch_sic_dev(lcs_ctx *c, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap, const double *f_search_set, uint16_t n_f,
                             const double *fc_requested, const double *fc_programmed, double fs_programmed, lcs_cell *cells,
                             int max_cells_per_buf, int *n_cells, int max_rounds, int mask, int32_t *round_of_cell, lcs_sic_info *info) {
  int rc = sic_check(c, fmt, n_buf, n_cap, mask);
  if (rc) return rc;
  if (max_rounds < 1 || max_rounds > LCS_SIC_MAX_ROUNDS || max_cells_per_buf < 1) { c->err = "lcs_search_batch_sic_dev: max_rounds 1 .. 4, max_cells_per_buf >= 1"; return LCS_ERR_BAD_ARG; }
  rc = lcs_search_batch_dev(c, d_capbufs, fmt, n_buf, n_cap, f_search_set, n_f, fc_requested, fc_programmed, fs_programmed, LCS_STAGE_FULL, cells,
                            max_cells_per_buf, n_cells);
  if (rc) return rc;
  return sic_rounds(c, d_capbufs, fmt, n_buf, n_cap, f_search_set, n_f, fc_requested, fc_programmed, fs_programmed, cells, max_cells_per_buf, n_cells,
                    max_rounds, mask, round_of_cell, info);
}

int lcs_last_sic_stats(lcs_ctx *c, int stats[4]) {
  if (!c || !stats) return LCS_ERR_BAD_ARG;
  for (int i = 0; i < 4; ++i) stats[i] = c->sic.stats[i];
  return LCS_OK;
}

int lcs_last_sic_tdd_info(lcs_ctx *c, lcs_tdd_info *info, int max_cells_per_buf) {
  if (!c || !info) return LCS_ERR_BAD_ARG;
  if (max_cells_per_buf != c->sic.h_max_cells || c->sic.h_n_buf < 1) { c->err = "lcs_last_sic_tdd_info: no lcs_search_*_sic call with this max_cells_per_buf"; return LCS_ERR_BAD_ARG; }
  std::copy(c->sic.h_tdd.begin(), c->sic.h_tdd.end(), info);
  return LCS_OK;
}
int lcs_last_sic_cell_meas(lcs_ctx *c, lcs_meas_info *info, int max_cells_per_buf) {
  if (!c || !info) return LCS_ERR_BAD_ARG;
  if (max_cells_per_buf != c->sic.h_max_cells || c->sic.h_n_buf < 1) { c->err = "lcs_last_sic_cell_meas: no lcs_search_*_sic call with this max_cells_per_buf"; return LCS_ERR_BAD_ARG; }
  std::copy(c->sic.h_meas.begin(), c->sic.h_meas.end(), info);
  return LCS_OK;
}

int lcs_table_pbch_symbols(int n_id_cell, int n_ports, int n_rb_dl, int phich_duration, int phich_resource, int sfn, int cp_type, double *out) {
  if (!out || sfn < 0 || sfn > 1023) return LCS_ERR_BAD_ARG;
  return lcs_tables::pbch_encode(n_id_cell, n_ports, n_rb_dl, phich_duration, phich_resource, sfn, cp_type, out) ? LCS_OK : LCS_ERR_BAD_ARG;
}

// ------------------------------------------------------------------- one buffer, hypotheses split over GPUs
// SURVEY 8e "latency mode": every rank correlates its contiguous share of f_search_set; the shares meet where the
// reference takes the maximum over the frequency axis (src/searcher.cpp:369-382).  RCCL has no arg-max: the collapsed
// power (a non-negative float: ordered like its bit pattern) and the complemented GLOBAL hypothesis index are packed
// into one 64-bit word, (bits(pow) << 32) | (0xFFFFFFFF - foi), and an ordinary MAX all-reduce then reproduces the
// reference's first-maximum rule (strict >: the lowest index wins a tie, :374).  The words never leave the GPUs:
// lcs_foe_partial leaves them in a device buffer of the caller (a torch tensor handed to torch.distributed), the caller
// all-reduces in place, lcs_foe_finish reads them back in, runs peak_search (identical on every rank) and the per-peak
// stages, and reports the cells whose winning hypothesis this rank owns (it alone holds the xc_incoherent_single slice
// the refinement of `ind` reads, :457-465).
int lcs_foe_partial(lcs_ctx *c, const double *capbuf, uint32_t n_cap, const double *f_search_set, uint16_t n_f, int f_first, int f_count,
                    double fc_req, double fc_prog, double fs_prog, void *d_words, double *d_meta) {
  int rc = check_common(c, n_cap, n_f);
  if (rc) return rc;
  if (!capbuf || !f_search_set || !d_words || !d_meta || f_first < 0 || f_count < 0 || f_first + f_count > n_f) { c->err = "bad argument"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  c->foe_ready = false;
  // a rank without hypotheses still takes part: it correlates one (the first) so that its buffer, tables and power
  // estimate exist, and contributes words that never win
  const int cnt = std::max(1, f_count), first = f_count ? f_first : 0;
  if ((rc = ensure_ws(c, 1, n_cap, n_f, false))) return rc;      // lcs_foe_finish puts the WHOLE grid into fset_ws (this rank correlates its share only)
  if ((rc = ensure_percell(c))) return rc;      // before the Launch is built, as in lcs_search_capbuf; lcs_foe_finish keeps this call's cells per round
  Launch L;
  if ((rc = upload_host_capbuf(c, capbuf, n_cap, f_search_set + first, cnt, 2, fc_req, fc_prog, fs_prog, false, &L))) return rc;
  // no tie repair here: a near-tie may span two ranks' shares -- lcs_foe_contend settles them after the all-reduce, identically
  // for every split; the collapse keeps the runner-up values for it
  L.repair = FrqRepair::none_keep_2nd;
  L.needed_rows_only = true;
  if ((rc = lcs_launch_xcorr(c, L, false, false))) return rc;
  L.geo.foi0 = f_count ? f_first : -1;            // -1: owns nothing
  if ((rc = lcs_launch_foe_pack(c, L, static_cast<long long *>(d_words), d_meta))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));    // the caller's collective runs on another stream
  c->foe = L;
  c->foe_ready = true;
  return LCS_OK;
}

// Exactness of the split (round 5).  The packed MAX decides between float values that the kernels reproduce to ~1e-7: where two
// hypotheses -- of one rank or of two -- lie closer than LCS_FRQ_TIE_EPS, the winner has to be decided in the reference's own
// arithmetic (k_frq_repair).  After the all-reduce of d_words every rank knows the global maximum of every position; it CONTENDS
// for a position when a hypothesis of its own other than the winner lies within the distance of that maximum, recomputes its
// contenders AND the global winner exactly (it holds the whole buffer and the whole grid), and writes the packed exact first
// maximum into d_words2 (-1 elsewhere).  The caller MAX-all-reduces d_words2 -- the exact first maximum over every contender of
// every rank, identical whatever the split -- and lcs_foe_resolve puts those words in place of the approximate ones.
int lcs_foe_contend(lcs_ctx *c, const double *f_search_set, uint16_t n_f, const void *d_words, void *d_words2) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (!c->foe_ready) { c->err = "lcs_foe_contend needs the lcs_foe_partial call of the same buffer first"; return LCS_ERR_BAD_ARG; }
  if (!f_search_set || !d_words || !d_words2 || n_f < 1 || n_f > LCS_NF_LIMIT) { c->err = "bad argument"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (n_f > c->fset_g.capacity()) HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = c->fset_g.reserve(c, (size_t)n_f))) return rc;      // the whole grid (fset_ws holds this rank's share)
  HIPCHK(c, hipMemcpyAsync(c->fset_g, f_search_set, sizeof(double) * n_f, hipMemcpyHostToDevice, c->stream));
  if ((rc = lcs_launch_foe_contend(c, c->foe, c->fset_g, static_cast<const long long *>(d_words), static_cast<long long *>(d_words2)))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the caller's collective runs on another stream (and f_search_set may go away)
  return LCS_OK;
}

int lcs_foe_resolve(lcs_ctx *c, void *d_words, const void *d_words2) {
  if (!c || !d_words || !d_words2) return LCS_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = lcs_launch_foe_resolve(c, static_cast<long long *>(d_words), static_cast<const long long *>(d_words2)))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

int lcs_foe_finish(lcs_ctx *c, const void *d_words, const double *d_meta, const double *f_search_set, uint16_t n_f, lcs_cell *cells,
                   int32_t *order, int max_cells, int *n_cells, lcs_cell *peaks, int max_peaks, int *n_peaks) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (!c->foe_ready) { c->err = "lcs_foe_finish needs the lcs_foe_partial call of the same buffer first"; return LCS_ERR_BAD_ARG; }
  if (!d_words || !d_meta || !f_search_set || !n_cells || (max_cells > 0 && (!cells || !order)) || n_f < 1 || n_f > LCS_NF_LIMIT) { c->err = "bad argument"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  c->foe_ready = false;
  const Launch &L = c->foe;
  int rc;
  // peak_search names the winning hypothesis by its GLOBAL index: the whole grid now, not this rank's share
  HIPCHK(c, hipMemcpyAsync(c->fset_ws, f_search_set, sizeof(double) * n_f, hipMemcpyHostToDevice, c->stream));
  if ((rc = lcs_launch_foe_unpack(c, L, static_cast<const long long *>(d_words), d_meta))) return rc;
  if ((rc = lcs_launch_peak_search(c, L, kPeakThresh, true))) return rc;
  if ((rc = launch_per_peak(c, L, 0, 1))) return rc;
  return read_cells_and_peaks(c, cells, order, max_cells, n_cells, peaks, max_peaks, n_peaks);
}

// ---------------------------------------------------------------------------- streaming mode
// LTE-Tracker's searcher thread (ref src/searcher_thread.cpp:83-246) runs the whole chain on every
// 80 ms capture buffer with a single frequency hypothesis (the tracked frequency offset, :97-98) and
// skips cells that are already tracked (:157-177).  Per buffer that is ~25 small launches: here the
// chain is captured ONCE as a hipGraph and replayed per push.  Everything that changes between
// pushes (samples, frequency offset, tracked identities) travels through fixed pinned host buffers
// that the graph's copy nodes read at execution time.
namespace {
// xc_route for the stream: the sets its open allocates, the kernel its chain runs
extern "C++" XcRoute stream_route(const lcs_ctx *c, int fmt, const XcGeom &geo) { return xc_route(route_facts(c, XcCaller::stream, fmt == LCS_FMT_IQ_U8, geo.n_comb)); }
// the chain as slot k sees it: its own pinned input buffer and parameter / result block, the shared device workspace.  Its kernels
// take the slot parameters and the hypothesis from the stream's device mirror (one copy per push), not from the workspace arrays the
// other entry points fill.
int stream_chain(lcs_ctx *c, int k) {
  StreamHost *h = c->st_host[k];
  int rc;
  c->foe_ready = false;
  HIPCHK(c, hipMemcpyAsync(c->st_din, c->st_hin[k], c->st_in_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->st_dmirror, h, LCS_STREAM_IN_BYTES, hipMemcpyHostToDevice, c->stream));      // parameters, tracked list, hypothesis: one copy
  CapSrc src;
  if ((rc = lcs_launch_ingest(c, c->st_din, c->st_fmt, 1, c->st_n_cap, &src))) return rc;
  Launch L = make_launch(c, 1, c->st_n_cap, src);
  L.geo = make_geo(c->st_n_cap, 1, 2);      // one hypothesis: no window-start spread, every kernel's image holds it
  L.params = reinterpret_cast<const SlotParams *>(c->st_dmirror + offsetof(StreamHost, p));
  L.fset = reinterpret_cast<const double *>(c->st_dmirror + offsetof(StreamHost, f));
  L.xc = stream_route(c, c->st_fmt, L.geo).kernel;
  L.needed_rows_only = true;
  if ((rc = lcs_launch_xcorr(c, L, false, false))) return rc;
  if ((rc = lcs_launch_peak_search(c, L, kPeakThresh, true))) return rc;
  if ((rc = launch_per_peak(c, L, 0, 1))) return rc;
  HIPCHK(c, hipMemcpyAsync(h->res, c->peaks, sizeof(h->res), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&h->n_peaks, c->npeaks, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h->n_work, c->n_work, sizeof(h->n_work), hipMemcpyDeviceToHost, c->stream));
  return LCS_OK;
}
}  // namespace

int lcs_stream_close(lcs_ctx *c) {
  if (!c) return LCS_ERR_BAD_ARG;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (int k = 0; k < 2; ++k) {
    if (c->st_exec[k]) (void)hipGraphExecDestroy(c->st_exec[k]);
    if (c->st_graph[k]) (void)hipGraphDestroy(c->st_graph[k]);
    c->st_hin[k].reset();
    c->st_host[k].reset();
    if (c->st_ev0[k]) (void)hipEventDestroy(c->st_ev0[k]);
    if (c->st_ev1[k]) (void)hipEventDestroy(c->st_ev1[k]);
    c->st_exec[k] = nullptr; c->st_graph[k] = nullptr; c->st_ev0[k] = c->st_ev1[k] = nullptr;
  }
  c->st_din.reset();
  c->st_dmirror.reset();
  c->st_dtracked = nullptr; c->st_dntracked = nullptr;
  // the saved launches of a batch or an lcs_foe_partial made while the stream was open borrowed its tracked list: what is left of
  // them (late rounds of lcs_batch_collect, lcs_foe_finish) runs without a filter, as every launch on a context without a stream
  c->batch.l.tracked = c->foe.tracked = nullptr;
  c->batch.l.n_tracked = c->foe.n_tracked = nullptr;
  c->st_open = false;
  c->st_head = c->st_count = 0;
  return LCS_OK;
}

// Two slots: the chain is captured twice, once per pinned input buffer + parameter / result block, so that the host may
// fill and launch buffer i + 1 while the graph of buffer i is still running (the launches themselves serialise on the
// context's stream and share the device workspace).
namespace {
int stream_open(lcs_ctx *c, int fmt, uint32_t n_cap, double fc_requested, double fc_programmed, double fs_programmed) {
  int rc;
  if ((rc = ensure_ws(c, 1, n_cap, 1, false))) return rc;
  if ((rc = ensure_percell(c))) return rc;
  if ((rc = lcs_ensure_xc(c, stream_route(c, fmt, make_geo(n_cap, 1, 2)).sets))) return rc;
  c->st_fmt = fmt;
  c->st_n_cap = n_cap;
  c->st_in_bytes = (size_t)n_cap * (fmt == LCS_FMT_IQ_U8 ? 2 : sizeof(float2));
  if ((rc = c->st_din.alloc(c, c->st_in_bytes)) || (rc = c->st_dmirror.alloc(c, LCS_STREAM_IN_BYTES))) return rc;
  c->st_dntracked = reinterpret_cast<int *>(c->st_dmirror + offsetof(StreamHost, n_tracked));
  c->st_dtracked = reinterpret_cast<int16_t *>(c->st_dmirror + offsetof(StreamHost, tracked));
  for (int k = 0; k < 2; ++k) {
    if ((rc = c->st_hin[k].alloc(c, c->st_in_bytes)) || (rc = c->st_host[k].alloc(c, 1))) return rc;
    HIPCHK(c, hipEventCreate(&c->st_ev0[k]));
    HIPCHK(c, hipEventCreate(&c->st_ev1[k]));
    std::memset(c->st_hin[k], fmt == LCS_FMT_IQ_U8 ? 127 : 0, c->st_in_bytes);
    std::memset(c->st_host[k], 0, sizeof(StreamHost));
    c->st_host[k].get()->p = SlotParams{fc_requested, fc_programmed, fs_programmed};
  }
  c->st_open = true;
  c->st_head = c->st_count = 0;
  // one eager pass (lazy allocations, function attributes), then the same call sequence under capture, per slot
  if ((rc = stream_chain(c, 0))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 2; ++k) {
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    rc = stream_chain(c, k);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (rc || e != hipSuccess || !g) {
      if (!rc) { c->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e); rc = LCS_ERR_HIP; }
      return rc;
    }
    c->st_graph[k] = g;
    HIPCHK(c, hipGraphInstantiate(&c->st_exec[k], c->st_graph[k], nullptr, nullptr, 0));
  }
  return LCS_OK;
}
}  // namespace

int lcs_stream_open(lcs_ctx *c, int fmt, uint32_t n_cap, double fc_requested, double fc_programmed, double fs_programmed) {
  int rc = check_common(c, n_cap, 1);
  if (rc) return rc;
  if (fmt != LCS_FMT_C64 && fmt != LCS_FMT_IQ_U8) { c->err = "unknown capture format"; return LCS_ERR_BAD_ARG; }
  if (c->tdd_config) {
    c->err = "the streaming mode does not carry the uplink-downlink estimate: lcs_set_tdd_config(ctx, 0) first";
    return LCS_ERR_BAD_ARG;
  }
  if (c->cell_meas) {
    c->err = "the streaming mode does not carry the cell measurement: lcs_set_cell_meas(ctx, 0) first";
    return LCS_ERR_BAD_ARG;
  }
  if (c->st_open) lcs_stream_close(c);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = stream_open(c, fmt, n_cap, fc_requested, fc_programmed, fs_programmed))) lcs_stream_close(c);      // whatever a failed open got hold of goes again
  return rc;
}

int lcs_stream_push(lcs_ctx *c, const void *samples, double f_off, const int16_t *tracked_ids, int n_tracked) {
  if (!c || !c->st_open || !samples) { if (c) c->err = "stream not open"; return LCS_ERR_BAD_ARG; }
  if (c->st_count >= 2) { c->err = "two buffers are in flight already: lcs_stream_collect first"; return LCS_ERR_BAD_ARG; }
  if (n_tracked < 0 || n_tracked > 504 || (n_tracked > 0 && !tracked_ids)) { c->err = "bad tracked list"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  c->foe_ready = false;      // the graph overwrites slot 0
  const int k = (c->st_head + c->st_count) & 1;
  std::memcpy(c->st_hin[k], samples, c->st_in_bytes);
  StreamHost *h = c->st_host[k];
  h->f = f_off;
  h->n_tracked = n_tracked;
  for (int i = 0; i < n_tracked; ++i) h->tracked[i] = tracked_ids[i];
  HIPCHK(c, hipEventRecord(c->st_ev0[k], c->stream));
  HIPCHK(c, hipGraphLaunch(c->st_exec[k], c->stream));
  HIPCHK(c, hipEventRecord(c->st_ev1[k], c->stream));
  ++c->st_count;
  return LCS_OK;
}

// Results of the OLDEST buffer in flight.
int lcs_stream_collect(lcs_ctx *c, lcs_cell *cells, int max_cells, int *n_cells, int *n_redetected, float *gpu_ms) {
  if (!c || !c->st_open || c->st_count < 1 || !n_cells || (max_cells > 0 && !cells)) { if (c) c->err = "nothing to collect"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  const int k = c->st_head;
  HIPCHK(c, hipEventSynchronize(c->st_ev1[k]));
  c->st_head ^= 1;
  --c->st_count;
  if (gpu_ms) HIPCHK(c, hipEventElapsedTime(gpu_ms, c->st_ev0[k], c->st_ev1[k]));
  const StreamHost *h = c->st_host[k];
  int rc = LCS_OK, n = 0;
  const int np = std::min(h->n_peaks, (int)LCS_MAXP);
  if (h->n_peaks > LCS_MAXP || h->n_work[1] > std::min(c->max_work, c->percell_cap)) rc = LCS_ERR_OVERFLOW;
  // The reference appends a decoded cell to the tracked list AT ONCE (ref src/searcher_thread.cpp:233-236), so a later peak of the
  // same buffer that sss_detect gives the same identity -- a second path of a fading channel, a sidelobe -- meets "already being
  // tracked" (:157-177) before anything else is done with it.  The chain here decodes every peak in parallel; in peak order the
  // first decoded record of an identity is the one the reference keeps, the later peaks of that identity count as seen again.
  int seen[LCS_MAXP], n_seen = 0, again = 0;
  for (int i = 0; i < np; ++i) {
    const lcs_cell &pc = h->res[i];
    if (pc.n_id_1 == -1) continue;                          // no SSS
    const int id = pc.n_id_2 + 3 * pc.n_id_1;
    bool known = false;
    for (int q = 0; q < n_seen; ++q) known = known || seen[q] == id;
    if (known) { ++again; continue; }
    if (pc.n_rb_dl == -1) continue;                         // no MIB / tracked before this buffer (never decoded: counted on the device)
    if (n < max_cells) cells[n] = pc; else rc = LCS_ERR_OVERFLOW;
    ++n;
    seen[n_seen++] = id;
  }
  *n_cells = n;
  if (n_redetected) *n_redetected = h->n_work[2] + again;
  if (rc) c->err = "more results than the output array holds";
  return rc;
}

int lcs_last_xcorr_ms(lcs_ctx *c, float *ms, int *n_launches) {
  if (!c || !ms) return LCS_ERR_BAD_ARG;
  HIPCHK(c, hipEventSynchronize(c->ev_xc1));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev_xc0, c->ev_xc1));
  if (n_launches) *n_launches = c->last_xc_launches;
  return LCS_OK;
}

int lcs_last_frq_repairs(lcs_ctx *c, int *n_positions) {
  if (!c || !n_positions || !c->n_fix) return LCS_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = lcs_launch_xcorr_complete(c, c->batch.l)) return rc;
  HIPCHK(c, hipMemcpyAsync(n_positions, c->n_fix, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LCS_OK;
}

double lcs_frq_tie_eps(void) { return (double)LCS_FRQ_TIE_EPS; }

int lcs_last_frq_repair_stats(lcs_ctx *c, int *n_listed, int *n_unrepaired) {
  if (!c || !n_listed || !n_unrepaired || !c->n_fix) return LCS_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int v[2] = {0, 0};
  if (int rc = lcs_launch_xcorr_complete(c, c->batch.l)) return rc;
  HIPCHK(c, hipMemcpyAsync(v, c->n_fix, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_listed = v[0];
  *n_unrepaired = v[1];
  return LCS_OK;
}

int lcs_last_xcorr_info(lcs_ctx *c, double *executed_ops, const char **kernel) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (executed_ops) *executed_ops = c->last_xc_ops;
  if (kernel) *kernel = c->last_xc_kernel;
  return LCS_OK;
}

// ----------------------------------------------------------------------- channelizer
int lcs_channelizer_taps(int decim, double *taps) {
  if (decim < 2 || decim > 16 || !taps) return LCS_ERR_BAD_ARG;
  lcs_chan_taps(decim, taps);
  return LCS_OK;
}

// The entry points fill one ChanCall and refuse by chan_refusal (channelizer.h); lcs_channelize_u8 refuses what the call it
// extends refuses, then looks at d_gain.
static int chan_refused(lcs_ctx *c, const char *entry, const char *what) {
  c->err = std::string(entry) + ": " + what;
  return LCS_ERR_BAD_ARG;
}

int lcs_channelize(lcs_ctx *c, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int decim, const double *f_shift, int n_ch,
                   void *d_out, uint32_t n_out) {
  if (!c) return LCS_ERR_BAD_ARG;
  const ChanCall a = {d_wide, fmt, n_in, fs_in, 1, decim, f_shift, n_ch, d_out, n_out};
  if (const char *what = chan_refusal(a, CHAN_DECIM)) return chan_refused(c, "lcs_channelize", what);
  HIPCHK(c, hipSetDevice(c->device));
  return lcs_launch_channelize(c, a, nullptr);
}

int lcs_channelizer_proto(int down, double *taps) {
  if (down < 2 || down > 128 || !taps) return LCS_ERR_BAD_ARG;
  lcs_chan_taps(down, taps);
  return LCS_OK;
}

int lcs_channelize_rational(lcs_ctx *c, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int up, int down, const double *f_shift,
                            int n_ch, void *d_out, uint32_t n_out) {
  if (!c) return LCS_ERR_BAD_ARG;
  const ChanCall a = {d_wide, fmt, n_in, fs_in, up, down, f_shift, n_ch, d_out, n_out};
  if (const char *what = chan_refusal(a, CHAN_RATE_ONLY)) return chan_refused(c, "lcs_channelize_rational", what);
  if (up == 1) return lcs_channelize(c, d_wide, fmt, n_in, fs_in, down, f_shift, n_ch, d_out, n_out);      // the integer path, bit for bit
  if (const char *what = chan_refusal(a, CHAN_RATE)) return chan_refused(c, "lcs_channelize_rational", what);
  HIPCHK(c, hipSetDevice(c->device));
  return lcs_launch_channelize(c, a, nullptr);
}

int lcs_channelize_u8(lcs_ctx *c, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int up, int down, const double *f_shift, int n_ch,
                      void *d_out, uint32_t n_out, float *d_gain) {
  if (!c) return LCS_ERR_BAD_ARG;
  const ChanCall a = {d_wide, fmt, n_in, fs_in, up, down, f_shift, n_ch, d_out, n_out};
  const char *what = chan_refusal(a, CHAN_RATE);
  if (!what && (reinterpret_cast<uintptr_t>(d_gain) & 3)) what = "d_gain is not aligned to a float";
  if (what) return chan_refused(c, "lcs_channelize_u8", what);
  HIPCHK(c, hipSetDevice(c->device));
  return lcs_launch_channelize_u8(c, a, d_gain);
}

// The continuous form.  open refuses what the one-shot forms refuse of a rate, a format, the shifts and n_ch -- chan_refusal on a
// call whose capture and outputs break no rule -- and everything else by chan_stream_refusal; a refused call launches nothing and
// leaves the stream where it was.
int lcs_chan_stream_open(lcs_ctx *c, int fmt, double fs_in, int up, int down, const double *f_shift, int n_ch) {
  if (!c) return LCS_ERR_BAD_ARG;
  alignas(16) static char any[16];      // stands for d_wide and d_out: never null, never misaligned, never read
  const ChanCall a = {any, fmt, ~0ull, fs_in, up, down, f_shift, n_ch, any, 1};
  const char *what = chan_refusal(a, CHAN_RATE);
  if (!what) what = chan_stream_refusal(ChanPush{c->chan_stream.open}, CHAN_STREAM_OPEN);
  if (what) return chan_refused(c, "lcs_chan_stream_open", what);
  HIPCHK(c, hipSetDevice(c->device));
  return lcs_chan_stream_start(c, fmt, fs_in, up, down, f_shift, n_ch);
}

static uint64_t chan_stream_emit(const lcs_ctx *c, uint64_t n_chunk, uint64_t *m_first) {
  const lcs_ctx::ChanStream &st = c->chan_stream;
  const unsigned long long m0 = cs_count(st.n_total, st.up, st.down);
  if (m_first) *m_first = m0;
  return cs_count(st.n_total + n_chunk, st.up, st.down) - m0;
}

int lcs_chan_stream_count(lcs_ctx *c, uint64_t n_chunk, uint32_t *n_emit) {
  if (!c || !n_emit) return LCS_ERR_BAD_ARG;
  ChanPush a = {c->chan_stream.open};
  a.n_chunk = n_chunk;
  if (const char *what = chan_stream_refusal(a, CHAN_STREAM_COUNT)) return chan_refused(c, "lcs_chan_stream_count", what);
  *n_emit = (uint32_t)chan_stream_emit(c, n_chunk, nullptr);      // < n_chunk <= 2^31
  return LCS_OK;
}

int lcs_chan_stream_push(lcs_ctx *c, const void *d_chunk, uint64_t n_chunk, void *d_out, uint32_t row_stride, uint32_t out_cap, uint32_t *n_emit,
                         uint64_t *m_first) {
  if (!c) return LCS_ERR_BAD_ARG;
  const bool open = c->chan_stream.open;
  uint64_t m0 = 0;
  ChanPush a = {open, c->chan_stream.fmt, d_chunk, n_chunk, d_out, row_stride, out_cap, 0, c->chan_stream.u8};
  if (open && n_chunk <= (1ull << 31)) a.n_emit = chan_stream_emit(c, n_chunk, &m0);
  if (const char *what = chan_stream_refusal(a, CHAN_STREAM_PUSH)) return chan_refused(c, "lcs_chan_stream_push", what);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = lcs_chan_stream_enqueue(c, d_chunk, n_chunk, d_out, row_stride)) return rc;
  if (n_emit) *n_emit = (uint32_t)a.n_emit;
  if (m_first) *m_first = m0;
  return LCS_OK;
}

// The stream of 8-bit captures: open_u8 refuses what open refuses and then by chan_stream_u8_refusal, as count_u8 and push_u8 do.
int lcs_chan_stream_open_u8(lcs_ctx *c, int fmt, double fs_in, int up, int down, const double *f_shift, int n_ch, uint32_t n_cap) {
  if (!c) return LCS_ERR_BAD_ARG;
  alignas(16) static char any[16];
  const ChanCall a = {any, fmt, ~0ull, fs_in, up, down, f_shift, n_ch, any, 1};
  const char *what = chan_refusal(a, CHAN_RATE);
  ChanPushU8 u = {c->chan_stream.open};
  u.n_cap = n_cap;
  if (!what) what = chan_stream_u8_refusal(u, CHAN_STREAM_OPEN);
  if (what) return chan_refused(c, "lcs_chan_stream_open_u8", what);
  HIPCHK(c, hipSetDevice(c->device));
  return lcs_chan_stream_start_u8(c, fmt, fs_in, up, down, f_shift, n_ch, n_cap);
}

// a push as chan_stream_u8_refusal sees it; n_done only where the rules in front of it let it be computed
static ChanPushU8 chan_stream_u8_call(const lcs_ctx *c, const void *d_chunk, uint64_t n_chunk, void *d_out, const float *d_gain, uint32_t cap_room) {
  const lcs_ctx::ChanStream &st = c->chan_stream;
  ChanPushU8 a = {st.open, st.u8, st.fmt, d_chunk, n_chunk, d_out, d_gain, cap_room, st.n_cap, 0};
  if (st.open && st.u8 && n_chunk <= (1ull << 31)) a.n_done = cs_cap_done(st.n_total, n_chunk, st.n_cap, st.up, st.down);
  return a;
}

int lcs_chan_stream_count_u8(lcs_ctx *c, uint64_t n_chunk, uint32_t *n_done) {
  if (!c || !n_done) return LCS_ERR_BAD_ARG;
  const ChanPushU8 a = chan_stream_u8_call(c, nullptr, n_chunk, nullptr, nullptr, 0);
  if (const char *what = chan_stream_u8_refusal(a, CHAN_STREAM_COUNT)) return chan_refused(c, "lcs_chan_stream_count_u8", what);
  *n_done = (uint32_t)a.n_done;      // <= outputs < n_chunk <= 2^31
  return LCS_OK;
}

int lcs_chan_stream_push_u8(lcs_ctx *c, const void *d_chunk, uint64_t n_chunk, void *d_out, float *d_gain, uint32_t cap_room, uint32_t *n_done,
                            uint64_t *cap_first) {
  if (!c) return LCS_ERR_BAD_ARG;
  const ChanPushU8 a = chan_stream_u8_call(c, d_chunk, n_chunk, d_out, d_gain, cap_room);
  if (const char *what = chan_stream_u8_refusal(a, CHAN_STREAM_PUSH)) return chan_refused(c, "lcs_chan_stream_push_u8", what);
  const lcs_ctx::ChanStream &st = c->chan_stream;
  const uint64_t first = cs_cap_count(st.n_total, st.n_cap, st.up, st.down);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = lcs_chan_stream_enqueue_u8(c, d_chunk, n_chunk, d_out, d_gain)) return rc;
  if (n_done) *n_done = (uint32_t)a.n_done;
  if (cap_first) *cap_first = first;
  return LCS_OK;
}

int lcs_chan_stream_close(lcs_ctx *c) {
  if (!c) return LCS_ERR_BAD_ARG;
  if (const char *what = chan_stream_refusal(ChanPush{c->chan_stream.open}, CHAN_STREAM_CLOSE)) return chan_refused(c, "lcs_chan_stream_close", what);
  HIPCHK(c, hipSetDevice(c->device));
  return lcs_chan_stream_end(c);
}

int lcs_last_channelize_ms(lcs_ctx *c, float *ms) {
  if (!c || !ms) return LCS_ERR_BAD_ARG;
  return lcs_chan_last_ms(c, ms);
}

// ---------------------------------------------------------------------------- tables
int lcs_table_pss_td(int n_id_2, double *out) { if (n_id_2 < 0 || n_id_2 > 2 || !out) return LCS_ERR_BAD_ARG; lcs_tables::pss_td(n_id_2, out); return LCS_OK; }
int lcs_table_pss_fd(int n_id_2, double *out) { if (n_id_2 < 0 || n_id_2 > 2 || !out) return LCS_ERR_BAD_ARG; lcs_tables::pss_fd(n_id_2, out); return LCS_OK; }
int lcs_table_sss_fd(int n_id_1, int n_id_2, int slot_num, int32_t *out) {
  if (n_id_1 < 0 || n_id_1 > 167 || n_id_2 < 0 || n_id_2 > 2 || !out) return LCS_ERR_BAD_ARG;
  lcs_tables::sss_fd(n_id_1, n_id_2, slot_num, out);
  return LCS_OK;
}
int lcs_table_lte_pn(uint32_t c_init, uint32_t len, uint8_t *out) { if (!out) return LCS_ERR_BAD_ARG; lcs_tables::lte_pn(c_init, len, out); return LCS_OK; }
double lcs_chi2cdf_inv(double p, double k) { return lcs_tables::chi2cdf_inv(p, k); }

}  // extern "C"
