// lcs_internal.h -- shared declarations of the MI355X-native searcher (not installed).
//
// Device data layout (everything lives in one workspace, slot-major; a "slot" is one
// capture buffer in flight):
//   cap32   [S][n_cap]            float2   capture buffer, fp32 (PSS correlation input)
//   cap64   [1][n_cap]            double2  fp64 copy, only when a host entry point hands over complex<double>
//   tmpl    [S][n_f][3][137]      float2   conj(fshift(pss_td))/137   (searcher.cpp:146-151)
//   start   [S][NW][n_f]          int      window starts (pss_ref.h: lcs_win_start)
//   smin/kp2[S][NW][G]            int      per (window, 16-template group): first lag offset, tap pairs
//   btab    [S][NW][G][KP2][64]   float    MFMA B operands: delay-shifted templates (fp32 kernel)
//   brow8   [S][G][LCS_I8_IMG]    uint32   int8 kernel: three-digit operand rows of a group, as they sit in LDS
//   single  [S][G][9600][16]      float    xc_incoherent_single, group-major (16 templates = one 64 B row)
//   sref    [3][9600][n_f]        float    reference-layout staging of single for the stage entry points
//   pow/frq [S][3][9600]          double/int
//   spinc/zth [S][9600]           double
//   peaks   [S][MAXP] lcs_cell, npeaks [S]
// The tracker's buffers (lcs_ctx::trk) are not in this workspace: trk_layout.h holds the one table of their arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstddef>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/lcs.h"
#include "lcs_mem.h"
#include "trk_layout.h"
#include "xcorr_route.h"   // XcKernel, and what a template group holds: LCS_KP2_MAX, LCS_KP2_UNROLL, LCS_I8_OFF, LCS_I8_MAX_TAPS

#define FS_LTE 30720000.0    // LTE sampling rate at 2048 subcarriers; the searcher works at FS_LTE / 16
#define LCS_NW_MAX 16        // incoherent-combining windows (15 for a 153600-sample buffer)
// Frequency hypotheses per call: the reference loops over whatever f_search_set holds (src/searcher.cpp:113-174; CellSearch builds
// n_f = 2 floor((fc ppm / 1e6 + 2500) / 5000) + 1, src/CellSearch.cpp:463-465: 125 at 2.6 GHz, 289 at 6 GHz for the default 120 ppm).
// Every table is sized per call (lcs_api.hip: ensure_ws) and laid out with the call's own strides; this is a sanity bound only
// (+-2.56 MHz of search span, ~120 MB of xc_incoherent_single per buffer).
#define LCS_NF_LIMIT 1024
// Every kernel other than the PSS correlation is small and latency-bound; in the pipelined chain it
// shares CUs with the next batch's correlation waves.  Raising the wave priority lets the SIMD
// arbiter issue these few waves ahead of the MFMA stream instead of round-robin behind 4-5 of them.
#define LCS_TAIL_PRIO() __builtin_amdgcn_s_setprio(3)
#define LCS_TG 16            // templates per MFMA column group
#define LCS_LAG_TILE 64      // lags per wave
#define LCS_PS 336           // LDS plane stride in floats: >= 64 + 2*KP2_MAX, == 16 (mod 32)
#define LCS_MAXP LCS_MAX_PEAKS   // peaks kept per capture buffer: the most peak_search can return (lcs.h)
// xc_incoherent_collapsed_frq: positions whose two best hypotheses lie within this (relative) of each other are recomputed in the
// reference's arithmetic (k_frq_repair, pss_xcorr.hip).  Two values further apart than this keep their order as long as every
// element of xc_incoherent_single is within HALF of it (relative) of the reference's: the suite asserts that on every array it
// compares (worst measured 1.8e-6: the int8 kernel on a two-window buffer).  lcs_frq_tie_eps() hands it out.
#define LCS_FRQ_TIE_EPS 4e-6f
#define LCS_I8_KB 5          // 32-tap blocks of the int8 correlation kernel
#define LCS_I8_IMG 17024     // dwords of the int8 kernel's operand image per (buffer, group) (pss_xcorr_i8.hip)
#define LCS_I8_LAGS 512      // lags per workgroup (lag tile) of the int8 kernel, and its tiles per buffer: what the batch screen flags
#define LCS_I8_TILES ((LCS_N_IDX + LCS_I8_LAGS - 1) / LCS_I8_LAGS)
#define LCS_SCREEN_SKIP 63   // batches that go unscreened after one that flagged more than 1 / LCS_SCREEN_DENSE of its tiles
#define LCS_SCREEN_DENSE 5
#define LCS_F16_IMG 11840    // the same for the fp16 kernel (pss_xcorr_f16.hip)
#define LCS_MAX_WORK 1024    // most cells carried into the TFG/MIB stages per round (~6 MB each)
#define LCS_WORK_DEFAULT 512 // cells per round a context starts with (3 GB, allocated on first use); it doubles by itself when a batch carries more
// grid sizes of the work-list kernels (every one loops over its list, so these only trade latency for workgroups)
#define LCS_WIN_GRID 4096
#define LCS_ITEM_GRID 1024
#define LCS_TFG_GRID 4096
#define LCS_TFA_GRID 2048
#define LCS_TFG_ROWS 854
#define LCS_TFG_DESC_BYTES (856 * 32 + 128 * 16)   // tfg_mib.hip: TfgRow records + the frequency correction's position factors
#define LCS_CELL_SCRATCH 4608 // doubles of per-cell scratch (RS table, shifts, noise powers, PBCH candidates)

struct SlotParams {
  double fc_req, fc_prog, fs_prog;
};

struct XcGeom {
  uint32_t n_cap;
  int n_f;
  int n_tmpl;   // 3*n_f
  int cpg;      // template columns in use per 16-column group: 16 = dense packing, 15/12/9/6/3 = whole hypotheses per group
  int G;        // ceil(n_tmpl / cpg)
  int n_comb;   // n_comb_xc
  int ds;       // ds_comb_arm
  int foi0;     // hypothesis split over GPUs (lcs_foe_*): global index of this rank's first hypothesis; frq then holds GLOBAL indices
  int n_narrow; // windows 0 .. n_narrow - 1: the window starts of every template group (of every buffer of the call) lie within
                // LCS_NARROW_SPREAD samples of each other, so 137 taps + delay fit 144.  When that holds for every window of a call
                // (every grid the CLI builds) the fp16 kernel runs nine 16-tap blocks per window instead of ten (pss_xcorr_f16.hip);
                // the int8 kernel's half-depth last block was built and measured: no gain (profiles/r04/experiments)
};
#define LCS_NARROW_SPREAD 7

// int8 copies of a u8 capture buffer: slot stride in samples (a multiple of 8, so that every slot starts 16-byte
// aligned) with LCS_I8_PAD zero samples behind the data -- the correlation kernel's LDS-DMA reads run past n_cap
#define LCS_I8_PAD 1024
__host__ __device__ static inline size_t lcs_cap8_stride(uint32_t n_cap) { return (((size_t)n_cap + 7) & ~(size_t)7) + LCS_I8_PAD; }

// Template (foi * 3 + pss) held by column j of group g, or -1.  With the dense packing (cpg 16) consecutive templates fill
// the columns and a hypothesis may straddle two groups; a frequency grid too sparse for that (the window starts of the
// hypotheses in one group drift apart by more samples than the correlation kernels' tap blocks hold) is packed with
// fewer, whole hypotheses per group -- down to one (cpg 3), whose three templates share one window start.
__host__ __device__ static inline int lcs_col_tmpl(const XcGeom &geo, int g, int j) {
  const int c = g * geo.cpg + j;
  return (j < geo.cpg && c < geo.n_tmpl) ? c : -1;
}

// The capture buffers as the fp64 stages see them (exactly one pointer is set): the fp64 copy when a host entry
// point handed over complex<double>; the int8 pairs 127 - u8 of an RTL-SDR source ((u8-127)/128 = -a/128, exact);
// otherwise the fp32 copy widened on the fly (exact for float input).
struct CapSrc {
  const float2 *c32;
  const double2 *c64;
  const uint16_t *c8;
  uint32_t n_cap;
};
struct CapView {
  const float2 *c32;
  const double2 *c64;
  const uint16_t *c8;
};
// The kernels that read the capture buffers are templates over the kind of source (0: int8 pairs, 1: fp32, 2: fp64):
// lcs_by_cap_kind(src, [&](auto kind) { launch k<decltype(kind)::value> }) picks the instantiation for a CapSrc.
template <class F> inline void lcs_by_cap_kind(const CapSrc &s, F &&launch) {
  if (s.c8) launch(std::integral_constant<int, 0>{});
  else if (s.c32) launch(std::integral_constant<int, 1>{});
  else launch(std::integral_constant<int, 2>{});
}
#ifdef __HIPCC__
// Hand-over of LDS data between the lanes of ONE wave (the wave-local FFT stages): the wave barrier alone is IntrNoMem --
// no memory fence -- so the ordering of the LDS accesses around it is pinned by a release / acquire fence pair at
// wavefront scope (no instructions beyond the s_waitcnt the LDS reads need anyway).
__device__ __forceinline__ void lcs_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// What the kind of source decides, in one place: the raw sample type, where a slot starts, and the sample as the fp64 stages see it.
template <int KIND> struct CapKind;
template <> struct CapKind<0> {
  typedef uint16_t T;
  static __host__ __device__ __forceinline__ const T *slot(const CapSrc &s, int slot) { return s.c8 + (size_t)slot * lcs_cap8_stride(s.n_cap); }
  static __host__ __device__ __forceinline__ const T *of(const CapView &v) { return v.c8; }
  static __host__ __device__ __forceinline__ double2 cvt(T p) {      // (u8 - 127) / 128 of the int8 pair 127 - u8
    return make_double2(-(double)(int)(int8_t)(p & 255u) / 128.0, -(double)(int)(int8_t)(p >> 8) / 128.0);
  }
};
template <> struct CapKind<1> {
  typedef float2 T;
  static __host__ __device__ __forceinline__ const T *slot(const CapSrc &s, int slot) { return s.c32 + (size_t)slot * s.n_cap; }
  static __host__ __device__ __forceinline__ const T *of(const CapView &v) { return v.c32; }
  static __host__ __device__ __forceinline__ double2 cvt(T f) { return make_double2((double)f.x, (double)f.y); }
};
template <> struct CapKind<2> {
  typedef double2 T;
  static __host__ __device__ __forceinline__ const T *slot(const CapSrc &s, int slot) { return s.c64 + (size_t)slot * s.n_cap; }
  static __host__ __device__ __forceinline__ const T *of(const CapView &v) { return v.c64; }
  static __host__ __device__ __forceinline__ double2 cvt(T d) { return d; }
};
__device__ __forceinline__ CapView cap_view(const CapSrc &s, int slot) {
  CapView v;
  v.c32 = s.c32 ? CapKind<1>::slot(s, slot) : nullptr;
  v.c64 = s.c64 ? CapKind<2>::slot(s, slot) : nullptr;
  v.c8 = s.c8 ? CapKind<0>::slot(s, slot) : nullptr;
  return v;
}
__device__ __forceinline__ double2 cap_at(const CapView &v, size_t i) {
  if (v.c64) return CapKind<2>::cvt(v.c64[i]);
  if (v.c8) return CapKind<0>::cvt(v.c8[i]);
  return CapKind<1>::cvt(v.c32[i]);
}
#endif

// One "cell work item" for the per-cell stages (TFG / TFOEC / channel estimate / PBCH).
struct WorkItem {
  int slot;
  int peak;      // index into peaks[slot]
};

// Everything a launcher needs to know about the call it serves, apart from the context's memory: built by the entry point
// (lcs_api.hip: make_launch) and handed to every lcs_launch_* function.  No launcher reads a mode from lcs_ctx.
enum class FrqRepair {
  all,            // every near-tie of the arg-max is recomputed in the reference's arithmetic (the arrays leave the call)
  peaks_only,     // only the near-ties at or above their position's Z_th1: the peak list is what has to be exact (lcs_search_capbuf)
  none_keep_2nd   // no repair, the collapse keeps the runner-up: a rank sees only its share of the hypotheses (lcs_foe_partial)
};
struct Launch {
  int n_buf = 0;
  uint32_t n_cap = 0;
  XcGeom geo{};
  const SlotParams *params = nullptr;   // per-slot parameter records and the hypotheses: the workspace's arrays (params_ws / fset_ws),
  const double *fset = nullptr;         // or the device mirror of the streaming mode's pinned block
  XcKernel xc = XcKernel::fp32;         // xc_route's choice (xcorr_route.h)
  CapSrc src{};                         // what the fp64 stages read: decided where the data is ingested (lcs_launch_ingest*)
  FrqRepair repair = FrqRepair::all;
  bool screen = false;                  // xc_route's `screen`: the int8 kernel's two-digit pass, then three digits over the flagged tiles
  bool single_stream = false;           // everything on `stream`, no hand-over to stream_xc (a context with an open stream)
  bool needed_rows_only = false;        // fused chains: compute only the grid rows later stages read (tfg_mib.hip)
  int grid_items = 64;                  // workgroups per work-list axis of the per-cell kernels (they loop over the list)
  int round_cells = 0;                  // cells per per-cell round (k_gather_work's limit)
  int tfoec_parts = 4;                  // workgroups per cell for the timing estimate: 2 in batches
  const int16_t *tracked = nullptr;     // identities k_gather_work leaves out (the streaming mode's tracked list), null: no filter
  const int *n_tracked = nullptr;
  int duplex = LCS_DUPLEX_FDD;          // lcs_set_duplex: where the SSS lies relative to the PSS (sss_foe.hip: the Dx table)
  int foe_unwrap = 0;                   // lcs_set_foe_unwrap: pss_sss_foe unwrapped by the PSS-only coarse estimate (foe_coarse.h)
  int tdd_config = 0;                   // lcs_set_tdd_config AND duplex == LCS_DUPLEX_TDD: k_tdd_config behind k_mib_select (tdd_config.h)
  int cell_meas = 0;                    // lcs_set_cell_meas: k_cell_meas behind k_mib_select and k_tdd_config (cell_meas.h)
};
// The last enqueued batch: lcs_batch_collect (its late per-cell rounds), lcs_batch_readback and lcs_last_batch_stats read it.
struct BatchRecord {
  Launch l;                             // l.n_buf == 0: no batch yet, or its workspace has been replaced since (ensure_ws)
  int stage_mask = 0;
  int fmt = 0;                          // the format the caller handed over
  int cell_rounds = 0;                  // per-cell rounds launched so far (l.round_cells cells each)
  bool list_ops_counted = false;        // a screened batch: lcs_batch_collect has added the flagged tiles' launch to last_xc_ops
};

// Pinned block shared with the captured graph of the streaming mode.
// The first LCS_STREAM_IN_BYTES of it (parameters, tracked identities, the frequency hypothesis LAST) go to a device mirror of the same
// layout in ONE copy per push (rounds 2-5: four copy nodes per replay); the captured chain's kernels read their parameters and
// hypothesis from that mirror (stream_chain builds its Launch with `params` / `fset` pointing into it).
struct StreamHost {
  SlotParams p;
  int n_tracked;
  int pad_;
  int16_t tracked[504];
  double f;
  lcs_cell res[LCS_MAXP];
  int n_peaks;
  int n_work[4];
};

#define LCS_STREAM_IN_BYTES (offsetof(StreamHost, f) + sizeof(double))

// The continuous tracker's carried state (tracker.hip: lcs_track_stream_block)
struct TrkStreamCell {
  std::vector<double> fo, ft, late;          // metadata of the carried symbols
  double bpo_before_tail = 0;                // bulk phase before the first carried symbol
  long long tail_start = 0;                  // stream index of the first carried symbol (a frame boundary)
  long long n_seen = 0;                      // symbols delivered so far
  long long next_raw[4] = {1, 1, 1, 1};      // per port: reference-symbol row (counted from the stream start) whose filter is emitted next
  long long ce_upto[4] = {0, 0, 0, 0};       // per port: channel estimates emitted for symbols below this
  long long mib_next = 0;                    // first frame offset not attempted yet
  int cp_type = 0, n_id_1 = -1, n_id_2 = -1, n_ports = 0;
};
// The carried symbols themselves stay on the DEVICE, already transformed: per CP type the frequency-domain rows
// [cells of that type][carried symbols][72] of the previous call (round 3 kept the time-domain samples on the host and ran
// them through get_fd again with every call).
struct TrkStream {
  std::vector<TrkStreamCell> cells;
  // indexed by LCS_CP_NORMAL / LCS_CP_EXTENDED: the carried rows, and a second buffer the next call's tail is written into
  // before the two change places at the commit (no allocation or release -- a device-wide synchronisation -- per call)
  DevBuf<double2> d_tail[3], d_spare[3];
};
// The device buffers FIRST .. FIRST + N - 1 of trk_layout.h's table and the capacity they were allocated for
struct TrkCutCap { size_t n_cells = 0, n = 0; };   // the most cells, and the most cells x symbols, of any call
template <int FIRST, int N, class Cap> struct TrkPart {
  DevBuf<char> buf[N];
  Cap cap;
  template <class T> T *at(const TrkLay &l, int a) const { return l.at<T>(buf[TRK_ROWS[a].buf - FIRST].get(), a); }
  // Every buffer anew, as `l` sizes it for `want`, once the stream has drained (the body follows lcs_ctx).  The capacity describes a
  // complete set or nothing: if an allocation fails, later calls must not take the half-replaced buffers for the old shape.
  int regrow(lcs_ctx *c, const TrkLay &l, const Cap &want);
  int reserve(lcs_ctx *c, TrkShape s) { return trk_fits(cap, s) ? LCS_OK : regrow(c, trk_layout(trk_grow(cap, s)), trk_grow(cap, s)); }   // grow only
};

// Buffers of the int8 correlation path (u8 sources) and of the fp16 three-product path (complex<float> sources of the batch
// entry points): each set is sized like the workspace, exists as a whole or not at all (`ready`), and goes with the workspace
// it was sized for.  With the fp32 kernel's operand tables they are the XcBufs of a context: lcs_ensure_xc (pss_xcorr.hip) is the one
// place any of them is allocated, ensure_ws drops them all by assigning an empty XcBufs.
struct I8Set {
  DevBuf<uint16_t> cap8;             // capture buffers as (re, im) int8 pairs 127 - u8, slot stride lcs_cap8_stride (pss_xcorr_i8.hip)
  DevBuf<uint16_t> cap8s;            // the same shifted down by one sample: cap8s[i] = cap8[i + 1]
  DevBuf<uint32_t> brow8;            // int8 three-digit template operands: one image of resident rows per (slot, group)
  DevBuf<double> tq;                 // per template: integer scale q
  DevBuf<float> tsc;                 // per template: 1 / (128 q)
  // the batch screen (k_screen_flag): what the three-digit kernel redoes
  DevBuf<int> scr_state;             // [4]: work items, tiles flagged, buffers that flagged everything, last tiles among the flagged
  DevBuf<int> scr_tile;              // [S][LCS_I8_TILES]: 1 = the tile is flagged
  DevBuf<unsigned> scr_items;        // [S * LCS_I8_TILES * G]: the work items of k_xcorr_i8x3<3, true>
  DevBuf<float> scr_theta;            // [S]: the buffer's theta (screen_bound.h), rounded down: nothing below it is recordable (0: the buffer flagged everything, or nothing)
  bool ready = false;
};
struct F16Set {
  DevBuf<uint32_t> cap16h, cap16l;   // (re, im) fp16 pairs, hi and lo parts, slot stride lcs_cap8_stride
  DevBuf<uint32_t> brow16;           // template operands, hi and lo terms: one image of resident rows per (slot, group)
  DevBuf<int> texp16;                // per template column: power-of-two scale exponent
  DevBuf<float> tsc16;               // per template column: 2^-(k_x + k_t)
  DevBuf<unsigned> xmax16;           // per slot: bits of the largest |component|
  DevBuf<unsigned> xpart16;          // per slot: 128 partial maxima (one per workgroup of the read-only maximum pass)
  bool ready = false;
};
struct XcBufs {
  I8Set i8;
  F16Set f16;
  DevBuf<float> btab;                // fp32 kernel only: sized for the workspace's slots and groups (0.5 MB per slot, window and group)
};

// A table beside the peak table and laid out like it, [n_buf][LCS_MAXP], that a fused call fills when its mode is on (k_tdd_config's,
// k_cell_meas's): the block, whether the last fused call made it, and the 32-bit word a record that belongs to no decoded cell is
// made of.  The bodies follow lcs_ctx.
struct lcs_ctx;
template <class Rec> struct SideTable {
  explicit SideTable(int sentinel_word) : sentinel(sentinel_word) {}
  DevBuf<Rec> tab;
  bool made = false;       // whether the last fused call ran the kernel that fills it: otherwise it reads the sentinel throughout
  const int sentinel;
  Rec *get() const { return tab.get(); }
  // launch_per_peak's first round: `on`, the table of n_buf buffers exists and every word of it is the sentinel (it synchronises the
  // stream only when the block has to grow); later rounds -- lcs_batch_collect's among them -- fill in their own cells
  int begin(lcs_ctx *c, int n_buf, bool on);
  // The table of the last fused call (n_buf buffers) in the order of the records that call handed out -- the peaks with SSS and MIB
  // in peak order (k_pack_results, read_cells_and_peaks): out[b * max_cells_per_buf + k] belongs to cell k of buffer b, `none`
  // everywhere else and throughout when the table was not made.  A record whose field `key` reads the sentinel belongs to no cell.
  int read_last(lcs_ctx *c, int n_buf, const Rec &none, int32_t Rec::*key, Rec *out, int max_cells_per_buf);
};

// The streams and events of a context (the streaming mode's own events and graphs: lcs_stream_close).  A BASE of lcs_ctx,
// because a base is destroyed after every member of the struct derived from it: see the note on ownership at lcs_ctx.
struct lcs_ctx_queues {
  int device = 0;
  hipStream_t stream = nullptr;      // everything except the PSS correlation (highest priority)
  hipStream_t stream_xc = nullptr;   // the PSS correlation kernel (lowest priority), see lcs_launch_xcorr
  hipEvent_t ev_pre = nullptr, ev_post = nullptr;
  hipEvent_t ev_xc0 = nullptr, ev_xc1 = nullptr;
  hipEvent_t ev_stage[2] = {nullptr, nullptr};      // guard the pinned slots h_stage
  hipEvent_t ev_chan_slot[2] = {nullptr, nullptr};  // channelizer.hip: guard the page-locked parameter slots chan_hpin
  hipEvent_t ev_chan0 = nullptr, ev_chan1 = nullptr;
  ~lcs_ctx_queues();                 // lcs_api.hip: the events, then the streams
};

// Ownership.  Every block of device or page-locked memory of a context is a Buf member (lcs_mem.h) of this struct or of a struct
// that is one, and nothing else frees it; a plain pointer member is a VIEW of memory owned elsewhere and says so.  What a launch
// depends on beyond memory travels in a Launch, not in fields of this struct; the two records kept here (`batch`, `foe`) are saved
// copies of the Launch of a call whose work a later call continues, and a saved copy's pointers end with what they point into:
// ensure_ws drops both records when it replaces the workspace (and `xcb`, the correlation kernels' buffer sets, sized for it),
// lcs_stream_close takes the stream's tracked list out of them, lcs_batch_collect the caller's complex<float> buffers.  lcs_destroy
// is `delete`: ~lcs_ctx makes the context's device current, closes an open stream (graphs first) and synchronises both
// streams; then the members go, the owners freeing their memory; the base goes last, with the events and then the streams --
// the order the hand-written tear-down had.
struct lcs_ctx : lcs_ctx_queues {
  ~lcs_ctx();                        // lcs_api.hip
  std::string err;

  // capacity the workspace is currently sized for
  int cap_slots = 0;
  uint32_t cap_n_cap = 0;
  int cap_n_f = 0;
  int cap_G = 0;                     // template groups per buffer the tables are sized for
  bool cap_debug = false;

  // device buffers
  DevBuf<float2> cap32;
  XcBufs xcb;                        // what the correlation kernels read beyond the workspace: lcs_ensure_xc
  DevBuf<double2> cap64;             // slot 0 only: fp64 copy for the host (complex<double>) entry points
  DevBuf<SlotParams> params_ws;      // the workspace's parameter records and hypotheses (ensure_ws): what every entry point but the
  DevBuf<double> fset_ws;            // streaming chain uploads to and hands to its launches (Launch::params / fset)
  DevBuf<float2> tmpl;
  DevBuf<int> start, smin, kp2;
  DevBuf<float> single, incoh, sref;
  DevBuf<double> pow_, work, spinc, zth, sp;
  DevBuf<int> frq;
  DevBuf<unsigned> fix_list;         // [S][3][9600]: positions (slot * 3 + t) * 9600 + idx whose arg-max is a near-tie (capacity: every position)
  DevBuf<int> n_fix;                 // [4]: entries on the list (zeroed by k_prep_tables)
  DevBuf<float> second32;            // [S][3][9600]: the runner-up of the collapse's maximum (written for lcs_foe_partial only: lcs_foe_contend reads it)
  DevBuf<double> fset_g;             // the whole grid, for lcs_foe_contend (fset_ws holds the rank's share then)
  DevBuf<lcs_cell> peaks;
  DevBuf<int> npeaks;
  DevBuf<float2> xc;                // debug: raw correlations [3][n_cap-136][n_f]
  // SSS / FOE stage (sss_foe.hip): work list of (buffer, peak) pairs and per-(peak, occurrence) records
  DevBuf<WorkItem> pk_items;
  DevBuf<int> n_pk;
  DevBuf<double> sss_ws;
  // per-cell stage buffers
  DevBuf<WorkItem> work_items;
  DevBuf<int> n_work;
  DevBuf<double2> tfg;              // [MAX_WORK][854][72]
  DevBuf<double2> tfg_comp;         // [MAX_WORK][854][72]
  DevBuf<double2> ce;               // [MAX_WORK][4][854][72]
  DevBuf<char> tfg_desc;            // [MAX_WORK][LCS_TFG_DESC_BYTES]: per cell 856 window records in k_tfg's job order + 128 position factors (k_cell_prep)
  DevBuf<double> tfg_ts;            // [MAX_WORK][854]
  DevBuf<double> tfg_ts_comp;       // [MAX_WORK][854]
  DevBuf<double> cell_scratch;      // [MAX_WORK][CELL_SCRATCH]
  DevBuf<lcs_cell> cells_out;       // [MAX_WORK]
  // constant tables on the device
  DevBuf<double2> d_pss_td;         // [3][137]
  DevBuf<double2> d_pss_fd;         // [3][62]
  DevBuf<int8_t> d_sss_fd;          // [168][3][2][62]
  DevBuf<uint8_t> d_pbch_scr;       // [504][1920]
  DevBuf<uint32_t> d_pn_jump;       // [32]: Gold-sequence jump-ahead by 1600 + 208 clocks (lcs_tables::pn_jump_table)
  DevBuf<int16_t> d_derm_inv;       // [2][120][16]: for every coded bit (stream*40+col) the rate-matched PBCH bit positions carrying it (ascending, -1 padded)
  DevBuf<double> d_dbg;             // debug outputs of the single-cell stage entry points
  DevBuf<int> d_flag;               // exactness verdict of k_ingest_c128
  int duplex = LCS_DUPLEX_FDD;      // lcs_set_duplex: copied into every Launch by make_launch, read by nothing else
  int foe_unwrap = 0;               // lcs_set_foe_unwrap: likewise
  DevBuf<double> foe_coarse;        // [4]: what lcs_pss_foe_coarse reads back (k_foe_fin_unwrap)
  int tdd_config = 0;               // lcs_set_tdd_config: likewise (it reaches a Launch only in LCS_DUPLEX_TDD)
  int cell_meas = 0;                // lcs_set_cell_meas: likewise
  int fused_n_buf = 0;              // buffers of the last fused call (lcs_last_tdd_info, lcs_last_cell_meas), 0: none yet
  SideTable<lcs_tdd_info> tdd_info{LCS_TDD_NOT_ESTIMATED};        // what k_tdd_config writes in the fused chain
  SideTable<lcs_meas_info> cell_meas_tab{LCS_MEAS_NOT_MEASURED};  // what k_cell_meas writes in the fused chain
  // the full-bandwidth grid and measurement (tfg_wide.hip: lcs_extract_tfg_wide, lcs_cell_meas_wide): every block is allocated by
  // the first call that needs it and grown on demand; a context that never calls the stage holds none of them
  struct MeasWide {
    DevBuf<double2> tw[5];          // [n_fft / 2] per n_fft = 128 << i: the transform's twiddles W^t, built in double on the host by the first call at that length
    DevBuf<double2> grid;           // [rows][12 n_rb]: the rows of the last call
    DevBuf<double> ideal;           // [rows]: the ideal location of every requested row
    DevBuf<double> rowv;            // [MEAS_NV][TC_MAX_Q]: the seven values of every reference row
    DevBuf<double> binrb;           // [40][MEASW_NRB][100]: the per-RB values of every bin
    DevBuf<uint32_t> pn_jump;       // [32]: Gold-sequence jump-ahead to c(2 (110 - n_rb)) of the call's n_rb
    uint32_t h_pn_jump[32] = {};    // ... and the host block it is uploaded from (it outlives the launcher's frame)
    DevBuf<lcs_meas_wide_info> rec; // [1]
    // the PCFICH on the same grid (pcfich.hip: lcs_pcfich_wide, lcs_pcfich), allocated by the first call of that stage
    DevBuf<int> pcf_rows;           // [LCS_PCFICH_MAX_SF][2]: the grid rows of every subframe's symbols 0 and 1, -1: not read
    DevBuf<uint32_t> pcf_jump;      // [2][32]: jump-ahead to the call's reference sequence, and by 1600 clocks for the scrambling
    DevBuf<lcs_pcfich_info> pcf_rec;   // [1]
    int h_pcf_rows[2 * LCS_PCFICH_MAX_SF] = {};   // the host blocks those two are uploaded from
    uint32_t h_pcf_jump[64] = {};
    int pcf_jump_rb = 0;            // the n_rb pcf_jump holds the tables of, 0: none
  } meas_wide;
  // the PDCCH common search space on that grid (pdcch.hip: lcs_pdcch_wide, lcs_pdcch), allocated by the first call of that stage.
  // The tables are built on the host (pdcch.h) when the key changes, not per call.
  struct Pdcch {
    DevBuf<int> map;                // [3 m_i][3 cfi] PdcMap: n_reg, n_cce, re[576]
    DevBuf<int16_t> derm;           // [2 sizes][2 levels][192][8]: the de-rate-matching lists
    DevBuf<uint32_t> jump;          // [2][32]: jump-ahead to the call's reference sequence, and by 1600 clocks for the scrambling
    DevBuf<int> sf;                 // [n_sf][4] grid rows of every subframe's symbols 0 .. 3 (-1: not read), m_i[10], [n_sf][2] the PCFICH's rows
    DevBuf<double> llr;             // [LCS_PCFICH_MAX_SF][1152]
    DevBuf<lcs_pdcch_info> rec;     // [1]
    DevBuf<lcs_pcfich_info> pcf_rec;   // [1]: the PCFICH's decisions on the call's rows, a record of this stage's own
    std::vector<int> h_map;         // the host blocks they are uploaded from
    std::vector<int16_t> h_derm;
    uint32_t h_jump[64] = {};
    int h_sf[6 * LCS_PCFICH_MAX_SF + 10] = {};
    int key[9] = {};                // n_rb, ports, cp_type, id, phich_duration, phich_resource, n_sizes, size[2] of the tables; n_rb 0: none
    int jump_rb = 0;
  } pdcch;
  // the blind search of every CCE on that grid (pdcch_scan.hip: lcs_pdcch_scan_wide, lcs_pdcch_scan), allocated by the first call of
  // that stage.  The tables are built on the host (pdcch_scan.h) when the key changes, not per call.
  struct PdcchScan {
    DevBuf<int> map;                // [3 m_i][3 cfi] PscMap: n_reg, n_cce, re[3168]
    DevBuf<int16_t> derm;           // [6 sizes][4 levels][240][8]: the de-rate-matching lists
    DevBuf<uint32_t> jump;          // [32] to the call's reference sequence, then psc_build_jump's [544]
    DevBuf<int> sf;                 // as Pdcch::sf
    DevBuf<double> llr;             // [LCS_PCFICH_MAX_SF][6336]
    DevBuf<lcs_pdcch_scan_dec> tab; // [LCS_PCFICH_MAX_SF][165][6]: every decode of the last scan
    DevBuf<lcs_pdcch_scan_msg> stage;   // [LCS_PCFICH_MAX_SF][990]: every subframe's listed entries in order, before the cap
    DevBuf<int> sfc;                // [LCS_PCFICH_MAX_SF][8]: every subframe's counts for the head
    DevBuf<unsigned char> pres;     // [65536][LCS_PCFICH_MAX_SF]: the subframes in which an RNTI has an in-space decode of sufficient quality
    DevBuf<lcs_pdcch_scan_info> rec;   // [1]
    DevBuf<lcs_pcfich_info> pcf_rec;   // [1]: the PCFICH's decisions on the call's rows, a record of this stage's own
    std::vector<int> h_map;         // the host blocks they are uploaded from
    std::vector<int16_t> h_derm;
    std::vector<lcs_pdcch_scan_dec> h_tab;   // one subframe of tab, for lcs_pdcch_scan_decodes
    uint32_t h_jump[32 + 544] = {};
    int h_sf[6 * LCS_PCFICH_MAX_SF + 10] = {};
    int key[13] = {};               // n_rb, ports, cp_type, id, phich_duration, phich_resource, n_sizes, size[6] of the tables; n_rb 0: none
    int jump_rb = 0;
    int cand_cap = 0;               // the candidates of the largest N_CCE among the key's maps
    int last_n_sf = 0, last_n_sizes = 0, last_n_cand[LCS_PCFICH_MAX_SF] = {};   // the last scan, for lcs_pdcch_scan_decodes; n_sf 0: none
  } pdcch_scan;
  // the PHICH on that grid (phich.hip: lcs_phich_wide, lcs_phich, lcs_phich_values), allocated by the first call of that stage.  The
  // unit tables are built on the host (phich.h) when the key changes, not per call.
  struct PhichEntry { double value, dsum, S; };   // phich.h: PhiEntry
  struct Phich {
    DevBuf<int> map;                // [3 m_i] PhiMap: n_unit, re[600]
    DevBuf<uint32_t> jump;          // [2][32]: jump-ahead to the call's reference sequence, and by 1600 clocks for the scrambling
    DevBuf<int> sf;                 // [n_sf][3] grid rows of every subframe's symbols 0 .. 2 (-1: not read / not needed), m_i[10]
    DevBuf<PhichEntry> tab;         // [LCS_PCFICH_MAX_SF][400]: every (group, seq) of the last call
    DevBuf<int> sfu;                // [LCS_PCFICH_MAX_SF]: n_unit of every subframe, -1: not read
    DevBuf<lcs_phich_info> rec;     // [1]
    std::vector<int> h_map;         // the host blocks they are uploaded from
    std::vector<PhichEntry> h_tab;  // one subframe of tab, for lcs_phich_values
    uint32_t h_jump[64] = {};
    int h_sf[3 * LCS_PCFICH_MAX_SF + 10] = {};
    int key[6] = {};                // n_rb, ports, cp_type, id, phich_duration, phich_resource of the tables; n_rb 0: none
    int jump_rb = 0;
    int last_n_sf = 0, last_n_unit[LCS_PCFICH_MAX_SF] = {};   // the last call, for lcs_phich_values; n_sf 0: none
  } phich;
  // the PDSCH behind that search space's grants (pdsch.hip: lcs_pdsch_wide, lcs_pdsch, lcs_turbo_decode), allocated by the first call
  // of that stage.  The tables are built on the host (pdsch.h) once, a forced grant's when its (K, F) changes; not per call.
  struct Pdsch {
    Pdcch pdc;                      // the PDCCH's blocks of this stage's own: the PDCCH stage's are not touched
    DevBuf<int> tabs;               // transport block sizes [2][27], QPP (f1, f2) [127][2]
    DevBuf<int> heads;              // PdsTabHead [2 * 27 + 4 + 32]
    DevBuf<int16_t> rank;           // [2 * 27 + 4 + 32][3][2244]: the de-rate-matching ranks (1A, forced, 1C)
    DevBuf<uint32_t> jump;          // [320]: to the reference sequence, by 1600 clocks, by 160 2^b clocks
    DevBuf<uint32_t> x1s;           // [256]: the Gold sequence's first register 1600 + 160 j clocks on
    DevBuf<int> sfrow;              // [n_sf]: the grid row of symbol 0 of every subframe that is there whole, else -1
    DevBuf<lcs_pdsch_block> blk;    // [n_sf][2]: the plan's blocks
    DevBuf<int> job;                // PdsJob [n_sf][2]
    DevBuf<int> res;                // [n_sf][2][2]: n_iter, status
    DevBuf<uint8_t> hard;           // [n_sf][2][2240]: the decisions
    DevBuf<double> llr;             // [n_sf][2][2 * 12 n_rb * 14]
    DevBuf<double> ws;              // [n_sf][2][32][8][72]: the forward metrics of the windows
    DevBuf<double> din;             // [3][2244]: lcs_turbo_decode's input
    DevBuf<lcs_pdsch_info> rec;     // [1]
    DevBuf<unsigned long long> sets;    // [n_sf][2][4]: the two sets of PRBs of every grant slot; allocated by the first call with a non-zero lcs_set_pdsch_alloc
    lcs_pdsch_alloc_cfg alloc = {0, -1, 0, 0};   // lcs_set_pdsch_alloc: stored here, handed to the launch as an argument
    bool tables_1c_ready = false;   // the 32 rank tables of format 1C behind the others: built by the first call that follows 1C
    int last_n_rb = 0;              // of the last call: lcs_pdsch_last_alloc
    // the combined redundancy versions (lcs_pdsch_comb_wide, lcs_pdsch_comb), allocated by the first call of those
    DevBuf<int> cjob;               // PdsCombJob [8]
    DevBuf<int> cres;               // [8][2]: n_iter, status
    DevBuf<uint8_t> chard;          // [8][2240]: the decisions of the groups that are decoded
    DevBuf<double> cws;             // [8][32][8][72]
    DevBuf<lcs_pdsch_comb_info> crec;   // [1]
    std::vector<int> h_tabs, h_heads;   // the host blocks they are uploaded from
    std::vector<int16_t> h_rank;
    std::vector<double> h_din;
    uint32_t h_jump[320] = {}, h_x1s[256] = {};
    int h_sfrow[LCS_PCFICH_MAX_SF] = {}, h_job[32] = {};
    int forced_key[LCS_PDSCH_MAX_FORCED][2] = {};   // K, F + 1 of the forced grants' rank tables; K 0: none
    bool tables_ready = false;
    int jump_rb = 0;
    size_t last_stride = 0;         // of llr in the last call, and its subframes: lcs_pdsch_last_soft
    int last_n_sf = 0;
  } pdsch;
  bool batch_screen = true;         // lcs_set_batch_screen: int8 batches of two or more windows are screened (xcorr_route.h)
  int screen_skip = 0;              // batches left unscreened before the next one is screened again: a batch that flagged more than a fifth of
                                    // its tiles (a busy band) costs more screened than not, and the next ones will be alike (lcs_batch_collect)
  bool screen_pending = false;      // the last correlation call was a screened batch: outside its flagged tiles the arrays hold the screen's
                                    // values until a debug call completes them (lcs_launch_xcorr_complete)
  bool c64_probe = false;           // lcs_set_float_batch_probe: complex<float> batches are checked for dongle data (every component k/128) and then take the u8 route
  DevBuf<uint8_t> c64_u8;           // ... the bytes such a batch is turned into
  int c64_skip = 0;                 // batches left before the next probe (after a batch that was NOT dongle data)
  bool last_c64_routed = false;     // the last lcs_batch_enqueue of a complex<float> batch took the u8 route
  bool percell_ready = false;
  // streaming mode (lcs_stream_*): the one-buffer, n_f = 1 chain captured once as a hipGraph; every
  // per-push input reaches the device through fixed pinned buffers, so the graph never changes
  bool st_open = false;              // the captured graph holds the workspace's addresses: nothing it reads may be reallocated
  int st_head = 0, st_count = 0;                  // two slots: oldest buffer in flight, number in flight
  int st_fmt = 0;
  uint32_t st_n_cap = 0;
  PinnedBuf<char> st_hin[2];                      // pinned copies of the pushed buffers
  DevBuf<char> st_din;                            // device copy (shared: the graph launches serialise)
  size_t st_in_bytes = 0;                         // bytes of one pushed buffer
  PinnedBuf<StreamHost> st_host[2];               // pinned parameter + result blocks
  int16_t *st_dtracked = nullptr;     // VIEWS (both point into st_dmirror)
  int *st_dntracked = nullptr;
  DevBuf<char> st_dmirror;           // device mirror of StreamHost's input part
  hipGraph_t st_graph[2] = {nullptr, nullptr};
  hipGraphExec_t st_exec[2] = {nullptr, nullptr};
  hipEvent_t st_ev0[2] = {nullptr, nullptr}, st_ev1[2] = {nullptr, nullptr};
  // the tracker (tracker.hip): trk_layout.h says which arrays every buffer holds and where
  struct Tracker {
    TrkPart<TB_TD, TRK_BLOCK_BUFS, TrkShape> block;                // lcs_track_block's workspace: any block of up to cap cells x symbols ...
    TrkShape last;                                                 // ... and the block the last call processed (lcs_track_stats reads it)
    TrkPart<TB_ACFD, TRK_STAT_BUFS, TrkShape> stats;               // lcs_track_stats' outputs
    TrkPart<TB_CUT_HIT, TRK_CUT_BUFS, TrkCutCap> cut;              // lcs_track_cut: laid out by the capacity, not by the call
    TrkStream stream;                                              // carried state of lcs_track_stream_block
    Buf<char, LcsPageableMem> stage;                               // reusable host staging block of a block (pageable): metadata up, measurement tables down
  } trk;
  // wideband channelizer (channelizer.hip)
  DevBuf<char> chan_par;            // [n_ch] phase steps, then the taps
  DevBuf<float> chan_tab;           // the filter bank in A-operand order
  PinnedBuf<char> chan_hpin[2];     // page-locked parameter slots, used in turn
  DevBuf<float2> chan_y;            // lcs_channelize_u8: the float outputs [n_ch][n_out] its bytes are made from
  DevBuf<float> chan_part;          // lcs_channelize_u8: [n_ch][workgroups along the outputs] sums of |y|^2
  int chan_slot = 0;
  bool chan_timed = false;
  // the continuous form (lcs_chan_stream_*): one stream per context, with its own parameters, table and history -- the one-shot
  // calls above stay legal while it is open and touch none of this
  struct ChanStream {
    bool open = false;
    int fmt = 0, up = 0, down = 0, n_ch = 0;
    DevBuf<char> par;               // [n_ch] phase steps, then the taps
    DevBuf<float> tab;              // the filter bank in A-operand order, built once by open
    DevBuf<char> hist[2];           // two history slots of cs_keep_max samples, written in turn
    int cur = 0;                    // the slot that holds samples [n_total - n_hist, n_total)
    unsigned n_hist = 0;
    unsigned long long n_total = 0; // samples pushed since open
    // the stream of 8-bit captures (lcs_chan_stream_open_u8): the capture in hand as floats until it is full and its gain is known
    bool u8 = false;
    uint32_t n_cap = 0, filled = 0; // outputs per capture, and how many of the capture in hand have been computed
    DevBuf<float2> cap;             // [n_ch][n_cap], and one sample of padding (k_chan_cap_power)
    DevBuf<float> cap_part;         // [n_ch][cap_power_blocks(n_cap)] sums of |y|^2 (k_chan_cap_power)
  } chan_stream;
  // the cancellation stage (sic.hip): every block is allocated by the first call that needs it and grown on demand
  struct Sic {
    DevBuf<char> cells;             // [n] SicCell records of the call, then [n_buf][2] first cell / cell count per buffer
    DevBuf<float2> pbch;            // [n][SIC_MAX_FRAMES][240]: the PBCH symbols of every frame of every cell
    DevBuf<double2> grid, grid_res; // [symbols of all cells][72]: the capture's grid, and the residual's
    DevBuf<double2> chan;           // [slots of all cells][4][72]
    DevBuf<double2> gain;           // [n]
    DevBuf<float2> td;              // [symbols of all cells][128]: what each symbol subtracts, before the carrier rotation
    DevBuf<double> part;            // [symbols of all cells][4]: energy per component
    DevBuf<lcs_sic_info> info;      // [n]
    DevBuf<float2> cap, res;        // lcs_search_*_sic: the single-buffer call's capture as complex<float>, and the residuals
    int stats[4] = {0, 0, 0, 0};    // lcs_last_sic_stats
    // lcs_search_*_sic: the side-table records of every cell the call handed out, gathered round by round on the host
    // (lcs_last_sic_tdd_info, lcs_last_sic_cell_meas), [h_n_buf][h_max_cells]
    std::vector<lcs_tdd_info> h_tdd;
    std::vector<lcs_meas_info> h_meas;
    int h_n_buf = 0, h_max_cells = 0;
  } sic;
  // results of a batch, compacted on the device (k_pack_results): [8 ints header][n_buf counts][records]; h_res = its page-locked mirror
  DevBuf<char> res_pack;
  PinnedBuf<char> h_res;
  double last_collect_host_us = 0;   // host time of the last lcs_batch_collect outside its wait for the GPU
  int collect_hint = 0;              // records the last collected batch returned: sizes the first copy of the next collect
  // host staging
  SlotParams h_params{};             // source of asynchronous parameter uploads of the single-buffer entry points
  PinnedBuf<char> h_pinned;
  DevBuf<char> h2d;                  // device staging of lcs_batch_enqueue_host
  PinnedBuf<char> h_stage[2];        // pinned slots for host sources that are not page-locked

  // launch records that outlive the call that built them
  BatchRecord batch;                 // the last enqueued batch
  Launch foe;                        // lcs_foe_partial -> lcs_foe_contend / lcs_foe_finish: this rank's share of the hypotheses (valid while foe_ready)
  bool foe_ready = false;
  int max_work = LCS_WORK_DEFAULT;   // cells per per-cell round (lcs_set_max_cells_in_flight; grows to LCS_MAX_WORK by itself unless the caller set it)
  bool max_work_pinned = false;      // the caller set the limit: it stays
  int percell_cap = 0;               // cells the per-cell buffers are allocated for
  int work_hint = 0;                 // cells the last collected batch carried into the per-cell stages: sizes the next batch's rounds and grids
  int hint_n_buf = 0, hint_fmt = -1, hint_stage = 0;   // the batch shape the hint was measured on
  int last_xc_launches = 0;
  double last_xc_ops = 0;            // matrix-core operations (2 x MACs) the correlation launches of the last batch executed
  const char *last_xc_kernel = "";
};

#ifndef LCS_EVENT_NOFENCE
#define LCS_EVENT_NOFENCE hipEventDisableSystemFence
#endif

inline int lcs_hip_error(lcs_ctx *c, const char *call, hipError_t e) {
  c->err = std::string(call) + ": " + hipGetErrorString(e);
  return LCS_ERR_HIP;
}
#define HIPCHK(ctx, call)                                                        \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) return lcs_hip_error((ctx), #call, e_);                \
  } while (0)

template <int FIRST, int N, class Cap> int TrkPart<FIRST, N, Cap>::regrow(lcs_ctx *c, const TrkLay &l, const Cap &want) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  cap = Cap();
  for (int b = 0, rc; b < N; ++b) if ((rc = buf[b].alloc(c, l.bytes[FIRST + b]))) return rc;
  cap = want;
  return LCS_OK;
}
template <class Rec> int SideTable<Rec>::begin(lcs_ctx *c, int n_buf, bool on) {
  made = on;
  if (!on) return LCS_OK;
  const size_t n = (size_t)n_buf * LCS_MAXP;
  if (n > tab.capacity()) HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc;
  if ((rc = tab.reserve(c, n))) return rc;
  HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(tab.get()), sentinel, n * (sizeof(Rec) / 4), c->stream));
  return LCS_OK;
}
template <class Rec> int SideTable<Rec>::read_last(lcs_ctx *c, int n_buf, const Rec &none, int32_t Rec::*key, Rec *out, int max_cells_per_buf) {
  for (size_t i = 0; i < (size_t)n_buf * max_cells_per_buf; ++i) out[i] = none;
  if (!made) return LCS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<Rec> t((size_t)n_buf * LCS_MAXP);
  HIPCHK(c, hipMemcpyAsync(t.data(), tab.get(), t.size() * sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = LCS_OK;
  for (int b = 0; b < n_buf; ++b) {
    int k = 0;
    for (int p = 0; p < LCS_MAXP; ++p) {
      const Rec &r = t[(size_t)b * LCS_MAXP + p];
      if (r.*key == sentinel) continue;
      if (k < max_cells_per_buf) out[(size_t)b * max_cells_per_buf + k] = r; else rc = LCS_ERR_OVERFLOW;
      ++k;
    }
  }
  if (rc) c->err = "more results than the output array holds";
  return rc;
}

// ---- host tables (lte_tables.cpp) --------------------------------------------------
namespace lcs_tables {
void pss_fd(int n_id_2, double *re_im /*62*2*/);
void pss_td(int n_id_2, double *re_im /*137*2*/);
void sss_fd(int n_id_1, int n_id_2, int slot_num, int32_t *out /*62*/);
void lte_pn(uint32_t c_init, uint32_t len, uint8_t *out);
void pn_jump_table(uint32_t steps, uint32_t out[32]);
// the block every stage on the full-bandwidth grid hands its kernels: [0 .. 31] to the reference sequence of n_rb resource blocks,
// [32 .. 63] by 1600 clocks for the scrambling.  32 x 1600-odd clocks of host work apiece: a stage builds it when its bandwidth
// changes, into a block of its own
inline void wide_jump_block(int n_rb, uint32_t out[64]) {
  pn_jump_table(1600 + 2 * (110 - n_rb), out);
  pn_jump_table(1600, out + 32);
}
double chi2cdf_inv(double p, double k);
void pbch_deratematch_map(int n_e, uint8_t *out /*n_e*/);   // ref src/lte_lib.cpp:409-463 via :473-478
bool pbch_derm_inv(int n_e, int16_t *out /*[120][16]*/);    // its inverse: per coded bit the positions carrying it (ascending, -1 padded)
// lte_pbch_enc.cpp: the QPSK symbols of one PBCH period from a record's fields (960 / 864 pairs); false: no MIB carries them
bool pbch_encode(int n_id_cell, int n_ports, int n_rb_dl, int phich_duration, int phich_resource, int sfn, int cp_type, double *out_re_im);
}  // namespace lcs_tables

// sic.hip: the cancellation of `cells` (records of buffer b at cells[b * max_cells_per_buf], n_cells_per_buf[b] of them) from the
// n_buf captures at d_cap (fmt U8 / C64) into d_res [n_buf][n_cap]; src_of (nullable: the identity): the capture of d_cap that slot b --
// its records, its carrier, its residual -- belongs to
int lcs_launch_sic(lcs_ctx *c, const void *d_cap, int fmt, int n_buf, uint32_t n_cap, const lcs_cell *cells, const int *n_cells_per_buf,
                   int max_cells_per_buf, const double *fc_req, const double *fc_prog, double fs_prog, int mask, int duplex, const int *src_of,
                   const int32_t *ul_dl_config /*like cells, nullable: the TDD cells' configurations, < 0 where there is none*/, float2 *d_res, lcs_sic_info *info);

// ---- kernel launchers (one per .hip file) -------------------------------------------
// pss_xcorr.hip
// The ingest launchers say what the fp64 stages read afterwards (*src): the int8 pairs of a u8 source, the fp32 copy, the
// caller's own complex<float> buffers read in place (lcs_launch_ingest_f16), or cap64.
int lcs_launch_ingest(lcs_ctx *c, const void *d_src, int fmt, int n_buf, uint32_t n_cap, CapSrc *src);
int lcs_launch_ingest_c128(lcs_ctx *c, uint32_t n_cap, bool *exact, CapSrc *src);   // cap64 -> cap32 + int8 copies; exact: every component is (u8 - 127) / 128
int lcs_launch_xcorr(lcs_ctx *c, const Launch &L, bool want_incoh, bool time_it);
int lcs_launch_xcorr_complete(lcs_ctx *c, const Launch &L);   // after a screened batch: the three-digit kernel over every tile, full collapse, full repair
int lcs_ensure_xc(lcs_ctx *c, unsigned sets);   // XcSet bits: the sets a call needs, allocated for the current workspace on first use
int lcs_launch_single_layout(lcs_ctx *c, const Launch &L, int slot, float *ref_layout, int to_ref);   // group-major <-> [t][idx][foi]
int lcs_launch_foe_contend(lcs_ctx *c, const Launch &L, const double *fset_g, const long long *d_words, long long *d_words2);
int lcs_launch_foe_resolve(lcs_ctx *c, long long *d_words, const long long *d_words2);
// pss_xcorr_i8.hip
int lcs_launch_fill_brow_i8(lcs_ctx *c, const Launch &L);
int lcs_launch_xcorr_i8(lcs_ctx *c, hipStream_t sxc, const Launch &L, int slot0, int n_slots, int xcd_map);   // L.screen: the two-digit pass
int lcs_launch_screen_refine(lcs_ctx *c, const Launch &L);   // behind the screen's collapse: flags, work list, the three-digit kernel over it
double lcs_i8_list_ops(const XcGeom &geo, int tiles, int last_tiles);   // matrix-core operations of that launch, once the host knows the counts
// pss_xcorr_f16.hip
int lcs_launch_ingest_f16(lcs_ctx *c, const void *d_src, int n_buf, uint32_t n_cap, CapSrc *src);   // complex<float> -> fp16 hi / lo pairs + per-buffer scale (+ cap32 unless read in place)
int lcs_launch_fill_brow_f16(lcs_ctx *c, const Launch &L);
int lcs_launch_xcorr_f16(lcs_ctx *c, hipStream_t sxc, const Launch &L, int slot0, int n_slots, int xcd_map);

int lcs_launch_xc_debug(lcs_ctx *c, const Launch &L);   // raw xc for slot 0 (debug output only)
// peak_search.hip
int lcs_launch_peak_search(lcs_ctx *c, const Launch &L, double udb10_m12, bool fp32_exact);
int lcs_launch_foe_pack(lcs_ctx *c, const Launch &L, long long *d_words, double *d_meta);      // collapsed (pow, frq) -> packed words
int lcs_launch_foe_unpack(lcs_ctx *c, const Launch &L, const long long *d_words, const double *d_meta);
// sss_foe.hip
int lcs_launch_sss_foe(lcs_ctx *c, const Launch &L, double thresh2_n_sigma, double *dbg /*device, nullable*/);
int lcs_launch_sss_only(lcs_ctx *c, const Launch &L, double thresh2_n_sigma, double *dbg);
int lcs_launch_foe_only(lcs_ctx *c, const Launch &L);
int lcs_launch_foe_coarse(lcs_ctx *c, const Launch &L, double *coarse /*device, 4: f_coarse, C.re, C.im, occurrences*/);
// tfg_mib.hip
int lcs_launch_gather_work(lcs_ctx *c, const Launch &L, int skip /* cells already handled by earlier rounds */);
__host__ __device__ static inline size_t lcs_pack_rec_offset(int n_buf) { return ((size_t)(8 + n_buf) * sizeof(int) + 63) & ~(size_t)63; }
int lcs_launch_pack_results(lcs_ctx *c, const Launch &L, bool full);   // peaks / npeaks (+ n_work) -> c->res_pack
int lcs_launch_rs_build(lcs_ctx *c, const Launch &L);
int lcs_launch_tfg(lcs_ctx *c, const Launch &L, bool with_rs /* also build RS_DL (the fused chain) */);
int lcs_launch_tfoec(lcs_ctx *c, const Launch &L, bool apply_grid);
int lcs_launch_mib(lcs_ctx *c, const Launch &L, bool fused);   // chan_est + PBCH candidates + selection (+ record back into the peak table)
int lcs_launch_chan_est(lcs_ctx *c, const Launch &L);
int lcs_launch_pbch_soft(lcs_ctx *c, const Launch &L, int guess, int n_ports, double *out /*[2048]*/);   // chan_est + one forced PBCH candidate's soft values
void lcs_pbch_soft_layout(int *d_est, int *bits, int *ok);                                              // where k_pbch_soft leaves them in `out`
int lcs_launch_tdd_config(lcs_ctx *c, const Launch &L, lcs_tdd_info *out /*device*/, bool force /* the stage: out[item], whatever the record carries */);
// cell_meas.hip
int lcs_launch_cell_meas(lcs_ctx *c, const Launch &L, const lcs_tdd_info *tdd /*device: this launch's k_tdd_config table, or null*/, lcs_meas_info *out /*device*/,
                         int dl_mask, bool force /* the stage: out[item] with dl_mask, whatever the record carries */);
// tfg_wide.hip
// rows of an n_fft-point grid from complex<float> samples on the device: row i is taken at round_i(h_ideal[i]) and lands in
// c->meas_wide.grid[i][12 n_rb].  kk: the frequency correction's phase step in half turns per sample
int lcs_launch_tfg_wide(lcs_ctx *c, const float2 *d_cap, uint32_t n_cap, const double *h_ideal, int n_rows, double kk, int n_fft, int n_rb);
// the measurement on the n_q reference rows that call left in c->meas_wide.grid -> c->meas_wide.rec
int lcs_launch_cell_meas_wide(lcs_ctx *c, const lcs_cell &cell, int n_q, int n_fft, int n_rb, int dl_mask);
// pcfich.hip
// a host grid of n_elem (re, im) pairs -> c->meas_wide.grid
int lcs_pcfich_stage_grid(lcs_ctx *c, const double *h_grid, size_t n_elem);
// the PCFICH of the n_sf subframes whose rows (rows[2 g], rows[2 g + 1]: symbols 0 and 1, -1: not read) c->meas_wide.grid holds
// -> c->meas_wide.pcf_rec
int lcs_launch_pcfich(lcs_ctx *c, const lcs_cell &cell, const int *rows, int n_sf, int n_rb, int dl_mask);
// pdcch.hip
// the resolved configuration of a call (wide_call.h: what cfg and the cell say together)
struct PdcchPlan;
// rows4 [n_sf][4]: the rows of c->meas_wide.grid that hold symbols 0 .. 3 of every subframe (-1: not read) -> c->pdcch.rec
int lcs_launch_pdcch(lcs_ctx *c, const lcs_cell &cell, const int *rows4, int n_sf, int n_rb, int dl_mask, const PdcchPlan &plan);
// the same into the blocks p (the PDSCH stage keeps a set of its own for the grants it follows) -> p.rec
int lcs_launch_pdcch_in(lcs_ctx *c, lcs_ctx::Pdcch &p, const lcs_cell &cell, const int *rows4, int n_sf, int n_rb, int dl_mask, const PdcchPlan &plan);
// pdcch_scan.hip
struct PdcchScanPlan;
// rows4 as lcs_launch_pdcch's -> c->pdcch_scan.rec, c->pdcch_scan.tab
int lcs_launch_pdcch_scan(lcs_ctx *c, const lcs_cell &cell, const int *rows4, int n_sf, int n_rb, int dl_mask, const PdcchScanPlan &plan);
// phich.hip
struct PhichPlan;
// the unit tables of (n_rb, ports, CP, id, PHICH duration and Ng), on the host and on the device: built when that key changes
int lcs_phich_tables(lcs_ctx *c, const lcs_cell &cell, int n_rb, const PhichPlan &plan);
// n_unit of the table of m_i (0 .. 2) that lcs_phich_tables left: -1 for a refused map
int lcs_phich_map_units(const lcs_ctx *c, int mi);
// rows3 [n_sf][3]: the rows of c->meas_wide.grid that hold symbols 0 .. 2 of every subframe (-1: not read, or not needed)
// -> c->phich.rec, c->phich.tab
int lcs_launch_phich(lcs_ctx *c, const lcs_cell &cell, const int *rows3, int n_sf, int n_rb, int dl_mask, const PhichPlan &plan);
// pdsch.hip
struct PdschPlan { int i_1a, max_iter, rnti_mask, n_forced, tdd; lcs_pdsch_grant forced[LCS_PDSCH_MAX_FORCED]; int alloc_flags, sfn0, si_window; };
// the PCFICH and PDCCH of rows4 into c->pdsch.pdc, then the grants' blocks -> c->pdsch.rec.  sfrow [n_sf]: the row of c->meas_wide.grid
// that holds symbol 0 of every subframe whose rows are all there, else -1
// comb (or null): after the decode the SI blocks are grouped and every group that needs it is decoded from the sum of its members'
// soft bits -> c->pdsch.crec
struct PdschCombPlan { int si_window, no_sib1; };
int lcs_launch_pdsch(lcs_ctx *c, const lcs_cell &cell, const int *rows4, const int *sfrow, int n_sf, int n_rb, int dl_mask, const PdcchPlan &plan, const PdschPlan &ps,
                     const PdschCombPlan *comb = nullptr);
// d [3][K + 4] from the host through the decode kernel -> c->pdsch.res[0 .. 1], c->pdsch.hard[0 .. K - 1]
int lcs_launch_turbo(lcs_ctx *c, const double *h_d, int K, int F, int max_iter);
void lcs_chan_est_np_layout(int *first, int *per_port, int *n_rs_first);   // where k_chan_est leaves its noise-power partial sums in cell_scratch
