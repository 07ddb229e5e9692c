/*
 * lcs.h -- C ABI of the MI355X-native LTE cell-search hot path (liblcs_amd.so).
 *
 * Drop-in boundary for the searcher of Evrytania/LTE-Cell-Scanner: every entry point
 * below replaces one free function of the reference's include/searcher.h (cited per
 * function) with plain pointers and sizes -- no IT++ or torch types.  The C++ wrappers
 * in include/searcher_amd.h re-expose the reference's exact C++ signatures on top of
 * this ABI; INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions
 *  - complex arrays are interleaved (re, im); capture buffers are complex<double>
 *    exactly as itpp::cvec stores them (host entry points) or complex<float> / raw
 *    u8 I/Q already resident in HBM (device entry points).
 *  - 2-D outputs [3][9600] are row-major (PSS index major); the reference's itpp::mat is
 *    column-major, the C++ wrapper transposes.
 *  - 3-D outputs are [t][idx][foi] with foi fastest, identical to the reference's
 *    nested-vector vf3d / vcf3d (include/common.h.in:41-44).
 *  - every function returns LCS_OK (0) or a negative error; "not found" stays in-band in
 *    lcs_cell (n_id_1 == -1 / n_rb_dl == -1) exactly as in the reference
 *    (src/CellSearch.cpp:530, 554).
 *  - correlation kernel: the DATA decides.  Dongle samples are exactly (u8 - 127) / 128 (src/capbuf.cpp:172-181) and exact
 *    in int8: handed over as raw bytes (LCS_FMT_IQ_U8) or as complex<double> through the reference's call shape (the host
 *    entry points check every component on the device), they run on the int8 matrix cores (templates as 24-bit integers
 *    in three int8 digits, exact int32 accumulation); batches of complex<float> buffers (LCS_FMT_C64) run on the fp16
 *    matrix cores (fp16 hi + lo parts of samples and templates, three products, fp32 accumulation), any other single
 *    buffer on the fp32 MFMA kernel.  All agree with the reference to ~1e-6 relative or better.  Templates are processed 16 to a group; any f_search_set is accepted: a grid whose
 *    hypotheses' window starts drift apart by more samples than a group's operand rows hold (> 15 samples for int8 / fp16, > 111
 *    for fp32 -- far sparser than the 5 kHz grids of the CLI) is packed with fewer whole hypotheses per group, down to
 *    one, at proportionally more work.
 *  - a context owns one HIP device + stream + workspace; calls on one context are
 *    serialised by the caller, different contexts are independent (the reference's
 *    functions are re-entrant).
 *  - there is NO CPU fallback: if no gfx950 device is usable, lcs_create fails.
 */
#ifndef LCS_H
#define LCS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCS_OK 0
#define LCS_ERR_NO_DEVICE (-1)
#define LCS_ERR_BAD_ARG (-2)
#define LCS_ERR_HIP (-3)
#define LCS_ERR_OVERFLOW (-4)   /* more results than the caller's array holds (outputs truncated) */
#define LCS_ERR_NOMEM (-5)

#define LCS_CP_UNKNOWN 0
#define LCS_CP_NORMAL 1
#define LCS_CP_EXTENDED 2

#define LCS_N_PSS 3
#define LCS_N_IDX 9600          /* 5 ms at 1.92 Msps */
#define LCS_TFG_NSC 72
#define LCS_TFG_MAX_OFDM 854    /* 6 frames + 2 slots, normal CP (src/searcher.cpp:895) */
/* The reference's peak_search appends to a std::list<Cell> without a bound (src/searcher.cpp:468-476).  The list is bounded
 * all the same: every peak zeroes 274 positions either side of itself in its PSS row (:480-485), so two peaks of one row lie
 * at least 275 positions apart on the circle of 9600 -- at most 34 per row, 102 per buffer -- and the loop ends at the
 * first maximum below Z_th1 (:449).  The library keeps LCS_MAX_PEAKS records per buffer: every list the reference can return
 * for a buffer whose thresholds are positive fits.  (A buffer of zeros has Z_th1 == 0 everywhere: the reference's loop then
 * never ends; here it stops at LCS_MAX_PEAKS peaks and the call reports LCS_ERR_OVERFLOW.) */
#define LCS_MAX_PEAKS 104
/* Footprint that follows from that bound: the SSS / FOE stage keeps 60 KB of window records per POSSIBLE peak of a batch
 * (n_buf x LCS_MAX_PEAKS x 8 half-frame occurrences x 3 KB -- 800 MB for a 128-buffer context, allocated by the first full-chain
 * batch), the peak table 104 x 104 B per buffer.  Real buffers carry a handful of peaks; the worst case is what is reserved. */

/* POD mirror of class Cell -- include/common.h.in:101-129, defaults src/common.cpp:36-56. */
typedef struct lcs_cell {
  double fc_requested;
  double fc_programmed;
  double pss_pow;
  double freq;
  double frame_start;
  double freq_fine;
  double freq_superfine;
  int32_t ind;
  int32_t n_id_2;
  int32_t n_id_1;
  int32_t cp_type;        /* LCS_CP_* */
  int32_t n_ports;
  int32_t n_rb_dl;
  int32_t phich_duration; /* 0 UNKNOWN, 1 NORMAL, 2 EXTENDED */
  int32_t phich_resource; /* 0 UNKNOWN, 1 oneSixth, 2 half, 3 one, 4 two */
  int32_t sfn;
  int32_t reserved;
} lcs_cell;

typedef struct lcs_ctx lcs_ctx;

/* ---- context ------------------------------------------------------------------- */
/* device < 0: use the current HIP device.  Fails (LCS_ERR_NO_DEVICE) without a GPU. */
int lcs_create(int device, lcs_ctx **out);
void lcs_destroy(lcs_ctx *ctx);
const char *lcs_last_error(const lcs_ctx *ctx);
const char *lcs_version(void);
void lcs_cell_init(lcs_cell *c);                      /* src/common.cpp:36-56 */
/* Memory-footprint limit: the per-cell stages (time-frequency grid, channel estimate, PBCH) hold at most n
 * detected cells at a time, ~6 MB each, allocated on first use FOR THAT MANY CELLS (n <= 1024).  Without this call a context
 * starts at 512 (3 GB) and doubles to 1024 by itself after a batch that carried more cells past SSS than that (a busy
 * band); after the call the limit stays where the caller put it.  A batch with more cells is processed in rounds:
 * lcs_batch_enqueue launches the rounds the PREVIOUS batch of the same shape needed (at least one detected cell per buffer),
 * lcs_batch_collect launches the rest if the device-side count says the batch had more.  Results do not depend on it and
 * no batch is truncated. */
int lcs_set_max_cells_in_flight(lcs_ctx *ctx, int n);
/* complex<float> BATCHES that are dongle data.  A float pipeline in front of the searcher often still carries RTL-SDR samples --
 * every component exactly (u8 - 127) / 128 (src/capbuf.cpp:172-181).  The host entry points recognise such data in complex<double> by
 * themselves and correlate the bytes (int8 kernel); for device-resident LCS_FMT_C64 batches the same check is opt-in, because it costs
 * lcs_batch_enqueue a host synchronisation: with on != 0 every such batch is first checked on the device (one pass that also writes the
 * bytes; the host waits for the verdict while the other contexts' kernels keep the GPU busy) and, if every component of every buffer
 * compares equal to one of the 256 values (one ulp beside one, or a tiny value, is no dongle data), takes the u8 route from there -- the same numbers through the int8 kernel (1.4 x the fp16 kernel's rate) and
 * the caller's buffer is not read again after the call returns; anything else takes the fp16 kernel as before (and the next fifteen
 * batches of the context are not checked).  Off by default.  Results do not depend on it. */
int lcs_set_float_batch_probe(lcs_ctx *ctx, int on);
/* Duplex mode of the band a context searches: where the SSS lies relative to the PSS.  LCS_DUPLEX_FDD (the default, and the
 * reference's only mode: frame structure type 1, PSS in the last symbol of slots 0 / 10, SSS directly before it) or
 * LCS_DUPLEX_TDD (36.211 frame structure type 2, bands 33-53: PSS in symbol 2 of slots 2 / 12, SSS in the last symbol of slots
 * 1 / 11, three symbols earlier).  Under FDD every record and every array is what it was before the mode existed, bit for bit.  The mode
 * is context-wide -- one wideband capture covers one band, and a band has one duplex -- and reaches every entry point that runs
 * sss_detect or pss_sss_foe: lcs_sss_detect, lcs_pss_sss_foe, lcs_search_capbuf, the batch entry points (device and host, enqueue
 * and collect: a batch keeps the mode it was enqueued with), the streaming mode and lcs_foe_finish.  Everything behind those two
 * stages (lcs_extract_tfg, lcs_tfoec, lcs_decode_mib) takes the frame timing from the cell record and needs no mode.  In samples at
 * 1.92 Msps, sc = 16 / FS_LTE * fs_programmed * k_factor:
 *                                                FDD                              TDD
 *   SSS DFT window, normal / extended CP         pss_dft - 137 / - 160            pss_dft - 412 / - 480
 *   peak moved right by 9600 k_factor when       peak_loc + 9 < 162               peak_loc + 9 < 482
 *   PSS DFT start inside the frame (P)           832                              2204 normal CP, 2272 extended CP
 *   frame_start before half-frame step and wrap  cell.ind + (9 - 2 - P) sc        peak_loc + (9 - 2 - P) sc
 *   pss_sss_dist, normal / extended CP           round(137 sc) / round(160 k)     round(412 sc) / round(480 k)
 *   first SSS DFT start minus frame_start        695 sc / 672 sc                  1792 sc
 * (TDD's frame_start reads the peak position BEHIND the room rule, as the reference's Matlab original does; FDD keeps the C++
 * reference's cell.ind, which is half a frame off for the peaks the rule moved -- the first 153 samples there, the first 473 here.)
 * lcs_set_duplex refuses (LCS_ERR_BAD_ARG, an lcs_last_error text) any other value, and a change while an lcs_stream_open stream
 * is open: the captured graph holds the mode it was opened with.
 * NO AUTOMATIC DECISION between the two is made: trying both would double the SSS windows per occurrence (the window kernel has two
 * idle window slots per pair of occurrences and would need four) and would change the population the second threshold
 * (thresh2_n_sigma) is taken over, i.e. the decision itself, for FDD cells too.
 * RANGE OF THE FREQUENCY ESTIMATE.  pss_sss_foe measures a phase over pss_sss_dist samples and is by itself unambiguous within
 * +- fs k / (2 pss_sss_dist) of the hypothesis the peak was found at: FDD +- 7.0 kHz (normal CP) / +- 6.0 kHz (extended), TDD
 * +- 2330 Hz / +- 2000 Hz.  On the reference's 5 kHz hypothesis grid the residual reaches +- 2500 Hz: a TDD search needs a grid step
 * of at most 4 kHz (host/CellSearch -x tdd and the Python helper f_search_set_for(..., step=2.5e3) use 2.5 kHz) unless
 * lcs_set_foe_unwrap is on, which gives TDD +- 1.5 periods (+- 6990 Hz / +- 6000 Hz) and with them the 5 kHz grid.  The library
 * does not touch the caller's f_search_set.
 * The tracker entry points (lcs_track_*) stay FDD whatever the mode: lcs_track_cut and lcs_track_block take symbol positions from
 * the caller, and the PSS / SSS positions of lcs_track_stats are frame structure type 1's. */
#define LCS_DUPLEX_FDD 0
#define LCS_DUPLEX_TDD 1
int lcs_set_duplex(lcs_ctx *ctx, int duplex);
int lcs_get_duplex(const lcs_ctx *ctx, int *duplex);
/* A second mode of the frequency estimate: pss_sss_foe unwrapped by a PSS-only coarse estimate.  The native estimate aliases by
 * whole periods fs / pss_sss_dist (see above); nothing else in the chain minds a residual of +- 2.5 kHz -- the PSS correlation and
 * the peak search do not, and sss_detect removes the common PSS -> SSS phase before its likelihood.  With on = 1 every call that
 * runs pss_sss_foe also computes, per cell and on the device, the phase between the two halves of the PSS's time-domain symbol,
 * 64 samples apart (range +- 15 kHz): with fs = fs_programmed k_factor, dist = pss_sss_dist, and first_sss, step, n_sss as
 * pss_sss_foe forms them in the context's duplex mode,
 *   P_k      = round(first_sss + k step) + dist + 2                       first sample of the PSS's useful part, k = 0 .. n_sss - 1
 *   z_k[t]   = capbuf[P_k + t] cis(-2 pi cell.freq / fs t) conj(p[t])     t = 0 .. 127, p[t] = entry 9 + t of lcs_table_pss_td(n_id_2)
 *   A_k, B_k = the sums of z_k over t < 64 and t >= 64;  C = sum_k conj(A_k) B_k, in occurrence order, unweighted
 *   f_coarse = atan2(C.im, C.re) / (2 pi) fs / 64                         relative to cell.freq
 *   n        = clamp(rint((f_coarse - (native - cell.freq)) / (fs / dist)), -1, +1);  0 if n_sss = 0 or C is zero or not finite
 *   freq_fine = native if n = 0 (the same double), native + n fs / dist otherwise
 * where native is the reference's freq_fine.  One rule for both duplex modes (in FDD n is 0 on any sane grid).  Off by default, and
 * then every record and every array is what it was before the mode existed, bit for bit.  Context-wide like the duplex mode, and it
 * reaches the same entry points: lcs_pss_sss_foe, lcs_search_capbuf, the batch entry points (device and host, enqueue and collect:
 * a batch keeps the mode it was enqueued with), the streaming mode and lcs_foe_finish.  lcs_set_foe_unwrap refuses
 * (LCS_ERR_BAD_ARG, an lcs_last_error text) any value other than 0 / 1, and a change while an lcs_stream_open stream is open. */
int lcs_set_foe_unwrap(lcs_ctx *ctx, int on);
int lcs_get_foe_unwrap(const lcs_ctx *ctx, int *on);
/* The uplink-downlink configuration of a TDD cell (36.211 table 4.2-2), estimated from its cell-specific reference signals.  The
 * configuration is broadcast in SIB1, which a 1.92 Msps searcher cannot read for a cell wider than 6 RB; but CRS are sent in every
 * downlink subframe and in the DwPTS and never in an uplink subframe, and the chain holds 61 subframes of the grid of every cell
 * that decoded a MIB.  THE RULE (lte-cell-scanner_amd/csrc/tdd_config.h, host and device), for a cell with n_id_1, n_id_2, cp_type
 * and a grid tfg[n_ofdm][72] whose row 0 is slot 0 symbol 0 of a frame -- what lcs_extract_tfg delivers for a record behind
 * lcs_decode_mib.  No frequency or timing correction is applied: a row's frequency correction is a common phase and drops out of
 * the products below, the timing correction turns every product by one angle and drops out in the projection on ref; the rule
 * gives the same answer on the raw grid (which the fused chain holds) and on the compensated one.  With n_symb = 7 / 6:
 *   rows used   r with sym = r mod n_symb in {0, n_symb - 3}: port 0's reference symbols.  slot = (r / n_symb) mod 20, s = slot / 2,
 *               j = 2 (slot & 1) + (sym != 0)
 *   per row     h_m = tfg[r][shift + 6 m] conj(rs[m]), m = 0 .. 11 (shift, rs: RS_DL of (slot, sym, port 0));
 *               c_r = sum_{m = 0 .. 10} h_m conj(h_{m+1})
 *   per bin     C[s][j] = sum of c_r in row order, N[s][j] = rows;  C[s] = sum_j C[s][j], N[s] = sum_j N[s][j]
 *   statistic   ref = C[0] + C[5], n_ref = N[0] + N[5] (subframes 0 and 5 are downlink in every configuration);
 *               T[s] = Re(C[s] conj(ref)) / |ref|^2  n_ref / N[s]      ~ 1 with CRS, ~ 0 without, whatever the uplink carries
 *   decision    subframe s is downlink iff T[s] > 1/2.  The pattern over s = (3, 4, 7, 8, 9) names the configuration:
 *               UUUUU 0, UDUUD 1, DDUDD 2, UUDDD 3, UDDDD 4, DDDDD 5, UUUUD 6; any other pattern gives -1, and so does a subframe 2
 *               that reads downlink (it is uplink in every configuration: a grid that is no TDD frame gets no number)
 *   margin      min |T[s] - 1/2| over s = 2, 3, 4, 7, 8, 9
 *   DwPTS       R[j] = Re((C[1][j] (+ C[6][j])) conj(ref)) / |ref|^2  n_ref / (N[1][j] (+ N[6][j])), subframe 6 joining only where
 *               the configuration found has it special (0, 1, 2, 6); row j is present iff R[j] > 1/2; dwpts_rs_rows = the number of
 *               rows present if they are a prefix that starts with row 0, else -1 (and -1 without a configuration):
 *                 1: DwPTS of 3 symbols (either CP)   2: 6 (normal CP) / 5 (extended)   3: 9-11 / 8-9   4: 12 / 10
 *   no decision when ref is zero or not finite, a subframe has no row, or a T is not finite: configuration -1, margin 0.
 * WHAT IT CANNOT SEE: the special-subframe configuration beyond these four DwPTS classes (GP and UpPTS carry no CRS), and anything
 * at all for a cell that decodes no MIB -- its records read LCS_TDD_NOT_ESTIMATED in both integer fields.
 * lcs_set_tdd_config(ctx, 1) makes every fused call of a context in LCS_DUPLEX_TDD run the rule, once per per-cell round behind
 * the MIB decode, on the device (one kernel, k_tdd_config): lcs_search_capbuf and the batch entry points (device and host, enqueue
 * and collect: a batch keeps the mode it was enqueued with).  After any of them lcs_last_tdd_info hands out one record
 * per cell: info[b * max_cells_per_buf + k] belongs to cells[b][k] of that call (b = 0 for lcs_search_capbuf); entries beyond a
 * buffer's cells, and every entry after a call with the mode off or in FDD, read LCS_TDD_NOT_ESTIMATED.  It waits for the context's
 * stream.  lcs_cell does not change.  Off by default, context-wide; with the mode off, or in FDD, every record and every array is
 * what it was before the mode existed, bit for bit, and no additional kernel is launched.  The streaming mode does not carry the
 * estimate yet: lcs_stream_open refuses (LCS_ERR_BAD_ARG, an lcs_last_error text) a context with the mode on, and
 * lcs_set_tdd_config refuses a change while a stream is open, and any value other than 0 / 1. */
typedef struct lcs_tdd_info {
  int32_t ul_dl_config;   /* 0 .. 6, -1: no configuration fits, LCS_TDD_NOT_ESTIMATED */
  int32_t dwpts_rs_rows;  /* 1 .. 4, -1, LCS_TDD_NOT_ESTIMATED */
  double margin;
  double T[10];
  double R[4];
} lcs_tdd_info;           /* 128 bytes */
#define LCS_TDD_NOT_ESTIMATED (-2)
int lcs_set_tdd_config(lcs_ctx *ctx, int on);
int lcs_get_tdd_config(const lcs_ctx *ctx, int *on);
int lcs_last_tdd_info(lcs_ctx *ctx, lcs_tdd_info *info, int max_cells_per_buf);
/* How strong and how clean a cell is: RSRP, RSSI, RSRQ (36.214 5.1.1, 5.1.3) and the noise power on its cell-specific reference
 * signals, from the grid the chain holds of every cell that decoded a MIB.  pss_pow (the reference's "RXPWR") is the peak of a
 * normalised PSS correlation: no power per resource element, and silent about noise and load.  THE RULE
 * (lte-cell-scanner_amd/csrc/cell_meas.h, host and device), for a cell with n_id_1, n_id_2, cp_type and n_ports, a grid
 * tfg[n_ofdm][72] whose row 0 is slot 0 symbol 0 of a frame (lcs_extract_tfg, raw or compensated), and a 10-bit dl_mask whose bit s
 * says that subframe s is measured:
 *   rows used   port 0's reference rows q = 0, 1, .. (grid row (q >> 1) n_symb + ((q & 1) ? n_symb - 3 : 0), as for lcs_set_tdd_config)
 *               whose subframe s = ((q >> 1) mod 20) / 2 has its bit in dl_mask; n_rows of them
 *   ports       P = 2 if n_ports >= 2, else 1 (n_ports 0 / unknown: port 0 alone).  Ports 0 and 1 share these rows and the row's RS_DL
 *               sequence rs; port p's first subcarrier shift_p is RS_DL's shift of (slot, symbol, port p)
 *   per row, port   h_m = tfg[row][shift_p + 6 m] conj(rs[m]), m = 0 .. 11;  a_p = sum_{m<11} h_m conj(h_{m+1});  e_p = sum_{m<12} |h_m|^2
 *   per row     w = sum_{k<72} |tfg[row][k]|^2
 *   sums        A_p = sum a_p, E_p = sum e_p, W = sum w over the used rows
 *   rsrp[p]     |A_p| / (11 n_rows): the signal power per reference resource element -- the noise of neighbouring subcarriers is
 *               independent, so the neighbour product keeps it out
 *   noise[p]    E_p / (12 n_rows) - rsrp[p]: what is on the reference resource elements beside the signal.  It may come out <= 0 on a
 *               short, clean grid and is handed out as it is
 *   rssi        W / n_rows: the power of one OFDM symbol that carries port 0's reference signals, over the 6 resource blocks seen
 *   rsrq        6 rsrp[0] / rssi (36.214: N RSRP / RSSI with N = 6)
 *   a_re_im     A_0 and A_1 as (re, im) pairs
 * The SINR of port p is rsrp[p] / noise[p]: the caller's division, infinite where noise[p] <= 0.  UNITS are the grid's: with the
 * reference's dft scaling a bin's power is the capture's power per sample, so for dongle bytes 1.0 is full scale, (u8 - 127) / 128.
 * status: 0 measured; -1 no number (no used row, an rssi of zero, or a sum that is not finite: every double of the record is then 0);
 * LCS_MEAS_NOT_MEASURED: the record was never written (all four integers then read so).
 * WHAT IT IS NOT: it assumes that the channel hardly changes over 6 subcarriers -- on a strongly frequency-selective channel at
 * high SNR noise reads high (a 25 % amplitude ripple over the 72 subcarriers at 25 dB: 2.3 to 2.6 times the true noise); other
 * cells count as noise; it sees the 6 centre resource blocks whatever n_rb_dl is; and it says nothing about a cell without a MIB.
 * lcs_set_cell_meas(ctx, 1) makes every fused call run the rule once per per-cell round, behind the MIB decode (and behind
 * k_tdd_config where that runs), on the device (one kernel, k_cell_meas): lcs_search_capbuf and the batch entry points (device and
 * host, enqueue and collect: a batch keeps the mode it was enqueued with).  The chain's dl_mask: 0x3ff in LCS_DUPLEX_FDD; 0x021
 * (subframes 0 and 5, downlink in every configuration) in LCS_DUPLEX_TDD; and where lcs_set_tdd_config is on as well and gave the
 * cell a configuration 0 .. 6, lcs_tdd_dl_mask of it (its D subframes, special subframes excluded).  The record says which was used.
 * lcs_last_cell_meas has the semantics of lcs_last_tdd_info: info[b * max_cells_per_buf + k] belongs to cells[b][k] of the last
 * fused call; entries beyond a buffer's cells, and every entry after a call with the mode off, read LCS_MEAS_NOT_MEASURED.
 * lcs_cell does not change.  Off by default, context-wide, 0 / 1 only; with the mode off no kernel is launched, no buffer is
 * allocated, and every record and array is bit for bit what it was.  The streaming mode does not carry the measurement:
 * lcs_stream_open refuses (LCS_ERR_BAD_ARG, an lcs_last_error text) a context with the mode on, and lcs_set_cell_meas refuses a
 * change while a stream is open. */
typedef struct lcs_meas_info {
  int32_t status, n_rows, n_ports, dl_mask;   /* n_ports: the ports measured, P */
  double rsrp[2], noise[2], rssi, rsrq, a_re_im[4];
  double reserved[4];
} lcs_meas_info;          /* 128 bytes; (lcs_cell_meas is the stage's name, so the record cannot have it) */
#define LCS_MEAS_NOT_MEASURED (-2)
int lcs_set_cell_meas(lcs_ctx *ctx, int on);
int lcs_get_cell_meas(const lcs_ctx *ctx, int *on);
int lcs_last_cell_meas(lcs_ctx *ctx, lcs_meas_info *info, int max_cells_per_buf);
/* the downlink subframes of uplink-downlink configuration 0 .. 6 (36.211 table 4.2-2) as a dl_mask, special subframes excluded; -1
 * for anything else */
int lcs_tdd_dl_mask(int ul_dl_config);
/* The same measurement over the cell's whole bandwidth, from wide samples that are resident on the device (lcs_cell_meas_wide,
 * lcs_extract_tfg_wide below; a stage of its own, not part of the fused chain).  THE RULE (lte-cell-scanner_amd/csrc/cell_meas_wide.h,
 * host and device), for a cell with n_id_1, n_id_2, cp_type, n_ports, frame_start and freq_fine, a DEVICE buffer of n_cap
 * complex<float> samples at fs_programmed ~ 1.92e6 R centred on the cell's carrier (frame_start counts in that buffer's samples),
 * n_fft = 128 R with R in {1, 2, 4, 8, 16}, n_rb resource blocks with 6 <= n_rb <= {6, 15, 25, 50, 100}[log2 R] (fewer than the
 * cell has is fine), n_ofdm rows with 2 n_symb <= n_ofdm <= 122 n_symb, and a dl_mask as above:
 *   positions   extract_tfg's with the caller's rate (src/searcher.cpp:875-934): k_factor = (fc_requested - freq_fine) / fc_programmed;
 *               the first DFT starts at frame_start + {10 | 32} 16 / FS_LTE fs_programmed k_factor, moved 10 ms back where that stays
 *               > -0.5; the steps are (128 + 9 | 10 | 32) 16 / FS_LTE fs_programmed k_factor; every DFT is taken at round_i of its location
 *   correction  sample i of the buffer is turned by fshift(-freq_fine, fs_programmed k_factor), i.e. by exp(j pi kk i) with
 *               kk = -freq_fine / (fs_programmed k_factor / 2), the phase kk i formed in double and reduced exactly (sincospi)
 *   grid row    concat(dft.right(6 n_rb), dft.mid(1, 6 n_rb)) of the n_fft samples, dft = fft / sqrt(n_fft) as the reference's, times
 *               exp(-j 2 pi late / n_fft cn), late = round_i(location) - location, cn = -6 n_rb .. -1, 1 .. 6 n_rb: 12 n_rb columns
 *   rs          36.211 6.10.1.1 for N_RB = n_rb: r(m'), m' = m + 110 - n_rb, m = 0 .. 2 n_rb - 1 (at n_rb = 6 RS_DL's twelve); the
 *               shifts of ports 0 and 1 as above
 *   per row, port   h_m = tfg[row][shift_p + 6 m] conj(rs[m]);  a_p = sum_{m < 2 n_rb - 1} h_m conj(h_{m+1});  e_p = sum_m |h_m|^2
 *   per row     w = sum_k |tfg[row][k]|^2;  per resource block i: b_p[i] = h_{2i} conj(h_{2i+1}), w[i] = the power of its 12 columns
 *   rsrp[p]     |A_p| / ((2 n_rb - 1) n_rows);  noise[p] = E_p / (2 n_rb n_rows) - rsrp[p];  rssi = W / n_rows;  rsrq = n_rb rsrp[0] / rssi
 *   rsrp_rb[p][i]   |B_p[i]| / n_rows;  rssi_rb[i] = W[i] / n_rows;  entries i >= n_rb are zero
 * over port 0's reference rows under the mask, as above; status and the conditions for "no number" are lcs_meas_info's (the per-RB
 * arrays are then zero as well).  Resource block 0 is the lowest in frequency (columns 0 .. 11 of a grid row).  UNITS are the
 * buffer's power per sample, as above; the same cell fills 1 / R of the bins of a buffer at 1.92e6 R, so its rsrp, noise and rssi
 * read R times (10 log10 R dB above) what they read at 1.92 Msps.  rsrq and the SINR are ratios. */
#define LCS_MEAS_WIDE_MAX_RB 100
typedef struct lcs_meas_wide_info {
  int32_t status, n_rows, n_ports, dl_mask;
  int32_t n_rb, n_fft, reserved_i[2];
  double rsrp[2], noise[2], rssi, rsrq, a_re_im[4];
  double reserved[2];
  double rsrp_rb[2][LCS_MEAS_WIDE_MAX_RB];
  double rssi_rb[LCS_MEAS_WIDE_MAX_RB];
} lcs_meas_wide_info;     /* 2528 bytes */

/* The PCFICH of a wide cell: the control format indicator of every downlink subframe of a full-bandwidth grid (lcs_pcfich_wide,
 * lcs_pcfich below; a stage of its own beside the chain).  THE RULE (lte-cell-scanner_amd/csrc/pcfich.h, host and device), on a grid
 * tfg[n_ofdm][12 n_rb] whose row 0 is symbol 0 of slot 0 of a frame (row r: symbol r mod n_symb of slot (r / n_symb) mod 20), for
 * n_id_cell, the CP type, n_ports in {1, 2, 4} (anything else counts as 1), n_rb in {6, 15, 25, 50, 75, 100} and a 10-bit dl_mask:
 *   subframes   grid subframe g = 0, 1, .. starts at row 2 g n_symb and is subframe g mod 10 of its frame; it is decoded iff that bit
 *               of dl_mask is set, the row lies inside n_ofdm and, with 4 ports, the row after it does too
 *   elements    36.211 6.7.4: kbar = 6 (n_id_cell mod 2 n_rb); quadruplet i < 4 sits in the resource-element group of symbol 0 that
 *               starts at column (kbar + 6 floor(i n_rb / 2)) mod 12 n_rb and takes, in increasing order, the four of its six
 *               columns that are not = n_id_cell (mod 3): both reference positions stay free whatever the port count
 *   channel     per port p, h_p[m] = tfg[row][shift_p + 6 m] conj(rs[m]) on the port's reference row (symbol 0 for ports 0 and 1,
 *               symbol 1 of the same slot for ports 2 and 3; shift and rs as for lcs_meas_wide_info), interpolated linearly between
 *               the two reference elements that bracket the column and, outside the first and the last, extrapolated on the line
 *               through the nearest two; no smoothing, nothing across time
 *   combining   1 port: s = conj(h) y.  2 ports, per pair (y0 at k0, y1 at k1) of a quadruplet: s0 = conj(h0(k0)) y0 + h1(k1) conj(y1),
 *               s1 = conj(h0(k1)) y1 - h1(k0) conj(y0).  4 ports: the same with ports (0, 2) for a quadruplet's first pair and (1, 3)
 *               for its second
 *   soft bits   b[2 j] = Re s_j, b[2 j + 1] = Im s_j, 32 of them, times 1 - 2 c(i) of the Gold sequence with
 *               c_init = (sf + 1) (2 n_id_cell + 1) 2^9 + n_id_cell, sf = g mod 10
 *   decision    corr[c] = sum_i b_i (1 - 2 w_c[i]) / sum_i |b_i| over the codewords of 36.212 table 5.3.4-1 (w_c[i] = 0 iff i mod 3
 *               = c, c = cfi - 1); cfi = 1 + argmax (the lowest on a tie), margin = best - second, n_ctrl_sym = cfi + (n_rb <= 10).
 *               A subframe whose sum of |b_i| is zero or not finite is not decoded.
 * Per subframe g < n_sf = ceil(n_ofdm / (2 n_symb)): cfi[g] (0: not decoded, its corr and margin are zero), corr[g], margin[g]; the
 * entries beyond n_sf are zero.  n_decoded and n_cfi count the decoded subframes, mean_n_ctrl_sym and min_margin are taken over
 * them in subframe order (zero without one).  It does not equalise across time and reads neither PHICH nor PDCCH; the CFI of a
 * TDD special subframe (one or two symbols at most) is the caller's to mask out. */
#define LCS_PCFICH_MAX_SF ((LCS_TFG_MAX_OFDM + 11) / 12)
typedef struct lcs_pcfich_info {
  int32_t n_sf, n_decoded, n_cfi[3], dl_mask, n_rb, n_ports;   /* n_ports: 1, 2 or 4 as the rule took it */
  double mean_n_ctrl_sym, min_margin;
  int32_t cfi[LCS_PCFICH_MAX_SF];
  double corr[LCS_PCFICH_MAX_SF][3];
  double margin[LCS_PCFICH_MAX_SF];
} lcs_pcfich_info;        /* 2640 bytes */

/* The PDCCH common search space of a wide cell: the DCIs whose CRC is masked with the SI-RNTI, the P-RNTI or an RA-RNTI, in every
 * downlink subframe of a full-bandwidth grid (lcs_pdcch_wide, lcs_pdcch below; a stage of its own beside the chain).  THE RULE
 * (lte-cell-scanner_amd/csrc/pdcch.h, host and device; grid, subframes, channel and combining as for lcs_pcfich_info):
 *   control     symbols 0 .. n_ctrl - 1 of the subframe's first slot, n_ctrl = cfi + (n_rb <= 10); the cfi is the PCFICH's decision
 *               for that subframe, or cfi_force.  A subframe is read iff its bit of dl_mask is set, the rows of symbols 0 .. 2 (0 .. 3
 *               for n_rb <= 10) lie inside n_ofdm and its cfi was decoded
 *   REGs        36.211 6.2.4: symbol 0 has two per resource block (six columns, the four that are not = n_id_cell (mod 3)); symbol 1
 *               three of four consecutive columns, with 4 ports two as symbol 0; symbol 2 three; symbol 3 three, with the extended
 *               CP two as symbol 0.  A REG is named (k', l'), k' its lowest column
 *   PCFICH      its four REGs of symbol 0.   PHICH (36.211 6.9.3): U = m_i ceil(Ng n_rb / 8) units of three REGs; with n_l the REGs
 *               of symbol l beside the PCFICH numbered by ascending k', REG i = 0, 1, 2 of unit m' is number (floor(n_id_cell n_l /
 *               n_0) + m' + floor(i n_l / 3)) mod n_l of symbol l = 0 (normal duration) or l = i (extended; needs n_ctrl >= 3)
 *   order       the N_REG other REGs sorted by (k', l'); N_CCE = floor(N_REG / 9); REG i carries quadruplet w((i + n_id_cell) mod
 *               N_REG) of the multiplexed stream, w the sub-block interleaver of 36.212 5.1.4.2.1 on quadruplets (32 columns, the
 *               nulls in front, the PBCH's column permutation); bit j of CCE c is bit 72 c + j of the stream
 *   soft bits   b[2 e] = Re s_e, b[2 e + 1] = Im s_e for the elements e of quadruplets 0 .. 143, times 1 - 2 c(i) of the Gold
 *               sequence with c_init = sf 2^9 + n_id_cell; no noise scaling
 *   candidates  slot s = 0 .. 3: L = 4 from CCE 4 s, while s < min(4, floor(N_CCE / 4)); slot 4, 5: L = 8 from CCE 8 (s - 4), while
 *               s - 4 < min(2, floor(N_CCE / 8))
 *   decoding    per candidate and payload size A (K = A + 16): every coded bit is the SUM of its soft bits among the 72 L (36.212
 *               5.1.4.2 inverted, ascending position); the tail-biting decoder over K steps (the lowest start state among equal
 *               end metrics); rnti_x = CRC-16 of the first A bits ^ the received sixteen, MSB first
 *   accepted    rnti_x = 0xFFFF (rnti_mask bit 0, SI), 0xFFFE (bit 1, paging) or 0x0001 .. 0x003C (bit 2, random-access response).
 *               A silent candidate (every soft bit zero) decodes to all zeros with rnti_x = 0 and is never accepted.
 * dec[g][s][i]: bits = the A payload bits (bit t = the t-th bit sent); flags 1 = decoded, | 2 = accepted; quality = -(the winning
 * end metric) / sum |coded bit|: the decoder MINIMISES the sum of -(+-value), so a noise-free codeword gives +1 and noise values
 * near 0 (0 for a silent candidate).  A slot beyond the subframe's candidates, a subframe that is not read and a candidate with a
 * value that is not finite leave a zero entry.  cfi, n_reg, n_cce: what the subframe was read with (0: not read).  n_read counts the
 * subframes read, n_accepted the accepted entries (a DCI found at L = 4 and L = 8 counts twice), n_si / n_paging / n_ra by kind. */
#define LCS_PDCCH_SLOTS 6
#define LCS_PDCCH_MAX_SIZES 2
typedef struct lcs_pdcch_cfg {            /* zero = take from the cell / defaults */
  int32_t phich_duration, phich_resource; /* 0: the cell's (refused when the cell has none); else as lcs_cell's */
  int32_t phich_mi[10];                   /* m_i of subframe 0 .. 9: 0, 1 or 2; -1: FDD's 1.  A call with any entry >= 0 is a TDD
                                             call: with the extended PHICH duration its subframes 1 and 6 are not read */
  int32_t n_sizes, size[LCS_PDCCH_MAX_SIZES];   /* payload sizes A, 8 .. 48 */
  int32_t rnti_mask;                      /* bit 0 SI, 1 paging, 2 RA; 0 = all three */
  int32_t cfi_force;                      /* 0: the PCFICH's decision per subframe */
} lcs_pdcch_cfg;          /* 68 bytes */
typedef struct lcs_pdcch_dec { uint64_t bits; uint32_t rnti_x; int32_t flags /*1 decoded, 2 accepted*/; double quality; } lcs_pdcch_dec;
typedef struct lcs_pdcch_info {
  int32_t n_sf, n_read, n_accepted, n_si, n_paging, n_ra, dl_mask, n_rb, n_ports, reserved;
  int32_t cfi[LCS_PCFICH_MAX_SF], n_reg[LCS_PCFICH_MAX_SF], n_cce[LCS_PCFICH_MAX_SF];
  lcs_pdcch_dec dec[LCS_PCFICH_MAX_SF][LCS_PDCCH_SLOTS][LCS_PDCCH_MAX_SIZES];
} lcs_pdcch_info;         /* 21640 bytes */

/* The blind search of the whole control region: every CCE of every downlink subframe, at every aggregation level, for the grants
 * the cell gives to its users (lcs_pdcch_scan_wide, lcs_pdcch_scan, lcs_pdcch_scan_decodes below; a stage of its own beside the
 * PDCCH stage, which it leaves as it is).  THE RULE (lte-cell-scanner_amd/csrc/pdcch_scan.h, host and device; everything up to the
 * soft bit as lcs_pdcch_info's, with pdcch.h's functions):
 *   soft bits   of quadruplets 0 .. 9 N_CCE - 1, N_CCE <= 88: 6336 per subframe at most; the first 1152 are lcs_pdcch_info's
 *   candidates  every L in {1, 2, 4, 8} and every first CCE c with c mod L = 0 and c + L <= N_CCE, by L ascending and then c (165 at
 *               most).  At payload size A (K = A + 16) a candidate is formed only if 4 K <= 3 * 72 L (a code rate of 3/4 at most);
 *               otherwise it leaves a zero entry
 *   decoding    coded bit d_b = the sum of its soft bits in ascending position (fp64).  m = max |d_b|; a value that is not finite
 *               leaves a zero entry; m = 0 is a silent candidate: decoded, all zero, never accepted.  q_b = rint(127.0 d_b / m)
 *               (round half to even), -127 .. 127.  From there integers only: a wrap-around Viterbi decoder with int32 path metrics
 *               that start at 0 and are carried through three passes over the K steps; branch metric -sum_j (1 - 2 w_j) q_j;
 *               predecessors 2 j and 2 j + 1 lead to state j + 32 b, the odd one taken only if strictly smaller; decisions kept for
 *               the last pass; end state = the lowest state among the smallest metrics; K steps of traceback
 *   reported    tb_ok: the traced start state equals the end state.  The K bits are re-encoded with the tail-biting code: n_obs =
 *               the coded bits with q_b != 0, n_err = those whose sign disagrees with the re-encoded bit c_b, quality =
 *               sum q_b (1 - 2 c_b) / sum |q_b| (integer sums, one fp64 division).  rnti_x as lcs_pdcch_info's
 *   common      rnti_x is SI, paging or RA per rnti_mask, L in {4, 8}, c < 16: accepted (as lcs_pdcch_info's)
 *   in space    0x003D <= rnti_x <= 0xFFF3 and the candidate lies in that RNTI's search space of the subframe (36.213 9.1.1):
 *               Y_-1 = rnti, Y_k = 39827 Y_(k-1) mod 65537, k = g mod 10; c = L ((Y_k + m') mod floor(N_CCE / L)) for an
 *               m' < M(L) = 6, 6, 2, 2
 *   UE accept   in space, quality >= min_quality, and n_repeat >= min_repeat: n_repeat = the number of distinct subframes of the
 *               call in which the same rnti_x has an in-space decode of that quality, at any size and level
 * flags: 1 decoded, 2 accepted, 4 in space, 8 tb_ok, 16 common kind.  msg[] lists every entry that is in space with quality >=
 * min_quality or an accepted common one, ordered by subframe, L, c and size; entries beyond LCS_PDCCH_SCAN_MAX_MSG are counted in
 * n_dropped and not written.  sf[g]: what the subframe was read with, its candidates, the accepted common and UE entries, and the
 * CCEs that accepted entries cover.  n_rnti counts the distinct RNTIs of accepted UE entries.  Nothing depends on the order in which
 * workgroups run: the list is placed by ordered prefix sums. */
#define LCS_PDCCH_SCAN_MAX_SIZES 6
#define LCS_PDCCH_SCAN_MAX_CCE 88
#define LCS_PDCCH_SCAN_MAX_CAND 165
#define LCS_PDCCH_SCAN_MAX_MSG 1024
#define LCS_PDCCH_SCAN_MIN_QUALITY 0.75   /* what the bindings pass for min_quality when the caller names none */
typedef struct lcs_pdcch_scan_cfg {
  int32_t phich_duration, phich_resource, phich_mi[10];   /* as lcs_pdcch_cfg's */
  int32_t n_sizes, size[LCS_PDCCH_SCAN_MAX_SIZES];        /* payload sizes A, 8 .. 64 */
  int32_t rnti_mask, cfi_force;           /* as lcs_pdcch_cfg's */
  int32_t min_repeat;                     /* >= 1; 2 is the bindings' default, 1 turns the recurrence rule off */
  int32_t reserved[2];                    /* zero */
  double min_quality;                     /* 0 .. 1; the bindings' default is LCS_PDCCH_SCAN_MIN_QUALITY */
} lcs_pdcch_scan_cfg;     /* 104 bytes */
typedef struct lcs_pdcch_scan_dec {
  uint64_t bits;                          /* the A payload bits, bit t = the t-th bit sent */
  uint32_t rnti_x;
  int32_t flags;
  int16_t n_err, n_obs;
  int32_t n_repeat;                       /* of an entry in space with quality >= min_quality, else 0 */
  double quality;
} lcs_pdcch_scan_dec;     /* 32 bytes */
typedef struct lcs_pdcch_scan_msg { int16_t g; uint8_t L, cce, size_index, pad[3]; lcs_pdcch_scan_dec d; } lcs_pdcch_scan_msg;   /* 40 bytes */
typedef struct lcs_pdcch_scan_sf { int32_t cfi, n_reg, n_cce, n_cand, n_common, n_ue; uint32_t cce_mask[3]; } lcs_pdcch_scan_sf;   /* 36 bytes */
typedef struct lcs_pdcch_scan_info {
  int32_t n_sf, n_read, n_accepted, n_si, n_paging, n_ra, dl_mask, n_rb, n_ports, n_ue, n_rnti, n_msg, n_dropped, n_sizes, reserved[2];
  lcs_pdcch_scan_sf sf[LCS_PCFICH_MAX_SF];
  lcs_pdcch_scan_msg msg[LCS_PDCCH_SCAN_MAX_MSG];
} lcs_pdcch_scan_info;    /* 43616 bytes */

/* The PHICH of a wide cell: the HARQ indicators (ACK / NACK of uplink transport blocks) of every downlink subframe of a
 * full-bandwidth grid (lcs_phich_wide, lcs_phich, lcs_phich_values below; a stage of its own beside the others, which it leaves as
 * they are).  THE RULE (lte-cell-scanner_amd/csrc/phich.h, host and device) IS WRITTEN FROM MEMORY OF 36.211 6.9 AND 36.212 5.3.5, NOT
 * FROM THEIR TEXT: what pins it is the generator (synth.phich_region, written from the same memory but as a transmitter), the numpy
 * statement tests/phich_ref.py, and the REG list, which is the PDCCH stage's own (pdc_build_map_t, pinned there).  It needs no CFI:
 *   grid        as lcs_pcfich_info's.  Grid subframe g is read iff its bit of dl_mask is set, the rows of symbol 0 (symbols 0 .. 2
 *               with the extended PHICH duration, symbols 0 and 1 with 4 ports) lie inside n_ofdm, and the PHICH map of m_i of
 *               subframe g mod 10 is not refused (the units do not fit their symbol).  A TDD call is one with any phich_mi >= 0: at
 *               the extended duration its subframes 1 and 6 are not read, as in the PDCCH stage
 *   channel     the PDCCH stage's: symbol 0's reference row for ports 0 and 1, symbol 1's for ports 2 and 3, at the element's
 *               column whatever its own symbol, interpolated as the PCFICH's
 *   units       U = m_i ceil(Ng n_rb / 8) mapping units of three REGs: exactly the `phich` list of pdc_build_map_t (the rule of
 *               lcs_pdcch_info above, line PHICH), called with cfi 3; REG i = 0, 1, 2 of unit m' holds quadruplet i, four elements
 *               in increasing column.  U = 0 is a subframe that is read with nothing in it
 *   groups      normal CP: group n = unit n, N_SF = 4, 8 sequences.  Extended CP: groups 2 m' and 2 m' + 1 share unit m', N_SF = 2,
 *               4 sequences; the even group sits on elements 0, 1 of each quadruplet, the odd one on elements 2, 3
 *   sequences   36.211 table 6.9.1-2.  Normal CP: w = ++++, +-+-, ++--, +--+ for seq 0 .. 3 and j times the same for seq 4 .. 7.
 *               Extended CP: ++, +- for seq 0, 1 and j times the same for seq 2, 3
 *   modulation  HI = 1 (ACK) is 111, HI = 0 (NACK) is 000; BPSK, bit 0 -> (1 + j) / sqrt 2, bit 1 -> -(1 + j) / sqrt 2;
 *               d(i) = w(i mod N_SF) (1 - 2 c(i)) z(floor(i / N_SF)), i < 3 N_SF: repetition r of the indicator lies on quadruplet r.
 *               c is the Gold sequence with the PCFICH's c_init = (sf + 1) (2 n_id_cell + 1) 2^9 + n_id_cell
 *   combining   1 and 2 ports: as the PCFICH's on the pairs (elements 0, 1 and 2, 3) of a quadruplet.  4 ports: quadruplet i of
 *               unit m' goes through ports (0, 2) when i + m' is even and through ports (1, 3) when it is odd, for the WHOLE
 *               quadruplet (not the PDCCH's alternation inside a quadruplet).  The gain of element e is G_e = |h_a(k_e)|^2 +
 *               |h_b(k_e')|^2, e' the other element of its pair (|h(k_e)|^2 with one port); nothing is divided by it
 *   despreading per (group, seq) and repetition r: X = sum_j Re(w_j) or Im(w_j) times (1 - 2 c(i)) s_e over the N_SF elements (a
 *               Hadamard butterfly), a_r = K (Re X + Im X) for a real sequence and K (Im X - Re X) for one with j, K = 1 / sqrt 2
 *               with one port and 1 with two or four; d_r = the sum of G_e over the same elements.
 *               value = (a_0 + a_1 + a_2) / (d_0 + d_1 + d_2): a PHICH planted at the amplitude of one unit-power resource element
 *               reads +1 for NACK and -1 for ACK on a noise-free grid at every port count
 *   noise       per (group, seq), S = sum_r d_r (a_r / d_r - value)^2 (a repetition with d_r = 0 adds nothing): the spread of the
 *               three repetitions around their weighted mean, free of the signal whatever the loading.  noise[g] = the mean of S
 *               over all (group, seq) of the subframe whose d sum is above zero (0 without one: an entry that does not read has
 *               no spread to add); sigma = sqrt(noise[g] / (2 (d_0 + d_1 + d_2))): in white noise S is the element noise power
 *               times a chi-square of 2 degrees of freedom over 2, so value / sigma of a silent entry has unit variance but for
 *               the factor nu / (nu - 2) of a t distribution with nu = 2 N entries of the subframe
 *   decision    present iff |value| >= min_amp and |value| >= min_sigma sigma; a present entry is an ACK iff value < 0.  An entry
 *               whose d sum is zero, or whose value is not finite, is absent with value 0 (sigma 0 too)
 * The order of every sum is fixed in phich.h; plain fp64, so the device and the host twin agree byte for byte.  sf[g]: n_unit (-1: not
 * read; then the other fields are zero), n_group, the counts of present entries and noise[g].  hi[] lists the present entries by (g,
 * group, seq), placed by ordered prefix sums without atomics; those beyond LCS_PHICH_MAX_HI are counted in n_dropped and not
 * written, n_hi are listed.  NOT READ: TDD grant timing (which uplink subframe an indicator answers) and I_PHICH beyond the bindings'
 * argument; subframes 1 and 6 of a TDD cell at the extended duration; MBSFN subframes; nothing of this is in the streaming mode,
 * and the blind search does not use a grant's PHICH as an acceptance condition. */
#define LCS_PHICH_MAX_HI 1024
#define LCS_PHICH_MAX_GROUP 100           /* 25 units x m_i 2, x 2 groups per unit with the extended CP */
#define LCS_PHICH_MAX_ENTRIES 400         /* (group, seq) pairs of a subframe */
#define LCS_PHICH_MIN_AMP 0.25            /* a design floor: a PHICH 12 dB below a reference element is not worth reporting */
#define LCS_PHICH_MIN_SIGMA 3.5           /* measured: tools/phich_accuracy.py, profiles/phich/accuracy.json */
typedef struct lcs_phich_cfg {
  int32_t phich_duration, phich_resource, phich_mi[10];   /* as lcs_pdcch_cfg's */
  int32_t reserved[2];                    /* zero */
  double min_amp, min_sigma;              /* >= 0; the bindings' defaults are LCS_PHICH_MIN_AMP and LCS_PHICH_MIN_SIGMA */
} lcs_phich_cfg;          /* 72 bytes */
typedef struct lcs_phich_sf { int32_t n_unit, n_group, n_present, n_ack, n_nack, reserved; double noise; } lcs_phich_sf;   /* 32 bytes */
typedef struct lcs_phich_hi { int16_t g; uint8_t group, seq; int32_t flags /*1 present, 2 ack*/; double value, sigma; } lcs_phich_hi;   /* 24 bytes */
typedef struct lcs_phich_info {
  int32_t n_sf, n_read, n_present, n_ack, n_nack, n_hi, n_dropped, dl_mask, n_rb, n_ports, reserved[2];
  lcs_phich_sf sf[LCS_PCFICH_MAX_SF];
  lcs_phich_hi hi[LCS_PHICH_MAX_HI];
} lcs_phich_info;         /* 26928 bytes */

/* The PDSCH behind the format 1A grants of that search space: the transport blocks of SI, paging and random-access responses
 * (lcs_pdsch_wide, lcs_pdsch, lcs_turbo_decode below; a stage of its own beside the chain).  THE RULE (lte-cell-scanner_amd/csrc/
 * pdsch.h, host and device; grid, subframes, channel values and combining as for lcs_pcfich_info, the grants as lcs_pdcch_info):
 *   grants      per grid subframe, the accepted entries dec[g][s][i_1a] whose first payload bit is 1 and whose kind is in rnti_mask,
 *               by ascending slot s; the same payload and RNTI found again (L = 4 and L = 8) is one grant; at most two are followed.
 *               The fields are format 1A's (36.212 5.3.3.1.3; the TDD layout iff the PDCCH call is a TDD call).  A grant is decoded
 *               iff distributed = 0, mcs <= 26, every row of its subframe lies inside n_ofdm and, in a TDD call, it is not in
 *               subframe 1 or 6; otherwise it is listed with the status that says why.  Forced grants (n_forced > 0) replace the
 *               PDCCH's: forced[f] = {grid subframe, rnti, rb_start, n_prb, tbs, rv}, slot = f; the CFI is still the subframe's
 *   block size  36.213 7.1.7.2.1: I_TBS = mcs, column N_PRB = 2 if the low TPC bit is 0, else 3; B = tbs + 24, K = the smallest
 *               turbo block size >= B (K = B for every table entry), F = K - B fillers; QPSK, one code block
 *   elements    resource blocks rb_start .. rb_start + n_prb - 1 in both slots, by symbol l = n_ctrl .. 2 n_symb - 1 of the subframe
 *               and then by ascending column, n_ctrl = cfi + (n_rb <= 10); without the reference elements of the cell's ports (one
 *               port: port 0's; two: the columns = n_id_cell (mod 3) of symbols 0 and n_symb - 3 of each slot; four: also of symbol 1
 *               of each slot), without the central 72 columns of symbols 0 .. 3 of slot 1 of subframe 0 (PBCH) and of the PSS / SSS
 *               symbols of subframes 0 and 5 (FDD: the last two symbols of the first slot; TDD: the last symbol of the second)
 *   channel     per port and reference row of the subframe the PCFICH's value at the column; in time linear between the two
 *               reference rows of that port that bracket the symbol inside the subframe, the nearest row's value outside them
 *   soft bits   combining as the PCFICH's on consecutive elements (pairs 2 u, 2 u + 1; four ports: (0, 2), (1, 3) alternating);
 *               b[2 e] = Re s_e, b[2 e + 1] = Im s_e, times 1 - 2 c(i), c_init = rnti 2^14 + sf 2^9 + n_id_cell; G = 2 N_RE of them;
 *               no division by |h|^2, no noise scaling; positive means 0
 *   de-rate-m.  36.212 5.1.4.1 inverted: D = K + 4, 32 columns, the turbo code's column permutation for d0 and d1, pi(k) for d2,
 *               w = v0, then v1 and v2 interlaced, N_cb = K_w, k0 = R (2 ceil(N_cb / (8 R)) rv + 2), nulls (dummies, fillers of d0
 *               and d1) skipped; every position is the SUM of its soft bits in ascending e: the position of rank r among the N
 *               non-nulls counted from k0 takes e = r, r + N, r + 2 N, .. < G.  A block whose 3 (K + 4) values are all zero or not
 *               all finite is not decoded (status LCS_PDSCH_SILENT)
 *   decoding    max-log-MAP on the two 8-state constituents (36.212 5.1.3.2: feedback 1 + D^2 + D^3, parity 1 + D + D^3, the
 *               twelve tail values in the standard's order, QPP interleaver), branch metric 0.5 ((Ls + La) su + Lp sc), plain fp64
 *               sums and maxima, extrinsic = 0.75 (posterior - Ls - La).  The trellis is cut into windows of 32 steps (the last
 *               shorter): a window's starting forward and ending backward metrics are those the same constituent had at that step in
 *               the previous iteration, zeros in the first; step 0 starts in state 0; the last window ends with the metrics of the
 *               three tail steps run back from state 0.  A filler step admits input 0 only.  After every iteration: decisions of
 *               the second constituent's posterior (negative = 1), de-interleaved; CRC24A (0x864CFB) over bits F .. K - 1; stop at a
 *               zero remainder or after max_iter iterations
 * block[]: the grants in (subframe, slot) order, at most LCS_PDSCH_MAX_BLOCKS (n_overflow counts those beyond); payload: the tbs
 * bits after the fillers, MSB first, for status OK and CRC (zeros otherwise); n_iter: the iterations run.  n_si / n_paging / n_ra
 * count the listed blocks by kind, n_status[] by status, n_ok = n_status[LCS_PDSCH_OK].  The transport block sizes and the QPP
 * parameters in pdsch.h are written from memory of the standard: what pins them is said there. */
#define LCS_PDSCH_MAX_BLOCKS 32
#define LCS_PDSCH_MAX_FORCED 4
#define LCS_PDSCH_PAYLOAD 280
#define LCS_PDSCH_N_STATUS 10
enum { LCS_PDSCH_OK = 1, LCS_PDSCH_CRC = 2, LCS_PDSCH_DISTRIBUTED = 3, LCS_PDSCH_MCS = 4, LCS_PDSCH_ROWS = 5, LCS_PDSCH_SPECIAL = 6,
       LCS_PDSCH_SILENT = 7, LCS_PDSCH_BAD_ALLOC = 8 /* an allocation outside the band, or no such block size */,
       LCS_PDSCH_NO_CFI = 9 /* a forced grant in a subframe whose control region was not read */ };
typedef struct lcs_pdsch_grant { int32_t subframe, rnti, rb_start, n_prb, tbs, rv; } lcs_pdsch_grant;
typedef struct lcs_pdsch_cfg {            /* zero = defaults */
  int32_t i_1a;                           /* the index of format 1A's size among the PDCCH configuration's sizes */
  int32_t max_iter;                       /* 1 .. 16; 0 = 8 */
  int32_t rnti_mask;                      /* as lcs_pdcch_cfg's: the kinds that are followed; 0 = all three */
  int32_t n_forced;                       /* 0 .. LCS_PDSCH_MAX_FORCED, at most two per subframe */
  lcs_pdsch_grant forced[LCS_PDSCH_MAX_FORCED];
} lcs_pdsch_cfg;          /* 112 bytes */
typedef struct lcs_pdsch_block {
  int32_t subframe, slot, rnti, kind /*1 SI, 2 paging, 4 RA, 0 none*/, rb_start, n_prb, mcs /*-1: forced*/, rv, tbs, n_re, K, F, n_iter, status;
  uint8_t payload[LCS_PDSCH_PAYLOAD];
} lcs_pdsch_block;        /* 336 bytes */
typedef struct lcs_pdsch_info {
  int32_t n_sf, n_blocks, n_ok, n_si, n_paging, n_ra, n_overflow, dl_mask, n_rb, n_ports;
  int32_t n_status[LCS_PDSCH_N_STATUS];
  lcs_pdsch_block block[LCS_PDSCH_MAX_BLOCKS];
} lcs_pdsch_info;         /* 10832 bytes */

/* Distributed allocations and format 1C (lcs_set_pdsch_alloc, lcs_pdsch_last_alloc below): a setting of the context that the PDSCH
 * calls read; zero = the stage as stated above, in which a distributed 1A grant is listed as LCS_PDSCH_DISTRIBUTED and format 1C is
 * not read.  THE RULE (pdsch.h, host and device; this project's reading of 36.211 6.2.3.2, 36.212 5.3.3.1.3 / .4, 36.213 7.1.6.3 /
 * 7.1.7.2.3 and 36.321 5.3.1, WRITTEN FROM MEMORY OF THE STANDARD; what pins it is said in pdsch.h and DESIGN.md):
 *   gap         N_gap,1 = ceil(n_rb / 2) for n_rb 6 .. 10, 4 for 11, 8 for 12 .. 19, 12 for 20 .. 26, 18 for 27 .. 44, 27 for 45 .. 63,
 *               32 for 64 .. 79, 48 for 80 .. 110; N_gap,2 = 9 for 50 .. 63, 16 for 64 .. 110, none below 50
 *   sizes       N_VRB = 2 min(N_gap, n_rb - N_gap) (gap 1), floor(n_rb / (2 N_gap)) 2 N_gap (gap 2); the interleaving unit N~ = N_VRB
 *               (gap 1), 2 N_gap (gap 2); P = 1 / 2 / 3 / 4 for n_rb <= 10 / 26 / 63 / 110; N_row = ceil(N~ / (4 P)) P; N_null =
 *               4 N_row - N~
 *   map         VRB v: t = v mod N~, o = N~ floor(v / N~), a = 2 N_row (t mod 2) + floor(t / 2), b = N_row (t mod 4) + floor(t / 4).
 *               Even slot: with N_null != 0 and t >= N~ - N_null, r = a - N_row (t odd) or a - N_row + N_null / 2 (t even); with
 *               N_null != 0, t < N~ - N_null and t mod 4 >= 2, r = b - N_null / 2; otherwise r = b.  Odd slot: r <- (r + N~ / 2)
 *               mod N~.  PRB = o + (r < N~ / 2 ? r : r + N_gap - N~ / 2)
 *   1A          (flags bit 0) a grant with the distributed bit set: fields as before; (rb_start, n_prb) from the RIV read with n_rb
 *               are VRBs; rb_start + n_prb > N_VRB gives LCS_PDSCH_BAD_ALLOC; gap 2 iff n_rb >= 50 and the NDI bit is 1
 *   1C          (flags bit 1) the accepted entries at the PDCCH configuration's other size index, 1 - i_1a.  Bits in the order sent:
 *               one gap bit iff n_rb >= 50 (1 = gap 2), the RIV, I_TBS in 5 bits.  N_step = 2 for n_rb < 50, else 4; the RIV is
 *               ceil(log2(v1 (v1 + 1) / 2)) bits wide, v1 = floor(N_VRB,gap1 / N_step); with N' = floor(N_VRB / N_step) of the
 *               indicated gap: L' = floor(RIV / N') + 1, S' = RIV mod N', and if L' + S' > N': L' = N' - L' + 2, S' = N' - 1 - S';
 *               rb_start = N_step S', n_prb = N_step L' (VRBs); RIV >= N' (N' + 1) / 2 gives LCS_PDSCH_BAD_ALLOC.  Always distributed
 *               and QPSK; mcs = I_TBS; tbs = entry I_TBS of 40, 56, 72, 120, 136, 144, 176, 208, 224, 256, 280, 296, 328, 336, 392, 488,
 *               552, 600, 632, 696, 776, 840, 904, 1000, 1064, 1128, 1224, 1288, 1384, 1480, 1608, 1736
 *   1C's rv     format 1C carries none; the block's rv says what was ASSUMED: 0 for paging and RA.  For SI with sfn0 >= 0 (sfn =
 *               (sfn0 + floor(g / 10)) mod 1024, sf = g mod 10): in subframe 5 of an even frame ceil(3 k / 2) mod 4 with k =
 *               floor(sfn / 2) mod 4; otherwise, with si_window = w > 0 and w != 15, the same with k = ((10 sfn + sf) mod w) mod 4.
 *               In every other case 0.  A WRONG ASSUMPTION SHOWS AS STATUS LCS_PDSCH_CRC, not as a wrong payload
 *   grants      per subframe by ascending candidate slot, then size index; a payload accepted at both sizes is two grants, the same
 *               payload, RNTI and size found again (L = 4 and L = 8) is one; still at most two are followed
 *   elements    as above, over the slot's own set of resource blocks: the PRBs of the grant's VRBs in slot 0 for the symbols of the
 *               first slot, those in slot 1 for the second; within a symbol by ascending column over the set.  The exclusions are
 *               unchanged; the central 72 columns cut a resource block in half when n_rb is odd
 * Such a block is listed like any other: rb_start / n_prb are VRBs.  Not read: 1C's rv where sfn0 or the window is unknown or the
 * window is 15 subframes (0 is assumed), TDD special subframes, distributed forced grants (forced grants are localized). */
#define LCS_PDSCH_ALLOC_RB 112
typedef struct lcs_pdsch_alloc_cfg {      /* zero = the stage without distributed allocations and format 1C */
  int32_t flags;                          /* bit 0: follow distributed 1A grants; bit 1: follow format 1C (needs two PDCCH sizes) */
  int32_t sfn0;                           /* the frame number of grid subframe 0, 0 .. 1023; -1: unknown */
  int32_t si_window;                      /* the SI window in subframes, 0 .. 61; 0: unknown */
  int32_t reserved;
} lcs_pdsch_alloc_cfg;    /* 16 bytes */
typedef struct lcs_pdsch_alloc {
  int32_t format /*0: 1A or forced, 1: 1C*/, distributed, gap /*0: N_gap,1; 1: N_gap,2*/, n_gap /*0: localized*/, n_vrb /*n_rb: localized*/,
      n_step, n_prb /*entries of each list; 0 where the allocation was not followed or lies outside N_VRB*/, reserved;
  uint8_t prb[2][LCS_PDSCH_ALLOC_RB];     /* [slot of the subframe][i]: the PRB of VRB rb_start + i */
} lcs_pdsch_alloc;        /* 256 bytes */

/* The redundancy versions of one SI transport block, combined (lcs_pdsch_comb_wide, lcs_pdsch_comb below: the PDSCH stage, then one
 * more decode per group of blocks that repeat a transport block).  THE RULE (lte-cell-scanner_amd/csrc/pdsch_comb.h, host and device,
 * on top of pdsch.h's functions):
 *   members     the listed blocks of the PDSCH record (index < n_blocks) of kind SI whose status is LCS_PDSCH_OK or LCS_PDSCH_CRC: the
 *               blocks whose soft bits were formed and decoded; forced grants with the SI-RNTI count like any other.  Paging and RA
 *               blocks and blocks of any other status never become members
 *   rule 1      (SIB1; on unless no_sib1) members with subframe % 10 == 5; key (tbs, (subframe / 10) % 2); all members of one key, in
 *               block order, form a group; a group takes at most 4 members, a fifth opens the next group of that key
 *   rule 2      (an SI window; on iff si_window > 0, in subframes, 1 .. 61) the members rule 1 did not take, walked in block order: a
 *               member joins the open (the latest) group of its tbs if that group has fewer than 4 members and the member's subframe
 *               minus the group's first member's is below si_window; otherwise it opens a new group for that tbs
 *   listing     groups in the order of their first member, at most LCS_PDSCH_COMB_MAX_GROUPS (n_overflow counts the rest); a group of
 *               one member is listed too
 *   result      n_ok_members: the members of status OK.  If there is one: status LCS_PDSCH_COMB_MEMBER, n_iter 0, the payload of the
 *               first such member, no decode; n_same: how many OK members carry a payload byte-equal to the first OK member's (below
 *               n_ok_members: the content changed inside the group).  Otherwise n_same = 0 and, with at least 2 members, value k of
 *               stream s is 0 + the sum over the members m, in ascending member order, of the member's de-rate-matched value (pdsch.h:
 *               pds_derm_value(llr_m, G_m, N, base(rv_m), rank)); N and rank are those of (K, F), the same for every member since tbs
 *               is part of the key; the members may differ in allocation, n_re, TBS column and mcs.  The silent check (status
 *               LCS_PDSCH_COMB_SILENT, n_iter 0, a zero payload), the windows, the iteration rule, the CRC stop and max_iter are
 *               exactly the stage's: status LCS_PDSCH_COMB_OK or LCS_PDSCH_COMB_CRC, n_iter and payload as for a block.  A single
 *               member of status CRC: LCS_PDSCH_COMB_CRC, n_iter 0, the member's payload
 * rv_mask: bit rv set for every member's rv.  n_status[] counts the listed groups by status. */
#define LCS_PDSCH_COMB_MAX_GROUPS 8
#define LCS_PDSCH_COMB_MAX_MEMBERS 4
#define LCS_PDSCH_COMB_N_STATUS 5
enum { LCS_PDSCH_COMB_MEMBER = 1, LCS_PDSCH_COMB_OK = 2, LCS_PDSCH_COMB_CRC = 3, LCS_PDSCH_COMB_SILENT = 4 };
typedef struct lcs_pdsch_comb_cfg {       /* zero = defaults */
  int32_t si_window;                      /* rule 2: 0 = off, else 1 .. 61 subframes */
  int32_t no_sib1;                        /* 1: rule 1 off */
  int32_t reserved[2];
} lcs_pdsch_comb_cfg;     /* 16 bytes */
typedef struct lcs_pdsch_comb_group {
  int32_t n_members, member[LCS_PDSCH_COMB_MAX_MEMBERS] /* block indices; -1 beyond n_members */, rule /*1, 2*/, tbs, K, F, rv_mask,
      n_ok_members, n_same, n_iter, status, reserved[2];
  uint8_t payload[LCS_PDSCH_PAYLOAD];
} lcs_pdsch_comb_group;   /* 344 bytes */
typedef struct lcs_pdsch_comb_info {
  int32_t n_groups, n_overflow, n_members /* of the listed groups */, n_decoded /* groups whose sum was decoded: OK + CRC with n_iter > 0 */;
  int32_t n_status[LCS_PDSCH_COMB_N_STATUS], reserved[3];
  lcs_pdsch_comb_group group[LCS_PDSCH_COMB_MAX_GROUPS];
} lcs_pdsch_comb_info;    /* 2800 bytes */

/* ---- stage entry points (host buffers in / out) ------------------------------------ */

/* Replaces xcorr_pss -- include/searcher.h:22-41, src/searcher.cpp:389-419
 * (xc_correlate :113-174, xc_combine :263-308, xc_delay_spread :312-347, sp_est :185-221,
 * xc_peak_freq :353-383).  xc_re_im and sp are debug outputs of the reference and may be
 * NULL (raw xc is then never materialised); incoherent may be NULL. */
int lcs_xcorr_pss(lcs_ctx *ctx, const double *capbuf_re_im, uint32_t n_cap,
                  const double *f_search_set, uint16_t n_f, uint8_t ds_comb_arm,
                  double fc_requested, double fc_programmed, double fs_programmed,
                  double *xc_incoherent_collapsed_pow /*[3][9600]*/,
                  int32_t *xc_incoherent_collapsed_frq /*[3][9600]*/,
                  float *xc_incoherent_single /*[3][9600][n_f]*/,
                  float *xc_incoherent /*[3][9600][n_f] or NULL*/,
                  double *sp_incoherent /*[9600]*/,
                  float *xc_re_im /*[3][n_cap-136][n_f][2] or NULL*/,
                  double *sp /*[n_comb_sp*9600] or NULL*/,
                  uint16_t *n_comb_xc, uint16_t *n_comb_sp);

/* Replaces peak_search -- include/searcher.h:44-56, src/searcher.cpp:422-510.
 * Appends up to max_cells records; *n_cells receives the number found. */
int lcs_peak_search(lcs_ctx *ctx, const double *xc_incoherent_collapsed_pow,
                    const int32_t *xc_incoherent_collapsed_frq, const double *Z_th1 /*[9600]*/,
                    const double *f_search_set, uint16_t n_f, double fc_requested,
                    double fc_programmed, const float *xc_incoherent_single, uint8_t ds_comb_arm,
                    lcs_cell *cells, int max_cells, int *n_cells);

/* Replaces sss_detect -- include/searcher.h:59-76, src/searcher.cpp:696-761.  The eight
 * trailing outputs are the reference's "only used for testing" arrays; each may be NULL. */
int lcs_sss_detect(lcs_ctx *ctx, const lcs_cell *cell, const double *capbuf_re_im, uint32_t n_cap,
                   double thresh2_n_sigma, double fc_requested, double fc_programmed,
                   double fs_programmed, lcs_cell *cell_out,
                   double *sss_h1_np_est /*62*/, double *sss_h2_np_est /*62*/,
                   double *sss_h1_nrm_est /*62*2*/, double *sss_h2_nrm_est /*62*2*/,
                   double *sss_h1_ext_est /*62*2*/, double *sss_h2_ext_est /*62*2*/,
                   double *log_lik_nrm /*[168][2]*/, double *log_lik_ext /*[168][2]*/);

/* Replaces pss_sss_foe -- include/searcher.h:79-85, src/searcher.cpp:767-850. */
int lcs_pss_sss_foe(lcs_ctx *ctx, const lcs_cell *cell_in, const double *capbuf_re_im,
                    uint32_t n_cap, double fc_requested, double fc_programmed,
                    double fs_programmed, lcs_cell *cell_out);

/* The PSS-only coarse estimate of lcs_set_foe_unwrap as a stage of its own, in the context's duplex mode and whatever the unwrap
 * setting: *f_coarse in Hz relative to cell->freq, c_re_im = C (2 doubles, or NULL), *n_occ = the occurrences summed (or NULL).
 * Refuses a cell without n_id_1 / n_id_2 / CP type, as lcs_pss_sss_foe does. */
int lcs_pss_foe_coarse(lcs_ctx *ctx, const lcs_cell *cell, const double *capbuf_re_im, uint32_t n_cap,
                       double fc_requested, double fc_programmed, double fs_programmed,
                       double *f_coarse, double *c_re_im /*2, or NULL*/, int *n_occ /*or NULL*/);

/* Replaces extract_tfg -- include/searcher.h:88-98, src/searcher.cpp:857-935.
 * tfg is [n_ofdm][72] row-major; *n_ofdm = 854 (normal CP) or 732 (extended). */
int lcs_extract_tfg(lcs_ctx *ctx, const lcs_cell *cell, const double *capbuf_re_im, uint32_t n_cap,
                    double fc_requested, double fc_programmed, double fs_programmed,
                    double *tfg_re_im, double *tfg_timestamp, int *n_ofdm);

/* Replaces tfoec -- include/searcher.h:101-112, src/searcher.cpp:952-1069.  The RS_DL
 * argument of the reference is a pure function of (n_id_cell, cp_type) and is rebuilt
 * on the device (src/lte_lib.cpp:305-405). */
int lcs_tfoec(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_re_im,
              const double *tfg_timestamp, int n_ofdm, double fc_requested, double fc_programmed,
              double *tfg_comp_re_im, double *tfg_comp_timestamp, lcs_cell *cell_out);

/* Replaces decode_mib -- include/searcher.h:115-119, src/searcher.cpp:1526-1692
 * (chan_est :1369-1477, ce_interp_hex :1223-1362, pbch_extract :1482-1522). */
int lcs_decode_mib(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_re_im, int n_ofdm,
                   lcs_cell *cell_out);

/* What lcs_decode_mib computes for ONE of its twelve candidates before it looks at the CRC, exported so that it can be tested
 * directly: the grid is staged exactly as by lcs_decode_mib, the candidate (frame_timing_guess 0 .. 3, n_ports 1, 2 or 4) is forced.
 * e_est: the descrambled LLRs (1920 with the normal CP, 1728 with the extended; room for 1920), d_est: the de-rate-matched values
 * [3][40], bits40: the decoded word (bit t = c_est(t)), crc_ok: whether its CRC passes under the n_ports mask.  Refuses
 * (LCS_ERR_BAD_ARG, an lcs_last_error text) what lcs_decode_mib refuses, and a candidate outside those values. */
int lcs_pbch_soft(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_comp_re_im, int n_ofdm, int frame_timing_guess, int n_ports,
                  double *e_est, double *d_est, uint64_t *bits40, int *crc_ok);

/* chan_est (src/searcher.cpp:1369-1477 with ce_interp_hex :1223-1362), the first half of decode_mib, as a stage of its
 * own: channel estimate of antenna port `port` on the whole compensated grid and the port's noise power.  Internal to the
 * reference's searcher.cpp (not in searcher.h); exported so that it can be tested directly. */
int lcs_chan_est(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_re_im, int n_ofdm, int port,
                 double *ce_tfg_re_im /*[n_ofdm][72]*/, double *np);

/* The uplink-downlink configuration of a TDD cell as a stage of its own (the rule: lcs_set_tdd_config above), whatever the
 * context's modes: the grid of lcs_extract_tfg, raw or compensated, of a cell with n_id_1, n_id_2 and a CP type.  n_ofdm may be
 * any number of rows from two frames (280 normal CP / 240 extended) to LCS_TFG_MAX_OFDM; a partial last slot counts with the
 * rows it has.  Refuses (LCS_ERR_BAD_ARG, an lcs_last_error text) a cell without identity or CP type and an n_ofdm outside that
 * range. */
int lcs_tdd_config(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_re_im, int n_ofdm, lcs_tdd_info *out);

/* RSRP, RSSI, RSRQ and the noise power as a stage of its own (the rule: lcs_set_cell_meas above), whatever the context's modes, on
 * the grid of lcs_extract_tfg, raw or compensated; the table of the last fused call (lcs_last_cell_meas) stays what it is.
 * n_ofdm as for lcs_tdd_config; a cell whose n_ports is 0 or unknown is measured on port 0 alone.  Refuses (LCS_ERR_BAD_ARG, an
 * lcs_last_error text) a cell without identity or CP type, an n_ofdm outside the range, and a dl_mask that is 0 or has a bit
 * above bit 9. */
int lcs_cell_meas(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_re_im, int n_ofdm, int dl_mask, lcs_meas_info *out);

/* The full-bandwidth grid and measurement (the rule: lcs_meas_wide_info above) on wide samples that are already on the device:
 * d_capbuf holds n_cap complex<float> samples at fs_programmed, 8-byte aligned -- a channel of lcs_channelize at decim = K / R of a
 * K x 1.92 Msps capture, centred on the cell.  lcs_extract_tfg_wide hands out all n_ofdm rows, [n_ofdm][12 n_rb] (re, im) pairs, and
 * their ideal locations (timestamp_out, or NULL); lcs_cell_meas_wide transforms port 0's reference rows only.  Both wait for the
 * context's stream, work whatever the context's modes are and with a stream open, and leave the modes and the last fused call's
 * tables alone; their device buffers are allocated on first use.  They refuse (LCS_ERR_BAD_ARG, an lcs_last_error text), launching
 * nothing: a null pointer or a misaligned buffer; an n_fft that is not 128 {1, 2, 4, 8, 16}; |fs_programmed / (15000 n_fft) - 1| >=
 * 1e-3; an n_rb or n_ofdm outside its range; a dl_mask that is 0 or has a bit above bit 9; a cell without n_id_1, n_id_2 or CP
 * type; and a capture that does not hold every requested row (one starts before sample 0, or round_i(location) + n_fft > n_cap). */
int lcs_extract_tfg_wide(lcs_ctx *ctx, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap,
                         double fc_requested, double fc_programmed, double fs_programmed, int n_fft, int n_rb, int n_ofdm,
                         double *tfg_out_re_im /*host [n_ofdm][12 n_rb][2]*/, double *timestamp_out /*host [n_ofdm] or NULL*/);
int lcs_cell_meas_wide(lcs_ctx *ctx, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap,
                       double fc_requested, double fc_programmed, double fs_programmed, int n_fft, int n_rb, int n_ofdm,
                       int dl_mask, lcs_meas_wide_info *out);

/* The PCFICH (the rule: lcs_pcfich_info above).  lcs_pcfich_wide takes lcs_cell_meas_wide's arguments with its conventions and its
 * refusals, and transforms only the rows it reads: symbol 0 of the first slot of every subframe of the mask, and symbol 1 with 4
 * ports.  lcs_pcfich runs the same stage on a grid from the host, [n_ofdm][12 n_rb] (re, im) pairs, 2 n_symb <= n_ofdm <=
 * 122 n_symb.  Both also refuse an n_rb that is not 6, 15, 25, 50, 75 or 100 and one that contradicts a known cell->n_rb_dl; n_ofdm
 * holds at least one whole subframe.  Like the measurement they work in any mode and with a stream open and leave the modes and
 * the last fused call's tables alone. */
int lcs_pcfich_wide(lcs_ctx *ctx, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap,
                    double fc_requested, double fc_programmed, double fs_programmed, int n_fft, int n_rb, int n_ofdm,
                    int dl_mask, lcs_pcfich_info *out);
int lcs_pcfich(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_wide_re_im /*host [n_ofdm][12 n_rb][2]*/, int n_ofdm, int n_rb,
               int dl_mask, lcs_pcfich_info *out);

/* The PDCCH common search space (the rule: lcs_pdcch_info above).  The two take lcs_pcfich_wide's and lcs_pcfich's arguments, with
 * their conventions and refusals, and a configuration (cfg == NULL is refused: the payload sizes have no default in the library).
 * lcs_pdcch_wide transforms symbols 0 .. 2 (0 .. 3 for n_rb <= 10) of the first slot of every subframe of the mask before the CFI
 * is known; then both run the PCFICH on those rows (unless cfi_force says the CFI), the soft bits of CCE 0 .. 15 and one decode per
 * (subframe, candidate, size), all on the device without a host round trip.  Refused beyond the PCFICH's refusals, with
 * LCS_ERR_BAD_ARG, a text and no launch: a PHICH duration / resource that neither cfg nor the cell says, or outside 1 .. 2 /
 * 1 .. 4; n_sizes outside 1 .. 2 or a size outside 8 .. 48; cfi_force outside 0 .. 3, or one that the extended PHICH duration does
 * not fit (n_ctrl < 3); an m_i outside -1 .. 2; an rnti_mask outside 0 .. 7.  The REG map and the de-rate-matching lists are built
 * on the host once per (n_rb, ports, CP, n_id_cell, PHICH configuration, sizes) and kept in the context.  Isolation as the PCFICH's;
 * the PCFICH decisions go into a record of this stage's own. */
int lcs_pdcch_wide(lcs_ctx *ctx, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap,
                   double fc_requested, double fc_programmed, double fs_programmed, int n_fft, int n_rb, int n_ofdm,
                   int dl_mask, const lcs_pdcch_cfg *cfg, lcs_pdcch_info *out);
int lcs_pdcch(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_wide_re_im /*host [n_ofdm][12 n_rb][2]*/, int n_ofdm, int n_rb,
              int dl_mask, const lcs_pdcch_cfg *cfg, lcs_pdcch_info *out);

/* The blind search of the whole control region (the rule: lcs_pdcch_scan_info above).  The two take lcs_pdcch_wide's and lcs_pdcch's
 * arguments, with their conventions and refusals, and a configuration of their own (cfg == NULL is refused).  The PCFICH (unless
 * cfi_force says the CFI), the soft bits of every CCE, one decode per (subframe, candidate, size) and the acceptance run on the
 * device without a host round trip, in blocks of this stage's own: the records of the PCFICH, PDCCH and PDSCH stages are not
 * touched.  Refused beyond the PDCCH's refusals, with LCS_ERR_BAD_ARG, a text and no launch: n_sizes outside 1 .. 6, a size outside
 * 8 .. 64, min_repeat < 1, a min_quality outside 0 .. 1 or not a number, a non-zero reserved field.  The tables (the REG maps of 792
 * quadruplets, the de-rate-matching lists of every size and level, the scrambling jumps) are built on the host once per key.
 * lcs_pdcch_scan_decodes copies the decode table of grid subframe g of the context's last scan to out: n_cand * n_sizes entries in
 * candidate and size order; it returns their number, or LCS_ERR_BAD_ARG before any scan, for a g outside the scan's subframes or
 * a cap that is too small. */
int lcs_pdcch_scan_wide(lcs_ctx *ctx, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap,
                        double fc_requested, double fc_programmed, double fs_programmed, int n_fft, int n_rb, int n_ofdm,
                        int dl_mask, const lcs_pdcch_scan_cfg *cfg, lcs_pdcch_scan_info *out);
int lcs_pdcch_scan(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_wide_re_im /*host [n_ofdm][12 n_rb][2]*/, int n_ofdm, int n_rb,
                   int dl_mask, const lcs_pdcch_scan_cfg *cfg, lcs_pdcch_scan_info *out);
int lcs_pdcch_scan_decodes(lcs_ctx *ctx, int g, lcs_pdcch_scan_dec *out, int cap);

/* The PHICH (the rule: lcs_phich_info above).  The two take lcs_pdcch_wide's and lcs_pdcch's arguments, with their conventions and
 * the PCFICH's refusals; cfg == NULL means the cell's PHICH configuration, FDD (every m_i 1) and the default thresholds.
 * lcs_phich_wide transforms only the rows the rule reads: symbol 0 of every subframe read, symbol 1 too with 4 ports, symbols
 * 0 .. 2 at the extended duration.  Two kernels, no host round trip.  Refused with LCS_ERR_BAD_ARG, a text and no launch: the PDCCH
 * stage's refusals for the PHICH duration / resource and the m_i; a min_amp or min_sigma that is negative or not finite; a non-zero
 * reserved field.  The unit tables are built on the host once per (n_rb, ports, CP, n_id_cell, PHICH duration and Ng) and kept in
 * the context.  Isolation as the PCFICH's: the blocks are this stage's own, allocated by its first call.
 * lcs_phich_values copies the full table of grid subframe g of the context's last call to out: n_group * n_seq values (n_seq = 8
 * with the normal CP, 4 with the extended), group by group; it returns their number (0 for a subframe that was not read or holds
 * no unit), or LCS_ERR_BAD_ARG before any call, for a g outside the call's subframes or a cap that is too small. */
int lcs_phich_wide(lcs_ctx *ctx, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap,
                   double fc_requested, double fc_programmed, double fs_programmed, int n_fft, int n_rb, int n_ofdm,
                   int dl_mask, const lcs_phich_cfg *cfg, lcs_phich_info *out);
int lcs_phich(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_wide_re_im /*host [n_ofdm][12 n_rb][2]*/, int n_ofdm, int n_rb,
              int dl_mask, const lcs_phich_cfg *cfg, lcs_phich_info *out);
int lcs_phich_values(lcs_ctx *ctx, int g, double *out, int cap);

/* The PDSCH of the common search space's grants (the rule: lcs_pdsch_info above).  The two take lcs_pdcch_wide's and lcs_pdcch's
 * arguments with their conventions and refusals, the stage's configuration (NULL = defaults) and, optionally, a place for the PDCCH
 * record the grants were read from (pdcch_out, or NULL).  lcs_pdsch_wide transforms every row of the subframes of the mask that lie
 * whole inside n_ofdm (and the control symbols of a cut last one); then the PCFICH, the PDCCH, the plan of the grants, the soft bits
 * and the turbo decoder run on the device without a host round trip.  The PCFICH and PDCCH run into records of this stage's own: the
 * PDCCH stage's and the PCFICH stage's blocks are not touched.  Refused beyond the PDCCH's refusals, with LCS_ERR_BAD_ARG, a text
 * and no launch: max_iter outside 0 .. 16; an rnti_mask outside 0 .. 7; i_1a outside the PDCCH configuration's sizes; n_forced
 * outside 0 .. 4; a forced grant outside the grid's subframes or resource blocks, with an rnti outside 1 .. 65535, an rv outside
 * 0 .. 3 or a tbs outside 1 .. 2216; more than two forced grants in one subframe.  The tables (transport block sizes, interleaver
 * parameters, de-rate-matching ranks) are built on the host once per context, a forced grant's when its (K, F) changes. */
int lcs_pdsch_wide(lcs_ctx *ctx, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap,
                   double fc_requested, double fc_programmed, double fs_programmed, int n_fft, int n_rb, int n_ofdm,
                   int dl_mask, const lcs_pdcch_cfg *cfg, const lcs_pdsch_cfg *pdsch_cfg, lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out);
int lcs_pdsch(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_wide_re_im /*host [n_ofdm][12 n_rb][2]*/, int n_ofdm, int n_rb,
              int dl_mask, const lcs_pdcch_cfg *cfg, const lcs_pdsch_cfg *pdsch_cfg, lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out);

/* The same two calls with the redundancy versions combined (the rule: lcs_pdsch_comb_info above).  They take lcs_pdsch_wide's and
 * lcs_pdsch's arguments, fill `out` and the optional pdcch_out exactly as those do, and after the stage's decode group the SI blocks
 * on the device, decode every group that needs it from the sum of its members' soft bits and fill comb_out.  comb_cfg NULL =
 * defaults (rule 1 on, rule 2 off).  Refused beyond those calls' refusals (LCS_ERR_BAD_ARG, a text, no launch): a null comb_out, an
 * si_window outside 0 .. 61, a no_sib1 outside 0 .. 1. */
int lcs_pdsch_comb_wide(lcs_ctx *ctx, const lcs_cell *cell, const void *d_capbuf, uint32_t n_cap,
                        double fc_requested, double fc_programmed, double fs_programmed, int n_fft, int n_rb, int n_ofdm,
                        int dl_mask, const lcs_pdcch_cfg *cfg, const lcs_pdsch_cfg *pdsch_cfg, lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out,
                        const lcs_pdsch_comb_cfg *comb_cfg, lcs_pdsch_comb_info *comb_out);
int lcs_pdsch_comb(lcs_ctx *ctx, const lcs_cell *cell, const double *tfg_wide_re_im /*host [n_ofdm][12 n_rb][2]*/, int n_ofdm, int n_rb,
                   int dl_mask, const lcs_pdcch_cfg *cfg, const lcs_pdsch_cfg *pdsch_cfg, lcs_pdsch_info *out, lcs_pdcch_info *pdcch_out,
                   const lcs_pdsch_comb_cfg *comb_cfg, lcs_pdsch_comb_info *comb_out);

/* The soft bits the last lcs_pdsch_wide / lcs_pdsch call of this context formed for grant slot `which` (0, 1) of grid `subframe` --
 * the subframe's grants in the order of the record's blocks, followed or not --, exported so that they can be tested directly: the
 * first n of the grant's G = 2 n_re.  Refuses (LCS_ERR_BAD_ARG, a text) a null pointer, a subframe or `which` outside the last
 * call's, a slot whose grant was not followed in that call (no grant, or a status other than OK, CRC and SILENT), an n beyond its G,
 * and any call after lcs_turbo_decode, which takes over the stage's job block. */
int lcs_pdsch_last_soft(lcs_ctx *ctx, int subframe, int which, double *llr_out, int n);

/* Distributed allocations and format 1C (the rule: lcs_pdsch_alloc_cfg above).  lcs_set_pdsch_alloc stores the setting that every later
 * lcs_pdsch_wide / lcs_pdsch / lcs_pdsch_comb_wide / lcs_pdsch_comb call of the context reads; NULL or zeros restores the stage
 * without them, whose records are what they were.  Refused (LCS_ERR_BAD_ARG, a text): flags outside 0 .. 3, sfn0 outside -1 .. 1023,
 * si_window outside 0 .. 61, a non-zero reserved field; and, by the PDSCH calls, flags bit 1 with a PDCCH configuration of fewer
 * than two sizes or whose other size (index 1 - i_1a) is not format 1C's for n_rb.  lcs_pdsch_last_alloc says how block `block_index` of the record of the last such call was allocated: a localized
 * block gives the trivial lists.  It refuses a null pointer, an index that is no listed block of the last call, and any call after
 * lcs_turbo_decode. */
int lcs_set_pdsch_alloc(lcs_ctx *ctx, const lcs_pdsch_alloc_cfg *cfg);
int lcs_pdsch_last_alloc(lcs_ctx *ctx, int block_index, lcs_pdsch_alloc *out);

/* The turbo decoder of that rule as a stage of its own: d [3][K + 4] de-rate-matched values (d0, d1, d2; positive means 0), K one
 * of the 127 block sizes up to 2240, F fillers, max_iter 1 .. 16 (0 = 8) -> bits_out [K] (one byte per bit, the fillers zero),
 * the iterations run and whether the CRC24A over bits F .. K - 1 is zero.  A block that is all zero or not all finite is not decoded:
 * n_iter 0, crc_ok 0, bits zero.  Refuses (LCS_ERR_BAD_ARG, a text, no launch) a null pointer, a K that is no block size, F outside
 * 0 .. K - 1 and max_iter outside 0 .. 16. */
int lcs_turbo_decode(lcs_ctx *ctx, const double *d, int K, int F, int max_iter, uint8_t *bits_out, int *n_iter_out, int *crc_ok_out);

/* ---- fused chain ------------------------------------------------------------------- */

/* One capture buffer through the whole chain of the reference's main loop
 * (src/CellSearch.cpp:484-558: xcorr_pss, Z_th1, peak_search, then per peak sss_detect,
 * pss_sss_foe, extract_tfg, tfoec, decode_mib, dropping peaks without SSS / MIB).
 * The buffer stays resident on the device across all stages.  peaks / n_peaks (nullable)
 * receive the raw peak_search list. */
int lcs_search_capbuf(lcs_ctx *ctx, const double *capbuf_re_im, uint32_t n_cap,
                      const double *f_search_set, uint16_t n_f, double fc_requested,
                      double fc_programmed, double fs_programmed,
                      lcs_cell *cells, int max_cells, int *n_cells,
                      lcs_cell *peaks, int max_peaks, int *n_peaks);

/* Batched, device-resident form used by sweeps and by bench.py: n_buf capture buffers of
 * n_cap samples each, ALREADY IN HBM, as complex<float> (fmt 0) or raw RTL-SDR u8 I/Q
 * bytes (fmt 1; (x-127)/128 is applied on the device, src/capbuf.cpp:172-181).
 * fc_requested / fc_programmed are per buffer (host arrays, n_buf).  cells is
 * [n_buf][max_cells_per_buf] on the host; n_cells [n_buf].  stage_mask selects how far the
 * chain runs: 1 = PSS correlation + peak_search only (BASELINE config 2), 3 = full chain. */
#define LCS_FMT_C64 0
#define LCS_FMT_IQ_U8 1
#define LCS_FMT_C128 2      /* complex<double>: lcs_track_cut only (the batch entry points take LCS_FMT_C64 / LCS_FMT_IQ_U8) */
#define LCS_STAGE_PSS 1
#define LCS_STAGE_FULL 3
int lcs_search_batch_dev(lcs_ctx *ctx, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap,
                         const double *f_search_set, uint16_t n_f, const double *fc_requested,
                         const double *fc_programmed, double fs_programmed, int stage_mask,
                         lcs_cell *cells, int max_cells_per_buf, int *n_cells);

/* The same for buffers in HOST memory (copied to the device by the call): what a caller holding recorded
 * capbuf_NNNN.it files or dongle bytes uses.  RTL-SDR captures are exactly (u8-127)/128 (src/capbuf.cpp:172-181):
 * handing them over as LCS_FMT_IQ_U8 moves 8x fewer bytes than complex<double> and takes the int8 correlation
 * kernel.  lcs_batch_enqueue_host returns as soon as the copy and the kernels are queued (results: lcs_batch_collect);
 * used round-robin over two or three contexts the PCIe transfer of batch i + 1 runs under the kernels of batch i.
 * The copy is a DMA straight from the caller's memory when that memory is page-locked (lcs_host_alloc); any other
 * pointer is staged through pinned slots inside the call (correct, but bounded by a CPU memcpy). */
int lcs_search_batch_host(lcs_ctx *ctx, const void *h_capbufs, int fmt, int n_buf, uint32_t n_cap,
                          const double *f_search_set, uint16_t n_f, const double *fc_requested,
                          const double *fc_programmed, double fs_programmed, int stage_mask,
                          lcs_cell *cells, int max_cells_per_buf, int *n_cells);
int lcs_batch_enqueue_host(lcs_ctx *ctx, const void *h_capbufs, int fmt, int n_buf, uint32_t n_cap,
                           const double *f_search_set, uint16_t n_f, const double *fc_requested,
                           const double *fc_programmed, double fs_programmed, int stage_mask);
/* Page-locked host memory for capture buffers (freed with lcs_host_free before the context is destroyed). */
int lcs_host_alloc(lcs_ctx *ctx, size_t bytes, void **out);
int lcs_host_free(lcs_ctx *ctx, void *p);
/* Device memory for callers that have no HIP toolchain of their own (the host tools are plain g++): buffers they hand to the
 * device-resident entry points (lcs_batch_enqueue, lcs_track_block with td_on_device, lcs_track_stream_block). */
int lcs_device_alloc(lcs_ctx *ctx, size_t bytes, void **out);
int lcs_device_free(lcs_ctx *ctx, void *p);
int lcs_device_upload(lcs_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);      /* synchronous host -> device copy */
/* Number of usable GPUs (0 without one): a sweep driver creates one context per device and shards the carriers
 * (host/CellSearch.cpp -g all; src/CellSearch.cpp:471-569 is the loop being sharded). */
int lcs_device_count(void);

/* Enqueue-only variant for timing: same work, results stay on the device until
 * lcs_batch_collect.  Between enqueue and collect nothing synchronises with the host.
 * The caller's device buffers must stay valid and unchanged until lcs_batch_collect has returned: u8 buffers are
 * converted by the first kernel of the chain, complex<float> buffers (even n_cap, 16-byte aligned) are read IN PLACE by
 * the SSS / FOE / grid stages as well -- the library keeps no float copy of them (lcs_batch_collect drops the reference
 * to them when it returns).  lcs_batch_collect copies only what the batch found: the records are compacted on the device,
 * and one small copy into page-locked memory of the context brings them over (no allocation inside the call). */
int lcs_batch_enqueue(lcs_ctx *ctx, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap,
                      const double *f_search_set, uint16_t n_f, const double *fc_requested,
                      const double *fc_programmed, double fs_programmed, int stage_mask);
int lcs_batch_collect(lcs_ctx *ctx, lcs_cell *cells, int max_cells_per_buf, int *n_cells);
/* Host time (microseconds) the last lcs_batch_collect of the context spent OUTSIDE its wait for the GPU: queueing the copy
 * and scattering the records into the caller's array (bench.py reports it as host_ms_per_batch.collect_excl_wait). */
int lcs_last_collect_host_us(lcs_ctx *ctx, double *us);
/* Counters of the last collected batch: stats[0] = records returned, [1] = 1 if a buffer overflowed LCS_MAX_PEAKS, [4] = cells the
 * last per-cell round took, [5] = peaks of the whole batch that passed sss_detect (the cells carried into extract_tfg .. decode_mib),
 * [6] = cells skipped as already tracked (streaming mode), [7] = PBCH candidates (frame timing x port count, 12 per cell:
 * src/searcher.cpp:1547, :1567) actually decoded -- the reference stops at the first candidate that passes, the batch kernel skips
 * a candidate whose cell already shows an earlier pass. */
int lcs_last_batch_stats(lcs_ctx *ctx, int stats[8]);
/* Debug readback of the last batch (after lcs_batch_collect / lcs_search_batch_*): the xcorr_pss outputs of
 * buffer `buf` in the layouts of lcs_xcorr_pss, plus the detection threshold Z_th1 (src/CellSearch.cpp:500-503).
 * Every pointer may be NULL.  This is how the tests pin the batched kernels to the oracle array by array. */
/* Batches on the int8 kernel with two or more combining windows are SCREENED (on by default): the correlation runs two of the
 * template integers' three base-256 digits over every lag tile, and all three only over the tiles in which a collapsed power can
 * reach the buffer's theta -- the smallest value that an entry which reaches the Z_th1 of its own lag can have -- by a
 * data-independent bound on what the dropped digit changes.  The records a batch returns are the unscreened batch's, byte for byte.  The debug arrays are completed on demand: the first lcs_batch_readback,
 * lcs_last_frq_repairs or lcs_last_frq_repair_stats after a screened batch runs the three-digit kernel over every tile of the
 * context's own int8 copies (valid until the next enqueue), the full collapse and the full repair, and then answers with exactly
 * what a batch without the screen leaves -- the cost lands on that debug call, never on enqueue or collect.
 * The screen pays while few tiles are flagged (two digit passes over everything + three over the flagged tiles against three over
 * everything: break-even near a quarter).  A collected batch that flagged more than a fifth of its tiles -- a busy band -- makes the
 * context's next 63 batches run unscreened before one is screened again; lcs_set_batch_screen forgets that count. */
int lcs_set_batch_screen(lcs_ctx *ctx, int on);
int lcs_get_batch_screen(const lcs_ctx *ctx, int *on);
/* Of the last collected batch: stats[0] = lag tiles (512 lags of one buffer) flagged for the three-digit kernel, [1] = tiles in
 * all, [2] = work items (tile x template group) that kernel ran, [3] = buffers that flagged everything because no usable bound
 * exists for them (a silent buffer).  All 0 for a batch that was not screened.  The numbers arrive with the collect's header copy. */
int lcs_last_screen_stats(lcs_ctx *ctx, int stats[4]);
int lcs_batch_readback(lcs_ctx *ctx, int buf, float *xc_incoherent_single /*[3][9600][n_f]*/,
                       double *xc_incoherent_collapsed_pow /*[3][9600]*/, int32_t *xc_incoherent_collapsed_frq /*[3][9600]*/,
                       double *sp_incoherent /*[9600]*/, double *z_th1 /*[9600]*/);
/* xc_incoherent_collapsed_frq is an integer output of the reference (include/searcher.h:31): the first maximum over the
 * hypotheses of float values which the matrix-core kernels reproduce to ~1e-7, not to the bit.  Positions whose best two
 * hypotheses lie within 4e-6 (relative) of each other are therefore recomputed in the reference's own arithmetic (fp64
 * accumulation in tap order -> complex<float> -> float running sum over the windows -> float box filter, src/searcher.cpp:
 * 160-169, 299-305, 329-345) and decided with its strict comparison (:374): a few positions per buffer, rewritten in place
 * (index and power) before the peak search reads them.  *n_positions = how many the last correlation call of the context
 * repaired (all buffers of the batch).  lcs_search_capbuf and the streaming mode hand out no arrays, only peaks and cells: they
 * repair only the near-ties whose power reaches their position's threshold Z_th1 (a peak's power does, src/searcher.cpp:449) --
 * the peak list is exact all the same, and the latency of the repair stays off the single-buffer path.  lcs_foe_partial does not
 * repair (a near-tie may span two ranks' shares): lcs_foe_contend / lcs_foe_resolve settle those after the all-reduce. */
int lcs_last_frq_repairs(lcs_ctx *ctx, int *n_positions);
/* The repair's work is bounded: real captures list ~2 positions per buffer, but a degenerate input (duplicated entries of
 * f_search_set make every position an exact tie) lists all 3 x 9600.  Once a call lists more than 32 positions per repair
 * workgroup (2048 for up to eight buffers, 16384 for a 128-buffer batch) only positions whose power reaches their Z_th1 -- the ones a peak can
 * come from -- are recomputed, and each workgroup stops after 256 candidates; *n_unrepaired counts the listed positions left with
 * the correlation kernel's own arg-max (0 on any real data; for exact duplicates that arg-max is the reference's anyway:
 * identical templates give identical values and the first one wins). */
int lcs_last_frq_repair_stats(lcs_ctx *ctx, int *n_listed, int *n_unrepaired);
/* The relative margin below which the two best hypotheses of a position count as a near-tie and are listed for the repair.  The
 * listing catches every position where the correlation kernels could order two hypotheses differently from the reference iff every
 * compared value lies within HALF this margin (relative) of the reference's: the bound the test suite asserts on
 * xc_incoherent_single, the array the compared box-filter means are formed from. */
double lcs_frq_tie_eps(void);
/* HIP-event time (ms) of the PSS correlation kernel launches of the last enqueue, and the
 * number of launches it covers; used by bench.py for the roofline figure. */
int lcs_last_xcorr_ms(lcs_ctx *ctx, float *ms, int *n_launches);
/* Which correlation kernel the last enqueue launched and the matrix-core operations (2 x multiply-accumulates,
 * padding included) those launches executed -- 0 when the kernel does not count them.  For bench.py's
 * roofline.frac_executed. */
int lcs_last_xcorr_info(lcs_ctx *ctx, double *executed_ops, const char **kernel);
/* ---- one capture buffer, frequency hypotheses split over GPUs ("latency mode") ----------------------------
 * a1 / a3 / a4 (src/searcher.cpp:113-347) are independent per hypothesis; the hypotheses meet only where xc_peak_freq takes
 * the maximum over the frequency axis (:369-382).  Every rank calls lcs_foe_partial with the whole f_search_set and its
 * contiguous share [f_first, f_first + f_count) (f_count may be 0); d_words (DEVICE memory of the caller, 3 x 9600 int64)
 * receives, per position, (bits(pow as float) << 32) | (0xFFFFFFFF - global hypothesis index): non-negative floats order
 * like their bit patterns and the complemented index makes the LOWEST hypothesis win a tie, as the reference's strict > does
 * (:374).  d_meta (DEVICE, 9601 doubles) receives sp_incoherent and n_comb_xc.  The caller all-reduces d_words with MAX
 * (RCCL: ncclMax on int64) and broadcasts rank 0's d_meta, both in place on the device, then every rank calls
 * lcs_foe_finish with the reduced buffers: peak_search runs identically everywhere; sss_detect .. decode_mib run for the
 * peaks whose winning hypothesis the rank owns (only it holds the xc_incoherent_single slice the refinement of `ind`
 * reads, :457-465).  cells / order: the rank's decoded cells and their positions in the peak list -- the caller gathers
 * them and sorts by `order` to get the reference's list.  peaks (nullable): the whole peak list; entries won by another
 * rank have ind = -1 and reserved = 1. */
int lcs_foe_partial(lcs_ctx *ctx, const double *capbuf_re_im, uint32_t n_cap, const double *f_search_set, uint16_t n_f,
                    int f_first, int f_count, double fc_requested, double fc_programmed, double fs_programmed,
                    void *d_words /*device int64[3][9600]*/, double *d_meta /*device double[9601]*/);
int lcs_foe_finish(lcs_ctx *ctx, const void *d_words, const double *d_meta, const double *f_search_set, uint16_t n_f,
                   lcs_cell *cells, int32_t *order, int max_cells, int *n_cells, lcs_cell *peaks, int max_peaks, int *n_peaks);
/* The exact index under the split (round 5), between the all-reduce of d_words and lcs_foe_finish:
 *   lcs_foe_contend(ctx, f_search_set, n_f, d_words [reduced], d_words2 [device int64[3][9600], out])
 *   MAX all-reduce of d_words2
 *   lcs_foe_resolve(ctx, d_words, d_words2)
 * A rank contends for a position when a hypothesis of its own other than the global winner lies within 4e-6 (relative) of the
 * global maximum; it recomputes its contenders and the winner in the reference's arithmetic (see lcs_last_frq_repairs) and packs
 * the exact first maximum into d_words2 (-1 where it does not contend).  After the second all-reduce and lcs_foe_resolve the words
 * -- index and power -- are the reference's at every near-tie, identically for every world size and every split of the grid.
 * Without these two calls the index is exact except at near-ties (the rounds before). */
int lcs_foe_contend(lcs_ctx *ctx, const double *f_search_set, uint16_t n_f, const void *d_words, void *d_words2);
int lcs_foe_resolve(lcs_ctx *ctx, void *d_words, const void *d_words2);

/* ---- streaming mode: LTE-Tracker's searcher thread (src/searcher_thread.cpp:83-246) ----------
 * One 80 ms capture buffer at a time, a single frequency hypothesis (the tracked frequency offset,
 * :97-98), cells whose identity is already tracked are reported as re-detected and not decoded again
 * (:157-177).  lcs_stream_open captures the whole chain as a hipGraph (twice: one graph per pinned input slot);
 * lcs_stream_push copies the HOST buffer (fmt LCS_FMT_C64: n_cap complex<float>, LCS_FMT_IQ_U8: 2*n_cap bytes) into
 * pinned memory and replays the graph asynchronously -- up to TWO buffers may be in flight, so the host fills and
 * launches buffer i + 1 while buffer i is on the GPU; lcs_stream_collect waits for the OLDEST buffer in flight and
 * returns its NEW cells (SSS and MIB decoded; one record per identity -- the first decoded peak in peak order, as the reference's
 * loop keeps it: it appends a decoded cell to the tracked list at once, :233-236, so later peaks of the same identity in the same
 * buffer count as seen again), the number of tracked cells seen again and the GPU time of the pass.
 * frame_start is in samples of the pushed buffer; the tracker's 1.92 MHz time base is
 * frame_start*(FS_LTE/16)/(fs_programmed*k_factor) + capture latency (:224).
 * While a stream is open the captured graph holds the context's workspace addresses: any other call on the
 * same context that would need a larger workspace (more buffers, a longer n_cap, more hypotheses) fails with
 * LCS_ERR_BAD_ARG until lcs_stream_close; use a second context for such work. */
int lcs_stream_open(lcs_ctx *ctx, int fmt, uint32_t n_cap, double fc_requested, double fc_programmed,
                    double fs_programmed);
int lcs_stream_push(lcs_ctx *ctx, const void *samples, double f_off, const int16_t *tracked_n_id_cell, int n_tracked);
int lcs_stream_collect(lcs_ctx *ctx, lcs_cell *cells, int max_cells, int *n_cells, int *n_redetected, float *gpu_ms);
int lcs_stream_close(lcs_ctx *ctx);

/* ---- LTE-Tracker's per-symbol pipeline on blocks of OFDM symbols (src/tracker_thread.cpp:823-1068) ------------
 * The reference tracks every detected cell with a thread that takes one OFDM symbol at a time: get_fd (:91-174), the
 * cell-specific reference symbols, filter_ce (:176-201) with its power measurements (:906-931), the frequency and
 * timing measurements of do_foe (:203-243) and do_toe_v2 (:245-288), interp2d (:383-477) and the MIB re-decode
 * (pbch_extract_rt :494-529, do_mib_decode :531-749).  lcs_track_block does that work for a BLOCK of n_sym
 * consecutive symbols (starting at slot 0 symbol 0 of a frame) of n_cells tracked cells at once.
 *   td            [n_cells][n_sym][128] complex<double>: the samples the producer thread queues per symbol
 *                 (src/producer_thread.cpp:196-246), in host memory or (td_on_device != 0) already in HBM
 *   freq_off, frame_timing, late [n_cells][n_sym]: the capture metadata queued with every symbol (host)
 *   cells         identity of each tracked cell; bulk_phase_offset is get_fd's running phase, in before / out after
 * Outputs (host; NULL = not wanted):
 *   syms          [n_cells][n_sym][72] complex: get_fd's output
 *   ce, ce_pw     [n_cells][4][n_sym][72] complex channel estimate and [n_cells][4][n_sym][4] (tp, sp, sp_raw, np) after
 *                 interp2d, valid for symbols < ce_upto[cell][port]
 *   meas          [n_cells][4][max_rs][LCS_TRK_MEAS]: per filtered reference symbol: symbol index, np, tp, sp_raw, sp,
 *                 frequency_offset + residual_f, residual_f_np (what do_foe feeds its recurrence, :235-242),
 *                 rs_curr.frame_timing + delay, delay_np (do_toe_v2, :283-287); n_meas [n_cells][4] rows filled
 *   mib_ok        [n_cells][max_off]: one decode attempt per frame offset o (frames o..o+3 of the block): bit 0 = CRC
 *                 matches, bit 1 = bandwidth / PHICH fields equal the tracked cell's (lock test of :689-694 = both), -1 = not
 *                 attempted (no channel estimate that far into the block); mib_bits: the 40 decoded bits, bit i = c_est(i)
 * The scalar recurrences those results feed (global frequency offset, frame timing, the mib_decode_failures counter)
 * stay with the caller (lte-cell-scanner_amd/tracker.py). */
typedef struct lcs_track_cell {
  int32_t n_id_1, n_id_2, cp_type, n_ports, n_rb_dl, phich_duration, phich_resource, reserved;
  double bulk_phase_offset;
} lcs_track_cell;
#define LCS_TRK_MEAS 9
int lcs_track_block(lcs_ctx *ctx, lcs_track_cell *cells, int n_cells, int n_sym, const void *td, int td_on_device,
                    const double *freq_off, const double *frame_timing, const double *late, double fc_requested,
                    double fc_programmed, double fs_programmed, double *syms, double *ce, double *ce_pw, int32_t *ce_upto,
                    double *meas, int max_rs, int32_t *n_meas, int32_t *mib_ok, uint64_t *mib_bits, int max_off, float *gpu_ms);

/* The producer thread's symbol extraction on the device (src/producer_thread.cpp:96-131, 196-246).  LTE-Tracker's producer stamps
 * every sample of the dongle's stream with a time on the cell-independent 1.92 MHz time base -- sample n of a buffer whose first
 * sample has timestamp ts_first: WRAP(ts_first + n step, 0, 19200), step = (FS_LTE/16) / (fs_programmed k_factor), k_factor =
 * (fc_requested - freq_off) / fc_programmed (:99, :127-131) -- and, per tracked cell, starts a 128-sample capture at the first sample
 * behind the previous capture whose tdiff = WRAP(timestamp - (frame_timing + target), -9600, 9600) satisfies |tdiff| < 0.5 or
 * 0 < tdiff < 3 (:203-213); target = 10 (normal CP) / 32 (extended) for slot 0 symbol 0, advancing by 137 / 138 / 160 per symbol
 * (:236-241); tdiff at that sample is the symbol's `late`.  lcs_track_cut does this for n_cells cells on ONE capture buffer that is
 * already in HBM -- 0.3 MB of dongle bytes per 80 ms instead of 2 KB per symbol and cell over PCIe -- and leaves the symbols where
 * lcs_track_block (td_on_device = 1) and lcs_track_stream_block read them:
 *   d_capbuf      DEVICE memory, n_cap samples: LCS_FMT_IQ_U8 (2 bytes per sample, (u8 - 127) / 128 as :121-124), LCS_FMT_C64,
 *                 LCS_FMT_C128
 *   ts_first      timestamp of the buffer's first sample (0 for a buffer cut from its start)
 *   cp_type, frame_timing, freq_off [n_cells] (host): the values in force while the buffer was recorded
 *   sym_first, pos_first [n_cells] (host; NULL = zeros): the first symbol to cut, counted from slot 0 symbol 0 of the stream's first
 *                 frame, and the sample of THIS buffer its search starts at
 *   d_td          DEVICE memory [n_cells][n_sym][128] complex<double>; rows from n_cut[cell] on are zero
 *   late          host [n_cells][n_sym] (may be NULL); n_cut [n_cells]: symbols found before the buffer ends (<= n_sym);
 *                 pos_next [n_cells] (may be NULL): the sample behind the last capture
 * A stream longer than one buffer: hand over the next buffer starting o samples into this one (o <= the smallest pos_next, so that a
 * capture the buffer's end cut off is whole in the next one) with ts_first' = WRAP(ts_first + o step, 0, 19200), sym_first' =
 * sym_first + n_cut, pos_first' = pos_next - o -- the producer's state between two blocks of samples, with the frame_timing and
 * frequency offset then in force.
 * Sample for sample what the host cutters produce (lte-cell-scanner_amd/tracker.py cut_symbols, host/TrackCells.cpp): the
 * window's position is known in closed form, the predicate itself is evaluated in the same double arithmetic on the candidates. */
int lcs_track_cut(lcs_ctx *ctx, const void *d_capbuf, int fmt, uint32_t n_cap, double ts_first, int n_cells, const int32_t *cp_type,
                  const double *frame_timing, const double *freq_off, const int64_t *sym_first, const int64_t *pos_first,
                  double fc_requested, double fc_programmed, double fs_programmed, int n_sym, void *d_td, double *late, int32_t *n_cut,
                  int64_t *pos_next);

/* Display statistics of the tracker thread for the block the LAST lcs_track_block call on this context processed (same
 * n_cells, n_sym; its symbols and raw reference-signal estimates are read from the workspace, nothing is recomputed):
 *   ac_fd   [n_cells][4][max_rs][12] complex: do_ac_fd (src/tracker_thread.cpp:318-341): autocorrelation over the 12 raw
 *           estimates of reference symbol row + 1 of the port (row = row of `meas`), divided by its signal power -- the
 *           value the reference then folds into tracked_cell.ac_fd with weight 1 / ac_fd_np (:335-338)
 *   ac_td   [n_cells][4][max_rs][72] complex: do_ac_td (:343-371): this_xc of the row against the 71 reference symbols
 *           before it, from row 71 on (NaN before: the reference's 72-deep history is not full)
 *   sync    [n_cells][max_hf][4] = (tp, sp, np, np_blank), sync_ce [n_cells][max_hf][72] complex: do_pss_sss_sigpower_ce
 *           (:754-820) of the k-th PSS/SSS pair of the block; n_hf [n_cells] pairs found
 * The running averages (ac_fd, ac_td, sync_*_av) are scalar recurrences and stay with the caller (tracker.py).
 * NULL = not wanted. */
int lcs_track_stats(lcs_ctx *ctx, int n_cells, int n_sym, double *ac_fd, double *ac_td, int max_rs, double *sync, double *sync_ce,
                    int max_hf, int32_t *n_hf);

/* Continuous form of lcs_track_block for callers that deliver a tracked cell's symbols block after block, as the reference's
 * producer thread does (src/producer_thread.cpp:196-246 -> the per-cell fifo read at src/tracker_thread.cpp:823-1068).  The
 * first call of a stream starts at slot 0 symbol 0 of a frame; every later call continues where the previous one ended
 * (any n_sym >= 1, the same cells in the same order).  Nothing is lost at the cut: the three-symbol window of filter_ce
 * (:176-201), the interpolation between filtered reference symbols (:383-477), the 72-deep history of do_ac_td (:343-371)
 * and the four-frame PBCH fifo (:552-745) all see the previous blocks' symbols, because the context carries the last 3-4
 * frames -- as frequency-domain rows (get_fd's output) on the device -- in front of the new symbols and runs the same
 * kernels over both (so every row is bit-identical to what ONE lcs_track_block call over the whole stream returns); the
 * carried frames are not transformed again, and frame offsets an earlier call attempted are not decoded again.  A call that
 * fails leaves the stream where it was.  Every output row is handed out exactly once, by the first call that can compute it,
 * under its index in the whole stream:
 *   syms      [n_cells][n_sym][72]: get_fd of the symbols of this call
 *   meas, ac_fd, ac_td [n_cells][4][max_rs][9 | 12 | 72 complex]: the filtered reference symbols that became available (a
 *             reference symbol's filter needs the NEXT one, so the last one of a block arrives with the next call); n_meas
 *             [n_cells][4] rows; meas[.][0] is the symbol index counted from the start of the stream
 *   ce, ce_pw [n_cells][4][ce_cap][72 complex | 4]: row r = symbol ce_from[cell][port] + r of the stream, ce_n rows
 *   mib_ok, mib_bits [n_cells][max_off]: entry k = frame offset mib_from[cell] + k of the stream (frames o..o+3), n_mib entries
 * cells[].bulk_phase_offset: in at the first call, out after every call.  td may be ordinary host memory, page-locked host
 * memory (lcs_host_alloc: DMA'd in place) or device memory (the kind is detected).  LIFETIME: page-locked and device memory
 * are copied asynchronously -- td must stay valid and unchanged until the call returns (the call synchronises with its stream
 * before it returns, so nothing of td is referenced afterwards); layout [n_cells][n_sym][128] complex<double>, rows exactly
 * n_sym * 128 elements apart.  lcs_track_stream_reset forgets the
 * stream (the next call starts a new one).  The PSS/SSS statistics (do_pss_sss_sigpower_ce) have no state across symbols
 * and stay with lcs_track_stats. */
int lcs_track_stream_block(lcs_ctx *ctx, lcs_track_cell *cells, int n_cells, int n_sym, const void *td, const double *freq_off,
                           const double *frame_timing, const double *late, double fc_requested, double fc_programmed,
                           double fs_programmed, double *syms, double *ce, double *ce_pw, int ce_cap, int64_t *ce_from, int32_t *ce_n,
                           double *meas, double *ac_fd, double *ac_td, int max_rs, int32_t *n_meas, int32_t *mib_ok,
                           uint64_t *mib_bits, int max_off, int64_t *mib_from, int32_t *n_mib);
int lcs_track_stream_reset(lcs_ctx *ctx);

/* ---- wideband channelizer: one SDR capture in HBM feeds a whole band search ----------------
 * A digital down-converter per carrier (mix, low-pass, decimate) in front of lcs_batch_enqueue: ONE wideband capture x[n] at
 * fs_in = decim * fs_out (2 <= decim <= 16) resident in HBM becomes n_ch narrowband buffers at fs_out, the batch layout
 * LCS_FMT_C64 of lcs_batch_enqueue.  Output k is, exactly ("valid" mode, nothing is zero-padded, T = 16 * decim),
 *
 *   y_k[m] = sum_{t=0}^{T-1} h[t] * x[m*decim + T-1-t] * exp(-2 pi i * f_shift[k] / fs_in * (m*decim + T-1-t)),  m = 0 .. n_out-1
 *
 * with the fixed low-pass h[t] = sinc((t - (T-1)/2) / decim) * kaiser(T, beta = 7.75)[t], normalised to sum(h) = 1 (computed in
 * double, handed to the device as float): at fs_out = 1.92 Msps the passband |f| <= 0.66 MHz ripples by <= 0.0034 dB and
 * everything that aliases into it (|f| >= 1.26 MHz) is down by 71.5 dB (decim 2), 75.6 dB (3), >= 78 dB (4 .. 16).  The carrier
 * phase is kept in 64-bit fixed point (2^64 = one turn), so sample 2.4 M of an 80 ms capture is as exact as sample 0.
 *   d_wide   DEVICE, n_in samples of fmt: LCS_FMT_C64, LCS_FMT_IQ_S8 (interleaved signed 8-bit, value v / 128) or
 *            LCS_FMT_IQ_S16 (interleaved signed 16-bit, value v / 32768), aligned to one sample
 *   f_shift  HOST [n_ch], Hz: carrier centre minus capture centre, |f_shift| <= fs_in / 2
 *   d_out    DEVICE [n_ch][n_out] complex<float>, 16-byte aligned; n_in >= (n_out - 1) * decim + 16 * decim
 * The kernels are queued on the context's stream and the call returns without waiting for them: an lcs_batch_enqueue on the
 * same context that reads d_out is ordered behind them.  d_wide and d_out stay the caller's.  LCS_ERR_BAD_ARG (with an
 * lcs_last_error text) for a null pointer, decim outside 2..16, n_ch < 1, a capture too short for n_out, a shift beyond
 * fs_in / 2, an unknown fmt or a misaligned buffer; nothing is launched then.  fp32 matrix cores, fp32 accumulation: within
 * 1e-5 of the largest output of a channel against the sum evaluated in double. */
#define LCS_FMT_IQ_S8 3
#define LCS_FMT_IQ_S16 4
/* ctx-free, like the lcs_table_* accessors: the T = 16 * decim taps h[t] */
int lcs_channelizer_taps(int decim, double *taps /*[16*decim]*/);
int lcs_channelize(lcs_ctx *ctx, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int decim,
                   const double *f_shift, int n_ch, void *d_out, uint32_t n_out);
/* The same stage at a rational rate change, for front ends that do not run at a multiple of 1.92 Msps (HackRF 10 / 20 Msps,
 * Airspy 2.5 / 6 / 10, SDRplay 6 / 8 / 10, a dongle at 2.048 / 2.4 / 2.56): fs_out = fs_in * up / down, gcd(up, down) = 1.  It is
 * lcs_channelize applied to the capture zero-stuffed by `up`: with Tg = 16 * down and g[t] the rule of lcs_channelizer_taps at
 * D = down for ANY down (lcs_channelizer_proto: sinc((t - (Tg-1)/2) / down) * kaiser(Tg, 7.75)[t], sum 1, computed in double,
 * handed to the device as float), exactly, in "valid" mode,
 *
 *   y_k[m] = up * sum_n g[m*down + Tg-1 - n*up] * x[n] * exp(-2 pi i * f_shift[k] / fs_in * n),   m = 0 .. n_out-1,
 *            over the n with 0 <= m*down + Tg-1 - n*up < Tg, i.e. n = ceil(m*down / up) .. floor((m*down + Tg-1) / up)
 *
 * and needs n_in >= floor(((n_out-1)*down + Tg-1) / up) + 1.  For up = 1 this is lcs_channelize term for term, and a call with
 * up = 1 and down in 2..16 IS that call (forwarded, bit-identical).  g is the same design at the fine rate up * fs_in
 * = down * fs_out, so at fs_out = 1.92 Msps it has the figures stated above for decim 4 .. 16: passband (|f| <= 0.66 MHz) ripple
 * <= 0.0022 dB, and everything from 1.26 MHz outward -- the images of the zero-stuffing included -- at -78.1 dB or below
 * (down = 4, 5, 16, 25, 125, 128).  The carrier phase is kept in 64-bit fixed point per input sample n.
 *   1 < down / up <= 16,  2 <= down <= 128,  1 <= up <= 127;  20 Msps is 12/125, 10 Msps 24/125, 8 Msps 6/25, 6 Msps 8/25,
 *   2.56 Msps 3/4, 2.5 Msps 96/125, 2.4 Msps 4/5, 2.048 Msps 15/16.
 * Formats, alignment, the shift limit |f_shift| <= fs_in / 2, stream ordering, ownership and the 1e-5 bar are lcs_channelize's.
 * Non-finite samples (LCS_FMT_C64 only): the kernel multiplies every output's window out to a whole number of four-sample steps,
 * 4 * ceil(ceil(Tg / up) / 4) samples from n = ceil(m*down / up) on, with zero taps behind the last real one, and 0 * Inf is NaN.  An
 * Inf or NaN sample therefore makes every output whose sum above holds it non-finite, as the sum says, and MAY also spoil the
 * outputs whose window ends up to 4 samples before it (samples behind the capture's end count as zeros); every other output is
 * what it is without that sample.
 * LCS_ERR_BAD_ARG (with an lcs_last_error text, nothing launched) for a ratio above 16, down > 128, a common factor, up >= down
 * (no interpolation), a capture one sample too short, and everything lcs_channelize refuses.  lcs_channelizer_proto is ctx-free
 * and refuses down outside 2..128 or a null pointer. */
int lcs_channelizer_proto(int down, double *taps /*[16*down]*/);
int lcs_channelize_rational(lcs_ctx *ctx, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int up, int down,
                            const double *f_shift, int n_ch, void *d_out, uint32_t n_out);
/* The same stage with 8-bit carriers: d_out is the LCS_FMT_IQ_U8 batch layout of lcs_batch_enqueue, so a band search from one
 * wideband capture takes the int8 correlation kernel and holds a quarter of the bytes per carrier.  y_k[m] is the sum defined
 * above: lcs_channelize's (decim = down) when up == 1 and down is in 2..16, lcs_channelize_rational's otherwise; the argument rules
 * and the refusals (LCS_ERR_BAD_ARG, an lcs_last_error text, nothing launched) are those of that call.  Carrier k is scaled by a
 * power of two of its own and rounded to bytes:
 *   Power.   With P_k = (1/n_out) sum_m |y_k[m]|^2, the exponent e_k is the integer for which the component rms of 2^e_k * y_k lies
 *            in (16, 32]:  16^2 < 4^e_k * P_k / 2 <= 32^2.
 *   Code.    code = clamp(127 + rint(2^e_k * component), 0, 255), ties rounding to even; I then Q, the dongle convention
 *            (u8 - 127) / 128 of LCS_FMT_IQ_U8.
 *   Gain.    d_gain[k] = 2^e_k, an exact float (DEVICE [n_ch], or NULL): what converts reported powers back.
 *   Zero or non-finite power.  P_k equal to zero or not finite gives e_k = 0.  A non-finite component gives code 127.
 *   Layout.  d_out is DEVICE [n_ch][n_out][2] bytes: rows lie 2 * n_out bytes apart, so a row may start at any even address when
 *            n_out is odd; d_out itself is 16-byte aligned; any n_out >= 1 is accepted, as the float form accepts.
 *   Stream.  Everything is queued on the context's stream and the call returns without waiting; lcs_last_channelize_ms then spans
 *            the call through its last kernel.
 * Every threshold of the chain is relative to the buffer's own power, so the gain changes no decision; the quantisation noise
 * (1/12 per component) lies 38 dB or more below the carrier.  P_k is summed from the float outputs (fp32 per workgroup, double
 * across workgroups, one fixed order: two calls give the same bytes).  The float outputs live in a scratch buffer of the context
 * ([n_ch][n_out] complex<float>, grown on demand, freed with the context).  LCS_FMT_IQ_U8 is an OUTPUT here: as an input format it
 * is refused like any unknown one. */
int lcs_channelize_u8(lcs_ctx *ctx, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int up, int down,
                      const double *f_shift, int n_ch, void *d_out /*DEVICE [n_ch][n_out][2] u8*/, uint32_t n_out,
                      float *d_gain /*DEVICE [n_ch] or NULL*/);
/* Continuous form of lcs_channelize / lcs_channelize_rational for front ends that deliver a wideband stream in transfer buffers of
 * any size (HackRF, Airspy, USRP): the carrier phase runs on over the cuts and no sample at a buffer's end is lost.  A context holds
 * one such stream, as it holds one lcs_stream_open stream.  With N the samples pushed since open and Tg = 16 * down,
 *
 *   M(N) = 0 when N * up < Tg, otherwise (N * up - Tg) / down + 1 in integer division
 *
 * is the largest n_out for which the one-shot call accepts n_in = N (its rule is (n_out - 1) * down + Tg - 1 < N * up).  After a push
 * exactly the outputs m < M(N) of every carrier have been handed out, each once, by the first push that can compute it: a push
 * writes the outputs m_first .. m_first + n_emit - 1, m_first = the previous M, n_emit = M(N) - m_first, output m_first + j of
 * carrier k to d_out[k * row_stride + j], and touches nothing else of d_out.  Every output is, bit for bit, output m of ONE
 * lcs_channelize_rational call (lcs_channelize when up == 1, down in 2..16) on all N samples with n_out = M(N), for finite samples:
 * a column of the matrix product has the same filter rows, the same samples and the same order of summation wherever a launch
 * places it, and the carrier phase is step * n mod 2^64 of the stream's own sample index n, so a stream has no length limit.
 *   open   fmt, fs_in, up, down, f_shift (HOST [n_ch]) and n_ch as the one-shot forms take and refuse them, with their texts; up = 1
 *          is the integer form.  The filter taps, the phase steps and the filter bank are built here, once, into memory of the
 *          stream's own: lcs_channelize, lcs_channelize_rational and lcs_channelize_u8 on the same context stay legal while the
 *          stream is open and give what they give without it.
 *   count  n_emit of a push of n_chunk samples now; nothing is queued.
 *   push   d_chunk: DEVICE, n_chunk samples of fmt, aligned to one sample, n_chunk <= 2^31; NULL only with n_chunk == 0.  It must
 *          stay valid and unchanged until the work the push queued has run (everything is queued on the context's stream).
 *          d_out: DEVICE complex<float>, 8-byte aligned -- a caller advances it by 8 bytes per output it has taken; rows are
 *          row_stride samples apart, row_stride >= out_cap, and out_cap is the room per row.  n_emit and m_first (either may be
 *          NULL) are known in closed form and returned without waiting for the GPU.  A push may hand out nothing (a chunk shorter
 *          than the filter, n_chunk == 0): the samples are kept.  A push with n_emit > out_cap is refused: counts grow by at most one
 *          per sample (up < down), so count finds the chunk length of any exact split.
 *   close  waits for the queued pushes and frees the stream's memory; lcs_destroy closes an open stream.
 * Between pushes the context keeps the samples from the first one of the output column that holds output M(N) on (a column = the
 * `up` outputs whose windows start in one stretch of `down` samples): fewer than 16 * down / up + down, at most 365, in the input's
 * own format.  A push therefore costs two kernels (one when it hands out nothing) and recomputes at most up - 1 outputs.
 * Non-finite samples (LCS_FMT_C64): the caveat of lcs_channelize_rational holds with one more clause.  The up to 4 samples behind an
 * output's window that the one-shot call multiplies by zero taps may not have arrived yet when the stream computes the output, and
 * count as zeros then: an output whose window holds no non-finite sample may be finite here where the one-shot call makes it
 * non-finite, never the reverse.
 * LCS_ERR_BAD_ARG (an lcs_last_error text, nothing launched, the stream where it was): open with a stream already open; count, push
 * or close with none; n_chunk above 2^31; a null chunk with n_chunk > 0; a misaligned chunk or d_out; a null d_out with outputs to
 * hand out; row_stride < out_cap; out_cap < n_emit.  lcs_last_channelize_ms is not set by a push: it keeps the time of the last
 * one-shot call. */
int lcs_chan_stream_open(lcs_ctx *ctx, int fmt, double fs_in, int up, int down, const double *f_shift /*host [n_ch]*/, int n_ch);
int lcs_chan_stream_count(lcs_ctx *ctx, uint64_t n_chunk, uint32_t *n_emit);
int lcs_chan_stream_push(lcs_ctx *ctx, const void *d_chunk /*DEVICE, n_chunk samples of fmt*/, uint64_t n_chunk,
                         void *d_out /*DEVICE complex<float>*/, uint32_t row_stride /*samples between carrier rows*/, uint32_t out_cap,
                         uint32_t *n_emit, uint64_t *m_first);
int lcs_chan_stream_close(lcs_ctx *ctx);
/* The continuous form with 8-bit carriers: the stream hands out whole CAPTURES of n_cap outputs per carrier as bytes, the
 * LCS_FMT_IQ_U8 batch layout, each capture of each carrier scaled by a power of two of its own -- what a live band search feeds the
 * int8 correlation kernel.  M(N), the formats, the rates, the chunk's alignment, the stream ordering and the non-finite clause are
 * lcs_chan_stream_open's.  Capture c is the outputs m = c * n_cap .. (c + 1) * n_cap - 1 of every carrier.  After a push exactly the
 * captures c < M(N) / n_cap (integer division) have been handed out, each once: a push writes the captures cap_first .. cap_first +
 * n_done - 1, capture cap_first + j to slot j of d_out and of d_gain, and touches nothing else of either; slots >= n_done stay as
 * they were.  n_done and cap_first (either may be NULL) are closed forms of N and are returned without waiting for the GPU.
 *   Bytes.   With y_k[m] the floats lcs_chan_stream_push hands out for the same samples (bit for bit those of one
 *            lcs_channelize_rational call), capture c of carrier k is lcs_channelize_u8's rule on y_k[c * n_cap ..]: P = the mean of
 *            |y|^2 over the capture; e the integer with 16^2 < 4^e * P / 2 <= 32^2, 0 for a P that is zero or not finite; code =
 *            clamp(127 + rint(2^e * component), 0, 255), ties to even, 127 for a component that is not finite; d_gain = 2^e.
 *   Chunking.  A gain is constant inside a capture and free between captures: every threshold of the search chain is relative to the
 *            buffer's own power.  It is known when the capture is complete, so the stream keeps the capture in hand as floats
 *            ([n_ch][n_cap] complex<float>, allocated by open_u8, freed by close) and sums P from those floats in ONE order that
 *            depends on n_cap only (fp32 over fixed blocks of a row, double across the blocks): any two ways of cutting the same
 *            samples into pushes, and any two runs, give the same bytes and the same gains, bit for bit.
 *   Layout.  A capture is [n_ch][n_cap][2] bytes, I then Q: rows lie 2 * n_cap bytes apart (at any even address when n_cap is odd),
 *            captures 2 * n_ch * n_cap bytes apart.  d_out: DEVICE [cap_room][n_ch][n_cap][2], 16-byte aligned; d_gain: DEVICE
 *            [cap_room][n_ch] floats, or NULL.
 *   open_u8  as open, plus n_cap >= 1.  A context holds ONE channelizer stream of either kind; close closes either.
 *   count_u8 n_done of a push of n_chunk samples now; nothing is queued.  lcs_chan_stream_count works on either kind of stream.
 *   push_u8  d_chunk as push takes it.  A push may complete no capture (it writes nothing then) or many.
 * LCS_ERR_BAD_ARG (an lcs_last_error text, nothing launched, the stream where it was; all decided before the first launch): everything
 * open refuses; n_cap < 1; a stream already open; count_u8 or push_u8 with no stream or on a stream opened by lcs_chan_stream_open;
 * lcs_chan_stream_push on a stream opened here; n_chunk above 2^31; a null chunk with n_chunk > 0; a misaligned chunk; a null d_out
 * with captures to hand out; d_out not 16-byte aligned; d_gain not aligned to a float; cap_room < n_done.  lcs_last_channelize_ms is
 * not set by a push. */
int lcs_chan_stream_open_u8(lcs_ctx *ctx, int fmt, double fs_in, int up, int down, const double *f_shift /*host [n_ch]*/, int n_ch,
                            uint32_t n_cap);
int lcs_chan_stream_count_u8(lcs_ctx *ctx, uint64_t n_chunk, uint32_t *n_done);
int lcs_chan_stream_push_u8(lcs_ctx *ctx, const void *d_chunk /*DEVICE, n_chunk samples of fmt*/, uint64_t n_chunk,
                            void *d_out /*DEVICE [cap_room][n_ch][n_cap][2] u8, 16-byte aligned*/,
                            float *d_gain /*DEVICE [cap_room][n_ch] or NULL*/, uint32_t cap_room, uint32_t *n_done, uint64_t *cap_first);
/* HIP-event time (ms) of the last lcs_channelize, lcs_channelize_rational or lcs_channelize_u8 of the context (filter-bank build
 * through the call's last kernel), as lcs_last_xcorr_ms */
int lcs_last_channelize_ms(lcs_ctx *ctx, float *ms);

/* ---- successive cancellation (csrc/sic.h, sic.hip) --------------------------------------------------------------------
 * peak_search reports one peak per 549 lags of a PSS row and nothing 12 dB below a buffer's strongest peak: a cell under a
 * synchronised neighbour with the same n_id_2 is never listed.  What a decoded MIB makes known of a cell -- PSS, SSS, the
 * cell-specific reference signals of its ports and the PBCH of every frame -- is rebuilt here through the cell's own channel
 * estimate (from the CRS alone) over the WHOLE capture and subtracted on the device; the unchanged chain then searches the
 * residual.  csrc/sic.h states the rule, tests/sic_ref.py restates it in numpy.
 *
 * lcs_sic_cancel_dev: n_buf device-resident captures (LCS_FMT_IQ_U8 or LCS_FMT_C64, n_cap samples each), cells
 * [n_buf][max_cells_per_buf] with n_cells_per_buf[b] records in use, -> d_residual_c64 [n_buf][n_cap] complex<float> (the
 * LCS_FMT_C64 batch layout; a buffer without cells is copied).  Records without a decoded MIB (n_rb_dl, n_ports or cp_type
 * unknown) are left in the capture: their info has n_sym == 0.  On a context in LCS_DUPLEX_TDD the sync signals are taken at the
 * TDD positions and CRS / PBCH are cancelled in subframes 0 and 5 only -- a record carries no uplink-downlink configuration;
 * lcs_sic_cancel_cfg_dev takes one per record (ul_dl_config, laid out like cells, nullable; 0 .. 6 as lcs_last_tdd_info reports it,
 * anything else: none) and then cancels CRS / PBCH in that configuration's downlink subframes (lcs_tdd_dl_mask) and in symbol 0 of
 * subframes 1 and 6 as well: the mask rule of lcs_cell_meas.  mask selects the components; 0, or bits beyond LCS_SIC_ALL, is
 * refused.  So is a capture of more than 268800 samples (14 frames at 1.92 Msps), or one that spans more than 16 frames of a cell: the
 * per-cell PBCH table holds 16.  info (nullable) is [n_buf][max_cells_per_buf]. */
#define LCS_SIC_PSS 1
#define LCS_SIC_SSS 2
#define LCS_SIC_CRS 4
#define LCS_SIC_PBCH 8
#define LCS_SIC_ALL 15
#define LCS_SIC_MAX_ROUNDS 4
typedef struct lcs_sic_info {
  double power[4];          /* energy of the rebuilt PSS, SSS, CRS, PBCH over the symbols' transform windows (sum |x|^2 of the samples) */
  double gain_re, gain_im;  /* the sync gain: received SSS over (port-0 channel x sequence) */
  double pss_before;        /* energy of the 62 PSS subcarriers over the cell's PSS symbols in the capture ... */
  double pss_after;         /* ... and in the residual (every cell of the buffer cancelled): the suppression is their ratio */
  int32_t n_sym;            /* OFDM symbols covered, 0: the cell was not cancelled */
  int32_t n_pss;            /* PSS symbols among them */
  int32_t n_dup;            /* lcs_search_*_sic: times a later round found this identity again (the record was dropped) */
  int32_t ul_dl_config;     /* the TDD configuration whose downlink subframes were cancelled, LCS_TDD_NOT_ESTIMATED: subframes 0 and 5 (TDD) / all (FDD) */
} lcs_sic_info;             /* 80 bytes */
int lcs_sic_cancel_dev(lcs_ctx *ctx, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap, const lcs_cell *cells,
                       const int *n_cells_per_buf, int max_cells_per_buf, const double *fc_requested, const double *fc_programmed,
                       double fs_programmed, int mask, void *d_residual_c64, lcs_sic_info *info);
int lcs_sic_cancel_cfg_dev(lcs_ctx *ctx, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap, const lcs_cell *cells,
                           const int *n_cells_per_buf, int max_cells_per_buf, const int32_t *ul_dl_config, const double *fc_requested,
                           const double *fc_programmed, double fs_programmed, int mask, void *d_residual_c64, lcs_sic_info *info);
/* The search with cancellation rounds.  Round 0 is the plain call (lcs_search_capbuf / lcs_search_batch_dev: the same records,
 * the u8 route kept).  Every further round (max_rounds 1 .. LCS_SIC_MAX_ROUNDS in all; 2 = one cancellation) cancels ALL cells
 * found so far from the ORIGINAL capture and runs the chain on the residual as complex<float>; cells whose n_id_cell the buffer
 * already lists are dropped (n_dup of the listed record counts them), the others are appended with their round in round_of_cell.
 * A buffer whose last round added nothing, or that has no cell, takes no further part; the call ends when no buffer does.
 * round_of_cell and info (both nullable) are laid out like cells; info holds what the last cancellation a cell took part in
 * reported.  peaks / n_peaks are round 0's.
 * On a context in LCS_DUPLEX_TDD with lcs_set_tdd_config on, every cell is cancelled with the uplink-downlink configuration its own
 * round's chain found for it (lcs_sic_cancel_cfg_dev's rule; info.ul_dl_config says which).
 * Every round >= 1 is a fused call of its own on a COMPACTED batch of residuals: after lcs_search_*_sic the context's
 * lcs_last_tdd_info, lcs_last_cell_meas, lcs_last_xcorr_ms and lcs_last_batch_stats describe the last round's batch, not the caller's
 * buffers.  The side-table records of the cells this call handed out are gathered round by round instead: lcs_last_sic_tdd_info and
 * lcs_last_sic_cell_meas, laid out like cells ([n_buf][max_cells_per_buf], the call's own max_cells_per_buf -- another value is
 * refused), a cell of round r carrying what round r's chain measured on ITS input (the residual for r >= 1), and
 * LCS_TDD_NOT_ESTIMATED / LCS_MEAS_NOT_MEASURED where the mode was off. */
int lcs_search_capbuf_sic(lcs_ctx *ctx, const double *capbuf_re_im, uint32_t n_cap, const double *f_search_set, uint16_t n_f,
                          double fc_requested, double fc_programmed, double fs_programmed, lcs_cell *cells, int max_cells,
                          int *n_cells, lcs_cell *peaks, int max_peaks, int *n_peaks, int max_rounds, int mask,
                          int32_t *round_of_cell, lcs_sic_info *info);
int lcs_search_batch_sic_dev(lcs_ctx *ctx, const void *d_capbufs, int fmt, int n_buf, uint32_t n_cap, const double *f_search_set,
                             uint16_t n_f, const double *fc_requested, const double *fc_programmed, double fs_programmed,
                             lcs_cell *cells, int max_cells_per_buf, int *n_cells, int max_rounds, int mask,
                             int32_t *round_of_cell, lcs_sic_info *info);
/* The last lcs_search_*_sic call: stats[0] rounds run (1: round 0 alone), [1] cancellation launches, [2] cells appended by
 * rounds >= 1, [3] records dropped as already listed. */
int lcs_last_sic_stats(lcs_ctx *ctx, int stats[4]);
int lcs_last_sic_tdd_info(lcs_ctx *ctx, lcs_tdd_info *info, int max_cells_per_buf);
int lcs_last_sic_cell_meas(lcs_ctx *ctx, lcs_meas_info *info, int max_cells_per_buf);

/* Stream the context launches on (hipStream_t as void*), for external event timing. */
void *lcs_stream(lcs_ctx *ctx);
int lcs_sync(lcs_ctx *ctx);

/* ---- table accessors (tests compare them with the oracle) ---------------------------- */
int lcs_table_pss_td(int n_id_2, double *out_re_im /*137*2*/);    /* src/lte_lib.cpp:177-188 */
int lcs_table_pss_fd(int n_id_2, double *out_re_im /*62*2*/);     /* src/lte_lib.cpp:155-161 */
int lcs_table_sss_fd(int n_id_1, int n_id_2, int slot_num, int32_t *out /*62*/); /* :199-257 */
int lcs_table_lte_pn(uint32_t c_init, uint32_t len, uint8_t *out);               /* :41-147 */
double lcs_chi2cdf_inv(double p, double k);                       /* include/dsp.h:188-193 */
/* The QPSK symbols of one 40 ms PBCH period from a record's fields (csrc/lte_pbch_enc.cpp): 960 (normal CP) or 864 pairs */
int lcs_table_pbch_symbols(int n_id_cell, int n_ports, int n_rb_dl, int phich_duration, int phich_resource, int sfn, int cp_type,
                           double *out_re_im);

#ifdef __cplusplus
}
#endif
#endif /* LCS_H */
