// trk_layout.h -- how the tracker's host side (tracker.hip) cuts its buffers into arrays, and the integer rules of the continuous
// form: the one definition of each.  Plain C++17 with no HIP in it, so that a host compiler takes it: tests/test_trk_layout_host.py
// walks every shape of its domain through tests/host/trk_layout_host.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/lcs.h"

// ---- what a symbol count implies
inline int trk_rs_cap(int n_sym) { return n_sym / 3 + 4; }                                   // reference symbols of one port in a block: at most 2 per slot of >= 6 symbols
inline int trk_n_off(int n_sym) { return n_sym / 120 - 3 > 0 ? n_sym / 120 - 3 : 0; }        // frame offsets that could hold four frames (120 = extended-CP frame)
inline int trk_hf_cap(int n_sym) { return n_sym / 60 + 2; }                                  // PSS/SSS pairs of a block: two per frame of >= 120 symbols

// A block shape, and the rule a set of buffers grows by: to the largest number of cells seen, and in symbols with head room (the
// continuous form's tail varies in length from call to call).  A set sized for `cap` serves every shape that fits it.
struct TrkShape { int n_cells = 0, n_sym = 0; };
inline bool trk_fits(TrkShape cap, TrkShape s) { return s.n_cells <= cap.n_cells && s.n_sym <= cap.n_sym; }
inline TrkShape trk_grow(TrkShape cap, TrkShape s) {
  const int head = s.n_sym + s.n_sym / 8;
  TrkShape g;
  g.n_cells = s.n_cells > cap.n_cells ? s.n_cells : cap.n_cells;
  g.n_sym = head > cap.n_sym ? head : cap.n_sym;
  return g;
}

// ---- the buffers and the arrays in them
enum TrkBuf {
  // the block workspace (lcs_track_block; lcs_track_stats reads it back)
  TB_TD, TB_META, TB_CELLS, TB_SYMS, TB_RS, TB_IDX, TB_RAW, TB_FMETA, TB_CE, TB_PW, TB_SMALL,
  TB_STAGE,                                       // the host staging block of a call: the up part, then the down part
  TB_ACFD, TB_ACTD, TB_SYNC, TB_SYNCCE,           // lcs_track_stats
  TB_CUT_HIT, TB_CUT_META,                        // lcs_track_cut
  TB_N
};
enum { TRK_BLOCK_BUFS = TB_STAGE - TB_TD, TRK_STAT_BUFS = TB_CUT_HIT - TB_ACFD, TRK_CUT_BUFS = TB_N - TB_CUT_HIT };
enum TrkArr {
  TA_TD, TA_FO, TA_FT, TA_LATE, TA_BPO, TA_CELLS, TA_SYMS, TA_RS, TA_SHIFT, TA_IDX, TA_NRS, TA_RAW, TA_FILT, TA_FM, TA_MEAS, TA_CE, TA_PW,
  TA_NMEAS, TA_UPTO, TA_MIBOK, TA_MIBBITS, TA_MIBFIRST,
  TH_FO, TH_FT, TH_LATE, TH_CELLS_UP, TH_MEAS, TH_BITS, TH_NMEAS, TH_UPTO, TH_MIBOK, TH_CELLS_DOWN,
  TA_ACFD, TA_ACTD, TA_SYNC, TA_SYNCCE,
  TA_CUT_HIT, TA_CUT_N, TA_CUT_FLAGS, TA_CUT_POS, TA_CUT_LATE, TA_CUT_CELLS,
  TA_N
};
// An array holds `per` elements for every unit of its dimension; the dimensions of a layout (TrkDims) are the cells and the cells
// times (symbols, rs_cap, n_off, hf_cap).
enum TrkDim { TD_CELL, TD_SYM, TD_RS, TD_OFF, TD_HF, TD_N };
struct TrkDims { size_t d[TD_N]; };
inline TrkDims trk_dims(TrkShape s) {
  const size_t c = (size_t)s.n_cells;
  return TrkDims{{c, c * s.n_sym, c * trk_rs_cap(s.n_sym), c * trk_n_off(s.n_sym), c * trk_hf_cap(s.n_sym)}};
}
// The cutter's buffers are laid out by their CAPACITY (the most cells, and the most cells x symbols, of any call so far): the
// per-cell flags behind the hits must keep their zeros from call to call, so they may not move with the call's shape.
inline TrkDims trk_cut_dims(size_t cells_cap, size_t n_cap) { return TrkDims{{cells_cap, n_cap, 0, 0, 0}}; }

struct TrkRow { uint8_t buf, dim; uint16_t elem, align; uint32_t per; };       // in TrkArr's order; arrays of a buffer follow each other
#define TRK_Z 16, 16        /* complex<double> (double2): element and alignment in bytes */
#define TRK_D 8, 8          /* double, and the 64-bit integers */
#define TRK_I 4, 4
#define TRK_C (uint16_t)sizeof(lcs_track_cell), 8
inline constexpr TrkRow TRK_ROWS[TA_N] = {
    {TB_TD, TD_SYM, TRK_Z, 128},                  // TA_TD       [c][n_sym][128]
    {TB_META, TD_SYM, TRK_D, 1},                  // TA_FO       [c][n_sym]   fo, ft and late go up as ONE copy: adjacent, here and in the staging block
    {TB_META, TD_SYM, TRK_D, 1},                  // TA_FT
    {TB_META, TD_SYM, TRK_D, 1},                  // TA_LATE
    {TB_META, TD_SYM, TRK_D, 1},                  // TA_BPO      the running bulk phase at every symbol
    {TB_CELLS, TD_CELL, TRK_C, 1},                // TA_CELLS
    {TB_SYMS, TD_SYM, TRK_Z, 72},                 // TA_SYMS     [c][n_sym][72]
    {TB_RS, TD_CELL, TRK_D, 140 * 24},            // TA_RS       [c][140][24]
    {TB_RS, TD_CELL, TRK_D, 140 * 4},             // TA_SHIFT    [c][140][4]
    {TB_IDX, TD_RS, TRK_I, 4},                    // TA_IDX      [c][4][rs_cap]
    {TB_IDX, TD_CELL, TRK_I, 4},                  // TA_NRS      [c][4]
    {TB_RAW, TD_RS, TRK_Z, 4 * 12},               // TA_RAW      [c][4][rs_cap][12]
    {TB_RAW, TD_RS, TRK_Z, 4 * 12},               // TA_FILT
    {TB_FMETA, TD_RS, TRK_D, 4 * 4},              // TA_FM       [c][4][rs_cap][4]: tp, sp, sp_raw, np
    {TB_FMETA, TD_RS, TRK_D, 4 * LCS_TRK_MEAS},   // TA_MEAS     [c][4][rs_cap][LCS_TRK_MEAS]
    {TB_CE, TD_SYM, TRK_Z, 4 * 72},               // TA_CE       [c][4][n_sym][72]
    {TB_PW, TD_SYM, TRK_D, 4 * 4},                // TA_PW       [c][4][n_sym][4]
    {TB_SMALL, TD_CELL, TRK_I, 4},                // TA_NMEAS    [c][4]       nmeas, upto and mibok come down as ONE copy: adjacent
    {TB_SMALL, TD_CELL, TRK_I, 4},                // TA_UPTO     [c][4]
    {TB_SMALL, TD_OFF, TRK_I, 1},                 // TA_MIBOK    [c][n_off]
    {TB_SMALL, TD_OFF, TRK_D, 1},                 // TA_MIBBITS  [c][n_off] 64-bit words
    {TB_SMALL, TD_CELL, TRK_I, 1},                // TA_MIBFIRST [c]          the continuous form's first frame offset still to attempt
    {TB_STAGE, TD_SYM, TRK_D, 1},                 // TH_FO       the up part: the metadata as the caller hands it over, and the cells
    {TB_STAGE, TD_SYM, TRK_D, 1},                 // TH_FT
    {TB_STAGE, TD_SYM, TRK_D, 1},                 // TH_LATE
    {TB_STAGE, TD_CELL, TRK_C, 1},                // TH_CELLS_UP
    {TB_STAGE, TD_RS, 8, 16, 4 * LCS_TRK_MEAS},   // TH_MEAS     the down part starts on 16 bytes: TA_MEAS, ...
    {TB_STAGE, TD_OFF, TRK_D, 1},                 // TH_BITS     ... TA_MIBBITS, ...
    {TB_STAGE, TD_CELL, TRK_I, 4},                // TH_NMEAS    ... TA_NMEAS, TA_UPTO and TA_MIBOK as they lie in the workspace ...
    {TB_STAGE, TD_CELL, TRK_I, 4},                // TH_UPTO
    {TB_STAGE, TD_OFF, TRK_I, 1},                 // TH_MIBOK
    {TB_STAGE, TD_CELL, TRK_C, 1},                // TH_CELLS_DOWN  ... and the cells with the bulk phase after the block
    {TB_ACFD, TD_RS, TRK_Z, 4 * 12},              // TA_ACFD     [c][4][rs_cap][12]
    {TB_ACTD, TD_RS, TRK_Z, 4 * 72},              // TA_ACTD     [c][4][rs_cap][72]
    {TB_SYNC, TD_HF, TRK_D, 4},                   // TA_SYNC     [c][hf_cap][4]
    {TB_SYNCCE, TD_HF, TRK_Z, 72},                // TA_SYNCCE   [c][hf_cap][72]
    {TB_CUT_HIT, TD_SYM, TRK_I, 1},               // TA_CUT_HIT  [cells][symbols]: first sample of every symbol
    {TB_CUT_HIT, TD_CELL, TRK_I, 1},              // TA_CUT_N    symbols found per cell
    {TB_CUT_HIT, TD_CELL, TRK_I, 1},              // TA_CUT_FLAGS
    {TB_CUT_HIT, TD_CELL, TRK_D, 1},              // TA_CUT_POS  64-bit: where the next call's search starts
    {TB_CUT_META, TD_SYM, TRK_D, 1},              // TA_CUT_LATE [cells][symbols]
    {TB_CUT_META, TD_CELL, TRK_D, 5},             // TA_CUT_CELLS [cells][5]: cp_type, frame_timing, freq_off, first symbol, first sample
};
#undef TRK_Z
#undef TRK_D
#undef TRK_I
#undef TRK_C

// Where every array starts in its buffer and how many elements it holds, and every buffer's length, all in one walk of the table:
// a size and an offset are the same running sum.  (Every array's length is monotone in every dimension, and so is every offset.)
struct TrkLay {
  size_t off[TA_N], n[TA_N];     // bytes from the start of the array's buffer; elements
  size_t bytes[TB_N];
  size_t size(int a) const { return n[a] * TRK_ROWS[a].elem; }
  template <class T> T *at(void *buf_start, int a) const { return reinterpret_cast<T *>(static_cast<char *>(buf_start) + off[a]); }
};
inline TrkLay trk_layout(const TrkDims &dims) {
  TrkLay l{};
  for (int a = 0; a < TA_N; ++a) {
    const TrkRow &r = TRK_ROWS[a];
    size_t &end = l.bytes[r.buf];
    l.off[a] = (end + r.align - 1) / r.align * r.align;
    l.n[a] = dims.d[r.dim] * r.per;
    end = l.off[a] + l.size(a);
  }
  return l;
}
inline TrkLay trk_layout(TrkShape s) { return trk_layout(trk_dims(s)); }

// ---- the continuous form (lcs_track_stream_block): a call's block is [carried tail ++ n_sym new symbols], the tail starting at a
// frame boundary of the stream (F = 140 or 120 symbols); afterwards the stream carries whole frames from the last boundary that
// leaves at least three of them behind it.
struct TrkStreamStep {
  int n_tail, L;                 // carried symbols in front of the new ones, and the length of the block
  long long n_after, T_next;     // symbols delivered after this call; stream index of the next tail's first symbol
  size_t keep_from, n_keep;      // the next tail is the block's symbols [keep_from, keep_from + n_keep): keep_from + n_keep == L
};
inline TrkStreamStep trk_stream_step(long long n_seen, long long tail_start, int n_sym, int F) {
  TrkStreamStep s;
  s.n_tail = (int)(n_seen - tail_start);
  s.L = s.n_tail + n_sym;
  s.n_after = n_seen + n_sym;
  s.T_next = (s.n_after - 3 * F) / F * F > 0 ? (s.n_after - 3 * F) / F * F : 0;
  s.keep_from = (size_t)(s.T_next - tail_start);
  s.n_keep = (size_t)(s.n_after - s.T_next);
  return s;
}
// frame offset of the block (whose first symbol has stream index T) below which every offset was attempted by an earlier call
inline int trk_mib_first(long long mib_next, long long T, int F) { return mib_next - T / F > 0 ? (int)(mib_next - T / F) : 0; }
