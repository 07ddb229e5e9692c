// cell_meas.hip -- RSRP, RSSI, RSRQ and the noise power of the cells on the work list (lcs_set_cell_meas, lcs_cell_meas; the rule:
// cell_meas.h).  A translation unit of its own, so that the code object of the per-cell chain (tfg_mib.hip) is what it is without it:
// with the mode off no kernel of this file runs, and none of the chain's kernels moves.
#include "lcs_internal.h"
#include "tfg_layout.h"
#include "lte_device.h"
#include "cell_meas.h"
static_assert(TDD_ROW_LANES == 16, "tfg_layout.h: TC_GROUPS");

// ------------------------------------------------------------------ RSRP, RSSI, RSRQ and noise power of a cell (cell_meas.h)
// k_tdd_config's shape: one workgroup per cell, eight waves over port 0's reference rows, 16 lanes per row, a thread's rows
// q = group + 32 pass.  Lane m < 12 loads the six contiguous subcarriers 6 m .. 6 m + 5 of its row as six 16-byte loads (the 12 lanes
// of a row read 1152 contiguous bytes): they hold the lane's reference element of port 0 and of port 1 -- picked by selects, not
// by a register index -- and the lane's share of w.  The shifts of all of a thread's rows are loaded first (and packed into one
// 64-bit word: nine-entry arrays of them ended up in scratch); the grid values follow
// in MC_CHUNK = 3 rows at a time, all 21 loads of a chunk in flight before its first use: three round trips per cell instead of
// one, because all nine rows at once are 216 registers of load data alone, which does not fit beside a resident correlation
// workgroup (tests/test_tables_abi.py) and would leave the compiler the choice between scratch and serial loads.  Rows outside the
// mask are not loaded at all (TDD: 2 of 10 subframes).  The seven row sums (meas_row_sum_lanes) meet in LDS; 7 x 40 threads add up
// their value of their bin in row order, seven add up the bins of the mask, one finishes (meas_finish) and sixteen copy the record out.
// It reads the RAW grid (rows 0 and n_symb - 3 of every slot: tfg_needed_row) and the RS_DL table of k_cell_prep.
// The mask: `dl_mask` for every cell, unless `tdd` (the table k_tdd_config filled on this stream just before) gives the cell a
// configuration 0 .. 6.  `force`: the stage entry point -- out[it], whatever the cell carries; in the fused chain the record goes to
// the cell's place in a table laid out like the peak table, and a cell without a MIB keeps LCS_MEAS_NOT_MEASURED.
#define MC_CHUNK 3
static_assert(TC_PASSES % MC_CHUNK == 0 && sizeof(lcs_meas_info) == 128 && MEAS_NV * TDD_BINS <= TC_THREADS, "k_cell_meas's row split");
__global__ __launch_bounds__(TC_THREADS) void k_cell_meas(const lcs_cell *__restrict__ cells, const WorkItem *__restrict__ items,
                                                          const int *__restrict__ n_work, const double *__restrict__ scratch,
                                                          const double2 *__restrict__ tfg, const lcs_tdd_info *__restrict__ tdd,
                                                          lcs_meas_info *__restrict__ out, int dl_mask, int force) {
  LCS_TAIL_PRIO();
  __shared__ double s_row[MEAS_NV][TC_MAX_Q];
  __shared__ double s_bin[MEAS_NV][TDD_BINS];
  __shared__ double s_tot[MEAS_NV];
  __shared__ lcs_meas_info s_info;
  const int tid = threadIdx.x, grp = tid / TDD_ROW_LANES, m = tid % TDD_ROW_LANES;
  for (int it = blockIdx.x; it < *n_work; it += gridDim.x) {
    const lcs_cell c = cells[it];
    const double *sc = scratch + (size_t)it * CS_SIZE;
    const int n_symb = cell_n_symb(c);
    const size_t place = force ? (size_t)it : (size_t)items[it].slot * LCS_MAXP + items[it].peak;
    const bool measure = n_symb > 0 && cell_id(c) >= 0 && (force || c.n_rb_dl != -1);      // the same for the whole workgroup
    if (measure) {
      int mask = dl_mask;
      if (tdd && !force) { const int cfg_mask = meas_tdd_dl_mask(tdd[place].ul_dl_config); mask = cfg_mask > 0 ? cfg_mask : mask; }
      const int ports = meas_ports(c.n_ports);
      const int n_ofdm = min(max((int)sc[CS_N_OFDM], 0), ROWS);
      const int n_q = min(tdd_n_ref_rows(n_ofdm, n_symb), TC_MAX_Q);
      const double2 *g = tfg + (size_t)it * ROWS * NSC;
      // per pass seven bits: shift_0, shift_1 (three bits each) and "live" -- a used row of a table that has both ports on it
      // (without: the row counts as zeros)
      unsigned long long shp = 0ull;
#pragma unroll
      for (int p = 0; p < TC_PASSES; ++p) {
        const int q = grp + TC_GROUPS * p;
        const int row20 = d_imod(q >> 1, 20) * n_symb + ((q & 1) ? n_symb - 3 : 0);
        const bool used = q < n_q && m < 12 && meas_bin_used(q % TDD_BINS, mask);
        const int a = used ? (int)sc[CS_SHIFT + row20 * 4] : -1, b = used ? (int)sc[CS_SHIFT + row20 * 4 + 1] : -1;
        const bool live = a >= 0 && a <= 5 && b >= 0 && b <= 5;
        shp |= (unsigned long long)(live ? (a | (b << 3) | 64) : 0) << (7 * p);
      }
#pragma unroll
      for (int p0 = 0; p0 < TC_PASSES; p0 += MC_CHUNK) {
        double2 x[MC_CHUNK][6], r[MC_CHUNK];
#pragma unroll
        for (int pp = 0; pp < MC_CHUNK; ++pp) {
          const int p = p0 + pp, q = grp + TC_GROUPS * p;
          const int row20 = d_imod(q >> 1, 20) * n_symb + ((q & 1) ? n_symb - 3 : 0);
          const bool live = (shp >> (7 * p + 6)) & 1ull;
          const double2 *src = g + (size_t)tdd_grid_row(q, n_symb) * NSC + 6 * m;
#pragma unroll
          for (int k = 0; k < 6; ++k) x[pp][k] = live ? src[k] : make_double2(0, 0);
          r[pp] = live ? *reinterpret_cast<const double2 *>(&sc[CS_RS + (row20 * 12 + m) * 2]) : make_double2(0, 0);
        }
#pragma unroll
        for (int pp = 0; pp < MC_CHUNK; ++pp) {
          const int p = p0 + pp, q = grp + TC_GROUPS * p;
          const meas_x6 xs = {mk(x[pp][0].x, x[pp][0].y), mk(x[pp][1].x, x[pp][1].y), mk(x[pp][2].x, x[pp][2].y),
                              mk(x[pp][3].x, x[pp][3].y), mk(x[pp][4].x, x[pp][4].y), mk(x[pp][5].x, x[pp][5].y)};
          const cd2 rs = mk(r[pp].x, r[pp].y);
          const cd2 h0 = meas_h(xs, (int)(shp >> (7 * p)) & 7, rs), h1 = meas_h(xs, (int)(shp >> (7 * p + 3)) & 7, rs);
          const cd2 h0n = mk(__shfl_down(h0.re, 1, TDD_ROW_LANES), __shfl_down(h0.im, 1, TDD_ROW_LANES));
          const cd2 h1n = mk(__shfl_down(h1.re, 1, TDD_ROW_LANES), __shfl_down(h1.im, 1, TDD_ROW_LANES));
          double v[MEAS_NV];
          meas_entry(xs, m, ports, h0, h0n, h1, h1n, v, 12);
#pragma unroll
          for (int i = 0; i < MEAS_NV; ++i) {
            const double s = meas_row_sum_lanes<TDD_ROW_LANES>(m < 12 ? v[i] : 0.0);
            if (m == 0 && q < n_q) s_row[i][q] = s;
          }
        }
      }
      __syncthreads();
      if (tid < MEAS_NV * TDD_BINS) {
        const int i = tid / TDD_BINS, b = tid % TDD_BINS;
        s_bin[i][b] = meas_bin_sum(s_row[i], b, n_q);
      }
      __syncthreads();
      if (tid < MEAS_NV) s_tot[tid] = meas_total(s_bin[tid], mask);
      __syncthreads();
      if (tid == 0) meas_finish(s_tot, meas_n_rows(n_q, mask), ports, mask, &s_info);
    } else if (tid == 0) {
      meas_clear(&s_info, LCS_MEAS_NOT_MEASURED);
    }
    __syncthreads();
    if (tid < 16) reinterpret_cast<double *>(out + place)[tid] = reinterpret_cast<const double *>(&s_info)[tid];
    __syncthreads();                                     // the next cell rewrites the shared arrays
  }
}

// RSRP / RSSI / RSRQ / noise of every cell on the work list (lcs_set_cell_meas, lcs_cell_meas): behind k_mib_select and k_tdd_config,
// on the raw grid.  tdd: k_tdd_config's table of this launch, or null
int lcs_launch_cell_meas(lcs_ctx *c, const Launch &L, const lcs_tdd_info *tdd, lcs_meas_info *out, int dl_mask, bool force) {
  hipLaunchKernelGGL(k_cell_meas, dim3(L.grid_items), dim3(TC_THREADS), 0, c->stream, c->cells_out, c->work_items, c->n_work,
                     c->cell_scratch, (const double2 *)c->tfg, tdd, out, dl_mask, force ? 1 : 0);
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}
