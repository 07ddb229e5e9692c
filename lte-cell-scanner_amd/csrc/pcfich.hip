// pcfich.hip -- the PCFICH of a wide cell on the device (lcs_pcfich_wide, lcs_pcfich; the rule: pcfich.h, include/lcs.h).  A
// translation unit of its own, like tfg_wide.hip whose grid it reads: a context that never calls the stage runs no kernel of this
// file and allocates none of its buffers, and the code objects of the chain and of the measurement are what they are without it.
#include "lcs_internal.h"
#include "lte_device.h"
#include "pcfich.h"

// ------------------------------------------------------------------ one wave per subframe
// Workgroup g (one wave) takes grid subframe g: rows[2 g] and rows[2 g + 1] are the rows of c->meas_wide.grid that hold its symbols
// 0 and 1, -1 for a subframe that is not read (outside the mask or the grid).  Lanes 0 and 1 build the reference sequences of the
// two rows side by side (the second with four ports only), lane 0 the 32 scrambling bits.  Then every lane takes resource element
// lane mod 16 -- its column, its y and the two channel values at that column, from the two reference elements around it and no
// others --, the lanes of a pair trade hb and y, and the four values of the sixteen live lanes go through the wave's butterfly.
// Lane 0 decides and writes the subframe's entry; nobody else writes it, and no entry depends on another wave.
__global__ __launch_bounds__(PCF_LANES) void k_pcfich(const double2 *__restrict__ grid, const int *__restrict__ rows, const uint32_t *__restrict__ jump /*[2][32]: rs, scrambling*/,
                                                      lcs_pcfich_info *__restrict__ out, int n_sf, int id, int cp_type, int n_symb, int ports, int n_rb) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= n_sf) return;
  __shared__ uint32_t s_bits[2][RS_DL_WIDE_WORDS];
  __shared__ double s_shift[4];
  __shared__ uint32_t s_scr;
  const int r0 = rows[2 * g], r1 = rows[2 * g + 1];         // the same for the whole workgroup
  double corr[3] = {0.0, 0.0, 0.0}, margin = 0.0;
  int cfi = 0;
  if (r0 >= 0 && (ports != 4 || r1 >= 0)) {
    const int sf = g % 10;
    if (lane < 4) s_shift[lane] = 0.0;
    __syncthreads();
    if (lane < (ports == 4 ? 2 : 1)) rs_dl_row_wide(2 * sf, lane, id, cp_type, n_symb, n_rb, jump, s_bits[lane], s_shift);
    if (lane == 0) s_scr = pcf_scramble(sf, id, jump + 32);
    __syncthreads();
    const size_t ncol = (size_t)12 * n_rb;
    const double *row0 = reinterpret_cast<const double *>(grid + (size_t)r0 * ncol);
    const double *row1 = reinterpret_cast<const double *>(grid + (size_t)(ports == 4 ? r1 : r0) * ncol);
    const int e = lane & 15;
    cd2 y, ha, hb;
    pcf_elem(e, id, n_rb, ports, row0, row1, s_bits[0], s_bits[1], s_shift, &y, &ha, &hb);
    const cd2 hb_pair = mk(__shfl_xor(hb.re, 1), __shfl_xor(hb.im, 1)), y_pair = mk(__shfl_xor(y.re, 1), __shfl_xor(y.im, 1));
    const cd2 s = pcf_soft(e, ports, y, ha, hb_pair, y_pair);
    double v[PCF_NV], tot[PCF_NV];
    pcf_lane_values(e, s_scr, s, v);
#pragma unroll
    for (int i = 0; i < PCF_NV; ++i) tot[i] = meas_row_sum_lanes<PCF_LANES>(lane < 16 ? v[i] : 0.0);
    cfi = pcf_decide(tot, corr, &margin);
  }
  if (lane == 0) {
    out->cfi[g] = cfi;
    out->corr[g][0] = corr[0]; out->corr[g][1] = corr[1]; out->corr[g][2] = corr[2];
    out->margin[g] = margin;
  }
}

// the entries beyond n_sf, and the record's head from the entries in subframe order: one thread, no atomics
__global__ __launch_bounds__(PCF_LANES) void k_pcfich_fin(lcs_pcfich_info *__restrict__ out, int n_sf, int dl_mask, int n_rb, int ports) {
  const int tid = threadIdx.x;
  for (int g = n_sf + tid; g < PCF_MAX_SF; g += PCF_LANES) {
    out->cfi[g] = 0;
    out->corr[g][0] = out->corr[g][1] = out->corr[g][2] = 0.0;
    out->margin[g] = 0.0;
  }
  if (tid == 0) pcf_summary(out, n_sf, dl_mask, n_rb, ports);
}

// ------------------------------------------------------------------ launchers
int lcs_pcfich_stage_grid(lcs_ctx *c, const double *h_grid, size_t n_elem) {
  lcs_ctx::MeasWide &w = c->meas_wide;
  if (n_elem > w.grid.capacity()) {
    int rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));            // nothing reads the block that goes
    if ((rc = w.grid.reserve(c, n_elem))) return rc;
  }
  HIPCHK(c, hipMemcpyAsync(w.grid, h_grid, sizeof(double2) * n_elem, hipMemcpyHostToDevice, c->stream));
  return LCS_OK;
}

int lcs_launch_pcfich(lcs_ctx *c, const lcs_cell &cell, const int *rows, int n_sf, int n_rb, int dl_mask) {
  lcs_ctx::MeasWide &w = c->meas_wide;
  int rc;
  if (n_sf <= 0 || n_sf > PCF_MAX_SF) { c->err = "pcfich: no such number of subframes"; return LCS_ERR_BAD_ARG; }
  if ((rc = w.pcf_rows.reserve(c, (size_t)2 * PCF_MAX_SF)) || (rc = w.pcf_jump.reserve(c, 64)) || (rc = w.pcf_rec.reserve(c, 1))) return rc;
  for (int i = 0; i < 2 * n_sf; ++i) w.h_pcf_rows[i] = rows[i];
  HIPCHK(c, hipMemcpyAsync(w.pcf_rows, w.h_pcf_rows, sizeof(int) * 2 * n_sf, hipMemcpyHostToDevice, c->stream));
  if (w.pcf_jump_rb != n_rb) {
    // a quarter of the call: built when the bandwidth changes, not per call
    w.pcf_jump_rb = 0;
    lcs_tables::wide_jump_block(n_rb, w.h_pcf_jump);
    HIPCHK(c, hipMemcpyAsync(w.pcf_jump, w.h_pcf_jump, sizeof(w.h_pcf_jump), hipMemcpyHostToDevice, c->stream));
    w.pcf_jump_rb = n_rb;
  }
  const int n_symb = cell.cp_type == LCS_CP_NORMAL ? 7 : 6, id = cell.n_id_2 + 3 * cell.n_id_1, ports = pcf_ports(cell.n_ports);
  hipLaunchKernelGGL(k_pcfich, dim3(n_sf), dim3(PCF_LANES), 0, c->stream, (const double2 *)w.grid.get(), (const int *)w.pcf_rows.get(),
                     (const uint32_t *)w.pcf_jump.get(), w.pcf_rec.get(), n_sf, id, (int)cell.cp_type, n_symb, ports, n_rb);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_pcfich_fin, dim3(1), dim3(PCF_LANES), 0, c->stream, w.pcf_rec.get(), n_sf, dl_mask, n_rb, ports);
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}
