// Host-side harness for the PBCH de-rate-matching tables of lte_tables.cpp -- the very functions lcs_create calls to build the
// `derm_inv` table that pbch_decode_wave reads: tests/test_pbch_host.py recovers the same map from the oracle's de-rate-matcher
// with one-hot inputs.  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/lte_tables.cpp"

extern "C" void pbch_host_deratematch_map(int n_e, uint8_t *out /*n_e*/) { lcs_tables::pbch_deratematch_map(n_e, out); }
extern "C" int pbch_host_derm_inv(int n_e, int16_t *out /*[120][16]*/) { return lcs_tables::pbch_derm_inv(n_e, out) ? 1 : 0; }
