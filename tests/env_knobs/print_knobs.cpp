// Prints every field of the table of SIPX_* switches as the reader fills it from this process's environment
// (tests/test_env_knobs.py compares the lines with what each switch meant before the table existed).
#include <cstdio>

#include "env_knobs.h"

int main() {
  const sipx::EnvKnobs k = sipx::read_env_knobs();
  std::printf("cds_march=%lld\n", (long long)k.cds_march);
  std::printf("cds_march_zchunk=%lld\n", (long long)k.cds_march_zchunk);
  std::printf("multi_zchunk=%lld\n", (long long)k.multi_zchunk);
  std::printf("rhs_march=%lld\n", (long long)k.rhs_march);
  std::printf("rhs_march_zchunk=%lld\n", (long long)k.rhs_march_zchunk);
  std::printf("q_plan=%lld\n", (long long)k.q_plan);
  std::printf("q_table=%lld\n", (long long)k.q_table);
  std::printf("serial_sets=%lld\n", (long long)k.serial_sets);
  std::printf("cds_full=%lld\n", (long long)k.cds_full);
  std::printf("slab_card_gather=%lld\n", (long long)k.slab_card_gather);
  std::printf("slab_dft_gather=%lld\n", (long long)k.slab_dft_gather);
  std::printf("slab_local=%lld\n", (long long)k.slab_local);
  std::printf("cg_fused=%lld\n", (long long)k.cg_fused);
  std::printf("yl_multi=%lld\n", (long long)k.yl_multi);
  std::printf("lean_multi=%lld\n", (long long)k.lean_multi);
  std::printf("search_batch=%lld\n", (long long)k.search_batch);
  std::printf("pass_multi=%lld\n", (long long)k.pass_multi);
  std::printf("spec_exchange=%lld\n", (long long)k.spec_exchange);
  std::printf("l1_sample=%lld\n", (long long)k.l1_sample);
  std::printf("rank_lane=%lld\n", (long long)k.rank_lane);
  std::printf("dft_real=%lld\n", (long long)k.dft_real);
  std::printf("rank_subspace=%lld\n", (long long)k.rank_subspace);
  std::printf("rank_cheb=%lld\n", (long long)k.rank_cheb);
  std::printf("rank_pack=%lld\n", (long long)k.rank_pack);
  std::printf("rank_strict=%lld\n", (long long)k.rank_strict);
  std::printf("comm_group=%lld\n", (long long)k.comm_group);
  std::printf("comm_selftest=%lld\n", (long long)k.comm_selftest);
  std::printf("gemm_tune=%lld\n", (long long)k.gemm_tune);
  std::printf("prefault_threads=%lld\n", (long long)k.prefault_threads);
  std::printf("trace_kernels=%lld\n", (long long)k.trace_kernels);
  std::printf("trace_searches=%lld\n", (long long)k.trace_searches);
  std::printf("mark_stride=%lld\n", (long long)k.mark_stride);
  std::printf("ext_debug=%lld\n", (long long)k.ext_debug);
  std::printf("spec_debug=%lld\n", (long long)k.spec_debug);
  std::printf("dft_debug=%lld\n", (long long)k.dft_debug);
  std::printf("gemm_tune_debug=%lld\n", (long long)k.gemm_tune_debug);
  std::printf("finalize_fail_rank=%lld\n", (long long)k.finalize_fail_rank);
  std::printf("comm_selftest_fail=%s\n", k.comm_selftest_fail);
  std::printf("gather_cap=%lld\n", (long long)k.gather_cap);
  std::printf("gather_fast_cap=%lld\n", (long long)k.gather_fast_cap);
  std::printf("l1_rounds_min=%lld\n", (long long)k.l1_rounds_min);
  std::printf("l1_rounds_max=%lld\n", (long long)k.l1_rounds_max);
  std::printf("l1_sample_runs=%lld\n", (long long)k.l1_sample_runs);
  std::printf("rank_cert_check=%lld\n", (long long)k.rank_cert_check);
  return 0;
}
