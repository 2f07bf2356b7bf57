// Every SIPX_* environment variable the library reads: one table (EnvKnobs), one reader (read_env_knobs).  No other file of
// csrc/ calls getenv.  The table is refreshed at every entry that begins something -- context creation, sipx_finalize,
// sipx_project, communicator creation, the standalone helpers of api.cpp -- and read through env_knobs() where a decision
// is made, never at a launch or inside an iteration: a test that sets a switch builds a new context afterwards.
// (INTEGRATION.md lists the same names with their values; tests/test_env_knobs.py keeps the two in step.)
// No HIP header: this file compiles with a plain host compiler.
#pragma once
#include <cstdlib>
#include <cstring>

namespace sipx {

// The raw values: clamps and combinations with properties of the problem stay where the value is used.
struct EnvKnobs {
  // ---- A/B switches of the launchers ----
  int cds_march = 1;              // SIPX_CDS_MARCH: 0 never, 2 also on grids too small to fill the chip (tests)
  long long cds_march_zchunk = 0; // SIPX_CDS_MARCH_ZCHUNK (with =2)
  long long multi_zchunk = 0;     // SIPX_MULTI_ZCHUNK: planes per chunk of the one-sweep y/l update (0: chosen by grid size)
  int rhs_march = 1;              // SIPX_RHS_MARCH: 0 never, 2 also on small grids
  long long rhs_march_zchunk = 0; // SIPX_RHS_MARCH_ZCHUNK (with =2)
  int q_plan = 1;                 // SIPX_Q_PLAN=0: the Q update regenerates every band value per element (k_q_update) instead of adding planned products
  int q_table = 1;                // SIPX_Q_TABLE=0: the z-marching products read Q's four stored bands instead of its class table
  // ---- A/B switches of the context (Engine constructor, finalize) ----
  int serial_sets = -1;           // SIPX_SERIAL_SETS: 1 y/l updates on the engine stream alone; any other value keeps the set streams whatever the grid size; -1 (unset): by grid size
  bool cds_full = false;          // SIPX_CDS_FULL=1: read all d bands of Q (no symmetric partner reads)
  bool slab_card_gather = false;  // SIPX_SLAB_CARD_GATHER=1: slab-decomposed, the cardinality set through an owner rank as well
  bool slab_dft_gather = false;   // SIPX_SLAB_DFT_GATHER=1: slab-decomposed, the l1-DFT set through an owner rank
  bool slab_local = true;         // SIPX_SLAB_LOCAL=0: slab-decomposed, full-size arrays on every rank
  int cg_fused = -1;              // SIPX_CG_FUSED: 0 / 1 force the one-kernel CG iteration off / on; -1 (unset): by grid size and matrix
  bool yl_multi = true;           // SIPX_YL_MULTI=0: one k_yl launch per set on every iteration
  int lean_multi = -1;            // SIPX_LEAN_MULTI: 0 / 1 the lean first passes of the l1 searches per set / in one sweep; -1 (unset): by grid size
  bool search_batch = true;       // SIPX_SEARCH_BATCH=0: the per-set search chains instead of the batched chain on the engine stream
  bool pass_multi = false;        // SIPX_PASS_MULTI=1: full first passes / fallback passes of the batched searches in one sweep per group (measured slower)
  bool spec_exchange = true;      // SIPX_SPEC_EXCHANGE=0: slab-decomposed, every search through (all-reduce, ..., all-gather)
  bool l1_sample = true;          // SIPX_L1_SAMPLE=0: no sampled prediction in front of an l1 search
  bool rank_lane = true;          // SIPX_RANK_LANE=0: the slice-rank / nuclear set in turn on the engine stream
  // ---- A/B switches of the library-backed projectors (read when a projector is built) ----
  bool dft_real = true;           // SIPX_DFT_REAL=0: the complex transform of the packed model
  int rank_subspace = 1;          // SIPX_RANK_SUBSPACE=0: the full decomposition on every call
  bool rank_cheb = true;          // SIPX_RANK_CHEB=0: plain subspace iteration only (spectra with a gap)
  bool rank_pack = true;          // SIPX_RANK_PACK=0: every filter on the whole batch
  bool rank_strict = false;       // SIPX_RANK_STRICT=1: Ritz pairs accepted at the strict level tol theta_max
  // ---- compatibility escapes ----
  bool comm_group = true;         // SIPX_COMM_GROUP=0: all-reduce and send/recv pairs never share one ncclGroup
  bool comm_selftest = true;      // SIPX_COMM_SELFTEST=0: skip the communicator's self-test in sipx_finalize
  bool gemm_tune = true;          // SIPX_GEMM_TUNE=0: the library's own choice of GEMM kernel (the cache of results stays per process)
  // ---- deployment ----
  int prefault_threads = -1;      // SIPX_PREFAULT_THREADS: threads that touch the destination of a large download (0: off; -1, unset: by core count)
  // ---- debugging aids ----
  int trace_kernels = 0;          // SIPX_TRACE_KERNELS=1: name every launch on stderr and drain the stream behind it
  int trace_searches = 0;         // SIPX_TRACE_SEARCHES=1: every threshold search of the batched chain that needed its fallback sweeps, on stderr
  int mark_stride = 0;            // SIPX_MARK_STRIDE: section timing marks on iterations 1-4 and every such iteration after them (<= 1: every iteration)
  int ext_debug = 0;              // SIPX_EXT_DEBUG: 1 the rank route of every call on stderr, 2 milliseconds per phase, 3 open matrices and Jacobi sweeps per step
  bool spec_debug = false;        // SIPX_SPEC_DEBUG (set at all): the verdicts and search states of the speculative exchange on stderr (synchronises)
  bool dft_debug = false;         // SIPX_DFT_DEBUG (set at all): the state the slab-decomposed DFT search ended in, per rank (synchronises)
  bool gemm_tune_debug = false;   // SIPX_GEMM_TUNE_DEBUG (set at all): every tuned GEMM shape with its candidates on stderr
  // ---- test hooks ----
  int finalize_fail_rank = -1;    // SIPX_FINALIZE_FAIL_RANK: this rank "runs out of memory" in sipx_finalize
  char comm_selftest_fail[32] = "";  // SIPX_COMM_SELFTEST_FAIL: "mapped" / "base" / "alltoall", optionally ":rank"
  long long gather_cap = 0;       // SIPX_GATHER_CAP: magnitudes an exchange segment holds (used when >= 4, rounded down to a multiple of 4)
  long long gather_fast_cap = 0;  // SIPX_GATHER_FAST_CAP: the same for the segments of the speculative exchange
  int l1_rounds_min = 0;          // SIPX_L1_ROUNDS_MIN: refinement rounds a slab-decomposed search enqueues at least (a problem whose brackets shrink slowly)
  int l1_rounds_max = 6;          // SIPX_L1_ROUNDS_MAX: ... at most (6 is the built-in limit; tests force an overflow with less)
  long long l1_sample_runs = 0;   // SIPX_L1_SAMPLE_RUNS: sampled runs of 64 grid points (0: by grid size; tests sample small grids too)
  bool rank_cert_check = false;   // SIPX_RANK_CERT_CHECK (set at all): both factorisations of the inertia certificate, compared matrix by matrix
};

// The parse rules, one per helper.  A value that is neither unset, "0" nor "1" is read as follows:
//   env_on      (default on):  off if and only if the value begins with '0'
//   env_off     (default off): on if and only if the value begins with '1'
//   env_number: atoll of the value (text without leading digits is 0); unset gives the default
//   env_is_set: "set at all means on", whatever the value (the debugging aids and SIPX_RANK_CERT_CHECK)
inline bool env_on(const char* name) { const char* e = std::getenv(name); return !(e && e[0] == '0'); }
inline bool env_off(const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; }
inline long long env_number(const char* name, long long dflt) { const char* e = std::getenv(name); return e ? std::atoll(e) : dflt; }
inline bool env_is_set(const char* name) { return std::getenv(name) != nullptr; }

inline EnvKnobs read_env_knobs() {
  EnvKnobs k;
  k.cds_march = (int)env_number("SIPX_CDS_MARCH", k.cds_march);
  k.cds_march_zchunk = env_number("SIPX_CDS_MARCH_ZCHUNK", k.cds_march_zchunk);
  k.multi_zchunk = env_number("SIPX_MULTI_ZCHUNK", k.multi_zchunk);
  k.rhs_march = (int)env_number("SIPX_RHS_MARCH", k.rhs_march);
  k.rhs_march_zchunk = env_number("SIPX_RHS_MARCH_ZCHUNK", k.rhs_march_zchunk);
  k.q_plan = (int)env_number("SIPX_Q_PLAN", k.q_plan);
  k.q_table = (int)env_number("SIPX_Q_TABLE", k.q_table);
  k.serial_sets = (int)env_number("SIPX_SERIAL_SETS", k.serial_sets);
  k.cds_full = env_off("SIPX_CDS_FULL");
  k.slab_card_gather = env_off("SIPX_SLAB_CARD_GATHER");
  k.slab_dft_gather = env_off("SIPX_SLAB_DFT_GATHER");
  k.slab_local = env_on("SIPX_SLAB_LOCAL");
  k.cg_fused = (int)env_number("SIPX_CG_FUSED", k.cg_fused);
  k.yl_multi = env_on("SIPX_YL_MULTI");
  k.lean_multi = (int)env_number("SIPX_LEAN_MULTI", k.lean_multi);
  k.search_batch = env_on("SIPX_SEARCH_BATCH");
  k.pass_multi = env_off("SIPX_PASS_MULTI");
  k.spec_exchange = env_on("SIPX_SPEC_EXCHANGE");
  k.l1_sample = env_on("SIPX_L1_SAMPLE");
  k.rank_lane = env_on("SIPX_RANK_LANE");
  k.dft_real = env_on("SIPX_DFT_REAL");
  k.rank_subspace = (int)env_number("SIPX_RANK_SUBSPACE", k.rank_subspace);
  k.rank_cheb = env_on("SIPX_RANK_CHEB");
  k.rank_pack = env_on("SIPX_RANK_PACK");
  k.rank_strict = env_off("SIPX_RANK_STRICT");
  k.comm_group = env_on("SIPX_COMM_GROUP");
  k.comm_selftest = env_on("SIPX_COMM_SELFTEST");
  k.gemm_tune = env_on("SIPX_GEMM_TUNE");
  k.prefault_threads = (int)env_number("SIPX_PREFAULT_THREADS", k.prefault_threads);
  k.trace_kernels = (int)env_number("SIPX_TRACE_KERNELS", k.trace_kernels);
  k.trace_searches = (int)env_number("SIPX_TRACE_SEARCHES", k.trace_searches);
  k.mark_stride = (int)env_number("SIPX_MARK_STRIDE", k.mark_stride);
  k.ext_debug = (int)env_number("SIPX_EXT_DEBUG", k.ext_debug);
  k.spec_debug = env_is_set("SIPX_SPEC_DEBUG");
  k.dft_debug = env_is_set("SIPX_DFT_DEBUG");
  k.gemm_tune_debug = env_is_set("SIPX_GEMM_TUNE_DEBUG");
  k.finalize_fail_rank = (int)env_number("SIPX_FINALIZE_FAIL_RANK", k.finalize_fail_rank);
  if (const char* e = std::getenv("SIPX_COMM_SELFTEST_FAIL")) std::strncpy(k.comm_selftest_fail, e, sizeof(k.comm_selftest_fail) - 1);
  k.gather_cap = env_number("SIPX_GATHER_CAP", k.gather_cap);
  k.gather_fast_cap = env_number("SIPX_GATHER_FAST_CAP", k.gather_fast_cap);
  k.l1_rounds_min = (int)env_number("SIPX_L1_ROUNDS_MIN", k.l1_rounds_min);
  k.l1_rounds_max = (int)env_number("SIPX_L1_ROUNDS_MAX", k.l1_rounds_max);
  k.l1_sample_runs = env_number("SIPX_L1_SAMPLE_RUNS", k.l1_sample_runs);
  k.rank_cert_check = env_is_set("SIPX_RANK_CERT_CHECK");
  return k;
}

// the table as of the last refresh (engine.cpp)
const EnvKnobs& env_knobs();
void refresh_env_knobs();

}  // namespace sipx
