// Host engine behind the sipx C ABI: owns the device-resident PARSDMM state and drives the HIP
// kernels phase by phase, in the order of the reference's main loop (src/PARSDMM.jl:97-254).
// No CPU fallback exists: every numerical step below is a kernel launch.
#include "engine.h"
#include "comm.h"
#include "device_memory.h"
#include "dist_dft.h"
#include "ext_proj.h"
#include "host_prefault.h"
#include "set_config.h"
#include "solve_rules.h"
#include "sparse_granules.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <exception>

namespace sipx {

const LaunchObserver*& launch_observer() {
  static thread_local const LaunchObserver* obs = nullptr;
  return obs;
}

namespace {
EnvKnobs g_env_knobs;
}
const EnvKnobs& env_knobs() { return g_env_knobs; }
void refresh_env_knobs() { g_env_knobs = read_env_knobs(); }

namespace {

// every entry point that may be the first to touch the device asks here; returns the number of devices
int hip_device_count() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    throw std::runtime_error("libsipx: no HIP device visible -- this engine has no CPU fallback");
  return count;
}

// installs a context's observer for the duration of one entry point (the launchers consult it through launch_observer())
struct ObserverGuard {
  const LaunchObserver* prev;
  explicit ObserverGuard(const LaunchObserver* o) : prev(launch_observer()) { launch_observer() = o; }
  ~ObserverGuard() { launch_observer() = prev; }
};

constexpr int SLOTS = SET_SLOTS;      // reduction slots per set: 0..12 k_yl, 13 ||A'dy||^2, 14/15 two-pass feasibility

// ---- small values of the whole-solve loop ------------------------------------------------------------------------------------
static_assert(YL_FEAS == SIPX_YL_FEAS && YL_BB == SIPX_YL_BB && YL_FIRST == SIPX_YL_FIRST, "solve_rules.h numbers the flags like sipx.h");

// How one y/l update hands its sums to the host and whether its sweep may write the coming right-hand side: decided once per
// call (yl_step; the phase entry point sipx_update_y_l takes the default) and passed down to where it is acted on.
struct YlPlan {
  enum class Route {
    ByEvent,        // the host waits on an event recorded behind the reduction
    ByWord,         // one rank: the host spins on a pinned word the last workgroup of the reduction publishes (k_fin_sum)
    WithNextHead    // sharded: the all-reduce of the sums rides with the residual sums of the next x-step's head (argmin_x_head)
  };
  Route route = Route::ByEvent;
  bool collect_now = true;           // the update waits for its sums itself; off: the caller collects them later (collect_set_sums)
  bool fuse_rhs = false;             // rho cannot change before the next iteration: the sweep may write that iteration's rhs
};

// adds the host time of a scope to a section of log.timing (the host-only sections: bookkeeping, stop rule, rho / gamma rules)
struct HostSection {
  double& acc;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit HostSection(double& a) : acc(a) {}
  ~HostSection() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Section timing of the whole-solve loop: ONE chain of marks on the engine stream (a record costs the stream about 5 us); the
// time between two consecutive marks goes to the section named at the later one (-1: a mark that only opens an interval), four
// marks per step in the common path.  Two sets of marks, by parity of the step: a step never waits for its own timing, the
// marks of step i are resolved when step i + 2 begins.
// timing_ms: [0] initialization (host side) [1] rhs [2] argmin x [3] y/l update [4] stop rule [5] rho / gamma rules [6] Q update
// Grids of up to 2^23 points on one rank: the marks are recorded on iterations 1-4 and on every seventh after them (coprime
// with the usual rho_update_frequency 2 / 3 and with the feasibility estimate's 10, so that the sample holds plain,
// Barzilai-Borwein and feasibility iterations in their proportions), what they measure stands for the iterations since the
// last such one, and the sums of the y/l update are awaited on a pinned word instead of the record behind them (k_fin_sum).
// A record costs the stream up to 6 us -- two on a plain iteration, five on one that may change rho: 2048^2 2277 -> 2352 it/s,
// the buckets then estimates (within 12 % of the every-iteration figures over 35 iterations); at 256^3 the same buys 0.4 % and
// the buckets stay exact.  SIPX_MARK_STRIDE: 1 = every iteration, k = every k-th, whatever the grid.
// (sharded: every iteration, unless SIPX_MARK_STRIDE says otherwise -- a rank's share of the headline on eight GPUs through RCCL
//  with a world of one ran at 2215 it/s with the marks sampled and at 2219 without: its collectives leave gaps the records hide
//  in; the sums then keep an event of their own, ev_sums_, where the marks are left out)
// (round 5: every iteration by default at every size -- log.timing is a public field and means the same thing for every
//  caller; the sampling that round 4 switched on by itself for grids of up to 2^23 points is opt-in: SIPX_MARK_STRIDE=7)
struct SectionMarks {
  enum { MAXMARK = 12 };
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> ev;          // 2 x MAXMARK
  hipEvent_t open_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool open_valid[4] = {false, false, false, false};
  int step[2] = {0, 0};                // the step whose marks sit in a parity's slots
  double weight[2] = {1.0, 1.0};       // the iterations a timed step stands for
  int n[2] = {0, 0};
  int sec[2][MAXMARK];
  int stride = 1, maxit = 0, last_timed = 0, par = 0;      // of the solve / the step in progress
  bool timed = false;

  void create(hipStream_t s) {
    stream = s;
    for (int k = 0; k < 2 * MAXMARK; ++k) {
      hipEvent_t e;
      SIPX_HIP(hipEventCreate(&e));
      ev.push_back(e);
    }
  }
  void destroy() {
    for (hipEvent_t e : open_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  void begin_solve(int maxit_) {
    stride = env_knobs().mark_stride > 0 ? env_knobs().mark_stride : 1;
    maxit = maxit_;
    last_timed = 0;
    for (bool& v : open_valid) v = false;
    weight[0] = weight[1] = 1.0;
  }
  void reset() {                       // sipx_reset: whatever a solve that ended in an error left behind
    begin_solve(0);
    n[0] = n[1] = 0;
    step[0] = step[1] = 0;
  }
  bool is_timed(int it) const { return it <= maxit && (stride <= 1 || it <= 4 || it % stride == 0); }
  void begin_step(int i) {
    par = i & 1;
    step[par] = i;
    timed = is_timed(i);
    if (timed) {
      weight[par] = (double)(i - last_timed);
      last_timed = i;
    }
  }
  void mark(int section) {
    if (!timed || n[par] >= MAXMARK) return;
    SIPX_HIP(hipEventRecord(ev[par * MAXMARK + n[par]], stream));
    sec[par][n[par]++] = section;
  }
  // the latest mark of the step in progress (nullptr: it has none)
  hipEvent_t last_event() const { return timed && n[par] > 0 ? ev[par * MAXMARK + n[par] - 1] : nullptr; }
  // the event a timed step's first interval starts from (round 4: the first mark of a step used to open nothing when the residual
  // product had been queued ahead, and the x-step of every such iteration went uncounted -- "argmin x" read 0.21 of 0.5 ms)
  // (four slots, by step: the opening of step i + 1 is recorded during step i, before the marks of step i - 1 are resolved)
  void open(int at_step) {
    if (!is_timed(at_step)) return;
    const int k = at_step & 3;
    if (!open_ev[k]) SIPX_HIP(hipEventCreate(&open_ev[k]));
    SIPX_HIP(hipEventRecord(open_ev[k], stream));
    open_valid[k] = true;
  }
  void resolve(sipx_log* log, int parity) {
    const int cnt = n[parity];
    const int slot = step[parity] & 3;
    if (!cnt) { open_valid[slot] = false; return; }
    n[parity] = 0;
    SIPX_HIP(hipEventSynchronize(ev[parity * MAXMARK + cnt - 1]));
    hipEvent_t prev = open_valid[slot] ? open_ev[slot] : nullptr;
    open_valid[slot] = false;
    const double w = weight[parity] > 0 ? weight[parity] : 1.0;
    for (int k = 0; k < cnt; ++k) {
      hipEvent_t e = ev[parity * MAXMARK + k];
      if (sec[parity][k] >= 0 && prev) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, prev, e) == hipSuccess) log->timing_ms[sec[parity][k]] += w * ms;
        else (void)hipGetLastError();
      }
      prev = e;
    }
  }
};

// A set of a context: what its descriptor fixed (SetConfig, set_config.h) and, below, what finalize and the solve own -- device
// arrays, the decomposition's routing, streams, events and warm starts.
template <typename T>
struct SetState : SetConfig<T> {
  SetState() = default;
  explicit SetState(SetConfig<T>&& c) : SetConfig<T>(std::move(c)) {}
  // rho changed since this set's last l1 search: v is rescaled and theta moves like 1/rho -- by rescale_factor
  bool rescaled(T rho) const { return this->prox == PX_L1 && last_rho > T(0) && last_rho != rho; }
  double rescale_factor(T rho) const { return (double)last_rho / (double)rho; }
  // device copies of a caller-supplied sparse operator (SIPX_OP_CSC): CSC, the CSR copy, and s = A x
  long long *d_colptr = nullptr, *d_rowval = nullptr, *d_rowptr = nullptr, *d_colidx = nullptr;
  T *d_nzval = nullptr, *d_rval = nullptr, *sbuf = nullptr;
  // a matrix-free term of Q.  mf_rho: the set's current rho_i as Q holds it (assemble_Q, q_update); mf_t: A p of a product (M values).
  T mf_rho = T(0);
  int *mf_colptr = nullptr, *mf_rowidx = nullptr, *mf_rowptr = nullptr, *mf_colidx = nullptr;
  T* mf_t = nullptr;
  MfOp<T> mfA, mfAt;                 // CSR copy (t = A p), CSC arrays (A' t)
  bool is_dist = false, owned = true;
  bool in_sweep = false;             // the one-sweep update (k_yl_multi) takes this set; the others keep their per-set kernels
  // y, l: the arrays holding the current iterate; y0, l0: the other pair.  The snapshot (y_0, l_0) of the BB rule lives
  // in whichever pair `snap` names: on a snapshot iteration the update is written over the old snapshot (after it has
  // been read), on the others into the pair that is not the snapshot -- the reference's copies y_0 <- y, l_0 <- l never
  // happen (PARSDMM.jl:174-177,200-203).
  T *y = nullptr, *l = nullptr, *dy = nullptr, *lh0 = nullptr, *y0 = nullptr, *s0 = nullptr, *l0 = nullptr;
  T *y2 = nullptr, *l2 = nullptr;    // third pair of the one-sweep update (allocated by sipx_finalize, see sweep_launch)
  int snap = -1;                     // -1: no snapshot yet; 0: (y, l) is also the snapshot; 1: (y0, l0) is
  T *lb = nullptr, *ub = nullptr, *ata = nullptr;
  // vectors sipx_set_data_dev handed over before sipx_finalize, as given (device copies; finalize expands and frees them)
  T *pend_lb = nullptr, *pend_ub = nullptr;
  int searches_done = 0;             // slab-decomposed l1 searches of this set so far (sizes the refinement rounds)
  // Sharded solve: a rank / nuclear-norm set on the slices orthogonal to the last grid dimension is projected by ALL ranks,
  // each factorising the slices of its z-slab (`ext` is then built for the slab on every rank, owner or not)
  bool dist_ext = false;
  int owner_rank = 0;
  // Slab-decomposed solve (round 5, the long lists: BASELINE config 4): y, l of EVERY set live on the ranks' z-slabs; a set whose
  // projector cannot work from sums over the grid is projected on a materialised v --
  //   slab_ext: slice-wise rank / nuclear norm on the z-slices of the identity: every rank projects the slices of its own slab,
  //             nothing crosses the fabric;
  //   fan:      everything else (a projector behind a transform, cardinality): rank fan_owner gathers v, projects the whole
  //             array, scatters P(v) back (two fan exchanges of N w bytes for that set; the others stay slab-local).
  //   slab_card: cardinality of the whole array: a search of its own through the slab collectives (all-reduced probe counts, the
  //             pairs inside the final bracket all-gathered: launch_chain, kernels_proj.hip), then the per-set update.
  //   slab_dft:  the l1 ball behind the DFT on a 3-D grid: the transform itself is slab-decomposed (dist_dft.h: 2-D transforms of
  //             the rank's planes, one all-to-all, 1-D transforms along z; the threshold through the slab collectives).
  bool slab_ext = false, fan = false, slab_card = false, slab_dft = false;
  std::shared_ptr<DistDft<T>> ddft;
  int fan_owner = 0;
  bool fan_on_side = false;          // this update's projection was queued on the fan stream
  T* fanv = nullptr;                 // a gathered set's own whole-size vector (v, then P(v)): its owner projects it on the fan stream
  hipEvent_t fan_ev = nullptr;       // ... and records this when P(v) is ready
  std::shared_ptr<ExtProj<T>> ext;
  ProjScalars<T>* ps = nullptr;    // scalars of prox_i (warm-started across iterations)
  ProjScalars<T>* psf = nullptr;   // scalars of the feasibility estimate P_i(A_i x)
  double sums[SLOTS] = {0};
  bool bb_valid = false;
  T last_rho = T(-1), last_gamma = T(-1);   // parameters of the previous y/l update (speculation of the l1 search)
  // y/l updates of different sets are independent (the reference runs them on separate workers): the sets are dealt onto
  // a small pool of HIP streams, each with private search scratch, so the one-workgroup decide / solve kernels of one l1
  // search overlap with the streaming passes of another set instead of leaving the GPU idle
  hipStream_t st = nullptr;
  hipEvent_t ev = nullptr;
  long long cbuf_len = 0;            // elements cbuf holds
  double* ptmp = nullptr;
  T *mpart = nullptr, *cbuf = nullptr;
};

}  // namespace

template <typename T>
class Engine : public EngineBase {
 public:
  Engine(int ndim, const int64_t* n, const double* h, int device) : device_(device) {
    const ConfigCtx grid = grid_ctx<T>(ndim, n, h);      // (refuses a grid before anything is created for it)
    ndim_ = grid.ndim;
    G_ = grid.G;
    for (int a = 0; a < 3; ++a) ih_[a] = (T)grid.ih[a];
    SIPX_HIP(hipSetDevice(device));
    SIPX_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    SIPX_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
    SIPX_HIP(hipEventCreateWithFlags(&ev_fork2_, hipEventDisableTiming));
    set_streams_ = env_knobs().serial_sets != 1;
    // Up to 2^22 grid points the kernels of the searches are too short for a second stream to hide anything: the cross-stream
    // dependencies (an event wait costs 15-25 us on this stack) outweigh the overlap.  2048^2, C2: 2130 -> 2300 it/s on one
    // stream; 256^3 gains 6 % from its three.  SIPX_SERIAL_SETS=0 keeps the streams whatever the size.
    if (G_.N <= (1ll << 22) && env_knobs().serial_sets < 0) set_streams_ = false;
  }
  ~Engine() override {
    (void)hipSetDevice(device_);
    if (lane_thr_.joinable()) lane_thr_.join();
    if (lane_st_) { (void)hipStreamSynchronize(lane_st_); (void)hipStreamDestroy(lane_st_); }
    for (hipEvent_t e : {lane_fork_, lane_ev_}) if (e) (void)hipEventDestroy(e);
    if (fan_st_) { (void)hipStreamSynchronize(fan_st_); (void)hipStreamDestroy(fan_st_); }
    if (fan_fork_) (void)hipEventDestroy(fan_fork_);
    (void)hipStreamSynchronize(stream_);
    for (auto& s : sets_) free_set(s);
    comm_.reset();
    if (cstream_) (void)hipStreamDestroy(cstream_);
    for (auto e : ev_c_) if (e) (void)hipEventDestroy(e);
    if (ev_sums_) (void)hipEventDestroy(ev_sums_);
    if (ev_cgb_) (void)hipEventDestroy(ev_cgb_);
    for (const PinnedBlock& b : pinned_blocks()) if (*b.p) (void)hipHostFree(*b.p);
    marks_.destroy();
    for (auto e : stat_ev_) (void)hipEventDestroy(e);
    for (auto e : cg_ev_) if (e) (void)hipEventDestroy(e);
    for (hipStream_t q : pool_) if (q != stream_) (void)hipStreamDestroy(q);
    if (ev_io_in_) (void)hipEventDestroy(ev_io_in_);
    if (ev_io_out_) (void)hipEventDestroy(ev_io_out_);
    if (ev_fork_) (void)hipEventDestroy(ev_fork_);
    if (ev_fork2_) (void)hipEventDestroy(ev_fork2_);
    (void)hipStreamDestroy(stream_);
  }      // (the device arrays go with mem_, a projector's with the projector)

  // ------------------------------------------------------------------------------------------
  int add_set(const sipx_set_desc* d, const void* ata_R, const int64_t* ata_off, int d_i) override {
    if (finalized_) throw std::runtime_error("sipx_add_set after sipx_finalize");
    sets_.emplace_back(configure_set<T>(config_ctx(), d, ata_R, ata_off, d_i));
    need_ext_ |= sets_.back().needs_ext_scratch;       // the context's scratch is decided by the sets it was given
    need_idx_ |= sets_.back().needs_index_scratch;
    return (int)sets_.size() - 1;
  }
  // what the descriptor rules (set_config.h) read from this context, as it stands now
  ConfigCtx config_ctx() const {
    return ConfigCtx{ndim_, G_, {(double)ih_[0], (double)ih_[1], (double)ih_[2]}, !(comm_ || slab_req_ || !owned_.empty())};
  }

  int64_t set_rows(int set) override {
    if (set == (int)sets_.size() && !finalized_) return G_.N;   // the distance term to come
    if (set < 0 || set >= (int)sets_.size()) throw std::runtime_error("set index out of range");
    return sets_[set].Mtrue;
  }
  void num_terms(int* p, int* pp) override {
    if (p) *p = p_n_;
    if (pp) *pp = pp_n_;
  }
  void set_owned(const int32_t* owned) override {
    if (finalized_) throw std::runtime_error("sipx_set_owned must precede sipx_finalize");
    owned_.assign(owned, owned + sets_.size() + 1);
  }

  void set_decomp(int mode) override {
    if (finalized_) throw std::runtime_error("sipx_set_decomp must precede sipx_finalize");
    if (mode != SIPX_DECOMP_SETS && mode != SIPX_DECOMP_SLAB && mode != SIPX_DECOMP_SLAB_FULL) throw std::runtime_error("unknown decomposition");
    slab_req_ = mode != SIPX_DECOMP_SETS;
    slab_full_req_ = mode == SIPX_DECOMP_SLAB_FULL;
  }

  void set_comm(Comm* c) override {
    std::unique_ptr<Comm> hold(c);
    if (finalized_) throw std::runtime_error("the communicator must be attached before sipx_finalize");
    counting_ = c ? new CountingComm(hold.release()) : nullptr;      // (owns c)
    comm_.reset(counting_);
  }
  void comm_info(int* nranks, int* rank, char* version, int version_len, int* decomposition) override {
    if (version && version_len > 0) version[0] = 0;
    if (nranks) *nranks = 1;
    if (rank) *rank = 0;
    if (decomposition) *decomposition = (finalized_ ? slab_ : (slab_req_ && comm_)) ? SIPX_DECOMP_SLAB : SIPX_DECOMP_SETS;
    if (comm_) comm_->info(nranks, rank, version, version_len > 0 ? (size_t)version_len : 0);
    else if (version && version_len > 0) std::snprintf(version, (size_t)version_len, "none");
  }
  void bind_device() override { SIPX_HIP(hipSetDevice(device_)); }
  void device_bytes(int64_t* context_bytes, int64_t* device_used, int64_t* device_total) override {
    SIPX_HIP(hipSetDevice(device_));
    size_t fr = 0, tot = 0;
    SIPX_HIP(hipMemGetInfo(&fr, &tot));
    if (context_bytes) {
      long long b = mem_.bytes();
      for (const auto& s : sets_) b += (s.ext ? s.ext->device_bytes() : 0) + (s.ddft ? s.ddft->device_bytes() : 0);
      *context_bytes = b;
    }
    if (device_used) *device_used = (int64_t)(tot - fr);
    if (device_total) *device_total = (int64_t)tot;
  }
  void slab(int64_t* row0, int64_t* row1, int64_t* chunk) override {
    need_final();
    if (row0) *row0 = r0_;
    if (row1) *row1 = r1_;
    if (chunk) *chunk = comm_ ? chunk_ : Nx_;
  }

  void set_q_mode(int mode) override {
    if (finalized_) throw std::runtime_error("sipx_set_q_mode must precede sipx_finalize");
    if (mode != SIPX_Q_CDS && mode != SIPX_Q_STENCIL) throw std::runtime_error("unknown Q mode");
    stencil_q_ = mode == SIPX_Q_STENCIL;
  }

  // ------------------------------------------------------------------------------------------
  // sipx_finalize, step by step.  What the steps hand on that is not state of the context:
  struct FinalizePlan {
    long long Npad = 0;          // length of a vector of the exchange layout (world equal chunks; N without a communicator)
    long long fullpad = 0;       // what a whole vector of the exchange layout takes: the owner of a gathered set
    bool sparse_wanted = false;  // slab-decomposed: the list allows sparse arrays and the device can map them
  };
  void finalize(const void* m, const double* rho_ini, int n_rho, double gamma_ini, int feasibility_only,
                int zero_ini_guess, const void* x0, const void* const* l0, const void* const* y0,
                double* feasibility_initial) override {
    if (finalized_) throw std::runtime_error("sipx_finalize called twice");
    SIPX_HIP(hipSetDevice(device_));
    refresh_env_knobs();                  // the launchers' A/B switches: read once per context, not per launch
    feasibility_only_ = feasibility_only != 0;
    const ConfigCtx ctx = config_ctx();     // (a communicator, a decomposition or ownership may have come after the sets)
    for (const auto& s : sets_) {
      if (s.seg_radii) refuse_sharded(ctx, Sharded::RADII);
      if (s.op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
      if (s.ext_kind == EXT_L21 || s.ext_kind == EXT_L21_SEG || s.ext_kind == EXT_L21_JOINT || s.ext_kind == EXT_TNV) refuse_sharded(ctx, Sharded::L21);
      if (s.ext_kind == EXT_L21_GROUPS) refuse_sharded(ctx, Sharded::L21_GROUPS);
      if (s.ext_kind == EXT_L1_WEIGHTED) refuse_sharded(ctx, Sharded::L1_WEIGHTED);
      if (s.ext_kind == EXT_SIMPLEX_SEG) refuse_sharded(ctx, Sharded::SIMPLEX);
      if (s.ext_kind == EXT_CARD_GROUPS) refuse_sharded(ctx, Sharded::CARD_GROUPS);
      if (s.ext_kind == EXT_L20 || s.ext_kind == EXT_L20_SEG || s.ext_kind == EXT_L20_JOINT) refuse_sharded(ctx, Sharded::L20);
      if (s.ext_kind == EXT_L21_STACKED) refuse_sharded(ctx, Sharded::L21_STACKED);
      if (is_l2inf(s.ext_kind)) refuse_sharded(ctx, Sharded::L2INF);
    }
    FinalizePlan P;
    plan_sets();
    init_rho_gamma(rho_ini, n_rho, gamma_ini);
    plan_layout(P);
    const bool warm = !zero_ini_guess;     // PARSDMM_initialize.jl:304-313
    all_ranks_or_none([&] {
      plan_sparse_windows(P);
      plan_sweep_and_streams();
      alloc_iterate_arrays(P, m);
      alloc_scratch_and_partials(P);
      for (int i = 0; i < p_n_; ++i) init_set(i, P, warm ? l0 : nullptr, warm ? y0 : nullptr);
      if (search_batch_) {                    // the sets' header segments and decision registers of the batched searches
        int n2 = 0;
        for (auto& s : sets_) n2 += s.two_pass ? 1 : 0;
        fbuf_ = mem_.alloc<T>((size_t)n2 * fast_hdr<T>(), Mem::State);
        stage_ = mem_.alloc<double>((size_t)n2 * (PREP_SLOTS + 1 + 2), Mem::State);
      }
      if (dev_io_) {
        import_dev(m, warm ? x0 : nullptr, warm ? l0 : nullptr, warm ? y0 : nullptr);
      } else if (warm && x0) {                 // Minkowski: [u; v], 2N entries (sparse arrays: the rank's share)
        const long long c0 = slab_local_ ? std::max<long long>(0, wlo_) : 0, c1 = slab_local_ ? std::min<long long>(Nx_, whi_) : Nx_;
        if (c1 > c0) {
          SIPX_HIP(hipMemcpy(x_ + c0, (const T*)x0 + c0, (c1 - c0) * sizeof(T), hipMemcpyHostToDevice));
          io_h2d_ += (c1 - c0) * (long long)sizeof(T);
        }
      }
      assemble_Q();
      build_q_table();
      create_lane(P);
      if (!comm_ && !ev_io_in_) set_caller_stream((void*)caller_);      // (the events of the device-resident calls: none is created later)
    });
    finalized_ = true;
    initial_feasibility(feasibility_initial);
    for (auto& s : sets_) {                   // (read by now: the initial feasibility has waited for the engine stream)
      mem_.release(s.pend_lb); mem_.release(s.pend_ub);
      s.pend_lb = s.pend_ub = nullptr;
    }
  }

  // step 1: the set list as the solve sees it (the distance term appended), what it allows, which decomposition it gets
  void plan_sets() {
    pp_n_ = (int)sets_.size();
    if (!feasibility_only_) {             // PARSDMM_precompute_distribute.jl:17-26: identity operator for 1/2||x-m||^2
      SetState<T> s;
      configure_op(config_ctx(), s, SIPX_OP_IDENTITY);
      s.prox = PX_DIST;
      s.is_dist = true;
      s.ata_off = {0};
      sets_.push_back(std::move(s));
    }
    p_n_ = (int)sets_.size();
    {
      int with = 0;
      for (int i = 0; i < pp_n_; ++i) with += sets_[i].comp != 0;
      if (with != 0 && with != pp_n_) throw std::runtime_error("either every set names its Minkowski component or none does");
      mk_ = with > 0;
      if (mk_ && !feasibility_only_) sets_.back().comp = 3;        // distance term [I I]
      if (mk_ && stencil_q_) throw std::runtime_error("the stencil form of Q is not available for Minkowski sets");
      if (mk_ && !owned_.empty()) throw std::runtime_error("set sharding is not available for Minkowski sets");
      if (mk_)
        for (auto& st : sets_) st.ata_off = default_ata_offsets(config_ctx(), st);
    }
    for (int i = 0; i < p_n_; ++i) {
      if (!sets_[i].mfree) continue;
      const std::string who = "set " + std::to_string(i) + " is a custom sparse operator (SIPX_OP_CSC) passed without its A'A, a matrix-free term of Q: ";
      if (stencil_q_) throw std::runtime_error(who + "the stencil form of Q has no place for it -- use SIPX_Q_CDS (Q_mode = \"cds\")");
      if (comm_) throw std::runtime_error(who + "a sharded solve (either decomposition) has no form for it -- solve on one device, or pass the operator's A'A in CDS if it has at most " +
                                          std::to_string(MAXD) + " bands");
      if (mk_) throw std::runtime_error(who + "Minkowski components are not available for it -- use the built-in operators for Minkowski sets");
      ++n_mfree_;
    }
    Nx_ = mk_ ? 2 * G_.N : G_.N;
    if (Nx_ >= (1ll << 31)) throw std::runtime_error("2^31 unknowns or more are not supported");
    if (p_n_ > 99) throw std::runtime_error("at most 99 sets (PARSDMM_initialize.jl:217)");
    if (comm_) {                            // this context is one rank of a sharded solve
      if (mk_) throw std::runtime_error("the sharded solve is not available for Minkowski sets");
      if (stencil_q_) throw std::runtime_error("the sharded solve needs the CDS form of Q");
      if (owned_.empty()) {                 // PARSDMM_initialize.jl:78-80 deals one set per worker; here round robin
        owned_.resize(p_n_);
        for (int i = 0; i < p_n_; ++i) owned_[i] = (i % comm_->world) == comm_->rank;
      }
    }
    if (!owned_.empty())
      for (int i = 0; i < p_n_; ++i) sets_[i].owned = owned_[i] != 0;
    // Slab decomposition of the WHOLE iteration (sipx_set_decomp): every rank holds every set and works on its z-slab of the
    // globally indexed arrays; no N-vector crosses the fabric any more.  For the sets whose projector needs no
    // more than sums over the grid: element-wise ones, l1 / l2 balls and the annulus on the identity or D_x / D_y / D_z / TV.
    slab_ = slab_req_ && comm_ != nullptr;
    if (!slab_) return;
    if (mk_ || stencil_q_) throw std::runtime_error("the slab decomposition is not available for Minkowski contexts or the stencil form of Q");
    int nfan = 0;
    for (int i = 0; i < p_n_; ++i) {
      SetState<T>& s = sets_[i];
      if (s.custom)
        throw std::runtime_error("the slab decomposition has no form for a caller-supplied sparse operator (set " + std::to_string(i) + "): use the set decomposition");
      // (SIPX_SLAB_CARD_GATHER=1 / SIPX_SLAB_DFT_GATHER=1: cardinality / the l1-DFT set through an owner rank as well -- A/B switches, tests)
      if (s.sliced_on_last_dim(ndim_)) s.slab_ext = true;
      else if (s.prox == PX_CARD && !s.ext_kind && !env_knobs().slab_card_gather) s.slab_card = true;
      else if (s.ext_kind == EXT_L1_DFT && ndim_ == 3 && s.ident && G_.n[0] >= 2 && !env_knobs().slab_dft_gather) s.slab_dft = true;
      else if (s.ext_kind || s.prox == PX_CARD) { s.fan = true; s.fan_owner = (nfan++) % comm_->world; }
      if (s.fan && s.nblk > 1) throw std::runtime_error("internal: a gathered set with more than one operator block");
      slab_loose_ |= s.slab_ext || s.fan || s.slab_card || s.slab_dft;
      s.owned = true;
    }
    // (the searches with their collectives run on the engine stream, in one order on every rank; the y/l updates that
    // follow have no collectives inside and are dealt onto the set streams as usual)
  }

  // step 2 (and sipx_reset): rho, gamma at their initial values (PARSDMM_initialize.jl:58-63,107-114,159)
  void init_rho_gamma(const double* rho_ini, int n_rho, double gamma_ini) {
    rho_.resize(p_n_);
    gamma_.resize(p_n_);
    if (n_rho == 1) std::fill(rho_.begin(), rho_.end(), (T)rho_ini[0]);
    else if (n_rho == p_n_) for (int i = 0; i < p_n_; ++i) rho_[i] = (T)rho_ini[i];
    else throw std::runtime_error("rho_ini must have 1 or p entries");
    T g0 = (T)gamma_ini;
    any_ncvx_ = false;
    for (int i = 0; i < pp_n_; ++i) any_ncvx_ |= sets_[i].ncvx != 0;
    if (any_ncvx_) g0 = T(0.75);
    std::fill(gamma_.begin(), gamma_.end(), g0);
  }

  // step 3: halo, the rank's slab and the grids of its kernels, whether sparse arrays are wanted; the communicator's self-test
  void plan_layout(FinalizePlan& P) {
    const long long N = G_.N;
    // Q offsets first: the SpMV inputs (x, p) carry a zero halo of max|offset| on both sides so that the
    // kernels need no bounds checks on neighbour loads
    plan_Q_offsets();
    halo_ = 4;
    for (int b = 0; b < cds_.d; ++b) halo_ = std::max<long long>(halo_, std::llabs(cds_.off[b]));
    for (int a = 0; a < 3; ++a) halo_ = std::max<long long>(halo_, G_.st[a]);
    halo_ = (halo_ + 3) / 4 * 4;
    r0_ = 0; r1_ = Nx_;
    P.Npad = Nx_;
    if (comm_) {
      // z-slabs of the x-step: ceil(n_last / world) planes per rank (the last ranks may hold fewer, or none); the exchange
      // buffers (rhs, x) are padded to world equal chunks, the pad stays zero
      const long long nlast = G_.n[ndim_ - 1];
      plane_ = N / nlast;
      long long maxoff = 0;
      for (int b = 0; b < cds_.d; ++b) maxoff = std::max<long long>(maxoff, std::llabs(cds_.off[b]));
      if (maxoff > plane_) throw std::runtime_error("the sharded solve needs operators whose A'A reaches no further than one plane of the grid");
      const long long planes = (nlast + comm_->world - 1) / comm_->world;
      chunk_ = planes * plane_;
      P.Npad = chunk_ * comm_->world;
      r0_ = std::min<long long>(N, (long long)comm_->rank * chunk_);
      r1_ = std::min<long long>(N, (long long)(comm_->rank + 1) * chunk_);
      prev_ = (r0_ > 0 && r0_ < N) ? comm_->rank - 1 : -1;
      next_ = (r1_ < N && r1_ > r0_) ? comm_->rank + 1 : -1;
      qr0_ = r1_ > r0_ ? std::max<long long>(0, r0_ - maxoff) : 0;      // the symmetric read reaches |offset| rows back
      qr1_ = r1_ > r0_ ? r1_ : 0;
      SIPX_HIP(hipStreamCreateWithFlags(&cstream_, hipStreamNonBlocking));
      for (auto& e : ev_c_) SIPX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    } else {
      qr0_ = 0; qr1_ = N;
    }
    Gr_ = G_;
    Gyl_ = G_;
    if (slab_) {
      Gr_.e0 = r0_; Gr_.e1 = r1_;
      // k_yl recomputes the last plane of the rank below (y, l of a difference along the slab direction are read one plane
      // back by the adjoint stencils): bit for bit what that rank computes, instead of an exchange of y, l and y - y_old
      Gyl_.e0 = (prev_ >= 0) ? r0_ - plane_ : r0_; Gyl_.e1 = r1_; Gyl_.s0 = r0_;
      if (r1_ <= r0_) { Gr_.e0 = Gr_.e1 = 0; Gyl_.e0 = Gyl_.e1 = 0; }
    }
    wlo_ = -halo_; whi_ = P.Npad + halo_;
    if (slab_ && !slab_full_req_) {
      int vmm = 0;
      (void)hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, device_);
      P.sparse_wanted = vmm != 0 && env_knobs().slab_local && list_allows_sparse();      // SIPX_SLAB_LOCAL=0: full-size arrays on every rank (A/B switch)
      // (lists with materialised sets keep sparse arrays too: their vectors are addressed by global index -- loose_v_ / loose_w_ --
      //  and whole only on the rank that projects a gathered set)
    }
    if (comm_) {                                            // (every rank takes the same branch: the verdict is all-reduced)
      bool any_dft = false;
      for (const auto& st : sets_) any_dft |= st.slab_dft;
      comm_self_test(P.sparse_wanted, any_dft);
      if (selftest_alltoall_failed_) {       // the transposition of the slab-decomposed DFT does not work here: an owner rank projects such sets
        int nfan = 0;
        for (auto& st : sets_) nfan += st.fan ? 1 : 0;
        for (auto& st : sets_)
          if (st.slab_dft) { st.slab_dft = false; st.fan = true; st.fan_owner = (nfan++) % comm_->world; }
      }
    }
  }
  // per-element bound vectors arrive whole; the initial feasibility of an element-wise set on a difference operator
  // takes the whole-grid kernels: such lists keep full-size arrays
  bool list_allows_sparse() const {
    for (const auto& st : sets_)
      if (st.prox == PX_BOUNDS_VEC || (!st.two_pass && st.nblk > 0) || !st.host_ata.empty()) return false;
    return true;
  }

  // Everything from the communicator's self-test to the initial feasibility allocates and uploads -- no collective.  A rank that
  // fails in there (out of device memory: the likeliest rank-local failure of a first multi-GPU run) must not throw by itself:
  // the others would go on into the collectives of the initial feasibility and wait for it for ever.  Every rank reports to one
  // all-reduce on the self-test's plain buffer and all of them throw together (bench.py then falls back to the next
  // decomposition on every rank).
  template <typename Steps>
  void all_ranks_or_none(Steps allocate_and_upload) {
    std::string alloc_err;
    try {
      if (comm_ && env_knobs().finalize_fail_rank == comm_->rank)       // SIPX_FINALIZE_FAIL_RANK (tests): this rank "runs out of memory"
        throw std::runtime_error("test hook: out of device memory");
      allocate_and_upload();
    } catch (const std::exception& ex) {
      if (!comm_ || comm_->world <= 1 || !agree_buf_) throw;
      alloc_err = ex.what();
    }
    if (!comm_ || comm_->world <= 1 || !agree_buf_) return;
    const double flag = alloc_err.empty() ? 0.0 : 1.0;
    double sum = flag;
    try {
      SIPX_HIP(hipMemcpy(agree_buf_, &flag, sizeof(double), hipMemcpyHostToDevice));
      comm_->allreduce_sum(agree_buf_, 1, SIPX_F64, stream_);
      SIPX_HIP(hipStreamSynchronize(stream_));
      SIPX_HIP(hipMemcpy(&sum, agree_buf_, sizeof(double), hipMemcpyDeviceToHost));
    } catch (const std::exception& ex) {
      throw std::runtime_error(std::string("sipx_finalize: the ranks could not agree on the outcome of their allocations (") + ex.what() + ")" +
                               (alloc_err.empty() ? "" : "; this rank: " + alloc_err));
    }
    if (sum != 0.0)
      throw std::runtime_error("sipx_finalize failed on " + std::to_string((int)sum) + " of " + std::to_string(comm_->world) + " ranks while allocating" +
                               (alloc_err.empty() ? std::string(" (not on this one)") : ": " + alloc_err));
  }

  // sparse arrays or not (the self-test's verdict is in), and the grid points [wlo_, whi_) a rank then backs with memory
  void plan_sparse_windows(const FinalizePlan& P) {
    if (!slab_ || slab_full_req_) return;
    slab_local_ = P.sparse_wanted && !selftest_mapped_failed_;
    if (!slab_local_) return;
    // what a rank's kernels touch: its planes, one plane behind (forward differences, the neighbour's copy of x and p), two
    // planes in front (the recomputed last plane of the rank below, and the plane the z-march loads in front of THAT one)
    const long long N = G_.N, a = r1_ > r0_ ? r0_ : N, b = r1_ > r0_ ? r1_ : N;
    wlo_ = std::max<long long>(-halo_, a - 2 * plane_ - 64);
    whi_ = std::min<long long>(P.Npad + halo_, b + plane_ + 64);
  }

  // step 4: which sets the sweep takes, how many set streams exist, whether the searches are batched (nothing is allocated)
  void plan_sweep_and_streams() {
    // x0 mode of the one-sweep update: when EVERY y/l update of this context goes through the sweep (its block layout is
    // compiled in, no set needs the per-set kernels on feasibility iterations), s_0 = A x_0 is recomputed from a snapshot of
    // x instead of being stored per set: two N-vectors instead of one M_i-vector per set, and 8 N w less traffic on every
    // Barzilai-Borwein iteration of the headline list.  (A list the sweep does not take whole keeps the per-set s_0 arrays.)
    yl_multi_ = env_knobs().yl_multi;            // SIPX_YL_MULTI=0: one k_yl launch per set on every iteration (A/B switch, tests)
    // the lean first passes of the l1 searches in one sweep: pays where the re-reads of x are real traffic (512^3, settled
    // iterations: 133 -> 139 it/s); at 256^3 three concurrent per-set passes on their own streams are as fast or faster
    // (1028 against 1012 it/s settled, default window equal), so it is the default above 2^24 grid points only
    lean_multi_ = env_knobs().lean_multi >= 0 ? env_knobs().lean_multi != 0 : G_.N > (1ll << 24);      // SIPX_LEAN_MULTI: A/B switch, tests
    {
      // which sets the sweep takes: all of them (the layouts of C2 / C3 / C5 and of the short lists), or -- one rank only -- the
      // element-wise and l1 / l2 terms of a list with sets it cannot take (C4), provided the layout of that subset is compiled in
      MultiArgs<T> probe0;
      const bool any_sweep = sweep_applicable(0, probe0, true);
      has_loose_ = false;
      for (auto& st : sets_) {
        st.in_sweep = any_sweep && sweep_eligible(st);
        has_loose_ |= any_sweep && st.owned && !st.in_sweep;
      }
      sweep_partial_ = has_loose_;
    }
    MultiArgs<T> probe;
    x0_mode_ = !has_loose_ && sweep_applicable(SIPX_YL_FEAS | SIPX_YL_BB, probe, true);
    // Set streams when the sweep does the updates: all that runs on them is the threshold / scale searches, chains of short
    // kernels whose latencies should overlap -- every searching set a stream of its own (up to three; one of them the engine
    // stream, so that its search starts without a cross-stream dependency), the other sets on the engine stream.  256^3, C3:
    // 715 -> 760 it/s with three instead of two; 512^3 unchanged; four lose (no search left on the engine stream); 2048^2 with
    // its one searching set keeps two.  Without the sweep the per-set y/l kernels run there too: two streams, sets dealt round robin.
    MultiArgs<T> probe2;
    search_streams_ = sweep_applicable(SIPX_YL_BB, probe2, true);
    if (search_streams_) {
      int ntp = 0;
      for (const auto& st : sets_) ntp += st.two_pass ? 1 : 0;
      n_set_streams_ = std::max(2, std::min(3, ntp));
    }
    {
      // One rank and EVERY update through the sweep: the searches of all two-pass sets as one chain of launches on the engine
      // stream (batched_searches) -- no set streams at all.  SIPX_SEARCH_BATCH=0 keeps the per-set chains (A/B switch, tests).
      int ntp = 0;
      for (const auto& st : sets_) ntp += (st.two_pass && st.in_sweep) ? 1 : 0;
      MultiArgs<T> probe3;
      search_batch_ = !comm_ && env_knobs().search_batch && ntp >= 1 && ntp <= SPEC_MAX_SETS &&
                      sweep_applicable(SIPX_YL_FEAS | SIPX_YL_BB, probe3, true);
      if (search_batch_) set_streams_ = false;
    }
    {
      MultiArgs<T> probe4;
      sweep_plain_ = sweep_applicable(0, probe4, true);
    }
    for (const auto& st : sets_) slab_dist_logs_ |= slab_ && !mk_ && st.is_dist;
    // (the snapshot of x of the x0 mode is a member of the ring of x buffers: nothing to allocate)
  }

  // step 5a: the vectors of the x-step, and m uploaded
  void alloc_iterate_arrays(const FinalizePlan& P, const void* m) {
    const long long N = G_.N, Npad = P.Npad;
    for (int k = 0; k < 3; ++k) { xr_base_[k] = galloc(Npad + 2 * halo_, halo_, 1, 0, Mem::State); xr_[k] = xr_base_[k] + halo_; }
    x_cur_ = 0; x_snap_ = -1;
    x_ = xr_[0]; xold_ = x_;                // (no x-step yet: x_old names x itself)
    p_base_ = galloc(Nx_ + 2 * halo_, halo_, 1, 0, Mem::State); p_ = p_base_ + halo_;
    rhs_ = galloc(Npad, 0, 1, 0, Mem::State);
    if (mk_) { w_base_ = mem_.alloc<T>(N + 2 * halo_, Mem::State); w_ = w_base_ + halo_; }   // u + v, read through the stencils
    m_base_ = galloc(N + 2 * halo_, halo_, 1, 0); m_ = m_base_ + halo_;   // forward stencils of A m read past the end
    r_base_ = galloc(Nx_ + 2 * halo_, halo_, 1, 0, Mem::State); r_ = r_base_ + halo_;      // (halo: the fused CG product reads r through the bands)
    Ap_ = galloc(Nx_, 0, 1, 0, Mem::State);
    {
      // CG iterations from the second on as ONE kernel (scalar step + product on p = r + beta p_old formed on the fly,
      // k_cds_fused): one launch and a host round trip less per iteration -- what a launch-bound grid (2048^2) is made of --
      // against a product that reads two vectors instead of one.  SIPX_CG_FUSED=0 / 1 forces it off / on.
      const int forced = env_knobs().cg_fused;
      const bool small = Nx_ <= (1ll << 23);
      // (the z-marching product has a fused form of its own, k_cds_march<MODE 3>: there the fusion also saves traffic -- 8 N w
      //  instead of the 9 of product + p-update -- so it is the default at every size for the matrices the march takes)
      // (a matrix-free term of Q has no fused form: the product is followed by the term's two kernels)
      cg_fused_ = !comm_ && !stencil_q_ && n_mfree_ == 0 && (forced >= 0 ? forced == 1 : (small || cds_.march != 0));
      if (cg_fused_) { p2_base_ = mem_.alloc<T>(Nx_ + 2 * halo_, Mem::State); p2_ = p2_base_ + halo_; }
    }
    const long long c0 = std::max<long long>(0, wlo_), c1 = std::min<long long>(N, whi_);      // (sparse arrays: the rank's share only)
    // (device-resident call: m arrives with the warm start, in the one launch of import_dev)
    if (c1 > c0 && !dev_io_) {
      SIPX_HIP(hipMemcpy(m_ + c0, (const T*)m + c0, (c1 - c0) * sizeof(T), hipMemcpyHostToDevice));
      io_h2d_ += (c1 - c0) * (long long)sizeof(T);
    }
  }

  // The pinned host blocks of a context {pointer, bytes, fill byte}: sipx_finalize allocates and fills them, sipx_reset fills
  // them again, the destructor frees them -- each walks this one table.
  struct PinnedBlock {
    void** p;
    size_t bytes;
    int fill;
  };
  std::array<PinnedBlock, 7> pinned_blocks() {
    const size_t np = (size_t)p_n_ + 1;
    return {{{(void**)&cg_host_, 2 * sizeof(CgState<T>), 0},
             {(void**)&ticket_, 64, 0xff},
             {(void**)&hres_, sizeof(double) * np * SLOTS, 0},
             {(void**)&sums_word_, 64, 0},
             {(void**)&hlean_, sizeof(int) * np, 0},
             {(void**)&hovf_, sizeof(int) * np, 0},
             {(void**)&hverd_, sizeof(unsigned) * np, 0}}};
  }

  // step 5b: the exchange buffers of the slab-decomposed searches, the engine-wide scratch, the partial sums, the pinned blocks
  void alloc_scratch_and_partials(FinalizePlan& P) {
    const long long N = G_.N, Npad = P.Npad;
    long long maxpad = N;
    for (auto& s : sets_) maxpad = std::max(maxpad, s.Mpad);
    if (comm_) {
      for (int i = 0; i < p_n_; ++i) {
        SetState<T>& s = sets_[i];
        s.owner_rank = i % comm_->world;
        if (!s.sliced_on_last_dim(ndim_) || slab_) continue;               // (slab-decomposed: SetState::slab_ext, no exchange at all)
        if (s.owned != (s.owner_rank == comm_->rank))
          throw std::runtime_error("a slice-wise rank / nuclear set is projected by all ranks: it needs the default set ownership (set i on rank i mod world)");
        s.dist_ext = true;
        need_ext_ = true;
        maxpad = std::max(maxpad, Npad);            // v travels through the padded exchange layout of x
      }
    }
    if (slab_loose_) need_ext_ = true;              // (the feasibility estimates keep a copy of s = A x)
    if (slab_) {
      maxpad = std::max(maxpad, Npad);              // slabs of y, l are gathered through the padded exchange layout at download
      hooks_.world = comm_->world; hooks_.rank = comm_->rank; hooks_.user = comm_.get();
      hooks_.allreduce_sum = [](void* u, double* buf, size_t n, hipStream_t q) { static_cast<Comm*>(u)->allreduce_sum(buf, n, SIPX_F64, q); };
      hooks_.allgather = [](void* u, void* buf, size_t chunk, int f64, hipStream_t q) {
        static_cast<Comm*>(u)->allgather(buf, chunk, f64 ? SIPX_F64 : SIPX_F32, q);
      };
      // what a search may gather inside its final bracket over ALL ranks (and the size of a rank's full-size exchange segment:
      // the all-gather moves whole segments): 2^17 magnitudes up to 256^3, N / 512 above (512^3: 2^18), at most 2^20
      hooks_.gcap = std::min<long long>(std::min<long long>(1ll << 20, std::max<long long>(1ll << 17, G_.N / 512)), (maxpad + 3) / 4 * 4);
      if (env_knobs().gather_cap >= 4) hooks_.gcap = env_knobs().gather_cap / 4 * 4;      // SIPX_GATHER_CAP (tests): a segment small enough to overflow
      int n2 = 0, nl1 = 0;
      for (auto& s : sets_) { n2 += s.two_pass ? 1 : 0; nl1 += (s.two_pass && s.prox == PX_L1) ? 1 : 0; }
      // the searches of all sets run in lock step: one staging buffer for their sums (one all-reduce per stage), one exchange
      // buffer with a segment per l1 set and rank (one all-gather)
      gbuf_ = mem_.alloc<T>((size_t)comm_->world * std::max(nl1, 1) * (hooks_.gcap + GATHER_HDR), Mem::State);
      hooks_.gbuf = gbuf_;
      // speculative exchange: a small segment per two-pass set and rank (header with the rank's sums + what its first pass
      // gathered inside the speculative range: a few thousand magnitudes once theta moves slowly)
      // (a rank's share of what the full-size segment holds, times two for uneven shares; at least 16 K values)
      hooks_.fcap = std::min<long long>(hooks_.gcap, std::max<long long>(1ll << 14, (2 * hooks_.gcap / comm_->world + 3) / 4 * 4));
      if (env_knobs().gather_fast_cap >= 4) hooks_.fcap = std::min<long long>(hooks_.gcap, env_knobs().gather_fast_cap / 4 * 4);      // SIPX_GATHER_FAST_CAP (tests)
      fbuf_ = mem_.alloc<T>((size_t)comm_->world * std::max(n2, 1) * (hooks_.fcap + fast_hdr<T>()), Mem::State);
      stage_ = mem_.alloc<double>((size_t)std::max(n2, 1) * (PREP_SLOTS + 1 + 2 * comm_->world), Mem::State);
      sstage_ = mem_.alloc<double>((size_t)std::max(n2, 1) * (2 * SAMPLE_BINS + 3), Mem::State);
    }
    P.fullpad = maxpad;
    if (slab_local_) {                 // the whole-array scratch is not needed: searches compact at most what the rank's planes hold
      int nbmax = 1;
      for (auto& s : sets_) nbmax = std::max(nbmax, s.nblk_or1());
      // (... or what the exchange of a search strings together from all ranks: at most gcap magnitudes, by the search's own rule)
      maxpad = std::min<long long>(maxpad, std::max<long long>((long long)nbmax * (whi_ - wlo_), hooks_.gcap + 64));
    }
    scr_v_ = mem_.alloc<T>(maxpad, Mem::State);
    scr_c_ = mem_.alloc<T>(maxpad, Mem::State);
    scr_c_len_ = maxpad;
    if (need_idx_) scr_i_ = mem_.alloc<long long>(maxpad, Mem::State);
    if (need_ext_) scr_w_ = mem_.alloc<T>(maxpad, Mem::State);
    // the vectors the materialised sets of a slab-decomposed list are stored into, addressed by GLOBAL index (v, P(v), s = A x and
    // its copy): the engine-wide scratch where that is whole; with sparse arrays a rank that projects a gathered set holds them
    // whole, every other rank its planes only
    loose_v_ = scr_v_; loose_w_ = scr_w_;
    if (slab_local_ && slab_loose_) {
      bool owner = false;
      for (auto& st : sets_) owner |= st.fan && st.fan_owner == comm_->rank;
      loose_whole_ = owner;
      loose_v_ = owner ? mem_.alloc<T>(P.fullpad) : loose_alloc(Npad);
      loose_w_ = owner ? mem_.alloc<T>(P.fullpad) : loose_alloc(Npad);
    }
    // (the reduced per-set sums sit right behind the CG partials: sharded, ONE all-reduce can carry both, see argmin_x_head)
    part_cg_ = mem_.alloc<double>(2 * NB + (size_t)(p_n_ + 1) * SLOTS, Mem::State);
    part_tmp_ = mem_.alloc<double>((size_t)(PREP_SLOTS + 2) * NB, Mem::State);
    part_sets_ = mem_.alloc<double>((size_t)(p_n_ + 1) * SLOTS * NB, Mem::State);   // + one group of slots for whole-x sums
    maxpart_ = mem_.alloc<T>(2 * NB, Mem::State);     // per-block max | per-block smallest non-zero magnitude
    cg_dev_ = mem_.alloc<CgState<T>>(1, Mem::State);
    dres_ = part_cg_ + 2 * NB;
    sums_ticket_ = mem_.alloc<unsigned>(1, Mem::State);
    for (const PinnedBlock& b : pinned_blocks()) {
      SIPX_HIP(hipHostMalloc(b.p, b.bytes, hipHostMallocDefault));
      std::memset(*b.p, b.fill, b.bytes);
    }
    for (int k = 0; k < 2; ++k) SIPX_HIP(hipEventCreateWithFlags(&cg_ev_[k], hipEventDisableTiming));
    SIPX_HIP(hipEventCreateWithFlags(&ev_cgb_, hipEventDisableTiming));
    SIPX_HIP(hipEventCreateWithFlags(&ev_sums_, hipEventDisableTiming));
    marks_.create(stream_);
  }

  // step 6: the device state of set i, its streams and scratch; step 7 for its own vectors: bounds and the warm start of l, y
  void init_set(int i, const FinalizePlan& P, const void* const* l0, const void* const* y0) {
    const long long N = G_.N;
    SetState<T>& s = sets_[i];
    // explicit AtA bands are kept on the device (every rank: Q is global); descriptor-generated
    // ones are never stored -- the fused Q update regenerates their values on the fly
    if (!s.host_ata.empty()) {
      s.ata = mem_.alloc<T>((size_t)N * s.ata_off.size(), Mem::NoFill);
      SIPX_HIP(hipMemcpy(s.ata, s.host_ata.data(), s.host_ata.size() * sizeof(T), hipMemcpyHostToDevice));
      io_h2d_ += (long long)(s.host_ata.size() * sizeof(T));
      s.host_ata.clear();
      s.host_ata.shrink_to_fit();
    }
    if ((s.dist_ext || s.slab_ext) && r1_ > r0_) {              // this rank's share of the slices: the projector on the slab grid
      ExtSpec sp = s.spec;
      const long long planes = (r1_ - r0_) / plane_;
      sp.G.n[ndim_ - 1] = planes;
      sp.G.N = planes * plane_;
      sp.dims[ndim_ - 1] = planes;
      s.ext = std::make_shared<ExtProj<T>>(sp, stream_);
    }
    if (!s.owned) return;
    // vectors read through adjoint stencils (w[g - stride]) carry a zero front halo: no bounds checks in the kernels
    auto halloc = [&](long long n) { return galloc(n + halo_, halo_, s.nblk_or1(), N, Mem::State) + halo_; };
    s.y = halloc(s.Mpad); s.l = halloc(s.Mpad);
    s.lh0 = galloc(s.Mpad, 0, s.nblk_or1(), N, Mem::State);
    if (!x0_mode_) s.s0 = galloc(s.Mpad, 0, s.nblk_or1(), N, Mem::State);
    s.y0 = halloc(s.Mpad); s.l0 = halloc(s.Mpad);       // take turns with y, l as the current iterate: same halo
    if (!s.ident) s.dy = halloc(s.Mpad);
    // the third pair of the one-sweep update (two plain iterations in a row: the snapshot has to survive in the other pair
    // and the sweep never writes in place) -- allocated HERE, so that running out of memory is an error of sipx_finalize and
    // not of an iteration whose state has already advanced
    if (sweep_plain_ && s.in_sweep) { s.y2 = halloc(s.Mpad); s.l2 = halloc(s.Mpad); }
    if (s.custom) upload_custom(s);
    if (s.slab_dft) {
      const long long nn[3] = {G_.n[0], G_.n[1], G_.n[2]};
      s.ddft = std::make_shared<DistDft<T>>(nn, r0_ / plane_, r1_ / plane_, chunk_ / plane_, comm_->world, comm_->rank, (double)s.spec.pmax, stream_);
    }
    if (s.ext_kind && !s.dist_ext && !s.slab_ext && !s.slab_dft && !(s.fan && s.fan_owner != comm_->rank)) {      // (a gathered set: its owner only)
      s.spec.lb = s.host_lb.empty() ? nullptr : s.host_lb.data();
      s.spec.ub = s.host_ub.empty() ? nullptr : s.host_ub.data();
      s.spec.basis = s.host_basis.empty() ? nullptr : s.host_basis.data();
      s.ext = std::make_shared<ExtProj<T>>(s.spec, stream_);
      if (s.ext_kind == EXT_HISTOGRAM || s.seg_radii || s.weighted) {
        s.host_lb.clear(); s.host_ub.clear();
        if (s.pend_lb || s.pend_ub) s.ext->set_data(s.pend_lb, s.pend_ub, true);
      }
      s.host_basis.clear();
      s.host_basis.shrink_to_fit();
    }
    if (s.fan) {
      // the gathered sets are collected FIRST in an update (update_y_l), their owners project on a stream of their own while
      // every rank goes on with the sets of its own slab: each such set keeps its own whole-size vector, the fan stream its scratch
      s.fanv = (s.fan_owner == comm_->rank || !slab_local_) ? mem_.alloc<T>(P.fullpad) : loose_alloc(P.Npad);
      SIPX_HIP(hipEventCreateWithFlags(&s.fan_ev, hipEventDisableTiming));
      if (s.fan_owner == comm_->rank && !fan_st_) {
        SIPX_HIP(hipStreamCreateWithFlags(&fan_st_, hipStreamNonBlocking));
        SIPX_HIP(hipEventCreateWithFlags(&fan_fork_, hipEventDisableTiming));
        fan_ptmp_ = mem_.alloc<double>((size_t)(PREP_SLOTS + 2) * NB);
        fan_mpart_ = mem_.alloc<T>(2 * NB);
        fan_c_ = mem_.alloc<T>(P.fullpad);
      }
    }
    if (s.two_pass) {
      s.ps = mem_.alloc<ProjScalars<T>>(1);
      s.psf = mem_.alloc<ProjScalars<T>>(1);
      K<T>::ps_init(stream_, s.ps, scr_i_);
      K<T>::ps_init(stream_, s.psf, scr_i_);
    }
    if ((slab_ || search_batch_) && s.two_pass) {        // searches in lock step: every set keeps its own partial slots and gather buffer
      s.ptmp = mem_.alloc<double>((size_t)(PREP_SLOTS + 2) * NB, Mem::State);
      s.mpart = mem_.alloc<T>(2 * NB, Mem::State);
      s.cbuf_len = slab_local_ ? std::min<long long>(s.Mpad, std::max<long long>((long long)s.nblk_or1() * (whi_ - wlo_), hooks_.gcap + 64)) : s.Mpad;
      s.cbuf = mem_.alloc<T>(s.cbuf_len, Mem::State);
    }
    const bool had_scratch = s.ptmp != nullptr;
    if (set_streams_ && !s.ext_kind && s.prox != PX_CARD) {     // those two share the engine-wide scratch: main stream
      // the engine stream itself is the first of the set streams: the set dealt onto it starts right behind the x-step,
      // with no cross-stream dependency (about 20 us) on the critical path; that of the others hides behind its work
      auto grow_pool = [&]() {
        hipStream_t q = stream_;
        if (!pool_.empty()) SIPX_HIP(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
        pool_.push_back(q);
      };
      if ((int)pool_.size() < n_set_streams_) grow_pool();
      if (search_streams_) {               // searching sets: streams 1, 2, 0, 1, ... ; the others: the engine stream
        while ((int)pool_.size() < n_set_streams_) grow_pool();
        s.st = s.two_pass ? pool_[(size_t)(++search_next_) % pool_.size()] : pool_[0];
      } else {
        s.st = pool_[pool_next_++ % pool_.size()];
      }
      SIPX_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
      if (s.two_pass && !had_scratch) {
        s.ptmp = mem_.alloc<double>((size_t)(PREP_SLOTS + 2) * NB, Mem::State);
        s.mpart = mem_.alloc<T>(2 * NB, Mem::State);
        s.cbuf = mem_.alloc<T>(s.Mpad, Mem::State);
      }
    }
    if (s.prox == SIPX_PROJ_BOUNDS_VEC) {
      s.lb = mem_.alloc<T>(s.Mpad); s.ub = mem_.alloc<T>(s.Mpad);
      if (!s.pend_lb) upload_rows(s, s.host_lb.data(), s.lb);
      if (!s.pend_ub) upload_rows(s, s.host_ub.data(), s.ub);
      if (s.pend_lb || s.pend_ub) {          // (sipx_set_data_dev before sipx_finalize: the first build takes them from device memory)
        IoArgs<T> A;
        if (s.pend_lb) io_add_bounds(A, s, s.pend_lb, s.lb);
        if (s.pend_ub) io_add_bounds(A, s, s.pend_ub, s.ub);
        io_rows<T>(stream_, A, false, NB);
      }
    }
    if (!dev_io_ && l0 && l0[i]) upload_rows_ranged(s, (const T*)l0[i], s.l);
    if (!dev_io_ && y0 && y0[i]) upload_rows_ranged(s, (const T*)y0[i], s.y);
  }

  // step 9: The lane: one rank, a list the sweep takes in part (C4) -- the slice-rank / nuclear-norm set, a chain of batched GEMMs and
  // small factorisations with host round trips in it (ext_proj.hip), runs on a stream of its own, queued by a host thread of
  // its own, beside the searches, the sweep and the other loose sets on the engine stream; its update only needs x.
  // SIPX_RANK_LANE=0: in turn on the engine stream (A/B switch, tests).
  // Slab-decomposed (round 5): the slice-rank set of a long list projects the z-slices of the rank's own planes -- no collective
  // anywhere in its update -- so it takes the same lane, beside the lock-step searches, the sweep and the transform set with
  // their collectives on the engine stream.  A rank's share of C4 is where this pays most: a call on 64 slices is a chain of
  // small launches with host round trips in it that leaves most of the chip idle.
  void create_lane(const FinalizePlan& P) {
    const bool one_rank = !comm_ && !mk_ && sweep_partial_;
    const bool slabbed = comm_ && slab_ && slab_loose_ && !mk_ && sweep_partial_;
    lane_set_ = -1;
    if (env_knobs().rank_lane && (one_rank || slabbed))
      for (int i = 0; i < p_n_ && lane_set_ < 0; ++i) {
        const SetState<T>& s = sets_[i];
        // (s.ext: a slab-decomposed rank without planes has no projector and nothing to overlap)
        if (s.owned && !s.in_sweep && (one_rank ? !s.dist_ext : s.slab_ext) && s.ident && !s.custom && s.ext && s.rank_like()) lane_set_ = i;
      }
    if (lane_set_ < 0) return;
    // A stream of the highest priority: the runtime keeps its hardware queues per priority, so the lane can never share a
    // queue with the engine stream (streams of one priority are dealt onto four queues in turn; in the slab-decomposed
    // context the lane had landed on the engine stream's queue and ran strictly behind it: tools/lane_overlap.py, 0.00 ms
    // together), and the chain of small launches that is the iteration's critical path does not wait behind the sweep.
    int pr_least = 0, pr_greatest = 0;
    SIPX_HIP(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
    SIPX_HIP(hipStreamCreateWithPriority(&lane_st_, hipStreamNonBlocking, pr_greatest));
    SIPX_HIP(hipEventCreateWithFlags(&lane_fork_, hipEventDisableTiming));
    SIPX_HIP(hipEventCreateWithFlags(&lane_ev_, hipEventDisableTiming));
    // (slab-decomposed: a vector of the exchange layout addressed by global index, like loose_v_)
    if (slab_) lane_v_ = (slab_local_ && !loose_whole_) ? loose_alloc(P.Npad) : mem_.alloc<T>((size_t)std::max<long long>(P.fullpad, sets_[lane_set_].Mpad), Mem::State);
    else lane_v_ = mem_.alloc<T>((size_t)sets_[lane_set_].Mpad, Mem::State);
  }

  // ------------------------------------------------------------------------------------------
  // sipx_reset (round 5): the SAME sets on the SAME grid with a new model m (and, optionally, a new warm start and rho_ini) --
  // what the reference's callers do when they wrap PARSDMM as a projector inside an outer loop
  // (examples/constrained_freq_FWI_simple.jl:468, examples/Constraint_examples_2D.jl:222-223).  Nothing is allocated, no plan,
  // handle, stream or event is created: every array of the context is zero-filled, m is uploaded, rho / gamma return to their
  // initial values, Q is assembled again (the solve updated it incrementally: Q_update!.jl:45-48), every warm start of the
  // searches and of the library-backed projectors is forgotten, the initial feasibility is taken again.  The context then is in
  // the state sipx_finalize leaves, and a solve on it gives the bits a new context gives (tests/test_gpu_round5.py).
  void reset(const void* m, const double* rho_ini, int n_rho, double gamma_ini, int zero_ini_guess, const void* x0,
             const void* const* l0, const void* const* y0, double* feasibility_initial) override {
    need_final();
    if (comm_) throw std::runtime_error("sipx_reset is not available for a rank of a sharded solve (build a new context)");
    SIPX_HIP(hipSetDevice(device_));
    if (lane_thr_.joinable()) lane_thr_.join();
    lane_err_ = nullptr;
    SIPX_HIP(hipStreamSynchronize(stream_));
    for (hipStream_t q : pool_) if (q && q != stream_) SIPX_HIP(hipStreamSynchronize(q));
    if (lane_st_) SIPX_HIP(hipStreamSynchronize(lane_st_));
    if (cstream_) SIPX_HIP(hipStreamSynchronize(cstream_));
    const long long N = G_.N;
    // ---- arrays
    mem_.zero_state(stream_);      // everything allocated as Mem::State: the vectors, partials and scratch of the engine and of its sets
    if (!dev_io_) {
      SIPX_HIP(hipMemcpyAsync(m_, m, N * sizeof(T), hipMemcpyHostToDevice, stream_));
      io_h2d_ += N * (long long)sizeof(T);
    }
    x_cur_ = 0; x_snap_ = -1;
    x_ = xr_[0]; xold_ = x_;
    init_rho_gamma(rho_ini, n_rho, gamma_ini);
    // ---- sets
    const bool warm = !zero_ini_guess;
    for (int i = 0; i < p_n_; ++i) {
      SetState<T>& s = sets_[i];
      s.snap = -1;
      s.searches_done = 0;
      std::fill(s.sums, s.sums + SLOTS, 0.0);
      s.bb_valid = false;
      s.last_rho = T(-1); s.last_gamma = T(-1);
      if (s.ps) K<T>::ps_init(stream_, s.ps, scr_i_);
      if (s.psf) K<T>::ps_init(stream_, s.psf, scr_i_);
      if (s.ext) { s.ext->set_stream(stream_); s.ext->reset(); }
      if (warm && !dev_io_ && l0 && l0[i]) upload_rows_ranged(s, (const T*)l0[i], s.l);
      if (warm && !dev_io_ && y0 && y0[i]) upload_rows_ranged(s, (const T*)y0[i], s.y);
    }
    if (dev_io_) {
      import_dev(m, warm ? x0 : nullptr, warm ? l0 : nullptr, warm ? y0 : nullptr);
    } else if (warm && x0) {
      SIPX_HIP(hipMemcpyAsync(x_, x0, Nx_ * sizeof(T), hipMemcpyHostToDevice, stream_));
      io_h2d_ += Nx_ * (long long)sizeof(T);
    }
    // ---- pinned words and the scalars that live beside them
    for (const PinnedBlock& b : pinned_blocks()) std::memset(*b.p, b.fill, b.bytes);
    sums_seq_ = 0; cg_seq_ = 0; spec_seq_ = 0;
    spec_searches_ = spec_fallbacks_ = spec_rounds_ = 0;
    batch_searches_ = batch_fallbacks_ = 0;
    for (long long& c : routes_) c = 0;
    head_done_ = false; rs_pending_ = false; sums_pending_ = false; merged_nslots_ = 0;
    rhs_fused_ = false; have_log_sums_ = false;
    obj_ss_ = evo_ss_ = xx_ss_ = 0;
    sums_flags_ = 0;
    marks_.reset();
    run_ = Run();
    assemble_Q();
    build_q_table();
    initial_feasibility(feasibility_initial);
  }

  void initial_feasibility(double* feasibility_initial) {
    // initial feasibility ||P_i(A_i m) - A_i m|| / (||A_i m|| + 100 eps)   (PARSDMM_initialize.jl:97-99)
    feas_init_.assign(pp_n_, 0.0);
    for (int i = 0; i < pp_n_; ++i) {
      SetState<T>& s = sets_[i];
      if (s.dist_ext || s.slab_ext || s.slab_dft) {           // every rank: its slab of slices / its planes of the transform
        dist_feasibility(s, m_, fe2_part(i), i);
        continue;
      }
      if (s.fan) {                              // the set's owner, on the gathered array
        SetArgs<T> a = set_args(s, rho_[i], gamma_[i], 0);
        a.x = m_;
        fan_feasibility(s, a, fe2_part(i));
        continue;
      }
      if (!s.owned) continue;
      if (slab_local_ && !s.two_pass && !s.ext_kind && !s.custom) {      // an element-wise set on the identity: every rank its planes
        SetArgs<T> a = set_args(s, rho_[i], gamma_[i], 0);
        a.x = m_;
        K<T>::proj_dist_set(stream_, Gr_, a, 1, (const ProjScalars<T>*)nullptr, fe2_part(i));
        continue;
      }
      if (slab_ && !s.two_pass && comm_->rank != 0) continue;      // an element-wise set: rank 0 takes the whole grid (one-off)
      double* dst = fe2_part(i);
      // Minkowski: TD_OP[i] * [m; 0] = A m for components 1 and 3, A 0 = 0 for component 2 (w_ is still all zero here)
      const T* mm = s.comp == 2 ? w_ : m_;
      if (s.ext_kind) {
        SetArgs<T> a = set_args(s, rho_[i], gamma_[i], 0);
        a.x = mm;
        if (s.custom) {                                        // (EXT_L21_STACKED: s = A m materialised, the projector acts on its M entries)
          custom_fwd(stream_, s, mm, s.sbuf);
          a.x = s.sbuf;
        }
        ext_feasibility(s, a, dst);
      } else if (s.custom) {                                   // s = A m materialised, then as for an identity set
        custom_fwd(stream_, s, mm, s.sbuf);
        if (s.two_pass) {
          SetArgs<T> a = set_args(s, rho_[i], gamma_[i], 0);
          a.x = s.sbuf;
          K<T>::proj_scalars_set(stream_, s.gm, a, 1, s.psf, part_tmp_, maxpart_, scr_c_, s.Mtrue);
          K<T>::proj_dist_set(stream_, s.gm, a, 1, s.psf, dst);
        } else {
          proj_dist_grid<T>(stream_, s.gm, 0, s.dir, s.Mpad, s.sbuf, s.prox, s.plo, s.phi, s.lb, s.ub, nullptr, dst);
        }
      } else if (s.two_pass) {
        SetArgs<T> a = set_args(s, rho_[i], gamma_[i], 0);
        a.x = mm;                                              // s = A m produced on the fly
        SampleCtl cf;
        cf.host_ovf = (int*)hovf_ + i;
        cf.compact_cap = scr_c_len_;
        K<T>::proj_scalars_set(stream_, Gr_, a, 1, s.psf, part_tmp_, maxpart_, scr_c_, s.Mtrue, cf, hooks());
        K<T>::proj_dist_set(stream_, Gr_, a, 1, s.psf, dst);
      } else {
        K<T>::fwd(stream_, G_, s.nblk, s.dir, s.ih, mm, scr_v_);
        proj_dist_grid<T>(stream_, G_, s.nblk, s.dir, s.Mpad, scr_v_, s.prox, s.plo, s.phi, s.lb, s.ub, nullptr, dst);
      }
    }
    reduce_set_sums(p_n_ * SLOTS, YlPlan::Route::ByEvent);
    SIPX_HIP(hipStreamSynchronize(stream_));
    for (int i = 0; i < p_n_ && slab_; ++i)
      if (hovf_[i]) {
        hovf_[i] = 0;
        throw std::runtime_error("initial feasibility of set " + std::to_string(i) + ": the magnitudes inside the final bracket of the " + std::string(sets_[i].prox == PX_CARD ? "cardinality" : "l1") +
                                 " search, gathered over all ranks, exceed the exchange segment of " +
                                 std::to_string(hooks_.gcap) + " values per rank (slab decomposition) -- use the set decomposition for this problem");
      }
    for (int i = 0; i < pp_n_; ++i) {
      if (!sets_[i].owned && !comm_) continue;     // sharded: the all-reduced sums of every set are here
      feas_init_[i] = (double)feas_value(hres_[i * SLOTS + SL_FE2], hres_[i * SLOTS + SL_SS2]);
    }
    if (feasibility_initial)
      for (int i = 0; i < pp_n_; ++i) feasibility_initial[i] = feas_init_[i];
  }

  // ------------------------------------------------------------------------------------------
  void rhs_compose(const double* rho) override {
    need_final();
    ObserverGuard og(observer());
    head_done_ = false;           // a residual product queued ahead belonged to the right-hand side that is replaced here
    if (rs_pending_) {          // a right-hand side that was never consumed: let its exchange finish before rhs is rewritten
      SIPX_HIP(hipStreamWaitEvent(stream_, ev_c_[1], 0));
      rs_pending_ = false;
    }
    if (mk_) {    // rhs = sum_i [A 0]'w_i / [0 A]'w_i / [A A]'w_i, w_i = rho_i y_i + l_i, sets added in order per half
      for (int half = 0; half < 2; ++half) {
        T* out = rhs_ + (long long)half * G_.N;
        RhsBatch b(stream_, G_, out, false);
        for (int pass = 0; pass < 2; ++pass) {            // own component first (it precedes the sum sets in TD_OP order)
          for (int i = 0; i < p_n_; ++i)
            if (sets_[i].comp == (pass == 0 ? half + 1 : 3)) b.add(sets_[i], (T)rho[i]);
          b.finish();
        }
        if (b.launched == 0) SIPX_HIP(hipMemsetAsync(out, 0, G_.N * sizeof(T), stream_));
      }
      return;
    }
    RhsBatch b(stream_, Gr_, rhs_, false);
    for (int i = 0; i < p_n_; ++i)
      if (sets_[i].owned && !sets_[i].custom) b.add(sets_[i], (T)rho[i]);
    if (b.launched == 0) b.flush();            // (no set at all: the launch still writes rhs = 0)
    else b.finish();
    for (int i = 0; i < p_n_; ++i) {       // caller-supplied sparse operators: rhs += A_i'(rho_i y_i + l_i), one launch each
      const SetState<T>& s = sets_[i];
      if (s.owned && s.custom) custom_adj_rhs(stream_, s, (T)rho[i]);
    }
    if (comm_ && !slab_) {
      // the (+) reduction of the partial right-hand sides (rhs_compose.jl:17-20), delivered by z-slab: every rank receives
      // the rows its part of the x-step needs.  It runs on the communication stream; whatever the engine stream is given
      // next (the Q update, the log-only kernels of the previous y/l update) overlaps with it, argmin_x joins.
      SIPX_HIP(hipEventRecord(ev_c_[0], stream_));
      SIPX_HIP(hipStreamWaitEvent(cstream_, ev_c_[0], 0));
      comm_->reduce_scatter_sum(rhs_, (size_t)chunk_, dtype_code(), cstream_);
      SIPX_HIP(hipEventRecord(ev_c_[1], cstream_));
      rs_pending_ = true;
    }
  }

  // First part of the x-step: the residual product r_0 = rhs - Q x (which also keeps x_old and serves the tolerance chain), and,
  // sharded, the grouped call that makes its sums global and hands the boundary planes of p_1 = r_0 to the neighbours.  The
  // whole-solve loop queues it AHEAD -- right behind the y/l update of the previous iteration, before the host waits for that
  // iteration's sums -- whenever the right-hand side is known by then (rho cannot change): the device runs the product while the
  // host reads the sums and evaluates the stop rule (a stop leaves x, y, l untouched: p, x_old and the partials are scratch),
  // and, sharded, the all-reduce of the per-set sums rides in the same call (dres_ sits behind part_cg_).
  void argmin_x_head() {
    if (rs_pending_) {                       // the reduce-scatter of rhs (communication stream) has to have landed
      SIPX_HIP(hipStreamWaitEvent(stream_, ev_c_[1], 0));
      rs_pending_ = false;
    }
    const long long r0 = r0_, r1 = r1_;
    const int dt = dtype_code();
    // the initial residual goes straight into the p buffer (p_1 = r_0, cg.jl:57): the first iteration reads it from there
    // as both r and p and writes r_1 into the r buffer, so the copy p <- r is never made
    // (x_old is not written: the x-step leaves x_k behind in its own buffer, see the ring of x buffers)
    if (stencil_q_) K<T>::sq_resid(stream_, G_, sq_, x_, rhs_, p_, (T*)nullptr, (T*)nullptr, part_cg_);
    else K<T>::resid(stream_, Nx_, r0, r1, Q_, cds_, x_, rhs_, p_, (T*)nullptr, (T*)nullptr, part_cg_);
    // matrix-free terms: r_0 -= rho_i A_i'(A_i x); the last launch replaces the partials of ||r_0||^2 (||rhs||^2 stays as it is)
    mf_terms(x_, p_, /*sign*/ T(-1), /*dot*/ 2, nullptr, nullptr);
    if (comm_) {         // ||r_0||^2, ||rhs||^2 block partials [+ the per-set sums of the y/l update queued just before]; p_1 = r_0 is in p_
      comm_->allreduce_with_halo(part_cg_, (size_t)(2 * NB + merged_nslots_), SIPX_F64, p_ + r0, p_ + r0 - plane_, prev_, p_ + r1 - plane_,
                                 p_ + r1, next_, (size_t)plane_, dt, stream_);
      if (merged_nslots_ > 0) K<T>::copy_f64(stream_, dres_, hres_, merged_nslots_);
      merged_nslots_ = 0;
    }
    head_done_ = true;
  }

  void argmin_x(int it, double* tol_ref_io, int64_t* cg_it, double* cg_relres, int* cg_flag) override {
    need_final();
    ObserverGuard og(observer());
    if (!head_done_) argmin_x_head();
    head_done_ = false;
    const long long r0 = r0_, r1 = r1_, nloc = r1 - r0;      // rows of this rank's part of the x-step (all of them unless sharded)
    const int dt = dtype_code();
    // Sharded (either decomposition): the rows of the x-step are split by z-slab and a product needs the boundary planes of p
    // from the two neighbours.  They are never sent: a rank keeps copies of the neighbours' boundary planes of p AND x and
    // takes them through the same updates (x += alpha p, p = r + beta p: same scalars, same operands, same bits), which only
    // needs the boundary planes of r -- and those do not depend on the all-reduce of ||r||^2 that follows the same kernel, so
    // the two travel in ONE grouped call.  Per CG iteration: all-reduce (p.Ap), then {all-reduce (||r||^2) + planes of r};
    // before the first: {all-reduce (||r_0||^2, ||rhs||^2) + planes of r_0 = p_1} (argmin_x_head); no exchange of x after the solve.
    const long long hlo = (comm_ && prev_ >= 0) ? plane_ : 0, hhi = (comm_ && next_ >= 0) ? plane_ : 0;
    const unsigned seq = ++cg_seq_;
    K<T>::cg_begin(stream_, part_cg_, cg_dev_, cg_host_, it, (T)*tol_ref_io, seq, (unsigned long long*)ticket_);
    // One CG iteration = product + p.Ap -> x, r update + ||r||^2 -> p update.
    // The host enqueues iteration k+1 as soon as the ticket word says that k did not converge, which workgroup 0 of the
    // p-update publishes before it starts streaming: the GPU does not idle on the round trip and nothing is launched
    // for an iteration that does not run.
    // where this x-step writes x: a ring buffer that holds neither the current x nor the snapshot of the x0 mode
    int tgt = 0;
    while (tgt == x_cur_ || tgt == x_snap_) ++tgt;
    T* const xn = xr_[tgt];
    auto enqueue = [&](int k) {
      CgState<T>* mirror = cg_host_ + (k & 1);
      if (stencil_q_) K<T>::sq_spmv_dot(stream_, G_, sq_, p_, Ap_, part_cg_, cg_dev_);
      else K<T>::spmv_dot(stream_, Nx_, r0, r1, Q_, cds_, p_, Ap_, part_cg_, cg_dev_);
      // matrix-free terms: Ap += rho_i A_i'(A_i p); the last launch writes the partials of the complete p . Ap where the banded
      // product put those of its part, so the x / r update reads what it always reads
      mf_terms(p_, Ap_, T(1), /*dot*/ 1, p_, &cg_dev_->done);
      if (comm_) comm_->allreduce_sum(part_cg_, NB, SIPX_F64, stream_);
      K<T>::cg_update_xr(stream_, nloc, (k == 1 ? x_ : xn) + r0, xn + r0, (k == 1 ? p_ : r_) + r0, r_ + r0, p_ + r0, Ap_ + r0, part_cg_, cg_dev_, mirror, k,
                         (unsigned long long*)ticket_, hlo, hhi);
      if (comm_)
        comm_->allreduce_with_halo(part_cg_ + NB, NB, SIPX_F64, r_ + r0, r_ + r0 - plane_, prev_, r_ + r1 - plane_, r_ + r1, next_,
                                   (size_t)plane_, dt, stream_);
      K<T>::cg_update_p(stream_, nloc, p_ + r0, r_ + r0, part_cg_, cg_dev_, mirror, (unsigned long long*)ticket_, hlo, hhi);
    };
    // Fused form (cg_fused_): iteration 1 = product on p_1 (= r_0, in p_), x / r update, then the fused kernel of iteration 2
    // queued at once; iteration k >= 2 = x / r update on the p_k and A p_k the fused kernel left, then the fused kernel of
    // iteration k + 1.  p_k lives in p_ for odd k, in p2_ for even k.
    auto enqueue_fused = [&](int k) {
      CgState<T>* mirror = cg_host_ + (k & 1);
      T* pk = (k & 1) ? p_ : p2_;
      T* pn = (k & 1) ? p2_ : p_;
      if (k == 1) K<T>::spmv_dot(stream_, Nx_, r0, r1, Q_, cds_, p_, Ap_, part_cg_, cg_dev_);
      K<T>::cg_update_xr(stream_, nloc, k == 1 ? x_ : xn, xn, k == 1 ? p_ : r_, r_, pk, Ap_, part_cg_, cg_dev_, mirror, k, (unsigned long long*)ticket_);
      K<T>::spmv_fused(stream_, Nx_, Q_, cds_, r_, pk, pn, Ap_, part_cg_, cg_dev_, mirror, (unsigned long long*)ticket_);
    };
    // (no event is recorded inside this loop: a record costs the stream about 5 us, more than the p-update of a small grid)
    // The first iteration is queued before the verdict of k_cg_begin is back: it is almost always needed, and its kernels
    // return at once on the device-side `done` flag when it is not (zero right-hand side, cg.jl:51; x already solves the
    // system to the tolerance, cg.jl:73-76) -- such a launch is not counted as a sample of the dominant kernel.
    // The first outer iteration of a solve is the one place where that is common (zero start: rhs = 0): there the verdict is
    // awaited first, so that rocprofv3's per-kernel averages hold launches with work only.
    const size_t stat0 = samples_.size();
    const bool ahead = it > 1;
    auto enq = [&](int k) { if (cg_fused_) enqueue_fused(k); else enqueue(k); };
    if (ahead) enq(1);
    bool done = wait_ticket(seq, 0, cg_host_);
    const bool done_at_begin = done;
    CgState<T> fin;
    if (done) {
      fin = cg_host_[0];
      drop_samples_from(stat0);          // the iteration queued ahead returned at once: not a sample of its kernels
      if (fin.flag == -9) SIPX_HIP(hipMemsetAsync(xn + r0 - hlo, 0, (nloc + hlo + hhi) * sizeof(T), stream_));   // cg.jl:51 (the copies of the neighbours' planes too)
    } else {
      const int maxIter = 1000;                       // argmin_x.jl:39
      int iter = 1;
      if (!ahead) enq(1);
      // (Queueing iteration k+1 before the verdict of k -- under a kernel name of its own -- was measured on the small
      // grid where the p-update is shorter than the round trip, 2048^2: 1940 against 2040 it/s.  Not adopted.)
      for (;;) {
        done = wait_ticket(seq, iter, cg_host_ + (iter & 1));
        if (done || iter == maxIter) break;
        enq(++iter);
      }
      fin = cg_host_[iter & 1];         // written before the ticket (release / acquire): complete
    }
    cg_host_[0] = fin;
    // Did the solve write x?  Zero right-hand side (flag -9): x = 0, into the target buffer.  x already good enough (cg.jl:73-76),
    // or the very first step refused (flag -2 at iteration 1, cg.jl:91-93): x is what it was, and x_old names the same buffer.
    const bool wrote = fin.flag == -9 || (!done_at_begin && !(fin.flag == -2 && fin.iters <= 1));
    if (wrote) {
      xold_ = x_;
      x_cur_ = tgt;
      x_ = xn;
    } else {
      xold_ = x_;
    }
    if (comm_) {
      // obj / evol_x sums over the slab (x_old is only kept for the slab), then x is completed on every rank
      // (slab-decomposed with a distance term: the y/l update of that set forms the same three sums over the same rows -- x, m
      //  and x_old of the slab -- and they travel in the same all-reduce; no pass of its own)
      if (!slab_dist_logs_) K<T>::log3(stream_, nloc, x_ + r0, m_ + r0, xold_ + r0, part_sets_ + (size_t)p_n_ * SLOTS * NB);
      // slab-decomposed: the planes of x next to the slab (forward differences read one plane up, the recomputed plane below
      // needs one down) were kept current by the CG updates themselves -- nothing to exchange
      if (!slab_) comm_->allgather(x_, (size_t)chunk_, dt, stream_);
    }
    *tol_ref_io = (double)cg_host_->tol_ref;
    *cg_it = cg_host_->iters;
    *cg_relres = (double)cg_host_->res_last;
    if (cg_flag) *cg_flag = cg_host_->flag;
  }

  // The four mutually exclusive regimes of a y/l update.  Which one a call is follows from the context and from whether the
  // sweep takes this call's flags; update_y_l decides it once and runs that regime's steps in order.
  enum class YlRegime {
    SweepAll,       // one rank, the sweep takes every set
    SweepPartial,   // one rank, the sweep takes a subset: loose sets with their per-set kernels, one of them maybe on the lane
    Slab,           // slab-decomposed: lock-step searches with their collectives, then the sweep or the per-set kernels
    PerSet          // per-set kernels on the set streams: Minkowski, set-sharded, custom operators, SIPX_YL_MULTI=0
  };
  struct LaneGuard {                       // whatever ends update_y_l, the lane's host thread is joined first
    Engine<T>* e;
    ~LaneGuard() {
      if (!e->lane_thr_.joinable()) return;              // (lane_join has run: nothing is left over)
      // an exception on the caller's thread between lane_start and lane_join: the lane's work is waited for, its projector
      // goes back to the engine stream, its own error (if any) is dropped in favour of the one that is propagating.  The
      // iterate of the lane set may be half updated: the solve is over, sipx_reset gives the context a defined state again.
      e->lane_thr_.join();
      if (e->lane_st_) (void)hipStreamSynchronize(e->lane_st_);
      try { e->sets_[e->lane_set_].ext->set_stream(e->stream_); } catch (...) {}
      e->lane_err_ = nullptr;
      e->lane_sample_ = -1;
    }
  };

  // the phase entry point: the default plan -- the sums by an event of their own, collected here, nothing fused
  void update_y_l(int it, int flags, const double* rho, const double* gamma, double* r_pri, double* r_dual,
                  double* feas) override {
    yl_update(it, flags, rho, gamma, YlPlan(), r_pri, r_dual, feas);
  }
  // everything of a y/l update queued, the reduction of its sums included; then, unless the plan leaves that to the caller,
  // the sums collected into r_pri, r_dual, feas (collect_set_sums)
  void yl_update(int it, int flags, const double* rho, const double* gamma, const YlPlan& plan, double* r_pri = nullptr,
                 double* r_dual = nullptr, double* feas = nullptr) {
    need_final();
    ObserverGuard og(observer());
    rhs_fused_ = false;
    MultiArgs<T> ma;
    const bool sweep = sweep_applicable(flags, ma);
    if (x0_mode_ && !sweep) throw std::runtime_error("internal: an x0-mode context met an update the one-sweep kernel does not take");
    // PARTIAL sweep (round 4): set lists with terms the sweep cannot take -- a projector behind a transform or a factorisation,
    // cardinality (BASELINE config 4: l1 behind the DFT, slice rank, cardinality on D_z) -- have their element-wise and l1 / l2 terms
    // updated by the sweep all the same (x read once for them, r_dual in the same pass); the other sets ("loose") keep their
    // per-set kernels, on the engine stream.  The fused right-hand side then holds the sets in front of the first loose
    // one (MultiBlk::in_rhs; the sets are added in order, rhs_compose.jl:24-31) and k_rhs adds the rest.
    const YlRegime regime = slab_ ? YlRegime::Slab : !sweep ? YlRegime::PerSet : has_loose_ ? YlRegime::SweepPartial : YlRegime::SweepAll;
    // (the all-kernel statistics window keeps everything on the engine stream: its event pairs time one kernel at a time)
    const bool lane_now = sweep && lane_set_ >= 0 && stats_mode_ != 2;
    LaneGuard lane_guard{this};
    if (lane_now) lane_start(flags, rho, gamma);
    switch (regime) {
      case YlRegime::SweepAll:
        one_rank_searches(flags, rho, gamma);
        sweep_launch(flags, rho, gamma, ma, plan.fuse_rhs);
        break;
      case YlRegime::SweepPartial:
        one_rank_searches(flags, rho, gamma);
        sweep_launch(flags, rho, gamma, ma, plan.fuse_rhs);
        update_sets_in_turn(flags, rho, gamma, /*skip_swept*/ true, lane_now, /*own_streams*/ false);
        if (lane_now) lane_join(flags);
        rest_of_fused_rhs(rho);
        break;
      case YlRegime::Slab:
        slab_lockstep_searches(it, flags, rho, gamma);
        if (sweep) {
          // the searches ran in lock step above; every set's update in one sweep over the rank's planes (plus the last plane of
          // the rank below, recomputed), then the feasibility searches of the two-pass sets with their collectives, on the
          // engine stream, in one order on every rank
          for (int i = 0; i < p_n_; ++i)
            if (sets_[i].two_pass) { sets_[i].last_rho = (T)rho[i]; sets_[i].last_gamma = (T)gamma[i]; }
          sweep_launch(flags, rho, gamma, ma, plan.fuse_rhs);
          if (flags & SIPX_YL_FEAS) slab_feasibility_searches(it, flags, rho, gamma);
        } else if (set_streams_) {
          SIPX_HIP(hipEventRecord(ev_fork_, stream_));      // the searches are done: the updates may start
        }
        for (int i = 0; i < p_n_ && slab_loose_; ++i)          // the gathered sets first: their owners project beside what follows
          if (sets_[i].fan) fan_begin(sets_[i], set_args(sets_[i], (T)rho[i], (T)gamma[i], flags));
        update_sets_in_turn(flags, rho, gamma, /*skip_swept*/ sweep, lane_now, /*own_streams*/ true);
        if (lane_now) lane_join(flags);
        if (sweep) rest_of_fused_rhs(rho);
        else join_set_streams([this](int i) { return sets_[i].owned; });      // the reductions see every set
        break;
      case YlRegime::PerSet:
        if (mk_) K<T>::sum_uv(stream_, G_.N, x_, x_ + G_.N, w_);
        if (set_streams_) SIPX_HIP(hipEventRecord(ev_fork_, stream_));     // x (and u + v) are final: the sets may start
        update_sets_in_turn(flags, rho, gamma, /*skip_swept*/ false, /*lane_now*/ false, /*own_streams*/ true);
        update_sets_of_all_ranks(flags, rho, gamma);
        join_set_streams([this](int i) { return sets_[i].owned; });      // the reductions see every set
        break;
    }
    // Minkowski: evol_x runs over all 2N unknowns (PARSDMM.jl:145); the distance-term kernel only saw u + v
    if (mk_) K<T>::log3(stream_, Nx_, x_, (const T*)nullptr, xold_, part_sets_ + (size_t)p_n_ * SLOTS * NB);
    reduce_set_sums((p_n_ + ((mk_ || comm_) ? 1 : 0)) * SLOTS, plan.route);
    sums_flags_ = flags;
    sums_pending_ = true;
    if (plan.collect_now) {
      SIPX_HIP(hipEventRecord(ev_sums_, stream_));
      sums_event_ = ev_sums_;
      collect_set_sums(plan.route, rho, r_pri, r_dual, feas);
    }
  }

  // one rank, the sweep does the updates: the searches of its two-pass sets, batched or on the set streams
  void one_rank_searches(int flags, const double* rho, const double* gamma) {
    if (search_batch_) batched_searches(flags, rho, gamma);
    else sweep_searches(flags, rho, gamma);
  }

  // ---- small rules of the y/l update, each written once --------------------------------------------------------------------
  double* set_part(int i) const { return part_sets_ + (size_t)i * SLOTS * NB; }                 // the reduction slots of set i
  double* fe2_part(int i) const { return part_sets_ + ((size_t)i * SLOTS + SL_FE2) * NB; }      // ... its feasibility slots

  // a set's search scratch: its own (searches in lock step, set streams) or the engine-wide one; cap: elements the gather buffer holds
  struct SetScratch {
    double* ptmp;
    T *mpart, *cbuf;
    long long cap;
  };
  SetScratch scratch_of(const SetState<T>& s) const {
    return {s.ptmp ? s.ptmp : part_tmp_, s.mpart ? s.mpart : maxpart_, s.cbuf ? s.cbuf : scr_c_, s.cbuf ? s.cbuf_len : scr_c_len_};
  }

  // SampleCtl of set i's prox search: the set's pinned words, and the sampled prediction of theta in front of the search
  // (kernels_proj.hip, k_sample) when the previous search of this set asked for it (theta moved, fallback sweeps were needed) or
  // rho was changed: its verdict sits in pinned memory, written by k_l1_solve before the sums of that iteration reached the
  // host.  (A stale word costs time only: the kernels check the device-side state themselves.)  `here`: what the calling
  // regime adds to that rule.
  SampleCtl search_ctl(int i, bool rescaled, bool here) const {
    SampleCtl c;
    c.host_want = (int*)hlean_ + i;
    c.host_ovf = (int*)hovf_ + i;
    c.runs = env_knobs().l1_sample_runs;
    c.enable = env_knobs().l1_sample && here && sets_[i].prox == PX_L1 && (rescaled || (hlean_[i] & 0xff) != 0);
    return c;
  }

  // Where a per-set update writes y_new, l_new (a.yo, a.lo) and how (y, l) / (y0, l0) / snap rotate once it is queued (see
  // SetState): snapshot iterations overwrite the old snapshot, the others stay off it.  First iteration: in place, (y, l) becomes
  // the snapshot; no snapshot yet: the zero-filled other pair stands in for it.  (The sweep never writes in place and has a
  // third pair: its own rule is in sweep_launch.)
  struct YlTarget {
    bool to_other, snapshot;
  };
  static YlTarget aim(const SetState<T>& s, int flags, SetArgs<T>& a) {
    const bool snapshot = (flags & (SIPX_YL_BB | SIPX_YL_FIRST)) != 0, first = (flags & SIPX_YL_FIRST) != 0;
    const bool to_other = snapshot ? (!first && s.snap != 0) : (s.snap == 0);
    a.yo = to_other ? s.y0 : s.y;
    a.lo = to_other ? s.l0 : s.l;
    return {to_other, snapshot};
  }
  static void rotate(SetState<T>& s, YlTarget t) {
    if (t.to_other) { std::swap(s.y, s.y0); std::swap(s.l, s.l0); }     // (y, l) always names the current iterate
    if (t.snapshot) s.snap = 0;
    else if (t.to_other && s.snap == 0) s.snap = 1;
  }

  // the engine stream waits for every set stream, behind the last of the sets `on` names that was dealt onto it (one event per stream)
  template <typename Pred>
  void join_set_streams(Pred on) {
    for (size_t k = 0; k < pool_.size(); ++k) {
      if (pool_[k] == stream_) continue;
      SetState<T>* last = nullptr;
      for (int i = 0; i < p_n_; ++i)
        if (sets_[i].st == pool_[k] && on(i)) last = &sets_[i];
      if (!last) continue;
      SIPX_HIP(hipEventRecord(last->ev, last->st));
      SIPX_HIP(hipStreamWaitEvent(stream_, last->ev, 0));
    }
  }

  // the sets of a right-hand side, MAX_SETS to a launch: the first launch writes `out` (unless it accumulates), the others add
  struct RhsBatch {
    hipStream_t q;
    const Grid& g;
    T* out;
    int launched;
    RhsArgs<T> a;
    RhsBatch(hipStream_t q_, const Grid& g_, T* out_, bool accumulate) : q(q_), g(g_), out(out_), launched(accumulate ? 1 : 0) { a.nsets = 0; }
    void add(const SetState<T>& s, T rho) {
      RhsSet<T>& r = a.s[a.nsets++];
      r.y = s.y; r.l = s.l; r.rho = rho; r.nblk = s.nblk;
      for (int d = 0; d < 3; ++d) { r.dir[d] = s.dir[d]; r.ih[d] = s.ih[d]; }
      if (a.nsets == MAX_SETS) flush();
    }
    void flush() {
      K<T>::rhs_compose(q, g, a, out, launched++ > 0);
      a.nsets = 0;
    }
    void finish() { if (a.nsets > 0) flush(); }
  };

  // ---- steps of the y/l update ------------------------------------------------------------------------------------------------
  // The two-pass sets among the first n that search in lock step on a slab-decomposed grid (a gathered set and cardinality have
  // searches of their own), their arguments and their segments in rank 0's chunk of the full-size exchange buffer: one per l1
  // set, `chunk` to the next rank's.  (The distance term is never a two-pass set: n = p_n_ and n = pp_n_ name the same sets.)
  struct LockStep {
    std::vector<int> tp;
    std::vector<SetArgs<T>> args;
    std::vector<SampleCtl> ctl;
    std::vector<T*> gseg;              // (empty: no exchange -- the batched searches of one rank)
    long long chunk = 0;
    int nl1 = 0;
    size_t RS = 0;                     // doubles of a set's region of stage_
    int v_is_s = 0;
    bool feas_ps = false;              // the searches of the feasibility estimates: each set's second scalar state
    const ChainHooks* hk = nullptr;
  };
  LockStep lockstep_sets(int n, int flags, const double* rho, const double* gamma) {
    LockStep L;
    for (int i = 0; i < n; ++i)
      if (sets_[i].two_pass && !sets_[i].fan && !sets_[i].slab_card) L.tp.push_back(i);
    if (L.tp.empty()) return L;
    const long long seg = hooks_.gcap + GATHER_HDR;
    L.args.resize(L.tp.size());
    L.ctl.resize(L.tp.size());
    L.gseg.assign(L.tp.size(), nullptr);
    for (size_t j = 0; j < L.tp.size(); ++j) {
      const SetState<T>& s = sets_[L.tp[j]];
      L.args[j] = set_args(s, (T)rho[L.tp[j]], (T)gamma[L.tp[j]], flags);
      if (s.prox == PX_L1) L.gseg[j] = gbuf_ + (long long)(L.nl1++) * seg;
    }
    L.chunk = (long long)std::max(L.nl1, 1) * seg;
    L.RS = (size_t)(PREP_SLOTS + 1 + 2 * comm_->world);
    L.hk = &hooks_;
    return L;
  }
  // one stage of the search of set j of a lock-step group; reg: the set's region of the staging buffer, seg / segchunk: its
  // segment in rank 0's chunk of an exchange buffer and the distance to the next rank's
  void search_stage(int stage, hipStream_t q, const LockStep& L, size_t j, double* reg, T* seg, long long segchunk) {
    SetState<T>& s = sets_[L.tp[j]];
    K<T>::proj_scalars_stage(stage, q, Gr_, L.args[j], L.v_is_s, L.feas_ps ? s.psf : s.ps, s.ptmp, s.mpart, s.cbuf, s.Mtrue, L.ctl[j], L.hk,
                             reg, seg, segchunk);
  }
  void search_stage(int stage, hipStream_t q, const LockStep& L, size_t j) {      // (staging region, full-size exchange segment)
    search_stage(stage, q, L, j, stage_ + j * L.RS, L.gseg.empty() ? nullptr : L.gseg[j], L.chunk);
  }

  // Slab-decomposed iteration: the threshold / scale searches of ALL sets in lock step -- every rank sweeps its planes,
  // ONE all-reduce makes the probe sums of all sets global (twice: first pass, gated refinement), ONE all-gather strings
  // the gathered magnitudes of all l1 sets together; every rank then solves the same small problems (same bits).
  void slab_lockstep_searches(int it, int flags, const double* rho, const double* gamma) {
    LockStep L = lockstep_sets(p_n_, flags, rho, gamma);
    if (L.tp.empty()) return;
    const std::vector<int>& tp = L.tp;
    const bool batch = env_knobs().spec_exchange && (int)tp.size() <= SPEC_MAX_SETS;
    RescaleMulti<T> rs;
    rs.n = 0;
    // sampled prediction of theta (kernels_proj.hip, k_sample) for the l1 sets whose last search asked for it: every rank
    // samples its planes, ONE all-reduce adds the histograms (float64 holding exact integers), every rank decides alike
    bool any_sample = false;
    const size_t SS = (size_t)(2 * SAMPLE_BINS + 3);
    for (size_t j = 0; j < tp.size(); ++j) {
      SetState<T>& s = sets_[tp[j]];
      const bool rescaled = s.rescaled(L.args[j].rho);
      if (rescaled) {
        if (batch && rs.n < SPEC_MAX_SETS) { rs.ps[rs.n] = s.ps; rs.factor[rs.n++] = s.rescale_factor(L.args[j].rho); }
        else K<T>::ps_rescale(stream_, s.ps, s.rescale_factor(L.args[j].rho));
      }
      L.ctl[j] = search_ctl(tp[j], rescaled, true);
      L.ctl[j].compact_cap = s.cbuf_len;
      any_sample |= L.ctl[j].enable != 0;
    }
    K<T>::ps_rescale_multi(stream_, rs);          // (one launch for all of them)
    if (any_sample && batch && Gr_.n[0] % 4 == 0) {      // every sampling set in one launch per stage
      SampleMulti<T> sm;
      sm.ns = 0;
      for (size_t j = 0; j < tp.size(); ++j) {
        if (!L.ctl[j].enable || sets_[tp[j]].prox != PX_L1) continue;
        SampleSet<T>& S = sm.s[sm.ns++];
        S.a = L.args[j]; S.a.ps = sets_[tp[j]].ps; S.ps = sets_[tp[j]].ps; S.partials = sets_[tp[j]].ptmp;
        S.reg = sstage_ + j * SS; S.true_len = sets_[tp[j]].Mtrue;
      }
      K<T>::sample_multi(10, stream_, Gr_, sm, env_knobs().l1_sample_runs, &hooks_);
      comm_->allreduce_sum(sstage_, tp.size() * SS, SIPX_F64, stream_);
      K<T>::sample_multi(11, stream_, Gr_, sm, env_knobs().l1_sample_runs, &hooks_);
    } else if (any_sample) {
      for (int stage = 10; stage <= 11; ++stage) {
        for (size_t j = 0; j < tp.size(); ++j)
          if (L.ctl[j].enable) search_stage(stage, stream_, L, j, sstage_ + j * SS, L.gseg[j], L.chunk);
        if (stage == 10) comm_->allreduce_sum(sstage_, tp.size() * SS, SIPX_F64, stream_);
      }
    }
    for (size_t j = 0; j < tp.size(); ++j) L.ctl[j].enable = 0;
    // Refinement rounds (a gated probe pass + one all-reduce each): the bracket has to shrink until what it holds, over
    // all ranks, fits the exchange segments -- a rank cannot keep what does not fit.  How many rounds are enqueued follows
    // the previous search of each l1 set (pinned word written by k_l1_solve; the same on every rank): two more than it
    // used, all of them while nothing is known (the first searches of a solve); a search that needs more ends in the
    // error return of collect_set_sums, never in a wrong theta.
    int rounds = 1;
    for (size_t j = 0; j < tp.size(); ++j) {
      SetState<T>& s = sets_[tp[j]];
      if (s.prox != PX_L1) continue;
      const int used = (hlean_[tp[j]] >> 8) & 0xff;
      const int want = s.searches_done < 2 ? 6 : std::min(6, std::max(2, used + 2));
      rounds = std::max(rounds, want);
      s.searches_done += 1;
    }
    rounds = std::min(6, std::max(rounds, env_knobs().l1_rounds_min));      // SIPX_L1_ROUNDS_MIN: a problem whose brackets shrink slowly
    rounds = std::max(1, std::min(rounds, env_knobs().l1_rounds_max));      // SIPX_L1_ROUNDS_MAX (tests): force an overflow
    if (env_knobs().spec_exchange) {
      spec_exchange_searches(L, it);
      return;
    }
    for (int stage = 0; stage < 4; ++stage) {
      const int reps = stage == 1 ? rounds : 1;
      for (int rep = 0; rep < reps; ++rep) {
        const int st = (stage == 1 && rep > 0) ? 4 : stage;
        for (size_t j = 0; j < tp.size(); ++j) search_stage(st, stream_, L, j);
        if (stage < 2 && (stage == 0 || L.nl1 > 0)) comm_->allreduce_sum(stage_, tp.size() * L.RS, SIPX_F64, stream_);
      }
      if (stage == 2 && L.nl1 > 0) comm_->allgather(gbuf_, (size_t)L.chunk, dtype_code(), stream_);
    }
  }

  // Slab-decomposed, behind the sweep: the feasibility estimates ||P_i(A_i x) - A_i x|| of the two-pass sets.
  void slab_feasibility_searches(int it, int flags, const double* rho, const double* gamma) {
    if (env_knobs().spec_exchange) {
      // their searches (on v = A_i x itself, each set's second scalar state) in lock step through the same exchange -- one
      // all-gather for all of them -- then the distances
      LockStep L = lockstep_sets(pp_n_, flags, rho, gamma);
      if (L.tp.empty()) return;
      for (size_t j = 0; j < L.tp.size(); ++j) {
        L.ctl[j].host_ovf = (int*)hovf_ + L.tp[j];
        L.ctl[j].compact_cap = sets_[L.tp[j]].cbuf_len;
      }
      L.v_is_s = 1;
      L.feas_ps = true;
      spec_exchange_searches(L, it);
      for (size_t j = 0; j < L.tp.size(); ++j) K<T>::proj_dist_set(stream_, Gr_, L.args[j], 1, sets_[L.tp[j]].psf, fe2_part(L.tp[j]));
      return;
    }
    for (int i = 0; i < pp_n_; ++i) {
      SetState<T>& s = sets_[i];
      if (!s.two_pass || s.fan || s.slab_card) continue;
      SetArgs<T> a = set_args(s, (T)rho[i], (T)gamma[i], flags);
      const SetScratch scr = scratch_of(s);
      SampleCtl cf;
      cf.host_ovf = (int*)hovf_ + i;
      cf.compact_cap = scr.cap;
      K<T>::proj_scalars_set(stream_, Gr_, a, 1, s.psf, scr.ptmp, scr.mpart, scr.cbuf, s.Mtrue, cf, hooks());
      K<T>::proj_dist_set(stream_, Gr_, a, 1, s.psf, fe2_part(i));
    }
  }

  // the per-set updates of this rank's sets, in set order; skip_swept: the sweep has updated its sets; lane_now: the lane set is
  // on its lane (lane_start); own_streams: every set on the stream it was dealt onto (false: all on the engine stream)
  void update_sets_in_turn(int flags, const double* rho, const double* gamma, bool skip_swept, bool lane_now, bool own_streams) {
    for (int i = 0; i < p_n_; ++i) {
      const SetState<T>& s = sets_[i];
      if (!s.owned || s.dist_ext || (skip_swept && s.in_sweep) || (lane_now && i == lane_set_)) continue;
      update_one_set(i, flags, rho, gamma, own_streams);
    }
  }

  // The per-set update of set i: prox_i of v = x_hat - l / rho -- the threshold / scale search of a two-pass set, or a projector
  // on the materialised v -- then the fused update of y and l with its sums, and the set's feasibility estimate when asked.
  void update_one_set(int i, int flags, const double* rho, const double* gamma, bool own_stream) {
    SetState<T>& s = sets_[i];
    const bool feas = (flags & SIPX_YL_FEAS) && i < pp_n_;
    SetArgs<T> a = set_args(s, (T)rho[i], (T)gamma[i], flags);
    if (mk_) a.x = s.comp == 1 ? x_ : (s.comp == 2 ? x_ + G_.N : w_);
    double* part = set_part(i);
    hipStream_t q = (s.st && own_stream) ? s.st : stream_;
    // slab-decomposed: a feasibility search carries collectives -- those stay on the engine stream, in one order on every rank
    if (slab_ && feas && s.two_pass) q = stream_;
    const SetScratch scr = scratch_of(s);
    if (q != stream_) SIPX_HIP(hipStreamWaitEvent(q, ev_fork_, 0));
    const YlTarget tgt = aim(s, flags, a);
    const Grid& gs = s.custom ? s.gm : Gr_;          // (the rank's slab when the whole iteration is slab-decomposed)
    const Grid& gy = s.custom ? s.gm : Gyl_;
    if (s.custom) {     // s = A x once, then the identity-shaped kernels on the M entries of s
      custom_fwd(q, s, a.x, s.sbuf);
      a.x = s.sbuf;
      a.flags |= F_STORE_DY;
    }
    if (s.slab_ext) {   // slab-decomposed, slices of the rank's own planes: nothing crosses the fabric
      q = stream_;
      K<T>::store_v(q, Gr_, a, 0, loose_v_);
      if (r1_ > r0_) {
        ObsScope obs(KID_EXT, stream_, 0.0);
        s.ext->project(loose_v_ + r0_, false, scr.ptmp, scr.mpart, scr.cbuf);
      }
      a.v = loose_v_;
      a.vsrc = 2;
    } else if (s.slab_dft) {   // slab-decomposed transform: every rank its planes, one all-to-all each way, the threshold over all ranks
      q = stream_;
      K<T>::store_v(q, Gr_, a, 0, loose_v_);
      {
        ObsScope obs(KID_EXT, stream_, 0.0);
        s.ddft->project(loose_v_ + r0_, false, comm_.get(), &hooks_, part_tmp_, maxpart_, scr_c_, scr_c_len_, (int*)hovf_ + i);
      }
      a.v = loose_v_;
      a.vsrc = 2;
    } else if (s.fan) { // slab-decomposed, a projector that needs the whole array: its owner has gathered v (fan_begin, in front of
      q = stream_;      // the per-set updates) and scatters P(v)
      fan_return(s);
      a.v = s.fanv;
      a.vsrc = 2;
    } else if (s.ext_kind) {   // library-backed projector: materialise v, project it in place, hand y to the fused update
      K<T>::store_v(q, s.custom ? gs : G_, a, 0, scr_v_);      // (a custom operator: the M entries of s = A x, EXT_L21_STACKED)
      {
        ObsScope obs(KID_EXT, stream_, 0.0);
        s.ext->project(scr_v_, false, scr.ptmp, scr.mpart, scr.cbuf);
      }
      a.vsrc = 2;
    }
    // (a gathered set was projected above; slab-decomposed, a two-pass set but cardinality was searched in lock step with the others)
    if (s.two_pass && !s.fan && !(slab_ && !s.slab_card)) {   // threshold / scale of prox_i from one pass that produces v on the fly (nothing stored)
      const bool rescaled = s.rescaled(a.rho);
      if (rescaled) K<T>::ps_rescale(q, s.ps, s.rescale_factor(a.rho));                      // v rescaled: theta moves like 1/rho
      K<T>::proj_scalars_set(q, gs, a, 0, s.ps, scr.ptmp, scr.mpart, scr.cbuf, s.Mtrue, search_ctl(i, rescaled, !slab_ && !s.custom), hooks());
    }
    if (s.two_pass || s.fan) {
      s.last_rho = a.rho;
      s.last_gamma = a.gamma;
    }
    K<T>::yl(q, (s.slab_ext || s.slab_dft || (s.fan && s.ident)) ? gs : gy, a, part);      // (no adjoint stencil reads the plane below: nothing to recompute)
    if (s.custom) custom_adj_norm(q, s, part + (size_t)SL_ADJ * NB);
    else if (!s.ident) K<T>::adj_norm(q, gs, a, part + (size_t)SL_ADJ * NB);
    if (feas && (s.slab_ext || s.slab_dft)) dist_feasibility(s, x_, fe2_part(i), i);
    else if (feas && s.fan) fan_feasibility(s, a, fe2_part(i));
    else if (feas && s.ext_kind) ext_feasibility(s, a, fe2_part(i));
    if (feas && s.two_pass && !s.fan) {
      // ||P_i(s) - s|| with s = A_i x produced on the fly; its own warm-started scalars (psf)
      SampleCtl cf;
      cf.host_ovf = (int*)hovf_ + i;
      cf.compact_cap = scr.cap;
      K<T>::proj_scalars_set(q, gs, a, 1, s.psf, scr.ptmp, scr.mpart, scr.cbuf, s.Mtrue, cf, hooks());
      K<T>::proj_dist_set(q, gs, a, 1, s.psf, fe2_part(i));
    }
    rotate(s, tgt);
  }

  // Sets whose projector is shared by all ranks (slice-wise rank / nuclear norm), in set order on every rank, after the
  // rank's own sets are queued: the owner materialises v = x_hat - l / rho and scatters it by slab (seven links at once:
  // 7/8 of N w bytes leave it, a broadcast would move seven times that), every rank projects the slices of its slab, a
  // gather returns P(v), the owner finishes the update with it.  (Engine stream: the
  // collectives are ordered against the rank's other work; what runs on the second set stream overlaps.)
  void update_sets_of_all_ranks(int flags, const double* rho, const double* gamma) {
    for (int i = 0; i < p_n_; ++i) {
      SetState<T>& s = sets_[i];
      if (!s.dist_ext) continue;
      const int dt = dtype_code();
      SetArgs<T> a;
      YlTarget tgt{false, false};
      if (s.owned) {
        a = set_args(s, (T)rho[i], (T)gamma[i], flags);
        tgt = aim(s, flags, a);
        K<T>::store_v(stream_, G_, a, 0, scr_v_);
      }
      comm_->scatter(scr_v_, (size_t)chunk_, dt, s.owner_rank, stream_);
      if (s.ext) {
        ObsScope obs(KID_EXT, stream_, 0.0);
        s.ext->project(scr_v_ + r0_, false, part_tmp_, maxpart_, scr_c_);
      }
      comm_->gather(scr_v_, (size_t)chunk_, dt, s.owner_rank, stream_);
      if (s.owned) {
        a.vsrc = 2;
        K<T>::yl(stream_, G_, a, set_part(i));
        rotate(s, tgt);
      }
      if ((flags & SIPX_YL_FEAS) && i < pp_n_) dist_feasibility(s, x_, fe2_part(i));
    }
  }

  // the sweep wrote the sum over the sets in front of the first loose one (YlPlan::fuse_rhs); the rest, in order
  void rest_of_fused_rhs(const double* rho) {
    if (!rhs_fused_) return;
    RhsBatch b(stream_, Gr_, rhs_, true);
    bool behind = false;
    for (int i = 0; i < p_n_; ++i) {
      behind |= !sets_[i].in_sweep;
      if (behind) b.add(sets_[i], (T)rho[i]);
    }
    b.finish();
  }

  // The lane set's y/l update (see sipx_finalize): x is final on the engine stream; store v, project it, update y and l on the
  // lane stream, queued by a host thread (the projector waits for its own stream between its steps).  The pointer rotation of
  // the set happens here, on the caller's thread; the thread only launches.
  void lane_start(int flags, const double* rho, const double* gamma) {
    SetState<T>& s = sets_[lane_set_];
    SetArgs<T> a = set_args(s, (T)rho[lane_set_], (T)gamma[lane_set_], flags);
    const YlTarget tgt = aim(s, flags, a);
    a.v = lane_v_;
    lane_args_ = a;
    SIPX_HIP(hipEventRecord(lane_fork_, stream_));
    SIPX_HIP(hipStreamWaitEvent(lane_st_, lane_fork_, 0));
    s.ext->set_stream(lane_st_);
    lane_err_ = nullptr;
    // the lane's kernels are launched by a thread without a launch observer (the sample list is not shared between threads): the
    // whole update of the set is booked from HERE as one inclusive interval on the lane stream, closed in lane_join -- in the
    // all-kernel statistics the slice-rank set of C4 used to be missing altogether
    lane_sample_ = -1;
    if (stats_mode_ >= 2) {
      const size_t i = samples_.size();
      samples_.push_back(KSample{KID_EXT, 0.0, 0.0});
      SIPX_HIP(hipEventRecord(stat_event(2 * i), lane_st_));
      lane_sample_ = (long long)i;
    }
    double* part = set_part(lane_set_);
    const SetScratch scr = scratch_of(s);
    ExtProj<T>* ext = s.ext.get();
    lane_thr_ = std::thread([this, a, part, scr, ext]() {
      try {
        SIPX_HIP(hipSetDevice(device_));
        K<T>::store_v(lane_st_, slab_ ? Gr_ : G_, a, 0, lane_v_);
        if (!slab_) ext->project(lane_v_, false, scr.ptmp, scr.mpart, scr.cbuf);
        else if (r1_ > r0_) ext->project(lane_v_ + r0_, false, scr.ptmp, scr.mpart, scr.cbuf);      // (the slices of the rank's own planes)
        SetArgs<T> a2 = a;
        a2.vsrc = 2;
        K<T>::yl(lane_st_, slab_ ? Gr_ : Gyl_, a2, part);
        SIPX_HIP(hipEventRecord(lane_ev_, lane_st_));
      } catch (...) {
        lane_err_ = std::current_exception();
      }
    });
    rotate(s, tgt);
  }
  void lane_join(int flags) {
    SetState<T>& s = sets_[lane_set_];
    if (lane_thr_.joinable()) lane_thr_.join();
    s.ext->set_stream(stream_);
    if (lane_sample_ >= 0 && (size_t)lane_sample_ < samples_.size())
      SIPX_HIP(hipEventRecord(stat_event(2 * (size_t)lane_sample_ + 1), lane_st_));
    lane_sample_ = -1;
    if (lane_err_) {
      (void)hipStreamSynchronize(lane_st_);
      std::exception_ptr e = lane_err_;
      lane_err_ = nullptr;
      std::rethrow_exception(e);
    }
    SIPX_HIP(hipStreamWaitEvent(stream_, lane_ev_, 0));
    if ((flags & SIPX_YL_FEAS) && lane_set_ < pp_n_) {
      if (slab_) dist_feasibility(s, x_, fe2_part(lane_set_), lane_set_);
      else {
        SetArgs<T> a = lane_args_;
        a.v = scr_v_;
        ext_feasibility(s, a, fe2_part(lane_set_));
      }
    }
  }


  // ---- communicator self-test (round 5) -------------------------------------------------------------------------
  // RcclComm has only ever run with a world of one here (a gpurun box has one GPU), and the slab decomposition hands RCCL halo
  // planes that live in mapped (sparse-array) memory.  Before any array of the context is allocated every rank therefore runs the
  // communicator's operations once on KNOWN data -- the grouped all-reduce + neighbour exchange, the in-place reduce-scatter and
  // all-gather (the offsets RcclComm computes), the fan scatter / gather, the all-to-all, all on plain memory; then the neighbour exchange once
  // more with its four buffers inside a mapped granule between two unmapped ones -- compares what arrived with what must have
  // arrived, and the ranks agree on the outcome through one more all-reduce on plain memory.  Wrong data from a base operation
  // is an error of sipx_finalize on every rank alike (the caller may attach another communicator: bench.py goes on with
  // torch.distributed callbacks); a failure of the mapped exchange alone switches THIS context to full-size arrays on every
  // rank.  SIPX_COMM_SELFTEST=0 skips it.  The same code runs through the callback communicator (tests: 2-4 ranks on one GPU).
  void comm_self_test(bool want_mapped, bool want_a2a = false) {
    if (!env_knobs().comm_selftest) {
      selftest_ = "skipped (SIPX_COMM_SELFTEST=0)";
      if (!agree_buf_) agree_buf_ = mem_.alloc<double>(64);
      return;
    }
    Comm& c = *comm_;
    const int W = c.world, R = c.rank, dt = dtype_code();
    const size_t chunk = 1024, hc = 256;
    const int prev = R > 0 ? R - 1 : -1, next = R + 1 < W ? R + 1 : -1;
    auto val = [](int r, size_t e) { return (double)((r + 1) * 256 + (int)(e & 255)); };
    std::vector<T> h(std::max<size_t>(W * chunk, 4 * hc));
    std::vector<double> hr(64);
    DeviceMemory tmp;
    T* buf = tmp.alloc<T>(W * chunk);
    T* hal = tmp.alloc<T>(4 * hc);
    // (the first one is kept: the ranks agree on the outcome of their allocations through it)
    double* red = agree_buf_ ? tmp.alloc<double>(64) : (agree_buf_ = mem_.alloc<double>(64));
    std::string why;
    auto put = [&](T* dst, size_t n) { SIPX_HIP(hipMemcpy(dst, h.data(), n * sizeof(T), hipMemcpyHostToDevice)); };
    auto get = [&](const T* src, size_t n) {
      SIPX_HIP(hipStreamSynchronize(stream_));
      SIPX_HIP(hipMemcpy(h.data(), src, n * sizeof(T), hipMemcpyDeviceToHost));
    };
    auto fill_halo = [&](T* base) {            // [send_prev | send_next | recv_prev | recv_next], hc entries each
      for (size_t j = 0; j < hc; ++j) { h[j] = (T)((R + 1) * 4096 + (int)j); h[hc + j] = (T)((R + 1) * 4096 + 2048 + (int)j); h[2 * hc + j] = h[3 * hc + j] = T(-1); }
      put(base, 4 * hc);
    };
    auto check_halo = [&](const T* base, const char* what) {
      get(base, 4 * hc);
      for (size_t j = 0; j < hc; ++j) {
        if (prev >= 0 && h[2 * hc + j] != (T)(R * 4096 + 2048 + (int)j)) { why = std::string(what) + ": the plane received from the rank below is not what it sent"; return false; }
        if (next >= 0 && h[3 * hc + j] != (T)((R + 2) * 4096 + (int)j)) { why = std::string(what) + ": the plane received from the rank above is not what it sent"; return false; }
        if (prev < 0 && h[2 * hc + j] != T(-1)) { why = std::string(what) + ": a receive buffer without a neighbour was written"; return false; }
      }
      return true;
    };
    auto red_fill = [&]() {
      for (int i = 0; i < 64; ++i) hr[i] = (double)((R + 1) * 1000 + i);
      SIPX_HIP(hipMemcpy(red, hr.data(), 64 * sizeof(double), hipMemcpyHostToDevice));
    };
    auto red_check = [&](const char* what) {
      SIPX_HIP(hipStreamSynchronize(stream_));
      SIPX_HIP(hipMemcpy(hr.data(), red, 64 * sizeof(double), hipMemcpyDeviceToHost));
      for (int i = 0; i < 64; ++i)
        if (hr[i] != 1000.0 * W * (W + 1) / 2 + (double)W * i) { why = std::string(what) + ": the all-reduced sums are wrong"; return false; }
      return true;
    };
    bool ok = true, mapped_ok = true, a2a_ok = true;
    try {
      // A: grouped all-reduce + neighbour exchange, plain memory
      red_fill();
      fill_halo(hal);
      c.allreduce_with_halo(red, 64, SIPX_F64, hal, hal + 2 * hc, prev, hal + hc, hal + 3 * hc, next, hc, dt, stream_);
      ok = red_check("all-reduce + neighbour exchange") && check_halo(hal, "all-reduce + neighbour exchange");
      // B: reduce-scatter in place
      if (ok) {
        for (size_t q = 0; q < W * chunk; ++q) h[q] = (T)val(R, q);
        put(buf, W * chunk);
        c.reduce_scatter_sum(buf, chunk, dt, stream_);
        get(buf, W * chunk);
        for (size_t q = R * chunk; q < (R + 1) * chunk && ok; ++q)
          if (h[q] != (T)(256.0 * W * (W + 1) / 2 + (double)W * (double)(q & 255))) { ok = false; why = "reduce-scatter (in place): the rank's range does not hold the sums"; }
      }
      // C: all-gather in place
      if (ok) {
        for (size_t q = 0; q < W * chunk; ++q) h[q] = (q / chunk == (size_t)R) ? (T)val(R, q) : T(-3);
        put(buf, W * chunk);
        c.allgather(buf, chunk, dt, stream_);
        get(buf, W * chunk);
        for (size_t q = 0; q < W * chunk && ok; ++q)
          if (h[q] != (T)val((int)(q / chunk), q)) { ok = false; why = "all-gather (in place): a range does not hold its rank's values"; }
      }
      // D: fan scatter from rank 0, fan gather to the last rank
      if (ok) {
        for (size_t q = 0; q < W * chunk; ++q) h[q] = R == 0 ? (T)(val((int)(q / chunk), q) + 7.0) : T(-5);
        put(buf, W * chunk);
        c.scatter(buf, chunk, dt, 0, stream_);
        get(buf, W * chunk);
        for (size_t q = R * chunk; q < (R + 1) * chunk && ok; ++q)
          if (h[q] != (T)(val(R, q) + 7.0)) { ok = false; why = "scatter: the rank's range is not what the root sent"; }
      }
      if (ok) {
        for (size_t q = 0; q < W * chunk; ++q) h[q] = (q / chunk == (size_t)R) ? (T)(val(R, q) + 11.0) : T(-7);
        put(buf, W * chunk);
        c.gather(buf, chunk, dt, W - 1, stream_);
        get(buf, W * chunk);
        if (R == W - 1)
          for (size_t q = 0; q < W * chunk && ok; ++q)
            if (h[q] != (T)(val((int)(q / chunk), q) + 11.0)) { ok = false; why = "gather: a range at the root is not what its rank sent"; }
      }
    } catch (const std::exception& ex) {
      ok = false;
      why = std::string("an operation failed: ") + ex.what();
    }
    // D2 (only where a set needs it: the slab-decomposed DFT): all-to-all -- range d of what rank r sends carries (r, d).  A failure
    // here does not fail sipx_finalize: the set goes through an owner rank instead (two fan exchanges), on every rank alike.
    if (ok && want_a2a) {
      T* a2a = nullptr;
      try {
        a2a = tmp.alloc<T>(3 * W * chunk);
        for (size_t q = 0; q < W * chunk; ++q) h[q] = (T)((R + 1) * 64 + (int)(q / chunk) + (double)(q & 15) / 16.0);
        put(a2a, W * chunk);
        c.alltoall(a2a, a2a + W * chunk, a2a + 2 * W * chunk, chunk, dt, stream_);
        get(a2a + W * chunk, W * chunk);
        for (size_t q = 0; q < W * chunk && a2a_ok; ++q)
          if (h[q] != (T)(((int)(q / chunk) + 1) * 64 + R + (double)(q & 15) / 16.0)) { a2a_ok = false; a2a_why_ = "a range is not what its rank sent to this one"; }
      } catch (const std::exception& ex) {
        a2a_ok = false;
        a2a_why_ = ex.what();
      }
      tmp.release(a2a);
    }
    // E: the neighbour exchange out of / into the memory of a sparse array (one mapped granule between two that are not)
    if (ok && want_mapped) {
      try {
        T* vm_base = (T*)tmp.alloc_sparse(3 * SPARSE_GRAN, {{SPARSE_GRAN, 2 * SPARSE_GRAN}}, device_);
        T* vm = (T*)((char*)vm_base + SPARSE_GRAN) + 64;
        red_fill();
        fill_halo(vm);
        c.allreduce_with_halo(red, 64, SIPX_F64, vm, vm + 2 * hc, prev, vm + hc, vm + 3 * hc, next, hc, dt, stream_);
        std::string keep = why;
        mapped_ok = red_check("mapped memory") && check_halo(vm, "mapped memory");
        if (!mapped_ok) mapped_why_ = why;
        why = keep;
      } catch (const std::exception& ex) {
        mapped_ok = false;
        mapped_why_ = ex.what();
      }
    }
    if (const char* f = env_knobs().comm_selftest_fail; f[0]) {      // SIPX_COMM_SELFTEST_FAIL (tests): "mapped" / "base", optionally ":rank" (one rank only)
      const char* colon = std::strchr(f, ':');
      if (!colon || std::atoi(colon + 1) == R) {
        if (!std::strncmp(f, "mapped", 6) && want_mapped) { mapped_ok = false; mapped_why_ = "test hook"; }
        if (!std::strncmp(f, "base", 4)) { ok = false; why = "test hook"; }
        if (!std::strncmp(f, "alltoall", 8) && want_a2a) { a2a_ok = false; a2a_why_ = "test hook"; }
      }
    }
    // the verdict, the same on every rank
    bool all_ok = ok, all_mapped = mapped_ok, all_a2a = a2a_ok;
    try {
      hr[0] = 4096.0 + (ok ? 0.0 : 1.0);
      hr[1] = 4096.0 + (mapped_ok ? 0.0 : 1.0);
      hr[2] = 4096.0 + (a2a_ok ? 0.0 : 1.0);
      SIPX_HIP(hipMemcpy(red, hr.data(), 3 * sizeof(double), hipMemcpyHostToDevice));
      c.allreduce_sum(red, 3, SIPX_F64, stream_);
      SIPX_HIP(hipStreamSynchronize(stream_));
      SIPX_HIP(hipMemcpy(hr.data(), red, 3 * sizeof(double), hipMemcpyDeviceToHost));
      all_ok = hr[0] == 4096.0 * W;
      all_mapped = hr[1] == 4096.0 * W;
      all_a2a = hr[2] == 4096.0 * W;
    } catch (const std::exception& ex) {
      all_ok = false;
      if (why.empty()) why = std::string("the verdict's all-reduce failed: ") + ex.what();
    }
    if (!all_ok)
      throw std::runtime_error("communicator self-test failed (" + std::string(c.kind()) + ", rank " + std::to_string(R) + " of " + std::to_string(W) +
                               "): " + (why.empty() ? std::string("another rank reports wrong data") : why));
    selftest_ = "passed";
    if (want_mapped && !all_mapped) {
      selftest_ = "passed; exchange out of hipMemMap-backed memory failed (" + (mapped_why_.empty() ? std::string("on another rank") : mapped_why_) +
                  "): full-size arrays";
      selftest_mapped_failed_ = true;
    }
    if (want_a2a && !all_a2a) {
      selftest_ += "; all-to-all failed (" + (a2a_why_.empty() ? std::string("on another rank") : a2a_why_) + "): the l1-DFT set through an owner rank";
      selftest_alltoall_failed_ = true;
    }
  }

  // An array over the grid: `total` elements, entry g of block q at front + q * bstride + g.  Full size, or (slab_local_) backed
  // by memory for the grid points [wlo_, whi_) of every block only.
  T* galloc(long long total, long long front, int nblk, long long bstride, Mem kind = Mem::Zeroed) {
    if (!slab_local_) return mem_.alloc<T>((size_t)total, kind);
    std::vector<std::pair<size_t, size_t>> rg;
    for (int q = 0; q < std::max(nblk, 1); ++q) {
      const long long lo = std::max<long long>(0, front + (long long)q * bstride + wlo_);
      const long long hi = std::min<long long>(total, front + (long long)q * bstride + whi_);
      if (hi > lo) rg.push_back({(size_t)lo * sizeof(T), (size_t)hi * sizeof(T)});
    }
    return (T*)mem_.alloc_sparse((size_t)total * sizeof(T), rg, device_, kind);
  }

  // A rank's part of a whole vector of the exchange layout (sparse arrays, a materialised set this rank does not project whole):
  // backed for its chunk of the layout -- what a fan gather sends and a scatter receives -- and for the planes its kernels touch
  // around its slab.
  T* loose_alloc(long long Npad) {
    const long long c0 = (long long)comm_->rank * chunk_, c1 = c0 + chunk_;
    const long long lo = std::min(std::max<long long>(0, wlo_), c0), hi = std::min(Npad, std::max(std::max<long long>(0, whi_), c1));
    std::vector<std::pair<size_t, size_t>> rg{{(size_t)lo * sizeof(T), (size_t)hi * sizeof(T)}};
    return (T*)mem_.alloc_sparse((size_t)Npad * sizeof(T), rg, device_);
  }

  // does the sweep take this context / iteration?  (asked before any search is queued; fills the layout part of `ma`)
  bool sweep_applicable(int flags, MultiArgs<T>& ma, bool planning = false) {
    if (!yl_multi_ || mk_ || (comm_ && !slab_)) return false;
    const bool feas = (flags & SIPX_YL_FEAS) != 0;
    ma.nblk = 0;
    ma.rhs = nullptr;
    ma.flags = flags;
    const long long nlast = G_.n[ndim_ - 1];
    ma.zlo = 0; ma.zhi = nlast; ma.zsum = 0;
    if (slab_ && !planning) {                   // the rank's planes, plus the last plane of the rank below (recomputed, see Gyl_)
      ma.zsum = r0_ / plane_;
      ma.zlo = ma.zsum - ((prev_ >= 0 && r1_ > r0_) ? 1 : 0);
      ma.zhi = r1_ / plane_;
      if (r1_ <= r0_) ma.zlo = ma.zhi = ma.zsum = 0;
    }
    bool behind = false;                        // a loose set has been seen: what follows is not part of the fused right-hand side
    for (int i = 0; i < p_n_; ++i) {
      const SetState<T>& s = sets_[i];
      if (planning ? !sweep_eligible(s) : !s.in_sweep) {
        // a set the sweep cannot take: it keeps its per-set kernels (one rank only; never a caller-supplied sparse operator,
        // whose right-hand side term is added out of order)
        // (... or slab-decomposed, the sets projected on a materialised v: SetState::slab_ext, fan)
        if ((slab_ && !(s.slab_ext || s.fan || s.slab_card || s.slab_dft)) || (comm_ && !slab_) || s.custom || !s.owned || s.dist_ext || (planning ? false : !sweep_partial_)) return false;
        behind = true;
        continue;
      }
      if (ma.nblk + s.nblk_or1() > MULTI_MAXB) return false;
      // (the sweep takes the feasibility estimate of an element-wise set on the identity only)
      if (feas && i < pp_n_ && !s.two_pass && s.nblk > 0) return false;
      for (int qb = 0; qb < s.nblk_or1(); ++qb) {
        MultiBlk<T>& B = ma.b[ma.nblk++];
        B.dir = s.nblk == 0 ? -1 : s.dir[qb];
        B.last = qb == s.nblk_or1() - 1;
        B.dist = s.is_dist ? 1 : 0;
        B.prox = s.prox;
        B.in_rhs = behind ? 0 : 1;
      }
    }
    if (ma.nblk == 0) return false;
    return K<T>::yl_multi(stream_, G_, ma, true);
  }
  static bool sweep_eligible(const SetState<T>& s) {
    return s.owned && !s.custom && !s.ext_kind && !s.dist_ext &&
           (s.prox == PX_BOUNDS || s.prox == PX_L1 || s.prox == PX_PROX_L1 || s.prox == PX_L2 || s.prox == PX_ANNULUS || s.prox == PX_DIST);
  }

  // set j of a lock-step group in the arguments of the two launches that close the first stage of all its searches (sums of the
  // partial slots + packing; decision + unpacking + solve): fseg: a set's header segment, rank_off: where this rank's segments
  // start in fbuf_, cap_max: what a final bracket may gather (0: no exchange)
  void spec_fill(const LockStep& L, size_t j, long long fseg, long long rank_off, double cap_max, SpecPackArgs<T>& pk, SpecFinishArgs<T>& fa) {
    const SetState<T>& s = sets_[L.tp[j]];
    ProjScalars<T>* ps = L.feas_ps ? s.psf : s.ps;
    SpecPackSet<T>& P = pk.s[j];
    P.ps = ps; P.partials = s.ptmp; P.maxpart = s.mpart; P.compact = s.cbuf;
    P.seg = fbuf_ + rank_off + (long long)j * fseg;
    P.is_l1 = s.prox == PX_L1 ? 1 : 0;
    SpecFinishSet<T>& F = fa.s[j];
    F.ps = ps;
    F.da = DecideArgs{L.args[j].prox, (L.args[j].flags & F_NOSPEC) ? 1 : 0, (double)L.args[j].plo, (double)L.args[j].phi, cap_max, s.Mtrue};
    F.reg = stage_ + j * L.RS;
    F.fseg0 = fbuf_ + (long long)j * fseg;
    F.compact = s.cbuf; F.partials = s.ptmp; F.radius = L.args[j].phi;
    F.host_want = L.ctl[j].host_want; F.verdict = L.ctl[j].verdict;
  }

  // Threshold / scale searches of the two-pass sets of a lock-step group on a slab-decomposed grid through the SPECULATIVE
  // EXCHANGE (used for the searches of the y/l update, and -- L.feas_ps, L.v_is_s -- for those of the feasibility estimates, on the
  // sets' second scalar state and v = A x itself).
  void spec_exchange_searches(LockStep& L, int it) {
    const std::vector<int>& tp = L.tp;
    // SPECULATIVE EXCHANGE (kernels_proj.hip, k_spec_pack): first pass of every set, then ONE all-gather carrying every
    // rank's probe sums and the magnitudes it gathered inside the speculative range.  Every rank adds the sums up itself,
    // decides, and -- when the range held theta, the rule once rho and gamma move slowly -- solves from the gathered values:
    // one collective per iteration for all the searches.  Whether a set needs its fallback (refinement rounds with an
    // all-reduce each, then the full-size exchange) the host reads from a pinned word per set; the decision kernel,
    // the unpacking and the solve are queued before that wait, so the device does not idle on it.
    const long long fseg = hooks_.fcap + fast_hdr<T>();
    const long long fchunk = (long long)tp.size() * fseg;
    const unsigned seq = ++spec_seq_ & 0x3fffffffu;
    for (size_t j = 0; j < tp.size(); ++j) {
      L.ctl[j].verdict = (unsigned*)hverd_ + tp[j];
      L.ctl[j].seq = seq;
    }
    if ((int)tp.size() <= SPEC_MAX_SETS) {
      // Batched form (the default): every set's first pass on the engine stream, then TWO launches for all sets -- sums of
      // the partial slots + packing, and, after the all-gather, decision + unpacking + solve (one workgroup per set).  A rank's
      // share of the grid is small when the ranks are many and the iteration is then bound by the launches the host can
      // issue: 21 small kernels and four cross-stream dependencies of three searches become 8 launches on one stream.
      SpecPackArgs<T> pk;
      SpecFinishArgs<T> fa;
      pk.nsets = fa.nsets = (int)tp.size();
      pk.cap = hooks_.fcap;
      fa.world = comm_->world; fa.fchunk = fchunk; fa.seq = seq;
      // (the lean first passes of the l1 sets in one sweep: everything that prepares a search -- rescaling, sampled prediction --
      //  was queued on this very stream before, so the device-side state a lean pass reads is final when the sweep starts)
      if (!L.feas_ps && !L.v_is_s && Gr_.n[0] % 4 == 0) {
        LeanMulti<T> lm;
        lm.ns = 0;
        std::vector<size_t> who;
        for (size_t j = 0; j < tp.size() && lm.ns < LEAN_MAX; ++j) {
          SetState<T>& s = sets_[tp[j]];
          if (s.prox != PX_L1 || (L.args[j].flags & F_NOSPEC)) continue;
          LeanSet<T>& S = lm.s[lm.ns++];
          S.a = L.args[j]; S.a.ps = s.ps; S.ps = s.ps; S.compact = s.cbuf; S.partials = s.ptmp; S.maxpart = s.mpart;
          who.push_back(j);
        }
        if (lm.ns >= 2) {
          K<T>::lean_multi(stream_, Gr_, lm);
          for (size_t j : who) {
            L.ctl[j].lean_done = 1;
            L.ctl[j].lean_known = (hlean_[tp[j]] >> 16) & 1;       // published by the set's last solve: its full first pass need not be launched
          }
        }
      }
      for (size_t j = 0; j < tp.size(); ++j) {
        search_stage(13, stream_, L, j);
        spec_fill(L, j, fseg, (long long)comm_->rank * fchunk, (double)hooks_.gcap, pk, fa);
      }
      K<T>::spec_sums_pack(stream_, pk);
      comm_->allgather(fbuf_, (size_t)fchunk, dtype_code(), stream_);
      K<T>::spec_finish(stream_, fa);
    } else {
      // The sets' chains of small kernels (slot sums, packing; decision, unpacking, solve) run side by side on the set
      // streams -- every set has its own partial slots, gather buffer and segments -- the collective itself on the engine stream.
      auto in_group = [&tp](int i) { return std::binary_search(tp.begin(), tp.end(), i); };
      auto stream_of = [this](const SetState<T>& s) { return (set_streams_ && s.st) ? s.st : stream_; };
      if (set_streams_) SIPX_HIP(hipEventRecord(ev_fork_, stream_));
      for (size_t j = 0; j < tp.size(); ++j) {
        hipStream_t q = stream_of(sets_[tp[j]]);
        if (q != stream_) SIPX_HIP(hipStreamWaitEvent(q, ev_fork_, 0));
        search_stage(0, q, L, j);
        search_stage(5, q, L, j, stage_ + j * L.RS, fbuf_ + (long long)j * fseg, fchunk);
      }
      join_set_streams(in_group);
      comm_->allgather(fbuf_, (size_t)fchunk, dtype_code(), stream_);
      if (set_streams_) SIPX_HIP(hipEventRecord(ev_fork2_, stream_));
      for (size_t j = 0; j < tp.size(); ++j) {
        hipStream_t q = stream_of(sets_[tp[j]]);
        if (q != stream_) SIPX_HIP(hipStreamWaitEvent(q, ev_fork2_, 0));
        search_stage(6, q, L, j, stage_ + j * L.RS, fbuf_ + (long long)j * fseg, fchunk);
      }
      join_set_streams(in_group);
    }
    std::vector<size_t> fb;                  // the sets whose search goes on (the same on every rank)
    bool refine = false;
    for (size_t j = 0; j < tp.size(); ++j) {
      const unsigned w = wait_verdict(hverd_ + tp[j], seq);
      if (w & 1u) fb.push_back(j);
      refine |= (w & 2u) != 0;
    }
    spec_searches_ += (long long)tp.size();
    spec_fallbacks_ += (long long)fb.size();
    const bool spec_debug = env_knobs().spec_debug;
    if (spec_debug) {
      for (size_t j : fb) dump_ps(tp[j], stage_ + j * L.RS);
      std::fprintf(stderr, "[sipx spec] it %d:", it);
      for (size_t j = 0; j < tp.size(); ++j) std::fprintf(stderr, " set %d verdict %u", tp[j], (unsigned)(hverd_[tp[j]] & 3u));
      std::fprintf(stderr, "\n");
    }
    if (fb.empty()) return;
    // Fallback (the summed first-pass sums of every set are in its region of stage_, where k_spec_decide left them):
    // refinement rounds -- gated probe pass, ONE all-reduce, decision -- for as long as some set's bracket holds more than
    // the exchange segments take (the host reads that from the sets' pinned words after every round: exactly as many
    // all-reduces as are needed, at most L1_REFINES_SLAB), then the compaction of every final bracket and the full-size
    // all-gather.  The sets the exchange settled take no part.
    const int max_rounds = std::max(0, std::min(6, env_knobs().l1_rounds_max));      // SIPX_L1_ROUNDS_MAX (tests): force an overflow
    for (int rep = 0; refine && rep < max_rounds; ++rep) {
      const unsigned rseq = ++spec_seq_ & 0x3fffffffu;
      for (size_t j : fb) search_stage(8, stream_, L, j);
      comm_->allreduce_sum(stage_, tp.size() * L.RS, SIPX_F64, stream_);
      for (size_t j : fb) {
        L.ctl[j].seq = rseq;
        search_stage(9, stream_, L, j);
      }
      refine = false;
      for (size_t j : fb)
        if (sets_[tp[j]].prox == PX_L1) refine |= (wait_verdict(hverd_ + tp[j], rseq) & 2u) != 0;
      spec_rounds_ += 1;
      if (spec_debug) {
        std::fprintf(stderr, "[sipx spec]   round %d -> refine %d\n", rep + 1, (int)refine);
        for (size_t j : fb) dump_ps(tp[j], stage_ + j * L.RS);
      }
    }
    for (int stage : {12, 3}) {
      for (size_t j : fb) search_stage(stage, stream_, L, j);
      if (stage == 12) comm_->allgather(gbuf_, (size_t)L.chunk, dtype_code(), stream_);
    }
  }

  // One rank, the sweep does the updates: the threshold / scale searches of ALL two-pass sets as ONE chain of launches on the
  // engine stream (round 4) -- rescaling after a change of rho and the sampled prediction for every set that asks for them (one
  // launch each), the lean first passes in one sweep that reads x once (k_lean_multi), a full first pass per set only where the
  // host does not know that the pass will be a lean one, then two launches for all sets: sums of the partial slots (+ header),
  // decision + solve (one workgroup per set) -- the batched form of the slab-decomposed search without its exchange.  Whether
  // a set needs its fallback sweeps (theta left the speculative range) the host reads from one pinned word per set, published
  // by the decision before the solve starts: the gated launches of the per-set chains -- three no-ops per search in the common
  // case, each a few microseconds on the critical path -- are only made when they have work, and no stream forks or joins.
  // Per iteration of the headline list: 5 launches instead of 27 on three streams, x read once instead of three times.
  // Same decisions (decide_body with cap_max = 0), same gathered values, same double-double solve: theta bit for bit.
  void batched_searches(int flags, const double* rho, const double* gamma) {
    LockStep L;
    for (int i = 0; i < p_n_; ++i)
      if (sets_[i].two_pass && sets_[i].in_sweep) L.tp.push_back(i);
    if (L.tp.empty()) return;
    run_batched(L, flags, rho, gamma);
    if (flags & SIPX_YL_FEAS) {               // ||P_i(s) - s|| with s = A_i x itself: the sets' second scalar state
      LockStep F;
      F.feas_ps = true;
      for (int i : L.tp)
        if (i < pp_n_) F.tp.push_back(i);
      if (!F.tp.empty()) {
        run_batched(F, flags, rho, gamma);
        for (int i : F.tp) {
          SetArgs<T> a = set_args(sets_[i], (T)rho[i], (T)gamma[i], flags);
          K<T>::proj_dist_set(stream_, Gr_, a, 1, sets_[i].psf, fe2_part(i));
        }
      }
    }
  }
  // the searches of the sets L.tp (L.feas_ps: those of their feasibility estimates) as one chain; fills the rest of L
  void run_batched(LockStep& L, int flags, const double* rho, const double* gamma) {
    const std::vector<int>& tp = L.tp;
    const bool feas_ps = L.feas_ps;
    L.RS = (size_t)(PREP_SLOTS + 1 + 2);
    L.v_is_s = feas_ps ? 1 : 0;
    L.args.resize(tp.size());
    L.ctl.resize(tp.size());
    const long long fseg = fast_hdr<T>();
    const unsigned seq = ++spec_seq_ & 0x3fffffffu;
    const bool vec = Gr_.n[0] % 4 == 0;
    RescaleMulti<T> rs;
    rs.n = 0;
    SampleMulti<T> sm;
    sm.ns = 0;
    auto sample = [&](size_t j, ProjScalars<T>* ps) {
      SampleSet<T>& S = sm.s[sm.ns++];
      S.a = L.args[j]; S.a.ps = ps; S.ps = ps; S.partials = sets_[tp[j]].ptmp; S.reg = nullptr; S.true_len = sets_[tp[j]].Mtrue;
    };
    for (size_t j = 0; j < tp.size(); ++j) {
      SetState<T>& s = sets_[tp[j]];
      L.args[j] = set_args(s, (T)rho[tp[j]], (T)gamma[tp[j]], flags);
      L.ctl[j].verdict = (unsigned*)hverd_ + tp[j];
      L.ctl[j].seq = seq;
      if (feas_ps) {
        // the search of a feasibility estimate comes every tenth iteration: its own last theta is ten iterations old and missed
        // the range every time (three fallbacks of two sweeps each per such iteration: 7 % of the 512^3 window) -- a sampled
        // estimate first, whenever the set's last such search asked for one (device side: ProjScalars::want_sample)
        if (env_knobs().l1_sample && s.prox == PX_L1 && vec) sample(j, s.psf);
        continue;
      }
      const bool rescaled = s.rescaled(L.args[j].rho);
      if (rescaled) { rs.ps[rs.n] = s.ps; rs.factor[rs.n++] = s.rescale_factor(L.args[j].rho); }
      // (the sampled prediction is a launch of its own for all sets here: of the set's SampleCtl the chain takes the pinned word
      //  of the prediction and the number of runs, nothing raises an overflow word without an exchange)
      const SampleCtl c = search_ctl(tp[j], rescaled, vec);
      L.ctl[j].host_want = c.host_want;
      L.ctl[j].runs = c.runs;
      if (c.enable) sample(j, s.ps);
      s.last_rho = L.args[j].rho;
      s.last_gamma = L.args[j].gamma;
    }
    K<T>::ps_rescale_multi(stream_, rs);
    sm.v_is_s = L.v_is_s;
    if (sm.ns > 0) K<T>::sample_multi(10, stream_, Gr_, sm, env_knobs().l1_sample_runs, nullptr);
    // the passes: groups of up to LEAN_MAX sets per launch (x read once per group) -- the lean first passes of the l1 sets whose
    // device-side state asks for one, then the full first passes of everybody else; each kernel returns at once when no set
    // of its group wants it.  (A grid whose lines are no multiple of four points keeps one scalar pass per set.)
    auto group = [&](const std::vector<size_t>& who, size_t from) {
      LeanMulti<T> G;
      G.ns = 0;
      G.v_is_s = L.v_is_s;
      for (size_t k = from; k < who.size() && G.ns < LEAN_MAX; ++k) {
        const size_t j = who[k];
        SetState<T>& s = sets_[tp[j]];
        ProjScalars<T>* ps = feas_ps ? s.psf : s.ps;
        LeanSet<T>& S = G.s[G.ns++];
        S.a = L.args[j]; S.a.ps = ps; S.ps = ps; S.compact = s.cbuf; S.partials = s.ptmp; S.maxpart = s.mpart;
      }
      return G;
    };
    std::vector<size_t> all(tp.size());
    for (size_t j = 0; j < tp.size(); ++j) all[j] = j;
    // the lean first passes of the l1 sets in one sweep (x read once)
    std::vector<size_t> l1s;
    for (size_t j = 0; vec && j < tp.size(); ++j)
      if (sets_[tp[j]].prox == PX_L1 && !(L.args[j].flags & F_NOSPEC)) l1s.push_back(j);
    for (size_t k = 0; k < l1s.size(); k += LEAN_MAX) K<T>::lean_multi(stream_, Gr_, group(l1s, k));
    // (SIPX_PASS_MULTI=1: the FULL first passes and the fallback passes of a group in one sweep as well -- measured and NOT the
    //  default: eight probes for three sets make that kernel ALU-bound at 161-173 VGPRs, 512^3 first passes 800-1000 us against
    //  3 x 285 us one after the other, refinement 1009 against 3 x 264; 512^3 116.2 against 118.7 it/s.  SIPX_PASS_MULTI=1, tests)
    if (vec && env_knobs().pass_multi) {
      for (size_t k = 0; k < all.size(); k += LEAN_MAX) K<T>::pass_multi(0, stream_, Gr_, group(all, k), L.v_is_s);
    } else {
      // a full first pass per set only where the host does not know from the set's pinned word that the pass will be a lean
      // one (it returns at once when the device-side state says lean)
      for (size_t j : l1s) {
        L.ctl[j].lean_done = 1;
        L.ctl[j].lean_known = feas_ps ? 0 : ((hlean_[tp[j]] >> 16) & 1);      // published by the set's last solve; nothing since can have taken the flag back
      }
      for (size_t j = 0; j < tp.size(); ++j) search_stage(13, stream_, L, j);
    }
    SpecPackArgs<T> pk;
    SpecFinishArgs<T> fa;
    pk.nsets = fa.nsets = (int)tp.size();
    pk.local = fa.local = 1;
    pk.cap = 0;
    fa.world = 1; fa.fchunk = (long long)tp.size() * fseg; fa.seq = seq;
    for (size_t j = 0; j < tp.size(); ++j) spec_fill(L, j, fseg, 0, 0.0, pk, fa);
    K<T>::spec_sums_pack(stream_, pk);
    K<T>::spec_finish(stream_, fa);
    // Fallback of the sets whose pinned verdict asks for it (theta left the speculative range, or the range gathered too much):
    // refinement pass + decision (where the decision asked for one), compaction of the bracket, solve -- the passes of all
    // such sets in one sweep each.
    std::vector<size_t> fb;
    bool refine = false;
    for (size_t j = 0; j < tp.size(); ++j) {
      const unsigned w = wait_verdict(hverd_ + tp[j], seq);
      batch_searches_ += 1;
      if (!(w & 1u)) continue;
      batch_fallbacks_ += 1;
      if (env_knobs().trace_searches)
        std::fprintf(stderr, "[sipx search] search %lld (set %d%s): fallback%s\n", batch_searches_, tp[j], feas_ps ? ", feasibility" : "", (w & 2u) ? " with refinement" : "");
      fb.push_back(j);
      refine |= (w & 2u) != 0;
    }
    const bool spec_debug = env_knobs().spec_debug;
    if (spec_debug && !feas_ps) {                // (diagnostics: the state every search of the chain ended its first stage with; synchronises)
      std::fprintf(stderr, "[sipx spec] batched chain, search seq %u\n", seq);
      for (size_t j = 0; j < tp.size(); ++j) dump_ps(tp[j], stage_ + j * L.RS);
    }
    if (fb.empty()) return;
    auto tail = [&](int stage) {
      for (size_t j : fb) {
        SetState<T>& s = sets_[tp[j]];
        K<T>::search_tail(stage, stream_, L.args[j], feas_ps ? s.psf : s.ps, s.ptmp, s.mpart, s.cbuf, s.Mtrue, L.ctl[j], stage_ + j * L.RS);
      }
    };
    if (vec && env_knobs().pass_multi) {
      if (refine) {
        for (size_t k = 0; k < fb.size(); k += LEAN_MAX) K<T>::pass_multi(1, stream_, Gr_, group(fb, k), L.v_is_s);
        tail(1);
      }
      for (size_t k = 0; k < fb.size(); k += LEAN_MAX) K<T>::pass_multi(2, stream_, Gr_, group(fb, k), L.v_is_s);
      tail(3);
    } else {
      for (size_t j : fb)
        for (int stage : {1, 2, 3})
          if (stage != 1 || refine) search_stage(stage, stream_, L, j);
    }
  }

  // one rank (or no communicator): the searches of the two-pass sets on the set streams, joined before the sweep
  void sweep_searches(int flags, const double* rho, const double* gamma) {
    const bool feas = (flags & SIPX_YL_FEAS) != 0;
    // The lean first passes of the l1 searches in ONE sweep (k_lean_multi: x read once): on iterations where no search of the
    // group is rescaled or sampled first (the device-side state a lean pass needs is then final when the engine stream gets
    // here), for two or three l1 sets on stencil operators of this grid.  Each set's chain then launches its full first
    // pass only, which returns at once for the sets the sweep served.
    std::vector<char> lean_done(p_n_, 0);
    if (lean_multi_ && Gr_.n[0] % 4 == 0) {
      LeanMulti<T> lm;
      lm.ns = 0;
      bool ok = true;
      std::vector<int> who;
      for (int i = 0; i < p_n_ && ok; ++i) {
        SetState<T>& s = sets_[i];
        if (!s.two_pass || !s.in_sweep || s.prox != PX_L1 || s.custom || s.ext_kind) continue;
        SetArgs<T> a = set_args(s, (T)rho[i], (T)gamma[i], flags);
        if (a.flags & F_NOSPEC) continue;
        const bool rescaled = s.rescaled(a.rho);
        if (rescaled || search_ctl(i, rescaled, true).enable) { ok = false; break; }
        if (lm.ns == LEAN_MAX) break;
        const SetScratch scr = scratch_of(s);
        LeanSet<T>& S = lm.s[lm.ns++];
        S.a = a; S.a.ps = s.ps; S.ps = s.ps;
        S.compact = scr.cbuf; S.partials = scr.ptmp; S.maxpart = scr.mpart;
        who.push_back(i);
      }
      bool own = true;                     // every set of the group needs scratch of its own
      for (int i : who) own &= sets_[i].ptmp != nullptr && sets_[i].mpart != nullptr && sets_[i].cbuf != nullptr;
      if (ok && own && lm.ns >= 2) {
        K<T>::lean_multi(stream_, Gr_, lm);
        for (int i : who) lean_done[i] = 1;
      }
    }
    if (set_streams_) SIPX_HIP(hipEventRecord(ev_fork_, stream_));       // x is final: the searches may start
    for (int i = 0; i < p_n_; ++i) {
      SetState<T>& s = sets_[i];
      if (!s.two_pass || !s.in_sweep) continue;
      SetArgs<T> a = set_args(s, (T)rho[i], (T)gamma[i], flags);
      hipStream_t q = s.st ? s.st : stream_;
      const SetScratch scr = scratch_of(s);
      if (q != stream_) SIPX_HIP(hipStreamWaitEvent(q, ev_fork_, 0));
      const bool rescaled = s.rescaled(a.rho);
      if (rescaled) K<T>::ps_rescale(q, s.ps, s.rescale_factor(a.rho));
      SampleCtl ctl = search_ctl(i, rescaled, true);
      ctl.lean_done = lean_done[i];
      K<T>::proj_scalars_set(q, Gr_, a, 0, s.ps, scr.ptmp, scr.mpart, scr.cbuf, s.Mtrue, ctl, nullptr);
      s.last_rho = a.rho;
      s.last_gamma = a.gamma;
      if (feas && i < pp_n_) {                 // ||P_i(s) - s|| with s = A_i x produced on the fly; its own warm-started scalars
        SampleCtl cf;                          // (a sampled estimate first, as in the batched chain: run_batched)
        cf.runs = env_knobs().l1_sample_runs;
        cf.enable = env_knobs().l1_sample && a.prox == PX_L1;
        K<T>::proj_scalars_set(q, Gr_, a, 1, s.psf, scr.ptmp, scr.mpart, scr.cbuf, s.Mtrue, cf, nullptr);
        K<T>::proj_dist_set(q, Gr_, a, 1, s.psf, fe2_part(i));
      }
    }
    join_set_streams([this](int i) { return sets_[i].two_pass && sets_[i].in_sweep; });      // theta / scale of every set are known
  }

  // The y/l update of EVERY set in one sweep over the grid (kernels_multi.hip), on the engine stream, once the threshold /
  // scale of every two-pass set is known: one kernel updates all sets, forms the r_pri / r_dual / obj sums -- on
  // Barzilai-Borwein iterations the six BB sums and the snapshot refresh, every tenth iteration the feasibility estimates of
  // the element-wise sets -- and, when the caller has announced that rho cannot change before the next iteration (YlPlan::fuse_rhs),
  // writes the right-hand side of that iteration.
  // The sweep never updates in place (neighbouring tiles re-read the OLD y, l of a few points): it writes into the pair that
  // holds the old snapshot (BB / first iteration: it is read first), into the free pair, or -- when both other pairs are
  // taken, i.e. the snapshot must survive and sits in the other pair -- into a third pair, allocated by sipx_finalize.
  // (The per-set kernels may write in place and have two pairs: their rule is aim / rotate.)
  void sweep_launch(int flags, const double* rho, const double* gamma, MultiArgs<T>& ma, bool fuse_rhs) {
    const bool first = (flags & SIPX_YL_FIRST) != 0, bb = (flags & SIPX_YL_BB) != 0 && !first;
    ma.nblk = 0;
    std::vector<int> target(p_n_, 0);          // 0: the other pair (y0, l0); 2: the third pair
    bool behind = false;
    for (int i = 0; i < p_n_; ++i) {
      SetState<T>& s = sets_[i];
      if (!s.in_sweep) { behind = true; target[i] = -1; continue; }
      SetArgs<T> a = set_args(s, (T)rho[i], (T)gamma[i], flags);
      target[i] = (!first && !bb && s.snap == 1) ? 2 : 0;
      if (target[i] == 2 && !s.y2) throw std::runtime_error("internal: the third y / l pair of the sweep was not allocated at sipx_finalize");
      T* ty = target[i] == 2 ? s.y2 : s.y0;
      T* tl = target[i] == 2 ? s.l2 : s.l0;
      for (int qb = 0; qb < s.nblk_or1(); ++qb) {
        MultiBlk<T>& B = ma.b[ma.nblk++];
        const long long off = (long long)qb * G_.N;
        B.y = s.y + off; B.l = s.l + off;
        B.yo = ty + off; B.lo = tl + off;
        B.lh0 = s.lh0 + off; B.s0 = s.s0 + off;
        B.y0 = a.y0 + off; B.l0 = a.l0 + off;         // the snapshot pair (set_args)
        B.ps = s.ps;
        B.dir = s.nblk == 0 ? -1 : s.dir[qb];
        B.set = i;
        B.first = qb == 0;
        B.last = qb == s.nblk_or1() - 1;
        B.dist = s.is_dist ? 1 : 0;
        B.feas_el = (i < pp_n_ && (s.prox == PX_BOUNDS || s.prox == PX_PROX_L1)) ? 1 : 0;
        B.ih = s.nblk == 0 ? T(0) : s.ih[qb];
        B.rho = a.rho; B.rho1 = a.rho1; B.gamma = a.gamma;
        B.prox = s.prox; B.plo = s.plo; B.phi = s.phi;
        B.in_rhs = behind ? 0 : 1;
      }
    }
    ma.x = x_; ma.m = m_; ma.xold = xold_;
    // x0 mode: s_0 = A x_0 from the ring buffer that held x on the last BB / first iteration; the new snapshot is x itself --
    // the coming x-steps leave its buffer alone (argmin_x)
    ma.x0 = (x0_mode_ && x_snap_ >= 0) ? xr_[x_snap_] : (x0_mode_ ? x_ : nullptr);
    ma.x0w = nullptr;
    ma.rhs = fuse_rhs ? rhs_ : nullptr;
    ma.partials = part_sets_;
    if (!K<T>::yl_multi(stream_, G_, ma)) throw std::runtime_error("internal: the fused y/l sweep refused a block list it was prepared for");
    rhs_fused_ = ma.rhs != nullptr;
    if (x0_mode_ && (first || bb)) x_snap_ = x_cur_;
    for (int i = 0; i < p_n_; ++i) {           // (y, l) always names the current iterate; snap says where the snapshot sits
      SetState<T>& s = sets_[i];
      if (target[i] < 0) continue;
      if (target[i] == 2) {
        std::swap(s.y, s.y2); std::swap(s.l, s.l2);                     // the snapshot stays in (y0, l0)
      } else {
        std::swap(s.y, s.y0); std::swap(s.l, s.l0);
        if (first || bb) s.snap = 0;                                    // the pair just written IS the new snapshot
        else if (s.snap == 0) s.snap = 1;                               // the snapshot stayed behind in what is now (y0, l0)
      }
    }
  }

  // second half of update_y_l: waits for the reduced sums and turns them into the per-set scalars.  The whole-solve loop
  // calls it late (YlPlan::collect_now off), after it has queued the work of the next iteration that cannot depend on them.
  void collect_set_sums(YlPlan::Route route, const double* rho, double* r_pri, double* r_dual, double* feas) {
    if (!sums_pending_) throw std::runtime_error("no y/l update is pending");
    sums_pending_ = false;
    const int flags = sums_flags_;
    if (route == YlPlan::Route::ByWord) wait_word(sums_word_, sums_seq_);
    else SIPX_HIP(hipEventSynchronize(sums_event_));
    have_log_sums_ = false;
    if (slab_) {
      // a threshold search whose final bracket, over all ranks, held more magnitudes than the exchange segments: every rank saw
      // the same segment headers and raised its word, so every rank leaves here with the same error -- never with NaN iterates
      for (int i = 0; i < p_n_; ++i) {
        if (!hovf_[i]) continue;
        for (int k = 0; k <= p_n_; ++k) hovf_[k] = 0;
        ProjScalars<T> h;                    // what the search knew when it gave up (diagnostics): the update's search or the feasibility estimate's
        SIPX_HIP(hipStreamSynchronize(stream_));
        char dbg[512];
        int at = 0;
        for (const ProjScalars<T>* d : {sets_[i].ps, sets_[i].psf}) {
          if (!d) continue;
          SIPX_HIP(hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost));
          if (!h.gather_overflow) continue;
          at += std::snprintf(dbg + at, sizeof dbg - at, " [%s: bracket (%.9g, %.9g], refinement rounds %d, ||v||_1 %.6g, radius %.6g, speculative range (%.9g, %.9g]]",
                              d == sets_[i].ps ? "y/l update" : "feasibility estimate", h.lo, h.hi, h.rounds_used, h.asum, (double)sets_[i].phi, h.spec_lo, h.spec_hi);
        }
        dbg[at] = 0;
        throw std::runtime_error(std::string(sets_[i].prox == PX_CARD ? "cardinality search" : "l1 threshold search") + " of set " + std::to_string(i) + ": the magnitudes inside the final bracket, gathered over all "
                                 "ranks, exceed the exchange segment of " + std::to_string(hooks_.gcap) + " values per rank "
                                 "(slab decomposition) after the refinement rounds of the search; the iterate of this step is not valid -- "
                                 "use the set decomposition for this problem" + std::string(dbg));
      }
    }
    const bool all = comm_ != nullptr;       // sharded: the all-reduced sums of every set are here, on every rank
    for (int i = 0; i < p_n_; ++i) {
      SetState<T>& s = sets_[i];
      if (r_pri) r_pri[i] = 0;
      if (r_dual) r_dual[i] = 0;
      if (!s.owned && !all) continue;
      const double* h = hres_ + (size_t)i * SLOTS;
      std::copy(h, h + SLOTS, s.sums);
      if (r_pri) r_pri[i] = (double)(T)std::sqrt(h[SL_RPRI]);                                   // update_y_l.jl:81
      // :84; in Minkowski mode [A A]'d = [A'd; A'd] doubles the sum of squares
      if (r_dual) r_dual[i] = (double)((T)rho[i] * (T)std::sqrt((s.comp == 3 ? 2.0 : 1.0) * (s.ident ? h[SL_DY] : h[SL_ADJ])));
      s.bb_valid = (flags & (SIPX_YL_BB | SIPX_YL_FIRST)) != 0;
      if (s.is_dist) {
        obj_ss_ = h[SL_OBJ]; evo_ss_ = h[SL_EVO]; xx_ss_ = h[SL_XX];     // obj = 1/2 ||TD_OP[end] x - m||^2  PARSDMM.jl:139-143
        if (mk_) { evo_ss_ = hres_[(size_t)p_n_ * SLOTS + SL_EVO]; xx_ss_ = hres_[(size_t)p_n_ * SLOTS + SL_XX]; }
        have_log_sums_ = true;
      }
    }
    if (all && !slab_dist_logs_) {           // the slab sums of argmin_x: the distance-term kernel saw x_old on its own slab only
      const double* g = hres_ + (size_t)p_n_ * SLOTS;
      obj_ss_ = g[SL_OBJ]; evo_ss_ = g[SL_EVO]; xx_ss_ = g[SL_XX];
      have_log_sums_ = true;
    }
    if ((flags & SIPX_YL_FEAS) && feas) {
      for (int i = 0; i < pp_n_; ++i) {
        feas[i] = 0;
        if (!sets_[i].owned && !all) continue;
        const double* h = hres_ + (size_t)i * SLOTS;
        feas[i] = (sets_[i].two_pass || sets_[i].ext_kind) ? (double)feas_value(h[SL_FE2], h[SL_SS2])
                                                            : (double)feas_value(h[SL_FE], h[SL_SS]);
      }
    }
  }

  void log_scalars(double* obj, double* evol_x) override {
    need_final();
    ObserverGuard og(observer());
    if (!have_log_sums_) {
      K<T>::log3(stream_, G_.N, mk_ ? w_ : x_, m_, xold_, part_sets_);
      if (mk_) K<T>::log3(stream_, Nx_, x_, (const T*)nullptr, xold_, part_sets_ + (size_t)SLOTS * NB);
      K<T>::fin_sum(stream_, part_sets_, (mk_ ? 2 : 1) * SLOTS, nullptr, hres_);
      SIPX_HIP(hipStreamSynchronize(stream_));
      obj_ss_ = hres_[SL_OBJ]; evo_ss_ = hres_[SL_EVO]; xx_ss_ = hres_[SL_XX];
      if (mk_) { evo_ss_ = hres_[SLOTS + SL_EVO]; xx_ss_ = hres_[SLOTS + SL_XX]; }
    }
    const T nd = (T)std::sqrt(obj_ss_);
    *obj = (double)(T(0.5) * (nd * nd));                                   // PARSDMM.jl:140
    *evol_x = (double)((T)std::sqrt(evo_ss_) / (T)std::sqrt(xx_ss_));      // PARSDMM.jl:145
  }

  void adapt_rho_gamma(int adjust_rho, int adjust_gamma, double* rho_io, double* gamma_io) override {
    need_final();
    for (int i = 0; i < p_n_; ++i) {
      SetState<T>& s = sets_[i];
      if (!s.owned && !comm_) continue;
      if (!s.bb_valid)
        throw std::runtime_error("sipx_adapt_rho_gamma: call sipx_update_y_l with SIPX_YL_BB (or _FIRST) first");
      T rho = (T)rho_io[i], gamma = (T)gamma_io[i];
      const double* h = s.sums;
      bb_rule<T>((T)h[SL_HL], (T)std::sqrt(h[SL_HH]), (T)std::sqrt(h[SL_LH]), (T)std::sqrt(h[SL_DL]),
                 (T)std::sqrt(h[SL_GG]), (T)h[SL_GL], adjust_rho != 0, adjust_gamma != 0, rho, gamma);
      rho_io[i] = (double)rho;
      gamma_io[i] = (double)gamma;
    }
  }

  void q_update(const double* rho_new, const double* rho_old) override {
    need_final();
    ObserverGuard og(observer());
    if (stencil_q_) {
      stencil_weights(rho_new);
      return;
    }
    if (mk_) {
      std::vector<T> al(p_n_);
      for (int i = 0; i < p_n_; ++i) al[i] = rho_new[i] == rho_old[i] ? T(0) : (T)rho_new[i] - (T)rho_old[i];
      mk_q_update(al);
      return;
    }
    QArgs<T> a;
    a.nsets = 0;
    for (int i = 0; i < p_n_; ++i) {
      if (rho_new[i] == rho_old[i]) continue;                       // ind_updated, PARSDMM.jl:230
      if (sets_[i].mfree) { sets_[i].mf_rho = (T)rho_new[i]; continue; }   // a matrix-free term: its rho is all Q holds of it
      push_qset(a, sets_[i], (T)rho_new[i] - (T)rho_old[i]);        // Q_update!.jl:47
    }
    q_apply(a);
  }
  // a batch of the Q update (Q[:, b] += alpha_i A_i'A_i[:, b], set order): on the class table while the products use it -- the
  // bands go stale -- else on the bands
  void q_apply(const QArgs<T>& a) {
    if (cds_.qtab) {
      if (K<T>::qtab_update(stream_, G_, cds_, a, qtab_)) {
        q_stale_ = q_stale_ || a.nsets > 0;
        return;
      }
      ensure_q_bands();                    // no plan (explicit A'A bands, SIPX_Q_PLAN=0): the bands for the rest of the context
      cds_.qtab = nullptr;
      qtab_reason_ = "an update without a plan";
    }
    K<T>::q_update(stream_, G_, qr0_, qr1_, cds_, a, Q_);
  }
  // the four stored bands written from the class table, if an update went to the table only: before anything reads Q_ itself
  void ensure_q_bands() {
    if (!q_stale_) return;
    K<T>::qtab_write_bands(stream_, Nx_, cds_, qtab_, Q_);
    q_stale_ = false;
  }
  // The class table of Q (CdsArgs::qtab, kernels_cds.hip): the z-marching products take the coefficients of the 7-band matrix
  // from 4 x 27 values -- one per stored band and boundary class of a row -- instead of loading four bands (8 -> 4, 7 -> 3,
  // 6 -> 2 N w per product), and a planned update touches the table only.  Seeded from the assembled Q and used only if every
  // stored value equals its class's entry bit for bit (the check reads the bands once per solve); a Q that is not constant on
  // the classes (caller-supplied A'A bands that vary per point) keeps the bands.
  void build_q_table() {
    cds_.qtab = nullptr;
    q_stale_ = false;
    const char* why = nullptr;
    if (!env_knobs().q_table) why = "SIPX_Q_TABLE=0";
    else if (stencil_q_) why = "stencil Q";
    else if (mk_) why = "Minkowski";
    else if (comm_) why = "sharded";
    else if (!cds_.march || !cds_.sym || cds_.d != 7) why = "not the 7-band matrix of a 3-D grid";
    else if (qr0_ != 0 || qr1_ != Nx_ || !K<T>::march_applies(Nx_, cds_)) why = "the z-marching product does not apply";
    if (why) {
      qtab_reason_ = why;
      return;
    }
    if (!qtab_) qtab_ = mem_.alloc<T>(QT_N + 8);          // (+ the check's flag)
    int* ok = (int*)(qtab_ + QT_N);
    K<T>::qtab_build(stream_, Nx_, cds_, Q_, qtab_, ok);
    int h = 0;
    SIPX_HIP(hipMemcpyAsync(&h, ok, sizeof(int), hipMemcpyDeviceToHost, stream_));
    SIPX_HIP(hipStreamSynchronize(stream_));
    if (!h) {
      qtab_reason_ = "Q is not constant on the boundary classes";
      return;
    }
    cds_.qtab = qtab_;
    qtab_reason_ = "";
  }

  // Warm start of this (finer) level from a solved coarser one, device to device: x by nearest-neighbour resampling of the
  // grid (PARSDMM_multi_level.jl:61-67), l_i and y_i set by set as interpolate_y_l does (interpolate_y_l.jl:16-94) -- a
  // single-block operator resamples its TD_n-shaped array; TV splits its rows into chunks of the sizes of [D_x; D_y; D_z]
  // blocks (although the storage is [D_z; D_y; D_x]: replicated as written) and resamples each.  The reference's row
  // order is recovered from / restored to the padded layout by the pack / unpack kernels of the import / export path.
  void warm_start_from(EngineBase* coarse_base) override {
    need_final();
    auto* c = dynamic_cast<Engine<T>*>(coarse_base);
    if (!c || !c->finalized_) throw std::runtime_error("warm start: the coarse context must be a finalized context of the same precision");
    if (c->device_ != device_) throw std::runtime_error("warm start: both levels must live on one device");
    if (c->p_n_ != p_n_ || c->ndim_ != ndim_ || mk_ || c->mk_) throw std::runtime_error("warm start: the two levels must hold the same sets");
    if ((comm_ != nullptr) != (c->comm_ != nullptr) || (comm_ && !(slab_ && c->slab_)))
      throw std::runtime_error("warm start between levels of a sharded solve needs both levels slab-decomposed (sipx_set_decomp)");
    // Block by block (x, then l_i and y_i of every set): the coarse block is completed in ONE whole-size temporary of the COARSE
    // level -- an all-gather of the coarse ranks' slabs where that level is slab-decomposed (a collective: every rank makes the same
    // calls); one rank: the block itself -- and resampled from there, padded layout to padded layout (k_resample_padded: entry by entry
    // the copy the reference makes on the chunks in row order, interpolate_y_l.jl:16-94), into the grid points THIS rank stores of
    // the fine block: its planes and the halo planes around them where the fine level holds sparse arrays (round 5: the levels of a
    // slab-decomposed multilevel solve no longer need whole arrays, PARSDMM_multi_level.jl:56-83), all of it otherwise.  A coarse
    // array is 1 / 8 of a fine one: the temporary is the size of a rank's slab of the fine grid on eight GPUs.
    long long nc[3], nf[3];
    for (int a = 0; a < 3; ++a) { nc[a] = c->G_.n[a]; nf[a] = G_.n[a]; }
    const long long Nc = c->G_.N, Nf = G_.N;
    const long long cpad = c->comm_ ? c->chunk_ * c->comm_->world : Nc;
    int nbmax = 1;
    for (auto& st : c->sets_) nbmax = std::max(nbmax, st.nblk_or1());
    DeviceMemory tmp;
    T* whole = c->slab_ ? tmp.alloc<T>((size_t)nbmax * cpad, Mem::NoFill) : nullptr;
    const int dt = dtype_code();
    const long long f0 = slab_local_ ? std::max<long long>(0, wlo_) : 0, f1 = slab_local_ ? std::min<long long>(Nf, whi_) : Nf;
    // (all blocks of a set's coarse vector side by side: a chunk of the reference's row vector may straddle two of them)
    auto complete = [&](const T* src, int nb) -> const T* {
      if (!c->slab_) return src;             // one rank: the blocks themselves (stride Nc)
      const long long nloc = c->r1_ - c->r0_;
      for (int q = 0; q < nb; ++q) {          // the coarse ranks' planes -> the whole block
        T* w = whole + (long long)q * cpad;
        if (nloc > 0) SIPX_HIP(hipMemcpyAsync(w + c->r0_, src + (long long)q * Nc + c->r0_, nloc * sizeof(T), hipMemcpyDeviceToDevice, stream_));
        c->comm_->allgather(w, (size_t)c->chunk_, dt, stream_);
      }
      return whole;
    };
    const long long cstride = c->slab_ ? cpad : Nc;
    SIPX_HIP(hipStreamSynchronize(c->stream_));
    resample_nn_padded<T>(stream_, nc, nf, nc, nf, f0, f1, complete(c->x_, 1), x_);
    for (int i = 0; i < p_n_; ++i) {
      SetState<T>&f = sets_[i], &g = c->sets_[i];
      if (f.custom || g.custom || f.nblk != g.nblk) throw std::runtime_error("warm start: operator kinds differ between the levels");
      if (f.op == SIPX_OP_TV_XY || g.op == SIPX_OP_TV_XY) throw std::runtime_error("warm start: the TV_xy operator is not built for multilevel solves");
      for (int q = 0; q < f.nblk; ++q)
        if (f.dir[q] != g.dir[q]) throw std::runtime_error("warm start: operator kinds differ between the levels");
      if (!f.owned || !g.owned) continue;
      for (int which = 0; which < 2; ++which) {
        const T* src = complete(which ? g.y : g.l, g.nblk_or1());
        T* dst = which ? f.y : f.l;
        if (f.nblk >= 2) {       // TV / D2D / D3D: the reference's D_x-, D_y-, D_z-sized chunks of the row vector (interpolate_y_l.jl:21-30,53-57)
          for (int q = 0; q < f.nblk; ++q)
            resample_nn_rows<T>(stream_, nc, nf, f.nblk, f.dir, q, cstride, f0, f1, src, dst + (long long)q * Nf);
        } else {                 // one block: the grid, minus one along the direction of its difference operator (TD_n, get_TD_operator.jl)
          long long cc[3], cf[3];
          for (int a = 0; a < 3; ++a) { cc[a] = nc[a]; cf[a] = nf[a]; }
          if (f.nblk == 1) { cc[f.dir[0]] -= 1; cf[f.dir[0]] -= 1; }
          resample_nn_padded<T>(stream_, nc, nf, cc, cf, f0, f1, src, dst);
        }
      }
    }
    SIPX_HIP(hipStreamSynchronize(stream_));
  }

  // Slab-decomposed context: completes x and / or the y_i, l_i named on every rank from the ranks' slabs (all-gathers on the
  // engine stream; afterwards the arrays are whole and identical everywhere).  A collective.
  void gather_slabs(bool want_x, const std::vector<char>& want_l, const std::vector<char>& want_y) {
    const int dt = dtype_code();
    if (want_x) comm_->allgather(x_, (size_t)chunk_, dt, stream_);
    for (int i = 0; i < p_n_; ++i)
      for (int which = 0; which < 2; ++which) {
        if (!(which ? want_y[i] : want_l[i])) continue;
        T* arr = which ? sets_[i].y : sets_[i].l;
        const int nb = sets_[i].nblk > 0 ? sets_[i].nblk : 1;
        for (int q = 0; q < nb; ++q) {
          T* blk = arr + (long long)q * G_.N;
          if (r1_ > r0_) SIPX_HIP(hipMemcpyAsync(scr_v_ + r0_, blk + r0_, (r1_ - r0_) * sizeof(T), hipMemcpyDeviceToDevice, stream_));
          comm_->allgather(scr_v_, (size_t)chunk_, dt, stream_);
          SIPX_HIP(hipMemcpyAsync(blk, scr_v_, G_.N * sizeof(T), hipMemcpyDeviceToDevice, stream_));
        }
      }
  }

  // Sparse arrays: nothing whole exists on a rank.  x and the requested y_i, l_i are completed in whole-size TEMPORARIES (the
  // exchange buffer of one N-vector, and the blocks of one set strung together) and go to the host from there.  A collective.
  void download_sparse(void* x, void* const* l, void* const* y) {
    const int dt = dtype_code();
    const long long N = G_.N, Npad = chunk_ * comm_->world, nloc = r1_ - r0_;
    int nbmax = 1;
    for (auto& s : sets_) nbmax = std::max(nbmax, s.nblk_or1());
    DeviceMemory tmp;
    T* exch = tmp.alloc<T>((size_t)Npad);
    T* whole = tmp.alloc<T>((size_t)nbmax * N);
    auto complete = [&](const T* src) {      // src: a block of a sparse array (global indexing); afterwards exch[0, N) holds all of it
      if (nloc > 0) SIPX_HIP(hipMemcpyAsync(exch + r0_, src + r0_, nloc * sizeof(T), hipMemcpyDeviceToDevice, stream_));
      comm_->allgather(exch, (size_t)chunk_, dt, stream_);
    };
    if (x) {
      complete(x_);
      SIPX_HIP(hipStreamSynchronize(stream_));
      host_prefault(x, N * sizeof(T));
      SIPX_HIP(hipMemcpy(x, exch, N * sizeof(T), hipMemcpyDeviceToHost));
      io_d2h_ += N * (long long)sizeof(T);
    }
    for (int i = 0; i < p_n_; ++i)
      for (int which = 0; which < 2; ++which) {
        void* const* dst = which ? y : l;
        if (!(dst && dst[i])) continue;
        const T* arr = which ? sets_[i].y : sets_[i].l;
        for (int q = 0; q < sets_[i].nblk_or1(); ++q) {
          complete(arr + (long long)q * N);
          SIPX_HIP(hipMemcpyAsync(whole + (long long)q * N, exch, N * sizeof(T), hipMemcpyDeviceToDevice, stream_));
        }
        download_rows(sets_[i], whole, (T*)dst[i]);
      }
    SIPX_HIP(hipStreamSynchronize(stream_));
  }

  void download(void* x, void* const* l, void* const* y) override {
    need_final();
    if (slab_local_) { download_sparse(x, l, y); return; }
    if (slab_) {       // every rank holds its planes only: complete x and the requested y, l (a collective: every rank calls it)
      std::vector<char> wl(p_n_, 0), wy(p_n_, 0);
      for (int i = 0; i < p_n_; ++i) { wl[i] = l && l[i]; wy[i] = y && y[i]; }
      gather_slabs(x != nullptr, wl, wy);
    }
    SIPX_HIP(hipStreamSynchronize(stream_));
    if (x) {
      host_prefault(x, Nx_ * sizeof(T));
      SIPX_HIP(hipMemcpy(x, x_, Nx_ * sizeof(T), hipMemcpyDeviceToHost));
      io_d2h_ += Nx_ * (long long)sizeof(T);
    }
    for (int i = 0; i < p_n_; ++i) {
      if (!sets_[i].owned) continue;
      if (l && l[i]) download_rows(sets_[i], sets_[i].l, (T*)l[i]);
      if (y && y[i]) download_rows(sets_[i], sets_[i].y, (T*)y[i]);
    }
  }

  // ------------------------------------------------------------------------------------------
  // Device-resident boundary: m, x0, l0[i], y0[i] and the results x, l[i], y[i] are buffers of the caller on this context's GPU,
  // in the reference's row order.  A call that uses PARSDMM as a projector inside a loop whose data lives on the device
  // (examples/constrained_freq_FWI_simple.jl:468) then moves no N-vector over PCIe.  finalize / reset run as in the host form
  // -- same arrays, same values in the same places, so the solve that follows returns the same bits -- with the uploads
  // replaced by ONE launch that reads the caller's buffers (import_dev); download_dev is one launch that writes them.
  // Ordering: the import waits for an event recorded on the caller's stream, the export records an event the caller's stream
  // waits for; neither waits on the host (sipx_finalize / sipx_reset end with the host wait of the initial feasibility, as ever).
  void need_dev_io(const char* what) const {
    if (comm_ || slab_req_ || !owned_.empty())
      throw std::runtime_error(std::string(what) + " takes single-process contexts only: this one is slab-decomposed or set-sharded (use the host form)");
  }
  void set_caller_stream(void* stream) override {
    SIPX_HIP(hipSetDevice(device_));
    caller_ = (hipStream_t)stream;                      // null: the default stream
    if (!ev_io_in_) SIPX_HIP(hipEventCreateWithFlags(&ev_io_in_, hipEventDisableTiming));
    if (!ev_io_out_) SIPX_HIP(hipEventCreateWithFlags(&ev_io_out_, hipEventDisableTiming));
  }
  void io_bytes(int64_t* host_to_device, int64_t* device_to_host, int reset) override {
    if (host_to_device) *host_to_device = io_h2d_;
    if (device_to_host) *device_to_host = io_d2h_;
    if (reset) io_h2d_ = io_d2h_ = 0;
  }
  // the engine stream goes on once the caller's stream has reached this point / the caller's stream once the engine stream has
  void engine_after_caller() {
    if (!ev_io_in_) set_caller_stream((void*)caller_);
    SIPX_HIP(hipEventRecord(ev_io_in_, caller_));
    SIPX_HIP(hipStreamWaitEvent(stream_, ev_io_in_, 0));
  }
  void caller_after_engine() {
    SIPX_HIP(hipEventRecord(ev_io_out_, stream_));
    SIPX_HIP(hipStreamWaitEvent(caller_, ev_io_out_, 0));
  }
  void io_add(IoArgs<T>& A, bool pack, int dir, long long nrows, const T* rows, const T* pad) {
    if (nrows <= 0) return;
    if (A.nseg == IO_MAXSEG) {           // (more than 32 operator blocks in one call: another launch)
      io_rows<T>(stream_, A, pack, NB);
      A.nseg = 0;
    }
    io_seg_shape<T>(A.seg[A.nseg++], G_, dir, nrows, rows, pad);
  }
  void io_add_set(IoArgs<T>& A, bool pack, const SetState<T>& s, const T* rows, const T* dev) {
    if (s.ident || s.custom) { io_add(A, pack, -1, s.Mtrue, rows, dev); return; }
    long long r0 = 0;
    for (int q = 0; q < s.nblk; ++q) {
      io_add(A, pack, s.dir[q], s.blk_rows[q], rows + r0, dev + (long long)q * G_.N);
      r0 += s.blk_rows[q];
    }
  }
  // m, and the warm start where there is one, from the caller's buffers into the (zero-filled) arrays of the context
  void import_dev(const void* m, const void* x0, const void* const* l0, const void* const* y0) {
    engine_after_caller();
    IoArgs<T> A;
    io_add(A, false, -1, G_.N, (const T*)m, m_);
    if (x0) io_add(A, false, -1, Nx_, (const T*)x0, x_);
    for (int i = 0; i < p_n_; ++i) {
      const SetState<T>& s = sets_[i];
      if (l0 && l0[i]) io_add_set(A, false, s, (const T*)l0[i], s.l);
      if (y0 && y0[i]) io_add_set(A, false, s, (const T*)y0[i], s.y);
    }
    io_rows<T>(stream_, A, false, NB);
  }
  void finalize_dev(const void* m, const double* rho_ini, int n_rho, double gamma_ini, int feasibility_only, int zero_ini_guess,
                    const void* x0, const void* const* l0, const void* const* y0, double* feasibility_initial) override {
    need_dev_io("sipx_finalize_dev");
    if (!m) throw std::runtime_error("sipx_finalize_dev: m is a null pointer");
    DevIoGuard g(&dev_io_);
    finalize(m, rho_ini, n_rho, gamma_ini, feasibility_only, zero_ini_guess, x0, l0, y0, feasibility_initial);
  }
  void reset_dev(const void* m, const double* rho_ini, int n_rho, double gamma_ini, int zero_ini_guess, const void* x0,
                 const void* const* l0, const void* const* y0, double* feasibility_initial) override {
    need_final();
    need_dev_io("sipx_reset_dev");
    if (!m) throw std::runtime_error("sipx_reset_dev: m is a null pointer");       // (before anything of the context is zeroed)
    DevIoGuard g(&dev_io_);
    reset(m, rho_ini, n_rho, gamma_ini, zero_ini_guess, x0, l0, y0, feasibility_initial);
  }
  void download_dev(void* x, void* const* l, void* const* y) override {
    need_final();
    need_dev_io("sipx_download_dev");
    SIPX_HIP(hipSetDevice(device_));
    engine_after_caller();                // (whatever the caller's stream still does with the result buffers comes first)
    IoArgs<T> A;
    if (x) io_add(A, true, -1, Nx_, (const T*)x, x_);
    for (int i = 0; i < p_n_; ++i) {
      const SetState<T>& s = sets_[i];
      if (l && l[i]) io_add_set(A, true, s, (const T*)l[i], s.l);
      if (y && y[i]) io_add_set(A, true, s, (const T*)y[i], s.y);
    }
    io_rows<T>(stream_, A, true, NB);
    caller_after_engine();
  }

  // ------------------------------------------------------------------------------------------
  // sipx_set_data / sipx_set_data_dev: new vectors for a set that carries some -- element-wise or per-fiber bounds, the relaxed
  // histogram -- in a context that stays alive.  The reference's application examples replace one projector of a list between
  // images, P_sub[end] = x -> project_bounds!(x, LBD, UBD) (examples/Indonesia_desaturation/
  // image_desaturation_by_constraint_learning.jl:264); here that is one launch of the transfer kernel into the arrays the set
  // already has.  Before sipx_finalize the call replaces what sipx_add_set was given.  On a finalized context nothing is
  // allocated and no stream or event is created; the new data holds from the next sipx_reset on (a solve in progress is given
  // up: the host form stages through the engine's scratch).
  // segments that take a bound vector as given (src: device memory) into the padded array of the set
  void io_add_bounds(IoArgs<T>& A, const SetState<T>& s, const T* src, T* dev) {
    if (s.bmode != SIPX_MODE_FIBER) { io_add_set(A, false, s, src, dev); return; }
    if (A.nseg == IO_MAXSEG) {
      io_rows<T>(stream_, A, false, NB);
      A.nseg = 0;
    }
    io_seg_bcast<T>(A.seg[A.nseg++], G_, s.nblk == 1 ? s.dir[0] : -1, s.bdir, s.Mtrue, src, dev);      // (one block: configure_proj)
  }
  void set_data(int set, const void* lb, const void* ub, bool on_device) override {
    const std::string what = on_device ? "sipx_set_data_dev" : "sipx_set_data";
    const char* way_out = ": build a new context for that";
    if (comm_ || slab_req_ || !owned_.empty())
      throw std::runtime_error(what + " takes single-process contexts only, this one is sharded or slab-decomposed" + way_out);
    const int nsets = finalized_ ? pp_n_ : (int)sets_.size();
    if (set == nsets && !(finalized_ && feasibility_only_))
      throw std::runtime_error(what + ": index " + std::to_string(set) + " is the distance term, which holds no vectors (its data is m: sipx_reset)");
    if (set < 0 || set >= nsets)
      throw std::runtime_error(what + ": set index " + std::to_string(set) + " out of range (" + std::to_string(nsets) + " sets)");
    SetState<T>& s = sets_[set];
    if (s.comp) throw std::runtime_error(what + " is not available for Minkowski sets" + way_out);
    if (s.ext_kind == EXT_CARD_GROUPS) throw std::runtime_error(what + ": " + CARDG_NO_SET_DATA);
    if (s.ext_kind == EXT_L20 || s.ext_kind == EXT_L20_JOINT || (s.ext_kind == EXT_L20_SEG && !s.seg_radii))
      throw std::runtime_error(what + ": " + L20_NO_SET_DATA);
    if (s.ext_kind == EXT_L20_SEG && lb) throw std::runtime_error(what + ": " + L20_SET_DATA_UB);
    if (is_l2inf(s.ext_kind) && lb) throw std::runtime_error(what + ": " + L2INF_NO_WEIGHTS);
    if (is_l2inf(s.ext_kind) && !s.seg_radii) throw std::runtime_error(what + ": " + L2INF_NO_SET_DATA);
    const bool bounds = !s.ext_kind && s.prox == SIPX_PROJ_BOUNDS_VEC, hist = s.ext_kind == EXT_HISTOGRAM || s.seg_radii || s.weighted;
    if (!bounds && !hist)
      throw std::runtime_error(what + ": set " + std::to_string(set) + " holds no replaceable vectors -- element-wise and per-fiber bounds "
                               "(no transform), the relaxed histogram and per-fiber / per-slice l1, l2 and annulus sets built with a "
                               "vector of radii do, and the l2,1 sets built with weights; scalars, vector bounds behind the DCT, the DFT mask and "
                               "subspace bases are fixed at sipx_add_set" + way_out);
    if (s.seg_radii && lb && s.ext_kind != EXT_ANNULUS_SEG)
      throw std::runtime_error(what + ": only the annulus has inner radii (lb); the radii of an l1 / l2 set are its ub");
    if (s.ext_kind == EXT_L1_WEIGHTED && ub) throw std::runtime_error(what + ": " + L1W_SET_DATA_UB);
    if (s.weighted && ub)
      throw std::runtime_error(what + ": the weights of an l2,1 set are its lb; it has no ub (the radius is fixed at sipx_add_set)");
    const ConfigCtx ctx = config_ctx();
    const long long len = data_len(ctx, s);
    if (s.ext_kind == EXT_L1_WEIGHTED && lb && !on_device) check_l1w_weights((const T*)lb, len);
    else if (s.weighted && lb && !on_device) check_l21_weights((const T*)lb, len, s.ext_kind == EXT_L21_JOINT ? "l21_joint" : (s.ext_kind == EXT_L21_GROUPS ? "l21_groups" : "l21"));
    if (s.seg_radii && (s.ext_kind == EXT_L1_SEG || s.ext_kind == EXT_L21_SEG) && ub && !on_device) check_l1_radii((const T*)ub, len);
    if (s.ext_kind == EXT_L20_SEG && ub && !on_device) l20_check_k_vector<T>((const T*)ub, len, G_.n[0] * G_.n[1]);
    if (is_l2inf(s.ext_kind) && ub && !on_device) {
      const long long per = s.ext_kind == EXT_L2INF && s.op == SIPX_OP_TV_XY ? G_.st[2] : len;
      l2inf_check_vector<T>((const T*)ub, len, [&](long long p) { return s.ext_kind == EXT_L2INF_STACKED || p % per != per - 1; });
    }
    if (bounds && s.bmode == SIPX_MODE_FIBER && s.custom)
      throw std::runtime_error(what + ": per-fiber bounds need one of the built-in operators" + way_out);
    if (!lb && !ub) return;
    SIPX_HIP(hipSetDevice(device_));
    const T *LB = (const T*)lb, *UB = (const T*)ub;
    const size_t bytes = (size_t)len * sizeof(T);
    if (!finalized_) {
      if (on_device) {                       // kept as given until sipx_finalize expands it; the caller may reuse its buffers
        engine_after_caller();
        if (LB && !s.pend_lb) s.pend_lb = mem_.alloc<T>((size_t)len, Mem::NoFill);
        if (UB && !s.pend_ub) s.pend_ub = mem_.alloc<T>((size_t)len, Mem::NoFill);
        if (LB) SIPX_HIP(hipMemcpyAsync(s.pend_lb, LB, bytes, hipMemcpyDeviceToDevice, stream_));
        if (UB) SIPX_HIP(hipMemcpyAsync(s.pend_ub, UB, bytes, hipMemcpyDeviceToDevice, stream_));
        caller_after_engine();
        return;
      }
      auto take = [&](const T* src, std::vector<T>& host, T*& pend) {      // (uploaded, and counted, by sipx_finalize)
        if (!src) return;
        mem_.release(pend);
        pend = nullptr;
        if (bounds && s.bmode == SIPX_MODE_FIBER) expand_fiber_bounds(ctx, s, src, host);
        else host.assign(src, src + len);
      };
      take(LB, s.host_lb, s.pend_lb);
      take(UB, s.host_ub, s.pend_ub);
      return;
    }
    if (on_device) {
      // the engine stream behind the caller's and behind the set streams, which may still read the old vectors
      engine_after_caller();
      for (auto& o : sets_)
        if (o.st && o.st != stream_ && o.ev) {
          SIPX_HIP(hipEventRecord(o.ev, o.st));
          SIPX_HIP(hipStreamWaitEvent(stream_, o.ev, 0));
        }
    } else {
      if (lane_thr_.joinable()) lane_thr_.join();
      SIPX_HIP(hipStreamSynchronize(stream_));
      for (hipStream_t q : pool_) if (q && q != stream_) SIPX_HIP(hipStreamSynchronize(q));
      if (lane_st_) SIPX_HIP(hipStreamSynchronize(lane_st_));
      io_h2d_ += (long long)bytes * ((LB ? 1 : 0) + (UB ? 1 : 0));
    }
    if (hist) {
      if (!s.ext) throw std::runtime_error("internal: histogram / segment-radii set without its projector");
      s.ext->set_stream(stream_);
      s.ext->set_data(LB, UB, on_device);
    } else {
      if (!on_device) {                      // one copy each into the engine's scratch, idle between solves
        if (LB) { SIPX_HIP(hipMemcpyAsync(scr_v_, LB, bytes, hipMemcpyHostToDevice, stream_)); LB = scr_v_; }
        if (UB) { SIPX_HIP(hipMemcpyAsync(scr_c_, UB, bytes, hipMemcpyHostToDevice, stream_)); UB = scr_c_; }
      }
      IoArgs<T> A;
      if (LB) io_add_bounds(A, s, LB, s.lb);
      if (UB) io_add_bounds(A, s, UB, s.ub);
      io_rows<T>(stream_, A, false, NB);
    }
    if (on_device) caller_after_engine();
    else SIPX_HIP(hipStreamSynchronize(stream_));      // (the caller's arrays have been read)
  }

  // ------------------------------------------------------------------------------------------
  // Whole solve: src/PARSDMM.jl:63-257 restated (serial path).  begin / step so a caller can advance the
  // solve iteration by iteration (bench warm-up + timed steps); sipx_parsdmm = begin + steps until done.
  void parsdmm_begin(const sipx_options* opt, sipx_log* log) override {
    need_final();
    for (auto& s : sets_)
      if (!s.owned && !comm_) throw std::runtime_error("sipx_parsdmm needs every set local, or a communicator (sipx_set_comm*)");
    Run& R = run_;
    R = Run();
    head_done_ = false;
    marks_.begin_solve(opt->maxit);
    R.log = log;
    R.maxit = opt->maxit;
    const int p = p_n_, pp = pp_n_;
    R.tol.evol_rel = (T)opt->evol_rel_tol; R.tol.feas = (T)opt->feas_tol; R.tol.obj = (T)opt->obj_tol;   // convert_options!
    R.sw.adjust_rho = opt->adjust_rho; R.sw.adjust_gamma = opt->adjust_gamma; R.sw.adjust_feas_rho = opt->adjust_feasibility_rho;
    R.sw.freq = opt->rho_update_frequency;
    if (any_ncvx_) { R.sw.freq = 3; R.sw.adjust_gamma = false; }      // PARSDMM_initialize.jl:107-114
    R.sw.ind_ref = R.maxit;
    std::fill(log->timing_ms, log->timing_ms + 7, 0.0);
    log->stopped_feasible = 0;
    for (int i = 0; i < pp; ++i) log->set_feasibility[i] = feas_init_[i];   // :236
    R.active = true;
    if (pp > 0 && julia_maximum(feas_init_.begin(), feas_init_.end()) < (double)R.tol.feas) {     // :101-104
      already_feasible();
      return;
    }
    R.counter = 2;
    R.tol_ref = 1.0;
    R.rho.resize(p); R.gamma.resize(p); R.rho_new.resize(p); R.rpri.resize(p); R.rdual.resize(p);
    R.feas.resize(std::max(pp, 1));
    for (int i = 0; i < p; ++i) { R.rho[i] = (double)rho_[i]; R.gamma[i] = (double)gamma_[i]; }
    log->n_iter = R.maxit;
    log->n_feas_rows = R.counter;
    if (R.maxit < 1) R.done = true;
  }
  // m lies in every set already: x = m, no iteration (PARSDMM.jl:63-82)
  void already_feasible() {
    sipx_log* log = run_.log;
    {
      const long long c0 = slab_local_ ? std::max<long long>(0, wlo_) : 0, c1 = slab_local_ ? std::min<long long>(G_.N, whi_) : G_.N;
      if (c1 > c0) SIPX_HIP(hipMemcpyAsync(x_ + c0, m_ + c0, (c1 - c0) * sizeof(T), hipMemcpyDeviceToDevice, stream_));
    }
    if (mk_) SIPX_HIP(hipMemsetAsync(x_ + G_.N, 0, G_.N * sizeof(T), stream_));      // x = [m; 0]  PARSDMM.jl:64-69
    SIPX_HIP(hipStreamSynchronize(stream_));
    log->n_iter = 1;
    log->n_feas_rows = 1;
    log->stopped_feasible = 1;
    run_.done = true;
  }

  // One iteration, PARSDMM.jl:97-254, as a software pipeline: nothing the GPU is given next may depend on the sums the host is
  // about to read, so the right-hand side and the residual product of iteration i + 1 are queued (queue_ahead) before the
  // host collects the sums of iteration i and runs the rules on them.
  bool parsdmm_step() override {
    Run& R = run_;
    if (!R.active) throw std::runtime_error("sipx_parsdmm_steps: call sipx_parsdmm_begin first");
    if (R.done) return true;
    ObserverGuard og(observer());
    const int i = ++R.i;
    begin_step(i);
    x_step(i);
    const YlPlan plan = yl_step(i);
    queue_ahead(i, plan);
    collect_set_sums(plan.route, R.rho.data(), R.rpri.data(), R.rdual.data(), R.feas.data());
    record_log_row(i);
    if (stop_rule(i)) {
      finish_solve(i);
      return true;
    }
    next_rho(i);
    apply_rho(i);
    if (i == R.maxit) finish_solve(i);
    return R.done;
  }

  // the marks of step i - 2 (same parity) have long completed: into log.timing; then this step's parity, marks and weight
  void begin_step(int i) {
    marks_.resolve(run_.log, i & 1);
    marks_.begin_step(i);
  }

  // rhs_i unless it was queued ahead, then x_i (PARSDMM.jl:101-107)
  void x_step(int i) {
    Run& R = run_;
    // (the x-step's section opens where its residual product is queued: here, or in the step before when that was queued ahead)
    if (!head_done_) marks_.open(i);
    if (!R.rhs_ready) {
      rhs_compose(R.rho.data());
      marks_.mark(1);
    }
    R.rhs_ready = false;
    int64_t cg_it; double relres; int flag;
    argmin_x(i, &R.tol_ref, &cg_it, &relres, &flag);
    R.log->cg_it[i - 1] = cg_it;
    R.log->cg_relres[i - 1] = relres;
    marks_.mark(2);
  }

  // y_i, l_i and the reduction of their sums, queued; the sums are collected further down (PARSDMM.jl:133).  Decides the plan:
  // can the rules at the end of this iteration change rho?  If not, the right-hand side of iteration i + 1 is known as soon as
  // the y/l kernels are queued, and the sweep that forms y, l may write it.
  YlPlan yl_step(int i) {
    Run& R = run_;
    YlPlan plan;
    plan.collect_now = false;
    plan.fuse_rhs = i < R.maxit && !rho_may_change<T>(R.sw, i, pp_n_, R.rho.data(), p_n_);
    if (comm_) plan.route = plan.fuse_rhs ? YlPlan::Route::WithNextHead : YlPlan::Route::ByEvent;
    else plan.route = marks_.stride > 1 ? YlPlan::Route::ByWord : YlPlan::Route::ByEvent;
    yl_update(i, yl_flags(R.sw, i), R.rho.data(), R.gamma.data(), plan);
    marks_.mark(3);                        // also the event the host waits on for the sums (unless they come with the pinned word)
    if (plan.route != YlPlan::Route::ByWord) sums_event_here();
    return plan;
  }
  // the sums of the y/l update are complete behind the step's latest mark -- or, on a step without marks, behind ev_sums_, recorded here
  void sums_event_here() {
    sums_event_ = marks_.last_event();
    if (sums_event_) return;
    SIPX_HIP(hipEventRecord(ev_sums_, stream_));
    sums_event_ = ev_sums_;
  }

  // Software pipeline: when the rules cannot touch rho, rhs_{i+1} = sum_i A_i'(rho_i y_i + l_i) (and, sharded, its
  // reduce-scatter on the communication stream) is queued now and runs while the host waits for the sums and evaluates the
  // stop rule -- and so is the residual product of the coming x-step.  A stop leaves x, y, l as they are: rhs is scratch.
  void queue_ahead(int i, const YlPlan& plan) {
    Run& R = run_;
    if (rhs_fused_) {
      R.rhs_ready = true;                  // written by the y/l sweep itself (kernels_multi.hip)
    } else if (plan.fuse_rhs) {
      rhs_compose(R.rho.data());
      marks_.mark(1);
      R.rhs_ready = true;
    }
    // (round 3 had the product store x_old <- x, which a context without a distance term -- feasibility only -- still had to read
    //  for evol_x after this point: its logged evol_x was zero.  The product no longer touches x_old: x_k stays behind in its own
    //  ring buffer when the x-step moves on, tests/test_gpu_round4.py::test_feasibility_only_logs_evol_x...)
    if (!R.rhs_ready) return;
    marks_.open(i + 1);                    // (if the coming step is a timed one: its x-step section opens here)
    argmin_x_head();
    if (comm_) {                           // (sharded: the sums arrive with the grouped call of the head)
      marks_.mark(-1);                     // (an opening mark: the head's time belongs to the coming step's x-step section, which opened in front of it)
      sums_event_here();
    }
  }

  // row i of the log: residuals, rho, gamma, obj, evol_x; every tenth iteration a row of set_feasibility (PARSDMM.jl:134-147)
  void record_log_row(int i) {
    Run& R = run_;
    sipx_log* log = R.log;
    const int p = p_n_, pp = pp_n_;
    HostSection t(log->timing_ms[3]);      // bookkeeping of the y/l section
    for (int k = 0; k < p; ++k) {
      log->r_pri[(size_t)(i - 1) * p + k] = R.rpri[k];
      log->r_dual[(size_t)(i - 1) * p + k] = R.rdual[k];
      log->rho[(size_t)(i - 1) * p + k] = R.rho[k];
      log->gamma[(size_t)(i - 1) * p + k] = R.gamma[k];
    }
    log->r_dual_total[i - 1] = seq_sum<T>(R.rdual.data(), p);        // PARSDMM.jl:134
    log->r_pri_total[i - 1] = seq_sum<T>(R.rpri.data(), p);          // :138
    if (feas_due(i)) {                                               // update_y_l.jl:90-105
      for (int k = 0; k < pp; ++k) log->set_feasibility[(size_t)(R.counter - 1) * pp + k] = R.feas[k];
      R.counter += 1;
    }
    log_scalars(&log->obj[i - 1], &log->evol_x[i - 1]);
  }

  // stop_PARSDMM.jl:23-52 on the log so far; may switch the adjust_* rules off for the rest of the solve
  bool stop_rule(int i) {
    Run& R = run_;
    HostSection t(R.log->timing_ms[4]);
    const LogView view{R.log->set_feasibility, R.log->obj, R.log->evol_x, R.log->r_pri_total};
    return sipx::stop_rule<T>(view, i, R.counter, pp_n_, R.tol, R.sw);
  }

  // adjust rho and gamma (PARSDMM.jl:163-227) into rho_new; l_hat / snapshots were fused into update_y_l
  void next_rho(int i) {
    Run& R = run_;
    HostSection t(R.log->timing_ms[5]);
    R.rho_new = R.rho;
    if (bb_due(R.sw, i)) adapt_rho_gamma(R.sw.adjust_rho, R.sw.adjust_gamma, R.rho_new.data(), R.gamma.data());
    const double* latest = R.log->set_feasibility + (size_t)(R.counter - 2) * pp_n_;
    sipx::next_rho<T>(R.sw, i, pp_n_, latest, R.rho_new.data(), p_n_);
  }

  // rho_new takes effect: the right-hand side of the coming iteration if it is not queued yet, then the Q update (:230-243)
  void apply_rho(int i) {
    Run& R = run_;
    if (R.rhs_ready && R.rho_new != R.rho) throw std::runtime_error("internal: rho changed under a right-hand side queued ahead");
    bool changed = false;
    for (int k = 0; k < p_n_; ++k) changed |= R.rho_new[k] != R.rho[k];
    const bool rhs_due = i < R.maxit && !R.rhs_ready;
    if (rhs_due || changed) marks_.mark(-1);     // the stream sat idle while the host decided
    if (rhs_due) {                         // rho is final now; queued ahead of the Q update so that, sharded, the
      rhs_compose(R.rho_new.data());       // reduce-scatter (communication stream) runs beside it
      marks_.mark(1);
      R.rhs_ready = true;
    }
    if (changed) {
      q_update(R.rho_new.data(), R.rho.data());
      marks_.mark(6);
    }
    R.rho = R.rho_new;
  }

  // common exit of the whole solve (stop rule or maxit): timing resolved, logs truncated, and the context left so that a
  // later solve on it continues from here -- Q holds sum_i rho_i AtA_i for exactly these rho
  void finish_solve(int n_iter) {
    Run& R = run_;
    if (rs_pending_) {                      // a right-hand side queued ahead: let its exchange finish before anyone touches rhs
      SIPX_HIP(hipStreamWaitEvent(stream_, ev_c_[1], 0));
      rs_pending_ = false;
    }
    marks_.resolve(R.log, 0);
    marks_.resolve(R.log, 1);
    R.log->n_iter = n_iter;
    R.log->n_feas_rows = R.counter;
    for (int k = 0; k < p_n_; ++k) { rho_[k] = (T)R.rho[k]; gamma_[k] = (T)R.gamma[k]; }
    R.rhs_ready = false;
    R.done = true;
    head_done_ = false;
  }

  void parsdmm(const sipx_options* opt, sipx_log* log) override {
    parsdmm_begin(opt, log);
    while (!parsdmm_step()) {
    }
  }

  // ------------------------------------------------------------------------------------------
  // The stand-alone calls (sipx_apply_op, sipx_project, sipx_l21_norms, sipx_segment_norms) configure a throw-away set like
  // sipx_add_set does and work in scratch of the call.  What they share:
  // x behind the halo the difference kernels read across (dx) and the padded blocks of A x (dv), each only where wanted
  struct OpScratch {
    T *dx = nullptr, *dv = nullptr;
    OpScratch(DeviceMemory& tmp, const Grid& G, long long Mpad, bool want_x, bool want_v) {
      long long H = 4;
      for (int a = 0; a < 3; ++a) H = std::max<long long>(H, G.st[a]);
      H = (H + 3) / 4 * 4;
      if (want_x) dx = tmp.alloc<T>(G.N + 2 * H) + H;
      if (want_v) dv = tmp.alloc<T>(Mpad + H) + H;
    }
  };
  // ... for A x of host or device x: device x of the identity is read where it lies
  OpScratch forward_scratch(DeviceMemory& tmp, const SetConfig<T>& s, bool on_device) const {
    return OpScratch(tmp, G_, s.Mpad, !(on_device && !s.nblk), s.nblk > 0);
  }
  // A x (x itself for the identity) queued on the engine stream, behind the caller's stream for device x
  const T* queue_forward(const OpScratch& w, const SetConfig<T>& s, const void* x, bool on_device) {
    if (on_device) engine_after_caller();
    if (w.dx) SIPX_HIP(hipMemcpyAsync(w.dx, x, G_.N * sizeof(T), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream_));
    const T* dx = w.dx ? w.dx : (const T*)x;
    if (s.nblk) K<T>::fwd(stream_, G_, s.nblk, s.dir, s.ih, dx, w.dv);
    return s.nblk ? w.dv : dx;
  }
  // the scratch of a threshold search over n entries (ps: where the engine's own two-pass search runs)
  struct SearchScratch {
    T *dc = nullptr, *mp = nullptr;
    double* part = nullptr;
    ProjScalars<T>* ps = nullptr;
    SearchScratch(DeviceMemory& tmp, long long n, bool with_ps) {
      dc = tmp.alloc<T>(n);
      part = tmp.alloc<double>((size_t)(PREP_SLOTS + 2) * NB);
      mp = tmp.alloc<T>(2 * NB);
      if (with_ps) ps = tmp.alloc<ProjScalars<T>>(1);
    }
  };
  // the result of a call: left in the caller's device memory behind the caller's stream, or copied to the host
  void finish_call(bool on_device, void* out, const T* dout, long long n) {
    if (on_device) {
      caller_after_engine();
      SIPX_HIP(hipStreamSynchronize(stream_));      // (the scratch of this call goes when it returns)
    } else {
      SIPX_HIP(hipStreamSynchronize(stream_));
      SIPX_HIP(hipMemcpy(out, dout, n * sizeof(T), hipMemcpyDeviceToHost));
    }
  }

  void apply_op(int op, const void* x, void* out, bool adjoint) override {
    SIPX_HIP(hipSetDevice(device_));
    SetConfig<T> s;
    configure_op(config_ctx(), s, op);
    DeviceMemory tmp;
    const OpScratch w(tmp, G_, s.Mpad, true, true);
    if (!adjoint) {
      SIPX_HIP(hipMemcpy(w.dx, x, G_.N * sizeof(T), hipMemcpyHostToDevice));
      K<T>::fwd(stream_, G_, s.nblk, s.dir, s.ih, w.dx, w.dv);
      download_rows(s, w.dv, (T*)out);
    } else {
      upload_rows(s, (const T*)x, w.dv);
      K<T>::adj(stream_, G_, s.nblk, s.dir, s.ih, w.dv, w.dx);
      finish_call(false, out, w.dx, G_.N);
    }
  }

  // SIPX_PROJ_L21 of sipx_project: the M-vector of the TV range in the reference's row order, through the packing of a TV set's y / l;
  // SIPX_PROJ_L21_GROUPS alike on the range of its one-block operator
  void project_l21(const sipx_set_desc* d, void* v, int64_t len) {
    SetConfig<T> st;
    const bool groups = d->proj == SIPX_PROJ_L21_GROUPS;
    if (d->proj == SIPX_PROJ_L21_JOINT && d->op != SIPX_OP_TV_XY)
      throw std::runtime_error(L21_JOINT_ROUTE);
    if (d->proj == SIPX_PROJ_TNV && d->op != SIPX_OP_TV_XY) throw std::runtime_error(TNV_ROUTE);
    if (groups && d->op != SIPX_OP_IDENTITY && d->op != SIPX_OP_DX && d->op != SIPX_OP_DY && d->op != SIPX_OP_DZ)
      throw std::runtime_error(L21G_ONE_BLOCK);
    if (!groups && d->op != SIPX_OP_TV && d->op != SIPX_OP_TV_XY)
      throw std::runtime_error("the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)");
    const ConfigCtx ctx = config_ctx();
    configure_op(ctx, st, d->op);
    configure_proj(ctx, st, d);
    if (len != st.Mtrue)
      throw std::runtime_error(std::string("the l2,1 ball projects a vector of the ") +
                               (groups ? "operator's" : (d->op == SIPX_OP_TV ? "TV" : "TV_xy")) + " range: " +
                               std::to_string(st.Mtrue) + " entries on this grid, " + std::to_string((long long)len) + " given");
    st.spec.ub = st.host_ub.empty() ? nullptr : st.host_ub.data();      // (per frame: one radius each)
    st.spec.lb = st.weighted ? st.host_lb.data() : nullptr;             // (weighted: one weight per group)
    DeviceMemory tmp;
    T* dv = tmp.alloc<T>(st.Mpad);               // (zeroed: the rows a block does not have)
    const SearchScratch q(tmp, G_.N, false);
    upload_rows(st, (const T*)v, dv);
    {
      ExtProj<T> ext(st.spec, stream_);
      ext.project(dv, false, q.part, q.mp, q.dc);
      download_rows(st, dv, (T*)v);               // (synchronises the stream)
    }
  }

  // sipx_l21_norm(s)(_dev), sipx_l21_joint_norm(_dev): what the (proj, op, mode) set compares with its radius on A x -- ||TV x||_2,1 or
  // its TV_xy form, the n3 per-frame sums of TV_xy with (slice, z), the sum over the pixels of the joint set or of the singular values of
  // SIPX_PROJ_TNV (sipx_tnv_norm) -- by the observe() of a
  // throw-away projector of that set (ext_group.hip): the launches and the sums of its project()
  void l21_norms(int proj, int op, int mode, int dir, const void* x, void* out, int64_t* nseg, bool on_device, bool query) override {
    auto need_x_out = [&] { if (!x || !out) throw std::runtime_error("l2,1 norm: x and out are needed"); };
    if (proj == SIPX_PROJ_L21 && !query) need_x_out();    // (sipx_l21_norm refuses a null pointer before the context is looked at)
    SIPX_HIP(hipSetDevice(device_));
    if (proj == SIPX_PROJ_TNV && op != SIPX_OP_TV_XY) throw std::runtime_error(TNV_ROUTE);
    if (op != SIPX_OP_TV && op != SIPX_OP_TV_XY)
      throw std::runtime_error("the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)");
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> s;
    configure_op(ctx, s, op);
    if (op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
    sipx_set_desc d{};
    d.op = op; d.proj = proj; d.mode = mode; d.dir = dir; d.pmax = 1.0;
    configure_proj(ctx, s, &d);                // the refusals, and the ExtSpec, of the set
    const long long nout = s.ext_kind == EXT_L21_SEG ? G_.n[2] : 1;
    if (nseg) *nseg = nout;
    if (query && !x && !out) return;           // (sipx_l21_norms: a query of the length)
    need_x_out();
    DeviceMemory tmp;
    const OpScratch w = forward_scratch(tmp, s, on_device);
    const SearchScratch q(tmp, s.ext_kind == EXT_L21_JOINT ? G_.st[2] : G_.N, false);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(nout);
    ExtProj<T> ext(s.spec, stream_);
    const T* dv = queue_forward(w, s, x, on_device);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, (double)(s.nblk + 1) * G_.N * sizeof(T));
      ext.observe(dv, dout, q.part, q.mp, q.dc);
    }
    finish_call(on_device, out, dout, nout);
  }

  // sipx_l21_weighted_norm(_dev): (T) sum_p w_p g_p of the weighted (op, joint) set on A x, by the observe() of a throw-away projector
  // of that set: its norms launch and the first pass of its iteration (l21_weighted.h)
  void l21_weighted_norm(int op, bool joint, const void* x, const void* w, void* out, bool on_device) override {
    if (!x || !w || !out) throw std::runtime_error("weighted l2,1 norm: x, w and out are needed");
    SIPX_HIP(hipSetDevice(device_));
    if (joint && op != SIPX_OP_TV_XY) throw std::runtime_error(L21_JOINT_ROUTE);
    if (op != SIPX_OP_TV && op != SIPX_OP_TV_XY)
      throw std::runtime_error("the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)");
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> s;
    configure_op(ctx, s, op);
    if (op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
    sipx_set_desc d{};
    d.op = op; d.proj = joint ? SIPX_PROJ_L21_JOINT : SIPX_PROJ_L21; d.mode = SIPX_MODE_WHOLE; d.pmax = 1.0;
    configure_proj(ctx, s, &d);                // the refusals, and the ExtSpec, of the unweighted set
    const long long ng = l21_groups(ctx, s.ext_kind);
    if (!on_device) check_l21_weights((const T*)w, ng, joint ? "l21_joint" : "l21");
    s.spec.weighted = 1;
    s.spec.lb = on_device ? nullptr : w;
    DeviceMemory tmp;
    const OpScratch ws = forward_scratch(tmp, s, on_device);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(1);
    ExtProj<T> ext(s.spec, stream_);
    const T* dv = queue_forward(ws, s, x, on_device);     // (device x, w: the engine stream is behind the caller's from here on)
    if (on_device) ext.set_data((const T*)w, nullptr, true);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, (double)(s.nblk + 1) * G_.N * sizeof(T));
      ext.observe(dv, dout, nullptr, nullptr, nullptr);
    }
    finish_call(on_device, out, dout, 1);
  }

  // SIPX_PROJ_L1_WEIGHTED of sipx_project: the M-vector of the operator's range in the reference's row order, as project_l21 takes it
  void project_l1_weighted(const sipx_set_desc* d, void* v, int64_t len) {
    if (d->op == SIPX_OP_CSC) throw std::runtime_error(L1W_NO_CUSTOM);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> st;
    configure_op(ctx, st, d->op);
    if (st.op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
    configure_proj(ctx, st, d);
    if (!d->lb) throw std::runtime_error(L1W_NEEDS_WEIGHTS);
    if (len != st.Mtrue)
      throw std::runtime_error("the weighted l1 ball projects a vector of the operator's range: " + std::to_string(st.Mtrue) +
                               " entries on this grid, " + std::to_string((long long)len) + " given");
    st.spec.lb = st.host_lb.data();
    DeviceMemory tmp;
    T* dv = tmp.alloc<T>(st.Mpad);               // (zeroed: the rows a block does not have)
    upload_rows(st, (const T*)v, dv);
    {
      ExtProj<T> ext(st.spec, stream_);
      ext.project(dv, false, nullptr, nullptr, nullptr);
      download_rows(st, dv, (T*)v);               // (synchronises the stream)
    }
  }

  // SIPX_PROJ_SIMPLEX of sipx_project: the M-vector of the range of its one-block operator in the reference's row order
  void project_simplex(const sipx_set_desc* d, void* v, int64_t len) {
    if (d->op != SIPX_OP_IDENTITY && d->op != SIPX_OP_DX && d->op != SIPX_OP_DY && d->op != SIPX_OP_DZ) throw std::runtime_error(SIMPLEX_ONE_BLOCK);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> st;
    configure_op(ctx, st, d->op);
    configure_proj(ctx, st, d);
    if (len != st.Mtrue)
      throw std::runtime_error("the simplex set projects a vector of the operator's range: " + std::to_string(st.Mtrue) +
                               " entries on this grid, " + std::to_string((long long)len) + " given");
    DeviceMemory tmp;
    T* dv = tmp.alloc<T>(st.Mpad);               // (zeroed: the rows a block does not have)
    upload_rows(st, (const T*)v, dv);
    {
      ExtProj<T> ext(st.spec, stream_);
      ext.project(dv, false, nullptr, nullptr, nullptr);
      long long c[4];                            // the route of a stand-alone call counts like a set's (simplex row of sipx_kernel_stats)
      ext.route_counts(c);
      for (int q = 0; q < 3; ++q) project_sc_[q] += c[q];
      project_sc_[3] = c[3];
      download_rows(st, dv, (T*)v);               // (synchronises the stream)
    }
  }

  // sipx_segment_sums(_dev): (T) sum of the positive parts of every fiber / slice of A x, in the order of sipx_segment_norms, by the
  // observe() of a throw-away projector of the simplex set on (op, mode, dir): pass 1 of its own route (seg_simplex.h)
  void segment_sums(int op, int mode, int dir, const void* x, void* out, int64_t* nseg, bool on_device) override {
    SIPX_HIP(hipSetDevice(device_));
    if (op != SIPX_OP_IDENTITY && op != SIPX_OP_DX && op != SIPX_OP_DY && op != SIPX_OP_DZ) throw std::runtime_error(SIMPLEX_ONE_BLOCK);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> s;
    configure_op(ctx, s, op);
    sipx_set_desc d{};
    d.op = op; d.proj = SIPX_PROJ_SIMPLEX; d.mode = mode; d.dir = dir; d.pmin = 0.0; d.pmax = 1.0;
    configure_proj(ctx, s, &d);                // the refusals, and the ExtSpec, of the set
    const long long ns = seg_count(s.spec);
    if (nseg) *nseg = ns;
    if (!x || !out) return;                    // (a query of the length)
    DeviceMemory tmp;
    const OpScratch w = forward_scratch(tmp, s, on_device);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(ns);
    ExtProj<T> ext(s.spec, stream_);
    const T* dv = queue_forward(w, s, x, on_device);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, (double)s.Mtrue * sizeof(T));
      ext.observe(dv, dout, nullptr, nullptr, nullptr);
    }
    finish_call(on_device, out, dout, ns);
  }

  // SIPX_PROJ_CARD_GROUPS of sipx_project: the M-vector of the range of its one-block operator in the reference's row order
  void project_card_groups(const sipx_set_desc* d, void* v, int64_t len) {
    if (d->op != SIPX_OP_IDENTITY && d->op != SIPX_OP_DX && d->op != SIPX_OP_DY && d->op != SIPX_OP_DZ) throw std::runtime_error(CARDG_ONE_BLOCK);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> st;
    configure_op(ctx, st, d->op);
    configure_proj(ctx, st, d);
    if (len != st.Mtrue)
      throw std::runtime_error("group cardinality projects a vector of the operator's range: " + std::to_string(st.Mtrue) +
                               " entries on this grid, " + std::to_string((long long)len) + " given");
    DeviceMemory tmp;
    T* dv = tmp.alloc<T>(st.Mpad);               // (zeroed: the rows a block does not have)
    const SearchScratch q(tmp, seg_count(st.spec), false);
    upload_rows(st, (const T*)v, dv);
    {
      ExtProj<T> ext(st.spec, stream_);
      ext.project(dv, false, q.part, q.mp, q.dc);
      long long c[4];                            // the route of a stand-alone call counts like a set's (card_groups row of sipx_kernel_stats)
      ext.route_counts(c);
      for (int r = 0; r < 3; ++r) project_gc_[r] += c[r];
      project_gc_[3] = c[3];
      download_rows(st, dv, (T*)v);               // (synchronises the stream)
    }
  }

  // SIPX_PROJ_L20 / SIPX_PROJ_L20_JOINT of sipx_project: the M-vector of the TV / TV_xy range in the reference's row order
  void project_l20(const sipx_set_desc* d, void* v, int64_t len) {
    if (d->proj == SIPX_PROJ_L20_JOINT && d->op != SIPX_OP_TV_XY) throw std::runtime_error(L20_JOINT_ROUTE);
    if (d->op != SIPX_OP_TV && d->op != SIPX_OP_TV_XY) throw std::runtime_error(L20_NEEDS_TV);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> st;
    configure_op(ctx, st, d->op);
    if (d->op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
    configure_proj(ctx, st, d);
    if (len != st.Mtrue)
      throw std::runtime_error(std::string("the l2,0 set projects a vector of the ") + (d->op == SIPX_OP_TV ? "TV" : "TV_xy") + " range: " +
                               std::to_string(st.Mtrue) + " entries on this grid, " + std::to_string((long long)len) + " given");
    st.spec.ub = st.host_ub.empty() ? nullptr : st.host_ub.data();      // (per frame: one budget each)
    DeviceMemory tmp;
    T* dv = tmp.alloc<T>(st.Mpad);               // (zeroed: the rows a block does not have)
    const SearchScratch q(tmp, G_.N, false);
    upload_rows(st, (const T*)v, dv);
    {
      ExtProj<T> ext(st.spec, stream_);
      ext.project(dv, false, q.part, q.mp, q.dc);
      long long c[4];                            // the route of a stand-alone call counts like a set's (l20 row of sipx_kernel_stats)
      ext.route_counts(c);
      l20_count(st.ext_kind, c, project_l20c_);
      download_rows(st, dv, (T*)v);               // (synchronises the stream)
    }
  }
  // the l20 row of sipx_kernel_stats from a projector's route_counts: calls, small, search, frames, groups
  static void l20_count(int ext_kind, const long long c[4], long long row[5]) {
    row[0] += c[0];
    if (ext_kind == EXT_L20_SEG) row[3] += c[2];
    else { row[1] += c[1]; row[2] += c[2]; }
    row[4] = c[3];
  }

  // sipx_tv_group_norms(_dev): the norm of every gradient group of A x -- N entries in point order, joint: n1 n2 in pixel order -- by the
  // observe() of a throw-away projector of the l20 / l20_joint set on op: its own norms launch (l20.h)
  void tv_group_norms(int op, bool joint, const void* x, void* out, int64_t* ngroups, bool on_device) override {
    SIPX_HIP(hipSetDevice(device_));
    if (joint && op != SIPX_OP_TV_XY) throw std::runtime_error(L20_JOINT_ROUTE);
    if (op != SIPX_OP_TV && op != SIPX_OP_TV_XY) throw std::runtime_error(L20_NEEDS_TV);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> s;
    configure_op(ctx, s, op);
    if (op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
    sipx_set_desc d{};
    d.op = op; d.proj = joint ? SIPX_PROJ_L20_JOINT : SIPX_PROJ_L20; d.mode = SIPX_MODE_WHOLE; d.pmax = 1.0;
    configure_proj(ctx, s, &d);                // the refusals, and the ExtSpec, of the set
    const long long ng = joint ? G_.st[2] : G_.N;
    if (ngroups) *ngroups = ng;
    if (!x && !out) return;                    // (a query of the length)
    if (!x || !out) throw std::runtime_error("sipx_tv_group_norms: x and out are needed");
    DeviceMemory tmp;
    const OpScratch w = forward_scratch(tmp, s, on_device);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(ng);
    ExtProj<T> ext(s.spec, stream_);
    const T* dv = queue_forward(w, s, x, on_device);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, (double)(s.nblk + 1) * G_.N * sizeof(T));
      ext.observe(dv, dout, nullptr, nullptr, nullptr);
    }
    finish_call(on_device, out, dout, ng);
  }

  // sipx_group_norms(_dev): the l2 norm of every fiber / slice of A x, in the order of sipx_segment_norms, by the observe() of a throw-away
  // projector of the card_groups set on (op, mode, dir): its own norms launch (card_groups.h)
  void group_norms(int op, int mode, int dir, const void* x, void* out, int64_t* nseg, bool on_device) override {
    SIPX_HIP(hipSetDevice(device_));
    if (op != SIPX_OP_IDENTITY && op != SIPX_OP_DX && op != SIPX_OP_DY && op != SIPX_OP_DZ) throw std::runtime_error(CARDG_ONE_BLOCK);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> s;
    configure_op(ctx, s, op);
    sipx_set_desc d{};
    d.op = op; d.proj = SIPX_PROJ_CARD_GROUPS; d.mode = mode; d.dir = dir; d.pmax = 1.0;
    configure_proj(ctx, s, &d);                // the refusals, and the ExtSpec, of the set
    const long long ns = seg_count(s.spec);
    if (nseg) *nseg = ns;
    if (!x || !out) return;                    // (a query of the length)
    DeviceMemory tmp;
    const OpScratch w = forward_scratch(tmp, s, on_device);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(ns);
    ExtProj<T> ext(s.spec, stream_);
    const T* dv = queue_forward(w, s, x, on_device);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, (double)s.Mtrue * sizeof(T));
      ext.observe(dv, dout, nullptr, nullptr, nullptr);
    }
    finish_call(on_device, out, dout, ns);
  }

  // sipx_l1_weighted_norm(_dev): (T) sum_i w_i |(A x)_i| of the weighted l1 set behind op, by the observe() of a throw-away projector of
  // that set: the first pass of its iteration (l1_weighted.h)
  void l1_weighted_norm(int op, const void* x, const void* w, void* out, bool on_device) override {
    if (!x || !w || !out) throw std::runtime_error("weighted l1 norm: x, w and out are needed");
    SIPX_HIP(hipSetDevice(device_));
    if (op == SIPX_OP_CSC) throw std::runtime_error(L1W_NO_CUSTOM);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> s;
    configure_op(ctx, s, op);
    if (op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
    sipx_set_desc d{};
    d.op = op; d.proj = SIPX_PROJ_L1_WEIGHTED; d.mode = SIPX_MODE_WHOLE; d.pmax = 1.0;
    d.lb = on_device ? nullptr : w;            // (device weights: brought by set_data below, unchecked -- a bad one counts as 0)
    d.reserved = (int32_t)s.Mtrue;
    configure_proj(ctx, s, &d);                // the refusals, the check of host weights, and the ExtSpec
    s.spec.lb = on_device ? nullptr : s.host_lb.data();
    DeviceMemory tmp;
    const OpScratch ws = forward_scratch(tmp, s, on_device);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(1);
    ExtProj<T> ext(s.spec, stream_);
    const T* dv = queue_forward(ws, s, x, on_device);     // (device x, w: the engine stream is behind the caller's from here on)
    if (on_device) ext.set_data((const T*)w, nullptr, true);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, 2.0 * (double)s.Mpad * sizeof(T));
      ext.observe(dv, dout, nullptr, nullptr, nullptr);
    }
    finish_call(on_device, out, dout, 1);
  }

  // sipx_l21_groups_norm(_dev): (T) sum_s w_s g_s over the segments of the (op, mode, dir) set on A x (w NULL: every weight 1), by the
  // observe() of a throw-away projector of that set: its norms launch and the first pass of its iteration (l21_groups.h)
  void l21_groups_norm(int op, int mode, int dir, const void* x, const void* w, void* out, bool on_device) override {
    if (!x || !out) throw std::runtime_error("l2,1 norm over fibers or slices: x and out are needed");
    SIPX_HIP(hipSetDevice(device_));
    if (op != SIPX_OP_IDENTITY && op != SIPX_OP_DX && op != SIPX_OP_DY && op != SIPX_OP_DZ) throw std::runtime_error(L21G_ONE_BLOCK);
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> s;
    configure_op(ctx, s, op);
    sipx_set_desc d{};
    d.op = op; d.proj = SIPX_PROJ_L21_GROUPS; d.mode = mode; d.dir = dir; d.pmax = 1.0;
    configure_proj(ctx, s, &d);                // the refusals, and the ExtSpec, of the set without weights
    if (w && !on_device) check_l21_weights((const T*)w, seg_count(s.spec), "l21_groups");
    s.spec.weighted = w ? 1 : 0;
    s.spec.lb = on_device ? nullptr : w;
    DeviceMemory tmp;
    const OpScratch ws = forward_scratch(tmp, s, on_device);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(1);
    ExtProj<T> ext(s.spec, stream_);
    const T* dv = queue_forward(ws, s, x, on_device);     // (device x, w: the engine stream is behind the caller's from here on)
    if (on_device && w) ext.set_data((const T*)w, nullptr, true);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, (double)s.Mtrue * sizeof(T));
      ext.observe(dv, dout, nullptr, nullptr, nullptr);
    }
    finish_call(on_device, out, dout, 1);
  }

  // SIPX_PROJ_L21_STACKED of sipx_project: the M-vector itself, d->blocks blocks of len / blocks entries (l21_stacked.h); the operator of
  // the descriptor is not looked at
  void project_l21_stacked(const sipx_set_desc* d, void* v, int64_t len) {
    if (d->mode != SIPX_MODE_WHOLE) throw std::runtime_error(L21S_WHOLE_ONLY);
    if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(L21S_NO_TRANSFORM);
    if (d->component) throw std::runtime_error(L21S_NO_MINKOWSKI);
    if (d->lb || d->ub || d->reserved) throw std::runtime_error(L21S_NO_VECTORS);
    l21s_check_shape(len, d->blocks);
    refuse_sharded(config_ctx(), Sharded::L21_STACKED);
    if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    ExtSpec sp;
    l21s_spec(sp, len, d->blocks);
    sp.pmax = d->pmax;
    DeviceMemory tmp;
    T* dv = tmp.alloc<T>(len);
    const SearchScratch q(tmp, len / d->blocks, false);
    SIPX_HIP(hipMemcpy(dv, v, len * sizeof(T), hipMemcpyHostToDevice));
    {
      ExtProj<T> ext(sp, stream_);
      ext.project(dv, false, q.part, q.mp, q.dc);
      finish_call(false, v, dv, len);
    }
  }

  // the SIPX_PROJ_L2INF kinds of sipx_project (l2inf.h): the M-vector of the TV / TV_xy range in the reference's row order, or for the
  // stacked set the M-vector itself, d->blocks blocks of len / blocks entries (the operator of the descriptor is not looked at)
  void project_l2inf(const sipx_set_desc* d, void* v, int64_t len) {
    const ConfigCtx ctx = config_ctx();
    if (d->proj == SIPX_PROJ_L2INF_STACKED) {
      if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(L2INF_NO_TRANSFORM);
      if (d->component) throw std::runtime_error(L2INF_NO_MINKOWSKI);
      if (d->mode != SIPX_MODE_WHOLE) throw std::runtime_error(L2INF_MODES);
      if (d->pmin != 0) throw std::runtime_error(L2INF_MIN);
      if (d->lb) throw std::runtime_error(L2INF_NO_WEIGHTS);
      const long long G = l2infs_check_shape(len, d->blocks);
      refuse_sharded(ctx, Sharded::L2INF);
      if (d->ub) {
        if (d->reserved != G) throw std::runtime_error(l2inf_bad_length(d->reserved, G));
        l2inf_check_vector<T>((const T*)d->ub, G, [](long long) { return true; });
      } else {
        l2inf_check_c(d->pmax);
      }
      ExtSpec sp;
      l21s_spec(sp, len, d->blocks);
      sp.kind = EXT_L2INF_STACKED;
      sp.pmax = d->pmax;
      sp.ub = d->ub;
      DeviceMemory tmp;
      T* dv = tmp.alloc<T>(len);
      SIPX_HIP(hipMemcpy(dv, v, len * sizeof(T), hipMemcpyHostToDevice));
      {
        ExtProj<T> ext(sp, stream_);
        ext.project(dv, false, nullptr, nullptr, nullptr);
        finish_call(false, v, dv, len);
      }
      return;
    }
    if (d->proj == SIPX_PROJ_L2INF_JOINT && d->op != SIPX_OP_TV_XY) throw std::runtime_error(L2INF_JOINT_ROUTE);
    if (d->op != SIPX_OP_TV && d->op != SIPX_OP_TV_XY) throw std::runtime_error(L2INF_NEEDS_TV);
    SetConfig<T> st;
    configure_op(ctx, st, d->op);
    if (d->op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
    configure_proj(ctx, st, d);
    if (len != st.Mtrue)
      throw std::runtime_error(std::string("the l2,inf ball projects a vector of the ") + (d->op == SIPX_OP_TV ? "TV" : "TV_xy") + " range: " +
                               std::to_string(st.Mtrue) + " entries on this grid, " + std::to_string((long long)len) + " given");
    st.spec.ub = st.host_ub.empty() ? nullptr : st.host_ub.data();      // (one bound per group)
    DeviceMemory tmp;
    T* dv = tmp.alloc<T>(st.Mpad);               // (zeroed: the rows a block does not have)
    upload_rows(st, (const T*)v, dv);
    {
      ExtProj<T> ext(st.spec, stream_);
      ext.project(dv, false, nullptr, nullptr, nullptr);
      download_rows(st, dv, (T*)v);               // (synchronises the stream)
    }
  }

  // sipx_l2inf_norm(_dev): max_p g_p of A x for the SIPX_PROJ_L2INF kind the descriptor names, by the observe() of a throw-away projector
  // of that set (ext_group.hip, L2InfProj): the norms launch whose arithmetic its clip kernels repeat, and the two-stage maximum
  void l2inf_norm(const sipx_set_desc* d, const void* x, void* out, bool on_device) override {
    if (!d || !x || !out) throw std::runtime_error("l2,inf norm: the descriptor, x and out are needed");
    SIPX_HIP(hipSetDevice(device_));
    if (d->proj != SIPX_PROJ_L2INF && d->proj != SIPX_PROJ_L2INF_JOINT && d->proj != SIPX_PROJ_L2INF_STACKED)
      throw std::runtime_error("l2,inf norm: the descriptor's proj must be SIPX_PROJ_L2INF, SIPX_PROJ_L2INF_JOINT or SIPX_PROJ_L2INF_STACKED");
    const ConfigCtx ctx = config_ctx();
    sipx_set_desc dd = *d;
    dd.pmin = 0.0; dd.pmax = 1.0; dd.ncvx = 0; dd.lb = dd.ub = nullptr; dd.reserved = 0;
    DeviceMemory tmp;
    T* dout = on_device ? (T*)out : tmp.alloc<T>(1);
    if (d->proj == SIPX_PROJ_L2INF_STACKED) {
      if (d->op != SIPX_OP_CSC) throw std::runtime_error(L2INF_STACKED_NEEDS_CSC);
      SetState<T> s;
      configure_custom(ctx, s, d);
      configure_proj(ctx, s, &dd);               // the refusals, and the ExtSpec, of the set
      upload_custom(s, tmp);
      T* dx = on_device ? nullptr : tmp.alloc<T>(G_.N);
      ExtProj<T> ext(s.spec, stream_);
      if (on_device) engine_after_caller();
      else SIPX_HIP(hipMemcpyAsync(dx, x, G_.N * sizeof(T), hipMemcpyHostToDevice, stream_));
      custom_fwd(stream_, s, on_device ? (const T*)x : dx, s.sbuf);
      {
        ObserverGuard og(observer());
        ObsScope obs(KID_EXT, stream_, (double)(s.spec.nblk + 2) * s.spec.bstride * sizeof(T));
        ext.observe(s.sbuf, dout, nullptr, nullptr, nullptr);
      }
      finish_call(on_device, out, dout, 1);
      return;
    }
    if (d->proj == SIPX_PROJ_L2INF_JOINT && d->op != SIPX_OP_TV_XY) throw std::runtime_error(L2INF_JOINT_ROUTE);
    if (d->op != SIPX_OP_TV && d->op != SIPX_OP_TV_XY) throw std::runtime_error(L2INF_NEEDS_TV);
    SetConfig<T> s;
    configure_op(ctx, s, d->op);
    if (d->op == SIPX_OP_TV_XY) refuse_sharded(ctx, Sharded::TV_XY);
    configure_proj(ctx, s, &dd);                 // the refusals, and the ExtSpec, of the set
    const OpScratch w = forward_scratch(tmp, s, on_device);
    ExtProj<T> ext(s.spec, stream_);
    const T* dv = queue_forward(w, s, x, on_device);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, (double)(s.nblk + 2) * G_.N * sizeof(T));
      ext.observe(dv, dout, nullptr, nullptr, nullptr);
    }
    finish_call(on_device, out, dout, 1);
  }

  // sipx_l21_stacked_norm(_dev): what the SIPX_PROJ_L21_STACKED set of descriptor d compares with its radius on A x -- A x by custom_fwd
  // through a CSR copy in scratch of the call, then the observe() of a throw-away projector of that set (ext_group.hip, BallProj): the
  // norms launch and the first pass of the search of its project()
  void l21_stacked_norm(const sipx_set_desc* d, const void* x, void* out, bool on_device) override {
    if (!d || !x || !out) throw std::runtime_error("stacked l2,1 norm: the descriptor, x and out are needed");
    SIPX_HIP(hipSetDevice(device_));
    if (d->op != SIPX_OP_CSC) throw std::runtime_error(L21S_NEEDS_CSC);
    const ConfigCtx ctx = config_ctx();
    SetState<T> s;
    configure_custom(ctx, s, d);
    sipx_set_desc dd = *d;
    dd.proj = SIPX_PROJ_L21_STACKED; dd.pmax = 1.0; dd.ncvx = 0;
    configure_proj(ctx, s, &dd);               // the refusals, and the ExtSpec, of the set
    DeviceMemory tmp;
    upload_custom(s, tmp);
    T* dx = on_device ? nullptr : tmp.alloc<T>(G_.N);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(1);
    const SearchScratch q(tmp, s.spec.bstride, false);
    ExtProj<T> ext(s.spec, stream_);
    if (on_device) engine_after_caller();
    else SIPX_HIP(hipMemcpyAsync(dx, x, G_.N * sizeof(T), hipMemcpyHostToDevice, stream_));
    custom_fwd(stream_, s, on_device ? (const T*)x : dx, s.sbuf);
    {
      ObserverGuard og(observer());
      ObsScope obs(KID_EXT, stream_, (double)(s.spec.nblk + 1) * s.spec.bstride * sizeof(T));
      ext.observe(s.sbuf, dout, q.part, q.mp, q.dc);
    }
    finish_call(on_device, out, dout, 1);
  }

  void project(const sipx_set_desc* d, void* v, int64_t len) override {
    SIPX_HIP(hipSetDevice(device_));
    if (d->proj == SIPX_PROJ_L21 || d->proj == SIPX_PROJ_L21_JOINT || d->proj == SIPX_PROJ_L21_GROUPS || d->proj == SIPX_PROJ_TNV) {
      project_l21(d, v, len);
      return;
    }
    if (d->proj == SIPX_PROJ_L1_WEIGHTED) {
      project_l1_weighted(d, v, len);
      return;
    }
    if (d->proj == SIPX_PROJ_SIMPLEX) {
      project_simplex(d, v, len);
      return;
    }
    if (d->proj == SIPX_PROJ_CARD_GROUPS) {
      project_card_groups(d, v, len);
      return;
    }
    if (d->proj == SIPX_PROJ_L20 || d->proj == SIPX_PROJ_L20_JOINT) {
      project_l20(d, v, len);
      return;
    }
    if (d->proj == SIPX_PROJ_L21_STACKED) {
      project_l21_stacked(d, v, len);
      return;
    }
    if (d->proj == SIPX_PROJ_L2INF || d->proj == SIPX_PROJ_L2INF_JOINT || d->proj == SIPX_PROJ_L2INF_STACKED) {
      project_l2inf(d, v, len);
      return;
    }
    Grid g1;
    g1.n[0] = len; g1.n[1] = 1; g1.n[2] = 1; g1.N = len; g1.st[0] = 1; g1.st[1] = len; g1.st[2] = len;
    DeviceMemory tmp;
    T* dv = tmp.alloc<T>(len);
    const SearchScratch q(tmp, len, true);
    T *lb = nullptr, *ub = nullptr;
    SIPX_HIP(hipMemcpy(dv, v, len * sizeof(T), hipMemcpyHostToDevice));
    const int prox = d->proj;
    const T plo = (T)d->pmin, phi = (T)d->pmax;
    if (prox == SIPX_PROJ_BOUNDS_VEC && d->mode == SIPX_MODE_WHOLE && d->transform == SIPX_TRANSFORM_NONE) {
      if (!d->lb || !d->ub) throw std::runtime_error("per-element bounds need lb and ub");
      lb = tmp.alloc<T>(len); ub = tmp.alloc<T>(len);
      SIPX_HIP(hipMemcpy(lb, d->lb, len * sizeof(T), hipMemcpyHostToDevice));
      SIPX_HIP(hipMemcpy(ub, d->ub, len * sizeof(T), hipMemcpyHostToDevice));
    }
    if (prox == SIPX_PROJ_L1 && !(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    if (d->mode != SIPX_MODE_WHOLE || d->transform != SIPX_TRANSFORM_NONE || prox == SIPX_PROJ_L1_DFT || prox >= SIPX_PROJ_RANK) {   // incl. SIPX_PROJ_BOUNDS_DFT   // acts on the context grid
      if (len != G_.N) throw std::runtime_error("this projector / application mode needs a vector of the grid size");
      const ConfigCtx ctx = config_ctx();
      SetConfig<T> st;
      configure_op(ctx, st, SIPX_OP_IDENTITY);
      configure_proj(ctx, st, d);
      if (st.ext_kind) {
        st.spec.lb = st.host_lb.empty() ? nullptr : st.host_lb.data();
        st.spec.ub = st.host_ub.empty() ? nullptr : st.host_ub.data();
        st.spec.basis = st.host_basis.empty() ? nullptr : st.host_basis.data();
        ExtProj<T> ext(st.spec, stream_);
        ext.project(dv, false, q.part, q.mp, q.dc);
        if (st.ext_kind == EXT_RANK) {             // the route of a stand-alone call counts like a set's (rank_route)
          long long c[4];
          ext.route_counts(c);
          for (int q = 0; q < 4; ++q) project_rc_[q] += c[q];
        }
      } else {                                   // per-fiber bounds, expanded by configure_proj (set_config.h)
        lb = tmp.alloc<T>(len); ub = tmp.alloc<T>(len);
        SIPX_HIP(hipMemcpy(lb, st.host_lb.data(), len * sizeof(T), hipMemcpyHostToDevice));
        SIPX_HIP(hipMemcpy(ub, st.host_ub.data(), len * sizeof(T), hipMemcpyHostToDevice));
        proj_apply_grid<T>(stream_, g1, 0, nullptr, len, dv, st.prox, st.plo, st.phi, lb, ub, nullptr);
      }
      finish_call(false, v, dv, len);
      return;
    }
    const bool two = prox == SIPX_PROJ_L1 || prox == SIPX_PROJ_L2 || prox == SIPX_PROJ_ANNULUS || prox == SIPX_PROJ_CARDINALITY;
    long long* di = prox == SIPX_PROJ_CARDINALITY ? tmp.alloc<long long>(len) : nullptr;
    if (two) {
      K<T>::ps_init(stream_, q.ps, di);
      K<T>::proj_scalars_arr(stream_, len, dv, prox, plo, phi, q.ps, q.part, q.mp, q.dc, len);
    }
    proj_apply_grid<T>(stream_, g1, 0, nullptr, len, dv, prox, prox == SIPX_PROJ_BOUNDS_VEC ? T(0) : plo, phi, lb, ub, two ? q.ps : nullptr);
    finish_call(false, v, dv, len);
  }

  // sipx_segment_norms(_dev): the l1 / l2 norms of the fibers / slices of A x, in the order of the per-segment radii.  A x through the
  // operator product of apply_op into scratch of the call, one launch of k_seg_observe (seg_norm.h) on it.
  void segment_norms(int op, int mode, int dir, int norm, const void* x, void* out, int64_t* nseg, bool on_device) override {
    SIPX_HIP(hipSetDevice(device_));
    if (norm != 0 && norm != 1) throw std::runtime_error("segment norms: norm must be 0 (l1) or 1 (l2)");
    if (op != SIPX_OP_IDENTITY && op != SIPX_OP_DX && op != SIPX_OP_DY && op != SIPX_OP_DZ)
      throw std::runtime_error("fiber / slice modes need an operator with one block (identity, D_x, D_y, D_z)");
    const ConfigCtx ctx = config_ctx();
    SetConfig<T> s;
    configure_op(ctx, s, op);
    sipx_set_desc d{};
    d.op = op; d.proj = SIPX_PROJ_L2; d.mode = mode; d.dir = dir;
    if (mode == SIPX_MODE_WHOLE) throw std::runtime_error("segment norms need a fiber or slice mode");
    configure_proj(ctx, s, &d);                // the refusals, and the ExtSpec, of the sets
    const long long ns = seg_count(s.spec);
    if (nseg) *nseg = ns;
    if (!x || !out) return;                    // (a query of the length)
    DeviceMemory tmp;
    const OpScratch w = forward_scratch(tmp, s, on_device);
    T* dout = on_device ? (T*)out : tmp.alloc<T>(ns);
    const T* dv = queue_forward(w, s, x, on_device);
    {
      ObserverGuard og(observer());            // (sipx_kernel_stats mode 2 times the launch: the row of the materialised projectors)
      ObsScope obs(KID_EXT, stream_, (double)s.Mtrue * sizeof(T));
      seg_observe<T>(s.spec, norm, dv, dout, stream_);
    }
    finish_call(on_device, out, dout, ns);
  }

  void get_Q(void* Q, int64_t* offsets, int* d) override {
    need_final();
    SIPX_HIP(hipStreamSynchronize(stream_));
    if (d) *d = cds_.d;
    if (offsets) for (int b = 0; b < cds_.d; ++b) offsets[b] = cds_.off[b];
    if (Q && stencil_q_) throw std::runtime_error("stencil Q mode stores no bands (use sipx_apply_Q)");
    if (Q && comm_ && comm_->world > 1) throw std::runtime_error("a sharded context maintains its slab of Q only");
    if (Q) ensure_q_bands();
    if (Q && cds_.sym) {      // the negative bands are not maintained while solving: rebuild them from their partners
      K<T>::mirror_bands(stream_, Nx_, cds_, Q_);
      SIPX_HIP(hipStreamSynchronize(stream_));
    }
    if (Q) SIPX_HIP(hipMemcpy(Q, Q_, (size_t)Nx_ * cds_.d * sizeof(T), hipMemcpyDeviceToHost));
  }

  void q_terms(int* bands, int* matrix_free) override {
    need_final();
    if (bands) *bands = stencil_q_ ? 0 : cds_.d;
    if (matrix_free) *matrix_free = n_mfree_;
  }

  void apply_Q(const void* x, void* y) override {     // y = Q x through the solver's own kernel (either mode)
    need_final();
    if (comm_ && comm_->world > 1) throw std::runtime_error("a sharded context maintains its slab of Q only");
    SIPX_HIP(hipStreamSynchronize(stream_));
    SIPX_HIP(hipMemcpy(p_, x, Nx_ * sizeof(T), hipMemcpyHostToDevice));
    ObserverGuard og(observer());
    if (stencil_q_) K<T>::sq_spmv(stream_, G_, sq_, p_, Ap_);
    else K<T>::spmv(stream_, G_, Nx_, Q_, cds_, p_, Ap_);
    mf_terms(p_, Ap_, T(1), 0, nullptr, nullptr);
    SIPX_HIP(hipStreamSynchronize(stream_));
    SIPX_HIP(hipMemcpy(y, Ap_, Nx_ * sizeof(T), hipMemcpyDeviceToHost));
  }

  double time_spmv(int reps) override {
    need_final();
    hipEvent_t a, b;
    SIPX_HIP(hipEventCreate(&a));
    SIPX_HIP(hipEventCreate(&b));
    auto one = [&]() {
      if (stencil_q_) K<T>::sq_spmv(stream_, G_, sq_, x_, Ap_);
      else K<T>::spmv(stream_, G_, Nx_, Q_, cds_, x_, Ap_);
      mf_terms(x_, Ap_, T(1), 0, nullptr, nullptr);
    };
    one();   // warm
    SIPX_HIP(hipEventRecord(a, stream_));
    for (int k = 0; k < reps; ++k) one();
    SIPX_HIP(hipEventRecord(b, stream_));
    SIPX_HIP(hipEventSynchronize(b));
    float ms = 0;
    SIPX_HIP(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return (double)ms / reps;
  }

  // Per-kernel statistics.  mode 0: off; 1: the product of the CG iteration only (k_cds<MODE=1> / k_sq<MODE=1>: what the
  // bench line's `roofline` is measured on, inside the timed region -- two event records per CG iteration); 2: EVERY kernel
  // the engine launches (two records around each: about 5 us per launch, so this mode is for a window of its own, not for
  // the timed region).  Samples are bracketed on the stream the kernel is launched on.
  void kernel_stats(int enable, int64_t* launches, double* total_ms) override {
    need_final();
    std::vector<KAgg> agg = aggregate_samples();
    const KAgg& a = stencil_q_ ? agg[KID_SQ_DOT] : agg[KID_CDS_DOT];
    if (launches) *launches = a.launches;
    if (total_ms) *total_ms = a.ms;
    start_stats(enable);
  }
  // enable = -1: the counters only (slab_searches, rank_route) -- no synchronisation, the collection and its samples stay as they are
  const char* kernel_stats_json(int enable) override {
    const bool peek = enable < 0;
    if (!peek) need_final();         // (the counters exist before that: a context that only served sipx_project has its rank_route)
    std::vector<KAgg> agg = peek ? std::vector<KAgg>(KID_COUNT) : aggregate_samples();
    std::string& o = stats_json_;
    o = "{\"mode\": " + std::to_string(stats_mode_) + ", \"event_pair_overhead_ms\": " + std::to_string(stat_pair_ms_) + ", \"kernels\": [";
    bool first = true;
    char buf[512];
    for (int k = 0; k < KID_COUNT; ++k) {
      if (!agg[k].launches) continue;
      const bool gated = gated_kernel(k);
      std::snprintf(buf, sizeof buf,
                    "%s{\"name\": \"%s\", \"launches\": %lld, \"noop_launches\": %lld, \"total_ms\": %.6f, \"bytes_survey\": %.0f, "
                    "\"bytes_moved\": %.0f, \"gated\": %s, \"inclusive\": %s}",
                    first ? "" : ", ", kernel_name(k), (long long)agg[k].launches, (long long)agg[k].noops, agg[k].ms, agg[k].bytes_survey,
                    agg[k].bytes_moved,
                    gated ? "true" : "false", k == KID_EXT ? "true" : "false");
      o += buf;
      first = false;
    }
    // slab-decomposed solve: threshold searches that went through the speculative exchange since the context was finalised,
    // and how many of them needed their fallback (refinement rounds + full-size exchange)
    o += "], \"slab_searches\": {\"speculative_exchange\": " + std::to_string(spec_searches_) + ", \"fallbacks\": " +
         std::to_string(spec_fallbacks_) + ", \"refinement_rounds\": " + std::to_string(spec_rounds_) + "}";
    // one rank: searches through the batched chain (batched_searches) and how many of them needed their fallback sweeps
    o += std::string(", \"sparse_arrays\": ") + (slab_local_ ? "true" : "false");
    {
      // slab-decomposed long lists: which sets are projected on a materialised v -- by every rank on its own slices, or by an
      // owner rank on the gathered array -- and the fan exchanges (gathers + scatters of N w bytes) that took so far
      std::string loc, fan;
      for (int i = 0; i < p_n_; ++i) {
        if (sets_[i].slab_ext || sets_[i].slab_card || sets_[i].slab_dft) loc += (loc.empty() ? "" : ", ") + std::to_string(i);
        if (sets_[i].fan) fan += (fan.empty() ? "" : ", ") + std::to_string(i);
      }
      if (counting_)
        o += ", \"collectives\": {\"allreduce\": " + std::to_string(counting_->n_allreduce) + ", \"allreduce_with_halo\": " + std::to_string(counting_->n_grouped) +
             ", \"allgather\": " + std::to_string(counting_->n_allgather) + ", \"reduce_scatter\": " + std::to_string(counting_->n_reduce_scatter) +
             ", \"halo\": " + std::to_string(counting_->n_halo) + ", \"scatter_gather\": " + std::to_string(counting_->n_fan) +
             ", \"alltoall\": " + std::to_string(counting_->n_alltoall) + "}";
      o += ", \"slab_loose\": {\"slab_local_sets\": [" + loc + "], \"gathered_sets\": [" + fan + "], \"fan_exchanges\": " + std::to_string(fan_exchanges_) + "}";
    }
    {
      std::string t = selftest_;
      for (auto& ch : t) if (ch == '"' || ch == '\\' || (unsigned char)ch < 32) ch = ' ';
      o += ", \"comm_selftest\": \"" + t + "\"";
    }
    o += ", \"lane_set\": " + std::to_string(lane_set_);
    o += std::string(", \"q_table\": {\"on\": ") + (cds_.qtab ? "true" : "false") + ", \"reason\": \"" + qtab_reason_ + "\"}";       // the set updated on a stream of its own (-1: none), lane_start
    o += ", \"batched_searches\": {\"searches\": " + std::to_string(batch_searches_) + ", \"fallbacks\": " + std::to_string(batch_fallbacks_) + "}";
    // launches per route since the context was finalised, where one observer name covers two kernels (RouteId)
    o += ", \"routes\": {";
    for (int r = 0; r < RT_COUNT; ++r) o += std::string(r ? ", \"" : "\"") + route_name(r) + "\": " + std::to_string(routes_[r]);
    o += "}";
    // slice-rank / matrix-rank sets: which route their projector took since the context was finalised (ext_proj.hip)
    long long rc[4] = {project_rc_[0], project_rc_[1], project_rc_[2], project_rc_[3]};      // stand-alone calls (project)
    for (const auto& st : sets_) {
      if (!st.ext || st.ext_kind != EXT_RANK) continue;
      long long c[4];
      st.ext->route_counts(c);
      for (int q = 0; q < 4; ++q) rc[q] += c[q];
    }
    o += ", \"rank_route\": {\"calls\": " + std::to_string(rc[0]) + ", \"warm_started_subspace\": " + std::to_string(rc[1]) +
         ", \"full_decomposition\": " + std::to_string(rc[2]) + ", \"products_with_gram\": " + std::to_string(rc[3]) + "}";
    // per-frame l2,1 sets: Michelot's passes of the last projection (total over the frames, most in one frame, frames)
    long long fc[4] = {0, 0, 0, 0};
    for (const auto& st : sets_) {
      if (!st.ext || st.ext_kind != EXT_L21_SEG) continue;
      long long c[4];
      st.ext->route_counts(c);
      fc[0] += c[0]; fc[1] = std::max(fc[1], c[1]); fc[3] += c[3];
    }
    o += ", \"l21_frames\": {\"passes_total\": " + std::to_string(fc[0]) + ", \"passes_max\": " + std::to_string(fc[1]) +
         ", \"frames\": " + std::to_string(fc[3]) + "}";
    // weighted l2,1 sets: the Michelot passes and the flag reads of the last projection (summed over such sets), their calls and groups
    long long wc[4] = {0, 0, 0, 0};
    for (const auto& st : sets_) {
      if (!st.ext || !st.weighted || st.ext_kind == EXT_L21_GROUPS || st.ext_kind == EXT_L1_WEIGHTED) continue;
      long long c[4];
      st.ext->route_counts(c);
      for (int q = 0; q < 4; ++q) wc[q] += c[q];
    }
    o += ", \"l21_weighted\": {\"passes\": " + std::to_string(wc[0]) + ", \"flag_reads\": " + std::to_string(wc[1]) +
         ", \"calls\": " + std::to_string(wc[2]) + ", \"groups\": " + std::to_string(wc[3]) + "}";
    // l2,1 sets over fibers / slices, with or without weights: the same counts, and their segments
    long long gc[4] = {0, 0, 0, 0};
    for (const auto& st : sets_) {
      if (!st.ext || st.ext_kind != EXT_L21_GROUPS) continue;
      long long c[4];
      st.ext->route_counts(c);
      for (int q = 0; q < 4; ++q) gc[q] += c[q];
    }
    o += ", \"l21_groups\": {\"passes\": " + std::to_string(gc[0]) + ", \"flag_reads\": " + std::to_string(gc[1]) +
         ", \"calls\": " + std::to_string(gc[2]) + ", \"nseg\": " + std::to_string(gc[3]) + "}";
    // weighted l1 sets: the same counts, and the padded rows their passes run over
    long long lc[4] = {0, 0, 0, 0};
    for (const auto& st : sets_) {
      if (!st.ext || st.ext_kind != EXT_L1_WEIGHTED) continue;
      long long c[4];
      st.ext->route_counts(c);
      for (int q = 0; q < 4; ++q) lc[q] += c[q];
    }
    o += ", \"l1_weighted\": {\"passes\": " + std::to_string(lc[0]) + ", \"flag_reads\": " + std::to_string(lc[1]) +
         ", \"calls\": " + std::to_string(lc[2]) + ", \"n\": " + std::to_string(lc[3]) + "}";
    // simplex sets: the calls since the reset, those of the lane route and of the tile route (summed over such sets and the stand-alone
    // projections of this context), the segments of the last one
    long long sc[4] = {project_sc_[0], project_sc_[1], project_sc_[2], project_sc_[3]};
    for (const auto& st : sets_) {
      if (!st.ext || st.ext_kind != EXT_SIMPLEX_SEG) continue;
      long long c[4];
      st.ext->route_counts(c);
      for (int q = 0; q < 3; ++q) sc[q] += c[q];
      sc[3] = c[3];
    }
    o += ", \"simplex\": {\"calls\": " + std::to_string(sc[0]) + ", \"lane\": " + std::to_string(sc[1]) + ", \"tile\": " +
         std::to_string(sc[2]) + ", \"nseg\": " + std::to_string(sc[3]) + "}";
    // card_groups sets: the projections since the reset, the selections run by the small route and by the search route -- a projection
    // with k >= nseg runs none -- (summed over such sets and the stand-alone projections of this context), the segments of the last one
    long long cg[4] = {project_gc_[0], project_gc_[1], project_gc_[2], project_gc_[3]};
    for (const auto& st : sets_) {
      if (!st.ext || st.ext_kind != EXT_CARD_GROUPS) continue;
      long long c[4];
      st.ext->route_counts(c);
      for (int q = 0; q < 3; ++q) cg[q] += c[q];
      cg[3] = c[3];
    }
    o += ", \"card_groups\": {\"calls\": " + std::to_string(cg[0]) + ", \"small\": " + std::to_string(cg[1]) + ", \"search\": " +
         std::to_string(cg[2]) + ", \"nseg\": " + std::to_string(cg[3]) + "}";
    // l20 / l20_joint sets: the projections since the reset, the selections run by the small route, by the search route and by the
    // per-frame kernel -- a projection whose k keeps every group runs none -- (summed over such sets and the stand-alone projections of
    // this context), the groups of the last one (per frame: of a frame)
    long long l0c[5] = {project_l20c_[0], project_l20c_[1], project_l20c_[2], project_l20c_[3], project_l20c_[4]};
    for (const auto& st : sets_) {
      if (!st.ext || (st.ext_kind != EXT_L20 && st.ext_kind != EXT_L20_SEG && st.ext_kind != EXT_L20_JOINT)) continue;
      long long c[4];
      st.ext->route_counts(c);
      l20_count(st.ext_kind, c, l0c);
    }
    o += ", \"l20\": {\"calls\": " + std::to_string(l0c[0]) + ", \"small\": " + std::to_string(l0c[1]) + ", \"search\": " +
         std::to_string(l0c[2]) + ", \"frames\": " + std::to_string(l0c[3]) + ", \"groups\": " + std::to_string(l0c[4]) + "}}";
    if (!peek) start_stats(enable);
    return o.c_str();
  }
  double stat_pair_overhead_ms() const { return stat_pair_ms_; }

  void debug_proj(int set, int which, double* o) override {
    need_final();
    for (int k = 0; k < 16; ++k) o[k] = 0;
    if (set < 0 || set >= p_n_) throw std::runtime_error("set index out of range");
    const ProjScalars<T>* d = (which & 1) ? sets_[set].psf : sets_[set].ps;
    if (!d) return;
    ProjScalars<T> h;
    SIPX_HIP(hipStreamSynchronize(stream_));
    SIPX_HIP(hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost));
    o[0] = h.need; o[1] = h.theta; o[2] = h.theta_prev; o[3] = h.hw; o[4] = h.spec_lo; o[5] = h.spec_hi; o[6] = h.lo;
    o[7] = h.hi; o[8] = h.asum; o[9] = h.vmax; o[10] = h.dbg[0]; o[11] = h.dbg[1]; o[12] = h.dbg[2]; o[13] = h.dbg[3];
    o[14] = h.refine;
    o[15] = h.lean + 2 * h.dbg_sampled;
    if (which & 2) { o[4] = h.samp_theta; o[5] = h.samp_lo; o[6] = h.samp_hi; o[7] = h.samp_c; }     // the sampled prediction
  }

  void* stream() override { return (void*)stream_; }
  void* dev_rhs() override { return rhs_; }
  void* dev_x() override { return x_; }
  void get_rhs(void* out) override {
    need_final();
    if (slab_local_ && comm_->world > 1) throw std::runtime_error("a slab-decomposed context holds its planes of rhs only");
    SIPX_HIP(hipStreamSynchronize(stream_));
    SIPX_HIP(hipMemcpy(out, rhs_, Nx_ * sizeof(T), hipMemcpyDeviceToHost));
  }

 private:
  struct KSample { int kid; double bytes_survey, bytes_moved; };
  struct KAgg { long long launches = 0, noops = 0; double ms = 0, bytes_survey = 0, bytes_moved = 0; };
  hipEvent_t stat_event(size_t i) {
    while (stat_ev_.size() <= i) {
      hipEvent_t e;
      SIPX_HIP(hipEventCreate(&e));
      stat_ev_.push_back(e);
    }
    return stat_ev_[i];
  }
  static void obs_begin(void* user, int kid, hipStream_t s, double bytes_survey, double bytes_moved) {
    auto* e = static_cast<Engine<T>*>(user);
    if (e->stats_mode_ == 0 || (e->stats_mode_ == 1 && kid != KID_CDS_DOT && kid != KID_SQ_DOT)) return;
    const size_t i = e->samples_.size();
    e->samples_.push_back(KSample{kid, bytes_survey, bytes_moved});
    e->open_.push_back(i);
    SIPX_HIP(hipEventRecord(e->stat_event(2 * i), s));
  }
  static void obs_end(void* user, int kid, hipStream_t s) {
    auto* e = static_cast<Engine<T>*>(user);
    if (e->stats_mode_ == 0 || (e->stats_mode_ == 1 && kid != KID_CDS_DOT && kid != KID_SQ_DOT)) return;
    if (e->open_.empty()) return;
    const size_t i = e->open_.back();
    e->open_.pop_back();
    if (i < e->samples_.size()) SIPX_HIP(hipEventRecord(e->stat_event(2 * i + 1), s));
  }
  static void obs_route(void* user, int route) {
    if (route >= 0 && route < RT_COUNT) static_cast<Engine<T>*>(user)->routes_[route] += 1;
  }
  void drop_samples_from(size_t n) {
    if (n < samples_.size()) samples_.resize(n);
    open_.clear();
  }
  void sync_all_streams() {
    SIPX_HIP(hipStreamSynchronize(stream_));
    for (hipStream_t q : pool_) if (q != stream_) SIPX_HIP(hipStreamSynchronize(q));
    if (cstream_) SIPX_HIP(hipStreamSynchronize(cstream_));
  }
  // kernels some of whose launches return at once on a device-side condition
  static bool gated_kernel(int k) {
    return k == KID_PASS_FIRST || k == KID_PASS_LEAN || k == KID_PASS_PROBE || k == KID_PASS_COMPACT || k == KID_SAMPLE ||
           k == KID_DECIDE || k == KID_CDS_FUSED || k == KID_CG_XR || k == KID_CG_P || k == KID_SLOT_SUMS;
  }
  std::vector<KAgg> aggregate_samples() {
    sync_all_streams();
    std::vector<KAgg> agg(KID_COUNT);
    for (size_t i = 0; i < samples_.size(); ++i) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, stat_ev_[2 * i], stat_ev_[2 * i + 1]) != hipSuccess) { (void)hipGetLastError(); continue; }
      KAgg& a = agg[samples_[i].kid];
      // two records with nothing between them are still some microseconds apart on the stream's timeline; that share of
      // every sample is not kernel time (calibrated on the idle stream when the collection is switched on)
      const double t = (double)ms - stat_pair_ms_;
      a.launches += 1;
      a.ms += t > 0 ? t : 0;
      // a gated launch (the pass of an l1 search that the device-side state did not ask for, a CG kernel past convergence) returns at
      // once: a launch that finished sooner than its bytes could cross the fabric at twice the HBM peak did not move them
      const bool noop = gated_kernel(samples_[i].kid) && samples_[i].bytes_moved > 0 && t * 1e-3 < samples_[i].bytes_moved / 16e12;
      a.noops += noop ? 1 : 0;
      a.bytes_survey += noop ? 0.0 : samples_[i].bytes_survey;
      a.bytes_moved += noop ? 0.0 : samples_[i].bytes_moved;
    }
    return agg;
  }
  void start_stats(int mode) {
    samples_.clear();
    open_.clear();
    stats_mode_ = 0;
    if (mode) {
      std::vector<float> gap;
      for (int k = 0; k < 16; ++k) {
        SIPX_HIP(hipEventRecord(stat_event(2 * k), stream_));
        SIPX_HIP(hipEventRecord(stat_event(2 * k + 1), stream_));
      }
      SIPX_HIP(hipStreamSynchronize(stream_));
      for (int k = 0; k < 16; ++k) {
        float ms = 0;
        SIPX_HIP(hipEventElapsedTime(&ms, stat_ev_[2 * k], stat_ev_[2 * k + 1]));
        gap.push_back(ms);
      }
      std::sort(gap.begin(), gap.end());
      stat_pair_ms_ = gap[gap.size() / 2];
    }
    stats_mode_ = mode;
  }
  // always installed: the route counters run whether or not statistics are collected (obs_begin / obs_end return at once then)
  const LaunchObserver* observer() const { return &obs_; }

  void need_final() const {
    if (!finalized_) throw std::runtime_error("call sipx_finalize first");
    SIPX_HIP(hipSetDevice(device_));
  }

  // Lanes that share one row of a compressed view: the smallest power of two that covers the mean length of the non-empty rows,
  // 1 .. 64.  A wave then reads 64 / G rows' runs of values and indices per step; rows longer than the group take further strides,
  // shorter ones leave lanes idle -- by the mean, as many lanes idle in the short rows as extra strides are walked in the long.
  static int mf_lanes(const std::vector<int>& ptr) {
    long long rows = 0;
    for (size_t r = 0; r + 1 < ptr.size(); ++r) rows += ptr[r + 1] > ptr[r];
    if (rows == 0) return 1;
    const double mean = (double)ptr.back() / (double)rows;
    int g = 1;
    while (g < 64 && (double)g < mean) g *= 2;
    return g;
  }
  // s = A x, rhs += A'(rho y + l), partials of ||A'(y - y_old)||^2 of a caller-supplied operator: a matrix-free term through the
  // kernels its term of Q uses, a set that handed over CDS bands through the one-thread-per-row kernels as ever
  void custom_fwd(hipStream_t q, const SetState<T>& s, const T* x, T* out) {
    if (s.mfree) K<T>::mf_fwd(q, s.mfA, x, out, nullptr);
    else K<T>::csr_spmv(q, s.Mtrue, s.d_rowptr, s.d_colidx, s.d_rval, x, out);
  }
  void custom_adj_rhs(hipStream_t q, const SetState<T>& s, T rho) {
    if (!s.mfree) { K<T>::csc_adj_rhs(q, G_.N, s.d_colptr, s.d_rowval, s.d_nzval, s.y, s.l, rho, rhs_, 1); return; }
    MfAdj<T> a;
    a.y = s.y; a.l = s.l; a.rho = rho; a.in_mode = 1;
    a.out = rhs_;
    K<T>::mf_adj(q, s.mfAt, a);
  }
  void custom_adj_norm(hipStream_t q, const SetState<T>& s, double* partials) {
    if (!s.mfree) { K<T>::csc_adj_norm(q, G_.N, s.d_colptr, s.d_rowval, s.d_nzval, s.dy, partials); return; }
    MfAdj<T> a;
    a.y = s.dy;
    a.dot = 2; a.partials = partials;
    K<T>::mf_adj(q, s.mfAt, a);
  }
  // out += sign * sum_i rho_i A_i'(A_i v) over the matrix-free terms, in set order, on the engine stream.  dot (MfAdj::dot) is
  // taken by the LAST adjoint launch, on the complete `out`, into slot 0 of the CG partials.
  void mf_terms(const T* v, T* out, T sign, int dot, const T* p, const int* done) {
    if (n_mfree_ == 0) return;
    int left = n_mfree_;
    for (int i = 0; i < p_n_; ++i) {
      const SetState<T>& s = sets_[i];
      if (!s.mfree) continue;
      K<T>::mf_fwd(stream_, s.mfA, v, s.mf_t, done);
      MfAdj<T> a;
      a.y = s.mf_t;
      a.alpha = sign * s.mf_rho;
      a.out = out;
      a.done = done;
      if (--left == 0 && dot) { a.dot = dot; a.p = p; a.partials = part_cg_; a.slot = 0; }
      K<T>::mf_adj(stream_, s.mfAt, a);
    }
  }
  void upload_mfree(SetState<T>& s) {
    const long long N = G_.N, M = s.Mtrue, nnz = (long long)s.h_rowval.size();
    std::vector<int> colptr(s.h_colptr.begin(), s.h_colptr.end()), rowidx(s.h_rowval.begin(), s.h_rowval.end());
    std::vector<int> rowptr(M + 1, 0), colidx(nnz);
    std::vector<T> rval(nnz);
    for (long long k = 0; k < nnz; ++k) rowptr[rowidx[k] + 1]++;
    for (long long r = 0; r < M; ++r) rowptr[r + 1] += rowptr[r];
    std::vector<int> next(rowptr.begin(), rowptr.end() - 1);
    for (long long j = 0; j < N; ++j)                       // (columns ascend inside a row of the CSR copy, as in upload_custom)
      for (int k = colptr[j]; k < colptr[j + 1]; ++k) {
        const int q = next[rowidx[k]]++;
        colidx[q] = (int)j;
        rval[q] = s.h_nzval[k];
      }
    auto up = [&](auto*& dst, const auto& src) {
      using E = typename std::remove_reference<decltype(src)>::type::value_type;
      dst = mem_.alloc<E>(std::max<size_t>(src.size(), 1), Mem::NoFill);
      if (!src.empty()) SIPX_HIP(hipMemcpy(dst, src.data(), src.size() * sizeof(E), hipMemcpyHostToDevice));
    };
    up(s.mf_colptr, colptr); up(s.mf_rowidx, rowidx); up(s.d_nzval, s.h_nzval);
    up(s.mf_rowptr, rowptr); up(s.mf_colidx, colidx); up(s.d_rval, rval);
    s.sbuf = mem_.alloc<T>(M, Mem::State);
    s.mf_t = mem_.alloc<T>(M, Mem::State);
    s.mfA.rows = (int)M; s.mfA.nnz = nnz; s.mfA.ptr = s.mf_rowptr; s.mfA.idx = s.mf_colidx; s.mfA.val = s.d_rval; s.mfA.lanes = mf_lanes(rowptr);
    s.mfAt.rows = (int)N; s.mfAt.nnz = nnz; s.mfAt.ptr = s.mf_colptr; s.mfAt.idx = s.mf_rowidx; s.mfAt.val = s.d_nzval; s.mfAt.lanes = mf_lanes(colptr);
    s.h_colptr.clear(); s.h_rowval.clear(); s.h_nzval.clear();
  }
  // device copies: CSC as given, and the CSR view (rows ascending, columns ascending inside a row: a counting sort by row
  // of the column-major entries keeps that order) for s = A x
  void upload_custom(SetState<T>& s) {
    if (s.mfree) { upload_mfree(s); return; }
    upload_custom(s, mem_);
  }
  // (mem: the context's memory for a set; the scratch of a stand-alone call, sipx_l21_stacked_norm)
  void upload_custom(SetState<T>& s, DeviceMemory& mem) {
    const long long N = G_.N, M = s.Mtrue, nnz = (long long)s.h_rowval.size();
    std::vector<long long> rowptr(M + 1, 0), colidx(nnz);
    std::vector<T> rval(nnz);
    for (long long k = 0; k < nnz; ++k) rowptr[s.h_rowval[k] + 1]++;
    for (long long r = 0; r < M; ++r) rowptr[r + 1] += rowptr[r];
    std::vector<long long> next(rowptr.begin(), rowptr.end() - 1);
    for (long long j = 0; j < N; ++j)
      for (long long k = s.h_colptr[j]; k < s.h_colptr[j + 1]; ++k) {
        const long long q = next[s.h_rowval[k]]++;
        colidx[q] = j;
        rval[q] = s.h_nzval[k];
      }
    auto up = [&](auto*& dst, const auto& src) {
      using E = typename std::remove_reference<decltype(src)>::type::value_type;
      dst = mem.alloc<E>(std::max<size_t>(src.size(), 1), Mem::NoFill);
      if (!src.empty()) SIPX_HIP(hipMemcpy(dst, src.data(), src.size() * sizeof(E), hipMemcpyHostToDevice));
    };
    up(s.d_colptr, s.h_colptr); up(s.d_rowval, s.h_rowval); up(s.d_nzval, s.h_nzval);
    up(s.d_rowptr, rowptr); up(s.d_colidx, colidx); up(s.d_rval, rval);
    s.sbuf = mem.alloc<T>(M, Mem::State);
    s.h_colptr.clear(); s.h_rowval.clear(); s.h_nzval.clear();
  }

  int q_col(long long off) const {
    for (int b = 0; b < cds_.d; ++b)
      if (cds_.off[b] == off) return b;
    throw std::runtime_error("attempted to update a diagonal in A in CDS storage that does not exist. A and B need "
                             "to have the same nonzero diagonals");   // CDS_scaled_add!.jl:18-20
  }

  void plan_Q_offsets() {  // PARSDMM_initialize.jl:216-221: first-seen offsets over a zero-padded table
    std::vector<long long> seen;
    auto see = [&](long long o) {
      if (std::find(seen.begin(), seen.end(), o) == seen.end()) seen.push_back(o);
    };
    for (auto& s : sets_) {
      if (s.mfree) continue;               // a matrix-free term contributes no bands
      if (s.ata_off.size() > 999) throw std::runtime_error("more than 999 bands in one set");
      for (long long o : s.ata_off) see(o);
      see(0);
    }
    see(0);                                // (every set matrix-free: Q keeps its -- zero -- diagonal band)
    if ((int)seen.size() > MAXD)
      throw std::runtime_error("Q has more bands than this build supports (" + std::to_string(seen.size()) + " > " + std::to_string(MAXD) +
                               "): a custom sparse operator (SIPX_OP_CSC) can be passed without its A'A (ata_R = NULL) -- it then enters Q "
                               "as a matrix-free term and contributes no bands");
    cds_.d = (int)seen.size();
    for (int b = 0; b < cds_.d; ++b) cds_.off[b] = seen[b];
    // symmetric read of Q (CdsArgs::sym): every negative band needs its positive partner, at a band index >= 1 so that
    // the shifted address never leaves the allocation; explicit AtA bands must be symmetric bit for bit
    bool ok = !env_knobs().cds_full;      // SIPX_CDS_FULL=1: read all d bands of Q (no symmetric partner reads)
    for (int b = 0; b < cds_.d && ok; ++b) {
      cds_.partner[b] = b;
      if (cds_.off[b] >= 0) continue;
      int pb = -1;
      for (int c = 0; c < cds_.d; ++c)
        if (cds_.off[c] == -cds_.off[b]) pb = c;
      if (pb < 1) ok = false;
      else cds_.partner[b] = pb;
    }
    for (auto& s : sets_) ok = ok && (s.host_ata.empty() || explicit_bands_symmetric(s));
    cds_.sym = ok ? 1 : 0;
    // the z-marching product (k_cds_march): the 7-band matrix of a 3-D grid in one of the two band orders it is compiled for
    cds_.march = 0;
    if (cds_.sym && cds_.d == 7 && ndim_ == 3 && !mk_) {
      const long long s1 = G_.st[1], s2 = G_.st[2];
      const long long o1[7] = {0, -1, 1, -s1, s1, -s2, s2}, o2[7] = {0, -s2, -s1, -1, 1, s1, s2};
      bool m1 = true, m2 = true;
      for (int b = 0; b < 7; ++b) { m1 = m1 && cds_.off[b] == o1[b]; m2 = m2 && cds_.off[b] == o2[b]; }
      cds_.march = m1 ? 1 : (m2 ? 2 : 0);
      const long long want[4] = {0, 1, s1, s2};
      for (int q = 0; q < 4; ++q)
        for (int b = 0; b < 7; ++b)
          if (cds_.off[b] == want[q]) cds_.mb[q] = b;
      for (int a = 0; a < 3; ++a) cds_.gn[a] = G_.n[a];
    }
  }

  bool explicit_bands_symmetric(const SetState<T>& s) const {
    const long long N = G_.N;
    for (size_t b = 0; b < s.ata_off.size(); ++b) {
      const long long o = s.ata_off[b];
      if (o >= 0) continue;
      long long pb = -1;
      for (size_t c = 0; c < s.ata_off.size(); ++c)
        if (s.ata_off[c] == -o) pb = (long long)c;
      if (pb < 0) return false;
      const T* lo = s.host_ata.data() + b * (size_t)N;
      const T* up = s.host_ata.data() + (size_t)pb * (size_t)N;
      for (long long r = -o; r < N; ++r)
        if (std::memcmp(&lo[r], &up[r + o], sizeof(T)) != 0) return false;
    }
    return true;
  }

  // stencil mode: the whole of Q is four scalars, recomputed from the current rho (no update history)
  void stencil_weights(const double* rho) {
    double w0 = 0, w[3] = {0, 0, 0};
    sq_.mask = 0;
    for (int i = 0; i < p_n_; ++i) {
      const SetState<T>& s = sets_[i];
      const double r = (double)(T)rho[i];
      if (s.nblk == 0) w0 += r;
      for (int q = 0; q < s.nblk; ++q) {
        w[s.dir[q]] += r * (double)(T)(s.ih[q] * s.ih[q]);
        sq_.mask |= 1 << s.dir[q];
      }
    }
    sq_.w0 = (T)w0;
    for (int d = 0; d < 3; ++d) sq_.w[d] = (T)w[d];
  }

  void assemble_Q() {      // PARSDMM_initialize.jl:222-230
    cds_.qtab = nullptr;      // (the bands are assembled; build_q_table decides about the table afterwards)
    q_stale_ = false;
    if (stencil_q_) {
      for (auto& s : sets_)
        if (s.ata) throw std::runtime_error("stencil Q mode needs descriptor-generated AtA for every set (pass ata_R = NULL)");
      std::vector<double> r(rho_.begin(), rho_.end());
      stencil_weights(r.data());
      return;
    }
    // (sparse arrays: the rows of every band that the rank's part of the x-step reads)
    if (Q_) {                       // sipx_reset: the bands are there, zero them and add the sets up again
      mem_.zero(Q_, stream_);
    } else if (slab_local_) {
      std::vector<std::pair<size_t, size_t>> rg;
      long long maxoff = 0;
      for (int b = 0; b < cds_.d; ++b) maxoff = std::max<long long>(maxoff, std::llabs(cds_.off[b]));
      for (int b = 0; b < cds_.d; ++b) {
        // rows [r0 - maxoff, r1) of every band: the symmetric read takes band +o at row r - o -- for the first rows of the grid
        // that is the TAIL of the band stored in front (masked, but loaded), so the range is not clipped at the band's first row
        const long long lo = std::max<long long>(0, (long long)b * Nx_ + (r1_ > r0_ ? r0_ : 0) - maxoff - 64);
        const long long hi = std::min<long long>((long long)Nx_ * cds_.d, (long long)b * Nx_ + std::max(qr1_, qr0_) + 64);
        if (hi > lo) rg.push_back({(size_t)lo * sizeof(T), (size_t)hi * sizeof(T)});
      }
      Q_ = (T*)mem_.alloc_sparse((size_t)Nx_ * cds_.d * sizeof(T), rg, device_);
    } else {
      Q_ = mem_.alloc<T>((size_t)Nx_ * cds_.d);
    }
    if (mk_) {
      std::vector<T> al(rho_.begin(), rho_.end());
      mk_q_update(al);
      return;
    }
    QArgs<T> a;
    a.nsets = 0;
    for (int i = 0; i < p_n_; ++i) {                                 // Q = 0 + rho_1 AtA_1 + rho_2 AtA_2 + ...
      if (sets_[i].mfree) sets_[i].mf_rho = rho_[i];                 // (a matrix-free term: no bands; sipx_reset comes through here too)
      else push_qset(a, sets_[i], rho_[i]);
    }
    q_apply(a);
  }

  // Minkowski mode: Q[:, b] += alpha_i AtA_i[:, b] for the sets with alpha_i != 0, batches of MAX_SETS in set order
  void mk_q_update(const std::vector<T>& alpha) {
    MkArgs<T> a;
    a.nsets = 0;
    for (int i = 0; i < p_n_; ++i) {
      if (alpha[i] == T(0)) continue;
      const SetState<T>& s = sets_[i];
      for (long long o : s.ata_off) (void)q_col(o);
      MkSet<T>& m = a.s[a.nsets++];
      m.alpha = alpha[i];
      m.nblk = s.nblk;
      m.comp = s.comp;
      for (int k = 0; k < 3; ++k) { m.dir[k] = s.dir[k]; m.ih[k] = s.ih[k]; }
      if (a.nsets == MAX_SETS) {
        K<T>::q_update_mk(stream_, G_, cds_, a, Q_);
        a.nsets = 0;
      }
    }
    K<T>::q_update_mk(stream_, G_, cds_, a, Q_);
  }

  void push_qset(QArgs<T>& a, const SetState<T>& s, T alpha) {
    if (s.ata_off.size() > 9) throw std::runtime_error("more than 9 bands in one set's AtA are not supported");
    for (long long o : s.ata_off) (void)q_col(o);     // CDS_scaled_add!.jl:18-20: the diagonal must exist in Q
    if (a.nsets == MAX_SETS) {                         // flush a full batch, keep the order
      q_apply(a);
      a.nsets = 0;
    }
    QSet<T>& q = a.s[a.nsets++];
    q.alpha = alpha;
    q.ata = s.ata;
    q.nblk = s.nblk;
    for (int k = 0; k < 3; ++k) { q.dir[k] = s.dir[k]; q.ih[k] = s.ih[k]; }
    q.nband = (int)s.ata_off.size();
    for (int k = 0; k < q.nband; ++k) q.off[k] = s.ata_off[k];
  }

  SetArgs<T> set_args(const SetState<T>& s, T rho, T gamma, int flags) const {
    SetArgs<T> a;
    a.y = s.y; a.l = s.l; a.dy = s.dy; a.lh0 = s.lh0; a.s0 = s.s0;
    a.y0 = s.snap == 0 ? s.y : s.y0;          // the snapshot pair (the zero-filled other pair before the first snapshot)
    a.l0 = s.snap == 0 ? s.l : s.l0;
    a.yo = s.y; a.lo = s.l;
    a.v = scr_v_;
    a.x = x_; a.m = m_; a.xold = xold_; a.lb = s.lb; a.ub = s.ub;
    a.nblk = s.nblk;
    for (int q = 0; q < 3; ++q) { a.dir[q] = s.dir[q]; a.ih[q] = s.ih[q]; }
    a.rho = rho;
    a.rho1 = T(1) / rho;       // rho1 = TF(1.0) ./ rho   update_y_l.jl:33-34
    a.gamma = gamma;
    a.prox = s.prox;
    a.plo = s.plo; a.phi = s.phi;
    a.ps = s.ps;
    a.flags = flags;
    a.vsrc = 0;
    return a;
  }

  // The same for a set that all ranks project together (identity operator: s = src): this rank's slab of slices only, the
  // partial sums of the ranks add up in the all-reduce of the packed per-set sums.
  void dist_feasibility(SetState<T>& s, const T* src, double* dst, int set = 0) {
    const long long nloc = r1_ - r0_;
    if (nloc > 0) {
      SIPX_HIP(hipMemcpyAsync(loose_v_ + r0_, src + r0_, nloc * sizeof(T), hipMemcpyDeviceToDevice, stream_));
      SIPX_HIP(hipMemcpyAsync(loose_w_ + r0_, src + r0_, nloc * sizeof(T), hipMemcpyDeviceToDevice, stream_));
      if (!s.slab_dft) s.ext->project(loose_v_ + r0_, true, part_tmp_, maxpart_, scr_c_);
    }
    // (the slab-decomposed transform is a collective: ranks without planes take part)
    if (s.slab_dft) s.ddft->project(loose_v_ + r0_, true, comm_.get(), &hooks_, part_tmp_, maxpart_, scr_c_, scr_c_len_, (int*)hovf_ + set);
    ext_dist2<T>(stream_, nloc, loose_v_ + r0_, loose_w_ + r0_, dst);
  }

  // A gathered set of a slab-decomposed solve (SetState::fan).  fan_collect: every rank materialises v (v_is_s = 0) or s = A x
  // (1) on its planes -- rows a difference operator does not have stay zero -- and the owner gathers the whole array;
  // fan_project_owner: P in place on the owner (a library-backed projector, or the cardinality search on the array: the k-th
  // magnitude and the tie rule by lowest padded index are those of the on-the-fly search, the zeros of the missing rows are the
  // smallest magnitudes there are); fan_return: every rank receives its planes of P(v), and the last plane of the rank below,
  // which the update recomputes for the adjoint stencils (Gyl_).  Engine stream, set order: the same on every rank.
  // In an update the gathered sets come FIRST (fan_begin: collect, the owner projects on the fan stream, which waits for the
  // gather), then every rank's own sets on the engine stream, and only then the scatters (fan_return waits for the fan stream): an
  // owner's whole-array projection runs beside its share of the slab-local sets instead of in front of everybody's.
  void fan_collect(SetState<T>& s, const SetArgs<T>& a, int v_is_s, T* buf) {
    if (r1_ > r0_) SIPX_HIP(hipMemsetAsync(buf + r0_, 0, (size_t)(r1_ - r0_) * sizeof(T), stream_));
    SetArgs<T> b = a;
    b.v = buf;
    K<T>::store_v(stream_, Gr_, b, v_is_s, buf);
    comm_->gather(buf, (size_t)chunk_, dtype_code(), s.fan_owner, stream_);
    ++fan_exchanges_;
  }
  void fan_project_owner(SetState<T>& s, bool feas, T* buf, hipStream_t q, double* ptmp, T* mpart, T* cbuf) {
    ObsScope obs(KID_EXT, q, 0.0);
    if (s.ext_kind) {
      s.ext->set_stream(q);
      s.ext->project(buf, feas, ptmp, mpart, cbuf);
    } else {
      ProjScalars<T>* ps = feas ? s.psf : s.ps;
      K<T>::proj_scalars_arr(q, G_.N, buf, s.prox, s.plo, s.phi, ps, ptmp, mpart, cbuf, s.Mtrue);
      proj_apply_grid<T>(q, G_, s.nblk, s.dir, G_.N, buf, s.prox, s.plo, s.phi, (const T*)nullptr, (const T*)nullptr, ps);
    }
  }
  void fan_begin(SetState<T>& s, const SetArgs<T>& a) {
    fan_collect(s, a, 0, s.fanv);
    if (comm_->rank != s.fan_owner) return;
    // (the all-kernel statistics window times one kernel at a time on the engine stream: in turn there)
    hipStream_t q = (fan_st_ && stats_mode_ != 2) ? fan_st_ : stream_;
    if (q != stream_) {
      SIPX_HIP(hipEventRecord(fan_fork_, stream_));
      SIPX_HIP(hipStreamWaitEvent(q, fan_fork_, 0));
    }
    // (in turn on the engine stream the fan stream's scratch is idle: its compaction buffer is whole-size, the engine's may not be)
    fan_project_owner(s, false, s.fanv, q, fan_ptmp_, fan_mpart_, fan_c_);
    if (q != stream_) SIPX_HIP(hipEventRecord(s.fan_ev, q));
    s.fan_on_side = q != stream_;
  }
  void fan_return(SetState<T>& s) {
    const int dt = dtype_code();
    T* buf = s.fanv;
    if (s.fan_on_side) { SIPX_HIP(hipStreamWaitEvent(stream_, s.fan_ev, 0)); s.fan_on_side = false; }
    comm_->scatter(buf, (size_t)chunk_, dt, s.fan_owner, stream_);
    ++fan_exchanges_;
    if (!s.ident && r1_ > r0_ && (prev_ >= 0 || next_ >= 0))
      comm_->halo_exchange(buf + r0_, buf + r0_ - plane_, prev_, buf + r1_ - plane_, buf + r1_, next_, (size_t)plane_, dt, stream_);
  }
  void fan_feasibility(SetState<T>& s, const SetArgs<T>& a, double* dst) {
    fan_collect(s, a, 1, loose_v_);
    if (comm_->rank != s.fan_owner) return;
    SIPX_HIP(hipMemcpyAsync(loose_w_, loose_v_, (size_t)s.Mpad * sizeof(T), hipMemcpyDeviceToDevice, stream_));
    fan_project_owner(s, true, loose_v_, stream_, part_tmp_, maxpart_, fan_c_);      // (fan_c_: whole-size, this rank owns a gathered set)
    ext_dist2<T>(stream_, s.Mpad, loose_v_, loose_w_, dst);
  }

  // ||P(s) - s||^2, ||s||^2 for a library-backed projector: s = A x materialised twice, one copy projected
  void ext_feasibility(SetState<T>& s, const SetArgs<T>& a, double* dst) {
    K<T>::store_v(stream_, s.custom ? s.gm : G_, a, 1, scr_v_);      // (a custom operator: a.x is s = A x, M entries)
    SIPX_HIP(hipMemcpyAsync(scr_w_, scr_v_, s.Mpad * sizeof(T), hipMemcpyDeviceToDevice, stream_));
    s.ext->project(scr_v_, true, part_tmp_, maxpart_, scr_c_);
    ext_dist2<T>(stream_, s.Mpad, scr_v_, scr_w_, dst);
  }

  T feas_value(double fe, double ss) const {
    return (T)std::sqrt(fe) / ((T)std::sqrt(ss) + T(100) * std::numeric_limits<T>::epsilon());
  }

  // Import / export between the reference's row order (host) and the padded layout (device): one contiguous PCIe
  // copy plus a device gather / scatter per operator block (the pads keep the zeros they were allocated with).
  void upload_rows(const SetConfig<T>& s, const T* rows, T* dev) const {
    io_h2d_ += s.Mtrue * (long long)sizeof(T);
    if (s.ident || s.custom) {
      SIPX_HIP(hipMemcpy(dev, rows, (size_t)s.Mtrue * sizeof(T), hipMemcpyHostToDevice));
      return;
    }
    DeviceMemory own;
    T* tmp = own.alloc<T>(s.Mtrue, Mem::NoFill);
    SIPX_HIP(hipMemcpy(tmp, rows, (size_t)s.Mtrue * sizeof(T), hipMemcpyHostToDevice));
    long long r0 = 0;
    for (int q = 0; q < s.nblk; ++q) {
      K<T>::rows_unpack(stream_, G_, s.dir[q], s.blk_rows[q], tmp + r0, dev + (long long)q * G_.N);
      r0 += s.blk_rows[q];
    }
    SIPX_HIP(hipStreamSynchronize(stream_));
  }
  // (sparse arrays: through a whole-size temporary, of which the rank's share is kept)
  void upload_rows_ranged(const SetState<T>& s, const T* rows, T* dev) const {
    if (!slab_local_) { upload_rows(s, rows, dev); return; }
    DeviceMemory tmp;
    T* full = tmp.alloc<T>((size_t)s.Mpad);
    upload_rows(s, rows, full);
    const long long c0 = std::max<long long>(0, wlo_), c1 = std::min<long long>(G_.N, whi_);
    for (int q = 0; q < s.nblk_or1() && c1 > c0; ++q)
      SIPX_HIP(hipMemcpy(dev + (long long)q * G_.N + c0, full + (long long)q * G_.N + c0, (c1 - c0) * sizeof(T), hipMemcpyDeviceToDevice));
    SIPX_HIP(hipDeviceSynchronize());
  }
  void download_rows(const SetConfig<T>& s, const T* dev, T* rows) const {
    io_d2h_ += s.Mtrue * (long long)sizeof(T);
    SIPX_HIP(hipStreamSynchronize(stream_));
    if (s.ident || s.custom) {
      host_prefault(rows, (size_t)s.Mtrue * sizeof(T));
      SIPX_HIP(hipMemcpy(rows, dev, (size_t)s.Mtrue * sizeof(T), hipMemcpyDeviceToHost));
      return;
    }
    DeviceMemory own;
    T* tmp = own.alloc<T>(s.Mtrue, Mem::NoFill);
    long long r0 = 0;
    for (int q = 0; q < s.nblk; ++q) {
      K<T>::rows_pack(stream_, G_, s.dir[q], s.blk_rows[q], dev + (long long)q * G_.N, tmp + r0);
      r0 += s.blk_rows[q];
    }
    SIPX_HIP(hipStreamSynchronize(stream_));
    host_prefault(rows, (size_t)s.Mtrue * sizeof(T));
    SIPX_HIP(hipMemcpy(rows, tmp, (size_t)s.Mtrue * sizeof(T), hipMemcpyDeviceToHost));
  }

  int dtype_code() const { return sizeof(T) == 8 ? SIPX_F64 : SIPX_F32; }

  // partials of the per-set slots -> hres_ (pinned).  Sharded: summed over the ranks on the way (sets a rank does not own
  // contribute the zeros their slots were allocated with), so every rank reads the sums of every set.
  void reduce_set_sums(int nslots, YlPlan::Route route) {
    if (comm_ && route == YlPlan::Route::WithNextHead) {
      K<T>::fin_sum(stream_, part_sets_, nslots, dres_, nullptr);
      merged_nslots_ = nslots;
    } else if (comm_) {
      K<T>::fin_sum(stream_, part_sets_, nslots, dres_, nullptr);
      comm_->allreduce_sum(dres_, (size_t)nslots, SIPX_F64, stream_);
      K<T>::copy_f64(stream_, dres_, hres_, nslots);
    } else if (route == YlPlan::Route::ByWord) {
      K<T>::fin_sum(stream_, part_sets_, nslots, nullptr, hres_, sums_ticket_, (unsigned long long*)sums_word_, ++sums_seq_);
    } else {
      K<T>::fin_sum(stream_, part_sets_, nslots, nullptr, hres_);
    }
  }

  // The one spin-wait on a pinned word the device publishes.  arrived() loads the word (each caller with its own memory order)
  // and says whether it holds what is awaited.  Whenever (spins & query_mask) == 0 the stream is queried -- a query costs the
  // runtime tens of microseconds: rarely -- and should it have run dry without the word (a faulted kernel), ran_dry() decides.
  template <typename Arrived, typename RanDry>
  void spin_until(Arrived arrived, unsigned query_mask, RanDry ran_dry) {
    for (unsigned spins = 1;; ++spins) {
      if (arrived()) return;
      if ((spins & query_mask) == 0) {
        const hipError_t q = hipStreamQuery(stream_);
        if (q == hipSuccess) {
          if (!arrived()) ran_dry();
          return;
        }
        if (q != hipErrorNotReady) SIPX_HIP(q);
        (void)hipGetLastError();        // hipErrorNotReady is not an error: keep it out of the launch checks
      }
    }
  }

  // Verdict of CG iteration `iter` of solve `seq`: spins on the ticket word, which the device publishes as soon as the
  // verdict is known (and after the state mirror, so that is complete too).  Every enqueued iteration publishes one; should
  // the stream nevertheless run dry without it, the mirror decides.
  bool wait_ticket(unsigned seq, int iter, const CgState<T>* mirror) {
    // ticket = (seq << 32) | (iter << 1) | done.  A ticket of a LATER iteration of this solve (small grids queue one
    // iteration ahead) means that this one did not converge: past `done` no kernel publishes anything.
    bool done = false;
    spin_until([&] {
      const unsigned long long t = __atomic_load_n(ticket_, __ATOMIC_ACQUIRE);
      if ((unsigned)(t >> 32) != seq) return false;
      const unsigned ti = (unsigned)(t & 0xffffffffull) >> 1;
      if (ti < (unsigned)iter) return false;
      done = ti == (unsigned)iter ? (t & 1ull) != 0 : false;
      return true;
    }, 0xfff, [&] { done = mirror->done != 0; });
    return done;
  }

  // the sequence number k_fin_sum publishes behind the sums (pinned; see there)
  void wait_word(volatile unsigned long long* word, unsigned long long seq) {
    spin_until([&] { return __atomic_load_n((unsigned long long*)word, __ATOMIC_ACQUIRE) == seq; }, 0x3ffff, [] {
      throw std::runtime_error("internal: the stream ran dry without the sums of the y/l update (a kernel faulted?)");
    });
  }

  // the word k_spec_decide publishes for a set: (seq << 2) | verdict bits
  unsigned wait_verdict(volatile unsigned* word, unsigned seq) {
    unsigned w = 0;
    spin_until([&] { return ((w = __atomic_load_n((unsigned*)word, __ATOMIC_ACQUIRE)) >> 2) == seq; }, 0x3ffff, [] {
      throw std::runtime_error("internal: the stream ran dry without the verdict of a threshold search (a kernel faulted?)");
    });
    return w & 3u;
  }

  void dump_ps(int set, const double* reg) {       // SIPX_SPEC_DEBUG: the state of a search as the device sees it (synchronises)
    ProjScalars<T> h;
    double r[PREP_SLOTS + 1];
    SIPX_HIP(hipStreamSynchronize(stream_));
    SIPX_HIP(hipMemcpy(&h, sets_[set].ps, sizeof(h), hipMemcpyDeviceToHost));
    SIPX_HIP(hipMemcpy(r, reg, sizeof(r), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[sipx spec]     set %d: need %d spec_ok %d refine %d lean %d ovf %d bracket (%.9g, %.9g] spec (%.9g, %.9g] n_compact %llu t0 %.9g t7 %.9g\n"
                 "[sipx spec]       S", set, h.need, h.spec_ok, h.refine, h.lean, h.spec_overflow, h.lo, h.hi, h.spec_lo, h.spec_hi,
                 (unsigned long long)h.n_compact, h.t[0], h.t[L1_K - 1]);
    for (int k = 0; k < L1_K; ++k) std::fprintf(stderr, " %.6g", r[3 + k]);
    std::fprintf(stderr, " C");
    for (int k = 0; k < L1_K; ++k) std::fprintf(stderr, " %.0f", r[3 + L1_K + k]);
    std::fprintf(stderr, " asum %.6g ovf %.0f\n", r[0], r[PREP_SLOTS]);
    std::fprintf(stderr, "[sipx spec]       theta %.9g theta_prev %.9g hw %.4g sampled %d samp_theta %.9g samp (%.9g, %.9g) samp_c %.0f want_sample %d rescaled %d\n",
                 (double)h.theta, h.theta_prev, h.hw, h.sampled, h.samp_theta, h.samp_lo, h.samp_hi, h.samp_c, h.want_sample, h.rescaled);
  }

  void free_set(SetState<T>& s) {
    if (s.st) (void)hipStreamSynchronize(s.st);
    if (s.ev) (void)hipEventDestroy(s.ev);
    if (s.fan_ev) (void)hipEventDestroy(s.fan_ev);
  }

  struct Run {     // state of one whole solve (sipx_parsdmm_begin / _steps)
    bool active = false, done = false;
    sipx_log* log = nullptr;
    int maxit = 0, counter = 2, i = 0;
    Tolerances<T> tol;
    RuleSwitches sw;               // what the options switch on, as the stop rule has left it
    double tol_ref = 1.0;
    bool rhs_ready = false;        // the right-hand side of the coming iteration is already queued
    std::vector<double> rho, gamma, rho_new, rpri, rdual, feas;
  };
  Run run_;
  SectionMarks marks_;
  int device_ = 0, ndim_ = 2;
  hipStream_t stream_ = nullptr;
  // device-resident boundary: the caller's stream and the two events that order it against the engine stream; whether the call
  // in progress reads device buffers; bytes of the N-sized host transfers of finalize / reset / download (sipx_io_bytes)
  hipStream_t caller_ = nullptr;
  hipEvent_t ev_io_in_ = nullptr, ev_io_out_ = nullptr;
  bool dev_io_ = false;
  mutable long long io_h2d_ = 0, io_d2h_ = 0;
  struct DevIoGuard {
    bool* f;
    explicit DevIoGuard(bool* flag) : f(flag) { *f = true; }
    ~DevIoGuard() { *f = false; }
  };
  Grid G_;
  T ih_[3];
  std::vector<SetState<T>> sets_;
  std::vector<int32_t> owned_;
  bool finalized_ = false, feasibility_only_ = false, any_ncvx_ = false;
  int p_n_ = 0, pp_n_ = 0;
  std::vector<T> rho_, gamma_;
  std::vector<double> feas_init_;
  T *p_base_ = nullptr, *m_base_ = nullptr, *r_base_ = nullptr, *p2_base_ = nullptr, *p2_ = nullptr;
  bool cg_fused_ = false;
  int n_mfree_ = 0;                   // matrix-free terms of Q (custom sparse operators passed without A'A)
  long long halo_ = 0;
  T *x_ = nullptr, *xold_ = nullptr, *rhs_ = nullptr, *m_ = nullptr, *r_ = nullptr, *p_ = nullptr, *Ap_ = nullptr;
  T *Q_ = nullptr, *scr_v_ = nullptr, *scr_c_ = nullptr, *maxpart_ = nullptr;
  long long* scr_i_ = nullptr;
  long long scr_c_len_ = 0;
  T* scr_w_ = nullptr;
  T *loose_v_ = nullptr, *loose_w_ = nullptr;    // global-indexed vectors of the materialised sets of a slab-decomposed list (finalize)
  bool loose_whole_ = false;
  bool need_idx_ = false, need_ext_ = false;
  CdsArgs cds_;
  bool set_streams_ = true;       // SIPX_SERIAL_SETS=1 keeps every set on the engine stream (A/B measurements)
  hipEvent_t ev_fork_ = nullptr, ev_fork2_ = nullptr;
  std::vector<hipStream_t> pool_;   // streams the sets are dealt onto, round robin
  bool search_streams_ = false;
  int search_next_ = 0;
  int n_set_streams_ = 2, pool_next_ = 0;   // measured: 2 beats 1 by 1-4 %, 3+ lose again at 512^3 (streaming passes collide)
  bool mk_ = false;               // Minkowski mode: unknowns [u; v]
  long long Nx_ = 0;              // number of unknowns (N, or 2N in Minkowski mode)
  T *w_base_ = nullptr, *w_ = nullptr;
  StencilQ<T> sq_{};
  bool stencil_q_ = false;
  double *part_cg_ = nullptr, *part_tmp_ = nullptr, *part_sets_ = nullptr;
  CgState<T>*cg_dev_ = nullptr, *cg_host_ = nullptr;
  double* hres_ = nullptr;
  volatile unsigned long long* sums_word_ = nullptr;   // pinned: sequence number of the latest reduction of the set sums (k_fin_sum)
  unsigned* sums_ticket_ = nullptr;
  unsigned long long sums_seq_ = 0;
  volatile int* hlean_ = nullptr;     // per set: the coming l1 search wants a sampled prediction (written by k_l1_solve)
  volatile int* hovf_ = nullptr;      // per set: the slab-decomposed search overflowed its exchange segments (k_gather_unpack)
  volatile unsigned* hverd_ = nullptr;   // per set: verdict of the speculative exchange of a slab-decomposed search (k_spec_decide)
  unsigned spec_seq_ = 0;
  long long spec_searches_ = 0, spec_fallbacks_ = 0, spec_rounds_ = 0;     // searches through the speculative exchange / of those, fallbacks / refinement rounds (all-reduces) of the fallbacks
  // the lane of the slice-rank / nuclear-norm set (sipx_finalize, lane_start)
  int lane_set_ = -1;
  hipStream_t lane_st_ = nullptr;
  hipEvent_t lane_fork_ = nullptr, lane_ev_ = nullptr;
  T* lane_v_ = nullptr;
  std::thread lane_thr_;
  std::exception_ptr lane_err_;
  long long lane_sample_ = -1;        // index of the statistics sample that books the lane's interval (-1: none open)
  SetArgs<T> lane_args_;
  bool sweep_partial_ = false, has_loose_ = false;   // the sweep takes a subset of the sets (in_sweep); some owned set keeps its per-set kernels
  bool sweep_plain_ = false;          // the sweep takes the plain iterations of this context: every set carries a third y / l pair
  bool search_batch_ = false;         // one rank + sweep: the searches of all sets as one chain of launches (batched_searches; SIPX_SEARCH_BATCH=0: per-set chains on the set streams)
  long long batch_searches_ = 0, batch_fallbacks_ = 0;
  long long routes_[RT_COUNT] = {};     // launches per route since finalize (RouteId; obs_route)
  long long project_rc_[4] = {0, 0, 0, 0};   // route counters of the rank projectors that project() built and dropped
  long long project_sc_[4] = {0, 0, 0, 0};   // ... and of the simplex projectors (calls, lane route, tile route; the segments of the last)
  long long project_l20c_[5] = {0, 0, 0, 0, 0};   // ... and of the l20 projectors (calls, small route, search route, per-frame kernel; the groups of the last)
  long long project_gc_[4] = {0, 0, 0, 0};   // ... and of the card_groups projectors (calls, small route, search route; the segments of the last)
  T* fbuf_ = nullptr;                 // fast segments: world x two-pass sets x (fcap + header)
  bool yl_multi_ = true;              // SIPX_YL_MULTI=0: never take the one-sweep y/l update (A/B switch)
  bool x0_mode_ = false;              // s_0 = A x_0 recomputed from a snapshot of x (see finalize)
  // x lives in a RING of three buffers (round 4): the x-step writes x_{k+1} = x_k + alpha_1 p_1 into a buffer that holds neither
  // x_k nor the Barzilai-Borwein snapshot x_0 and goes on in place there, so x_k stays behind untouched as x_old (the reference's
  // copy, PARSDMM.jl:128, is never made -- the residual product used to write it: 1 N w per iteration) and the snapshot of the
  // x0 mode is simply the buffer that held x on the last BB / first iteration (1 N w per BB iteration written before).
  T *xr_base_[3] = {nullptr, nullptr, nullptr}, *xr_[3] = {nullptr, nullptr, nullptr};
  int x_cur_ = 0, x_snap_ = -1;
  bool rhs_fused_ = false;            // the sweep of the latest y/l update wrote the right-hand side of the coming iteration (YlPlan::fuse_rhs)
  hipEvent_t sums_event_ = nullptr;   // the event behind which the sums of the latest y/l update are complete (unless they come by word)
  // sharded solve: communicator, this rank's slab [r0_, r1_) of the x-step, rows of Q it maintains
  std::unique_ptr<Comm> comm_;
  CountingComm* counting_ = nullptr;   // comm_ itself, with its call counters
  long long plane_ = 0, chunk_ = 0, r0_ = 0, r1_ = 0, qr0_ = 0, qr1_ = 0;
  int prev_ = -1, next_ = -1;
  hipStream_t cstream_ = nullptr;           // communication stream: the reduce-scatter of rhs runs beside the engine stream
  hipEvent_t ev_c_[2] = {nullptr, nullptr};
  bool rs_pending_ = false;
  double* dres_ = nullptr;                  // device copy of the reduced per-set sums (all-reduce buffer)
  hipEvent_t ev_sums_ = nullptr, ev_cgb_ = nullptr;
  bool sums_pending_ = false;
  T* qtab_ = nullptr;                   // class table of Q + the check's flag (build_q_table)
  bool q_stale_ = false;                // the stored bands lag the table (ensure_q_bands)
  std::string qtab_reason_ = "not built";   // why the products use the bands ("": they use the table)
  DeviceMemory mem_;                  // every device array the context keeps (the library-backed projectors own theirs)
  bool slab_dist_logs_ = false;       // slab-decomposed and a distance term among the sets: obj / evol_x sums come from its y/l update
  bool lean_multi_ = false;           // k_lean_multi for the lean first passes of the l1 searches (finalize: above 2^24 grid points; SIPX_LEAN_MULTI=0/1)
  bool head_done_ = false;            // the residual product of the coming x-step is queued already (argmin_x_head)
  int merged_nslots_ = 0;             // sums whose all-reduce the coming argmin_x_head carries (YlPlan::Route::WithNextHead)
  int sums_flags_ = 0;
  volatile unsigned long long* ticket_ = nullptr;   // pinned: verdict of the latest CG iteration (publish_ticket)
  unsigned cg_seq_ = 0;
  // slab decomposition of the whole iteration (sipx_set_decomp): the grids the set kernels are launched on, the collectives
  // of the threshold searches, the exchange buffer of their gathered magnitudes
  bool slab_req_ = false, slab_ = false;
  hipStream_t fan_st_ = nullptr;      // the stream a gathered set's owner projects on (beside the engine stream)
  hipEvent_t fan_fork_ = nullptr;
  double* fan_ptmp_ = nullptr;
  T *fan_mpart_ = nullptr, *fan_c_ = nullptr;
  long long fan_exchanges_ = 0;       // gathers + scatters of the gathered sets so far (stats)
  bool slab_loose_ = false;           // slab-decomposed with sets projected on a materialised v (SetState::slab_ext, fan)
  // slab-decomposed with SPARSE arrays: every N-sized array of the context is backed by memory for the rank's planes (and the
  // halo planes around them) only -- see DeviceMemory::alloc_sparse.  [wlo_, whi_): the grid points whose entries exist on this rank.
  bool slab_full_req_ = false, slab_local_ = false;
  // verdict of the communicator self-test of sipx_finalize ("none" without a communicator)
  std::string selftest_ = "none", mapped_why_;
  double* agree_buf_ = nullptr;
  bool selftest_mapped_failed_ = false, selftest_alltoall_failed_ = false;
  std::string a2a_why_;
  long long wlo_ = 0, whi_ = 0;
  Grid Gr_, Gyl_;
  ChainHooks hooks_;
  T* gbuf_ = nullptr;
  double *stage_ = nullptr, *sstage_ = nullptr;
  const ChainHooks* hooks() const { return slab_ ? &hooks_ : nullptr; }
  double obj_ss_ = 0, evo_ss_ = 0, xx_ss_ = 0;
  bool have_log_sums_ = false;
  hipEvent_t cg_ev_[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> stat_ev_;       // events 2 i, 2 i + 1 bracket sample i
  std::vector<KSample> samples_;
  std::vector<size_t> open_;              // samples whose closing record is still to come (launch scopes may nest)
  int stats_mode_ = 0;
  LaunchObserver obs_{this, &Engine<T>::obs_begin, &Engine<T>::obs_end, &Engine<T>::obs_route};
  std::string stats_json_;
  double stat_pair_ms_ = 0;       // elapsed time between two adjacent event records (median of 16 on the idle stream)
};

EngineBase* make_engine(int dtype, int ndim, const int64_t* n, const double* h, int device) {
  const int count = hip_device_count();
  if (device < 0 || device >= count) throw std::runtime_error("libsipx: device index out of range");
  if (dtype == SIPX_F32) return new Engine<float>(ndim, n, h, device);
  if (dtype == SIPX_F64) return new Engine<double>(ndim, n, h, device);
  throw std::runtime_error("dtype must be SIPX_F32 or SIPX_F64");
}

template <typename T>
static void cds_spmv_T(int64_t N, int d, const void* R, const int64_t* off, const void* x, void* y) {
  if (d < 1 || d > MAXD) throw std::runtime_error("cds_spmv: band count out of range");
  long long H = 4;
  for (int b = 0; b < d; ++b) H = std::max<long long>(H, std::llabs((long long)off[b]));
  H = (H + 3) / 4 * 4;
  DeviceMemory tmp;
  T* dR = tmp.alloc<T>((size_t)N * d, Mem::NoFill);
  T* dxb = tmp.alloc<T>(N + 2 * H);          // zero halo on both sides
  T* dx = dxb + H;
  T* dy = tmp.alloc<T>(N);
  SIPX_HIP(hipMemcpy(dR, R, (size_t)N * d * sizeof(T), hipMemcpyHostToDevice));
  SIPX_HIP(hipMemcpy(dx, x, N * sizeof(T), hipMemcpyHostToDevice));
  CdsArgs a;
  a.d = d;
  for (int b = 0; b < d; ++b) a.off[b] = off[b];
  Grid g;
  g.n[0] = N; g.n[1] = 1; g.n[2] = 1; g.N = N; g.st[0] = 1; g.st[1] = N; g.st[2] = N;
  K<T>::spmv(nullptr, g, N, dR, a, dx, dy);
  SIPX_HIP(hipDeviceSynchronize());
  SIPX_HIP(hipMemcpy(y, dy, N * sizeof(T), hipMemcpyDeviceToHost));
}

template <typename T>
static void resample_T(int ndim, const int64_t* nc, const int64_t* nf, const void* in, void* out) {
  long long c[3] = {1, 1, 1}, f[3] = {1, 1, 1};
  for (int q = 0; q < ndim && q < 3; ++q) { c[q] = nc[q]; f[q] = nf[q]; }
  const long long Nc = c[0] * c[1] * c[2], Nf = f[0] * f[1] * f[2];
  if (Nc < 1 || Nf < 1) throw std::runtime_error("resample: empty array");
  DeviceMemory tmp;
  T* di = tmp.alloc<T>(Nc, Mem::NoFill);
  T* dout = tmp.alloc<T>(Nf, Mem::NoFill);
  SIPX_HIP(hipMemcpy(di, in, Nc * sizeof(T), hipMemcpyHostToDevice));
  resample_nn<T>(nullptr, c, f, di, dout);
  SIPX_HIP(hipDeviceSynchronize());
  SIPX_HIP(hipMemcpy(out, dout, Nf * sizeof(T), hipMemcpyDeviceToHost));
}
void resample_nn_host(int dtype, int ndim, const int64_t* nc, const int64_t* nf, const void* in, void* out, int device) {
  hip_device_count();
  if (ndim < 1 || ndim > 3) throw std::runtime_error("resample: ndim must be 1..3");
  SIPX_HIP(hipSetDevice(device));
  if (dtype == SIPX_F32) resample_T<float>(ndim, nc, nf, in, out);
  else if (dtype == SIPX_F64) resample_T<double>(ndim, nc, nf, in, out);
  else throw std::runtime_error("dtype must be SIPX_F32 or SIPX_F64");
}

template <typename T>
static void dwt_T(int ndim, const long long* n, int inverse, const void* in, void* out) {
  const long long N = n[0] * n[1] * n[2];
  DeviceMemory tmp;
  T* di = tmp.alloc<T>(N, Mem::NoFill);
  T* dout = tmp.alloc<T>(N, Mem::NoFill);
  T* ds = tmp.alloc<T>(N, Mem::NoFill);
  SIPX_HIP(hipMemcpy(di, in, N * sizeof(T), hipMemcpyHostToDevice));
  if (inverse) dwt_inverse<T>(nullptr, ndim, n, di, dout, ds);
  else dwt_forward<T>(nullptr, ndim, n, di, dout, ds);
  SIPX_HIP(hipDeviceSynchronize());
  SIPX_HIP(hipMemcpy(out, dout, N * sizeof(T), hipMemcpyDeviceToHost));
}
void dwt_host(int dtype, int ndim, const int64_t* n, int inverse, const void* in, void* out, int device) {
  hip_device_count();
  if (ndim != 2 && ndim != 3) throw std::runtime_error("wavelet transform: ndim must be 2 or 3");
  long long nn[3] = {1, 1, 1};
  for (int q = 0; q < ndim; ++q) nn[q] = n[q];
  dwt_check_grid(ndim, nn);
  SIPX_HIP(hipSetDevice(device));
  if (dtype == SIPX_F32) dwt_T<float>(ndim, nn, inverse, in, out);
  else if (dtype == SIPX_F64) dwt_T<double>(ndim, nn, inverse, in, out);
  else throw std::runtime_error("dtype must be SIPX_F32 or SIPX_F64");
}

template <typename T>
static void prox_l2s_T(int64_t n, void* x, double rho, const void* m) {
  DeviceMemory tmp;
  T* dx = tmp.alloc<T>(n, Mem::NoFill);
  T* dm = tmp.alloc<T>(n, Mem::NoFill);
  SIPX_HIP(hipMemcpy(dx, x, n * sizeof(T), hipMemcpyHostToDevice));
  SIPX_HIP(hipMemcpy(dm, m, n * sizeof(T), hipMemcpyHostToDevice));
  prox_l2s_dev<T>(nullptr, n, dx, dm, (T)rho);
  SIPX_HIP(hipDeviceSynchronize());
  SIPX_HIP(hipMemcpy(x, dx, n * sizeof(T), hipMemcpyDeviceToHost));
}
void prox_l2s_host(int dtype, int64_t n, void* x, double rho, const void* m, int device) {
  hip_device_count();
  if (n < 1) return;
  SIPX_HIP(hipSetDevice(device));
  if (dtype == SIPX_F32) prox_l2s_T<float>(n, x, rho, m);
  else if (dtype == SIPX_F64) prox_l2s_T<double>(n, x, rho, m);
  else throw std::runtime_error("dtype must be SIPX_F32 or SIPX_F64");
}

void cds_spmv_host(int dtype, int64_t N, int d, const void* R, const int64_t* off, const void* x, void* y, int device) {
  hip_device_count();
  SIPX_HIP(hipSetDevice(device));
  if (dtype == SIPX_F32) cds_spmv_T<float>(N, d, R, off, x, y);
  else if (dtype == SIPX_F64) cds_spmv_T<double>(N, d, R, off, x, y);
  else throw std::runtime_error("dtype must be SIPX_F32 or SIPX_F64");
}

}  // namespace sipx
