// dfh_handles.h — what the library's three handles hold (dfh_ctx, dfh_table, dfh_batch), the thread's error text and the
// event bracket of the timed kernel classes.  Every file after it in dfh_api.hip's list reads these fields; the types of the
// views inside them come from the kernel files before it.
namespace dfh {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace dfh

// --------------------------------------------------------------------- handles
struct dfh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // preparation streams (copies, Localizer, key lookup): with pipelining on, the batches being
  // prepared take them round-robin while an earlier batch trains on `stream`
  std::vector<hipStream_t> preps;
  std::vector<hipStream_t> extra;  // other streams that carry work on this context's tables (a shard's collectives stream): drained by sync_all
  hipStream_t parse = nullptr;     // the device text parse (dfh_textparse.hip): one stream for all of a context's chunks, created with the first
  std::mutex parse_mu;
  unsigned nprep = 0;       // streams in use (0: pipelining off, everything on `stream`)
  unsigned next_prep = 0;
  bool pipeline = false;
  // monotonic scratch for the literal (host-pointer) calls
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  int num_cu = 256;
  // launch tuning (dfh_ctx_set_option); the defaults are the measured optima for C3 on MI355X
  int fwd_depth = 5;           // independent V-row loads a forward lane issues before consuming any
  int fwd_blocks = 0;          // cap on the forward grid (0: one wave per example)
  int bwd_small_blocks = 2048; // cap on the short-segment blocks of the backward/update launch
  // k_update_fused (fused update on the resident table): 1 = on (default), 0 = k_backward_all's fused form;
  // caps on the blocks of its four roles
  int upd_kernel = 1;
  // (C3 on MI355X, profiles/r03_update_roles.txt: alone, hot needs >= 1024 blocks to reach 17 us, mid 1024 for 16 us,
  // few 1024 for 20 us, the singles 37 us from 1280 blocks on; together 512 / 512 / 1024, list roles first, is the best
  // found: 58.7 us; more list blocks cost more in block dispatch than they save in chain length)
  int upd_hot_blocks = 512, upd_mid_blocks = 512, upd_few_blocks = 1024, upd_single_blocks = 4096;
  int upd_interleave = 0;      // n > 1: every n-th block of the launch is a list-role block; 0 / 1: list roles first
  int owner_per_key = 0;       // sharded store, owner side per distinct key in two launches (1) or per received entry in three (0); env DFH_OWNER_PER_KEY=1 sets the default
  int upd_split = 1;           // keys with more than HOT_SPLIT occurrences part by part, a block per part (0: the hot role walks them whole; A/B)
  int auc_in_update = 1;       // a training step's AUC as the first blocks of k_update_fused (1) or a launch of its own (0)
  int shard_mixed_update = 1;  // sharded step: one k_update_fused<MIXED> launch for own + others' keys (1) or round 4's two launches (0)
  int grow_initial_rows = 1 << 20;  // first allocation of a growing table (dfh_table_create with capacity_rows = 0)
  // cross-stream events without the system-scope fence (no L2 write-back / invalidate at the record): every
  // consumer of these events is a stream of this device
  int event_flags = 1;
  int prep_priority = -1;      // preparation streams: -1 lowest, 0 default, 1 highest stream priority
  // The single-queue step (dfh_riders.hip): no preparation stream.  dfh_localize on a batch object only NOTES the work
  // (pend, in call order); the stages of the sample sort then ride, one per launch and minibatch, as extra blocks of the
  // launches later steps make on the main stream — stage s in the launch of kind rider_slot[s] (0 = the step's lookup pass,
  // 1 = forward, 2 = update); rider_alone[s]: as a launch of its own just before that launch instead (A/B).  A consumer that
  // needs a minibatch before its stages have all found a carrier runs the rest as plain launches (flush_pending).
  int single_queue = 0;
  int rider_slot[4] = {2, 0, 1, 2};     // count, scatter, sort, emit
  int rider_alone[4] = {0, 0, 0, 0};
  int rider_period[3] = {1, 1, 1};      // L, F, U: one group of 8 rider blocks every n groups of 8 blocks (1: riders first — the best measured, profiles/r06a_*)
  int rider_start[3] = {0, 0, 0};       // L, F, U: per cent of the carrier's own blocks dispatched before the first rider group
  std::vector<dfh_batch*> pend;
  // The library's code object (8 MB, a few hundred kernel instantiations) is loaded by the runtime on the FIRST launch of any
  // of its kernels: 30-40 ms that used to fall into a job's first minibatch (build/difacto: the first dfh_batch_prepare_rows
  // took 32-42 ms, profiles/r05e_e2e_startup.txt).  A helper thread makes that first launch while the caller goes on to
  // allocate its model table; joined when the context is destroyed.
  std::thread warm;

  // optional per-kernel HIP-event timing (dfh_ctx_set_timing)
  uint32_t timing = 0;  // bit i: time kernel id i
  struct Span { int id; hipEvent_t a, b; int ride = 0; };  // ride: the events travel on the dispatch itself (main stream)
  std::vector<Span> spans;
  std::vector<hipEvent_t> pool;
  double t_ms[DFH_K_COUNT] = {0};
  uint64_t t_calls[DFH_K_COUNT] = {0};
};

namespace {
// brackets the launches of one logical kernel with HIP events on the ctx stream
struct TimeScope {
  dfh_ctx* c;
  int id;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  static hipEvent_t get(dfh_ctx* c) {
    if (!c->pool.empty()) {
      hipEvent_t e = c->pool.back();
      c->pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  TimeScope(dfh_ctx* ctx, int kid, hipStream_t s = nullptr) : c(ctx), id(kid), st(s ? s : ctx->stream) {
    if (kid >= DFH_K_COUNT || !((c->timing >> kid) & 1u)) return;
    a = get(c);
    b = get(c);
    if (a && b) (void)hipEventRecord(a, st);
  }
  ~TimeScope() {
    if (!a || !b) return;
    (void)hipEventRecord(b, st);
    c->spans.push_back({id, a, b});
  }
};
}  // namespace

struct dfh_table {
  dfh_ctx* ctx = nullptr;
  TableView v{};
  uint64_t hslots = 0;
  uint64_t bytes = 0;
  bool has_aux = true;  // SGDUpdater::has_aux_ (sgd_updater.h:80): false after loading a model saved without optimiser state
  // capacity_rows = 0 at creation: the table GROWS like the reference's unordered_map (sgd_updater.h:78).  rows_bound is a
  // host-side upper bound of the rows allocated so far (every launch that may insert adds the keys it carries); when it
  // reaches the capacity the true count is read back and, if the headroom is short, the arrays are re-allocated.
  bool auto_grow = false;
  uint64_t rows_bound = 0;
  uint64_t grows = 0;
  // REFRAND scratch (need/rank/urow per pushed key) for the literal + shard calls
  uint32_t* d_need = nullptr;
  uint32_t* d_rank = nullptr;
  uint32_t* d_urow = nullptr;
  uint32_t* d_total = nullptr;
  size_t aux_cap = 0;
};

struct dfh_batch {
  dfh_ctx* ctx = nullptr;
  size_t max_rows = 0, max_nnz = 0;
  size_t nrows = 0, nnz = 0;
  bool has_value = false;
  bool has_cnt = false;
  bool localized = false;
  // raw input: own buffers (o_*), or caller-owned device memory attached without a copy
  uint64_t* d_raw = nullptr;
  uint32_t* d_offset = nullptr;
  float* d_value = nullptr;
  float* d_label = nullptr;
  void* arena = nullptr;     // the one device allocation the object's arrays are carved from (dfh_batch_create)
  void* shared_arena = nullptr;  // SharedArena*: dfh_batch_create_many
  size_t arena_bytes = 0;
  uint64_t* o_raw = nullptr;
  uint32_t* o_offset = nullptr;
  float* o_value = nullptr;
  float* o_label = nullptr;
  // pinned staging of dfh_batch_load_host and of the device feed (one block, laid out by `stage`), allocated on first use
  StageLayout stage;
  char* h_stage = nullptr;
  size_t stage_bytes = 0;          // allocated size of h_stage (ensure_stage: the row-description paths need ~160 KB, load_host the whole batch)
  hipEvent_t ev_staged = nullptr;  // the copies out of h_stage (or the kernels that read it in place) have completed
  bool staged_pending = false;
  double t_prof[6] = {0, 0, 0, 0, 0, 0};  // DFH_PROFILE_PREP: host seconds inside dfh_batch_prepare_rows, by section
  uint64_t n_prof = 0;
  char* d_stage_view = nullptr;    // h_stage as the device sees it (dfh_batch_prepare_rows: the gather reads it in place)
  bool defer_ready = false;        // inside a combined preparation call: the intermediate phases do not record ev_ready
  // localizer workspace
  uint64_t *d_keys = nullptr, *d_skeys = nullptr;   // bucket-major / sorted keys
  uint32_t *d_pos = nullptr, *d_spos = nullptr;     // row of every nnz position (d_pos) / sorted positions
  uint32_t *d_bpos = nullptr;                       // bucket-major positions
  uint32_t *d_head = nullptr, *d_uid = nullptr;     // library-sort path only
  void* d_temp = nullptr;
  size_t temp_bytes = 0;
  // sample-sort localizer: bootstrap samples, persistent splitters, per-call bucket bookkeeping
  uint64_t *d_smp_key = nullptr, *d_spl_key = nullptr, *d_first_key = nullptr, *d_last_key = nullptr;
  uint32_t *d_smp_rank = nullptr, *d_smp_pos = nullptr, *d_spl_pos = nullptr, *d_packed = nullptr, *d_run_off = nullptr,
           *d_bstart = nullptr, *d_btotal = nullptr, *d_nheads = nullptr, *d_lh = nullptr;
  size_t max_tiles = 0;
  int spl_P = 0;                   // number of buckets the stored splitters partition into (0: none yet)
  // localized view
  uint64_t* d_feaids = nullptr;
  float* d_feacnt = nullptr;
  uint32_t *d_col_ptr = nullptr, *d_index = nullptr, *d_s_row = nullptr;
  float* d_s_val = nullptr;
  uint32_t* d_U = nullptr;
  // step workspace
  // long-segment key lists for the backward pass (SegLists): list buckets = sort buckets
  uint2 *d_mid = nullptr, *d_hot = nullptr, *d_few = nullptr;  // [list buckets] {cnt, off}
  SegEnt *d_mid_ent = nullptr, *d_hot_ent = nullptr, *d_few_ent = nullptr;
  // the parts of the keys with more than HOT_SPLIT_MIN occurrences (SegLists::split_ent), their partial sums and tickets
  SegEnt* d_split_ent = nullptr;
  uint32_t* d_split_ticket = nullptr;
  float* d_split_part = nullptr;
  size_t split_cap = 0;
  // the list's two counters, d_U + 2 + {0, 1} (SplitOut): split_sel = the one the next listing step appends to (zero by then),
  // split_last = the one the last listing step filled; split_listing: a launch of the running step has taken the list
  int split_sel = 0, split_last = 0;
  bool split_listing = false;
  uint32_t seg_nb = 0;                              // list buckets of the current localized view
  uint32_t view_P = 0;                              // ... which came out of the sample sort with this many buckets (d_bstart); 0: not
  size_t few_cap = 0, mid_cap = 0, hot_cap = 0;     // entries d_few_ent / d_mid_ent / d_hot_ent hold (dfh_batch_get_key_view)
  uint2* d_uw = nullptr;          // {table row, w} per unique key, written by the step's k_lookup
  uint32_t *d_urow = nullptr, *d_need = nullptr, *d_rank = nullptr, *d_total = nullptr;
  float *d_pred = nullptr, *d_slope = nullptr, *d_xv = nullptr;
  size_t xv_floats = 0;
  static constexpr size_t kProgDoubles = 2 * PROG_SLOTS + 64;   // [2][PROG_SLOTS] partials, then the AUC accumulator
  double* d_prog = nullptr;        // [kProgDoubles]
  float nrows_seen = 0;
  // pipelining: prep-stream work -> ev_ready -> main-stream step -> ev_free -> next prep
  hipEvent_t ev_ready = nullptr, ev_free = nullptr;
  bool ready_pending = false, free_pending = false;
  hipStream_t prep = nullptr;      // stream of the current preparation phase (load .. localize .. lookup)
  bool compute_auc = false;        // dfh_sgd_step also accumulates BinClassMetric::AUC per batch
  uint32_t *d_auc_keys = nullptr, *d_auc_skeys = nullptr, *d_auc_lab = nullptr, *d_auc_slab = nullptr;
  uint32_t* d_auc_part = nullptr;  // auc_pairs_block: one count per unit + the positives per row tile
  uint32_t auc_pending_n = 0;      // examples of the AUC whose units have been queued but not finalised (0: none)
  bool force_radix = false;        // tests: take the library-sort path of dfh_localize
  bool force_sort_fallback = false;  // tests: k_ss_sort's global-memory path for every bucket
  dfh_table* looked_up = nullptr;  // dfh_batch_lookup already resolved urow against this table
  // device feed: a minibatch DESCRIBED by dfh_batch_prepare_rows whose rows are still in their row buffers: gathered by the
  // Localizer's count pass itself (k_loc_count_gather) or, where that pass cannot (first call of a size class, the large size
  // class, the library sort, a tile spanning too many rows, more than four buffers), by k_gather_rows_staged first
  struct GatherSeg { struct dfh_rowbuf* rb; size_t at, n; };
  std::vector<GatherSeg> gsegs;
  GatherSrc gsrc{};
  bool gather_pending = false, gather_fusable = false, gather_any_value = false, loc_fuse_gather = false;
  const uint32_t *g_rows = nullptr, *g_off = nullptr;   // the description as the device sees it (mapped host memory)
  const float* g_lab = nullptr;
  // single-queue step: the sample sort of the loaded minibatch as noted by dfh_localize (arguments of its four stages) and the
  // first stage that has not been queued yet (RID_STAGES: nothing pending)
  LocView loc_v{};
  EmitOut loc_o{};
  uint32_t loc_gsort = 0;
  bool loc_big = false;
  int pend_stage = RID_STAGES;
};

namespace dfh::chunks {
inline hipError_t reset_prog(dfh_batch* b, hipStream_t s) {   // d_prog back to zero
  return hipMemsetAsync(b->d_prog, 0, dfh_batch::kProgDoubles * sizeof(double), s);
}
}  // namespace dfh::chunks

namespace {
// dfh_localize_api.hip; it queues the gather of dfh_feed.hip, whose prepare calls run it: the one cycle among the files
int localize_impl(dfh_batch* b, uint64_t max_index, dfh_table* probe);
}  // namespace
