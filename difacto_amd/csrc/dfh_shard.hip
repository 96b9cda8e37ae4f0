// Multi-GPU store: the model row-sharded by key range over the ranks of one node, one process per
// GPU, behind the C ABI (include/difacto_hip.h, "sharded store").  Replaces the ps-lite Push / Pull
// of src/store (include/difacto/store.h:53-93): every rank is a worker (it trains its own
// minibatches) and a server (it owns a contiguous range of the reversed keys — what ReverseBytes is
// for, include/difacto/base.h:29-38).  Because the Localizer emits a minibatch's keys in ascending
// order (src/data/localizer.cc:28-48) every owner's keys are one contiguous slice: send buffers need
// no permutation.
//
// One dfh_shard_step = the batch executor of SGDLearner::IterateData (sgd_learner.cc:131-178) with
// the store calls turned into one exchange each way:
//     counts   every rank learns how many keys each peer sends it (+ "I still have data")
//     L        the keys THIS rank owns never leave it: k_lookup on its own table (row ids, Push(kFeaCount))
//     K        the other keys (+ epoch-0 counts) --alltoallv--> owners
//     R        owners: resolve keys -> rows once, Push(kFeaCount) per source, Pull (one gather)
//     RW       rows --alltoallv--> workers          fixed stride dfh_row_stride(V_dim)
//     F        FMLoss::Predict / Evaluate on a mixed source: own keys read the table in place, the others
//              the pulled rows (k_forward<MIXED>); CalcGrad and the update in ONE launch of k_update_fused<MIXED>:
//              gradient rows for the others' keys, the in-place update for the own ones (ctx option
//              shard_mixed_update = 0: a launch each, the others' gradient rows first)
//     G        gradients --alltoallv--> owners
//     P        owners: Push(kGradient) of the other sources, applied in ascending rank order in ONE launch
// A key's pushes are applied owner first, then the other sources in ascending rank order — one legal
// execution of the reference's asynchronous Push protocol, the same on every run.  With one rank
// nothing is exchanged and nothing waits for the host.  L and F are step_lookup and step_math (dfh_step.hip), the two
// worker stages dfh_sgd_step is made of as well: with one rank both steps queue the same launches.
// Every stage is one function of the minibatch's Flight (flight_L, flight_K, flight_R, flight_RW, flight_F, flight_G,
// flight_P); the two exchange modes are two schedules over them: shard_step_sync (every stage on the context's stream, one
// minibatch at a time in exchange slot 0) and shard_step_overlap (K, RW, G on a collectives' stream, two minibatches in
// flight in alternating slots, events between the stages).
// Zero staleness: every minibatch reads the model all earlier ones have updated.  No all-reduce:
// the traffic is key-routed rows, an all-to-all that uses every xGMI link of a GPU at once.  Transport: dfh_comm (dfh_comm.hip).
#ifndef DFH_SHARD_HIP_
#define DFH_SHARD_HIP_
#include <optional>

namespace dfh {

// per-destination {keys I send you, do I still have data} -> device words for the counts exchange
__global__ void k_shard_counts(const int64_t* __restrict__ bounds, int world, int64_t has_data, int64_t* __restrict__ out) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < world) {
    out[2 * d] = bounds ? bounds[d + 1] - bounds[d] : 0;
    out[2 * d + 1] = has_data;
  }
}

}  // namespace dfh

using namespace dfh;

struct dfh_shard {
  dfh_table* t = nullptr;
  dfh_comm* c = nullptr;
  uint64_t* d_splits = nullptr;         // [world-1] first keys of shards 1.. (NULL: uniform ranges)
  std::vector<uint64_t> h_splits;       // the same on the host, uniform ranges spelled out
  int64_t* d_bounds = nullptr;          // [world+1]
  int64_t* d_cnt = nullptr;             // [2][2*world]: what I send every peer / what every peer sends me
  int64_t* h_cnt = nullptr;             // pinned copy
  // Two sets of exchange buffers (slots): the sync schedule uses set 0 and so do the literal host calls; the overlap
  // schedule (two minibatches in flight) alternates, one set per minibatch under way.  Sized by slot_bufs alone.
  // owner side, sized to the keys received in a step
  uint64_t* r_keys[2] = {nullptr, nullptr};
  float* r_cnt[2] = {nullptr, nullptr};
  uint32_t* r_rowid[2] = {nullptr, nullptr};
  float* r_rows[2] = {nullptr, nullptr};   // rows out, then gradients in
  size_t r_cap[2] = {0, 0};
  // worker side, sized to the batch's unique keys
  float* w_rows[2] = {nullptr, nullptr};
  size_t w_cap[2] = {0, 0};
  float* w_grads[2] = {nullptr, nullptr};
  size_t g_cap[2] = {0, 0};
  std::vector<size_t> xsb, xrb, xso;    // bytes per peer of the exchange being queued (flight_bytes)
  uint64_t steps = 0;
  // counts of the FOLLOWING step, exchanged inside the current one (dfh_shard_prefetch_counts)
  dfh_batch* next_b = nullptr;
  bool next_armed = false;            // the next dfh_shard_step issues the counts exchange of next_b
  bool counts_ready = false;          // h_cnt holds the counts of counts_for; cnt_ev marks their arrival
  dfh_batch* counts_for = nullptr;
  hipEvent_t cnt_ev = nullptr;
  // ---- overlapped exchange (dfh_shard_set_exchange(s, 1)): two minibatches in flight
  int exchange = 0;                   // 0: sync (one minibatch at a time, zero staleness), 1: overlap (staleness <= 1)
  hipStream_t cs = nullptr;           // the collectives' own stream (the sync step exchanges on the context's stream)
  hipEvent_t ev_k[2] = {nullptr, nullptr}, ev_r[2] = {nullptr, nullptr}, ev_rw[2] = {nullptr, nullptr};
  hipEvent_t ev_f = nullptr, ev_g = nullptr;
  hipEvent_t ev_m = nullptr;          // the main stream up to a minibatch's Localizer, where no preparation stream ran it (cs_behind_prep)
  // P (or the release) of the minibatch that last used exchange slot q has been queued and recorded: the next K into
  // r_keys[q] / r_cnt[q] waits for it (P reads r_keys / r_rowid / r_rows on the main stream; K writes on the collectives')
  hipEvent_t ev_p[2] = {nullptr, nullptr};
  bool p_pending[2] = {false, false};
  struct Flight {                     // one minibatch on its way through the stages (flight_L ... flight_P)
    dfh_batch* b = nullptr;           // NULL: this rank has no minibatch in that step (it still serves its shard)
    bool described = false;           // the counts exchange is through: the sizes below are valid
    bool pulled = false;              // K, R, RW are queued: the other owners' rows are on their way to w_rows[slot]
    bool have = false;
    std::vector<size_t> send, recv, seg, off;
    size_t nrecv = 0, U = 0, active = 0;
    uint32_t own_lo = 0, own_hi = 0xFFFFFFFFu;
    bool any_own = false, any_remote = false;
    int slot = 0;
    bool listed = false;              // R left the key lists of the per-key owner side: P runs over them
  } fl[2];
  // overlap: fl[cur] is the minibatch the next step trains, fl[cur ^ 1] the one after.  The sync schedule describes its one
  // minibatch in fl[0] and never marks it pulled.
  int cur = 0;
  // ---- per-stage timing (dfh_shard_set_timing): counts, L, K, R, RW, F, G, P
  bool timing = false;
  struct Span { int id; hipEvent_t a, b; };
  std::vector<Span> spans;
  std::vector<hipEvent_t> ev_pool;
  double stage_ms[DFH_SHARD_STAGES] = {0};
  uint64_t stage_steps = 0;
};

namespace {

template <typename T>
int grow(T** p, size_t n, hipStream_t sync_stream) {
  if (*p) {
    DFH_HIP(hipStreamSynchronize(sync_stream));
    DFH_HIP(hipFree(*p));
    *p = nullptr;
  }
  DFH_HIP(hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(n, 1) * sizeof(T)));
  return DFH_OK;
}

}  // namespace

extern "C" {

int dfh_shard_balanced_splits(dfh_comm* c, const uint64_t* sample_keys, size_t n, uint64_t* splits) {
  DFH_ARG(c && splits && (n == 0 || sample_keys), "dfh_shard_balanced_splits: NULL argument");
  const int W = c->world;
  if (W == 1) return DFH_OK;
  // a fixed-size message per rank: {count, keys[S]} — S evenly spaced keys of the rank's sorted sample
  constexpr size_t S = 2048;
  std::vector<uint64_t> mine(sample_keys, sample_keys + n);
  std::sort(mine.begin(), mine.end());
  std::vector<uint64_t> msg(1 + S, 0), all((size_t)W * (1 + S));
  const size_t take = std::min(S, mine.size());
  msg[0] = take;
  for (size_t i = 0; i < take; ++i) msg[1 + i] = mine[(i * mine.size()) / take];
  int rc = dfh_comm_allgather(c, msg.data(), msg.size() * sizeof(uint64_t), all.data());
  if (rc) return rc;
  std::vector<uint64_t> uni;
  for (int p = 0; p < W; ++p) {
    const uint64_t* m = &all[(size_t)p * (1 + S)];
    DFH_ARG(m[0] <= S, "dfh_shard_balanced_splits: corrupt sample message");
    uni.insert(uni.end(), m + 1, m + 1 + m[0]);
  }
  std::sort(uni.begin(), uni.end());
  const uint64_t span = (~0ULL / (uint64_t)W) + 1;
  for (int d = 1; d < W; ++d) {
    // the first key of shard d: the d/W quantile of the union (ascending by construction); no sample at all: uniform
    splits[d - 1] = uni.empty() ? (uint64_t)d * span : uni[((size_t)d * uni.size()) / W];
  }
  return DFH_OK;
}

int dfh_shard_create(dfh_table* t, dfh_comm* c, const uint64_t* splits, dfh_shard** out) {
  DFH_ARG(t && c && out && t->ctx == c->ctx, "dfh_shard_create: table and communicator must share a context");
  if (!(t->v.p.init_mode == DFH_INIT_HASH || t->v.k == 0)) {
    set_error("the sharded store needs V_init = hash (the rand_r chain of the reference depends on the global order of allocations)");
    return DFH_ERR_STATE;
  }
  const int W = c->world;
  for (int d = 1; splits && d < W - 1; ++d) DFH_ARG(splits[d] >= splits[d - 1], "splits must be ascending");
  DFH_HIP(hipSetDevice(t->ctx->device));
  dfh_shard* s = new (std::nothrow) dfh_shard();
  DFH_ARG(s != nullptr, "out of host memory");
  s->t = t;
  s->c = c;
  hipStream_t st = t->ctx->stream;
  {
    const uint64_t span = W == 1 ? ~0ULL : (~0ULL / (uint64_t)W) + 1;
    for (int d = 1; d < W; ++d) s->h_splits.push_back(splits ? splits[d - 1] : (uint64_t)d * span);
  }
  if (splits && W > 1) {
    DFH_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_splits), (W - 1) * sizeof(uint64_t)));
    DFH_HIP(hipMemcpyAsync(s->d_splits, splits, (W - 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  DFH_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_bounds), (W + 1) * sizeof(int64_t)));
  DFH_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_cnt), 4 * (size_t)W * sizeof(int64_t)));
  DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->h_cnt), 4 * (size_t)W * sizeof(int64_t), hipHostMallocDefault));
  DFH_HIP(hipEventCreateWithFlags(&s->cnt_ev, hipEventDisableTiming));
  DFH_HIP(hipStreamSynchronize(st));
  *out = s;
  return DFH_OK;
}

int dfh_shard_destroy(dfh_shard* s) {
  if (!s) return DFH_OK;
  hipSetDevice(s->t->ctx->device);
  sync_all(s->t->ctx);
  void* ptrs[] = {s->d_splits, s->d_bounds, s->d_cnt, s->r_keys[0], s->r_cnt[0], s->r_rowid[0], s->r_rows[0], s->w_rows[0], s->w_grads[0], s->w_grads[1],
                  s->r_keys[1], s->r_cnt[1], s->r_rowid[1], s->r_rows[1], s->w_rows[1]};
  for (void* p : ptrs)
    if (p) hipFree(p);
  if (s->h_cnt) hipHostFree(s->h_cnt);
  if (s->cnt_ev) hipEventDestroy(s->cnt_ev);
  for (hipEvent_t e : {s->ev_k[0], s->ev_k[1], s->ev_r[0], s->ev_r[1], s->ev_rw[0], s->ev_rw[1], s->ev_f, s->ev_g, s->ev_m, s->ev_p[0], s->ev_p[1]})
    if (e) hipEventDestroy(e);
  for (auto& sp : s->spans) {
    hipEventDestroy(sp.a);
    hipEventDestroy(sp.b);
  }
  for (hipEvent_t e : s->ev_pool) hipEventDestroy(e);
  if (s->cs) {
    auto& ex = s->c->ctx->extra;
    ex.erase(std::remove(ex.begin(), ex.end(), s->cs), ex.end());
    hipStreamDestroy(s->cs);
  }
  delete s;
  return DFH_OK;
}

int dfh_shard_owned_range(dfh_shard* s, const uint64_t* splits, uint64_t* key_lo, uint64_t* key_hi) {
  DFH_ARG(s && key_lo && key_hi, "NULL argument");
  const int W = s->c->world, r = s->c->rank;
  const uint64_t span = W == 1 ? ~0ULL : (~0ULL / (uint64_t)W) + 1;
  *key_lo = r == 0 ? 0 : (splits ? splits[r - 1] : (uint64_t)r * span);
  *key_hi = r == W - 1 ? 0 : (splits ? splits[r] : (uint64_t)(r + 1) * span);  // 0: no upper bound
  return DFH_OK;
}

}  // extern "C"

namespace {
using Flight = dfh_shard::Flight;

// queue, on the main stream: owner ranges of b's keys -> {keys for every owner, "I have a minibatch"} ->
// every peer -> pinned host memory
int queue_counts(dfh_shard* s, dfh_batch* b, hipStream_t on = nullptr) {
  dfh_comm* c = s->c;
  hipStream_t st = on ? on : c->ctx->stream;
  const int W = c->world;
  const bool have = b != nullptr && b->nnz > 0;
  if (have) {
    const uint64_t span = (~0ULL / (uint64_t)W) + 1;
    hipLaunchKernelGGL(k_key_ranges64, dim3((W + 256) / 256), dim3(256), 0, st, b->d_feaids, b->d_U, W, span, s->d_splits,
                       s->d_bounds, 0u);
  }
  hipLaunchKernelGGL(k_shard_counts, dim3(1), dim3(64), 0, st, have ? s->d_bounds : (const int64_t*)nullptr, W,
                     (int64_t)(b != nullptr ? 1 : 0), s->d_cnt);
  DFH_HIP(hipGetLastError());
  std::vector<size_t> cb(W, 2 * sizeof(int64_t));
  int rc = comm_alltoallv(c, s->d_cnt, cb.data(), s->d_cnt + 2 * W, cb.data(), st, DFH_XCHG_COUNTS);
  if (rc) return rc;
  DFH_HIP(hipMemcpyAsync(s->h_cnt, s->d_cnt, 4 * (size_t)W * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  return DFH_OK;
}

// brackets one stage of a step with two events on `st` when per-stage timing is on
struct StageScope {
  dfh_shard* s;
  int id;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  static hipEvent_t get(dfh_shard* s) {
    if (!s->ev_pool.empty()) {
      hipEvent_t e = s->ev_pool.back();
      s->ev_pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
  }
  StageScope(dfh_shard* sh, int stage, hipStream_t stream) : s(sh), id(stage), st(stream) {
    if (!s->timing) return;
    a = get(s);
    b = get(s);
    if (a && b) (void)hipEventRecord(a, st);
  }
  ~StageScope() {
    if (!a || !b) return;
    (void)hipEventRecord(b, st);
    s->spans.push_back({id, a, b});
  }
};

// ---- The stages of a step (the table in the header of this file), each written once as a function of the minibatch's
// Flight.  dfh_shard_step is one of two SCHEDULES over them, shard_step_sync and shard_step_overlap: a schedule decides
// whether a stage runs, on which stream an exchange (K, RW, G) is queued — L, R, F and P launch the table's and the batch's
// kernels, which run on the context's stream — and which events order the stages.  The events are the overlap schedule's:
// a stage waits for the ones it is handed inside its timing bracket, before its work, and records `done` behind it; the
// sync schedule hands none.
// The list of the very hot keys' parts for the update's split role (split_out, dfh_phases.hip) is filled by the launches of a
// training step that see the minibatch's keys — the own keys' lookup (L, ranks offset by own_lo) and the others' row words
// (k_uw_remote in F, or folded into L), BOTH appending to the one counter the batch object's previous step left at zero (SplitOut).
inline int wait_on(hipStream_t st, hipEvent_t e) {
  if (e) DFH_HIP(hipStreamWaitEvent(st, e, 0));
  return DFH_OK;
}
inline int record_on(hipStream_t st, hipEvent_t e) {
  if (e) DFH_HIP(hipEventRecord(e, st));
  return DFH_OK;
}

// sizes of a minibatch's exchange from the counts that have arrived in h_cnt
void flight_sizes(dfh_shard* s, Flight& f, dfh_batch* b, int slot) {
  const int W = s->c->world, me = s->c->rank;
  f.b = b;
  f.have = b != nullptr && b->nnz > 0;
  f.send.assign(W, 0);
  f.recv.assign(W, 0);
  f.seg.assign(W + 1, 0);
  f.off.assign(W + 1, 0);
  f.active = 0;
  f.nrecv = 0;
  if (W == 1) {
    // one rank: there are no counts.  Every key is its own, and how many there are stays on the device (b->d_U): the
    // own range is open-ended (the kernels clamp to *d_U) and U is not known here
    f.active = b != nullptr ? 1 : 0;
    f.own_lo = 0;
    f.own_hi = 0xFFFFFFFFu;
  } else {
    for (int p = 0; p < W; ++p) {
      f.send[p] = (size_t)s->h_cnt[2 * p];
      f.recv[p] = (size_t)s->h_cnt[2 * W + 2 * p];
      f.active += s->h_cnt[2 * W + 2 * p + 1] != 0 ? 1 : 0;
      f.off[p + 1] = f.off[p] + f.send[p];  // owner p's keys are ranks [off[p], off[p+1]) of the minibatch's key list
    }
    f.own_lo = (uint32_t)f.off[me];
    f.own_hi = (uint32_t)f.off[me + 1];
    f.send[me] = f.recv[me] = 0;  // the rank's own keys are not exchanged
    for (int p = 0; p < W; ++p) {
      f.nrecv += f.recv[p];
      f.seg[p + 1] = f.seg[p] + f.recv[p];
    }
  }
  f.U = f.off[W];
  f.any_own = f.have && f.own_hi > f.own_lo;
  f.any_remote = f.have && (f.own_lo > 0 || (size_t)f.own_hi < f.U);
  f.described = true;
  f.pulled = false;
  f.slot = slot;
}

// The one place a slot's exchange buffers are sized: the owner side for r_need received keys, the worker side for the
// pulled rows of w_need keys and the gradient rows of g_need keys (0: not needed).  slack: the growth policy of a step,
// 1.5x + 1024 (dfh_shard_reserve asks for exact sizes).  Growing waits for everything queued on every stream: rare.
int slot_bufs(dfh_shard* s, int q, size_t r_need, size_t w_need, size_t g_need, bool slack) {
  if (r_need <= s->r_cap[q] && w_need <= s->w_cap[q] && g_need <= s->g_cap[q]) return DFH_OK;
  hipStream_t st = s->t->ctx->stream;
  const size_t stride = dfh_row_stride(s->t->v.k);
  int rc = sync_all(s->t->ctx);  // (the collectives' stream is one of the context's extra streams)
  if (rc) return rc;
  auto cap_for = [slack](size_t n) { return slack ? n + n / 2 + 1024 : n; };
  if (r_need > s->r_cap[q]) {
    const size_t cap = cap_for(r_need);
    if ((rc = grow(&s->r_keys[q], cap, st)) || (rc = grow(&s->r_cnt[q], cap, st)) || (rc = grow(&s->r_rowid[q], multi_words(cap, s->c->world), st)) ||
        (rc = grow(&s->r_rows[q], cap * stride, st)))
      return rc;
    s->r_cap[q] = cap;
  }
  if (w_need > s->w_cap[q]) {
    const size_t cap = cap_for(w_need);
    if ((rc = grow(&s->w_rows[q], cap * stride, st))) return rc;
    s->w_cap[q] = cap;
  }
  if (g_need > s->g_cap[q]) {
    const size_t cap = cap_for(g_need);
    if ((rc = grow(&s->w_grads[q], cap * stride, st))) return rc;
    s->g_cap[q] = cap;
  }
  return DFH_OK;
}

// the exchange buffers of a flight's slot
int flight_bufs(dfh_shard* s, const Flight& f) {
  const size_t w = f.any_remote ? f.U : 0;
  return slot_bufs(s, f.slot, f.nrecv, w, w, true);
}

// bytes per peer of one exchange of f at `unit` bytes per key, into the shard's lists (comm_exchange has read them when it
// returns)
void flight_bytes(dfh_shard* s, const Flight& f, size_t unit) {
  const int W = s->c->world;
  s->xsb.resize(W);
  s->xrb.resize(W);
  s->xso.resize(W);
  for (int p = 0; p < W; ++p) {
    s->xsb[p] = f.send[p] * unit;
    s->xrb[p] = f.recv[p] * unit;
    s->xso[p] = f.off[p] * unit;  // worker-side buffers are indexed by the key's rank u: owner p's slice starts at off[p]
  }
}

// ctx option "owner_per_key" (DFH_OWNER_PER_KEY=1 sets its default; measurement): the owner side per DISTINCT key in two launches (dfh_shard_count_pull_multi,
// dfh_shard_push_grad_listed) instead of per received entry in three.  Built in round 6 on VERDICT r5 #2, bit-identical
// (tests/test_gpu_parity.py "listed"), and NOT faster: 101 against 98 us for the owner side of an N = 8 step
// (profiles/r06o_owner_side_per_key.txt) — the default stays per entry.
bool owner_per_entry(const dfh_table* t) { return !t->ctx->owner_per_key; }

// L: this rank's own keys: rows + Push(kFeaCount) on its own table, {row, w} per key for the forward (step_lookup on
// [own_lo, own_hi)).  rows_in: the rows of the other owners are already on their way (the overlap schedule, every step but
// an epoch's first) — the launch waits for them and writes the row words of the others' keys too (F is then told uw_done)
int flight_L(dfh_shard* s, Flight& f, int is_train, int push_cnt, hipEvent_t rows_in = nullptr) {
  if (!f.any_own) return DFH_OK;
  dfh_table* t = s->t;
  dfh_batch* b = f.b;
  const bool one = s->c->world == 1;  // the number of keys is on the device (the kernel clamps to *d_U): rows and threads for nnz of them
  const size_t n = one ? (size_t)b->nnz : (size_t)(f.own_hi - f.own_lo);
  if (int rcr = table_reserve(t, n)) return rcr;
  StageScope ts(s, DFH_SHARD_STAGE_L, t->ctx->stream);
  return step_lookup(t, b, is_train, push_cnt, f.own_lo, one ? b->d_U : (const uint32_t*)nullptr, n, StepExtras{},
                     rows_in ? s->w_rows[f.slot] : (const float*)nullptr, f.U, rows_in);
}

// K: the keys other ranks own (+ their epoch-0 counts) to their owners.  Two message groups, one send and one receive per
// peer each — the pattern every RCCL release serves (several sends to one peer inside a group are not).
// ready: the minibatch's Localizer (preparation stream); freed: the previous user of this slot's receive buffers has applied
// (or released) what it received
int flight_K(dfh_shard* s, Flight& f, int push_cnt, hipStream_t st, hipEvent_t ready = nullptr, hipEvent_t freed = nullptr,
             hipEvent_t done = nullptr) {
  dfh_comm* c = s->c;
  dfh_batch* b = f.b;
  int rc;
  StageScope ts(s, DFH_SHARD_STAGE_K, st);
  if ((rc = wait_on(st, ready)) || (rc = wait_on(st, freed))) return rc;
  flight_bytes(s, f, sizeof(uint64_t));
  XPart xk{f.have ? b->d_feaids : nullptr, s->xsb.data(), s->xso.data(), s->r_keys[f.slot], s->xrb.data(), nullptr};
  rc = comm_exchange(c, &xk, 1, st, DFH_XCHG_KEYS);
  if (rc) return rc;
  if (push_cnt) {
    if (f.have && !b->has_cnt) {
      hipLaunchKernelGGL(k_loc_counts, dim3(grid_for_threads(b->nnz, c->ctx)), dim3(256), 0, st, b->d_col_ptr, b->d_U, b->d_feacnt);
      DFH_HIP(hipGetLastError());
      b->has_cnt = true;
    }
    flight_bytes(s, f, sizeof(float));
    XPart xc{f.have ? b->d_feacnt : nullptr, s->xsb.data(), s->xso.data(), s->r_cnt[f.slot], s->xrb.data(), nullptr};
    rc = comm_exchange(c, &xc, 1, st, DFH_XCHG_CNT);
    if (rc) return rc;
  }
  return record_on(st, done);
}

// R: owners resolve the received keys once, count-push, pull (every source reads the same model version); per received
// entry or per distinct key (owner_per_entry) — P follows the choice through f.listed
int flight_R(dfh_shard* s, Flight& f, int push_cnt, hipEvent_t keys_in = nullptr, hipEvent_t done = nullptr) {
  dfh_table* t = s->t;
  const int W = s->c->world, q = f.slot;
  hipStream_t st = t->ctx->stream;
  int rc;
  StageScope ts(s, DFH_SHARD_STAGE_R, st);
  if ((rc = wait_on(st, keys_in))) return rc;
  if (f.nrecv) {
    rc = dfh_shard_resolve_multi(t, s->r_keys[q], f.seg.data(), W, q, s->r_rowid[q]);
    if (rc) return rc;
    f.listed = !owner_per_entry(t);
    if (!f.listed) {
      if (push_cnt) {
        rc = dfh_shard_push_count_multi(t, s->r_rowid[q], s->r_keys[q], f.seg.data(), W, q, s->r_cnt[q]);
        if (rc) return rc;
      }
      rc = dfh_shard_pull_resolved(t, s->r_rowid[q], f.nrecv, s->r_rows[q]);
    } else {
      rc = dfh_shard_count_pull_multi(t, s->r_rowid[q], s->r_keys[q], f.seg.data(), W, q, push_cnt ? s->r_cnt[q] : nullptr, s->r_rows[q]);
    }
    if (rc) return rc;
  }
  return record_on(st, done);
}

// RW: rows back to the workers, each owner's slice to its place among the minibatch's keys
int flight_RW(dfh_shard* s, Flight& f, hipStream_t st, hipEvent_t rows_out = nullptr, hipEvent_t done = nullptr) {
  const int q = f.slot;
  int rc;
  StageScope ts(s, DFH_SHARD_STAGE_RW, st);
  if ((rc = wait_on(st, rows_out))) return rc;
  flight_bytes(s, f, dfh_row_stride(s->t->v.k) * sizeof(float));
  XPart x{s->r_rows[q], s->xrb.data(), nullptr, s->w_rows[q], s->xsb.data(), s->xso.data()};
  rc = comm_exchange(s->c, &x, 1, st, DFH_XCHG_ROWS);
  if (rc) return rc;
  return record_on(st, done);
}

// F: the worker's math (step_math): own keys on the table, the others on the pulled rows.  uw_done: L wrote the others' row
// words (and waited for their rows); rows_in: the event to wait for otherwise.  grads_done: recorded between the gradient
// rows of the others' keys and the own keys' in-place update, so that G may start while that runs — the stage is then
// timed in two brackets around it
int flight_F(dfh_shard* s, Flight& f, int is_train, int push_cnt, bool uw_done = false, hipEvent_t rows_in = nullptr,
             hipEvent_t grads_done = nullptr) {
  dfh_table* t = s->t;
  dfh_ctx* ctx = t->ctx;
  dfh_batch* b = f.b;
  hipStream_t st = ctx->stream;
  const int q = f.slot;
  if (!b) return record_on(st, is_train ? grads_done : nullptr);  // a rank out of data: nothing to wait for
  std::optional<StageScope> ts(std::in_place, s, DFH_SHARD_STAGE_F, st);
  int rc = ensure_xv(b, t->v.kp);
  if (rc) return rc;
  if ((rc = wait_on(st, rows_in))) return rc;  // the rows of the other owners have arrived
  const StepRemote rem{f.any_remote ? s->w_rows[q] : nullptr, s->w_grads[q], dfh_row_stride(t->v.k)};
  if (f.any_remote && !uw_done) {
    hipLaunchKernelGGL(k_uw_remote, dim3(grid_for_threads(f.U, ctx)), dim3(256), 0, st, rem.rows, rem.stride, b->d_U, f.own_lo, f.own_hi,
                       b->d_uw, b->d_col_ptr, split_out(ctx, b, is_train, 0u), t->v.err);
    DFH_HIP(hipGetLastError());
  }
  return step_math(t, b, is_train, push_cnt, KeyRange{f.own_lo, f.own_hi, 0u}, s->c->world > 1 ? &rem : nullptr, StepExtras{},
                   [&](bool own_follows) -> int {
                     if (!grads_done) return DFH_OK;
                     ts.reset();
                     if (is_train) DFH_HIP(hipEventRecord(grads_done, st));  // the gradient rows are complete: G may start ...
                     if (own_follows) ts.emplace(s, DFH_SHARD_STAGE_F, st);  // ... while the own keys are updated in place
                     return DFH_OK;
                   });
}

// G: gradient rows to the owners (into the buffer their rows came from)
int flight_G(dfh_shard* s, Flight& f, hipStream_t st, hipEvent_t grads_in = nullptr, hipEvent_t done = nullptr) {
  const int q = f.slot;
  int rc;
  StageScope ts(s, DFH_SHARD_STAGE_G, st);
  if ((rc = wait_on(st, grads_in))) return rc;
  flight_bytes(s, f, dfh_row_stride(s->t->v.k) * sizeof(float));
  XPart x{s->w_grads[q], s->xsb.data(), s->xso.data(), s->r_rows[q], s->xrb.data(), nullptr};
  rc = comm_exchange(s->c, &x, 1, st, DFH_XCHG_GRADS);
  if (rc) return rc;
  return record_on(st, done);
}

// P: the other sources' gradients, applied source rank after source rank over what R left (f.listed); a step that does not
// train releases the rows R resolved
int flight_P(dfh_shard* s, Flight& f, int is_train, hipEvent_t grads_in = nullptr) {
  dfh_table* t = s->t;
  const int W = s->c->world, q = f.slot;
  if (!is_train) return f.nrecv ? dfh_shard_release(t, s->r_rowid[q], f.nrecv, q) : DFH_OK;
  hipStream_t st = t->ctx->stream;
  int rc;
  StageScope ts(s, DFH_SHARD_STAGE_P, st);
  if ((rc = wait_on(st, grads_in))) return rc;
  if (f.nrecv) {
    rc = !f.listed ? dfh_shard_push_grad_multi(t, s->r_rowid[q], s->r_keys[q], f.seg.data(), W, q, s->r_rows[q])
                   : dfh_shard_push_grad_listed(t, s->r_rowid[q], s->r_keys[q], f.seg.data(), W, q, s->r_rows[q]);
    if (rc) return rc;
  }
  return DFH_OK;
}

// ---- the sync schedule: one minibatch at a time, described in fl[0], exchange slot 0; every stage on the context's
// stream, ordered by it alone.  One rank: nothing is counted, nothing exchanged, nothing waits for the host.
int shard_step_sync(dfh_shard* s, dfh_batch* b, int is_train, int push_cnt, int* any_active) {
  dfh_ctx* ctx = s->t->ctx;
  if (s->timing) ++s->stage_steps;
  DFH_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int W = s->c->world;
  int rc;
  if (b) {
    rc = main_begin(b);
    if (rc) return rc;
  }
  // ---- counts: {keys for every owner, "I have a minibatch"} -> every peer, then to the host (the step's one host wait)
  if (W > 1) {
    if (s->counts_ready && s->counts_for == b) {
      // exchanged inside the previous step: long arrived
      DFH_HIP(hipEventSynchronize(s->cnt_ev));
    } else {
      DFH_ARG(!s->counts_ready, "dfh_shard_step: the batch differs from the one announced to dfh_shard_prefetch_counts");
      {
        StageScope ts(s, DFH_SHARD_STAGE_COUNTS, st);
        rc = queue_counts(s, b);
        if (rc) return rc;
      }
      DFH_HIP(hipStreamSynchronize(st));
    }
    s->counts_ready = false;
  }
  Flight& f = s->fl[0];
  flight_sizes(s, f, b, 0);
  if (any_active) *any_active = f.active != 0 ? 1 : 0;
  ++s->steps;
  if (b) b->nrows_seen += (float)b->nrows;
  if (f.active == 0) {
    s->next_armed = false;  // the epoch is over: nothing follows
    return b ? main_end(b) : DFH_OK;
  }
  if ((rc = flight_bufs(s, f))) return rc;
  if ((rc = flight_L(s, f, is_train, push_cnt))) return rc;
  if (W > 1 && (rc = flight_K(s, f, push_cnt, st))) return rc;
  if (f.nrecv && (rc = flight_R(s, f, push_cnt))) return rc;
  if (W > 1 && (rc = flight_RW(s, f, st))) return rc;
  if ((rc = flight_F(s, f, is_train, push_cnt))) return rc;
  // ---- the counts of the FOLLOWING step (dfh_shard_prefetch_counts): on their way to the host while this
  // step's gradients travel and are applied, so that the next call finds them there
  if (s->next_armed) {
    s->next_armed = false;
    dfh_batch* nb = s->next_b;
    if (nb) {
      rc = main_begin(nb);  // its Localizer (preparation stream) has to be through
      if (rc) return rc;
    }
    rc = queue_counts(s, nb);
    if (rc) return rc;
    DFH_HIP(hipEventRecord(s->cnt_ev, st));
    s->counts_ready = true;
    s->counts_for = nb;
  }
  if (is_train && W > 1 && (rc = flight_G(s, f, st))) return rc;
  if (f.nrecv && (rc = flight_P(s, f, is_train))) return rc;
  return b ? main_end(b) : DFH_OK;
}

// The collectives' stream reads a minibatch's key list (its counts, then K): behind the minibatch's Localizer, wherever that
// was queued.  With preparation streams that is the batch's ready event.  Without them the Localizer sits on the main stream
// — on the single queue maybe only noted, to ride in later launches: it is queued here — and nothing else orders the
// collectives' stream behind it: an event recorded on the main stream now does (everything queued there so far comes first).
int cs_behind_prep(dfh_shard* s, dfh_batch* b) {
  if (!b) return DFH_OK;
  if (int rc = flush_pending(b)) return rc;
  if (b->ready_pending) {
    DFH_HIP(hipStreamWaitEvent(s->cs, b->ev_ready, 0));
  } else if (!b->ctx->pipeline) {
    DFH_HIP(hipEventRecord(s->ev_m, b->ctx->stream));
    DFH_HIP(hipStreamWaitEvent(s->cs, s->ev_m, 0));
  }
  return DFH_OK;
}

// ---- the overlap schedule: two minibatches in flight (dfh_shard_set_exchange(s, 1)); world > 1.  K, RW and G on the
// collectives' stream, events between the stages.
// cur = the minibatch this call trains.  If it was announced to the previous call (dfh_shard_prefetch_counts) its
// counts, keys and rows were exchanged in there; otherwise (first step of an epoch) they are exchanged now.
int shard_step_overlap(dfh_shard* s, dfh_batch* b, int is_train, int push_cnt, int* any_active) {
  dfh_comm* c = s->c;
  dfh_ctx* ctx = s->t->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream, cs = s->cs;
  int rc;
  if (s->timing) ++s->stage_steps;
  static const bool trace = getenv("DFH_SHARD_TRACE") != nullptr;
  Flight& cur = s->fl[s->cur];
  if (trace)
    fprintf(stderr, "[shard %d] step %llu: b=%p cur{slot %d described %d pulled %d b=%p} armed %d next_b=%p\n", c->rank,
            (unsigned long long)s->steps, (void*)b, s->cur, (int)cur.described, (int)cur.pulled, (void*)cur.b, (int)s->next_armed,
            (void*)s->next_b);
  if (!(cur.described && cur.b == b)) {
    // not announced: describe it now (its counts over the collectives' stream, one host wait)
    DFH_ARG(!cur.described || !cur.pulled, "dfh_shard_step: the batch differs from the one announced to dfh_shard_prefetch_counts");
    if ((rc = cs_behind_prep(s, b))) return rc;
    {
      StageScope ts(s, DFH_SHARD_STAGE_COUNTS, cs);
      rc = queue_counts(s, b, cs);
      if (rc) return rc;
    }
    DFH_HIP(hipStreamSynchronize(cs));
    flight_sizes(s, cur, b, s->cur);
  }
  if (any_active) *any_active = cur.active != 0 ? 1 : 0;
  ++s->steps;
  if (b) b->nrows_seen += (float)b->nrows;
  // the minibatch after this one, if the caller named it
  const bool look = s->next_armed;
  dfh_batch* nb = look ? s->next_b : nullptr;
  s->next_armed = false;
  Flight& nxt = s->fl[s->cur ^ 1];
  nxt = Flight();
  if (cur.active == 0) {
    // nobody has a minibatch: the epoch is over (nothing can have been announced behind it)
    cur = Flight();
    return b ? main_end(b) : DFH_OK;
  }
  // K of a minibatch on the collectives' stream, behind its Localizer (preparation stream) and behind P (or the release)
  // of the minibatch that last received into its slot; then R on the main stream and RW on the collectives'
  auto keys_out = [&](Flight& f) {
    const int q = f.slot;
    hipEvent_t ready = f.b && f.b->ready_pending ? f.b->ev_ready : nullptr;
    hipEvent_t freed = s->p_pending[q] ? s->ev_p[q] : nullptr;
    s->p_pending[q] = false;
    return flight_K(s, f, push_cnt, cs, ready, freed, s->ev_k[q]);
  };
  auto rows_back = [&](Flight& f) {
    const int q = f.slot;
    int r = flight_R(s, f, push_cnt, s->ev_k[q], s->ev_r[q]);
    if (!r) r = flight_RW(s, f, cs, s->ev_r[q], s->ev_rw[q]);
    f.pulled = r == DFH_OK;  // the other owners' rows are on their way to w_rows[q]
    return r;
  };
  rc = flight_bufs(s, cur);
  if (rc) return rc;
  if (b) {
    rc = main_begin(b);  // its Localizer (preparation stream) -> main stream
    if (rc) return rc;
    // (the split list of THIS minibatch: every launch that appends to it — L's, or F's k_uw_remote at the pipeline fill — is
    // made below, in this call, on this stream, behind this batch object's previous update; none for the next minibatch)
  }
  const int q = cur.slot;
  // L runs after everything the previous step applied: own keys are read with zero staleness.  The row words of the
  // others' keys ride in its launch when their rows are already on their way (every step but an epoch's first)
  const bool uw_folded = cur.any_own && cur.pulled && cur.any_remote && b != nullptr;
  if ((rc = flight_L(s, cur, is_train, push_cnt, uw_folded ? s->ev_rw[q] : nullptr))) return rc;
  if (!cur.pulled) {  // pipeline fill: K, R, RW of this very minibatch, in the sync step's order (after L)
    if ((rc = keys_out(cur)) || (rc = rows_back(cur))) return rc;
  }
  // ---- counts of the next minibatch: on their way while F is queued and runs
  if (look) {
    if ((rc = cs_behind_prep(s, nb))) return rc;
    StageScope ts(s, DFH_SHARD_STAGE_COUNTS, cs);
    rc = queue_counts(s, nb, cs);
    if (rc) return rc;
    DFH_HIP(hipEventRecord(s->cnt_ev, cs));
  }
  if ((rc = flight_F(s, cur, is_train, push_cnt, uw_folded, uw_folded ? nullptr : s->ev_rw[q], s->ev_f))) return rc;
  // ---- the next minibatch's sizes (the one host wait; the device is busy with F), then its keys
  bool ahead = false;
  if (look) {
    DFH_HIP(hipEventSynchronize(s->cnt_ev));
    flight_sizes(s, nxt, nb, s->cur ^ 1);
    ahead = nxt.active != 0;
    if (trace)
      fprintf(stderr, "[shard %d]   next: active %zu U %zu nrecv %zu own [%u, %u) -> ahead %d\n", c->rank, nxt.active, nxt.U, nxt.nrecv,
              nxt.own_lo, nxt.own_hi, (int)ahead);
    if (ahead) {
      rc = flight_bufs(s, nxt);
      if (rc) return rc;
      rc = keys_out(nxt);  // small; travels while F computes
      if (rc) return rc;
    }
  }
  if (is_train && (rc = flight_G(s, cur, cs, s->ev_f, s->ev_g))) return rc;
  // ---- R, RW of the next minibatch: the owners pull while this step's gradients travel — before they are applied
  // (staleness 1 for the rows of other owners) — and the rows travel while they are applied
  if (ahead && (rc = rows_back(nxt))) return rc;
  if ((rc = flight_P(s, cur, is_train, s->ev_g))) return rc;
  if (cur.nrecv) {  // r_keys[q] / r_rowid[q] / r_rows[q] are free again once this point of the main stream is reached
    DFH_HIP(hipEventRecord(s->ev_p[q], st));
    s->p_pending[q] = true;
  }
  cur = Flight();
  if (look) s->cur ^= 1;  // the announced minibatch (described, maybe pulled) is the next call's
  return b ? main_end(b) : DFH_OK;
}
}  // namespace

extern "C" {

int dfh_shard_prefetch_counts(dfh_shard* s, dfh_batch* b_next) {
  DFH_ARG(s, "dfh_shard_prefetch_counts: NULL shard");
  DFH_ARG(!b_next || b_next->ctx == s->t->ctx, "batch and shard must share a context");
  if (b_next && !b_next->localized) {
    set_error("dfh_shard_prefetch_counts: batch is not localized (call dfh_localize first)");
    return DFH_ERR_STATE;
  }
  s->next_b = b_next;
  s->next_armed = s->c->world > 1;  // one rank: there is nothing to count
  return DFH_OK;
}

int dfh_shard_set_exchange(dfh_shard* s, int mode) {
  DFH_ARG(s && (mode == 0 || mode == 1), "dfh_shard_set_exchange: mode 0 (sync) or 1 (overlap)");
  if (s->fl[0].pulled || s->fl[1].pulled || s->counts_ready) {
    set_error("dfh_shard_set_exchange: a minibatch is under way (call it between epochs)");
    return DFH_ERR_STATE;
  }
  dfh_ctx* ctx = s->t->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  int rc = sync_all(ctx);
  if (rc) return rc;
  if (mode == 1 && !s->cs) {
    DFH_HIP(hipStreamCreateWithFlags(&s->cs, hipStreamNonBlocking));
    s->c->ctx->extra.push_back(s->cs);  // a growing table drains it before it re-allocates (table_grow)
    // these events order two streams of ONE device: no system-scope fence at the record
    const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
    for (hipEvent_t* e : {&s->ev_k[0], &s->ev_k[1], &s->ev_r[0], &s->ev_r[1], &s->ev_rw[0], &s->ev_rw[1], &s->ev_f, &s->ev_g,
                          &s->ev_m, &s->ev_p[0], &s->ev_p[1]})
      DFH_HIP(hipEventCreateWithFlags(e, evf));
  }
  if (s->cs) DFH_HIP(hipStreamSynchronize(s->cs));
  s->exchange = mode;
  s->p_pending[0] = s->p_pending[1] = false;  // everything was drained above
  s->fl[0] = Flight();
  s->fl[1] = Flight();
  s->cur = 0;
  s->next_armed = false;
  return DFH_OK;
}

int dfh_shard_reserve(dfh_shard* s, size_t batch_keys, size_t recv_keys) {
  DFH_ARG(s, "dfh_shard_reserve: NULL shard");
  if (s->fl[0].pulled || s->fl[1].pulled || s->counts_ready) {
    set_error("dfh_shard_reserve: a minibatch is under way (call it before the first step or between epochs)");
    return DFH_ERR_STATE;
  }
  DFH_HIP(hipSetDevice(s->t->ctx->device));
  const size_t w = s->c->world > 1 ? batch_keys : 0;
  const int nslots = s->exchange == 1 ? 2 : 1;
  for (int q = 0; q < nslots; ++q)
    if (int rc = slot_bufs(s, q, recv_keys, w, w, false)) return rc;
  return DFH_OK;
}

int dfh_shard_set_timing(dfh_shard* s, int enable) {
  DFH_ARG(s, "dfh_shard_set_timing: NULL shard");
  s->timing = enable != 0;
  return DFH_OK;
}

int dfh_shard_get_timing(dfh_shard* s, int reset, double* ms, uint64_t* steps) {
  DFH_ARG(s && ms, "dfh_shard_get_timing: NULL argument");
  DFH_HIP(hipSetDevice(s->t->ctx->device));
  if (s->cs) DFH_HIP(hipStreamSynchronize(s->cs));
  int rc = sync_all(s->t->ctx);
  if (rc) return rc;
  for (auto& sp : s->spans) {
    float e = 0;
    if (hipEventElapsedTime(&e, sp.a, sp.b) == hipSuccess) s->stage_ms[sp.id] += e;
    s->ev_pool.push_back(sp.a);
    s->ev_pool.push_back(sp.b);
  }
  s->spans.clear();
  for (int i = 0; i < DFH_SHARD_STAGES; ++i) {
    ms[i] = s->stage_ms[i];
    if (reset) s->stage_ms[i] = 0;
  }
  if (steps) *steps = s->stage_steps;
  if (reset) s->stage_steps = 0;
  return DFH_OK;
}

int dfh_shard_step(dfh_shard* s, dfh_batch* b, int is_train, int push_cnt, int* any_active) {
  DFH_ARG(s, "dfh_shard_step: NULL shard");
  DFH_ARG(!b || b->ctx == s->t->ctx, "batch and shard must share a context");
  if (b && !b->localized) {
    set_error("dfh_shard_step: batch is not localized (call dfh_localize first)");
    return DFH_ERR_STATE;
  }
  if (is_train) {
    if (int rca = require_aux(s->t, "dfh_shard_step(is_train)")) return rca;
  }
  // one rank takes the sync schedule whatever the mode: there is nothing to overlap
  return (s->exchange == 1 && s->c->world > 1) ? shard_step_overlap(s, b, is_train, push_cnt, any_active)
                                              : shard_step_sync(s, b, is_train, push_cnt, any_active);
}

}  // extern "C"

namespace {
// ---- the literal, call-by-call Store::Pull / Push on the sharded model (dfh_shard_pull_host / dfh_shard_push_host)
struct HostCall {
  std::vector<size_t> send, recv, seg, soff;  // keys per owner / per source, prefix sums
  size_t nrecv = 0;
};

// who owns what of `keys` (ascending), and how much every rank sends this one: the W x W count matrix is gathered
int host_call_sizes(dfh_shard* s, const uint64_t* keys, size_t n, HostCall* h) {
  dfh_comm* c = s->c;
  const int W = c->world, me = c->rank;
  for (size_t i = 1; i < n; ++i) DFH_ARG(keys[i] > keys[i - 1], "keys must be strictly ascending (a Localizer's output)");
  h->send.assign(W, 0);
  h->soff.assign(W + 1, 0);
  for (int p = 0; p < W; ++p) {
    const uint64_t* e = p + 1 < W ? std::lower_bound(keys, keys + n, s->h_splits[p]) : keys + n;
    h->soff[p + 1] = (size_t)(e - keys);
    h->send[p] = h->soff[p + 1] - h->soff[p];
  }
  std::vector<uint64_t> mine(h->send.begin(), h->send.end()), all((size_t)W * W);
  int rc = dfh_comm_allgather(c, mine.data(), (size_t)W * sizeof(uint64_t), all.data());
  if (rc) return rc;
  h->recv.assign(W, 0);
  h->seg.assign(W + 1, 0);
  for (int p = 0; p < W; ++p) {
    h->recv[p] = (size_t)all[(size_t)p * W + me];
    h->seg[p + 1] = h->seg[p] + h->recv[p];
  }
  h->nrecv = h->seg[W];
  return DFH_OK;
}

void bytes_of(const HostCall& h, int W, size_t unit, std::vector<size_t>& sb, std::vector<size_t>& rb) {
  sb.resize(W);
  rb.resize(W);
  for (int p = 0; p < W; ++p) {
    sb[p] = h.send[p] * unit;
    rb[p] = h.recv[p] * unit;
  }
}

int host_call_guard(dfh_shard* s, const char* who) {
  if (s->fl[0].pulled || s->fl[1].pulled || s->counts_ready) {
    set_error(std::string(who) + ": a minibatch of dfh_shard_step is under way");
    return DFH_ERR_STATE;
  }
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_shard_pull_host(dfh_shard* s, const uint64_t* keys, size_t n, float* vals, size_t* nvals, int* lens, size_t* nlens) {
  DFH_ARG(s && nvals && nlens && (n == 0 || (keys && vals && lens)), "dfh_shard_pull_host: NULL argument");
  if (int g = host_call_guard(s, "dfh_shard_pull_host")) return g;
  dfh_table* t = s->t;
  dfh_comm* c = s->c;
  dfh_ctx* ctx = t->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int W = c->world, k = t->v.k;
  const size_t stride = dfh_row_stride(k);
  *nvals = 0;
  *nlens = k == 0 ? 0 : n;  // sgd_updater.cc:40
  if (int rck = check_keys(keys, n)) return rck;
  HostCall h;
  int rc = host_call_sizes(s, keys, n, &h);
  if (rc) return rc;
  rc = slot_bufs(s, 0, h.nrecv, n, 0, true);
  if (rc) return rc;
  rc = ensure_scratch(ctx, padded<uint64_t>(std::max<size_t>(n, 1)));
  if (rc) return rc;
  uint64_t* d_keys = static_cast<uint64_t*>(ctx->scratch);
  if (n) DFH_HIP(hipMemcpyAsync(d_keys, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  std::vector<size_t> sb, rb;
  bytes_of(h, W, sizeof(uint64_t), sb, rb);
  XPart xk{d_keys, sb.data(), nullptr, s->r_keys[0], rb.data(), nullptr};
  rc = comm_exchange(c, &xk, 1);
  if (rc) return rc;
  if (h.nrecv) {  // owners: SGDUpdater::Get for every requester (sgd_updater.cc:32-56)
    rc = dfh_shard_resolve(t, s->r_keys[0], h.nrecv, s->r_rowid[0]);
    if (rc) return rc;
    rc = dfh_shard_pull_resolved(t, s->r_rowid[0], h.nrecv, s->r_rows[0]);
    if (rc) return rc;
  }
  bytes_of(h, W, stride * sizeof(float), sb, rb);
  XPart xr{s->r_rows[0], rb.data(), nullptr, s->w_rows[0], sb.data(), nullptr};
  rc = comm_exchange(c, &xr, 1);
  if (rc) return rc;
  std::vector<float> rows(std::max<size_t>(n, 1) * stride);
  if (n) DFH_HIP(hipMemcpyAsync(rows.data(), s->w_rows[0], n * stride * sizeof(float), hipMemcpyDeviceToHost, st));
  DFH_HIP(hipStreamSynchronize(st));
  rc = check_table_err(t);
  if (rc) return rc;
  size_t p = 0;
  for (size_t i = 0; i < n; ++i) {  // ragged layout of SGDUpdater::Get (sgd_updater.cc:46-53)
    const float* r = rows.data() + i * stride;
    vals[p++] = r[0];
    if (r[1] != 0.0f) {
      memcpy(vals + p, r + 4, sizeof(float) * (size_t)k);
      p += (size_t)k;
      lens[i] = k + 1;
    } else if (k != 0) {
      lens[i] = 1;
    }
  }
  *nvals = p;
  return DFH_OK;
}

int dfh_shard_push_host(dfh_shard* s, const uint64_t* keys, size_t n, int val_type, const float* vals, size_t nvals, const int* lens,
                        size_t nlens) {
  DFH_ARG(s && (n == 0 || (keys && vals)), "dfh_shard_push_host: NULL argument");
  DFH_ARG(val_type == DFH_FEA_COUNT || val_type == DFH_GRADIENT, "dfh_shard_push_host: unknown val_type (sgd_updater.cc:99)");
  if (int g = host_call_guard(s, "dfh_shard_push_host")) return g;
  dfh_table* t = s->t;
  dfh_comm* c = s->c;
  dfh_ctx* ctx = t->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int W = c->world, k = t->v.k;
  const size_t stride = dfh_row_stride(k);
  if (int rck = check_keys(keys, n)) return rck;
  const bool grad = val_type == DFH_GRADIENT;
  std::vector<float> rows;
  if (grad) {
    if (int rca = require_aux(t, "dfh_shard_push_host(kGradient)")) return rca;
    const bool w_only = nlens == 0;
    if (w_only) {
      DFH_ARG(nvals == n, "kGradient: CHECK_EQ(values.size(), size) (sgd_updater.cc:79)");
    } else {
      DFH_ARG(nlens == n && lens, "kGradient: CHECK_EQ(lens.size(), size) (sgd_updater.cc:81)");
    }
    rows.assign(std::max<size_t>(n, 1) * stride, 0.0f);
    size_t p = 0;
    for (size_t i = 0; i < n; ++i) {
      float* r = rows.data() + i * stride;
      DFH_ARG(p < nvals, "kGradient: values shorter than lens imply (sgd_updater.cc:96)");
      r[0] = vals[p++];
      if (!w_only && lens[i] > 1) {
        DFH_ARG(lens[i] == k + 1, "kGradient: CHECK_EQ(lens[i], V_dim+1) (sgd_updater.cc:91)");
        DFH_ARG(p + (size_t)k <= nvals, "kGradient: values shorter than lens imply (sgd_updater.cc:96)");
        r[1] = 1.0f;
        memcpy(r + 4, vals + p, sizeof(float) * (size_t)k);
        p += (size_t)k;
      }
    }
    DFH_ARG(p == nvals, "kGradient: CHECK_EQ(p, values.size()) (sgd_updater.cc:96)");
  } else {
    DFH_ARG(nvals == n, "kFeaCount: CHECK_EQ(fea_ids.size(), values.size()) (sgd_updater.cc:63)");
  }
  HostCall h;
  int rc = host_call_sizes(s, keys, n, &h);
  if (rc) return rc;
  rc = slot_bufs(s, 0, h.nrecv, n, 0, true);
  if (rc) return rc;
  rc = ensure_scratch(ctx, padded<uint64_t>(std::max<size_t>(n, 1)) + padded<float>(std::max<size_t>(n, 1)));
  if (rc) return rc;
  Carver cv(ctx->scratch);
  uint64_t* d_keys = cv.take<uint64_t>(std::max<size_t>(n, 1));
  float* d_cnt = cv.take<float>(std::max<size_t>(n, 1));
  if (n) DFH_HIP(hipMemcpyAsync(d_keys, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  std::vector<size_t> sb, rb;
  bytes_of(h, W, sizeof(uint64_t), sb, rb);
  XPart xk{d_keys, sb.data(), nullptr, s->r_keys[0], rb.data(), nullptr};
  rc = comm_exchange(c, &xk, 1);
  if (rc) return rc;
  if (grad) {
    if (n) DFH_HIP(hipMemcpyAsync(s->w_rows[0], rows.data(), n * stride * sizeof(float), hipMemcpyHostToDevice, st));
    bytes_of(h, W, stride * sizeof(float), sb, rb);
    XPart xg{s->w_rows[0], sb.data(), nullptr, s->r_rows[0], rb.data(), nullptr};
    rc = comm_exchange(c, &xg, 1);
    if (rc) return rc;
    DFH_HIP(hipStreamSynchronize(st));  // `rows` leaves scope
  } else {
    if (n) DFH_HIP(hipMemcpyAsync(d_cnt, vals, n * sizeof(float), hipMemcpyHostToDevice, st));
    bytes_of(h, W, sizeof(float), sb, rb);
    XPart xc{d_cnt, sb.data(), nullptr, s->r_cnt[0], rb.data(), nullptr};
    rc = comm_exchange(c, &xc, 1);
    if (rc) return rc;
  }
  if (h.nrecv) {  // owners: SGDUpdater::Update, the sources one after the other in ascending rank order
    rc = dfh_shard_resolve_multi(t, s->r_keys[0], h.seg.data(), W, 0, s->r_rowid[0]);
    if (rc) return rc;
    if (grad) {
      rc = dfh_shard_push_grad_multi(t, s->r_rowid[0], s->r_keys[0], h.seg.data(), W, 0, s->r_rows[0]);
      if (rc) return rc;
    } else {
      rc = dfh_shard_push_count_multi(t, s->r_rowid[0], s->r_keys[0], h.seg.data(), W, 0, s->r_cnt[0]);
      if (rc) return rc;
      rc = dfh_shard_release(t, s->r_rowid[0], h.nrecv, 0);
      if (rc) return rc;
    }
  }
  DFH_HIP(hipStreamSynchronize(st));
  return check_table_err(t);
}

}  // extern "C"
#endif  // DFH_SHARD_HIP_
