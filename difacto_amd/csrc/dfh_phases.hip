// dfh_phases.hip — the stream phases of a batch object (preparation stream -> ev_ready -> main stream -> ev_free), the
// split list's counters, and what every launch site shares: grid sizes, the scratch block, the dispatch by lanes per row
// and the timed launch.
namespace {
// stream of the batch's current preparation phase
inline hipStream_t prep_of(const dfh_batch* b) {
  const dfh_ctx* c = b->ctx;
  return (c->pipeline && b->prep) ? b->prep : c->stream;
}
// a new phase (a load / attach call) takes the next preparation stream
void phase_begin(dfh_batch* b) {
  dfh_ctx* c = b->ctx;
  // a new minibatch is loaded into an object whose noted Localizer has not been queued completely: finish it first (its
  // stages leave per-object state behind — bucket totals reset by the sort, the next call's splitters written by emit)
  if (b->pend_stage < RID_STAGES) (void)flush_pending(b);
  hipStream_t next = c->pipeline ? c->preps[c->next_prep++ % c->nprep] : nullptr;
  if (next && b->prep && next != b->prep && b->ready_pending) {
    // the previous phase's output was never consumed by a step: keep the two phases ordered
    (void)hipStreamWaitEvent(next, b->ev_ready, 0);
  }
  b->prep = next;
}
// prep-stream work on a batch must not overwrite buffers a queued step still reads
int prep_begin(dfh_batch* b) {
  dfh_ctx* c = b->ctx;
  if (c->pipeline && !b->prep) phase_begin(b);
  if (c->pipeline && b->free_pending) {
    DFH_HIP(hipStreamWaitEvent(prep_of(b), b->ev_free, 0));
    b->free_pending = false;
  }
  return DFH_OK;
}
int prep_end(dfh_batch* b) {
  dfh_ctx* c = b->ctx;
  if (c->pipeline && !b->defer_ready) {
    DFH_HIP(hipEventRecord(b->ev_ready, prep_of(b)));
    b->ready_pending = true;
  }
  return DFH_OK;
}
int main_begin(dfh_batch* b) {
  dfh_ctx* c = b->ctx;
  if (b->pend_stage < RID_STAGES) {  // consumed before every stage found a carrier launch (the first steps of a loop)
    int rc = flush_pending(b);
    if (rc) return rc;
  }
  if (b->ready_pending) {
    DFH_HIP(hipStreamWaitEvent(c->stream, b->ev_ready, 0));
    b->ready_pending = false;
  }
  return DFH_OK;
}
int main_end(dfh_batch* b) {
  dfh_ctx* c = b->ctx;
  if (b->split_listing) {  // this step's launches filled one counter of the split list and zeroed the other: the next step's
    b->split_listing = false;
    b->split_last = b->split_sel;
    b->split_sel ^= 1;
  }
  if (c->pipeline) {
    DFH_HIP(hipEventRecord(b->ev_free, c->stream));
    b->free_pending = true;
  }
  return DFH_OK;
}
int sync_all(dfh_ctx* c) {
  for (hipStream_t p : c->preps) DFH_HIP(hipStreamSynchronize(p));
  for (hipStream_t p : c->extra) DFH_HIP(hipStreamSynchronize(p));
  DFH_HIP(hipStreamSynchronize(c->stream));
  return DFH_OK;
}
// the list of the very hot keys' parts for the update's split role (SplitOut, dfh_kernels.hip): handed to the launches of a
// TRAINING step that see the minibatch's keys with their segments; u_base = rank of the first key such a launch sees
inline bool split_listed(const dfh_ctx* c, const dfh_batch* b, int is_train) { return b && is_train && c->upd_kernel && c->upd_split; }
// (every launch that takes it appends to the batch object's current counter and zeroes the other one; the step's main_end then
// swaps the two — the owner of SplitOut's invariant.  Called after main_begin: behind the batch object's previous update.)
inline uint32_t* split_counter(const dfh_batch* b) { return b->d_U + 2 + b->split_sel; }
inline SplitOut split_out(const dfh_ctx* c, dfh_batch* b, int is_train, uint32_t u_base) {
  if (!split_listed(c, b, is_train)) return SplitOut{nullptr, nullptr, 0u, 0u};
  b->split_listing = true;
  return SplitOut{b->d_split_ent, split_counter(b), u_base, (uint32_t)b->split_cap};
}

inline int grid_for_threads(size_t n, const dfh_ctx* c) {
  size_t b = (n + 255) / 256;
  size_t cap = (size_t)c->num_cu * 8;
  return (int)std::max<size_t>(1, std::min(b, cap));
}
inline int grid_for_waves(size_t nwaves, const dfh_ctx* c) {
  size_t b = (nwaves + 3) / 4;
  size_t cap = (size_t)c->num_cu * 8;
  return (int)std::max<size_t>(1, std::min(b, cap));
}

int ensure_scratch(dfh_ctx* c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return DFH_OK;
  if (c->scratch) {
    DFH_HIP(hipStreamSynchronize(c->stream));
    DFH_HIP(hipFree(c->scratch));
    c->scratch = nullptr;
    c->scratch_bytes = 0;
  }
  size_t want = std::max(bytes, (size_t)1 << 20);
  want = (want + 255) & ~(size_t)255;
  DFH_HIP(hipMalloc(&c->scratch, want));
  c->scratch_bytes = want;
  return DFH_OK;
}

// carve aligned pieces out of the scratch block
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return p;
  }
};
template <typename T>
size_t padded(size_t n) { return ((n * sizeof(T)) + 255 + 256) & ~(size_t)255; }

inline int lanes_for(int kp) {
  int nvec = kp / 4;
  int L = 1;
  while (L < nvec) L <<= 1;
  return L;
}

template <typename F>
int dispatch_L(int kp, F&& f) {
  switch (lanes_for(kp)) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    case 64: f(std::integral_constant<int, 64>()); break;
    default:
      set_error("V_dim > 256 is not supported by the wave-per-row kernels");
      return DFH_ERR_ARG;
  }
  return DFH_OK;
}

constexpr KeyRange kAllKeys{0u, 0xFFFFFFFFu, 0u};
constexpr size_t kSmallBatchPairs = 16384;  // at or below: no probe ahead on the preparation stream (launch-bound sizes)

// One kernel launch.  timed: the dispatch itself carries the two events (hipExtLaunchKernelGGL), so the span is the kernel's
// own begin / end as the command processor stamps them — what a profiler reports — and no marker packet drains the stream
// around it.  Otherwise the plain launch.  (The arguments are converted to the kernel's parameter types here: the timed
// form packs them as it gets them.)
template <typename... P, typename... A>
void launch_span(dfh_ctx* c, bool timed, int kid, int ride, void (*kernel)(P...), dim3 grid, dim3 block, size_t shm, hipStream_t s,
                 const A&... args) {
  hipEvent_t ea = timed ? TimeScope::get(c) : nullptr, eb = timed ? TimeScope::get(c) : nullptr;
  if (ea && eb) {
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)shm, s, ea, eb, 0, static_cast<P>(args)...);
    c->spans.push_back({kid, ea, eb, ride});
  } else {
    hipLaunchKernelGGL(kernel, grid, block, shm, s, static_cast<P>(args)...);
  }
}
// a launch of kernel class kid (DFH_K_*): timed when dfh_ctx_set_timing turned that class on
template <typename... P, typename... A>
void launch_k(dfh_ctx* c, int kid, void (*kernel)(P...), dim3 grid, dim3 block, size_t shm, hipStream_t s, const A&... args) {
  launch_span(c, ((c->timing >> kid) & 1u) != 0, kid, 0, kernel, grid, block, shm, s, args...);
}
}  // namespace
