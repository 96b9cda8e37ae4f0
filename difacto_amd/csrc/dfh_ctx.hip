// dfh_ctx.hip — the context calls: create / destroy, preparation streams, the option table (measurement switches and launch
// tuning), per-kernel timing, and the plain device memory calls.
namespace {
// the options of dfh_ctx_set_option that store an int of [lo, hi] and do nothing else (defaults and meaning: dfh_handles.h)
struct IntOption { const char* name; int dfh_ctx::*field; int lo, hi; const char* msg; };
const IntOption kIntOptions[] = {
    {"fwd_blocks", &dfh_ctx::fwd_blocks, 0, PROG_SLOTS, "fwd_blocks must be in [0, 16384] (0: one wave per example)"},
    {"bwd_small_blocks", &dfh_ctx::bwd_small_blocks, 1, 65536, "bwd_small_blocks must be in [1, 65536]"},
    {"upd_kernel", &dfh_ctx::upd_kernel, 0, 1, "upd_kernel must be 0 (k_backward_all) or 1 (k_update_fused)"},
    {"upd_hot_blocks", &dfh_ctx::upd_hot_blocks, 1, 65536, "upd_*_blocks must be in [1, 65536]"},
    {"upd_mid_blocks", &dfh_ctx::upd_mid_blocks, 1, 65536, "upd_*_blocks must be in [1, 65536]"},
    {"upd_few_blocks", &dfh_ctx::upd_few_blocks, 1, 65536, "upd_*_blocks must be in [1, 65536]"},
    {"upd_single_blocks", &dfh_ctx::upd_single_blocks, 1, 65536, "upd_*_blocks must be in [1, 65536]"},
    {"grow_initial_rows", &dfh_ctx::grow_initial_rows, 16, 1 << 28, "grow_initial_rows must be in [16, 2^28]"},
    {"auc_in_update", &dfh_ctx::auc_in_update, 0, 1, "auc_in_update must be 0 (k_auc_pairs as its own launch) or 1 (a role of k_update_fused)"},
    {"shard_mixed_update", &dfh_ctx::shard_mixed_update, 0, 1, "shard_mixed_update must be 0 or 1"},
    {"owner_per_key", &dfh_ctx::owner_per_key, 0, 1, "owner_per_key must be 0 (count push, Pull, gradient push per received entry) or 1 (per distinct key)"},
    {"upd_split", &dfh_ctx::upd_split, 0, 1, "upd_split must be 0 (one block per hot key, whatever its length) or 1 (a block per part of 1 024 occurrences)"},
    {"upd_interleave", &dfh_ctx::upd_interleave, 0, 64, "upd_interleave must be in [0, 64]"},
    {"event_flags", &dfh_ctx::event_flags, 0, 1, "event_flags must be 0 (default events) or 1 (no system-scope fence); set before batches are created"},
};
}  // namespace

extern "C" {

const char* dfh_last_error(void) { return g_err.c_str(); }

void dfh_updater_param_default(dfh_updater_param* p, int V_dim) {
  // src/sgd/sgd_param.h:95-105
  p->l1 = 1.0f;
  p->l2 = 0.0f;
  p->V_l2 = 0.01f;
  p->lr = 0.01f;
  p->lr_beta = 1.0f;
  p->V_lr = 0.01f;
  p->V_lr_beta = 1.0f;
  p->V_init_scale = 0.01f;
  p->V_threshold = 10;
  p->V_dim = V_dim;
  p->seed = 0;
  p->init_mode = DFH_INIT_HASH;
}

uint64_t dfh_reverse_bytes(uint64_t x) { return reverse_bytes(x); }
uint64_t dfh_encode_fea_grp_id(uint64_t x, int gid, int nbits) { return (x << nbits) | (uint64_t)gid; }
size_t dfh_row_stride(int V_dim) { return 4 + (size_t)((V_dim + 3) / 4) * 4; }

// ------------------------------------------------------------------ context
int dfh_ctx_create(int device, void* stream, dfh_ctx** out) {
  DFH_ARG(out != nullptr, "dfh_ctx_create: out is NULL");
  int ndev = 0;
  DFH_HIP(hipGetDeviceCount(&ndev));
  if (ndev <= 0 || device < 0 || device >= ndev) {
    set_error("dfh_ctx_create: no such HIP device (this library has no CPU fallback)");
    return DFH_ERR_HIP;
  }
  DFH_HIP(hipSetDevice(device));
  // DFH_SCHEDULE = spin | yield | blocking (experiment, tools/gpu_r04u.sh): how host threads wait for the device
  if (const char* e = getenv("DFH_SCHEDULE")) {
    const unsigned f = !strcmp(e, "spin") ? hipDeviceScheduleSpin : !strcmp(e, "yield") ? hipDeviceScheduleYield
                       : !strcmp(e, "blocking") ? hipDeviceScheduleBlockingSync : hipDeviceScheduleAuto;
    if (hipSetDeviceFlags(f) != hipSuccess) (void)hipGetLastError();
  }
  dfh_ctx* c = new (std::nothrow) dfh_ctx();
  DFH_ARG(c != nullptr, "out of host memory");
  c->device = device;
  if (const char* e = getenv("DFH_OWNER_PER_KEY")) c->owner_per_key = atoi(e) != 0;  // (measurement: bench.py --emulate-world)
  if (stream) {
    c->stream = static_cast<hipStream_t>(stream);
  } else {
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete c;
      set_error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
      return DFH_ERR_HIP;
    }
    c->own_stream = true;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
  if (!(getenv("DFH_WARM_LOAD") && atoi(getenv("DFH_WARM_LOAD")) == 0)) {   // (0: A/B)
    try {
    c->warm = std::thread([device] {
      if (hipSetDevice(device) != hipSuccess) return;
      hipStream_t s = nullptr;
      uint32_t* d = nullptr;
      if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d), 256) == hipSuccess) {
        hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, s, d, 0u);
        (void)hipStreamSynchronize(s);
      }
      (void)hipGetLastError();
      if (d) (void)hipFree(d);
      if (s) (void)hipStreamDestroy(s);
    });
    } catch (...) {  // no thread to be had: the first launch loads the code object, as before round 5 (nothing crosses the C ABI)
    }
  }
  *out = c;
  return DFH_OK;
}

int dfh_ctx_destroy(dfh_ctx* c) {
  if (!c) return DFH_OK;
  if (c->warm.joinable()) c->warm.join();
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  if (c->scratch) hipFree(c->scratch);
  for (auto& sp : c->spans) {
    hipEventDestroy(sp.a);
    hipEventDestroy(sp.b);
  }
  for (auto e : c->pool) hipEventDestroy(e);
  for (hipStream_t p : c->preps) {
    hipStreamSynchronize(p);
    hipStreamDestroy(p);
  }
  if (c->parse) {
    hipStreamSynchronize(c->parse);
    hipStreamDestroy(c->parse);
  }
  if (c->own_stream) hipStreamDestroy(c->stream);
  delete c;
  return DFH_OK;
}

int dfh_ctx_sync(dfh_ctx* c) {
  DFH_ARG(c, "ctx is NULL");
  return sync_all(c);
}

int dfh_ctx_set_pipeline(dfh_ctx* c, int enable) {
  DFH_ARG(c, "ctx is NULL");
  DFH_ARG(enable >= 0 && enable <= 4, "dfh_ctx_set_pipeline: 0 (off) .. 4 preparation streams");
  if (c->single_queue && enable) {  // the single-queue step has no preparation stream; minibatches are still prepared ahead
    return DFH_OK;
  }
  int rc = sync_all(c);
  if (rc) return rc;
  while ((int)c->preps.size() < enable) {
    // lowest priority: the main stream (lookup -> forward -> backward) is the critical path of a
    // step; the preparation of later batches has a whole step (or two) of slack and fills the gaps
    // (measured: highest 72.9, normal 72.7, lowest 75.8 M examples/sec)
    int lo = 0, hi = 0;
    DFH_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    const int prio = c->prep_priority < 0 ? lo : (c->prep_priority > 0 ? hi : 0);
    hipStream_t p = nullptr;
    DFH_HIP(hipStreamCreateWithPriority(&p, hipStreamNonBlocking, prio));
    c->preps.push_back(p);
  }
  c->nprep = (unsigned)enable;
  c->next_prep = 0;
  c->pipeline = enable != 0;
  return DFH_OK;
}
int dfh_ctx_set_option(dfh_ctx* c, const char* name, int value) {
  DFH_ARG(c && name, "dfh_ctx_set_option: NULL argument");
  const std::string n(name);
  for (const IntOption& o : kIntOptions) {
    if (n != o.name) continue;
    DFH_ARG(value >= o.lo && value <= o.hi, o.msg);
    c->*o.field = value;
    return DFH_OK;
  }
  if (n == "fwd_depth") {
    DFH_ARG(value == 4 || value == 5 || value == 8 || value == 10, "fwd_depth must be 4, 5, 8 or 10");
    c->fwd_depth = value;
  } else if (n == "single_queue") {
    DFH_ARG(value == 0 || value == 1, "single_queue must be 0 (preparation streams) or 1 (the Localizer's stages ride in the step's launches)");
    if (value != c->single_queue) {
      for (dfh_batch* p : std::vector<dfh_batch*>(c->pend)) {
        int rcf = flush_pending(p);
        if (rcf) return rcf;
      }
      int rcs = sync_all(c);
      if (rcs) return rcs;
      if (value) {  // one queue: no preparation streams
        c->nprep = 0;
        c->next_prep = 0;
        c->pipeline = false;
      }
      c->single_queue = value;
    }
  } else if (n == "rider_slot_count" || n == "rider_slot_scatter" || n == "rider_slot_sort" || n == "rider_slot_emit") {
    // which launch of a step carries the stage: 0 lookup, 1 forward, 2 update; + 4: as a launch of its own just before it
    DFH_ARG(value >= 0 && value <= 6 && (value & 3) <= 2, "rider_slot_*: 0 lookup, 1 forward, 2 update (+ 4: alone, before that launch)");
    const int st = n == "rider_slot_count" ? 0 : n == "rider_slot_scatter" ? 1 : n == "rider_slot_sort" ? 2 : 3;
    c->rider_slot[st] = value & 3;
    c->rider_alone[st] = (value >> 2) & 1;
  } else if (n == "rider_start_lookup" || n == "rider_start_forward" || n == "rider_start_update") {
    DFH_ARG(value >= 0 && value <= 100, "rider_start_*: per cent of the carrier's own blocks dispatched before the first rider group");
    c->rider_start[n == "rider_start_lookup" ? 0 : n == "rider_start_forward" ? 1 : 2] = value;
  } else if (n == "rider_period_lookup" || n == "rider_period_forward" || n == "rider_period_update") {
    DFH_ARG(value >= 1 && value <= 4096, "rider_period_*: one group of 8 rider blocks every n groups (1: riders first)");
    c->rider_period[n == "rider_period_lookup" ? 0 : n == "rider_period_forward" ? 1 : 2] = value;
  } else if (n == "prep_priority") {
    DFH_ARG(value >= -1 && value <= 1, "prep_priority must be -1 (lowest), 0 (default) or 1 (highest)");
    DFH_ARG(c->preps.empty(), "prep_priority must be set before dfh_ctx_set_pipeline creates the streams");
    c->prep_priority = value;
  } else {
    set_error("dfh_ctx_set_option: unknown option " + n);
    return DFH_ERR_ARG;
  }
  return DFH_OK;
}
void* dfh_ctx_stream(dfh_ctx* c) { return c ? c->stream : nullptr; }
int dfh_ctx_device(dfh_ctx* c) { return c ? c->device : -1; }

int dfh_ctx_set_timing(dfh_ctx* c, int enable) {
  DFH_ARG(c, "ctx is NULL");
  c->timing = enable ? ~0u : 0u;
  return DFH_OK;
}

int dfh_ctx_set_timing_mask(dfh_ctx* c, uint32_t mask) {
  DFH_ARG(c, "ctx is NULL");
  c->timing = mask;
  return DFH_OK;
}

int dfh_ctx_get_timing(dfh_ctx* c, int reset, double* total_ms, uint64_t* calls) {
  DFH_ARG(c, "ctx is NULL");
  {
    int rc = sync_all(c);
    if (rc) return rc;
  }
  if (getenv("DFH_GAP_TRACE") && c->spans.size() > 1) {
    double g[DFH_K_COUNT][DFH_K_COUNT] = {};
    uint64_t n[DFH_K_COUNT][DFH_K_COUNT] = {};
    const dfh_ctx::Span* prev = nullptr;  // the main stream's launches only: lookup (its own events), forward, update
    for (const auto& sp : c->spans) {
      const bool main_launch = sp.ride || sp.id == DFH_K_FORWARD || sp.id == DFH_K_BACKWARD;
      if (!main_launch) continue;
      float ms = 0;
      if (prev && hipEventElapsedTime(&ms, prev->b, sp.a) == hipSuccess) {
        g[prev->id][sp.id] += ms;
        n[prev->id][sp.id] += 1;
      }
      prev = &sp;
    }
    for (int x = 0; x < DFH_K_COUNT; ++x)
      for (int y = 0; y < DFH_K_COUNT; ++y)
        if (n[x][y])
          fprintf(stderr, "gap trace: end of %s -> start of %s: %.2f us on average (%llu pairs)\n", dfh_kernel_name(x), dfh_kernel_name(y),
                  g[x][y] / n[x][y] * 1e3, (unsigned long long)n[x][y]);
  }
  for (auto& sp : c->spans) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
      c->t_ms[sp.id] += ms;
      c->t_calls[sp.id] += 1;
    }
    c->pool.push_back(sp.a);
    c->pool.push_back(sp.b);
  }
  c->spans.clear();
  for (int i = 0; i < DFH_K_COUNT; ++i) {
    if (total_ms) total_ms[i] = c->t_ms[i];
    if (calls) calls[i] = c->t_calls[i];
    if (reset) {
      c->t_ms[i] = 0;
      c->t_calls[i] = 0;
    }
  }
  return DFH_OK;
}

const char* dfh_kernel_name(int id) {
  static const char* names[DFH_K_COUNT] = {"localize", "lookup", "forward", "backward", "pull_rows", "push_grad", "misc", "auc"};
  return (id >= 0 && id < DFH_K_COUNT) ? names[id] : "?";
}

int dfh_malloc(dfh_ctx* c, size_t bytes, void** dptr) {
  DFH_ARG(c && dptr, "dfh_malloc: NULL argument");
  DFH_HIP(hipSetDevice(c->device));
  DFH_HIP(hipMalloc(dptr, std::max<size_t>(bytes, 16)));
  return DFH_OK;
}
int dfh_free(dfh_ctx* c, void* dptr) {
  DFH_ARG(c, "ctx is NULL");
  if (dptr) DFH_HIP(hipFree(dptr));
  return DFH_OK;
}
int dfh_memcpy_h2d(dfh_ctx* c, void* dst, const void* src, size_t bytes) {
  DFH_ARG(c, "ctx is NULL");
  DFH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  return DFH_OK;
}
int dfh_memcpy_d2h(dfh_ctx* c, void* dst, const void* src, size_t bytes) {
  DFH_ARG(c, "ctx is NULL");
  DFH_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  DFH_HIP(hipStreamSynchronize(c->stream));
  return DFH_OK;
}
}  // extern "C"
