// dfh_feed.hip — the device feed of the SGD worker loop (included in dfh_api.hip ahead of dfh_batch.hip, whose load calls
// share its staging helpers).  The shuffle buffer of BatchReader (src/reader/batch_reader.cc:38-52) lives in HBM as a row
// buffer (dfh_rowbuf); a minibatch is DESCRIBED by row numbers — the host sends 4 B per row instead of copying ~300 B per row
// twice (batch_reader.cc:53-63) — in the batch object's page-locked staging block, which the device reads in place
// (dfh_feed_layout.h), and its rows are gathered on the device: by the Localizer's count pass, or by k_gather_rows_staged
// where that pass cannot.  dfh_batch_prepare_rows / _cached are what a worker loop queues per minibatch
// (src/sgd/sgd_learner.cc:196-224: read, localize, pull); a slice without values beside slices with values holds ones
// (compressed_row_block.h:36-44).
struct dfh_rowbuf {
  dfh_ctx* ctx = nullptr;
  size_t max_rows = 0, max_nnz = 0, nrows = 0, nnz = 0;
  uint32_t* d_off = nullptr;   // [max_rows + 1]
  uint64_t* d_idx = nullptr;   // [max_nnz]
  float* d_val = nullptr;      // [max_nnz]
  float* d_lab = nullptr;      // [max_rows] the rows' labels (dfh_rowbuf_set_labels: allocated by the first call)
  bool has_value = false, has_labels = false;
  hipStream_t up = nullptr;    // uploads: the feed thread's own stream
  hipEvent_t ev_loaded = nullptr;
  // one "gathered" event per stream that has gathered out of this buffer (the two batch objects of a worker loop gather on
  // different preparation streams: one shared event would only remember the LAST gather); `pending` marks the ones
  // recorded since the last upload.  Set by the thread that gathers, read by the thread that uploads.
  struct Used { hipStream_t stream; hipEvent_t ev; bool pending; };
  std::mutex mu;
  std::vector<Used> used;
  std::vector<hipStream_t> seen_loaded;  // streams ordered behind the current upload already (one wait per stream and upload)
  double t_prof[3] = {0, 0, 0};          // DFH_PROFILE_PREP: host seconds of dfh_rowbuf_load_host (offsets, queue, wait)
  uint64_t n_prof = 0, bytes_prof = 0;
  std::vector<uint32_t> off32;
};

namespace {
// DFH_PROFILE_PREP: host seconds by section of a call, added up in acc[]
struct PrepLaps {
  double* acc;
  bool on;
  double tp;
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  explicit PrepLaps(double* a) : acc(a) {
    static const bool prof = getenv("DFH_PROFILE_PREP") != nullptr;
    on = prof;
    tp = on ? now() : 0;
  }
  void lap(int k) {
    if (!on) return;
    const double x = now();
    acc[k] += x - tp;
    tp = x;
  }
};

// page-locked staging of a batch object, sized for what the calling path puts there: a minibatch DESCRIBED by row numbers
// needs offsets + labels + row numbers (~160 KB), dfh_batch_load_host the ids and values too (9 MB at C3's sizes — 2.4 ms
// of hipHostMalloc each, which the worker loop's twelve batch objects paid on their first minibatch before round 4).
// mapped: the device reads the block in place (d_stage_view)
int ensure_stage(dfh_batch* b, size_t need, bool mapped) {
  if (!b->h_stage || b->stage_bytes < need) {
    if (b->h_stage) {
      if (b->staged_pending) DFH_HIP(hipEventSynchronize(b->ev_staged));
      b->staged_pending = false;
      DFH_HIP(hipHostFree(b->h_stage));
      b->h_stage = nullptr;
      b->d_stage_view = nullptr;
    }
    DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->h_stage), need, hipHostMallocDefault));
    b->stage_bytes = need;
    if (!b->ev_staged) DFH_HIP(hipEventCreateWithFlags(&b->ev_staged, hipEventDisableTiming));
  }
  if (mapped && !b->d_stage_view) DFH_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->d_stage_view), b->h_stage, 0));
  return DFH_OK;
}
// the previous minibatch staged here has been read (long ago: this wait is a formality)
int stage_wait(dfh_batch* b) {
  if (!b->staged_pending) return DFH_OK;
  // (a query first: hipEventSynchronize costs ~100 us of host time even on an event that completed long ago)
  if (hipEventQuery(b->ev_staged) != hipSuccess) DFH_HIP(hipEventSynchronize(b->ev_staged));
  b->staged_pending = false;
  return DFH_OK;
}
// a new phase on the object's own arrays (dfh_batch_attach_device points them elsewhere)
int phase_own_arrays(dfh_batch* b) {
  phase_begin(b);
  int rc = prep_begin(b);
  if (rc) return rc;
  b->d_raw = b->o_raw; b->d_offset = b->o_offset; b->d_value = b->o_value; b->d_label = b->o_label;
  return DFH_OK;
}
// a new minibatch is in (or on its way into) the object: nothing derived from the previous one holds
void batch_loaded(dfh_batch* b, size_t nrows, size_t nnz, bool has_value) {
  b->nrows = nrows;
  b->nnz = nnz;
  b->has_value = has_value;
  b->has_cnt = false;
  b->localized = false;
  b->looked_up = nullptr;
}

__global__ void k_fill_f32(float* __restrict__ p, size_t n, float v) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

// The body of the uploads: `offset` [nrows + 1] are the buffer's own (cumulative) offsets, the ids / values arrive as
// `nslices` pieces that follow one another (slice g: nnz ids at index, values at value; with has_value, a slice without a
// value array holds ones; a slice that names a parsed text chunk takes its ids from [first, first + nnz) of the chunk's ids
// in HBM, which dfh_textchunk_parse_criteo has completed).  One copy per piece, straight out of the caller's arrays, which
// are free on return.
int rowbuf_upload(const char* name, dfh_rowbuf* rb, size_t nrows, const size_t* offset, int nslices, const dfh_slice* slices, bool has_value) {
  const size_t base = offset[0], nnz = offset[nrows] - base;
  DFH_HIP(hipSetDevice(rb->ctx->device));
  {
    // every gather out of the previous contents, on whichever stream it was queued, precedes the copies below
    std::lock_guard<std::mutex> lk(rb->mu);
    for (auto& u : rb->used) {
      if (!u.pending) continue;
      DFH_HIP(hipStreamWaitEvent(rb->up, u.ev, 0));
      u.pending = false;
    }
    rb->seen_loaded.clear();
  }
  PrepLaps laps(rb->t_prof);
  rb->off32.resize(nrows + 1);
  for (size_t i = 0; i <= nrows; ++i) {
    DFH_ARG(offset[i] >= base && (i == 0 || offset[i] >= offset[i - 1]), std::string(name) + ": offsets must not decrease");
    rb->off32[i] = (uint32_t)(offset[i] - base);
  }
  laps.lap(0);
  DFH_HIP(hipMemcpyAsync(rb->d_off, rb->off32.data(), (nrows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, rb->up));
  size_t at = 0;
  for (int g = 0; g < nslices; ++g) {
    const dfh_slice& sl = slices[g];
    const size_t n = sl.nnz;
    if (!n) continue;
    if (sl.chunk) {
      DFH_HIP(hipMemcpyAsync(rb->d_idx + at, sl.chunk->d_ids + sl.first, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, rb->up));
    } else {
      DFH_HIP(hipMemcpyAsync(rb->d_idx + at, sl.index, n * sizeof(uint64_t), hipMemcpyHostToDevice, rb->up));
    }
    if (has_value && !sl.chunk && sl.value) {
      DFH_HIP(hipMemcpyAsync(rb->d_val + at, sl.value, n * sizeof(float), hipMemcpyHostToDevice, rb->up));
    } else if (has_value) {
      hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, rb->up, rb->d_val + at, n, 1.0f);
      DFH_HIP(hipGetLastError());
    }
    at += n;
  }
  DFH_HIP(hipEventRecord(rb->ev_loaded, rb->up));
  laps.lap(1);
  DFH_HIP(hipStreamSynchronize(rb->up));   // the caller's arrays are free again
  laps.lap(2);
  if (laps.on) {
    ++rb->n_prof;
    rb->bytes_prof += nnz * (has_value ? 12 : 8) + nrows * 4;
  }
  rb->nrows = nrows;
  rb->nnz = nnz;
  rb->has_value = has_value;
  rb->has_labels = false;   // (they were the previous contents')
  return DFH_OK;
}

// this stream has gathered out of the buffer: the next upload waits for it
int rowbuf_mark_used(dfh_rowbuf* rb, hipStream_t s) {
  std::lock_guard<std::mutex> lk(rb->mu);
  dfh_rowbuf::Used* u = nullptr;
  for (auto& x : rb->used)
    if (x.stream == s) u = &x;
  if (!u) {
    hipEvent_t ev = nullptr;
    DFH_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    rb->used.push_back({s, ev, false});
    u = &rb->used.back();
  }
  DFH_HIP(hipEventRecord(u->ev, s));
  u->pending = true;
  return DFH_OK;
}

// The description of the minibatch (row numbers, offsets, labels) is read where the host wrote it — page-locked host memory
// mapped into the device's address space — coalesced, and passed on: the minibatch's own offsets / labels land in HBM by the
// same kernel that gathers its rows, no copy is queued.  (A cached minibatch's have been derived into HBM already: h_off /
// h_lab then ARE dst_off / dst_lab.)
__global__ void __launch_bounds__(256) k_gather_rows_staged(const uint32_t* __restrict__ src_off, const uint64_t* __restrict__ src_idx,
                                                            const float* __restrict__ src_val, const uint32_t* __restrict__ h_rows,
                                                            const uint32_t* __restrict__ h_off, const float* __restrict__ h_lab, uint32_t n,
                                                            uint32_t* __restrict__ dst_off, float* __restrict__ dst_lab,
                                                            uint64_t* __restrict__ dst_idx, float* __restrict__ dst_val, int write_end) {
  // GR rows per block and pass: few enough that a minibatch spreads over the whole chip (10 000 rows = 313 blocks; 256
  // rows per block left 216 of the 256 CUs idle and took 92 us), enough that the description is read in 128 B pieces
  constexpr uint32_t GR = 32;
  __shared__ uint32_t s_lo[GR], s_len[GR], s_d0[GR];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  for (uint32_t q0 = blockIdx.x * GR; q0 < n; q0 += gridDim.x * GR) {
    const uint32_t m = min(GR, n - q0);
    __syncthreads();
    if (threadIdx.x < m) {
      const uint32_t q = q0 + threadIdx.x;
      const uint32_t r = h_rows[q], o = h_off[q];
      const uint32_t lo = src_off[r];
      s_lo[threadIdx.x] = lo;
      s_len[threadIdx.x] = src_off[r + 1] - lo;
      s_d0[threadIdx.x] = o;
      dst_off[q] = o;
      dst_lab[q] = h_lab[q];
    }
    if (threadIdx.x == 255 && write_end && q0 + m == n) dst_off[n] = h_off[n];
    __syncthreads();
    for (uint32_t t = w; t < m; t += 4u) {   // 8 rows per wave, independent addresses: the copies overlap
      const uint32_t lo = s_lo[t], len = s_len[t], d0 = s_d0[t];
      for (uint32_t j = lane; j < len; j += 64u) {
        dst_idx[d0 + j] = src_idx[lo + j];
        if (dst_val) dst_val[d0 + j] = src_val ? src_val[lo + j] : 1.0f;   // a buffer without values holds ones
      }
    }
  }
}

// after the launch(es) that read a described minibatch's rows out of their buffers have been queued on s: the buffers may be
// refilled, the page-locked description rewritten, once those launches are through
int gather_queued(dfh_batch* b, hipStream_t s) {
  for (const auto& g : b->gsegs) {
    int rc = rowbuf_mark_used(g.rb, s);
    if (rc) return rc;
  }
  DFH_HIP(hipEventRecord(b->ev_staged, s));   // the page-locked block may be rewritten once the launches have read it
  b->staged_pending = true;
  b->gather_pending = false;
  return DFH_OK;
}
// the rows of a described minibatch by launches of their own (k_gather_rows_staged): where the count pass cannot gather
int gather_alone(dfh_batch* b, hipStream_t s) {
  for (const auto& g : b->gsegs) {
    dfh_rowbuf* rb = g.rb;
    const unsigned blocks = (unsigned)std::min<size_t>((g.n + 31) / 32, 2048);
    hipLaunchKernelGGL(k_gather_rows_staged, dim3(blocks), dim3(256), 0, s, rb->d_off, rb->d_idx,
                       rb->has_value ? rb->d_val : (const float*)nullptr, b->g_rows + g.at, b->g_off + g.at, b->g_lab + g.at, (uint32_t)g.n,
                       b->d_offset + g.at, b->d_label + g.at, b->d_raw, b->gather_any_value ? b->d_value : (float*)nullptr,
                       g.at + g.n == b->nrows ? 1 : 0);
  }
  DFH_HIP(hipGetLastError());
  return gather_queued(b, s);
}

// what the segments of a described minibatch add up to
struct SegSum {
  bool any_value = false;   // one of the buffers carries values: the minibatch has a value array (the others' rows hold ones)
  size_t used = 0;          // segments with rows
  size_t nblk = 0;          // blocks of k_loc_describe, one launch per segment
};
// the segments of entry point `name`: buffers of the batch's context (with their labels: the cached form), row numbers where
// there are rows, nrows rows in all
int check_segments(const char* name, const dfh_batch* b, int nseg, dfh_rowbuf* const* bufs, const uint32_t* const* rows,
                   const size_t* seg_rows, size_t nrows, bool need_labels, SegSum* sum) {
  size_t total = 0;
  for (int g = 0; g < nseg; ++g) {
    DFH_ARG(bufs[g] && bufs[g]->ctx == b->ctx && (seg_rows[g] == 0 || rows[g]), std::string(name) + ": bad segment");
    DFH_ARG(!need_labels || (bufs[g]->has_labels && bufs[g]->off32.size() == bufs[g]->nrows + 1),
            std::string(name) + ": a row buffer without labels (dfh_rowbuf_set_labels)");
    total += seg_rows[g];
    sum->nblk += (seg_rows[g] + LOC_DESC_ROWS - 1) / LOC_DESC_ROWS;
    sum->used += seg_rows[g] != 0;
    sum->any_value = sum->any_value || bufs[g]->has_value;
  }
  DFH_ARG(total == nrows, std::string(name) + ": the segments must hold nrows rows");
  return DFH_OK;
}

// offsets | labels | row numbers of a minibatch the caller describes in full, into the batch's staging block (waited for)
int write_description(const char* name, dfh_batch* b, size_t nrows, const size_t* offset, const float* label, int nseg,
                      dfh_rowbuf* const* bufs, const uint32_t* const* rows, const size_t* seg_rows) {
  const StageLayout& L = b->stage;
  const size_t base = offset[0];
  uint32_t* h_off = reinterpret_cast<uint32_t*>(b->h_stage + L.o_off);
  for (size_t i = 0; i <= nrows; ++i) {
    DFH_ARG(offset[i] >= base && (i == 0 || offset[i] >= offset[i - 1]), std::string(name) + ": offsets must not decrease");
    h_off[i] = (uint32_t)(offset[i] - base);
  }
  memcpy(b->h_stage + L.o_lab, label, nrows * 4);
  uint32_t* h_rows = reinterpret_cast<uint32_t*>(b->h_stage + L.o_idx);
  size_t at = 0;
  for (int g = 0; g < nseg; ++g) {
    const uint32_t lim = (uint32_t)bufs[g]->nrows;
    const uint32_t* src = rows[g];
    uint32_t worst = 0;
    for (size_t i = 0; i < seg_rows[g]; ++i) {
      h_rows[at + i] = src[i];
      worst = std::max(worst, src[i]);
    }
    DFH_ARG(seg_rows[g] == 0 || worst < lim, std::string(name) + ": row number beyond the buffer");
    at += seg_rows[g];
  }
  return DFH_OK;
}

// A described minibatch whose description lies in the batch's page-locked block, as the device sees it (v_*).  `v_base`
// (cached only): the minibatch's offsets and labels are not part of the description; k_loc_describe derives them first, into
// the minibatch's own arrays, and the gather reads them there (v_off / v_lab are NULL).
struct DescribedIn {
  size_t nrows, nnz;
  int nseg;
  dfh_rowbuf* const* bufs;
  const size_t* seg_rows;
  bool any_value;
  const uint32_t *v_rows, *v_off;
  const float* v_lab;
  const uint32_t* v_tile;
  bool fusable;
  const uint32_t* v_base;
};
// the description as in.v_* of the staging block as the device sees it
DescribedIn described(const dfh_batch* b, size_t nrows, size_t nnz, int nseg, dfh_rowbuf* const* bufs, const size_t* seg_rows,
                      const SegSum& sum, bool fusable, bool cached) {
  const StageLayout& L = b->stage;
  const char* v = b->d_stage_view;
  return DescribedIn{nrows, nnz, nseg, bufs, seg_rows, sum.any_value, reinterpret_cast<const uint32_t*>(v + L.o_idx),
                     cached ? nullptr : reinterpret_cast<const uint32_t*>(v + L.o_off),
                     cached ? nullptr : reinterpret_cast<const float*>(v + L.o_lab), reinterpret_cast<const uint32_t*>(v + L.o_tile),
                     fusable, cached ? reinterpret_cast<const uint32_t*>(v + L.o_base) : nullptr};
}

// The gather of a described minibatch is NOTED, on the preparation stream behind the buffers' uploads: the rows stay where
// they are until the Localizer's count pass gathers them as it reads them (k_loc_count_gather), or gather_alone does where
// that pass cannot (see dfh_batch::gsegs).  The object then holds a loaded minibatch with gather_pending set.
int describe(dfh_batch* b, const DescribedIn& in) {
  hipStream_t s = prep_of(b);
  const size_t nrows = in.nrows;
  const bool cached = in.v_base != nullptr;
  b->gsegs.clear();
  size_t at = 0, blk0 = 0;
  for (int g = 0; g < in.nseg; ++g) {
    dfh_rowbuf* rb = in.bufs[g];
    const size_t n = in.seg_rows[g];
    if (n == 0) continue;
    bool waited;
    {
      std::lock_guard<std::mutex> lk(rb->mu);
      waited = std::find(rb->seen_loaded.begin(), rb->seen_loaded.end(), s) != rb->seen_loaded.end();
      if (!waited) rb->seen_loaded.push_back(s);
    }
    if (!waited) DFH_HIP(hipStreamWaitEvent(s, rb->ev_loaded, 0));
    if (cached) {
      const unsigned blocks = (unsigned)((n + LOC_DESC_ROWS - 1) / LOC_DESC_ROWS);
      hipLaunchKernelGGL(k_loc_describe, dim3(blocks), dim3(LOC_DESC_ROWS), 0, s, rb->d_off, rb->d_lab, in.v_rows + at, in.v_base + blk0,
                         (uint32_t)n, b->d_offset + at, b->d_label + at, at + n == nrows ? 1 : 0);
      blk0 += blocks;
    }
    b->gsegs.push_back({rb, at, n});
    at += n;
  }
  if (cached) DFH_HIP(hipGetLastError());
  const uint32_t* v_off = cached ? b->d_offset : in.v_off;
  const float* v_lab = cached ? b->d_label : in.v_lab;
  b->g_rows = in.v_rows;
  b->g_off = v_off;
  b->g_lab = v_lab;
  b->gather_any_value = in.any_value;
  b->gather_pending = true;
  GatherSrc& gs = b->gsrc;
  const bool ok = in.fusable;
  b->gather_fusable = ok;
  gs.nseg = (int)b->gsegs.size();
  for (int g = 0; g <= LOC_GATHER_SEGS; ++g) gs.seg_row0[g] = (uint32_t)nrows;
  for (int g = 0; g < LOC_GATHER_SEGS; ++g) {
    const bool have = g < gs.nseg && ok;
    gs.seg_row0[g] = have ? (uint32_t)b->gsegs[g].at : (uint32_t)nrows;
    gs.src_off[g] = have ? b->gsegs[g].rb->d_off : nullptr;
    gs.src_idx[g] = have ? b->gsegs[g].rb->d_idx : nullptr;
    gs.src_val[g] = (have && b->gsegs[g].rb->has_value) ? b->gsegs[g].rb->d_val : nullptr;
  }
  gs.h_rows = in.v_rows;
  gs.h_off = v_off;
  gs.h_lab = v_lab;
  gs.h_tile_row = in.v_tile;
  gs.dst_raw = b->d_raw;
  gs.dst_val = in.any_value ? b->d_value : nullptr;
  gs.dst_off = b->d_offset;
  gs.dst_lab = b->d_label;
  batch_loaded(b, nrows, in.nnz, in.any_value);
  return DFH_OK;
}

// describe, then Localizer::Compact + the key-index probe in the same phase, ONE ev_ready at the end
int queue_described(dfh_table* t, dfh_batch* b, const DescribedIn& in, uint64_t max_index, PrepLaps& laps) {
  dfh_ctx* c = b->ctx;
  int rc = describe(b, in);
  if (rc) return rc;
  laps.lap(3);  // gather queued
  b->defer_ready = true;
  rc = localize_impl(b, max_index, nullptr);
  laps.lap(4);  // Localizer queued
  if (!rc && in.nnz > kSmallBatchPairs && !c->single_queue) {   // (a small minibatch: the step's own pass probes, see dfh_batch_lookup)
    hipLaunchKernelGGL(k_lookup, dim3(grid_for_threads(b->nnz, c)), dim3(256), 0, prep_of(b), t->v, b->d_feaids, b->d_U, 0u, b->d_urow,
                       (const float*)nullptr, b->d_col_ptr, 0, (uint32_t*)nullptr, 0, (uint2*)nullptr, AucFin{nullptr, 0u, nullptr});
    if (hipGetLastError() != hipSuccess) rc = DFH_ERR_HIP;
    b->looked_up = t;
  }
  b->defer_ready = false;
  if (rc) return rc;
  rc = prep_end(b);
  laps.lap(5);  // lookup queued, ev_ready recorded
  if (laps.on) ++b->n_prof;
  return rc;
}
}  // namespace

extern "C" {

int dfh_rowbuf_create(dfh_ctx* c, size_t max_rows, size_t max_nnz, dfh_rowbuf** out) {
  DFH_ARG(c && out && max_rows >= 1 && max_nnz >= 1, "dfh_rowbuf_create: bad argument");
  DFH_ARG(max_nnz < 0xFFFFFFF0ULL && max_rows < 0xFFFFFFF0ULL, "dfh_rowbuf_create: a row buffer holds fewer than 2^32 rows / nonzeros");
  DFH_HIP(hipSetDevice(c->device));
  dfh_rowbuf* rb = new (std::nothrow) dfh_rowbuf();
  if (!rb) {
    set_error("dfh_rowbuf_create: out of host memory");
    return DFH_ERR_HIP;
  }
  rb->ctx = c;
  rb->max_rows = max_rows;
  rb->max_nnz = max_nnz;
  hipError_t e;
  if ((e = hipMalloc(reinterpret_cast<void**>(&rb->d_off), (max_rows + 1) * sizeof(uint32_t))) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&rb->d_idx), max_nnz * sizeof(uint64_t))) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&rb->d_val), max_nnz * sizeof(float))) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&rb->up, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&rb->ev_loaded, hipEventDisableTiming)) != hipSuccess) {
    set_error(std::string("dfh_rowbuf_create: ") + hipGetErrorString(e));
    dfh_rowbuf_destroy(rb);
    return DFH_ERR_HIP;
  }
  *out = rb;
  return DFH_OK;
}

int dfh_rowbuf_destroy(dfh_rowbuf* rb) {
  if (!rb) return DFH_OK;
  if (rb->n_prof)
    fprintf(stderr, "dfh_rowbuf_load_host x %llu (%.1f MB): offsets %.4f s, queue copies %.4f, wait %.4f\n", (unsigned long long)rb->n_prof,
            rb->bytes_prof / 1e6, rb->t_prof[0], rb->t_prof[1], rb->t_prof[2]);
  hipSetDevice(rb->ctx->device);
  // the gathers out of this buffer, wherever they were queued (NOT sync_all: this may run beside the thread that drives
  // the context, and only this buffer's own consumers matter)
  for (auto& u : rb->used) {
    if (u.pending) hipEventSynchronize(u.ev);
    hipEventDestroy(u.ev);
  }
  if (rb->up) {
    hipStreamSynchronize(rb->up);
    hipStreamDestroy(rb->up);
  }
  if (rb->ev_loaded) hipEventDestroy(rb->ev_loaded);
  for (void* p : {(void*)rb->d_off, (void*)rb->d_idx, (void*)rb->d_val, (void*)rb->d_lab})
    if (p) hipFree(p);
  delete rb;
  return DFH_OK;
}

int dfh_rowbuf_load_host(dfh_rowbuf* rb, size_t nrows, const size_t* offset, const uint64_t* index, const float* value) {
  DFH_ARG(rb && offset && nrows >= 1 && nrows <= rb->max_rows, "dfh_rowbuf_load_host: bad argument / more rows than the buffer holds");
  const size_t base = offset[0], nnz = offset[nrows] - base;
  DFH_ARG(nnz <= rb->max_nnz, "dfh_rowbuf_load_host: more nonzeros than the buffer holds");
  DFH_ARG(nnz == 0 || index, "dfh_rowbuf_load_host: index is NULL");
  // one slice; without a value array the buffer has no values (the gather reads its rows as ones)
  const dfh_slice sl{nnz ? index + base : nullptr, value ? value + base : nullptr, nullptr, 0, nnz};
  return rowbuf_upload("dfh_rowbuf_load_host", rb, nrows, offset, 1, &sl, value != nullptr);
}

// dfh_rowbuf_load_host for a buffer that was never assembled on the host: the buffer has values iff one of its slices has
int dfh_rowbuf_load_host_slices(dfh_rowbuf* rb, size_t nrows, const size_t* offset, int nslices, const uint64_t* const* index,
                                const float* const* value, const size_t* nnz_of) {
  DFH_ARG(rb && offset && nrows >= 1 && nrows <= rb->max_rows, "dfh_rowbuf_load_host_slices: bad argument / more rows than the buffer holds");
  DFH_ARG(nslices >= 0 && (nslices == 0 || (index && value && nnz_of)), "dfh_rowbuf_load_host_slices: NULL slice arrays");
  const size_t nnz = offset[nrows] - offset[0];
  DFH_ARG(nnz <= rb->max_nnz, "dfh_rowbuf_load_host_slices: more nonzeros than the buffer holds");
  size_t total = 0;
  bool any_value = false;
  std::vector<dfh_slice> slices((size_t)nslices);
  for (int g = 0; g < nslices; ++g) {
    DFH_ARG(nnz_of[g] == 0 || index[g], "dfh_rowbuf_load_host_slices: a slice without ids");
    total += nnz_of[g];
    any_value = any_value || (nnz_of[g] && value[g]);
    slices[g] = dfh_slice{index[g], value[g], nullptr, 0, nnz_of[g]};
  }
  DFH_ARG(total == nnz, "dfh_rowbuf_load_host_slices: the slices must hold the buffer's nonzeros");
  return rowbuf_upload("dfh_rowbuf_load_host_slices", rb, nrows, offset, nslices, slices.data(), any_value);
}

// dfh_rowbuf_load_host_slices where a slice may name the ids of a parsed text chunk (dfh_textparse.hip) instead of host arrays:
// those are copied device to device on the buffer's stream; such a slice has no values (ones beside slices with values)
int dfh_rowbuf_load_slices(dfh_rowbuf* rb, size_t nrows, const size_t* offset, int nslices, const dfh_slice* slices) {
  DFH_ARG(rb && offset && nrows >= 1 && nrows <= rb->max_rows, "dfh_rowbuf_load_slices: bad argument / more rows than the buffer holds");
  DFH_ARG(nslices >= 0 && (nslices == 0 || slices), "dfh_rowbuf_load_slices: NULL slice array");
  const size_t nnz = offset[nrows] - offset[0];
  DFH_ARG(nnz <= rb->max_nnz, "dfh_rowbuf_load_slices: more nonzeros than the buffer holds");
  size_t total = 0;
  bool any_value = false;
  for (int g = 0; g < nslices; ++g) {
    const dfh_slice& sl = slices[g];
    if (sl.chunk) {
      DFH_ARG(sl.chunk->ctx == rb->ctx && sl.chunk->valid && sl.first <= sl.chunk->nnz && sl.nnz <= sl.chunk->nnz - sl.first,
              "dfh_rowbuf_load_slices: a slice beyond the ids of its parsed chunk (or of a chunk that was not regular)");
    } else {
      DFH_ARG(sl.nnz == 0 || sl.index, "dfh_rowbuf_load_slices: a slice without ids");
      any_value = any_value || (sl.nnz && sl.value);
    }
    total += sl.nnz;
  }
  DFH_ARG(total == nnz, "dfh_rowbuf_load_slices: the slices must hold the buffer's nonzeros");
  return rowbuf_upload("dfh_rowbuf_load_slices", rb, nrows, offset, nslices, slices, any_value);
}

// The labels of the rows a row buffer holds (after dfh_rowbuf_load_host / _slices, same thread): with them — and its own
// offsets, which the buffer keeps on the device and, 4 B per row, on the host — a minibatch out of this buffer is described by
// its row numbers alone (dfh_batch_prepare_cached).  A reload drops them.
int dfh_rowbuf_set_labels(dfh_rowbuf* rb, size_t nrows, const float* label) {
  DFH_ARG(rb && label && nrows >= 1 && nrows == rb->nrows, "dfh_rowbuf_set_labels: one label per row of the loaded buffer");
  DFH_HIP(hipSetDevice(rb->ctx->device));
  if (!rb->d_lab) DFH_HIP(hipMalloc(reinterpret_cast<void**>(&rb->d_lab), rb->max_rows * sizeof(float)));
  DFH_HIP(hipMemcpyAsync(rb->d_lab, label, nrows * sizeof(float), hipMemcpyHostToDevice, rb->up));
  DFH_HIP(hipEventRecord(rb->ev_loaded, rb->up));   // whoever waits for the upload waits for the labels too
  DFH_HIP(hipStreamSynchronize(rb->up));            // the caller's array is free again
  {
    std::lock_guard<std::mutex> lk(rb->mu);
    rb->seen_loaded.clear();
  }
  rb->has_labels = true;
  return DFH_OK;
}

// The described path in three calls (this one, dfh_localize, dfh_batch_lookup): the gather runs here, as launches of its own,
// and leaves a loaded minibatch.  The DIFACTO_SPLIT_PREP A/B branch of the learner, and tests.
int dfh_batch_gather_rows(dfh_batch* b, size_t nrows, const size_t* offset, const float* label, int nseg, dfh_rowbuf* const* bufs,
                          const uint32_t* const* rows, const size_t* seg_rows) {
  DFH_ARG(b && offset && label && nseg >= 1 && bufs && rows && seg_rows, "dfh_batch_gather_rows: NULL argument");
  DFH_ARG(nrows >= 1 && nrows <= b->max_rows, "dfh_batch_gather_rows: nrows out of range");
  const size_t nnz = offset[nrows] - offset[0];
  DFH_ARG(nnz <= b->max_nnz && nnz < 0xFFFFFFFFULL, "dfh_batch_gather_rows: nnz exceeds max_nnz");
  SegSum sum;
  int rc = check_segments("dfh_batch_gather_rows", b, nseg, bufs, rows, seg_rows, nrows, false, &sum);
  if (rc) return rc;
  DFH_HIP(hipSetDevice(b->ctx->device));
  rc = phase_own_arrays(b);
  if (!rc) rc = ensure_stage(b, b->stage.rows_bytes(), true);
  if (!rc) rc = stage_wait(b);
  if (!rc) rc = write_description("dfh_batch_gather_rows", b, nrows, offset, label, nseg, bufs, rows, seg_rows);
  if (!rc) rc = describe(b, described(b, nrows, nnz, nseg, bufs, seg_rows, sum, false, false));
  if (!rc) rc = gather_alone(b, prep_of(b));
  return rc;
}

int dfh_batch_prepare_rows(dfh_table* t, dfh_batch* b, size_t nrows, const size_t* offset, const float* label, int nseg,
                           dfh_rowbuf* const* bufs, const uint32_t* const* rows, const size_t* seg_rows, uint64_t max_index) {
  DFH_ARG(t && b && t->ctx == b->ctx && offset && label && nseg >= 1 && bufs && rows && seg_rows, "dfh_batch_prepare_rows: NULL argument");
  DFH_ARG(nrows >= 1 && nrows <= b->max_rows, "dfh_batch_prepare_rows: nrows out of range");
  DFH_ARG(max_index != 0, "max_index must be nonzero");
  const size_t nnz = offset[nrows] - offset[0];
  DFH_ARG(nnz <= b->max_nnz && nnz < 0xFFFFFFFFULL, "dfh_batch_prepare_rows: nnz exceeds max_nnz");
  SegSum sum;
  int rc = check_segments("dfh_batch_prepare_rows", b, nseg, bufs, rows, seg_rows, nrows, false, &sum);
  if (rc) return rc;
  PrepLaps laps(b->t_prof);
  DFH_HIP(hipSetDevice(b->ctx->device));
  if (nnz) {
    int rcr = table_reserve(t, nnz);  // U <= nnz keys may be new; before anything of this phase is queued
    if (rcr) return rcr;
  }
  rc = phase_own_arrays(b);
  if (!rc) rc = ensure_stage(b, b->stage.rows_bytes(), true);
  if (rc) return rc;
  laps.lap(0);  // set-up, prep_begin (wait for the batch object's previous step)
  rc = stage_wait(b);
  if (rc) return rc;
  laps.lap(1);  // the previous description has been read
  rc = write_description("dfh_batch_prepare_rows", b, nrows, offset, label, nseg, bufs, rows, seg_rows);
  if (rc) return rc;
  laps.lap(2);  // description written
  // what the count pass needs on top: the first row of every tile, behind the row numbers in the same page-locked block
  uint32_t* h_tile = reinterpret_cast<uint32_t*>(b->h_stage + b->stage.o_tile);
  const size_t ntiles = tile_rows_fill(reinterpret_cast<const uint32_t*>(b->h_stage + b->stage.o_off), nrows, h_tile);
  const bool fusable = tile_rows_finish(h_tile, ntiles, nrows, nnz, sum.used);
  return queue_described(t, b, described(b, nrows, nnz, nseg, bufs, seg_rows, sum, fusable, false), max_index, laps);
}

// dfh_batch_prepare_rows for a minibatch out of buffers that carry their own labels (dfh_rowbuf_set_labels): the caller names
// the rows, nothing else.  The host's share: the row numbers into the page-locked block (4 B per row), and — read off the
// buffers' host-side offsets while it copies them — the minibatch's nnz (the launches that follow are sized by it), the running
// total at every 256th row of a segment (k_loc_describe's block bases) and the first row of every tile (the count pass's
// gather, as in dfh_batch_prepare_rows).  Offsets and labels are derived on the device (k_loc_describe, dfh_localize.hip).
int dfh_batch_prepare_cached(dfh_table* t, dfh_batch* b, size_t nrows, int nseg, dfh_rowbuf* const* bufs, const uint32_t* const* rows,
                             const size_t* seg_rows, uint64_t max_index) {
  DFH_ARG(t && b && t->ctx == b->ctx && nseg >= 1 && bufs && rows && seg_rows, "dfh_batch_prepare_cached: NULL argument");
  DFH_ARG(nrows >= 1 && nrows <= b->max_rows, "dfh_batch_prepare_cached: nrows out of range");
  DFH_ARG(max_index != 0, "max_index must be nonzero");
  SegSum sum;
  int rc = check_segments("dfh_batch_prepare_cached", b, nseg, bufs, rows, seg_rows, nrows, true, &sum);
  if (rc) return rc;
  PrepLaps laps(b->t_prof);
  DFH_HIP(hipSetDevice(b->ctx->device));
  const StageLayout& L = b->stage;
  rc = ensure_stage(b, L.cached_bytes(sum.nblk), true);
  if (!rc) rc = stage_wait(b);
  if (rc) return rc;
  laps.lap(1);  // the previous description has been read
  uint32_t* h_rows = reinterpret_cast<uint32_t*>(b->h_stage + L.o_idx);
  uint32_t* h_tile = reinterpret_cast<uint32_t*>(b->h_stage + L.o_tile);
  uint32_t* h_base = reinterpret_cast<uint32_t*>(b->h_stage + L.o_base);
  // h_tile[t] = the last row that starts at or before position t * LOC_TILE: when row q starts beyond it, that row is q - 1
  size_t at = 0, nnz = 0, nt = 0, nb = 0;
  const size_t tile_cap = b->max_tiles + 1;   // (a minibatch beyond max_nnz is refused below; its surplus tiles are not written)
  for (int g = 0; g < nseg; ++g) {
    const uint32_t lim = (uint32_t)bufs[g]->nrows;
    const uint32_t* src = rows[g];
    const uint32_t* off = bufs[g]->off32.data();
    for (size_t i = 0; i < seg_rows[g]; ++i) {
      const uint32_t r = src[i];
      DFH_ARG(r < lim, "dfh_batch_prepare_cached: row number beyond the buffer");
      h_rows[at + i] = r;
      if (i % LOC_DESC_ROWS == 0) h_base[nb++] = (uint32_t)nnz;
      while (nt * (size_t)LOC_TILE < nnz && nt < tile_cap) h_tile[nt++] = (uint32_t)(at + i - 1);
      nnz += off[r + 1] - off[r];
    }
    at += seg_rows[g];
  }
  DFH_ARG(nnz <= b->max_nnz && nnz < 0xFFFFFFFFULL, "dfh_batch_prepare_cached: nnz exceeds max_nnz");
  const size_t ntiles = (nnz + LOC_TILE - 1) / LOC_TILE;
  while (nt < ntiles) h_tile[nt++] = (uint32_t)(nrows - 1);
  const bool fusable = tile_rows_finish(h_tile, ntiles, nrows, nnz, sum.used);
  laps.lap(2);  // description written
  if (nnz) {
    int rcr = table_reserve(t, nnz);  // U <= nnz keys may be new; before anything of this phase is queued
    if (rcr) return rcr;
  }
  rc = phase_own_arrays(b);
  if (rc) return rc;
  laps.lap(0);  // prep_begin (wait for the batch object's previous step)
  return queue_described(t, b, described(b, nrows, nnz, nseg, bufs, seg_rows, sum, fusable, true), max_index, laps);
}

// the loaded minibatch's own offsets [nrows + 1] and labels [nrows] as the device holds them (tests: a described minibatch's
// are written by the gather, a cached one's derived by k_loc_describe).  Synchronises.
int dfh_batch_get_rows(dfh_batch* b, uint32_t* offset, float* label) {
  DFH_ARG(b && b->nrows > 0 && offset && label, "dfh_batch_get_rows: no batch loaded / NULL argument");
  DFH_HIP(hipSetDevice(b->ctx->device));
  int rc = sync_all(b->ctx);
  if (rc) return rc;
  DFH_HIP(hipMemcpy(offset, b->d_offset, (b->nrows + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  DFH_HIP(hipMemcpy(label, b->d_label, b->nrows * sizeof(float), hipMemcpyDeviceToHost));
  return DFH_OK;
}

}  // extern "C"
