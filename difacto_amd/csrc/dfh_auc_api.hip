// dfh_auc_api.hip — the launches of a minibatch's AUC (dfh_auc.hip), either form behind one function, for the two callers
// that make it a launch of its own: a step whose update launch does not carry it (launch_auc, dfh_step.hip) and the
// literal call on host arrays (dfh_auc_times_n); and the AUC a step's update launch left pending.
namespace {
// an AUC whose units have run (inside an update launch) but whose slots have not been added up yet
AucFin auc_pending(dfh_batch* b) { return AucFin{b->d_auc_part, b->auc_pending_n, b->d_prog + PROG_AUC * PROG_SLOTS}; }
int auc_flush_pending(dfh_batch* b) {
  if (!b->auc_pending_n) return DFH_OK;
  hipLaunchKernelGGL(k_auc_finalize, dim3(1), dim3(256), 0, b->ctx->stream, auc_pending(b));
  b->auc_pending_n = 0;
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// BinClassMetric::AUC * n of n predictions, added to *out_slot, on the context's stream.  part: AUC_PART_WORDS words;
// keys, skeys, lab, slab: n words each, and temp: what the sort of n pairs asks for — read only beyond AUC_PAIRS_MAX_N
int auc_launch(dfh_ctx* c, const float* pred, const float* label, uint32_t n, uint32_t* part, uint32_t* keys, uint32_t* skeys,
               uint32_t* lab, uint32_t* slab, void* temp, size_t temp_bytes, double* out_slot) {
  hipStream_t s = c->stream;
  if (n <= AUC_PAIRS_MAX_N) {
    // minibatch-sized: pair counting (auc_pairs_block units), then one block adds the units' slots up
    hipLaunchKernelGGL(k_auc_pairs, dim3(auc_units(n)), dim3(256), 0, s, pred, label, n, part);
    hipLaunchKernelGGL(k_auc_finalize, dim3(1), dim3(256), 0, s, AucFin{part, n, out_slot});
  } else {
    hipLaunchKernelGGL(k_auc_keys, dim3(grid_for_threads(n, c)), dim3(256), 0, s, pred, label, n, keys, lab);
    DFH_HIP(rocprim::radix_sort_pairs(temp, temp_bytes, keys, skeys, lab, slab, (size_t)n, 0, 32, s));
    hipLaunchKernelGGL(k_auc_area, dim3(1), dim3(1024), 0, s, slab, n, out_slot);
  }
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// BinClassMetric::AUC of the batch's predictions, accumulated into the progress block
int launch_auc(dfh_batch* b) {
  int rc = auc_flush_pending(b);  // the slots are about to be overwritten
  if (rc) return rc;
  // NB: d_temp is shared with the localizer's library-sort path, which only runs on the prep stream of
  // ANOTHER batch object; within one batch the step follows its own preparation
  return auc_launch(b->ctx, b->d_pred, b->d_label, (uint32_t)b->nrows, b->d_auc_part, b->d_auc_keys, b->d_auc_skeys, b->d_auc_lab,
                    b->d_auc_slab, b->d_temp, b->temp_bytes, b->d_prog + PROG_AUC * PROG_SLOTS);
}
}  // namespace

extern "C" {

int dfh_auc_times_n(dfh_ctx* c, const float* label, const float* pred, size_t n, float* auc_n) {
  DFH_ARG(c && auc_n, "NULL argument");
  *auc_n = 1.0f;
  if (n == 0) return DFH_OK;
  DFH_ARG(label && pred && n < 0xFFFFFFF0ULL, "dfh_auc_times_n: bad argument");
  DFH_HIP(hipSetDevice(c->device));
  size_t tb = 0;
  rocprim::radix_sort_pairs(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32,
                            c->stream);
  int rc = ensure_scratch(c, 2 * padded<float>(n) + 4 * padded<uint32_t>(n) + tb + padded<uint32_t>(AUC_PART_WORDS) + 2048);
  if (rc) return rc;
  Carver cv(c->scratch);
  float* d_l = cv.take<float>(n);
  float* d_p = cv.take<float>(n);
  double* d_o = cv.take<double>(1);
  uint32_t* d_part = cv.take<uint32_t>(AUC_PART_WORDS);
  uint32_t* k0 = cv.take<uint32_t>(n);
  uint32_t* k1 = cv.take<uint32_t>(n);
  uint32_t* l0 = cv.take<uint32_t>(n);
  uint32_t* l1 = cv.take<uint32_t>(n);
  char* temp = cv.take<char>(tb + 16);
  hipStream_t s = c->stream;
  DFH_HIP(hipMemcpyAsync(d_l, label, n * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(d_p, pred, n * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemsetAsync(d_o, 0, sizeof(double), s));
  rc = auc_launch(c, d_p, d_l, (uint32_t)n, d_part, k0, k1, l0, l1, temp, tb, d_o);
  if (rc) return rc;
  double o = 0;
  DFH_HIP(hipMemcpyAsync(&o, d_o, sizeof(double), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  *auc_n = (float)o;
  return DFH_OK;
}
}  // extern "C"
