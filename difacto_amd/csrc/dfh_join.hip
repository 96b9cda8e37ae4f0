// dfh_join.hip — the device-side join of a loaded model onto a learner's own key order (included in dfh_api.hip before
// dfh_lbfgs.hip and dfh_bcd.hip): what dfh_lbfgs_set_model and dfh_bcd_set_model share.
//
// The learner's keys are ascending and unique; the input keys come in any order.  One lane per input key searches the
// learner's key array (k_join_match): pos[i] = the key's model position, -1 when the model does not hold it.  The input
// keys must be unique: a sorted copy (rocprim radix sort) is scanned for equal neighbours (k_join_dups).  The only
// atomics are integer counters; nothing here depends on the order in which lanes run.
namespace dfh {
namespace join {

constexpr int THREADS = 256;

// counters[0] += input keys found in the model
__global__ void __launch_bounds__(THREADS) k_join_match(const uint64_t* __restrict__ mkeys, uint64_t K, const uint64_t* __restrict__ in,
                                                        uint64_t n, int32_t* __restrict__ pos, unsigned long long* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  bool hit = false;
  if (i < n) {
    const uint64_t key = in[i];
    uint64_t lo = 0, hi = K;   // the first model key >= key
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (mkeys[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    hit = lo < K && mkeys[lo] == key;
    pos[i] = hit ? (int32_t)lo : -1;
  }
  const uint64_t ball = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && ball) atomicAdd(counters, (unsigned long long)__popcll(ball));
}

// counters[1] += positions of the sorted input whose key repeats the one before
__global__ void __launch_bounds__(THREADS) k_join_dups(const uint64_t* __restrict__ sorted, uint64_t n,
                                                       unsigned long long* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  const bool dup = i >= 1 && i < n && sorted[i] == sorted[i - 1];
  const uint64_t ball = __ballot(dup);
  if ((threadIdx.x & 63) == 0 && ball) atomicAdd(counters + 1, (unsigned long long)__popcll(ball));
}

struct Result {
  char* mem = nullptr;       // one allocation: the caller frees it (hipFree) once pos / extra are no longer read
  int32_t* pos = nullptr;    // [n] device: model position of every input key, -1 = not in the model
  char* extra = nullptr;     // [extra_bytes] device, 256-byte aligned: the caller's payload
  uint64_t matched = 0, dups = 0;
};

// mkeys [K] (host, ascending, unique), keys [n] (host, n >= 1).  Synchronises.
inline int run(dfh_ctx* c, const uint64_t* mkeys, size_t K, const uint64_t* keys, size_t n, size_t extra_bytes, Result* out) {
  DFH_ARG(K < (size_t(1) << 31) && n < (size_t(1) << 31), "model join: fewer than 2^31 model keys and input keys");
  hipStream_t s = c->stream;
  size_t sort_tmp = 0;
  DFH_HIP(rocprim::radix_sort_keys(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, 64, s));
  auto pad = [](size_t b) { return (std::max<size_t>(b, 1) + 255) / 256 * 256; };
  const size_t bytes = pad(K * 8) + 2 * pad(n * 8) + pad(n * 4) + pad(16) + pad(sort_tmp) + pad(extra_bytes);
  size_t free_b = 0, total_b = 0;
  DFH_HIP(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b) {
    char buf[160];
    snprintf(buf, sizeof(buf), "model join: needs %zu bytes of HBM, %zu are free", bytes, free_b);
    set_error(buf);
    return DFH_ERR_CAPACITY;
  }
  DFH_HIP(hipMalloc(reinterpret_cast<void**>(&out->mem), bytes));
  Carver cv(out->mem);   // an empty piece still gets 256 bytes of its own, as bytes counts it (pad)
  uint64_t* d_mkeys = cv.take<uint64_t>(std::max<size_t>(K, 1));
  uint64_t* d_in = cv.take<uint64_t>(n);
  uint64_t* d_sorted = cv.take<uint64_t>(n);
  out->pos = cv.take<int32_t>(n);
  unsigned long long* d_cnt = cv.take<unsigned long long>(2);
  void* d_tmp = cv.take<char>(std::max<size_t>(sort_tmp, 1));
  out->extra = cv.take<char>(extra_bytes);
  unsigned long long h_cnt[2] = {0, 0};
  const int grid = (int)((n + THREADS - 1) / THREADS);
  int rc = DFH_OK;
  do {
    if ((K && hipMemcpyAsync(d_mkeys, mkeys, K * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
        hipMemcpyAsync(d_in, keys, n * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d_cnt, 0, 16, s) != hipSuccess) {
      rc = DFH_ERR_HIP;
      break;
    }
    hipLaunchKernelGGL(k_join_match, dim3(grid), dim3(THREADS), 0, s, d_mkeys, (uint64_t)K, d_in, (uint64_t)n, out->pos, d_cnt);
    size_t tsz = sort_tmp;
    if (rocprim::radix_sort_keys(d_tmp, tsz, d_in, d_sorted, n, 0, 64, s) != hipSuccess) {
      rc = DFH_ERR_HIP;
      break;
    }
    hipLaunchKernelGGL(k_join_dups, dim3(grid), dim3(THREADS), 0, s, d_sorted, (uint64_t)n, d_cnt);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h_cnt, d_cnt, 16, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = DFH_ERR_HIP;
  } while (0);
  if (rc) {
    (void)hipFree(out->mem);
    *out = Result();
    set_error("model join: matching the input keys on the device failed");
    return rc;
  }
  out->matched = h_cnt[0];
  out->dups = h_cnt[1];
  return DFH_OK;
}

}  // namespace join
}  // namespace dfh
