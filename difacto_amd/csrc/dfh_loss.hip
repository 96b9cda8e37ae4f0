// dfh_loss.hip — the literal Loss calls on host pointers (FMLoss::Predict / CalcGrad, LogitLoss::Evaluate), staged through
// the context's scratch block; to_u32_offsets also serves the host load calls of dfh_batch.hip.
namespace {
int to_u32_offsets(const size_t* offset, size_t nrows, std::vector<uint32_t>* out) {
  out->resize(nrows + 1);
  const size_t base = offset[0];
  for (size_t i = 0; i <= nrows; ++i) {
    size_t o = offset[i] - base;
    DFH_ARG(o < 0xFFFFFFFFULL, "batch has >= 2^32 nonzeros (localizer.cc:19 CHECK_LT)");
    (*out)[i] = (uint32_t)o;
  }
  return DFH_OK;
}
}  // namespace

extern "C" {

int dfh_fm_predict(dfh_ctx* c, int V_dim, size_t nrows, const size_t* offset, const uint32_t* index, const float* value,
                   const float* weights, size_t nweights, const int* w_pos, const int* V_pos, size_t npos, float* pred) {
  DFH_ARG(c && V_dim >= 0, "dfh_fm_predict: bad argument");
  if (nrows == 0) return DFH_OK;
  DFH_ARG(offset && pred && weights, "dfh_fm_predict: NULL argument");
  DFH_ARG(V_dim == 0 || (w_pos && V_pos), "dfh_fm_predict: V_dim > 0 needs w_pos and V_pos");
  DFH_HIP(hipSetDevice(c->device));
  std::vector<uint32_t> off32;
  int rc = to_u32_offsets(offset, nrows, &off32);
  if (rc) return rc;
  const size_t base = offset[0];
  const size_t nnz = off32[nrows];
  DFH_ARG(nnz == 0 || index, "dfh_fm_predict: index is NULL");
  const size_t ncols = w_pos ? npos : nweights;
  for (size_t j = 0; j < nnz; ++j) DFH_ARG(index[base + j] < ncols, "dfh_fm_predict: index out of range");
  if (w_pos) {  // SpMV/SpMM::CheckPos (spmv.h:194-202, spmm.h:172-180)
    for (size_t u = 0; u < npos; ++u) {
      DFH_ARG(w_pos[u] == -1 || (w_pos[u] >= 0 && (size_t)w_pos[u] < nweights), "w_pos out of range");
      if (V_dim > 0) DFH_ARG(V_pos[u] == -1 || (V_pos[u] >= 0 && (size_t)V_pos[u] + V_dim <= nweights), "V_pos out of range");
    }
  }
  rc = ensure_scratch(c, padded<uint32_t>(nrows + 1) + padded<uint32_t>(nnz) + padded<float>(nnz) + padded<float>(nweights) +
                             2 * padded<int>(npos) + padded<float>(nrows));
  if (rc) return rc;
  Carver cv(c->scratch);
  uint32_t* d_off = cv.take<uint32_t>(nrows + 1);
  uint32_t* d_idx = cv.take<uint32_t>(std::max<size_t>(nnz, 1));
  float* d_val = cv.take<float>(std::max<size_t>(nnz, 1));
  float* d_w = cv.take<float>(std::max<size_t>(nweights, 1));
  int* d_wp = cv.take<int>(std::max<size_t>(npos, 1));
  int* d_vp = cv.take<int>(std::max<size_t>(npos, 1));
  float* d_pred = cv.take<float>(nrows);
  hipStream_t s = c->stream;
  DFH_HIP(hipMemcpyAsync(d_off, off32.data(), (nrows + 1) * 4, hipMemcpyHostToDevice, s));
  if (nnz) DFH_HIP(hipMemcpyAsync(d_idx, index + base, nnz * 4, hipMemcpyHostToDevice, s));
  if (nnz && value) DFH_HIP(hipMemcpyAsync(d_val, value + base, nnz * 4, hipMemcpyHostToDevice, s));
  if (nweights) DFH_HIP(hipMemcpyAsync(d_w, weights, nweights * 4, hipMemcpyHostToDevice, s));
  if (w_pos) {
    DFH_HIP(hipMemcpyAsync(d_wp, w_pos, npos * 4, hipMemcpyHostToDevice, s));
    if (V_pos) DFH_HIP(hipMemcpyAsync(d_vp, V_pos, npos * 4, hipMemcpyHostToDevice, s));
  }
  DFH_HIP(hipMemcpyAsync(d_pred, pred, nrows * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_predict_generic, dim3(grid_for_waves(nrows, c)), dim3(256), 0, s, (uint32_t)nrows, d_off, d_idx,
                     value ? d_val : (const float*)nullptr, d_w, w_pos ? d_wp : (const int*)nullptr,
                     (w_pos && V_pos) ? d_vp : (const int*)nullptr, V_dim, d_pred, (float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (float*)nullptr);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipMemcpyAsync(pred, d_pred, nrows * 4, hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

int dfh_fm_calcgrad(dfh_ctx* c, int V_dim, size_t nrows, const size_t* offset, const uint32_t* index, const float* value,
                    const float* label, const float* weights, size_t nweights, const int* w_pos, const int* V_pos,
                    size_t npos, const float* pred, float* grad) {
  DFH_ARG(c && V_dim >= 0, "dfh_fm_calcgrad: bad argument");
  if (nrows == 0) return DFH_OK;
  DFH_ARG(offset && pred && weights && grad && label, "dfh_fm_calcgrad: NULL argument");
  DFH_ARG(V_dim == 0 || (w_pos && V_pos), "dfh_fm_calcgrad: V_dim > 0 needs w_pos and V_pos");
  DFH_HIP(hipSetDevice(c->device));
  std::vector<uint32_t> off32;
  int rc = to_u32_offsets(offset, nrows, &off32);
  if (rc) return rc;
  const size_t base = offset[0];
  const size_t nnz = off32[nrows];
  const size_t ncols = w_pos ? npos : nweights;
  // column-major view (stable counting sort by column => ascending rows per column,
  // the order SpMV/SpMM::TransTimes accumulate in: spmv.h:152-168, spmm.h:137-156)
  std::vector<uint32_t> col_ptr(ncols + 1, 0), s_row(std::max<size_t>(nnz, 1));
  std::vector<float> s_val(value ? std::max<size_t>(nnz, 1) : 0);
  for (size_t j = 0; j < nnz; ++j) {
    DFH_ARG(index[base + j] < ncols, "dfh_fm_calcgrad: index out of range");
    ++col_ptr[index[base + j] + 1];
  }
  for (size_t u = 0; u < ncols; ++u) col_ptr[u + 1] += col_ptr[u];
  {
    std::vector<uint32_t> fill(col_ptr.begin(), col_ptr.end() - 1);
    for (size_t i = 0; i < nrows; ++i) {
      for (uint32_t j = off32[i]; j < off32[i + 1]; ++j) {
        uint32_t q = fill[index[base + j]]++;
        s_row[q] = (uint32_t)i;
        if (value) s_val[q] = value[base + j];
      }
    }
  }
  if (w_pos) {
    for (size_t u = 0; u < npos; ++u) {
      DFH_ARG(w_pos[u] == -1 || (w_pos[u] >= 0 && (size_t)w_pos[u] < nweights), "w_pos out of range");
      if (V_dim > 0) DFH_ARG(V_pos[u] == -1 || (V_pos[u] >= 0 && (size_t)V_pos[u] + V_dim <= nweights), "V_pos out of range");
    }
  }
  const size_t xvn = nrows * (size_t)std::max(V_dim, 1);
  rc = ensure_scratch(c, padded<uint32_t>(nrows + 1) + 2 * padded<uint32_t>(nnz) + 2 * padded<float>(nnz) +
                             2 * padded<float>(nweights) + 2 * padded<int>(npos) + 3 * padded<float>(nrows) +
                             padded<float>(xvn) + padded<uint32_t>(ncols + 1));
  if (rc) return rc;
  Carver cv(c->scratch);
  uint32_t* d_off = cv.take<uint32_t>(nrows + 1);
  uint32_t* d_idx = cv.take<uint32_t>(std::max<size_t>(nnz, 1));
  float* d_val = cv.take<float>(std::max<size_t>(nnz, 1));
  uint32_t* d_srow = cv.take<uint32_t>(std::max<size_t>(nnz, 1));
  float* d_sval = cv.take<float>(std::max<size_t>(nnz, 1));
  uint32_t* d_colptr = cv.take<uint32_t>(ncols + 1);
  float* d_w = cv.take<float>(std::max<size_t>(nweights, 1));
  float* d_grad = cv.take<float>(std::max<size_t>(nweights, 1));
  int* d_wp = cv.take<int>(std::max<size_t>(npos, 1));
  int* d_vp = cv.take<int>(std::max<size_t>(npos, 1));
  float* d_pred = cv.take<float>(nrows);
  float* d_label = cv.take<float>(nrows);
  float* d_slope = cv.take<float>(nrows);
  float* d_xv = cv.take<float>(xvn);
  hipStream_t s = c->stream;
  DFH_HIP(hipMemcpyAsync(d_off, off32.data(), (nrows + 1) * 4, hipMemcpyHostToDevice, s));
  if (nnz) {
    DFH_HIP(hipMemcpyAsync(d_idx, index + base, nnz * 4, hipMemcpyHostToDevice, s));
    DFH_HIP(hipMemcpyAsync(d_srow, s_row.data(), nnz * 4, hipMemcpyHostToDevice, s));
    if (value) {
      DFH_HIP(hipMemcpyAsync(d_val, value + base, nnz * 4, hipMemcpyHostToDevice, s));
      DFH_HIP(hipMemcpyAsync(d_sval, s_val.data(), nnz * 4, hipMemcpyHostToDevice, s));
    }
  }
  DFH_HIP(hipMemcpyAsync(d_colptr, col_ptr.data(), (ncols + 1) * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(d_w, weights, nweights * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(d_grad, grad, nweights * 4, hipMemcpyHostToDevice, s));
  if (w_pos) {
    DFH_HIP(hipMemcpyAsync(d_wp, w_pos, npos * 4, hipMemcpyHostToDevice, s));
    if (V_pos) DFH_HIP(hipMemcpyAsync(d_vp, V_pos, npos * 4, hipMemcpyHostToDevice, s));
  }
  DFH_HIP(hipMemcpyAsync(d_pred, pred, nrows * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(d_label, label, nrows * 4, hipMemcpyHostToDevice, s));
  const float* dv = value ? d_val : nullptr;
  const int* dwp = w_pos ? d_wp : nullptr;
  const int* dvp = (w_pos && V_pos) ? d_vp : nullptr;
  // pass A: XV = X*V (what Predict left in XV_, fm_loss.h:81-83) and the slope p (fm_loss.h:157-161)
  hipLaunchKernelGGL(k_predict_generic, dim3(grid_for_waves(nrows, c)), dim3(256), 0, s, (uint32_t)nrows, d_off, d_idx, dv,
                     d_w, dwp, dvp, V_dim, (float*)nullptr, V_dim > 0 ? d_xv : (float*)nullptr, d_label, d_pred, d_slope);
  // pass B: per-column accumulation
  hipLaunchKernelGGL(k_calcgrad_generic, dim3(grid_for_waves(ncols, c)), dim3(256), 0, s, (uint32_t)ncols, d_colptr,
                     d_srow, value ? d_sval : (const float*)nullptr, d_w, dwp, dvp, V_dim, d_slope, d_xv, d_grad);
  DFH_HIP(hipGetLastError());
  DFH_HIP(hipMemcpyAsync(grad, d_grad, nweights * 4, hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

int dfh_loss_evaluate(dfh_ctx* c, const float* label, const float* pred, size_t n, float* objv) {
  DFH_ARG(c && objv, "NULL argument");
  *objv = 0;
  if (n == 0) return DFH_OK;
  DFH_ARG(label && pred, "NULL argument");
  DFH_HIP(hipSetDevice(c->device));
  int rc = ensure_scratch(c, 2 * padded<float>(n) + 512);
  if (rc) return rc;
  Carver cv(c->scratch);
  float* d_l = cv.take<float>(n);
  float* d_p = cv.take<float>(n);
  double* d_o = cv.take<double>(1);
  hipStream_t s = c->stream;
  DFH_HIP(hipMemcpyAsync(d_l, label, n * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemcpyAsync(d_p, pred, n * 4, hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemsetAsync(d_o, 0, sizeof(double), s));
  hipLaunchKernelGGL(k_logloss, dim3(grid_for_threads(n, c)), dim3(256), 0, s, d_l, d_p, (uint32_t)n, d_o);
  DFH_HIP(hipGetLastError());
  double o = 0;
  DFH_HIP(hipMemcpyAsync(&o, d_o, sizeof(double), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  *objv = (float)o;
  return DFH_OK;
}
}  // extern "C"
