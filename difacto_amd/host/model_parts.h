/**
 * model_parts.h — how a learner commits model_out.  One process: the file itself.  A sharded run: one part per rank
 * (<model_out>.part-<rank>) plus a manifest (<model_out>.parts: the number of parts, written by rank 0, which also
 * removes the parts a run with more ranks left behind under the same name).  SGDLearner::LoadModel reads exactly the
 * parts the manifest names, keeping the keys of its own range: a model can be re-loaded under any number of ranks, and
 * stale parts of an earlier save are never imported.  Used by learner = sgd and learner = lbfgs.
 *
 * LoadModelEntries is the way back for learner = lbfgs and learner = bcd (model_in): the entries of a key range out of
 * the file, or out of the parts its manifest names, through a scratch dfh_table (dfh_table_load + dfh_table_export) —
 * SaveDenseModel, the end of both learners' SaveModel, goes the other way through the same calls.
 */
#ifndef DIFACTO_HOST_MODEL_PARTS_H_
#define DIFACTO_HOST_MODEL_PARTS_H_
#include <unistd.h>
#include <cstdio>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "./device_context.h"
#include "difacto_hip.h"
#include "dmlc/logging.h"

namespace difacto {

/*! \brief write(tmp) writes this rank's file under a temporary name; it is renamed into place when complete, so a reader
 * never sees half a file and a rank that dies mid-save leaves the previous part in place.  comm: NULL for one process;
 * otherwise COLLECTIVE over its ranks. */
inline void SaveModelParts(dfh_comm* comm, int rank, int world, const std::string& model_out,
                           const std::function<void(const std::string& tmp)>& write) {
  const std::string path = comm ? model_out + ".part-" + std::to_string(rank) : model_out;
  const std::string tmp = path + ".tmp";
  write(tmp);
  if (comm) {
    // the manifest is the commit point of a sharded save: it may only name parts that are complete.  Every rank has closed
    // its part when this all-reduce returns (a rank that failed never arrives: no new manifest); the parts are then
    // renamed into place and rank 0 writes the manifest after a second round.
    double ok[1] = {1.0};
    DFH_CALL(dfh_comm_allreduce_sum(comm, ok, 1));
    CHECK_EQ(static_cast<int>(ok[0]), world) << "a rank did not finish its model part";
  }
  CHECK_EQ(rename(tmp.c_str(), path.c_str()), 0) << "cannot move " << tmp << " to " << path;
  LOG(INFO) << "model saved to " << path;
  if (comm) {
    double done[1] = {1.0};
    DFH_CALL(dfh_comm_allreduce_sum(comm, done, 1));   // every part is in place
  }
  if (comm && rank == 0) {
    for (int n = world;; ++n) {  // parts of an earlier save with more ranks
      const std::string stale = model_out + ".part-" + std::to_string(n);
      if (access(stale.c_str(), F_OK) != 0) break;
      CHECK_EQ(unlink(stale.c_str()), 0) << "cannot remove the stale model part " << stale;
      LOG(INFO) << "removed the stale model part " << stale;
    }
    const std::string mf = model_out + ".parts";
    FILE* f = fopen((mf + ".tmp").c_str(), "w");
    CHECK(f) << "cannot write " << mf;
    fprintf(f, "%d\n", world);
    CHECK_EQ(fclose(f), 0);
    CHECK_EQ(rename((mf + ".tmp").c_str(), mf.c_str()), 0);
  }
}

/*! \brief the entries of a model file: w, and V [V_dim] where has_V (optimiser state in the file is left behind) */
struct ModelEntries {
  int V_dim = 0;
  std::vector<uint64_t> keys;   // any order
  std::vector<float> w;
  std::vector<int> has_V;
  std::vector<float> V;         // [keys x V_dim], zeros where !has_V
};

/*! \brief the files behind model_in: the file itself, or, when it does not exist and <model_in>.parts does, the parts the
 * manifest names.  Nothing readable is fatal, with the path. */
inline std::vector<std::string> ModelInFiles(const std::string& model_in) {
  std::vector<std::string> files;
  if (access(model_in.c_str(), R_OK) == 0) {
    files.push_back(model_in);
    return files;
  }
  const std::string mf = model_in + ".parts";
  FILE* f = fopen(mf.c_str(), "r");
  CHECK(f) << "model_in: cannot read " << model_in << " (nor the manifest " << mf << ")";
  int want = -1;
  const bool ok = fscanf(f, "%d", &want) == 1 && want >= 1 && want <= 4096;
  fclose(f);
  CHECK(ok) << "bad model manifest " << mf;
  for (int i = 0; i < want; ++i) {
    files.push_back(model_in + ".part-" + std::to_string(i));
    CHECK_EQ(access(files.back().c_str(), R_OK), 0)
        << "model part " << files.back() << " is missing (the manifest names " << want << " parts)";
  }
  return files;
}

/*! \brief V_dim and the number of entries in the header of a model file (the format: dfh_table_save) */
inline void ReadModelHeader(const std::string& path, int* V_dim, uint64_t* n) {
  FILE* f = fopen(path.c_str(), "rb");
  CHECK(f) << "model_in: cannot read " << path;
  char magic[4];
  uint32_t ver = 0;
  int32_t k = 0, aux = 0;
  const bool ok = fread(magic, 1, 4, f) == 4 && !memcmp(magic, "DFHM", 4) && fread(&ver, 4, 1, f) == 1 && fread(&k, 4, 1, f) == 1 &&
                  fread(&aux, 4, 1, f) == 1 && fread(n, 8, 1, f) == 1;
  fclose(f);
  CHECK(ok && k >= 0) << path << " is not a model file";
  *V_dim = k;
}

/*! \brief the entries with key in [key_lo, key_hi) (key_hi = 0: no upper bound) of the model behind model_in, whatever
 * sharding wrote it; a file saved with optimiser state (learner = sgd, has_aux) is accepted, only w and V are taken */
inline void LoadModelEntries(const std::string& model_in, uint64_t key_lo, uint64_t key_hi, ModelEntries* out) {
  const std::vector<std::string> files = ModelInFiles(model_in);
  uint64_t total = 0;
  for (size_t i = 0; i < files.size(); ++i) {
    int k = 0;
    uint64_t n = 0;
    ReadModelHeader(files[i], &k, &n);
    CHECK(i == 0 || k == out->V_dim) << files[i] << " has V_dim = " << k << ", " << files[0] << " has " << out->V_dim;
    out->V_dim = k;
    total += n;
  }
  const int k = out->V_dim;
  dfh_updater_param up;
  dfh_updater_param_default(&up, k);
  dfh_table* t = nullptr;
  DFH_CALL(dfh_table_create(DeviceContext::Get(), &up, std::max<uint64_t>(total + total / 2 + 1024, 1024), &t));
  for (const auto& path : files) DFH_CALL(dfh_table_load(t, path.c_str(), key_lo, key_hi, nullptr, nullptr));
  uint64_t n = 0;
  DFH_CALL(dfh_table_size(t, &n));
  const uint64_t cap = std::max<uint64_t>(n, 1);
  std::vector<float> scal(4 * cap), V2(static_cast<size_t>(2) * std::max(k, 1) * cap);
  out->keys.resize(cap);
  out->has_V.resize(cap);
  DFH_CALL(dfh_table_export(t, cap, out->keys.data(), scal.data(), out->has_V.data(), V2.data(), &n));
  DFH_CALL(dfh_table_destroy(t));
  out->keys.resize(n);
  out->has_V.resize(n);
  out->w.resize(n);
  out->V.assign(static_cast<size_t>(k) * n, 0.f);
  for (uint64_t i = 0; i < n; ++i) {
    out->w[i] = scal[4 * i + 1];   // {fea_cnt, w, sqrt_g, z}
    if (out->has_V[i])
      for (int j = 0; j < k; ++j) out->V[static_cast<size_t>(k) * i + j] = V2[static_cast<size_t>(2) * k * i + j];
  }
}

/*! \brief SaveModel of those learners: nkeys entries as learner = sgd's model file without optimiser state, through a
 * scratch table.  scal [nkeys x 4] {fea_cnt, w, sqrt_g, z}, has [nkeys], V [nkeys x 2 V_dim] (NULL with V_dim = 0) */
inline void SaveDenseModel(const std::string& path, int V_dim, uint64_t nkeys, const uint64_t* keys, const float* scal,
                           const int* has, const float* V) {
  dfh_updater_param up;
  dfh_updater_param_default(&up, V_dim);
  dfh_table* t = nullptr;
  DFH_CALL(dfh_table_create(DeviceContext::Get(), &up, std::max<uint64_t>(nkeys + nkeys / 2 + 1024, 1024), &t));
  if (nkeys) DFH_CALL(dfh_table_import(t, nkeys, keys, scal, has, V));
  uint64_t saved = 0;
  DFH_CALL(dfh_table_save(t, path.c_str(), 0, &saved));
  DFH_CALL(dfh_table_destroy(t));
}

}  // namespace difacto
#endif  // DIFACTO_HOST_MODEL_PARTS_H_
