/**
 * sharded_store.h — ShardedDeviceStore : Store, the model row-sharded by key range over the GPUs
 * of one node, one process per GPU.  It takes the place of the reference's distributed store
 * (Store::Create() under DMLC_ROLE, src/store/store.cc:8-15 — KVStoreDist over ps-lite there):
 * every process is a worker AND the server of one key range; NumWorkers() is the number of ranks, so
 * SGDLearner::RunEpoch cuts the data into NumWorkers() x num_jobs_per_epoch parts as the reference
 * does (src/sgd/sgd_learner.cc:78-89).
 *
 * The exchange lives inside libdifacto_hip.so (dfh_shard_step: RCCL ncclSend / ncclRecv over xGMI);
 * this class owns the communicator and the shard handle and exposes them to the learner's sharded
 * worker loop.  The store is COLLECTIVE — every rank takes part in every step — so the literal,
 * one-sided Push / Pull of the interface is not offered here: use device_path = fused (the default).
 *
 * Process environment (one process per GPU; example/run_local_gpus.sh):
 *   DMLC_ROLE=worker            distributed mode (include/difacto/base.h: IsDistributed())
 *   DMLC_NUM_WORKER=<G>         ranks
 *   DIFACTO_RANK=<r>            this rank, 0 .. G-1 (also the default DIFACTO_DEVICE)
 *   DIFACTO_RENDEZVOUS=<path>   rank 0 writes the RCCL unique id there, the others read it
 *   DIFACTO_COMM=rccl|file      transport; "file" (exchange through files in the directory
 *                               DIFACTO_RENDEZVOUS) exists for tests with several ranks on one GPU
 */
#ifndef DIFACTO_HOST_SHARDED_STORE_H_
#define DIFACTO_HOST_SHARDED_STORE_H_
#include <sys/stat.h>
#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>
#include "./comm_setup.h"
#include "./device_store.h"

namespace difacto {

class ShardedDeviceStore : public Store {
 public:
  ShardedDeviceStore() {
    const RankEnv env = ReadRankEnv();
    world_ = env.world;
    rank_ = env.rank;
  }
  virtual ~ShardedDeviceStore() {
    if (shard_) dfh_shard_destroy(shard_);
    if (comm_) dfh_comm_destroy(comm_);
  }

  /*! \brief connects the ranks; called after SetUpdater (sgd_learner.cc:234-240), so the shard's table exists */
  KWArgs Init(const KWArgs& kwargs) override {
    auto* up = CHECK_NOTNULL(dynamic_cast<DeviceSGDUpdater*>(CHECK_NOTNULL(updater_.get())));
    CHECK(up->device_param().V_init == "hash" || up->param().V_dim == 0)
        << "the sharded store needs V_init=hash: the rand_r chain of the reference depends on the global order of allocations";
    comm_ = ConnectRanks(rank_, world_, &files_);
    LOG(INFO) << "sharded store: rank " << rank_ << " of " << world_ << " connected ("
              << (files_ ? "file transport" : "RCCL") << ")";
    return kwargs;
  }

  /**
   * \brief cuts the key space and creates this rank's shard.  COLLECTIVE; called once by the learner after Init,
   * before a model is loaded.  sample: reversed keys of (the beginning of) this rank's part of the data, any number,
   * for shard_ranges = balanced (dfh_shard_balanced_splits: the quantiles of the union of all ranks' samples);
   * ignored for uniform ranges.
   */
  void CreateShard(const std::vector<feaid_t>& sample) {
    CHECK(!shard_) << "the shard exists already";
    auto* up = CHECK_NOTNULL(dynamic_cast<DeviceSGDUpdater*>(CHECK_NOTNULL(updater_.get())));
    const auto& dp = up->device_param();
    CHECK(dp.shard_ranges == "balanced" || dp.shard_ranges == "uniform") << "shard_ranges = balanced | uniform";
    CHECK(dp.shard_exchange == "overlap" || dp.shard_exchange == "sync") << "shard_exchange = overlap | sync";
    std::vector<uint64_t> splits(world_ > 1 ? world_ - 1 : 1, 0);
    const bool balanced = dp.shard_ranges == "balanced" && world_ > 1;
    if (balanced) DFH_CALL(dfh_shard_balanced_splits(comm_, sample.data(), sample.size(), splits.data()));
    DFH_CALL(dfh_shard_create(up->table(), comm_, balanced ? splits.data() : nullptr, &shard_));
    if (dp.shard_exchange == "overlap") DFH_CALL(dfh_shard_set_exchange(shard_, 1));
    if (reserve_keys_) DFH_CALL(dfh_shard_reserve(shard_, reserve_keys_, 2 * reserve_keys_));  // no re-allocation inside a step
    if (balanced) splits_ = splits;
    uint64_t lo = 0, hi = 0;
    DFH_CALL(dfh_shard_owned_range(shard_, balanced ? splits.data() : nullptr, &lo, &hi));
    LOG(INFO) << "sharded store: rank " << rank_ << " owns the reversed keys [" << lo << ", " << (hi ? std::to_string(hi) : "2^64")
              << ") (" << dp.shard_ranges << " ranges), exchange = " << dp.shard_exchange;
  }

  /**
   * \brief the literal Store::Push / Pull (include/difacto/store.h:53-73) on the sharded model: keys routed to their owners,
   * rows / acknowledgements back (dfh_shard_push_host / dfh_shard_pull_host).  COLLECTIVE: every rank makes the same
   * sequence of calls (a rank without a minibatch passes empty arrays) — what SGDLearner's literal worker loop does.
   * Synchronous: the arrays are consumed, and on_complete has run, on return.
   */
  int Push(const SArray<feaid_t>& fea_ids, int val_type, const SArray<real_t>& vals, const SArray<int>& lens,
           const std::function<void()>& on_complete) override {
    DFH_CALL(dfh_shard_push_host(CHECK_NOTNULL(shard_), fea_ids.data(), fea_ids.size(), val_type, vals.data(), vals.size(), lens.data(),
                                 lens.size()));
    if (on_complete) on_complete();
    return time_++;
  }
  int Pull(const SArray<feaid_t>& fea_ids, int val_type, SArray<real_t>* vals, SArray<int>* lens,
           const std::function<void()>& on_complete) override {
    CHECK_EQ(val_type, Store::kWeight);
    auto* up = CHECK_NOTNULL(dynamic_cast<DeviceSGDUpdater*>(CHECK_NOTNULL(updater_.get())));
    const size_t n = fea_ids.size();
    CHECK_NOTNULL(vals)->resize(n * (1 + up->param().V_dim));
    CHECK_NOTNULL(lens)->resize(n);
    size_t nvals = 0, nlens = 0;
    DFH_CALL(dfh_shard_pull_host(CHECK_NOTNULL(shard_), fea_ids.data(), n, vals->data(), &nvals, lens->data(), &nlens));
    vals->resize(nvals);
    lens->resize(nlens);
    if (on_complete) on_complete();
    return time_++;
  }
  void Wait(int time) override {}
  int Rank() override { return rank_; }
  int NumWorkers() override { return world_; }
  int NumServers() override { return world_; }

  dfh_shard* shard() { return shard_; }
  /*! \brief unique keys of the largest minibatch to expect (batch_size x ids per row): the exchange buffers are sized for it
   *  when the shard is created; 0: they grow when a step first meets a size */
  void set_reserve_keys(size_t n) { reserve_keys_ = n; }
  dfh_comm* comm() { return comm_; }
  /*! \brief the split keys the shard was created with, NULL for the uniform ranges (what dfh_shard_owned_range takes) */
  const uint64_t* splits() const { return splits_.empty() ? nullptr : splits_.data(); }

 private:
  int rank_ = 0, world_ = 1;
  int time_ = 0;
  dfh_comm* comm_ = nullptr;
  dfh_shard* shard_ = nullptr;
  size_t reserve_keys_ = 0;
  std::vector<uint64_t> splits_;
  std::unique_ptr<FileExchange> files_;
};

}  // namespace difacto
#endif  // DIFACTO_HOST_SHARDED_STORE_H_
