/**
 * bcd_learner.cc — BCDLearner (bcd_learner.h).  Reference: src/bcd/bcd_learner.cc, src/bcd/bcd_utils.h.
 */
#include "./bcd_learner.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <mutex>
#include "./batch_reader.h"
#include "./device_context.h"
#include "./model_parts.h"
#include "./resident_data.h"

namespace difacto {

DMLC_REGISTER_PARAMETER(BCDLearnerParam);
DMLC_REGISTER_PARAMETER(BCDUpdaterParam);

namespace bcd {

void PartitionFeature(int feagrp_nbits, const std::vector<std::pair<int, int>>& feagrps, std::vector<Range>* feablks) {
  CHECK_EQ(feagrp_nbits % 4, 0) << "should be 0, 4, 8, ...";
  feablks->clear();
  for (auto f : feagrps) {
    const int gid = f.first;
    Range rg(ReverseBytes(EncodeFeaGrpID(0, gid, feagrp_nbits)),
             ReverseBytes(EncodeFeaGrpID(std::numeric_limits<feaid_t>::max(), gid, feagrp_nbits)));
    for (int i = 0; i < f.second; ++i) {
      feablks->push_back(rg.Segment(i, f.second));
      CHECK(feablks->back().Valid());
    }
  }
  std::sort(feablks->begin(), feablks->end(), [](const Range& a, const Range& b) { return a.begin < b.begin; });
  for (size_t i = 1; i < feablks->size(); ++i) {
    auto& before = feablks->at(i - 1);
    const auto& after = feablks->at(i);
    if (before.end < after.begin) ++before.end;
    CHECK_LE(before.end, after.begin);
  }
}

FeaGroupStats::FeaGroupStats(int nbits) {
  CHECK_LE(nbits, 16);
  nbits_ = nbits;
  value_.resize((1 << nbits_) + 2);
}

void FeaGroupStats::Add(size_t nrows, const size_t* offset, const feaid_t* index) {
  real_t n = 0;
  for (size_t i = 0; i < nrows; i += skip_) {
    for (size_t j = offset[i]; j < offset[i + 1]; ++j) ++value_[DecodeFeaGrpID(index[j], nbits_)];
    ++n;
  }
  value_[1 << nbits_] += n;
  value_[(1 << nbits_) + 1] += nrows;
}

}  // namespace bcd

BCDLearner::~BCDLearner() {
  if (obj_) dfh_bcd_destroy(obj_);
  if (comm_) dfh_comm_destroy(comm_);
}

KWArgs BCDLearner::Init(const KWArgs& kwargs) {
  for (const auto& kw : kwargs)
    CHECK(!(kw.first == "task" && kw.second == "predict"))
        << "learner = bcd has no prediction task: train with model_out=<file>, then score with "
           "task=predict learner=sgd model_in=<file> V_dim=0 pred_out=<file>";
  const char* nw = getenv("DMLC_NUM_WORKER");
  bool shard_rows = false;
  for (const auto& kw : kwargs)
    if (kw.first == "shard_rows") shard_rows = atoi(kw.second.c_str()) != 0;
  if (shard_rows) {
    // one process per GPU only with the whole environment of a rank; a scheduler or server role is refused as the
    // sharded store of learner = sgd refuses it
    const char* role = getenv("DMLC_ROLE");
    if (role && std::string(role) != "worker") ReadRankEnv();
    std::string missing;
    for (const char* name : {"DMLC_ROLE", "DMLC_NUM_WORKER", "DIFACTO_RANK", "DIFACTO_RENDEZVOUS"})
      if (!getenv(name)) missing += std::string(missing.size() ? ", " : "") + name;
    CHECK(missing.empty()) << "learner = bcd shard_rows=1 needs the complete environment of a rank (DMLC_ROLE=worker, "
                           << "DMLC_NUM_WORKER, DIFACTO_RANK, DIFACTO_RENDEZVOUS): " << missing << " is not set";
  } else {
    CHECK(!IsDistributed() && !(nw && atoi(nw) > 1))
        << "learner = bcd runs in one process on one GPU: a sharded store (DMLC_ROLE / DMLC_NUM_WORKER > 1) is not supported";
  }
  // bcd_learner.cc:15-34: the learner's, then the updater's keys; the loss (logit_delta) and the tile store take none
  auto remain = Learner::Init(kwargs);
  remain = param_.InitAllowUnknown(remain);
  remain = updater_param_.InitAllowUnknown(remain);
  CHECK_EQ(param_.num_feature_group_bits % 4, 0) << "num_feature_group_bits should be 0, 4, 8, ...";
  CHECK(param_.num_feature_group_bits >= 0 && param_.num_feature_group_bits <= 16) << "num_feature_group_bits <= 16";
  if (shard_rows) {
    const RankEnv env = ReadRankEnv();   // before the device context: the rank's device
    rank_ = env.rank;
    world_ = env.world;
    comm_ = ConnectRanks(rank_, world_, &files_, 120.0);
    LOG(INFO) << "bcd: rank " << rank_ << " of " << world_ << " connected (" << (files_ ? "file transport" : "RCCL")
              << "): a worker for part " << rank_ << " of the rows and the server of one slice of every block";
    DFH_CALL(dfh_bcd_create_sharded(DeviceContext::Get(), comm_, &obj_));
  } else {
    DFH_CALL(dfh_bcd_create(DeviceContext::Get(), &obj_));
  }
  return remain;
}

void BCDLearner::PrepareData(std::vector<real_t>* fea_stats) {
  // Reader blocks of data_chunk_size bytes (bcd_learner.cc:98-108); a block beyond the batch object's 32-bit positions is
  // cut by rows
  const size_t chunk_bytes = std::max<size_t>(64, static_cast<size_t>(param_.data_chunk_size));
  bcd::FeaGroupStats stats(param_.num_feature_group_bits);
  auto read = [&](const std::string& uri, int is_val) {
    Reader reader(uri, param_.data_format, rank_, world_, chunk_bytes);   // part rank_ of world_
    ForEachChunk(&reader, kMaxChunkNnz, [&](size_t r0, size_t r1, const dmlc::RowBlock<feaid_t>& blk) {
      if (!is_val) {
        stats.Add(r1 - r0, blk.offset + r0, blk.index);   // bcd_learner.cc:107
        chunk_rows_.push_back(r1 - r0);
      }
      DFH_CALL(dfh_bcd_add_chunk(obj_, is_val, r1 - r0, blk.offset + r0, blk.index, blk.value, blk.label + r0));
    });
  };
  read(param_.data_in, 0);
  stats.Get(fea_stats);
  if (comm_) {
    // every rank's statistics added in rank order (they are counts: the floats of one process reading every row while
    // they stay below 2^24), so every rank cuts the same blocks
    LOG(INFO) << "rank " << rank_ << ": " << fea_stats->back() << " training examples in " << chunk_rows_.size() << " chunks";
    for (size_t i = 0; i < fea_stats->size(); i += 64) {
      double t[64];
      const int n = static_cast<int>(std::min<size_t>(64, fea_stats->size() - i));
      for (int k = 0; k < n; ++k) t[k] = (*fea_stats)[i + k];
      DFH_CALL(dfh_comm_allreduce_sum(comm_, t, n));
      for (int k = 0; k < n; ++k) (*fea_stats)[i + k] = static_cast<real_t>(t[k]);
    }
  }
  if (param_.data_val.size()) read(param_.data_val, 1);   // bcd_learner.cc:118-129
}

void BCDLearner::RunScheduler() {
  // bcd_learner.cc:51-92, with the worker / server jobs as calls on the dfh_bcd object
  LOG(INFO) << "loading data... ";
  std::vector<real_t> load_rets;
  PrepareData(&load_rets);
  LOG(INFO) << "loaded " << load_rets.back() << " examples";

  // partition feature group and build feature map
  std::vector<std::pair<int, int>> feagrp;
  const int nfeablk = static_cast<int>(load_rets.size()) - 2;
  for (int i = 0; i < nfeablk; ++i) {
    const int nblk = static_cast<int>(std::ceil(load_rets[i] / load_rets[nfeablk] * param_.block_ratio));
    if (nblk > 0) feagrp.push_back(std::make_pair(i, nblk));
  }
  std::vector<bcd::Range> ranges;
  bcd::PartitionFeature(param_.num_feature_group_bits, feagrp, &ranges);
  LOG(INFO) << "partitioning feature into " << ranges.size() << " blocks";
  std::vector<uint64_t> beg(ranges.size()), end(ranges.size());
  for (size_t i = 0; i < ranges.size(); ++i) {
    beg[i] = ranges[i].begin;
    end[i] = ranges[i].end;
  }
  uint64_t nkeys = 0;
  DFH_CALL(dfh_bcd_build(obj_, static_cast<float>(updater_param_.tail_feature_filter), static_cast<int>(ranges.size()), beg.data(),
                         end.data(), updater_param_.l1, updater_param_.lr, &nkeys));
  if (param_.model_in.size()) LoadModel(nkeys);

  // iterate over data: the block order is std::random_shuffle on the process-wide rand() stream (bcd_learner.cc:79)
  std::vector<int> feablks(ranges.size());
  for (size_t i = 0; i < feablks.size(); ++i) feablks[i] = static_cast<int>(i);
  for (int epoch = 0; epoch < param_.max_num_epochs; ++epoch) {
    {
      std::lock_guard<std::mutex> lk(*RefRand::GlobalLock());
      RefRand::Global()->Shuffle(&feablks);
    }
    std::vector<real_t> progress(4, 0);
    CHECK(feablks.size()) << "no feature block";
    DFH_CALL(dfh_bcd_epoch(obj_, feablks.data(), static_cast<int>(feablks.size()), progress.data()));
    for (const auto& cb : epoch_end_callback_) cb(epoch, progress);
    const real_t cnt = progress[0];
    LL << "epoch: " << epoch << ", objv: " << progress[1] / cnt << ", auc: " << progress[2] / cnt
       << ", acc: " << progress[3] / cnt;
  }
  if (param_.model_out.size() && rank_ == 0) SaveModel();   // the model is replicated: one file, from rank 0
}

// model_in: the file's w joined onto the model's keys on the device, the predictions of every chunk rebuilt from it
// (dfh_bcd_set_model).  V in the file is ignored; keys the model does not hold (filtered, or not in this data) are dropped.
void BCDLearner::LoadModel(uint64_t nkeys) {
  ModelEntries m;
  LoadModelEntries(param_.model_in, 0, 0, &m);
  uint64_t matched = 0;
  DFH_CALL(dfh_bcd_set_model(obj_, m.keys.size(), m.keys.data(), m.w.data(), &matched));
  LOG(INFO) << "model loaded from " << param_.model_in << ": " << matched << " of " << m.keys.size() << " keys matched " << nkeys
            << " model keys";
}

// the final w as learner = sgd's model file without optimiser state (dfh_table_save, save_aux = 0)
void BCDLearner::SaveModel() {
  uint64_t nkeys = 0;
  DFH_CALL(dfh_bcd_shape(obj_, &nkeys, nullptr, nullptr, nullptr));
  std::vector<uint64_t> keys(std::max<uint64_t>(nkeys, 1));
  std::vector<float> cnt(keys.size()), w(keys.size());
  DFH_CALL(dfh_bcd_get_model(obj_, keys.data(), cnt.data(), w.data(), nullptr, nullptr));
  std::vector<float> scal(4 * keys.size(), 0.f);
  std::vector<int> has(keys.size(), 0);
  for (size_t i = 0; i < nkeys; ++i) {
    scal[4 * i] = cnt[i];   // {fea_cnt, w, sqrt_g, z}
    scal[4 * i + 1] = w[i];
  }
  SaveDenseModel(param_.model_out, 0, nkeys, keys.data(), scal.data(), has.data(), nullptr);
  LOG(INFO) << "model saved to " << param_.model_out;
}

}  // namespace difacto
