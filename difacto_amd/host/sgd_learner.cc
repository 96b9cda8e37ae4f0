/**
 * sgd_learner.cc — see sgd_learner.h.  Reference: src/sgd/sgd_learner.cc.
 */
#include "./sgd_learner.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <thread>
#include <unistd.h>
#include "./device_feed.h"
#include "./device_rec_decode.h"
#include "./device_text_parse.h"
#include "./hip_fm_loss.h"
#include "./host_localizer.h"
#include "./libsvm_reader.h"
#include "./model_parts.h"
#include "./sharded_store.h"
#include "data/row_block.h"

namespace difacto {

DMLC_REGISTER_PARAMETER(SGDLearnerParam);
DMLC_REGISTER_PARAMETER(SGDUpdaterParam);
DMLC_REGISTER_PARAMETER(DeviceParam);
DMLC_REGISTER_PARAMETER(FMLossParam);

SGDLearner::~SGDLearner() {
  if (eval_) dfh_eval_destroy(eval_);
  if (predtext_) dfh_predtext_destroy(predtext_);
  delete loss_;
  delete store_;
}

// reference: SGDLearner::Init, sgd_learner.cc:229-246 — every stage consumes
// the keys it knows and hands the rest on; what is left is returned (and warned about by main)
KWArgs SGDLearner::Init(const KWArgs& kwargs) {
  auto remain = Learner::Init(kwargs);
  remain = param_.InitAllowUnknown(remain);
  CHECK(param_.data_format == "libsvm" || param_.data_format == "criteo" || param_.data_format == "criteo_test" ||
        param_.data_format == "adfea" || param_.data_format == "rec")
      << "data_format " << param_.data_format << " is not one of the reference's (libsvm, criteo, criteo_test, adfea, rec)";
  // data_cache: checked before anything touches the device
  CHECK(param_.data_cache.empty() || param_.data_cache == "hbm")
      << "data_cache=" << param_.data_cache << " is not one of \"\" (off, the default) and hbm";
  CHECK_GE(param_.data_cache_max_gb, 0) << "data_cache_max_gb is a size in GB (0: no budget)";
  if (param_.data_cache == "hbm") {
    CHECK(param_.task != "predict") << "data_cache=hbm with task=predict: a prediction is one pass over the data, no later epoch "
                                       "would read the cache (caching is for task=train)";
    CHECK(!IsDistributed()) << "data_cache=hbm with a sharded store (DMLC_ROLE is set): the sharded worker loop does not read "
                               "through the device feed yet; run one process, or leave data_cache out";
    for (const auto& kv : remain)
      CHECK(!(kv.first == "device_path" && kv.second == "literal"))
          << "data_cache=hbm with device_path=literal: the literal loop hands host arrays to Store and Loss, only "
             "device_path=fused gathers its minibatches out of device row buffers";
  }
  // exact_metrics: checked before anything touches the device, like data_cache
  CHECK(param_.exact_metrics == 0 || param_.exact_metrics == 1)
      << "exact_metrics=" << param_.exact_metrics << " is not one of 0 (off, the default) and 1";
  if (param_.exact_metrics == 1) {
    CHECK(!IsDistributed()) << "exact_metrics=1 with a sharded store (DMLC_ROLE is set): the pairs of all ranks would have to meet "
                               "on one device, which this build does not do; run one process, or leave exact_metrics out";
    for (const auto& kv : remain)
      CHECK(!(kv.first == "device_path" && kv.second == "literal"))
          << "exact_metrics=1 with device_path=literal: the literal loop keeps its predictions in host arrays, only "
             "device_path=fused leaves them on the device; use device_path=fused, or leave exact_metrics out";
    CHECK(param_.task != "train" || param_.data_val.size())
        << "exact_metrics=1 with task=train and no data_val: there is nothing to evaluate; name a validation file with "
           "data_val=<file>, or leave exact_metrics out";
  }
  // pred_write: checked before anything touches the device, like data_cache
  CHECK(param_.pred_write == "host" || param_.pred_write == "device")
      << "pred_write=" << param_.pred_write << " is not one of host (the default) and device";
  CHECK_GE(param_.pred_unit_rows, 1) << "pred_unit_rows=" << param_.pred_unit_rows << " is not a number of rows: a unit of "
                                        "pred_write=device closes at 1 row or more (the default is 4194304)";
  if (param_.pred_write == "device") {
    CHECK(param_.task == "predict") << "pred_write=device with task=" << param_.task << ": nothing is predicted, the key says where "
                                       "the text of task=predict is formatted; use task=predict, or leave pred_write out";
    CHECK(!IsDistributed()) << "pred_write=device with a sharded store (DMLC_ROLE is set): the sharded worker loop writes its "
                               "predictions on the host; run one process, or leave pred_write out";
  }
  // text_parse: checked before anything touches the device, like data_cache.  "device" is accepted only where the device feed
  // reads the training data (IterateDataFused); validation and prediction readers outside the feed keep the host parser
  for (const auto& kv : remain) {
    if (kv.first != "text_parse") continue;
    CHECK(kv.second == "host" || kv.second == "device")
        << "text_parse=" << kv.second << " is not one of host (the default) and device";
    if (kv.second != "device") continue;
    CHECK(param_.data_format == "criteo" || param_.data_format == "criteo_test")
        << "text_parse=device with data_format=" << param_.data_format << ": the device parses criteo and criteo_test text only "
           "(libsvm and adfea need the host's number parsing, rec is not text)";
    CHECK(!IsDistributed()) << "text_parse=device with a sharded store (DMLC_ROLE is set): the sharded worker loop does not read "
                               "through the device feed; run one process, or leave text_parse out";
    for (const auto& kw : remain)
      CHECK(!(kw.first == "device_path" && kw.second == "literal"))
          << "text_parse=device with device_path=literal: the literal loop hands host arrays to Store and Loss, only "
             "device_path=fused reads its minibatches out of device row buffers";
    CHECK(param_.shuffle > 0 || param_.data_cache == "hbm" || param_.task == "predict")
        << "text_parse=device without a shuffle buffer: training data goes through the device feed only with shuffle > 0 or "
           "data_cache=hbm; set one of them, or leave text_parse out";
  }
  // rec_decode: the same conditions for the records of a .rec file
  for (const auto& kv : remain) {
    if (kv.first != "rec_decode") continue;
    CHECK(kv.second == "host" || kv.second == "device")
        << "rec_decode=" << kv.second << " is not one of host (the default) and device";
    if (kv.second != "device") continue;
    CHECK(param_.data_format == "rec")
        << "rec_decode=device with data_format=" << param_.data_format << ": the device decodes the records of rec files only "
           "(criteo text has text_parse=device, libsvm and adfea need the host's number parsing)";
    CHECK(!IsDistributed()) << "rec_decode=device with a sharded store (DMLC_ROLE is set): the sharded worker loop does not read "
                               "through the device feed; run one process, or leave rec_decode out";
    for (const auto& kw : remain)
      CHECK(!(kw.first == "device_path" && kw.second == "literal"))
          << "rec_decode=device with device_path=literal: the literal loop hands host arrays to Store and Loss, only "
             "device_path=fused reads its minibatches out of device row buffers";
    CHECK(param_.shuffle > 0 || param_.data_cache == "hbm" || param_.task == "predict")
        << "rec_decode=device without a shuffle buffer: training data goes through the device feed only with shuffle > 0 or "
           "data_cache=hbm; set one of them, or leave rec_decode out";
  }
  auto updater = new DeviceSGDUpdater();
  remain = updater->Init(remain);
  remain.push_back(std::make_pair("V_dim", std::to_string(updater->param().V_dim)));
  store_ = Store::Create();
  store_->SetUpdater(std::shared_ptr<Updater>(updater));
  remain = store_->Init(remain);
  loss_ = Loss::Create(param_.loss, blk_nthreads_);
  remain = loss_->Init(remain);
  if (auto* ss = dynamic_cast<ShardedDeviceStore*>(store_)) {
    // the key ranges of the shards: balanced on a sample of the keys this rank is going to see (the first minibatches
    // of its first data part), gathered over the ranks
    std::vector<feaid_t> sample;
    if (GetUpdater()->device_param().shard_ranges == "balanced" && store_->NumWorkers() > 1) {
      sgd::Job job;
      job.type = param_.task == "predict" ? sgd::Job::kPrediction : sgd::Job::kTraining;
      const int n = store_->NumWorkers() * param_.num_jobs_per_epoch;
      BatchReader reader(JobData(job), param_.data_format, store_->Rank(), n, param_.batch_size, 0, 1.0f);
      while (sample.size() < (1u << 18) && reader.Next()) {
        const auto& blk = reader.Value();
        for (size_t i = blk.offset[0]; i < blk.offset[blk.size]; ++i) sample.push_back(ReverseBytes(blk.index[i]));
      }
    }
    // exchange buffers for this job's minibatches up front (batch_size x feed_ids_per_row keys): nothing is re-allocated
    // inside a step unless the data has more ids per row than announced
    ss->set_reserve_keys(static_cast<size_t>(param_.batch_size) * static_cast<size_t>(GetUpdater()->device_param().feed_ids_per_row));
    ss->CreateShard(sample);
  }
  if (param_.model_in.size()) LoadModel();
  return remain;
}

// reference: SGDLearner::RunScheduler, sgd_learner.cc:31-68
void SGDLearner::RunScheduler() {
  if (param_.task == "predict") {
    RunPrediction();
    return;
  }
  CHECK(param_.task == "train") << "unknown task " << param_.task;
  real_t pre_loss = 0, pre_val_auc = 0;
  for (int k = 0; k < param_.max_num_epochs; ++k) {
    sgd::Progress train_prog;
    LOG(INFO) << "Start epoch " << k;
    RunEpoch(k, sgd::Job::kTraining, &train_prog);
    LOG(INFO) << " - Training: " << train_prog.TextString();
    sgd::Progress val_prog;
    if (param_.data_val.size()) {
      RunEpoch(k, sgd::Job::kValidation, &val_prog);
      LOG(INFO) << " - Validation: " << val_prog.TextString();
    }
    for (const auto& cb : epoch_end_callback_) cb(k, train_prog, val_prog);

    real_t eps = std::fabs(train_prog.loss - pre_loss) / pre_loss;
    if (eps < param_.stop_rel_objv) {
      LOG(INFO) << "Change of loss [" << eps << "] < stop_rel_objv [" << param_.stop_rel_objv << "]";
      break;
    }
    if (val_prog.auc > 0) {
      eps = (val_prog.auc - pre_val_auc) / val_prog.nrows;
      if (eps < param_.stop_val_auc) {
        LOG(INFO) << "Change of validation AUC [" << eps << "] < stop_val_auc [" << param_.stop_val_auc << "]";
        break;
      }
    }
    if (k + 1 >= param_.max_num_epochs) LOG(INFO) << "Reach maximal number of epochs";
    pre_loss = train_prog.loss;
    pre_val_auc = val_prog.auc;
  }
  if (param_.model_out.size()) SaveModel();
}

// reference: SGDLearner::RunEpoch, sgd_learner.cc:70-94.  The data is cut into NumWorkers() x
// num_jobs_per_epoch parts; in a sharded run every rank is its own scheduler and takes the parts
// j * NumWorkers() + Rank(), then the ranks' progress records are summed so that all of them see the
// same epoch result (and take the same stopping decision).
void SGDLearner::RunEpoch(int epoch, int job_type, sgd::Progress* prog) {
  tracker_->SetMonitor([prog](int node_id, const std::string& rets) { prog->Merge(rets); });
  const int nworkers = store_->NumWorkers();
  const int n = nworkers * param_.num_jobs_per_epoch;
  const bool sharded = dynamic_cast<ShardedDeviceStore*>(store_) != nullptr;
  std::vector<std::pair<int, std::string>> jobs;
  for (int i = 0; i < n; ++i) {
    if (sharded && i % nworkers != store_->Rank()) continue;
    sgd::Job job;
    job.type = job_type;
    job.epoch = epoch;
    job.num_parts = n;
    job.part_idx = i;
    jobs.emplace_back(0, std::string());
    job.SerializeToString(&jobs.back().second);
  }
  // exact_metrics = 1: the evaluator starts the pass empty; the worker loop appends every minibatch of it
  const bool exact = param_.exact_metrics == 1 && job_type != sgd::Job::kTraining;
  if (exact) {
    if (!eval_) DFH_CALL(dfh_eval_create(DeviceContext::Get(), 0, &eval_));
    DFH_CALL(dfh_eval_reset(eval_));
  }
  tracker_->Issue(jobs);
  while (tracker_->NumRemains()) std::this_thread::sleep_for(std::chrono::microseconds(200));
  if (sharded) MergeAcrossRanks(prog);
  if (exact) LogExactMetrics(job_type == sgd::Job::kValidation ? " - Validation (whole set): " : "whole file: ");
}

void SGDLearner::LogExactMetrics(const char* what) {
  dfh_eval_result r;
  DFH_CALL(dfh_eval_finish(CHECK_NOTNULL(eval_), &r));
  char num[3][40];
  const uint64_t rows = r.n - r.n_nan;
  if (r.n_pos && r.n_neg) {
    snprintf(num[0], sizeof(num[0]), "%.17g", static_cast<double>(r.auc2) / (2.0 * r.n_pos * r.n_neg));
  } else {
    snprintf(num[0], sizeof(num[0]), "undefined");
  }
  if (rows) {
    snprintf(num[1], sizeof(num[1]), "%.17g", r.objv / rows);
    snprintf(num[2], sizeof(num[2]), "%.17g", static_cast<double>(r.correct) / rows);
  } else {
    snprintf(num[1], sizeof(num[1]), "undefined");
    snprintf(num[2], sizeof(num[2]), "undefined");
  }
  LOG(INFO) << what << "rows=" << r.n << " pos=" << r.n_pos << " neg=" << r.n_neg << " nan=" << r.n_nan << " auc2=" << r.auc2
            << " auc=" << num[0] << " logloss=" << num[1] << " accuracy=" << num[2];
}

// task = predict (src/main.cc:61-62 is a TODO in the reference; sgd_param.h:24-28: "model_in ... should be specified if it
// is a prediction task").  One pass, no shuffling, no sampling, nothing pushed: every data part is a job of kind
// kPrediction whose worker loop is the validation loop (Localizer -> Pull -> FMLoss::Predict) plus the logits going to
// a file.  One process: the parts run in order and append to <pred_out>.  Sharded: rank r takes the parts i = r (mod
// ranks) and writes <pred_out>.part-<i>; the parts are consecutive byte ranges of the data, so concatenating the files
// in part order gives the predictions in file order.
void SGDLearner::RunPrediction() {
  CHECK(param_.model_in.size()) << "task=predict needs model_in (sgd_param.h:24-28)";
  CHECK(param_.pred_out.size()) << "task=predict needs pred_out=<file>";
  sgd::Progress prog;
  RunEpoch(0, sgd::Job::kPrediction, &prog);
  LOG(INFO) << "predicted " << prog.nrows << " examples of " << (param_.data_val.size() ? param_.data_val : param_.data_in)
            << " -> " << param_.pred_out << " (against their labels: " << prog.TextString() << ")";
}

const std::string& SGDLearner::JobData(const sgd::Job& job) const {
  if (job.type == sgd::Job::kTraining) return param_.data_in;
  if (job.type == sgd::Job::kPrediction) return param_.data_val.size() ? param_.data_val : param_.data_in;
  return param_.data_val;
}

void SGDLearner::WritePredictions(dfh_batch* b) {
  size_t nrows = 0;
  DFH_CALL(dfh_batch_shape(b, &nrows, nullptr, nullptr));
  pred_buf_.resize(nrows);
  if (nrows == 0) return;
  DFH_CALL(dfh_batch_get_pred(b, pred_buf_.data()));  // waits for the step
  for (size_t i = 0; i < nrows; ++i) {
    const float v = param_.pred_prob ? 1.0f / (1.0f + std::exp(-pred_buf_[i])) : pred_buf_[i];
    CHECK_GT(fprintf(CHECK_NOTNULL(pred_file_), "%.9g\n", v), 0) << "cannot write " << param_.pred_out;
  }
}

void SGDLearner::WaitPredWrite() {
  if (pred_write_.valid()) pred_write_.get();
}

// pred_write = device.  pred_prob = 1: the sigmoid stays the host's expression (the device's expf is not the C library's bit for
// bit, and pred_out must not depend on the key): the unit's logits come down, the probabilities go back up to be formatted
void SGDLearner::ClosePredUnit() {
  dfh_predtext* pt = CHECK_NOTNULL(predtext_);
  const size_t n = pred_unit_n_;
  pred_unit_n_ = 0;
  if (param_.pred_prob) {
    pred_buf_.resize(n);
    DFH_CALL(dfh_predtext_values(pt, pred_buf_.data()));
    for (size_t i = 0; i < n; ++i) pred_buf_[i] = 1.0f / (1.0f + std::exp(-pred_buf_[i]));
    DFH_CALL(dfh_predtext_reset(pt));
    DFH_CALL(dfh_predtext_append_host(pt, pred_buf_.data(), n));
  }
  size_t nbytes = 0;
  uint64_t irregular = 0;
  DFH_CALL(dfh_predtext_format(pt, &nbytes, &irregular));
  if (irregular == 0) {
    // unit u - 1 may still be on its way to the file out of the other buffer: its write overlaps this download, and ends
    // before this unit's write begins
    std::vector<char>& text = pred_text_[pred_text_cur_];
    pred_text_cur_ ^= 1;
    text.resize(nbytes);
    DFH_CALL(dfh_predtext_read(pt, text.data()));
    WaitPredWrite();
    FILE* f = CHECK_NOTNULL(pred_file_);
    const std::string* name = &param_.pred_out;
    pred_write_ = std::async(std::launch::async, [f, name, &text] {
      CHECK_EQ(fwrite(text.data(), 1, text.size(), f), text.size()) << "cannot write " << *name;
    });
    pred_counts_.dev_rows += n;
    ++pred_counts_.dev_units;
  } else {   // a value the device does not format: the whole unit as pred_write = host writes it
    if (!param_.pred_prob) {
      pred_buf_.resize(n);
      DFH_CALL(dfh_predtext_values(pt, pred_buf_.data()));
    }
    WaitPredWrite();
    for (size_t i = 0; i < n; ++i)
      CHECK_GT(fprintf(CHECK_NOTNULL(pred_file_), "%.9g\n", pred_buf_[i]), 0) << "cannot write " << param_.pred_out;
    pred_counts_.host_rows += n;
    ++pred_counts_.host_units;
  }
  DFH_CALL(dfh_predtext_reset(pt));
}

void SGDLearner::MergeAcrossRanks(sgd::Progress* prog) {
  auto* ss = dynamic_cast<ShardedDeviceStore*>(store_);
  if (!ss) return;
  double v[5] = {prog->loss, prog->penalty, prog->auc, prog->nnz_w, prog->nrows};
  DFH_CALL(dfh_comm_allreduce_sum(ss->comm(), v, 5));
  prog->loss = static_cast<real_t>(v[0]);
  prog->penalty = static_cast<real_t>(v[1]);
  prog->auc = static_cast<real_t>(v[2]);
  prog->nnz_w = static_cast<real_t>(v[3]);
  prog->nrows = static_cast<real_t>(v[4]);
}

// reference: SGDLearner::Process, sgd_learner.h:42-53
void SGDLearner::Process(const std::string& args, std::string* rets) {
  sgd::Progress prog;
  sgd::Job job;
  job.ParseFromString(args);
  if (job.type == sgd::Job::kTraining || job.type == sgd::Job::kValidation) {
    IterateData(job, &prog);
  } else if (job.type == sgd::Job::kPrediction) {
    const bool sharded = dynamic_cast<ShardedDeviceStore*>(store_) != nullptr;
    const std::string path = sharded ? param_.pred_out + ".part-" + std::to_string(job.part_idx) : param_.pred_out;
    pred_file_ = fopen(path.c_str(), (sharded || job.part_idx == 0) ? "w" : "a");
    CHECK(pred_file_) << "cannot open " << path;
    IterateData(job, &prog);
    CHECK_EQ(fclose(pred_file_), 0) << "cannot write " << path;
    pred_file_ = nullptr;
  }
  prog.SerializeToString(rets);
}

void SGDLearner::IterateData(const sgd::Job& job, sgd::Progress* prog) {
  if (GetUpdater()->device_param().device_path == "literal" && job.type != sgd::Job::kPrediction) {
    IterateDataLiteral(job, prog);  // sharded store too: its Push / Pull are collective, the loop keeps the ranks in step
  } else if (dynamic_cast<ShardedDeviceStore*>(store_)) {
    IterateDataSharded(job, prog);
  } else {
    IterateDataFused(job, prog);
  }
}

static size_t NnzOf(const dmlc::RowBlock<feaid_t>& blk) { return blk.offset[blk.size] - blk.offset[0]; }

// ---- the fused worker loop: sgd_learner.cc:129-227 on the device

/*! \brief what a job of the fused loop reads from */
struct SGDLearner::FusedSource {
  // data_cache = hbm (not for predictions): a part that is in the cache is read from there (cpart); one that is not yet is read
  // through the device feed whatever the job — training without a shuffle buffer and validation too, in buffers of batch_size x
  // max(shuffle, 1) rows that are read through in order — and its buffers are kept (cache_fill)
  bool cache_on = false, cache_fill = false;
  const CachedPart* cpart = nullptr;
  // minibatches are described and their rows gathered out of device row buffers (device_feed.h): those parts, and training
  // with a shuffle buffer (DIFACTO_HOST_FEED=1 keeps the host-side gather); else host arrays are loaded
  bool device_feed = false;
  // text_parse = device: the reader's parser threads hand every chunk of criteo text to the device, the ids stay in HBM with the
  // chunk's container.  A chunk that is not regular is left to the host parser (counted: logged at the end of the job)
  bool device_parse = false;
  // rec_decode = device: the same for the records of a .rec file, whose LZ4 blocks the device decodes (a record with values or
  // weights is left to the host decoder, counted)
  bool device_decode = false;
  // pred_write = device: the prediction job reads through the device feed too, in file order as a cache_fill validation job does
  // (buffers of batch_size x max(shuffle, 1) rows read through in order), without keeping the buffers
  bool pred_feed = false;
  bool in_order() const { return cache_fill || pred_feed; }
  bool uploads() const { return device_feed && !cpart; }   // the feed uploads the reader's buffers (a cached part's are there)
};

SGDLearner::FusedSource SGDLearner::SourceOf(const sgd::Job& job, const SgdLoopEnv& env) {
  FusedSource s;
  s.cache_on = param_.data_cache == "hbm" && job.type != sgd::Job::kPrediction;
  s.cpart = s.cache_on ? cache_.Find(job.type, job.part_idx) : nullptr;
  s.cache_fill = s.cache_on && !s.cpart && !cache_.refused.count(std::make_pair(job.type, job.part_idx));
  s.pred_feed = job.type == sgd::Job::kPrediction && param_.pred_write == "device";
  s.device_feed = s.cpart || s.cache_fill || s.pred_feed || (job.type == sgd::Job::kTraining && param_.shuffle > 0 && !env.host_feed);
  const bool criteo = param_.data_format == "criteo" || param_.data_format == "criteo_test";
  s.device_parse = GetUpdater()->device_param().text_parse == "device" && s.uploads() && criteo;
  s.device_decode = GetUpdater()->device_param().rec_decode == "device" && s.uploads() && param_.data_format == "rec";
  return s;
}

// Minibatches are cut (permutation + row selection) ahead on the reader's own thread, the reference's reader / executor
// overlap (sgd_learner.cc:196-224).  Device feed: buffers as slices of the parsed chunks (no host assembly), uploaded by the
// thread that builds them
BatchReader* SGDLearner::NewFusedReader(const sgd::Job& job, const FusedSource& src, const SgdLoopEnv& env, DeviceFeed* feed,
                                        DeviceTextParse* text_parse, DeviceRecDecode* rec_decode) {
  const bool train = job.type == sgd::Job::kTraining;
  const bool permute = train && param_.shuffle > 0;
  const unsigned cache_buf_rows = static_cast<unsigned>(param_.batch_size) * static_cast<unsigned>(std::max(param_.shuffle, 1));
  const float sampling = train ? param_.neg_sampling : 1.0f;
  if (src.cpart) return new BatchReader(new CachedBuffers(src.cpart), param_.batch_size, cache_buf_rows, sampling, permute);
  BatchReader::SliceFn upload;
  if (src.uploads()) {
    // (a buffer that is kept gets an allocation of its own size: nothing is created ahead)
    const size_t buf_rows = src.pred_feed ? cache_buf_rows : static_cast<size_t>(param_.batch_size) * param_.shuffle;
    feed->Start(src.cache_fill ? 0 : buf_rows, buf_rows * static_cast<size_t>(GetUpdater()->device_param().feed_ids_per_row));
    upload = [feed](const dmlc::RowBlock<feaid_t>& blk, const std::vector<BufSlice>& slices, uint64_t serial) {
      feed->Upload(blk, slices, serial);
    };
  }
  ParseHook parse_hook;
  if (src.device_parse) parse_hook = text_parse->Hook(DeviceContext::Get(), param_.data_format == "criteo" ? 1 : 0);
  if (src.device_decode) parse_hook = rec_decode->Hook(DeviceContext::Get());
  // the device parses: the parser threads only upload and wait (DeviceTextParse::kThreads; DIFACTO_PARSER_THREADS overrides)
  const int parser_threads = env.parser_threads_set  ? 0
                             : src.device_parse      ? DeviceTextParse::kThreads
                             : src.device_decode     ? DeviceRecDecode::kThreads
                                                     : 0;
  BatchReader* reader = new BatchReader(JobData(job), param_.data_format, job.part_idx, job.num_parts, param_.batch_size,
                                        src.in_order() ? cache_buf_rows : (train ? param_.batch_size * param_.shuffle : 0), sampling,
                                        src.device_feed, upload, src.in_order() ? permute : true, parse_hook, parser_threads);
  if (src.uploads()) reader->DescribeSlices(nullptr);
  return reader;
}

void SGDLearner::IterateDataFused(const sgd::Job& job, sgd::Progress* progress) {
  const SgdLoopEnv env;
  const FusedSource src = SourceOf(job, env);
  dfh_ctx* ctx = DeviceContext::Get();
  // DIFACTO_SINGLE_QUEUE=1: the single-queue step (csrc/dfh_riders.hip; minibatches then prepared TWO ahead so that every
  // stage finds a launch to ride in).  Off by default: through this loop it loses at every size (profiles/r06m_*: 1.59 against
  // 2.22 M rows/s at batch 100, 21.9 against 28.7 M at 2 000) — two queues hide the whole preparation behind the step
  DFH_CALL(dfh_ctx_set_option(ctx, "single_queue", env.single_queue ? 1 : 0));
  env.SetPrepPriorityOnce(ctx, src.device_feed);
  // preparation streams (DIFACTO_PREP_STREAMS=1..4; ignored on the single queue).  With the device feed the preparation is the
  // row gather + Localizer + probe, a chain as long as the step, and two streams let consecutive preparations overlap (.rec
  // 53.6 -> 59.4 M rows/s by this loop's clock); bench.py, whose inputs are in HBM already, loses 5 % with two: it keeps one
  DFH_CALL(dfh_ctx_set_pipeline(ctx, env.prep_streams ? env.prep_streams : (src.device_feed ? 2 : 1)));
  DeviceTextParse text_parse;   // (outlives the reader, whose parser threads count into it)
  DeviceRecDecode rec_decode;   // (the same)
  DeviceFeed feed(ctx, env);    // outlives the reader, whose thread uploads into it
  feed.cached = src.cpart;
  feed.retain = src.cache_fill;
  if (src.cache_fill && param_.data_cache_max_gb > 0) {
    const double cap = static_cast<double>(param_.data_cache_max_gb) * (1ULL << 30);
    feed.budget = cap > static_cast<double>(cache_.bytes) ? static_cast<size_t>(cap - static_cast<double>(cache_.bytes)) : 0;
  }
  // described minibatches are ~120 KB each: a deeper queue lets the loop ride out the reader's pause at a buffer boundary
  PrefetchSource reader(NewFusedReader(job, src, env, &feed, &text_parse, &rec_decode), src.device_feed ? BatchRing::kMax : 2);
  RunFused(job, src, env, &reader, &feed, progress);
  uint64_t nkeys;
  DFH_CALL(dfh_table_size(GetUpdater()->table(), &nkeys));  // surfaces a full table as an error
  if (src.device_parse) text_parse.Log(JobData(job));
  if (src.device_decode) rec_decode.Log(JobData(job));
  if (src.cache_on) CloseCachedJob(job, src, &feed);
}

// prepare minibatch t+1 (H2D copy or row gather, Localizer, key lookup) while minibatch t trains.  Minibatch i sits in object
// i mod nrot; `ahead` minibatches are prepared in front of the one that steps (1: prepare(i + 1), step(i) — the two minibatches
// the reference keeps in flight, sgd_learner.cc:219-223; 2 on the single queue)
void SGDLearner::RunFused(const sgd::Job& job, const FusedSource& src, const SgdLoopEnv& env, BatchSource* reader, DeviceFeed* feed,
                          sgd::Progress* progress) {
  const bool train = job.type == sgd::Job::kTraining;
  const bool predict = job.type == sgd::Job::kPrediction;
  const bool push_cnt = train && job.epoch == 0;  // sgd_learner.cc:201-202
  dfh_ctx* ctx = DeviceContext::Get();
  dfh_table* table = GetUpdater()->table();
  // objects in rotation: a dozen only where a dozen steps can be queued (the device feed's bursts); validation, prediction
  // and host-feed jobs have a prefetch depth of 2 and rotate three (six times the HBM and creation time for nothing)
  const int nrot = src.device_feed ? BatchRing::kMax : 3;
  const int ahead = env.single_queue ? 2 : 1;
  if (src.pred_feed) {
    if (!predtext_) DFH_CALL(dfh_predtext_create(ctx, 0, &predtext_));
    DFH_CALL(dfh_predtext_reset(predtext_));
    pred_unit_n_ = 0;
    pred_counts_ = PredCounts();
  }
  // DIFACTO_PROFILE=1: where the host thread of this loop spends its time (reader wait + batch assembly, staging + Localizer /
  // lookup queueing, step queueing; t_feed: inside the second, waiting for a buffer's upload), printed at the end of the job
  const bool prof = env.profile;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_read = 0, t_prep = 0, t_step = 0, t_feed = 0, t_first = 0;
  double t0 = prof ? now() : 0;
  auto lap = [&](double* t) { if (prof) { const double t1 = now(); *t += t1 - t0; t0 = t1; } };
  // the batch objects while the reader parses its first chunks (sizes: this job's batch_size at feed_ids_per_row — default 48,
  // the criteo rows of the reference's example have 39 — or what an earlier job left; a bigger minibatch re-creates them)
  if (src.device_feed && env.feed_precreate && !ring_.AllFit(nrot, 0, 0))
    ring_.Grow(ctx, nrot, param_.batch_size,
               static_cast<size_t>(param_.batch_size) * static_cast<size_t>(GetUpdater()->device_param().feed_ids_per_row), progress);
  const double t_created = prof ? now() : 0;
  std::vector<dfh_rowbuf*> bufs;
  std::vector<const uint32_t*> rows;
  std::vector<size_t> cnts;
  auto prepare = [&](dfh_batch* b) {   // the reader's current minibatch into b
    const auto& blk = reader->Value();
    if (env.trace && (blk.index || NnzOf(blk) == 0)) {
      uint64_t cs = 0;
      double ls = 0;
      for (size_t i = blk.offset[0]; i < blk.offset[blk.size]; ++i) cs += blk.index[i] * (i - blk.offset[0] + 1);
      for (size_t i = 0; i < blk.size; ++i) ls += blk.label[i] * (i + 1);
      LOG(INFO) << "batch rows " << blk.size << " nnz " << NnzOf(blk) << " off0 " << blk.offset[0]
                << " idxsum " << cs << " labsum " << ls << " value " << (blk.value != nullptr);
    }
    const std::vector<RowSeg>& segs = reader->Aux();
    if (!segs.empty()) {   // a described minibatch: its rows are gathered out of the device-resident buffers
      bufs.resize(segs.size());
      rows.resize(segs.size());
      cnts.resize(segs.size());
      const double tf = prof ? now() : 0;
      uint64_t last = 0;
      for (size_t g = 0; g < segs.size(); ++g) {
        bufs[g] = CHECK_NOTNULL(feed->Of(segs[g].buf));
        rows[g] = segs[g].rows.data();
        cnts[g] = segs[g].rows.size();
        last = std::max<uint64_t>(last, segs[g].buf);
      }
      if (prof) t_feed += now() - tf;
      // gather + Localizer (Localizer lc(-1, ...), sgd_learner.cc:203) + key lookup as one preparation phase
      // (DIFACTO_SPLIT_PREP=1: the three calls, for A/B)
      const int nseg = static_cast<int>(segs.size());
      if (src.cpart) {   // the buffers carry their offsets and labels: the row numbers are all that is sent
        DFH_CALL(dfh_batch_prepare_cached(table, b, blk.size, nseg, bufs.data(), rows.data(), cnts.data(), ~0ULL));
      } else if (env.split_prep) {
        DFH_CALL(dfh_batch_gather_rows(b, blk.size, blk.offset, blk.label, nseg, bufs.data(), rows.data(), cnts.data()));
      } else {
        DFH_CALL(dfh_batch_prepare_rows(table, b, blk.size, blk.offset, blk.label, nseg, bufs.data(), rows.data(), cnts.data(), ~0ULL));
      }
      // minibatches take their rows from the buffers in order: the buffers before this one's last are exhausted
      feed->Release(last);
      if (!env.split_prep || src.cpart) return;
    } else {
      DFH_CALL(dfh_batch_load_host(b, blk.size, blk.offset, blk.index, blk.value, blk.label));
    }
    DFH_CALL(dfh_localize(b, ~0ULL));  // Localizer lc(-1, ...), sgd_learner.cc:203
    DFH_CALL(dfh_batch_lookup(table, b));  // (dfh_localize_lookup does both in one pass; measured 0.4 % slower per step)
  };
  int prepared = 0, i = 0;   // minibatches prepared / stepped so far
  bool more = true;
  auto step_one = [&] {
    dfh_batch* b = ring_[BatchRing::SlotOf(i, nrot)];
    DFH_CALL(dfh_sgd_step(table, b, train ? 1 : 0, push_cnt ? 1 : 0));
    if (eval_ && !train) DFH_CALL(dfh_eval_append_batch(eval_, b));  // exact_metrics = 1: queued behind the step
    if (predict && src.pred_feed) {   // pred_write = device: queued behind the step, nothing waits
      DFH_CALL(dfh_predtext_append_batch(predtext_, b));
      size_t nrows = 0;
      DFH_CALL(dfh_batch_shape(b, &nrows, nullptr, nullptr));
      pred_unit_n_ += nrows;
      if (pred_unit_n_ >= static_cast<size_t>(param_.pred_unit_rows)) ClosePredUnit();
    } else if (predict) {
      WritePredictions(b);
    }
    ++i;
  };
  auto prepare_next = [&] {
    if (!more) return;
    more = reader->Next();
    if (prepared == 0 && prof) t_first = now();
    lap(&t_read);
    if (!more) return;
    const auto& blk = reader->Value();
    if (!ring_.AllFit(nrot, blk.size, NnzOf(blk))) {
      // growing re-creates ALL batch objects: the prepared, not yet trained minibatches go first, then the device drains
      while (i < prepared) step_one();
      lap(&t_step);
      DFH_CALL(dfh_ctx_sync(ctx));
      ring_.Grow(ctx, nrot, blk.size, NnzOf(blk), progress);
    }
    prepare(ring_[BatchRing::SlotOf(prepared, nrot)]);
    ++prepared;
    lap(&t_prep);
  };
  for (int a = 0; a < ahead; ++a) prepare_next();
  if (prof)
    LOG(INFO) << "start-up: batch objects " << t_created - (t_first - t_read) << " s, first minibatch from the reader after "
              << t_first - t_created << " s more, the first preparations queued in " << now() - t_first << " s";
  while (i < prepared) {
    prepare_next();
    step_one();
    lap(&t_step);
  }
  if (src.pred_feed) {   // a unit closes at the end of every data part
    if (pred_unit_n_) ClosePredUnit();
    WaitPredWrite();
    lap(&t_step);
  }
  if (prof)
    LOG(INFO) << "host loop over " << i << " minibatches: reader " << t_read << " s, stage + localize + lookup " << t_prep
              << " s (" << t_feed << " s of it waiting for a buffer's upload), step " << t_step << " s";
  if (src.pred_feed) {
    LOG(INFO) << "pred_write=device: " << pred_counts_.dev_rows << " rows in " << pred_counts_.dev_units
              << " units formatted on the device, " << pred_counts_.host_rows << " rows in " << pred_counts_.host_units
              << " units on the host";
  }
  ring_.Drain(progress);
}

// data_cache = hbm, one line per job: where its rows came from; a part that was read to be kept enters the cache, or is refused
void SGDLearner::CloseCachedJob(const sgd::Job& job, const FusedSource& src, DeviceFeed* feed) {
  const std::string what = "part " + std::to_string(job.part_idx) + " of " + std::to_string(job.num_parts) +
                           (job.type == sgd::Job::kTraining ? " (training): " : " (validation): ");
  const std::pair<int, int> ckey(job.type, job.part_idx);
  if (src.cpart) {
    LOG(INFO) << what << src.cpart->rows << " rows from the HBM cache";
  } else if (!src.cache_fill) {
    LOG(INFO) << what << "parsed from " << JobData(job) << ", not cached";
  } else if (std::unique_ptr<CachedPart> part = feed->TakeCache()) {
    LOG(INFO) << what << part->rows << " rows parsed from " << JobData(job) << ", cached " << (part->bytes + (1 << 19)) / (1 << 20) << " MB";
    cache_.bytes += part->bytes;
    cache_.parts[ckey] = std::move(part);
  } else {
    LOG(WARNING) << what << "does not fit the HBM cache: its " << feed->rows_seen << " rows need " << feed->need_bytes << " bytes, "
                 << feed->budget << " are left of data_cache_max_gb=" << param_.data_cache_max_gb << "; it is read from "
                 << JobData(job) << " in every epoch";
    LOG(INFO) << what << feed->rows_seen << " rows parsed from " << JobData(job) << ", not cached";
    cache_.refused[ckey] = true;
  }
}

// ---- the sharded worker loop: sgd_learner.cc:129-227 with Store::Pull / Push turned into the exchange of
// dfh_shard_step.  The ranks step together; a rank whose part of the data is exhausted keeps serving
// its shard (b = NULL) until nobody has a minibatch left.  Four batch objects in rotation: while minibatch t steps,
// minibatch t+1 — copied in and localized one step EARLIER — has its per-owner key counts (and, overlapped, its keys
// and rows) exchanged inside the running step (dfh_shard_prefetch_counts), and minibatch t+2 is copied in and localized
// on the preparation stream: the keys of t+1 are ready when step t starts (round 5: localized only one ahead, the
// Localizer of t+1 ran beside step t's forward and the exchange waited for it).  The two minibatches the
// reference's batch tracker keeps in flight (sgd_learner.cc:219-223), without its staleness in sync mode.
void SGDLearner::IterateDataSharded(const sgd::Job& job, sgd::Progress* progress) {
  const SgdLoopEnv env;
  const bool train = job.type == sgd::Job::kTraining;
  const bool predict = job.type == sgd::Job::kPrediction;
  const bool push_cnt = train && job.epoch == 0;  // sgd_learner.cc:201-202
  auto* ss = CHECK_NOTNULL(dynamic_cast<ShardedDeviceStore*>(store_));
  // minibatches are cut (permutation + row gather) two ahead on the reader's own thread, the reference's reader /
  // executor overlap (sgd_learner.cc:196-224)
  PrefetchSource reader(new BatchReader(JobData(job), param_.data_format, job.part_idx, job.num_parts, param_.batch_size,
                                        train ? param_.batch_size * param_.shuffle : 0, train ? param_.neg_sampling : 1.0f), 2);
  dfh_ctx* ctx = DeviceContext::Get();
  DFH_CALL(dfh_ctx_set_option(ctx, "single_queue", 0));  // (a fused job of small minibatches may have left it on)
  DFH_CALL(dfh_ctx_set_pipeline(ctx, 1));
  constexpr int kSlots = 4;
  ring_.TakeOverForSlots(kSlots, progress);
  // minibatch t of this rank into its slot (whose previous occupant, t - kSlots, has been stepped), or NULL.  Only that slot
  // grows: the others may hold prepared minibatches that have not stepped yet
  auto prepare = [&](int t) -> dfh_batch* {
    if (!reader.Next()) return nullptr;
    const auto& blk = reader.Value();
    const int q = BatchRing::SlotOf(t, kSlots);
    if (!ring_.Fits(q, blk.size, NnzOf(blk))) ring_.GrowSlot(ctx, q, blk.size, NnzOf(blk), progress);
    DFH_CALL(dfh_batch_load_host(ring_[q], blk.size, blk.offset, blk.index, blk.value, blk.label));
    DFH_CALL(dfh_localize(ring_[q], ~0ULL));  // Localizer lc(-1, ...), sgd_learner.cc:203
    return ring_[q];
  };
  dfh_batch* cur = prepare(0);
  dfh_batch* nxt = prepare(1);   // localized a step before it is announced
  int active = 1;
  for (int i = 0; active; ++i) {
    dfh_batch* ahead = prepare(i + 2);
    DFH_CALL(dfh_shard_prefetch_counts(ss->shard(), nxt));
    if (env.trace) LOG(INFO) << "shard step: batch " << (cur ? "yes" : "none");
    DFH_CALL(dfh_shard_step(ss->shard(), cur, train ? 1 : 0, push_cnt ? 1 : 0, &active));
    if (predict && cur) WritePredictions(cur);
    if (env.trace) LOG(INFO) << "shard step done: active " << active;
    cur = nxt;
    nxt = ahead;
  }
  ring_.NormalizeSlots(kSlots, progress);
  uint64_t nkeys;
  DFH_CALL(dfh_table_size(GetUpdater()->table(), &nkeys));  // surfaces a full shard as an error
}

// reference: SGDLearner::GetPos, sgd_learner.cc:113-127
void SGDLearner::GetPos(const SArray<int>& len, SArray<int>* w_pos, SArray<int>* V_pos) {
  const size_t n = len.size();
  w_pos->resize(n);
  V_pos->resize(n);
  int p = 0;
  for (size_t i = 0; i < n; ++i) {
    const int l = len[i];
    (*w_pos)[i] = l == 0 ? -1 : p;
    (*V_pos)[i] = l > 1 ? p + 1 : -1;
    p += l;
  }
}

// reference: SGDLearner::EvaluatePenalty, sgd_learner.cc:249-273
real_t SGDLearner::EvaluatePenalty(const SArray<real_t>& weights, const SArray<int>& w_pos, const SArray<int>& V_pos) {
  double objv = 0;
  const auto& param = GetUpdater()->param();
  if (w_pos.size()) {
    for (int p : w_pos) {
      if (p == -1) continue;
      const double w = weights[p];
      objv += param.l1 * std::fabs(w) + .5 * param.l2 * w * w;
    }
    for (int p : V_pos) {
      if (p == -1) continue;
      for (int i = 0; i < param.V_dim; ++i) {
        const double V = weights[p + i];
        objv += .5 * param.V_l2 * V * V;
      }
    }
  } else {
    for (auto wf : weights) {
      const double w = wf;
      objv += param.l1 * std::fabs(w) + .5 * param.l2 * w * w;
    }
  }
  return static_cast<real_t>(objv);
}

// ---- the literal worker loop: the reference's sequence of interface calls
void SGDLearner::IterateDataLiteral(const sgd::Job& job, sgd::Progress* progress) {
  const bool train = job.type == sgd::Job::kTraining;
  const bool push_cnt = train && job.epoch == 0;
  PrefetchSource reader(new BatchReader(train ? param_.data_in : param_.data_val, param_.data_format, job.part_idx, job.num_parts,
                                        param_.batch_size, train ? param_.batch_size * param_.shuffle : 0,
                                        train ? param_.neg_sampling : 1.0f), 2);
  // the sharded store's Push / Pull are collective: every rank makes the same calls until no rank has a minibatch
  // left; a rank whose part of the data is exhausted goes on with empty arrays
  auto* ss = dynamic_cast<ShardedDeviceStore*>(store_);
  bool more = true;
  for (;;) {
    const bool have = more && reader.Next();
    more = have;
    if (ss) {
      double any = have ? 1.0 : 0.0;
      DFH_CALL(dfh_comm_allreduce_sum(ss->comm(), &any, 1));
      if (any == 0.0) break;
    } else if (!have) {
      break;
    }
    dmlc::data::RowBlockContainer<unsigned> data;
    auto feaids = std::make_shared<std::vector<feaid_t>>();
    auto feacnt = std::make_shared<std::vector<real_t>>();
    if (have) {
      Localizer lc(-1, blk_nthreads_);
      lc.Compact(reader.Value(), &data, feaids.get(), push_cnt ? feacnt.get() : nullptr);
    }
    SArray<feaid_t> keys(feaids);
    if (push_cnt) store_->Wait(store_->Push(keys, Store::kFeaCount, SArray<real_t>(feacnt), {}));
    SArray<real_t> values;
    SArray<int> lengths;
    store_->Wait(store_->Pull(keys, Store::kWeight, &values, &lengths));
    SArray<real_t> grads;
    if (have) {
      auto blk = data.GetBlock();
      progress->nrows += blk.size;
      SArray<real_t> pred(blk.size);
      SArray<int> w_pos, V_pos;
      GetPos(lengths, &w_pos, &V_pos);
      std::vector<SArray<char>> inputs = {SArray<char>(values), SArray<char>(w_pos), SArray<char>(V_pos)};
      loss_->Predict(blk, inputs, &pred);
      progress->loss += loss_->Evaluate(blk.label, pred);
      progress->penalty += EvaluatePenalty(values, w_pos, V_pos);
      float auc_n = 0;
      DFH_CALL(dfh_auc_times_n(DeviceContext::Get(), blk.label, pred.data(), pred.size(), &auc_n));
      progress->auc += auc_n;
      if (train) {
        grads.resize(values.size());
        inputs.push_back(SArray<char>(pred));
        loss_->CalcGrad(blk, inputs, &grads);
      }
    }
    if (train) store_->Wait(store_->Push(keys, Store::kGradient, grads, lengths));
  }
}

// Updater::Save / Load.  A sharded run writes one part per rank plus a manifest and reads exactly the parts the manifest
// names, keeping the keys of its own range (model_parts.h).
void SGDLearner::SaveModel() {
  auto* ss = dynamic_cast<ShardedDeviceStore*>(store_);
  SaveModelParts(ss ? ss->comm() : nullptr, store_->Rank(), store_->NumWorkers(), param_.model_out, [&](const std::string& tmp) {
    std::unique_ptr<dmlc::Stream> fo(dmlc::Stream::Create(tmp.c_str(), "w"));
    GetUpdater()->Save(true, fo.get());
  });
}

void SGDLearner::LoadModel() {
  auto* ss = dynamic_cast<ShardedDeviceStore*>(store_);
  if (!ss) {
    std::unique_ptr<dmlc::Stream> fi(dmlc::Stream::Create(param_.model_in.c_str(), "r"));
    bool has_aux = false;
    GetUpdater()->Load(fi.get(), &has_aux);
    LOG(INFO) << "model loaded from " << param_.model_in << (has_aux ? " (with optimiser state)" : "");
    return;
  }
  uint64_t lo = 0, hi = 0, total = 0;
  DFH_CALL(dfh_shard_owned_range(ss->shard(), ss->splits(), &lo, &hi));   // the range the shard serves
  // how many parts: the manifest of the save; a model saved before manifests existed: every part up to the first gap
  int want = -1;
  const std::string mf = param_.model_in + ".parts";
  if (FILE* f = fopen(mf.c_str(), "r")) {
    CHECK(fscanf(f, "%d", &want) == 1 && want >= 1 && want <= 4096) << "bad model manifest " << mf;
    fclose(f);
  } else {
    LOG(WARNING) << "no manifest " << mf << ": reading " << param_.model_in << ".part-<n> up to the first gap";
  }
  int parts = 0;
  for (;; ++parts) {
    if (want >= 0 && parts == want) break;
    const std::string path = param_.model_in + ".part-" + std::to_string(parts);
    if (access(path.c_str(), R_OK) != 0) {
      CHECK(want < 0) << "model part " << path << " is missing (the manifest names " << want << " parts)";
      break;
    }
    uint64_t n = 0;
    int aux = 0;
    DFH_CALL(dfh_table_load(GetUpdater()->table(), path.c_str(), lo, hi, &aux, &n));
    total += n;
  }
  CHECK_GT(parts, 0) << "no model part files " << param_.model_in << ".part-<n>";
  LOG(INFO) << "rank " << store_->Rank() << ": " << total << " entries of its key range loaded from " << parts << " part files";
}

}  // namespace difacto
