/**
 * lbfgs_learner.cc — LBFGSLearner (lbfgs_learner.h).  Reference: src/lbfgs/lbfgs_learner.cc.
 */
#include "./lbfgs_learner.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iomanip>
#include <memory>
#include <thread>
#include "./batch_reader.h"
#include "./comm_setup.h"
#include "./device_context.h"
#include "./model_parts.h"
#include "./resident_data.h"

namespace difacto {

DMLC_REGISTER_PARAMETER(LBFGSLearnerParam);
DMLC_REGISTER_PARAMETER(LBFGSUpdaterParam);

LBFGSLearner::~LBFGSLearner() {
  if (obj_) dfh_lbfgs_destroy(obj_);
  if (comm_) dfh_comm_destroy(comm_);
}

KWArgs LBFGSLearner::Init(const KWArgs& kwargs) {
  for (const auto& kw : kwargs)
    CHECK(!(kw.first == "task" && kw.second == "predict"))
        << "learner = lbfgs has no prediction task: train with model_out=<file>, then score with "
           "task=predict learner=sgd model_in=<file> V_dim=<V_dim> pred_out=<file>";
  const char* nw = getenv("DMLC_NUM_WORKER");
  const char* role = getenv("DMLC_ROLE");
  // one process per GPU only with the whole environment of a rank; a scheduler or server role is refused as the
  // sharded store of learner = sgd refuses it
  if (role && std::string(role) != "worker") ReadRankEnv();
  const bool sharded = role && nw && getenv("DIFACTO_RANK") && getenv("DIFACTO_RENDEZVOUS");
  CHECK(sharded || (!IsDistributed() && !(nw && atoi(nw) > 1)))
      << "learner = lbfgs runs in one process on one GPU: a sharded store (DMLC_ROLE / DMLC_NUM_WORKER > 1) is not supported";
  // lbfgs_learner.cc:369-393
  auto remain = Learner::Init(kwargs);
  remain = param_.InitAllowUnknown(remain);
  nthreads_ = param_.num_threads <= 0 ? static_cast<int>(std::thread::hardware_concurrency()) : param_.num_threads;
  remain = updater_.Init(remain);
  CHECK(param_.loss == "fm" || param_.loss == "logit") << "unknown loss type: " << param_.loss << " (this build provides fm and logit)";
  const int k = param_.loss == "logit" ? 0 : updater_.param().V_dim;
  if (sharded) {
    const RankEnv env = ReadRankEnv();   // before the device context: the rank's device
    rank_ = env.rank;
    world_ = env.world;
    comm_ = ConnectRanks(rank_, world_, &files_, 120.0);
    LOG(INFO) << "lbfgs: rank " << rank_ << " of " << world_ << " connected (" << (files_ ? "file transport" : "RCCL")
              << "): a worker for part " << rank_ << " of the data and the server of one key range";
    DFH_CALL(dfh_lbfgs_create_sharded(DeviceContext::Get(), comm_, k, updater_.param().m, &obj_));
  } else {
    DFH_CALL(dfh_lbfgs_create(DeviceContext::Get(), k, updater_.param().m, &obj_));
  }
  return remain;
}

void LBFGSLearner::PrepareData(std::vector<real_t>* rets) {
  // Reader blocks of data_chunk_size MB (lbfgs_learner.cc:167-171); a block beyond the batch object's 32-bit positions
  // is cut by rows
  const size_t chunk_bytes = std::max<size_t>(64, static_cast<size_t>(param_.data_chunk_size * 1024 * 1024));
  double cnt[6] = {0, 0, 0, 0, 0, 0};
  auto read = [&](const std::string& uri, int is_val, double* out) {
    Reader reader(uri, param_.data_format, rank_, world_, chunk_bytes);   // part rank_ of world_
    size_t nrows = 0, nnz = 0, nchunks = 0;
    ForEachChunk(&reader, kMaxChunkNnz, [&](size_t r0, size_t r1, const dmlc::RowBlock<feaid_t>& blk) {
      DFH_CALL(dfh_lbfgs_add_chunk(obj_, is_val, r1 - r0, blk.offset + r0, blk.index, blk.value, blk.label + r0));
      ++nchunks;
      nrows += r1 - r0;
      nnz += blk.offset[r1] - blk.offset[r0];
    });
    out[0] = nrows;
    out[1] = nchunks;
    out[2] = nnz;
  };
  read(param_.data_in, 0, cnt);
  if (param_.data_val.size()) read(param_.data_val, 1, cnt + 3);
  if (comm_) {
    LOG(INFO) << "rank " << rank_ << ": " << cnt[0] << " training examples in " << cnt[1] << " chunks";
    DFH_CALL(dfh_comm_allreduce_sum(comm_, cnt, 6));   // the counts the log shows are global
  }
  rets->assign(cnt, cnt + 6);
}

void LBFGSLearner::InitServer(std::vector<real_t>* rets) {
  const auto& p = updater_.param();
  uint64_t nkeys = 0, n = 0;
  DFH_CALL(dfh_lbfgs_init_model(obj_, static_cast<float>(p.tail_feature_filter), p.V_threshold, p.V_init_scale, p.l2, p.V_l2,
                                &nkeys, &n));
  DFH_CALL(dfh_lbfgs_set_l1(obj_, p.l1));   // l1 = 0 leaves the object as it is; r(w) below includes l1 |w|
  if (updater_.weight_initializer()) {  // SetWeightInitializer (lbfgs_updater.h:54-56): weight_lens_ is empty without V
    SArray<int> lens;
    SArray<real_t> w(n, 0);
    if (p.V_dim) {
      lens.resize(nkeys);
      DFH_CALL(dfh_lbfgs_get_model(obj_, nullptr, lens.data(), nullptr, nullptr));
    }
    updater_.weight_initializer()(lens, &w);
    DFH_CALL(dfh_lbfgs_set_weights(obj_, w.data()));
  }
  if (param_.model_in.size()) LoadModel(nkeys);
  float nnz = 0, r = 0;
  DFH_CALL(dfh_lbfgs_evaluate(obj_, nullptr, &nnz, &r));
  double total = static_cast<double>(n);   // this rank's slice; the log shows the model's size
  if (comm_) {
    LOG(INFO) << "rank " << rank_ << " owns " << nkeys << " keys, " << n << " parameters";
    DFH_CALL(dfh_comm_allreduce_sum(comm_, &total, 1));
  }
  rets->assign({r, static_cast<real_t>(total)});
}

float LBFGSLearner::Direction() {
  // PrepareCalcDirection then CalcDirection (lbfgs_updater.h:86-123); the B matrix and the two-loop coefficients are
  // host work (lbfgs_twoloop.h:45-107), the vectors stay on the device
  std::vector<real_t> incr(6 * updater_.param().m + 1), coef;
  int hist = 0;
  DFH_CALL(dfh_lbfgs_prepare_direction(obj_, incr.data(), &hist));
  float pg = 0;
  if (hist == 0) {   // no (s, y) pair yet: p = -g
    DFH_CALL(dfh_lbfgs_calc_direction(obj_, nullptr, &pg));
    return pg;
  }
  incr.resize(6 * hist + 1);
  twoloop_.ApplyIncreB(incr);
  // orthant-wise: without the curvature test a pair can have <s, y> <= 0 (incr_B[hist + hist - 1] = <s_last, y_last>); it
  // leaves both rings and B before the coefficients divide by it
  if (updater_.param().l1 > 0 && !(incr[2 * hist - 1] > 0)) {
    LOG(INFO) << " - <s,y> = " << incr[2 * hist - 1] << " <= 0: the pair is dropped";
    DFH_CALL(dfh_lbfgs_drop_last_pair(obj_));
    twoloop_.DropLast();
    if (--hist == 0) {   // no pair left: p = -pg
      DFH_CALL(dfh_lbfgs_calc_direction(obj_, nullptr, &pg));
      return pg;
    }
  }
  twoloop_.CalcCoefficients(&coef);
  DFH_CALL(dfh_lbfgs_calc_direction(obj_, coef.data(), &pg));
  return pg;
}

real_t LBFGSLearner::LineSearch(real_t step, real_t objv, float pg, float* auc) {
  // backtracking until both Wolfe conditions hold, at most max_num_linesearchs trials (lbfgs_learner.cc:52-73)
  real_t f = objv;
  const int trials = param_.max_num_linesearchs;
  const bool owlqn = updater_.param().l1 > 0;
  for (int t = 1; t <= trials; ++t, step *= param_.rho) {
    float trial_pg = 0;
    DFH_CALL(dfh_lbfgs_line_search(obj_, step, param_.gamma, &f, &trial_pg, auc));
    LOG(INFO) << " - alpha = " << step << ", objv = " << f << ", <p,g> = " << trial_pg;
    if (owlqn) {
      // trial_pg = sum pg (w - w0) of the projected step: sufficient decrease alone, no curvature test
      if (f <= objv + param_.c1 * trial_pg) {
        LOG(INFO) << " - sufficient decrease is satisfied";
        break;
      }
      if (t == trials) LOG(INFO) << " - reach the maximal number of linesearch steps [" << t << "]";
      continue;
    }
    const bool decrease = f <= objv + param_.c1 * step * pg;   // sufficient decrease
    const bool curvature = trial_pg >= param_.c2 * pg;         // curvature
    if (decrease && curvature) {
      LOG(INFO) << " - wolfe condition is satisifed";
      break;
    }
    if (t == trials) LOG(INFO) << " - reach the maximal number of linesearch steps [" << t << "]";
  }
  return f;
}

void LBFGSLearner::RunScheduler() {
  // lbfgs_learner.cc:14-126, with the worker / server jobs as calls on the dfh_lbfgs object
  LOG(INFO) << "Staring training using L-BFGS with " << nthreads_ << " threads";
  LOG(INFO) << "Scaning data... ";
  std::vector<real_t> scan;
  PrepareData(&scan);
  const real_t ntrain = scan[0], train_chunks = scan[1], train_nnz = scan[2];
  const real_t nval = scan[3], val_chunks = scan[4];
  LOG(INFO) << " - found " << ntrain << " training examples, splitted into " << train_chunks << " chunks";
  if (nval > 0) LOG(INFO) << " - found " << nval << " validation examples, splitted into " << val_chunks << " chunks";

  std::vector<real_t> init;   // {r(w), parameters}
  InitServer(&init);
  LOG(INFO) << "Inited model with " << init[1] << " parameters";
  float loss0 = 0, auc = 0;
  DFH_CALL(dfh_lbfgs_calc_grad(obj_, param_.gamma, &loss0, &auc));
  real_t f_prev = init[0] + loss0;   // the scheduler adds the server's and the worker's share

  const bool owlqn = updater_.param().l1 > 0;
  if (owlqn)
    LOG(INFO) << "l1 = " << updater_.param().l1 << ": orthant-wise L-BFGS on w; the line search accepts on sufficient "
              << "decrease alone, c2 is unused";
  real_t prev_val_auc = 0;
  for (int epoch = std::max(param_.load_epoch, 0); epoch < param_.max_num_epochs; ++epoch) {
    LOG(INFO) << "Epoch " << epoch << ":";
    const float pg = Direction();
    if (owlqn && pg == 0) {   // no descent direction in any orthant: w is optimal
      LOG(INFO) << " - pseudo-gradient is zero: objv = " << std::setprecision(8) << f_prev << std::setprecision(6) << ", training stops";
      break;
    }
    LOG(INFO) << " - start linesearch with objv = " << f_prev << ", <p,g> = " << pg;
    // the first epoch's step: init_alpha, or #examples / #nonzeros when it is not positive
    real_t step = param_.alpha;
    if (epoch == 0) step = param_.init_alpha > 0 ? param_.init_alpha : ntrain / train_nnz;
    const real_t f = LineSearch(step, f_prev, pg, &auc);

    // Evaluate job (lbfgs_learner.cc:77-88): training AUC of the last gradient pass, validation AUC, nnz(w)
    float val_auc_n = 0, nnz = 0;
    DFH_CALL(dfh_lbfgs_evaluate(obj_, nval > 0 ? &val_auc_n : nullptr, &nnz, nullptr));
    lbfgs::Progress prog{f, auc / ntrain, val_auc_n, nnz};
    LOG(INFO) << " - training AUC = " << prog.auc;
    if (owlqn) LOG(INFO) << " - nnz(w) = " << static_cast<uint64_t>(nnz);
    if (nval > 0) {
      prog.val_auc /= nval;
      LOG(INFO) << " - validation AUC = " << prog.val_auc;
    }
    for (const auto& cb : epoch_end_callback_) cb(epoch, prog);
    if (owlqn) {
      double moved = 0;
      DFH_CALL(dfh_lbfgs_get_owlqn_moved(obj_, &moved));
      if (moved == 0) {
        LOG(INFO) << " - no coordinate moved, training stops";
        break;
      }
    }

    // stop tests, only once more than min_num_epochs have passed (lbfgs_learner.cc:92-110)
    if (epoch > param_.min_num_epochs) {
      const real_t rel = fabs(f - f_prev) / f_prev;
      if (rel < param_.stop_rel_objv) {
        LOG(INFO) << "Change of objective [" << rel << "] < stop_rel_objv [" << param_.stop_rel_objv << "]";
        break;
      }
      const real_t gain = prog.val_auc - prev_val_auc;
      if (nval > 0 && gain < param_.stop_val_auc) {
        LOG(INFO) << "Change of validation AUC [" << gain << "] < stop_val_auc [" << param_.stop_val_auc << "]";
        break;
      }
    }
    if (epoch + 1 >= param_.max_num_epochs) LOG(INFO) << "Reach maximal number of epochs";
    f_prev = f;
    prev_val_auc = prog.val_auc;
  }
  LOG(INFO) << "Training is done";
  if (param_.model_out.size()) SaveModel();
}

// model_in: the file's entries of this rank's key range (the whole model in one process) joined onto the model's keys on
// the device (dfh_lbfgs_set_model): w, and V where both the file and the model carry one
void LBFGSLearner::LoadModel(uint64_t nkeys) {
  const int k = param_.loss == "logit" ? 0 : updater_.param().V_dim;
  uint64_t lo = 0, hi = 0;
  DFH_CALL(dfh_lbfgs_owned_range(obj_, &lo, &hi));
  ModelEntries m;
  LoadModelEntries(param_.model_in, lo, hi, &m);
  CHECK(k == 0 || m.V_dim == k) << "model_in " << param_.model_in << " has V_dim = " << m.V_dim << ", this job has V_dim = " << k;
  const size_t n = m.keys.size();
  std::vector<int> lens(n, 1);
  std::vector<real_t> vals;
  vals.reserve(n * (1 + static_cast<size_t>(k)));
  for (size_t i = 0; i < n; ++i) {
    vals.push_back(m.w[i]);
    if (k && m.has_V[i]) {
      lens[i] = 1 + k;
      vals.insert(vals.end(), m.V.begin() + static_cast<size_t>(k) * i, m.V.begin() + static_cast<size_t>(k) * (i + 1));
    }
  }
  uint64_t matched = 0;
  DFH_CALL(dfh_lbfgs_set_model(obj_, n, m.keys.data(), lens.data(), vals.data(), &matched));   // collective; matched: over ranks
  double tot[2] = {static_cast<double>(n), static_cast<double>(nkeys)};
  if (comm_) DFH_CALL(dfh_comm_allreduce_sum(comm_, tot, 2));   // the log line shows the job's counts on every rank
  LOG(INFO) << "model loaded from " << param_.model_in << ": " << matched << " of " << static_cast<uint64_t>(tot[0])
            << " keys matched " << static_cast<uint64_t>(tot[1]) << " model keys";
}

// the final weights as learner = sgd's model file without optimiser state (dfh_table_save, save_aux = 0)
void LBFGSLearner::SaveModel() {
  uint64_t nkeys = 0, n = 0;
  DFH_CALL(dfh_lbfgs_shape(obj_, &nkeys, &n, nullptr, nullptr));
  std::vector<uint64_t> keys(nkeys);
  std::vector<int> lens(nkeys);
  std::vector<float> cnt(nkeys), w(n);
  DFH_CALL(dfh_lbfgs_get_model(obj_, keys.data(), lens.data(), cnt.data(), w.data()));
  const int k = param_.loss == "logit" ? 0 : updater_.param().V_dim;
  std::vector<float> scal(4 * nkeys, 0.f), V(static_cast<size_t>(2) * k * nkeys, 0.f);
  std::vector<int> has(nkeys, 0);
  size_t p = 0;
  for (size_t i = 0; i < nkeys; ++i) {
    scal[4 * i] = cnt[i];   // {fea_cnt, w, sqrt_g, z}
    scal[4 * i + 1] = w[p];
    has[i] = lens[i] > 1;
    for (int j = 1; j < lens[i]; ++j) V[2 * k * i + j - 1] = w[p + j];
    p += lens[i];
  }
  // a sharded run: this rank's key range into <model_out>.part-<rank>, committed with the manifest (model_parts.h)
  SaveModelParts(comm_, rank_, world_, param_.model_out, [&](const std::string& tmp) {
    SaveDenseModel(tmp, k, nkeys, keys.data(), scal.data(), has.data(), V.data());
  });
}

}  // namespace difacto
