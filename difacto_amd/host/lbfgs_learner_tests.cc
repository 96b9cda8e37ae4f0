/**
 * lbfgs_learner_tests.cc — the reference's LBFGSLearner tests (tests/cpp/lbfgs_learner_test.cc:8-146) restated through
 * Learner::Create("lbfgs"): the per-epoch objective of 19 epochs on tests/golden/rcv1_100.libsvm (= the reference's
 * tests/data) against its golden trajectories.
 *
 *   difacto_lbfgs_tests <data> [data_chunk_size in MB]
 *
 * Prints one "<case> epoch <k> objv <value>" line per epoch and "<case> ok" / "<case> FAILED"; exits 1 on any failure.
 */
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>
#include "./lbfgs_learner.h"

using namespace difacto;

static int failures = 0;

static void RunCase(const char* name, const std::string& data, const std::string& chunk_mb, KWArgs args,
                    const std::vector<real_t>& objv, double tol, const LBFGSUpdater::WeightInitializer& init = nullptr) {
  std::unique_ptr<Learner> base(Learner::Create("lbfgs"));
  LBFGSLearner* learner = static_cast<LBFGSLearner*>(base.get());
  args.insert(args.begin(), {"data_in", data});
  if (!chunk_mb.empty()) args.push_back({"data_chunk_size", chunk_mb});
  auto remain = learner->Init(args);
  bool ok = remain.empty();   // EXPECT_EQ(remain.size(), 0)
  if (init) learner->GetUpdater()->SetWeightInitializer(init);
  int epochs = 0;
  double worst = 0;
  learner->AddEpochEndCallback([&](int epoch, const lbfgs::Progress& prog) {
    printf("%s epoch %d objv %.9g\n", name, epoch, prog.objv);
    const double err = std::fabs(static_cast<double>(objv[epoch]) - prog.objv);
    worst = std::max(worst, err);
    if (!(err < tol)) ok = false;
    ++epochs;
  });
  learner->Run();
  if (epochs != 19) ok = false;
  printf("%s %s (%d epochs, worst |objv - golden| = %.3g, tolerance %g)\n", name, ok ? "ok" : "FAILED", epochs, worst, tol);
  fflush(stdout);
  if (!ok) ++failures;
}

int main(int argc, char* argv[]) {
  if (argc < 2) {
    fprintf(stderr, "usage: difacto_lbfgs_tests <data> [data_chunk_size]\n");
    return 2;
  }
  const std::string data = argv[1], chunk = argc > 2 ? argv[2] : "";
  // lbfgs_learner_test.cc:8-46
  RunCase("Basic", data, chunk,
          {{"m", "5"}, {"V_dim", "0"}, {"l2", "0"}, {"init_alpha", "1"}, {"tail_feature_filter", "0"}, {"max_num_epochs", "19"}},
          {34.603421, 12.655075, 5.224232, 2.713903, 1.290586, 0.645131, 0.317889, 0.156723, 0.075331, 0.032091, 0.018044,
           0.008562, 0.004336, 0.002132, 0.001051, 0.000506, 0.000227, 0.000119, 0.000059},
          1e-5);
  // :48-84
  RunCase("RemoveTailFeatures", data, chunk,
          {{"m", "5"}, {"V_dim", "0"}, {"init_alpha", "1"}, {"l2", "0"}, {"tail_feature_filter", "2"}, {"max_num_epochs", "19"}},
          {43.865008, 21.728511, 10.893458, 5.038567, 2.293318, 1.064151, 0.518891, 0.257997, 0.128646, 0.064974, 0.028329,
           0.016543, 0.007910, 0.004053, 0.002001, 0.000978, 0.000437, 0.000216, 0.000112},
          1e-5);
  // :86-146
  // WithV's weight initializer (lbfgs_learner_test.cc:128-138): w = 0, and the V entries of a key centred on zero in
  // steps of .01, V_j = (j - (len - 1) / 2) * .01 for j = 1 .. len - 1
  auto centred_V = [](const SArray<int>& lens, SArray<real_t>* w) {
    size_t at = 0;
    for (size_t key = 0; key < lens.size(); ++key) {
      const int len = lens[key];
      const real_t mid = (len - 1) / 2.0f;
      for (int j = 1; j < len; ++j) (*w)[at + j] = (j - mid) * .01;
      at += len;
    }
  };
  RunCase("WithV", data, chunk,
          {{"m", "5"}, {"V_dim", "5"}, {"l2", ".1"}, {"init_alpha", "1"}, {"V_l2", ".01"}, {"V_threshold", "0"}, {"rho", ".5"},
           {"tail_feature_filter", "0"}, {"max_num_epochs", "19"}},
          {35.224265, 21.631514, 18.394319, 16.077692, 12.389012, 8.888516, 8.446880, 8.146090, 8.023501, 7.981967, 7.955119,
           7.937092, 7.922456, 7.880596, 7.861660, 7.838057, 7.807892, 7.784401, 7.756756},
          1e-4, centred_V);
  printf("%s\n", failures ? "FAILED" : "ALL OK");
  return failures ? 1 : 0;
}
