/**
 * bcd_learner_tests.cc — the reference's BCDLearner tests (tests/cpp/bcd_learner_test.cc:8-73) restated through
 * Learner::Create("bcd") on tests/golden/rcv1_100.libsvm (= the reference's tests/data).
 *
 *   difacto_bcd_tests <data> [data_chunk_size in bytes]
 *
 * Prints one "<case> epoch <k> objv <value>" line per epoch, "<case> chunks <rows> ..." and "<case> ok" / "<case> FAILED";
 * exits 1 on any failure.  The cases run in one process, in the reference's order: the block shuffles draw from one
 * process-wide stream.
 */
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>
#include "./bcd_learner.h"

using namespace difacto;

static int failures = 0;

// runs one learner; returns the last epoch's objective, checks every epoch against objv (when given) within rel
static real_t RunCase(const std::string& name, const std::string& data, const std::string& chunk, KWArgs args,
                      const std::vector<real_t>& objv, double rel, int epochs) {
  std::unique_ptr<Learner> base(Learner::Create("bcd"));
  BCDLearner* learner = static_cast<BCDLearner*>(base.get());
  args.insert(args.begin(), {"data_in", data});
  if (!chunk.empty()) args.push_back({"data_chunk_size", chunk});
  auto remain = learner->Init(args);
  bool ok = remain.empty();   // EXPECT_EQ(remain.size(), 0)
  int seen = 0;
  real_t last = 0;
  double worst = 0;
  learner->AddEpochEndCallback([&](int epoch, const std::vector<real_t>& prog) {
    printf("%s epoch %d objv %.9g\n", name.c_str(), epoch, prog[1]);
    last = prog[1];
    if (!objv.empty()) {
      const double err = std::fabs(prog[1] - objv[epoch]) / prog[1];
      worst = std::max(worst, err);
      if (!(err < rel)) ok = false;
    }
    ++seen;
  });
  learner->Run();
  printf("%s chunks", name.c_str());
  for (size_t r : learner->train_chunk_rows()) printf(" %zu", r);
  printf("\n");
  if (seen != epochs) ok = false;
  if (!objv.empty())
    printf("%s %s (%d epochs, worst relative error %.3g, tolerance %g)\n", name.c_str(), ok ? "ok" : "FAILED", seen, worst, rel);
  fflush(stdout);
  if (!ok) ++failures;
  return last;
}

int main(int argc, char* argv[]) {
  if (argc < 2) {
    fprintf(stderr, "usage: difacto_bcd_tests <data> [data_chunk_size]\n");
    return 2;
  }
  const std::string data = argv[1], chunk = argc > 2 ? argv[2] : "";
  // bcd_learner_test.cc:8-39
  RunCase("DiagNewton", data, chunk,
          {{"l1", ".1"}, {"lr", ".05"}, {"block_ratio", "0.001"}, {"tail_feature_filter", "0"}, {"max_num_epochs", "10"}},
          {34.877064, 33.885559, 29.572740, 27.458964, 25.317689, 23.917098, 22.855843, 22.099876, 21.552682, 21.137216}, 1e-5,
          10);
  // :44-73: the optimal solution with l1 = .1 is objv = 15.884923
  for (const char* r : {".4", "1", "10"}) {
    const std::string name = std::string("Convergence_") + r;
    const real_t objv = RunCase(name, data, chunk,
                                {{"l1", ".1"}, {"lr", ".8"}, {"block_ratio", r}, {"tail_feature_filter", "0"}, {"max_num_epochs", "50"}},
                                {}, 0, 50);
    const double err = std::fabs(objv - 15.884923) / objv;
    const bool ok = err < 1e-3;
    printf("%s %s (final objv %.9g, relative error %.3g, tolerance 1e-3)\n", name.c_str(), ok ? "ok" : "FAILED", objv, err);
    fflush(stdout);
    if (!ok) ++failures;
  }
  printf("%s\n", failures ? "FAILED" : "ALL OK");
  return failures ? 1 : 0;
}
