/**
 * sgd_cache_tests.cc — data_cache = hbm of the SGD learner through Learner::Create("sgd") on tests/golden/rcv1_100.libsvm.
 *
 *   difacto_sgd_cache_tests <data>
 *
 * Every case trains twice, three epochs: once uncached over <data>, once with data_cache=hbm over a temporary COPY of it
 * that an epoch-end callback unlinks after epoch 0.  Epochs 1 and 2 of the cached run must complete — they have no file to
 * read — and every epoch's training loss (and validation loss, where the case has one) must equal the uncached run's bit
 * for bit.  Prints "<case> <run> epoch <k> loss <value> ..." per epoch and "<case> ok" / "<case> FAILED"; exits 1 on any
 * failure.  The shuffle buffers' permutations come from one process-wide stream, which every run restarts.
 */
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "./sgd_learner.h"

using namespace difacto;

static int failures = 0;

struct Epoch {
  real_t loss, val_loss, auc, nrows;
};

static std::vector<Epoch> Run(const std::string& name, const char* run, const std::string& data, bool with_val, KWArgs args,
                              bool unlink_after_first) {
  RefRand::Global()->Seed(1);
  std::unique_ptr<Learner> base(Learner::Create("sgd"));
  SGDLearner* learner = static_cast<SGDLearner*>(base.get());
  args.insert(args.begin(), {"data_in", data});
  if (with_val) args.push_back({"data_val", data});
  auto remain = learner->Init(args);
  if (!remain.empty()) {
    printf("%s %s: unrecognised key %s\n", name.c_str(), run, remain[0].first.c_str());
    ++failures;
  }
  std::vector<Epoch> out;
  learner->AddEpochEndCallback([&](int epoch, const sgd::Progress& train, const sgd::Progress& val) {
    printf("%s %s epoch %d loss %.9g val_loss %.9g auc %.9g rows %g\n", name.c_str(), run, epoch, train.loss, val.loss, train.auc,
           train.nrows);
    out.push_back(Epoch{train.loss, val.loss, train.auc, train.nrows});
    if (unlink_after_first && epoch == 0) {
      if (unlink(data.c_str()) != 0) {
        printf("%s: cannot unlink %s\n", name.c_str(), data.c_str());
        ++failures;
      }
    }
  });
  learner->Run();
  fflush(stdout);
  return out;
}

static std::string CopyOf(const std::string& data) {
  char path[] = "/tmp/difacto_sgd_cache_XXXXXX";
  const int fd = mkstemp(path);
  CHECK(fd >= 0) << "cannot create a temporary file";
  FILE* in = fopen(data.c_str(), "rb");
  CHECK(in) << "cannot open " << data;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), in)) > 0) CHECK_EQ(write(fd, buf, n), static_cast<ssize_t>(n));
  fclose(in);
  close(fd);
  return path;
}

static void Case(const std::string& name, const std::string& data, bool with_val, const KWArgs& extra) {
  const int epochs = 3;
  KWArgs args = {{"batch_size", "25"}, {"num_jobs_per_epoch", "2"}, {"V_dim", "4"}, {"V_threshold", "2"}, {"l1", ".1"}, {"lr", ".1"},
                 {"max_num_epochs", std::to_string(epochs)}, {"stop_rel_objv", "0"}, {"stop_val_auc", "-1e30"}};
  args.insert(args.end(), extra.begin(), extra.end());
  const std::vector<Epoch> plain = Run(name, "uncached", data, with_val, args, false);
  const std::string copy = CopyOf(data);
  KWArgs cargs = args;
  cargs.push_back({"data_cache", "hbm"});
  // (with_val: data_val is the same copy; the callback follows epoch 0's validation jobs)
  const std::vector<Epoch> cached = Run(name, "cached", copy, with_val, cargs, true);
  bool ok = plain.size() == static_cast<size_t>(epochs) && cached.size() == plain.size();
  for (size_t k = 0; ok && k < plain.size(); ++k)
    ok = memcmp(&plain[k].loss, &cached[k].loss, sizeof(real_t)) == 0 && memcmp(&plain[k].val_loss, &cached[k].val_loss, sizeof(real_t)) == 0 &&
         memcmp(&plain[k].auc, &cached[k].auc, sizeof(real_t)) == 0 && plain[k].nrows == cached[k].nrows && plain[k].nrows > 0;
  printf("%s %s (%zu uncached, %zu cached epochs)\n", name.c_str(), ok ? "ok" : "FAILED", plain.size(), cached.size());
  fflush(stdout);
  if (!ok) ++failures;
}

int main(int argc, char* argv[]) {
  if (argc < 2) {
    fprintf(stderr, "usage: difacto_sgd_cache_tests <data>\n");
    return 2;
  }
  const std::string data = argv[1];
  Case("Shuffled", data, false, {{"shuffle", "2"}});
  Case("Sampled", data, false, {{"shuffle", "2"}, {"neg_sampling", "0.5"}});
  Case("InOrder", data, false, {{"shuffle", "0"}});
  Case("Validated", data, true, {{"shuffle", "2"}});
  printf("%s\n", failures ? "FAILED" : "ALL OK");
  return failures ? 1 : 0;
}
