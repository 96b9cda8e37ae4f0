/**
 * model_parts.h — how a learner commits model_out.  One process: the file itself.  A sharded run: one part per rank
 * (<model_out>.part-<rank>) plus a manifest (<model_out>.parts: the number of parts, written by rank 0, which also
 * removes the parts a run with more ranks left behind under the same name).  SGDLearner::LoadModel reads exactly the
 * parts the manifest names, keeping the keys of its own range: a model can be re-loaded under any number of ranks, and
 * stale parts of an earlier save are never imported.  Used by learner = sgd and learner = lbfgs.
 */
#ifndef DIFACTO_HOST_MODEL_PARTS_H_
#define DIFACTO_HOST_MODEL_PARTS_H_
#include <unistd.h>
#include <cstdio>
#include <functional>
#include <string>
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

}  // namespace difacto
#endif  // DIFACTO_HOST_MODEL_PARTS_H_
