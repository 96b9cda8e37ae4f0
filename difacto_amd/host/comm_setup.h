/**
 * comm_setup.h — what every multi-GPU learner of this build does before its first exchange: the process environment
 * of one rank (DMLC_ROLE / DMLC_NUM_WORKER / DIFACTO_RANK, the rank's device) and the communicator (DIFACTO_RENDEZVOUS,
 * DIFACTO_COMM=rccl|file: rank 0 writes the RCCL unique id into the rendezvous file, the others read it).  Used by
 * ShardedDeviceStore (learner = sgd) and by the sharded modes of LBFGSLearner and BCDLearner.
 */
#ifndef DIFACTO_HOST_COMM_SETUP_H_
#define DIFACTO_HOST_COMM_SETUP_H_
#include <sys/stat.h>
#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include "./device_context.h"
#include "difacto_hip.h"
#include "dmlc/logging.h"

namespace difacto {

/*! \brief test transport: an all-to-all-v through files in a shared directory */
class FileExchange {
 public:
  FileExchange(const std::string& dir, int rank, int world) : dir_(dir), rank_(rank), world_(world) {}
  static int Call(void* user, const void* send, const size_t* sb, void* recv, const size_t* rb) {
    return static_cast<FileExchange*>(user)->Run(static_cast<const char*>(send), sb, static_cast<char*>(recv), rb);
  }

 private:
  std::string Name(uint64_t seq, int src, int dst) const {
    return dir_ + "/ex" + std::to_string(seq) + "." + std::to_string(src) + "." + std::to_string(dst);
  }
  int Run(const char* send, const size_t* sb, char* recv, const size_t* rb) {
    const uint64_t seq = seq_++;
    size_t off = 0;
    for (int d = 0; d < world_; ++d) {
      const std::string fin = Name(seq, rank_, d), tmp = fin + ".tmp";
      FILE* f = fopen(tmp.c_str(), "wb");
      if (!f) return 1;
      if (sb[d] && fwrite(send + off, 1, sb[d], f) != sb[d]) return 1;
      fclose(f);
      if (rename(tmp.c_str(), fin.c_str()) != 0) return 1;
      off += sb[d];
    }
    off = 0;
    for (int s = 0; s < world_; ++s) {
      const std::string fin = Name(seq, s, rank_);
      FILE* f = nullptr;
      for (int tries = 0; tries < 600000 && !(f = fopen(fin.c_str(), "rb")); ++tries)
        std::this_thread::sleep_for(std::chrono::microseconds(100));
      if (!f) return 1;
      if (rb[s] && fread(recv + off, 1, rb[s], f) != rb[s]) return 1;
      fclose(f);
      unlink(fin.c_str());
      off += rb[s];
    }
    return 0;
  }
  std::string dir_;
  int rank_, world_;
  uint64_t seq_ = 0;
};

/*! \brief one rank's place in a multi-GPU run, read from the environment */
struct RankEnv {
  int rank = 0, world = 1;
};

/*! \brief the environment checks of a rank: only workers run (each owns a key range of the model on its GPU and runs
 * the scheduler loop itself), DIFACTO_RANK is required with more than one rank, and the rank's device defaults to
 * DIFACTO_DEVICE = rank unless the launcher narrowed the visible devices already */
inline RankEnv ReadRankEnv() {
  const char* w = getenv("DMLC_NUM_WORKER");
  const char* r = getenv("DIFACTO_RANK");
  // In the reference's launch a scheduler and servers run beside the workers and park in tracker_->Wait().  Here
  // the workers own the model shards and schedule themselves: any other role joining would race the workers for
  // rank 0.  It is refused, not parked: a launcher that starts one is misconfigured for this build.
  const char* role = getenv("DMLC_ROLE");
  CHECK(!role || std::string(role) == "worker")
      << "DMLC_ROLE=" << role << ": this build runs workers only (each worker owns a key range of the model on its GPU and "
      << "runs the scheduler loop itself); start DMLC_NUM_WORKER worker processes, no scheduler, no servers";
  RankEnv e;
  e.world = w ? atoi(w) : 1;
  CHECK(r || e.world <= 1) << "DMLC_NUM_WORKER=" << e.world << " needs DIFACTO_RANK (0.." << e.world - 1
                           << ") in every worker's environment: without it every process would come up as rank 0";
  e.rank = r ? atoi(r) : 0;
  CHECK(e.world >= 1 && e.world <= 32 && e.rank >= 0 && e.rank < e.world)
      << "DMLC_NUM_WORKER (1..32) / DIFACTO_RANK (0..DMLC_NUM_WORKER-1) are not consistent";
  // one GPU per rank, unless the launcher already narrowed the visible devices to this rank's
  if (!getenv("DIFACTO_DEVICE") && !getenv("HIP_VISIBLE_DEVICES") && !getenv("ROCR_VISIBLE_DEVICES"))
    setenv("DIFACTO_DEVICE", std::to_string(e.rank).c_str(), 0);
  return e;
}

/*! \brief connects the ranks over DIFACTO_COMM = rccl (default) | file through DIFACTO_RENDEZVOUS; *files keeps the file
 * transport alive.  With selfcheck_s > 0 the first exchange is polled (dfh_comm_selfcheck): a missing rank or a wrong
 * rendezvous fails the run after that many seconds instead of hanging it. */
inline dfh_comm* ConnectRanks(int rank, int world, std::unique_ptr<FileExchange>* files, double selfcheck_s = 0) {
  const char* rv = getenv("DIFACTO_RENDEZVOUS");
  const char* kind = getenv("DIFACTO_COMM");
  CHECK(rv || world == 1) << "DIFACTO_RENDEZVOUS must name the rendezvous file (rccl) or directory (file transport)";
  dfh_ctx* ctx = DeviceContext::Get();
  dfh_comm* comm = nullptr;
  if (kind && std::string(kind) == "file") {
    files->reset(new FileExchange(rv ? rv : "/tmp", rank, world));
    DFH_CALL(dfh_comm_create_callback(ctx, rank, world, &FileExchange::Call, files->get(), &comm));
  } else {
    char id[DFH_COMM_ID_BYTES];
    if (rank == 0) {
      DFH_CALL(dfh_comm_unique_id(id));
      if (world > 1) {
        const std::string tmp = std::string(rv) + ".tmp";
        FILE* f = CHECK_NOTNULL(fopen(tmp.c_str(), "wb"));
        CHECK_EQ(fwrite(id, 1, sizeof(id), f), sizeof(id));
        fclose(f);
        CHECK_EQ(rename(tmp.c_str(), rv), 0);
      }
    } else {
      FILE* f = nullptr;
      for (int tries = 0; tries < 120000 && !(f = fopen(rv, "rb")); ++tries)
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
      CHECK(f) << "rank 0 never wrote the rendezvous file " << rv;
      CHECK_EQ(fread(id, 1, sizeof(id), f), sizeof(id));
      fclose(f);
    }
    DFH_CALL(dfh_comm_create_rccl(ctx, rank, world, id, &comm));
  }
  if (selfcheck_s > 0) DFH_CALL(dfh_comm_selfcheck(comm, selfcheck_s));
  return comm;
}

}  // namespace difacto
#endif  // DIFACTO_HOST_COMM_SETUP_H_
