/**
 * sgd_loop_env.h — the environment switches of the SGD worker loops (sgd_learner.cc) and of the device feed (device_feed.h),
 * read in ONE place: a loop fills an SgdLoopEnv at the start of a job and nothing below it calls getenv for these names.
 */
#ifndef DIFACTO_HOST_SGD_LOOP_ENV_H_
#define DIFACTO_HOST_SGD_LOOP_ENV_H_
#include <algorithm>
#include <cstdlib>
#include "./device_context.h"

namespace difacto {

struct SgdLoopEnv {
  int prep_streams = 0;            // DIFACTO_PREP_STREAMS=1..4 (0: not set — two with the device feed, else one)
  bool single_queue = false;       // DIFACTO_SINGLE_QUEUE=1: the single-queue step, minibatches prepared two ahead
  bool prep_priority_set = false;  // DIFACTO_PREP_PRIORITY=-1|0|1
  int prep_priority = 0;
  bool host_feed = false;          // DIFACTO_HOST_FEED: training with a shuffle buffer keeps the host-side gather
  bool split_prep = false;         // DIFACTO_SPLIT_PREP: gather, Localizer and lookup as three calls (A/B)
  bool profile = false;            // DIFACTO_PROFILE: where the loop's host thread spends its time, logged per job
  bool trace = false;              // DIFACTO_TRACE: one line per minibatch / per sharded step
  bool feed_precreate = true;      // DIFACTO_FEED_PRECREATE=0: row buffers and batch objects on first use
  int upload_threads = 2;          // DIFACTO_UPLOAD_THREADS=1..8
  bool parser_threads_set = false; // DIFACTO_PARSER_THREADS (the reader reads its value): the loop chooses no count of its own

  SgdLoopEnv() {
    if (const char* e = getenv("DIFACTO_PREP_STREAMS")) prep_streams = std::max(1, std::min(atoi(e), 4));
    if (const char* e = getenv("DIFACTO_SINGLE_QUEUE")) single_queue = atoi(e) != 0;
    if (const char* e = getenv("DIFACTO_PREP_PRIORITY")) prep_priority_set = true, prep_priority = atoi(e);
    host_feed = getenv("DIFACTO_HOST_FEED") != nullptr;
    split_prep = getenv("DIFACTO_SPLIT_PREP") != nullptr;
    profile = getenv("DIFACTO_PROFILE") != nullptr;
    trace = getenv("DIFACTO_TRACE") != nullptr;
    if (const char* e = getenv("DIFACTO_FEED_PRECREATE")) feed_precreate = atoi(e) != 0;
    if (const char* e = getenv("DIFACTO_UPLOAD_THREADS")) upload_threads = std::max(1, std::min(atoi(e), 8));
    parser_threads_set = getenv("DIFACTO_PARSER_THREADS") != nullptr;
  }
  /*! \brief the preparation streams' priority, decided by the first job of the PROCESS (not per learner: the streams are
   *  created once per context): DIFACTO_PREP_PRIORITY, else the default priority if that job reads through the device feed —
   *  its preparation chain is as long as the step and sets the pace at bench.py's lowest (profiles/r06e2e_prep_priority.txt) */
  void SetPrepPriorityOnce(dfh_ctx* ctx, bool device_feed) const {
    static bool decided = false;
    if (!decided && (prep_priority_set || device_feed)) DFH_CALL(dfh_ctx_set_option(ctx, "prep_priority", prep_priority));
    decided = true;
  }
};

}  // namespace difacto
#endif  // DIFACTO_HOST_SGD_LOOP_ENV_H_
