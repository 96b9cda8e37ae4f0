// C ABI of libdifacto_hip (include/difacto_hip.h): the root of the library's one translation unit.  It holds no code of its
// own: the files of csrc/ in the order their helpers need one another (every C ABI entry is declared in difacto_hip.h, so
// only the helpers in anonymous namespaces order the list).  DESIGN.md has the same map with a line per file.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>

#include <hip/hip_ext.h>
#include <rocprim/rocprim.hpp>

#include "dfh_kernels.hip"       // the views and kernels of table and step, the update arithmetic (dfh_internal.h: the error macros)
#include "dfh_owner.hip"         // the owner side of the sharded store, four forms: find_or_insert and the update arithmetic
#include "dfh_localize.hip"      // the Localizer's kernels (dfh_feed_layout.h: the staging layout shared with the host side)
#include "dfh_update.hip"        // k_update_fused: the views of dfh_kernels.hip
#include "dfh_riders.hip"        // the rider forms of lookup, forward and update: the kernels of the three files above

using namespace dfh;

#include "dfh_handles.h"         // dfh_ctx, dfh_table, dfh_batch, TimeScope: the views and constants of the kernel files
#include "dfh_pending.hip"       // the single queue's noted Localizer stages: the handles, the Localizer's and riders' kernels
#include "dfh_phases.hip"        // stream phases, split list, launch helpers: flush_pending (dfh_pending.hip)
#include "dfh_ctx.hip"           // context calls and the option table: sync_all (dfh_phases.hip), flush_pending
#include "dfh_table.hip"         // table growth and the table calls: sync_all, the grid and scratch helpers
#include "dfh_store_calls.hip"   // owner-side and literal Store calls: table_reserve, require_aux, refrand_flush, dispatch_L
#include "dfh_loss.hip"          // literal Loss calls: the scratch helpers
#include "dfh_step.hip"          // the step's launches, its two stages, dfh_sgd_step: collect_riders, the phases, the table helpers
#include "dfh_textparse.hip"     // the device text parse, chunks whose ids the feed's uploads take device to device: the handles
#include "dfh_lz4enc.hip"        // the device LZ4 block encoder and the row-block records of task = convert: the parsed chunks
#include "dfh_lz4dec.hip"        // the device LZ4 block decoder, .rec records decoded into chunks like the parsed ones: dfh_textparse.hip
#include "dfh_feed.hip"          // the device feed and the staging helpers of a load: the phases, the parsed chunks
#include "dfh_batch.hip"         // the batch object and its load calls: the feed's staging helpers, to_u32_offsets, auc_flush_pending
#include "dfh_localize_api.hip"  // localize_impl and its calls: the feed's gather, launch_loc_stage, table_reserve
#include "dfh_comm.hip"          // the communicator: the handles, the scratch block
#include "dfh_shard.hip"         // the sharded store's schedules: step_lookup / step_math, the store calls, the communicator
#include "dfh_join.hip"          // a loaded model joined onto a learner's key order: the handles
#include "dfh_chunks.hip"        // the resident chunk set of lbfgs and bcd: batch_create_impl (dfh_batch.hip)
#include "dfh_lbfgs.hip"         // learner = lbfgs: the chunk set, the join, the communicator
#include "dfh_owlqn.hip"         // l1 on w for learner = lbfgs, the orthant-wise forms of its vector passes: dfh_lbfgs.hip
#include "dfh_bcd.hip"           // learner = bcd: the chunk set, the join, the communicator
#include "dfh_eval.hip"          // whole-set evaluation, exact AUC, logloss and accuracy of the appended rows: the handles
#include "dfh_predtext.hip"      // prediction text, the bytes of fprintf("%.9g\n") for the appended values: the handles
#include "dfh_dumptext.hip"      // a model table as sorted text, "<id>\t<w>[\t<V_j>]" per kept entry: the table calls, dfh_predtext_fmt.h
#include "dfh_rowstore.hip"      // a whole data set's rows in HBM and its shuffled blocks: the encoder, the parsed and decoded chunks
