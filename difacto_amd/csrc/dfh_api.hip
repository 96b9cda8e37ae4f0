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

#include "dfh_device.h"          // lane, wave and lane-group helpers, float4 loads and stores (dfh_internal.h: the views, the error macros)
#include "dfh_updater.h"         // the update arithmetic per key, the values InitV writes: dfh_device.h
#include "dfh_index.hip"         // the key index and the table as arrays: hash_init_value (dfh_updater.h)
#include "dfh_auc.hip"           // a minibatch's AUC, by pairs and by sort: dfh_device.h
#include "dfh_lookup.hip"        // the lookup passes and REFRAND: the key index, InitV, auc_finalize_block
#include "dfh_forward.hip"       // k_forward, the progress slots, KeyRange, k_penalty: dfh_device.h
#include "dfh_backward.hip"      // k_backward_all and k_seg_lists: the update arithmetic, the progress slots and KeyRange
#include "dfh_owner.hip"         // the owner side of the sharded store, four forms: find_or_insert and the update arithmetic
#include "dfh_localize.hip"      // the Localizer's kernels, sample sort and library sort, and the key ranges of its output: find_or_insert,
                                 // BWD_* (dfh_feed_layout.h: the staging layout shared with the host side)
#include "dfh_update.hip"        // k_update_fused: the update arithmetic, auc_pairs_block, KeyRange, BWD_*
#include "dfh_riders.hip"        // the rider forms of lookup, forward and update: lookup_body, forward_body, the two files above

using namespace dfh;

#include "dfh_handles.h"         // dfh_ctx, dfh_table, dfh_batch, TimeScope: the views and constants of the kernel files
#include "dfh_pending.hip"       // the single queue's noted Localizer stages: the handles, the Localizer's and riders' kernels
#include "dfh_phases.hip"        // stream phases, split list, launch helpers: flush_pending (dfh_pending.hip)
#include "dfh_ctx.hip"           // context calls and the option table: sync_all (dfh_phases.hip), flush_pending
#include "dfh_table.hip"         // table growth and the table calls: sync_all, the grid and scratch helpers
#include "dfh_store_calls.hip"   // owner-side and literal Store calls: table_reserve, require_aux, refrand_flush, dispatch_L
#include "dfh_loss.hip"          // literal Loss calls and their kernels: the scratch helpers
#include "dfh_auc_api.hip"       // the AUC's launches, either form, and dfh_auc_times_n: the handles, the scratch helpers
#include "dfh_step.hip"          // the step's launches, its two stages, dfh_sgd_step: collect_riders, the phases, the table helpers, launch_auc
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
#include "dfh_textout.hip"       // what the device formatters share, workspace, two-pass driver, download, the kernels' common parts, and dev_grow: the handles
#include "dfh_eval_groups.hip"   // the same rows by group, per-group records and the grouped AUC: the evaluator, the batch's step, dev_grow
#include "dfh_predtext.hip"      // prediction text, the bytes of fprintf("%.9g\n") for the appended values: dfh_textout.hip
#include "dfh_dumptext.hip"      // a model table as sorted text, "<id>\t<w>[\t<V_j>]" per kept entry: the table calls, dfh_textout.hip, dfh_predtext_fmt.h
#include "dfh_pairs.hip"         // each entry's top-k FM interaction partners, a blocked V V^T on MFMA that is never stored: the dump's entries, dev_grow
#include "dfh_explain.hip"       // each row's top-k FM interaction pairs, a wave per row and a 32 x 32 Gram tile per panel pair on MFMA: the batch's step, pr_* (dfh_pairs.hip), TextWork
#include "dfh_recommend.hip"     // each row's top-k catalogue items, a rectangular S_q S_i^T + b_i on MFMA that is never stored: the batch's step, pr_* (dfh_pairs.hip), TextWork
#include "dfh_listtext.hip"      // the lines of explain_out and recommend_out formatted on the device, ragged lines of lists: the two objects above, dfh_textout.hip
#include "dfh_rowstore.hip"      // a whole data set's rows in HBM and its shuffled blocks: the encoder, the parsed and decoded chunks
