/*
 * difacto_hip.h — the C ABI of the MI355X-native FM/SGD worker path.
 *
 * This is the drop-in boundary: plain C, opaque handles, caller-owned buffers,
 * int return codes (0 = ok; message via dfh_last_error()).  Each entry point
 * names the reference interface (dmlc/difacto, file:line) it replaces, so the
 * C++ adaptors in difacto_amd/host/ (HipFMLoss : Loss, DeviceStore : Store) and
 * any other FFI (ctypes in difacto_amd/capi.py) bind 1:1.
 *
 * Conventions
 *   - "keys" are the byte-reversed feature ids the reference's Localizer emits
 *     (ReverseBytes(id % max_index), src/data/localizer.cc:24); ~0ULL is reserved.
 *   - host-pointer calls ("literal" API) are synchronous: on return the outputs
 *     are valid and the model state is updated.
 *   - device-pointer calls are asynchronous on the context's HIP stream; use
 *     dfh_ctx_sync() or stream-ordered work of your own.
 *   - there is NO CPU fallback: every compute entry point runs HIP kernels on
 *     the context's device and fails with DFH_ERR_HIP if that is impossible.
 */
#ifndef DIFACTO_HIP_H_
#define DIFACTO_HIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DFH_OK = 0,
  DFH_ERR_ARG = 1,      /* bad argument / reference CHECK would fail */
  DFH_ERR_HIP = 2,      /* HIP runtime error */
  DFH_ERR_CAPACITY = 3, /* model table is full */
  DFH_ERR_STATE = 4     /* call sequence error (e.g. step before localize) */
};

/* Store value types — include/difacto/store.h:31-33 */
enum { DFH_FEA_COUNT = 1, DFH_WEIGHT = 2, DFH_GRADIENT = 3 };

/* how a lazily allocated embedding row is initialised */
enum {
  DFH_INIT_REFRAND = 0, /* bit-compatible with SGDUpdater::InitV's glibc rand_r chain
                           (src/sgd/sgd_updater.cc:140-147); serial in key order */
  DFH_INIT_HASH = 1     /* counter-based hash of (key, j, seed): order/sharding independent */
};

/* SGDUpdaterParam — src/sgd/sgd_param.h:66-107: same names, meanings, defaults */
typedef struct {
  float l1, l2, V_l2;
  float lr, lr_beta, V_lr, V_lr_beta;
  float V_init_scale;
  int V_dim;
  int V_threshold;
  unsigned seed;
  int init_mode; /* DFH_INIT_* */
} dfh_updater_param;

/* sgd::Progress — src/sgd/sgd_utils.h:40-75 */
typedef struct {
  float loss, penalty, auc, nnz_w, nrows;
} dfh_progress;

typedef struct dfh_ctx dfh_ctx;     /* a device + a HIP stream */
typedef struct dfh_table dfh_table; /* one shard of the model: replaces Store+Updater state */
typedef struct dfh_batch dfh_batch; /* a device-resident minibatch + its workspace */

const char* dfh_last_error(void);
void dfh_updater_param_default(dfh_updater_param* p, int V_dim);

/* ---------------------------------------------------------------- context */
/* stream: an existing hipStream_t (e.g. torch's current stream) or NULL to create one */
int dfh_ctx_create(int device, void* stream, dfh_ctx** out);
int dfh_ctx_destroy(dfh_ctx* ctx);
int dfh_ctx_sync(dfh_ctx* ctx);
void* dfh_ctx_stream(dfh_ctx* ctx);
int dfh_ctx_device(dfh_ctx* ctx);

/* Pipelining: with enable = n in 1..4 batch preparation (dfh_batch_load_*, dfh_localize,
 * dfh_batch_lookup) runs on n preparation streams of the lowest priority, taken round-robin, so
 * batches t+1 .. t+n are prepared while batch t trains — the overlap the reference gets from its
 * reader thread (src/sgd/sgd_learner.cc:196-224); steps are still applied strictly in batch order.
 * Ordering per batch object is kept with events inside the library; use n + 1 (better n + 2)
 * dfh_batch objects in rotation.  0 = everything on the context's stream. */
int dfh_ctx_set_pipeline(dfh_ctx* ctx, int enable);
/* launch tuning, validated (unknown names / out-of-range values: DFH_ERR_ARG):
 *   "fwd_depth"         4 | 5 | 8 | 10  independent V-row loads per forward lane (default 5)
 *   "fwd_blocks"        0 .. 16384      cap on the forward grid, 0 = one wave per example (default)
 *   "bwd_small_blocks"  1 .. 65536      cap on the short-segment blocks of the backward launch (default 2048)
 *   "prep_priority"     -1 | 0 | 1      stream priority of the preparation streams: lowest (default),
 *                                       normal, highest; before dfh_ctx_set_pipeline creates them
 *   "upd_kernel", "upd_*_blocks", "upd_interleave", "event_flags": see csrc/dfh_ctx.hip (measurement switches)
 *   "grow_initial_rows" 16 .. 2^28      first allocation of a growing table (dfh_table_create, capacity_rows = 0; default 2^20)
 *   "auc_in_update"     0 | 1           BinClassMetric::AUC of a training step (batch option "compute_auc") as the first
 *                                       blocks of the update launch (default 1) or as a launch of its own
 *   "single_queue"      0 | 1           1: no preparation stream — dfh_localize only notes the Localizer's four stages, which then
 *                                       ride as extra blocks of the launches later dfh_sgd_step calls make (the two minibatches the
 *                                       reference keeps in flight, src/sgd/sgd_learner.cc:196-224, on ONE hardware queue; prepare
 *                                       two ahead).  Same results bit for bit; pays for small minibatches only (default 0)
 *   "rider_slot_count / _scatter / _sort / _emit"  0 lookup | 1 forward | 2 update (+ 4: as a launch of its own before it):
 *                                       which launch of a step carries the stage;  "rider_period_lookup / _forward / _update"
 *                                       1 .. 4096 and "rider_start_*" 0 .. 100: where the rider blocks sit in the carrier's grid
 *   "upd_split"         0 | 1           keys with more than 4 096 occurrences in a minibatch go through the update kernel in
 *                                       parts of 1 024, a block per part (default 1; 0 = one block walks the whole segment)
 *   "owner_per_key"     0 | 1           dfh_shard_step's owner side per distinct key (dfh_shard_count_pull_multi +
 *                                       dfh_shard_push_grad_listed) instead of per received entry; same results, not faster
 *                                       (default 0; measurement switch) */
int dfh_ctx_set_option(dfh_ctx* ctx, const char* name, int value);

/* optional per-kernel timing with HIP events recorded on the context's stream
 * (what bench.py's roofline block reads); ids index total_ms[]/calls[] */
enum {
  DFH_K_LOCALIZE = 0, DFH_K_LOOKUP, DFH_K_FORWARD, DFH_K_BACKWARD, DFH_K_PULL, DFH_K_PUSH, DFH_K_MISC, DFH_K_AUC, DFH_K_COUNT
};
int dfh_ctx_set_timing(dfh_ctx* ctx, int enable);
/* time only the kernels whose bit (1u << DFH_K_*) is set.  Single-launch kernels (forward,
 * backward) carry their event pair on the dispatch itself (hipExtLaunchKernelGGL: the kernel's own
 * begin/end, as a profiler reports it); multi-launch groups (Localizer, lookup) are bracketed by
 * recorded events, each of which drains the stream (~10 us on MI355X) — so production loops
 * leave timing off and a benchmark samples: one kernel, every n-th step */
int dfh_ctx_set_timing_mask(dfh_ctx* ctx, uint32_t mask);
int dfh_ctx_get_timing(dfh_ctx* ctx, int reset, double* total_ms, uint64_t* calls); /* synchronises */
const char* dfh_kernel_name(int id);

/* ------------------------------------------------------- id transforms (a1) */
/* ReverseBytes / EncodeFeaGrpID — include/difacto/base.h:39-51,60-63 (host helpers) */
uint64_t dfh_reverse_bytes(uint64_t x);
uint64_t dfh_encode_fea_grp_id(uint64_t x, int gid, int nbits);

/* ------------------------------------------------------------ model table */
/* Replaces SGDUpdater's unordered_map<feaid_t,SGDEntry> (src/sgd/sgd_updater.h:78)
 * with a row store in HBM: capacity_rows fixed-stride rows + an open-addressing
 * key index.  Unseen keys are inserted as zero rows on first touch, exactly as
 * SGDUpdater::Get/Update do through model_[id] (sgd_updater.cc:44,66,87).
 * capacity_rows = 0: the table GROWS like the reference's map (it starts at 2^20 rows and is re-allocated at twice
 * the size whenever fewer than 32 launches' worth of new keys would still fit; row ids are stable, only the key index
 * is rebuilt; needs old + new arrays side by side, so a model beyond a third of the HBM wants an explicit capacity).
 * capacity_rows > 0: fixed; inserting beyond it is reported as DFH_ERR_CAPACITY, never silent.  At most 2^28 - 1 rows (the four top bits of a row word carry flags). */
int dfh_table_create(dfh_ctx* ctx, const dfh_updater_param* p, uint64_t capacity_rows, dfh_table** out);
/* rows the arrays hold now, and how often the table has grown (0 for a fixed capacity) */
int dfh_table_capacity(dfh_table* t, uint64_t* capacity_rows, uint64_t* grows);
int dfh_table_destroy(dfh_table* t);
int dfh_table_size(dfh_table* t, uint64_t* nkeys); /* synchronises */
int dfh_table_param(dfh_table* t, dfh_updater_param* out);
uint64_t dfh_table_bytes(dfh_table* t);
/* SGDUpdater::has_aux_ (src/sgd/sgd_updater.h:80): cleared by dfh_table_load of a file saved
 * without optimiser state (or by a host that parsed such a file itself); while cleared, every
 * gradient push and training step fails with DFH_ERR_STATE — the reference's
 * CHECK(has_aux_) << "no aux data" (src/sgd/sgd_updater.cc:75) */
int dfh_table_set_has_aux(dfh_table* t, int has_aux);
int dfh_table_has_aux(dfh_table* t);

/* Store::Pull(fea_ids, kWeight, vals, lens) -> SGDUpdater::Get
 * (include/difacto/store.h:69-73, src/store/store_local.h:36-44, src/sgd/sgd_updater.cc:32-56).
 * Host pointers.  vals capacity n*(1+V_dim), lens capacity n; ragged layout and
 * lens in {1, 1+V_dim}; *nlens == 0 iff V_dim == 0 — as the reference. */
int dfh_pull(dfh_table* t, const uint64_t* keys, size_t n, float* vals, size_t* nvals, int* lens, size_t* nlens);

/* Store::Push(fea_ids, kFeaCount|kGradient, vals, lens) -> SGDUpdater::Update
 * (include/difacto/store.h:53-57, src/store/store_local.h:24-34, src/sgd/sgd_updater.cc:58-148):
 * FTRL on w, AdaGrad on V, lazy InitV.  Host pointers.  Keys must be unique (checked: DFH_ERR_ARG). */
int dfh_push(dfh_table* t, const uint64_t* keys, size_t n, int val_type, const float* vals, size_t nvals,
             const int* lens, size_t nlens);

/* model I/O helpers (Updater::Save/Load are TODO in the reference, src/sgd/sgd_updater.h:44-50):
 * dump every entry: keys[n], scal[n*4] = {fea_cnt,w,sqrt_g,z}, has_V[n], V[n*2*V_dim] */
int dfh_table_export(dfh_table* t, uint64_t cap, uint64_t* keys, float* scal, int* has_V, float* V, uint64_t* n);
int dfh_table_import(dfh_table* t, uint64_t n, const uint64_t* keys, const float* scal, const int* has_V, const float* V);
/* Updater::Save / Load to a file (include/difacto/updater.h:40-47; TODO stubs in the reference,
 * src/sgd/sgd_updater.h:44-50, so the format is ours — the one the C++ host's --model_out / --model_in
 * read and write).  save_aux: also keep fea_cnt, the FTRL state and the AdaGrad accumulators, i.e.
 * everything needed to continue training; without it, entries with w == 0 and no V are dropped.
 * dfh_table_load imports only keys in [key_lo, key_hi) (key_hi == 0: no upper bound): a shard
 * loads its own range out of any number of part files, whatever sharding wrote them.
 * Host-side I/O; both synchronise. */
int dfh_table_save(dfh_table* t, const char* path, int save_aux, uint64_t* n_saved);
int dfh_table_load(dfh_table* t, const char* path, uint64_t key_lo, uint64_t key_hi, int* has_aux, uint64_t* n_loaded);

/* warm start (resume / benchmark preload): insert n unique keys (DEVICE pointer)
 * with w = w0, fea_cnt = cnt0 and an allocated V (hash init).  Asynchronous. */
int dfh_table_warm_start(dfh_table* t, const uint64_t* d_keys, size_t n, float w0, float cnt0);

/* ------------------------------------------------ literal Loss API (a6-a8) */
/* FMLoss::Predict (src/loss/fm_loss.h:67-119).  Host pointers; pred is
 * accumulated into (caller zeroes it, src/sgd/sgd_learner.cc:142).  w_pos/V_pos
 * NULL => dense weights, no V (the V_dim==0 / LogitLoss case). */
int dfh_fm_predict(dfh_ctx* ctx, int V_dim, size_t nrows, const size_t* offset, const uint32_t* index,
                   const float* value, const float* weights, size_t nweights, const int* w_pos,
                   const int* V_pos, size_t npos, float* pred);

/* FMLoss::CalcGrad (src/loss/fm_loss.h:148-199).  Host pointers; grad (shape of
 * weights) is accumulated into.  Stateless: recomputes X*V instead of relying
 * on the preceding Predict's members. */
int dfh_fm_calcgrad(dfh_ctx* ctx, int V_dim, size_t nrows, const size_t* offset, const uint32_t* index,
                    const float* value, const float* label, const float* weights, size_t nweights,
                    const int* w_pos, const int* V_pos, size_t npos, const float* pred, float* grad);

/* Loss::Evaluate (include/difacto/loss.h:57-66): sum_i log(1+exp(-y_i pred_i)) */
int dfh_loss_evaluate(dfh_ctx* ctx, const float* label, const float* pred, size_t n, float* objv);

/* BinClassMetric::AUC (src/loss/bin_class_metric.h:35-56): returns AUC * n */
int dfh_auc_times_n(dfh_ctx* ctx, const float* label, const float* pred, size_t n, float* auc_n);

/* ------------------------------------------------- device-resident batches */
int dfh_batch_create(dfh_ctx* ctx, size_t max_rows, size_t max_nnz, dfh_batch** out);
/* n batch objects of one size out of ONE device allocation (freed with the last of them): what a worker loop that rotates a
 * dozen objects creates at the start of a job — one allocation instead of n (a job's start-up) */
int dfh_batch_create_many(dfh_ctx* ctx, int n, size_t max_rows, size_t max_nnz, dfh_batch** out);
int dfh_batch_destroy(dfh_batch* b);

/* raw minibatch = what Reader::Value() hands the worker (dmlc::RowBlock<feaid_t>,
 * src/reader/reader.h:49-51): CSR with u64 feature ids.  value may be NULL (binary).  The arrays
 * are staged in page-locked memory of the batch object and copied asynchronously: on return the
 * caller may reuse them, and nothing has waited for the device. */
int dfh_batch_load_host(dfh_batch* b, size_t nrows, const size_t* offset, const uint64_t* index,
                        const float* value, const float* label);
/* same, from DEVICE pointers (u32 offsets); copies into the batch's own buffers */
int dfh_batch_load_device(dfh_batch* b, size_t nrows, size_t nnz, const uint32_t* d_offset,
                          const uint64_t* d_index, const float* d_value, const float* d_label);

/* same, WITHOUT a copy: the batch reads the caller's device arrays in place; they must stay
 * valid and unchanged until the work queued on this batch has finished */
int dfh_batch_attach_device(dfh_batch* b, size_t nrows, size_t nnz, const uint32_t* d_offset,
                            const uint64_t* d_index, const float* d_value, const float* d_label);

/* Localizer::Compact on device (src/data/localizer.h:41-51, localizer.cc:11-103):
 * keys = ReverseBytes(id % max_index), sorted unique keys + counts + compact
 * index per nnz — bit-exact with the reference — plus the key-ordered view the
 * backward pass's segmented sum walks. */
int dfh_localize(dfh_batch* b, uint64_t max_index);
/* dfh_localize is a pure function of the minibatch, but a batch object remembers the exact quantiles
 * of the last minibatch it localized and partitions the next one with them (consecutive minibatches
 * of one stream share their key distribution); they affect speed only, never the result.
 * tuning / test switches: "force_radix_sort" = 1 makes dfh_localize take its
 * large-batch path (library LSD radix sort) whatever the batch size;
 * "force_sort_fallback" = 1 sorts every bucket through the oversize-bucket path;
 * "reset_splitters" = 1 forgets the stored quantiles (the next call samples again);
 * "compute_auc" = 1 makes dfh_sgd_step accumulate BinClassMetric::AUC (x nrows) of every
 * batch into dfh_progress.auc, as src/sgd/sgd_learner.cc:153-155 does */
int dfh_batch_set_option(dfh_batch* b, const char* name, int value);

/* resolve the batch's unique keys to table rows ahead of dfh_sgd_step (inserting
 * unseen keys as zero rows, src/sgd/sgd_updater.cc:44): the random probes of the key index run
 * with the preparation work, and the step's own pass over the keys (count push, current w) finds
 * the rows known.  Optional: dfh_sgd_step probes itself when this was not called. */
int dfh_batch_lookup(dfh_table* t, dfh_batch* b);
/* dfh_localize and dfh_batch_lookup in one call: the Localizer's last pass (the thread that writes a unique key has it
 * in hand) probes the key index itself — one launch and one cross-stream event fewer per minibatch
 * (src/data/localizer.cc:11-103 followed by src/sgd/sgd_updater.cc:32-56's model_[id] lookups).  Same results as the two
 * calls; on MI355X at the C3 size the two calls are 0.4 % faster per step (the longer last pass runs beside the forward
 * kernel), so the worker loops use those. */
int dfh_localize_lookup(dfh_table* t, dfh_batch* b, uint64_t max_index);

/* Device feed.  BatchReader's shuffle buffer (src/reader/batch_reader.cc:38-52: batch_size x shuffle rows, permuted, cut into
 * minibatches) held in HBM: the host uploads every buffer once (dfh_rowbuf_load_host, callable from a reader thread: it uses a
 * stream of its own and returns when the caller's arrays are free) and a minibatch is gathered out of at most a few buffers
 * by row number on the device (dfh_batch_gather_rows, in place of dfh_batch_load_host): `offset` [nrows + 1] and `label`
 * [nrows] are the minibatch's own (the host knows the row lengths), segment g takes rows[g][0 .. seg_rows[g]) of bufs[g], in
 * order.  A buffer without values counts as all ones.  The same minibatch as the host-side gather, byte for byte.  The gather
 * kernel reads the description in place, in the batch object's page-locked staging block, as dfh_batch_prepare_rows' does. */
typedef struct dfh_rowbuf dfh_rowbuf;
int dfh_rowbuf_create(dfh_ctx* c, size_t max_rows, size_t max_nnz, dfh_rowbuf** out);
int dfh_rowbuf_destroy(dfh_rowbuf* rb);
int dfh_rowbuf_load_host(dfh_rowbuf* rb, size_t nrows, const size_t* offset, const uint64_t* index, const float* value);
/* the same for a buffer whose ids / values were never assembled on the host: `offset` [nrows + 1] are the buffer's own,
 * slice g brings nnz[g] ids (and values, or NULL = all ones) that follow those of slice g - 1 — one copy per slice, straight
 * out of the parser's chunks (round 4: assembling 31 MB per buffer on one host thread was what the worker loop waited for) */
int dfh_rowbuf_load_host_slices(dfh_rowbuf* rb, size_t nrows, const size_t* offset, int nslices, const uint64_t* const* index,
                                const float* const* value, const size_t* nnz);
/* Device text parse (the SGD learner's text_parse = device).  A dfh_textchunk is one parsed chunk of criteo text: the text and
 * its delimiter positions in HBM, the ids in HBM, the rows' offsets and labels on the host.  dfh_textchunk_parse_criteo uploads
 * `len` bytes of `text` (data_format = criteo: is_train = 1, criteo_test: 0), parses them on the device and returns when the
 * host-side results are there.  *regular = 1: the chunk is made of regular rows only (it is non-empty, ends with '\n' and holds
 * no '\r'; no empty line; every line has 39 / 38 tabs; the label is one character '0'..'9'; an integer field has 0 .. 16 bytes;
 * a categorical field 0 bytes, or 8 that do not start with ' ', '\v' or '\f') and *nrows, *nnz, the offsets, labels and ids are
 * CriteoParser::ParseNext's (src/reader/criteo_parser.h:40-94), bit for bit.  *regular = 0 is not an error: nothing else is
 * valid and the caller parses the chunk on the host.  The object's arrays grow to what a chunk needs (max_bytes: the text
 * buffer's first size; a chunk has fewer than 2^31 bytes); all chunks of a context share one stream, a call waits for its
 * own work only, and calls on different objects may run on different threads.  dfh_textchunk_rows: the host copies
 * (offset [nrows + 1], label [nrows]); dfh_textchunk_ids: the ids [nnz] copied back (tests). */
typedef struct dfh_textchunk dfh_textchunk;
int dfh_textchunk_create(dfh_ctx* ctx, size_t max_bytes, dfh_textchunk** out);
int dfh_textchunk_destroy(dfh_textchunk* tc);
int dfh_textchunk_parse_criteo(dfh_textchunk* tc, const char* text, size_t len, int is_train, int* regular, size_t* nrows, size_t* nnz);
int dfh_textchunk_rows(dfh_textchunk* tc, uint32_t* offset, float* label);
int dfh_textchunk_ids(dfh_textchunk* tc, uint64_t* index);
/* rec_decode = device (csrc/dfh_lz4dec.hip).  dfh_lz4_decompress is the counterpart of dfh_lz4_compress: the ONE LZ4 block of `n`
 * bytes at `src` (host; they are uploaded) is decoded on the device.  *ok = 1 and dst[0 .. expect) is filled exactly when the host
 * decoder (host/lz4_block.h: Lz4DecompressBlock(src, n, dst, expect)) returns `expect`; otherwise *ok = 0, the call returns DFH_OK
 * and nothing is written to dst.  n = 0 is ok only with expect = 0; n or expect >= 2^31 - 2^25 is refused (DFH_ERR_ARG).
 * The call is a test and tool entry, not a hot path: it creates its device arrays and frees them again on every call (the
 * arrays that grow and are reused belong to a dfh_textchunk: dfh_textchunk_decode_crb).
 * dfh_textchunk_decode_crb: one CompressedRowBlock record (the payload of a RecordIO record of a .rec file) becomes a chunk in
 * the state dfh_textchunk_parse_criteo leaves a regular chunk in: ids in HBM, u32 offsets from 0 and labels on the host
 * (dfh_textchunk_rows / _ids).  *regular = 1 only if the header is the one DecompressRowBlock accepts (host/batch_reader.h),
 * nrows >= 1, the offset array is present, does not decrease and spans fewer than 2^31 nonzeros, the index array is present and
 * inflates to exactly 8 nnz bytes, the label array is absent (labels are 0) or inflates to 4 nrows bytes, VALUE AND WEIGHT ARE
 * ABSENT, and every present block is a valid LZ4 block.  *regular = 0 is not an error: nothing else is valid and the caller
 * inflates the record on the host.  The host waits twice per record: for the blocks' sizes, and for the rows' 8 bytes each. */
int dfh_lz4_decompress(dfh_ctx* c, const void* src, size_t n, void* dst, size_t expect, int* ok);
int dfh_textchunk_decode_crb(dfh_textchunk* tc, const void* record, size_t len, int* regular, size_t* nrows, size_t* nnz);
/* task = convert: .rec records written on the device (csrc/dfh_lz4enc.hip).  dfh_lz4_compress: `n` bytes at `src` (host; they are
 * uploaded) -> ONE LZ4 block at `dst` that a conforming decoder (LZ4_decompress_safe, host/lz4_block.h) inflates to exactly those
 * bytes: the last sequence is literals only, the last 5 bytes are literals, no match starts within the last 12 bytes, offsets are
 * 1 .. 65535; *out_bytes <= n + n / 255 + 16 (DFH_ERR_ARG when cap is smaller than the block).  The bytes are not liblz4's; the
 * same input gives the same bytes on every run.  n >= 2^31 - 2^25 is refused (DFH_ERR_ARG).
 * A dfh_crb is an encoder with its device arrays and a stream of its own; the arrays grow to what a block needs.
 * dfh_crb_encode_host: CompressedRowBlock::Compress (src/data/compressed_row_block.h:23-49) of host arrays: label [nrows],
 * offset [nrows + 1] (written as given), index / value [offset[nrows] - offset[0]] = the block's own nonzeros (index[0] is the
 * first id of row 0), weight [nrows]; index, value and weight may be NULL (index only without nonzeros).  The record is int32
 * magic 1196140743, int32 8, int32 nrows, then per array label, offset, index, value, weight: int32 size of the LZ4 block and
 * the block; an absent array, an array of zero elements and values that are all exactly 1 are written as int32 0.
 * dfh_crb_encode_textchunk: the same for a regular parsed chunk of criteo text — the ids are taken where they are in HBM, the
 * offsets widened to 64 bits on the device, no values — byte for byte the record dfh_crb_encode_host gives for the chunk's rows.
 * An encode call returns when the caller's arrays (the text chunk) may be reused and *record_bytes is known; dfh_crb_record
 * copies the record of the last encode to dst [record_bytes].  Calls on different objects may run on different threads. */
int dfh_lz4_compress(dfh_ctx* c, const void* src, size_t n, void* dst, size_t cap, size_t* out_bytes);
typedef struct dfh_crb dfh_crb;
int dfh_crb_create(dfh_ctx* c, dfh_crb** out);
int dfh_crb_destroy(dfh_crb* e);
int dfh_crb_encode_host(dfh_crb* e, size_t nrows, const size_t* offset, const float* label, const uint64_t* index, const float* value,
                        const float* weight, size_t* record_bytes);
int dfh_crb_encode_textchunk(dfh_crb* e, dfh_textchunk* tc, size_t* record_bytes);
int dfh_crb_record(dfh_crb* e, void* dst);
/* task = convert with shuffle_rows / val_fraction: the rows of a whole data set in HBM (csrc/dfh_rowstore.hip).  A dfh_rowstore
 * holds ids (u64), labels and row lengths, values once a chunk brought some and weights when every chunk brings them.  Ids and
 * values live in slabs of slab_bytes (0: 64 MiB; 1 KiB .. 16 GiB): a row never straddles two slabs, a row longer than a slab
 * gets one of its own size, and an append allocates what it adds and copies nothing that is stored.  An allocation that fails is
 * DFH_ERR_CAPACITY with the bytes it needed in the message and leaves the store as it was; a store holds fewer than 2^32 - 16
 * rows (DFH_ERR_ARG).
 * dfh_rowstore_append_host: arguments as dfh_crb_encode_host (index / value are the chunk's own nonzeros; value and weight may
 * be NULL); dfh_rowstore_append_textchunk: the regular chunk last parsed into `tc`, its ids copied device to device.  Both
 * return when the source may be reused.  A chunk without values counts as all 1.0f; weights in some chunks and not in others
 * are DFH_ERR_ARG.  Rows are numbered in the order they were appended, however they were cut into appends; an append drops
 * the order.
 * dfh_rowstore_order fixes the order of the rows: shuffle = 0 the identity, shuffle = 1 ascending by (key(r), r), key(r) =
 * output r of splitmix64 seeded with `seed` (z = seed + (r + 1) 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31; mod 2^64), made and sorted on the device: a stable argsort of the keys.
 * It may be called again; no encode or read may run beside it.  dfh_rowstore_get_order: order [nrows] (tests).
 * dfh_rowstore_read: rows order[first .. first + count) on the host: offset [count + 1] from 0, label [count], *nnz, and when
 * index is not NULL index [*nnz], value [*nnz] (all 1.0f from a store without values) and weight [count] (only of a store
 * that has weights); value and weight may be NULL.  A caller that does not know *nnz asks with index = NULL first.
 * dfh_crb_encode_rowstore: the same rows gathered on the encoder's stream into its own staging and encoded: byte for byte
 * the record dfh_crb_encode_host gives for them with offsets from 0 (values that are all 1.0f in the block are dropped).
 * Several encoders may work on one ordered store from different threads.  Without an order read and encode are
 * DFH_ERR_STATE; first + count > nrows is DFH_ERR_ARG. */
typedef struct dfh_rowstore dfh_rowstore;
int dfh_rowstore_create(dfh_ctx* c, size_t slab_bytes, dfh_rowstore** out);
int dfh_rowstore_destroy(dfh_rowstore* st);
int dfh_rowstore_append_host(dfh_rowstore* st, size_t nrows, const size_t* offset, const float* label, const uint64_t* index,
                             const float* value, const float* weight);
int dfh_rowstore_append_textchunk(dfh_rowstore* st, dfh_textchunk* tc);
int dfh_rowstore_shape(dfh_rowstore* st, uint64_t* nrows, uint64_t* nnz, int* has_value, int* has_weight, uint64_t* device_bytes);
int dfh_rowstore_order(dfh_rowstore* st, int shuffle, uint64_t seed);
int dfh_rowstore_get_order(dfh_rowstore* st, uint32_t* order);
int dfh_rowstore_read(dfh_rowstore* st, uint64_t first, size_t count, size_t* offset, float* label, uint64_t* index, float* value,
                      float* weight, size_t* nnz);
int dfh_crb_encode_rowstore(dfh_crb* e, dfh_rowstore* st, uint64_t first, size_t count, size_t* record_bytes);
/* dfh_rowbuf_load_host_slices whose slices are either host arrays (chunk = NULL; value may be NULL = all ones) or ids
 * [first, first + nnz) of a regular parsed chunk (index and value unused; no values), copied device to device on the
 * buffer's stream.  Same contract: it returns when the sources may be reused (the chunk may be parsed into again). */
typedef struct {
  const uint64_t* index;
  const float* value;
  dfh_textchunk* chunk;
  size_t first;
  size_t nnz;
} dfh_slice;
int dfh_rowbuf_load_slices(dfh_rowbuf* rb, size_t nrows, const size_t* offset, int nslices, const dfh_slice* slices);
int dfh_batch_gather_rows(dfh_batch* b, size_t nrows, const size_t* offset, const float* label, int nseg, dfh_rowbuf* const* bufs,
                          const uint32_t* const* rows, const size_t* seg_rows);
/* dfh_batch_gather_rows + dfh_localize + dfh_batch_lookup as ONE preparation phase — what a worker loop queues per
 * minibatch (src/sgd/sgd_learner.cc:196-224: read, localize, pull): the minibatch's description is read by the gather
 * kernel where the host wrote it (page-locked, mapped: no copy is queued), the phase records one cross-stream event.
 * Same results as the three calls; about half their host time per minibatch. */
int dfh_batch_prepare_rows(dfh_table* t, dfh_batch* b, size_t nrows, const size_t* offset, const float* label, int nseg,
                           dfh_rowbuf* const* bufs, const uint32_t* const* rows, const size_t* seg_rows, uint64_t max_index);
/* Row buffers that stay (the SGD learner's data_cache = hbm): dfh_rowbuf_set_labels gives a loaded buffer the labels of its
 * rows [nrows = the rows it holds]; the buffer keeps its own offsets already.  A minibatch out of such buffers is then
 * described by its row numbers alone: dfh_batch_prepare_cached is dfh_batch_prepare_rows without `offset` and `label` — the
 * same phase (row gather + Localizer + lookup, one cross-stream event), the minibatch's offsets (an exclusive scan of the
 * gathered rows' lengths) and labels (a gather) derived on the device (k_loc_describe) into the arrays
 * dfh_batch_gather_rows fills.  The same batch, bit for bit.  A reload of the buffer drops its labels. */
int dfh_rowbuf_set_labels(dfh_rowbuf* rb, size_t nrows, const float* label);
int dfh_batch_prepare_cached(dfh_table* t, dfh_batch* b, size_t nrows, int nseg, dfh_rowbuf* const* bufs, const uint32_t* const* rows,
                             const size_t* seg_rows, uint64_t max_index);

/* already-localized batch from the host (what SGDLearner hands its batch thread,
 * src/sgd/sgd_learner.cc:203-212): feaids sorted unique, compact u32 index */
int dfh_batch_load_localized_host(dfh_batch* b, size_t nrows, const size_t* offset, const uint32_t* index,
                                  const float* value, const float* label, const uint64_t* feaids,
                                  const float* feacnt, size_t U);
/* read back the localizer's outputs (any may be NULL); synchronises */
int dfh_batch_get_localized(dfh_batch* b, size_t* U, uint64_t* feaids, float* feacnt, uint32_t* index);
int dfh_batch_shape(dfh_batch* b, size_t* nrows, size_t* nnz, size_t* U); /* synchronises for U */
/* the loaded minibatch's CSR offsets [nrows + 1] and labels [nrows] as the device holds them; synchronises */
int dfh_batch_get_rows(dfh_batch* b, uint32_t* offset, float* label);

/* ---------------------------------------------------------- the fused step */
/* The batch executor of SGDLearner::IterateData (src/sgd/sgd_learner.cc:131-178)
 * for one localized batch, entirely on device:
 *   [push_cnt: Push(kFeaCount)] -> Pull -> Predict -> Evaluate(+penalty,+AUC)
 *   -> [is_train: CalcGrad -> Push(kGradient) -> FTRL/AdaGrad in place].
 * Asynchronous; metrics accumulate in the batch and are read with dfh_batch_progress. */
int dfh_sgd_step(dfh_table* t, dfh_batch* b, int is_train, int push_cnt);
int dfh_batch_progress(dfh_batch* b, dfh_progress* out, int reset); /* synchronises */
int dfh_batch_get_pred(dfh_batch* b, float* pred);                  /* synchronises */
/* entries of the batch's split list: the parts (of 1 024 occurrences) of the keys with more than 4 096 occurrences that the
 * last TRAINING step (dfh_sgd_step, dfh_shard_step) of this batch object listed for its update; 0 before the first.  Every
 * training step starts from an empty list, so the value does not depend on how often the batch was stepped since it was
 * localized.  Read-only; synchronises. */
int dfh_batch_split_entries(dfh_batch* b, uint32_t* n);

/* The localized minibatch as the backward and update passes walk it, read back for the tests: the key-ordered view and the
 * segment lists.  dfh_batch_key_view_info gives the sizes to allocate; dfh_batch_get_key_view fills host arrays (any may be
 * NULL).  Both synchronise the way dfh_batch_shape does, launch nothing and write no batch state: a step taken afterwards
 * gives the bits it would have given without them.  A batch that is not localized is refused and stays usable. */
typedef struct dfh_key_view_info {
  uint64_t U, nnz;
  uint32_t has_value;   /* 0: a binary minibatch, there is no s_val */
  uint32_t seg_nb;      /* list buckets: every list has seg_nb {cnt, off} descriptors */
  uint32_t P;           /* sort buckets, where the view came out of the sample sort (then seg_nb == P); else 0 */
  uint32_t split_n;     /* entries of the split list: what dfh_batch_split_entries reads */
  uint64_t few_cap, mid_cap, hot_cap, split_cap;   /* entries the four arrays were allocated for (dfh_batch_create) */
  uint32_t bwd_small, bwd_mid, hot_split, hot_split_min;   /* the class bounds the library was built with */
} dfh_key_view_info;
int dfh_batch_key_view_info(dfh_batch* b, dfh_key_view_info* out);
/* col_ptr [U + 1], s_row [nnz], s_val [nnz] (ignored for a binary minibatch); few / mid / hot: desc [seg_nb][2] = {cnt, off}
 * and ent [cap][4] = the WHOLE entry array {u, beg, end, 0}, of which only the ranges [off, off + cnt) of the descriptors
 * mean anything; split_ent [split_n][4] = {u, beg_p, end_p, p << 16 | nparts}; bstart [P + 1] where P > 0. */
int dfh_batch_get_key_view(dfh_batch* b, uint32_t* col_ptr, uint32_t* s_row, float* s_val, uint32_t* few_desc, uint32_t* few_ent,
                           uint32_t* mid_desc, uint32_t* mid_ent, uint32_t* hot_desc, uint32_t* hot_ent, uint32_t* split_ent,
                           uint32_t* bstart);

/* -------------------------------------------- sharded (multi-GPU) building blocks */
/* Rows cross the wire in a fixed-stride layout of dfh_row_stride(V_dim) floats:
 *   [w, has_V (0/1 as float), 0, 0 | V[0..V_dim) zero-padded to a multiple of 4]
 * gradients use the same layout: [gw, has_V, 0, 0 | gV...].  All DEVICE pointers. */
size_t dfh_row_stride(int V_dim);
/* owner side of Pull: look up / insert n unique keys, write rows */
int dfh_shard_pull(dfh_table* t, const uint64_t* d_keys, size_t n, float* d_rows);
/* owner side of Push(kFeaCount) and Push(kGradient) for n unique keys */
int dfh_shard_push_count(dfh_table* t, const uint64_t* d_keys, size_t n, const float* d_cnt);
int dfh_shard_push_grad(dfh_table* t, const uint64_t* d_keys, size_t n, const float* d_grads);
/* worker side: Predict+Evaluate on pulled rows [U x stride], then (is_train)
 * CalcGrad into d_grads [U x stride]; pointers to the batch's device feaids/cnt */
int dfh_batch_forward(dfh_batch* b, int V_dim, const float* d_rows);
int dfh_batch_backward(dfh_batch* b, int V_dim, const float* d_rows, float* d_grads);
int dfh_batch_device_keys(dfh_batch* b, const uint64_t** d_feaids, const float** d_feacnt, size_t* U);
/* key-range partition of the batch's (ascending) unique keys over nparts shards:
 * shard d owns keys in [d*span, (d+1)*span), span = ceil(2^64/nparts) — the range
 * partitioning ReverseBytes exists for (include/difacto/base.h:29-38).  HOST output
 * bounds[nparts+1]: shard d gets feaids[bounds[d] .. bounds[d+1]).  Synchronises. */
int dfh_batch_key_ranges(dfh_batch* b, int nparts, uint32_t* bounds);
/* the same bounds as int64 into DEVICE memory d_bounds[nparts+1], enqueued on the main
 * stream after the batch's preparation; does not synchronise (d_bounds[nparts] = U).
 * d_splits == NULL: the uniform partition above.  Otherwise d_splits[nparts-1] (device,
 * ascending): shard d >= 1 owns keys in [d_splits[d-1], d_splits[d]) — still contiguous key
 * ranges, with boundaries the caller balanced for its id space (feature-group ids sit in the
 * top bits of a reversed key, base.h:60-63, so uniform ranges can be badly skewed). */
int dfh_batch_key_ranges_device(dfh_batch* b, int nparts, const uint64_t* d_splits, int64_t* d_bounds);

/* Owner side in resolved form, for keys arriving from several source ranks in one step
 * (StoreLocal::Push/Pull per source, src/store/store_local.h:24-44; SGDUpdater::Get/Update,
 * src/sgd/sgd_updater.cc:32-102).  dfh_shard_resolve probes/inserts ALL received keys once
 * (the same key may appear under several sources) and writes their row ids; Pull is then one
 * gather over all of them; the two Push kinds take one source's slice at a time (keys unique
 * inside a call) and are applied in call order.  V_init must be "hash". */
int dfh_shard_resolve(dfh_table* t, const uint64_t* d_keys, size_t n, uint32_t* d_rowid);
int dfh_shard_pull_resolved(dfh_table* t, const uint32_t* d_rowid, size_t n, float* d_rows);
int dfh_shard_push_count_resolved(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, size_t n, const float* d_cnt);
int dfh_shard_push_grad_resolved(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, size_t n, const float* d_grads);
/* The same for ALL source ranks of a step in one launch per operation.  d_keys is the
 * concatenation of nsrc ascending key lists, source s holding entries [seg[s], seg[s+1]) (seg:
 * HOST array of nsrc+1 offsets, nsrc <= 32; n = seg[nsrc] < 2^27 entries).  d_rowid holds
 * dfh_shard_multi_words(n, nsrc) words: [0, n) the entries' row words (the row id in the low 29
 * bits — what dfh_shard_pull_resolved reads), behind them, per entry, the indices of the other
 * entries that carry the same key (written by resolve_multi for ONE entry per key, the first to
 * be resolved; read by the Push calls).  In the two Push calls that entry applies every
 * source's value in ascending source order (the result of nsrc per-source calls) and stores the
 * row once.  push_grad_multi ends the step for these rows; a step without it (validation) ends
 * with dfh_shard_release.  mask_slot (0 or 1) names which of two per-row step words the step
 * uses: an owner may hold two steps at once — one resolved and pulled, the other still awaiting
 * its gradients (the reference keeps two minibatches in flight, sgd_learner.cc:219-223) — and
 * they must use different slots. */
size_t dfh_shard_multi_words(size_t n, int nsrc);
int dfh_shard_resolve_multi(dfh_table* t, const uint64_t* d_keys, const size_t* seg, int nsrc, int mask_slot,
                            uint32_t* d_rowid);
int dfh_shard_push_count_multi(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, const size_t* seg, int nsrc,
                               int mask_slot, const float* d_cnt);
int dfh_shard_push_grad_multi(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, const size_t* seg, int nsrc,
                              int mask_slot, const float* d_grads);
/* The owner side per DISTINCT key (what dfh_shard_step uses): dfh_shard_count_pull_multi is Push(kFeaCount) of all sources
 * (d_cnt; NULL = no counts this step) and Pull in one launch — a key's row is read once and written to the output row of
 * every entry that carries the key (d_rows: n rows of dfh_row_stride floats, entry order) — and leaves, behind the extras in
 * d_rowid, the step's keys as lists; dfh_shard_push_grad_listed is Push(kGradient) of all sources over those lists (same
 * seg / mask_slot; d_grads in entry order; ends the step like push_grad_multi).  Results equal the per-entry calls above. */
int dfh_shard_count_pull_multi(dfh_table* t, uint32_t* d_rowid, const uint64_t* d_keys, const size_t* seg, int nsrc, int mask_slot,
                               const float* d_cnt, float* d_rows);
int dfh_shard_push_grad_listed(dfh_table* t, const uint32_t* d_rowid, const uint64_t* d_keys, const size_t* seg, int nsrc,
                               int mask_slot, const float* d_grads);
int dfh_shard_release(dfh_table* t, const uint32_t* d_rowid, size_t n, int mask_slot);
/* fetch and report the table's sticky device-side error word (capacity exceeded, gradient
 * with V for a row without V); synchronises */
int dfh_table_check(dfh_table* t);

/* ------------------------------------------------------ sharded store (multi-GPU) */
/* The ps-lite Push / Pull of the reference (include/difacto/store.h:53-93, src/store) for the ranks
 * of one node, one process per GPU: rank r owns a contiguous range of the reversed keys (uniform:
 * [r*span, (r+1)*span), span = ceil(2^64/world); or the explicit split keys given to
 * dfh_shard_create) and trains its own minibatches.  Nothing here is a collective on host data:
 * all traffic is device buffers over the communicator. */
typedef struct dfh_comm dfh_comm;
typedef struct dfh_shard dfh_shard;
#define DFH_COMM_ID_BYTES 128
/* RCCL transport (ncclSend / ncclRecv over xGMI).  Rank 0 obtains an id and hands it to the other
 * ranks out of band (a file, an env var, MPI ...); every rank then creates its communicator. */
int dfh_comm_unique_id(void* id128);
int dfh_comm_create_rccl(dfh_ctx* ctx, int rank, int world, const void* id128, dfh_comm** out);
/* Host-callback transport: the library stages every exchange through host memory and calls
 * fn(user, send, send_bytes[world], recv, recv_bytes[world]) — an all-to-all-v of bytes, contiguous in peer
 * order on both sides; 0 = ok.  For process groups RCCL cannot serve (several ranks sharing one GPU in
 * a test, a gloo / MPI / socket fabric of the host). */
typedef int (*dfh_alltoallv_fn)(void* user, const void* send, const size_t* send_bytes, void* recv, const size_t* recv_bytes);
int dfh_comm_create_callback(dfh_ctx* ctx, int rank, int world, dfh_alltoallv_fn fn, void* user, dfh_comm** out);
/* Loop-back transport — MEASUREMENT ONLY: rank `rank` of a `world`-rank job alone on its GPU.  Every exchange of
 * dfh_shard_step moves messages of the exact sizes a real job would move, as device-to-device copies instead of wires:
 * what this rank "sends" is read out of its send buffer (and dropped), what it "receives" is copied out of a buffer the
 * caller has FED for that kind of exchange (dfh_comm_loopback_feed) — laid out like the receive side of the exchange
 * (contiguous in peer order, or at the receive offsets) — so that every owner-side and worker-side kernel of the step
 * runs at its real size on valid data, on a chip no other rank shares (Store::Push / Pull of the reference with the
 * seven other workers played back: include/difacto/store.h:53-93, src/sgd/sgd_learner.cc:78-89).  The rank's own slot
 * of an exchange is a real self-copy.  An exchange whose kind was not fed echoes the rank's own send data.
 * Optional wire model: an exchange holds its stream for latency_us + (largest per-peer message, either direction) /
 * link_gbps (one xGMI link per peer and direction), whichever of that and the copies is longer; link_gbps = 0: copies only. */
enum { DFH_XCHG_COUNTS = 0, DFH_XCHG_KEYS, DFH_XCHG_CNT, DFH_XCHG_ROWS, DFH_XCHG_GRADS, DFH_XCHG_OTHER, DFH_XCHG_KINDS };
int dfh_comm_create_loopback(dfh_ctx* ctx, int rank, int world, dfh_comm** out);
/* the source of the NEXT exchange of `kind` (a FIFO per kind; sticky != 0: of every later exchange of that kind
 * until the next feed).  d_src must stay valid until that exchange has run. */
int dfh_comm_loopback_feed(dfh_comm* c, int kind, const void* d_src, int sticky);
int dfh_comm_loopback_wire(dfh_comm* c, double link_gbps, double latency_us);
/* modelled wire time (microseconds) of all exchanges since the last reset */
int dfh_comm_loopback_wire_time(dfh_comm* c, int reset, double* us);
int dfh_comm_destroy(dfh_comm* c);
int dfh_comm_rank(dfh_comm* c);
int dfh_comm_world(dfh_comm* c);
/* sum of n <= 64 host doubles over the ranks (same result on every rank): progress merging, votes */
int dfh_comm_allreduce_sum(dfh_comm* c, double* vals, int n);
/* every rank's `bytes` host bytes to every rank: recv holds world * bytes, in rank order.  COLLECTIVE. */
int dfh_comm_allgather(dfh_comm* c, const void* send, size_t bytes, void* recv);
/* payload bytes this rank has sent to / received from OTHER ranks and the number of message groups, since the last
 * reset (what the N > 1 bench line prices against the xGMI links: `roofline_exchange`) */
int dfh_comm_stats(dfh_comm* c, int reset, uint64_t* bytes_sent, uint64_t* bytes_recv, uint64_t* groups);
/* which transport is bound: "rccl <version> from <file> (already loaded by the host process | loaded by libdifacto_hip)"
 * or "host callback transport".  A host that already carries an RCCL (PyTorch bundles one) shares it. */
int dfh_comm_info(dfh_comm* c, char* buf, size_t n);
/* start-up self-check, collective: a first exchange of the ranks' ids, polled; DFH_ERR_STATE after timeout_s seconds
 * if a peer never joins (bad rendezvous) or if the ids do not add up — fails loudly instead of hanging the first step.
 * The reference's Store has no such call: its ps-lite van blocks in Postoffice::Barrier (include/difacto/store.h:53-93
 * is the interface this transport serves). */
int dfh_comm_selfcheck(dfh_comm* c, double timeout_s);
/* what the wires give: `reps` grouped exchanges (after two untimed ones) in which this rank sends bytes_per_peer to and
 * receives bytes_per_peer from EVERY other rank — the shape of dfh_shard_step's key / row / gradient exchanges (the
 * reference's ps-lite Push / Pull traffic, include/difacto/store.h:53-93), every xGMI link of a full mesh carrying one
 * message each way at once — timed on the context's stream.  *us_per_exchange = the average; bytes_per_peer over it is
 * what one link gave per direction.  COLLECTIVE; 0 with one rank.  bench.py --gpus N runs it before the timed region. */
int dfh_comm_wire_probe(dfh_comm* c, size_t bytes_per_peer, int reps, double* us_per_exchange);
/* Split keys that balance the shards on the DATA instead of on the key space: every rank hands in a sample of the
 * reversed keys it will see (n may differ per rank, 0 allowed); the samples are gathered and splits[world-1] receives
 * the (identical on every rank) quantiles of their union — the argument for dfh_shard_create.  With feature-group ids
 * in the low bits of an id (EncodeFeaGrpID, include/difacto/base.h:60-63) ReverseBytes moves them to the top of the
 * key and a uniform cut of the key space is badly skewed (39 criteo slots over 8 shards: one shard 2.3x the
 * average).  COLLECTIVE.  With no key in any sample the uniform split keys are returned. */
int dfh_shard_balanced_splits(dfh_comm* c, const uint64_t* sample_keys, size_t n, uint64_t* splits);

/* this rank's shard of the model + the exchange buffers.  splits: world-1 ascending first keys of
 * shards 1.., identical on every rank, or NULL for the uniform ranges.  The table must use
 * DFH_INIT_HASH (order- and sharding-independent V init). */
int dfh_shard_create(dfh_table* t, dfh_comm* c, const uint64_t* splits, dfh_shard** out);
int dfh_shard_destroy(dfh_shard* s);
/* [key_lo, key_hi) owned by this rank (key_hi = 0: no upper bound) — the range to hand dfh_table_load */
int dfh_shard_owned_range(dfh_shard* s, const uint64_t* splits, uint64_t* key_lo, uint64_t* key_hi);
/* One step of SGDLearner::IterateData (src/sgd/sgd_learner.cc:131-178) against the sharded model:
 * keys -> owners, rows back, Predict / Evaluate / CalcGrad on the pulled rows, gradients -> owners,
 * applied in ascending source-rank order (zero staleness).  COLLECTIVE: every rank calls it the same
 * number of times with the same is_train / push_cnt; a rank whose data is exhausted passes
 * b = NULL and keeps serving its shard.  *any_active = 0 when no rank had a minibatch (the step was a
 * no-op: the epoch is over).  Asynchronous apart from one small host wait; progress accumulates in
 * the batch as in dfh_sgd_step. */
int dfh_shard_step(dfh_shard* s, dfh_batch* b, int is_train, int push_cnt, int* any_active);
/* Optional, COLLECTIVE like the step: called on every rank right before dfh_shard_step, it names the
 * minibatch of the FOLLOWING step (its dfh_localize already queued; NULL if this rank has none left).
 * The step then sends that minibatch's per-owner key counts on their way inside itself — behind its own
 * backward pass, while its gradients travel — and the following dfh_shard_step (which must be given
 * exactly that batch) starts with the counts already on the host instead of waiting for them mid-way:
 * what the reference's batch tracker achieves by keeping two minibatches in flight
 * (sgd_learner.cc:219-223), here without staleness.  No-op with one rank. */
int dfh_shard_prefetch_counts(dfh_shard* s, dfh_batch* b_next);
/* How dfh_shard_step moves the rows.  0 (default) = sync: one minibatch at a time, every exchange on the context's
 * stream, zero staleness.  1 = overlap: TWO minibatches in flight, what the reference's batch tracker does
 * (src/sgd/sgd_learner.cc:219-223: the next minibatch is issued while one is pending, so its Pull may be served
 * before the previous Push has landed).  Inside dfh_shard_step(b) the minibatch named by the preceding
 * dfh_shard_prefetch_counts has its counts, keys and rows exchanged on a second stream while b computes:
 *     collectives' stream:  counts(t+1)  K(t+1)              G(t)            RW(t+1)
 *     main stream:          L(t) F(t) [gradient rows | own keys updated in place]  R(t+1)        P(t)
 * so the gradients of t travel while the owners pull for t+1, and the rows of t+1 travel while the gradients of t
 * are applied.  Staleness: the keys a rank owns itself are read with zero staleness (L(t+1) runs after P(t)); rows
 * pulled from other owners miss the gradients the OTHER ranks computed in step t (staleness 1, exactly one
 * minibatch), and contain the owner's own step-t update.  Every table operation runs on the main stream in program
 * order: nothing races on a row, every pulled row is one consistent version of its key.  The announced minibatch
 * is pulled (and its epoch-0 counts pushed) with the push_cnt of the call it rides in: the flag is a property of the
 * job (src/sgd/sgd_learner.cc:201-202), keep it constant from one announcement to the step.  Call between steps only
 * (no minibatch under way); COLLECTIVE in effect: every rank must use the same mode. */
int dfh_shard_set_exchange(dfh_shard* s, int mode);
/* Exchange buffers for minibatches of up to batch_keys unique keys and up to recv_keys keys received from the other
 * ranks per step, allocated NOW (after dfh_shard_set_exchange: the overlapped exchange keeps two sets).  Optional: without
 * it — and for a minibatch beyond these sizes — dfh_shard_step grows the buffers when it first meets the size, which
 * drains the streams and re-allocates in the middle of a step (the reference's store has no counterpart: ps-lite
 * allocates per message).  With key ranges balanced on the data, recv_keys ~ batch_keys; 2 x is generous. */
int dfh_shard_reserve(dfh_shard* s, size_t batch_keys, size_t recv_keys);
/* Per-stage device time of the steps since the last reset (HIP events around every stage; they cost the streams a
 * few microseconds each: for a diagnostic pass, not for the timed run).  ms[DFH_SHARD_STAGES]: counts, L (own keys'
 * lookup), K, R, RW, F (forward + backward / own update), G, P; *steps = steps covered. */
enum { DFH_SHARD_STAGE_COUNTS = 0, DFH_SHARD_STAGE_L, DFH_SHARD_STAGE_K, DFH_SHARD_STAGE_R, DFH_SHARD_STAGE_RW, DFH_SHARD_STAGE_F,
       DFH_SHARD_STAGE_G, DFH_SHARD_STAGE_P, DFH_SHARD_STAGES };
int dfh_shard_set_timing(dfh_shard* s, int enable);
int dfh_shard_get_timing(dfh_shard* s, int reset, double* ms, uint64_t* steps);

/* The literal Store::Pull / Store::Push (include/difacto/store.h:53-73) against the SHARDED model, with host arrays in the
 * layout of dfh_pull / dfh_push: what the reference's worker loop calls once per minibatch when it runs call by call
 * (device_path = literal) instead of through dfh_shard_step.  keys: ascending, unique (a Localizer's output).
 * COLLECTIVE: every rank makes the same sequence of calls with the same val_type; a rank with nothing to ask passes
 * n = 0 and still serves its shard.  One exchange each way per call, everything on the context's stream, synchronous.
 * Pushes from several ranks to one key are applied in ascending rank order (FTRL / AdaGrad are not linear: the order is
 * part of the result, and fixed). */
int dfh_shard_pull_host(dfh_shard* s, const uint64_t* keys, size_t n, float* vals, size_t* nvals, int* lens, size_t* nlens);
int dfh_shard_push_host(dfh_shard* s, const uint64_t* keys, size_t n, int val_type, const float* vals, size_t nvals, const int* lens,
                        size_t nlens);

/* ------------------------------------------------ full-batch L-BFGS (learner = lbfgs) */
/* Vector kernels of LBFGSUpdater on DEVICE pointers (16-byte aligned), fp32 elements; every reduction runs in a fixed
 * order (the same answer on every run) and synchronises.
 * dfh_vec_inner_multi: out[i * nb + j] = <a_i, b_j> as lbfgs::Inner (src/lbfgs/lbfgs_utils.h:62-72): fp32 products summed
 * in fp64, one pass that reads every distinct vector once (Twoloop::CalcIncreB, lbfgs_twoloop.h:19-43); na <= 3, nb <= 33. */
int dfh_vec_inner_multi(dfh_ctx* ctx, uint64_t n, int na, const float* const* a, int nb, const float* const* b, double* out);
/* dfh_vec_combine: per element p = 0; lbfgs::Add(coef[k], v[k], &p) for k = 0 .. nv-1 in order (coef 0 skipped, coef 1 a
 * plain add, lbfgs_utils.h:74-88); p clamped to +-clampv (lbfgs_updater.h:117); out = p (out may be one of v); *out_dot =
 * <dot, p> when dot is not NULL (LBFGSUpdater::CalcDirection, lbfgs_updater.h:107-123).  nv <= 33. */
int dfh_vec_combine(dfh_ctx* ctx, uint64_t n, int nv, const float* const* v, const float* coef, float clampv, float* out,
                    const float* dot, double* out_dot);
/* dfh_vec_line_step: lbfgs::Add(x, p, &w) (p may be NULL: no step), then out3 = { r(w) = sum .5 coef w^2, <coef w, p>,
 * nnz(w) } with coef = V_l2 where bit i of vmask is set and l2 elsewhere (vmask NULL: l2 everywhere) —
 * LBFGSUpdater::LineSearch / Evaluate / AddRegularizerGrad (lbfgs_updater.h:125-133, 170-203) */
int dfh_vec_line_step(dfh_ctx* ctx, uint64_t n, float* w, const float* p, float x, const uint32_t* vmask, float l2, float V_l2,
                      double* out3);

/* The learner's state, resident in HBM from load to finish: the localized training and validation chunks (one dfh_batch
 * each, plus its key -> model map), the model (keys ascending, lens, w: per key w [, V]) and w, g_new, g and the s / y
 * history of m pairs (1 <= m <= 16).  One process, one GPU.  Calls follow the jobs of LBFGSLearner::Process
 * (src/lbfgs/lbfgs_learner.cc:128-163); each synchronises.  Data or state that does not fit in HBM fails with
 * DFH_ERR_CAPACITY and the bytes needed. */
typedef struct dfh_lbfgs dfh_lbfgs;
int dfh_lbfgs_create(dfh_ctx* ctx, int V_dim, int m, dfh_lbfgs** out);
/* The same learner over the ranks of a communicator (RCCL or host callback; not the loop-back transport): each rank is a
 * worker for its own chunks (1/N of the rows) and the owner of one slice of the ascending keys (1/N of the model and
 * of the optimiser state), what the reference's RunScheduler does with its worker and server groups
 * (src/lbfgs/lbfgs_learner.cc:14-163).  On such an object EVERY dfh_lbfgs_* call below is COLLECTIVE: every rank makes
 * the same calls in the same order (a rank without rows adds no chunk and still takes part).  What they return —
 * loss, AUC x n, incr_B, <p, g>, objv, nnz(w), r(w) — are sums over the ranks (each rank's fp64 partials added in rank
 * order): every rank gets the same bits, and with one rank the bits of dfh_lbfgs_create's object.
 *   init_model  split keys balanced on the ranks' training keys; the owner adds the counts over ranks and filters
 *               (tail_feature_filter, V_threshold) on the global counts; V comes from the one rand_r(seed = 0) chain in
 *               global key order, so the union of the shards is the model one process builds from the same rows.
 *   calc_grad   the owners' rows go to the workers that use them (k_lb_pack + all-to-all-v), the chunks run on the
 *               local copy, the local gradients go back and each owned element adds its contributions in ascending
 *               source rank (k_lb_reduce): no float atomics, the same bits over every run and transport.
 *   the others  run on the rank's own slice; only their fp64 partials cross the wire.
 * shape, get_model and set_weights see the rank's own slice (keys ascending).  DFH_ERR_CAPACITY applies per rank. */
int dfh_lbfgs_create_sharded(dfh_ctx* ctx, dfh_comm* comm, int V_dim, int m, dfh_lbfgs** out);
int dfh_lbfgs_destroy(dfh_lbfgs* o);
/* a chunk of raw rows (Reader::Value()), localized on the device with Localizer(-1) (TileBuilder::Add) and kept */
int dfh_lbfgs_add_chunk(dfh_lbfgs* o, int is_val, size_t nrows, const size_t* offset, const uint64_t* index, const float* value,
                        const float* label);
/* InitWeight (lbfgs_updater.h:33-76) + InitWorker's filter and colmap (lbfgs_learner.cc:189-212): merged training counts,
 * keys with cnt > tail_feature_filter survive (filter <= 0: all), lens = 1 + (cnt > V_threshold ? V_dim : 0), w = 0 and
 * V from the rand_r(seed = 0) chain in key order */
int dfh_lbfgs_init_model(dfh_lbfgs* o, float tail_feature_filter, int V_threshold, float V_init_scale, float l2, float V_l2,
                         uint64_t* nkeys, uint64_t* nparams);
int dfh_lbfgs_shape(dfh_lbfgs* o, uint64_t* nkeys, uint64_t* nparams, int* ntrain_chunks, int* nval_chunks);
/* read the model back (any pointer may be NULL): keys [nkeys], lens [nkeys], merged counts [nkeys], w [nparams] */
int dfh_lbfgs_get_model(dfh_lbfgs* o, uint64_t* keys, int* lens, float* feacnt, float* w);
/* SetWeightInitializer: replace w [nparams] before training starts */
int dfh_lbfgs_set_weights(dfh_lbfgs* o, const float* w);
/* [key_lo, key_hi) of the keys this rank owns on a dfh_lbfgs_create_sharded object (key_hi = 0: no upper bound; a plain
 * object owns everything: 0, 0), known after dfh_lbfgs_init_model — the range to hand dfh_table_load */
int dfh_lbfgs_owned_range(dfh_lbfgs* o, uint64_t* key_lo, uint64_t* key_hi);
/* after dfh_lbfgs_init_model, before the first dfh_lbfgs_calc_grad: start from a model given by key.
 * keys [n] unique, any order; lens [n] in {1, 1 + V_dim}; vals ragged [sum lens] = w then V, the layout of dfh_pull.
 * The keys are matched against the object's ascending keys on the device (one lane per input key, a binary search; no
 * host-side map).  A matched key takes the input's w, and the input's V only where BOTH the model's lens and the input's
 * are 1 + V_dim; otherwise the model's V keeps its rand_r initial value (or the model has none).  An input key the model
 * does not hold (filtered, or never seen in the training data) is dropped; a model key that is not in the input keeps
 * what init_model gave it, bit for bit.  Given the whole model, the object equals one that took the same floats through
 * dfh_lbfgs_set_weights.  *n_matched (may be NULL): input keys that are keys of the model.
 * On a dfh_lbfgs_create_sharded object COLLECTIVE: every rank passes the entries of ITS OWN key range
 * (dfh_lbfgs_owned_range; an entry outside it is an error) and *n_matched is the sum over ranks; nothing crosses the
 * wire but one dfh_comm_allreduce_sum of that count (and of whether every rank accepted its entries: they fail together).
 * Errors: DFH_ERR_STATE after a gradient pass; DFH_ERR_ARG for repeated keys, a bad lens or a foreign key. */
int dfh_lbfgs_set_model(dfh_lbfgs* o, uint64_t n, const uint64_t* keys, const int* lens, const float* vals, uint64_t* n_matched);
/* CalcGrad (lbfgs_learner.cc:246-305) into g_new: loss and AUC x n summed per chunk as the reference sums them */
int dfh_lbfgs_calc_grad(dfh_lbfgs* o, float gamma, float* loss, float* auc_n);
/* PrepareCalcDirection: *mcur = history pairs in use (0 at epoch 0: nothing is returned), incr_B [6 mcur + 1] */
int dfh_lbfgs_prepare_direction(dfh_lbfgs* o, float* incr_B, int* mcur);
/* CalcDirection with the two-loop coefficients d [2 mcur + 1] (NULL at epoch 0: p = -g); *p_g = <p, g> */
int dfh_lbfgs_calc_direction(dfh_lbfgs* o, const float* d, float* p_g);
/* LineSearch(alpha): w += (alpha - alpha_) p, CalcGrad; *objv = f(w + alpha p), *p_g = <grad f, p>, *auc_n (may be NULL) */
int dfh_lbfgs_line_search(dfh_lbfgs* o, float alpha, float gamma, float* objv, float* p_g, float* auc_n);
/* Evaluate: validation AUC x n (NULL: skipped), nnz(w), r(w) */
int dfh_lbfgs_evaluate(dfh_lbfgs* o, float* val_auc_n, float* nnz_w, float* r_w);
/* read one of the object's model-sized vectors back, out [nparams] (on a sharded object the rank's owned slice): a copy on
 * the context's stream and a synchronise, no kernel.  It exists so that tests can assert the state element by element.
 *   which 0  g_new  (i ignored)
 *         1  g      (i ignored; DFH_ERR_ARG before the first dfh_lbfgs_prepare_direction)
 *         2  s      logical index i, oldest first, 0 <= i < the number of s vectors held
 *         3  y      logical index i, oldest first, 0 <= i < the number of y vectors held
 * Any other which, or an index outside the history, is DFH_ERR_ARG. */
int dfh_lbfgs_get_vector(dfh_lbfgs* o, int which, int i, float* out);

/* l1 on w: orthant-wise L-BFGS (OWL-QN, Andrew & Gao 2007; csrc/dfh_owlqn.hip states every rule and its fp32 order).
 * The objective becomes F(w) = loss + sum .5 coef w^2 + l1 sum |w| over the w elements; V keeps V_l2 alone.
 * dfh_lbfgs_set_l1: after dfh_lbfgs_init_model and before the first dfh_lbfgs_calc_grad (DFH_ERR_STATE later); l1 < 0 or
 * NaN is DFH_ERR_ARG; l1 == 0 leaves the object as it is and allocates nothing: every launch and bit stays what it is
 * without the call.  l1 > 0 allocates two more model-sized vectors (the pseudo-gradient pg and the line search's origin
 * w0; DFH_ERR_CAPACITY with the bytes needed) and from then on, on the plain and the sharded object alike:
 *   prepare_direction  g stays the SMOOTH gradient g' = g_new + coef w and y_last = g' - g_old; pg is the pseudo-gradient
 *                      of g'; s_last = w - w0, the real displacement; incr_B has its layout with pg in g's place
 *   calc_direction     the Add chain over s, y, pg and the clamp, then on w elements p is kept only where it descends along
 *                      pg (else +0); *p_g = <pg, p>; w0 = w
 *   line_search        w = w0 + alpha p projected onto the orthant of w0 (of -pg where w0 is 0); *objv = F(w) and
 *                      *p_g = sum pg (w - w0), the term of the sufficient-decrease test F(w) <= F(w0) + c1 *p_g
 *   evaluate           r_w includes l1 sum |w| */
int dfh_lbfgs_set_l1(dfh_lbfgs* o, float l1);
/* out [nparams]: which 0 = the pseudo-gradient (after the first prepare_direction), 1 = w0 (after the first
 * calc_direction); only on an object with l1 > 0 */
int dfh_lbfgs_get_owlqn_vector(dfh_lbfgs* o, int which, float* out);
/* between prepare_direction and calc_direction: drop the newest (s, y) pair from both rings (a pair with <s, y> <= 0, which
 * a line search without the curvature test can produce); with no pair left calc_direction takes d = NULL: p = -pg */
int dfh_lbfgs_drop_last_pair(dfh_lbfgs* o);
/* elements the last line_search trial moved off w0, summed over the ranks (l1 > 0 only) */
int dfh_lbfgs_get_owlqn_moved(dfh_lbfgs* o, double* moved);

/* ------------------------------------------------ block coordinate descent (learner = bcd) */
/* The learner's state, resident in HBM from load to finish: the localized training and validation chunks (one dfh_batch
 * each) with their per-block layouts (a column-major slice for the gradient, a row-major slice for the prediction), the
 * predictions of every chunk and the model (keys ascending, w, delta, delta w).  Logistic loss, diagonal Newton steps
 * with l1 (src/bcd/).  One process, one GPU.  Data or state that does not fit in HBM fails with DFH_ERR_CAPACITY and the
 * bytes needed. */
typedef struct dfh_bcd dfh_bcd;
int dfh_bcd_create(dfh_ctx* ctx, dfh_bcd** out);
/* The same learner over the ranks of a communicator (RCCL or host callback; not the loop-back transport): each rank is a
 * worker for its own chunks (1/N of the rows) and, in every block step, the server of one slice of the block's keys, what
 * the reference's RunScheduler does with its worker and server groups (src/bcd/bcd_learner.cc:171-315,
 * bcd_updater.h:138-162).  The model is REPLICATED: every rank holds keys, w, delta and delta w of the whole model (12
 * bytes per key).  On such an object EVERY dfh_bcd_* call below is COLLECTIVE: every rank makes the same calls in the
 * same order with the same arguments apart from the chunks (a rank without rows adds no chunk and still takes part).
 *   build       the ranks exchange the (key, count) lists of their training chunks; a key's counts are added in
 *               ascending source rank and tail_feature_filter runs on the global counts, so every rank builds the same
 *               keys, block positions and colmaps (a key of other ranks' rows alone is a model key here too).
 *   epoch/step  per block, positions [pb, pe), n = pe - pb, slice r = [pb + floor(r n / W), pb + floor((r + 1) n / W)):
 *               the rank's partial g, h over its own chunks; the partials of slice p to rank p (all-to-all-v, 16 bytes
 *               per key); k_bcd_reduce adds each owned key's W partials in ascending source rank; the update on the
 *               owned slice; the slice's delta w to every peer (all-to-all-v, 4 bytes per key); k_bcd_apply stores w,
 *               delta and delta w of the other slices exactly as the update stored them; the predictions of the rank's
 *               own chunks.  A rank sends 16 (n - own) + 4 own (W - 1) bytes per block.  No float atomics: the model has
 *               the same bits on every rank, run and transport, and with one rank the bits of dfh_bcd_create's object.
 *               With the RCCL transport everything is queued on the context's stream and an epoch synchronises once.
 *   step's g, h the global sums (the owners' reduced slices, gathered: one more exchange), the same on every rank.
 *   progress    taken per local chunk, then summed over the ranks in rank order (dfh_comm_allreduce_sum).
 *   set_model   every rank passes the same input; nothing crosses the wire.
 * shape, block_info's positions and get_model see the whole model; block_info's entries and rows and get_pred see the
 * rank's own chunks.  DFH_ERR_CAPACITY applies per rank. */
int dfh_bcd_create_sharded(dfh_ctx* ctx, dfh_comm* comm, dfh_bcd** out);
int dfh_bcd_destroy(dfh_bcd* o);
/* a chunk of raw rows (Reader::Value()), localized on the device with Localizer(-1) (TileBuilder::Add) and kept */
int dfh_bcd_add_chunk(dfh_bcd* o, int is_val, size_t nrows, const size_t* offset, const uint64_t* index, const float* value,
                      const float* label);
/* BuildFeatureMap (bcd_learner.cc:118-169): merged training counts, keys with cnt > tail_feature_filter survive, w = 0,
 * delta = 1; nblk key ranges [blk_begin, blk_end) (ReverseBytes keys, sorted, disjoint: PartitionFeature) cut the keys
 * into blocks; every chunk's layouts are built on the device.  l1, lr: BCDUpdaterParam. */
int dfh_bcd_build(dfh_bcd* o, float tail_feature_filter, int nblk, const uint64_t* blk_begin, const uint64_t* blk_end, float l1,
                  float lr, uint64_t* nkeys);
int dfh_bcd_shape(dfh_bcd* o, uint64_t* nkeys, int* nblk, int* ntrain_chunks, int* nval_chunks);
/* block blk: its model positions [pos_begin, pos_end), its training entries and its touched rows (any pointer NULL) */
int dfh_bcd_block_info(dfh_bcd* o, int blk, int* pos_begin, int* pos_end, uint64_t* nnz, uint64_t* rows);
/* one epoch (IterateData, bcd_learner.cc:171-194): the blocks order[0 .. n-1] in turn, each gradient -> update -> the
 * predictions of every chunk, queued back to back; progress[4] = {count, LogitObjv, AUC x n, Accuracy(.5)} summed over
 * the training and validation chunks after the last block.  Synchronises once. */
int dfh_bcd_epoch(dfh_bcd* o, const int* order, int n, float* progress);
/* one block, synchronised: g, h (NULL: not returned) = the block's summed gradient and diagonal Hessian [pos_end -
 * pos_begin] in fp64 before the update; progress as dfh_bcd_epoch (NULL: not computed) */
int dfh_bcd_step(dfh_bcd* o, int blk, double* g, double* h, float* progress);
/* after dfh_bcd_build, before the first dfh_bcd_epoch / dfh_bcd_step: start from a model.
 * keys [n] (ReverseBytes keys as dfh_bcd_get_model returns them, unique, any order), w [n]: host arrays.
 * *n_matched (may be NULL): input keys that are keys of the model.
 * The keys are matched against the model's ascending keys on the device (one lane per input key, a binary search; no
 * host-side map).  An input key that is not in the model (filtered by tail_feature_filter, or never seen in the training
 * data) is dropped; a model key that is not in the input keeps w = 0; delta stays 1 and the last delta w stays 0, as
 * dfh_bcd_build leaves them.  Every call starts from the built state, so n = 0 leaves the object as built.
 * The predictions of EVERY training and validation chunk are rebuilt from the new w.  Definition, per row r:
 *     pred[r] = 0; for each surviving entry of the row whose key lies in a block, in ascending model position (ascending
 *     block, then ascending column inside the block): if (w != 0) pred[r] = pred[r] + w * x
 * in float, without contraction, x = 1 in a chunk without values — exactly what the block steps' own prediction update
 * computes from pred = 0 with delta w := w, block after block in ascending block order.  No float atomics: two calls
 * give the same bits.
 * Errors: DFH_ERR_STATE before dfh_bcd_build or after a step has run; DFH_ERR_ARG when the input keys are not unique
 * or w holds a non-finite value. */
int dfh_bcd_set_model(dfh_bcd* o, uint64_t n, const uint64_t* keys, const float* w, uint64_t* n_matched);
/* the model (any pointer may be NULL): keys [nkeys], merged counts, w, delta, the last delta w */
int dfh_bcd_get_model(dfh_bcd* o, uint64_t* keys, float* feacnt, float* w, float* delta, float* dw);
/* the predictions of a chunk (pred NULL: only *nrows) */
int dfh_bcd_get_pred(dfh_bcd* o, int is_val, int chunk, float* pred, size_t* nrows);

/* ------------------------------------------------ whole-set evaluation (exact_metrics = 1) */
/* BinClassMetric::AUC (src/loss/bin_class_metric.h:35-56) is taken per minibatch and averaged by the reference's learner, which
 * is not the AUC of the set.  A dfh_eval keeps every (label, prediction) row appended since the last reset in device memory
 * (8 B per row; the arrays grow by doubling, earlier content survives) and ranks them once (csrc/dfh_eval.hip).
 *   - a row is positive iff label > 0 (the reference's rule: a NaN label is negative); a row whose prediction is a NaN is
 *     counted in n_nan and takes part in nothing else; scores compare as floats (-0.0 == +0.0, +-inf are ordinary values)
 *   - auc2 is exact (an integer); AUC = auc2 / (2 n_pos n_neg), undefined when either count is 0 (then auc2 = 0)
 *   - objv is summed in fp64 in a fixed order, each term in the stable form max(-m, 0) + log1p(exp(-|m|)), m = y s; objv and
 *     correct cover the rows that are not counted in n_nan
 *   - the same appended sequence gives the same bits in every field on every run, however it was cut into appends
 * dfh_eval_append_batch queues a copy of the batch's nrows predictions and labels on the context's stream, behind the batch's
 * last step (dfh_sgd_step), and does not wait for the device; call it before the next minibatch is loaded into the batch
 * object (with pipelining on, that load waits for the copies: the call moves the object's `free` event behind them).
 * dfh_eval_append_host copies host arrays and returns when they are free.  An evaluator holds fewer than 2^32 - 16 rows (DFH_ERR_ARG); a failed allocation is DFH_ERR_CAPACITY with the
 * bytes needed in the message.  capacity_hint: the rows of the first allocation (0: 65 536).  dfh_eval_finish waits and covers
 * everything appended since the last reset; it changes nothing: more may be appended and a later finish covers all of it. */
typedef struct dfh_eval dfh_eval;
typedef struct {
  uint64_t n, n_pos, n_neg, n_nan;   /* n = n_pos + n_neg + n_nan                      */
  uint64_t auc2;                     /* 2 * #{(p,q): s_p > s_q} + #{(p,q): s_p == s_q}, p over the positives, q over the negatives */
  uint64_t correct;                  /* (label > 0 && s > 0) || (!(label > 0) && s <= 0) */
  double   objv;                     /* sum of log(1 + exp(-y s)), y = label > 0 ? 1 : -1 */
} dfh_eval_result;
int dfh_eval_create(dfh_ctx* ctx, size_t capacity_hint, dfh_eval** out);
int dfh_eval_destroy(dfh_eval* e);
int dfh_eval_reset(dfh_eval* e);
int dfh_eval_append_batch(dfh_eval* e, dfh_batch* b);
int dfh_eval_append_host(dfh_eval* e, const float* label, const float* pred, size_t n);
int dfh_eval_finish(dfh_eval* e, dfh_eval_result* out);

/* ------------------------------------------------ prediction text (pred_write = device) */
/* A dfh_predtext keeps every value appended since the last reset in device memory (4 B per value; the array grows by doubling,
 * earlier content survives) and turns them into the text fprintf("%.9g\n", v) writes for each, byte for byte, concatenated in
 * order (csrc/dfh_predtext.hip; the arithmetic, exact and integer only: csrc/dfh_predtext_fmt.h).
 *   - the device formats the REGULAR values: +0, -0 and the finite v with 2^-64 <= |v| < 2^32.  Every logit the FM forward
 *     clamps to +-20 is regular unless it is nonzero and below 5.4e-20, and so is every sigmoid of one.  Anything else
 *     (non-finite, tiny, huge, subnormal) is counted: dfh_predtext_format then reports irregular > 0, the text is not to be
 *     used, and the caller formats that set itself from dfh_predtext_values
 *   - a line has at most 16 bytes with its '\n'
 * capacity_hint: the values of the first allocation (0: 65 536).  The object holds fewer than 2^32 - 16 values (DFH_ERR_ARG); a
 * failed allocation is DFH_ERR_CAPACITY with the bytes needed in the message. */
typedef struct dfh_predtext dfh_predtext;
int dfh_predtext_create(dfh_ctx* ctx, size_t capacity_hint, dfh_predtext** out);
int dfh_predtext_destroy(dfh_predtext* p);
/* n = 0; the arrays stay */
int dfh_predtext_reset(dfh_predtext* p);
/* queues a copy of the batch's nrows predictions on the context's stream, behind the batch's last step (dfh_sgd_step), and does
 * not wait for the device; call it before the next minibatch is loaded into the batch object (with pipelining on, that load
 * waits for the copy: the call moves the object's `free` event behind it).  It may stand beside dfh_eval_append_batch on the
 * same batch, in either order. */
int dfh_predtext_append_batch(dfh_predtext* p, dfh_batch* b);
/* copies a host array and returns when it is free */
int dfh_predtext_append_host(dfh_predtext* p, const float* v, size_t n);
/* the values appended since the last reset */
int dfh_predtext_count(dfh_predtext* p, uint64_t* n);
/* the appended floats into out [count]; synchronises */
int dfh_predtext_values(dfh_predtext* p, float* out);
/* formats everything appended since the last reset: two launches and a scan between them, then ONE host round trip for
 * *nbytes (the text's length) and *irregular (the values the device does not format; > 0: the text is not valid).  It changes
 * nothing: more may be appended, and a later format covers all of it. */
int dfh_predtext_format(dfh_predtext* p, size_t* nbytes, uint64_t* irregular);
/* the text of the last format into dst [nbytes] (downloaded into page-locked memory of the object's, then copied); valid when
 * that format reported irregular == 0.  DFH_ERR_STATE when something was appended or reset since the last format. */
int dfh_predtext_read(dfh_predtext* p, char* dst);
/* the values a block of the format kernels takes: the text of a tile starts wherever the tile before it ends (for tests) */
int dfh_predtext_tile(void);

/* ------------------------------------------------ a model as sorted text (task = dump) */
/* A dfh_dump is a view of a table's KEPT entries (w != 0 || has_V: dfh_table_save's rule without aux) in ascending order of the
 * id they are printed under, and a formatter of their text (csrc/dfh_dumptext.hip; the arithmetic: csrc/dfh_predtext_fmt.h and
 * csrc/dfh_dumptext_fmt.h).  A line is "<id>\t<w>" and, when the entry has V, "\t<V_j>" for j = 0 .. V_dim - 1, then "\n": the
 * id as %llu, every float as %.9g; at most 20 + 16 (1 + V_dim) + 1 bytes.  No header line, no optimiser state.
 *   - ids_mode: DFH_DUMP_IDS_FEATURE prints reverse_bytes(key), the id as it stands in the user's data (the table stores the
 *     Localizer's reversed ids); DFH_DUMP_IDS_KEY prints the stored key.  Keys are unique, so the order, and with it every byte,
 *     is a function of the model alone: not of hash slots, capacity or import order
 *   - dfh_dump_open selects and sorts once (12 B of device memory per kept entry, twice that and the sort's workspace during
 *     the call); the rows are read in place afterwards.  The table must outlive the dump and stay unchanged while it is open
 *   - the device formats the REGULAR floats (+-0 and 2^-64 <= |v| < 2^32, see dfh_predtext above); a unit with any other value
 *     reports irregular > 0, its text is not to be used, and the caller formats the unit from dfh_dump_entries
 * Errors: DFH_ERR_ARG for NULL arguments, another ids_mode and first + count beyond the entries; DFH_ERR_CAPACITY for a failed
 * allocation, with the bytes needed in the message. */
enum { DFH_DUMP_IDS_FEATURE = 0, DFH_DUMP_IDS_KEY = 1 };
typedef struct dfh_dump dfh_dump;
int dfh_dump_open(dfh_table* t, int ids_mode, dfh_dump** out, uint64_t* n_entries);
int dfh_dump_close(dfh_dump* d);
/* the kept entries, those of them that have V, the table's V_dim (any pointer may be NULL) */
int dfh_dump_shape(dfh_dump* d, uint64_t* n_entries, uint64_t* n_with_V, int* V_dim);
/* formats entries [first, first + count) of the sorted list: two launches and a scan between them, then ONE host round trip
 * for *nbytes (the text's length) and *irregular (the values the device does not format; > 0: the text is not valid) */
int dfh_dump_format(dfh_dump* d, uint64_t first, size_t count, size_t* nbytes, uint64_t* irregular);
/* the text of the last format into dst [nbytes] (downloaded into page-locked memory of the object's, then copied); valid when
 * that format reported irregular == 0.  DFH_ERR_STATE before the first format. */
int dfh_dump_read(dfh_dump* d, char* dst);
/* the same entries as arrays: ids [count] as printed, w [count], has_V [count], V [count x V_dim] (zeros where !has_V; may be
 * NULL with V_dim = 0): for the host's formatting of a unit and for tests */
int dfh_dump_entries(dfh_dump* d, uint64_t first, size_t count, uint64_t* ids, float* w, int* has_V, float* V);
/* the entries a block of the format kernels takes, by the table's V_dim so that a tile's longest text fits the LDS image (for
 * tests; tiles count from the unit's first entry).  0: V_dim is above 2045, dfh_dump_format refuses (DFH_ERR_ARG) and the
 * entries are formatted on the host */
int dfh_dump_tile(dfh_dump* d);

/* raw device memory for hosts without a HIP runtime of their own */
int dfh_malloc(dfh_ctx* ctx, size_t bytes, void** dptr);
int dfh_free(dfh_ctx* ctx, void* dptr);
int dfh_memcpy_h2d(dfh_ctx* ctx, void* dst, const void* src, size_t bytes);
int dfh_memcpy_d2h(dfh_ctx* ctx, void* dst, const void* src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* DIFACTO_HIP_H_ */
