/**
 * device_feed.h — the SGD worker loop's device feed, host half: the reader's shuffle buffers in HBM (the device half is
 * csrc/dfh_feed.hip).  The reader thread uploads every buffer once, when it becomes current (BatchReader::Describe), into a
 * device row buffer; the worker loop then sends 4 B per row of a minibatch and the rows are gathered on the device
 * (dfh_batch_gather_rows) instead of being copied twice on the host (into the minibatch, into the pinned staging area).
 * Buffers are named by their serial: `live` holds every uploaded buffer that a minibatch may still name; the worker loop hands
 * a buffer back (Release) once the gather of the last minibatch that names it has been queued — with down-sampling
 * (neg_sampling < 1) one minibatch may span any number of buffers, so there is no fixed ring.  A buffer that is handed back is
 * reused by a later upload, which waits ON THE DEVICE for the gathers queued on it (dfh_rowbuf_load_host); buffers are freed on
 * the loop's thread, at the end of the job.
 */
#ifndef DIFACTO_HOST_DEVICE_FEED_H_
#define DIFACTO_HOST_DEVICE_FEED_H_
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include "./batch_reader.h"
#include "./device_context.h"
#include "./sgd_data_cache.h"
#include "./sgd_loop_env.h"

namespace difacto {

struct DeviceFeed {
  DeviceFeed(dfh_ctx* ctx, const SgdLoopEnv& env) : ctx(ctx), env(env) {}
  dfh_ctx* const ctx;
  const SgdLoopEnv env;
  std::mutex mu;
  std::condition_variable cv;
  std::map<uint64_t, dfh_rowbuf*> live;        // serial -> uploaded buffer
  std::vector<dfh_rowbuf*> spare;              // handed back
  struct Cap { size_t rows, nnz; };
  std::map<dfh_rowbuf*, Cap> owned;            // every buffer this feed has to destroy, with the size it was created for
  /*! \brief a new buffer of the feed's; the return code of dfh_rowbuf_create */
  int Create(size_t rows, size_t nnz, dfh_rowbuf** rb) {
    const int rc = dfh_rowbuf_create(ctx, rows, nnz, rb);
    if (rc != DFH_OK) return rc;
    std::lock_guard<std::mutex> lk(mu);
    owned[*rb] = Cap{rows, nnz};
    return rc;
  }
  void Disown(dfh_rowbuf* rb) { owned.erase(rb); }   // under mu: the buffer is somebody else's to destroy
  size_t num_owned() { std::lock_guard<std::mutex> lk(mu); return owned.size(); }
  size_t num_spare() { std::lock_guard<std::mutex> lk(mu); return spare.size(); }
  // A buffer's upload is queued by the thread that builds it, as soon as it exists — one buffer ahead of the one being cut
  // into minibatches (BatchReader's on_built) — and carried out by a few upload threads, each on the stream of the row
  // buffer it fills (one pageable copy per slice: ~1.4 ms per 31 MB buffer on one thread, more than the device needs for
  // the buffer's ten minibatches)
  struct Job {
    std::vector<size_t> offset;     // the buffer's own offsets (copied: the builder's container moves on)
    std::vector<real_t> label;      // (retain) the buffer's labels
    std::vector<BufSlice> slices;   // shared ownership of the parsed chunks
    uint64_t serial;
  };
  // data_cache = hbm (sgd_data_cache.h).  `cached`: the job reads a part that is in the cache — Of() names its buffers, nothing
  // is uploaded or handed back.  `retain`: the job fills the cache — every buffer gets an allocation of its own size and its
  // labels, and Release() moves it to `kept` instead of `spare`.  Before a buffer is retained its bytes are added to the part's;
  // when they exceed `budget` (or the allocation fails) the part is given up: what was kept goes to `spare` and the job goes on
  // as an uncached one does.
  const CachedPart* cached = nullptr;
  bool retain = false, overflow = false;
  size_t budget = ~static_cast<size_t>(0), kept_bytes = 0, need_bytes = 0, rows_seen = 0;
  std::map<uint64_t, CachedBuffer> desc, kept;   // serial -> retained buffer: still live / handed back
  static size_t BytesOf(size_t rows, size_t nnz) { return nnz * 12 + (rows + 1) * 4 + rows * 4; }   // dfh_rowbuf's arrays + labels
  void GiveUp() {   // under mu
    overflow = true;
    for (auto& k : kept) spare.push_back(k.second.rb);
    kept.clear();
    desc.clear();   // (their buffers are live: Release recycles them)
    kept_bytes = 0;
  }
  /*! \brief after the job's last minibatch: the part's buffers in order, or NULL (it did not fit) */
  std::unique_ptr<CachedPart> TakeCache() {
    StopWorkers();   // an upload nobody waited for (a buffer none of whose rows was drawn) ends here
    std::lock_guard<std::mutex> lk(mu);
    if (!retain || overflow) return nullptr;
    for (auto& l : live) {
      auto it = desc.find(l.first);
      CHECK(it != desc.end());
      kept.emplace(l.first, std::move(it->second));
    }
    live.clear();
    desc.clear();
    std::unique_ptr<CachedPart> part(new CachedPart());
    for (auto& k : kept) {
      CHECK_EQ(k.first, part->bufs.size() + 1) << "a shuffle buffer is missing from the cache";
      Disown(k.second.rb);
      part->rows += k.second.label.size();
      part->bytes += k.second.bytes;
      part->bufs.push_back(std::move(k.second));
    }
    kept.clear();
    return part;
  }
  void StopWorkers() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto& w : workers)
      if (w.joinable()) w.join();
  }
  std::deque<Job> jobs;
  std::vector<std::thread> workers;
  bool stop = false;
  // rows / nnz: what a shuffle buffer is expected to hold.  Every upload thread creates one row buffer of that size right
  // away — the buffer's arrays, its stream (a hardware queue: milliseconds) and events — while the reader is still parsing
  // the first chunks, instead of when the first shuffle buffer is already waiting for its upload (DIFACTO_FEED_PRECREATE=0:
  // as before).  A buffer that turns out too small stays spare and a fitting one is created then, as always.
  void Start(size_t rows, size_t nnz) {
    const bool precreate = rows > 0 && env.feed_precreate;
    for (int t = 0; t < env.upload_threads; ++t)
      workers.emplace_back([this, rows, nnz, precreate] {
        dfh_rowbuf* rb = nullptr;
        if (precreate && Create(rows, std::max<size_t>(nnz, 1), &rb) == DFH_OK) {
          std::lock_guard<std::mutex> lk(mu);
          spare.push_back(rb);
        }
        Work();
      });
  }
  void Upload(const dmlc::RowBlock<feaid_t>& blk, const std::vector<BufSlice>& slices, uint64_t serial) {   // builder's thread
    Job j;
    j.offset.assign(blk.offset, blk.offset + blk.size + 1);
    j.slices = slices;
    j.serial = serial;
    {
      std::lock_guard<std::mutex> lk(mu);
      rows_seen += blk.size;
      if (retain && !overflow) j.label.assign(blk.label, blk.label + blk.size);
      jobs.push_back(std::move(j));
    }
    cv.notify_all();
  }
  void Work() {
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !jobs.empty(); });
        if (jobs.empty()) return;
        j = std::move(jobs.front());
        jobs.pop_front();
      }
      DoUpload(j);
    }
  }
  void DoUpload(const Job& j) {
    const std::vector<BufSlice>& slices = j.slices;
    const uint64_t serial = j.serial;
    const size_t nrows = j.offset.size() - 1;
    const size_t nnz = j.offset[nrows] - j.offset[0];
    dfh_rowbuf* rb = nullptr;
    bool keep = false;
    const size_t bytes = BytesOf(std::max<size_t>(nrows, 1), std::max<size_t>(nnz, 1));
    if (retain) {   // a buffer that stays: an allocation of exactly its size, if the part still fits
      {
        std::lock_guard<std::mutex> lk(mu);
        need_bytes += bytes;
        if (!overflow && j.label.size() == nrows) {
          if (kept_bytes + bytes > budget) GiveUp(); else { keep = true; kept_bytes += bytes; }
        }
      }
      if (keep && Create(std::max<size_t>(nrows, 1), std::max<size_t>(nnz, 1), &rb) != DFH_OK) {
        rb = nullptr;   // no room on the device: the part streams
        keep = false;
        std::lock_guard<std::mutex> lk(mu);
        GiveUp();
      }
    }
    if (!rb) {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < spare.size() && !rb; ++i) {
        const Cap& c = owned.at(spare[i]);
        if (c.rows >= nrows && c.nnz >= nnz) {
          rb = spare[i];
          spare.erase(spare.begin() + i);
        }
      }
    }
    if (!rb) {   // none fits: a new one, in place of a spare that has proved too small (such buffers — ~58 MB and a stream
                 // each — used to stay until the feed was destroyed)
      dfh_rowbuf* small = nullptr;
      {
        std::lock_guard<std::mutex> lk(mu);
        if (!spare.empty()) {
          small = spare.back();
          spare.pop_back();
          Disown(small);
        }
      }
      if (small) DFH_CALL(dfh_rowbuf_destroy(small));   // waits for the gathers queued out of it, nothing else
      DFH_CALL(Create(std::max<size_t>(nrows, 1), std::max<size_t>(nnz + nnz / 4, 1), &rb));
    }
    std::vector<const uint64_t*> idx(slices.size());
    std::vector<const float*> val(slices.size());
    std::vector<size_t> cnt(slices.size());
    for (size_t g = 0; g < slices.size(); ++g) {
      idx[g] = slices[g].index();
      val[g] = slices[g].value();
      cnt[g] = slices[g].nnz();
    }
    bool any_device = false;
    for (const BufSlice& sl : slices) any_device = any_device || sl.device() != nullptr;
    if (any_device) {   // text_parse = device: those slices' ids are in HBM already
      std::vector<dfh_slice> mixed(slices.size());
      for (size_t g = 0; g < slices.size(); ++g)
        mixed[g] = dfh_slice{idx[g], val[g], static_cast<dfh_textchunk*>(slices[g].device()), slices[g].first(), cnt[g]};
      DFH_CALL(dfh_rowbuf_load_slices(rb, nrows, j.offset.data(), static_cast<int>(mixed.size()), mixed.data()));
    } else {
      DFH_CALL(dfh_rowbuf_load_host_slices(rb, nrows, j.offset.data(), static_cast<int>(slices.size()), idx.data(), val.data(), cnt.data()));
    }
    if (keep) DFH_CALL(dfh_rowbuf_set_labels(rb, nrows, j.label.data()));
    {
      std::lock_guard<std::mutex> lk(mu);
      CHECK(live.emplace(serial, rb).second) << "shuffle buffer " << serial << " uploaded twice";
      if (keep && !overflow) {
        CachedBuffer& d = desc[serial];
        d.rb = rb;
        d.offset.resize(nrows + 1);
        for (size_t i = 0; i <= nrows; ++i) d.offset[i] = j.offset[i] - j.offset[0];
        d.label = j.label;
        d.bytes = bytes;
      }
    }
    cv.notify_all();
  }
  dfh_rowbuf* Of(uint64_t serial) {   // on the worker loop's thread: waits for an upload still under way
    if (cached) {
      CHECK(serial >= 1 && serial <= cached->bufs.size()) << "minibatch names buffer " << serial << ", which the cache does not hold";
      return cached->bufs[serial - 1].rb;
    }
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return live.count(serial) != 0; });
    auto it = live.find(serial);
    CHECK(it != live.end()) << "minibatch names shuffle buffer " << serial << ", which is not (or no longer) on the device";
    return it->second;
  }
  // the gathers of every minibatch that names a buffer below `serial` have been queued
  void Release(uint64_t serial) {
    if (cached) return;
    std::lock_guard<std::mutex> lk(mu);
    while (!live.empty() && live.begin()->first < serial) {
      auto d = desc.find(live.begin()->first);
      if (d != desc.end()) {   // (retain, and the part still fits)
        kept.emplace(d->first, std::move(d->second));
        desc.erase(d);
      } else {
        spare.push_back(live.begin()->second);
      }
      live.erase(live.begin());
    }
  }
  ~DeviceFeed() {
    StopWorkers();
    for (auto& o : owned) dfh_rowbuf_destroy(o.first);
  }
};

}  // namespace difacto
#endif  // DIFACTO_HOST_DEVICE_FEED_H_
