/**
 * batch_ring.h — the minibatch objects (dfh_batch) of the SGD worker loops behind one owner.  The learner keeps one ring for
 * its lifetime; jobs of the fused loop and of the sharded loop may follow one another on it in any order.  Two invariants
 * hold BETWEEN jobs, whichever loop ran last:
 *   1. every object the ring holds has the ring's common size (rows(), nnz()), and the objects are slots 0, 1, .. without a
 *      gap — "the first n are there and the block fits" is all the fused loop asks;
 *   2. no object has progress pending: every job drains what it stepped into its own record.
 * The fused loop keeps the first by construction (Grow re-creates ALL objects alike).  The sharded loop breaks it while it
 * runs — it grows one slot at a time, the others may hold minibatches in flight — and restores it at its end
 * (NormalizeSlots); at its start it must not build on objects that share one allocation (TakeOverForSlots).
 */
#ifndef DIFACTO_HOST_BATCH_RING_H_
#define DIFACTO_HOST_BATCH_RING_H_
#include <algorithm>
#include "./device_context.h"
#include "./sgd_utils.h"

namespace difacto {

class BatchRing {
 public:
  // The fused loop rotates kMax objects with the device feed: the reader delivers minibatches in bursts (ten at a time, when
  // a shuffle buffer becomes current) and the loop queues a whole burst on the device without waiting for any step — with two
  // or three objects the device idled while the loop waited for the reader and the loop waited while the device caught up
  static constexpr int kMax = 12;
  BatchRing() = default;
  BatchRing(const BatchRing&) = delete;
  ~BatchRing() {
    for (int q = 0; q < kMax; ++q) Destroy(q);
  }
  /*! \brief the slot of minibatch i in a rotation of n */
  static int SlotOf(int i, int n) { return i % n; }
  dfh_batch* operator[](int q) const { return s_[q].b; }
  int count() const { return static_cast<int>(std::count_if(s_, s_ + kMax, [](const Slot& s) { return s.b != nullptr; })); }
  /*! \brief the common size; the size of the object in slot q (0 without one) */
  size_t rows() const { return rows_; }
  size_t nnz() const { return nnz_; }
  size_t rows(int q) const { return s_[q].rows; }
  size_t nnz(int q) const { return s_[q].nnz; }
  /*! \brief does a block of that shape fit the object in slot q; ... every one of the first n */
  bool Fits(int q, size_t rows, size_t nnz) const { return s_[q].b && rows <= s_[q].rows && nnz <= s_[q].nnz; }
  bool AllFit(int n, size_t rows, size_t nnz) const {
    for (int q = 0; q < n; ++q)
      if (!Fits(q, rows, nnz)) return false;
    return true;
  }
  /*! \brief the fused loop: EVERY object goes (drained into *prog; none may be in flight) and n of one size take their
   *  place, rows = max(old, needed), nnz = max(old, 2 x needed) — out of one device allocation (dfh_batch_create_many):
   *  twelve objects used to be 12 x 61 hipMallocs, ~35 ms of a job's start-up */
  void Grow(dfh_ctx* ctx, int n, size_t rows, size_t nnz, sgd::Progress* prog) {
    CHECK(n >= 1 && n <= kMax);
    Drain(prog);
    for (int q = 0; q < kMax; ++q) Destroy(q);
    rows_ = std::max(rows, rows_);
    nnz_ = std::max(nnz * 2, nnz_);
    dfh_batch* made[kMax] = {};
    DFH_CALL(dfh_batch_create_many(ctx, n, rows_, std::max<size_t>(nnz_, 1), made));
    arena_ = true;
    for (int q = 0; q < n; ++q) Created(q, made[q], rows_, nnz_);
  }
  /*! \brief entry of the sharded loop, which rotates n slots and grows them one by one.  Objects carved from one allocation
   *  ALL go — the allocation lives as long as any of them, n survivors would pin twelve objects' worth of HBM — and so do
   *  objects beyond the n; objects of their own allocation stay, with their size */
  void TakeOverForSlots(int n, sgd::Progress* prog) {
    for (int q = arena_ ? 0 : n; q < kMax; ++q) Drain(q, prog), Destroy(q);
    arena_ = false;
  }
  /*! \brief the sharded loop: slot q alone is re-created (drained into *prog, which waits for its last step; the other
   *  slots may hold minibatches that have not stepped), at max(needed, its old size, the common size), nnz x 2 */
  void GrowSlot(dfh_ctx* ctx, int q, size_t rows, size_t nnz, sgd::Progress* prog) {
    CHECK(!arena_) << "TakeOverForSlots first";
    const size_t r = std::max(rows, std::max(s_[q].rows, rows_)), z = std::max(nnz * 2, std::max(s_[q].nnz, nnz_));
    Drain(q, prog);
    Destroy(q);
    dfh_batch* b = nullptr;
    DFH_CALL(dfh_batch_create(ctx, r, std::max<size_t>(z, 1), &b));
    Created(q, b, r, z);
  }
  /*! \brief end of a sharded job over n slots: every object drained, the common size becomes the largest slot's, objects of
   *  another size go and the survivors move to the front — invariant 1 again for whichever job runs next */
  void NormalizeSlots(int n, sgd::Progress* prog) {
    rows_ = nnz_ = 0;
    for (int q = 0; q < n; ++q) rows_ = std::max(rows_, s_[q].rows), nnz_ = std::max(nnz_, s_[q].nnz);
    for (int q = 0, w = 0; q < n; ++q) {
      Drain(q, prog);
      if (s_[q].rows != rows_ || s_[q].nnz != nnz_) Destroy(q);
      if (s_[q].b) std::swap(s_[q], s_[w++]);
    }
  }
  /*! \brief reads and resets the progress of the object in slot q (waits for its steps) and merges it into *prog (NULL:
   *  discarded); ... of every object, in slot order */
  void Drain(int q, sgd::Progress* prog) {
    if (!s_[q].b) return;
    dfh_progress p;
    DFH_CALL(dfh_batch_progress(s_[q].b, &p, 1));
    sgd::Progress m;
    m.loss = p.loss; m.penalty = p.penalty; m.auc = p.auc; m.nrows = p.nrows;
    if (prog) prog->Merge(m);
  }
  void Drain(sgd::Progress* prog) {
    for (int q = 0; q < kMax; ++q) Drain(q, prog);
  }

 private:
  struct Slot {
    dfh_batch* b = nullptr;
    size_t rows = 0, nnz = 0;
  };
  void Created(int q, dfh_batch* b, size_t rows, size_t nnz) {
    s_[q].b = b, s_[q].rows = rows, s_[q].nnz = nnz;
    DFH_CALL(dfh_batch_set_option(b, "compute_auc", 1));  // BinClassMetric::AUC of every minibatch, sgd_learner.cc:153-155
  }
  void Destroy(int q) {
    if (s_[q].b) dfh_batch_destroy(s_[q].b);
    s_[q] = Slot();
  }
  Slot s_[kMax];
  size_t rows_ = 0, nnz_ = 0;
  bool arena_ = false;   // the objects were carved from ONE device allocation, which is freed when the last of them goes
};

}  // namespace difacto
#endif  // DIFACTO_HOST_BATCH_RING_H_
