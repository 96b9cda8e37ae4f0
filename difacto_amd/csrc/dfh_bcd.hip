// dfh_bcd.hip — the block coordinate descent learner's device side (included at the end of dfh_api.hip): the layouts
// of every data chunk per feature block, the kernels of one block step, and the dfh_bcd object that keeps the data, the
// predictions and the whole model (w, delta, delta w) resident in HBM.
//
// Restated from the reference (src/bcd/, src/loss/, src/common/):
//   CalcGrad              bcd_learner.cc:247-275, logit_loss_delta.h:90-146   k_bcd_grad + k_bcd_fixup, per training chunk
//                         p = -y / (1 + exp(y pred)), g += x p, h += x^2 (-p (y + p)): float terms, fp64 sums in a fixed order
//   BCDUpdater::UpdateWeight  bcd_updater.h:138-162, bcd_utils.h:146-165       k_bcd_update, float as written
//   UpdtPred / TransTimes     bcd_learner.cc:277-315, spmv.h:139-167           k_bcd_pred: pred_r += dw_j x_rj in float, columns
//                                                                              ascending, dw == 0 skipped
//   progress                  bcd_learner.cc:295-314, bin_class_metric.h:35-91 k_bcd_prog (objv, accuracy) + the AUC path
//
// Warm start (dfh_bcd_set_model; the reference declares model_in, bcd_param.h:44, and never reads it): the input keys are
// joined onto the model's ascending keys on the device (dfh_join.hip), matched keys take the input's w, every other key
// keeps w = 0, delta = 1 and delta w = 0 stay as dfh_bcd_build leaves them.  The predictions of every training and
// validation chunk are then rebuilt from w.  Definition, per row r:
//   pred[r] = 0.f; for every surviving entry of the row whose key lies in a block, in ascending model position
//   (ascending block, then ascending column inside the block): if (w != 0) pred[r] = pred[r] + w * x   (x = 1 in a
//   chunk without values), in float, without contraction
// which is what k_bcd_pred computes from pred = 0 with delta w := w, block after block in ascending block order: that
// is how it is done, so the bits are those of an epoch's own prediction updates.  No float atomics.
//
// Layouts of a chunk (built once, dfh_bcd_build), both cut into contiguous per-block slices:
//   column-major: the Localizer's key-ordered view (col_ptr, s_row, s_val) plus s_gk, the model position of every entry
//                 (-1: a filtered key); block b's entries are [nz[b].x, nz[b].y)
//   row-major:    the entries of the blocks' keys stably sorted by (block, row), so that a row's entries of one block are
//                 contiguous and in ascending column order: r_key (model position), r_val; one record per touched
//                 (block, row) pair: rec_row, rec_lo (the record's entries are [rec_lo[i], rec_lo[i + 1])); block b's
//                 records are [rec[b], rec[b + 1])
// Neither pass needs atomics.  The block id of a launch is read from a device-side order array, so that an epoch's
// launches are queued back to back on one stream; every launch of a chunk has the grid of its largest block.
//
// Over the ranks of a communicator (dfh_bcd_create_sharded; the reference's workers and servers, bcd_learner.cc:171-315):
// every rank keeps its own rows and the whole model.  The positions of a block are cut into `world` slices, rank r the
// "server" of slice r.  One block step: the rank's partial g, h over its own chunks (k_bcd_grad + k_bcd_fixup) -> every
// slice's partials to its owner (all-to-all-v) -> k_bcd_reduce adds a key's partials in ascending source rank ->
// k_bcd_update on the owned slice -> the slice's delta w to every peer (all-to-all-v) -> k_bcd_apply stores w, delta,
// delta w of the other slices as k_bcd_update stored them -> k_bcd_pred over the rank's own chunks.  No float atomics: the
// model has the same bits on every rank, run and transport.
#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace dfh {
namespace bcd {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int STEPS = 2;                     // 64-entry steps per wave share: 128 entries, enough waves per CU for the gathers
constexpr uint32_t SHARE = 64u * STEPS;      // entries of one share of a block's column-major slice
constexpr int NONE = -2;                     // slab: no partial
constexpr int PROG_BLOCKS = 256;

struct Slab {          // per share: the partial of the key it continues (first) and of the key it hands on (last)
  int* fk;
  double* fg;
  double* fh;
  int* lk;
  double* lg;
  double* lh;
};

struct GradArgs {
  const int* order;      // block order of the epoch
  int at;                // position in order
  const uint2* nz;       // [nblk] column-major slice of each block in this chunk
  const int* pbeg;       // [nblk] first model position of each block
  const int* s_gk;       // [nnz] model position per entry, key order
  const uint32_t* s_row; // [nnz]
  const float* s_val;    // [nnz] or NULL
  const float* pred;     // [nrows]
  const float* label;    // [nrows]
  double* gacc;          // [max keys per block] g, block-local position
  double* hacc;
  Slab slab;
};

__device__ __forceinline__ double shfl_up_d(double v, int d) { return __shfl_up(v, d, 64); }

// CalcGrad of one chunk for block order[at]: wave w takes entries [a, a + SHARE) of the block's slice in steps of 64, a
// segmented inclusive scan by key across the lanes (fixed order) carried from step to step.  A key whose entries all lie
// in this share is added to gacc / hacc by this wave alone; the partials of a key that crosses a share boundary go to the
// slab, and k_bcd_fixup adds them up in share order.
__global__ void __launch_bounds__(THREADS) k_bcd_grad(GradArgs A) {
  const int blk = A.order[A.at];
  const uint2 nz = A.nz[blk];
  const int lane = threadIdx.x & 63;
  const uint32_t share = blockIdx.x * WAVES + (threadIdx.x >> 6);
  const uint64_t a64 = (uint64_t)nz.x + (uint64_t)share * SHARE;
  if (a64 >= nz.y) return;
  const uint32_t a = (uint32_t)a64, b = (uint32_t)min<uint64_t>(a64 + SHARE, nz.y);
  const int pb = A.pbeg[blk];
  const int key0 = A.s_gk[a];
  const bool first_before = a > nz.x && A.s_gk[a - 1] == key0;       // key0 began in an earlier share
  const bool last_after = b < nz.y && A.s_gk[b] == A.s_gk[b - 1];    // the last key goes on in a later share
  const int key_last = A.s_gk[b - 1];
  int ckey = NONE;
  double cg = 0.0, ch = 0.0;
  // the slab cells no lane of this share writes below are cleared (each cell has one writer)
  if (lane == 0) {
    if (!(first_before && key0 >= 0)) A.slab.fk[share] = NONE;
    if (!(last_after && key_last >= 0 && !(key_last == key0 && first_before))) A.slab.lk[share] = NONE;
  }
  for (uint32_t e0 = a; e0 < b; e0 += 64) {
    const uint32_t e = e0 + lane;
    const bool valid = e < b;
    int key = valid ? A.s_gk[e] : -3 - lane;   // invalid lanes: a key of their own
    double vg = 0.0, vh = 0.0;
    if (valid && key >= 0) {
      const uint32_t r = A.s_row[e];
      const float y = A.label[r] > 0 ? 1.f : -1.f;
      const float p = -y / (1.f + expf(y * A.pred[r]));   // logit_loss_delta.h:101-104
      const float t = -p * (y + p);                       // :126-130, tau (1 - tau)
      if (A.s_val) {
        const float x = A.s_val[e];
        vg = (double)(p * x);
        vh = (double)(t * (x * x));
      } else {
        vg = (double)p;
        vh = (double)t;
      }
    }
    // the carry of the previous step joins lane 0's segment first
    if (lane == 0 && key == ckey) {
      vg = cg + vg;
      vh = ch + vh;
    }
    const int kprev = __shfl_up(key, 1, 64);
    int f = (lane == 0 || kprev != key) ? 1 : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double ug = shfl_up_d(vg, d), uh = shfl_up_d(vh, d);
      const int uf = __shfl_up(f, d, 64);
      if (lane >= d) {
        if (!f) {
          vg = ug + vg;
          vh = uh + vh;
        }
        f |= uf;
      }
    }
    int knext = __shfl_down(key, 1, 64);
    if (lane == 63) knext = e + 1 < b ? A.s_gk[e + 1] : NONE;
    const bool tail = valid && (knext != key || e + 1 >= b);
    if (tail && key >= 0) {
      const bool is_end = e + 1 >= b;               // the share's last entry
      const bool begins_before = key == key0 && first_before;
      const bool goes_on = is_end && last_after;
      if (!begins_before && !goes_on) {
        A.gacc[key - pb] += vg;
        A.hacc[key - pb] += vh;
      } else if (begins_before) {                    // also when it goes on: the chain runs through this share
        A.slab.fk[share] = key;
        A.slab.fg[share] = vg;
        A.slab.fh[share] = vh;
      } else {
        A.slab.lk[share] = key;
        A.slab.lg[share] = vg;
        A.slab.lh[share] = vh;
      }
    }
    // carry lane 63 into the next step
    ckey = __shfl(key, 63, 64);
    cg = __shfl(vg, 63, 64);
    ch = __shfl(vh, 63, 64);
  }
}

// the keys that cross share boundaries: the wave of the share where such a key begins adds its partial and those of
// the following shares (their "first" partials, in share order, 64 at a time through a fixed butterfly) to gacc / hacc
__global__ void __launch_bounds__(THREADS) k_bcd_fixup(GradArgs A) {
  const int blk = A.order[A.at];
  const uint2 nz = A.nz[blk];
  const int lane = threadIdx.x & 63;
  const uint32_t share = blockIdx.x * WAVES + (threadIdx.x >> 6);
  const uint64_t nshares = ((uint64_t)nz.y - nz.x + SHARE - 1) / SHARE;
  if (share >= nshares) return;
  const int key = A.slab.lk[share];
  if (key < 0) return;
  double g = A.slab.lg[share], h = A.slab.lh[share];
  for (uint64_t t0 = share + 1; t0 < nshares; t0 += 64) {
    const uint64_t t = t0 + lane;
    const bool m = t < nshares && A.slab.fk[t] == key;
    const uint64_t ball = __ballot(m);
    const int len = ball == ~0ULL ? 64 : __builtin_ctzll(~ball);   // the chain is a prefix of the shares
    double vg = lane < len ? A.slab.fg[t] : 0.0, vh = lane < len ? A.slab.fh[t] : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      vg += __shfl_xor(vg, o, 64);
      vh += __shfl_xor(vh, o, 64);
    }
    g += vg;
    h += vh;
    if (len < 64) break;
  }
  if (lane == 0) {
    const int pb = A.pbeg[blk];
    A.gacc[key - pb] += g;
    A.hacc[key - pb] += h;
  }
}

struct UpdArgs {
  const int* order;
  int at;
  const int* pbeg;
  const int* pend;
  double* gacc;
  double* hacc;
  float* w;
  float* delta;
  float* dw;
  float l1, lr;
  int zero;    // clear gacc / hacc for the next block
  int lo, hi;  // the block-local positions [lo, hi) this launch updates (a plain object: the whole block)
};

// BCDUpdater::UpdateWeight (bcd_updater.h:138-162) on the block's summed g, h, then bcd::Delta::Update (bcd_utils.h:158-163)
__global__ void __launch_bounds__(THREADS) k_bcd_update(UpdArgs A) {
  const int blk = A.order[A.at];
  const int pb = A.pbeg[blk], n = A.pend[blk] - pb;
  const int k = A.lo + blockIdx.x * THREADS + threadIdx.x;
  if (k >= n || k >= A.hi) return;
  const float g = (float)A.gacc[k];
  const float hh = (float)A.hacc[k];
  if (A.zero) {
    A.gacc[k] = 0.0;
    A.hacc[k] = 0.0;
  }
  const float g_pos = g + A.l1, g_neg = g - A.l1;
  const float u = (float)((double)(hh / A.lr) + 1e-10);
  const float w = A.w[pb + k];
  const float dl = A.delta[pb + k];
  float d = -w;
  const float uw = u * w;
  if (g_pos <= uw) {
    d = -g_pos / u;
  } else if (g_neg >= uw) {
    d = -g_neg / u;
  }
  const float lo = -dl;
  d = (d < lo) ? lo : d;       // std::max(-delta, d)
  d = (dl < d) ? dl : d;       // std::min(delta, .)
  const float nd = (float)((double)fabsf(d) * 2.0 + .1);
  A.delta[pb + k] = (nd < 5.f) ? nd : 5.f;   // std::min(max_val, .)
  A.w[pb + k] = w + d;
  A.dw[pb + k] = d;
}

// sharded: the owner of slice [lo, lo + own) of a block's n keys adds the W partials of each of its keys (xg / xh: [W][own],
// source rank major) in ascending source rank, starting from rank 0's value, and writes gacc / hacc of the slice once;
// the other slices are cleared for the next block's k_bcd_grad
__global__ void __launch_bounds__(THREADS) k_bcd_reduce(const double* __restrict__ xg, const double* __restrict__ xh, int W, int n,
                                                        int lo, int own, double* __restrict__ gacc, double* __restrict__ hacc) {
  const int k = blockIdx.x * THREADS + threadIdx.x;
  if (k >= n) return;
  double g = 0.0, h = 0.0;
  const int j = k - lo;
  if (j >= 0 && j < own) {
    g = xg[j];
    h = xh[j];
    for (int p = 1; p < W; ++p) {
      g += xg[(size_t)p * own + j];
      h += xh[(size_t)p * own + j];
    }
  }
  gacc[k] = g;
  hacc[k] = h;
}

// sharded: the keys of the slices this rank does not own take the step d their owners computed (xd: the block's n steps
// in position order): exactly the three stores of k_bcd_update
__global__ void __launch_bounds__(THREADS) k_bcd_apply(const float* __restrict__ xd, int n, int lo, int hi, int pb,
                                                       float* __restrict__ w, float* __restrict__ delta, float* __restrict__ dw) {
  const int k = blockIdx.x * THREADS + threadIdx.x;
  if (k >= n || (k >= lo && k < hi)) return;
  const float d = xd[k];
  const float nd = (float)((double)fabsf(d) * 2.0 + .1);
  delta[pb + k] = (nd < 5.f) ? nd : 5.f;
  w[pb + k] = w[pb + k] + d;
  dw[pb + k] = d;
}

struct PredArgs {
  const int* order;
  int at;
  const uint32_t* rec;      // [nblk + 1]
  const uint32_t* rec_row;  // [nrec]
  const uint32_t* rec_lo;   // [nrec + 1]
  const int* r_key;         // [m]
  const float* r_val;       // [m] or NULL
  const float* dw;
  float* pred;
};

// UpdtPred (TransTimes, spmv.h:139-167): one lane per touched row; the adds go into a float that starts at pred_r, in
// ascending column order, dw == 0 skipped — the reference's float order, bit for bit
__global__ void __launch_bounds__(THREADS) k_bcd_pred(PredArgs A) {
  const int blk = A.order[A.at];
  const uint32_t r0 = A.rec[blk], r1 = A.rec[blk + 1];
  const uint64_t i = (uint64_t)r0 + (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= r1) return;
  const uint32_t row = A.rec_row[i], lo = A.rec_lo[i], hi = A.rec_lo[i + 1];
  float acc = A.pred[row];
  for (uint32_t q = lo; q < hi; ++q) {
    const float x = A.dw[A.r_key[q]];
    if (x == 0.f) continue;
    if (A.r_val) acc = acc + x * A.r_val[q];
    else acc = acc + x;
  }
  A.pred[row] = acc;
}

// LogitObjv and Accuracy(.5) of a chunk (bin_class_metric.h:50-91): per-thread fp64 sums, a fixed-order block reduction
// into part[block][2]; k_bcd_prog_finish adds the blocks in order into out[0..1]
__global__ void __launch_bounds__(THREADS) k_bcd_prog(const float* __restrict__ pred, const float* __restrict__ label, uint32_t n,
                                                      double* __restrict__ part) {
  __shared__ double sh[2][WAVES];
  double o = 0.0, c = 0.0;
  for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < n; i += gridDim.x * THREADS) {
    const float p = pred[i], l = label[i];
    const double y = l > 0 ? 1.0 : -1.0;
    o += log(1.0 + exp(-y * (double)p));
    if ((l > 0 && p > .5f) || (l <= 0 && p <= .5f)) c += 1.0;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    o += __shfl_xor(o, s, 64);
    c += __shfl_xor(c, s, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = o;
    sh[1][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double so = 0.0, sc = 0.0;
    for (int w = 0; w < WAVES; ++w) {
      so += sh[0][w];
      sc += sh[1][w];
    }
    part[2 * blockIdx.x] = so;
    part[2 * blockIdx.x + 1] = sc;
  }
}

__global__ void k_bcd_prog_finish(const double* __restrict__ part, int nparts, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double o = 0.0, c = 0.0;
  for (int i = 0; i < nparts; ++i) {
    o += part[2 * i];
    c += part[2 * i + 1];
  }
  out[0] = o;
  out[1] = c;
}

// warm start: the matched input keys' w into the model (pos from the key join; input keys are unique: one writer per w)
__global__ void __launch_bounds__(THREADS) k_bcd_set_w(const int32_t* __restrict__ pos, const float* __restrict__ win, uint64_t n,
                                                       float* __restrict__ w) {
  const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t p = pos[i];
  if (p >= 0) w[p] = win[i];
}

// ---- layout build (once per chunk)
// per entry of the key-ordered view: its column (binary search in col_ptr), its model position and the sort key
// (block << 32 | row) of the row-major layout (~0: a filtered key or a key in no block, sorted behind everything)
__global__ void __launch_bounds__(THREADS) k_bcd_entries(const uint32_t* __restrict__ col_ptr, uint32_t U, uint32_t nnz,
                                                         const uint32_t* __restrict__ s_row, const int* __restrict__ gmap,
                                                         const int* __restrict__ cblk, int* __restrict__ s_gk,
                                                         uint64_t* __restrict__ skey, uint32_t* __restrict__ perm) {
  const uint64_t e64 = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (e64 >= nnz) return;
  const uint32_t e = (uint32_t)e64;
  uint32_t lo = 0, hi = U;   // the last u with col_ptr[u] <= e
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (col_ptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  s_gk[e] = gmap[lo];
  const int b = cblk[lo];
  skey[e] = b >= 0 ? ((uint64_t)(uint32_t)b << 32 | s_row[e]) : ~0ULL;
  perm[e] = e;
}

// the row-major arrays out of the sorted order, and a 1 at the head of every (block, row) record
__global__ void __launch_bounds__(THREADS) k_bcd_rowmajor(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm,
                                                          uint32_t m, const int* __restrict__ s_gk, const float* __restrict__ s_val,
                                                          int* __restrict__ r_key, float* __restrict__ r_val,
                                                          uint32_t* __restrict__ head) {
  const uint64_t q64 = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (q64 >= m) return;
  const uint32_t q = (uint32_t)q64, e = perm[q];
  r_key[q] = s_gk[e];
  if (r_val) r_val[q] = s_val[e];
  head[q] = (q == 0 || skey[q] != skey[q - 1]) ? 1u : 0u;
}

// records: the inclusive scan of the heads numbers them
__global__ void __launch_bounds__(THREADS) k_bcd_records(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ head,
                                                         const uint32_t* __restrict__ idx, uint32_t m, uint32_t* __restrict__ rec_row,
                                                         uint32_t* __restrict__ rec_lo) {
  const uint64_t q64 = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
  if (q64 >= m) return;
  const uint32_t q = (uint32_t)q64;
  if (q == m - 1) rec_lo[idx[q]] = m;
  if (!head[q]) return;
  const uint32_t i = idx[q] - 1;
  rec_row[i] = (uint32_t)skey[q];
  rec_lo[i] = q;
}

// rec[b] = the first record of block b (or later): a binary search over the records' blocks
__global__ void __launch_bounds__(THREADS) k_bcd_rec_begin(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ rec_lo,
                                                           uint32_t nrec, int nblk, uint32_t* __restrict__ rec) {
  const int b = blockIdx.x * THREADS + threadIdx.x;
  if (b > nblk) return;
  uint32_t lo = 0, hi = nrec;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((int)(skey[rec_lo[mid]] >> 32) < b) lo = mid + 1;
    else hi = mid;
  }
  rec[b] = lo;
}

inline int grid_of(uint64_t n, int per_block) { return (int)std::max<uint64_t>(1, (n + per_block - 1) / per_block); }

}  // namespace bcd
}  // namespace dfh

#pragma clang fp contract(fast)

struct dfh_bcd {
  dfh_ctx* ctx = nullptr;
  struct Chunk : chunks::Resident {
    // device layout
    int* s_gk = nullptr;          // [nnz]
    uint2* nz = nullptr;          // [nblk]
    int* r_key = nullptr;         // [m]
    float* r_val = nullptr;       // [m] or NULL
    uint32_t* rec = nullptr;      // [nblk + 1]
    uint32_t* rec_row = nullptr;  // [nrec]
    uint32_t* rec_lo = nullptr;   // [nrec + 1]
    uint32_t m = 0, nrec = 0;
    uint32_t max_nz = 0, max_rec = 0;   // largest block slice: the grids of the chunk's launches
  };
  std::vector<Chunk> chunks[2];   // [0] training, [1] validation
  bool built = false;
  bool stepped = false;           // a block step has run: the model can no longer be replaced
  int nblk = 0;
  float l1 = 1, lr = .9f;
  std::vector<uint64_t> keys;     // the model's keys (filtered, ascending)
  std::vector<float> cnts;
  std::vector<int> pbeg, pend;    // model positions of every block
  int max_keys = 0;
  int* d_pbeg = nullptr;
  int* d_pend = nullptr;
  float *d_w = nullptr, *d_delta = nullptr, *d_dw = nullptr;
  double *d_gacc = nullptr, *d_hacc = nullptr;
  bcd::Slab slab{};
  void* slab_mem = nullptr;
  int* d_order = nullptr;
  std::vector<int> h_order;
  double* d_part = nullptr;       // [PROG_BLOCKS][2]
  double* d_res = nullptr;        // [chunks][4] {objv, correct, auc x n, -}
  size_t res_cap = 0;
  // ---- sharded (dfh_bcd_create_sharded): a worker for its own chunks, the server of one slice of every block
  dfh_comm* comm = nullptr;
  int max_slice = 0;              // keys of the largest slice of any block
  double *d_xg = nullptr, *d_xh = nullptr;   // [world][max_slice] the partials of the own slice, source rank major
  float* d_xd = nullptr;          // [max_keys] the block's delta w as the owners sent it
  std::vector<size_t> xsb, xso, xrb, xsb4, xrb4, xzero;   // bytes and offsets per peer of the block under way
  // slice p of a block of n keys: block-local positions [slice(p, n), slice(p + 1, n))
  int slice(int p, int n) const { return (int)((long long)p * n / comm->world); }
};

namespace {

constexpr const char* kBcdWho = "dfh_bcd";
constexpr const char* kBcdTail = "out-of-core BCD is not supported";

// device bytes a chunk's layouts keep (m <= nnz entries, records <= nnz) and the transient build buffers
inline size_t bcd_layout_bytes(size_t nnz, int nblk, bool val) {
  return nnz * (sizeof(int) + sizeof(int) + (val ? 4 : 0) + 2 * sizeof(uint32_t)) + (size_t)(nblk + 2) * 16 + 1024;
}
inline size_t bcd_build_bytes(size_t nnz, size_t sort_tmp) { return nnz * (8 + 8 + 4 + 4 + 4 + 4) + sort_tmp + 1024; }

// sharded, between the gradient and the predictions of block h_order[at]: the slices' partials to their owners, the sums
// in rank order, the update of the owned slice, its delta w to every peer, the peers' slices applied.  Byte counts come
// from pbeg / pend on the host; with the RCCL transport everything is queued on the context's stream.  A block without
// keys exchanges nothing (every rank knows it).
int bcd_block_servers(dfh_bcd* o, int at, int zero) {
  hipStream_t s = o->ctx->stream;
  const int blk = o->h_order[at];
  const int pb = o->pbeg[blk], n = o->pend[blk] - pb;
  if (!n) return DFH_OK;
  const int W = o->comm->world, r = o->comm->rank;
  const int lo = o->slice(r, n), hi = o->slice(r + 1, n), own = hi - lo;
  for (int p = 0; p < W; ++p) {
    const size_t np = (size_t)(o->slice(p + 1, n) - o->slice(p, n));
    o->xsb[p] = np * sizeof(double);                       // slice p's partials to rank p
    o->xso[p] = (size_t)o->slice(p, n) * sizeof(double);
    o->xrb[p] = (size_t)own * sizeof(double);              // every rank's partials of the own slice
    o->xsb4[p] = (size_t)own * sizeof(float);              // the own slice's delta w to every rank
    o->xrb4[p] = np * sizeof(float);                       // every slice's delta w, in position order
  }
  const XPart gh[2] = {{o->d_gacc, o->xsb.data(), o->xso.data(), o->d_xg, o->xrb.data(), nullptr},
                       {o->d_hacc, o->xsb.data(), o->xso.data(), o->d_xh, o->xrb.data(), nullptr}};
  int rc = comm_exchange(o->comm, gh, 2, nullptr, DFH_XCHG_GRADS);
  if (rc) return rc;
  const dim3 grid(bcd::grid_of(n, bcd::THREADS)), block(bcd::THREADS);
  hipLaunchKernelGGL(bcd::k_bcd_reduce, grid, block, 0, s, o->d_xg, o->d_xh, W, n, lo, own, o->d_gacc, o->d_hacc);
  if (own) {
    bcd::UpdArgs u{o->d_order, at, o->d_pbeg, o->d_pend, o->d_gacc, o->d_hacc, o->d_w, o->d_delta, o->d_dw, o->l1, o->lr, zero, lo, hi};
    hipLaunchKernelGGL(bcd::k_bcd_update, dim3(bcd::grid_of(own, bcd::THREADS)), block, 0, s, u);
  }
  DFH_HIP(hipGetLastError());
  const XPart d{o->d_dw + pb + lo, o->xsb4.data(), o->xzero.data(), o->d_xd, o->xrb4.data(), nullptr};
  rc = comm_exchange(o->comm, &d, 1, nullptr, DFH_XCHG_ROWS);
  if (rc) return rc;
  if (own < n) {
    hipLaunchKernelGGL(bcd::k_bcd_apply, grid, block, 0, s, o->d_xd, n, lo, hi, pb, o->d_w, o->d_delta, o->d_dw);
    DFH_HIP(hipGetLastError());
  }
  return DFH_OK;
}

// sharded, dfh_bcd_step's g and h: the owners' reduced slices of block blk gathered into d_xg / d_xh in position order
int bcd_gather_gh(dfh_bcd* o, int blk) {
  const int n = o->pend[blk] - o->pbeg[blk];
  if (!n) return DFH_OK;
  const int W = o->comm->world, r = o->comm->rank;
  const int lo = o->slice(r, n), own = o->slice(r + 1, n) - lo;
  for (int p = 0; p < W; ++p) {
    o->xsb[p] = (size_t)own * sizeof(double);
    o->xrb[p] = (size_t)(o->slice(p + 1, n) - o->slice(p, n)) * sizeof(double);
  }
  const XPart gh[2] = {{o->d_gacc + lo, o->xsb.data(), o->xzero.data(), o->d_xg, o->xrb.data(), nullptr},
                       {o->d_hacc + lo, o->xsb.data(), o->xzero.data(), o->d_xh, o->xrb.data(), nullptr}};
  return comm_exchange(o->comm, gh, 2, nullptr, DFH_XCHG_GRADS);
}

// sharded, set-up: every rank's n[p] elements of `elem` host bytes to every rank, in rank order; synchronous (the
// host-staged exchange of dfh_comm.hip, transient buffers; one send buffer for every peer: offsets all zero)
int bcd_allgatherv(dfh_bcd* o, const void* mine, size_t elem, const std::vector<uint64_t>& n, void* all) {
  const int W = o->comm->world;
  std::vector<size_t> sb(W, (size_t)n[o->comm->rank] * elem), so(W, 0), rb(W);
  for (int p = 0; p < W; ++p) rb[p] = (size_t)n[p] * elem;
  return HostXchg{o->comm, "dfh_bcd_build", HostXchg::TRANSIENT}.exchange(mine, sb.data(), so.data(), all, rb.data(), DFH_XCHG_KEYS);
}

// one block (order[at]) over every chunk: the gradient over the training chunks, the update, the predictions of every chunk
int bcd_block(dfh_bcd* o, int at, int zero) {
  hipStream_t s = o->ctx->stream;
  bcd::GradArgs g{};
  g.order = o->d_order;
  g.at = at;
  g.pbeg = o->d_pbeg;
  g.gacc = o->d_gacc;
  g.hacc = o->d_hacc;
  g.slab = o->slab;
  for (auto& ch : o->chunks[0]) {
    if (!ch.max_nz) continue;
    g.nz = ch.nz;
    g.s_gk = ch.s_gk;
    g.s_row = ch.b->d_s_row;
    g.s_val = ch.b->has_value ? ch.b->d_s_val : nullptr;
    g.pred = ch.b->d_pred;
    g.label = ch.b->d_label;
    const uint64_t shares = (ch.max_nz + bcd::SHARE - 1) / bcd::SHARE;
    const int grid = bcd::grid_of(shares, bcd::WAVES);
    hipLaunchKernelGGL(bcd::k_bcd_grad, dim3(grid), dim3(bcd::THREADS), 0, s, g);
    hipLaunchKernelGGL(bcd::k_bcd_fixup, dim3(grid), dim3(bcd::THREADS), 0, s, g);
  }
  DFH_HIP(hipGetLastError());
  if (o->comm) {
    const int rc = bcd_block_servers(o, at, zero);
    if (rc) return rc;
  } else if (o->max_keys) {
    bcd::UpdArgs u{o->d_order, at, o->d_pbeg, o->d_pend, o->d_gacc, o->d_hacc, o->d_w, o->d_delta, o->d_dw, o->l1, o->lr, zero,
                   0, INT_MAX};
    hipLaunchKernelGGL(bcd::k_bcd_update, dim3(bcd::grid_of(o->max_keys, bcd::THREADS)), dim3(bcd::THREADS), 0, s, u);
  }
  for (auto& cs : o->chunks)
    for (auto& ch : cs) {
      if (!ch.max_rec) continue;
      bcd::PredArgs p{o->d_order, at, ch.rec, ch.rec_row, ch.rec_lo, ch.r_key, ch.r_val, o->d_dw, ch.b->d_pred};
      hipLaunchKernelGGL(bcd::k_bcd_pred, dim3(bcd::grid_of(ch.max_rec, bcd::THREADS)), dim3(bcd::THREADS), 0, s, p);
    }
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// the progress of every chunk, training then validation: {count, LogitObjv, AUC x n, Accuracy(.5)} summed in float in
// chunk order, as the reference's progress vector sums them (bcd_learner.cc:303-314)
int bcd_progress(dfh_bcd* o, float* prog) {
  hipStream_t s = o->ctx->stream;
  size_t i = 0;
  for (auto& cs : o->chunks)
    for (auto& ch : cs) {
      double* res = o->d_res + 4 * i++;
      const int nb = std::min<int>(bcd::PROG_BLOCKS, bcd::grid_of(ch.nrows, bcd::THREADS));
      hipLaunchKernelGGL(bcd::k_bcd_prog, dim3(nb), dim3(bcd::THREADS), 0, s, ch.b->d_pred, ch.b->d_label, (uint32_t)ch.nrows,
                         o->d_part);
      hipLaunchKernelGGL(bcd::k_bcd_prog_finish, dim3(1), dim3(64), 0, s, o->d_part, nb, res);
      DFH_HIP(hipGetLastError());
      int rc = launch_auc(ch.b);
      if (rc) return rc;
      DFH_HIP(hipMemcpyAsync(res + 2, ch.b->d_prog + PROG_AUC * PROG_SLOTS, sizeof(double), hipMemcpyDeviceToDevice, s));
      DFH_HIP(chunks::reset_prog(ch.b, s));
    }
  std::vector<double> r(4 * i);
  if (i) DFH_HIP(hipMemcpyAsync(r.data(), o->d_res, r.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  float v[4] = {0, 0, 0, 0};
  i = 0;
  for (auto& cs : o->chunks)
    for (auto& ch : cs) {
      const float n = (float)ch.nrows;
      const float correct = (float)r[4 * i + 1];
      v[0] += n;
      v[1] += (float)r[4 * i];
      v[2] += (float)r[4 * i + 2];
      v[3] += correct > 0.5f * n ? correct : n - correct;
      ++i;
    }
  if (o->comm) {   // the ranks' values added in rank order: the same bits on every rank, with one rank the plain object's
    double t[4] = {v[0], v[1], v[2], v[3]};
    const int rc = dfh_comm_allreduce_sum(o->comm, t, 4);
    if (rc) return rc;
    for (int k = 0; k < 4; ++k) v[k] = (float)t[k];
  }
  for (int k = 0; k < 4; ++k) prog[k] = v[k];
  return DFH_OK;
}

void bcd_free_chunk(dfh_bcd::Chunk& ch) {
  chunks::release(ch);
  for (void* p : {(void*)ch.s_gk, (void*)ch.nz, (void*)ch.r_key, (void*)ch.r_val, (void*)ch.rec, (void*)ch.rec_row, (void*)ch.rec_lo})
    if (p) (void)hipFree(p);
}

int bcd_free(dfh_bcd* o) {
  if (!o) return DFH_OK;
  if (o->ctx) (void)hipSetDevice(o->ctx->device);
  for (auto& cs : o->chunks)
    for (auto& ch : cs) bcd_free_chunk(ch);
  for (void* p : {(void*)o->d_pbeg, (void*)o->d_pend, (void*)o->d_w, (void*)o->d_delta, (void*)o->d_dw, (void*)o->d_gacc,
                  (void*)o->d_hacc, o->slab_mem, (void*)o->d_order, (void*)o->d_part, (void*)o->d_res, (void*)o->d_xg,
                  (void*)o->d_xh, (void*)o->d_xd})
    if (p) (void)hipFree(p);
  delete o;
  return DFH_OK;
}

// the layouts of one chunk (see the head of this file); gmap / cblk: model position and block of every chunk key
int bcd_build_chunk(dfh_bcd* o, dfh_bcd::Chunk& ch, const std::vector<int>& gmap, const std::vector<int>& cblk,
                    const uint64_t* blk_begin, const uint64_t* blk_end) {
  hipStream_t s = o->ctx->stream;
  const int nblk = o->nblk;
  const size_t U = ch.U, nnz = ch.nnz;
  std::vector<uint32_t> col_ptr(U + 1, 0);
  if (U) DFH_HIP(hipMemcpyAsync(col_ptr.data(), ch.b->d_col_ptr, (U + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  // per block: the slice of the key-ordered view over the block's key range (filtered keys inside it stay, s_gk = -1);
  // entries of the row-major layout: those of the keys in a block
  std::vector<uint2> nz(std::max(nblk, 1), make_uint2(0, 0));
  for (int b = 0; b < nblk; ++b) {
    const size_t c0 = std::lower_bound(ch.keys.begin(), ch.keys.end(), blk_begin[b]) - ch.keys.begin();
    const size_t c1 = std::lower_bound(ch.keys.begin() + c0, ch.keys.end(), blk_end[b]) - ch.keys.begin();
    nz[b] = make_uint2(col_ptr[c0], col_ptr[c1]);
    ch.max_nz = std::max<uint32_t>(ch.max_nz, col_ptr[c1] - col_ptr[c0]);
  }
  size_t m = 0;
  for (size_t u = 0; u < U; ++u)
    if (cblk[u] >= 0) m += col_ptr[u + 1] - col_ptr[u];
  ch.m = (uint32_t)m;
  size_t sort_tmp = 0, scan_tmp = 0;
  DFH_HIP(rocprim::radix_sort_pairs(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                    std::max<size_t>(nnz, 1), 0, 64, s));
  DFH_HIP(rocprim::inclusive_scan(nullptr, scan_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, std::max<size_t>(m, 1),
                                  rocprim::plus<uint32_t>(), s));
  const size_t tmp = std::max(sort_tmp, scan_tmp);
  int rc = chunks::check_free(kBcdWho, "the layouts of a data chunk", kBcdTail, bcd_layout_bytes(nnz, nblk, ch.b->has_value) + bcd_build_bytes(nnz, tmp));
  if (rc) return rc;
  const bool val = ch.b->has_value;
  DFH_HIP(hipMalloc(&ch.s_gk, std::max<size_t>(nnz, 1) * sizeof(int)));
  DFH_HIP(hipMalloc(&ch.nz, nz.size() * sizeof(uint2)));
  DFH_HIP(hipMalloc(&ch.r_key, std::max<size_t>(m, 1) * sizeof(int)));
  if (val) DFH_HIP(hipMalloc(&ch.r_val, std::max<size_t>(m, 1) * sizeof(float)));
  DFH_HIP(hipMalloc(&ch.rec, (size_t)(nblk + 1) * sizeof(uint32_t)));
  DFH_HIP(hipMemcpyAsync(ch.nz, nz.data(), nz.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
  // transient: gmap, cblk, sort keys in / out, positions in / out, heads, their scan, library temp
  char* t = nullptr;
  const size_t n1 = std::max<size_t>(nnz, 1), u1 = std::max<size_t>(U, 1);
  const size_t tb = u1 * 8 + n1 * (8 + 8 + 4 + 4 + 4 + 4) + tmp + 8 * 256;
  DFH_HIP(hipMalloc(&t, tb));
  Carver cv(t);   // nine pieces, each begun on 256 bytes: at most 8 x 255 bytes of padding
  int* d_gmap = cv.take<int>(u1);
  int* d_cblk = cv.take<int>(u1);
  uint64_t* k_in = cv.take<uint64_t>(n1);
  uint64_t* k_out = cv.take<uint64_t>(n1);
  uint32_t* v_in = cv.take<uint32_t>(n1);
  uint32_t* v_out = cv.take<uint32_t>(n1);
  uint32_t* head = cv.take<uint32_t>(n1);
  uint32_t* idx = cv.take<uint32_t>(n1);
  void* d_tmp = cv.take<char>(tmp);
  rc = DFH_OK;
  do {
    if (U) {
      if (hipMemcpyAsync(d_gmap, gmap.data(), U * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
          hipMemcpyAsync(d_cblk, cblk.data(), U * 4, hipMemcpyHostToDevice, s) != hipSuccess) {
        rc = DFH_ERR_HIP;
        break;
      }
    }
    if (nnz) {
      hipLaunchKernelGGL(bcd::k_bcd_entries, dim3(bcd::grid_of(nnz, bcd::THREADS)), dim3(bcd::THREADS), 0, s, ch.b->d_col_ptr,
                         (uint32_t)U, (uint32_t)nnz, ch.b->d_s_row, d_gmap, d_cblk, ch.s_gk, k_in, v_in);
      int bits = 1;
      while ((1 << bits) <= nblk) ++bits;
      size_t tsz = tmp;
      if (rocprim::radix_sort_pairs(d_tmp, tsz, k_in, k_out, v_in, v_out, nnz, 0, 32 + bits, s) != hipSuccess) {
        rc = DFH_ERR_HIP;
        break;
      }
    }
    ch.nrec = 0;
    if (m) {
      hipLaunchKernelGGL(bcd::k_bcd_rowmajor, dim3(bcd::grid_of(m, bcd::THREADS)), dim3(bcd::THREADS), 0, s, k_out, v_out,
                         (uint32_t)m, ch.s_gk, val ? ch.b->d_s_val : nullptr, ch.r_key, ch.r_val, head);
      size_t tsz = tmp;
      if (rocprim::inclusive_scan(d_tmp, tsz, head, idx, m, rocprim::plus<uint32_t>(), s) != hipSuccess ||
          hipMemcpyAsync(&ch.nrec, idx + m - 1, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess) {
        rc = DFH_ERR_HIP;
        break;
      }
    }
    if (hipMalloc(&ch.rec_row, std::max<size_t>(ch.nrec, 1) * 4) != hipSuccess ||
        hipMalloc(&ch.rec_lo, ((size_t)ch.nrec + 1) * 4) != hipSuccess) {
      rc = DFH_ERR_HIP;
      break;
    }
    if (m) {
      hipLaunchKernelGGL(bcd::k_bcd_records, dim3(bcd::grid_of(m, bcd::THREADS)), dim3(bcd::THREADS), 0, s, k_out, head, idx,
                         (uint32_t)m, ch.rec_row, ch.rec_lo);
      hipLaunchKernelGGL(bcd::k_bcd_rec_begin, dim3(bcd::grid_of(nblk + 1, bcd::THREADS)), dim3(bcd::THREADS), 0, s, k_out,
                         ch.rec_lo, ch.nrec, nblk, ch.rec);
    } else if (hipMemsetAsync(ch.rec, 0, (size_t)(nblk + 1) * 4, s) != hipSuccess ||
               hipMemsetAsync(ch.rec_lo, 0, 4, s) != hipSuccess) {
      rc = DFH_ERR_HIP;
      break;
    }
    if (hipGetLastError() != hipSuccess) {
      rc = DFH_ERR_HIP;
      break;
    }
    std::vector<uint32_t> rec(nblk + 1);
    if (hipMemcpyAsync(rec.data(), ch.rec, rec.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemsetAsync(ch.b->d_pred, 0, ch.nrows * sizeof(float), s) != hipSuccess ||
        chunks::reset_prog(ch.b, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      rc = DFH_ERR_HIP;
      break;
    }
    for (int b = 0; b < nblk; ++b) ch.max_rec = std::max(ch.max_rec, rec[b + 1] - rec[b]);
  } while (0);
  (void)hipFree(t);
  if (rc == DFH_ERR_HIP) set_error("dfh_bcd_build: building the layouts of a chunk failed");
  return rc;
}

}  // namespace

extern "C" {

int dfh_bcd_create(dfh_ctx* c, dfh_bcd** out) {
  DFH_ARG(c && out, "dfh_bcd_create: NULL argument");
  dfh_bcd* o = new (std::nothrow) dfh_bcd();
  DFH_ARG(o != nullptr, "out of host memory");
  o->ctx = c;
  *out = o;
  return DFH_OK;
}

int dfh_bcd_create_sharded(dfh_ctx* c, dfh_comm* comm, dfh_bcd** out) {
  DFH_ARG(c && comm && out && comm->ctx == c, "dfh_bcd_create_sharded: the context and the communicator must match");
  DFH_ARG(!comm->loopback, "dfh_bcd_create_sharded: the loop-back transport is for dfh_shard_step measurements only");
  const int rc = dfh_bcd_create(c, out);
  if (rc) return rc;
  (*out)->comm = comm;
  const size_t W = (size_t)comm->world;
  for (auto* v : {&(*out)->xsb, &(*out)->xso, &(*out)->xrb, &(*out)->xsb4, &(*out)->xrb4, &(*out)->xzero}) v->assign(W, 0);
  return DFH_OK;
}

int dfh_bcd_destroy(dfh_bcd* o) { return bcd_free(o); }

int dfh_bcd_add_chunk(dfh_bcd* o, int is_val, size_t nrows, const size_t* offset, const uint64_t* index, const float* value,
                      const float* label) {
  DFH_ARG(o && offset && label && nrows >= 1, "dfh_bcd_add_chunk: bad argument");
  DFH_ARG(!o->built, "dfh_bcd_add_chunk: the layouts are already built");
  const size_t nnz = offset[nrows] - offset[0];
  DFH_ARG(nnz < (size_t(1) << 31) && nrows < (size_t(1) << 31), "dfh_bcd_add_chunk: a chunk holds fewer than 2^31 rows and entries");
  dfh_bcd::Chunk ch;
  // + the layouts dfh_bcd_build adds to the chunk
  const int rc = chunks::add(o->ctx, kBcdWho, kBcdTail, bcd_layout_bytes(nnz, 0, value != nullptr), nrows, offset, index, value,
                             label, &ch);
  if (rc) return rc;
  o->chunks[is_val ? 1 : 0].push_back(std::move(ch));
  return DFH_OK;
}

int dfh_bcd_build(dfh_bcd* o, float tail_feature_filter, int nblk, const uint64_t* blk_begin, const uint64_t* blk_end, float l1,
                  float lr, uint64_t* nkeys) {
  DFH_ARG(o && !o->built, "dfh_bcd_build: bad argument or called twice");
  DFH_ARG(o->comm || !o->chunks[0].empty(), "dfh_bcd_build: no training chunk");
  DFH_ARG(nblk >= 0 && (nblk == 0 || (blk_begin && blk_end)), "dfh_bcd_build: bad block ranges");
  for (int b = 0; b < nblk; ++b) {
    DFH_ARG(blk_begin[b] < blk_end[b], "dfh_bcd_build: an empty block range");
    DFH_ARG(b == 0 || blk_end[b - 1] <= blk_begin[b], "dfh_bcd_build: block ranges must be sorted and disjoint");
  }
  DFH_HIP(hipSetDevice(o->ctx->device));
  hipStream_t s = o->ctx->stream;
  o->nblk = nblk;
  o->l1 = l1;
  o->lr = lr;
  // merged feature counts (KVUnion in chunk order, tile_builder.h:171-176), keys with count > filter kept
  // (BuildFeatureMap, bcd_learner.cc:127-146)
  {
    std::vector<const chunks::Resident*> train(o->chunks[0].size());
    for (size_t i = 0; i < train.size(); ++i) train[i] = &o->chunks[0][i];
    std::vector<uint64_t> tk;
    std::vector<float> tc;
    chunks::merged_counts(train, &tk, &tc);
    if (o->comm) {
      // the ranks' (key, count) lists to every rank; a key's counts are added in ascending source rank, so every rank
      // filters the same global counts and builds the same model
      const int W = o->comm->world;
      std::vector<uint64_t> n(W, 0);
      const uint64_t mine = tk.size();
      int rc = dfh_comm_allgather(o->comm, &mine, sizeof(mine), n.data());
      if (rc) return rc;
      size_t tot = 0;
      for (int p = 0; p < W; ++p) tot += n[p];
      std::vector<uint64_t> ak(std::max<size_t>(tot, 1));
      std::vector<float> ac(std::max<size_t>(tot, 1));
      rc = bcd_allgatherv(o, tk.data(), sizeof(uint64_t), n, ak.data());
      if (!rc) rc = bcd_allgatherv(o, tc.data(), sizeof(float), n, ac.data());
      if (rc) return rc;
      std::vector<chunks::Resident> parts(W);
      std::vector<const chunks::Resident*> ranks(W);
      size_t at = 0;
      for (int p = 0; p < W; ++p) {
        parts[p].U = n[p];
        parts[p].keys.assign(ak.begin() + at, ak.begin() + at + n[p]);
        parts[p].cnt.assign(ac.begin() + at, ac.begin() + at + n[p]);
        at += n[p];
        ranks[p] = &parts[p];
      }
      chunks::merged_counts(ranks, &tk, &tc);
    }
    for (size_t i = 0; i < tk.size(); ++i)
      if (tc[i] > tail_feature_filter) {
        o->keys.push_back(tk[i]);
        o->cnts.push_back(tc[i]);
      }
  }
  const size_t K = o->keys.size();
  DFH_ARG(K < (size_t(1) << 31), "dfh_bcd_build: more than 2^31 - 1 keys");
  // each block's positions among the keys (TileBuilder::FindPosition, tile_builder.h:117-135)
  o->pbeg.assign(nblk, 0);
  o->pend.assign(nblk, 0);
  for (int b = 0; b < nblk; ++b) {
    o->pbeg[b] = (int)(std::lower_bound(o->keys.begin(), o->keys.end(), blk_begin[b]) - o->keys.begin());
    o->pend[b] = (int)(std::lower_bound(o->keys.begin(), o->keys.end(), blk_end[b]) - o->keys.begin());
    o->max_keys = std::max(o->max_keys, o->pend[b] - o->pbeg[b]);
  }
  const size_t K1 = std::max<size_t>(K, 1), B1 = std::max(nblk, 1);
  const size_t mk = std::max(o->max_keys, 1);
  size_t max_shares = 1;
  // shares bound: the largest block slice of any training chunk is at most the chunk's nnz
  for (auto& ch : o->chunks[0]) max_shares = std::max<size_t>(max_shares, (ch.nnz + bcd::SHARE - 1) / bcd::SHARE + bcd::WAVES);
  o->res_cap = 4 * (o->chunks[0].size() + o->chunks[1].size());
  // sharded: the staging of the two exchanges, sized for the largest block
  if (o->comm) o->max_slice = (o->max_keys + o->comm->world - 1) / o->comm->world;
  const size_t xs = std::max<size_t>((o->comm ? (size_t)o->comm->world : 0) * o->max_slice, mk);
  const size_t state = K1 * 12 + mk * 16 + max_shares * 40 + B1 * 12 + bcd::PROG_BLOCKS * 16 + o->res_cap * 8 + 4096 +
                       (o->comm ? xs * 16 + mk * 4 : 0);
  int rc = chunks::check_free(kBcdWho, "the model and the block state", kBcdTail, state);
  if (rc) return rc;
  DFH_HIP(hipMalloc(&o->d_pbeg, B1 * sizeof(int)));
  DFH_HIP(hipMalloc(&o->d_pend, B1 * sizeof(int)));
  DFH_HIP(hipMalloc(&o->d_w, K1 * sizeof(float)));
  DFH_HIP(hipMalloc(&o->d_delta, K1 * sizeof(float)));
  DFH_HIP(hipMalloc(&o->d_dw, K1 * sizeof(float)));
  DFH_HIP(hipMalloc(&o->d_gacc, mk * sizeof(double)));
  DFH_HIP(hipMalloc(&o->d_hacc, mk * sizeof(double)));
  DFH_HIP(hipMalloc(&o->slab_mem, max_shares * 40));
  {
    char* p = static_cast<char*>(o->slab_mem);
    o->slab.fg = reinterpret_cast<double*>(p);
    o->slab.fh = o->slab.fg + max_shares;
    o->slab.lg = o->slab.fh + max_shares;
    o->slab.lh = o->slab.lg + max_shares;
    o->slab.fk = reinterpret_cast<int*>(o->slab.lh + max_shares);
    o->slab.lk = o->slab.fk + max_shares;
  }
  DFH_HIP(hipMalloc(&o->d_order, B1 * sizeof(int)));
  DFH_HIP(hipMalloc(&o->d_part, bcd::PROG_BLOCKS * 2 * sizeof(double)));
  DFH_HIP(hipMalloc(&o->d_res, std::max<size_t>(o->res_cap, 4) * sizeof(double)));
  if (o->comm) {
    DFH_HIP(hipMalloc(&o->d_xg, xs * sizeof(double)));
    DFH_HIP(hipMalloc(&o->d_xh, xs * sizeof(double)));
    DFH_HIP(hipMalloc(&o->d_xd, mk * sizeof(float)));
  }
  if (nblk) {
    DFH_HIP(hipMemcpyAsync(o->d_pbeg, o->pbeg.data(), nblk * sizeof(int), hipMemcpyHostToDevice, s));
    DFH_HIP(hipMemcpyAsync(o->d_pend, o->pend.data(), nblk * sizeof(int), hipMemcpyHostToDevice, s));
  }
  // w = 0, delta = 1 (bcd::Delta::Init), dw = 0
  std::vector<float> ones(K1, 1.f);
  DFH_HIP(hipMemsetAsync(o->d_w, 0, K1 * sizeof(float), s));
  DFH_HIP(hipMemsetAsync(o->d_dw, 0, K1 * sizeof(float), s));
  DFH_HIP(hipMemcpyAsync(o->d_delta, ones.data(), K1 * sizeof(float), hipMemcpyHostToDevice, s));
  DFH_HIP(hipMemsetAsync(o->d_gacc, 0, mk * sizeof(double), s));
  DFH_HIP(hipMemsetAsync(o->d_hacc, 0, mk * sizeof(double), s));
  DFH_HIP(hipStreamSynchronize(s));
  // every chunk: colmap (TileBuilder::BuildColmap, tile_builder.h:62-76: -1 = filtered) and each key's block, then the layouts
  for (auto& cs : o->chunks)
    for (auto& ch : cs) {
      std::vector<int> gmap, cblk(std::max<size_t>(ch.U, 1), -1);
      chunks::colmap(ch, o->keys, &gmap);
      int b = 0;
      for (size_t u = 0; u < ch.U; ++u) {
        const uint64_t key = ch.keys[u];
        while (b < nblk && blk_end[b] <= key) ++b;
        if (gmap[u] >= 0 && b < nblk && blk_begin[b] <= key) cblk[u] = b;
      }
      rc = bcd_build_chunk(o, ch, gmap, cblk, blk_begin, blk_end);
      if (rc) return rc;
    }
  o->built = true;
  if (nkeys) *nkeys = K;
  return DFH_OK;
}

int dfh_bcd_shape(dfh_bcd* o, uint64_t* nkeys, int* nblk, int* ntrain_chunks, int* nval_chunks) {
  DFH_ARG(o, "NULL argument");
  if (nkeys) *nkeys = o->keys.size();
  if (nblk) *nblk = o->nblk;
  if (ntrain_chunks) *ntrain_chunks = (int)o->chunks[0].size();
  if (nval_chunks) *nval_chunks = (int)o->chunks[1].size();
  return DFH_OK;
}

int dfh_bcd_block_info(dfh_bcd* o, int blk, int* pos_begin, int* pos_end, uint64_t* nnz, uint64_t* rows) {
  DFH_ARG(o && o->built && blk >= 0 && blk < o->nblk, "dfh_bcd_block_info: bad argument");
  if (pos_begin) *pos_begin = o->pbeg[blk];
  if (pos_end) *pos_end = o->pend[blk];
  if (nnz || rows) {
    uint64_t z = 0, r = 0;
    hipStream_t s = o->ctx->stream;
    for (auto& cs : o->chunks)
      for (auto& ch : cs) {
        uint2 v;
        uint32_t rr[2];
        DFH_HIP(hipMemcpyAsync(&v, ch.nz + blk, sizeof(v), hipMemcpyDeviceToHost, s));
        DFH_HIP(hipMemcpyAsync(rr, ch.rec + blk, sizeof(rr), hipMemcpyDeviceToHost, s));
        DFH_HIP(hipStreamSynchronize(s));
        if (&cs == &o->chunks[0]) z += v.y - v.x;
        r += rr[1] - rr[0];
      }
    if (nnz) *nnz = z;
    if (rows) *rows = r;
  }
  return DFH_OK;
}

int dfh_bcd_epoch(dfh_bcd* o, const int* order, int n, float* progress) {
  DFH_ARG(o && o->built && order && n >= 1 && n <= o->nblk, "dfh_bcd_epoch: bad argument");
  for (int i = 0; i < n; ++i) DFH_ARG(order[i] >= 0 && order[i] < o->nblk, "dfh_bcd_epoch: a block id out of range");
  DFH_HIP(hipSetDevice(o->ctx->device));
  hipStream_t s = o->ctx->stream;
  o->stepped = true;
  o->h_order.assign(order, order + n);
  DFH_HIP(hipMemcpyAsync(o->d_order, o->h_order.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
  for (int i = 0; i < n; ++i) {
    int rc = bcd_block(o, i, 1);
    if (rc) return rc;
  }
  float prog[4];
  int rc = bcd_progress(o, prog);   // synchronises
  if (rc) return rc;
  if (progress) std::copy(prog, prog + 4, progress);
  return DFH_OK;
}

int dfh_bcd_step(dfh_bcd* o, int blk, double* g, double* h, float* progress) {
  DFH_ARG(o && o->built && blk >= 0 && blk < o->nblk, "dfh_bcd_step: bad argument");
  DFH_HIP(hipSetDevice(o->ctx->device));
  hipStream_t s = o->ctx->stream;
  o->stepped = true;
  o->h_order.assign(1, blk);
  DFH_HIP(hipMemcpyAsync(o->d_order, o->h_order.data(), sizeof(int), hipMemcpyHostToDevice, s));
  const bool keep = g || h;
  int rc = bcd_block(o, 0, keep ? 0 : 1);
  if (rc) return rc;
  if (keep) {
    const size_t nk = (size_t)(o->pend[blk] - o->pbeg[blk]);
    if (o->comm) {   // the global sums: the owners' reduced slices, gathered
      rc = bcd_gather_gh(o, blk);
      if (rc) return rc;
    }
    if (g && nk) DFH_HIP(hipMemcpyAsync(g, o->comm ? o->d_xg : o->d_gacc, nk * sizeof(double), hipMemcpyDeviceToHost, s));
    if (h && nk) DFH_HIP(hipMemcpyAsync(h, o->comm ? o->d_xh : o->d_hacc, nk * sizeof(double), hipMemcpyDeviceToHost, s));
    DFH_HIP(hipMemsetAsync(o->d_gacc, 0, std::max(o->max_keys, 1) * sizeof(double), s));
    DFH_HIP(hipMemsetAsync(o->d_hacc, 0, std::max(o->max_keys, 1) * sizeof(double), s));
  }
  if (progress) return bcd_progress(o, progress);
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

int dfh_bcd_set_model(dfh_bcd* o, uint64_t n, const uint64_t* keys, const float* w, uint64_t* n_matched) {
  DFH_ARG(o && (n == 0 || (keys && w)), "dfh_bcd_set_model: NULL argument");
  if (!o->built) {
    set_error("dfh_bcd_set_model: the layouts are not built (call dfh_bcd_build first)");
    return DFH_ERR_STATE;
  }
  if (o->stepped) {
    set_error("dfh_bcd_set_model: a block step has run: the model is set before the first dfh_bcd_epoch / dfh_bcd_step");
    return DFH_ERR_STATE;
  }
  for (uint64_t i = 0; i < n; ++i) DFH_ARG(std::isfinite(w[i]), "dfh_bcd_set_model: w holds a non-finite value");
  DFH_HIP(hipSetDevice(o->ctx->device));
  hipStream_t s = o->ctx->stream;
  // from the state dfh_bcd_build leaves: w = 0, pred = 0 (delta and delta w are untouched before the first step)
  const size_t K = o->keys.size();
  DFH_HIP(hipMemsetAsync(o->d_w, 0, std::max<size_t>(K, 1) * sizeof(float), s));
  for (auto& cs : o->chunks)
    for (auto& ch : cs) DFH_HIP(hipMemsetAsync(ch.b->d_pred, 0, ch.nrows * sizeof(float), s));
  if (n_matched) *n_matched = 0;
  if (n == 0 || K == 0) {
    DFH_HIP(hipStreamSynchronize(s));
    return DFH_OK;
  }
  join::Result j;
  int rc = join::run(o->ctx, o->keys.data(), K, keys, n, n * sizeof(float), &j);
  if (rc) return rc;
  if (j.dups) {
    (void)hipFree(j.mem);
    set_error("dfh_bcd_set_model: the input keys are not unique");
    return DFH_ERR_ARG;
  }
  rc = DFH_OK;
  do {
    if (!j.matched) break;
    float* d_win = reinterpret_cast<float*>(j.extra);
    if (hipMemcpyAsync(d_win, w, n * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) {
      rc = DFH_ERR_HIP;
      break;
    }
    hipLaunchKernelGGL(bcd::k_bcd_set_w, dim3(bcd::grid_of(n, bcd::THREADS)), dim3(bcd::THREADS), 0, s, j.pos, d_win, (uint64_t)n,
                       o->d_w);
    // the predictions: k_bcd_pred from pred = 0 with delta w := w, the blocks in ascending order
    o->h_order.resize(o->nblk);
    for (int b = 0; b < o->nblk; ++b) o->h_order[b] = b;
    if (o->nblk && hipMemcpyAsync(o->d_order, o->h_order.data(), o->nblk * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) {
      rc = DFH_ERR_HIP;
      break;
    }
    for (int b = 0; b < o->nblk; ++b) {
      if (o->pend[b] == o->pbeg[b]) continue;   // a block without keys touches no row
      for (auto& cs : o->chunks)
        for (auto& ch : cs) {
          if (!ch.max_rec) continue;
          bcd::PredArgs p{o->d_order, b, ch.rec, ch.rec_row, ch.rec_lo, ch.r_key, ch.r_val, o->d_w, ch.b->d_pred};
          hipLaunchKernelGGL(bcd::k_bcd_pred, dim3(bcd::grid_of(ch.max_rec, bcd::THREADS)), dim3(bcd::THREADS), 0, s, p);
        }
    }
    if (hipGetLastError() != hipSuccess) rc = DFH_ERR_HIP;
  } while (0);
  if (hipStreamSynchronize(s) != hipSuccess) rc = DFH_ERR_HIP;
  (void)hipFree(j.mem);
  if (rc) {
    set_error("dfh_bcd_set_model: setting the model on the device failed");
    return rc;
  }
  if (n_matched) *n_matched = j.matched;
  return DFH_OK;
}

int dfh_bcd_get_model(dfh_bcd* o, uint64_t* keys, float* feacnt, float* w, float* delta, float* dw) {
  DFH_ARG(o && o->built, "dfh_bcd_get_model: the layouts are not built");
  const size_t K = o->keys.size();
  if (keys) std::copy(o->keys.begin(), o->keys.end(), keys);
  if (feacnt) std::copy(o->cnts.begin(), o->cnts.end(), feacnt);
  hipStream_t s = o->ctx->stream;
  DFH_HIP(hipSetDevice(o->ctx->device));
  if (K) {
    if (w) DFH_HIP(hipMemcpyAsync(w, o->d_w, K * sizeof(float), hipMemcpyDeviceToHost, s));
    if (delta) DFH_HIP(hipMemcpyAsync(delta, o->d_delta, K * sizeof(float), hipMemcpyDeviceToHost, s));
    if (dw) DFH_HIP(hipMemcpyAsync(dw, o->d_dw, K * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

int dfh_bcd_get_pred(dfh_bcd* o, int is_val, int chunk, float* pred, size_t* nrows) {
  DFH_ARG(o && chunk >= 0 && chunk < (int)o->chunks[is_val ? 1 : 0].size(), "dfh_bcd_get_pred: bad argument");
  auto& ch = o->chunks[is_val ? 1 : 0][chunk];
  if (nrows) *nrows = ch.nrows;
  if (pred) {
    DFH_ARG(o->built, "dfh_bcd_get_pred: the layouts are not built");
    DFH_HIP(hipSetDevice(o->ctx->device));
    DFH_HIP(hipMemcpyAsync(pred, ch.b->d_pred, ch.nrows * sizeof(float), hipMemcpyDeviceToHost, o->ctx->stream));
    DFH_HIP(hipStreamSynchronize(o->ctx->stream));
  }
  return DFH_OK;
}

}  // extern "C"
