// dfh_eval_groups.hip — exact_metrics by group: the AUC, logloss and accuracy of every GROUP of the appended rows (a user, a
// site, a campaign) and the grouped AUC of the set (included behind dfh_eval.hip, whose evaluator it extends; the learner's
// exact_metrics_group).  With dfh_eval_group_by_slot set, the evaluator keeps one more pair of device arrays: a row's 64-bit
// group id and a byte that says whether it has one (9 B per row).
//   k_geval_rowgroup  (an append of a stepped batch) a lane group of 8 lanes per row, 32 rows per block: the lanes take the
//                  row's positions eight at a time in ascending order, id = reverse_bytes(feaids[index[j]]); the first position
//                  with (id & 4095) == slot is the lowest set bit of the lane group's byte of the wave's ballot, and its id comes
//                  over by a shuffle.  It reads what the step left in the batch object; nothing is uploaded
// dfh_eval_finish_groups, T = GV_TILE = 2 048 rows per tile (256 threads x 8 consecutive rows):
//   k_geval_count / k_geval_scan_cnt / k_geval_compact   the rows WITH a group, in appended order, as two u64 words each: the
//                  group id and (score key << 1 | label bit), the key of k_eval_keys (-0.0 as +0.0, every NaN 0xFFFFFFFF).  No
//                  id value is a sentinel: rows without a group are left out here and counted (n_nogroup)
//   rocprim::radix_sort_pairs twice, least significant first: 33 bits of the score word, then 64 bits of the id; the sort is
//                  stable, so the order is (id, key, label bit, appended order) — a function of the appended sequence alone
//   k_geval_tile<0>  per tile: its negatives, its GROUP HEADS (a row whose id differs from the row before it), its last group
//                  head and its last TIE HEAD (id or key differs from the row before: a tie never reaches across a group
//                  border), each with the tile's negatives in front of it
//   k_geval_scan   one block over the tiles: negatives and group heads in front of every tile, the last tie head and the last
//                  group head in front of every tile with the negatives of the whole order in front of them
//   k_geval_tile<1>  per tile again.  A tie group [s, e) of a group that starts at b closes at its LAST row and gives that row
//                      P (NEG(s) - NEG(b) + NEG(e) - NEG(b)),  P = (e - s) - (NEG(e) - NEG(s))
//                  (NEG(i): negatives in front of row i; a NaN tie gives 0; s and b come from the scans, tiles back if need be).
//                  A row's values (1, positive, NaN, correct, that u64, its fp64 logloss term) are then summed by group: a thread
//                  adds its 8 rows from its last group head on, a segmented inclusive scan in LDS keyed by "this thread holds a
//                  group head" (Hillis-Steele, eight rounds, the left operand first) gives every thread the sum from the last
//                  head in front of it, and a second walk closes every group at its last row.  A group that lies inside the tile
//                  writes its record to slot (group heads in front of its head); the rows in front of the tile's first head are
//                  the tile's HEAD PARTIAL, the rows from its last head on, when their group goes on, its TAIL PARTIAL
//   k_geval_carry  a thread per tile with a tail partial: tail + the head partials of the following tiles up to the first tile
//                  that holds a group head, in tile order, is the record of that group
//   k_geval_summary  one block: n_mixed, rows_mixed and gauc_num over the records, a thread's records in ascending slot, then
//                  the fixed tree
// The fp64 sum of a group is therefore a fixed expression of the positions of its rows and of the group heads in the sorted
// order (which rows share a thread, which threads a tile), and the sorted order is a function of the appended sequence: the same
// bits on every run, however the rows were cut into appends.  No floating-point atomics (no atomics at all), no block waits on
// another block, vector stores and plain C++ only.  The records stay in device memory (dfh_eval_read_groups).
namespace {
constexpr uint32_t GV_TILE = EV_TILE;
constexpr uint32_t GV_NAN = 0xFFFFFFFFu;

struct GSum {   // what a group sums over its rows (32 B)
  uint32_t n, pos, nan, cor;
  uint64_t auc;
  double obj;
};
__device__ __forceinline__ GSum gv_zero() { return GSum{0u, 0u, 0u, 0u, 0ull, 0.0}; }
__device__ __forceinline__ GSum gv_add(const GSum& a, const GSum& b) {   // a's rows are in front of b's
  return GSum{a.n + b.n, a.pos + b.pos, a.nan + b.nan, a.cor + b.cor, a.auc + b.auc, a.obj + b.obj};
}

struct GRec {   // the records, one array per field, n_groups long
  uint64_t *gid, *n, *n_pos, *n_nan, *auc2, *correct;
  double* objv;
};
__device__ __forceinline__ void gv_write(const GRec& r, uint64_t slot, uint64_t gid, const GSum& v) {
  r.gid[slot] = gid;
  r.n[slot] = v.n;
  r.n_pos[slot] = v.pos;
  r.n_nan[slot] = v.nan;
  r.auc2[slot] = v.auc;
  r.correct[slot] = v.cor;
  r.objv[slot] = v.obj;
}

struct GHdr {   // (dfh_eval_groups_result's fields, in its order)
  uint64_t n_groups, n_mixed, rows_mixed, n_nogroup;
  double gauc_num;
};

// a lane group of 8 lanes per row; at[row] / has[row] are the evaluator's arrays at the append's first row
__global__ void __launch_bounds__(256) k_geval_rowgroup(const uint32_t* __restrict__ offset, const uint32_t* __restrict__ index,
                                                        const uint64_t* __restrict__ feaids, uint32_t nrows, uint32_t slot,
                                                        uint64_t* __restrict__ gid, uint8_t* __restrict__ has) {
  const uint32_t lane = threadIdx.x & 63u, sub = lane & 7u, lead = lane & ~7u;
  const uint32_t row = blockIdx.x * 32u + (threadIdx.x >> 3);
  uint32_t j = 0, end = 0;
  if (row < nrows) {
    j = offset[row] + sub;
    end = offset[row + 1];
  }
  bool found = false;
  uint64_t g = 0;
  // every lane of the wave makes the same number of rounds: the ballot is taken with all of them in step
  while (__ballot(!found && j < end) != 0ull) {
    uint64_t id = 0;
    bool hit = false;
    if (!found && j < end) {
      id = reverse_bytes(feaids[index[j]]);
      hit = (uint32_t)(id & 4095u) == slot;
    }
    const uint32_t mine = (uint32_t)(__ballot(hit) >> lead) & 0xFFu;
    const int src = (int)lead + (mine ? __ffs((int)mine) - 1 : 0);
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)id, src), hi = (uint32_t)__shfl((int)(uint32_t)(id >> 32), src);
    if (!found && mine) {
      found = true;
      g = (uint64_t)hi << 32 | lo;
    }
    j += 8;
  }
  if (row < nrows && sub == 0) {
    gid[row] = g;
    has[row] = found ? 1 : 0;
  }
}

__global__ void __launch_bounds__(256) k_geval_count(const uint8_t* __restrict__ has, uint64_t n, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t sh_u[256];
  const uint64_t first = (uint64_t)blockIdx.x * GV_TILE + (uint64_t)threadIdx.x * EV_ITEMS;
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < EV_ITEMS; ++j)
    if (first + j < n && has[first + j]) ++c;
  const uint32_t sum = ev_block_sum(c, sh_u);
  if (threadIdx.x == 0) cnt[blockIdx.x] = sum;
}

// pre[t] = the sum of cnt[0 .. t), pre[ntiles] = the total
__global__ void __launch_bounds__(256) k_geval_scan_cnt(const uint32_t* __restrict__ cnt, uint32_t ntiles, uint32_t* __restrict__ pre) {
  __shared__ uint32_t sh_u[256];
  uint32_t run = 0;
  for (uint32_t b = 0; b < ntiles; b += 256) {
    const uint32_t t = b + threadIdx.x;
    const uint32_t v = t < ntiles ? cnt[t] : 0u;
    const uint32_t incl = ev_block_scan(v, sh_u, EvSum());
    if (t < ntiles) pre[t] = run + incl - v;
    __syncthreads();
    sh_u[threadIdx.x] = incl;
    __syncthreads();
    run += sh_u[255];
  }
  if (threadIdx.x == 0) pre[ntiles] = run;
}

// the rows with a group, in appended order: og[d] = the id, ok[d] = score key << 1 | (label > 0); d < pre[ntiles]
__global__ void __launch_bounds__(256) k_geval_compact(const float* __restrict__ pred, const float* __restrict__ label,
                                                       const uint64_t* __restrict__ gid, const uint8_t* __restrict__ has, uint64_t n,
                                                       const uint32_t* __restrict__ pre, uint64_t* __restrict__ og,
                                                       uint64_t* __restrict__ ok) {
  __shared__ uint32_t sh_u[256];
  const uint64_t first = (uint64_t)blockIdx.x * GV_TILE + (uint64_t)threadIdx.x * EV_ITEMS;
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < EV_ITEMS; ++j)
    if (first + j < n && has[first + j]) ++c;
  const uint32_t incl = ev_block_scan(c, sh_u, EvSum());
  uint64_t d = (uint64_t)pre[blockIdx.x] + (incl - c);
#pragma unroll
  for (uint32_t j = 0; j < EV_ITEMS; ++j) {
    const uint64_t i = first + j;
    if (i >= n || !has[i]) continue;
    const float s = pred[i];
    uint32_t key = GV_NAN;
    if (s == s) {
      const uint32_t u = s == 0.0f ? 0u : __float_as_uint(s);
      key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    og[d] = gid[i];
    ok[d] = (uint64_t)key << 1 | (label[i] > 0.0f ? 1u : 0u);
    ++d;
  }
}

// FINAL = 0: tile_cnt[t] = (negatives, group heads), tile_tie[t], tile_grp[t] (head records with the tile's negatives).
// FINAL = 1: pre_cnt / prev_tie / prev_grp (k_geval_scan) in; records, hp[t], tp[t], tgid[t] out (hp and tp zeroed before).
template <int FINAL>
__global__ void __launch_bounds__(256) k_geval_tile(const uint64_t* __restrict__ gid, const uint64_t* __restrict__ kf, uint64_t m,
                                                    uint2* __restrict__ tile_cnt, uint64_t* __restrict__ tile_tie,
                                                    uint64_t* __restrict__ tile_grp, const uint2* __restrict__ pre_cnt,
                                                    const uint64_t* __restrict__ prev_tie, const uint64_t* __restrict__ prev_grp,
                                                    GSum* __restrict__ hp, GSum* __restrict__ tp, uint64_t* __restrict__ tgid, GRec rec) {
  __shared__ uint32_t sh_u[256];
  __shared__ uint64_t sh_w[256];
  __shared__ GSum sh_s[256];
  __shared__ uint32_t sh_f[256];
  const uint32_t t = threadIdx.x;
  const uint64_t tile0 = (uint64_t)blockIdx.x * GV_TILE, first = tile0 + (uint64_t)t * EV_ITEMS;
  // rows first - 1 .. first + 8: slot 0 is the row in front of this thread's, slot 9 the row behind them
  uint64_t g[EV_ITEMS + 2];
  uint32_t k[EV_ITEMS + 2];
  uint32_t lab = 0;   // bit j: row first + j is labelled positive
  {
    const bool in = first > 0 && first - 1 < m;
    const uint64_t w = in ? kf[first - 1] : 0;
    g[0] = in ? gid[first - 1] : 0;
    k[0] = (uint32_t)(w >> 1);
  }
#pragma unroll
  for (uint32_t j = 0; j <= EV_ITEMS; ++j) {
    const uint64_t i = first + j;
    const bool in = i < m;
    const uint64_t w = in ? kf[i] : 0;
    g[j + 1] = in ? gid[i] : 0;
    k[j + 1] = (uint32_t)(w >> 1);
    if (j < EV_ITEMS) lab |= (uint32_t)(w & 1u) << j;
  }
  // bit j of: a valid row, a group head, a tie head, a negative
  uint32_t valid = 0, ghead = 0, thead = 0, negm = 0;
#pragma unroll
  for (uint32_t j = 0; j < EV_ITEMS; ++j) {
    const uint64_t i = first + j;
    if (i >= m) continue;
    valid |= 1u << j;
    const bool gh = i == 0 || g[j + 1] != g[j];
    if (gh) ghead |= 1u << j;
    if (gh || k[j + 1] != k[j]) thead |= 1u << j;
    if (!((lab >> j) & 1u) && k[j + 1] != GV_NAN) negm |= 1u << j;
  }
  const uint32_t tneg = __popc(negm), nh = __popc(ghead);
  const uint32_t incl_neg = ev_block_scan(tneg, sh_u, EvSum());
  const uint32_t incl_h = ev_block_scan(nh, sh_u, EvSum());
  uint32_t np = incl_neg - tneg;   // negatives in front of this thread's rows: of the tile, FINAL: of the whole order
  uint64_t hb = incl_h - nh;       // group heads in front of them
  if (FINAL) {
    const uint2 pc = pre_cnt[blockIdx.x];
    np += pc.x;
    hb += pc.y;
  }
  uint64_t last_t = 0, last_g = 0;   // this thread's last tie head and group head
  {
    uint32_t q = np;
#pragma unroll
    for (uint32_t j = 0; j < EV_ITEMS; ++j) {
      if ((thead >> j) & 1u) last_t = ev_head(first + j, q);
      if ((ghead >> j) & 1u) last_g = ev_head(first + j, q);
      q += (negm >> j) & 1u;
    }
  }
  const uint64_t ti = ev_block_scan(last_t, sh_w, EvMax());
  if (!FINAL) {
    const uint64_t gi = ev_block_scan(last_g, sh_w, EvMax());
    if (t == 255) {
      tile_cnt[blockIdx.x] = make_uint2(incl_neg, incl_h);
      tile_tie[blockIdx.x] = ti;
      tile_grp[blockIdx.x] = gi;
    }
    return;
  }
  // the last tie head and group head in front of this thread's rows: in the tile (the exclusive scan) or before it
  __syncthreads();
  sh_w[t] = ti;
  __syncthreads();
  uint64_t sT = t > 0 ? sh_w[t - 1] : 0;
  const uint64_t gi = ev_block_scan(last_g, sh_w, EvMax());
  __syncthreads();
  sh_w[t] = gi;
  __syncthreads();
  uint64_t sB = t > 0 ? sh_w[t - 1] : 0;
  {
    const uint64_t ct = prev_tie[blockIdx.x], cg = prev_grp[blockIdx.x];
    if (ct > sT) sT = ct;
    if (cg > sB) sB = cg;
  }
  // a row's values; a tie group closes at its last row
  uint64_t a[EV_ITEMS];
  double d[EV_ITEMS];
  uint32_t corm = 0;
  GSum tail = gv_zero();   // this thread's rows from its last group head on (all of them when it holds none)
  {
    uint32_t q = np;
#pragma unroll
    for (uint32_t j = 0; j < EV_ITEMS; ++j) {
      a[j] = 0;
      d[j] = 0.0;
      if (!((valid >> j) & 1u)) continue;
      const uint64_t i = first + j;
      if ((thead >> j) & 1u) sT = ev_head(i, q);
      if ((ghead >> j) & 1u) {
        sB = ev_head(i, q);
        tail = gv_zero();
      }
      q += (negm >> j) & 1u;
      const uint32_t key = k[j + 1];
      const bool pos = (lab >> j) & 1u, nan = key == GV_NAN;
      if (!nan) {
        const float s = __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
        const double mg = pos ? (double)s : -(double)s;
        d[j] = fmax(-mg, 0.0) + log1p(exp(-fabs(mg)));
        if ((pos && s > 0.0f) || (!pos && s <= 0.0f)) corm |= 1u << j;
        const bool tlast = i + 1 >= m || g[j + 2] != g[j + 1] || k[j + 2] != key;
        if (tlast) {   // the tie group [s, i + 1) of the group that starts at sB: NEG(i + 1) = q
          const uint64_t s0 = (sT >> 32) - 1, nps = sT & 0xFFFFFFFFu, npb = sB & 0xFFFFFFFFu;
          const uint64_t P = (i + 1 - s0) - (q - nps);
          a[j] = P * ((nps - npb) + (q - npb));
        }
      }
      tail = gv_add(tail, GSum{1u, (pos && !nan) ? 1u : 0u, nan ? 1u : 0u, (corm >> j) & 1u, a[j], d[j]});
    }
  }
  // the segmented inclusive scan over the threads, keyed by "holds a group head"
  __syncthreads();
  sh_s[t] = tail;
  sh_f[t] = nh ? 1u : 0u;
  __syncthreads();
  {
    GSum v = tail;
    uint32_t f = nh ? 1u : 0u;
#pragma unroll
    for (uint32_t dd = 1; dd < 256; dd <<= 1) {
      GSum o = gv_zero();
      uint32_t of = 0;
      if (t >= dd) {
        o = sh_s[t - dd];
        of = sh_f[t - dd];
      }
      __syncthreads();
      if (t >= dd) {
        if (!f) v = gv_add(o, v);
        f |= of;
        sh_s[t] = v;
        sh_f[t] = f;
      }
      __syncthreads();
    }
  }
  GSum acc = t > 0 ? sh_s[t - 1] : gv_zero();   // from the last group head of the tile in front of this thread's rows
  bool in_tile = t > 0 && sh_f[t - 1];          // ... which exists
  uint64_t h = hb;
#pragma unroll
  for (uint32_t j = 0; j < EV_ITEMS; ++j) {
    if (!((valid >> j) & 1u)) continue;
    const uint64_t i = first + j;
    if ((ghead >> j) & 1u) {
      acc = gv_zero();
      in_tile = true;
      ++h;
    }
    const uint32_t key = k[j + 1];
    const bool pos = (lab >> j) & 1u, nan = key == GV_NAN;
    acc = gv_add(acc, GSum{1u, (pos && !nan) ? 1u : 0u, nan ? 1u : 0u, (corm >> j) & 1u, a[j], d[j]});
    const bool glast = i + 1 >= m || g[j + 2] != g[j + 1];
    if (glast) {
      if (in_tile) gv_write(rec, h - 1, g[j + 1], acc);
      else hp[blockIdx.x] = acc;
    } else if (i + 1 == tile0 + GV_TILE) {   // the group goes on behind the tile
      if (in_tile) {
        tp[blockIdx.x] = acc;
        tgid[blockIdx.x] = g[j + 1];
      } else {
        hp[blockIdx.x] = acc;
      }
    }
  }
}

// pre_cnt[t] = (negatives, group heads) in front of tile t, prev_tie[t] / prev_grp[t] = the last tie head / group head in front
// of tile t with the negatives of the whole order in front of it; pre_cnt[ntiles]: the totals
__global__ void __launch_bounds__(256) k_geval_scan(const uint2* __restrict__ tile_cnt, const uint64_t* __restrict__ tile_tie,
                                                    const uint64_t* __restrict__ tile_grp, uint32_t ntiles, uint2* __restrict__ pre_cnt,
                                                    uint64_t* __restrict__ prev_tie, uint64_t* __restrict__ prev_grp) {
  __shared__ uint32_t sh_u[256];
  __shared__ uint64_t sh_w[256];
  uint32_t run_neg = 0, run_h = 0;
  uint64_t run_t = 0, run_g = 0;
  for (uint32_t b = 0; b < ntiles; b += 256) {
    const uint32_t t = b + threadIdx.x;
    const uint2 c = t < ntiles ? tile_cnt[t] : make_uint2(0u, 0u);
    const uint32_t ineg = ev_block_scan(c.x, sh_u, EvSum());
    __syncthreads();
    sh_u[threadIdx.x] = ineg;
    __syncthreads();
    const uint32_t tot_neg = sh_u[255];
    const uint32_t ih = ev_block_scan(c.y, sh_u, EvSum());
    __syncthreads();
    sh_u[threadIdx.x] = ih;
    __syncthreads();
    const uint32_t tot_h = sh_u[255];
    const uint32_t pre = run_neg + ineg - c.x;
    uint64_t ht = t < ntiles ? tile_tie[t] : 0, hg = t < ntiles ? tile_grp[t] : 0;
    if (ht) ht += pre;   // the low word: negatives of the tile in front of the head -> of the whole order (< 2^32: no carry)
    if (hg) hg += pre;
    const uint64_t it = ev_block_scan(ht, sh_w, EvMax());
    __syncthreads();
    sh_w[threadIdx.x] = it;
    __syncthreads();
    uint64_t pt = threadIdx.x > 0 ? sh_w[threadIdx.x - 1] : 0;
    const uint64_t lt = sh_w[255];
    const uint64_t ig = ev_block_scan(hg, sh_w, EvMax());
    __syncthreads();
    sh_w[threadIdx.x] = ig;
    __syncthreads();
    uint64_t pg = threadIdx.x > 0 ? sh_w[threadIdx.x - 1] : 0;
    const uint64_t lg = sh_w[255];
    if (run_t > pt) pt = run_t;
    if (run_g > pg) pg = run_g;
    if (t < ntiles) {
      pre_cnt[t] = make_uint2(pre, run_h + ih - c.y);
      prev_tie[t] = pt;
      prev_grp[t] = pg;
    }
    if (lt > run_t) run_t = lt;
    if (lg > run_g) run_g = lg;
    run_neg += tot_neg;
    run_h += tot_h;
    __syncthreads();
  }
  if (threadIdx.x == 0) pre_cnt[ntiles] = make_uint2(run_neg, run_h);
}

// a group that spans tiles: the tail partial of the tile of its head, then the head partials of the tiles behind it, in order
__global__ void __launch_bounds__(256) k_geval_carry(const GSum* __restrict__ hp, const GSum* __restrict__ tp,
                                                     const uint64_t* __restrict__ tgid, const uint2* __restrict__ pre_cnt,
                                                     uint32_t ntiles, GRec rec) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  GSum acc = tp[t];
  if (acc.n == 0) return;
  for (uint32_t u = t + 1; u < ntiles; ++u) {
    acc = gv_add(acc, hp[u]);
    if (pre_cnt[u + 1].y != pre_cnt[u].y) break;   // tile u holds a group head: the group ended in front of it
  }
  gv_write(rec, (uint64_t)pre_cnt[t + 1].y - 1, tgid[t], acc);
}

__global__ void __launch_bounds__(256) k_geval_summary(GRec rec, uint64_t n_groups, uint64_t n_nogroup, GHdr* __restrict__ hdr) {
  __shared__ double sh_d[256];
  __shared__ uint64_t sh_w[256];
  double num = 0;
  uint64_t mixed = 0, rows = 0;
  for (uint64_t r = threadIdx.x; r < n_groups; r += 256) {   // ascending id per thread, then the fixed tree
    const uint64_t p = rec.n_pos[r], q = rec.n[r] - rec.n_nan[r] - p;
    if (p == 0 || q == 0) continue;
    ++mixed;
    rows += p + q;
    num += (double)(p + q) * (double)rec.auc2[r] / (2.0 * (double)p * (double)q);
  }
  const double o = ev_block_sum(num, sh_d);
  const uint64_t a = ev_block_sum(mixed, sh_w);
  const uint64_t b = ev_block_sum(rows, sh_w);
  if (threadIdx.x == 0) {
    hdr->n_groups = n_groups;
    hdr->n_mixed = a;
    hdr->rows_mixed = b;
    hdr->n_nogroup = n_nogroup;
    hdr->gauc_num = o;
  }
}

// room for the groups of `extra` more rows (the arrays follow d_pred / d_label; copies ride the stream like theirs)
int gv_reserve(dfh_eval* e, size_t extra) {
  const size_t need = e->n + extra;
  if (need <= e->gcap) return DFH_OK;
  size_t cap = e->gcap ? e->gcap : (e->hint ? e->hint : (size_t)1 << 16);
  while (cap < need) cap *= 2;
  uint64_t* ng = nullptr;
  uint8_t* nh = nullptr;
  if (hipMalloc((void**)&ng, cap * sizeof(uint64_t)) != hipSuccess || hipMalloc((void**)&nh, cap) != hipSuccess) {
    (void)hipGetLastError();
    if (ng) (void)hipFree(ng);
    set_error("dfh_eval: no device memory for the groups of " + std::to_string(cap) + " rows (" + std::to_string(cap * 9) +
              " bytes needed)");
    return DFH_ERR_CAPACITY;
  }
  if (e->n) {
    hipError_t er = hipMemcpyAsync(ng, e->d_gid, e->n * sizeof(uint64_t), hipMemcpyDeviceToDevice, e->ctx->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(nh, e->d_has, e->n, hipMemcpyDeviceToDevice, e->ctx->stream);
    if (er != hipSuccess) {
      e->retired.push_back(ng);
      e->retired.push_back(nh);
      set_error(std::string("dfh_eval: hipMemcpyAsync: ") + hipGetErrorString(er));
      return DFH_ERR_HIP;
    }
  }
  if (e->d_gid) e->retired.push_back(e->d_gid);
  if (e->d_has) e->retired.push_back(e->d_has);
  e->d_gid = ng;
  e->d_has = nh;
  e->gcap = cap;
  return DFH_OK;
}

// the groups of a stepped batch's rows, behind its step, into the evaluator's rows [at, at + nrows)
int gv_rowgroup(dfh_eval* e, dfh_batch* b, size_t at) {
  if (b->nrows == 0) return DFH_OK;
  hipLaunchKernelGGL(k_geval_rowgroup, dim3((unsigned)((b->nrows + 31) / 32)), dim3(256), 0, e->ctx->stream, b->d_offset, b->d_index,
                     b->d_feaids, (uint32_t)b->nrows, (uint32_t)e->slot, e->d_gid + at, e->d_has + at);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

void gv_free(dfh_eval* e) {
  if (e->d_gid) (void)hipFree(e->d_gid);
  if (e->d_has) (void)hipFree(e->d_has);
  if (e->d_gpre) (void)hipFree(e->d_gpre);
  if (e->d_rec) (void)hipFree(e->d_rec);
}

GRec gv_rec(char* p, size_t G) {
  uint64_t* w = (uint64_t*)p;
  return GRec{w, w + G, w + 2 * G, w + 3 * G, w + 4 * G, w + 5 * G, (double*)(w + 6 * G)};
}
}  // namespace

extern "C" {

int dfh_eval_group_by_slot(dfh_eval* e, int slot) {
  DFH_ARG(e, "dfh_eval_group_by_slot: NULL argument");
  DFH_ARG(slot >= -1 && slot <= 4095, "dfh_eval_group_by_slot: slot must be -1 (off) or one of 0 .. 4095, the low 12 bits of an id");
  if (e->n) {
    set_error("dfh_eval_group_by_slot: the evaluator holds " + std::to_string(e->n) + " rows; set the slot while it is empty (after "
              "dfh_eval_create or dfh_eval_reset)");
    return DFH_ERR_STATE;
  }
  e->slot = slot;
  return DFH_OK;
}

int dfh_eval_append_host_groups(dfh_eval* e, const float* label, const float* pred, const uint64_t* gid, const uint8_t* has_group,
                                size_t n) {
  DFH_ARG(e, "dfh_eval_append_host_groups: NULL argument");
  DFH_ARG(n < EV_MAX_ROWS && e->n + (uint64_t)n < EV_MAX_ROWS, "dfh_eval_append_host_groups: an evaluator holds fewer than 2^32 - 16 rows");
  DFH_ARG(n == 0 || (label && pred && gid), "dfh_eval_append_host_groups: NULL argument");
  if (e->slot < 0) {
    set_error("dfh_eval_append_host_groups: grouping is off; call dfh_eval_group_by_slot on the empty evaluator first");
    return DFH_ERR_STATE;
  }
  if (n == 0) return DFH_OK;
  hipStream_t s = e->ctx->stream;
  DFH_HIP(hipSetDevice(e->ctx->device));
  int rc = gv_reserve(e, n);
  if (rc) return rc;
  const size_t at = e->n;
  rc = ev_append(e, label, pred, n, hipMemcpyHostToDevice);
  if (rc) return rc;
  hipError_t er = hipMemcpyAsync(e->d_gid + at, gid, n * sizeof(uint64_t), hipMemcpyHostToDevice, s);
  if (er == hipSuccess)
    er = has_group ? hipMemcpyAsync(e->d_has + at, has_group, n, hipMemcpyHostToDevice, s) : hipMemsetAsync(e->d_has + at, 1, n, s);
  const hipError_t es = hipStreamSynchronize(s);   // the caller's arrays are free on return
  if (er != hipSuccess || es != hipSuccess) {
    e->n = at;   // the rows are not kept without their groups
    set_error(std::string("dfh_eval_append_host_groups: ") + hipGetErrorString(er != hipSuccess ? er : es));
    return DFH_ERR_HIP;
  }
  return DFH_OK;
}

int dfh_eval_finish_groups(dfh_eval* e, dfh_eval_groups_result* out) {
  DFH_ARG(e && out, "dfh_eval_finish_groups: NULL argument");
  static_assert(sizeof(dfh_eval_groups_result) == sizeof(GHdr) && offsetof(dfh_eval_groups_result, gauc_num) == offsetof(GHdr, gauc_num),
                "GHdr is the result");
  memset(out, 0, sizeof(*out));
  if (e->slot < 0) {
    set_error("dfh_eval_finish_groups: grouping is off; call dfh_eval_group_by_slot on the empty evaluator first");
    return DFH_ERR_STATE;
  }
  hipStream_t s = e->ctx->stream;
  DFH_HIP(hipSetDevice(e->ctx->device));
  e->rec_n = 0;
  const size_t n = e->n;
  // 1. how many rows have a group
  uint32_t m32 = 0;
  const uint32_t ntn = (uint32_t)((n + GV_TILE - 1) / GV_TILE);
  uint32_t *cnt = nullptr, *pre = nullptr;
  if (n) {
    int rc = dev_grow(&e->d_gpre, &e->gpre_bytes, ev_pad((size_t)ntn * 4) + ev_pad(((size_t)ntn + 1) * 4), "dfh_eval_finish_groups", "the tiles' row counts");
    if (rc) return rc;
    cnt = (uint32_t*)e->d_gpre;
    pre = (uint32_t*)(e->d_gpre + ev_pad((size_t)ntn * 4));
    hipLaunchKernelGGL(k_geval_count, dim3(ntn), dim3(256), 0, s, e->d_has, (uint64_t)n, cnt);
    hipLaunchKernelGGL(k_geval_scan_cnt, dim3(1), dim3(256), 0, s, cnt, ntn, pre);
    DFH_HIP(hipGetLastError());
    DFH_HIP(hipMemcpyAsync(&m32, pre + ntn, 4, hipMemcpyDeviceToHost, s));
  }
  DFH_HIP(hipStreamSynchronize(s));
  ev_free_retired(e);
  const size_t m = m32;
  out->n_nogroup = n - m;
  if (m == 0) return DFH_OK;
  // 2. order them and count the groups
  const uint32_t nt = (uint32_t)((m + GV_TILE - 1) / GV_TILE);
  size_t tb1 = 0, tb2 = 0;
  DFH_HIP(rocprim::radix_sort_pairs(nullptr, tb1, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, m, 0, 33, s));
  DFH_HIP(rocprim::radix_sort_pairs(nullptr, tb2, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, m, 0, 64, s));
  const size_t tb = std::max(tb1, tb2);
  // the workspace: header | id x 2 | score word x 2 | per tile: counts, tie, group, pre (+1), prev tie, prev group, head partial,
  // tail partial, tail id | the sort's
  const size_t o_hdr = 0;
  const size_t o_g0 = o_hdr + ev_pad(sizeof(GHdr)), o_g1 = o_g0 + ev_pad(m * 8);
  const size_t o_k0 = o_g1 + ev_pad(m * 8), o_k1 = o_k0 + ev_pad(m * 8);
  const size_t o_tc = o_k1 + ev_pad(m * 8), o_tt = o_tc + ev_pad((size_t)nt * 8);
  const size_t o_tg = o_tt + ev_pad((size_t)nt * 8), o_pc = o_tg + ev_pad((size_t)nt * 8);
  const size_t o_pt = o_pc + ev_pad(((size_t)nt + 1) * 8), o_pg = o_pt + ev_pad((size_t)nt * 8);
  const size_t o_hp = o_pg + ev_pad((size_t)nt * 8), o_tp = o_hp + ev_pad((size_t)nt * sizeof(GSum));
  const size_t o_id = o_tp + ev_pad((size_t)nt * sizeof(GSum)), o_temp = o_id + ev_pad((size_t)nt * 8);
  const size_t bytes = o_temp + ev_pad(tb + 16);
  int rc = dev_grow(&e->d_work, &e->work_bytes, bytes, "dfh_eval_finish_groups", ("ranking " + std::to_string(m) + " rows by group").c_str());
  if (rc) return rc;
  char* w = e->d_work;
  GHdr* hdr = (GHdr*)(w + o_hdr);
  uint64_t *g0 = (uint64_t*)(w + o_g0), *g1 = (uint64_t*)(w + o_g1), *k0 = (uint64_t*)(w + o_k0), *k1 = (uint64_t*)(w + o_k1);
  uint2 *tc = (uint2*)(w + o_tc), *pc = (uint2*)(w + o_pc);
  uint64_t *tt = (uint64_t*)(w + o_tt), *tg = (uint64_t*)(w + o_tg), *pt = (uint64_t*)(w + o_pt), *pg = (uint64_t*)(w + o_pg);
  GSum *hp = (GSum*)(w + o_hp), *tp = (GSum*)(w + o_tp);
  uint64_t* tgid = (uint64_t*)(w + o_id);
  hipLaunchKernelGGL(k_geval_compact, dim3(ntn), dim3(256), 0, s, e->d_pred, e->d_label, e->d_gid, e->d_has, (uint64_t)n, pre, g0, k0);
  DFH_HIP(hipGetLastError());
  DFH_HIP(rocprim::radix_sort_pairs(w + o_temp, tb1, k0, k1, g0, g1, m, 0, 33, s));   // by the score word, the id rides
  DFH_HIP(rocprim::radix_sort_pairs(w + o_temp, tb2, g1, g0, k1, k0, m, 0, 64, s));   // by the id, the score word rides
  hipLaunchKernelGGL(k_geval_tile<0>, dim3(nt), dim3(256), 0, s, g0, k0, (uint64_t)m, tc, tt, tg, (const uint2*)nullptr,
                     (const uint64_t*)nullptr, (const uint64_t*)nullptr, (GSum*)nullptr, (GSum*)nullptr, (uint64_t*)nullptr, GRec{});
  hipLaunchKernelGGL(k_geval_scan, dim3(1), dim3(256), 0, s, tc, tt, tg, nt, pc, pt, pg);
  DFH_HIP(hipGetLastError());
  uint2 tot = make_uint2(0u, 0u);
  DFH_HIP(hipMemcpyAsync(&tot, pc + nt, sizeof(tot), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  const size_t G = tot.y;
  // 3. the records and the summary
  rc = dev_grow(&e->d_rec, &e->rec_bytes, G * 7 * 8, "dfh_eval_finish_groups", ("the records of " + std::to_string(G) + " groups").c_str());
  if (rc) return rc;
  const GRec rec = gv_rec(e->d_rec, G);
  DFH_HIP(hipMemsetAsync(hp, 0, (size_t)nt * sizeof(GSum), s));
  DFH_HIP(hipMemsetAsync(tp, 0, (size_t)nt * sizeof(GSum), s));
  hipLaunchKernelGGL(k_geval_tile<1>, dim3(nt), dim3(256), 0, s, g0, k0, (uint64_t)m, (uint2*)nullptr, (uint64_t*)nullptr,
                     (uint64_t*)nullptr, pc, pt, pg, hp, tp, tgid, rec);
  hipLaunchKernelGGL(k_geval_carry, dim3((nt + 255) / 256), dim3(256), 0, s, hp, tp, tgid, pc, nt, rec);
  hipLaunchKernelGGL(k_geval_summary, dim3(1), dim3(256), 0, s, rec, (uint64_t)G, (uint64_t)(n - m), hdr);
  DFH_HIP(hipGetLastError());
  GHdr h;
  DFH_HIP(hipMemcpyAsync(&h, hdr, sizeof(h), hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  e->rec_n = G;
  out->n_groups = h.n_groups;
  out->n_mixed = h.n_mixed;
  out->rows_mixed = h.rows_mixed;
  out->n_nogroup = h.n_nogroup;
  out->gauc_num = h.gauc_num;
  return DFH_OK;
}

int dfh_eval_read_groups(dfh_eval* e, uint64_t first, uint64_t count, uint64_t* gid, uint64_t* n, uint64_t* n_pos, uint64_t* n_nan,
                         uint64_t* auc2, uint64_t* correct, double* objv) {
  DFH_ARG(e, "dfh_eval_read_groups: NULL argument");
  DFH_ARG(first <= e->rec_n && count <= e->rec_n - first, "dfh_eval_read_groups: first + count is beyond the groups of the last "
                                                          "dfh_eval_finish_groups");
  if (count == 0) return DFH_OK;
  hipStream_t s = e->ctx->stream;
  DFH_HIP(hipSetDevice(e->ctx->device));
  const GRec r = gv_rec(e->d_rec, e->rec_n);
  const void* src[7] = {r.gid, r.n, r.n_pos, r.n_nan, r.auc2, r.correct, r.objv};
  void* dst[7] = {gid, n, n_pos, n_nan, auc2, correct, objv};
  for (int f = 0; f < 7; ++f)
    if (dst[f]) DFH_HIP(hipMemcpyAsync(dst[f], (const char*)src[f] + first * 8, count * 8, hipMemcpyDeviceToHost, s));
  DFH_HIP(hipStreamSynchronize(s));
  return DFH_OK;
}

}  // extern "C"
