// dfh_pending.hip — the single-queue step's noted Localizer stages, host side (the device side is dfh_riders.hip): a stage
// as a launch of its own, what is left of a minibatch's stages queued at once, and the riders of a step's next launch.
// Needs the handles only, so the stream phases (dfh_phases.hip) call flush_pending without a declaration.
namespace {
// one stage (RiderKind) of the noted sample sort of b's minibatch as a launch of its own on stream s
void launch_loc_stage(dfh_batch* b, int stage, hipStream_t s, dfh_table* probe = nullptr) {
  const LocView& v = b->loc_v;
  switch (stage) {
    case RID_COUNT:
      if (b->loc_big) hipLaunchKernelGGL(k_loc_count<LOC_BIG_BUCKETS>, dim3(v.ntiles), dim3(LOC_TILE_THREADS), 0, s, v);
      else if (b->loc_fuse_gather) hipLaunchKernelGGL(k_loc_count_gather<LOC_MAX_BUCKETS>, dim3(v.ntiles), dim3(LOC_TILE_THREADS), 0, s, v, b->gsrc);
      else hipLaunchKernelGGL(k_loc_count<LOC_MAX_BUCKETS>, dim3(v.ntiles), dim3(LOC_TILE_THREADS), 0, s, v);
      break;
    case RID_SCATTER:
      if (b->loc_big) hipLaunchKernelGGL(k_loc_scatter<LOC_BIG_BUCKETS>, dim3(v.ntiles), dim3(LOC_TILE_THREADS), 0, s, v);
      else hipLaunchKernelGGL(k_loc_scatter<LOC_MAX_BUCKETS>, dim3(v.ntiles), dim3(LOC_TILE_THREADS), 0, s, v);
      break;
    case RID_SORT:
      hipLaunchKernelGGL(k_loc_sort, dim3(b->loc_gsort), dim3(LOC_SORT_THREADS), loc_sort_smem(), s, v);   // (dynamic LDS: k_loc_sort)
      break;
    default:
      if (probe) hipLaunchKernelGGL(k_loc_emit<true>, dim3(b->loc_gsort), dim3(LOC_EMIT_THREADS), 0, s, v, b->loc_o, probe->v, b->d_urow);
      else hipLaunchKernelGGL(k_loc_emit<false>, dim3(b->loc_gsort), dim3(LOC_EMIT_THREADS), 0, s, v, b->loc_o, TableView{}, (uint32_t*)nullptr);
      break;
  }
}

void pend_remove(dfh_ctx* c, dfh_batch* b) {
  auto it = std::find(c->pend.begin(), c->pend.end(), b);
  if (it != c->pend.end()) c->pend.erase(it);
}

int flush_pending(dfh_batch* b) {
  dfh_ctx* c = b->ctx;
  if (b->pend_stage >= RID_STAGES) return DFH_OK;
  {
    TimeScope ts(c, DFH_K_LOCALIZE);
    for (int st = b->pend_stage; st < RID_STAGES; ++st) launch_loc_stage(b, st, c->stream);
  }
  b->pend_stage = RID_STAGES;
  pend_remove(c, b);
  DFH_HIP(hipGetLastError());
  return DFH_OK;
}

// the riders of the next launch of kind `slot` (0 lookup, 1 forward, 2 update): for every minibatch with noted stages, in the
// order they were noted, its next stage if that stage belongs into this kind of launch.  A stage configured to run alone, or
// one too many for the launch (can_ride false: the launch has no rider form), is queued here as a launch of its own — just
// before the carrier — and the minibatch's following stage is considered at once.  main_groups: the carrier's own blocks / 8.
void collect_riders(dfh_ctx* c, int slot, bool can_ride, uint32_t main_groups, RiderSet* rs) {
  rs->n = 0;
  rs->ngroups = 0;
  rs->period = 1;
  rs->start = 0;
  rs->first[0] = 0;
  if (!c->single_queue || c->pend.empty()) return;
  for (size_t i = 0; i < c->pend.size(); ++i) {
    dfh_batch* p = c->pend[i];
    while (p->pend_stage < RID_STAGES && c->rider_slot[p->pend_stage] == slot) {
      const int st = p->pend_stage;
      if (c->rider_alone[st] || !can_ride || rs->n == MAX_RIDERS) {
        TimeScope ts(c, DFH_K_LOCALIZE);
        launch_loc_stage(p, st, c->stream);
        ++p->pend_stage;
        continue;
      }
      Rider& r = rs->r[rs->n];
      r.v = p->loc_v;
      r.o = p->loc_o;
      r.kind = (uint32_t)st;
      r.nblk = (st == RID_COUNT || st == RID_SCATTER) ? (uint32_t)p->loc_v.ntiles : p->loc_gsort;
      rs->first[rs->n + 1] = rs->first[rs->n] + ((r.nblk + 7u) & ~7u);
      ++rs->n;
      ++p->pend_stage;
      break;  // the minibatch's next stage needs this launch to have ended
    }
  }
  // emit (the stage the next step's lookup waits for) before the others: its blocks are dispatched first
  for (uint32_t j = 1; j < rs->n; ++j) {
    if (rs->r[j].kind == RID_EMIT && rs->r[0].kind != RID_EMIT) {
      std::swap(rs->r[0], rs->r[j]);
      uint32_t at = 0;
      for (uint32_t q = 0; q < rs->n; ++q) {
        rs->first[q] = at;
        at += (rs->r[q].nblk + 7u) & ~7u;
      }
      rs->first[rs->n] = at;
      break;
    }
  }
  c->pend.erase(std::remove_if(c->pend.begin(), c->pend.end(), [](dfh_batch* p) { return p->pend_stage >= RID_STAGES; }), c->pend.end());
  rs->ngroups = rs->first[rs->n] / 8u;
  for (uint32_t q = rs->n + 1; q <= (uint32_t)MAX_RIDERS; ++q) rs->first[q] = rs->first[rs->n];  // (run_rider: no rider beyond n - 1)
  if (rs->ngroups) {
    // every rider group needs a place: the last one sits at group (ngroups - 1) * period of main_groups + ngroups
    rs->start = (uint32_t)((uint64_t)main_groups * (uint64_t)c->rider_start[slot] / 100u);
    const uint32_t left = main_groups - rs->start;   // main groups among which the rider groups are dealt
    uint32_t per = (uint32_t)std::max(1, c->rider_period[slot]);
    if (rs->ngroups > 1) per = std::min(per, (left + rs->ngroups - 1u) / (rs->ngroups - 1u));
    rs->period = std::max(1u, per);
  }
}
}  // namespace
