// The communicator behind the C ABI (include/difacto_hip.h, dfh_comm_*): what the sharded store (dfh_shard.hip) and the sharded
// learner=lbfgs / learner=bcd (dfh_lbfgs.hip, dfh_bcd.hip) exchange over: device buffers (comm_exchange), host bytes (HostXchg).
// Transport (dfh_comm): RCCL ncclSend / ncclRecv grouped per exchange, on the context's stream —
// the library is loaded at run time (dlopen) so that a process which already carries an RCCL (a
// Python host with torch) shares it, and a host without multi-GPU needs never loads one; or a host
// callback (exchange staged through host memory) for process groups RCCL cannot serve — tests with
// several ranks sharing one GPU; or the loop-back transport (measurement: one GPU as rank r of W).
#ifndef DFH_COMM_HIP_
#define DFH_COMM_HIP_
#include <dlfcn.h>
#include <link.h>

#include <deque>

namespace dfh {

// ---- the slice of RCCL's C API this file binds (rccl/rccl.h: ncclGetUniqueId :187, ncclCommInitRank :220,
// ncclCommDestroy :260, ncclGetErrorString :339, ncclSend :700, ncclRecv :722, ncclGroupStart/End :923-933)
struct RcclId { char internal[128]; };
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(RcclId*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*GetVersion)(int*) = nullptr;
  std::string path;        // the file ncclSend was bound from (dladdr)
  bool was_loaded = false; // the process already carried this library (e.g. the copy inside torch/lib)
};

// a library of the process whose file name contains "librccl": a host that already carries RCCL (PyTorch bundles
// one) must share it — two RCCLs in one process would each run their own bootstrap and proxy threads
inline int rccl_phdr_cb(struct dl_phdr_info* info, size_t, void* out) {
  if (info->dlpi_name && strstr(info->dlpi_name, "librccl")) {
    *static_cast<std::string*>(out) = info->dlpi_name;
    return 1;
  }
  return 0;
}

inline RcclApi* rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    // (1) whatever RCCL the process has already mapped, by its own path; (2) a loaded library under the usual
    // sonames; (3) load one
    std::string loaded;
    dl_iterate_phdr(rccl_phdr_cb, &loaded);
    if (!loaded.empty()) api.lib = dlopen(loaded.c_str(), RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    const char* names[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
    for (const char* n : names) {
      if (api.lib) break;
      api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    }
    api.was_loaded = api.lib != nullptr;
    for (const char* n : names) {
      if (api.lib) break;
      api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!api.lib) return;
#define DFH_SYM(field, name) api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.lib, name))
    DFH_SYM(GetUniqueId, "ncclGetUniqueId");
    DFH_SYM(CommInitRank, "ncclCommInitRank");
    DFH_SYM(CommDestroy, "ncclCommDestroy");
    DFH_SYM(GetErrorString, "ncclGetErrorString");
    DFH_SYM(Send, "ncclSend");
    DFH_SYM(Recv, "ncclRecv");
    DFH_SYM(GroupStart, "ncclGroupStart");
    DFH_SYM(GroupEnd, "ncclGroupEnd");
    DFH_SYM(GetVersion, "ncclGetVersion");
#undef DFH_SYM
    Dl_info di;
    if (api.Send && dladdr(reinterpret_cast<void*>(api.Send), &di) && di.dli_fname) api.path = di.dli_fname;
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.Send || !api.Recv || !api.GroupStart || !api.GroupEnd) {
      dlclose(api.lib);
      api.lib = nullptr;
    }
  });
  return api.lib ? &api : nullptr;
}

#define DFH_RCCL(call)                                                                                  \
  do {                                                                                                  \
    int r__ = (call);                                                                                   \
    if (r__ != 0) {                                                                                     \
      RcclApi* a__ = rccl_api();                                                                        \
      ::dfh::set_error(std::string(#call) + ": " + ((a__ && a__->GetErrorString) ? a__->GetErrorString(r__) : "RCCL error")); \
      return DFH_ERR_HIP;                                                                               \
    }                                                                                                   \
  } while (0)

// ---- loop-back transport (dfh_comm_create_loopback): the copies of one exchange in ONE launch
struct LoopSegs {
  const char* src[64];
  char* dst[64];            // NULL: a send — the bytes are read and dropped
  unsigned long long bytes[64];
  int n;
};

// block b walks the segments in 16 B (or, for a misaligned segment, 4 B) units, grid-stride.  A "send" is read in full
// (one xor per unit, stored only if it hits a value it cannot hit: the loads stay) — on real wires the send buffer is
// read out of this GPU's HBM once and nothing is written here.  Thread 0 of block 0 stamps the wall clock for k_loop_wait.
__global__ void __launch_bounds__(256) k_loop_copy(LoopSegs g, unsigned long long* __restrict__ stamp, unsigned* __restrict__ sink) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && stamp) *stamp = wall_clock64();
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
  unsigned acc = 0;
  for (int i = 0; i < g.n; ++i) {
    const char* s = g.src[i];
    char* d = g.dst[i];
    const size_t nb = g.bytes[i];
    const bool wide = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | nb) & 15) == 0;
    if (wide) {
      const uint4* s4 = reinterpret_cast<const uint4*>(s);
      uint4* d4 = reinterpret_cast<uint4*>(d);
      for (size_t j = tid; j < nb / 16; j += nth) {
        const uint4 v = s4[j];
        if (d) d4[j] = v; else acc ^= v.x ^ v.y ^ v.z ^ v.w;
      }
    } else {
      const unsigned* s1 = reinterpret_cast<const unsigned*>(s);
      unsigned* d1 = reinterpret_cast<unsigned*>(d);
      for (size_t j = tid; j < nb / 4; j += nth) {
        const unsigned v = s1[j];
        if (d) d1[j] = v; else acc ^= v;
      }
    }
  }
  if (acc == 0x9E3779B9u && sink) *sink = acc;
}

// holds the stream until `ticks` wall-clock ticks after the stamp k_loop_copy left: the modelled wire time of the exchange
__global__ void k_loop_wait(const unsigned long long* __restrict__ stamp, unsigned long long ticks) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = *stamp;
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
  }
}

}  // namespace dfh

using namespace dfh;

struct dfh_comm {
  dfh_ctx* ctx = nullptr;
  int rank = 0, world = 1;
  void* rccl = nullptr;                 // ncclComm_t, or
  dfh_alltoallv_fn fn = nullptr;        // host callback
  void* user = nullptr;
  char* h_send = nullptr;               // pinned staging of the callback transport
  char* h_recv = nullptr;
  size_t h_cap = 0;
  // payload this rank handed to / took from OTHER ranks since the last reset, and the message groups it took
  uint64_t bytes_sent = 0, bytes_recv = 0, groups = 0;
  // loop-back transport (measurement): fed sources per kind of exchange, the wire model
  bool loopback = false;
  std::deque<const void*> feed[DFH_XCHG_KINDS];
  const void* sticky[DFH_XCHG_KINDS] = {nullptr};
  unsigned long long* d_stamp = nullptr;   // [0]: wall clock at the start of the current exchange's copies; [1]: sink
  double link_gbps = 0, latency_us = 0;
  double wall_khz = 100000.0;              // hipDeviceAttributeWallClockRate
  double wire_us_sum = 0;                  // modelled wire time of all exchanges since the last stats reset
};

namespace {

// one part of an exchange: per peer p, send_b[p] bytes from d_send + send_off[p] and recv_b[p] bytes into
// d_recv + recv_off[p] (offsets NULL: contiguous in peer order)
struct XPart {
  const void* d_send;
  const size_t* send_b;
  const size_t* send_off;
  void* d_recv;
  const size_t* recv_b;
  const size_t* recv_off;
};

// alltoallv of device buffers; nparts parts would share ONE message group (callers pass one part: one send and
// one receive per peer and group)
int comm_exchange(dfh_comm* c, const XPart* parts, int nparts, hipStream_t on = nullptr, int kind = DFH_XCHG_OTHER) {
  hipStream_t s = on ? on : c->ctx->stream;
  const int W = c->world;
  for (int i = 0; i < nparts; ++i)
    for (int p = 0; p < W; ++p)
      if (p != c->rank) {
        c->bytes_sent += parts[i].send_b[p];
        c->bytes_recv += parts[i].recv_b[p];
      }
  ++c->groups;
  if (c->loopback) {
    // every message of the exchange as a device copy of its exact size, one launch per part
    for (int i = 0; i < nparts; ++i) {
      const XPart& x = parts[i];
      const char* fed = nullptr;
      if (!c->feed[kind].empty()) {
        fed = static_cast<const char*>(c->feed[kind].front());
        c->feed[kind].pop_front();
      } else if (c->sticky[kind]) {
        fed = static_cast<const char*>(c->sticky[kind]);
      }
      LoopSegs g;
      g.n = 0;
      size_t so = 0, ro = 0, total = 0, largest = 0;
      for (int p = 0; p < W; ++p) {
        const size_t sp = x.send_off ? x.send_off[p] : so, rp = x.recv_off ? x.recv_off[p] : ro;
        const size_t sb = x.send_b[p], rb = x.recv_b[p];
        if (p == c->rank) {  // the rank's own slot: a real self-copy
          const size_t nb = std::min(sb, rb);
          if (nb) {
            g.src[g.n] = static_cast<const char*>(x.d_send) + sp;
            g.dst[g.n] = static_cast<char*>(x.d_recv) + rp;
            g.bytes[g.n++] = nb;
          }
        } else {
          if (sb) {  // out: read and dropped
            g.src[g.n] = static_cast<const char*>(x.d_send) + sp;
            g.dst[g.n] = nullptr;
            g.bytes[g.n++] = sb;
          }
          if (rb) {  // in: from the fed source (laid out like the receive side), or an echo of what this rank sends
            g.src[g.n] = fed ? fed + rp : static_cast<const char*>(x.d_send) + sp;
            g.dst[g.n] = static_cast<char*>(x.d_recv) + rp;
            g.bytes[g.n++] = fed ? rb : std::min(sb, rb);
            if (!g.bytes[g.n - 1]) --g.n;
          }
          largest = std::max(largest, std::max(sb, rb));
        }
        total += sb + rb;
        so += sb;
        ro += rb;
      }
      if (!total) continue;
      const int blocks = (int)std::min<size_t>(1024, std::max<size_t>(1, total / (256 * 64)));
      hipLaunchKernelGGL(k_loop_copy, dim3(blocks), dim3(256), 0, s, g, c->d_stamp, reinterpret_cast<unsigned*>(c->d_stamp + 1));
      DFH_HIP(hipGetLastError());
      if (c->link_gbps > 0 && largest) {
        const double us = c->latency_us + (double)largest / (c->link_gbps * 1e3);
        c->wire_us_sum += us;
        hipLaunchKernelGGL(k_loop_wait, dim3(1), dim3(64), 0, s, c->d_stamp, (unsigned long long)(us * 1e-3 * c->wall_khz));
        DFH_HIP(hipGetLastError());
      }
    }
    return DFH_OK;
  }
  if (c->rccl) {
    RcclApi* a = rccl_api();
    bool any = false;
    for (int i = 0; i < nparts && !any; ++i)
      for (int p = 0; p < W; ++p) any = any || parts[i].send_b[p] || parts[i].recv_b[p];
    if (!any) return DFH_OK;
    DFH_RCCL(a->GroupStart());
    for (int i = 0; i < nparts; ++i) {
      const XPart& x = parts[i];
      size_t so = 0, ro = 0;
      for (int p = 0; p < W; ++p) {
        const size_t sp = x.send_off ? x.send_off[p] : so, rp = x.recv_off ? x.recv_off[p] : ro;
        if (x.send_b[p]) DFH_RCCL(a->Send(static_cast<const char*>(x.d_send) + sp, x.send_b[p], 0 /* ncclChar */, p, c->rccl, s));
        if (x.recv_b[p]) DFH_RCCL(a->Recv(static_cast<char*>(x.d_recv) + rp, x.recv_b[p], 0, p, c->rccl, s));
        so += x.send_b[p];
        ro += x.recv_b[p];
      }
    }
    DFH_RCCL(a->GroupEnd());
    return DFH_OK;
  }
  // host callback: every part staged contiguously through pinned memory
  for (int i = 0; i < nparts; ++i) {
    const XPart& x = parts[i];
    size_t st = 0, rt = 0;
    for (int p = 0; p < W; ++p) {
      st += x.send_b[p];
      rt += x.recv_b[p];
    }
    const size_t need = std::max(st, rt);
    if (need > c->h_cap) {
      if (c->h_send) DFH_HIP(hipHostFree(c->h_send));
      if (c->h_recv) DFH_HIP(hipHostFree(c->h_recv));
      c->h_send = c->h_recv = nullptr;
      c->h_cap = 0;
      const size_t cap = std::max<size_t>(need * 2, 1 << 16);
      DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->h_send), cap, hipHostMallocDefault));
      DFH_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->h_recv), cap, hipHostMallocDefault));
      c->h_cap = cap;
    }
    size_t so = 0, ro = 0;
    for (int p = 0; p < W; ++p) {
      const size_t sp = x.send_off ? x.send_off[p] : so;
      if (x.send_b[p])
        DFH_HIP(hipMemcpyAsync(c->h_send + so, static_cast<const char*>(x.d_send) + sp, x.send_b[p], hipMemcpyDeviceToHost, s));
      so += x.send_b[p];
    }
    DFH_HIP(hipStreamSynchronize(s));
    if (c->fn(c->user, c->h_send, x.send_b, c->h_recv, x.recv_b) != 0) {
      set_error("dfh_comm: the host exchange callback failed");
      return DFH_ERR_HIP;
    }
    for (int p = 0; p < W; ++p) {
      const size_t rp = x.recv_off ? x.recv_off[p] : ro;
      if (x.recv_b[p])
        DFH_HIP(hipMemcpyAsync(static_cast<char*>(x.d_recv) + rp, c->h_recv + ro, x.recv_b[p], hipMemcpyHostToDevice, s));
      ro += x.recv_b[p];
    }
    // h_recv is reused by the next part: its copies must have left it
    if (i + 1 < nparts) DFH_HIP(hipStreamSynchronize(s));
  }
  return DFH_OK;
}

int comm_alltoallv(dfh_comm* c, const void* d_send, const size_t* send_b, void* d_recv, const size_t* recv_b, hipStream_t on = nullptr,
                   int kind = DFH_XCHG_OTHER) {
  XPart x{d_send, send_b, nullptr, d_recv, recv_b, nullptr};
  return comm_exchange(c, &x, 1, on, kind);
}

// ---- The host-staged exchange: host bytes over the communicator, staged through device memory on the context's stream:
// the send bytes host -> device, ONE comm_exchange (one message group), the received bytes device -> host, and the wait
// for the stream (NO_WAIT: left to the caller — dfh_comm_selfcheck, which must not block, polls the stream).  Peer p is sent
// send_b[p] bytes from send + send_off[p] (send_off NULL: one peer's bytes after the other's); `recv` takes the peers'
// recv_b[p] bytes one after the other.  Two buffer policies: SCRATCH carves the device buffers from the context's scratch
// (no allocation once it has the size: the calls made per iteration or epoch); TRANSIENT allocates them for this one exchange
// and frees them when the object goes, on every path (set-up exchanges of whole key lists: the scratch must not grow for good).
struct HostXchg {
  enum Buffers { SCRATCH, TRANSIENT };
  enum { NO_WAIT = 1, CLEAR_RECV = 2 };  // CLEAR_RECV: the device receive buffer is zeroed first (bytes that never arrive read as zeros)
  dfh_comm* c;
  const char* who;  // the caller's name, for the error text
  Buffers buffers;
  char *d_s = nullptr, *d_r = nullptr;
  ~HostXchg() {
    if (buffers != TRANSIENT || !d_s) return;
    (void)hipStreamSynchronize(c->ctx->stream);  // a copy queued before a failure may still use them
    (void)hipFree(d_s);
    if (d_r) (void)hipFree(d_r);
  }
  int hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return DFH_OK;
    set_error(std::string(who) + ": " + what + " of the host-staged exchange: " + hipGetErrorString(e));
    return DFH_ERR_HIP;
  }
  // recv_align: the peers' receive slots on the device start at multiples of it (1: one after the other)
  int exchange(const void* send, const size_t* send_b, const size_t* send_off, void* recv, const size_t* recv_b, int kind,
               size_t recv_align = 1, int flags = 0) {
    dfh_ctx* ctx = c->ctx;
    hipStream_t s = ctx->stream;
    const int W = c->world;
    int rc;
    if ((rc = hip(hipSetDevice(ctx->device), "hipSetDevice"))) return rc;
    size_t st = 0, rt = 0, roff[32];  // device bytes of the two sides, every peer's receive slot (at most 32 ranks)
    for (int p = 0; p < W; ++p) {
      st = send_off ? std::max(st, send_off[p] + send_b[p]) : st + send_b[p];
      roff[p] = rt;
      rt += (recv_b[p] + recv_align - 1) / recv_align * recv_align;
    }
    if (buffers == SCRATCH) {
      if ((rc = ensure_scratch(ctx, st + rt + 512))) return rc;
      Carver cv(ctx->scratch);
      d_s = cv.take<char>(st);
      d_r = cv.take<char>(rt);
    } else {  // (a failed hipMalloc leaves its pointer NULL: the destructor frees the first buffer when the second fails)
      if ((rc = hip(hipMalloc(reinterpret_cast<void**>(&d_s), std::max<size_t>(st, 16)), "the send buffer"))) return rc;
      if ((rc = hip(hipMalloc(reinterpret_cast<void**>(&d_r), std::max<size_t>(rt, 16)), "the receive buffer"))) return rc;
    }
    if (st && (rc = hip(hipMemcpyAsync(d_s, send, st, hipMemcpyHostToDevice, s), "the upload"))) return rc;
    if ((flags & CLEAR_RECV) && (rc = hip(hipMemsetAsync(d_r, 0, rt, s), "the clearing"))) return rc;
    const XPart x{d_s, send_b, send_off, d_r, recv_b, roff};
    if ((rc = comm_exchange(c, &x, 1, nullptr, kind))) return rc;
    char* h = static_cast<char*>(recv);
    if (recv_align == 1 && rt) rc = hip(hipMemcpyAsync(h, d_r, rt, hipMemcpyDeviceToHost, s), "the download");  // one copy: the slots lie as the host wants them
    for (int p = 0; recv_align != 1 && p < W && !rc; h += recv_b[p++])
      if (recv_b[p]) rc = hip(hipMemcpyAsync(h, d_r + roff[p], recv_b[p], hipMemcpyDeviceToHost, s), "the download");
    return rc || (flags & NO_WAIT) ? rc : hip(hipStreamSynchronize(s), "the wait");
  }
};

}  // namespace

extern "C" {

int dfh_comm_unique_id(void* id128) {
  DFH_ARG(id128, "dfh_comm_unique_id: NULL argument");
  RcclApi* a = rccl_api();
  if (!a) {
    set_error("RCCL is not available (librccl.so.1 could not be loaded)");
    return DFH_ERR_HIP;
  }
  RcclId id;
  DFH_RCCL(a->GetUniqueId(&id));
  memcpy(id128, id.internal, sizeof(id.internal));
  return DFH_OK;
}

int dfh_comm_create_rccl(dfh_ctx* ctx, int rank, int world, const void* id128, dfh_comm** out) {
  DFH_ARG(ctx && id128 && out && world >= 1 && world <= 32 && rank >= 0 && rank < world,
          "dfh_comm_create_rccl: bad argument (1 <= world <= 32)");
  RcclApi* a = rccl_api();
  if (!a) {
    set_error("RCCL is not available (librccl.so.1 could not be loaded)");
    return DFH_ERR_HIP;
  }
  DFH_HIP(hipSetDevice(ctx->device));
  RcclId id;
  memcpy(id.internal, id128, sizeof(id.internal));
  void* comm = nullptr;
  DFH_RCCL(a->CommInitRank(&comm, world, id, rank));
  dfh_comm* c = new (std::nothrow) dfh_comm();
  DFH_ARG(c != nullptr, "out of host memory");
  c->ctx = ctx;
  c->rank = rank;
  c->world = world;
  c->rccl = comm;
  *out = c;
  return DFH_OK;
}

int dfh_comm_create_callback(dfh_ctx* ctx, int rank, int world, dfh_alltoallv_fn fn, void* user, dfh_comm** out) {
  DFH_ARG(ctx && fn && out && world >= 1 && world <= 32 && rank >= 0 && rank < world,
          "dfh_comm_create_callback: bad argument (1 <= world <= 32)");
  dfh_comm* c = new (std::nothrow) dfh_comm();
  DFH_ARG(c != nullptr, "out of host memory");
  c->ctx = ctx;
  c->rank = rank;
  c->world = world;
  c->fn = fn;
  c->user = user;
  *out = c;
  return DFH_OK;
}

int dfh_comm_create_loopback(dfh_ctx* ctx, int rank, int world, dfh_comm** out) {
  DFH_ARG(ctx && out && world >= 1 && world <= 32 && rank >= 0 && rank < world, "dfh_comm_create_loopback: bad argument (1 <= world <= 32)");
  DFH_HIP(hipSetDevice(ctx->device));
  dfh_comm* c = new (std::nothrow) dfh_comm();
  DFH_ARG(c != nullptr, "out of host memory");
  c->ctx = ctx;
  c->rank = rank;
  c->world = world;
  c->loopback = true;
  if (hipMalloc(reinterpret_cast<void**>(&c->d_stamp), 2 * sizeof(unsigned long long)) != hipSuccess) {
    delete c;
    set_error("dfh_comm_create_loopback: hipMalloc failed");
    return DFH_ERR_HIP;
  }
  (void)hipMemset(c->d_stamp, 0, 2 * sizeof(unsigned long long));
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) == hipSuccess && khz > 0) c->wall_khz = khz;
  *out = c;
  return DFH_OK;
}

int dfh_comm_loopback_feed(dfh_comm* c, int kind, const void* d_src, int sticky) {
  DFH_ARG(c && c->loopback && kind >= 0 && kind < DFH_XCHG_KINDS, "dfh_comm_loopback_feed: a loop-back communicator and a DFH_XCHG_* kind");
  if (sticky) {
    c->sticky[kind] = d_src;
  } else {
    DFH_ARG(d_src, "dfh_comm_loopback_feed: NULL source");
    c->feed[kind].push_back(d_src);
  }
  return DFH_OK;
}

int dfh_comm_loopback_wire(dfh_comm* c, double link_gbps, double latency_us) {
  DFH_ARG(c && c->loopback && link_gbps >= 0 && latency_us >= 0, "dfh_comm_loopback_wire: a loop-back communicator, link_gbps >= 0, latency_us >= 0");
  c->link_gbps = link_gbps;
  c->latency_us = latency_us;
  return DFH_OK;
}

int dfh_comm_loopback_wire_time(dfh_comm* c, int reset, double* us) {
  DFH_ARG(c && c->loopback && us, "dfh_comm_loopback_wire_time: bad argument");
  *us = c->wire_us_sum;
  if (reset) c->wire_us_sum = 0;
  return DFH_OK;
}

int dfh_comm_destroy(dfh_comm* c) {
  if (!c) return DFH_OK;
  hipSetDevice(c->ctx->device);
  hipStreamSynchronize(c->ctx->stream);
  if (c->d_stamp) {
    hipDeviceSynchronize();  // exchanges of the collectives' stream may still read the stamp
    hipFree(c->d_stamp);
  }
  if (c->rccl) {
    RcclApi* a = rccl_api();
    if (a) a->CommDestroy(c->rccl);
  }
  if (c->h_send) hipHostFree(c->h_send);
  if (c->h_recv) hipHostFree(c->h_recv);
  delete c;
  return DFH_OK;
}

int dfh_comm_rank(dfh_comm* c) { return c ? c->rank : -1; }
int dfh_comm_world(dfh_comm* c) { return c ? c->world : 0; }

int dfh_comm_allreduce_sum(dfh_comm* c, double* vals, int n) {
  DFH_ARG(c && vals && n >= 1 && n <= 64, "dfh_comm_allreduce_sum: 1 <= n <= 64 host doubles");
  const int W = c->world;
  std::vector<size_t> cnt(W, (size_t)n * sizeof(double));
  std::vector<double> h((size_t)W * n);
  for (int p = 0; p < W; ++p) memcpy(&h[(size_t)p * n], vals, cnt[p]);
  const int rc = HostXchg{c, "dfh_comm_allreduce_sum", HostXchg::SCRATCH}.exchange(h.data(), cnt.data(), nullptr, h.data(), cnt.data(), DFH_XCHG_OTHER);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    double s = 0;
    for (int p = 0; p < W; ++p) s += h[(size_t)p * n + i];  // rank order: the same sum on every rank
    vals[i] = s;
  }
  return DFH_OK;
}

int dfh_comm_stats(dfh_comm* c, int reset, uint64_t* bytes_sent, uint64_t* bytes_recv, uint64_t* groups) {
  DFH_ARG(c, "dfh_comm_stats: NULL communicator");
  if (bytes_sent) *bytes_sent = c->bytes_sent;
  if (bytes_recv) *bytes_recv = c->bytes_recv;
  if (groups) *groups = c->groups;
  if (reset) c->bytes_sent = c->bytes_recv = c->groups = 0;
  return DFH_OK;
}

int dfh_comm_info(dfh_comm* c, char* buf, size_t n) {
  DFH_ARG(c && buf && n >= 1, "dfh_comm_info: bad argument");
  std::string t;
  if (c->rccl) {
    RcclApi* a = rccl_api();
    int v = 0;
    if (a && a->GetVersion) a->GetVersion(&v);
    t = "rccl " + std::to_string(v) + " from " + (a ? a->path : std::string("?")) +
        (a && a->was_loaded ? " (already loaded by the host process)" : " (loaded by libdifacto_hip)");
  } else if (c->loopback) {
    char w[160];
    snprintf(w, sizeof w, "loop-back transport (measurement: rank %d of %d alone on its GPU; wire model %s", c->rank, c->world,
             c->link_gbps > 0 ? "" : "off)");
    t = w;
    if (c->link_gbps > 0) {
      snprintf(w, sizeof w, "%.1f GB/s per link and direction + %.1f us per exchange)", c->link_gbps, c->latency_us);
      t += w;
    }
  } else {
    t = "host callback transport";
  }
  snprintf(buf, n, "%s", t.c_str());
  return DFH_OK;
}

// start-up self-check: every rank contributes rank + 1 to an all-to-all and must read world (world + 1) / 2 back.
// The exchange is queued and then POLLED: a peer that never joined (bad rendezvous, wrong world size, a dead rank)
// makes this return DFH_ERR_STATE after timeout_s seconds instead of hanging the job in its first step.
int dfh_comm_selfcheck(dfh_comm* c, double timeout_s) {
  DFH_ARG(c && timeout_s > 0, "dfh_comm_selfcheck: bad argument");
  if (c->loopback) return DFH_OK;  // there are no peers to hear from
  const int W = c->world;
  std::vector<double> h(W, (double)(c->rank + 1));
  std::vector<size_t> cnt(W, sizeof(double));
  const int rc = HostXchg{c, "dfh_comm_selfcheck", HostXchg::SCRATCH}.exchange(h.data(), cnt.data(), nullptr, h.data(), cnt.data(), DFH_XCHG_OTHER, 1,
                                                                              HostXchg::NO_WAIT | HostXchg::CLEAR_RECV);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipStreamQuery(c->ctx->stream);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) {
      set_error(std::string("dfh_comm_selfcheck: ") + hipGetErrorString(q));
      return DFH_ERR_HIP;
    }
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
      set_error("dfh_comm_selfcheck: the first exchange did not complete within " + std::to_string((int)timeout_s) +
                " s — a rank is missing or the rendezvous is wrong (rank " + std::to_string(c->rank) + " of " + std::to_string(W) + ")");
      return DFH_ERR_STATE;
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(2));
  }
  double sum = 0;
  for (int p = 0; p < W; ++p) sum += h[p];
  if (sum != 0.5 * W * (W + 1)) {
    set_error("dfh_comm_selfcheck: the ranks' ids do not add up (got " + std::to_string(sum) + "): duplicate or missing ranks");
    return DFH_ERR_STATE;
  }
  return DFH_OK;
}

// What do the wires give?  `reps` grouped exchanges in which this rank sends bytes_per_peer to and receives bytes_per_peer
// from EVERY other rank (the shape of dfh_shard_step's K / RW / G exchanges: on a full xGMI mesh every link carries one
// message each way at once), timed with HIP events on the context's stream after two untimed ones.  *us_per_exchange: the
// average; bytes_per_peer / that = what one link gave per direction.  COLLECTIVE.  The projection of DESIGN 6a rests on an
// assumed link rate: with this the first run on a real node replaces the assumption by itself (bench.py --gpus N).
int dfh_comm_wire_probe(dfh_comm* c, size_t bytes_per_peer, int reps, double* us_per_exchange) {
  DFH_ARG(c && us_per_exchange && bytes_per_peer >= 1 && bytes_per_peer <= ((size_t)1 << 30) && reps >= 1 && reps <= 1000,
          "dfh_comm_wire_probe: 1 <= bytes_per_peer <= 1 GiB, 1 <= reps <= 1000");
  dfh_ctx* ctx = c->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int W = c->world;
  *us_per_exchange = 0;
  if (W < 2) return DFH_OK;
  char *d_s = nullptr, *d_r = nullptr;
  const size_t total = (size_t)W * bytes_per_peer;
  if (hipMalloc(reinterpret_cast<void**>(&d_s), total) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d_r), total) != hipSuccess) {
    if (d_s) (void)hipFree(d_s);
    (void)hipGetLastError();
    set_error("dfh_comm_wire_probe: no device memory for the probe's buffers");
    return DFH_ERR_HIP;
  }
  std::vector<size_t> cnt(W, bytes_per_peer);
  cnt[c->rank] = 0;   // nothing to itself: the wires are what is measured
  const uint64_t bs = c->bytes_sent, br = c->bytes_recv, gr = c->groups;   // the probe is not part of the job's statistics
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = DFH_OK;
  auto fail = [&](hipError_t e) {
    if (e != hipSuccess && rc == DFH_OK) {
      set_error(std::string("dfh_comm_wire_probe: ") + hipGetErrorString(e));
      rc = DFH_ERR_HIP;
    }
  };
  fail(hipMemsetAsync(d_s, 1, total, ctx->stream));
  fail(hipEventCreate(&e0));
  fail(hipEventCreate(&e1));
  // (offsets spelled out: a peer's slot is W-indexed although this rank's own slot carries nothing)
  std::vector<size_t> off(W);
  for (int p = 0; p < W; ++p) off[p] = (size_t)p * bytes_per_peer;
  XPart x{d_s, cnt.data(), off.data(), d_r, cnt.data(), off.data()};
  for (int i = 0; i < 2 && rc == DFH_OK; ++i) rc = comm_exchange(c, &x, 1);
  const auto t0 = std::chrono::steady_clock::now();
  if (rc == DFH_OK) fail(hipEventRecord(e0, ctx->stream));
  for (int i = 0; i < reps && rc == DFH_OK; ++i) rc = comm_exchange(c, &x, 1);
  if (rc == DFH_OK) fail(hipEventRecord(e1, ctx->stream));
  if (rc == DFH_OK) fail(hipStreamSynchronize(ctx->stream));
  if (rc == DFH_OK) {
    float ms = 0;
    fail(hipEventElapsedTime(&ms, e0, e1));
    // the host-callback transport exchanges on the host between two drains of the stream: its time is the host's
    const double host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    *us_per_exchange = (c->fn ? host_us : (double)ms * 1e3) / reps;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(d_s);
  (void)hipFree(d_r);
  c->bytes_sent = bs;
  c->bytes_recv = br;
  c->groups = gr;
  return rc;
}

int dfh_comm_allgather(dfh_comm* c, const void* send, size_t bytes, void* recv) {
  DFH_ARG(c && send && recv && bytes >= 1 && bytes <= (1u << 24), "dfh_comm_allgather: 1 <= bytes <= 16 MiB of host memory");
  // the same bytes to every peer: W sends out of one buffer (offsets all zero), W receives side by side in 16 B aligned slots
  std::vector<size_t> cnt(c->world, bytes), zero(c->world, 0);
  return HostXchg{c, "dfh_comm_allgather", HostXchg::SCRATCH}.exchange(send, cnt.data(), zero.data(), recv, cnt.data(), DFH_XCHG_OTHER, 16);
}

}  // extern "C"
#endif  // DFH_COMM_HIP_
