// gpu_exchange.hip -- the exchanges between ranks behind the C ABI of include/cfdproxy_hip.h: grouped RCCL send/recv
// issued by the library itself, the xGMI write + notify exchange through HIP IPC (set-up, step schedules, hipGraph
// replays), and the scaled-field validation of either.  Context and launch helpers: gpu_ctx.h / gpu_abi.hip.
#include "gpu_ctx.h"

#include <dlfcn.h>
#include <unistd.h>

extern "C" {

// ----------------------------------------------------- scaled-field validation of the exchange
// See gg_validate_kernel.  begin: the flux the context holds NOW (from an iteration whose exchange the caller knows to be
// complete: device syncs and a barrier between the ranks, then one step without exchange) becomes the reference; from
// then on every step entry point (cfdp_gpu_step_post, _step_ipc*, _run_steps_*, _rank_flux; the drop-in layer's
// compute_psd_flux) ends with the validation kernel: compare the flux the step produced with reference * 2^e, then
// var *= 2, 2, 1/4, ...  Every step must exchange and compute the flux while the mode is on.  end: the deferred flux of
// the last iteration is compared too, var is restored exactly, the evidence is returned.
extern "C++" void cfdp_detail::drop_ipc_graphs(cfdp_gpu *g) { g->ipc.drop_graph_sets(); }

int cfdp_gpu_scaled_check_begin(cfdp_gpu *g) {
  NEED_UPLOAD(g);
  if (g->sc.on) return fail("the scaled-field validation is already on");
  if (flush_flux(g)) return 1;
  HIP_TRY(hipDeviceSynchronize());
  const size_t nf = (size_t)g->nown * 3;
  if (!g->sc.d_state) HIP_TRY(hipMalloc(&g->sc.d_state, GG_V_WORDS * sizeof(int)));
  if (!g->sc.d_fref) HIP_TRY(hipMalloc(&g->sc.d_fref, (nf + 1) * sizeof(double)));
  if (!g->sc.d_skip && !g->faceless.empty()) {
    std::vector<unsigned char> skip((size_t)g->nown, 0);
    for (int i : g->faceless) skip[(size_t)i] = 1;
    HIP_TRY(hipMalloc(&g->sc.d_skip, skip.size()));
    HIP_TRY(hipMemcpy(g->sc.d_skip, skip.data(), skip.size(), hipMemcpyHostToDevice));
  }
  HIP_TRY(cfdp_memset_sync(g->sc.d_state, 0, GG_V_WORDS * sizeof(int)));
  if (!g->sc.d_var0) HIP_TRY(hipMalloc(&g->sc.d_var0, sizeof(double) * 8 * (size_t)g->nall));
  HIP_TRY(cfdp_copy_d2d_sync(g->sc.d_var0, g->d_var, sizeof(double) * 8 * (size_t)g->nall));
  // bit for bit: the reference must come from the kernel form the steps will use.  The flux phase of the fused pass
  // sums a point's faces on 4 lanes, the separate flux kernel by default on 8 (another association): with fused
  // iterations on, the separate kernel -- reference now, last iteration's deferred flux later -- runs on 4 as well
  g->sc.saved_flux_lanes = g->flux_lanes;
  if (g->fusion && g->d_grad_alt) g->flux_lanes = 4;
  if (launch_flux(g, g->last_flux_mode, g->s_main)) return 1;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(cfdp_copy_d2d_sync(g->sc.d_fref, g->d_flux, nf * sizeof(double)));
  g->sc.on = true;
  g->drop_graphs();  // graphs captured without the validation kernel
  drop_ipc_graphs(g);
  return 0;
}

int cfdp_gpu_scaled_check_end(cfdp_gpu *g, cfdp_scaled_check *out) {
  NEED_UPLOAD(g);
  if (!g->sc.on) return fail("the scaled-field validation is not on");
  const int rc = flush_flux(g);  // compares the last iteration's flux as well
  g->sc.on = false;
  g->flux_lanes = g->sc.saved_flux_lanes;
  const hipError_t es = hipDeviceSynchronize();  // (a graph that is still replaying must not be destroyed under it)
  g->drop_graphs();
  drop_ipc_graphs(g);
  if (rc) return 1;
  HIP_TRY(es);
  int st[GG_V_WORDS];
  HIP_TRY(hipMemcpy(st, g->sc.d_state, sizeof st, hipMemcpyDeviceToHost));
  const int m = st[GG_V_ITER] % 3;  // var holds var0 * 2^m -- verified: a verdict from a mode whose own bookkeeping slipped is void
  unsigned long long var_bad = 0;
  {
    unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(g->sc.d_state + 12);  // (words 12..13 of the state block)
    HIP_TRY(cfdp_memset_sync(d_bad, 0, sizeof(unsigned long long)));
    HIP_TRY(gg_launch_var_check(g->d_var, g->sc.d_var0, g->nall, m == 0 ? 1.0 : (m == 1 ? 2.0 : 4.0), d_bad, g->s_main));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&var_bad, d_bad, sizeof var_bad, hipMemcpyDeviceToHost));
  }
  // restore exactly (from the copy: also right if the bookkeeping slipped)
  HIP_TRY(cfdp_copy_d2d_sync(g->d_var, g->sc.d_var0, sizeof(double) * 8 * (size_t)g->nall));
  if (out) {
    unsigned long long bad = 0;
    memcpy(&bad, &st[GG_V_BAD], sizeof bad);
    out->iterations = st[GG_V_ITER];
    out->flux_checks = st[GG_V_CHECKS];
    out->mismatches = bad > 0x7FFFFFFFull ? 0x7FFFFFFF : (int)bad;
    out->var_mismatches = var_bad > 0x7FFFFFFFull ? 0x7FFFFFFF : (int)var_bad;
    out->first_iteration = st[GG_V_CLAIM] ? st[GG_V_FIRST_ITER] : 0;
    out->first_point = st[GG_V_CLAIM] ? g->new2old[(size_t)(st[GG_V_FIRST_IDX] / 3)] : -1;
    out->first_component = st[GG_V_CLAIM] ? st[GG_V_FIRST_IDX] % 3 : -1;
    out->seen = out->expected = 0.0;
    if (st[GG_V_CLAIM]) {
      memcpy(&out->seen, &st[GG_V_SEEN], sizeof(double));
      memcpy(&out->expected, &st[GG_V_EXPECT], sizeof(double));
    }
  }
  return 0;
}

// ------------------------------------------------------- one process per GPU: RCCL from C
// The halo exchange of a step issued straight from this library: one ncclGroup of
// ncclSend/ncclRecv per iteration on the context's comm stream, between the two step brackets
// -- the analogue of exchange_dbl_mpi_send / _post_recv (src/exchange_data_mpi.c:96-166) with
// the receive side being the ghost block itself.  A host pays ONE call per iteration (or one
// per hipGraph replay of several).  RCCL is resolved at run time from the library the process
// already uses (PyTorch ships its own librccl.so; a C host names the system one), so this
// library has no link-time dependency on it.
namespace {
struct rccl_api {
  void *lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
} rccl;

#define RCCL_TRY(expr)                                                                              \
  do {                                                                                              \
    ncclResult_t r_ = (expr);                                                                       \
    if (r_ != ncclSuccess)                                                                          \
      return fail("%s failed: %s [%s:%d]", #expr, rccl.GetErrorString ? rccl.GetErrorString(r_) : "?", \
                  __FILE__, __LINE__);                                                              \
  } while (0)

// this iteration's messages: sends from the packed arena, receives into the current ghost block
int enqueue_exchange(cfdp_gpu *g) {
  if (g->comm_nranks == 1 && !g->partner.empty() && !g->rccl_self_exchange)
    return fail("the communicator has ONE rank: this exchange would send every partner's rows to the rank itself (for loopback "
                "measurements say so first: cfdp_gpu_rccl_allow_self_exchange)");
  RCCL_TRY(rccl.GroupStart());
  for (size_t s = 0; s < g->partner.size(); s++) {
    size_t sb = 0, rb = 0;
    void *sp = cfdp_gpu_send_ptr(g, (int)s, &sb), *rp = cfdp_gpu_recv_ptr(g, (int)s, &rb);
    // MEASUREMENT ONLY, asked for by name (cfdp_gpu_rccl_allow_self_exchange): a communicator of ONE rank exchanges with
    // itself (the fall-back transport priced on one GPU, bench.py's loopback table; the plumbing test): a send must then
    // meet a receive of its own length
    if (g->comm_nranks == 1 && g->rccl_self_exchange) sb = rb = sb < rb ? sb : rb;
    if (sb) RCCL_TRY(rccl.Send(sp, sb / sizeof(double), ncclDouble, g->peer[s], g->comm, g->s_comm));
    if (rb) RCCL_TRY(rccl.Recv(rp, rb / sizeof(double), ncclDouble, g->peer[s], g->comm, g->s_comm));
  }
  RCCL_TRY(rccl.GroupEnd());
  return 0;
}

}  // namespace

// the same messages for another per-point field (the adjoint's gbar rows and volumes: csrc/gpu_adjoint.hip)
extern "C++" int cfdp_detail::rccl_exchange_rows(cfdp_gpu *g, const double *send, double *recv, int rowlen, hipStream_t st) {
  if (!g->comm) return fail("no communicator: call cfdp_gpu_rccl_init()");
  if (g->comm_nranks == 1 && !g->partner.empty() && !g->rccl_self_exchange)
    return fail("the communicator has ONE rank: this exchange would send every partner's rows to the rank itself (for loopback "
                "measurements say so first: cfdp_gpu_rccl_allow_self_exchange)");
  RCCL_TRY(rccl.GroupStart());
  for (size_t s = 0; s < g->partner.size(); s++) {
    size_t sn = (size_t)(g->send_off[s + 1] - g->send_off[s]) * rowlen, rn = (size_t)(g->recv_off[s + 1] - g->recv_off[s]) * rowlen;
    if (g->comm_nranks == 1 && g->rccl_self_exchange) sn = rn = sn < rn ? sn : rn;  // (measurement / plumbing only, as above)
    if (sn) RCCL_TRY(rccl.Send(send + (size_t)g->send_off[s] * rowlen, sn, ncclDouble, g->peer[s], g->comm, st));
    if (rn) RCCL_TRY(rccl.Recv(recv + (size_t)g->recv_off[s] * rowlen, rn, ncclDouble, g->peer[s], g->comm, st));
  }
  RCCL_TRY(rccl.GroupEnd());
  return 0;
}

namespace {
int one_step(cfdp_gpu *g, int with_exchange, int overlap, int with_flux, int flux_mode) {
  if (cfdp_gpu_step_pre(g, with_exchange, overlap)) return 1;
  if (g->pending_exchange && enqueue_exchange(g)) return 1;
  return cfdp_gpu_step_post(g, with_flux, flux_mode);
}
}  // namespace

int cfdp_rccl_load(const char *libpath) {
  if (rccl.lib) return 0;
  const char *names[] = {libpath, "librccl.so.1", "librccl.so"};
  for (const char *n : names) {
    if (!n || !*n) continue;
    rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (rccl.lib) break;
  }
  if (!rccl.lib) return fail("cannot load RCCL (%s): %s", libpath ? libpath : "librccl.so.1", dlerror());
#define RCCL_SYM(field, name)                                                      \
  do {                                                                             \
    *(void **)(&rccl.field) = dlsym(rccl.lib, name);                               \
    if (!rccl.field) { rccl.lib = nullptr; return fail("RCCL symbol %s not found", name); } \
  } while (0)
  RCCL_SYM(GetUniqueId, "ncclGetUniqueId");
  RCCL_SYM(CommInitRank, "ncclCommInitRank");
  RCCL_SYM(CommDestroy, "ncclCommDestroy");
  RCCL_SYM(CommCount, "ncclCommCount");
  RCCL_SYM(GroupStart, "ncclGroupStart");
  RCCL_SYM(GroupEnd, "ncclGroupEnd");
  RCCL_SYM(Send, "ncclSend");
  RCCL_SYM(Recv, "ncclRecv");
  RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef RCCL_SYM
  return 0;
}

int cfdp_rccl_unique_id(void *id128) {
  if (!rccl.lib) return fail("cfdp_rccl_load() has not been called");
  if (!id128) return fail("null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  RCCL_TRY(rccl.GetUniqueId(static_cast<ncclUniqueId *>(id128)));
  return 0;
}

int cfdp_gpu_rccl_init(cfdp_gpu *g, const void *id128, int nranks, int rank, const int *rank_of_partner) {
  NEED_UPLOAD(g);
  if (!rccl.lib) return fail("cfdp_rccl_load() has not been called");
  if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail("bad communicator arguments");
  if (g->comm) return fail("this context already has a communicator");
  g->peer.resize(g->partner.size());
  for (size_t s = 0; s < g->partner.size(); s++) {
    g->peer[s] = rank_of_partner ? rank_of_partner[s] : g->partner[s];
    if (g->peer[s] < 0 || g->peer[s] >= nranks)
      return fail("partner %d maps to communicator rank %d outside [0,%d)", g->partner[s], g->peer[s], nranks);
  }
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  RCCL_TRY(rccl.CommInitRank(&g->comm, nranks, id, rank));
  // what the communicator itself says: a bench line reports THIS (config.rccl_nranks), not the world size it asked for
  int cnt = 0;
  RCCL_TRY(rccl.CommCount(g->comm, &cnt));
  g->comm_nranks = cnt;
  return 0;
}

// ranks in this context's RCCL communicator as ncclCommCount reports it; 0 without a communicator
int cfdp_gpu_rccl_nranks(const cfdp_gpu *g) { return g && g->comm ? g->comm_nranks : 0; }
int cfdp_gpu_rccl_allow_self_exchange(cfdp_gpu *g, int on) {
  if (!g) return fail("null context");
  g->rccl_self_exchange = on != 0;
  return 0;
}

int cfdp_gpu_rccl_finalize(cfdp_gpu *g) {
  if (!g) return fail("null context");
  if (g->comm) {
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipDeviceSynchronize());
    RCCL_TRY(rccl.CommDestroy(g->comm));
    g->comm = nullptr;
    g->comm_nranks = 0;
  }
  return 0;
}

// the RCCL group of the iteration opened by cfdp_gpu_step_pre (nothing if that step has no exchange)
int cfdp_gpu_exchange_rccl(cfdp_gpu *g) {
  NEED_UPLOAD(g);
  if (!g->pending_exchange) return 0;
  if (!g->comm) return fail("no communicator: call cfdp_gpu_rccl_init()");
  return enqueue_exchange(g);
}

int cfdp_gpu_step_rccl(cfdp_gpu *g, int with_exchange, int overlap, int with_flux, int flux_mode) {
  NEED_UPLOAD(g);
  if (with_exchange && !g->partner.empty() && !g->comm) return fail("no communicator: call cfdp_gpu_rccl_init()");
  return one_step(g, with_exchange, overlap, with_flux, flux_mode);
}

// `steps` iterations enqueued by one call.  (Capturing the step -- RCCL group included -- in a
// hipGraph was tried: with RCCL 2.26.6 / ROCm 7.0 hipStreamEndCapture crashes once ncclSend/
// ncclRecv have been captured, so the steps are stream launches: ~54 us of host time each.)
int cfdp_gpu_run_steps_rccl(cfdp_gpu *g, int steps, int with_exchange, int overlap, int with_flux,
                            int flux_mode) {
  NEED_UPLOAD(g);
  if (steps < 1) return fail("steps must be >= 1");
  if (with_exchange && !g->partner.empty() && !g->comm) return fail("no communicator: call cfdp_gpu_rccl_init()");
  for (int i = 0; i < steps; i++)
    if (one_step(g, with_exchange, overlap, with_flux, flux_mode)) return 1;
  return 0;
}

// --------------------------------------- one process per GPU: xGMI write + notify (HIP IPC)
// See gg_push_kernel.  Setup: every rank exports its block (cfdp_gpu_ipc_export), the host
// exchanges the 64-byte handles and tells each rank, per partner slot, where in the partner's
// block its rows land for either parity and where its arrival counter is (cfdp_gpu_ipc_connect);
// cfdp_gpu_ipc_ready uploads the tables and switches the context's ghost block to the landing
// arenas.  A step needs no communication library and no host involvement beyond kernel launches,
// so a run of steps is replayed from one hipGraph.
namespace {
double g_ipc_wait_seconds = 0.0;
}
// polls (~1 us each) before a device-side wait for a partner gives up: about 10 s by default
extern "C++" long cfdp_detail::ipc_max_polls() {
  if (g_ipc_wait_seconds <= 0.0) {
    const char *e = getenv("CFDP_IPC_WAIT_SECONDS");
    g_ipc_wait_seconds = e && atof(e) > 0 ? atof(e) : 10.0;
  }
  return (long)(g_ipc_wait_seconds * 1e6);
}

extern "C++" void cfdp_detail::ipc_release(cfdp_gpu *g) {
  auto &I = g->ipc;
  I.wait_pending = false;
  I.drop_graph_sets();
  for (void *p : I.opened) (void)hipIpcCloseMemHandle(p);
  I.opened.clear(); I.opened_handle.clear();
  for (int par = 0; par < 2; par++) { (void)hipFree(I.d_dst[par]); I.d_dst[par] = nullptr; I.dst[par].clear(); }
  (void)hipFree(I.d_rflag); I.d_rflag = nullptr; I.rflag.clear();
  (void)hipFree(I.d_slot_of_row); (void)hipFree(I.d_send_off);
  (void)hipFree(I.d_tile_off); (void)hipFree(I.d_ent); (void)hipFree(I.d_ent_row);
  (void)hipFree(I.d_pt_first); (void)hipFree(I.d_tile_xoff); (void)hipFree(I.d_rng);
  I.d_rng = nullptr; I.jitter_us = 0;
  I.d_pt_first = nullptr; I.d_tile_xoff = nullptr;
  I.d_slot_of_row = I.d_send_off = I.d_tile_off = I.d_ent = I.d_ent_row = nullptr;
  I.inkernel = false; I.put = false;
  (void)hipFree(I.d_done); (void)hipFree(I.d_need); (void)hipFree(I.d_tile_mask); (void)hipFree(I.d_tile_iter);
  I.d_done = I.d_need = I.d_tile_iter = nullptr; I.d_tile_mask = nullptr; I.per_partner = false; I.counters = false;
  (void)hipFree(I.flags); I.flags = nullptr;
  (void)hipFree(I.block); I.block = nullptr;
  I.on = false; I.xiter = 0;
}

// the tables a tile of the pass (or of the closing flux kernel) needs to push, notify and wait
extern "C++" void cfdp_detail::ipc_push_args(cfdp_gpu *g, int par, gg_push_args *out) {
  auto &I = g->ipc;
  gg_push_args pa;
  pa.tile_off = I.d_tile_off; pa.ent = I.d_ent; pa.ent_row = I.d_ent_row; pa.dst = I.d_dst[par];
  pa.hdr = g->ipc_hdr(); pa.rflag = I.d_rflag; pa.done = I.d_done;
  pa.need = I.per_partner ? I.d_need : nullptr; pa.tile_mask = I.per_partner ? I.d_tile_mask : nullptr;
  pa.pt_first = I.d_pt_first; pa.pt_stride = I.pt_stride; pa.tile_xoff = I.d_tile_xoff;
  pa.nbtiles = g->nbtiles; pa.nslots = (int)g->partner.size();
  pa.inv_after_flag = I.mode == 2 ? 1 : 0;
  pa.counters = I.counters ? 1 : 0;
  pa.tile_iter = I.d_tile_iter;
  pa.wait_polls = I.wait_pending && I.wait_inkernel && !I.fault_skip_wait ? (long)ipc_max_polls() : 0;
  *out = pa;
}

namespace {
// the rows of this exchange to the partners, then the notification, on `st`: the push kernel (stores over the IPC mappings),
// or -- the put rung -- pack kernel + one copy per partner slice; either way the notify kernel behind it in stream order
int ipc_send_rows(cfdp_gpu *g, const gg_grad_view &src, int par, hipStream_t st) {
  auto &I = g->ipc;
  const int nslots = (int)g->partner.size();
  if (I.put) {
    HIP_TRY(gg_launch_pack(g->d_sendidx, g->send_off.back(), src, g->d_sendbuf, st));
    for (int s = 0; s < nslots; s++) {
      const size_t n = (size_t)(g->send_off[s + 1] - g->send_off[s]) * 21 * sizeof(double);
      if (n) HIP_TRY(hipMemcpyAsync(I.dst[par][s], g->d_sendbuf + (size_t)g->send_off[s] * 21, n, hipMemcpyDeviceToDevice, st));
    }
  } else {
    HIP_TRY(gg_launch_push(g->d_sendidx, g->send_off.back(), I.d_slot_of_row, I.d_send_off, src, I.d_dst[par], st));
  }
  HIP_TRY(gg_launch_notify(g->ipc_hdr(), I.d_rflag, nslots, I.counters ? I.d_need : nullptr, I.d_tile_iter, g->nbtiles, st));
  return 0;
}

int ipc_pre(cfdp_gpu *g, int with_exchange, int overlap) {
  const bool comm = with_exchange && !g->partner.empty();
  if (g->ipc.jitter_us > 0 && g->ipc.d_rng) {
    g->main_marked = false;
    HIP_TRY(gg_launch_jitter(g->ipc.d_rng, g->ipc.jitter_us, g->s_main));
  }
  g->pending_exchange = false;
  g->iter++;
  const bool fused = g->will_fuse();
  if (!fused && flush_flux(g)) return 1;
  auto grad_tiles = [&](int which, hipStream_t st) { return fused ? launch_fused(g, which, st) : launch_grad(g, which, st); };
  // a pending wait for the previous exchange is absorbed by the boundary tiles of a pushing fused pass;
  // every other schedule reads ghost rows without that check and needs the wait kernel first
  if (!(comm && fused && g->ipc.inkernel && g->ipc.wait_inkernel) && ipc_settle(g)) return 1;
  if (!comm) {
    if (grad_tiles(CFDP_TILES_ALL, g->s_main)) return 1;
    if (fused) fused_done(g);
  } else {
    auto &I = g->ipc;
    const int par = (int)((I.xiter + 1) & 1);
    const gg_grad_view src = fused ? g->alt_view() : g->grad_view();  // the buffer this iteration's gradients go to
    int pushed = 0;
    if (fused && I.inkernel) {
      // ONE launch for all tiles: the boundary tiles (first in the grid) push their send rows to the
      // partners straight from their registers, the last of them raises the flags; the partners'
      // rows arrive while the interior tiles run.  (Both exchange schedules map to this one: a
      // fork/join between two streams costs 8-18 us per iteration inside a hipGraph.)
      gg_push_args pa;
      ipc_push_args(g, par, &pa);
      const int rc = launch_fused(g, CFDP_TILES_ALL, g->s_main, &pa);
      if (rc == 1) return 1;
      pushed = rc == 0;
      if (pushed) I.wait_pending = false;  // absorbed (or there was none)
      else if (ipc_settle(g)) return 1;    // no fused kernel fits these tiles: the separate kernels below
    }
    if (pushed) {
    } else if (overlap) {
      // boundary tiles -> push -> notify on the comm stream, the interior tiles on the main stream at
      // the same time (see cfdp_gpu_step_pre); the wait joins them
      if (fork_comm(g)) return 1;  // the comm stream forks off the main stream here
      if (grad_tiles(CFDP_TILES_BOUNDARY, g->s_comm)) return 1;
      if (ipc_send_rows(g, src, par, g->s_comm)) return 1;
      HIP_TRY(hipEventRecord(g->ev_senddone, g->s_comm));
      if (grad_tiles(CFDP_TILES_INTERIOR, g->s_main)) return 1;
      HIP_TRY(hipStreamWaitEvent(g->s_main, g->ev_senddone, 0));
    } else {
      if (grad_tiles(CFDP_TILES_ALL, g->s_main)) return 1;
      if (ipc_send_rows(g, src, par, g->s_main)) return 1;
    }
    if (fused) fused_done(g);
    I.xiter++;  // from here on the ghost block is the arena this exchange lands in
    g->main_marked = false;
    // the wait for this exchange: left to the boundary tiles of the next pushing pass (one launch per
    // iteration), or -- ipc_settle -- to a wait kernel in front of whatever else reads the ghost rows first
    I.wait_pending = true;
    if (!(pushed && I.wait_inkernel) && ipc_settle(g)) return 1;
  }
  return 0;
}

int ipc_post(cfdp_gpu *g, int with_flux, int flux_mode);

int one_step_ipc(cfdp_gpu *g, int with_exchange, int overlap, int with_flux, int flux_mode) {
  if (ipc_pre(g, with_exchange, overlap)) return 1;
  return ipc_post(g, with_flux, flux_mode);
}

int ipc_post(cfdp_gpu *g, int with_flux, int flux_mode) {
  if (with_flux) {
    if (flux_mode != CFDP_FLUX_CONSISTENT && flux_mode != CFDP_FLUX_REFERENCE) return fail("bad flux mode %d", flux_mode);
    if (g->fusion && g->d_grad_alt) g->flux_pending = flux_mode;
    else if (launch_flux(g, flux_mode, g->s_main)) return 1;
  }
  if (scaled_tail(g, scaled_lag(g, with_flux), true, g->s_main)) return 1;
  // no end-of-iteration marker here (each costs ~5 us on the device): a later step that needs to
  // fork its comm stream records one itself (fork_comm), and the single-stream schedules need none
  g->main_marked = false;
  return 0;
}
}  // namespace

// CFDP_IPC_MODE = coarse | split | fine (CFDP_IPC_FINEGRAINED=1 is the older spelling of fine)
static int ipc_mode_from_env() {
  if (const char *m = getenv("CFDP_IPC_MODE")) {
    if (!strcmp(m, "fine")) return 1;
    if (!strcmp(m, "split")) return 2;
    if (!strcmp(m, "coarse")) return 0;
  }
  const char *fg = getenv("CFDP_IPC_FINEGRAINED");
  return fg && atoi(fg) != 0 ? 1 : 0;
}

// a partner's block (or flag block), mapped once per handle
static int ipc_open(cfdp_gpu *g, const void *handle64, unsigned char **base_out) {
  auto &I = g->ipc;
  void *base = nullptr;
  for (size_t i = 0; i < I.opened.size(); i++)
    if (!memcmp(I.opened_handle[i].data(), handle64, 64)) base = I.opened[i];
  if (!base) {
    hipIpcMemHandle_t h;
    memcpy(&h, handle64, sizeof h);
    HIP_TRY(hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess));
    I.opened.push_back(base);
    I.opened_handle.emplace_back((const unsigned char *)handle64, (const unsigned char *)handle64 + 64);
  }
  *base_out = static_cast<unsigned char *>(base);
  return 0;
}

// how the next cfdp_gpu_ipc_export / _ready set the exchange up, per context and by argument instead of through the
// process environment (-1 = as the environment says, else the library default):
//   memory_mode    0 coarse, 1 fine, 2 split                        (CFDP_IPC_MODE)
//   wait_inkernel  1 the boundary tiles wait themselves, 0 wait kernel (CFDP_IPC_WAIT_INKERNEL; ranks sharing a device: 0)
//   notify         1 counters (fire-and-forget atomic adds), 0 flags   (CFDP_IPC_NOTIFY=counter|flag)
//   push_inkernel  1 the fused pass pushes and notifies itself, 0 push / notify / wait are kernels of their own -- the
//                  conservative rung: release / acquire at kernel boundaries instead of inside a kernel (CFDP_IPC_INKERNEL);
//                  2 the copy-engine put: pack kernel, one hipMemcpyAsync per partner slice into its landing slice, then
//                  the notify kernel (the reference's MPI_Put variants, src/exchange_data_mpidma.c:93-127)
int cfdp_gpu_ipc_configure(cfdp_gpu *g, int memory_mode, int wait_inkernel, int notify, int push_inkernel) {
  if (!g) return fail("null context");
  if (memory_mode < -1 || memory_mode > 2 || wait_inkernel < -1 || wait_inkernel > 1 || notify < -1 || notify > 1 ||
      push_inkernel < -1 || push_inkernel > 2)
    return fail("cfdp_gpu_ipc_configure(%d, %d, %d, %d): out of range", memory_mode, wait_inkernel, notify, push_inkernel);
  g->ipc.cfg_mode = memory_mode;
  g->ipc.cfg_wait_inkernel = wait_inkernel;
  g->ipc.cfg_notify = notify;
  g->ipc.cfg_inkernel = push_inkernel;
  return 0;
}

int cfdp_gpu_ipc_header_bytes(void) { return GG_IPC_HDR_BYTES; }
// where, in a rank's block (or flag block), the word of partner slot `slot` lives: a cache line of its own
size_t cfdp_gpu_ipc_flag_offset(int slot) { return (size_t)slot * GG_IPC_SLOT_STRIDE * sizeof(int); }

int cfdp_gpu_ipc_export(cfdp_gpu *g, void *handle64, size_t *land_bytes) {
  NEED_UPLOAD(g);
  if (!handle64) return fail("null argument");
  if ((int)g->partner.size() > GG_IPC_MAXSLOTS) return fail("more than %d partners", GG_IPC_MAXSLOTS);
  for (size_t s = 0; s < g->partner.size(); s++)  // the double-buffered arenas rely on traffic in both directions
    if (g->send_off[s + 1] == g->send_off[s] || g->recv_off[s + 1] == g->recv_off[s])
      return fail("partner %d is not a two-way partner", g->partner[s]);
  // the two landing arenas are safe without credit messages because only tiles that hold send
  // points read ghost rows, and those tiles are done before this rank's next push is announced
  if (g->interior_reads_ghosts)
    return fail("a tile without send points reads ghost rows (one-way halo): not supported by this exchange");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "HIP IPC handles are 64 bytes");
  ipc_release(g);
  auto &I = g->ipc;
  I.land_bytes = (((size_t)(g->nall - g->nown) * 21 * sizeof(double)) + 255) & ~(size_t)255;
  const size_t bytes = GG_IPC_HDR_BYTES + 2 * I.land_bytes;
  I.mode = I.cfg_mode >= 0 ? I.cfg_mode : ipc_mode_from_env();
  if (I.mode == 1) HIP_TRY(hipExtMallocWithFlags((void **)&I.block, bytes, hipDeviceMallocFinegrained));
  else HIP_TRY(hipMalloc(&I.block, bytes));
  HIP_TRY(cfdp_memset_sync(I.block, 0, bytes));
  if (I.mode == 2) {  // the flag words alone in fine-grained memory (the header of `block` stays unused)
    HIP_TRY(hipExtMallocWithFlags((void **)&I.flags, 64 * 1024, hipDeviceMallocFinegrained));
    HIP_TRY(cfdp_memset_sync(I.flags, 0, 64 * 1024));
  }
  hipIpcMemHandle_t h;
  HIP_TRY(hipIpcGetMemHandle(&h, I.block));
  memcpy(handle64, &h, sizeof h);
  memcpy(I.my_handle, &h, sizeof h);
  if (land_bytes) *land_bytes = I.land_bytes;
  const int nslots = (int)g->partner.size();
  I.dst[0].assign(nslots, nullptr); I.dst[1].assign(nslots, nullptr); I.rflag.assign(nslots, nullptr);
  return 0;
}

int cfdp_gpu_ipc_connect(cfdp_gpu *g, int slot, const void *partner_handle64, size_t land_off0,
                         size_t land_off1, size_t flag_off) {
  NEED_UPLOAD(g);
  auto &I = g->ipc;
  if (!I.block) return fail("cfdp_gpu_ipc_export() first");
  if (slot < 0 || slot >= (int)g->partner.size() || !partner_handle64) return fail("bad partner slot");
  unsigned char *b = nullptr;
  if (ipc_open(g, partner_handle64, &b)) return 1;
  I.dst[0][slot] = reinterpret_cast<double *>(b + land_off0);
  I.dst[1][slot] = reinterpret_cast<double *>(b + land_off1);
  I.rflag[slot] = reinterpret_cast<int *>(b + flag_off);
  return 0;
}

// the handle of the block that holds this rank's flag words: a block of its own in split mode, else the main block
int cfdp_gpu_ipc_export_flags(cfdp_gpu *g, void *handle64) {
  NEED_UPLOAD(g);
  auto &I = g->ipc;
  if (!I.block || !handle64) return fail("cfdp_gpu_ipc_export() first");
  if (I.flags) {
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, I.flags));
    memcpy(handle64, &h, sizeof h);
  } else {
    memcpy(handle64, I.my_handle, 64);
  }
  return 0;
}

// my arrival counter at partner `slot` lives at flag_off in the block of THAT handle (after cfdp_gpu_ipc_connect)
int cfdp_gpu_ipc_connect_flags(cfdp_gpu *g, int slot, const void *partner_flags_handle64, size_t flag_off) {
  NEED_UPLOAD(g);
  auto &I = g->ipc;
  if (!I.block) return fail("cfdp_gpu_ipc_export() first");
  if (slot < 0 || slot >= (int)g->partner.size() || !partner_flags_handle64) return fail("bad partner slot");
  unsigned char *b = nullptr;
  if (ipc_open(g, partner_flags_handle64, &b)) return 1;
  I.rflag[slot] = reinterpret_cast<int *>(b + flag_off);
  return 0;
}

// MEASUREMENT ONLY (tools/loopback_probe.py): partner slot `slot` is this rank ITSELF -- its rows land in its own arenas
// at the slot's receive offset, its flag is its own flag word.  The ghost rows then hold this rank's own send rows (wrong
// values, right traffic): what one iteration of the write + notify protocol costs when the partner is never late.
int cfdp_gpu_ipc_connect_loopback(cfdp_gpu *g, int slot) {
  NEED_UPLOAD(g);
  auto &I = g->ipc;
  if (!I.block) return fail("cfdp_gpu_ipc_export() first");
  if (slot < 0 || slot >= (int)g->partner.size()) return fail("bad partner slot");
  if (g->send_off[slot + 1] - g->send_off[slot] > g->recv_off[slot + 1] - g->recv_off[slot])
    return fail("loopback needs a receive slice at least as long as the send slice (slot %d)", slot);
  const size_t base = GG_IPC_HDR_BYTES + (size_t)g->recv_off[slot] * 21 * sizeof(double);
  I.dst[0][slot] = reinterpret_cast<double *>(I.block + base);
  I.dst[1][slot] = reinterpret_cast<double *>(I.block + base + I.land_bytes);
  I.rflag[slot] = g->ipc_hdr() + slot * GG_IPC_SLOT_STRIDE;
  return 0;
}

// what the exchange set up by cfdp_gpu_ipc_ready does: bit 0 the fused pass pushes and notifies itself, bit 1 its
// boundary tiles wait themselves, bit 2 per-partner notification and wait masks, bit 3 notification by counters
// (fire-and-forget atomic adds), bits 4-5 the memory mode (0 coarse, 1 fine, 2 split), bit 6 the copy-engine put rung
int cfdp_gpu_ipc_mode(const cfdp_gpu *g) {
  if (!g || !g->ipc.block) return -1;
  const auto &I = g->ipc;
  return (I.inkernel ? 1 : 0) | (I.inkernel && I.wait_inkernel ? 2 : 0) | (I.per_partner ? 4 : 0) | (I.counters ? 8 : 0) | (I.mode << 4) |
         (I.put ? 64 : 0);
}

int cfdp_gpu_ipc_ready(cfdp_gpu *g) {
  NEED_UPLOAD(g);
  auto &I = g->ipc;
  if (!I.block) return fail("cfdp_gpu_ipc_export() first");
  const int nslots = (int)g->partner.size();
  for (int s = 0; s < nslots; s++)
    if (!I.dst[0][s] || !I.dst[1][s] || !I.rflag[s]) return fail("partner slot %d is not connected", s);
  const size_t nsend = (size_t)g->send_off.back();
  std::vector<int> slot_of_row(nsend ? nsend : 1, 0);
  for (int s = 0; s < nslots; s++)
    for (int j = g->send_off[s]; j < g->send_off[s + 1]; j++) slot_of_row[j] = s;
  for (int par = 0; par < 2; par++) {
    HIP_TRY(hipMalloc(&I.d_dst[par], sizeof(double *) * (size_t)(nslots ? nslots : 1)));
    if (nslots) HIP_TRY(hipMemcpy(I.d_dst[par], I.dst[par].data(), sizeof(double *) * (size_t)nslots, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMalloc(&I.d_rflag, sizeof(int *) * (size_t)(nslots ? nslots : 1)));
  if (nslots) HIP_TRY(hipMemcpy(I.d_rflag, I.rflag.data(), sizeof(int *) * (size_t)nslots, hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&I.d_slot_of_row, sizeof(int) * slot_of_row.size()));
  HIP_TRY(hipMemcpy(I.d_slot_of_row, slot_of_row.data(), sizeof(int) * slot_of_row.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&I.d_send_off, sizeof(int) * g->send_off.size()));
  HIP_TRY(hipMemcpy(I.d_send_off, g->send_off.data(), sizeof(int) * g->send_off.size(), hipMemcpyHostToDevice));
  // what this rank's word at partner s advances by per exchange: the boundary tiles that count towards s when it
  // notifies by counters, 1 when it stores its exchange number (flags, every rung).  The partner's waits multiply by it
  // whatever THEIR form is: the per-partner protocol depends on a rank's own partition, so neighbours may resolve to
  // different forms and must still understand each other
  std::vector<int> advance((size_t)(nslots ? nslots : 1), 1);
  {  // the send rows of every boundary tile: (tile-local point | slot << 16, row in the partner's slice)
    std::vector<int> tile_off((size_t)g->ntiles + 1, 0), ent(nsend ? nsend : 1, 0), ent_row(nsend ? nsend : 1, 0), tile_of(nsend ? nsend : 1, 0);
    bool ok = nslots <= 0x7FFF;
    for (size_t j = 0; j < nsend && ok; j++) {
      const int p = g->send_idx_host[j];
      int lo = 0, hi = g->nbtiles - 1, t = -1;  // boundary tiles hold the send points, sorted by pstart
      while (lo <= hi) {
        const int mid = (lo + hi) / 2;
        if (p < g->h_tiles[mid].pstart) hi = mid - 1;
        else if (p >= g->h_tiles[mid].pstart + g->h_tiles[mid].npts) lo = mid + 1;
        else { t = mid; break; }
      }
      if (t < 0 || p - g->h_tiles[t].pstart > 0xFFFF) { ok = false; break; }
      tile_of[j] = t;
      tile_off[t + 1]++;
    }
    I.inkernel = false;
    if (ok && nsend) {
      for (int t = 0; t < g->ntiles; t++) tile_off[t + 1] += tile_off[t];
      // a point's FIRST destination (message order) goes into the point-major table and to the front of its tile's
      // entries; further destinations (points on an edge or corner between partners) behind them, from tile_xoff on
      // (stride = the lanes-per-point groups of the LARGEST workgroup a launch over all tiles can have: every thread of
      // a boundary tile's workgroup reads its group's entry, also the groups beyond the tile's points)
      int tpmax = 1;
      for (int t = 0; t < g->ntiles; t++) tpmax = g->h_tiles[t].npts > tpmax ? g->h_tiles[t].npts : tpmax;
      for (const auto &G : g->groups) tpmax = G.tp > tpmax ? G.tp : tpmax;  // (lane groups: points + the helper groups of long lists)
      I.pt_stride = (tpmax + 63) & ~63;
      std::vector<int2> pt_first((size_t)(g->nbtiles ? g->nbtiles : 1) * I.pt_stride, make_int2(-1, 0));
      std::vector<int> tile_xoff((size_t)g->ntiles + 1, 0), nfirst((size_t)g->ntiles, 0);
      std::vector<char> is_first(nsend, 0);
      for (size_t j = 0; j < nsend; j++) {
        const int t = tile_of[j], li = g->send_idx_host[j] - g->h_tiles[t].pstart;
        int2 &f = pt_first[(size_t)t * I.pt_stride + li];
        if (f.x < 0) { f = make_int2(slot_of_row[j], (int)j - g->send_off[slot_of_row[j]]); is_first[j] = 1; nfirst[t]++; }
      }
      std::vector<int> fill(tile_off.begin(), tile_off.end() - 1), fillx((size_t)g->ntiles, 0);
      for (int t = 0; t < g->ntiles; t++) { tile_xoff[t] = tile_off[t] + nfirst[t]; fillx[t] = tile_xoff[t]; }
      tile_xoff[g->ntiles] = tile_off[g->ntiles];
      for (size_t j = 0; j < nsend; j++) {
        const int t = tile_of[j], s = slot_of_row[j], at = is_first[j] ? fill[t]++ : fillx[t]++;
        ent[at] = (g->send_idx_host[j] - g->h_tiles[t].pstart) | (s << 16);
        ent_row[at] = (int)j - g->send_off[s];
      }
      HIP_TRY(hipMalloc(&I.d_pt_first, sizeof(int2) * pt_first.size()));
      HIP_TRY(hipMemcpy(I.d_pt_first, pt_first.data(), sizeof(int2) * pt_first.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMalloc(&I.d_tile_xoff, sizeof(int) * tile_xoff.size()));
      HIP_TRY(hipMemcpy(I.d_tile_xoff, tile_xoff.data(), sizeof(int) * tile_xoff.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMalloc(&I.d_tile_off, sizeof(int) * tile_off.size()));
      HIP_TRY(hipMemcpy(I.d_tile_off, tile_off.data(), sizeof(int) * tile_off.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMalloc(&I.d_ent, sizeof(int) * ent.size()));
      HIP_TRY(hipMemcpy(I.d_ent, ent.data(), sizeof(int) * ent.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMalloc(&I.d_ent_row, sizeof(int) * ent_row.size()));
      HIP_TRY(hipMemcpy(I.d_ent_row, ent_row.data(), sizeof(int) * ent_row.size(), hipMemcpyHostToDevice));
      const char *e = getenv("CFDP_IPC_INKERNEL");
      // the tiles push what they have just computed; a send point WITHOUT faces is computed by nobody
      // and its stored row must travel (as pack / the push kernel send it, and the reference's
      // exchange_dbl_copy_in, src/threads.c:791-813): such partitions keep the separate push kernel
      const int how = I.cfg_inkernel >= 0 ? I.cfg_inkernel : (e ? atoi(e) : 1);  // 1 in the fused pass, 0 kernels of their own, 2 put
      I.inkernel = g->nbtiles > 0 && !g->faceless_send && how == 1;
      I.put = how == 2;
      const char *w = getenv("CFDP_IPC_WAIT_INKERNEL");  // 0: always a separate wait kernel (A/B timing)
      I.wait_inkernel = I.cfg_wait_inkernel >= 0 ? I.cfg_wait_inkernel != 0 : !(w && atoi(w) == 0);
      // per-partner notification needs: every boundary tile reads ghost rows only of partners it sends to (then the
      // flags a tile waits for also cover the rows it is about to overwrite at those partners, see gg_kernels.hip)
      std::vector<unsigned long long> smask((size_t)g->nbtiles, 0ull);
      std::vector<int> need((size_t)(nslots ? nslots : 1), 0);
      for (int t = 0; t < g->nbtiles; t++)
        for (int e2 = tile_off[t]; e2 < tile_off[t + 1]; e2++) smask[(size_t)t] |= 1ull << (ent[e2] >> 16);
      bool pp = nslots <= GG_IPC_MAXSLOTS && (int)g->tile_recv_mask.size() == g->nbtiles;
      for (int t = 0; t < g->nbtiles && pp; t++) pp = (g->tile_recv_mask[(size_t)t] & ~smask[(size_t)t]) == 0;
      for (int t = 0; t < g->nbtiles; t++)
        for (int s2 = 0; s2 < nslots; s2++)
          if ((smask[(size_t)t] >> s2) & 1ull) need[(size_t)s2]++;
      for (int s2 = 0; s2 < nslots; s2++) pp = pp && need[(size_t)s2] > 0;
      const char *ppe = getenv("CFDP_IPC_PER_PARTNER");  // 0: one counter, all flags raised by the last boundary tile (A/B)
      I.per_partner = pp && !(ppe && atoi(ppe) == 0);
      // notification: counters raised by fire-and-forget atomic adds (default wherever the per-partner protocol holds),
      // or flags raised by the tile that completes a partner's rows (CFDP_IPC_NOTIFY=flag; cfdp_gpu_ipc_configure)
      const char *ne = getenv("CFDP_IPC_NOTIFY");
      const int want_counters = I.cfg_notify >= 0 ? I.cfg_notify : !(ne && !strcmp(ne, "flag"));
      I.counters = I.per_partner && want_counters;
      HIP_TRY(hipMalloc(&I.d_need, sizeof(int) * need.size()));
      HIP_TRY(hipMemcpy(I.d_need, need.data(), sizeof(int) * need.size(), hipMemcpyHostToDevice));
      if (I.counters) advance = need;
      HIP_TRY(hipMalloc(&I.d_tile_mask, sizeof(unsigned long long) * (smask.size() + 1)));
      if (!smask.empty())
        HIP_TRY(hipMemcpy(I.d_tile_mask, smask.data(), sizeof(unsigned long long) * smask.size(), hipMemcpyHostToDevice));
      if (const char *j = cfdp_experiment_getenv("CFDP_IPC_JITTER_US")) {
        I.jitter_us = atoi(j) > 0 ? atoi(j) : 0;
        if (I.jitter_us) {
          const unsigned seed = 2463534242u ^ (unsigned)(uintptr_t)g ^ (unsigned)getpid() * 2654435761u;
          HIP_TRY(hipMalloc(&I.d_rng, sizeof(unsigned)));
          HIP_TRY(hipMemcpy(I.d_rng, &seed, sizeof seed, hipMemcpyHostToDevice));
          fprintf(stderr, "[cfdp] TEST MODE: up to %d us of random idle time in front of every step (CFDP_IPC_JITTER_US)\n", I.jitter_us);
        }
      }
      const char *f = cfdp_experiment_getenv("CFDP_IPC_FAULT");
      I.fault_skip_wait = f && !strcmp(f, "skip_wait");
      if (I.fault_skip_wait) fprintf(stderr, "[cfdp] FAULT INJECTION: boundary tiles do not wait for the previous exchange (CFDP_IPC_FAULT)\n");
    }
  }
  if (nslots > 0 && nslots <= 64) {
    // every partner learns it: word NEED_IN of this rank's slot line in ITS header, next to the arrival word itself.  Written
    // once, here, from THIS device with system-scope stores like every push; read by the partner's waits from its first
    // exchanging step on -- the hosts meet between _ready and that step (every set-up in this repo validates collectively
    // first; cfdproxy_hip.h says so for other hosts)
    int *d_advance = nullptr;
    HIP_TRY(hipMalloc(&d_advance, sizeof(int) * advance.size()));
    HIP_TRY(hipMemcpy(d_advance, advance.data(), sizeof(int) * advance.size(), hipMemcpyHostToDevice));
    HIP_TRY(gg_launch_poke(I.d_rflag, d_advance, GG_IPC_NEED_IN, nslots, g->s_main));
    HIP_TRY(hipStreamSynchronize(g->s_main));
    (void)hipFree(d_advance);
  } else if (nslots > 64) {
    return fail("%d partners: the write + notify exchange is built for at most 64", nslots);
  }
  HIP_TRY(hipMalloc(&I.d_done, sizeof(int) * (GG_IPC_MAXSLOTS + 1) * GG_DONE_STRIDE));
  HIP_TRY(cfdp_memset_sync(I.d_done, 0, sizeof(int) * (GG_IPC_MAXSLOTS + 1) * GG_DONE_STRIDE));
  HIP_TRY(hipMalloc(&I.d_tile_iter, sizeof(int) * (size_t)(g->nbtiles > 0 ? g->nbtiles : 1)));
  HIP_TRY(cfdp_memset_sync(I.d_tile_iter, 0, sizeof(int) * (size_t)(g->nbtiles > 0 ? g->nbtiles : 1)));
  if (flush_flux(g)) return 1;
  HIP_TRY(hipDeviceSynchronize());
  // the ghost rows move into the landing arenas
  if (g->nall > g->nown)
    for (int par = 0; par < 2; par++)
      HIP_TRY(cfdp_copy_d2d_sync(g->land(par), g->d_grad + (size_t)g->nown * 6, sizeof(double) * 21 * (size_t)(g->nall - g->nown)));
  I.xiter = 0;
  I.on = true;
  g->drop_graphs();
  return 0;
}

// switch between the landing arenas and the ghost block of grad (e.g. to time another transport
// on the same context); the mappings stay
int cfdp_gpu_ipc_enable(cfdp_gpu *g, int on) {
  NEED_UPLOAD(g);
  auto &I = g->ipc;
  if (on && (!I.block || !I.d_rflag)) return fail("cfdp_gpu_ipc_ready() has not been called");
  if (flush_flux(g)) return 1;
  HIP_TRY(hipDeviceSynchronize());
  I.on = on != 0;
  g->drop_graphs();
  return 0;
}

// how long a device-side wait polls before it gives up (process-wide; also CFDP_IPC_WAIT_SECONDS).
// Graphs captured earlier keep the bound they were captured with.
int cfdp_ipc_set_wait_seconds(double seconds) {
  if (!(seconds > 0.0)) return fail("the wait bound must be positive");
  g_ipc_wait_seconds = seconds;
  return 0;
}

int cfdp_gpu_ipc_disconnect(cfdp_gpu *g) {
  if (!g) return fail("null context");
  HIP_TRY(hipSetDevice(g->device));
  HIP_TRY(hipDeviceSynchronize());
  ipc_release(g);
  return 0;
}

// 1 if a wait for a partner's rows gave up (the partner is gone or far behind), else 0; -1 on error
int cfdp_gpu_ipc_error(cfdp_gpu *g) {
  if (!g || !g->ipc.block) return 0;
  if (hipSetDevice(g->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
  int h[8], slot0 = 0;  // [ITER, ERR .. ERR + 4]
  if (hipMemcpy(h, g->ipc_hdr() + GG_IPC_ITER, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemcpy(&slot0, g->ipc_hdr(), sizeof slot0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const int *e = h + (GG_IPC_ERR - GG_IPC_ITER);
  if (getenv("CFDP_DEBUG_TRACE"))
    fprintf(stderr, "[cfdp] ipc state: host xiter %ld, device iteration counter %d (flag notification), arrival word of slot 0: "
                    "%d; %d waits gave up (last: slot %d, waiting for %d, saw %d)\n",
            g->ipc.xiter, h[0], slot0, e[4], e[1], e[2], e[3]);
  return e[0] != 0;
}

// for hosts that call the two face loops separately: the part of an iteration before the flux
// (gradients, push, notify, wait) and the flux part
int cfdp_gpu_step_ipc_post(cfdp_gpu *g, int with_flux, int flux_mode) {
  NEED_UPLOAD(g);
  if (!g->ipc.on) return fail("cfdp_gpu_ipc_ready() has not been called");
  return ipc_post(g, with_flux, flux_mode);
}

int cfdp_gpu_step_ipc_pre(cfdp_gpu *g, int with_exchange, int overlap) {
  NEED_UPLOAD(g);
  if (!g->ipc.on) return fail("cfdp_gpu_ipc_ready() has not been called");
  return ipc_pre(g, with_exchange, overlap);
}

int cfdp_gpu_step_ipc(cfdp_gpu *g, int with_exchange, int overlap, int with_flux, int flux_mode) {
  NEED_UPLOAD(g);
  if (!g->ipc.on) return fail("cfdp_gpu_ipc_ready() has not been called");
  return one_step_ipc(g, with_exchange, overlap, with_flux, flux_mode);
}

// `steps` iterations.  use_graph: after two lead-in steps (the first iteration of a run has no flux to
// fuse with), the steps are replayed from hipGraphs -- both streams, the push / notify / wait kernels
// included: whole chunks of 50 from one graph, the even part of the remainder from a second one (an
// even count restores the parity of the landing arenas and of the two grad buffers, which the kernels'
// arguments bake in), at most one step launched from the streams -- so short runs replay as well.
// use_graph = 2: a batch of 4..64 fused steps is ONE graph from its first pass to the flux of its last iteration and the
// wait for its last exchange ("closed": the state the caller's cfdp_gpu_sync would establish anyway, without the two
// stream launches behind the graph that a short batch pays on few steps); longer batches as with use_graph = 1.
int cfdp_gpu_run_steps_ipc(cfdp_gpu *g, int steps, int with_exchange, int overlap, int with_flux,
                           int flux_mode, int use_graph) {
  NEED_UPLOAD(g);
  if (!g->ipc.on) return fail("cfdp_gpu_ipc_ready() has not been called");
  if (steps < 1) return fail("steps must be >= 1");
  auto &I = g->ipc;
  const int full = 50;  // steps per replay of the main graph (2 kernels each with the in-kernel push)
  int done = 0;
  if (use_graph && steps >= 4) {
    // The first iteration of a run has no flux to fuse with: it would take the un-fused schedule (with exchange: gradient
    // kernel on two streams, push, notify and wait kernels: 57-120 us per step in loopback where the pushing fused pass
    // takes 41) from the streams.  In a batch of steps that all compute the flux, pretend the previous flux is pending
    // again instead: the first pass recomputes it from the gradients and ghost rows it was computed from (the same values;
    // psd_flux is rewritten by every step of the batch anyway) and the run is in its steady state -- and in its
    // hipGraphs -- from step one, with and without exchange alike (a benchmark compares the two).
    if (with_flux && g->fusion && g->d_grad_alt && g->flux_pending < 0 && !g->sc.on &&
        (!with_exchange || g->partner.empty() || I.inkernel))
      g->flux_pending = flux_mode;
    // lead-in steps from the streams until the state every captured chunk starts and ends in is reached: a flux pending
    // (fused schedule), the arena parity even
    for (const int lead = g->flux_pending >= 0 ? 0 : 2; done < lead; done++) {
      if (one_step_ipc(g, with_exchange, overlap, with_flux, flux_mode)) return 1;
      I.steps_streamed++;
    }
    // closed: the whole batch is one graph, its last flux and the wait for its last exchange included (its graph set is
    // keyed by the arena parity and the grad buffer it starts from: no parity step, any count)
    const bool closed = use_graph == 2 && done == 0 && steps <= 64 && g->flux_pending >= 0 && g->fusion && g->d_grad_alt && with_flux;
    if (!closed && (I.xiter & 1)) {  // a graph is tied to the arena parity it was captured at: even
      if (one_step_ipc(g, with_exchange, overlap, with_flux, flux_mode)) return 1;
      I.steps_streamed++;
      done++;
    }
    // The state a captured chunk starts AND ends in depends on who waits for an exchange.  A schedule whose fused pass
    // absorbs the wait (in-kernel push + in-kernel wait) ends every step with the wait for its exchange PENDING: its chunks
    // are captured with the wait pending at the start as well (the first pass waits in the kernel; a wait for flags that
    // have arrived long ago returns at once), so a chunk is right whatever the state at replay.  Every other schedule --
    // the wait kernel (ranks sharing a device, CFDP_IPC_WAIT_INKERNEL=0), push / notify kernels of their own, un-fused
    // steps, steps without exchange -- settles the wait at the end of every step: its chunks start settled (a pending wait
    // is settled HERE, in front of the capture) and end settled.  (Round 4 forced "pending" for all of them: their captures
    // could never close in the state they started in, were abandoned, and every step ran from the streams -- unreported.)
    const bool comm = with_exchange && !g->partner.empty();
    bool absorbs = comm && with_flux && g->fusion && g->d_grad_alt && I.inkernel && I.wait_inkernel;
    auto chunk_start_state = [&]() -> int {
      if (absorbs) { I.wait_pending = true; return 0; }
      return ipc_settle(g);
    };
    if (chunk_start_state()) return 1;
    // the graph set of this configuration (the arena the ghost rows are read from and the current grad buffer are baked
    // into the kernels' arguments too), or the least recently used one to capture into
    cfdp_gpu::ipc_state::graph_set *S = nullptr;
    for (auto &x : I.gs)
      if (x.exch == with_exchange && x.overlap == overlap && x.flux == with_flux && x.mode == flux_mode && x.cur == g->d_grad &&
          x.xpar == (int)(I.xiter & 1) && x.scaled == (int)g->sc.on && x.closed == (int)closed)
        S = &x;
    if (!S) {
      S = &I.gs[0];
      for (auto &x : I.gs)
        if (x.used < S->used) S = &x;
      if (S->graph || S->graph_rem) HIP_TRY(hipStreamSynchronize(g->s_main));  // (it may still be replaying)
      if (S->graph) (void)hipGraphExecDestroy(S->graph);
      if (S->graph_rem) (void)hipGraphExecDestroy(S->graph_rem);
      if (S->tmpl) (void)hipGraphDestroy(S->tmpl);
      if (S->tmpl_rem) (void)hipGraphDestroy(S->tmpl_rem);
      *S = cfdp_gpu::ipc_state::graph_set();
      S->exch = with_exchange; S->overlap = overlap; S->flux = with_flux; S->mode = flux_mode; S->cur = g->d_grad;
      S->xpar = (int)(I.xiter & 1); S->scaled = (int)g->sc.on; S->closed = (int)closed;
    }
    S->used = ++I.gs_clock;
    auto capture_once = [&](hipGraphExec_t &slot, int &slot_n, int n) -> bool {  // false: run from the streams instead
      hipGraph_t &tmpl = &slot == &S->graph ? S->tmpl : S->tmpl_rem;
      if (slot && slot_n == n) return true;
      if (slot) {  // another length wanted: the old one may still be replaying
        (void)hipStreamSynchronize(g->s_main);
        (void)hipGraphExecDestroy(slot);
        slot = nullptr;
      }
      if (tmpl) { (void)hipGraphDestroy(tmpl); tmpl = nullptr; }
      slot_n = 0;
      const double *cur0 = g->d_grad;
      const int pend0 = g->flux_pending;
      const long iter0 = g->iter, x0 = I.xiter;
      const unsigned passes0 = g->fused_passes;
      const bool wait0 = I.wait_pending;  // a chunk starts and ends with the wait of its last exchange pending
      hipGraph_t gr = nullptr;
      if (hipStreamBeginCapture(g->s_main, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return false; }
      g->main_marked = false;  // the first captured step must fork off a record made INSIDE the capture
      int rc = 0;
      for (int i = 0; i < n && !rc; i++) rc = one_step_ipc(g, with_exchange, overlap, with_flux, flux_mode);
      if (closed && !rc) rc = flush_flux(g, false);  // the wait kernel if a wait is pending, the last iteration's flux
      hipError_t ec = hipStreamEndCapture(g->s_main, &gr);
      (void)hipEventRecord(g->ev_fork, g->s_main);      // events last recorded inside a capture may not
      (void)hipEventRecord(g->ev_senddone, g->s_comm);  // be waited for outside it: re-arm them
      (void)mark_main(g);
      // an open chunk ends in the state it started in; a closed batch ends settled, its flux computed, and may leave the
      // two grad buffers swapped (an odd number of passes)
      const bool flipped = g->d_grad != cur0;
      const bool ok = !rc && ec == hipSuccess && gr &&
                      (closed ? g->flux_pending < 0 && !I.wait_pending
                              : !flipped && g->flux_pending == pend0 && I.wait_pending == wait0);
      if (closed && ok) {  // nothing of the capture has run: back to the start state (replay() establishes the end state)
        if (flipped) { std::swap(g->d_grad, g->d_grad_alt); std::swap(g->own_grad, g->own_grad_alt); }
        g->flux_pending = pend0;
        S->closed_flips = flipped;
      }
      if (ok && hipGraphInstantiate(&slot, gr, nullptr, nullptr, 0) != hipSuccess) slot = nullptr;
      if (ok && slot) tmpl = gr;  // kept: cfdp_gpu_refresh_graphs instantiates from it again
      else if (gr) (void)hipGraphDestroy(gr);
      g->iter = iter0;
      I.xiter = x0;  // nothing of the capture has run
      g->fused_passes = passes0;
      I.wait_pending = wait0;
      if (!ok || !slot) {
        if (g->d_grad != cur0) { std::swap(g->d_grad, g->d_grad_alt); std::swap(g->own_grad, g->own_grad_alt); }
        g->flux_pending = pend0;
        (void)hipGetLastError();
        I.captures_failed++;
        return false;
      }
      slot_n = n;
      return true;
    };
    auto capture = [&](hipGraphExec_t &slot, int &slot_n, int n) -> bool {
      if (capture_once(slot, slot_n, n)) return true;
      // the pass did not absorb the wait after all (no fused kernel fits these tiles: the separate kernels ran and
      // settled it): the chunk is one that starts and ends settled
      if (!absorbs) return false;
      absorbs = false;
      if (chunk_start_state()) return false;
      return capture_once(slot, slot_n, n);
    };
    auto replay = [&](hipGraphExec_t ge, int n) -> int {
      HIP_TRY(hipGraphLaunch(ge, g->s_main));
      // (a replay does not touch the event OBJECTS recorded inside the capture: whatever is ordered
      // after "the previous iteration" later needs a fresh record -- fork_comm makes one)
      g->main_marked = false;
      g->iter += n;
      if (with_exchange && !g->partner.empty()) I.xiter += n;
      done += n;
      I.steps_replayed += n;
      if (closed) {
        if (S->closed_flips) { std::swap(g->d_grad, g->d_grad_alt); std::swap(g->own_grad, g->own_grad_alt); }
        g->flux_pending = -1;
        I.wait_pending = false;
      }
      return 0;
    };
    if (closed) {
      if (capture(S->graph_rem, S->graph_rem_n, steps)) return replay(S->graph_rem, steps);
      // (not capturable: every step from the streams, below)
    } else {
      if (steps - done >= full && capture(S->graph, S->graph_n, full))
        while (steps - done >= full)
          if (replay(S->graph, full)) return 1;
      const int rem = (steps - done) & ~1;
      if (rem >= 2 && rem < full && capture(S->graph_rem, S->graph_rem_n, rem) && replay(S->graph_rem, rem)) return 1;
    }
  }
  for (; done < steps; done++) {
    if (one_step_ipc(g, with_exchange, overlap, with_flux, flux_mode)) return 1;
    I.steps_streamed++;
  }
  return 0;
}

// diagnostics: cfdp_gpu_debug_phase_stamps for steps of the write + notify schedule (launched from the streams, with or
// without the exchange riding in the pass): the stamps of the LAST of `passes` steps
int cfdp_gpu_debug_phase_stamps_ipc(cfdp_gpu *g, int passes, int with_exchange, unsigned long long *stamps) {
  NEED_UPLOAD(g);
  if (!g->ipc.on) return fail("cfdp_gpu_ipc_ready() has not been called");
  if (!g->fusion || !g->d_grad_alt || passes < 1 || !stamps) return fail("fusion must be on");
  if (const char *why = gg_diag_available()) return fail("%s", why);
  for (int i = 0; i < 2; i++)  // (the first step of a run has no flux to fuse with)
    if (one_step_ipc(g, with_exchange, 1, 1, CFDP_FLUX_CONSISTENT)) return 1;
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long *d = nullptr;
  const size_t n = (size_t)g->ntiles * 24;
  HIP_TRY(hipMalloc(&d, n * sizeof(unsigned long long)));
  HIP_TRY(cfdp_memset_sync(d, 0, n * sizeof(unsigned long long)));
  HIP_TRY(gg_set_stamp_buffer(d));
  const int saved = gg_debug_flags;
  gg_debug_flags |= 0x20000;
  int rc = 0;
  for (int i = 0; i < passes && !rc; i++) rc = one_step_ipc(g, with_exchange, 1, 1, CFDP_FLUX_CONSISTENT);
  gg_debug_flags = saved;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(gg_set_stamp_buffer(nullptr));
  if (!rc) HIP_TRY(hipMemcpy(stamps, d, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return rc ? 1 : 0;
}

// how the steps of cfdp_gpu_run_steps_ipc have run on this context so far: replayed from hipGraphs, launched from the
// streams (lead-in steps, odd remainders, runs of fewer than 4 steps, use_graph = 0 -- or every step when a capture
// failed), and how many captures were abandoned (0 in every schedule the library selects by itself)
int cfdp_gpu_ipc_graph_stats(cfdp_gpu *g, long *steps_replayed, long *steps_streamed, long *captures_failed) {
  if (!g) return fail("null context");
  if (steps_replayed) *steps_replayed = g->ipc.steps_replayed;
  if (steps_streamed) *steps_streamed = g->ipc.steps_streamed;
  if (captures_failed) *captures_failed = g->ipc.captures_failed;
  return 0;
}

}  // extern "C"
