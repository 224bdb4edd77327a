// gpu_adjoint.hip -- the adjoint of the Green-Gauss gradient behind the C ABI of include/cfdproxy_hip.h: its buffers, its
// halo path (the forward exchange of 21-double gbar rows over the existing send / receive lists) and its launches.
//
// Why the forward exchange is enough: every face touching an owned point is in that point's partition
// -- what makes the forward gradient exact under partitioning -- and the other ends of those faces are exactly the ghost
// points the exchange fills.  The adjoint at an owned point q needs s = gbar / V of q and of those other ends only, so the
// owners' s rows, delivered as ghost rows, give the global adjoint on every owned point; no accumulating (reverse) exchange
// exists here.  The tile scales the raw rows itself (1/V per row from a table in device numbering; a ghost row's 1/V is its
// OWNER's, sent once through the same path), so the exchange moves the raw gbar rows and no scale kernel runs.
#include "gpu_ctx.h"
#include "gg_adjoint.h"

namespace {

int adjoint_alloc(cfdp_gpu *g) {
  auto &A = g->adj;
  if (A.d_gbar) return 0;
  const size_t nall = (size_t)g->nall, nown = (size_t)g->nown, nsend = (size_t)g->send_off.back();
  auto alloc = [&]() -> int {
    HIP_TRY(hipMalloc(&A.d_ivol, sizeof(double) * (nall ? nall : 1)));
    HIP_TRY(hipMalloc(&A.d_vbar, sizeof(double) * 7 * (nown ? nown : 1)));
    HIP_TRY(hipMalloc(&A.d_send, sizeof(double) * 21 * (nsend + 1)));
    HIP_TRY(hipEventCreateWithFlags(&A.ev_sent, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&A.ev_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(A.ev_done, g->s_main));
    {  // own rows 1/V; ghost rows 0 until the owners' volumes have arrived (a ghost row with 1/V = 0 stages as s = 0)
      std::vector<double> iv(nall ? nall : 1, 0.0);
      for (size_t i = 0; i < nown; i++) iv[i] = 1.0 / g->vol[i];
      HIP_TRY(hipMemcpy(A.d_ivol, iv.data(), sizeof(double) * nall, hipMemcpyHostToDevice));
    }
    HIP_TRY(cfdp_memset_sync(A.d_vbar, 0, sizeof(double) * 7 * (nown ? nown : 1)));
    double *gb = nullptr;
    HIP_TRY(hipMalloc(&gb, sizeof(double) * 21 * (nall ? nall : 1)));
    A.d_gbar = gb;  // last: a context holding d_gbar holds every adjoint buffer
    HIP_TRY(cfdp_memset_sync(A.d_gbar, 0, sizeof(double) * 21 * (nall ? nall : 1)));
    A.ghost_ivol = nall == nown;
    return 0;
  };
  if (alloc()) {
    adjoint_release(g);  // (the message of the failed step stays the calling thread's last error)
    return 1;
  }
  return 0;
}

// every tile of the partition, one launch per launch group (the gradient's groups: two capacity classes, a GENERIC group of
// hub tiles in a launch of its own)
int launch_adjoint(cfdp_gpu *g, int ghosts, hipStream_t st) {
  auto &A = g->adj;
  gg_adj_args a;
  a.tiles = g->d_tiles; a.blob = g->d_blob; a.halo_idx = g->d_halo;
  a.gbar = A.d_gbar; a.ivol = A.d_ivol; a.vbar = A.d_vbar; a.nown = g->nown; a.ghosts = ghosts;
  g->main_marked = false;
  for (const tile_range &r : segs_of(g, CFDP_TILES_ALL)) {
    const hipError_t e = gg_launch_adjoint(a, g->grad_lanes, r.begin, r.n, r.tp, r.max_rows, r.max_blob, g->streaming, st);
    if (e == hipErrorInvalidConfiguration)
      return fail("adjoint: tiles of %d lane groups x %d lanes with %d staged rows and %d blob pieces fit no launch "
                  "(%zu bytes of LDS for one equation per row): use a smaller tile_points", r.tp, g->grad_lanes, r.max_rows,
                  r.max_blob, gg_adjoint_lds_bytes(r.max_rows, r.max_blob, 1));
    if (e != hipSuccess) return fail("adjoint launch failed: %s", hipGetErrorString(e));
  }
  return 0;
}

int refuse_ipc(const cfdp_gpu *g) {
  if (g->ipc.on)
    return fail("the xGMI write + notify transport is on for this context: the adjoint exchange has no form over it (no "
                "silent fall-back to another transport) -- cfdp_gpu_ipc_enable(g, 0) first");
  return 0;
}

// one forward exchange among in-process ranks of a per-point field of `rowlen` doubles: rank a's send rows (gathered
// from field(a)) are copied into the ghost rows of field(b) of every partner b, on a's main stream; ev_sent marks the end
template <typename F>
int group_exchange(cfdp_gpu **ranks, int G, int rowlen, F field) {
  for (int a = 0; a < G; a++) {
    cfdp_gpu *ga = ranks[a];
    HIP_TRY(hipSetDevice(ga->device));
    HIP_TRY(gg_launch_gather_rows(ga->d_sendidx, ga->send_off.back(), field(ga), rowlen, ga->adj.d_send, ga->s_main));
  }
  for (int a = 0; a < G; a++) {
    cfdp_gpu *ga = ranks[a];
    HIP_TRY(hipSetDevice(ga->device));
    for (size_t s = 0; s < ga->partner.size(); s++) {
      cfdp_gpu *gb = ranks[ga->partner[s]];
      int slot = -1;
      for (size_t i = 0; i < gb->partner.size(); i++)
        if (gb->partner[i] == a) slot = (int)i;
      const size_t n = (size_t)(ga->send_off[s + 1] - ga->send_off[s]) * rowlen;
      if (!n) continue;
      // b's ghost rows may still be read by b's previous adjoint launch (write-after-read)
      HIP_TRY(hipStreamWaitEvent(ga->s_main, gb->adj.ev_done, 0));
      double *dst = field(gb) + ((size_t)gb->nown + gb->recv_off[slot]) * rowlen;
      HIP_TRY(hipMemcpyPeerAsync(dst, gb->device, ga->adj.d_send + (size_t)ga->send_off[s] * rowlen, ga->device,
                                 n * sizeof(double), ga->s_main));
    }
    HIP_TRY(hipEventRecord(ga->adj.ev_sent, ga->s_main));
  }
  return 0;
}

}  // namespace

extern "C++" void cfdp_detail::adjoint_release(cfdp_gpu *g) {
  auto &A = g->adj;
  if (A.d_gbar || A.d_vbar || A.d_ivol || A.d_send) (void)hipDeviceSynchronize();
  (void)hipFree(A.d_gbar); (void)hipFree(A.d_vbar); (void)hipFree(A.d_ivol); (void)hipFree(A.d_send);
  if (A.ev_sent) (void)hipEventDestroy(A.ev_sent);
  if (A.ev_done) (void)hipEventDestroy(A.ev_done);
  A = cfdp_gpu::adjoint_state();
}

extern "C" {

int cfdp_gpu_set_grad_adjoint(cfdp_gpu *g, const double *gbar) {
  NEED_UPLOAD(g);
  if (!gbar) return fail("null gbar");
  if (adjoint_alloc(g)) return 1;
  const size_t len = (size_t)g->nown * 21;
  double *tmp = g->stage(len ? len : 1);
  if (!tmp) return fail("no pinned host memory for the staging image");
  const int nown = g->nown;
  const int *new2old = g->new2old.data();
#pragma omp parallel for schedule(static)
  for (int i = 0; i < nown; i++) memcpy(tmp + (size_t)i * 21, gbar + (size_t)new2old[i] * 21, 21 * sizeof(double));
  HIP_TRY(hipDeviceSynchronize());  // nothing may still read gbar
  if (len) HIP_TRY(hipMemcpy(g->adj.d_gbar, tmp, len * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int cfdp_gpu_get_var_adjoint(cfdp_gpu *g, double *vbar) {
  NEED_UPLOAD(g);
  if (!vbar) return fail("null vbar");
  if (adjoint_alloc(g)) return 1;
  HIP_TRY(hipDeviceSynchronize());
  const size_t len = (size_t)g->nown * 7;
  double *tmp = g->stage(len ? len : 1);
  if (!tmp) return fail("no pinned host memory for the staging image");
  if (len) HIP_TRY(hipMemcpy(tmp, g->adj.d_vbar, len * sizeof(double), hipMemcpyDeviceToHost));
  const int nown = g->nown;
  const int *new2old = g->new2old.data();
#pragma omp parallel for schedule(static)
  for (int i = 0; i < nown; i++) memcpy(vbar + (size_t)new2old[i] * 7, tmp + (size_t)i * 7, 7 * sizeof(double));
  return 0;
}

int cfdp_gpu_gradients_adjoint(cfdp_gpu *g, void *stream) {
  NEED_UPLOAD(g);
  if (adjoint_alloc(g)) return 1;
  return launch_adjoint(g, 0, stream ? (hipStream_t)stream : g->s_main);
}

int cfdp_gpu_adjoint_ptrs(cfdp_gpu *g, void **dev_gbar, void **dev_vbar) {
  NEED_UPLOAD(g);
  if (!dev_gbar || !dev_vbar) return fail("null output pointer");
  if (adjoint_alloc(g)) return 1;
  *dev_gbar = g->adj.d_gbar;
  *dev_vbar = g->adj.d_vbar;
  return 0;
}

int cfdp_gpu_adjoint_group(cfdp_gpu **ranks, int G, int with_exchange) {
  if (!ranks || G < 1) return fail("bad rank group");
  // everything is checked before anything is enqueued
  for (int a = 0; a < G; a++) {
    cfdp_gpu *ga = ranks[a];
    if (!ga) return fail("null context for rank %d", a);
    NEED_UPLOAD(ga);
    if (refuse_ipc(ga)) return 1;
    for (size_t s = 0; with_exchange && s < ga->partner.size(); s++) {
      const int b = ga->partner[s];
      if (b < 0 || b >= G || !ranks[b]) return fail("partner rank %d outside the in-process group", b);
      cfdp_gpu *gb = ranks[b];
      int slot = -1;
      for (size_t i = 0; i < gb->partner.size(); i++)
        if (gb->partner[i] == a) slot = (int)i;
      if (slot < 0) return fail("rank %d sends to %d which does not list it as partner", a, b);
      if (ga->send_off[s + 1] - ga->send_off[s] != gb->recv_off[slot + 1] - gb->recv_off[slot])
        return fail("halo size mismatch %d->%d: %d vs %d rows", a, b, ga->send_off[s + 1] - ga->send_off[s],
                    gb->recv_off[slot + 1] - gb->recv_off[slot]);
    }
  }
  for (int a = 0; a < G; a++)
    if (adjoint_alloc(ranks[a])) return 1;
  if (with_exchange) {
    bool vols = true;
    for (int a = 0; a < G; a++) vols = vols && ranks[a]->adj.ghost_ivol;
    if (!vols) {  // once: the owners' volumes into the ghost rows of every 1/V table
      if (group_exchange(ranks, G, 1, [](cfdp_gpu *x) { return x->adj.d_ivol; })) return 1;
      for (int a = 0; a < G; a++) ranks[a]->adj.ghost_ivol = true;
    }
    if (group_exchange(ranks, G, 21, [](cfdp_gpu *x) { return x->adj.d_gbar; })) return 1;
  }
  for (int b = 0; b < G; b++) {
    cfdp_gpu *gb = ranks[b];
    HIP_TRY(hipSetDevice(gb->device));
    if (with_exchange)
      for (int a : gb->partner) HIP_TRY(hipStreamWaitEvent(gb->s_main, ranks[a]->adj.ev_sent, 0));
    if (launch_adjoint(gb, with_exchange ? 1 : 0, gb->s_main)) return 1;
    HIP_TRY(hipEventRecord(gb->adj.ev_done, gb->s_main));
  }
  return 0;
}

int cfdp_gpu_step_adjoint_rccl(cfdp_gpu *g, int with_exchange) {
  NEED_UPLOAD(g);
  if (refuse_ipc(g)) return 1;
  const bool comm = with_exchange && !g->partner.empty();
  if (comm && !g->comm) return fail("no communicator: call cfdp_gpu_rccl_init()");
  if (adjoint_alloc(g)) return 1;
  auto &A = g->adj;
  // gather, messages and the face loop in the order of the main stream (the messages are ncclSend / ncclRecv on it)
  if (comm) {
    const int nsend = g->send_off.back();
    if (!A.ghost_ivol) {  // once: the owners' volumes into the ghost rows of the 1/V table
      HIP_TRY(gg_launch_gather_rows(g->d_sendidx, nsend, A.d_ivol, 1, A.d_send, g->s_main));
      if (rccl_exchange_rows(g, A.d_send, A.d_ivol + g->nown, 1, g->s_main)) return 1;
      A.ghost_ivol = true;
    }
    HIP_TRY(gg_launch_gather_rows(g->d_sendidx, nsend, A.d_gbar, 21, A.d_send, g->s_main));
    if (rccl_exchange_rows(g, A.d_send, A.d_gbar + (size_t)g->nown * 21, 21, g->s_main)) return 1;
  }
  if (launch_adjoint(g, comm ? 1 : 0, g->s_main)) return 1;
  HIP_TRY(hipEventRecord(A.ev_done, g->s_main));
  return 0;
}

}  // extern "C"
