// gg_adjoint.h -- launch wrappers of the adjoint (transposed) Green-Gauss face loop (csrc/gg_adjoint.hip; internal to
// libcfdproxy_hip.so).
//
// Forward, per owned point p (src/gradients.c:25-147):  g[p][e][d] = 1/V_p sum_{f in p} sigma_{f,p} n_f[d] 1/2 (v[p0][e] + v[p1][e]).
// Adjoint: with s[p] = gbar[p] / V_p (21 numbers per point), for every owned point q
//     vbar[q][e] = sum_{f in q} sigma_{f,q} 1/2 n_f . (s[q][e] - s[r_f][e])          (r_f = the other end of f)
// A ghost point's s is either 0 (ghosts = 0: the transpose of the partition's own map v_own -> g_own) or its owner's s,
// delivered by the forward halo exchange of raw 21-double gbar rows (ghosts = 1: the transpose of the global operator).
#ifndef CFDP_GG_ADJOINT_H
#define CFDP_GG_ADJOINT_H

#include <hip/hip_runtime.h>

#include "cfdproxy_host.h"  // cfdp_tile_desc

struct gg_adj_args {
  const cfdp_tile_desc *tiles;  // device copies
  const uint4 *blob;
  const int *halo_idx;
  const double *gbar;           // [nall][21] device numbering: owned rows, then ghost rows in message order
  const double *ivol;           // [nall] 1/V per row, device numbering (ghost rows: the OWNER's volume)
  double *vbar;                 // [nown][7] device numbering
  int nown;
  int ghosts;                   // 0: s[ghost] = 0; 1: ghost rows of gbar hold the owners' rows
};

// one launch -- or one per equation slice, when whole 168-byte rows of every staged point do not fit the LDS -- over the
// tiles [tile_begin, tile_begin + ntiles): tile_points = lane groups per tile (points + helper groups), max_rows = staged
// rows (own + halo) and max_blob_qw = blob 16-byte units of the largest tile among them
hipError_t gg_launch_adjoint(const gg_adj_args &a, int lanes, int tile_begin, int ntiles, int tile_points, int max_rows,
                             int max_blob_qw, bool nt, hipStream_t stream);
// LDS bytes of one workgroup of the adjoint loop with `eq_n` (1..7) equations of every row staged
size_t gg_adjoint_lds_bytes(int max_rows, int max_blob_qw, int eq_n);
// the equations per row one launch stages for these sizes (7: whole rows; 0: not even one fits)
int gg_adjoint_slice(int max_rows, int max_blob_qw);
// out row j = the `rowlen` doubles of row idx[j] of `rows` (plain rows: no stored form)
hipError_t gg_launch_gather_rows(const int *idx, int n, const double *rows, int rowlen, double *out, hipStream_t stream);

#endif
