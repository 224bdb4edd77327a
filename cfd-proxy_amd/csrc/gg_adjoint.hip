// gg_adjoint.hip -- the adjoint of the Green-Gauss gradient on gfx950: gbar -> vbar, the transposed face loop
// (operator and exchange argument: csrc/gg_adjoint.h).
//
// Owner computes, as the gradient loop does: one workgroup per tile, LPP lanes per point (1, 2, 4 or 8, the equations
// split across them as grad_cfg splits them), one walk over each owned point's incidence list in file order, partial sums
// in registers -- no atomics, the result is deterministic.  The data flow is the flux loop's: the rows of BOTH ends of
// every face are read, own and halo alike, so the tile stages the gbar rows of its own and halo points (168 bytes each)
// next to its blob, scales each staged row by 1/2V in place ONCE (as the flux loop forms P(g) once per staged row), and
// the face loop then needs one subtraction and three FMAs per equation and incidence.
//
// LDS image of a tile: [blob: 16-byte pieces, whole waves][rows: npts + nhalo rows of 3 eq_n doubles, + a wave of padding]
// [1/2V per row][the halo rows' numbers].
// Staging is LDS-DMA (global_load_lds): the blob in 16-byte pieces, the rows in 4-byte pieces -- a 168-byte row starts at
// 8 mod 16 every other row, which the 16-byte form cannot address.
#include "gg_adjoint.h"
#include "gg_device.h"  // xcd_tile, grad_cfg, gg_helpers / tile_helpers / list_chunk, glds16[_nt]

namespace {

constexpr size_t ADJ_LDS_MAX = 160 * 1024;

__device__ __forceinline__ void glds4(const void *src, unsigned char *lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                   (__attribute__((address_space(3))) void *)lds_wave_base, 4, 0, 0);
}

// U consecutive incidences of a point as one batch (the gradient loop's grad_batch): all words, then all operands, then
// the arithmetic.  eo[j] = where equation eq0 + j sits in a staged row (0 for a lane's equation outside the slice: it is
// computed from valid LDS and never stored).
template <int U, int NE>
__device__ __forceinline__ void adj_batch(const uint32_t *__restrict__ inc, int k, const double *__restrict__ nx,
                                          const double *__restrict__ ny, const double *__restrict__ nz,
                                          const double *__restrict__ srow, int rs, const int (&eo)[NE],
                                          const double (&sq)[NE][3], double (&acc)[NE]) {
  uint32_t w[U];
#pragma unroll
  for (int i = 0; i < U; i++) w[i] = inc[k + i];
  double n0[U], n1[U], n2[U], sn[U][NE][3];
#pragma unroll
  for (int i = 0; i < U; i++) {
    const uint32_t f = (w[i] >> 16) & 0x7FFFu;
    n0[i] = nx[f];
    n1[i] = ny[f];
    n2[i] = nz[f];
    const double *rp = srow + (w[i] & 0xFFFFu) * rs;
#pragma unroll
    for (int j = 0; j < NE; j++)
#pragma unroll
      for (int c = 0; c < 3; c++) sn[i][j][c] = rp[eo[j] + c];
  }
#pragma unroll
  for (int i = 0; i < U; i++) {
    // sigma = -1 (the owned end is p1 of the face): bit 31 of the word, put onto the sign bit of the term
    const int sgn = (int)(w[i] & 0x80000000u);
#pragma unroll
    for (int j = 0; j < NE; j++) {
      double d = n0[i] * (sq[j][0] - sn[i][j][0]);
      d = fma(n1[i], sq[j][1] - sn[i][j][1], d);
      d = fma(n2[i], sq[j][2] - sn[i][j][2], d);
      acc[j] += __hiloint2double(__double2hiint(d) ^ sgn, __double2loint(d));
    }
  }
}

// eq_lo, eq_n: the equations [eq_lo, eq_lo + eq_n) are staged and computed by this launch (0, 7 unless the LDS is short);
// FULL: eq_n == 7 (the staged row is the whole 168-byte row: compile-time row strides)
template <int LPP, bool NT, bool FULL>
__global__ __launch_bounds__(1024) void gg_adjoint_dma_kernel(gg_adj_args a, int tile_begin, int eq_lo, int eq_n_arg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = tile_begin + xcd_tile(blockIdx.x, gridDim.x);
  const cfdp_tile_desc td = a.tiles[t];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, w0 = tid & ~63;
  const int npts = td.npts, nrows = td.npts + td.nhalo;
  const int eq_n = FULL ? 7 : eq_n_arg;
  const int rw = 6 * eq_n, rs = 3 * eq_n;  // a staged row: 4-byte pieces, doubles
  const size_t rows_off = (size_t)((td.blob_qw + 63) & ~63) * 16;
  // (+ one wave of pieces: the halo part starts at any piece, so its last DMA instruction may reach 63 pieces past the end)
  const size_t fac_off = rows_off + (size_t)((nrows * rw + 63) & ~63) * 4 + 256;
  int *lrow = reinterpret_cast<int *>(smem + fac_off + (size_t)nrows * 8);  // [nhalo] the halo rows' numbers
  double *fac = reinterpret_cast<double *>(smem + fac_off);                  // [nrows] 1/2V (0: a ghost row whose s is 0)
  const int *hid = a.halo_idx + td.halo_off;
  const double *gb = a.gbar + eq_lo * 3;

  // ---- stage.  Every wave issues whole-wave DMA instructions; a lane past the end of a part re-reads that part's last
  // piece into the padding behind it (or into the first pieces of the next part, which are written again later, behind a
  // vmcnt(0) + barrier), so EXEC stays full.  (1) the blob and the OWN rows -- addresses known from the descriptor -- go
  // out first; (2) the halo rows' numbers and every row's 1/2V come in meanwhile (plain loads, one round trip); (3) then
  // the halo rows, all DMA instructions back to back, their numbers read from LDS.
  {
    const uint4 *b4 = a.blob + td.blob_off;
    const int qmax = td.blob_qw - 1;
    for (int q0 = w0; q0 < td.blob_qw; q0 += nthr) {
      const int q = q0 + lane < qmax ? q0 + lane : qmax;
      if constexpr (NT) glds16_nt(b4 + q, smem + (size_t)q0 * 16);
      else glds16(b4 + q, smem + (size_t)q0 * 16);
    }
    const int own = npts * rw, omax = own - 1;
    const uint32_t *gown = reinterpret_cast<const uint32_t *>(gb + (size_t)td.pstart * 21);
    for (int q0 = w0; q0 < own; q0 += nthr) {
      const int q = q0 + lane < omax ? q0 + lane : omax;
      const int r = q / rw, c = q - r * rw;
      glds4(gown + (size_t)r * 42 + c, smem + rows_off + (size_t)q0 * 4);
    }
    for (int r = tid; r < nrows; r += nthr) {
      const int row = r < npts ? td.pstart + r : hid[r - npts];
      if (r >= npts) lrow[r - npts] = row;
      fac[r] = row < a.nown || a.ghosts ? 0.5 * a.ivol[row] : 0.0;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
  __syncthreads();
  {
    const int q1 = nrows * rw, qmax = q1 - 1;
    for (int q0 = npts * rw + w0; q0 < q1; q0 += nthr) {
      const int q = q0 + lane < qmax ? q0 + lane : qmax;
      const int r = q / rw, c = q - r * rw;
      glds4(reinterpret_cast<const uint32_t *>(gb + (size_t)lrow[r - npts] * 21) + c, smem + rows_off + (size_t)q0 * 4);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
  __syncthreads();
  double *srow = reinterpret_cast<double *>(smem + rows_off);
  // s = gbar / 2V, in place, once per staged row (a ghost row of ghosts = 0: exactly 0, whatever its bytes are)
  for (int q = tid; q < nrows * rs; q += nthr) {
    const double f = fac[q / rs], x = srow[q];
    srow[q] = f != 0.0 ? x * f : 0.0;
  }
  __syncthreads();

  // ---- the face loop
  constexpr int NE = grad_cfg<LPP>::NE;
  constexpr int U = NE <= 2 ? 4 : (NE <= 4 ? 2 : 1);
  const int li = tid / LPP, sub = tid % LPP;
  const bool active = li < npts;
  const int plane = (td.nfaces * 8 + 15) & ~15;
  const int inc_bytes = (td.ninc * 4 + 15) & ~15;
  const double *nx = reinterpret_cast<const double *>(smem);
  const double *ny = reinterpret_cast<const double *>(smem + plane);
  const double *nz = reinterpret_cast<const double *>(smem + 2 * plane);
  const uint32_t *inc = reinterpret_cast<const uint32_t *>(smem + 3 * plane);
  const uint32_t *ioff = reinterpret_cast<const uint32_t *>(smem + 3 * plane + inc_bytes);
  // a long list is walked in chunks (cfdproxy_host.h): a HELPER lane group in a slot behind the tile's points takes one
  // chunk of some point's list; its sums join the point's below, in chunk order
  const gg_helpers hp = tile_helpers(smem, td, plane, inc_bytes);
  const bool helper = !active && li < npts + hp.n;
  int src = li, chunk = 0;
  if (helper) {
    const uint32_t hw = hp.tab[li - npts];
    src = (int)(hw & 0xFFFFu);
    chunk = (int)(hw >> 16);
  }
  const int eq0 = sub * NE;
  bool in[NE];
  int eo[NE];
#pragma unroll
  for (int j = 0; j < NE; j++) {
    const int e = eq0 + j;
    in[j] = e < 7 && e >= eq_lo && e < eq_lo + eq_n;
    eo[j] = in[j] ? (e - eq_lo) * 3 : 0;
  }
  double acc[NE];
#pragma unroll
  for (int j = 0; j < NE; j++) acc[j] = 0.0;
  int nchunks = 1;
  if (active || helper) {
    int k, ke, ks0, ke0;
    list_chunk(ioff, src, chunk, k, ke, ks0, ke0, nchunks);
    double sq[NE][3];
#pragma unroll
    for (int j = 0; j < NE; j++)
#pragma unroll
      for (int c = 0; c < 3; c++) sq[j][c] = srow[src * rs + eo[j] + c];
    for (; k + U <= ke; k += U) adj_batch<U, NE>(inc, k, nx, ny, nz, srow, rs, eo, sq, acc);
    for (; k < ke; k++) adj_batch<1, NE>(inc, k, nx, ny, nz, srow, rs, eo, sq, acc);
  }
  if (hp.n) {  // (uniform per workgroup) the helpers' sums, through the scratch rows of the blob (24 doubles per helper)
    if (helper) {
#pragma unroll
      for (int j = 0; j < NE; j++)
        if (eq0 + j < 7) hp.scratch[(li - npts) * 24 + eq0 + j] = acc[j];
    }
    __syncthreads();
    if (active && nchunks > 1)
      for (int h = 0; h < hp.n; h++)
        if ((int)(hp.tab[h] & 0xFFFFu) == li) {
#pragma unroll
          for (int j = 0; j < NE; j++)
            if (eq0 + j < 7) acc[j] += hp.scratch[h * 24 + eq0 + j];
        }
  }
  // ---- vbar rows (a point without faces: 0)
  if (active) {
    double *out = a.vbar + (size_t)(td.pstart + li) * 7;
#pragma unroll
    for (int j = 0; j < NE; j++)
      if (in[j]) out[eq0 + j] = acc[j];
  }
}

__global__ void gg_gather_rows_kernel(const int *__restrict__ idx, int n, const double *__restrict__ rows, int rowlen,
                                      double *__restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * rowlen) return;
  const long j = i / rowlen, c = i - j * rowlen;
  out[i] = rows[(size_t)idx[j] * rowlen + c];
}

template <typename K> hipError_t allow_lds(K *kernel) {
  static bool done[64] = {false};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ADJ_LDS_MAX);
  if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
  return e;
}

template <int L, bool NT>
hipError_t launch_adjoint(const gg_adj_args &a, int tile_begin, int ntiles, int block, size_t lds, int eq_lo, int eq_n,
                          hipStream_t stream) {
  auto *k = eq_n == 7 ? gg_adjoint_dma_kernel<L, NT, true> : gg_adjoint_dma_kernel<L, NT, false>;
  if (lds > 64 * 1024) {
    const hipError_t e = allow_lds(k);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, dim3(ntiles), dim3(block), lds, stream, a, tile_begin, eq_lo, eq_n);
  return hipGetLastError();
}

}  // namespace

size_t gg_adjoint_lds_bytes(int max_rows, int max_blob_qw, int eq_n) {
  const size_t blob = (size_t)((max_blob_qw + 63) & ~63) * 16;
  const size_t rows = (size_t)(((size_t)max_rows * 6 * eq_n + 63) & ~(size_t)63) * 4 + 256;
  return blob + rows + (size_t)max_rows * 12;
}

int gg_adjoint_slice(int max_rows, int max_blob_qw) {
  int n = 7;
  while (n > 0 && gg_adjoint_lds_bytes(max_rows, max_blob_qw, n) > ADJ_LDS_MAX) n--;
  return n;
}

hipError_t gg_launch_adjoint(const gg_adj_args &a, int lanes, int tile_begin, int ntiles, int tile_points, int max_rows,
                             int max_blob_qw, bool nt, hipStream_t stream) {
  if (ntiles <= 0) return hipSuccess;
  const int block = ((tile_points * lanes + 63) / 64) * 64;
  if (block > 1024 || block <= 0) return hipErrorInvalidConfiguration;
  // (a staged row index must fit the 16 bits of an incidence word, as it does in every plan the tiler emits)
  const int slice = gg_adjoint_slice(max_rows, max_blob_qw);
  if (slice <= 0) return hipErrorInvalidConfiguration;
  for (int lo = 0; lo < 7; lo += slice) {
    const int n = 7 - lo < slice ? 7 - lo : slice;
    const size_t lds = gg_adjoint_lds_bytes(max_rows, max_blob_qw, n);
    hipError_t e = hipErrorInvalidValue;
#define ADJ_CASE(L)                                                                                   \
  case L:                                                                                             \
    e = nt ? launch_adjoint<L, true>(a, tile_begin, ntiles, block, lds, lo, n, stream)                \
           : launch_adjoint<L, false>(a, tile_begin, ntiles, block, lds, lo, n, stream);              \
    break;
    switch (lanes) {
      ADJ_CASE(1)
      ADJ_CASE(2)
      ADJ_CASE(4)
      ADJ_CASE(8)
      default: break;
    }
#undef ADJ_CASE
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t gg_launch_gather_rows(const int *idx, int n, const double *rows, int rowlen, double *out, hipStream_t stream) {
  const long total = (long)n * rowlen;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(gg_gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, idx, n, rows, rowlen, out);
  return hipGetLastError();
}
