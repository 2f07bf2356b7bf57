// Device-resident boundary (sipx_finalize_dev / sipx_reset_dev / sipx_download_dev): every vector of a call -- m, x and the
// y_i, l_i of all sets -- moves between the caller's device buffers (the reference's row order) and the context's padded
// arrays in ONE launch.  A launch carries a table of segments in its arguments; a segment is one operator block of one
// vector (or a whole vector where the two layouts coincide).  The workgroups are dealt onto the segments in proportion to
// their sizes, each walks its segment with a grid stride.  Pure streaming: 16-byte accesses per lane wherever both sides
// allow them (the rows of a block run along dimension 1 in both layouts: a vector of four never leaves its row when n1 is a
// multiple of four and both bases are 16-byte aligned), one element per lane otherwise (difference along dimension 1, odd
// grids).  The pads of the padded layout are never written: they keep their zeros.
#include <algorithm>
#include <stdexcept>
#include <string>

#include "sipx_device.h"

namespace sipx {

// Row r = (i, j, k), column-major over the block's own extents (d0, d1, .), lives at padded entry i + n0 (j + n1 k).
// PACK: rows[r] = pad[e];  otherwise pad[e] = rows[r].
template <typename T, bool PACK, int V>
__device__ __forceinline__ void io_walk(const IoSeg<T>& S, unsigned first, unsigned stride) {
  const unsigned items = S.nrows / V;
  for (unsigned it = first; it < items; it += stride) {
    const unsigned r = it * V;
    unsigned e = r;
    if (!S.linear) {
      const unsigned t = r / S.d0, i = r - t * S.d0, k = t / S.d1, j = t - k * S.d1;
      e = i + S.n0 * (j + S.n1 * k);
    }
    if (PACK) stv<T, V>(S.rows + r, ldv<T, V>(S.pad + e));
    else stv<T, V>(S.pad + e, ldv<T, V>(S.rows + r));
  }
}

// Broadcast segment: row r = (i, j, k) of the block takes rows[c], c its coordinate along the segment's direction.  With V = 4 the
// four entries share j and k (d0 == n0, a multiple of four): along dimension 1 they are four consecutive values of `rows`, one
// 16-byte load; along the others one value, read once (every lane of a row reads the same address: one request per wave and
// row) and stored as 16 bytes.
template <typename T, int V>
__device__ __forceinline__ void io_walk_bcast(const IoSeg<T>& S, unsigned first, unsigned stride) {
  const unsigned items = S.nrows / V, bdir = S.bdir - 1u;
  for (unsigned it = first; it < items; it += stride) {
    const unsigned r = it * V;
    const unsigned t = r / S.d0, i = r - t * S.d0, k = t / S.d1, j = t - k * S.d1;
    const unsigned e = i + S.n0 * (j + S.n1 * k);
    Vec<T, V> x;
    if (bdir == 0u) {
      x = ldv<T, V>(S.rows + i);
    } else {
      const T b = S.rows[bdir == 1u ? j : k];
#pragma unroll
      for (int q = 0; q < V; ++q) x.v[q] = b;
    }
    stv<T, V>(S.pad + e, x);
  }
}

template <typename T, bool PACK>
__global__ __launch_bounds__(BLOCK) void k_io_rows(IoArgs<T> A) {
  int s = 0;                                                    // (uniform over the workgroup)
  while (s + 1 < A.nseg && blockIdx.x >= A.seg[s + 1].blk0) ++s;
  const IoSeg<T> S = A.seg[s];
  const unsigned nb = (s + 1 < A.nseg ? A.seg[s + 1].blk0 : A.nblocks) - S.blk0;
  const unsigned first = (blockIdx.x - S.blk0) * BLOCK + threadIdx.x, stride = nb * BLOCK;
  if (!PACK && S.bdir) {
    if (S.vec) io_walk_bcast<T, 4>(S, first, stride);
    else io_walk_bcast<T, 1>(S, first, stride);
    return;
  }
  if (S.vec) io_walk<T, PACK, 4>(S, first, stride);
  else io_walk<T, PACK, 1>(S, first, stride);
}

template <typename T>
void io_seg_shape(IoSeg<T>& S, const Grid& g, int dir, long long nrows, const T* rows, const T* pad) {
  S.rows = const_cast<T*>(rows);
  S.pad = const_cast<T*>(pad);
  S.nrows = (unsigned)nrows;
  S.n0 = (unsigned)g.n[0];
  S.n1 = (unsigned)g.n[1];
  S.d0 = S.n0 - (dir == 0 ? 1u : 0u);
  S.d1 = S.n1 - (dir == 1 ? 1u : 0u);
  // the layouts coincide when no pad lies in front of the last row: whole vectors (dir < 0), a difference along the last dimension
  S.linear = (S.d0 == S.n0 && (S.d1 == S.n1 || nrows <= (long long)S.d0 * S.d1)) ? 1u : 0u;
  const bool rows_fit = S.linear ? (nrows % 4 == 0) : (S.d0 == S.n0 && S.n0 % 4 == 0);
  S.vec = (rows_fit && aligned16(rows, pad)) ? 1u : 0u;
  S.blk0 = 0;
  S.bdir = 0;
}

template <typename T>
void io_seg_bcast(IoSeg<T>& S, const Grid& g, int dir, int fdir, long long nrows, const T* rows, const T* pad) {
  if (fdir < 0 || fdir > 2) throw std::runtime_error("internal: broadcast segment along an unknown direction");
  io_seg_shape<T>(S, g, dir, nrows, rows, pad);
  S.bdir = 1u + (unsigned)fdir;
  // four entries of one grid row at a time: the rows of the block are whole grid rows, a multiple of four long (so nrows is one
  // too); `rows` is then read at multiples of four (fdir == 0) or one value at a time
  S.vec = (S.d0 == S.n0 && S.n0 % 4 == 0 && aligned16(pad) && (fdir != 0 || aligned16(rows))) ? 1u : 0u;
}

template <typename T>
void io_rows(hipStream_t s, IoArgs<T>& A, bool pack, int max_blocks) {
  if (A.nseg <= 0) return;
  if (A.nseg > IO_MAXSEG) throw std::runtime_error("internal: too many segments in one transfer launch");
  // workgroups in proportion to the thread-iterations of a segment, at least one each, no more than a segment has work for
  double total = 0;
  for (int q = 0; q < A.nseg; ++q) total += (double)(A.seg[q].nrows / (A.seg[q].vec ? 4 : 1) + 1);
  const int cap = max_blocks > A.nseg ? max_blocks : A.nseg;
  unsigned at = 0;
  double bytes = 0;
  for (int q = 0; q < A.nseg; ++q) {
    const long long items = A.seg[q].nrows / (A.seg[q].vec ? 4 : 1);
    long long nb = (long long)((double)cap * (double)(items + 1) / total);
    nb = std::min<long long>(nb, (items + BLOCK - 1) / BLOCK);
    if (nb < 1) nb = 1;
    A.seg[q].blk0 = at;
    at += (unsigned)nb;
    bytes += 2.0 * (double)A.seg[q].nrows * sizeof(T);
  }
  A.nblocks = at;
  ObsScope obs(KID_OTHER, s, bytes);
  if (pack) hipLaunchKernelGGL((k_io_rows<T, true>), dim3(at), dim3(BLOCK), 0, s, A);
  else hipLaunchKernelGGL((k_io_rows<T, false>), dim3(at), dim3(BLOCK), 0, s, A);
  SIPX_HIP(hipGetLastError());
}

#define SIPX_IO_INST(T)                                                                                   \
  template void io_seg_shape<T>(IoSeg<T>&, const Grid&, int, long long, const T*, const T*);             \
  template void io_seg_bcast<T>(IoSeg<T>&, const Grid&, int, int, long long, const T*, const T*);        \
  template void io_rows<T>(hipStream_t, IoArgs<T>&, bool, int);
SIPX_IO_INST(float)
SIPX_IO_INST(double)

}  // namespace sipx
