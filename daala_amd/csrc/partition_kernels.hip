/* partition_kernels.hip - the leaves of a block-size map as lists, and the copies that put them into
   planes tiled by ONE block size and back.

   The PVQ band stages (pvq_bands.hip, pvq_refbands.hip) take planes tiled by one block size.  A frame coded
   at its own block-size map (odhip_forward_partition, odhip_inverse_partition) holds leaves of up to five
   sizes, each transformed where it lies.  So the leaves of each size s are listed, gathered into a dense
   plane set of N x N blocks (N = 4 << s) - a plane of whole blocks is all the band stages ask for -, the
   stages run on the dense sets as they are, and the dequantised blocks are scattered back.

   The rule (od_compute_dcts, src/encode.c:1466-1470, walked top-down): node (bx, by) of luma level bsi reads
   the map at its top-left entry, bs = max(value, dec); bs == bsi is a leaf of size bsi - dec, anything else
   splits.  Block (bx, by) of size s is therefore a leaf iff no ancestor is one and its own entry says so:
   at most five map reads per block, no recursion, and the same function on the host and on the device.

   Kernels:
     k_part_rows<false>   one wavefront per (size, block row, plane): counts the leaves of the row
     k_part_scan          one workgroup per (size, plane): exclusive scan of the row counts, the list's length
     k_part_rows<true>    the same walk again: a ballot per 64 blocks gives every leaf its place behind the
                          row's offset - ascending index order, no atomics, the same lists every run
     k_part_copy<SCATTER> 16-byte vectors.  Consecutive lanes take consecutive vectors of a row of the DENSE
                          set (N/4 lanes cover one block row, 4N contiguous bytes on both sides; a wavefront
                          covers 64/(N/4) blocks, sixty-four of them at 4x4), and every lane moves four rows
                          of its block: one list entry and one division per 64 bytes, four loads in flight.
                          The gather writes every vector of the dense set, zeros where no leaf lies.
     k_cfl_part           chroma-from-luma references at a map (odhip_cfl_refs_partition): one workgroup per
                          64x64 luma superblock and luma plane, the 64 map bytes in LDS, four chroma samples of
                          one row per thread - see "chroma from luma at a map" below. */
#include <string.h>
#include "../../include/daala_hip.h"
#include "od_buf.cuh"
#include "od_cfl.cuh"
#include "od_ctx.cuh"

namespace {

constexpr int kTop = ODHIP_NBSIZES - 1;   /* the superblock's luma level */
constexpr int kCopyThreads = 256;
constexpr int kCopyPlanes = 32;           /* planes per copy launch: their counts travel in the arguments */

struct PartMap {
  const unsigned char *bsize;    /* frame f's map at bsize + f*frame_stride */
  long frame_stride;
  int bstride;
  int planes_per_frame;
  int dec;
};

/* Is block (bx, by) of size s (in units of its own size) a leaf of plane p's map? */
__host__ __device__ inline bool part_is_leaf(const PartMap &m, int p, int s, int bx, int by) {
  const unsigned char *map = m.bsize + (long)(p/m.planes_per_frame)*m.frame_stride;
  const int bsi = s + m.dec;
  for (int l = kTop; l >= bsi; l--) {
    const int ax = bx >> (l - bsi);
    const int ay = by >> (l - bsi);
    int v = map[(long)((ay << l) >> 1)*m.bstride + ((ax << l) >> 1)];
    if (v < m.dec) v = m.dec;
    if (v == l) return l == bsi;
  }
  return false;
}

struct PartGeom {
  int nplanes;
  int w;
  int h;
  int nsizes;                       /* 5 - dec */
  int row0[ODHIP_NBSIZES + 1];      /* first block row of size s among the rows of all sizes */
  size_t list0[ODHIP_NBSIZES + 1];  /* first entry of size s's lists: [nplanes][(w/N)*(h/N)] */
};

PartGeom part_geom(int nplanes, int w, int h, int dec) {
  PartGeom g;
  memset(&g, 0, sizeof(g));
  g.nplanes = nplanes;
  g.w = w;
  g.h = h;
  g.nsizes = ODHIP_NBSIZES - dec;
  for (int s = 0; s < ODHIP_NBSIZES; s++) {
    const int n = 4 << s;
    const bool on = s < g.nsizes;
    g.row0[s + 1] = g.row0[s] + (on ? h/n : 0);
    g.list0[s + 1] = g.list0[s] + (on ? (size_t)nplanes*(w/n)*(h/n) : 0);
  }
  return g;
}

/* What every entry point checks first (odhip_forward_partition's rules for the plane set). */
bool part_planes_ok(int nplanes, int w, int h, int dec) {
  if (nplanes <= 0 || (dec != 0 && dec != 1)) return false;
  const int tile = 64 >> dec;
  return w > 0 && h > 0 && w % tile == 0 && h % tile == 0;
}

bool part_map_ok(const void *bsize, int w, int dec, int bstride, int planes_per_frame) {
  return bsize && planes_per_frame >= 1 && bstride >= (w/(64 >> dec))*8;
}

struct PartRowsArgs {
  PartMap m;
  PartGeom g;
  unsigned *rows;      /* [nplanes][rows of all sizes]: the count, after the scan the offset, of a block row */
  uint32_t *lists;
};

template <bool WRITE>
__global__ __launch_bounds__(64) void k_part_rows(PartRowsArgs a) {
  const int lane = threadIdx.x;
  const int r = blockIdx.x;
  const int p = blockIdx.y;
  int s = 0;
  while (r >= a.g.row0[s + 1]) s++;
  const int by = r - a.g.row0[s];
  const int n = 4 << s;
  const int nbx = a.g.w/n;
  unsigned *row = a.rows + (size_t)p*a.g.row0[ODHIP_NBSIZES] + r;
  uint32_t *list = a.lists + a.g.list0[s] + (size_t)p*nbx*(a.g.h/n);
  unsigned at = WRITE ? *row : 0;
  for (int x0 = 0; x0 < nbx; x0 += 64) {
    const int bx = x0 + lane;
    const bool leaf = bx < nbx && part_is_leaf(a.m, p, s, bx, by);
    const unsigned long long mask = __ballot(leaf);
    if (WRITE && leaf) list[at + __popcll(mask & ((1ull << lane) - 1))] = (uint32_t)by*nbx + bx;
    at += __popcll(mask);
  }
  if (!WRITE && lane == 0) *row = at;
}

/* counts[s*nplanes + p] = the leaves of size s in plane p; the row counts become the rows' offsets */
__global__ __launch_bounds__(256) void k_part_scan(PartGeom g, unsigned *rows, int32_t *counts) {
  __shared__ unsigned sh[256];
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const int p = blockIdx.y;
  unsigned *row = rows + (size_t)p*g.row0[ODHIP_NBSIZES] + g.row0[s];
  const int n = g.row0[s + 1] - g.row0[s];
  unsigned carry = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + tid;
    const unsigned v = i < n ? row[i] : 0;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const unsigned t = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    if (i < n) row[i] = carry + sh[tid] - v;
    carry += sh[255];
    __syncthreads();
  }
  if (tid == 0) counts[s*g.nplanes + p] = (int32_t)carry;
}

struct PartCopyArgs {
  od_coeff *dst;            /* SCATTER: the coefficient planes; else the dense set */
  const od_coeff *src;
  const uint32_t *list;     /* [nplanes][cap] of this size */
  int w;
  int s;
  int nbx;                  /* w / N */
  unsigned cap;             /* (w/N)*(h/N) */
  int hd;                   /* rows of a dense plane */
  int h;
  int plane0;               /* first plane of this launch */
  int count[kCopyPlanes];
};

template <bool SCATTER>
__global__ __launch_bounds__(kCopyThreads) void k_part_copy(PartCopyArgs a) {
  const unsigned vw = (unsigned)a.w >> 2;                   /* vectors per row */
  const unsigned t = blockIdx.x*kCopyThreads + threadIdx.x;
  if (t >= vw*((unsigned)a.hd >> 2)) return;
  const int p = a.plane0 + blockIdx.y;
  const unsigned y0 = (t/vw) << 2;                          /* four rows of one block: N >= 4 */
  const unsigned xv = t % vw;
  const int n = 4 << a.s;
  const unsigned j = (y0 >> (2 + a.s))*a.nbx + (xv >> a.s); /* the block's place in the dense plane */
  const bool listed = j < (unsigned)a.count[blockIdx.y];
  unsigned idx = listed ? a.list[(size_t)p*a.cap + j] : 0;
  const bool leaf = listed && idx < a.cap;                  /* a foreign list cannot send a copy outside */
  if (!leaf) idx = 0;
  const unsigned sby = idx/a.nbx;
  const unsigned sbx = idx - sby*a.nbx;
  const size_t sparse = ((size_t)p*a.h + sby*n + (y0 & (n - 1)))*a.w + (size_t)sbx*n + ((xv & ((1u << a.s) - 1)) << 2);
  const size_t dense = ((size_t)p*a.hd + y0)*a.w + ((size_t)xv << 2);
  const size_t from = SCATTER ? dense : sparse;
  const size_t to = SCATTER ? sparse : dense;
  if (SCATTER && !leaf) return;
  int4 v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    v[k] = leaf ? *reinterpret_cast<const int4 *>(a.src + from + (size_t)k*a.w) : make_int4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) *reinterpret_cast<int4 *>(a.dst + to + (size_t)k*a.w) = v[k];
}

/* per context: the block rows' counts / offsets and the landing place of the lists' lengths */
struct PartState {
  DeviceBuf<unsigned> rows;
  DeviceBuf<int32_t> d_counts;
  PinnedBuf<int32_t> h_counts;
};

/* Hd_s = N * max_p ceil(count[p] / (w/N)); -1 for a count outside 0 .. (w/N)*(h/N) */
int dense_rows(const int32_t *count, int nplanes, int w, int h, int s) {
  const int n = 4 << s;
  const int nbx = w/n;
  const long cap = (long)nbx*(h/n);
  int rows = 0;
  for (int p = 0; p < nplanes; p++) {
    if (count[p] < 0 || count[p] > cap) return -1;
    const int r = (count[p] + nbx - 1)/nbx;
    if (r > rows) rows = r;
  }
  return rows*n;
}

template <bool SCATTER>
int part_copy(od_coeff *d_dst, const od_coeff *d_src, int s, const uint32_t *d_list, const int32_t *count, int nplanes,
 int w, int h, int dec, odhip_stream stream) {
  if (!d_dst || !d_src || !d_list || !count || !part_planes_ok(nplanes, w, h, dec) || s < 0 || s > kTop - dec
   || (((uintptr_t)d_dst | (uintptr_t)d_src) & 15)) {
    return ODHIP_EINVAL;
  }
  const int hd = dense_rows(count, nplanes, w, h, s);
  if (hd < 0) return ODHIP_EINVAL;
  if (hd == 0) return ODHIP_SUCCESS;      /* no leaf of this size: there is no dense set */
  const int n = 4 << s;
  PartCopyArgs a;
  memset(&a, 0, sizeof(a));
  a.dst = d_dst;
  a.src = d_src;
  a.list = d_list;
  a.w = w;
  a.s = s;
  a.nbx = w/n;
  a.cap = (unsigned)(w/n)*(unsigned)(h/n);
  a.hd = hd;
  a.h = h;
  const size_t units = (size_t)(w >> 2)*(hd >> 2);
  if (units > 0xffffffffu - kCopyThreads) return ODHIP_EINVAL;
  const unsigned gx = (unsigned)((units + kCopyThreads - 1)/kCopyThreads);
  for (int p0 = 0; p0 < nplanes; p0 += kCopyPlanes) {
    const int np = nplanes - p0 < kCopyPlanes ? nplanes - p0 : kCopyPlanes;
    a.plane0 = p0;
    for (int i = 0; i < np; i++) a.count[i] = count[p0 + i];
    k_part_copy<SCATTER><<<dim3(gx, (unsigned)np), kCopyThreads, 0, (hipStream_t)stream>>>(a);
  }
  return odhip_check_launch();
}


/* ---- chroma from luma at a map ------------------------------------------------------------------------
   od_resample_luma_coeffs (src/intra.c:72-109) as od_block_encode calls it per leaf (src/encode.c:1681-1686),
   read from the DEQUANTISED luma plane that odhip_partition_scatter leaves and odhip_inverse_partition takes.
   4:2:0: a luma leaf of N = 4 << m, m >= 1, at luma (Y0, X0) predicts the chroma leaf at (Y0/2, X0/2) with its
   upper-left quarter, DC included; map value 0 merges the 2x2 corners of four 4x4 luma blocks with
   od_tf_up_hv_lp (src/tf.c:82-108) and scales by OD_CFL_SCALING4 (src/intra.c:65-70): od_cfl_tf4 of od_cfl.cuh,
   which k_cfl_ref_tf of pvq_bands.hip feeds from pulses.  The MAP VALUE decides between the two 4x4 chroma leaves
   (obs at src/encode.c:1685), not the chroma size.  4:4:4: the block itself.

   Addresses: chroma sample (cy, cx) of a superblock's 32 x 32, in a leaf with chroma origin (oy, ox) inside
   that superblock, reads luma (cy + oy, cx + ox) of the superblock's 64 x 64 - oy <= cy < 32, so the sum stays
   below 64 whatever byte the map holds; the TF rows are 2*oy + (cy & 3)/2 + {0, 4} <= 61.  The map is read at
   (oy/4, ox/4) of the superblock's 8 x 8 entries only.  The same two functions serve the kernel and the host
   entry point. */
constexpr int kCflThreads = 256;

struct CflLeaf {
  int oy;     /* the leaf's origin in the superblock's chroma samples */
  int ox;
  bool tf;    /* map value 0: four 4x4 luma blocks */
};

/* The 4:2:0 chroma leaf that holds sample (cy, cx) of a superblock: odhip_partition_leaves' walk (part_is_leaf
   with dec = 1) from the top down; what reaches the 8x8 luma level is a 4x4 chroma leaf. */
__host__ __device__ inline CflLeaf cfl_leaf(const unsigned char *sbmap, int mstride, int cy, int cx) {
  for (int l = kTop; l > 1; l--) {
    const int mask = ~((2 << l) - 1);       /* a node of luma level l is 2 << l chroma samples wide */
    const int oy = cy & mask;
    const int ox = cx & mask;
    if (sbmap[(oy >> 2)*mstride + (ox >> 2)] == l) return {oy, ox, false};
  }
  const int oy = cy & ~3;
  const int ox = cx & ~3;
  return {oy, ox, sbmap[(oy >> 2)*mstride + (ox >> 2)] == 0};
}

/* N consecutive coefficients: one 16- or 8-byte vector on the device (the entry point checks the bases), plain
   copies on the host, whose planes need no alignment */
template <int N>
__host__ __device__ inline void cfl_load(od_coeff *v, const od_coeff *p) {
#ifdef __HIP_DEVICE_COMPILE__
  if (N == 4) {
    const int4 t = *reinterpret_cast<const int4 *>(p);
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  }
  else {
    const int2 t = *reinterpret_cast<const int2 *>(p);
    v[0] = t.x;
    v[1] = t.y;
  }
#else
  memcpy(v, p, N*sizeof(od_coeff));
#endif
}

/* out = the reference of chroma samples (cy, cx .. cx + 3), cx a multiple of 4, of the superblock whose luma
   samples start at luma (row stride w) and whose map entries start at sbmap (row stride mstride; not read at
   dec = 0).  No leaf is narrower than 4, so the four samples share their leaf. */
__host__ __device__ inline void cfl_group(od_coeff out[4], const od_coeff *luma, int w, const unsigned char *sbmap,
 int mstride, int dec, int cy, int cx) {
  if (!dec) {
    cfl_load<4>(out, luma + (long)cy*w + cx);
    return;
  }
  const CflLeaf lf = cfl_leaf(sbmap, mstride, cy, cx);
  if (!lf.tf) {
    cfl_load<4>(out, luma + (long)(cy + lf.oy)*w + cx + lf.ox);
    return;
  }
  /* row i of the 4x4 leaf comes from the Haar groups (gy, 0) and (gy, 1) of od_tf_up_hv_lp: coefficient
     (gy, gx) of the four 4x4 luma blocks of the 8x8 area */
  const int i = cy & 3;
  const int gy = i >> 1;
  const od_coeff *top = luma + (long)(2*lf.oy + gy)*w + 2*lf.ox;
  od_coeff a[2];      /* upper left block */
  od_coeff b[2];      /* upper right */
  od_coeff c[2];      /* lower left */
  od_coeff d[2];      /* lower right */
  cfl_load<2>(a, top);
  cfl_load<2>(b, top + 4);
  cfl_load<2>(c, top + 4*(long)w);
  cfl_load<2>(d, top + 4*(long)w + 4);
#pragma unroll
  for (int j = 0; j < 4; j++) out[j] = od_cfl_tf4(a[j >> 1], b[j >> 1], c[j >> 1], d[j >> 1], i, j);
}

struct CflPartArgs {
  od_coeff *ref;
  const od_coeff *luma;
  const unsigned char *bsize;
  long frame_stride;
  int bstride;
  int w;
  int h;
  int dec;
  int planes_per_frame;
  int plane0;              /* first luma plane of this launch */
};

/* blockIdx.x: the superblock, blockIdx.y: the luma plane.  A thread owns groups tid, tid + 256, ..: one at
   4:2:0 (32 rows x 8 groups), four at 4:4:4 (64 rows x 16 groups). */
__global__ __launch_bounds__(kCflThreads) void k_cfl_part(CflPartArgs a) {
  __shared__ unsigned char sbmap[64];
  const int tid = threadIdx.x;
  const int nsbx = a.w >> 6;
  const int sby = blockIdx.x/nsbx;
  const int sbx = blockIdx.x - sby*nsbx;
  const int p = a.plane0 + blockIdx.y;
  if (a.dec) {
    if (tid < 64) {
      sbmap[tid] = a.bsize[p*a.frame_stride + (long)(sby*8 + (tid >> 3))*a.bstride + sbx*8 + (tid & 7)];
    }
    __syncthreads();
  }
  const int side = 64 >> a.dec;            /* the superblock in samples of the reference planes */
  const int gshift = 4 - a.dec;            /* log2 of the groups of a row */
  const int cw = a.w >> a.dec;
  const int ch = a.h >> a.dec;
  const size_t per = (size_t)cw*ch;
  const od_coeff *luma = a.luma + ((size_t)p*a.h + sby*64)*a.w + sbx*64;
  od_coeff *ref = a.ref + (size_t)p*a.planes_per_frame*per + (size_t)sby*side*cw + sbx*side;
  for (int g = tid; g < side << gshift; g += kCflThreads) {
    const int cy = g >> gshift;
    const int cx = (g & ((1 << gshift) - 1)) << 2;
    od_coeff v[4];
    cfl_group(v, luma, a.w, sbmap, 8, a.dec, cy, cx);
    const int4 o = make_int4(v[0], v[1], v[2], v[3]);
    od_coeff *dst = ref + (size_t)cy*cw + cx;
    for (int k = 0; k < a.planes_per_frame; k++) *reinterpret_cast<int4 *>(dst + k*per) = o;
  }
}

/* odhip_cfl_refs_partition's rules for the plane and the map, shared with the host entry point */
bool cfl_part_ok(const void *ref, const void *luma, int w, int h, int dec, const void *bsize, int bstride) {
  return ref && luma && bsize && ref != luma && (dec == 0 || dec == 1) && w > 0 && h > 0 && w % 64 == 0 && h % 64 == 0
   && bstride >= w/8;
}
}  // namespace

extern "C" int odhip_partition_leaves_host(uint32_t *lists, int32_t *count, int nplanes, int w, int h, int dec,
 const uint8_t *bsize, int bstride, long bsize_frame_stride, int planes_per_frame) {
  if (!lists || !count || !part_planes_ok(nplanes, w, h, dec) || !part_map_ok(bsize, w, dec, bstride, planes_per_frame)) {
    return ODHIP_EINVAL;
  }
  const PartGeom g = part_geom(nplanes, w, h, dec);
  const PartMap m = {bsize, bsize_frame_stride, bstride, planes_per_frame, dec};
  for (int s = 0; s < ODHIP_NBSIZES; s++) {
    const int n = 4 << s;
    for (int p = 0; p < nplanes; p++) {
      int32_t c = 0;
      if (s < g.nsizes) {
        const int nbx = w/n;
        uint32_t *list = lists + g.list0[s] + (size_t)p*nbx*(h/n);
        for (int by = 0; by < h/n; by++) {
          for (int bx = 0; bx < nbx; bx++) {
            if (part_is_leaf(m, p, s, bx, by)) list[c++] = (uint32_t)by*nbx + bx;
          }
        }
      }
      count[s*nplanes + p] = c;
    }
  }
  return ODHIP_SUCCESS;
}

extern "C" int odhip_partition_leaves(uint32_t *d_lists, int32_t *count, int nplanes, int w, int h, int dec,
 const uint8_t *d_bsize, int bstride, long bsize_frame_stride, int planes_per_frame, odhip_stream stream) {
  if (!d_lists || !count || !part_planes_ok(nplanes, w, h, dec) || nplanes > 65535
   || !part_map_ok(d_bsize, w, dec, bstride, planes_per_frame)) {
    return ODHIP_EINVAL;
  }
  ODHIP_CTX_OR_RETURN(ctx);
  PartState *st = odhip_ctx_state<PartState>(ctx, ODHIP_SLOT_PARTITION);
  hipStream_t s = (hipStream_t)stream;
  PartRowsArgs a;
  a.m = {d_bsize, bsize_frame_stride, bstride, planes_per_frame, dec};
  a.g = part_geom(nplanes, w, h, dec);
  const int nrows = a.g.row0[ODHIP_NBSIZES];
  const size_t ncounts = (size_t)ODHIP_NBSIZES*nplanes;
  int rc = st->rows.grow((size_t)nplanes*nrows, s);
  if (!rc) rc = st->d_counts.grow(ncounts, s);
  if (!rc) rc = st->h_counts.grow(ncounts, s);
  if (rc) return rc;
  a.rows = st->rows.p;
  a.lists = d_lists;
  const dim3 grid((unsigned)nrows, (unsigned)nplanes);
  k_part_rows<false><<<grid, 64, 0, s>>>(a);
  k_part_scan<<<dim3((unsigned)a.g.nsizes, (unsigned)nplanes), 256, 0, s>>>(a.g, a.rows, st->d_counts.p);
  k_part_rows<true><<<grid, 64, 0, s>>>(a);
  rc = odhip_check_launch();
  if (rc) return rc;
  ODHIP_TRY(hipMemcpyAsync(st->h_counts.p, st->d_counts.p, (size_t)a.g.nsizes*nplanes*sizeof(int32_t),
   hipMemcpyDeviceToHost, s));
  ODHIP_TRY(hipStreamSynchronize(s));
  memset(count, 0, ncounts*sizeof(int32_t));
  memcpy(count, st->h_counts.p, (size_t)a.g.nsizes*nplanes*sizeof(int32_t));
  return ODHIP_SUCCESS;
}

extern "C" int odhip_partition_gather(od_coeff *d_dense, const od_coeff *d_src, int s, const uint32_t *d_list,
 const int32_t *count, int nplanes, int w, int h, int dec, odhip_stream stream) {
  return part_copy<false>(d_dense, d_src, s, d_list, count, nplanes, w, h, dec, stream);
}

extern "C" int odhip_partition_scatter(od_coeff *d_dst, const od_coeff *d_dense, int s, const uint32_t *d_list,
 const int32_t *count, int nplanes, int w, int h, int dec, odhip_stream stream) {
  return part_copy<true>(d_dst, d_dense, s, d_list, count, nplanes, w, h, dec, stream);
}

extern "C" int odhip_cfl_refs_partition_host(od_coeff *ref, const od_coeff *luma, int w, int h, int dec,
 const uint8_t *bsize, int bstride) {
  if (!cfl_part_ok(ref, luma, w, h, dec, bsize, bstride)) return ODHIP_EINVAL;
  const int side = 64 >> dec;
  const int cw = w >> dec;
  for (int sby = 0; sby < h/64; sby++) {
    for (int sbx = 0; sbx < w/64; sbx++) {
      const od_coeff *sb = luma + (size_t)sby*64*w + sbx*64;
      const uint8_t *sbmap = bsize + (size_t)sby*8*bstride + sbx*8;
      for (int cy = 0; cy < side; cy++) {
        for (int cx = 0; cx < side; cx += 4) {
          cfl_group(ref + (size_t)(sby*side + cy)*cw + sbx*side + cx, sb, w, sbmap, bstride, dec, cy, cx);
        }
      }
    }
  }
  return ODHIP_SUCCESS;
}

extern "C" int odhip_cfl_refs_partition(od_coeff *d_ref, const od_coeff *d_luma, int nplanes, int w, int h, int dec,
 const uint8_t *d_bsize, int bstride, long bsize_frame_stride, int planes_per_frame, odhip_stream stream) {
  if (!cfl_part_ok(d_ref, d_luma, w, h, dec, d_bsize, bstride) || nplanes < 1 || planes_per_frame < 1
   || (((uintptr_t)d_ref | (uintptr_t)d_luma) & 15)) {
    return ODHIP_EINVAL;
  }
  CflPartArgs a;
  memset(&a, 0, sizeof(a));
  a.ref = d_ref;
  a.luma = d_luma;
  a.bsize = d_bsize;
  a.frame_stride = bsize_frame_stride;
  a.bstride = bstride;
  a.w = w;
  a.h = h;
  a.dec = dec;
  a.planes_per_frame = planes_per_frame;
  const unsigned nsb = (unsigned)(w/64)*(unsigned)(h/64);
  for (int p0 = 0; p0 < nplanes; p0 += 65535) {
    const int np = nplanes - p0 < 65535 ? nplanes - p0 : 65535;
    a.plane0 = p0;
    k_cfl_part<<<dim3(nsb, (unsigned)np), kCflThreads, 0, (hipStream_t)stream>>>(a);
  }
  return odhip_check_launch();
}
