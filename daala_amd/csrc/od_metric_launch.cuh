/* od_metric_launch.cuh - what the tiled metrics (SSIM in metrics_kernels.hip, MS-SSIM, FastSSIM) launch alike: a call's
   pairs go out in launch groups (od_metric_groups.h); a group's tile kernel is a flat grid over (pair, column, tile) - a
   column is a scale of MS-SSIM, a level of FastSSIM, the one sum of SSIM - and leaves one partial per 32 x 32 tile.

   k_metric_tile_sum  one workgroup per (pair, column): lane i adds the tile partials i, i + 256, ... in order, then the
                      tile kernels' tree -> sums[pair][column].  The tools keep running doubles over a plane, which no
                      parallel order reproduces; this order is fixed, so a result repeats bit for bit.

   The pyramid metrics also share the group's planes - every reconstruction and every DISTINCT source plane, with the
   place of its pyramid in the scratch and its first workgroup in the pyramid grid - and the scratch itself, one per
   metric and context.  What differs comes in through a traits struct:
     kLevels, pyr_elems(w, h) and pyr_blocks(w, h) of a plane's pyramid, tiles(w, h, level). */
#pragma once
#include <string.h>
#include "od_buf.cuh"
#include "od_metric_groups.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBatch = 32;                            /* pairs of a launch group (kernel argument size) */
constexpr int kTile = 32;                             /* output tile: 32 x 32 */
constexpr int kMaxColumns = 5;
constexpr long kLaunchTiles = 1L << 22;               /* tiles of one launch group (a single larger run goes alone) */

/* A group's grids as int, for planes up to 65535 x 65535 (pair_ok).  No level is larger than its plane, so a (pair,
   column) has at most 2048 x 2048 = 2^22 tiles and a group of kBatch pairs at most 32 x 5 x 2^22 = 671 088 640, whatever
   kLaunchTiles lets through; the pyramid grid has one workgroup per kTile x kTile sums of a plane halved once, fewer
   than that plane's tiles, for at most 2 kBatch planes: below 64 x 2^22 = 2^28. */
constexpr long kMaxLevelTiles = (long)((65535 + kTile - 1)/kTile)*((65535 + kTile - 1)/kTile);
static_assert(kBatch*kMaxColumns*kMaxLevelTiles <= 0x7fffffffL && 2*kBatch*kMaxLevelTiles <= 0x7fffffffL,
 "the tile grid and the pyramid grid of a launch group are ints");

/* the entry e of a nondecreasing table with first[e] <= at < first[e + 1], n entries */
__device__ __forceinline__ int find_entry(const int *first, int n, int at) {
  int lo = 0;
  int hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (first[mid + 1] > at) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

struct MetricTiles {
  int first[kBatch*kMaxColumns + 1];                  /* first tile of (pair, column) in the grid */
  int out[kBatch];                                    /* the pair's index in the call: its row of the sums */
  int columns;
};

__global__ __launch_bounds__(kThreads) void k_metric_tile_sum(MetricTiles t, const double *part, double *out) {
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int e = (int)blockIdx.x;
  const int first = t.first[e];
  const int n = t.first[e + 1] - first;
  double s = 0;
  for (int i = tid; i < n; i += kThreads) s += part[first + i];
  red[tid] = s;
  __syncthreads();
  for (int k = kThreads/2; k > 0; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  if (tid == 0) out[(size_t)t.out[e/t.columns]*t.columns + e%t.columns] = red[0];
}

/* the sums of the group's m pairs from its tile partials */
inline void metric_tile_sum(const MetricTiles &t, int m, const double *part, double *d_sums, hipStream_t s) {
  k_metric_tile_sum<<<(unsigned)(m*t.columns), kThreads, 0, s>>>(t, part, d_sums);
}

struct MetricPlane {
  const void *base;
  int fmt, stride, w, h, depth;
  size_t pyr;                                         /* first element of its pyramid in the scratch */
};

struct MetricPyrBatch {
  MetricPlane pl[2*kBatch];
  int block0[2*kBatch + 1];                           /* first workgroup of plane i in the grid */
};

/* what a pyramid metric's tile kernel is told about the group, beside its own */
struct MetricGroup {
  MetricTiles t;
  size_t spyr[kBatch];                                /* the pyramids of pair i's source and reconstruction */
  size_t rpyr[kBatch];
  int n;
};

/* the scratch of one launch group, per metric and context (one call sequence in flight per context) */
struct MetricScratch {
  DeviceBuf<int32_t> pyr;          /* the pyramids of the group's distinct source planes and reconstructions */
  DeviceBuf<double> part;          /* tile partials */
};

struct MetricLaunch {
  MetricPyrBatch pb;
  MetricGroup g;
  int nplanes;
  int blocks;                      /* the pyramid grid */
  int tiles;                       /* the tile grid */
};

template <class T>
long metric_tiles_all(int w, int h) {
  long n = 0;
  for (int l = 0; l < T::kLevels; l++) n += T::tiles(w, h, l);
  return n;
}

/* One launch group: the pairs pairs[idx[0 .. m)], m <= kBatch, pairs of one source plane next to each other; their sums
   go to row idx[i].  only_level >= 0 (the test surface): the tiles of that level alone.  The scratch grows on `s`. */
template <class T>
int metric_launch_build(MetricLaunch *L, MetricScratch *st, const odhip_metrics_pair *pairs, const int *idx, int m,
 int only_level, hipStream_t s) {
  static_assert(T::kLevels <= kMaxColumns, "MetricTiles holds kMaxColumns columns");
  memset(L, 0, sizeof(*L));
  MetricGroup &g = L->g;
  size_t elems = 0;
  auto add_plane = [&](const void *base, int fmt, int stride, const odhip_metrics_pair &q) {
    L->pb.pl[L->nplanes] = MetricPlane{base, fmt, stride, q.w, q.h, q.depth, elems};
    L->pb.block0[L->nplanes++] = L->blocks;
    elems += T::pyr_elems(q.w, q.h);
    L->blocks += (int)T::pyr_blocks(q.w, q.h);
    return L->pb.pl[L->nplanes - 1].pyr;
  };
  for (int i = 0; i < m; i++) {
    const odhip_metrics_pair &q = pairs[idx[i]];
    g.t.out[i] = idx[i];
    g.spyr[i] = i > 0 && same_plane(q, pairs[idx[i - 1]]) ? g.spyr[i - 1] : add_plane(q.src, q.src_fmt, q.src_stride, q);
    g.rpyr[i] = add_plane(q.rec, q.rec_fmt, q.rec_stride, q);
    for (int l = 0; l < T::kLevels; l++) {
      g.t.first[i*T::kLevels + l] = L->tiles;
      if (only_level < 0 || l == only_level) L->tiles += (int)T::tiles(q.w, q.h, l);
    }
  }
  g.t.first[m*T::kLevels] = L->tiles;
  g.t.columns = T::kLevels;
  g.n = m;
  for (int i = L->nplanes; i <= 2*kBatch; i++) L->pb.block0[i] = L->blocks;
  const int rc = st->pyr.grow(elems, s);
  return rc ? rc : st->part.grow((size_t)L->tiles, s);
}

/* odhip_*_prepare: the scratch of a group of min(pairs, kBatch) pairs of w x h, no source shared */
template <class T>
int metric_prepare(MetricScratch *st, int w, int h, int pairs) {
  const size_t m = (size_t)std::min(pairs, kBatch);
  const int rc = st->pyr.reserve(2*m*T::pyr_elems(w, h));
  return rc ? rc : st->part.reserve(m*(size_t)metric_tiles_all<T>(w, h));
}

/* odhip_*_planes of a pyramid metric, its pairs checked: launch(idx, m) once per group, in order */
template <class T, class Launch>
int metric_planes(const odhip_metrics_pair *pairs, int n, Launch launch) {
  /* pairs of one source plane next to each other: a group builds that plane's pyramid once */
  const MetricGroups g = metric_groups(pairs, n, [](const odhip_metrics_pair &q) { return metric_tiles_all<T>(q.w, q.h); },
   kBatch, kLaunchTiles, true);
  for (int k = 0; k < g.count(); k++) {
    const int rc = launch(g.idx.data() + g.first[k], g.first[k + 1] - g.first[k]);
    if (rc) return rc;
  }
  return ODHIP_SUCCESS;
}

}  // namespace
