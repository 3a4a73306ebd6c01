/* od_metric_groups.h - how a call of a tiled metric (SSIM, MS-SSIM, FastSSIM) is cut into launch groups.  Host code
   only and nothing of HIP, so that tests/test_metric_groups_host.py compiles it with the host compiler.

   A launch group is what one set of kernel arguments describes: at most `max_pairs` pairs and, unless a single run is
   larger, at most `max_tiles` tiles.  A pyramid metric builds the pyramid of a source plane once per group, so its pairs
   are put in a stable order by source plane, and a RUN - up to max_pairs neighbouring pairs of one source plane - joins
   a group whole. */
#pragma once
#include <algorithm>
#include <functional>
#include <vector>
#include "../../include/daala_hip.h"

namespace {

inline bool same_plane(const odhip_metrics_pair &a, const odhip_metrics_pair &b) {
  return a.src == b.src && a.src_fmt == b.src_fmt && a.src_stride == b.src_stride && a.w == b.w && a.h == b.h
   && a.depth == b.depth;
}

inline bool plane_before(const odhip_metrics_pair &a, const odhip_metrics_pair &b) {
  if (a.src != b.src) return std::less<const void *>()(a.src, b.src);
  if (a.src_fmt != b.src_fmt) return a.src_fmt < b.src_fmt;
  if (a.src_stride != b.src_stride) return a.src_stride < b.src_stride;
  if (a.w != b.w) return a.w < b.w;
  if (a.h != b.h) return a.h < b.h;
  return a.depth < b.depth;
}

struct MetricGroups {
  std::vector<int> idx;            /* the pairs in launch order */
  std::vector<int> first;          /* group g is pairs[idx[first[g] .. first[g + 1])] */
  int count() const { return (int)first.size() - 1; }
};

/* tiles_of(pair): the tiles of one pair.  by_plane: order the pairs by plane_before and keep runs whole; otherwise the
   order is the call's and every pair is a run of its own.  A group is closed when the next run would exceed either
   cap; the first run of a group always goes in, even alone above max_tiles. */
template <class Tiles>
MetricGroups metric_groups(const odhip_metrics_pair *pairs, int n, Tiles tiles_of, int max_pairs, long max_tiles,
 bool by_plane) {
  MetricGroups g;
  g.idx.resize((size_t)n);
  for (int i = 0; i < n; i++) g.idx[i] = i;
  if (by_plane) {
    std::stable_sort(g.idx.begin(), g.idx.end(), [&](int a, int b) { return plane_before(pairs[a], pairs[b]); });
  }
  g.first.push_back(0);
  int first = 0;
  while (first < n) {
    int m = 0;
    long tiles = 0;
    while (first + m < n && m < max_pairs) {
      const odhip_metrics_pair &q = pairs[g.idx[first + m]];
      int run = 1;
      while (by_plane && run < max_pairs && first + m + run < n && same_plane(q, pairs[g.idx[first + m + run]])) run++;
      const long t = run*(long)tiles_of(q);
      if (m > 0 && (m + run > max_pairs || tiles + t > max_tiles)) break;
      tiles += t;
      m += run;
    }
    first += m;
    g.first.push_back(first);
  }
  return g;
}

}  // namespace
