/* mc_kernels.hip - overlapped-block motion compensation from motion-vector grids.

   The prediction the reference builds with od_state_mc_predict (src/state.c:932-959), given the vectors:
   every leaf of the grid's quadtree (mc_walk.cuh) is the blend of up to four predictions, one per corner,
   each a separable 6-tap interpolation at 1/8 pel of a reference plane (src/mc.c:94-340), weighted
   bilinearly - with the weights of od_mc_setup_s_split where a neighbour leaf is larger (src/mc.c:352-404,
   1056-1200).  Integer only; every intermediate has the reference's width (the 8-bit variant keeps its
   first pass in int16, the full-precision one in int32).

   Two kernels:
     k_mc_classify        one lane per 8x8 cell: is it the upper-left cell of a leaf, which size, outside
                          corner and split flags; descriptors appended to one bucket per leaf size
     k_mc_predict<T, TS>  one 256-lane block per 16x16 tile of a large leaf, or per 4 / 16 whole leaves of
                          the two small sizes; per corner the (TS + 5)^2 source window is staged in LDS with
                          clamped coordinates (= the reference's replicated border), both filter passes run
                          from LDS, the blend runs in registers.  Corners with the same slot and vector are
                          filtered once.
   Reference planes are UNPADDED coded-size planes.  A vector that would take a read outside the
   reference's 64-sample border is refused on the host (ODHIP_ERANGE) before anything is launched. */
#include <algorithm>
#include <vector>
#include "../../include/daala_hip.h"
#include "od_buf.cuh"
#include "od_ctx.cuh"
#include "mc_walk.cuh"
#include "mc_filter.cuh"

namespace {

constexpr int kThreads = 256;

struct McArgs {
  const void *ref[3];
  void *dst;
  const odhip_mv_point *grid;    /* [npics][nv + 1][nh + 1] */
  const uint32_t *leaves;        /* [npics][cap]: bucket of size lg at lvl_off(lg) */
  const int *counts;             /* [npics][4] */
  long long ref_plane_stride;
  long long dst_plane_stride;
  int ref_stride;
  int dst_stride;
  int nh;
  int nv;
  int dec;
  int w;                         /* the plane: coded size >> dec */
  int h;
  int npics;
  int nrefs;
  int cap;
  int lg;                        /* the leaf size this launch predicts */
  int lvl_off;
};

__host__ __device__ inline int lvl_off(int n, int lg) {
  int off = 0;
  for (int l = 0; l < lg; l++) off += n >> (2*l);
  return off;
}

__global__ __launch_bounds__(kThreads) void k_mc_classify(const odhip_mv_point *grid, int nh, int nv, int cap,
 uint32_t *leaves, int *counts) {
  const int cell = blockIdx.x*kThreads + threadIdx.x;
  const int pic = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const odhip_mv_point *g = grid + (size_t)pic*(nh + 1)*(nv + 1);
  auto valid = [&](int x, int y) { return g[y*(nh + 1) + x].valid != 0; };
  uint32_t desc = 0;
  int lg = -1;
  if (cell < nh*nv && od_mc_leaf_at(valid, cell%nh, cell/nh, &desc)) lg = OD_MC_LEAF_LOG(desc);
  /* one atomic per wavefront and size, not per leaf: a picture's leaves of one size share one counter */
  for (int l = 0; l <= OD_MC_LOG_MVB_MAX; l++) {
    const unsigned long long mine = __ballot(lg == l);
    if (!mine) continue;
    const int leader = __ffsll((long long)mine) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&counts[pic*4 + l], __popcll(mine));
    base = __shfl(base, leader);
    if (lg == l) {
      leaves[(size_t)pic*cap + lvl_off(nh*nv, l) + base + __popcll(mine & ((1ull << lane) - 1))] = desc;
    }
  }
}

/* One corner's bilinear weight at (i, j), times 2 << 2*lb (sh = 0) or half of that (sh = 1): corner 0 starts
   with all the weight, the weight moves to corner 1 along i, to corner 3 along j and to corner 2 along both. */
__device__ inline int corner_weight(int n, int sh, int lb, int i, int j) {
  const int s0 = n == 0 ? 2 << 2*lb : 0;
  const int di = n == 0 ? -(2 << lb) : n == 1 ? 2 << lb : 0;
  const int dj = n == 0 ? -(2 << lb) : n == 3 ? 2 << lb : 0;
  const int dd = (n & 1) ? -2 : 2;
  return (s0 >> sh) + (dj >> sh)*j + ((di >> sh) + (dd >> sh)*j)*i;
}

/* The blend weight of corner k at (i, j) of a leaf with outside corner oc whose neighbour across the edge
   towards corner (oc + 1) & 3 / (oc + 3) & 3 is larger where s lacks bit 0 / bit 1: that corner keeps half
   its weight and the outside corner takes the other half - the closed form of the reference's running sums
   (every halved term is even, so the halves are exact). */
__device__ inline int split_weight(int k, int oc, int s, int lb, int i, int j) {
  const int n1 = (oc + 1) & 3;
  const int n3 = (oc + 3) & 3;
  const bool h1 = !(s & 1);
  const bool h3 = !(s & 2);
  int w = corner_weight(k, (h1 && k == n1) || (h3 && k == n3), lb, i, j);
  if (k == oc) w += (h1 ? corner_weight(n1, 1, lb, i, j) : 0) + (h3 ? corner_weight(n3, 1, lb, i, j) : 0);
  return w;
}

template <class T, int TS>
__global__ __launch_bounds__(kThreads) void k_mc_predict(McArgs a) {
  typedef typename McTraits<T>::mid_t mid_t;
  constexpr int kLanes = TS*TS;            /* lanes of one tile */
  constexpr int kGroups = kThreads/kLanes; /* tiles of one block */
  constexpr int WS = TS + kApron;
  __shared__ T win[kGroups][WS*WS];
  __shared__ mid_t mid[kGroups][WS*TS];
  const int plane = blockIdx.y;
  const int pic = plane%a.npics;
  const int grp = threadIdx.x/kLanes;
  const int lt = threadIdx.x%kLanes;
  const int i = lt%TS;
  const int j = lt/TS;
  const int lb = a.lg + 3 - a.dec;         /* log2 of the leaf in samples of this plane */
  const int ltiles = lb > 4 ? lb - 4 : 0;  /* log2 of the tiles across a leaf */
  const int count = a.counts[pic*4 + a.lg];
  const long long nwork = (long long)count << 2*ltiles;
  const uint32_t *leaves = a.leaves + (size_t)pic*a.cap + a.lvl_off;
  const odhip_mv_point *grid = a.grid + (size_t)pic*(a.nh + 1)*(a.nv + 1);
  T *dst = (T *)a.dst + plane*a.dst_plane_stride;
  for (long long unit = blockIdx.x; unit*kGroups < nwork; unit += gridDim.x) {
    const long long work = unit*kGroups + grp;
    const bool active = work < nwork;
    int mvx[4] = {0, 0, 0, 0};
    int mvy[4] = {0, 0, 0, 0};
    int slot[4] = {0, 0, 0, 0};
    int oc = 0;
    int s = 3;
    int bx = 0;
    int by = 0;
    int ti = i;                            /* this lane's sample inside the leaf */
    int tj = j;
    if (active) {
      const uint32_t d = leaves[work >> 2*ltiles];
      const int tile = (int)(work & ((1 << 2*ltiles) - 1));
      oc = OD_MC_LEAF_OC(d);
      s = OD_MC_LEAF_S(d);
      const int vx = OD_MC_LEAF_VX(d);
      const int vy = OD_MC_LEAF_VY(d);
      bx = vx << (3 - a.dec);
      by = vy << (3 - a.dec);
      ti += (tile & ((1 << ltiles) - 1))*TS;
      tj += (tile >> ltiles)*TS;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        int dx;
        int dy;
        od_mc_vertex(oc, s, k, &dx, &dy);
        const odhip_mv_point pt = grid[(vy + (dy << a.lg))*(a.nh + 1) + vx + (dx << a.lg)];
        mvx[k] = od_mc_scale_mv(pt.mvx, a.dec);
        mvy[k] = od_mc_scale_mv(pt.mvy, a.dec);
        slot[k] = min((int)pt.ref, a.nrefs - 1);   /* a device grid is not validated */
      }
    }
    int pred[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      int same = -1;
#pragma unroll
      for (int e = k - 1; e >= 0; e--) {
        if (mvx[e] == mvx[k] && mvy[e] == mvy[k] && slot[e] == slot[k]) same = e;
      }
      const bool need = active && same < 0;
      const int fxi = mvx[k] & 7;
      const int fyi = mvy[k] & 7;
      __syncthreads();                     /* the previous corner's passes have read win / mid */
      if (need) {
        const T *src = (const T *)a.ref[slot[k]] + plane*a.ref_plane_stride;
        const int x0 = bx + ti - i + (mvx[k] >> 3) - kTop;
        const int y0 = by + tj - j + (mvy[k] >> 3) - kTop;
        for (int e = lt; e < WS*WS; e += kLanes) {
          const int x = min(max(x0 + e%WS, 0), a.w - 1);
          const int y = min(max(y0 + e/WS, 0), a.h - 1);
          win[grp][e] = src[(size_t)y*a.ref_stride + x];
        }
      }
      __syncthreads();
      if (need && (fxi | fyi)) {
        for (int e = lt; e < WS*TS; e += kLanes) {
          mid[grp][e] = (mid_t)mc_hpass<T>(&win[grp][(e/TS)*WS + e%TS], fxi);
        }
      }
      __syncthreads();
      if (need) {
        if (!(fxi | fyi)) pred[k] = win[grp][(j + kTop)*WS + i + kTop];
        else pred[k] = mc_vpass<T>(&mid[grp][j*TS + i], TS, fyi);
      }
      else {
        pred[k] = 0;
#pragma unroll
        for (int e = 0; e < k; e++) {
          if (same == e) pred[k] = pred[e];
        }
      }
    }
    if (active) {
      int out;
      if (s == 3) {
        const int p = pred[0]*(1 << lb) + (pred[1] - pred[0])*ti;
        const int q = pred[3]*(1 << lb) + (pred[2] - pred[3])*ti;
        out = (p*(1 << lb) + (q - p)*tj + (1 << (2*lb - 1))) >> 2*lb;
      }
      else {
        const int p = pred[0];
        out = (p*(1 << (2*lb + 1)) + (pred[1] - p)*split_weight(1, oc, s, lb, ti, tj)
         + (pred[2] - p)*split_weight(2, oc, s, lb, ti, tj) + (pred[3] - p)*split_weight(3, oc, s, lb, ti, tj)
         + (1 << 2*lb)) >> (2*lb + 1);
      }
      dst[(size_t)(by + tj)*a.dst_stride + bx + ti] = (T)out;
    }
  }
}

/* grid copy, leaf buckets and their counters of one call sequence, per context */
struct McState {
  DeviceBuf<odhip_mv_point> grid;
  DeviceBuf<uint32_t> leaves;
  DeviceBuf<int> counts;      /* 4 per picture */
  int reserve(size_t points, size_t nleaves, int npics, bool want_grid) {
    int rc = want_grid ? grid.reserve(points) : ODHIP_SUCCESS;
    if (!rc) rc = leaves.reserve(nleaves);
    if (!rc) rc = counts.reserve((size_t)4*npics);
    return rc;
  }
};

int leaf_cap_of(int nh, int nv) { return lvl_off(nh*nv, 4); }

/* the walk on the host: every leaf's corners point into a given slot, and no filter window leaves the
   border the reference replicates round its frames */
int check_grid(const odhip_mv_point *grid, int nh, int nv, int npics, int dec, int nrefs) {
  for (int pic = 0; pic < npics; pic++) {
    const odhip_mv_point *g = grid + (size_t)pic*(nh + 1)*(nv + 1);
    auto valid = [&](int x, int y) { return g[y*(nh + 1) + x].valid != 0; };
    for (int vy = 0; vy < nv; vy++) {
      for (int vx = 0; vx < nh; vx++) {
        uint32_t d;
        if (!od_mc_leaf_at(valid, vx, vy, &d)) continue;
        const int lg = OD_MC_LEAF_LOG(d);
        for (int k = 0; k < 4; k++) {
          int dx;
          int dy;
          od_mc_vertex(OD_MC_LEAF_OC(d), OD_MC_LEAF_S(d), k, &dx, &dy);
          const int px = vx + dx*(1 << lg);
          const int py = vy + dy*(1 << lg);
          if (px < 0 || px > nh || py < 0 || py > nv) return ODHIP_EINVAL;
          const odhip_mv_point &pt = g[py*(nh + 1) + px];
          if (pt.ref >= nrefs) return ODHIP_EINVAL;
          if (!od_mc_window_ok(vx, pt.mvx, lg, dec, nh) || !od_mc_window_ok(vy, pt.mvy, lg, dec, nv)) {
            return ODHIP_ERANGE;
          }
        }
      }
    }
  }
  return ODHIP_SUCCESS;
}

bool vector_ok(const odhip_mv_point &pt) {
  return pt.mvx > -(1 << 20) && pt.mvx < (1 << 20) && pt.mvy > -(1 << 20) && pt.mvy < (1 << 20);
}

int classify(McState *st, const odhip_mv_point *d_grid, int nh, int nv, int npics, hipStream_t s) {
  ODHIP_TRY(hipMemsetAsync(st->counts.p, 0, sizeof(int)*4*npics, s));
  k_mc_classify<<<dim3((unsigned)((nh*nv + kThreads - 1)/kThreads), (unsigned)npics), kThreads, 0, s>>>(d_grid,
   nh, nv, leaf_cap_of(nh, nv), st->leaves.p, st->counts.p);
  return odhip_check_launch();
}

template <class T>
void launch_predict(const McArgs &a, int nplanes, hipStream_t s) {
  const int lb = a.lg + 3 - a.dec;
  const int n = (a.nh*a.nv) >> 2*a.lg;     /* the most leaves of this size */
  long long units;
  if (lb >= 4) units = (long long)n << 2*(lb - 4);
  else units = ((long long)n + (kThreads >> 2*lb) - 1)/(kThreads >> 2*lb);
  const unsigned gx = (unsigned)std::min<long long>(units, 4096);
  const dim3 g(gx, (unsigned)nplanes);
  if (lb >= 4) k_mc_predict<T, 16><<<g, kThreads, 0, s>>>(a);
  else if (lb == 3) k_mc_predict<T, 8><<<g, kThreads, 0, s>>>(a);
  else k_mc_predict<T, 4><<<g, kThreads, 0, s>>>(a);
}

}  // namespace

extern "C" size_t odhip_mc_sizeof(int what) {
  return what == 0 ? sizeof(odhip_mv_point) : what == 1 ? sizeof(odhip_mc_job) : 0;
}

extern "C" int odhip_mc_check_grid(const odhip_mv_point *grid, int coded_w, int coded_h, int npics, int dec,
 int nrefs) {
  if (!grid || !od_mc_size_ok(coded_w, coded_h) || npics < 1 || dec < 0 || dec > 1 || nrefs < 1 || nrefs > 3) {
    return ODHIP_EINVAL;
  }
  const int nh = coded_w >> 3;
  const int nv = coded_h >> 3;
  const size_t points = (size_t)npics*(nh + 1)*(nv + 1);
  for (size_t e = 0; e < points; e++) {
    if (!vector_ok(grid[e])) return ODHIP_ERANGE;
  }
  return check_grid(grid, nh, nv, npics, dec, nrefs);
}

extern "C" int odhip_mc_prepare(int coded_w, int coded_h, int npics) {
  if (!od_mc_size_ok(coded_w, coded_h) || npics < 1) return ODHIP_EINVAL;
  ODHIP_CTX_OR_RETURN(ctx);
  McState *st = odhip_ctx_state<McState>(ctx, ODHIP_SLOT_MC);
  const int nh = coded_w >> 3;
  const int nv = coded_h >> 3;
  return st->reserve((size_t)npics*(nh + 1)*(nv + 1), (size_t)npics*leaf_cap_of(nh, nv), npics, true);
}

extern "C" int odhip_mc_predict_planes(const odhip_mc_job *job, odhip_stream stream) {
  if (!job || !job->grid || !job->dst || !od_mc_size_ok(job->coded_w, job->coded_h) || job->dec < 0 || job->dec > 1
   || job->npics < 1 || job->nplanes < job->npics || job->nplanes%job->npics || job->nplanes > 65535
   || job->nrefs < 1 || job->nrefs > 3
   || (job->sample != ODHIP_SAMPLE_U8 && job->sample != ODHIP_SAMPLE_I16_12)) {
    return ODHIP_EINVAL;
  }
  const int w = job->coded_w >> job->dec;
  const int h = job->coded_h >> job->dec;
  if (job->ref_stride < w || job->dst_stride < w || job->ref_plane_stride < (int64_t)job->ref_stride*h
   || job->dst_plane_stride < (int64_t)job->dst_stride*h) {
    return ODHIP_EINVAL;
  }
  for (int r = 0; r < job->nrefs; r++) {
    if (!job->ref[r]) return ODHIP_EINVAL;
  }
  const int nh = job->coded_w >> 3;
  const int nv = job->coded_h >> 3;
  if (!job->grid_on_device) {
    const int rc = odhip_mc_check_grid(job->grid, job->coded_w, job->coded_h, job->npics, job->dec, job->nrefs);
    if (rc) return rc;
  }
  ODHIP_CTX_OR_RETURN(ctx);
  McState *st = odhip_ctx_state<McState>(ctx, ODHIP_SLOT_MC);
  hipStream_t s = (hipStream_t)stream;
  const size_t points = (size_t)job->npics*(nh + 1)*(nv + 1);
  const int cap = leaf_cap_of(nh, nv);
  int rc = st->reserve(points, (size_t)job->npics*cap, job->npics, !job->grid_on_device);
  if (rc) return rc;
  const odhip_mv_point *d_grid = job->grid;
  if (!job->grid_on_device) {
    ODHIP_TRY(hipMemcpyAsync(st->grid.p, job->grid, points*sizeof(odhip_mv_point), hipMemcpyHostToDevice, s));
    d_grid = st->grid.p;
  }
  rc = classify(st, d_grid, nh, nv, job->npics, s);
  if (rc) return rc;
  McArgs a;
  for (int r = 0; r < 3; r++) a.ref[r] = r < job->nrefs ? job->ref[r] : nullptr;
  a.dst = job->dst;
  a.grid = d_grid;
  a.leaves = st->leaves.p;
  a.counts = st->counts.p;
  a.ref_plane_stride = job->ref_plane_stride;
  a.dst_plane_stride = job->dst_plane_stride;
  a.ref_stride = job->ref_stride;
  a.dst_stride = job->dst_stride;
  a.nh = nh;
  a.nv = nv;
  a.dec = job->dec;
  a.w = w;
  a.h = h;
  a.npics = job->npics;
  a.nrefs = job->nrefs;
  a.cap = cap;
  for (int lg = OD_MC_LOG_MVB_MAX; lg >= 0; lg--) {
    a.lg = lg;
    a.lvl_off = lvl_off(nh*nv, lg);
    if (job->sample == ODHIP_SAMPLE_U8) launch_predict<uint8_t>(a, job->nplanes, s);
    else launch_predict<int16_t>(a, job->nplanes, s);
  }
  return odhip_check_launch();
}

extern "C" int odhip_mc_leaves(const odhip_mv_point *grid, int coded_w, int coded_h, int npics, uint32_t *out,
 int *counts, int cap) {
  if (!grid || !out || !counts || !od_mc_size_ok(coded_w, coded_h) || npics < 1 || cap < 1) return ODHIP_EINVAL;
  const int nh = coded_w >> 3;
  const int nv = coded_h >> 3;
  ODHIP_CTX_OR_RETURN(ctx);
  McState *st = odhip_ctx_state<McState>(ctx, ODHIP_SLOT_MC);
  const size_t points = (size_t)npics*(nh + 1)*(nv + 1);
  const int lcap = leaf_cap_of(nh, nv);
  int rc = st->reserve(points, (size_t)npics*lcap, npics, true);
  if (rc) return rc;
  ODHIP_TRY(hipMemcpy(st->grid.p, grid, points*sizeof(odhip_mv_point), hipMemcpyHostToDevice));
  rc = classify(st, st->grid.p, nh, nv, npics, nullptr);
  if (rc) return rc;
  std::vector<uint32_t> all((size_t)npics*lcap);
  std::vector<int> per((size_t)npics*4);
  ODHIP_TRY(hipMemcpy(all.data(), st->leaves.p, all.size()*sizeof(uint32_t), hipMemcpyDeviceToHost));
  ODHIP_TRY(hipMemcpy(per.data(), st->counts.p, per.size()*sizeof(int), hipMemcpyDeviceToHost));
  for (int pic = 0; pic < npics; pic++) {
    std::vector<uint32_t> got;
    for (int lg = 0; lg < 4; lg++) {
      const uint32_t *b = all.data() + (size_t)pic*lcap + lvl_off(nh*nv, lg);
      got.insert(got.end(), b, b + per[pic*4 + lg]);
    }
    std::sort(got.begin(), got.end());
    counts[pic] = (int)got.size();
    if ((int)got.size() > cap) return ODHIP_EINVAL;
    std::copy(got.begin(), got.end(), out + (size_t)pic*cap);
  }
  return ODHIP_SUCCESS;
}
