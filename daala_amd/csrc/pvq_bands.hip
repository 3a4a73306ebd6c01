/* pvq_bands.hip - the PVQ band stage on gfx950: everything in pvq_theta's
   no-reference keyframe path (reference src/pvq_encoder.c:333-641) that does
   not depend on the adaptive entropy coder, for every block of every level of
   a batch of coefficient planes, plus the choice/dequantisation that follows.

   MULTI-JOB launches.  One (plane set, block size) pair is a "job"; a frame
   batch has nine (5 luma + 4 chroma levels).  Every kernel takes a table of
   (job, band) work items with a prefix sum of workgroup counts and covers ALL
   jobs in one launch, so small levels overlap with large ones.

   Two generations of kernels share the parts below (the candidate walk and
   the pulse packer, the record head, the 1/sqrt table in LDS):

   DECIDED IN PLACE, the frame step (odhip_pvq_noref_bands_priced_multi).  The
   lanes that load a band scale it, search both gain candidates in their LDS
   columns, make the priced choice and write the choice and the pulses that
   are read: no scaled vectors, records, sort keys or sorted order in memory.

     k_decide_corner<0 / 1>        band 0 of every block (15 coefficients) /
                                   bands 1, 2 of blocks of 8x8 and up (8
                                   each), one block per lane
     k_decide_lane32               the 32-coefficient bands, a lane pair per
     k_decide_pair128              band / the 128-coefficient bands likewise
                                   (od_decide_group; k_decide_quad128, a lane
                                   quad, in the experiments build)
     k_choose_list                 the close calls again, with the host's
                                   rates (odhip_pvq_choose_priced_resolve)

   SORTED TWO-PASS STAGE: odhip_pvq_noref_bands_multi, the frame cache and the
   exporting hosts, which keep every record and both candidates' pulses.  The
   cost of a band is its pulse count, which spans 1..350 within one level,
   and a wavefront runs as long as its slowest lane.  So:

     k_prep_corner / k_prep_lane   QM scaling to x16 (library scratch), gain, the
       / k_prep_wide               two candidates' K and pruning decision
                                   (first half of the band record), and a SORT
                                   KEY = binned (pulses of candidate 0, extra
                                   pulses of candidate 1)
     k_sort_hist / _prefix /       counting sort of the block indices of each
       _scatter                    (job, band) item by key, heavy first
                                   (od_band_stage.cuh)
     k_search<N, S>                one band per lane (or lane pair) over the
                                   sorted order: the bands of a wavefront need
                                   (almost) the same number of pulses (pvq_lane.cuh)
     k_choose                      per band: `cost <= best_cost` choice,
                                   od_gain_expand, synthesis scale
                                   (src/pvq.c:766, :1057-1078)
     k_synth                       per coefficient: y*scale, inverse QM,
                                   scan -> raster (src/pvq.c:1081-1092,
                                   src/partition.c:176-194)

   Memory: every global access of the hot kernels is a whole 16-byte vector per
   lane and every record half a whole 32-byte sector (odhip_pvq_band in
   include/daala_hip.h): the earlier structure-of-arrays layout with 2..8-byte
   scattered stores wrote 3x the bytes (rocprofv3 WRITE_SIZE). */
#include "../../include/daala_hip.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "od_ctx.cuh"
#include "od_pvq_math.cuh"
#include "od_pvq_synth.cuh"
#include "od_occupancy.cuh"
#include "od_krange.cuh"
#include "od_band_stage.cuh"
#include "od_cfl.cuh"
#include "gen/od_scan_tables.h"
#define OD_RSQ_HUGE
#include "pvq_search.cuh"
#include "pvq_lane.cuh"

namespace {

constexpr int kMaxJobs = 16;
constexpr int kMaxItems = kMaxJobs*ODHIP_MAX_BANDS;

struct DJob {
  const od_coeff *coef;
  const int16_t *qm;
  const int16_t *qm_inv;
  odhip_pvq_band *rec;
  int16_t *y;
  int32_t *choice;
  double *cos_dist;
  od_coeff *dq;
  const double *rate;
  int32_t *qg_out;
  /* library scratch of the sorted band stage */
  int16_t *x16;            /* [B][len]  QM-scaled band vectors, coding order      */
  unsigned short *keys;    /* [nb][B]   sort key (pulse-count class)              */
  unsigned *ids;           /* [nb][B]   block indices sorted by key               */
  unsigned *krange;        /* od_krange.cuh: the calling context's counter        */
  long nblocks;
  int nplanes;
  int w;
  int h;
  int bs;
  int nb_bands;
  int len;
  int bw;
  int bh;
  int q[ODHIP_MAX_BANDS];
  int beta[ODHIP_MAX_BANDS];
  int off[ODHIP_MAX_BANDS + 1];
  /* planes from plane_split on (blocks from split_blk on) take q2: the Cr half of a
     chroma plane set - pvq_qm_q4[pli] is per plane, src/encode.c:3052-3072 */
  long split_blk;
  int q2[ODHIP_MAX_BANDS];
  /* odhip_pvq_job.d_q_plane: every plane its own row of band steps (plane_blocks blocks per
     plane); q and q2 are then 0 (a step is at least 1), so that the lookup costs the kernels
     nothing but a compare while they are NULL */
  const int *qp;
  unsigned plane_blocks;
};

/* The step of band `band` of block blk: the Cb / Cr split, or the row of its plane. */
__device__ __forceinline__ int plane_q(const DJob &jb, int band, long blk) {
  return jb.qp[(unsigned)blk/jb.plane_blocks*ODHIP_MAX_BANDS + band];
}
__device__ __forceinline__ int band_q(const DJob &jb, int band, long blk) {
  const int q = blk >= jb.split_blk ? jb.q2[band] : jb.q[band];
  return q ? q : plane_q(jb, band, blk);
}

/* A band whose priced choice the host (re)decides: candidate rates from the host libm. */
struct PUnc {
  int job;
  unsigned sb;             /* blk*nb_bands + band */
  double rate[2];
};
constexpr int kPUncCap = 1 << 16;

struct Items : ItemTable<kMaxItems> {
  int force_seq;           /* pair-mode search: always take the sequential combine */
  double lambda;
  const DJob *jobs;        /* the calling context's device job table [kMaxJobs]   */
  unsigned *pcount;        /* priced choice: bands too close to call on the device; pcount[1]: bands with a
                              candidate above ODHIP_PVQ_MAX_K (od_krange.cuh), cleared only when taken */
  struct PUnc *plist;      /* ... and their list [kPUncCap]                       */
  double tol_scale;        /* test hook: multiplies the decision margin           */
};

/* Scan tables.  kScanXY is indexed wave-uniformly by the one-band-per-lane
   preparation kernel (scalar loads); the kernels that index per lane copy
   their table into LDS first - a constant-memory access with 64 different
   addresses serialises. */
__constant__ unsigned char kScanXY[OD_SCAN_LEN][2];
/* Round 5, the staged load (LoadStaged) of k_decide_pair128.  A 128-coefficient band (coding positions 128..255, 256..383 or
   384..511) covers a region of its block that consists of 32 aligned 4-coefficient row segments: kSeg128[g][q] =
   y << 8 | x of segment q of geometry g = off/128 - 1, in raster order; kSlot128[g][p] = where coding position
   off + p sits in that staged order (segment*4 + element). */
__constant__ unsigned short kSeg128[3][32];
__constant__ unsigned char kSlot128[3][128];
/* ... and the 32-coefficient bands (coding positions 32..63, 64..95, 96..127; k_decide_lane32): 16 aligned
   2-coefficient segments (band 3 of an 8x8 block starts at x = 2 in its rows 4..7), geometry off/32 - 1. */
__constant__ unsigned short kSeg32[3][16];
__constant__ unsigned char kSlot32[3][32];
__device__ __attribute__((aligned(16))) unsigned short gScanXY[OD_SCAN_LEN];  /* y << 8 | x */
__device__ short gInvScan[32*32];                /* raster (y*32 + x) -> coding index, -1 */
__device__ unsigned char gBandOf[OD_SCAN_LEN];

struct BlockPos {
  const od_coeff *src;
  long blk;
  bool live;
};

__device__ __forceinline__ BlockPos locate(const DJob &j, long blk) {
  BlockPos r;
  r.live = blk < j.nblocks;
  r.blk = blk;
  const long b = r.live ? blk : j.nblocks - 1;
  const int N = 4 << j.bs;
  const long per = (long)j.bw*j.bh;
  const int p = (int)(b/per);
  const int rem = (int)(b - p*per);
  const int by = rem/j.bw;
  const int bx = rem - by*j.bw;
  r.src = j.coef + (long)p*j.w*j.h + (long)by*N*j.w + bx*N;
  return r;
}

/* The sort key of a band (od_band_stage.cuh sorts by it, heavy first): one wavefront of 128-coefficient bands with
   K = 90 runs for ~250 us, as long as the rest of its launch. */
constexpr int kKeyBins = 1024;
constexpr int kSortChunk = 4096;

__device__ __forceinline__ int od_pulse_bin(int p) {   /* 0..63, monotone */
  if (p < 24) return p;
  if (p < 32) return 24 + ((p - 24) >> 1);
  if (p < 64) return 28 + ((p - 32) >> 2);
  if (p < 128) return 36 + ((p - 64) >> 3);
  if (p < 256) return 44 + ((p - 128) >> 4);
  if (p < 512) return 52 + ((p - 256) >> 5);
  const int t = (p - 512) >> 7;
  return 60 + (t < 3 ? t : 3);
}

__device__ __forceinline__ int od_extra_bin(int p) {   /* 0..15, monotone */
  if (p < 12) return p;
  if (p < 16) return 12;
  if (p < 24) return 13;
  if (p < 48) return 14;
  return 15;
}

/* First half of a band record as the two 16-byte vectors it is stored in. */
struct RecHead {
  int32_t cg;
  int32_t gain[2];
  int k[2];
  int flags[2];
};

__device__ __forceinline__ RecHead rec_head(int4 a, int4 b) {
  RecHead h;
  h.cg = a.x;
  h.gain[0] = a.y;
  h.gain[1] = a.z;
  h.k[0] = (int16_t)(a.w & 0xffff);
  h.k[1] = a.w >> 16;
  h.flags[0] = b.x & 0xff;
  h.flags[1] = b.x >> 8 & 0xff;
  return h;
}

__device__ __forceinline__ RecHead rec_head_load(const odhip_pvq_band *r) {
  return rec_head(reinterpret_cast<const int4 *>(r)[0], reinterpret_cast<const int4 *>(r)[1]);
}

/* Everything the preparation kernels need of a job, read ONCE at the top of the
   kernel: g_jobs is global memory that the kernels' own stores might alias as
   far as the compiler knows, so a field read after a store is reloaded with an
   exposed memory latency (five serialised reloads per band before this). */
struct PrepCtx {
  const int16_t *qm;       /* + off */
  int16_t *x16;            /* + off - pad */
  odhip_pvq_band *rec;     /* + band */
  unsigned short *keys;    /* + band*nblocks */
  int w;
  int len;
  int nb_bands;
  int q;
  int q2;
  long split_blk;
  int beta;
  unsigned *krange;        /* od_krange.cuh: the context's counter (Items::pcount + 1) */
};

/* The band's quantiser step for block blk (0: the row of its plane, band_q). */
__device__ __forceinline__ int prep_q(const PrepCtx &cx, const DJob &jb, int band, long blk) {
  const int q = blk >= cx.split_blk ? cx.q2 : cx.q;
  return q ? q : plane_q(jb, band, blk);
}

__device__ __forceinline__ PrepCtx prep_ctx(const DJob &jb, int band, int off, int pad) {
  PrepCtx c;
  c.krange = jb.krange;
  c.qm = jb.qm + off;
  c.x16 = jb.x16 + off - pad;
  c.rec = jb.rec + band;
  c.keys = jb.keys + (long)band*jb.nblocks;
  c.w = jb.w;
  c.len = jb.len;
  c.nb_bands = jb.nb_bands;
  c.q = jb.q[band];
  c.q2 = jb.q2[band];
  c.split_blk = jb.split_blk;
  c.beta = jb.beta[band];
  return c;
}

/* Everything of a band that precedes the search, from cg on: the two gain
   candidates (src/pvq_encoder.c:578-592), the first half of the record and the
   sort key.  Heavy bands get SMALL keys so that they are dispatched first. */
struct BandHead {
  int4 h0;                 /* cg, gain[2], k[0] | k[1] << 16                  */
  int4 h1;                 /* flags[0] | flags[1] << 8, 0, dist0 (lo, hi)     */
  unsigned short key;
};

constexpr double kCgainScale2 = (1./256)*(1./256);   /* OD_CGAIN_SCALE_2 */

/* src/pvq_encoder.c:586-587, a gain candidate in front of its search (the gain term alone), and :593-595, its
   distortion after the search */
__device__ __forceinline__ double noref_dist_gate(int32_t qcg, int32_t cg) {
  return ((1.4*(qcg - cg))*(qcg - cg))*kCgainScale2;
}

__device__ __forceinline__ double noref_dist(int32_t qcg, int32_t cg, double cos_dist) {
  return ((1.4*(qcg - cg))*(qcg - cg) + (qcg*(double)cg)*(2 - 2*cos_dist))*kCgainScale2;
}

__device__ __forceinline__ BandHead od_band_head(int beta, int n, int32_t cg) {
  const double dist0 = ((1.4*cg)*cg)*kCgainScale2;
  const int gain_bound = cg >> ODQ_CGAIN_SHIFT;
  const int first = gain_bound > 1 ? gain_bound : 1;
  int kk[2] = {0, 0};
  int fl[2] = {0, 0};
  int gain[2] = {0, 0};
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const int i = first + c;
    if (i <= gain_bound + 1) {
      const int32_t qcg = odq_shl32(i, ODQ_CGAIN_SHIFT);
      gain[c] = i;
      kk[c] = odq_compute_k_noref(qcg, n, beta);
      fl[c] = !(noref_dist_gate(qcg, cg) > dist0 && kk[c] != 0);
      if (fl[c] && kk[c] > kMaxK) fl[c] = 2;   /* not representable: reported, not searched */
      if (kk[c] > kMaxK) kk[c] = kMaxK;
    }
  }
  BandHead bh;
  bh.h0 = make_int4(cg, gain[0], gain[1], (kk[0] & 0xffff) | kk[1] << 16);
  bh.h1 = make_int4(fl[0] | fl[1] << 8, 0, __double2loint(dist0), __double2hiint(dist0));
  const bool s0 = fl[0] == 1;
  const bool s1 = fl[1] == 1;
  const int p0 = s0 ? kk[0] : 0;
  int p1 = 0;
  if (s1) p1 = s0 && kk[0] > 0 && kk[0] <= kk[1] ? kk[1] - kk[0] : kk[1];
  bh.key = (unsigned short)(kKeyBins - 1 - (od_pulse_bin(p0) << 4 | od_extra_bin(p1)));
  return bh;
}

__device__ __forceinline__ void od_band_candidates(const PrepCtx &cx, int n, long blk, int32_t cg) {
  const BandHead bh = od_band_head(cx.beta, n, cg);
  if (bh.h1.x & 0x0202) atomicAdd(cx.krange, 1u);
  int4 *out = reinterpret_cast<int4 *>(cx.rec + blk*cx.nb_bands);
  out[0] = bh.h0;
  out[1] = bh.h1;
  cx.keys[blk] = bh.key;
}

/* ---- prep, bands of up to 32 coefficients: one band per lane ------------------
   The band is gathered in coding order (od_raster_to_coding_order,
   src/partition.c:144-170) with ALL its loads in flight at once (one exposed
   memory latency per band, not one per four coefficients),
   od_vector_log_mag (src/pvq.c:472-484) gives the scaling shift, and the QM
   scaling (src/pvq_encoder.c:381,:398) is written as whole 16-byte groups of
   x16 (the 15-coefficient band includes the unused DC slot of its block). */
template <int N>
__device__ __forceinline__ void od_prep_lane(const DJob &jb, int band, int off, const BlockPos &bp) {
  constexpr int PAD = N == 15 ? 1 : 0;
  constexpr int NV = (N + PAD)/8;
  const PrepCtx cx = prep_ctx(jb, band, off, PAD);
  int qm[N];
#pragma unroll
  for (int j = 0; j < N; j++) qm[j] = cx.qm[j];
  int v[N];
#pragma unroll
  for (int j = 0; j < N; j++) v[j] = bp.src[kScanXY[off + j][1]*cx.w + kScanXY[off + j][0]];
  int sum = 0;
#pragma unroll
  for (int j = 0; j < N; j++) {
    const int t = (int16_t)(v[j] >> 8);
    sum += t*t;
  }
  const int xshift = odq_log_mag_shift(N, sum);
  int4 *xo = reinterpret_cast<int4 *>(cx.x16 + bp.blk*cx.len);
  int acc = 0;
#pragma unroll
  for (int g = 0; g < NV; g++) {
    int d[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      int x[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int j = g*8 + 2*t + u - PAD;
        x[u] = 0;
        if (j >= 0) x[u] = (int16_t)odq_shr_round(v[j]*qm[j], ODQ_QM_SHIFT + xshift);
        acc += x[u]*x[u];
      }
      d[t] = (x[0] & 0xffff) | x[1] << 16;
    }
    if (bp.live) xo[g] = make_int4(d[0], d[1], d[2], d[3]);
  }
  if (!bp.live) return;
  int32_t g;
  const int32_t cg = odq_gain_from_acc(acc, prep_q(cx, jb, band, bp.blk), cx.beta, xshift, &g);
  od_band_candidates(cx, N, bp.blk, cg);
}

__global__ __launch_bounds__(kWave) void k_prep_lane(Items it) {
  const int item = find_item(it, blockIdx.x);
  const DJob &jb = it.jobs[it.job[item]];
  const int band = it.band[item];
  const int off = jb.off[band];
  const int n = jb.off[band + 1] - off;
  const BlockPos bp = locate(jb, (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x);
  if (n == 8) od_prep_lane<8>(jb, band, off, bp);
  else if (n == 15) od_prep_lane<15>(jb, band, off, bp);
  else od_prep_lane<32>(jb, band, off, bp);
}

/* ---- prep, the CxC low-frequency corner of every block: one block per lane -----
   Coding positions 0..15 of a 4x4 block and 0..63 of every larger block lie in
   its top-left 4x4 / 8x8 corner (od_raster_to_coding_order,
   src/partition.c:144-170) and hold band 0 (15 coefficients) resp. bands 0..3
   (15, 8, 8, 32).  A lane loads its block's corner as whole 16-byte row
   segments - adjacent lanes read adjacent blocks, so a wavefront's loads are
   (nearly) contiguous, where one-band-per-lane gathers fetched every 32-byte
   sector once per coefficient - permutes it to coding order in registers (the
   scan is a compile-time constant), and prepares all of the corner's bands. */
/* Compile-time loop: f(std::integral_constant<int, J>) for J in [J0, J1).  The
   corner kernel indexes its register arrays with scan-table entries; the
   indices must be constant expressions for the arrays to stay in registers
   (a plain unrolled loop left them in scratch memory: 784 bytes per lane). */
template <int J0, int J1, class F>
__device__ __forceinline__ void od_static_for(F &&f) {
  if constexpr (J0 < J1) {
    f(std::integral_constant<int, J0>{});
    od_static_for<J0 + 1, J1>(f);
  }
}

/* Band B of a block (coding positions kCornerOff[B] .. kCornerOff[B + 1]) from its corner in registers, r =
   the raster of pitch C: od_vector_log_mag (src/pvq.c:472-484) gives the scaling shift, the QM scaling
   (src/pvq_encoder.c:381,:398) fills x16[position]; qmp = the block's QM row.  Returns the shift and the
   sum of the squares of the scaled vector. */
constexpr int kCornerOff[5] = {1, 16, 24, 32, 64};
struct CornerBand {
  int xshift;
  int acc;
};

template <int B, int C>
__device__ __forceinline__ CornerBand od_scale_corner_band(const int *r, const int16_t *qmp, int *x16) {
  constexpr int off = kCornerOff[B];
  constexpr int n = kCornerOff[B + 1] - off;
  int sum = 0;
  od_static_for<off, off + n>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const int t = (int16_t)(r[OD_SCAN_XY[j][1]*C + OD_SCAN_XY[j][0]] >> 8);
    sum += t*t;
  });
  CornerBand cb;
  cb.xshift = odq_log_mag_shift(n, sum);
  cb.acc = 0;
  od_static_for<off, off + n>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    x16[j] = (int16_t)odq_shr_round(r[OD_SCAN_XY[j][1]*C + OD_SCAN_XY[j][0]]*qmp[j],
     ODQ_QM_SHIFT + cb.xshift);
    cb.acc += x16[j]*x16[j];
  });
  return cb;
}

template <int C>
__global__ __launch_bounds__(kWave) void k_prep_corner(Items it) {
  constexpr int NC = C*C;
  constexpr int NBANDS = C == 4 ? 1 : 4;
  const int item = find_item(it, blockIdx.x);
  const DJob &jb = it.jobs[it.job[item]];
  const BlockPos bp = locate(jb, (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x);
  PrepCtx cx[NBANDS];
#pragma unroll
  for (int b = 0; b < NBANDS; b++) cx[b] = prep_ctx(jb, b, 0, 0);
  const int16_t *const qmp = cx[0].qm;
  const int w = cx[0].w;
  int r[NC];        /* raster, row-major CxC */
#pragma unroll
  for (int y = 0; y < C; y++) {
#pragma unroll
    for (int x = 0; x < C; x += 4) {
      const int4 q = *reinterpret_cast<const int4 *>(bp.src + y*w + x);
      r[y*C + x] = q.x;
      r[y*C + x + 1] = q.y;
      r[y*C + x + 2] = q.z;
      r[y*C + x + 3] = q.w;
    }
  }
  int x16[NC];
  x16[0] = 0;
  od_static_for<0, NBANDS>([&](auto bc) {
    constexpr int b = decltype(bc)::value;
    const CornerBand cb = od_scale_corner_band<b, C>(r, qmp, x16);
    if (bp.live) {
      int32_t g;
      const int32_t cg = odq_gain_from_acc(cb.acc, prep_q(cx[b], jb, b, bp.blk), cx[b].beta, cb.xshift, &g);
      od_band_candidates(cx[b], kCornerOff[b + 1] - kCornerOff[b], bp.blk, cg);
    }
  });
  if (bp.live) {
    int4 *xo = reinterpret_cast<int4 *>(cx[0].x16 + bp.blk*cx[0].len);
    od_static_for<0, NC/8>([&](auto gc) {
      constexpr int g = decltype(gc)::value;
      xo[g] = make_int4((x16[g*8] & 0xffff) | x16[g*8 + 1] << 16,
       (x16[g*8 + 2] & 0xffff) | x16[g*8 + 3] << 16,
       (x16[g*8 + 4] & 0xffff) | x16[g*8 + 5] << 16,
       (x16[g*8 + 6] & 0xffff) | x16[g*8 + 7] << 16);
    });
  }
}

/* ---- prep, 128-coefficient bands: one band per 16-lane DPP row ---------------- */
__global__ __launch_bounds__(kWave) void k_prep_wide(Items it) {
  constexpr int E = 8;
  constexpr int n = 16*E;
  const int item = find_item(it, blockIdx.x);
  const DJob &jb = it.jobs[it.job[item]];
  const int band = it.band[item];
  const int off = jb.off[band];
  const int lane = threadIdx.x;
  const int row = lane >> 4;
  const int l = lane & 15;
  const BlockPos bp = locate(jb, (long)(blockIdx.x - it.wg_start[item])*4 + row);
  const PrepCtx cx = prep_ctx(jb, band, off, 0);
  __shared__ unsigned short s_scan[n];
  for (int j = lane; j < n; j += kWave) s_scan[j] = gScanXY[off + j];
  const int4 qm4 = *reinterpret_cast<const int4 *>(cx.qm + l*E);
  __syncthreads();
  int v[E];
  int sum = 0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int xy = s_scan[l*E + e];
    v[e] = bp.src[(xy >> 8)*cx.w + (xy & 255)];
  }
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int t = (int16_t)(v[e] >> 8);
    sum += t*t;
  }
  sum = row_sum(sum);
  const int xshift = odq_log_mag_shift(n, sum);
  int acc = 0;
  int d[E/2];
  const int qd[4] = {qm4.x, qm4.y, qm4.z, qm4.w};
#pragma unroll
  for (int e = 0; e < E; e += 2) {
    const int x0 = (int16_t)odq_shr_round(v[e]*(int)(short)qd[e/2], ODQ_QM_SHIFT + xshift);
    const int x1 = (int16_t)odq_shr_round(v[e + 1]*(qd[e/2] >> 16), ODQ_QM_SHIFT + xshift);
    acc += x0*x0 + x1*x1;
    d[e/2] = (x0 & 0xffff) | x1 << 16;
  }
  if (bp.live) {
    *reinterpret_cast<int4 *>(cx.x16 + bp.blk*cx.len + l*E) = make_int4(d[0], d[1], d[2], d[3]);
  }
  acc = row_sum(acc);
  if (!bp.live || l != 0) return;
  int32_t g;
  const int32_t cg = odq_gain_from_acc(acc, prep_q(cx, jb, band, bp.blk), cx.beta, xshift, &g);
  od_band_candidates(cx, n, bp.blk, cg);
}

template <int PRICE>
__device__ __forceinline__ int choose_core(const Items &it, int job, const DJob &jb, long sb, int band,
 const RecHead &hd, double best_cost, int yy0, int yy1, int mom0, int mom1, double dist0, double dist1,
 const double *given);

/* ---- the two gain candidates of a band: one walk, one packer --------------------
   What k_search and the decided kernels (od_decide_band) share.  A band is S adjacent lanes (`half` = the
   lane's index in its group), each holding NL = N/S coefficients as |x| << 16 | 2*y in its LDS column pk
   (pvq_lane.cuh). */

/* Where the packer takes the sign (0 or -1) of the lane's coefficient j from */
struct SignRegs {          /* the scaled coefficients in registers */
  const int *xs;
  __device__ __forceinline__ int operator()(int j) const { return xs[j] >> 31; }
};
struct SignMask {          /* one bit per coefficient */
  unsigned long long sg;
  __device__ __forceinline__ int operator()(int j) const { return -(int)(sg >> j & 1u); }
};
template <int PAD>
struct SignX16 {           /* x16 as stored: 16-byte groups of int16, PAD slots in front of coefficient 0 */
  const int4 *x;
  __device__ __forceinline__ int operator()(int j) const {
    const int4 q = x[(j + PAD) >> 3];       /* (a whole group: its eight callers share one load) */
    const int d[4] = {q.x, q.y, q.z, q.w};
    const int e = d[(j + PAD) >> 1 & 3];
    return (j + PAD) & 1 ? e >> 31 : (int)(short)e >> 31;
  }
};

/* The candidate in the lane's column -> signed int16 pulses (src/pvq_encoder.c:220-222), 16 bytes at a time
   into sink(v, int4); zeros where !on.  PAD: the vectors of the 15-coefficient band begin with the unused DC
   slot of its block.  Returns the lane's part of od_pvq_rate's centre-of-mass sum SUM i*|y_i|
   (src/pvq_encoder.c:258-259), taken while the pulses pass through on their way out: the priced choice then
   never reads the vectors again. */
template <int NL, int PAD, class Sign, class Sink>
__device__ __forceinline__ int od_pack_pulses(const uint32_t *pk, int lane, int half, bool on, const Sign &sign,
 Sink &&sink) {
  int mom = 0;
#pragma unroll
  for (int v = 0; v < (NL + PAD)/8; v++) {
    int o[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int j0 = v*8 + 2*t - PAD;       /* -1: the DC slot */
      const int jc = j0 < 0 ? 0 : j0;
      const int y0 = j0 >= 0 && on ? (int)(pk[jc*kWave + lane] >> 1 & 0x7fffu) : 0;
      const int y1 = on ? (int)(pk[(j0 + 1)*kWave + lane] >> 1 & 0x7fffu) : 0;
      const int s0 = j0 >= 0 ? sign(jc) : 0;
      const int s1 = sign(j0 + 1);
      o[t] = (((y0 ^ s0) - s0) & 0xffff) | ((y1 ^ s1) - s1) << 16;
      mom += (half*NL + j0)*y0 + (half*NL + j0 + 1)*y1;          /* y0 = 0 where j0 < 0 */
    }
    sink(v, make_int4(o[0], o[1], o[2], o[3]));
  }
  return mom;
}

/* Per candidate: sum y^2, the distortion, SUM i*|y_i| of the whole band (the second half of a band record),
   and what the caller's hook kept of it. */
template <class Keep>
struct Walked {
  int yy0, yy1;
  int mom0, mom1;
  double dist0, dist1;
  Keep keep0, keep1;
};
struct KeepNothing {};

/* Both candidates of the head hd in the reference's order (src/pvq_encoder.c:578-595); the second continues from
   the pulses of the first where its K is not smaller (:128-137).  hook(c, on, keep) gets each finished candidate
   while its pulses are still in the column - the next search overwrites them - fills `keep` and returns the
   lane's moment sum (0 from a lane that does not pack).  `keep` is handed in, not captured by the hook: an
   array a closure holds by reference stayed in scratch (128 bytes in the 128-coefficient kernel).  The
   cosine distances go to jb.cos_dist where that is set.  A slot that is not in use has distortion 0. */
template <int NL, int S, class Keep, class Hook>
__device__ __forceinline__ Walked<Keep> od_walk_candidates(const Items &it, const DJob &jb, int band, long blk,
 bool live, const RecHead &hd, uint32_t *pk, const double *rsq, int lane, int half, Hook &&hook) {
  LaneSearch st;
  od_lane_prepare<NL, S>(st, pk, lane);
  const int32_t cg = hd.cg;
  int prev_k = 0;
  Walked<Keep> w;
#pragma unroll 1
  for (int c = 0; c < 2; c++) {
    /* selects, not hd.x[c] / w.x[c]: a dynamically indexed local array lives in scratch */
    const bool on = (c ? hd.flags[1] : hd.flags[0]) == 1;
    const int k = c ? hd.k[1] : hd.k[0];
    const int gain = c ? hd.gain[1] : hd.gain[0];
    const int32_t qcg = odq_shl32(gain, ODQ_CGAIN_SHIFT);
    const double g2 = (qcg*(double)cg)*kCgainScale2;
    const bool fresh = !(prev_k > 0 && prev_k <= k);
    const double cos_dist = od_lane_search<NL, S>(st, pk, rsq, lane, half, on, fresh, k, g2, it.lambda,
     it.force_seq != 0);
    int yy = 0;
    double dist = gain ? noref_dist_gate(qcg, cg) : 0.;
    if (on) {
      prev_k = k;
      yy = (int)st.yy;
      dist = noref_dist(qcg, cg, cos_dist);
    }
    if (live && half == 0 && jb.cos_dist) jb.cos_dist[2*(blk*jb.nb_bands + band) + c] = on ? cos_dist : 0.;
    Keep keep;
    const int mom = od_grp_add<S>(hook(c, on, keep));          /* the parts of the band */
    if (c) {
      w.yy1 = yy;
      w.dist1 = dist;
      w.mom1 = mom;
      w.keep1 = keep;
    }
    else {
      w.yy0 = yy;
      w.dist0 = dist;
      w.mom0 = mom;
      w.keep0 = keep;
    }
  }
  return w;
}

/* ---- search: one band per lane over the sorted order --------------------------
   Every lane reads its band's x16 with 16-byte loads, unpacks |x| << 16 into
   its LDS column, searches both candidates, and writes the signed pulses
   with 16-byte stores and the second half of the band record as one 32-byte
   sector.  No cross-lane traffic.

   A wavefront handles ONE group of 64 sorted positions.  Several groups per
   wavefront, strided by the item's wavefront count (one from each of as many
   weight classes), with the dependent loads of a group (sorted index ->
   record head and x16) issued one / two groups ahead, measured +30% on the
   short bands on MI355X: the extra live registers cost more occupancy than
   the prefetch buys, and the exposed latency that motivated it turned out to
   be eight serialised loads of the 1/sqrt table (od_rsq_stage).

   N = band size, S = lanes per band (pvq_lane.cuh: S = 2 for the 32- and the
   128-coefficient bands). */
template <int N, int S>
__global__ __launch_bounds__(kWave, (S == 2 ? 2 : 1)) void k_search(Items it) {
  constexpr int NL = N/S;                   /* coefficients per lane */
  constexpr int PAD = N == 15 ? 1 : 0;      /* leading DC slot */
  constexpr int NV = (NL + PAD)/8;          /* 16-byte groups of int16 */
  constexpr int SLOTS = kWave/S;            /* bands per wavefront */
  static_assert(N % S == 0 && (NL + PAD)%8 == 0, "a lane holds whole 16-byte groups");
  static_assert(S == 1 || PAD == 0, "pair mode has no padded band");
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  double *rsq = lds_d;                                   /* [kRsqN]  */
  uint32_t *pk = (uint32_t *)(rsq + kRsqN);              /* [NL][64] */
  const int lane = threadIdx.x;
  od_rsq_stage(rsq, lane);
  const int item = find_item(it, blockIdx.x);
  const DJob &jb = it.jobs[it.job[item]];
  const int band = it.band[item];
  const int half = S == 2 ? lane & 1 : 0;
  const int off = jb.off[band] - PAD + half*NL;
  const long nblocks = jb.nblocks;
  const int len = jb.len;
  const int nb_bands = jb.nb_bands;
  const unsigned *const ids = jb.ids + (long)band*nblocks;
  odhip_pvq_band *const recs = jb.rec + band;
  int16_t *const yout = jb.y + off;
  const long spos = (long)(blockIdx.x - it.wg_start[item])*SLOTS + lane/S;
  const bool live = spos < nblocks;
  const long blk = live ? ids[spos] : 0;
  const int4 *const hp = reinterpret_cast<const int4 *>(recs + blk*nb_bands);
  const int4 *const xp = reinterpret_cast<const int4 *>(jb.x16 + off + blk*len);
  const int4 h0 = hp[0];
  const int4 h1 = hp[1];
  int4 x[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) x[v] = xp[v];
  __syncthreads();   /* the 1/sqrt table */
  RecHead hd = rec_head(h0, h1);
  hd.flags[0] = live ? hd.flags[0] : 0;
  hd.flags[1] = live ? hd.flags[1] : 0;
#pragma unroll
  for (int v = 0; v < NV; v++) {
    const int d[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int j0 = v*8 + 2*t - PAD;
      if (j0 >= 0) pk[j0*kWave + lane] = (uint32_t)abs((int)(short)d[t]) << 16;
      pk[(j0 + 1)*kWave + lane] = (uint32_t)abs(d[t] >> 16) << 16;
    }
  }
  /* signs: from the registers for the short bands, re-read (L2) for the 128-coefficient band, whose
     registers are better spent on the pipelined search loops */
  const SignX16<PAD> sign = {N > 32 ? xp : x};
  const Walked<KeepNothing> w = od_walk_candidates<NL, S, KeepNothing>(it, jb, band, blk, live, hd, pk, rsq, lane,
   half, [&](int c, bool on, KeepNothing &) {
    if (!live) return 0;
    int4 *yo = reinterpret_cast<int4 *>(yout + ((long)c*nblocks + blk)*len);
    return od_pack_pulses<NL, PAD>(pk, lane, half, on, sign, [&](int v, int4 q) { yo[v] = q; });
  });
  if (live && half == 0) {
    int4 *out = reinterpret_cast<int4 *>(recs + blk*nb_bands) + 2;
    out[0] = make_int4(w.yy0, w.yy1, __double2loint(w.dist0), __double2hiint(w.dist0));
    out[1] = make_int4(__double2loint(w.dist1), __double2hiint(w.dist1), w.mom0, w.mom1);
  }
}

/* ---- corner bands decided where they are prepared ---------------------------------
   odhip_pvq_noref_bands_priced_multi: band 0 of every block (15 coefficients) and bands 1, 2
   of every block of 8x8 and up (8 each) - 4.2 of the 5.5 M bands of a 16-frame step - never
   leave the lane that prepared them.  The block's corner is in registers (k_prep_corner);
   the lane scales it, forms the band's record head in registers, runs both K-pulse searches
   (od_lane_search, |x| and pulses in its LDS column as in k_search), makes the priced choice
   and writes the choice record and the pulses that are read: no x16, no band record, no sort
   key, no sorted index for these bands - the two-pass stage wrote and re-read ~300 bytes per
   band for them, 16 bytes at a time in sorted order.  Natural block order instead of the
   sort by pulse class costs these short bands 3-12 % (measured with the sort keys forced
   equal); the records of a band listed as a close call are written whole, for the resolve.
   The 32- and the 128-coefficient bands are decided the same way, a lane group per band (od_decide_group). */
/* N = band size, S = lanes per band (2: the lane pair of pvq_lane.cuh, 4: the quad; `half` = the lane's
   index in its group, each lane holding NL = N/S coefficients in xs). */
/* MASK: the lane's LDS column already holds |x| << 16 and the signs come as one bit per coefficient in
   `sg` (a band too long to keep signed in registers across the searches); xs is not read. */
template <int N, int S = 1, bool MASK = false>
__device__ __forceinline__ void od_decide_band(const Items &it, int job, const DJob &jb, int band, long blk,
 bool live, const BandHead &bh, const int *xs, uint32_t *pk, const double *rsq, int lane, int half = 0,
 unsigned long long sg = 0) {
  constexpr int NL = N/S;
  constexpr int PAD = N == 15 ? 1 : 0;
  constexpr int NV = (NL + PAD)/8;
  /* a long band's first candidate leaves as it is packed (32 registers not held across the second
     search); a short one waits for the decision */
  constexpr bool EARLY0 = NL >= 64 || (S == 4 && NL >= 32);
  static_assert(S == 1 || PAD == 0, "group mode has no padded band");
  RecHead hd = rec_head(bh.h0, bh.h1);
  hd.flags[0] = live ? hd.flags[0] : 0;
  hd.flags[1] = live ? hd.flags[1] : 0;
  /* flags == 2: the reference would search this candidate; its K does not fit (od_krange.cuh).  In group mode
     every lane of the group holds the same head: the first one counts */
  if (live && half == 0 && (bh.h1.x & 0x0202)) atomicAdd(jb.krange, 1u);
  std::conditional_t<MASK, SignMask, SignRegs> sign;
  if constexpr (MASK) sign.sg = sg;
  else {
    sign.xs = xs;
#pragma unroll
    for (int j = 0; j < NL; j++) pk[j*kWave + lane] = (uint32_t)abs(xs[j]) << 16;
  }
  const int off = jb.off[band] - PAD + half*NL;
  const long nblocks = jb.nblocks;
  const int len = jb.len;
  struct Pulses {
    int4 q[NV];
  };
  const Walked<Pulses> w = od_walk_candidates<NL, S, Pulses>(it, jb, band, blk, live, hd, pk, rsq, lane, half,
   [&](int c, bool on, Pulses &y) {
    const int mom = od_pack_pulses<NL, PAD>(pk, lane, half, on, sign, [&](int v, int4 o) { y.q[v] = o; });
    if (EARLY0 && !c && live) {
      int4 *yo = reinterpret_cast<int4 *>(jb.y + off + blk*len);
#pragma unroll
      for (int v = 0; v < NV; v++) yo[v] = y.q[v];
    }
    return mom;
  });
  int res = 0;
  if (live && half == 0) {
    res = choose_core<1>(it, job, jb, blk*jb.nb_bands + band, band, hd, __hiloint2double(bh.h1.w, bh.h1.z), w.yy0,
     w.yy1, w.mom0, w.mom1, w.dist0, w.dist1, nullptr);
  }
  if constexpr (S > 1) res = od_grp_bcast<S, 0>(res);      /* decided by lane 0 of the group */
  if (!live) return;
  /* sel | close << 1: the chosen candidate's pulses; both, and the whole record, for a close call */
  if constexpr (!EARLY0) {
    if (!(res & 1) || (res & 2)) {
      int4 *yo = reinterpret_cast<int4 *>(jb.y + off + blk*len);
#pragma unroll
      for (int v = 0; v < NV; v++) yo[v] = w.keep0.q[v];
    }
  }
  if (res) {
    int4 *yo = reinterpret_cast<int4 *>(jb.y + off + (nblocks + blk)*len);
#pragma unroll
    for (int v = 0; v < NV; v++) yo[v] = w.keep1.q[v];
  }
  if ((res & 2) && half == 0) {
    int4 *out = reinterpret_cast<int4 *>(jb.rec + blk*jb.nb_bands + band);
    out[0] = bh.h0;
    out[1] = bh.h1;
    out[2] = make_int4(w.yy0, w.yy1, __double2loint(w.dist0), __double2hiint(w.dist0));
    out[3] = make_int4(__double2loint(w.dist1), __double2hiint(w.dist1), w.mom0, w.mom1);
  }
}

/* PART 0: band 0 of every block of every size (the 4x4 corner); PART 1: bands 1 and 2 of the blocks
   of 8x8 and up (x 4..7 of rows 0..1 and x 0..1 of rows 4..7, gen/od_scan_tables.h).  Two kernels
   rather than one per block: searched in one kernel the three bands hold 150 VGPRs (three waves
   per SIMD), apart 121 and ~100 (four and five). */
template <int PART>
__global__ __launch_bounds__(kWave) OD_DECIDE_OCC_ATTR void k_decide_corner(Items it) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  OD_SEARCH_VGPR_FLOOR();
  double *rsq = lds_d;                                   /* [kRsqN]  */
  uint32_t *pk = (uint32_t *)(rsq + kRsqN);              /* [15][64] */
  const int lane = threadIdx.x;
  od_rsq_stage(rsq, lane);
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const DJob &jb = it.jobs[job];
  const BlockPos bp = locate(jb, (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x);
  const int16_t *const qmp = jb.qm;
  const int w = jb.w;
  constexpr int C = 8;
  int r[C*C];       /* raster, row-major; only what the part's bands cover is loaded */
  if constexpr (PART == 0) {
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const int4 q = *reinterpret_cast<const int4 *>(bp.src + y*w);
      r[y*C] = q.x;
      r[y*C + 1] = q.y;
      r[y*C + 2] = q.z;
      r[y*C + 3] = q.w;
    }
  }
  else {
#pragma unroll
    for (int y = 0; y < 2; y++) {
      const int4 q = *reinterpret_cast<const int4 *>(bp.src + y*w + 4);
      r[y*C + 4] = q.x;
      r[y*C + 5] = q.y;
      r[y*C + 6] = q.z;
      r[y*C + 7] = q.w;
    }
#pragma unroll
    for (int y = 4; y < 8; y++) {
      const int2 q = *reinterpret_cast<const int2 *>(bp.src + y*w);
      r[y*C] = q.x;
      r[y*C + 1] = q.y;
    }
  }
  __syncthreads();   /* the 1/sqrt table */
  int x16[32];
  /* band b scaled into x16; its companded gain */
  auto scale_band = [&](auto bc) {
    constexpr int b = decltype(bc)::value;
    const CornerBand cb = od_scale_corner_band<b, C>(r, qmp, x16);
    int32_t g;
    return odq_gain_from_acc(cb.acc, band_q(jb, b, bp.blk), jb.beta[b], cb.xshift, &g);
  };
  if constexpr (PART == 0) {
    const int32_t cg = scale_band(std::integral_constant<int, 0>{});
    od_decide_band<15>(it, job, jb, 0, bp.blk, bp.live, od_band_head(jb.beta[0], 15, cg), x16 + 1, pk, rsq, lane);
  }
  else {
    /* band 2 waits as packed int16 pairs and its gain while band 1 is searched */
    int32_t cg2 = scale_band(std::integral_constant<int, 2>{});
    int packed[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      packed[i] = (x16[24 + 2*i] & 0xffff) | x16[25 + 2*i] << 16;
      /* materialise here: sunk below the search, the raster values it is made of would stay live */
      asm volatile("" : "+v"(packed[i]));
    }
    asm volatile("" : "+v"(cg2));
    const int32_t cg1 = scale_band(std::integral_constant<int, 1>{});
    od_decide_band<8>(it, job, jb, 1, bp.blk, bp.live, od_band_head(jb.beta[1], 8, cg1), x16 + 16, pk, rsq, lane);
    int xs[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      xs[2*i] = (int)(short)packed[i];
      xs[2*i + 1] = packed[i] >> 16;
    }
    od_decide_band<8>(it, job, jb, 2, bp.blk, bp.live, od_band_head(jb.beta[2], 8, cg2), xs, pk, rsq, lane);
  }
}

/* ---- the 32- and the 128-coefficient bands the same way, a lane group per band ---
   Band 3 of every block of 8x8 and up and bands 4 and 5 of 16x16 and up (32 coefficients), the three bands of
   128: S lanes per band as in k_search, lane `half` of the group holding NL = N/S coding positions.
   od_decide_group is the kernel; what differs by size is how the coefficients come in - a loader,
   load(v, src, w, off, pk, lane, half): v[j] = coding position off + half*NL + j of the block at src (row
   pitch w), the group's LDS columns pk being free until the scaled vector is written - and where the scaled
   vector waits (MASK, od_decide_band). */

/* STAGED ROW SEGMENTS (round 5), a lane pair per band.  The band's N coefficients come in as aligned row
   segments of 2 (N = 32: 8 bytes) or 4 coefficients (N = 128: 16 bytes), half of them per lane - whole
   sectors, every byte fetched is used; the 64 four-byte gathers per lane this replaces for N = 128 touched a
   different 64-byte line per lane and instruction: 951 MB of HBM traffic per launch for 198 MB of
   coefficients, profiles/r4_pmc_traffic.json - are parked in the pair's two LDS columns in that staged order,
   and each lane picks its coding positions out of them (kSeg* / kSlot*; both lanes of a pair are in one
   wavefront: no barrier). */
template <int N>
struct LoadStaged {
  static __device__ __forceinline__ int seg(int geo, int q) {
    if constexpr (N == 32) return kSeg32[geo][q];
    else return kSeg128[geo][q];
  }
  static __device__ __forceinline__ int slot(int geo, int p) {
    if constexpr (N == 32) return kSlot32[geo][p];
    else return kSlot128[geo][p];
  }
  template <int NL>
  static __device__ __forceinline__ void load(int (&v)[NL], const od_coeff *src, int w, int off, uint32_t *pk,
   int lane, int half) {
    static_assert((N == 32 || N == 128) && 2*NL == N, "a lane pair of a band that has tables");
    constexpr int SEG = N == 32 ? 2 : 4;        /* coefficients per segment */
    constexpr int NSEG = NL/SEG;                /* segments per lane */
    using Vec = std::conditional_t<SEG == 2, int2, int4>;
    const int geo = (unsigned)off/N - 1;
    Vec raw[NSEG];
#pragma unroll
    for (int i = 0; i < NSEG; i++) {
      const int s0 = seg(geo, i);
      const int s1 = seg(geo, NSEG + i);
      const int sg_ = half ? s1 : s0;
      raw[i] = *reinterpret_cast<const Vec *>(src + (sg_ >> 8)*w + (sg_ & 255));
    }
#pragma unroll
    for (int i = 0; i < NSEG; i++) {
#pragma unroll
      for (int e = 0; e < SEG; e++) {
        pk[(SEG*i + e)*kWave + lane] = (uint32_t)reinterpret_cast<const int *>(&raw[i])[e];
      }
    }
    const int pair0 = lane & ~1;
#pragma unroll
    for (int j = 0; j < NL; j++) {
      const int t0 = slot(geo, j);
      const int t1 = slot(geo, NL + j);
      const int sl = half ? t1 : t0;
      v[j] = (int)pk[(sl & (NL - 1))*kWave + pair0 + (unsigned)sl/NL];
    }
  }
};

/* SCAN GATHERS, a lane quad per band (experiments build). */
struct LoadGather {
  template <int NL>
  static __device__ __forceinline__ void load(int (&v)[NL], const od_coeff *src, int w, int off, uint32_t *,
   int, int sub) {
#pragma unroll
    for (int j = 0; j < NL; j++) {
      /* the scan positions of the four parts are wave-uniform (scalar loads), the lane takes its own */
      const int oa = kScanXY[off + j][1]*w + kScanXY[off + j][0];
      const int ob = kScanXY[off + NL + j][1]*w + kScanXY[off + NL + j][0];
      const int oc = kScanXY[off + 2*NL + j][1]*w + kScanXY[off + 2*NL + j][0];
      const int od = kScanXY[off + 3*NL + j][1]*w + kScanXY[off + 3*NL + j][0];
      v[j] = src[sub == 0 ? oa : sub == 1 ? ob : sub == 2 ? oc : od];
    }
  }
};

/* The per-size register choices were measured: 32 coefficients load qm[] with the segments and keep the scaled
   vector xs[] in registers (MASK = false); 128 read qmp[j] at the scaling step and write |x| << 16 straight
   into the column, the raw coefficients waiting in registers only until the band's scaling shift is known and
   the signs as one bit each (MASK = true).  rsq = the kernel's dynamic LDS: the 1/sqrt table, then the
   wavefront's NL columns. */
template <int N, int S, bool MASK, class Load>
__device__ __forceinline__ void od_decide_group(const Items &it, double *rsq) {
  constexpr int NL = N/S;
  uint32_t *pk = (uint32_t *)(rsq + kRsqN);              /* [NL][64] */
  const int lane = threadIdx.x;
  od_rsq_stage(rsq, lane);
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const DJob &jb = it.jobs[job];
  const int band = it.band[item];
  const int half = lane & (S - 1);
  const int off = jb.off[band];
  const BlockPos bp = locate(jb, (long)(blockIdx.x - it.wg_start[item])*(kWave/S) + lane/S);
  const int16_t *const qmp = jb.qm + off + half*NL;
  int v[NL];
  Load::load(v, bp.src, jb.w, off, pk, lane, half);
  int qm[NL];
  if constexpr (!MASK) {
#pragma unroll
    for (int j = 0; j < NL; j++) qm[j] = qmp[j];
  }
  __syncthreads();   /* the 1/sqrt table */
  int sum = 0;
#pragma unroll
  for (int j = 0; j < NL; j++) {
    const int t = (int16_t)(v[j] >> 8);
    sum += t*t;
  }
  const int xshift = odq_log_mag_shift(N, od_grp_add<S>(sum));
  int xs[MASK ? 1 : NL];
  unsigned long long sg = 0;
  int acc = 0;
#pragma unroll
  for (int j = 0; j < NL; j++) {
    if constexpr (MASK) qm[j] = qmp[j];
    const int x = (int16_t)odq_shr_round(v[j]*qm[j], ODQ_QM_SHIFT + xshift);
    acc += x*x;
    if constexpr (MASK) {
      sg |= (unsigned long long)(x < 0) << j;
      pk[j*kWave + lane] = (uint32_t)abs(x) << 16;
    }
    else xs[j] = x;
  }
  acc = od_grp_add<S>(acc);
  int32_t g;
  const int32_t cg = odq_gain_from_acc(acc, band_q(jb, band, bp.blk), jb.beta[band], xshift, &g);
  od_decide_band<N, S, MASK>(it, job, jb, band, bp.blk, bp.live, od_band_head(jb.beta[band], N, cg), xs, pk, rsq,
   lane, half, sg);
}

/* Natural order costs the 32-coefficient bands 1 % against the sort by pulse class (measured). */
__global__ __launch_bounds__(kWave) OD_DECIDE_OCC_ATTR void k_decide_lane32(Items it) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  OD_SEARCH_VGPR_FLOOR();
  od_decide_group<32, 2, false, LoadStaged<32>>(it, lds_d);
}

/* The sort by pulse class buys the 128-coefficient bands -2 % on the default content and +8 % on the natural
   one (measured with the keys forced equal) against 130 us of preparation and sort and a 600 MB round trip of
   scaled vectors. */
__global__ __launch_bounds__(kWave, 2) void k_decide_pair128(Items it) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  od_decide_group<128, 2, true, LoadStaged<128>>(it, lds_d);
}

#ifdef ODHIP_EXPERIMENTS
/* The 128-coefficient bands on a QUAD of lanes per band (round 5; k_decide_pair128 above is the pair form it
   was measured against, experiments build only): 32 coding positions per lane, 8 KiB of LDS columns per wavefront instead
   of 16.  The pair form held two wavefronts per SIMD (20 KiB each) and ran at 0.67 of VALU issue: its
   argmax scans are chains of dependent selects, and two wavefronts do not cover a dependency chain
   (the same effect the 64x64 transforms showed at 2.25 wavefronts per SIMD).  Same bands
   in flight per CU, twice the wavefronts, every scan half as long; the 64 gathers per lane become 32 and
   the raw coefficients held until the band's shift is known 32 registers instead of 64. */
__global__ __launch_bounds__(kWave, 3) void k_decide_quad128(Items it) {
  extern __shared__ __attribute__((aligned(16))) double lds_d[];
  od_decide_group<128, 4, true, LoadGather>(it, lds_d);
}
#endif

/* ---- choice: one (block, band) per lane --------------------------------------
   The comparison `cost <= best_cost` of src/pvq_encoder.c:597-609 with
   cost = dist + lambda*rate (rate from the host entropy model, or absent),
   then od_gain_expand (src/pvq.c:766-811) and the synthesis scale of
   od_pvq_synthesis_partial (src/pvq.c:1057-1078).  choice = {sel, qg, scale,
   qshift}. */
/* PRICE = 0: cost = dist + lambda*rate with the host's rate table (or no rate at all);
   PRICE = 1: the rate is od_pvq_rate's closed form (speed > 0) evaluated HERE from the
   candidate's pulses with the device's log.  The device's and the host libm's log may
   differ in the last place, so a comparison whose two costs lie within odq_rate_tol of each
   other is not trusted: the band is listed, odhip_pvq_choose_priced_resolve recomputes its
   rates with the host's libm (the function the reference calls) and k_choose_list decides
   it again; PRICE = 2 is that second decision (rates given per band). */
/* The decision itself, on values: from the record (k_choose) or straight from the
   registers of the search that produced them (od_decide_band). */
/* od_pvq_rate's pulse part (the whole rate of a no-reference candidate: theta == -1) is a function of
   (sum, k, n) alone: read from tables filled ONCE per device by the function they replace (k_nrate_fill:
   same code, same device log - identical values; pvq_refbands.hip does the same for the with-reference
   stage), two logs and two divisions per candidate otherwise.  Entries [k][sum], k <= NRateTab<N>::K,
   sum <= (N - 1)*K; the depths cover the pulse counts the luma bands of a 1080p keyframe reach at the
   operating points measured except band 0 of the 32x32 / 64x64 blocks (K 100-360: computed inline). */
template <int N> struct NRateTab {
  static constexpr int K = N == 15 ? 128 : N == 8 ? 64 : 80;
  static constexpr int W = (N - 1)*K + 1;
  static constexpr int SIZE = (K + 1)*W;
};
__device__ double gNRate8[NRateTab<8>::SIZE];
__device__ double gNRate15[NRateTab<15>::SIZE];
__device__ double gNRate32[NRateTab<32>::SIZE];
__device__ double gNRate128[NRateTab<128>::SIZE];

template <int N>
__device__ __forceinline__ double *nrate_tab(void) {
  return N == 8 ? gNRate8 : N == 15 ? gNRate15 : N == 32 ? gNRate32 : gNRate128;
}

template <int N>
__global__ void k_nrate_fill(void) {
  constexpr int W = NRateTab<N>::W;
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i >= NRateTab<N>::SIZE) return;
  const int k = i/W;
  const int sum = i - k*W;
  nrate_tab<N>()[i] = k == 0 ? 0. : odq_pvq_rate_pulses(sum, k, N);
}

/* odq_pvq_rate_fast(sum, k, n, qg, 0, -1, 0, 1, 0): the join adds nothing when theta < 0 */
__device__ __forceinline__ double noref_rate(int sum, int k, int n) {
  if (n == 15) {
    if (k <= NRateTab<15>::K) return gNRate15[k*NRateTab<15>::W + sum];
  }
  else if (n == 8) {
    if (k <= NRateTab<8>::K) return gNRate8[k*NRateTab<8>::W + sum];
  }
  else if (n == 32) {
    if (k <= NRateTab<32>::K) return gNRate32[k*NRateTab<32>::W + sum];
  }
  else if (n == 128) {
    if (k <= NRateTab<128>::K) return gNRate128[k*NRateTab<128>::W + sum];
  }
  return odq_pvq_rate_pulses(sum, k, n);
}

/* Returns sel | close << 1. */
template <int PRICE>
__device__ __forceinline__ int choose_core(const Items &it, int job, const DJob &jb, long sb, int band,
 const RecHead &hd, double best_cost, int yy0, int yy1, int mom0, int mom1, double dist0, double dist1,
 const double *given) {
  const int qb = band_q(jb, band, sb/jb.nb_bands);
  const int betab = jb.beta[band];
  const double *const rate = jb.rate;
  int4 *const choice = reinterpret_cast<int4 *>(jb.choice);
  int32_t *const qg_out = jb.qg_out;
  const int yys[2] = {yy0, yy1};
  const int moms[2] = {mom0, mom1};
  const double dists[2] = {dist0, dist1};
  int qg = 0;
  int sel = 0;
  bool close = false;
  for (int c = 0; c < 2; c++) {
    if (hd.flags[c] != 1) continue;
    double cost = dists[c];
    if (PRICE == 0) {
      if (rate) cost = cost + it.lambda*rate[2*sb + c];
    }
    else if (PRICE == 1) {
      const int n = jb.off[band + 1] - jb.off[band];
      cost = cost + it.lambda*noref_rate(moms[c], hd.k[c], n);
      const double d = cost - best_cost;
      if ((d < 0 ? -d : d) <= it.tol_scale*odq_rate_tol(cost, best_cost)) close = true;
    }
    else cost = cost + it.lambda*given[c];
    if (cost <= best_cost) {
      best_cost = cost;
      qg = hd.gain[c];
      sel = c;
    }
  }
  if (PRICE == 1 && close) {
    const unsigned slot = atomicAdd(it.pcount, 1u);
    if (slot < (unsigned)kPUncCap) {
      PUnc e;
      e.job = job;
      e.sb = (unsigned)sb;
      e.rate[0] = 0;
      e.rate[1] = 0;
      it.plist[slot] = e;
    }
  }
  int32_t scale = 0;
  int qshift = ODQ_QM_INV_SHIFT;
  if (qg != 0) {
    const int32_t g = odq_gain_expand(odq_shl32(qg, ODQ_CGAIN_SHIFT), qb, betab);
    const int yy = sel ? yys[1] : yys[0];
    int gshift = odq_ilog(g) - 14;
    gshift = gshift > 0 ? gshift : 0;
    if (yy != 0) {
      int rsqrt_shift;
      const int16_t rsqrt = odq_rsqrt(yy, &rsqrt_shift);
      scale = odq_vshr_round(rsqrt*(int64_t)g, rsqrt_shift + gshift - 16);
    }
    qshift = ODQ_QM_INV_SHIFT - gshift;
  }
  choice[sb] = make_int4(sel, qg, scale, qshift);
  if (qg_out) qg_out[sb] = qg;
  return sel | (close ? 2 : 0);
}

template <int PRICE>
__device__ __forceinline__ void choose_band(const Items &it, int job, const DJob &jb, long sb,
 const double *given) {
  const int band = (int)(sb % jb.nb_bands);
  const int4 *r = reinterpret_cast<const int4 *>(jb.rec + sb);
  const RecHead hd = rec_head_load(jb.rec + sb);
  const int4 r1 = r[1];
  const int4 r2 = r[2];
  const int4 r3 = r[3];
  choose_core<PRICE>(it, job, jb, sb, band, hd, __hiloint2double(r1.w, r1.z), r2.x, r2.y, r3.z, r3.w,
   __hiloint2double(r2.w, r2.z), __hiloint2double(r3.y, r3.x), given);
}

template <int PRICE>
__global__ __launch_bounds__(256) void k_choose(Items it) {
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const DJob &jb = it.jobs[job];
  const long sb = (long)(blockIdx.x - it.wg_start[item])*256 + threadIdx.x;
  if (sb >= jb.nblocks*jb.nb_bands) return;
  choose_band<PRICE>(it, job, jb, sb, nullptr);
}

__global__ __launch_bounds__(kWave) void k_choose_list(Items it, const PUnc *list, int count) {
  const int i = blockIdx.x*kWave + threadIdx.x;
  if (i >= count) return;
  const PUnc e = list[i];
  choose_band<2>(it, e.job, it.jobs[e.job], e.sb, list[i].rate);
}

/* ---- synthesis: four horizontally adjacent coefficients per lane -------------
   x = y*scale (Q16, no rounding), out = SHR_ROUND(x*qm_inv, qshift)
   (src/pvq.c:1081-1092) scattered to raster by the inverse scan; DC passed
   through (keyframes quantise it in the Haar DC tree, src/encode.c:1377);
   positions PVQ never codes are zero (od_init_skipped_coeffs,
   src/state.c:1347-1358).  Every store is a coalesced 16-byte row segment. */
__global__ __launch_bounds__(256) void k_synth(Items it) {
  const int item = find_item(it, blockIdx.x);
  const DJob &jb = it.jobs[it.job[item]];
  __shared__ short s_inv[32*32];
  __shared__ unsigned char s_band[OD_SCAN_LEN];
  for (int i = threadIdx.x; i < 32*32; i += 256) s_inv[i] = gInvScan[i];
  for (int i = threadIdx.x; i < OD_SCAN_LEN; i += 256) s_band[i] = gBandOf[i];
  /* One workgroup = one 1024-coefficient segment of one plane row: the
     decomposition of the workgroup index is scalar (once per wave), the
     per-lane one is shifts only. */
  __shared__ int4 s_choice[256*ODHIP_MAX_BANDS/4];  /* <= 1024/N blocks x nb bands */
  const int segs = (jb.w + 1023) >> 10;
  const int wg = blockIdx.x - it.wg_start[item];
  const int seg = wg % segs;
  const int prow = wg / segs;                 /* plane * h + y */
  const int y = prow % jb.h;
  const int p = prow / jb.h;
  const int sh = jb.bs + 2;
  const int N = 1 << sh;
  const int by = y >> sh;
  const int ly = y & (N - 1);
  const int x0 = seg << 10;
  const int bx0 = x0 >> sh;
  const int nbx = min(1024 >> sh, jb.bw - bx0);    /* blocks this segment touches */
  const long blk0 = ((long)p*jb.bh + by)*jb.bw + bx0;
  for (int i = threadIdx.x; i < nbx*jb.nb_bands; i += 256) {
    s_choice[i] = reinterpret_cast<const int4 *>(jb.choice)[blk0*jb.nb_bands + i];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x*4;
  if (x >= jb.w) return;
  const int bxl = (x >> sh) - bx0;
  const int lx = x & (N - 1);
  const long blk = blk0 + bxl;
  const long idx = (long)p*jb.w*jb.h + (long)y*jb.w + x;
  int out[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int v = 0;
    if (ly < 32 && lx + i < 32) {
      const int j = s_inv[ly*32 + lx + i];
      if (j == 0) v = jb.coef[idx];
      else if (j > 0 && j < jb.len) {
        const int band = s_band[j];
        const int4 ch = s_choice[bxl*jb.nb_bands + band];
        if (ch.y != 0) {
          const int yv = jb.y[((long)ch.x*jb.nblocks + blk)*jb.len + j];
          v = od_synth_noref(OdSynthExact(ch.z), yv, jb.qm_inv[j], ch.w);
        }
      }
    }
    out[i] = v;
  }
  *reinterpret_cast<int4 *>(jb.dq + idx) = make_int4(out[0], out[1], out[2], out[3]);
}

/* ---- chroma-from-luma predictions ------------------------------------------------
   od_resample_luma_coeffs (reference src/intra.c:72-109) for 4:2:0 when the luma
   block is at least 8x8 (:97-108): the prediction of the chroma block is the
   upper-left quarter of the decoded luma block's coefficients.  Here the decoded
   luma coefficients are not read from a plane: they are dequantised on the fly
   from the chosen pulses of the luma band stage (od_synth_noref, od_pvq_synth.cuh),
   the DC passed through as k_synth passes it.  One output coefficient per thread;
   the result is written `copies` times (Cb and Cr share the prediction). */
struct CflOut {
  od_coeff *ref[kMaxJobs];
  int copies;
};

/* Eight consecutive coding positions of one luma block per thread.  The scan is
   nested: the first n*n coding positions of a 2n x 2n block are its n x n corner
   (for 64x64 blocks only 512 of the corner's 1024 positions are coded; the host
   clears those planes first), and a chunk of eight never straddles a band, so
   pulses, inverse QM and scan positions are 16-byte loads and one choice record
   serves the chunk. */
__global__ __launch_bounds__(256) void k_cfl_ref(Items it, CflOut out) {
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const DJob &jb = it.jobs[job];
  const int N = 4 << jb.bs;
  const int n = N >> 1;
  const int cw = jb.w >> 1;
  const int ncode = n*n < jb.len ? n*n : jb.len;       /* coded positions inside the corner */
  const int cpb = ncode >> 3;
  const long t = (long)(blockIdx.x - it.wg_start[item])*256 + threadIdx.x;
  const long blk = t/cpb;
  if (blk >= jb.nblocks) return;
  const int c0 = (int)(t - blk*cpb) << 3;
  const long per_blocks = (long)jb.bw*jb.bh;
  const int p = (int)(blk/per_blocks);
  const int rem = (int)(blk - p*per_blocks);
  const int by = rem/jb.bw;
  const int bx = rem - by*jb.bw;
  const long per = (long)cw*(jb.h >> 1);
  od_coeff *dst = out.ref[job] + p*per + (long)by*n*cw + bx*n;
  const long copy_stride = per*jb.nplanes;
  const uint4 sc4 = *reinterpret_cast<const uint4 *>(gScanXY + c0);
  const unsigned scw[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
  const int4 ch = reinterpret_cast<const int4 *>(jb.choice)[blk*jb.nb_bands + gBandOf[c0 ? c0 : 1]];
  unsigned yw[4] = {0, 0, 0, 0};
  if (ch.y != 0) {
    const uint4 y4 = *reinterpret_cast<const uint4 *>(jb.y + ((long)ch.x*jb.nblocks + blk)*jb.len + c0);
    yw[0] = y4.x;
    yw[1] = y4.y;
    yw[2] = y4.z;
    yw[3] = y4.w;
  }
  const uint4 q4 = *reinterpret_cast<const uint4 *>(jb.qm_inv + c0);
  const unsigned qw[4] = {q4.x, q4.y, q4.z, q4.w};
  od_noref_chunk8(OdSynthExact(ch.z), ch.w, yw, qw, [&](int e, int val) {
    const unsigned pk = (scw[e >> 1] >> (16*(e & 1))) & 0xffffu;
    if (c0 == 0 && e == 0) val = jb.coef[(long)p*jb.w*jb.h + (long)by*N*jb.w + bx*N];
    od_coeff *d = dst + (long)(pk >> 8)*cw + (pk & 255);
    for (int k = 0; k < out.copies; k++) d[k*copy_stride] = val;
  });
}

/* Decoded coefficient (v, u), v, u < 2, of the 4x4 luma block blk of a level-0
   job: the DC passed through, the others dequantised from the chosen pulses. */
__device__ __forceinline__ int cfl_luma4(const DJob &jb, long blk, int p, int by, int bx, int v, int u) {
  const int c = gInvScan[v*32 + u];
  if (c == 0) return jb.coef[(long)p*jb.w*jb.h + (long)by*4*jb.w + bx*4];
  const int4 ch = reinterpret_cast<const int4 *>(jb.choice)[blk*jb.nb_bands];
  if (ch.y == 0) return 0;
  const int yv = jb.y[((long)ch.x*jb.nblocks + blk)*jb.len + c];
  return od_synth_noref(OdSynthExact(ch.z), yv, jb.qm_inv[c], ch.w);
}

/* The 4x4 luma case of od_resample_luma_coeffs (src/intra.c:77-89): the four 4x4
   luma blocks over a 4x4 chroma block are merged by od_tf_up_hv_lp
   (src/tf.c:82-108, OD_HAAR_KERNEL src/tf.h:34-45) and scaled by
   OD_CFL_SCALING4 (src/intra.c:65-70): od_cfl_tf4 (od_cfl.cuh).  One output
   coefficient per thread: it evaluates the Haar kernel of its 2x2 group and
   keeps its own output. */
__global__ __launch_bounds__(256) void k_cfl_ref_tf(Items it, CflOut out) {
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const DJob &jb = it.jobs[job];
  const int cw = jb.w >> 1;
  const int chh = jb.h >> 1;
  const long t = (long)(blockIdx.x - it.wg_start[item])*256 + threadIdx.x;
  const long per = (long)cw*chh;
  if (t >= per*jb.nplanes) return;
  const int p = (int)(t/per);
  const int rem = (int)(t - p*per);
  const int y = rem/cw;
  const int x = rem - y*cw;
  const int cby = y >> 2;
  const int i = y & 3;
  const int cbx = x >> 2;
  const int j = x & 3;
  const int gy = i >> 1;          /* the loop indices y, x of od_tf_up_hv_lp */
  const int gx = j >> 1;
  int v[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {   /* ll, lh (right block), hl (lower block), hh */
    const int by = 2*cby + (q >> 1);
    const int bx = 2*cbx + (q & 1);
    const long blk = ((long)p*jb.bh + by)*jb.bw + bx;
    v[q] = cfl_luma4(jb, blk, p, by, bx, gy, gx);
  }
  const int val = od_cfl_tf4(v[0], v[1], v[2], v[3], i, j);
  od_coeff *dst = out.ref[job] + t;
  for (int k = 0; k < out.copies; k++) dst[k*per*jb.nplanes] = val;
}

/* ---- host side ----------------------------------------------------------------- */
odhip_device_once g_tables_once;

int upload_tables_now(void) {
  short inv[32*32];
  unsigned char band_of[OD_SCAN_LEN];
  for (int i = 0; i < 32*32; i++) inv[i] = -1;
  for (int j = 0; j < OD_SCAN_LEN; j++) inv[OD_SCAN_XY[j][1]*32 + OD_SCAN_XY[j][0]] = (short)j;
  for (int j = 0; j < OD_SCAN_LEN; j++) {
    int b = 0;
    while (b + 1 < OD_NBANDS[4] && j >= OD_BAND_OFFS[4][b + 1]) b++;
    band_of[j] = (unsigned char)b;
  }
  unsigned short packed[OD_SCAN_LEN];
  for (int j = 0; j < OD_SCAN_LEN; j++) packed[j] = (unsigned short)(OD_SCAN_XY[j][1] << 8 | OD_SCAN_XY[j][0]);
  ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(kScanXY), OD_SCAN_XY, sizeof(OD_SCAN_XY)));
  {
    unsigned short seg[3][32];
    unsigned char slot[3][128];
    for (int g = 0; g < 3; g++) {
      const int off = 128*(g + 1);
      /* the distinct (y, x / 4) groups of the band's positions, in raster order */
      int n = 0;
      for (int y = 0; y < 32; y++) {
        for (int x4 = 0; x4 < 8; x4++) {
          int cnt = 0;
          for (int p = 0; p < 128; p++) cnt += OD_SCAN_XY[off + p][1] == y && OD_SCAN_XY[off + p][0]/4 == x4;
          if (cnt == 0) continue;
          if (cnt != 4 || n >= 32) return ODHIP_EFAULT;     /* the region is made of whole aligned segments */
          seg[g][n++] = (unsigned short)(y << 8 | 4*x4);
        }
      }
      if (n != 32) return ODHIP_EFAULT;
      for (int p = 0; p < 128; p++) {
        const int key = OD_SCAN_XY[off + p][1] << 8 | (OD_SCAN_XY[off + p][0] & ~3);
        int q = 0;
        while (seg[g][q] != key) q++;
        slot[g][p] = (unsigned char)(4*q + (OD_SCAN_XY[off + p][0] & 3));
      }
    }
    ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(kSeg128), seg, sizeof(seg)));
    ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(kSlot128), slot, sizeof(slot)));
  }
  {
    unsigned short seg[3][16];
    unsigned char slot[3][32];
    for (int g = 0; g < 3; g++) {
      const int off = 32*(g + 1);
      int n = 0;
      for (int y = 0; y < 16; y++) {
        for (int x2 = 0; x2 < 8; x2++) {
          int cnt = 0;
          for (int p = 0; p < 32; p++) cnt += OD_SCAN_XY[off + p][1] == y && OD_SCAN_XY[off + p][0]/2 == x2;
          if (cnt == 0) continue;
          if (cnt != 2 || n >= 16) return ODHIP_EFAULT;
          seg[g][n++] = (unsigned short)(y << 8 | 2*x2);
        }
      }
      if (n != 16) return ODHIP_EFAULT;
      for (int p = 0; p < 32; p++) {
        const int key = OD_SCAN_XY[off + p][1] << 8 | (OD_SCAN_XY[off + p][0] & ~1);
        int q = 0;
        while (seg[g][q] != key) q++;
        slot[g][p] = (unsigned char)(2*q + (OD_SCAN_XY[off + p][0] & 1));
      }
    }
    ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(kSeg32), seg, sizeof(seg)));
    ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(kSlot32), slot, sizeof(slot)));
  }
  ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gScanXY), packed, sizeof(packed)));
  ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gInvScan), inv, sizeof(inv)));
  ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gBandOf), band_of, sizeof(band_of)));
  k_rsq_fill<<<1, kRsqN, 0, 0>>>();
  od_rsqrt_huge_fill_launch();
  k_nrate_fill<8><<<(NRateTab<8>::SIZE + 255)/256, 256, 0, 0>>>();
  k_nrate_fill<15><<<(NRateTab<15>::SIZE + 255)/256, 256, 0, 0>>>();
  k_nrate_fill<32><<<(NRateTab<32>::SIZE + 255)/256, 256, 0, 0>>>();
  k_nrate_fill<128><<<(NRateTab<128>::SIZE + 255)/256, 256, 0, 0>>>();
  ODHIP_TRY(hipDeviceSynchronize());
  return ODHIP_SUCCESS;
}

int upload_tables(void) {
  return odhip_once_per_device(g_tables_once, upload_tables_now);
}

/* Everything the band stage keeps between calls, owned by the calling thread's
   current context (od_ctx.cuh): ONE call sequence may be in flight per context. */
struct BandState {
  JobTables<DJob, kMaxJobs> tabs;  /* device job tables, cached by content         */
  Counters<2> counters;            /* [0] priced choice: bands too close to call on the
                                      device, [1] bands above ODHIP_PVQ_MAX_K (od_krange.cuh) */
  DeviceBuf<PUnc> plist;           /* ... the list of the former [kPUncCap]        */
  PinnedCount priced;              /* counters[0] behind the priced choice         */
  BlockSort<kKeyBins, kSortChunk, DJob, kMaxItems> sort;   /* + sort keys, sorted ids */
  DeviceBuf<int16_t> x16;          /* QM-scaled band vectors; grown on demand      */
  SideStreams streams;             /* kernels that may overlap                     */
  ProfEvents prof;                 /* odhip_pvq_profile                            */
  double tol_scale = 1.;           /* odhip_ctx_set_test_hooks */
};

int band_state(BandState **out) {
  ODHIP_CTX_OR_RETURN(ctx);
  BandState *st = odhip_ctx_state<BandState>(ctx, ODHIP_SLOT_BANDS);
  if (!st->tabs.d.p) {
    int rc = st->tabs.alloc();
    if (!rc) rc = st->sort.alloc();
    if (!rc) rc = st->counters.alloc();
    if (!rc) rc = st->plist.alloc(kPUncCap);
    if (rc) return rc;
  }
  st->streams.serial = ctx->serial != 0;
  st->tol_scale = ctx->price_tol_scale > 0 ? ctx->price_tol_scale : 1.;   /* test hook of the context */
  *out = st;
  return ODHIP_SUCCESS;
}
#define BAND_STATE_OR_RETURN(st) STAGE_STATE_OR_RETURN(BandState, band_state, st)

int fill_job(DJob &d, const odhip_pvq_job &j, JobMode mode) {
  const odhip_pvq_cands &c = j.cands;
  if (!j.d_coef || !c.band || !c.y || !c.choice) return ODHIP_EINVAL;
  if (((uintptr_t)c.band & 63) || ((uintptr_t)c.y & 15) || ((uintptr_t)c.choice & 15)) {
    return ODHIP_EINVAL;
  }
  if (mode == kJobBands ? !j.d_qm : mode == kJobSynth ? (!j.d_qm_inv || !j.d_dq) : false) return ODHIP_EINVAL;
  /* 16-byte loads of QM rows and of coefficient row segments */
  if (mode == kJobBands && (((uintptr_t)j.d_qm & 15) || ((uintptr_t)j.d_coef & 15))) return ODHIP_EINVAL;
  if (j.w & 3) return ODHIP_EINVAL;
  memset(&d, 0, sizeof(d));
  d.coef = j.d_coef;
  d.qm = j.d_qm;
  d.qm_inv = j.d_qm_inv;
  d.rec = c.band;
  d.y = c.y;
  d.choice = c.choice;
  d.cos_dist = c.cos_dist;
  d.dq = j.d_dq;
  d.rate = j.d_rate;
  d.qg_out = j.d_qg;
  /* block indices must fit 32 bits only where per-plane quantiser rows divide them */
  return fill_geometry(d, j, j.d_q_plane != nullptr);
}

int fill_jobs(const odhip_pvq_job *jobs, int njobs, JobMode mode, DJob *host) {
  if (!jobs || njobs <= 0 || njobs > kMaxJobs) return ODHIP_EINVAL;
  int rc = upload_tables();
  if (rc) return rc;
  for (int i = 0; i < njobs; i++) {
    rc = fill_job(host[i], jobs[i], mode);
    if (rc) return rc;
  }
  return ODHIP_SUCCESS;
}

/* fill_job zeroes every host job first: the table cache compares jobs by content (od_band_stage.cuh) */
int upload_jobs(BandState &st, DJob *host, int njobs, hipStream_t s) {
  for (int i = 0; i < njobs; i++) host[i].krange = st.counters.d.p + 1;
  return st.tabs.upload(host, njobs, s);
}

int stage_jobs(BandState &st, const odhip_pvq_job *jobs, int njobs, JobMode mode, DJob *host,
 hipStream_t s) {
  const int rc = fill_jobs(jobs, njobs, mode, host);
  if (rc) return rc;
  return upload_jobs(st, host, njobs, s);
}

void items_begin(Items &it, const BandState &st, double lambda) {
  memset(&it, 0, sizeof(it));
  it.lambda = lambda;
  it.jobs = st.tabs.cur;
  it.pcount = st.counters.d.p;
  it.plist = st.plist.p;
  it.tol_scale = st.tol_scale;
  it.force_seq = odhip_env_force_seq();
}

template <int N, int S>
void launch_search(BandState &st, const DJob *host, int njobs, double lambda, hipStream_t s) {
  Items it;
  items_begin(it, st, lambda);
  items_add_size(it, host, njobs, N, kWave/S);
  if (!it.nitems) return;
  constexpr size_t lds = kRsqN*sizeof(double) + (size_t)(N/S)*kPitch*4;
  const auto launch = [&] { k_search<N, S><<<it.wg_start[it.nitems], kWave, lds, s>>>(it); };
  /* odhip_pvq_profile times the dominant kernel of the band stage */
  if (N == 128) st.prof.around(s, launch);
  else launch();
}

}  // namespace

extern "C" int odhip_pvq_profile(int enable) {
  BAND_STATE_OR_RETURN(st);
  return st.prof.enable(enable);
}

extern "C" int odhip_pvq_profile_read(float *ms, int max_n) {
  BAND_STATE_OR_RETURN(st);
  return st.prof.read(ms, max_n);
}

extern "C" int odhip_pvq_band_layout(int bs, int *nb_bands, int *offsets, int *len) {
  if (bs < 0 || bs >= ODHIP_NBSIZES) return ODHIP_EINVAL;
  const int n = 4 << bs;
  if (nb_bands) *nb_bands = OD_NBANDS[bs];
  if (offsets) for (int i = 0; i <= OD_NBANDS[bs]; i++) offsets[i] = OD_BAND_OFFS[bs][i];
  if (len) *len = n*n < OD_SCAN_LEN ? n*n : OD_SCAN_LEN;
  return ODHIP_SUCCESS;
}

namespace {

int noref_bands(const odhip_pvq_job *jobs, int njobs, double pvq_norm_lambda, odhip_stream stream,
 bool fuse) {
  BAND_STATE_OR_RETURN(st);
  hipStream_t s = (hipStream_t)stream;
  const double lambda = pvq_norm_lambda;
  DJob host[kMaxJobs];
  int rc = fill_jobs(jobs, njobs, kJobBands, host);
  if (rc) return rc;
  if (fuse) ODHIP_TRY(hipMemsetAsync(st.counters.d.p, 0, sizeof(unsigned), s));
  size_t x16_elems = 0;
  for (int j = 0; j < njobs; j++) {
    x16_elems += (size_t)host[j].nblocks*host[j].len;
    for (int b = 0; b < host[j].nb_bands; b++) {
      const int n = host[j].off[b + 1] - host[j].off[b];
      if (n != 8 && n != 15 && n != 32 && n != 128) return ODHIP_EINVAL;
    }
  }
  if (!fuse) {
    /* scaled vectors, sort keys and sorted indices of the two-pass stage (the stage that decides in place
       keeps none of them) */
    rc = st.x16.grow(x16_elems, s);
    if (!rc) rc = st.sort.place(host, njobs, s);
    if (rc) return rc;
    x16_elems = 0;
    for (int j = 0; j < njobs; j++) {
      host[j].x16 = st.x16.p + x16_elems;
      x16_elems += (size_t)host[j].nblocks*host[j].len;
    }
  }
  rc = upload_jobs(st, host, njobs, s);
  if (rc) return rc;
  hipStream_t side[2] = {s, s};
  if (st.streams.fork(s, side) != ODHIP_SUCCESS) return ODHIP_EFAULT;
  Items it;
  if (fuse) {
    /* With the priced choice every band is prepared, searched and decided by the lanes that load it
       (k_decide_corner, k_decide_lane32, k_decide_pair128): no preparation pass, no sort, no scaled
       vectors or records in memory.  Four independent launches. */
    constexpr size_t lane_lds = kRsqN*sizeof(double) + (size_t)16*kPitch*4;
    constexpr size_t pair_lds = kRsqN*sizeof(double) + (size_t)64*kPitch*4;
    /* the 128-coefficient bands: a lane pair per band.  Round 5 measured a QUAD per band
       (k_decide_quad128: half the LDS per wavefront, three wavefronts per SIMD instead of two, every scan
       half as long) at 586 us against 550-568 for the pair on the same content: what the pair form lacks
       is not occupancy, and the quad pays a two-level combine per pulse.  The quad stays in the experiments
       build (ODHIP_PVQ_QUAD128=1), bit-identical. */
    const bool pair128 = ODHIP_EXP_ENV("ODHIP_PVQ_QUAD128") == nullptr;
    /* add() names the launch's items; odhip_pvq_profile times the one of the 128-coefficient bands */
    const auto decide = [&](hipStream_t on, bool timed, auto &&add, auto &&launch) {
      items_begin(it, st, lambda);
      add();
      items_heavy_first(it);
      const auto go = [&] {
        if (it.nitems) launch(it.wg_start[it.nitems], on);
      };
      if (timed) st.prof.around(on, go);
      else go();
    };
    decide(s, true, [&] { items_add_size(it, host, njobs, 128, pair128 ? kWave/2 : kWave/4); },
     [&](int grid, hipStream_t on) {
      if (pair128) k_decide_pair128<<<grid, kWave, pair_lds, on>>>(it);
#ifdef ODHIP_EXPERIMENTS
      else {
        constexpr size_t quad_lds = kRsqN*sizeof(double) + (size_t)32*kPitch*4;
        k_decide_quad128<<<grid, kWave, quad_lds, on>>>(it);
      }
#endif
    });
    decide(side[0], false, [&] { items_add_size(it, host, njobs, 32, kWave/2); },
     [&](int grid, hipStream_t on) { k_decide_lane32<<<grid, kWave, lane_lds, on>>>(it); });
    decide(side[1], false, [&] {
      for (int j = 0; j < njobs; j++) items_add(it, j, 0, (host[j].nblocks + kWave - 1)/kWave);
    }, [&](int grid, hipStream_t on) { k_decide_corner<0><<<grid, kWave, lane_lds, on>>>(it); });
    decide(side[1], false, [&] {
      for (int j = 0; j < njobs; j++) {
        if (host[j].bs > 0) items_add(it, j, 1, (host[j].nblocks + kWave - 1)/kWave);
      }
    }, [&](int grid, hipStream_t on) { k_decide_corner<1><<<grid, kWave, lane_lds, on>>>(it); });
    if (st.streams.join(s, side) != ODHIP_SUCCESS) return ODHIP_EFAULT;
    const int rc2 = st.priced.post(st.counters.d.p, s);
    if (rc2) return rc2;
    return odhip_check_launch();
  }
  /* prep: the low-frequency corner of every block one block per lane (bands
     0..3), the remaining 32-coefficient bands (4 and 5) one band per lane, the
     128-coefficient bands one per 16-lane row */
  items_begin(it, st, lambda);
  for (int j = 0; j < njobs; j++) {
    if (host[j].bs == 0) items_add(it, j, 0, (host[j].nblocks + kWave - 1)/kWave);
  }
  if (it.nitems) k_prep_corner<4><<<it.wg_start[it.nitems], kWave, 0, s>>>(it);
  items_begin(it, st, lambda);
  for (int j = 0; j < njobs; j++) {
    if (host[j].bs > 0) items_add(it, j, 0, (host[j].nblocks + kWave - 1)/kWave);
  }
  if (it.nitems) k_prep_corner<8><<<it.wg_start[it.nitems], kWave, 0, s>>>(it);
  items_begin(it, st, lambda);
  items_add_size(it, host, njobs, 32, kWave, 4);
  if (it.nitems) k_prep_lane<<<it.wg_start[it.nitems], kWave, 0, side[1]>>>(it);
  items_begin(it, st, lambda);
  items_add_size(it, host, njobs, 128, 4);
  if (it.nitems) k_prep_wide<<<it.wg_start[it.nitems], kWave, 0, side[0]>>>(it);
  if (st.streams.join(s, side) != ODHIP_SUCCESS) return ODHIP_EFAULT;
  /* counting sort of every item's blocks by pulse class */
  rc = st.sort.run(host, st.tabs.cur, njobs, s);
  if (rc) return rc;
  /* search: the band sizes are independent launches on forked streams */
  if (st.streams.fork(s, side) != ODHIP_SUCCESS) return ODHIP_EFAULT;
  launch_search<128, 2>(st, host, njobs, lambda, s);
  launch_search<32, 2>(st, host, njobs, lambda, side[0]);
  launch_search<15, 1>(st, host, njobs, lambda, side[1]);
  launch_search<8, 1>(st, host, njobs, lambda, side[1]);
  if (st.streams.join(s, side) != ODHIP_SUCCESS) return ODHIP_EFAULT;
  return odhip_check_launch();
}

}  // namespace

extern "C" int odhip_pvq_noref_bands_multi(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream) {
  return noref_bands(jobs, njobs, pvq_norm_lambda, stream, false);
}

/* The band stage AND the priced choice of odhip_pvq_choose_priced_multi in one pass: the
   search kernels decide each band from the values they hold in registers (no separate
   choice kernel reading the records back).  Follow with odhip_pvq_choose_priced_resolve. */
extern "C" int odhip_pvq_noref_bands_priced_multi(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream) {
  return noref_bands(jobs, njobs, pvq_norm_lambda, stream, true);
}

namespace {

/* The choice of every band from its two candidates' records: priced on the device (its close calls listed,
   their count on its way to the host) or by the records' rates; with kJobSynth the synthesis follows. */
int choose(const odhip_pvq_job *jobs, int njobs, double lambda, hipStream_t s, JobMode mode, bool price) {
  BAND_STATE_OR_RETURN(st);
  DJob host[kMaxJobs];
  int rc = stage_jobs(st, jobs, njobs, mode, host, s);
  if (rc) return rc;
  if (price) ODHIP_TRY(hipMemsetAsync(st.counters.d.p, 0, sizeof(unsigned), s));
  Items it;
  items_begin(it, st, lambda);
  for (int j = 0; j < njobs; j++) {
    items_add(it, j, 0, (host[j].nblocks*host[j].nb_bands + 255)/256);
  }
  if (!price) k_choose<0><<<it.wg_start[it.nitems], 256, 0, s>>>(it);
  else {
    k_choose<1><<<it.wg_start[it.nitems], 256, 0, s>>>(it);
    rc = st.priced.post(st.counters.d.p, s);
    if (rc) return rc;
  }
  if (mode == kJobSynth) {
    items_begin(it, st, lambda);
    for (int j = 0; j < njobs; j++) {
      items_add(it, j, 0, (long)host[j].nplanes*host[j].h*((host[j].w + 1023) >> 10));
    }
    k_synth<<<it.wg_start[it.nitems], 256, 0, s>>>(it);
  }
  return odhip_check_launch();
}

}  // namespace

extern "C" int odhip_pvq_select_synth_noref_multi(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream) {
  return choose(jobs, njobs, pvq_norm_lambda, (hipStream_t)stream, kJobSynth, false);
}

extern "C" int odhip_pvq_choose_multi(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream) {
  return choose(jobs, njobs, pvq_norm_lambda, (hipStream_t)stream, kJobChoice, false);
}

/* The choice with od_pvq_rate's closed form evaluated on the device (see choose_band). */
extern "C" int odhip_pvq_choose_priced_multi(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream) {
  return choose(jobs, njobs, pvq_norm_lambda, (hipStream_t)stream, kJobChoice, true);
}

/* Waits for the stream, then settles the bands odhip_pvq_choose_priced_multi listed:
   their candidates' rates are recomputed with the HOST libm's log (src/pvq_encoder.c:263,
   the call the reference makes) and the bands decided again.  Returns how many (normally
   0), or a negative code.  Pass the same jobs. */
extern "C" int odhip_pvq_choose_priced_resolve(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream) {
  BAND_STATE_OR_RETURN(st);
  hipStream_t s = (hipStream_t)stream;
  /* normal case: only the count is waited for (it was sent right behind the choice) */
  const int posted = st.priced.wait();
  if (posted <= 0) return posted;
  std::vector<PUnc> list;
  const int count = take_listed(s, st.counters.d.p, st.plist.p, kPUncCap, "priced bands inside the decision margin",
   list);
  if (count <= 0) return count;
  DJob host[kMaxJobs];
  int rc = stage_jobs(st, jobs, njobs, kJobChoice, host, s);
  if (rc) return rc;
  if (!listed_jobs_valid(list.data(), count, njobs)) return ODHIP_EINVAL;
  for (PUnc &e : list) {
    const DJob &jb = host[e.job];
    const int band = (int)(e.sb % jb.nb_bands);
    const int n = jb.off[band + 1] - jb.off[band];
    odhip_pvq_band rec;
    ODHIP_TRY(hipMemcpy(&rec, jb.rec + e.sb, sizeof(rec), hipMemcpyDeviceToHost));
    for (int c = 0; c < 2; c++) {
      e.rate[c] = 0;
      if (rec.flags[c] != 1) continue;
      e.rate[c] = odq_pvq_rate_fast_host(rec.moment[c], rec.k[c], n, rec.gain[c], 0, -1, 0, 1, 0);
    }
  }
  DeviceBuf<PUnc> d_list;
  if (upload_list(d_list, list.data(), count)) return ODHIP_EFAULT;
  Items it;
  items_begin(it, st, pvq_norm_lambda);
  k_choose_list<<<(count + kWave - 1)/kWave, kWave, 0, s>>>(it, d_list.p, (int)count);
  rc = odhip_check_launch();
  if (hipStreamSynchronize(s) != hipSuccess) rc = ODHIP_EFAULT;
  return rc ? rc : count;
}

extern "C" int odhip_cfl_refs_from_luma(const odhip_pvq_job *luma_jobs, int njobs,
 od_coeff *const *d_ref, int copies, odhip_stream stream) {
  return odhip_cfl_refs_from_luma_ex(luma_jobs, njobs, d_ref, copies, 0, stream);
}

extern "C" int odhip_cfl_refs_from_luma_ex(const odhip_pvq_job *luma_jobs, int njobs,
 od_coeff *const *d_ref, int copies, int prezeroed, odhip_stream stream) {
  BAND_STATE_OR_RETURN(st);
  hipStream_t s = (hipStream_t)stream;
  if (!d_ref || copies < 1 || copies > 4) return ODHIP_EINVAL;
  DJob host[kMaxJobs];
  int rc = fill_jobs(luma_jobs, njobs, kJobChoice, host);
  if (rc) return rc;
  rc = upload_jobs(st, host, njobs, s);     /* before items_begin: it selects the table */
  if (rc) return rc;
  CflOut out;
  memset(&out, 0, sizeof(out));
  out.copies = copies;
  Items it;
  items_begin(it, st, 0.);
  for (int j = 0; j < njobs; j++) {
    if (!d_ref[j] || !luma_jobs[j].d_qm_inv || (host[j].w & 7) || (host[j].h & 7)) return ODHIP_EINVAL;
    out.ref[j] = d_ref[j];
    if (host[j].bs >= 1) {
      const int n = 2 << host[j].bs;
      const int ncode = n*n < host[j].len ? n*n : host[j].len;
      items_add(it, j, 0, (host[j].nblocks*(ncode >> 3) + 255)/256);
      if (n*n > ncode && !prezeroed) {
        /* 64x64 luma blocks: half of the 32x32 corner is not coded */
        ODHIP_TRY(hipMemsetAsync(d_ref[j], 0, sizeof(od_coeff)*(size_t)copies*host[j].nplanes
         *(host[j].w >> 1)*(host[j].h >> 1), s));
      }
    }
  }
  if (it.nitems) k_cfl_ref<<<it.wg_start[it.nitems], 256, 0, s>>>(it, out);
  /* level-0 jobs: the TF branch */
  items_begin(it, st, 0.);
  for (int j = 0; j < njobs; j++) {
    if (host[j].bs == 0) {
      items_add(it, j, 0, ((long)host[j].nplanes*(host[j].w >> 1)*(host[j].h >> 1) + 255)/256);
    }
  }
  if (it.nitems) k_cfl_ref_tf<<<it.wg_start[it.nitems], 256, 0, s>>>(it, out);
  return odhip_check_launch();
}

extern "C" int odhip_pvq_noref_bands(const od_coeff *d_coef, int nplanes, int w, int h,
 int bs, const int16_t *d_qm, const int32_t *q_band, const int32_t *beta_band,
 double pvq_norm_lambda, const odhip_pvq_cands *out, odhip_stream stream) {
  if (!out) return ODHIP_EINVAL;
  odhip_pvq_job j;
  memset(&j, 0, sizeof(j));
  j.d_coef = d_coef;
  j.nplanes = nplanes;
  j.w = w;
  j.h = h;
  j.bs = bs;
  j.d_qm = d_qm;
  j.q_band = q_band;
  j.beta_band = beta_band;
  j.cands = *out;
  return odhip_pvq_noref_bands_multi(&j, 1, pvq_norm_lambda, stream);
}

extern "C" int odhip_pvq_select_synth_noref(od_coeff *d_dq, const od_coeff *d_coef,
 int nplanes, int w, int h, int bs, const int16_t *d_qm_inv, const int32_t *q_band,
 const int32_t *beta_band, double pvq_norm_lambda, const odhip_pvq_cands *in,
 const double *d_rate, int32_t *d_qg_out, odhip_stream stream) {
  if (!in) return ODHIP_EINVAL;
  odhip_pvq_job j;
  memset(&j, 0, sizeof(j));
  j.d_coef = d_coef;
  j.nplanes = nplanes;
  j.w = w;
  j.h = h;
  j.bs = bs;
  j.d_qm_inv = d_qm_inv;
  j.q_band = q_band;
  j.beta_band = beta_band;
  j.cands = *in;
  j.d_dq = d_dq;
  j.d_rate = d_rate;
  j.d_qg = d_qg_out;
  return odhip_pvq_select_synth_noref_multi(&j, 1, pvq_norm_lambda, stream);
}

/* od_krange.cuh: the current context's count since the last call, then cleared (blocking copies: the stream of the band
   stage must have been synchronised) */
int od_k_range_take_noref(unsigned *count) {
  BAND_STATE_OR_RETURN(st);
  return st.counters.take(1, count);
}
