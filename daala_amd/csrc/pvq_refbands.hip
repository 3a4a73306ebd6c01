/* pvq_refbands.hip - pvq_theta WITH a reference (reference
   src/pvq_encoder.c:333-641: keyframe chroma predicted from luma, inter frames)
   for every block and band of a batch of coefficient planes, up to the
   rate-dependent choice, and the choice + synthesis that follows it.

     k_refb_prep_*      per band: chroma-from-luma sign flip of the block
                        (od_pvq_encode, :846-872), gather of x and r in coding
                        order (od_raster_to_coding_order, src/partition.c:144),
                        QM scaling, gains, correlation, initial distortion
                        (:381-455), od_compute_householder / od_apply_householder
                        (src/pvq.c:498-623), theta = floor(.5 + OD_THETA_SCALE *
                        acos(corr)) (:478) with the DEVICE acos and the
                        uncertainty test described in include/daala_hip.h
     k_refb_cands       the (gain, theta) candidates in the reference's stable
                        (k, gain) order (:466-504) followed by the no-reference
                        candidates (:571-581)
     k_refb_search      one band per lane: the candidate loop (:506-565) - pruning,
                        K-pulse searches on the reflected vector chained through
                        prev_k, distortions - then the no-reference loop
                        (:578-595)
     k_refb_choose      `cost < best_cost` / `cost <= best_cost` (:553, :600),
                        skip rules (:611-622), od_gain_expand and the band-wide
                        part of od_pvq_synthesis_partial (:623-633,
                        src/pvq.c:1037-1115)
     k_refb_synth       its per-coefficient part and od_coding_order_to_raster

   The libm call of the path: the reference's theta comes from glibc's acos.
   Everything downstream depends only on the INTEGER theta, so the device value
   is the reference's whenever OD_THETA_SCALE*acos(corr) + .5 is not within the
   margin (1e-9, 30x the worst disagreement of two <= 2-ulp implementations at
   this magnitude) of an integer; the bands inside the margin are listed and
   odhip_pvq_ref_resolve recomputes their theta on the host with the very libm
   the reference calls, re-running a band when it differs.

   Mappings: 15- and 8-coefficient bands one band per lane, 32- and
   128-coefficient bands one band per quad / 16-lane DPP row (pvq_row.cuh); in the
   decided stage the 32-coefficient bands one per lane PAIR and the 128-coefficient ones
   one per lane QUAD (pvq_lane.cuh).  The per-lane
   searches are not yet sorted by pulse count.  All double arithmetic
   is one IEEE operation per reference operation (-ffp-contract=off). */
#include "../../include/daala_hip.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "od_ctx.cuh"
#include "od_pvq_math.cuh"
#include "od_pvq_synth.cuh"
#include "od_occupancy.cuh"
#include "od_krange.cuh"
#include "od_band_stage.cuh"
#include "gen/od_scan_tables.h"
#define OD_RSQ_TABLE_N 512
#define OD_RSQ_HUGE
#include "pvq_search.cuh"
#include "pvq_row.cuh"
#include "pvq_regs.cuh"
#include "pvq_lane.cuh"

namespace {

/* All state between calls (device job table, uncertainty list, sort arrays, scratch,
   side streams, pinned counter) belongs to the calling thread's current context
   (od_ctx.cuh): independent call sequences (e.g. the Cb and the Cr planes of a
   batch on two streams) run in two contexts. */
constexpr int kMaxJobs = 8;
constexpr int kMaxItems = kMaxJobs*ODHIP_MAX_BANDS;
constexpr int kSlots = ODHIP_PVQ_REF_SLOTS;
constexpr int kUncCap = 1 << 16;
constexpr double kDefaultMargin = 1e-9;

struct RJob {
  const od_coeff *coef;
  const od_coeff *ref;
  const int16_t *qm;
  const int16_t *qm_inv;
  odhip_pvq_refband *rec;
  void *items;
  int16_t *y;
  int16_t *r16;
  int16_t *x16;
  int16_t *xr;
  const double *rate;
  int32_t *choice;
  od_coeff *dq;
  /* library scratch of the sorted searches */
  unsigned short *keys;   /* [nb][B] work class of the band (heavy = small)       */
  unsigned *ids;          /* [nb][B] block indices sorted by key                  */
  unsigned *krange;       /* od_krange.cuh: the calling context's counter          */
  long nblocks;
  int nplanes;
  int w;
  int h;
  int bs;
  int nb_bands;
  int len;
  int bw;
  int bh;
  int is_keyframe;
  int pli;
  int q[ODHIP_MAX_BANDS];
  int beta[ODHIP_MAX_BANDS];
  int off[ODHIP_MAX_BANDS + 1];
  /* planes from plane_split on (blocks from split_blk on) take q2: the Cr half of a
     chroma plane set - pvq_qm_q4[pli] is per plane, src/encode.c:3052-3072 */
  long split_blk;
  int q2[ODHIP_MAX_BANDS];
  /* odhip_pvq_refjob.d_q_plane: every plane its own row of band steps (plane_blocks blocks per
     plane); q and q2 are then 0 (a step is at least 1), so that the lookup costs the kernels
     nothing but a compare while they are NULL */
  const int *qp;
  unsigned plane_blocks;
  /* chroma-from-luma reference taken straight from the luma band stage (odhip_pvq_refjob.luma):
     the chosen pulses / choice records / inverse QM of the luma level one size up (4:4:4: the
     same level); the reference plane itself never exists */
  const int16_t *ly;
  const int32_t *lchoice;
  const int16_t *lqmi;
  long lnblocks;
  long lsplit;      /* blocks of one luma plane set: chroma plane p uses luma plane p mod planes */
  int llen;
  int lnb;
};

/* The band's quantiser step for block blk: the row of its plane, or the Cb / Cr split. */
__device__ __forceinline__ int job_q(const RJob &jb, int band, long blk) {
  const int q = blk >= jb.split_blk ? jb.q2[band] : jb.q[band];
  return q ? q : jb.qp[(unsigned)blk/jb.plane_blocks*ODHIP_MAX_BANDS + band];
}

/* od_resample_luma_coeffs for luma blocks of 8x8 and larger (src/intra.c:97-108: the
   upper-left quarter of the decoded luma block; 4:4:4, :95-108 without decimation: the whole
   decoded luma block of the same level) for the eight coding positions c0 .. c0 + 7
   of chroma block blk, band `band`: the scan is nested (the first n*n coding positions of a
   2n x 2n block are its n x n corner, and the band offsets coincide), so they are coding
   positions c0 .. c0 + 7 of the same band of the co-located luma block, dequantised from its
   chosen pulses exactly as od_pvq_synthesis_partial without reference writes them
   (src/pvq.c:1081-1092).  Position 0 (the DC slot, never used by PVQ) comes out as 0.
   The arithmetic apart from the loads (the luma block's choice record of the band: sel, qg,
   scale, qshift; its chosen pulses), so that a lane can issue the loads of several pieces
   before it uses one. */
__device__ __forceinline__ long lref_block(const RJob &jb, long blk) {
  return blk >= jb.lsplit ? blk - jb.lsplit : blk;
}

/* od_noref_chunk8 (od_pvq_synth.cuh) with the product by the inverse QM kept in 64 bits: the same values
   on the synthesis's domain, and the text the preparation kernels had (profiles/synth_once.txt). */
__device__ __forceinline__ void lref_dequant(const int4 &ch, const uint4 &y4, const uint4 &q4, int (&rv)[8]) {
  const unsigned yw[4] = {y4.x, y4.y, y4.z, y4.w};
  const unsigned qw[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const int yv = (int16_t)(yw[e >> 1] >> (16*(e & 1)));
    const int qmi = (int16_t)(qw[e >> 1] >> (16*(e & 1)));
    rv[e] = odq_shr_round(odq_mult16_32_q16(yv, ch.z)*qmi, ch.w);
  }
}

__device__ __forceinline__ void lref_piece(const RJob &jb, int band, long blk, int c0, int (&rv)[8]) {
  const long lblk = lref_block(jb, blk);
  const int4 ch = reinterpret_cast<const int4 *>(jb.lchoice)[lblk*jb.lnb + band];
  uint4 y4 = make_uint4(0, 0, 0, 0);
  if (ch.y != 0) y4 = *reinterpret_cast<const uint4 *>(jb.ly + ((long)ch.x*jb.lnblocks + lblk)*jb.llen + c0);
  lref_dequant(ch, y4, *reinterpret_cast<const uint4 *>(jb.lqmi + c0), rv);
}

struct Unc;
/* What the decided stage hands from its preparation to its searches, in the library's own buffer
   (RefState::lean_rec) instead of the job's 64-byte odhip_pvq_refband: the fields those searches read and
   nothing else, 32 bytes.  icgr and gain_offset are the two halves of cgr (prep_scalars). */
struct LeanRec {
  int32_t cg;
  int32_t cgr;
  int32_t theta;
  uint32_t msf;            /* m | (uint8_t)s << 16 | flags << 24 */
  double corr;
  double dist0;
};
static_assert(sizeof(LeanRec) == 32, "two records to a 64-byte line");

/* A LeanRec as a search holds it, under the names odhip_pvq_refband gives the same values (m and s are read
   again where refb_finish needs them: held across the walk they spill). */
struct LeanVals {
  int32_t cg;
  int32_t gain_offset;
  int32_t icgr;
  int32_t theta;
  int flags;
  double corr;
  double dist0;
};

__device__ __forceinline__ uint32_t lean_msf(int m, int s, int flags) {
  return (uint32_t)(uint16_t)m | (uint32_t)(uint8_t)s << 16 | (uint32_t)flags << 24;
}

__device__ __forceinline__ LeanVals lean_vals(const LeanRec &m) {
  LeanVals r;
  r.cg = m.cg;
  r.icgr = odq_shr_round(m.cgr, ODQ_CGAIN_SHIFT);
  r.gain_offset = m.cgr - odq_shl32(r.icgr, ODQ_CGAIN_SHIFT);
  r.theta = m.theta;
  r.flags = (int)(m.msf >> 24);
  r.corr = m.corr;
  r.dist0 = m.dist0;
  return r;
}

/* A band whose priced choice the host (re)decides: rate[0] = the initial candidate,
   rate[1 + i] = candidate i, from the host libm. */
struct PUncR {
  int job;
  int band;
  unsigned blk;
  int reserved;
  double rate[ODHIP_PVQ_REF_SLOTS + 1];
};
constexpr int kPUncCap = 1 << 14;

struct RItems : ItemTable<kMaxItems> {
  int perturb;
  double lambda;
  double margin;
  const RJob *jobs;        /* the context's device job table [kMaxJobs]            */
  unsigned *unc_count;     /* its uncertainty list: counter ...                    */
  Unc *unc;                /* ... and entries [kUncCap]                            */
  unsigned *pcount;        /* priced choice: bands too close to call on the device; pcount[1]: bands with a
                              candidate above ODHIP_PVQ_MAX_K (od_krange.cuh), cleared only when taken */
  struct PUncR *plist;     /* ... and their list [kPUncCap]                        */
  double tol_scale;        /* test hook: multiplies the decision margin            */
  int fuse;                /* the per-lane searches also make the priced choice    */
  int sort_weights;        /* weights of the work class, packed (sort_weights())   */
#ifdef ODHIP_EXPERIMENTS
  int abl;                 /* ODHIP_REFB_ABL: ablation bits (tools/gpu_r6_ablate.sh)  */
#endif
  /* the decided stage's records: job j's at lean + lean_at[j], indexed like its rec (blk*nb_bands + band) */
  LeanRec *lean;
  long lean_at[kMaxJobs];
};

__device__ __forceinline__ LeanRec *lean_rec(const RItems &it, int job, const RJob &jb, long blk, int band) {
  return it.lean + (it.lean_at[job] + blk*jb.nb_bands + band);
}

/* The flip of a block as its band 0 recorded it: in the job's record, or (the decided stage) in the lean one. */
__device__ __forceinline__ int block_flip(const RItems &it, int job, const RJob &jb, long blk, bool lean) {
  const int flags = lean ? (int)(lean_rec(it, job, jb, blk, 0)->msf >> 24) : jb.rec[blk*jb.nb_bands].flags;
  return (flags & ODHIP_REFBAND_FLIP) != 0;
}

/* One band whose theta lies inside the margin (written by k_refb_prep) or has
   to be re-run with the host's theta (read by the *_list kernels). */
struct Unc {
  int job;
  int band;
  unsigned blk;
  int theta;
  double corr;
};

__constant__ unsigned char kRScanXY[OD_SCAN_LEN][2];

/* Offset of block blk inside its plane set. */
__device__ __forceinline__ long block_base(const RJob &j, long blk) {
  const int N = 4 << j.bs;
  const long per = (long)j.bw*j.bh;
  const int p = (int)(blk/per);
  const int rem = (int)(blk - p*per);
  const int by = rem/j.bw;
  const int bx = rem - by*j.bw;
  return (long)p*j.w*j.h + (long)by*N*j.w + bx*N;
}

__device__ __forceinline__ long coef_pos(const RJob &j, int c) {
  return (long)kRScanXY[c][1]*j.w + kRScanXY[c][0];
}

constexpr double kPi = 3.14159265358979323846;       /* M_PI */
constexpr double kThetaScale = 32768*2./kPi;         /* OD_THETA_SCALE, src/pvq.h:78 */

/* .5 + OD_THETA_SCALE*acos(corr): the argument of the floor at
   src/pvq_encoder.c:478 (OD_ROUND32, src/odintrin.h:169). */
__device__ __forceinline__ double theta_arg(double corr) {
  return .5 + kThetaScale*acos(corr);
}

__global__ __launch_bounds__(kWave) void k_theta_probe(const double *corr, double *t, long n) {
  const long i = (long)blockIdx.x*kWave + threadIdx.x;
  if (i < n) t[i] = theta_arg(corr[i]);
}

/* ---- preparation -------------------------------------------------------------------
   Two mappings: the 15- and 8-coefficient bands one band per lane with the band
   in registers - a lane takes band 0 of a block and, for blocks of 8x8 and up,
   its bands 1 and 2, whose segments share lines with band 0's
   (k_refb_prep_corner) -, the 32- and 128-coefficient bands one band per
   16-lane row (k_refb_prep_row; a frame batch has too few of them to fill the
   chip one per lane, and a lane walking 128 coefficients three times is a chain
   of exposed latencies).  Band 0 decides the chroma-from-luma flip of its block;
   the row kernels, launched behind it, read it from band 0's record.  Sums of integers are accumulated in any order (exact); the
   Householder pivot is the first largest |r| (src/pvq.c:505-512; |r16| < 2^15
   by construction of rshift, so the int16 running maximum of the reference
   cannot wrap). */
__device__ __attribute__((aligned(16))) unsigned short gRScanPk[OD_SCAN_LEN];   /* y << 8 | x */

struct PrepScalars {
  int32_t g, gr, cg, cgr, gain_offset;
  int icgr;
  double corr, dist0;
  bool ran;
};

/* :404-455 from the band sums. */
__device__ __forceinline__ PrepScalars prep_scalars(int accx, int accr, double corr_sum, int xshift,
 int rshift, int q0, int beta, int cfl_enabled, int is_keyframe, int r_null) {
  PrepScalars o;
  o.cg = odq_gain_from_acc(accx, q0, beta, xshift, &o.g);
  o.cgr = odq_gain_from_acc(accr, q0, beta, rshift, &o.gr);
  if (cfl_enabled) o.cgr = 256;
  o.icgr = odq_shr_round(o.cgr, ODQ_CGAIN_SHIFT);
  o.gain_offset = o.cgr - odq_shl32(o.icgr, ODQ_CGAIN_SHIFT);
  double corr = __ddiv_rn(corr_sum,
   1e-100 + __ddiv_rn(o.g*(double)o.gr, (double)odq_shl32(1, xshift + rshift)));
  corr = corr < 1. ? corr : 1.;
  corr = corr > -1. ? corr : -1.;
  o.corr = corr;
  const double s2 = (1./256)*(1./256);
  double dist0 = ((1.4*o.cg)*o.cg)*s2;
  if (!is_keyframe && o.icgr == 0) {
    const int32_t scgr = o.gain_offset > 0 ? o.gain_offset : 0;
    dist0 = (1.4*(o.cg - scgr))*(o.cg - scgr) + (scgr*(double)o.cg)*(2 - 2*corr);
    dist0 *= s2;
  }
  o.dist0 = dist0;
  o.ran = !r_null && corr > 0;
  return o;
}

/* ---- sorting the bands of an item by work -----------------------------------------
   The cost of a band is the number of pulses its chains place, which spans
   0..hundreds within one level, and a wavefront (64 bands, or 4 rows) runs as
   long as its slowest member.  Every band is classified (kSortBins classes, heavy
   first); a counting sort per (job, band) item - LDS histogram per chunk of blocks,
   one global atomic per non-empty class per chunk (od_band_stage.cuh) - yields the
   block order the searches walk. */
constexpr int kSortBins = 256;
constexpr int kSortChunk = 2048;

__device__ __forceinline__ int od_work_bin(int pulses) {   /* 0..kSortBins-1, monotone */
  if (pulses < 96) return pulses;
  const int b = 96 + ((pulses - 96) >> 3);
  return b < kSortBins ? b : kSortBins - 1;
}

/* Whether a band has no-reference candidates (src/pvq_encoder.c:571-581): the bands whose search reads x16. */
__device__ __forceinline__ bool refb_has_noref(const RJob &jb, int32_t cg, double corr) {
  return (jb.is_keyframe && jb.pli == 0) || corr < .5 || cg < odq_shl32(2, ODQ_CGAIN_SHIFT);
}

/* The candidates of a band in the reference's ENUMERATION order (src/pvq_encoder.c:466-504,
   then :571-581), handed to a sink:
     sink.gain(gi, i, ts, lower)   gain index i = gain_bound - 1 + gi (gi = 0..2) is about to
                                   be enumerated: its angular resolution and first angle
     sink.theta(gi, i, j, ts, k)   one (gain, theta) candidate with its pulse count
     sink.noref(c, i, k)           no-reference candidate c = 0 / 1
   At most kSlots - 2 theta candidates, as refb_candidates keeps. */
template <class Sink>
__device__ __forceinline__ void refb_enumerate(const RJob &jb, int band, int32_t cg, int32_t gain_offset,
 int32_t theta, int flags, double corr, Sink &sink) {
  const int n = jb.off[band + 1] - jb.off[band];
  const int beta = jb.beta[band];
  if (flags & ODHIP_REFBAND_THETA) {
    int nth = 0;
    const int gain_bound = (cg - gain_offset) >> ODQ_CGAIN_SHIFT;
    const double scale_1 = __ddiv_rn(1., kThetaScale);   /* OD_THETA_SCALE_1 */
    for (int i = gain_bound - 1 > 1 ? gain_bound - 1 : 1; i <= gain_bound + 1; i++) {
      const int32_t qcg = odq_shl32(i, ODQ_CGAIN_SHIFT) + gain_offset;
      const int ts = odq_pvq_compute_max_theta(qcg, beta);
      /* same left-to-right products as src/pvq_encoder.c:482-484 */
      const double t = __ddiv_rn(((theta*scale_1)*2), kPi)*ts;
      int lower = (int)floor(.5 + t) - 2;
      if (lower < 0) lower = 0;
      int upper = (int)ceil(t);
      if (upper > ts - 1) upper = ts - 1;
      const int gi = i - (gain_bound - 1);
      sink.gain(gi, i, ts, lower);
      for (int j = lower; j <= upper && nth < ODHIP_PVQ_REF_SLOTS - 2; j++) {
        sink.theta(gi, i, j, ts, odq_compute_k_ref(j, n));
        nth++;
      }
    }
  }
  if (refb_has_noref(jb, cg, corr)) {
    const int gain_bound = cg >> ODQ_CGAIN_SHIFT;
    int c = 0;
    for (int i = gain_bound > 1 ? gain_bound : 1; i <= gain_bound + 1; i++) {
      sink.noref(c++, i, odq_compute_k_noref(odq_shl32(i, ODQ_CGAIN_SHIFT), n, beta));
    }
  }
}

/* The work class of a band.  Its chains place about kmax pulses (~240 instructions each for a
   15-coefficient band), but most bands place 0-3 pulses and their cost is the candidates themselves
   (~300 instructions each) and the searches (~400 each beside their pulses): round 4 measured 0.56 of
   the lanes active in k_refb_lean_lane<15> with the pulses alone as the key
   (SQ_THREAD_CYCLES_VALU / SQ_ACTIVE_INST_VALU, tools/gpu_r4_lanes.sh), so the class is
   pulses + candidates + 2 * distinct pulse counts (one search each). */
struct KeySink {
  int kt = 0;
  int kn = 0;
  int c = 0;
  unsigned long long mt = 0;
  unsigned long long mn = 0;
  __device__ __forceinline__ void gain(int, int, int, int) {}
  __device__ __forceinline__ void theta(int, int, int, int, int k) {
    kt = k > kt ? k : kt;
    c++;
    if (k) mt |= 1ull << (k & 63);
  }
  __device__ __forceinline__ void noref(int, int, int k) {
    kn = k > kn ? k : kn;
    c++;
    if (k) mn |= 1ull << (k & 63);
  }
  /* w: weights in quarters, pulses | candidates << 8 | searches << 16 */
  __device__ __forceinline__ int work(int w) const {
    return ((w & 255)*(kt + kn) + (w >> 8 & 255)*c + (w >> 16 & 255)*(__popcll(mt) + __popcll(mn))) >> 2;
  }
};

/* Record of the band, theta with the device acos and the uncertainty list
   (one lane per band). */
__device__ __forceinline__ void prep_write(const RItems &it, const RJob &jb, odhip_pvq_refband *rec, int job, int band,
 long blk, int xshift, int rshift, const PrepScalars &p, int r_null, int flip, int m, int s) {
  int flags = (r_null ? ODHIP_REFBAND_R_NULL : 0) | (flip ? ODHIP_REFBAND_FLIP : 0);
  int32_t theta = 0;
  if (p.ran) {
    flags |= ODHIP_REFBAND_THETA;
    const double u = theta_arg(p.corr);
    theta = (int32_t)floor(u);
    if (fabs(u - rint(u)) < it.margin) {
      flags |= ODHIP_REFBAND_UNCERTAIN;
      if (it.perturb & 1) theta += 1;
      const unsigned slot = atomicAdd(it.unc_count, 1u);
      if (slot < (unsigned)kUncCap) {
        Unc e;
        e.job = job;
        e.band = band;
        e.blk = (unsigned)blk;
        e.theta = theta;
        e.corr = p.corr;
        it.unc[slot] = e;
      }
    }
  }
  if (it.fuse == 2) {
    /* the decided stage: its own record; the job's rec is not written */
    LeanRec o;
    o.cg = p.cg;
    o.cgr = p.cgr;
    o.theta = theta;
    o.msf = lean_msf(m, s, flags);
    o.corr = p.corr;
    o.dist0 = p.dist0;
    *lean_rec(it, job, jb, blk, band) = o;
    /* it has no candidate kernel: the work class comes from here */
    KeySink ks;
    refb_enumerate(jb, band, p.cg, p.gain_offset, theta, flags, p.corr, ks);
    jb.keys[(long)band*jb.nblocks + blk] = (unsigned short)(kSortBins - 1 - od_work_bin(ks.work(it.sort_weights)));
    /* a candidate of this band's list has more pulses than the pulse vectors hold: the searches skip it
       (conservative: counted even when the reference's own pruning test would have dropped it) */
    if (ks.kt > ODHIP_PVQ_MAX_K || ks.kn > ODHIP_PVQ_MAX_K) atomicAdd(jb.krange, 1u);
    return;
  }
  odhip_pvq_refband o;
  o.xshift = xshift;
  o.rshift = rshift;
  o.g = p.g;
  o.gr = p.gr;
  o.cg = p.cg;
  o.cgr = p.cgr;
  o.icgr = p.icgr;
  o.gain_offset = p.gain_offset;
  o.m = (int16_t)m;
  o.s = (int8_t)s;
  o.flags = (uint8_t)flags;
  o.theta = theta;
  o.nitems = 0;
  o.ntheta = 0;
  o.corr = p.corr;
  o.dist0 = p.dist0;
  *rec = o;
}

__device__ __forceinline__ uint32_t pack16(int lo, int hi) {
  return (uint32_t)(lo & 0xffff) | (uint32_t)hi << 16;
}

/* E signed pulses y(0) .. y(E - 1) to dst as whole 16-byte pieces.  The 15-coefficient band shares its
   first piece with the unused DC slot in front of it, which is written 0. */
template <int E, class YGet>
__device__ __forceinline__ void store_pulses(int16_t *dst, YGet y) {
  constexpr int SH = E == 15 ? 1 : 0;
  static_assert((E + SH) % 8 == 0, "whole 16-byte pieces");
  uint4 *p = reinterpret_cast<uint4 *>(dst - SH);
  int t[E + SH];
  if (SH) t[0] = 0;
#pragma unroll
  for (int i = 0; i < E; i++) t[i + SH] = y(i);
#pragma unroll
  for (int q = 0; q < (E + SH)/8; q++) {
    p[q] = make_uint4(pack16(t[8*q], t[8*q + 1]), pack16(t[8*q + 2], t[8*q + 3]),
     pack16(t[8*q + 4], t[8*q + 5]), pack16(t[8*q + 6], t[8*q + 7]));
  }
}

/* The per-lane bands arrive as row segments and are permuted to coding order through the
   compile-time scan: band 0 is the 4x4 low-frequency corner without the DC (four 16-byte
   segments; adjacent lanes = adjacent blocks: contiguous for 4x4 blocks), band 1 columns 4..7
   of rows 0 and 1 (two 16-byte segments), band 2 columns 0..1 of rows 4..7 (four 8-byte
   segments).  No other band has 8 coefficients: */
constexpr bool lane_band_layout_ok() {
  for (int bs = 0; bs < 5; bs++) {
    const int nb = OD_NBANDS[bs];
    if (OD_BAND_OFFS[bs][0] != 1 || OD_BAND_OFFS[bs][1] != 16 || (nb > 1 && nb < 3)) return false;
    for (int b = 1; b < nb; b++) {
      const bool lane = OD_BAND_OFFS[bs][b + 1] - OD_BAND_OFFS[bs][b] == 8;
      if (lane != (OD_BAND_OFFS[bs][b] == 8 + 8*b && b <= 2)) return false;
    }
  }
  return true;
}
static_assert(lane_band_layout_ok(), "k_refb_prep_corner: band 0 at 1..15, 8-coefficient bands at 16 and 24 only");

struct CornerSegs {
  int4 b0[4];
  int4 b1[2];
  int2 b2[4];
};

/* A pointer read from the job table is a generic one to the compiler: its loads are flat loads, whose
   completion cannot be counted, so the first use of any of them waits for all.  The job's buffers are
   device memory: as global loads, the loads of a lane complete in order and each use waits for its own. */
typedef int od_int4v __attribute__((ext_vector_type(4)));
typedef int od_int2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int4 global_load4(const void *p) {
  const od_int4v v = *(const __attribute__((address_space(1))) od_int4v *)p;
  return make_int4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ int2 global_load2(const void *p) {
  const od_int2v v = *(const __attribute__((address_space(1))) od_int2v *)p;
  return make_int2(v.x, v.y);
}

/* The QM tables are the same for every lane and never written by a kernel: constant memory, scalar loads. */
typedef const __attribute__((address_space(4))) int16_t *od_const_i16;

__device__ __forceinline__ od_const_i16 const_table(const int16_t *p) {
  return (od_const_i16)p;
}

__device__ __forceinline__ uint4 const_load4(const int16_t *p) {
  const od_int4v v = *(const __attribute__((address_space(4))) od_int4v *)p;
  return make_uint4((unsigned)v.x, (unsigned)v.y, (unsigned)v.z, (unsigned)v.w);
}

/* The segments of one block; bands 1 and 2 only where the block has them. */
__device__ __forceinline__ void corner_load(const od_coeff *p, int w, bool more, CornerSegs &s) {
#pragma unroll
  for (int y = 0; y < 4; y++) s.b0[y] = global_load4(p + (long)y*w);
#pragma unroll
  for (int y = 0; y < 2; y++) s.b1[y] = more ? global_load4(p + (long)y*w + 4) : make_int4(0, 0, 0, 0);
#pragma unroll
  for (int y = 0; y < 4; y++) s.b2[y] = more ? global_load2(p + (long)(4 + y)*w) : make_int2(0, 0);
}

/* The luma stage's choice record of a band, and eight of its chosen pulses: always loaded - from slot 0
   where none was placed (qg = 0), a line the block's other bands read anyway - and zeroed afterwards, so
   that no lane's branch stands between the loads. */
__device__ __forceinline__ int4 lref_choice(const RJob &jb, int band, long lblk) {
  return global_load4(jb.lchoice + (lblk*jb.lnb + band)*4);
}

__device__ __forceinline__ uint4 lref_pulses(const RJob &jb, const int4 &ch, long lblk, int c0) {
  const long slot = ch.y != 0 ? ch.x : 0;
  const int4 y4 = global_load4(jb.ly + (slot*jb.lnblocks + lblk)*jb.llen + c0);
  const unsigned keep = ch.y != 0 ? ~0u : 0u;
  return make_uint4(y4.x & keep, y4.y & keep, y4.z & keep, y4.w & keep);
}

__device__ __forceinline__ void corner_zero(CornerSegs &s) {
#pragma unroll
  for (int y = 0; y < 4; y++) {
    s.b0[y] = make_int4(0, 0, 0, 0);
    s.b1[y & 1] = make_int4(0, 0, 0, 0);
    s.b2[y] = make_int2(0, 0);
  }
}

__device__ __forceinline__ int int4_at(const int4 &a, int i) {
  return i == 0 ? a.x : i == 1 ? a.y : i == 2 ? a.z : a.w;
}

__device__ __forceinline__ void unpack_band0(const int4 (&s)[4], int (&v)[15]) {
#pragma unroll
  for (int i = 0; i < 15; i++) v[i] = int4_at(s[OD_SCAN_XY[1 + i][1]], OD_SCAN_XY[1 + i][0]);
}

__device__ __forceinline__ void unpack_band1(const int4 (&s)[2], int (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = int4_at(s[OD_SCAN_XY[16 + i][1] & 1], OD_SCAN_XY[16 + i][0] - 4);
}

__device__ __forceinline__ void unpack_band2(const int2 (&s)[4], int (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int2 a = s[(OD_SCAN_XY[24 + i][1] - 4) & 3];
    v[i] = OD_SCAN_XY[24 + i][0] == 0 ? a.x : a.y;
  }
}

/* The chroma-from-luma sign flip of a block, decided from its band 0 before the flip is applied
   (src/pvq_encoder.c:846-872: OD_QM_SHIFT + OD_CFL_FLIP_SHIFT = 11 + 4, doubled). */
__device__ __forceinline__ int cfl_flip15(const int (&xv)[15], const int (&rv)[15], od_const_i16 qmp) {
  uint32_t xy = 0;
#pragma unroll
  for (int i = 0; i < 15; i++) {
    const int qm = qmp[i];
    const int32_t rq = (int32_t)((uint32_t)rv[i]*(uint32_t)qm);
    const int32_t inq = (int32_t)((uint32_t)xv[i]*(uint32_t)qm);
    xy += (uint32_t)((rq*(int64_t)inq) >> 30);
  }
  return (int32_t)xy < 0;
}

/* One band of a lane from its x and r in coding order (r before the flip): everything from
   od_vector_log_mag to the record.  N = 15 (band 0) or N = 8 (the band at coding position off). */
template <int N>
__device__ __forceinline__ void prep_lane_band(const RItems &it, const RJob &jb, int job, int band, long blk,
 int off, const int (&xv)[N], int (&rv)[N], int flip) {
  const int len = jb.len;
  const int q0 = job_q(jb, band, blk);
  const int beta = jb.beta[band];
  const int is_keyframe = jb.is_keyframe;
  const int cfl_enabled = is_keyframe && jb.pli != 0;
  const od_const_i16 qmp = const_table(jb.qm + off);
  int16_t *x16o = jb.x16 + blk*len;
  int16_t *r16o = jb.r16 + blk*len;
  int16_t *xro = jb.xr + blk*len;
  int qm[N];
#pragma unroll
  for (int i = 0; i < N; i++) qm[i] = qmp[i];
  /* od_vector_log_mag, src/pvq.c:472-484; src/pvq_encoder.c:381-385 */
  int sx = 0;
  int sr = 0;
  int r_null = 1;
#pragma unroll
  for (int i = 0; i < N; i++) {
    if (flip) rv[i] = -rv[i];
    const int tx = (int16_t)(xv[i] >> 8);
    const int tr = (int16_t)(rv[i] >> 8);
    sx += tx*tx;
    sr += tr*tr;
    if (rv[i]) r_null = 0;
  }
  const int xshift = odq_log_mag_shift(N, sx);
  int rshift = 8 + 1 + odq_ilog(N + sr)/2 - 14;
  rshift = rshift > 0 ? rshift : 0;
  int x16[N];
  int r16[N];
  double corr = 0;
  int accx = 0;
  int accr = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    x16[i] = (int16_t)odq_shr_round((int32_t)((uint32_t)xv[i]*(uint32_t)qm[i]), ODQ_QM_SHIFT + xshift);
    r16[i] = (int16_t)odq_shr_round((int32_t)((uint32_t)rv[i]*(uint32_t)qm[i]), ODQ_QM_SHIFT + rshift);
    corr += odq_mult16_16(x16[i], r16[i]);
    accx += x16[i]*x16[i];
    accr += r16[i]*r16[i];
  }
  const PrepScalars p = prep_scalars(accx, accr, corr, xshift, rshift, q0, beta, cfl_enabled,
   is_keyframe, r_null);
  int m = 0;
  int s = 1;
  int xr[N];
#pragma unroll
  for (int i = 0; i < N; i++) xr[i] = 0;
  if (p.ran) {
    /* od_compute_householder, src/pvq.c:498-521 */
    int maxr = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
      const int a = abs(r16[i]);
      if (a > maxr) {
        maxr = a;
        m = i;
      }
    }
    int rm = 0;
#pragma unroll
    for (int i = 0; i < N; i++) if (i == m) rm = r16[i];
    s = rm > 0 ? 1 : -1;
    const int upd = (int16_t)(rm + odq_shr_round(p.gr*s, rshift));
    int32_t l2r = 0;
    int32_t proj = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
      if (i == m) r16[i] = upd;
      l2r += odq_mult16_16(r16[i], r16[i]);
      proj += odq_mult16_16(r16[i], x16[i]);
    }
    const OdHouseholder hb = od_householder_back(l2r, proj);
    int v[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
      int32_t tmp = odq_mult16_16(r16[i], hb.proj_1);
      tmp = hb.outshift >= 0 ? odq_shr_round(tmp, hb.outshift) : odq_shl32(tmp, -hb.outshift);
      v[i] = (int16_t)(x16[i] - tmp);
    }
    /* the reflected vector without element m (src/pvq_encoder.c:481) */
#pragma unroll
    for (int i = 0; i < N - 1; i++) xr[i] = i < m ? v[i] : v[i + 1];
  }
#ifdef ODHIP_EXPERIMENTS
  const bool abl_nostore = (it.abl & 1) != 0;
  const bool abl_norec = (it.abl & 4) != 0;
#else
  constexpr bool abl_nostore = false;
  constexpr bool abl_norec = false;
#endif
  /* the decided stage's searches read x16 for the no-reference candidates and xr for the theta candidates
     alone (refb_loops_lean); r16 is the inverse's too */
  const bool keep_x = it.fuse != 2 || refb_has_noref(jb, p.cg, p.corr);
  const bool keep_xr = it.fuse != 2 || p.ran;
  /* whole 16-byte vectors: the 15-coefficient band shares its first vector with
     the (unused) DC slot of the block */
  if (abl_nostore) {
  }
  else if (N == 15) {
    uint4 *xo = reinterpret_cast<uint4 *>(x16o);
    uint4 *ro = reinterpret_cast<uint4 *>(r16o);
    uint4 *xro4 = reinterpret_cast<uint4 *>(xro);
    if (keep_x) {
      xo[0] = make_uint4(pack16(0, x16[0]), pack16(x16[1], x16[2]), pack16(x16[3], x16[4]),
       pack16(x16[5], x16[6]));
      xo[1] = make_uint4(pack16(x16[7], x16[8]), pack16(x16[9], x16[10]), pack16(x16[11], x16[12]),
       pack16(x16[13], x16[N - 1]));
    }
    ro[0] = make_uint4(pack16(0, r16[0]), pack16(r16[1], r16[2]), pack16(r16[3], r16[4]),
     pack16(r16[5], r16[6]));
    ro[1] = make_uint4(pack16(r16[7], r16[8]), pack16(r16[9], r16[10]), pack16(r16[11], r16[12]),
     pack16(r16[13], r16[N - 1]));
    if (keep_xr) {
      xro4[0] = make_uint4(pack16(0, xr[0]), pack16(xr[1], xr[2]), pack16(xr[3], xr[4]),
       pack16(xr[5], xr[6]));
      xro4[1] = make_uint4(pack16(xr[7], xr[8]), pack16(xr[9], xr[10]), pack16(xr[11], xr[12]),
       pack16(xr[13], 0));
    }
  }
  else {
    if (keep_x) {
      *reinterpret_cast<uint4 *>(x16o + off) = make_uint4(pack16(x16[0], x16[1]), pack16(x16[2], x16[3]),
       pack16(x16[4], x16[5]), pack16(x16[6], x16[7]));
    }
    *reinterpret_cast<uint4 *>(r16o + off) = make_uint4(pack16(r16[0], r16[1]), pack16(r16[2], r16[3]),
     pack16(r16[4], r16[5]), pack16(r16[6], r16[7]));
    if (keep_xr) {
      *reinterpret_cast<uint4 *>(xro + off) = make_uint4(pack16(xr[0], xr[1]), pack16(xr[2], xr[3]),
       pack16(xr[4], xr[5]), pack16(xr[6], 0));
    }
  }
  if (!abl_norec) {
    prep_write(it, jb, jb.rec + blk*jb.nb_bands + band, job, band, blk, xshift, rshift, p, r_null, flip, m, s);
  }
}

/* One block per lane: band 0 and, for blocks of 8x8 and up (wave-uniform: an item is a job), bands 1
   and 2.  The three bands of a block lie in the same lines - band 1 continues band 0's sectors of rows
   0-1; the luma choice records of bands 0-2 are adjacent and their pulses are the first 64 bytes of one
   vector - so every load of the lane is issued before the first use, and a band is prepared and stored
   before the next is unpacked: only loaded words wait.  The flip is decided from band 0 first and stays
   in a register; band 0 itself, the widest, goes last, when nothing else is held. */
__global__ __launch_bounds__(kWave) void k_refb_prep_corner(RItems it) {
  const int item = find_item(it, blockIdx.x);
  /* the same for every lane, and said so: the job's fields are then scalar loads */
  const int job = __builtin_amdgcn_readfirstlane(it.job[item]);
  /* the job's fields are the same for every lane: read once, here, where nothing has been stored yet and
     they are scalar loads - behind a lane's first store the compiler must fetch each with a vector load
     and wait for it, a dozen times per band */
  const RJob jb = it.jobs[job];
  const long blk = (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x;
  if (blk >= jb.nblocks) return;
  const bool more = jb.nb_bands > 1;
  const int w = jb.w;
  const long base = block_base(jb, blk);
  /* the reference: a plane of the job's layout, or (keyframe chroma) taken straight from
     the luma band stage - lref_piece */
  const bool lref = jb.ly != nullptr;
#ifdef ODHIP_EXPERIMENTS
  const bool lref_read = lref && !(it.abl & 2);
#else
  const bool lref_read = lref;
#endif
  const long lblk = lref_block(jb, blk);
  int4 ch[3];
  uint4 ly[4];
#pragma unroll
  for (int b = 0; b < 3; b++) ch[b] = make_int4(0, 0, 0, 0);
#pragma unroll
  for (int i = 0; i < 4; i++) ly[i] = make_uint4(0, 0, 0, 0);
  if (lref_read) {
    ch[0] = lref_choice(jb, 0, lblk);
    if (more) {
      ch[1] = lref_choice(jb, 1, lblk);
      ch[2] = lref_choice(jb, 2, lblk);
    }
  }
  CornerSegs xs;
  CornerSegs rs;
  corner_load(jb.coef + base, w, more, xs);
  if (!lref) corner_load(jb.ref + base, w, more, rs);
  else {
    corner_zero(rs);
    if (lref_read) {
      ly[0] = lref_pulses(jb, ch[0], lblk, 0);
      ly[1] = lref_pulses(jb, ch[0], lblk, 8);
      if (more) {
        ly[2] = lref_pulses(jb, ch[1], lblk, 16);
        ly[3] = lref_pulses(jb, ch[2], lblk, 24);
      }
    }
  }
  int xv[15];
  int rv[15];
  unpack_band0(xs.b0, xv);
  unpack_band0(rs.b0, rv);
  if (lref_read) {
    /* coding order is what the luma stage keeps: whole 16-byte pieces */
    int lo[8];
    int hi[8];
    lref_dequant(ch[0], ly[0], const_load4(jb.lqmi), lo);
    lref_dequant(ch[0], ly[1], const_load4(jb.lqmi + 8), hi);
#pragma unroll
    for (int i = 0; i < 15; i++) rv[i] = i + 1 < 8 ? lo[(i + 1) & 7] : hi[(i + 1) & 7];
  }
  const int cfl_enabled = jb.is_keyframe && jb.pli != 0;
  const int flip = cfl_enabled ? cfl_flip15(xv, rv, const_table(jb.qm + jb.off[0])) : 0;
  if (more) {
    int xb[8];
    int rb[8];
    unpack_band1(xs.b1, xb);
    unpack_band1(rs.b1, rb);
    if (lref_read) lref_dequant(ch[1], ly[2], const_load4(jb.lqmi + 16), rb);
    prep_lane_band<8>(it, jb, job, 1, blk, 16, xb, rb, flip);
    unpack_band2(xs.b2, xb);
    unpack_band2(rs.b2, rb);
    if (lref_read) lref_dequant(ch[2], ly[3], const_load4(jb.lqmi + 24), rb);
    prep_lane_band<8>(it, jb, job, 2, blk, 24, xb, rb, flip);
  }
  prep_lane_band<15>(it, jb, job, 0, blk, jb.off[0], xv, rv, flip);
}

#ifdef ODHIP_EXPERIMENTS
/* The split form k_refb_prep_corner replaced (ODHIP_REFB_PREP_SPLIT: the A/B baseline of the tests and of
   profiles/refprep_corner.txt): (job, band) items, N = 15 (band 0: the flip is decided here) or N = 8
   (launched behind it: the flip is read back from band 0's record). */
template <int N>
__global__ __launch_bounds__(kWave) void k_refb_prep_lane(RItems it) {
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const RJob &jb = it.jobs[job];
  const int band = it.band[item];
  const long blk = (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x;
  if (blk >= jb.nblocks) return;
  const int off = jb.off[band];
  const int w = jb.w;
  const long base = block_base(jb, blk);
  const od_coeff *x0 = jb.coef + base;
  const bool lref = jb.ly != nullptr;
  const od_coeff *r0 = lref ? jb.coef + base : jb.ref + base;
  int xv[N];
  int rv[N];
  if constexpr (N == 15) {
    int4 xs[4];
    int4 rs[4];
#pragma unroll
    for (int y = 0; y < 4; y++) {
      xs[y] = *reinterpret_cast<const int4 *>(x0 + (long)y*w);
      rs[y] = lref ? make_int4(0, 0, 0, 0) : *reinterpret_cast<const int4 *>(r0 + (long)y*w);
    }
    unpack_band0(xs, xv);
    unpack_band0(rs, rv);
  }
  else {
    if (off == 16) {
      int4 xs[2];
      int4 rs[2];
#pragma unroll
      for (int y = 0; y < 2; y++) {
        xs[y] = *reinterpret_cast<const int4 *>(x0 + (long)y*w + 4);
        rs[y] = lref ? make_int4(0, 0, 0, 0) : *reinterpret_cast<const int4 *>(r0 + (long)y*w + 4);
      }
      unpack_band1(xs, xv);
      unpack_band1(rs, rv);
    }
    else if (off == 24) {
      int2 xs[4];
      int2 rs[4];
#pragma unroll
      for (int y = 0; y < 4; y++) {
        xs[y] = *reinterpret_cast<const int2 *>(x0 + (long)(4 + y)*w);
        rs[y] = lref ? make_int2(0, 0) : *reinterpret_cast<const int2 *>(r0 + (long)(4 + y)*w);
      }
      unpack_band2(xs, xv);
      unpack_band2(rs, rv);
    }
    else {
#pragma unroll
      for (int i = 0; i < N; i++) {
        const long p = (long)kRScanXY[off + i][1]*w + kRScanXY[off + i][0];
        xv[i] = x0[p];
        rv[i] = lref ? 0 : r0[p];
      }
    }
  }
  if (lref && !(it.abl & 2)) {
    if constexpr (N == 15) {
      int lo[8];
      int hi[8];
      lref_piece(jb, band, blk, 0, lo);
      lref_piece(jb, band, blk, 8, hi);
#pragma unroll
      for (int i = 0; i < N; i++) rv[i] = i + 1 < 8 ? lo[(i + 1) & 7] : hi[(i + 1) & 7];
    }
    else {
      int pc[8];
      lref_piece(jb, band, blk, off, pc);
#pragma unroll
      for (int i = 0; i < N; i++) rv[i] = pc[i & 7];
    }
  }
  int flip = 0;
  if (jb.is_keyframe && jb.pli != 0) {
    if constexpr (N == 15) flip = cfl_flip15(xv, rv, const_table(jb.qm + off));
    else flip = block_flip(it, job, jb, blk, it.fuse == 2);
  }
  prep_lane_band<N>(it, jb, job, band, blk, off, xv, rv, flip);
}
#endif

/* n = G*E coefficients per group of G lanes (G = 16: a DPP row, G = 4: a quad),
   64/G bands per wavefront; lane l of the group owns coding positions l*E ..
   l*E+E-1 of the band.  The group prepares block blk0 (none past the job's last: it redoes the last block
   without storing); s_scan holds the band's n scan positions; lean_flip: where band 0 left the flip. */
template <int E, int G>
__device__ __forceinline__ void prep_row_band(const RItems &it, int job, const RJob &jb, int band, long blk0,
 bool lean_flip, const unsigned short *s_scan) {
  constexpr int n = G*E;
  const int off = jb.off[band];
  const int l = threadIdx.x%G;
  const long nblocks = jb.nblocks;
  const bool live = blk0 < nblocks;
  const long blk = live ? blk0 : nblocks - 1;
  const int w = jb.w;
  const int len = jb.len;
  const int nb_bands = jb.nb_bands;
  const int q0 = job_q(jb, band, blk);
  const int beta = jb.beta[band];
  const int is_keyframe = jb.is_keyframe;
  const int cfl_enabled = is_keyframe && jb.pli != 0;
  const long base = block_base(jb, blk);
  const od_coeff *x0 = jb.coef + base;
  const bool lref = jb.ly != nullptr;
  const od_coeff *r0 = lref ? jb.coef + base : jb.ref + base;
  const int16_t *qmp = jb.qm + off + l*E;
  odhip_pvq_refband *rec = jb.rec + blk*nb_bands;
  int16_t *x16o = jb.x16 + blk*len + off;
  int16_t *r16o = jb.r16 + blk*len + off;
  int16_t *xro = jb.xr + blk*len + off;
  const int flip = cfl_enabled ? block_flip(it, job, jb, blk, lean_flip) : 0;
  int xv[E];
  int rv[E];
  int qm[E];
  int sx = 0;
  int sr = 0;
  int nz = 0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int pk = s_scan[l*E + e];
    const long p = (long)(pk >> 8)*w + (pk & 255);
    xv[e] = x0[p];
    const int r = lref ? 0 : r0[p];
    rv[e] = flip ? -r : r;
    qm[e] = qmp[e];
  }
  if (lref) {
    static_assert(E == 8, "one 16-byte piece of the luma stage's pulses per lane");
    int pc[8];
    lref_piece(jb, band, blk, off + l*E, pc);
#pragma unroll
    for (int e = 0; e < E; e++) rv[e] = flip ? -pc[e] : pc[e];
  }
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int tx = (int16_t)(xv[e] >> 8);
    const int tr = (int16_t)(rv[e] >> 8);
    sx += tx*tx;
    sr += tr*tr;
    nz |= rv[e] != 0;
  }
  sx = grp_sum<G>(sx);
  sr = grp_sum<G>(sr);
  const int r_null = grp_max<G>(nz) == 0;
  const int xshift = odq_log_mag_shift(n, sx);
  int rshift = 8 + 1 + odq_ilog(n + sr)/2 - 14;
  rshift = rshift > 0 ? rshift : 0;
  int x16[E];
  int r16[E];
  double corr = 0;
  int accx = 0;
  int accr = 0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    x16[e] = (int16_t)odq_shr_round((int32_t)((uint32_t)xv[e]*(uint32_t)qm[e]), ODQ_QM_SHIFT + xshift);
    r16[e] = (int16_t)odq_shr_round((int32_t)((uint32_t)rv[e]*(uint32_t)qm[e]), ODQ_QM_SHIFT + rshift);
    corr += odq_mult16_16(x16[e], r16[e]);
    accx += x16[e]*x16[e];
    accr += r16[e]*r16[e];
  }
  corr = grp_sum<G>(corr);
  accx = grp_sum<G>(accx);
  accr = grp_sum<G>(accr);
  const PrepScalars p = prep_scalars(accx, accr, corr, xshift, rshift, q0, beta, cfl_enabled,
   is_keyframe, r_null);
  int m = 0;
  int s = 1;
  if (p.ran) {
    /* od_compute_householder: (largest |r|, lowest index) over the row */
    int ba = -1;
    int bi = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int a = abs(r16[e]);
      if (a > ba) {
        ba = a;
        bi = l*E + e;
      }
    }
#define OD_ARGMAX_STEP(CTRL) \
    { \
      const int oa = row_mov<CTRL>(ba); \
      const int oi = row_mov<CTRL>(bi); \
      const bool take = oa > ba || (oa == ba && oi < bi); \
      ba = take ? oa : ba; \
      bi = take ? oi : bi; \
    }
    OD_ARGMAX_STEP(OD_DPP_XOR1)
    OD_ARGMAX_STEP(OD_DPP_XOR2)
    if (G == 16) {
      OD_ARGMAX_STEP(OD_DPP_HALF_MIRROR)
      OD_ARGMAX_STEP(OD_DPP_MIRROR)
    }
#undef OD_ARGMAX_STEP
    m = bi;
    int rm = 0;
#pragma unroll
    for (int e = 0; e < E; e++) if (l*E + e == m) rm = r16[e];
    rm = grp_sum<G>(rm);
    s = rm > 0 ? 1 : -1;
    const int upd = (int16_t)(rm + odq_shr_round(p.gr*s, rshift));
    int32_t l2r = 0;
    int32_t proj = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      if (l*E + e == m) r16[e] = upd;
      l2r += odq_mult16_16(r16[e], r16[e]);
      proj += odq_mult16_16(r16[e], x16[e]);
    }
    l2r = grp_sum<G>(l2r);
    proj = grp_sum<G>(proj);
    const OdHouseholder hb = od_householder_back(l2r, proj);
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int i = l*E + e;
      int32_t tmp = odq_mult16_16(r16[e], hb.proj_1);
      tmp = hb.outshift >= 0 ? odq_shr_round(tmp, hb.outshift) : odq_shl32(tmp, -hb.outshift);
      const int16_t v = (int16_t)(x16[e] - tmp);
      /* the reflected vector without element m (src/pvq_encoder.c:481) */
      if (live && i != m) xro[i - (i > m)] = v;
    }
  }
  if (live) {
    /* (the decided stage: x16 where a search reads it, as in prep_lane_band; xr above is stored for the
       theta candidates alone in every stage) */
    const bool keep_x = it.fuse != 2 || refb_has_noref(jb, p.cg, p.corr);
    if constexpr (E == 8) {
      if (keep_x) {
        *reinterpret_cast<uint4 *>(x16o + l*E) = make_uint4(pack16(x16[0], x16[1]),
         pack16(x16[2], x16[3]), pack16(x16[4], x16[5]), pack16(x16[6], x16[7]));
      }
      *reinterpret_cast<uint4 *>(r16o + l*E) = make_uint4(pack16(r16[0], r16[1]),
       pack16(r16[2], r16[3]), pack16(r16[4], r16[5]), pack16(r16[6], r16[7]));
    }
    else {
#pragma unroll
      for (int e = 0; e < E; e += 2) {
        if (keep_x) *reinterpret_cast<uint32_t *>(x16o + l*E + e) = pack16(x16[e], x16[e + 1]);
        *reinterpret_cast<uint32_t *>(r16o + l*E + e) = pack16(r16[e], r16[e + 1]);
      }
    }
    if (l == 0) prep_write(it, jb, rec + band, job, band, blk, xshift, rshift, p, r_null, flip, m, s);
  }
}

template <int E, int G>
__global__ __launch_bounds__(kWave) void k_refb_prep_row(RItems it) {
  constexpr int n = G*E;
  __shared__ unsigned short s_scan[n];
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const RJob &jb = it.jobs[job];
  const int band = it.band[item];
  const int off = jb.off[band];
  const int lane = threadIdx.x;
  for (int j = lane; j < n; j += kWave) s_scan[j] = gRScanPk[off + j];
  __syncthreads();
  const long blk0 = (long)(blockIdx.x - it.wg_start[item])*(kWave/G) + lane/G;
  prep_row_band<E, G>(it, job, jb, band, blk0, it.fuse == 2, s_scan);
}

/* ---- the listed bands of the decided stage -------------------------------------------
   The decided stage writes neither the job's records nor the vectors its searches do not read, and the
   resolve paths re-run their bands (theta inside the acos margin, a priced comparison inside the log margin)
   through the exporting kernels, which read all of them.  In front of such a re-run the listed bands are
   prepared again in the exporting form (it.fuse = kStageRecords, no margin: nothing is listed twice), one
   band per wavefront - the lists are a handful of bands.  The flip of the block and the band's theta are the
   decided stage's own, from the lean record (theta: what its search used - the perturbed one under the test
   hook - or, once the host has recomputed it, the host's, which is kept there for a later priced resolve). */
template <int N>
__device__ __forceinline__ void prep_lane_listed(const RItems &it, int job, const RJob &jb, int band, long blk) {
  const int off = jb.off[band];
  const long base = block_base(jb, blk);
  const bool lref = jb.ly != nullptr;
  int xv[N];
  int rv[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
    const long p = base + coef_pos(jb, off + i);
    xv[i] = jb.coef[p];
    rv[i] = lref ? 0 : jb.ref[p];
  }
  if (lref) {
    if constexpr (N == 15) {
      int lo[8];
      int hi[8];
      lref_piece(jb, band, blk, 0, lo);
      lref_piece(jb, band, blk, 8, hi);
#pragma unroll
      for (int i = 0; i < N; i++) rv[i] = i + 1 < 8 ? lo[(i + 1) & 7] : hi[(i + 1) & 7];
    }
    else {
      int pc[8];
      lref_piece(jb, band, blk, off, pc);
#pragma unroll
      for (int i = 0; i < N; i++) rv[i] = pc[i & 7];
    }
  }
  int flip = 0;
  if (jb.is_keyframe && jb.pli != 0) {
    if constexpr (N == 15) flip = cfl_flip15(xv, rv, const_table(jb.qm + off));
    else flip = block_flip(it, job, jb, blk, true);
  }
  prep_lane_band<N>(it, jb, job, band, blk, off, xv, rv, flip);
}

__global__ __launch_bounds__(kWave) void k_refb_prep_list(RItems it, const Unc *list, int count) {
  __shared__ unsigned short s_scan[128];
  if ((int)blockIdx.x >= count) return;
  const Unc e = list[blockIdx.x];
  const int job = e.job;
  const RJob &jb = it.jobs[job];
  const int band = e.band;
  const long blk = e.blk;
  const int off = jb.off[band];
  const int n = jb.off[band + 1] - off;
  const int lane = threadIdx.x;
  if (n >= 32) {
    /* the first group of the wavefront; the others take part without a block */
    for (int j = lane; j < n; j += kWave) s_scan[j] = gRScanPk[off + j];
    __syncthreads();
    if (n == 32) prep_row_band<8, 4>(it, job, jb, band, lane < 4 ? blk : jb.nblocks, true, s_scan);
    else prep_row_band<8, 16>(it, job, jb, band, lane < 16 ? blk : jb.nblocks, true, s_scan);
  }
  else if (lane == 0) {
    if (n == 15) prep_lane_listed<15>(it, job, jb, band, blk);
    else prep_lane_listed<8>(it, job, jb, band, blk);
  }
  if (lane == 0) {
    /* (the lane that wrote the record) */
    LeanRec *lr = lean_rec(it, job, jb, blk, band);
    odhip_pvq_refband *rec = jb.rec + blk*jb.nb_bands + band;
    if (e.theta >= 0) lr->theta = e.theta;
    rec->theta = lr->theta;
    rec->flags = (uint8_t)(lr->msf >> 24);
  }
}


/* ---- candidate records -------------------------------------------------------------
   odhip_pvq_refitem in memory: three planes of 16-byte vectors, each
   [nb][ODHIP_PVQ_REF_SLOTS][B] (block index fastest, so the lanes of a
   wavefront - adjacent blocks - touch one contiguous kilobyte per access):
     head  {gain, theta, ts, k}          written by the candidate kernel
     tail  {qcg, qtheta, flags, yslot}   written by the search
     res   {cos_dist, dist}              written by the search
   The first layout - 48-byte records per (block, band, slot), fields read and
   written one by one - made every access of a wavefront 64 separate sectors. */
struct ItemPtr {
  int4 *head;
  int4 *tail;
  int4 *res;
  long stride;   /* vectors between consecutive slots */
};

__device__ __forceinline__ ItemPtr item_ptr(const RJob &jb, int band, long blk) {
  ItemPtr p;
  const long plane = (long)jb.nb_bands*kSlots*jb.nblocks;
  p.head = reinterpret_cast<int4 *>(jb.items) + (long)band*kSlots*jb.nblocks + blk;
  p.tail = p.head + plane;
  p.res = p.tail + plane;
  p.stride = jb.nblocks;
  return p;
}

/* ---- candidate lists -------------------------------------------------------------- */
/* The list is built in LDS (stage[slot][lane]: the stable insertion walks it
   backwards) and written to the head plane once, slot by slot - adjacent lanes are
   adjacent blocks, so every slot is one coalesced 1 KiB store per wavefront.  Round 1
   inserted directly in the head plane: a read-modify-write chain through HBM per
   candidate (242 us per 16-frame launch). */
__device__ __forceinline__ void refb_candidates(const RJob &jb, int band, long blk,
 int theta_override, int4 (*stage)[kWave]) {
  const int lane = threadIdx.x;
  odhip_pvq_refband *rp = jb.rec + blk*jb.nb_bands + band;
  odhip_pvq_refband r = *rp;
  if (theta_override >= 0) r.theta = theta_override;
  const int n = jb.off[band + 1] - jb.off[band];
  const int beta = jb.beta[band];
  const ItemPtr ip = item_ptr(jb, band, blk);
  int nitems = 0;
  int kmax_theta = 0;
  int kmax_noref = 0;
  if (r.flags & ODHIP_REFBAND_THETA) {
    const int gain_bound = (r.cg - r.gain_offset) >> ODQ_CGAIN_SHIFT;
    const double scale_1 = __ddiv_rn(1., kThetaScale);   /* OD_THETA_SCALE_1 */
    for (int i = gain_bound - 1 > 1 ? gain_bound - 1 : 1; i <= gain_bound + 1; i++) {
      const int32_t qcg = odq_shl32(i, ODQ_CGAIN_SHIFT) + r.gain_offset;
      const int ts = odq_pvq_compute_max_theta(qcg, beta);
      /* same left-to-right products as src/pvq_encoder.c:482-484 */
      const double t = __ddiv_rn(((r.theta*scale_1)*2), kPi)*ts;
      int lower = (int)floor(.5 + t) - 2;
      if (lower < 0) lower = 0;
      int upper = (int)ceil(t);
      if (upper > ts - 1) upper = ts - 1;
      for (int j = lower; j <= upper && nitems < kSlots - 2; j++) {
        const int4 c = make_int4(i, j, ts, odq_compute_k_ref(j, n));
        kmax_theta = c.w > kmax_theta ? c.w : kmax_theta;
        /* stable insertion by (k, gain): items_compare, src/pvq_encoder.c:301-305
           (glibc's qsort is a stable merge sort at this size) */
        int pos = nitems;
        while (pos > 0) {
          const int4 q = stage[pos - 1][lane];
          const int cmp = q.w == c.w ? q.x - c.x : q.w - c.w;
          if (cmp <= 0) break;
          stage[pos][lane] = q;
          pos--;
        }
        stage[pos][lane] = c;
        nitems++;
      }
    }
  }
  const int ntheta = nitems;
  int flags = r.flags & ~ODHIP_REFBAND_NOREF;
  /* src/pvq_encoder.c:571-581 */
  if ((jb.is_keyframe && jb.pli == 0) || r.corr < .5 || r.cg < odq_shl32(2, ODQ_CGAIN_SHIFT)) {
    flags |= ODHIP_REFBAND_NOREF;
    const int gain_bound = r.cg >> ODQ_CGAIN_SHIFT;
    for (int i = gain_bound > 1 ? gain_bound : 1; i <= gain_bound + 1; i++) {
      const int kk = odq_compute_k_noref(odq_shl32(i, ODQ_CGAIN_SHIFT), n, beta);
      stage[nitems][lane] = make_int4(i, -1, 0, kk);
      kmax_noref = kk > kmax_noref ? kk : kmax_noref;
      nitems++;
    }
  }
  for (int i = 0; i < nitems; i++) ip.head[i*ip.stride] = stage[i][lane];
  /* third vector of the record: {m, s, flags | theta | nitems | ntheta} */
  int4 v;
  v.x = (int)((uint32_t)(uint16_t)r.m | (uint32_t)(uint8_t)r.s << 16 | (uint32_t)flags << 24);
  v.y = r.theta;
  v.z = nitems;
  v.w = ntheta;
  reinterpret_cast<int4 *>(rp)[2] = v;
  /* work class for the sorted searches: the chains place about kmax pulses */
  jb.keys[(long)band*jb.nblocks + blk] = (unsigned short)(kSortBins - 1 - od_work_bin(kmax_theta + kmax_noref));
}

__global__ __launch_bounds__(kWave) void k_refb_cands(RItems it) {
  const int item = find_item(it, blockIdx.x);
  const RJob &jb = it.jobs[it.job[item]];
  const long blk = (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x;
  __shared__ int4 stage[kSlots][kWave];
  if (blk >= jb.nblocks) return;
  refb_candidates(jb, it.band[item], blk, -1, stage);
}

__global__ __launch_bounds__(kWave) void k_refb_cands_list(const RJob *jobs, const Unc *list, int count) {
  __shared__ int4 stage[kSlots][kWave];
  const int i = blockIdx.x*kWave + threadIdx.x;
  if (i >= count) return;
  const Unc e = list[i];
  refb_candidates(jobs[e.job], e.band, e.blk, e.theta, stage);
}

/* ---- the candidate loops -----------------------------------------------------------
   src/pvq_encoder.c:506-565 (theta candidates) and :578-595 (no-reference
   candidates) for one band, over a vector holder V that owns the band's |x|,
   signs and pulses in whatever form its mapping uses:
     V::load(src, pad)      the band vector (pad: the last position is not part
                            of it - the n - 1 reflected coefficients)
     V::search(n, k, prev_k, g2, lambda)   pvq_search_rdo_double on it
     V::store(dst)          the signed pulses, coding order
     V::moment()            SUM i*|y_i| of the pulses it holds (od_pvq_rate's centre-of-
                            mass sum, src/pvq_encoder.c:258-259), kept in the item's
                            flags word above ODHIP_REFITEM_MOMENT_SHIFT so that the priced
                            choice never reads the vectors
   `writer`: this lane records the band's results (one lane per band). */
/* What the choice among a band's candidates keeps (src/pvq_encoder.c:417-609). */
struct RefBest {
  double best_cost;
  int chosen;              /* item, -1 = the initial candidate */
  int yslot;
  int noref;
  int32_t qtheta;
  int gain;                /* the winner's head {gain, theta, ts, k} */
  int theta;
  int ts;
  int k;
  bool close;              /* a comparison too close for the device's log */
};

/* The reference's distortion expressions (src/pvq_encoder.c), each spelt ONCE: the stage is bit-exact
   because these lines keep the reference's operand order and parentheses (the build has -ffp-contract=off).
   qcg / cg: the candidate's and the band's companded gain; cosd = od_pvq_cos(theta - qtheta). */
constexpr double kCgainScale2 = (1./256)*(1./256);   /* OD_CGAIN_SCALE_2 */
constexpr double kTrigScale1 = 1./32768;             /* OD_TRIG_SCALE_1 */

__device__ __forceinline__ double refb_cos_term(int cosd) {
  return 2 - (2.*cosd)*kTrigScale1;
}

__device__ __forceinline__ double refb_sin_prod(int sin_theta, int sin_qtheta) {
  return ((sin_theta*kTrigScale1)*sin_qtheta)*kTrigScale1;
}

/* :526-531, the gate in front of a theta candidate's search: dist_theta = refb_cos_term */
__device__ __forceinline__ double refb_dist_gate(int32_t qcg, int32_t cg, double dist_theta) {
  double dist = (1.4*(qcg - cg))*(qcg - cg) + (qcg*(double)cg)*dist_theta;
  dist *= kCgainScale2;
  return dist;
}

/* :548-552, a theta candidate after its search */
__device__ __forceinline__ double refb_dist_theta(int32_t qcg, int32_t cg, double cos_term, double sin_prod,
 double cos_dist) {
  return refb_dist_gate(qcg, cg, cos_term + sin_prod*(2 - 2*cos_dist));
}

/* :585-595, a no-reference candidate: its gate (the gain term alone) and its distortion after the search */
__device__ __forceinline__ double refb_dist_noref_gate(int32_t qcg, int32_t cg) {
  double dist = (1.4*(qcg - cg))*(qcg - cg);
  dist *= kCgainScale2;
  return dist;
}

__device__ __forceinline__ double refb_dist_noref(int32_t qcg, int32_t cg, double cos_dist) {
  return refb_dist_gate(qcg, cg, 2 - 2*cos_dist);
}

/* refb_loops offers every searched candidate, in the reference's order, to a decider:
   nothing (the choice is a later kernel's) or FuseDecide below. */
struct NoDecide {
  template <class V>
  __device__ __forceinline__ void offer(int, bool, const int4 &, int32_t, int, double, int, const V &) {}
};

template <class V, class D>
__device__ __forceinline__ void refb_loops(const RJob &jb, int band, long blk, bool writer,
 bool may_store, double lambda, V &v, D &dec) {
  const odhip_pvq_refband r = jb.rec[blk*jb.nb_bands + band];
  const int off = jb.off[band];
  const int n = jb.off[band + 1] - off;
  const long nblocks = jb.nblocks;
  const int len = jb.len;
  int16_t *const yout = jb.y;
  const ItemPtr ip = item_ptr(jb, band, blk);
  const int32_t cg = r.cg;
  const double dist0 = r.dist0;
  if (r.ntheta > 0) {
    v.load(jb.xr + blk*len + off, true);
    int prev_k = 0;
    int cur_slot = -1;
    int cur_mom = 0;
    double cos_dist = 0;
    const int32_t theta = r.theta;
    int4 hnext = ip.head[0];
    for (int idx = 0; idx < r.ntheta; idx++) {
      const int4 h = hnext;                       /* gain, theta, ts, k */
      /* the next candidate's head is requested before this one is worked on */
      hnext = ip.head[(idx + 1 < r.nitems ? idx + 1 : idx)*ip.stride];
      const int32_t qcg = odq_shl32(h.x, ODQ_CGAIN_SHIFT) + r.gain_offset;
      const int32_t qtheta = odq_pvq_compute_theta(h.y, h.z);
      const int k = h.w;
      if (refb_dist_gate(qcg, cg, refb_cos_term(odq_pvq_cos(theta - qtheta))) > dist0 + 1.0*lambda && k != 0) {
        if (writer) ip.tail[idx*ip.stride] = make_int4(qcg, qtheta, ODHIP_REFITEM_WITH_REF, -1);
        continue;
      }
      if (k > ODHIP_PVQ_MAX_K) {
        /* pulses are stored as int16: reported, never searched or chosen (the
           candidates are sorted by K, so every later one is skipped as well) */
        if (writer) {
          atomicAdd(jb.krange, 1u);
          ip.tail[idx*ip.stride] = make_int4(qcg, qtheta, ODHIP_REFITEM_WITH_REF | ODHIP_REFITEM_K_RANGE,
           -1);
        }
        continue;
      }
      const double sin_prod = refb_sin_prod(odq_pvq_sin(theta), odq_pvq_sin(qtheta));
      if (k == 0) {
        cos_dist = 0;
        cur_slot = -1;
        cur_mom = 0;
      }
      else if (k != prev_k) {
        cos_dist = v.search(n - 1, k, prev_k, ((qcg*(double)cg)*sin_prod)*kCgainScale2, lambda);
        cur_slot = idx;
        cur_mom = v.moment();
        if (may_store) v.store(yout + ((long)idx*nblocks + blk)*len + off);
      }
      prev_k = k;
      /* (the cosine term is formed again, not carried through the search) */
      const double dist = refb_dist_theta(qcg, cg, refb_cos_term(odq_pvq_cos(theta - qtheta)), sin_prod, cos_dist);
      if (writer) {
        ip.tail[idx*ip.stride] = make_int4(qcg, qtheta,
         ODHIP_REFITEM_WITH_REF | ODHIP_REFITEM_SEARCHED | cur_mom << ODHIP_REFITEM_MOMENT_SHIFT, cur_slot);
        ip.res[idx*ip.stride] = make_int4(__double2loint(cos_dist), __double2hiint(cos_dist),
         __double2loint(dist), __double2hiint(dist));
      }
      dec.offer(idx, true, h, qtheta, cur_slot, dist, cur_mom, v);
    }
  }
  if (r.nitems > r.ntheta) {
    v.load(jb.x16 + blk*len + off, false);
    int prev_k = 0;
    for (int idx = r.ntheta; idx < r.nitems; idx++) {
      const int4 h = ip.head[idx*ip.stride];
      const int32_t qcg = odq_shl32(h.x, ODQ_CGAIN_SHIFT);
      const int k = h.w;
      if (refb_dist_noref_gate(qcg, cg) > dist0 && k != 0) {
        if (writer) ip.tail[idx*ip.stride] = make_int4(qcg, 0, 0, -1);
        continue;
      }
      if (k > ODHIP_PVQ_MAX_K) {
        if (writer) atomicAdd(jb.krange, 1u);
        if (writer) ip.tail[idx*ip.stride] = make_int4(qcg, 0, ODHIP_REFITEM_K_RANGE, -1);
        continue;
      }
      const double cos_dist = v.search(n, k, prev_k, (qcg*(double)cg)*kCgainScale2, lambda);
      prev_k = k;
      const int mom = v.moment();
      if (may_store) v.store(yout + ((long)idx*nblocks + blk)*len + off);
      const double dist = refb_dist_noref(qcg, cg, cos_dist);
      if (writer) {
        ip.tail[idx*ip.stride] = make_int4(qcg, 0, ODHIP_REFITEM_SEARCHED | mom << ODHIP_REFITEM_MOMENT_SHIFT, idx);
        ip.res[idx*ip.stride] = make_int4(__double2loint(cos_dist), __double2hiint(cos_dist),
         __double2loint(dist), __double2hiint(dist));
      }
      dec.offer(idx, false, h, 0, idx, dist, mom, v);
    }
  }
}

/* One band per lane, |x| and pulses in LDS columns, any n (pvq_search.cuh): the
   resolve path and, with ODHIP_PVQ_REF_LANE=1, every band size. */
struct LdsVector {
  short *xs;
  unsigned short *ys;
  int lane;
  int n;
  __device__ __forceinline__ void load(const int16_t *src, bool pad) {
    const int cnt = n - (pad ? 1 : 0);
    for (int j = 0; j < cnt; j++) xs[j*kWave + lane] = src[j];
  }
  __device__ __forceinline__ double search(int n_true, int k, int prev_k, double g2, double lambda) {
    double yy;
    cur = n_true;
    return od_pvq_search_lane(xs, ys, lane, n_true, k, prev_k, g2, lambda, &yy);
  }
  __device__ __forceinline__ void store(int16_t *dst) {
    for (int j = 0; j < cur; j++) {
      const int yj = ys[j*kWave + lane];
      dst[j] = (int16_t)(xs[j*kWave + lane] < 0 ? -yj : yj);
    }
  }
  __device__ __forceinline__ int moment() const {
    int m = 0;
    for (int j = 1; j < cur; j++) m += j*ys[j*kWave + lane];
    return m;
  }
  int cur;
};

#ifdef ODHIP_EXPERIMENTS
/* ODHIP_PVQ_REF_LANE (experiments build): every band size one band per lane, vectors in LDS. */
__global__ __launch_bounds__(kWave) void k_refb_search(RItems it) {
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  od_rsqrt_init(threadIdx.x);
  const int item = find_item(it, blockIdx.x);
  const RJob &jb = it.jobs[it.job[item]];
  const int band = it.band[item];
  const int n = jb.off[band + 1] - jb.off[band];
  const long pos = (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x;
  if (pos >= jb.nblocks) return;
  const long blk = jb.ids[(long)band*jb.nblocks + pos];
  LdsVector v = {(short *)lds, lds + n*kWave, (int)threadIdx.x, n, 0};
  NoDecide nd;
  refb_loops(jb, band, blk, true, true, it.lambda, v, nd);
}
#endif

/* One listed band per wavefront (lane 0): the list is a handful of bands. */
__global__ __launch_bounds__(kWave) void k_refb_search_list(const RJob *jobs, const Unc *list, int count,
 double lambda) {
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  od_rsqrt_init(threadIdx.x);
  if (threadIdx.x != 0 || (int)blockIdx.x >= count) return;
  const Unc e = list[blockIdx.x];
  const RJob &jb = jobs[e.job];
  LdsVector v = {(short *)lds, lds + 128*kWave, 0, jb.off[e.band + 1] - jb.off[e.band], 0};
  NoDecide nd;
  refb_loops(jb, e.band, e.blk, true, true, lambda, v, nd);
}

__device__ __forceinline__ uint32_t pack_pulses(int s0, int y0, int s1, int y1) {
  return pack16(s0 ? -y0 : y0, s1 ? -y1 : y1);
}

/* One band per group of G lanes (pvq_row.cuh): bands of G*E coefficients (G = 16,
   E = 8: 128; G = 4, E = 8: 32), all state in registers; lane l of the group owns
   positions l*E .. l*E+E-1.  The decisions of a group are uniform over its lanes
   (every lane evaluates them on the same record and items). */
template <int E, int G>
struct RowVector {
  int ax[E];
  unsigned sg;      /* bit e: coefficient e is negative */
  int y[E];
  int row;
  int l;
  int force;
  double xx;
  double norm_1;
  double cxy;       /* sum |x_j|*y_j and sum y_j^2 as the last search of the chain left them */
  double cyy;
  __device__ __forceinline__ void load(const int16_t *src, bool pad) {
    const int16_t *p = src + l*E;
    sg = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int v = p[e];
      ax[e] = abs(v);
      sg |= (unsigned)(v < 0) << e;
      y[e] = 0;
    }
    if (pad && l == G - 1) {
      ax[E - 1] = 0;
      sg &= ~(1u << (E - 1));
    }
    od_row_norm<E, G>(ax, &xx, &norm_1);
  }
  __device__ __forceinline__ double search(int n_true, int k, int prev_k, double g2, double lambda) {
#ifdef ODHIP_EXPERIMENTS
    /* how often the double-precision replay of a greedy pulse fires on real content
       (odhip_exp_row_replay_stats; tools/replay_rate.py) */
    const int placed = prev_k > 0 && prev_k <= k ? prev_k : 0;
    const int greedy = k - (1 + k/4) - placed;
    pulses += greedy > 0 ? greedy : 0;
    /* (an upper bound when k > 2 starts from the projection, which places some pulses itself) */
    rate_pulses += k - placed - (greedy > 0 ? greedy : 0);
    return od_pvq_search_row<E, G>(ax, y, row, l, n_true, k, prev_k, g2, lambda, force, xx, norm_1,
     &cxy, &cyy, &replays);
#else
    return od_pvq_search_row<E, G>(ax, y, row, l, n_true, k, prev_k, g2, lambda, force, xx, norm_1,
     &cxy, &cyy);
#endif
  }
#ifdef ODHIP_EXPERIMENTS
  int replays = 0;
  int pulses = 0;
  int rate_pulses = 0;
#endif
  __device__ __forceinline__ int moment() const {
    int m = 0;
#pragma unroll
    for (int e = 0; e < E; e++) m += (l*E + e)*y[e];
    return grp_sum<G>(m);
  }
  __device__ __forceinline__ void store(int16_t *dst) {
    int16_t *p = dst + l*E;
    if constexpr (E == 8) {
      *reinterpret_cast<uint4 *>(p) = make_uint4(pack_pulses(sg & 1, y[0], sg & 2, y[1]),
       pack_pulses(sg & 4, y[2], sg & 8, y[3]), pack_pulses(sg & 16, y[4], sg & 32, y[5]),
       pack_pulses(sg & 64, y[6], sg & 128, y[7]));
    }
    else {
#pragma unroll
      for (int e = 0; e < E; e += 2) {
        *reinterpret_cast<uint32_t *>(p + e) = pack_pulses(sg & (1u << e), y[e], sg & (2u << e), y[e + 1]);
      }
    }
  }
};

#ifdef ODHIP_EXPERIMENTS
/* [0] greedy pulses placed by the row searches of the with-reference stage, [1] those that took the
   double-precision replay (pvq_row.cuh, point 3), [2] pulses placed by the rate-penalised pass (:192-219),
   [3] bands - counted once per band */
__device__ unsigned long long gRowReplayStats[4];
#endif

/* The row search on plain band vectors (odhip_pvq_search_row_batch): one band per group of G lanes,
   no chain (prev_k = 0).  replays_out[b] = the greedy pulses of band b that the single-precision
   screen could not vouch for and replayed with the literal double-precision scan. */
template <int E, int G>
__global__ __launch_bounds__(kWave) void k_pvq_search_row(const int16_t *x_in, int n_true, const int32_t *k_in,
 od_coeff *y_out, const double *g2_in, double lambda, int force_scan, double *cos_out, int32_t *replays_out,
 long nbands) {
  constexpr int n = E*G;
  constexpr int C = kWave/G;
  od_rsqrt_init(threadIdx.x);
  const int lane = threadIdx.x;
  const int row = lane/G;
  const int l = lane%G;
  const long band = (long)blockIdx.x*C + row;
  const bool live = band < nbands;
  const long b = live ? band : nbands - 1;
  int ax[E];
  int y[E];
  unsigned sg = 0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int j = l*E + e;
    const int v = j < n_true ? x_in[b*n_true + j] : 0;
    ax[e] = abs(v);
    sg |= (unsigned)(v < 0) << e;
    y[e] = 0;
  }
  double xx;
  double norm_1;
  od_row_norm<E, G>(ax, &xx, &norm_1);
  double cxy = 0;
  double cyy = 0;
  int replays = 0;
  int k = k_in[b];
  k = k < 0 ? 0 : k > 32767 ? 32767 : k;
  const double c = od_pvq_search_row<E, G>(ax, y, row, l, n_true, k, 0, g2_in[b], lambda, force_scan, xx, norm_1,
   &cxy, &cyy, &replays);
  if (live) {
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int j = l*E + e;
      if (j < n_true) y_out[band*n_true + j] = sg >> e & 1 ? -y[e] : y[e];
    }
    if (l == 0) {
      cos_out[band] = c;
      if (replays_out) replays_out[band] = replays;
    }
  }
  (void)n;
}

template <int E, int G>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_refb_search_row(RItems it) {
  od_rsqrt_init(threadIdx.x);
  const int item = find_item(it, blockIdx.x);
  const RJob &jb = it.jobs[it.job[item]];
  const int lane = threadIdx.x;
  RowVector<E, G> v;
  v.row = lane/G;
  v.l = lane%G;
  v.force = it.perturb >> 1;
  const long nblocks = jb.nblocks;
  const long pos = (long)(blockIdx.x - it.wg_start[item])*(kWave/G) + v.row;
  const bool live = pos < nblocks;
  /* rows beyond the end redo the last band without storing anything */
  const long blk = jb.ids[(long)it.band[item]*nblocks + (live ? pos : nblocks - 1)];
  NoDecide nd;
  refb_loops(jb, it.band[item], blk, live && v.l == 0, live, it.lambda, v, nd);
}

/* The short bands (N = 15, 8): one band per lane, the band in registers
   (pvq_regs.cuh).  Vectors are read and written as whole 16-byte pieces; the
   15-coefficient band shares its first piece with the unused DC slot. */
template <int N>
struct RegVector {
  static constexpr int SH = N == 15 ? 1 : 0;
  int ax[N];
  unsigned sg;      /* bit i: coefficient i is negative */
  int y[N];
  double xx;
  double norm_1;
  double cxy;       /* sum |x_j|*y_j and sum y_j^2 as the last search of the chain left them */
  double cyy;
  __device__ __forceinline__ void load(const int16_t *src, bool pad) {
    const uint4 *p = reinterpret_cast<const uint4 *>(src - SH);
    sg = 0;
    uint32_t w[(N + SH)/2];
#pragma unroll
    for (int q = 0; q < (N + SH)/8; q++) {
      const uint4 t = p[q];
      w[4*q] = t.x;
      w[4*q + 1] = t.y;
      w[4*q + 2] = t.z;
      w[4*q + 3] = t.w;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
      const int t = (int16_t)(w[(i + SH) >> 1] >> (16*((i + SH) & 1)));
      ax[i] = abs(t);
      sg |= (unsigned)(t < 0) << i;
      y[i] = 0;
    }
    if (pad) {
      ax[N - 1] = 0;
      sg &= ~(1u << (N - 1));
    }
    od_regs_norm<N>(ax, &xx, &norm_1);
  }
  __device__ __forceinline__ double search(int n_true, int k, int prev_k, double g2, double lambda) {
    return od_pvq_search_regs<N>(ax, y, n_true, k, prev_k, g2, lambda, xx, norm_1, &cxy, &cyy);
  }
  __device__ __forceinline__ int moment() const {
    int m = 0;
#pragma unroll
    for (int i = 1; i < N; i++) m += i*y[i];
    return m;
  }
  __device__ __forceinline__ void store(int16_t *dst) {
    store_pulses<N>(dst, [&](int i) -> int { return (sg >> i) & 1 ? -y[i] : y[i]; });
  }
};

/* One band per GROUP of S lanes (pvq_lane.cuh, S = 2 or 4): the 32- and 128-coefficient bands of the decided
   stage.  Lane l of the group owns coding positions l*NL .. l*NL + NL - 1 as words |x| << 16 | 2*y of its own
   column of `pk` ([NL][kPitch], one array per wavefront); the LaneSearch persists along a chain, so a chained
   search (0 < prev_k <= k) goes on from the pulses and sums the previous one left and any other one starts
   from the projection again.  The interface is RowVector's; `y` reads the lane's pulse counts out of its
   column.  Limits, for any NL*S up to 128 (int16 magnitudes, K <= ODHIP_PVQ_MAX_K = kMaxK = 32767): the sums
   xy <= 32768 K and yy <= K^2 stay below 2^30 and t = xy + |x_j| below 2^31 whatever the band's size; 2*y
   <= 65534 fits the word's low half; moment() is at most 127*32767 < 2^22. */
template <int NY>
struct LeanSigns {     /* one sign bit per position a lane holds (GroupVector, LeanDecide) */
  using type = std::conditional_t<(NY > 32), unsigned long long, unsigned>;
};

template <int NL, int S>
struct GroupVector {
  static_assert(S == 2 || S == 4, "a pair or a quad per band");
  struct Pulses {
    const uint32_t *col;
    __device__ __forceinline__ int operator[](int e) const { return (int)(col[e*kPitch] >> 1 & 0x7fffu); }
  };
  using Signs = typename LeanSigns<NL>::type;
  uint32_t *pk;
  Pulses y;
  Signs sg;         /* bit e: coefficient l*NL + e is negative */
  int lane;
  int l;
  bool force_seq;   /* ODHIP_PVQ_FORCE_SEQ: the group's parts always combined by the sequential rescan */
  LaneSearch st;
  __device__ __forceinline__ void init(uint32_t *columns, int lane_in, bool force) {
    pk = columns;
    y.col = columns + lane_in;
    lane = lane_in;
    l = lane_in & (S - 1);
    force_seq = force;
  }
  __device__ __forceinline__ void load(const int16_t *src, bool pad) {
    static_assert(NL % 8 == 0, "whole 16-byte pieces");
    const uint4 *p = reinterpret_cast<const uint4 *>(src + l*NL);
    sg = 0;
#pragma unroll
    for (int q = 0; q < NL/8; q++) {
      const uint4 t = p[q];
      const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int j = 8*q + e;
        int v = (int16_t)(w[e >> 1] >> (16*(e & 1)));
        if (j == NL - 1 && pad && l == S - 1) v = 0;     /* PAD (od_lane_search): the last position of the last lane */
        pk[j*kPitch + lane] = (uint32_t)abs(v) << 16;
        sg |= (Signs)(v < 0) << j;
      }
    }
    od_lane_prepare<NL, S>(st, pk, lane);
  }
  __device__ __forceinline__ double search(int n_true, int k, int prev_k, double g2, double lambda) {
    const bool fresh = !(prev_k > 0 && prev_k <= k);
    return od_lane_search<NL, S, true>(st, pk, od_rsq_lds, lane, l, true, fresh, k, g2, lambda, force_seq,
     n_true != S*NL);
  }
  __device__ __forceinline__ int moment() const {
    int m = 0;
#pragma unroll
    for (int e = 0; e < NL; e++) m += (l*NL + e)*y[e];
    return od_grp_add<S>(m);
  }
};
template <int NL>
using PairVector = GroupVector<NL, 2>;

/* ---- choice + synthesis -----------------------------------------------------------
   k_refb_choose<N>  one band per lane: the reference's selection among the
                     candidates, the skip rules, and everything of
                     od_pvq_synthesis_partial that is a property of the whole
                     band (sum of squared pulses -> scale, the Householder
                     projection of the synthesised vector), with the band's
                     pulses and reference held as packed 16-byte vectors
   k_refb_synth      one coefficient per thread in coding order: the
                     per-coefficient part (scale, reflection, inverse QM) and
                     od_coding_order_to_raster

   choice[(blk*nb + band)*16 ..]: [0..7] as documented in include/daala_hip.h;
   [8] mode (0 zero, 1 copy the reference, 4 copy the negated reference, 2
   no-reference synthesis, 3 with reference), [9] pulse slot, [10] scale, [11]
   qshift, [12] xm, [13] m, [14] proj_1, [15] outshift. */
__device__ __forceinline__ int neg_interleave(int x, int ref) { /* src/pvq_encoder.c:235-239 */
  if (x < ref) return -2*(x - ref) - 1;
  if (x < 2*ref) return 2*(x - ref);
  return x - 1;
}

__device__ unsigned char gRBandOf[OD_SCAN_LEN];

/* A band spread over a group of G lanes, E positions each (G = 1: the whole band in one lane).
   One lane to the left within the group: 0 into the group's first lane, the lane's own value for G = 1. */
template <int G>
__device__ __forceinline__ int grp_from_prev(int v, int l) {
  if (G == 1) return v;
  if (G == 16) return __builtin_amdgcn_update_dpp(0, v, 0x111 /* row_shr:1 */, 0xf, 0xf, true);
  const int t = G == 2 ? od_pair_swap(v) : row_mov<0x90>(v);     /* the pair's other lane; quad_perm [0,0,1,2] */
  return l == 0 ? 0 : t;
}

/* Sum over the group: the value itself, a pair (pvq_lane.cuh), a quad or a DPP row (pvq_row.cuh). */
template <int G>
__device__ __forceinline__ int grp_total(int v) {
  if constexpr (G == 1) return v;
  else if constexpr (G == 2) return od_grp_add<2>(v);
  else return grp_sum<G>(v);
}

/* After the decision, the part that is a function of uniform values only: the band is listed when a
   comparison was too close, the quantised gain, the skip rules (:611-622), choice words 0-7 and - of a
   skipped band - the whole record.  `writer`: this lane records the band's results. */
struct RefOutcome {
  int qg;
  int skip;
};

template <class R>
__device__ __forceinline__ RefOutcome refb_decide(const RItems &it, int job, const RJob &jb, int band, long blk,
 const R &r, const RefBest &best, bool writer, int4 *ch) {
  const int cfl_enabled = jb.is_keyframe && jb.pli != 0;
  const int noref = best.noref;
  RefOutcome o;
  o.qg = 0;
  int itheta = jb.is_keyframe ? -1 : 0;
  int max_theta = 0;
  int best_k = 0;
  if (best.close && writer) {
    const unsigned slot = atomicAdd(it.pcount, 1u);
    if (slot < (unsigned)kPUncCap) {
      PUncR *e = it.plist + slot;
      e->job = job;
      e->band = band;
      e->blk = (unsigned)blk;
    }
  }
  if (best.chosen >= 0) {
    o.qg = best.gain;
    best_k = best.k;
    if (noref) {
      itheta = -1;
      max_theta = 0;
    }
    else {
      itheta = best.theta;
      max_theta = best.ts;
    }
  }
  const int qg = o.qg;
  /* :611-622 */
  o.skip = 0;
  if (noref) {
    if (qg == 0) o.skip = 1;
  }
  else {
    if (!jb.is_keyframe && qg == 0) o.skip = r.icgr ? 1 : 2;
    if (qg == r.icgr && itheta == 0 && !cfl_enabled) o.skip = 2;
  }
  if (writer) {
    ch[0] = make_int4(best.chosen, qg, noref, itheta);
    ch[1] = make_int4(max_theta, best_k, o.skip, jb.is_keyframe ? (noref ? qg : neg_interleave(qg, r.icgr))
     : (noref ? qg - 1 : neg_interleave(qg + 1, r.icgr + 1)));
  }
  if (o.skip && writer) {
    const int flip = (r.flags & ODHIP_REFBAND_FLIP) != 0;
    ch[2] = make_int4(o.skip == 2 ? (flip ? 4 : 1) : 0, -1, 0, 0);
    ch[3] = make_int4(0, 0, 0, 0);
  }
  return o;
}

/* The Householder pivot and sign of a band, read from the record in memory where refb_finish needs them: the
   job's record, or the lean one of a band the decided stage holds as LeanVals. */
__device__ __forceinline__ void band_pivot(const RItems &, int, const RJob &jb, int band, long blk,
 const odhip_pvq_refband &, int &m, int &s) {
  const odhip_pvq_refband *rec = jb.rec + (blk*jb.nb_bands + band);
  m = rec->m;
  s = rec->s;
}

__device__ __forceinline__ void band_pivot(const RItems &it, int job, const RJob &jb, int band, long blk,
 const LeanVals &, int &m, int &s) {
  const uint32_t w = lean_rec(it, job, jb, blk, band)->msf;
  m = (int)(w & 0xffffu);
  s = (int8_t)(w >> 16);
}

/* Everything after the decision, for lane l of the G that share the band: refb_decide, then what
   od_pvq_synthesis_partial needs of the whole band (:623-633, src/pvq.c:1037-1115).  y(e) = the winner's
   signed pulse at position l*E + e; the decisions are uniform over the group, the band-wide sums are group
   reductions, lane 0 of a `live` group writes the record.  STORE: the lane also writes its pulses to slot 0
   of the job's pulse buffer (the decided stage's group kernels). */
template <int E, int G, bool STORE, class R, class YGet>
__device__ __forceinline__ void refb_finish(const RItems &it, int job, const RJob &jb, int band, long blk,
 const R &r, const RefBest &best, int l, bool live, YGet y) {
  constexpr int SH = E == 15 ? 1 : 0;     /* the 15-coefficient band is read from the DC slot on */
  static_assert(G == 1 || SH == 0, "only a whole band in one lane starts inside a 16-byte piece");
  const bool writer = live && l == 0;
  int4 *ch = reinterpret_cast<int4 *>(jb.choice + (blk*jb.nb_bands + band)*16);
  const RefOutcome o = refb_decide(it, job, jb, band, blk, r, best, writer, ch);
  if (o.skip) return;
  const int noref = best.noref;
  const int yslot = best.yslot;
  const long at = blk*jb.len + jb.off[band] + l*E;
  int wy[E];
#pragma unroll
  for (int e = 0; e < E; e++) wy[e] = y(e);
  if (STORE && live && yslot >= 0) store_pulses<E>(jb.y + at, [&](int e) -> int { return wy[e]; });
  /* od_gain_expand + od_pvq_synthesis_partial (band-wide part) */
  const int32_t g = odq_gain_expand(odq_shl32(o.qg, ODQ_CGAIN_SHIFT) + (noref ? 0 : r.gain_offset),
   job_q(jb, band, blk), jb.beta[band]);
  /* Position n - 1 is no part of a theta winner.  A group's searches keep 0 there (the PAD of od_lane_search
     and of the row searches); a whole band in one lane may come out of a pulse buffer whose last slot was
     not written (LdsVector::store), so it is masked. */
  const int nn = G == 1 ? E - (!noref) : E;
  int yy = 0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int v = e < nn ? wy[e] : 0;
    yy += v*v;
  }
  yy = grp_total<G>(yy);
  const OdSynthScale sy = od_synth_scale(g, yy);
  int32_t scale = sy.scale;
  if (noref) {
    if (writer) {
      ch[2] = make_int4(2, yslot, scale, sy.qshift);
      ch[3] = make_int4(0, 0, 0, 0);
    }
    return;
  }
  int m;
  int s;
  band_pivot(it, job, jb, band, blk, r, m, s);
  /* od_synth_theta (od_pvq_synth.cuh) written out: through the helper the decided searches came out with
     other register numbers, and their text is kept as it was (profiles/synth_once.txt) */
  scale = (int32_t)floor(.5 + (scale*(1./32768))*odq_pvq_sin(best.qtheta));
  const int16_t xm = (int16_t)floor(.5 + ((-s*odq_shr_round(g, sy.gshift))*(1./32768))*odq_pvq_cos(best.qtheta));
  uint32_t rw[(E + SH)/2];
  {
    const uint4 *rp = reinterpret_cast<const uint4 *>(jb.r16 + at - SH);
#pragma unroll
    for (int q = 0; q < (E + SH)/8; q++) {
      const uint4 r4 = rp[q];
      rw[4*q] = r4.x;
      rw[4*q + 1] = r4.y;
      rw[4*q + 2] = r4.z;
      rw[4*q + 3] = r4.w;
    }
  }
  /* position i of the band takes pulse i below the Householder pivot m and pulse i - 1 above (the last
     position is never below m: a whole band in one lane does not select its masked slot) */
  const int yprev = grp_from_prev<G>(wy[E - 1], l);
  int32_t l2r = 0;
  int32_t proj = 0;
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = l*E + e;
    const int ri = (int16_t)(rw[(e + SH) >> 1] >> (16*((e + SH) & 1)));
    const int ysrc = i < m ? wy[e < E - 1 || G > 1 ? e : E - 2] : (e == 0 ? yprev : wy[e > 0 ? e - 1 : 0]);
    const int16_t xi = od_synth_xi(OdSynthExact(scale), i == m, xm, ysrc);
    l2r += odq_mult16_16(ri, ri);
    proj += odq_mult16_16(ri, xi);
  }
  l2r = grp_total<G>(l2r);
  proj = grp_total<G>(proj);
  const OdHouseholder hb = od_householder_back(l2r, proj);
  if (writer) {
    ch[2] = make_int4(3, yslot, scale, sy.qshift);
    ch[3] = make_int4(xm, m, hb.proj_1, hb.outshift);
  }
}

/* PRICE = 0: the host's rate table (or none); 1: od_pvq_rate's closed form (speed > 0,
   src/pvq_encoder.c:247-287) evaluated here from every searched candidate's pulses with the
   device's log - a comparison whose two costs lie within odq_rate_tol of each other is not
   trusted and the band is listed for odhip_pvq_ref_choose_priced_resolve, which prices it
   with the host libm; 2: that second decision (rates given per band). */
template <int N, int PRICE>
__device__ __forceinline__ void refb_choose_band(const RItems &it, int job, const RJob &jb, int band,
 long blk, const double *given) {
  constexpr int SH = N == 15 ? 1 : 0;     /* the 15-coefficient band is read from the DC slot on */
  constexpr int NW = (N + SH)/2;
  const long bi = blk*jb.nb_bands + band;
  const odhip_pvq_refband r = jb.rec[bi];
  const ItemPtr ip = item_ptr(jb, band, blk);
  const double *rate = PRICE == 2 ? given : PRICE == 0 && jb.rate ? jb.rate + bi*(kSlots + 1) : nullptr;
  const double lambda = it.lambda;
  const int off = jb.off[band];
  /* :417-455 (the initial candidate places no pulse and has qg = 0: its rate is 0) */
  double best_cost = r.dist0 + lambda*(rate ? rate[0] : 0.);
  bool close = false;
  int noref = jb.is_keyframe ? 1 : 0;
  int32_t best_qtheta = 0;
  int chosen = -1;
  int yslot = -1;
  /* Every candidate's result and tail vector is requested before the first one is
     looked at (static slots, predicated on the band's candidate count): one exposed
     memory latency per band instead of one per candidate - the loop was a serial chain
     of up to fourteen dependent round trips.  The head {gain, theta, ts, k} is read for
     the winner only. */
  int4 tails[kSlots];
  int dlo[kSlots];
  int dhi[kSlots];
#pragma unroll
  for (int idx = 0; idx < kSlots; idx++) {
    tails[idx] = make_int4(0, 0, 0, -1);
    dlo[idx] = 0;
    dhi[idx] = 0;
    if (idx < r.nitems) {
      tails[idx] = ip.tail[idx*ip.stride];      /* qcg, qtheta, flags, yslot */
      const int4 res = ip.res[idx*ip.stride];   /* cos_dist, dist */
      dlo[idx] = res.z;
      dhi[idx] = res.w;
    }
  }
#pragma unroll
  for (int idx = 0; idx < kSlots; idx++) {
    if (idx >= r.nitems) continue;
    const int4 tail = tails[idx];
    if (!(tail.z & ODHIP_REFITEM_SEARCHED)) continue;
    double cost = __hiloint2double(dhi[idx], dlo[idx]);
    if (PRICE == 1) {
      const int4 hd = ip.head[idx*ip.stride];     /* gain, theta, ts, k */
      const bool with_ref = idx < r.ntheta;
      const int sum = (int)((unsigned)tail.z >> ODHIP_REFITEM_MOMENT_SHIFT);
      cost = cost + lambda*odq_pvq_rate_fast(sum, hd.w, N, hd.x, with_ref ? r.icgr : 0, with_ref ? hd.y : -1,
       with_ref ? hd.z : 0, jb.is_keyframe, jb.pli);
      const double d = cost - best_cost;
      if ((d < 0 ? -d : d) <= it.tol_scale*odq_rate_tol(cost, best_cost)) close = true;
    }
    else cost = cost + lambda*(rate ? rate[1 + idx] : 0.);
    if (idx < r.ntheta ? cost < best_cost : cost <= best_cost) {
      best_cost = cost;
      chosen = idx;
      yslot = tail.w;
      if (idx < r.ntheta) {
        best_qtheta = tail.y;
        noref = 0;
      }
      else noref = 1;
    }
  }
  RefBest best;
  best.best_cost = best_cost;
  best.chosen = chosen;
  best.yslot = yslot;
  best.noref = noref;
  best.qtheta = best_qtheta;
  best.gain = best.theta = best.ts = best.k = 0;
  best.close = PRICE == 1 && close;
  if (chosen >= 0) {
    const int4 head = ip.head[chosen*ip.stride];    /* gain, theta, ts, k */
    best.gain = head.x;
    best.theta = head.y;
    best.ts = head.z;
    best.k = head.w;
  }
  /* the winner's pulses, as packed 16-byte pieces */
  uint32_t yw[NW];
  if (yslot >= 0) {
    const uint4 *yp = reinterpret_cast<const uint4 *>(jb.y + ((long)yslot*jb.nblocks + blk)*jb.len
     + off - SH);
    if constexpr (NW >= 4) {
#pragma unroll
      for (int v = 0; v < NW/4; v++) {
        const uint4 q = yp[v];
        yw[4*v] = q.x;
        yw[4*v + 1] = q.y;
        yw[4*v + 2] = q.z;
        yw[4*v + 3] = q.w;
      }
    }
  }
  else {
#pragma unroll
    for (int v = 0; v < NW; v++) yw[v] = 0;
  }
  refb_finish<N, 1, false>(it, job, jb, band, blk, r, best, 0, true,
   [&](int i) -> int { return (int16_t)(yw[(i + SH) >> 1] >> (16*((i + SH) & 1))); });
}

/* The running choice of a band searched one per lane (RegVector): every searched candidate
   is priced with od_pvq_rate's closed form as it comes out of the search, in the
   reference's order and with its comparisons (`<` for theta candidates, :559; `<=` for the
   no-reference ones, :601), and the winner's signed pulses are kept in registers - what
   k_refb_choose<N, 1> does from the candidate records, without reading them back. */
template <int N>
struct FuseDecide {
  RefBest b;
  int y[N];
  double lambda;
  double tol_scale;
  int icgr;
  int is_keyframe;
  int pli;
  __device__ __forceinline__ void init(const odhip_pvq_refband &r, const RJob &jb, double lam, double tol) {
    b.best_cost = r.dist0;       /* the initial candidate places no pulse: its rate is 0 */
    b.chosen = -1;
    b.yslot = -1;
    b.noref = jb.is_keyframe ? 1 : 0;
    b.qtheta = 0;
    b.gain = b.theta = b.ts = b.k = 0;
    b.close = false;
    lambda = lam;
    tol_scale = tol;
    icgr = r.icgr;
    is_keyframe = jb.is_keyframe;
    pli = jb.pli;
#pragma unroll
    for (int i = 0; i < N; i++) y[i] = 0;
  }
  __device__ __forceinline__ void offer(int idx, bool with_ref, const int4 &h, int32_t qtheta, int slot,
   double dist, int mom, const RegVector<N> &v) {
    const double cost = dist + lambda*odq_pvq_rate_fast(mom, h.w, N, h.x, with_ref ? icgr : 0,
     with_ref ? h.y : -1, with_ref ? h.z : 0, is_keyframe, pli);
    const double d = cost - b.best_cost;
    if ((d < 0 ? -d : d) <= tol_scale*odq_rate_tol(cost, b.best_cost)) b.close = true;
    if (with_ref ? cost < b.best_cost : cost <= b.best_cost) {
      b.best_cost = cost;
      b.chosen = idx;
      b.yslot = slot;
      b.noref = !with_ref;
      if (with_ref) b.qtheta = qtheta;
      b.gain = h.x;
      b.theta = h.y;
      b.ts = h.z;
      b.k = h.w;
#pragma unroll
      for (int i = 0; i < N; i++) y[i] = slot < 0 ? 0 : ((v.sg >> i) & 1 ? -v.y[i] : v.y[i]);
    }
  }
};

/* FUSE: odhip_pvq_ref_bands_priced_multi - the lane also decides its band and writes the
   choice record (the candidate records are still written: a listed band's resolve and the
   theta-margin re-run read them). */
template <int N, bool FUSE>
__global__ __launch_bounds__(kWave) void k_refb_search_regs(RItems it) {
  od_rsqrt_init(threadIdx.x);
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const RJob &jb = it.jobs[job];
  const long pos = (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x;
  if (pos >= jb.nblocks) return;
  const int band = it.band[item];
  const long blk = jb.ids[(long)band*jb.nblocks + pos];
  RegVector<N> v;
  if constexpr (FUSE) {
    const odhip_pvq_refband r = jb.rec[blk*jb.nb_bands + band];
    FuseDecide<N> dec;
    dec.init(r, jb, it.lambda, it.tol_scale);
    refb_loops(jb, band, blk, true, true, it.lambda, v, dec);
    refb_finish<N, 1, false>(it, job, jb, band, blk, r, dec.b, 0, true, [&](int i) -> int { return dec.y[i]; });
  }
  else {
    NoDecide nd;
    refb_loops(jb, band, blk, true, true, it.lambda, v, nd);
  }
}


/* ==== the DECIDED band stage (odhip_pvq_ref_bands_decided_multi) =========================
   With od_pvq_rate's closed form the choice of a band needs nothing but the band itself, so
   the searches make it and NOTHING per candidate ever reaches HBM: no candidate heads (the
   lists are rebuilt in LDS by the kernel that walks them - round 2's candidate kernel wrote
   0.33 GB of them per 16-frame step and the searches read them back one exposed latency per
   candidate), no tail / result vectors, no pulse vector per searched candidate (1.76 GB per
   launch of the 15-coefficient bands alone).  A band costs one 32-byte record (LeanRec, the
   stage's own: the job's 64-byte odhip_pvq_refband is not written) and the vectors its
   candidates need in - xr for theta candidates, x16 for no-reference ones; the preparation
   stores no other -, one 64-byte choice record and the winner's pulses (slot 0 of the job's
   pulse buffer) out.  The resolve paths (theta inside the acos margin, a priced comparison
   inside the log margin: a handful of bands per 10^9) re-run their bands through the
   exporting kernels above, behind k_refb_prep_list, which gives them the job's records and
   vectors of just those bands.

   The pulse part of a candidate's rate is computed once per SEARCH (candidates that reuse a
   pulse vector, :539-544, share it) and .9*log2(ts) once per gain index; both are the very
   doubles odq_pvq_rate_fast forms, joined in its order. */
constexpr int kLeanAux = 12;            /* per band: ts[3], lower[3], .9*log2(ts)[3] (two words each) */

/* od_pvq_rate's pulse part is a function of (sum, k, n) alone and .9*log2(ts) of ts: for the
   small pulse counts nearly every search ends with they are read from tables filled ONCE per
   device by the very functions they replace (k_rate_fill: same code, same device log - the
   values are identical, two logs and two divisions per search become one load).  NR = band
   size; entries [k][sum], k = 1..K, sum = 0..(NR - 1)*K, K = RateTab<NR>::K: the pulse counts the
   chroma bands of a 1080p keyframe reach at the operating points measured (band 0 of the 16x16 and
   32x32 blocks: K up to 95 / 280; the 128-coefficient bands of the 32x32 blocks: up to 47). */
constexpr int kRateTs = 64;
template <int NR> struct RateTab {
  static constexpr int K = NR == 15 ? 128 : NR == 128 ? 64 : NR == 32 ? 48 : 32;
  static constexpr int W = (NR - 1)*K + 1;
  static constexpr int SIZE = (K + 1)*W;
};
__device__ double gRate8[RateTab<8>::SIZE];
__device__ double gRate15[RateTab<15>::SIZE];
__device__ double gRate32[RateTab<32>::SIZE];
/* round 4: the 128-coefficient bands too (4.2 MB): their searches run four bands to a wavefront,
   so the two logs and two divisions were paid once per candidate per FOUR bands */
__device__ double gRate128[RateTab<128>::SIZE];
__device__ double gRateTs[kRateTs];

template <int NR>
__device__ __forceinline__ double *rate_tab(void) {
  return NR == 8 ? gRate8 : NR == 15 ? gRate15 : NR == 32 ? gRate32 : gRate128;
}

template <int NR>
__global__ void k_rate_fill(void) {
  constexpr int W = RateTab<NR>::W;
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i >= RateTab<NR>::SIZE) return;
  const int k = i/W;
  const int sum = i - k*W;
  rate_tab<NR>()[i] = k == 0 ? 0. : odq_pvq_rate_pulses(sum, k, NR);
}

__global__ void k_rate_ts_fill(void) {
  const int ts = threadIdx.x;
  if (ts < kRateTs) gRateTs[ts] = ts > 0 ? odq_pvq_rate_ts(ts) : 0.;
}

template <int NR>
__device__ __forceinline__ double lean_rate_pulses(int sum, int k) {
  if constexpr (NR == 8 || NR == 15 || NR == 32 || NR == 128) {
    if (k <= RateTab<NR>::K) return rate_tab<NR>()[k*RateTab<NR>::W + sum];
  }
  return odq_pvq_rate_pulses(sum, k, NR);
}

__device__ __forceinline__ double lean_rate_ts(int ts) {
  if (ts > 0 && ts < kRateTs) return gRateTs[ts];
  return odq_pvq_rate_ts(ts);
}
constexpr int kLeanWords = kSlots + kLeanAux;

/* The lean kernels run kSearchWaves INDEPENDENT wavefronts per workgroup (wavefront w of workgroup g is
   work unit g*kSearchWaves + w: what a 64-thread workgroup was in rounds 3-5) that share one 1/sqrt
   table; how many of them a CU holds: od_occupancy.cuh. */
constexpr int kSearchWaves = ODHIP_SEARCH_WAVES;
constexpr int kSearchThreads = kSearchWaves*kWave;

/* A band's candidate list in LDS: word s of the band at col[s*stride].  Theta candidate:
   gi | min(k, 65535) << 2 | (j - lower[gi]) << 18 - the low 18 bits order by (k, gain) as
   items_compare does (src/pvq_encoder.c:301-305); no-reference candidate: c | k << 2. */
struct CandList {
  uint32_t *col;
  int stride;
  int ntheta;
  int nitems;
  int gb1;       /* gain index of gi = 0 */
  int gbn;       /* gain index of no-reference candidate 0 */
};

struct ListSink {
  uint32_t *col;
  int stride;
  bool writer;
  int n = 0;
  int lower_cur = 0;
  __device__ __forceinline__ void gain(int gi, int, int ts, int lower) {
    lower_cur = lower;
    if (!writer) return;
    const double l = lean_rate_ts(ts);
    col[(kSlots + gi)*stride] = (uint32_t)ts;
    col[(kSlots + 3 + gi)*stride] = (uint32_t)lower;
    col[(kSlots + 6 + 2*gi)*stride] = (uint32_t)__double2loint(l);
    col[(kSlots + 7 + 2*gi)*stride] = (uint32_t)__double2hiint(l);
  }
  __device__ __forceinline__ void theta(int gi, int, int j, int, int k) {
    const uint32_t c = (uint32_t)gi | (uint32_t)(k < 65535 ? k : 65535) << 2 | (uint32_t)(j - lower_cur) << 18;
    /* stable insertion by (k, gain): glibc's qsort is a stable merge sort at this size */
    int pos = n;
    while (pos > 0) {
      const uint32_t q = col[(pos - 1)*stride];
      if ((q & 0x3ffffu) <= (c & 0x3ffffu)) break;
      if (writer) col[pos*stride] = q;
      pos--;
    }
    if (writer) col[pos*stride] = c;
    n++;
  }
  __device__ __forceinline__ void noref(int c, int, int k) {
    if (writer) col[n*stride] = (uint32_t)c | (uint32_t)(k < 65535 ? k : 65535) << 2;
    n++;
  }
};

/* Every lane that calls this computes the list (uniformly over a group that shares the
   band); `writer` lanes store it. */
__device__ __forceinline__ CandList refb_build_list(const RJob &jb, int band, const LeanVals &r,
 uint32_t *col, int stride, bool writer) {
  ListSink sink;
  sink.col = col;
  sink.stride = stride;
  sink.writer = writer;
  CandList cl;
  cl.col = col;
  cl.stride = stride;
  cl.gb1 = ((r.cg - r.gain_offset) >> ODQ_CGAIN_SHIFT) - 1;
  const int gbn = r.cg >> ODQ_CGAIN_SHIFT;
  cl.gbn = gbn > 1 ? gbn : 1;
  /* the theta candidates first: ListSink::n is their count when the no-reference ones start */
  struct Split {
    ListSink &s;
    int ntheta = -1;
    __device__ __forceinline__ void gain(int gi, int i, int ts, int lower) { s.gain(gi, i, ts, lower); }
    __device__ __forceinline__ void theta(int gi, int i, int j, int ts, int k) { s.theta(gi, i, j, ts, k); }
    __device__ __forceinline__ void noref(int c, int i, int k) {
      if (ntheta < 0) ntheta = s.n;
      s.noref(c, i, k);
    }
  } split{sink};
  refb_enumerate(jb, band, r.cg, r.gain_offset, r.theta, r.flags, r.corr, split);
  cl.nitems = sink.n;
  cl.ntheta = split.ntheta < 0 ? sink.n : split.ntheta;
  return cl;
}

/* A theta candidate's list entry, decoded: gain index i, theta index j of ts. */
struct ThetaCand {
  int gi;
  int i;
  int ts;
  int j;
};

__device__ __forceinline__ ThetaCand theta_cand(const CandList &cl, uint32_t w) {
  ThetaCand c;
  c.gi = (int)(w & 3u);
  c.i = cl.gb1 + c.gi;
  c.ts = (int)cl.col[(kSlots + c.gi)*cl.stride];
  c.j = (int)cl.col[(kSlots + 3 + c.gi)*cl.stride] + (int)(w >> 18);
  return c;
}

/* What a theta candidate is before its search, a function of the band record and the list entry alone:
   quantised gain, quantised theta, od_pvq_cos(theta - qtheta) and whether the candidate is skipped - by
   the gate (:526-531) or because its K does not fit the pulse format. */
struct ThetaGate {
  int32_t qcg;
  int32_t qtheta;
  int cosd;
  bool skip;
};

__device__ __forceinline__ ThetaGate refb_theta_gate(const LeanVals &r, const ThetaCand &c, int k,
 double lambda) {
  ThetaGate g;
  g.qcg = odq_shl32(c.i, ODQ_CGAIN_SHIFT) + r.gain_offset;
  g.qtheta = odq_pvq_compute_theta(c.j, c.ts);
  g.cosd = odq_pvq_cos(r.theta - g.qtheta);
  g.skip = (refb_dist_gate(g.qcg, r.cg, refb_cos_term(g.cosd)) > r.dist0 + 1.0*lambda && k != 0)
   || k > ODHIP_PVQ_MAX_K;
  return g;
}

/* refb_loops_lean takes the four pre-search values of a theta candidate - quantised gain, skipped or not,
   2 - 2cos(theta - qtheta)/32768 and sin(theta)sin(qtheta)/2^30 - from a provider:
     prepare()  whatever the provider does in front of the chain
     skip()     in front of the gathering vote
     values()   gain and sine product of a candidate that is not skipped, in front of its search
     cos_term() behind the search, where :548-552 uses it (formed again there, or kept from values() by
                the providers that would have to read LDS again)
   PreInline: one band per lane, nothing to share - every value is computed where the walk needs it. */
struct PreInline {
  ThetaGate g;
  __device__ __forceinline__ void prepare(const LeanVals &, const CandList &, double) {}
  __device__ __forceinline__ bool skip(const LeanVals &r, const ThetaCand &c, int, int k, double lambda) {
    g = refb_theta_gate(r, c, k, lambda);
    return g.skip;
  }
  __device__ __forceinline__ void values(const LeanVals &r, const ThetaCand &, int, int32_t &qcg,
   double &sin_prod) const {
    qcg = g.qcg;
    sin_prod = refb_sin_prod(odq_pvq_sin(r.theta), odq_pvq_sin(g.qtheta));
  }
  __device__ __forceinline__ double cos_term(const LeanVals &r, int) const {
    return refb_cos_term(odq_pvq_cos(r.theta - g.qtheta));
  }
};

/* A band spread over a group of G lanes: in lock step every lane of the group would compute the gate again
   for every candidate - ~140 instructions each, the same values in all G lanes.  Lane c % G of the group
   computes candidate c once, before the chain, and store(c, gate) puts it into the group's own slice of LDS. */
template <int G, class Store>
__device__ __forceinline__ void refb_prepass(const LeanVals &r, const CandList &cl, double lambda, int l,
 Store store) {
  /* every lane takes part (a group past the end of the item replays its last band) */
  for (int c = l; c < kSlots; c += G) {
    if (c < cl.ntheta) {
      const uint32_t w = cl.col[c*cl.stride];
      store(c, refb_theta_gate(r, theta_cand(cl, w), (int)(w >> 2 & 0xffffu), lambda));
    }
  }
}

/* The slice is the wavefront's own: with several independent wavefronts per workgroup (WAVES > 1, some of
   which may have left already) only this wavefront's LDS writes have to be ordered. */
template <int WAVES>
__device__ __forceinline__ void refb_prepass_fence(void) {
  if constexpr (WAVES == 1) __syncthreads();
  else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

/* k_refb_lean_row: kPreWords words per candidate, the chain reads five of them back. */
constexpr int kPreWords = 6;       /* qcg, skip, (2 - 2cos(theta - qtheta)/32768) lo/hi, sin(theta)sin(qtheta)/2^30 lo/hi */
template <int G, int WAVES>
struct PreLds {
  uint32_t *pre;
  int stride;
  int l;
  double cos = 0;
  __device__ __forceinline__ void prepare(const LeanVals &r, const CandList &cl, double lambda) {
    refb_prepass<G>(r, cl, lambda, l, [&](int c, const ThetaGate &g) {
      const double cos_term = refb_cos_term(g.cosd);
      const double sin_prod = refb_sin_prod(odq_pvq_sin(r.theta), odq_pvq_sin(g.qtheta));
      uint32_t *p = pre + c*kPreWords*stride;
      p[0] = (uint32_t)g.qcg;
      p[stride] = g.skip;
      p[2*stride] = (uint32_t)__double2loint(cos_term);
      p[3*stride] = (uint32_t)__double2hiint(cos_term);
      p[4*stride] = (uint32_t)__double2loint(sin_prod);
      p[5*stride] = (uint32_t)__double2hiint(sin_prod);
    });
    refb_prepass_fence<WAVES>();
  }
  __device__ __forceinline__ bool skip(const LeanVals &, const ThetaCand &, int idx, int, double) const {
    return pre[(idx*kPreWords + 1)*stride] != 0;
  }
  __device__ __forceinline__ void values(const LeanVals &, const ThetaCand &, int idx, int32_t &qcg,
   double &sin_prod) {
    const uint32_t *p = pre + idx*kPreWords*stride;
    qcg = (int32_t)p[0];
    cos = __hiloint2double((int)p[3*stride], (int)p[2*stride]);
    sin_prod = __hiloint2double((int)p[5*stride], (int)p[4*stride]);
  }
  __device__ __forceinline__ double cos_term(const LeanVals &, int) const { return cos; }
};

/* k_refb_lean_pair (a lane pair or quad per band: 32 or 16 bands' slices in a wavefront's LDS): ONE word per
   candidate, the two table values cos(theta - qtheta) | sin(qtheta) << 16 (od_pvq_cos returns an int16), the
   skips as a bit mask in a register; the chain forms the two doubles from them with the operations PreLds
   stores the results of, and the quantised gain from the list entry. */
constexpr int kPrePacked = 1;
template <int G, int WAVES>
struct PrePacked {
  static_assert((G == 2 || G == 4) && kSlots <= 32, "the parts of a group's skip mask");
  uint32_t *pre;
  int stride;
  int l;
  uint32_t skips = 0;       /* bit c = candidate c is skipped */
  double cos = 0;
  __device__ __forceinline__ void prepare(const LeanVals &r, const CandList &cl, double lambda) {
    refb_prepass<G>(r, cl, lambda, l, [&](int c, const ThetaGate &g) {
      skips |= (uint32_t)g.skip << c;
      pre[c*kPrePacked*stride] = ((uint32_t)g.cosd & 0xffffu) | (uint32_t)odq_pvq_sin(g.qtheta) << 16;
    });
    skips = od_grp_or<G>(skips);
    refb_prepass_fence<WAVES>();
  }
  __device__ __forceinline__ bool skip(const LeanVals &, const ThetaCand &, int idx, int, double) const {
    return (skips >> idx & 1u) != 0;
  }
  __device__ __forceinline__ void values(const LeanVals &r, const ThetaCand &c, int idx, int32_t &qcg,
   double &sin_prod) {
    const uint32_t cs = pre[idx*kPrePacked*stride];
    qcg = odq_shl32(c.i, ODQ_CGAIN_SHIFT) + r.gain_offset;
    cos = refb_cos_term((int16_t)(cs & 0xffffu));
    sin_prod = refb_sin_prod(odq_pvq_sin(r.theta), (int16_t)(cs >> 16));
  }
  __device__ __forceinline__ double cos_term(const LeanVals &, int) const { return cos; }
};

/* A list entry's K (ODHIP_REFB_ABL bit 3: every candidate without pulses). */
template <class D>
__device__ __forceinline__ int lean_k(const D &dec, uint32_t w) {
#ifdef ODHIP_EXPERIMENTS
  if (dec.abl & 8) return 0;
#endif
  (void)dec;
  return (int)(w >> 2 & 0xffffu);
}

/* The decided stage's walk over a band's candidate list (refb_loops without a single store:
   candidates from the LDS list, every searched candidate offered to the decider with its rate halves),
   with the searches of a wavefront gathered.  Every lane (or group of lanes that shares a band) walks its
   own candidate list in list order (the skips, searches and offers a lock-step walk by list index would
   make - round 3's form, removed in round 5 - in the same order: the result per band is identical),
   but a lane whose next candidate needs
   a SEARCH waits while any other lane can still advance without one, so a search runs when every
   lane still working is at one.  Lists are sorted by K, not aligned between bands: walking them in
   lock step by index ran a search (~700 instructions beside its pulses) in almost every iteration
   with about half of the lanes idle (0.56-0.62 of the lanes active, SQ_THREAD_CYCLES_VALU /
   SQ_ACTIVE_INST_VALU, tools/gpu_r4_lanes.sh). */
template <int NR, class Pre, class V, class D>
__device__ __forceinline__ void refb_loops_lean(const RJob &jb, int band, long blk, const LeanVals &r,
 const CandList &cl, double lambda, V &v, D &dec, Pre &pre) {
  const int off = jb.off[band];
  const int n = jb.off[band + 1] - off;
  const int len = jb.len;
  const int32_t cg = r.cg;
  pre.prepare(r, cl, lambda);
  if (cl.ntheta > 0) {
    v.load(jb.xr + blk*len + off, true);
    int prev_k = 0;
    bool has = false;
    double cos_dist = 0;
    double prate = 0;
    int idx = 0;
    while (idx < cl.ntheta) {
      const uint32_t w = cl.col[idx*cl.stride];
      const int k = lean_k(dec, w);
      const ThetaCand c = theta_cand(cl, w);
      const bool skip = pre.skip(r, c, idx, k, lambda);
      const bool want = !skip && k != 0 && k != prev_k;
      /* over the lanes still inside the loop; evaluated by all of them */
      const bool others = __any(!want);
      if (want && others) continue;
      idx++;
      if (skip) continue;
      int32_t qcg;
      double sin_prod;
      pre.values(r, c, idx - 1, qcg, sin_prod);
      if (k == 0) {
        cos_dist = 0;
        has = false;
        prate = 0;
      }
      else if (want) {
        cos_dist = v.search(n - 1, k, prev_k, ((qcg*(double)cg)*sin_prod)*kCgainScale2, lambda);
        has = true;
        prate = lean_rate_pulses<NR>(v.moment(), k);
      }
      prev_k = k;
      const double dist = refb_dist_theta(qcg, cg, pre.cos_term(r, idx - 1), sin_prod, cos_dist);
      const double lts = __hiloint2double((int)cl.col[(kSlots + 7 + 2*c.gi)*cl.stride],
       (int)cl.col[(kSlots + 6 + 2*c.gi)*cl.stride]);
      dec.offer(idx - 1, true, c.i, c.j, dist, prate, lts, has, v);
    }
  }
  if (cl.nitems > cl.ntheta) {
    v.load(jb.x16 + blk*len + off, false);
    int prev_k = 0;
    int idx = cl.ntheta;
    while (idx < cl.nitems) {
      const uint32_t w = cl.col[idx*cl.stride];
      const int i = cl.gbn + (int)(w & 3u);
      const int k = lean_k(dec, w);
      const int32_t qcg = odq_shl32(i, ODQ_CGAIN_SHIFT);
      const bool skip = (refb_dist_noref_gate(qcg, cg) > r.dist0 && k != 0) || k > ODHIP_PVQ_MAX_K;
      const bool others = __any(skip);
      if (!skip && others) continue;
      idx++;
      if (skip) continue;
      const double cos_dist = v.search(n, k, prev_k, (qcg*(double)cg)*kCgainScale2, lambda);
      prev_k = k;
      const double prate = lean_rate_pulses<NR>(v.moment(), k);
      dec.offer(idx - 1, false, i, -1, refb_dist_noref(qcg, cg, cos_dist), prate, 0., true, v);
    }
  }
}

/* The running choice over NY pulses held by this lane (the whole band, or its E positions
   of a band spread over a group): the reference's comparisons (`<` theta candidates, :559;
   `<=` no-reference ones, :601) on cost = dist + lambda*rate.  Only the cost, the winner's
   list index and its pulses are carried through the chain; everything else about the winner
   is read back from the list at the end (lean_best). */
template <int NY>
struct LeanDecide {
  double best_cost;
  int chosen;              /* list index, -1 = the initial candidate */
  bool close;              /* a comparison too close for the device's log */
  int y[NY];
  typename LeanSigns<NY>::type sg;
  double lambda;
  double tol_scale;
  int icgr;
  int is_keyframe;
  int pli;
#ifdef ODHIP_EXPERIMENTS
  int abl = 0;
#endif
  __device__ __forceinline__ void init(const LeanVals &r, const RJob &jb, double lam, double tol) {
    best_cost = r.dist0;       /* the initial candidate places no pulse: its rate is 0 */
    chosen = -1;
    close = false;
    lambda = lam;
    tol_scale = tol;
    icgr = r.icgr;
    is_keyframe = jb.is_keyframe;
    pli = jb.pli;
    sg = 0;
#pragma unroll
    for (int i = 0; i < NY; i++) y[i] = 0;
  }
  template <class V>
  __device__ __forceinline__ void offer(int idx, bool with_ref, int i, int j, double dist, double prate,
   double lts, bool has, const V &v) {
    const double rate = odq_pvq_rate_join(prate, lts, i, with_ref ? icgr : 0, with_ref ? j : -1, is_keyframe,
     pli);
    const double cost = dist + lambda*rate;
    const double d = cost - best_cost;
    if ((d < 0 ? -d : d) <= tol_scale*odq_rate_tol(cost, best_cost)) close = true;
    if (with_ref ? cost < best_cost : cost <= best_cost) {
      best_cost = cost;
      chosen = idx;
      sg = v.sg;
#pragma unroll
      for (int e = 0; e < NY; e++) y[e] = has ? v.y[e] : 0;
    }
  }
  __device__ __forceinline__ int signed_y(int e) const {
    return (sg >> e) & 1 ? -y[e] : y[e];
  }
};

/* RefBest of the winner, decoded from the list. */
template <int NY>
__device__ __forceinline__ RefBest lean_best(const LeanDecide<NY> &dec, const CandList &cl, int is_keyframe) {
  RefBest b;
  b.best_cost = dec.best_cost;
  b.chosen = dec.chosen;
  b.yslot = -1;
  b.noref = is_keyframe ? 1 : 0;
  b.qtheta = 0;
  b.gain = b.theta = b.ts = b.k = 0;
  b.close = dec.close;
  if (dec.chosen >= 0) {
    const uint32_t w = cl.col[dec.chosen*cl.stride];
    b.k = (int)(w >> 2 & 0xffffu);
    b.yslot = b.k > 0 ? 0 : -1;     /* the winner's pulses go to slot 0 */
    if (dec.chosen < cl.ntheta) {
      const ThetaCand c = theta_cand(cl, w);
      b.noref = 0;
      b.gain = c.i;
      b.ts = c.ts;
      b.theta = c.j;
      b.qtheta = odq_pvq_compute_theta(b.theta, b.ts);
    }
    else {
      b.noref = 1;
      b.gain = cl.gbn + (int)(w & 3u);
    }
  }
  return b;
}

/* What the kernels of the decided stage share in front of the walk: work unit (wavefront `wave` of the
   workgroup) -> item -> job and band; the lane's place (band `row` of the wavefront's kWave/G, lane l of the
   band's G); the band's block, record, candidate list (built in the wavefront's slice of s_list_w) and
   decider, ablation bits included.  Past the end of an item a lane that holds a whole band (G = 1) has
   nothing to do: false, as for a unit past the last item.  A group there redoes the item's last band without
   storing anything (`live` is false): its lanes take part in the wavefront's votes and lane moves. */
template <int E, int G>
struct LeanBand {
  int wave;
  int lane;
  int row;
  int l;
  int job;
  int band;
  const RJob *jb;
  bool live;
  long blk;
  LeanVals r;
  CandList cl;
  LeanDecide<E> dec;
};

template <int E, int G, int WAVES>
__device__ __forceinline__ bool lean_band(const RItems &it, uint32_t (&s_list_w)[WAVES][kLeanWords*(kWave/G)],
 LeanBand<E, G> &b) {
  constexpr int C = kWave/G;            /* bands per wavefront */
  b.wave = __builtin_amdgcn_readfirstlane(threadIdx.x/kWave);     /* (uniform: keeps the item search scalar) */
  const int unit = blockIdx.x*WAVES + b.wave;
  if (unit >= it.wg_start[it.nitems]) return false;
  const int item = find_item(it, unit);
  b.job = it.job[item];
  b.jb = &it.jobs[b.job];
  b.band = it.band[item];
  b.lane = threadIdx.x%kWave;
  b.row = b.lane/G;
  b.l = b.lane%G;
  const RJob &jb = *b.jb;
  const long nblocks = jb.nblocks;
  const long pos = (long)(unit - it.wg_start[item])*C + b.row;
  b.live = pos < nblocks;
  if (G == 1 && !b.live) return false;
  b.blk = jb.ids[(long)b.band*nblocks + (b.live ? pos : nblocks - 1)];
  b.r = lean_vals(*lean_rec(it, b.job, jb, b.blk, b.band));
  b.cl = refb_build_list(jb, b.band, b.r, s_list_w[b.wave] + b.row, C, b.l == 0);
  b.dec.init(b.r, jb, it.lambda, it.tol_scale);
#ifdef ODHIP_EXPERIMENTS
  b.dec.abl = it.abl;
#endif
  return true;
}

template <int N>
__global__ __launch_bounds__(kSearchThreads) OD_SEARCH_OCC_ATTR void k_refb_lean_lane(RItems it) {
  __shared__ uint32_t s_list_w[kSearchWaves][kLeanWords*kWave];
  OD_SEARCH_VGPR_FLOOR();
  od_rsqrt_init(threadIdx.x);
  LeanBand<N, 1> b;
  if (!lean_band<N, 1, kSearchWaves>(it, s_list_w, b)) return;
  const RJob &jb = *b.jb;
  RegVector<N> v;
  PreInline pre;
  refb_loops_lean<N>(jb, b.band, b.blk, b.r, b.cl, it.lambda, v, b.dec, pre);
  const RefBest best = lean_best(b.dec, b.cl, jb.is_keyframe);
  const auto y = [&](int i) -> int { return b.dec.signed_y(i); };
  /* (a skipped band's pulses are written too: this form always did) */
  if (best.yslot >= 0) store_pulses<N>(jb.y + b.blk*jb.len + jb.off[b.band], y);
  refb_finish<N, 1, false>(it, b.job, jb, b.band, b.blk, b.r, best, 0, true, y);
}

template <int E, int G>
__global__ __launch_bounds__(kSearchThreads) OD_SEARCH_OCC_ATTR void k_refb_lean_row(RItems it) {
  constexpr int C = kWave/G;            /* bands per wavefront */
  __shared__ uint32_t s_list_w[kSearchWaves][kLeanWords*C];
  __shared__ uint32_t s_pre_w[kSearchWaves][kSlots*kPreWords*C];
  OD_SEARCH_VGPR_FLOOR();
  od_rsqrt_init(threadIdx.x);
  LeanBand<E, G> b;
  if (!lean_band<E, G, kSearchWaves>(it, s_list_w, b)) return;
  const RJob &jb = *b.jb;
  RowVector<E, G> v;
  v.row = b.row;
  v.l = b.l;
  v.force = it.perturb >> 1;
  PreLds<G, kSearchWaves> pre = {s_pre_w[b.wave] + b.row, C, b.l};
  refb_loops_lean<G*E>(jb, b.band, b.blk, b.r, b.cl, it.lambda, v, b.dec, pre);
  refb_finish<E, G, true>(it, b.job, jb, b.band, b.blk, b.r, lean_best(b.dec, b.cl, jb.is_keyframe), b.l, b.live,
   [&](int e) -> int { return b.dec.signed_y(e); });
#ifdef ODHIP_EXPERIMENTS
  if (b.live && b.l == 0) {
    if (v.pulses) atomicAdd(&gRowReplayStats[0], (unsigned long long)v.pulses);
    if (v.replays) atomicAdd(&gRowReplayStats[1], (unsigned long long)v.replays);
    if (v.rate_pulses) atomicAdd(&gRowReplayStats[2], (unsigned long long)v.rate_pulses);
    atomicAdd(&gRowReplayStats[3], 1ull);
  }
#endif
}

/* The 32- and 128-coefficient bands of the decided stage a GROUP of S lanes per band (GroupVector), kWave/S
   bands per wavefront: k_refb_lean_row's items, heavy-first order, candidate list, lock-step walk, decider
   and outputs, with the searches of pvq_lane.cuh - the literal scan of NL positions per lane out of its LDS
   column, nothing to screen or replay - and everything that is uniform per band issued once for kWave/S
   bands instead of 16 or 4.  WAVES independent wavefronts per workgroup share the 1/sqrt table.  A
   wavefront's LDS is kLeanWords + kSlots words per band and NL*kPitch words of columns (od_occupancy.cuh):
     <16, 2>  32 bands of 32:   3.5 KB of lists, 2 KB of `pre`,  4 KB of columns
     <32, 4>  16 bands of 128: 1.75 KB,          1 KB,           8 KB
     <64, 2>  32 bands of 128:  3.5 KB,          2 KB,          16 KB
   (The kernel keeps the name of its first geometry; S = 4 is a quad.)  The default build compiles <16, 2> and
   the 128-coefficient form ODHIP_GROUP128_LANES names, the experiments build all three (group_lanes). */
constexpr int kGroup128Lanes = ODHIP_GROUP128_LANES;
static_assert(kGroup128Lanes == 4 || kGroup128Lanes == 2, "a quad or a pair per 128-coefficient band");

/* Wavefronts per workgroup of a geometry (the occupancy attribute beside it: OD_GROUP_OCC_ATTR). */
template <int NL, int S>
constexpr int kGroupWaves = NL*S == 32 ? ODHIP_PAIR_WAVES : S == 4 ? ODHIP_GROUP128_WAVES : ODHIP_GROUP128_PAIR_WAVES;

template <int NL, int S>
__global__ __launch_bounds__((kGroupWaves<NL, S>*kWave)) OD_GROUP_OCC_ATTR(NL, S) void k_refb_lean_pair(RItems it) {
  constexpr int G = S;
  constexpr int WAVES = kGroupWaves<NL, S>;
  constexpr int C = kWave/G;            /* bands per wavefront */
  static_assert(kRsqN == OD_RSQ_TABLE_N && kPitch == kWave, "od_lane_search on this unit's table and columns");
  __shared__ uint32_t s_list_w[WAVES][kLeanWords*C];
  __shared__ uint32_t s_pre_w[WAVES][kSlots*kPrePacked*C];
  __shared__ uint32_t s_pk_w[WAVES][NL*kPitch];
  OD_SEARCH_VGPR_FLOOR();
  od_rsqrt_init(threadIdx.x);
  LeanBand<NL, G> b;
  if (!lean_band<NL, G, WAVES>(it, s_list_w, b)) return;
  const RJob &jb = *b.jb;
  GroupVector<NL, S> v;
  v.init(s_pk_w[b.wave], b.lane, (it.perturb >> 1) != 0);
  PrePacked<G, WAVES> pre = {s_pre_w[b.wave] + b.row, C, b.l};
  refb_loops_lean<G*NL>(jb, b.band, b.blk, b.r, b.cl, it.lambda, v, b.dec, pre);
  refb_finish<NL, G, true>(it, b.job, jb, b.band, b.blk, b.r, lean_best(b.dec, b.cl, jb.is_keyframe), b.l, b.live,
   [&](int e) -> int { return b.dec.signed_y(e); });
}

/* The bands a theta-margin re-run rebuilt (records, candidates and pulses of every slot, by
   the exporting kernels) decided from those records, as k_refb_choose<N, 1> does. */
template <int N>
__global__ __launch_bounds__(kWave) void k_refb_choose_unc_list(RItems it, const Unc *list, int count) {
  const int i = blockIdx.x*kWave + threadIdx.x;
  if (i >= count) return;
  const Unc e = list[i];
  const RJob &jb = it.jobs[e.job];
  if (jb.off[e.band + 1] - jb.off[e.band] != N) return;
  refb_choose_band<N, 1>(it, e.job, jb, e.band, e.blk, nullptr);
}

template <int N, int PRICE>
__global__ __launch_bounds__(kWave) void k_refb_choose(RItems it) {
  const int item = find_item(it, blockIdx.x);
  const int job = it.job[item];
  const RJob &jb = it.jobs[job];
  const long blk = (long)(blockIdx.x - it.wg_start[item])*kWave + threadIdx.x;
  if (blk >= jb.nblocks) return;
  refb_choose_band<N, PRICE>(it, job, jb, it.band[item], blk, nullptr);
}

/* The listed bands of size N decided again with the host's rates. */
template <int N>
__global__ __launch_bounds__(kWave) void k_refb_choose_list(RItems it, const PUncR *list, int count) {
  const int i = blockIdx.x*kWave + threadIdx.x;
  if (i >= count) return;
  const PUncR *e = list + i;
  const RJob &jb = it.jobs[e->job];
  if (jb.off[e->band + 1] - jb.off[e->band] != N) return;
  refb_choose_band<N, 2>(it, e->job, jb, e->band, e->blk, e->rate);
}

/* Eight consecutive coding positions of one block per thread into the dequantised plane
   (od_ref_chunk, od_pvq_synth.cuh). */
__global__ __launch_bounds__(256) void k_refb_synth(RItems it) {
  const int item = find_item(it, blockIdx.x);
  const RJob &jb = it.jobs[it.job[item]];
  const int len = jb.len;
  const int cpb = len >> 3;                       /* chunks per block */
  const long t = (long)(blockIdx.x - it.wg_start[item])*256 + threadIdx.x;
  const long blk = t/cpb;
  if (blk >= jb.nblocks) return;
  const int c0 = (int)(t - blk*cpb) << 3;
  const long base = block_base(jb, blk);
  const int band = gRBandOf[c0 ? c0 : 1];
  od_ref_chunk<OdSynthExact>(OdPlaneSink{jb.dq + base, jb.w}, reinterpret_cast<const int4 *>(jb.choice + (blk*jb.nb_bands + band)*16),
   c0, jb.off[band], len, blk, jb.nblocks, jb.coef + base, jb.ref + base, jb.w, jb.y, jb.r16, jb.qm_inv, gRScanPk);
}

/* ---- host side --------------------------------------------------------------------- */
odhip_device_once g_tables_once;

int upload_tables_now(void) {
  ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(kRScanXY), OD_SCAN_XY, sizeof(OD_SCAN_XY)));
  unsigned short packed[OD_SCAN_LEN];
  for (int j = 0; j < OD_SCAN_LEN; j++) packed[j] = (unsigned short)(OD_SCAN_XY[j][1] << 8 | OD_SCAN_XY[j][0]);
  ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gRScanPk), packed, sizeof(packed)));
  unsigned char band_of[OD_SCAN_LEN];
  for (int j = 0; j < OD_SCAN_LEN; j++) {
    int b = 0;
    while (b + 1 < OD_NBANDS[4] && j >= OD_BAND_OFFS[4][b + 1]) b++;
    band_of[j] = (unsigned char)b;
  }
  ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gRBandOf), band_of, sizeof(band_of)));
  od_rsqrt_fill_launch();
  od_rsqrt_huge_fill_launch();
  k_rate_fill<8><<<(RateTab<8>::SIZE + 255)/256, 256, 0, 0>>>();
  k_rate_fill<15><<<(RateTab<15>::SIZE + 255)/256, 256, 0, 0>>>();
  k_rate_fill<32><<<(RateTab<32>::SIZE + 255)/256, 256, 0, 0>>>();
  k_rate_fill<128><<<(RateTab<128>::SIZE + 255)/256, 256, 0, 0>>>();
  k_rate_ts_fill<<<1, kRateTs, 0, 0>>>();
  ODHIP_TRY(hipDeviceSynchronize());
  return ODHIP_SUCCESS;
}

int upload_tables(void) {
  return odhip_once_per_device(g_tables_once, upload_tables_now);
}

}  // namespace

/* The probes of single device functions on plain vectors: they need the tables and no stage state.  (They
   stand before the stage because a code object lists its kernels in the order of their first launch in
   this file.) */
extern "C" {

int odhip_pvq_ref_theta_probe(const double *d_corr, double *d_t, long n, odhip_stream stream) {
  if (!d_corr || !d_t || n < 0) return ODHIP_EINVAL;
  if (n == 0) return ODHIP_SUCCESS;
  k_theta_probe<<<(unsigned)((n + kWave - 1)/kWave), kWave, 0, (hipStream_t)stream>>>(d_corr, d_t, n);
  return odhip_check_launch();
}

/* pvq_search_rdo_double (src/pvq_encoder.c:93-224) in its ROW form - what the 32- and 128-coefficient
   bands of the with-reference stage run (pvq_row.cuh) - on plain band vectors. */
int odhip_pvq_search_row_batch(const int16_t *d_x, int n, const int32_t *d_k, od_coeff *d_y,
 const double *d_g2, double pvq_norm_lambda, int force_scan, double *d_cos, int32_t *d_replays, long nbands,
 odhip_stream stream) {
  if (!d_x || !d_k || !d_y || !d_g2 || !d_cos || nbands < 0) return ODHIP_EINVAL;
  if (n != 31 && n != 32 && n != 127 && n != 128) return ODHIP_EINVAL;
  if (nbands == 0) return ODHIP_SUCCESS;
  const int rc = upload_tables();
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int per_wg = n >= 127 ? 4 : 16;
  const long grid = (nbands + per_wg - 1)/per_wg;
  if (grid > 0x7fffffffL) return ODHIP_EINVAL;
  if (n >= 127) {
    k_pvq_search_row<8, 16><<<(unsigned)grid, kWave, 0, s>>>(d_x, n, d_k, d_y, d_g2, pvq_norm_lambda, force_scan, d_cos,
     d_replays, nbands);
  }
  else {
    k_pvq_search_row<8, 4><<<(unsigned)grid, kWave, 0, s>>>(d_x, n, d_k, d_y, d_g2, pvq_norm_lambda, force_scan, d_cos,
     d_replays, nbands);
  }
  return odhip_check_launch();
}

}  // extern "C"

namespace {

int fill_job(RJob &d, const odhip_pvq_refjob &j, JobMode mode) {
  if (!j.d_coef || (!j.d_ref && !j.luma) || !j.band || !j.items || !j.y || !j.r16) return ODHIP_EINVAL;
  if (((uintptr_t)j.band & 63) || ((uintptr_t)j.items & 15) || ((uintptr_t)j.y & 15)
   || ((uintptr_t)j.r16 & 15) || ((uintptr_t)j.x16 & 15) || ((uintptr_t)j.xr & 15)
   || ((uintptr_t)j.choice & 15)) {
    return ODHIP_EINVAL;
  }
  if (mode == kJobBands ? (!j.d_qm || !j.x16 || !j.xr) : mode == kJobSynth ? (!j.d_qm_inv || !j.choice || !j.d_dq)
   : !j.choice) {
    return ODHIP_EINVAL;
  }
  /* 16-byte row loads of the coefficient and reference planes */
  if (mode == kJobBands && (((uintptr_t)j.d_coef & 15) || ((uintptr_t)j.d_ref & 15))) return ODHIP_EINVAL;
  if (j.luma && !j.d_ref && mode == kJobSynth) return ODHIP_EINVAL;   /* the synthesis into planes may copy the reference */
  memset(&d, 0, sizeof(d));
  d.coef = j.d_coef;
  d.ref = j.d_ref;
  d.qm = j.d_qm;
  d.qm_inv = j.d_qm_inv;
  d.rec = j.band;
  d.items = j.items;
  d.y = j.y;
  d.r16 = j.r16;
  d.x16 = j.x16;
  d.xr = j.xr;
  d.rate = j.d_rate;
  d.choice = j.choice;
  d.dq = j.d_dq;
  const int rc = fill_geometry(d, j, true);
  if (rc) return rc;
  d.is_keyframe = j.is_keyframe != 0;
  d.pli = j.pli;
  if (j.luma) {
    /* the luma level one size up over the same grid of blocks (4:2:0), or the same level over
       the same planes (4:4:4), nplanes or nplanes / 2 planes (Cb and Cr share the prediction).
       Both read the luma block's coding positions c0 .. c0 + 7 of the same band (lref_piece):
       the whole block at the same level, its nested upper-left quarter one size up */
    const odhip_pvq_job &l = *j.luma;
    const bool up = l.bs == j.bs + 1 && l.w == 2*j.w && l.h == 2*j.h;
    const bool same = l.bs == j.bs && l.w == j.w && l.h == j.h;
    if ((!up && !same) || !l.cands.y || !l.cands.choice || !l.d_qm_inv
     || (l.nplanes != j.nplanes && 2*l.nplanes != j.nplanes) || !j.is_keyframe || j.pli == 0
     || ((uintptr_t)l.cands.y & 15) || ((uintptr_t)l.cands.choice & 15) || ((uintptr_t)l.d_qm_inv & 15)) {
      return ODHIP_EINVAL;
    }
    const int ln = 4 << l.bs;
    d.ly = l.cands.y;
    d.lchoice = l.cands.choice;
    d.lqmi = l.d_qm_inv;
    d.lsplit = (long)l.nplanes*d.bw*d.bh;
    d.lnblocks = d.lsplit;
    d.llen = ln*ln < OD_SCAN_LEN ? ln*ln : OD_SCAN_LEN;
    d.lnb = OD_NBANDS[l.bs];
  }
  return ODHIP_SUCCESS;
}

/* Everything the stage keeps between calls, owned by the calling thread's current
   context: ONE call sequence (bands -> resolve -> choice / synthesis) may be in
   flight per context. */
struct RefState {
  long theta_listed = 0;             /* bands found inside the acos margin so far (recomputed on the host) */
  JobTables<RJob, kMaxJobs> tabs;    /* device job tables, cached by content        */
  /* [0] bands inside the theta margin, [1] priced choice: bands too close to call on the device - adjacent,
     so that one memset clears both per band stage; [2] bands above ODHIP_PVQ_MAX_K, cleared only by
     od_k_range_take_ref */
  Counters<3> counters;
  DeviceBuf<Unc> unc;                /* the list of counters[0] [kUncCap]           */
  DeviceBuf<PUncR> plist;            /* the list of counters[1] [kPUncCap]          */
  DeviceBuf<LeanRec> lean_rec;       /* the decided stage's band records, grown on its stream ... */
  long lean_at[kMaxJobs] = {};       /* ... and where each job's start (RItems::lean_at)          */
  PinnedCount unc_posted;            /* counters[0] behind the band stage           */
  PinnedCount priced;                /* counters[1] behind the priced choice        */
  BlockSort<kSortBins, kSortChunk, RJob, kMaxItems> sort;   /* + sort keys, sorted ids */
  SideStreams streams;               /* searches of the four band sizes             */
  ProfEvents prof;                   /* odhip_pvq_ref_profile                       */
  double margin = kDefaultMargin;    /* test hooks of the context */
  int perturb = 0;
  double tol_scale = 1.;
  bool lean = false;                 /* the last band stage was the decided one: no
                                        candidate records exist unless a resolve re-ran
                                        the band                                    */
  unsigned *unc_count() const { return counters.d.p; }
  unsigned *pcount() const { return counters.d.p + 1; }
};

int ref_state(RefState **out) {
  ODHIP_CTX_OR_RETURN(ctx);
  RefState *st = odhip_ctx_state<RefState>(ctx, ODHIP_SLOT_REFBANDS);
  if (!st->tabs.d.p) {
    int rc = st->tabs.alloc();
    if (!rc) rc = st->counters.alloc();
    if (!rc) rc = st->unc.alloc(kUncCap);
    if (!rc) rc = st->sort.alloc();
    if (!rc) rc = st->plist.alloc(kPUncCap);
    if (rc) return rc;
  }
  st->streams.serial = ctx->serial != 0;
  /* the context's test hooks (odhip_ctx_set_test_hooks), refreshed per call like `serial` */
  st->margin = ctx->theta_margin > 0 ? ctx->theta_margin : kDefaultMargin;
  st->perturb = ctx->theta_perturb != 0;
  st->tol_scale = ctx->price_tol_scale > 0 ? ctx->price_tol_scale : 1.;
  *out = st;
  return ODHIP_SUCCESS;
}
#define REF_STATE_OR_RETURN(st) STAGE_STATE_OR_RETURN(RefState, ref_state, st)

/* fill_job zeroes every host job first: the table cache compares jobs by content (od_band_stage.cuh) */
int stage_jobs(RefState &st, const odhip_pvq_refjob *jobs, int njobs, JobMode mode, RJob *host,
 hipStream_t s) {
  if (!jobs || njobs <= 0 || njobs > kMaxJobs) return ODHIP_EINVAL;
  int rc = upload_tables();
  if (rc) return rc;
  for (int i = 0; i < njobs; i++) {
    rc = fill_job(host[i], jobs[i], mode);
    if (rc) return rc;
    host[i].krange = st.counters.d.p + 2;
  }
  if (mode == kJobBands) {
    rc = st.sort.place(host, njobs, s);
    if (rc) return rc;
  }
  return st.tabs.upload(host, njobs, s);
}

/* Weights of the work class (KeySink::work), quarters: pulses, candidates, searches.
   ODHIP_SORT_W="p,c,s" overrides them (experiments). */
int sort_weights(void) {
  static const int w = [] {
    int p = 4, c = 4, s = 8;
    const char *e = ODHIP_EXP_ENV("ODHIP_SORT_W");
    if (e) sscanf(e, "%d,%d,%d", &p, &c, &s);
    return (p & 255) | (c & 255) << 8 | (s & 255) << 16;
  }();
  return w;
}

void items_begin(RItems &it, const RefState &st, double lambda) {
  memset(&it, 0, sizeof(it));
  it.lambda = lambda;
  it.margin = st.margin;
  it.perturb = st.perturb;
  it.jobs = st.tabs.cur;
  it.unc_count = st.unc_count();
  it.unc = st.unc.p;
  it.pcount = st.pcount();
  it.plist = st.plist.p;
  it.tol_scale = st.tol_scale;
  it.sort_weights = sort_weights();
  it.lean = st.lean_rec.p;
  for (int j = 0; j < kMaxJobs; j++) it.lean_at[j] = st.lean_at[j];
#ifdef ODHIP_EXPERIMENTS
  /* bit 0: the preparation kernels do not store x16 / r16 / xr; 1: they take a zero reference instead of reading the
     luma choices (lref_piece); 2: they do not write the band record (the decided stage: its lean record); 3: the deciding searches (k_refb_lean_lane,
     k_refb_lean_row, k_refb_lean_pair) place no pulse (K = 0 for every candidate); 4: k_refb_lean_lane does not load
     its vectors.  Timing only: results are wrong. */
  static const int abl = [] {
    const char *e = getenv("ODHIP_REFB_ABL");
    return e ? atoi(e) : 0;
  }();
  it.abl = abl;
#endif
}

/* The three generations of the band stage; the value is what the kernels read as RItems::fuse. */
enum RefStage {
  kStageRecords = 0,      /* candidate records for a later choice                    */
  kStageLanePriced = 1,   /* the bands searched one per lane are decided in place    */
  kStageDecided = 2       /* every band is decided in place: no records (st.lean)    */
};

/* The per-lane bands of every block first, one item per job (band 0 decides the chroma-from-luma flip
   of the block), then the 32- / 128-coefficient bands per row. */
void launch_prep(const RefState &st, const RJob *host, int njobs, double lambda, RefStage stage, hipStream_t s) {
  RItems pi;
  /* size 0: one item per job */
  const auto prep = [&](void (*kernel)(RItems), int size, long per_wg) {
    items_begin(pi, st, lambda);
    pi.fuse = stage;
    if (size) items_add_size(pi, host, njobs, size, per_wg, 1);
    else for (int j = 0; j < njobs; j++) items_add(pi, j, 0, (host[j].nblocks + per_wg - 1)/per_wg);
    if (pi.nitems) kernel<<<pi.wg_start[pi.nitems], kWave, 0, s>>>(pi);
  };
#ifdef ODHIP_EXPERIMENTS
  /* ODHIP_REFB_PREP_SPLIT: band 0 of every block, then bands 1 and 2 as items of a second launch */
  static const bool split = getenv("ODHIP_REFB_PREP_SPLIT") != nullptr;
  if (split) {
    prep(k_refb_prep_lane<15>, 0, kWave);
    prep(k_refb_prep_lane<8>, 8, kWave);
  }
  else
#endif
  prep(k_refb_prep_corner, 0, kWave);
  prep(k_refb_prep_row<8, 4>, 32, 16);
  prep(k_refb_prep_row<8, 16>, 128, 4);
}

/* Counting sort of every item's blocks by work class: the step between the preparation and the searches. */
int sort_blocks(RefState &st, const RJob *host, int njobs, hipStream_t s) {
  return st.sort.run(host, st.tabs.cur, njobs, s);
}

/* The searches of one band size: the 128-coefficient bands one band per 16-lane row, the 32-coefficient ones
   per quad - in the decided stage both per lane GROUP, a quad and a pair (group_lanes) -, 15 and 8 one per
   lane.  `on` indexes {the caller's stream, side[0], side[1]}. */
struct RefSearch {
  int size;
  int on;
  int per_wg;    /* blocks per workgroup */
  bool row;
};
constexpr RefSearch kRefSearches[4] = {{128, 0, 4, true}, {32, 1, 16, true}, {15, 2, kWave, false},
 {8, 2, kWave, false}};

/* Lanes per band of the group search (k_refb_lean_pair, kWave/lanes bands to a wavefront) that serves this size
   in this stage; 0: none, the row / lane kernels do.
   32 coefficients, decided stage: a pair; ODHIP_REFB_ROW32 (experiments build) keeps them in
   k_refb_lean_row<8, 4>, the form they left: the cross-check of tests/test_gpu_refb_pair32.py.
   128 coefficients, decided stage: kGroup128Lanes in the default build, always.  The experiments build
   DIFFERS: it is the build that carries the row searches' replay counters (gRowReplayStats, what
   tests/test_gpu_pvq_corpus_decided.py reads of the single-precision screen inside the stage), so there
   these bands stay in k_refb_lean_row<8, 16> unless ODHIP_REFB_GROUP128=4 (a quad per band) or =2 (a pair)
   asks for a group search: the cross-check of tests/test_gpu_refb_group128.py. */
int group_lanes(const RefSearch &r, RefStage stage) {
  if (stage != kStageDecided) return 0;
  if (r.size == 32) {
    static const bool row32 = ODHIP_EXP_ENV("ODHIP_REFB_ROW32") != nullptr;
    return row32 ? 0 : 2;
  }
  if (r.size == 128) {
#ifdef ODHIP_EXPERIMENTS
    static const int lanes = [] {
      const char *e = ODHIP_EXP_ENV("ODHIP_REFB_GROUP128");
      const int v = e ? atoi(e) : 0;
      return v == 4 || v == 2 ? v : 0;
    }();
    return lanes;
#else
    return kGroup128Lanes;
#endif
  }
  return 0;
}

void launch_search(RefState &st, RItems &it, const RefSearch &r, RefStage stage, hipStream_t s) {
  if (stage == kStageDecided) items_heavy_first(it);
  const int wgs = it.wg_start[it.nitems];
  const int groups = (wgs + kSearchWaves - 1)/kSearchWaves;
  /* the row kernels exist for 128 and 32 coefficients, the lane kernels for 15 and 8, the group kernels for 32 and 128 */
  const auto regs = [&](auto priced) {
    for_band_size(r.size, [&](auto size) {
      constexpr int N = decltype(size)::value;
      if constexpr (N <= 15) k_refb_search_regs<N, decltype(priced)::value><<<wgs, kWave, 0, s>>>(it);
    });
  };
  const int lanes = group_lanes(r, stage);
  const auto group = [&](auto nl, auto lanes_c) {
    constexpr int NL = decltype(nl)::value;
    constexpr int S = decltype(lanes_c)::value;
    constexpr int W = kGroupWaves<NL, S>;
    k_refb_lean_pair<NL, S><<<(wgs + W - 1)/W, W*kWave, 0, s>>>(it);
  };
  const auto launch = [&] {
    if (lanes && r.size == 32) group(std::integral_constant<int, 16>(), std::integral_constant<int, 2>());
#if defined(ODHIP_EXPERIMENTS) || ODHIP_GROUP128_LANES == 4
    else if (lanes == 4) group(std::integral_constant<int, 32>(), std::integral_constant<int, 4>());
#endif
#if defined(ODHIP_EXPERIMENTS) || ODHIP_GROUP128_LANES == 2
    else if (lanes == 2) group(std::integral_constant<int, 64>(), std::integral_constant<int, 2>());
#endif
    else if (r.row) {
      for_band_size(r.size, [&](auto size) {
        constexpr int N = decltype(size)::value;
        if constexpr (N >= 32) {
          if (stage == kStageDecided) k_refb_lean_row<8, N/8><<<groups, kSearchThreads, 0, s>>>(it);
          else k_refb_search_row<8, N/8><<<wgs, kWave, 0, s>>>(it);
        }
      });
    }
    else if (stage == kStageDecided) {
      for_band_size(r.size, [&](auto size) {
        constexpr int N = decltype(size)::value;
        if constexpr (N <= 15) k_refb_lean_lane<N><<<groups, kSearchThreads, 0, s>>>(it);
      });
    }
    else if (stage == kStageLanePriced) regs(std::true_type());
    else regs(std::false_type());
  };
  /* odhip_pvq_ref_profile times the dominant kernel of the stage */
  if (r.size == 128) st.prof.around(s, launch);
  else launch();
}

int launch_searches(RefState &st, const RJob *host, int njobs, double lambda, RefStage stage, hipStream_t s) {
  const bool lane_only = stage != kStageDecided && ODHIP_EXP_ENV("ODHIP_PVQ_REF_LANE") != nullptr;
  hipStream_t side[2] = {s, s};
  if (st.streams.fork(s, side) != ODHIP_SUCCESS) return ODHIP_EFAULT;
  const hipStream_t streams[3] = {s, side[0], side[1]};
  RItems it;
  for (const RefSearch &r : kRefSearches) {
    items_begin(it, st, lambda);
    if (r.row && !lane_only && odhip_env_force_seq()) it.perturb |= 2;   /* every greedy pulse by the literal scan */
    const int lanes = group_lanes(r, stage);
    items_add_size(it, host, njobs, r.size, lane_only ? kWave : lanes ? kWave/lanes : r.per_wg);
    if (it.nitems && !lane_only) launch_search(st, it, r, stage, streams[r.on]);
#ifdef ODHIP_EXPERIMENTS
    /* ODHIP_PVQ_REF_LANE: every size one band per lane with its vectors in LDS (rounds 1-2) */
    if (it.nitems && lane_only) {
      k_refb_search<<<it.wg_start[it.nitems], kWave, (size_t)2*r.size*kWave*sizeof(unsigned short), streams[r.on]>>>(it);
    }
#endif
  }
  if (st.streams.join(s, side) != ODHIP_SUCCESS) return ODHIP_EFAULT;
  return ODHIP_SUCCESS;
}

int ref_bands(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda, odhip_stream stream, RefStage stage) {
  hipStream_t s = (hipStream_t)stream;
  REF_STATE_OR_RETURN(st);
  RJob host[kMaxJobs];
  int rc = stage_jobs(st, jobs, njobs, kJobBands, host, s);
  if (rc) return rc;
  ODHIP_TRY(hipMemsetAsync(st.unc_count(), 0, (stage != kStageRecords ? 2 : 1)*sizeof(unsigned), s));
  st.lean = stage == kStageDecided;
  if (st.lean) {
    /* the stage's own band records, job after job */
    size_t recs = 0;
    for (int j = 0; j < njobs; j++) {
      st.lean_at[j] = (long)recs;
      recs += (size_t)host[j].nblocks*host[j].nb_bands;
    }
    rc = st.lean_rec.grow(recs, s);
    if (rc) return rc;
  }
  RItems it;
  items_begin(it, st, pvq_norm_lambda);
  items_add_size(it, host, njobs, 0, kWave);
  if (!it.nitems) return ODHIP_SUCCESS;
  launch_prep(st, host, njobs, pvq_norm_lambda, stage, s);
  /* (the decided stage has no candidate kernel: the work classes came from the preparation) */
  if (stage != kStageDecided) k_refb_cands<<<it.wg_start[it.nitems], kWave, 0, s>>>(it);
  rc = sort_blocks(st, host, njobs, s);
  if (rc) return rc;
  rc = launch_searches(st, host, njobs, pvq_norm_lambda, stage, s);
  if (rc) return rc;
  if (stage == kStageDecided) {
    /* both counts of listed bands on their way to the host */
    rc = st.unc_posted.post(st.unc_count(), s);
    if (!rc) rc = st.priced.post(st.pcount(), s);
    if (rc) return rc;
  }
  return odhip_check_launch();
}

/* The listed bands searched again by the exporting kernels, with the theta their list entry names: their
   candidate records and pulses exist afterwards.  The job table is in its band-stage form. */
void rerun_listed(const RefState &st, const Unc *d_list, unsigned n, double lambda, hipStream_t s) {
  k_refb_cands_list<<<(n + kWave - 1)/kWave, kWave, 0, s>>>(st.tabs.cur, d_list, (int)n);
  k_refb_search_list<<<n, kWave, (size_t)2*128*kWave*sizeof(unsigned short), s>>>(st.tabs.cur, d_list, (int)n,
   lambda);
}

/* In front of rerun_listed after the decided stage: the job's records and vectors of the listed bands
   (k_refb_prep_list). */
void prep_listed(const RefState &st, const Unc *d_list, unsigned n, double lambda, hipStream_t s) {
  RItems it;
  items_begin(it, st, lambda);
  it.fuse = kStageRecords;
  it.margin = 0;
  k_refb_prep_list<<<n, kWave, 0, s>>>(it, d_list, (int)n);
}

/* After the decided stage nobody else will choose for the bands a theta resolve re-ran: decided here from
   the records the re-run just wrote (a close call joins the price list, whose count is sent again). */
void decide_listed(RefState &st, const Unc *d_list, unsigned n, double lambda, hipStream_t s) {
  RItems it;
  items_begin(it, st, lambda);
  const unsigned grid = (n + kWave - 1)/kWave;
  for (const int size : kBandSizes) {
    for_band_size(size, [&](auto N) {
      k_refb_choose_unc_list<decltype(N)::value><<<grid, kWave, 0, s>>>(it, d_list, (int)n);
    });
  }
  (void)st.priced.post(st.pcount(), s);
}

/* What follows a record-writing band stage. */
enum RefSelect {
  kSelectSynth,        /* the choice by the records' rates, then the synthesis into planes      */
  kSelectChoice,       /* that choice alone                                                     */
  kSelectPriced,       /* the choice priced on the device, its close calls listed               */
  kSelectPricedRest    /* ... of the 128- and 32-coefficient bands only: the per-lane bands were
                          decided (and their close calls listed) inside
                          odhip_pvq_ref_bands_priced_multi, which also cleared the counter      */
};

int ref_select(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda, hipStream_t s, RefSelect sel) {
  const bool synth = sel == kSelectSynth;
  const bool price = sel == kSelectPriced || sel == kSelectPricedRest;
  REF_STATE_OR_RETURN(st);
  RJob host[kMaxJobs];
  int rc = stage_jobs(st, jobs, njobs, synth ? kJobSynth : kJobChoice, host, s);
  if (rc) return rc;
  for (int j = 0; synth && j < njobs; j++) {
    /* 32x32 and 64x64 blocks code their lowest 512 coefficients only; the rest is what
       od_init_skipped_coeffs leaves (src/state.c:1347-1366): zero on a keyframe, the
       prediction's coefficients on an inter frame */
    if (host[j].bs >= 3) {
      const size_t bytes = sizeof(od_coeff)*(size_t)host[j].nplanes*host[j].w*host[j].h;
      if (host[j].is_keyframe) ODHIP_TRY(hipMemsetAsync(host[j].dq, 0, bytes, s));
      else ODHIP_TRY(hipMemcpyAsync(host[j].dq, host[j].ref, bytes, hipMemcpyDeviceToDevice, s));
    }
  }
  if (sel == kSelectPriced) ODHIP_TRY(hipMemsetAsync(st.pcount(), 0, sizeof(unsigned), s));
  RItems it;
  const auto choose = [&](int n, auto priced) {
    for_band_size(n, [&](auto N) {
      k_refb_choose<decltype(N)::value, decltype(priced)::value><<<it.wg_start[it.nitems], kWave, 0, s>>>(it);
    });
  };
  for (int i = 0; i < (sel == kSelectPricedRest ? 2 : 4); i++) {
    items_begin(it, st, pvq_norm_lambda);
    items_add_size(it, host, njobs, kBandSizes[i], kWave);
    if (!it.nitems) continue;
    if (price) choose(kBandSizes[i], std::true_type());
    else choose(kBandSizes[i], std::false_type());
  }
  if (price) {
    const int rcp = st.priced.post(st.pcount(), s);
    if (rcp) return rcp;
  }
  if (!synth) return odhip_check_launch();
  items_begin(it, st, pvq_norm_lambda);
  for (int j = 0; j < njobs; j++) items_add(it, j, 0, (host[j].nblocks*(host[j].len >> 3) + 255)/256);
  k_refb_synth<<<it.wg_start[it.nitems], 256, 0, s>>>(it);
  return odhip_check_launch();
}

}  // namespace

extern "C" {

/* Profiling aid: HIP events around the dominant kernel of the stage - the
   row-parallel search of the 128-coefficient bands - on the stream it is launched
   on, for the calls of the current context. */
int odhip_pvq_ref_profile(int enable) {
  REF_STATE_OR_RETURN(st);
  return st.prof.enable(enable);
}

int odhip_pvq_ref_profile_read(float *ms, int max_n) {
  REF_STATE_OR_RETURN(st);
  return st.prof.read(ms, max_n);
}

#ifdef ODHIP_EXPERIMENTS
/* out[0] = greedy pulses placed by the row searches of the with-reference band stage since the last
   reset, out[1] = those that took the double-precision replay, out[2] = pulses of the rate-penalised pass,
   out[3] = bands.  Synchronises the device. */
int odhip_exp_row_replay_stats(unsigned long long *out, int reset) {
  if (!out) return ODHIP_EINVAL;
  ODHIP_TRY(hipDeviceSynchronize());
  ODHIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(gRowReplayStats), 4*sizeof(unsigned long long)));
  if (reset) {
    const unsigned long long zero[4] = {0, 0, 0, 0};
    ODHIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gRowReplayStats), zero, sizeof(zero)));
  }
  return ODHIP_SUCCESS;
}
#endif

int odhip_pvq_ref_bands_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  return ref_bands(jobs, njobs, pvq_norm_lambda, stream, kStageRecords);
}

/* The band stage with the priced choice of the bands searched one per lane (the 15- and
   8-coefficient bands, 77 % of all bands) made inside their search kernels; follow with
   odhip_pvq_ref_choose_priced_rest_multi for the 32- and 128-coefficient bands and with
   odhip_pvq_ref_choose_priced_resolve.  A job must carry its choice buffer. */
int odhip_pvq_ref_bands_priced_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  for (int j = 0; jobs && j < njobs; j++) {
    if (!jobs[j].choice) return ODHIP_EINVAL;
  }
  return ref_bands(jobs, njobs, pvq_norm_lambda, stream, kStageLanePriced);
}

/* The whole band stage with the priced choice of EVERY band made inside its search (see
   "the DECIDED band stage" above): choice records and the winners' pulse vectors (slot 0 of
   each job's y) are the only outputs; the candidate arrays of the jobs (items, the other
   slots of y) are scratch of the resolve paths.  The counts of bands inside the theta margin
   and inside the price margin are on their way to the host when this returns; follow with
   odhip_pvq_ref_resolve_finish and odhip_pvq_ref_choose_priced_resolve (both normally find
   nothing and return 0; a band they re-run is decided again by them), then consume the
   choices.  A job must carry its choice buffer. */
int odhip_pvq_ref_bands_decided_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  for (int j = 0; jobs && j < njobs; j++) {
    if (!jobs[j].choice) return ODHIP_EINVAL;
  }
  return ref_bands(jobs, njobs, pvq_norm_lambda, stream, kStageDecided);
}

/* The count of listed bands travels to pinned host memory behind the band stage;
   nothing waits for it here. */
int odhip_pvq_ref_resolve_begin(odhip_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  REF_STATE_OR_RETURN(st);
  return st.unc_posted.post(st.unc_count(), s);
}

/* Bands of the current context found inside the margin of the device acos so far: each one had its theta
   recomputed by the host's libm (odhip_pvq_ref_resolve); the ones whose theta CHANGED are the resolve's return
   value. */
long odhip_pvq_ref_theta_listed(void) {
  RefState *st = nullptr;
  if (ref_state(&st) != ODHIP_SUCCESS) return -1;
  return st->theta_listed;
}

int odhip_pvq_ref_resolve(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda, odhip_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  REF_STATE_OR_RETURN(st);
  std::vector<Unc> list;
  unsigned seen = 0;
  const int count = take_listed(s, st.unc_count(), st.unc.p, kUncCap, "bands inside the theta margin", list, &seen);
  st.theta_listed += seen;
  if (count <= 0) return count;
  /* the reference's own expression with the host libm, src/pvq_encoder.c:478 */
  unsigned nfix = 0;
  for (int i = 0; i < count; i++) {
    const int32_t theta = (int32_t)floor(.5 + (32768*2./M_PI)*acos(list[i].corr));
    if (theta != list[i].theta) {
      list[nfix] = list[i];
      list[nfix].theta = theta;
      nfix++;
    }
  }
  if (nfix == 0) return 0;
  RJob host[kMaxJobs];
  int rc = stage_jobs(st, jobs, njobs, kJobBands, host, s);
  if (rc) return rc;
  if (!listed_jobs_valid(list.data(), nfix, njobs)) return ODHIP_EINVAL;
  DeviceBuf<Unc> d_list;
  if (upload_list(d_list, list.data(), nfix, &s)) return ODHIP_EFAULT;
  if (st.lean) prep_listed(st, d_list.p, nfix, pvq_norm_lambda, s);
  rerun_listed(st, d_list.p, nfix, pvq_norm_lambda, s);
  if (st.lean) decide_listed(st, d_list.p, nfix, pvq_norm_lambda, s);
  rc = odhip_check_launch();
  const hipError_t e = hipStreamSynchronize(s);
  if (rc) return rc;
  if (e != hipSuccess) return ODHIP_EFAULT;
  return (int)nfix;
}

int odhip_pvq_ref_resolve_finish(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  REF_STATE_OR_RETURN(st);
  const int posted = st.unc_posted.wait();
  if (posted <= 0) return posted;
  return odhip_pvq_ref_resolve(jobs, njobs, pvq_norm_lambda, stream);
}

int odhip_pvq_ref_select_synth_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  return ref_select(jobs, njobs, pvq_norm_lambda, (hipStream_t)stream, kSelectSynth);
}

int odhip_pvq_ref_choose_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  return ref_select(jobs, njobs, pvq_norm_lambda, (hipStream_t)stream, kSelectChoice);
}

/* The choice alone with od_pvq_rate's closed form (speed > 0) evaluated on the device from
   every searched candidate's pulses (see refb_choose_band); odhip_pvq_ref_choose_priced_resolve
   waits for the stream and settles the bands whose decision was too close to take from the
   device's log with the host libm.  Returns how many (normally 0) or a negative code. */
int odhip_pvq_ref_choose_priced_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  return ref_select(jobs, njobs, pvq_norm_lambda, (hipStream_t)stream, kSelectPriced);
}

/* After odhip_pvq_ref_bands_priced_multi: the priced choice of the bands it did not decide
   (32 and 128 coefficients, searched one per group of lanes), and the count of listed
   bands of both on its way to the host. */
int odhip_pvq_ref_choose_priced_rest_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  return ref_select(jobs, njobs, pvq_norm_lambda, (hipStream_t)stream, kSelectPricedRest);
}

int odhip_pvq_ref_choose_priced_resolve(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  REF_STATE_OR_RETURN(st);
  const int posted = st.priced.wait();
  if (posted <= 0) return posted;
  std::vector<PUncR> list;
  const int count = take_listed(s, st.pcount(), st.plist.p, kPUncCap, "priced bands inside the decision margin",
   list);
  if (count <= 0) return count;
  RJob host[kMaxJobs];
  int rc = stage_jobs(st, jobs, njobs, kJobChoice, host, s);
  if (rc) return rc;
  if (!listed_jobs_valid(list.data(), count, njobs)) return ODHIP_EINVAL;
  if (st.lean) {
    /* the decided stage kept no candidate records: the listed bands are searched again by
       the exporting kernels (their theta as the record holds it) */
    std::vector<Unc> ul;
    try {
      ul.resize(count);
    }
    catch (const std::bad_alloc &) {
      return ODHIP_EFAULT;
    }
    for (int i = 0; i < count; i++) {
      ul[i].job = list[i].job;
      ul[i].band = list[i].band;
      ul[i].blk = list[i].blk;
      ul[i].theta = -1;
      ul[i].corr = 0;
    }
    DeviceBuf<Unc> d_ul;
    if (upload_list(d_ul, ul.data(), count)) return ODHIP_EFAULT;
    /* the band-stage form of the job table (sort scratch, work vectors) for the re-run, then
       the choice form again */
    RJob host0[kMaxJobs];
    rc = stage_jobs(st, jobs, njobs, kJobBands, host0, s);
    if (rc) return rc;
    prep_listed(st, d_ul.p, count, pvq_norm_lambda, s);
    rerun_listed(st, d_ul.p, count, pvq_norm_lambda, s);
    rc = odhip_check_launch();
    if (hipStreamSynchronize(s) != hipSuccess) rc = ODHIP_EFAULT;
    if (!rc) rc = stage_jobs(st, jobs, njobs, kJobChoice, host, s);
    if (rc) return rc;
  }
  /* every searched candidate's rate with the host libm's log */
  for (PUncR &e : list) {
    const RJob &jb = host[e.job];
    const int n = jb.off[e.band + 1] - jb.off[e.band];
    const long B = jb.nblocks;
    odhip_pvq_refband rec;
    ODHIP_TRY(hipMemcpy(&rec, jb.rec + (long)e.blk*jb.nb_bands + e.band, sizeof(rec), hipMemcpyDeviceToHost));
    const int4 *head = reinterpret_cast<const int4 *>(jb.items) + (long)e.band*kSlots*B + e.blk;
    const int4 *tail = head + (long)jb.nb_bands*kSlots*B;
    for (int c = 0; c <= kSlots; c++) e.rate[c] = 0;
    for (int idx = 0; idx < rec.nitems && idx < kSlots; idx++) {
      int4 hd;
      int4 tl;
      ODHIP_TRY(hipMemcpy(&hd, head + (long)idx*B, sizeof(hd), hipMemcpyDeviceToHost));
      ODHIP_TRY(hipMemcpy(&tl, tail + (long)idx*B, sizeof(tl), hipMemcpyDeviceToHost));
      if (!(tl.z & ODHIP_REFITEM_SEARCHED)) continue;
      const bool with_ref = idx < rec.ntheta;
      const int sum = (int)((unsigned)tl.z >> ODHIP_REFITEM_MOMENT_SHIFT);
      e.rate[1 + idx] = odq_pvq_rate_fast_host(sum, hd.w, n, hd.x, with_ref ? rec.icgr : 0,
       with_ref ? hd.y : -1, with_ref ? hd.z : 0, jb.is_keyframe, jb.pli);
    }
  }
  DeviceBuf<PUncR> d_list;
  if (upload_list(d_list, list.data(), count)) return ODHIP_EFAULT;
  RItems it;
  items_begin(it, st, pvq_norm_lambda);
  const unsigned grid = (count + kWave - 1)/kWave;
  for (const int n : kBandSizes) {
    for_band_size(n, [&](auto size) {
      k_refb_choose_list<decltype(size)::value><<<grid, kWave, 0, s>>>(it, d_list.p, (int)count);
    });
  }
  rc = odhip_check_launch();
  if (hipStreamSynchronize(s) != hipSuccess) rc = ODHIP_EFAULT;
  return rc ? rc : count;
}

int odhip_pvq_k_range_take(unsigned *noref_bands, unsigned *ref_bands) {
  unsigned a = 0;
  unsigned b = 0;
  const int rc = od_k_range_take_noref(&a);
  if (rc) return rc;
  const int rc2 = od_k_range_take_ref(&b);
  if (rc2) return rc2;
  if (noref_bands) *noref_bands = a;
  if (ref_bands) *ref_bands = b;
  return a || b ? ODHIP_ERANGE : ODHIP_SUCCESS;
}

}  // extern "C"

/* od_krange.cuh */
int od_k_range_take_ref(unsigned *count) {
  REF_STATE_OR_RETURN(st);
  return st.counters.take(2, count);
}
