/* pipeline.hip - odhip_pipe: the frame-batch step as ONE C call.

   One step = one pass of the block-transform hot path over F resident 4:2:0 (or,
   with cfg.chroma_444, 4:4:4) pictures (what bench.py times and a frame-parallel
   all-intra encoder would run per batch; round 1 drove it from Python with ~100
   ctypes calls per step):

     luma chain   (context / stream A)       chroma chain (context / stream B)
       od_img_plane_copy_pad                   od_img_plane_copy_pad
       forward pyramid, 5 levels               forward pyramid, 4 levels (4:4:4: 5)
       PVQ band stage, no reference            [wait: references of this step]
       choice                                  PVQ band stage WITH the chroma-from-luma
       chroma-from-luma references  ------>      reference (src/encode.c:1680-1687)
       dequantise + inverse, 5 levels          choice, dequantise + inverse, 4 levels

   The two chains are software-pipelined over steps: the luma chain of step i+1
   overlaps the chroma chain of step i (two reference buffers, events both ways).
   Each chain has its OWN odhip_ctx - scratch, edge strips, job tables and side
   streams are never shared between streams - and the pipe owns every device
   buffer and both streams.

   With cfg.chroma_cfl == 0 chroma goes through the no-reference stage together with
   luma on one stream (round 1's first workload).  Rate tables (the host's od_pvq_rate
   results, one double per candidate) are optional per plane set: without them the
   choice is made on distortion alone.

   4:2:0 chroma level bs takes its reference from luma level bs + 1 (the upper-left
   quarter of the co-located luma block); 4:4:4 chroma is a set of 2F undecimated planes
   whose level bs takes it from luma level bs (the whole block, src/intra.c:95-108).
   Everything else is the same chain at dec 0 over the chroma levels the plane set has:
   PlaneSet.nlev, and chroma jobs / sections 5 .. 5 + nlev - 1.

   Host code only; the kernels are the batched entry points of daala_hip.h. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <initializer_list>
#include <vector>
#include "od_buf.cuh"
#include "od_ctx.cuh"
#include "gen/od_scan_tables.h"

namespace {

constexpr int kStages = ODHIP_PIPE_NSTAGES;
constexpr int kMaxTimed = 4096;

struct PlaneSet {
  int dec;
  int pli;
  int nplanes;
  int w, h;          /* coded plane size */
  int pw, ph;        /* picture size in this plane */
  int nlev;
  uint8_t *pic;      /* the pictures the next step reads: pic_buf[front] */
  uint8_t *pic_buf[2];
  uint8_t *px;
  /* inter mode: the motion-compensated prediction of every picture, its padded plane and
     its pyramid (the reference of every block at every level, mdtmp in the encoder) */
  uint8_t *pred_pic;
  uint8_t *pred_px;
  od_coeff *pred_levels[ODHIP_NBSIZES];
  od_coeff *levels[ODHIP_NBSIZES];
  uint8_t *recon[ODHIP_NBSIZES];
  int16_t *qm[ODHIP_NBSIZES];
  int16_t *qm_inv[ODHIP_NBSIZES];
  int32_t q[ODHIP_NBSIZES][ODHIP_MAX_BANDS];
  /* the chroma set holds F Cb planes, then F Cr planes: per-band steps of the second
     half (pvq_qm_q4[2], src/encode.c:3052-3072) */
  int32_t q2[ODHIP_NBSIZES][ODHIP_MAX_BANDS];
  int plane_split;   /* 0: one table */
  int32_t beta[ODHIP_NBSIZES][ODHIP_MAX_BANDS];
  long nblocks[ODHIP_NBSIZES];
};

/* A ring of host slots handed out step by step (the export ring, the metrics ring): step s, numbered from the call
   that set the ring up, lands in slot s % n and the slot's event follows its last copy.  Steps below `sent` have their
   copies enqueued; take and release walk the steps in order, possibly from another thread (hence atomics). */
struct SlotRing {
  std::vector<hipEvent_t> ev;
  long next = 0;                  /* the step the next odhip_pipe_step starts */
  std::atomic<long> sent{0}, taken{0}, released{0};

  /* the slot of step `next` still holds a step the host has not released */
  bool full() const {
    return next >= released + (long)ev.size();
  }
  /* 1: the oldest untaken step and its slot, complete; 0: none (wait blocks only for a step whose copies are enqueued) */
  int poll(bool wait, long *step, size_t *slot) const {
    const long s = taken;
    if (s >= sent) return 0;
    const size_t i = (size_t)(s % (long)ev.size());
    if (wait) ODHIP_TRY(hipEventSynchronize(ev[i]));
    else {
      const hipError_t e = hipEventQuery(ev[i]);
      if (e == hipErrorNotReady) return 0;
      ODHIP_TRY(e);
    }
    *step = s;
    *slot = i;
    return 1;
  }
  void clear() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
    next = 0;
    sent = taken = released = 0;
  }
  int create(int n) {
    for (int i = 0; i < n; i++) {
      hipEvent_t e = nullptr;
      ODHIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      ev.push_back(e);
    }
    return ODHIP_SUCCESS;
  }
};

/* The columns of a metrics slot, in the slot's order (the table of include/daala_hip.h): a column is there when
   `always`, or when its bit is set, and holds `width` 8-byte entries per value - per plane value (met_values of them),
   or (per_picture) per picture and luma level, the first 5F entries of a column of width 1. */
struct MetricColumn {
  int bit;
  int width;
  bool always;
  bool per_picture;
};
enum { MET_SSE, MET_HVS, MET_SSIM, MET_MSSSIM, MET_FASTSSIM, MET_CIEDE, MET_NCOLS };
const MetricColumn kMetricColumns[MET_NCOLS] = {
  {ODHIP_METRIC_SSE, 1, true, false},
  {ODHIP_METRIC_PSNRHVS, 1, true, false},
  {ODHIP_METRIC_SSIM, 1, false, false},
  {ODHIP_METRIC_MSSSIM, ODHIP_MSSSIM_SCALES, false, false},
  {ODHIP_METRIC_FASTSSIM, ODHIP_FASTSSIM_LEVELS, false, false},
  {ODHIP_METRIC_CIEDE, 1, false, true},
};

}  // namespace

struct odhip_pipe {
  odhip_pipe_config cfg = {};
  int pic_w = 0, pic_h = 0, W = 0, H = 0;
  odhip_ctx *ctx[2] = {};         /* 0: luma chain, 1: chroma chain */
  hipStream_t stream[2] = {};
  bool serial = false;
  PlaneSet set[2] = {};
  int cdec = 1;                   /* chroma decimation: 1 (4:2:0), 0 (cfg.chroma_444) */
  /* [parity]: luma 0..4, chroma (no-reference mode) 5..8 (4:4:4: 5..9).  With chroma from luma the
     chroma chain of step i reads the luma CHOICES of step i (pulses and choice records,
     odhip_pvq_refjob.luma) while the luma chain of step i + 1 already writes the next ones:
     two sets that share everything but those two buffers; otherwise only [0] is used */
  odhip_pvq_job jobs[2][2*ODHIP_NBSIZES] = {};
  int njobs = 0;
  odhip_pvq_refjob refjobs[2][ODHIP_NBSIZES] = {};
  odhip_pvq_refjob interjobs[2][ODHIP_NBSIZES] = {};   /* inter mode: [plane set][level] */
  bool inter_pending[2] = {};
  double *rate[2][ODHIP_NBSIZES] = {};
  hipEvent_t ev_refs[2] = {};
  hipEvent_t ev_used[2] = {};
  long nstep = 0;
  int pending = -1;               /* parity of the step whose theta list is unchecked, -1 */
  long reruns = 0;                /* bands re-run with the host's theta so far */
  long price_reruns = 0;          /* priced choices re-decided with the host libm so far */
  double wait_ms = 0;             /* host time spent waiting for the margin count */
  long k_range = 0;               /* bands above ODHIP_PVQ_MAX_K seen at syncs */
  bool record = false;
  /* odhip_pipe_feed: the pictures of the NEXT step arrive in the back buffers on their
     own stream while the current step computes */
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_fed = nullptr;    /* the back buffers hold the fed pictures */
  hipEvent_t ev_pad[2] = {};      /* the padding kernel of a chain has read its pictures */
  int front = 0;
  bool fed = false;
  /* odhip_pipe_set_export: what a host entropy coder consumes - choice records and pulse vectors of
     every band - leaves for pinned host memory on a third stream, behind the stage that produced it */
  hipStream_t export_stream = nullptr;
  uint8_t *export_host = nullptr;
  /* the packed decisions (export_kernels.hip) of the step being exported, by step parity: the used part of
     the streams of step i leaves while step i + 1 is being packed */
  uint8_t *export_dev[2] = {};
  odhip_export_layout export_lay = {};
  PinnedBuf<odhip_export_header> export_hdr[2];   /* the totals of that step, read by the host one step late */
  hipEvent_t ev_exp_hdr[2] = {};
  hipEvent_t ev_exp_sent[2] = {}; /* the streams of that parity's buffer have left */
  int export_pending = -1;        /* parity of the step whose streams have not been sent yet, -1 */
  long export_stale = 0;          /* steps re-decided by a late resolve after their export had left */
  bool in_flush = false;
  hipEvent_t ev_exp_luma[2] = {}; /* the luma sections of parity [i] are packed */
  /* odhip_pipe_set_export_ring: step s leaves in ring[s % n] (ring_slots).  exp_step[par]: the ring step packed in
     export_dev[par]. */
  std::vector<uint8_t *> ring;
  SlotRing ring_slots;
  long exp_step[2] = {};
  /* a late resolve re-packed sections of the pending step (export_repack): export_finish ships its header and fixed
     part again first */
  bool export_redo = false;
  hipEvent_t ev_exp_repack = nullptr;
  std::vector<hipEvent_t> timed[kStages];    /* pairs */
  std::vector<void *> owned;
  std::vector<hipEvent_t> owned_events;      /* pipe_event: the events that live as long as the pipe */
  /* odhip_pipe_set_quants: the band steps of every plane, [set][level][plane][ODHIP_MAX_BANDS], plane set si at
     qp_off[si][bs].  qp_next is what the next step codes with (empty: the config's quant, the jobs' q_band);
     a step copies it into the pinned qp_host[parity] and from there into qp_dev[parity] on the stream of each
     plane set (ev_qp[parity][set]: that copy has completed, the pinned rows may be rewritten) */
  int use_masking = 0, hvs_qm = 0;           /* of the config's quant: per pipe */
  std::vector<int32_t> qp_next;
  size_t qp_off[2][ODHIP_NBSIZES] = {};
  size_t qp_set[2][2] = {};       /* [set]: first word, words */
  PinnedBuf<int32_t> qp_host[2];
  int32_t *qp_dev[2] = {};
  hipEvent_t ev_qp[2][2] = {};
  bool qp_sent[2][2] = {};        /* ev_qp recorded */
  /* odhip_pipe_set_metrics: step s (numbered from that call, met_slots: a taken step's slot is released at once) is
     measured into device slot s % met_n - the columns of kMetricColumns that met_flags asks for, in that order (the
     table of include/daala_hip.h), column c at met_off[c]: met_cols columns of met_values 8-byte entries - and copied
     into the pinned slot s % met_n once complete (metrics_finish); met_step[par]: the metrics step of the pipe step at
     that parity, -1 unmeasured; met_ev_luma[par]: its luma values are written */
  int met_flags = 0;
  int met_depth = 0;
  int met_n = 0;
  int met_cols = 2;
  size_t met_off[MET_NCOLS] = {};         /* in columns; of a column the slot has */
  size_t met_values = 0;
  DeviceBuf<uint8_t> met_dev;
  PinnedBuf<uint8_t> met_host;
  SlotRing met_slots;
  hipEvent_t met_ev_luma[2] = {};
  /* ODHIP_METRIC_CIEDE reads both plane sets of a step in front of the slot's copy (measure_ciede): ev_ciede follows
     that measurement, and the luma chain of the next step, which overwrites the luma source plane and the
     single-buffered luma reconstructions, starts behind it */
  hipEvent_t ev_ciede = nullptr;
  long met_step[2] = {-1, -1};
  int met_pending = -1;           /* parity of the measured step whose slot is not complete yet, -1 */
  /* odhip_pipe_set_reference_frames / _set_mvs / _feed_*: inter steps build their prediction from reference frames
     (coded size, the planes' sample type) and motion-vector grids, each chain its own plane set into pred_px.  Frames
     and grids are double-buffered like the pictures: a step reads [mc_ffront] / [mc_gfront], a feed writes the other
     one on the copy stream behind ev_mc (the prediction kernels of the last enqueued step of each chain) and the
     next step takes it.  mc_nslots == 0 / !mc_grid_set: nothing allocated, nothing launched. */
  int mc_nslots = 0;
  bool mc_grid_set = false;
  uint8_t *mc_ref[2][2][3] = {};  /* [buffer][set][slot] */
  odhip_mv_point *mc_grid[2] = {};
  int mc_ffront = 0, mc_gfront = 0;
  bool mc_ffed = false, mc_gfed = false;
  hipEvent_t ev_mc[2] = {};
  hipEvent_t ev_mc_fed = nullptr;
  /* odhip_pipe_set_motion_search: every inter step searches its grids itself (me_kernels.hip), on the luma stream in
     front of the luma prediction, into the grid buffer no enqueued prediction reads; the buffers flip with the step
     and the chroma chain waits for ev_me.  me_on false: nothing allocated, nothing launched. */
  bool me_on = false;
  int me_log_size = 0, me_range = 0, me_res = 0, me_lambda = 0, me_lambda_subpel = 0, me_flags = 0;
  int me_levels = 0, me_refine = 1;  /* odhip_pipe_set_motion_search3: pyramids and centres live in me_scratch */
  /* odhip_pipe_set_motion_search_vbs: sizes me_log_min .. me_log_size; the per-size grids, predictions and cell
     distortions live in me_scratch too.  me_log_min == me_log_size: the uniform search */
  int me_log_min = 0, me_split_penalty = 0;
  void *me_scratch = nullptr;
  size_t me_scratch_bytes = 0;
  uint32_t *me_cost[2] = {};
  hipEvent_t ev_me = nullptr;
};

namespace {

int alloc(odhip_pipe *p, void **out, size_t bytes, bool zero) {
  void *d = nullptr;
  ODHIP_TRY(hipMalloc(&d, bytes ? bytes : 16));
  p->owned.push_back(d);
  if (zero) ODHIP_TRY(hipMemset(d, 0, bytes ? bytes : 16));
  *out = d;
  return ODHIP_SUCCESS;
}

/* An event that lives as long as the pipe (odhip_pipe_destroy frees it); nothing to do when it exists already. */
int pipe_event(odhip_pipe *p, hipEvent_t *e) {
  if (*e) return ODHIP_SUCCESS;
  ODHIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  p->owned_events.push_back(*e);
  return ODHIP_SUCCESS;
}

/* Bytes of the resident pictures of plane set si, which keep their own depth, and of one set of its coded planes - the
   padded planes, the reconstructions, the reference frames: int16 samples with full-precision references. */
size_t picture_bytes(const odhip_pipe *p, int si) {
  const PlaneSet &t = p->set[si];
  return (size_t)t.nplanes*t.pw*t.ph*(p->cfg.fpr_bits > 8 ? 2 : 1);
}

size_t plane_bytes(const odhip_pipe *p, int si) {
  const PlaneSet &t = p->set[si];
  return (size_t)t.nplanes*t.w*t.h*(p->cfg.fpr_bits ? 2 : 1);
}

#define STEP_TRY(expr) \
  do { \
    const int rc_ = (expr); \
    if (rc_) return rc_; \
  } while (0)

#define PIPE_ALLOC(p, ptr, bytes, zero) \
  do { \
    const int rc_ = alloc((p), (void **)&(ptr), (bytes), (zero)); \
    if (rc_) return rc_; \
  } while (0)

struct Timed {
  odhip_pipe *p;
  int stage;
  hipStream_t s;
  bool on;
  Timed(odhip_pipe *p_, int stage_, hipStream_t s_) : p(p_), stage(stage_), s(s_) {
    on = p->record && p->timed[stage].size() < (size_t)2*kMaxTimed;
    if (on) mark();
  }
  ~Timed() {
    if (on) mark();
  }
  void mark() {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) {
      on = false;
      return;
    }
    (void)hipEventRecord(e, s);
    p->timed[stage].push_back(e);
  }
};

int setup_set(odhip_pipe *p, int si, int dec, int pli, int nplanes) {
  const odhip_quant *qt = p->cfg.quant;
  PlaneSet &s = p->set[si];
  s.dec = dec;
  s.pli = pli;
  s.nplanes = nplanes;
  s.w = p->W >> dec;
  s.h = p->H >> dec;
  s.pw = (p->pic_w + dec) >> dec;
  s.ph = (p->pic_h + dec) >> dec;
  s.nlev = ODHIP_NBSIZES - dec;
  s.plane_split = pli == 1 ? nplanes/2 : 0;
  PIPE_ALLOC(p, s.pic_buf[0], picture_bytes(p, si), true);
  PIPE_ALLOC(p, s.pic_buf[1], picture_bytes(p, si), true);
  s.pic = s.pic_buf[0];
  PIPE_ALLOC(p, s.px, plane_bytes(p, si), true);
  s.pred_pic = s.pred_px = nullptr;
  if (p->cfg.inter) {
    PIPE_ALLOC(p, s.pred_pic, picture_bytes(p, si), true);
    PIPE_ALLOC(p, s.pred_px, plane_bytes(p, si), true);
  }
  for (int bs = 0; bs < s.nlev; bs++) {
    const int n = 4 << bs;
    const int len = n*n < OD_SCAN_LEN ? n*n : OD_SCAN_LEN;
    PIPE_ALLOC(p, s.levels[bs], sizeof(od_coeff)*(size_t)nplanes*s.w*s.h, true);
    s.pred_levels[bs] = nullptr;
    if (p->cfg.inter) PIPE_ALLOC(p, s.pred_levels[bs], sizeof(od_coeff)*(size_t)nplanes*s.w*s.h, true);
    PIPE_ALLOC(p, s.recon[bs], plane_bytes(p, si), true);
    PIPE_ALLOC(p, s.qm[bs], sizeof(int16_t)*len, false);
    PIPE_ALLOC(p, s.qm_inv[bs], sizeof(int16_t)*len, false);
    const int off = odhip_qm_offset(bs, dec);
    ODHIP_TRY(hipMemcpy(s.qm[bs], qt->qm + off, sizeof(int16_t)*len, hipMemcpyHostToDevice));
    ODHIP_TRY(hipMemcpy(s.qm_inv[bs], qt->qm_inv + off, sizeof(int16_t)*len, hipMemcpyHostToDevice));
    if (odhip_quant_bands(qt, pli, bs, s.q[bs], s.beta[bs]) < 0) return ODHIP_EINVAL;
    if (pli == 1 && odhip_quant_bands(qt, 2, bs, s.q2[bs], nullptr) < 0) return ODHIP_EINVAL;
    s.nblocks[bs] = (long)nplanes*(s.w/n)*(s.h/n);
  }
  return ODHIP_SUCCESS;
}

int setup_job(odhip_pipe *p, odhip_pvq_job &j, PlaneSet &s, int bs, const odhip_pvq_job *share = nullptr) {
  int nb = 0;
  int len = 0;
  odhip_pvq_band_layout(bs, &nb, nullptr, &len);
  memset(&j, 0, sizeof(j));
  j.d_coef = s.levels[bs];
  j.nplanes = s.nplanes;
  j.w = s.w;
  j.h = s.h;
  j.bs = bs;
  j.d_qm = s.qm[bs];
  j.d_qm_inv = s.qm_inv[bs];
  j.q_band = s.q[bs];
  j.beta_band = s.beta[bs];
  if (s.plane_split) {
    j.q_band2 = s.q2[bs];
    j.plane_split = s.plane_split;
  }
  const long B = s.nblocks[bs];
  /* The two parities of the luma job set share ONE band-record buffer while the chroma chain of
     step i runs beside the luma chain of step i + 1.  That is race-free only because (a) the
     records are written by close-call bands alone and luma_choose resolves them on the host
     BEFORE the next step is enqueued, (b) lref_piece and the inverse read the choice and pulse
     buffers (which ARE per parity), never the records, (c) the unpriced choice kernel runs on the
     luma stream itself.  A new consumer of luma band records on the side stream (e.g. a deferred
     resolve, or a host dump through odhip_pipe_buffer(BUF_BAND) while a step is in flight) must
     give parity 1 its own buffer here. */
  if (share) j.cands.band = share->cands.band;       /* the other parity's set: own pulses and choices */
  else PIPE_ALLOC(p, j.cands.band, sizeof(odhip_pvq_band)*(size_t)B*nb, true);
  PIPE_ALLOC(p, j.cands.y, sizeof(int16_t)*(size_t)2*B*len, true);
  PIPE_ALLOC(p, j.cands.choice, sizeof(int32_t)*(size_t)B*nb*4, true);
  return ODHIP_SUCCESS;
}

int setup_refjob(odhip_pipe *p, odhip_pvq_refjob &j, PlaneSet &s, int bs, const od_coeff *ref,
 const odhip_pvq_refjob *share, const odhip_pvq_job *luma = nullptr) {
  int nb = 0;
  int len = 0;
  odhip_pvq_band_layout(bs, &nb, nullptr, &len);
  memset(&j, 0, sizeof(j));
  j.d_coef = s.levels[bs];
  j.d_ref = ref;
  j.luma = luma;
  j.nplanes = s.nplanes;
  j.w = s.w;
  j.h = s.h;
  j.bs = bs;
  j.is_keyframe = 1;
  j.pli = s.pli;
  j.d_qm = s.qm[bs];
  j.d_qm_inv = s.qm_inv[bs];
  j.q_band = s.q[bs];
  j.beta_band = s.beta[bs];
  if (s.plane_split) {
    j.q_band2 = s.q2[bs];
    j.plane_split = s.plane_split;
  }
  if (share) {
    /* same planes, the other reference buffer: outputs and work vectors are shared
       (the chroma chains of consecutive steps run in order on one stream) */
    j.band = share->band;
    j.items = share->items;
    j.y = share->y;
    j.r16 = share->r16;
    j.x16 = share->x16;
    j.xr = share->xr;
    j.choice = share->choice;
    return ODHIP_SUCCESS;
  }
  const long B = s.nblocks[bs];
  PIPE_ALLOC(p, j.band, sizeof(odhip_pvq_refband)*(size_t)B*nb, true);
  PIPE_ALLOC(p, j.items, (size_t)3*nb*ODHIP_PVQ_REF_SLOTS*B*16, true);
  PIPE_ALLOC(p, j.y, sizeof(int16_t)*(size_t)ODHIP_PVQ_REF_SLOTS*B*len, true);
  PIPE_ALLOC(p, j.r16, sizeof(int16_t)*(size_t)B*len, true);
  PIPE_ALLOC(p, j.x16, sizeof(int16_t)*(size_t)B*len, true);
  PIPE_ALLOC(p, j.xr, sizeof(int16_t)*(size_t)B*len, true);
  PIPE_ALLOC(p, j.choice, sizeof(int32_t)*(size_t)B*nb*16, true);
  return ODHIP_SUCCESS;
}

/* inter mode: every plane through the with-reference stage against its own prediction pyramid */
int setup_inter_jobs(odhip_pipe *p) {
  for (int si = 0; si < 2; si++) {
    for (int bs = 0; bs < p->set[si].nlev; bs++) {
      STEP_TRY(setup_refjob(p, p->interjobs[si][bs], p->set[si], bs, p->set[si].pred_levels[bs], nullptr));
      p->interjobs[si][bs].is_keyframe = 0;
    }
  }
  p->njobs = 0;
  return ODHIP_SUCCESS;
}

/* keyframes: luma without reference; chroma beside it, or from luma with its reference jobs and events */
int setup_keyframe_jobs(odhip_pipe *p) {
  PlaneSet &ch = p->set[1];
  for (int bs = 0; bs < 5; bs++) STEP_TRY(setup_job(p, p->jobs[0][bs], p->set[0], bs));
  p->njobs = 5;
  if (!p->cfg.chroma_cfl) {
    for (int bs = 0; bs < ch.nlev; bs++) STEP_TRY(setup_job(p, p->jobs[0][5 + bs], ch, bs));
    p->njobs = 5 + ch.nlev;
    return ODHIP_SUCCESS;
  }
  for (int bs = 0; bs < 5; bs++) STEP_TRY(setup_job(p, p->jobs[1][bs], p->set[0], bs, &p->jobs[0][bs]));
  for (int par = 0; par < 2; par++) {
    for (int bs = 0; bs < ch.nlev; bs++) {
      /* the chroma-from-luma reference of chroma level bs: the choices of luma level
         bs + 1 (4:4:4: bs) of the same step, read in place (no reference planes) */
      STEP_TRY(setup_refjob(p, p->refjobs[par][bs], ch, bs, nullptr, par ? &p->refjobs[0][bs] : nullptr,
       &p->jobs[par][bs + ch.dec]));
    }
    STEP_TRY(pipe_event(p, &p->ev_refs[par]));
    STEP_TRY(pipe_event(p, &p->ev_used[par]));
  }
  return ODHIP_SUCCESS;
}

int pipe_init(odhip_pipe *p) {
  const odhip_pipe_config &c = p->cfg;
  ODHIP_TRY(hipSetDevice(c.device));
  p->pic_w = c.pic_w;
  p->pic_h = c.pic_h;
  p->W = (c.pic_w + 63) & ~63;     /* coded frame size, src/state.c:376-379 */
  p->H = (c.pic_h + 63) & ~63;
  p->serial = c.serial || odhip_env_serial();
  /* with two chains side by side (chroma from luma, inter) the band stages do not fork
     their searches onto side streams: more concurrency only interleaves the searches of
     one chain (measured: 5.72 -> 5.58 ms per step; ODHIP_PIPE_FORK=3 restores the forks).
     The single chain of the chroma-without-reference mode keeps them (3.56 vs 3.45 ms). */
  const bool two_chains = c.chroma_cfl || c.inter;
  /* ODHIP_PIPE_FORK: a bit mask - bit 0 = the luma chain forks, bit 1 = the chroma chain forks.
     Rounds 1-2 read the variable as a flag ("set = both chains fork"): a value that is not a
     number in 0..3 (e.g. "yes", "true") keeps that meaning; the parsed mask is logged once. */
  int forkmask = 0;
  if (const char *fe = ODHIP_EXP_ENV("ODHIP_PIPE_FORK")) {
    char *end = nullptr;
    const long v = strtol(fe, &end, 10);
    forkmask = (end == fe || *end != '\0' || v < 0 || v > 3) ? 3 : (int)v;
    static bool logged = false;
    if (!logged) {
      fprintf(stderr, "odhip_pipe: ODHIP_PIPE_FORK=%s -> fork mask %d (bit 0 luma chain, bit 1 chroma chain)\n",
       fe, forkmask);
      logged = true;
    }
  }
  for (int i = 0; i < 2; i++) {
    p->ctx[i] = odhip_create(c.device);
    if (!p->ctx[i]) return ODHIP_EFAULT;
    odhip_ctx_set_serial(p->ctx[i], p->serial || (two_chains && !(forkmask >> i & 1)));
    odhip_ctx_set_fpr(p->ctx[i], c.fpr_bits != 0);
  }
  /* Experiment knob: ODHIP_PIPE_CUSPLIT=n (1..7) gives the luma chain n of every 8 compute
     units and the chroma chain the other 8 - n (hipExtStreamCreateWithCUMask) instead of
     letting the two chains share every CU. */
  const char *split_env = ODHIP_EXP_ENV("ODHIP_PIPE_CUSPLIT");
  const int split = split_env ? atoi(split_env) : 0;
  if (!p->serial && split >= 1 && split <= 7) {
    hipDeviceProp_t prop;
    ODHIP_TRY(hipGetDeviceProperties(&prop, c.device));
    const int words = (prop.multiProcessorCount + 31)/32;
    std::vector<uint32_t> ma(words), mb(words);
    const uint32_t byte_a = (1u << split) - 1u;
    for (int i = 0; i < words; i++) {
      ma[i] = byte_a*0x01010101u;
      mb[i] = ~ma[i];
    }
    ODHIP_TRY(hipExtStreamCreateWithCUMask(&p->stream[0], (uint32_t)words, ma.data()));
    ODHIP_TRY(hipExtStreamCreateWithCUMask(&p->stream[1], (uint32_t)words, mb.data()));
  }
  else if (const char *prio_env = p->serial ? nullptr : ODHIP_EXP_ENV("ODHIP_PIPE_PRIO")) {
    /* Experiment knob: ODHIP_PIPE_PRIO=1 gives the luma chain the highest queue priority the device
       offers and the chroma chain the lowest, 2 the other way round. */
    int lo = 0;
    int hi = 0;
    ODHIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    const bool luma_high = atoi(prio_env) == 1;
    ODHIP_TRY(hipStreamCreateWithPriority(&p->stream[0], hipStreamNonBlocking, luma_high ? hi : lo));
    ODHIP_TRY(hipStreamCreateWithPriority(&p->stream[1], hipStreamNonBlocking, luma_high ? lo : hi));
  }
  else {
    ODHIP_TRY(hipStreamCreateWithFlags(&p->stream[0], hipStreamNonBlocking));
    if (p->serial) p->stream[1] = p->stream[0];
    else ODHIP_TRY(hipStreamCreateWithFlags(&p->stream[1], hipStreamNonBlocking));
  }
  STEP_TRY(setup_set(p, 0, 0, 0, c.frames));
  p->cdec = c.chroma_444 ? 0 : 1;
  STEP_TRY(setup_set(p, 1, p->cdec, 1, 2*c.frames));
  STEP_TRY(c.inter ? setup_inter_jobs(p) : setup_keyframe_jobs(p));
  ODHIP_TRY(hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
  STEP_TRY(pipe_event(p, &p->ev_fed));
  STEP_TRY(pipe_event(p, &p->ev_pad[0]));
  STEP_TRY(pipe_event(p, &p->ev_pad[1]));
  ODHIP_TRY(hipDeviceSynchronize());
  return ODHIP_SUCCESS;
}

/* The with-reference jobs of plane set si at step parity par: inter steps code every plane set against its prediction
   (one set of jobs per plane set), keyframes code chroma against luma (one set per parity). */
odhip_pvq_refjob *ref_jobs(odhip_pipe *p, int si, int par) {
  return p->cfg.inter ? p->interjobs[si] : p->refjobs[par];
}

/* The job of level bs of plane set si at step parity par in this pipe's mode: exactly one of the two is set.  Keyframe
   luma alternates between two job sets only with chroma from luma; chroma without reference follows luma in set 0. */
struct JobAt {
  odhip_pvq_job *noref;
  odhip_pvq_refjob *ref;
};

JobAt job_at(odhip_pipe *p, int si, int bs, int par) {
  if (p->cfg.inter || (si == 1 && p->cfg.chroma_cfl)) return {nullptr, ref_jobs(p, si, par) + bs};
  if (si == 0) return {&p->jobs[p->cfg.chroma_cfl ? par : 0][bs], nullptr};
  return {&p->jobs[0][5 + bs], nullptr};
}

/* The per-plane band steps of this step (parity par) for the jobs of plane set si: the jobs point at
   qp_dev[par], or at nothing (the config's quant) while no odhip_pipe_set_quants table is in force. */
void quants_point(odhip_pipe *p, int si, int par) {
  const int32_t *d = p->qp_next.empty() ? nullptr : p->qp_dev[par];
  const PlaneSet &t = p->set[si];
  for (int bs = 0; bs < t.nlev; bs++) {
    const int32_t *row = d ? d + p->qp_off[si][bs] : nullptr;
    const JobAt j = job_at(p, si, bs, par);
    if (j.ref) j.ref->d_q_plane = row;
    else j.noref->d_q_plane = row;
  }
}

/* ... and their upload, in order on the stream s that runs every kernel of this step reading them: behind
   the step two before, which read the same parity's table on s. */
int quants_upload(odhip_pipe *p, int si, int par, hipStream_t s) {
  if (p->qp_next.empty()) return ODHIP_SUCCESS;
  const size_t first = p->qp_set[si][0];
  const size_t bytes = sizeof(int32_t)*p->qp_set[si][1];
  if (p->qp_sent[par][si]) ODHIP_TRY(hipEventSynchronize(p->ev_qp[par][si]));
  memcpy(p->qp_host[par].p + first, p->qp_next.data() + first, bytes);
  ODHIP_TRY(hipMemcpyAsync(p->qp_dev[par] + first, p->qp_host[par].p + first, bytes, hipMemcpyHostToDevice, s));
  ODHIP_TRY(hipEventRecord(p->ev_qp[par][si], s));
  p->qp_sent[par][si] = true;
  return ODHIP_SUCCESS;
}

int stage_pad_run(odhip_pipe *p, int si, hipStream_t s);
int export_luma(odhip_pipe *p, int par);
int export_chroma(odhip_pipe *p, int par);
int export_finish(odhip_pipe *p);
int export_repack(odhip_pipe *p, int si, int par, hipStream_t s);

/* a host buffer (odhip_pipe_set_export) or a ring of them (odhip_pipe_set_export_ring) receives the steps */
bool exporting(const odhip_pipe *p) {
  return p->export_host != nullptr || !p->ring.empty();
}

/* ---- odhip_pipe_set_metrics ---- */
size_t metrics_bytes(const odhip_pipe *p) {
  return sizeof(int64_t)*p->met_cols*p->met_values;
}
static_assert(sizeof(int64_t) == sizeof(double), "metrics slot: columns of 8-byte values");

/* the plane values of a step: luma [5][F], then chroma [nlev][2F] */
size_t metrics_values(const odhip_pipe *p) {
  return (size_t)5*p->set[0].nplanes + (size_t)p->set[1].nlev*p->set[1].nplanes;
}

/* the bits of the columns up to and including `last`: what the entry point that introduced that column accepts */
int metrics_mask(int last) {
  int mask = 0;
  for (int c = 0; c <= last; c++) mask |= kMetricColumns[c].bit;
  return mask;
}

/* column c, which the slot has, of slot `slot` of the device ring or the pinned one */
template <typename T = double>
T *metrics_col(const odhip_pipe *p, uint8_t *ring, size_t slot, int c) {
  return reinterpret_cast<T *>(ring + slot*metrics_bytes(p) + p->met_off[c]*sizeof(int64_t)*p->met_values);
}

bool ciede_on(const odhip_pipe *p) {
  return (p->met_flags & ODHIP_METRIC_CIEDE) != 0;
}

/* plane `plane` of plane set si: the padded source and the reconstruction of `level`, their format and stride */
struct MetricPlane {
  const uint8_t *src, *rec;
  int fmt, stride;
};
MetricPlane metric_plane(const odhip_pipe *p, int si, int level, int plane) {
  const PlaneSet &t = p->set[si];
  const bool fpr = p->cfg.fpr_bits != 0;
  const size_t off = (size_t)plane*t.w*t.h*(fpr ? 2 : 1);
  return {t.px + off, t.recon[level] + off, fpr ? ODHIP_SAMPLE_I16_12 : ODHIP_SAMPLE_U8, t.w};
}

/* ODHIP_METRIC_CIEDE: every picture of the step whose metrics step is st at every luma level, against the padded source
   planes of both chains, on s, the chroma chain's stream: luma level l with chroma level max(l - 1, 0) at 4:2:0, l at
   4:4:4.  The five levels of a picture share its source: one call, so that its Lab is computed once per tile.  The
   caller has ordered s behind the luma chain's last reconstruction (met_ev_luma). */
int measure_ciede(odhip_pipe *p, long st, hipStream_t s) {
  const int F = p->cfg.frames;
  std::vector<odhip_ciede_pair> pairs((size_t)5*F);
  for (int l = 0; l < 5; l++) {
    const int cl = p->cdec ? std::max(l - 1, 0) : l;
    for (int f = 0; f < F; f++) {
      odhip_ciede_pair &q = pairs[(size_t)l*F + f];
      const MetricPlane m[3] = {metric_plane(p, 0, l, f), metric_plane(p, 1, cl, f), metric_plane(p, 1, cl, F + f)};
      for (int k = 0; k < 3; k++) {
        q.src[k] = m[k].src;
        q.rec[k] = m[k].rec;
      }
      q.src_fmt = q.rec_fmt = m[0].fmt;
      q.src_stride = q.rec_stride = m[0].stride;
      q.src_cstride = q.rec_cstride = m[1].stride;
      q.w = p->set[0].pw;
      q.h = p->set[0].ph;
      q.depth = p->met_depth;
      q.cdec = p->cdec;
    }
  }
  double *de = metrics_col(p, p->met_dev.p, (size_t)(st % p->met_n), MET_CIEDE);
  /* the scratch of the chain whose stream this is */
  Current cur(p->ctx[s == p->stream[1] ? 1 : 0]);
  return odhip_ciede_pictures(pairs.data(), (int)pairs.size(), de, s);
}

/* Every level and plane of plane set si of the step at parity par against its source, on the chain's stream s behind
   the inverse that wrote the reconstructions (a re-run of the inverse measures again).  The padded plane px holds the
   picture region of the source until the next step's padding on the same stream. */
int measure(odhip_pipe *p, int si, int par, hipStream_t s) {
  if (!p->met_flags || p->met_step[par] < 0) return ODHIP_SUCCESS;
  const PlaneSet &t = p->set[si];
  const int F = p->cfg.frames;
  std::vector<odhip_metrics_pair> pairs((size_t)t.nlev*t.nplanes);
  for (int bs = 0; bs < t.nlev; bs++) {
    for (int pl = 0; pl < t.nplanes; pl++) {
      odhip_metrics_pair &q = pairs[(size_t)bs*t.nplanes + pl];
      const MetricPlane m = metric_plane(p, si, bs, pl);
      q.src = m.src;
      q.rec = m.rec;
      q.src_fmt = q.rec_fmt = m.fmt;
      q.src_stride = q.rec_stride = m.stride;
      q.w = t.pw;
      q.h = t.ph;
      q.depth = p->met_depth;
      q.csf = si == 0 ? ODHIP_CSF_Y : pl < F ? ODHIP_CSF_CB : ODHIP_CSF_CR;
    }
  }
  const int n = (int)pairs.size();
  const size_t slot = (size_t)(p->met_step[par] % p->met_n);
  /* this plane set's values of column c: luma first, chroma behind its 5F */
  const size_t first = si == 0 ? 0 : (size_t)5*F;
  auto col = [&](int c) { return metrics_col(p, p->met_dev.p, slot, c) + first*kMetricColumns[c].width; };
  const int flags = p->met_flags & (ODHIP_METRIC_SSE | ODHIP_METRIC_PSNRHVS);
  if (flags) {
    int64_t *sse = metrics_col<int64_t>(p, p->met_dev.p, slot, MET_SSE) + first;
    STEP_TRY(odhip_metrics_planes(pairs.data(), n, flags, sse, col(MET_HVS), nullptr, nullptr, s));
  }
  if (p->met_flags & ODHIP_METRIC_SSIM) STEP_TRY(odhip_ssim_planes(pairs.data(), n, 1., col(MET_SSIM), nullptr, s));
  /* MS-SSIM, FastSSIM: the levels of a plane share its source: one call, so that its pyramid is built once */
  if (p->met_flags & ODHIP_METRIC_MSSSIM) STEP_TRY(odhip_msssim_planes(pairs.data(), n, col(MET_MSSSIM), nullptr, s));
  if (p->met_flags & ODHIP_METRIC_FASTSSIM) STEP_TRY(odhip_fastssim_planes(pairs.data(), n, col(MET_FASTSSIM), s));
  if (si == 0) ODHIP_TRY(hipEventRecord(p->met_ev_luma[par], s));
  return ODHIP_SUCCESS;
}

/* The measured step at parity met_pending is final (its late resolve, if any, is enqueued): its values leave for the
   pinned slot on s, the stream of its chroma measurements, behind its luma ones. */
int metrics_finish(odhip_pipe *p, hipStream_t s) {
  if (p->met_pending < 0) return ODHIP_SUCCESS;
  const int par = p->met_pending;
  p->met_pending = -1;
  const long st = p->met_step[par];
  if (!p->met_flags || st < 0) return ODHIP_SUCCESS;
  const size_t slot = (size_t)(st % p->met_n);
  const size_t n = metrics_bytes(p);
  ODHIP_TRY(hipStreamWaitEvent(s, p->met_ev_luma[par], 0));
  if (ciede_on(p)) {
    /* every late resolve of the step is enqueued, on this stream or in front of met_ev_luma */
    STEP_TRY(measure_ciede(p, st, s));
    ODHIP_TRY(hipEventRecord(p->ev_ciede, s));
  }
  ODHIP_TRY(hipMemcpyAsync(p->met_host.p + slot*n, p->met_dev.p + slot*n, n, hipMemcpyDeviceToHost, s));
  ODHIP_TRY(hipEventRecord(p->met_slots.ev[slot], s));
  p->met_slots.sent = st + 1;
  return ODHIP_SUCCESS;
}

/* the end of a step's enqueue: its slot completes in metrics_finish, now or behind its late resolve */
void metrics_step_done(odhip_pipe *p, int par) {
  if (p->met_flags && p->met_step[par] >= 0) p->met_pending = par;
}

/* Padding is the only reader of the resident pictures unless the motion search is on: its completion frees them
   for the next feed.  With the search on that search reads the luma pictures too, behind the padding on the luma
   stream; a feed then also waits for ev_me, recorded behind it (odhip_pipe_feed). */
int stage_pad(odhip_pipe *p, int si, hipStream_t s) {
  const int rc = stage_pad_run(p, si, s);
  if (rc) return rc;
  ODHIP_TRY(hipEventRecord(p->ev_pad[si], s));
  return ODHIP_SUCCESS;
}

/* Pictures of plane set si (src: the sources or the prediction pictures, at the pictures' depth) into its coded
   planes dst, extended into the padding. */
int pad_planes(odhip_pipe *p, int si, uint8_t *dst, const uint8_t *src, hipStream_t s) {
  const PlaneSet &t = p->set[si];
  if (p->cfg.fpr_bits) {
    return odhip_image_planes_copy_pad16(reinterpret_cast<uint16_t *>(dst), t.w, (long)t.w*t.h, t.w, t.h, src,
     p->cfg.fpr_bits, t.pw, (long)t.pw*t.ph, t.pw, t.ph, t.nplanes, s);
  }
  return odhip_image_planes_copy_pad(dst, t.w, (long)t.w*t.h, t.w, t.h, src, t.pw, (long)t.pw*t.ph,
   t.pw, t.ph, t.nplanes, s);
}

/* ... and the coefficients of every level of those planes. */
int pyramid(odhip_pipe *p, int si, od_coeff *const *dst, const uint8_t *src, hipStream_t s) {
  const PlaneSet &t = p->set[si];
  return odhip_forward_pyramid(dst, src, t.w, (long)t.w*t.h, t.nplanes, t.w, t.h, t.dec, p->pic_w, p->pic_h, s);
}

int stage_pad_run(odhip_pipe *p, int si, hipStream_t s) {
  Timed tm(p, si ? ODHIP_PIPE_PAD_CHROMA : ODHIP_PIPE_PAD_LUMA, s);
  return pad_planes(p, si, p->set[si].px, p->set[si].pic, s);
}

int stage_pyramid(odhip_pipe *p, int si, hipStream_t s) {
  Timed tm(p, si ? ODHIP_PIPE_PYRAMID_CHROMA : ODHIP_PIPE_PYRAMID_LUMA, s);
  return pyramid(p, si, p->set[si].levels, p->set[si].px, s);
}

int stage_inverse_noref(odhip_pipe *p, int si, hipStream_t s, int jpar) {
  PlaneSet &t = p->set[si];
  Timed tm(p, si ? ODHIP_PIPE_INVERSE_CHROMA : ODHIP_PIPE_INVERSE_LUMA, s);
  return odhip_inverse_levels_pvq(t.recon, t.w, (long)t.w*t.h, p->jobs[jpar] + (si ? 5 : 0), t.nlev, t.dec,
   p->pic_w, p->pic_h, s);
}

/* ---- the with-reference chain of plane set si at step parity par (ref_jobs), on the stream s of its context:
   keyframe chroma against luma, and both plane sets of an inter step against the pyramid of their prediction
   (pvq_theta with is_keyframe = 0, src/encode.c:1326-1360). */
int ref_bands(odhip_pipe *p, int si, int par, hipStream_t s) {
  const double lam = p->cfg.pvq_norm_lambda;
  const int nlev = p->set[si].nlev;
  Timed tm(p, si ? ODHIP_PIPE_BANDS_CHROMA : ODHIP_PIPE_BANDS_LUMA, s);
  /* (the decided stage sends its two counts itself) */
  if (p->cfg.price) return odhip_pvq_ref_bands_decided_multi(ref_jobs(p, si, par), nlev, lam, s);
  STEP_TRY(odhip_pvq_ref_bands_multi(ref_jobs(p, si, par), nlev, lam, s));
  return odhip_pvq_ref_resolve_begin(s);
}

int ref_choose(odhip_pipe *p, int si, int par, hipStream_t s) {
  Timed tm(p, si ? ODHIP_PIPE_CHOOSE_CHROMA : ODHIP_PIPE_CHOOSE_LUMA, s);
  return odhip_pvq_ref_choose_multi(ref_jobs(p, si, par), p->set[si].nlev, p->cfg.pvq_norm_lambda, s);
}

int ref_inverse(odhip_pipe *p, int si, int par, hipStream_t s) {
  const PlaneSet &t = p->set[si];
  Timed tm(p, si ? ODHIP_PIPE_INVERSE_CHROMA : ODHIP_PIPE_INVERSE_LUMA, s);
  return odhip_inverse_levels_pvq_ref(t.recon, t.w, (long)t.w*t.h, ref_jobs(p, si, par), t.nlev, t.dec, p->pic_w,
   p->pic_h, s);
}

/* Choice (only when the host prices or nobody does: with cfg.price the band stage decided
   every band itself, odhip_pvq_ref_bands_decided_multi), the inverse and its measurement. */
int ref_tail(odhip_pipe *p, int si, int par, hipStream_t s) {
  if (!p->cfg.price) STEP_TRY(ref_choose(p, si, par, s));
  STEP_TRY(ref_inverse(p, si, par, s));
  return measure(p, si, par, s);
}

/* The count of bands inside the device-acos margin of a with-reference stage (and, with cfg.price, inside the price
   margin: those are decided again with the host libm, as is a band re-run with the host's theta) is checked one step
   late, so the host never waits inside a step; a listed band the host corrects (never seen outside the forced tests)
   repeats what consumed it - the buffers are intact until the next chain of that plane set is enqueued.  A resolve
   rewrites choices and pulses of that step behind the pack kernels that read them, which run on the same stream.
   *changed: the step was re-decided. */
int ref_resolve(odhip_pipe *p, int si, int par, hipStream_t s, bool *changed) {
  odhip_pvq_refjob *jobs = ref_jobs(p, si, par);
  const int nlev = p->set[si].nlev;
  const double lam = p->cfg.pvq_norm_lambda;
  const auto t0 = std::chrono::steady_clock::now();
  const int n = odhip_pvq_ref_resolve_finish(jobs, nlev, lam, s);
  const int m = n >= 0 && p->cfg.price ? odhip_pvq_ref_choose_priced_resolve(jobs, nlev, lam, s) : 0;
  p->wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (n < 0) return n;
  if (m < 0) return m;
  p->reruns += n;
  p->price_reruns += m;
  *changed = n > 0 || m > 0;
  if (*changed) STEP_TRY(ref_tail(p, si, par, s));
  return ODHIP_SUCCESS;
}

/* The late resolve of the chroma chain of the previous keyframe step. */
int finish_pending(odhip_pipe *p) {
  if (p->pending < 0) return ODHIP_SUCCESS;
  const int par = p->pending;
  p->pending = -1;
  Current cur(p->ctx[1]);
  bool changed = false;
  STEP_TRY(ref_resolve(p, 1, par, p->stream[1], &changed));
  if (!changed) return ODHIP_SUCCESS;
  /* the resolves and the re-run read that step's luma pulses and choices (the chroma-from-luma
     references, in place): the luma chain of step + 2 reuses those buffers and waits for this */
  ODHIP_TRY(hipEventRecord(p->ev_used[par], p->stream[1]));
  if (!exporting(p)) return ODHIP_SUCCESS;
  if (!p->ring.empty()) {
    /* ring mode: the step's export has not been completed (export_finish follows the resolve; odhip_pipe_sync leaves
       a step with a pending resolve alone) - its chroma sections are packed again */
    if (p->export_pending == par) STEP_TRY(export_repack(p, 1, par, p->stream[1]));
  }
  else if (p->in_flush) {
    /* what left for the host is superseded.  Inside odhip_pipe_flush nothing newer has been packed: the step is
       exported again (step, flush, sync, read is exact) */
    p->export_pending = -1;        /* (the streams packed before the resolve are not sent) */
    ODHIP_TRY(hipStreamSynchronize(p->export_stream));
    ODHIP_TRY(hipStreamSynchronize(p->stream[0]));
    ODHIP_TRY(hipStreamSynchronize(p->stream[1]));
    ODHIP_TRY(hipMemset(p->export_dev[par], 0, sizeof(odhip_export_header)));
    STEP_TRY(export_luma(p, par));
    /* (the chroma packs, on the side stream, wait for the cleared header) */
    ODHIP_TRY(hipStreamWaitEvent(p->stream[1], p->ev_exp_luma[par], 0));
    STEP_TRY(export_chroma(p, par));
  }
  /* ... inside the NEXT step the host has already been told the buffer was complete - counted
     (odhip_pipe_export_stale) */
  else p->export_stale++;
  return ODHIP_SUCCESS;
}

/* ODHIP_METRIC_CIEDE: the luma chain on s is about to overwrite the luma source plane and reconstructions that the last
   step's measurement reads on the chroma chain's stream (an event never recorded holds nothing back) */
int ciede_hold(odhip_pipe *p, hipStream_t s) {
  if (ciede_on(p)) ODHIP_TRY(hipStreamWaitEvent(s, p->ev_ciede, 0));
  return ODHIP_SUCCESS;
}

int luma_bands(odhip_pipe *p, hipStream_t s, int jpar) {
  const double lam = p->cfg.pvq_norm_lambda;
  /* with pricing the searches make the choice themselves (no separate choice kernel) */
  Timed tm(p, ODHIP_PIPE_BANDS_LUMA, s);
  return p->cfg.price ? odhip_pvq_noref_bands_priced_multi(p->jobs[jpar], p->njobs, lam, s)
   : odhip_pvq_noref_bands_multi(p->jobs[jpar], p->njobs, lam, s);
}

int luma_front(odhip_pipe *p, hipStream_t s, int jpar) {
  STEP_TRY(ciede_hold(p, s));
  STEP_TRY(stage_pad(p, 0, s));
  STEP_TRY(stage_pyramid(p, 0, s));
  if (!p->cfg.chroma_cfl) {
    STEP_TRY(stage_pad(p, 1, s));
    STEP_TRY(stage_pyramid(p, 1, s));
  }
  else {
    /* the chroma chain of step i - 2 has read the choices this band stage overwrites */
    ODHIP_TRY(hipStreamWaitEvent(s, p->ev_used[jpar], 0));
  }
  const int par = (int)(p->nstep & 1);
  STEP_TRY(quants_upload(p, 0, par, s));
  if (!p->cfg.chroma_cfl) STEP_TRY(quants_upload(p, 1, par, s));
  return luma_bands(p, s, jpar);
}

int luma_choose(odhip_pipe *p, hipStream_t s, int jpar) {
  const double lam = p->cfg.pvq_norm_lambda;
  if (!p->cfg.price) {
    Timed tm(p, ODHIP_PIPE_CHOOSE_LUMA, s);
    return odhip_pvq_choose_multi(p->jobs[jpar], p->njobs, lam, s);
  }
  /* (the choice was made inside the band stage: odhip_pvq_noref_bands_priced_multi) */
  /* The luma choices feed this step's chroma references and inverse: a band whose priced
     decision is too close to take from the device is settled (host libm) before they are
     enqueued.  The host waits here for the luma front of this step while the chroma chain
     of the previous step keeps the GPU busy. */
  const auto t0 = std::chrono::steady_clock::now();
  const int n = odhip_pvq_choose_priced_resolve(p->jobs[jpar], p->njobs, lam, s);
  p->wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (n < 0) return n;
  p->price_reruns += n;
  return ODHIP_SUCCESS;
}

/* ---- inter mode: the two chains are independent, each in its own context on its own stream. */
/* the late resolve of the previous step's chain si */
int inter_finish(odhip_pipe *p, int si) {
  if (!p->inter_pending[si]) return ODHIP_SUCCESS;
  p->inter_pending[si] = false;
  hipStream_t s = p->stream[si];
  Current cur(p->ctx[si]);
  const int par = (int)((p->nstep - 1) & 1);
  bool changed = false;
  STEP_TRY(ref_resolve(p, si, par, s, &changed));
  if (changed && exporting(p)) {
    /* the previous step's sections of this plane set are packed again (its streams leave behind both resolves,
       export_finish in step_inter) - unless odhip_pipe_sync already sent them (the single buffer only) */
    if (p->export_pending == par) STEP_TRY(export_repack(p, si, par, s));
    else if (p->ring.empty()) p->export_stale++;
  }
  return ODHIP_SUCCESS;
}

/* the search job of the pipe's pictures and frames, but grid, cost and scratch */
void motion_job(const odhip_pipe *p, odhip_me_job4 *job4) {
  memset(job4, 0, sizeof(*job4));
  odhip_me_job3 *job3 = &job4->base;
  odhip_me_job2 &job2 = job3->base;
  odhip_me_job &job = job2.luma;
  job.coded_w = p->W;
  job.coded_h = p->H;
  job.pic_w = p->pic_w;
  job.pic_h = p->pic_h;
  job.npics = p->cfg.frames;
  job.nrefs = p->mc_nslots;
  job.log_size = p->me_log_size;
  job.range = p->me_range;
  job.res = p->me_res;
  job.lambda = p->me_lambda;
  job.src_stride = p->pic_w;
  job.ref_stride = p->W;
  job.src_plane_stride = (int64_t)p->pic_w*p->pic_h;
  job.ref_plane_stride = (int64_t)p->W*p->H;
  job.src = p->set[0].pic;
  for (int r = 0; r < p->mc_nslots; r++) job.ref[r] = p->mc_ref[p->mc_ffront][0][r];
  job2.flags = p->me_flags;
  job2.cdec = p->cdec;
  job2.lambda_subpel = p->me_lambda_subpel;
  if (p->me_flags & ODHIP_ME_CHROMA) {
    const PlaneSet &c = p->set[1];
    job2.csrc_stride = c.pw;
    job2.cref_stride = c.w;
    job2.csrc_plane_stride = (int64_t)c.pw*c.ph;
    job2.cref_plane_stride = (int64_t)c.w*c.h;
    job2.csrc = c.pic;
    for (int r = 0; r < p->mc_nslots; r++) job2.cref[r] = p->mc_ref[p->mc_ffront][1][r];
  }
  job3->levels = p->me_levels;
  job3->refine = p->me_refine;
  job4->log_min = p->me_log_min;
  job4->split_penalty = p->me_split_penalty;
}

/* This step's grids from its own pictures and reference frames, on the luma stream: written into the grid
   buffer that is not being read once the predictions of the last enqueued step have left the other one - as a feed
   does, without a sync; the buffers flip with the step.  It reads the step's luma pictures (set[0].pic) after the
   padding kernel has: ev_me, recorded behind it, is what a picture feed waits for besides ev_pad.
   With ODHIP_ME_CHROMA it also reads, still on the luma stream, the step's chroma pictures (set[1].pic) and chroma
   reference frames (mc_ref[mc_ffront][1]).  Both arrive on the copy stream, and the luma stream has waited for
   ev_fed / ev_mc_fed in odhip_pipe_step like the chroma stream.  What may overwrite them:
     a picture feed writes set[1].pic_buf[back] behind ev_me (odhip_pipe_feed), recorded here behind the search;
     a reference-frame feed writes mc_ref[back][1] behind ev_mc[0], which inter_chain records on this stream
     behind the luma prediction, so behind the search;
     the chroma chain only reads the pictures (its padding kernel) and the frames (its prediction).
   Without the flag the chroma half of the job stays zero and nothing of chroma is read.
   A coarse-to-fine search builds its pyramids itself, in front of its kernels on this stream, into scratch nothing
   else uses; so does a search at variable block sizes its per-size grids, predictions and cell distortions (its
   predictions go through this chain's context, like the step's own luma prediction behind it on this stream).  With
   one size odhip_me_search_vbs is odhip_me_search3. */
int motion_search(odhip_pipe *p, hipStream_t s) {
  ODHIP_TRY(hipStreamWaitEvent(s, p->ev_mc[0], 0));
  ODHIP_TRY(hipStreamWaitEvent(s, p->ev_mc[1], 0));
  p->mc_gfront ^= 1;
  odhip_me_job4 job4;
  motion_job(p, &job4);
  job4.base.base.luma.grid = p->mc_grid[p->mc_gfront];
  job4.base.base.luma.cost = p->me_cost[p->mc_gfront];
  job4.base.scratch = p->me_scratch;
  job4.base.scratch_bytes = p->me_scratch_bytes;
  STEP_TRY(odhip_me_search_vbs(&job4, s));
  ODHIP_TRY(hipEventRecord(p->ev_me, s));
  return ODHIP_SUCCESS;
}

int inter_chain(odhip_pipe *p, int si) {
  PlaneSet &t = p->set[si];
  hipStream_t s = p->stream[si];
  const int par = (int)(p->nstep & 1);
  Current cur(p->ctx[si]);
  if (si == 0) STEP_TRY(ciede_hold(p, s));
  STEP_TRY(stage_pad(p, si, s));
  STEP_TRY(stage_pyramid(p, si, s));
  if (p->mc_grid_set || p->me_on) {
    /* the prediction of the whole coded frame from this step's frames and grids, straight into the plane the
       prediction pyramid reads (the reference predicts the coded frame, src/encode.c:2370-2374: nothing is padded) */
    Timed tm(p, si ? ODHIP_PIPE_PAD_CHROMA : ODHIP_PIPE_PAD_LUMA, s);
    if (p->me_on) {
      /* luma searches this step's grids first; chroma waits for them */
      if (si) ODHIP_TRY(hipStreamWaitEvent(s, p->ev_me, 0));
      else STEP_TRY(motion_search(p, s));
    }
    odhip_mc_job job;
    memset(&job, 0, sizeof(job));
    job.coded_w = p->W;
    job.coded_h = p->H;
    job.dec = t.dec;
    job.sample = p->cfg.fpr_bits ? ODHIP_SAMPLE_I16_12 : ODHIP_SAMPLE_U8;
    job.npics = p->cfg.frames;
    job.nplanes = t.nplanes;
    job.nrefs = p->mc_nslots;
    job.grid_on_device = 1;
    job.ref_stride = job.dst_stride = t.w;
    job.ref_plane_stride = job.dst_plane_stride = (int64_t)t.w*t.h;
    for (int r = 0; r < p->mc_nslots; r++) job.ref[r] = p->mc_ref[p->mc_ffront][si][r];
    job.dst = t.pred_px;
    job.grid = p->mc_grid[p->mc_gfront];
    STEP_TRY(odhip_mc_predict_planes(&job, s));
    ODHIP_TRY(hipEventRecord(p->ev_mc[si], s));
  }
  else {
    /* the prediction pictures: same padding, same pyramid */
    Timed tm(p, si ? ODHIP_PIPE_PAD_CHROMA : ODHIP_PIPE_PAD_LUMA, s);
    STEP_TRY(pad_planes(p, si, t.pred_px, t.pred_pic, s));
  }
  {
    Timed tm(p, si ? ODHIP_PIPE_PYRAMID_CHROMA : ODHIP_PIPE_PYRAMID_LUMA, s);
    STEP_TRY(pyramid(p, si, t.pred_levels, t.pred_px, s));
  }
  STEP_TRY(ref_bands(p, si, par, s));
  if (exporting(p)) {
    /* the decisions of this plane set, behind its band stage on its own stream, into this parity's buffer once the
       step two before has left it (export_finish).  The interjobs are single-buffered: the pack reads them before
       inter_chain of the next step overwrites them because both run on this stream, in order.  Luma packs first (the
       loop in step_inter); the chroma chain then copies the header of both sets (export_chroma). */
    ODHIP_TRY(hipStreamWaitEvent(s, p->ev_exp_sent[par], 0));
    STEP_TRY(si ? export_chroma(p, par) : export_luma(p, par));
  }
  STEP_TRY(ref_tail(p, si, par, s));
  p->inter_pending[si] = true;
  return ODHIP_SUCCESS;
}

int step_inter(odhip_pipe *p) {
  const int par = (int)(p->nstep & 1);
  if (ciede_on(p)) {
    /* the last step is measured in front of this step's luma chain (ciede_hold): both its resolves first (the calls
       below then find nothing pending) */
    STEP_TRY(inter_finish(p, 0));
    STEP_TRY(inter_finish(p, 1));
    STEP_TRY(metrics_finish(p, p->stream[1]));
  }
  for (int si = 0; si < 2; si++) {
    STEP_TRY(inter_finish(p, si));
    /* both resolves of the previous step are enqueued: its streams follow, one step late as in step_cfl */
    if (si == 1 && exporting(p)) STEP_TRY(export_finish(p));
    if (si == 1) STEP_TRY(metrics_finish(p, p->stream[1]));
    /* (the resolve above re-ran the previous step with its own table) */
    quants_point(p, si, par);
    STEP_TRY(quants_upload(p, si, par, p->stream[si]));
    STEP_TRY(inter_chain(p, si));
  }
  metrics_step_done(p, par);
  return ODHIP_SUCCESS;
}

int step_noref(odhip_pipe *p) {
  hipStream_t s = p->stream[0];
  const int par = (int)(p->nstep & 1);
  Current cur(p->ctx[0]);
  quants_point(p, 0, par);
  quants_point(p, 1, par);
  STEP_TRY(luma_front(p, s, 0));
  STEP_TRY(luma_choose(p, s, 0));
  STEP_TRY(stage_inverse_noref(p, 0, s, 0));
  STEP_TRY(measure(p, 0, par, s));
  STEP_TRY(stage_inverse_noref(p, 1, s, 0));
  STEP_TRY(measure(p, 1, par, s));
  /* no late resolve: the step is final */
  metrics_step_done(p, par);
  return metrics_finish(p, s);
}

/* ---- the output side of the PCIe-inclusive rate (odhip_pipe_set_export) ------------------
   Sections of the export buffer (include/daala_hip.h, export_kernels.hip): luma levels 0..4, chroma
   levels 0..3 (4:4:4: 0..4).  The luma sections are packed as soon as the luma choices are final, the chroma ones
   behind the chroma band stage; then ONE ship kernel moves the header, the records and the used part
   of every stream to the host.  The band stages may overwrite choices and pulses as soon as the PACK
   kernels have read them, not only after the transfer: each pack runs on the stream of the band stage that
   overwrites its inputs next, so stream order alone holds that stage back (ev_exp_luma only tells the chroma
   chain that the luma totals are in the header it copies). */
int export_layout(const odhip_pipe *p, odhip_export_layout *lay) {
  long nblocks[2*ODHIP_NBSIZES];
  int bs[2*ODHIP_NBSIZES];
  int with_ref[2*ODHIP_NBSIZES];
  for (int i = 0; i < 5; i++) {
    nblocks[i] = p->set[0].nblocks[i];
    bs[i] = i;
    with_ref[i] = p->cfg.inter ? 1 : 0;    /* inter luma is coded against its prediction too */
  }
  const int nlev = p->set[1].nlev;
  for (int i = 0; i < nlev; i++) {
    nblocks[5 + i] = p->set[1].nblocks[i];
    bs[5 + i] = i;
    with_ref[5 + i] = 1;
  }
  return odhip_export_layout_make(lay, 5 + nlev, nblocks, bs, with_ref);
}

/* The pack kernels run INSIDE the chains, behind the stage whose outputs they read (luma: main stream, behind the
   choice; chroma: side stream, behind the band stage): on a stream of their own they waited for the searches of
   both chains to leave registers free (profiles/r6_overlap.txt) and held back, through their events, the band
   stages that reuse the buffers they read - 7.2 ms per step instead of 3.6. */
/* ODHIP_EXPORT_DBG (experiments build): bit 0 no pack kernels, bit 1 no copy of the fixed part, bit 2 no
   stream copies - which part of the export a step pays for. */
int export_dbg() {
  static int v = -1;
  if (v < 0) {
    const char *e = ODHIP_EXP_ENV("ODHIP_EXPORT_DBG");
    v = e ? atoi(e) : 0;
  }
  return v;
}

/* Where the step packed in export_dev[par] lands on the host: the single buffer, or its ring slot. */
uint8_t *export_dst(const odhip_pipe *p, int par) {
  if (p->ring.empty()) return p->export_host;
  return p->ring[(size_t)(p->exp_step[par] % (long)p->ring.size())];
}

/* The sections of plane set si (luma 0..4, chroma 5 ..) of the step at parity par, from the buffers its band stage
   left: keyframe luma without reference (the luma set of that parity), keyframe chroma and every inter plane with. */
int export_pack_set(odhip_pipe *p, int si, int par, hipStream_t s) {
  if (export_dbg() & 1) return ODHIP_SUCCESS;
  const PlaneSet &t = p->set[si];
  const int32_t *choice[ODHIP_NBSIZES];
  const int16_t *y[ODHIP_NBSIZES];
  long nblocks[ODHIP_NBSIZES];
  int bss[ODHIP_NBSIZES];
  for (int bs = 0; bs < t.nlev; bs++) {
    const JobAt j = job_at(p, si, bs, par);
    choice[bs] = j.ref ? j.ref->choice : j.noref->cands.choice;
    y[bs] = j.ref ? j.ref->y : j.noref->cands.y;
    nblocks[bs] = t.nblocks[bs];
    bss[bs] = bs;
  }
  return odhip_export_pack_multi(p->export_dev[par], &p->export_lay, si ? 5 : 0, t.nlev, choice, y, nblocks, bss,
   p->cfg.inter || si == 1, s);
}

int export_luma(odhip_pipe *p, int par) {
  hipStream_t s = p->stream[0];
  STEP_TRY(export_pack_set(p, 0, par, s));
  ODHIP_TRY(hipEventRecord(p->ev_exp_luma[par], s));
  return ODHIP_SUCCESS;
}

/* The chroma sections, then everything whose size the host knows - header, records, group bases - on its way on
   the export stream (copy engine: no compute unit involved).  The streams follow in export_finish. */
int export_chroma(odhip_pipe *p, int par) {
  hipStream_t s = p->stream[1];
  hipStream_t x = p->export_stream;
  STEP_TRY(export_pack_set(p, 1, par, s));
  /* the totals travel IN the chain (like the band stages' counts): on the export stream even this 128-byte copy
     waited for the searches */
  ODHIP_TRY(hipStreamWaitEvent(s, p->ev_exp_luma[par], 0));
  if (!(export_dbg() & 8)) {
    ODHIP_TRY(hipMemcpyAsync(p->export_hdr[par].p, p->export_dev[par], sizeof(odhip_export_header), hipMemcpyDeviceToHost, s));
  }
  ODHIP_TRY(hipEventRecord(p->ev_exp_hdr[par], s));
  ODHIP_TRY(hipStreamWaitEvent(x, p->ev_exp_hdr[par], 0));
  if (!(export_dbg() & 2)) {
    ODHIP_TRY(hipMemcpyAsync(export_dst(p, par), p->export_dev[par], (size_t)p->export_lay.fixed_bytes,
     hipMemcpyDeviceToHost, x));
  }
  p->export_pending = par;
  return ODHIP_SUCCESS;
}

/* A late resolve re-decided bands of plane set si of the step at parity par before its streams left (ring mode, and
   inter steps): those sections are packed again on the chain's stream s - behind the resolve and its re-run, before
   the next band stage of that set overwrites the choices and pulses (same stream) - with their totals cleared in
   stream order; export_finish then ships the header and the fixed part again, behind this. */
int export_repack(odhip_pipe *p, int si, int par, hipStream_t s) {
  const int first = si ? 5 : 0;
  const int n = p->set[si].nlev;
  odhip_export_header *h = reinterpret_cast<odhip_export_header *>(p->export_dev[par]);
  ODHIP_TRY(hipMemsetAsync(h->total_words + first, 0, sizeof(uint32_t)*n, s));
  ODHIP_TRY(hipMemsetAsync(h->overflow + first, 0, sizeof(uint32_t)*n, s));
  STEP_TRY(export_pack_set(p, si, par, s));
  ODHIP_TRY(hipEventRecord(p->ev_exp_repack, s));
  ODHIP_TRY(hipStreamWaitEvent(p->export_stream, p->ev_exp_repack, 0));
  p->export_redo = true;
  return ODHIP_SUCCESS;
}

/* The used part of every stream of the step packed last, once its totals have reached the host: called one
   step late (behind finish_pending, when the chroma band stage of that step is known to have ended) and from
   odhip_pipe_sync. */
int export_finish(odhip_pipe *p) {
  if (p->export_pending < 0) return ODHIP_SUCCESS;
  const int par = p->export_pending;
  p->export_pending = -1;
  if (!exporting(p)) return ODHIP_SUCCESS;
  uint8_t *dst = export_dst(p, par);
  if (p->export_redo) {
    /* behind the re-packs (export_repack): the new totals, then the fixed part again over the first copy */
    p->export_redo = false;
    ODHIP_TRY(hipMemcpyAsync(p->export_hdr[par].p, p->export_dev[par], sizeof(odhip_export_header), hipMemcpyDeviceToHost,
     p->export_stream));
    ODHIP_TRY(hipEventRecord(p->ev_exp_hdr[par], p->export_stream));
    ODHIP_TRY(hipMemcpyAsync(dst, p->export_dev[par], (size_t)p->export_lay.fixed_bytes, hipMemcpyDeviceToHost,
     p->export_stream));
  }
  if (!(export_dbg() & 16)) ODHIP_TRY(hipEventSynchronize(p->ev_exp_hdr[par]));
  const odhip_export_header *h = p->export_hdr[par].p;
  for (int s = 0; s < p->export_lay.nsections; s++) {
    const odhip_export_section &sec = p->export_lay.section[s];
    uint32_t words = h->total_words[s];
    if (words > sec.cap_words) words = sec.cap_words;
    const size_t bytes = ((size_t)words*2 + 15) & ~(size_t)15;
    if (bytes && !(export_dbg() & 4)) {
      ODHIP_TRY(hipMemcpyAsync(dst + sec.stream_off, p->export_dev[par] + sec.stream_off, bytes,
       hipMemcpyDeviceToHost, p->export_stream));
    }
  }
  /* export_dev[par] is packed again two steps later: totals and flags cleared for it */
  STEP_TRY(odhip_export_begin(p->export_dev[par], &p->export_lay, p->export_stream));
  ODHIP_TRY(hipEventRecord(p->ev_exp_sent[par], p->export_stream));
  if (!p->ring.empty()) {
    /* the step is complete once the export stream has come this far: odhip_pipe_export_take */
    const long st = p->exp_step[par];
    ODHIP_TRY(hipEventRecord(p->ring_slots.ev[(size_t)(st % (long)p->ring.size())], p->export_stream));
    p->ring_slots.sent = st + 1;
  }
  return ODHIP_SUCCESS;
}

int step_cfl(odhip_pipe *p) {
  hipStream_t main = p->stream[0];
  hipStream_t side = p->stream[1];
  const int par = (int)(p->nstep & 1);
  const bool exp_on = exporting(p);
  quants_point(p, 0, par);
  if (ciede_on(p)) {
    /* the last step is measured in front of this step's luma chain (ciede_hold), so its late resolve comes first and
       the chains no longer overlap (the calls below then find nothing pending) */
    STEP_TRY(finish_pending(p));
    STEP_TRY(metrics_finish(p, side));
  }
  {
    Current cur(p->ctx[0]);
    STEP_TRY(luma_front(p, main, par));
    STEP_TRY(luma_choose(p, main, par));
    /* this parity's export buffer: its last contents (step i - 2) have left and its header has been cleared behind
       them, on the export stream (export_finish) - not here: even a 128-byte memset in this chain waits for the
       other chain's searches to leave registers free (profiles/r6_overlap.txt) */
    if (exp_on) ODHIP_TRY(hipStreamWaitEvent(main, p->ev_exp_sent[par], 0));
    /* the luma choices of this step are final: the chroma chain takes its references from
       them (odhip_pvq_refjob.luma) */
    ODHIP_TRY(hipEventRecord(p->ev_refs[par], main));
    if (exp_on) STEP_TRY(export_luma(p, par));
    STEP_TRY(stage_inverse_noref(p, 0, main, par));
    STEP_TRY(measure(p, 0, par, main));
  }
  STEP_TRY(finish_pending(p));
  /* (the chroma band stage of the previous step has ended: its export is packed or about to be) */
  if (exp_on) STEP_TRY(export_finish(p));
  STEP_TRY(metrics_finish(p, side));
  {
    Current cur(p->ctx[1]);
    STEP_TRY(stage_pad(p, 1, side));
    STEP_TRY(stage_pyramid(p, 1, side));
    ODHIP_TRY(hipStreamWaitEvent(side, p->ev_refs[par], 0));
    /* (behind finish_pending: a resolve of the previous step re-runs it with the other parity's table) */
    quants_point(p, 1, par);
    STEP_TRY(quants_upload(p, 1, par, side));
    STEP_TRY(ref_bands(p, 1, par, side));
    /* only the preparation kernels of the band stage read the luma choices */
    ODHIP_TRY(hipEventRecord(p->ev_used[par], side));
    if (exp_on) STEP_TRY(export_chroma(p, par));
    STEP_TRY(ref_tail(p, 1, par, side));
  }
  p->pending = par;
  metrics_step_done(p, par);
  return ODHIP_SUCCESS;
}

}  // namespace

extern "C" odhip_pipe *odhip_pipe_create(const odhip_pipe_config *cfg) {
  /* (odd picture sizes are a 4:2:0 restriction of this pipe; the reference codes odd 4:4:4 sizes) */
  if (!cfg || !cfg->quant || cfg->frames <= 0 || cfg->pic_w <= 0 || cfg->pic_h <= 0
   || (cfg->chroma_444 != 0 && cfg->chroma_444 != 1)
   || (!cfg->chroma_444 && ((cfg->pic_w & 1) || (cfg->pic_h & 1)))
   || (cfg->fpr_bits != 0 && cfg->fpr_bits != 8 && cfg->fpr_bits != 10 && cfg->fpr_bits != 12)) {
    return nullptr;
  }
  odhip_pipe *p = new odhip_pipe();
  p->cfg = *cfg;
  p->use_masking = cfg->quant->use_masking;
  p->hvs_qm = cfg->quant->hvs_qm;
  p->met_depth = cfg->fpr_bits ? cfg->fpr_bits : 8;
  if (pipe_init(p) != ODHIP_SUCCESS) {
    odhip_pipe_destroy(p);
    return nullptr;
  }
  /* the quantiser tables were copied to the device; do not keep the caller's pointer */
  p->cfg.quant = nullptr;
  return p;
}

extern "C" int odhip_pipe_chroma_levels(const odhip_pipe *p) {
  return p ? p->set[1].nlev : ODHIP_EINVAL;
}

extern "C" void odhip_pipe_destroy(odhip_pipe *p) {
  if (!p) return;
  (void)hipSetDevice(p->cfg.device);
  (void)hipDeviceSynchronize();
  for (int i = 0; i < 2; i++) {
    if (p->ctx[i]) odhip_destroy(p->ctx[i]);
  }
  for (hipEvent_t e : p->owned_events) (void)hipEventDestroy(e);
  p->ring_slots.clear();
  p->met_slots.clear();
  if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
  if (p->export_stream) (void)hipStreamDestroy(p->export_stream);
  if (p->stream[1] && p->stream[1] != p->stream[0]) (void)hipStreamDestroy(p->stream[1]);
  if (p->stream[0]) (void)hipStreamDestroy(p->stream[0]);
  for (int i = 0; i < kStages; i++) {
    for (hipEvent_t e : p->timed[i]) (void)hipEventDestroy(e);
  }
  for (void *d : p->owned) (void)hipFree(d);
  delete p;     /* and the buffers that own themselves (met_*, export_hdr, qp_host) */
}

extern "C" int odhip_pipe_set_pictures(odhip_pipe *p, const uint8_t *luma, const uint8_t *chroma,
 int on_device) {
  if (!p || !luma || !chroma) return ODHIP_EINVAL;
  /* a step still in flight may be reading the pictures */
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  ODHIP_TRY(hipMemcpyAsync(p->set[0].pic, luma, picture_bytes(p, 0), kind, p->stream[0]));
  ODHIP_TRY(hipMemcpyAsync(p->set[1].pic, chroma, picture_bytes(p, 1), kind, p->stream[0]));
  ODHIP_TRY(hipStreamSynchronize(p->stream[0]));
  /* a feed that no step has taken yet is dropped: these are the pictures of the next step */
  ODHIP_TRY(hipStreamSynchronize(p->copy_stream));
  p->fed = false;
  return ODHIP_SUCCESS;
}

/* The pictures of the NEXT step, from host memory, while the steps already enqueued
   compute: copied on the pipe's own copy stream into the back buffers (after the padding
   kernels that may still read them), taken by the next odhip_pipe_step.  Pinned host
   memory (hipHostMalloc / hipHostRegister) makes the copy asynchronous; the buffers must
   stay valid until that step has been enqueued AND the copy has completed
   (odhip_pipe_sync waits for it too). */
extern "C" int odhip_pipe_feed(odhip_pipe *p, const uint8_t *luma, const uint8_t *chroma) {
  if (!p || !luma || !chroma) return ODHIP_EINVAL;
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  const int back = p->front ^ 1;
  ODHIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_pad[0], 0));
  ODHIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_pad[1], 0));
  /* the motion search of the last enqueued step reads the luma pictures behind its padding kernel */
  if (p->me_on) ODHIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_me, 0));
  ODHIP_TRY(hipMemcpyAsync(p->set[0].pic_buf[back], luma, picture_bytes(p, 0), hipMemcpyHostToDevice,
   p->copy_stream));
  ODHIP_TRY(hipMemcpyAsync(p->set[1].pic_buf[back], chroma, picture_bytes(p, 1), hipMemcpyHostToDevice,
   p->copy_stream));
  ODHIP_TRY(hipEventRecord(p->ev_fed, p->copy_stream));
  p->fed = true;
  return ODHIP_SUCCESS;
}

/* Size of the export buffer (odhip_pipe_set_export), 0 for the modes that do not export. */
extern "C" size_t odhip_pipe_export_bytes(const odhip_pipe *p) {
  /* keyframes with chroma from luma, and inter steps (every plane against its prediction), priced on the device */
  if (!p || !(p->cfg.chroma_cfl || p->cfg.inter) || !p->cfg.price) return 0;
  odhip_export_layout lay;
  if (export_layout(p, &lay) != ODHIP_SUCCESS) return 0;
  return (size_t)lay.total_bytes;
}

extern "C" int odhip_pipe_export_layout(const odhip_pipe *p, odhip_export_layout *out) {
  if (!p || !out) return ODHIP_EINVAL;
  if (odhip_pipe_export_bytes(p) == 0) return ODHIP_EIMPL;
  return export_layout(p, out);
}

extern "C" long odhip_pipe_export_stale(const odhip_pipe *p) {
  return p ? p->export_stale : 0;
}

namespace {
/* The export stream, its events and the two device buffers, on first use (set_export, set_export_ring; the pipe is
   idle).  Each object on its own: a call that failed half way is completed by the next one. */
int export_setup(odhip_pipe *p) {
  if (!p->export_stream) ODHIP_TRY(hipStreamCreateWithFlags(&p->export_stream, hipStreamNonBlocking));
  for (hipEvent_t *e : {&p->ev_exp_luma[0], &p->ev_exp_luma[1], &p->ev_exp_repack}) STEP_TRY(pipe_event(p, e));
  if (!p->export_dev[0]) {
    STEP_TRY(export_layout(p, &p->export_lay));
    for (int i = 0; i < 2; i++) {
      PIPE_ALLOC(p, p->export_dev[i], (size_t)p->export_lay.total_bytes, false);
      ODHIP_TRY(hipMemset(p->export_dev[i], 0, (size_t)p->export_lay.fixed_bytes));
      STEP_TRY(p->export_hdr[i].reserve(1));
      STEP_TRY(pipe_event(p, &p->ev_exp_hdr[i]));
      STEP_TRY(pipe_event(p, &p->ev_exp_sent[i]));
    }
  }
  return ODHIP_SUCCESS;
}
}  // namespace

/* host != NULL: every following step leaves its decisions - record and pulses of every band, compacted on the
   device (export_kernels.hip) - in `host`, odhip_pipe_export_bytes(p) bytes of pinned host memory, on the
   pipe's export stream, overlapped with the rest of the step; the buffer holds step i once odhip_pipe_sync()
   returns after step i.  NULL: stop exporting.  Device-priced keyframe steps with chroma from luma and inter
   steps only (ODHIP_EIMPL otherwise); ODHIP_EINVAL while a ring is set (odhip_pipe_set_export_ring). */
extern "C" int odhip_pipe_set_export(odhip_pipe *p, void *host) {
  if (!p) return ODHIP_EINVAL;
  if (!p->ring.empty()) return ODHIP_EINVAL;
  if (host && odhip_pipe_export_bytes(p) == 0) return ODHIP_EIMPL;
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  if (host) STEP_TRY(export_setup(p));
  p->export_pending = -1;
  if (host) {
    /* (the pipe is idle: odhip_pipe_sync above) */
    for (int i = 0; i < 2; i++) ODHIP_TRY(hipMemset(p->export_dev[i], 0, sizeof(odhip_export_header)));
  }
  p->export_host = static_cast<uint8_t *>(host);
  return ODHIP_SUCCESS;
}

/* n >= 2 pinned host buffers of odhip_pipe_export_bytes(p) bytes: step s from now on (s = 0, 1, ...) leaves in
   pinned[s % n] (odhip_pipe_export_take / _release).  NULL / n == 0: stop - the pipe is synced and the steps
   nobody took are dropped. */
extern "C" int odhip_pipe_set_export_ring(odhip_pipe *p, void *const *pinned, int n) {
  if (!p) return ODHIP_EINVAL;
  const bool on = pinned != nullptr && n != 0;
  if (on) {
    if (n < 2) return ODHIP_EINVAL;
    for (int i = 0; i < n; i++) {
      if (!pinned[i]) return ODHIP_EINVAL;
    }
    if (p->export_host) return ODHIP_EINVAL;      /* odhip_pipe_set_export holds the export */
    if (odhip_pipe_export_bytes(p) == 0) return ODHIP_EIMPL;
  }
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  p->ring_slots.clear();
  p->ring.clear();
  p->export_pending = -1;
  p->export_redo = false;
  if (!on) return ODHIP_SUCCESS;
  STEP_TRY(export_setup(p));
  STEP_TRY(p->ring_slots.create(n));
  /* headers cleared in order on the export stream, which the idle pipe then waits for */
  for (int i = 0; i < 2; i++) STEP_TRY(odhip_export_begin(p->export_dev[i], &p->export_lay, p->export_stream));
  ODHIP_TRY(hipStreamSynchronize(p->export_stream));
  for (int i = 0; i < n; i++) p->ring.push_back(static_cast<uint8_t *>(pinned[i]));
  return ODHIP_SUCCESS;
}

/* 1: the oldest untaken complete step - its number, its slot and the sections whose stream overflowed (bit s);
   0: none (wait = 1 blocks only for a step whose copies are enqueued). */
extern "C" int odhip_pipe_export_take(odhip_pipe *p, int wait, long *step, void **buf, uint32_t *overflow) {
  if (!p || !step || !buf || p->ring.empty()) return ODHIP_EINVAL;
  long s = 0;
  size_t slot = 0;
  const int rc = p->ring_slots.poll(wait != 0, &s, &slot);
  if (rc <= 0) return rc;
  const odhip_export_header *h = reinterpret_cast<const odhip_export_header *>(p->ring[slot]);
  uint32_t mask = 0;
  for (int i = 0; i < p->export_lay.nsections; i++) {
    if (h->overflow[i]) mask |= 1u << i;
  }
  *step = s;
  *buf = p->ring[slot];
  if (overflow) *overflow = mask;
  p->ring_slots.taken = s + 1;
  return 1;
}

/* The oldest taken step's slot may be written again. */
extern "C" int odhip_pipe_export_release(odhip_pipe *p, long step) {
  if (!p || p->ring.empty()) return ODHIP_EINVAL;
  if (step != p->ring_slots.released || step >= p->ring_slots.taken) return ODHIP_EINVAL;
  p->ring_slots.released = step + 1;
  return ODHIP_SUCCESS;
}

/* Picture f of every following step at quants[f] (plane sets: luma plane f, chroma planes f (Cb, pli 1) and
   F + f (Cr, pli 2)); NULL / n == 0: the config's quant again.  Steps already enqueued keep theirs. */
extern "C" int odhip_pipe_set_quants(odhip_pipe *p, const odhip_quant *const *quants, int n) {
  if (!p) return ODHIP_EINVAL;
  if (!quants || n == 0) {
    p->qp_next.clear();
    return ODHIP_SUCCESS;
  }
  const int F = p->cfg.frames;
  if (n != F) return ODHIP_EINVAL;
  for (int f = 0; f < F; f++) {
    /* the QM tables and the OD_PVQ_BETA rows are the pipe's: only the steps may differ */
    if (!quants[f] || quants[f]->use_masking != p->use_masking || quants[f]->hvs_qm != p->hvs_qm) {
      return ODHIP_EINVAL;
    }
  }
  size_t words = 0;
  for (int si = 0; si < 2; si++) {
    p->qp_set[si][0] = words;
    for (int bs = 0; bs < p->set[si].nlev; bs++) {
      p->qp_off[si][bs] = words;
      words += (size_t)p->set[si].nplanes*ODHIP_MAX_BANDS;
    }
    p->qp_set[si][1] = words - p->qp_set[si][0];
  }
  std::vector<int32_t> next(words, 0);
  for (int si = 0; si < 2; si++) {
    const PlaneSet &t = p->set[si];
    for (int bs = 0; bs < t.nlev; bs++) {
      for (int pl = 0; pl < t.nplanes; pl++) {
        const int f = si == 0 || pl < F ? pl : pl - F;
        const int pli = si == 0 ? 0 : pl < F ? 1 : 2;
        int32_t *row = next.data() + p->qp_off[si][bs] + (size_t)pl*ODHIP_MAX_BANDS;
        const int nb = odhip_quant_bands(quants[f], pli, bs, row, nullptr);
        if (nb <= 0) return ODHIP_EINVAL;
        for (int b = 0; b < nb; b++) {
          if (row[b] < 1) return ODHIP_EINVAL;
        }
      }
    }
  }
  if (!p->qp_dev[0]) {
    ODHIP_TRY(hipSetDevice(p->cfg.device));
    for (int i = 0; i < 2; i++) {
      PIPE_ALLOC(p, p->qp_dev[i], sizeof(int32_t)*words, true);
      STEP_TRY(p->qp_host[i].reserve(words));
      for (int si = 0; si < 2; si++) STEP_TRY(pipe_event(p, &p->ev_qp[i][si]));
    }
  }
  p->qp_next.swap(next);
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_step(odhip_pipe *p) {
  if (!p) return ODHIP_EINVAL;
  /* ring mode: this step's slot still holds step ring_slots.next - n until the host releases it - enqueue nothing */
  const bool ring = !p->ring.empty();
  if (ring && p->ring_slots.full()) return ODHIP_EBUSY;
  /* ... and so does a metrics slot that holds an untaken step */
  if (p->met_flags && p->met_slots.full()) return ODHIP_EBUSY;
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  if (ring) p->exp_step[p->nstep & 1] = p->ring_slots.next;
  p->met_step[p->nstep & 1] = p->met_flags ? p->met_slots.next++ : -1;
  if (p->fed) {
    /* odhip_pipe_feed: this step codes the fed pictures */
    p->front ^= 1;
    p->set[0].pic = p->set[0].pic_buf[p->front];
    p->set[1].pic = p->set[1].pic_buf[p->front];
    ODHIP_TRY(hipStreamWaitEvent(p->stream[0], p->ev_fed, 0));
    if (p->stream[1] != p->stream[0]) ODHIP_TRY(hipStreamWaitEvent(p->stream[1], p->ev_fed, 0));
    p->fed = false;
  }
  if (p->mc_ffed || p->mc_gfed) {
    /* odhip_pipe_feed_reference_frames / _feed_mvs: this step predicts from what was fed */
    if (p->mc_ffed) p->mc_ffront ^= 1;
    if (p->mc_gfed) {
      p->mc_gfront ^= 1;
      p->mc_grid_set = true;
    }
    ODHIP_TRY(hipStreamWaitEvent(p->stream[0], p->ev_mc_fed, 0));
    if (p->stream[1] != p->stream[0]) ODHIP_TRY(hipStreamWaitEvent(p->stream[1], p->ev_mc_fed, 0));
    p->mc_ffed = p->mc_gfed = false;
  }
  const int rc = p->cfg.inter ? step_inter(p) : p->cfg.chroma_cfl ? step_cfl(p) : step_noref(p);
  p->nstep++;
  if (ring) p->ring_slots.next++;
  return rc;
}

extern "C" int odhip_pipe_flush(odhip_pipe *p) {
  if (!p) return ODHIP_EINVAL;
  if (p->cfg.inter) {
    STEP_TRY(inter_finish(p, 0));
    STEP_TRY(inter_finish(p, 1));
  }
  else {
    p->in_flush = true;
    const int rc = finish_pending(p);
    p->in_flush = false;
    if (rc) return rc;
  }
  /* ring mode: the last step's resolve is done - its streams leave now and odhip_pipe_export_take can wait for it */
  if (!p->ring.empty()) STEP_TRY(export_finish(p));
  /* ... and so are its metrics */
  return metrics_finish(p, p->stream[1]);
}

/* Inter mode: the prediction pictures (what motion compensation produced for each picture
   of the batch), same layouts and depth as odhip_pipe_set_pictures. */
extern "C" int odhip_pipe_set_reference_pictures(odhip_pipe *p, const uint8_t *luma, const uint8_t *chroma,
 int on_device) {
  if (!p || !luma || !chroma || !p->cfg.inter) return ODHIP_EINVAL;
  /* a step takes its prediction one way: drop the grids first (odhip_pipe_set_mvs(p, NULL)) */
  if (p->mc_grid_set || p->mc_gfed || p->me_on) return ODHIP_EINVAL;
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  ODHIP_TRY(hipMemcpyAsync(p->set[0].pred_pic, luma, picture_bytes(p, 0), kind, p->stream[0]));
  ODHIP_TRY(hipMemcpyAsync(p->set[1].pred_pic, chroma, picture_bytes(p, 1), kind, p->stream[0]));
  ODHIP_TRY(hipStreamSynchronize(p->stream[0]));
  return ODHIP_SUCCESS;
}

namespace {

size_t mc_grid_points(const odhip_pipe *p) {
  return (size_t)p->cfg.frames*(p->W/8 + 1)*(p->H/8 + 1);
}

/* both decimations of the pipe, every slot in range */
int mc_check(const odhip_pipe *p, const odhip_mv_point *grid) {
  const int rc = odhip_mc_check_grid(grid, p->W, p->H, p->cfg.frames, 0, p->mc_nslots);
  if (rc || !p->cdec) return rc;
  return odhip_mc_check_grid(grid, p->W, p->H, p->cfg.frames, p->cdec, p->mc_nslots);
}

int mc_alloc(odhip_pipe *p, int nslots) {
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  for (int b = 0; b < 2; b++) {
    for (int si = 0; si < 2; si++) {
      for (int r = 0; r < nslots; r++) {
        if (!p->mc_ref[b][si][r]) PIPE_ALLOC(p, p->mc_ref[b][si][r], plane_bytes(p, si), true);
      }
    }
    if (!p->mc_grid[b]) PIPE_ALLOC(p, p->mc_grid[b], mc_grid_points(p)*sizeof(odhip_mv_point), true);
  }
  if (!p->ev_mc_fed) {
    for (hipEvent_t *e : {&p->ev_mc[0], &p->ev_mc[1], &p->ev_mc_fed}) STEP_TRY(pipe_event(p, e));
    /* the leaf buckets of each chain's context, so that no step allocates */
    for (int si = 0; si < 2; si++) {
      Current cur(p->ctx[si]);
      STEP_TRY(odhip_mc_prepare(p->W, p->H, p->cfg.frames));
    }
  }
  return ODHIP_SUCCESS;
}

}  // namespace

/* Inter mode: the reference frames every step predicts from until others are set or fed - nslots (1..3) plane sets
   of the CODED size in the planes' sample type (uint8, with fpr_bits int16 at 12 bits), luma[slot]: [F][H][W],
   chroma[slot]: [2F][H >> cdec][W >> cdec].  Syncs the pipe (resident data, like odhip_pipe_set_pictures).  nslots 0
   drops frames and grids: odhip_pipe_set_reference_pictures supplies the prediction again. */
extern "C" int odhip_pipe_set_reference_frames(odhip_pipe *p, int nslots, const void *const *luma,
 const void *const *chroma, int on_device) {
  if (!p || !p->cfg.inter || nslots < 0 || nslots > 3 || (nslots && (!luma || !chroma))) return ODHIP_EINVAL;
  for (int r = 0; r < nslots; r++) {
    if (!luma[r] || !chroma[r]) return ODHIP_EINVAL;
  }
  int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  p->mc_ffed = false;
  if (nslots == 0) {
    p->mc_nslots = 0;
    p->mc_grid_set = p->mc_gfed = p->me_on = false;
    return ODHIP_SUCCESS;
  }
  /* a resident grid was checked against the slots it had */
  if (p->mc_grid_set && nslots < p->mc_nslots) return ODHIP_EINVAL;
  rc = mc_alloc(p, nslots);
  if (rc) return rc;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  for (int r = 0; r < nslots; r++) {
    ODHIP_TRY(hipMemcpyAsync(p->mc_ref[p->mc_ffront][0][r], luma[r], plane_bytes(p, 0), kind, p->stream[0]));
    ODHIP_TRY(hipMemcpyAsync(p->mc_ref[p->mc_ffront][1][r], chroma[r], plane_bytes(p, 1), kind, p->stream[0]));
  }
  ODHIP_TRY(hipStreamSynchronize(p->stream[0]));
  p->mc_nslots = nslots;
  return ODHIP_SUCCESS;
}

/* The resident grids ([F][H/8 + 1][W/8 + 1], host memory): checked for the luma and the chroma decimation
   (ODHIP_ERANGE / ODHIP_EINVAL: nothing changes), then every inter step builds its prediction from them.  NULL: no
   grid - the pipe pads and transforms the pictures of odhip_pipe_set_reference_pictures as before.  Syncs. */
extern "C" int odhip_pipe_set_mvs(odhip_pipe *p, const odhip_mv_point *grid) {
  if (!p || !p->cfg.inter || p->me_on) return ODHIP_EINVAL;
  if (grid) {
    if (!p->mc_nslots) return ODHIP_EINVAL;
    const int rc = mc_check(p, grid);
    if (rc) return rc;
  }
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  p->mc_gfed = false;
  if (!grid) {
    p->mc_grid_set = false;
    return ODHIP_SUCCESS;
  }
  ODHIP_TRY(hipMemcpy(p->mc_grid[p->mc_gfront], grid, mc_grid_points(p)*sizeof(odhip_mv_point),
   hipMemcpyHostToDevice));
  p->mc_grid_set = true;
  return ODHIP_SUCCESS;
}

/* The reference frames / the grids of the NEXT step from (pinned) host memory, like odhip_pipe_feed: copied on the
   copy stream into the back buffers, behind the prediction kernels that may still read them, without a sync; the next
   odhip_pipe_step takes them, the steps already enqueued keep theirs.  The slots are those of
   odhip_pipe_set_reference_frames (call it once first).  The host buffers stay valid until that step is enqueued and
   the copy has completed. */
extern "C" int odhip_pipe_feed_reference_frames(odhip_pipe *p, const void *const *luma, const void *const *chroma) {
  if (!p || !p->cfg.inter || !p->mc_nslots || !luma || !chroma) return ODHIP_EINVAL;
  for (int r = 0; r < p->mc_nslots; r++) {
    if (!luma[r] || !chroma[r]) return ODHIP_EINVAL;
  }
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  const int back = p->mc_ffront ^ 1;
  ODHIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_mc[0], 0));
  ODHIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_mc[1], 0));
  for (int r = 0; r < p->mc_nslots; r++) {
    ODHIP_TRY(hipMemcpyAsync(p->mc_ref[back][0][r], luma[r], plane_bytes(p, 0), hipMemcpyHostToDevice,
     p->copy_stream));
    ODHIP_TRY(hipMemcpyAsync(p->mc_ref[back][1][r], chroma[r], plane_bytes(p, 1), hipMemcpyHostToDevice,
     p->copy_stream));
  }
  ODHIP_TRY(hipEventRecord(p->ev_mc_fed, p->copy_stream));
  p->mc_ffed = true;
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_feed_mvs(odhip_pipe *p, const odhip_mv_point *grid) {
  if (!p || !p->cfg.inter || !p->mc_nslots || !grid || p->me_on) return ODHIP_EINVAL;
  const int rc = mc_check(p, grid);
  if (rc) return rc;
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  const int back = p->mc_gfront ^ 1;
  ODHIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_mc[0], 0));
  ODHIP_TRY(hipStreamWaitEvent(p->copy_stream, p->ev_mc[1], 0));
  ODHIP_TRY(hipMemcpyAsync(p->mc_grid[back], grid, mc_grid_points(p)*sizeof(odhip_mv_point), hipMemcpyHostToDevice,
   p->copy_stream));
  ODHIP_TRY(hipEventRecord(p->ev_mc_fed, p->copy_stream));
  p->mc_gfed = true;
  return ODHIP_SUCCESS;
}

/* Every inter step searches its grids itself (include/daala_hip.h); range < 0 switches the search off, and the steps
   take their prediction from odhip_pipe_set_mvs / odhip_pipe_set_reference_pictures again.  Syncs. */
extern "C" int odhip_pipe_set_motion_search(odhip_pipe *p, int log_size, int range, int res, int lambda) {
  return odhip_pipe_set_motion_search2(p, log_size, range, res, lambda, lambda, 0);
}

extern "C" int odhip_pipe_set_motion_search2(odhip_pipe *p, int log_size, int range, int res, int lambda,
 int lambda_subpel, int flags) {
  return odhip_pipe_set_motion_search3(p, log_size, range, res, lambda, lambda_subpel, flags, 0, 1);
}

extern "C" int odhip_pipe_set_motion_search3(odhip_pipe *p, int log_size, int range, int res, int lambda,
 int lambda_subpel, int flags, int levels, int refine) {
  return odhip_pipe_set_motion_search_vbs(p, log_size, log_size, range, res, lambda, lambda_subpel, flags, levels,
   refine, 0);
}

extern "C" int odhip_pipe_set_motion_search_vbs(odhip_pipe *p, int log_min, int log_size, int range, int res,
 int lambda, int lambda_subpel, int flags, int levels, int refine, int split_penalty) {
  if (!p || !p->cfg.inter) return ODHIP_EINVAL;
  if (range < 0) {
    if (!p->me_on) return ODHIP_SUCCESS;
    const int rc = odhip_pipe_sync(p);
    if (rc) return rc;
    p->me_on = false;
    return ODHIP_SUCCESS;
  }
  if (p->cfg.fpr_bits) return ODHIP_EIMPL;
  /* a step takes its grids one way: drop resident or fed ones first (odhip_pipe_set_mvs(p, NULL)) */
  if (!p->mc_nslots || p->mc_grid_set || p->mc_gfed) return ODHIP_EINVAL;
  if (log_size < 0 || log_size > 3 || log_min < 0 || log_min > log_size || split_penalty < 0
   || split_penalty > 1 << 24 || range > 32 || res < 0 || res > 3 || lambda < 0 || lambda > 1 << 20
   || lambda_subpel < 0 || lambda_subpel > 1 << 20 || (flags & ~(ODHIP_ME_CHROMA | ODHIP_ME_SATD)) || levels < 0
   || levels > 2 || levels > log_size + 1
   || (levels && (refine < 1 || refine > 8 || lambda > 1 << 19 || lambda_subpel > 1 << 19))) {
    return ODHIP_EINVAL;
  }
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  /* the scratch of the job the steps will run: its size follows the pipe's sizes, the block sizes and levels */
  odhip_me_job4 job4;
  motion_job(p, &job4);
  job4.base.base.luma.log_size = log_size;
  job4.base.base.luma.nrefs = 3;             /* whatever number of slots later reference frames bring */
  job4.base.levels = levels;
  job4.log_min = log_min;
  const size_t need = odhip_me_vbs_scratch_bytes(&job4);
  if (need > p->me_scratch_bytes) {
    PIPE_ALLOC(p, p->me_scratch, need, false);   /* (a smaller one it replaces stays owned until the pipe goes) */
    p->me_scratch_bytes = need;
  }
  for (int b = 0; b < 2; b++) {
    if (!p->me_cost[b]) PIPE_ALLOC(p, p->me_cost[b], mc_grid_points(p)*sizeof(uint32_t), true);
  }
  if (!p->ev_me) STEP_TRY(pipe_event(p, &p->ev_me));
  p->me_log_size = log_size;
  p->me_range = range;
  p->me_res = res;
  p->me_lambda = lambda;
  p->me_lambda_subpel = lambda_subpel;
  p->me_flags = flags;
  p->me_levels = levels;
  p->me_refine = refine;
  p->me_log_min = log_min;
  p->me_split_penalty = split_penalty;
  p->me_on = true;
  return ODHIP_SUCCESS;
}

/* The grids the last enqueued step predicted from, and - while the search is on - their winners' costs.  Syncs. */
extern "C" int odhip_pipe_mvs_read(odhip_pipe *p, odhip_mv_point *grid, uint32_t *cost) {
  if (!p || !grid || !p->cfg.inter || !p->nstep || !(p->me_on || p->mc_grid_set) || (cost && !p->me_on)) {
    return ODHIP_EINVAL;
  }
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  const size_t points = mc_grid_points(p);
  ODHIP_TRY(hipMemcpy(grid, p->mc_grid[p->mc_gfront], points*sizeof(odhip_mv_point), hipMemcpyDeviceToHost));
  if (cost) ODHIP_TRY(hipMemcpy(cost, p->me_cost[p->mc_gfront], points*sizeof(uint32_t), hipMemcpyDeviceToHost));
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_sync(odhip_pipe *p) {
  if (!p) return ODHIP_EINVAL;
  ODHIP_TRY(hipStreamSynchronize(p->stream[0]));
  if (p->stream[1] != p->stream[0]) ODHIP_TRY(hipStreamSynchronize(p->stream[1]));
  ODHIP_TRY(hipStreamSynchronize(p->copy_stream));
  if (p->export_stream) {
    /* (a ring step whose late resolve has not run yet is completed by the next step or odhip_pipe_flush) */
    const bool resolved = p->pending < 0 && !p->inter_pending[0] && !p->inter_pending[1];
    if (p->ring.empty() || resolved) STEP_TRY(export_finish(p));
    ODHIP_TRY(hipStreamSynchronize(p->export_stream));
  }
  /* bands whose reference candidate has more pulses than the pulse vectors hold (include/daala_hip.h,
     ODHIP_PVQ_MAX_K): their results are not the reference's - say so */
  unsigned kr[2] = {0, 0};
  for (int i = 0; i < 2; i++) {
    /* the counters belong to the contexts of the two chains */
    if (i == 1 && p->ctx[1] == p->ctx[0]) break;
    Current cur(p->ctx[i]);
    unsigned a = 0;
    unsigned b = 0;
    const int rc = odhip_pvq_k_range_take(&a, &b);
    if (rc != ODHIP_SUCCESS && rc != ODHIP_ERANGE) return rc;
    kr[0] += a;
    kr[1] += b;
  }
  p->k_range += (long)kr[0] + kr[1];
  if (kr[0] || kr[1]) {
    fprintf(stderr, "libdaalahip: %u + %u band(s) need more than %d pulses (quantiser too fine for the int16 pulse "
     "vectors): the steps since the last odhip_pipe_sync are not the reference's\n", kr[0], kr[1], ODHIP_PVQ_MAX_K);
    return ODHIP_ERANGE;
  }
  return ODHIP_SUCCESS;
}

/* Bands counted by odhip_pvq_k_range_take at this pipe's syncs so far. */
extern "C" long odhip_pipe_k_range(const odhip_pipe *p) {
  return p ? p->k_range : 0;
}

/* The stages one at a time, in order on the luma stream (tests, the priced
   verification flow of bench.py: the host prices candidates between the band
   stage and the choice).  parity selects the reference buffer. */
extern "C" int odhip_pipe_stage(odhip_pipe *p, int stage, int parity) {
  if (!p || stage < 0 || stage >= kStages || (parity != 0 && parity != 1)) return ODHIP_EINVAL;
  if (p->cfg.inter) return ODHIP_EINVAL;       /* inter mode runs whole steps only */
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  hipStream_t s = p->stream[0];
  const bool cfl = p->cfg.chroma_cfl != 0;
  const double lam = p->cfg.pvq_norm_lambda;
  const bool chroma_stage = stage == ODHIP_PIPE_PAD_CHROMA || stage == ODHIP_PIPE_PYRAMID_CHROMA
   || stage == ODHIP_PIPE_BANDS_CHROMA || stage == ODHIP_PIPE_CHOOSE_CHROMA
   || stage == ODHIP_PIPE_INVERSE_CHROMA;
  Current cur(p->ctx[chroma_stage && cfl ? 1 : 0]);
  const int jpar = cfl ? parity : 0;     /* the luma set of that parity */
  switch (stage) {
    case ODHIP_PIPE_PAD_LUMA: return stage_pad(p, 0, s);
    case ODHIP_PIPE_PYRAMID_LUMA: return stage_pyramid(p, 0, s);
    case ODHIP_PIPE_PAD_CHROMA: return stage_pad(p, 1, s);
    case ODHIP_PIPE_PYRAMID_CHROMA: return stage_pyramid(p, 1, s);
    case ODHIP_PIPE_BANDS_LUMA: {
      /* the quantisers in force now (odhip_pipe_set_quants), for this stage and those behind it */
      for (int si = 0; si < (cfl ? 1 : 2); si++) {
        quants_point(p, si, parity);
        STEP_TRY(quants_upload(p, si, parity, s));
      }
      return luma_bands(p, s, jpar);
    }
    case ODHIP_PIPE_CHOOSE_LUMA: return luma_choose(p, s, jpar);
    /* (the references are read in place from the luma choices, 4:2:0 and 4:4:4 alike: nothing to run) */
    case ODHIP_PIPE_CFL_REFS: return cfl ? ODHIP_SUCCESS : ODHIP_EINVAL;
    case ODHIP_PIPE_INVERSE_LUMA: return stage_inverse_noref(p, 0, s, jpar);
    case ODHIP_PIPE_BANDS_CHROMA: {
      if (!cfl) return ODHIP_SUCCESS;      /* part of ODHIP_PIPE_BANDS_LUMA */
      quants_point(p, 1, parity);
      STEP_TRY(quants_upload(p, 1, parity, s));
      STEP_TRY(ref_bands(p, 1, parity, s));
      /* (at once: nothing runs beside a single stage, and no tail has consumed the choices yet) */
      const int n = odhip_pvq_ref_resolve_finish(ref_jobs(p, 1, parity), p->set[1].nlev, lam, s);
      if (n < 0) return n;
      p->reruns += n;
      return ODHIP_SUCCESS;
    }
    case ODHIP_PIPE_CHOOSE_CHROMA: {
      if (!cfl) return ODHIP_SUCCESS;
      if (p->cfg.price) {
        /* the band stage decided; what is left is the host-libm resolve of listed bands */
        const int m = odhip_pvq_ref_choose_priced_resolve(ref_jobs(p, 1, parity), p->set[1].nlev, lam, s);
        if (m < 0) return m;
        p->price_reruns += m;
        return ODHIP_SUCCESS;
      }
      return ref_choose(p, 1, parity, s);
    }
    case ODHIP_PIPE_INVERSE_CHROMA: return cfl ? ref_inverse(p, 1, parity, s) : stage_inverse_noref(p, 1, s, 0);
    default: return ODHIP_EINVAL;
  }
}

extern "C" int odhip_pipe_buffer(odhip_pipe *p, int what, int set, int level, int parity, void **d_ptr,
 size_t *bytes) {
  if (!p || !d_ptr || !bytes || (set != 0 && set != 1) || parity < -1 || parity > 1) {
    return ODHIP_EINVAL;
  }
  /* -1: the buffers of the LAST odhip_pipe_step (the luma choices and the chroma references
     alternate between two sets from step to step) */
  if (parity < 0) parity = p->nstep > 0 ? (int)((p->nstep - 1) & 1) : 0;
  PlaneSet &t = p->set[set];
  if (what != ODHIP_PIPE_BUF_PIC && what != ODHIP_PIPE_BUF_PX && what != ODHIP_PIPE_BUF_PRED && (level < 0 || level >= t.nlev)) {
    return ODHIP_EINVAL;
  }
  int nb = 0;
  int len = 0;
  if (level >= 0 && level < ODHIP_NBSIZES) odhip_pvq_band_layout(level, &nb, nullptr, &len);
  const long B = level >= 0 && level < ODHIP_NBSIZES ? t.nblocks[level] : 0;
  const bool inter = p->cfg.inter != 0;
  /* (the buffers of a level; BUF_PIC, BUF_PX and BUF_PRED take any level and use neither) */
  const JobAt at = level >= 0 && level < t.nlev ? job_at(p, set, level, parity) : JobAt{nullptr, nullptr};
  const odhip_pvq_job *j = at.noref;
  const odhip_pvq_refjob *r = at.ref;
  void *ptr = nullptr;
  size_t n = 0;
  switch (what) {
    case ODHIP_PIPE_BUF_PIC: ptr = t.pic; n = picture_bytes(p, set); break;
    case ODHIP_PIPE_BUF_PX: ptr = t.px; n = plane_bytes(p, set); break;
    case ODHIP_PIPE_BUF_LEVEL: ptr = t.levels[level]; n = sizeof(od_coeff)*(size_t)t.nplanes*t.w*t.h; break;
    case ODHIP_PIPE_BUF_RECON: ptr = t.recon[level]; n = plane_bytes(p, set); break;
    case ODHIP_PIPE_BUF_BAND:
      ptr = j ? (void *)j->cands.band : (void *)r->band;
      n = (size_t)64*B*nb;
      break;
    case ODHIP_PIPE_BUF_Y:
      ptr = j ? j->cands.y : r->y;
      n = sizeof(int16_t)*(size_t)(j ? 2 : ODHIP_PVQ_REF_SLOTS)*B*len;
      break;
    case ODHIP_PIPE_BUF_CHOICE:
      ptr = j ? j->cands.choice : r->choice;
      n = sizeof(int32_t)*(size_t)B*nb*(j ? 4 : 16);
      break;
    case ODHIP_PIPE_BUF_ITEMS:
      if (!r) return ODHIP_EINVAL;
      ptr = r->items;
      n = (size_t)3*nb*ODHIP_PVQ_REF_SLOTS*B*16;
      break;
    case ODHIP_PIPE_BUF_REF:
      if (!r) return ODHIP_EINVAL;
      /* inter mode: the reference of every block is the pyramid of its prediction picture;
         keyframe chroma takes its reference from the luma choices in place: no plane exists */
      if (!inter) return ODHIP_EINVAL;
      ptr = t.pred_levels[level];
      n = sizeof(od_coeff)*(size_t)t.nplanes*t.w*t.h;
      break;
    case ODHIP_PIPE_BUF_RATE: {
      /* allocated (zero: every candidate free = choice on distortion alone) and
         attached on first request: [B][nb][2] without reference,
         [B][nb][ODHIP_PVQ_REF_SLOTS + 1] with */
      n = sizeof(double)*(size_t)B*nb*(j ? 2 : ODHIP_PVQ_REF_SLOTS + 1);
      if (!p->rate[set][level]) {
        ODHIP_TRY(hipSetDevice(p->cfg.device));
        PIPE_ALLOC(p, p->rate[set][level], n, true);
        for (int par = 0; par < 2; par++) {
          const JobAt a = job_at(p, set, level, par);
          if (a.ref) a.ref->d_rate = p->rate[set][level];
          else a.noref->d_rate = p->rate[set][level];
        }
      }
      ptr = p->rate[set][level];
      break;
    }
    case ODHIP_PIPE_BUF_PRED:
      if (!inter) return ODHIP_EINVAL;
      ptr = t.pred_px;
      n = plane_bytes(p, set);
      break;
    default: return ODHIP_EINVAL;
  }
  *d_ptr = ptr;
  *bytes = n;
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_read(odhip_pipe *p, void *host, const void *d_ptr, size_t bytes) {
  if (!p || !host || !d_ptr) return ODHIP_EINVAL;
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  ODHIP_TRY(hipMemcpy(host, d_ptr, bytes, hipMemcpyDeviceToHost));
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_write(odhip_pipe *p, void *d_ptr, const void *host, size_t bytes) {
  if (!p || !host || !d_ptr) return ODHIP_EINVAL;
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  ODHIP_TRY(hipMemcpy(d_ptr, host, bytes, hipMemcpyHostToDevice));
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_record(odhip_pipe *p, int enable) {
  if (!p) return ODHIP_EINVAL;
  p->record = enable != 0;
  for (int i = 0; i < kStages; i++) {
    for (hipEvent_t e : p->timed[i]) (void)hipEventDestroy(e);
    p->timed[i].clear();
  }
  /* the dominant kernels of the two band stages, on the streams they run on */
  {
    Current cur(p->ctx[0]);
    const int rc = odhip_pvq_profile(enable);
    if (rc) return rc;
  }
  if (p->cfg.chroma_cfl) {
    Current cur(p->ctx[1]);
    const int rc = odhip_pvq_ref_profile(enable);
    if (rc) return rc;
  }
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_timings(odhip_pipe *p, double avg_ms[ODHIP_PIPE_NSTAGES],
 int count[ODHIP_PIPE_NSTAGES]) {
  if (!p || !avg_ms || !count) return ODHIP_EINVAL;
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  for (int i = 0; i < kStages; i++) {
    double sum = 0;
    int n = 0;
    for (size_t k = 0; k + 1 < p->timed[i].size(); k += 2) {
      float ms = 0;
      ODHIP_TRY(hipEventElapsedTime(&ms, p->timed[i][k], p->timed[i][k + 1]));
      sum += ms;
      n++;
    }
    avg_ms[i] = n ? sum/n : 0;
    count[i] = n;
  }
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_search_timings(odhip_pipe *p, int chroma, float *ms, int max_n) {
  if (!p || !ms) return ODHIP_EINVAL;
  if (chroma && !p->cfg.chroma_cfl) return 0;
  Current cur(p->ctx[chroma ? 1 : 0]);
  return chroma ? odhip_pvq_ref_profile_read(ms, max_n) : odhip_pvq_profile_read(ms, max_n);
}

/* The luma forward pyramid launched n times on an otherwise idle GPU: average
   milliseconds per launch (the filter + DCT stage of the north star, timed alone). */
extern "C" int odhip_pipe_time_pyramid(odhip_pipe *p, int n, double *avg_ms) {
  if (!p || n <= 0 || !avg_ms) return ODHIP_EINVAL;
  int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  hipStream_t s = p->stream[0];
  PlaneSet &t = p->set[0];
  hipEvent_t a = nullptr;
  hipEvent_t b = nullptr;
  ODHIP_TRY(hipEventCreate(&a));
  ODHIP_TRY(hipEventCreate(&b));
  rc = pyramid(p, 0, t.levels, t.px, s);
  (void)hipEventRecord(a, s);
  for (int i = 0; i < n && !rc; i++) rc = pyramid(p, 0, t.levels, t.px, s);
  (void)hipEventRecord(b, s);
  float ms = 0;
  if (!rc && (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess)) {
    rc = ODHIP_EFAULT;
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *avg_ms = ms/n;
  return rc;
}

/* One filter + DCT stage (padding, forward pyramid or dequantise + inverse of one plane set)
   launched n times on an otherwise idle GPU, on the buffers the last step left: average
   milliseconds per launch group.  parity as for odhip_pipe_stage (-1: the last step's). */
extern "C" int odhip_pipe_time_stage(odhip_pipe *p, int stage, int parity, int n, double *avg_ms) {
  if (!p || n <= 0 || !avg_ms || parity < -1 || parity > 1) return ODHIP_EINVAL;
  if (stage != ODHIP_PIPE_PAD_LUMA && stage != ODHIP_PIPE_PAD_CHROMA && stage != ODHIP_PIPE_PYRAMID_LUMA
   && stage != ODHIP_PIPE_PYRAMID_CHROMA && stage != ODHIP_PIPE_INVERSE_LUMA && stage != ODHIP_PIPE_INVERSE_CHROMA) {
    return ODHIP_EINVAL;     /* the other stages are not idempotent on their own buffers */
  }
  if (parity < 0) parity = p->nstep > 0 ? (int)((p->nstep - 1) & 1) : 0;
  int rc = odhip_pipe_flush(p);
  if (rc) return rc;
  rc = odhip_pipe_sync(p);
  if (rc) return rc;
  hipStream_t s = p->stream[0];
  hipEvent_t a = nullptr;
  hipEvent_t b = nullptr;
  /* the events first: a failure here must neither leak one nor leave recording switched off */
  ODHIP_TRY(hipEventCreate(&a));
  if (hipEventCreate(&b) != hipSuccess) {
    (void)hipEventDestroy(a);
    return ODHIP_EFAULT;
  }
  const bool rec = p->record;
  p->record = false;
  rc = odhip_pipe_stage(p, stage, parity);
  (void)hipEventRecord(a, s);
  for (int i = 0; i < n && !rc; i++) rc = odhip_pipe_stage(p, stage, parity);
  (void)hipEventRecord(b, s);
  float ms = 0;
  if (!rc && (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess)) {
    rc = ODHIP_EFAULT;
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  p->record = rec;
  *avg_ms = ms/n;
  return rc;
}

/* Host milliseconds spent so far waiting for the margin counts (the only host waits
   of a step; everything else in odhip_pipe_step is launch work). */
extern "C" double odhip_pipe_host_wait_ms(const odhip_pipe *p) {
  return p ? p->wait_ms : 0;
}

extern "C" int odhip_pipe_set_test_hooks(odhip_pipe *p, double theta_margin, int theta_perturb,
 double price_tol_scale) {
  if (!p) return ODHIP_EINVAL;
  for (int i = 0; i < 2; i++) {
    const int rc = odhip_ctx_set_test_hooks(p->ctx[i], theta_margin, theta_perturb, price_tol_scale);
    if (rc) return rc;
  }
  return ODHIP_SUCCESS;
}

extern "C" long odhip_pipe_price_reruns(const odhip_pipe *p) {
  return p ? p->price_reruns : 0;
}

extern "C" long odhip_pipe_theta_reruns(const odhip_pipe *p) {
  return p ? p->reruns : 0;
}

/* Bands whose theta lay inside the margin of the device acos and were recomputed with the host's libm so far
   (odhip_pipe_theta_reruns counts the ones whose theta changed). */
extern "C" long odhip_pipe_theta_listed(odhip_pipe *p) {
  if (!p) return 0;
  long n = 0;
  for (int i = 0; i < 2; i++) {
    if (i == 0 && !p->cfg.inter) continue;      /* keyframes: only the chroma chain runs the with-reference stage */
    Current cur(p->ctx[i]);
    const long v = odhip_pvq_ref_theta_listed();
    if (v > 0) n += v;
  }
  return n;
}

/* ---- odhip_pipe_set_metrics .. 5: the metrics of every step (include/daala_hip.h) ---- */
namespace {

/* every odhip_pipe_set_metricsN: `last` is the newest column that entry point accepts */
int set_metrics(odhip_pipe *p, int flags, int depth, int last) {
  if (!p || (flags & ~metrics_mask(last)) || (flags && depth < 2)) return ODHIP_EINVAL;
  if (flags & ODHIP_METRIC_FASTSSIM) {
    /* a plane set the metric does not take: refused here, not inside a step */
    for (const PlaneSet &t : p->set) {
      int wl, hl;
      if (odhip_fastssim_level_size(t.pw, t.ph, 0, &wl, &hl)) return ODHIP_EINVAL;
    }
  }
  if (flags & ODHIP_METRIC_MSSSIM) {
    /* a plane set whose scale 4 is empty: refused here, not inside a step */
    for (const PlaneSet &t : p->set) {
      if (t.pw < ODHIP_MSSSIM_MIN_SIZE || t.ph < ODHIP_MSSSIM_MIN_SIZE) return ODHIP_EINVAL;
    }
  }
  if (flags & ODHIP_METRIC_SSIM) {
    /* a radius the tiling does not take: refused here, not inside a step */
    for (int i = 0; i < 2; i++) {
      std::vector<uint32_t> taps((size_t)2*ODHIP_SSIM_MAX_RADIUS + 3);
      const PlaneSet &t = p->set[i];
      const int size = odhip_ssim_taps(t.ph*(1.5/256), std::min(t.pw, t.ph), taps.data(), (int)taps.size());
      if (size < 0 || size > 2*ODHIP_SSIM_MAX_RADIUS + 1) return ODHIP_EIMPL;
    }
  }
  const int rc = odhip_pipe_sync(p);
  if (rc) return rc;
  ODHIP_TRY(hipSetDevice(p->cfg.device));
  /* the idle pipe drops what it measured: a late re-run of a step measured before this call measures nothing */
  p->met_flags = 0;
  p->met_step[0] = p->met_step[1] = -1;
  p->met_pending = -1;
  p->met_slots.clear();
  (void)p->met_dev.drop();
  (void)p->met_host.drop();
  p->met_n = 0;
  if (!flags) return ODHIP_SUCCESS;
  p->met_values = metrics_values(p);
  p->met_cols = 0;
  for (int c = 0; c < MET_NCOLS; c++) {
    const MetricColumn &col = kMetricColumns[c];
    if (!col.always && !(flags & col.bit)) continue;
    p->met_off[c] = (size_t)p->met_cols;
    p->met_cols += col.width;
  }
  const size_t n = metrics_bytes(p)*(size_t)depth;
  STEP_TRY(p->met_dev.alloc(n));
  ODHIP_TRY(hipMemset(p->met_dev.p, 0, n));
  STEP_TRY(p->met_host.alloc(n));
  memset(p->met_host.p, 0, n);
  STEP_TRY(p->met_slots.create(depth));
  for (int i = 0; i < 2; i++) STEP_TRY(pipe_event(p, &p->met_ev_luma[i]));
  if (flags & ODHIP_METRIC_CIEDE) STEP_TRY(pipe_event(p, &p->ev_ciede));
  /* the scratch of both chains' contexts now, not inside a step */
  for (int i = 0; i < 2; i++) {
    Current cur(p->ctx[i]);
    STEP_TRY(odhip_metrics_prepare());
    if (flags & ODHIP_METRIC_SSIM) {
      /* either chain may measure either plane set (an inter step's tail runs both on one) */
      long tiles = 1;
      for (const PlaneSet &t : p->set) {
        tiles = std::max(tiles, std::min(32L, (long)t.nlev*t.nplanes)*odhip_ssim_tile_count(t.pw, t.ph));
      }
      STEP_TRY(odhip_ssim_prepare(tiles));
    }
    if (flags & ODHIP_METRIC_MSSSIM) {
      for (const PlaneSet &t : p->set) STEP_TRY(odhip_msssim_prepare(t.pw, t.ph, t.nlev*t.nplanes));
    }
    if (flags & ODHIP_METRIC_FASTSSIM) {
      for (const PlaneSet &t : p->set) STEP_TRY(odhip_fastssim_prepare(t.pw, t.ph, t.nlev*t.nplanes));
    }
    if (flags & ODHIP_METRIC_CIEDE) STEP_TRY(odhip_ciede_prepare(p->set[0].pw, p->set[0].ph, 5*p->cfg.frames));
  }
  p->met_n = depth;
  p->met_flags = flags;
  return ODHIP_SUCCESS;
}

/* every odhip_pipe_metrics_takeN: out[c] receives column c where the slot has it; NULL skips one.
   1: the oldest complete step not taken yet - its number and values; its slot is free again.  0: none. */
int metrics_take(odhip_pipe *p, int wait, long *step, std::initializer_list<void *> out) {
  if (!p || !step || !p->met_flags) return ODHIP_EINVAL;
  long s = 0;
  size_t slot = 0;
  const int rc = p->met_slots.poll(wait != 0, &s, &slot);
  if (rc <= 0) return rc;
  int c = 0;
  for (void *dst : out) {
    const MetricColumn &col = kMetricColumns[c];
    const size_t entries = col.per_picture ? (size_t)5*p->cfg.frames : col.width*p->met_values;
    if (dst && (col.always || (p->met_flags & col.bit))) {
      memcpy(dst, metrics_col(p, p->met_host.p, slot, c), sizeof(int64_t)*entries);
    }
    c++;
  }
  *step = s;
  p->met_slots.taken = p->met_slots.released = s + 1;
  return 1;
}

}  // namespace

extern "C" int odhip_pipe_set_metrics(odhip_pipe *p, int flags, int depth) {
  return set_metrics(p, flags, depth, MET_HVS);
}

extern "C" int odhip_pipe_set_metrics2(odhip_pipe *p, int flags, int depth) {
  return set_metrics(p, flags, depth, MET_SSIM);
}

extern "C" int odhip_pipe_set_metrics3(odhip_pipe *p, int flags, int depth) {
  return set_metrics(p, flags, depth, MET_MSSSIM);
}

extern "C" int odhip_pipe_set_metrics4(odhip_pipe *p, int flags, int depth) {
  return set_metrics(p, flags, depth, MET_FASTSSIM);
}

extern "C" int odhip_pipe_set_metrics5(odhip_pipe *p, int flags, int depth) {
  return set_metrics(p, flags, depth, MET_CIEDE);
}

extern "C" int odhip_pipe_metrics_take(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs) {
  return metrics_take(p, wait, step, {sse, hvs});
}

extern "C" int odhip_pipe_metrics_take2(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs, double *ssim) {
  return metrics_take(p, wait, step, {sse, hvs, ssim});
}

extern "C" int odhip_pipe_metrics_take3(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs, double *ssim,
 double *msssim) {
  return metrics_take(p, wait, step, {sse, hvs, ssim, msssim});
}

extern "C" int odhip_pipe_metrics_take4(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs, double *ssim,
 double *msssim, double *fastssim) {
  return metrics_take(p, wait, step, {sse, hvs, ssim, msssim, fastssim});
}

extern "C" int odhip_pipe_metrics_take5(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs, double *ssim,
 double *msssim, double *fastssim, double *ciede) {
  return metrics_take(p, wait, step, {sse, hvs, ssim, msssim, fastssim, ciede});
}

extern "C" int odhip_pipe_metrics_ciede_values(const odhip_pipe *p) {
  return p ? 5*p->cfg.frames : ODHIP_EINVAL;
}

extern "C" int odhip_pipe_metrics_layout(const odhip_pipe *p, odhip_pipe_metrics_info *out) {
  if (!p || !out) return ODHIP_EINVAL;
  out->luma_levels = p->set[0].nlev;
  out->chroma_levels = p->set[1].nlev;
  out->luma_planes = p->set[0].nplanes;
  out->chroma_planes = p->set[1].nplanes;
  out->values = (int32_t)metrics_values(p);
  out->depth = p->met_depth;
  out->flags = p->met_flags;
  out->slots = p->met_n;
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_metrics_counts(const odhip_pipe *p, long npixels[2], long nwindows[2]) {
  if (!p || !npixels || !nwindows) return ODHIP_EINVAL;
  for (int si = 0; si < 2; si++) {
    npixels[si] = (long)p->set[si].pw*p->set[si].ph;
    nwindows[si] = odhip_psnrhvs_window_count(p->set[si].pw, p->set[si].ph, nullptr, nullptr);
  }
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_metrics_ssim_weights(const odhip_pipe *p, int64_t weight[2]) {
  if (!p || !weight) return ODHIP_EINVAL;
  for (int si = 0; si < 2; si++) {
    const int rc = odhip_ssim_weight(p->set[si].pw, p->set[si].ph, 1., &weight[si]);
    if (rc) return rc;
  }
  return ODHIP_SUCCESS;
}

extern "C" int odhip_pipe_metrics_msssim_weights(const odhip_pipe *p, int64_t weight[2][5]) {
  if (!p || !weight) return ODHIP_EINVAL;
  for (int si = 0; si < 2; si++) {
    const int rc = odhip_msssim_weights(p->set[si].pw, p->set[si].ph, weight[si]);
    if (rc) return rc;
  }
  return ODHIP_SUCCESS;
}
