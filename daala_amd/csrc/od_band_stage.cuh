/* od_band_stage.cuh - what the two PVQ band stages share around their search kernels:
   pvq_bands.hip (pvq_theta without a reference) and pvq_refbands.hip (with one).

   - ItemTable: the (job, band) work items of a multi-job launch, each with a
     prefix sum of workgroup counts; a workgroup finds its item by binary search.
   - the counting sort of each item's block indices by key, heavy first
     (k_sort_hist / k_sort_prefix / k_sort_scatter, BlockSort);
   - the per-context state both stages keep between calls: content-keyed device
     job tables, device buffers (od_buf.cuh), side streams, profiling events and
     pinned counters.  Every piece frees what it holds in its own destructor.
   - host helpers of both stages: the dispatch of a band size to a kernel template,
     the part of a job both stages fill alike, and the lists of bands the device
     leaves to the host (take_listed, upload_list).

   Included by both translation units; everything is in an anonymous namespace. */
#pragma once
#include <stdio.h>
#include <string.h>
#include <new>
#include <type_traits>
#include <vector>
#include "od_buf.cuh"
#include "od_ctx.cuh"
#include "gen/od_scan_tables.h"

namespace {

/* ---- work items ------------------------------------------------------------------ */
template <int MaxItems>
struct ItemTable {
  int nitems;
  int wg_start[MaxItems + 1];   /* first workgroup of each item; [nitems] = the grid */
  unsigned char job[MaxItems];
  unsigned char band[MaxItems];
};

template <int M>
__device__ __forceinline__ int find_item(const ItemTable<M> &t, int wg) {
  int lo = 0;
  int hi = t.nitems - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.wg_start[mid] <= wg) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

/* The (job, band) pair of an item as an index into per-item arrays such as the sort's. */
template <int M>
__device__ __forceinline__ int item_slot(const ItemTable<M> &t, int item) {
  return t.job[item]*ODHIP_MAX_BANDS + t.band[item];
}

template <int M>
void items_add(ItemTable<M> &t, int job, int band, long wgs) {
  if (wgs <= 0) return;
  t.job[t.nitems] = (unsigned char)job;
  t.band[t.nitems] = (unsigned char)band;
  t.wg_start[t.nitems + 1] = t.wg_start[t.nitems] + (int)wgs;
  t.nitems++;
}

/* Every (job, band) from band first_band on whose band has n coefficients (n = 0: every size), with
   per_wg blocks to a workgroup. */
template <int M, class Job>
void items_add_size(ItemTable<M> &t, const Job *host, int njobs, int n, long per_wg, int first_band = 0) {
  for (int j = 0; j < njobs; j++) {
    for (int b = first_band; b < host[j].nb_bands; b++) {
      if (n == 0 || host[j].off[b + 1] - host[j].off[b] == n) {
        items_add(t, j, b, (host[j].nblocks + per_wg - 1)/per_wg);
      }
    }
  }
}

/* Heaviest items first: the jobs arrive by ascending block size, and the bands of the largest
   blocks place the most pulses (K ~ 70 against 0-25 for the 128-coefficient luma bands) in the fewest
   wavefronts - launched last they were the tail of their kernel.  ODHIP_ITEMS_FWD=1 keeps the
   order of the jobs (experiments). */
template <int M>
void items_heavy_first(ItemTable<M> &t) {
  static const bool fwd = ODHIP_EXP_ENV("ODHIP_ITEMS_FWD") != nullptr;
  if (fwd) return;
  const int n = t.nitems;
  int size[M];
  for (int i = 0; i < n; i++) size[i] = t.wg_start[i + 1] - t.wg_start[i];
  for (int i = 0; i < n/2; i++) {
    const unsigned char j = t.job[i];
    const unsigned char b = t.band[i];
    const int z = size[i];
    t.job[i] = t.job[n - 1 - i];
    t.band[i] = t.band[n - 1 - i];
    size[i] = size[n - 1 - i];
    t.job[n - 1 - i] = j;
    t.band[n - 1 - i] = b;
    size[n - 1 - i] = z;
  }
  for (int i = 0; i < n; i++) t.wg_start[i + 1] = t.wg_start[i] + size[i];
}

/* ---- counting sort of each item's block indices by key (heavy first) ------------------
   Every (job, band) item's blocks carry a key of Bins classes (jb.keys[band*nblocks + blk], heavy =
   small); the sort writes the block indices in key order to jb.ids.  LDS histogram per chunk of
   blocks, one global atomic per non-empty bin per chunk.  The order inside a bin stays close to block
   order (workgroups reserve contiguous ranges per bin) but depends on atomics: the sort decides only
   which lanes take which bands, never a band's result.  The global arrays: the histogram (zero between
   calls) and the cursors, which k_sort_prefix sets to the exclusive prefix and k_sort_scatter
   advances. */
template <class Job, int M>
struct SortArgs {
  ItemTable<M> t;          /* chunks (hist, scatter) or one workgroup per item (prefix) */
  const Job *jobs;         /* the device job table                                  */
  unsigned *hist;          /* [M][Bins] histogram, then [M][Bins] cursors            */
};

template <int Bins, int Chunk, class Job, int M>
__global__ __launch_bounds__(256) void k_sort_hist(SortArgs<Job, M> a) {
  __shared__ unsigned h[Bins];
  const int item = find_item(a.t, blockIdx.x);
  const Job &jb = a.jobs[a.t.job[item]];
  const long nblocks = jb.nblocks;
  const unsigned short *keys = jb.keys + (long)a.t.band[item]*nblocks;
  for (int b = threadIdx.x; b < Bins; b += 256) h[b] = 0;
  __syncthreads();
  const long start = (long)(blockIdx.x - a.t.wg_start[item])*Chunk;
  const long end = start + Chunk < nblocks ? start + Chunk : nblocks;
  for (long i = start + threadIdx.x; i < end; i += 256) atomicAdd(&h[keys[i]], 1u);
  __syncthreads();
  unsigned *gh = a.hist + item_slot(a.t, item)*Bins;
  for (int b = threadIdx.x; b < Bins; b += 256) {
    if (h[b]) atomicAdd(&gh[b], h[b]);
  }
}

/* One workgroup per item: the cursors become the exclusive prefix sum of the histogram, which is
   cleared for the next call. */
template <int Bins, class Job, int M>
__global__ __launch_bounds__(256) void k_sort_prefix(SortArgs<Job, M> a) {
  constexpr int kPer = Bins/256;
  __shared__ unsigned part[256];
  const int slot = item_slot(a.t, blockIdx.x);
  unsigned *gh = a.hist + slot*Bins + threadIdx.x*kPer;
  unsigned *cursor = a.hist + (M + slot)*Bins + threadIdx.x*kPer;
  unsigned c[kPer];
  unsigned sum = 0;
  for (int i = 0; i < kPer; i++) {
    c[i] = gh[i];
    gh[i] = 0;
    sum += c[i];
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += t;
    __syncthreads();
  }
  unsigned run = part[threadIdx.x] - sum;
  for (int i = 0; i < kPer; i++) {
    cursor[i] = run;
    run += c[i];
  }
}

template <int Bins, int Chunk, class Job, int M>
__global__ __launch_bounds__(256) void k_sort_scatter(SortArgs<Job, M> a) {
  __shared__ unsigned h[Bins];
  const int item = find_item(a.t, blockIdx.x);
  const Job &jb = a.jobs[a.t.job[item]];
  const long nblocks = jb.nblocks;
  const unsigned short *keys = jb.keys + (long)a.t.band[item]*nblocks;
  unsigned *ids = jb.ids + (long)a.t.band[item]*nblocks;   /* read before the atomics: no reload after them */
  for (int b = threadIdx.x; b < Bins; b += 256) h[b] = 0;
  __syncthreads();
  const long start = (long)(blockIdx.x - a.t.wg_start[item])*Chunk;
  int key[Chunk/256];
  unsigned rank[Chunk/256];
#pragma unroll
  for (int t = 0; t < Chunk/256; t++) {
    const long i = start + t*256 + threadIdx.x;
    key[t] = -1;
    if (i < nblocks) {
      key[t] = keys[i];
      rank[t] = atomicAdd(&h[key[t]], 1u);
    }
  }
  __syncthreads();
  unsigned *cursor = a.hist + (M + item_slot(a.t, item))*Bins;
  for (int b = threadIdx.x; b < Bins; b += 256) {
    if (h[b]) h[b] = atomicAdd(&cursor[b], h[b]);
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < Chunk/256; t++) {
    if (key[t] >= 0) ids[h[key[t]] + rank[t]] = (unsigned)(start + t*256 + threadIdx.x);
  }
}

/* A context's sort: its global arrays and the key / sorted-index scratch of every (band, block) pair
   of a call, grown on demand. */
template <int Bins, int Chunk, class Job, int M>
struct BlockSort {
  static_assert(Bins % 256 == 0 && Chunk % 256 == 0, "the sort kernels run 256 threads");
  DeviceBuf<unsigned> arrays;     /* histogram + cursors                                */
  DeviceBuf<unsigned short> keys;
  DeviceBuf<unsigned> ids;
  bool dirty = false;             /* the histogram may hold counts of a failed call     */

  int alloc() {
    const int rc = arrays.alloc((size_t)2*M*Bins);
    if (rc) return rc;
    ODHIP_TRY(hipMemset(arrays.p, 0, sizeof(unsigned)*2*M*Bins));
    return ODHIP_SUCCESS;
  }

  /* Points every job's keys / ids at its part of the scratch. */
  int place(Job *host, int njobs, hipStream_t s) {
    size_t pairs = 0;
    for (int j = 0; j < njobs; j++) pairs += (size_t)host[j].nblocks*host[j].nb_bands;
    int rc = keys.grow(pairs, s);
    if (!rc) rc = ids.grow(pairs, s);
    if (rc) return rc;
    pairs = 0;
    for (int j = 0; j < njobs; j++) {
      host[j].keys = keys.p + pairs;
      host[j].ids = ids.p + pairs;
      pairs += (size_t)host[j].nblocks*host[j].nb_bands;
    }
    return ODHIP_SUCCESS;
  }

  /* Sorts every (job, band) of the call: host[] as uploaded to d_jobs. */
  int run(const Job *host, const Job *d_jobs, int njobs, hipStream_t s) {
    SortArgs<Job, M> chunks;
    SortArgs<Job, M> all;
    memset(&chunks, 0, sizeof(chunks));
    memset(&all, 0, sizeof(all));
    chunks.jobs = all.jobs = d_jobs;
    chunks.hist = all.hist = arrays.p;
    for (int j = 0; j < njobs; j++) {
      for (int b = 0; b < host[j].nb_bands; b++) {
        items_add(chunks.t, j, b, (host[j].nblocks + Chunk - 1)/Chunk);
        items_add(all.t, j, b, 1);
      }
    }
    /* the histogram is consumed and cleared by k_sort_prefix; only a call that failed between the two
       leaves it dirty */
    if (dirty) {
      ODHIP_TRY(hipMemsetAsync(arrays.p, 0, sizeof(unsigned)*M*Bins, s));
      dirty = false;
    }
    dirty = true;
    k_sort_hist<Bins, Chunk><<<chunks.t.wg_start[chunks.t.nitems], 256, 0, s>>>(chunks);
    k_sort_prefix<Bins><<<all.t.nitems, 256, 0, s>>>(all);
    dirty = odhip_check_launch() != ODHIP_SUCCESS;
    k_sort_scatter<Bins, Chunk><<<chunks.t.wg_start[chunks.t.nitems], 256, 0, s>>>(chunks);
    return ODHIP_SUCCESS;
  }
};

/* ---- per-context host state --------------------------------------------------------- */
/* Device job tables are CACHED by content: a caller that repeats its calls (a frame pipeline: the same
   jobs step after step) finds every table already resident and nothing is copied - a hipMemcpy from
   pageable host memory stalls the host until the stream has drained.  The content comparison (memcmp)
   is meaningful only because each stage's fill_job zeroes a host job with memset before filling it:
   padding bytes and unused fields compare equal. */
template <class Job, int MaxJobs>
struct JobTables {
  static constexpr int kSlots = 8;
  DeviceBuf<Job> d;               /* kSlots device tables of MaxJobs                    */
  Job host[kSlots][MaxJobs];
  int n[kSlots] = {};
  unsigned long stamp[kSlots] = {};
  unsigned long clock = 0;
  const Job *cur = nullptr;       /* the table of the call in progress                  */

  int alloc() { return d.alloc((size_t)kSlots*MaxJobs); }

  int upload(const Job *jobs, int njobs, hipStream_t s) {
    int lru = 0;
    for (int i = 0; i < kSlots; i++) {
      if (n[i] == njobs && memcmp(host[i], jobs, sizeof(Job)*njobs) == 0) {
        stamp[i] = ++clock;
        cur = d.p + (size_t)i*MaxJobs;
        return ODHIP_SUCCESS;
      }
      if (stamp[i] < stamp[lru]) lru = i;
    }
    /* miss: the least recently used slot is rewritten once nothing in flight on the caller's stream
       (side streams are joined into it at the end of every call) can still read it */
    if (n[lru]) ODHIP_TRY(hipStreamSynchronize(s));
    memcpy(host[lru], jobs, sizeof(Job)*njobs);
    n[lru] = njobs;
    stamp[lru] = ++clock;
    Job *dst = d.p + (size_t)lru*MaxJobs;
    ODHIP_TRY(hipMemcpy(dst, jobs, sizeof(Job)*njobs, hipMemcpyHostToDevice));
    cur = dst;
    return ODHIP_SUCCESS;
  }
};

/* Two side streams for kernels that may overlap (created on first use). */
struct SideStreams : NoCopy {
  bool serial = false;            /* the context's setting, refreshed per call          */
  hipStream_t side[2] = {nullptr, nullptr};
  hipEvent_t fork_ev = nullptr;
  hipEvent_t join_ev[2] = {nullptr, nullptr};
  ~SideStreams() {
    for (int i = 0; i < 2; i++) {
      if (side[i]) (void)hipStreamDestroy(side[i]);
      if (join_ev[i]) (void)hipEventDestroy(join_ev[i]);
    }
    if (fork_ev) (void)hipEventDestroy(fork_ev);
  }
  /* out[] = the side streams, ordered after the work queued on s so far; left as they are (s) when the
     context or ODHIP_PVQ_SERIAL asks for serial execution */
  int fork(hipStream_t s, hipStream_t out[2]) {
    if (serial || odhip_env_serial()) return ODHIP_SUCCESS;
    if (!fork_ev) {
      ODHIP_TRY(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
      for (int i = 0; i < 2; i++) {
        ODHIP_TRY(hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
        ODHIP_TRY(hipEventCreateWithFlags(&join_ev[i], hipEventDisableTiming));
      }
    }
    ODHIP_TRY(hipEventRecord(fork_ev, s));
    for (int i = 0; i < 2; i++) {
      ODHIP_TRY(hipStreamWaitEvent(side[i], fork_ev, 0));
      out[i] = side[i];
    }
    return ODHIP_SUCCESS;
  }
  int join(hipStream_t s, const hipStream_t out[2]) {
    for (int i = 0; i < 2; i++) {
      if (out[i] == s) continue;
      ODHIP_TRY(hipEventRecord(join_ev[i], out[i]));
      ODHIP_TRY(hipStreamWaitEvent(s, join_ev[i], 0));
    }
    return ODHIP_SUCCESS;
  }
};

/* Profiling aid (odhip_pvq_profile, odhip_pvq_ref_profile): HIP events around the dominant kernel of a
   stage, on the stream it is launched on. */
struct ProfEvents : NoCopy {
  static constexpr int kSlots = 256;
  bool on = false;
  bool made = false;
  int n = 0;
  hipEvent_t ev[kSlots][2];
  ~ProfEvents() {
    if (!made) return;
    for (int i = 0; i < kSlots; i++) {
      (void)hipEventDestroy(ev[i][0]);
      (void)hipEventDestroy(ev[i][1]);
    }
  }
  int enable(int e) {
    if (e && !made) {
      for (int i = 0; i < kSlots; i++) {
        ODHIP_TRY(hipEventCreate(&ev[i][0]));
        ODHIP_TRY(hipEventCreate(&ev[i][1]));
      }
      made = true;
    }
    on = e != 0;
    n = 0;
    return ODHIP_SUCCESS;
  }
  /* the times recorded since the last read, in ms; returns how many */
  int read(float *ms, int max_n) {
    int i = 0;
    for (; i < n && i < max_n; i++) {
      ODHIP_TRY(hipEventSynchronize(ev[i][1]));
      ODHIP_TRY(hipEventElapsedTime(&ms[i], ev[i][0], ev[i][1]));
    }
    n = 0;
    return i;
  }
  /* launch() between a pair of events when profiling is on */
  template <class F>
  void around(hipStream_t s, F &&launch) {
    const bool rec = on && n < kSlots;
    if (rec) (void)hipEventRecord(ev[n][0], s);
    launch();
    if (rec) (void)hipEventRecord(ev[n++][1], s);
  }
};

/* A device counter's value on its way to pinned host memory behind the kernels that count, so that the
   caller later waits for the count alone rather than for the whole stream. */
struct PinnedCount : NoCopy {
  PinnedBuf<unsigned> host;
  hipEvent_t ev = nullptr;
  ~PinnedCount() {
    if (ev) (void)hipEventDestroy(ev);
  }
  int post(const unsigned *d_count, hipStream_t s) {
    if (!host.p) {
      const int rc = host.alloc(1);
      if (rc) return rc;
      ODHIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    *host.p = 0xffffffffu;
    ODHIP_TRY(hipMemcpyAsync(host.p, d_count, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    ODHIP_TRY(hipEventRecord(ev, s));
    return ODHIP_SUCCESS;
  }
  /* 1 when the count posted last is nonzero, 0 when it is zero; ODHIP_EINVAL when nothing was posted */
  int wait() {
    if (!ev) return ODHIP_EINVAL;
    ODHIP_TRY(hipEventSynchronize(ev));
    return *host.p != 0;
  }
};

/* A stage's device counters, zero at first.  Read-and-clear with blocking copies: the stream that counts
   must have been synchronised. */
template <int N>
struct Counters {
  DeviceBuf<unsigned> d;
  int alloc() {
    const int rc = d.alloc(N);
    if (rc) return rc;
    ODHIP_TRY(hipMemset(d.p, 0, N*sizeof(unsigned)));
    return ODHIP_SUCCESS;
  }
  int take(int i, unsigned *count) {
    unsigned v = 0;
    ODHIP_TRY(hipMemcpy(&v, d.p + i, sizeof(v), hipMemcpyDeviceToHost));
    if (v) ODHIP_TRY(hipMemset(d.p + i, 0, sizeof(v)));
    *count = v;
    return ODHIP_SUCCESS;
  }
};

/* ---- host helpers of both stages ------------------------------------------------------ */
/* A stage's state of the calling thread's current context as `State &st`, or the getter's code returned. */
#define STAGE_STATE_OR_RETURN(State, getter, st) \
  State *st##_p; \
  { \
    const int rc0_ = getter(&st##_p); \
    if (rc0_) return rc0_; \
  } \
  State &st = *st##_p

/* The band sizes of every block size, and f(std::integral_constant<int, n>) for one of them: a generic
   lambda launches the kernel template of that size.  A call site whose kernels exist for fewer sizes
   restricts itself with `if constexpr`. */
constexpr int kBandSizes[4] = {128, 32, 15, 8};

template <class F>
int for_band_size(int n, F &&f) {
  switch (n) {
    case 128: f(std::integral_constant<int, 128>()); return ODHIP_SUCCESS;
    case 32: f(std::integral_constant<int, 32>()); return ODHIP_SUCCESS;
    case 15: f(std::integral_constant<int, 15>()); return ODHIP_SUCCESS;
    case 8: f(std::integral_constant<int, 8>()); return ODHIP_SUCCESS;
    default: return ODHIP_EINVAL;
  }
}

/* What a stage's fill_job prepares a job for, and so which of its buffers it insists on. */
enum JobMode {
  kJobBands,    /* the band stage: forward QM, work vectors, 16-byte aligned planes */
  kJobSynth,    /* choice + synthesis: inverse QM, choices, the output planes       */
  kJobChoice    /* choice only                                                      */
};

/* The part of a job both stages fill alike, into a zeroed d: geometry, band offsets, q / q2 / beta, the
   plane split, per-plane quantiser rows.  cap_blocks: block indices must fit 32 bits. */
template <class Job, class In>
int fill_geometry(Job &d, const In &j, bool cap_blocks) {
  if (!j.q_band || !j.beta_band || j.bs < 0 || j.bs >= ODHIP_NBSIZES || j.nplanes <= 0) return ODHIP_EINVAL;
  const int n = 4 << j.bs;
  if (j.w <= 0 || j.h <= 0 || j.w % n || j.h % n) return ODHIP_EINVAL;
  d.nplanes = j.nplanes;
  d.w = j.w;
  d.h = j.h;
  d.bs = j.bs;
  d.bw = j.w/n;
  d.bh = j.h/n;
  d.nblocks = (long)j.nplanes*d.bw*d.bh;
  if (cap_blocks && d.nblocks > 0xffffffffL) return ODHIP_EINVAL;
  d.nb_bands = OD_NBANDS[j.bs];
  d.len = n*n < OD_SCAN_LEN ? n*n : OD_SCAN_LEN;
  for (int i = 0; i <= d.nb_bands; i++) d.off[i] = OD_BAND_OFFS[j.bs][i];
  for (int i = 0; i < d.nb_bands; i++) {
    d.q[i] = j.q_band[i];
    d.q2[i] = j.q_band2 ? j.q_band2[i] : j.q_band[i];
    if (d.q[i] < 1 || d.q2[i] < 1) return ODHIP_EINVAL;
    d.beta[i] = j.beta_band[i];
  }
  d.split_blk = d.nblocks;
  if (j.q_band2) {
    if (j.plane_split <= 0 || j.plane_split >= j.nplanes) return ODHIP_EINVAL;
    d.split_blk = (long)j.plane_split*d.bw*d.bh;
  }
  d.qp = j.d_q_plane;
  d.plane_blocks = (unsigned)(d.bw*d.bh);
  if (d.qp) {
    for (int i = 0; i < d.nb_bands; i++) d.q[i] = d.q2[i] = 0;
  }
  return ODHIP_SUCCESS;
}

/* The bands a stage's kernels left to the host: counted at d_count, listed at d_list [cap].  Waits for
   the stream; returns how many (0: none, the normal case) with the list in `list`, or a negative code.
   *seen, when given, is the count even where it exceeds the list. */
template <class T>
int take_listed(hipStream_t s, const unsigned *d_count, const T *d_list, int cap, const char *what,
 std::vector<T> &list, unsigned *seen = nullptr) {
  ODHIP_TRY(hipStreamSynchronize(s));
  unsigned count = 0;
  ODHIP_TRY(hipMemcpy(&count, d_count, sizeof(count), hipMemcpyDeviceToHost));
  if (seen) *seen = count;
  if (count == 0) return 0;
  if (count > (unsigned)cap) {
    fprintf(stderr, "libdaalahip: %u %s exceed the list (%d)\n", count, what, cap);
    return ODHIP_EFAULT;
  }
  try {
    list.resize(count);
  }
  catch (const std::bad_alloc &) {
    return ODHIP_EFAULT;
  }
  if (hipMemcpy(list.data(), d_list, sizeof(T)*count, hipMemcpyDeviceToHost) != hipSuccess) return ODHIP_EFAULT;
  return (int)count;
}

/* Every listed band names one of the call's jobs. */
template <class T>
bool listed_jobs_valid(const T *list, unsigned n, int njobs) {
  for (unsigned i = 0; i < n; i++) {
    if (list[i].job < 0 || list[i].job >= njobs) return false;
  }
  return true;
}

/* The first n entries of a host list in a device buffer of the caller's scope, which frees it on every
   path; the copy is queued on *async or, without one, blocking. */
template <class T>
int upload_list(DeviceBuf<T> &d, const T *list, unsigned n, const hipStream_t *async = nullptr) {
  if (d.alloc(n)) return ODHIP_EFAULT;
  const hipError_t e = async ? hipMemcpyAsync(d.p, list, sizeof(T)*n, hipMemcpyHostToDevice, *async)
   : hipMemcpy(d.p, list, sizeof(T)*n, hipMemcpyHostToDevice);
  return e == hipSuccess ? ODHIP_SUCCESS : ODHIP_EFAULT;
}

}  // namespace
