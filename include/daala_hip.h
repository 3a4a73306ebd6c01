/* daala_hip.h - C ABI of libdaalahip.so: the MI355X (gfx950) implementation of
   Daala's block-transform encode hot path (lapped pre/post filter, 4..64 point
   integer DCT/iDCT, PVQ band search), as a drop-in for the reference's own
   surfaces for that path.

   Plain C: pointers, sizes and ints only.  Two families of entry points:

   (1) PER-CALL, HOST-POINTER functions with exactly the reference's
       signatures and conventions (synchronous, caller-owned host buffers, void
       return).  These are what the reference's function-pointer tables / call
       sites bind.  One small block per call is
       dominated by launch + PCIe latency; they exist for parity and for
       drop-in completeness, not for throughput.

   (2) BATCHED, DEVICE-POINTER functions (prefix odhip_) that the per-call
       ones are built on and that a batched caller (bench.py, the frame-sharded
       driver) uses directly: inputs already resident in HBM, asynchronous on a
       caller-supplied HIP stream, int return (0 or a negative OD_E* value as
       in the reference's include/daala/codec.h:89-103).

   All coefficient data is od_coeff = int32_t (reference src/filter.h:29) at
   scale 2^4 (OD_COEFF_SHIFT, src/internal.h:124).  Results are bit-exact with
   the reference C path; the CPU checker lives in oracle/ (tests only). */
#ifndef DAALA_HIP_H
#define DAALA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t od_coeff;

#define ODHIP_SUCCESS (0)
#define ODHIP_EFAULT (-1)   /* OD_EFAULT: HIP runtime failure / bad pointer */
#define ODHIP_EINVAL (-10)  /* OD_EINVAL: bad argument */
#define ODHIP_EIMPL (-23)   /* OD_EIMPL: not implemented */
#define ODHIP_ERANGE (-24)  /* a band needs more pulses than ODHIP_PVQ_MAX_K: odhip_pvq_k_range_take */
#define ODHIP_EBUSY (-101)  /* the export ring slot of the next step is still held (odhip_pipe_export_release);
                               outside the reference's OD_E* range */

#define ODHIP_NBSIZES 5     /* OD_NBSIZES: 4,8,16,32,64 (src/internal.h:53-59) */

/* A HIP stream as an opaque pointer (hipStream_t); NULL = the default stream. */
typedef void *odhip_stream;

/* ------------------------------------------------------------------------ */
/* (1) Per-call surfaces                                                     */
/* ------------------------------------------------------------------------ */

/* od_dct_func_2d, reference src/dct.h:61-62:
     void f(od_coeff *out, int out_stride, const od_coeff *in, int in_stride)
   Strides in elements.  Replace OD_FDCT_2D_C / OD_IDCT_2D_C
   (src/dct.c:54-68), i.e. od_bin_fdctNxN / od_bin_idctNxN (src/dct.c:151-163,
   351-363, 792-806, 4890-4920), in od_state_opt_vtbl.fdct_2d[] / idct_2d[]
   (src/state.h:128-129).  Called from src/encode.c:1304,1308,1397,1410,1449,
   1477 and src/decode.c:521,596.  Arbitrary od_coeff input: exact 32-bit
   products like the C. */
typedef void (*odhip_dct_func_2d)(od_coeff *out, int out_stride,
 const od_coeff *in, int in_stride);

void od_bin_fdct4x4_hip(od_coeff *y, int ystride, const od_coeff *x, int xstride);
void od_bin_idct4x4_hip(od_coeff *x, int xstride, const od_coeff *y, int ystride);
void od_bin_fdct8x8_hip(od_coeff *y, int ystride, const od_coeff *x, int xstride);
void od_bin_idct8x8_hip(od_coeff *x, int xstride, const od_coeff *y, int ystride);
void od_bin_fdct16x16_hip(od_coeff *y, int ystride, const od_coeff *x, int xstride);
void od_bin_idct16x16_hip(od_coeff *x, int xstride, const od_coeff *y, int ystride);
void od_bin_fdct32x32_hip(od_coeff *y, int ystride, const od_coeff *x, int xstride);
void od_bin_idct32x32_hip(od_coeff *x, int xstride, const od_coeff *y, int ystride);
void od_bin_fdct64x64_hip(od_coeff *y, int ystride, const od_coeff *x, int xstride);
void od_bin_idct64x64_hip(od_coeff *x, int xstride, const od_coeff *y, int ystride);

/* Installer with the shape of od_state_opt_vtbl_init_x86
   (src/x86/x86state.c:39-97): overwrites the five fdct_2d and five idct_2d
   slots of a table pair.  The one line of reference glue is
     odhip_install_dct_vtbl(state->opt_vtbl.fdct_2d, state->opt_vtbl.idct_2d);
   after od_state_opt_vtbl_init_c (src/state.c:346-352). */
void odhip_install_dct_vtbl(odhip_dct_func_2d fdct_2d[ODHIP_NBSIZES],
 odhip_dct_func_2d idct_2d[ODHIP_NBSIZES]);

/* od_filter_func, reference src/filter.h:43 (OD_PRE_FILTER[0] /
   OD_POST_FILTER[0] = od_pre_filter4 / od_post_filter4, src/filter.c:147-222):
   four samples, in place allowed. */
void od_pre_filter4_hip(od_coeff y[4], const od_coeff x[4]);
void od_post_filter4_hip(od_coeff x[4], const od_coeff y[4]);
/* The larger lapping filters of the same tables, od_pre_filter8/16/32 and
   od_post_filter8/16/32 (src/filter.c:279-1321, the TYPE3 parameter sets its
   `#elif 1` chains select).  The codec does not use them (OD_FILT_SIZE == 0,
   src/filter.h:77); the reference's own tests do (dcttest dynamic_range,
   src/dct.c:8606; the filter test).  odhip_install_filter_tables fills
   OD_PRE_FILTER[0..3] / OD_POST_FILTER[0..3]-shaped arrays (src/filter.c:115-127)
   with the host-pointer functions; odhip_filter_batch runs `count` independent
   (4 << f)-tap filters on contiguous device vectors [count][4 << f] (16-byte
   aligned; in place allowed), f = 0..3, inverse = 0 pre / 1 post. */
typedef void (*odhip_filter_func)(od_coeff out[], const od_coeff in[]);   /* od_filter_func, src/filter.h:43 */
void od_pre_filter8_hip(od_coeff y[8], const od_coeff x[8]);
void od_post_filter8_hip(od_coeff x[8], const od_coeff y[8]);
void od_pre_filter16_hip(od_coeff y[16], const od_coeff x[16]);
void od_post_filter16_hip(od_coeff x[16], const od_coeff y[16]);
void od_pre_filter32_hip(od_coeff y[32], const od_coeff x[32]);
void od_post_filter32_hip(od_coeff x[32], const od_coeff y[32]);
void odhip_install_filter_tables(odhip_filter_func pre[4], odhip_filter_func post[4]);
int odhip_filter_batch(int f, int inverse, od_coeff *d_out, const od_coeff *d_in, long count,
 odhip_stream stream);

/* Block- and frame-level lapping drivers, same signatures as the reference
   (src/filter.h:80-87; definitions src/filter.c:1459-1619), in place on a host
   plane.  `f` must be 0 (OD_FILT_SIZE is identically 0, src/filter.h:77); q,
   skip, skip_stride are unused exactly as in the reference's non-deblocking
   build.  Link-time replacements for the calls at src/encode.c:1489,1760,1789,
   2571,2675 and src/decode.c:807,823,962,994. */
void od_prefilter_split_hip(od_coeff *c0, int stride, int bs, int f,
 int hfilter, int vfilter);
void od_postfilter_split_hip(od_coeff *c0, int stride, int bs, int f, int q,
 unsigned char *skip, int skip_stride, int hfilter, int vfilter);
void od_apply_prefilter_frame_sbs_hip(od_coeff *c, int stride, int nhsb,
 int nvsb, int xdec, int ydec);
void od_apply_postfilter_frame_sbs_hip(od_coeff *c, int stride, int nhsb,
 int nvsb, int xdec, int ydec, int q, unsigned char *skip, int skip_stride);

/* pvq_search_rdo_double, reference src/pvq_encoder.c:93-224 (file-static
   there; BASELINE.json calls it od_pvq_search_rdo_double).  Same arguments and
   return value: xcoeff[n] int16 (od_val16), ypulse[n] in/out (input only when
   prev_k > 0), returns the cosine distance.  Called from pvq_theta,
   src/pvq_encoder.c:542,589. */
double od_pvq_search_rdo_double_hip(const int16_t *xcoeff, int n, int k,
 od_coeff *ypulse, double g2, double pvq_norm_lambda, int prev_k);
/* od_pvq_synthesis_partial, src/pvq.h:164 (src/pvq.c:1037-1115): the synthesis of one decoded / chosen band -
   what od_pvq_decode's pvq_decode_partition (src/pvq_decoder.c:77-89) and pvq_theta (src/pvq_encoder.c:631) call. */
void od_pvq_synthesis_partial_hip(od_coeff *xcoeff, const od_coeff *ypulse, const int16_t *r16, int n, int noref,
 int32_t g, int32_t theta, int m, int s, const int16_t *qm_inv);

/* ------------------------------------------------------------------------ */
/* (2) Batched device-pointer API                                            */
/* ------------------------------------------------------------------------ */

/* Library / device bring-up.  odhip_init selects the HIP device for the
   calling thread and returns 0, or ODHIP_EFAULT when no gfx950 device is
   usable (there is NO CPU fallback in this library). */
int odhip_init(int device);
const char *odhip_version(void);

/* Contexts (shaped after the reference's per-od_state backend
   installation, src/x86/x86state.c:39-97: nothing is process-global).  Every
   piece of state the batched entry points keep between calls - edge strips of
   the inverse stage, scratch / job tables / side streams / sort arrays /
   profiling events of the two PVQ band stages, the list of bands inside the
   device-acos margin - is owned by an odhip_ctx.  The batched odhip_* functions
   below use the CURRENT context of the calling thread: the one passed to
   odhip_make_current, or (NULL / never called) a default context the thread gets
   for the HIP device that is current when it calls in.  Rules:
     - one call sequence in flight per context (calls of a context are ordered on
       the caller's stream; scratch is reused from call to call);
     - sequences that overlap - two streams, e.g. the luma and the chroma chain of
       a frame batch, or two host threads, or two devices - use one context each;
     - a context belongs to the device it was created for; calling with another
       current device returns ODHIP_EINVAL.
   odhip_create returns NULL when the device does not exist; odhip_destroy waits
   for the device to go idle, then frees everything the context owns. */
typedef struct odhip_ctx odhip_ctx;
odhip_ctx *odhip_create(int device);
void odhip_destroy(odhip_ctx *ctx);
int odhip_make_current(odhip_ctx *ctx);    /* also makes ctx's device current */
odhip_ctx *odhip_get_current(void);        /* NULL = the thread's default context */
int odhip_ctx_device(const odhip_ctx *ctx);
/* serial != 0: the band stages of this context launch everything on the caller's
   stream instead of forking independent kernels onto the context's side streams
   (exclusive kernel durations for profiling; ODHIP_PVQ_SERIAL=1 does the same for
   every context). */
int odhip_ctx_set_serial(odhip_ctx *ctx, int serial);

/* ---- quantiser set-up (host) ----------------------------

   What the reference derives on the host per encoder / per frame and the band
   stages take as plain data:
     odhip_init_qm        od_init_qm, src/pvq.c:322-381 (same arguments: x, x_inv
                          of ODHIP_QM_BUFFER_SIZE int16, qm = an 8x8 Q4 matrix):
                          per-coefficient QM with magnitude compensation (Q11) and
                          its inverse (Q12) in coding order, for every block size
                          and both decimations; block (bs, xydec) starts at
                          odhip_qm_offset(bs, xydec) (od_qm_offset, src/pvq.c:306).
                          Entries the reference leaves unwritten (32x32 / 64x64
                          blocks have coding positions for 512 coefficients only)
                          are zero here.
     odhip_interp_qm      od_interp_qm as the frame header code selects its
                          entries per plane (src/encode.c:2903-2940, :3052-3072)
                          from the encoder's default matrices: pvq_qm_q4 of plane
                          pli for rc.base_quantizer.
     odhip_qm_get_index   od_qm_get_index, src/pvq.c:408-413.
     odhip_quant_setup    both of the above into one odhip_quant: quantizer =
                          od_state.quantizer (0 = lossless), base_quantizer =
                          rc.base_quantizer, hvs_qm = OD_SET_QM (1 = HVS, the
                          encoder's default), use_masking = OD_SET_ACTIVITY_MASKING.
     odhip_quant_bands    per band of block size bs in plane pli: the step
                          max(1, q0*pvq_qm_q4[index(bs, i + 1)] >> 4) with q0 =
                          max(1, quantizer) (src/pvq_encoder.c:874,
                          src/encode.c:1336) and OD_PVQ_BETA[masking][pli][bs][i]
                          (Q12, src/pvq.c:243-268); returns the number of bands. */
#define ODHIP_QM_SIZE 30              /* OD_QM_SIZE, src/pvq.h:108 */
#define ODHIP_QM_BUFFER_SIZE 10912    /* OD_QM_BUFFER_SIZE, src/pvq.h:72-74 */
typedef struct {
  int quantizer;
  int base_quantizer;
  int use_masking;
  int hvs_qm;
  uint8_t pvq_qm_q4[3][ODHIP_QM_SIZE];
  int16_t qm[ODHIP_QM_BUFFER_SIZE];
  int16_t qm_inv[ODHIP_QM_BUFFER_SIZE];
} odhip_quant;
void odhip_init_qm(int16_t *x, int16_t *x_inv, const int *qm);
int odhip_qm_offset(int bs, int xydec);
int odhip_qm_get_index(int bs, int band);
int odhip_interp_qm(uint8_t out[ODHIP_QM_SIZE], int base_quantizer, int use_masking, int pli);
int odhip_quant_setup(odhip_quant *qt, int base_quantizer, int quantizer, int use_masking,
 int hvs_qm);
int odhip_quant_bands(const odhip_quant *qt, int pli, int bs, int32_t *q_band, int32_t *beta_band);

/* nblocks contiguous N x N tiles, N = 4 << ln; d_out may equal d_in; both 16-byte
   aligned (ODHIP_EINVAL otherwise: the kernels move 16-byte vectors).
   exact32 != 0 forces exact 32-bit products (arbitrary input); 0 uses the
   24-bit multiplier, valid while |intermediate| < 2^23 (always true for data
   that came from pixels). */
int odhip_fdct2d_batch(int ln, od_coeff *d_out, const od_coeff *d_in,
 long nblocks, int exact32, odhip_stream stream);
int odhip_idct2d_batch(int ln, od_coeff *d_out, const od_coeff *d_in,
 long nblocks, int exact32, odhip_stream stream);

/* Every N x N block of a w x h plane (w, h multiples of N; pointers 16-byte
   aligned, strides multiples of 4 and at least w - ODHIP_EINVAL otherwise; the
   two strides need not be equal), strides in
   elements: the `d` plane layout of the reference encoder (block (bx,by)'s
   coefficient (v,u) at [(by*N+v)*stride + bx*N+u]). */
int odhip_fdct2d_plane(int ln, od_coeff *d_out, int out_stride,
 const od_coeff *d_in, int in_stride, int w, int h, int exact32,
 odhip_stream stream);
int odhip_idct2d_plane(int ln, od_coeff *d_out, int out_stride,
 const od_coeff *d_in, int in_stride, int w, int h, int exact32,
 odhip_stream stream);

/* PICTURE PLANE LAYOUT - the `d_px, px_stride, px_plane_stride` arguments of
   odhip_forward_pyramid, odhip_inverse_level(s), odhip_inverse_level(s)_pvq,
   odhip_inverse_levels_pvq_ref, odhip_inverse_partition and odhip_forward_partition.  Sample (x, y) of plane p is at
   d_px[p*px_plane_stride + y*px_stride + x], counted in samples (bytes, or the int16
   samples of a full-precision context, below).  A caller may pass its own frame strides
   as long as
     px_stride >= w                       rows do not overlap
     px_plane_stride >= px_stride*h       planes do not overlap (also when nplanes == 1)
     px_stride % 4 == 0, px_plane_stride % 4 == 0
     d_px aligned to 4 bytes, to 8 bytes in a full-precision context
   (the kernels read and write groups of four samples).  Anything else is ODHIP_EINVAL,
   returned before anything is launched or allocated.  Nothing outside the w x h windows
   is read or written: the gaps behind rows and between planes are the caller's.
   When base, px_stride and px_plane_stride are all multiples of 16 the 8-bit inverse
   stores whole 16-byte pieces (faster); the results are the same.
   The pulse-fed inverses keep their own rule on top: the y, choice, qm_inv (and r16)
   buffers of their jobs are 16-byte aligned.

   Forward lapped-transform pyramid of a batch of planes: for each plane
     od_ref_plane_to_coeff            (src/state.c:1216-1277)
     od_apply_prefilter_frame_sbs     (src/filter.c:1529-1559)
     for bs = top .. 0:  fdct_2d[bs] of every block, then od_prefilter_split
                         of every block   (src/encode.c:1455-1512 forced to
                                           split everywhere)
   d_px:  nplanes planes of w x h 8-bit pixels, plane p at d_px + p*px_plane_stride,
          row stride px_stride (layout rules above).
   d_levels[bs] (bs = 0..4-dec): nplanes coefficient planes of w x h, plane p at
          + p*(long)w*h, row stride w.  NULL skips the store of that level.
   dec:   0 for luma (64x64 superblocks), 1 for 4:2:0 chroma (32x32).
   pic_w, pic_h: UNPADDED LUMA picture size; gates the split filters exactly
          like src/encode.c:1487-1488.  w, h: multiples of 64 >> dec. */
int odhip_forward_pyramid(od_coeff *const d_levels[ODHIP_NBSIZES],
 const uint8_t *d_px, int px_stride, long px_plane_stride, int nplanes, int w,
 int h, int dec, int pic_w, int pic_h, odhip_stream stream);

/* Inverse at a uniform partition level leaf_bs for a batch of planes:
   idct_2d[leaf_bs] of every block, od_postfilter_split for levels
   leaf_bs+1 .. top (src/encode.c:1780-1789), od_apply_postfilter_frame_sbs
   (src/filter.c:1589-1618), od_coeff_to_ref_plane (src/state.c:1281-1345).
   d_coef: nplanes planes w x h, row stride w.  d_px as above (output; layout rules above). */
int odhip_inverse_level(uint8_t *d_px, int px_stride, long px_plane_stride,
 const od_coeff *d_coef, int nplanes, int w, int h, int dec, int leaf_bs,
 int pic_w, int pic_h, odhip_stream stream);

/* odhip_inverse_level for several partition levels of ONE plane set (same
   nplanes, w, h, dec; at most 5) in a single set of launches: level leaf_bs[i]
   is reconstructed from d_coef[i] into d_px[i] (distinct buffers, same strides). */
int odhip_inverse_levels(uint8_t *const *d_px, int px_stride, long px_plane_stride,
 const od_coeff *const *d_coef, const int *leaf_bs, int nlevels, int nplanes, int w, int h,
 int dec, int pic_w, int pic_h, odhip_stream stream);

/* Inverse at an ARBITRARY partition: the decoder's reconstruction of nplanes planes
   from their dequantised coefficient planes (d_coef, layout as above) and the
   block-size map of their frames: idct_2d of every leaf block, od_postfilter_split of
   every split node (od_decode_recursive, src/decode.c:603-660; the encoder's final pass
   src/encode.c:1657-1810 is the same), od_apply_postfilter_frame_sbs, od_coeff_to_ref_plane.
   d_bsize: od_state.bsize (src/state.h:250-259) - one byte per 8x8 LUMA area, 0 = four
   4x4 blocks ... 4 = one 64x64 block, rows of bstride bytes, origin at the frame's
   first superblock (the reference's pointer already skips its one-superblock border);
   plane p uses the map at d_bsize + (p / planes_per_frame)*bsize_frame_stride (luma:
   planes_per_frame = 1; 4:2:0 chroma with Cb and Cr of a frame adjacent: 2).  dec = 1
   derives the chroma blocks (one size down, 4x4 for 8x8 and 4x4 luma).  d_px: picture
   plane layout rules above; d_coef 16-byte aligned, bstride >= 8*(w / (64 >> dec)). */
int odhip_inverse_partition(uint8_t *d_px, int px_stride, long px_plane_stride,
 const od_coeff *d_coef, int nplanes, int w, int h, int dec, const uint8_t *d_bsize, int bstride,
 long bsize_frame_stride, int planes_per_frame, int pic_w, int pic_h, odhip_stream stream);
/* What a call of the inverse (odhip_inverse_level(s), their pulse-fed forms) would launch
   for one level of a plane set w samples wide - host arithmetic only, nothing is launched or
   allocated; for tests and tools that must know which kernel a case reached.
   src: 0 coefficient planes, 1 odhip_inverse_level(s)_pvq, 2 odhip_inverse_levels_pvq_ref,
   3 odhip_inverse_partition.  px_aligned16: pixel base, px_stride and px_plane_stride are
   all multiples of 16.
   *route: ODHIP_ROUTE_*; *nedges: the vertical superblock edges of a row that go through
   the strip buffers and the edge kernel (the joints between the walkers' segments, the edge
   between pairs, or every edge).  Returns 1 when the walkers store whole 16-byte pieces
   (8-bit context and px_aligned16), 0 when they store 4-sample groups, ODHIP_EINVAL for
   arguments the inverse itself refuses. */
enum {
  ODHIP_ROUTE_WALK_HI = 0,   /* walking workgroups, 32x32 leaves of 4:2:0 chroma */
  ODHIP_ROUTE_TOP2 = 1,      /* one workgroup per superblock pair: pulse-fed 32x32 / 64x64 luma */
  ODHIP_ROUTE_SB_TOP = 2,    /* one workgroup per superblock, 32x32 / 64x64 luma */
  ODHIP_ROUTE_SB_REF = 3,    /* one workgroup per superblock, with-reference source */
  ODHIP_ROUTE_SB_ALL = 4,    /* one workgroup per superblock, every level of 4:2:0 chroma */
  ODHIP_ROUTE_WALK_LO = 5,   /* walking workgroups, leaves up to 16x16 */
  ODHIP_ROUTE_SB_LO = 6,     /* one workgroup per superblock, luma leaves up to 16x16: not reachable
                                in a default build (a luma plane can always be walked) */
  ODHIP_ROUTE_PARTITION = 7  /* odhip_inverse_partition */
};
int odhip_inverse_route(int dec, int src, int leaf_bs, int w, int px_aligned16, int *route, int *nedges);

/* The same for ONE plane with host pointers (synchronous; staging through device
   scratch): coef = the decoder's state.dtmp[pli] (stride w), bsize = state.bsize.
   px is 8-bit: ODHIP_EIMPL, before anything is staged or launched, when the current context
   has full-precision references (its inverse stores int16 samples). */
int odhip_inverse_partition_host(uint8_t *px, int px_stride, const od_coeff *coef, int w, int h, int dec,
 const uint8_t *bsize, int bstride, int pic_w, int pic_h);

/* Forward at an ARBITRARY partition, the mirror of odhip_inverse_partition: the coefficients
   the encoder codes at the block-size map of each frame.  od_ref_plane_to_coeff and
   od_apply_prefilter_frame_sbs as in odhip_forward_pyramid, then od_compute_dcts' recursion
   (src/encode.c:1455-1512; the final pass of od_encode_recursive, :1660-1791):
   od_prefilter_split of every node that splits, fdct_2d of every leaf.  A leaf's
   coefficients depend on its ancestors' split filters, so they are NOT a level of the
   pyramid unless the whole superblock is one size.
   d_px: picture plane layout rules above (int16 samples in a full-precision context).
   d_coef: nplanes planes of w x h, plane p at + p*(long)w*h, row stride w, 16-byte aligned:
   what odhip_inverse_partition reads.  Each leaf holds its own forward DCT where it lies, DC
   included - what od_compute_dcts leaves for an inter frame (is_keyframe == 0) and what
   od_block_encode transforms in the final pass; the keyframe Haar tree over the DCs
   (src/encode.c:1497-1510, :1593-1657) is not built.
   d_bsize, bstride, bsize_frame_stride, planes_per_frame, dec, pic_w, pic_h: exactly as for
   odhip_inverse_partition.  A map that is not a quadtree gives unspecified coefficients, but
   no read or write leaves the planes and the map.
   ODHIP_EINVAL before anything is launched: w, h no multiples of 64 >> dec, the layout rules,
   bstride < 8*(w / (64 >> dec)), a NULL pointer, planes_per_frame < 1. */
int odhip_forward_partition(od_coeff *d_coef, const uint8_t *d_px, int px_stride, long px_plane_stride,
 int nplanes, int w, int h, int dec, const uint8_t *d_bsize, int bstride, long bsize_frame_stride,
 int planes_per_frame, int pic_w, int pic_h, odhip_stream stream);
/* The same for ONE plane with host pointers (synchronous; staging through device scratch):
   px = the encoder's 8-bit plane, bsize = state.bsize, coef = a d plane of stride w.
   ODHIP_EIMPL, before anything is staged or launched, when the current context has
   full-precision references (its forward reads int16 samples). */
int odhip_forward_partition_host(od_coeff *coef, const uint8_t *px, int px_stride, int w, int h, int dec,
 const uint8_t *bsize, int bstride, int pic_w, int pic_h);

/* ---- the PVQ band stages on the leaves of a block-size map -------------------------------

   The band stages below (odhip_pvq_job.bs, odhip_pvq_refjob.bs) take planes tiled by ONE block size;
   the planes of odhip_forward_partition / odhip_inverse_partition hold leaves of up to five.  These
   four calls connect them: list the leaves of each size, gather them into a dense plane set of that
   size, run the band stages on the dense sets unchanged (forward at the map -> PVQ of every leaf at
   its own size -> inverse at the map: the encoder's final pass), scatter the dequantised blocks back.

   Planes: nplanes planes of w x h coefficients, plane p at + p*(long)w*h, row stride w.  d_bsize,
   bstride, bsize_frame_stride, planes_per_frame, dec: exactly as for odhip_forward_partition.
   Leaf of size s (N = 4 << s, s = 0 .. 4 - dec): a block odhip_forward_partition transforms with
     fdct_2d[s] - od_compute_dcts' walk (src/encode.c:1466-1470): bs = max(map value at the node's
     top-left entry, dec), a leaf when bs equals the node's level, transform size bs - dec.  At
     dec = 1 an 8x8 luma area with map value 0 or 1 is one 4x4 chroma leaf.
   List of (s, p): the leaves of size s in plane p, each a uint32 index by*(w/N) + bx into the plane's
     grid of N x N blocks, in strictly ascending order (the same list every run); count[s*nplanes + p]
     is its length, at most (w/N)*(h/N).  In `lists` it starts at entry
       nplanes*SUM(t < s) (w/(4 << t))*(h/(4 << t)) + p*(w/N)*(h/N),
     so the lists of all sizes need fewer than nplanes*w*h/12 entries.
   Dense set of size s: nplanes planes of w x Hd_s, Hd_s = N * max over p of ceil(count / (w/N)),
     plane p at + p*(long)w*Hd_s; leaf i of plane p is the block at block row i / (w/N), block column
     i % (w/N) of plane p; every other block is zero.  Planes keep their identity (q_band2 /
     plane_split and d_q_plane of the jobs work on dense sets).  Hd_s == 0: no leaf, no job.
   A map that is not a quadtree gives unspecified lists, but no index repeats within a list and
   nothing outside the buffers is read or written.

   odhip_partition_leaves_host: host arithmetic on a host map, no HIP call - what a host entropy coder
     walks the exported decisions with.  Writes every list and count[ODHIP_NBSIZES*nplanes] (zero for
     the sizes above 4 - dec).
   odhip_partition_leaves: the same from a device map into device lists, on `stream`.  count is HOST
     memory: the call SYNCHRONISES the stream before it returns.
   odhip_partition_gather: copies every listed leaf of size s from the planes d_src into the dense set
     d_dense and writes the zero padding - every sample of the dense set is written.  d_list: the list
     of (s, plane 0) (the lists of one size are consecutive); count: HOST, the nplanes counts of size s.
     Any plane set of the layout: the source coefficients, and a reference (odhip_forward_partition of
     the prediction at the same map).  All counts zero: nothing is launched.
   odhip_partition_scatter: the inverse copy, leaves only.  After the scatter of every size present,
     d_dst is what odhip_inverse_partition takes as d_coef.
   ODHIP_EINVAL before anything is launched or allocated: w, h no multiples of 64 >> dec, dec, nplanes
   < 1, bstride < 8*(w / (64 >> dec)), a NULL pointer, planes_per_frame < 1, s outside 0 .. 4 - dec, a
   coefficient or dense base off 16 bytes, a count outside 0 .. (w/N)*(h/N).
   Chroma-from-luma at a map: odhip_cfl_refs_partition below builds the reference planes of keyframe chroma
   from the scattered luma planes (odhip_pvq_refjob.luma reads a uniform luma job and stays NULL here).
   Not covered: the keyframe Haar DC tree (DC passes through the band stages as it does at uniform
   levels), the pipe (odhip_pipe_*) and its decision export. */
int odhip_partition_leaves_host(uint32_t *lists, int32_t *count, int nplanes, int w, int h, int dec,
 const uint8_t *bsize, int bstride, long bsize_frame_stride, int planes_per_frame);
int odhip_partition_leaves(uint32_t *d_lists, int32_t *count, int nplanes, int w, int h, int dec,
 const uint8_t *d_bsize, int bstride, long bsize_frame_stride, int planes_per_frame, odhip_stream stream);
int odhip_partition_gather(od_coeff *d_dense, const od_coeff *d_src, int s, const uint32_t *d_list,
 const int32_t *count, int nplanes, int w, int h, int dec, odhip_stream stream);
int odhip_partition_scatter(od_coeff *d_dst, const od_coeff *d_dense, int s, const uint32_t *d_list,
 const int32_t *count, int nplanes, int w, int h, int dec, odhip_stream stream);

/* Chroma-from-luma reference planes at a block-size map: od_resample_luma_coeffs (src/intra.c:72-109) of
   every chroma leaf, as od_block_encode calls it (src/encode.c:1681-1686), so that a keyframe's chroma is
   coded at the frame's map: odhip_bsize_decide -> odhip_forward_partition -> no-reference band stage on the
   luma leaves -> THIS -> with-reference band stage (is_keyframe = 1) on the chroma leaves, the result
   gathered as their reference -> odhip_inverse_partition.

   d_luma: nplanes DEQUANTISED luma coefficient planes of w x h, plane p at + p*(long)w*h, row stride w -
   what odhip_partition_scatter leaves after the luma band stages and odhip_inverse_partition takes, so no
   extra pass produces it.  d_bsize, bstride, bsize_frame_stride: as for the partition calls at dec = 0;
   luma plane p uses the map at + p*bsize_frame_stride.
   d_ref: nplanes*planes_per_frame planes of (w >> dec) x (h >> dec), plane q at + q*(long)(w >> dec)*(h >> dec),
   row stride w >> dec; plane q is predicted from luma plane q / planes_per_frame (Cb and Cr of a frame
   adjacent: planes_per_frame = 2, both planes get the same values) - a plane set that
   odhip_partition_gather takes as the reference of the chroma planes at dec with the same planes_per_frame.

   dec = 1 (4:2:0), per chroma leaf of odhip_partition_leaves' walk:
     luma map value m >= 1  the luma leaf of N = 4 << m at luma (Y0, X0) gives the chroma leaf of n = N/2 at
                            (Y0/2, X0/2): ref[i][j] = luma[Y0 + i][X0 + j], i, j < n - the upper-left
                            quarter, the DC position copied as it is.
     luma map value 0       the 4x4 chroma leaf over the 8x8 luma area is od_tf_up_hv_lp (src/tf.c:82-108) of
                            the four 4x4 luma blocks, then (OD_CFL_SCALING4[j][i]*v + 64) >> 7 with
                            arithmetic shifts.
     The map value decides between the two kinds of 4x4 chroma leaf (obs at src/encode.c:1685): a 4x4 chroma
     leaf over an 8x8 luma BLOCK is the quarter copy.
   dec = 0 (4:4:4): od_resample_luma_coeffs copies the whole block, so every reference plane is a copy of its
     luma plane (the map is not read).  The path exists for a uniform interface; a 4:4:4 caller may hand the
     luma planes themselves over as the reference instead.

   Every sample of d_ref is written.  A map that is not a quadtree gives unspecified values, but nothing
   outside the planes and the map is read or written: a chroma sample reads luma samples and map entries of
   its own superblock only, whatever the bytes are.
   odhip_cfl_refs_partition_host: the same for ONE plane in host memory (ref (h >> dec) x (w >> dec), luma
     h x w, bsize rows of bstride), no HIP call and no alignment rule - what a host entropy coder or the shim
     calls.  The kernel and this function share their code.
   ODHIP_EINVAL before anything is launched or allocated: w or h no positive multiple of 64, dec outside
   0..1, nplanes < 1, planes_per_frame < 1, bstride < w/8, a NULL pointer, a device base off 16 bytes,
   d_ref == d_luma.
   Not covered: a pulse-fed form that reads the dense luma jobs through the leaf lists instead of the plane,
   4:2:2. */
int odhip_cfl_refs_partition(od_coeff *d_ref, const od_coeff *d_luma, int nplanes, int w, int h, int dec,
 const uint8_t *d_bsize, int bstride, long bsize_frame_stride, int planes_per_frame, odhip_stream stream);
int odhip_cfl_refs_partition_host(od_coeff *ref, const od_coeff *luma, int w, int h, int dec,
 const uint8_t *bsize, int bstride);

/* ---- a frame's block-size map by activity masking (bsize_kernels.hip) ----------

   What produces the d_bsize that odhip_forward_partition, odhip_inverse_partition and odhip_partition_leaves
   take: od_split_superblock (src/block_size_enc.c:331-456; its statistics od_compute_stats :56-131, the region
   averages od_noise_var4x4 :191-212 / od_noise_var8x8 :266-288, the masking sums od_psy_var4x4 :225-246 /
   od_psy_var8x8 :291-313) of every 32x32 cell of a luma plane - the psychovisual decider, a pure function of
   the pixels, an optional prediction and the quantiser.  The reference's frame-level wrapper
   (od_split_superblocks, src/encode.c:2381-2439) steps at the 64-sample superblock pitch over a bsize array it
   only partly writes and is not followed; the tiling is this library's: one call of the per-cell function for
   every 32x32 cell at a 32-sample pitch, and the samples of its 44x44 window (OD_BLOCK_OFFSET = 6 before and
   after the cell, src/block_size_enc.h:50-51) that fall outside the w x h plane are the plane's edge samples
   (coordinates clamped).  Map values are 0..3 (4x4 .. 32x32) - a legal quadtree for every reader of d_bsize.

   d_px, d_pred: nframes 8-bit planes of w x h, frame f at + f*plane_stride, row stride >= w (no alignment
   rule: the kernel reads bytes).  d_pred == NULL: a keyframe.  d_pred == d_px with equal strides is treated as
   NULL (the reference's psy_img == pred branch, :356: no coding-gain adjustment).  Otherwise the variances come
   from clamp(px - pred, -128, 127) and OD_CG4 / OD_CG8 are lowered above a quantiser of 40 << 4 (:361-362) -
   d_pred is what odhip_mc_predict_planes produces.
   d_bsize: one byte per 8x8 luma area, frame f's map at + f*bsize_frame_stride, row stride bstride >= w/8:
   exactly odhip_forward_partition's d_bsize at dec = 0 with planes_per_frame = 1.  Only the (h/8) x (w/8)
   entries of each frame are written; nothing outside the planes and the maps is read or written.
   quantizer: HOST memory, one value per frame: od_state.quantizer, scaled by 1 << OD_COEFF_SHIFT (the q of
   :334); read before the call returns.

   The device's log is OCML's, the reference's glibc's; every other operation is IEEE and identical.  A cell in
   which a step of an accumulation psy = (float)((double)psy + term) falls within the margin of a float
   rounding midpoint (derivation in bsize_kernels.hip) is not decided from the device's terms: it is LISTED.

   odhip_bsize_decide: asynchronous on `stream`.  Writes every map entry (a listed cell's from the device's
     terms, until the resolve) and keeps the list in the current context: one decide .. resolve sequence per
     context at a time.
   odhip_bsize_resolve: the same arguments again.  Synchronises the stream, decides the listed cells of the
     context's last decide again on the host with libm, writes their 16 map bytes to the device (blocking
     copies) and *relisted = their number.  ODHIP_EINVAL when no decide of these nframes, w, h precedes it.
   odhip_bsize_terms: test surface, like odhip_ssim_terms: decide and resolve in one synchronous call that
     also writes, per cell (cell = (f*(h/32) + cy)*(w/32) + cx), the ODHIP_BSIZE_TERMS noise averages and psy
     values the map was decided from - the host's for a relisted cell.  Order, as the reference keeps them in
     od_block_size_comp (src/block_size_enc.h:86-113): noise4_4[8][8], noise4_8[4][4], noise4_16[2][2],
     noise4_32, noise8_16[2][2], noise8_32; psy4[8][8], psy8[4][4], psy16[2][2], psy32 (both after OD_MAXF
     with the 8x8-based value, as the struct holds them), then the five od_psy_var8x8 values themselves, which
     the reference does not keep.
   odhip_bsize_decide_host, odhip_bsize_terms_host: the function restated in C++ for ONE plane in host memory -
     what the resolve runs.  No HIP call.  noise and psy optional (both or neither); *listed, optional: the
     cells that a device run with margin_scale (<= 0: 1) times the margin would have listed, judged from the
     host's own terms.
   No caller scratch (no odhip_bsize_sizeof): the list is nframes*(w/32)*(h/32) + 1 words of the context.

   ODHIP_EINVAL before anything is launched or allocated, and before any HIP call: w or h no positive multiple
   of 32 or above 8192, bstride < w/8, px_stride (pred_stride, with a prediction) < w, a NULL d_bsize, d_px,
   quantizer (d_noise, d_psy, relisted where they are taken), nframes < 1, a negative quantiser.  ODHIP_EIMPL in
   a full-precision-references context: the reference function takes 8-bit samples only.
   Not covered: the RDO decider (od_split_superblocks_rdo: sequential, bound to the entropy coder's state; it
   stays on the host), a pipe mode (odhip_pipe_* cannot code at a map yet), the binding behind the
   real encoder through the shim, and 64x64 decisions (the reference function has none). */
#define ODHIP_BSIZE_TERMS 90
int odhip_bsize_decide(uint8_t *d_bsize, int bstride, long bsize_frame_stride, const uint8_t *d_px,
 int px_stride, long px_plane_stride, const uint8_t *d_pred, int pred_stride, long pred_plane_stride, int nframes,
 int w, int h, const int32_t *quantizer, odhip_stream stream);
int odhip_bsize_resolve(uint8_t *d_bsize, int bstride, long bsize_frame_stride, const uint8_t *d_px,
 int px_stride, long px_plane_stride, const uint8_t *d_pred, int pred_stride, long pred_plane_stride, int nframes,
 int w, int h, const int32_t *quantizer, odhip_stream stream, int *relisted);
int odhip_bsize_terms(int32_t *d_noise, float *d_psy, uint8_t *d_bsize, int bstride,
 long bsize_frame_stride, const uint8_t *d_px, int px_stride, long px_plane_stride, const uint8_t *d_pred,
 int pred_stride, long pred_plane_stride, int nframes, int w, int h, const int32_t *quantizer, odhip_stream stream,
 int *relisted);
int odhip_bsize_decide_host(uint8_t *bsize, int bstride, const uint8_t *px, int px_stride,
 const uint8_t *pred, int pred_stride, int w, int h, int quantizer);
int odhip_bsize_terms_host(int32_t *noise, float *psy, uint8_t *bsize, int bstride, const uint8_t *px,
 int px_stride, const uint8_t *pred, int pred_stride, int w, int h, int quantizer, double margin_scale, int *listed);
/* Test hooks of the decision, per context (NULL: the calling thread's current one) like
   odhip_ctx_set_test_hooks: margin_scale multiplies the margin (<= 0: 1); perturb != 0 makes the device's map
   bytes and terms of every listed cell deliberately wrong, so that only the resolve's re-run can make them right. */
int odhip_ctx_set_bsize_test_hooks(odhip_ctx *ctx, double margin_scale, int perturb);

/* Batched pvq_search_rdo_double: band b has d_x[b*n .. b*n+n) int16,
   d_k[b], d_g2[b], optional d_prev_k[b] (NULL = 0; when > 0 d_y holds the
   previous pulses), writes d_y[b*n ..) and d_cos[b].  n <= 128; 0 <= k <= 65535
   (pulse magnitudes are kept in 16 bits): a band with K outside that range is not
   searched, its d_y is zero and its d_cos NaN. */
int odhip_pvq_search_batch(const int16_t *d_x, int n, const int32_t *d_k,
 od_coeff *d_y, const double *d_g2, double pvq_norm_lambda,
 const int32_t *d_prev_k, double *d_cos, long nbands, odhip_stream stream);

/* The same search (src/pvq_encoder.c:93-224, no chain: prev_k = 0) in its ROW form - one band per
   quad (n = 31, 32) or per 16-lane row (n = 127, 128), what the 32- and 128-coefficient bands of
   the with-reference stage run.  Its greedy pulses are screened in single precision and replayed
   with the reference's left-to-right double-precision scan whenever the screen cannot vouch for
   the argmax (a candidate within a relative 2^-17 of the best key that is not its exact
   duplicate); d_replays[b], when given, receives the number of pulses of band b that were
   replayed, force_scan != 0 replays every one (the cross-check).  Other n: ODHIP_EINVAL;
   K is clamped to 0..32767. */
int odhip_pvq_search_row_batch(const int16_t *d_x, int n, const int32_t *d_k, od_coeff *d_y,
 const double *d_g2, double pvq_norm_lambda, int force_scan, double *d_cos, int32_t *d_replays,
 long nbands, odhip_stream stream);

/* ---- PVQ band stage (the data-parallel part of pvq_theta) -------------------

   For every block of side N = 4 << bs of a batch of coefficient planes and
   every PVQ band of that block size (OD_BAND_OFFSETS, src/partition.c:77-91),
   the no-reference path of pvq_theta (src/pvq_encoder.c:333-641) up to, but
   not including, the rate-dependent choice: QM scaling to x16 (:381,:398),
   companded gain (:404), null-candidate distortion (:417), and for both gain
   candidates (:578-609) the pulse count K, the pruning test (:588), the
   K-pulse search and the distortion (:593-595).  The choice needs the rate of
   each candidate from the ADAPTIVE entropy coder (od_pvq_rate, :247-287), which
   is sequential host state in the reference and stays there; the host (or
   odhip_pvq_select_synth_noref with a rate table) applies `cost <= best_cost`.

   Block index: blk = (plane*(h/N) + by)*(w/N) + bx; B = number of blocks. */
#define ODHIP_MAX_BANDS 12
#define ODHIP_PVQ_MAX_K 32767
/* The reference's pulse count K is an int (od_pvq_compute_k, src/pvq.c:436-470); the pulse vectors here are int16.  A
   candidate the reference SEARCHES with K above ODHIP_PVQ_MAX_K - seen only below encoder_example's quantiser range, on
   saturated content in 64x64 blocks - is never searched or chosen by the band stages, so the band would differ from the
   reference's.  Every such band is counted on the device, per context (with-reference bands conservatively: before the
   reference's pruning test).  odhip_pvq_k_range_take: the current context's counts since the last call, cleared; returns
   ODHIP_ERANGE when either is non-zero (blocking copies; call it after the stream of the band stage has been synchronised).
   odhip_pipe_sync calls it and returns ODHIP_ERANGE: the results of the steps since the last sync are NOT the reference's. */
int odhip_pvq_k_range_take(unsigned *noref_bands, unsigned *ref_bands);
/* One record per (block, band), 64 bytes, 64-byte aligned: both halves are
   whole 32-byte HBM sectors and are written by different kernels (the first by
   the preparation pass, the second by the search). */
typedef struct {
  int32_t cg;          /* companded gain of x, Q8 (od_pvq_compute_gain)            */
  int32_t gain[2];     /* candidate gain index i; 0 = slot unused                  */
  int16_t k[2];        /* pulses (od_pvq_compute_k), saturated at ODHIP_PVQ_MAX_K  */
  uint8_t flags[2];    /* 1 = searched, 0 = pruned / unused, 2 = K above
                          ODHIP_PVQ_MAX_K (not representable: never chosen)        */
  uint8_t reserved0[6];
  double dist0;        /* distortion of the null (gain 0) candidate                */
  int32_t yy[2];       /* sum of squared pulses of the candidate                   */
  double dist[2];      /* distortion of the candidate                              */
  int32_t moment[2];   /* SUM i*|y_i| of the candidate's pulses: od_pvq_rate's
                          centre-of-mass sum (src/pvq_encoder.c:258-259)           */
} odhip_pvq_band;

typedef struct {
  odhip_pvq_band *band; /* [B][nb]                                                  */
  int16_t *y;           /* [2][B][len] signed pulse vectors in coding order (index
                           0 = DC slot, unused, may be overwritten with 0),
                           len = min(N*N, 512); 16-byte aligned                    */
  int32_t *choice;      /* [B][nb][4] written by odhip_pvq_select_synth_noref* /
                           odhip_pvq_choose_multi: {chosen slot, chosen gain index
                           qg (0 = null), synthesis scale, qshift}; 16-byte aligned */
  double *cos_dist;     /* optional [B][nb][2]: return value of
                           pvq_search_rdo_double per candidate (parity checks);
                           NULL = not stored                                       */
} odhip_pvq_cands;

/* One (plane set, block size) unit of work for the multi-job entry points.
   q_band / beta_band are HOST arrays [nb_bands]; everything prefixed d_ and the
   arrays inside `cands` are device memory.  d_qm is needed by the band stage,
   d_qm_inv and d_dq by select_synth; d_rate and d_qg are optional (NULL). */
typedef struct odhip_pvq_job_s {
  const od_coeff *d_coef;
  int nplanes;
  int w;
  int h;
  int bs;
  const int16_t *d_qm;
  const int16_t *d_qm_inv;
  const int32_t *q_band;
  const int32_t *beta_band;
  odhip_pvq_cands cands;
  od_coeff *d_dq;
  const double *d_rate;
  int32_t *d_qg;
  /* optional: planes plane_split .. nplanes-1 use q_band2 instead of q_band (HOST
     [nb_bands]): a chroma plane set holding the Cb planes first and the Cr planes
     after them - the per-band step comes from pvq_qm_q4[pli], which differs between
     Cb and Cr (OD_DEFAULT_QMS, src/encode.c:118-131, :3052-3072).  NULL = one table. */
  const int32_t *q_band2;
  int plane_split;
  /* optional, DEVICE [nplanes][ODHIP_MAX_BANDS]: the step of band b of plane p is
     d_q_plane[p*ODHIP_MAX_BANDS + b] (every plane its own quantiser, odhip_pipe_set_quants);
     q_band / q_band2 are then still checked but not used by the kernels.  NULL = q_band /
     q_band2 as above.  Read by the kernels of every call on this job, in stream order. */
  const int32_t *d_q_plane;
} odhip_pvq_job;

/* All jobs (at most 16) in one set of launches, so that small levels (510
   64x64 blocks per frame) overlap with large ones instead of serialising their
   tails.  Jobs of one call must use one stream. */
int odhip_pvq_noref_bands_multi(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);
int odhip_pvq_select_synth_noref_multi(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);

/* The choice alone (fills cands.choice and the optional d_qg of every job):
   for callers that dequantise inside the inverse stage, below. */
int odhip_pvq_choose_multi(const odhip_pvq_job *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);

/* odhip_inverse_level fed directly by the band stage: the chosen pulse vectors
   of `job` (cands.y, cands.choice after odhip_pvq_choose_multi or
   odhip_pvq_select_synth_noref*) are dequantised while the superblock tile is
   loaded (od_pvq_synthesis_partial noref src/pvq.c:1081-1092,
   od_coding_order_to_raster src/partition.c:176-194), DCs come from
   job->d_coef; the dequantised plane is never written to HBM.  Partition level
   = job->bs; needs job->d_qm_inv.  Same output as odhip_pvq_select_synth_noref
   followed by odhip_inverse_level. */
int odhip_inverse_level_pvq(uint8_t *d_px, int px_stride, long px_plane_stride,
 const odhip_pvq_job *job, int dec, int pic_w, int pic_h, odhip_stream stream);

/* Chroma-from-luma predictions of a 4:2:0 keyframe: od_resample_luma_coeffs
   (src/intra.c:72-109) for luma blocks of 8x8 and larger (:97-108: the upper-left
   quarter of the decoded luma block's coefficients), fed directly by the luma band
   stage - the decoded coefficients are dequantised on the fly from the chosen
   pulses (cands.y, cands.choice after odhip_pvq_choose_multi) exactly as
   odhip_pvq_select_synth_noref would write them; no dequantised luma plane is
   needed.  luma_jobs[j] (level bs >= 1, blocks of N = 4 << bs; needs d_qm_inv)
   yields the reference planes of the chroma level bs - 1 (blocks of N/2) in
   d_ref[j]: `copies` consecutive plane sets of [nplanes][h/2][w/2] (Cb and Cr
   share the prediction: copies = 2), ready to be odhip_pvq_refjob.d_ref.  A
   level-0 job (4x4 luma blocks) yields the 4x4 chroma predictions of the 4:2:0
   TF branch (:77-89: od_tf_up_hv_lp of the four luma blocks over the chroma block,
   src/tf.c:82-108, then OD_CFL_SCALING4), the alternative prediction of chroma
   level 0 when the luma partition there is 4x4. */
int odhip_cfl_refs_from_luma(const odhip_pvq_job *luma_jobs, int njobs, od_coeff *const *d_ref,
 int copies, odhip_stream stream);
/* prezeroed != 0: the caller guarantees that the positions a 64x64 luma level never codes
   (half of each 32x32 chroma reference block) are already zero in d_ref - buffers that were
   cleared once and are only ever written by this function - and the per-call clear of that
   plane set is skipped. */
int odhip_cfl_refs_from_luma_ex(const odhip_pvq_job *luma_jobs, int njobs, od_coeff *const *d_ref,
 int copies, int prezeroed, odhip_stream stream);

/* Profiling aid (bench.py): while enabled, odhip_pvq_noref_bands_multi brackets
   its dominant kernel - the search of the 128-coefficient bands,
   k_search<128,2> - with HIP events on the stream the kernel is launched on
   (up to 256 calls are kept).  odhip_pvq_profile_read waits for the recorded
   events, writes one duration in milliseconds per call to ms[] and returns how
   many (or a negative ODHIP_E* code), then starts over. */
int odhip_pvq_profile(int enable);
int odhip_pvq_profile_read(float *ms, int max_n);

/* odhip_inverse_level_pvq for several partition levels of ONE plane set (same
   nplanes, w, h, dec; at most 5 jobs) in a single set of launches: level i of
   jobs[] is reconstructed into d_px[i] (distinct buffers, same strides). */
int odhip_inverse_levels_pvq(uint8_t *const *d_px, int px_stride, long px_plane_stride,
 const odhip_pvq_job *jobs, int njobs, int dec, int pic_w, int pic_h, odhip_stream stream);

/* nb_bands, offsets[nb_bands+1] and len for block size bs. */
int odhip_pvq_band_layout(int bs, int *nb_bands, int *offsets, int *len);

/* d_qm: QM in coding order for this (bs, decimation): od_state.qm +
   od_qm_offset(bs, xdec) (src/pvq.c:306, src/encode.c:1355-1358), int16,
   device.  q_band / beta_band: HOST arrays [nb_bands]: the per-band quantiser
   max(1, q0*pvq_qm_q4[od_qm_get_index(bs, i+1)] >> 4) (src/pvq_encoder.c:874)
   and OD_PVQ_BETA[masking][pli][bs][i] (src/pvq.c:243-268). */
int odhip_pvq_noref_bands(const od_coeff *d_coef, int nplanes, int w, int h,
 int bs, const int16_t *d_qm, const int32_t *q_band, const int32_t *beta_band,
 double pvq_norm_lambda, const odhip_pvq_cands *out, odhip_stream stream);

/* Choice + decoder-identical dequantisation of the chosen candidate into d_dq
   (same plane layout as d_coef; DC passed through; uncoded positions zero):
   od_gain_expand (src/pvq.c:766), od_pvq_synthesis_partial noref
   (src/pvq.c:1037-1093), od_coding_order_to_raster (src/partition.c:176).
   d_rate: [B][nb][2] bits per candidate from the host entropy model, or NULL
   (distortion-only choice).  There is no slot for the null (gain 0) candidate:
   its rate is identically zero in the reference (od_pvq_rate returns 0 for k == 0
   and adds the theta terms only when qg > 0, src/pvq_encoder.c:250-251,:276), so
   best_cost starts at dist0 exactly as at :417-421.  d_qg_out: optional [B][nb] chosen gain index. */
int odhip_pvq_select_synth_noref(od_coeff *d_dq, const od_coeff *d_coef,
 int nplanes, int w, int h, int bs, const int16_t *d_qm_inv,
 const int32_t *q_band, const int32_t *beta_band, double pvq_norm_lambda,
 const odhip_pvq_cands *in, const double *d_rate, int32_t *d_qg_out,
 odhip_stream stream);

/* ---- with-reference (theta / Householder) path: data-parallel pieces -----------

   pvq_theta with a reference vector r (inter frames, chroma-from-luma;
   src/pvq_encoder.c:381-565) around its one libm call, acos(corr) (:478), which
   is not reproducible bit for bit on the device and stays on the host, as does
   od_pvq_rate (adaptive entropy coder).  All vectors are plain band vectors
   [band][n] in coding order, device memory; n <= 128 (OD_MAX_PVQ_SIZE).

   odhip_pvq_ref_prepare    :381-438 and the Householder reflection
                            (od_compute_householder / od_apply_householder,
                            src/pvq.c:498-623): x16, r16 (r16[m] updated as the
                            reference does when the reflection is computed, i.e.
                            when r != 0 and corr > 0), the reflected x without
                            element m in d_xr [band][n-1], and one record per
                            band.  q0 = per-band quantiser, beta = OD_PVQ_BETA
                            entry (Q12), cfl_enabled as at :410.
   odhip_pvq_ref_candidates :466-504 given d_theta[band] =
                            floor(.5 + OD_THETA_SCALE*acos(corr)) from the host:
                            the (gain, theta) candidates with their K
                            (od_pvq_compute_max_theta, od_pvq_compute_theta,
                            od_pvq_compute_k nodesync branch, src/pvq.c:855-953)
                            in the reference's stable (k, gain) order; up to
                            ODHIP_PVQ_MAX_REFCANDS per band.
   odhip_pvq_synthesis      od_pvq_synthesis_partial (src/pvq.c:1037-1115) of a
                            chosen candidate; d_params[band] = {noref, g
                            (od_gain_expand result), theta (Q15 angle), m, s};
                            d_y holds n pulses (n-1 used when noref == 0).

   The K-pulse searches of the candidates are odhip_pvq_search_batch on d_xr. */
typedef struct {
  int32_t xshift, rshift;
  int32_t g, gr;          /* raw gains (od_pvq_compute_gain *g)                 */
  int32_t cg, cgr;        /* companded gains, Q8 (cgr = 256 when cfl_enabled)   */
  int32_t icgr, gain_offset;
  int32_t m, s;           /* Householder pivot and sign (0, 1 when not computed) */
  int32_t r_null;         /* 1 = the reference vector is all zero                */
  int32_t reserved;
  double corr;            /* clamped correlation, :436-438                       */
  double reserved2;
} odhip_pvq_refprep;      /* 64 bytes */

#define ODHIP_PVQ_MAX_REFCANDS 24
typedef struct {
  int32_t gain, theta, ts, k, qcg, qtheta;
} odhip_pvq_refcand;

int odhip_pvq_ref_prepare(const od_coeff *d_x0, const od_coeff *d_r0, int n, long nbands,
 const int16_t *d_qm, int q0, int beta, int cfl_enabled, int16_t *d_x16, int16_t *d_r16,
 int16_t *d_xr, odhip_pvq_refprep *d_out, odhip_stream stream);
int odhip_pvq_ref_candidates(const odhip_pvq_refprep *d_prep, const int32_t *d_theta, int n,
 long nbands, int beta, odhip_pvq_refcand *d_items, int32_t *d_nitems, odhip_stream stream);
int odhip_pvq_synthesis(od_coeff *d_out, const od_coeff *d_y, const int16_t *d_r16, int n,
 long nbands, const int32_t *d_params, const int16_t *d_qm_inv, odhip_stream stream);

/* ---- decoder side: a PVQ band from its decoded symbols ------------------------------

   pvq_decode_partition (src/pvq_decoder.c:122-298; od_pvq_decode :300-376 calls it per band)
   AFTER its entropy-decoder reads, for a batch of band vectors [band][n] in coding order
   (device memory): d_sym[band] = {the gain symbol as read - id & 1, or 1 + the
   generic_decode value, before deinterleaving (:190-208) -, itheta after the theta decode
   (:248-254), noref, unused}; d_y the decoded pulses (n - !noref of them, :262-266), d_ref
   the reference band (the prediction, after the chroma-from-luma flip where one was read).
   Computes what the function computes from them: the reference's scaling and gain, the
   deinterleaved gain, gain_offset, theta (:213-255), the skip rules, od_gain_expand and
   pvq_synthesis = od_compute_householder + od_pvq_synthesis_partial (:78-89, :268-279) into
   d_out; d_info (optional) [band][2] = {K as the decoder derives it under OD_ROBUST_STREAM
   (od_pvq_compute_k, nodesync), skip code 0 / OD_PVQ_SKIP_ZERO 1 / OD_PVQ_SKIP_COPY 2}.
   The entropy decoding itself (od_decode_cdf_adapt, generic_decode,
   od_decode_pvq_codeword) is sequential host state and stays the reference's; under
   OD_ROBUST_STREAM (nodesync = 1, src/encode.c:1354) none of its reads depends on a value
   computed here, so a decoder can parse a whole frame first and reconstruct its bands in
   batches.  q0 / beta: the band's quantiser step and OD_PVQ_BETA entry. */
int odhip_pvq_decode_bands(od_coeff *d_out, const od_coeff *d_ref, const od_coeff *d_y, int n,
 long nbands, const int32_t *d_sym, const int16_t *d_qm, const int16_t *d_qm_inv, int q0, int beta,
 int is_keyframe, int pli, int32_t *d_info, odhip_stream stream);

/* ---- with-reference band stage on whole planes ---------------------------------

   pvq_theta (src/pvq_encoder.c:333-641) for every block of side N = 4 << bs of a
   batch of coefficient planes and every PVQ band, WITH a reference plane of the
   same layout (keyframe chroma: the chroma-from-luma prediction; inter frames:
   the transformed motion-compensated prediction), up to but not including the
   rate-dependent choice:

     - the chroma-from-luma sign flip of od_pvq_encode (:846-872) per block when
       is_keyframe && pli != 0 (the reference plane itself is not modified: the
       flip is recorded and applied on the fly);
     - QM scaling of x and r, gains, correlation, null-candidate distortion
       (:381-455), od_compute_householder / od_apply_householder
       (src/pvq.c:498-623);
     - theta = floor(.5 + OD_THETA_SCALE*acos(corr)) (:478) with the device's
       acos.  The reference's value comes from the host libm, which is not
       reproducible bit for bit on the device; the integer theta is, except when
       OD_THETA_SCALE*acos(corr) + .5 lies within 1e-9 of an integer (the two
       libraries agree to < 1e-10 there, tests/test_gpu_pvq_refbands.py).  Such bands
       are listed and odhip_pvq_ref_resolve settles them with the host's libm;
     - the (gain, theta) candidates in the reference's order (:466-504), the
       pruning test (:531), the K-pulse searches on the reflected vector with the
       prev_k chain (:536-545) and the distortion of every candidate (:548-552);
     - the no-reference candidates (:571-609) when the reference's condition
       (:571-573) holds.

   od_pvq_rate (adaptive entropy coder) stays on the host:
   odhip_pvq_ref_select_synth_multi takes its rate table, applies `cost <
   best_cost` to the theta candidates and `cost <= best_cost` to the
   no-reference ones in the reference's order, then the skip rules (:611-622)
   and the decoder-identical synthesis (:623-633).

   Block index blk = (plane*(h/N) + by)*(w/N) + bx, B = number of blocks, nb =
   bands of the block size, len = min(N*N, 512).  Band i of block blk: record
   band[blk*nb + i]; its candidates occupy slots 0 .. nitems-1 (theta candidates
   first, in search order, then the no-reference ones); pulse vector of slot s at
   y[(s*B + blk)*len + off[i] ..] (signed int16, coding order; n-1 values for a
   theta candidate, n for a no-reference one).

   `items` holds the candidates of all bands as THREE planes of 16-byte vectors,
   each [nb][ODHIP_PVQ_REF_SLOTS][B] (block index fastest: adjacent lanes =
   adjacent blocks = adjacent vectors): vector (i*ODHIP_PVQ_REF_SLOTS + s)*B + blk
   of plane 0 is {gain, theta, ts, k}, of plane 1 (at + nb*SLOTS*B vectors)
   {qcg, qtheta, flags, yslot}, of plane 2 {cos_dist, dist}; odhip_pvq_refitem
   below names the fields (it is the gathered form, 48 bytes). */
#define ODHIP_PVQ_REF_SLOTS 16
#define ODHIP_REFBAND_R_NULL 1      /* the reference band is all zero                   */
#define ODHIP_REFBAND_THETA 2       /* the theta search ran (:452)                      */
#define ODHIP_REFBAND_NOREF 4       /* the no-reference candidates ran (:571)           */
#define ODHIP_REFBAND_FLIP 8        /* chroma-from-luma: reference of the block negated */
#define ODHIP_REFBAND_UNCERTAIN 16  /* theta within the margin: see odhip_pvq_ref_resolve */
typedef struct {
  int32_t xshift, rshift;
  int32_t g, gr;          /* raw gains                                          */
  int32_t cg, cgr;        /* companded gains, Q8 (cgr = 256 with CfL)           */
  int32_t icgr, gain_offset;
  int16_t m;              /* Householder pivot (0 when not computed)            */
  int8_t s;               /* Householder sign (1 when not computed)             */
  uint8_t flags;          /* ODHIP_REFBAND_*                                    */
  int32_t theta;          /* Q15 angle index, 0 when the theta search did not run */
  int32_t nitems;         /* candidates in items[]                              */
  int32_t ntheta;         /* how many of them are theta candidates (the first)  */
  double corr;            /* clamped correlation (:436-438)                     */
  double dist0;           /* distortion of the initial candidate (:455)         */
} odhip_pvq_refband;      /* 64 bytes */

#define ODHIP_REFITEM_SEARCHED 1    /* not pruned (:531, :588)                          */
#define ODHIP_REFITEM_WITH_REF 2    /* theta candidate                                  */
#define ODHIP_REFITEM_K_RANGE 4     /* K above ODHIP_PVQ_MAX_K: pulses would not fit the
                                       int16 vectors; reported, never searched or chosen */
#define ODHIP_REFITEM_MOMENT_SHIFT 8 /* flags >> 8: SUM i*|y_i| of the candidate's pulses
                                       (od_pvq_rate's centre-of-mass sum, :258-259; below
                                       2^24 for n <= 128, K <= 32767), 0 when not searched */
typedef struct {
  int32_t gain;           /* i                                                  */
  int32_t theta;          /* j, -1 for a no-reference candidate                 */
  int32_t ts;             /* max_theta                                          */
  int32_t k;
  int32_t qcg;
  int32_t qtheta;
  int32_t flags;          /* ODHIP_REFITEM_* in bits 0-7, the pulse moment above  */
  int32_t yslot;          /* slot holding this candidate's pulses (a candidate
                             with the K of its predecessor shares its slot,
                             :539-544); -1 = all zero                           */
  double cos_dist;        /* return value of pvq_search_rdo_double              */
  double dist;
} odhip_pvq_refitem;      /* 48 bytes */

/* choice[(blk*nb + i)*16 ..]: {item (-1 = the initial candidate), qg, noref,
   itheta, max_theta, k, skip (0, OD_PVQ_SKIP_ZERO 1, OD_PVQ_SKIP_COPY 2), the
   return value of pvq_theta (:636-637)}, then 8 words of synthesis parameters
   private to the library. */
typedef struct {
  const od_coeff *d_coef;    /* nplanes planes w x h of level bs               */
  const od_coeff *d_ref;     /* reference planes, same layout                  */
  int nplanes;
  int w;
  int h;
  int bs;
  int is_keyframe;
  int pli;
  const int16_t *d_qm;       /* as odhip_pvq_job                               */
  const int16_t *d_qm_inv;   /* select_synth only                              */
  const int32_t *q_band;     /* HOST [nb]                                      */
  const int32_t *beta_band;  /* HOST [nb]                                      */
  odhip_pvq_refband *band;   /* out [B][nb], 64-byte aligned                   */
  void *items;               /* out: 3 planes [nb][ODHIP_PVQ_REF_SLOTS][B] of 16-byte
                                vectors (see above), 16-byte aligned           */
  int16_t *y;                /* out [ODHIP_PVQ_REF_SLOTS][B][len]; y, r16, x16,
                                xr 16-byte aligned                             */
  int16_t *r16;              /* out [B][len]: QM-scaled reference after
                                od_compute_householder (input of the synthesis) */
  int16_t *x16;              /* work [B][len]                                  */
  int16_t *xr;               /* work [B][len]: reflected x without element m   */
  const double *d_rate;      /* select_synth: optional [B][nb][ODHIP_PVQ_REF_SLOTS + 1]
                                bits; entry 0 = the initial candidate (:420 /
                                :452), entry 1 + i = items[i]; NULL = choose on
                                distortion alone                               */
  int32_t *choice;           /* select_synth out [B][nb][16], 16-byte aligned  */
  od_coeff *d_dq;            /* select_synth out: dequantised planes, layout of
                                d_coef; DC passed through; uncoded positions 0 */
  const int32_t *q_band2;    /* optional, HOST [nb]: as odhip_pvq_job.q_band2 - */
  int plane_split;           /* planes plane_split.. (the Cr half) use q_band2  */
  const struct odhip_pvq_job_s *luma; /* optional (keyframe chroma): the chroma-from-luma reference
                                taken STRAIGHT from the luma band stage instead of a
                                reference plane - od_resample_luma_coeffs for luma blocks
                                of 8x8 and larger, src/intra.c:97-108.  `luma` is the
                                job of the luma level bs + 1 over the same picture(s)
                                (4:2:0: planes 2w x 2h, nplanes or nplanes / 2 of them:
                                Cb and Cr share the prediction) or, for 4:4:4, the job
                                of the SAME level bs over planes of the same w x h (the
                                copy branch, :95-108: the whole decoded luma block;
                                chroma block blk reads luma block blk mod the luma
                                job's block count) after its choice
                                (odhip_pvq_choose_multi / the priced band stage): its
                                cands.y, cands.choice and d_qm_inv are read by the
                                preparation kernels, which dequantise the co-located
                                coefficients on the fly.  d_ref may then be NULL (the
                                synthesis into planes, odhip_pvq_ref_select_synth_multi,
                                still needs it).  What odhip_cfl_refs_from_luma would
                                have written, without the planes: 0.8 GB of traffic per
                                16-frame step and a kernel less.                     */
  const int32_t *d_q_plane;  /* optional, DEVICE [nplanes][ODHIP_MAX_BANDS]: as
                                odhip_pvq_job.d_q_plane                          */
} odhip_pvq_refjob;

/* At most 8 jobs per call, all on one stream.  The stage keeps per-call state
   (job table, scratch, uncertainty list) in the current odhip_ctx: ONE call
   sequence (bands -> resolve -> select_synth) may be in flight per context.
   odhip_pvq_ref_set_context(0 | 1) is round 1's form of that: it selects which of
   the calling thread's two DEFAULT contexts the next calls use while no explicit
   context is current (so that e.g. the Cb and the Cr planes of a batch can run on
   two streams at once); new code creates contexts with odhip_create. */
int odhip_pvq_ref_set_context(int ctx);
int odhip_pvq_ref_bands_multi(const odhip_pvq_refjob *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);
/* Settles the bands odhip_pvq_ref_bands_multi flagged ODHIP_REFBAND_UNCERTAIN:
   waits for the stream, evaluates floor(.5 + OD_THETA_SCALE*acos(corr)) with the
   HOST libm (the function the reference itself calls) for the listed bands and
   re-runs those whose theta differs.  Pass the same jobs.  Returns the number
   of bands re-run (normally 0; about 2 in 10^9 bands are listed at all), or a
   negative ODHIP_E* code.  Results are exact only after this call. */
int odhip_pvq_ref_resolve(const odhip_pvq_refjob *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);
/* The same without a host wait in the middle of a pipeline: _begin (right after
   odhip_pvq_ref_bands_multi, same stream) sends the count of listed bands to
   pinned host memory; the caller enqueues whatever follows (choice, synthesis,
   inverse) speculatively; _finish waits for the count only, returns 0 when no band
   is listed (the normal case) and otherwise does what odhip_pvq_ref_resolve does
   and returns how many bands were re-run - the caller then repeats the steps that
   consumed the candidates. */
int odhip_pvq_ref_resolve_begin(odhip_stream stream);
int odhip_pvq_ref_resolve_finish(const odhip_pvq_refjob *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);
int odhip_pvq_ref_select_synth_multi(const odhip_pvq_refjob *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);
/* Profiling aid (bench.py), as odhip_pvq_profile: while enabled,
   odhip_pvq_ref_bands_multi brackets the dominant kernel of this stage - the
   row-parallel search of the 128-coefficient bands, k_refb_search_row<8> - with
   HIP events on the stream the kernel is launched on (calls of the current context). */
int odhip_pvq_ref_profile(int enable);
int odhip_pvq_ref_profile_read(float *ms, int max_n);
/* The choice alone (fills `choice` incl. the synthesis parameters), for callers that
   dequantise inside the inverse stage: odhip_inverse_levels_pvq_ref reconstructs the
   partition levels jobs[i].bs of ONE plane set (same nplanes, w, h, dec; at most 5
   jobs) into d_px[i], dequantising the chosen candidates of the with-reference
   stage while the superblock tile is loaded (od_pvq_synthesis_partial with or
   without reference, skip-copy and skip-zero bands included; DCs from d_coef); the
   dequantised plane never exists in HBM.  Same pixels as
   odhip_pvq_ref_select_synth_multi followed by odhip_inverse_levels. */
int odhip_pvq_ref_choose_multi(const odhip_pvq_refjob *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);
int odhip_inverse_levels_pvq_ref(uint8_t *const *d_px, int px_stride, long px_plane_stride,
 const odhip_pvq_refjob *jobs, int njobs, int dec, int pic_w, int pic_h, odhip_stream stream);
/* The whole band stage with the priced choice (od_pvq_rate's closed form, speed > 0,
   src/pvq_encoder.c:250-264) of EVERY band made inside its search: nothing per candidate
   reaches memory.  Outputs: choice[] of every job and the winner's pulse vector of every
   coded band in slot 0 of the job's y (choice word 9 names the slot: 0, or -1 when the
   winner places no pulse); items and the other slots of y are scratch of the resolve
   paths.  The counts of bands inside the theta margin and inside the price margin are on
   their way to the host when this returns: follow with odhip_pvq_ref_resolve_finish and
   odhip_pvq_ref_choose_priced_resolve (same jobs and stream; both normally return 0; a band
   they re-run through the exporting kernels is decided again by them), then consume the
   choices (odhip_inverse_levels_pvq_ref).  A job must carry its choice buffer. */
int odhip_pvq_ref_bands_decided_multi(const odhip_pvq_refjob *jobs, int njobs,
 double pvq_norm_lambda, odhip_stream stream);
/* (Test hooks - the uncertainty margin, a deliberately wrong device theta for listed bands,
   the scale of the priced choice's margin - are per context: odhip_ctx_set_test_hooks.) */
/* S*acos(corr) + .5 as the device evaluates it (parity check of the margin). */
int odhip_pvq_ref_theta_probe(const double *d_corr, double *d_t, long n, odhip_stream stream);

/* ---- deringing filter (src/dering.c) ----------------------

   od_dering_hip has od_dering's arguments (src/dering.h:64-69, definition
   src/dering.c:252-257: ..., nhb, nvb, ...) minus the function table it
   dispatches through (od_dering_opt_vtbl): host pointers, synchronous, full
   superblocks (nhb == nvb == 8) and partial ones (1..8 blocks a side: only those
   blocks are read, filtered and written, and only their dir[][] entries).  A
   reference build binds it with
     #define od_dering(vtbl, ...) od_dering_hip(__VA_ARGS__)
   at its call sites (src/encode.c:2787,2826; src/decode.c).

   odhip_dering_planes filters EVERY superblock of nplanes planes for ncand
   candidate thresholds in one launch (what the encoder's per-superblock level
   search, src/encode.c:2785-2810, evaluates): d_x int16 [plane][h][stride]
   (h = nvsb*64 >> xdec), d_y int16 [plane][cand][h][stride], d_dirs int32
   [plane][nvsb*8][nhsb*8] (written when pli == 0, read otherwise), d_bskip the
   skip map of each plane (rows of skip_stride bytes, planes
   bskip_plane_stride bytes apart), d_thresholds int32 [plane][cand][nvsb*nhsb]
   (0 leaves a superblock unchanged). */
void od_dering_hip(int16_t *y, int ystride, const int16_t *x, int xstride, int nhb, int nvb,
 int sbx, int sby, int nhsb, int nvsb, int xdec, int dir[8][8], int pli, unsigned char *bskip,
 int skip_stride, int threshold, int overlap, int coeff_shift);
int odhip_dering_planes(int16_t *d_y, const int16_t *d_x, int stride, int nhsb, int nvsb, int xdec,
 int nplanes, int32_t *d_dirs, int pli, const uint8_t *d_bskip, int skip_stride,
 long bskip_plane_stride, const int32_t *d_thresholds, int ncand, int overlap, int coeff_shift,
 odhip_stream stream);

/* ---- the deringing level search of a frame behind od_dering -----------------------

   After coding a frame the reference searches the deringing level superblock by
   superblock (src/encode.c:2697-2832): od_dering on the luma superblock for each of
   the five non-zero levels, then on the three planes with the level chosen - up to
   4 080 calls per 1080p frame, every one reading the same unfiltered copy of the frame
   (state->etmp) and skip map.  An odhip_dering_cache serves them from batched passes:
   the first call with a (plane, threshold) pair filters every superblock of the plane
   in one launch (odhip_dering_planes) and keeps the filtered plane on the host; that
   call and all later ones with the same pair copy their superblock out (and, for luma,
   the directions od_dering returns in dir[][]).  The level decision, its cost and the
   adaptation stay in the encoder.

   odhip_dering_cache_begin marks a new frame (the planes and the skip map have been
   rewritten: where the encoder copies ctmp to etmp, src/encode.c:2700-2707).
   odhip_dering_cache_call has od_dering's arguments minus the function table; x must
   point into the plane at the superblock (as the encoder's call sites do, :2787,:2826)
   and bskip into the skip map likewise.  Glue in a reference build:
     odhip_dering_cache_begin(cache);                                    at :2697
     #define od_dering(vtbl, ...) odhip_dering_cache_call(cache, __VA_ARGS__)
   Partial superblocks and chroma calls that precede every luma call of the frame go
   to the per-call path od_dering_hip.  After a luma pass of a frame, a full-superblock
   chroma call whose nhsb / nvsb are not that luma plane's is ODHIP_EINVAL (the frame's
   directions do not fit it).  One cache per encoder (it binds the thread's
   current odhip_ctx at creation). */
typedef struct odhip_dering_cache odhip_dering_cache;
odhip_dering_cache *odhip_dering_cache_create(void);
void odhip_dering_cache_destroy(odhip_dering_cache *c);
void odhip_dering_cache_begin(odhip_dering_cache *c);
int odhip_dering_cache_call(odhip_dering_cache *c, int16_t *y, int ystride, const int16_t *x, int xstride,
 int nhb, int nvb, int sbx, int sby, int nhsb, int nvsb, int xdec, int dir[8][8], int pli,
 unsigned char *bskip, int skip_stride, int threshold, int overlap, int coeff_shift);
void odhip_dering_cache_stats(const odhip_dering_cache *c, long *launches, long *served);
/* The level search's distortions (od_compute_dist, src/encode.c:1170-1226, called six times per
   superblock at :2776-2801) from the same batched passes: after odhip_dering_cache_begin, hand the
   frame's luma source picture (8-bit samples; host and device copies, e.g. odhip_cache_plane_pixels
   of the frame cache) to odhip_dering_cache_set_source - every luma pass then also computes the
   distortion parts of its whole output against it (odhip_dist_parts_px16) - and ask
   odhip_dering_cache_dist in front of od_compute_dist: it answers (1, *dist) only when x IS the
   source superblock and y IS the cached filtered superblock of that threshold (both compared sample
   by sample), with the host-libm finish of odhip_dist_finish; otherwise 0 and the C function runs. */
int odhip_dering_cache_set_source(odhip_dering_cache *c, const uint8_t *h_px, const uint8_t *d_px, int stride,
 int use_masking, int flat_qm);
int odhip_dering_cache_dist(odhip_dering_cache *c, const od_coeff *x, const od_coeff *y, int n, int sbx, int sby,
 int threshold, int use_masking, int flat_qm, int coded_quantizer, double *dist);
long odhip_dering_cache_dist_served(const odhip_dering_cache *c);

/* ---- od_compute_dist: the block-size RDO's distortion ----------

   od_compute_dist(enc, x, y, n) (src/encode.c:1202-1226, od_compute_dist_8x8
   :1113-1169, od_compute_var_4x4 :1082-1103) for EVERY n x n block (n = 4 << bs, bs =
   1..4) of a batch of plane pairs x (source) / y (reconstruction), both od_coeff planes
   of w x h (multiples of n) in the lapped domain, as the encoder compares them at
   src/encode.c:1418-1421, :1797-1798.  Split at the libm call:
     odhip_dist_parts   (device) per 8x8 block three doubles: the sum of the squared
                        [1 5 1]^2 low-passed error, vardist, and the ARGUMENT of pow
                        (.25 + var_stat/256) - d_parts [plane][h/8][w/8][3];
     odhip_dist_finish  (host)   activity = calibration*pow(arg, -1/6) with the host
                        libm the reference calls, activity^2*(0.92/7^4*sum + vardist), the
                        sum over the block's 8x8 blocks in raster order and the
                        coded-quantiser factor: dist [plane][h/n][w/n].
   use_masking = enc->use_activity_masking, flat_qm = (enc->qm == OD_FLAT_QM: plain
   squared error), coded_quantizer = state.coded_quantizer. */
/* Per-call form with od_compute_dist's arguments (host pointers, compact n x n blocks,
   synchronous; enc's three fields passed): a reference build binds it at the top of its
   file-static od_compute_dist (oracle/Makefile builds that variant,
   _ref/libdaalaref_disthip.so, for tests/test_gpu_dropin_encoder.py). */
double od_compute_dist_hip(const od_coeff *x, const od_coeff *y, int n, int use_masking, int flat_qm,
 int coded_quantizer);
int odhip_dist_parts(double *d_parts, const od_coeff *d_x, const od_coeff *d_y, int nplanes, int w,
 int h, int bs, int use_masking, int flat_qm, odhip_stream stream);
int odhip_dist_parts_px16(double *d_parts, const uint8_t *d_x8, int x8_stride, const int16_t *d_y16,
 int y16_stride, int nplanes, int w, int h, int bs, int use_masking, int flat_qm, odhip_stream stream);
int odhip_dist_finish(double *dist, const double *parts, int nplanes, int w, int h, int bs,
 int use_masking, int flat_qm, int coded_quantizer);

/* ---- input side: padding a picture to the coded frame size ----

   od_img_plane_copy_pad (src/encode.c:752-837; daala_image_copy_pad :1896-1909,
   called when a frame enters the input queue) for a batch of 8-bit planes of one
   size: the pic_w x pic_h picture at d_src (row stride src_stride, planes
   src_plane_stride bytes apart) is copied into the plane_w x plane_h plane at
   d_dst and extended into the padding by the reference's [1 2 1]/4 low-pass
   recurrences (right side over the picture rows, then the bottom over the whole
   width).  plane_w = frame_width >> xdec, pic_w = (pic_width + xdec) >> xdec, and
   likewise for the heights; at most 64 padded columns / rows, sides up to 8192.
   pic_w == 0 or pic_h == 0 clears the plane (:764-770).
   dst_stride >= plane_w, dst_plane_stride >= dst_stride*plane_h, src_stride >= pic_w,
   src_plane_stride >= src_stride*pic_h (ODHIP_EINVAL otherwise); neither side has an
   alignment rule of its own (odd strides and bases are fine: 16-byte copies where both
   happen to be aligned, single samples elsewhere), but a destination meant for
   odhip_forward_pyramid has to follow its picture plane layout rules.  Nothing outside
   the plane_w x plane_h windows is written. */
int odhip_image_planes_copy_pad(uint8_t *d_dst, int dst_stride, long dst_plane_stride,
 int plane_w, int plane_h, const uint8_t *d_src, int src_stride, long src_plane_stride,
 int pic_w, int pic_h, int nplanes, odhip_stream stream);

/* ---- full-precision references ------------------------------------------------------
   An encoder created with daala_info.full_precision_references keeps its picture buffers
   as 16-bit samples at 8 + OD_COEFF_SHIFT = 12 bits (src/encode.c:212-213,
   src/state.c:256-258: xstride 2), which is how 10- and 12-bit video is coded and how an
   8-bit source keeps four more bits through prediction.  odhip_ctx_set_fpr(ctx, 1) puts a
   context in that mode: every PICTURE plane its calls take or produce - the `px` arguments
   of odhip_forward_pyramid, odhip_inverse_level(s), odhip_inverse_level(s)_pvq,
   odhip_inverse_levels_pvq_ref and odhip_inverse_partition, typed uint8_t * like the
   reference's daala_image_plane.data - then holds int16 samples, 8-byte aligned, with
   strides in SAMPLES: coefficient = p - 2048 on the way in (od_ref_buf_to_coeff,
   src/state.c:1238-1254), OD_CLAMPFPR(c + 2048) on the way out (od_coeff_to_ref_buf,
   :1306-1321).  Everything between (filters, transforms, PVQ) is the same arithmetic.
   odhip_image_planes_copy_pad16 is od_img_plane_copy_pad for such buffers: the copy step is
   od_img_plane_copy's bit-depth conversion (src/state.c:93-213; src_bitdepth 8: uint8_t
   samples, 10 / 12: int16_t samples, shifted up to 12 bits and clamped), the extension runs
   on the 16-bit samples (src/encode.c:791-803, :821-832); its strides count samples and obey the
   rules of odhip_image_planes_copy_pad. */
int odhip_ctx_set_fpr(odhip_ctx *ctx, int on);
int odhip_ctx_get_fpr(const odhip_ctx *ctx);
/* TEST HOOKS, per context (ctx == NULL: the calling thread's current context; nothing here
   is process-wide).  theta_margin: the distance from an integer inside which
   OD_THETA_SCALE*acos(corr) + .5 is not trusted to the device acos (default 1e-9; <= 0
   restores it); theta_perturb != 0: the device theta of a listed band is deliberately wrong
   (+1), so that tests exercise the host-libm re-run on real data; price_tol_scale multiplies
   the margin inside which a priced choice is left to the host libm (<= 0: 1).  A production
   caller never touches these. */
int odhip_ctx_set_test_hooks(odhip_ctx *ctx, double theta_margin, int theta_perturb,
 double price_tol_scale);
int odhip_image_planes_copy_pad16(uint16_t *d_dst, int dst_stride, long dst_plane_stride, int plane_w,
 int plane_h, const void *d_src, int src_bitdepth, int src_stride, long src_plane_stride, int pic_w,
 int pic_h, int nplanes, odhip_stream stream);

/* ---- frame cache: one batched pyramid serving every per-block fdct_2d call ---

   The samples a block of level bs sees in the reference encoder depend only on
   the source plane and on "every ancestor was split" (SURVEY.md section 7), so
   one odhip_forward_pyramid per plane yields the output of every fdct_2d call
   the encoder will make on that plane, in both RDO passes.

   odhip_cache_load_plane is called when the encoder has just converted plane
   `pli` to coefficients and is about to lap it across superblock edges
   (od_apply_prefilter_frame_sbs, src/encode.c:2571): `coef` must still hold
   (p - 128) << 4 (src/state.c:1233), stride == w.  odhip_cache_lookup serves an
   fdct_2d(out, out_stride, in, in_stride) whose `in` lies inside a loaded plane
   (returns 1) or reports a miss (returns 0).  odhip_install_cached_dct_vtbl
   installs fdct_2d entries that try the calling thread's current cache first
   and fall back to the per-call GPU transform (idct_2d entries are the per-call
   ones).  ODHIP_CACHE_CHECK=1 verifies every hit against the per-call path. */
typedef struct odhip_frame_cache odhip_frame_cache;
odhip_frame_cache *odhip_cache_create(void);
void odhip_cache_destroy(odhip_frame_cache *c);
void odhip_cache_set_picture(odhip_frame_cache *c, int pic_w, int pic_h);
void odhip_cache_make_current(odhip_frame_cache *c);
/* The 8-bit source samples of a loaded plane (host and device copies; valid until the slot is
   loaded again): the input of odhip_dering_cache_set_source. */
int odhip_cache_plane_pixels(const odhip_frame_cache *c, int pli, const uint8_t **h_px, const uint8_t **d_px,
 int *w, int *h);
int odhip_cache_load_plane(odhip_frame_cache *c, int pli, const od_coeff *coef,
 int stride, int w, int h, int dec);
int odhip_cache_lookup(odhip_frame_cache *c, const od_coeff *in, int in_stride,
 int bs, od_coeff *out, int out_stride);
void odhip_cache_stats(const odhip_frame_cache *c, long *hits, long *misses);
void odhip_install_cached_dct_vtbl(odhip_dct_func_2d fdct_2d[ODHIP_NBSIZES],
 odhip_dct_func_2d idct_2d[ODHIP_NBSIZES]);

/* ---- pricing on the device: od_pvq_rate's closed form (the
   speed > 0 half) --------------------------------------------------------------------

   od_pvq_rate (src/pvq_encoder.c:247-287) has two modes.  speed == 0 (the default
   complexity) runs the real codeword coder on a copy of the live adaptive context:
   sequential host state, not batchable.  speed > 0 - what the
   block-size RDO pass prices with below complexity 5, src/encode.c:1359 - is a closed
   form in (K, n, the centre of mass of the pulse vector, theta terms): a pure function of
   the candidate.  odhip_pvq_choose_priced_multi / odhip_pvq_ref_choose_priced_multi are
   odhip_pvq_choose_multi / odhip_pvq_ref_choose_multi with that rate evaluated ON THE
   DEVICE from the pulses the searches stored - no rate table, no candidate export.

   Its two libm calls (log) are not reproducible bit for bit on the device; the costs
   they enter are compared with each other, so a decision is taken from the device only
   when the two costs differ by more than 1e-10 of their magnitude (the two logs agree to
   ~1e-16).  A band with a closer decision is listed; *_priced_resolve (same jobs, same
   stream, after the *_priced_multi call) waits for the count of listed bands only -
   normally 0 - and otherwise recomputes those bands' rates with the HOST libm, the
   function the reference calls, and decides them again.  It returns the number of
   bands re-decided; consumers of the choice records enqueued before it must then be
   repeated.  (odhip_ctx_set_test_hooks can widen the margin to force this path.) */
int odhip_pvq_choose_priced_multi(const odhip_pvq_job *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream);
int odhip_pvq_choose_priced_resolve(const odhip_pvq_job *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream);
/* odhip_pvq_noref_bands_multi AND odhip_pvq_choose_priced_multi in one pass: every band is
   decided where its search ends, from the values held in registers; no choice kernel reads the
   records back.  What leaves the stage is what its consumers read: the choice record and the
   CHOSEN candidate's pulses (slot = choice[0]).  Every band is prepared, searched and
   decided by the lane (or lane pair) that loads its coefficients, in natural block order: no
   scaled vector, band record, sort key or sorted index exists in memory for it.  A losing
   candidate's pulses and the band record (gains, pulse counts, sums, distortions, moments) are
   written only for a band listed as a close call - the resolve decides it again from exactly
   those.  A host that wants both candidates of every band uses
   odhip_pvq_noref_bands_multi.  Follow with odhip_pvq_choose_priced_resolve. */
int odhip_pvq_noref_bands_priced_multi(const odhip_pvq_job *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream);
int odhip_pvq_ref_choose_priced_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream);
int odhip_pvq_ref_choose_priced_resolve(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream);
/* The same split as odhip_pvq_noref_bands_priced_multi: the band stage with the priced choice
   of the bands searched one per lane (15 and 8 coefficients: 77 % of the bands of a 4:2:0
   chroma plane) made INSIDE their search kernels, from the registers; then the choice
   kernels for the rest (32 and 128 coefficients) and the count of listed bands.  The
   candidate records are written as always (the theta-margin re-run and the price-margin
   resolve read them; after a theta-margin re-run use odhip_pvq_ref_choose_priced_multi, which
   decides every band from the records). */
int odhip_pvq_ref_bands_priced_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream);
int odhip_pvq_ref_choose_priced_rest_multi(const odhip_pvq_refjob *jobs, int njobs, double pvq_norm_lambda,
 odhip_stream stream);

/* ---- od_pvq_rate at the default complexity (speed == 0), batched on the host ----------

   At speed == 0 od_pvq_rate (src/pvq_encoder.c:247-287) prices a candidate by running
   od_encode_pvq_codeword on a scratch range coder against a COPY of the live adaptive
   od_pvq_codeword_ctx (:265-275): the price depends on every symbol coded before, which is
   sequential host state (SURVEY hard part 1) - but not on most of what that call moves.
   odhip_pvq_rate_batch prices all `ncand` candidates of one band against one snapshot of
   the live context with a rate-only range coder (range + bit count: all od_ec_enc_tell_frac
   reads) and copy-on-touch CDF rows: no allocation, no context copy, no output bytes; the
   doubles are the reference's bit for bit.  ctx: the live context itself (the layout below
   is the reference's struct, src/pvq.h:125-132; &adapt->pvq.pvq_codeword_ctx sits at offset
   0 of od_adapt_ctx); it is only read.  Candidate c: pulses y[c][0 .. n - (theta[c] != -1))
   (NULL allowed when k[c] == 0), k[c], gain index qg[c], theta[c] (-1: no reference),
   ts[c] = max_theta; n = band size, icgr, is_keyframe, pli as od_pvq_rate takes them.
   _batch16: the pulses as int16 (what the band stages export). */
typedef struct {
  int32_t pvq_adapt[2*ODHIP_NBSIZES*4];
  int32_t pvq_k1_increment;
  uint16_t pvq_k1_cdf[12][16];
  uint16_t pvq_split_cdf[14*7][8];
  int32_t pvq_split_increment;
} odhip_pvq_codeword_ctx;
int odhip_pvq_rate_batch(double *rate, const odhip_pvq_codeword_ctx *ctx, int ncand,
 const od_coeff *const *y, const int *k, const int *qg, const int *theta, const int *ts, int n, int icgr,
 int is_keyframe, int pli);
int odhip_pvq_rate_batch16(double *rate, const odhip_pvq_codeword_ctx *ctx, int ncand,
 const int16_t *const *y, const int *k, const int *qg, const int *theta, const int *ts, int n, int icgr,
 int is_keyframe, int pli);

/* ---- frame cache, second half: the batched band stage behind pvq_theta ------------

   odhip_cache_load_bands (after odhip_cache_load_plane(pli), same frame): the
   no-reference PVQ band stage of every block of every level of that plane in one
   set of launches on the pyramid still resident in HBM, with the quantiser set-up
   `qt` (the encoder's state.qm / pvq_qm_q4 / quantizer: odhip_quant_setup, or the
   caller copies its own tables into an odhip_quant); records and pulse vectors go
   to pinned host memory.

   odhip_cache_band serves ONE pvq_theta call of the encoder's block loop
   (src/pvq_encoder.c:333-641) whose reference vector r0 is null - the case in which
   pvq_theta runs exactly the no-reference candidates (:452 fails, :571-609): block
   (bx, by) of level bs (block units), band index `band`.  Returns 1 and fills *out
   (views into the cache, valid until the next load), or 0 (not loaded / out of
   range: the caller falls back to the reference's own pvq_theta).  x0 is optional:
   with ODHIP_CACHE_CHECK=1 the band the encoder presents is compared with the band
   the batch coded and a mismatch aborts.  The caller then does what stays on the
   host in the reference: per candidate s with flags[s] == 1, cost = dist[s] +
   lambda*od_pvq_rate(gain[s], 0, -1, 0, adapt, y[s], k[s], n, ...), `cost <=
   best_cost` starting from best_cost = dist0 (:417-421, :597-609), then skip rule,
   od_gain_expand and od_pvq_synthesis_partial (:611-633).  INTEGRATION.md section 7
   shows that glue; tests/interpose/interpose.c is its load-time form. */
typedef struct {
  int n;                 /* coefficients of the band                               */
  int32_t q;             /* the band's quantiser step and beta (Q12) the batch used:   */
  int32_t beta;          /* the caller checks them against its own pvq_theta arguments */
  int32_t cg;            /* companded gain of x, Q8                                */
  int32_t gain[2];       /* candidate gain index i (0 = slot unused)               */
  int32_t k[2];
  int32_t flags[2];      /* 1 = searched, 0 = pruned / unused, 2 = K out of range  */
  double dist0;          /* distortion of the null candidate                       */
  double dist[2];
  const int16_t *y[2];   /* signed pulses of the candidate, coding order, n values */
} odhip_band_cands;
int odhip_cache_load_bands(odhip_frame_cache *c, int pli, const odhip_quant *qt,
 double pvq_norm_lambda);
int odhip_cache_band(odhip_frame_cache *c, int pli, int bs, int bx, int by, int band,
 const od_coeff *x0, odhip_band_cands *out);
void odhip_cache_band_stats(const odhip_frame_cache *c, long *hits, long *misses);

/* ---- YUV4MPEG2 input (host; SURVEY.md 8(f) rank 4, input side) ---------------------

   The reference reads its input in examples/encoder_example.c:89-160, :190-400,
   :449-508.  odhip_y4m_open parses the stream header (W, H, F, I, C tags) of a
   progressive 8-bit 4:2:0 file (C420, C420jpeg, C420mpeg2, C420paldv or no C tag);
   anything else - 4:4:4, 4:2:2, 4:1:1, mono, 10..16-bit, interlaced - returns NULL with
   *err = ODHIP_EIMPL (ODHIP_EINVAL: unreadable / not a YUV4MPEG2 stream).
   odhip_y4m_open2 with flags = ODHIP_Y4M_ALLOW_444 also takes progressive 8-bit 4:4:4
   (C444; C444p10 / C444p12 / C444alpha stay refused) and reports the chroma
   decimation in *chroma_dec (1: 4:2:0, 0: 4:4:4; may be NULL); flags = 0 is
   odhip_y4m_open.  odhip_y4m_read reads one FRAME into tightly packed planes (luma
   w x h, chroma ((w + dec) >> dec) x ((h + dec) >> dec): what odhip_pipe_set_pictures
   takes, one picture at a time); returns 1, 0 at the end of the stream, a negative
   code on loss of framing or a short read. */
typedef struct odhip_y4m odhip_y4m;
#define ODHIP_Y4M_ALLOW_444 1
odhip_y4m *odhip_y4m_open(const char *path, int *pic_w, int *pic_h, int *fps_n, int *fps_d, int *err);
odhip_y4m *odhip_y4m_open2(const char *path, int flags, int *pic_w, int *pic_h, int *fps_n, int *fps_d,
 int *chroma_dec, int *err);
int odhip_y4m_read(odhip_y4m *y, uint8_t *luma, uint8_t *cb, uint8_t *cr);
/* Steps over one FRAME without reading it (frame-sharded input: a rank reads only the
   frames it owns); 1, 0 at the end of the stream, negative on loss of framing. */
int odhip_y4m_skip(odhip_y4m *y);
void odhip_y4m_close(odhip_y4m *y);

/* ---- odhip_pipe: the frame-batch step as one C call ------------------------------

   One step = one pass of the hot path over `frames` resident 4:2:0 pictures of
   pic_w x pic_h (coded size = both rounded up to 64, src/state.c:376-379): input
   padding, forward pyramid (every level), PVQ band stage of every block of every
   level (luma: no reference; chroma: WITH the chroma-from-luma reference produced
   inside the step from the luma choices when chroma_cfl != 0, as the reference codes
   keyframe chroma, src/encode.c:1680-1687; without reference otherwise), choice,
   dequantisation + inverse of every level.  The luma and the chroma chain run on the
   pipe's two streams, each in its own odhip_ctx, software-pipelined over steps (the
   luma chain of step i+1 overlaps the chroma chain of step i); `serial` (or
   ODHIP_PVQ_SERIAL=1) puts everything on one stream.  The pipe owns all device
   memory and both streams.  The quantiser tables are copied at creation;
   odhip_pipe_set_quants gives every picture of the batch a quantiser of its own.

   odhip_pipe_step enqueues one step and returns (asynchronous); odhip_pipe_flush
   settles the last step's device-acos margin check (see odhip_pvq_ref_resolve_*);
   odhip_pipe_sync waits for both streams.  odhip_pipe_stage runs ONE stage in order
   on the first stream (tests; the flow in which a host prices the candidates between
   the band stage and the choice); odhip_pipe_buffer hands out the device buffers
   (ODHIP_PIPE_BUF_RATE allocates the rate table of a (plane set, level) on first
   use, zero-filled, and from then on the choice of that level is
   cost = dist + lambda*rate: [B][nb][2] doubles without reference,
   [B][nb][ODHIP_PVQ_REF_SLOTS + 1] with - the d_rate layouts above);
   odhip_pipe_read / _write copy after odhip_pipe_sync.  odhip_pipe_record brackets
   every stage (and the dominant kernel of each band stage) with HIP events on the
   stream it is launched on; odhip_pipe_timings returns the average milliseconds and
   the count per stage, odhip_pipe_search_timings the bracketed search kernels
   (chroma = 0: k_search<128,2>; 1: k_refb_search_row<8,16>). */
typedef struct odhip_pipe odhip_pipe;
typedef struct {
  int device;
  int frames;
  int pic_w;
  int pic_h;
  int chroma_cfl;
  int serial;
  int price;                    /* 1: the choice prices every candidate with od_pvq_rate's
                                   closed form on the device (odhip_pvq_*choose_priced_*);
                                   0: on distortion alone, or with rate tables             */
  int fpr_bits;                 /* 0: 8-bit picture buffers.  8 / 10 / 12: full-precision
                                   references - the coded planes and the reconstructions are
                                   int16 samples at 12 bits (odhip_ctx_set_fpr on both
                                   contexts), the resident pictures are uint8_t (8) or int16
                                   (10, 12) samples of that depth */
  int inter;                    /* 1: an INTER frame - every plane goes through the with-reference
                                   stage (pvq_theta with is_keyframe = 0) against the pyramid of
                                   its prediction picture (odhip_pipe_set_reference_pictures: what
                                   motion compensation produced; the encoder's mctmp / mdtmp,
                                   src/encode.c:880-886, :1326-1360); chroma_cfl is ignored */
  int chroma_444;               /* 0: 4:2:0 (chroma planes (pic_w + 1)/2 x (pic_h + 1)/2 at
                                   4 levels, 4x4 .. 32x32; pic_w and pic_h even).  1: 4:4:4 -
                                   chroma planes pic_w x pic_h at all 5 levels, 4x4 .. 64x64,
                                   odd sizes accepted; the chroma-from-luma reference of chroma
                                   level bs is the decoded luma block of the SAME level and
                                   position (od_resample_luma_coeffs' copy branch,
                                   src/intra.c:95-108).  Composes with every other field. */
  double pvq_norm_lambda;       /* OD_PVQ_LAMBDA, src/pvq.h:49 */
  const odhip_quant *quant;     /* every picture's quantiser, until odhip_pipe_set_quants gives each
                                   picture its own (same use_masking / hvs_qm: the QM tables are per pipe) */
} odhip_pipe_config;
enum {
  ODHIP_PIPE_PAD_LUMA = 0, ODHIP_PIPE_PYRAMID_LUMA, ODHIP_PIPE_BANDS_LUMA, ODHIP_PIPE_CHOOSE_LUMA,
  ODHIP_PIPE_CFL_REFS, ODHIP_PIPE_INVERSE_LUMA, ODHIP_PIPE_PAD_CHROMA, ODHIP_PIPE_PYRAMID_CHROMA,
  ODHIP_PIPE_BANDS_CHROMA, ODHIP_PIPE_CHOOSE_CHROMA, ODHIP_PIPE_INVERSE_CHROMA, ODHIP_PIPE_NSTAGES
};
enum {
  ODHIP_PIPE_BUF_PIC = 0,   /* pictures: luma [F][pic_h][pic_w], chroma [2F][pic_h/2][pic_w/2]
                               (4:4:4: [2F][pic_h][pic_w]; all Cb, then all Cr)        */
  ODHIP_PIPE_BUF_PX,        /* padded planes                                           */
  ODHIP_PIPE_BUF_LEVEL,     /* coefficient planes of a pyramid level                   */
  ODHIP_PIPE_BUF_RECON,     /* reconstructed pixels of a partition level               */
  ODHIP_PIPE_BUF_BAND,      /* odhip_pvq_band / odhip_pvq_refband records              */
  ODHIP_PIPE_BUF_Y,         /* pulse vectors                                           */
  ODHIP_PIPE_BUF_CHOICE,    /* choice records                                          */
  ODHIP_PIPE_BUF_ITEMS,     /* with-reference candidates (3 planes of 16-byte vectors) */
  ODHIP_PIPE_BUF_REF,       /* inter mode: the prediction pyramid.  (Keyframe chroma takes
                               its chroma-from-luma reference in place from the luma
                               choices, odhip_pvq_refjob.luma: no plane exists)        */
  ODHIP_PIPE_BUF_RATE,      /* rate table (allocated on first request)                 */
  ODHIP_PIPE_BUF_PRED       /* inter mode: the coded-size prediction planes the prediction pyramid reads */
};
odhip_pipe *odhip_pipe_create(const odhip_pipe_config *cfg);
void odhip_pipe_destroy(odhip_pipe *p);
/* Levels of the chroma plane set: 4 (4:2:0) or 5 (chroma_444); ODHIP_EINVAL for NULL. */
int odhip_pipe_chroma_levels(const odhip_pipe *p);
int odhip_pipe_set_pictures(odhip_pipe *p, const uint8_t *luma, const uint8_t *chroma, int on_device);
/* A stream of pictures instead of resident ones: odhip_pipe_feed copies the pictures of
   the NEXT step from host memory (same layouts as odhip_pipe_set_pictures) into the pipe's
   back buffers on its own copy stream - behind the padding kernels (and, with
   odhip_pipe_set_motion_search on, the motion search) that may still read
   them, beside the steps already enqueued - and the next odhip_pipe_step codes them.
   Asynchronous for pinned host memory; the host buffers must stay untouched until
   odhip_pipe_sync (or any later odhip_pipe_feed of the same pipe followed by a sync).
     for (;;) { odhip_pipe_feed(p, next_luma, next_chroma); odhip_pipe_step(p); ... } */
int odhip_pipe_feed(odhip_pipe *p, const uint8_t *luma, const uint8_t *chroma);
/* ---- the decisions of a step in the form a host entropy coder reads them (export_kernels.hip) ----
   What od_pvq_encode hands to its entropy coder per band (src/pvq_encoder.c:874-979, the arguments of
   pvq_encode_partition): the coded gain index, theta and its range, K, the skip / no-reference flags and
   the pulse vector - K pulses over n positions, nearly all zero.  One SECTION per (plane set, level):
     records     odhip_export_record4 / odhip_export_record8 [blocks][bands] (record_bytes of the section)
     stream      uint16 words.  The words of a band are consecutive; the bands of one GROUP (the records
                 of blocks_per_group consecutive blocks: 128 / 32 / 8 / 4 / 4 for 4x4 ... 64x64) follow each
                 other in record order; group g starts at word group_base[g] of the section's stream (groups
                 are placed in the order their workgroups finish: placement varies from run to run, content
                 does not).
     word        bits 0-6 the position inside the band, bits 7-15 the signed pulse count (-255 .. 255); a
                 count of -256 is an escape - the next word holds the count as an int16.
   A band without words holds no pulse (skipped, null gain, or K = 0).  Header first: words written per
   section, and a flag per section that is set when a stream outgrew its capacity (as many words as the
   level has coefficients; never seen - the dense vectors remain readable through odhip_pipe_read). */
#define ODHIP_EXPORT_MAX_SECTIONS 16
/* `fn` of a record: bits 0-8 the words of this band in the stream (0 .. 256), bit 9 coded without reference
   (pvq_theta's noref), bits 10-11 skip (0, OD_PVQ_SKIP_ZERO 1, OD_PVQ_SKIP_COPY 2).  K is not exported: for a
   coded band it is the sum of the magnitudes of its words' counts. */
#define ODHIP_EXPORT_NWORDS(fn) ((fn) & 0x1ff)
#define ODHIP_EXPORT_NOREF(fn) ((fn) >> 9 & 1)
#define ODHIP_EXPORT_SKIP(fn) ((fn) >> 10 & 3)
typedef struct {
  int16_t qg;          /* the coded gain index; 0 = the null vector */
  uint16_t fn;
} odhip_export_record4;   /* sections coded without a reference (keyframe luma): 4 bytes */
typedef struct {
  int16_t qg;          /* the coded gain index: pvq_theta's return value (:636-637) */
  int16_t itheta;
  int16_t max_theta;
  uint16_t fn;
} odhip_export_record8;   /* sections coded against a reference: 8 bytes */
typedef struct {
  uint32_t total_words[ODHIP_EXPORT_MAX_SECTIONS];
  uint32_t overflow[ODHIP_EXPORT_MAX_SECTIONS];
} odhip_export_header;
typedef struct {
  int32_t bs;
  uint32_t ngroups;
  uint32_t cap_words;
  uint32_t blocks_per_group;
  uint32_t record_bytes;     /* 4: odhip_export_record4, 8: odhip_export_record8 */
  uint32_t pad;
  uint64_t nrecords;         /* blocks x bands */
  uint64_t records_off;      /* byte offsets from the start of the buffer, multiples of 16 */
  uint64_t group_base_off;   /* uint32 [ngroups] */
  uint64_t stream_off;
} odhip_export_section;
typedef struct {
  int32_t nsections;
  int32_t pad;
  uint64_t fixed_bytes;      /* header + records + group bases of every section (always shipped) */
  uint64_t total_bytes;      /* the whole buffer: fixed part + the streams at full capacity */
  odhip_export_section section[ODHIP_EXPORT_MAX_SECTIONS];
} odhip_export_layout;
int odhip_export_layout_make(odhip_export_layout *lay, int nsections, const long *nblocks, const int *bs,
 const int *with_ref);
int odhip_export_begin(void *d_buf, const odhip_export_layout *lay, odhip_stream stream);
int odhip_export_pack(void *d_buf, const odhip_export_layout *lay, int section, const int32_t *d_choice,
 const int16_t *d_y, long nblocks, int bs, int with_ref, odhip_stream stream);
/* sections first_section .. first_section + n - 1 in one launch per five (arrays of n device pointers / sizes) */
int odhip_export_pack_multi(void *d_buf, const odhip_export_layout *lay, int first_section, int n,
 const int32_t *const *d_choice, const int16_t *const *d_y, const long *nblocks, const int *bs, int with_ref,
 odhip_stream stream);
int odhip_export_ship(void *pinned_host, const void *d_buf, const odhip_export_layout *lay, odhip_stream stream);

/* The OUTPUT side of a streaming host (SURVEY hard part 5: "timed GPU-side incl. transfers"): every step leaves
   what a host entropy coder consumes - the record and the pulses of every band of every level, compacted as above
   - in pinned host memory, packed behind the stage that produced it and shipped on a third stream, overlapped with
   the rest of the step.  Sections: luma levels 0..4, then chroma levels 0..3 (0..4 with chroma_444: 10 sections,
   chroma 64x64 in odhip_export_record8 too).  Keyframe luma records are odhip_export_record4, keyframe chroma
   odhip_export_record8; inter steps code every plane against its prediction, so all 9 (10) sections of an inter
   step are odhip_export_record8, luma 64x64 included.  odhip_pipe_export_layout: the offsets;
   odhip_pipe_export_bytes: the size of one host buffer (= total_bytes; only the used part of every stream crosses
   the bus; 0: this pipe's mode does not export - only device-priced keyframe steps with chroma from luma and
   device-priced inter steps do).

   The streaming consumer sets a RING of n >= 2 such buffers (odhip_pipe_set_export_ring): step s, counted from
   that call, lands in slot s % n, in the format above (odhip_pipe_export_layout).  odhip_pipe_export_take hands out
   the oldest complete step not taken yet: 1 with *step, *buf (its slot) and *overflow (bit s set: the stream of
   section s outgrew its capacity, from the header the step ships); 0 when none is complete.  wait = 1 blocks for
   a step whose copies are enqueued - a step's streams leave behind its late resolve, i.e. inside the next
   odhip_pipe_step or odhip_pipe_flush (odhip_pipe_sync alone does not complete a step whose resolve is pending) -
   and returns 0 without blocking otherwise.  odhip_pipe_export_release gives the slot back; takes and releases go
   in step order (ODHIP_EINVAL otherwise).  odhip_pipe_step returns ODHIP_EBUSY, enqueuing nothing, while its slot
   still holds an unreleased step.  A band that a late resolve re-decides is packed again before its step is
   complete: odhip_pipe_export_stale stays 0.  take / release may run on one consumer thread while another
   thread steps the pipe.
     set_export_ring(p, bufs, 3);
     for (s = 0;; s++) {
       feed(p, ...); step(p);                               (ODHIP_EBUSY: release first)
       while (take(p, 0, &t, &buf, &ovf) == 1) { code(buf); release(p, t); }    (step s - 2, s - 1 while s runs)
     }
     flush(p); while (take(p, 1, &t, &buf, &ovf) == 1) { code(buf); release(p, t); }
   set_export_ring(p, NULL, 0) stops: it syncs the pipe and drops the steps nobody took.

   The single buffer (odhip_pipe_set_export) holds step i after the odhip_pipe_sync that follows it: reading it
   drains the pipe (step, flush, sync, read).  A band that the host-libm resolve of a keyframe step re-decides one
   step late (none on any content measured) is shipped again when that happens inside odhip_pipe_flush - step,
   flush, sync, read is exact - and counted by odhip_pipe_export_stale when it happens inside the next step, i.e.
   after the host read the buffer.  Inter steps are packed again as long as odhip_pipe_sync has not shipped them.
   set_export and set_export_ring exclude each other (ODHIP_EINVAL). */
size_t odhip_pipe_export_bytes(const odhip_pipe *p);
int odhip_pipe_export_layout(const odhip_pipe *p, odhip_export_layout *out);
long odhip_pipe_export_stale(const odhip_pipe *p);
int odhip_pipe_set_export(odhip_pipe *p, void *pinned_host);
int odhip_pipe_set_export_ring(odhip_pipe *p, void *const *pinned, int n);
int odhip_pipe_export_take(odhip_pipe *p, int wait, long *step, void **buf, uint32_t *overflow);
int odhip_pipe_export_release(odhip_pipe *p, long step);
/* Inter mode (odhip_pipe_config.inter): the prediction pictures of the batch, same layouts
   and depth as odhip_pipe_set_pictures. */
int odhip_pipe_set_reference_pictures(odhip_pipe *p, const uint8_t *luma, const uint8_t *chroma,
 int on_device);
/* Per-picture quantisers: picture f of every step enqueued from now on is coded with quants[f]
   (n == frames): luma plane f with its pvq_qm_q4[0], chroma plane f (Cb) with pvq_qm_q4[1] and
   chroma plane F + f (Cr) with pvq_qm_q4[2] - what a rate controller that picks
   quantizer / base_quantizer frame by frame (src/encode.c:2903-2940) gives a batch, or one picture
   replicated F times at F quantisers (a quality ladder).  NULL / n == 0 returns to the config's quant
   for every picture.  Every quants[f] must have the config quant's use_masking and hvs_qm (the QM
   tables and OD_PVQ_BETA rows are per pipe); quantizer and base_quantizer are free.  The tables are
   copied.  A step is coded entirely with the quantisers in force when odhip_pipe_step enqueued it,
   its chroma chain and late resolves included: no sync is needed between set_quants and step.
   ODHIP_EINVAL for n != frames, a NULL entry or a use_masking / hvs_qm that differs. */
int odhip_pipe_set_quants(odhip_pipe *p, const odhip_quant *const *quants, int n);
int odhip_pipe_step(odhip_pipe *p);
int odhip_pipe_flush(odhip_pipe *p);
int odhip_pipe_sync(odhip_pipe *p);       /* ODHIP_ERANGE: see ODHIP_PVQ_MAX_K - the steps since the last sync coded
                                             a band otherwise than the reference would */
long odhip_pipe_k_range(const odhip_pipe *p);      /* such bands over this pipe's syncs so far */
int odhip_pipe_stage(odhip_pipe *p, int stage, int parity);
/* parity: with chroma from luma the luma pulse vectors / choice records alternate between
   two sets from step to step (the chroma chain of step i reads them while the luma chain of
   step i + 1 writes the next); 0 / 1 selects one, -1 the set of the last odhip_pipe_step. */
int odhip_pipe_buffer(odhip_pipe *p, int what, int set, int level, int parity, void **d_ptr,
 size_t *bytes);
int odhip_pipe_read(odhip_pipe *p, void *host, const void *d_ptr, size_t bytes);
int odhip_pipe_write(odhip_pipe *p, void *d_ptr, const void *host, size_t bytes);
int odhip_pipe_record(odhip_pipe *p, int enable);
int odhip_pipe_timings(odhip_pipe *p, double avg_ms[ODHIP_PIPE_NSTAGES], int count[ODHIP_PIPE_NSTAGES]);
int odhip_pipe_search_timings(odhip_pipe *p, int chroma, float *ms, int max_n);
int odhip_pipe_time_pyramid(odhip_pipe *p, int n, double *avg_ms);
/* The practical HBM ceiling beside the 8 TB/s specification: a device-to-device copy of
   `bytes` (a multiple of 16; scratch owned by the call) in 16-byte vectors, n timed launches after a
   warm-up, (read + written) bytes per second in GB/s.  variant 0 / 1 / 2: 2 / 4 / 8 vectors in flight
   per lane. */
int odhip_copy_ceiling(size_t bytes, int n, int variant, double *gbs, odhip_stream stream);
/* One stage of the filter + DCT path (ODHIP_PIPE_PAD_*, _PYRAMID_*, _INVERSE_*) launched n times on
   the idle GPU over the buffers the last step left: average milliseconds per launch group (the
   roofline_* entries of bench.py).  parity as for odhip_pipe_stage, -1 = the last step's. */
int odhip_pipe_time_stage(odhip_pipe *p, int stage, int parity, int n, double *avg_ms);
long odhip_pipe_theta_reruns(const odhip_pipe *p);
/* ... and the bands that were listed (inside the acos margin, theta recomputed by the host), changed or not */
long odhip_pipe_theta_listed(odhip_pipe *p);
long odhip_pvq_ref_theta_listed(void);
long odhip_pipe_price_reruns(const odhip_pipe *p);
double odhip_pipe_host_wait_ms(const odhip_pipe *p);
/* odhip_ctx_set_test_hooks on both contexts of the pipe. */
int odhip_pipe_set_test_hooks(odhip_pipe *p, double theta_margin, int theta_perturb, double price_tol_scale);

/* ---- quality metrics: PSNR and PSNR-HVS-M on the device (metrics_kernels.hip) ----
   The two metrics the reference's RD tools report first (tools/dump_psnr.c, tools/dump_psnrhvs.c), over the
   picture region of source / reconstruction plane pairs at the source depth (8, 10, 12).
     SSE       the exact int64 sum of squared sample differences;
               PSNR = 10*(log10(max^2) + log10(npixels) - log10(sse)), max = (1 << depth) - 1
     HVS       the sum of calc_psnrhvs's per-window terms: 8x8 windows at step 7, every term the tool's
               float value bit for bit, summed in double in a fixed order (the tool keeps one running float,
               which no parallel order reproduces; results differ from it in the last bits of that float);
               PSNR-HVS-M = 10*(-log10(sum/(64*nwindows)/max^2))
   Sample formats: ODHIP_SAMPLE_U8 (uint8, depth 8), ODHIP_SAMPLE_U16 (uint16 at the depth), ODHIP_SAMPLE_I16_12
   (int16 at 12 bits - the full-precision planes of a pipe - brought to the depth by the reference's output
   conversion, OD_CLAMPI(0, (s + (1 << sh >> 1)) >> sh, (1 << depth) - 1), sh = 12 - depth, src/state.c:158-182).
   csf: the contrast sensitivity table - ODHIP_CSF_Y for luma, ODHIP_CSF_CB for the first chroma plane and
   ODHIP_CSF_CR for the second (the tool uses its 4:2:0 chroma tables for every chroma format). */
#define ODHIP_METRIC_SSE 1
#define ODHIP_METRIC_PSNRHVS 2
/* bit value 4, for odhip_pipe_set_metrics2 only: odhip_metrics_planes has no array for it and odhip_pipe_set_metrics
   keeps its two flags - both answer ODHIP_EINVAL, as they did for every unknown bit */
#define ODHIP_METRIC_SSIM (1 << 2)
/* bit value 8, for odhip_pipe_set_metrics3 only: the older entry points keep refusing it */
#define ODHIP_METRIC_MSSSIM (1 << 3)
/* bit value 16, for odhip_pipe_set_metrics4 only: the older entry points keep refusing it */
#define ODHIP_METRIC_FASTSSIM (1 << 4)
/* bit value 32, for odhip_pipe_set_metrics5 only: the older entry points keep refusing it */
#define ODHIP_METRIC_CIEDE (1 << 5)
#define ODHIP_SAMPLE_U8 0
#define ODHIP_SAMPLE_U16 1
#define ODHIP_SAMPLE_I16_12 2
#define ODHIP_CSF_Y 0
#define ODHIP_CSF_CB 1
#define ODHIP_CSF_CR 2
typedef struct {
  const void *src;          /* device pointers to sample (0, 0) of the picture region */
  const void *rec;
  int32_t src_fmt;          /* ODHIP_SAMPLE_* */
  int32_t rec_fmt;
  int32_t src_stride;       /* in samples */
  int32_t rec_stride;
  int32_t w;                /* the picture region */
  int32_t h;
  int32_t depth;            /* 8, 10, 12 */
  int32_t csf;              /* ODHIP_CSF_* */
} odhip_metrics_pair;
/* n pairs: sse[i] / hvs[i] (device arrays; the metrics `flags` asks for, the others untouched), npixels[i] and
   nwindows[i] (host, may be NULL) - asynchronous on `stream`.  Scratch of the current context. */
int odhip_metrics_planes(const odhip_metrics_pair *pairs, int n, int flags, int64_t *d_sse, double *d_hvs,
 long *npixels, long *nwindows, odhip_stream stream);
/* The current context's scratch, ahead of a first odhip_metrics_planes (which allocates it otherwise). */
int odhip_metrics_prepare(void);
/* Windows of a w x h region (*nwx across, *nwy down, either may be NULL). */
long odhip_psnrhvs_window_count(int w, int h, int *nwx, int *nwy);
/* Test surface: d_out[wy*nwx + wx] = the 64 terms of window (wx, wy) summed in float in (i, j) order. */
int odhip_psnrhvs_windows(const odhip_metrics_pair *pair, float *d_out, odhip_stream stream);

/* ---- SSIM on the device (k_ssim, metrics_kernels.hip), as the reference's tools/dump_ssim.c computes it ----
   calc_ssim (:79-189) of a w x h plane pair at depth 8, 10 or 12: an integer Gaussian of weight 256 runs along the
   rows and then down the columns over the moments mux, muy, x2, xy, y2 and the weight w; taps that fall outside the
   plane are dropped, never replaced.  Both tap tables follow the plane's own HEIGHT: sigma = h*(1.5/256) down the
   columns, sigma/par along the rows (par: the pixel aspect ratio, 1 unless the caller says otherwise), their length
   capped to 2*min(w, h) - 1; they are built on the host, by the host libm, exactly as gaussian_filter_init (:33-63)
   builds them, and handed to the kernel.  The moments are the mathematical integers (a horizontal one is below 2^32,
   a vertical one below 2^41): at 12 bits the tool's own `signed` products can overflow, so depth 12 has no tool
   yardstick.  Every sample then gives the term of :172-179 in double, one IEEE operation per C operation in the C
   expression's association, bit for bit the tool's.
     plane value = sum of the terms / sum of the weights
   The device returns the SUM OF THE TERMS, added in a fixed order (a lane's samples, a workgroup tree, the tile
   partials): it repeats bit for bit from run to run and lies within N*2^-53*sum|term| of the exact sum.  The tool
   keeps one running double over the plane, which no parallel order reproduces; results differ from it in the last
   bits of that double.  The sum of the weights is an exact integer that depends only on w, h and par: the host
   computes it (odhip_ssim_weight).  The tool's scores: sum/weight (-r), or 10*(log10(weight) - log10(weight - sum)).
   Radius: a 1080-row plane has 16 (33 taps), a 64-row plane 1.  The tiling takes a radius up to
   ODHIP_SSIM_MAX_RADIUS in either direction (heights up to 5000 and more; par < 1 widens the horizontal one);
   above it every entry point that would launch returns ODHIP_EIMPL before any launch. */
#define ODHIP_SSIM_MAX_RADIUS 64
/* Host only.  The tap table of gaussian_filter_init(sigma, max_len): returns the kernel size 2*len + 1 <= 2*max_len - 1
   and fills taps[0 .. size).  ODHIP_EINVAL: sigma <= 0, max_len < 1, taps NULL or cap < size. */
int odhip_ssim_taps(double sigma, int max_len, uint32_t *taps, int cap);
/* Host only.  *weight = the sum of the weight moment over a w x h plane (w, h <= 65535). */
int odhip_ssim_weight(int w, int h, double par, int64_t *weight);
/* n pairs (csf is not used): d_sum[i] (device) = the sum of pair i's terms, weights[i] (host, may be NULL) - asynchronous
   on `stream`.  Scratch of the current context: tile partials (grown when a launch needs more, which syncs the
   device - odhip_ssim_prepare does it ahead) and the tap tables of the (w, h, par) seen so far. */
int odhip_ssim_planes(const odhip_metrics_pair *pairs, int n, double par, double *d_sum, int64_t *weights,
 odhip_stream stream);
/* The current context's scratch for launches of up to `tiles` tiles (odhip_ssim_tile_count of each pair, summed over the
   up to 32 pairs of a launch). */
int odhip_ssim_prepare(long tiles);
long odhip_ssim_tile_count(int w, int h);
/* Test surface: d_terms[y*w + x] = the term of sample (x, y), raster order. */
int odhip_ssim_terms(const odhip_metrics_pair *pair, double par, double *d_terms, odhip_stream stream);

/* ---- MS-SSIM on the device (k_msssim, msssim_kernels.hip), as the reference's tools/dump_msssim.c computes it ----
   calc_msssim (:228-273) of a w x h plane pair at depth 8, 10 or 12 over ODHIP_MSSSIM_SCALES = 5 scales: scale 0 is
   the pair, scale i > 0 the 2x2 SUM (no division) of scale i - 1 at (w >> 1) x (h >> 1), an odd last row or column
   dropped, and max - (1 << depth) - 1 at scale 0 - times 4 (k_msssim_pyramid writes scales 1..4 as int32).  At every
   scale calc_ssim (:88-195) runs the nine taps of gaussian_filter_init(1.5, 5) at weight 1024 - 8 37 112 218 274 218
   112 37 8, a compile-time table in the kernel, rebuilt by the host libm in odhip_msssim_taps - along the rows and
   down the columns over the moments mux, muy, x2, xy, y2 and the weight w; taps that fall outside the plane are
   dropped, never replaced.  The moments are the mathematical integers in int64 (below 2^61 at 12 bits and scale 4;
   above 2^53 they enter the terms through an int64 -> double conversion, which rounds to nearest).  Every sample
   gives the two terms of :175-184, cs and ssim, in double, one IEEE operation per C operation in the C expressions'
   association, bit for bit the tool's.
     score = pow(cs0, .0448) * pow(cs1, .2856) * pow(cs2, .3001) * pow(cs3, .2363) * pow(ssim4, .1333),
     cs_i = sum of scale i's cs terms / sum of its weights, ssim4 likewise of scale 4's ssim terms
   The device returns the FIVE SUMS, each added in a fixed order (a lane's samples, a workgroup tree, the tile
   partials): they repeat bit for bit from run to run and lie within N*2^-53*sum|term| of the exact sums.  The tool
   keeps running doubles over a plane, which no parallel order reproduces; results differ from it in the last bits.
   The sums of the weights are exact integers of the size alone: the host computes them (odhip_msssim_weights).  The
   tool prints score (-r) or 10*(log10(1) - log10(1 - score)); a negative cs makes it print NAN, and so does
   odhip_msssim_score.  The reference's Y4M reader takes 8 and 10 bits only: depth 12 has the restatement
   (tests/_msssim_ref.py) as its only yardstick.  Scale 4 of a 16 x 16 plane is 1 x 1; below ODHIP_MSSSIM_MIN_SIZE in
   either direction the tool divides 0 by 0, so every entry point answers ODHIP_EINVAL before any launch. */
#define ODHIP_MSSSIM_SCALES 5
#define ODHIP_MSSSIM_MIN_SIZE 16
/* Host only.  The nine taps as gaussian_filter_init(1.5, 5) builds them at weight 1024, by the host libm, compared
   with the table the kernels were compiled with: ODHIP_EIMPL if they differ (taps[] is filled all the same). */
int odhip_msssim_taps(uint32_t taps[9]);
/* Host only.  weight[i] = the sum of the weight moment over scale i of a w x h plane (16 <= w, h <= 65535). */
int odhip_msssim_weights(int w, int h, int64_t weight[5]);
/* n pairs (csf is not used; w, h >= 16): d_sums[i][0..3] (device) = the sums of the cs terms of scales 0..3 of pair i,
   d_sums[i][4] = the sum of the ssim terms of scale 4; weights[i][5] (host, may be NULL) - asynchronous on `stream`.
   ODHIP_EINVAL before any launch: a NULL array, n < 0, a pair below 16 or above 65535 in either direction or at a depth
   other than 8 / 10 / 12; n == 0 succeeds.  Pairs go in launch groups of up to 32; pairs with the same source plane
   (pointer, format, stride, size, depth) share its pyramid, built once per call while they fit one group.  Scratch of
   the current context: the pyramids and tile partials of one group (grown when a group needs more, which waits for
   the stream - odhip_msssim_prepare does it ahead). */
int odhip_msssim_planes(const odhip_metrics_pair *pairs, int n, double *d_sums, int64_t *weights, odhip_stream stream);
/* The current context's scratch for launch groups of up to `pairs` (at most 32 count) pairs of w x h. */
int odhip_msssim_prepare(int w, int h, int pairs);
/* Host only.  *score = the tool's product of the five sums and weights, by the host libm's pow. */
int odhip_msssim_score(const double sums[5], const int64_t weight[5], double *score);
/* Test surface: d_cs[y*ws + x], d_ssim[y*ws + x] = both terms of sample (x, y) of scale `scale` (0..4), whose size is
   ws x hs = (w >> scale) x (h >> scale), raster order. */
int odhip_msssim_terms(const odhip_metrics_pair *pair, int scale, double *d_cs, double *d_ssim, odhip_stream stream);

/* ---- FastSSIM on the device (k_fastssim, fastssim_kernels.hip), as the reference's tools/dump_fastssim.c computes it ----
   calc_ssim (:445-463) of a w x h plane pair at depth 8, 10 or 12 over ODHIP_FASTSSIM_LEVELS = 4 levels.  Level 0 is
   the 2x2 SUM (no division) of the pair at ceil(w/2) x ceil(h/2), a missing right or bottom neighbour replaced by the
   last sample (fs_downsample_level0); level l > 0 is the 2x2 sum of level l - 1, again at the rounded-up size, and max
   - (1 << depth) - 1 times 4 at level 0 - times 4 again (k_fastssim_pyramid writes all four as int32: max 4^4 is
   below 2^20 at 12 bits).
   A DEFECT OF THE TOOL THAT IS NOT COPIED: fs_downsample_level clamps the neighbour with FS_MINI(i0 + 1, w2) and
   FS_MINI(2*j + 1, h2), where w2 - 1 and h2 - 1 are the last column and row.  When the level it reads has an odd
   width it takes the first sample of the next row; when it has an odd height it reads one row past the level - for the
   first plane that is the second plane's first row, for the second the bytes of an array of doubles.  1920 x 1080 is
   such a size (540 -> 270 -> 135 rows): the tool's own 1080p numbers contain that row.  The library defines levels
   1..3 with the clamp level 0 uses (last row, last column) and equals the tool for exactly the sizes where the tool's
   reads stay inside the level: levels 0, 1 and 2 even in both directions, i.e. ceil(w/2) and ceil(h/2) multiples of 8
   (odhip_fastssim_tool_exact; 1920 x 1088 is one).
   Every level (fs_calc_structure): gradient magnitudes g = 4 max(g1, g2) + min(g1, g2), g1 = |s[j+1][i+1] - s[j][i]|,
   g2 = |s[j+1][i] - s[j][i+1]|, on the (w_l - 1) x (h_l - 1) interior and zero outside; the three sums of gx^2, gy^2
   and gx gy under a fixed 8 x 8 integer window of total weight 104 - the tool's sliding scheme of doubling, halving
   and subtracting columns over an 8-row ring buffer IS that window, truncated only by the zeros at the borders: an
   impulse at gradient position (y, x) lands on output rows y - 4 .. y + 3 and columns x - 3 .. x + 4 with the weights
     1 2 4 8 8 4 2 1 / 1 2 4 8 8 4 2 1 / 0 1 2 4 4 2 1 0 / 0 0 1 2 2 1 0 0 /
     0 0 0 1 1 0 0 0 / 0 0 0 1 1 0 0 0 / 0 0 1 2 2 1 0 0 / 0 1 2 4 4 2 1 0
   (the ring buffer's row rotation, not a centred window) - and the term (2 mugxgy + c2)/(mugx2 + mugy2 + c2),
   c2 = max^2 * 0.0009 * 16^l * 16 * 104 evaluated on the host in the tool's association.  With samples within the
   depth (ODHIP_SAMPLE_U16 planes are read as they are, not clamped) g <= 5 * 4095 * 256 < 2^22.33, so 104 g^2 <
   2^51.36 < 2^52: the sums are mathematical integers, accumulated in int64 and converted once,
   and the tool's doubles (its halved intermediates included) are exact too, so any summation order gives its values.
   Level 3 only (fs_apply_luminance): the term is multiplied by (2 mux muy + c1)/(mux^2 + muy^2 + c1) over 8 x 8 BOX
   sums (rows j - 4 .. j + 3, columns i - 4 .. i + 3, coordinates clamped to the level) held in `unsigned`, modulo
   2^32.  The tool slides muy along a row with x's column sums (:243-244), in bounds and deterministic, so it is
   reproduced: muy(j, i) = muy(j, 0) + mux(j, i) - mux(j, 0) modulo 2^32, which wraps whenever x darkens along a row
   by more than muy(j, 0).  2*mux is an unsigned product, everything else one IEEE operation per C operation.
     score = product over l of pow(sum of level l's terms / (w_l h_l), FS_WEIGHTS[l]), from 1 in level order
   The device returns the FOUR SUMS, each added in a fixed order (a lane's samples, a workgroup tree, the tile
   partials): they repeat bit for bit from run to run and lie within N*2^-53*sum|term| of the exact sums.  The tool
   keeps one running double per level, which no parallel order reproduces; results differ from it in the last bits.
   Every per-sample term is the tool's bit for bit (tests/_fastssim_ref.py restates them and reproduces the tool's
   printed lines and return values).  The reference's Y4M reader takes 8 and 10 bits only: depth 12, and sizes outside
   odhip_fastssim_tool_exact, have the restatement as their only yardstick.  Sizes from 16 x 16 (level 3 is 1 x 1) to
   65535 in either direction; anything else is ODHIP_EINVAL before any launch. */
#define ODHIP_FASTSSIM_LEVELS 4
/* Host only.  *wl x *hl = the size of level `level` (0..3) of a w x h plane. */
int odhip_fastssim_level_size(int w, int h, int level, int *wl, int *hl);
/* Host only.  1 where the tool's downsampling reads stay inside the level they read, so that the library equals the
   tool; 0 where the tool reads a foreign sample or row (see above); ODHIP_EINVAL for a size the library does not take. */
int odhip_fastssim_tool_exact(int w, int h);
/* n pairs (csf is not used; w, h >= 16): d_sums[i][l] (device) = the sum of the terms of level l of pair i -
   asynchronous on `stream`.  ODHIP_EINVAL before any launch: a NULL array, n < 0, a pair below 16 or above 65535 in
   either direction or at a depth other than 8 / 10 / 12; n == 0 succeeds.  Pairs go in launch groups of up to 32; pairs
   with the same source plane (pointer, format, stride, size, depth) share its pyramid, built once per call while they
   fit one group.  Scratch of the current context: the pyramids and tile partials of one group (grown when a group
   needs more, which waits for the stream - odhip_fastssim_prepare does it ahead). */
int odhip_fastssim_planes(const odhip_metrics_pair *pairs, int n, double *d_sums, odhip_stream stream);
/* The current context's scratch for launch groups of up to `pairs` (at most 32 count) pairs of w x h. */
int odhip_fastssim_prepare(int w, int h, int pairs);
/* Host only.  *score = the tool's product of the four sums of a w x h plane, by the host libm's pow. */
int odhip_fastssim_score(const double sums[4], int w, int h, double *score);
/* Test surface: d_terms[y*wl + x] = the term of sample (x, y) of level `level` (0..3), raster order; at level 3 the
   product of the structure and the luminance term. */
int odhip_fastssim_terms(const odhip_metrics_pair *pair, int level, double *d_terms, odhip_stream stream);

/* ---- CIEDE2000 on the device (k_ciede, ciede_kernels.hip), as the reference's tools/dump_ciede2000.py computes it ----
   The colour difference of a whole picture pair - Y, Cb and Cr meet in one term - at depth d = 8, 10 or 12 (the tool
   reads 8 and 10; 12 is the same formula), s = 2^(d - 8), 4:4:4 or 4:2:0, where chroma sample (x >> 1, y >> 1)
   serves pixel (x, y) (the tool's np.kron box).  Everything is IEEE binary64, one operation per operation below in
   the order written (-ffp-contract=off), so that only pow, cbrt, atan2, sin, cos, exp and sqrt can differ from a host:
     Y' = (Y - 16s)/(219s), Cb' = (Cb - 128s)/(224s), Cr' likewise;
     R = Y' + 1.28033 Cr', G = (Y' - 0.21482 Cb') - 0.38059 Cr', B = Y' + 2.12798 Cb' (BT.709, unclipped);
     linear c = pow((c + 0.055)/1.055, 2.4) where c > 0.04045, else c/12.92 (negative values included);
     X = (0.412453 r + 0.357580 g) + 0.180423 b, Y and Z likewise with 0.212671 0.715160 0.072169 and 0.019334
     0.119193 0.950227; x = X/0.95047, y = Y/1.0, z = Z/1.08883;
     f(t) = cbrt(t) where t > 0.008856, else 7.787 t + 16/116; L = 116 f(y) - 16, a = 500 (f(x) - f(y)),
     b = 200 (f(y) - f(z));
     dE00 of source (L1, a1, b1) and reconstruction (L2, a2, b2) in the standard formulation (Sharma, Wu, Dalal
     2005) with kL = 0.65, kC = 1, kH = 4 (the tool's, after Yang, Ming, Yu 2012); seventh powers are products
     ((c^2)^2 c^2 c), hues are degrees, atan2 times 180/pi brought into [0, 360), and an angle enters sin or cos
     times pi/180; the radicand of the last root is clamped at 0.
   DEPARTURES FROM THE TOOL: the tool is a Python script over scikit-image, whose order of operations is whatever its
   numpy expressions give; here it is fixed as above (tests/_ciede_ref.py restates it and reproduces the published
   table of Sharma et al.).  Negative XYZ are NOT clipped: newer scikit-image releases clip Z < 0 to 0 with a
   warning, this definition does not.  Depth 12 is an extension.
   dE00 is discontinuous where the two hues are 180 degrees apart.  Whether |h2' - h1'| exceeds 180 is decided by the
   sign of the cross product a1' b2 - b1 a2' (with |h2' - h1'| beyond 90), which is the same comparison in exact
   arithmetic and, unlike the rounded difference of two atan2 results, exact for exactly opposite hues: (a, b) against
   (-a, -b) is "not above 180", as two rows of the published table require.  Elsewhere within the last bits of the jump
   the side is the rounding's - grey pixels on either side of Y = 16 s sit there, at a chroma so small that both sides
   agree to ~1e-13.
   The device returns SUM dE00 over the w x h pixels, added in a fixed order (a lane's 2 x 2 pixels, a workgroup tree,
   the tile partials): it repeats bit for bit and lies within N*2^-53*sum|term| of the exact sum.  Identical
   pictures give exactly 0.  score = 45 - 20 log10(sum/(w h)) (odhip_ciede_score, host libm; +infinity at sum 0, as
   the tool prints); the tool's Total is the mean of the per-frame scores, the caller's job. */
typedef struct {
  const void *src[3];       /* device pointers to sample (0, 0) of Y, Cb, Cr */
  const void *rec[3];
  int32_t src_fmt;          /* ODHIP_SAMPLE_*, of all three planes of a side */
  int32_t rec_fmt;
  int32_t src_stride;       /* luma, in samples */
  int32_t src_cstride;      /* chroma, in samples */
  int32_t rec_stride;
  int32_t rec_cstride;
  int32_t w;                /* the picture, in luma samples */
  int32_t h;
  int32_t depth;            /* 8, 10, 12 */
  int32_t cdec;             /* 0: 4:4:4, 1: 4:2:0 (chroma planes (w/2) x (h/2), w and h even) */
} odhip_ciede_pair;
/* n pairs: d_sum[i] (device) = SUM dE00 of pair i - asynchronous on `stream`.  ODHIP_EINVAL before any launch or
   allocation: a NULL pointer, n < 1, w or h < 1 or above 65535, odd w or h at cdec == 1, a stride below the plane's
   width, a depth other than 8 / 10 / 12, an unknown format or ODHIP_SAMPLE_U8 at another depth than 8, cdec outside
   0..1.  Pairs go in launch groups of up to 32; neighbouring pairs of a group with the same source picture (the
   levels of a pipe step) share its Lab values, computed once per tile.  Scratch of the current context: the tile
   partials of one group (grown when a group needs more, which waits for the stream - odhip_ciede_prepare does it
   ahead). */
int odhip_ciede_pictures(const odhip_ciede_pair *pairs, int n, double *d_sum, odhip_stream stream);
/* The current context's scratch for launch groups of up to `pairs` (at most 32 count) pairs of w x h. */
int odhip_ciede_prepare(int w, int h, int pairs);
/* Host only.  *score = 45 - 20 log10(sum/(w h)) by the host libm; +infinity for sum == 0. */
int odhip_ciede_score(double sum, int w, int h, double *score);
/* Test surface: d_terms[y*w + x] = dE00 of pixel (x, y), raster order. */
int odhip_ciede_terms(const odhip_ciede_pair *pair, double *d_terms, odhip_stream stream);
/* Test surface: d_out[i] = dE00 of the Lab triples d_lab1[3i .. 3i + 2] and d_lab2[3i .. 3i + 2] (device arrays of
   doubles) with the given kL, kC, kH, through the __device__ function k_ciede calls (k_ciede_lab); n >= 1. */
int odhip_ciede_lab_terms(const double *d_lab1, const double *d_lab2, long n, double kL, double kC, double kH,
 double *d_out, odhip_stream stream);

/* ---- the metrics of every pipe step ----
   odhip_pipe_set_metrics(p, flags, depth): from the next step on, every step measures every picture, plane and
   partition level against its source - luma behind the luma inverse, chroma behind the chroma inverse, on the
   chain that produced the reconstruction, so a late resolve that runs the inverse again measures again - and
   leaves the values in an internal ring of `depth` >= 2 pinned slots.  A step's slot completes where its export
   would: at once (chroma without reference), or behind its late resolve inside the next odhip_pipe_step or
   odhip_pipe_flush (chroma from luma, inter).  odhip_pipe_metrics_take copies out the oldest complete step: 1
   with *step (counted from set_metrics) and the values, 0 when none is complete (wait = 1 blocks only for a
   step whose copy is enqueued).  Taking frees the slot; odhip_pipe_step returns ODHIP_EBUSY, enqueuing nothing,
   while its slot holds an untaken step.  Arrays [set][level][plane]: luma [5][F], then chroma [nlev][2F] (all
   Cb planes, then all Cr), odhip_pipe_metrics_layout.values entries; NULL skips one.  flags 0 (the default):
   nothing is allocated or launched.  set_metrics syncs the pipe and drops the steps nobody took.  The source is
   the chain's padded plane, whose picture region is the source (shifted up to 12 bits with fpr_bits: brought
   back exactly); the depth is 8, or fpr_bits.
   A slot holds the columns of this table that `flags` asks for, in this order, a column `values` 8-byte entries; the
   others keep their places in front of a new one.  With its bit clear nothing of a column is allocated, launched or
   waited for, and a take leaves its array untouched.  Every odhip_pipe_set_metricsN is one call that accepts the bits
   down to its row (any other bit: ODHIP_EINVAL, so a caller never gets a column it has no array for), and every
   odhip_pipe_metrics_takeN one call that returns the columns down to its row, the sums of every [set][level][plane];
   the older ones stay.  A set_metrics that refuses leaves the metrics as they were.
     bit                    columns                          accepted / returned    set_metrics refuses
     ODHIP_METRIC_SSE       sse[values], always there        set_metrics / take
     ODHIP_METRIC_PSNRHVS   hvs[values], always there        set_metrics / take
     ODHIP_METRIC_SSIM      ssim[values]: the terms at       set_metrics2 / take2   ODHIP_EIMPL: a picture whose radius
                            par = 1                                                 exceeds ODHIP_SSIM_MAX_RADIUS
     ODHIP_METRIC_MSSSIM    msssim[values][5]                set_metrics3 / take3   ODHIP_EINVAL: a plane set below
                                                                                    ODHIP_MSSSIM_MIN_SIZE in either
                                                                                    direction (4:2:0 chroma of 64 x 24)
     ODHIP_METRIC_FASTSSIM  fastssim[values][4]              set_metrics4 / take4   ODHIP_EINVAL: a plane set below 16
                                                                                    in either direction
     ODHIP_METRIC_CIEDE     one; its first 5F entries are    set_metrics5 / take5
                            ciede[5][F], take5's ciede[5F]
   The scores: odhip_pipe_metrics_ssim_weights gives the weight and odhip_pipe_metrics_msssim_weights the five weights
   of a plane of each set, [0] luma, [1] chroma; odhip_fastssim_score with the plane's size and odhip_ciede_score with
   the picture's give the tools' scores.  k_ssim and k_msssim_pyramid / k_msssim run where k_metrics does, and
   k_fastssim_pyramid / k_fastssim behind the other metrics, so a late resolve measures them again too; MS-SSIM and
   FastSSIM take one odhip_msssim_planes / odhip_fastssim_planes call per plane set, so the source pyramid of a plane
   is built once per step for all its levels.
   ciede is SUM dE00 (odhip_ciede_pictures) of every picture and luma level, odhip_pipe_metrics_ciede_values entries;
   odhip_pipe_metrics_layout does not change with it.  Luma level l pairs with chroma level max(l - 1, 0) at 4:2:0 -
   the block size chroma is coded at under a luma block of that size - and with chroma level l at 4:4:4.  It is the one
   metric that reads both plane sets, so it is measured ONCE per step, on the chroma chain's stream, behind every late
   resolve of the step on either plane set and immediately before the step's slot is copied out: at once where no late
   resolve can come, otherwise inside the next odhip_pipe_step or odhip_pipe_flush.  The luma chain of the next step
   overwrites the luma source plane and the single-buffered luma reconstructions: while the bit is set it starts behind
   an event recorded after the measurement, so the luma chain of step i + 1 no longer overlaps the chroma chain of
   step i.  No sync, no stream is added, and with the bit clear a step is enqueued exactly as before. */
typedef struct {
  int32_t luma_levels;      /* 5 */
  int32_t chroma_levels;    /* 4 (4:2:0) or 5 (4:4:4) */
  int32_t luma_planes;      /* F */
  int32_t chroma_planes;    /* 2F */
  int32_t values;           /* 5F + chroma_levels*2F */
  int32_t depth;            /* the sample depth measured at */
  int32_t flags;            /* ODHIP_METRIC_* in force */
  int32_t slots;            /* ring depth */
} odhip_pipe_metrics_info;
int odhip_pipe_set_metrics(odhip_pipe *p, int flags, int depth);
int odhip_pipe_set_metrics2(odhip_pipe *p, int flags, int depth);
int odhip_pipe_set_metrics3(odhip_pipe *p, int flags, int depth);
int odhip_pipe_set_metrics4(odhip_pipe *p, int flags, int depth);
int odhip_pipe_set_metrics5(odhip_pipe *p, int flags, int depth);
int odhip_pipe_metrics_take(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs);
int odhip_pipe_metrics_take2(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs, double *ssim);
int odhip_pipe_metrics_take3(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs, double *ssim,
 double *msssim);
int odhip_pipe_metrics_take4(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs, double *ssim,
 double *msssim, double *fastssim);
int odhip_pipe_metrics_take5(odhip_pipe *p, int wait, long *step, int64_t *sse, double *hvs, double *ssim,
 double *msssim, double *fastssim, double *ciede);
/* Entries of take5's ciede array: 5F. */
int odhip_pipe_metrics_ciede_values(const odhip_pipe *p);
int odhip_pipe_metrics_ssim_weights(const odhip_pipe *p, int64_t weight[2]);
int odhip_pipe_metrics_msssim_weights(const odhip_pipe *p, int64_t weight[2][5]);
int odhip_pipe_metrics_layout(const odhip_pipe *p, odhip_pipe_metrics_info *out);
/* Per plane of each set [0] luma, [1] chroma: picture samples and PSNR-HVS-M windows. */
int odhip_pipe_metrics_counts(const odhip_pipe *p, long npixels[2], long nwindows[2]);

/* ---- motion compensation from motion-vector grids (mc_kernels.hip) ----
   The prediction od_state_mc_predict builds (src/state.c:932-959), given the vectors, as the decoder has them:
   overlapped-block motion compensation over the grid's quadtree, bit-exact.  The vectors come from the caller, or from
   the block-matching search below (odhip_me_search).
   A grid has a point every 8 luma pixels: [picture][coded_h/8 + 1][coded_w/8 + 1], coded size = the picture
   rounded up to 64.  A point carries its vector in 1/8 luma pel (the caller resolves the reference's mv / mv1
   by the frame the point refers to), the `valid` flag that drives the quadtree, and the slot of the reference
   plane set it points into.  A chroma plane set uses the same grid with dec = 1: vectors and leaves shrink.
   Reference planes are UNPADDED coded-size planes (8-bit, or int16 at 12 bits: ODHIP_SAMPLE_U8 /
   ODHIP_SAMPLE_I16_12); reads beyond them take the nearest edge sample, which equals the border of 64 luma
   samples the reference replicates round its frames.  A vector whose 6-tap window would leave that border is
   outside the reference's defined behaviour: ODHIP_ERANGE from the host-side check, nothing launched. */
typedef struct {
  int32_t mvx;              /* 1/8 luma pel */
  int32_t mvy;
  uint8_t valid;
  uint8_t ref;              /* slot: index into odhip_mc_job.ref */
  uint16_t reserved;
} odhip_mv_point;
typedef struct {
  int32_t coded_w;          /* luma coded size: multiples of 64 */
  int32_t coded_h;
  int32_t dec;              /* 0, or 1 for 4:2:0 chroma: planes are (coded_w >> dec) x (coded_h >> dec) */
  int32_t sample;           /* ODHIP_SAMPLE_U8 or ODHIP_SAMPLE_I16_12, references and destination alike */
  int32_t npics;            /* F grids */
  int32_t nplanes;          /* planes of a set, a multiple of F: plane p is predicted from grid p % F */
  int32_t nrefs;            /* 1..3 reference plane sets */
  int32_t grid_on_device;   /* the grid is device memory the caller has checked (odhip_mc_check_grid) */
  int32_t ref_stride;       /* in samples, >= the plane width; no alignment rule (odd strides and bases are fine) */
  int32_t dst_stride;
  int64_t ref_plane_stride; /* in samples, between the planes of a set: >= stride * plane rows (ODHIP_EINVAL otherwise) */
  int64_t dst_plane_stride;
  const void *ref[3];       /* device: [nplanes] planes per slot */
  void *dst;                /* device: [nplanes] planes, every sample of the coded size is written */
  const odhip_mv_point *grid;
} odhip_mc_job;
/* Asynchronous on `stream`; a host grid is checked, then copied on the stream.  Scratch of the current context. */
int odhip_mc_predict_planes(const odhip_mc_job *job, odhip_stream stream);
/* The host-side check of a host grid: ODHIP_EINVAL (a corner's slot >= nrefs), ODHIP_ERANGE, or 0. */
int odhip_mc_check_grid(const odhip_mv_point *grid, int coded_w, int coded_h, int npics, int dec, int nrefs);
/* Test surface: the leaves the device walk finds in a host grid, per picture sorted ascending in out[pic*cap ..],
   counts[pic] of them: vx | vy << 12 | log2(size/8) << 24 | outside corner << 26 | split flags << 28. */
int odhip_mc_leaves(const odhip_mv_point *grid, int coded_w, int coded_h, int npics, uint32_t *out, int *counts,
 int cap);
/* sizeof of 0: odhip_mv_point, 1: odhip_mc_job (for language bindings). */
size_t odhip_mc_sizeof(int what);
/* The current context's scratch for grids of this size, ahead of a first call (which allocates - and, when a later
   call needs more, frees and allocates again, which syncs the device - otherwise). */
int odhip_mc_prepare(int coded_w, int coded_h, int npics);

/* ---- motion search: grids by exhaustive block matching (me_kernels.hip) ----
   8-bit luma only.  The output is a uniform grid in the layout above: spacing B = 8 << log_size luma pixels, a
   point (vx, vy) valid iff vx and vy are multiples of 1 << log_size, every other point all zero; every point of
   the buffer is written.  The block of a point is the B x B square centred on it (src/mcenc.c:2589-2611), top
   left (8 vx - B/2, 8 vy - B/2).
   Cost of a candidate (slot r, vector (mvx, mvy) in 1/8 luma pel): the prediction is od_mc_predict1fmv8_c of plane
   r at that block and vector (reads beyond the unpadded coded-size plane by clamped coordinates, as in
   odhip_mc_predict_planes); SAD is od_enc_sad of it against the source picture: the block is clipped to
   [0, pic_w) x [0, pic_h) and only the surviving samples are summed (src/mcenc.c:2224-2264, 1615-1679); a block
   with nothing left has SAD 0.  cost = 8 SAD + lambda (|mvx| + |mvy|).
   A vector is legal for a point when the grid that holds it passes odhip_mc_check_grid at dec = 0 and dec = 1:
   every leaf of size B inside the coded frame with that point as a corner keeps its (blk + 5)-wide filter window
   inside the 64-sample border.  Illegal candidates are never evaluated; the zero vector is always legal.
   Stage 1: all (dx, dy) with |dx|, |dy| <= range in all nrefs slots at mv = (8 dx, 8 dy); the winner is the smallest
   key (cost, |mvx| + |mvy|, slot, mvy, mvx), compared lexicographically - a total order.
   Stage 2: res 0: 1/8 pel, 1: 1/4, 2: 1/2, 3: none.  For step = 4, 2, 1 eighth-pels down to 1 << res: the current
   best and its eight neighbours (+-step, +-step) in the same slot, illegal ones dropped, the same key.
   ODHIP_EINVAL before any launch: sizes, log_size outside 0..3, range outside 0..32, res outside 0..3, lambda
   outside 0..2^20 (the cost stays inside int32), strides below the widths, NULL planes.  ODHIP_EIMPL: a context with
   full-precision references (odhip_ctx_set_fpr). */
typedef struct {
  int32_t coded_w, coded_h;      /* multiples of 64, as odhip_mc_job */
  int32_t pic_w, pic_h;          /* 1..coded: the cost is clipped to it */
  int32_t npics, nrefs;          /* F; 1..3 slots */
  int32_t log_size, range, res, lambda;
  int32_t src_stride, ref_stride;                 /* in bytes, >= pic_w / >= coded_w; no alignment rule */
  int64_t src_plane_stride, ref_plane_stride;     /* between pictures: >= stride * rows */
  const uint8_t *src;            /* device: [F] luma pictures, pic_h rows */
  const uint8_t *ref[3];         /* device: [F] coded-size luma planes per slot, unpadded */
  odhip_mv_point *grid;          /* device out: [F][coded_h/8 + 1][coded_w/8 + 1] */
  uint32_t *cost;                /* device out, optional: the winner's cost, same shape, 0 at invalid points */
} odhip_me_job;
typedef struct {
  int32_t pic, vx, vy, slot, mvx, mvy;
} odhip_me_cand;
/* Asynchronous on `stream`; needs no scratch. */
int odhip_me_search(const odhip_me_job *job, odhip_stream stream);
/* Host: the full-pel offsets xmin, xmax, ymin, ymax that are legal for the valid point (vx, vy), both decimations. */
int odhip_me_limits(int coded_w, int coded_h, int log_size, int vx, int vy, int lim[4]);
/* Test surface: the SAD of n listed candidates (device memory) on the job's planes and block size, legal or not,
   no choice; grid, cost and the search parameters of the job are not read.  A candidate whose picture, point or
   slot does not exist gets 0xffffffff. */
int odhip_me_costs(const odhip_me_job *job, const odhip_me_cand *d_cands, long n, uint32_t *d_sad,
 odhip_stream stream);
/* sizeof of 0: odhip_me_job, 1: odhip_me_cand, 2: odhip_me_job2, 4: odhip_me_job3, 5: odhip_me_job4 (for language
   bindings); 3 and everything else: 0. */
size_t odhip_me_sizeof(int what);

/* ---- the search with chroma in the cost and SATD as the sub-pel metric (odhip_me_search2) ----
   The reference searches with OD_MC_USE_CHROMA (src/mcenc.c:1809) and, from the sub-pel stage on, with od_enc_satd
   (mc_use_satd, src/mcenc.c:1681-1748, 6520-6541).  The candidates, the key, the legality predicate and the two stages
   are those of odhip_me_search; the cost of a candidate (slot r, (mvx, mvy), point (vx, vy), B = 8 << log_size, luma
   block at (bx, by) = (8 vx - B/2, 8 vy - B/2)) becomes, per plane with decimation d (0 for luma, cdec for Cb, Cr):
     block       top left (bx >> d, by >> d) (bx, by are multiples of 4: exact), size B >> d
     vector      od_mc_scale_mv(mv, d) (OD_DIV_POW2_RE, src/state.c:660-661, as odhip_mc_predict_planes); at half-pel
                 multiples, all the reference's BMA visits, this is the mv*(1 << (2 - xdec)) of od_mv_est_bma_sad
     prediction  od_mc_predict1fmv8_c on the unpadded coded-size plane, read coordinates clamped
     clip        the block is cut to [0, OD_PLANE_SZ(pic_w, d)) x [0, OD_PLANE_SZ(pic_h, d)), OD_PLANE_SZ(n, d) =
                 (n + (1 << d) - 1) >> d, the prediction advanced with the cut; nothing left: distortion 0
     SAD         the sum of |prediction - source| over the clipped w x h rectangle
     SATD        od_enc_satd on the CLIPPED size: w == h == 4: the 4x4 Hadamard transform of the difference,
                 (sum |coeff| + 2) >> 2; w == h in {8, 16, 32, 64}: the sum over its 8x8 tiles of (sum |coeff of the
                 tile's 8x8 Hadamard| + 4) >> 3; any other rectangle: its SAD
   dist = D_Y + (D_Cb >> 2) + (D_Cr >> 2) with ODHIP_ME_CHROMA (each plane shifted before the add), else D_Y;
   cost = 8 dist + lambda' (|mvx| + |mvy|).
   Stage 1 (full-pel): D is SAD, lambda' = luma.lambda.  Stage 2 (the sub-pel rounds): D is SATD with ODHIP_ME_SATD,
   else SAD; lambda' = lambda_subpel; it starts by costing the stage-1 winner under its own metric and lambda', and
   the reported cost is the stage-2 cost.  With res = 3 stage 2 does not run: the SATD flag and lambda_subpel have no
   effect.  With flags = 0 and lambda_subpel = luma.lambda this is odhip_me_search, byte for byte (which calls it).
   The library takes the lambdas as given.  To reproduce the reference's, a caller that derives lambda as the
   reference does for luma passes lambda + 2 (lambda >> (2 cdec + 2)) with chroma in the cost, and 0.6 times that
   as lambda_subpel under SATD (src/mcenc.c:6431-6449, 6523-6527).
   ODHIP_EINVAL before any launch: everything odhip_me_search refuses, unknown flag bits, cdec outside 0..1,
   lambda_subpel outside 0..2^20 (a tile's SATD is at most its maximal SAD and chroma adds at most half of luma, so
   the cost stays inside int32 for both lambdas), and with ODHIP_ME_CHROMA NULL chroma pointers or strides below the
   widths.  Without ODHIP_ME_CHROMA nothing of the chroma half is read.  ODHIP_EIMPL: full-precision references. */
#define ODHIP_ME_CHROMA 1
#define ODHIP_ME_SATD   2
typedef struct {
  odhip_me_job luma;                 /* exactly as for odhip_me_search; luma.lambda is stage 1's */
  int32_t flags, cdec, lambda_subpel, reserved;
  int32_t csrc_stride, cref_stride;              /* bytes, >= the chroma picture / plane width */
  int64_t csrc_plane_stride, cref_plane_stride;  /* between chroma planes: >= stride * rows */
  const uint8_t *csrc;               /* device: [2F] chroma pictures, all Cb then all Cr (the pipe's order) */
  const uint8_t *cref[3];            /* device: [2F] coded-size chroma planes per slot, unpadded */
} odhip_me_job2;
int odhip_me_search2(const odhip_me_job2 *job, odhip_stream stream);
/* Test surface: per listed candidate the three UNSHIFTED plane distortions [n][3] (Y, Cb, Cr; chroma 0 without the
   flag) under metric 0 = SAD / 1 = SATD; a candidate that names nothing gets 0xffffffff three times. */
int odhip_me_costs2(const odhip_me_job2 *job, const odhip_me_cand *d_cands, long n, int metric, uint32_t *d_dist,
 odhip_stream stream);

/* ---- the search coarse to fine, to reach +-128 pixels (odhip_me_search3) ----
   Everything not said here is as in odhip_me_search2: the block of a point, legality (od_me_mv_ok on the
   FULL-RESOLUTION vector), the key (cost, |mvx| + |mvy|, slot, mvy, mvx), the grid layout, stage 2.
   Pyramid.  Level 0 is the plane itself; level j + 1 of a plane of w x h samples has ((w + 1) >> 1) x ((h + 1) >> 1):
     out[y][x] = (p[2y][2x] + p[2y][2x + 1] + p[2y + 1][2x] + p[2y + 1][2x + 1] + 2) >> 2,
   read coordinates clamped to the plane (an odd last row or column is replicated).  Level 2 is the halving of level
   1: it rounds twice.  Reference planes are coded-size, so their levels are (coded_w >> j) x (coded_h >> j); the
   source picture's level j has OD_PLANE_SZ(pic_w, j) x OD_PLANE_SZ(pic_h, j) samples.
   Parameters.  levels L in 0..2 with L <= log_size + 1 (the coarsest block B >> L is at least 4 x 4); luma.range in
   0..32 is the radius at the top level, in level-L samples; refine in 1..8 the radius at every level below the top.
   Coarse levels.  Each slot descends on its own: for a valid point and slot r the centre c starts at (0, 0); for
   j = L down to 1 the candidates are v = c + (8 << j) (dx, dy), |dx|, |dy| <= range at j = L, else <= refine, illegal
   ones dropped (zero is always legal and a winner is legal: never empty).  D_j(v) is the luma SAD of level j of
   reference plane r against level j of the source picture as a plane of decimation j: block top left
   (bx >> j, by >> j), size B >> j, sample offset v / (8 << j), read coordinates clamped, the block clipped to
   OD_PLANE_SZ(pic, j), an empty clip 0.  cost_j = 8 (D_j << 2j) + lambda (|vx| + |vy|): the shift puts a coarse SAD
   on the scale of the B x B block, so one lambda serves all levels.  c becomes the vector of the smallest key within
   the slot.
   Level 0 is stage 1 of odhip_me_search2 (SAD, chroma in the cost with ODHIP_ME_CHROMA, luma.lambda) over
   c_r + 8 (dx, dy), |dx|, |dy| <= refine, in every slot r round that slot's own centre; at 4:2:0 the chroma phase
   follows the ABSOLUTE full-pel offset.  The winner is the smallest key over all slots; stage 2 is unchanged.  With
   L = 0 the centre is 0, the radius is luma.range and this IS odhip_me_search2 (which it calls): byte for byte.
   Components reach 8 (32 << 2) + refine (16 + 8) + 7 <= 1223 eighth-pels, so with levels > 0 both lambdas stop at
   2^19: 8 * 1.5 * 64*64*255 + 2^19 * 2 * 1223 < 2^31.  The limit stays 2^20 at levels = 0.
   Scratch (device memory, any alignment) holds the pyramids and the per-slot centres; its layout is private,
   odhip_me_scratch_bytes gives its size: 0 at levels = 0 (or for a job whose sizes odhip_me_search refuses), where
   scratch is not read.
   ODHIP_EINVAL before any launch: everything odhip_me_search2 refuses, levels outside 0..min(2, log_size + 1), with
   levels > 0 refine outside 1..8, a lambda above 2^19, scratch NULL or scratch_bytes short.  ODHIP_EIMPL:
   full-precision references. */
typedef struct {
  odhip_me_job2 base;                /* exactly as for odhip_me_search2; luma.range is the top level's radius */
  int32_t levels, refine;
  void *scratch;                     /* device: odhip_me_scratch_bytes(job) bytes, written by every call */
  size_t scratch_bytes;
} odhip_me_job3;
int odhip_me_search3(const odhip_me_job3 *job, odhip_stream stream);
size_t odhip_me_scratch_bytes(const odhip_me_job3 *job);
/* One halving, as defined above, of nplanes 8-bit planes of w x h samples (device memory) into planes of
   ((w + 1) >> 1) x ((h + 1) >> 1); strides in bytes, >= the widths, plane strides >= stride * rows, no alignment
   rule.  Asynchronous on `stream`. */
int odhip_me_downsample(uint8_t *dst, int dst_stride, int64_t dst_plane_stride, const uint8_t *src, int src_stride,
 int64_t src_plane_stride, int w, int h, int nplanes, odhip_stream stream);
/* Test surface: D_level (level in 0..levels, luma only) of n listed candidates; it builds the pyramids in the job's
   scratch like the search.  0xffffffff for a candidate that names nothing or whose vector is no multiple of
   8 << level.  Of the search parameters only `levels` is read. */
int odhip_me_costs3(const odhip_me_job3 *job, const odhip_me_cand *d_cands, long n, int level, uint32_t *d_sad,
 odhip_stream stream);

/* ---- the search at variable block sizes, 8x8 to 64x64 (odhip_me_search_vbs) ----
   The producer of the mixed-size grids odhip_mc_predict_planes takes: large leaves where one vector serves, small
   ones where it does not.  Not the reference's sequential decimation (od_mv_est) but a fixed procedure that depends
   on no order, made of the block-matching cost above and the prediction, both pinned to the reference.
   Sizes.  log_max = base.base.luma.log_size, 0 <= log_min <= log_max <= 3; split_penalty in 0..2^24.  Everything else
   is read as odhip_me_search3 reads it.
   Legality.  A component is legal for the point at grid coordinate v of an axis of n steps when a leaf of
   1 << log_max steps at the origin of every cell of that size inside the frame whose CLOSED extent holds v keeps its
   filter window inside the 64-sample border, at dec 0 and dec 1 (od_me_mv_ok_cells, mc_walk.cuh).  Every leaf of the
   final grid that reads a point lies inside such a cell, its window inside the cell's, so every produced grid passes
   odhip_mc_check_grid at both decimations.  At a multiple of the size it is the uniform search's predicate.
   1.  For lg = log_min .. log_max: (G_lg, C_lg) = odhip_me_search3 at log_size = lg, levels = min(levels, lg + 1),
       under the legality above.
   2.  P_lg = odhip_mc_predict_planes of G_lg: luma, 8-bit, dec 0, the job's reference slots.
   3.  d_lg[pic][cy][cx] = the SAD of P_lg against the source picture over the 8x8 luma cell (cx, cy) clipped to
       pic_w x pic_h, an empty clip 0.  D_lg of a larger cell is the sum over its 8x8 cells.
   4.  Decisions, from the top: all cells of size log_max exist; an existing cell of size lg > log_min splits iff
       8 D_{lg-1}(cell) + split_penalty < 8 D_lg(cell), strictly; its four quadrants then exist.  A decision reads the d
       arrays alone.
   5.  The `valid` pattern: points at multiples of 8 steps; from the 64x64 cells down, the centre of a cell whose four
       corners are valid when the cell is larger than 1 << log_max or step 4 splits it; every edge midpoint the grid's
       rule allows (both ends valid, every cell inside the frame that shares the edge split).  A quadrant one of whose
       corners is the midpoint of an edge shared with an unsplit neighbour therefore stays whole.
   6.  A valid point takes (mvx, mvy, ref), and cost, from G_s / C_s, s the log size of the smallest leaf of the final
       pattern that has the point among its own four corners.  Invalid points are all zero; every point is written.
   With log_min == log_max the call IS odhip_me_search3 (which it calls): byte for byte, and scratch is that call's.
   cell_dist, optional: the d arrays, [log_max - log_min + 1][F][coded_h/8][coded_w/8], log_min first.
   Scratch: base.scratch, base.scratch_bytes name ONE device buffer of odhip_me_vbs_scratch_bytes(job) bytes (any
   alignment; 0 for a job whose sizes are refused) that holds the per-size grids, costs and predictions, the
   odhip_me_search3 scratch, the d arrays and the decisions.  Asynchronous on `stream`: no sync; the prediction uses
   the context's scratch, which odhip_mc_prepare allocates ahead of a first call.
   ODHIP_EINVAL before any launch: everything odhip_me_search3 refuses at any of the sizes, log_min or split_penalty
   outside their ranges, scratch NULL or short.  ODHIP_EIMPL: full-precision references. */
typedef struct {
  odhip_me_job3 base;                /* as for odhip_me_search3 at log_max; its scratch is the whole call's */
  int32_t log_min, split_penalty;
  uint32_t *cell_dist;               /* device out, optional */
} odhip_me_job4;
int odhip_me_search_vbs(const odhip_me_job4 *job, odhip_stream stream);
size_t odhip_me_vbs_scratch_bytes(const odhip_me_job4 *job);
/* Test and timing surface: step 3 alone.  pred[0 .. nsizes - 1] (nsizes 1..4) are device pointers, 8-byte aligned, to
   [F] coded-size 8-bit planes each, rows coded_w apart; dist is [nsizes][F][coded_h/8][coded_w/8].  Of the job the
   sizes and the source pictures are read (its reference pointers are checked, not read). */
int odhip_me_cell_dist(const odhip_me_job *job, const uint8_t *const *pred, int nsizes, uint32_t *dist,
 odhip_stream stream);

/* ---- inter steps that build their own prediction (pipeline.hip) ----
   odhip_pipe_set_reference_frames: nslots (1..3) resident reference plane sets of the CODED size in the planes' sample
   type (uint8; with fpr_bits int16 at 12 bits) - luma[slot]: [F][H][W], chroma[slot]: [2F][H >> cdec][W >> cdec], all
   Cb, then all Cr; syncs like odhip_pipe_set_pictures.  nslots = 0 drops frames and grids.
   odhip_pipe_set_mvs: the resident grids, [F][H/8 + 1][W/8 + 1] in host memory, checked for both decimations
   (ODHIP_ERANGE / ODHIP_EINVAL: nothing changes); NULL drops them.  Syncs.
   Once grids are set every inter step builds its prediction on the chain that consumes it (luma planes on the luma
   stream, chroma planes on the chroma stream) straight into the coded-size plane the prediction pyramid reads
   (ODHIP_PIPE_BUF_PRED); the prediction picture is not padded - the reference predicts the whole coded frame,
   src/encode.c:2370-2374.  While no grid is set nothing is allocated or launched and
   odhip_pipe_set_reference_pictures supplies the prediction; with a grid set it answers ODHIP_EINVAL (a step takes its
   prediction one way).
   odhip_pipe_feed_reference_frames / odhip_pipe_feed_mvs: the frames / grids of the NEXT step from pinned host memory,
   copied on the copy stream into back buffers without a sync, like odhip_pipe_feed; a step keeps the frames and grids
   it was enqueued with, its late resolve included (which reads the prediction pyramid on the chain's own stream before
   the next step's prediction is written).  The buffers stay valid until that step is enqueued and the copy is done. */
int odhip_pipe_set_reference_frames(odhip_pipe *p, int nslots, const void *const *luma, const void *const *chroma,
 int on_device);
int odhip_pipe_set_mvs(odhip_pipe *p, const odhip_mv_point *grid);
int odhip_pipe_feed_reference_frames(odhip_pipe *p, const void *const *luma, const void *const *chroma);
int odhip_pipe_feed_mvs(odhip_pipe *p, const odhip_mv_point *grid);
/* odhip_pipe_set_motion_search: from now on every inter step searches its own grids (odhip_me_search with these
   parameters: its ODHIP_PIPE_BUF_PIC luma against its luma reference frames) on the luma stream in front of the luma
   prediction, inside the timing bracket of that prediction, into the grid buffer no enqueued prediction reads; the
   chroma chain waits for an event behind the search; no sync is added.  Needs inter = 1, fpr_bits == 0 (ODHIP_EIMPL
   otherwise), reference frames set and no resident or fed grid (drop them with odhip_pipe_set_mvs(p, NULL));
   ODHIP_EINVAL for parameters odhip_me_search refuses.  While it is on, odhip_pipe_set_mvs, odhip_pipe_feed_mvs and
   odhip_pipe_set_reference_pictures answer ODHIP_EINVAL: a step takes its grids one way.  range < 0 switches it off
   (the grids are gone with it); while it is off nothing is allocated or launched.  Syncs.
   odhip_pipe_mvs_read: syncs and copies out the grids the last enqueued step predicted from
   ([F][H/8 + 1][W/8 + 1]) and, with the search on and cost != NULL, the winners' costs (same shape): the host entropy
   coder needs the vectors beside the export. */
int odhip_pipe_set_motion_search(odhip_pipe *p, int log_size, int range, int res, int lambda);
/* odhip_pipe_set_motion_search2: the same with odhip_me_search2's lambda_subpel and flags; (.., l, l, 0) is
   odhip_pipe_set_motion_search(.., l).  With ODHIP_ME_CHROMA the search also reads the step's chroma pictures and
   chroma reference frames (cdec = the pipe's), still on the luma stream; odhip_pipe_mvs_read's costs are stage 2's. */
int odhip_pipe_set_motion_search2(odhip_pipe *p, int log_size, int range, int res, int lambda, int lambda_subpel,
 int flags);
/* odhip_pipe_set_motion_search3: the same through odhip_me_search3; (.., 0, refine) is
   odhip_pipe_set_motion_search2(..).  The scratch is allocated here; a step builds its pyramids on the luma stream in
   front of its search, inside the same timing bracket; events and buffers are as above and no sync is added. */
int odhip_pipe_set_motion_search3(odhip_pipe *p, int log_size, int range, int res, int lambda, int lambda_subpel,
 int flags, int levels, int refine);
/* odhip_pipe_set_motion_search_vbs: the same through odhip_me_search_vbs, sizes log_min .. log_max; with
   log_min == log_max it is odhip_pipe_set_motion_search3 at that size.  Place, events, buffers and answers are those
   of odhip_pipe_set_motion_search3; the scratch is allocated here, and the step's own prediction takes the mixed-size
   grid as it takes any. */
int odhip_pipe_set_motion_search_vbs(odhip_pipe *p, int log_min, int log_max, int range, int res, int lambda,
 int lambda_subpel, int flags, int levels, int refine, int split_penalty);
int odhip_pipe_mvs_read(odhip_pipe *p, odhip_mv_point *grid, uint32_t *cost);

/* ---- lossless and Haar-wavelet frames (haar_kernels.hip) ----
   The coefficient path of a frame coded with use_haar_wavelet (always when lossless, src/encode.c:3027): every
   superblock one block of 64 >> dec samples (:3087-3088), the reversible integer Haar wavelet (od_haar / od_haar_inv,
   src/dct.c:4822-4888), od_wavelet_quantize (src/encode.c:1003-1080) and the sums of its three magnitude trees
   (od_compute_max_tree :899-919).  Integers only: every output is the reference's, bit for bit.

   The bare transforms: od_haar (inverse == 0) or od_haar_inv of every (1 << ln)-square block, ln = 2..6, of nplanes
   coefficient planes of w x h (row stride w, plane p at + p*w*h; w, h multiples of 1 << ln; both pointers 16-byte
   aligned; d_out may equal d_in).  ODHIP_EINVAL otherwise, before anything is launched. */
int odhip_haar_planes(od_coeff *d_out, const od_coeff *d_in, int nplanes, int w, int h, int ln, int inverse,
 odhip_stream stream);

/* The coded path of a plane set.  Samples are 8-bit, or int16 in a full-precision-references context; d_px, d_pred
   and d_rec share px_stride and px_plane_stride under the picture plane layout rules above.  d_q, d_tree: od_coeff
   [nplanes][h][w], 16-byte aligned; d_dc_rec: int32 [nplanes][(h/tile)*(w/tile)], tile = 64 >> dec. */
typedef struct {
  const void *d_px;          /* source planes (the encoder's; the decoder does not read them) */
  const void *d_pred;        /* prediction planes; NULL: keyframe */
  void *d_rec;               /* reconstructed sample planes; optional for the encoder */
  od_coeff *d_q;             /* the quantised coefficients where they lie; the DC slot holds the CODED DC symbol: keyframe
                                `quant` of src/encode.c:1581, inter scalar_out[0] of :1338-1343 (before :1373) */
  od_coeff *d_tree;          /* tree_sum[y][x] where coefficient (y, x) lies, the DC slot tree_sum[0][0] of :1033 */
  int32_t *d_dc_rec;         /* optional: the reconstructed superblock DCs (keyframe: sb_dc_mem) */
  int64_t px_plane_stride;
  int32_t px_stride;
  int32_t nplanes;
  int32_t w, h;              /* multiples of 64 >> dec */
  int32_t dec;               /* 0, or 1 for 4:2:0 chroma (32 x 32 blocks, the first five levels of OD_HAAR_QM) */
  int32_t pic_w, pic_h;      /* in plane samples, 1 .. w / h: inter source samples outside are replaced by the
                                prediction's (src/encode.c:2589-2602) */
  int32_t lossless;          /* selects the sample conversion with depth (src/state.c:1216-1255, :1281-1323) */
  int32_t depth;             /* 8, 10, 12 */
  int32_t quant;             /* state.quantizer: 0 (every sub-band step 1) iff lossless; at most 1 << 20 */
  int32_t dc_quant[2];       /* planes below plane_split use [0], the rest [1]; 1 .. 1 << 24, computed by the caller as
                                src/encode.c:1555-1559 (keyframe) and :1330-1335 (inter) do */
  int32_t plane_split;       /* 0 .. nplanes */
  int32_t reserved;
} odhip_haar_job;
/* Encoder: source (and prediction) -> d_q, d_tree, and when given d_dc_rec, d_rec.  Asynchronous on `stream`.  A
   keyframe job, the encoder's or the decoder's, keeps its superblock DCs in ONE scratch buffer of the current
   context: keyframe jobs of one context must not overlap - queue them on one stream, or order the streams with
   events, or give each stream its own context (inter jobs use no scratch).  ODHIP_EINVAL before anything is
   launched: a NULL d_px / d_q / d_tree, w or h no multiple of 64 >> dec, dec, depth, lossless with quant != 0 or
   lossy with quant == 0, quant < 0, a dc_quant below 1, pic_w / pic_h outside 1 .. w / h, plane_split outside
   0 .. nplanes, nplanes or h / (64 >> dec) above 65535 (the launch grid), the layout rules - all of them checked
   before the context is looked up, but for the 8-byte sample alignment of a full-precision-references context. */
int odhip_haar_encode_planes(const odhip_haar_job *job, odhip_stream stream);
/* Decoder: d_q (the symbols, the DC symbol included; not written) and the optional prediction -> d_rec (required) and
   d_dc_rec, through the kernels the encoder runs behind its quantiser.  d_px and d_tree are not used. */
int odhip_haar_decode_planes(const odhip_haar_job *job, odhip_stream stream);
size_t odhip_haar_sizeof(void);   /* sizeof(odhip_haar_job), for language bindings */

#ifdef __cplusplus
}
#endif
#endif
