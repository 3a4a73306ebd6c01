/* tools/partition_recorder.c - DEV-TIME TEST INFRASTRUCTURE, CPU only (tools/make_golden_partition.py
   compiles it against the reference's public headers and oracle/_ref/libdaalaref.so; never committed
   in built form; it calls nothing of libdaalahip).

   A sibling of tests/interpose's GPU decode check: inside the REAL reference decoder, at the frame-level
   post-filter of every plane (src/decode.c:988-996), hand the caller
     - the dequantised coefficient plane (state.dtmp[pli]) and the block-size map the decoder is about
       to have reconstructed from,
     - the decoder's own reconstruction AFTER its od_apply_postfilter_frame_sbs (state.ctmp[pli]; the
       recorder turns it into pixels as tests/interpose/interpose.c does),
   so that tests/_partition_ref.py's inverse() can be pinned to the decoder at real mixed partitions.

   Load it with RTLD_GLOBAL: its od_apply_postfilter_frame_sbs and daala_decode_packet_in then front
   the reference's own, which it reaches with RTLD_NEXT.  partrec_roundtrip drives an encoder and a
   decoder through the public API, as oracle/ref_encoder_driver.c's ref_roundtrip_yuv420 does, but with
   a keyframe interval of the caller's so that inter frames occur. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "daala/codec.h"
#include "daala/daalaenc.h"
#include "daala/daaladec.h"

typedef int32_t od_coeff;

/* oracle/ref_encoder_driver.c */
int ref_state_recon_view(void *statep, const od_coeff *c, const od_coeff **d, const unsigned char **bsize,
 int *bstride, int *pic_w, int *pic_h);

typedef void (*partrec_fn)(int pli, int xdec, int keyframe, int w, int h, int pic_w, int pic_h,
 const od_coeff *d, const od_coeff *c, const unsigned char *bsize, int bstride);

static partrec_fn g_record;
static void *g_dec;
static int g_keyframe;

void partrec_set_callback(partrec_fn fn) {
  g_record = fn;
}

int daala_decode_packet_in(daala_dec_ctx *dec, const daala_packet *dp) {
  typedef int (*fn)(daala_dec_ctx *, const daala_packet *);
  static fn next;
  if (!next) next = (fn)dlsym(RTLD_NEXT, "daala_decode_packet_in");
  g_dec = dec;
  g_keyframe = daala_packet_iskeyframe((daala_packet *)dp) > 0;
  return next(dec, dp);
}

void od_apply_postfilter_frame_sbs(od_coeff *c, int stride, int nhsb, int nvsb, int xdec, int ydec, int q,
 unsigned char *skip, int skip_stride) {
  typedef void (*fn)(od_coeff *, int, int, int, int, int, int, unsigned char *, int);
  static fn next;
  const od_coeff *d;
  const unsigned char *bsize;
  int bstride;
  int pic_w;
  int pic_h;
  int pli;
  if (!next) next = (fn)dlsym(RTLD_NEXT, "od_apply_postfilter_frame_sbs");
  next(c, stride, nhsb, nvsb, xdec, ydec, q, skip, skip_stride);
  /* only the decoder's planes: the encoder in the same process laps its own */
  if (!g_record || !g_dec || xdec != ydec) return;
  pli = ref_state_recon_view(g_dec, c, &d, &bsize, &bstride, &pic_w, &pic_h);
  if (pli < 0) return;
  if (stride != nhsb << 6 >> xdec) abort();
  g_record(pli, xdec, g_keyframe, stride, nvsb << 6 >> ydec, pic_w, pic_h, d, c, bsize, bstride);
}

/* frames: nframes pictures, planar 4:2:0, 8 bits, tightly packed.  Returns the number of decoded
   pictures or a negative code. */
int partrec_roundtrip(const unsigned char *frames, int w, int h, int nframes, int quality, int complexity,
 int keyframe_rate) {
  daala_info di;
  daala_info di2;
  daala_comment dc;
  daala_comment dc2;
  daala_setup_info *ds;
  daala_enc_ctx *enc;
  daala_dec_ctx *dec;
  daala_packet dp;
  daala_image img;
  daala_image out;
  long frame_bytes;
  int cw;
  int ch;
  int ndecoded;
  int f;
  int ret;
  int pli;
  daala_info_init(&di);
  di.pic_width = w;
  di.pic_height = h;
  di.bitdepth_mode = OD_BITDEPTH_MODE_8;
  di.timebase_numerator = 30;
  di.timebase_denominator = 1;
  di.frame_duration = 1;
  di.pixel_aspect_numerator = 1;
  di.pixel_aspect_denominator = 1;
  di.nplanes = 3;
  for (pli = 0; pli < 3; pli++) di.plane_info[pli].xdec = di.plane_info[pli].ydec = pli > 0;
  di.keyframe_rate = keyframe_rate;
  enc = daala_encode_create(&di);
  if (enc == NULL) return -1;
  daala_comment_init(&dc);
  daala_encode_ctl(enc, OD_SET_QUANT, &quality, sizeof(quality));
  daala_encode_ctl(enc, OD_SET_COMPLEXITY, &complexity, sizeof(complexity));
  daala_info_init(&di2);
  daala_comment_init(&dc2);
  ds = NULL;
  for (;;) {
    ret = daala_encode_flush_header(enc, &dc, &dp);
    if (ret < 0) return ret;
    if (ret == 0) break;
    ret = daala_decode_header_in(&di2, &dc2, &ds, &dp);
    if (ret < 0) return ret;
  }
  dec = daala_decode_create(&di2, ds);
  if (dec == NULL) return -3;
  cw = (w + 1) >> 1;
  ch = (h + 1) >> 1;
  frame_bytes = (long)w*h + 2L*cw*ch;
  memset(&img, 0, sizeof(img));
  img.nplanes = 3;
  img.width = w;
  img.height = h;
  ndecoded = 0;
  for (f = 0; f <= nframes; f++) {
    int last;
    last = f == nframes;
    while (daala_encode_packet_out(enc, last, &dp)) {
      ret = daala_decode_packet_in(dec, &dp);
      if (ret < 0) return ret;
      while (daala_decode_img_out(dec, &out) > 0) ndecoded++;
    }
    if (!last) {
      unsigned char *base;
      base = (unsigned char *)frames + f*frame_bytes;
      for (pli = 0; pli < 3; pli++) {
        img.planes[pli].xdec = img.planes[pli].ydec = pli > 0;
        img.planes[pli].xstride = 1;
        img.planes[pli].ystride = pli ? cw : w;
        img.planes[pli].bitdepth = 8;
      }
      img.planes[0].data = base;
      img.planes[1].data = base + (long)w*h;
      img.planes[2].data = img.planes[1].data + (long)cw*ch;
      ret = daala_encode_img_in(enc, &img, 0);
      if (ret < 0) return ret;
    }
  }
  g_dec = NULL;
  daala_setup_free(ds);
  daala_decode_free(dec);
  daala_comment_clear(&dc);
  daala_comment_clear(&dc2);
  daala_encode_free(enc);
  return ndecoded;
}
