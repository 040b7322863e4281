/* C99 host: two analysed utterances joined with a cross-fade that never leaves the device, through llsm_gpu.h alone:
 * analyse, layer 1, undo the phase propagation, gather the frames of both utterances into ONE output utterance
 * (llsm_gpu_batch_splice: utterance 0 up to the fade, ten frames of both with the weight of utterance 1 rising from 0 to 1,
 * utterance 1 from there on), rebuild the harmonic model from layer 1, propagate the phases again, synthesise.
 * Checks: the output is ny(nfrm) samples long and finite, the level of the fade lies between the levels of the frames on
 * either side of it (+- 3 dB), and splice refuses NULL arguments, the same batch twice, a map without pos_a, a second side
 * given in part, and positions, utterances and weights out of range.
 * Built and run by tests/test_gpu_splice.py (gcc -std=c99 -pedantic -Wall -Wextra -Werror). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llsm.h"
#include "llsm_gpu.h"

#define CHECK(c) do { if(!(c)) { fprintf(stderr, "CHECK failed: %s (line %d): %s\n", #c, __LINE__, llsm_gpu_last_error()); return 1; } } while(0)
#define REFUSED(call) do { CHECK((call) == -1); CHECK(strncmp(llsm_gpu_last_error(), "llsm_gpu_batch_splice:", 22) == 0); } while(0)
static const double PI = 3.14159265358979323846;
enum { NUTT = 2, NPRE = 60, NFADE = 10, B0 = 40 };

static double level_db(const FP_TYPE* y, int t0, int t1) {
  double e = 0;
  for(int t = t0; t < t1; t ++) e += (double)y[t] * y[t];
  return 10.0 * log10(e / (t1 > t0 ? t1 - t0 : 1) + 1e-30);
}

int main(void) {
  if(llsm_gpu_device_count() == 0) { printf("splice_batch: no device\n"); return 2; }
  const FP_TYPE fs = 22050.0f;
  const int nhop = 128, nx[NUTT] = {21000, 21000};
  int nfrm[NUTT], xtot = 0, ftot = 0;
  for(int u = 0; u < NUTT; u ++) { nfrm[u] = nx[u] / nhop; xtot += nx[u]; ftot += nfrm[u]; }
  FP_TYPE* x = (FP_TYPE*)calloc((size_t)xtot, sizeof(FP_TYPE));
  FP_TYPE* f0 = (FP_TYPE*)calloc((size_t)ftot, sizeof(FP_TYPE));
  /* two voiced glides a fifth apart with a formant-ish roll-off and a little noise */
  unsigned s = 4321u;
  for(int u = 0, xo = 0, fo = 0; u < NUTT; xo += nx[u], fo += nfrm[u], u ++) {
    double ph = 0;
    const double f_lo = u ? 180.0 : 120.0;
    for(int t = 0; t < nx[u]; t ++) {
      const double f = f_lo + 30.0 * t / nx[u];
      ph += 2 * PI * f / fs;
      double v = 0;
      for(int k = 1; k <= 25; k ++) v += 0.25 / k * (1.0 + 0.8 * exp(-pow((k * f - 900.0) / 400.0, 2))) * cos(k * ph + 0.2 * k);
      s = s * 1664525u + 1013904223u;
      x[xo + t] = (FP_TYPE)((u ? 0.7 : 1.0) * v + 0.004 * ((double)(s >> 8) / 8388608.0 - 1.0));
    }
    for(int i = 0; i < nfrm[u]; i ++) f0[fo + i] = (FP_TYPE)(f_lo + 30.0 * (i * nhop) / nx[u]);
  }

  /* the join: NPRE frames of utterance 0, NFADE frames of both, the rest of utterance 1 from frame B0 + NFADE on */
  const int npost = nfrm[1] - (B0 + NFADE), F = NPRE + NFADE + npost, zero = 0;
  CHECK(NPRE + NFADE <= nfrm[0] && npost > NFADE);
  int* utt_a = (int*)calloc((size_t)F, sizeof(int));
  int* utt_b = (int*)calloc((size_t)F, sizeof(int));
  FP_TYPE* pos_a = (FP_TYPE*)calloc((size_t)F, sizeof(FP_TYPE));
  FP_TYPE* pos_b = (FP_TYPE*)calloc((size_t)F, sizeof(FP_TYPE));
  FP_TYPE* mix = (FP_TYPE*)calloc((size_t)F, sizeof(FP_TYPE));
  for(int i = 0; i < F; i ++) {
    const int a = i < NPRE + NFADE ? i : NPRE + NFADE - 1, b = i - NPRE + B0;
    utt_a[i] = 0; pos_a[i] = (FP_TYPE)a;
    utt_b[i] = 1; pos_b[i] = (FP_TYPE)(b < 0 ? 0 : b);
    mix[i] = i < NPRE ? 0.0f : (i >= NPRE + NFADE ? 1.0f : (FP_TYPE)(i - NPRE + 1) / (FP_TYPE)(NFADE + 1));
  }

  llsm_aoptions* oa = llsm_create_aoptions();
  oa -> thop = (FP_TYPE)nhop / fs; oa -> f0_refine = 0;
  llsm_soptions* os = llsm_create_soptions(fs);
  llsm_gpu_context* ctx = llsm_gpu_create_context(0, NULL);
  CHECK(ctx != NULL);
  llsm_gpu_batch* src = llsm_gpu_create_batch(ctx, oa, fs, NUTT, nx, nfrm);
  llsm_gpu_batch* dst = llsm_gpu_create_batch(ctx, oa, fs, 1, & zero, & F);
  CHECK(src != NULL && dst != NULL);
  CHECK(llsm_gpu_batch_upload(src, LLSM_GPU_X, x, sizeof(FP_TYPE) * (size_t)xtot) == 0);
  CHECK(llsm_gpu_batch_upload(src, LLSM_GPU_F0, f0, sizeof(FP_TYPE) * (size_t)ftot) == 0);
  CHECK(llsm_gpu_batch_analyze(src) == 0);
  CHECK(llsm_gpu_batch_tolayer1(src, 2048) == 0);
  CHECK(llsm_gpu_batch_phasepropagate(src, -1) == 0);

  llsm_gpu_splice_map map;
  map.utt_a = utt_a; map.pos_a = pos_a; map.utt_b = utt_b; map.pos_b = pos_b; map.mix = mix;
  CHECK(llsm_gpu_batch_splice(dst, src, & map) == 0);
  CHECK(llsm_gpu_batch_tolayer0(dst, 1) == 0);
  CHECK(llsm_gpu_batch_phasepropagate(dst, 1) == 0);
  CHECK(llsm_gpu_batch_synthesize(dst, os, 5, 0) == 0);
  llsm_gpu_layout lay;
  CHECK(llsm_gpu_batch_layout(dst, & lay) == 0);
  FP_TYPE* y = (FP_TYPE*)malloc(sizeof(FP_TYPE) * (size_t)lay.total_out);
  CHECK(llsm_gpu_batch_download(dst, LLSM_GPU_Y, y, sizeof(FP_TYPE) * (size_t)lay.total_out) == 0);
  const int want = llsm_gpu_plan_index(5, F, 0, 0, oa -> thop, fs, oa -> rel_winsize);
  int bad = 0;
  for(int t = 0; t < lay.total_out; t ++) if(!isfinite(y[t])) bad ++;
  const double la = level_db(y, (NPRE - NFADE) * nhop, NPRE * nhop), lf = level_db(y, NPRE * nhop, (NPRE + NFADE) * nhop),
    lb = level_db(y, (NPRE + NFADE) * nhop, (NPRE + 2 * NFADE) * nhop);
  printf("splice_batch: %d frames -> %d samples (ny(nfrm) = %d), non-finite %d, level before / in / after the fade "
    "%+.2f / %+.2f / %+.2f dB\n", F, lay.total_out, want, bad, la, lf, lb);
  CHECK(lay.total_out == want && bad == 0);
  CHECK(lf >= (la < lb ? la : lb) - 3.0 && lf <= (la > lb ? la : lb) + 3.0);

  /* refusals: nothing is written, the message is prefixed */
  llsm_gpu_splice_map m = map;
  REFUSED(llsm_gpu_batch_splice(NULL, src, & map));
  REFUSED(llsm_gpu_batch_splice(dst, NULL, & map));
  REFUSED(llsm_gpu_batch_splice(dst, src, NULL));
  REFUSED(llsm_gpu_batch_splice(src, src, & map));
  m.pos_a = NULL; REFUSED(llsm_gpu_batch_splice(dst, src, & m)); m = map;
  m.mix = NULL; REFUSED(llsm_gpu_batch_splice(dst, src, & m)); m = map;
  m.utt_b = NULL; m.pos_b = NULL; REFUSED(llsm_gpu_batch_splice(dst, src, & m)); m = map;
  pos_a[3] = (FP_TYPE)nfrm[0]; REFUSED(llsm_gpu_batch_splice(dst, src, & map)); pos_a[3] = 3;
  pos_b[F - 1] = -0.5f; REFUSED(llsm_gpu_batch_splice(dst, src, & map)); pos_b[F - 1] = (FP_TYPE)(nfrm[1] - 1);
  utt_b[5] = NUTT; REFUSED(llsm_gpu_batch_splice(dst, src, & map)); utt_b[5] = 1;
  utt_a[0] = -1; REFUSED(llsm_gpu_batch_splice(dst, src, & map)); utt_a[0] = 0;
  mix[7] = 1.5f; REFUSED(llsm_gpu_batch_splice(dst, src, & map)); mix[7] = 0;
  m.utt_b = NULL; m.pos_b = NULL; m.mix = NULL;
  CHECK(llsm_gpu_batch_splice(dst, src, & m) == 0);        /* one side alone, and the full map again */
  CHECK(llsm_gpu_batch_splice(dst, src, & map) == 0);
  CHECK(llsm_gpu_synchronize(ctx) == 0);

  llsm_gpu_delete_batch(dst); llsm_gpu_delete_batch(src); llsm_gpu_delete_context(ctx);
  llsm_delete_aoptions(oa); llsm_delete_soptions(os);
  free(x); free(f0); free(y); free(utt_a); free(utt_b); free(pos_a); free(pos_b); free(mix);
  printf("splice_batch ok\n");
  return 0;
}
