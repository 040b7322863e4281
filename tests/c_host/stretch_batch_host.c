/* C99 host: a two-fold time stretch that never leaves the device, through llsm_gpu.h alone -- the batch form of the
 * recipe tests/c_host/stretch_host.c walks on containers: analyse, layer 1, undo the phase propagation, blend the frames
 * onto a grid of twice as many (llsm_gpu_batch_retime, uniform map), rebuild the harmonic model from layer 1, propagate
 * the phases again, synthesise.  Two utterances in one batch; only the waveforms come back to the host.
 * Checks: every output is ny(2 nfrm) samples long and finite, its level within 1 dB of the unstretched resynthesis, and
 * the phase operations / retime refuse a NULL batch.
 * Built and run by tests/test_gpu_retime.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "llsm.h"
#include "llsm_gpu.h"

#define CHECK(c) do { if(!(c)) { fprintf(stderr, "CHECK failed: %s (line %d): %s\n", #c, __LINE__, llsm_gpu_last_error()); return 1; } } while(0)
static const double PI = 3.14159265358979323846;
enum { NUTT = 2 };

static double power_of(const FP_TYPE* y, int n) {
  double e = 0;
  for(int t = 0; t < n; t ++) e += (double)y[t] * y[t];
  return e / (n > 0 ? n : 1);
}

int main(void) {
  if(llsm_gpu_device_count() == 0) { printf("stretch_batch: no device\n"); return 2; }
  const FP_TYPE fs = 22050.0f;
  const int nhop = 128, nx[NUTT] = {30000, 21000};
  int nfrm[NUTT], nfrm2[NUTT], nx0[NUTT] = {0, 0};
  int xtot = 0, ftot = 0;
  for(int u = 0; u < NUTT; u ++) { nfrm[u] = nx[u] / nhop; nfrm2[u] = 2 * nfrm[u]; xtot += nx[u]; ftot += nfrm[u]; }
  FP_TYPE* x = (FP_TYPE*)calloc((size_t)xtot, sizeof(FP_TYPE));
  FP_TYPE* f0 = (FP_TYPE*)calloc((size_t)ftot, sizeof(FP_TYPE));
  /* glides with a formant-ish roll-off, an unvoiced gap, a little noise */
  unsigned s = 4321u;
  for(int u = 0, xo = 0, fo = 0; u < NUTT; xo += nx[u], fo += nfrm[u], u ++) {
    double ph = 0;
    const double f_lo = u ? 190.0 : 120.0;
    for(int t = 0; t < nx[u]; t ++) {
      const double f = f_lo + 40.0 * t / nx[u];
      const int voiced = !(t > 9000 && t < 11500);
      ph += 2 * PI * f / fs;
      double v = 0;
      if(voiced) for(int k = 1; k <= 25; k ++) v += 0.25 / k * (1.0 + 0.8 * exp(-pow((k * f - 900.0) / 400.0, 2))) * cos(k * ph + 0.2 * k);
      s = s * 1664525u + 1013904223u;
      x[xo + t] = (FP_TYPE)(v + 0.004 * ((double)(s >> 8) / 8388608.0 - 1.0));
    }
    for(int i = 0; i < nfrm[u]; i ++) {
      const int t = i * nhop;
      f0[fo + i] = (t > 9000 && t < 11500) ? 0.0f : (FP_TYPE)(f_lo + 40.0 * t / nx[u]);
    }
  }

  llsm_aoptions* oa = llsm_create_aoptions();
  oa -> thop = (FP_TYPE)nhop / fs; oa -> f0_refine = 0;
  llsm_soptions* os = llsm_create_soptions(fs);
  llsm_gpu_context* ctx = llsm_gpu_create_context(0, NULL);
  CHECK(ctx != NULL);
  llsm_gpu_batch* src = llsm_gpu_create_batch(ctx, oa, fs, NUTT, nx, nfrm);
  llsm_gpu_batch* dst = llsm_gpu_create_batch(ctx, oa, fs, NUTT, nx0, nfrm2);
  CHECK(src != NULL && dst != NULL);
  CHECK(llsm_gpu_batch_upload(src, LLSM_GPU_X, x, sizeof(FP_TYPE) * (size_t)xtot) == 0);
  CHECK(llsm_gpu_batch_upload(src, LLSM_GPU_F0, f0, sizeof(FP_TYPE) * (size_t)ftot) == 0);
  CHECK(llsm_gpu_batch_analyze(src) == 0);
  CHECK(llsm_gpu_batch_synthesize(src, os, 5, 0) == 0);           /* the unstretched resynthesis */
  llsm_gpu_layout l1, l2;
  CHECK(llsm_gpu_batch_layout(src, & l1) == 0 && llsm_gpu_batch_layout(dst, & l2) == 0);
  FP_TYPE* y1 = (FP_TYPE*)malloc(sizeof(FP_TYPE) * (size_t)l1.total_out);
  FP_TYPE* y2 = (FP_TYPE*)malloc(sizeof(FP_TYPE) * (size_t)l2.total_out);
  CHECK(llsm_gpu_batch_download(src, LLSM_GPU_Y, y1, sizeof(FP_TYPE) * (size_t)l1.total_out) == 0);

  /* the recipe, on the device */
  CHECK(llsm_gpu_batch_tolayer1(src, 2048) == 0);
  CHECK(llsm_gpu_batch_phasepropagate(src, -1) == 0);
  CHECK(llsm_gpu_batch_retime(dst, src, NULL, NULL) == 0);
  CHECK(llsm_gpu_batch_tolayer0(dst, 1) == 0);
  CHECK(llsm_gpu_batch_phasepropagate(dst, 1) == 0);
  CHECK(llsm_gpu_batch_synthesize(dst, os, 5, 0) == 0);
  CHECK(llsm_gpu_batch_download(dst, LLSM_GPU_Y, y2, sizeof(FP_TYPE) * (size_t)l2.total_out) == 0);

  int yo1[NUTT + 1], yo2[NUTT + 1];
  CHECK(llsm_gpu_batch_offsets(src, NULL, NULL, yo1) == 0 && llsm_gpu_batch_offsets(dst, NULL, NULL, yo2) == 0);
  for(int u = 0; u < NUTT; u ++) {
    const int n1 = yo1[u + 1] - yo1[u], n2 = yo2[u + 1] - yo2[u];
    const int want = llsm_gpu_plan_index(5, nfrm2[u], 0, 0, oa -> thop, fs, oa -> rel_winsize);
    int bad = 0;
    for(int t = 0; t < n2; t ++) if(!isfinite(y2[yo2[u] + t])) bad ++;
    const double lvl = 10.0 * log10(power_of(y2 + yo2[u], n2) / power_of(y1 + yo1[u], n1));
    printf("stretch_batch: utterance %d: %d -> %d samples (ny(2 nfrm) = %d), level %+.2f dB, non-finite %d\n",
      u, n1, n2, want, lvl, bad);
    CHECK(n2 == want && bad == 0 && fabs(lvl) < 1.0);
  }
  /* refusals */
  CHECK(llsm_gpu_batch_retime(NULL, src, NULL, NULL) == -1);
  CHECK(llsm_gpu_batch_retime(src, src, NULL, NULL) == -1);
  CHECK(llsm_gpu_batch_phasepropagate(NULL, 1) == -1 && llsm_gpu_batch_phasesync_rps(NULL, 0) == -1);

  llsm_gpu_delete_batch(dst); llsm_gpu_delete_batch(src); llsm_gpu_delete_context(ctx);
  llsm_delete_aoptions(oa); llsm_delete_soptions(os);
  free(x); free(f0); free(y1); free(y2);
  printf("stretch_batch ok\n");
  return 0;
}
