/* C99 host: a pitch shift by 1.5 with a formant shift by 1.1 that never leaves the device, through llsm_gpu.h alone -- the
 * batch form of the reference's layer-1 pitch-shift recipe: analyse, layer 1, undo the phase propagation, scale F0 and
 * compensate VTMAGN per frame (llsm_gpu_batch_pitch_formant, PSD warped too), rebuild the harmonic model from layer 1,
 * propagate the phases again, synthesise.  Two utterances in one batch; only the waveforms come back to the host.
 * Checks: every output is as long as the unshifted resynthesis and finite, its level within 6 dB of it, and bad calls
 * (NULL batch, unknown flag, NaN or out-of-range ratio, batch without layer 1) are refused.
 * Built and run by tests/test_gpu_pitch.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic). */
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
  if(llsm_gpu_device_count() == 0) { printf("pitch_batch: no device\n"); return 2; }
  const FP_TYPE fs = 22050.0f;
  const int nhop = 128, nx[NUTT] = {30000, 21000};
  int nfrm[NUTT];
  int xtot = 0, ftot = 0;
  for(int u = 0; u < NUTT; u ++) { nfrm[u] = nx[u] / nhop; xtot += nx[u]; ftot += nfrm[u]; }
  FP_TYPE* x = (FP_TYPE*)calloc((size_t)xtot, sizeof(FP_TYPE));
  FP_TYPE* f0 = (FP_TYPE*)calloc((size_t)ftot, sizeof(FP_TYPE));
  FP_TYPE* rho = (FP_TYPE*)malloc(sizeof(FP_TYPE) * (size_t)ftot);
  FP_TYPE* alpha = (FP_TYPE*)malloc(sizeof(FP_TYPE) * (size_t)ftot);
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
  for(int g = 0; g < ftot; g ++) { rho[g] = 1.5f; alpha[g] = 1.1f; }

  llsm_aoptions* oa = llsm_create_aoptions();
  oa -> thop = (FP_TYPE)nhop / fs; oa -> f0_refine = 0;
  llsm_soptions* os = llsm_create_soptions(fs);
  llsm_gpu_context* ctx = llsm_gpu_create_context(0, NULL);
  CHECK(ctx != NULL);
  llsm_gpu_batch* b = llsm_gpu_create_batch(ctx, oa, fs, NUTT, nx, nfrm);
  CHECK(b != NULL);
  CHECK(llsm_gpu_batch_upload(b, LLSM_GPU_X, x, sizeof(FP_TYPE) * (size_t)xtot) == 0);
  CHECK(llsm_gpu_batch_upload(b, LLSM_GPU_F0, f0, sizeof(FP_TYPE) * (size_t)ftot) == 0);
  CHECK(llsm_gpu_batch_analyze(b) == 0);
  /* refused while the batch has no layer 1 */
  CHECK(llsm_gpu_batch_pitch_formant(b, rho, NULL, 0) == -1);
  CHECK(llsm_gpu_batch_synthesize(b, os, 5, 0) == 0);             /* the unshifted resynthesis */
  llsm_gpu_layout lay;
  CHECK(llsm_gpu_batch_layout(b, & lay) == 0);
  FP_TYPE* y1 = (FP_TYPE*)malloc(sizeof(FP_TYPE) * (size_t)lay.total_out);
  FP_TYPE* y2 = (FP_TYPE*)malloc(sizeof(FP_TYPE) * (size_t)lay.total_out);
  CHECK(llsm_gpu_batch_download(b, LLSM_GPU_Y, y1, sizeof(FP_TYPE) * (size_t)lay.total_out) == 0);

  /* the recipe, on the device */
  CHECK(llsm_gpu_batch_tolayer1(b, 2048) == 0);
  CHECK(llsm_gpu_batch_phasepropagate(b, -1) == 0);
  CHECK(llsm_gpu_batch_pitch_formant(b, rho, alpha, LLSM_GPU_WARP_PSD) == 0);
  CHECK(llsm_gpu_batch_tolayer0(b, 1) == 0);
  CHECK(llsm_gpu_batch_phasepropagate(b, 1) == 0);
  CHECK(llsm_gpu_batch_synthesize(b, os, 5, 0) == 0);
  CHECK(llsm_gpu_batch_download(b, LLSM_GPU_Y, y2, sizeof(FP_TYPE) * (size_t)lay.total_out) == 0);

  int yo[NUTT + 1];
  CHECK(llsm_gpu_batch_offsets(b, NULL, NULL, yo) == 0);
  for(int u = 0; u < NUTT; u ++) {
    const int n = yo[u + 1] - yo[u];
    int bad = 0;
    for(int t = 0; t < n; t ++) if(!isfinite(y2[yo[u] + t])) bad ++;
    const double lvl = 10.0 * log10(power_of(y2 + yo[u], n) / power_of(y1 + yo[u], n));
    printf("pitch_batch: utterance %d: %d samples, level %+.2f dB, non-finite %d\n", u, n, lvl, bad);
    CHECK(n > 0 && bad == 0 && fabs(lvl) < 6.0);
  }
  /* refusals */
  CHECK(llsm_gpu_batch_pitch_formant(NULL, rho, alpha, 0) == -1);
  CHECK(llsm_gpu_batch_pitch_formant(b, rho, alpha, 2) == -1);
  rho[7] = NAN;
  CHECK(llsm_gpu_batch_pitch_formant(b, rho, NULL, 0) == -1);
  rho[7] = 1.5f; alpha[3] = 5.0f;
  CHECK(llsm_gpu_batch_pitch_formant(b, NULL, alpha, 0) == -1);

  llsm_gpu_delete_batch(b); llsm_gpu_delete_context(ctx);
  llsm_delete_aoptions(oa); llsm_delete_soptions(os);
  free(x); free(f0); free(rho); free(alpha); free(y1); free(y2);
  printf("pitch_batch ok\n");
  return 0;
}
