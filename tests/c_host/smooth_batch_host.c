/* C99 host: a join between two recordings, smoothed without leaving the device, through llsm_gpu.h alone: analyse two
 * utterances of different pitch, layer 1, render an index list that hops from the first to the second in the form
 * llsm_gpu_batch_select returns it (llsm_gpu_batch_splice), turn the list into radii (llsm_gpu_join_radii), smooth the tracks
 * around the join (llsm_gpu_batch_smooth), rebuild the harmonic model from layer 1 and synthesise.  Only the F0 row and the
 * waveform come back to the host.
 * Checks: one join is found, the radii are reach at the join and 0 far from it, the F0 step across the join is smaller after
 * the call than before, frames far from the join keep their F0 bit for bit, the output is finite and not silent, and bad calls
 * (NULL batch, NULL radius, unknown flag, radius out of range, batch without layer 1, reach out of range) are refused.
 * Built and run by tests/test_gpu_smooth.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "llsm.h"
#include "llsm_gpu.h"

#define CHECK(c) do { if(!(c)) { fprintf(stderr, "CHECK failed: %s (line %d): %s\n", #c, __LINE__, llsm_gpu_last_error()); return 1; } } while(0)
static const double PI = 3.14159265358979323846;
enum { NUTT = 2, NDST = 80, HALF = 40, REACH = 8 };

int main(void) {
  if(llsm_gpu_device_count() == 0) { printf("smooth_batch: no device\n"); return 2; }
  const FP_TYPE fs = 22050.0f;
  const int nhop = 128, nx[NUTT] = {21000, 21000};
  int nfrm[NUTT];
  int xtot = 0, ftot = 0;
  for(int u = 0; u < NUTT; u ++) { nfrm[u] = nx[u] / nhop; xtot += nx[u]; ftot += nfrm[u]; }
  FP_TYPE* x = (FP_TYPE*)calloc((size_t)xtot, sizeof(FP_TYPE));
  FP_TYPE* f0 = (FP_TYPE*)calloc((size_t)ftot, sizeof(FP_TYPE));
  /* two voiced glides a fifth apart, a little noise */
  unsigned s = 99u;
  for(int u = 0, xo = 0, fo = 0; u < NUTT; xo += nx[u], fo += nfrm[u], u ++) {
    double ph = 0;
    const double f_lo = u ? 180.0 : 120.0;
    for(int t = 0; t < nx[u]; t ++) {
      const double f = f_lo + 20.0 * t / nx[u];
      ph += 2 * PI * f / fs;
      double v = 0;
      for(int k = 1; k <= 25; k ++) v += 0.25 / k * cos(k * ph + 0.2 * k);
      s = s * 1664525u + 1013904223u;
      x[xo + t] = (FP_TYPE)(v + 0.004 * ((double)(s >> 8) / 8388608.0 - 1.0));
    }
    for(int i = 0; i < nfrm[u]; i ++) f0[fo + i] = (FP_TYPE)(f_lo + 20.0 * (i * nhop) / nx[u]);
  }

  llsm_aoptions* oa = llsm_create_aoptions();
  oa -> thop = (FP_TYPE)nhop / fs; oa -> f0_refine = 0;
  llsm_soptions* os = llsm_create_soptions(fs);
  llsm_gpu_context* ctx = llsm_gpu_create_context(0, NULL);
  CHECK(ctx != NULL);
  llsm_gpu_batch* bank = llsm_gpu_create_batch(ctx, oa, fs, NUTT, nx, nfrm);
  CHECK(bank != NULL);
  CHECK(llsm_gpu_batch_upload(bank, LLSM_GPU_X, x, sizeof(FP_TYPE) * (size_t)xtot) == 0);
  CHECK(llsm_gpu_batch_upload(bank, LLSM_GPU_F0, f0, sizeof(FP_TYPE) * (size_t)ftot) == 0);
  CHECK(llsm_gpu_batch_analyze(bank) == 0);
  int radius[NDST];
  for(int i = 0; i < NDST; i ++) radius[i] = 1;
  CHECK(llsm_gpu_batch_smooth(bank, radius, LLSM_GPU_SMOOTH_ALL) == -1);     /* refused while there is no layer 1 */
  CHECK(llsm_gpu_batch_tolayer1(bank, 1024) == 0);

  /* the index list: frames 30 ... 69 of utterance 0, then frames 90 ... 129 of utterance 1 */
  int utt[NDST]; FP_TYPE pos[NDST];
  for(int i = 0; i < NDST; i ++) { utt[i] = i < HALF ? 0 : 1; pos[i] = (FP_TYPE)(i < HALF ? 30 + i : 90 + i - HALF); }
  const int nx_dst = 0, nfrm_dst = NDST;
  llsm_gpu_batch* dst = llsm_gpu_create_batch(ctx, oa, fs, 1, & nx_dst, & nfrm_dst);
  CHECK(dst != NULL);
  llsm_gpu_splice_map map;
  memset(& map, 0, sizeof(map));
  map.utt_a = utt; map.pos_a = pos;
  CHECK(llsm_gpu_batch_splice(dst, bank, & map) == 0);
  FP_TYPE before[NDST], after[NDST];
  CHECK(llsm_gpu_batch_download(dst, LLSM_GPU_F0, before, sizeof(before)) == 0);

  CHECK(llsm_gpu_join_radii(1, & nfrm_dst, utt, pos, REACH, radius) == 1);
  CHECK(radius[HALF - 1] == REACH && radius[HALF] == REACH && radius[HALF - 2] == REACH - 1);
  CHECK(radius[HALF - 1 - REACH] == 0 && radius[HALF + REACH] == 0 && radius[0] == 0 && radius[NDST - 1] == 0);
  CHECK(llsm_gpu_batch_smooth(dst, radius, LLSM_GPU_SMOOTH_ALL) == 0);
  CHECK(llsm_gpu_batch_download(dst, LLSM_GPU_F0, after, sizeof(after)) == 0);
  const double step0 = fabs((double)before[HALF] - before[HALF - 1]), step1 = fabs((double)after[HALF] - after[HALF - 1]);
  printf("smooth_batch: F0 step across the join: %.3f Hz -> %.3f Hz\n", step0, step1);
  CHECK(before[HALF - 1] > 0 && before[HALF] > 0 && step1 < step0);
  for(int i = 0; i < NDST; i ++) if(radius[i] == 0) CHECK(memcmp(& before[i], & after[i], sizeof(FP_TYPE)) == 0);

  CHECK(llsm_gpu_batch_tolayer0(dst, 1) == 0);
  CHECK(llsm_gpu_batch_synthesize(dst, os, 5, 0) == 0);
  llsm_gpu_layout lay;
  CHECK(llsm_gpu_batch_layout(dst, & lay) == 0);
  FP_TYPE* y = (FP_TYPE*)malloc(sizeof(FP_TYPE) * (size_t)lay.total_out);
  CHECK(llsm_gpu_batch_download(dst, LLSM_GPU_Y, y, sizeof(FP_TYPE) * (size_t)lay.total_out) == 0);
  int bad = 0; double e = 0;
  for(int t = 0; t < lay.total_out; t ++) { if(!isfinite(y[t])) bad ++; e += (double)y[t] * y[t]; }
  printf("smooth_batch: %d samples, rms %.4f, non-finite %d\n", lay.total_out, sqrt(e / (lay.total_out > 0 ? lay.total_out : 1)), bad);
  CHECK(lay.total_out > 0 && bad == 0 && sqrt(e / lay.total_out) > 1e-3);

  /* refusals */
  CHECK(llsm_gpu_batch_smooth(NULL, radius, LLSM_GPU_SMOOTH_ALL) == -1);
  CHECK(llsm_gpu_batch_smooth(dst, NULL, LLSM_GPU_SMOOTH_ALL) == -1);
  CHECK(llsm_gpu_batch_smooth(dst, radius, 32) == -1);
  radius[7] = LLSM_GPU_SMOOTH_MAX_RADIUS + 1;
  CHECK(llsm_gpu_batch_smooth(dst, radius, LLSM_GPU_SMOOTH_F0) == -1);
  radius[7] = -1;
  CHECK(llsm_gpu_batch_smooth(dst, radius, LLSM_GPU_SMOOTH_F0) == -1);
  CHECK(llsm_gpu_join_radii(1, & nfrm_dst, utt, pos, LLSM_GPU_SMOOTH_MAX_RADIUS + 1, radius) == -1);
  CHECK(llsm_gpu_join_radii(1, & nfrm_dst, utt, NULL, REACH, radius) == -1);

  llsm_gpu_delete_batch(dst); llsm_gpu_delete_batch(bank); llsm_gpu_delete_context(ctx);
  llsm_delete_aoptions(oa); llsm_delete_soptions(os);
  free(x); free(f0); free(y);
  printf("smooth_batch ok\n");
  return 0;
}
