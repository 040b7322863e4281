// coder_kernels.hip -- what llsm_gpu_batch_decode (batch_coder.cpp) writes besides the rows of k_coder_decode
// (l1_kernels.hip): the members the host decoder leaves as llsm_create_frame(nhar, nchannel, maxnhar_e, npsd) made them,
// as llsm_chunk_to_flat / llsm_chunk_to_flat_l1 flatten them.
//
//   k_batch_decode_rest   per frame: EDC = 1e-5 on every channel, NHAR_E = maxnhar_e with zero EENV_AMPL / EENV_PHSE rows,
//                         HAS_PSDRES = 0, PBPSYN = 0; decoding to layer 0, zero AMPL / PHSE rows on frames without harmonics
//                         (k_coder_decode writes those rows on frames with harmonics only).  Four frames per 256-thread
//                         workgroup, one wavefront each; runs after k_coder_decode on the same stream (it reads NHAR).
//
// The transforms themselves stay with k_coder_encode / k_coder_decode, one wavefront per frame: a 16-frame MFMA tile kernel
// for the two cosine transforms was measured slower per frame in both directions and was not kept.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "launch.h"

__global__ __launch_bounds__(256) void k_batch_decode_rest(ModRows r, int use_l1) {
  const int g = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if(g >= r.nframes) return;
  const size_t G = (size_t)g;
  const int nch = r.nchannel, me = r.maxnhar_e > 0 ? r.maxnhar_e : 1, mh = r.maxnhar;
  if(lane == 0) { r.nhar_e[g] = r.maxnhar_e; r.has_psdres[g] = 0; r.pbpsyn[g] = 0; }
  for(int k = lane; k < nch; k += 64) r.edc[G * nch + k] = 1e-5f;
  for(int k = lane; k < nch * me; k += 64) { r.eenv_ampl[G * nch * me + k] = 0.0f; r.eenv_phse[G * nch * me + k] = 0.0f; }
  if(! use_l1 && r.nhar[g] <= 0)
    for(int k = lane; k < mh; k += 64) { r.ampl[G * mh + k] = 0.0f; r.phse[G * mh + k] = 0.0f; }
}

int launch_batch_decode_rest(LaunchCtx* P, const ModRows& r, int use_l1) {
  if(r.nframes <= 0) return 0;
  LAUNCH("k_batch_decode_rest", k_batch_decode_rest, dim3((r.nframes + 3) / 4), dim3(256), 0, r, use_l1);
  return 0;
}
