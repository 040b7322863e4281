// batch_coder.cpp -- the frame coder on a device-resident batch (rules: llsm_gpu.h).
//
//   llsm_gpu_batch_enable_coder      allocates LLSM_GPU_CODE and builds the mel axis
//   llsm_gpu_batch_coder_dimension   order_spec + order_bap + 3, 0 before enable_coder
//   llsm_gpu_batch_encode            rows -> LLSM_GPU_CODE
//   llsm_gpu_batch_decode            LLSM_GPU_CODE -> rows (layer 1 or layer 0)
//
// The kernels are the host API's (coder.cpp: k_coder_encode / k_coder_decode, one wavefront per frame), launched on the
// batch's own rows: no containers, no copies.  A tile kernel with the transforms on the MFMA was measured slower per frame
// and was not kept.  k_batch_decode_rest (coder_kernels.hip) adds the rows the host decoder leaves
// at their llsm_create_frame values.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "batch.h"

namespace {
const size_t kLdsMax = 160 * 1024;

int refuse(const char* fn, const std::string& why) { llsm_set_error(std::string(fn) + ": " + why); return -1; }

double freq2mel(double f) { return 1127.01048 * std::log(1.0 + f / 700.0); }
double mel2freq(double m) { return 700.0 * (std::exp(m / 1127.01048) - 1.0); }

// LDS of one workgroup of k_coder_encode (use_l1 < 0) / k_coder_decode, as their launchers size it (l1_kernels.hip): three
// float rows of nspec bins, and for decode two rows of maxnhar harmonics and the minimum-phase transform with its twiddles
size_t lds_bytes(int nspec, int maxnhar, int use_l1) {
  size_t n = sizeof(float) * 3 * (size_t)nspec;
  if(use_l1 < 0) return n;
  const int nmax = l1_minphase_nmax(maxnhar);
  return n + sizeof(float) * 2 * (size_t)((maxnhar + 3) & ~3) + sizeof(float2) * ((size_t)nmax + nmax / 2);
}
std::string lds_message(int nspec, int maxnhar, size_t need) {
  return "rows too long for the kernel's LDS: nspec = " + std::to_string(nspec) + " bins and maxnhar = " + std::to_string(maxnhar) +
    " harmonics need " + std::to_string(need) + " bytes, at most " + std::to_string(kLdsMax);
}
int launch_failed(const char* fn, int rc) {
  return refuse(fn, rc > 0 ? std::string("launch failed: ") + hipGetErrorString((hipError_t)rc) : "unsupported configuration");
}
}  // namespace

extern "C" int llsm_gpu_batch_enable_coder(llsm_gpu_batch* b, int order_spec, int order_bap) {
  const char* fn = "llsm_gpu_batch_enable_coder";
  if(! b) return refuse(fn, "NULL batch");
  if(b -> l1_nspec == 0) return refuse(fn, "the batch has no layer 1 (llsm_gpu_batch_enable_layer1 / _tolayer1)");
  const int ns = b -> l1_nspec, N = ns - 1;
  if(order_spec < 1 || order_bap < 1 || order_spec > N)
    return refuse(fn, "orders out of range: order_spec in [1, nspec - 1 = " + std::to_string(N) + "], order_bap >= 1");
  if(ns < 33 || (N & (N - 1))) return refuse(fn, "nspec - 1 = " + std::to_string(N) + " is not a power of two >= 32");
  if(order_spec == b -> coder_os && order_bap == b -> coder_ob) return 0;
  const size_t need = lds_bytes(ns, b -> lay.maxnhar, -1);
  if(need > kLdsMax) return refuse(fn, lds_message(ns, b -> lay.maxnhar, need));
  hipSetDevice(b -> ctx -> device);
  hipStream_t st = b -> ctx -> stream;
  const size_t bytes = (size_t)b -> lay.total_frames * (order_spec + order_bap + 3) * sizeof(float);
  void* code = nullptr;
  if(bytes) {
    const hipError_t e = llsm_dev_malloc(& code, bytes);
    if(e != hipSuccess) return refuse(fn, std::string("hipMalloc(LLSM_GPU_CODE): ") + hipGetErrorString(e));
  }
  if(! b -> coder_mel.p) {                              // the mel axis of llsm_create_coder (coder.c:67-72): orders do not enter
    const double ceil_ = freq2mel(b -> fnyq), floor_ = freq2mel(50);
    std::vector<float> mel(ns);
    for(int i = 0; i < ns; i ++) mel[i] = (float)mel2freq(floor_ + (ceil_ - floor_) * i / ns);
    if(upload_vec(b -> coder_mel, mel)) { llsm_dev_free(code); return -1; }
    b -> coder_mel_floor = (float)floor_; b -> coder_mel_ceil = (float)ceil_;
  }
  HIP_OK(hipStreamSynchronize(st));                       // earlier launches may still use the old array
  llsm_dev_free(b -> arr[LLSM_GPU_CODE]);
  b -> arr[LLSM_GPU_CODE] = code; b -> arr_bytes[LLSM_GPU_CODE] = bytes;
  b -> coder_os = order_spec; b -> coder_ob = order_bap;
  if(bytes) HIP_OK(hipMemsetAsync(code, 0, bytes, st));
  return 0;
}

extern "C" int llsm_gpu_batch_coder_dimension(llsm_gpu_batch* b) {
  return (b && b -> coder_os > 0) ? b -> coder_os + b -> coder_ob + 3 : 0;
}

extern "C" int llsm_gpu_batch_encode(llsm_gpu_batch* b) {
  const char* fn = "llsm_gpu_batch_encode";
  if(! b) return refuse(fn, "NULL batch");
  if(b -> l1_nspec == 0) return refuse(fn, "the batch has no layer 1 (llsm_gpu_batch_tolayer1)");
  if(b -> coder_os == 0) return refuse(fn, "coder not enabled (llsm_gpu_batch_enable_coder)");
  hipSetDevice(b -> ctx -> device);
  const ModRows r = mod_rows(b);
  const int rc = launch_coder_encode(& b -> ctx -> lc, b -> coder_os, b -> coder_ob, r.nspec, r.npsd, b -> fnyq, b -> opt.lip_radius,
    b -> coder_mel.p, r.nframes, r.f0, r.rd, r.psd, r.vtmagn, r.nvsphse, (float*)b -> arr[LLSM_GPU_CODE]);
  return rc ? launch_failed(fn, rc) : 0;
}

extern "C" int llsm_gpu_batch_decode(llsm_gpu_batch* b, int use_layer1) {
  const char* fn = "llsm_gpu_batch_decode";
  if(! b) return refuse(fn, "NULL batch");
  if(b -> l1_nspec == 0) return refuse(fn, "the batch has no layer 1 (llsm_gpu_batch_enable_layer1)");
  if(b -> coder_os == 0) return refuse(fn, "coder not enabled (llsm_gpu_batch_enable_coder)");
  if(use_layer1 != 0 && use_layer1 != 1) return refuse(fn, "use_layer1 = " + std::to_string(use_layer1) + " is not 0 or 1");
  const ModRows r = mod_rows(b);
  const size_t need = lds_bytes(r.nspec, r.maxnhar, use_layer1);
  if(need > kLdsMax) return refuse(fn, lds_message(r.nspec, r.maxnhar, need));
  int tw_nmax = 0; const float2* tw = llsm_engine_twiddles(b -> ctx, & tw_nmax);
  if(l1_minphase_nmax(r.maxnhar) > tw_nmax)
    return refuse(fn, "maxnhar = " + std::to_string(r.maxnhar) + " needs a larger minimum-phase transform than the context holds");
  // accepted: from here on the batch changes.  The F0 row is written on the device.
  b -> min_f0 = 0; b -> f0_unknown = true;
  hipSetDevice(b -> ctx -> device);
  LaunchCtx* P = & b -> ctx -> lc;
  int rc = launch_coder_decode(P, b -> coder_os, b -> coder_ob, r.nspec, r.npsd, r.maxnhar, b -> fnyq, b -> opt.lip_radius,
    b -> coder_mel.p, b -> coder_mel_floor, b -> coder_mel_ceil, r.nframes, (const float*)b -> arr[LLSM_GPU_CODE], use_layer1, tw,
    tw_nmax, r.f0, r.rd, r.nhar, r.ampl, r.phse, r.psd, r.vtmagn, r.vsphse, r.nvsphse, r.has_hm);
  if(! rc) rc = launch_batch_decode_rest(P, r, use_layer1);
  return rc ? launch_failed(fn, rc) : 0;
}
