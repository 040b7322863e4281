// f0.cpp -- F0 estimation of a batch's waveforms on the device: host side of f0_kernels.hip.
//
//   llsm_gpu_f0_default_options   the defaults of llsm_gpu.h
//   llsm_gpu_f0_plan              host only: the sizes the options imply at a sampling rate, and every refusal that needs no batch
//   llsm_gpu_batch_estimate_f0    LLSM_GPU_X -> LLSM_GPU_F0 (rules: llsm_gpu.h): the utterances' sums
//                                 of squares (k_f0_energy), rules 2 - 7 per frame (k_f0_cmndf_wf), rule 8 (k_f0_median)
//   llsm_gpu_f0_track_default_options, llsm_gpu_f0_track_check   the same for the options of the tracker
//   llsm_gpu_batch_track_f0       LLSM_GPU_X -> LLSM_GPU_F0 through a path search (rules T1 - T5: llsm_gpu.h, DESIGN.md
//                                 section 22): k_f0_energy, rules 2 - 5 and T1 per frame (k_f0_cmndf_wf<, true>) into the
//                                 candidate plane, rules T2 - T5 per utterance (k_f0_viterbi)
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "batch.h"

namespace {
const char* kEstimate = "llsm_gpu_batch_estimate_f0";
const char* kTrack = "llsm_gpu_batch_track_f0";
const int kMaxFft = 4096;                                 // the largest transform of wave_fft.h

// every refusal below names the call it is made for
struct Refuse {
  const char* fn;
  int operator()(const std::string& why) const { llsm_set_error(std::string(fn) + ": " + why); return -1; }
};

struct F0Sizes { int lmin, lmax, W, nfft, logn; };

// the options checked and turned into sizes (rule 1); -1 with the error set
int plan(const llsm_gpu_f0_options& o, float fs, F0Sizes* z, Refuse refuse) {
  if(std::isnan(o.fmin) || std::isnan(o.fmax) || std::isnan(o.threshold) || std::isnan(o.silence_rel))
    return refuse("an option is NaN");
  if(!(fs > 0) || std::isinf(fs)) return refuse("the sampling rate is not a positive number");
  if(!(o.fmin > 0)) return refuse("fmin <= 0");
  if(!(o.fmin < o.fmax)) return refuse("fmin >= fmax");
  if(std::isinf(o.fmax)) return refuse("fmax is infinite");
  if(!(o.threshold > 0 && o.threshold <= 1)) return refuse("threshold outside (0, 1]");
  if(!(o.silence_rel >= 0) || std::isinf(o.silence_rel)) return refuse("silence_rel < 0 or infinite");
  if(o.window_extra < 1) return refuse("window_extra < 1");
  if(o.smooth != 0 && o.smooth != 1) return refuse("smooth is neither 0 nor 1");
  if(o.keep_cmndf != 0 && o.keep_cmndf != 1) return refuse("keep_cmndf is neither 0 nor 1");
  const double dmin = (double)fs / (double)o.fmax, dmax = (double)fs / (double)o.fmin;
  if(dmax + (double)o.window_extra > (double)kMaxFft)     // (also keeps the conversions to int below in range)
    return refuse("W + lmax > 4096, the largest transform");
  z -> lmin = (int)dmin; z -> lmax = (int)dmax;
  if(z -> lmin < 2) return refuse("lmin = (int)(fs / fmax) = " + std::to_string(z -> lmin) + " < 2");
  if(z -> lmax <= z -> lmin + 1)
    return refuse("lmax = " + std::to_string(z -> lmax) + " <= lmin + 1 = " + std::to_string(z -> lmin + 1));
  z -> W = z -> lmax + o.window_extra;
  if(z -> W + z -> lmax > kMaxFft)
    return refuse("W + lmax = " + std::to_string(z -> W + z -> lmax) + " > 4096, the largest transform");
  z -> nfft = 256; z -> logn = 8;
  while(z -> nfft < z -> W + z -> lmax) { z -> nfft *= 2; z -> logn ++; }
  return 0;
}

// the options of the tracker checked; -1 with the error set
int check_track(const llsm_gpu_f0_track_options& t) {
  const Refuse refuse{kTrack};
  const float v[5] = {t.cand_threshold, t.unvoiced_cost, t.switch_cost, t.jump_cost, t.octave_cost};
  for(float x : v) if(std::isnan(x)) return refuse("a track option is NaN");
  for(float x : v) if(std::isinf(x)) return refuse("a track option is infinite");
  if(!(t.cand_threshold > 0 && t.cand_threshold <= 1)) return refuse("cand_threshold outside (0, 1]");
  if(t.unvoiced_cost < 0) return refuse("unvoiced_cost < 0");
  if(t.switch_cost < 0) return refuse("switch_cost < 0");
  if(t.jump_cost < 0) return refuse("jump_cost < 0");
  if(t.octave_cost < 0) return refuse("octave_cost < 0");
  return 0;
}

// the batch's tables and waveforms and the sizes of the plan, as the kernels take them
F0Dev device_view(llsm_gpu_batch* b, const llsm_gpu_f0_options& o, const F0Sizes& z) {
  F0Dev d;
  d.n_utt = b -> lay.n_utt; d.nframes = b -> lay.total_frames; d.thop = b -> opt.thop; d.fs = b -> fs;
  d.x_off = b -> d_x_off.p; d.nx = b -> d_nx.p; d.frm_off = b -> d_frm_off.p; d.nfrm = b -> d_nfrm.p;
  d.frm_utt = b -> d_frm_utt.p; d.pairs = b -> d_pairs.p; d.npairs = b -> npairs;
  d.x = (const float*)b -> arr[LLSM_GPU_X];
  d.lmin = z.lmin; d.lmax = z.lmax; d.W = z.W;
  d.threshold = (double)o.threshold; d.gate = (double)o.silence_rel * (double)o.silence_rel;
  return d;
}
}  // namespace

extern "C" void llsm_gpu_f0_default_options(llsm_gpu_f0_options* dst) {
  if(! dst) return;
  dst -> fmin = 50; dst -> fmax = 500; dst -> threshold = 0.15f; dst -> silence_rel = 0.05f;
  dst -> window_extra = 200; dst -> smooth = 1; dst -> keep_cmndf = 0;
}

extern "C" int llsm_gpu_f0_plan(const llsm_gpu_f0_options* opt, FP_TYPE fs, int* lmin, int* lmax, int* W, int* nfft) {
  llsm_gpu_f0_options o;
  if(opt) o = *opt; else llsm_gpu_f0_default_options(& o);
  F0Sizes z;
  if(plan(o, fs, & z, Refuse{kEstimate})) return -1;
  if(lmin) *lmin = z.lmin;
  if(lmax) *lmax = z.lmax;
  if(W) *W = z.W;
  if(nfft) *nfft = z.nfft;
  return 0;
}

extern "C" int llsm_gpu_batch_estimate_f0(llsm_gpu_batch* b, const llsm_gpu_f0_options* opt) {
  const Refuse refuse{kEstimate};
  if(! b) return refuse("NULL batch");
  llsm_gpu_f0_options o;
  if(opt) o = *opt; else llsm_gpu_f0_default_options(& o);
  F0Sizes z;
  if(plan(o, b -> fs, & z, refuse)) return -1;
  const int F = b -> lay.total_frames;
  if(F > 0 && b -> lay.total_samples == 0) return refuse("the batch has frames but no samples");
  if(F == 0) return 0;
  // accepted: from here on the batch changes
  hipSetDevice(b -> ctx -> device);
  const int cols = z.lmax + 1;
  if(b -> f0_uss.alloc((size_t)b -> lay.n_utt) || (o.smooth && b -> f0_raw.alloc((size_t)F))) return -1;
  if(o.keep_cmndf) {
    if(b -> f0_cmndf.alloc((size_t)F * (size_t)cols)) return -1;
    b -> f0_cm_cols = cols;                                         // (a plane of another width is overwritten whole)
  }
  b -> min_f0 = 0; b -> f0_unknown = true;                          // the F0 row is written on the device
  const F0Dev d = device_view(b, o, z);
  LaunchCtx* P = & b -> ctx -> lc;
  float* f0 = (float*)b -> arr[LLSM_GPU_F0];
  int rc = launch_f0_energy(P, d, b -> f0_uss.p);
  if(! rc) rc = launch_f0_cmndf(P, d, z.logn, b -> f0_uss.p, o.smooth ? b -> f0_raw.p : f0, o.keep_cmndf ? b -> f0_cmndf.p : nullptr,
    F0Cand{nullptr, 0.0f, 0.0f});
  if(! rc && o.smooth) rc = launch_f0_median(P, d, b -> f0_raw.p, f0);
  if(rc) return refuse(std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" void llsm_gpu_f0_track_default_options(llsm_gpu_f0_track_options* dst) {
  if(! dst) return;
  dst -> cand_threshold = 0.5f; dst -> unvoiced_cost = 0.2f; dst -> switch_cost = 0.05f; dst -> jump_cost = 0.5f;
  dst -> octave_cost = 0.02f;
}

extern "C" int llsm_gpu_f0_track_check(const llsm_gpu_f0_track_options* topt) {
  llsm_gpu_f0_track_options t;
  if(topt) t = *topt; else llsm_gpu_f0_track_default_options(& t);
  return check_track(t);
}

extern "C" int llsm_gpu_batch_track_f0(llsm_gpu_batch* b, const llsm_gpu_f0_options* opt,
  const llsm_gpu_f0_track_options* topt) {
  const Refuse refuse{kTrack};
  if(! b) return refuse("NULL batch");
  llsm_gpu_f0_options o;
  if(opt) o = *opt; else llsm_gpu_f0_default_options(& o);
  llsm_gpu_f0_track_options t;
  if(topt) t = *topt; else llsm_gpu_f0_track_default_options(& t);
  F0Sizes z;
  if(plan(o, b -> fs, & z, refuse) || check_track(t)) return -1;
  const int F = b -> lay.total_frames;
  if(F > 0 && b -> lay.total_samples == 0) return refuse("the batch has frames but no samples");
  if(F == 0) return 0;
  // accepted: from here on the batch changes
  hipSetDevice(b -> ctx -> device);
  const int cols = z.lmax + 1;
  if(b -> f0_uss.alloc((size_t)b -> lay.n_utt) || b -> f0_cand.alloc((size_t)F * 24) || b -> f0_bp.alloc((size_t)F)) return -1;
  if(o.keep_cmndf) {
    if(b -> f0_cmndf.alloc((size_t)F * (size_t)cols)) return -1;
    b -> f0_cm_cols = cols;
  }
  b -> f0_cand_filled = true;
  b -> min_f0 = 0; b -> f0_unknown = true;                          // the F0 row is written on the device
  const F0Dev d = device_view(b, o, z);
  const F0Cand c{b -> f0_cand.p, t.cand_threshold, (float)std::log2((double)b -> fs / (double)z.lmin)};
  const F0Track costs{t.unvoiced_cost, t.switch_cost, t.jump_cost, t.octave_cost};
  LaunchCtx* P = & b -> ctx -> lc;
  int rc = launch_f0_energy(P, d, b -> f0_uss.p);
  if(! rc) rc = launch_f0_cmndf(P, d, z.logn, b -> f0_uss.p, nullptr, o.keep_cmndf ? b -> f0_cmndf.p : nullptr, c);
  if(! rc) rc = launch_f0_viterbi(P, d, c.plane, costs, b -> f0_bp.p, (float*)b -> arr[LLSM_GPU_F0]);
  if(rc) return refuse(std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
  return 0;
}
