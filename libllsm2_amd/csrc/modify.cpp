// modify.cpp -- edits of a device-resident batch between analysis and synthesis: host side of modify_kernels.hip.
//
//   llsm_gpu_batch_phasesync_rps     llsm_chunk_phasesync_rps over every frame (model.cpp)
//   llsm_gpu_batch_phasepropagate    llsm_chunk_phasepropagate per utterance (model.cpp)
//   llsm_gpu_batch_retime            the frame-blending step of the reference's time-stretch recipe, onto the frame grid
//                                    of another batch (rules: llsm_gpu.h)
//   llsm_gpu_retime_uniform_positions  the map retime uses when it is given none
//   llsm_gpu_batch_splice            retime's pair rule across utterances and between two sides: unit selection, joins with
//                                    cross-fades and morphs from index lists (rules: llsm_gpu.h)
//   llsm_gpu_batch_pitch_formant     F0 and formant ratios per frame on a layer-1 batch, the edit of the reference's
//                                    pitch-shift recipe (rules: llsm_gpu.h)
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "batch.h"

namespace {
const double kPi = 3.14159265358979323846;

int launch_failed(const char* what, int rc) {
  llsm_set_error(std::string(what) + ": launch failed: " + hipGetErrorString((hipError_t)rc));
  return -1;
}

int refuse(const std::string& why) { llsm_set_error("llsm_gpu_batch_retime: " + why); return -1; }
}  // namespace

extern "C" int llsm_gpu_batch_phasesync_rps(llsm_gpu_batch* b, int layer1_based) {
  if(! b) { llsm_set_error("llsm_gpu_batch_phasesync_rps: NULL batch"); return -1; }
  hipSetDevice(b -> ctx -> device);
  const int rc = launch_phase_shift(& b -> ctx -> lc, mod_rows(b), nullptr, layer1_based);
  return rc ? launch_failed("llsm_gpu_batch_phasesync_rps", rc) : 0;
}

extern "C" int llsm_gpu_batch_phasepropagate(llsm_gpu_batch* b, int sign) {
  if(! b) { llsm_set_error("llsm_gpu_batch_phasepropagate: NULL batch"); return -1; }
  const int F = b -> lay.total_frames;
  if(F == 0) return 0;
  hipSetDevice(b -> ctx -> device);
  if(b -> mod_theta.alloc((size_t)F)) return -1;
  // the factor of model.cpp's llsm_chunk_phasepropagate, formed the same way: (double)(float)(thop * sign) * 2 * pi
  const double k2pi = (double)(float)(b -> opt.thop * (float)sign) * 2.0 * kPi;
  LaunchCtx* P = & b -> ctx -> lc;
  int rc = launch_phase_propagate_theta(P, b -> lay.n_utt, b -> d_frm_off.p, b -> d_nfrm.p, (const float*)b -> arr[LLSM_GPU_F0],
    k2pi, b -> mod_theta.p);
  if(! rc) rc = launch_phase_shift(P, mod_rows(b), b -> mod_theta.p, 0);
  return rc ? launch_failed("llsm_gpu_batch_phasepropagate", rc) : 0;
}

extern "C" void llsm_gpu_retime_uniform_positions(int nfrm_src, int nfrm_dst, FP_TYPE* pos) {
  if(! pos || nfrm_dst <= 0) return;
  const float last = (float)(nfrm_src - 1);
  for(int i = 0; i < nfrm_dst; i ++) {
    const float t = (float)i * (float)nfrm_src / (float)nfrm_dst;
    pos[i] = t < last ? t : last;
  }
}

extern "C" int llsm_gpu_batch_retime(llsm_gpu_batch* dst, const llsm_gpu_batch* src_c, const FP_TYPE* pos,
  const int* psdres_src) {
  llsm_gpu_batch* src = const_cast<llsm_gpu_batch*>(src_c);         // read only: the rows are not changed
  if(! dst || ! src) return refuse("NULL batch");
  if(src == dst) return refuse("src and dst are the same batch");
  if(src -> ctx != dst -> ctx) return refuse("the two batches are on different contexts");
  const llsm_aoptions& a = src -> opt; const llsm_aoptions& d = dst -> opt;
  if(a.thop != d.thop || src -> fs != dst -> fs || a.nchannel != d.nchannel || a.npsd != d.npsd || a.maxnhar != d.maxnhar ||
     a.maxnhar_e != d.maxnhar_e || src -> chanfreq != dst -> chanfreq)
    return refuse("the batches were created with different options or sampling rates");
  if(src -> lay.n_utt != dst -> lay.n_utt) return refuse("the batches hold different numbers of utterances");
  if(src -> l1_nspec == 0) return refuse("src has no layer 1 (llsm_gpu_batch_tolayer1)");
  if(dst -> l1_nspec != 0 && dst -> l1_nspec != src -> l1_nspec) return refuse("dst has layer 1 enabled with another size");
  const int n_utt = dst -> lay.n_utt, Fd = dst -> lay.total_frames;
  for(int u = 0; u < n_utt; u ++)
    if((src -> nfrm[u] == 0) != (dst -> nfrm[u] == 0))
      return refuse("utterance " + std::to_string(u) + " has frames on one side only");
  // the map: positions checked (and formed, without one) on the host, then staged in page-locked memory
  if(dst -> mod_ev) HIP_OK(hipEventSynchronize(dst -> mod_ev));    // the previous call's copy has left the stage
  if(! dst -> mod_stage.resize(2 * (size_t)Fd + 1)) return -1;
  float* hpos = (float*)dst -> mod_stage.data(); int* hres = dst -> mod_stage.data() + Fd;
  for(int u = 0; u < n_utt; u ++) {
    const int n = src -> nfrm[u], m = dst -> nfrm[u], o = dst -> frm_off[u];
    if(pos) {
      const float last = (float)(n - 1);
      for(int i = 0; i < m; i ++) {
        const float t = pos[o + i];
        if(!(t >= 0.0f && t <= last))
          return refuse("position " + std::to_string(o + i) + " (utterance " + std::to_string(u) + ") is NaN or outside [0, " +
            std::to_string(n - 1) + "]");
        hpos[o + i] = t;
      }
    } else llsm_gpu_retime_uniform_positions(n, m, hpos + o);
    if(psdres_src)
      for(int i = 0; i < m; i ++) {
        const int k = psdres_src[o + i];
        if(k < 0 || k >= n)
          return refuse("psdres_src[" + std::to_string(o + i) + "] = " + std::to_string(k) + " is not a frame of utterance " +
            std::to_string(u));
        hres[o + i] = k;
      }
  }
  // accepted: from here on dst changes
  hipSetDevice(dst -> ctx -> device);
  if(llsm_gpu_batch_enable_layer1(dst, (src -> l1_nspec - 1) * 2)) return -1;
  dst -> fnyq = src -> fnyq;
  dst -> maxnhar_conf = src -> maxnhar_conf;
  dst -> min_f0 = 0; dst -> f0_unknown = true;           // the F0 row is written on the device
  if(Fd == 0) return 0;
  hipStream_t st = dst -> ctx -> stream;
  if(dst -> mod_pos.alloc((size_t)Fd) || (psdres_src && dst -> mod_res.alloc((size_t)Fd))) return -1;
  HIP_OK(hipMemcpyAsync(dst -> mod_pos.p, hpos, (size_t)Fd * sizeof(float), hipMemcpyHostToDevice, st));
  if(psdres_src) HIP_OK(hipMemcpyAsync(dst -> mod_res.p, hres, (size_t)Fd * sizeof(int), hipMemcpyHostToDevice, st));
  if(! dst -> mod_ev) HIP_OK(hipEventCreateWithFlags(& dst -> mod_ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(dst -> mod_ev, st));
  RetimeMap m;
  m.pos = dst -> mod_pos.p; m.res = psdres_src ? dst -> mod_res.p : nullptr; m.utt = dst -> d_frm_utt.p;
  m.src_off = src -> d_frm_off.p; m.src_nfrm = src -> d_nfrm.p;
  const int rc = launch_retime(& dst -> ctx -> lc, mod_rows(src), mod_rows(dst), m);
  return rc ? launch_failed("llsm_gpu_batch_retime", rc) : 0;
}

namespace {
int refuse_sp(const std::string& why) { llsm_set_error("llsm_gpu_batch_splice: " + why); return -1; }

// One side of a splice map resolved into `ga` (flat source frame a) and `r`, formed from the position exactly as k_retime
// forms them; utt NULL: the output frame's own utterance.  Returns false (error set) at the first bad entry.
bool stage_side(const llsm_gpu_batch* src, const llsm_gpu_batch* dst, const char* side, const int* utt, const float* pos,
  int* ga, float* r) {
  const int n_src = src -> lay.n_utt;
  for(int u = 0; u < dst -> lay.n_utt; u ++)
    for(int g = dst -> frm_off[u]; g < dst -> frm_off[u] + dst -> nfrm[u]; g ++) {
      const int v = utt ? utt[g] : u;
      const std::string where = std::string(side) + "[" + std::to_string(g) + "]";
      if(v < 0 || v >= n_src) {
        refuse_sp("utt_" + where + " = " + std::to_string(v) + " is not an utterance of src (" + std::to_string(n_src) + ")");
        return false;
      }
      const int n = src -> nfrm[v];
      if(n == 0) { refuse_sp("utt_" + where + " = " + std::to_string(v) + " names an utterance without frames"); return false; }
      const float t = pos[g];
      if(!(t >= 0.0f && t <= (float)(n - 1))) {
        refuse_sp("pos_" + where + " (utterance " + std::to_string(v) + ") is NaN or outside [0, " + std::to_string(n - 1) + "]");
        return false;
      }
      int a = 0; float ra = 0;
      if(n > 1) { const int fl = (int)std::floor(t); a = fl < n - 2 ? fl : n - 2; ra = t - (float)a; }
      ga[g] = src -> frm_off[v] + a; r[g] = ra;
    }
  return true;
}
}  // namespace

extern "C" int llsm_gpu_batch_splice(llsm_gpu_batch* dst, const llsm_gpu_batch* src_c, const llsm_gpu_splice_map* map) {
  llsm_gpu_batch* src = const_cast<llsm_gpu_batch*>(src_c);         // read only: the rows are not changed
  if(! dst || ! src) return refuse_sp("NULL batch");
  if(! map) return refuse_sp("NULL map");
  if(! map -> pos_a) return refuse_sp("pos_a is NULL");
  const bool two = map -> utt_b || map -> pos_b || map -> mix;
  if(two && !(map -> utt_b && map -> pos_b && map -> mix))
    return refuse_sp("the second side is given in part: utt_b, pos_b and mix are all NULL or all given");
  if(src == dst) return refuse_sp("src and dst are the same batch");
  if(src -> ctx != dst -> ctx) return refuse_sp("the two batches are on different contexts");
  const llsm_aoptions& a = src -> opt; const llsm_aoptions& d = dst -> opt;
  if(a.thop != d.thop || src -> fs != dst -> fs || a.nchannel != d.nchannel || a.npsd != d.npsd || a.maxnhar != d.maxnhar ||
     a.maxnhar_e != d.maxnhar_e || src -> chanfreq != dst -> chanfreq)
    return refuse_sp("the batches were created with different options or sampling rates");
  if(src -> l1_nspec == 0) return refuse_sp("src has no layer 1 (llsm_gpu_batch_tolayer1)");
  if(dst -> l1_nspec != 0 && dst -> l1_nspec != src -> l1_nspec) return refuse_sp("dst has layer 1 enabled with another size");
  if(! map -> utt_a && dst -> lay.n_utt > src -> lay.n_utt)
    return refuse_sp("utt_a is NULL and dst holds more utterances (" + std::to_string(dst -> lay.n_utt) + ") than src (" +
      std::to_string(src -> lay.n_utt) + ")");
  // the map: checked and resolved on the host, then staged in page-locked memory ([ga | ra] and, with a second side,
  // [gb | rb | mix], Fd words each)
  const int Fd = dst -> lay.total_frames;
  const size_t words = (two ? 5 : 2) * (size_t)Fd;
  if(dst -> mod_ev) HIP_OK(hipEventSynchronize(dst -> mod_ev));    // the previous call's copy has left the stage
  if(! dst -> mod_stage.resize(words + 1)) return -1;
  int* h = dst -> mod_stage.data();
  if(! stage_side(src, dst, "a", map -> utt_a, map -> pos_a, h, (float*)h + Fd)) return -1;
  if(two) {
    if(! stage_side(src, dst, "b", map -> utt_b, map -> pos_b, h + 2 * (size_t)Fd, (float*)h + 3 * (size_t)Fd)) return -1;
    float* hmix = (float*)h + 4 * (size_t)Fd;
    for(int g = 0; g < Fd; g ++) {
      const float w = map -> mix[g];
      if(!(w >= 0.0f && w <= 1.0f)) return refuse_sp("mix[" + std::to_string(g) + "] is NaN or outside [0, 1]");
      hmix[g] = w;
    }
  }
  // accepted: from here on dst changes
  hipSetDevice(dst -> ctx -> device);
  if(llsm_gpu_batch_enable_layer1(dst, (src -> l1_nspec - 1) * 2)) return -1;
  dst -> fnyq = src -> fnyq;
  dst -> maxnhar_conf = src -> maxnhar_conf;
  dst -> min_f0 = 0; dst -> f0_unknown = true;           // the F0 row is written on the device
  if(Fd == 0) return 0;
  hipStream_t st = dst -> ctx -> stream;
  if(dst -> mod_splice.alloc(words)) return -1;
  int* dm = dst -> mod_splice.p;
  HIP_OK(hipMemcpyAsync(dm, h, words * sizeof(int), hipMemcpyHostToDevice, st));
  if(! dst -> mod_ev) HIP_OK(hipEventCreateWithFlags(& dst -> mod_ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(dst -> mod_ev, st));
  SpliceMap m;
  m.ga = dm; m.ra = (const float*)dm + Fd;
  m.gb = two ? dm + 2 * (size_t)Fd : nullptr; m.rb = two ? (const float*)dm + 3 * (size_t)Fd : nullptr;
  m.mix = two ? (const float*)dm + 4 * (size_t)Fd : nullptr;
  const int rc = launch_splice(& dst -> ctx -> lc, mod_rows(src), mod_rows(dst), m);
  return rc ? launch_failed("llsm_gpu_batch_splice", rc) : 0;
}

namespace {
int refuse_pf(const std::string& why) { llsm_set_error("llsm_gpu_batch_pitch_formant: " + why); return -1; }

// ratios of frames [0, F) into `out` (NULL: all 1), each within [lo, hi]; first / last frame with a ratio != 1 widen
// [*g_lo, *g_hi), *mn takes the smallest.  Returns false (error set) on the first bad value.
bool stage_ratios(const float* v, int F, float lo, float hi, const char* name, const char* range, float* out, int* g_lo,
  int* g_hi, float* mn) {
  if(! v) return true;
  for(int g = 0; g < F; g ++) {
    const float x = v[g];
    if(!(x >= lo && x <= hi)) {
      refuse_pf(std::string(name) + " of frame " + std::to_string(g) + " (" + std::to_string(x) +
        ") is NaN, infinite or outside " + range);
      return false;
    }
    out[g] = x;
    if(x != 1.0f) { if(g < *g_lo) *g_lo = g; if(g + 1 > *g_hi) *g_hi = g + 1; }
    if(x < *mn) *mn = x;
  }
  return true;
}
}  // namespace

extern "C" int llsm_gpu_batch_pitch_formant(llsm_gpu_batch* b, const FP_TYPE* f0_ratio, const FP_TYPE* formant_ratio,
  int flags) {
  if(! b) return refuse_pf("NULL batch");
  if(b -> l1_nspec == 0) return refuse_pf("the batch has no layer 1 (llsm_gpu_batch_tolayer1)");
  if(flags & ~LLSM_GPU_WARP_PSD) return refuse_pf("unknown flag bits " + std::to_string(flags & ~LLSM_GPU_WARP_PSD));
  const size_t lds = (size_t)4 * (b -> l1_nspec + b -> lay.npsd) * sizeof(float);
  if(lds > 160 * 1024) return refuse_pf("nspec + npsd = " + std::to_string(b -> l1_nspec + b -> lay.npsd) +
    " floats per frame do not fit the kernel's LDS (at most 10240)");
  const int F = b -> lay.total_frames;
  // the ratios: checked on the host, then staged in page-locked memory ([2][F]: F0, formant)
  if(b -> mod_ev) HIP_OK(hipEventSynchronize(b -> mod_ev));       // the previous call's copy has left the stage
  if(! b -> mod_stage.resize(2 * (size_t)F + 1)) return -1;
  float* hr = (float*)b -> mod_stage.data(); float* ha = hr + F;
  int g_lo = F, g_hi = 0; float rho_min = 1.0f, alpha_min = 1.0f;
  if(! stage_ratios(f0_ratio, F, 1.0f / 16.0f, 16.0f, "f0_ratio", "[1/16, 16]", hr, & g_lo, & g_hi, & rho_min)) return -1;
  if(! stage_ratios(formant_ratio, F, 0.25f, 4.0f, "formant_ratio", "[1/4, 4]", ha, & g_lo, & g_hi, & alpha_min)) return -1;
  if(g_hi <= g_lo) return 0;                                       // every ratio is 1: nothing changes
  // accepted: from here on the batch changes.  Lowest voiced F0: every voiced F0' = fl(F0 rho) >= fl(min_f0 rho_min)
  // (rounding is monotonic), so the product stays a lower bound of the new rows; unknown stays unknown.
  if(b -> min_f0 > 0 && ! b -> f0_unknown) b -> min_f0 = b -> min_f0 * rho_min;
  hipSetDevice(b -> ctx -> device);
  hipStream_t st = b -> ctx -> stream;
  if(b -> mod_ratio.alloc(2 * (size_t)F)) return -1;
  float* dr = f0_ratio ? b -> mod_ratio.p : nullptr;
  float* da = formant_ratio ? b -> mod_ratio.p + F : nullptr;
  if(dr) HIP_OK(hipMemcpyAsync(dr, hr, (size_t)F * sizeof(float), hipMemcpyHostToDevice, st));
  if(da) HIP_OK(hipMemcpyAsync(da, ha, (size_t)F * sizeof(float), hipMemcpyHostToDevice, st));
  if(! b -> mod_ev) HIP_OK(hipEventCreateWithFlags(& b -> mod_ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(b -> mod_ev, st));
  const int rc = launch_pitch_formant(& b -> ctx -> lc, mod_rows(b), g_lo, g_hi, dr, da, flags & LLSM_GPU_WARP_PSD);
  return rc ? launch_failed("llsm_gpu_batch_pitch_formant", rc) : 0;
}
