// modify.cpp -- edits of a device-resident batch between analysis and synthesis: host side of modify_kernels.hip.
//
//   llsm_gpu_batch_phasesync_rps     llsm_chunk_phasesync_rps over every frame (model.cpp)
//   llsm_gpu_batch_phasepropagate    llsm_chunk_phasepropagate per utterance (model.cpp)
//   llsm_gpu_batch_retime            the frame-blending step of the reference's time-stretch recipe, onto the frame grid
//                                    of another batch (rules: llsm_gpu.h)
//   llsm_gpu_retime_uniform_positions  the map retime uses when it is given none
//   llsm_gpu_batch_splice            retime's pair rule across utterances and between two sides: unit selection, joins with
//                                    cross-fades and morphs from index lists (rules: llsm_gpu.h);
//                                    retime and splice share their refusals, their path to the device (fit, blend_frames)
//                                    and their kernel (k_splice)
//   llsm_gpu_batch_pitch_formant     F0 and formant ratios per frame on a layer-1 batch, the edit of the reference's
//                                    pitch-shift recipe (rules: llsm_gpu.h)
//   llsm_gpu_batch_smooth            triangular means of F0, RD, VTMAGN, PSD and EDC along the frames around joins, from a
//                                    snapshot of the rows (rules: llsm_gpu.h)
//   llsm_gpu_join_radii              the radii smooth takes, from the index lists splice renders
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "batch.h"

namespace {
const double kPi = 3.14159265358979323846;

int launch_failed(const char* what, int rc) {
  llsm_set_error(std::string(what) + ": launch failed: " + hipGetErrorString((hipError_t)rc));
  return -1;
}

int refuse(const char* fn, const std::string& why) { llsm_set_error(std::string(fn) + ": " + why); return -1; }
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

namespace {
// What llsm_gpu_batch_retime and llsm_gpu_batch_splice refuse alike: two batches that do not fit each other.  `fn` words the
// message.
int fit(const char* fn, const llsm_gpu_batch* dst, const llsm_gpu_batch* src) {
  if(! dst || ! src) return refuse(fn, "NULL batch");
  if(src == dst) return refuse(fn, "src and dst are the same batch");
  if(src -> ctx != dst -> ctx) return refuse(fn, "the two batches are on different contexts");
  const llsm_aoptions& a = src -> opt; const llsm_aoptions& d = dst -> opt;
  if(a.thop != d.thop || src -> fs != dst -> fs || a.nchannel != d.nchannel || a.npsd != d.npsd || a.maxnhar != d.maxnhar ||
     a.maxnhar_e != d.maxnhar_e || src -> chanfreq != dst -> chanfreq)
    return refuse(fn, "the batches were created with different options or sampling rates");
  if(src -> l1_nspec == 0) return refuse(fn, "src has no layer 1 (llsm_gpu_batch_tolayer1)");
  if(dst -> l1_nspec != 0 && dst -> l1_nspec != src -> l1_nspec) return refuse(fn, "dst has layer 1 enabled with another size");
  return 0;
}

// Position t of an utterance of n frames (0 <= t <= n - 1) as the pair rule takes it: frame *a and the weight *r of frame
// a + 1, with a = min(floor(t), n - 2) so that the last frame is reached through r = 1; a one-frame utterance is its frame.
inline void pair_at(float t, int n, int* a, float* r) {
  *a = 0; *r = 0;
  if(n > 1) { const int fl = (int)t; *a = fl < n - 2 ? fl : n - 2; *r = t - (float)*a; }   // (t >= 0: truncation is floor)
}

// The rest of what the two calls share, for batches that fit: the caller's map of `words` words, checked and written into
// the page-locked stage by resolve(h) (-1 with the error set: refused, dst untouched); dst made ready for src's frames; one
// copy of the map into mod_map; launch(dm) on the device copy.
template <class Resolve, class Launch>
int blend_frames(const char* fn, llsm_gpu_batch* dst, const llsm_gpu_batch* src, size_t words, Resolve resolve, Launch launch) {
  if(dst -> mod_ev) HIP_OK(hipEventSynchronize(dst -> mod_ev));    // the previous call's copy has left the stage
  if(! dst -> mod_stage.resize(words + 1)) return -1;
  if(resolve(dst -> mod_stage.data())) return -1;
  // accepted: from here on dst changes
  hipSetDevice(dst -> ctx -> device);
  if(llsm_gpu_batch_enable_layer1(dst, (src -> l1_nspec - 1) * 2)) return -1;
  dst -> fnyq = src -> fnyq;
  dst -> maxnhar_conf = src -> maxnhar_conf;
  dst -> min_f0 = 0; dst -> f0_unknown = true;           // the F0 row is written on the device
  if(dst -> lay.total_frames == 0) return 0;
  hipStream_t st = dst -> ctx -> stream;
  if(dst -> mod_map.alloc(words)) return -1;
  HIP_OK(hipMemcpyAsync(dst -> mod_map.p, dst -> mod_stage.data(), words * sizeof(int), hipMemcpyHostToDevice, st));
  if(! dst -> mod_ev) HIP_OK(hipEventCreateWithFlags(& dst -> mod_ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(dst -> mod_ev, st));
  const int rc = launch(dst -> mod_map.p);
  return rc ? launch_failed(fn, rc) : 0;
}
}  // namespace

extern "C" int llsm_gpu_batch_retime(llsm_gpu_batch* dst, const llsm_gpu_batch* src_c, const FP_TYPE* pos,
  const int* psdres_src) {
  const char* fn = "llsm_gpu_batch_retime";
  llsm_gpu_batch* src = const_cast<llsm_gpu_batch*>(src_c);         // read only: the rows are not changed
  if(fit(fn, dst, src)) return -1;
  if(src -> lay.n_utt != dst -> lay.n_utt) return refuse(fn, "the batches hold different numbers of utterances");
  const int n_utt = dst -> lay.n_utt;
  const size_t Fd = (size_t)dst -> lay.total_frames;
  for(int u = 0; u < n_utt; u ++)
    if((src -> nfrm[u] == 0) != (dst -> nfrm[u] == 0))
      return refuse(fn, "utterance " + std::to_string(u) + " has frames on one side only");
  // the map resolved into flat source frames and weights, [ga | ra] and with psdres_src [gr], Fd words each: positions
  // checked (and formed, without one) on the host
  return blend_frames(fn, dst, src, (psdres_src ? 3 : 2) * Fd, [&](int* h) {
    int* ga = h; float* ra = (float*)h + Fd; int* gr = h + 2 * Fd;
    for(int u = 0; u < n_utt; u ++) {
      const int n = src -> nfrm[u], m = dst -> nfrm[u], o = dst -> frm_off[u], so = src -> frm_off[u];
      if(pos) {
        const float last = (float)(n - 1);
        for(int i = 0; i < m; i ++) {
          const float t = pos[o + i];
          if(!(t >= 0.0f && t <= last))
            return refuse(fn, "position " + std::to_string(o + i) + " (utterance " + std::to_string(u) + ") is NaN or outside [0, " +
              std::to_string(n - 1) + "]");
          ra[o + i] = t;
        }
      } else llsm_gpu_retime_uniform_positions(n, m, ra + o);
      for(int i = 0; i < m; i ++) {                                  // the row of positions becomes the row of weights
        int a;
        pair_at(ra[o + i], n, & a, & ra[o + i]);
        ga[o + i] = so + a;
      }
      if(psdres_src)
        for(int i = 0; i < m; i ++) {
          const int k = psdres_src[o + i];
          if(k < 0 || k >= n)
            return refuse(fn, "psdres_src[" + std::to_string(o + i) + "] = " + std::to_string(k) + " is not a frame of utterance " +
              std::to_string(u));
          gr[o + i] = so + k;
        }
    }
    return 0;
  }, [&](const int* dm) {
    // Without psdres_src gr stays NULL: the kernel's own ga + (ra == 1) is the frame at min(floor(t), n - 1).  For n > 1,
    // ra == 1 only at t = n - 1, where a + 1 = n - 1 (t - (float)a is exact on [a, a + 1], so below it ra < 1 and
    // a = floor(t)); for n == 1 both are 0.
    SpliceMap m = {};
    m.ga = dm; m.ra = (const float*)dm + Fd; m.gr = psdres_src ? dm + 2 * Fd : nullptr;
    return launch_splice(& dst -> ctx -> lc, mod_rows(src), mod_rows(dst), m);
  });
}

namespace {
// One side of a splice map resolved into `ga` (flat source frame a) and `r`, formed from the position by pair_at; utt NULL:
// the output frame's own utterance.  Returns -1 (error set) at the first bad entry; the message is
// built there and nowhere else.
int stage_side(const char* fn, const llsm_gpu_batch* src, const llsm_gpu_batch* dst, const char* side, const int* utt,
  const float* pos, int* ga, float* r) {
  const int n_src = src -> lay.n_utt;
  auto at = [&](const char* what, int g) { return std::string(what) + "_" + side + "[" + std::to_string(g) + "]"; };
  for(int u = 0; u < dst -> lay.n_utt; u ++)
    for(int g = dst -> frm_off[u]; g < dst -> frm_off[u] + dst -> nfrm[u]; g ++) {
      const int v = utt ? utt[g] : u;
      if(v < 0 || v >= n_src)
        return refuse(fn, at("utt", g) + " = " + std::to_string(v) + " is not an utterance of src (" + std::to_string(n_src) + ")");
      const int n = src -> nfrm[v];
      if(n == 0) return refuse(fn, at("utt", g) + " = " + std::to_string(v) + " names an utterance without frames");
      const float t = pos[g];
      if(!(t >= 0.0f && t <= (float)(n - 1)))
        return refuse(fn, at("pos", g) + " (utterance " + std::to_string(v) + ") is NaN or outside [0, " + std::to_string(n - 1) + "]");
      int a;
      pair_at(t, n, & a, & r[g]);
      ga[g] = src -> frm_off[v] + a;
    }
  return 0;
}
}  // namespace

extern "C" int llsm_gpu_batch_splice(llsm_gpu_batch* dst, const llsm_gpu_batch* src_c, const llsm_gpu_splice_map* map) {
  const char* fn = "llsm_gpu_batch_splice";
  llsm_gpu_batch* src = const_cast<llsm_gpu_batch*>(src_c);         // read only: the rows are not changed
  if(! dst || ! src) return refuse(fn, "NULL batch");              // (fit's first refusal, named before a NULL map)
  if(! map) return refuse(fn, "NULL map");
  if(! map -> pos_a) return refuse(fn, "pos_a is NULL");
  const bool two = map -> utt_b || map -> pos_b || map -> mix;
  if(two && !(map -> utt_b && map -> pos_b && map -> mix))
    return refuse(fn, "the second side is given in part: utt_b, pos_b and mix are all NULL or all given");
  if(fit(fn, dst, src)) return -1;
  if(! map -> utt_a && dst -> lay.n_utt > src -> lay.n_utt)
    return refuse(fn, "utt_a is NULL and dst holds more utterances (" + std::to_string(dst -> lay.n_utt) + ") than src (" +
      std::to_string(src -> lay.n_utt) + ")");
  // the map resolved into flat source frames and weights: [ga | ra] and, with a second side, [gb | rb | mix], Fd words each;
  // the rows of the stage and of its device copy are named in one place
  const size_t Fd = (size_t)dst -> lay.total_frames;
  struct Rows { int* ga; float* ra; int* gb; float* rb; float* mix; };
  auto rows = [&](int* p) { return Rows{p, (float*)p + Fd, p + 2 * Fd, (float*)p + 3 * Fd, (float*)p + 4 * Fd}; };
  return blend_frames(fn, dst, src, (two ? 5 : 2) * Fd, [&](int* stage) {
    const Rows h = rows(stage);
    if(stage_side(fn, src, dst, "a", map -> utt_a, map -> pos_a, h.ga, h.ra)) return -1;
    if(! two) return 0;
    if(stage_side(fn, src, dst, "b", map -> utt_b, map -> pos_b, h.gb, h.rb)) return -1;
    for(size_t g = 0; g < Fd; g ++) {
      const float w = map -> mix[g];
      if(!(w >= 0.0f && w <= 1.0f)) return refuse(fn, "mix[" + std::to_string(g) + "] is NaN or outside [0, 1]");
      h.mix[g] = w;
    }
    return 0;
  }, [&](int* dm) {
    const Rows d = rows(dm);
    SpliceMap m = {};                                              // (gr NULL: PSDRES by the kernel's own rule)
    m.ga = d.ga; m.ra = d.ra;
    if(two) { m.gb = d.gb; m.rb = d.rb; m.mix = d.mix; }
    return launch_splice(& dst -> ctx -> lc, mod_rows(src), mod_rows(dst), m);
  });
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

static_assert(kSmoothMaxRadius == LLSM_GPU_SMOOTH_MAX_RADIUS, "the kernels' reach is the header's");
static_assert(SM_F0 == LLSM_GPU_SMOOTH_F0 && SM_RD == LLSM_GPU_SMOOTH_RD && SM_VTMAGN == LLSM_GPU_SMOOTH_VTMAGN &&
  SM_PSD == LLSM_GPU_SMOOTH_PSD && SM_EDC == LLSM_GPU_SMOOTH_EDC, "the kernels' flag bits are the header's");

extern "C" int llsm_gpu_batch_smooth(llsm_gpu_batch* b, const int* radius, int flags) {
  const char* fn = "llsm_gpu_batch_smooth";
  if(! b) return refuse(fn, "NULL batch");
  if(! radius) return refuse(fn, "NULL radius");
  if(b -> l1_nspec == 0) return refuse(fn, "the batch has no layer 1 (llsm_gpu_batch_tolayer1)");
  if(flags & ~LLSM_GPU_SMOOTH_ALL) return refuse(fn, "unknown flag bits " + std::to_string(flags & ~LLSM_GPU_SMOOTH_ALL));
  const int F = b -> lay.total_frames;
  size_t listed = 0;
  for(int g = 0; g < F; g ++) {
    if(radius[g] < 0 || radius[g] > LLSM_GPU_SMOOTH_MAX_RADIUS)
      return refuse(fn, "radius of frame " + std::to_string(g) + " (" + std::to_string(radius[g]) + ") is outside [0, " +
        std::to_string(LLSM_GPU_SMOOTH_MAX_RADIUS) + "]");
    listed += radius[g] > 0;
  }
  if(flags == 0 || listed == 0) return 0;                          // nothing changes
  // the listed frames (radius > 0) cut into tiles: runs of consecutive frames of one utterance, kSmoothTile at the most;
  // staged in page-locked memory as [tiles | radii of the listed frames]
  const size_t tile_words = sizeof(SmoothTile) / sizeof(int);
  if(b -> mod_ev) HIP_OK(hipEventSynchronize(b -> mod_ev));         // the previous call's copy has left the stage
  if(! b -> mod_stage.resize((tile_words + 1) * listed + 1)) return -1;
  SmoothTile* ht = (SmoothTile*)b -> mod_stage.data();
  int* hr = b -> mod_stage.data() + tile_words * listed;           // (at most one tile per listed frame)
  int ntiles = 0, slot = 0;
  for(int u = 0; u < b -> lay.n_utt; u ++) {
    const int u0 = b -> frm_off[u], u1 = u0 + b -> nfrm[u] - 1;
    for(int g = u0; g <= u1; g ++) {
      if(radius[g] == 0) continue;
      const bool grow = ntiles > 0 && ht[ntiles - 1].u0 == u0 && ht[ntiles - 1].g0 + ht[ntiles - 1].cnt == g &&
        ht[ntiles - 1].cnt < kSmoothTile;
      if(grow) ht[ntiles - 1].cnt ++;
      else ht[ntiles ++] = SmoothTile{g, 1, u0, u1, slot};
      hr[slot ++] = radius[g];
    }
  }
  // the tiles move up against the radii: one block, one copy
  const size_t words = tile_words * (size_t)ntiles + listed;
  std::memmove(b -> mod_stage.data() + tile_words * (size_t)ntiles, hr, listed * sizeof(int));
  hipSetDevice(b -> ctx -> device);
  hipStream_t st = b -> ctx -> stream;
  const ModRows rows = mod_rows(b);
  // a failed allocation is a refusal: nothing has changed yet
  if(b -> mod_smooth.alloc(listed * ((size_t)smooth_row_width(rows) + 1))) return -1;
  if(b -> mod_map.alloc(words)) return -1;
  HIP_OK(hipMemcpyAsync(b -> mod_map.p, b -> mod_stage.data(), words * sizeof(int), hipMemcpyHostToDevice, st));
  if(! b -> mod_ev) HIP_OK(hipEventCreateWithFlags(& b -> mod_ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(b -> mod_ev, st));
  SmoothJob job;
  job.tiles = (const SmoothTile*)b -> mod_map.p; job.ntiles = ntiles;
  job.radius = b -> mod_map.p + tile_words * (size_t)ntiles;
  job.rows = b -> mod_smooth.p; job.mark = (int*)(b -> mod_smooth.p + listed * (size_t)smooth_row_width(rows));
  job.flags = flags;
  // accepted: from here on the batch changes.  The lowest-F0 bound stays (rule S9).
  int rc = launch_smooth_rows(& b -> ctx -> lc, rows, job);
  if(! rc) rc = launch_smooth_store(& b -> ctx -> lc, rows, job);
  return rc ? launch_failed(fn, rc) : 0;
}

extern "C" int llsm_gpu_join_radii(int n_utt, const int* nfrm, const int* utt_a, const FP_TYPE* pos_a, int reach,
  int* radius) {
  const char* fn = "llsm_gpu_join_radii";
  if(! nfrm || ! pos_a || ! radius) return refuse(fn, ! nfrm ? "NULL nfrm" : (! pos_a ? "NULL pos_a" : "NULL radius"));
  if(n_utt < 0) return refuse(fn, "n_utt = " + std::to_string(n_utt) + " is negative");
  for(int u = 0; u < n_utt; u ++)
    if(nfrm[u] < 0) return refuse(fn, "nfrm[" + std::to_string(u) + "] = " + std::to_string(nfrm[u]) + " is negative");
  if(reach < 0 || reach > LLSM_GPU_SMOOTH_MAX_RADIUS)
    return refuse(fn, "reach = " + std::to_string(reach) + " is outside [0, " + std::to_string(LLSM_GPU_SMOOTH_MAX_RADIUS) + "]");
  int joins = 0;
  for(int u = 0, o = 0; u < n_utt; o += nfrm[u], u ++) {
    const int n = nfrm[u];
    auto join_at = [&](int i) {                                    // between frames i - 1 and i, 1 <= i < n
      const float next = pos_a[o + i - 1] + 1.0f;                  // (float32, one rounding)
      return !((! utt_a || utt_a[o + i] == utt_a[o + i - 1]) && pos_a[o + i] == next);
    };
    // distance to the last join at or below i, then to the first join above it
    int d = reach;
    for(int i = 0; i < n; i ++) {
      if(i >= 1 && join_at(i)) { d = 0; joins ++; }
      radius[o + i] = reach - d;
      if(d < reach) d ++;
    }
    d = reach;
    for(int i = n - 1; i >= 1; i --) {
      if(join_at(i)) d = 0;                                         // frame i - 1 is at distance 0
      if(reach - d > radius[o + i - 1]) radius[o + i - 1] = reach - d;
      if(d < reach) d ++;
    }
  }
  return joins;
}
