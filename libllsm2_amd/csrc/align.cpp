// align.cpp -- alignment of utterance pairs on the device: host side of align_kernels.hip.
//
//   llsm_gpu_align_default_options   the defaults of llsm_gpu.h
//   llsm_gpu_align_check             host only: every refusal that needs no batch beyond the orders of its coder
//   llsm_gpu_batch_align             LLSM_GPU_CODE of two batches -> per-frame positions and path costs on the host (rules
//                                    D1 - D3: llsm_gpu.h): the distance planes of all pairs
//                                    (k_align_dist), one path per pair (k_align_dtw), one copy back
//   llsm_gpu_align_band_min / _rows  host only: the least connected band of a pair and the column range of every row (rule B1)
//   llsm_gpu_batch_align_band        the same inside a band around the diagonal (rules B1 - B4):
//                                    k_align_band_dist, k_align_band_dtw, scratch of its own
//
// Every check runs before anything is allocated, copied or launched.  The scratch lives on batch a, grow-only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "batch.h"

namespace {
const char* kAlign = "llsm_gpu_batch_align";
const char* kBand = "llsm_gpu_batch_align_band";
const long long kMaxCells = 1ll << 28;

int refuse(const std::string& why, const char* who = kAlign) { llsm_set_error(std::string(who) + ": " + why); return -1; }
int refuse_band(const std::string& why) { return refuse(why, kBand); }

// rule B1: the least connected band of an na x nb pair (na, nb >= 1).  The last row ends on nb - 1 whatever the band
// (c = nb - 1 there) unless it is the only row, and row i + 1 starts no later than one past the end of row i iff
// 2 band + 1 >= c_{i+1} - c_i.
int band_min(int na, int nb) {
  if(na == 1) return nb - 1;
  int gap = 0;
  for(int i = 0, c = 0; i + 1 < na; i ++) {
    const int n = align_band_center(i + 1, na, nb);
    gap = std::max(gap, n - c); c = n;
  }
  return gap / 2;                                                   // ceil((gap - 1) / 2) for gap >= 0
}

// the options checked against a coder of these orders, count resolved; -1 with the error set in the name of `who`
int check(llsm_gpu_align_options* o, int order_spec, int order_bap, const char* who = kAlign) {
  if(order_spec < 1 || order_bap < 1) return refuse("the coder is not enabled", who);
  const int dim = order_spec + order_bap + 3;
  if(o -> count <= 0) o -> count = order_spec;
  if(o -> first < 0 || o -> first >= dim || o -> count > dim - o -> first)
    return refuse("columns [" + std::to_string(o -> first) + ", " + std::to_string((long long)o -> first + o -> count) +
      ") lie outside [0, " + std::to_string(dim) + ")", who);
  if(std::isnan(o -> step_cost) || std::isnan(o -> voicing_cost)) return refuse("a cost is NaN", who);
  if(std::isinf(o -> step_cost) || std::isinf(o -> voicing_cost)) return refuse("a cost is infinite", who);
  if(o -> step_cost < 0) return refuse("step_cost < 0", who);
  if(o -> voicing_cost < 0) return refuse("voicing_cost < 0", who);
  return 0;
}
}  // namespace

extern "C" void llsm_gpu_align_default_options(llsm_gpu_align_options* dst) {
  if(! dst) return;
  dst -> first = 3; dst -> count = 0; dst -> step_cost = 0; dst -> voicing_cost = 0;
}

extern "C" int llsm_gpu_align_check(const llsm_gpu_align_options* opt, int order_spec, int order_bap) {
  llsm_gpu_align_options o;
  if(opt) o = *opt; else llsm_gpu_align_default_options(& o);
  return check(& o, order_spec, order_bap);
}

extern "C" int llsm_gpu_batch_align(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a,
  const int* utt_b, const llsm_gpu_align_options* opt, FP_TYPE* pos, FP_TYPE* cost) {
  if(! a || ! b) return refuse("NULL batch");
  if(n_pairs < 0) return refuse("n_pairs < 0");
  if(a -> ctx != b -> ctx) return refuse("the batches belong to different contexts");
  if(a -> coder_os == 0 || b -> coder_os == 0) return refuse("the coder is not enabled on both batches");
  if(a -> coder_os + a -> coder_ob != b -> coder_os + b -> coder_ob)
    return refuse("the coder dimensions differ: " + std::to_string(a -> coder_os + a -> coder_ob + 3) + " and " +
      std::to_string(b -> coder_os + b -> coder_ob + 3));
  llsm_gpu_align_options o;
  if(opt) o = *opt; else llsm_gpu_align_default_options(& o);
  if(check(& o, a -> coder_os, a -> coder_ob)) return -1;
  if(n_pairs == 0) return 0;
  if(! utt_a || ! utt_b) return refuse("NULL utterance list");
  if(! pos) return refuse("NULL pos");
  std::vector<AlignPair> pairs((size_t)n_pairs);
  long long cells = 0, rows = 0, frames = 0, steps = 0, n_tiles = 0;
  for(int p = 0; p < n_pairs; p ++) {
    const int ua = utt_a[p], ub = utt_b[p];
    if(ua < 0 || ua >= a -> lay.n_utt) return refuse("pair " + std::to_string(p) + ": utterance " + std::to_string(ua) + " is outside batch a");
    if(ub < 0 || ub >= b -> lay.n_utt) return refuse("pair " + std::to_string(p) + ": utterance " + std::to_string(ub) + " is outside batch b");
    const int na = a -> nfrm[ua], nb = b -> nfrm[ub];
    if(na <= 0 || nb <= 0) return refuse("pair " + std::to_string(p) + ": an utterance without frames");
    AlignPair& q = pairs[p];
    q.a0 = a -> frm_off[ua]; q.na = na; q.b0 = b -> frm_off[ub]; q.nb = nb;
    q.cell0 = (int)cells; q.row0 = (int)rows; q.pos0 = (int)frames; q.pad = 0; q.mv0 = steps;
    cells += (long long)na * nb;                                   // (checked below: the offsets above are only used if it fits)
    if(cells > kMaxCells) {                                         // the total of the whole list, for the message
      for(int r = p + 1; r < n_pairs; r ++)
        if(utt_a[r] >= 0 && utt_a[r] < a -> lay.n_utt && utt_b[r] >= 0 && utt_b[r] < b -> lay.n_utt)
          cells += (long long)std::max(a -> nfrm[utt_a[r]], 0) * std::max(b -> nfrm[utt_b[r]], 0);
      return refuse("the distance planes hold " + std::to_string(cells) + " cells, more than 2^28 = " + std::to_string(kMaxCells));
    }
    rows += nb; frames += na;
    steps += (long long)((na + 63) / 64) * ALIGN_STEPS(nb);
    n_tiles += (long long)((na + ALIGN_TILE - 1) / ALIGN_TILE) * ((nb + ALIGN_TILE - 1) / ALIGN_TILE);
  }
  // accepted: from here on a's scratch changes
  std::vector<int4> tiles; tiles.reserve((size_t)n_tiles);
  for(int p = 0; p < n_pairs; p ++)
    for(int i0 = 0; i0 < pairs[p].na; i0 += ALIGN_TILE)
      for(int j0 = 0; j0 < pairs[p].nb; j0 += ALIGN_TILE) tiles.push_back(make_int4(p, i0, j0, 0));
  hipSetDevice(a -> ctx -> device);
  const size_t n_out = (size_t)frames + (size_t)n_pairs;
  if(a -> al_plane.alloc((size_t)cells) || a -> al_row.alloc((size_t)rows) || a -> al_out.alloc(n_out) ||
     a -> al_moves.alloc((size_t)steps) || a -> al_pairs.alloc(pairs.size()) || a -> al_tiles.alloc(tiles.size())) return -1;
  a -> al_cells = 0;                                                // the planes are being rewritten
  LaunchCtx* P = & a -> ctx -> lc;
  // (pageable sources: the copies have left the vectors when the calls return, and run in stream order)
  HIP_OK(hipMemcpyAsync(a -> al_pairs.p, pairs.data(), pairs.size() * sizeof(AlignPair), hipMemcpyHostToDevice, P -> stream));
  HIP_OK(hipMemcpyAsync(a -> al_tiles.p, tiles.data(), tiles.size() * sizeof(int4), hipMemcpyHostToDevice, P -> stream));
  AlignDev d;
  d.code_a = (const float*)a -> arr[LLSM_GPU_CODE]; d.code_b = (const float*)b -> arr[LLSM_GPU_CODE];
  d.dim = a -> coder_os + a -> coder_ob + 3; d.first = o.first; d.count = o.count;
  d.step_cost = o.step_cost; d.voicing_cost = o.voicing_cost;
  d.pairs = a -> al_pairs.p; d.n_pairs = n_pairs;
  int rc = launch_align_dist(P, d, a -> al_tiles.p, (int)tiles.size(), a -> al_plane.p);
  if(! rc) rc = launch_align_dtw(P, d, a -> al_plane.p, a -> al_moves.p, a -> al_row.p, a -> al_out.p, (int)frames);
  if(rc) return refuse(std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
  // into memory of our own first: a failed copy leaves pos and cost untouched
  std::vector<float> host(n_out);
  HIP_OK(hipMemcpyAsync(host.data(), a -> al_out.p, n_out * sizeof(float), hipMemcpyDeviceToHost, P -> stream));
  HIP_OK(hipStreamSynchronize(P -> stream));
  std::copy(host.begin(), host.begin() + frames, pos);
  if(cost) std::copy(host.begin() + frames, host.end(), cost);
  a -> al_cells = cells;
  return 0;
}

// ---------------------------------------------------------------- inside a diagonal band (rules B1 - B4)
extern "C" int llsm_gpu_align_band_min(int na, int nb) {
  if(na < 1 || nb < 1) { llsm_set_error("llsm_gpu_align_band_min: na < 1 or nb < 1"); return -1; }
  return band_min(na, nb);
}

extern "C" int llsm_gpu_align_band_rows(int na, int nb, int band, int* lo, int* hi) {
  const char* who = "llsm_gpu_align_band_rows";
  if(na < 1 || nb < 1) return refuse("na < 1 or nb < 1", who);
  if(band < 0) return refuse("band < 0", who);
  if(! lo || ! hi) return refuse("NULL lo or hi", who);
  const int least = band_min(na, nb);
  if(band < least)
    return refuse("a band of " + std::to_string(band) + " is not connected for " + std::to_string(na) + " x " + std::to_string(nb) +
      " frames: the least is " + std::to_string(least), who);
  for(int i = 0; i < na; i ++) {
    const long long c = align_band_center(i, na, nb);
    lo[i] = (int)std::max(c - band, 0ll); hi[i] = (int)std::min(c + band, (long long)nb - 1);
  }
  return 0;
}

extern "C" int llsm_gpu_batch_align_band(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a,
  const int* utt_b, const int* band, const llsm_gpu_align_options* opt, FP_TYPE* pos, FP_TYPE* cost) {
  if(! a || ! b) return refuse_band("NULL batch");
  if(n_pairs < 0) return refuse_band("n_pairs < 0");
  if(a -> ctx != b -> ctx) return refuse_band("the batches belong to different contexts");
  if(a -> coder_os == 0 || b -> coder_os == 0) return refuse_band("the coder is not enabled on both batches");
  if(a -> coder_os + a -> coder_ob != b -> coder_os + b -> coder_ob)
    return refuse_band("the coder dimensions differ: " + std::to_string(a -> coder_os + a -> coder_ob + 3) + " and " +
      std::to_string(b -> coder_os + b -> coder_ob + 3));
  llsm_gpu_align_options o;
  if(opt) o = *opt; else llsm_gpu_align_default_options(& o);
  if(check(& o, a -> coder_os, a -> coder_ob, kBand)) return -1;
  if(n_pairs == 0) return 0;
  if(! utt_a || ! utt_b) return refuse_band("NULL utterance list");
  if(! band) return refuse_band("NULL band");
  if(! pos) return refuse_band("NULL pos");
  // the cells of one pair's band plane, held below 2^61 so that the total of any list fits 64 bits
  auto plane_cells = [](int na, int bd) { return std::min((long long)na * (2ll * bd + 1), 1ll << 61); };
  std::vector<AlignBandPair> pairs((size_t)n_pairs);
  long long cells = 0, rows = 0, frames = 0, steps = 0;
  for(int p = 0; p < n_pairs; p ++) {
    const int ua = utt_a[p], ub = utt_b[p], bd = band[p];
    const std::string pair = "pair " + std::to_string(p) + ": ";
    if(ua < 0 || ua >= a -> lay.n_utt) return refuse_band(pair + "utterance " + std::to_string(ua) + " is outside batch a");
    if(ub < 0 || ub >= b -> lay.n_utt) return refuse_band(pair + "utterance " + std::to_string(ub) + " is outside batch b");
    const int na = a -> nfrm[ua], nb = b -> nfrm[ub];
    if(na <= 0 || nb <= 0) return refuse_band(pair + "an utterance without frames");
    if(bd < 0) return refuse_band(pair + "band < 0");
    const int least = band_min(na, nb);
    if(bd < least)
      return refuse_band(pair + "a band of " + std::to_string(bd) + " is not connected for " + std::to_string(na) + " x " +
        std::to_string(nb) + " frames: llsm_gpu_align_band_min is " + std::to_string(least));
    AlignBandPair& q = pairs[p];
    q.a0 = a -> frm_off[ua]; q.na = na; q.b0 = b -> frm_off[ub]; q.nb = nb;
    q.cell0 = (int)cells; q.row0 = (int)rows; q.pos0 = (int)frames; q.band = bd; q.mv0 = steps; q.pad = 0;
    cells += plane_cells(na, bd);                                   // (checked below: the offsets above are only used if it fits)
    if(cells > kMaxCells) {                                         // the total of the whole list, for the message
      for(int r = p + 1; r < n_pairs && cells < (1ll << 61); r ++)
        if(utt_a[r] >= 0 && utt_a[r] < a -> lay.n_utt) cells += plane_cells(std::max(a -> nfrm[utt_a[r]], 0), std::max(band[r], 0));
      return refuse_band("the band planes hold " + std::to_string(cells) + " cells, more than 2^28 = " + std::to_string(kMaxCells));
    }
    // the moves of a strip of 64 rows: one entry per anti-diagonal of its column window [lo of its first row, hi of its last]
    int widest = 0;
    for(int i0 = 0; i0 < na; i0 += 64) {
      const int i1 = std::min(i0 + 63, na - 1);
      const int wlo = std::max(align_band_center(i0, na, nb) - bd, 0), whi = std::min(align_band_center(i1, na, nb) + bd, nb - 1);
      widest = std::max(widest, whi - wlo + 1 + i1 - i0);
    }
    q.steps = widest;
    rows += nb; frames += na;
    steps += (long long)((na + 63) / 64) * widest;
  }
  // accepted: from here on a's band scratch changes (the scratch of llsm_gpu_batch_align, plane 6 among it, is not touched)
  std::vector<int4> tiles;
  for(int p = 0; p < n_pairs; p ++) {
    const AlignBandPair& q = pairs[p];
    for(int i0 = 0; i0 < q.na; i0 += ALIGN_TILE) {                  // the tiles of the matrix that meet the band, overhang included
      const int jlo = align_band_center(i0, q.na, q.nb) - q.band;
      const int jhi = align_band_center(std::min(i0 + ALIGN_TILE, q.na) - 1, q.na, q.nb) + q.band;
      const int j_first = jlo >= 0 ? jlo / ALIGN_TILE * ALIGN_TILE : -((-jlo + ALIGN_TILE - 1) / ALIGN_TILE * ALIGN_TILE);
      for(int j0 = j_first; j0 <= jhi; j0 += ALIGN_TILE) tiles.push_back(make_int4(p, i0, j0, 0));
    }
  }
  hipSetDevice(a -> ctx -> device);
  const size_t n_out = (size_t)frames + (size_t)n_pairs;
  if(a -> alb_plane.alloc((size_t)cells) || a -> alb_row.alloc((size_t)rows) || a -> alb_out.alloc(n_out) ||
     a -> alb_moves.alloc((size_t)steps) || a -> alb_pairs.alloc(pairs.size()) || a -> alb_tiles.alloc(tiles.size())) return -1;
  a -> alb_cells = 0;                                               // the planes are being rewritten
  LaunchCtx* P = & a -> ctx -> lc;
  // (pageable sources: the copies have left the vectors when the calls return, and run in stream order)
  HIP_OK(hipMemcpyAsync(a -> alb_pairs.p, pairs.data(), pairs.size() * sizeof(AlignBandPair), hipMemcpyHostToDevice, P -> stream));
  HIP_OK(hipMemcpyAsync(a -> alb_tiles.p, tiles.data(), tiles.size() * sizeof(int4), hipMemcpyHostToDevice, P -> stream));
  AlignBandDev d;
  d.code_a = (const float*)a -> arr[LLSM_GPU_CODE]; d.code_b = (const float*)b -> arr[LLSM_GPU_CODE];
  d.dim = a -> coder_os + a -> coder_ob + 3; d.first = o.first; d.count = o.count;
  d.step_cost = o.step_cost; d.voicing_cost = o.voicing_cost;
  d.pairs = a -> alb_pairs.p; d.n_pairs = n_pairs;
  int rc = launch_align_band_dist(P, d, a -> alb_tiles.p, (int)tiles.size(), a -> alb_plane.p);
  if(! rc) rc = launch_align_band_dtw(P, d, a -> alb_plane.p, a -> alb_moves.p, a -> alb_row.p, a -> alb_out.p, (int)frames);
  if(rc) return refuse_band(std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
  // into memory of our own first: a failed copy leaves pos and cost untouched
  std::vector<float> host(n_out);
  HIP_OK(hipMemcpyAsync(host.data(), a -> alb_out.p, n_out * sizeof(float), hipMemcpyDeviceToHost, P -> stream));
  HIP_OK(hipStreamSynchronize(P -> stream));
  std::copy(host.begin(), host.begin() + frames, pos);
  if(cost) std::copy(host.begin() + frames, host.end(), cost);
  a -> alb_cells = cells;
  return 0;
}
