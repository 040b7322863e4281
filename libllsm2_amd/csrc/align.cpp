// align.cpp -- alignment of utterance pairs on the device: host side of align_kernels.hip.
//
//   llsm_gpu_align_default_options   the defaults of llsm_gpu.h
//   llsm_gpu_align_check             host only: every refusal that needs no batch beyond the orders of its coder
//   llsm_gpu_batch_align             LLSM_GPU_CODE of two batches -> per-frame positions and path costs on the host (rules
//                                    D1 - D3: llsm_gpu.h): the distance planes of all pairs
//                                    (k_align_dist_t), one path per pair (k_align_dtw_t), one copy back
//   llsm_gpu_align_band_min / _rows  host only: the least connected band of a pair and the column range of every row (rule B1)
//   llsm_gpu_batch_align_band        the same inside a band around the diagonal (rules B1 - B4), with
//                                    scratch of its own
//   llsm_gpu_align_slope_rows        host only: whether a pair is admissible under the slope pattern and the column range of
//                                    every row (rule L1)
//   llsm_gpu_batch_align_slope       the whole planes again, and a path whose local slope stays within [1/2, 2] (rules L1 -
//                                    L4, DESIGN.md section 27: k_align_slope_dtw_t<false>), with scratch of its own
//   llsm_gpu_align_band_slope_min / _rows   host only: the least band that is connected for the slope pattern, and the
//                                    column range of every row of the region (rule K1: two integer sweeps over intervals)
//   llsm_gpu_batch_align_band_slope  the slope pattern inside the band (rules K1 - K4, DESIGN.md section 28: the band planes
//                                    of k_align_band_dist, the region's rows as a table, k_align_slope_dtw_t<true>), with
//                                    scratch of its own
//   llsm_gpu_align_around_min / _rows   host only: the same two questions for a band around a centre line of the caller's
//                                    (rule A1), for either pattern
//   llsm_gpu_align_center_line       host only: the positions of a coarse alignment as the centre line of a fine one
//   llsm_gpu_batch_align_around      either pattern inside a band around a centre line per pair (rules A1 - A3, DESIGN.md
//                                    section 30: the kernels of the banded calls instantiated for ALIGN_GEO_LINE, which read
//                                    the centre of a row from a table), with scratch of its own
//
//   llsm_gpu_align_sub_rows          host only: whether a query is admissible inside a take with free ends, and the column
//                                    range of every row (rule Q1)
//   llsm_gpu_batch_align_sub         a query inside a take: the whole planes, a path that starts anywhere on row 0 and ends
//                                    anywhere on the last row, under either pattern (rules Q1 - Q5, DESIGN.md section 35: the
//                                    two path kernels instantiated with free ends), with scratch of its own; its planes
//                                    through llsm_gpu_batch_align_sub_plane
//
//   llsm_gpu_pool_frames            host only: the coarse frames of an utterance under a pooling factor (rule P1)
//   llsm_gpu_batch_pool_code        the means of every `factor` consecutive rows of LLSM_GPU_CODE of the listed utterances
//                                    (rule P1, DESIGN.md section 34: k_pool_code) on the host
//   llsm_gpu_batch_align_pyramid    coarse to fine in one call (rules Y1 - Y5): both sides pooled on the device, the pooled
//                                    pairs through the full or the slope pass, llsm_gpu_align_center_line and
//                                    llsm_gpu_align_around_min on the host, the fine pairs through the pass around the line,
//                                    with two scratch sets of its own and no plane
//
// The five calls are one pass, align_pass behind align_head, told apart by an AlignMode (band, slope, around: batch.h): the
// steps of a strip (strip_steps) and the kernel instantiations follow from it, and for the five calls (align_run) the name in
// the messages and the scratch set do too.  A pass reads its two sides through AlignSide views and takes scratch set and name
// from its AlignJob, so the pyramid runs it twice: on the pooled rows and on the batches' own.  Every check
// runs before anything is allocated, copied or launched.  The scratch lives on batch a, grow-only, one set per call.
// Wherever a function takes `line`, NULL stands for the straight diagonal of rule B1, computed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "batch.h"

namespace {
const char* const kAlign = kAlignCalls[ALIGN_FULL].name;            // in whose name llsm_gpu_align_check refuses
const long long kMaxCells = 1ll << 28;

int refuse(const std::string& why, const char* who = kAlign) { llsm_set_error(std::string(who) + ": " + why); return -1; }

// c_i of an na x nb pair: the caller's line (rule A1), or without one the diagonal of rule B1
int center_at(const int* line, int i, int na, int nb) { return line ? line[i] : align_band_center(i, na, nb); }

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

// rule A1 without the slope pattern: the least connected band around a valid line.  Row 0 starts on column 0 iff band >= c_0,
// the last row ends on nb - 1 iff band >= nb - 1 - c_{na-1}, and the rows in between touch as in band_min (the clamps to
// the matrix never part two rows: c_{i+1} <= nb - 1 and c_i >= 0).
int around_min(int na, int nb, const int* line) {
  int least = std::max(line[0], nb - 1 - line[na - 1]);
  for(int i = 0; i + 1 < na; i ++) least = std::max(least, (line[i + 1] - line[i]) / 2);
  return least;
}

// rule A1: empty if `line` is a valid centre line of an na x nb pair, else the first row that is not and its value
std::string line_fault(int na, int nb, const int* line) {
  for(int i = 0; i < na; i ++) {
    if(line[i] < 0 || line[i] > nb - 1)
      return "center[" + std::to_string(i) + "] = " + std::to_string(line[i]) + " lies outside [0, " + std::to_string(nb - 1) + "]";
    if(i > 0 && line[i] < line[i - 1])
      return "center[" + std::to_string(i) + "] = " + std::to_string(line[i]) + " is below center[" + std::to_string(i - 1) + "] = " +
        std::to_string(line[i - 1]);
  }
  return "";
}

// rule L1: empty if an na x nb pair (na, nb >= 1) is admissible under the slope pattern, else the bound that fails
std::string slope_bound(int na, int nb) {
  const long long ra = (long long)na - 1, rb = (long long)nb - 1;
  if(rb > 2 * ra) return "nb - 1 = " + std::to_string(rb) + " exceeds 2 (na - 1) = " + std::to_string(2 * ra);
  if(ra > 2 * rb) return "na - 1 = " + std::to_string(ra) + " exceeds 2 (nb - 1) = " + std::to_string(2 * rb);
  return "";
}

// rule K1: the rows of the region of an admissible na x nb pair (na, nb >= 1) under the slope pattern inside a band >= 0
// around the diagonal or, rule A1, around a valid line (where row 0 need not hold column 0, and F_0 is then empty), by
// the two sweeps over intervals; an empty row is (1, 0).  Returns whether the band is connected for the pattern, i.e. whether
// the last row is non-empty.  A piece with lower end > upper end is empty and contributes nothing.
struct Interval {
  long long a = 1, b = 0;
  bool empty() const { return a > b; }
  void join(long long lo, long long hi) {                           // from the least lower end to the largest upper end
    if(lo > hi) return;
    if(empty()) { a = lo; b = hi; } else { a = std::min(a, lo); b = std::max(b, hi); }
  }
};
bool band_slope_rows(int na, int nb, int band, std::vector<int2>& rows, const int* line = nullptr) {
  using std::max; using std::min;
  std::vector<long long> p((size_t)na), q((size_t)na);
  for(int i = 0; i < na; i ++) {
    const long long c = center_at(line, i, na, nb);
    p[i] = max(c - band, 0ll); q[i] = min(c + band, (long long)nb - 1);
  }
  std::vector<Interval> F((size_t)na);
  if(p[0] <= 0) { F[0].a = 0; F[0].b = 0; }
  for(int i = 1; i < na; i ++) {
    const Interval& u = F[i - 1];
    if(! u.empty()) {
      F[i].join(max(u.a + 1, p[i]), min(u.b + 1, q[i]));                                      // move 0
      F[i].join(max(u.a + 2, p[i] + 1), min(u.b + 2, q[i]));                                  // move 2, past (i, j - 1)
    }
    if(i >= 2 && ! F[i - 2].empty())                                                           // move 1, past (i - 1, j)
      F[i].join(max(max(F[i - 2].a + 1, p[i]), p[i - 1]), min(min(F[i - 2].b + 1, q[i]), q[i - 1]));
  }
  rows.assign((size_t)na, make_int2(1, 0));
  Interval g1, g2;                                                  // G of rows i + 1 and i + 2
  for(int i = na - 1; i >= 0; i --) {
    Interval g;
    if(i == na - 1) { if(q[i] >= nb - 1) { g.a = nb - 1; g.b = nb - 1; } }
    else {
      if(! g1.empty()) {
        g.join(max(g1.a - 1, p[i]), min(g1.b - 1, q[i]));
        g.join(max(max(g1.a - 2, p[i]), p[i + 1] - 1), min(g1.b - 2, q[i]));
      }
      if(i + 2 < na && ! g2.empty())
        g.join(max(max(g2.a - 1, p[i]), p[i + 1] - 1), min(min(g2.b - 1, q[i]), q[i + 1] - 1));
    }
    if(! g.empty() && ! F[i].empty() && max(g.a, F[i].a) <= min(g.b, F[i].b))
      rows[i] = make_int2((int)max(g.a, F[i].a), (int)min(g.b, F[i].b));
    g2 = g1; g1 = g;
  }
  return rows[na - 1].x <= rows[na - 1].y;
}
// the least band that is connected for the slope pattern (connectedness is monotone in the band, and the band that covers
// the matrix is connected: its region is that of L1)
int band_slope_min(int na, int nb) {
  std::vector<int2> rows;
  int band = 0;
  while(band < nb - 1 && ! band_slope_rows(na, nb, band, rows)) band ++;
  return band;
}
// the same around a valid line, where the least band may be large: by bisection over [0, nb - 1]
int around_slope_min(int na, int nb, const int* line) {
  std::vector<int2> rows;
  int below = -1, band = nb - 1;                                    // `below` is not connected (or -1), `band` is
  while(band - below > 1) {
    const int mid = below + (band - below) / 2;
    if(band_slope_rows(na, nb, mid, rows, line)) band = mid; else below = mid;
  }
  return band;
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

namespace {
static_assert(ALIGN_TILE == 64, "a row of tiles of the distance kernel is a strip of 64 rows of the path kernel");

int tile_floor(int j) { return j >= 0 ? j / ALIGN_TILE * ALIGN_TILE : -((-j + ALIGN_TILE - 1) / ALIGN_TILE * ALIGN_TILE); }

// rows [i0, i0 + 63] of a pair, a strip of the path kernels and a row of tiles of the distance kernel: the first column of
// its first row and the last of its last as the plane stores them (under a band they may lie outside the matrix).  Returns
// the last row.
int strip_span(bool banded, const AlignPair& q, const int* line, int i0, int& jlo, int& jhi) {
  const int i1 = std::min(i0 + 63, q.na - 1);
  jlo = banded ? center_at(line, i0, q.na, q.nb) - q.band : 0;
  jhi = banded ? center_at(line, i1, q.na, q.nb) + q.band : q.nb - 1;
  return i1;
}

// The steps the path kernel of `mode` takes over the same rows: the anti-diagonals of the strip's column window [jlo, jhi],
// which each kernel finds the same way.  Without the slope pattern the window is the span within the matrix.  Under it a
// strip that has a successor takes one step more, as the first row of the successor may be entered past column jhi, and
// the window is, by rule L1, lo of the first row and hi of the last (neither decreases with the row), or inside a band, by
// rule K1, the least lo and the largest hi of the non-empty rows among the pair's rows of the region, `region`; with free
// ends, by rule Q1, lo of the first row and nb - 1.  Around a
// line c does not decrease either, and a connected band has c_{i+1} - c_i <= 2 band + 1, so the window of a strip is at most
// 63 (2 band + 1) + 2 band + 1 columns.
int strip_steps(int mode, const AlignPair& q, const int* line, int i0, const int2* region) {
  int jlo, jhi, unused;
  const int i1 = strip_span(mode & ALIGN_BAND, q, line, i0, jlo, jhi);
  if(! (mode & ALIGN_SLOPE)) { jlo = std::max(jlo, 0); jhi = std::min(jhi, q.nb - 1); }
  else if(mode & ALIGN_SUB) align_sub_row(i0, q.nb, jlo, jhi);       // rule Q1: lo of the first row, and every row ends on nb - 1
  else if(mode & ALIGN_BAND) {
    jlo = q.nb - 1; jhi = 0;
    for(int i = i0; i <= i1; i ++)
      if(region[i].x <= region[i].y) { jlo = std::min(jlo, region[i].x); jhi = std::max(jhi, region[i].y); }
  } else { align_slope_row(i0, q.na, q.nb, jlo, unused); align_slope_row(i1, q.na, q.nb, unused, jhi); }
  // (jhi < jlo takes a strip whose rows are all empty, which a connected band does not have)
  return std::max(jhi - jlo, 0) + 1 + i1 - i0 + ((mode & ALIGN_SLOPE) && i1 + 1 < q.na ? 1 : 0);
}

// One side of a call: the rows of LLSM_GPU_CODE of a batch and where its utterances lie in them -- or, in the coarse pass of
// llsm_gpu_batch_align_pyramid, the pooled rows of a pair list and where each pair's lie.  code is a device pointer and is
// not read on the host; the other two are host arrays of n_utt + 1 and n_utt entries.
struct AlignSide { const float* code; const int* frm_off; const int* nfrm; int n_utt; };
AlignSide side_of(const llsm_gpu_batch* b) {
  return AlignSide{(const float*)b -> arr[LLSM_GPU_CODE], b -> frm_off.data(), b -> nfrm.data(), b -> lay.n_utt};
}
// What a pass runs on and for: the batch whose context, stream and scratch it uses, the two sides (dim columns a row), the
// checked options, the scratch set it rewrites and the name its messages carry.
struct AlignJob {
  llsm_gpu_batch* owner; AlignSide a, b; int dim; llsm_gpu_align_options o; llsm_gpu_batch::AlignScratch* sc; const char* who;
};

std::string pair_of(int p) { return "pair " + std::to_string(p) + ": "; }   // (only a refusal pays for it)
// empty, or why the utterances of pair p cannot be aligned
std::string pair_fault(const AlignSide& a, const AlignSide& b, int p, int ua, int ub) {
  if(ua < 0 || ua >= a.n_utt) return pair_of(p) + "utterance " + std::to_string(ua) + " is outside batch a";
  if(ub < 0 || ub >= b.n_utt) return pair_of(p) + "utterance " + std::to_string(ub) + " is outside batch b";
  if(a.nfrm[ua] <= 0 || b.nfrm[ub] <= 0) return pair_of(p) + "an utterance without frames";
  return "";
}
// rule Q1: empty if a query of na frames is admissible in a take of nb under the slope pattern with free ends (na, nb >= 1),
// else the bound that fails
std::string sub_bound(int na, int nb) {
  const long long need = (long long)na / 2, rb = (long long)nb - 1;  // ceil((na - 1) / 2)
  return need > rb ? "ceil((na - 1) / 2) = " + std::to_string(need) + " exceeds nb - 1 = " + std::to_string(rb) : "";
}
// empty, or rule L1's refusal of pair p in the words of llsm_gpu_batch_align_slope
std::string inadmissible(int p, int na, int nb) {
  const std::string bound = slope_bound(na, nb);
  return bound.empty() ? "" : pair_of(p) + std::to_string(na) + " x " + std::to_string(nb) + " frames are not admissible: " + bound;
}

// What every call refuses of its two batches and its options before it looks at a pair, in the order in which the calls
// have always made these checks; o: the options, checked and resolved.
int align_head(const llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const llsm_gpu_align_options* opt, const char* who,
  llsm_gpu_align_options& o) {
  if(! a || ! b) return refuse("NULL batch", who);
  if(n_pairs < 0) return refuse("n_pairs < 0", who);
  if(a -> ctx != b -> ctx) return refuse("the batches belong to different contexts", who);
  if(a -> coder_os == 0 || b -> coder_os == 0) return refuse("the coder is not enabled on both batches", who);
  if(a -> coder_os + a -> coder_ob != b -> coder_os + b -> coder_ob)
    return refuse("the coder dimensions differ: " + std::to_string(a -> coder_os + a -> coder_ob + 3) + " and " +
      std::to_string(b -> coder_os + b -> coder_ob + 3), who);
  if(opt) o = *opt; else llsm_gpu_align_default_options(& o);
  return check(& o, a -> coder_os, a -> coder_ob, who);
}

// One pass over the pairs of a list, after align_head: the five calls and the two passes of llsm_gpu_batch_align_pyramid,
// told apart by `mode` (AlignMode: batch.h) and by the job.  With ALIGN_BAND the planes are band planes, else band is not
// read and the planes hold the whole matrix of every pair.  The checks run in the order in which the calls have always made
// them.  ALIGN_AROUND comes with ALIGN_BAND, with the centre lines of all pairs in `center` and with the caller's `slope` as
// `pattern`, which becomes the ALIGN_SLOPE bit once it has been checked; that call makes its checks in the order of its
// header, each over all pairs before the next.  ALIGN_SUB (rules Q1 - Q5) comes alone, with the caller's slope as `pattern`
// too, checked after everything llsm_gpu_batch_align refuses, its cap included; span and last_row are that call's further
// outputs and NULL in every other.
int align_pass(const AlignJob& J, int n_pairs, const int* utt_a, const int* utt_b, int mode, int pattern, const int* center,
  const int* band, FP_TYPE* pos, FP_TYPE* cost, int* span = nullptr, FP_TYPE* last_row = nullptr) {
  const bool banded = mode & ALIGN_BAND, around = mode & ALIGN_AROUND, sub = mode & ALIGN_SUB;
  const char* who = J.who;
  const AlignSide& a = J.a; const AlignSide& b = J.b;
  const llsm_gpu_align_options& o = J.o;
  if(n_pairs == 0) return 0;
  if(! utt_a || ! utt_b) return refuse("NULL utterance list", who);
  if(banded && ! around && ! band) return refuse("NULL band", who);
  if(! pos) return refuse("NULL pos", who);
  if(around) {                                                      // checks 1 - 6 of llsm_gpu_batch_align_around (7 and 8: below)
    for(int p = 0; p < n_pairs; p ++) { const std::string why = pair_fault(a, b, p, utt_a[p], utt_b[p]); if(! why.empty()) return refuse(why, who); }
    if(pattern != 0 && pattern != 1) return refuse("slope = " + std::to_string(pattern) + " is neither 0 nor 1", who);
    if(pattern) mode |= ALIGN_SLOPE;
    if(! band || ! center) return refuse("NULL band or center", who);
    for(int p = 0; p < n_pairs; p ++) if(band[p] < 0) return refuse(pair_of(p) + "band < 0", who);
    for(int p = 0; p < n_pairs && pattern; p ++) {
      const std::string why = inadmissible(p, a.nfrm[utt_a[p]], b.nfrm[utt_b[p]]);
      if(! why.empty()) return refuse(why, who);
    }
    long long at = 0;
    for(int p = 0; p < n_pairs; p ++) {
      const int na = a.nfrm[utt_a[p]];
      const std::string why = line_fault(na, b.nfrm[utt_b[p]], center + at);
      if(! why.empty()) return refuse(pair_of(p) + why, who);
      at += na;
    }
  }
  // (with free ends the pattern is checked below, behind the cap; a slope that is refused there sizes nothing that is used)
  if(sub && pattern == 1) mode |= ALIGN_SLOPE;
  const bool slope = mode & ALIGN_SLOPE, bslope = banded && slope;
  // the cells of pair r's plane as far as its utterances exist; a band plane is held below 2^61 so that the total of any
  // list fits 64 bits
  auto plane_cells = [&](int r) -> long long {
    const int ua = utt_a[r], ub = utt_b[r];
    if(ua < 0 || ua >= a.n_utt) return 0;
    const long long na = std::max(a.nfrm[ua], 0);
    if(banded) return std::min(na * (2ll * std::max(band[r], 0) + 1), 1ll << 61);
    return ub < 0 || ub >= b.n_utt ? 0 : na * std::max(b.nfrm[ub], 0);
  };
  std::vector<int2> table, region;                                  // rule K1: the rows of the region of all pairs, and of one
  std::vector<AlignPair> pairs((size_t)n_pairs);
  long long cells = 0, rows = 0, frames = 0, steps = 0, n_tiles = 0, takes = 0;
  bool over = false;                                                // around a line: the cap is passed, and refused after the last band
  for(int p = 0; p < n_pairs; p ++) {
    const int ua = utt_a[p], ub = utt_b[p], bd = banded ? band[p] : 0;
    const std::string fault = pair_fault(a, b, p, ua, ub);
    if(! fault.empty()) return refuse(fault, who);
    const int na = a.nfrm[ua], nb = b.nfrm[ub];
    const int* line = around ? center + frames : nullptr;           // (frames: the rows of the pairs before this one)
    if(bd < 0) return refuse(pair_of(p) + "band < 0", who);
    const int least = ! banded || slope ? 0 : around ? around_min(na, nb, line) : band_min(na, nb);
    if(bd < least)
      return refuse(pair_of(p) + "a band of " + std::to_string(bd) + " is not connected for " + std::to_string(na) + " x " +
        std::to_string(nb) + " frames: " + (around ? "llsm_gpu_align_around_min is " : "llsm_gpu_align_band_min is ") +
        std::to_string(least), who);
    if(slope && ! sub) {
      const std::string why = inadmissible(p, na, nb);
      if(! why.empty()) return refuse(why, who);
    }
    // (a pair of the shape and band of the pair before it shares that pair's rows of the table: equal takes are common)
    const bool as_before = bslope && ! around && p > 0 && na == pairs[p - 1].na && nb == pairs[p - 1].nb && bd == pairs[p - 1].band;
    if(bslope && ! as_before && ! band_slope_rows(na, nb, bd, region, line))
      return refuse(pair_of(p) + "a band of " + std::to_string(bd) + " is not connected for the slope pattern on " + std::to_string(na) +
        " x " + std::to_string(nb) + " frames: " + (around ? "llsm_gpu_align_around_min is " + std::to_string(around_slope_min(na, nb, line))
        : "llsm_gpu_align_band_slope_min is " + std::to_string(band_slope_min(na, nb))), who);
    if(over) {                                                      // only the bands of the remaining pairs are still looked at
      if(cells < (1ll << 61)) cells += plane_cells(p);
      frames += na;
      continue;
    }
    AlignPair& q = pairs[p];
    q.a0 = a.frm_off[ua]; q.na = na; q.b0 = b.frm_off[ub]; q.nb = nb;
    q.cell0 = (int)cells; q.row0 = (int)rows; q.pos0 = (int)frames; q.band = bd; q.mv0 = steps;
    q.pad = as_before ? pairs[p - 1].pad : (int)table.size();       // where the pair's rows of the region start
    if(sub) q.pad = (int)takes;                                     // ... or, with free ends, its row of the matching function
    if(bslope && ! as_before) table.insert(table.end(), region.begin(), region.end());
    cells += plane_cells(p);                                        // (checked below: the offsets above are only used if it fits)
    if(cells > kMaxCells && around) { over = true; frames += na; continue; }
    if(cells > kMaxCells) {                                         // the total of the whole list, for the message
      for(int r = p + 1; r < n_pairs && (! banded || cells < (1ll << 61)); r ++) cells += plane_cells(r);
      return refuse(std::string(banded ? "the band planes hold " : "the distance planes hold ") + std::to_string(cells) +
        " cells, more than 2^28 = " + std::to_string(kMaxCells), who);
    }
    // the moves of a strip: one entry per anti-diagonal of its column window, as many as the widest strip of the pair has
    q.steps = 0;
    for(int i0 = 0, jlo, jhi; i0 < na; i0 += 64) {
      strip_span(banded, q, line, i0, jlo, jhi);
      n_tiles += (jhi - tile_floor(jlo)) / ALIGN_TILE + 1;
      q.steps = std::max(q.steps, strip_steps(mode, q, line, i0, table.data() + q.pad));
    }
    rows += slope ? 2ll * nb : nb; frames += na; takes += nb;
    steps += (long long)((na + 63) / 64) * q.steps;
  }
  if(over)
    return refuse("the band planes hold " + std::to_string(cells) + " cells, more than 2^28 = " + std::to_string(kMaxCells), who);
  if(sub) {                                                         // behind the cap: the pattern, then rule Q1 pair by pair
    if(pattern != 0 && pattern != 1) return refuse("slope = " + std::to_string(pattern) + " is neither 0 nor 1", who);
    for(int p = 0; p < n_pairs && pattern; p ++) {
      const std::string bound = sub_bound(pairs[p].na, pairs[p].nb);
      if(! bound.empty())
        return refuse(pair_of(p) + std::to_string(pairs[p].na) + " x " + std::to_string(pairs[p].nb) + " frames are not admissible: " + bound, who);
    }
  }
  // accepted: from here on this pass's scratch set changes (and those of the other calls, their planes among them, do not)
  llsm_gpu_batch::AlignScratch& sc = *J.sc;
  std::vector<int4> tiles; tiles.reserve((size_t)n_tiles);
  for(int p = 0; p < n_pairs; p ++)                                 // the tiles of the matrix that meet the rows' columns, overhang included
    for(int i0 = 0, jlo, jhi; i0 < pairs[p].na; i0 += ALIGN_TILE) {
      strip_span(banded, pairs[p], around ? center + pairs[p].pos0 : nullptr, i0, jlo, jhi);
      for(int j0 = tile_floor(jlo); j0 <= jhi; j0 += ALIGN_TILE) tiles.push_back(make_int4(p, i0, j0, 0));
    }
  hipSetDevice(J.owner -> ctx -> device);
  const size_t n_out = (size_t)frames + (size_t)n_pairs;
  if(sc.plane.alloc((size_t)cells) || sc.row.alloc((size_t)rows) || sc.out.alloc(n_out) || sc.moves.alloc((size_t)steps) ||
     sc.pairs.alloc(pairs.size()) || sc.tiles.alloc(tiles.size()) || sc.region.alloc(table.size()) ||
     (around && sc.center.alloc((size_t)frames)) || (sub && (sc.last.alloc((size_t)takes) || sc.span.alloc((size_t)2 * n_pairs)))) return -1;
  sc.cells = 0;                                                     // the planes are being rewritten
  LaunchCtx* P = & J.owner -> ctx -> lc;
  // (pageable sources: the copies have left the vectors when the calls return, and run in stream order)
  HIP_OK(hipMemcpyAsync(sc.pairs.p, pairs.data(), pairs.size() * sizeof(AlignPair), hipMemcpyHostToDevice, P -> stream));
  HIP_OK(hipMemcpyAsync(sc.tiles.p, tiles.data(), tiles.size() * sizeof(int4), hipMemcpyHostToDevice, P -> stream));
  if(bslope) HIP_OK(hipMemcpyAsync(sc.region.p, table.data(), table.size() * sizeof(int2), hipMemcpyHostToDevice, P -> stream));
  if(around) HIP_OK(hipMemcpyAsync(sc.center.p, center, (size_t)frames * sizeof(int), hipMemcpyHostToDevice, P -> stream));
  const AlignGeo geo = around ? ALIGN_GEO_LINE : banded ? ALIGN_GEO_BAND : ALIGN_GEO_FULL;
  AlignDev d;
  d.code_a = a.code; d.code_b = b.code;
  d.dim = J.dim; d.first = o.first; d.count = o.count;
  d.step_cost = o.step_cost; d.voicing_cost = o.voicing_cost;
  d.pairs = sc.pairs.p; d.n_pairs = n_pairs;
  const int* lines = around ? sc.center.p : nullptr;
  int rc = launch_align_dist(P, geo, d, sc.tiles.p, (int)tiles.size(), sc.plane.p, lines);
  if(! rc) rc = sub ? launch_align_sub_dtw(P, slope, d, sc.plane.p, sc.moves.p, sc.row.p, sc.out.p, (int)frames, sc.last.p, sc.span.p) :
                slope ? launch_align_slope_dtw(P, geo, d, sc.plane.p, sc.region.p, sc.moves.p, sc.row.p, sc.out.p, (int)frames, lines)
                      : launch_align_dtw(P, geo, d, sc.plane.p, sc.moves.p, sc.row.p, sc.out.p, (int)frames, lines);
  if(rc) return refuse(std::string("launch failed: ") + hipGetErrorString((hipError_t)rc), who);
  // into memory of our own first: a failed copy leaves the outputs untouched
  std::vector<float> host(n_out), host_last(sub && last_row ? (size_t)takes : 0);
  std::vector<int> host_span(sub && span ? (size_t)2 * n_pairs : 0);
  HIP_OK(hipMemcpyAsync(host.data(), sc.out.p, n_out * sizeof(float), hipMemcpyDeviceToHost, P -> stream));
  if(! host_last.empty()) HIP_OK(hipMemcpyAsync(host_last.data(), sc.last.p, host_last.size() * sizeof(float), hipMemcpyDeviceToHost, P -> stream));
  if(! host_span.empty()) HIP_OK(hipMemcpyAsync(host_span.data(), sc.span.p, host_span.size() * sizeof(int), hipMemcpyDeviceToHost, P -> stream));
  HIP_OK(hipStreamSynchronize(P -> stream));
  std::copy(host.begin(), host.begin() + frames, pos);
  if(cost) std::copy(host.begin() + frames, host.end(), cost);
  if(span) std::copy(host_span.begin(), host_span.end(), span);
  if(last_row) std::copy(host_last.begin(), host_last.end(), last_row);
  sc.cells = cells;
  return 0;
}

// The five calls: the batches' own rows, the name and the scratch set on a that follow from `mode`
int align_run(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b, int mode, int pattern,
  const int* center, const int* band, const llsm_gpu_align_options* opt, FP_TYPE* pos, FP_TYPE* cost) {
  const char* who = kAlignCalls[align_call(mode)].name;
  llsm_gpu_align_options o;
  if(align_head(a, b, n_pairs, opt, who, o)) return -1;
  const AlignJob J{a, side_of(a), side_of(b), a -> coder_os + a -> coder_ob + 3, o, & a -> align[align_call(mode)], who};
  return align_pass(J, n_pairs, utt_a, utt_b, mode, pattern, center, band, pos, cost);
}
}  // namespace

extern "C" int llsm_gpu_batch_align(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a,
  const int* utt_b, const llsm_gpu_align_options* opt, FP_TYPE* pos, FP_TYPE* cost) {
  return align_run(a, b, n_pairs, utt_a, utt_b, ALIGN_FULL, 0, nullptr, nullptr, opt, pos, cost);
}

// ---------------------------------------------------------------- a query inside a take: free ends (rules Q1 - Q5)
namespace { const char* const kSub = "llsm_gpu_batch_align_sub"; }

extern "C" int llsm_gpu_align_sub_rows(int na, int nb, int slope, int* lo, int* hi) {
  const char* who = "llsm_gpu_align_sub_rows";
  if(na < 1 || nb < 1) return refuse("na < 1 or nb < 1 (na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ")", who);
  if(slope != 0 && slope != 1)
    return refuse("slope = " + std::to_string(slope) + " is neither 0 nor 1 (na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ")", who);
  const std::string bound = slope ? sub_bound(na, nb) : "";
  if(! bound.empty()) return refuse(std::to_string(na) + " x " + std::to_string(nb) + " frames are not admissible: " + bound, who);
  for(int i = 0, l = 0, h = nb - 1; i < na && (lo || hi); i ++) {
    if(slope) align_sub_row(i, nb, l, h);
    if(lo) lo[i] = l;
    if(hi) hi[i] = h;
  }
  return 0;
}

extern "C" int llsm_gpu_batch_align_sub(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a, const int* utt_b,
  int slope, const llsm_gpu_align_options* opt, FP_TYPE* pos, int* span, FP_TYPE* cost, FP_TYPE* last_row) {
  llsm_gpu_align_options o;
  if(align_head(a, b, n_pairs, opt, kSub, o)) return -1;
  const AlignJob J{a, side_of(a), side_of(b), a -> coder_os + a -> coder_ob + 3, o, & a -> align_sub, kSub};
  return align_pass(J, n_pairs, utt_a, utt_b, ALIGN_SUB, slope, nullptr, nullptr, pos, cost, span, last_row);
}

// the distance planes of the last successful llsm_gpu_batch_align_sub with this batch as a, pair after pair, each [na][nb];
// dst == NULL: only the size
extern "C" long long llsm_gpu_batch_align_sub_plane(llsm_gpu_batch* a, float* dst, long long cap) {
  const char* who = "llsm_gpu_batch_align_sub_plane";
  if(! a) { refuse("NULL batch", who); return -1; }
  const long long n = a -> align_sub.cells;
  if(n == 0 || ! a -> align_sub.plane.p) { refuse(std::string("no ") + kSub + " has run on this batch", who); return -1; }
  if(dst) {
    if(cap < n) { refuse("destination too small", who); return -1; }
    if(hipStreamSynchronize(a -> ctx -> lc.stream) != hipSuccess ||
       hipMemcpy(dst, a -> align_sub.plane.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
      refuse("copy failed", who); return -1;
    }
  }
  return n;
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
  return align_run(a, b, n_pairs, utt_a, utt_b, ALIGN_BAND, 0, nullptr, band, opt, pos, cost);
}

// ---------------------------------------------------------------- local slopes within [1/2, 2] (rules L1 - L4)
extern "C" int llsm_gpu_align_slope_rows(int na, int nb, int* lo, int* hi) {
  const char* who = "llsm_gpu_align_slope_rows";
  if(na < 1 || nb < 1) return refuse("na < 1 or nb < 1 (na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ")", who);
  const std::string bound = slope_bound(na, nb);
  if(! bound.empty()) return refuse(std::to_string(na) + " x " + std::to_string(nb) + " frames are not admissible: " + bound, who);
  for(int i = 0, l, h; i < na && (lo || hi); i ++) {
    align_slope_row(i, na, nb, l, h);
    if(lo) lo[i] = l;
    if(hi) hi[i] = h;
  }
  return 0;
}

extern "C" int llsm_gpu_batch_align_slope(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a,
  const int* utt_b, const llsm_gpu_align_options* opt, FP_TYPE* pos, FP_TYPE* cost) {
  return align_run(a, b, n_pairs, utt_a, utt_b, ALIGN_SLOPE, 0, nullptr, nullptr, opt, pos, cost);
}

// ---------------------------------------------------------------- the slope pattern inside the band (rules K1 - K4)
namespace {
// empty, or why a pair is refused by the two host calls below
std::string band_slope_pair(int na, int nb) {
  if(na < 1 || nb < 1) return "na < 1 or nb < 1 (na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ")";
  const std::string bound = slope_bound(na, nb);
  if(! bound.empty()) return std::to_string(na) + " x " + std::to_string(nb) + " frames are not admissible: " + bound;
  // (the sweeps hold a few words per row; a pair of more rows than a call has cells fits no call)
  return na > kMaxCells ? "na = " + std::to_string(na) + " exceeds 2^28, the cells of a call" : "";
}
}  // namespace

extern "C" int llsm_gpu_align_band_slope_min(int na, int nb) {
  const std::string why = band_slope_pair(na, nb);
  if(! why.empty()) return refuse(why, "llsm_gpu_align_band_slope_min");
  try { return band_slope_min(na, nb); }                            // (the sweeps hold a few words per row)
  catch(const std::bad_alloc&) { return refuse("out of memory for " + std::to_string(na) + " rows", "llsm_gpu_align_band_slope_min"); }
}

extern "C" int llsm_gpu_align_band_slope_rows(int na, int nb, int band, int* lo, int* hi) {
  const char* who = "llsm_gpu_align_band_slope_rows";
  const std::string why = band_slope_pair(na, nb);
  if(! why.empty()) return refuse(why, who);
  if(band < 0) return refuse("band < 0 (na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ", band = " + std::to_string(band) + ")", who);
  std::vector<int2> rows;
  try {
    if(! band_slope_rows(na, nb, band, rows))
      return refuse("a band of " + std::to_string(band) + " is not connected for the slope pattern on " + std::to_string(na) + " x " +
        std::to_string(nb) + " frames: llsm_gpu_align_band_slope_min is " + std::to_string(band_slope_min(na, nb)), who);
  } catch(const std::bad_alloc&) { return refuse("out of memory for " + std::to_string(na) + " rows", who); }
  for(int i = 0; i < na && (lo || hi); i ++) {
    if(lo) lo[i] = rows[i].x;
    if(hi) hi[i] = rows[i].y;
  }
  return 0;
}

extern "C" int llsm_gpu_batch_align_band_slope(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a,
  const int* utt_b, const int* band, const llsm_gpu_align_options* opt, FP_TYPE* pos, FP_TYPE* cost) {
  return align_run(a, b, n_pairs, utt_a, utt_b, ALIGN_BAND | ALIGN_SLOPE, 0, nullptr, band, opt, pos, cost);
}

// ---------------------------------------------------------------- either pattern around a centre line (rules A1 - A3)
namespace {
// empty, or why the two host calls below refuse a pair, its pattern and its line
std::string around_pair(int na, int nb, const int* center, int slope) {
  if(na < 1 || nb < 1) return "na < 1 or nb < 1 (na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ")";
  // (the sweeps hold a few words per row; a pair of more rows than a call has cells fits no call)
  if(na > kMaxCells) return "na = " + std::to_string(na) + " exceeds 2^28, the cells of a call";
  if(slope != 0 && slope != 1) return "slope = " + std::to_string(slope) + " is neither 0 nor 1";
  if(! center) return "NULL center";
  if(slope) {
    const std::string bound = slope_bound(na, nb);
    if(! bound.empty()) return std::to_string(na) + " x " + std::to_string(nb) + " frames are not admissible: " + bound;
  }
  return line_fault(na, nb, center);
}
}  // namespace

extern "C" int llsm_gpu_align_around_min(int na, int nb, const int* center, int slope) {
  const char* who = "llsm_gpu_align_around_min";
  const std::string why = around_pair(na, nb, center, slope);
  if(! why.empty()) return refuse(why, who);
  try { return slope ? around_slope_min(na, nb, center) : around_min(na, nb, center); }
  catch(const std::bad_alloc&) { return refuse("out of memory for " + std::to_string(na) + " rows", who); }
}

extern "C" int llsm_gpu_align_around_rows(int na, int nb, const int* center, int band, int slope, int* lo, int* hi) {
  const char* who = "llsm_gpu_align_around_rows";
  const std::string why = around_pair(na, nb, center, slope);
  if(! why.empty()) return refuse(why, who);
  if(band < 0) return refuse("band < 0 (na = " + std::to_string(na) + ", nb = " + std::to_string(nb) + ", band = " + std::to_string(band) + ")", who);
  auto unconnected = [&](int least) {
    return refuse("a band of " + std::to_string(band) + " is not connected" + (slope ? " for the slope pattern" : "") + " around this line on " +
      std::to_string(na) + " x " + std::to_string(nb) + " frames: llsm_gpu_align_around_min is " + std::to_string(least), who);
  };
  if(! slope) {
    const int least = around_min(na, nb, center);
    if(band < least) return unconnected(least);
    for(int i = 0; i < na && (lo || hi); i ++) {
      if(lo) lo[i] = (int)std::max((long long)center[i] - band, 0ll);
      if(hi) hi[i] = (int)std::min((long long)center[i] + band, (long long)nb - 1);
    }
    return 0;
  }
  std::vector<int2> rows;
  try { if(! band_slope_rows(na, nb, band, rows, center)) return unconnected(around_slope_min(na, nb, center)); }
  catch(const std::bad_alloc&) { return refuse("out of memory for " + std::to_string(na) + " rows", who); }
  for(int i = 0; i < na && (lo || hi); i ++) {
    if(lo) lo[i] = rows[i].x;
    if(hi) hi[i] = rows[i].y;
  }
  return 0;
}

// Every operation below is one float64 operation of llsm_gpu.h's recipe, in its order.
extern "C" int llsm_gpu_align_center_line(int na_c, int nb_c, const FP_TYPE* pos_c, int na, int nb, int* center) {
  const char* who = "llsm_gpu_align_center_line";
  if(na_c < 1 || nb_c < 1 || na < 1 || nb < 1)
    return refuse("a size below 1 (na_c = " + std::to_string(na_c) + ", nb_c = " + std::to_string(nb_c) + ", na = " + std::to_string(na) +
      ", nb = " + std::to_string(nb) + ")", who);
  if(! pos_c || ! center) return refuse("NULL pos_c or center", who);
  for(int k = 0; k < na_c; k ++)
    if(! (pos_c[k] >= 0 && pos_c[k] <= (FP_TYPE)(nb_c - 1)))         // (a NaN fails both comparisons)
      return refuse("pos_c[" + std::to_string(k) + "] = " + std::to_string(pos_c[k]) + " is NaN or outside [0, " + std::to_string(nb_c - 1) + "]", who);
  const double s = nb_c > 1 ? (double)(nb - 1) / (double)(nb_c - 1) : 0.0;
  long long top = 0;
  for(int i = 0; i < na; i ++) {
    double y = pos_c[0];
    if(na_c > 1 && na > 1) {
      const double prod = (double)i * (double)(na_c - 1);
      const double x = prod / (double)(na - 1);
      const long long k = std::min((long long)std::floor(x), (long long)na_c - 2);
      const double rise = (double)pos_c[k + 1] - (double)pos_c[k], frac = x - (double)k;
      const double part = rise * frac;
      y = (double)pos_c[k] + part;
    }
    const double scaled = y * s;
    const long long c = (long long)std::floor(scaled + 0.5);
    top = std::max(top, std::min((long long)nb - 1, std::max(0ll, c)));
    center[i] = (int)top;
  }
  return 0;
}

extern "C" int llsm_gpu_batch_align_around(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a,
  const int* utt_b, const int* center, const int* band, int slope, const llsm_gpu_align_options* opt, FP_TYPE* pos, FP_TYPE* cost) {
  return align_run(a, b, n_pairs, utt_a, utt_b, ALIGN_AROUND | ALIGN_BAND, slope, center, band, opt, pos, cost);
}

// ---------------------------------------------------------------- pooled vectors (rule P1) and coarse to fine in one call
namespace {
const char* const kPyramid = "llsm_gpu_batch_align_pyramid";
const char* const kPool = "llsm_gpu_batch_pool_code";

int pool_frames(int nfrm, int factor) { return (int)(((long long)nfrm + factor - 1) / factor); }

// the table of k_pool_code (kernels.h) to the device and the launch, in stream order; out: [coarse_frames][dim]
int pool_launch(llsm_gpu_context* ctx, const float* code_a, const float* code_b, const std::vector<int4>& tab, int dim, int factor,
  long long coarse_frames, DevBuf<int4>& d_tab, DevBuf<float>& out, const char* who) {
  if(d_tab.alloc(tab.size()) || out.alloc((size_t)coarse_frames * dim)) return -1;
  LaunchCtx* P = & ctx -> lc;
  HIP_OK(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * sizeof(int4), hipMemcpyHostToDevice, P -> stream));
  const int rc = launch_pool_code(P, code_a, code_b, d_tab.p, (int)tab.size(), dim, factor, coarse_frames, out.p);
  if(rc) return refuse(std::string("launch failed: ") + hipGetErrorString((hipError_t)rc), who);
  return 0;
}
}  // namespace

extern "C" int llsm_gpu_pool_frames(int nfrm, int factor) {
  if(nfrm < 1 || factor < 1 || factor > 64)
    return refuse("nfrm < 1 or a factor outside [1, 64] (nfrm = " + std::to_string(nfrm) + ", factor = " + std::to_string(factor) + ")",
      "llsm_gpu_pool_frames");
  return pool_frames(nfrm, factor);
}

extern "C" int llsm_gpu_batch_pool_code(const llsm_gpu_batch* b, int factor, int n, const int* utts, FP_TYPE* dst) {
  if(! b) return refuse("NULL batch", kPool);
  if(b -> coder_os == 0) return refuse("the coder is not enabled", kPool);
  if(factor < 1 || factor > 64) return refuse("factor = " + std::to_string(factor) + " lies outside [1, 64]", kPool);
  if(n < 0) return refuse("n < 0", kPool);
  if(n == 0) return 0;
  if(! utts || ! dst) return refuse("NULL list or dst", kPool);
  std::vector<int4> tab((size_t)n);
  long long frames = 0;
  for(int k = 0; k < n; k ++) {
    const int u = utts[k];
    if(u < 0 || u >= b -> lay.n_utt) return refuse("entry " + std::to_string(k) + ": utterance " + std::to_string(u) + " is outside the batch", kPool);
    if(b -> nfrm[u] <= 0) return refuse("entry " + std::to_string(k) + ": an utterance without frames", kPool);
    // (an offset that does not fit is never used: the total is refused below)
    tab[k] = make_int4(b -> frm_off[u], b -> nfrm[u], (int)frames, 0);
    frames += pool_frames(b -> nfrm[u], factor);
  }
  if(frames > kMaxCells) return refuse("the pooled vectors hold " + std::to_string(frames) + " frames, more than 2^28 = " + std::to_string(kMaxCells), kPool);
  const int dim = b -> coder_os + b -> coder_ob + 3;
  hipSetDevice(b -> ctx -> device);
  DevBuf<int4> d_tab; DevBuf<float> out;                            // (local: the stream is synchronised before they go)
  const float* code = (const float*)b -> arr[LLSM_GPU_CODE];
  if(pool_launch(b -> ctx, code, code, tab, dim, factor, frames, d_tab, out, kPool)) return -1;
  // into memory of our own first: a failed copy leaves dst untouched
  std::vector<float> host((size_t)frames * dim);
  hipStream_t stream = b -> ctx -> lc.stream;
  const hipError_t e = hipMemcpyAsync(host.data(), out.p, host.size() * sizeof(float), hipMemcpyDeviceToHost, stream);
  const hipError_t s = hipStreamSynchronize(stream);                // (whatever the copy said: the buffers are freed on return)
  if(e != hipSuccess || s != hipSuccess) return refuse(std::string("copy failed: ") + hipGetErrorString(e != hipSuccess ? e : s), kPool);
  std::copy(host.begin(), host.end(), dst);
  return 0;
}

extern "C" int llsm_gpu_batch_align_pyramid(llsm_gpu_batch* a, const llsm_gpu_batch* b, int n_pairs, const int* utt_a,
  const int* utt_b, int factor, int margin, int slope, const llsm_gpu_align_options* opt, FP_TYPE* pos, FP_TYPE* cost,
  int* center_out, int* band_out) {
  const char* who = kPyramid;
  // 1: what llsm_gpu_batch_align refuses short of its cap
  llsm_gpu_align_options o;
  if(align_head(a, b, n_pairs, opt, who, o)) return -1;
  if(n_pairs == 0) return 0;
  if(! utt_a || ! utt_b) return refuse("NULL utterance list", who);
  if(! pos) return refuse("NULL pos", who);
  const AlignSide fine_a = side_of(a), fine_b = side_of(b);
  for(int p = 0; p < n_pairs; p ++) {
    const std::string why = pair_fault(fine_a, fine_b, p, utt_a[p], utt_b[p]);
    if(! why.empty()) return refuse(why, who);
  }
  // 2
  if(factor < 2 || factor > 64) return refuse("factor = " + std::to_string(factor) + " lies outside [2, 64]", who);
  if(margin < 0) return refuse("margin < 0", who);
  if(slope != 0 && slope != 1) return refuse("slope = " + std::to_string(slope) + " is neither 0 nor 1", who);
  // 3: rule L1 on the fine and on the coarse pair
  std::vector<int> nca((size_t)n_pairs), ncb((size_t)n_pairs), off_a((size_t)n_pairs + 1, 0), off_b((size_t)n_pairs + 1, 0);
  for(int p = 0; p < n_pairs; p ++) {
    const int na = fine_a.nfrm[utt_a[p]], nb = fine_b.nfrm[utt_b[p]];
    nca[p] = pool_frames(na, factor); ncb[p] = pool_frames(nb, factor);
    if(! slope) continue;
    const std::string why = inadmissible(p, na, nb);
    if(! why.empty()) return refuse(why, who);
    const std::string bound = slope_bound(nca[p], ncb[p]);
    if(! bound.empty())
      return refuse(pair_of(p) + std::to_string(na) + " x " + std::to_string(nb) + " frames pool to " + std::to_string(nca[p]) + " x " +
        std::to_string(ncb[p]) + " at factor " + std::to_string(factor) + ", which are not admissible: " + bound + " (a smaller factor may admit the pair)", who);
  }
  // 4: the planes of the coarse pass.  Under the cap the coarse frames of either side are 2^28 at the most, as a pair has
  // no fewer cells than frames on either side, so every offset below fits an int.
  long long cells = 0;
  for(int p = 0; p < n_pairs; p ++) cells += (long long)nca[p] * ncb[p];
  if(cells > kMaxCells)
    return refuse("the coarse distance planes hold " + std::to_string(cells) + " cells, more than 2^28 = " + std::to_string(kMaxCells), who);
  // accepted.  Y1: the pooled rows of a's utterances, pair after pair, then those of b's, in one launch
  for(int p = 0; p < n_pairs; p ++) { off_a[p + 1] = off_a[p] + nca[p]; off_b[p + 1] = off_b[p] + ncb[p]; }
  const int frames_a = off_a[n_pairs], frames_b = off_b[n_pairs], dim = a -> coder_os + a -> coder_ob + 3;
  std::vector<int4> tab((size_t)2 * n_pairs);
  std::vector<int> own((size_t)n_pairs);                            // the coarse sides hold one utterance per pair
  for(int p = 0; p < n_pairs; p ++) {
    tab[p] = make_int4(fine_a.frm_off[utt_a[p]], fine_a.nfrm[utt_a[p]], off_a[p], 0);
    tab[(size_t)n_pairs + p] = make_int4(fine_b.frm_off[utt_b[p]], fine_b.nfrm[utt_b[p]], frames_a + off_b[p], 1);
    own[p] = p;
  }
  hipSetDevice(a -> ctx -> device);
  if(pool_launch(a -> ctx, fine_a.code, fine_b.code, tab, dim, factor, (long long)frames_a + frames_b, a -> pyramid_tab, a -> pyramid_code, who))
    return -1;
  // Y2: the coarse pass over the pooled rows
  const AlignSide coarse_a{a -> pyramid_code.p, off_a.data(), nca.data(), n_pairs};
  const AlignSide coarse_b{a -> pyramid_code.p + (size_t)frames_a * dim, off_b.data(), ncb.data(), n_pairs};
  std::vector<FP_TYPE> pos_c((size_t)frames_a);
  const AlignJob coarse{a, coarse_a, coarse_b, dim, o, & a -> pyramid[0], who};
  if(align_pass(coarse, n_pairs, own.data(), own.data(), slope ? ALIGN_SLOPE : ALIGN_FULL, 0, nullptr, nullptr, pos_c.data(), nullptr)) return -1;
  // Y3, Y4: the lines and the bands, by the public host calls
  long long rows = 0;
  for(int p = 0; p < n_pairs; p ++) rows += fine_a.nfrm[utt_a[p]];
  std::vector<int> center((size_t)rows), band((size_t)n_pairs);
  rows = 0;
  for(int p = 0; p < n_pairs; p ++) {
    const int na = fine_a.nfrm[utt_a[p]], nb = fine_b.nfrm[utt_b[p]];
    int* line = center.data() + rows;
    if(llsm_gpu_align_center_line(nca[p], ncb[p], pos_c.data() + off_a[p], na, nb, line)) return refuse(pair_of(p) + llsm_gpu_last_error(), who);
    const int least = llsm_gpu_align_around_min(na, nb, line, slope);
    if(least < 0) return refuse(pair_of(p) + llsm_gpu_last_error(), who);
    band[p] = std::max((int)std::min((long long)margin * factor, (long long)nb - 1), least);
    rows += na;
  }
  // Y5: the fine pass; it alone can still refuse, for its cap
  const AlignJob fine{a, fine_a, fine_b, dim, o, & a -> pyramid[1], who};
  if(align_pass(fine, n_pairs, utt_a, utt_b, ALIGN_AROUND | ALIGN_BAND, slope, center.data(), band.data(), pos, cost)) return -1;
  if(center_out) std::copy(center.begin(), center.end(), center_out);
  if(band_out) std::copy(band.begin(), band.end(), band_out);
  return 0;
}
