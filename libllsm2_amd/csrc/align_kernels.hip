// align_kernels.hip -- alignment of utterance pairs: llsm_gpu_batch_align (rules D1 - D3: llsm_gpu.h),
// llsm_gpu_batch_align_band (rules B1 - B4, section 25), llsm_gpu_batch_align_slope (rules L1 - L4, section 27; its planes are
// k_align_dist_t's full ones) and llsm_gpu_batch_align_band_slope (rules K1 - K4, section 28; its planes are k_align_dist_t's
// band ones); the path kernel of the last two, k_align_slope_dtw_t, is described above it; and llsm_gpu_batch_align_around
// (rules A1 - A3, section 30), which runs the band instantiations of all three around a centre line of the caller's; and
// k_pool_code (rule P1, section 34), the pooled vectors of llsm_gpu_batch_pool_code and of the coarse pass of
// llsm_gpu_batch_align_pyramid, which is otherwise made of the kernels above; and llsm_gpu_batch_align_sub (rules Q1 - Q5,
// section 35), whose planes are k_align_dist_t's full ones and whose paths are the two path kernels of the full geometry with
// free ends (k_align_sub_dtw, k_align_sub_slope_dtw: the note above k_align_dtw_t); host side: align.cpp.  Three kernel
// templates, each instantiated for the three geometries (AlignGeo: kernels.h):
//   full    row i spans columns 0 ... nb - 1 and is stored as it is: off = 0, width = nb, all of it known when compiling
//   band    row i spans lo_i = max(off_i, 0) ... hi_i = min(off_i + 2 band, nb - 1), off_i = c_i - band with c_i =
//           align_band_center(i), and entry q of its row of the plane [na][width = 2 band + 1] is column off_i + q
//   line    the band with c_i read from a device table of ints, center[pair.pos0 + i] (align_center): one read-only load
//           where the band computes -- per row of a tile in k_align_dist_t (the off[] staged in LDS), per lane and strip
//           for its own row and the row above in the path kernels, and once per strip in the walks back -- so the step
//           loops are the band's.  What is said of the band below holds for any line that does not decrease (rule A1), as
//           it rests on two facts alone: all lanes of a strip count their steps from one wlo, and lo and hi of the rows do
//           not decrease (without the slope pattern; with it the window is a reduction over the rows).  That covers the
//           distance between the reads and the writes of the hand-over rows and that every entry of a band plane is
//           written once: a row's entries are the columns off_i ... off_i + 2 band, all within the strip's tiles, which
//           reach from the first row's off to the last row's off + 2 band.
//
//   k_align_dist_t   D1 / B2: the distance planes of all pairs in one launch.  A workgroup of 256 threads takes a tile of
//                    64 x 64 cells of one pair's matrix from the host's tile table; wavefront w owns rows 16 w ... 16 w + 15
//                    of the tile and lane l column j0 + l, so a thread keeps 16 cells of one column in registers and a
//                    wavefront's stores to a row of the plane are consecutive words.  The two row blocks of LLSM_GPU_CODE
//                    go through the LDS 32 columns at a time, each element staged once per tile.  Every thread walks k
//                    ascending for each cell it owns: D1's order is per cell, there is no cross-lane reduction, and the
//                    bits follow from the rule.  A tile of a band may start left of column 0 or run past nb - 1 where the
//                    band of a row hangs over the matrix: its loads clamp to the matrix and it stores +infinity there, so
//                    every entry of a band plane is written, once.
//   k_align_dtw_t    D2 - D3 / B3 - B4: one wavefront per pair.  Lane l owns row 64 s + l of strip s and walks the
//                    anti-diagonals of the strip's column window [wlo, whi] = [lo of its first row, hi of its last]: at
//                    step t it is on column wlo + t - l, and a strip of r rows takes whi - wlo + r steps (full: wlo = 0, nb
//                    + r - 1 steps).
//
// LDS of k_align_dist_t.  The A block is [64][32 + 4] floats: a wavefront reads A[row][k ... k + 3] with every lane on the
// same address (a broadcast, one 16-byte read per row and four k), so the padding only keeps the rows 16-byte aligned.
// The B block is stored transposed, [32][64 + 1]: lane l reads Bt[k][l] -- consecutive words, no conflict -- and the
// staging pass, whose lanes run along k for the sake of coalesced global reads, writes Bt[k][row] at a stride of 65 words:
// an odd stride walks all 32 banks of a write, where the unpadded 64 would put the 32 lanes of a half-wavefront on one
// bank (the stride argument of the tile kernel of the coder).
//
// k_align_dtw_t, the forward pass.  acc[i-1][j] is what lane l - 1 computed one step ago and acc[i-1][j-1] what it computed
// two steps ago, i.e. what this lane received as `up` one step ago: one cross-lane move per step, a wavefront shift by one
// lane on the vector ALU (DPP), no LDS round trip.  Lane 0 takes both from the row the strip above left behind: its lane
// 63 stores acc[64 s + 63][j] into a per-pair row of nb floats, indexed by the column itself.  All lanes of a strip count
// their steps from the same wlo: lane 0 loads column x at step x - wlo - 2 DTW_U + 1 at the earliest ... x - wlo at the
// latest, lane 63 stores column x at step x - wlo + 63, so the reads stay ahead of the writes by 63 steps at the least,
// wherever the windows of the strips start, and one row serves.  The D values and that row are loaded DTW_U steps ahead, so
// the dependent chain of a step is the shift, two additions, the compare / selects and the addition of D.
// Which of the three candidates of a cell exist (rule B3; in the full geometry D2's forced borders: the left one alone on
// row 0, the upper one alone on column 0) is decided by integer comparisons, never by the values, so what a lane that was
// outside its row's range hands on -- and what an earlier strip left in the hand-over row outside the range of the row
// that wrote it last -- is never used.  `diag` of a strip starts as column wlo - 1 of the hand-over row: where the row above
// starts further left than the strip, lane 0's first cell has a diagonal predecessor there.  In the full geometry wlo is 0
// and column 0 has no diagonal candidate, so nothing is read.
// The moves of a step, 2 bits per lane, are two ballots: lane t % 64 keeps the pair of 64-bit masks of step t and the
// wavefront stores 64 steps (1 KiB) at a time; a strip has AlignPair::steps entries, the most any strip of the pair takes.
// The backtrack is a scalar walk: a move 0 goes two steps back, a move 1 or 2 one step back, so the walk reads the masks
// in descending order; the wavefront loads 64 steps at a time (lane k: step base + k) and reads them with v_readlane.  It
// notes lo / hi of each row and writes pos when it leaves the row.  It follows the stored moves -- the forward pass has
// stored the only move there is on row 0 and column 0 -- and stops rather than step outside the matrix or past a strip's
// masks, which no stored move asks for; it ends at (0, 0) after at most na + nb - 2 moves.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "kernels.h"
#include "dev_common.h"
#include "launch.h"

// c_i of pair p (0 <= i < na): rule B1's diagonal, computed, or with ALIGN_GEO_LINE rule A1's line, one load from the table
template <int GEO>
DEV int align_center(const int* __restrict__ center, const AlignPair& p, int i) {
  if constexpr(GEO == ALIGN_GEO_LINE) return center[(size_t)p.pos0 + i];
  else return align_band_center(i, p.na, p.nb);
}

// ---------------------------------------------------------------- D1: distance planes
#define AD_NT 256
#define AD_KC 32                                   // columns of CODE per LDS stage
#define AD_AS (AD_KC + 4)                          // row stride of the A block, floats
#define AD_BS (ALIGN_TILE + 1)                     // row stride of the transposed B block, floats
#define AD_R (ALIGN_TILE / (AD_NT / WAVE))         // rows per thread: 16

// The sums of rule D1 of the 16 cells this thread owns in the tile at (i0, j0) of the rows A [na][dim] against B [nb][dim].
// Rows beyond the last are read as the last row (and, with LOW, columns before the first as the first); the caller does
// not use their sums.  Ends after the barrier that follows the last stage.
template <bool LOW>
DEV void align_tile_sums(const float* __restrict__ A, const float* __restrict__ B, int dim, int first, int count, int na,
  int nb, int i0, int j0, float* sa, float* sb, float (& acc)[AD_R]) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), r0 = (tid >> 6) * AD_R;
#pragma unroll
  for(int r = 0; r < AD_R; r ++) acc[r] = 0.0f;
  const int sk = tid & (AD_KC - 1), sr = tid >> 5;                  // staging: lanes along k
  for(int k0 = 0; k0 < count; k0 += AD_KC) {
    const int kn = min(AD_KC, count - k0);
    __syncthreads();                                                // the stage before has been read
#pragma unroll
    for(int r = 0; r < ALIGN_TILE; r += AD_NT / AD_KC) {
      const int row = r + sr;
      float a = 0.0f, b = 0.0f;
      if(sk < kn) {
        const int jb = LOW ? max(min(j0 + row, nb - 1), 0) : min(j0 + row, nb - 1);
        a = A[(size_t)min(i0 + row, na - 1) * dim + first + k0 + sk];
        b = B[(size_t)jb * dim + first + k0 + sk];
      }
      sa[row * AD_AS + sk] = a;
      sb[sk * AD_BS + row] = b;
    }
    __syncthreads();
    if(kn == AD_KC) {
#pragma unroll
      for(int k = 0; k < AD_KC; k += 4) {
        const float b0 = sb[k * AD_BS + lane], b1 = sb[(k + 1) * AD_BS + lane], b2 = sb[(k + 2) * AD_BS + lane],
                    b3 = sb[(k + 3) * AD_BS + lane];
#pragma unroll
        for(int r = 0; r < AD_R; r ++) {
          const float4 a = *(const float4*)& sa[(r0 + r) * AD_AS + k];
          float t = __fsub_rn(a.x, b0); acc[r] = __fadd_rn(acc[r], __fmul_rn(t, t));
          t = __fsub_rn(a.y, b1); acc[r] = __fadd_rn(acc[r], __fmul_rn(t, t));
          t = __fsub_rn(a.z, b2); acc[r] = __fadd_rn(acc[r], __fmul_rn(t, t));
          t = __fsub_rn(a.w, b3); acc[r] = __fadd_rn(acc[r], __fmul_rn(t, t));
        }
      }
    } else {                                                        // the last stage of a count that is no multiple of 32
      for(int k = 0; k < kn; k ++) {
        const float b = sb[k * AD_BS + lane];
#pragma unroll
        for(int r = 0; r < AD_R; r ++) {
          const float t = __fsub_rn(sa[(r0 + r) * AD_AS + k], b);
          acc[r] = __fadd_rn(acc[r], __fmul_rn(t, t));
        }
      }
    }
  }
  __syncthreads();                                                  // (count == 0 never comes here)
}

// Lane l is on column j0 + l of the matrix, which with BAND may lie outside it; entry q = j - off_i of row i of the plane
// is stored if it is within the row (full: q = j)
template <int GEO>
__global__ __launch_bounds__(AD_NT) void k_align_dist_t(AlignDev d, const int4* __restrict__ tiles, float* __restrict__ plane,
  const int* __restrict__ center) {
  constexpr bool BAND = GEO != ALIGN_GEO_FULL;
  __shared__ __attribute__((aligned(16))) float sa[ALIGN_TILE * AD_AS];
  __shared__ float sb[AD_KC * AD_BS];
  __shared__ int va[ALIGN_TILE], vb[ALIGN_TILE], off[BAND ? ALIGN_TILE : 1];
  const int4 tl = tiles[blockIdx.x];
  const AlignPair p = d.pairs[tl.x];
  const int i0 = tl.y, j0 = tl.z;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), r0 = (tid >> 6) * AD_R;
  // rows beyond the pair's last are read as its last row and never written
  const float* A = d.code_a + (size_t)p.a0 * d.dim;
  const float* B = d.code_b + (size_t)p.b0 * d.dim;
  if(tid < ALIGN_TILE) {
    const int i = min(i0 + tid, p.na - 1);
    va[tid] = A[(size_t)i * d.dim] > 0.5f;
    if constexpr(BAND) off[tid] = align_center<GEO>(center, p, i) - p.band;
  } else if(tid < 2 * ALIGN_TILE) {
    const int jb = min(j0 + tid - ALIGN_TILE, p.nb - 1);
    vb[tid - ALIGN_TILE] = B[(size_t)(BAND ? max(jb, 0) : jb) * d.dim] > 0.5f;
  }
  float acc[AD_R];
  align_tile_sums<BAND>(A, B, d.dim, d.first, d.count, p.na, p.nb, i0, j0, sa, sb, acc);     // (va / vb / off are written)
  const int j = j0 + lane, width = BAND ? 2 * p.band + 1 : p.nb;
  const bool inside = (! BAND || j >= 0) && j < p.nb;
  if(! BAND && ! inside) return;
  const int vj = vb[lane];
  float* out = plane + (size_t)p.cell0;
#pragma unroll
  for(int r = 0; r < AD_R; r ++) {
    const int i = i0 + r0 + r, q = BAND ? j - off[r0 + r] : j;
    if(i < p.na && (! BAND || (q >= 0 && q < width)))
      out[(size_t)i * width + q] = BAND && ! inside ? __builtin_huge_valf() : va[r0 + r] != vj ? __fadd_rn(acc[r], d.voicing_cost) : acc[r];
  }
}

// ---------------------------------------------------------------- D2 - D3 / B3 - B4: the path
#define DTW_U 8                                    // steps loaded ahead
// lane l reads lane l - 1 (a wavefront shift right by one on the vector ALU); lane 0 keeps `first`
#define DPP_WAVE_SHR1 0x138
DEV float wave_shr1(float first, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, first), __builtin_bit_cast(int, v),
    DPP_WAVE_SHR1, 0xF, 0xF, false));
}

struct DtwBlock { float d[DTW_U], p[DTW_U]; };
// For the DTW_U steps ahead, the first of which has this lane on column j0: D of the lane's row (entry q = column - off of
// `width`) and the hand-over row, which lane 0 of a strip below the first alone uses -- so a lane may read it at lane 0's
// column or at its own: one address for the wavefront keeps the full geometry at 72 VGPRs, the own column is what a band
// has computed for D anyway.  Entries outside the rows are read at their ends and not used.
template <bool BAND>
DEV void dtw_load(DtwBlock& b, const float* __restrict__ drow, const float* hand, int j0, int lane, int off, int width, int nb) {
#pragma unroll
  for(int k = 0; k < DTW_U; k ++) {
    b.d[k] = drow[min(max(j0 + k - off, 0), width - 1)];
    b.p[k] = hand[min(max(BAND ? j0 + k : j0 + lane + k, 0), nb - 1)];
  }
}

// The free ends of llsm_gpu_batch_align_sub (rules Q1, Q3 - Q5) are one more template parameter of the two path kernels, a
// pack SUB that is empty -- the kernels as they were, argument for argument -- or (float* last_rows, int* span): acc of every
// pair's last row (pair p's nb floats from float pairs[p].pad) and {begin, end} of every pair.  OPEN = the pack is not empty.
// With the empty pack the six instantiations compile to the instructions they had before the parameter (72 / 74 / 72 and 94 /
// 96 / 96 VGPRs, no scratch: DESIGN.md section 35); a body shared through a device function did not keep them.  Under
// `if constexpr` OPEN changes four things, for the full geometry only:
//   row 0      takes acc = D on every column, not on (0, 0) alone, and the plain kernel's forced left move on row 0 goes;
//              column 0 stays forced.  What is stored as the move of a cell of row 0 is never read.
//   the rows   of the slope kernel are Q1's (align_sub_row: ceil(i / 2) ... nb - 1), not L1's; the three ranges follow from
//              them as they do from L1's, and the strip window is [lo of the first row, nb - 1].  Row 64 s starts on 32 s and
//              row 64 s - 1 on 32 s too, so lane 0 still meets no cell of the region left of wlo.
//   the end    lane (na - 1) & 63 of the last strip keeps (best, end) under Q4 while it walks its row -- it starts on the
//              row's first column and takes a later one only if acc is strictly smaller -- and stores acc[na-1][j] to the
//              pair's row of the matching function: one lane, one compare and one word a step, beside the hand-over store.
//              After the loop end goes to the wavefront as a scalar and is written with the cost.
//   the walk   starts on (na - 1, end) and stops on reaching row 0, whose column is begin; begin and end go into span as ints.
DEV float* sub_last_rows() { return nullptr; }
DEV float* sub_last_rows(float* last_rows, int*) { return last_rows; }
DEV int* sub_span() { return nullptr; }
DEV int* sub_span(float*, int* span) { return span; }

template <int GEO, class... SUB>
__global__ __launch_bounds__(WAVE) void k_align_dtw_t(AlignDev d, const float* __restrict__ plane, uint4* __restrict__ moves,
  float* __restrict__ hand_rows, float* __restrict__ out, int cost0, const int* __restrict__ center, SUB... sub) {
  constexpr bool BAND = GEO != ALIGN_GEO_FULL, OPEN = sizeof...(SUB) != 0;
  float* const last_rows = sub_last_rows(sub...); int* const span = sub_span(sub...);
  static_assert(! OPEN || ! BAND, "the free ends are instantiated for the full geometry only");
  const int lane = threadIdx.x;
  const AlignPair p = d.pairs[blockIdx.x];
  const int na = p.na, nb = p.nb, band = p.band, width = BAND ? 2 * band + 1 : nb;
  const float* D = plane + (size_t)p.cell0;
  float* hand = hand_rows + (size_t)p.row0;
  uint4* mv = moves + p.mv0;
  const long long per_strip = p.steps;
  const float step = d.step_cost;
  const int nstrips = (na + WAVE - 1) / WAVE;
  float v = 0.0f;                                                     // acc of this lane's last cell
  // OPEN (rule Q4): the lane that owns row na - 1 keeps the least acc of its row and its smallest column while it walks the
  // row in the last strip, and leaves the row itself in the pair's row of the matching function
  float* lastrow = OPEN ? last_rows + (size_t)p.pad : nullptr;
  float best = 0.0f; int end = 0;
  for(int s = 0; s < nstrips; s ++) {
    const int i = s * WAVE + lane, rows = min(WAVE, na - s * WAVE);
    const bool ender = OPEN && lane == ((na - 1) & (WAVE - 1)) && s + 1 == nstrips;
    // BAND: the ranges of this lane's row and of the row above; an empty range (1, 0) where there is no such row
    int off = 0, lo = 1, hi = 0, plo = 1, phi = 0;
    if constexpr(BAND) if(i < na) {
      const int c = align_center<GEO>(center, p, i);
      off = c - band; lo = max(off, 0); hi = min(c + band, nb - 1);
      if(i > 0) { const int cp = align_center<GEO>(center, p, i - 1); plo = max(cp - band, 0); phi = min(cp + band, nb - 1); }
    }
    const int wlo = BAND ? __shfl(lo, 0) : 0, whi = BAND ? __shfl(hi, rows - 1) : nb - 1, nsteps = whi - wlo + rows;
    const float* drow = D + (size_t)min(i, na - 1) * width;
    uint4* mvs = mv + (long long)s * per_strip;
    // what `up` was one step ago (file head; the full geometry has no such predecessor to read)
    float diag = BAND ? hand[max(wlo - 1, 0)] : 0.0f;
    unsigned long long w0 = 0, w1 = 0;                                // the masks of step (t & ~63) + lane
    DtwBlock cur, nxt;
    dtw_load<BAND>(cur, drow, hand, wlo - lane, lane, off, width, nb);
    for(int t0 = 0; t0 < nsteps; t0 += DTW_U) {
      dtw_load<BAND>(nxt, drow, hand, wlo + t0 + DTW_U - lane, lane, off, width, nb);
#pragma unroll
      for(int k = 0; k < DTW_U; k ++) {
        const int t = t0 + k;
        if(t >= nsteps) break;
        const int j = wlo + t - lane;
        const bool on = BAND ? j >= lo && j <= hi : i < na && j >= 0 && j < nb;
        // B3: which candidates exist, from the ranges of the row and of the row above (the full geometry does not ask).
        // The order of these statements is the one the banded kernel was measured with: the shift first cost it 0.8 %.
        const bool has_dg = j - 1 >= plo && j - 1 <= phi, has_up = j >= plo && j <= phi, has_lf = j - 1 >= lo;
        const float up_raw = wave_shr1(cur.p[k], v);                  // acc[i-1][j]
        const float up = __fadd_rn(up_raw, step), lf = __fadd_rn(v, step);
        float m = diag; int move = 0;
        if constexpr(BAND) {                                          // B3: the first candidate that exists ...
          if(! has_dg) { m = up; move = 1; }
          if(! has_dg && ! has_up) { m = lf; move = 2; }
          if(has_dg && has_up && up < m) { m = up; move = 1; }        // ... and a later one only if strictly smaller
          if((has_dg || has_up) && has_lf && lf < m) { m = lf; move = 2; }
        } else {                                                      // D2, which is B3 where every row spans 0 ... nb - 1
          if(up < m) { m = up; move = 1; }
          if(lf < m) { m = lf; move = 2; }
          if constexpr(! OPEN) if(i == 0) { m = lf; move = 2; }       // the borders are forced, not compared
          if(j == 0) { m = up; move = 1; }
        }
        float acc = __fadd_rn(m, cur.d[k]);
        if(OPEN ? i == 0 : i == 0 && j == 0) { acc = cur.d[k]; move = 0; }   // Q3: a path starts anywhere on row 0, at no cost
        diag = up_raw;
        if(on) v = acc;
        if constexpr(OPEN) if(on && ender) {
          lastrow[j] = acc;
          if(j == 0 || acc < best) { best = acc; end = j; }           // strictly smaller: the smallest column of least acc
        }
        const unsigned long long b0 = __ballot(on && (move & 1)), b1 = __ballot(on && (move & 2));
        if((t & (WAVE - 1)) == lane) { w0 = b0; w1 = b1; }
        if(((t & (WAVE - 1)) == WAVE - 1 || t == nsteps - 1) && lane <= (t & (WAVE - 1)))
          mvs[(t & ~(WAVE - 1)) + lane] = make_uint4((unsigned)w0, (unsigned)(w0 >> 32), (unsigned)w1, (unsigned)(w1 >> 32));
        if(on && lane == WAVE - 1 && s + 1 < nstrips) hand[j] = acc;  // for lane 0 of the next strip
      }
      cur = nxt;
    }
    __threadfence();                                                  // the hand-over row and the masks, before other lanes read them
  }
  const int last = (na - 1) & (WAVE - 1);
  if constexpr(OPEN) {
    if(lane == last) out[cost0 + blockIdx.x] = best;
    end = __builtin_amdgcn_readlane(end, last);                       // (to every lane, as a scalar: the walk below is one)
  } else if(lane == last) out[cost0 + blockIdx.x] = v;                // acc[na-1][nb-1]: the last cell of the last row's range

  // D3 / B4: back along the moves; Q5: from (na - 1, end) until row 0 is reached
  float* pos = out + (size_t)p.pos0;
  int i = na - 1, j = OPEN ? end : nb - 1, hi = j;
  int cur_s = -1, cur_b = -1, wlo = 0;
  uint4 w = make_uint4(0, 0, 0, 0);
  for(int guard = na + nb; guard > 0; guard --) {
    if(OPEN ? i == 0 : i == 0 && j == 0) break;
    const int s = i >> 6, l = i & (WAVE - 1);
    if constexpr(BAND) if(s != cur_s) wlo = max(align_center<GEO>(center, p, s * WAVE) - band, 0);
    const int t = j - wlo + l, blk = t & ~(WAVE - 1);
    if(BAND && (t < 0 || t >= per_strip)) break;                      // (a cell outside the band: no stored move leads there)
    if(s != cur_s || blk != cur_b) {
      w = make_uint4(0, 0, 0, 0);
      if((long long)blk + lane < per_strip) w = mv[(long long)s * per_strip + blk + lane];
      cur_s = s; cur_b = blk;
    }
    const int k = t & (WAVE - 1);
    const unsigned m0 = (unsigned)__builtin_amdgcn_readlane((int)(l < 32 ? w.x : w.y), k);
    const unsigned m1 = (unsigned)__builtin_amdgcn_readlane((int)(l < 32 ? w.z : w.w), k);
    const int move = (int)((m0 >> (l & 31)) & 1u) | (int)(((m1 >> (l & 31)) & 1u) << 1);
    if((move != 2 && i == 0) || (move != 1 && j == 0)) break;         // (likewise: it would leave the matrix)
    if(move == 2) j --;
    else {
      if(lane == 0) pos[i] = __fmul_rn((float)(j + hi), 0.5f);        // lo = j: the walk leaves row i here
      i --;
      if(move == 0) j --;
      hi = j;
    }
  }
  if(lane == 0) pos[0] = __fmul_rn((float)((OPEN ? j : 0) + hi), 0.5f);
  if constexpr(OPEN) if(lane == 0) { span[2 * blockIdx.x] = j; span[2 * blockIdx.x + 1] = end; }
}

// ---------------------------------------------------------------- L3 - L4 / K3 - K4: the path under the slope pattern
// k_align_slope_dtw_t<BAND>: <false> over whole-matrix planes (rules L1 - L4), <true> over band planes (rules K1 - K4).  The
// layout of k_align_dtw_t: lane l on row i = 64 s + l, on column j = wlo + t - l at step t of the strip's window [wlo, whi],
// which holds the range [lo_i, hi_i] of every row of the strip.  What a lane holds when it reaches (i, j):
//   diag   acc[i-1][j-1], the `up` it received one step ago: move 0
//   qi     (acc[i-2][j-1] + D[i-1][j]) + step_cost, which the lane above formed one step ago on (i - 1, j): move 1.  It comes
//          with a second wavefront shift (DPP); lane 0 takes it from the second hand-over row
//   qo     (acc[i-1][j-2] + D[i][j-1]) + step_cost, which the lane formed itself one step ago on (i, j - 1): move 2
// and one sum serves the last two: through (i, j) from (i - 1, j - 1) the path goes on to (i, j + 1) by move 2 or to
// (i + 1, j) by move 1, and either candidate is (diag + D[i][j]) + step_cost.  A lane forms it on every cell it passes,
// inside its row's range or not, because the cell between the two ends of an allowed move need not lie in the region.
// Whether a candidate exists is decided where it is used, by integer comparisons of j with three ranges a lane sets up once
// per strip ([a0, b0] for move 0, [a1, b1] for move 1, j - 1 in [c0, b0] for move 2), never by the values: so what a lane
// outside its range, an earlier strip or unwritten memory left in a register or in the hand-over rows is never used.  The
// moves of a step are two ballots, stored as k_align_dtw_t stores them.
// Hand-over: lane 63 leaves acc[i][j] in the first row and that sum in the second, both indexed by the column, for lane 0 of
// the next strip.  The sum is needed one column past whi, where a move 1 into row i + 1 at column j passes (i, j) with
// j <= whi + 1 (its other end (i - 1, j - 1) is in the region), so a strip that has a successor takes one step more.  Lane 0
// starts a strip on column wlo with diag = acc[i-1][wlo-1] and, for a move 2 from (i - 1, wlo - 2), qo = (acc[i-1][wlo-2] +
// D[i][wlo-1]) + step_cost, both from the first row before the loop; it meets no cell of the region left of wlo.
// Reads stay 63 steps ahead of the writes, whatever the window.  Every lane of a strip counts its steps from the strip's own
// wlo.  Lane 0 is on column x at step x - wlo and loads entry x of either row then at the latest (DTW_U to 2 DTW_U - 1 steps
// earlier in fact, and entries wlo - 1 and wlo - 2 before the first step); lane 63 is on column x at step x - wlo + 63 and
// stores entry x then.  So whatever whi - wlo is -- 0 under band 0, where lane 0 has left the window before lane 63 stores
// anything, or 140 and more under band 70, where lane 0 is still reading column wlo + 100 while lane 63 stores column wlo +
// 37 -- entry x is read at least 63 steps before it is overwritten, and one wavefront runs its steps in program order.
// Loads of columns past nb - 1 are clamped to nb - 1; they may see the new value, and are not used.
// The walk back reads the masks as k_align_dtw_t does, finding a strip's wlo again as the forward pass found it.  Every move
// leaves its row, so pos[i] follows from the cell and the move: columns j - 1 and j under move 2, else j alone; move 1 passes
// (i - 1, j) and nothing else of row i - 1.  Each move lowers i and j by one at the least: at most min(na, nb) - 1 moves.
// What BAND (either band geometry) changes, each under `if constexpr`:
//   rows     <false> rule L1 from align_slope_row for rows i, i - 1 and i - 2; the ranges of rows i - 1 and i - 2 moved one
//            column right are [a0, b0] and [a1, b1], and c0 is a0.  <true> the region's rows (rule K1) from the host's table,
//            one {lo, hi} per row, an empty row lo > hi, loaded for the same three rows once per strip, and the band's rows
//            p ... q from align_center (the diagonal or the line); K3's comparisons fold into the three ranges: move 0 needs j - 1 in row i - 1 of
//            the region; move 1 needs j - 1 in row i - 2 of the region and j in row i - 1 of the band; move 2 needs j - 2 in
//            row i - 1 of the region and j - 1 >= p_i (j - 1 <= q_i follows from j being in the region).  On a cell outside
//            the band the sum above holds +infinity or a clamped read, and no candidate uses it: those comparisons ask for
//            the passed cell to be in the band.
//   window   <false> [lo of the strip's first row, hi of its last]: lo and hi do not decrease with i, two __shfl.  <true> the
//            least lo and the largest hi of the strip's non-empty rows (band_slope_window, a wavefront reduction), and no
//            steps if every row is empty.  Over the non-empty rows of a connected band lo and hi do not decrease and no two
//            consecutive rows are empty (rule K1, measured), so a strip has a non-empty row.
//   D        <false> entry j of a row of nb, all known when compiling.  <true> entry j - (c_i - band) of a row of 2 band + 1,
//            clamped to the row.
// <false> does not read `region`.
struct SlopeBlock { float d[DTW_U], p[DTW_U], q[DTW_U]; };
// as dtw_load<false>, with the second hand-over row beside the first; D is entry q = column - off of a row of `width` (full:
// off is 0 and not subtracted -- with `- off` in the text the compiler orders the 16 add / max pairs of the D index otherwise)
template <bool BAND>
DEV void slope_load(SlopeBlock& b, const float* __restrict__ drow, const float* hand, const float* handq, int j0, int lane,
  int off, int width, int nb) {
#pragma unroll
  for(int k = 0; k < DTW_U; k ++) {
    const int x = min(max(j0 + lane + k, 0), nb - 1);
    b.d[k] = drow[min(max(BAND ? j0 + k - off : j0 + k, 0), width - 1)];
    b.p[k] = hand[x]; b.q[k] = handq[x];
  }
}

// [wlo, whi] of a strip from the range of each lane's row ((1, 0): empty or no row); whi < wlo if every row is empty
DEV void band_slope_window(int lo, int hi, int nb, int& wlo, int& whi) {
  wlo = lo <= hi ? lo : nb - 1; whi = lo <= hi ? hi : 0;
#pragma unroll
  for(int o = WAVE / 2; o > 0; o >>= 1) { wlo = min(wlo, __shfl_xor(wlo, o)); whi = max(whi, __shfl_xor(whi, o)); }
}

template <int GEO, class... SUB>
__global__ __launch_bounds__(WAVE) void k_align_slope_dtw_t(AlignDev d, const float* __restrict__ plane,
  const int2* __restrict__ region, uint4* __restrict__ moves, float* hand_rows, float* __restrict__ out, int cost0,
  const int* __restrict__ center, SUB... sub) {
  constexpr bool BAND = GEO != ALIGN_GEO_FULL, OPEN = sizeof...(SUB) != 0;
  float* const last_rows = sub_last_rows(sub...); int* const span = sub_span(sub...);
  static_assert(! OPEN || ! BAND, "the free ends are instantiated for the full geometry only");
  const int lane = threadIdx.x;
  const AlignPair p = d.pairs[blockIdx.x];
  const int na = p.na, nb = p.nb, band = p.band, width = BAND ? 2 * band + 1 : nb;
  const float* D = plane + (size_t)p.cell0;
  const int2* tab = BAND ? region + p.pad : nullptr;
  float* hand = hand_rows + (size_t)p.row0;
  float* handq = hand + nb;
  uint4* mv = moves + p.mv0;
  const long long per_strip = p.steps;
  const float step = d.step_cost;
  const int nstrips = (na + WAVE - 1) / WAVE;
  float v = 0.0f;                                                     // acc of this lane's last cell
  // OPEN (rule Q4), as in align_dtw; the row of the matching function is +infinity left of the last row's range
  float* lastrow = OPEN ? last_rows + (size_t)p.pad : nullptr;
  float best = 0.0f; int end = 0;
  if constexpr(OPEN) {
    int l, h;
    align_sub_row((long long)na - 1, nb, l, h);
    for(int j = lane; j < min(l, nb); j += WAVE) lastrow[j] = __builtin_huge_valf();
  }
  for(int s = 0; s < nstrips; s ++) {
    const int i = s * WAVE + lane, rows = min(WAVE, na - s * WAVE);
    const bool more = s + 1 < nstrips;
    const bool ender = OPEN && lane == ((na - 1) & (WAVE - 1)) && ! more;
    // the range of this lane's row of the region, and the columns j for which move 0, 1 and 2 have a candidate: [a0, b0],
    // [a1, b1], and j - 1 in [c0, b0]; empty ranges (1, 0) where there is no such row
    int off = 0, lo = 1, hi = 0, a0 = 1, b0 = 0, a1 = 1, b1 = 0, c0 = 1;
    if constexpr(BAND) {
      if(i < na) {
        const int2 r = tab[i];
        const int c = align_center<GEO>(center, p, i);
        lo = r.x; hi = r.y; off = c - band;
        if(i >= 1) {
          const int2 r1 = tab[i - 1];
          a0 = r1.x + 1; b0 = r1.y + 1; c0 = max(a0, max(off, 0));
        }
        if(i >= 2) {
          const int2 r2 = tab[i - 2];
          const int cp = align_center<GEO>(center, p, i - 1);
          a1 = max(r2.x + 1, max(cp - band, 0)); b1 = min(r2.y + 1, min(cp + band, nb - 1));
        }
      }
    } else if constexpr(OPEN) {                                       // Q1: the cells reached from row 0, no upper cut
      if(i < na) {
        align_sub_row(i, nb, lo, hi);
        if(i >= 1) { align_sub_row(i - 1, nb, a0, b0); a0 ++; b0 ++; }
        if(i >= 2) { align_sub_row(i - 2, nb, a1, b1); a1 ++; b1 ++; }
      }
      c0 = a0;
    } else {
      if(i < na) {
        align_slope_row(i, na, nb, lo, hi);
        if(i >= 1) { align_slope_row(i - 1, na, nb, a0, b0); a0 ++; b0 ++; }
        if(i >= 2) { align_slope_row(i - 2, na, nb, a1, b1); a1 ++; b1 ++; }
      }
      c0 = a0;
    }
    int wlo, whi, nsteps;
    if constexpr(BAND) {
      band_slope_window(lo, hi, nb, wlo, whi);
      nsteps = whi >= wlo ? whi - wlo + rows + (more ? 1 : 0) : 0;
    } else {
      wlo = __shfl(lo, 0); whi = __shfl(hi, rows - 1);
      nsteps = whi - wlo + rows + (more ? 1 : 0);
    }
    const float* drow = D + (size_t)min(i, na - 1) * width;
    uint4* mvs = mv + (long long)s * per_strip;
    // lane 0's first cell (in strip 0 nothing of it is used)
    float diag = hand[max(wlo - 1, 0)];
    float qo = __fadd_rn(__fadd_rn(hand[max(wlo - 2, 0)], drow[BAND ? min(max(wlo - 1 - off, 0), width - 1) : max(wlo - 1, 0)]), step);
    unsigned long long w0 = 0, w1 = 0;                                // the masks of step (t & ~63) + lane
    SlopeBlock cur, nxt;
    slope_load<BAND>(cur, drow, hand, handq, wlo - lane, lane, off, width, nb);
    for(int t0 = 0; t0 < nsteps; t0 += DTW_U) {
      slope_load<BAND>(nxt, drow, hand, handq, wlo + t0 + DTW_U - lane, lane, off, width, nb);
#pragma unroll
      for(int k = 0; k < DTW_U; k ++) {
        const int t = t0 + k;
        if(t >= nsteps) break;
        const int j = wlo + t - lane;
        const bool on = j >= lo && j <= hi;
        const bool has0 = j >= a0 && j <= b0, has1 = j >= a1 && j <= b1, has2 = j - 1 >= c0 && j - 1 <= b0;
        const float up_raw = wave_shr1(cur.p[k], v);                  // acc[i-1][j]
        const float qi = wave_shr1(cur.q[k], qo);
        float m = diag; int move = 0;                                 // L3 / K3: the first candidate that exists ...
        if(! has0) { m = qi; move = 1; }
        if(! has0 && ! has1) { m = qo; move = 2; }
        if(has0 && has1 && qi < m) { m = qi; move = 1; }              // ... and a later one only if strictly smaller
        if((has0 || has1) && has2 && qo < m) { m = qo; move = 2; }
        float acc = __fadd_rn(m, cur.d[k]);
        if(OPEN ? i == 0 : i == 0 && j == 0) { acc = cur.d[k]; move = 0; }   // Q3: a path starts anywhere on row 0, at no cost
        qo = __fadd_rn(__fadd_rn(diag, cur.d[k]), step);              // through (i, j) from (i - 1, j - 1)
        diag = up_raw;
        if(on) v = acc;
        if constexpr(OPEN) if(on && ender) {
          lastrow[j] = acc;
          if(j == lo || acc < best) { best = acc; end = j; }          // strictly smaller: the smallest column of least acc
        }
        const unsigned long long m0 = __ballot(on && (move & 1)), m1 = __ballot(on && (move & 2));
        if((t & (WAVE - 1)) == lane) { w0 = m0; w1 = m1; }
        if(((t & (WAVE - 1)) == WAVE - 1 || t == nsteps - 1) && lane <= (t & (WAVE - 1)))
          mvs[(t & ~(WAVE - 1)) + lane] = make_uint4((unsigned)w0, (unsigned)(w0 >> 32), (unsigned)w1, (unsigned)(w1 >> 32));
        if(lane == WAVE - 1 && more && j >= 0 && j < nb) {            // for lane 0 of the next strip
          handq[j] = qo;
          if(on) hand[j] = acc;
        }
      }
      cur = nxt;
    }
    __threadfence();                                                  // the hand-over rows and the masks, before other lanes read them
  }
  const int last = (na - 1) & (WAVE - 1);
  if constexpr(OPEN) {
    if(lane == last) out[cost0 + blockIdx.x] = best;
    end = __builtin_amdgcn_readlane(end, last);                       // (to every lane, as a scalar: the walk below is one)
  } else if(lane == last) out[cost0 + blockIdx.x] = v;                // acc[na-1][nb-1]: the last cell of the last row's range

  // L4 / K4: back along the moves; Q5: from (na - 1, end) until row 0 is reached, every move leaves its row
  float* pos = out + (size_t)p.pos0;
  int i = na - 1, j = OPEN ? end : nb - 1;
  int cur_s = -1, cur_b = -1, wlo = 0;
  uint4 w = make_uint4(0, 0, 0, 0);
  for(int guard = OPEN ? na : min(na, nb); guard > 0; guard --) {
    if(OPEN ? i == 0 : i == 0 && j == 0) break;
    const int s = i >> 6, l = i & (WAVE - 1);
    if(s != cur_s) {
      if constexpr(BAND) {
        const int2 r = tab[min(s * WAVE + lane, na - 1)];
        int whi;
        band_slope_window(s * WAVE + lane < na ? r.x : 1, s * WAVE + lane < na ? r.y : 0, nb, wlo, whi);
      } else if constexpr(OPEN) { int h; align_sub_row((long long)s * WAVE, nb, wlo, h); }
      else { int h; align_slope_row((long long)s * WAVE, na, nb, wlo, h); }
    }
    const int t = j - wlo + l, blk = t & ~(WAVE - 1);
    if(t < 0 || t >= per_strip) break;                                // (a cell outside the region: no stored move leads there)
    if(s != cur_s || blk != cur_b) {
      w = make_uint4(0, 0, 0, 0);
      if((long long)blk + lane < per_strip) w = mv[(long long)s * per_strip + blk + lane];
      cur_s = s; cur_b = blk;
    }
    const int k = t & (WAVE - 1);
    const unsigned m0 = (unsigned)__builtin_amdgcn_readlane((int)(l < 32 ? w.x : w.y), k);
    const unsigned m1 = (unsigned)__builtin_amdgcn_readlane((int)(l < 32 ? w.z : w.w), k);
    const int move = (int)((m0 >> (l & 31)) & 1u) | (int)(((m1 >> (l & 31)) & 1u) << 1);
    if(i < 1 || j < 1 || move == 3 || (move == 1 && i < 2) || (move == 2 && j < 2)) break;   // (likewise: it would leave the matrix)
    if(lane == 0) pos[i] = __fmul_rn((float)(2 * j - (move == 2)), 0.5f);
    if(move == 1) {
      if(lane == 0) pos[i - 1] = __fmul_rn((float)(2 * j), 0.5f);     // (i - 1, j) on the way to (i - 2, j - 1)
      i -= 2; j --;
    } else if(move == 2) { i --; j -= 2; }
    else { i --; j --; }
  }
  if constexpr(OPEN) {                                                // row 0 is (0, begin) alone
    if(lane == 0) { pos[0] = __fmul_rn((float)(2 * j), 0.5f); span[2 * blockIdx.x] = j; span[2 * blockIdx.x + 1] = end; }
  } else if(lane == 0) pos[0] = 0.0f;                                 // row 0 is (0, 0) alone
}

// ---------------------------------------------------------------- P1: the pooled vectors of a coarse pass
// k_pool_code: the mean of every `factor` consecutive rows of LLSM_GPU_CODE, per utterance (rule P1: llsm_gpu.h, DESIGN.md
// section 34).  One thread per (coarse frame, column) of the output, numbered as the output is laid out, so adjacent lanes
// read adjacent columns of the same rows -- every load of a row of CODE is coalesced, as is the store -- and a thread walks
// its at most 64 rows in ascending order, one addition per row and one correctly rounded division: the order is the rule,
// there is no cross-lane sum, no LDS and no atomic.  The rows are loaded eight at a time ahead of their additions: with one
// load in flight per thread the kernel waited on latency (2.4 TB/s on 1 024 utterances of 1 154 frames at factor 16, 3.9
// with eight: DESIGN.md section 34).  tab[u] = (first source frame, frames n, first coarse frame of the
// output, side) of pooled utterance u, ascending in the third member, which starts at 0; a thread finds its utterance by
// bisection over that member (the table of a call is a few KiB and stays in the caches).  side: 0 reads code_a, 1 code_b,
// so one launch pools both batches of llsm_gpu_batch_align_pyramid.  The kernel reads CODE once and writes 1 / factor of it.
#define POOL_NT 256
#define POOL_U 8                                   // rows loaded ahead of their additions
__global__ __launch_bounds__(POOL_NT) void k_pool_code(const float* __restrict__ code_a, const float* __restrict__ code_b,
  const int4* __restrict__ tab, int n_tab, int dim, int factor, long long total, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * POOL_NT + threadIdx.x;
  if(e >= total) return;
  const long long kg = e / dim;                                       // the coarse frame of the whole output
  const int c = (int)(e - kg * dim);
  int lo = 0, hi = n_tab - 1;                                         // the last utterance that starts at or before kg
  while(lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if(tab[mid].z <= kg) lo = mid; else hi = mid - 1;
  }
  const int4 u = tab[lo];
  const int j0 = (int)(kg - u.z) * factor, m = min(factor, u.y - j0);  // (m >= 1: the table holds ceil(n / factor) frames)
  const float* src = (u.w ? code_b : code_a) + ((size_t)u.x + j0) * dim + c;
  float s = 0.0f;
  int j = 0;
  for(; j + POOL_U <= m; j += POOL_U) {                               // POOL_U loads in flight, then their additions in order
    float v[POOL_U];
#pragma unroll
    for(int k = 0; k < POOL_U; k ++) v[k] = src[(size_t)(j + k) * dim];
#pragma unroll
    for(int k = 0; k < POOL_U; k ++) s = __fadd_rn(s, v[k]);
  }
  for(; j < m; j ++) s = __fadd_rn(s, src[(size_t)j * dim]);
  out[e] = __fdiv_rn(s, (float)m);
}

// ---------------------------------------------------------------- launchers
int launch_align_dist(LaunchCtx* P, AlignGeo geo, const AlignDev& d, const int4* tiles, int n_tiles, float* plane, const int* center) {
  if(n_tiles == 0) return 0;
  if(geo == ALIGN_GEO_LINE) LAUNCH("k_align_line_dist", k_align_dist_t<ALIGN_GEO_LINE>, dim3(n_tiles), dim3(AD_NT), 0, d, tiles, plane, center);
  else if(geo == ALIGN_GEO_BAND) LAUNCH("k_align_band_dist", k_align_dist_t<ALIGN_GEO_BAND>, dim3(n_tiles), dim3(AD_NT), 0, d, tiles, plane, center);
  else LAUNCH("k_align_dist", k_align_dist_t<ALIGN_GEO_FULL>, dim3(n_tiles), dim3(AD_NT), 0, d, tiles, plane, center);
  return 0;
}

int launch_align_dtw(LaunchCtx* P, AlignGeo geo, const AlignDev& d, const float* plane, uint4* moves, float* row, float* out, int cost0,
  const int* center) {
  if(d.n_pairs == 0) return 0;
  if(geo == ALIGN_GEO_LINE) LAUNCH("k_align_line_dtw", k_align_dtw_t<ALIGN_GEO_LINE>, dim3(d.n_pairs), dim3(WAVE), 0, d, plane, moves, row, out, cost0, center);
  else if(geo == ALIGN_GEO_BAND) LAUNCH("k_align_band_dtw", k_align_dtw_t<ALIGN_GEO_BAND>, dim3(d.n_pairs), dim3(WAVE), 0, d, plane, moves, row, out, cost0, center);
  else LAUNCH("k_align_dtw", k_align_dtw_t<ALIGN_GEO_FULL>, dim3(d.n_pairs), dim3(WAVE), 0, d, plane, moves, row, out, cost0, center);
  return 0;
}

int launch_align_slope_dtw(LaunchCtx* P, AlignGeo geo, const AlignDev& d, const float* plane, const int2* region, uint4* moves,
  float* row, float* out, int cost0, const int* center) {
  if(d.n_pairs == 0) return 0;
  if(geo == ALIGN_GEO_LINE) LAUNCH("k_align_line_slope_dtw", k_align_slope_dtw_t<ALIGN_GEO_LINE>, dim3(d.n_pairs), dim3(WAVE), 0, d, plane, region, moves, row, out, cost0, center);
  else if(geo == ALIGN_GEO_BAND) LAUNCH("k_align_band_slope_dtw", k_align_slope_dtw_t<ALIGN_GEO_BAND>, dim3(d.n_pairs), dim3(WAVE), 0, d, plane, region, moves, row, out, cost0, center);
  else LAUNCH("k_align_slope_dtw", k_align_slope_dtw_t<ALIGN_GEO_FULL>, dim3(d.n_pairs), dim3(WAVE), 0, d, plane, region, moves, row, out, cost0, center);
  return 0;
}

int launch_align_sub_dtw(LaunchCtx* P, bool slope, const AlignDev& d, const float* plane, uint4* moves, float* row, float* out, int cost0,
  float* last_rows, int* span) {
  if(d.n_pairs == 0) return 0;
  const int* none = nullptr; const int2* no_region = nullptr;      // (the full geometry reads neither a line nor a table of rows)
  if(slope) LAUNCH("k_align_sub_slope_dtw", (k_align_slope_dtw_t<ALIGN_GEO_FULL, float*, int*>), dim3(d.n_pairs), dim3(WAVE), 0, d, plane, no_region, moves, row, out, cost0, none, last_rows, span);
  else LAUNCH("k_align_sub_dtw", (k_align_dtw_t<ALIGN_GEO_FULL, float*, int*>), dim3(d.n_pairs), dim3(WAVE), 0, d, plane, moves, row, out, cost0, none, last_rows, span);
  return 0;
}

int launch_pool_code(LaunchCtx* P, const float* code_a, const float* code_b, const int4* tab, int n_tab, int dim, int factor,
  long long coarse_frames, float* out) {
  const long long total = coarse_frames * dim;
  if(total == 0) return 0;
  LAUNCH("k_pool_code", k_pool_code, dim3((unsigned)((total + POOL_NT - 1) / POOL_NT)), dim3(POOL_NT), 0, code_a, code_b, tab, n_tab,
    dim, factor, total, out);
  return 0;
}
