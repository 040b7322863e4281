// align_kernels.hip -- alignment of utterance pairs, llsm_gpu_batch_align (rules D1 - D3: llsm_gpu.h, DESIGN.md section 23;
// host side: align.cpp).  Two kernels:
//
//   k_align_dist   D1: the distance planes of all pairs in one launch.  A workgroup of 256 threads takes a tile of
//                  64 x 64 cells of one pair from the host's tile table; wavefront w owns rows 16 w ... 16 w + 15 of the
//                  tile and lane l column l, so a thread keeps 16 cells of one column in registers.  The two row blocks
//                  of LLSM_GPU_CODE go through the LDS 32 columns at a time, each element staged once per tile.  Every
//                  thread walks k ascending for each cell it owns: D1's order is per cell, there is no cross-lane
//                  reduction, and the bits follow from the rule.
//   k_align_dtw    D2 - D3: one wavefront per pair.  Lane l owns row 64 s + l of strip s and walks the anti-diagonals
//                  of the strip: at step t it is on column t - l.
// and their two counterparts for llsm_gpu_batch_align_band (rules B1 - B4), which keep to a band
// around the diagonal: k_align_band_dist (the tiles that meet the band, stored in the band's own layout) and
// k_align_band_dtw (each strip walks the column window of its rows only); both are described where they stand.
//
// LDS of k_align_dist.  The A block is [64][32 + 4] floats: a wavefront reads A[row][k ... k + 3] with every lane on the
// same address (a broadcast, one 16-byte read per row and four k), so the padding only keeps the rows 16-byte aligned.
// The B block is stored transposed, [32][64 + 1]: lane l reads Bt[k][l] -- consecutive words, no conflict -- and the
// staging pass, whose lanes run along k for the sake of coalesced global reads, writes Bt[k][row] at a stride of 65 words:
// an odd stride walks all 32 banks of a write, where the unpadded 64 would put the 32 lanes of a half-wavefront on one
// bank (the stride argument of the tile kernel of the coder).
//
// k_align_dtw, the forward pass.  acc[i-1][j] is what lane l - 1 computed one step ago and acc[i-1][j-1] what it computed
// two steps ago, i.e. what this lane received as `up` one step ago: one cross-lane move per step, a wavefront shift by one
// lane on the vector ALU (DPP), no LDS round trip.  Lane 0 takes both from the row the strip above left behind (its lane
// 63 stores acc[64 s + 63][j] into a per-pair row of nb floats; the reads of strip s + 1 run ahead of its own writes to
// the same row by at least 47 columns, so one row serves).  The D values and that row are loaded DTW_U steps ahead, so
// the dependent chain of a step is the shift, two additions, two compare / selects and the addition of D.  The moves of a
// step, 2 bits per lane, are two ballots: lane t % 64 keeps the pair of 64-bit masks of step t and the wavefront stores
// 64 steps (1 KiB) at a time.
// The backtrack is a scalar walk: a move 0 goes two steps back, a move 1 or 2 one step back, so the walk reads the masks
// in descending order; the wavefront loads 64 steps at a time (lane k: step base + k) and reads them with v_readlane.  It
// notes lo / hi of each row and writes pos when it leaves the row.  On the borders the moves are forced again, whatever
// the masks hold, so the walk ends at (0, 0) after at most na + nb - 2 moves.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "kernels.h"
#include "dev_common.h"
#include "launch.h"

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

__global__ __launch_bounds__(AD_NT) void k_align_dist(AlignDev d, const int4* __restrict__ tiles, float* __restrict__ plane) {
  __shared__ __attribute__((aligned(16))) float sa[ALIGN_TILE * AD_AS];
  __shared__ float sb[AD_KC * AD_BS];
  __shared__ int va[ALIGN_TILE], vb[ALIGN_TILE];
  const int4 tl = tiles[blockIdx.x];
  const AlignPair p = d.pairs[tl.x];
  const int i0 = tl.y, j0 = tl.z;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), r0 = (tid >> 6) * AD_R;
  // rows beyond the pair's last are read as its last row and never written
  const float* A = d.code_a + (size_t)p.a0 * d.dim;
  const float* B = d.code_b + (size_t)p.b0 * d.dim;
  if(tid < ALIGN_TILE) va[tid] = A[(size_t)min(i0 + tid, p.na - 1) * d.dim] > 0.5f;
  else if(tid < 2 * ALIGN_TILE) vb[tid - ALIGN_TILE] = B[(size_t)min(j0 + tid - ALIGN_TILE, p.nb - 1) * d.dim] > 0.5f;
  float acc[AD_R];
  align_tile_sums<false>(A, B, d.dim, d.first, d.count, p.na, p.nb, i0, j0, sa, sb, acc);   // (va / vb are written)
  const int j = j0 + lane;
  if(j >= p.nb) return;
  const int vj = vb[lane];
  float* out = plane + (size_t)p.cell0 + j;
#pragma unroll
  for(int r = 0; r < AD_R; r ++) {
    const int i = i0 + r0 + r;
    if(i < p.na) out[(size_t)i * p.nb] = va[r0 + r] != vj ? __fadd_rn(acc[r], d.voicing_cost) : acc[r];
  }
}

// B2: rule D1 for the cells inside the band, in the band layout.  The tile is one of the matrix (its first column may be
// negative or its columns run past nb - 1 where the band of a row hangs over the matrix); lane l is on column j0 + l, so a
// wavefront's stores to a row of the band plane are consecutive words.  Entry q of row i is column off_i + q, off_i =
// c_i - band: every entry of a tile's rows whose column lies in the tile is written, +infinity outside the matrix.
__global__ __launch_bounds__(AD_NT) void k_align_band_dist(AlignBandDev d, const int4* __restrict__ tiles, float* __restrict__ plane) {
  __shared__ __attribute__((aligned(16))) float sa[ALIGN_TILE * AD_AS];
  __shared__ float sb[AD_KC * AD_BS];
  __shared__ int va[ALIGN_TILE], vb[ALIGN_TILE], off[ALIGN_TILE];
  const int4 tl = tiles[blockIdx.x];
  const AlignBandPair p = d.pairs[tl.x];
  const int i0 = tl.y, j0 = tl.z;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), r0 = (tid >> 6) * AD_R;
  const float* A = d.code_a + (size_t)p.a0 * d.dim;
  const float* B = d.code_b + (size_t)p.b0 * d.dim;
  if(tid < ALIGN_TILE) {
    const int i = min(i0 + tid, p.na - 1);
    va[tid] = A[(size_t)i * d.dim] > 0.5f;
    off[tid] = align_band_center(i, p.na, p.nb) - p.band;
  } else if(tid < 2 * ALIGN_TILE) vb[tid - ALIGN_TILE] = B[(size_t)max(min(j0 + tid - ALIGN_TILE, p.nb - 1), 0) * d.dim] > 0.5f;
  float acc[AD_R];
  align_tile_sums<true>(A, B, d.dim, d.first, d.count, p.na, p.nb, i0, j0, sa, sb, acc);     // (va / vb / off are written)
  const int j = j0 + lane, width = 2 * p.band + 1;
  const bool inside = j >= 0 && j < p.nb;
  const int vj = vb[lane];
  float* out = plane + (size_t)p.cell0;
#pragma unroll
  for(int r = 0; r < AD_R; r ++) {
    const int i = i0 + r0 + r, q = j - off[r0 + r];
    if(i < p.na && q >= 0 && q < width)
      out[(size_t)i * width + q] = ! inside ? __builtin_huge_valf() : va[r0 + r] != vj ? __fadd_rn(acc[r], d.voicing_cost) : acc[r];
  }
}

// ---------------------------------------------------------------- D2 - D3: the path
#define DTW_U 8                                    // steps loaded ahead
// lane l reads lane l - 1 (a wavefront shift right by one on the vector ALU); lane 0 keeps `first`
#define DPP_WAVE_SHR1 0x138
DEV float wave_shr1(float first, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, first), __builtin_bit_cast(int, v),
    DPP_WAVE_SHR1, 0xF, 0xF, false));
}

struct DtwBlock { float d[DTW_U], p[DTW_U]; };
// D[i][t - lane] and, for lane 0 of a strip below the first, the hand-over row at t, for steps [t0, t0 + DTW_U); columns
// outside the row are read at its ends and not used
DEV void dtw_load(DtwBlock& b, const float* __restrict__ drow, const float* hand, int t0, int lane, int nb) {
#pragma unroll
  for(int k = 0; k < DTW_U; k ++) {
    b.d[k] = drow[min(max(t0 + k - lane, 0), nb - 1)];
    b.p[k] = hand[min(t0 + k, nb - 1)];
  }
}

__global__ __launch_bounds__(WAVE) void k_align_dtw(AlignDev d, const float* __restrict__ plane, uint4* __restrict__ moves,
  float* __restrict__ hand_rows, float* __restrict__ out, int cost0) {
  const int lane = threadIdx.x;
  const AlignPair p = d.pairs[blockIdx.x];
  const int na = p.na, nb = p.nb;
  const float* D = plane + (size_t)p.cell0;
  float* hand = hand_rows + (size_t)p.row0;
  uint4* mv = moves + p.mv0;
  const long long per_strip = ALIGN_STEPS(nb);
  const float step = d.step_cost;
  const int nstrips = (na + WAVE - 1) / WAVE;
  float v = 0.0f;                                                     // acc of this lane's last cell
  for(int s = 0; s < nstrips; s ++) {
    const int i = s * WAVE + lane, rows = min(WAVE, na - s * WAVE), nsteps = nb + rows - 1;
    const bool row_on = i < na;
    const float* drow = D + (size_t)min(i, na - 1) * nb;
    uint4* mvs = mv + (long long)s * per_strip;
    float diag = 0.0f;                                                // what `up` was one step ago
    unsigned long long w0 = 0, w1 = 0;                                // the masks of step (t & ~63) + lane
    DtwBlock cur, nxt;
    dtw_load(cur, drow, hand, 0, lane, nb);
    for(int t0 = 0; t0 < nsteps; t0 += DTW_U) {
      dtw_load(nxt, drow, hand, t0 + DTW_U, lane, nb);
#pragma unroll
      for(int k = 0; k < DTW_U; k ++) {
        const int t = t0 + k;
        if(t >= nsteps) break;
        const int j = t - lane;
        const bool on = row_on && j >= 0 && j < nb;
        const float up_raw = wave_shr1(cur.p[k], v);                  // acc[i-1][j]
        const float up = __fadd_rn(up_raw, step), lf = __fadd_rn(v, step);
        float m = diag; int move = 0;
        if(up < m) { m = up; move = 1; }
        if(lf < m) { m = lf; move = 2; }
        if(i == 0) { m = lf; move = 2; }                              // the borders are forced, not compared
        if(j == 0) { m = up; move = 1; }
        float acc = __fadd_rn(m, cur.d[k]);
        if(i == 0 && j == 0) { acc = cur.d[k]; move = 0; }
        diag = up_raw;
        if(on) v = acc;
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
  if(lane == last) out[cost0 + blockIdx.x] = v;                       // acc[na-1][nb-1]

  // D3: back along the moves
  float* pos = out + (size_t)p.pos0;
  int i = na - 1, j = nb - 1, hi = j;
  int cur_s = -1, cur_b = -1;
  uint4 w = make_uint4(0, 0, 0, 0);
  for(int guard = na + nb; guard > 0; guard --) {
    if(i == 0 && j == 0) break;
    const int s = i >> 6, l = i & (WAVE - 1), t = j + l, blk = t & ~(WAVE - 1);
    if(s != cur_s || blk != cur_b) {
      w = make_uint4(0, 0, 0, 0);
      if((long long)blk + lane < per_strip) w = mv[(long long)s * per_strip + blk + lane];
      cur_s = s; cur_b = blk;
    }
    const int k = t & (WAVE - 1);
    const unsigned m0 = (unsigned)__builtin_amdgcn_readlane((int)(l < 32 ? w.x : w.y), k);
    const unsigned m1 = (unsigned)__builtin_amdgcn_readlane((int)(l < 32 ? w.z : w.w), k);
    int move = (int)((m0 >> (l & 31)) & 1u) | (int)(((m1 >> (l & 31)) & 1u) << 1);
    if(i == 0) move = 2;
    else if(j == 0) move = 1;
    if(move == 2) j --;
    else {
      if(lane == 0) pos[i] = __fmul_rn((float)(j + hi), 0.5f);        // lo = j: the walk leaves row i here
      i --;
      if(move == 0) j --;
      hi = j;
    }
  }
  if(lane == 0) pos[0] = __fmul_rn((float)(0 + hi), 0.5f);
}

// ---------------------------------------------------------------- B3 - B4: the path inside the band
// D of this lane's row in the band layout (entry q = column - off) and, for lane 0, the hand-over row, for the steps
// [t0, t0 + DTW_U) of a strip whose window starts at column wlo; entries outside the row are read at its ends and not used
DEV void dtw_band_load(DtwBlock& b, const float* __restrict__ drow, const float* hand, int j0, int off, int width, int nb) {
#pragma unroll
  for(int k = 0; k < DTW_U; k ++) {
    b.d[k] = drow[min(max(j0 + k - off, 0), width - 1)];
    b.p[k] = hand[min(max(j0 + k, 0), nb - 1)];
  }
}

// The walk of k_align_dtw over the column window [lo of the strip's first row, hi of its last row] of each strip: at step t
// lane l is on column wlo + t - l.  Which of the three candidates exist is decided by lo / hi of the lane's row and of the
// row above (rule B3), never by the values, so what a lane that was outside its row's range hands on -- and what an
// earlier strip left in the hand-over row outside the range of the row that wrote it last -- is never used.
// The hand-over row is indexed by the column itself, and all lanes of a strip count their steps from the same wlo: lane 0
// loads column x at step x - wlo - 2 DTW_U + 1 at the earliest ... x - wlo at the latest, lane 63 stores column x at step
// x - wlo + 63, so the reads stay ahead of the writes by 63 steps at the least, wherever the windows of the strips start.
__global__ __launch_bounds__(WAVE) void k_align_band_dtw(AlignBandDev d, const float* __restrict__ plane,
  uint4* __restrict__ moves, float* __restrict__ hand_rows, float* __restrict__ out, int cost0) {
  const int lane = threadIdx.x;
  const AlignBandPair p = d.pairs[blockIdx.x];
  const int na = p.na, nb = p.nb, band = p.band, width = 2 * band + 1;
  const float* D = plane + (size_t)p.cell0;
  float* hand = hand_rows + (size_t)p.row0;
  uint4* mv = moves + p.mv0;
  const long long per_strip = p.steps;
  const float step = d.step_cost;
  const int nstrips = (na + WAVE - 1) / WAVE;
  float v = 0.0f;                                                     // acc of this lane's last cell
  for(int s = 0; s < nstrips; s ++) {
    const int i = s * WAVE + lane, rows = min(WAVE, na - s * WAVE);
    // the ranges of this lane's row and of the row above; an empty range (1, 0) where there is no such row
    int off = 0, lo = 1, hi = 0, plo = 1, phi = 0;
    if(i < na) {
      const int c = align_band_center(i, na, nb);
      off = c - band; lo = max(off, 0); hi = min(c + band, nb - 1);
      if(i > 0) { const int cp = align_band_center(i - 1, na, nb); plo = max(cp - band, 0); phi = min(cp + band, nb - 1); }
    }
    const int wlo = __shfl(lo, 0), whi = __shfl(hi, rows - 1), nsteps = whi - wlo + rows;
    const float* drow = D + (size_t)min(i, na - 1) * width;
    uint4* mvs = mv + (long long)s * per_strip;
    // what `up` was one step ago.  Lane 0 starts on column wlo, and where the row above starts further left its first
    // cell has a diagonal predecessor: column wlo - 1 of the hand-over row (the other lanes take a step before their first cell)
    float diag = hand[max(wlo - 1, 0)];
    unsigned long long w0 = 0, w1 = 0;                                // the masks of step (t & ~63) + lane
    DtwBlock cur, nxt;
    dtw_band_load(cur, drow, hand, wlo - lane, off, width, nb);       // (lane 0 alone uses the hand-over row: its j0 is wlo)
    for(int t0 = 0; t0 < nsteps; t0 += DTW_U) {
      dtw_band_load(nxt, drow, hand, wlo + t0 + DTW_U - lane, off, width, nb);
#pragma unroll
      for(int k = 0; k < DTW_U; k ++) {
        const int t = t0 + k;
        if(t >= nsteps) break;
        const int j = wlo + t - lane;
        const bool on = j >= lo && j <= hi;
        const bool has_dg = j - 1 >= plo && j - 1 <= phi, has_up = j >= plo && j <= phi, has_lf = j - 1 >= lo;
        const float up_raw = wave_shr1(cur.p[k], v);                  // acc[i-1][j]
        const float up = __fadd_rn(up_raw, step), lf = __fadd_rn(v, step);
        float m = diag; int move = 0;                                 // the first candidate that exists ...
        if(! has_dg) { m = up; move = 1; }
        if(! has_dg && ! has_up) { m = lf; move = 2; }
        if(has_dg && has_up && up < m) { m = up; move = 1; }          // ... and a later one only if strictly smaller
        if((has_dg || has_up) && has_lf && lf < m) { m = lf; move = 2; }
        float acc = __fadd_rn(m, cur.d[k]);
        if(i == 0 && j == 0) { acc = cur.d[k]; move = 0; }
        diag = up_raw;
        if(on) v = acc;
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
  if(lane == last) out[cost0 + blockIdx.x] = v;                       // acc[na-1][nb-1]: the last cell of the last row's range

  // B4: back along the moves, which by B3 stay inside the band; nothing is forced by value
  float* pos = out + (size_t)p.pos0;
  int i = na - 1, j = nb - 1, hi = j;
  int cur_s = -1, cur_b = -1, wlo = 0;
  uint4 w = make_uint4(0, 0, 0, 0);
  for(int guard = na + nb; guard > 0; guard --) {
    if(i == 0 && j == 0) break;
    const int s = i >> 6, l = i & (WAVE - 1);
    if(s != cur_s) wlo = max(align_band_center(s * WAVE, na, nb) - band, 0);
    const int t = j - wlo + l, blk = t & ~(WAVE - 1);
    if(t < 0 || t >= per_strip) break;                                // (a cell outside the band: no stored move leads there)
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
  if(lane == 0) pos[0] = __fmul_rn((float)(0 + hi), 0.5f);
}

// ---------------------------------------------------------------- launchers
int launch_align_dist(LaunchCtx* P, const AlignDev& d, const int4* tiles, int n_tiles, float* plane) {
  if(n_tiles == 0) return 0;
  LAUNCH("k_align_dist", k_align_dist, dim3(n_tiles), dim3(AD_NT), 0, d, tiles, plane);
  return 0;
}

int launch_align_dtw(LaunchCtx* P, const AlignDev& d, const float* plane, uint4* moves, float* row, float* out, int cost0) {
  if(d.n_pairs == 0) return 0;
  LAUNCH("k_align_dtw", k_align_dtw, dim3(d.n_pairs), dim3(WAVE), 0, d, plane, moves, row, out, cost0);
  return 0;
}

int launch_align_band_dist(LaunchCtx* P, const AlignBandDev& d, const int4* tiles, int n_tiles, float* plane) {
  if(n_tiles == 0) return 0;
  LAUNCH("k_align_band_dist", k_align_band_dist, dim3(n_tiles), dim3(AD_NT), 0, d, tiles, plane);
  return 0;
}

int launch_align_band_dtw(LaunchCtx* P, const AlignBandDev& d, const float* plane, uint4* moves, float* row, float* out, int cost0) {
  if(d.n_pairs == 0) return 0;
  LAUNCH("k_align_band_dtw", k_align_band_dtw, dim3(d.n_pairs), dim3(WAVE), 0, d, plane, moves, row, out, cost0);
  return 0;
}
