// select_kernels.hip -- unit selection, llsm_gpu_batch_select (rules S1 - S5: llsm_gpu.h) and
// llsm_gpu_batch_select_chain (rules C1 - C6: llsm_gpu.h); host side: select.cpp.  Five kernels:
//
//   k_select_knn    S1 - S2, the hot path: nt x nb x count x 3 operations, the nt x nb distances never leave the registers.
//                   A workgroup of 256 threads takes 64 target frames and one segment of the bank (select_seg_len(nb)
//                   frames: a rule of nb alone, so that few target frames against a large bank still fill the device).
//                   Lane l owns target frame 64 x + l; a block of 64 bank frames at a time goes through the LDS and
//                   wavefront w owns its rows 16 w ... 16 w + 15, so a thread keeps 16 cells of one target frame in
//                   registers and walks k ascending for each: S1's order is per cell, and the bits follow from the rule.
//                   The cells are held as 8 pairs of neighbouring bank rows, so that subtraction, multiplication and
//                   addition are each one packed operation on two cells (one rounding per element, as the scalar forms).
//                   A thread keeps the eight lowest (c, f) of its target frame in registers, sorted; it visits f ascending,
//                   so a cell enters only when its c is strictly below the eighth and goes behind its equals: off the
//                   common path.  At the end the four wavefronts merge their lists through the LDS under the total order
//                   (c, f), and wavefront 0 writes the list of the segment.
//   k_select_merge  the eight lowest of the n_seg lists of a target frame under (c, f) -> plane 7.  One wavefront per frame,
//                   lane = segment (at most 64); eight rounds of a 64-bit minimum over the heads.  Not launched with one
//                   segment: k_select_knn then writes plane 7 itself.
//   k_select_join   S3: one wavefront per target frame, lane 8 a + j.  The 16 bank rows of a frame pair (B[s] of the eight
//                   slots a, B[fb] of the eight slots j) are staged once in the LDS, 64 columns at a time, and every lane
//                   walks k ascending over its two.
//   k_select_path   S4 - S5: one wavefront per target utterance, lane 8 j + a (the layout of k_f0_viterbi).
//   k_select_chain  C2 - C6: one wavefront per target utterance; followers, joins and the path step of a frame in one
//                   sequential loop, because the followers of a frame depend on the accumulated costs of the frame before.
//
// LDS of k_select_knn.  Both blocks are stored transposed, k major.  The bank block bk is [32][64 + 4]: a wavefront reads
// rows r ... r + 3 at one k as one 16-byte read with every lane on the same address (a broadcast); the stride of 68 keeps
// the reads aligned.  The target block tg is [32][64 + 1]: lane l reads tg[k][l], consecutive words; the staging pass,
// whose lanes run along k for the sake of coalesced global reads, writes at the odd stride of 65 words (k_align_dist_t).
// Rows past the end of either side are read as the last row and never listed.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>

#include "kernels.h"
#include "dev_common.h"
#include "launch.h"

#define SEL_CAP 1e30f                              // S1: c = d if d < 1e30f, else 1e30f
#define SEL_NONE INT_MAX                           // the frame index of an empty slot in registers (c = infinity)

struct SelList { float c[SELECT_K]; int f[SELECT_K]; };

DEV bool sel_less(float c1, int f1, float c2, int f2) { return c1 < c2 || (c1 == c2 && f1 < f2); }

// (c, f) with c < L.c[7], and f above every f of L: behind its equals
DEV void sel_insert_behind(SelList& L, float c, int f) {
  L.c[SELECT_K - 1] = c; L.f[SELECT_K - 1] = f;
#pragma unroll
  for(int s = SELECT_K - 1; s > 0; s --)
    if(L.c[s] < L.c[s - 1]) {
      const float tc = L.c[s]; L.c[s] = L.c[s - 1]; L.c[s - 1] = tc;
      const int tf = L.f[s]; L.f[s] = L.f[s - 1]; L.f[s - 1] = tf;
    }
}

// (c, f) below the eighth of L under the total order
DEV void sel_insert_ordered(SelList& L, float c, int f) {
  L.c[SELECT_K - 1] = c; L.f[SELECT_K - 1] = f;
#pragma unroll
  for(int s = SELECT_K - 1; s > 0; s --)
    if(sel_less(L.c[s], L.f[s], L.c[s - 1], L.f[s - 1])) {
      const float tc = L.c[s]; L.c[s] = L.c[s - 1]; L.c[s - 1] = tc;
      const int tf = L.f[s]; L.f[s] = L.f[s - 1]; L.f[s - 1] = tf;
    }
}

// ---------------------------------------------------------------- S1 - S2: the nearest bank frames
#define SK_NT 256
#define SK_KC 32                                   // columns of CODE per LDS stage
#define SK_BK (64 + 4)                             // stride of the transposed bank block, floats
#define SK_TG (64 + 1)                             // stride of the transposed target block, floats
#define SK_R 16                                    // bank rows per thread and block
typedef float v2f __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(SK_NT) void k_select_knn(SelectDev d, float* __restrict__ lists) {
  __shared__ __attribute__((aligned(16))) float sm[SK_KC * SK_BK + SK_KC * SK_TG];
  __shared__ int vb[64];
  float* bk = sm; float* tg = sm + SK_KC * SK_BK;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid >> 6, r0 = w * SK_R;
  const int g0 = blockIdx.x * 64, g = g0 + lane, gc = min(g, d.nt - 1);
  const int j_lo = blockIdx.y * d.seg_len, j_hi = min(d.nb, j_lo + d.seg_len);
  const float* T = d.code_t; const float* B = d.code_b;
  const int vt = T[(size_t)gc * d.dim] > 0.5f;
  int own_lo = 0, own_hi = 0;                                       // S2: the bank frames of the target's own utterance
  if(d.skip_own) { const int u = d.t_frm_utt[gc]; own_lo = d.b_frm_off[u]; own_hi = own_lo + d.b_nfrm[u]; }
  SelList L;
#pragma unroll
  for(int s = 0; s < SELECT_K; s ++) { L.c[s] = INFINITY; L.f[s] = SEL_NONE; }
  const int sk = tid & (SK_KC - 1), sr = tid >> 5;                  // staging: lanes along k

  for(int j0 = j_lo; j0 < j_hi; j0 += 64) {
    v2f acc[SK_R / 2];
#pragma unroll
    for(int r = 0; r < SK_R / 2; r ++) acc[r] = (v2f){0.0f, 0.0f};
    for(int k0 = 0; k0 < d.count; k0 += SK_KC) {
      const int kn = min(SK_KC, d.count - k0);
      __syncthreads();                                              // the stage, and the block, before have been read
      if(k0 == 0 && tid < 64) vb[tid] = B[(size_t)min(j0 + tid, d.nb - 1) * d.dim] > 0.5f;
#pragma unroll
      for(int r = 0; r < 64; r += SK_NT / SK_KC) {
        const int row = r + sr;
        float xb = 0.0f, xt = 0.0f;
        if(sk < kn) {
          xb = B[(size_t)min(j0 + row, d.nb - 1) * d.dim + d.first + k0 + sk];
          xt = T[(size_t)min(g0 + row, d.nt - 1) * d.dim + d.first + k0 + sk];
        }
        bk[sk * SK_BK + row] = xb;
        tg[sk * SK_TG + row] = xt;
      }
      __syncthreads();
      // (no contraction: the build has -ffp-contract=off, and the three operations are separate packed instructions)
#define SK_STEP(k)                                                                       \
      {                                                                                  \
        const float x = tg[(k) * SK_TG + lane];                                          \
        const v2f xx = (v2f){x, x};                                                      \
        _Pragma("unroll")                                                                \
        for(int q = 0; q < SK_R / 4; q ++) {                                             \
          const float4 y = *(const float4*)& bk[(k) * SK_BK + r0 + 4 * q];               \
          const v2f t0 = xx - (v2f){y.x, y.y}, t1 = xx - (v2f){y.z, y.w};                \
          acc[2 * q] = acc[2 * q] + t0 * t0;                                             \
          acc[2 * q + 1] = acc[2 * q + 1] + t1 * t1;                                     \
        }                                                                                \
      }
      if(kn == SK_KC) {
#pragma unroll
        for(int k = 0; k < SK_KC; k ++) SK_STEP(k)
      } else {
        for(int k = 0; k < kn; k ++) SK_STEP(k)
      }
#undef SK_STEP
    }
    // the 16 cells of this block: f ascending
#pragma unroll
    for(int r = 0; r < SK_R; r ++) {
      const int f = j0 + r0 + r;
      float dd = acc[r >> 1][r & 1];
      if(vb[r0 + r] != vt) dd = __fadd_rn(dd, d.voicing_cost);
      const float c = dd < SEL_CAP ? dd : SEL_CAP;
      if(f < j_hi && (f < own_lo || f >= own_hi) && c < L.c[SELECT_K - 1]) sel_insert_behind(L, c, f);
    }
  }

  // the four lists of a target frame -> one, by wavefront 0
  __syncthreads();                                                  // bk / tg have been read: the merge block takes their place
  float* mg = sm;                                                   // [3][16][64]
  if(w > 0) {
#pragma unroll
    for(int s = 0; s < SELECT_K; s ++) {
      mg[((w - 1) * 16 + s) * 64 + lane] = L.c[s];
      mg[((w - 1) * 16 + 8 + s) * 64 + lane] = __int_as_float(L.f[s]);
    }
  }
  __syncthreads();
  if(w > 0) return;
  for(int o = 0; o < SK_NT / WAVE - 1; o ++)
#pragma unroll
    for(int s = 0; s < SELECT_K; s ++) {
      const float c = mg[(o * 16 + s) * 64 + lane];
      const int f = __float_as_int(mg[(o * 16 + 8 + s) * 64 + lane]);
      if(sel_less(c, f, L.c[SELECT_K - 1], L.f[SELECT_K - 1])) sel_insert_ordered(L, c, f);
    }
  if(g >= d.nt) return;
  float* out = lists + ((size_t)blockIdx.y * d.nt + g) * 16;
#pragma unroll
  for(int s = 0; s < SELECT_K; s ++) {
    const bool none = L.f[s] == SEL_NONE;
    out[s] = none ? SEL_CAP : L.c[s];
    out[8 + s] = none ? -1.0f : (float)L.f[s];
  }
}

// ---------------------------------------------------------------- the lists of the segments -> plane 7
// c is never negative (a sum of squares from +0, a cost >= 0, or the cap), so its bits order as it does: the key of a
// head is (bits of c, f), and that of an empty slot all ones
DEV unsigned long long sel_key(float c, float f) {
  return f < 0.0f ? ~0ull : ((unsigned long long)__float_as_uint(c) << 32) | (unsigned)(int)f;
}

__global__ __launch_bounds__(256) void k_select_merge(SelectDev d, const float* __restrict__ lists, float* __restrict__ p7) {
  const int lane = threadIdx.x & (WAVE - 1), g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if(g >= d.nt) return;                                             // (the whole wavefront)
  float c[SELECT_K], f[SELECT_K];
#pragma unroll
  for(int s = 0; s < SELECT_K; s ++) { c[s] = SEL_CAP; f[s] = -1.0f; }
  if(lane < d.n_seg) {
    const float4* src = (const float4*)(lists + ((size_t)lane * d.nt + g) * 16);
    const float4 c0 = src[0], c1 = src[1], f0 = src[2], f1 = src[3];
    c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w; c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w;
    f[0] = f0.x; f[1] = f0.y; f[2] = f0.z; f[3] = f0.w; f[4] = f1.x; f[5] = f1.y; f[6] = f1.z; f[7] = f1.w;
  }
  unsigned long long mine = ~0ull;                                  // lane r: the r-th lowest
#pragma unroll
  for(int r = 0; r < SELECT_K; r ++) {
    const unsigned long long key = sel_key(c[0], f[0]);
    unsigned long long m = key;
#pragma unroll
    for(int o = 32; o > 0; o >>= 1) { const unsigned long long v = __shfl_xor(m, o, WAVE); m = v < m ? v : m; }
    if(lane == r) mine = m;
    if(key == m && m != ~0ull) {                                    // one lane: the frames of the segments differ
#pragma unroll
      for(int s = 0; s < SELECT_K - 1; s ++) { c[s] = c[s + 1]; f[s] = f[s + 1]; }
      c[SELECT_K - 1] = SEL_CAP; f[SELECT_K - 1] = -1.0f;
    }
  }
  if(lane < SELECT_K) {
    const bool none = mine == ~0ull;
    p7[(size_t)g * 16 + lane] = none ? SEL_CAP : __uint_as_float((unsigned)(mine >> 32));
    p7[(size_t)g * 16 + 8 + lane] = none ? -1.0f : (float)(int)(unsigned)mine;
  }
}

// ---------------------------------------------------------------- S3: joins
#define SJ_KC 64                                   // columns per LDS stage
#define SJ_S (SJ_KC + 1)

__global__ __launch_bounds__(256) void k_select_join(SelectDev d, const float* __restrict__ p7, float* __restrict__ p8) {
  __shared__ float rows[4][16][SJ_S];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6, a = lane >> 3, j = lane & 7;
  const int g = blockIdx.x * 4 + w, gc = min(g, d.nt - 1);
  const int* bu = d.b_frm_utt;
  const bool head = gc == d.t_frm_off[d.t_frm_utt[gc]];             // the first frame of its utterance: no join
  // s of slot a of the frame before, fb of slot j of this frame; -1: absent
  int fa = -1, sa = -1, fb = -1;
  if(! head) {
    fa = (int)p7[(size_t)(gc - 1) * 16 + 8 + a];
    fb = (int)p7[(size_t)gc * 16 + 8 + j];
    if(fa >= 0) sa = fa + 1 < d.nb && bu[fa + 1] == bu[fa] ? fa + 1 : fa;
  }
  const bool absent = fa < 0 || fb < 0;
  const bool natural = ! absent && fb == fa + 1 && bu[fb] == bu[fa];
  // row r of the stage: r < 8: B[s] of slot r (lanes 8 r hold it); else B[fb] of slot r - 8 (lanes r - 8 hold it)
  float acc = 0.0f;
  for(int k0 = 0; k0 < d.count; k0 += SJ_KC) {
    const int kn = min(SJ_KC, d.count - k0);
    __syncthreads();                                                // the stage before has been read
#pragma unroll
    for(int r = 0; r < 16; r ++) {
      const int row = r < 8 ? __shfl(sa, 8 * r, WAVE) : __shfl(fb, r - 8, WAVE);
      rows[w][r][lane] = row >= 0 && lane < kn ? d.code_b[(size_t)row * d.dim + d.first + k0 + lane] : 0.0f;
    }
    __syncthreads();
    for(int k = 0; k < kn; k ++) {
      const float t = __fsub_rn(rows[w][a][k], rows[w][8 + j][k]);
      acc = __fadd_rn(acc, __fmul_rn(t, t));
    }
  }
  float J = 0.0f;
  if(! absent && ! natural) {
    const bool vs = d.code_b[(size_t)sa * d.dim] > 0.5f, vf = d.code_b[(size_t)fb * d.dim] > 0.5f;
    if(vs != vf) acc = __fadd_rn(acc, d.voicing_cost);
    const float c = acc < SEL_CAP ? acc : SEL_CAP;
    J = __fadd_rn(d.join_cost, __fmul_rn(d.join_weight, c));
  }
  if(g < d.nt) p8[(size_t)g * 64 + lane] = J;                       // entry 8 a + j
}

// ---------------------------------------------------------------- S4 - S5: the path
// Lane 8 j + a owns the transition from state a of frame i - 1 to state j of frame i.  The rows of planes 7 and 8 are
// loaded SP_U frames ahead; the dependent chain of a frame is one addition, the (value, a) minimum over the eight lanes
// of a group, the addition of c, and the transposition that hands acc[a] to the lanes 8 j + a.  The back pointers, 3 bits
// per state at bit 8 j of a 64-bit word, are three ballots per frame: lane i % 64 keeps the word of frame i and the
// wavefront stores 64 of them at a time.  The walk back loads them 64 at a time and reads them with scalar lane reads;
// lane k notes the state of frame base + k and writes utt and pos of that frame afterwards.
#define SP_U 4
#define DPP_XOR1 0xB1
#define DPP_XOR2 0x4E
#define DPP_ROR4 0x124
#define DPP_ROR12 0x12C
template <int CTRL> DEV int sp_dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }
template <int CTRL> DEV float sp_dpp_f(float v) { return __builtin_bit_cast(float, sp_dpp_i<CTRL>(__builtin_bit_cast(int, v))); }

struct SelRows { float c[SP_U], J[SP_U]; };
DEV void sp_load(SelRows& r, const float* __restrict__ p7, const float* __restrict__ p8, int base, int n, int j, int a) {
#pragma unroll
  for(int k = 0; k < SP_U; k ++) {
    const size_t i = (size_t)min(base + k, n - 1);
    r.c[k] = p7[i * 16 + j]; r.J[k] = p8[i * 64 + 8 * a + j];
  }
}

__global__ __launch_bounds__(WAVE) void k_select_path(SelectDev d, const float* __restrict__ p7g, const float* __restrict__ p8g,
  uint2* __restrict__ bp, int* __restrict__ out) {
  const int u = blockIdx.x, lane = threadIdx.x, j = lane >> 3, a = lane & 7;
  const int n = d.t_nfrm[u], g0 = d.t_frm_off[u];
  int* cost = out + 2 * (size_t)d.nt;
  if(n <= 0) { if(lane == 0) cost[u] = __float_as_int(0.0f); return; }
  const float* p7 = p7g + (size_t)g0 * 16; const float* p8 = p8g + (size_t)g0 * 64;
  uint2* bpu = bp + g0;
  // n_u: the slots of frame 0 that hold a frame (the same for every frame of the utterance)
  const int nu = __popcll(__ballot(a == 0 && p7[8 + j] >= 0.0f));
  float acc_a = 0.0f, acc_j = 0.0f;
  unsigned long long word = 0;                                         // the back pointers of frame (i & ~63) + lane
  SelRows cur, nxt;
  sp_load(cur, p7, p8, 0, n, j, a);
  for(int b = 0; b < n; b += SP_U) {
    sp_load(nxt, p7, p8, b + SP_U, n, j, a);
#pragma unroll
    for(int k = 0; k < SP_U; k ++) {
      const int i = b + k;
      if(i >= n) break;
      // frame 0: acc_0[j] = 0 + c_0[j] = c_0[j] (c is never -0); absent slots are no predecessor
      float v = i == 0 ? (a == 0 ? 0.0f : INFINITY) : (a < nu ? __fadd_rn(acc_a, cur.J[k]) : INFINITY);
      int arg = a;
      auto take = [&](float ov, int oa) { if(ov < v || (ov == v && oa < arg)) { v = ov; arg = oa; } };
      take(sp_dpp_f<DPP_XOR1>(v), sp_dpp_i<DPP_XOR1>(arg));
      take(sp_dpp_f<DPP_XOR2>(v), sp_dpp_i<DPP_XOR2>(arg));
      // lane ^ 4 is 12 or 4 lanes round the row; both reads are made with every lane active, then one is chosen
      const float v_up = sp_dpp_f<DPP_ROR12>(v), v_dn = sp_dpp_f<DPP_ROR4>(v);
      const int a_up = sp_dpp_i<DPP_ROR12>(arg), a_dn = sp_dpp_i<DPP_ROR4>(arg);
      take(a < 4 ? v_up : v_dn, a < 4 ? a_up : a_dn);
      v = __fadd_rn(v, cur.c[k]);
      acc_j = v;
      acc_a = __shfl(v, 8 * a, WAVE);
      const unsigned long long w = __ballot(a == 0 && (arg & 1)) | (__ballot(a == 0 && (arg & 2)) << 1) |
                                   (__ballot(a == 0 && (arg & 4)) << 2);
      if((i & (WAVE - 1)) == lane) word = w;
      if(((i & (WAVE - 1)) == WAVE - 1 || i == n - 1) && lane <= (i & (WAVE - 1)))
        bpu[(i & ~(WAVE - 1)) + lane] = make_uint2((unsigned)word, (unsigned)(word >> 32));
    }
    cur = nxt;
  }
  // the path ends in the smallest state of least acc on the last frame
  const float mine = j < nu ? acc_j : INFINITY;
  float m = mine;
#pragma unroll
  for(int o = 32; o >= 8; o >>= 1) m = fminf(m, __shfl_xor(m, o, WAVE));
  int s = __builtin_amdgcn_readfirstlane((__ffsll((long long)__ballot(mine == m)) - 1) >> 3);
  if(lane == 0) cost[u] = __float_as_int(m);
  for(int base = (n - 1) & ~(WAVE - 1); base >= 0; base -= WAVE) {
    const int cnt = min(WAVE, n - base);
    uint2 w = make_uint2(0, 0);
    if(lane < cnt) w = bpu[base + lane];                               // (the lane's own stores: the same thread reads them)
    int st = 0;
    for(int k = cnt - 1; k >= 0; k --) {                               // (a scalar chain: unrolled 64 times it spills scalars)
      if(lane == k) st = s;
      const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)w.x, k), hi = (unsigned)__builtin_amdgcn_readlane((int)w.y, k);
      s = ((s < 4 ? lo : hi) >> (8 * (s & 3))) & 7;                    // the state of frame base + k - 1
    }
    if(lane < cnt) {                                                   // S5
      const int g = g0 + base + lane;
      const int f = (int)p7[(size_t)(base + lane) * 16 + 8 + st];
      const int ub = d.b_frm_utt[f];
      out[g] = ub;
      out[(size_t)d.nt + g] = __float_as_int((float)(f - d.b_frm_off[ub]));
    }
  }
}

// ---------------------------------------------------------------- C2 - C6: followers, joins and the path, one loop
// A frame has up to 16 states: slots 0 ... 7 the near list of k_select_knn / k_select_merge, slots 8 ... 15 the followers.
// Lane s < 16 owns state s between frames: its bank frame (-1: absent), the end of that frame's bank utterance, and acc.
// Within a frame lane l owns the pairs (a, j) = (4 q + (l >> 4), l & 15), q = 0 ... 3: entry 16 a + j of plane 11 is word
// 64 q + l of the row, and the minimum over a is four values in the lane and two exchanges across the lanes l ^ 16, l ^ 32.
//
// Per frame i >= 1:
//   1. the rows loaded one frame ahead go into the LDS: rows 0 ... 15 B[s_a] of the states a of frame i - 1 (B[fa] where
//      there is no successor: rule S3), rows 16 ... 23 the near rows of frame i, row 24 T[g]; 64 columns at a time, and
//      column 64 of a row, the padding of the odd stride, holds whether the row is voiced
//   2. C3: pool membership (a successor, and not among the eight near frames), the rank of every pool state under (acc, a)
//      by 16 scalar lane reads, and the parent of every follower slot by 8 ballots; the new state set is then fixed
//   3. the loads of frame i + 1 are issued: its S rows follow from the state set alone, not from the path step below
//   4. k ascending, eight columns at a time, each lane: its four join sums (row a against row j: a near row, or the S row of j's parent, which is
//      the follower's own row) and one target sum (T[g] against S row l & 15: the cost of the follower it may become)
//   5. C4 / C5, the rows of planes 10 and 11, and the back pointers: four ballots, bit 4 j + b of the word = bit b of arg_j
// The near lists are loaded three frames ahead, the bank utterances of their frames two and the ends of those one, each a
// frame after the value it depends on: no load of a list stands in the chain.
#define SC_KC 64                                   // columns per LDS stage
#define SC_S (SC_KC + 1)                           // row stride; column SC_KC: voiced
#define SC_NS SELECT_STATES
#define SC_ROW_N SC_NS                             // first near row
#define SC_ROW_T (SC_NS + SELECT_K)                // the target row
#define SC_ROW_SPARE (SC_ROW_T + 1)                // never read
#define SC_ABSENT 99                               // the argument of a predecessor that is absent: above every state

struct ScRows { float s[SC_NS], n[SELECT_K], t, vs, vn, vt; };

// columns [k0, k0 + 64) of the rows of frame g: lane r < 16 holds srow of S row r (-1: none), lane r < 8 near frame nf.
// Every load is made: a row that is absent reads row 0 and a lane past the last column the last column -- no state
// that is present reads either -- so that the 28 loads are one straight run
DEV void sc_load(ScRows& r, const SelectDev& d, int srow, int nf, int g, int k0, int lane) {
  const int col = d.first + k0 + min(lane, min(SC_KC, d.count - k0) - 1);
  const float* B = d.code_b + col;
  const unsigned dim = (unsigned)d.dim;
#pragma unroll
  for(int q = 0; q < SC_NS; q ++)                                   // (a vector register each: 24 scalar row bases spill)
    r.s[q] = B[(size_t)(unsigned)max(__shfl(srow, q, WAVE), 0) * dim];
#pragma unroll
  for(int q = 0; q < SELECT_K; q ++)
    r.n[q] = B[(size_t)(unsigned)max(__shfl(nf, q, WAVE), 0) * dim];
  r.t = d.code_t[(size_t)g * dim + col];
  r.vs = d.code_b[(size_t)(unsigned)max(srow, 0) * dim];
  r.vn = d.code_b[(size_t)(unsigned)max(nf, 0) * dim];
  r.vt = d.code_t[(size_t)g * dim];
}

// The voicing words are stored by every lane, the lanes that hold none into a spare row: under a branch the loaded value
// would stay pending on the path around it, and the wait for it -- for every load, the rows of the next frame among them
// -- would land at the head of the column loop
DEV void sc_store(float (*rows)[SC_S], const ScRows& r, int lane) {
#pragma unroll
  for(int q = 0; q < SC_NS; q ++) rows[q][lane] = r.s[q];
#pragma unroll
  for(int q = 0; q < SELECT_K; q ++) rows[SC_ROW_N + q][lane] = r.n[q];
  rows[SC_ROW_T][lane] = r.t;
  float* spare = & rows[SC_ROW_SPARE][lane];
  *(lane < SC_NS ? & rows[lane][SC_KC] : spare) = r.vs > 0.5f ? 1.0f : 0.0f;
  *(lane < SELECT_K ? & rows[SC_ROW_N + lane][SC_KC] : spare) = r.vn > 0.5f ? 1.0f : 0.0f;
  *(lane == 0 ? & rows[SC_ROW_T][SC_KC] : spare) = r.vt > 0.5f ? 1.0f : 0.0f;
}

// bit i of the low 16 bits -> bit 4 i
DEV unsigned long long sc_spread(unsigned long long x) {
  x &= 0xFFFFull;
  x = (x | (x << 24)) & 0x000000FF000000FFull;
  x = (x | (x << 12)) & 0x000F000F000F000Full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}

DEV float sc_readlane_f(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

__global__ __launch_bounds__(WAVE) void k_select_chain(SelectDev d, const float* __restrict__ nearg, float* __restrict__ p10g,
  float* __restrict__ p11g, uint2* __restrict__ bp, int* __restrict__ out) {
  __shared__ float rows[SC_ROW_SPARE + 1][SC_S];
  const int u = blockIdx.x, lane = threadIdx.x, jj = lane & (SC_NS - 1), ah = lane >> 4;
  const int n = d.t_nfrm[u], g0 = d.t_frm_off[u];
  int* cost = out + 2 * (size_t)d.nt;
  if(n <= 0) { if(lane == 0) cost[u] = __float_as_int(0.0f); return; }
  const float* near = nearg + (size_t)g0 * 16;
  float* p10 = p10g + (size_t)g0 * 32; float* p11 = p11g + (size_t)g0 * 256;
  uint2* bpu = bp + g0;
  const int* bu = d.b_frm_utt;
  // the near list of frame i (clamped to the utterance) in lanes 0 ... 7; the other lanes hold an absent slot
  auto near_load = [&](int i, float& c, int& f) {
    const size_t at = (size_t)min(i, n - 1) * 16;
    c = lane < SELECT_K ? near[at + lane] : SEL_CAP;
    f = lane < SELECT_K ? (int)near[at + 8 + lane] : -1;
  };
  // frames i ... i + 3: f the bank frames, u their bank utterances, e the ends of those; each is asked for one frame after
  // the value it depends on, so that no load of the lists stands in the chain
  float c_i, c_1, c_2, c_3; int f_i, f_1, f_2, f_3, e_i, e_1, u_1, u_2;
  near_load(0, c_i, f_i); near_load(1, c_1, f_1); near_load(2, c_2, f_2); near_load(3, c_3, f_3);
  { const int ub = bu[max(f_i, 0)]; e_i = d.b_frm_off[ub] + d.b_nfrm[ub]; }
  { const int ub = bu[max(f_1, 0)]; e_1 = d.b_frm_off[ub] + d.b_nfrm[ub]; }
  u_2 = bu[max(f_2, 0)];
  // C2: the states of frame 0 are its near slots
  int sf = f_i, se = e_i;
  float sacc = sf >= 0 ? c_i : INFINITY;
  int srow = sf < 0 ? -1 : sf + 1 < se ? sf + 1 : sf;
  if(lane < SC_NS) { p10[lane] = c_i; p10[SC_NS + lane] = (float)sf; }
#pragma unroll
  for(int q = 0; q < 4; q ++) p11[64 * q + lane] = 0.0f;
  if(lane == 0) bpu[0] = make_uint2(0, 0);
  ScRows pre;                                                       // (the frame after the last: the last again, unused)
  sc_load(pre, d, srow, f_1, g0 + min(1, n - 1), 0, lane);

  for(int i = 1; i < n; i ++) {
    const int g = g0 + i;
    c_i = c_1; f_i = f_1; e_i = e_1;
    c_1 = c_2; f_1 = f_2; u_1 = u_2;
    c_2 = c_3; f_2 = f_3;
    near_load(i + 3, c_3, f_3);
    u_2 = bu[max(f_2, 0)];
    e_1 = d.b_frm_off[u_1] + d.b_nfrm[u_1];
    __syncthreads();                                                // the rows of the frame before have been read
    sc_store(rows, pre, lane);
    // ---- C3
    const bool has = sf >= 0 && sf + 1 < se;
    const int succ = sf + 1;
    bool isnear = false;
#pragma unroll
    for(int k = 0; k < SELECT_K; k ++) isnear |= __builtin_amdgcn_readlane(f_i, k) == succ;
    const bool inpool = has && ! isnear;
    const unsigned pm = (unsigned)__ballot(inpool);
    // the rank of a pool state: the pool states before it under (acc, a).  The comparisons are gathered as bits, one per
    // state b, and the parents as one byte per follower slot: predicates on the lane number alone, one per b and per
    // slot, would be kept as lane masks across the frame loop and spill scalar registers
    unsigned lt = 0, eq = 0;
#pragma unroll
    for(int b = 0; b < SC_NS; b ++) {
      const float ab = sc_readlane_f(sacc, b);
      lt |= (unsigned)(ab < sacc) << b; eq |= (unsigned)(ab == sacc) << b;
    }
    const int rank = __popc(pm & (lt | (eq & ((1u << (lane & 31)) - 1u))));
    const bool taken = inpool && rank < SELECT_K;
    unsigned long long pw = 0;                                      // byte r: 1 + the parent of follower slot r, 0: none
#pragma unroll
    for(int r = 0; r < SELECT_K; r ++)
      pw |= (unsigned long long)__ffsll((long long)__ballot(taken && rank == r)) << (8 * r);
    const int par = (lane >> 3) == 1 ? (int)((pw >> (8 * (lane & 7))) & 0xFF) - 1 : -1;   // lane 8 + r: the parent of slot r
    const int src = max(par, 0);
    const int f_par = __shfl(succ, src, WAVE), e_par = __shfl(se, src, WAVE);
    const int nf = lane < SELECT_K ? f_i : par >= 0 ? f_par : -1;  // the states of frame i (lanes >= 16: absent)
    const int ne = lane < SELECT_K ? e_i : e_par;
    const int srow_1 = nf < 0 ? -1 : nf + 1 < ne ? nf + 1 : nf;
    // ---- the rows of frame i + 1, one frame ahead of the chain
    ScRows nxt;
    sc_load(nxt, d, srow_1, f_1, g0 + min(i + 1, n - 1), 0, lane);
    // ---- the sums, k ascending
    const int par_j = __shfl(par, jj, WAVE);
    const int frow = jj < SELECT_K ? SC_ROW_N + jj : max(par_j, 0);
    float accJ[4] = {0.0f, 0.0f, 0.0f, 0.0f}, accT = 0.0f;
    for(int k0 = 0; k0 < d.count; k0 += SC_KC) {
      if(k0 > 0) {                                                  // further columns: loaded here
        ScRows x;
        sc_load(x, d, srow, f_i, g, k0, lane);
        __syncthreads();
        sc_store(rows, x, lane);
      }
      __syncthreads();
      const int kn = min(SC_KC, d.count - k0);
      // (eight columns at a time where there are eight: one wavefront per SIMD has nothing else to cover the LDS reads of
      // a column with, so the 56 reads of eight columns are issued together, ahead of the sums, which stay k ascending)
      int k = 0;
      for(; k + 8 <= kn; k += 8) {
        float y[8], x[4][8], tg[8], sj[8];
#pragma unroll
        for(int e = 0; e < 8; e ++) {
          y[e] = rows[frow][k + e]; tg[e] = rows[SC_ROW_T][k + e]; sj[e] = rows[jj][k + e];
#pragma unroll
          for(int q = 0; q < 4; q ++) x[q][e] = rows[4 * q + ah][k + e];
        }
#pragma unroll
        for(int e = 0; e < 8; e ++) {
#pragma unroll
          for(int q = 0; q < 4; q ++) {
            const float t = __fsub_rn(x[q][e], y[e]);
            accJ[q] = __fadd_rn(accJ[q], __fmul_rn(t, t));
          }
          const float tt = __fsub_rn(tg[e], sj[e]);
          accT = __fadd_rn(accT, __fmul_rn(tt, tt));
        }
      }
      for(; k < kn; k ++) {
        const float y = rows[frow][k];
#pragma unroll
        for(int q = 0; q < 4; q ++) {
          const float t = __fsub_rn(rows[4 * q + ah][k], y);
          accJ[q] = __fadd_rn(accJ[q], __fmul_rn(t, t));
        }
        const float tt = __fsub_rn(rows[SC_ROW_T][k], rows[jj][k]);
        accT = __fadd_rn(accT, __fmul_rn(tt, tt));
      }
    }
    // ---- the costs of the followers: lane a < 16 holds c(T[g], B[s_a]), slot 8 + r takes its parent's
    if(rows[SC_ROW_T][SC_KC] != rows[jj][SC_KC]) accT = __fadd_rn(accT, d.voicing_cost);
    const float ct = accT < SEL_CAP ? accT : SEL_CAP;
    const float c_par = __shfl(ct, src, WAVE);
    const float nc = lane < SELECT_K ? c_i : par >= 0 ? c_par : SEL_CAP;
    if(lane < SC_NS) { p10[(size_t)i * 32 + lane] = nc; p10[(size_t)i * 32 + SC_NS + lane] = (float)nf; }
    // ---- C4 and the minimum of C5 over a ascending
    const int fj = __shfl(nf, jj, WAVE);
    const float vj = rows[frow][SC_KC];
    float m = INFINITY; int arg = SC_ABSENT;
#pragma unroll
    for(int q = 0; q < 4; q ++) {
      const int a = 4 * q + ah;
      const int fa = __shfl(sf, a, WAVE), ea = __shfl(se, a, WAVE);
      const float acc_a = __shfl(sacc, a, WAVE);
      const bool absent = fa < 0 || fj < 0;
      const bool natural = fj == fa + 1 && fj < ea;
      float J = 0.0f;
      if(! absent && ! natural) {
        float dd = accJ[q];
        if(rows[a][SC_KC] != vj) dd = __fadd_rn(dd, d.voicing_cost);
        const float c = dd < SEL_CAP ? dd : SEL_CAP;
        J = __fadd_rn(d.join_cost, __fmul_rn(d.join_weight, c));
      }
      p11[(size_t)i * 256 + 64 * q + lane] = J;
      const float v = fa >= 0 ? __fadd_rn(acc_a, J) : INFINITY;
      const int va = fa >= 0 ? a : SC_ABSENT;
      if(v < m || (v == m && va < arg)) { m = v; arg = va; }
    }
#pragma unroll
    for(int o = 16; o <= 32; o <<= 1) {
      const float ov = __shfl_xor(m, o, WAVE); const int oa = __shfl_xor(arg, o, WAVE);
      if(ov < m || (ov == m && oa < arg)) { m = ov; arg = oa; }
    }
    const bool live = lane < SC_NS && nf >= 0;
    const float nacc = live ? __fadd_rn(m, nc) : INFINITY;
    const unsigned long long word = sc_spread(__ballot(live && (arg & 1))) | (sc_spread(__ballot(live && (arg & 2))) << 1) |
                                    (sc_spread(__ballot(live && (arg & 4))) << 2) | (sc_spread(__ballot(live && (arg & 8))) << 3);
    if(lane == 0) bpu[i] = make_uint2((unsigned)word, (unsigned)(word >> 32));
    // ---- frame i is done
    sf = nf; se = ne; sacc = nacc; srow = srow_1; pre = nxt;
  }

  // the path ends in the smallest state of least acc on the last frame
  const bool live = lane < SC_NS && sf >= 0;
  const float mine = live ? sacc : INFINITY;
  float m = mine;
#pragma unroll
  for(int o = 8; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, WAVE));
  m = sc_readlane_f(m, 0);
  int s = __builtin_amdgcn_readfirstlane(__ffsll((long long)__ballot(live && mine == m)) - 1);
  if(lane == 0) cost[u] = __float_as_int(m);
  __threadfence();                                                  // plane 10 and the back pointers were written by other lanes
  __syncthreads();
  for(int base = (n - 1) & ~(WAVE - 1); base >= 0; base -= WAVE) {
    const int cnt = min(WAVE, n - base);
    uint2 w = make_uint2(0, 0);
    if(lane < cnt) w = bpu[base + lane];
    int st = 0;
    for(int k = cnt - 1; k >= 0; k --) {
      if(lane == k) st = s;
      const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)w.x, k), hi = (unsigned)__builtin_amdgcn_readlane((int)w.y, k);
      s = ((s < 8 ? lo : hi) >> (4 * (s & 7))) & 15;                // the state of frame base + k - 1
    }
    if(lane < cnt) {                                                // C6
      const int g = g0 + base + lane;
      const int f = min(max((int)p10[(size_t)(base + lane) * 32 + SC_NS + st], 0), d.nb - 1);   // (a present state: in the bank)
      const int ub = bu[f];
      out[g] = ub;
      out[(size_t)d.nt + g] = __float_as_int((float)(f - d.b_frm_off[ub]));
    }
  }
}

// ---------------------------------------------------------------- launchers
int launch_select_knn(LaunchCtx* P, const SelectDev& d, float* lists) {
  if(d.nt == 0) return 0;
  LAUNCH("k_select_knn", k_select_knn, dim3((d.nt + 63) / 64, d.n_seg), dim3(SK_NT), 0, d, lists);
  return 0;
}

int launch_select_merge(LaunchCtx* P, const SelectDev& d, const float* lists, float* p7) {
  if(d.nt == 0) return 0;
  LAUNCH("k_select_merge", k_select_merge, dim3((d.nt + 3) / 4), dim3(256), 0, d, lists, p7);
  return 0;
}

int launch_select_join(LaunchCtx* P, const SelectDev& d, const float* p7, float* p8) {
  if(d.nt == 0) return 0;
  LAUNCH("k_select_join", k_select_join, dim3((d.nt + 3) / 4), dim3(256), 0, d, p7, p8);
  return 0;
}

int launch_select_path(LaunchCtx* P, const SelectDev& d, const float* p7, const float* p8, uint2* bp, int* out) {
  if(d.n_utt == 0) return 0;
  LAUNCH("k_select_path", k_select_path, dim3(d.n_utt), dim3(WAVE), 0, d, p7, p8, bp, out);
  return 0;
}

int launch_select_chain(LaunchCtx* P, const SelectDev& d, const float* near, float* p10, float* p11, uint2* bp, int* out) {
  if(d.n_utt == 0) return 0;
  LAUNCH("k_select_chain", k_select_chain, dim3(d.n_utt), dim3(WAVE), 0, d, near, p10, p11, bp, out);
  return 0;
}
