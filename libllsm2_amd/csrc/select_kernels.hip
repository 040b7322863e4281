// select_kernels.hip -- unit selection, llsm_gpu_batch_select (rules S1 - S5: llsm_gpu.h; host side:
// select.cpp).  Four kernels:
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
