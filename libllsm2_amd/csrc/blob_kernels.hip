// blob_kernels.hip -- a device-resident batch written out as chunk blobs (wire.cpp's format; host side: batch_blob.cpp).
//
// The bytes of an utterance's blob are those llsm_chunk_to_blob writes for the chunk that llsm_flat_to_chunk /
// llsm_flat_l1_to_chunk (has_rd = 1, HM dropped where HAS_HM is 0) build from the utterance's rows.  Going through the
// container tree normalises the rows; both kernels apply the same rules per frame (frame_counts below):
//   NHAR      survives on voiced frames (F0 != 0) whose HM is valid (HAS_HM != 0, or a batch without layer 1), else 0
//   NHAR_E    survives on voiced frames, else 0 (an unvoiced frame keeps the envelopes of a fresh frame)
//   NVSPHSE   survives where it is > 0 (layer 1 only); VTMAGN is zero where it is 0
//   AMPL / PHSE / VSPHSE / EENV rows are zero beyond their surviving count; PSDRES is zero where HAS_PSDRES is 0
//   HAS_PSDRES and HAS_HM are written as 0 / 1, HAS_RD as 1; F0, RD, PBPSYN, PSD and EDC go through unchanged
//
//   k_blob_widths  one workgroup per utterance: the largest surviving NHAR, NVSPHSE and NHAR_E over its frames -- the row
//                  widths of its blob (header maxnhar = max of the first two, maxnhar_e the third)
//   k_blob_pack    four consecutive frames of ONE utterance per 256-thread workgroup (k_pitch_formant's shape).  The rows
//                  that keep their width (PSD, PSDRES, VTMAGN) go one wavefront per frame with 16-byte stores on the
//                  destination's 16-byte grid (a blob's arrays start on multiples of 8, so up to three single floats lead
//                  and trail; the loads are 16 bytes at whatever alignment that leaves the source).  The rows that narrow
//                  to the blob's widths (AMPL, PHSE, VSPHSE, EENV) and EDC are contiguous over the four frames on the
//                  destination side and go as single floats across the whole workgroup.  One more workgroup per utterance
//                  writes the header, chanfreq, the zero word behind every array of odd length and the gap up to the next
//                  blob, so that every byte of the staging area comes from this kernel and none from a memset.
// Pure data movement: every row byte is read once and written once, no LDS beyond the four frames' counts.
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "kernels.h"
#include "launch.h"
#include "wire_layout.h"

using namespace llsm_wire;

namespace {
const int kBpFrames = 4, kBpThreads = 256;

struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };       // 16 bytes at float alignment

DEV int bclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the counts of frame g that survive the container tree (header comment)
DEV void frame_counts(const ModRows& r, int g, int* nh, int* nv, int* ne) {
  const bool voiced = r.f0[g] != 0.0f;
  const bool hm = voiced && (r.has_hm == nullptr || r.has_hm[g] != 0);
  *nh = hm ? bclamp(r.nhar[g], 0, r.maxnhar) : 0;
  *nv = r.nvsphse ? bclamp(r.nvsphse[g], 0, r.maxnhar) : 0;
  *ne = voiced ? bclamp(r.nhar_e[g], 0, r.maxnhar_e) : 0;
}

// one row of n floats by one wavefront: d <- s (live) or zeros
DEV void wide_row(float* __restrict__ d, const float* __restrict__ s, int n, bool live, int lane) {
  int head = (int)(((16u - ((unsigned)(uintptr_t)d & 15u)) & 15u) >> 2);
  if(head > n) head = n;
  if(lane < head) d[lane] = live ? s[lane] : 0.0f;
  const int n4 = (n - head) >> 2;
  float4* d4 = (float4*)(d + head); const F4U* s4 = (const F4U*)(s + head);
  for(int q = lane; q < n4; q += 64) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if(live) { const F4U t = s4[q]; v = make_float4(t.x, t.y, t.z, t.w); }
    d4[q] = v;
  }
  const int e = head + (n4 << 2) + lane;
  if(e < n) d[e] = live ? s[e] : 0.0f;
}

// rows of nf frames narrowed from width ws to wd (rows_per_frame of them per frame), contiguous on both sides per frame:
// element k of a row survives when k < cnt[frame]
DEV void narrow_rows(float* __restrict__ d, const float* __restrict__ s, int nf, int rows_per_frame, int wd, int ws,
  const int* cnt, int tid) {
  const int per = rows_per_frame * wd, n = nf * per;
  for(int e = tid; e < n; e += kBpThreads) {
    const int f = e / per, q = e - f * per, c = q / wd, k = q - c * wd;
    d[e] = k < cnt[f] ? s[((size_t)f * rows_per_frame + c) * ws + k] : 0.0f;
  }
}
}  // namespace

__global__ __launch_bounds__(256) void k_blob_widths(ModRows r, const int* __restrict__ frm_off, const int* __restrict__ nfrm,
  int* __restrict__ widths) {
  __shared__ int s_w[4][3];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int off = frm_off[u], n = nfrm[u];
  int mh = 0, mv = 0, me = 0;
  for(int i = tid; i < n; i += 256) {
    int nh, nv, ne; frame_counts(r, off + i, & nh, & nv, & ne);
    mh = max(mh, nh); mv = max(mv, nv); me = max(me, ne);
  }
  for(int o = 32; o > 0; o >>= 1) {
    mh = max(mh, __shfl_xor(mh, o, WAVE)); mv = max(mv, __shfl_xor(mv, o, WAVE)); me = max(me, __shfl_xor(me, o, WAVE));
  }
  if((tid & 63) == 0) { s_w[tid >> 6][0] = mh; s_w[tid >> 6][1] = mv; s_w[tid >> 6][2] = me; }
  __syncthreads();
  if(tid < 3) widths[3 * u + tid] = max(max(s_w[0][tid], s_w[1][tid]), max(s_w[2][tid], s_w[3][tid]));
}

// grid: x = utterance of the table, y = groups of four frames, strided; group index == number of groups: the header item
__global__ __launch_bounds__(kBpThreads) void k_blob_pack(ModRows r, const BlobEntry* __restrict__ tab,
  const float* __restrict__ chanfreq, unsigned char* __restrict__ stage) {
  __shared__ int s_nh[kBpFrames], s_nv[kBpFrames], s_ne[kBpFrames], s_res[kBpFrames];
  const BlobEntry& E = tab[blockIdx.x];
  const Header& h = E.h;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int F = h.nfrm, wh = h.maxnhar, we = h.maxnhar_e > 0 ? h.maxnhar_e : 1, ns = h.nspec;
  const int np = r.npsd, nch = r.nchannel, me = r.maxnhar_e > 0 ? r.maxnhar_e : 1;
  unsigned char* base = stage + E.base;
  const int ngroups = (F + kBpFrames - 1) / kBpFrames;
  for(int gi = blockIdx.y; gi <= ngroups; gi += gridDim.y) {
    if(gi == ngroups) {                                   // header, chanfreq, padding words, gap to the next blob
      const uint32_t* hw = (const uint32_t*)& h;
      if(tid < (int)(sizeof(Header) / 4)) ((uint32_t*)base)[tid] = hw[tid];
      if(tid < h.nchanfreq) ((float*)(base + h.offset[A_CHANFREQ]))[tid] = chanfreq[tid];
      if(tid < NARR) {
        Shape s; s.nfrm = F; s.maxnhar = wh; s.me = h.maxnhar_e; s.npsd = h.npsd; s.nch = h.nchannel; s.ncf = h.nchanfreq;
        s.nspec = ns;
        size_t b[NARR]; array_bytes(s, b);
        size_t mine = 0;
        for(int i = 0; i < NARR; i ++) if(i == tid) mine = b[i];
        if(mine & 4) *(uint32_t*)(base + h.offset[tid] + mine) = 0u;
      }
      const int gap = (int)((16u - (unsigned)(h.total_bytes & 15u)) & 15u) >> 2;
      if(tid < gap) ((uint32_t*)(base + h.total_bytes))[tid] = 0u;
      continue;
    }
    const int i0 = gi * kBpFrames, nf = min(kBpFrames, F - i0), g0 = E.frm0 + i0;
    __syncthreads();                                      // (the previous group's counts are no longer read)
    if(tid < nf) {
      const int g = g0 + tid, i = i0 + tid;
      int nh, nv, ne; frame_counts(r, g, & nh, & nv, & ne);
      nh = min(nh, wh); nv = min(nv, wh); ne = min(ne, h.maxnhar_e);       // (never past the blob's rows)
      const int res = r.has_psdres[g] != 0;
      s_nh[tid] = nh; s_nv[tid] = nv; s_ne[tid] = ne; s_res[tid] = res;
      ((float*)(base + h.offset[A_F0]))[i] = r.f0[g];
      ((int*)(base + h.offset[A_NHAR]))[i] = nh;
      ((int*)(base + h.offset[A_HASRES]))[i] = res;
      ((int*)(base + h.offset[A_NHAR_E]))[i] = ne;
      if(ns > 0) {
        ((float*)(base + h.offset[A_RD]))[i] = r.rd[g];
        ((int*)(base + h.offset[A_HASRD]))[i] = 1;
        ((int*)(base + h.offset[A_NVS]))[i] = nv;
        ((int*)(base + h.offset[A_PBPSYN]))[i] = r.pbpsyn[g];
        ((int*)(base + h.offset[A_HASHM]))[i] = r.has_hm[g] != 0;
      }
    }
    __syncthreads();
    const size_t G0 = (size_t)g0, I0 = (size_t)i0;
    // narrowed rows and EDC: single floats, the four frames contiguous on the destination side
    if(wh > 0) {
      narrow_rows((float*)(base + h.offset[A_AMPL]) + I0 * wh, r.ampl + G0 * r.maxnhar, nf, 1, wh, r.maxnhar, s_nh, tid);
      narrow_rows((float*)(base + h.offset[A_PHSE]) + I0 * wh, r.phse + G0 * r.maxnhar, nf, 1, wh, r.maxnhar, s_nh, tid);
      if(ns > 0)
        narrow_rows((float*)(base + h.offset[A_VSPHSE]) + I0 * wh, r.vsphse + G0 * r.maxnhar, nf, 1, wh, r.maxnhar, s_nv, tid);
    }
    narrow_rows((float*)(base + h.offset[A_EAMP]) + I0 * nch * we, r.eenv_ampl + G0 * nch * me, nf, nch, we, me, s_ne, tid);
    narrow_rows((float*)(base + h.offset[A_EPHS]) + I0 * nch * we, r.eenv_phse + G0 * nch * me, nf, nch, we, me, s_ne, tid);
    for(int e = tid; e < nf * nch; e += kBpThreads) ((float*)(base + h.offset[A_EDC]))[I0 * nch + e] = r.edc[G0 * nch + e];
    // rows that keep their width: one wavefront per frame
    if(wave < nf) {
      const size_t g = G0 + wave, i = I0 + wave;
      wide_row((float*)(base + h.offset[A_PSD]) + i * np, r.psd + g * np, np, true, lane);
      wide_row((float*)(base + h.offset[A_PSDRES]) + i * np, r.psdres + g * np, np, s_res[wave] != 0, lane);
      if(ns > 0) wide_row((float*)(base + h.offset[A_VTMAGN]) + i * ns, r.vtmagn + g * ns, ns, s_nv[wave] > 0, lane);
    }
  }
}

int launch_blob_widths(LaunchCtx* P, const ModRows& r, const int* frm_off, const int* nfrm, int n, int* widths) {
  if(n <= 0) return 0;
  LAUNCH("k_blob_widths", k_blob_widths, dim3(n), dim3(256), 0, r, frm_off, nfrm, widths);
  return 0;
}

int launch_blob_pack(LaunchCtx* P, const ModRows& r, const BlobEntry* tab, const float* chanfreq, int n, int max_nfrm,
  unsigned char* stage) {
  if(n <= 0) return 0;
  const int groups = (max_nfrm + kBpFrames - 1) / kBpFrames + 1;
  LAUNCH("k_blob_pack", k_blob_pack, dim3(n, groups < 65535 ? groups : 65535), dim3(kBpThreads), 0, r, tab, chanfreq, stage);
  return 0;
}
