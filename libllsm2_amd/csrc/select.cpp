// select.cpp -- unit selection on the device: host side of select_kernels.hip.
//
//   llsm_gpu_select_default_options  the defaults of llsm_gpu.h
//   llsm_gpu_select_check            host only: every refusal that needs no batch beyond the orders of its coder
//   llsm_gpu_batch_select            LLSM_GPU_CODE of a target batch and of a bank -> for every target frame the bank frame
//                                    that renders it, as splice takes it, and the path cost per utterance (rules S1 - S5:
//                                    llsm_gpu.h): the eight nearest bank frames of every target frame
//                                    (k_select_knn per bank segment, k_select_merge), the join costs between the candidates
//                                    of neighbouring frames (k_select_join), one path per utterance (k_select_path), one
//                                    copy back
//   llsm_gpu_batch_select_chain      the same inputs and outputs under rules C1 - C6: the same near lists, then followers,
//                                    joins and the path of every utterance in one kernel (k_select_chain)
//
// Every check runs before anything is allocated, copied or launched.  The scratch lives on batch t, grow-only.  The
// utterance tables of both batches (frame offsets, frame counts, frame -> utterance) are on the device since the batches
// were made, so the call uploads nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "batch.h"

namespace {
const char* kSelect = "llsm_gpu_batch_select";
const char* kChain = "llsm_gpu_batch_select_chain";
const long long kMaxBank = 1ll << 24;             // planes 7 and 10 keep frame indices as floats

// every message starts with the name of the call that refuses
int refuse(const char* who, const std::string& why) { llsm_set_error(std::string(who) + ": " + why); return -1; }

// the options checked against a coder of these orders, count resolved; -1 with the error set
int check(const char* who, llsm_gpu_select_options* o, int order_spec, int order_bap) {
  if(order_spec < 1 || order_bap < 1) return refuse(who, "the coder is not enabled");
  const int dim = order_spec + order_bap + 3;
  if(o -> count <= 0) o -> count = order_spec;
  if(o -> first < 0 || o -> first >= dim || o -> count > dim - o -> first)
    return refuse(who, "columns [" + std::to_string(o -> first) + ", " + std::to_string((long long)o -> first + o -> count) +
      ") lie outside [0, " + std::to_string(dim) + ")");
  if(std::isnan(o -> voicing_cost) || std::isnan(o -> join_cost)) return refuse(who, "a cost is NaN");
  if(std::isnan(o -> join_weight)) return refuse(who, "join_weight is NaN");
  if(std::isinf(o -> voicing_cost) || std::isinf(o -> join_cost)) return refuse(who, "a cost is infinite");
  if(std::isinf(o -> join_weight)) return refuse(who, "join_weight is infinite");
  if(o -> voicing_cost < 0) return refuse(who, "voicing_cost < 0");
  if(o -> join_cost < 0) return refuse(who, "join_cost < 0");
  if(o -> join_weight < 0) return refuse(who, "join_weight < 0");
  if(o -> skip_own_utterance != 0 && o -> skip_own_utterance != 1)
    return refuse(who, "skip_own_utterance is " + std::to_string(o -> skip_own_utterance) + ", not 0 or 1");
  return 0;
}

// Every check of llsm_gpu_batch_select and llsm_gpu_batch_select_chain, before anything is allocated, copied or launched:
// -1 refused (the error set, nothing written); 0 a t without frames (the costs filled with 0: the call is done); 1
// accepted, with d filled but for the segment rule's buffers
int accept(const char* who, llsm_gpu_batch* t, const llsm_gpu_batch* bank, const llsm_gpu_select_options* opt,
  int* utt, FP_TYPE* pos, FP_TYPE* cost, SelectDev& d) {
  if(! t || ! bank) return refuse(who, "NULL batch");
  if(t -> ctx != bank -> ctx) return refuse(who, "the batches belong to different contexts");
  if(t -> coder_os == 0 || bank -> coder_os == 0) return refuse(who, "the coder is not enabled on both batches");
  if(t -> coder_os + t -> coder_ob != bank -> coder_os + bank -> coder_ob)
    return refuse(who, "the coder dimensions differ: " + std::to_string(t -> coder_os + t -> coder_ob + 3) + " and " +
      std::to_string(bank -> coder_os + bank -> coder_ob + 3));
  llsm_gpu_select_options o;
  if(opt) o = *opt; else llsm_gpu_select_default_options(& o);
  if(check(who, & o, t -> coder_os, t -> coder_ob)) return -1;
  if(o.skip_own_utterance && t != bank) return refuse(who, "skip_own_utterance needs t == bank");
  const long long nt = t -> lay.total_frames, nb = bank -> lay.total_frames;
  const int n_utt = t -> lay.n_utt;
  if(nt == 0) {                                                     // nothing to select: every cost is 0
    if(cost) std::fill(cost, cost + n_utt, (FP_TYPE)0);
    return 0;
  }
  if(! utt) return refuse(who, "NULL utt");
  if(! pos) return refuse(who, "NULL pos");
  if(nb == 0) return refuse(who, "the bank has no frames");
  if(nb > kMaxBank) return refuse(who, "the bank holds " + std::to_string(nb) + " frames, more than 2^24 = " + std::to_string(kMaxBank));
  if(o.skip_own_utterance)
    for(int u = 0; u < n_utt; u ++)
      if(t -> nfrm[u] > 0 && nb - t -> nfrm[u] <= 0)
        return refuse(who, "skip_own_utterance leaves utterance " + std::to_string(u) + " without a bank frame");
  d.code_t = (const float*)t -> arr[LLSM_GPU_CODE]; d.code_b = (const float*)bank -> arr[LLSM_GPU_CODE];
  d.dim = t -> coder_os + t -> coder_ob + 3; d.first = o.first; d.count = o.count;
  d.voicing_cost = o.voicing_cost; d.join_cost = o.join_cost; d.join_weight = o.join_weight; d.skip_own = o.skip_own_utterance;
  d.nt = (int)nt; d.nb = (int)nb; d.n_utt = n_utt;
  d.t_frm_off = t -> d_frm_off.p; d.t_nfrm = t -> d_nfrm.p; d.t_frm_utt = t -> d_frm_utt.p;
  d.b_frm_off = bank -> d_frm_off.p; d.b_nfrm = bank -> d_nfrm.p; d.b_frm_utt = bank -> d_frm_utt.p;
  d.seg_len = select_seg_len(d.nb); d.n_seg = select_segments(d.nb);
  return 1;
}

// the device block [utt | pos | cost] into memory of our own first, so that a failed copy leaves the three arrays untouched
int fetch(LaunchCtx* P, const SelectDev& d, const int* out, int* utt, FP_TYPE* pos, FP_TYPE* cost) {
  const size_t nt = (size_t)d.nt, n_out = 2 * nt + (size_t)d.n_utt;
  std::vector<int> host(n_out);
  HIP_OK(hipMemcpyAsync(host.data(), out, n_out * sizeof(int), hipMemcpyDeviceToHost, P -> stream));
  HIP_OK(hipStreamSynchronize(P -> stream));
  std::copy(host.begin(), host.begin() + nt, utt);
  const float* fh = (const float*)host.data();
  std::copy(fh + nt, fh + 2 * nt, pos);
  if(cost) std::copy(fh + 2 * nt, fh + n_out, cost);
  return 0;
}
}  // namespace

extern "C" void llsm_gpu_select_default_options(llsm_gpu_select_options* dst) {
  if(! dst) return;
  dst -> first = 3; dst -> count = 0; dst -> voicing_cost = 0; dst -> join_cost = 0; dst -> join_weight = 1;
  dst -> skip_own_utterance = 0;
}

extern "C" int llsm_gpu_select_check(const llsm_gpu_select_options* opt, int order_spec, int order_bap) {
  llsm_gpu_select_options o;
  if(opt) o = *opt; else llsm_gpu_select_default_options(& o);
  return check(kSelect, & o, order_spec, order_bap);
}

extern "C" int llsm_gpu_batch_select(llsm_gpu_batch* t, const llsm_gpu_batch* bank, const llsm_gpu_select_options* opt,
  int* utt, FP_TYPE* pos, FP_TYPE* cost) {
  SelectDev d;
  const int go = accept(kSelect, t, bank, opt, utt, pos, cost, d);
  if(go <= 0) return go;
  // accepted: from here on t's scratch changes
  hipSetDevice(t -> ctx -> device);
  const size_t nt = (size_t)d.nt, n_out = 2 * nt + (size_t)d.n_utt;
  t -> sel_frames = 0;                    // from here on the planes of an earlier call may be gone (a buffer that grows is
                                          // freed first): they are readable again once this call has succeeded
  if((d.n_seg > 1 && t -> sel_lists.alloc((size_t)d.n_seg * nt * 16)) || t -> sel_p7.alloc(nt * 16) ||
     t -> sel_p8.alloc(nt * 64) || t -> sel_bp.alloc(nt) || t -> sel_out.alloc(n_out)) return -1;
  LaunchCtx* P = & t -> ctx -> lc;
  int rc = launch_select_knn(P, d, d.n_seg > 1 ? t -> sel_lists.p : t -> sel_p7.p);
  if(! rc && d.n_seg > 1) rc = launch_select_merge(P, d, t -> sel_lists.p, t -> sel_p7.p);
  if(! rc) rc = launch_select_join(P, d, t -> sel_p7.p, t -> sel_p8.p);
  if(! rc) rc = launch_select_path(P, d, t -> sel_p7.p, t -> sel_p8.p, t -> sel_bp.p, t -> sel_out.p);
  if(rc) return refuse(kSelect, std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
  if(fetch(P, d, t -> sel_out.p, utt, pos, cost)) return -1;
  t -> sel_frames = (long long)nt;
  return 0;
}

// Rules C1 - C6 (llsm_gpu.h).  The near lists are those of llsm_gpu_batch_select, by the same two
// kernels, in a buffer of this call's own; followers, joins and the path are one kernel, k_select_chain.  The scratch is
// the selc_* set of batch t: planes 7 and 8 stay what the last llsm_gpu_batch_select left.
extern "C" int llsm_gpu_batch_select_chain(llsm_gpu_batch* t, const llsm_gpu_batch* bank, const llsm_gpu_select_options* opt,
  int* utt, FP_TYPE* pos, FP_TYPE* cost) {
  SelectDev d;
  const int go = accept(kChain, t, bank, opt, utt, pos, cost, d);
  if(go <= 0) return go;
  hipSetDevice(t -> ctx -> device);
  const size_t nt = (size_t)d.nt, n_out = 2 * nt + (size_t)d.n_utt;
  t -> selc_frames = 0;                   // planes 10 and 11 are readable again once this call has succeeded
  if((d.n_seg > 1 && t -> selc_lists.alloc((size_t)d.n_seg * nt * 16)) || t -> selc_near.alloc(nt * 16) ||
     t -> selc_p10.alloc(nt * 32) || t -> selc_p11.alloc(nt * 256) || t -> selc_bp.alloc(nt) || t -> selc_out.alloc(n_out)) return -1;
  LaunchCtx* P = & t -> ctx -> lc;
  int rc = launch_select_knn(P, d, d.n_seg > 1 ? t -> selc_lists.p : t -> selc_near.p);
  if(! rc && d.n_seg > 1) rc = launch_select_merge(P, d, t -> selc_lists.p, t -> selc_near.p);
  if(! rc) rc = launch_select_chain(P, d, t -> selc_near.p, t -> selc_p10.p, t -> selc_p11.p, t -> selc_bp.p, t -> selc_out.p);
  if(rc) return refuse(kChain, std::string("launch failed: ") + hipGetErrorString((hipError_t)rc));
  if(fetch(P, d, t -> selc_out.p, utt, pos, cost)) return -1;
  t -> selc_frames = (long long)nt;
  return 0;
}
