// wire_layout.h -- the byte layout of a chunk blob (format: wire.cpp), shared by the host serialiser (wire.cpp), the export
// of device-resident batches (batch_blob.cpp) and its pack kernel (blob_kernels.hip): array order, header, array sizes and
// offsets are defined here once.  Not installed.
#ifndef LLSM_AMD_WIRE_LAYOUT_H
#define LLSM_AMD_WIRE_LAYOUT_H
#include <cstddef>
#include <cstdint>

#ifdef __HIP__
#include <hip/hip_runtime.h>
#define LLSM_WIRE_FN __host__ __device__ inline
#else
#define LLSM_WIRE_FN inline
#endif

namespace llsm_wire {
enum { A_CHANFREQ, A_F0, A_NHAR, A_AMPL, A_PHSE, A_PSD, A_PSDRES, A_HASRES, A_EDC, A_NHAR_E, A_EAMP, A_EPHS, NARR1,
       A_RD = NARR1, A_HASRD, A_VTMAGN, A_VSPHSE, A_NVS, A_PBPSYN, A_HASHM, NARR };

struct Header {
  char magic[8];
  uint32_t version, header_bytes;
  int32_t nfrm, maxnhar, maxnhar_e, npsd, nchannel, nchanfreq;
  float thop, fnyq, lip_radius; int32_t nspec;
  uint64_t total_bytes;
  uint64_t offset[NARR];                               // version 1 blobs carry the first NARR1 entries only
};
static_assert(sizeof(Header) == 64 + 8 * NARR, "blob header has no padding");

LLSM_WIRE_FN size_t header_bytes_of(uint32_t version) { return sizeof(Header) - (version == 1 ? sizeof(uint64_t) * (NARR - NARR1) : 0); }
LLSM_WIRE_FN size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

struct Shape { int nfrm, maxnhar, me, npsd, nch, ncf, nspec = 0; float thop, fnyq, lip; const float* chanfreq; };

// byte sizes of the arrays, in blob order
LLSM_WIRE_FN void array_bytes(const Shape& s, size_t* b) {
  const size_t F = (size_t)s.nfrm, me = (size_t)(s.me > 0 ? s.me : 1);
  b[A_CHANFREQ] = sizeof(float) * (size_t)s.ncf;
  b[A_F0] = sizeof(float) * F; b[A_NHAR] = sizeof(int32_t) * F;
  b[A_AMPL] = b[A_PHSE] = sizeof(float) * F * (size_t)s.maxnhar;
  b[A_PSD] = b[A_PSDRES] = sizeof(float) * F * (size_t)s.npsd;
  b[A_HASRES] = sizeof(int32_t) * F;
  b[A_EDC] = sizeof(float) * F * (size_t)s.nch;
  b[A_NHAR_E] = sizeof(int32_t) * F;
  b[A_EAMP] = b[A_EPHS] = sizeof(float) * F * (size_t)s.nch * me;
  const size_t L1 = s.nspec > 0 ? 1 : 0;
  b[A_RD] = sizeof(float) * F * L1; b[A_HASRD] = b[A_NVS] = b[A_PBPSYN] = b[A_HASHM] = sizeof(int32_t) * F * L1;
  b[A_VTMAGN] = sizeof(float) * F * (size_t)s.nspec; b[A_VSPHSE] = sizeof(float) * F * (size_t)s.maxnhar * L1;
}

LLSM_WIRE_FN size_t layout(const Shape& s, uint64_t* off, uint32_t version = 2) {
  size_t b[NARR]; array_bytes(s, b);
  size_t at = pad8(header_bytes_of(version));
  const int narr = version == 1 ? NARR1 : NARR;
  for(int i = 0; i < narr; i ++) { if(off) off[i] = at; at += pad8(b[i]); }
  return at;
}

// the version-2 header of a blob of this shape, offsets included; returns total_bytes
LLSM_WIRE_FN size_t fill_header(const Shape& s, Header& h) {
  const char magic[8] = {'L', 'L', 'S', 'M', '2', 'L', '0', '\0'};
  unsigned char* z = (unsigned char*)& h;
  for(size_t i = 0; i < sizeof(Header); i ++) z[i] = 0;
  const size_t total = layout(s, h.offset);
  for(int i = 0; i < 8; i ++) h.magic[i] = magic[i];
  h.version = 2; h.header_bytes = (uint32_t)header_bytes_of(2); h.nspec = s.nspec;
  h.nfrm = s.nfrm; h.maxnhar = s.maxnhar; h.maxnhar_e = s.me; h.npsd = s.npsd; h.nchannel = s.nch;
  h.nchanfreq = s.ncf; h.thop = s.thop; h.fnyq = s.fnyq; h.lip_radius = s.lip; h.total_bytes = total;
  return total;
}

// One utterance of an export (batch_blob.cpp -> k_blob_pack): where its blob starts in the device staging area (a multiple
// of 16), the first of its frames in the batch's rows, and the blob's header as the kernel writes it out.
struct BlobEntry { uint64_t base; int32_t frm0, reserved; Header h; };
}  // namespace llsm_wire
#endif
