// 58-bit lossless copy of fp64 rows of at most 1024 columns: the format shared by the packer
// (pack58.hip), the packed gradient kernel (grad_dense_packed.hip) and the host tests
// (tests/pack58_host.cpp).  Plain C++: everything here compiles for the host and the device.
//
// A row is padded to 1024 columns and stored as one 7424-byte block (128-byte aligned).  Lane l of a
// wave owns the 16 columns it owns in grad_dense_multi at 16 columns per lane: value k = 2 j + v of
// the lane is column c = (j * 64 + l) * 2 + v.
//   low plane, 4096 B: the low 32 mantissa bits; four [64 lanes][4 dwords] blocks, block m holding
//     values 4 m .. 4 m + 3 of every lane (one 16-byte load per lane and block);
//   high plane, 3328 B: per lane 16 fields of 26 bits, little-endian in 13 dwords; three
//     [64 lanes][4 dwords] blocks (dwords 0-3, 4-7, 8-11) and one [64 lanes][1 dword] block (dword 12).
//   field = sign:1 | code:5 | mant_hi:20; code = biased exponent - E0 + 1 for exponents in
//     [E0, E0 + 30], code 0 = +-0.  E0 belongs to the segment.  Pad columns are code 0.
// Whatever the window does not hold (other exponents, denormals, inf, NaN) has no encoding: the
// packer compares every decoded value with its source and flags the bundle, which then reads the
// plain fp64 rows.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define P58_HD __host__ __device__ __forceinline__
#else
#define P58_HD inline
#endif

namespace eh {
namespace p58 {

constexpr int kCols = 1024;        // padded row width
constexpr int kVals = 16;          // values per lane
constexpr int kLanes = 64;
constexpr int kLowBytes = 4096;
constexpr int kHiDwords = 13;      // 16 * 26 bits per lane
constexpr int kRowBytes = 7424;    // 4096 + 3 * 1024 + 256
constexpr int kWindow = 31;        // binades a segment's codes 1..31 span
constexpr int kE0Min = 1, kE0Max = 2046 - (kWindow - 1);

// byte offset within a row of low-plane block m (0..3), high-plane 16-byte block m (0..2) and the
// last high dword, for lane l
P58_HD int low_off(int m, int lane) { return m * 1024 + lane * 16; }
P58_HD int high_off(int m, int lane) { return kLowBytes + m * 1024 + lane * 16; }
P58_HD int tail_off(int lane) { return kLowBytes + 3 * 1024 + lane * 4; }
// column of value k of lane l
P58_HD int column(int k, int lane) { return ((k >> 1) * kLanes + lane) * 2 + (k & 1); }

// The 26-bit field and low dword of a value.  A value without an encoding gets SOME field; decoding
// it does not give the value back, which is what the packer tests.
P58_HD void encode(uint64_t u, int e0, uint32_t* field, uint32_t* low) {
  const uint32_t hi = static_cast<uint32_t>(u >> 32);
  const uint32_t sign = hi >> 31, e = (hi >> 20) & 0x7FFu, mh = hi & 0xFFFFFu;
  const uint32_t code = e >= static_cast<uint32_t>(e0) && e <= static_cast<uint32_t>(e0 + kWindow - 1)
                            ? e - static_cast<uint32_t>(e0) + 1u
                            : 0u;
  *field = (sign << 25) | (code << 20) | (code ? mh : 0u);
  *low = code ? static_cast<uint32_t>(u) : 0u;
}

// The high dword of the double behind a field: rebase, sign by and-or, select for code 0.
P58_HD uint32_t decode_hi(uint32_t f, int e0) {
  const uint32_t mag = (f & 0x1FFFFFFu) + (static_cast<uint32_t>(e0 - 1) << 20);
  return ((f & 0x1F00000u) ? mag : 0u) | ((f << 6) & 0x80000000u);
}
P58_HD uint64_t decode(uint32_t f, uint32_t low, int e0) {
  return (static_cast<uint64_t>(decode_hi(f, e0)) << 32) | low;
}

// Field k (0..15) of a lane's 13 high dwords; k is a compile-time constant after unrolling, so this
// is one bit-field extract, or one funnel shift and a mask where the field straddles two dwords.
P58_HD uint32_t field_of(const uint32_t (&h)[kHiDwords], int k) {
  const int bit = 26 * k, w = bit >> 5, s = bit & 31;
  if (s + 26 <= 32) return (h[w] >> s) & 0x3FFFFFFu;
  return ((h[w] >> s) | (h[w + 1] << (32 - s))) & 0x3FFFFFFu;  // 6 < s < 32 here
}
// The 13 high dwords of a lane from its 16 fields.
P58_HD void fields_to_dwords(const uint32_t (&f)[kVals], uint32_t (&h)[kHiDwords]) {
#pragma unroll
  for (int w = 0; w < kHiDwords; ++w) h[w] = 0;
#pragma unroll
  for (int k = 0; k < kVals; ++k) {
    const int bit = 26 * k, w = bit >> 5, s = bit & 31;
    h[w] |= f[k] << s;
    if (s + 26 > 32) h[w + 1] |= f[k] >> (32 - s);
  }
}

// Host / reference form: one row of ld <= 1024 doubles (as bits) into its 7424-byte block; returns
// whether every value decodes to itself.  The device packer does the same per lane.
inline bool pack_row(const uint64_t* x, int ld, int e0, uint32_t* row /* kRowBytes / 4 dwords */) {
  bool exact = true;
  for (int lane = 0; lane < kLanes; ++lane) {
    uint32_t f[kVals], lo[kVals], h[kHiDwords];
    for (int k = 0; k < kVals; ++k) {
      const int c = column(k, lane);
      const uint64_t u = c < ld ? x[c] : 0;
      encode(u, e0, &f[k], &lo[k]);
      exact = exact && decode(f[k], lo[k], e0) == u;
    }
    fields_to_dwords(f, h);
    for (int k = 0; k < kVals; ++k) row[(low_off(k >> 2, lane) >> 2) + (k & 3)] = lo[k];
    for (int w = 0; w < 12; ++w) row[(high_off(w >> 2, lane) >> 2) + (w & 3)] = h[w];
    row[tail_off(lane) >> 2] = h[12];
  }
  return exact;
}
inline void unpack_row(const uint32_t* row, int ld, int e0, uint64_t* x) {
  for (int lane = 0; lane < kLanes; ++lane) {
    uint32_t h[kHiDwords];
    for (int w = 0; w < 12; ++w) h[w] = row[(high_off(w >> 2, lane) >> 2) + (w & 3)];
    h[12] = row[tail_off(lane) >> 2];
    for (int k = 0; k < kVals; ++k) {
      const int c = column(k, lane);
      if (c < ld) x[c] = decode(field_of(h, k), row[(low_off(k >> 2, lane) >> 2) + (k & 3)], e0);
    }
  }
}

}  // namespace p58

// What a packed dense plan adds to a gradient launch (grad_dense_packed.hip): the packed copy and
// window of every segment, and one flag per bundle of the plan's bundle table (1: stream the packed
// rows; 0: read the plain fp64 rows).
struct PackedRows {
  const void* const* rows = nullptr;  // [nseg] packed copy of the segment's partition, row r at r * 7424
  const int* e0 = nullptr;            // [nseg]
  const int* flags = nullptr;         // [nbundles]
};

}  // namespace eh
