// Plan-time packer of the 58-bit row copy (pack58.h): one wave per bundle of the plan's bundle table writes the
// packed rows of that bundle, decodes every value again from the dwords it is about to store and compares all 64
// bits with the source, and writes the bundle's flag: 1 = every value of every row of the bundle is exact.
// Nothing is trusted that was not compared.
#include <hip/hip_runtime.h>

#include "common.h"
#include "grad_dense.h"
#include "launchers.h"
#include "pack58.h"

using namespace eh;

namespace {

__global__ void __launch_bounds__(256)
pack58_bundles(const Segment* __restrict__ segs, const Task* __restrict__ tasks, int nbundles, int R,
               void* const* __restrict__ rows, const int* __restrict__ e0s, int* __restrict__ flags, int ld) {
  const int lane = threadIdx.x & 63;
  const int bundle = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (bundle >= nbundles) return;
  const Task lead = tasks[bundle * R];
  if (lead.seg < 0) {  // pad bundle of a folded workgroup: no rows
    if (lane == 0) flags[bundle] = 1;
    return;
  }
  const Segment ls = segs[lead.seg];
  const double* __restrict__ X = static_cast<const double*>(ls.X);
  unsigned char* __restrict__ P = static_cast<unsigned char*>(rows[lead.seg]);
  const int e0 = __builtin_amdgcn_readfirstlane(e0s[lead.seg]);
  const int rowbytes = ld * static_cast<int>(sizeof(double));
  bool exact = true;
  for (int r = lead.row_begin; r < lead.row_end; ++r) {
    const auto rs = make_rsrc(X + static_cast<long long>(r) * ld, rowbytes);  // zeros past the row's end: pad columns
    uint32_t f[p58::kVals], lo[p58::kVals], h[p58::kHiDwords];
    uint64_t u[p58::kVals];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const ulonglong2 v = buf_load16<ulonglong2, 0>(rs, (j * kWave + lane) * 16);
      u[2 * j] = v.x;
      u[2 * j + 1] = v.y;
    }
#pragma unroll
    for (int k = 0; k < p58::kVals; ++k) p58::encode(u[k], e0, &f[k], &lo[k]);
    p58::fields_to_dwords(f, h);
#pragma unroll
    for (int k = 0; k < p58::kVals; ++k) exact = exact && p58::decode(p58::field_of(h, k), lo[k], e0) == u[k];
    unsigned char* row = P + static_cast<long long>(r) * p58::kRowBytes;
#pragma unroll
    for (int m = 0; m < 4; ++m)
      *reinterpret_cast<uint4*>(row + p58::low_off(m, lane)) = make_uint4(lo[4 * m], lo[4 * m + 1], lo[4 * m + 2], lo[4 * m + 3]);
#pragma unroll
    for (int m = 0; m < 3; ++m)
      *reinterpret_cast<uint4*>(row + p58::high_off(m, lane)) = make_uint4(h[4 * m], h[4 * m + 1], h[4 * m + 2], h[4 * m + 3]);
    *reinterpret_cast<uint32_t*>(row + p58::tail_off(lane)) = h[12];
  }
  const int all = __all(exact ? 1 : 0);
  if (lane == 0) flags[bundle] = all ? 1 : 0;
}

}  // namespace

namespace eh {

hipError_t pack58_launch(const void* segs, const void* tasks, int ntasks, int R, void* const* rows, const int* e0,
                         int* flags, int ld, hipStream_t st) {
  if (R < 1 || ntasks < R || ntasks % R || ld <= 512 || ld > p58::kCols || ld % 2 || !rows || !e0 || !flags)
    return hipErrorInvalidValue;
  const int nb = ntasks / R;
  hipLaunchKernelGGL(pack58_bundles, dim3((nb + 3) / 4), dim3(256), 0, st, static_cast<const Segment*>(segs),
                     static_cast<const Task*>(tasks), nb, R, rows, e0, flags, ld);
  return hipGetLastError();
}

}  // namespace eh
