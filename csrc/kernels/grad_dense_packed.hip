// One-wave replica bundles over the 58-bit copy of fp64 rows (pack58.h): grad_dense_multi<double, double, 16, ...,
// FOLD> reading 7424 bytes per row instead of ld * 8.  X is constant for a training run, so the copy is made once
// at plan time (pack58.hip), which also decides per bundle whether the copy is exact: a bundle with flag 1 streams
// the packed rows, three in flight, and decodes each into the 16 doubles per lane that the plain kernel holds; a
// bundle with flag 0 runs the plain kernel's two-buffer loop on the fp64 rows.  The branch is wave-uniform.
// Everything after the row is in registers -- step (dot products, reductions, residual, gradient), the fold and
// the slab stores -- is grad_dense_multi's code, copied verbatim: the same operations on the same bits in the
// same order, so the slab rows are bit-identical to the plain kernel's.
#include <hip/hip_runtime.h>

#include "common.h"
#include "grad_dense.h"
#include "launchers.h"
#include "pack58.h"

using namespace eh;

namespace {

// Rows in flight per wave on the packed stream: the row in hand, decoded to 16 doubles per lane, and two raw rows
// of 29 dwords per lane behind it -- one more than the plain stream's two, because the decode lengthens the
// stretch in which a wave has only prefetches outstanding.  (2 and 4 measured within 1.3 % of it at the headline,
// inside the run-to-run drift: docs/PERF_NOTES.md, 58-bit rows.)
constexpr int kPackedDepth = 3;

struct RawRow {
  uint4 lo[4];  // low plane: values 4 m .. 4 m + 3
  uint4 hi[3];  // high plane: dwords 0-11 of the lane's 16 fields
  uint32_t tail;  // dword 12
};

template <int LOSS, int R, int EPI>
__global__ void __launch_bounds__(256)
grad_dense_p58(const Segment* __restrict__ segs, const Task* __restrict__ tasks, int nbundles,
               const double* __restrict__ beta, double* __restrict__ slab, int ld, const int* __restrict__ gate,
               long long* __restrict__ stamps, const PackedRows pk) {
  using T = double;
  using A = double;
  constexpr int CPL = 16;
  constexpr int VN = Vec16<T>::N;
  constexpr int NV = CPL / VN;
  using Rw = typename Vec16<T>::raw;
  if (gate_closed(gate)) return;  // launch-uniform: the fold's barrier is never half-reached
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bundle = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + wv);
  if (stamps && lane == 0) {
    stamps[4 * bundle] = wall_clock64();
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    stamps[4 * bundle + 3] = xcc;
  }
  const Task lead = tasks[bundle * R];
  const bool live = lead.seg >= 0;  // pad bundles: no rows, zero accumulators
  const Segment ls = segs[live ? lead.seg : 0];
  const T* __restrict__ X = static_cast<const T*>(ls.X);
  const A* __restrict__ Y = static_cast<const A*>(ls.y);
  A coef[R];
  bool act[R];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const Task tq = tasks[bundle * R + q];
    act[q] = tq.seg >= 0;
    coef[q] = act[q] ? static_cast<A>(segs[tq.seg].coef) : A(0);
  }
  A b[NV][VN], g[R][NV][VN];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c0 = (j * kWave + lane) * VN;
#pragma unroll
    for (int v = 0; v < VN; ++v) {
      b[j][v] = c0 < ld ? beta[c0 + v] : A(0);
#pragma unroll
      for (int q = 0; q < R; ++q) g[q][j][v] = A(0);
    }
  }
  const int rowbytes = ld * static_cast<int>(sizeof(T));
  const int r0 = lead.row_begin, r1 = live ? lead.row_end : r0;
  // (the label behind its row, through a descriptor: grad_dense_multi)
  const auto yrs = make_rsrc(Y + r0, (r1 - r0) * static_cast<int>(sizeof(A)));
  auto load = [&](Rw (&x)[NV], A& yv, int r) {
    const bool in = r < r1;
    const auto rs = make_rsrc(X + static_cast<long long>(in ? r : r0) * ld, in ? rowbytes : 0);
#pragma unroll
    for (int j = 0; j < NV; ++j) x[j] = buf_load16<Rw>(rs, (j * kWave + lane) * VN * static_cast<int>(sizeof(T)));
    yv = buf_load_scalar<A>(yrs, (r - r0) * static_cast<int>(sizeof(A)));
  };
  auto step = [&](const Rw (&x)[NV], const A y) {
    A z[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      z[q] = A(0);
      asm volatile("" : "+v"(z[q]));  // opaque start: R separate dot products, not one shared
    }
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int v = 0; v < VN; ++v)
#pragma unroll
        for (int q = 0; q < R; ++q) z[q] = fma(Vec16<T>::template elem<A>(x[j], v), b[j][v], z[q]);
    A rr[R];
    if constexpr (R == 1 || EPI == 0) {
#pragma unroll
      for (int q = 0; q < R; ++q) rr[q] = act[q] ? residual<LOSS, A>(wave_allreduce_sum(z[q]), y, coef[q]) : A(0);
    } else {
      static_assert(R <= 3, "one-wave bundles hold at most 3 replicas");
      const bool hi = lane >= 32;
      A c0 = coef[0], c1 = coef[1];
      asm volatile("" : "+v"(c0), "+v"(c1));
      A tq = wave_pair_reduce(z[0], z[1], hi), cq = hi ? c1 : c0;
      constexpr int kLane[3] = {0, 32, 1};
      if constexpr (R == 3) {
        const A z2 = wave_allreduce_sum(z[2]);
        if (lane == 1) {
          tq = z2;
          cq = coef[2];
        }
      }
      const A rl = residual_branchfree<LOSS, A>(tq, y, cq);
#pragma unroll
      for (int q = 0; q < R; ++q) rr[q] = act[q] ? readlane_a(rl, kLane[q]) : A(0);
    }
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int v = 0; v < VN; ++v)
#pragma unroll
        for (int q = 0; q < R; ++q) g[q][j][v] = fma(rr[q], Vec16<T>::template elem<A>(x[j], v), g[q][j][v]);
  };
  const int packed = live ? __builtin_amdgcn_readfirstlane(pk.flags[bundle]) : 0;
  if (packed) {
    // (read through a pointer table: made wave-uniform by hand, or every load's descriptor goes through a
    // per-lane waterfall loop)
    const unsigned long long pa = reinterpret_cast<unsigned long long>(pk.rows[lead.seg]);
    const unsigned char* __restrict__ P = reinterpret_cast<const unsigned char*>(
        (static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(static_cast<unsigned>(pa >> 32))) << 32) |
        static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<unsigned>(pa))));
    const int e0 = __builtin_amdgcn_readfirstlane(pk.e0[lead.seg]);
    // A packed row is one 7424-byte block: seven 16-byte loads and one dword per lane, each a run of whole
    // cache lines across the wave; a row past the bundle gets a zero-size descriptor, as above.
    auto loadp = [&](RawRow& w, A& yv, int r) {
      const bool in = r < r1;
      const auto rs = make_rsrc(P + static_cast<long long>(in ? r : r0) * p58::kRowBytes, in ? p58::kRowBytes : 0);
#pragma unroll
      for (int m = 0; m < 4; ++m) w.lo[m] = buf_load16<uint4>(rs, p58::low_off(m, lane));
#pragma unroll
      for (int m = 0; m < 3; ++m) w.hi[m] = buf_load16<uint4>(rs, p58::high_off(m, lane));
      w.tail = __builtin_amdgcn_raw_buffer_load_b32(rs, p58::tail_off(lane), 0, kStreamAux);
      yv = buf_load_scalar<A>(yrs, (r - r0) * static_cast<int>(sizeof(A)));
    };
    auto decode = [&](const RawRow& w, Rw (&x)[NV]) {
      uint32_t h[p58::kHiDwords], lo[p58::kVals];
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        h[4 * m] = w.hi[m].x;
        h[4 * m + 1] = w.hi[m].y;
        h[4 * m + 2] = w.hi[m].z;
        h[4 * m + 3] = w.hi[m].w;
      }
      h[12] = w.tail;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        lo[4 * m] = w.lo[m].x;
        lo[4 * m + 1] = w.lo[m].y;
        lo[4 * m + 2] = w.lo[m].z;
        lo[4 * m + 3] = w.lo[m].w;
      }
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        x[j].x = __longlong_as_double(static_cast<long long>(p58::decode(p58::field_of(h, 2 * j), lo[2 * j], e0)));
        x[j].y = __longlong_as_double(
            static_cast<long long>(p58::decode(p58::field_of(h, 2 * j + 1), lo[2 * j + 1], e0)));
      }
    };
    constexpr int D = kPackedDepth;
    RawRow xr[D - 1];
    A yr[D - 1];
    Rw x[NV];
    // A row is decoded into x[] as soon as it has landed, and its raw buffer is loaded again at once: while a
    // row is computed from x[], the D - 1 rows behind it are in flight, D rows counting the one in hand.
    // Whole trips of D - 1 rows, then the rows left, which the last loads already hold: a trip has no way out
    // in its middle, so the buffers are the same registers at its end as at its start (with a break per row
    // the compiler copied rows still in flight at the loop's end, i.e. waited for them).
#pragma unroll
    for (int k = 0; k < D - 1; ++k) loadp(xr[k], yr[k], r0 + k);
    int r = r0;
    for (; r + D - 1 <= r1; r += D - 1) {
#pragma unroll
      for (int k = 0; k < D - 1; ++k) {
        decode(xr[k], x);
        const A y = yr[k];
        loadp(xr[k], yr[k], r + k + D - 1);
        step(x, y);
      }
    }
#pragma unroll
    for (int k = 0; k < D - 2; ++k) {
      if (r + k >= r1) break;
      decode(xr[k], x);
      step(x, yr[k]);
    }
  } else {
    Rw xa[NV], xb[NV];
    A ya = A(0), yb = A(0);
    load(xa, ya, r0);
    for (int r = r0; r < r1; r += 2) {  // two rows per trip: the buffers swap roles without copies
      load(xb, yb, r + 1);
      step(xa, ya);
      if (r + 1 >= r1) break;
      load(xa, ya, r + 2);
      step(xb, yb);
    }
  }
  if (stamps && lane == 0) stamps[4 * bundle + 1] = wall_clock64();
  {
    extern __shared__ __attribute__((aligned(16))) unsigned char fold_raw[];
    A* fb = reinterpret_cast<A*>(fold_raw);  // [3 waves][R][NV * VN][64 lanes]
    if (wv > 0) {
#pragma unroll
      for (int q = 0; q < R; ++q)
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
          for (int v = 0; v < VN; ++v) fb[((((wv - 1) * R + q) * NV + j) * VN + v) * kWave + lane] = g[q][j][v];
    }
    __syncthreads();
    if (wv > 0) return;
#pragma unroll 1
    for (int k = 0; k < 3; ++k)  // one wave's rows at a time: keeps the epilogue's registers low
#pragma unroll
      for (int q = 0; q < R; ++q)
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
          for (int v = 0; v < VN; ++v) g[q][j][v] += fb[(((k * R + q) * NV + j) * VN + v) * kWave + lane];
  }
#pragma unroll
  for (int q = 0; q < R; ++q) {
    if (!act[q]) continue;
    A* out = slab + static_cast<long long>(tasks[bundle * R + q].slab) * ld;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c0 = (j * kWave + lane) * VN;
#pragma unroll
      for (int v = 0; v < VN; ++v)
        if (c0 + v < ld) out[c0 + v] = g[q][j][v];
    }
  }
  if (stamps) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) stamps[4 * bundle + 2] = wall_clock64();
  }
}

template <int LOSS, int R>
hipError_t launch_p58(bool lane_epi, int nb, hipStream_t st, const Segment* segs, const Task* tasks, const double* beta,
                      double* slab, int ld, const int* gate, long long* stamps, const PackedRows& pk) {
  constexpr size_t lds = 3ull * R * 16 * kWave * sizeof(double);
  auto kern = lane_epi ? grad_dense_p58<LOSS, R, 1> : grad_dense_p58<LOSS, R, 0>;
  if (const hipError_t e = allow_dynamic_lds(kern, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(nb / 4), dim3(256), lds, st, segs, tasks, nb, beta, slab, ld, gate, stamps, pk);
  return hipGetLastError();
}

}  // namespace

namespace eh {

hipError_t grad_dense_packed_launch(int loss, const void* segs, const void* tasks, int ntasks, const void* beta,
                                    void* slab, int ld, hipStream_t st, const KernelChoice& k, const PackedRows& pk,
                                    const int* gate, long long* stamps) {
  const int R = k.replicas;
  if (k.kind != kGradMulti || !k.fold || k.pair || R < 1 || R > 3 || ntasks % R || (ntasks / R) % 4 || ld <= 512 ||
      ld > p58::kCols || !pk.rows || !pk.e0 || !pk.flags)
    return hipErrorInvalidValue;
  const Segment* S = static_cast<const Segment*>(segs);
  const Task* Tk = static_cast<const Task*>(tasks);
  const double* B = static_cast<const double*>(beta);
  double* Sl = static_cast<double*>(slab);
  const int nb = ntasks / R;
  const bool le = k.lane_epi != 0;
  return dispatch_loss(loss, [&](auto L) {
    constexpr int LS = decltype(L)::value;
    if (R == 1) return launch_p58<LS, 1>(le, nb, st, S, Tk, B, Sl, ld, gate, stamps, pk);
    if (R == 2) return launch_p58<LS, 2>(le, nb, st, S, Tk, B, Sl, ld, gate, stamps, pk);
    return launch_p58<LS, 3>(le, nb, st, S, Tk, B, Sl, ld, gate, stamps, pk);
  });
}

}  // namespace eh
