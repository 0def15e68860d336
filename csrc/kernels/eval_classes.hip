// Multi-class evaluation GEMM on MFMA: loss and accuracy of every round fused into the epilogue.
//
// For the rows X [n, ldx], labels y [n] (class indices held in the accumulator type) and the stored models
// B [R * C, ldb] (round-major, the class inside: ModelSpec.rows(betaset)) it adds, per round r,
//   loss[r] += sum_i l(z_i, y_i)    and    hits[r] += #{i : y_i == argmax_k z_ik, first index on ties},
// z_ik = X_i . B[r * C + k], without ever storing a logit:
//   mode 0 (softmax)                 l = log sum_k exp(z_k - max z) + max z - z_y
//   mode 1 / 2 (one-vs-rest)         l = sum_k loss_value(y_k z_k), y_k = +1 for the row's class, -1 for the others,
//                                    loss_value the logistic / squared-hinge loss of common.h
// The products run on v_mfma_f64_16x16x4_f64 (storage codes 0 and 3) or v_mfma_f32_16x16x4_f32 (code 1), the
// epilogue in fp64 from the accumulator values.
//
// Class groups on the fragment.  eval.hip puts the X rows on the MFMA's M side, which spreads a round's C logits
// over neighbouring lanes.  Here the model rows are the M side and the X rows the N side: lane (g = lane >> 4,
// i = lane & 15) of a 16 x 16 tile then holds, in its four accumulator registers, four model rows of ONE data row i.
// The f32 instruction gives a lane the rows 4 g + reg; the f64 instruction gives it g + 4 reg, so the f64 A operand
// is read from LDS through the permutation m -> 4 (m & 3) + (m >> 2) and every lane holds the STAGED columns
// 4 g .. 4 g + 3 in both types.  A round is padded to CP = 2, 4 or 8 staged columns while B goes into LDS (staged
// column j is B[(j / CP) C + j % CP] where j % CP < C and zeros elsewhere; no padded copy exists in memory), so a
// class group is
//   CP = 2   half a lane: two rounds per lane,
//   CP = 4   exactly one lane's registers,
//   CP = 8   the lanes g = 2 q and 2 q + 1, 16 apart: they exchange their partial maxima (and, for softmax, their
//            partial sums of exponentials) with v_permlane16_swap; each adds its own share of the row's loss.
// Padding columns are left out of the max, the sum and the argmax by selects.  MFMA columns wasted on padding:
// C = 3: 1 of 4 (25 %), C = 5: 3 of 8 (37.5 %), C = 6: 2 of 8 (25 %), C = 7: 1 of 8 (12.5 %); C = 2, 4, 8: none.
//
// Tiling (eval.hip's v2): 256 threads = 4 waves; a workgroup multiplies kRows = 128 data rows (32 per wave, two
// n-tiles) with kCols = 112 staged columns (7 m-tiles, kCols / CP rounds): 14 independent accumulators per wave,
// every model fragment read from LDS feeds two MFMAs.  K goes through LDS in 32-deep tiles (row stride padded to 34),
// the next K tile is fetched into registers while the current one is multiplied: 16-byte loads where the rows are
// 16-byte aligned, element loads with the same bounds where they are not.
//
// Reduction: a lane's loss and hit of one (row, round) are summed over the 16 lanes of its row group (DPP), then over
// the wave's two row tiles, then over the four waves through LDS in wave order; one fp64 atomicAdd per round per
// workgroup goes to loss and to hits (hits are small integers: exact).
//
// A label that is no integer in 0 .. C - 1 adds NaN to the row's loss in every round and never hits; z_y is a select
// over the classes, never an index.  A NaN logit reaches the loss through the sum.
#include <cstdint>
#include <cstdlib>

#include "common.h"
#include "launchers.h"

namespace eh {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// D = A B + C with A [16 model columns][4 k] and B [4 k][16 data rows]; lane (g, i) supplies A[m_of(i)][g] and
// B[g][i] and receives the staged columns 4 g + reg of data row i.
template <typename A> struct ClassMfma;
template <> struct ClassMfma<double> {
  using acc = f64x4;
  __device__ __forceinline__ static acc mma(double a, double b, acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // D row of (lane, reg) is g + 4 reg: feed row m from staged column 4 (m & 3) + (m >> 2)
  __device__ __forceinline__ static int m_of(int m) { return 4 * (m & 3) + (m >> 2); }
};
template <> struct ClassMfma<float> {
  using acc = f32x4;
  __device__ __forceinline__ static acc mma(float a, float b, acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  __device__ __forceinline__ static int m_of(int m) { return m; }  // D row of (lane, reg) is 4 g + reg
};

template <typename T, typename A>
__device__ __forceinline__ A widen(const T* p) { return static_cast<A>(*p); }

constexpr int kKT = 32;       // K tile
constexpr int kKS = 34;       // padded LDS row stride (elements)
constexpr int kRows = kEvalClassRows;       // data rows per workgroup
constexpr int kNT = kEvalClassCols / 16;    // 16-column m-tiles per workgroup

// Sum over the 16 lanes of a row group (lanes 16 g .. 16 g + 15); every lane of the group ends with the total.
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror
  return v;
}

// One lane's share of a class group: NL logits z of the classes c0 .. c0 + NL - 1 (those >= C are padding) of one
// data row with label yl.  PAIR: the group is shared with lane ^ 16 (CP = 8; hi = this is the upper lane, which
// holds classes 4 .. 7).  Adds the lane's share of the row's loss and hit.
template <int NL, int MODE, bool PAIR>
__device__ __forceinline__ void class_group(const double* z, int c0, int C, double yl, bool label_ok, bool hi,
                                            double& loss, double& hit) {
  // local maximum and its first index; class c0 itself is never padding
  double m = z[0];
  int a = 0;
#pragma unroll
  for (int k = 1; k < NL; ++k) {
    const bool gt = c0 + k < C && z[k] > m;
    m = gt ? z[k] : m;
    a = gt ? k : a;
  }
  bool win = true;
  if constexpr (PAIR) {
    const double mo = partner16(m, hi);
    win = hi ? m > mo : !(mo > m);  // the upper lane's maximum counts only when it is strictly larger
    m = win ? m : mo;
  }
  hit = (win && yl == static_cast<double>(c0 + a)) ? 1.0 : 0.0;
  const bool owner = !PAIR || !hi;  // the lane that adds what belongs to the group as a whole
  double v = 0.0;
  if constexpr (MODE == 0) {
    double s = 0.0, zy = 0.0;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const bool ok = c0 + k < C;
      s += ok ? exp(z[k] - m) : 0.0;
      zy = (ok && yl == static_cast<double>(c0 + k)) ? z[k] : zy;
    }
    if constexpr (PAIR) {
      const double so = partner16(s, hi);
      s = hi ? so + s : s + so;
    }
    v = (owner ? log(s) + m : 0.0) - zy;
  } else {
    constexpr int L = MODE == 1 ? kLogistic : kSquaredHinge;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const double yk = yl == static_cast<double>(c0 + k) ? 1.0 : -1.0;
      v += c0 + k < C ? loss_value<L>(yk, z[k]) : 0.0;
    }
  }
  loss = (owner && !label_ok) ? __builtin_nan("") : v;
}

template <typename T, typename A, int CP, int MODE>
__global__ void __launch_bounds__(256, 2)
eval_class_loss(const T* __restrict__ X, long long ldx, long long n, int d, const A* __restrict__ y,
                const A* __restrict__ B, int ldb, int R, int C, int vec, double* __restrict__ loss,
                double* __restrict__ hits) {
  using M = ClassMfma<A>;
  constexpr int NT = kNT;
  constexpr int NB = 16 * NT;
  constexpr int XV = Vec16<T>::N;
  constexpr int BV = Vec16<A>::N;
  constexpr int SUBS = CP == 2 ? 2 : 1;      // class groups per lane and tile
  constexpr int NL = CP == 2 ? 2 : 4;        // logits of a group in one lane
  constexpr int LPR = CP == 8 ? 2 : 1;       // row groups (lanes 16 apart) that share a round
  constexpr int SLOTS = NT * 4 * SUBS;       // (tile, row group, sub) sums of a wave; slot / LPR = the round
  __shared__ A Xs[kRows * kKS];
  __shared__ A Bs[NB * kKS];
  __shared__ double red[2][4][SLOTS];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long row0 = static_cast<long long>(blockIdx.x) * kRows;
  const int rnd0 = blockIdx.y * (NB / CP);  // first round of this workgroup
  // staging: thread -> (data row or staged column tid / 2, 16 consecutive k starting at (tid & 1) * 16)
  const int sr = tid >> 1, sk = (tid & 1) * 16;
  const bool xok = row0 + sr < n;
  const T* __restrict__ xrow = X + (xok ? row0 + sr : 0) * ldx;
  const int brnd = rnd0 + sr / CP, bcls = sr % CP;
  const bool bok = sr < NB && brnd < R && bcls < C;
  const A* __restrict__ brow = B + (bok ? static_cast<long long>(brnd) * C + bcls : 0) * ldb;

  A xr[16], br[16];
  auto fetch = [&](int k0) {
    if (vec) {
#pragma unroll
      for (int v = 0; v < 16 / XV; ++v) {
        const int gk = k0 + sk + v * XV;
        A t[XV];
        if (xok && gk < ldx) {
          Vec16<T>::load(xrow + gk, t);
        } else {
#pragma unroll
          for (int e = 0; e < XV; ++e) t[e] = A(0);
        }
#pragma unroll
        for (int e = 0; e < XV; ++e) xr[v * XV + e] = gk + e < d ? t[e] : A(0);
      }
#pragma unroll
      for (int v = 0; v < 16 / BV; ++v) {
        const int gk = k0 + sk + v * BV;
        A t[BV];
        if (bok && gk < ldb) {
          Vec16<A>::load(brow + gk, t);
        } else {
#pragma unroll
          for (int e = 0; e < BV; ++e) t[e] = A(0);
        }
#pragma unroll
        for (int e = 0; e < BV; ++e) br[v * BV + e] = gk + e < d ? t[e] : A(0);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int gk = k0 + sk + e;
        xr[e] = (xok && gk < d) ? widen<T, A>(xrow + gk) : A(0);
        br[e] = (bok && gk < d) ? brow[gk] : A(0);
      }
    }
  };

  typename M::acc acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[m][t] = typename M::acc{0, 0, 0, 0};

  const int fr = lane & 15, g = lane >> 4, fm = M::m_of(fr);
  fetch(0);
  for (int k0 = 0; k0 < d; k0 += kKT) {
    __syncthreads();  // the previous tile's MFMA reads are done
#pragma unroll
    for (int e = 0; e < 16; ++e) Xs[sr * kKS + sk + e] = xr[e];
    if (sr < NB) {
#pragma unroll
      for (int e = 0; e < 16; ++e) Bs[sr * kKS + sk + e] = br[e];
    }
    __syncthreads();
    if (k0 + kKT < d) fetch(k0 + kKT);  // in flight while this tile is multiplied
#pragma unroll
    for (int ks = 0; ks < kKT; ks += 4) {
      const int fk = ks + g;
      const A x0 = Xs[(wid * 32 + fr) * kKS + fk];
      const A x1 = Xs[(wid * 32 + 16 + fr) * kKS + fk];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const A b = Bs[(t * 16 + fm) * kKS + fk];
        acc[0][t] = M::mma(b, x0, acc[0][t]);
        acc[1][t] = M::mma(b, x1, acc[1][t]);
      }
    }
  }

  // Epilogue.  Lane (g, fr) holds the staged columns t * 16 + 4 g + reg of the data rows row0 + wid * 32 + m * 16 + fr.
  double yl[2];
  bool rok[2], lok[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const long long gr = row0 + wid * 32 + m * 16 + fr;
    rok[m] = gr < n;
    yl[m] = rok[m] ? static_cast<double>(y[gr]) : 0.0;
    lok[m] = yl[m] >= 0.0 && yl[m] < static_cast<double>(C) && yl[m] == floor(yl[m]);
  }
  const bool hi = CP == 8 && (g & 1);
  const int c0 = hi ? 4 : 0;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int s = 0; s < SUBS; ++s) {
      const int slot = (t * 4 + g) * SUBS + s;
      const bool cok = rnd0 + slot / LPR < R;
      double ls = 0.0, hs = 0.0;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        double z[NL];
#pragma unroll
        for (int k = 0; k < NL; ++k) z[k] = static_cast<double>(acc[m][t][s * NL + k]);
        double l, h;
        class_group<NL, MODE, CP == 8>(z, c0, C, yl[m], lok[m], hi, l, h);
        const bool use = cok && rok[m];
        ls += row16_sum(use ? l : 0.0);
        hs += row16_sum(use ? h : 0.0);
      }
      if (fr == 0) {
        red[0][wid][slot] = ls;
        red[1][wid][slot] = hs;
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < NB / CP; j += 256) {
    if (rnd0 + j >= R) continue;
    double ls = 0.0, hs = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int q = 0; q < LPR; ++q) {
        ls += red[0][w][j * LPR + q];
        hs += red[1][w][j * LPR + q];
      }
    atomicAdd(loss + rnd0 + j, ls);
    atomicAdd(hits + rnd0 + j, hs);
  }
}

template <typename T, typename A, int CP>
hipError_t launch_mode(int mode, dim3 grid, hipStream_t st, const void* X, long long ldx, long long n, int d,
                       const void* y, const void* B, int ldb, int R, int C, int vec, double* loss, double* hits) {
#define EH_CLASSES(MODE)                                                                                          \
  hipLaunchKernelGGL((eval_class_loss<T, A, CP, MODE>), grid, dim3(256), 0, st, (const T*)X, ldx, n, d, (const A*)y, \
                     (const A*)B, ldb, R, C, vec, loss, hits)
  if (mode == 0) EH_CLASSES(0);
  else if (mode == 1) EH_CLASSES(1);
  else EH_CLASSES(2);
#undef EH_CLASSES
  return hipGetLastError();
}

}  // namespace

hipError_t eval_classes_launch(int x_dtype, int mode, const void* X, long long ldx, long long n, int d, const void* y,
                               const void* B, int ldb, int R, int C, double* loss, double* hits, hipStream_t st) {
  if (x_dtype != 0 && x_dtype != 1 && x_dtype != 3) return hipErrorInvalidValue;
  if (mode < 0 || mode > 2 || C < kMinBlocks || C > kMaxBlocks) return hipErrorInvalidValue;
  if (n < 0 || R < 0 || d < 0 || d > ldx || d > ldb) return hipErrorInvalidValue;
  if (n == 0 || R == 0) return hipSuccess;
  const int cp = C <= 2 ? 2 : C <= 4 ? 4 : 8;
  const long long gx = (n + kRows - 1) / kRows, gy = (static_cast<long long>(R) * cp + 16 * kNT - 1) / (16 * kNT);
  if (gx > 0x7fffffffLL || gy > 65535) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
  // 16-byte loads need 16-byte aligned rows (every tensor the engine builds: ld is a vector multiple)
  const int xv = storage_vec(x_dtype), bv = 16 / storage_acc_bytes(x_dtype);
  const int vec = ldx % xv == 0 && ldb % bv == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(B) % 16 == 0;
  auto go = [&](auto tag, auto cpc) {
    using Tag = decltype(tag);
    return launch_mode<typename Tag::T, typename Tag::A, decltype(cpc)::value>(mode, grid, st, X, ldx, n, d, y, B, ldb,
                                                                               R, C, vec, loss, hits);
  };
  return dispatch_storage(x_dtype, [&](auto tag) {
    using Tag = decltype(tag);
    if constexpr (std::is_same_v<typename Tag::T, bf16_t>) {
      return hipErrorInvalidValue;
    } else {
      if (cp == 2) return go(tag, std::integral_constant<int, 2>{});
      if (cp == 4) return go(tag, std::integral_constant<int, 4>{});
      return go(tag, std::integral_constant<int, 8>{});
    }
  });
}

}  // namespace eh
