// One-vs-rest: C binary models of one scalar loss over the same rows, one pass over X for all of them.
//
// Labels are class indices 0..C-1 held as floats (as for softmax); model B [C][ld] class-major.  Model k is the
// binary classifier "class k against the rest": for a row x with class y,
//     y_k = (y == k) ? +1 : -1,   z_k = x . B_k,   r_k = residual<LOSS>(z_k, y_k, 1),   G_k += r_k x.
// That is the several-models kernel of an (alpha, lr) sweep (grad_multimodel.hip) with one compare and one select
// per row per wave in front of the residual, so the two are one text (grad_models_kernel.h, EH_MODELS_OVR = true):
// the same task table, wave layout, LDS ring and FMA order, and block k of the result is bit for bit what
// grad_models gives for the labels y_k.  LOSS is logistic or squared hinge (least squares has no one-vs-rest form
// here, the weighted codes keep their weight in the label).
#define EH_MODELS_KERNEL grad_ovr
#define EH_MODELS_OVR true
#include "grad_models_kernel.h"

namespace eh {

hipError_t grad_ovr_launch(int dtype, int loss, int classes, const void* segs, const void* tasks, int ntasks,
                           const int* part_task_begin, int nparts, const void* beta, void* slab, void* Gb, int d_x,
                           int ld_x, hipStream_t st, const int* gate) {
  if (classes < kMinBlocks || classes > kMaxBlocks || ld_x < 1 || ld_x > kBlockMaxLd || d_x < 1 || d_x > ld_x ||
      (dtype != 0 && dtype != 1 && dtype != 3) || ld_x % storage_vec(dtype) != 0 ||
      (loss != kLogistic && loss != kSquaredHinge))
    return hipErrorInvalidValue;
  if (nparts == 0) return hipSuccess;
  return dispatch_storage(dtype, [&](auto S) {
    using T = typename decltype(S)::T;
    using A = typename decltype(S)::A;
    if constexpr (std::is_same_v<T, bf16_t>) {
      return hipErrorInvalidValue;
    } else {
      const int rowbytes = ld_x * static_cast<int>(sizeof(T));
      const int srows = blocks_stage_rows(rowbytes);
      const size_t lds = blocks_ring_bytes(srows, rowbytes);
      auto with_loss = [&](auto L) -> hipError_t {
        constexpr int LOSS = decltype(L)::value;
        auto launch = [&](auto kern) {
          return launch_blocks<A>(kern, lds, srows, classes, segs, tasks, ntasks, part_task_begin, nparts, beta, slab,
                                  Gb, d_x, ld_x, st, gate);
        };
        return ld_x <= 256   ? launch(grad_ovr<T, A, 4, LOSS>)
               : ld_x <= 512 ? launch(grad_ovr<T, A, 8, LOSS>)
                             : launch(grad_ovr<T, A, 16, LOSS>);
      };
      return loss == kLogistic ? with_loss(std::integral_constant<int, kLogistic>{})
                               : with_loss(std::integral_constant<int, kSquaredHinge>{});
    }
  });
}

}  // namespace eh
