// K-fold cross-validation: the K fold models of one scalar loss over the same rows, one pass over X for all of them.
//
// Row i of a partition (its position in the partition, from 0) belongs to fold i mod K, and model k trains on every
// row whose fold is not k.  Model B [K][ld] model-major, labels as for the scalar losses.  For a row x of fold f:
//     z_k = x . B_k,   r_k = (k == f) ? 0 : residual<LOSS>(z_k, y, 1),   G_k += r_k x.
// That is the several-models kernel of an (alpha, lr) sweep (grad_multimodel.hip) at M = K with one compare and one
// select per row per wave behind the residual, so the two are one text (grad_models_kernel.h, EH_MODELS_FOLDS = true):
// the same task table, wave layout, LDS ring and FMA order.  A held-out row still runs through the dot products and
// the gradient FMAs, with r = 0: block k of the result is bit for bit what grad_models gives when the rows of fold k
// are zero rows (0 * x against r * 0; the rows must be finite, 0 * NaN is NaN).  The fold index is partition-local,
// never task- or stage-local, so every replica of a partition on every worker holds out the same rows.
#define EH_MODELS_KERNEL grad_folds
#define EH_MODELS_OVR false
#define EH_MODELS_FOLDS true
#include "grad_models_kernel.h"

namespace eh {

hipError_t grad_folds_launch(int dtype, int loss, int folds, const void* segs, const void* tasks, int ntasks,
                             const int* part_task_begin, int nparts, const void* beta, void* slab, void* Gb, int d_x,
                             int ld_x, hipStream_t st, const int* gate) {
  if (folds < kMinBlocks || folds > kMaxBlocks || ld_x < 1 || ld_x > kBlockMaxLd || d_x < 1 || d_x > ld_x ||
      (dtype != 0 && dtype != 1 && dtype != 3) || ld_x % storage_vec(dtype) != 0 || loss < 0 || loss > kSquaredHinge)
    return hipErrorInvalidValue;
  if (nparts == 0) return hipSuccess;
  return dispatch_storage(dtype, [&](auto S) {
    using T = typename decltype(S)::T;
    using A = typename decltype(S)::A;
    if constexpr (std::is_same_v<T, bf16_t>) {
      return hipErrorInvalidValue;
    } else {
      return dispatch_loss(loss, [&](auto L) -> hipError_t {
        constexpr int LOSS = decltype(L)::value;
        // the weighted codes have no cross-validation instance: the range check above rejects them
        if constexpr (LOSS > kSquaredHinge) {
          return hipErrorInvalidValue;
        } else {
          const int rowbytes = ld_x * static_cast<int>(sizeof(T));
          const int srows = blocks_stage_rows(rowbytes);
          const size_t lds = blocks_ring_bytes(srows, rowbytes);
          auto launch = [&](auto kern) {
            return launch_blocks<A>(kern, lds, srows, folds, segs, tasks, ntasks, part_task_begin, nparts, beta, slab,
                                    Gb, d_x, ld_x, st, gate);
          };
          return ld_x <= 256   ? launch(grad_folds<T, A, 4, LOSS>)
                 : ld_x <= 512 ? launch(grad_folds<T, A, 8, LOSS>)
                               : launch(grad_folds<T, A, 16, LOSS>);
        }
      });
    }
  });
}

}  // namespace eh
