// Several independent scalar-loss models over the same rows: one pass over X for all M models.
//
// An (alpha, lr) sweep trains M models that differ only in their update coefficients; their gradients
// at a round differ only through beta.  Model B [M][ld] model-major, labels as for the scalar losses.
// For a row x and model k:   z_k = x . B_k,  r_k = residual<LOSS>(z_k, y, 1),  G_k += r_k x.
// Running the one-model kernels M times would stream X once per model; here a workgroup streams a row
// range of one partition through grad_softmax.hip's transport (two-stage LDS ring with LDS-DMA, nt
// policy: every X element leaves HBM once per launch) and all M dot products, residuals and gradient
// rows are formed from the LDS copy.
//
// The kernel's text is grad_models_kernel.h, which the one-vs-rest kernel (grad_ovr.hip) compiles too; here every
// model sees the rows' own labels.
#define EH_MODELS_KERNEL grad_models
#define EH_MODELS_OVR false
#include "grad_models_kernel.h"

namespace eh {

hipError_t grad_models_launch(int dtype, int loss, int models, const void* segs, const void* tasks, int ntasks,
                              const int* part_task_begin, int nparts, const void* beta, void* slab, void* Gb, int d_x,
                              int ld_x, hipStream_t st, const int* gate) {
  if (models < kMinBlocks || models > kMaxBlocks || ld_x < 1 || ld_x > kBlockMaxLd || d_x < 1 || d_x > ld_x ||
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
        // the weighted codes (kLogisticW, kSquaredHingeW) have no multi-model instance: the range check above
        // rejects them, and nothing is instantiated for them here
        if constexpr (LOSS > kSquaredHinge) {
          return hipErrorInvalidValue;
        } else {
          const int rowbytes = ld_x * static_cast<int>(sizeof(T));
          const int srows = blocks_stage_rows(rowbytes);
          const size_t lds = blocks_ring_bytes(srows, rowbytes);
          auto launch = [&](auto kern) {
            return launch_blocks<A>(kern, lds, srows, models, segs, tasks, ntasks, part_task_begin, nparts, beta,
                                    slab, Gb, d_x, ld_x, st, gate);
          };
          return ld_x <= 256   ? launch(grad_models<T, A, 4, LOSS>)
                 : ld_x <= 512 ? launch(grad_models<T, A, 8, LOSS>)
                               : launch(grad_models<T, A, 16, LOSS>);
        }
      });
    }
  });
}

}  // namespace eh
