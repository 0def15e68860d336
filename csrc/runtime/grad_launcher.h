// GradLauncher: the per-round gradient launch of one rank's local messages, captured once from the
// Python plan (ops/grad.py, ops/blockplan.py) by the one validator of its kind (grad_launcher.cpp
// make_dense / make_blocked / make_sparse).  The plan object keeps every referenced tensor alive; the
// launcher also holds references.  The launch functions are inline: the pumps call them every round.
#pragma once

#include <memory>
#include <vector>

#include "kernels/grad_dense.h"
#include "kernels/launchers.h"
#include "kernels/pack58.h"
#include "runtime/host_util.h"

namespace eh {

struct GradLauncher {
  // 0 dense fused, 1 dense two-pass, 2 sparse, 3 multi-class softmax, 4 several scalar-loss models, 5 one-vs-rest,
  // 6 K-fold cross-validation
  int kind = 0;
  int dtype = 0, loss = 0, cpl = 0, ntasks = 0, nslots = 0, ld = 0;
  KernelChoice choice{};
  const void* segs = nullptr;
  const void* tasks = nullptr;
  void* slab = nullptr;
  const int* stb = nullptr;
  void* part = nullptr;
  const int* task_row_off = nullptr;
  void* rbuf = nullptr;
  int acc = 0;
  int rows = 0;   // rows of G a launch writes: nslots, enc_slots after set_encode, the shared message rows (sparse dst)
  SparseArgs sa{};  // kind 2 (grad_sparse.hip); Gb is the launch's output
  // kind 3 / 4 / 5 / 6 (grad_softmax.hip: blocks are classes; grad_multimodel.hip: models of the scalar loss `loss`;
  // grad_ovr.hip: one-vs-rest classes of the scalar loss `loss`; grad_folds.hip: fold models of the scalar loss `loss`):
  // blocks, data columns / row stride of a block (ld is the flattened blocks * ld_x), distinct partitions (the
  // rows the kernel writes) and their task ranges stb [nparts + 1]
  int blocks = 0, d_x = 0, ld_x = 0, nparts = 0;
  // optional device encoding (csrc/kernels/encode.hip): the kernels above write the distinct
  // partitions' gradients into Gb, then G[slot] = sum_k coef * Gb[idx] for the enc_slots messages
  void* Gb = nullptr;
  const int* enc_ptr = nullptr;
  const int* enc_idx = nullptr;
  const double* enc_coef = nullptr;
  int enc_slots = 0;
  // packed dense plans (set_packed): the 58-bit copy of every segment's rows and the bundle flags
  PackedRows pk{};
  bool packed = false;
  const PackedRows* packed_rows() const { return packed ? &pk : nullptr; }
  std::vector<at::Tensor> keep;

  // The operand checks of a launch from Python (the pumps pass pointers they validated themselves).
  void check_operands(const at::Tensor& beta, const at::Tensor& G) const {
    need_gpu(beta, "beta");
    need_gpu(G, "G");
    need(acc_code(beta) == acc && acc_code(G) == acc, "beta / G must have the plan's accumulator dtype");
    need(beta.numel() >= ld, "beta must have >= ld elements");
    need(G.dim() == 2 && G.size(0) == rows && G.size(1) == ld, "G must be [rows the plan writes, ld]");
  }

  // gate: a lazy-drain worker round's stale-round gate (common.h gate_closed); nullptr = always run
  hipError_t launch(const void* beta, void* G, hipStream_t st, const int* gate = nullptr) const {
    if (!Gb) return launch_raw(beta, G, st, gate);
    if (kind == 2 && sa.sub_begin) {  // row-blocked sparse pass: the encoding adds the sub-block sums
      SparseArgs a = sa;
      a.Gb = Gb;
      a.encode_from_subs = 1;
      const hipError_t e = grad_sparse_launch(acc, loss, a, beta, st, gate);
      if (e != hipSuccess) return e;
      return encode_messages_launch(acc, sa.Gs, enc_ptr, enc_idx, enc_coef, G, enc_slots, ld, st, gate, sa.sub_begin);
    }
    const hipError_t e = launch_raw(beta, Gb, st, gate);
    if (e != hipSuccess) return e;
    return encode_messages_launch(acc, Gb, enc_ptr, enc_idx, enc_coef, G, enc_slots, ld, st, gate);
  }

  // Dense fused plans without device encoding can hand their result rows straight to the
  // receiver's mailbox from the final reduction kernel (slab_reduce.hip slab_reduce_fused_put / _final_put).
  bool can_fuse_put(int n) const { return kind == 0 && !Gb && ntasks > 0 && nslots == n; }
  // Device-driven local rounds: the combine + update ride the slab reduction (grad_dense_update_launch).
  bool can_fuse_update() const { return kind == 0 && !Gb && ntasks > 0; }
  hipError_t launch_update(const void* beta, void* G, const LocalUpdate& up, hipStream_t st) const {
    return grad_dense_update_launch(dtype, loss, cpl, segs, tasks, ntasks, beta, slab, stb, nslots, part, G, ld, st,
                                    choice, up, packed_rows());
  }
  hipError_t launch_put(const void* beta, void* G, const PutDesc& put, hipStream_t st) const {
    return grad_dense_launch(dtype, loss, cpl, segs, tasks, ntasks, beta, slab, stb, nslots, part, G, ld, st, choice,
                             &put, put.gate, packed_rows());
  }

  hipError_t launch_raw(const void* beta, void* G, hipStream_t st, const int* gate = nullptr) const {
    switch (kind) {
      case 0:
        return ntasks ? grad_dense_launch(dtype, loss, cpl, segs, tasks, ntasks, beta, slab, stb, nslots, part, G, ld,
                                          st, choice, nullptr, gate, packed_rows())
                      : hipSuccess;
      case 1:
        return ntasks ? grad_dense_twopass_launch(dtype, loss, segs, tasks, ntasks, beta, task_row_off, rbuf, slab, stb,
                                                  nslots, part, G, ld, st, gate)
                      : hipSuccess;
      case 2: {
        SparseArgs a = sa;
        a.Gb = G;
        if (!a.sub_begin) a.Gs = G;  // no sub-blocks: pass 2 / 3 write the partitions directly
        return grad_sparse_launch(acc, loss, a, beta, st, gate);
      }
      case 3:
        return grad_softmax_launch(dtype, blocks, segs, tasks, ntasks, stb, nparts, beta, slab, G, d_x, ld_x, st,
                                   gate);
      case 4:
        return grad_models_launch(dtype, loss, blocks, segs, tasks, ntasks, stb, nparts, beta, slab, G, d_x, ld_x, st,
                                  gate);
      case 5:
        return grad_ovr_launch(dtype, loss, blocks, segs, tasks, ntasks, stb, nparts, beta, slab, G, d_x, ld_x, st,
                               gate);
      case 6:
        return grad_folds_launch(dtype, loss, blocks, segs, tasks, ntasks, stb, nparts, beta, slab, G, d_x, ld_x, st,
                                 gate);
      default:
        return hipErrorInvalidValue;
    }
  }
};

}  // namespace eh
