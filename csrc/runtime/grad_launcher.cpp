// The plan validators: every operand check of a gradient plan lives here, once.  What a launch adds per
// call (beta, G) is GradLauncher::check_operands.
#include "runtime/grad_launcher.h"

#include <c10/hip/HIPStream.h>
#include <pybind11/stl.h>
#include <torch/extension.h>

#include <algorithm>
#include <optional>

namespace {
namespace py = pybind11;
using at::Tensor;
using namespace eh;

std::shared_ptr<GradLauncher> make_dense(int64_t dtype, int64_t loss, int64_t cpl, const Tensor& segs,
                                         const Tensor& tasks, const Tensor& slab, const Tensor& stb,
                                         const Tensor& part, int64_t ld, std::optional<Tensor> task_row_off,
                                         std::optional<Tensor> rbuf, const eh::KernelChoice& choice) {
  for (auto* t : {&segs, &tasks, &slab, &stb, &part}) need_gpu(*t, "dense plan operand");
  need(eh::storage_code_ok((int)dtype),
       "dtype code must be 0 (fp64), 1 (fp32), 2 (bf16 storage) or 3 (fp32 storage, fp64 accumulators)");
  const int ac = eh::storage_acc_code((int)dtype);
  need(tasks.dim() == 2 && tasks.size(1) == 5 && tasks.scalar_type() == at::kInt, "tasks must be int32 [n,5]");
  need(segs.scalar_type() == at::kByte && segs.numel() % 32 == 0, "segs must be packed uint8 [nseg*32]");
  need(stb.scalar_type() == at::kInt && stb.numel() >= 1, "slot_task_begin must be int32 [nslots + 1]");
  need(ld % eh::storage_vec((int)dtype) == 0, "ld must be a multiple of the 16-byte vector width");
  need(slab.dim() == 2 && slab.size(0) >= tasks.size(0) && slab.size(1) == ld && acc_code(slab) == ac,
       "slab must be [>=ntasks, ld] in the accumulator dtype");
  need(acc_code(part) == ac, "part must have the accumulator dtype");
  auto g = std::make_shared<GradLauncher>();
  g->dtype = (int)dtype;
  g->loss = (int)loss;
  g->cpl = (int)cpl;
  g->choice = choice;
  g->ld = (int)ld;
  g->ntasks = (int)tasks.size(0);
  g->nslots = (int)stb.numel() - 1;
  g->rows = g->nslots;
  need(part.numel() * part.element_size() >= eh::slab_part_bytes(g->nslots, ld, eh::storage_acc_bytes((int)dtype)),
       "part must hold the slab partial sums (grad.py DenseGradPlan)");
  g->segs = segs.data_ptr();
  g->tasks = tasks.data_ptr();
  g->slab = slab.data_ptr();
  g->stb = stb.data_ptr<int>();
  g->part = part.data_ptr();
  g->keep = {segs, tasks, slab, stb, part};
  g->acc = ac;
  if (task_row_off) {
    need(rbuf.has_value(), "two-pass plan needs rbuf");
    need_gpu(*task_row_off, "task_row_off");
    need_gpu(*rbuf, "rbuf");
    need(task_row_off->scalar_type() == at::kInt && task_row_off->numel() >= tasks.size(0), "task_row_off too small");
    need(rbuf->numel() >= 1 && acc_code(*rbuf) == ac, "rbuf must have the accumulator dtype");
    g->kind = 1;
    g->task_row_off = task_row_off->data_ptr<int>();
    g->rbuf = rbuf->data_ptr();
    g->keep.push_back(*task_row_off);
    g->keep.push_back(*rbuf);
  } else {
    need(cpl <= 32 ? cpl * 64 >= ld
                   : ((cpl == 256 || cpl == 512) && cpl * (ac == 0 ? 16 : 32) >= ld),  // grad_dense.hip launch_wide
         "cpl (narrow: columns per lane, wide: block size) must cover ld");
    g->kind = 0;
  }
  return g;
}

// Blocked-model plans (ops/blockplan.py BlockGradPlan): every distinct local partition once with coefficient 1 into
// rows of blocks * ld_x elements; the plan's device encoding (set_encode) forms the messages unless they are exactly
// the partitions.  kind 3: softmax, blocks = classes (ops/softmax.py); kind 4: `blocks` independent models of the
// scalar loss `loss` (ops/multimodel.py); kind 5: one-vs-rest, blocks = classes of the scalar loss `loss`
// (ops/ovr.py); kind 6: K-fold cross-validation, blocks = fold models of the scalar loss `loss` (ops/cv.py).
// who / what: the prefix and the block noun of the error texts.
std::shared_ptr<GradLauncher> make_blocked(int kind, const std::string& who, const std::string& what, int64_t dtype,
                                           int64_t loss, int64_t blocks, const Tensor& segs, const Tensor& tasks,
                                           const Tensor& slab, const Tensor& part_task_begin, int64_t d_x,
                                           int64_t ld_x) {
  for (auto* t : {&segs, &tasks, &slab, &part_task_begin}) need_gpu(*t, (who + " plan operand").c_str());
  need(blocks >= eh::kMinBlocks && blocks <= eh::kMaxBlocks, who + ": " + what + " must be in 2..8");
  need(ld_x >= 1 && ld_x <= eh::kBlockMaxLd && d_x >= 1 && d_x <= ld_x && ld_x % eh::storage_vec((int)dtype) == 0,
       who + ": rows of at most 1024 columns, padded to the 16-byte vector width");
  need(tasks.dim() == 2 && tasks.size(1) == 5 && tasks.scalar_type() == at::kInt, "tasks must be int32 [n,5]");
  need(segs.scalar_type() == at::kByte && segs.numel() % 32 == 0, "segs must be packed uint8 [nseg*32]");
  need(part_task_begin.scalar_type() == at::kInt && part_task_begin.numel() >= 1, "part_task_begin must be int32");
  auto g = std::make_shared<GradLauncher>();
  g->kind = kind;
  g->dtype = (int)dtype;
  g->acc = eh::storage_acc_code((int)dtype);
  g->loss = (int)loss;
  g->blocks = (int)blocks;
  g->d_x = (int)d_x;
  g->ld_x = (int)ld_x;
  g->ld = (int)(blocks * ld_x);
  g->ntasks = (int)tasks.size(0);
  g->nparts = (int)part_task_begin.numel() - 1;
  g->nslots = g->rows = g->nparts;
  need(acc_code(slab) == g->acc && slab.numel() >= (int64_t)std::max(1, g->ntasks) * eh::kBlockSubs * g->ld,
       "slab must hold [ntasks][4][" + what + " * ld_x] partial sums (acc dtype)");
  {  // the kernel indexes segments, rows and slab rows with the task table: checked once, on the host
    const Tensor tc = tasks.cpu().contiguous(), pc = part_task_begin.cpu().contiguous(), sc = segs.cpu().contiguous();
    const auto* T = reinterpret_cast<const eh::Task*>(tc.data_ptr<int>());
    const int* P = pc.data_ptr<int>();
    const auto* S = reinterpret_cast<const eh::Segment*>(sc.data_ptr<uint8_t>());
    const int64_t nseg = segs.numel() / 32;
    for (int k = 0; k < g->ntasks; ++k) {
      const eh::Task& t = T[k];
      need(t.seg >= 0 && t.seg < nseg && t.row_begin >= 0 && t.row_begin <= t.row_end &&
               t.row_end <= S[t.seg].nrows && t.slab >= 0 && t.slab < std::max(1, g->ntasks),
           "tasks: (slot, segment, row_begin <= row_end <= the segment's rows, slab row) inside the tables");
    }
    need(P[0] == 0 && P[g->nparts] == g->ntasks, "part_task_begin: [0, .., ntasks]");
    for (int p = 0; p < g->nparts; ++p) need(P[p] <= P[p + 1], "part_task_begin: non-decreasing");
  }
  g->segs = segs.data_ptr();
  g->tasks = tasks.data_ptr();
  g->slab = slab.data_ptr();
  g->stb = part_task_begin.data_ptr<int>();
  g->keep = {segs, tasks, slab, part_task_begin};
  return g;
}

std::shared_ptr<GradLauncher> make_softmax(int64_t dtype, int64_t classes, const Tensor& segs, const Tensor& tasks,
                                           const Tensor& slab, const Tensor& part_task_begin, int64_t d_x,
                                           int64_t ld_x) {
  need(dtype == 0 || dtype == 1, "softmax: fp64 or fp32 storage");
  return make_blocked(3, "softmax", "classes", dtype, 3, classes, segs, tasks, slab, part_task_begin, d_x, ld_x);
}

std::shared_ptr<GradLauncher> make_multimodel(int64_t dtype, int64_t loss, int64_t models, const Tensor& segs,
                                              const Tensor& tasks, const Tensor& slab, const Tensor& part_task_begin,
                                              int64_t d_x, int64_t ld_x) {
  need(dtype == 0 || dtype == 1 || dtype == 3, "multi-model: fp64, fp32 or fp32x64 (fp32 storage, fp64 accumulators)");
  need(loss >= 0 && loss <= 2, "multi-model: logistic, least squares or squared hinge");
  return make_blocked(4, "multi-model", "models", dtype, loss, models, segs, tasks, slab, part_task_begin, d_x, ld_x);
}

std::shared_ptr<GradLauncher> make_ovr(int64_t dtype, int64_t loss, int64_t classes, const Tensor& segs,
                                       const Tensor& tasks, const Tensor& slab, const Tensor& part_task_begin,
                                       int64_t d_x, int64_t ld_x) {
  need(dtype == 0 || dtype == 1 || dtype == 3, "one-vs-rest: fp64, fp32 or fp32x64 (fp32 storage, fp64 accumulators)");
  need(loss == 0 || loss == 2, "one-vs-rest: logistic or squared hinge");
  return make_blocked(5, "one-vs-rest", "classes", dtype, loss, classes, segs, tasks, slab, part_task_begin, d_x, ld_x);
}

std::shared_ptr<GradLauncher> make_folds(int64_t dtype, int64_t loss, int64_t folds, const Tensor& segs,
                                         const Tensor& tasks, const Tensor& slab, const Tensor& part_task_begin,
                                         int64_t d_x, int64_t ld_x) {
  need(dtype == 0 || dtype == 1 || dtype == 3,
       "cross-validation: fp64, fp32 or fp32x64 (fp32 storage, fp64 accumulators)");
  need(loss >= 0 && loss <= 2, "cross-validation: logistic, least squares or squared hinge");
  return make_blocked(6, "cross-validation", "folds", dtype, loss, folds, segs, tasks, slab, part_task_begin, d_x, ld_x);
}

// Sparse plan (ops/grad.py SparseGradPlan): every distinct local partition once; the plan's device
// encoding (set_encode) forms the messages.  Tensors are kept alive by the launcher.
std::shared_ptr<GradLauncher> make_sparse(int64_t loss, const Tensor& y, const Tensor& u, std::optional<Tensor> ell_idx,
                                          std::optional<Tensor> lo, std::optional<Tensor> row_ptr,
                                          std::optional<Tensor> col_idx, std::optional<Tensor> vals, const Tensor& crow,
                                          std::optional<Tensor> cvals, const Tensor& col_ptr, const Tensor& tiles,
                                          const Tensor& part_entry0, const Tensor& part_row0, const Tensor& part_nnz,
                                          const Tensor& head, const Tensor& tail, const Tensor& span,
                                          const Tensor& empty, int64_t nparts, int64_t d, int64_t ld,
                                          std::optional<Tensor> wg, int64_t u_lds, std::optional<Tensor> Gs,
                                          std::optional<Tensor> sub_begin, std::optional<Tensor> runs,
                                          std::optional<Tensor> tkeys, std::optional<Tensor> wspan,
                                          std::optional<Tensor> wspan_ptr, std::optional<Tensor> dst, int64_t csr_fixed) {
  for (auto* t : {&y, &u, &crow, &col_ptr, &tiles, &part_entry0, &part_row0, &part_nnz, &head, &tail, &span, &empty})
    need_gpu(*t, "sparse plan operand");
  need(tiles.scalar_type() == at::kInt && tiles.dim() == 2 && tiles.size(1) == 4, "tiles: int32 [n, 4]");
  need(span.scalar_type() == at::kInt && span.dim() == 2 && span.size(1) == 4, "span: int32 [n, 4]");
  need(empty.scalar_type() == at::kInt && empty.dim() == 2 && empty.size(1) == 2, "empty: int32 [n, 2]");
  need(col_ptr.scalar_type() == at::kInt && col_ptr.numel() == nparts * (d + 1), "col_ptr: int32 [nparts, d + 1]");
  need(part_entry0.scalar_type() == at::kLong && part_row0.scalar_type() == at::kLong &&
           part_nnz.scalar_type() == at::kInt && part_nnz.numel() == nparts,
       "partition offsets");
  need(crow.scalar_type() == at::kShort || crow.scalar_type() == at::kInt, "crow: int16 | int32");
  auto g = std::make_shared<GradLauncher>();
  g->kind = 2;
  g->loss = (int)loss;
  g->acc = acc_code(y);
  need(acc_code(u) == g->acc && acc_code(head) == g->acc && acc_code(tail) == g->acc, "acc dtype mismatch");
  g->ld = (int)ld;
  g->nslots = g->rows = (int)nparts;
  eh::SparseArgs& a = g->sa;
  a.nrows = y.numel();
  a.y = y.data_ptr();
  a.u = u.data_ptr();
  g->keep = {y, u, crow, col_ptr, tiles, part_entry0, part_row0, part_nnz, head, tail, span, empty};
  if (ell_idx) {
    need_gpu(*ell_idx, "ell_idx");
    need(ell_idx->dim() == 2 && ell_idx->size(1) >= a.nrows, "ell_idx: [m, >= rows]");
    a.ell_ld = ell_idx->size(1);
    a.ell = 1;
    a.idx16 = ell_idx->scalar_type() == at::kShort ? 1 : 0;
    need(a.idx16 || ell_idx->scalar_type() == at::kInt, "ell_idx: int16 | int32");
    a.m = (int)ell_idx->size(0);
    a.ell_idx = ell_idx->data_ptr();
    if (a.idx16) {
      need(lo.has_value() && lo->numel() == a.m && lo->scalar_type() == at::kInt, "lo: int32 [m]");
      need_gpu(*lo, "lo");
      a.lo = lo->data_ptr<int>();
      g->keep.push_back(*lo);
    }
    g->keep.push_back(*ell_idx);
  } else {
    need(row_ptr.has_value() && col_idx.has_value(), "CSR row pass needs row_ptr / col_idx");
    need_gpu(*row_ptr, "row_ptr");
    need_gpu(*col_idx, "col_idx");
    need(row_ptr->scalar_type() == at::kLong && row_ptr->numel() == a.nrows + 1, "row_ptr: int64 [rows + 1]");
    a.row_ptr = reinterpret_cast<const long long*>(row_ptr->data_ptr<int64_t>());
    a.col_idx = col_idx->data_ptr<int>();
    need(csr_fixed >= 0 && (csr_fixed == 0 || col_idx->numel() == csr_fixed * a.nrows), "csr_fixed: nnz of every row");
    a.csr_fixed = (int)csr_fixed;
    g->keep.push_back(*row_ptr);
    g->keep.push_back(*col_idx);
  }
  if (vals) {
    need_gpu(*vals, "vals");
    need(acc_code(*vals) == g->acc, "vals dtype");
    need(!ell_idx || vals->sizes() == ell_idx->sizes(), "ELL vals: the shape of ell_idx");
    a.vals = vals->data_ptr();
    g->keep.push_back(*vals);
  }
  a.row16 = crow.scalar_type() == at::kShort ? 1 : 0;
  a.crow = crow.data_ptr();
  if (cvals) {
    need_gpu(*cvals, "cvals");
    need(acc_code(*cvals) == g->acc && cvals->numel() == crow.numel(), "cvals: acc dtype, one per CSC entry");
    a.cvals = cvals->data_ptr();
    g->keep.push_back(*cvals);
  }
  a.col_ptr = col_ptr.data_ptr<int>();
  a.tiles = reinterpret_cast<const int4*>(tiles.data_ptr<int>());
  a.ntiles = (int)tiles.size(0);
  need(crow.numel() >= static_cast<int64_t>(a.ntiles) * 512, "crow: every partition padded to whole 512-entry tiles");
  need(head.numel() >= a.ntiles && tail.numel() >= a.ntiles, "head / tail: one per tile");
  a.part_entry0 = reinterpret_cast<const long long*>(part_entry0.data_ptr<int64_t>());
  a.part_row0 = reinterpret_cast<const long long*>(part_row0.data_ptr<int64_t>());
  a.part_nnz = part_nnz.data_ptr<int>();
  a.head = head.data_ptr();
  a.tail = tail.data_ptr();
  a.span = reinterpret_cast<const int4*>(span.data_ptr<int>());
  a.nspan = (int)span.size(0);
  a.empty = reinterpret_cast<const int2*>(empty.data_ptr<int>());
  a.nempty = (int)empty.size(0);
  a.d = (int)d;
  a.ld = (int)ld;
  if (wg) {  // row-blocked column pass: `nparts` above counts sub-blocks
    need_gpu(*wg, "wg");
    need(wg->scalar_type() == at::kInt && wg->dim() == 2 && wg->size(1) == 4, "wg: int32 [n, 4]");
    need(u_lds > 0 && u_lds * (g->acc == 0 ? 8 : 4) <= 96 * 1024, "u_lds: sub-block rows staged in LDS (<= 96 KB)");
    {  // the column pass's chunks: 1..128 tiles each (grad_sparse.hip kMaxWgTiles), rows staged in LDS
      const Tensor wc = wg->cpu();
      const int* W = wc.data_ptr<int>();
      for (int64_t k = 0; k < wg->size(0); ++k)
        need(W[4 * k + 2] >= 1 && W[4 * k + 2] <= 128 && W[4 * k + 1] >= 0 && W[4 * k + 1] + W[4 * k + 2] <= tiles.size(0) &&
                 W[4 * k + 3] <= u_lds,
             "wg: (row0, first tile, 1..128 tiles, rows <= u_lds)");
    }
    a.wg = reinterpret_cast<const int4*>(wg->data_ptr<int>());
    a.nwg = (int)wg->size(0);
    a.u_lds = (int)u_lds;
    g->keep.push_back(*wg);
    need(runs.has_value() && tkeys.has_value(), "the row-blocked column pass needs the run lists (runs, tkeys)");
    need_gpu(*runs, "runs");
    need_gpu(*tkeys, "tkeys");
    need(runs->scalar_type() == at::kInt && runs->numel() >= 1, "runs: int32 [runs]");
    need(tkeys->scalar_type() == at::kInt && tkeys->dim() == 2 && tkeys->size(0) == a.ntiles && tkeys->size(1) == 4,
         "tkeys: int32 [tiles, 4]");
    a.runs = runs->data_ptr<int>();
    a.tkeys = reinterpret_cast<const int4*>(tkeys->data_ptr<int>());
    g->keep.push_back(*runs);
    g->keep.push_back(*tkeys);
    if (wspan_ptr) {  // column-aligned chunks: every crossing column summed inside its workgroup
      need(wspan.has_value(), "wspan_ptr needs wspan");
      need_gpu(*wspan, "wspan");
      need_gpu(*wspan_ptr, "wspan_ptr");
      need(a.nspan == 0, "column-aligned chunks leave no global spans");
      need(wspan->scalar_type() == at::kInt && wspan->dim() == 2 && wspan->size(1) == 4, "wspan: int32 [n, 4]");
      need(wspan_ptr->scalar_type() == at::kInt && wspan_ptr->numel() == a.nwg + 1, "wspan_ptr: int32 [workgroups + 1]");
      // the kernel indexes its LDS head / tail arrays with these: checked once, on the host
      const Tensor sp = wspan->cpu(), pp = wspan_ptr->cpu(), wc = wg->cpu();
      const int* P = pp.data_ptr<int>();
      const int* S = sp.data_ptr<int>();
      const int* W = wc.data_ptr<int>();
      need(P[0] == 0 && P[a.nwg] == sp.size(0), "wspan_ptr: [0, .., spans]");
      for (int k = 0; k < a.nwg; ++k) {
        need(P[k] <= P[k + 1] && P[k + 1] - P[k] < 128, "wspan_ptr: non-decreasing, < 128 spans per workgroup");
        for (int i = P[k]; i < P[k + 1]; ++i) {
          const int* e = S + 4 * i;
          need(e[0] >= 0 && e[0] < nparts && e[1] >= 0 && e[1] < d && e[2] >= 0 && e[2] < e[3] && e[3] < W[4 * k + 2],
               "wspan: (sub-block, column, first tile < last tile < the workgroup's tiles)");
        }
      }
      a.wspan = reinterpret_cast<const int4*>(wspan->data_ptr<int>());
      a.wspan_ptr = wspan_ptr->data_ptr<int>();
      g->keep.push_back(*wspan);
      g->keep.push_back(*wspan_ptr);
    }
  }
  if (dst) {  // shared message rows of merged FRC / AGC units (ops/grad.py SparseGradPlan.units)
    need_gpu(*dst, "dst");
    need(!sub_begin && wg && a.nspan == 0, "shared message rows need unblocked units and the row-blocked column pass");
    need(dst->scalar_type() == at::kInt && dst->dim() == 2 && dst->size(0) == nparts &&
             dst->size(1) == eh::kSparseMaxDst,
         "dst: int32 [units, 4]");
    const Tensor dc = dst->cpu();
    const int* D = dc.data_ptr<int>();
    g->rows = 0;
    for (int64_t k = 0; k < dst->numel(); ++k) {
      need(D[k] >= -1 && D[k] < 4096, "dst: message rows or -1");
      g->rows = std::max(g->rows, D[k] + 1);
    }
    a.dst = dst->data_ptr<int>();
    g->keep.push_back(*dst);
  }
  if (sub_begin) {
    need(Gs.has_value(), "sub-blocks need their Gs buffer");
    need_gpu(*sub_begin, "sub_begin");
    need_gpu(*Gs, "Gs");
    need(sub_begin->scalar_type() == at::kInt && sub_begin->numel() >= 2, "sub_begin: int32 [partitions + 1]");
    need(Gs->dim() == 2 && Gs->size(0) == nparts && Gs->size(1) == ld && acc_code(*Gs) == g->acc,
         "Gs: [sub-blocks, ld] in the accumulator dtype");
    a.sub_begin = sub_begin->data_ptr<int>();
    a.nparts = (int)sub_begin->numel() - 1;
    a.Gs = Gs->data_ptr();
    g->nslots = g->rows = a.nparts;  // Gb rows: the partitions
    g->keep.push_back(*sub_begin);
    g->keep.push_back(*Gs);
  }
  return g;
}

}  // namespace

namespace eh {
void bind_grad_launcher(py::module& m) {
  py::class_<GradLauncher, std::shared_ptr<GradLauncher>>(m, "GradLauncher")
      .def_static("dense", &make_dense, py::arg("dtype"), py::arg("loss"), py::arg("cpl"), py::arg("segs"),
                  py::arg("tasks"), py::arg("slab"), py::arg("slot_task_begin"), py::arg("part"), py::arg("ld"),
                  py::arg("task_row_off") = py::none(), py::arg("rbuf") = py::none(),
                  py::arg("choice") = eh::KernelChoice{})
      .def_static("softmax", &make_softmax, py::arg("dtype"), py::arg("classes"), py::arg("segs"), py::arg("tasks"),
                  py::arg("slab"), py::arg("part_task_begin"), py::arg("d_x"), py::arg("ld_x"))
      .def_static("multimodel", &make_multimodel, py::arg("dtype"), py::arg("loss"), py::arg("models"), py::arg("segs"),
                  py::arg("tasks"), py::arg("slab"), py::arg("part_task_begin"), py::arg("d_x"), py::arg("ld_x"))
      .def_static("ovr", &make_ovr, py::arg("dtype"), py::arg("loss"), py::arg("classes"), py::arg("segs"),
                  py::arg("tasks"), py::arg("slab"), py::arg("part_task_begin"), py::arg("d_x"), py::arg("ld_x"))
      .def_static("folds", &make_folds, py::arg("dtype"), py::arg("loss"), py::arg("folds"), py::arg("segs"),
                  py::arg("tasks"), py::arg("slab"), py::arg("part_task_begin"), py::arg("d_x"), py::arg("ld_x"))
      .def_static("sparse", &make_sparse, py::arg("loss"), py::arg("y"), py::arg("u"), py::arg("ell_idx"), py::arg("lo"),
                  py::arg("row_ptr"), py::arg("col_idx"), py::arg("vals"), py::arg("crow"), py::arg("cvals"),
                  py::arg("col_ptr"), py::arg("tiles"), py::arg("part_entry0"), py::arg("part_row0"),
                  py::arg("part_nnz"), py::arg("head"), py::arg("tail"), py::arg("span"), py::arg("empty"),
                  py::arg("nparts"), py::arg("d"), py::arg("ld"), py::arg("wg") = py::none(), py::arg("u_lds") = 0,
                  py::arg("Gs") = py::none(), py::arg("sub_begin") = py::none(),
                  py::arg("runs") = py::none(), py::arg("tkeys") = py::none(), py::arg("wspan") = py::none(),
                  py::arg("wspan_ptr") = py::none(), py::arg("dst") = py::none(), py::arg("csr_fixed") = 0)
      .def("set_encode",
           [](GradLauncher& g, const Tensor& ptr, const Tensor& idx, const Tensor& coef, const Tensor& Gb) {
             for (auto* t : {&ptr, &idx, &coef, &Gb}) need_gpu(*t, "encode operand");
             need(ptr.scalar_type() == at::kInt && idx.scalar_type() == at::kInt, "encode ptr/idx must be int32");
             need(coef.scalar_type() == at::kDouble, "encode coefficients must be fp64");
             need(Gb.dim() == 2 && Gb.size(0) == g.nslots && Gb.size(1) == g.ld && acc_code(Gb) == g.acc,
                  "Gb must be [distinct partitions, ld] in the accumulator dtype");
             need(idx.numel() == coef.numel(), "encode idx/coef size mismatch");
             g.enc_slots = g.rows = (int)ptr.numel() - 1;
             g.Gb = Gb.data_ptr();
             g.enc_ptr = ptr.data_ptr<int>();
             g.enc_idx = idx.data_ptr<int>();
             g.enc_coef = coef.data_ptr<double>();
             for (auto* t : {&ptr, &idx, &coef, &Gb}) g.keep.push_back(*t);
           })
      // Packed dense plan (ops/grad.py DenseGradPlan, kernels/pack58.h): rows[s] is the 7424-byte-per-row copy of
      // segment s's partition (replica segments share one tensor), seg_rows[s] its row count, e0 [nseg] the exponent
      // windows.  Packs every bundle's rows on the current stream, compares them with the source and fills
      // flags [bundles]; every launch from then on streams the packed rows of the bundles flagged 1.
      .def(
          "set_packed",
          [](GradLauncher& g, const std::vector<Tensor>& rows, const std::vector<int64_t>& seg_rows, const Tensor& e0,
             const Tensor& flags, bool pack) {
            const int R = g.choice.replicas;
            need(g.kind == 0 && g.dtype == 0 && g.cpl == 16 && g.choice.kind == eh::kGradMulti && g.choice.fold &&
                     !g.choice.pair && g.ld > 512 && g.ld <= eh::p58::kCols && R >= 1 && R <= 3 && g.ntasks > 0 &&
                     g.ntasks % (4 * R) == 0 && !g.packed,
                 "set_packed: fp64 folded one-wave bundles of 16 columns per lane only, once per launcher");
            const int64_t nseg = g.keep[0].numel() / 32;
            need((int64_t)rows.size() == nseg && (int64_t)seg_rows.size() == nseg, "set_packed: one packed copy per segment");
            need_gpu(e0, "e0");
            need_gpu(flags, "flags");
            need(e0.scalar_type() == at::kInt && e0.numel() == nseg && e0.is_contiguous(), "e0: int32 [segments]");
            need(flags.scalar_type() == at::kInt && flags.numel() == g.ntasks / R && flags.is_contiguous(),
                 "flags: int32 [bundles]");
            const Tensor eh0 = e0.cpu();
            std::vector<int64_t> ptrs;
            for (int64_t s = 0; s < nseg; ++s) {
              need_gpu(rows[s], "packed rows");
              need(rows[s].scalar_type() == at::kByte && rows[s].is_contiguous() && seg_rows[s] >= 0 &&
                       rows[s].numel() >= seg_rows[s] * eh::p58::kRowBytes &&
                       reinterpret_cast<uintptr_t>(rows[s].data_ptr()) % 128 == 0,
                   "packed rows: uint8 [rows * 7424], 128-byte aligned");
              const int e = eh0.data_ptr<int>()[s];
              need(e >= eh::p58::kE0Min && e <= eh::p58::kE0Max, "e0: a window of 31 normal binades");
              ptrs.push_back(static_cast<int64_t>(reinterpret_cast<uintptr_t>(rows[s].data_ptr())));
            }
            const Tensor ptr = torch::tensor(ptrs, torch::dtype(torch::kLong)).to(flags.device());
            void* const* P = reinterpret_cast<void* const*>(ptr.data_ptr<int64_t>());
            if (pack)  // (false: a further launcher of a plan whose first launcher packed these tensors)
              hcheck(eh::pack58_launch(g.segs, g.tasks, g.ntasks, R, P, e0.data_ptr<int>(), flags.data_ptr<int>(),
                                       g.ld, eh::stream_of(flags)),
                     "GradLauncher.set_packed");
            g.pk.rows = reinterpret_cast<const void* const*>(P);
            g.pk.e0 = e0.data_ptr<int>();
            g.pk.flags = flags.data_ptr<int>();
            g.packed = true;
            g.keep.push_back(ptr);
            g.keep.push_back(e0);
            g.keep.push_back(flags);
            for (const Tensor& t : rows) g.keep.push_back(t);
          },
          py::arg("rows"), py::arg("seg_rows"), py::arg("e0"), py::arg("flags"), py::arg("pack") = true)
      .def_property_readonly("packed", [](const GradLauncher& g) { return g.packed; })
      .def(
          "launch",
          [](const GradLauncher& g, const Tensor& beta, const Tensor& G, std::optional<Tensor> gate) {
            g.check_operands(beta, G);
            if (gate) need(gate->is_cuda() && gate->scalar_type() == at::kInt && gate->numel() >= 1, "gate: int32 GPU");
            hcheck(g.launch(beta.data_ptr(), G.data_ptr(), eh::stream_of(G), gate ? gate->data_ptr<int>() : nullptr),
                   "GradLauncher.launch");
          },
          py::arg("beta"), py::arg("G"), py::arg("gate") = py::none())
      // The gradient with its tagged put fused into the slab reduction (launch_put), for the kernel
      // tests: the same descriptor as ipc.cpp put_signal_tagged; the worker pump builds its own natively.
      .def(
          "launch_put_tagged",
          [](const GradLauncher& g, const Tensor& beta, const Tensor& G, const Tensor& dst, const Tensor& tags,
             uintptr_t flag, uint64_t value, int64_t rank, const Tensor& counters, const Tensor& csum, bool corrupt) {
            g.check_operands(beta, G);
            for (auto* t : {&dst, &tags, &counters, &csum}) need_gpu(*t, "launch_put_tagged operand");
            need(g.can_fuse_put((int)G.size(0)),
                 "launch_put_tagged: a dense fused plan and its [nslots, ld] message buffer");
            need(dst.sizes() == G.sizes() && dst.scalar_type() == G.scalar_type(), "launch_put_tagged: dst like G");
            need(G.size(0) <= eh::kMaxTagRows && tags.numel() * tags.element_size() >= G.size(0) * 16 &&
                     csum.scalar_type() == at::kLong && csum.numel() >= G.size(0) &&
                     counters.scalar_type() == at::kInt && counters.numel() >= 1 && flag != 0,
                 "launch_put_tagged: tags [rows*16 bytes], csum int64 [rows], counters int32, a flag");
            eh::PutDesc d{G.data_ptr(), dst.data_ptr(), G.numel() * G.element_size(),
                          reinterpret_cast<unsigned long long*>(flag), value,
                          reinterpret_cast<unsigned int*>(counters.data_ptr<int>())};
            d.tag = static_cast<eh::MsgTag*>(tags.data_ptr());
            d.csum = reinterpret_cast<unsigned long long*>(csum.data_ptr<int64_t>());
            d.rows = (int)G.size(0);
            d.es = (int)G.element_size();
            d.rank = static_cast<unsigned int>(rank);
            d.corrupt = corrupt ? 1 : 0;
            hcheck(g.launch_put(beta.data_ptr(), G.data_ptr(), d, eh::stream_of(G)), "GradLauncher.launch_put_tagged");
          },
          py::arg("beta"), py::arg("G"), py::arg("dst"), py::arg("tags"), py::arg("flag"), py::arg("value"),
          py::arg("rank"), py::arg("counters"), py::arg("csum"), py::arg("corrupt") = false);
}
}  // namespace eh
