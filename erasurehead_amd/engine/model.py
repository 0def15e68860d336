"""What kind of model a run trains, decided once (ModelSpec), and its update schedule (UpdateSchedule).

Five kinds share the engine: a ``single`` model of a scalar loss, ``softmax`` and one-vs-rest (``ovr``) with one
block per class, a ``sweep`` of M (alpha, lr, l1) models of one scalar loss, and the K fold models of a K-fold
cross-validation (``cv``) of one scalar loss.  Everything the engine keeps
(beta, messages, history, checkpoints) is one vector of ``ld`` elements, block-major ``[blocks][ld_x]`` with
``ld_x = prec.ld(d_x)`` and the padding columns of every block exactly zero; ``d`` of them are stored per round.
A single model is one block with ``d = d_x``; the other kinds have ``d = ld = blocks * ld_x``.

The spec owns the run's rejections, this layout (:meth:`ModelSpec.beta0`, :meth:`ModelSpec.pack`,
:meth:`ModelSpec.unpack`, :meth:`ModelSpec.rows`), the gradient plan, how the run is scored and named, and what
a rank report and a checkpoint say about it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from ..models.losses import (LEAST_SQUARES, LOGISTIC, LOSS_CHOICES, SOFTMAX, SQUARED_HINGE, UpdateRule, base_kind,
                             check_classes, is_classification, weighted_kind)
from ..ops.cv import CvGradPlan
from ..ops.grad import DenseGradPlan, SharedGradPlan, SparseGradPlan
from ..ops.multimodel import MultiModelGradPlan
from ..ops.ovr import OvrGradPlan
from ..ops.precision import Precision
from ..ops.softmax import SoftmaxGradPlan
from ..ops.update import combine_update, combine_update_blocks, combine_update_prox

SQHINGE_PREFIX = "sqhinge_"  # result files of squared-hinge runs (next to the logistic names)
SOFTMAX_PREFIX = "softmax_"
OVR_PREFIX = "ovr_"  # result files of one-vs-rest runs (before sqhinge_)
WEIGHTED_PREFIX = "weighted_"  # result files of runs with class / sample weights


def sweep_prefix(k: int) -> str:
    return f"sweep{k}_"


def cv_prefix(k: int) -> str:
    return f"cv{k}_"  # result files of fold model k of a cross-validation run (before sqhinge_)


@dataclass(frozen=True)
class ModelSpec:
    kind: str  # "single" | "softmax" | "ovr" | "sweep" | "cv"
    loss: int  # models/losses.py code, the weighted code of a weighted run; one-vs-rest: the binary loss
    weighted: bool  # class / sample weights: the labels carry them (data/source.py WeightedSource)
    classes: int  # softmax, one-vs-rest: the class blocks; 1 otherwise
    models: int  # sweep: its models; cv: its folds; 1 otherwise
    d_x: int  # the data's columns
    ld_x: int  # ... and row stride: one block of the model
    l1: float
    sweep_alpha: Optional[List[float]]  # the sweep's per-model lists, None without a sweep
    sweep_lr: Optional[List[float]]
    sweep_l1: Optional[List[float]]
    prec: Precision
    sparse: bool
    # cross-validation: K, the rows of every fold n_k = sum_p ceil((n_p - k) / K) over the run's partitions, and the
    # row count n of the run's gradient scale; 0 / None / 0 without --cv
    cv: int = 0
    fold_rows: Optional[Tuple[int, ...]] = None
    n_rows: int = 0

    # ---------------------------------------------------------------- resolution and rejections
    @classmethod
    def resolve(cls, cfg, scheme, sparse: bool, own_weights: bool, prec: Precision, gpu: bool) -> "ModelSpec":
        """The run's model from its config, scheme, data source (sparse; sample weights of its own), precision and
        whether the rank computes on a GPU.  Raises what the run cannot do, before anything is loaded."""
        if cfg.loss == "auto":
            loss = LEAST_SQUARES if (cfg.dataset == "kc_house_data" and scheme.has_linear) else LOGISTIC
        else:
            if cfg.loss not in LOSS_CHOICES:
                raise ValueError(f"unknown loss {cfg.loss!r}: auto or one of {sorted(LOSS_CHOICES)}")
            loss = LOSS_CHOICES[cfg.loss]
        # without weights the run takes exactly the code paths it takes without the feature
        weighted = bool(cfg.weighted or own_weights)
        if weighted and cfg.cv is not None:  # (a source that brings sample weights of its own; the flags are the
            raise ValueError("--cv: class / sample weights are not supported")  # config's to reject)
        if weighted:
            if loss not in (LOGISTIC, SQUARED_HINGE):
                name = {LEAST_SQUARES: "least squares", SOFTMAX: "softmax"}.get(loss, str(loss))
                raise ValueError(f"--class-weight / --sample-weights: not supported with the {name} loss (the label "
                                 f"cannot carry the weight there); logistic or squared_hinge")
            loss = weighted_kind(loss)
        kind, classes = "single", 1
        if loss == SOFTMAX:
            kind, classes = "softmax", check_classes(cfg.classes or 2)
        if cfg.ovr is not None:
            if loss == LEAST_SQUARES:
                raise ValueError("--ovr: --loss auto resolves to least squares for this run, which has no "
                                 "one-vs-rest form; name --loss logistic or squared_hinge")
            if weighted:  # (a source that brings sample weights of its own; the flags are the config's to reject)
                raise ValueError("--ovr: class / sample weights are not supported (the labels are class indices and "
                                 "cannot carry a weight)")
            kind, classes = "ovr", check_classes(cfg.ovr)
        sweep = cfg.sweep()
        if sweep:
            kind = "sweep"
        models, cv = (len(sweep) if sweep else 1), {}
        if cfg.cv is not None:
            kind, models = "cv", int(cfg.cv)
            # the fold counts, and with them n / (n - n_k), assume what the scheme does: equal partitions that add up
            # to n_rows (check_partitions holds the loaded partitions to it)
            if int(scheme.n_partition_files) * int(scheme.rows_per_partition) != int(cfg.n_rows):
                raise ValueError(f"--cv: n_rows = {cfg.n_rows} is not {scheme.n_partition_files} partitions of equal "
                                 f"size; the fold counts need n_rows to be a multiple of the partition count")
            per_part = CvGradPlan.fold_rows(scheme.rows_per_partition, models)
            cv = dict(cv=models, fold_rows=tuple(int(scheme.n_partition_files) * f for f in per_part),
                      n_rows=int(cfg.n_rows))
            if max(cv["fold_rows"]) >= cv["n_rows"]:
                raise ValueError(f"--cv: a fold holds every row ({cv['fold_rows']} of {cv['n_rows']}): its model "
                                 f"would have nothing to train on")
        d_x = int(cfg.n_cols)
        spec = cls(kind, loss, weighted, classes, models, d_x, prec.ld(d_x), float(cfg.l1),
                   [a for a, _ in sweep] if sweep else None, [x for _, x in sweep] if sweep else None,
                   cfg.sweep_l1s(), prec, bool(sparse), **cv)
        if kind == "softmax":
            SoftmaxGradPlan.check_supported(prec, classes, sparse)
        elif kind == "ovr":
            OvrGradPlan.check_supported(prec, loss, classes, sparse, spec.ld_x, gpu)
        elif kind == "sweep":
            MultiModelGradPlan.check_supported(prec, loss, spec.models, sparse, spec.ld_x, gpu)
        elif kind == "cv":
            CvGradPlan.check_supported(prec, loss, spec.models, sparse, spec.ld_x, gpu)
        return spec

    def check_partitions(self, parts, rows_per_partition: int) -> None:
        """A cross-validation run's loaded partitions {p: (X, y)} must have the scheme's rows each: fold_rows, and the
        scale of every fold model's gradient, are counted from that size.  Any other run: nothing to check."""
        if self.kind != "cv":
            return
        for p, (X, _) in sorted(parts.items()):
            if int(X.shape[0]) != int(rows_per_partition):
                raise ValueError(f"--cv: partition {p} has {X.shape[0]} rows, the scheme's partitions have "
                                 f"{rows_per_partition}: the fold counts n_k (and n / (n - n_k)) assume equal partitions")

    # ------------------------------------------------------------------------------- the layout
    @property
    def blocks(self) -> int:
        return self.classes * self.models

    @property
    def ld(self) -> int:
        """Everything model-sized (beta, messages, history rows) has this many elements."""
        return self.blocks * self.ld_x

    @property
    def d(self) -> int:
        """... of which the first d are stored per round: the data columns of a single model, else all."""
        return self.d_x if self.kind == "single" else self.ld

    @property
    def ovr(self) -> bool:
        return self.kind == "ovr"

    @property
    def per_model_scores(self) -> bool:
        """The run's scores carry a trailing model axis: the models of a sweep, the fold models of a cross-validation."""
        return self.kind in ("sweep", "cv")

    @property
    def cv_scale(self) -> Optional[np.ndarray]:
        """[K] n / (n - n_k): fold model k's mean is over the rows it trains on, so its gradient multiplier is the
        single model's times this; None without --cv."""
        if self.kind != "cv":
            return None
        n = float(self.n_rows)
        return np.array([n / (n - f) for f in self.fold_rows], dtype=np.float64)

    @property
    def blocked(self) -> bool:
        """The model is class-major blocks over class-index labels."""
        return self.kind in ("softmax", "ovr")

    @property
    def prox(self) -> bool:
        """L1 / elastic net: a soft threshold follows the update, only when some lambda > 0 -- a run whose lambdas
        are all 0 runs exactly the code it ran without them."""
        return any(x > 0 for x in (self.sweep_l1 if self.kind == "sweep" else [self.l1]))

    @property
    def label_classes(self) -> Optional[int]:
        """The classes a generated data set's labels index; None for labels in {-1, +1} / regression targets."""
        return self.classes if self.blocked else None

    def pack(self, x) -> np.ndarray:
        """[..., blocks, d_x] -> [..., ld]: every block in its ld_x columns, the padding columns zero."""
        x = np.asarray(x, dtype=np.float64)
        if x.shape[-2:] != (self.blocks, self.d_x):
            raise ValueError(f"expected [..., {self.blocks}, {self.d_x}], got {list(x.shape)}")
        out = np.zeros(x.shape[:-1] + (self.ld_x,))
        out[..., : self.d_x] = x
        return out.reshape(x.shape[:-2] + (self.ld,))

    def unpack(self, betaset) -> np.ndarray:
        """A trajectory [R, d] (or packed [R, ld]) viewed as [R, blocks, d_x]."""
        B = np.asarray(betaset)
        if B.ndim != 2 or B.shape[1] not in (self.d, self.ld):
            raise ValueError(f"expected [R, {self.d}] or [R, {self.ld}], got {list(B.shape)}")
        return B.reshape(B.shape[0], self.blocks, -1)[:, :, : self.d_x]

    def rows(self, betaset) -> np.ndarray:
        """A trajectory [R, d] as the [R * blocks, ld_x] model matrix of the evaluation GEMMs."""
        B = np.asarray(betaset, dtype=np.float64)
        full = np.zeros((B.shape[0], self.ld))
        full[:, : self.d] = B
        return full.reshape(B.shape[0] * self.blocks, self.ld_x)

    def beta0(self, init_zero: bool, seed: Optional[int]) -> np.ndarray:
        """beta_0 packed [ld]: randn (naive/replication/approx) or zeros (ref §2.2 'Per-scheme beta init').  Softmax
        and one-vs-rest draw classes * d_x values in one call; every model of a sweep starts from the single-model
        run's beta_0, and so does every fold model of a cross-validation."""
        nb = self.classes * self.d_x
        if init_zero:
            b0 = np.zeros(nb)
        elif seed is not None:
            b0 = np.random.RandomState(seed + 1).randn(nb)
        else:
            b0 = np.random.randn(nb)
        return self.pack(np.broadcast_to(b0.reshape(self.classes, 1, self.d_x),
                                         (self.classes, self.models, self.d_x)).reshape(self.blocks, self.d_x))

    def sparsity(self, betaset) -> Tuple[np.ndarray, np.ndarray]:
        """(nnz, l1 * ||beta||_1) of every iterate over the data columns: [R], or [R, M] for a sweep (softmax and
        one-vs-rest count over their class blocks: they are one model with one lambda)."""
        blocks = self.unpack(np.asarray(betaset, dtype=np.float64))
        if self.kind == "sweep":
            return np.count_nonzero(blocks, axis=2), np.abs(blocks).sum(axis=2) * np.asarray(self.sweep_l1, np.float64)
        if self.kind == "cv":  # [R, K]: every fold model with the run's one lambda
            return np.count_nonzero(blocks, axis=2), np.abs(blocks).sum(axis=2) * self.l1
        flat = blocks.reshape(blocks.shape[0], -1)
        return np.count_nonzero(flat, axis=1), np.abs(flat).sum(axis=1) * self.l1

    # --------------------------------------------------------------------------------- the plan
    def make_plan(self, messages, parts, cfg, device):
        """The gradient plan of this rank's messages (segments) over its resident partitions."""
        if self.kind == "softmax":
            return SoftmaxGradPlan(messages, parts, self.prec, self.classes, self.d_x)
        if self.kind == "ovr":
            return OvrGradPlan(messages, parts, self.prec, self.loss, self.classes, self.d_x)
        if self.kind == "sweep":
            return MultiModelGradPlan(messages, parts, self.prec, self.loss, self.models, self.d_x)
        if self.kind == "cv":
            return CvGradPlan(messages, parts, self.prec, self.loss, self.models, self.d_x)

        def one(msgs):
            if self.sparse:
                return SparseGradPlan(msgs, parts, self.prec, self.loss, self.d, device=device)
            kw = {"target_tasks": cfg.tasks} if cfg.tasks else {}
            if cfg.pack == "off":
                kw["pack"] = False
            return DenseGradPlan(msgs, parts, self.prec, self.loss, self.d, **kw)

        # (the blocked plans above stream every distinct partition once by themselves: --share-partitions
        # changes nothing for them)
        if cfg.share_partitions and SharedGradPlan.worthwhile(messages, lambda p: parts[p][0].shape[0]):
            return SharedGradPlan(messages, one)
        return one(messages)

    # ------------------------------------------------------------ how the run is scored and named
    @property
    def scoring(self) -> str:
        """"accuracy": class blocks scored by their loss and the test accuracy; "auc": labels in {-1, +1}, ROC AUC;
        "loss": a regression run, the loss alone."""
        if self.blocked:
            return "accuracy"
        return "auc" if is_classification(self.loss) else "loss"

    def scalar_models(self) -> List[Tuple[Optional[str], str, float]]:
        """(console header, result prefix, l1) of every model a scalar-loss run scores: a single model has no
        header and no prefix of its own."""
        if self.kind == "cv":  # n_k of n: the rows fold model k does not train on, of the objective's row count
            return [(">> Fold %d: held-out rows = %d of %d" % (k, self.fold_rows[k], self.n_rows), cv_prefix(k), self.l1)
                    for k in range(self.models)]
        if self.kind != "sweep":
            return [(None, "", self.l1)]
        return [(">> Model %d: alpha = %g, lr = %g" % (k, self.sweep_alpha[k], self.sweep_lr[k])
                 + (", l1 = %g" % self.sweep_l1[k] if self.prox else ""), sweep_prefix(k), self.sweep_l1[k])
                for k in range(self.models)]

    def per_model(self, a: np.ndarray) -> np.ndarray:
        """[R, M] scores as the run reports them: a trailing model axis only in a sweep or a cross-validation."""
        return a if self.per_model_scores else a[:, 0]

    def best(self, final: np.ndarray) -> Optional[int]:
        """A sweep's model with the lowest final test loss [M] (non-finite ones last); None otherwise."""
        if self.kind != "sweep":
            return None
        return int(np.argmin(np.where(np.isfinite(final), final, np.inf)))

    def result_names(self, names: Dict[str, str], model_prefix: str = "") -> Dict[str, str]:
        """The scheme's result names under the run's prefixes: ``sweep{k}_`` / ``cv{k}_`` first, then ``softmax_`` /
        ``ovr_``, ``weighted_``, ``sqhinge_``."""
        p = model_prefix + {"softmax": SOFTMAX_PREFIX, "ovr": OVR_PREFIX}.get(self.kind, "")
        p += (WEIGHTED_PREFIX if self.weighted else "") + (SQHINGE_PREFIX if base_kind(self.loss) == SQUARED_HINGE else "")
        return {k: p + v for k, v in names.items()}

    # ----------------------------------------------------------------------------- its identity
    def report(self) -> Dict[str, object]:
        """The model's fields of Trainer.rank_report()."""
        rep: Dict[str, object] = {}
        if self.kind == "sweep":
            rep.update(models=self.models, sweep_alpha=list(self.sweep_alpha), sweep_lr=list(self.sweep_lr))
        if self.kind == "ovr":
            rep.update(ovr=True, classes=self.classes)
        if self.kind == "cv":
            rep.update(cv=self.cv, fold_rows=list(self.fold_rows))
        rep.update(l1=list(self.sweep_l1) if self.kind == "sweep" else self.l1, prox=bool(self.prox),
                   weighted=bool(self.weighted))
        return rep

    def checkpoint_state(self, weight_spec) -> Dict[str, object]:
        """What a checkpoint says about the model; a feature the run does not use leaves its key out."""
        state: Dict[str, object] = {}
        if self.kind == "sweep":
            state["sweep_alpha"] = [float(a) for a in self.sweep_alpha]
            state["sweep_lr"] = [float(x) for x in self.sweep_lr]
            state["sweep_l1"] = [float(x) for x in self.sweep_l1]
        state["l1"] = self.l1
        if self.weighted:
            state["weights"] = weight_spec
        if self.kind == "ovr":
            state["ovr"] = int(self.classes)
        if self.kind == "cv":
            state["cv"] = int(self.cv)
        return state

    def check_checkpoint(self, st, path: str, weight_spec) -> None:
        """A checkpoint resumes only as the run that wrote it; an absent key: written without that feature."""
        sweep = self.kind == "sweep"
        if sweep or "sweep_alpha" in st:
            want = (self.sweep_alpha, self.sweep_lr)
            have = tuple(None if st.get(k) is None else [float(x) for x in st[k]] for k in ("sweep_alpha", "sweep_lr"))
            if have != want:
                raise ValueError(f"checkpoint {path} was written by a run with sweep lists alphas = {have[0]}, "
                                 f"lrs = {have[1]}; this run has alphas = {want[0]}, lrs = {want[1]}")
        have_l1 = float(st.get("l1", 0.0))
        if have_l1 != self.l1:
            raise ValueError(f"checkpoint {path} was written by a run with l1 = {have_l1:g}; this run has "
                             f"l1 = {self.l1:g}")
        if sweep:
            have_l1s = [float(x) for x in st["sweep_l1"]] if st.get("sweep_l1") is not None else [0.0] * self.models
            if have_l1s != [float(x) for x in self.sweep_l1]:
                raise ValueError(f"checkpoint {path} was written by a run with sweep_l1 = {have_l1s}; this run has "
                                 f"sweep_l1 = {list(self.sweep_l1)}")
        have_ovr, want_ovr = st.get("ovr"), (self.classes if self.kind == "ovr" else None)
        if have_ovr != want_ovr:
            raise ValueError(f"checkpoint {path} was written by a run with ovr = {have_ovr}; this run has "
                             f"ovr = {want_ovr} (--ovr)")
        have_cv, want_cv = st.get("cv"), (self.cv if self.kind == "cv" else None)
        if have_cv != want_cv:
            raise ValueError(f"checkpoint {path} was written by a run with cv = {have_cv}; this run has "
                             f"cv = {want_cv} (--cv)")
        have_w = st.get("weights")
        if have_w != weight_spec:
            raise ValueError(f"checkpoint {path} was written by a run with weights = {have_w}; this run has "
                             f"weights = {weight_spec} (--class-weight / --sample-weights)")
        if st["beta"].numel() != self.ld:
            raise ValueError("checkpoint beta has a different feature dimension")


@dataclass
class UpdateSchedule:
    """Every round's update coefficients, filled once per run from the UpdateRule (models/losses.py): B = the
    models of a sweep or the fold models of a cross-validation, 1 otherwise."""

    decay: np.ndarray  # [R, B]
    gm: np.ndarray  # [R, B]
    l2: np.ndarray  # [R, B]
    thr: Optional[np.ndarray]  # [R, B] soft thresholds; None when no lambda is positive
    theta: np.ndarray  # [R]
    code: int  # 0 GD, 1 AGD
    block_ld: int  # one block of the update: a sweep's model, otherwise the whole vector
    block_d: int
    # a sweep's pump is also given the single-model rows of the run's own (alpha, lr), [3, R]: decay, gm, l2
    single: np.ndarray

    @classmethod
    def build(cls, rule: UpdateRule, rounds: int, eta, sweep_etas, spec: ModelSpec) -> "UpdateSchedule":
        """eta: cfg.eta(); sweep_etas: cfg.sweep_etas(), [M, R] in a sweep."""
        R = int(rounds)
        co = [rule.coeffs(i, float(eta[i])) for i in range(R)]
        single = np.array([[c[k] for c in co] for k in range(3)], dtype=np.float64).reshape(3, R)
        theta = np.array([c[3] for c in co], dtype=np.float64)
        code = co[0][4] if co else 0
        if spec.kind == "sweep":
            B, block = spec.models, (spec.ld_x, spec.d_x)
            bco = [rule.block_coeffs(i, sweep_etas[:, i], spec.sweep_alpha) for i in range(R)]
            decay, gm, l2 = (np.array([c[k] for c in bco], dtype=np.float64).reshape(R, B) for k in range(3))
        elif spec.kind == "cv":  # every fold model takes the single-model coefficients; gm times n / (n - n_k)
            B, block = spec.models, (spec.ld_x, spec.d_x)
            decay, gm, l2 = (np.repeat(single[k].reshape(R, 1), B, axis=1) for k in range(3))
            gm = gm * spec.cv_scale[None, :]
        else:
            B, block = 1, (spec.ld, spec.d)
            decay, gm, l2 = (single[k].reshape(R, 1) for k in range(3))
        thr = None
        if spec.prox:  # the soft threshold eta_i * l1 (per model in a sweep)
            thr = [rule.block_thresholds(i, sweep_etas[:, i], spec.sweep_l1) if spec.kind == "sweep"
                   else [rule.threshold(i, float(eta[i]))] for i in range(R)]
            thr = np.array(thr, dtype=np.float64).reshape(R, -1)
            thr = np.repeat(thr, B, axis=1) if spec.kind == "cv" else thr.reshape(R, B)
        return cls(decay, gm, l2, thr, theta, code, *block, single)

    def apply(self, i: int, msgs, coefs, beta, u, hist, beta_w) -> None:
        """Round i's combine + update (ops/update.py): with a threshold the proximal form (a single model as one
        block), a sweep without one the blocked form, anything else the plain one."""
        theta = float(self.theta[i])
        if self.thr is not None:
            combine_update_prox(msgs, coefs, beta, u, self.block_ld, self.block_d, self.decay[i].tolist(),
                                self.gm[i].tolist(), self.l2[i].tolist(), self.thr[i].tolist(), theta, self.code,
                                hist=hist, beta_w=beta_w)
        elif self.decay.shape[1] > 1:  # every model block with its own (alpha_k, lr_k)
            combine_update_blocks(msgs, coefs, beta, u, self.block_ld, self.block_d, self.decay[i].tolist(),
                                  self.gm[i].tolist(), self.l2[i].tolist(), theta, self.code, hist=hist, beta_w=beta_w)
        else:
            combine_update(msgs, coefs, beta, u, self.block_d, float(self.decay[i, 0]), float(self.gm[i, 0]),
                           float(self.l2[i, 0]), theta, self.code, hist=hist, beta_w=beta_w)

    def install(self, pump, delays: List[float], rule_kind: int, rule_k: int, drain: bool) -> None:
        """The whole run's coefficients for a native MasterPump.  The delay table, the stop rule and the drain flag
        travel with set_schedule; they are the caller's."""
        pump.set_schedule(*(x.tolist() for x in self.single), self.theta.tolist(), self.code, delays, rule_kind,
                          rule_k, drain)
        if self.decay.shape[1] > 1:  # per-model (decay, gm, l2), flat [R * M]; theta and the rule are common
            pump.set_block_schedule(self.decay.shape[1], self.block_ld, self.block_d, self.decay.ravel().tolist(),
                                    self.gm.ravel().tolist(), self.l2.ravel().tolist())
        if self.thr is not None:  # soft thresholds [R] or [R * M]; the rounds then stay off both fused update paths
            pump.set_prox_schedule(self.thr.ravel().tolist())
