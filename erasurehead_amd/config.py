"""Run configuration: the reference's 13 positional arguments + hard-coded constants + extensions.

Positional CLI (ref main.py:20-27):
  n_procs n_rows n_cols input_dir is_real dataset is_coded n_stragglers partitions coded_ver
  num_collect add_delay update_rule
Constants (ref main.py:31-53): num_itrs = 100, alpha = 1/n_rows, eta_i = 10.0 for every round.

Everything past the 13 positionals is an opt-in extension (``--flags`` in cli.py); the
defaults reproduce the reference, including its quirks, unless
``fix_quirks`` is set.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

SWEEP_MIN_MODELS, SWEEP_MAX_MODELS = 2, 8  # csrc/kernels/launchers.h kMinBlocks / kMaxBlocks
OVR_MIN_CLASSES, OVR_MAX_CLASSES = 2, 8  # likewise: the classes of a one-vs-rest run are the blocks
CV_MIN_FOLDS, CV_MAX_FOLDS = 2, 8  # likewise: the fold models of a cross-validation run are the blocks


def parse_class_weight(spec):
    """--class-weight: None, "balanced", or the weights (P, N) of the +1 and the -1 class from "P:N" / a pair."""
    if spec is None or spec == "balanced":
        return spec
    try:
        p, n = spec.split(":") if isinstance(spec, str) else spec
        p, n = float(p), float(n)
    except (TypeError, ValueError):
        raise ValueError(f"--class-weight: expected 'balanced' or P:N (two positive numbers), got {spec!r}") from None
    if not (np.isfinite(p) and np.isfinite(n) and p > 0 and n > 0):
        raise ValueError(f"--class-weight: P and N must be finite and > 0, got {spec!r}")
    return (p, n)


@dataclass
class RunConfig:
    n_procs: int
    n_rows: int
    n_cols: int
    input_dir: str
    is_real: int = 0
    dataset: str = "synthetic"
    is_coded: int = 0
    n_stragglers: int = 0
    partitions: int = 0
    coded_ver: int = 0
    num_collect: int = 0
    add_delay: int = 0
    update_rule: str = "GD"

    # ---- reference constants (ref main.py:31-46) ----------------------------------
    num_itrs: int = 100
    alpha: Optional[float] = None  # default 1 / n_rows
    lr: float = 10.0  # learning_rate_schedule = lr * ones(num_itrs)
    lr_schedule: Optional[List[float]] = None
    lr_kind: str = "const"  # const (ref default) | invscaling | exponential (ref main.py:40-46, commented there)
    lr_t0: float = 90.0  # invscaling: eta_i = lr * t0 / (i + t0), i = 1..R
    lr_decay: float = 0.98  # exponential: eta_i = lr * decay**i, i = 1..R (the regression schedule)

    # ---- extensions -----------------------------------------------------------------
    precision: str = "fp64"  # fp64 | fp32 | bf16 | fp32x64 worker compute (master state always fp64)
    loss: str = "auto"  # auto (reference dispatch) | logistic | least_squares | squared_hinge | softmax
    classes: Optional[int] = None  # softmax only: number of classes, 2..8 (default 2)
    # one-vs-rest over C = 2..8 classes with the logistic or the squared-hinge loss (auto: logistic): C binary models,
    # class k against the rest, trained from one pass over X per round (ops/ovr.py); labels are class indices
    ovr: Optional[int] = None
    # K-fold cross-validation, K = 2..8, of the run's scalar loss: K models that share (alpha, lr, l1), model k trained
    # without the rows of fold k, from one pass over X per round (ops/cv.py); row i of a partition is in fold i mod K
    cv: Optional[int] = None
    # (alpha, lr) sweep: M = 2..8 models trained in one run from one pass over X per round (ops/multimodel.py).
    # The lists are zipped; an absent list or one of length 1 is broadcast (absent: the run's alpha / lr).
    sweep_alpha: Optional[List[float]] = None
    sweep_lr: Optional[List[float]] = None
    # L1 strength (lambda) of the penalty l1 * ||beta||_1: a soft threshold eta_i * l1 after every update of the
    # master (lasso / elastic net with alpha; models/losses.py UpdateRule).  sweep_l1: one lambda per model of a
    # sweep, zipped with sweep_alpha / sweep_lr under the same rules; alone it makes a sweep of len(sweep_l1) models.
    l1: float = 0.0
    sweep_l1: Optional[List[float]] = None
    # Row weights of the +-1-label losses (logistic, squared hinge): the labels carry them to the kernels
    # (data/source.py WeightedSource, csrc/kernels/common.h kLogisticW / kSquaredHingeW).  class_weight: "balanced"
    # (n / (2 n_c) over the training labels) or "P:N" / (P, N), the weights of the +1 and the -1 class;
    # sample_weights: a file in label.dat's format and length, entry i the weight of label i.  The two multiply.
    class_weight: Optional[object] = None
    sample_weights: Optional[str] = None
    seed: Optional[int] = None  # beta_0 / B matrix seed (reference: unseeded)
    data: str = "files"  # files | synthetic (on-device generator, no files)
    data_seed: int = 0
    allow_uneven_groups: bool = False  # FRC with W % (s+1) != 0
    # straggler tail after the stop rule (engine/trainer.py): None = the scheme's reference behaviour
    # ("all" for FRC/AGC, ref src/approximate_coding.py:182-183; "carry" for the rest, which never
    # Waitall); "all" | "carry" | "lazy" (no wait + stale-round skipping on the workers)
    drain: Optional[str] = None
    delay_mode: str = "exp"  # exp (reference) | fixed | none
    # where an injected delay happens: "collector" (a virtual arrival time on the master's clock, the
    # GPUs never idle) or "worker" (the worker rank is physically late: its messages leave after a
    # device spin / host sleep, after compute and before the send, like the reference's time.sleep)
    delay_on: str = "collector"
    # rank -> factor: that rank runs its gradient `factor` times per round (a physically slower GPU)
    slow_ranks: Dict[int, int] = field(default_factory=dict)
    delay_mean: float = 0.5
    fixed_stragglers: List[int] = field(default_factory=list)  # 1-based worker ids (fixed mode)
    fixed_sleep: float = 0.5
    kill_workers: List[int] = field(default_factory=list)  # 1-based ids that never arrive
    force_delay: bool = False  # inject delays even where the reference does not
    round_timeout: float = 600.0  # master waits at most this long per round (dead worker -> erasure)
    fix_quirks: bool = False
    save_linear: bool = False  # reference comments the linear-model outputs out
    full_precision_outputs: bool = False
    evaluate: bool = True
    verbose: bool = True
    checkpoint_every: int = 0
    checkpoint_path: Optional[str] = None
    resume: Optional[str] = None
    trace: bool = False
    tasks: int = 0  # override gradient-kernel workgroup count
    verify_beta: bool = False  # race detector: workers checksum beta before/after use (Python loop)
    native_loop: bool = True  # GPU rounds in the C++ executors (csrc/runtime/master_pump.cpp, worker_pump.cpp)
    sync_update: bool = False  # host waits for every round's update kernel (else timed by HIP events)
    transport: str = "auto"  # auto | ipc | rccl | gloo (parallel/transport.py)
    device_loop: str = "auto"  # auto|graph|stream|off: device-driven rounds when eligible (trainer._device_loop_mode)
    share_partitions: bool = False  # co-located workers: distinct partitions once + device encode (ops/grad.py)
    pack: str = "auto"  # auto|off: long fp64 streams read the lossless 58-bit copy of X (ops/grad.py pack_auto)
    # simultaneous arrivals (add_delay = 0, or one kernel finishing several local workers): "permute"
    # orders them by a per-round permutation seeded by (tie_seed, round) (csrc/runtime/collector.h,
    # tie model); "worker" keeps worker-id order (AGC then stops on the same k workers every round)
    tie_break: str = "permute"
    tie_seed: int = 0
    # placement unit: "message" (a logical worker's whole message on one rank), "partition" (one
    # shard per (message, partition): each partition's replicas on one rank; parallel/placement.py)
    # or "auto" (partition when there are several ranks)
    shard: str = "auto"
    instrument: bool = False  # per-round HIP-event timing of puts / gradient launches (Trainer.rank_report)
    # IPC messages carry (round, rank, checksum) tags that the receiver verifies (csrc/kernels/integrity.h)
    integrity: bool = True
    # the reference topology's master: rank 0 runs the master only and hosts no logical worker (worker
    # w on rank 1 + w mod (world - 1); ref main.py:16-18, run_approx_coding.sh:47-49).  Default: rank 0
    # hosts workers too (one process per GPU, no GPU idles)
    dedicated_master: bool = False
    # per-round device records of every rank (beta put / message put / spin / gate stamps on the GPU
    # clocks) and the master's probe log, kept as Trainer.device_records (tests/lazy_check.py)
    device_records: bool = False

    def __post_init__(self):
        self.update_rule = str(self.update_rule)
        if self.update_rule not in ("GD", "AGD"):
            raise ValueError("update_rule must be GD or AGD")  # ref src/naive.py:13 assert
        self.input_dir = self.input_dir if self.input_dir.endswith("/") else self.input_dir + "/"
        if self.tie_break not in ("permute", "worker"):
            raise ValueError("tie_break must be permute or worker")
        if self.delay_mode == "worker":  # shorthand: the reference's Exp delays, slept on the worker rank
            self.delay_mode, self.delay_on = "exp", "worker"
        if self.delay_on not in ("collector", "worker"):
            raise ValueError("delay_on must be collector or worker")
        if self.drain not in (None, "all", "carry", "lazy"):
            raise ValueError("drain must be all, carry or lazy")
        if self.ovr is not None:
            self._check_ovr()
        if self.cv is not None:
            self._check_cv()
        if self.loss == "softmax":
            self.classes = 2 if self.classes is None else int(self.classes)
            if not 2 <= self.classes <= 8:
                raise ValueError(f"classes must be in 2..8, got {self.classes}")
        elif self.classes is not None:
            raise ValueError(f"classes is an option of the softmax loss, not of {self.loss!r}")
        if any(int(f) < 1 for f in self.slow_ranks.values()):
            raise ValueError("slow rank factors must be integers >= 1")
        self.l1 = float(self.l1)
        if not (np.isfinite(self.l1) and self.l1 >= 0):
            raise ValueError(f"l1 must be a finite value >= 0, got {self.l1}")
        self.sweep()  # the sweep's limits, each a ValueError that names it
        self.class_weight = parse_class_weight(self.class_weight)
        if self.weighted and self.loss in ("least_squares", "softmax"):
            raise ValueError(f"--class-weight / --sample-weights: not supported with --loss {self.loss} (the label "
                             f"cannot carry the weight there); logistic or squared_hinge")
        if self.sample_weights is not None and self.data == "synthetic":
            raise ValueError("--sample-weights: not with --data synthetic (there is no label.dat the file could match)")

    def _check_ovr(self) -> None:
        """The limits of a one-vs-rest run that the configuration alone decides, each a ValueError naming --ovr."""
        self.ovr = int(self.ovr)
        if not OVR_MIN_CLASSES <= self.ovr <= OVR_MAX_CLASSES:
            raise ValueError(f"--ovr: classes must be in {OVR_MIN_CLASSES}..{OVR_MAX_CLASSES}, got {self.ovr}")
        if self.loss in ("least_squares", "softmax"):
            raise ValueError(f"--ovr: not supported with --loss {self.loss} (one-vs-rest trains binary classifiers: "
                             f"logistic or squared_hinge; auto means logistic)")
        if self.classes is not None:
            raise ValueError("--ovr: cannot be combined with --classes (a softmax option); --ovr C gives the classes")
        if self.sweep_alpha is not None or self.sweep_lr is not None or self.sweep_l1 is not None:
            raise ValueError("--ovr: cannot be combined with a sweep (--alphas / --lrs / --l1s): the class blocks "
                             "share one (alpha, lr, l1)")
        if self.class_weight is not None or self.sample_weights is not None:
            raise ValueError("--ovr: --class-weight / --sample-weights are not supported (the labels are class "
                             "indices and cannot carry a weight)")

    def _check_cv(self) -> None:
        """The limits of a cross-validation run that the configuration alone decides, each a ValueError naming --cv."""
        self.cv = int(self.cv)
        if not CV_MIN_FOLDS <= self.cv <= CV_MAX_FOLDS:
            raise ValueError(f"--cv: folds must be in {CV_MIN_FOLDS}..{CV_MAX_FOLDS}, got {self.cv}")
        if self.loss == "softmax":
            raise ValueError("--cv: not supported with --loss softmax (the fold models are models of a scalar loss: "
                             "logistic, least_squares or squared_hinge)")
        if self.ovr is not None:
            raise ValueError("--cv: cannot be combined with --ovr (the blocks of the model are the folds)")
        if self.classes is not None:
            raise ValueError("--cv: cannot be combined with --classes (a softmax option)")
        if self.sweep_alpha is not None or self.sweep_lr is not None or self.sweep_l1 is not None:
            raise ValueError("--cv: cannot be combined with a sweep (--alphas / --lrs / --l1s): the fold models "
                             "share one (alpha, lr, l1)")
        if self.class_weight is not None or self.sample_weights is not None:
            raise ValueError("--cv: --class-weight / --sample-weights are not supported")
        if self.precision == "bf16":
            raise ValueError("--cv: bf16 storage is not supported (--precision fp64, fp32 or fp32x64)")
        if self.is_real and self.data != "synthetic":
            raise ValueError("--cv: sparse data sources are not supported (dense partitions only)")

    def _sweep_lists(self) -> Optional[Tuple[List[float], List[float], List[float]]]:
        """([alpha_k], [lr_k], [l1_k]) of a sweep run, every list broadcast to the M models; None without a list."""
        if self.sweep_alpha is None and self.sweep_lr is None and self.sweep_l1 is None:
            return None
        al = [float(a) for a in (self.sweep_alpha if self.sweep_alpha is not None else [self.alpha_value])]
        lr = [float(x) for x in (self.sweep_lr if self.sweep_lr is not None else [self.lr])]
        l1 = [float(x) for x in (self.sweep_l1 if self.sweep_l1 is not None else [self.l1])]
        if not al or not lr:
            raise ValueError("sweep: --alphas / --lrs must not be empty")
        if not l1:
            raise ValueError("sweep: --l1s must not be empty")
        if any(not (np.isfinite(x) and x >= 0) for x in l1):
            raise ValueError(f"sweep: every value of --l1s must be finite and >= 0, got {l1}")
        if self.sweep_l1 is not None and self.l1 != 0:
            raise ValueError("sweep: --l1s gives every model's L1 strength; it cannot be combined with --l1")
        if len(al) > 1 and len(lr) > 1 and len(al) != len(lr):
            raise ValueError(f"sweep: {len(al)} alphas and {len(lr)} lrs: lists longer than 1 must have equal lengths")
        longest = max(len(al), len(lr))
        if len(l1) > 1 and longest > 1 and len(l1) != longest:
            raise ValueError(f"sweep: {len(l1)} l1s against {longest} alphas / lrs: lists longer than 1 must have "
                             f"equal lengths")
        M = max(longest, len(l1))
        if not SWEEP_MIN_MODELS <= M <= SWEEP_MAX_MODELS:
            raise ValueError(f"sweep: {M} models; a sweep trains {SWEEP_MIN_MODELS}..{SWEEP_MAX_MODELS} models "
                             f"(give {SWEEP_MIN_MODELS} to {SWEEP_MAX_MODELS} values in --alphas or --lrs)")
        if self.sweep_lr is not None and self.lr_schedule is not None:
            raise ValueError("sweep: --lrs cannot be combined with an explicit lr_schedule (one list of step sizes)")
        if self.loss == "softmax":
            raise ValueError("sweep: --loss softmax is not supported with --alphas / --lrs "
                             "(logistic, least_squares, squared_hinge or auto)")
        al = al * M if len(al) == 1 else al
        lr = lr * M if len(lr) == 1 else lr
        l1 = l1 * M if len(l1) == 1 else l1
        return al, lr, l1

    def sweep(self) -> Optional[List[Tuple[float, float]]]:
        """The (alpha_k, lr_k) of every model of a sweep run, or None without --alphas / --lrs / --l1s."""
        sw = self._sweep_lists()
        return None if sw is None else list(zip(sw[0], sw[1]))

    def sweep_l1s(self) -> Optional[List[float]]:
        """The L1 strength of every model of a sweep run (--l1s, or --l1 broadcast), or None without a sweep."""
        sw = self._sweep_lists()
        return None if sw is None else list(sw[2])

    def sweep_etas(self) -> Optional[np.ndarray]:
        """[M, num_itrs]: model k's step schedule, eta() evaluated with lr = lr_k."""
        sw = self.sweep()
        if sw is None:
            return None
        return np.stack([dataclasses.replace(self, lr=lr, sweep_alpha=None, sweep_lr=None, sweep_l1=None).eta()[: self.num_itrs]
                         for _, lr in sw])

    @property
    def weighted(self) -> bool:
        """The run names class or sample weights (an ArraySource may still bring sample weights of its own)."""
        return self.class_weight is not None or self.sample_weights is not None

    @property
    def tie_seed_value(self) -> int:
        return int(self.tie_seed) if self.tie_break == "permute" else -1

    @property
    def n_workers(self) -> int:
        return self.n_procs - 1

    @property
    def alpha_value(self) -> float:
        return 1.0 / self.n_rows if self.alpha is None else self.alpha

    def eta(self) -> np.ndarray:
        if self.lr_schedule is not None:
            s = np.asarray(self.lr_schedule, dtype=np.float64)
            if len(s) < self.num_itrs:
                raise ValueError("lr_schedule shorter than num_itrs")
            return s
        i = np.arange(1, self.num_itrs + 1, dtype=np.float64)
        if self.lr_kind == "const":
            return self.lr * np.ones(self.num_itrs)
        if self.lr_kind == "invscaling":
            return self.lr * self.lr_t0 / (i + self.lr_t0)
        if self.lr_kind == "exponential":
            return self.lr * self.lr_decay ** i
        raise ValueError(f"unknown lr schedule {self.lr_kind!r}")
