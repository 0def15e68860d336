"""Class and sample weights on the CPU: flags and rejections, unit weights against the unweighted run, trajectories
against this file's own NumPy replay of the weighted objective, evaluation, what a weight means (integer weights are
row duplication; balanced weights help the minority class), files, and checkpoints."""
import dataclasses
import os

import numpy as np
import pytest
import torch
from scipy.special import expit

import numerics as nx
import sample_weights_cases as sw
from erasurehead_amd import cli
from erasurehead_amd.codes import make_scheme
from erasurehead_amd.codes.schemes import Arrival
from erasurehead_amd.config import RunConfig
from erasurehead_amd.data.source import ArraySource, WeightedSource, balanced_class_weights
from erasurehead_amd.data.synthetic import generate_to_disk
from erasurehead_amd.engine import Trainer, evaluate
from erasurehead_amd.models import losses
from erasurehead_amd.models.losses import UpdateRule
from erasurehead_amd.ops import get_precision
from erasurehead_amd.ops.eval import auc_columns, sign_labels
from erasurehead_amd.parallel.dist import DistEnv
from test_multimodel_cpu import CASES, TOL, arrival_sets, make

ARGV = ["5", "400", "20", "/tmp/eh_sw_cli/", "0", "synthetic", "0", "0", "0", "0", "0", "0", "GD"]
BASE = dict(n_procs=5, n_rows=400, n_cols=20, input_dir="/tmp/x")
LR = {"logistic": 1.0, "squared_hinge": 0.1}
ALPHAS = [1e-3, 1e-2, 1e-1]
CW = (3.0, 0.5)


def draw_weights(parts, seed=11):
    """Per-partition weights in [0.25, 3) with about 10 % exact zeros."""
    rng = np.random.RandomState(seed)
    out = []
    for _, y in parts:
        w = rng.uniform(0.25, 3.0, len(y))
        w[rng.uniform(size=len(y)) < 0.1] = 0.0
        out.append(w)
    return out


def make_weighted(case, rule="GD", loss="logistic", weights=draw_weights, class_weight="3:0.5", sparse=False, **kw):
    kw.setdefault("lr", LR[loss])
    cfg, src, sch, parts = make(case, rule, loss=loss, class_weight=class_weight, **kw)
    wts = weights(parts) if callable(weights) else weights
    test = src._test
    if sparse:
        import scipy.sparse as sps

        src = ArraySource([(sps.csr_matrix(X), y) for X, y in parts], (sps.csr_matrix(test[0]), test[1]), sparse=True,
                          weights=wts)
    else:
        src = ArraySource(parts, test, weights=wts)
    return cfg, src, sch, parts, wts


def run(cfg, src, sch):
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    return tr, res


# ---- this file's replay of the weighted objective (1/n) sum w_i l(s_i, x_i beta) + alpha |beta|^2 (+ l1 |beta|_1)
def weighted_grad(loss, X, s, w, beta, coef):
    z = X @ beta
    if loss == "logistic":
        r = -coef * s * w * expit(-s * z)
    else:
        r = -2.0 * coef * s * w * np.maximum(0.0, 1.0 - s * z)
    return X.T @ r


def weighted_loss(loss, s, w, p):
    t = s * p
    if loss == "logistic":
        return w * (np.maximum(-t, 0.0) + np.log1p(np.exp(-np.abs(t))))
    return w * np.maximum(0.0, 1.0 - t) ** 2


def replay(loss, scheme, parts, wts, cw, beta0, arrivals_log, rule, alpha, n, eta, l1=0.0):
    up = UpdateRule("AGD" if scheme.fixed_agd else rule, alpha, n, scheme.grad_scale(), l1)
    beta = np.array(beta0, dtype=np.float64)
    u = np.zeros_like(beta)
    full = [np.where(y > 0, cw[0], cw[1]) * w for (_, y), w in zip(parts, wts)]
    out = []
    for i, arr in enumerate(arrivals_log):
        used = scheme.decode([Arrival(w, p, t) for (w, p, t) in arr])
        g = np.zeros_like(beta)
        for (w, part), c in used.items():
            m = [x for x in scheme.messages if x.worker == w and x.part == part][0]
            g += c * sum(weighted_grad(loss, parts[p][0], parts[p][1], full[p], beta, coef) for p, coef in m.segments)
        up.apply(i, eta[i], beta, u, g)
        out.append(beta.copy())
    return np.array(out)


# ---- 1. flags and rejections
def test_flags_parse(capsys):
    cfg, _ = cli.parse(ARGV)
    assert cfg.class_weight is None and cfg.sample_weights is None and not cfg.weighted
    cfg, _ = cli.parse(ARGV + ["--class-weight", "balanced"])
    assert cfg.class_weight == "balanced" and cfg.weighted
    cfg, _ = cli.parse(ARGV + ["--class-weight", "2:0.5", "--loss", "squared_hinge"])
    assert cfg.class_weight == (2.0, 0.5)
    cfg, _ = cli.parse(ARGV[:5] + ["x"] + ARGV[6:] + ["--sample-weights", "/tmp/w.dat", "--class-weight", "1:4"])
    assert cfg.sample_weights == "/tmp/w.dat" and cfg.class_weight == (1.0, 4.0) and cfg.weighted
    assert RunConfig(**BASE, class_weight=(2, 1)).class_weight == (2.0, 1.0)
    assert dataclasses.replace(RunConfig(**BASE, class_weight="2:1"), lr=3.0).class_weight == (2.0, 1.0)
    # the weighted codes are the engine's: no --loss name selects them
    assert set(losses.LOSS_NAMES.values()) == {0, 1, 2} and set(losses.LOSS_CHOICES.values()) == {0, 1, 2, 3}
    assert losses.weighted_kind(0) == 4 and losses.weighted_kind(2) == 5
    assert losses.base_kind(4) == 0 and losses.base_kind(5) == 2 and losses.base_kind(1) == 1
    for k in (1, 3, 4, 5, 7):
        with pytest.raises(ValueError):
            losses.weighted_kind(k)
    assert losses.is_classification(4) and losses.is_classification(5)
    capsys.readouterr()


@pytest.mark.parametrize("bad", ["1", "1:2:3", "a:b", "0:1", "1:-2", "nan:1", "1:inf", ""])
def test_class_weight_that_does_not_parse_or_is_not_positive(bad):
    with pytest.raises(ValueError, match="--class-weight"):
        RunConfig(**BASE, class_weight=bad)


def test_rejections_name_the_flag(tmp_path):
    for loss in ("least_squares", "softmax"):
        with pytest.raises(ValueError, match="--class-weight"):
            RunConfig(**BASE, loss=loss, class_weight="1:1")
        with pytest.raises(ValueError, match="--sample-weights"):
            RunConfig(**BASE, loss=loss, sample_weights="/tmp/w.dat")
    with pytest.raises(ValueError, match="--sample-weights"):
        RunConfig(**BASE, data="synthetic", sample_weights="/tmp/w.dat")
    # auto on kc_house_data is least squares
    cfg, src, sch, parts = make(CASES["naive"], "GD", loss="auto", class_weight="1:1")
    cfg.dataset = "kc_house_data"
    with pytest.raises(ValueError, match="--class-weight"):
        Trainer(cfg, DistEnv(), src, scheme=sch)
    # an ArraySource's own weights with least squares
    cfg, src, sch, parts = make(CASES["naive"], "GD", loss="least_squares")
    with pytest.raises(ValueError, match="--sample-weights"):
        Trainer(cfg, DistEnv(), ArraySource(parts, src._test, weights=[np.ones(len(y)) for _, y in parts]), scheme=sch)
    # a negative, NaN or infinite weight; a vector of the wrong length
    for bad in (-1.0, float("nan"), float("inf")):
        wts = [np.ones(len(y)) for _, y in parts]
        wts[1][3] = bad
        with pytest.raises(ValueError, match="weight"):
            ArraySource(parts, src._test, weights=wts)
    with pytest.raises(ValueError, match="weights"):
        ArraySource(parts, src._test, weights=[np.ones(len(y) + 1) for _, y in parts])
    with pytest.raises(ValueError, match="partitions"):
        ArraySource(parts, src._test, weights=[np.ones(40)])
    # labels other than +-1
    cfg, src, sch, parts = make(CASES["naive"], "GD", class_weight="2:1")
    zero_one = [(X, (y > 0).astype(np.float64)) for X, y in parts]
    with pytest.raises(ValueError, match=r"\{-1, \+1\}"):
        Trainer(cfg, DistEnv(), ArraySource(zero_one, src._test), scheme=sch)
    cfg.class_weight = "balanced"
    with pytest.raises(ValueError, match=r"\{-1, \+1\}"):
        Trainer(cfg, DistEnv(), ArraySource(zero_one, src._test), scheme=sch)
    # balanced: a class without rows
    with pytest.raises(ValueError, match="balanced"):
        Trainer(cfg, DistEnv(), ArraySource([(X, np.ones(len(y))) for X, y in parts], src._test), scheme=sch)


def test_balanced_is_n_over_two_n_c():
    assert balanced_class_weights(2, 6) == (8 / 4.0, 8 / 12.0)
    y = np.array([1.0, 1, 1, -1, 1, 1, 1, 1, -1, 1])  # hand-made: 8 positive, 2 negative
    cfg, src, sch, parts = make(CASES["naive"], "GD", class_weight="balanced")
    hand = [(X, np.resize(y, len(yy))) for X, yy in parts]  # 40 rows per partition: 32 positive, 8 negative
    tr = Trainer(cfg, DistEnv(), ArraySource(hand, src._test), scheme=sch)
    n, n_pos = 160, 128
    assert tr.class_weight == (n / (2.0 * n_pos), n / (2.0 * (n - n_pos))) == (0.625, 2.5)
    rep = tr.rank_report()
    assert rep["weighted"] is True and rep["class_weight"] == [0.625, 2.5] and rep["weight_sum_over_n"] == 1.0
    y0 = tr._parts[0][1].numpy()
    np.testing.assert_array_equal(y0, np.where(hand[0][1] > 0, 0.625, -2.5))
    with pytest.raises(ValueError, match="no training rows"):
        balanced_class_weights(5, 0)


def test_the_default_run_takes_todays_paths():
    cfg, src, sch, parts = make(CASES["agc_uneven"], "AGD")
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    assert tr.loss == losses.LOGISTIC and not tr.weighted and tr.source is src and tr.weight_spec is None
    rep = tr.rank_report()
    assert rep["weighted"] is False and rep["class_weight"] is None and rep["weight_sum_over_n"] is None


# ---- 2. unit weights: the unweighted run, bit for bit
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("loss", ["logistic", "squared_hinge"])
def test_unit_class_weights_give_the_unweighted_betaset(loss, rule, sparse):
    cfg, src, sch, parts, _ = make_weighted(CASES["agc_uneven"], rule, loss, weights=None, class_weight=None, sparse=sparse)
    _, plain = run(cfg, src, sch)
    cfg, src, sch, parts, _ = make_weighted(CASES["agc_uneven"], rule, loss, weights=None, class_weight="1:1",
                                            sparse=sparse)
    tr, res = run(cfg, src, sch)
    assert tr.weighted and tr.loss == losses.weighted_kind(losses.LOSS_NAMES[loss]) and tr.source.is_sparse == sparse
    assert arrival_sets(res) == arrival_sets(plain)
    np.testing.assert_array_equal(res.betaset, plain.betaset)
    # and so do unit sample weights
    ones = [np.ones(len(y)) for _, y in parts]
    cfg, src, sch, parts, _ = make_weighted(CASES["agc_uneven"], rule, loss, weights=ones, class_weight=None, sparse=sparse)
    tr, res = run(cfg, src, sch)
    assert tr.weighted and tr.weight_spec["sample_sha256"] is not None
    np.testing.assert_array_equal(res.betaset, plain.betaset)


# ---- 3. trajectories against the replay
@pytest.mark.parametrize("loss", ["logistic", "squared_hinge"])
@pytest.mark.parametrize("rule", ["GD", "AGD"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_engine_matches_the_weighted_replay(name, rule, loss):
    cfg, src, sch, parts, wts = make_weighted(CASES[name], rule, loss)
    tr, res = run(cfg, src, sch)
    assert tr.class_weight == CW and 0 < tr.weight_sum_over_n
    ref = replay(loss, sch, parts, wts, CW, tr.beta0, res.arrivals, rule, cfg.alpha_value, cfg.n_rows, cfg.eta())
    np.testing.assert_allclose(res.betaset, ref, **TOL)
    ones = [np.ones(len(y)) for _, y in parts]
    plain = replay(loss, sch, parts, ones, (1.0, 1.0), tr.beta0, res.arrivals, rule, cfg.alpha_value, cfg.n_rows,
                   cfg.eta())
    assert not np.allclose(ref, plain)  # the weights do change the trajectory


def test_csr_source_matches_the_weighted_replay():
    cfg, src, sch, parts, wts = make_weighted(CASES["cyclic"], "AGD", "squared_hinge", sparse=True)
    tr, res = run(cfg, src, sch)
    ref = replay("squared_hinge", sch, parts, wts, CW, tr.beta0, res.arrivals, "AGD", cfg.alpha_value, cfg.n_rows,
                 cfg.eta())
    np.testing.assert_allclose(res.betaset[:, : tr.d_x], ref, **TOL)


def test_weights_with_l1_match_the_replay():
    cfg, src, sch, parts, wts = make_weighted(CASES["agc_uneven"], "AGD", l1=0.02)
    tr, res = run(cfg, src, sch)
    assert tr.prox and tr.weighted
    ref = replay("logistic", sch, parts, wts, CW, tr.beta0, res.arrivals, "AGD", cfg.alpha_value, cfg.n_rows, cfg.eta(),
                 l1=0.02)
    np.testing.assert_allclose(res.betaset, ref, **TOL)
    np.testing.assert_array_equal(res.betaset == 0, ref == 0)
    assert 0 < np.count_nonzero(ref[-1]) < 33


def test_a_three_model_sweep_with_weights_matches_the_replay():
    cfg, src, sch, parts, wts = make_weighted(CASES["frc"], "GD", sweep_alpha=ALPHAS)
    tr, res = run(cfg, src, sch)
    assert tr.models == 3 and tr.loss == losses.LOGISTIC_W
    got = losses.sweep_unpack(res.betaset, 3, tr.d_x)
    etas = cfg.sweep_etas()
    b0 = tr.beta0.reshape(3, tr.ld_x)[0, : tr.d_x]
    for k in range(3):
        ref = replay("logistic", sch, parts, wts, CW, b0, res.arrivals, "GD", ALPHAS[k], cfg.n_rows, etas[k])
        np.testing.assert_allclose(got[:, k], ref, **TOL)
    ev = evaluate(tr, res, write=False)
    assert ev.training_loss.shape == (8, 3)


def test_a_weighted_sweep_on_a_gpu_is_rejected_by_name():
    """The multi-model GPU kernel has no weighted instance: the limit is a ValueError that names the flags, raised by
    the plan's check (which the trainer calls before it loads anything); CPU tensors run every code."""
    from erasurehead_amd.ops.multimodel import LOSSES, MultiModelGradPlan

    assert LOSSES == (0, 1, 2, 4, 5)
    prec = get_precision("fp64")
    for code in (4, 5):
        MultiModelGradPlan.check_supported(prec, code, 3)
        with pytest.raises(ValueError, match="--class-weight / --sample-weights"):
            MultiModelGradPlan.check_supported(prec, code, 3, ld_x=34, gpu=True)
    RunConfig(**BASE, class_weight="2:1", sweep_alpha=ALPHAS)  # the configuration does not know the device


# ---- 4. evaluation
def test_reported_losses_are_the_weighted_means_and_the_auc_is_unweighted(tmp_path):
    for loss in ("logistic", "squared_hinge"):
        cfg, src, sch, parts, wts = make_weighted(CASES["naive"], "GD", loss)
        cfg.input_dir, cfg.verbose = str(tmp_path) + "/", True
        tr = Trainer(cfg, DistEnv(), src, scheme=sch)
        lines = []
        res = tr.run(log=lines.append)
        ev = evaluate(tr, res, log=lines.append)
        Xt, yt = src._test
        used = range(len(parts) - 1)  # the reference's evaluation skips the last partition
        n_train = sum(len(parts[p][1]) for p in used)
        assert ev.n_train == n_train and ev.n_test == len(yt)
        for r, beta in enumerate(res.betaset):
            tl = sum(weighted_loss(loss, parts[p][1], np.where(parts[p][1] > 0, *CW) * wts[p], parts[p][0] @ beta).sum()
                     for p in used) / n_train
            np.testing.assert_allclose(ev.training_loss[r], tl, **TOL)
            te = weighted_loss(loss, yt, np.where(yt > 0, *CW), Xt @ beta).mean()  # test rows: the class weights
            np.testing.assert_allclose(ev.testing_loss[r], te, **TOL)
            assert ev.auc[r] == pytest.approx(losses.roc_auc(yt, Xt @ beta), rel=1e-12)
        # the objective's n is the row count, not sum w
        rows = sum(len(y) for _, y in parts)
        total = sum((np.where(y > 0, *CW) * w).sum() for (_, y), w in zip(parts, wts))
        assert tr.weight_sum_over_n == pytest.approx(total / rows, rel=1e-14) and abs(total / rows - 1) > 0.1
        # the console line, before the usual ones, and the file names
        first = ">> Weights: class_weight = 3:0.5, w+ = 3, w- = 0.5, sum w / n = %g" % tr.weight_sum_over_n
        eval_lines = lines[lines.index(first):]
        assert eval_lines[1].startswith("Total Time Elapsed") and eval_lines[-1] == ">>> Done"
        plain = tr.scheme.output_names(cfg.fix_quirks)
        prefix = "weighted_" + ("sqhinge_" if loss == "squared_hinge" else "")
        assert {k: os.path.basename(v) for k, v in ev.files.items()} == {k: prefix + v for k, v in plain.items()}
        assert all(os.path.exists(v) for v in ev.files.values())
    # a sweep: sweep{k}_ first
    cfg, src, sch, parts, wts = make_weighted(CASES["naive"], "GD", "squared_hinge", sweep_alpha=ALPHAS[:2])
    cfg.input_dir = str(tmp_path) + "/"
    tr, res = run(cfg, src, sch)
    ev = evaluate(tr, res)
    assert os.path.basename(ev.files["sweep1_auc"]) == "sweep1_weighted_sqhinge_" + plain["auc"]


class ZeroWeightTest(WeightedSource):
    """A weighted source whose TEST labels carry sample weights too (here: some of them zero, on both classes)."""

    def __init__(self, inner, class_weight, test_w):
        super().__init__(inner, class_weight)
        self.test_w = test_w

    def test(self, prec, device):
        X, y = self.inner.test(prec, device)
        return X, self.weigh(y, self.test_w)


def test_zero_weight_rows_of_both_signs_keep_their_class_in_the_auc():
    cfg, src, sch, parts, wts = make_weighted(CASES["naive"], "GD")
    tr, res = run(cfg, src, sch)
    Xt, yt = src._test
    w = np.ones(len(yt))
    w[:20] = 0.0
    assert {-1.0, 1.0} == set(yt[:20])  # both classes among the zero-weight rows
    plain = src
    plain.weights = None
    out = {}
    for name, tw in (("zeros", w), ("ones", np.ones(len(yt)))):
        tr.source = ZeroWeightTest(plain, CW, tw)
        _, lab = tr.source.test(tr.prec, "cpu")
        if name == "zeros":
            z = lab.numpy()[:20]
            assert np.all(z == 0) and set(np.signbit(z)) == {True, False}
        out[name] = evaluate(tr, res, write=False)
    np.testing.assert_array_equal(out["zeros"].auc, out["ones"].auc)
    assert out["zeros"].auc[-1] == pytest.approx(losses.roc_auc(yt, Xt @ res.betaset[-1]), rel=1e-12)
    assert np.all(out["zeros"].testing_loss < out["ones"].testing_loss)
    # the operator itself
    yz = torch.tensor([0.0, -0.0, 2.5, -0.25, -0.0, 0.0, 1.0, -3.0], dtype=torch.float64)
    s = sign_labels(yz)
    assert s.tolist() == [1.0, -1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0]
    P = torch.tensor(np.random.RandomState(0).randn(8, 3))
    want = [losses.roc_auc(s.numpy(), P[:, j].numpy()) for j in range(3)]
    np.testing.assert_allclose(auc_columns(s, P), want, rtol=1e-12)


def test_numpy_and_torch_forms_of_the_codes_agree_with_the_long_double_oracle():
    """models/losses.py, ops/grad.py and ops/eval.py on hostile weights against tests/sample_weights_cases.py."""
    from erasurehead_amd.ops.eval import _loss_torch
    from erasurehead_amd.ops.grad import _residual_torch

    prec = get_precision("fp64")
    parts, weights, host, beta, bh = sw.dense_case(prec, 37)
    for code in sw.WEIGHTED:
        for p in (0, 1, 2):
            yt = sw.carry(parts[p][1].numpy(), weights[p])
            ref, bound = sw.message(code, [(p, -0.7)], {p: (host[p], yt)}, bh, prec)
            nx.check_columns(losses.worker_grad(code, host[p], yt, bh, -0.7), ref, bound, f"numpy code {code}")
            X = torch.from_numpy(host[p])
            r = _residual_torch(code, X @ torch.from_numpy(bh), torch.from_numpy(yt), torch.tensor(-0.7, dtype=torch.float64))
            nx.check_columns((X.t() @ r).numpy(), ref, bound, f"torch code {code}")
            Bh = np.stack([bh, 0.1 * bh])
            P, dP, sref, ds = sw.evaluation(code, host[p], yt, Bh, prec)
            got = _loss_torch(code, torch.from_numpy(yt), torch.from_numpy(host[p] @ Bh.T)).numpy()
            assert np.all(np.abs(got.astype(nx.LD) - sref) <= ds)
            f = losses.logistic_w_loss if code == 4 else losses.squared_hinge_w_loss
            assert abs(f(yt, host[p] @ bh) * len(yt) - float(sref[0])) <= float(ds[0])
        # unit weights: the unweighted functions' values, bit for bit; zero weights: exactly zero
        y = parts[0][1].numpy()
        np.testing.assert_array_equal(losses.worker_grad(code, host[0], y, bh, 1.5),
                                      losses.worker_grad(sw.BASE[code], host[0], y, bh, 1.5))
        z = sw.mixed_zeros(np.random.RandomState(0), len(y))
        assert np.all(losses.worker_grad(code, host[0], z, bh, 1.5) == 0.0)


@pytest.mark.parametrize("prec_name", ["fp64", "fp32"])
@pytest.mark.parametrize("d,sizes", [(37, (257, 64, 1)), (1000, (64, 1))])
def test_a_sequential_reference_stays_inside_the_column_bounds(d, sizes, prec_name):
    """The bound is within a plain reference's reach: strictly sequential sums in the accumulator type."""
    prec = get_precision(prec_name)
    parts, weights, host, beta, bh = sw.dense_case(prec, d, sizes)
    dtype = np.float64 if prec_name == "fp64" else np.float32
    for code in sw.WEIGHTED:
        for p in range(len(sizes)):
            hostw = {p: (host[p], sw.carry(parts[p][1].double().numpy(), weights[p]))}
            ref, bound = sw.message(code, [(p, 1.0)], hostw, bh, prec)
            got = sw.sequential_message(code, [(p, 1.0)], hostw, bh, dtype)
            ratio = nx.column_ratio(got, ref, bound)
            print(prec_name, "d", d, "n", sizes[p], sw.IDS[code], "ratio", ratio)
            assert ratio <= 1.0


# ---- 5. what a weight means
@pytest.mark.parametrize("loss", ["logistic", "squared_hinge"])
def test_integer_weights_are_row_duplication(loss):
    rng = np.random.RandomState(5)
    cfg, src, sch, parts = make(CASES["naive"], "AGD", loss=loss, lr=LR[loss])
    ints = [rng.randint(1, 4, len(y)).astype(np.float64) for _, y in parts]
    tr, res = run(cfg, ArraySource(parts, src._test, weights=ints), sch)
    assert tr.weighted and tr.class_weight == (1.0, 1.0)
    dup = [(np.repeat(X, w.astype(int), axis=0), np.repeat(y, w.astype(int))) for (X, y), w in zip(parts, ints)]
    assert sum(len(y) for _, y in dup) > cfg.n_rows  # ... and the same n in the scale: cfg.n_rows stays
    tr2, res2 = run(cfg, ArraySource(dup, src._test), sch)
    assert not tr2.weighted
    np.testing.assert_array_equal(tr.beta0, tr2.beta0)
    np.testing.assert_allclose(res.betaset, res2.betaset, **TOL)


def test_balanced_weights_improve_the_minority_recall():
    rng = np.random.RandomState(2024)
    d, rows, W = 10, 200, 4
    wstar = rng.randn(d)

    def draw(n):
        X = rng.randn(n, d)
        X[:, -1] = 1.0  # a bias column: the model can place the threshold
        score = X @ wstar + 2.0 * rng.randn(n)  # overlapping classes
        return X, np.where(score > np.quantile(score, 0.9), 1.0, -1.0)  # 10 % positive

    parts = [draw(rows) for _ in range(W)]
    test = draw(2000)
    recall = {}
    for cw in (None, "balanced"):
        cfg = RunConfig(W + 1, rows * W, d, "/tmp/eh_sw_recall/", 0, "x", 0, 0, 0, 0, 0, 0, "GD", num_itrs=60, seed=0,
                        verbose=False, lr=1.0, class_weight=cw)
        sch = make_scheme("naive", W, 0, rows * W, 0, 0, rng=np.random.RandomState(7))
        tr, res = run(cfg, ArraySource(parts, test), sch)
        pred = test[0] @ res.betaset[-1]
        recall[cw] = float(np.mean(pred[test[1] > 0] > 0))
    print("minority recall", recall)
    assert recall["balanced"] - recall[None] > 0


# ---- 6. files: --sample-weights travels with label.dat
def test_a_sample_weight_file_follows_label_dat(tmp_path, capsys):
    n, d, W = 160, 6, 4
    data = str(tmp_path / "artificial-data" / f"{n}x{d}" / f"{W}") + "/"
    generate_to_disk(n, d, W, data, np.random.RandomState(1), verbose=False)
    label = np.loadtxt(data + "label.dat")
    w = np.random.RandomState(2).uniform(0.5, 2.0, n)
    w[::7] = 0.0
    wfile = str(tmp_path / "w.dat")
    np.savetxt(wfile, w, fmt="%.17g")

    def config(**kw):
        return RunConfig(W + 1, n, d, str(tmp_path) + "/", 0, "x", 0, 0, 0, 0, 0, 0, "GD", num_itrs=3, seed=0,
                         verbose=False, lr=1.0, **kw)

    tr = Trainer(config(sample_weights=wfile, class_weight="2:1"), DistEnv())
    rpw = n // W
    cw = np.where(label > 0, 2.0, 1.0)
    for p in range(W):
        np.testing.assert_array_equal(tr._parts[p][1].numpy(), (label * cw * w)[p * rpw:(p + 1) * rpw])
    # the evaluation's label prefix: partitions (1, 2) read labels -- and with them weights -- 0..2 rpw
    chunks = list(tr.source.train_eval_chunks([1, 2], tr.prec, "cpu"))
    got = np.concatenate([y.numpy() for _, y in chunks])
    np.testing.assert_array_equal(got, (label * cw * w)[: 2 * rpw])
    _, yt = tr.source.test(tr.prec, "cpu")
    lt = np.loadtxt(data + "label_test.dat")
    np.testing.assert_array_equal(yt.numpy(), lt * np.where(lt > 0, 2.0, 1.0))  # test rows: class weights only
    res = tr.run()
    ev = evaluate(tr, res)
    assert os.path.basename(ev.files["auc"]).startswith("weighted_")
    # the wrong length, and bad entries
    np.savetxt(wfile, w[:-1], fmt="%.17g")
    with pytest.raises(ValueError, match="--sample-weights"):
        Trainer(config(sample_weights=wfile), DistEnv())
    for bad in (-0.5, float("nan"), float("inf")):
        w2 = w.copy()
        w2[5] = bad
        np.savetxt(wfile, w2, fmt="%.17g")
        with pytest.raises(ValueError, match="--sample-weights"):
            Trainer(config(sample_weights=wfile), DistEnv())
    capsys.readouterr()


def test_cli_runs_balanced_weights_on_synthetic_data(capsys, tmp_path):
    argv = ["5", "160", "6", str(tmp_path) + "/", "0", "x", "0", "0", "0", "0", "0", "0", "GD"]
    rc = cli.main(argv + ["--data", "synthetic", "--device", "cpu", "--num-itrs", "3", "--lr", "1", "--seed", "0",
                          "--class-weight", "balanced"])
    assert rc == 0
    lines = capsys.readouterr().out.splitlines()
    head = [ln for ln in lines if ln.startswith(">> Weights: ")]
    assert len(head) == 1 and head[0].startswith(">> Weights: class_weight = balanced, w+ = ")
    assert head[0].endswith("sum w / n = 1")  # balanced weights keep the scale of the objective
    assert lines.index(head[0]) < min(i for i, ln in enumerate(lines) if ln.startswith("Iteration 0"))
    assert os.path.exists(os.path.join(str(tmp_path), "results", "weighted_naive_acc_auc.dat"))
    assert not os.path.exists(os.path.join(str(tmp_path), "results", "naive_acc_auc.dat"))


def test_three_gloo_ranks_use_rank_zeros_balanced_weights(tmp_path):
    import socket
    import subprocess
    import sys

    from erasurehead_amd.data.source import balanced_class_weights

    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "weights_gloo.npz")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]),
               EH_WEIGHTS_OUT=out, EH_WEIGHTS_DEVICE="cpu", EH_WEIGHTS_CASE="naive")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", f"--master-port={port}", os.path.join(here, "mp_sample_weights_run.py")]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    z = np.load(out, allow_pickle=True)
    cfg, src, sch, parts, wts = make_weighted(CASES["naive"], "AGD", class_weight="balanced")
    y = np.concatenate([yy for _, yy in parts])
    cw = balanced_class_weights(int((y > 0).sum()), int((y < 0).sum()))
    assert bool(z["weighted"]) and tuple(z["class_weight"]) == cw
    arrivals = [[tuple(a) for a in rnd] for rnd in z["arrivals"]]
    ref = replay("logistic", sch, parts, wts, cw, z["beta0"], arrivals, "AGD", cfg.alpha_value, cfg.n_rows, cfg.eta())
    np.testing.assert_allclose(np.asarray(z["betaset"])[:, :33], ref, **TOL)
    total = sum((np.where(yy > 0, *cw) * w).sum() for (_, yy), w in zip(parts, wts))
    assert float(z["weight_sum_over_n"]) == pytest.approx(total / len(y), rel=1e-12)  # over every rank's partitions


# ---- 7. checkpoints
def test_checkpoint_resumes_bitwise_and_refuses_another_specification(tmp_path):
    ck = str(tmp_path / "ck.pt")
    cfg, src, sch, parts, wts = make_weighted(CASES["cyclic"], "AGD")
    _, full = run(cfg, src, sch)
    cfg4, src, sch, parts, wts = make_weighted(CASES["cyclic"], "AGD", rounds=4, checkpoint_every=4, checkpoint_path=ck)
    tr4, _ = run(cfg4, src, sch)
    st = torch.load(ck, weights_only=True)
    assert st["weights"] == tr4.weight_spec == {"class_weight": [3.0, 0.5], "sample_sha256": st["weights"]["sample_sha256"]}
    assert len(st["weights"]["sample_sha256"]) == 64
    cfgr, src, sch, parts, wts = make_weighted(CASES["cyclic"], "AGD", resume=ck)
    _, resumed = run(cfgr, src, sch)
    np.testing.assert_array_equal(resumed.betaset, full.betaset)
    # other class weights, other sample weights, none at all
    cfgr, src, sch, parts, wts = make_weighted(CASES["cyclic"], "AGD", class_weight="3:1", resume=ck)
    with pytest.raises(ValueError, match="weights"):
        run(cfgr, src, sch)
    other = draw_weights(parts, seed=12)
    cfgr, src, sch, parts, wts = make_weighted(CASES["cyclic"], "AGD", weights=other, resume=ck)
    with pytest.raises(ValueError, match="sample_sha256"):
        run(cfgr, src, sch)
    cfgr, src, sch, parts = make(CASES["cyclic"], "AGD", resume=ck)
    with pytest.raises(ValueError, match="--class-weight"):
        run(cfgr, src, sch)
    # and an unweighted checkpoint does not resume as a weighted run
    plain = str(tmp_path / "plain.pt")
    cfgp, srcp, schp, _ = make(CASES["cyclic"], "AGD", rounds=4, checkpoint_every=4, checkpoint_path=plain)
    run(cfgp, srcp, schp)
    assert "weights" not in torch.load(plain, weights_only=True)
    cfgr, src, sch, parts, wts = make_weighted(CASES["cyclic"], "AGD", resume=plain)
    with pytest.raises(ValueError, match="weights = None"):
        run(cfgr, src, sch)
