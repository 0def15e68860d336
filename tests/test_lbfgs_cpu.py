"""--lbfgs M on the CPU: the Gram-space twin of ops/update.py lbfgs_update against a long-double, vector-space two-loop
replay of the method (replay_step, shared with tests/test_lbfgs_gpu.py), the engine against a replay through
UpdateRule.step_lbfgs, the flag's rejections, checkpoints, reports and file names.  The bound of a raw step: the error
max|x - ref| / max|ref| of p, and that of beta', may be BOUND_FACTOR = 64 times what the SAME replay in float64 shows on
that quantity, floored at 2^-53 (reading the dots off V^T V costs up to 13.6 times the vector-space loop's error on
this input family; the rest is headroom for a summation order)."""
import numpy as np
import pytest
import torch

from erasurehead_amd import cli
from erasurehead_amd.engine import Trainer
from erasurehead_amd.models import losses
from erasurehead_amd.ops.update import lbfgs_pairs, lbfgs_state, lbfgs_update
from erasurehead_amd.parallel.dist import DistEnv
from test_multimodel_cpu import ARGV, CASES, make

LD = np.longdouble
BOUND_FACTOR, FLOOR = 64, 2.0 ** -53
DS, MS = (1, 3, 4, 5, 63, 257, 1000), (1, 3, 7)


def replay_step(T, msgs, coefs, beta, st, rg, d, eta, gs, l2c, tau):
    """One step of the method in the number type T, full-length vectors, on the state layout of lbfgs_state:
    (beta' [d], direction [d], state', ring')."""
    M = (st.shape[0] - 3) // 2
    st, (head, count, started) = np.array(st, dtype=T), (int(x) for x in rg[:3])
    b, g = np.asarray(beta[:d], T), np.zeros(d, T)
    for m, c in zip(msgs, coefs):
        g += T(c) * np.asarray(m[:d], T)
    with np.errstate(all="ignore"):
        G = T(gs) * g + T(l2c) * b
        if started:
            s, y = b - st[2 * M, :d], G - st[2 * M + 1, :d]
            sy, ss, yy = s @ y, s @ s, y @ y
            if np.isfinite([sy, ss, yy]).all() and sy > T(1e-8) * np.sqrt(ss * yy):
                slot = (head + count) % M if count < M else head
                st[slot, :d], st[M + slot, :d] = s, y
                head, count = (head, count + 1) if count < M else ((head + 1) % M, count)
        pairs = [(st[(head + j) % M, :d], st[M + (head + j) % M, :d]) for j in range(count)]
        mode, q = 1, G
        if pairs:
            q, a = G.copy(), []
            for s, y in reversed(pairs):
                a.append((s @ q) / (s @ y))
                q = q - a[-1] * y
            q = q * ((pairs[-1][0] @ pairs[-1][1]) / (pairs[-1][1] @ pairs[-1][1]))
            for (s, y), aj in zip(pairs, reversed(a)):
                q = q + (aj - (y @ q) / (s @ y)) * s
            gp = G @ q
            mode = 0 if np.isfinite(gp) and gp > 0 else 2
            q = q if mode == 0 else G
        nb = b - T(tau) * q if mode == 0 else b - T(eta) * G
    st[2 * M, :d], st[2 * M + 1, :d], st[2 * M + 2, :d] = b, G, q
    return nb, q, st, [0 if mode == 2 else head, 0 if mode == 2 else count, 1, mode]


def case(D, M, nmsg, mdt=torch.float64, seed=0, candidate=1.0, newest=1.0):
    """A raw step's operands: a full ring of M pairs, s Gaussian, y = A s (A diagonal, spectrum in [1, 100]; the newest
    y times `newest`), G Gaussian from nmsg messages, a candidate of the family with y times `candidate`; ld = D + 3."""
    rng = np.random.RandomState(1000 * D + 10 * M + nmsg + seed)
    ld, A = D + 3, rng.uniform(1.0, 100.0, D)
    A[0], A[-1] = 1.0, 100.0
    co = dict(d=D, eta=0.3, gs=0.8, l2c=0.05, tau=0.9)
    msgs = [torch.from_numpy(np.pad(rng.randn(D), (0, 3))).to(mdt) for _ in range(nmsg)]
    coefs = rng.uniform(0.5, 1.5, nmsg) * np.where(np.arange(nmsg) % 3 == 1, -0.5, 1.0)
    beta = np.pad(rng.randn(D), (0, 3))
    G = co["gs"] * sum(c * m.double().numpy() for c, m in zip(coefs, msgs)) + co["l2c"] * beta
    state, ring = lbfgs_state(M, ld)
    st = state.numpy()
    st[:M, :D] = rng.randn(M, D)
    st[M:2 * M, :D] = A * st[:M, :D]
    head = M // 2  # the oldest pair sits mid-ring: the logical order wraps
    st[M + (head + M - 1) % M] *= newest
    s = rng.randn(D)
    st[2 * M, :D], st[2 * M + 1, :D] = beta[:D] - s, G[:D] - candidate * A * s
    ring[:] = torch.tensor([head, M, 1, 0], dtype=torch.int32)
    return msgs, coefs, torch.from_numpy(beta), state, ring, co


def rel(x, ref):
    return float(np.max(np.abs(np.asarray(x, LD) - ref)) / np.max(np.abs(ref)))


def check_step(run, D, M, nmsg, mdt=torch.float64, want_ring=None, **kw):
    """`run` (lbfgs_update on a device, returning beta, state, ring) on case(...) against the long-double replay: p and
    beta' each within its own bound, the ring word as the replay's.  Returns the two bounds (run = None: only that)."""
    msgs, coefs, beta, state, ring, co = case(D, M, nmsg, mdt, **kw)
    args = ([m.double().numpy() for m in msgs], coefs, beta.numpy().copy(), state.numpy().copy(), ring.tolist())
    nb, p, _, rg = replay_step(LD, *args, **co)
    nb64, p64 = replay_step(np.float64, *args, **co)[:2]
    bound_p, bound_b = BOUND_FACTOR * max(rel(p64, p), FLOOR), BOUND_FACTOR * max(rel(nb64, nb), FLOOR)
    if run is not None:
        assert rg == (want_ring or [(M // 2 + 1) % M, M, 1, 0])  # by default: accepted, the oldest pair evicted
        got_beta, got_state, got_ring = run(msgs, coefs, beta, state, ring, co)
        ep, eb = rel(got_state[2 * M + 2, :D], p), rel(got_beta[:D], nb)
        print(f"lbfgs step D={D} M={M} nmsg={nmsg} {mdt}: p {ep / bound_p:.3f} beta {eb / bound_b:.3f} of the bounds")
        assert got_ring.tolist() == rg and ep <= bound_p and eb <= bound_b, (ep, bound_p, eb, bound_b)
    return bound_p, bound_b


@pytest.mark.parametrize("nmsg", [1, 9])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", DS)
def test_cpu_twin_against_long_double(D, M, nmsg):
    def run(msgs, coefs, beta, state, ring, co):
        lbfgs_update(msgs, coefs, beta, state, ring, **co)
        return beta.numpy(), state.numpy(), ring

    check_step(run, D, M, nmsg)


@pytest.mark.parametrize("name,kw", [("naive", {}), ("frc", {}), ("naive", dict(d=5, rounds=7, loss="least_squares", lr=0.5))])
def test_engine_against_an_independent_replay(name, kw):
    """These schemes decode the whole gradient: step_lbfgs replays the run, and both end holding the same 3 pairs."""
    cfg, src, sch, parts = make(CASES[name], lbfgs=3, **dict(dict(lr=2.0), **kw))
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    res = tr.run()
    rule, eta, state = losses.UpdateRule("GD", cfg.alpha_value, cfg.n_rows), cfg.eta(), losses.LbfgsState(3)
    beta, want = tr.model.beta0(sch.init_zero, cfg.seed)[: cfg.n_cols].copy(), []
    for i in range(cfg.num_itrs):
        g = sum(losses.worker_grad(tr.model.loss, X, y, beta) for X, y in parts)
        rule.step_lbfgs(i, float(eta[i]), beta, g, state, cfg.lbfgs_step)
        want.append(beta.copy())
    np.testing.assert_allclose(res.betaset, want, rtol=1e-9, atol=1e-11)
    assert len(state.pairs) == 3 and tr.lbfgs_state[1].tolist() == [tr.lbfgs_state[1][0], 3, 1, 0]
    for got, pairs in zip(lbfgs_pairs(*tr.lbfgs_state), ([s for s, _ in state.pairs], [y for _, y in state.pairs])):
        np.testing.assert_allclose(got[:, : cfg.n_cols].numpy(), pairs, rtol=1e-7, atol=1e-9 * np.abs(pairs).max())
    assert tr.rank_report()["lbfgs"] == 3 and tr.rank_report()["lbfgs_step"] == 1.0
    assert all(v.startswith("lbfgs_") for v in tr.model.result_names({"a": "x.dat"}).values())


def test_checkpoint_and_resume_continue_the_trajectory(tmp_path):
    path = str(tmp_path / "ck.pt")
    cfg, src, sch, _ = make(CASES["naive"], lbfgs=2, lr=2.0)
    tr = Trainer(cfg, DistEnv(), src, scheme=sch)
    full = tr.run().betaset
    np.testing.assert_array_equal(tr.run().betaset, full)  # a second run starts without the first one's pairs
    cfg, src, sch, _ = make(CASES["naive"], lbfgs=2, lr=2.0, checkpoint_every=5, checkpoint_path=path, rounds=5)
    Trainer(cfg, DistEnv(), src, scheme=sch).run()
    st = torch.load(path, weights_only=True)
    assert st["lbfgs"] == 2 and st["lbfgs_step"] == 1.0 and tuple(st["lbfgs_state"].shape) == (7, st["beta"].numel())
    cfg, src, sch, _ = make(CASES["naive"], lbfgs=2, lr=2.0, resume=path)
    np.testing.assert_array_equal(Trainer(cfg, DistEnv(), src, scheme=sch).run().betaset, full)
    for kw in (dict(lbfgs=3), dict(lbfgs=2, lbfgs_step=0.5), {}):
        cfg, src, sch, _ = make(CASES["naive"], lr=2.0, resume=path, **kw)
        with pytest.raises(ValueError, match="--lbfgs"):
            Trainer(cfg, DistEnv(), src, scheme=sch).run()


@pytest.mark.parametrize("flags", [
    "--lbfgs 8", "--lbfgs -1", "--lbfgs-step 0 --lbfgs 3", "--lbfgs-step nan --lbfgs 3", "--lbfgs-step 0.5", "--lbfgs-step 1",
    "--lbfgs 3 --loss softmax", "--lbfgs 3 --ovr 3", "--lbfgs 3 --cv 2", "--lbfgs 3 --alphas 1e-3,1e-2", "--lbfgs 3 --lrs 1,2",
    "--lbfgs 3 --l1s 0,1e-3", "--lbfgs 3 --l1 1e-3", "--lbfgs 3 --precondition diag"])
def test_rejections_name_the_flag(flags):
    with pytest.raises(ValueError, match=flags.split()[0] + r"\b(?!-)"):
        cli.parse(ARGV + flags.split())


def test_agd_and_avoidstragg_are_rejected():
    with pytest.raises(ValueError, match="--lbfgs"):
        cli.parse(ARGV[:-1] + ["AGD", "--lbfgs", "3"])
    cfg, src, sch, _ = make((1, 0, 2, 7, 2, 0), lbfgs=3)  # avoidstragg: always AGD
    with pytest.raises(ValueError, match="--lbfgs"):
        Trainer(cfg, DistEnv(), src, scheme=sch)
    cfg = cli.parse(ARGV + ["--lbfgs", "5", "--lbfgs-step", "0.5"])[0]
    assert sch.fixed_agd and (cfg.lbfgs, cfg.lbfgs_step) == (5, 0.5) and cli.parse(ARGV)[0].lbfgs == 0
