"""--lbfgs M on the GPU: lbfgs_update (csrc/kernels/lbfgs.hip) against the long-double replay and the bounds of
tests/test_lbfgs_cpu.py, the ring over 2 M + 3 launches, the rules, the launcher's rejections, the engine.

Measured on an MI355X, error / bound of p and of beta' per raw-step case (each against its own bound, 64 x the float64
vector-space loop's error on that quantity, floored at 2^-53); columns M, messages, message type:
         1,1,f32     1,1,f64     1,9,f32     1,9,f64     3,1,f32     3,1,f64     3,9,f32     3,9,f64     7,1,f32     7,1,f64     7,9,f32     7,9,f64
D=1    0.009/0.000 0.007/0.007 0.002/0.007 0.014/0.002 0.001/0.001 0.016/0.010 0.019/0.008 0.064/0.013 0.043/0.000 0.035/0.009 0.009/0.002 0.035/0.018
D=3    0.010/0.003 0.020/0.007 0.003/0.003 0.016/0.005 0.051/0.006 0.060/0.009 0.018/0.004 0.016/0.005 0.018/0.012 0.009/0.003 0.034/0.023 0.016/0.016
D=4    0.026/0.003 0.013/0.004 0.021/0.007 0.006/0.006 0.030/0.006 0.004/0.003 0.040/0.020 0.014/0.006 0.017/0.012 0.016/0.004 0.007/0.012 0.010/0.004
D=5    0.017/0.010 0.020/0.008 0.015/0.004 0.032/0.005 0.017/0.014 0.025/0.003 0.021/0.008 0.008/0.014 0.005/0.008 0.024/0.006 0.005/0.008 0.008/0.011
D=63   0.023/0.007 0.020/0.012 0.014/0.007 0.016/0.010 0.009/0.012 0.005/0.008 0.018/0.007 0.009/0.008 0.019/0.009 0.008/0.007 0.007/0.008 0.007/0.010
D=257  0.014/0.010 0.013/0.010 0.012/0.012 0.017/0.011 0.011/0.009 0.011/0.010 0.010/0.008 0.018/0.009 0.021/0.008 0.016/0.008 0.010/0.008 0.007/0.008
D=1000 0.010/0.009 0.014/0.009 0.038/0.010 0.035/0.009 0.003/0.010 0.006/0.010 0.011/0.008 0.006/0.009 0.009/0.009 0.007/0.009 0.009/0.009 0.007/0.010"""  # noqa: E501
import numpy as np
import pytest
import torch

from erasurehead_amd.engine import Trainer
from erasurehead_amd.ops.update import lbfgs_pairs, lbfgs_state, lbfgs_update
from erasurehead_amd.parallel.dist import DistEnv
from test_lbfgs_cpu import BOUND_FACTOR, DS, FLOOR, LD, MS, case, check_step, rel, replay_step
from test_multimodel_cpu import CASES, arrival_sets, make

pytestmark = pytest.mark.gpu
DEV = "cuda"


def on_gpu(msgs, coefs, beta, state, ring, co, **kw):
    t = [x.to(DEV) for x in (beta, state, ring)]
    hist = torch.full((beta.numel(),), float("nan"), dtype=torch.float64, device=DEV)
    bw = torch.full((beta.numel(),), float("nan"), dtype=torch.float32, device=DEV)
    lbfgs_update([m.to(DEV) for m in msgs], coefs, *t, **co, hist=hist, beta_w=bw, **kw)
    torch.cuda.synchronize()
    return [x.cpu() for x in (*t, hist, bw)]


@pytest.mark.parametrize("mdt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nmsg", [1, 9])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", DS)
def test_raw_step_against_long_double(D, M, nmsg, mdt, native):
    def run(msgs, coefs, beta, state, ring, co):
        b, st, rg, hist, bw = on_gpu(msgs, coefs, beta, state, ring, co)
        assert torch.equal(hist[:D], b[:D]) and torch.equal(bw[:D], b[:D].float()) and torch.all(bw[D:] == 0) and \
            torch.all(b[D:] == 0) and torch.all(st[:, D:] == 0)  # padding: exact zeros
        return b.numpy(), st.numpy(), rg

    check_step(run, D, M, nmsg, mdt)


@pytest.mark.parametrize("M", MS)
def test_ring_fills_evicts_and_wraps(M, native):
    """2 M + 3 launches on one state over a quadratic (g = A beta - c, one fp64 message): after every launch the
    pairs in logical order, head, count, beta_prev and G_prev against the replay, which is fed the device's beta."""
    D, ld = 63, 64
    rng = np.random.RandomState(M)
    A, c = np.pad(rng.uniform(1.0, 100.0, D), (0, 1)), np.pad(rng.randn(D), (0, 1))
    beta = torch.from_numpy(np.pad(rng.randn(D), (0, 1))).to(DEV)
    state, ring = lbfgs_state(M, ld, DEV)
    st, rg = state.cpu().numpy().astype(LD), ring.tolist()
    co = dict(d=D, eta=1.0 / 128, gs=1.0, l2c=0.0, tau=1.0)
    for i in range(2 * M + 3):
        b = beta.cpu().numpy()
        g = A * b - c
        nb64 = replay_step(np.float64, [g], [1.0], b, st, rg, **co)[0]
        nb, _, st, rg = replay_step(LD, [g], [1.0], b, st, rg, **co)
        lbfgs_update([torch.from_numpy(g).to(DEV)], [1.0], beta, state, ring, **co)
        assert ring.tolist() == rg == [max(0, i - M) % M, min(i, M), 1, int(i == 0)], f"launch {i}"
        S, Y = (x.cpu().numpy() for x in lbfgs_pairs(state, ring))
        rows = [(rg[0] + j) % M for j in range(rg[1])]
        for got, want in ((S, st[rows]), (Y, st[[M + r for r in rows]]), (state[2 * M:2 * M + 2].cpu().numpy(), st[2 * M:2 * M + 2])):
            assert np.all(np.abs(got - want) <= 2.0 ** -52 * np.abs(want)), f"launch {i}"  # one rounding each
        assert rel(beta.cpu().numpy()[:D], nb) <= BOUND_FACTOR * max(rel(nb64, nb), FLOOR), f"launch {i}"


def test_rejected_candidate_leaves_the_ring_bitwise(native):
    def run(msgs, coefs, beta, state, ring, co):
        b, st, rg, _, _ = on_gpu(msgs, coefs, beta, state, ring, co)
        assert torch.equal(st[:6], state[:6])
        return b.numpy(), st.numpy(), rg

    check_step(run, 257, 3, 9, want_ring=[1, 3, 1, 0], candidate=-1.0)


@pytest.mark.parametrize("why", ["newest s.y < 0", "NaN in a message"])
def test_no_descent_takes_the_gd_step_and_empties_the_ring(why, native):
    msgs, coefs, beta, state, ring, co = case(257, 3, 9, candidate=-1.0, newest=-1.0 if why[0] == "n" else 1.0)
    if why[0] == "N":
        msgs[4][17] = float("nan")
    g = sum(c * m.numpy() for c, m in zip(coefs, msgs))
    want = beta.numpy() - co["eta"] * (co["gs"] * g + co["l2c"] * beta.numpy())
    b, st, rg, _, _ = on_gpu(msgs, coefs, beta, state, ring, co)
    assert rg.tolist() == [0, 0, 1, 2]
    np.testing.assert_allclose(b.numpy()[:257], want[:257], rtol=1e-14, atol=1e-15, equal_nan=True)
    assert np.isnan(b.numpy()).sum() == (why[0] == "N")


def test_closed_gate_writes_nothing(native):
    msgs, coefs, beta, state, ring, co = case(63, 3, 1)
    out = on_gpu(msgs, coefs, beta, state, ring, co, gate=torch.ones(1, dtype=torch.int32, device=DEV))
    assert torch.equal(out[0], beta) and torch.equal(out[1], state) and torch.equal(out[2], ring)
    assert torch.isnan(out[3]).all() and torch.isnan(out[4]).all()


@pytest.mark.parametrize("kw", [dict(memory=0), dict(memory=8), dict(memory=-1), dict(tau=0.0), dict(tau=-1.0),
                                dict(tau=float("nan")), dict(tau=float("inf"))], ids=str)
def test_launcher_rejects_invalid_arguments(kw, native):
    msgs, coefs, beta, state, ring, co = case(5, 3, 1)
    t = [x.to(DEV) for x in (beta, state, ring)]
    a = dict(dict(memory=3, tau=1.0), **kw)
    with pytest.raises(RuntimeError, match="invalid"):
        native.lbfgs_update([msgs[0].to(DEV)], [1.0], t[0], None, None, t[1], t[2], a["memory"], 5, 0.1, 1.0, 0.0,
                            a["tau"], None)
    torch.cuda.synchronize()
    assert torch.equal(t[0].cpu(), beta) and torch.equal(t[1].cpu(), state) and torch.equal(t[2].cpu(), ring)


@pytest.mark.parametrize("name", ["naive", "frc"])
def test_gpu_engine_follows_the_cpu_engine(name, native):
    """Stream = graph = a second stream run, bitwise; within a raw step's bound of beta' per round of the CPU run."""
    runs = {}
    for loop in ("stream", "graph", "stream"):
        cfg, src, sch, _ = make(CASES[name], lbfgs=3, lr=2.0)
        cfg.device_loop = loop
        tg = Trainer(cfg, DistEnv(device=torch.device(DEV)), src, scheme=sch)
        res = tg.run()
        assert tg.rank_report()["round_loop"] == loop and tg.rank_report()["lbfgs"] == 3
        assert int(tg.lbfgs_state[1][1]) == 3
        if loop in runs:
            np.testing.assert_array_equal(res.betaset, runs[loop].betaset)
        runs[loop] = res
    np.testing.assert_array_equal(runs["stream"].betaset, runs["graph"].betaset)
    cfg, src, sch, _ = make(CASES[name], lbfgs=3, lr=2.0)
    rc = Trainer(cfg, DistEnv(), src, scheme=sch).run()
    assert arrival_sets(runs["stream"]) == arrival_sets(rc)
    per_round = 2 * check_step(None, 33, 3, 1)[1]  # both engines may miss the exact beta' by a raw step's bound at d = 33
    for i, (got, want) in enumerate(zip(runs["stream"].betaset, rc.betaset)):
        print(f"lbfgs engine {name} round {i}: {rel(got, want.astype(LD)):.3e} bound {(i + 1) * per_round:.3e}")
        assert rel(got, want.astype(LD)) <= (i + 1) * per_round, f"round {i}"
