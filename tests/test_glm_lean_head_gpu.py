"""The lean launch head of the loader/consumer row path (csrc/glm.hip, glm_round_kernel HEAD > 0)
against the generic head, in one build (gk.set_head).

With blocks <= acc_reps every accumulator address receives exactly one add per round, so a deferred
fit does not depend on the order of the atomics: both heads must then agree BITWISE on the
coefficients, on the feedback after every launch and on all eight state words. Every case runs 7
launches on N = 5003 rows with integer weights, logistic loss and non-zero reg / elastic_net, so
every e % 3 accumulator slot and both round-word parities are seen twice. One case per replica
count the head is instantiated for, the per-row fill form, a block without rows, a wrapping batch
with a short last one, both stop rules, graph replay, and one parity check against the fp64 host
trainer (its reference knows no regularisation, so that case runs without)."""
import numpy as np
import pytest
import torch

from tests.test_glm_loader_prefetch_gpu import LOADER, N, _data, _deferred, _Loader, _need_gpu, _ref, _trainer

pytestmark = pytest.mark.gpu

LAUNCHES = 7


def _launches(gk, head, d, blocks, reps, B, pitch=0, max_iter=100, tol=0.0, use_graph=False):
    """[(coef, feedback, state)] on the host after each of LAUNCHES launches with the given head."""
    from flink_ml_amd.common.optimizer import SGD

    _, Xd, y, wt = _data(d, pitch)
    assert Xd.stride(0) == d + pitch
    out = []
    gk.set_tail_tuning(reps)
    gk.set_head(head)
    try:
        sgd = SGD(max_iter=max_iter, learning_rate=0.1, global_batch_size=B, tol=tol, reg=0.01, elastic_net=0.5)
        tr = _trainer(gk, sgd, d, Xd, y, wt, blocks, use_graph=use_graph)
        tr.rounds_per_graph = 1
        assert tr.defer and tr.scratch.nparts == blocks and tr.use_graph == use_graph
        for _ in range(LAUNCHES):
            tr.run_rounds(1)
            torch.cuda.synchronize()
            assert gk.row_path() == LOADER
            # the head that ran: the lean one is instantiated per replica count
            assert gk.last_head() == (reps if head else 0)
            out.append((tr.coef[:d].cpu().numpy().copy(), tr.feedback.cpu().numpy().copy(),
                        tr.state.cpu().numpy().copy()))
        assert bool(tr.graphs) == use_graph
    finally:
        gk.set_head(gk.HEAD)
        gk.set_tail_tuning()
    return out


def _same(gk, monkeypatch, d, blocks, reps, B, **kw):
    """Runs both heads; asserts bitwise agreement after every launch. Returns the lean head's record."""
    _deferred(gk, monkeypatch, blocks)
    with _Loader(gk):
        lean = _launches(gk, 1, d, blocks, reps, B, **kw)
        generic = _launches(gk, 0, d, blocks, reps, B, **kw)
    for i, (a, b) in enumerate(zip(lean, generic)):
        for name, x, y in zip(("coef", "feedback", "state"), a, b):
            # (bit patterns: NaN-safe and sign-of-zero-exact)
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), (i, name, x, y)
    return lean


@pytest.mark.parametrize("reps", [1, 2, 4, 8])
def test_each_replica_count(reps, monkeypatch):
    """acc_reps = blocks: one case per R the lean head is instantiated for."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    rec = _same(gk, monkeypatch, 1000, reps, reps, 1777)
    assert int(rec[-1][2][4]) == LAUNCHES - 1  # ST_EXECUTED: launch e + 1 completes round e
    assert np.abs(rec[-1][0]).max() > 0


@pytest.mark.parametrize("d", [520, 1024])
def test_per_row_fill(d, monkeypatch):
    """Row pitch d + 8: no contiguous 8-row group, every slot is filled row by row."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    _same(gk, monkeypatch, d, 3, 8, 1777, pitch=8)


def test_block_without_rows(monkeypatch):
    """8 blocks of 8 rows per step on a batch of 50 rows: block 6 owns two rows, block 7 none."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    _same(gk, monkeypatch, 1000, 8, 8, 50)


def test_wrapping_batch(monkeypatch):
    """B = 1500: four batches, the last of 503 rows; launch 4 starts the second pass."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    assert N % 1500 != 0
    rec = _same(gk, monkeypatch, 1000, 4, 4, 1500)
    w = (np.arange(N) % 7 + 1).astype(np.float64)
    # feedback[d] after launch e + 1 is Σweight of batch e % 4: an exact integer census
    for e in range(LAUNCHES - 1):
        b0 = (e % 4) * 1500
        assert float(rec[e + 1][1][1000]) == float(w[b0:min(b0 + 1500, N)].sum()), e


def test_stop_on_max_iter(monkeypatch):
    """max_iter = 3: launch 3 completes round 2 and raises ST_DONE, launches 4–6 return on it."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    rec = _same(gk, monkeypatch, 1000, 4, 4, 1777, max_iter=3)
    assert [int(r[2][4]) for r in rec] == [0, 1, 2, 3, 3, 3, 3]  # ST_EXECUTED
    assert int(rec[-1][2][6]) == 1  # ST_DONE
    for r in rec[4:]:
        assert np.array_equal(r[0], rec[3][0])


def test_stop_on_tol(monkeypatch):
    """tol = 10 (the first round's loss per weight is log 2): round 1's test ends the fit."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    rec = _same(gk, monkeypatch, 1000, 4, 4, 1777, tol=10.0)
    assert [int(r[2][4]) for r in rec] == [0, 1, 1, 1, 1, 1, 1]
    assert int(rec[-1][2][6]) == 1


def test_graph_replay(monkeypatch):
    """The same 7 rounds replayed from captured one-round graphs (one per round-word parity)."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    rec = _same(gk, monkeypatch, 1000, 4, 4, 1777, use_graph=True)
    assert int(rec[-1][2][4]) == LAUNCHES - 1


def test_lean_head_matches_host_trainer(monkeypatch):
    """The lean head's fit (3 blocks, 4 replicas: the atomics' order is free here) against the
    fp64 host trainer, at tests/test_glm_loader_prefetch_gpu.py's tolerance for this shape."""
    _need_gpu()
    from flink_ml_amd.common.optimizer import SGD
    from flink_ml_amd.ops import glm as gk

    d, B = 1000, 1777
    _deferred(gk, monkeypatch, 3)
    _, Xd, y, wt = _data(d)
    ref = _ref(d, B, 9)
    with _Loader(gk):
        gk.set_head(1)
        sgd = SGD(max_iter=9, learning_rate=0.1, global_batch_size=B, tol=0.0)
        tr = _trainer(gk, sgd, d, Xd, y, wt, 3)
        got = tr.fit()
        assert gk.row_path() == LOADER and gk.last_head() == 4
        assert tr.rounds_executed() == 9
    assert np.allclose(got, ref, rtol=2e-4, atol=2e-6), np.abs(got - ref).max()
