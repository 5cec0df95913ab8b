"""The loader/consumer row path's run-ahead schedule (csrc/glm.hip, DEPTH = LOADER): the loader
wave prefetches S − 2 ring steps, stays out of the deferred round completion (the 8 consumer waves
run it), meets them at one raw barrier and reads the stop decision from LDS (S = gk.LOADER_SLOTS;
the batch sizes follow it). The places where that schedule can go wrong:
blocks with fewer steps than the prefill, exactly as many, and just past one and two ring turns,
each with a ragged last step; per-row fills; a stop that finds the ring full; the same rounds
replayed from a captured graph; blocks that own no row at all. References: exact integer row
census, the fp64 host trainer."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 5003
LOADER = -1
BLOCKS = 3
STEP_ROWS = 8 * BLOCKS  # rows of one ring step of every block together


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_DATA = {}
_REF = {}


def _data(d, pitch=0):
    """(X bf16 [N, d] on the host, the same on the device with row pitch d + pitch, y, integer
    weights), built once."""
    key = (d, pitch)
    if key not in _DATA:
        g = torch.Generator(device="cpu").manual_seed(2000 + d)
        Xh = torch.rand((N, d), generator=g).to(torch.bfloat16)
        y = torch.randint(0, 2, (N,), generator=g).to(torch.float64)
        wt = (torch.arange(N) % 7 + 1).to(torch.float64)
        Xd = torch.zeros((N, d + pitch), dtype=torch.bfloat16, device="cuda")[:, :d]
        Xd.copy_(Xh)
        _DATA[key] = (Xh, Xd, y, wt)
    return _DATA[key]


def _ref(d, B, max_iter):
    """The fp64 host trainer's coefficients for (d, B, max_iter), computed once and shared."""
    from flink_ml_amd.common.optimizer import SGD, TorchGlmTrainer

    key = (d, B, max_iter)
    if key not in _REF:
        Xh, _, y, wt = _data(d)
        sgd = SGD(max_iter=max_iter, learning_rate=0.1, global_batch_size=B, tol=0.0)
        _REF[key] = TorchGlmTrainer(sgd, np.zeros(d), Xh.to(torch.float64), y, wt, "logistic").fit()
    return _REF[key]


def _trainer(gk, sgd, d, Xd, y, wt, blocks, use_graph=False):
    """A DeviceGlmTrainer on exactly ``blocks`` blocks (the trainer caps the grid by the batch
    size; the kernel must also cope with blocks that own no row)."""
    from flink_ml_amd.common.optimizer import DeviceGlmTrainer

    tr = DeviceGlmTrainer(sgd, np.zeros(d), Xd, y.cuda(), wt.cuda(), "logistic", use_graph=use_graph)
    if tr.nparts != blocks:
        tr.nparts = blocks
        tr.scratch = gk.RoundScratch(blocks, d, torch.float32, Xd.device, det=tr.scratch.det)
    return tr


class _Loader:
    """nt = 1 makes small data eligible, set_dma(-1) selects the path; both restored on exit."""

    def __init__(self, gk):
        self.gk = gk

    def __enter__(self):
        self.gk.RoundScratch(1, 8, torch.float32, "cuda")  # applies the process default first
        self.gk.set_tuning(-1, 1)
        self.gk.set_dma(LOADER)
        return self

    def __exit__(self, *exc):
        self.gk.set_tuning(-1, -1)
        self.gk.set_dma(self.gk.DMA_DEPTH)


def _deferred(gk, monkeypatch, blocks):
    monkeypatch.setattr(gk, "DEFER", True)
    monkeypatch.setattr(gk, "DETERMINISTIC", False)
    monkeypatch.setattr(gk, "GRAD_BLOCKS", blocks)


def _census(gk, d, blocks, batches, pitch=0):
    """Integer row weights make Σweight (feedback[d]) an exact, order-independent census of each
    round's batch: 6 completed rounds per batch size, so both launch parities; round 0 runs on
    w = 0, where every row's loss is log 2."""
    from flink_ml_amd.common.optimizer import SGD

    _, Xd, y, wt = _data(d, pitch)
    assert Xd.stride(0) == d + pitch
    with _Loader(gk):
        for B in batches:
            sgd = SGD(max_iter=8, learning_rate=0.1, global_batch_size=B, tol=0.0)
            tr = _trainer(gk, sgd, d, Xd, y, wt, blocks)
            assert tr.defer and tr.scratch.nparts == blocks
            P = -(-N // B)
            tr._launch_round(1)
            assert gk.row_path() == LOADER
            for e in range(6):  # launch e + 1 completes round e and publishes its feedback
                tr._launch_round(1)
                torch.cuda.synchronize()
                b0 = (e % P) * B
                want = float(wt[b0:min(b0 + B, N)].sum())
                got = float(tr.feedback[d].item())
                assert got == want, (B, e, got, want)
                if e == 0:
                    assert abs(float(tr.feedback[d + 1].item()) - want * math.log(2.0)) <= 1e-5 * want


def _step_counts(gk):
    S = gk.LOADER_SLOTS
    return [S - 3, S - 2, S - 1, S, S + 1, 2 * S + 1]


@pytest.mark.parametrize("d", [520, 1000])
def test_prefetch_census_around_the_ring_depth(d, monkeypatch):
    """3 blocks, 24 rows per step: a batch of 24·n rows gives every block exactly n steps, one row
    more gives block 0 a ragged step n + 1 of one row. n = S − 3 (fewer steps than the prefill),
    S − 2 (the prefill is everything), S − 1, S, S + 1 (one ring turn) and 2S + 1 (two)."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    _deferred(gk, monkeypatch, BLOCKS)
    _census(gk, d, BLOCKS, [STEP_ROWS * n + r for n in _step_counts(gk) for r in (0, 1)])


def test_prefetch_census_padded_pitch(monkeypatch):
    """ld = d + 24: no contiguous 8-row group, every slot is filled row by row; the prefill alone
    and two ring turns, each with the ragged extra step."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    _deferred(gk, monkeypatch, BLOCKS)
    S = gk.LOADER_SLOTS
    _census(gk, 1000, BLOCKS, [STEP_ROWS * n + r for n in (S - 2, 2 * S + 1) for r in (0, 1)], pitch=24)


def test_prefetch_census_blocks_without_rows(monkeypatch):
    """224 blocks, 61 rows: 8 blocks own rows (one step, the last ragged), 216 prefetch nothing and
    still meet the prologue's barrier."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    _deferred(gk, monkeypatch, 224)
    _census(gk, 1000, 224, [61])


@pytest.mark.parametrize("d", [520, 1000])
def test_stop_with_a_full_ring(d, monkeypatch):
    """max_iter = 3 on 74 steps per block: the fourth launch (the flush) has its whole prefill in
    flight when its consumers decide to stop; the loader must drain and leave. Later launches are
    no-ops: three rounds executed, coefficients untouched and equal to the fp64 host trainer's."""
    _need_gpu()
    from flink_ml_amd.common.optimizer import SGD
    from flink_ml_amd.ops import glm as gk

    _deferred(gk, monkeypatch, BLOCKS)
    B = 1777
    _, Xd, y, wt = _data(d)
    sgd = SGD(max_iter=3, learning_rate=0.1, global_batch_size=B, tol=0.0)
    with _Loader(gk):
        tr = _trainer(gk, sgd, d, Xd, y, wt, BLOCKS)
        assert tr.defer
        got = tr.fit()
        assert gk.row_path() == LOADER
        tr.flush()
        for _ in range(3):
            tr._launch_round(1)
        torch.cuda.synchronize()
        assert tr.rounds_executed() == 3
        after = tr.coef[:d].to(torch.float64).cpu().numpy()
    assert np.array_equal(got, after)
    ref = _ref(d, B, 3)
    assert np.allclose(got, ref, rtol=2e-4, atol=2e-6), np.abs(got - ref).max()


@pytest.mark.parametrize("d", [520, 1000])
def test_graph_replay_matches_direct_launches(d, monkeypatch):
    """9 rounds as three replays of a captured 3-round graph (the form the benchmark times: launch
    e + 1's prologue right behind launch e's tail) and as direct launches, both against the fp64
    host trainer."""
    _need_gpu()
    from flink_ml_amd.common.optimizer import SGD
    from flink_ml_amd.ops import glm as gk

    _deferred(gk, monkeypatch, BLOCKS)
    B = 1777
    _, Xd, y, wt = _data(d)
    ref = _ref(d, B, 9)
    out = {}
    with _Loader(gk):
        for graph in (True, False):
            sgd = SGD(max_iter=9, learning_rate=0.1, global_batch_size=B, tol=0.0)
            tr = _trainer(gk, sgd, d, Xd, y, wt, BLOCKS, use_graph=graph)
            tr.rounds_per_graph = 3
            assert tr.defer and tr.use_graph == graph
            out[graph] = tr.fit()
            assert gk.row_path() == LOADER
            assert tr.rounds_executed() == 9
            assert bool(tr.graphs) == graph
    for graph in (True, False):
        assert np.allclose(out[graph], ref, rtol=2e-4, atol=2e-6), (graph, np.abs(out[graph] - ref).max())
