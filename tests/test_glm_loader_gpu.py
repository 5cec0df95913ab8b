"""The fused round's loader/consumer row path (csrc/glm.hip, DEPTH = LOADER): bf16 rows of d
513–1024 streamed by a ninth wave per block through a ring of 16-KiB LDS slots. Small shapes at
which the path can go wrong: the narrowest two-chunk row (d 520 = 65 chunks), a ragged and a full
second piece (1000, 1024); 3 blocks (the ring wraps many times), 8, and 224 (most blocks own no
row and still join the prologue and the tail); batches of fewer rows than one slot, a partial last
slot, batch starts that are no multiple of 8 rows, a short last batch and the whole set; a padded
row pitch (per-row fills instead of contiguous groups); no row weights. References: exact integer
row census, the fp64 host trainer, and bit identity with the register loop under the fixed-order
tail."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 5003
LOADER = -1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_DATA = {}


def _data(d, pitch=0):
    """(X bf16 [N, d] on the device with row pitch d + pitch, y, integer weights), built once."""
    key = (d, pitch)
    if key not in _DATA:
        g = torch.Generator(device="cpu").manual_seed(1000 + d)
        Xh = torch.rand((N, d), generator=g).to(torch.bfloat16)
        y = torch.randint(0, 2, (N,), generator=g).to(torch.float64)
        wt = (torch.arange(N) % 7 + 1).to(torch.float64)
        Xd = torch.zeros((N, d + pitch), dtype=torch.bfloat16, device="cuda")[:, :d]
        Xd.copy_(Xh)
        _DATA[key] = (Xh, Xd, y, wt)
    return _DATA[key]


def _trainer(gk, sgd, d, Xd, y, wt, loss, blocks):
    """A DeviceGlmTrainer on exactly ``blocks`` blocks (the trainer caps the grid by the batch
    size; the kernel must also cope with blocks that own no row)."""
    from flink_ml_amd.common.optimizer import DeviceGlmTrainer

    tr = DeviceGlmTrainer(sgd, np.zeros(d), Xd, y.cuda(), None if wt is None else wt.cuda(), loss, use_graph=False)
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


def _census(gk, monkeypatch, d, blocks, pitch=0, weights=True):
    from flink_ml_amd.common.optimizer import SGD

    monkeypatch.setattr(gk, "DEFER", True)
    monkeypatch.setattr(gk, "DETERMINISTIC", False)
    monkeypatch.setattr(gk, "GRAD_BLOCKS", blocks)
    _, Xd, y, wt = _data(d, pitch)
    assert Xd.stride(0) == d + pitch
    wts = wt if weights else torch.ones(N, dtype=torch.float64)
    with _Loader(gk):
        for B in (1, 61, 1777, N):
            sgd = SGD(max_iter=8, learning_rate=0.1, global_batch_size=B, tol=0.0)
            tr = _trainer(gk, sgd, d, Xd, y, wt if weights else None, "logistic", blocks)
            assert tr.defer and tr.scratch.nparts == blocks
            P = -(-N // B)
            tr._launch_round(1)  # round 0 (w = 0: every row's loss is log 2)
            assert gk.row_path() == LOADER
            for e in range(6):  # launch e + 1 completes round e and publishes its feedback
                tr._launch_round(1)
                torch.cuda.synchronize()
                b0 = (e % P) * B
                want = float(wts[b0:min(b0 + B, N)].sum())
                got = float(tr.feedback[d].item())
                assert got == want, (B, e, got, want)
                if e == 0:
                    assert abs(float(tr.feedback[d + 1].item()) - want * math.log(2.0)) <= 1e-5 * want


@pytest.mark.parametrize("d", [520, 1000, 1024])
@pytest.mark.parametrize("blocks", [3, 8, 224])
def test_loader_round_covers_every_row_once(d, blocks, monkeypatch):
    """Integer row weights make Σweight (feedback[d]) an exact, order-independent census of each
    round's batch: 6 completed rounds per batch size (both launch parities), and round 0's Σloss
    is Σw · log 2."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    _census(gk, monkeypatch, d, blocks)


def test_loader_round_census_padded_pitch(monkeypatch):
    """ld = d + 24: no contiguous 8-row group, every slot is filled row by row."""
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    _census(gk, monkeypatch, 1000, 8, pitch=24)


def test_loader_round_census_no_weights(monkeypatch):
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    _census(gk, monkeypatch, 1000, 3, weights=False)


@pytest.mark.parametrize("loss", ["logistic", "hinge", "leastsquare"])
@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("d,blocks,B,pitch", [(1000, 8, 1777, 0), (520, 224, N, 0), (1024, 3, 61, 0), (1000, 3, 1777, 24)])
def test_loader_fit_matches_fp64(loss, defer, d, blocks, B, pitch, monkeypatch):
    """A 3-round fit against the fp64 host trainer at the tolerance the register loop's tests use,
    through the deferred and the ticketed tail."""
    _need_gpu()
    from flink_ml_amd.common.optimizer import SGD, TorchGlmTrainer
    from flink_ml_amd.ops import glm as gk

    monkeypatch.setattr(gk, "DEFER", defer)
    monkeypatch.setattr(gk, "DETERMINISTIC", False)
    monkeypatch.setattr(gk, "GRAD_BLOCKS", blocks)
    Xh, Xd, y, wt = _data(d, pitch)
    sgd = SGD(max_iter=3, learning_rate=0.1, global_batch_size=B, tol=1e-9)
    ref = TorchGlmTrainer(sgd, np.zeros(d), Xh.to(torch.float64), y, wt, loss).fit()
    with _Loader(gk):
        tr = _trainer(gk, sgd, d, Xd, y, wt, loss, blocks)
        assert tr.defer == defer
        got = tr.fit()
        assert gk.row_path() == LOADER
    assert tr.rounds_executed() == 3
    assert np.allclose(got, ref, rtol=2e-4, atol=2e-6), np.abs(got - ref).max()


@pytest.mark.parametrize("d,blocks,B,weights", [
    pytest.param(1000, 8, 1777, True, id="1000-8-1777"), pytest.param(520, 224, N, True, id="520-224-%d" % N),
    pytest.param(1024, 3, 1777, True, id="1024-3-1777"), pytest.param(1000, 3, 61, False, id="1000-3-61-noweights")])
def test_loader_deterministic_tail_bit_identical_to_register_loop(d, blocks, B, weights, monkeypatch):
    """Fixed-order tail: the loader path twice and the register loop give bit-identical
    coefficients — same per-row math, same rows in the same order per wave, same tail. The last
    case has no row weights, a ragged second piece, a ring that wraps many times and batches
    smaller than one slot."""
    _need_gpu()
    from flink_ml_amd.common.optimizer import SGD
    from flink_ml_amd.ops import glm as gk

    monkeypatch.setattr(gk, "DETERMINISTIC", True)
    monkeypatch.setattr(gk, "GRAD_BLOCKS", blocks)
    monkeypatch.setattr(gk, "GRAD_UNROLL", 0)
    _, Xd, y, wt = _data(d)
    out = []
    with _Loader(gk):
        for dma in (LOADER, LOADER, 0):
            gk.set_dma(dma)
            sgd = SGD(max_iter=5, learning_rate=0.1, global_batch_size=B, tol=0.0)
            tr = _trainer(gk, sgd, d, Xd, y, wt if weights else None, "logistic", blocks)
            assert tr.scratch.det and not tr.defer
            out.append(tr.fit())
            assert gk.row_path() == dma
    assert np.array_equal(out[0], out[1])
    assert np.array_equal(out[0], out[2]), np.abs(out[0] - out[2]).max()


def test_loader_selector_values():
    _need_gpu()
    from flink_ml_amd.ops import glm as gk

    gk.RoundScratch(1, 8, torch.float32, "cuda")  # applies the process default first
    try:
        for bad in (5, 1, 3):
            with pytest.raises(ValueError):
                gk.set_dma(bad)
        for ok in (0, LOADER):
            gk.set_dma(ok)
    finally:
        gk.set_dma(gk.DMA_DEPTH)
