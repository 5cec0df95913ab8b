"""Mini-batch SGD as an SPMD round loop (reference ``LIB/common/optimizer/SGD.java:67-390``).

Semantics reproduced exactly:
* local batch = globalBatchSize / P, remainder to the low ranks (``SGD.java:206-213``);
* round e trains on rows ``[off_e, min(off_e + B, n))`` of the rank's cached partition with
  ``off`` advancing by B and resetting to 0 once it passes the end (``SGD.java:263-268``);
* feedback = all-reduced [Σ mult·x | Σ weight | Σ loss] (``SGD.java:252,271-283``);
* termination: after round e the iteration continues iff ``e+1 < maxIter`` and
  ``Σloss/Σweight > tol`` (``TerminateOnMaxIterOrTol.java:62-68``); the final feedback is
  applied once more when the iteration terminates (``SGD.java:288-294``) — so every computed
  feedback is applied exactly once;
* update: ``w -= lr/Σw · Σg`` then elastic-net regularisation, skipped when Σw = 0.

MI355X execution (see ``ops/csrc/glm.hip``): the data partition stays resident in HBM and a
dense round is ONE kernel launch — loss+gradient over the batch, fixed-order in-kernel
reduction, then (1 GPU) the update, or (N GPUs) the feedback exchange with every peer over
xGMI (``parallel/xgmi.py``) followed by the same update on every rank. Without the xGMI
exchange the kernel ends with the feedback, RCCL all-reduces it and an update kernel follows.
All control state is on the device; rounds are captured once into a hipGraph and replayed; the
host only polls the device "running" flag every ``check_every`` rounds for early termination.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch

from ..ops import glm as gk
from ..parallel import comm
from ..parallel.checkpoint import AlgorithmCheckpoint, fault_point
from ..parallel.context import device_sharers, get_context
from ..table import SparseColumn
from ..utils import graphs, hostsync, tracing

# bucket-round fits shorter than this launch their rounds directly instead of capturing hipGraphs
BKT_GRAPH_MIN_ITERS = 200


def _dzeros(shape, dtype, dev) -> torch.Tensor:
    """Zero-filled device buffers of the trainers through the library's own fill kernel (torch's
    fill kernels load lazily: tens of ms inside the first fit of a process)."""
    if dev.type == "cuda":
        from ..ops import native

        return native.zeros(shape, dtype, dev)
    return torch.zeros(shape, dtype=dtype, device=dev)


def local_batch_size(global_batch: int, rank: int, world: int) -> int:
    b = global_batch // world
    if global_batch % world > rank:
        b += 1
    return b


class SGD:
    def __init__(self, max_iter: int = 20, learning_rate: float = 0.1, global_batch_size: int = 32,
                 tol: float = 1e-6, reg: float = 0.0, elastic_net: float = 0.0):
        self.max_iter = int(max_iter)
        self.learning_rate = float(learning_rate)
        self.global_batch_size = int(global_batch_size)
        self.tol = float(tol)
        self.reg = float(reg)
        self.elastic_net = float(elastic_net)

    def optimize(self, init_coef: Optional[np.ndarray], X, y: torch.Tensor, weight: Optional[torch.Tensor],
                 loss: str) -> np.ndarray:
        """``init_coef`` None: the reference's zero initial model (no host array of the model's
        width is made or scanned: a fresh 8 MB one costs ~0.5 ms of page faults per fit)."""
        trainer = make_trainer(self, init_coef, X, y, weight, loss)
        try:
            return trainer.fit()
        finally:
            if hasattr(trainer, "close"):
                trainer.close()


def make_trainer(sgd: SGD, init_coef, X, y, weight, loss, use_graph: Optional[bool] = None):
    dev = X.device if isinstance(X, (torch.Tensor, SparseColumn)) else torch.device("cpu")
    if dev.type == "cuda":
        return DeviceGlmTrainer(sgd, init_coef, X, y, weight, loss, use_graph=use_graph)
    if isinstance(X, (torch.Tensor, SparseColumn)) and isinstance(y, torch.Tensor) and y.device.type == "cuda":
        # a GPU fit whose dense or CSR partition stays in host memory (it exceeds the HBM budget):
        # the out-of-core trainer keeps what fits resident and streams the rest (common/outofcore.py)
        from .outofcore import StreamedGlmTrainer, hbm_budget

        return StreamedGlmTrainer(sgd, init_coef, X, y, weight, loss, y.device, hbm_budget(y.device))
    return TorchGlmTrainer(sgd, init_coef, X, y, weight, loss)


class TorchGlmTrainer:
    """Host reference implementation (fp64), used on CPU-only hosts and by the test-suite."""

    def __init__(self, sgd: SGD, init_coef, X, y, weight, loss: str):
        ctx = get_context()
        self.sgd = sgd
        self.loss = gk.LOSS_CODES[loss]
        self.sparse = isinstance(X, SparseColumn)
        if self.sparse:
            self.X = X
            self.n = len(X)
            self.d = X.size
        else:
            self.X = X.to(torch.float64)
            self.n, self.d = (int(X.shape[0]), int(X.shape[1]))
        self.y = y.to(torch.float64).reshape(-1)
        self.w = weight.to(torch.float64).reshape(-1) if weight is not None else torch.ones(self.n, dtype=torch.float64)
        self.coef = (torch.zeros(self.d, dtype=torch.float64) if init_coef is None
                     else torch.as_tensor(np.asarray(init_coef, dtype=np.float64)).clone())
        self.B = local_batch_size(sgd.global_batch_size, ctx.rank, ctx.world_size)
        self.offset = 0
        self.rounds = 0

    def _batch(self):
        s = self.offset
        e = min(s + self.B, self.n)
        self.offset += self.B
        if self.offset >= self.n:
            self.offset = 0
        return s, e

    def _feedback(self) -> torch.Tensor:
        fb = torch.zeros(self.d + 2, dtype=torch.float64)
        if self.n > 0:
            s, e = self._batch()
            if self.sparse:
                sub = self.X
                ip = sub.indptr[s:e + 1]
                idx = sub.indices[ip[0]:ip[-1]].long()
                val = sub.values[ip[0]:ip[-1]].to(torch.float64)
                rows = torch.repeat_interleave(torch.arange(e - s), ip[1:] - ip[:-1])
                dot = torch.zeros(e - s, dtype=torch.float64).index_add_(0, rows, val * self.coef[idx])
                l, m = gk.torch_loss_and_mult(self.loss, dot, self.y[s:e], self.w[s:e])
                fb[: self.d].index_add_(0, idx, m[rows] * val)
            else:
                xb = self.X[s:e]
                dot = xb @ self.coef
                l, m = gk.torch_loss_and_mult(self.loss, dot, self.y[s:e], self.w[s:e])
                fb[: self.d] = m @ xb
            fb[self.d] = self.w[s:e].sum()
            fb[self.d + 1] = l.sum()
        return comm.all_reduce_sum(fb)

    def _apply(self, fb: torch.Tensor) -> None:
        W = float(fb[self.d])
        if W > 0:
            self.coef -= self.sgd.learning_rate / W * fb[: self.d]
            gk.torch_regularize(self.coef, self.sgd.reg, self.sgd.elastic_net, self.sgd.learning_rate)

    def fit(self) -> np.ndarray:
        ck = AlgorithmCheckpoint("sgd")
        start = 0
        restored = ck.restore()
        if restored is not None:
            start, st = restored
            self.coef = st["coef"].to(torch.float64).clone()
            self.offset, self.rounds = int(st["offset"]), int(st["rounds"])
            if st["done"]:
                return self.coef.numpy().copy()
        for e in range(start, self.sgd.max_iter):
            fault_point(e)
            fb = self._feedback()
            self.rounds += 1
            self._apply(fb)
            W, L = float(fb[self.d]), float(fb[self.d + 1])
            crit = L / W if W != 0 else float("nan")
            tracing.log_round(kind="sgd", path="host", rank=get_context().rank, epoch=e, loss=L, weight=W,
                              bytes=int(fb.numel() * fb.element_size()))
            cont = e + 1 < self.sgd.max_iter and crit > self.sgd.tol
            ck.maybe_save(e + 1, lambda: {"coef": self.coef, "offset": self.offset, "rounds": self.rounds,
                                          "done": not cont})
            if not cont:
                break
        return self.coef.numpy().copy()


class DeviceGlmTrainer:
    """HBM-resident SGD on MI355X via the fused HIP kernels (one process per GPU)."""

    def __init__(self, sgd: SGD, init_coef, X, y, weight, loss: str, use_graph: Optional[bool] = None,
                 check_every: int = 8, pad: bool = True, bucket_nnz=None):
        ctx = get_context()
        self.ctx = ctx
        self.sgd = sgd
        self.loss = gk.LOSS_CODES[loss]
        self.sparse = isinstance(X, SparseColumn)
        dev = X.device
        self.device = dev
        if self.sparse:
            self.n, self.d = len(X), X.size
            acc = torch.float64 if X.values.dtype == torch.float64 else torch.float32
            self.indptr = X.indptr.to(device=dev, dtype=torch.int64).contiguous()
            self.indices = X.indices.to(device=dev, dtype=torch.int32).contiguous()
            self.values = X.values.to(device=dev, dtype=acc).contiguous()
        else:
            if X.dtype not in (torch.float32, torch.float64, torch.bfloat16):
                X = X.to(torch.float32)
            X = X.contiguous() if X.stride(-1) != 1 else X
            self.layout = gk.pick_layout(X)
            d_model = int(X.shape[1])
            if self.layout is None and pad and dev.type == "cuda":
                # misaligned width: a zero-padded copy keeps the fused kernel (padding columns'
                # coefficients stay 0; outputs are cut back to the model's width)
                Xp = gk.pad_columns(X)
                if Xp is not None:
                    X, self.layout = Xp, gk.pick_layout(Xp)
            self.X = X
            self.n, self.d = int(X.shape[0]), int(X.shape[1])
            acc = torch.float64 if X.dtype == torch.float64 else torch.float32
        self.d_model = d_model if not self.sparse else self.d
        self.acc = acc
        self.y = y.to(device=dev, dtype=acc).reshape(-1).contiguous()
        self.w = weight.to(device=dev, dtype=acc).reshape(-1).contiguous() if weight is not None else None
        self.B = local_batch_size(sgd.global_batch_size, ctx.rank, ctx.world_size)
        if self.sparse and dev.type == "cuda" and bucket_nnz is None:
            gk.prefetch_batch_bounds(self.indptr, self.n, self.B)  # (collected by the round set-up below)
        # the usual zero init (1M-wide sparse models): no pageable H2D copy. None (the library's
        # estimators) makes no host array at all; a given one is tested on the bit patterns (an
        # integer max: 0.17 ms on 1M doubles, against 1.2 ms for any() and 2.5 for count_nonzero —
        # host time a short fit's GPU idles through); −0.0 just takes the copy
        c0 = None
        if init_coef is not None:
            c0 = np.ascontiguousarray(init_coef, dtype=np.float64).reshape(-1)
            if c0.shape[0] < self.d:
                c0 = np.concatenate([c0, np.zeros(self.d - c0.shape[0])])
        zero_init = c0 is None or not c0.size or int(c0.view(np.uint64).max()) == 0
        self.bkt = self.csc = None
        self._zb = self._alloc_sparse_round(sgd, zero_init, bucket_nnz) if self.sparse else None
        if self._zb is not None:
            self.coef, self.state, self.feedback = self._zb[:3]
        else:
            if zero_init:
                self.coef = _dzeros((self.d,), acc, dev)
            else:
                c0 = torch.from_numpy(np.ascontiguousarray(c0)).to(acc)
                self.coef = (c0.pin_memory() if dev.type == "cuda" else c0).to(dev, non_blocking=True).contiguous()
            self.state = _dzeros(8, torch.int32, dev)
            self.feedback = _dzeros(self.d + 2, acc, dev)
        # running[0] (a fill kernel: `t[i] = scalar` is a blocking pageable copy)
        if dev.type == "cuda":
            from ..ops import native

            native.fill_i32(self.state[1:2], 1)
        else:
            self.state[1:2].fill_(1)
        self.distributed = ctx.is_distributed
        self.xg = None
        # dense rows one wave's registers cannot hold: the wide-row kernel (a block's 8 waves split
        # each row's columns, one read of the batch, fused atomic tail); beyond its width (or in
        # the deterministic mode) two bandwidth-bound GEMVs per round (X_b·w, then X_bᵀ·m,
        # rocBLAS) + the device update kernel
        self.wide_layout = None
        if not self.sparse and self.layout is None and dev.type == "cuda" and not gk.DETERMINISTIC and gk.WIDE_FUSED:
            self.wide_layout = gk.pick_wide_layout(self.X)
        self.wide_fused = self.wide_layout is not None
        self.wide = not self.sparse and self.layout is None and not self.wide_fused
        self._host_round = 0
        if self.sparse:
            self.scratch = None
            self.nparts = 0
        elif self.wide:
            self.scratch = None
            self.nparts = 0
            if self.w is None:
                self.w = torch.ones(self.n, dtype=acc, device=dev)
        elif self.wide_fused:
            # one or two 8-wave blocks per CU (by the slice's register need), each walking its rows
            cus = torch.cuda.get_device_properties(dev).multi_processor_count * gk.wide_blocks_per_cu(self.X)
            share = device_sharers(ctx) if self.distributed else 1
            self.nparts = max(1, min(cus // max(1, share), -(-max(self.B, 1) // 2)))
            self.scratch = gk.RoundScratch(self.nparts, self.d, acc, dev, det=False)
        else:
            self.nparts = max(1, min(gk.round_blocks(self.X), gk.max_round_blocks(), math.ceil(max(self.B, 1) / (gk.WPB * 16))))
            if self.distributed:
                from ..parallel import xgmi

                self.xg = xgmi.get()
                if self.xg is not None and self.d + 2 > self.xg.glm_max:
                    self.xg = None
                share = device_sharers(ctx)
                if self.xg is not None and share >= 2:
                    # ranks rehearsing on ONE GPU: the in-kernel exchange (and, deferred, every
                    # block spinning on its lead) waits for the peers' kernels, so every rank's
                    # grid must be resident at once. The round kernel's LDS pad lets at most
                    # ceil(blocks / CUs) of its blocks share a CU, so `share` grids of at most
                    # CUs / share blocks always fit (4 ranks of 85 blocks timed out; 2 ranks of
                    # the 512-block grid fill every slot before the second lead starts — ADVICE
                    # r4). A GPU per rank (measured by PCI id) never hits this cap.
                    cus = torch.cuda.get_device_properties(dev).multi_processor_count
                    self.nparts = max(1, min(self.nparts, cus // share))
            self.scratch = gk.RoundScratch(self.nparts, self.d, acc, dev)
        if self.wide_fused:
            self.mode = gk.TAIL_FEEDBACK if self.distributed else gk.TAIL_UPDATE
        elif self.sparse or self.wide or self.distributed and self.xg is None:
            self.mode = gk.TAIL_FEEDBACK  # feedback → RCCL all-reduce → update kernel
        else:
            self.mode = gk.TAIL_XGMI if self.distributed else gk.TAIL_UPDATE
        if use_graph is None:
            use_graph = os.environ.get("FMLX_HIPGRAPH", "1") == "1"
        if self.wide:
            use_graph = False  # the batch slice is chosen on the host each round
        if self.distributed and self.mode == gk.TAIL_FEEDBACK and ctx.backend != "nccl":
            use_graph = False  # a gloo all-reduce of device tensors cannot be captured
        self.use_graph = use_graph
        # 1 GPU, fused dense round with the atomic tail: launch e completes round e − 1 in its
        # prologue (no ticket / serial tail); launches alternate between two round-number words
        # (``parity``), so hipGraphs are keyed by (rounds, starting parity)
        # N GPUs over the in-kernel xGMI exchange: launch e + 1's lead block exchanges and applies
        # round e (csrc/glm.hip defer_prologue_xgmi); FMLX_GLM_DEFER_XGMI=0 keeps the ticketed tail
        self.defer = ((self.mode == gk.TAIL_UPDATE or self.mode == gk.TAIL_XGMI and gk.DEFER_XGMI)
                      and self.scratch is not None and not self.scratch.det and not self.wide_fused
                      and gk.defer_supported(self.d, acc))
        self.parity = 0
        self.cw = _dzeros((2, self.d), acc, dev) if self.defer else None
        self._flushed = False
        self._short = False  # fit(): too few rounds for hipGraph capture to pay (direct launches)
        self.bkt_graph_min_iters = BKT_GRAPH_MIN_ITERS
        self.graphs = {}
        self.timing = False
        self.check_every = max(1, int(check_every))
        self.rounds_per_graph = self.check_every
        self._launched = 0  # rounds launched so far (round e visits batch e mod P)

    def use_rccl(self) -> None:
        """Switches the dense rounds from the in-kernel xGMI exchange to feedback → RCCL
        all-reduce → update kernel (e.g. after a bounded xGMI wait gave up). The deferred
        completion only exists on the fused tails, so it is recomputed with the mode, together
        with everything captured for the old mode."""
        if self.defer and self._launched:
            raise RuntimeError("use_rccl() after deferred rounds ran: their last update is pending")
        self.xg = None
        if not self.sparse and not self.wide and self.distributed:
            self.mode = gk.TAIL_FEEDBACK  # (the wide-row kernel already runs its feedback tail)
        self.defer, self.cw, self.parity = False, None, 0
        if self.ctx.backend != "nccl":
            self.use_graph = False  # a gloo all-reduce of device tensors cannot be captured
        self.graphs.clear()

    def _alloc_sparse_round(self, sgd: SGD, zero_init: bool, bucket_nnz):
        """Chooses the sparse round form once and allocates for it: the single-visit bucket round
        (``self.bkt``, ``self.wl``), the transposed round (``self.csc``, ``self.mult``, ``self.wl``)
        or neither (the scattered-atomic kernel). Returns the bucket round's block of zeroed
        buffers when it made one — coefficients, round state, feedback, Σw/Σloss slots, the rounds'
        slice counters and accumulator as ONE allocation and ONE fill launch (a short fit's GPU
        idles through every Python-side launch) — else None."""
        dev, acc = self.device, self.acc
        live = dev.type == "cuda" and self.n > 0
        zb = None
        if bucket_nnz is not None or (live and self._bucket_pays(sgd)):
            if zero_init and live:
                from ..ops import native

                zb = native.zeros_many([((self.d,), acc), ((8,), torch.int32), ((self.d + 2,), acc),
                                        ((gk.wl_elems(),), acc), ((gk.BucketRound.nb_for(self.d) + 16,), torch.int32),
                                        ((self.d,), acc)], dev)
            if bucket_nnz is not None:
                # (the out-of-core trainer: one batch at a time, every round on the bucket path;
                # bucket_nnz = (largest batch's entries, mean row length))
                size = dict(most=bucket_nnz[0], avg=bucket_nnz[1])
            else:
                # each batch visited a few times (the reference's regime): the single-visit round,
                # nothing built per batch but the column-slice counts of the visited batches
                size = dict(batches=min(-(-self.n // max(self.B, 1)), sgd.max_iter))
            self.bkt = gk.BucketRound.alloc(self.indptr, self.values, max(1, self.n), self.d, self.B,
                                            zero_bufs=None if zb is None else (zb[4], zb[5]), **size)
            if self.bkt is not None:
                self.wl = zb[3] if zb is not None else _dzeros(gk.wl_elems(), acc, dev)
            elif bucket_nnz is not None:
                raise ValueError("streamed sparse batches need the bucket round (too many column slices)")
        if self.bkt is None and live:
            # allocated here, batches transposed lazily before the rounds that visit them
            self.csc = gk.BatchCsc.alloc(self.indptr, self.indices, self.values, self.n, self.d, self.B,
                                         max_rounds=sgd.max_iter)
            if self.csc is not None:
                self.mult = _dzeros(max(1, min(self.B, self.n)), acc, dev)
                self.wl = _dzeros(gk.wl_elems(), acc, dev)  # Σw/Σloss slots per parity
        return zb

    def _reduce_and_update(self) -> None:
        """The feedback tail of a round: all-reduce of the feedback row across the ranks, then the
        device update kernel (SGD step, regularisation, termination check)."""
        s = self.sgd
        if self.distributed:
            comm.all_reduce_sum(self.feedback)
        gk.update(self.feedback, self.d, self.coef, self.state, s.max_iter, s.tol, s.learning_rate, s.reg,
                  s.elastic_net)

    def _bucket_pays(self, sgd: SGD) -> bool:
        """The single-visit bucket round (no per-batch transpose) for fits that visit each batch
        fewer than ``gk.TILE_MIN_VISITS`` times; more visits amortise the transposed layout's
        build (its steady rounds are faster). Not in the deterministic mode (LDS float atomics)."""
        if gk.DETERMINISTIC or not gk.BUCKETS:
            return False
        P = -(-self.n // max(self.B, 1))
        return sgd.max_iter < gk.TILE_MIN_VISITS * max(P, 1)

    # -- one round as a fixed launch sequence (capturable) -------------------------------------
    def _launch_round(self, rounds: int = 1, ensure: bool = True) -> None:
        """Launches ``rounds`` consecutive rounds (one host call on the fused dense path,
        else ``rounds`` launch sequences). ``ensure=False``: the caller already ensured the
        column-major batches (the capture warm-up, whose ``_launched`` is already advanced past
        the rounds it replays — ensuring there could regrow the storage mid-replay)."""
        if rounds > 1 and not (self.csc is None and not self.wide and not self.wide_fused and not self.sparse
                               and self.mode != gk.TAIL_FEEDBACK):
            for _ in range(rounds):
                self._launch_round(1, ensure)
            return
        s = self.sgd
        if self.bkt is not None:
            if self.bkt.slots and self.bkt.slots < -(-self.n // self.B) and s.max_iter > self.bkt.slots:
                raise RuntimeError("bucket round counted %d batches, max_iter grew to %d" % (self.bkt.slots, s.max_iter))
            if not torch.cuda.is_current_stream_capturing():
                self.bkt.count_all(self.indptr, self.indices, self.n, self.B)  # (once per trainer)
            gk.bkt_round(self.bkt, self.indptr, self.indices, self.values, self.y, self.w, self.coef, self.n, self.d,
                         self.B, self.loss, self.state, self.wl, self.feedback, not self.distributed, s.max_iter, s.tol,
                         s.learning_rate, s.reg, s.elastic_net)
            if self.distributed:
                self._reduce_and_update()
            return
        if self.csc is not None:
            if ensure and not torch.cuda.is_current_stream_capturing():
                self._ensure_csc(self._launched, 1)
            # forward (per-row multipliers) + atomic-free column-major backward; on 1 GPU the
            # backward applies the update and the termination check itself
            gk.csc_round(self.csc, self.indptr, self.indices, self.values, self.y, self.w, self.coef, self.n, self.d,
                         self.B, self.loss, self.state, self.mult, self.wl, self.feedback, not self.distributed,
                         s.max_iter, s.tol, s.learning_rate, s.reg, s.elastic_net)
            if self.distributed:
                self._reduce_and_update()
            return
        if self.wide_fused:
            gk.glm_round_wide(self.X, self.y, self.w, self.coef, self.B, self.loss, self.state, self.scratch, self.mode,
                              self.feedback, s.max_iter, s.tol, s.learning_rate, s.reg, s.elastic_net)
            if self.mode == gk.TAIL_FEEDBACK:
                self._reduce_and_update()
            return
        if self.wide:
            # the device state advances once per launch whether or not the round runs, so the
            # host round counter selects the same batch as the device epoch
            e = self._host_round
            self._host_round += 1
            if self.n > 0:
                P = -(-self.n // self.B)
                b0 = (e % P) * self.B
                b1 = min(b0 + self.B, self.n)
                xb = self.X[b0:b1]
                if xb.dtype != self.acc:
                    xb = xb.to(self.acc)
                dot = torch.mv(xb, self.coef)
                l, m = gk.torch_loss_and_mult(self.loss, dot, self.y[b0:b1], self.w[b0:b1])
                torch.mv(xb.t(), m, out=self.feedback[: self.d])
                self.feedback[self.d] = self.w[b0:b1].sum()
                self.feedback[self.d + 1] = l.sum()
            else:
                self.feedback.zero_()
            self._reduce_and_update()
            return
        if self.sparse:
            self.feedback.zero_()
            if self.n > 0:
                gk.grad_csr(self.indptr, self.indices, self.values, self.y, self.w, self.coef, self.n, self.d, self.B,
                            self.loss, self.state, self.feedback)
            self._reduce_and_update()
            return
        # every rank launches the round, also one without rows: it still joins the reduction tail
        gk.glm_round(self.X, self.y, self.w, self.coef, self.B, self.loss, self.state, self.scratch, self.mode,
                     self.feedback, s.max_iter, s.tol, s.learning_rate, s.reg, s.elastic_net, xg=self.xg, rounds=rounds,
                     defer=self.defer, parity=self.parity, cw=self.cw)
        if self.defer:
            self.parity = (self.parity + rounds) & 1
        if self.mode == gk.TAIL_FEEDBACK:
            self._reduce_and_update()

    def _ensure_csc(self, first: int, k: int) -> None:
        """Column-major copies of the batches rounds first … first + k − 1 visit; rounds at or
        past max_iter never run (the device running flag predicates them off before any load).
        A storage re-allocation moves the device pointers the captured hipGraphs hold."""
        k = min(k, self.sgd.max_iter - first)
        if k <= 0:
            return
        v = self.csc.version
        self.csc.ensure_rounds(first, k)
        if self.csc.version != v:
            self.graphs.clear()

    def _graph_key(self, rounds: int, parity=None):
        if not self.defer:
            return rounds
        return (rounds, self.parity if parity is None else parity)

    def _capture(self, key):
        """Captures ``rounds`` consecutive SGD rounds into one hipGraph (state lives on device, so
        the same launch sequence repeats); replaying it costs one host submission per ``rounds``.
        Deferred mode: ``key`` = (rounds, starting parity)."""
        rounds, parity = key if self.defer else (key, None)
        side = graphs.aux_stream(self.device, "sgd-warmup")
        side.wait_stream(torch.cuda.current_stream(self.device))
        # everything a round mutates that the next round reads (the sparse path's Σw/Σloss
        # parity slots, the deferred mode's accumulator ring and coefficient ring included) is
        # rewound after the warm-up
        live = [self.state, self.coef] + ([self.wl] if self.csc is not None or self.bkt is not None else [])
        if self.defer:
            live += [self.scratch.acc, self.cw, self.scratch.cnt]  # cnt: the dynamic schedule's counters
        snapshot = [t.clone() for t in live]
        saved_parity = self.parity
        with torch.cuda.stream(side):
            self._launch_round(ensure=False)  # warm-up outside capture (allocator / RCCL lazy init)
        torch.cuda.current_stream(self.device).wait_stream(side)
        for t, v in zip(live, snapshot):
            t.copy_(v)
        if self.defer:
            self.parity = parity
        g = graphs.capture(lambda: self._launch_round(rounds), self.device)
        self.parity = saved_parity
        self.graphs[key] = g
        return g

    def _replay(self, rounds: int) -> None:
        key = self._graph_key(rounds)
        g = self.graphs.get(key) or self._capture(key)
        g.replay()
        if self.defer:
            self.parity = (self.parity + rounds) & 1

    def graph_sizes(self, k: int):
        """Round counts of the hipGraphs ``run_rounds(k)`` replays (R-round graphs, then the
        1-round graph for the remainder)."""
        if not self.use_graph or k <= 0:
            return []
        full, rem = divmod(k, self.rounds_per_graph)
        return ([self.rounds_per_graph] if full else []) + ([1] if rem else [])

    def graph_keys(self, k: int):
        """Keys of every hipGraph ``run_rounds(k)`` may replay, whatever the starting parity."""
        sizes = self.graph_sizes(k)
        return [(r, p) for r in sizes for p in (0, 1)] if self.defer else sizes

    def priming_rounds(self, k: int) -> int:
        """Upper bound of the rounds ``prime(k)`` runs."""
        keys = self.graph_keys(k)
        return sum(kk[0] + 1 for kk in keys) if self.defer else sum(keys)

    def precapture(self, k: int) -> None:
        """Captures (and instantiates) every hipGraph that ``run_rounds(k)`` will replay, so a
        timed ``run_rounds(k)`` afterwards only replays (capture costs ~1 ms per graph)."""
        for key in self.graph_keys(k):
            if key not in self.graphs:
                self._capture(key)

    def prime(self, k: int) -> int:
        """Replays every graph of ``graph_keys(k)`` once (first-replay upload costs), each at its
        own starting parity (a direct 1-round launch switches parity). Returns rounds run."""
        done = 0
        for key in self.graph_keys(k):
            if self.defer and key[1] != self.parity:
                self._launch_round(1)
                self._launched += 1
                done += 1
            r = key[0] if self.defer else key
            if self.csc is not None:
                self._ensure_csc(self._launched, r)
            g = self.graphs.get(key) or self._capture(key)
            g.replay()
            self._launched += r
            if self.defer:
                self.parity = (self.parity + r) & 1
            done += r
        return done

    def run_rounds(self, k: int) -> None:
        """Runs ``k`` SGD rounds (each predicated on the device running flag), no host sync."""
        if self.csc is not None:
            self._ensure_csc(self._launched, k)  # the batches these rounds visit
        first = self._launched
        self._launched += k
        if not self.use_graph or self._short:
            R = self.rounds_per_graph
            for i in range(0, k, R):
                self._launched = first + i
                self._launch_round(min(R, k - i))
            self._launched = first + k
            return
        R = self.rounds_per_graph
        full, rem = divmod(k, R)
        for _ in range(full):
            self._replay(R)
        for _ in range(rem):
            self._replay(1)

    def flush(self) -> None:
        """Deferred mode: the last round's update is applied by the NEXT launch; one more launch
        (a no-op round once the iteration stopped) completes it."""
        if self.defer and not self._flushed:
            self._launch_round(1)
            self._flushed = True

    def step(self) -> None:
        """Runs one SGD round (predicated on the device running flag)."""
        self.run_rounds(1)

    def running(self) -> bool:
        st = hostsync.to_host(self.state)  # polled, no blocking runtime wait
        if self.defer:
            return not bool(st[6])
        e = int(st[0])
        return bool(st[1 + (e & 1)])

    def _poll_stopped(self) -> bool:
        """Non-blocking termination check: the device state copied to pinned memory at the previous
        check is read if that copy has landed, and a new copy is queued. A stop is seen one check
        interval late at worst — the rounds launched meanwhile are predicated off on the device —
        and the host never waits for the GPU mid-fit (a blocking check drained the launch queue).

        Distributed: every rank must break after the SAME number of launched rounds (a host-issued
        all-reduce per round, or a captured one, has to find its peers), so the lag is fixed at
        exactly one interval — the copy queued at the previous check is waited for (it is one
        interval behind the launch front, so the wait rarely blocks) — instead of depending on
        each rank's own timing."""
        stopped = False
        ev = getattr(self, "_state_ev", None)
        if ev is not None and self.distributed:
            hostsync.wait_event(ev)
        if ev is not None and ev.query():
            st = self._state_host
            stopped = bool(st[6]) if self.defer else not bool(st[1 + (int(st[0]) & 1)])
        if ev is None:
            self._state_host = torch.empty(self.state.shape, dtype=self.state.dtype, pin_memory=True)
            self._state_ev = ev = torch.cuda.Event()
        if ev.query():
            self._state_host.copy_(self.state, non_blocking=True)
            ev.record()
        return stopped

    def rounds_executed(self) -> int:
        return int(self.state[4].item())

    def check_exchange(self) -> None:
        """Raises if a bounded xGMI wait gave up (a peer never arrived): the rounds since then
        used a partial feedback and must not be reported."""
        comm.check_collectives()

    def fit(self) -> np.ndarray:
        ck = AlgorithmCheckpoint("sgd")
        done = 0
        restored = ck.restore()
        if self.defer and (ck.mgr is not None or tracing.rounds_enabled()):
            # checkpoints and per-round logs read the round's own coefficients / feedback
            self.defer, self.cw = False, None
            self.graphs.clear()
        if restored is not None:
            done, st = restored
            self.coef.copy_(st["coef"].to(self.coef.dtype))
            self.state.copy_(st["state"])
            self._host_round = int(self.state[0].item())
            self._launched = self._host_round
            if st["done"]:
                return self.coef[:self.d_model].to(torch.float64).cpu().numpy()
        # a fit shorter than two graphs' worth of rounds launches directly: capture + first replay
        # (~1 ms per graph) would cost more than the launches it saves
        if not self.graphs and self.sgd.max_iter < 2 * self.rounds_per_graph:
            self._short = True
        if self.bkt is not None and not self.graphs and self.sgd.max_iter < self.bkt_graph_min_iters:
            # the bucket round's three launches take less host time than their GPU time
            # (~0.1 ms at 100k rows); the process's first capture + instantiate costs ~18 ms
            # (SVC 20-round first fit 22.2 ms with graphs, profiles/r6/INDEX.md)
            self._short = True
        if self.csc is not None:
            # every batch this fit visits in one go: one sort per run of up to CSC_RUN_MAX batches
            # instead of one per check interval
            self._ensure_csc(self._launched, self.sgd.max_iter - done)
        log = tracing.rounds_enabled()
        # per-round logs (a diagnostic mode) read every round's own feedback: one round per host
        # step; otherwise check-interval (or checkpoint-interval) rounds per host step
        step = 1 if log else (ck.interval if ck.interval else self.check_every)
        with tracing.range("sgd.fit"):
            while done < self.sgd.max_iter:
                fault_point(done)
                k = min(step, self.sgd.max_iter - done)
                if log:
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                with tracing.range("sgd.rounds[%d]" % k):
                    self.run_rounds(k)
                done += k
                if log:
                    # the device keeps the last round's global feedback [Σg | Σw | Σloss]
                    ev1.record()
                    fb = self.feedback[self.d:self.d + 2].double().cpu()
                    tracing.log_round(kind="sgd", path="device", rank=self.ctx.rank, epoch=self.rounds_executed() - 1,
                                      rounds=k, loss=float(fb[1]), weight=float(fb[0]),
                                      kernel_ms=round(ev0.elapsed_time(ev1), 4),
                                      bytes_per_round=int(self.B * (self.d * self.X.element_size() if not self.sparse
                                                                    and not self.wide else 0)))
                if done >= self.sgd.max_iter:
                    stop = False
                elif ck.mgr is not None or log:
                    stop = not self.running()  # checkpoints / round logs read this round's state
                else:
                    stop = self._poll_stopped()  # never drains the queue (see _poll_stopped)
                ck.maybe_save(done, lambda: {"coef": self.coef, "state": self.state,
                                             "done": stop or done >= self.sgd.max_iter})
                if stop:
                    break
            self.flush()
        # the coefficients: one stream-ordered copy into pinned memory, completion polled — a host
        # sync point, after which the exchange's error word is final
        # (widened on the device: a host-side conversion first-touches a fresh 8 MB array, ~2 ms of
        # page faults in the first fit of a process; the pinned copy is already faulted in)
        coef = hostsync.to_host(self.coef[:self.d_model].to(torch.float64)).numpy()
        self.check_exchange()
        return coef
