"""Knn / KnnModel (reference ``LIB/classification/knn/{Knn,KnnModel,KnnModelData}.java``).

fit packs every training point into one model (features as a column-major dim×n DenseMatrix,
squared norms, labels — ``Knn.java:98-135``); the ranks all-gather their partitions in rank order.

predict is the K3/K13 hot path: for a block of queries, one GEMM gives Q·Tᵀ (hipBLASLt on the GPU,
fp32 by default / fp64 on CPU), ``dist = sqrt(|‖q‖² + ‖t‖² − 2 q·t|)`` exactly as
``KnnModel.predictLabel``, then the k nearest (stable: among equal distances the earlier training
point wins, like the reference's strict-``>`` priority-queue replacement) and a majority vote.
On the GPU (fp32, D ≤ 128, k ≤ 64) distances and top-k are ONE fused HIP kernel (fp32 matrix-core
products, top-k in registers: the nq×n distance block never reaches HBM, ``ops/csrc/knn.hip``);
wider features take the split path (library GEMM block + one top-k scan of it, k ≤ 16).
Vote ties go to the tied label that occurs nearest to the query (resolved on the device, only
for the rows that tie).

A sparse feature column that takes the CSR route (``ops.knn.csr_route``, ``FMLX_KNN_CSR``) is never
densified: fit keeps the CSR arrays (``CsrPackedFeatures``: the model data's ``packedFeatures``,
dense only when ``save()`` asks for the reference bytes), and predict forms each product block from
the CSR query rows and the training set's column-major copy (``ops/csrc/knn_csr.hip``), then runs
the same selection kernels and the same vote.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import config
from ..api.stage import Estimator
from ..common.param import HasFeaturesCol, HasLabelCol, HasPredictionCol
from ..io import read_write as rw
from ..io import serialization as ser
from ..linalg.vectors import DenseMatrix, DenseVector
from ..param.param import IntParam, ParamValidators
from ..parallel import comm
from ..table import SparseColumn, Table
from .base import ModelWithData
from .linear import rw_update
from .stats import features_and_labels


class KnnModelParams(HasFeaturesCol, HasPredictionCol):
    K = IntParam("k", "The number of nearest neighbors", 5, ParamValidators.gt(0))


class KnnParams(KnnModelParams, HasLabelCol):
    pass


def _query_matrix(t: Table, col: str, dev):
    """The query column for the dense routes: a dense [nq, d] tensor, or the SparseColumn itself on
    ``dev`` (``knn_predict`` densifies it a query block at a time, in the compute dtype)."""
    c = t.column(col)
    if isinstance(c, SparseColumn):
        return c.to(device=dev)
    return config.features_for_compute(t, col, allow_sparse=False).to(dev)


def _query_rows(Q, s: int, e: int, dtype) -> torch.Tensor:
    """Rows [s, e) of the query column as a dense block in ``dtype``."""
    if isinstance(Q, SparseColumn):
        return Q.slice(s, e).to_dense(dtype)
    return Q[s:e].to(dtype)


class CsrPackedFeatures(DenseMatrix):
    """``packedFeatures`` of a model fitted on a CSR column: the training set as a ``SparseColumn``
    (``csr``: n rows of size D). As the reference's dim x n column-major matrix it has D rows and n
    columns; ``values`` materialises that array on first access only (``save()`` needs it: the
    reference format is dense)."""

    __slots__ = ("csr", "_host")

    def __init__(self, csr: SparseColumn):
        self.csr = csr
        self.num_rows = csr.size
        self.num_cols = len(csr)
        self._host = None

    @property
    def values(self):
        if self._host is None:
            # column i of the column-major matrix is training point i: the row-major [n, D] array
            self._host = np.ascontiguousarray(self.csr.to_dense(torch.float64).cpu().numpy()).reshape(-1)
        return self._host


class _CsrState:
    """Device state of a CSR-backed model on the CSR route: the training column in kernel form
    (compute dtype), its column-major copy, the norms in the compute dtype, the labels and the
    sorted classes; ``dense``: the dense state, built when a dense query column comes."""

    def __init__(self, X, cm, tnorm, labels):
        self.X, self.cm, self.tnorm, self.labels = X, cm, tnorm, labels
        self.classes = torch.unique(labels)
        self.dense = None


def _csr_block(n: int, es: int) -> int:
    """Queries per block of the routes that sort a whole distance block (host, or k beyond the
    selection kernel's)."""
    return int(max(1, min(4096, (256 << 20) // max(1, (es + 8) * n))))


def knn_topk_csr(Q: SparseColumn, st: _CsrState, k: int):
    """Per query block of the CSR column ``Q`` (on the state's device) the indices [block, k] of the
    k nearest training points, nearest first, ties to the earlier point: a generator."""
    from ..ops import knn as knn_ops
    from ..ops.csr import csr_arrays
    from ..ops.kmeans import check_csr_error

    cm, tn = st.cm, st.tnorm
    n, nq = cm.n, len(Q)
    if Q.size != cm.D:
        raise ValueError("Vector size mismatched.")
    kk = min(k, n)
    if not isinstance(cm, knn_ops.TorchColumnMajor):
        compute, dev = cm.acc, cm.crow.device
        Qk = SparseColumn(*csr_arrays(Q, compute), Q.size)
        qn = knn_ops.csr_sqnorm(Qk, compute, err=cm.err)
        if compute == torch.float32 and kk <= knn_ops.ROUTE_MAX_K and knn_ops.supported(kk, n, dev):
            qb, select = knn_ops.query_block(n), knn_ops.topk_from_products
        elif knn_ops.select_supported(kk, n, compute, dev):
            qb, select = knn_ops.select_query_block(n, tn.element_size()), knn_ops.select_topk
        else:  # k beyond the selection kernel's: a stable sort of the distance block
            qb, select = _csr_block(n, tn.element_size()), None
        G = torch.empty((min(qb, nq), n), dtype=compute, device=dev)
        for s in range(0, nq, qb):
            e = min(nq, s + qb)
            g = knn_ops.csr_products(Qk, cm, s, e, out=G[:e - s])
            if select is not None:
                yield select(g, qn[s:e], tn, kk).long()
            else:
                dist = torch.sqrt(torch.abs(qn[s:e, None] + tn[None, :] - 2.0 * g))
                yield torch.sort(dist, dim=1, stable=True).indices[:, :kk]
        try:
            check_csr_error(cm)  # a query index outside [0, D) was skipped
        finally:
            cm.err.zero_()  # (the word is the model's: the next query column starts clean)
        return
    qb = _csr_block(n, 8)
    for s in range(0, nq, qb):
        q = Q.slice(s, s + qb)
        g = knn_ops.torch_products_csr(q, cm)
        qn = knn_ops.csr_sqnorm(q, torch.float64)
        dist = torch.sqrt(torch.abs(qn[:, None] + tn[None, :] - 2.0 * g))
        yield torch.sort(dist, dim=1, stable=True).indices[:, :kk]


def knn_predict_csr(Q: SparseColumn, st: _CsrState, k: int) -> torch.Tensor:
    """Predicted labels of the CSR query column ``Q`` against a CSR-backed model's state."""
    out = [knn_vote(st.labels[idx], st.classes) for idx in knn_topk_csr(Q, st, k)]
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64, device=st.labels.device)


def knn_vote(top_labels: torch.Tensor, classes: torch.Tensor) -> torch.Tensor:
    """Majority label per row of ``top_labels`` [n, k] (sorted nearest→farthest)."""
    n, k = top_labels.shape
    ci = torch.searchsorted(classes, top_labels)
    counts = torch.zeros((n, classes.numel()), dtype=torch.int32, device=top_labels.device)
    counts.scatter_add_(1, ci, torch.ones_like(ci, dtype=torch.int32))
    best = counts.max(dim=1).values
    pred = classes[counts.argmax(dim=1)]
    ties = torch.nonzero((counts == best[:, None]).sum(1) > 1, as_tuple=True)[0]
    if ties.numel():
        # tied vote: the label met first walking outwards from the query wins (this is what the
        # reference tests pin — KnnTest.testFewerDistinctPointsThanCluster expects the nearest
        # point's label when every label has one vote)
        tl = top_labels[ties]
        tie_mask = counts[ties] == best[ties][:, None]
        ok = torch.gather(tie_mask, 1, torch.searchsorted(classes, tl))
        first = torch.argmax(ok.to(torch.int8), dim=1)
        pred = pred.clone()
        pred[ties] = tl[torch.arange(tl.shape[0], device=tl.device), first]
    return pred


# queries per fused launch: bounds the segment workspace (nq·S·k) and the vote temporaries
FUSED_QUERY_BLOCK = 1 << 18


def knn_predict(Q: torch.Tensor, T: torch.Tensor, tnorm: torch.Tensor, labels: torch.Tensor, k: int,
                block: int = 4096, pack=None, classes=None) -> torch.Tensor:
    """Predicted labels of queries Q [nq, d] (a dense tensor, or a SparseColumn that is densified a
    query block at a time) against training points T [n, d]. ``pack``: a cached
    ``ops.knn.TrainPack`` of T for the fused GPU path (built here when not given); ``classes``:
    the cached sorted distinct labels (a sort of all n labels otherwise)."""
    dev = Q.device
    nq = len(Q)
    if isinstance(Q, SparseColumn) and Q.size != T.shape[1]:
        raise ValueError("Vector size mismatched.")
    compute = torch.float64 if dev.type == "cpu" else config.acc_dtype()
    if classes is None:
        classes = torch.unique(labels)
    kk = min(k, T.shape[0])
    out = []
    if compute == torch.float32:
        from ..ops import knn as knn_ops

        if knn_ops.fused_supported(kk, T.shape[0], T.shape[1], dev):
            if pack is None:
                pack = knn_ops.TrainPack(T, tnorm)
            fb = FUSED_QUERY_BLOCK if not isinstance(Q, SparseColumn) else knn_ops.query_block(T.shape[1])
            for s in range(0, nq, fb):
                idx = knn_ops.fused_topk(_query_rows(Q, s, s + fb, torch.float32), pack, kk)
                out.append(knn_vote(labels[idx.long()], classes))
            return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64, device=dev)
    Tc = T.to(compute)
    tn = tnorm.to(compute)
    if compute == torch.float32:
        from ..ops import knn as knn_ops

        if kk <= knn_ops.ROUTE_MAX_K and knn_ops.supported(kk, T.shape[0], dev):
            tn32 = tn.contiguous()
            qb = knn_ops.query_block(T.shape[0])
            for s in range(0, nq, qb):
                q = _query_rows(Q, s, s + qb, compute)
                G = torch.mm(q, Tc.t())
                idx = knn_ops.topk_from_products(G, (q * q).sum(1), tn32, kk)
                out.append(knn_vote(labels[idx.long()], classes))
            return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64, device=dev)
    if dev.type == "cuda":
        from ..ops import knn as knn_ops

        if knn_ops.select_supported(kk, T.shape[0], compute, dev):
            # k beyond the fused / scan kernels' lists, or fp64 (parity mode): library GEMM per
            # query block + the radix-select kernel (csrc/knn_select.hip)
            tnc = tn.contiguous()
            qb = knn_ops.select_query_block(T.shape[0], Tc.element_size())
            for s in range(0, nq, qb):
                q = _query_rows(Q, s, s + qb, compute)
                idx = knn_ops.select_topk(torch.mm(q, Tc.t()), (q * q).sum(1), tnc, kk)
                out.append(knn_vote(labels[idx.long()], classes))
            return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64, device=dev)
    for s in range(0, nq, block):
        q = _query_rows(Q, s, s + block, compute)
        qn = (q * q).sum(1)
        d2 = torch.addmm(qn[:, None] + tn[None, :], q, Tc.t(), alpha=-2.0)
        dist = torch.sqrt(torch.abs(d2))
        if dev.type == "cpu":
            idx = torch.sort(dist, dim=1, stable=True).indices[:, :kk]
        else:
            idx = torch.topk(dist, kk, dim=1, largest=False, sorted=True).indices
        out.append(knn_vote(labels[idx], classes))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64, device=dev)


@rw.register_stage
class KnnModel(ModelWithData, KnnModelParams):
    JAVA_CLASS_NAME = "org.apache.flink.ml.classification.knn.KnnModel"
    MODEL_DATA_COLUMNS = ("packedFeatures", "featureNormSquares", "labels")

    @staticmethod
    def encode_record(out, row):
        ser.write_dense_matrix(out, row[0])
        ser.write_dense_vector(out, row[1])
        ser.write_dense_vector(out, row[2])

    @staticmethod
    def decode_record(inp):
        return (ser.read_dense_matrix(inp), ser.read_dense_vector(inp), ser.read_dense_vector(inp))

    @classmethod
    def make_model_data_table(cls, rows):
        return Table({"packedFeatures": [r[0] for r in rows], "featureNormSquares": [r[1] for r in rows],
                      "labels": [r[2] for r in rows]}, num_rows=len(rows))

    def _build_state(self, rows):
        dev = config.compute_device()
        m, norms, labels = rows[0]
        if isinstance(m, CsrPackedFeatures):
            st = self._csr_state(m, norms, labels, dev)
            if st is not None:
                return st
        return self._dense_state(rows, dev)

    @staticmethod
    def _csr_state(m, norms, labels, dev):
        """The CSR route's state, or None when the training set keeps the dense route: the route
        does not hold (``ops.knn.csr_route``), or a training row stores an index twice."""
        from ..ops import knn as knn_ops
        from ..ops.csr import ColumnMajor, csr_arrays
        from ..ops.kmeans import check_csr_error

        if not knn_ops.csr_route(m.csr, dev):
            return None
        compute = torch.float64 if dev.type == "cpu" else config.acc_dtype()
        X = m.csr.to(device=dev)
        X = SparseColumn(*csr_arrays(X, compute), X.size)
        if dev.type == "cuda":
            cm = ColumnMajor(X)
            check_csr_error(cm)
        else:
            cm = knn_ops.TorchColumnMajor(X)
        if knn_ops.has_duplicate_index(cm):
            return None
        return _CsrState(X, cm, torch.as_tensor(np.asarray(norms.values), device=dev).to(compute).contiguous(),
                         torch.as_tensor(np.asarray(labels.values), device=dev))

    @staticmethod
    def _dense_state(rows, dev):
        m, norms, labels = rows[0]
        # column i of the dim×n column-major matrix is training point i → row-major [n, dim]
        T = torch.from_numpy(np.asarray(m.values, dtype=np.float64).reshape(m.num_cols, m.num_rows)).to(dev)
        return (T, torch.as_tensor(np.asarray(norms.values), device=dev),
                torch.as_tensor(np.asarray(labels.values), device=dev))

    def _predict_cache(self, T, tnorm, labels):
        """Per model data, built once: the fused kernel's tile-ordered copy of the training points
        (GPU fp32 only) and the sorted distinct labels."""
        from ..ops import knn as knn_ops

        cached = getattr(self, "_pack_cache", None)
        if cached is None or cached[0] is not T:
            pack = None
            if knn_ops.fused_supported(1, T.shape[0], T.shape[1], T.device) and config.acc_dtype() == torch.float32:
                pack = knn_ops.TrainPack(T, tnorm)
            cached = (T, pack, torch.unique(labels))
            self._pack_cache = cached
        return cached[1], cached[2]

    def transform(self, *inputs):
        t = inputs[0]
        st = self._model_state()
        fcol = self.get(self.FEATURES_COL)
        if isinstance(st, _CsrState):
            if t.is_sparse(fcol):
                Q = config.features_for_compute(t, fcol, allow_sparse=True)
                pred = knn_predict_csr(Q, st, self.get(self.K))
                return [t.with_column(self.get(self.PREDICTION_COL), pred.to(torch.float64))]
            if st.dense is None:  # a dense query column: today's route, on the densified training set
                st.dense = self._dense_state(self.model_data_rows(), st.labels.device)
            st = st.dense
        T, tnorm, labels = st
        Q = _query_matrix(t, fcol, T.device)
        pack, classes = self._predict_cache(T, tnorm, labels)
        pred = knn_predict(Q, T, tnorm, labels, self.get(self.K), pack=pack, classes=classes)
        return [t.with_column(self.get(self.PREDICTION_COL), pred.to(torch.float64))]


@rw.register_stage
class Knn(Estimator, KnnParams):
    JAVA_CLASS_NAME = "org.apache.flink.ml.classification.knn.Knn"

    def _fit_csr(self, t: Table):
        """The model of a sparse feature column that takes the CSR route (None otherwise): the CSR
        arrays, labels and norms, all-gathered in rank order."""
        from ..ops import knn as knn_ops
        from ..parallel.context import get_context

        fcol, lcol = self.get(self.FEATURES_COL), self.get(self.LABEL_COL)
        if knn_ops.CSR_ROUTE == "0" or not t.is_sparse(fcol):
            return None
        dev = config.compute_device()
        X = t.column(fcol)
        if isinstance(X, SparseColumn):
            X = X.to(device=dev, dtype=None if X.values.dtype in (torch.float32, torch.float64) else torch.float64)
        else:
            X = config.features_for_compute(t, fcol, allow_sparse=True, exact=True)
        distributed = get_context().is_distributed
        route = knn_ops.csr_route(X, dev)
        if distributed:
            route = comm.all_agree(route)
        if not route:
            return None
        lab = t.column(lcol)
        if isinstance(lab, list) and any(v is None for v in lab):
            raise ValueError("Input data must contain label value.")
        y = t.scalars(lcol, dtype=torch.float64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        norms = knn_ops.csr_sqnorm(X, torch.float64, err=err)
        idx = X.indices
        if dev.type == "cuda":
            bad = bool(err.item())
        else:
            bad = bool(idx.numel()) and (int(idx.min()) < 0 or int(idx.max()) >= X.size)
        if bad:
            raise ValueError("sparse feature index out of range [0, size)")
        lens = (X.indptr[1:] - X.indptr[:-1]).to(torch.int64)
        val = X.values
        if distributed:
            lens, idx, val = comm.all_gather_cat(lens), comm.all_gather_cat(idx), comm.all_gather_cat(val)
            y, norms = comm.all_gather_cat(y), comm.all_gather_cat(norms)
        indptr = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=lens.device)
        indptr[1:] = torch.cumsum(lens, 0)
        md = (CsrPackedFeatures(SparseColumn(indptr, idx, val, X.size)), DenseVector(norms.cpu().numpy()),
              DenseVector(y.cpu().numpy()))
        return KnnModel().set_model_data(KnnModel.make_model_data_table([md]))

    def fit(self, *inputs):
        m = self._fit_csr(inputs[0])
        if m is not None:
            rw_update(m, self)
            return m
        X, y = features_and_labels(inputs[0], self.get(self.FEATURES_COL), self.get(self.LABEL_COL))
        packed = torch.cat([X, y[:, None], (X * X).sum(1)[:, None]], dim=1)
        from ..parallel.context import get_context

        if get_context().is_distributed:
            packed = comm.all_gather_cat(packed)
        packed = packed.cpu().numpy()
        d = packed.shape[1] - 2
        feats, labels, norms = packed[:, :d], packed[:, d], packed[:, d + 1]
        md = (DenseMatrix(d, feats.shape[0], np.ascontiguousarray(feats).reshape(-1)), DenseVector(norms),
              DenseVector(labels))
        m = KnnModel().set_model_data(KnnModel.make_model_data_table([md]))
        rw_update(m, self)
        return m
