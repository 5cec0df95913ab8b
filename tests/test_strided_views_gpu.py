"""Every dense (pointer, ld) kernel entry on views that separate the pointer from the pitch.

``Table.slice`` hands out zero-copy row views, so the dense wrappers under ``flink_ml_amd/ops`` pass a
base pointer plus ``X.stride(0)``. The rest of the suite feeds them fresh contiguous allocations
(``ld == d``, 256-byte-aligned base); here every stride-taking entry point runs on

===========  ===================================================================================
``contig``   ``X.cuda()``: the baseline
``pitch16``  rows inside a wider buffer, ``ld = d + p``, ``p > 0``, ``ld·es % 16 == 0``, base 16-byte
             aligned: ``ld != d`` while still vector-eligible
``pitch1``   ``ld = d + 1``: only element-aligned row starts
``offset1``  ``buf[1 : 1 + n·d].view(n, d)``: ``ld == d``, base one element off a 16-byte boundary
``offset4B`` bf16 only: the same with a lead-in of 2 elements (a 4-byte-aligned base)
``rowslice`` ``Xbig[3:]``, what ``Table.slice`` produces
===========  ===================================================================================

Every cell of the owning buffer outside the view (pitch columns, lead-in, tail) holds NaN, and
``View.check()`` asserts after each call that those cells are bit-for-bit what they were: an
over-read poisons the result, a stray write (the in-place ``axpby`` / ``scal`` / ``csr_axpy_dense``
on a ``Y`` view) is caught directly.

Per entry point and view: (1) the result against an fp64 torch reference of the same operation
under the tolerance the project applies to that kernel on contiguous input (exact equality for the
integer and selection kernels); (2) bitwise equality with the ``contig`` result wherever the
kernel's per-thread order of operations does not depend on the view — everything except the GLM
kernels, where the chunk width picked for the view changes which lane sums which element, and the
KMeans kernels that differ per route (stated at the case).

Launch spy: ``native.call`` is wrapped and every case asserts that the entry point it is about was
launched, so a wrapper that silently routed a view to a torch formulation would fail. A wrapper
that legitimately copies first keeps passing as long as the kernel ran: ``catstats._mat`` and the
BLAS wrappers for ``stride(1) != 1``, ``catstats.int_hist`` (always a contiguous column copy; the
kernel's own ``(ld, col)`` arguments are driven directly here as well), ``bounded_distinct_counts``
for non-fp64 input.

Skips: none. The one documented refusal, ``ops.kmeans.mfma_ok`` for a bf16 view with an odd ``ld``
or a 2-byte-aligned base (``pitch1``, ``offset1``), is asserted as a route instead: those cases
check that ``assign`` took ``fmlx_kmeans_assign_generic`` and still labels correctly.

``test_every_listed_entry_point_has_a_case`` pins the set of entry points the cases of this module
declare (and assert launched) to a fixed list: dropping a case fails it.
"""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
_BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ------------------------------------------------------------------------------------------------
# view builder
# ------------------------------------------------------------------------------------------------
class View:
    """``t``: the [n, d] view; ``buf``: the flat owning buffer (16-byte-aligned first cell);
    ``guard``: the cells of ``buf`` outside the view, with a snapshot of their bits."""

    def __init__(self, name, t, buf, guard):
        self.name, self.t, self.buf, self.guard = name, t, buf, guard
        self.snap = self._bits()[guard].clone()

    def _bits(self):
        return self.buf.view(_BITS[self.buf.element_size()])

    def check(self):
        """The cells outside the view are bit-for-bit what the builder wrote."""
        assert torch.equal(self._bits()[self.guard], self.snap), "write outside the view %r" % self.name


def _poison(dtype):
    return float("nan") if dtype.is_floating_point else torch.iinfo(dtype).min


def place(X, device, lead, ld, tail, name="custom", rowslice=0):
    """``X`` [n, d] copied into a fresh buffer whose first cell is 16-byte aligned: ``lead`` cells,
    then n rows of pitch ``ld``, then ``tail`` cells; everything outside the view poisoned (NaN for
    float dtypes). ``rowslice`` = s builds the view as ``Xbig[s:]`` of an [s + n, d] matrix."""
    n, d = X.shape
    es = X.element_size()
    if rowslice:
        lead, ld = rowslice * d, d
    assert ld >= d and lead >= 0 and tail >= 0
    total = lead + n * ld + tail
    raw = torch.empty(total + 16 // es, dtype=X.dtype, device=device)
    shift = (-raw.data_ptr() % 16) // es
    buf = raw[shift:shift + total]
    assert buf.data_ptr() % 16 == 0
    buf.fill_(_poison(X.dtype))
    if rowslice:
        t = buf[:(rowslice + n) * d].view(rowslice + n, d)[rowslice:]
    else:
        t = buf[lead:lead + n * ld].view(n, ld)[:, :d]
    t.copy_(X)
    guard = torch.ones(total, dtype=torch.bool, device=device)
    guard[lead:lead + n * ld].view(n, ld)[:, :d] = False
    return View(name, t, buf, guard)


def pitch16_ld(d, es):
    """The smallest ld > d whose rows are a whole number of 16-byte chunks."""
    ld = d + 1
    while (ld * es) % 16:
        ld += 1
    return ld


ROWSLICE_START = 3  # odd, as a mini-batch cut of Table.slice


def build_views(X, device="cuda"):
    """name -> View of the CPU matrix ``X`` on ``device``; every view holds the same values."""
    n, d = X.shape
    es = X.element_size()
    out = {
        "contig": place(X, device, 0, d, 0, "contig"),
        "pitch16": place(X, device, 0, pitch16_ld(d, es), 8, "pitch16"),
        "pitch1": place(X, device, 0, d + 1, 8, "pitch1"),
        "offset1": place(X, device, 1, d, 7, "offset1"),
    }
    if X.dtype == BF16:
        out["offset4B"] = place(X, device, 2, d, 6, "offset4B")
    out["rowslice"] = place(X, device, 0, d, 8, "rowslice", rowslice=ROWSLICE_START)
    return out


# ------------------------------------------------------------------------------------------------
# launch spy and the covered-names registry
# ------------------------------------------------------------------------------------------------
ENTRY_POINTS = [
    "fmlx_affine_cols",
    "fmlx_blas_axpby",
    "fmlx_blas_csr_axpy_dense",
    "fmlx_blas_gather_cols",
    "fmlx_blas_gather_prod",
    "fmlx_blas_gemv_t",
    "fmlx_blas_hdot",
    "fmlx_blas_interaction",
    "fmlx_blas_normalize",
    "fmlx_blas_rowreduce",
    "fmlx_colstats",
    "fmlx_cs_col_keys",
    "fmlx_cs_flags",
    "fmlx_cs_hist",
    "fmlx_cs_ihist",
    "fmlx_cs_small_distinct",
    "fmlx_glm_grad_partials",
    "fmlx_glm_predict",
    "fmlx_group_colstats",
    "fmlx_kmeans_assign_bf16",
    "fmlx_kmeans_assign_generic",
    "fmlx_kmeans_chunk_sum",
    "fmlx_kmeans_chunk_sum_bf16v",
    "fmlx_knn_fused",
    "fmlx_knn_select",
    "fmlx_radix_hist",
]
DECLARED = {}  # entry point -> the tests that declare (and assert) it


class Spy:
    def __init__(self):
        self.names = []
        self.asserted = set()

    @contextlib.contextmanager
    def expect(self, *names):
        """The calls inside launch every one of ``names`` through ``native.call``."""
        del self.names[:]
        yield
        for nm in names:
            assert nm in self.names, "%s was not launched (launched: %s)" % (nm, sorted(set(self.names)))
        self.asserted.update(names)


@pytest.fixture
def spy(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flink_ml_amd.ops import native

    s = Spy()
    real = native.call

    def call(name, *args):
        s.names.append(name)
        return real(name, *args)

    monkeypatch.setattr(native, "call", call)
    return s


def covers(*names):
    """Declares the entry points a test is about; after the test body, each of them must have been
    asserted launched through ``spy.expect``."""
    def deco(fn):
        for nm in names:
            DECLARED.setdefault(nm, []).append(fn.__name__)

        @functools.wraps(fn)
        def wrapper(**kw):
            fn(**kw)
            missing = [nm for nm in names if nm not in kw["spy"].asserted]
            assert not missing, "declared but never asserted launched: %s" % missing

        return wrapper

    return deco


def _bitwise(a, b):
    """Same shape, dtype and bits (NaN-safe)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(_BITS[a.element_size()]), b.contiguous().view(_BITS[b.element_size()])
    return torch.equal(a, b)


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _dense(n, d, seed, dtype=F64):  # tests/test_blas.py _dense
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g, dtype=F64).to(dtype)


def _tol(dtype):  # tests/test_blas.py _tol
    return {F64: 1e-12, F32: 1e-5, BF16: 1e-5}[dtype]


# ------------------------------------------------------------------------------------------------
# BLAS (csrc/blas.hip): scalar loads at r·ld + c throughout, any element-aligned view is valid
# ------------------------------------------------------------------------------------------------
BLAS_CASES = [pytest.param(dt, d, id="%s-%d" % (_name(dt), d)) for dt in (F64, F32, BF16) for d in (3, 17, 100)]
BLAS_N = 513


@pytest.mark.parametrize("dtype,d", BLAS_CASES)
@covers("fmlx_blas_rowreduce", "fmlx_blas_gemv_t")
def test_blas_reductions_on_views(dtype, d, spy):
    """row_norm / row_dot / gemv (fmlx_blas_rowreduce, both of its strides: X and Y of different
    pitch) and gemv_t; tolerance of test_blas.py::test_dense_reductions_and_gemv; bitwise equal to
    contig (lanes stride the row by column index, the grid comes from n and d)."""
    from flink_ml_amd.ops import blas

    n = BLAS_N
    X, Y = _dense(n, d, d, dtype), _dense(n, d, d + 1, dtype)
    g = torch.Generator().manual_seed(100 + d)
    v = torch.randn(d, generator=g, dtype=F64)
    m = torch.randn(n, generator=g, dtype=F64)
    Xr, Yr = X.double(), Y.double()
    tol = _tol(dtype) * max(1, d)
    ps = (1.0, 2.0, 3.5, math.inf)
    ref = {("norm", p): torch.linalg.vector_norm(Xr, ord=p, dim=1) for p in ps}
    ref["dot"] = (Xr * Yr).sum(1)
    ref["gemv"] = Xr @ v.to(dtype).double()  # the vector is rounded to the rows' dtype on the device
    ref["gemv_t"] = Xr.t() @ m
    vx, vy = build_views(X), build_views(Y)
    kinds = list(vx)
    base = None
    for i, kind in enumerate(kinds):
        a = vx[kind]
        b = vy["contig" if kind == "contig" else kinds[(i + 1) % len(kinds)]]  # a different pitch for Y
        got = {}
        for p in ps:
            with spy.expect("fmlx_blas_rowreduce"):
                got["norm", p] = blas.row_norm(a.t, p)
        with spy.expect("fmlx_blas_rowreduce"):
            got["dot"] = blas.row_dot(a.t, b.t)
        with spy.expect("fmlx_blas_rowreduce"):
            got["gemv"] = blas.gemv(a.t, v)
        with spy.expect("fmlx_blas_gemv_t"):
            got["gemv_t"] = blas.gemv_t(a.t, m)
        a.check()
        b.check()
        got = {k: r.cpu() for k, r in got.items()}
        for k in ref:
            assert torch.allclose(got[k].double(), ref[k], rtol=tol, atol=tol), (kind, k)
        if base is None:
            base = got
        for k in ref:
            assert _bitwise(got[k], base[k]), (kind, k)


@pytest.mark.parametrize("dtype,d", BLAS_CASES)
@covers("fmlx_blas_normalize", "fmlx_blas_hdot", "fmlx_blas_gather_cols", "fmlx_blas_axpby")
def test_blas_elementwise_on_views(dtype, d, spy):
    """normalize, hdot, gather_cols and the in-place axpby / scal on a Y view (X and Y of different
    pitch, per-row alpha); tolerances of test_blas.py::test_dense_elementwise. A bf16 Y, which that
    test leaves out, is the fp32 value rounded to bf16: relative error up to 2^-9, asserted at 2^-8
    (+ 1e-5 absolute for the fp32 sum under cancellation). Bitwise equal to contig throughout (one
    thread per element by flat index i -> (i / d, i % d))."""
    from flink_ml_amd.ops import blas

    n = BLAS_N
    X, Y = _dense(n, d, 7, dtype), _dense(n, d, 8, dtype)
    g = torch.Generator().manual_seed(200 + d)
    v = torch.randn(d, generator=g, dtype=F64)
    alpha = torch.randn(n, generator=g, dtype=F64)
    ar = alpha if dtype == F64 else alpha.float().double()  # per-row alpha in the accumulator dtype
    Xr, Yr = X.double(), Y.double()
    tol = max(_tol(dtype), 1e-6 if dtype == F32 else 0)
    ytol = dict(rtol=2.0 ** -8, atol=1e-5) if dtype == BF16 else dict(rtol=tol, atol=tol)
    ps = (1.0, 2.0, 3.0, math.inf)
    cols = [d - 1, 0, d // 2]
    ref = {("normalize", p): Xr / torch.linalg.vector_norm(Xr, ord=p, dim=1)[:, None] for p in ps}
    ref["hdot"] = Xr * v[None, :]
    ref["axpby"] = ar[:, None] * Xr + 0.5 * Yr
    ref["scal"] = 2.0 * Yr
    ref["gather_cols"] = X[:, cols]
    vx = build_views(X)
    kinds = list(vx)
    base = None
    for i, kind in enumerate(kinds):
        a = vx[kind]
        ykind = "contig" if kind == "contig" else kinds[(i + 1) % len(kinds)]
        got = {}
        for p in ps:
            with spy.expect("fmlx_blas_normalize"):
                got["normalize", p] = blas.normalize(a.t, p)
        with spy.expect("fmlx_blas_hdot"):
            got["hdot"] = blas.hdot(v, a.t)
        with spy.expect("fmlx_blas_gather_cols"):
            got["gather_cols"] = blas.gather_cols(a.t, cols)
        y1, y2 = build_views(Y)[ykind], build_views(Y)[ykind]
        with spy.expect("fmlx_blas_axpby"):
            blas.axpby(alpha.to(dtype) if dtype == F32 else alpha, a.t, 0.5, y1.t)
        with spy.expect("fmlx_blas_axpby"):
            blas.scal(2.0, y2.t)
        got["axpby"], got["scal"] = y1.t, y2.t
        got = {k: r.cpu() for k, r in got.items()}
        for w in (a, y1, y2):
            w.check()
        for p in ps:
            assert torch.allclose(got["normalize", p].double(), ref["normalize", p], rtol=tol * 10, atol=tol * 10), (kind, p)
        assert torch.allclose(got["hdot"].double(), ref["hdot"], rtol=tol, atol=tol), kind
        assert torch.equal(got["gather_cols"], ref["gather_cols"]), kind
        assert torch.allclose(got["axpby"].double(), ref["axpby"], **ytol), (kind, ykind)
        assert torch.allclose(got["scal"].double(), ref["scal"], **ytol), (kind, ykind)
        if base is None:
            base = got
        for k in got:
            assert _bitwise(got[k], base[k]), (kind, k)


@pytest.mark.parametrize("dtype,d", [pytest.param(dt, d, id="%s-%d" % (_name(dt), d)) for dt in (F64, F32) for d in (3, 17, 100)])
@covers("fmlx_blas_gather_prod")
def test_blas_gather_prod_on_views(dtype, d, spy):
    """PolynomialExpansion's monomials (fp32 / fp64 rows; a term index >= d is the constant 1) with
    the tolerance of test_blas.py::test_gather_prod_polynomial_terms; bitwise equal to contig."""
    from flink_ml_amd.ops import blas

    n = BLAS_N
    X = _dense(n, d, 4, dtype)
    terms = torch.tensor([[0, d - 1, d], [d // 2, d // 2, d // 2], [d, d, d], [1 % d, 0, d - 1]], dtype=torch.int32)
    Xp = torch.cat([X.double(), torch.ones(n, 1, dtype=F64)], 1)
    ref = Xp[:, terms.long()].prod(2)
    base = None
    for kind, a in build_views(X).items():
        with spy.expect("fmlx_blas_gather_prod"):
            got = blas.gather_prod(a.t, terms).cpu()
        a.check()
        assert got.dtype == dtype and got.shape == ref.shape
        assert torch.allclose(got.double(), ref, rtol=_tol(dtype), atol=_tol(dtype)), kind
        base = got if base is None else base
        assert _bitwise(got, base), kind


@covers("fmlx_blas_interaction")
def test_blas_interaction_on_views(spy):
    """Three fp64 inputs, each on a different view kind (one stride per input); tolerance of
    test_blas.py::test_interaction; bitwise equal to the all-contig result."""
    from flink_ml_amd.ops import blas

    n = BLAS_N
    a, b, c = _dense(n, 3, 1), _dense(n, 17, 2), _dense(n, 2, 3)
    ref = (a[:, :, None, None] * b[:, None, :, None] * c[:, None, None, :]).reshape(n, -1)
    va, vb, vc = build_views(a), build_views(b), build_views(c)
    base = None
    for ka, kb, kc in (("contig", "contig", "contig"), ("pitch16", "pitch1", "rowslice"),
                       ("offset1", "rowslice", "pitch16"), ("pitch1", "offset1", "offset1"),
                       ("rowslice", "pitch16", "pitch1")):
        with spy.expect("fmlx_blas_interaction"):
            got = blas.interaction([va[ka].t, vb[kb].t, vc[kc].t]).cpu()
        for w in (va[ka], vb[kb], vc[kc]):
            w.check()
        assert torch.allclose(got, ref, rtol=1e-14, atol=1e-14), (ka, kb, kc)
        base = got if base is None else base
        assert _bitwise(got, base), (ka, kb, kc)


@pytest.mark.parametrize("vdtype", [F64, F32], ids=_name)
@covers("fmlx_blas_csr_axpy_dense")
def test_blas_csr_axpy_dense_into_views(vdtype, spy):
    """Sparse rows added in place into an fp64 Y view (first k columns); tolerance of
    test_blas.py::test_csr_ops; bitwise equal to contig (one thread per row, entries in order)."""
    from flink_ml_amd.ops import blas
    from flink_ml_amd.table import SparseColumn

    n, d, k = BLAS_N, 100, 50
    rng = np.random.default_rng(4)
    indptr, idx, val = [0], [], []
    for _ in range(n):
        cnt = int(rng.integers(0, 31))
        idx.extend(np.sort(rng.choice(d, size=cnt, replace=False)).tolist())
        val.extend(rng.normal(size=cnt).tolist())
        indptr.append(len(idx))
    Xs = SparseColumn(torch.tensor(indptr), torch.tensor(idx, dtype=torch.int32), torch.tensor(val, dtype=F64).to(vdtype), d)
    Y = _dense(n, d, 9)
    ref = 2.0 * Xs.to_dense(F64)
    ref[:, k:] = 0
    ref += Y
    Xg = SparseColumn(Xs.indptr.cuda(), Xs.indices.cuda(), Xs.values.cuda(), d)
    base = None
    for kind, y in build_views(Y).items():
        with spy.expect("fmlx_blas_csr_axpy_dense"):
            blas.csr_axpy_dense(2.0, Xg, y.t, k=k)
        got = y.t.cpu()
        y.check()
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12), kind
        base = got if base is None else base
        assert _bitwise(got, base), kind


# ------------------------------------------------------------------------------------------------
# column statistics (csrc/colstats.hip, groupstats.hip): scalar loads at r·ld + c
# ------------------------------------------------------------------------------------------------
STATS_N = 4099  # five partial blocks of colstats (1024 rows each) and a tail of 3 rows after its 4-row unroll
STATS_CASES = [pytest.param(dt, d, id="%s-%d" % (_name(dt), d)) for dt in (F32, F64, BF16) for d in (3, 37)]


@pytest.mark.parametrize("dtype,d", STATS_CASES)
@covers("fmlx_colstats", "fmlx_affine_cols")
def test_colstats_and_affine_on_views(dtype, d, spy):
    """column_stats (rtol 1e-9 / atol 1e-8, min and max exact) and affine_cols (the bound of
    test_feature_gpu.py::test_affine_kernel for fp32 output; fp64 output: three fp64 operations,
    1e-12). Bitwise equal to contig: a block owns the same row range, a thread the same columns."""
    from flink_ml_amd.ops import features as fo

    n = STATS_N
    g = torch.Generator().manual_seed(3 + d)
    X = (torch.randn((n, d), generator=g, dtype=F64) * 3 + 1).to(dtype)
    sub, add = torch.randn(d, generator=g, dtype=F64), torch.randn(d, generator=g, dtype=F64)
    mul = torch.rand(d, generator=g, dtype=F64)
    Xd = X.double()
    ref = {"sum": Xd.sum(0), "sumsq": (Xd * Xd).sum(0), "min": Xd.min(0).values, "max": Xd.max(0).values}
    aref = (Xd - sub) * mul + add
    atol = dict(rtol=1e-12, atol=1e-12) if dtype == F64 else dict(rtol=1e-6, atol=1e-5)
    base = None
    for kind, a in build_views(X).items():
        with spy.expect("fmlx_colstats"):
            st = fo.column_stats(a.t)
        with spy.expect("fmlx_affine_cols"):
            out = fo.affine_cols(a.t, sub, mul, add)
        with spy.expect("fmlx_affine_cols"):
            out2 = fo.affine_cols(a.t, None, mul, None)
        a.check()
        assert st["count"] == n
        got = {k: st[k].cpu() for k in ref}
        got["affine"], got["scale"] = out.cpu(), out2.cpu()
        torch.testing.assert_close(got["sum"], ref["sum"], rtol=1e-9, atol=1e-8)
        torch.testing.assert_close(got["sumsq"], ref["sumsq"], rtol=1e-9, atol=1e-8)
        torch.testing.assert_close(got["min"], ref["min"], rtol=0, atol=0)
        torch.testing.assert_close(got["max"], ref["max"], rtol=0, atol=0)
        torch.testing.assert_close(got["affine"].double(), aref, **atol)
        torch.testing.assert_close(got["scale"].double(), Xd * mul, **atol)
        base = got if base is None else base
        for k in got:
            assert _bitwise(got[k], base[k]), (kind, k)


@pytest.mark.parametrize("G", [1, 32])
@pytest.mark.parametrize("dtype,d", STATS_CASES)
@covers("fmlx_group_colstats")
def test_group_colstats_on_views(dtype, d, G, spy):
    """Per-group weighted column sums, Σx and Σx² (rtol 1e-9 / atol 1e-8 as in
    test_feature_gpu.py::test_group_colstats_kernel); bitwise equal to contig (row lanes and
    column lanes come from n, d and G alone)."""
    from flink_ml_amd.ops import features as fo

    n = STATS_N
    g = torch.Generator().manual_seed(11 + d + G)
    X = torch.randn((n, d), generator=g, dtype=F64).to(dtype)
    gi = torch.randint(0, G, (n,), generator=g)
    w = torch.randn(n, generator=g, dtype=F64)
    Xd = X.double()
    ref = (torch.zeros(G, d, dtype=F64).index_add_(0, gi, Xd * w[:, None]), Xd.sum(0), (Xd * Xd).sum(0))
    gic, wc = gi.cuda(), w.cuda()
    base = None
    for kind, a in build_views(X).items():
        with spy.expect("fmlx_group_colstats"):
            got = [r.cpu() for r in fo.group_colstats(a.t, gic, G, wc)]
        a.check()
        for r, e in zip(got, ref):
            torch.testing.assert_close(r, e, rtol=1e-9, atol=1e-8)
        base = got if base is None else base
        for r, b in zip(got, base):
            assert _bitwise(r, b), kind


# ------------------------------------------------------------------------------------------------
# contingency statistics (csrc/catstats.hip)
# ------------------------------------------------------------------------------------------------
# cs_flags / cs_hist take the 16-byte flat stream only for ld == d and a 16-byte-aligned base
# (contig, and rowslice where 3·d·es is a multiple of 16); every other view takes the FlatWalk
# (row, column) walk. Grids (fmlx_cs_flags: ceil(n·d / 4096) blocks, fmlx_cs_hist: ceil(n·d / 16384),
# 256 threads each):
#   n = 20011, d = 7:   flags 35 blocks, 8960 threads, 15.6 steps per thread, column step 8960 % 7 = 0;
#                       hist 9 blocks, 2304 threads, 60.8 steps, column step 2304 % 7 = 1
#   n = 1000, d = 300:  flags 74 blocks, 18944 threads, 15.8 steps, column step 18944 % 300 = 44;
#                       hist 19 blocks, 4864 threads, 61.7 steps, column step 4864 % 300 = 64
# so every thread takes well over two steps of the walk and the carry (j >= d after the column step)
# fires at both widths for cs_hist and at d = 300 for cs_flags.
CS_CASES = [pytest.param(dt, n, d, id="%s-%dx%d" % (_name(dt), n, d)) for dt in (F32, F64)
            for n, d in ((20011, 7), (1000, 300))]
CS_L, CS_LO, CS_RANGE = 3, -2, 5


def _cs_data(n, d, dtype):
    g = torch.Generator().manual_seed(n + d)
    X = torch.randint(CS_LO, CS_LO + CS_RANGE, (n, d), generator=g).to(dtype)
    X[0, 0], X[n - 1, d - 1] = CS_LO, CS_LO + CS_RANGE - 1  # both ends of the range, the last at the last element
    li = torch.randint(0, CS_L, (n,), generator=g)
    return X, li


def test_catstats_grids_give_every_thread_two_walk_steps():
    """The shapes above against the launchers' grid rules (csrc/catstats.hip fmlx_cs_flags /
    fmlx_cs_hist): at least two steps per thread, and a non-zero column step where claimed."""
    for n, d in ((20011, 7), (1000, 300)):
        total = n * d
        flags_threads = min(1024, -(-total // 4096)) * 256
        hist_threads = min(512, -(-total // 16384)) * 256
        assert total >= 2 * flags_threads and total >= 2 * hist_threads
        assert hist_threads % d != 0
    assert (min(1024, -(-300000 // 4096)) * 256) % 300 != 0


@pytest.mark.parametrize("dtype,n,d", CS_CASES)
@covers("fmlx_cs_flags", "fmlx_cs_hist", "fmlx_cs_ihist")
def test_catstats_integer_kernels_on_views(dtype, n, d, spy):
    """flags (min, max, any non-integer: exact), int_table (fmlx_cs_hist: [d, L, V] counts, exact
    against numpy) and the one-column histogram fmlx_cs_ihist — through catstats.int_hist, which
    copies the column first (documented above), and directly with the view's (ld, column).
    Integer results: equal to contig exactly."""
    from flink_ml_amd.ops import catstats, native

    X, li = _cs_data(n, d, dtype)
    Xf = X.clone()
    Xf[n - 1, d - 1] = 0.5  # a fraction in the very last element: only a walk that gets there sees it
    V = CS_RANGE
    ref = np.zeros((d, CS_L, V), dtype=np.int64)
    np.add.at(ref, (np.arange(d)[None, :].repeat(n, 0), li.numpy()[:, None].repeat(d, 1),
                    X.numpy().astype(np.int64) - CS_LO), 1)
    lic = li.cuda()
    j = d // 2
    href = np.bincount(X[:, j].numpy().astype(np.int64) - CS_LO, minlength=V)
    vf = build_views(Xf)
    for kind, a in build_views(X).items():
        with spy.expect("fmlx_cs_flags"):
            assert catstats.flags(a.t) == (float(CS_LO), float(CS_LO + V - 1), False), kind
        with spy.expect("fmlx_cs_flags"):
            assert catstats.flags(vf[kind].t) == (Xf.min().item(), Xf.max().item(), True), kind
        with spy.expect("fmlx_cs_hist"):
            tab = catstats.int_table(a.t, lic, CS_L, CS_LO, V).cpu().numpy()
        np.testing.assert_array_equal(tab, ref, err_msg=kind)
        with spy.expect("fmlx_cs_ihist"):
            h = catstats.int_hist(a.t[:, j], CS_LO, V).cpu().numpy()
        np.testing.assert_array_equal(h, href, err_msg=kind)
        counts = torch.zeros(V, dtype=torch.int32, device="cuda")
        with spy.expect("fmlx_cs_ihist"):
            native.call("fmlx_cs_ihist", native.dtype_code(dtype), native.ptr(a.t), a.t.stride(0), n, j, CS_LO, V,
                        native.ptr(counts), native.stream_ptr())
        np.testing.assert_array_equal(counts.cpu().numpy(), href, err_msg=kind)
        a.check()
        vf[kind].check()


@pytest.mark.parametrize("dtype,n,d", CS_CASES)
@covers("fmlx_cs_col_keys", "fmlx_cs_small_distinct")
def test_catstats_distinct_kernels_on_views(dtype, n, d, spy):
    """distinct_codes (fmlx_cs_col_keys feeds the sort: codes and sorted distinct values per column
    against torch.unique, exact) and bounded_distinct_counts (fmlx_cs_small_distinct; fp64 views only:
    the wrapper converts any other dtype to a contiguous fp64 copy first)."""
    from flink_ml_amd.ops import catstats

    X, _ = _cs_data(n, d, dtype)
    X[::5, 1] = -0.0  # folded into +0
    uniq = [torch.unique(X[:, c].double(), sorted=True, return_inverse=True) for c in range(d)]
    for kind, a in build_views(X).items():
        with spy.expect("fmlx_cs_col_keys"):
            codes, vals = catstats.distinct_codes(a.t)
        codes = codes.cpu()
        assert len(vals) == d
        for c in range(d):
            assert torch.equal(vals[c].cpu(), uniq[c][0]), (kind, c)
            assert torch.equal(codes[c], uniq[c][1].to(torch.int32)), (kind, c)
        with spy.expect("fmlx_cs_small_distinct"):
            cnt = catstats.bounded_distinct_counts(a.t, 8)
        np.testing.assert_array_equal(cnt, [u[0].numel() for u in uniq], err_msg=kind)
        with spy.expect("fmlx_cs_small_distinct"):
            over = catstats.bounded_distinct_counts(a.t, 3)  # fewer than the 5 distinct values: cap + 1
        np.testing.assert_array_equal(over, np.full(d, 4), err_msg=kind)
        a.check()


# ------------------------------------------------------------------------------------------------
# radix select (csrc/radixselect.hip): 16-column blocks, scalar loads
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 17])
@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@covers("fmlx_radix_hist")
def test_kth_smallest_device_on_views(dtype, d, spy):
    """Q = 3 ranks of every column (first, median, last of the non-NaN values) with ±inf, −0.0, NaNs
    and an all-equal column, at the 16-column block edge; exact against the sorted column and
    bitwise equal to contig (integer histograms)."""
    from flink_ml_amd.ops.quantile import kth_smallest_device

    n = 4099
    g = torch.Generator().manual_seed(d)
    X = (torch.randn(n, d, generator=g, dtype=F64) * 50).to(dtype)
    X[:, 0] = 7.0
    X[::9, 1], X[1::9, 1], X[2::9, 1] = float("inf"), float("-inf"), -0.0
    X[3::9, 1] = 0.0
    X[::5, 2] = float("nan")
    X[:, d - 1] = torch.round(X[:, d - 1] / 20)  # many duplicates in the last column (a lone 17th one)
    nv = (~torch.isnan(X)).sum(0)
    ks = torch.stack([torch.ones(d, dtype=torch.int64), nv // 2, nv])
    cols = [torch.sort(X[:, c][~torch.isnan(X[:, c])]).values for c in range(d)]
    views = build_views(X)
    base = None
    for kind in ("contig", "pitch1", "rowslice", "pitch16", "offset1"):
        a = views[kind]
        with spy.expect("fmlx_radix_hist"):
            got = kth_smallest_device(a.t, ks.cuda()).cpu()
        a.check()
        for c in range(d):
            for q in range(3):
                assert got[q, c] == cols[c][int(ks[q, c]) - 1], (kind, q, c)
        base = got if base is None else base
        assert _bitwise(got, base), kind


# ------------------------------------------------------------------------------------------------
# KMeans (csrc/kmeans.hip)
# ------------------------------------------------------------------------------------------------
KM_N, KM_K = 1000, 33


def _km_data(D, dtype, seed=0):
    g = torch.Generator().manual_seed(D * 1000 + KM_K + seed)
    X = torch.randn((KM_N, D), generator=g).to(dtype)
    C = torch.randn((KM_K, D), generator=g, dtype=F64)
    return X, C


def _km_views(X):
    """The builder's views plus ld = d + 2 (bf16: an even pitch that is no multiple of 8)."""
    views = build_views(X)
    views["pitch2"] = place(X, "cuda", 0, X.shape[1] + 2, 8, "pitch2")
    return views


def _bf16_route(t, D):
    """The A-fragment load path of fmlx_kmeans_assign_bf16 for a view (csrc/kmeans.hip
    launch_assign_bf16 and the kernel's non-FULL branch), or None where mfma_ok refuses it."""
    from flink_ml_amd.ops import kmeans as kk

    if not kk.mfma_ok(t, "euclidean"):
        return None
    base16, ld8 = t.data_ptr() % 16 == 0, t.stride(0) % 8 == 0
    if D == 16 * kk.mfma_ks(D) and ld8 and base16:
        return "full"
    return "uint4" if ld8 and base16 else "uint32"


# view -> route, per D (64 = 16·KS: FULL possible; 44: KS = 3 pads to 48, so never FULL, and the last
# 16-wide step holds 4 real elements: the element tail)
KM_BF16_ROUTES = {
    64: {"contig": "full", "pitch16": "full", "pitch2": "uint32", "offset4B": "uint32", "rowslice": "full",
         "pitch1": None, "offset1": None},
    44: {"contig": "uint32", "pitch16": "uint4", "pitch2": "uint32", "offset4B": "uint32", "rowslice": "uint32",
         "pitch1": None, "offset1": None},
}


def _assert_labels_vs_distances(lab, ref, d, what):
    """The comparison of test_kmeans.py::test_gpu_assign_bf16_matches_torch: the reference label, or a
    centroid whose distance is within fp32 accumulation-order noise of the reference's."""
    dsel = d.gather(1, lab[:, None]).squeeze(1)
    dref = d.gather(1, ref[:, None]).squeeze(1)
    assert torch.all((lab == ref) | ((dsel - dref).abs() <= 1e-3 * (1 + dref.abs()))), what
    assert (lab == ref).float().mean() > 0.99, what


@pytest.mark.parametrize("D", [64, 44])
@covers("fmlx_kmeans_assign_bf16", "fmlx_kmeans_assign_generic")
def test_kmeans_assign_bf16_on_views(D, spy):
    """Every A-fragment load path of the MFMA assign: FULL (contig: the pipelined kernel at D = 64;
    ld = 72 and the row slice as well; the plain FULL kernel with the pipelined schedule off),
    non-FULL with 16-byte loads (D = 44 at ld = 48, 16-byte-aligned base), non-FULL with four 4-byte
    loads (ld = 66 / 46, a base offset of 2 elements, D = 44 contiguous) and the element tail
    (D = 44). A 4-byte-aligned base with ld % 8 == 0 (offset4B at D = 64) must take the 4-byte
    loads: the kernel is told whether the base is 16-byte aligned. Labels equal contig exactly;
    against torch_assign on the bf16-rounded operands the comparison of
    test_gpu_assign_bf16_matches_torch. Views mfma_ok refuses (odd ld, 2-byte base) are asserted to
    take fmlx_kmeans_assign_generic on their fp32 copy instead (no skip), and the launcher itself
    answers −2 for them."""
    from flink_ml_amd.ops import kmeans as kk
    from flink_ml_amd.ops import native

    X, C = _km_data(D, BF16)
    assert (kk.mfma_ks(D) * 16 == D) == (D == 64)
    cb = kk.CentroidBuffers(KM_K, D, torch.device("cuda"), F32)
    cb.set(C)
    Xf, Cf = X.float(), C.to(BF16).float()
    dist = (Cf ** 2).sum(1)[None, :] - 2 * Xf @ Cf.T  # fp32 distances on the bf16-rounded operands
    ref = kk.torch_assign(Xf, Cf, "euclidean")
    C32 = C.float().double()  # the generic route: the bf16 rows as fp32, the centroids rounded to fp32 only
    gref = kk.torch_assign(Xf, C32, "euclidean")
    gdist = (C32 ** 2).sum(1)[None, :] - 2 * Xf.double() @ C32.T
    views = _km_views(X)
    assert set(views) == set(KM_BF16_ROUTES[D])
    base = None
    for kind, a in views.items():
        route = _bf16_route(a.t, D)
        assert route == KM_BF16_ROUTES[D][kind], (kind, route)
        if route is None:
            with spy.expect("fmlx_kmeans_assign_generic"):
                lab = kk.assign(a.t, cb, "euclidean").cpu().long()
            assert "fmlx_kmeans_assign_bf16" not in spy.names
            out = torch.empty(KM_N, dtype=torch.int32, device="cuda")
            with pytest.raises(RuntimeError, match=r"fmlx_kmeans_assign_bf16 failed with error -2$"):
                # the launcher refuses the view too (its narrowest loads are 4 bytes wide): nothing is launched
                native.call("fmlx_kmeans_assign_bf16", native.ptr(a.t), a.t.stride(0), KM_N, D, cb.KS, native.ptr(cb.Cb),
                            native.ptr(cb.cnorm_b), cb.kpad, native.ptr(out), native.ptr(cb.baug), native.stream_ptr())
            a.check()
            _assert_labels_vs_distances(lab, gref, gdist, kind)
            continue
        with spy.expect("fmlx_kmeans_assign_bf16"):
            lab = kk.assign(a.t, cb, "euclidean").cpu().long()
        a.check()
        _assert_labels_vs_distances(lab, ref, dist, kind)
        base = lab if base is None else base
        assert torch.equal(lab, base), kind
    if D == 64:  # the plain FULL kernel (what widths other than 64 / 128 take), on contig and ld = 72
        kk.set_assign_sched(0)
        try:
            for kind in ("contig", "pitch16"):
                with spy.expect("fmlx_kmeans_assign_bf16"):
                    lab = kk.assign(views[kind].t, cb, "euclidean").cpu().long()
                views[kind].check()
                assert torch.equal(lab, base), kind
        finally:
            kk.set_assign_sched(kk.ASSIGN_SCHED)


@pytest.mark.parametrize("D", [64, 44])
@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@covers("fmlx_kmeans_assign_generic")
def test_kmeans_assign_generic_on_views(dtype, D, spy):
    """The wave-per-row assign (scalar loads, next row prefetched with a clamped index); labels
    equal contig exactly, and against torch_assign the bound of
    test_kmeans.py::test_gpu_assign_generic plus the near-tie comparison above (fp64: exact)."""
    from flink_ml_amd.ops import kmeans as kk

    X, C = _km_data(D, dtype, seed=1)
    cb = kk.CentroidBuffers(KM_K, D, torch.device("cuda"), F64 if dtype == F64 else F32)
    cb.set(C)
    ref = kk.torch_assign(X, C.to(dtype), "euclidean")
    Xd, Cd = X.double(), C.to(dtype).double()
    dist = (Cd ** 2).sum(1)[None, :] - 2 * Xd @ Cd.T
    base = None
    for kind, a in _km_views(X).items():
        with spy.expect("fmlx_kmeans_assign_generic"):
            lab = kk.assign(a.t, cb, "euclidean").cpu().long()
        a.check()
        if dtype == F64:
            assert torch.equal(lab, ref), kind
        else:
            assert (lab == ref).float().mean() > 0.999, kind
            _assert_labels_vs_distances(lab, ref, dist, kind)
        base = lab if base is None else base
        assert torch.equal(lab, base), kind


def _km_round_case(dtype, D, spy, monkeypatch):
    """One KMeans round per view: the ordered chunk sums against an fp64 index_add over the round's
    own labels, with the bounds the KMeans round tests of test_kmeans.py use (rtol 1e-5 / atol 1e-3;
    fp64 rows, summed in fp64: 1e-12 / 1e-10), counts exact. Bitwise: equal to the contig payload of
    the same route — the two chunk-sum kernels add in different orders, and a bf16 view mfma_ok
    refuses is labelled by the generic assign, so contig is run once per route (16-byte form, plain
    form, plain form after the generic assign). Returns whether the 16-byte form ran."""
    from flink_ml_amd.ops import kmeans as kk

    X, C = _km_data(D, dtype, seed=2)
    k = KM_K
    cb = kk.CentroidBuffers(k, D, torch.device("cuda"), F64 if dtype == F64 else F32)
    cb.set(C)
    tol = dict(rtol=1e-12, atol=1e-10) if dtype == F64 else dict(rtol=1e-5, atol=1e-3)
    views = _km_views(X)

    def run(view, fast=None, mfma=None):
        rnd = kk.KMeansRound(view.t, k, "euclidean")
        if fast is not None:
            rnd.fast = fast
        with monkeypatch.context() as mp:
            if mfma is False:
                mp.setattr(kk, "mfma_ok", lambda X, metric: False)
            entry = "fmlx_kmeans_chunk_sum_bf16v" if rnd.fast else "fmlx_kmeans_chunk_sum"
            with spy.expect(entry):
                p = rnd.run(cb).cpu()
        view.check()
        return (bool(rnd.fast), mfma is not False and kk.mfma_ok(view.t, "euclidean")), p, rnd.labels.cpu().long()

    base = {}
    contig = views["contig"]
    for fast, mfma in ((None, None), (False, None), (False, False)):
        if (fast is None or mfma is None) or dtype == BF16:
            route, p, _ = run(contig, fast, mfma)
            base.setdefault(route, p)
    fast_seen = False
    for kind, a in views.items():
        route, p, lab = run(a)
        fast_seen |= route[0]
        got = p.double()
        sums = torch.zeros((k, D), dtype=F64).index_add_(0, lab, X.double())
        assert torch.allclose(got[:k * D].reshape(k, D), sums, **tol), kind
        assert torch.equal(got[k * D:], torch.bincount(lab, minlength=k).double()), kind
        assert route in base, (kind, route)
        assert _bitwise(p, base[route]), (kind, route)
    return fast_seen


@pytest.mark.parametrize("dtype,D", [pytest.param(dt, D, id="%s-%d" % (_name(dt), D))
                                     for dt, D in ((BF16, 44), (F32, 64), (F32, 44), (F64, 64), (F64, 44))])
@covers("fmlx_kmeans_chunk_sum")
def test_kmeans_round_chunk_sums_on_views(dtype, D, spy, monkeypatch):
    """fmlx_kmeans_chunk_sum (scalar loads; bf16 rows too: D = 44 is not one of the 16-byte form's
    widths) on every view, see _km_round_case."""
    assert not _km_round_case(dtype, D, spy, monkeypatch)


@covers("fmlx_kmeans_chunk_sum", "fmlx_kmeans_chunk_sum_bf16v")
def test_kmeans_round_bf16_chunk_sums_on_views(spy, monkeypatch):
    """bf16 rows of D = 64: fmlx_kmeans_chunk_sum_bf16v (one 16-byte load per lane and row) where the
    base is 16-byte aligned and ld % 8 == 0 (contig, ld = 72, the row slice), fmlx_kmeans_chunk_sum on
    every other view, see _km_round_case."""
    assert _km_round_case(BF16, 64, spy, monkeypatch)


# ------------------------------------------------------------------------------------------------
# KNN (csrc/knn.hip, knn_select.hip): scalar loads of Q[r·ldq + c] / G[r·ldg + j]
# ------------------------------------------------------------------------------------------------
def _int_data(nq, n, d, seed, lo=-3, hi=4):  # tests/test_knn_gpu.py: every distance exact in fp32
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(lo, hi, (nq, d), generator=g).double(), torch.randint(lo, hi, (n, d), generator=g).double())


def _ref_fp64(Q, T, k):
    d2 = ((Q * Q).sum(1)[:, None] + (T * T).sum(1)[None, :] - 2.0 * Q @ T.t()).abs().sqrt()
    s = torch.sort(d2, dim=1, stable=True)
    return s.indices[:, :k], s.values[:, :k]


@covers("fmlx_knn_fused")
def test_knn_fused_topk_query_views(spy):
    """Queries on every view kind (ldq != D, element-aligned base) against the fp64 stable ranking
    of integer data: indices exact, distances as in test_knn_gpu.py::test_fused_topk_exact_vs_fp64;
    bitwise equal to contig."""
    from flink_ml_amd.ops import knn as ko

    nq, n, D, k = 130, 4099, 24, 5
    Q, T = _int_data(nq, n, D, seed=24)
    pack = ko.TrainPack(T.float().cuda(), (T * T).sum(1).cuda())
    ridx, rdist = _ref_fp64(Q, T, k)
    base = None
    for kind, a in build_views(Q.float()).items():
        with spy.expect("fmlx_knn_fused"):
            idx, dist = ko.fused_topk(a.t, pack, k, with_dist=True)
        idx, dist = idx.cpu(), dist.cpu()
        a.check()
        assert torch.equal(idx.long(), ridx), kind
        torch.testing.assert_close(dist.double(), rdist, rtol=1e-6, atol=0)
        base = (idx, dist) if base is None else base
        assert _bitwise(idx, base[0]) and _bitwise(dist, base[1]), kind


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@covers("fmlx_knn_select")
def test_knn_select_topk_product_block_views(dtype, spy):
    """The product block with a row stride of n + 1 and n + 3 (and the builder's views): the k
    nearest columns equal the fp64 stable sort exactly (integer data, many ties) and the contig
    result."""
    from flink_ml_amd.ops import knn as ko

    nq, n, k = 7, 4099, 65
    Q, T = _int_data(nq, n, 11, seed=65 + (7 if dtype == F64 else 0))
    G = (Q @ T.t()).to(dtype)  # exact: small integers
    qn, tn = (Q * Q).sum(1).to(dtype).cuda(), (T * T).sum(1).to(dtype).cuda()
    ridx, _ = _ref_fp64(Q, T, k)
    views = build_views(G)
    views["ld=n+1"] = views.pop("pitch1")
    views["ld=n+3"] = place(G, "cuda", 0, n + 3, 8, "ld=n+3")
    assert views["ld=n+1"].t.stride(0) == n + 1 and views["ld=n+3"].t.stride(0) == n + 3
    base = None
    for kind, a in views.items():
        with spy.expect("fmlx_knn_select"):
            idx = ko.select_topk(a.t, qn, tn, k).cpu()
        a.check()
        assert torch.equal(idx.long(), ridx), kind
        base = idx if base is None else base
        assert _bitwise(idx, base), kind


# ------------------------------------------------------------------------------------------------
# GLM (csrc/glm.hip with_layout): one case per (dtype, EPC) it instantiates
# ------------------------------------------------------------------------------------------------
# (dtype, d, view) -> the (epc, cpl) ops.glm.pick_layout must answer, for the round and the predict
# kernel alike at these widths. A chunk is one load of epc·es bytes at X + r·ld + c·epc: aligned
# because pick_layout demands d % epc == 0, (ld·es) % (epc·es) == 0 and base % (epc·es) == 0.
GLM_CASES = [
    (BF16, 96, "contig", (8, 1)), (BF16, 96, "pitch16", (8, 1)), (BF16, 96, "rowslice", (8, 1)),
    (BF16, 100, "contig", (4, 1)),
    (BF16, 98, "contig", (2, 1)), (BF16, 96, "offset4B", (2, 1)),
    (BF16, 97, "contig", (1, 2)), (BF16, 96, "offset1", (1, 2)), (BF16, 96, "pitch1", (1, 2)),
    (F32, 100, "contig", (4, 1)), (F32, 100, "pitch16", (4, 1)), (F32, 100, "rowslice", (4, 1)),
    (F32, 102, "contig", (2, 1)), (F32, 102, "rowslice", (2, 1)),
    (F32, 101, "contig", (1, 2)), (F32, 100, "pitch1", (1, 2)), (F32, 100, "offset1", (1, 2)),
    (F64, 34, "contig", (2, 1)), (F64, 34, "pitch16", (2, 1)),
    (F64, 33, "contig", (1, 1)), (F64, 34, "pitch1", (1, 1)), (F64, 34, "offset1", (1, 1)),
    (F64, 33, "rowslice", (1, 1)),
]
GLM_LAYOUTS = {(BF16, 8), (BF16, 4), (BF16, 2), (BF16, 1), (F32, 4), (F32, 2), (F32, 1), (F64, 2), (F64, 1)}
_GLM_IDS = ["%s-%d-%s-epc%d" % (_name(dt), d, kind, lay[0]) for dt, d, kind, lay in GLM_CASES]


def test_glm_cases_reach_every_instantiated_chunk_width():
    assert {(dt, lay[0]) for dt, _, _, lay in GLM_CASES} == GLM_LAYOUTS


def _glm_ref_round(X, y, w, coef, B, e, loss):  # tests/test_glm_gpu.py _ref_round
    from flink_ml_amd.ops.glm import torch_loss_and_mult

    n = X.shape[0]
    P = (n + B - 1) // B
    s = (e % P) * B
    t = min(s + B, n)
    xb = X[s:t].to(F64)
    dot = xb @ coef.to(F64)
    l, m = torch_loss_and_mult(loss, dot, y[s:t].to(F64), w[s:t].to(F64))
    return m @ xb, w[s:t].sum().item(), l.sum().item()


@pytest.mark.parametrize("dtype,d,kind,layout", GLM_CASES, ids=_GLM_IDS)
@covers("fmlx_glm_grad_partials")
def test_glm_grad_partials_on_views(dtype, d, kind, layout, spy):
    """grad_partials at the narrow chunk widths and on views, every loss, rounds 0 and 3, with the
    bounds of test_glm_gpu.py::test_grad_partials_match_torch. No bitwise comparison with contig:
    another EPC changes which lane sums which element."""
    from flink_ml_amd.ops import glm as gk

    dev = torch.device("cuda:0")
    n, B = 5000, 1500
    acc = F64 if dtype == F64 else F32
    g = torch.Generator(device="cpu").manual_seed(d * 7)
    X = torch.rand((n, d), generator=g).to(dtype)
    y = torch.randint(0, 2, (n,), generator=g).to(F64)
    w = torch.rand(n, generator=g).to(F64) + 0.5
    coef = (torch.randn(d, generator=g) * 0.1).to(acc)
    a = build_views(X)[kind]
    assert gk.pick_layout(a.t) == layout
    nparts = max(1, min(512, -(-B // (gk.WPB * 16))))
    partials = torch.zeros((nparts, d + 2), dtype=acc, device=dev)
    yd, wd, cd = y.to(dev, acc), w.to(dev, acc), coef.to(dev)
    tol = 1e-9 if dtype == F64 else 2e-4
    for loss in (0, 1, 2):
        for e in (0, 3):
            state = torch.tensor([e, 1, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
            with spy.expect("fmlx_glm_grad_partials"):
                gk.grad_partials(a.t, yd, wd, cd, B, loss, state, partials, nparts)
            got = partials.sum(0).double().cpu()
            ref_g, ref_w, ref_l = _glm_ref_round(X, y, w, coef, B, e, loss)
            scale = max(1.0, ref_g.abs().max().item())
            assert torch.allclose(got[:d], ref_g, atol=tol * scale * 10, rtol=tol), (loss, e, (got[:d] - ref_g).abs().max())
            assert abs(got[d].item() - ref_w) <= tol * abs(ref_w) * 10, (loss, e)
            assert abs(got[d + 1].item() - ref_l) <= 1e-3 * abs(ref_l) + 1e-6, (loss, e)
    a.check()


@pytest.mark.parametrize("dtype,d,kind,layout", GLM_CASES, ids=_GLM_IDS)
@covers("fmlx_glm_predict")
def test_glm_predict_dense_on_views(dtype, d, kind, layout, spy):
    """predict_dense, the three modes, with the bounds of test_glm_gpu.py::test_predict_matches_torch."""
    from flink_ml_amd.ops import glm as gk

    g = torch.Generator(device="cpu").manual_seed(d + 3)
    X = torch.rand((3000, d), generator=g).to(dtype)
    coef = torch.randn(d, generator=g, dtype=F64) * 0.1
    a = build_views(X)[kind]
    assert gk.pick_layout(a.t, rounds=False) == layout
    dot_err = 1e-2 if dtype == BF16 else 1e-5
    for mode in (0, 1, 2):
        with spy.expect("fmlx_glm_predict"):
            pred, raw = gk.predict_dense(a.t, coef, mode, 0.1)
        rp, rr = gk.dots_to_outputs(X.double() @ coef, mode, 0.1)
        if mode == 2:
            assert torch.allclose(pred.cpu(), rp, atol=dot_err), mode
        else:
            assert torch.allclose(raw.cpu(), rr, atol=dot_err), mode
    a.check()


# ------------------------------------------------------------------------------------------------
def test_every_listed_entry_point_has_a_case():
    """The entry points the cases above declare (each asserts, through the launch spy, that it
    launched them) are exactly the fixed list: dropping a case fails here."""
    assert sorted(DECLARED) == ENTRY_POINTS
