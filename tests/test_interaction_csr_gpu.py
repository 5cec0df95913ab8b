"""The CSR Interaction kernels (ops/csrc/interaction_csr.hip) on the cases and the numpy reference of
tests/test_interaction_csr.py: exact indices and products, bitwise equal to the CPU formulation and
to themselves under another chunk size, the refusals, and the stage taking the route."""
import numpy as np
import pytest
import torch

from flink_ml_amd.ops import blas, native
from flink_ml_amd.table import SparseColumn
from tests.test_interaction_csr import CASES, assert_is_reference, make_case, refusals, stage_case, stage_outputs

pytestmark = pytest.mark.gpu


def _cuda(cols):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = []
    for c in cols:
        if isinstance(c, SparseColumn) or c.dim() == 1:
            out.append(c.to("cuda"))
        else:  # every dense column as a strided view: ld = d + 1
            buf = torch.zeros((c.shape[0], c.shape[1] + 1), dtype=c.dtype, device="cuda")
            buf[:, :-1] = c.to("cuda")
            out.append(buf[:, :-1])
    return out


def _same(a, b):
    for x, y in ((a.indptr, b.indptr), (a.indices, b.indices), (a.values.view(torch.int64), b.values.view(torch.int64))):
        assert torch.equal(x.cpu(), y.cpu())


@pytest.mark.parametrize("name", CASES)
def test_matches_the_definition(name):
    cols = _cuda(make_case(name))
    out = blas.interaction_csr(cols)
    assert_is_reference(out, name)
    _same(out, blas.interaction_csr(make_case(name)))      # the CPU formulation
    _same(out, blas.interaction_csr(cols, chunk=768))      # chunks that end inside other pieces and rows


def test_fp32_values_widen_exactly():
    cols = [c.to(dtype=torch.float32) for c in make_case("ss_300x200")]
    _same(blas.interaction_csr(_cuda(cols)), blas.interaction_csr([c.to(dtype=torch.float64) for c in cols]))


@pytest.mark.parametrize("name", ["nan", "unsorted", "wide"])
def test_refusal_keeps_the_dense_route(monkeypatch, name):
    cols = _cuda(refusals()[name])
    assert blas.interaction_csr(cols) is None
    if name != "wide":
        got, want = (stage_outputs(monkeypatch, cols, route) for route in ("1", "0"))
        np.testing.assert_array_equal(got.to_dense().cpu().numpy(), want.to_dense().cpu().numpy())


def test_index_out_of_range_raises():
    a, b = _cuda(make_case("ss_7x5"))
    with pytest.raises(ValueError, match="sparse feature index out of range"):
        blas.interaction_csr([a, SparseColumn(b.indptr, b.indices, b.values, 4)])


def test_stage_takes_the_route(monkeypatch):
    cols = stage_case()
    seen, call = [], native.call
    monkeypatch.setattr(native, "call", lambda name, *a: (seen.append(name), call(name, *a))[1])
    out = stage_outputs(monkeypatch, _cuda(cols), "1")
    assert isinstance(out, SparseColumn) and "fmlx_interaction_csr_emit" in seen
    assert "fmlx_blas_interaction" not in seen
    dense = blas.interaction([c.to_dense() for c in cols])
    np.testing.assert_array_equal(out.to_dense().cpu().numpy(), dense.numpy())
