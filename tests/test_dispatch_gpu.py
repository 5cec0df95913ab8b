"""Return codes of the dtype / width dispatch of the native entry points (csrc/dispatch.h): a dtype
code or width an entry point does not ship comes back as its error code through ``native.check``
and launches nothing (so no buffer is needed), and the entry points that answer 0 for an empty
input before they look at the dtype still do."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64, BF16, F16, I32, I64 = range(6)  # FmlxDType (csrc/common.h)

# (entry point, arguments without the trailing stream, return code)
CASES = [
    # blas.hip: dense rows ship f32 / f64 / bf16, CSR values f32 / f64; n <= 0 answers first
    ("fmlx_blas_rowreduce", (I64, 4, None, 8, None, 0, None, 4, 8, 2, 2.0, None), -1),
    ("fmlx_blas_rowreduce", (I64, 4, None, 8, None, 0, None, 0, 8, 2, 2.0, None), 0),
    ("fmlx_blas_normalize", (F16, 4, None, 8, 4, 8, 2.0, 0, None, 8), -1),
    ("fmlx_blas_normalize", (F16, 4, None, 8, 0, 8, 2.0, 0, None, 8), 0),
    ("fmlx_blas_axpby", (I32, None, 8, None, 8, 4, 8, 1.0, None, 1.0, None), -1),
    ("fmlx_blas_axpby", (I32, None, 8, None, 8, 4, 0, 1.0, None, 1.0, None), 0),
    ("fmlx_blas_hdot", (I64, None, 8, None, 4, 8, None, 8), -1),
    ("fmlx_blas_hdot", (I64, None, 8, None, 0, 8, None, 8), 0),
    ("fmlx_blas_gemv_t", (I64, None, 8, None, 4, 8, None, None, 0.0), -1),
    ("fmlx_blas_gemv_t", (I64, None, 8, None, 0, 8, None, None, 0.0), -1),
    ("fmlx_blas_csr_rowreduce", (BF16, 4, None, None, None, None, 4, 2, 2.0, None), -1),
    ("fmlx_blas_csr_rowreduce", (BF16, 4, None, None, None, None, 0, 2, 2.0, None), 0),
    ("fmlx_blas_csr_scale", (BF16, None, None, None, None, None, 4, None), -1),
    ("fmlx_blas_csr_scale", (BF16, None, None, None, None, None, 0, None), 0),
    ("fmlx_blas_csr_axpy_dense", (I32, None, None, None, 1.0, 4, 8, None, 8), -1),
    ("fmlx_blas_csr_axpy_dense", (I32, None, None, None, 1.0, 0, 8, None, 8), 0),
    ("fmlx_blas_csr_csr_dot", (BF16, None, None, None, None, None, None, 4, None), -1),
    ("fmlx_blas_csr_csr_dot", (BF16, None, None, None, None, None, None, 0, None), 0),
    ("fmlx_blas_gather_cols", (3, None, 8, None, 4, 2, None), -1),  # element size in bytes: 8 / 4 / 2
    ("fmlx_blas_gather_cols", (16, None, 8, None, 4, 2, None), -1),
    ("fmlx_blas_gather_cols", (3, None, 8, None, 0, 2, None), 0),
    ("fmlx_blas_gather_prod", (BF16, None, 8, 8, None, 2, 4, 3, None), -1),
    ("fmlx_blas_gather_prod", (BF16, None, 8, 8, None, 2, 0, 3, None), 0),
    ("fmlx_blas_gather_prod", (F32, None, 8, 8, None, 0, 4, 3, None), -1),
    # kmeans.hip
    ("fmlx_kmeans_assign_generic", (BF16, None, 8, 4, 8, None, None, 2, 0, None), -1),
    ("fmlx_kmeans_assign_generic", (BF16, None, 2000, 4, 2000, None, None, 2, 0, None), -1),
    ("fmlx_kmeans_assign_generic", (BF16, None, 8, 0, 8, None, None, 2, 0, None), 0),
    ("fmlx_kmeans_chunk_sum", (I64, None, 8, 8, None, None, None, 2, 0, None), -1),  # the dtype comes first
    ("fmlx_kmeans_chunk_sum", (F32, None, 1032, 1025, None, None, None, 2, 0, None), -3),  # then the width
    ("fmlx_kmeans_chunk_sum", (F32, None, 1024, 1024, None, None, None, 2, 0, None), 0),  # then "no chunks"
    ("fmlx_kmeans_chunk_sum_bf16v", (None, 24, 24, None, None, None, 2, 1, None), -2),
    ("fmlx_kmeans_chunk_sum_bf16v", (None, 1024, 1024, None, None, None, 2, 1, None), -2),
    ("fmlx_kmeans_chunk_sum_bf16v", (None, 16, 12, None, None, None, 2, 1, None), -2),
    ("fmlx_kmeans_chunk_sum_bf16v", (None, 24, 24, None, None, None, 2, 0, None), 0),
    ("fmlx_kmeans_assign_bf16", (None, 144, 4, 144, 9, None, None, 32, None, None), -2),  # KS = 9 is not shipped
    ("fmlx_kmeans_assign_bf16", (None, 144, 4, 144, 11, None, None, 32, None, None), -2),
    ("fmlx_kmeans_assign_bf16", (None, 144, 4, 144, 8, None, None, 32, None, None), -2),  # 16·KS < D
    # catstats.hip: cs_flags / cs_hist / cs_col_keys f64 / f32, cs_ihist also int32
    ("fmlx_cs_flags", (I32, None, 8, 4, 8, None, None), -1),
    ("fmlx_cs_ihist", (BF16, None, 8, 4, 0, 0, 4, None), -1),
    ("fmlx_cs_ihist", (BF16, None, 8, 4, 0, 0, 0, None), -2),
    ("fmlx_cs_hist", (I32, None, 8, 4, 8, None, 2, 0, 4, None), -1),
    ("fmlx_cs_hist", (I32, None, 8, 4, 8, None, 0, 0, 4, None), -2),
    ("fmlx_cs_col_keys", (I32, None, 8, 4, 0, 2, None, None, None), -1),
    # colstats.hip: the (in, out) pairs of fmlx_affine_cols are f32→f32, f64→f64, bf16→f32, f32→f64
    ("fmlx_colstats", (I64, None, 8, 4, 8, None, 1, None), -1),
    ("fmlx_colstats", (F32, None, 8, 4, 8, None, 0, None), -1),
    ("fmlx_affine_cols", (F64, F32, None, 8, 4, 8, None, None, None, None), -1),
    ("fmlx_affine_cols", (BF16, F64, None, 8, 4, 8, None, None, None, None), -1),
    ("fmlx_affine_cols", (BF16, BF16, None, 8, 4, 8, None, None, None, None), -1),
    ("fmlx_affine_cols", (F32, BF16, None, 8, 4, 8, None, None, None, None), -1),
    ("fmlx_affine_cols", (I32, F32, None, 8, 4, 8, None, None, None, None), -1),
    ("fmlx_affine_cols", (F64, F32, None, 8, 0, 8, None, None, None, None), -1),  # the pair comes first
    ("fmlx_affine_cols", (F32, F64, None, 8, 0, 8, None, None, None, None), 0),
    ("fmlx_affine_cols", (BF16, F32, None, 8, 0, 8, None, None, None, None), 0),
    # groupstats.hip, radixselect.hip, datagen.hip
    ("fmlx_group_colstats", (I64, None, 8, 4, 8, None, 1, None, None, 1, None), -1),
    ("fmlx_radix_hist", (BF16, None, 8, 4, 8, None, 1, 0, 1, 1, None, None), -1),
    ("fmlx_java_rows", (I64, 1, 0, 0, 4, None, None, 1, 1, 1, None, None, None), -1),
    # dct.hip, knn.hip: the checks in front of the width ladders
    ("fmlx_dct_rows", (None, 4, 129, None, None, 0, 0), -1),
    ("fmlx_dct_rows_f64", (None, 4, 0, None, None, 0, 0), -1),
    ("fmlx_dct_rows", (None, 0, 128, None, None, 0, 0), 0),
    ("fmlx_knn_topk", (None, 100, 4, 100, 1, None, None, 33, None, None, None, None), -1),
    ("fmlx_knn_topk", (None, 100, 0, 100, 1, None, None, 32, None, None, None, None), 0),
    ("fmlx_knn_fused", (None, 8, 4, 8, None, 100, 4, 65, 1, None, None, None, None), -1),
    ("fmlx_knn_fused", (None, 8, 4, 8, None, 100, 68, 4, 1, None, None, None, None), -1),
    ("fmlx_knn_fused", (None, 8, 0, 8, None, 100, 4, 64, 1, None, None, None, None), 0),
]


@pytest.mark.parametrize("name,args,code", CASES, ids=["%s:%d" % (c[0][5:], i) for i, c in enumerate(CASES)])
def test_return_code(name, args, code):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flink_ml_amd.ops import native

    args = args + (native.stream_ptr(),)
    assert getattr(native.kernels(), name)(*args) == code
    if code == 0:
        native.call(name, *args)
    else:
        with pytest.raises(RuntimeError, match=r"%s failed with error %d$" % (name, code)):
            native.call(name, *args)
