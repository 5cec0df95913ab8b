"""What the strided-view GPU tests (tests/test_strided_views_gpu.py) rest on, checked without a GPU:
the view builder produces the views it claims, and ``ops.glm.pick_layout`` / ``pick_wide_layout``
only ever answer a chunk width whose loads are aligned for the view they were asked about."""
import pytest
import torch

from flink_ml_amd.ops import glm as gk
from tests import test_strided_views_gpu as sv

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DTYPES = [F64, F32, BF16]


def _matrix(n, d, dtype):
    return (torch.arange(n * d, dtype=torch.float64).reshape(n, d) % 251 - 100).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES + [torch.int32], ids=sv._name)
@pytest.mark.parametrize("d", [1, 3, 7, 8, 17, 64, 100])
def test_view_builder_produces_what_it_claims(dtype, d):
    n = 5
    X = _matrix(n, d, dtype)
    es = X.element_size()
    views = sv.build_views(X, device="cpu")
    assert list(views) == ["contig", "pitch16", "pitch1", "offset1"] + (["offset4B"] if dtype == BF16 else []) + ["rowslice"]
    for kind, v in views.items():
        t = v.t
        assert t.shape == (n, d) and t.stride(1) == 1 and torch.equal(t, X), kind
        assert v.buf.data_ptr() % 16 == 0, kind
        # every cell outside the view is poisoned, and only those
        assert int(v.guard.sum()) == v.buf.numel() - n * d, kind
        out = v.buf[v.guard]
        if dtype.is_floating_point:
            assert bool(torch.isnan(out).all()), kind
            assert not bool(torch.isnan(v.buf[~v.guard]).any()), kind
        else:
            assert bool((out == torch.iinfo(dtype).min).all()), kind
        assert torch.equal(v.buf[~v.guard].reshape(n, d), X), kind
        v.check()
    c, p16, p1, o1, rs = (views[k].t for k in ("contig", "pitch16", "pitch1", "offset1", "rowslice"))
    assert c.stride(0) == d and c.data_ptr() % 16 == 0 and c.is_contiguous()
    assert p16.stride(0) > d and (p16.stride(0) * es) % 16 == 0 and p16.data_ptr() % 16 == 0
    assert p1.stride(0) == d + 1 and p1.data_ptr() % 16 == 0
    assert o1.stride(0) == d and o1.data_ptr() % 16 == es and o1.is_contiguous()
    assert rs.stride(0) == d and rs.is_contiguous()
    assert rs.data_ptr() - views["rowslice"].buf.data_ptr() == sv.ROWSLICE_START * d * es and sv.ROWSLICE_START % 2 == 1
    if dtype == BF16:
        o4 = views["offset4B"].t
        assert o4.stride(0) == d and o4.data_ptr() % 16 == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=sv._name)
def test_view_check_catches_a_stray_write_and_allows_in_place_updates(dtype):
    X = _matrix(6, 5, dtype)
    for kind, v in sv.build_views(X, device="cpu").items():
        v.t.mul_(2)  # in place inside the view: allowed
        v.check()
        if not bool(v.guard.any()):
            assert kind == "contig"
            continue
        cell = int(torch.nonzero(v.guard)[-1])
        v.buf[cell] = 1.0
        with pytest.raises(AssertionError, match="outside the view"):
            v.check()
    # a NaN of another bit pattern is a change too
    v = sv.build_views(X, device="cpu")["pitch1"]
    cell = int(torch.nonzero(v.guard)[0])
    v._bits()[cell] ^= 1
    assert bool(torch.isnan(v.buf[cell]))
    with pytest.raises(AssertionError, match="outside the view"):
        v.check()


def _all_views(d, dtype):
    X = torch.zeros((4, d), dtype=dtype)
    views = sv.build_views(X, device="cpu")
    es = X.element_size()
    views["pitch2"] = sv.place(X, "cpu", 0, d + 2, 8, "pitch2")
    views["offset3"] = sv.place(X, "cpu", 3, d, 5, "offset3")
    views["pitch16+offset"] = sv.place(X, "cpu", 16 // es + 1, sv.pitch16_ld(d, es), 8, "pitch16+offset")
    return views


@pytest.mark.parametrize("dtype", DTYPES, ids=sv._name)
def test_pick_layout_keeps_chunk_loads_aligned(dtype):
    """Every view kind x d in 1..129: pick_layout answers None or an (epc, cpl) whose chunk of
    epc·es bytes divides the width, the pitch and the base address, and whose 64·cpl lanes' chunks
    cover the row."""
    es = torch.empty(0, dtype=dtype).element_size()
    seen = set()
    for d in range(1, 130):
        for kind, v in _all_views(d, dtype).items():
            t = v.t
            for rounds in (True, False):
                lay = gk.pick_layout(t, rounds=rounds)
                assert lay is not None, (kind, d)  # (these widths fit one wave at any chunk width)
                epc, cpl = lay
                vb = epc * es
                assert vb in (16, 8, 4, 2) and vb <= 16, (kind, d)
                assert d % epc == 0, (kind, d)
                assert (t.stride(0) * es) % vb == 0, (kind, d)
                assert t.data_ptr() % vb == 0, (kind, d)
                assert 64 * cpl * epc >= d and cpl in (1, 2, 4, 8), (kind, d)
                seen.add(epc)
    assert seen == {e for e in (8, 4, 2, 1) if e * es <= 16}
    # too wide for the register-resident kernel: None, not a narrower chunk that does not cover the row
    assert gk.pick_layout(torch.zeros((2, 64 * 8 * (16 // es) + 16 // es), dtype=dtype)) is None
    assert gk.pick_layout(torch.zeros((2, 8, 2), dtype=dtype)) is None
    assert gk.pick_layout(torch.zeros((8, 4), dtype=dtype).t()) is None


@pytest.mark.parametrize("dtype", DTYPES, ids=sv._name)
def test_pick_wide_layout_takes_16_byte_aligned_views_only(dtype):
    es = torch.empty(0, dtype=dtype).element_size()
    epc16 = 16 // es
    accepted = 0
    for d in list(range(1, 70)) + [4096, 4096 + epc16, 4097]:
        for kind, v in _all_views(d, dtype).items():
            t = v.t
            lay = gk.pick_wide_layout(t)
            aligned = t.data_ptr() % 16 == 0 and (t.stride(0) * es) % 16 == 0
            if not aligned:
                assert lay is None, (kind, d)
            if lay is not None:
                accepted += 1
                epc, cpl = lay
                assert epc == epc16 and d % epc == 0 and aligned, (kind, d)
                assert gk.WIDE_WAVES * 64 * cpl * epc >= d, (kind, d)
    assert accepted > 0


@pytest.mark.parametrize("dtype,d,kind,layout", sv.GLM_CASES, ids=sv._GLM_IDS)
def test_glm_view_cases_name_the_layout_pick_layout_answers(dtype, d, kind, layout):
    """The table the GPU cases assert before launching, on the same views built on the CPU."""
    t = sv.build_views(torch.zeros((4, d), dtype=dtype), device="cpu")[kind].t
    assert gk.pick_layout(t) == layout and gk.pick_layout(t, rounds=False) == layout


def test_gpu_module_bookkeeping():
    """The parts of the GPU module that need no GPU: its GLM cases reach every (dtype, chunk width)
    csrc/glm.hip with_layout instantiates, the catstats shapes give every thread two steps of the
    walk, and the entry points its cases declare are the fixed list."""
    sv.test_glm_cases_reach_every_instantiated_chunk_width()
    sv.test_catstats_grids_give_every_thread_two_walk_steps()
    sv.test_every_listed_entry_point_has_a_case()
    assert len(set(sv.ENTRY_POINTS)) == len(sv.ENTRY_POINTS)
