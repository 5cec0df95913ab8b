"""A/B of the two device paths of the DCT stage for rows wider than 128: the FFT kernel
(ops/csrc/dct_wide.hip, ``dct_rows_wide``) against the GEMM with the n × n basis already resident
(``Xd @ M.T``), per row type and n, on about 256 MB of rows.

Both paths alternate in one process; each shape is warmed, each side is timed with device events
over enough repetitions to fill 0.2 s, and the pair is then repeated in the reverse order. One JSON
line per shape: both times of both sides (ms per call, in the order measured), the bytes moved
(2 · rows · n · sizeof), the wide kernel's bytes/s and its share of the 6.2 TB/s streaming rate of
scripts/stream_probe.hip, and the max error of both paths against the exact reference of
tests/test_dct_wide.py on a 16-row sample (in units of eps · log2(L) · ‖x_row‖₂ as well).

The basis of the GEMM side is built on the device in fp64 by ``dct_matrix``'s formula and rounded
to the row type (the stage builds it on the host: the same values up to the last bit of cos; at
n = 16384 the host build alone takes 2 GiB and several seconds).

Usage: python scripts/bench_dct_wide.py [--out profiles/r10/dct_wide_ab.jsonl] [--mb 256]
       [--dtypes f32,f64] [--sizes 129,192,...]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [129, 192, 256, 384, 512, 1000, 1024, 2048, 4096, 8191, 8192, 16384]
STREAM_RATE = 6.2e12  # bytes/s, scripts/stream_probe.hip
MIN_SIDE_S = 0.2


def device_basis(n, dtype):
    k = torch.arange(n, dtype=torch.float64, device="cuda")[:, None]
    i = torch.arange(n, dtype=torch.float64, device="cuda")[None, :]
    m = torch.cos(math.pi * (2 * i + 1) * k / (2 * n))
    m[0] *= math.sqrt(1.0 / n)
    m[1:] *= math.sqrt(2.0 / n)
    return m.to(dtype)


def time_side(fn):
    """ms per call over ≥ MIN_SIDE_S of back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = max(3, int(math.ceil(MIN_SIDE_S * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "dct_wide_ab.jsonl"))
    ap.add_argument("--mb", type=float, default=256.0)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    a = ap.parse_args()
    from test_dct_wide import basis_product, fft_dct

    from flink_ml_amd.ops import dct as dk

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for name in a.dtypes.split(","):
            dtype = {"f32": torch.float32, "f64": torch.float64}[name]
            size = 8 if dtype == torch.float64 else 4
            eps = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
            for n in [int(s) for s in a.sizes.split(",")]:
                if not dk.dct_wide_supported(n, dtype):
                    continue
                rows = max(16, int(a.mb * 1e6 / (n * size)))
                g = torch.Generator().manual_seed(n)
                X = (torch.rand((rows, n), generator=g, dtype=torch.float64) * 2 - 1).to(dtype).cuda()
                M = device_basis(n, dtype)
                wide = lambda: dk.dct_rows_wide(X)  # noqa: E731
                gemm = lambda: X @ M.T  # noqa: E731
                for f in (wide, gemm, wide, gemm):  # warm: tables, code objects, GEMM heuristics
                    f()
                torch.cuda.synchronize()
                tw1, rw = time_side(wide)
                tg1, rg = time_side(gemm)
                tg2, _ = time_side(gemm)
                tw2, _ = time_side(wide)
                sample = X[:16].cpu()
                ref = basis_product(sample, n, False) if n <= 2048 else fft_dct(sample.double(), False)
                L = dk.wide_fft_len(n)
                unit = eps * math.log2(L) * sample.double().norm(dim=1, keepdim=True)
                ew = (wide()[:16].double().cpu() - ref).abs()
                eg = ((X[:16] @ M.T).double().cpu() - ref).abs()
                moved = 2 * rows * n * size
                best = min(tw1, tw2)
                rec = {"dtype": name, "n": n, "rows": rows, "L": L, "pow2": L == n,
                       "wide_ms": [round(tw1, 4), round(tw2, 4)], "gemm_ms": [round(tg1, 4), round(tg2, 4)],
                       "reps": [rw, rg], "bytes": moved, "wide_bytes_per_s": moved / (best * 1e-3),
                       "wide_share_of_stream": round(moved / (best * 1e-3) / STREAM_RATE, 4),
                       "wide_max_err": float(ew.max()), "gemm_max_err": float(eg.max()),
                       "wide_err_units": round(float((ew / unit).max()), 4),
                       "gemm_err_units": round(float((eg / unit).max()), 4),
                       "wide_wins_both_orders": max(tw1, tw2) < min(tg1, tg2)}
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                del X, M
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
