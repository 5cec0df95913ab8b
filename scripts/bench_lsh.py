"""A/B of the two device paths of the MinHashLSH search: the kernels of ops/csrc/lsh_join.hip
(``ops/lsh.py`` similarity_join / nearest) against the torch formulation they replace
(``FMLX_LSH_NATIVE=0``: the code of the commit before), on one GPU.

Inputs (generated on the device from a seed, outside every timed window): n rows of about 32
distinct indices out of d = 100,000 for A; every B row is an A row (a permutation of them) with
about a tenth of its elements replaced, so the join is not empty. 5 tables × 3 functions,
threshold 0.3. The signatures are computed once per size (``minhash.hip``), outside the timing.

Both paths alternate in one process: each is warmed once per size, then timed native, torch,
torch, native (host clock around calls that end in a device synchronise; the ops read their
results' sizes back, so a call is a whole number of launches and read-backs). Peak device memory
above what is allocated before the call is taken from ``torch.cuda.max_memory_allocated`` in a
separate call of each path. A path that runs out of memory is recorded as such, and skipped for
the larger sizes. One JSON line per size and op.

``--once N``: no timing; one ``MinHashLSHModel.approx_similarity_join`` of two device-resident
tables of N rows on the native path (the inputs are generated on the host), for a kernel trace:
rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_lsh.py --once 100000

Usage: python scripts/bench_lsh.py [--out profiles/r11/lsh_ab.jsonl] [--sizes 10000,...]
       [--max-torch 1000000] [--ops join,nearest]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [10_000, 30_000, 100_000, 300_000, 1_000_000]
D, NNZ, TABLES, FUNCS, THRESHOLD = 100_000, 32, 5, 3, 0.3


def make_sets(n, seed):
    """(A, B) SparseColumns on the device: A rows of ~32 distinct sorted indices; B row i = A row
    perm[i] with each element replaced with probability 0.1 (duplicates removed)."""
    from flink_ml_amd.table import SparseColumn

    g = torch.Generator(device="cuda").manual_seed(seed)

    def csr(cols):  # [n, NNZ] candidate indices → sorted distinct rows
        cols = torch.sort(cols, dim=1).values
        keep = torch.ones_like(cols, dtype=torch.bool)
        keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
        ptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        ptr[1:] = torch.cumsum(keep.sum(1), 0)
        ind = cols[keep].to(torch.int32)
        return SparseColumn(ptr, ind, torch.ones(ind.numel(), dtype=torch.float64, device="cuda"), D)

    a = torch.randint(0, D, (n, NNZ), generator=g, device="cuda")
    perm = torch.randperm(n, generator=g, device="cuda")
    swap = torch.rand((n, NNZ), generator=g, device="cuda") < 0.1
    b = torch.where(swap, torch.randint(0, D, (n, NNZ), generator=g, device="cuda"), a[perm])
    return csr(a), csr(b)


def timed(fn, min_s=0.3, max_reps=40):
    """(ms per call, last result): one call, then as many as fill ``min_s`` (a call ends in a
    device synchronise of its own; the clock is the host's)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    reps = min(max_reps, int(min_s / max(first, 1e-6)))
    if reps < 2:
        return first * 1e3, out
    del out
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del out
    return round(grown / 2 ** 20, 1)


def with_env(value, fn):
    def run():
        os.environ["FMLX_LSH_NATIVE"] = value
        try:
            return fn()
        finally:
            os.environ.pop("FMLX_LSH_NATIVE", None)

    return run


def ab(name, n, native, torch_path, torch_alive, same):
    """One record: times in the order native, torch, torch, native; peaks; equality of results."""
    rec = {"op": name, "n": n}
    _, ref = timed(native)  # warm
    if torch_alive:
        try:
            _, old = timed(torch_path)  # warm
            rec["equal"] = bool(same(ref, old))
            del old
        except torch.OutOfMemoryError:
            torch_alive = False
            rec["torch"] = "out of memory"
    del ref
    torch.cuda.empty_cache()
    t = {"native": [], "torch": []}
    for side in ("native", "torch", "torch", "native"):
        if side == "torch" and not torch_alive:
            continue
        ms, out = timed(native if side == "native" else torch_path)
        t[side].append(round(ms, 3))
        del out
    rec["native_ms"], rec["torch_ms"] = t["native"], t["torch"]
    rec["native_peak_mib"] = peak(native)
    if torch_alive:
        rec["torch_peak_mib"] = peak(torch_path)
        rec["native_wins_both_orders"] = max(t["native"]) < min(t["torch"])
    return rec, torch_alive


def once(n):
    """One stage-level join of host-generated tables moved to the device."""
    import numpy as np

    from flink_ml_amd import Table
    from flink_ml_amd.models import MinHashLSH
    from flink_ml_amd.table import SparseColumn

    rng = np.random.default_rng(n)
    a = np.sort(rng.integers(0, D, (n, NNZ)), axis=1)
    b = np.sort(np.where(rng.random((n, NNZ)) < 0.1, rng.integers(0, D, (n, NNZ)), a[rng.permutation(n)]), axis=1)

    def table(cols):
        keep = np.ones(cols.shape, dtype=bool)
        keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
        ptr = np.zeros(n + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(keep.sum(1))
        ind = torch.from_numpy(cols[keep].astype(np.int32))
        sc = SparseColumn(torch.from_numpy(ptr), ind, torch.ones(ind.numel(), dtype=torch.float64), D)
        return Table({"id": list(range(n)), "vec": sc}).to("cuda")  # (ids stay on the host, as a list)

    ta, tb = table(a), table(b)
    model = MinHashLSH().set_input_col("vec").set_output_col("hashes").set_seed(2022).set_num_hash_tables(TABLES) \
        .set_num_hash_functions_per_table(FUNCS).fit(ta)
    torch.cuda.synchronize()
    out = model.approx_similarity_join(ta, tb, THRESHOLD, "id")
    torch.cuda.synchronize()
    print(json.dumps({"once": n, "pairs": out.num_rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "lsh_ab.jsonl"))
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--max-torch", type=int, default=SIZES[-1], help="largest n the torch path is run at")
    ap.add_argument("--ops", default="join,nearest")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lsh.py measures on a GPU"
    if a.once:
        return once(a.once)
    from flink_ml_amd.models.feature.lsh import generate_model_data
    from flink_ml_amd.ops import lsh as ops

    _, _, ca, cb = generate_model_data(TABLES, FUNCS, D, 2022)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    alive = {"join": True, "nearest": True}
    with open(a.out, "w") as out:
        for n in [int(s) for s in a.sizes.split(",")]:
            sa, sb = make_sets(n, n)
            ha = ops.minhash(sa, ca, cb).reshape(-1, TABLES, FUNCS)
            hb = ops.minhash(sb, ca, cb).reshape(-1, TABLES, FUNCS)
            kset = sb.slice(0, 1)  # the key: B's first row (a near-copy of some A row)
            kh = hb[0].clone()
            torch.cuda.synchronize()
            calls = {"join": lambda: ops.similarity_join(ha, hb, sa, sb, THRESHOLD),
                     "nearest": lambda: ops.nearest(ha, kh, sa, kset, 10)}
            for name in a.ops.split(","):
                same = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))  # noqa: E731
                rec, alive[name] = ab(name, n, calls[name], with_env("0", calls[name]),
                                      alive[name] and n <= a.max_torch, same)
                if name == "join":
                    rec["pairs"] = int(calls[name]()[0].numel())
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
            del sa, sb, ha, hb
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
