"""Panel-multiplicity timings on one GPU: csa_unique_mult_async + csa_mult_spectrum_async
against csa_unique_async -- the distinct count every run already pays -- over the same device buffers in
the same process, and the product call legacy_panel_distribution against legacy_probabilities.

Inputs (--panels, default 10^6 drawn panels each): sf_e_110 (W = 27, every panel distinct) and couples
(W = 1, 100 distinct panels: every copy of a panel on one LDS address).  Each variant is warmed up, then
timed --reps times with device events, the variants alternating within a repetition; the median and the
spread go to --out.  The list must be as long as the distinct count and sum to the number of panels.

Usage:  python tools/multiplicity_bench.py [--panels N] [--reps R] [--out profiles/panel_multiplicity_rows.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, REPO)
PKG = "citizensassemblies-replication_amd"
INST = os.path.join(REPO, "tests", "golden", "instances")
INPUTS = [("sf_e_110", "sf_e_110", 110), ("couples", "couples_panel_from_twenty_people_no_constraints_2", 2)]


def instance(pkg, inst_dir, k):
    d = os.path.join(INST, inst_dir)
    return pkg.read_instance(os.path.join(d, "categories.csv"), os.path.join(d, "respondents.csv"), k)


def device_batch(pkg, A, N, inst, S, seed):
    """The batch's panels (device int64 words) and their hashes, as legacy_sample_device holds them."""
    import torch
    enc = pkg.encode(inst.categories, inst.agents)
    raw = A.legacy_sample_device(enc, inst.k, S, seed, keep_panels=True)
    panels = raw.panels
    hashes = torch.empty(2 * S, dtype=torch.int64, device=panels.device)
    N.check(N.lib().csa_panel_hash_async(N.ptr(panels), S, enc.W, N.ptr(hashes), None))
    torch.cuda.synchronize()
    return enc.W, panels, hashes, raw.unique


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def kernel_rows(N, name, W, panels, hashes, unique, S, reps, warmup):
    import torch
    D = importlib.import_module(PKG + ".distributed")
    L = N.lib()
    dev = panels.device
    st = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(st.cuda_stream)
    table = D.HashTable(S, dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    need = int(L.csa_unique_mult_scratch_bytes(S))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    first = torch.empty(S, dtype=torch.int32, device=dev)
    mult = torch.empty(S, dtype=torch.int32, device=dev)
    n_bins = 4096
    out = torch.empty(1 + n_bins + 4, dtype=torch.int64, device=dev)

    def run_unique():
        table.count.zero_()
        N.check(L.csa_unique_async(N.ptr(hashes), N.ptr(panels), S, W, N.ptr(table.table), table.slots,
                                   N.ptr(table.count), N.ptr(status), sp))

    def run_mult(spectrum=True):
        N.check(L.csa_unique_mult_async(N.ptr(hashes), N.ptr(panels), S, W, N.ptr(scratch), need, N.ptr(first),
                                        N.ptr(mult), N.ptr(out), N.ptr(status), sp))
        if spectrum:
            N.check(L.csa_mult_spectrum_async(N.ptr(mult), N.ptr(out), S, N.ptr(out[1:]), n_bins,
                                              N.ptr(out[1 + n_bins:]), sp))

    variants = {"unique": run_unique, "mult": run_mult, "mult_list_only": lambda: run_mult(False)}
    # results first: the list is as long as the distinct count and sums to S, in the list and in the summary
    run_mult()
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    ln = int(h[0])
    assert ln == unique and int(h[-1]) == S and int(status[0].item()) == 0, (name, ln, unique, int(h[-1]))
    assert int(mult[:ln].cpu().numpy().view(np.uint32).astype(np.int64).sum()) == S
    assert len(np.unique(first[:ln].cpu().numpy())) == ln
    run_unique()
    torch.cuda.synchronize()
    assert int(table.count.item()) == unique
    times = {v: [] for v in variants}
    for r in range(warmup + reps):
        for v, fn in variants.items():         # alternating: every repetition runs every variant once
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            if r >= warmup:
                times[v].append(e0.elapsed_time(e1))
    row = {"input": name, "panels": S, "W": W, "distinct": unique, "max_multiplicity": int(h[-3]),
           "timing": "device events around the enqueue(s), median of reps after %d warm-up repetitions" % warmup}
    row.update({v: summary(ms) for v, ms in times.items()})
    for v in variants:
        if v != "unique":
            row[v]["over_unique"] = round(row[v]["median_ms"] / row["unique"]["median_ms"], 3)
    return row


def call_rows(A, inst, S, seed, reps):
    """legacy_panel_distribution against legacy_probabilities: host clock around the whole call (each ends
    in its one host copy), alternating, after one warm-up of each."""
    import torch
    calls = {"legacy_probabilities": lambda: A.legacy_probabilities(inst, S, seed),
             "legacy_panel_distribution": lambda: A.legacy_panel_distribution(inst, S, seed)}
    times = {c: [] for c in calls}
    for r in range(1 + reps):
        for c, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if r:
                times[c].append((time.perf_counter() - t0) * 1e3)
            del res
    row = {"input": "sf_e_110", "panels": S, "timing": "host clock around the call, device idle before and after"}
    row.update({c: summary(ms) for c, ms in times.items()})
    row["added_ms"] = round(row["legacy_panel_distribution"]["median_ms"] - row["legacy_probabilities"]["median_ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panels", type=int, default=10 ** 6)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--call-reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "panel_multiplicity_rows.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("multiplicity_bench: no HIP device (a timing needs the GPU)")
    pkg = importlib.import_module(PKG)
    A = importlib.import_module(PKG + ".analysis")
    N = importlib.import_module(PKG + "._native")
    rows = {"device": torch.cuda.get_device_name(0), "kernels": [], "calls": []}
    for name, inst_dir, k in INPUTS:
        inst = instance(pkg, inst_dir, k)
        W, panels, hashes, unique = device_batch(pkg, A, N, inst, a.panels, 0)
        row = kernel_rows(N, name, W, panels, hashes, unique, a.panels, a.reps, a.warmup)
        print(json.dumps(row), flush=True)
        rows["kernels"].append(row)
        del panels, hashes
    row = call_rows(A, instance(pkg, "sf_e_110", 110), a.panels, 0, a.call_reps)
    print(json.dumps(row), flush=True)
    rows["calls"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
