"""Per-call cost of the sharded product path on one GPU: a one-rank RCCL process
group (backend "nccl") with the 24-byte key exchange forced on (CSA_FORCE_EXCHANGE=1, the world > 1
path: packed pair all_reduce, key all_to_alls, owner re-draws, one all_reduce of counts + statistics +
distinct count), then distributed.legacy_probabilities_distributed called repeatedly at one GPU's
share of BASELINE config 3 (1.25e6 example_large_200 panels) and config 5 (1.25e7 synthetic n = 8192
panels).  Every call after the first reuses the cached encoding, pipeline and exchange; the
per-stage host timings (setup / device incl. the one host wait / finish) are printed with the
results' invariants checked.  found_panels keep nothing (they are re-drawn where read), so
keep_panels=True and False cost the same per call; the re-draw itself (found.rows() on this rank,
alone) is timed separately.  Compare with `bench.py --job-panels P` for the same share (the same
kernels without the API).  Prints one JSON line.

``--multiplicity``: distributed.legacy_panel_distribution_distributed (the 32-byte exchange: the counts
travel with the keys, the owner merges, spectrum and top candidates inside the call) timed beside the plain
sharded call, alternating, at the config-3 share and at 10^6 sf_e_110 panels; both printed with their
``timings`` stages, every repetition kept.  On a tree without the new call only the plain call is timed, so
the same file run from a checkout of the parent commit gives the parent's figures.

Usage (GPU box): python tools/dist_call_bench.py [S_config3] [S_config5] [calls]
                 python tools/dist_call_bench.py --multiplicity [S_config3] [S_sf_e] [repetitions]"""
import json
import os
import socket
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import importlib  # noqa: E402

P = importlib.import_module("citizensassemblies-replication_amd")
A = importlib.import_module("citizensassemblies-replication_amd.analysis")
D = importlib.import_module("citizensassemblies-replication_amd.distributed")


def run(name, k, S, calls, modes):
    import torch
    d = os.path.join(REPO, "tests", "golden", "instances", name)
    inst = P.read_instance(os.path.join(d, "categories.csv"), os.path.join(d, "respondents.csv"), k)
    out = {"instance": name, "k": k, "panels": S}
    for label, kw in modes:
        rows = []
        for c in range(calls):
            torch.cuda.synchronize()
            tm = {}
            t = time.perf_counter()
            alloc, found, hist = D.legacy_probabilities_distributed(inst, S, 0, timings=tm, **kw)
            dt = time.perf_counter() - t
            total = sum(alloc.values())
            assert abs(total - k) < 1e-6 * k, total                      # sum of probabilities = k
            rows.append(dict(tm, call_ms=dt * 1e3))
        redraw_ms = None
        # (the host dedupe of rows() -- np.unique over S rows of W words, as the one-GPU call's -- is the cost
        # past a few GB: timed at the config-3 share only)
        if kw.get("keep_panels", True) and S * ((len(inst.agents) + 63) // 64) <= (64 << 20):
            t = time.perf_counter()
            u = found.rows()
            redraw_ms = (time.perf_counter() - t) * 1e3
            assert len(u) == len(found)
        best = min(rows[1:] or rows, key=lambda r: r["call_ms"])
        out[label] = {"calls_ms": [round(r["call_ms"], 3) for r in rows], "second_call_ms": round(rows[1]["call_ms"], 3)
                      if len(rows) > 1 else None, "best": {k_: round(v, 3) for k_, v in best.items()},
                      "panels_per_s_best": S / (best["call_ms"] / 1e3), "unique": len(found),
                      "stats": A.LAST_RUN_STATS, "found_rows_redraw_ms": redraw_ms}
        print(json.dumps({name: {label: out[label]}}), file=sys.stderr, flush=True)
    return out


def run_multiplicity(name, k, S, reps):
    """The plain sharded call and the multiplicity call, alternating, ``reps`` timed repetitions each after
    one untimed call of each (which builds the cached pipeline and exchange buffers)."""
    import torch
    d = os.path.join(REPO, "tests", "golden", "instances", name)
    inst = P.read_instance(os.path.join(d, "categories.csv"), os.path.join(d, "respondents.csv"), k)
    calls = [("plain", D.legacy_probabilities_distributed)]
    if hasattr(D, "legacy_panel_distribution_distributed"):
        calls.append(("multiplicity", D.legacy_panel_distribution_distributed))
    rows = {label: [] for label, _ in calls}
    extra = {}
    for rep in range(reps + 1):
        for label, fn in calls:
            torch.cuda.synchronize()
            tm = {}
            t = time.perf_counter()
            res = fn(inst, S, 0, timings=tm)
            dt = time.perf_counter() - t
            assert abs(sum(res[0].values()) - k) < 1e-6 * k
            if rep:
                rows[label].append({k_: round(v, 3) for k_, v in dict(tm, call_ms=dt * 1e3).items()})
            if label == "multiplicity":
                dd = res[3]
                assert dd.S == S and dd.distinct == len(res[1])
                extra = {"distinct": dd.distinct, "max_multiplicity": dd.max_multiplicity, "coverage": dd.coverage()}
    out = {"instance": name, "k": k, "panels": S, **extra}
    for label, _ in calls:
        ms = sorted(r["call_ms"] for r in rows[label])
        out[label] = {"median_call_ms": ms[len(ms) // 2], "min_call_ms": ms[0], "max_call_ms": ms[-1], "calls": rows[label]}
    if len(calls) == 2:
        out["added_median_ms"] = round(out["multiplicity"]["median_call_ms"] - out["plain"]["median_call_ms"], 3)
    return out


def main_multiplicity(argv):
    import torch
    import torch.distributed as dist
    s3 = int(argv[0]) if len(argv) > 0 else 1250000
    se = int(argv[1]) if len(argv) > 1 else 1000000
    reps = int(argv[2]) if len(argv) > 2 else 5
    os.environ.setdefault("CSA_FORCE_EXCHANGE", "1")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        print(json.dumps({"note": "1-rank RCCL group on one GPU, CSA_FORCE_EXCHANGE=%s; call_ms = host wall time of "
                                  "the call, the other fields its timings stages" % os.environ["CSA_FORCE_EXCHANGE"],
                          "config3_share": run_multiplicity("example_large_200", 200, s3, reps),
                          "sf_e_110": run_multiplicity("sf_e_110", 110, se, reps)}), flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    if "--multiplicity" in sys.argv[1:]:
        main_multiplicity([a for a in sys.argv[1:] if a != "--multiplicity"])
        sys.exit(0)
    import torch
    import torch.distributed as dist
    s3 = int(sys.argv[1]) if len(sys.argv) > 1 else 1250000
    s5 = int(sys.argv[2]) if len(sys.argv) > 2 else 12500000
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    os.environ.setdefault("CSA_FORCE_EXCHANGE", "1")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        res = {"note": "legacy_probabilities_distributed under a 1-rank RCCL group on one MI355X, the n-th call "
                       "(cached encoding / pipeline / exchange); call_ms = host wall time of the call; "
                       "found_rows_redraw_ms = found.rows() after the last call (re-draw of [0, S) + dedupe)",
               "force_exchange": os.environ.get("CSA_FORCE_EXCHANGE"),
               "config3_share": run("example_large_200", 200, s3, calls,
                                    [("no_panels", {"keep_panels": False}), ("keep_panels", {})]),
               "config5_share": run("synthetic8192_200", 200, s5, calls,
                                    [("no_panels", {"keep_panels": False}), ("keep_panels", {})])}
        print(json.dumps(res), flush=True)
    finally:
        dist.destroy_process_group()
