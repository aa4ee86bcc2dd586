"""Measure the Nash-welfare lottery over a run's table of distinct panels on one GPU; prints one JSON object and
writes it to <--out-dir>/<--out> (default profiles/rows_nash/bench.json).

Per table (sf_e_110, seed 0, --panels draws and 5 n = 8635 draws), over
``legacy_panel_distribution(...)[3].table()``, all in one process, every figure --runs times (default five) with
the best, the median and all of them listed:

  marginals_ms    csa_rows_marginals_async alone (rn_marginal_kernel + rn_finish_kernel, two launches) under the
                  run's own lottery p = mult / S, events around 5 enqueued calls
  price_ms        csa_rows_price_async with the scores written (the unchanged rp_score_kernel + rp_best_kernel, two
                  launches) over the same table, timed the same way: the yardstick of the marginal pass
  clone_ms        a device-to-device copy of the table's rows, timed the same way (it moves twice the bytes a pass
                  reads)
  start_ms        csa_rows_nash_async with CSA_NASH_START and no rounds (start, first holders, one pass)
  round_ms        one call of --rounds rounds (default 200) from a start between two events, minus start_ms, over
                  the rounds: step, marginal, finish, score, bound -- five launches
  rounds_ms       that whole call (the start included)
  nash_ms         PanelDistribution.nash(--rounds) over the table already built: wall clock, its copy and wait
                  included
  legacy_nash_ms  analysis.legacy_nash end to end -- the draws, the table, the rounds, the result: wall clock

and, once, what the rounds reached: start_geometric_mean, geometric_mean, gap, upper, psum.

``--trace-rounds R``: only the large table, one call of R rounds and five pricing calls, no timing -- the workload
for a ``rocprofv3 --kernel-trace --stats`` run of its own, which gives each kernel's time.

    python tools/rows_nash_bench.py [--panels 1000000] [--rounds 200] [--runs 5]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "citizensassemblies-replication_amd"
INST = os.path.join(REPO, "tests", "golden", "instances")
NAME, K = "sf_e_110", 110


def paths(name):
    return os.path.join(INST, name, "categories.csv"), os.path.join(INST, name, "respondents.csv")


def windows(torch, st, fn, runs, reps=5):
    """fn() enqueued reps times between two events, ``runs`` times after one warm-up call: ms per call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def spread(ms):
    return {"best": min(ms), "median": statistics.median(ms), "all": list(ms)}


def wall(torch, fn, runs):
    ms, out = [], None
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def table_row(P, torch, S, rounds, runs):
    A = importlib.import_module(PKG + ".analysis")
    St = importlib.import_module(PKG + ".stats")
    inst = P.read_instance(*paths(NAME), K)
    dist = A.legacy_panel_distribution(inst, S, 0)[3]
    t, n = dist.table(), dist._n
    dev = t.rows.device
    st = torch.cuda.current_stream(dev)
    T = St.DeviceRowTables(dev, st)
    row = {"instance": NAME, "k": K, "n": n, "W": t.W, "panels": S, "distinct": t.cap, "table_bytes": t.cap * t.W * 8,
           "rounds": rounds}
    d_p = (t.mult.to(torch.int64) & 0xFFFFFFFF).to(torch.float64) / float(S)
    d_w = torch.rand(n, dtype=torch.float64, device=dev) * 0.9 + 0.1
    row["marginals_ms"] = spread(windows(torch, st, lambda: T.marginals(t, n, d_p), runs))
    row["price_ms"] = spread(windows(torch, st, lambda: T.price(t, n, d_w, scores=True), runs))
    row["clone_ms"] = spread(windows(torch, st, lambda: t.rows.clone(), runs))
    row["marginals_over_price"] = row["marginals_ms"]["best"] / row["price_ms"]["best"]
    start = windows(torch, st, lambda: T.nash(t, n, 0, t.mult, S), runs, reps=1)
    row["start_ms"] = spread(start)
    whole = windows(torch, st, lambda: T.nash(t, n, rounds, t.mult, S), runs, reps=1)
    row["rounds_ms"] = spread(whole)
    row["round_ms"] = spread([(x - min(start)) / max(rounds, 1) for x in whole])
    ms, result = wall(torch, lambda: dist.nash(rounds), runs)
    row["nash_ms"] = spread(ms)
    ms, _ = wall(torch, lambda: A.legacy_nash(inst, S, 0, rounds), runs)
    row["legacy_nash_ms"] = spread(ms)
    b = St.nash_buffers_host(T.nash(t, n, rounds, t.mult, S), t.cap)
    row["reached"] = {"start_geometric_mean": result.start_geometric_mean, "geometric_mean": result.geometric_mean,
                      "gap": result.gap, "upper": result.upper, "psum": b.psum, "rounds_done": b.rounds,
                      "covered_agents": len(result.covered_agents), "portfolio_rows": len(result.portfolio()[1])}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panels", type=int, default=10 ** 6)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace-rounds", type=int, default=0)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "rows_nash"))
    ap.add_argument("--out", default="bench.json")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rows_nash_bench needs a GPU")
    P = importlib.import_module(PKG)
    if args.trace_rounds:
        A = importlib.import_module(PKG + ".analysis")
        St = importlib.import_module(PKG + ".stats")
        dist = A.legacy_panel_distribution(P.read_instance(*paths(NAME), K), args.panels, 0)[3]
        t, n = dist.table(), dist._n
        T = St.DeviceRowTables(t.rows.device, torch.cuda.current_stream(t.rows.device))
        d_w = torch.rand(n, dtype=torch.float64, device=t.rows.device) * 0.9 + 0.1
        T.nash(t, n, args.trace_rounds, t.mult, args.panels)
        for _ in range(5):
            T.price(t, n, d_w, scores=True)
        torch.cuda.synchronize()
        print(json.dumps({"traced": NAME, "distinct": t.cap, "rounds": args.trace_rounds}))
        return
    out = {"device": torch.cuda.get_device_name(0),
           "method": "events around 5 enqueued calls (marginals, price, clone) or one call (start, rounds), `runs` "
                     "windows after a warm-up call; round_ms = (rounds_ms - best start_ms) / rounds; nash_ms and "
                     "legacy_nash_ms are wall clock around a synchronised call; scratch and state from torch's "
                     "caching allocator per call (pool hits after the warm-up)",
           "tables": [table_row(P, torch, S, args.rounds, args.runs) for S in (args.panels, 8635)]}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.out), "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
