"""Measure the maximin lottery over a run's table of distinct panels on one GPU; prints one JSON object and
writes it to <--out-dir>/<--out> (default profiles/rows_maximin/).

Per instance (sf_e_110 and example_large_200, --panels draws, seed 0), over
``legacy_panel_distribution(...)[3].table()``, all in one process:

  start_ms             csa_rows_maximin_async with CSA_MAXIMIN_START and no rounds (first holders, one score pass,
                       the bound), events, best of 3 calls after a warm-up call
  round_ms[resync]     one call of --rounds rounds (default 3 n) from a start, between two events, minus start_ms,
                       over the rounds; resync = 16, 1 and 64 in turn, --windows times round the three (so the
                       versions alternate); every window is listed.  resync = 1 sends every round through the
                       unchanged rp_score_kernel: the baseline of the same session
  update_round_ms      a round that is not fresh (rm_pick_kernel + rm_update_kernel, two launches): the resync = 64
                       call's time minus its fresh rounds at the resync = 1 figure, over its other rounds
  price_ms             csa_rows_price_async alone (rp_score_kernel + rp_best_kernel, two launches), with and
                       without the scores written; best of 3 windows of 5 calls
  clone_ms             a device-to-device copy of the table's rows, timed the same way (it moves twice the bytes a
                       pass reads)
  lower, upper,        the bounds and the number of distinct panels picked after --rounds rounds at resync = 16
  distinct_picks       (and at resync = 1, for the bounds' dependence on it)

``--trace-rounds R``: only the sf_e_110 table, one call of R rounds at resync 16 and five price calls, no timing --
the workload for a ``rocprofv3 --kernel-trace --stats`` run of its own, which gives each kernel's time.

    python tools/rows_maximin_bench.py [--panels 1000000] [--rounds R] [--out maximin_sf_e_large.json]
"""
import argparse
import importlib
import json
import os
import sys
from fractions import Fraction

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "citizensassemblies-replication_amd"
INST = os.path.join(REPO, "tests", "golden", "instances")
INSTANCES = [("sf_e_110", 110), ("example_large_200", 200)]
RESYNCS = [16, 1, 64]
SHRINK = 0.8


def paths(name):
    return os.path.join(INST, name, "categories.csv"), os.path.join(INST, name, "respondents.csv")


def best_of(torch, st, fn, windows=3, reps=5):
    """fn() enqueued reps times between two events, `windows` times after one warm-up call: the best window's ms
    per call, and all of them."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return min(ms), ms


def fresh_rounds(rounds, resync):
    """How many of a call's rounds are fresh: every resync-th and the last."""
    return rounds // resync + (1 if rounds % resync else 0)


def table_of(P, name, k, S):
    A = importlib.import_module(PKG + ".analysis")
    dist = A.legacy_panel_distribution(P.read_instance(*paths(name), k), S, 0)[3]
    return dist.table(), dist._n


def bounds(St, torch, t, picks, buffers, rounds):
    state = St.maximin_buffers_host(buffers, t.cap)
    held = state.weights != 0.0
    lower = min(Fraction(int(c), rounds) for c in state.cover[held])
    return {"lower": float(lower), "lower_fraction": "%d/%d" % (lower.numerator, lower.denominator),
            "upper": state.upper, "covered_agents": int(held.sum()), "distinct_picks": int(torch.unique(picks).numel()),
            "rounds_done": state.rounds}


def instance_row(P, torch, name, k, S, rounds, windows):
    St = importlib.import_module(PKG + ".stats")
    t, n = table_of(P, name, k, S)
    dev = t.rows.device
    st = torch.cuda.current_stream(dev)
    T = St.DeviceRowTables(dev, st)
    R = 3 * n if rounds is None else rounds
    row = {"instance": name, "k": k, "n": n, "W": t.W, "panels": S, "distinct": t.cap, "table_bytes": t.cap * t.W * 8,
           "rounds": R, "shrink": SHRINK}
    d_w = torch.rand(n, dtype=torch.float64, device=dev) * 0.9 + 0.1
    for key, scores in (("price_ms", False), ("price_scores_ms", True)):
        best, w = best_of(torch, st, lambda: T.price(t, n, d_w, scores=scores))
        row[key], row[key[:-3] + "_windows_ms"] = best, w
    best, w = best_of(torch, st, lambda: t.rows.clone())
    row["clone_ms"], row["clone_windows_ms"] = best, w
    best, w = best_of(torch, st, lambda: T.maximin(t, n, 0, SHRINK, 16), reps=1)
    row["start_ms"], row["start_windows_ms"] = best, w
    T.maximin(t, n, 70, SHRINK, 16)                      # every kernel of a round loaded before the windows
    torch.cuda.synchronize()
    totals = {r: [] for r in RESYNCS}
    for _ in range(windows):
        for r in RESYNCS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            picks, buffers = T.maximin(t, n, R, SHRINK, r)
            e1.record(st)
            torch.cuda.synchronize()
            totals[r].append(e0.elapsed_time(e1))
            if r != 64 and "bounds_resync_%d" % r not in row:
                row["bounds_resync_%d" % r] = bounds(St, torch, t, picks, buffers, R)
    per_round = lambda ms: (ms - row["start_ms"]) / max(R, 1)
    row["total_windows_ms"] = {str(r): totals[r] for r in RESYNCS}
    row["round_ms"] = {str(r): per_round(min(totals[r])) for r in RESYNCS}
    row["round_windows_ms"] = {str(r): [per_round(x) for x in totals[r]] for r in RESYNCS}
    fresh = row["round_ms"]["1"]
    f64 = fresh_rounds(R, 64)
    row["update_round_ms"] = (min(totals[64]) - row["start_ms"] - f64 * fresh) / max(R - f64, 1)
    row["resync16_over_resync1"] = row["round_ms"]["16"] / fresh
    row["update_round_over_price"] = row["update_round_ms"] / row["price_scores_ms"]
    row["update_round_over_clone"] = row["update_round_ms"] / row["clone_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panels", type=int, default=10 ** 6)
    ap.add_argument("--rounds", type=int, default=None, help="rounds per call (default 3 n)")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--trace-rounds", type=int, default=0)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "rows_maximin"))
    ap.add_argument("--out", default="maximin_sf_e_large.json")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rows_maximin_bench needs a GPU")
    P = importlib.import_module(PKG)
    if args.trace_rounds:
        St = importlib.import_module(PKG + ".stats")
        t, n = table_of(P, *INSTANCES[0], args.panels)
        T = St.DeviceRowTables(t.rows.device, torch.cuda.current_stream(t.rows.device))
        d_w = torch.rand(n, dtype=torch.float64, device=t.rows.device) * 0.9 + 0.1
        T.maximin(t, n, args.trace_rounds, SHRINK, 16)
        for _ in range(5):
            T.price(t, n, d_w, scores=True)
        torch.cuda.synchronize()
        print(json.dumps({"traced": INSTANCES[0][0], "distinct": t.cap, "rounds": args.trace_rounds}))
        return
    out = {"device": torch.cuda.get_device_name(0),
           "method": "events around one call of `rounds` rounds, start_ms taken off, over the rounds; resync 16, 1, 64 "
                     "in turn, `windows` times; price and clone: events around 5 enqueued calls, best of 3 windows; "
                     "scratch and state from torch's caching allocator per call (pool hits after the warm-up)",
           "instances": [instance_row(P, torch, name, k, args.panels, args.rounds, args.windows) for name, k in INSTANCES]}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.out), "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
