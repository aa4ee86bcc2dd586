"""Measure pricing over a run's table of distinct panels on one GPU; prints one JSON object and writes it to
profiles/rows_price/<--out>.

Per instance (sf_e_110 and example_large_200, --panels draws, seed 0), over
``legacy_panel_distribution(...)[3].table()``, all in one process:

  price_ms           csa_rows_price_async (score pass + best), events, best of 3 windows of 5 calls after a
                     warm-up call; with and without the per-row scores written
  clone_ms           a device-to-device copy of the same table's rows (``clone``), timed the same way: it moves
                     twice the bytes the pass reads, so a pass slower than the copy is not bandwidth-bound
  mw_round_ms        csa_rows_mw_cover_async at 3 n rounds (--rounds overrides), one call between two events,
                     over the rounds; mw_round_minus_price_ms = the round kernel plus two launches
  first_holder_ms    csa_rows_first_holder_async, as price_ms
  mirror_ms          stats.rows_price_host on the first --mirror-rows rows on the host, one call (the bool
                     member matrix of the whole table would not fit); its best is checked equal to the device's
                     over the same rows

and once, --price-draws fresh example_large_200 draws through ``legacy_price`` (host clock around the call,
which ends in its host wait), second of two calls, beside the figure for the draw alone: ``bench.py --config
example_large_200 --job-panels <the same>``, to be run separately.

    python tools/rows_price_bench.py [--panels 1000000] [--price-draws 10000000] [--out price_sf_e_large.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "citizensassemblies-replication_amd"
INST = os.path.join(REPO, "tests", "golden", "instances")
INSTANCES = [("sf_e_110", 110), ("example_large_200", 200)]


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


def instance_row(P, torch, name, k, S, rounds, mirror_rows):
    A = importlib.import_module(PKG + ".analysis")
    St = importlib.import_module(PKG + ".stats")
    inst = P.read_instance(*paths(name), k)
    dist = A.legacy_panel_distribution(inst, S, 0)[3]
    t = dist.table()
    n = dist._n
    dev = t.rows.device
    st = torch.cuda.current_stream(dev)
    T = St.DeviceRowTables(dev, st)
    rng = np.random.default_rng(0)
    w = rng.uniform(0.1, 1.0, n)
    d_w = torch.from_numpy(w).to(dev)
    row = {"instance": name, "k": k, "n": n, "W": t.W, "panels": S, "distinct": t.cap, "table_bytes": t.cap * t.W * 8}
    for key, scores in (("price_ms", False), ("price_scores_ms", True)):
        best, windows = best_of(torch, st, lambda: T.price(t, n, d_w, scores=scores))
        row[key], row[key[:-3] + "_windows_ms"] = best, windows
    best, windows = best_of(torch, st, lambda: t.rows.clone())
    row["clone_ms"], row["clone_windows_ms"] = best, windows
    row["price_over_clone"] = row["price_ms"] / best
    row["price_read_GBps"] = row["table_bytes"] / row["price_ms"] / 1e6
    row["clone_moved_GBps"] = 2 * row["table_bytes"] / best / 1e6
    best, windows = best_of(torch, st, lambda: T.first_holder(t, n))
    row["first_holder_ms"], row["first_holder_windows_ms"] = best, windows
    R = 3 * n if rounds is None else rounds
    times = []
    for _ in range(2):
        ones = torch.ones(n, dtype=torch.float64, device=dev)
        chosen = torch.zeros(t.cap, dtype=torch.uint8, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        picks, _ = T.mw_cover(t, n, R, ones, chosen)
        e1.record(st)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    row["mw_rounds"], row["mw_total_ms"] = R, times
    row["mw_round_ms"] = min(times) / max(R, 1)
    row["mw_round_minus_price_ms"] = row["mw_round_ms"] - row["price_ms"]
    row["mw_distinct_picks"] = int(torch.unique(picks).numel())
    # the numpy mirror on a prefix of the table, and the device's answer over the same rows
    m = min(mirror_rows, t.cap)
    host_rows = t.rows[:m].cpu().numpy().view(np.uint64)
    t0 = time.perf_counter()
    at, value, _ = St.rows_price_host(host_rows, w)
    row["mirror_rows"], row["mirror_ms"] = m, (time.perf_counter() - t0) * 1e3
    prefix = St.RowTable(t.rows, None, None, torch.full((1,), m, dtype=torch.int64, device=dev), t.cap, t.W)
    got = T.price(prefix, n, d_w)[0].cpu().numpy()
    row["device_equals_mirror"] = bool(int(got[0]) == at and got[1:2].view(np.float64)[0] == value)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panels", type=int, default=10 ** 6)
    ap.add_argument("--rounds", type=int, default=None, help="multiplicative-weights rounds (default 3 n)")
    ap.add_argument("--mirror-rows", type=int, default=100000)
    ap.add_argument("--price-draws", type=int, default=10 ** 7)
    ap.add_argument("--out", default="price_sf_e_large.json")
    args = ap.parse_args()
    import torch
    P = importlib.import_module(PKG)
    A = importlib.import_module(PKG + ".analysis")
    out = {"device": torch.cuda.get_device_name(0),
           "method": "events around 5 enqueued calls, best of 3 windows after a warm-up call; scratch and outputs "
                     "from torch's caching allocator per call (pool hits after the warm-up)",
           "instances": [instance_row(P, torch, name, k, args.panels, args.rounds, args.mirror_rows)
                         for name, k in INSTANCES]}
    if args.price_draws:
        name, k = INSTANCES[1]
        inst = P.read_instance(*paths(name), k)
        n = len(inst.agents)
        w = np.random.default_rng(1).uniform(0.1, 1.0, n).tolist()
        secs = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            panel, value, at = A.legacy_price(inst, w, args.price_draws, 0)
            secs.append(time.perf_counter() - t0)
        out["legacy_price"] = {"instance": name, "draws": args.price_draws, "seconds": secs,
                               "panels_per_s": args.price_draws / min(secs), "value": value, "index": at,
                               "floor": "bench.py --config %s --job-panels %d (the draw alone)" % (name, args.price_draws)}
    line = json.dumps(out)
    os.makedirs(os.path.join(REPO, "profiles", "rows_price"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "rows_price", args.out), "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
