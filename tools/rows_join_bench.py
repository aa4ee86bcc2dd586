"""Measure the join of two runs' sorted panel tables on one GPU; prints one JSON object and writes it to
profiles/rows_join/<--out>.

Per instance (sf_e_110 and the couples instance, --panels draws per run, seeds 0 and 1), over the two
``legacy_panel_distribution(...)[3].table()`` tables, all in one process:

  join_ms          csa_rows_join_async, events, best of 3 windows of 5 calls after a warm-up call, for
                   select 0 (the record alone: what compare_panel_distributions and the comparisons run),
                   4 (the intersection's rows) and 7 (the whole union with both multiplicity lists)
  merge_ms         csa_rows_merge_unique_async over the same two tables, timed the same way: the same record
                   and merge-path passes and a compaction of its own -- the yardstick
  join_host_ms     stats.rows_join_host (select 4) on host copies of the same tables, one call
  python_set_ms    set(a) & set(b) on the two runs' found_panels: decoding every row into a tuple of agent
                   ids, then the intersection, one call (--set-rows caps the rows decoded per side)

The device record is checked equal to the host mirror's, and the intersection's size to Python's.

    python tools/rows_join_bench.py [--panels 1000000] [--set-rows 0] [--out join_sf_e_couples.json]
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
INSTANCES = [("sf_e_110", 110), ("couples_panel_from_twenty_people_no_constraints_2", 2)]


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


def instance_row(P, torch, name, k, S, set_rows):
    A = importlib.import_module(PKG + ".analysis")
    St = importlib.import_module(PKG + ".stats")
    N = importlib.import_module(PKG + "._native")
    inst = P.read_instance(*paths(name), k)
    runs = [A.legacy_panel_distribution(inst, S, seed) for seed in (0, 1)]
    ta, tb = (run[3].table() for run in runs)
    dev = ta.rows.device
    st = torch.cuda.current_stream(dev)
    T = St.DeviceRowTables(dev, st)
    row = {"instance": name, "k": k, "W": ta.W, "panels_per_run": S, "distinct": [ta.cap, tb.cap]}
    scales = (runs[0][3].S, runs[1][3].S)
    for select in (0, 4, 7):
        best, windows = best_of(torch, st, lambda: T.join(ta, tb, select, scales))
        row["join_select%d_ms" % select], row["join_select%d_windows_ms" % select] = best, windows
    out = T.new_table(ta.cap + tb.cap, ta.W)
    best, windows = best_of(torch, st, lambda: T.merge(ta, tb, out))
    row["merge_ms"], row["merge_windows_ms"] = best, windows
    row["join_select7_over_merge"] = row["join_select7_ms"] / best
    row["scratch_bytes"] = {"join": int(N.lib().csa_rows_join_scratch_bytes(ta.cap, tb.cap, ta.W)),
                            "merge": int(N.lib().csa_rows_merge_scratch_bytes(ta.cap, tb.cap, ta.W))}
    j = T.join(ta, tb, 4, scales)
    record = [int(x) for x in j.record.cpu().numpy().view(np.uint64)]
    N.raise_status(T.status.cpu().numpy().view(np.uint32))
    host = [(t.rows.cpu().numpy().view(np.uint64), t.mult.cpu().numpy().view(np.uint32).astype(np.int64)) for t in (ta, tb)]
    t0 = time.perf_counter()
    want = St.rows_join_host(host[0], host[1], 4, scales)
    row["join_host_ms"] = (time.perf_counter() - t0) * 1e3
    row["record"], row["record_equals_host"] = record, record == want[4]
    row["intersection_rows_equal_host"] = bool(np.array_equal(
        j.rows[:record[1]].cpu().numpy().view(np.uint64), want[0]))
    c = St.PanelComparison(record, *scales)
    row["figures"] = {"jaccard": c.jaccard(), "mass_b_on_a": c.mass_b_on_a(), "coverage_a": runs[0][3].coverage(),
                      "overlap": c.overlap(), "cross_collision": c.cross_collision(),
                      "collision_probability_a": runs[0][3].collision_probability()}
    sets = []
    for run, (rows, _) in zip(runs, host):
        keep = rows[:set_rows] if set_rows else rows
        sets.append(A.PanelSet(len(keep), keep.copy(), run[1]._n, run[1]._ids))
    t0 = time.perf_counter()
    both = set(sets[0]) & set(sets[1])
    row["python_set_ms"] = (time.perf_counter() - t0) * 1e3
    row["python_set_rows_per_side"] = [len(s) for s in sets]
    if not set_rows:
        row["intersection_equals_python"] = len(both) == record[1]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panels", type=int, default=10 ** 6)
    ap.add_argument("--set-rows", type=int, default=0, help="rows per side decoded for set(a) & set(b); 0: all")
    ap.add_argument("--out", default="join_sf_e_couples.json")
    args = ap.parse_args()
    import torch
    P = importlib.import_module(PKG)
    out = {"device": torch.cuda.get_device_name(0),
           "method": "events around 5 enqueued calls, best of 3 windows after a warm-up call; scratch and outputs "
                     "from torch's caching allocator per call (pool hits after the warm-up)",
           "instances": [instance_row(P, torch, name, k, args.panels, args.set_rows) for name, k in INSTANCES]}
    line = json.dumps(out)
    os.makedirs(os.path.join(REPO, "profiles", "rows_join"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "rows_join", args.out), "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
