"""Measure the SURVEY.md section 8(f) rows on one GPU; prints one JSON object.

  f1  xmin._get_panel_not_in_portfolio_if_possible (xmin.py:464-474): device call latency vs
      the same legacy_find calls in the C oracle (1 core)
  f2  cache.run_legacy_or_retrieve npz write / read at sf_e, 10^6 panels
  f3  pair_histogram_kernel (sorted pair-probability curve, analysis.py:339-342): kernel time and
      HBM GB/s over the upper triangle at sf_e (n=1727) and n=8192, vs numpy sort of the triangle
  f3b analysis.portfolio_probabilities (the LEXIMIN / XMIN analysis side, analysis.py:194-228) at
      sf_e with an XMIN-sized portfolio (5n panels): end to end, upload and triangle read included,
      vs the host PairHistogram.add_portfolio_of_panels_to_histogram (median of 5, one process);
      and portfolio_pairs_kernel alone, there and at n = 8192, P = 5n
  f3c group_hist_kernel (per-panel group composition, csrc/composition.inc) alone at sf_e (G = 377:
      31 features + the 346 intersections of tests/golden/sf_e_110_intersections.csv) and at
      synthetic8192 (G = its 40 features), 10^6 panels each, ms per launch next to the draw of the
      same panels in the same run; analysis.legacy_composition against legacy_probabilities at sf_e
      (median of 5, alternating, one process): the added ms; and the host numpy implementation over
      10^5 of the same panels, for scale (its table checked equal to the device's over them)

  f3d whist_count_kernel + whist_sum_kernel (weighted group composition of a portfolio,
      csrc/portfolio_composition.inc) alone, events, best of 3 windows after a warm-up: sf_e with
      P = 5n = 8635 drawn panels and G = 377, and synthetic8192 with P = 5n = 40 960 and its 40 features;
      in the same run stats.group_whist_host on the same input (its table checked bit-equal to the
      device's) and portfolio_pairs_kernel over the same portfolio, the yardstick to report against

    python tools/bench_rows.py [--panels 1000000] [--rows f1,f2,f3,f3b,f3c,f3d]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "citizensassemblies-replication_amd"
INST = os.path.join(REPO, "tests", "golden", "instances")


def paths(name):
    return os.path.join(INST, name, "categories.csv"), os.path.join(INST, name, "respondents.csv")


def portfolio_weights(P):
    """The goldens' weights (tools/make_portfolio_goldens.py): 12 binades, a 0.0, a 1e-13, sum 1."""
    rs = np.random.RandomState(7)
    w = rs.uniform(size=P) * 2.0 ** -rs.randint(0, 13, size=P).astype(np.float64)
    rest = np.ones(P, bool)
    rest[[P // 3, (2 * P) // 3]] = False
    w[rest] *= (1.0 - 1e-13) / w[rest].sum()
    w[P // 3], w[(2 * P) // 3] = 0.0, 1e-13
    return [float(x) for x in w]


def portfolio_kernel_ms(A, N, torch, rows, weights, n, reps=3):
    """portfolio_pairs_kernel alone (XT and weights already on the device), ms per launch."""
    L = N.lib()
    P = len(weights)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    d_rows = torch.from_numpy(rows.view(np.int64).reshape(-1)).cuda()
    w = torch.from_numpy(np.asarray(weights, np.float64)).cuda()
    xt = torch.empty(((P + 63) // 64) * L.csa_xt_pad(n), dtype=torch.int64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    N.check(L.csa_transpose_count_async(N.ptr(d_rows), P, n, N.ptr(xt), N.ptr(cnt), sp))
    tri = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device="cuda")
    al = torch.empty(n, dtype=torch.float64, device="cuda")
    call = lambda: N.check(L.csa_portfolio_pairs_async(N.ptr(xt), P, n, N.ptr(w), N.ptr(tri), N.ptr(al), 0, sp))
    call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call()
    e1.record(st)
    torch.cuda.synchronize()
    return {"kernel_ms": e0.elapsed_time(e1) / reps}


def portfolio_row(P_, torch):
    A = importlib.import_module(PKG + ".analysis")
    N = importlib.import_module(PKG + "._native")
    inst = P_.read_instance(*paths("sf_e_110"), 110)
    n = len(inst.agents)
    P = 5 * n
    P_.seed(5)
    portfolio = [frozenset(p) for p in A.legacy_find_batch(inst.categories, inst.agents, 110, P)]
    weights = portfolio_weights(P)
    pos = {a: q for q, a in enumerate(inst.agents)}
    as_positions = [sorted(pos[a] for a in p) for p in portfolio]

    def device_call():
        alloc, panels, hist = A.portfolio_probabilities(inst, portfolio, weights)
        return hist.upper()

    def host_call():
        h = A.PairHistogram(n)
        h.add_portfolio_of_panels_to_histogram(as_positions, weights)
        return h.upper()

    def median5(fn):
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t)
        return sorted(ts)[2], r
    device_call()                                   # warm-up: library load, encode, allocator
    dev_s, dev_u = median5(device_call)
    host_s, host_u = median5(host_call)
    row = {"instance": "sf_e_110", "n": n, "panels": P,
           "device_end_to_end_ms": dev_s * 1e3, "host_method_ms": host_s * 1e3,
           "bit_equal": bool(np.array_equal(dev_u.view(np.uint64), host_u.view(np.uint64))),
           "note": "device: pack + upload + transpose + kernel + alloc read + panel set + triangle read; "
                   "host: add_portfolio_of_panels_to_histogram alone (no alloc, no set)"}
    row["kernel_sf_e"] = portfolio_kernel_ms(A, N, torch, A._pack_positions(as_positions, n), weights, n)
    n2, k2 = 8192, 200
    P2 = 5 * n2
    rs = np.random.RandomState(11)     # Bernoulli(k / n) members: LEGACY's density without an instance's quotas
    rows2 = np.concatenate([np.packbits(rs.rand(min(2048, P2 - o), n2) < k2 / n2, axis=1, bitorder="little")
                            for o in range(0, P2, 2048)]).view("<u8").reshape(P2, n2 // 64)
    row["kernel_n8192"] = dict(n=n2, panels=P2, density=k2 / n2, **portfolio_kernel_ms(
        A, N, torch, rows2, portfolio_weights(P2), n2))
    return row


def events_ms(torch, st, fn, reps):
    """fn() enqueued reps times on stream st between two events, after one warm-up call: ms per call."""
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def composition_kernel(P_, torch, name, k, S, groups_of, host_panels=0):
    """Draw S panels of the instance once, then time the draw and group_hist_kernel over them."""
    N = importlib.import_module(PKG + "._native")
    St = importlib.import_module(PKG + ".stats")
    Dv = importlib.import_module(PKG + ".device")
    inst = P_.read_instance(*paths(name), k)
    enc = P_.encode(inst.categories, inst.agents)
    groups = groups_of(inst)
    G, W, bins = len(groups), enc.W, k + 1
    pipe = Dv.DevicePipeline(enc, k, S, want_pairs=False, want_unique=False)
    st = pipe.stream
    draw_ms = events_ms(torch, st, lambda: pipe.draw(0, 0, S), 3)
    pipe.check_status()
    d_masks = torch.from_numpy(groups.masks.view(np.int64).reshape(-1)).cuda()
    hist = torch.zeros(G * bins, dtype=torch.int64, device="cuda")
    kernel_ms = events_ms(torch, st, lambda: St.group_hist_device(pipe.panels, S, W, d_masks, G, bins, hist,
                                                                    pipe.status, st), 5)
    pipe.check_status()
    table = hist.cpu().numpy().reshape(G, bins)
    row = {"instance": name, "n": enc.n, "W": W, "k": k, "groups": G, "bins": bins, "panels": S,
           "draw_kernel": pipe.draw_kernel_name(), "draw_ms": draw_ms, "group_hist_kernel_ms": kernel_ms,
           "rows_sum_to_launches_x_panels": bool(np.all(table.sum(axis=1) == 6 * S))}
    if host_panels:
        m = min(S, host_panels)
        head = pipe.panels[:m * W].cpu().numpy().view(np.uint64).reshape(m, W)
        t = time.perf_counter()
        want = St.group_hist_host(groups.masks, head, bins)
        row["host_numpy_panels"], row["host_numpy_ms"] = m, (time.perf_counter() - t) * 1e3
        hist.zero_()
        St.group_hist_device(pipe.panels, m, W, d_masks, G, bins, hist, pipe.status, st)
        pipe.check_status()
        row["device_equals_host_over_them"] = bool(np.array_equal(hist.cpu().numpy().reshape(G, bins), want))
    return row


def composition_row(P_, torch, S):
    A = importlib.import_module(PKG + ".analysis")
    St = importlib.import_module(PKG + ".stats")
    fixture = os.path.join(REPO, "tests", "golden", "sf_e_110_intersections.csv")
    both = lambda inst: St.feature_groups(inst) + St.intersection_groups(inst, fixture)
    row = {"kernel_sf_e": composition_kernel(P_, torch, "sf_e_110", 110, S, both, host_panels=10 ** 5),
           "kernel_synthetic8192": composition_kernel(P_, torch, "synthetic8192_200", 200, S, St.feature_groups),
           "estimate": "derived before the kernel existed, VALU-bound at sf_e: about 1 ms per 10^6 panels "
                       "(4W + 4 wave instructions per panel and 64-group slab, 6 slabs)"}
    inst = P_.read_instance(*paths("sf_e_110"), 110)
    groups = both(inst)
    calls = {"legacy_probabilities": lambda: A.legacy_probabilities(inst, S, 1, keep_panels=False),
             "legacy_composition": lambda: A.legacy_composition(inst, S, 1, groups, keep_panels=False)}
    times = {name: [] for name in calls}
    for name, fn in calls.items():                     # warm-up: encode, pipeline buffers, allocator
        fn()
    for _ in range(5):                                  # alternating, so both see the same machine
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t) * 1e3)
    med = {name: sorted(ts)[2] for name, ts in times.items()}
    row["api_sf_e"] = {"panels": S, "groups": len(groups), "median_of": 5,
                       "legacy_probabilities_ms": med["legacy_probabilities"],
                       "legacy_composition_ms": med["legacy_composition"],
                       "added_ms": med["legacy_composition"] - med["legacy_probabilities"],
                       "all_ms": times}
    return row


def best_of(torch, st, fn, windows=3, reps=5):
    """fn() enqueued reps times between two events, `windows` times after one warm-up call: the best
    window's ms per call, and all of them."""
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


def weighted_composition_kernel(P_, torch, name, k, groups_of):
    """Draw P = 5n panels of the instance as the portfolio, then time csa_group_whist_async (both
    kernels) over them, the host implementation, and portfolio_pairs_kernel over the same portfolio."""
    A = importlib.import_module(PKG + ".analysis")
    N = importlib.import_module(PKG + "._native")
    St = importlib.import_module(PKG + ".stats")
    Dv = importlib.import_module(PKG + ".device")
    inst = P_.read_instance(*paths(name), k)
    enc = P_.encode(inst.categories, inst.agents)
    groups = groups_of(inst)
    n, G, W, bins = enc.n, len(groups), enc.W, k + 1
    P = 5 * n
    pipe = Dv.DevicePipeline(enc, k, P, want_pairs=False, want_unique=False)
    st = pipe.stream
    pipe.draw(0, 0, P)
    pipe.check_status()
    weights = np.asarray(portfolio_weights(P), np.float64)
    with torch.cuda.stream(st):
        d_w = torch.from_numpy(weights).cuda()
        d_masks = torch.from_numpy(groups.masks.view(np.int64).reshape(-1)).cuda()
        hist = torch.empty(G * bins, dtype=torch.float64, device="cuda")
        best, all_ms = best_of(torch, st, lambda: St.group_whist_device(pipe.panels, P, W, d_w, d_masks, G, bins, hist,
                                                                         pipe.status, st))
    pipe.check_status()
    table = hist.cpu().numpy().reshape(G, bins)
    rows = pipe.panels[:P * W].cpu().numpy().view(np.uint64).reshape(P, W)
    t = time.perf_counter()
    want = St.group_whist_host(groups.masks, rows, weights, bins)
    host_ms = (time.perf_counter() - t) * 1e3
    pairs_best, pairs_all = None, []
    for _ in range(3):                                   # the same best-of-3 for the yardstick
        pairs_all.append(portfolio_kernel_ms(A, N, torch, rows, weights, n, reps=5)["kernel_ms"])
    pairs_best = min(pairs_all)
    return {"instance": name, "n": n, "W": W, "k": k, "groups": G, "bins": bins, "panels": P,
            "group_whist_ms": best, "group_whist_windows_ms": all_ms,
            "scratch_bytes": int(N.lib().csa_group_whist_scratch_bytes(P, G)),
            "group_whist_host_ms": host_ms,
            "device_bit_equal_to_host": bool(np.array_equal(table.view(np.uint64), want.view(np.uint64))),
            "portfolio_pairs_kernel_ms": pairs_best, "portfolio_pairs_windows_ms": pairs_all,
            "composition_over_pairs": best / pairs_best}


def weighted_composition_row(P_, torch):
    St = importlib.import_module(PKG + ".stats")
    fixture = os.path.join(REPO, "tests", "golden", "sf_e_110_intersections.csv")
    both = lambda inst: St.feature_groups(inst) + St.intersection_groups(inst, fixture)
    return {"kernel_sf_e": weighted_composition_kernel(P_, torch, "sf_e_110", 110, both),
            "kernel_synthetic8192": weighted_composition_kernel(P_, torch, "synthetic8192_200", 200, St.feature_groups),
            "note": "group_whist_ms: whist_count_kernel + whist_sum_kernel per csa_group_whist_async call, events, "
                    "best of 3 windows of 5 calls after a warm-up call; the scratch is allocated per call from "
                    "torch's caching allocator (a pool hit after the warm-up)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--panels", type=int, default=10 ** 6)
    ap.add_argument("--rows", default="f1,f2,f3,f3b", help="comma-separated rows to measure")
    args = ap.parse_args()
    rows = set(args.rows.split(","))
    import torch
    P = importlib.import_module(PKG)
    X = importlib.import_module(PKG + ".xmin")
    Cc = importlib.import_module(PKG + ".cache")
    St = importlib.import_module(PKG + ".stats")
    Dv = importlib.import_module(PKG + ".device")
    N = importlib.import_module(PKG + "._native")
    from oracle import coracle
    from oracle.legacy_oracle import read_instance as oread
    out = {}
    if "f3b" in rows:
        out["f3b_portfolio"] = portfolio_row(P, torch)
    if "f3c" in rows:
        out["f3c_composition"] = composition_row(P, torch, args.panels)
    if "f3d" in rows:
        out["f3d_weighted_composition"] = weighted_composition_row(P, torch)
    if not rows & {"f1", "f2", "f3"}:
        print(json.dumps(out))
        return

    # ---- f1 -------------------------------------------------------------------------------
    inst = P.read_instance(*paths("sf_e_110"), 110)
    enc = P.encode(inst.categories, inst.agents)
    o = oread(*paths("sf_e_110"), 110)
    _, head, _, _ = coracle.draw(o, 110, 0, 0, 40)
    portfolio = [frozenset(enc.agent_ids[p] for p in P.instance.unpack_panel(r, enc.n)) for r in head]
    X._get_panel_not_in_portfolio_if_possible(inst.categories, inst.agents, 110, portfolio)   # warm-up
    reps = 20
    t = time.perf_counter()
    for _ in range(reps):
        P.seed(0)
        X._get_panel_not_in_portfolio_if_possible(inst.categories, inst.agents, 110, portfolio)
    dev_s = (time.perf_counter() - t) / reps
    t = time.perf_counter()
    coracle.draw(o, 110, 0, 0, 41, threads=1)
    cpu_s = time.perf_counter() - t
    out["f1_xmin_caller"] = {"instance": "sf_e_110", "portfolio": len(portfolio), "first_non_member": 40,
                             "device_ms_per_call": dev_s * 1e3, "c_oracle_1core_ms_same_41_draws": cpu_s * 1e3,
                             "reference_python_ms_est": 41 * 1e3 / 30.2,
                             "note": "device call includes encode, portfolio upload + hash table, chunked draws"}

    # ---- f2 -------------------------------------------------------------------------------
    S = args.panels
    with tempfile.TemporaryDirectory() as d:
        t = time.perf_counter()
        Cc.run_legacy_or_retrieve("sf_e_110", inst, False, directory=d, iterations=S, keep_panels=False)
        first = time.perf_counter() - t
        f = Cc.legacy_cache_path("sf_e_110", 110, False, d)
        size = os.path.getsize(f)
        t = time.perf_counter()
        _, _, hist = Cc.run_legacy_or_retrieve("sf_e_110", inst, False, directory=d, iterations=S, keep_panels=False)
        second = time.perf_counter() - t
    out["f2_cache"] = {"instance": "sf_e_110", "panels": S, "compute_and_write_s": first, "read_s": second,
                       "npz_bytes": size, "pair_entries": enc.n * (enc.n - 1) // 2}

    # ---- f3 -------------------------------------------------------------------------------
    f3 = {}
    for name, k, S3 in [("sf_e_110", 110, S), ("synthetic8192_200", 200, 20000)]:
        inst3 = P.read_instance(*paths(name), k)
        enc3 = P.encode(inst3.categories, inst3.agents)
        pipe = Dv.DevicePipeline(enc3, k, S3, want_unique=False)
        pipe.reset()
        pipe.run(0, 0, S3)
        pipe.check_status()
        n = enc3.n
        n_bins = int(pipe.counts.max().item()) + 1
        hist = torch.empty(n_bins, dtype=torch.int64, device="cuda")
        over = torch.empty(1, dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream()
        for _ in range(3):
            N.check(N.lib().csa_pair_histogram_async(N.ptr(pipe.pairs), n, N.ptr(hist), n_bins, N.ptr(over),
                                                     ctypes.c_void_p(st.cuda_stream)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        e0.record(st)
        for _ in range(reps):
            N.check(N.lib().csa_pair_histogram_async(N.ptr(pipe.pairs), n, N.ptr(hist), n_bins, N.ptr(over),
                                                     ctypes.c_void_p(st.cuda_stream)))
        e1.record(st)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        tri = n * (n - 1) // 2
        m = pipe.pairs.view(n, n).cpu().numpy()
        t = time.perf_counter()
        np.sort(m[np.triu_indices(n, 1)])
        np_s = time.perf_counter() - t
        f3[name] = {"n": n, "panels": S3, "bins": n_bins, "kernel_ms": ms, "bytes": tri * 8,
                    "hbm_GBps": tri * 8 / (ms * 1e-3) / 1e9, "numpy_sort_ms": np_s * 1e3,
                    "note": "kernel_ms includes the two memsets of the histogram"}
    out["f3_pair_histogram"] = f3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
