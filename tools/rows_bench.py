"""Cost of reading found_panels: ``found.rows()`` after a sharded call (one-rank RCCL group, the key exchange
forced on, so nothing is kept and the read re-draws the job) and after a one-GPU call (the panels kept on the
device), at the sizes DESIGN section 4 quotes, and over one synthetic duplicate-heavy batch of wide rows.
Each timed read is a fresh result's first ``rows()`` -- a result caches its rows -- bracketed by device
synchronises; the host's resident set is sampled every millisecond during the read and its rise over the
value before the read is reported (``host_rise_mb``).

``--root DIR`` imports the package from another checkout (the parent commit's, for A/B runs: alternate the two
commands); CSA_ROWS_HOST=1 forces this tree's host path.  Prints one JSON line.

Usage (GPU box): python tools/rows_bench.py [--root DIR] [--reps 3] [--only NAME[,NAME]]"""
import argparse
import importlib
import json
import os
import socket
import sys
import threading
import time

CASES = [  # name, instance, k, panels, sharded
    ("config3_share_sharded", "example_large_200", 200, 1250000, True),
    ("sf_e_1e6_sharded", "sf_e_110", 110, 1000000, True),
    ("sf_e_1e6_kept", "sf_e_110", 110, 1000000, False),
    ("couples_1e4_kept", "couples_panel_from_twenty_people_no_constraints_2", 2, 10000, False),
    ("example_small_1e4_kept", "example_small_20", 20, 10000, False),
    ("example_large_1e4_kept", "example_large_200", 200, 10000, False),
    # no instance: 10^6 rows of 32 words drawn from a pool of 1000 rows, kept on the device -- wide rows with
    # ~1000 copies each, where equal word 0s send most compares of the sort through the rows themselves
    ("pool1000_1e6_w32_kept", None, 0, 1000000, False),
]


def _rss_mb():
    with open("/proc/self/statm") as fh:
        return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 2 ** 20


class RssPeak:
    def __enter__(self):
        self.base = self.peak = _rss_mb()
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def _run(self):
        while not self._stop.wait(0.001):
            self.peak = max(self.peak, _rss_mb())

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.peak = max(self.peak, _rss_mb())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    pkg = "citizensassemblies-replication_amd"
    P = importlib.import_module(pkg)
    A = importlib.import_module(pkg + ".analysis")
    D = importlib.import_module(pkg + ".distributed")
    import torch
    import torch.distributed as dist
    os.environ.setdefault("CSA_FORCE_EXCHANGE", "1")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    only = [s for s in args.only.split(",") if s]
    out = {"root": root, "rows_host": os.environ.get("CSA_ROWS_HOST"), "reps": args.reps}
    try:
        for name, instance, k, S, sharded in CASES:
            if only and name not in only:
                continue
            if instance is None:
                import numpy as np
                rng = np.random.default_rng(1)
                pool = rng.integers(0, 1 << 64, size=(1000, 32), dtype=np.uint64)
                batch = torch.from_numpy(pool[rng.integers(0, 1000, size=S)].view(np.int64).reshape(-1)).cuda()
                call = lambda: (None, A.PanelSet(1000, batch, 2048, list(range(2048))))
            else:
                d = os.path.join(root, "tests", "golden", "instances", instance)
                inst = P.read_instance(os.path.join(d, "categories.csv"), os.path.join(d, "respondents.csv"), k)
                call = (lambda: D.legacy_probabilities_distributed(inst, S, 0)) if sharded else \
                    (lambda: A.legacy_probabilities(inst, S, 0))
            call()[1].rows()                                   # untimed: code objects, cached pipeline, allocator
            ms, rise, distinct = [], [], None
            for _ in range(args.reps):
                found = call()[1]
                torch.cuda.synchronize()
                with RssPeak() as rss:
                    t = time.perf_counter()
                    rows = found.rows()
                    torch.cuda.synchronize()
                    ms.append(round((time.perf_counter() - t) * 1e3, 3))
                rise.append(round(rss.peak - rss.base, 1))
                assert len(rows) == len(found)
                distinct, W = len(rows), rows.shape[1]
                del rows, found
            out[name] = {"panels": S, "W": W, "distinct": distinct, "rows_ms": ms, "host_rise_mb": rise,
                         "all_panels_mb": round(S * W * 8 / 2 ** 20, 1),
                         "distinct_rows_mb": round(distinct * W * 8 / 2 ** 20, 1)}
            print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    finally:
        dist.destroy_process_group()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
