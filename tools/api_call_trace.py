"""The C-ABI calls behind each public entry point, in order (diagnostic, GPU box): _native._lib is swapped
for a proxy that logs every call as its name, its integer arguments, None / ptr for each pointer argument
and the stream as the ordinal of its first appearance in that section.  Two trees that print the same log
put the same work on the same streams in the same order, whatever their Python looks like.

Usage: python tools/api_call_trace.py [--golden DIR]     (DIR: a tests/golden, default this tree's)"""
import ctypes
import importlib
import json
import os
import socket
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
P = importlib.import_module("citizensassemblies-replication_amd")
N = importlib.import_module("citizensassemblies-replication_amd._native")
A = importlib.import_module("citizensassemblies-replication_amd.analysis")
D = importlib.import_module("citizensassemblies-replication_amd.distributed")
St = importlib.import_module("citizensassemblies-replication_amd.stats")

POINTERS = (ctypes.c_void_p, ctypes.c_char_p)
LOG, STREAMS = [], {}


def _address(arg):
    return arg.value if isinstance(arg, ctypes.c_void_p) else arg


def _takes_stream(name):
    return name.endswith("_async") or name == "csa_instance_draw_stats_reset"


class Proxy:
    """Stands in for the ctypes library: every function it hands out logs its call, then makes it."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        types = N.SIGNATURES[name][1]

        def call(*args):
            shown = []
            for i, (arg, tp) in enumerate(zip(args, types)):
                if tp not in POINTERS:
                    shown.append(repr((float if tp is ctypes.c_double else int)(getattr(arg, "value", arg))))
                elif i == len(types) - 1 and _takes_stream(name):
                    shown.append("stream%d" % STREAMS.setdefault(_address(arg), len(STREAMS)))
                else:
                    shown.append("None" if _address(arg) is None else "ptr")
            LOG.append("%s(%s)" % (name, ", ".join(shown)))
            return fn(*args)
        return call


def section(title, call):
    import torch
    LOG.clear()
    STREAMS.clear()
    call()
    torch.cuda.synchronize()
    print("== %s: %d calls" % (title, len(LOG)))
    for line in LOG:
        print("  " + line)


def main(golden):
    import torch
    import torch.distributed as dist

    def instance(name, k):
        d = os.path.join(golden, "instances", name)
        return P.read_instance(os.path.join(d, "categories.csv"), os.path.join(d, "respondents.csv"), k)

    N._lib = Proxy(N.lib())
    sf_e = instance("sf_e_110", 110)
    groups = St.feature_groups(sf_e)
    section("legacy_probabilities, one chunk", lambda: A.legacy_probabilities(sf_e, 3000, 5))
    section("legacy_probabilities, one chunk, again", lambda: A.legacy_probabilities(sf_e, 3000, 6))
    section("legacy_probabilities, three chunks", lambda: A.legacy_probabilities(sf_e, (2 << 20) + 1000, 5))
    section("legacy_composition", lambda: A.legacy_composition(sf_e, 3000, 5, groups))
    section("legacy_panel_distribution", lambda: A.legacy_panel_distribution(sf_e, 3000, 5))
    small = instance("example_small_20", 20)
    section("legacy_probabilities, rng=mt", lambda: A.legacy_probabilities(small, 500, 0, rng="mt"))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        for force in ("0", "1"):
            os.environ["CSA_FORCE_EXCHANGE"] = force
            section("legacy_probabilities_distributed, one rank, CSA_FORCE_EXCHANGE=%s" % force,
                    lambda: D.legacy_probabilities_distributed(sf_e, 3000, 5))
            section("legacy_probabilities_distributed with groups, one rank, CSA_FORCE_EXCHANGE=%s" % force,
                    lambda: D.legacy_probabilities_distributed(sf_e, 3000, 5, groups=groups))
    finally:
        os.environ.pop("CSA_FORCE_EXCHANGE", None)
        dist.destroy_process_group()
    import numpy as np
    with open(os.path.join(golden, "portfolio_sf_e_110.json")) as fh:
        g = json.load(fh)
    with np.load(os.path.join(golden, "portfolio_sf_e_110.npz"), allow_pickle=False) as z:
        g.update({key: z[key].tolist() for key in z.files})
    ids = list(sf_e.agents)
    portfolio = [frozenset(ids[p] for p in panel) for panel in g["portfolio"]]
    section("portfolio_composition", lambda: A.portfolio_composition(sf_e, portfolio, g["weights"], groups))


if __name__ == "__main__":
    main(sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--golden" else os.path.join(REPO, "tests", "golden"))
