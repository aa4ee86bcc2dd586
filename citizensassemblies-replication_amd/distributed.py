"""Multi-GPU LEGACY estimation: one process per GPU, torch.distributed over RCCL.

Sharding (DESIGN.md "Multi-GPU"): the global panel range [0, S) is cut into
contiguous per-rank ranges.  Every random draw is keyed by the GLOBAL panel
index (Philox counter = (step, attempt, panel)), so the union of the shards is
bit-identical to a single-GPU run for any world size; no data-path collective
is needed for the draw itself.

Exchange steps (the only collectives on the path), all
stream-ordered -- the host never waits for the device:
  * per-person counts  all_reduce(SUM) int64[n]
  * pair counts        all_reduce(SUM) of the upper triangle packed to int32
                       (csa_pairs_pack/unpack_async; int64[n*n] if a count may
                       reach 2^31)
  * distinct panels    each rank first reduces its panels to its exact LOCAL
                       distinct set (hash AND bitmask), then sends every one --
                       its 128-bit hash and W-word bitmask -- to its OWNER rank
                       (h1 % world; equal panels have equal hashes, so all copies
                       of a panel meet at one owner).  The segments per owner have
                       a FIXED capacity (binomial bound on a uniform hash, see
                       exchange_capacity), so the three all_to_alls (segment
                       counts, hashes, bitmasks) have equal splits and need no
                       host-side size negotiation (csa_exchange_pack_async).  The
                       owner counts the distinct panels among the valid entries
                       exactly (csa_unique_segments_async: bitmask comparison on a
                       hash match; analysis.py:171,186 is a set of sorted tuples),
                       then all_reduce(SUM).  A segment past its capacity is an
                       error in the status block, never a wrong count.
On CPU (gloo, tests) the same exchange runs on host tensors with numpy mirrors
of the two kernels; ``panel_hashes`` mirrors the device hash for that path.
"""
import ctypes
import os

import numpy as np

M64 = 0xFFFFFFFFFFFFFFFF


def world_size():
    try:
        import torch.distributed as dist
    except Exception:
        return 1
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return 1


def rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def shard_range(S, world, r):
    """Contiguous shard [begin, end) of S panels for rank r of world."""
    per, extra = divmod(int(S), int(world))
    begin = r * per + min(r, extra)
    return begin, begin + per + (1 if r < extra else 0)


def _fmix_a(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _fmix_b(z):
    z = z ^ (z >> np.uint64(33))
    z = z * np.uint64(0xFF51AFD7ED558CCD)
    z = z ^ (z >> np.uint64(33))
    z = z * np.uint64(0xC4CEB9FE1A85EC53)
    return z ^ (z >> np.uint64(33))


def panel_hashes(panels):
    """Host mirror of the device 128-bit panel hash: uint64[S, 2] from uint64[S, W]."""
    p = np.ascontiguousarray(panels, np.uint64)
    S, W = p.shape
    w = np.arange(W, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h1 = _fmix_a(p ^ (w * np.uint64(0x9E3779B97F4A7C15))).sum(axis=1, dtype=np.uint64)
        h2 = _fmix_b(p + (w + np.uint64(1)) * np.uint64(0xD6E8FEB86659FD93)).sum(axis=1, dtype=np.uint64)
    return np.stack([h1, h2], axis=1)


def exchange_capacity(n_local, world):
    """Entries per owner segment for a rank with n_local panels: the distinct panels reaching one
    owner are Binomial(m <= n_local, 1/world) under a uniform hash, so mean + 8 sd + 64 never
    overflows in practice (P < 1e-15 per segment); never more than n_local."""
    n_local, world = max(int(n_local), 1), int(world)
    mean = -(-n_local // world)
    return min(n_local, mean + 8 * int(mean ** 0.5 + 1) + 64)


def local_distinct(hashes, panels):
    """Host mirror of the first stage of csa_exchange_pack_async: the exact distinct rows (hash AND
    bitmask) of uint64[m, 2] / uint64[m, W]."""
    h = np.asarray(hashes, np.uint64).reshape(-1, 2)
    p = np.asarray(panels, np.uint64)
    assert p.ndim == 2 and len(p) == len(h)
    if len(h) == 0:
        return h, p
    u = np.unique(np.concatenate([h, p], axis=1), axis=0)
    return np.ascontiguousarray(u[:, :2]), np.ascontiguousarray(u[:, 2:])


def segment_buckets(hashes, panels, world, cap):
    """Host mirror of csa_exchange_pack_async (panels uint64[m, W]): the local distinct panels in
    fixed-capacity owner segments.  Returns (uint64[world, cap, 2], uint64[world, cap, W], int64[world] counts)."""
    h, p = local_distinct(hashes, panels)
    W = p.shape[1]
    sh = np.zeros((world, cap, 2), np.uint64)
    sp = np.zeros((world, cap, W), np.uint64)
    sc = np.zeros(world, np.int64)
    owner = (h[:, 0] % np.uint64(world)).astype(np.int64) if len(h) else np.zeros(0, np.int64)
    for w in range(world):
        sel = np.nonzero(owner == w)[0]
        if len(sel) > cap:
            raise RuntimeError("distinct-panel exchange: %d panels for owner %d exceed the segment capacity %d"
                               % (len(sel), w, cap))
        sh[w, : len(sel)] = h[sel]
        sp[w, : len(sel)] = p[sel]
        sc[w] = len(sel)
    return sh, sp, sc


def distinct_exact(hashes, panels):
    """Host mirror of csa_unique_async: distinct panels, equal iff hash AND bitmask are equal."""
    p = np.asarray(panels, np.uint64)
    if len(p) == 0:
        return 0
    h = np.asarray(hashes, np.uint64).reshape(len(p), 2)
    return int(len(np.unique(np.concatenate([h, p.reshape(len(p), -1)], axis=1), axis=0)))


def distinct_segments(hashes, panels, counts):
    """Host mirror of csa_unique_segments_async: distinct panels among the valid leading entries of
    each segment (uint64[world, cap, 2], uint64[world, cap, W], counts[world])."""
    h = np.asarray(hashes, np.uint64)
    p = np.asarray(panels, np.uint64)
    c = [int(x) for x in counts]
    hv = np.concatenate([h[w, : c[w]] for w in range(len(c))]) if c else np.zeros((0, 2), np.uint64)
    pv = np.concatenate([p[w, : c[w]] for w in range(len(c))]) if c else np.zeros((0, p.shape[-1]), np.uint64)
    return distinct_exact(hv, pv)


def _local_multiplicities(h, p):
    """Host mirror of csa_unique_mult_async: per distinct (hash, bitmask) row of uint64[m, 2] / uint64[m, W]
    its lowest index and its number of copies, ascending in the index (int64 each)."""
    if len(h) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, first, mult = np.unique(np.concatenate([h, p], axis=1), axis=0, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    return first[order].astype(np.int64), mult[order].astype(np.int64)


def mult_key_buckets(hashes, panels, panel_begin, world, cap):
    """Host mirror of csa_unique_mult_async + csa_exchange_mult_keys_async (hashes uint64[m, 2], panels
    uint64[m, W], this rank's, global indices from ``panel_begin``): one 32-byte key (h1, h2, panel_begin
    + first local index, local multiplicity) per local distinct panel, in fixed-capacity owner segments
    (h1 % world).  Returns (uint64[world, cap, 4], int64[world] counts); a segment past ``cap`` raises."""
    h = np.asarray(hashes, np.uint64).reshape(-1, 2)
    p = np.asarray(panels, np.uint64)
    assert p.ndim == 2 and len(p) == len(h)
    first, mult = _local_multiplicities(h, p)
    keys = np.zeros((world, cap, 4), np.uint64)
    sc = np.zeros(world, np.int64)
    owner = (h[first, 0] % np.uint64(world)).astype(np.int64)
    for w in range(world):
        sel = np.nonzero(owner == w)[0]
        if len(sel) > cap:
            raise RuntimeError("panel-multiplicity exchange: %d panels for owner %d exceed the segment capacity %d"
                               % (len(sel), w, cap))
        keys[w, : len(sel), :2] = h[first[sel]]
        keys[w, : len(sel), 2] = (first[sel] + int(panel_begin)).astype(np.uint64)
        keys[w, : len(sel), 3] = mult[sel].astype(np.uint64)
        sc[w] = len(sel)
    return keys, sc


def merge_mult_keys(keys, counts, panels_of):
    """Host mirror of csa_merge_mult_keys_async: the valid leading keys of each segment (uint64[segments, cap,
    4], counts[segments]) merged into one entry per distinct panel -- equal 128-bit hash AND equal bitmask;
    multiplicity = the sum of the keys', first = the lowest of their global indices.  ``panels_of(global
    indices)`` -> uint64[len, W] stands for the owner's re-draw and is asked only for keys whose hash occurs
    more than once.  Returns (first int64[u], mult int64[u]) ascending in first."""
    k = np.asarray(keys, np.uint64)
    c = [int(x) for x in counts]
    v = np.concatenate([k[s, : c[s]] for s in range(len(c))]) if c else np.zeros((0, 4), np.uint64)
    if len(v) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, group, size = np.unique(v[:, :2], axis=0, return_inverse=True, return_counts=True)
    group = group.reshape(-1)
    shared = np.nonzero(size[group] > 1)[0]
    label = np.stack([group.astype(np.int64), np.zeros(len(v), np.int64)], axis=1)
    if len(shared):
        rows = np.ascontiguousarray(panels_of(v[shared, 2].astype(np.int64)), np.uint64).reshape(len(shared), -1)
        _, which = np.unique(rows, axis=0, return_inverse=True)
        label[shared, 1] = which.reshape(-1) + 1
    _, entry = np.unique(label, axis=0, return_inverse=True)
    entry = entry.reshape(-1)
    u = int(entry.max()) + 1
    mult = np.zeros(u, np.int64)
    np.add.at(mult, entry, v[:, 3].astype(np.int64))
    first = np.full(u, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, entry, v[:, 2].astype(np.int64))
    order = np.argsort(first, kind="stable")
    return first[order], mult[order]


def mult_record(mult, n_bins):
    """Host mirror of csa_mult_spectrum_async's record over a list's multiplicities: int64 [length |
    spectrum[n_bins] | entries >= n_bins, max, sum m^2, sum m]."""
    m = np.asarray(mult, np.int64)
    out = np.zeros(1 + n_bins + 4, np.int64)
    out[0] = len(m)
    out[1:1 + n_bins] = np.bincount(m[m < n_bins], minlength=n_bins)
    out[1 + n_bins:] = [int((m >= n_bins).sum()), int(m.max()) if len(m) else 0, int((m * m).sum()), int(m.sum())]
    return out


class HashTable:
    """Reusable device table + count for csa_unique_async (grows on demand)."""

    def __init__(self, max_hashes, device):
        import torch
        self.device = device
        self.count = torch.zeros(1, dtype=torch.int64, device=device)
        self.slots = 0
        self.ensure(max_hashes)

    def ensure(self, n_hashes):
        import torch
        slots = 64
        while slots < 2 * max(int(n_hashes), 1):
            slots <<= 1
        if slots > self.slots:
            self.slots = slots
            self.table = torch.empty(slots, dtype=torch.int64, device=self.device)


def _host_collectives(t):
    """gloo rehearsals of the device path (CSA_BENCH_BACKEND=gloo) run the collectives on host copies."""
    import torch.distributed as dist
    return t.is_cuda and dist.get_backend() != "nccl"


def _all_to_all(out, inp):
    """Equal-split all_to_all_single, through host copies for a gloo rehearsal on device tensors."""
    import torch.distributed as dist
    if _host_collectives(inp):
        o = out.cpu()
        dist.all_to_all_single(o, inp.cpu())
        out.copy_(o)
    else:
        dist.all_to_all_single(out, inp)


class PanelExchange:
    """The distinct-panel exchange of one rank, buffers sized once for n_local panels of W words.

    ``run(hashes, panels, n, status, stream, panel_begin)`` returns this rank's owner count (a
    1-element int64 tensor, device or host like the inputs); the caller all_reduces it.  Device
    inputs: no host synchronisation, so a caller can enqueue the next steps behind it.

    With ``redraw = (instance handle, k, seed, max_attempts)`` (the draw that made the panels, Philox
    mode) the 24-byte exchange runs: keys (h1, h2, global panel index) instead of bitmasks
    (csa_exchange_keys_async -> two equal-split all_to_alls -> csa_unique_keys_async, which re-draws
    only the hash-matched entries to compare their bitmasks).  Without it, the bitmasks travel
    (csa_exchange_pack_async -> three all_to_alls -> csa_unique_segments_async); host tensors always
    take that form through its numpy mirrors."""

    def __init__(self, n_local, W, world, device, redraw=None):
        import torch
        from . import _native as N
        self.W, self.world, self.device = int(W), int(world), device
        self.n_local = max(int(n_local), 1)
        self.cap = exchange_capacity(self.n_local, self.world)
        self.cuda = torch.device(device).type == "cuda"
        self.redraw = redraw if self.cuda else None
        if not self.cuda:
            return
        i64 = torch.int64
        seg = self.world * self.cap
        sb = int(N.lib().csa_exchange_scratch_bytes(self.n_local))
        self.scratch = torch.empty((sb + 7) // 8, dtype=i64, device=device)
        self.send_c = torch.zeros(self.world, dtype=i64, device=device)
        self.recv_c = torch.zeros_like(self.send_c)
        self.unique = torch.zeros(1, dtype=i64, device=device)
        if self.redraw is not None:
            self.send_k = torch.empty(3 * seg, dtype=i64, device=device)
            self.recv_k = torch.empty_like(self.send_k)
            ob = int(N.lib().csa_unique_keys_scratch_bytes(seg, self.W))
            self.owner_scratch = torch.empty((ob + 7) // 8, dtype=i64, device=device)
            return
        self.send_h = torch.empty(2 * seg, dtype=i64, device=device)
        self.send_p = torch.empty(seg * self.W, dtype=i64, device=device)
        self.recv_h = torch.empty_like(self.send_h)
        self.recv_p = torch.empty_like(self.send_p)
        self.table = HashTable(seg, device)

    def bytes_sent(self):
        """Bytes this rank puts into the all_to_alls per run (segments of every owner, itself included)."""
        per = 24 if self.redraw is not None else 16 + 8 * self.W
        return self.world * self.cap * per + 8 * self.world

    def run(self, hashes, panels, n, status=None, stream=None, panel_begin=0, redraw=None):
        """``redraw`` overrides the constructor's (instance, k, seed, max_attempts) for this run (a
        cached exchange serves calls with different seeds); the form -- keys or bitmasks -- is the
        constructor's."""
        import torch
        n = int(n)
        if redraw is not None and self.redraw is not None:
            self.redraw = redraw
        assert n <= self.n_local
        if not hashes.is_cuda:
            import torch.distributed as dist
            sh, sp, sc = segment_buckets(hashes.numpy().view(np.uint64)[: 2 * n],
                                         panels.numpy().view(np.uint64)[: n * self.W].reshape(n, self.W),
                                         self.world, self.cap)
            rh, rp, rc = (torch.empty(x.shape, dtype=torch.int64) for x in (sh, sp, sc))
            dist.all_to_all_single(rc, torch.from_numpy(sc))
            dist.all_to_all_single(rh, torch.from_numpy(sh.view(np.int64)))
            dist.all_to_all_single(rp, torch.from_numpy(sp.view(np.int64)))
            u = distinct_segments(rh.numpy().view(np.uint64), rp.numpy().view(np.uint64), rc.numpy())
            return torch.tensor([u], dtype=torch.int64)
        from . import _native as N
        assert status is not None, "the device exchange reports a full segment in the status block"
        st = stream or torch.cuda.current_stream(hashes.device)
        sp_ = ctypes.c_void_p(st.cuda_stream)
        L = N.lib()
        if self.redraw is not None:
            handle, k, seed, max_att = self.redraw
            N.check(L.csa_exchange_keys_async(N.ptr(hashes), N.ptr(panels), n, self.W, int(panel_begin), self.world,
                                              self.cap, N.ptr(self.scratch), self.scratch.numel() * 8,
                                              N.ptr(self.send_k), N.ptr(self.send_c), N.ptr(status), sp_))
            with torch.cuda.stream(st):
                _all_to_all(self.recv_c, self.send_c)
                _all_to_all(self.recv_k, self.send_k)
                self.unique.zero_()
            N.check(L.csa_unique_keys_async(handle, int(k), int(seed) & M64, int(max_att), N.ptr(self.recv_k),
                                            self.world, self.cap, N.ptr(self.recv_c), N.ptr(self.owner_scratch),
                                            self.owner_scratch.numel() * 8, N.ptr(self.unique), N.ptr(status), sp_))
            with torch.cuda.stream(st):
                return self.unique.clone()
        N.check(L.csa_exchange_pack_async(N.ptr(hashes), N.ptr(panels), n, self.W, self.world, self.cap,
                                          N.ptr(self.scratch), self.scratch.numel() * 8, N.ptr(self.send_h),
                                          N.ptr(self.send_p), N.ptr(self.send_c), N.ptr(status), sp_))
        with torch.cuda.stream(st):
            _all_to_all(self.recv_c, self.send_c)
            _all_to_all(self.recv_h, self.send_h)
            _all_to_all(self.recv_p, self.send_p)
            self.table.count.zero_()
        N.check(L.csa_unique_segments_async(N.ptr(self.recv_h), N.ptr(self.recv_p), self.world, self.cap,
                                            N.ptr(self.recv_c), self.W, N.ptr(self.table.table), self.table.slots,
                                            N.ptr(self.table.count), N.ptr(status), sp_))
        with torch.cuda.stream(st):
            return self.table.count.clone()


    # ---- the 32-byte exchange: the panel multiplicities travel with the keys --------------------
    def _mult_buffers(self, n_bins):
        """The buffers of run_multiplicity, sized once for this exchange (and one spectrum width)."""
        import torch
        from . import _native as N
        b = getattr(self, "_mult", None)
        if b is not None and b["n_bins"] == n_bins:
            return b
        L, dev, seg = N.lib(), self.device, self.world * self.cap
        i64, i32 = torch.int64, torch.int32
        lb = int(L.csa_unique_mult_scratch_bytes(self.n_local))
        ob = int(L.csa_merge_mult_keys_scratch_bytes(seg, self.W))
        b = self._mult = {
            "n_bins": n_bins,
            "local_scratch": torch.empty((lb + 7) // 8, dtype=i64, device=dev),
            "local_first": torch.empty(self.n_local, dtype=i32, device=dev),
            "local_mult": torch.empty(self.n_local, dtype=i32, device=dev),
            "local_len": torch.zeros(1, dtype=i64, device=dev),
            "send_k": torch.empty(4 * seg, dtype=i64, device=dev),
            "recv_k": torch.empty(4 * seg, dtype=i64, device=dev),
            "owner_scratch": torch.empty((ob + 7) // 8, dtype=i64, device=dev),
            "first": torch.empty(seg, dtype=i32, device=dev),
            "mult": torch.empty(seg, dtype=i32, device=dev),
            "record": torch.zeros(1 + n_bins + 4, dtype=i64, device=dev),
        }
        return b

    def run_multiplicity(self, hashes, panels, n, status=None, stream=None, panel_begin=0, redraw=None, n_bins=4096,
                         panels_of=None):
        """The exchange in which the counts travel.  This rank's (first, multiplicity) list
        (csa_unique_mult_async -- the local dedupe, run once) goes out as 32-byte keys (h1, h2, global first
        index, multiplicity) to the hashes' owners (csa_exchange_mult_keys_async, two equal-split
        all_to_alls: counts and keys); the owner merges what it received (csa_merge_mult_keys_async,
        re-drawing hash-matched keys with ``redraw`` = (instance, k, seed, max_attempts)) and takes the
        spectrum of its list (csa_mult_spectrum_async, ``n_bins`` bins).

        Returns (first, mult, record): the owner's list -- the panels whose h1 % world is this rank, int32
        tensors of world * cap uint32 words, zero past the list -- and int64 [length | spectrum[n_bins] |
        overflow, max, sum m^2, sum m].  All three are buffers of the exchange, overwritten by its next run.
        Device inputs: nothing waits.  Host tensors run the numpy mirrors (mult_key_buckets, merge_mult_keys
        with ``panels_of(global indices)`` for the re-draw) and return int64 tensors of the list's length."""
        import torch
        n, n_bins = int(n), int(n_bins)
        assert n <= self.n_local
        if not hashes.is_cuda:
            import torch.distributed as dist
            keys, sc = mult_key_buckets(hashes.numpy().view(np.uint64)[: 2 * n].reshape(n, 2),
                                        panels.numpy().view(np.uint64)[: n * self.W].reshape(n, self.W),
                                        panel_begin, self.world, self.cap)
            rk, rc = (torch.empty(x.shape, dtype=torch.int64) for x in (keys, sc))
            dist.all_to_all_single(rc, torch.from_numpy(sc))
            dist.all_to_all_single(rk, torch.from_numpy(keys.view(np.int64)))
            first, mult = merge_mult_keys(rk.numpy().view(np.uint64), rc.numpy(), panels_of)
            return torch.from_numpy(first), torch.from_numpy(mult), torch.from_numpy(mult_record(mult, n_bins))
        from . import _native as N
        assert status is not None, "the device exchange reports a full segment in the status block"
        assert self.redraw is not None, "the multiplicity exchange re-draws: build the exchange with redraw="
        handle, k, seed, max_att = redraw if redraw is not None else self.redraw
        st = stream or torch.cuda.current_stream(hashes.device)
        sp_ = ctypes.c_void_p(st.cuda_stream)
        L = N.lib()
        with torch.cuda.stream(st):
            b = self._mult_buffers(n_bins)
        rec = b["record"]
        N.check(L.csa_unique_mult_async(N.ptr(hashes), N.ptr(panels), n, self.W, N.ptr(b["local_scratch"]),
                                        b["local_scratch"].numel() * 8, N.ptr(b["local_first"]), N.ptr(b["local_mult"]),
                                        N.ptr(b["local_len"]), N.ptr(status), sp_))
        N.check(L.csa_exchange_mult_keys_async(N.ptr(hashes), n, N.ptr(b["local_first"]), N.ptr(b["local_mult"]),
                                               N.ptr(b["local_len"]), int(panel_begin), self.world, self.cap,
                                               N.ptr(b["send_k"]), N.ptr(self.send_c), N.ptr(status), sp_))
        with torch.cuda.stream(st):
            _all_to_all(self.recv_c, self.send_c)
            _all_to_all(b["recv_k"], b["send_k"])
        N.check(L.csa_merge_mult_keys_async(handle, int(k), int(seed) & M64, int(max_att), N.ptr(b["recv_k"]),
                                            self.world, self.cap, N.ptr(self.recv_c), N.ptr(b["owner_scratch"]),
                                            b["owner_scratch"].numel() * 8, N.ptr(b["first"]), N.ptr(b["mult"]),
                                            N.ptr(rec), N.ptr(status), sp_))
        N.check(L.csa_mult_spectrum_async(N.ptr(b["mult"]), N.ptr(rec), self.world * self.cap, N.ptr(rec[1:]), n_bins,
                                          N.ptr(rec[1 + n_bins:]), sp_))
        return b["first"], b["mult"], rec


def _all_gather(out, inp):
    """all_gather of equal 1-D tensors into ``out`` (world * len), through host copies for a gloo rehearsal
    on device tensors."""
    import torch.distributed as dist
    if _host_collectives(inp) or not inp.is_cuda:
        parts = list(out.cpu().split(inp.numel()))
        dist.all_gather(parts, inp.cpu())
        import torch
        out.copy_(torch.cat(parts))
    else:
        dist.all_gather_into_tensor(out, inp)


def _all_reduce_pairs(pairs, pair_bound, stream):
    """all_reduce(SUM) of the pair counts.  On GPU tensors with every summed count < 2^31
    (``pair_bound``: the panels of the whole job) only the upper triangle travels, as int32."""
    import torch
    import torch.distributed as dist
    n = int(round(pairs.numel() ** 0.5))
    if pairs.is_cuda and pair_bound is not None and pair_bound < 2 ** 31 and not _host_collectives(pairs):
        from . import _native as N
        sp = ctypes.c_void_p((stream or torch.cuda.current_stream(pairs.device)).cuda_stream)
        packed = torch.empty(n * (n + 1) // 2, dtype=torch.int32, device=pairs.device)
        N.check(N.lib().csa_pairs_pack_async(N.ptr(pairs), n, N.ptr(packed), sp))
        dist.all_reduce(packed, op=dist.ReduceOp.SUM)
        N.check(N.lib().csa_pairs_unpack_async(N.ptr(packed), n, N.ptr(pairs), sp))
    elif _host_collectives(pairs):
        h = pairs.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM)
        pairs.copy_(h)
    else:
        dist.all_reduce(pairs, op=dist.ReduceOp.SUM)


def _all_reduce(t, op=None):
    import torch.distributed as dist
    op = dist.ReduceOp.SUM if op is None else op
    if _host_collectives(t):
        h = t.cpu()
        dist.all_reduce(h, op=op)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=op)


def combine(counts, pairs, hashes, panels, W, exchange=None, stream=None, pair_bound=None, status=None, redraw=None,
            panel_begin=0):
    """Exchange steps for this rank; returns (counts, pairs, unique_tensor), all stream-ordered.

    counts int64[n], pairs int64[n*n] or None, hashes int64[2*S_local] and panels
    int64[S_local*W] (this rank's panels, global indices from ``panel_begin``).  Counts and pairs:
    all_reduce(SUM).  Distinct panels: ``exchange`` (a PanelExchange, built here if None, with
    ``redraw`` for the 24-byte keys) sends the local distinct panels to their owners, each owner
    counts exactly, all_reduce(SUM) of the counts.
    """
    import torch
    import torch.distributed as dist
    n_local = hashes.numel() // 2
    if exchange is None:
        # every rank must size its segments alike (equal-split all_to_all): the largest shard's
        n_max = torch.tensor([n_local], dtype=torch.int64, device=hashes.device)
        _all_reduce(n_max, op=dist.ReduceOp.MAX)
        exchange = PanelExchange(int(n_max.item()), W, dist.get_world_size(), hashes.device, redraw=redraw)
    _all_reduce(counts)
    if pairs is not None:
        _all_reduce_pairs(pairs, pair_bound, stream)
    u = exchange.run(hashes, panels, n_local, status=status, stream=stream, panel_begin=panel_begin)
    if u.is_cuda:
        with torch.cuda.stream(stream or torch.cuda.current_stream(u.device)):
            _all_reduce(u)
    else:
        _all_reduce(u)
    return counts, pairs, u


def local_distinct_rows(hashes, panels, n, W, status=None, stream=None):
    """This rank's exact distinct panels (hash AND bitmask): (uint64 rows as an int64 tensor of
    count*W words on the inputs' device, count).  Device inputs: csa_exchange_pack_async with one
    owner (the partitioned dedupe + bucketing of the exchange); host inputs: local_distinct."""
    import torch
    n, W = int(n), int(W)
    if not hashes.is_cuda:
        _, p = local_distinct(hashes.numpy().view(np.uint64)[: 2 * n], panels.numpy().view(np.uint64)[: n * W]
                              .reshape(n, W))
        return torch.from_numpy(np.ascontiguousarray(p).view(np.int64).reshape(-1)), len(p)
    from . import _native as N
    dev = hashes.device
    st = stream or torch.cuda.current_stream(dev)
    m = max(n, 1)
    send_h = torch.empty(2 * m, dtype=torch.int64, device=dev)
    send_p = torch.empty(m * W, dtype=torch.int64, device=dev)
    send_c = torch.zeros(1, dtype=torch.int64, device=dev)
    sb = int(N.lib().csa_exchange_scratch_bytes(m))
    scratch = torch.empty((sb + 7) // 8, dtype=torch.int64, device=dev)
    own_status = status if status is not None else torch.zeros(4, dtype=torch.int32, device=dev)
    N.check(N.lib().csa_exchange_pack_async(N.ptr(hashes), N.ptr(panels), n, W, 1, m, N.ptr(scratch), sb,
                                            N.ptr(send_h), N.ptr(send_p), N.ptr(send_c), N.ptr(own_status),
                                            ctypes.c_void_p(st.cuda_stream)))
    st.synchronize()
    if status is None:
        N.raise_status(own_status.cpu().numpy().astype(np.uint32))
    cnt = int(send_c.item())
    return send_p[: cnt * W], cnt


class PanelRedraw:
    """found_panels of a sharded run, re-made where they are read instead of gathered.

    Every panel is a pure function of (instance, k, seed, global panel index): the Philox counter
    of each draw is (step, attempt, panel) under the key ``seed``, so the
    panels [0, S) of the whole job -- every rank's shard -- can be drawn again on any one process.
    Calling this re-draws them in chunks of ``chunk`` panels through ``draw(begin, count)`` (a
    callable returning uint64[count, W]; ``device_redraw`` for the product path) into one host
    array -- or, where the draw offers device chunks (``streams``), ``table`` folds them on the device
    into the sorted table of distinct panels, bounded by the distinct count and not by S -- with no
    collective: any rank may iterate, test membership or pickle its found_panels at any time, alone.
    The reference only ever takes len() of the set (analysis.py:575, 580) and
    pickles it (analysis.py:290); len() needs no re-draw (the exchange's exact count)."""

    def __init__(self, draw, S, W, chunk=1 << 20):
        self.draw, self.S, self.W, self.chunk = draw, int(S), int(W), max(1, int(chunk))

    def __call__(self):
        out = np.empty((self.S, max(self.W, 1)), np.uint64)
        for off in range(0, self.S, self.chunk):
            c = min(self.chunk, self.S - off)
            out[off:off + c] = self.draw(off, c)
        return out

    def streams(self):
        """The draw offers device chunks (``device_chunk`` / ``tables``, as ``device_redraw``'s does) and
        CSA_ROWS_HOST=1 does not force the host path: ``table`` is the way to read the panels."""
        from .stats import rows_host_path
        return hasattr(self.draw, "device_chunk") and hasattr(self.draw, "tables") and not rows_host_path()

    def table(self, count, lists=False):
        """The streaming form: the job's distinct panels as host ``(rows uint64[D, W] sorted as
        PanelSet.rows() sorts them, first int64[D], mult int64[D])`` -- the lists None unless ``lists`` --
        without the S x W array.  Per chunk: re-draw it on the device, sort-unique it with its global
        indices (csa_rows_sort_unique_async), merge it into the table so far (csa_rows_merge_unique_async),
        whose capacity is ``count``, the run's exact distinct count, in ping-pong buffers; nothing is read
        in between.  Then one host wait: status, length, the D rows and lists.  A length other than
        ``count`` -- or a table that overflowed, i.e. more distinct panels than counted -- raises
        RuntimeError; so does, before anything is drawn, a job whose buffers exceed the free device memory
        (stats.table_bytes)."""
        from . import _native as N
        from .stats import table_bytes
        count, W = int(count), max(self.W, 1)
        C = max(1, min(self.chunk, self.S))
        ops = self.draw.tables()
        need, free = table_bytes(count, C, W), ops.free_bytes()
        if need > free:
            raise RuntimeError("found_panels: reading %d distinct panels of %d draws needs %d bytes of device memory, "
                               "%d are free" % (count, self.S, need, free))
        acc, spare = ops.new_table(count, W), ops.new_table(count, W)
        for off in range(0, self.S, self.chunk):
            c = min(self.chunk, self.S - off)
            part = ops.sort_unique(self.draw.device_chunk(off, c), c, W, off)
            acc, spare = ops.merge(acc, part, spare), acc
        words, length, rows, first, mult = ops.read(acc, lists, getattr(self.draw, "status", None))
        N.raise_status(words[:4])                       # the re-draw's own status block
        if words[4] == N.CSA_E_UNSUPPORTED:
            raise RuntimeError("found_panels: the re-drawn panels hold more than %d distinct panels, the run "
                               "counted %d" % (count, count))
        N.raise_status(words[4:])
        if length != count:
            raise RuntimeError("found_panels: the re-drawn panels hold %d distinct panels, the run counted %d"
                               % (length, count))
        return rows, first, mult


def device_redraw(enc, k, seed, device, max_attempts=0):
    """``draw(begin, count)`` for PanelRedraw on ``device``: csa_redraw_async (the batch draw's kernel
    and Philox counters, not counted in the instance's draw statistics) into a device buffer, then one
    copy to the host.  The callable also carries ``device_chunk(begin, count)``, the same chunk left on the
    device with no copy and no status read, ``status``, the one block all such chunks raise into, and
    ``tables()``, the sorted-table operations PanelRedraw.table streams them through.  The re-drawn
    status block is decoded: the original call already succeeded on every rank, so an error here is
    raised, never ignored."""
    import torch
    from . import _native as N
    W = enc.W
    seed64 = int(seed) & M64

    def draw(begin, count):
        with torch.cuda.device(device):
            st = torch.cuda.current_stream(device)
            buf = torch.empty(max(count * W, 1), dtype=torch.int64, device=device)
            status = torch.zeros(4, dtype=torch.int32, device=device)
            N.check(N.lib().csa_redraw_async(enc.handle, int(k), seed64, int(begin), int(count), int(max_attempts),
                                             N.ptr(buf), N.ptr(status), ctypes.c_void_p(st.cuda_stream)))
            host = buf[:count * W].cpu()
            words = status.cpu().numpy().astype(np.uint32)
        N.raise_status(words)
        return host.numpy().view(np.uint64).reshape(count, W)

    def device_chunk(begin, count):
        """The chunk as a device tensor (int64 words, count * W), enqueued on the device's current stream:
        no host copy, no status read -- every chunk of a re-draw raises into ``draw.status``."""
        with torch.cuda.device(device):
            st = torch.cuda.current_stream(device)
            if draw.status is None:
                draw.status = torch.zeros(4, dtype=torch.int32, device=device)
            buf = torch.empty(max(count * W, 1), dtype=torch.int64, device=device)
            N.check(N.lib().csa_redraw_async(enc.handle, int(k), seed64, int(begin), int(count), int(max_attempts),
                                             N.ptr(buf), N.ptr(draw.status), ctypes.c_void_p(st.cuda_stream)))
        return buf

    def tables():
        """The table operations of a streamed read (stats.DeviceRowTables) on the same device and stream; a
        fresh status block for the re-draw it serves."""
        from .stats import DeviceRowTables
        with torch.cuda.device(device):
            draw.status = torch.zeros(4, dtype=torch.int32, device=device)
            return DeviceRowTables(device, torch.cuda.current_stream(device))

    draw.status = None
    draw.device_chunk, draw.tables = device_chunk, tables
    return draw


ERR_DRAW_PRIORITY = 1 << 16     # status codes are small; draw errors reduce above every other code


def _decode_status(words, reduced_code):
    """Raise the error of a status block (host uint32[4]); a rank whose own block is clean -- or holds
    another error than the one the ranks agreed on (``reduced_code``) -- raises the agreed code
    (KeyError for a missing candidate, legacy.py:188), so every rank raises the same error."""
    from . import _native as N
    h = np.asarray(words, np.uint32)
    if int(h[0]) != int(reduced_code):
        h = np.array([reduced_code, 0xFFFFFFFF, 0xFFFFFFFF, 0], np.uint32)
    N.raise_status(h)


def _shard_exchange(enc, n_max, world, dev):
    """The encoding's cached PanelExchange (24-byte keys) for shares of at most n_max panels."""
    ex = getattr(enc, "_xchg", None)
    if ex is None or ex.n_local < max(int(n_max), 1) or ex.world != int(world) or ex.device != dev:
        enc._xchg = None
        ex = enc._xchg = PanelExchange(n_max, enc.W, world, dev, redraw=(enc.handle, 0, 0, 0))
    return ex


def shard_device():
    """The GPU of this rank: LOCAL_RANK (one process per GPU, as torchrun sets it), modulo the visible
    devices so rehearsals can put several ranks on one GPU; without LOCAL_RANK, the current device.
    Never changes the caller's current device."""
    import torch
    lr = os.environ.get("LOCAL_RANK")
    idx = int(lr) % max(torch.cuda.device_count(), 1) if lr is not None else torch.cuda.current_device()
    return torch.device("cuda", idx)


def legacy_probabilities_distributed(instance, iterations, random_seed, keep_panels=True, chunk=None,
                                     timings=None, groups=None, multiplicity=False, top_keep=64):
    """analysis.py:162-191 with the panels sharded over the ranks of the default group.  Every rank
    returns the whole job's alloc, pair histogram and exact distinct-panel count.

    Per call (cheap when repeated): the encoding, the device pipeline (picks / XT / pair scratch
    sized to one ``chunk`` of panels, default 2^20 or CSA_SHARD_CHUNK) and the 24-byte key exchange
    are cached on the encoding; the share's panels and hashes and the n*n pair matrix are fresh
    tensors (caching allocator).  Draws, counting, pairs, the draw statistics and every collective
    are stream-ordered; the host waits once, for one copy of [counts | statistics | distinct count |
    status].  The pair counts stay on the device behind the returned PairHistogram (packed and
    divided there when first read).  Runs on ``shard_device()`` without changing the caller's current
    device.

    found_panels: len() is the exchange's exact global count.  With more than one rank (or a forced
    exchange) nothing else is kept and nothing is sent: iterating, ``in``, ``rows()`` or pickling on
    ANY rank re-draws the job's panels [0, S) on that rank's GPU (PanelRedraw, csa_redraw_async) and
    deduplicates them there, chunk by chunk into the sorted table of distinct panels (PanelRedraw.table:
    the read is bounded by the distinct count, not by S) -- no collective, so a rank may do it alone, at
    any time.  One rank (no exchange): the panels of the call are the whole run's and stay on the device, decoded when read, as
    the one-GPU call does.  ``keep_panels=False``: len() only.  The draw statistics
    (analysis.LAST_RUN_STATS) are summed over ranks.  ``timings`` (a dict) gets the host-side stage
    times in ms.  ``groups`` (a stats.GroupSet; analysis.legacy_composition's sharded form): every rank
    runs group_hist_kernel over its share and the tables are summed in one more all_reduce; the call
    then returns a fourth value, the CompositionHistogram of the whole job on every rank -- never a
    share's.

    ``multiplicity`` (``legacy_panel_distribution_distributed``): the run also returns, last, its
    stats.PanelDistribution.  With an exchange the 32-byte one (PanelExchange.run_multiplicity) runs in
    place of the 24-byte one -- the distinct count is the sum of the owners' list lengths -- the owners'
    spectra and sums ride in the same all_reduce(SUM), the maximum in the MAX reduce beside the status
    code, and each owner's ``top_keep`` most frequent entries are gathered to every rank; all of it comes
    back in the one host copy.  Only a global maximum of MULT_BINS or more costs a second spectrum pass,
    all_reduce and copy, on every rank alike.  Without an exchange the one-GPU passes run
    (stats.unique_mult_device), as in analysis.legacy_sample_device."""
    import time
    import torch
    import torch.distributed as dist
    from . import analysis as A
    from . import _native as N
    t0 = time.perf_counter()
    world, r = world_size(), rank()
    S = int(iterations)
    if multiplicity and S >= 1 << 32:     # the same on every rank, before any collective
        raise ValueError("panel multiplicities: %d draws do not fit the lists' 32-bit counts and indices" % S)
    top_keep = max(0, int(top_keep))
    mb = A.MULT_BINS
    A.seed(random_seed)
    A.STREAM.take_panels(S)
    enc = A.encode_cached(instance.categories, instance.agents)
    k = int(instance.k)
    enc.check_quotas(k)
    begin, end = shard_range(S, world, r)
    local = end - begin
    n_max = shard_range(S, world, 0)[1]          # rank 0 holds the largest share
    dev = shard_device()
    C = max(1, min(max(local, 1), int(chunk or os.environ.get("CSA_SHARD_CHUNK", 1 << 20))))
    W, n = enc.W, enc.n
    with torch.cuda.device(dev):
        pipe = A.cached_pipeline(enc, k, C)
        # (CSA_FORCE_EXCHANGE=1: the key exchange even for one rank -- tests of its collectives on one GPU)
        ex = _shard_exchange(enc, n_max, world, dev) if world > 1 or os.environ.get("CSA_FORCE_EXCHANGE") == "1" \
            else None
        st = pipe.stream
        t1 = time.perf_counter()
        with torch.cuda.stream(st):
            panels = torch.empty(max(local * W, 1), dtype=torch.int64, device=dev)
            hashes = torch.empty(max(2 * local, 2), dtype=torch.int64, device=dev)
            pairs = torch.empty(n * n, dtype=torch.int64, device=dev)
            # [counts (n) | attempts, SelectionErrors, rejections | distinct count]: one all_reduce(SUM)
            # (a multiplicity run through the exchange: | spectrum[mb] | overflow, sum m^2, sum m)
            sharded_mult = multiplicity and ex is not None
            acc = torch.zeros(n + 4 + (mb + 3 if sharded_mult else 0), dtype=torch.int64, device=dev)
            d_counts, d_stats, d_unique = acc[:n + 4].split([n, 3, 1])
            pipe.reset(pairs=False)
            A.reset_draw_stats(enc, st)
            # one rank: its distinct-count table before the draws (analysis.distinct_table)
            table = A.distinct_table(enc, local, dev) if ex is None else None
            with pipe.bound(counts=d_counts, pairs=pairs):
                if local:
                    pipe.draw_count_chunks(random_seed, begin, local, panels, hashes, C, overwrite_pairs=True,
                                           reset_counts=True)
                else:
                    pairs.zero_()
            # this shard's draw statistics, before the exchange's re-draws (device, no host wait)
            A.read_draw_stats(enc, d_stats, st)
            fields = [("counts", d_counts), ("stats", d_stats), ("unique", d_unique)]
            if groups is not None:
                # the share's composition table on the pipeline stream (ordered after every draw); with
                # more than one rank (or a forced exchange) the tables are summed below
                d_hist = A.enqueue_group_hist(groups, groups.device_masks(dev, W), panels, local, W, k, pipe.status, st)
                fields.append(("hist", d_hist))
            if ex is not None:
                # a shard whose draw failed still enters the collectives (every rank must, or the others
                # hang); its status block joins the MAX all_reduce below, so every rank raises the draw's
                # error -- the exchange writes its own status only past a full segment, and the first
                # error recorded in a block wins (csa_status_decode)
                _all_reduce_pairs(pairs, S, st)
                if multiplicity:
                    o_first, o_mult, rec = ex.run_multiplicity(hashes, panels, local, status=pipe.status, stream=st,
                                                               panel_begin=begin, n_bins=mb,
                                                               redraw=(enc.handle, k, random_seed, 0))
                    u = rec[:1]          # the owners' list lengths sum to the job's distinct count
                    acc[n + 4:n + 4 + mb] = rec[1:1 + mb]
                    acc[n + 4 + mb:n + 5 + mb] = rec[1 + mb:2 + mb]      # overflow | (max: below) | sum m^2, sum m
                    acc[n + 5 + mb:] = rec[3 + mb:]
                else:
                    u = ex.run(hashes, panels, local, status=pipe.status, stream=st, panel_begin=begin,
                               redraw=(enc.handle, k, random_seed, 0))
            else:
                # one rank owns every panel: nothing to reduce, and the exact local distinct count runs on
                # a side stream after the draws, beside the last chunk's counting and pairs
                ust = pipe.distinct_count(table, hashes, panels, local,
                                          (pipe.draw_stream if local else st).record_event())
                if multiplicity:
                    from .stats import unique_mult_device
                    m_first, m_mult, m_out = unique_mult_device(hashes, panels, local, W, pipe.status, ust, mb)
                    fields += zip(A.MULT_FIELDS, m_out.split([1, mb, 4]))
                pipe.rejoin(ust)
                u = table.count
            d_unique.copy_(u)
            code = pipe.status[:1].to(torch.int64)
            if sharded_mult:
                # [status code | the largest multiplicity]: one MAX reduce
                red = torch.cat([code, rec[2 + mb:3 + mb]])
                code = red[:1]
            if ex is not None:
                _all_reduce(acc)
                if groups is not None:
                    _all_reduce(d_hist)
                # MAX over ranks of a priority key: a draw error (KeyError / attempt limit) on any rank
                # outranks an exchange error on another (an overflowing segment), whatever their codes
                code += ERR_DRAW_PRIORITY * ((code == N.CSA_E_NO_CANDIDATE) | (code == N.CSA_E_ATTEMPT_LIMIT))
                _all_reduce(red if sharded_mult else code, op=dist.ReduceOp.MAX)
                code %= ERR_DRAW_PRIORITY
            if sharded_mult:
                fields += [("mult_sums", acc[n + 4:]), ("mult_max", red[1:]), ("mult_owned", rec[:1])]
                if top_keep:
                    # each owner's top_keep best entries, to every rank: (multiplicity descending, first index
                    # ascending) is a total order, so the job's top_keep lie in the union of the owners'
                    best = _mult_order_keys(o_first, o_mult).topk(min(top_keep, o_mult.numel())).values
                    gathered = torch.empty(world * best.numel(), dtype=torch.int64, device=dev)
                    _all_gather(gathered, best)
                    fields.append(("mult_top", gathered))
            h, words = pipe.host_fields(fields + [("code", code)])     # the one host wait
        t2 = time.perf_counter()
    agreed = int(h["code"][0])
    if agreed:
        _decode_status(words, agreed)
    distribution = None
    if multiplicity:
        with torch.cuda.device(dev), torch.cuda.stream(st):
            if sharded_mult:
                distribution = _sharded_distribution(h, o_first, o_mult, rec, S, mb, top_keep, st)
            else:
                mult = A._multiplicity(h, m_first, m_mult, S, int(h["unique"][0]), st)
    stats = dict(zip(A.STAT_KEYS, (int(x) for x in h["stats"])))
    # one rank (no exchange): its panels are the whole run's, so found_panels keeps them on the device and
    # decodes them when iterated, as the one-GPU call does
    solo = ex is None and keep_panels
    comp = h["hist"][:len(groups) * (k + 1)].reshape(len(groups), k + 1).copy() if groups is not None else None
    raw = A.LegacyRaw(h["counts"].copy(), pairs.view(n, n), int(h["unique"][0]), panels[: local * W] if solo else None,
                      None, stats, comp)
    out = A.finish(instance, enc, raw, S) + ((A.composition(groups, raw, S, k),) if groups is not None else ())
    if keep_panels and not solo:
        # nothing kept, nothing sent: the whole job's panels are re-drawn where they are read
        out[1]._redraw = PanelRedraw(device_redraw(enc, k, random_seed, dev), S, W, chunk=max(C, 1 << 16))
    if multiplicity:
        from .stats import PanelDistribution
        if sharded_mult:
            distribution.bind(out[1]._redraw if keep_panels else None, enc.n, enc.agent_ids)
        else:
            distribution = PanelDistribution(S, mult["first"], mult["mult"], raw.panels, enc.n, enc.agent_ids,
                                             spectrum=mult["spectrum"], sum_squares=mult["sum_squares"])
        out = out + (distribution,)
    if timings is not None:
        t3 = time.perf_counter()
        timings.update(setup_ms=(t1 - t0) * 1e3, device_ms=(t2 - t1) * 1e3, finish_ms=(t3 - t2) * 1e3,
                       total_ms=(t3 - t0) * 1e3)
    return out


def _mult_order_keys(first, mult):
    """int64 keys of a device (first, multiplicity) list (uint32 words) whose SIGNED order is multiplicity
    descending-is-larger, then first index ascending-is-larger: (mult << 32 | ~first) with the sign bit
    flipped.  Zero entries past the list give the smallest key of all."""
    import torch
    m32 = 0xFFFFFFFF
    key = ((mult.to(torch.int64) & m32) << 32) | (m32 - (first.to(torch.int64) & m32))
    return key ^ (-1 << 63)


def mult_order_decode(keys):
    """Host (first, mult) int64 arrays of _mult_order_keys' keys, the zero entries dropped, ordered by
    multiplicity descending, then first index ascending."""
    k = np.asarray(keys, np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    k = np.sort(k[(k >> np.uint64(32)) != 0])[::-1]
    mult = (k >> np.uint64(32)).astype(np.int64)
    first = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return first, mult


def _sharded_distribution(h, o_first, o_mult, rec, S, mb, top_keep, stream):
    """The whole job's stats.ShardedPanelDistribution from the call's host copy ``h`` (the reduced record)
    and this rank's owner list (buffers of the exchange, ``rec`` its record: the list's entries are copied
    out here, on ``stream``).  A global maximum of ``mb`` or more takes the spectrum again with max + 1
    bins: every rank sees the same reduced maximum, so every rank enters the all_reduce."""
    import torch
    from . import _native as N
    from .stats import ShardedPanelDistribution
    over, sq, total = (int(x) for x in h["mult_sums"][mb:])
    top, distinct, owned = int(h["mult_max"][0]), int(h["unique"][0]), int(h["mult_owned"][0])
    spectrum = h["mult_sums"][:mb]
    if total != S:
        raise RuntimeError("panel multiplicities: the owners' lists sum to %d, the run drew %d panels" % (total, S))
    if over or top >= mb:
        out = torch.empty(top + 1 + 4, dtype=torch.int64, device=o_mult.device)
        N.check(N.lib().csa_mult_spectrum_async(N.ptr(o_mult), N.ptr(rec), o_mult.numel(), N.ptr(out), top + 1,
                                                N.ptr(out[top + 1:]), ctypes.c_void_p(stream.cuda_stream)))
        _all_reduce(out)
        spectrum = out.cpu().numpy()
        if spectrum[top + 1] or int(spectrum[top + 4]) != S:
            raise RuntimeError("panel multiplicities: the spectrum's second pass disagrees with its first")
    cand = mult_order_decode(h["mult_top"]) if top_keep else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    return ShardedPanelDistribution(S, distinct, spectrum[:top + 1].copy(), sq, o_first[:owned].clone(),
                                    o_mult[:owned].clone(), cand, top_keep)


def legacy_panel_distribution_distributed(instance, iterations, random_seed, keep_panels=True, chunk=None,
                                          top_keep=64, timings=None):
    """analysis.legacy_panel_distribution with the panels sharded over the ranks of the default group:
    returns ``(alloc, found_panels, pair_histogram, panel_distribution)`` on every rank, the first three
    equal, bit for bit, to what ``legacy_probabilities_distributed`` returns (the same body runs).

    ``panel_distribution`` (a stats.ShardedPanelDistribution with an exchange -- more than one rank, or
    CSA_FORCE_EXCHANGE=1 -- a stats.PanelDistribution over the device list otherwise) describes the WHOLE
    job on every rank: S, distinct, spectrum, sum_squares, max_multiplicity and the estimators.  Each
    rank counts its share once (csa_unique_mult_async), the counts travel with the exchange's keys (32
    bytes: h1, h2, global first index, multiplicity) to the hash's owner, which merges them exactly
    (csa_merge_mult_keys_async); the owners' spectra are summed in the call's all_reduce and each owner's
    ``top_keep`` most frequent entries are gathered, all inside the call and its one host copy.
    ``owned()`` is this rank's owner list; ``top(m)`` for m <= ``top_keep`` re-draws m panels by index on
    this rank, alone; ``multiplicities()``, ``count()``, a longer ``top`` and pickling re-draw the job's
    panels on this rank (distributed.PanelRedraw, as found_panels) and count them there -- no collective.
    ``top_keep=0`` gathers nothing.  With ``keep_panels=False`` the estimators work and those raise.
    Philox mode only: MT-mode runs are not sharded.  S < 2^32."""
    return legacy_probabilities_distributed(instance, iterations, random_seed, keep_panels=keep_panels, chunk=chunk,
                                            timings=timings, multiplicity=True, top_keep=top_keep)
