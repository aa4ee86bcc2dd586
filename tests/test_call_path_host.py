"""The Python call path's shared pieces, without a device: the one-copy helpers of device.py on CPU
tensors, DevicePipeline.bound on a bare object, _native.raise_status and distributed._decode_status
against the loaded library (csa_status_decode is host code), and the two composition histograms
rebuilt from the attribute dicts old pickles hold."""
import itertools

import numpy as np
import pytest
import torch

from conftest import pkg

FULL = 0xFFFFFFFF


def _status(words):
    """int32[4] as the device holds it: words above 2^31 are negative there."""
    return torch.from_numpy(np.array(words, np.uint32).view(np.int32).copy())


def test_host_fields_every_order_and_sign_extended_status():
    """Fields of lengths n, 3, 1, 0 and 0 (an empty group table, G = 0, and an empty multiplicity block) in
    every order; the status block's panel words are 0xFFFFFFFF: negative as int32, sign-extended when
    widened, and back as the same uint32[4]."""
    Dv = pkg("device")
    n = 7
    values = {"counts": torch.arange(1, n + 1, dtype=torch.int64) * -3, "stats": torch.tensor([2 ** 40, 5, 0]),
              "unique": torch.tensor([2 ** 62]), "hist": torch.zeros(0, dtype=torch.int64),
              "mult": torch.zeros(0, dtype=torch.int64)}
    words = [5, FULL, FULL, 0]
    pipe = object.__new__(Dv.DevicePipeline)
    pipe.status = status = _status(words)
    assert status.tolist() == [5, -1, -1, 0] and status.to(torch.int64).tolist() == [5, -1, -1, 0]
    for order in itertools.permutations(values):
        h, st = pipe.host_fields([(name, values[name]) for name in order])
        assert h.dtype.names == order + ("status",)
        for name in order:
            assert h[name].dtype == np.int64 and h[name].tolist() == values[name].tolist(), (order, name)
        assert st.dtype == np.uint32 and st.tolist() == words, order
    pipe.status = _status([0, 0, 0, 0])
    h, st = pipe.host_fields([])
    assert h.dtype.names == ("status",) and st.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype", [torch.int64, torch.float64])
@pytest.mark.parametrize("sizes", [(4, 6), (1, 0), (0, 1), (5,)])
def test_status_block_views_and_read_back(dtype, sizes):
    """StatusBlock: what is written through the named views and the int32 status view comes back under
    the same names, for tables of either element type, an empty field in either place, and a status
    whose panel words are 0xFFFFFFFF."""
    Dv = pkg("device")
    names = ["alloc", "table"][:len(sizes)]
    blk = Dv.StatusBlock(list(zip(names, sizes)), dtype, "cpu")
    assert blk.status.dtype == torch.int32 and blk.status.tolist() == [0, 0, 0, 0]     # zeroed on creation
    for i, name in enumerate(names):
        assert blk.views[name].numel() == sizes[i]
        blk.views[name].copy_(torch.arange(sizes[i]).to(dtype) + 10 * (i + 1))
    blk.status.copy_(_status([1, FULL, FULL, 0]))
    h, words = blk.host()
    for i, name in enumerate(names):
        assert h[name].tolist() == [10 * (i + 1) + j for j in range(sizes[i])]
    assert words.dtype == np.uint32 and words.tolist() == [1, FULL, FULL, 0]
    # without a status block: the fields alone, no words
    bare = Dv.StatusBlock([("alloc", 3)], dtype, "cpu", status=False)
    bare.views["alloc"].fill_(2)
    h, words = bare.host()
    assert bare.status is None and words is None and h["alloc"].tolist() == [2, 2, 2] and bare.out.numel() == 3
    # zero=True: the fields are zeroed too
    z = Dv.StatusBlock([("table", 5)], dtype, "cpu", zero=True)
    assert z.out.tolist() == [0] * 7


def _bare_pipeline():
    Dv = pkg("device")
    pipe = object.__new__(Dv.DevicePipeline)
    pipe.panels, pipe.hashes, pipe.xt, pipe.pairs, pipe.counts = "P", "H", "X", "PR", "C"
    return pipe


def _buffers(pipe):
    return pipe.panels, pipe.hashes, pipe.xt, pipe.pairs, pipe.counts


def test_bound_rebinds_and_restores():
    pipe = _bare_pipeline()
    with pipe.bound(panels="p1", counts="c1") as same:
        assert same is pipe and _buffers(pipe) == ("p1", "H", "X", "PR", "c1")
        pipe.panels = "chunk"                 # the stages go on assigning inside the block
    assert _buffers(pipe) == ("P", "H", "X", "PR", "C")
    with pipe.bound():
        pass
    assert _buffers(pipe) == ("P", "H", "X", "PR", "C")


def test_bound_restores_after_exception():
    pipe = _bare_pipeline()
    with pytest.raises(ZeroDivisionError):
        with pipe.bound(panels="p1", hashes="h1", xt="x1", pairs="pr1", counts="c1"):
            pipe.hashes = "chunk"
            1 / 0
    assert _buffers(pipe) == ("P", "H", "X", "PR", "C")


def test_bound_nests():
    pipe = _bare_pipeline()
    with pipe.bound(counts="c1", pairs="pr1"):
        with pipe.bound(panels="p2", pairs="pr2"):
            assert _buffers(pipe) == ("p2", "H", "X", "pr2", "c1")
            with pytest.raises(KeyError):
                with pipe.bound(panels="p3", counts="c3"):
                    raise KeyError("")
            assert _buffers(pipe) == ("p2", "H", "X", "pr2", "c1")
        assert _buffers(pipe) == ("P", "H", "X", "pr1", "c1")
    assert _buffers(pipe) == ("P", "H", "X", "PR", "C")


def test_bound_rejects_unknown_buffer():
    pipe = _bare_pipeline()
    pipe.status = "S"
    with pytest.raises(TypeError, match="status"):
        with pipe.bound(panels="p1", status="s1"):
            pass
    assert _buffers(pipe) == ("P", "H", "X", "PR", "C") and pipe.status == "S"     # nothing was rebound


def test_raise_status_codes():
    N = pkg("_native")
    N.lib()
    assert N.raise_status(np.zeros(4, np.uint32)) is None
    assert N.raise_status(np.array([0, FULL, FULL, 7], np.uint32)) is None          # only the code word counts
    with pytest.raises(KeyError) as e:
        N.raise_status(np.array([N.CSA_E_NO_CANDIDATE, 12, 0, 0], np.uint32))
    assert e.value.args == ("",)                                                    # legacy.py:188
    with pytest.raises(N.CsaError) as e:
        N.raise_status(np.array([N.CSA_E_ATTEMPT_LIMIT, 17, 1, 0], np.uint32))
    assert e.value.code == N.CSA_E_ATTEMPT_LIMIT and "panel %d" % (17 + (1 << 32)) in str(e.value)
    for low, text in ((FULL - 1, "owner segment"), (FULL, "LDS table")):            # the exchange's, the dedupe's
        with pytest.raises(N.CsaError) as e:
            N.raise_status(np.array([N.CSA_E_UNSUPPORTED, low, FULL, 0], np.uint32))
        assert e.value.code == N.CSA_E_UNSUPPORTED and text in str(e.value)
    # a non-contiguous view of a longer host copy is read as its own four words
    tail = np.array([9, 9, N.CSA_E_ATTEMPT_LIMIT, 9, 3, 9, 0, 9, 0, 9], np.uint32)[2::2]
    with pytest.raises(N.CsaError) as e:
        N.raise_status(tail)
    assert e.value.code == N.CSA_E_ATTEMPT_LIMIT and "panel 3:" in str(e.value)


def test_decode_status_raises_the_agreed_code():
    N, Dd = pkg("_native"), pkg("distributed")
    clean = np.zeros(4, np.uint32)
    with pytest.raises(KeyError):                          # own block clean, the ranks agreed on a missing candidate
        Dd._decode_status(clean, N.CSA_E_NO_CANDIDATE)
    with pytest.raises(N.CsaError) as e:
        Dd._decode_status(clean, N.CSA_E_ATTEMPT_LIMIT)
    assert e.value.code == N.CSA_E_ATTEMPT_LIMIT
    own = np.array([N.CSA_E_UNSUPPORTED, FULL - 1, FULL, 0], np.uint32)      # own block: the exchange's overflow
    with pytest.raises(KeyError):
        Dd._decode_status(own, N.CSA_E_NO_CANDIDATE)
    with pytest.raises(N.CsaError) as e:
        Dd._decode_status(own, N.CSA_E_ATTEMPT_LIMIT)
    assert e.value.code == N.CSA_E_ATTEMPT_LIMIT
    with pytest.raises(N.CsaError) as e:                   # own block holds the agreed code: its panel is named
        Dd._decode_status(np.array([N.CSA_E_ATTEMPT_LIMIT, 41, 0, 0], np.uint32), N.CSA_E_ATTEMPT_LIMIT)
    assert e.value.code == N.CSA_E_ATTEMPT_LIMIT and "panel 41:" in str(e.value)
    assert Dd._decode_status(clean, 0) is None


DERIVED = ("probabilities", "mean", "panel_share", "variance", "prob_absent")


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_rebuilt(cls, fresh, state, table, norm, index_dtype):
    """An object made as pickle makes it from a parent-shaped attribute dict gives every derived array
    of a freshly constructed one, and those are the parent's expressions bit for bit."""
    old = cls.__new__(cls)
    old.__dict__.update(state)
    assert len(old) == len(fresh) == len(state["labels"])
    for name in DERIVED:
        _same(getattr(old, name)(), getattr(fresh, name)())
    for a, b in zip(old.support(), fresh.support()):
        _same(a, b)
    k = state["k"]
    mean = (table * np.arange(k + 1, dtype=index_dtype)).sum(axis=1) / norm
    d = np.arange(k + 1, dtype=np.float64)[None, :] - mean[:, None]
    _same(fresh.probabilities(), table / norm)
    _same(fresh.mean(), mean)
    _same(fresh.panel_share(), mean / k)
    _same(fresh.variance(), (table * d * d).sum(axis=1) / norm)
    _same(fresh.prob_absent(), table[:, 0] / norm)
    nz = table != 0
    lo, hi = fresh.support()
    assert lo.tolist() == [int(np.flatnonzero(r)[0]) if r.any() else -1 for r in nz]
    assert hi.tolist() == [int(np.flatnonzero(r)[-1]) if r.any() else -1 for r in nz]


def test_composition_histogram_from_old_attribute_dict():
    St = pkg("stats")
    rng = np.random.default_rng(11)
    k, G = 6, 5
    counts = rng.integers(0, 2 ** 40, size=(G, k + 1)).astype(np.int64)
    counts[1] = 0                                  # an empty group: support (-1, -1)
    counts[2, :3] = 0
    S = int(counts[0].sum())
    labels = [("c", "f%d" % g) for g in range(G)]
    fresh = St.CompositionHistogram(labels, counts, S, k)
    _check_rebuilt(St.CompositionHistogram, fresh, {"labels": labels, "counts": counts.copy(), "S": S, "k": k}, counts,
                   S, np.int64)
    merged = fresh + fresh
    assert isinstance(merged, St.CompositionHistogram) and merged.S == 2 * S and (merged.counts == 2 * counts).all()


def test_weighted_composition_histogram_from_old_attribute_dict():
    St = pkg("stats")
    rng = np.random.default_rng(12)
    k, G, P = 4, 6, 33
    values = rng.random((G, k + 1))
    values[3] = 0.0
    values[4, 2:] = 0.0
    total = float(values[0].sum())
    labels = list(range(G))
    fresh = St.WeightedCompositionHistogram(labels, values, total, P, k)
    state = {"labels": labels, "values": values.copy(), "total": total, "P": P, "k": k}
    _check_rebuilt(St.WeightedCompositionHistogram, fresh, state, values, total, np.float64)
    diff = St.composition_difference(fresh, fresh)
    assert not diff["total_variation"].any() and not diff["mean"].any()
