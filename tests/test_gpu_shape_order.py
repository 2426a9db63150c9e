"""The order within a kind (batch.cpp shape_keys) changes nothing the caller sees, on the MI355X with the bench policy
set and the runtime-compiled kernels: a batch built with the order on and the same batch built with KYV_SHAPE_ORDER=0
give equal verdict matrices in input order, equal per-rule counts and equal failing-path rows, and both equal the
oracle's verdicts, paths and messages."""
import numpy as np
import pytest

import bench
import parity_util as PU
import shape_order_cases as C
from kyverno_amd import synth

pytestmark = pytest.mark.gpu


def batches():
    mixed, nsl = synth.mixed(130, edge=True)
    big = mixed + C.extremes()
    return {"mixed+extremes": (big, nsl), "one": (mixed[:1], nsl), "wave+1": (mixed[:65], nsl)}


def evaluate(docs, nsl, backend="gpu"):
    st, res = PU.compare(bench.load_policies("c3"), docs, nsl, backend=backend, **({"jit": True} if backend == "gpu" else {}))
    assert st["nbad"] == 0, st["bad"]
    assert st["compared"] > 0
    return st, res


def sorted_failures(res):
    f = res.failures()
    return f[np.lexsort((f["key"][:, 1], f["key"][:, 0], f["idx"][:, 3], f["idx"][:, 2], f["idx"][:, 1], f["idx"][:, 0],
                         f["path_template"], f["alt"], f["rule"], f["res"]))]


@pytest.mark.parametrize("name", ["mixed+extremes", "one", "wave+1"])
def test_order_on_and_off_agree_and_match_oracle(name, monkeypatch, backend="gpu"):
    docs, nsl = batches()[name]
    monkeypatch.setenv("KYV_SHAPE_ORDER", "0")
    st_off, off = evaluate(docs, nsl, backend)
    assert not off.batch.wave_facts()["shape_ordered"]
    monkeypatch.delenv("KYV_SHAPE_ORDER")
    st_on, on = evaluate(docs, nsl, backend)
    f = on.batch.wave_facts()
    assert f["shape_ordered"]
    if name == "mixed+extremes":
        assert not np.array_equal(f["order"], off.batch.wave_facts()["order"])  # the two orders do differ
    if backend == "gpu":
        assert on.jit and off.jit
    assert np.array_equal(on.raw, off.raw)
    assert np.array_equal(on.rule_counts, off.rule_counts) and on.counts == off.counts
    assert np.array_equal(sorted_failures(on), sorted_failures(off))
    assert st_on["compared"] == st_off["compared"] and st_on["messages"] == st_off["messages"]
