"""The per-rule verdict totals at the histogram's edges (cases: result_edge_cases.py): rows that start at every
alignment modulo 16, rows shorter than one 16-byte load, every status the device writes (marks in the high bits
included), and rows of one status long enough for several trips per thread -- with the round-12 kernel and with round 11's
(KYV_RESULT_KERNELS=0). The totals are compared with numpy.bincount over the verdict bytes the evaluation left on the
device and with the CPU backend's totals."""
import functools

import numpy as np
import pytest

import result_edge_cases as R
from kyverno_amd import _lib as K
from kyverno_amd import engine as E

pytestmark = pytest.mark.gpu
KERNELS = pytest.mark.parametrize("kernels", [None, "0"], ids=["planes", "round11"])


def _switch(monkeypatch, kernels):
    if kernels is None:
        monkeypatch.delenv("KYV_RESULT_KERNELS", raising=False)
    else:
        monkeypatch.setenv("KYV_RESULT_KERNELS", kernels)


def _bincount(status):
    return np.stack([np.bincount(row & 7, minlength=8) for row in status])


@functools.lru_cache(maxsize=None)
def hist_case(n):
    rs = E.Ruleset(R.hist_policies())
    docs = R.hist_corpus(n)
    return rs, docs, E.evaluate(rs, E.Batch(rs, docs), backend="cpu")


@KERNELS
@pytest.mark.parametrize("n", R.HIST_SIZES)
def test_rule_totals(n, kernels, monkeypatch):
    _switch(monkeypatch, kernels)
    rs, docs, cpu = hist_case(n)
    assert len(rs.rules) == R.HIST_RULES and rs.rules[3]["kind"] == "fallback"
    b = E.Batch(rs, docs)
    res = E.evaluate(rs, b, jit=False, copy_back=False)
    want = _bincount(b.resident_status())
    assert want.sum() == 5 * n
    assert np.array_equal(res.rule_counts, want)
    assert np.array_equal(res.rule_counts, cpu.rule_counts)
    assert res.counts == {K.STATUS_NAMES[s]: int(want[:, s].sum()) for s in range(8)}
    if n >= 31:  # every status of the case is there, and the skips carry the precondition mark in the high bits
        for s in (K.ST_NONE, K.ST_PASS, K.ST_FAIL, K.ST_SKIP, K.ST_ERROR, K.ST_FALLBACK):
            assert want[:, s].sum() > 0, (s, want)
        raw = E.evaluate(rs, b, jit=False).raw
        skips = raw[(raw & 7) == K.ST_SKIP]
        assert len(skips) and (skips >> 3 == 30).all()
        assert np.array_equal(_bincount(raw), want)


def test_rows_start_at_every_alignment():
    assert {(k * n) % 16 for n in R.HIST_SIZES for k in range(R.HIST_RULES)} == set(range(16))
    assert len(R.hist_policies()[0]["spec"]["rules"]) == R.HIST_RULES


@functools.lru_cache(maxsize=None)
def long_batch():
    rs = E.Ruleset(R.one_status_policies())
    return rs, E.Batch(rs, R.one_status_corpus(R.LONG_N))


@KERNELS
def test_long_one_status_rows(kernels, monkeypatch):
    """Rows of one status (PASS, FAIL, 30 x NONE) long enough that a thread makes several trips through the
    two-loads-in-flight loop. The length comes from the launch (result_edge_cases.long_row_trips): a row gets
    ceil(CUs x 8 / rules) blocks of 256 threads, so with 32 rules and 2,000,003 bytes a thread loads 7.6 times on 256
    CUs and 3.8 times on a chip of 512; the odd length starts rows at odd addresses. The bit-plane kernel tallies in
    32 bits per thread (population counts), so it has no byte fields and no flush interval: what a long row can break
    is the loop's stride and its remainder"""
    _switch(monkeypatch, kernels)
    monkeypatch.delenv("KYV_HIST", raising=False)
    assert R.long_row_trips() > 3.5 and R.long_row_trips(cus=256) > 7
    n = R.LONG_N
    rs, b = long_batch()
    assert b.n == n and len(rs.rules) == R.LONG_RULES
    res = E.evaluate(rs, b, jit=False, copy_back=False)
    want = np.zeros((R.LONG_RULES, 8), dtype=np.int64)
    want[:, K.ST_NONE] = n
    want[0] = want[1] = 0
    want[0, K.ST_PASS] = want[1, K.ST_FAIL] = n
    assert np.array_equal(res.rule_counts, want)
    st = b.resident_status()
    assert (st[0] == K.ST_PASS).all() and (st[1] == K.ST_FAIL).all() and not st[2:].any()
