"""GPU side of the field-chain tests (rules and resources: cond_preload_cases.py; the oracle's results, computed
once: test_cond_preload.py): the compiled condition kernels with the chains, without them (KYV_JC_PRELOAD=0) and the
interpreted kernels, each pair by pair against the oracle; the accounting build's condition-phase bytes with and
without the chains."""
import collections
import functools
import os

import numpy as np
import pytest

import cond_preload_cases as M
import parity_util as PU
import test_cond_preload as C
from kyverno_amd import _lib as K
from kyverno_amd import engine as E

pytestmark = pytest.mark.gpu
RUNS = {"preload": (True, None), "no-preload": (True, "0"), "interpreter": (False, None)}


class switch:
    """KYV_JC_PRELOAD for the evaluations inside (read where the source is generated)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("KYV_JC_PRELOAD", None)
        if self.value is not None:
            os.environ["KYV_JC_PRELOAD"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("KYV_JC_PRELOAD", None)
        if self.old is not None:
            os.environ["KYV_JC_PRELOAD"] = self.old


@functools.lru_cache(maxsize=None)
def run(mode):
    """one parity run over the crafted batch: every pair against the oracle (PU.compare: status, and the message of
    every pair that has one), -> (stats, results)"""
    jit, value = RUNS[mode]
    docs, nsl = M.corpus()
    ora = C.oracle()
    saved = PU.oracle_pairs
    PU.oracle_pairs = lambda *a, **k: ora
    try:
        with switch(value):
            st, res = PU.compare(M.policies(), docs, nsl, backend="gpu", jit=jit)
    finally:
        PU.oracle_pairs = saved
    assert bool(res.jit) == jit
    return st, res


@pytest.mark.parametrize("mode", list(RUNS))
def test_parity(mode):
    st, res = run(mode)
    assert st["nbad"] == 0, st["bad"]
    assert st["nd"] == 0 and st["compared"] > 2500 and st["messages"] > 2500, st
    # per rule: the device's own PASS, FAIL and SKIP counts are nonzero (SKIP where the rule can skip)
    rs, status = res.ruleset, np.asarray(res.status)
    for k, r in enumerate(rs.rules):
        n = collections.Counter(status[k].tolist())
        assert n[K.ST_PASS] > 0 and n[K.ST_FAIL] > 0, (r["name"], n)
        if M.can_skip(r["name"]):
            assert n[K.ST_SKIP] > 0, (r["name"], n)


def test_same_verdict_bytes():
    """the verdict bytes, marks included: equal with and without the chains; equal to the interpreter's wherever
    neither side leaves the pair to the CPU engine"""
    on, off, interp = (np.asarray(run(m)[1].raw) for m in RUNS)
    assert np.array_equal(on, off)
    both = (on != K.ST_FALLBACK) & (interp != K.ST_FALLBACK)
    assert both.sum() > 2500 and np.array_equal(on[both], interp[both])


def test_accounting_counts_fewer_condition_bytes():
    """the accounting build: same verdicts as the product build either way, and the condition phase reads fewer
    counted bytes with the chains than without (their intermediate steps are not loaded at all)"""
    docs, nsl = M.corpus()
    out = {}
    for mode in ("preload", "no-preload"):
        with switch(RUNS[mode][1]):
            rs = E.Ruleset(M.policies())
            b = E.Batch(rs, docs, nsl)
            acct = E.evaluate(rs, b, backend="gpu", jit=True, account_bytes=True)
        assert acct.jit and np.array_equal(np.asarray(acct.raw), np.asarray(run(mode)[1].raw))
        out[mode] = acct.alg_bytes_phase["cond"]
    print("condition phase bytes:", out)
    assert 0 < out["preload"] < out["no-preload"], out
