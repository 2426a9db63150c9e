"""GPU side of the column-facts tests (rules and resources: col_facts_cases.py; the oracle's results, computed once:
test_col_facts.py): the compiled walk and condition kernels with the facts, with the batch reporting nothing
(KYV_FACT_COLS=0), with the generator switch off (KYV_JIT_COLFACTS=0) and the interpreted kernels, each pair by pair
against the oracle -- verdicts, failing paths and messages; the accounting build's verdicts and its counted walk and
condition bytes with and without the facts."""
import functools
import os

import numpy as np
import pytest

import col_facts_cases as M
import parity_util as PU
import test_col_facts as C
from kyverno_amd import engine as E

pytestmark = pytest.mark.gpu
# mode -> (compiled kernels?, environment of the run)
RUNS = {"facts": (True, {}), "facts-masked": (True, {"KYV_FACT_COLS": "0"}), "generator-off": (True, {"KYV_JIT_COLFACTS": "0"}),
        "interpreter": (False, {})}
SWITCHES = ("KYV_FACT_COLS", "KYV_JIT_COLFACTS")


class switches:
    """the environment switches for the evaluations inside (read per evaluation / where the source is generated)"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in SWITCHES:
            os.environ.pop(k, None)
            if self.old[k] is not None:
                os.environ[k] = self.old[k]


@functools.lru_cache(maxsize=None)
def run(mode):
    jit, env = RUNS[mode]
    docs, nsl = M.parity_corpus()
    ora = C.oracle()
    saved = PU.oracle_pairs
    PU.oracle_pairs = lambda *a, **k: ora
    try:
        with switches(env):
            st, res = PU.compare(M.parity_policies(), docs, nsl, backend="gpu", jit=jit)
    finally:
        PU.oracle_pairs = saved
    assert bool(res.jit) == jit
    return st, res


@pytest.mark.parametrize("mode", list(RUNS))
def test_parity(mode):
    st, res = run(mode)
    assert st["nbad"] == 0, st["bad"]
    # no pair is left out: the oracle decides every one (test_col_facts.test_parity_corpus_is_decided_by_the_oracle)
    assert st["nd"] == 0 and st["compared"] > 5000 and st["messages"] > 2000, st


def test_same_verdict_bytes():
    """the verdict bytes, marks included, are equal whatever the facts say and whether the source reads them"""
    on, masked, off = (np.asarray(run(m)[1].raw) for m in ("facts", "facts-masked", "generator-off"))
    assert np.array_equal(on, masked) and np.array_equal(on, off)


def account(docs, env):
    with switches(env):
        rs = E.Ruleset(M.parity_policies())
        b = E.Batch(rs, docs)
        prod = E.evaluate(rs, b, backend="gpu", jit=True)
        acct = E.evaluate(rs, b, backend="gpu", jit=True, account_bytes=True)
    assert acct.jit and np.array_equal(np.asarray(acct.raw), np.asarray(prod.raw))
    return acct.alg_bytes_phase


def test_accounting_counts_what_is_issued():
    """the accounting build's verdicts equal the product's; on a batch without init, ephemeral or port lists the walk
    and the condition phase read fewer counted bytes with the facts than with KYV_FACT_COLS=0; on a batch whose every
    wave holds every list and a malformed step they read no more"""
    plain = {m: account(M.plain_batch(), env) for m, env in (("facts", {}), ("masked", {"KYV_FACT_COLS": "0"}))}
    dense = {m: account(M.dense_batch(), env) for m, env in (("facts", {}), ("masked", {"KYV_FACT_COLS": "0"}))}
    print("plain:", plain, "dense:", dense)
    for phase in ("walk", "cond"):
        assert 0 < plain["facts"][phase] < plain["masked"][phase], (phase, plain)
        assert 0 < dense["facts"][phase] <= dense["masked"][phase], (phase, dense)
