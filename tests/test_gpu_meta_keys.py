"""GPU side of the meta-key plane tests (corpus, rulesets, model: meta_keys_cases.py; the oracle's results, computed
once: test_meta_keys.py): the compiled walk with the plane, the compiled walk without it (KYV_META_KEYS=0) and the
interpreted kernels, each pair by pair against the oracle; the plane the device filled against the host's."""
import numpy as np
import pytest

import meta_keys_cases as M
import parity_util as PU
import table_edge_cases as T
import test_meta_keys as C
from kyverno_amd import _lib as K
from kyverno_amd import engine as E

pytestmark = pytest.mark.gpu
RUNS = {"plane": (True, None), "no-plane": (True, "0"), "interpreter": (False, None)}


def run(name, mode, monkeypatch):
    """one parity run of ruleset `name`: every pair against the oracle (PU.compare leaves out nothing but both-sides-ND
    pairs), failing paths and messages included"""
    jit, switch = RUNS[mode]
    if switch is not None:
        monkeypatch.setenv("KYV_META_KEYS", switch)
    else:
        monkeypatch.delenv("KYV_META_KEYS", raising=False)
    docs, nsl, _ = M.corpus()
    ora = C.oracle(name)
    monkeypatch.setattr(PU, "oracle_pairs", lambda *a, **k: ora)
    st, res = PU.compare(M.ruleset(name), docs, nsl, backend="gpu", jit=jit)
    assert bool(res.jit) == jit
    return st, res, ora


@pytest.mark.parametrize("mode", list(RUNS))
@pytest.mark.parametrize("name", list(M.RULESETS))
def test_parity(name, mode, monkeypatch):
    st, res, ora = run(name, mode, monkeypatch)
    assert st["nbad"] == 0, st["bad"]
    assert st["compared"] > 20 and st["messages"] >= 20, st
    # the pairs the oracle calls nondeterministic are ST_ND on the device (but for a rule the compiler leaves to the CPU
    # engine as a whole: each of its pairs is ST_FALLBACK)
    rs = res.ruleset
    nd = 0
    for (pol, rule, ri), rr in ora.items():
        if rr.get("nondeterministic"):
            k = [i for i, r in enumerate(rs.rules) if r["name"] == rule and rs.policies[r["policy"]]["name"] == pol][0]
            if rs.rules[k]["kind"] == "fallback":
                assert int(res.status[k, ri]) == K.ST_FALLBACK, (pol, rule, ri)
                continue
            assert int(res.status[k, ri]) == K.ST_ND, (pol, rule, ri)
            nd += 1
    assert nd == st["nd"] and nd >= 1
    # the plane: filled by the run that reads it, byte for byte the host's; no plane otherwise
    host = res.batch.meta_keys()
    if mode == "plane" and host["classes"]:
        dev = res.batch.meta_keys(device=0)
        assert dev["rows"].shape == host["rows"].shape and dev["rows"].tobytes() == host["rows"].tobytes()
        assert dev["decoded"] == host["decoded"]
        assert res.batch.stats()["device_bytes"] >= 16 * len(host["classes"]) * res.batch.n
    else:
        if host["classes"]:
            with pytest.raises(K.KyvError):
                res.batch.meta_keys(device=0)
        assert res.meta_keys_ms == 0


@pytest.mark.parametrize("name", list(M.RULESETS))
def test_accounting_build_same_verdicts(name, monkeypatch):
    monkeypatch.delenv("KYV_META_KEYS", raising=False)
    docs, nsl, _ = M.corpus()
    rs = E.Ruleset(M.ruleset(name))
    b = E.Batch(rs, docs, nsl)
    prod = E.evaluate(rs, b, backend="gpu", jit=True)
    acct = E.evaluate(rs, b, backend="gpu", jit=True, account_bytes=True)
    assert prod.jit and acct.jit
    assert np.array_equal(prod.raw, acct.raw) and prod.counts == acct.counts
    assert acct.alg_bytes_phase["walk"] > 0


def test_plane_is_per_batch_not_per_slice(monkeypatch):
    """the C3 ruleset cut into rule slices (KYV_SLICE_MB=1, as test_gpu_table_edges.py forces them): one plane serves
    every slice, equal to the host's, and the verdicts and failing-path records equal the unsliced run's"""
    monkeypatch.delenv("KYV_META_KEYS", raising=False)
    docs, nsl = T.slice_corpus()
    rs = E.Ruleset(T.slice_policies())
    monkeypatch.delenv("KYV_SLICE_MB", raising=False)
    one = E.evaluate(rs, E.Batch(rs, docs, nsl), jit=True)
    monkeypatch.setenv("KYV_SLICE_MB", "1")
    b = E.Batch(rs, docs, nsl)
    cut = E.evaluate(rs, b, jit=True)
    assert one.jit and cut.jit and len(one.plan()["slices"]) == 1 and len(cut.plan()["slices"]) >= 3
    host, dev = b.meta_keys(), b.meta_keys(device=0)
    assert len(host["classes"]) == 3 and dev["rows"].tobytes() == host["rows"].tobytes()
    assert np.array_equal(one.raw, cut.raw) and np.array_equal(one.rule_counts, cut.rule_counts)
    key = lambda f: (int(f["res"]), int(f["rule"]), int(f["alt"]), int(f["path_template"]), tuple(map(int, f["idx"])),
                     tuple(map(int, f["key"])))
    assert sorted(map(key, one.failures())) == sorted(map(key, cut.failures()))
    again = E.evaluate(rs, b, jit=True)
    assert again.meta_keys_ms == cut.meta_keys_ms > 0  # filled once per batch and device, not per evaluation
