"""The compiled condition rules' field chains on the CPU (rules and resources: cond_preload_cases.py): what the oracle
says about the crafted pairs (computed once, shared with test_gpu_cond_preload.py), the CPU engine against it, and
what KYV_JC_PRELOAD does to the generated source."""
import collections
import functools
import hashlib
import re

import cases
import cond_preload_cases as M
import parity_util as PU
from kyverno_amd import engine as E

@functools.lru_cache(maxsize=None)
def oracle():
    docs, nsl = M.corpus()
    return PU.oracle_pairs(M.policies(), docs, nsl)


def rule_counts(ora):
    n = collections.defaultdict(collections.Counter)
    for (pol, rule, ri), rr in ora.items():
        n[(pol, rule)][rr["status"]] += 1
        n[(pol, rule)]["nd"] += bool(rr.get("nondeterministic"))
    return n


def test_corpus_is_not_vacuous():
    """the oracle decides every pair (none nondeterministic, none unsupported); every rule passes and fails, and skips
    where it can (M.can_skip: it has a precondition or is a foreach; the two plain denies without preconditions decide
    every resource they match, so no input makes them skip); the batch is several waves per kind with mixed
    neighbours"""
    docs, _ = M.corpus()
    n = rule_counts(oracle())
    assert len(n) == 24, sorted(n)  # 8 rules, each with its workload and CronJob form
    for key, c in n.items():
        assert c["nd"] == 0 and c["unsupported"] == 0, (key, c)
        assert c["pass"] > 0 and c["fail"] > 0, (key, c)
        if M.can_skip(key[1]):
            assert c["skip"] > 0, (key, c)
    assert sum(not M.can_skip(key[1]) for key in n) == 6  # adding-capabilities, restricted-volumes and their forms
    kinds = collections.Counter(d["kind"] for d in docs)
    assert all(kinds[k] > 64 and kinds[k] % 64 for k in ("Pod", "Deployment", "CronJob")), kinds


def test_every_rule_is_a_compiled_condition_rule():
    rs = E.Ruleset(M.policies())
    src = rs.jit_source()[0]
    for k, r in enumerate(rs.rules):
        assert r["kind"] in ("deny", "foreach") and ("jr%d(" % k) in src, r


def test_cpu_backend_parity():
    docs, nsl = M.corpus()
    st, _ = PU.compare(M.policies(), docs, nsl, backend="cpu")
    assert st["nbad"] == 0, st["bad"]
    assert st["compared"] > 2500 and st["nd"] == 0


# ---------------------------------------------------------------- generated source
def source(pols):
    return E.Ruleset(pols).jit_source()[0]


def c3_policies():
    return cases.best_practices() + cases.chart_restricted()


def test_switch_off_restores_the_source(monkeypatch):
    """KYV_JC_PRELOAD=0: the source of the C3 ruleset is, byte for byte, what the commit before the chains generated
    (its size and hash, recorded from that commit: golden/cond_preload_parent_source.json). A later change to what
    jit.cpp emits for this ruleset records them again from its own parent or drops that one assertion; the structural
    assertions are the ones that last."""
    monkeypatch.delenv("KYV_JC_PRELOAD", raising=False)
    monkeypatch.delenv("KYV_META_KEYS", raising=False)
    on = source(c3_policies())
    monkeypatch.setenv("KYV_JC_PRELOAD", "0")
    off = source(c3_policies())
    parent = cases.load("cond_preload_parent_source.json")
    assert len(off.encode()) == parent["bytes"] and hashlib.sha256(off.encode()).hexdigest() == parent["sha256"]
    assert "jc_field_e(" not in off and "jc_field_e(" in on
    monkeypatch.delenv("KYV_JC_PRELOAD")
    assert source(c3_policies()) == on


def cond_part(src):
    """the condition rules' functions of a generated source"""
    lo = src.index("jc_match(const View& v")
    hi = src.rindex("static __device__ __forceinline__ uint8_t jr")
    return src[lo:src.index("\n}\n", hi)]


COLUMN_FIELD = r"jc_field\(v, R, \w+, \w+, (\d+)u,"  # a field read through its column in place


def test_chains_read_their_last_step_only(monkeypatch):
    """with the chains, no field of a condition function reads its own column step by step: each chain is one
    jc_field_e on its last step's column, with the walk by node index in its cold block, and the columns read are a
    subset of the ones read before -- the intermediate steps (spec below the root; securityContext and capabilities
    below a container) are gone"""
    monkeypatch.delenv("KYV_JC_PRELOAD", raising=False)
    on = cond_part(source(c3_policies()))
    monkeypatch.setenv("KYV_JC_PRELOAD", "0")
    off = cond_part(source(c3_policies()))
    assert not re.search(COLUMN_FIELD, on)
    before = re.findall(COLUMN_FIELD, off)
    after = re.findall(r"jc_field_e\(jc_col\(v, (\d+)u,", on)
    assert after and set(after) < set(before)
    assert len(after) < len(before) * 0.6, (len(after), len(before))
    # every chain keeps its fallback: as many cold steps (by node index, no row, no column) as there were column steps
    assert len(re.findall(r"    jc_field\(v, R, \w+, NONE, NONE, \d+u,", on)) == len(before)
    # everything but the fields is as before
    for call in ("jc_arr(v, R", "jc_elem(v, R"):
        assert on.count(call) == off.count(call)


def test_switch_and_compile_for_gfx950(monkeypatch):
    """the crafted ruleset's source follows the switch, and the default source of a policy with streamed foreach lists
    and element programs compiles for gfx950"""
    srcs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("KYV_JC_PRELOAD", mode)
        srcs[mode] = source(M.policies())
    assert srcs["0"] != srcs["1"] and "jc_field_e(" in srcs["1"] and "jc_field_e(" not in srcs["0"]
    monkeypatch.delenv("KYV_JC_PRELOAD")
    monkeypatch.setenv("KYV_JIT_CACHE", "0")  # compile for real; keep the in-tree code-object cache untouched
    assert source(M.policies()) == srcs["1"]
    monkeypatch.setenv("KYV_META_KEYS", "0")  # stands for the source of before the plane: no chains unless asked for
    assert source(M.policies()) == srcs["0"]
    monkeypatch.delenv("KYV_META_KEYS")
    strict = [p for p in M.policies() if p["metadata"]["name"] == "disallow-capabilities-strict"]
    secs, size = E.Ruleset(strict).jit_compile()
    assert size > 1000
