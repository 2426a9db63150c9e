"""GPU side of the table-edge parity tests (generators: table_edge_cases.py; shared checks and the oracle's results:
test_table_edges.py): the device code past its glob-mask, match-table and rule-slice capacities, pair by pair against
the oracle. Every test asserts from the evaluation's plan report (Results.plan()) that it ran in the regime it names."""
import functools

import numpy as np
import pytest

import parity_util as PU
import table_edge_cases as T
import test_table_edges as C
from kyverno_amd import _lib as K
from kyverno_amd import engine as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu
JIT = pytest.mark.parametrize("jit", [True, False], ids=["compiled", "interpreter"])


# ---------------------------------------------------------------- 3a: wildcard semantics at every mask position
@JIT
@pytest.mark.parametrize("rung", T.vector_rungs(), ids=lambda r: r[0])
def test_wildcard_routes_gpu(rung, jit):
    plans = C.check_rung(rung, "gpu", jit)
    C.check_rung_plan(rung, plans)
    for p in plans:
        assert len(p["slices"]) == 1, p


# ---------------------------------------------------------------- label selectors and Go map order
@pytest.mark.parametrize("variant", C.VARIANTS)
def test_selector_map_order_cases_gpu(variant):
    """the selector cases of test_table_edges.py through each of the device's three match paths, proven from the plan
    report: every rule the device decides is a branch-free record ("facts"), a record that runs its tail ("tail") or a
    rule of the generic match kernel ("generic")"""
    res = C.check_selector_cases(variant, "gpu", jit=False)
    p = res.plan()
    decided = sum(1 for c in C.SELECTOR_CASES if c[5] != "fallback")
    counts = {"facts": p["fasteval_records"], "tail": p["fast_records"] - p["fasteval_records"],
              "generic": p["generic_rules"]}
    assert counts[variant] >= decided, (variant, p)
    for other in set(counts) - {variant}:
        assert counts[other] <= len(C.SELECTOR_CASES) - decided, (variant, p)


# ---------------------------------------------------------------- 3b: match tables past their capacities
CAPS = {"slots": 8, "ns_slots": 4, "wildcards": 16, "annotations": 32, "group_versions": 16}


def check_table_plan(case, p):
    used, cand = p["tail_used"], p["tail_candidates"]
    over = {t for t in CAPS if cand[t] > CAPS[t]}
    for t in CAPS:
        assert used[t] == min(cand[t], CAPS[t]) and cand[t] > 0, (case, t, p)
    if case == "within":
        assert not over and p["onemask"] == 1 and p["gmask_words"] == 1, (case, p)
    elif case == "over":
        assert over == set(CAPS) and p["onemask"] == 0 and p["gmask_words"] >= 2, (case, p)
    else:
        assert over and over != set(CAPS), (case, p)
    # staged records decided from the lane facts, staged records that run their tails, and rules on the generic kernel
    assert p["fasteval_records"] > 0 and p["fast_records"] > p["fasteval_records"] and p["generic_rules"] > 0, (case, p)


@JIT
@pytest.mark.parametrize("case", list(T.VOCAB))
def test_table_cases_gpu(case, jit, monkeypatch):
    pols, docs, nsl, names, m, tx = C.table_case(case)
    monkeypatch.setattr(O, "validate_matrix", lambda *a, **k: (names, m, tx))
    st, res = PU.compare_matrix(pols, docs, nsl, backend="gpu", jit=jit, texts=True)
    assert bool(res.jit) == jit
    assert st["nbad"] == 0, st["bad"]
    assert st["texts"]["fail_pairs"] > 500 and st["texts"]["messages_compared"] > 500, st["texts"]
    check_table_plan(case, res.plan())


@JIT
@pytest.mark.parametrize("case", list(T.VOCAB))
def test_table_cases_partial_wave_gpu(case, jit, monkeypatch):
    """130 resources: kind boundaries inside the two full waves, and a wave of two lanes"""
    pols, docs, nsl, names, m, tx = C.table_case(case, small=True)
    monkeypatch.setattr(O, "validate_matrix", lambda *a, **k: (names, m, tx))
    st, res = PU.compare_matrix(pols, docs, nsl, backend="gpu", jit=jit, texts=True)
    assert bool(res.jit) == jit
    assert st["nbad"] == 0, st["bad"]
    assert st["matched"] > 500, st
    check_table_plan(case, res.plan())


@pytest.mark.parametrize("case", list(T.VOCAB))
def test_table_cases_sliced_gpu(case, monkeypatch):
    """the same evaluation cut into rule slices (KYV_SLICE_MB=1; the slices are laid out by a batch's first evaluation)
    is byte-equal to the unsliced one, failing-path records and per-rule tallies included"""
    pols, docs, nsl = C.table_case(case)[:3]
    rs = E.Ruleset(pols)
    one = E.evaluate(rs, E.Batch(rs, docs, nsl), jit=True)
    assert one.jit and len(one.plan()["slices"]) == 1
    monkeypatch.setenv("KYV_SLICE_MB", "1")
    cut = E.evaluate(rs, E.Batch(rs, docs, nsl), jit=True)
    assert cut.jit
    sl = cut.plan()["slices"]
    assert len(sl) >= 3 and sl[0]["k0"] == 0 and sl[-1]["k1"] == len(rs.rules), sl
    assert all(a["k1"] == b["k0"] for a, b in zip(sl, sl[1:])), sl
    assert np.array_equal(one.raw, cut.raw)
    assert np.array_equal(one.rule_counts, cut.rule_counts)
    assert sorted(map(_frow, one.failures())) == sorted(map(_frow, cut.failures()))
    check_table_plan(case, cut.plan())


def _frow(f):
    return (int(f["res"]), int(f["rule"]), int(f["alt"]), int(f["path_template"]), tuple(int(x) for x in f["idx"]),
            tuple(int(x) for x in f["key"]))


# ---------------------------------------------------------------- 3c: rule slices through the compiled C3 kernels
@functools.lru_cache(maxsize=None)
def slice_runs():
    """the C3 ruleset over 226 match waves, compiled kernels forced: one slice, KYV_SLICE_MB=1 and KYV_SLICE_MB=3 (the
    budget is read when a batch's first evaluation lays its slices out, so each run has a batch of its own)"""
    import os
    pols = T.slice_policies()
    docs, nsl = T.slice_corpus()
    rs = E.Ruleset(pols)
    runs = {}
    saved = os.environ.pop("KYV_SLICE_MB", None)
    try:
        for mb in (None, "1", "3"):
            if mb:
                os.environ["KYV_SLICE_MB"] = mb
            b = E.Batch(rs, docs, nsl)
            runs[mb] = (b, E.evaluate(rs, b, jit=True))
    finally:
        os.environ.pop("KYV_SLICE_MB", None)
        if saved is not None:
            os.environ["KYV_SLICE_MB"] = saved
    return pols, docs, nsl, rs, runs


def test_c3_slice_plans():
    """the regimes, from the plan report: one slice; every walk rule alone at 1 MiB with slice edges on the gate-word
    edges 32 and 64, compiled-condition rules sharing a slice and spread over several; staggered multi-rule slices at
    3 MiB"""
    _, _, _, rs, runs = slice_runs()
    for _, res in runs.values():
        assert res.jit and res.jit_cond
    one = runs[None][1].plan()["slices"]
    assert len(one) == 1 and (one[0]["k0"], one[0]["k1"]) == (0, len(rs.rules)) and len(rs.rules) > 64
    assert one[0]["fused_rules"] > 0 and one[0]["cond_rules"] >= 2
    s1 = runs["1"][1].plan()["slices"]
    edges = {s["k0"] for s in s1} | {s["k1"] for s in s1}
    assert {0, 32, 64, len(rs.rules)} <= edges, s1
    assert all(s["fused_rules"] + s["chunk_rules"] <= 1 for s in s1), s1
    assert any(s["cond_rules"] >= 2 for s in s1), s1
    assert sum(1 for s in s1 if s["cond_rules"]) >= 2, s1
    for key in ("fused_rules", "chunk_rules", "cond_rules"):
        assert sum(s[key] for s in s1) == one[0][key], (key, s1, one)
    s3 = runs["3"][1].plan()["slices"]
    assert 1 < len(s3) < len(s1), (len(s3), len(s1))
    assert any(s["fused_rules"] + s["chunk_rules"] >= 2 for s in s3), s3
    assert any(s["k0"] % 32 and s["k1"] % 32 for s in s3), s3  # edges inside gate words
    for key in ("fused_rules", "chunk_rules", "cond_rules"):
        assert sum(s[key] for s in s3) == one[0][key], (key, s3, one)


def test_c3_one_slice_against_oracle():
    """every verdict, every FAIL path and message of the one-slice run the sliced runs are compared with"""
    pols, docs, nsl, rs, runs = slice_runs()
    st, res = PU.compare_matrix(pols, docs, nsl, backend="gpu", jit=True, texts=True)
    assert res.jit and len(res.plan()["slices"]) == 1
    assert st["nbad"] == 0, st["bad"]
    ts = st["texts"]
    assert ts["fail_pairs"] > 10000 and ts["paths_compared"] > 5000 and ts["messages_compared"] > 5000, ts
    assert np.array_equal(res.raw, runs[None][1].raw)


@pytest.mark.parametrize("mb", ["1", "3"])
def test_c3_sliced_equals_one_slice(mb):
    _, docs, _, rs, runs = slice_runs()
    one, cut = runs[None][1], runs[mb][1]
    assert np.array_equal(one.raw, cut.raw)
    assert np.array_equal(one.rule_counts, cut.rule_counts)
    assert one.counts == cut.counts
    nfail = 0
    for k in range(len(rs.rules)):  # every FAIL pair renders the same path and message
        if not one.rule_counts[k, K.ST_FAIL]:
            continue
        for what in ("path", "message"):
            a, b = one.texts(k, what), cut.texts(k, what)
            assert a == b, (k, what)
        nfail += int(one.rule_counts[k, K.ST_FAIL])
    assert nfail > 10000
    assert sorted(map(_frow, one.failures())) == sorted(map(_frow, cut.failures()))


RESIDENT = r"""
import os, sys
sys.path.insert(0, os.environ["ROOT"]); sys.path.insert(0, os.path.join(os.environ["ROOT"], "tests"))
import numpy as np
import table_edge_cases as T
from kyverno_amd import engine as E, scan as SC
docs, nsl = T.slice_corpus()
rs = E.Ruleset(T.slice_policies())
comm = SC.Comm(SC.Comm.unique_id(), 1, 0, 0)
for mb in ("1", "3"):
    os.environ["KYV_SLICE_MB"] = mb
    b = E.Batch(rs, docs, nsl)
    ref = E.evaluate(rs, b, jit=True)
    f = ref.failures()
    want = sorted(zip(f["res"].tolist(), f["rule"].tolist(), f["alt"].tolist(), f["path_template"].tolist(),
                      map(tuple, f["idx"].tolist())))
    kept = E.evaluate(rs, b, jit=True, copy_back=False)  # every slice's rows stay on one resident list
    assert kept.jit and len(kept.plan()["slices"]) == len(ref.plan()["slices"]) > 1
    assert np.array_equal(kept.rule_counts, ref.rule_counts)
    assert np.array_equal(b.resident_status(), ref.status)
    comm.gather_report(b, 0, root=0)
    got = sorted((int(r[0]), int(r[1]), int(r[2]), int(r[3]), tuple(int(x) for x in r[4:8])) for r in comm.failures_of(0))
    assert got == want and len(got) > 10000, (mb, len(got), len(want))
comm.close()
print("resident rows ok")
"""


def test_c3_sliced_resident_failures():
    """copy_back=False keeps every slice's failing-path rows on one resident list: read back through the library's
    report gather (a one-rank communicator, in a process of its own as in test_gpu_gather.py), they are the rows the
    copy-back run gathered slice by slice. An exported row is (resource, rule, alternative, path template, idx[4]):
    the wire format carries no resolved metadata keys (kyv_batch_export_failures), so those columns of failures() have
    nothing to be compared with here; test_c3_sliced_equals_one_slice compares them between the copy-back runs."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROOT=root)
    env.pop("KYV_SLICE_MB", None)
    r = subprocess.run([sys.executable, "-c", RESIDENT], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "resident rows ok" in r.stdout
