"""The dense failing-path record list at the compaction's edges (cases and the expected order: result_edge_cases.py):
tiles that end inside a rule, on a rule boundary and across two rules, wide and narrow staged records, chunks of 512
records, all-empty tiles, no records at all, more tiles than resident workgroups, one workgroup over every tile, rule
slices, repeated evaluations -- with the round-12 kernels and with round 11's (KYV_RESULT_KERNELS=0). Every list is
compared, order included, with the CPU backend's records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import result_edge_cases as R
from kyverno_amd import engine as E

pytestmark = pytest.mark.gpu
KERNELS = pytest.mark.parametrize("kernels", [None, "0"], ids=["wide", "round11"])


def _switch(monkeypatch, kernels):
    monkeypatch.delenv("KYV_SLICE_MB", raising=False)
    monkeypatch.delenv("KYV_COMPACT_GRID", raising=False)
    if kernels is None:
        monkeypatch.delenv("KYV_RESULT_KERNELS", raising=False)
    else:
        monkeypatch.setenv("KYV_RESULT_KERNELS", kernels)


def _check(res, cpu, want):
    assert np.array_equal(res.raw, cpu.raw)
    assert np.array_equal(res.rule_counts, cpu.rule_counts) and res.counts == cpu.counts
    got = R.rows(res.failures())
    assert len(got) == len(want)
    assert got == want


@KERNELS
@pytest.mark.parametrize("n", R.SIZES)
def test_record_list(n, kernels, monkeypatch):
    _switch(monkeypatch, kernels)
    rs, docs, want, cpu = R.compact_case(n)
    assert len(want) >= 8  # the anyPattern rule alone stages 8 records per Pod
    b = E.Batch(rs, docs)
    res = E.evaluate(rs, b, jit=False)
    assert len(res.plan()["slices"]) == 1
    _check(res, cpu, want)
    # a second evaluation on the same batch (the device buffers are reused) gives the same list
    _check(E.evaluate(rs, b, jit=False), cpu, want)


@pytest.mark.parametrize("n", [65, 64 * 64 + 1])
def test_switch_gives_identical_lists(n, monkeypatch):
    rs, docs, want, cpu = R.compact_case(n)
    b = E.Batch(rs, docs)
    _switch(monkeypatch, None)
    new = E.evaluate(rs, b, jit=False)
    _switch(monkeypatch, "0")
    old = E.evaluate(rs, b, jit=False)
    assert new.failures().tobytes() == old.failures().tobytes() and len(new.failures()) == len(want)
    assert np.array_equal(new.rule_counts, old.rule_counts) and new.counts == old.counts
    assert np.array_equal(new.raw, old.raw)


@KERNELS
def test_more_tiles_than_workgroups(kernels, monkeypatch):
    """256 rules over 4097 match waves: 16,388 tiles, twice the one-wave workgroups that 256 CUs keep resident, most of
    them without records (result_edge_cases.big_policies). A wave of the wide copy then reads several tile totals
    with one load, finds its live tiles by the ballot at r0 + bit * grid, and fills its LDS tables once per tile"""
    _switch(monkeypatch, kernels)
    rs, data, want, counts = R.big_case()
    assert len(rs.rules) * ((R.BIG_N + 63) // 64) // 64 > 2 * 8192 and len(want) > 500000
    res = E.evaluate(rs, E.Batch(rs, data), jit=False)
    assert len(res.plan()["slices"]) == 1
    assert np.array_equal(res.rule_counts, counts)
    got = R._packed(res.failures())
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("grid", ["1", "3", "7"])
def test_few_workgroups(grid, monkeypatch):
    """KYV_COMPACT_GRID caps the wide copy's workgroups: with 72 tiles one workgroup takes two rounds of 64 tile
    totals and every live tile in turn through the same LDS tables; 3 and 7 stride over the tiles"""
    _switch(monkeypatch, None)
    rs, docs, want = R.many_rules_case()
    assert len(rs.rules) * 65 > 64 * 64
    b = E.Batch(rs, docs)
    base = E.evaluate(rs, b, jit=False)
    assert len(base.plan()["slices"]) == 1  # all 72 tiles in one compaction
    assert R.rows(base.failures()) == want
    monkeypatch.setenv("KYV_COMPACT_GRID", grid)
    res = E.evaluate(rs, b, jit=False)
    assert R.rows(res.failures()) == want
    assert np.array_equal(res.raw, base.raw) and np.array_equal(res.rule_counts, base.rule_counts)


@KERNELS
@pytest.mark.parametrize("n", [65, 64 * 64])
def test_every_pair_passes(n, kernels, monkeypatch):
    """no record at all: every tile's total is 0"""
    _switch(monkeypatch, kernels)
    rs, docs, want, cpu = R.compact_case(n, failing=False, passing=True)
    assert want == [] and cpu.counts["fail"] == 0 and cpu.counts["pass"] > 0
    _check(E.evaluate(rs, E.Batch(rs, docs), jit=False), cpu, want)


@KERNELS
def test_rule_slices_copy_back(kernels, monkeypatch):
    """the ruleset cut into rule slices (KYV_SLICE_MB=1, read when a batch's first evaluation lays its slices out):
    copy-back gathers the records slice by slice, and the list is the unsliced one"""
    _switch(monkeypatch, kernels)
    rs, docs, want, cpu = R.compact_case(64 * 64 + 1)
    monkeypatch.setenv("KYV_SLICE_MB", "1")
    b = E.Batch(rs, docs)
    cut = E.evaluate(rs, b, jit=False)
    assert len(cut.plan()["slices"]) >= 2, cut.plan()["slices"]
    _check(cut, cpu, want)
    _check(E.evaluate(rs, b, jit=False), cpu, want)


RESIDENT = r"""
import json, os, sys
sys.path.insert(0, os.environ["ROOT"]); sys.path.insert(0, os.path.join(os.environ["ROOT"], "tests"))
import numpy as np
import result_edge_cases as R
from kyverno_amd import engine as E, scan as SC
comm = SC.Comm(SC.Comm.unique_id(), 1, 0, 0)
out = {}
for n in (65, 64 * 64 + 1):
    rs, docs, want, cpu = R.compact_case(n)
    want = [[r[0], r[1], r[2], r[3]] + list(r[4]) for r in want]  # an exported row carries no resolved keys
    for mb in (None, "1"):
        for kernels in (None, "0"):
            for k, v in (("KYV_SLICE_MB", mb), ("KYV_RESULT_KERNELS", kernels)):
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
            b = E.Batch(rs, docs)
            for again in (0, 1):  # the resident list of a second evaluation replaces the first's
                kept = E.evaluate(rs, b, jit=False, copy_back=False)
                slices = len(kept.plan()["slices"])
                assert n == 65 or (slices >= 2) == (mb == "1"), (n, mb, slices)
                assert np.array_equal(kept.rule_counts, cpu.rule_counts)
                assert np.array_equal(b.resident_status(), cpu.status)
                comm.gather_report(b, 0, root=0)
                got = comm.failures_of(0).tolist()
                assert got == want, (n, mb, kernels, again, len(got), len(want))
            out["%d/%s/%s" % (n, mb, kernels)] = [slices, len(got)]
comm.close()
print("resident lists ok " + json.dumps(out))
"""


def test_resident_lists():
    """copy_back=False keeps the list on the device, and a rule-sliced evaluation appends every slice's records to it
    (`accumulate`): read back through the library's report gather (a one-rank communicator, in a process of its own as
    in test_gpu_gather.py), the rows are the expected list in its order, sliced or not, with either set of kernels,
    also after a second evaluation"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ROOT=root)
    for k in ("KYV_SLICE_MB", "KYV_RESULT_KERNELS", "KYV_COMPACT_GRID"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", RESIDENT], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("resident lists ok ")]
    assert line, r.stdout[-2000:]
    seen = json.loads(line[0][len("resident lists ok "):])
    assert len(seen) == 8 and all(v[1] > 0 for v in seen.values()), seen
    assert all(seen["4097/1/%s" % k][0] >= 2 for k in (None, "0")), seen
