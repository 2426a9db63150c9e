"""The hot header plane and the per-wave facts on the MI355X (runtime-compiled kernels, jit=True): verdicts, failing
paths and messages of crafted batches -- clean waves, a wave with ephemeralContainers, waves whose lists hold something
other than objects -- and of a mixed corpus equal the oracle's; the run-time switches (KYV_HOTHDR, KYV_FACT_MAPS) change
no verdict; and the byte-accounting build counts fewer walk bytes where a wave's facts let it
skip loads, wave by wave."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as PU
import wave_facts_cases as W
from kyverno_amd import _lib as K
from kyverno_amd import engine as E
from kyverno_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIDED = (K.ST_PASS, K.ST_FAIL, K.ST_ERROR)
# rules whose patterns walk the list an odd class spoils (the oracle decides them PASS / FAIL / ERROR on these
# resources: checked with backend="cpu")
CLASS_RULES = {"containers_null": ("validate-privileged", "require-image-tag", "validate-host-port"),
               "containers_str": ("validate-privileged", "require-image-tag", "validate-host-port"),
               "containers_obj_int": ("validate-privileged", "require-image-tag", "validate-host-port"),
               "ports_null": ("validate-host-port", "host-ports-none"),
               "volumes_int": ("validate-hostPath", "host-path")}


def crafted(n):
    """the crafted batches of n resources: name -> (docs, {odd class: resource index})"""
    odd, where = W.with_odd(n, max(0, n - len(W.ODD_CLASSES)))
    return {"clean": (W.clean(n), {}), "ephemeral": (W.with_ephemeral(n, n - 1), {}), "odd": (odd, where)}


def parity(docs, nsl=None):
    st, res = PU.compare(W.policies(), docs, nsl, backend="gpu", jit=True)
    assert res.jit
    assert st["nbad"] == 0, st["bad"]
    assert st["compared"] > 0
    return st, res


@pytest.mark.parametrize("n", W.SIZES)
@pytest.mark.parametrize("name", ["clean", "ephemeral", "odd"])
def test_crafted_batches_match_oracle(n, name):
    docs, where = crafted(n)[name]
    _, res = parity(docs)
    rules = {r["name"]: k for k, r in enumerate(res.ruleset.rules)}
    for cls, at in where.items():
        got = [int(res.status[rules[nm], at]) for nm in CLASS_RULES[cls]]
        assert all(s in DECIDED for s in got), (cls, [K.STATUS_NAMES[s] for s in got])


def test_mixed_corpus_matches_oracle():
    docs, nsl = synth.mixed(3000, edge=True)
    parity(docs, nsl)


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import wave_facts_cases as W
from kyverno_amd import engine as E, synth
rs = E.Ruleset(W.policies())
docs, where = W.with_odd(130, 66)
docs[100]["spec"]["ephemeralContainers"] = [{"name": "debug", "image": "registry.example.io/debug:1.0.0"}]
mixed, nsl = synth.mixed(3000, edge=True)
out = {}
for name, (d, l) in {"crafted": (docs, None), "mixed": (mixed, nsl)}.items():
    r = E.evaluate(rs, E.Batch(rs, d, l), backend="gpu", jit=True)
    assert r.jit
    out[name] = np.asarray(r.status)
np.savez(sys.argv[1], **out)
"""


def test_switches_change_no_verdict(tmp_path):
    """every mechanism on (this process's defaults) against every mechanism off, the off case in a fresh process"""
    off = dict(os.environ, KYV_HOTHDR="0", KYV_FACT_MAPS="0")
    res = {}
    for tag, env in (("on", dict(os.environ)), ("off", off)):
        path = str(tmp_path / (tag + ".npz"))
        subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), path], env=env, check=True,
                       timeout=300)
        res[tag] = np.load(path)
    for name in ("crafted", "mixed"):
        assert res["on"][name].shape == res["off"][name].shape
        assert np.array_equal(res["on"][name], res["off"][name]), name


def walk_bytes(rs, docs):
    b = E.Batch(rs, docs)
    prod = E.evaluate(rs, b, backend="gpu", jit=True)
    acct = E.evaluate(rs, b, backend="gpu", jit=True, account_bytes=True)
    assert np.array_equal(prod.raw, acct.raw)
    # the walk phase's counted bytes, reads and writes together (the counters are per phase or per class, not both): the
    # verdicts, and so the walk's writes and staged records, are the same with the facts on and off, so a difference
    # between two evaluations of one batch is a difference in read bytes
    return acct.alg_bytes_phase["walk"]


def test_accounted_walk_bytes_follow_the_facts(monkeypatch):
    rs = E.Ruleset(W.policies())
    clean = W.clean(130)
    mixed = W.with_ephemeral(130, 70)  # waves 0 and 2 stay clean; wave 1 has ephemeralContainers and an odd list
    mixed[70]["spec"]["ephemeralContainers"].append(7)
    mixed[71] = W.make_odd(mixed[71], "containers_obj_int")
    on_clean, on_mixed = walk_bytes(rs, clean), walk_bytes(rs, mixed)
    monkeypatch.setenv("KYV_FACT_MAPS", "0")
    off_clean, off_mixed = walk_bytes(rs, clean), walk_bytes(rs, mixed)
    print("walk bytes: clean on %d off %d, mixed on %d off %d" % (on_clean, off_clean, on_mixed, off_mixed))
    assert on_clean < off_clean
    # waves 0 and 2 still elide: the mixed batch lies strictly between the all-clean and the all-off figures
    assert on_clean < on_mixed < off_mixed
    assert on_mixed < off_clean
