"""bench.py's set-up shortcuts and --dump-outputs: the prebuilt corpus entry holds the bytes the generator returns,
the sampled verdict blocks are fixed and bounded, and (GPU) a plain run's dumped arrays are what an evaluation of the
same corpus returns to its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from kyverno_amd import synth  # noqa: E402


def test_corpus_cache_entry_is_the_generated_corpus(tmp_path):
    d = str(tmp_path)
    for n, start, workers in ((5000, 0, 2), (3000, 4000, 1)):
        want, nsl = synth.corpus_ndjson(n, kind="mixed", seed=bench.SEED, chunk=2000, start=start, workers=1)
        assert not synth.corpus_is_cached(d, n, kind="mixed", seed=bench.SEED, start=start)
        size = synth.write_corpus_cache(d, n, kind="mixed", seed=bench.SEED, start=start, workers=workers, chunk=2000)
        assert synth.corpus_is_cached(d, n, kind="mixed", seed=bench.SEED, start=start)
        got, nsl2 = synth.cached_corpus(n, kind="mixed", seed=bench.SEED, start=start, cache_dir=d)
        assert size == len(want) and got == want and nsl2 == nsl
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]


@pytest.mark.parametrize("n,nrules", [(1000, 89), (10_000_000, 89), (1_000_000, 25000), (4097, 4000), (7, 1)])
def test_dump_sample_blocks_fixed_and_bounded(n, nrules):
    blocks = bench.dump_sample_blocks(n, nrules)
    assert blocks == bench.dump_sample_blocks(n, nrules)
    cols = sum(k for _, k in blocks)
    assert 0 < cols <= n and cols * nrules * 4 <= max(bench.DUMP_SAMPLE_BYTES, 4 * nrules)
    end = 0
    for r0, k in blocks:  # ascending, disjoint, inside the batch
        assert r0 >= end and k > 0 and r0 + k <= n
        end = r0 + k
    if n * nrules * 4 <= bench.DUMP_SAMPLE_BYTES:
        assert blocks == [(0, n)]


@pytest.mark.gpu
def test_plain_run_dumps_what_the_evaluation_returns(tmp_path):
    from kyverno_amd import _lib as K
    from kyverno_amd import engine as E
    n = 20000
    out = str(tmp_path / "dump")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KYV_CORPUS_CACHE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--resources", str(n), "--steps",
                        "2", "--warmup", "1", "--dump-outputs", out], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["full"] is False
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity_prefix"] is None
    assert line["report_gather"] is None and line["host"]["e2e"] is None
    assert sorted(os.listdir(out)) == ["counts.npy", "rule_counts.npy", "verdict_resources.npy", "verdicts.npy"]
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())

    data, nsl = synth.corpus_ndjson(n, kind="mixed", seed=bench.SEED)
    rs = E.Ruleset(bench.load_policies("c3"))
    res = E.evaluate(rs, E.Batch(rs, data, nsl), backend="gpu")
    assert np.array_equal(got["verdict_resources"], np.arange(n))  # the whole matrix fits at this size
    assert np.array_equal(got["verdicts"], res.status.astype(np.float32))
    assert np.array_equal(got["rule_counts"], res.rule_counts.astype(np.float64))
    assert got["counts"].tolist() == [float(res.counts[s]) for s in K.STATUS_NAMES]
    assert line["value"] * line["ms_per_step"] / 1e3 == pytest.approx(line["config"]["pairs_per_step"], rel=1e-9)
