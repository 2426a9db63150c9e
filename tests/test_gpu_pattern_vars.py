"""GPU side of the pattern-variable tests (policies, corpus and checker: pattern_vars_cases.py; CPU side:
test_pattern_vars.py): `{{ request.object.<field chain> }}` leaves of validate.pattern / anyPattern on the MI355X,
through the interpreted wave walker and the runtime-compiled walk, pair by pair against the oracle on the substituted
policy."""
import functools

import numpy as np
import pytest

import pattern_vars_cases as M
from kyverno_amd import _lib as K

pytestmark = pytest.mark.gpu
JIT = pytest.mark.parametrize("jit", [False, True], ids=["interpreter", "compiled"])


@functools.lru_cache(maxsize=None)
def run(n, jit, shape_names=False):
    rs, res = M.evaluate(n, "gpu", jit=jit, shape_names=shape_names)
    assert bool(res.jit) == jit
    return rs, res


def check_compiled_plan(rs, res):
    """the rules stay in the fused and chunk kernels of the compiled walk: none is left to the interpreter"""
    p = res.plan()
    npat = sum(r["kind"] in ("pattern", "anyPattern") for r in rs.rules)
    assert sum(s["fused_rules"] + s["chunk_rules"] for s in p["slices"]) == npat == len(rs.rules), p
    assert p["generic_rules"] == 0, p


@JIT
@pytest.mark.parametrize("n", [200, 2000])
def test_parity(n, jit):
    """200 documents: a partial last wave; 2,000: several waves, each with mixed cases"""
    rs, res = run(n, jit)
    st = M.check(res, rs, n)
    M.check_counts(st, rs)
    assert st["compared"] > 6 * n and st["errors"] > n // 8 and st["error_messages"] > n // 8, st
    if jit:
        check_compiled_plan(rs, res)


@JIT
def test_one_lane_alone_in_the_second_wave(jit):
    """(65 documents do not hold every case of every rule, so the per-rule status counts are asserted at 200 and
    2,000 documents, not here; every pair is still checked)"""
    rs, res = run(65, jit)
    st = M.check(res, rs, 65)
    assert st["compared"] > 300, st


def test_two_rules_one_shape_through_the_shape_tables():
    """the two rules that differ only in the variable they name, decided from the pattern-shape tables: each needs its
    own shape"""
    rs, res = run(2000, True, shape_names=True)
    assert res.jit and res.jit_shapes
    st = M.check(res, rs, 2000, shape_names=True)
    M.check_counts(st, rs)
    v, w = (st["counts"][r] for r in ("shape-v", "shape-w"))
    assert v != w, (v, w)
    for c in (v, w):
        assert c[K.ST_PASS] > 0 and c[K.ST_FAIL] > 0 and c[K.ST_ERROR] > 0, (v, w)


def test_gpu_and_cpu_status_matrices_are_identical():
    cpu = np.asarray(M.evaluate(2000, "cpu")[1].raw)
    for jit in (False, True):
        assert np.array_equal(np.asarray(run(2000, jit)[1].raw), cpu), jit
