"""Order of a batch within a kind (kyv_batch_shape_keys, batch.cpp shape_keys / order_by_kind): the order the library
reports equals a stable sort by (kind class position, shape key, input index), the key recomputed here from the
documents over the list positions the library names; it does not depend on the thread count; KYV_SHAPE_ORDER=0
restores the plain kind-major order; and on a mixed corpus the order brings the per-wave list-loop trip counts down."""
import numpy as np
import pytest

import bench
import shape_order_cases as C
import wave_facts_cases as W
from kyverno_amd import engine as E
from kyverno_amd import synth


@pytest.fixture(scope="module")
def ruleset():
    return E.Ruleset(W.policies())


def check_order(ruleset, docs, threads=0, ordered=True):
    f = E.Batch(ruleset, docs, threads=threads).wave_facts()
    paths, bits = f["shape_paths"], f["shape_bits"]
    assert f["shape_ordered"] == ordered
    assert bits == 3 and 0 < len(paths) * bits <= 64
    first = [p for p in paths if p.count("[*]") == 1]
    assert paths[:len(first)] == first  # first-level lists in the most significant bits
    assert [p.count("[*]") for p in paths] == sorted(p.count("[*]") for p in paths)
    want = [C.key_of(d, paths, bits) if ordered else 0 for d in docs]
    assert [int(k) for k in f["shape_keys"]] == want
    assert f["order"].tolist() == C.expected_order(docs, want)
    return f


@pytest.mark.parametrize("n", W.SIZES)
def test_order_is_class_key_input_index(ruleset, n):
    f = check_order(ruleset, C.mixed_kinds(n))
    assert sorted(f["order"].tolist()) == list(range(n))


def test_kinds_of_fewer_than_64_share_waves(ruleset):
    docs = C.mixed_kinds(130)
    f = check_order(ruleset, docs)
    kinds = [docs[int(i)]["kind"] for i in f["order"]]
    assert max(kinds.count(k) for k in set(kinds)) < 64
    assert kinds.index("Deployment") < 64 and kinds.index("CronJob") // 64 == (kinds.index("CronJob") - 1) // 64
    keys = f["shape_keys"][f["order"]]
    for w0 in (0, 64):  # key boundaries inside both full waves
        assert len(set(keys[w0:w0 + 64].tolist())) > 2


@pytest.mark.parametrize("n", W.SIZES)
def test_all_keys_equal_keeps_input_order(ruleset, n):
    f = check_order(ruleset, C.equal_keys(n))
    assert len(set(f["shape_keys"].tolist())) == 1
    assert f["order"].tolist() == list(range(n))


@pytest.mark.parametrize("n", W.SIZES)
def test_all_keys_distinct(ruleset, n):
    f = check_order(ruleset, C.distinct_keys(n))
    assert len(set(f["shape_keys"].tolist())) == n
    sk = f["shape_keys"][f["order"]]
    assert (sk[1:] > sk[:-1]).all()


def test_extremes(ruleset):
    docs = C.extremes()
    f = check_order(ruleset, docs + W.clean(60))
    paths, bits = f["shape_paths"], f["shape_bits"]

    def field(i, path):
        return (int(f["shape_keys"][i]) >> (bits * (len(paths) - 1 - paths.index(list(path))))) & 7

    cont, ports = ("spec", "containers", "[*]"), ("spec", "containers", "[*]", "ports", "[*]")
    assert [field(i, cont) for i in range(6)] == [0, 0, 0, 7, 3, 2]
    assert [field(i, ports) for i in range(6)] == [0, 0, 0, 1, 1, 4]
    assert field(6, ("spec", "volumes", "[*]")) == 0 and field(6, ("spec", "securityContext", "sysctls", "[*]")) == 2


@pytest.mark.parametrize("threads", [1, 2, 3, 8])
def test_order_does_not_depend_on_threads(ruleset, threads):
    # 260 documents are one slice of the sort whatever `threads` says (the parse is what runs on two threads here);
    # the sliced tests below are the ones that run the parallel sort on several slices
    docs = C.mixed_kinds(130) + C.distinct_keys(130)
    base = E.Batch(ruleset, docs, threads=1).wave_facts()
    f = check_order(ruleset, docs, threads=threads)
    assert np.array_equal(f["order"], base["order"]) and np.array_equal(f["shape_keys"], base["shape_keys"])
    assert np.array_equal(f["hot"], base["hot"]) and np.array_equal(f["facts"], base["facts"])


@pytest.mark.parametrize("n", W.SIZES)
def test_switch_off_restores_kind_major_input_order(ruleset, n, monkeypatch):
    monkeypatch.setenv("KYV_SHAPE_ORDER", "0")
    docs = C.mixed_kinds(n)
    f = check_order(ruleset, docs, ordered=False)
    order = f["order"].tolist()
    for kind in {d["kind"] for d in docs}:
        at = [i for i in order if docs[i]["kind"] == kind]
        assert at == sorted(at)  # positions within a class ascend with the input index
    monkeypatch.setenv("KYV_SHAPE_ORDER", "1")
    check_order(ruleset, docs, ordered=True)


@pytest.mark.parametrize("threads", [1, 3])
def test_many_distinct_keys_take_the_comparison_sort(ruleset, threads, monkeypatch):
    # beyond KYV_SHAPE_BUCKETS distinct (class, key) pairs (default 65536) the library sorts by comparison instead of
    # counting: the same order
    docs = C.mixed_kinds(130) + C.distinct_keys(130)
    base = check_order(ruleset, docs, threads=threads)
    assert len(set(base["shape_keys"].tolist())) > 16
    monkeypatch.setenv("KYV_SHAPE_BUCKETS", "16")
    f = check_order(ruleset, docs, threads=threads)
    assert np.array_equal(f["order"], base["order"]) and np.array_equal(f["hot"], base["hot"])


# ---------------------------------------------------------------- several slices of the parallel sort
# The flattener works on a batch with min(threads, documents / 256 + 1) threads; the key pre-pass runs in chunks of
# 4096 resources and the counting sort in min(2 * threads, n / 4096 + 1) slices, each with its own set of distinct
# pairs and its own histogram, joined by an exclusive prefix over (rank, slice) before the parallel scatter. The
# crafted batches above are one slice. 20,000 mixed resources are 5 chunks of the pre-pass and, for threads = 1, 2, 3, 8,
# 2, 4, 5 and 5 slices of the sort, with kinds and keys interleaved through every slice.
@pytest.fixture(scope="module")
def sliced(ruleset):
    docs, nsl = synth.mixed(20000, seed=7)
    base = E.Batch(ruleset, docs, nsl, threads=1).wave_facts()
    paths, bits = base["shape_paths"], base["shape_bits"]
    keys = [C.key_of(d, paths, bits) for d in docs]  # the reference, computed once
    assert len({(d["kind"], k) for d, k in zip(docs, keys)}) > 64 and len({d["kind"] for d in docs}) > 2
    return docs, nsl, keys, C.expected_order(docs, keys), base


def check_sliced(ruleset, sliced, threads):
    docs, nsl, keys, order, base = sliced
    f = E.Batch(ruleset, docs, nsl, threads=threads).wave_facts()
    assert f["shape_ordered"] and f["shape_paths"] == base["shape_paths"]
    assert [int(k) for k in f["shape_keys"]] == keys
    assert f["order"].tolist() == order  # the Python stable sort by (class position, recomputed key, input index)
    for what in ("order", "shape_keys", "hot", "facts"):
        assert np.array_equal(f[what], base[what]), what
    assert [int(x) for x in f["facts"]] == W.expected_facts(docs, f["order"], f["maps"])


@pytest.mark.parametrize("threads", [1, 2, 3, 8])
def test_sliced_counting_sort_equals_reference_order(ruleset, sliced, threads):
    check_sliced(ruleset, sliced, threads)


@pytest.mark.parametrize("threads", [1, 2, 3, 8])
def test_sliced_comparison_sort_equals_reference_order(ruleset, sliced, threads, monkeypatch):
    monkeypatch.setenv("KYV_SHAPE_BUCKETS", "16")  # every slice finds more than 16 distinct pairs
    check_sliced(ruleset, sliced, threads)


@pytest.mark.parametrize("threads", [1, 8])
def test_sliced_switch_off_keeps_input_order_within_a_class(ruleset, sliced, threads, monkeypatch):
    docs, nsl, _, _, _ = sliced
    monkeypatch.setenv("KYV_SHAPE_ORDER", "0")
    f = E.Batch(ruleset, docs, nsl, threads=threads).wave_facts()
    assert not f["shape_ordered"] and not f["shape_keys"].any()
    assert f["order"].tolist() == C.expected_order(docs, [0] * len(docs))


# ---------------------------------------------------------------- what the order is for
def trip_sum(docs, order, paths):
    """sum over waves of 64 positions and key paths of the wave's largest list length: the iterations the waves'
    per-lane list loops run"""
    lens = np.array([[C.max_len(d, p[:-1]) for p in paths] for d in docs], dtype=np.int64)[np.asarray(order)]
    pad = (-len(docs)) % 64
    lens = np.concatenate([lens, np.zeros((pad, len(paths)), dtype=np.int64)])
    return int(lens.reshape(-1, 64, len(paths)).max(axis=1).sum())


def test_bench_corpus_wave_trip_counts(monkeypatch):
    rs = E.Ruleset(bench.load_policies("c3"))
    docs, nsl = synth.mixed(20000, seed=7)
    on = E.Batch(rs, docs, nsl).wave_facts()
    monkeypatch.setenv("KYV_SHAPE_ORDER", "0")
    off = E.Batch(rs, docs, nsl).wave_facts()
    assert on["shape_ordered"] and not off["shape_ordered"]
    assert on["shape_paths"] == off["shape_paths"]
    paths = on["shape_paths"]
    assert any(p.count("[*]") > 1 for p in paths)  # nested lists are in the key
    s_on, s_off = trip_sum(docs, on["order"], paths), trip_sum(docs, off["order"], paths)
    print("per-wave maximum list lengths, summed: shape order %d, kind-major order %d, ratio %.3f"
          % (s_on, s_off, s_on / s_off))
    assert s_on <= 0.6 * s_off
