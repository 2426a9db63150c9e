"""Per-wave facts and hot header rows of a batch (kyv_batch_wave_facts, kyv_layout.h WaveFacts / HotHdr): what the
flattener reports for crafted batches must equal a straightforward recomputation from the documents, for batches of
one resource, one full wave, a wave plus one lane and a tail wave of two lanes; chunks of the parallel flatten that
meet inside a wave must merge their bits; the environment switch makes the batch report "nothing known"; and the
generated source that reads the facts compiles for gfx950."""
import numpy as np
import pytest

import wave_facts_cases as W
from kyverno_amd import engine as E


@pytest.fixture(scope="module")
def ruleset():
    return E.Ruleset(W.policies())


def check_facts(ruleset, docs, threads=0):
    b = E.Batch(ruleset, docs, threads=threads)
    f = b.wave_facts()
    assert sorted(f["order"].tolist()) == list(range(len(docs)))
    assert f["facts"].shape == ((len(docs) + 63) // 64,)
    assert [int(x) for x in f["facts"]] == W.expected_facts(docs, f["order"], f["maps"])
    return f


def bit(paths, path):
    return paths.index(list(path))


@pytest.mark.parametrize("n", W.SIZES)
def test_clean_batch(ruleset, n):
    f = check_facts(ruleset, W.clean(n))
    assert 0 < len(f["maps"]) <= 32
    assert (f["facts"] == (1 << len(f["maps"])) - 1).all()  # every list element everywhere is an object


@pytest.mark.parametrize("n", W.SIZES)
def test_one_pod_with_ephemeral_containers(ruleset, n):
    # a well-formed ephemeralContainers list (the tail wave's last lane): one more list of objects, every bit stays set
    f = check_facts(ruleset, W.with_ephemeral(n, n - 1))
    assert (f["facts"] == (1 << len(f["maps"])) - 1).all()
    docs = W.with_ephemeral(n, n - 1)
    docs[n - 1]["spec"]["ephemeralContainers"].append(None)
    f = check_facts(ruleset, docs)
    pos = int(np.nonzero(f["order"] == n - 1)[0][0])
    eph = bit(f["maps"], ("spec", "ephemeralContainers", "[*]"))
    for w, mw in enumerate(f["facts"]):
        assert (int(mw) >> eph) & 1 == (0 if w == pos // 64 else 1)


@pytest.mark.parametrize("n", W.SIZES)
def test_odd_list_elements(ruleset, n):
    docs, where = W.with_odd(n, max(0, n - len(W.ODD_CLASSES)))
    f = check_facts(ruleset, docs)
    want_clear = {"containers_null": ("spec", "containers", "[*]"), "containers_str": ("spec", "containers", "[*]"),
                  "containers_obj_int": ("spec", "containers", "[*]"),
                  "ports_null": ("spec", "containers", "[*]", "ports", "[*]"), "volumes_int": ("spec", "volumes", "[*]")}
    for cls, at in where.items():
        pos = int(np.nonzero(f["order"] == at)[0][0])
        assert not (int(f["facts"][pos // 64]) >> bit(f["maps"], want_clear[cls])) & 1, cls


def test_each_odd_class_alone_clears_only_its_wave(ruleset):
    for cls in W.ODD_CLASSES:
        docs = W.clean(130)
        docs[70] = W.make_odd(docs[70], cls)
        f = check_facts(ruleset, docs)
        full = (1 << len(f["maps"])) - 1
        pos = int(np.nonzero(f["order"] == 70)[0][0])
        for w, mw in enumerate(f["facts"]):
            assert (int(mw) != full) == (w == pos // 64), (cls, w)


@pytest.mark.parametrize("threads", [2, 3, 8])
def test_parallel_flatten_merges_chunks_inside_a_wave(ruleset, threads):
    # 130 resources over threads * 8 chunks: chunk boundaries fall inside every wave; the odd resources sit next to
    # each other in wave 1 (in different chunks), everything else is clean
    docs, _ = W.with_odd(130, 66)
    docs[100]["spec"]["ephemeralContainers"] = [{"name": "debug", "image": "registry.example.io/debug:1.0.0"}, 5]
    serial = check_facts(ruleset, docs, threads=1)
    par = check_facts(ruleset, docs, threads=threads)
    assert np.array_equal(serial["facts"], par["facts"]) and np.array_equal(serial["hot"], par["hot"])


def test_hot_rows(ruleset):
    docs = W.clean(65) + [{"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "cm"}, "data": {"k": "v"}}]
    f = check_facts(ruleset, docs)
    hot, order = f["hot"], f["order"]
    assert hot.shape == (len(docs), 4)
    spans = []
    for p in range(len(docs)):
        root, nnodes, flags, kclass = (int(x) for x in hot[p])
        assert nnodes == W.count_values(docs[int(order[p])])  # one node row per JSON value
        assert flags & W.RF_ROOT_MAP
        spans.append((root, root + nnodes))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))  # the resources' node ranges do not overlap
    kinds = [docs[int(order[p])]["kind"] for p in range(len(docs))]
    assert len({(k, int(hot[p, 3])) for p, k in enumerate(kinds)}) == 2  # one kind class per kind
    assert [int(x) for x in hot[:, 3]] == sorted(int(x) for x in hot[:, 3])  # kind-major order


def test_switches_report_nothing_known(ruleset, monkeypatch):
    docs, _ = W.with_odd(130, 66)
    b = E.Batch(ruleset, docs)
    on = b.wave_facts()["facts"]
    assert on.any()
    monkeypatch.setenv("KYV_FACT_MAPS", "0")
    assert (b.wave_facts()["facts"] == 0).all()
    monkeypatch.delenv("KYV_FACT_MAPS")
    assert np.array_equal(b.wave_facts()["facts"], on)


def test_generated_source_reads_facts_and_compiles_for_gfx950(ruleset, monkeypatch):
    monkeypatch.setenv("KYV_JIT_CACHE", "0")  # compile for real; keep the in-tree code-object cache untouched
    src, n = ruleset.jit_source()
    assert n > 0
    assert "wave_maps(v, w)" in src and "w.am >>" in src and "ghot(v, r)" in src
    assert "v.hdr[r]" not in src  # the compiled kernels take the header words from the hot rows
    secs, size = ruleset.jit_compile()
    assert size > 1000
