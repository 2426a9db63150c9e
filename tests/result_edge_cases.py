"""Crafted batches for the result passes (test_gpu_compact_edges.py, test_gpu_hist_edges.py): the dense failing-path
record list (compact_* kernels) and the per-rule verdict totals (status_hist kernels).

The record list's order is the compaction's: rule, then match wave (64 resources of the batch's kind-major order), then
the order the walk staged the chunk's records in -- one staging round per anyPattern alternative, the lanes of a round
in resource order. `expected_records` lays the CPU backend's records (resource-major, per thread) out in that order."""
import functools

import numpy as np

from kyverno_amd import engine as E

WILD = "a.example.com/*"
NALT = 8
# resource counts and their match waves: 1, 1, 1, 2, 64, 64, 65 -- tiles of 64 (rule, wave) chunks that end inside a
# rule, on a rule boundary, and straddle two rules
SIZES = (1, 63, 64, 65, 64 * 64 - 1, 64 * 64, 64 * 64 + 1)


def _pol(name, rules):
    return {"apiVersion": "kyverno.io/v1", "kind": "ClusterPolicy", "metadata": {"name": name},
            "spec": {"validationFailureAction": "audit", "background": True, "rules": rules}}


def _rule(name, kinds, validate, **extra):
    return dict({"name": name, "match": {"any": [{"resources": {"kinds": kinds}}]}, "validate": validate}, **extra)


def compact_policies(failing=True):
    """a rule with a metadata-expansion site (whole FailRecs staged), plain pattern rules, a rule no resource's kind
    admits (all-empty tiles between full ones) and, with `failing`, an anyPattern rule of 8 alternatives none of which
    any Pod satisfies (512 records per chunk)"""
    rules = [
        _rule("wide-annotation", ["Pod"], {"message": "wide", "pattern": {"metadata": {"annotations": {WILD: "x"}}}}),
        _rule("no-latest", ["Pod"], {"message": "latest", "pattern": {"spec": {"containers": [{"image": "!*:latest"}]}}}),
        _rule("nobody", ["Service"], {"message": "nobody", "pattern": {"spec": {"type": "ClusterIP"}}}),
        _rule("cm-owner", ["ConfigMap"], {"message": "owner", "pattern": {"metadata": {"labels": {"owner": "?*"}}}}),
    ]
    if failing:
        rules.append(_rule("eight-ways", ["Pod"], {"message": "any", "anyPattern": [
            {"metadata": {"labels": {"never-%d" % a: "set"}}} for a in range(NALT)]}))
    rules.append(_rule("named", ["Pod", "ConfigMap"], {"message": "named", "pattern": {"metadata": {"name": "r-*"}}}))
    return [_pol("result-edges", rules)]


def compact_corpus(n, passing=False):
    """n resources, Pods with a ConfigMap every fifth: the kind boundary falls inside a match wave. Unless `passing`,
    Pods fail the wide rule (every third), the image rule (every second, at container 0 or 1) and the name rule (every
    seventh resource); ConfigMaps fail the owner rule (every second)"""
    docs = []
    for i in range(n):
        bad = not passing
        name = "x-%d" % i if bad and i % 7 == 3 else "r-%d" % i
        if i % 5 == 4:
            labels = {} if bad and i % 2 else {"owner": "me"}
            docs.append({"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": name, "labels": labels}})
            continue
        cs = [{"name": "c0", "image": "nginx:1.25"}, {"name": "c1", "image": "redis:7"}]
        if bad and i % 2:
            cs[(i // 2) % 2]["image"] = "nginx:latest"
        ann = {"a.example.com/k": "y" if bad and i % 3 == 0 else "x", "note": "n%d" % i}
        docs.append({"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "d", "annotations": ann},
                     "spec": {"containers": cs}})
    return docs


def rows(f):
    """failures() -> list of (res, rule, alt, path template, idx, key) tuples, in list order"""
    return list(zip(f["res"].tolist(), f["rule"].tolist(), f["alt"].tolist(), f["path_template"].tolist(),
                    map(tuple, f["idx"].tolist()), map(tuple, f["key"].tolist())))


def expected_records(batch, cpu):
    """the CPU backend's records in the compaction's order (module docstring)"""
    order = batch.wave_facts()["order"]  # kind-major position -> input index
    pos = np.empty(batch.n, dtype=np.int64)
    pos[order] = np.arange(batch.n)
    return sorted(rows(cpu.failures()), key=lambda r: (r[1], pos[r[0]] // 64, r[2], pos[r[0]] % 64))


def _packed(f, pos=None):
    """failures() as one uint64 row of 9 columns per record (res, rule, alt, path template, idx[4]... key[2]), for
    comparisons of long lists; with `pos` the compaction's sort key of each record comes back as well"""
    a = np.column_stack([f["res"], f["rule"], f["alt"], f["path_template"], f["idx"], f["key"]]).astype(np.uint64)
    if pos is None:
        return a
    p = pos[f["res"].astype(np.int64)]
    return a, np.lexsort((p % 64, f["alt"], p // 64, f["rule"]))


def expected_array(batch, cpu):
    """expected_records for long lists: the rows of `_packed` in the compaction's order"""
    order = batch.wave_facts()["order"]
    pos = np.empty(batch.n, dtype=np.int64)
    pos[order] = np.arange(batch.n)
    a, key = _packed(cpu.failures(), pos)
    return a[key]


def many_rules_policies(nrules):
    """`nrules` plain pattern rules over two kinds: with 65 match waves, 70 of them are 72 tiles, more than one round
    of 64 for a single workgroup"""
    rules = [_rule("r%d" % i, ["Pod"] if i % 3 else ["ConfigMap"],
                   {"message": "m", "pattern": {"metadata": {"name": "r-*"} if i % 2 else {"labels": {"owner": "?*"}}}})
             for i in range(nrules)]
    return [_pol("many-rules", rules)]


@functools.lru_cache(maxsize=None)
def many_rules_case(nrules=70, n=64 * 64 + 1):
    rs = E.Ruleset(many_rules_policies(nrules))
    docs = compact_corpus(n)
    b = E.Batch(rs, docs)
    return rs, docs, expected_records(b, E.evaluate(rs, b, backend="cpu"))


BIG_N = 64 * 4096 + 1   # 4097 match waves
BIG_RULES = 256         # x 4097 waves / 64 = 16,388 tiles: twice the 8,192 one-wave workgroups 256 CUs keep resident


def big_policies():
    """256 rules, 4 of them over Pods (a wide one, an image rule, an anyPattern of 8 alternatives that all fail for
    one Pod in 32, the name rule) among 252 over ConfigMaps: the Pod waves of a ConfigMap rule are tiles without
    records, as most tiles of the benchmark's ruleset are"""
    rules = []
    for i in range(BIG_RULES):
        if i == 10:
            rules.append(_rule("wide-annotation", ["Pod"], {"message": "wide", "pattern": {"metadata": {"annotations": {WILD: "x"}}}}))
        elif i == 90:
            rules.append(_rule("no-latest", ["Pod"], {"message": "latest", "pattern": {"spec": {"containers": [{"image": "!*:latest"}]}}}))
        elif i == 170:
            rules.append(_rule("eight-ways", ["Pod"], {"message": "any", "anyPattern": [
                {"metadata": {"labels": {"ok": "a%d" % a}}} for a in range(NALT)]}))
        elif i == 250:
            rules.append(_rule("named", ["Pod", "ConfigMap"], {"message": "named", "pattern": {"metadata": {"name": "r-*"}}}))
        else:
            rules.append(_rule("cm-owner-%d" % i, ["ConfigMap"], {"message": "owner", "pattern": {"metadata": {"labels": {"owner": "?*"}}}}))
    return [_pol("big", rules)]


def big_corpus(n=BIG_N):
    """NDJSON: a ConfigMap every fifth resource, one in 16 of them without the owner label; Pods fail the wide rule
    (one in 16), the image rule (one in 8), every alternative (one in 32) and the name rule (one in 64)"""
    out = []
    for i in range(n):
        name = "x-%d" % i if i % 64 == 3 else "r-%d" % i
        if i % 5 == 4:
            out.append('{"apiVersion":"v1","kind":"ConfigMap","metadata":{"name":"%s","labels":{%s}}}'
                       % (name, "" if i % 80 == 4 else '"owner":"me"'))
            continue
        out.append('{"apiVersion":"v1","kind":"Pod","metadata":{"name":"%s","namespace":"d","labels":{%s},"annotations":'
                   '{"a.example.com/k":"%s"}},"spec":{"containers":[{"name":"c0","image":"%s"}]}}'
                   % (name, "" if i % 32 == 1 else '"ok":"a0"', "y" if i % 16 == 2 else "x",
                      "nginx:latest" if i % 8 == 5 else "nginx:1.25"))
    return "\n".join(out).encode()


@functools.lru_cache(maxsize=None)
def big_case():
    """-> (ruleset, corpus, expected rows (expected_array), the CPU backend's per-rule totals)"""
    rs = E.Ruleset(big_policies())
    data = big_corpus()
    b = E.Batch(rs, data)
    cpu = E.evaluate(rs, b, backend="cpu", threads=16)
    return rs, data, expected_array(b, cpu), cpu.rule_counts.copy()


@functools.lru_cache(maxsize=None)
def compact_case(n, failing=True, passing=False):
    """-> (ruleset, documents, the expected record list, the CPU backend's results), computed once per case"""
    rs = E.Ruleset(compact_policies(failing))
    docs = compact_corpus(n, passing)
    b = E.Batch(rs, docs)
    cpu = E.evaluate(rs, b, backend="cpu")
    return rs, docs, expected_records(b, cpu), cpu


# ---------------------------------------------------------------- histogram
GOOD_C = {"name": "c", "image": "nginx", "securityContext": {"allowPrivilegeEscalation": False, "runAsNonRoot": True,
          "capabilities": {"drop": ["ALL"]}, "seccompProfile": {"type": "RuntimeDefault"}}}
HIST_SIZES = (1, 15, 16, 17, 18, 21, 23, 31, 35, 43, 4097, 70001)
HIST_RULES = 5  # row k of a case starts at byte k * n of the verdict plane: over HIST_SIZES, every alignment modulo 16


def hist_policies():
    """five rules, so verdict rows start at every alignment modulo 16 for the odd sizes: a pattern (PASS / FAIL), a
    pattern behind preconditions (SKIP with the precondition mark), podSecurity (ERROR on a pod that does not decode),
    a rule the compiler leaves to the CPU engine (FALLBACK) and one no resource's kind admits (NONE)"""
    return [_pol("hist-edges", [
        _rule("no-latest", ["Pod"], {"message": "latest", "pattern": {"spec": {"containers": [{"image": "!*:latest"}]}}}),
        _rule("web-only", ["Pod"], {"message": "web", "pattern": {"metadata": {"labels": {"team": "?*"}}}},
              preconditions={"all": [{"key": "{{ request.object.metadata.labels.tier || '' }}", "operator": "Equals",
                                      "value": "web"}]}),
        _rule("psa", ["Pod"], {"podSecurity": {"level": "restricted", "version": "latest"}}),
        _rule("claims", ["Pod", "ConfigMap"], {"message": "claims", "pattern": {"spec": {"=(volumeClaimTemplates)": [
            {"=(metadata)": {"=(annotations)": {"=(" + WILD + ")": "x"}}}]}}}),
        _rule("nobody", ["Service"], {"message": "nobody", "pattern": {"spec": {"type": "ClusterIP"}}}),
    ])]


def hist_corpus(n):
    docs = []
    for i in range(n):
        if i % 6 == 5:
            docs.append({"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "cm-%d" % i}})
            continue
        c = dict(GOOD_C)
        if i % 3 == 1:
            c["image"] = "nginx:latest"
        if i % 4 == 2:
            c["env"] = [{"name": "A", "value": 5}]  # not a corev1.Pod: the podSecurity rule errors
        if i % 7 == 0:
            c["securityContext"] = {"privileged": True}
        labels = {"tier": "web"} if i % 2 else {"tier": "db"}
        if i % 4 == 1:
            labels["team"] = "t"
        docs.append({"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "p-%d" % i, "namespace": "d", "labels": labels},
                     "spec": {"containers": [c]}})
    return docs


LONG_RULES = 32
LONG_N = 2_000_003
HIST_BLOCK, HIST_PER_CU, MAX_CUS = 256, 8, 512  # the kernel's block, its blocks per CU, the largest chip assumed


def long_row_trips(n=LONG_N, nrules=LONG_RULES, cus=MAX_CUS):
    """16-byte loads per thread of the histogram over a row of n bytes: the launch takes ceil(cus * 8 / rules) blocks
    of 256 threads per row (fewer when the row is short), and a thread strides over the row's 16-byte words"""
    nv = n // 16
    hgrid = max(1, min(-(-cus * HIST_PER_CU // nrules), -(-nv // HIST_BLOCK)))
    return nv / (hgrid * HIST_BLOCK)


def one_status_corpus(n):
    """n ConfigMaps of one shape: a whole verdict row of a single status"""
    return b"\n".join(b'{"apiVersion":"v1","kind":"ConfigMap","metadata":{"name":"c"}}' for _ in range(n))


def one_status_policies():
    """32 rules: a row of PASS, a row of FAIL and 30 rows of NONE (rules no resource's kind admits, which cost the
    evaluation nothing): the more rules, the fewer blocks per row and the more trips per thread"""
    return [_pol("one-status", [
        _rule("has-name", ["ConfigMap"], {"message": "name", "pattern": {"metadata": {"name": "?*"}}}),
        _rule("has-owner", ["ConfigMap"], {"message": "owner", "pattern": {"metadata": {"labels": {"owner": "?*"}}}}),
    ] + [_rule("nobody-%d" % i, ["Service"], {"message": "nobody", "pattern": {"spec": {"type": "ClusterIP"}}})
         for i in range(LONG_RULES - 2)])]
