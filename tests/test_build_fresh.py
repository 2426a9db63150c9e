"""kyverno_amd/build.py rebuilds a product whose input changed WHILE the product was being built. The kernel translation
units compile for minutes; a header saved in that time is not in the object, yet the object is written after the
header, so a freshness test on the time of writing would keep it, and kernels and host code could be linked that
disagree about a struct's layout. The same for the library and an object replaced while it links. No compiler runs
here: the compile and link steps are replaced by ones that write their product and, once, change an input meanwhile."""
import os
import time

from kyverno_amd import build as B


class Clock:
    """the build script's clock in the tests of a change DURING a step, 10 s further at every look: the steps of a test
    lie further apart than any slack the script takes off its stamps. step = 0: the real clock."""
    def __init__(self, step):
        self.step = step
        self.ns = time.time_ns() - 3600 * 10**9

    def time_ns(self):
        if not self.step:
            return time.time_ns()
        self.ns += self.step
        return self.ns


def _tree(tmp_path, monkeypatch, during_compile=None, during_link=None):
    stepping = during_compile is not None or during_link is not None
    csrc, obj = tmp_path / "csrc", tmp_path / "obj"
    csrc.mkdir()
    (csrc / "a.h").write_text("struct V { int x; };\n")
    (csrc / "unit.cpp").write_text('#include "a.h"\nint f() { return sizeof(V); }\n')
    clock = Clock(10 * 10**9 if stepping else 0)
    if stepping:
        monkeypatch.setattr(B, "time", clock, raising=False)
    for f in ("a.h", "unit.cpp"):
        _save(clock, csrc / f, ahead=-100 * 10**9)
    monkeypatch.setattr(B, "CSRC", str(csrc))
    monkeypatch.setattr(B, "HOST_SRCS", ["unit.cpp"])
    monkeypatch.setattr(B, "HIP_SRCS", [])
    steps = []
    hooks = {"compile": during_compile, "link": during_link}

    class Done:
        returncode, stderr = 0, ""

    def run(cmd, **kw):
        step = "link" if "-shared" in cmd else "compile"
        steps.append(step)
        hook, hooks[step] = hooks[step], None  # (once)
        if hook:
            hook(clock, csrc, str(obj))
        with open(cmd[cmd.index("-o") + 1], "w") as f:
            f.write(step)
        return Done()

    monkeypatch.setattr(B.subprocess, "run", run)
    return clock, csrc, steps, lambda: B.build(lib=str(tmp_path / "lib.so"), obj_dir=str(obj))


def _save(clock, path, text=None, ahead=0):
    if text is not None:
        with open(path, "w") as f:
            f.write(text)
    now = clock.time_ns() + ahead
    os.utime(path, ns=(now, now))


def test_unchanged_sources_build_once(tmp_path, monkeypatch):
    clock, csrc, steps, build = _tree(tmp_path, monkeypatch)
    build()
    build()
    assert steps == ["compile", "link"]


def test_header_saved_after_the_build_rebuilds(tmp_path, monkeypatch):
    clock, csrc, steps, build = _tree(tmp_path, monkeypatch)
    build()
    _save(clock, csrc / "a.h", "struct V { int x; int y; };\n", ahead=10**9)
    build()
    assert steps == ["compile", "link"] * 2


def test_header_saved_during_the_compile_rebuilds(tmp_path, monkeypatch):
    clock, csrc, steps, build = _tree(tmp_path, monkeypatch,
                               during_compile=lambda clock, csrc, obj: _save(clock, csrc / "a.h",
                                                                             "struct V { int x; int y; };\n"))
    build()
    build()  # the object of the first build does not hold the header as saved: compiled and linked again
    build()
    assert steps == ["compile", "link"] * 2


def test_object_replaced_during_the_link_relinks(tmp_path, monkeypatch):
    clock, csrc, steps, build = _tree(tmp_path, monkeypatch,
                               during_link=lambda clock, csrc, obj: _save(clock, os.path.join(obj, "unit.cpp.o"),
                                                                          "another compile"))
    build()
    build()  # the library of the first build does not hold the object as replaced: linked again
    build()
    assert steps == ["compile", "link", "link"]
