"""Which kernel a launch record asks for (csrc/pocs_launch_forms.hpp) is what the launchers' if / else ladders answered before the
choosers replaced them: tests/launch_forms_demo.cpp, compiled with g++ (no GPU), enumerates stand-in records, and its output is
tests/golden/launch_forms.txt byte for byte -- a fixture generated from the ladders themselves (its first line says how), never from
the choosers.  From the fixture alone: the forms that records reach are exactly the hot-path kernels of the library's code object
(tests/golden/launch_form_kernels.txt, the parent's; that the library still holds exactly these is profiles/launch_forms_isa.txt)."""
import re
import subprocess
from pathlib import Path

import pytest

from conftest import SAN_FLAGS, SAN_SUFFIX

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "golden"


def _lines(path):
    return [ln for ln in path.read_text().splitlines() if ln and not ln.startswith("#")]


@pytest.fixture(scope="module")
def fixture_forms():
    """The form of every accepted record of the fixture."""
    forms = [ln.split(" : ", 1)[1].split(" ! ", 1)[0] for ln in _lines(GOLDEN / "launch_forms.txt")]
    assert forms and all(re.fullmatch(r"k_\w+(<[\w, ]+>)?", f) for f in forms)
    return forms


@pytest.fixture(scope="module")
def kernels():
    """The hot-path kernels of the code object as {form: set of K} (an MC kernel has no K: {None}): K, the first argument of every
    k_gmm_step* kernel, and TB, the one that is 512, leave the name."""
    out = {}
    for ln in _lines(GOLDEN / "launch_form_kernels.txt"):
        m = re.fullmatch(r"(?:void )?\(anonymous namespace\)::(k_\w+?)(?:<(.*)>)?\(pocs_(gmm|mc)_launch\)", ln)
        assert m, ln
        name, args, K = m.group(1), (m.group(2) or "").split(", ") if m.group(2) else [], None
        if m.group(3) == "gmm":
            K, args = int(args[0]), [a for a in args[1:] if a != "512"]
        out.setdefault(name + ("<" + ", ".join(args) + ">" if args else ""), set()).add(K)
    return out


def test_the_choosers_answer_what_the_ladders_answered():
    src, exe = HERE / "launch_forms_demo.cpp", HERE / ("_launch_forms_demo" + SAN_SUFFIX)
    hdr = HERE.parent / "probability-of-collision-for-safe-planning_amd" / "csrc" / "pocs_launch_forms.hpp"
    if not exe.exists() or exe.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O1", "-std=c++17"] + SAN_FLAGS + ["-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    want = "\n".join(_lines(GOLDEN / "launch_forms.txt")) + "\n"
    if out != want:      # (name the first line that differs: the whole texts are 30 KB)
        got, exp = out.splitlines(), want.splitlines()
        i = next((i for i, (g, e) in enumerate(zip(got, exp)) if g != e), min(len(got), len(exp)))
        assert False, "line %d: got %r, the ladders gave %r" % (i + 1, got[i] if i < len(got) else None, exp[i] if i < len(exp) else None)


def test_the_forms_are_the_hot_path_kernels(fixture_forms, kernels):
    """Every form that a record reaches has a kernel, and every hot-path kernel is reached by some record: no instantiation that no
    launch can choose, no choice without one.  A GMM form stands for its eight instantiations, K = 1 .. 8."""
    assert set(fixture_forms) == set(kernels)
    for form, ks in kernels.items():
        assert ks == (set(range(1, 9)) if form.startswith("k_gmm_") else {None}), form
    assert sum(len(ks) for ks in kernels.values()) == len(_lines(GOLDEN / "launch_form_kernels.txt"))


def test_every_family_is_reachable(fixture_forms):
    """The families the header declares (POCS_FORM_FAMILIES) are the families of the forms that records reach."""
    hdr = (HERE.parent / "probability-of-collision-for-safe-planning_amd" / "csrc" / "pocs_launch_forms.hpp").read_text()
    block = hdr[hdr.index("#define POCS_FORM_FAMILIES(X)"):hdr.index("enum Family")]
    declared = set(re.findall(r"X\((k_\w+),", block))
    assert len(declared) == 37
    assert declared == {f.split("<")[0] for f in fixture_forms}
