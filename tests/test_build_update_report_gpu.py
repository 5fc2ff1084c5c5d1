"""The report of `ganon-build --hibf --update` on stdout, byte for byte: three commands on the seeded families of
test_build_extend_gpu (seed 86) -- a plain update, a removal alone, and the command of test_remove_extend_and_fold_in_one_command --
against the files under tests/golden/update_report/, which were recorded from the binary of the commit before the report moved into
build_update_report.cpp (two runs of that binary gave the same bytes).  Every path on a command line is relative and the commands run
in the test's own folder, so that no line and no file size depends on where that folder is."""
import os
import subprocess

import pytest

from test_build_cpu import BIN_BUILD
from test_build_extend_gpu import MEMBERS, families, inputs  # noqa: F401  (families: a fixture)
from test_build_hibf_gpu import K, W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_report")
OLD_FAMILIES = [f"F{f}" for f in range(6)]
# what test_remove_extend_and_fold_in_one_command arrives at on these inputs: the restated extension plan accepts the fifth member of
# every family but F3, which leaves; 9 bins is the least bound the fold reaches
GONE, FOLD = "F3", 9


def reports(families, d, binary):
    """{name: stdout} of the three commands, run with `binary` in folder d.  The combined command works on the one IBF of
    test_remove_extend_and_fold_in_one_command; the other two on a tree of the same targets under --tmax 4, so that merged bins are
    touched and left stale"""
    d = str(d)

    def run(args):
        p = subprocess.run([binary] + args + ["-t", "2"], capture_output=True, text=True, timeout=300, cwd=d)
        assert p.returncode == 0, (args, p.stdout[-2000:], p.stderr[-2000:])
        return p.stdout
    inputs(families, {f: [0, 1, 2, 3] for f in OLD_FAMILIES}, os.path.join(d, "base.tsv"))
    for out, tmax in (("old.hibf", "8"), ("tree.hibf", "4")):
        run(["-i", "base.tsv", "-o", out, "--quiet", "-k", str(K), "-w", str(W), "-s", "3", "-p", "0.05", "--hibf", "--tmax", tmax, "--layout", "rule"])
    new = {"F6": list(range(MEMBERS)), "F7": list(range(MEMBERS))}
    inputs(families, {"F6": [0], "F7": list(range(MEMBERS))}, os.path.join(d, "new.tsv"))  # (one member of F6: small enough to go below a merged bin)
    more = {f: [4] for f in OLD_FAMILIES if f != GONE}
    more.update(new)
    inputs(families, more, os.path.join(d, "more.tsv"))
    for name, target in (("gone.txt", GONE), ("small.txt", "F0")):  # (F0 is one of the three small families below a merged bin, which it leaves stale)
        with open(os.path.join(d, name), "w") as o:
            o.write(target + "\n")
    return {"update": run(["--hibf", "--update", "tree.hibf", "-i", "new.tsv", "-o", "update.hibf"]),
            "remove": run(["--hibf", "--update", "tree.hibf", "--remove", "small.txt", "-o", "remove.hibf"]),
            "remove_extend_fold": run(["--hibf", "--update", "old.hibf", "--fold", str(FOLD), "-i", "more.tsv", "--extend", "--remove", "gone.txt",
                                       "-o", "remove_extend_fold.hibf"])}


def test_reports_are_the_recorded_ones(families, tmp_path):
    got = reports(families, tmp_path, BIN_BUILD)
    for name, text in got.items():
        want = open(os.path.join(GOLDEN, name + ".txt")).read()
        assert text == want, f"{name}: first differing line: " + next(
            (f"{a!r} != {b!r}" for a, b in zip(text.splitlines(), want.splitlines()) if a != b), "one report is a prefix of the other")
    assert "user bin(s) extended" in got["remove_extend_fold"] and "IBF(s) created under" in got["remove_extend_fold"]
