"""`ganon-build --hibf --verify-index` in parts, without a GPU: the state carried from part to part (ganon_amd/host/hibf_verify_parts.hpp)
-- the bitmaps, the bit planes of a cut IBF and their closing rule, the merge of two workers' planes -- against a per-hash evaluation
made here, and the command's refusals that need no device.  The driver is a stand-alone program under AddressSanitizer and UBSan with
buffers of exactly the words there are; nothing is preloaded."""
import os
import subprocess

import numpy as np
import pytest

from test_build_cpu import BIN_BUILD
from test_build_hibf_cpu import tiny_input  # noqa: F401  (a fixture)
from test_build_verify_cpu import tiny_index  # noqa: F401  (a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (0, 1, 63, 64, 65, 512, 513)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("build_verify_parts") / "build_verify_parts_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(HERE, "build_verify_parts_driver.cpp")])
    return exe


def run(driver, text):
    p = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])  # (a sanitizer report ends the program with a status)
    out = []
    for ln in p.stdout.splitlines():
        f = ln.split()
        assert f[0] == "unit"
        alive = np.array([c == "1" for c in f[6][len("alive="):].replace("-", "")], dtype=bool)
        out.append(dict(found=int(f[2]), first_lost=int(f[3]), open=int(f[4]), plane_words=int(f[5]), alive=alive,
                        lost=[int(x) for x in f[7][len("lost="):].split(",")]))
    return out


def bits(a):
    return "".join("1" if x else "0" for x in a) or "-"


def slab_line(cmd, u, d, planes):
    """planes: bool [n_bins, n]"""
    return f"{cmd} {u} {d} {len(planes)} " + " ".join(bits(p) for p in planes)


def every_pattern(n, n_bins, n_slabs, seed):
    """in[s, b, q] = "every row of hash q in slab s has the bit of bin b": hash q takes pattern number q of all 2^(slabs * bins), shuffled,
    so that 512 hashes meet every hit pattern of up to three bins in up to three slabs; the shorter sets take a random choice of them"""
    rng = np.random.default_rng(seed)
    k = n_slabs * n_bins
    pat = rng.permutation(1 << k)[np.arange(n) % (1 << k)] if n >= (1 << k) else rng.integers(0, 1 << k, size=n)
    return np.array([[(pat >> (s * n_bins + b)) & 1 for b in range(n_bins)] for s in range(n_slabs)], dtype=bool).reshape(n_slabs, n_bins, n)


@pytest.mark.parametrize("n_slabs", [2, 3])
@pytest.mark.parametrize("n_bins", [1, 2, 3])
def test_the_closing_rule_over_every_hit_pattern(driver, n_bins, n_slabs):
    text, want = [], []
    for n in SIZES:
        ins = every_pattern(n, n_bins, n_slabs, n + n_bins)
        if n >= 512:
            assert len({tuple(ins[:, :, q].ravel()) for q in range(n)}) == 1 << (n_bins * n_slabs), "every hit pattern"
        text += [f"new 1 1 {n}"] + [slab_line("slab", 0, 0, ins[s]) for s in range(n_slabs)] + ["report", "close 0 0", "report"]
        # a hash is in the run when ONE bin has its bit in every slab -- not when every slab has some bin
        want.append(np.array([any(all(ins[s, b, q] for s in range(n_slabs)) for b in range(n_bins)) for q in range(n)], dtype=bool))
    got = run(driver, "\n".join(text) + "\n")
    assert len(got) == 2 * len(SIZES)
    for n, hit, before, after in zip(SIZES, want, got[0::2], got[1::2]):
        words = (n + 63) // 64
        assert before["found"] == n and before["first_lost"] == -1 and before["lost"] == [0], "nothing is known before the entry is closed"
        assert (before["open"], before["plane_words"]) == (1, n_bins * words), "n_bins bits per hash while the group runs"
        assert (after["open"], after["plane_words"]) == (0, 0), "the planes are freed"
        assert np.array_equal(after["alive"], hit), n
        assert after["found"] == int(hit.sum()) and after["lost"] == [n - int(hit.sum())]
        assert after["first_lost"] == (-1 if hit.all() else int(np.argmin(hit)))


def test_a_per_slab_or_would_call_it_found(driver):
    """bin 0 only in slab A, bin 1 only in slab B: lost"""
    a = np.array([[True], [False]])
    b = np.array([[False], [True]])
    got = run(driver, "\n".join(["new 1 1 1", slab_line("slab", 0, 0, a), slab_line("slab", 0, 0, b), "close 0 0", "report"]) + "\n")
    assert got[0]["found"] == 0 and got[0]["first_lost"] == 0 and got[0]["lost"] == [1]


@pytest.mark.parametrize("n", [1, 65, 513])
def test_lost_at_two_levels_and_twice_in_one_level(driver, n):
    """depth 3: entry 0 in a cut IBF of two slabs (two bins), entry 1 whole in one part, entry 2 in a cut IBF of three slabs (one bin).
    Hash 0 is lost in entries 0 and 1; the last hash is lost in two different slabs of entry 2; one in the middle is lost nowhere."""
    rng = np.random.default_rng(n)
    e0 = rng.random((2, 2, n)) < 0.9
    e1 = rng.random(n) < 0.9
    e2 = rng.random((3, 1, n)) < 0.9
    e0[:, :, 0] = [[True, False], [False, True]]
    e1[0] = False
    e2[:, 0, n - 1] = [False, True, False]
    mid = n // 2
    if 0 < mid < n - 1:
        e0[:, :, mid], e1[mid], e2[:, :, mid] = True, True, True
    # the parts come in any order, and a closed entry is not closed again by a later report
    text = ["new 3 1 " + str(n), slab_line("slab", 0, 2, e2[2]), slab_line("slab", 0, 0, e0[1]), "whole 0 1 " + bits(e1), slab_line("slab", 0, 2, e2[0]),
            slab_line("slab", 0, 0, e0[0]), "close 0 0", slab_line("slab", 0, 2, e2[1]), "close 0 2", "close 0 2", "report"]
    got = run(driver, "\n".join(text) + "\n")[0]
    c0 = (e0[0] & e0[1]).any(axis=0)
    c2 = (e2[0] & e2[1] & e2[2]).any(axis=0)
    ok = c0 & e1 & c2
    assert not ok[0] and (n == 1 or not ok[n - 1]) and (not 0 < mid < n - 1 or ok[mid])
    assert got["lost"] == [int((~c0).sum()), int((~e1).sum()), int((~c2).sum())], "each entry counted on its own"
    assert got["found"] == int(ok.sum()), "a hash lost at two levels, or twice in one, is counted once"
    assert got["first_lost"] == int(np.argmin(ok)) == 0
    assert np.array_equal(got["alive"], ok) and got["open"] == 0


def test_units_do_not_share_words(driver):
    """two units, the second of no hash; an entry nobody answered closes to nothing"""
    text = ["new 2 3 65 0 64", "whole 0 0 " + "1" * 64 + "0", "whole 2 1 " + "0" + "1" * 63, "whole 1 0 -", slab_line("slab", 1, 1, np.zeros((2, 0), bool)), "close 1 1",
            "close 0 1", "report"]
    got = run(driver, "\n".join(text) + "\n")
    assert [g["found"] for g in got] == [64, 0, 63] and [g["first_lost"] for g in got] == [64, -1, 0]
    assert [g["lost"] for g in got] == [[1, 0], [0, 0], [0, 1]] and got[0]["open"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_the_merge_of_two_workers_planes(driver, n):
    """two slabs answered by two workers into planes of their own (one with the padding bits set, one with them clear), merged, closed: the
    same as the two slabs one after the other, and as the per-hash evaluation"""
    rng = np.random.default_rng(n + 5)
    a, b = rng.random((3, n)) < 0.7, rng.random((3, n)) < 0.7
    both = f"slabs2 0 0 3 " + " ".join(bits(p) for p in a) + " | " + " ".join(bits(p) for p in b)
    got = run(driver, "\n".join([f"new 1 1 {n}", both, "close 0 0", "report",
                                 f"new 1 1 {n}", slab_line("slab", 0, 0, b), slab_line("slab", 0, 0, a), "close 0 0", "report"]) + "\n")
    hit = (a & b).any(axis=0)
    for g in got:
        assert np.array_equal(g["alive"], hit) and g["found"] == int(hit.sum()) and g["lost"] == [n - int(hit.sum())] and g["open"] == 0


def test_slabs_that_disagree_on_the_bins_are_refused(driver):
    p = subprocess.run([driver], input="new 1 1 3\nslab 0 0 2 111 111\nslab 0 0 1 111\n", capture_output=True, text=True)
    assert p.returncode != 0 and "disagree" in p.stderr


# ------------------------------------------------------------------------------------------------------------ the command's refusals
def test_refusals_that_need_no_device(tiny_input, tiny_index, tmp_path):  # noqa: F811
    inp, out = tiny_input
    verify = ["-i", inp, "--hibf", "--verify-index", tiny_index]
    for args, word in ((["-i", inp, "--hibf", "-o", out, "--verify-memory", "1000"], "--verify-memory needs --verify-index"),
                       (["-i", inp, "--hibf", "-o", out, "--verify-devices", "0,0"], "--verify-devices needs --verify-index"),
                       (["-i", inp, "-o", out, "--verify-memory", "1000"], "--verify-memory needs --verify-index"),
                       (["-i", inp, "--hibf", "--update", tiny_index, "-o", out, "--verify-devices", "0"], "--verify-devices needs --verify-index"),
                       (verify + ["--verify-memory", "0"], "--verify-memory has to be > 0"),
                       (verify + ["--verify-memory", "-5"], "failed to parse"),
                       (verify + ["--verify-memory", "1k"], "failed to parse"),
                       (verify + ["--verify-memory", ""], "failed to parse"),
                       (verify + ["--verify-devices", "0,"], "failed to parse"),
                       (verify + ["--verify-devices", "0,,1"], "failed to parse"),
                       (verify + ["--verify-devices", "a"], "failed to parse"),
                       # the build's switches stay the build's
                       (verify + ["--hibf-memory", "1000"], "--hibf-memory cannot be used with --verify-index"),
                       (verify + ["--hibf-devices", "0"], "--hibf-devices cannot be used with --verify-index")):
        p = subprocess.run([BIN_BUILD] + args, capture_output=True, text=True)
        assert p.returncode == 1 and word in p.stderr and p.stdout == "" and not os.path.exists(out), (args, p.stderr)
    p = subprocess.run([BIN_BUILD, "--help"], capture_output=True, text=True)
    assert "--verify-memory arg" in p.stderr and "--verify-devices arg" in p.stderr and "--hibf-memory arg" in p.stderr
