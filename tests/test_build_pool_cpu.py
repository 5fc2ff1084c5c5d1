"""Which hash sets `ganon-build --hibf`, `--update` and `--verify-index` hand to the device together (ganon_amd/host/hibf_pool.hpp),
without a GPU: the pooler runs in a driver this test compiles, with thresholds small enough that every branch is taken, and is compared
call for call with the rule restated here."""
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ALONE, BATCH = 4, 8


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hibf_pool") / "hibf_pool_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(HERE, "..", "include"), "-o", out, os.path.join(HERE, "hibf_pool_driver.cpp")])
    return out


def run_driver(driver, cases, alone=ALONE, batch=BATCH):
    """-> (defaults, [calls of case]) with a call = (own, ids, offsets, paths)"""
    text = "".join(f"{alone} {batch} {len(sizes)} " + " ".join(map(str, sizes)) + "\n" for sizes in cases)
    lines = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[0].startswith("defaults ")
    got = []
    for ln in lines[1:]:
        f = ln.split()
        if f[0] == "case":
            got.append([])
        elif f[0] == "call":
            kv = dict(x.split("=", 1) for x in f[2:])
            assert kv["data"] == "ok", ln  # every set's hashes lie where the offsets say
            got[-1].append((f[1] == "own", [int(x) for x in kv["ids"].split(",")], [int(x) for x in kv["offsets"].split(",")],
                            [tuple(map(int, x.split(":"))) for x in kv["paths"].split(",")]))
    assert len(got) == len(cases)
    return tuple(int(x) for x in lines[0].split()[1:]), got


def expected(sizes, alone=ALONE, batch=BATCH):
    """the rule: a set of `alone` or more goes by itself, out of its own storage, when it is met; the others gather until the pool holds
    `batch`, and what is left goes at the end"""
    calls, ids = [], []
    for i, n in enumerate(sizes):
        if n >= alone:
            calls.append((True, [i]))
            continue
        ids.append(i)
        if sum(sizes[j] for j in ids) >= batch:
            calls.append((False, ids))
            ids = []
    return calls + ([(False, ids)] if ids else [])


def check(sizes, calls, alone=ALONE, batch=BATCH):
    assert [(own, ids) for own, ids, _, _ in calls] == expected(sizes, alone, batch), sizes
    for own, ids, offsets, paths in calls:
        assert offsets == [sum(sizes[i] for i in ids[:j]) for j in range(len(ids) + 1)], (sizes, ids)
        assert paths == [(i, 2 * i + d) for i in ids for d in (0, 1)], (sizes, ids)  # every set with its own path
    assert sorted(i for _, ids, _, _ in calls for i in ids) == list(range(len(sizes))), sizes  # every set exactly once


CASES = [
    ("all small, below batch", [1, 2, 3], [(False, [0, 1, 2])]),
    ("flush after the third", [3, 3, 3, 3], [(False, [0, 1, 2]), (False, [3])]),
    ("alone, alone - 1, alone + 1", [4, 3, 5], [(True, [0]), (True, [2]), (False, [1])]),
    ("a large set between two small ones", [2, 9, 2], [(True, [1]), (False, [0, 2])]),
    ("a single set", [3], [(False, [0])]),
    ("a single large set", [8], [(True, [0])]),
    ("no sets", [], []),
    ("exactly batch on the last set", [3, 3, 2], [(False, [0, 1, 2])]),
]


@pytest.mark.parametrize("what,sizes,calls", CASES, ids=[c[0] for c in CASES])
def test_cases(driver, what, sizes, calls):
    assert expected(sizes) == calls  # the restated rule says what the issue's list says
    _, got = run_driver(driver, [sizes])
    check(sizes, got[0])


def test_random_size_lists(driver):
    rng = random.Random(20261018)
    cases = [[rng.randrange(0, 10) for _ in range(rng.randrange(0, 24))] for _ in range(50)]
    _, got = run_driver(driver, cases)
    for sizes, calls in zip(cases, got):
        check(sizes, calls)
    kinds = [own for calls in got for own, ids, _, _ in calls]
    assert any(kinds) and not all(kinds)
    assert any(len(calls) > 2 for calls in got)  # flushes in mid-loop


def test_default_thresholds(driver):
    """16 Mi hashes a pool, 4 Mi hashes and more alone -- and they are what the pooler uses when none are given"""
    defaults, got = run_driver(driver, [[5, 6]], alone=0, batch=0)
    assert defaults == (16 << 20, 4 << 20)
    check([5, 6], got[0], alone=4 << 20, batch=16 << 20)
