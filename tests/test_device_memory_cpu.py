"""Which granules of a sparse array get memory (csrc/sparse_granules.h, used by DeviceMemory::alloc_sparse), on the CPU.

tests/device_memory/granules_driver.cpp is compiled with a plain host compiler against the header -- once as it is and once with
the address and undefined-behaviour sanitizers, both run as programs of their own -- reads cases from stdin and prints the merged
ranges.  The expected answer is restated here by granule index: the 2 MiB granules that intersect any [first, last) with
last > first, clipped to ceil(total / 2 MiB)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
GRAN = 2 << 20


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def granules(request, tmp_path_factory):
    """granules(cases) -> per case the merged [(first, last), ...] in bytes; a case is (total_bytes, [(first, last), ...])."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("device_memory") / ("granules_driver_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC,
                        os.path.join(ROOT, "tests", "device_memory", "granules_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(cases):
        text = "".join(" ".join(str(v) for v in [total, len(rg)] + [b for r in rg for b in r]) + "\n" for total, rg in cases)
        p = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr
        out = [[int(t) for t in line.split()] for line in p.stdout.splitlines()]
        assert len(out) == len(cases)
        assert all(len(o) == 1 + 2 * o[0] for o in out)
        return [list(zip(o[1::2], o[2::2])) for o in out]
    return run


def expected_granules(total, ranges):
    """indices of the granules that hold a byte of some non-empty [first, last), below ceil(total / GRAN)"""
    ngran = -(-total // GRAN)
    want = set()
    for first, last in ranges:
        if last > first:
            want.update(k for k in range(first // GRAN, (last - 1) // GRAN + 1) if k < ngran)
    return want


def check(total, ranges, merged):
    want = expected_granules(total, ranges)
    got = set()
    prev_last = None
    for first, last in merged:
        assert first % GRAN == 0 and last % GRAN == 0 and last > first, (total, ranges, merged)
        if prev_last is not None:        # sorted, disjoint, and apart: at least one unbacked granule lies between two ranges
            assert first > prev_last, (total, ranges, merged)
            assert any(k not in want for k in range(prev_last // GRAN, first // GRAN)), (total, ranges, merged)
        prev_last = last
        got.update(range(first // GRAN, last // GRAN))
    assert got == want, (total, ranges, merged)


def galloc_ranges(total, front, nblk, bstride, wlo, whi, w):
    """the byte ranges Engine::galloc asks for: the grid points [wlo, whi) of every block behind a front halo"""
    rg = []
    for q in range(max(nblk, 1)):
        lo, hi = max(0, front + q * bstride + wlo), min(total, front + q * bstride + whi)
        if hi > lo:
            rg.append((lo * w, hi * w))
    return rg


G = GRAN
N_, H_ = 96 * 80 * 64, 96 * 80        # a grid and one plane of it as the front halo
FIXED = [
    ("unsorted", 20 * G, [(11 * G + 5, 12 * G + 9), (G, 2 * G), (5 * G + 1, 5 * G + 2)]),
    ("overlapping", 20 * G, [(G + 10, 4 * G + 10), (3 * G, 6 * G - 1), (2 * G, 2 * G + 1)]),
    ("touching at a granule boundary", 20 * G, [(2 * G, 4 * G), (4 * G, 5 * G), (8 * G, 9 * G), (7 * G + 1, 8 * G)]),
    ("inside one granule", 20 * G, [(3 * G + 100, 3 * G + 200)]),
    ("an empty range", 20 * G, [(5 * G, 5 * G), (7 * G + 3, 7 * G + 3), (9 * G, 8 * G), (G, G + 1)]),
    ("only empty ranges", 20 * G, [(5 * G, 5 * G)]),
    ("no range", 20 * G, []),
    ("a range past total", 6 * G, [(4 * G + 1, 9 * G), (10 * G, 12 * G)]),
    ("total not a multiple of the granule", 5 * G + 12345, [(0, 1), (5 * G + 1, 5 * G + 12345), (4 * G - 1, 4 * G)]),
    ("total inside the first granule", 1000, [(10, 900)]),
    ("three blocks behind a front halo", (3 * N_ + H_) * 4, galloc_ranges(3 * N_ + H_, H_, 3, N_, 20 * H_ - H_, 36 * H_ + H_, 4)),
    ("three blocks behind a front halo, float64, first slab", (3 * N_ + H_) * 8, galloc_ranges(3 * N_ + H_, H_, 3, N_, -H_, 16 * H_ + H_, 8)),
]


@pytest.mark.parametrize("name,total,ranges", FIXED, ids=[c[0] for c in FIXED])
def test_fixed_cases(granules, name, total, ranges):
    (merged,) = granules([(total, ranges)])
    check(total, ranges, merged)


def test_known_answers(granules):
    """a few answers written out by hand, so that the restatement above is not the only witness"""
    got = granules([(20 * G, [(11 * G + 5, 12 * G + 9), (G, 2 * G)]), (5 * G + 1, [(5 * G, 5 * G + 1), (0, 1)]), (6 * G, [(4 * G + 1, 9 * G)]),
                    (20 * G, [(2 * G, 4 * G), (4 * G, 5 * G)])])
    assert got == [[(G, 2 * G), (11 * G, 13 * G)], [(0, G), (5 * G, 6 * G)], [(4 * G, 6 * G)], [(2 * G, 5 * G)]]


def test_random_cases(granules):
    rng = np.random.default_rng(20261018)
    cases = []
    for _ in range(400):
        total = int(rng.integers(1, 40 * G))
        rg = []
        for _ in range(int(rng.integers(0, 9))):
            first = int(rng.integers(0, 44 * G))
            if rng.random() < 0.3:
                first = first // G * G                                    # on a granule boundary
            length = int(rng.choice([0, 1, G - 1, G, G + 1, int(rng.integers(0, 6 * G))]))
            last = first + length
            if rng.random() < 0.3:
                last = -(-last // G) * G
            if rng.random() < 0.05:
                first, last = last, first                                 # reversed: empty
            rg.append((first, last))
        if rg and rng.random() < 0.3:                                     # one that starts exactly where another ends
            rg.append((rg[0][1], rg[0][1] + int(rng.integers(1, 3 * G))))
        cases.append((total, rg))
    for (total, rg), merged in zip(cases, granules(cases)):
        check(total, rg, merged)


def test_header_is_host_only_and_listed():
    head = _read(os.path.join(CSRC, "sparse_granules.h"))
    assert "#include <hip" not in head and "sipx_common.h" not in head
    hdrs = re.search(r"^HDRS\s*=(.*)$", _read(os.path.join(CSRC, "Makefile")), re.M).group(1).split()
    assert "sparse_granules.h" in hdrs and "device_memory.h" in hdrs
