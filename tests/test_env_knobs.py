"""The SIPX_* switches of the library: one table and one reader (csrc/env_knobs.h), one documented list.

Source scan: getenv only in the reader, every "SIPX_..." literal of csrc/ in the table, the table and the documented list
name the same switches, every name the tests and tools put into an environment is known, and the switches that were removed
are gone everywhere but from DESIGN_HISTORY.md.

Parser: tests/env_knobs/print_knobs.cpp is compiled with a plain host compiler against the header and prints the table for
a given environment; the expected values are written out from what each site did with its own getenv before the table
existed (unset, "0", "1" and the numbers the tests and tools pass)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
HEADER = os.path.join(CSRC, "env_knobs.h")

# read by host.py, multilevel.py, sharded.py, bench.py, the launcher, the tools or the test suite itself -- not by the library
PYTHON_SIDE = {"SIPX_LIBRARY", "SIPX_CONTEXT_CACHE", "SIPX_MULTILEVEL_CACHE", "SIPX_MULTILEVEL_SLAB_FULL", "SIPX_COMM", "SIPX_DECOMP",
               "SIPX_F64_VEC", "SIPX_DRY_COMM_CPU", "SIPX_RANK", "SIPX_WORLD", "SIPX_DEVICE", "SIPX_ID_FILE", "SIPX_NONCE",
               "SIPX_FORCE_DIST", "SIPX_FUZZ_RANDOM", "SIPX_FUZZ_SCALE"}
PYTHON_SIDE_PREFIX = "SIPX_BENCH_"

REMOVED = ["SIPX_" + s for s in (
    "FAN_OVERLAP", "FEAS_SAMPLE", "L1_LEAN", "LANE_PRIORITY", "RESID_AHEAD", "SET_STREAMS", "SLAB_LEAN_MULTI", "SLAB_LOOSE_SPARSE",
    "SPEC_BATCH", "SWEEP_PARTIAL", "X0_SNAPSHOT", "L1_CAPDIV", "L1_HWMAX", "SOLVE_COOP_MIN", "RANK_CHEB_BUDGET", "RANK_CHEB_GUARD",
    "RANK_CHEB_MMAX", "RANK_CHEB_TOL", "RANK_EPS", "RANK_FLOOR", "RANK_GUARDS")]


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _table_names():
    return set(re.findall(r'"(SIPX_[A-Z0-9_]+)"', _read(HEADER)))


def _csrc_files():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp")) or f == "Makefile")


def test_getenv_only_in_the_reader():
    users = [f for f in _csrc_files() if "getenv" in _read(os.path.join(CSRC, f))]
    assert users == ["env_knobs.h"]
    assert "env_knobs.h" in re.search(r"^HDRS\s*=(.*)$", _read(os.path.join(CSRC, "Makefile")), re.M).group(1).split()
    head = _read(HEADER)
    assert "#include <hip" not in head and "sipx_common.h" not in head


def test_every_literal_of_csrc_is_in_the_table():
    table = _table_names()
    assert len(table) == 44
    for f in _csrc_files():
        extra = set(re.findall(r'"(SIPX_[A-Z0-9_]+)"', _read(os.path.join(CSRC, f)))) - table
        assert not extra, (f, extra)


def test_table_and_documented_list_name_the_same_switches():
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    rows = set(re.findall(r"^\| `(SIPX_[A-Z0-9_]+)` \|", doc, re.M))
    assert rows == _table_names()
    for name in PYTHON_SIDE:
        assert name in doc, name
    assert PYTHON_SIDE_PREFIX + "*" in doc


def test_names_the_tests_and_tools_set_are_known():
    known = _table_names() | PYTHON_SIDE
    pats = [r'(?:setenv|delenv|setdefault|pop)\(\s*"(SIPX_[A-Z0-9_]+)"', r'environ\["(SIPX_[A-Z0-9_]+)"\]\s*=', r'env\["(SIPX_[A-Z0-9_]+)"\]\s*=',
            r'"(SIPX_[A-Z0-9_]+)"\s*:\s*"', r"\b(SIPX_[A-Z0-9_]+)="]
    seen = set()
    for sub in ("tests", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if not f.endswith((".py", ".sh", ".c", ".cpp", ".hip", ".jl")):
                    continue
                text = _read(os.path.join(d, f))
                for p in pats:
                    seen |= set(re.findall(p, text))
    unknown = {n for n in seen if n not in known and not n.startswith(PYTHON_SIDE_PREFIX)}
    assert not unknown, unknown
    assert {"SIPX_L1_ROUNDS_MAX", "SIPX_GATHER_CAP", "SIPX_YL_MULTI", "SIPX_RANK_LANE"} <= seen      # (the patterns do find them)


def _repository_files():
    """What belongs to the repository: git's own list where there is one, else every file outside the directories .gitignore names."""
    r = subprocess.run(["git", "ls-files", "-co", "--exclude-standard"], cwd=ROOT, capture_output=True, text=True)
    if r.returncode == 0 and r.stdout.strip():
        return [f for f in r.stdout.splitlines() if os.path.isfile(os.path.join(ROOT, f))]
    ignored = {".git", "__pycache__"} | {l.strip().strip("/").split("/")[-1] for l in _read(os.path.join(ROOT, ".gitignore")).splitlines()
                                        if l.strip().endswith("/")}
    out = []
    for d, dirs, files in os.walk(ROOT):
        dirs[:] = [x for x in dirs if x not in ignored]
        out += [os.path.relpath(os.path.join(d, f), ROOT) for f in files]
    return out


def test_removed_switches_are_gone():
    hits = []
    for rel in _repository_files():
        path = os.path.join(ROOT, rel)
        if rel.endswith((".so", ".o", ".a", ".pyc", ".npy", ".npz")) or rel == "DESIGN_HISTORY.md" or os.path.getsize(path) > (4 << 20):
            continue
        with open(path, "rb") as fh:
            data = fh.read()
        hits += [(rel, n) for n in REMOVED if re.search(n.encode() + rb"(?![A-Z0-9_])", data)]
    assert not hits, hits
    history = _read(os.path.join(ROOT, "DESIGN_HISTORY.md"))
    assert all(n in history for n in REMOVED)


# ---- parser ------------------------------------------------------------------------------------------------------------------
# name -> (field, {value: what the table must hold}); None = unset.  Written from the former sites:
#   !(e && e[0] == '0')   default on   -> 1, 0, 1          e && e[0] == '1'   default off  -> 0, 0, 1
#   atoi / atoll          numbers      -> the number       getenv(...) != nullptr          -> 0, 1, 1
#   SIPX_CG_FUSED   (e ? e[0] == '1' : by size)            -> -1 (by size), 0, 1
#   SIPX_LEAN_MULTI (by size unless set; lm[0] != '0')     -> -1 (by size), 0, 1
#   SIPX_SERIAL_SETS (serial iff '1'; set at all: no size rule) -> -1, 0, 1
#   SIPX_PREFAULT_THREADS (max(0, atoi); unset: by core count)  -> -1, 0, 1
#   SIPX_L1_ROUNDS_MAX: clamped to 1..rounds / 0..6 at its two sites, rounds <= 6: unset acts like 6
#   SIPX_FINALIZE_FAIL_RANK: compared with the rank; unset matches no rank
ON = {None: 1, "0": 0, "1": 1}
OFF = {None: 0, "0": 0, "1": 1}
PRESENT = {None: 0, "0": 1, "1": 1}
CASES = {
    "SIPX_CDS_MARCH": ("cds_march", {None: 1, "0": 0, "1": 1, "2": 2}),
    "SIPX_CDS_MARCH_ZCHUNK": ("cds_march_zchunk", {None: 0, "0": 0, "1": 1, "4": 4, "5": 5}),
    "SIPX_MULTI_ZCHUNK": ("multi_zchunk", {None: 0, "0": 0, "1": 1, "5": 5}),
    "SIPX_RHS_MARCH": ("rhs_march", {None: 1, "0": 0, "1": 1, "2": 2}),
    "SIPX_RHS_MARCH_ZCHUNK": ("rhs_march_zchunk", {None: 0, "0": 0, "1": 1, "5": 5}),
    "SIPX_Q_PLAN": ("q_plan", ON),
    "SIPX_Q_TABLE": ("q_table", ON),
    "SIPX_SERIAL_SETS": ("serial_sets", {None: -1, "0": 0, "1": 1}),
    "SIPX_CDS_FULL": ("cds_full", OFF),
    "SIPX_SLAB_CARD_GATHER": ("slab_card_gather", OFF),
    "SIPX_SLAB_DFT_GATHER": ("slab_dft_gather", OFF),
    "SIPX_SLAB_LOCAL": ("slab_local", ON),
    "SIPX_CG_FUSED": ("cg_fused", {None: -1, "0": 0, "1": 1}),
    "SIPX_YL_MULTI": ("yl_multi", ON),
    "SIPX_LEAN_MULTI": ("lean_multi", {None: -1, "0": 0, "1": 1}),
    "SIPX_SEARCH_BATCH": ("search_batch", ON),
    "SIPX_PASS_MULTI": ("pass_multi", OFF),
    "SIPX_SPEC_EXCHANGE": ("spec_exchange", ON),
    "SIPX_L1_SAMPLE": ("l1_sample", ON),
    "SIPX_RANK_LANE": ("rank_lane", ON),
    "SIPX_DFT_REAL": ("dft_real", ON),
    "SIPX_RANK_SUBSPACE": ("rank_subspace", ON),
    "SIPX_RANK_CHEB": ("rank_cheb", ON),
    "SIPX_RANK_PACK": ("rank_pack", ON),
    "SIPX_RANK_STRICT": ("rank_strict", OFF),
    "SIPX_COMM_GROUP": ("comm_group", ON),
    "SIPX_COMM_SELFTEST": ("comm_selftest", ON),
    "SIPX_GEMM_TUNE": ("gemm_tune", ON),
    "SIPX_PREFAULT_THREADS": ("prefault_threads", {None: -1, "0": 0, "1": 1, "16": 16}),
    "SIPX_TRACE_KERNELS": ("trace_kernels", OFF),
    "SIPX_TRACE_SEARCHES": ("trace_searches", OFF),
    "SIPX_MARK_STRIDE": ("mark_stride", {None: 0, "0": 0, "1": 1, "7": 7}),
    "SIPX_EXT_DEBUG": ("ext_debug", {None: 0, "0": 0, "1": 1, "2": 2, "3": 3}),
    "SIPX_SPEC_DEBUG": ("spec_debug", PRESENT),
    "SIPX_DFT_DEBUG": ("dft_debug", PRESENT),
    "SIPX_GEMM_TUNE_DEBUG": ("gemm_tune_debug", PRESENT),
    "SIPX_FINALIZE_FAIL_RANK": ("finalize_fail_rank", {None: -1, "0": 0, "1": 1}),
    "SIPX_COMM_SELFTEST_FAIL": ("comm_selftest_fail", {None: "", "mapped": "mapped", "base": "base", "alltoall:1": "alltoall:1", "mapped:0": "mapped:0"}),
    "SIPX_GATHER_CAP": ("gather_cap", {None: 0, "0": 0, "1": 1, "4": 4, "256": 256}),
    "SIPX_GATHER_FAST_CAP": ("gather_fast_cap", {None: 0, "0": 0, "1": 1, "8": 8}),
    "SIPX_L1_ROUNDS_MIN": ("l1_rounds_min", {None: 0, "0": 0, "1": 1, "6": 6}),
    "SIPX_L1_ROUNDS_MAX": ("l1_rounds_max", {None: 6, "0": 0, "1": 1}),
    "SIPX_L1_SAMPLE_RUNS": ("l1_sample_runs", {None: 0, "0": 0, "1": 1, "3": 3, "64": 64, "96": 96, "2048": 2048, "4096": 4096}),
    "SIPX_RANK_CERT_CHECK": ("rank_cert_check", PRESENT),
}


@pytest.fixture(scope="module")
def print_knobs(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("env_knobs") / "print_knobs")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "env_knobs", "print_knobs.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(**env):
        base = {k: v for k, v in os.environ.items() if not k.startswith("SIPX_")}
        base.update(env)
        out = subprocess.run([exe], env=base, capture_output=True, text=True, check=True).stdout
        return dict(line.split("=", 1) for line in out.splitlines())
    return run


def test_cases_cover_the_table():
    assert set(CASES) == _table_names()


def test_defaults(print_knobs):
    got = print_knobs()
    assert len(got) == len(CASES)
    for name, (field, want) in CASES.items():
        assert got[field] == str(want[None]), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_values(print_knobs, name):
    field, want = CASES[name]
    defaults = print_knobs()
    for value, expect in want.items():
        if value is None:
            continue
        got = print_knobs(**{name: value})
        assert got[field] == str(expect), (name, value)
        assert {k: v for k, v in got.items() if k != field} == {k: v for k, v in defaults.items() if k != field}, (name, value)
