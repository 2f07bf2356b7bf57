"""The host rules of the whole-solve loop (csrc/solve_rules.h) against the numpy oracle, bit for bit, on the CPU.

tests/solve_rules/rules_driver.cpp is compiled with a plain host compiler against the header; it reads cases from stdin and
prints one answer line per case.  Numbers travel as hex floats, so "equal" means the same bits, for float and double."""
import itertools
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from oracle import parsdmm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
HEADER = os.path.join(CSRC, "solve_rules.h")
TYPES = [("f", np.float32), ("d", np.float64)]
YL_FEAS, YL_BB, YL_FIRST = 1, 2, 4      # include/sipx.h


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """rules(cases) -> one list of tokens per case; a case is a list of tokens (numbers become hex floats)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("solve_rules") / "rules_driver")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "solve_rules", "rules_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def tok(v):
        if isinstance(v, (bool, np.bool_)):
            return str(int(v))
        if isinstance(v, (int, np.integer, str)):
            return str(v)
        v = float(v)
        return "nan" if v != v else v.hex()

    def run(cases):
        text = "\n".join(" ".join(tok(v) for v in c) for c in cases) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [line.split() for line in out]
    return run


def _same(got, want):
    """a token of the driver against a value of the oracle: the same bits (every NaN is one value)"""
    g, w = float.fromhex(got), float(want)
    return (g != g and w != w) or (g == w and np.signbit(g) == np.signbit(w))


def _sw(adjust_rho=True, adjust_gamma=True, adjust_feas=True, freq=2, ind_ref=0):
    return [adjust_rho, adjust_gamma, adjust_feas, freq, ind_ref]


# ---- header hygiene ----------------------------------------------------------------------------------------------------------
def test_header_is_host_only_and_listed():
    head = _read(HEADER)
    assert "#include <hip" not in head and "sipx_common.h" not in head
    assert "solve_rules.h" in re.search(r"^HDRS\s*=(.*)$", _read(os.path.join(CSRC, "Makefile")), re.M).group(1).split()


def test_engine_holds_none_of_the_arithmetic():
    eng = _read(os.path.join(CSRC, "engine.cpp"))
    for pat in (r"\b1e4\b", r"%\s*10\b", r"\bi > 20\b", r"ind_ref \+ 25", r"\bi > 6\b", r"T\(0\.3\)"):
        assert not re.search(pat, eng), pat
    assert '#include "solve_rules.h"' in eng
    for name in ("julia_maximum", "bb_rule"):             # moved, not copied
        assert not re.search(r"^\S.*\b%s\(.*\{\s*$" % name, eng, re.M), name


# ---- bb_rule against bb_scalars ----------------------------------------------------------------------------------------------
def _bb_tuples(TF):
    """(d_dHh_dlh, n_d_H_hat, n_d_l_hat, n_d_l, n_d_G_hat, d_dGh_dl): hand-made for every branch, then random"""
    one, up, dn = TF(1), (lambda v: np.nextafter(TF(v), TF(np.inf))), (lambda v: np.nextafter(TF(v), TF(-np.inf)))
    sg = TF(1e-10) if TF == np.float64 else TF(1e-6)
    c = TF(0.3)
    good_a, good_b = (TF(0.5), one, one), (one, one, TF(0.5))        # correlation 0.5 on either side: sd - mg / 2
    none = (TF(0), TF(0), TF(0))
    hand = [none + none,                                             # neither estimate reliable
            good_a + none, none + good_b, good_a + good_b,           # alpha only, beta only, both
            (TF(0.5), one, TF(0.6)) + (TF(0.6), one, TF(0.5)),       # 2 mg > sd on both sides: the estimate is mg
            (TF(0.1), one, one) + (one, one, TF(0.1)),               # reliable, correlation 0.1: not used
            (TF(-0.5), one, one) + (one, one, TF(-0.5))]             # negative inner products
    for v in (dn(c), c, up(c)):                                      # correlation just below, at and just above 0.3
        hand += [(v, one, one) + none, none + (one, one, v), (v, one, one) + (one, one, v)]
    for v in (dn(sg), sg, up(sg)):                                   # the safeguard, each of its three conditions, both sides
        hand += [(v, TF(1e-3), TF(1e-3)) + none, none + (TF(1e-3), TF(1e-3), v),
                 (one, np.sqrt(v), one) + none, none + (one, np.sqrt(v), one),
                 (TF(0.5), one, v) + none, none + (v, one, TF(0.5)),
                 (TF(0.5), v, one) + none, none + (one, v, TF(0.5))]
    rng = np.random.default_rng(7)
    rand = []
    for _ in range(300):
        mag = 10.0 ** rng.uniform(-7 if TF == np.float64 else -5, 3, size=6)
        mag[[0, 5]] *= rng.choice([1.0, 1.0, 1.0, -1.0], size=2) * rng.uniform(0.05, 1.0, size=2)
        if rng.random() < 0.5:                                       # inner products consistent with the norms: correlations in (0, 1)
            mag[0] = mag[1] * mag[2] * rng.uniform(0.05, 1.0)
            mag[5] = mag[4] * mag[3] * rng.uniform(0.05, 1.0)
        rand.append(tuple(TF(v) for v in mag))
    return [tuple(TF(v) for v in t) for t in hand], rand


@pytest.mark.parametrize("code,TF", TYPES)
def test_bb_rule_equals_bb_scalars(rules, code, TF):
    hand, rand = _bb_tuples(TF)
    cases, want = [], []
    for t in hand + rand:
        for adjust_rho, adjust_gamma in itertools.product((False, True), repeat=2):
            rho, gamma = TF(10.0), TF(1.0)
            cases.append(["bb", code, *t, rho, gamma, adjust_rho, adjust_gamma])
            with np.errstate(all="ignore"):
                want.append(O.bb_scalars(TF, *t, rho, gamma, adjust_rho, adjust_gamma))
    got = rules(cases)
    for c, g, w in zip(cases, got, want):
        assert _same(g[0], w[0]) and _same(g[1], w[1]), (c, g, [float(v).hex() for v in w])
    # the hand-made tuples do reach every branch (read off the oracle's answers with both rules on)
    both_on = [w for c, w in zip(cases, want) if c[-2] and c[-1]][:len(hand)]
    gammas = {float(w[1]) for w in both_on}
    assert {float(TF(1.5)), float(TF(1.9)), float(TF(1.1))} <= gammas and len(gammas) > 3
    assert float(both_on[1][0]) == 1.75 and float(both_on[4][0]) == 0.5            # sd - mg / 2; mg
    k = 7
    for j in range(3):                                     # correlation below / at 0.3: unused; above: used
        used = [float(both_on[k + 3 * j + q][1]) != 1.5 for q in range(3)]
        assert used == [j == 2] * 3
    assert len({(float(w[0]).hex(), float(w[1]).hex()) for w in want[4 * len(hand):]}) > 100      # the random ones are not all one branch


# ---- the small rules ---------------------------------------------------------------------------------------------------------
NAN = float("nan")
ROWS = [[0.5], [0.1, 0.7, 0.7], [0.7, 0.1, 0.7], [3.0, 2.0, 1.0], [NAN, 1.0], [1.0, NAN, 5.0, NAN], [-np.inf, -np.inf], [np.inf, NAN],
        [0.0, -0.0], [1e-30, 1e30, 1e30]]


def test_julia_argmax(rules):
    rng = np.random.default_rng(3)
    rows = ROWS + [list(rng.integers(0, 4, size=rng.integers(1, 7)).astype(float)) for _ in range(50)]
    got = rules([["argmax", "d", len(r), *r] for r in rows])
    assert [int(g[0]) for g in got] == [O._julia_argmax(r) for r in rows]


@pytest.mark.parametrize("code,TF", TYPES)
def test_clamp_rho(rules, code, TF):
    lo, hi = TF(1e-2), TF(1e4)
    vals = [lo, hi, np.nextafter(lo, TF(0)), np.nextafter(lo, TF(1)), np.nextafter(hi, TF(0)), np.nextafter(hi, TF(np.inf)),
            TF(1e5), TF(1e-3), TF(0), TF(-1), TF(np.inf), TF(1), TF(10), TF(9999.5), TF(0.0100001)]
    got = rules([["clamp", code, v] for v in vals])
    for v, g in zip(vals, got):
        want = np.maximum(np.minimum(np.asarray([v], TF), TF(1e4)), TF(1e-2))[0]             # oracle: PARSDMM, the clamp
        assert _same(g[0], want), (v, g)
    assert float.fromhex(got[6][0]) == float(hi) and float.fromhex(got[7][0]) == float(lo)


@pytest.mark.parametrize("code,TF", TYPES)
def test_row_sum(rules, code, TF):
    rng = np.random.default_rng(5)
    rows = [list(TF(v) for v in rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)) for n in (1, 2, 3, 5, 8) for _ in range(10)]
    rows += [[TF(1), TF(NAN), TF(2)], [TF(1e30), TF(1), TF(-1e30)], [TF(np.inf), TF(1)]]
    got = rules([["sum", code, len(r), *r] for r in rows])
    with np.errstate(all="ignore"):
        for r, g in zip(rows, got):
            assert _same(g[0], O._seq_sum(r, TF)), r


def _next_rho_oracle(TF, sw, it, pp, row, rho):
    """The feasibility doubling and the clamp as oracle/parsdmm_oracle.py has them inline in PARSDMM, between the Barzilai-Borwein
    rule and the Q update ("if adjust_feasibility_rho and i % 10 == 0:" ... "rho = np.maximum(np.minimum(rho, TF(1e4)), TF(1e-2))",
    lines 1160-1165, src/PARSDMM.jl:213-226), with its own _julia_argmax.  Keep the two in step."""
    rho = np.asarray(rho, TF).copy()
    adjust_feasibility_rho = sw[2]
    if adjust_feasibility_rho and it % 10 == 0:
        if it > 10 and pp > 0:
            k = O._julia_argmax(row)
            rho[k] = TF(2.0) * rho[k]
    return np.maximum(np.minimum(rho, TF(1e4)), TF(1e-2))


@pytest.mark.parametrize("code,TF", TYPES)
def test_next_rho(rules, code, TF):
    rows = [[0.1, 0.7], [0.7, 0.1], [NAN, 0.5], [0.5, NAN], [0.3, 0.3]]
    rhos = [[1.0, 10.0, 100.0], [6000.0, 9000.0, 1.0], [1e5, 1e-3, 5.0], [1e4, 1e-2, 5e3], [float(np.nextafter(TF(5e3), TF(1e4))), 0.004, 0.006]]
    cases, want = [], []
    for it, feas, row, rho in itertools.product((9, 10, 11, 19, 20, 21, 30, 40), (False, True), rows, rhos):
        sw = _sw(adjust_feas=feas)
        rho = [TF(v) for v in rho]
        cases.append(["next", code, *sw, it, 2, 3, *row, *rho])
        want.append(_next_rho_oracle(TF, sw, it, 2, row, rho))
    got = rules(cases)
    doubled = 0
    for c, g, w in zip(cases, got, want):
        assert all(_same(a, b) for a, b in zip(g, w)) and len(g) == 3, (c, g, w)
        doubled += any(float(b) == 2 * float(a) for a, b in zip(c[-3:], w))
    assert doubled > 20


def test_yl_flags(rules):
    # expected: the oracle's conditions, inline there -- update_y_l "if i % 10 == 0" (line 930), PARSDMM "if i == 1" (1150) and
    # "(adjust_rho or adjust_gamma) and i % rho_update_frequency == 0" (1154)
    cases, want = [], []
    for ar, ag, freq, it in itertools.product((False, True), (False, True), (2, 3), range(1, 41)):
        cases.append(["flags", "d", *_sw(ar, ag, True, freq), it])
        want.append((YL_FEAS if it % 10 == 0 else 0) | (YL_FIRST if it == 1 else 0) | (YL_BB if (ar or ag) and it % freq == 0 else 0))   # oracle: update_y_l, PARSDMM
    assert [int(g[0]) for g in rules(cases)] == want


@pytest.mark.parametrize("code,TF", TYPES)
def test_prediction_never_says_cannot_where_rho_changes(rules, code, TF):
    """rho_may_change against next_rho, as an implication: "cannot" means that no Barzilai-Borwein step is due (flags) and that
    next_rho returns what it is given -- with the switches of the prediction, and with whatever the stop rule may have
    switched off in between."""
    rhos = [[1.0, 10.0, 100.0], [1e4, 1e-2, 5.0], [1e5, 1.0, 1.0], [1.0, 1e-3, 1.0], [float(np.nextafter(TF(1e4), TF(np.inf))), 1.0, 1.0]]
    rows = [[0.1, 0.7], [NAN, 0.5]]
    grid = list(itertools.product((2, 3), range(1, 41), (0, 2), itertools.product((False, True), repeat=3), rhos))
    may = rules([["may", code, *_sw(*adj, freq), it, pp, 3, *[TF(v) for v in rho]] for freq, it, pp, adj, rho in grid])
    may = [int(g[0]) for g in may]
    assert 0 in may and 1 in may
    cases, expect = [], []
    for (freq, it, pp, adj, rho), m in zip(grid, may):
        if m:
            continue
        rho = [TF(v) for v in rho]
        cases.append(["flags", code, *_sw(*adj, freq), it])
        expect.append(None)
        for later in (adj, (False, False, False)):             # the switches as they stood, and after a switch-off
            for row in rows:
                cases.append(["next", code, *_sw(*later, freq, it), it, pp, 3, *row[:pp], *rho])
                expect.append(rho)
    for c, g, e in zip(cases, rules(cases), expect):
        if e is None:
            assert int(g[0]) & YL_BB == 0, c
        else:
            assert all(_same(a, b) for a, b in zip(g, e)), (c, g)
    # and it is not "may" across the board: inside the clamp, with no rule due, nothing can change
    quiet = [m for (freq, it, pp, adj, rho), m in zip(grid, may) if rho == rhos[0] and it % freq and it % 10]
    assert quiet and not any(quiet)
    assert all(m for (freq, it, pp, adj, rho), m in zip(grid, may) if rho in rhos[2:])


# ---- stop_rule against stop_PARSDMM ------------------------------------------------------------------------------------------
def _oracle_steps(TF, lg, maxit, tol, sw):
    """the oracle's rule stepped over i = 1..maxit like the solve does; per iteration (stop, adjust_*, ind_ref), and why it stopped"""
    ar, ag, af, _, ind_ref = sw
    log = types.SimpleNamespace(**lg)
    tol = [TF(t) for t in tol]
    counter, steps, why = 2, [], "none"
    for i in range(1, maxit + 1):
        if i % 10 == 0:
            counter += 1
        before = (ar, ag, af, ind_ref)
        stop, ar, ag, af, ind_ref = O.stop_PARSDMM(log, i, tol[0], tol[1], tol[2], ar, ag, af, ind_ref, counter, TF)
        steps.append([int(stop), int(ar), int(ag), int(af), ind_ref])
        if stop:
            # which exit: ask again with the other two made impossible (a tolerance of zero: nothing is below it)
            z = TF(0)
            if O.stop_PARSDMM(log, i, z, tol[1], z, *before, counter, TF)[0]:
                why = "late"
            elif O.stop_PARSDMM(log, i, z, tol[1], tol[2], *before, counter, TF)[0]:
                why = "objective"
            else:
                why = "evol_x"
            break
    return steps, why


def _random_log(TF, seed, maxit=90, pp=2):
    rng = np.random.default_rng(seed)
    i = np.arange(1, maxit + 1)
    noise = lambda a: 1 + a * rng.uniform(-1, 1, maxit)
    lg = dict(obj=(rng.uniform(1, 100) * (1 + rng.uniform(0.1, 2) * rng.uniform(0.7, 0.97) ** i)),
              evol_x=rng.uniform(0.01, 1) * rng.uniform(0.8, 0.99) ** i * noise(0.3),
              r_pri_total=rng.uniform(0.1, 10) * rng.uniform(0.95, 1.02) ** i * noise(rng.choice([0.0, 0.05, 0.5])),
              set_feasibility=rng.uniform(0.01, 0.5) * (rng.uniform(0.3, 0.9) ** np.arange(maxit))[:, None] * rng.uniform(0.5, 1, (maxit, pp)))
    lg = {k: np.asarray(v, TF).astype(np.float64) for k, v in lg.items()}
    tol = (10.0 ** rng.uniform(-5, -2), 10.0 ** rng.uniform(-4, -1), 10.0 ** rng.uniform(-5, -2))
    return lg, maxit, tol


def _late_stop_log(TF, maxit=60):
    """r_pri_total constant for 25 iterations, then strictly increasing, evol_x large: the rules switch off at 26, the solve stops at 52"""
    i = np.arange(1, maxit + 1)
    lg = dict(obj=100.0 + 1.0 / i, evol_x=np.full(maxit, 0.5), r_pri_total=np.where(i <= 25, 1.0, 1.0 + 0.01 * (i - 25)),
              set_feasibility=np.full((maxit, 2), 0.5))
    return {k: np.asarray(v, TF).astype(np.float64) for k, v in lg.items()}, maxit, (1e-3, 1e-3, 1e-3)


def _window_log(TF, spike_at, maxit=70):
    """r_pri_total flat but for a spike of 5 at iteration `spike_at` and a 3 at iteration 60, whose window of fifty starts at 10"""
    i = np.arange(1, maxit + 1)
    lg = dict(obj=100.0 + 1.0 / i, evol_x=np.full(maxit, 0.5), r_pri_total=np.where(i == spike_at, 5.0, np.where(i == 60, 3.0, 1.0)),
              set_feasibility=np.full((maxit, 2), 0.5))
    return {k: np.asarray(v, TF).astype(np.float64) for k, v in lg.items()}, maxit, (1e-3, 1e-3, 1e-3)


def _settled_log(TF, maxit=40):
    """everything small from the start: stops at the first iteration that may (6: evol_x; 7 with evol_x off: objective)"""
    lg = dict(obj=np.full(maxit, 50.0), evol_x=np.full(maxit, 1e-6), r_pri_total=0.9 ** np.arange(maxit), set_feasibility=np.full((maxit, 2), 1e-6))
    return {k: np.asarray(v, TF).astype(np.float64) for k, v in lg.items()}, maxit


def _stop_case(code, lg, maxit, tol, sw):
    pp = lg["set_feasibility"].shape[1]
    return ["stop", code, *sw, maxit, pp, *tol, lg["set_feasibility"].shape[0], *lg["set_feasibility"].ravel(), *lg["obj"], *lg["evol_x"], *lg["r_pri_total"]]


@pytest.mark.parametrize("code,TF", TYPES)
def test_stop_rule_equals_stop_PARSDMM(rules, code, TF):
    problems = []                                          # (name, log, maxit, tolerances, switches)
    for seed in range(80):
        lg, maxit, tol = _random_log(TF, seed)
        problems.append(("random", lg, maxit, tol, _sw(ind_ref=maxit)))
    lg, maxit, tol = _late_stop_log(TF)
    problems.append(("late", lg, maxit, tol, _sw(ind_ref=maxit)))
    problems.append(("late, rules off from the start", lg, maxit, tol, _sw(False, True, True, ind_ref=0)))
    for spike_at in (9, 10):
        lg, maxit, tol = _window_log(TF, spike_at)
        problems.append(("window, spike at %d" % spike_at, lg, maxit, tol, _sw(ind_ref=maxit)))
    lg, maxit = _settled_log(TF)
    problems.append(("settled", lg, maxit, (1e-3, 1e-3, 1e-3), _sw(ind_ref=maxit)))
    problems.append(("settled, objective", lg, maxit, (0.0, 1e-3, 1e-3), _sw(ind_ref=maxit)))
    for name, key, at, tol in (("nan evol_x", "evol_x", 4, (1e-3, 0.0, 1e-3)), ("nan obj", "obj", 5, (0.0, 1e-3, 1e-3)),
                               ("nan feasibility", "set_feasibility", 0, (0.0, 1e-3, 1e-3))):
        bad = {k: v.copy() for k, v in lg.items()}
        if key == "set_feasibility":
            bad[key][0, 1] = NAN                           # the row the rule reads until iteration 10 fills the next one
        else:
            bad[key][at] = NAN
        problems.append((name, bad, maxit, tol, _sw(ind_ref=maxit)))
        problems.append((name + " (without the NaN)", lg, maxit, tol, _sw(ind_ref=maxit)))
    want = [_oracle_steps(TF, lg, maxit, tol, sw) for _, lg, maxit, tol, sw in problems]
    got = rules([_stop_case(code, lg, maxit, tol, sw) for _, lg, maxit, tol, sw in problems])
    for (name, *_), g, (steps, _) in zip(problems, got, want):
        assert [int(t) for t in g] == [v for s in steps for v in s], name
    # every exit is taken, read off the oracle's own answers
    by_name = {name: w for (name, *_), w in zip(problems, want)}
    whys = [why for _, why in want[:80]]
    switched_off = [any(a[1] and not b[1] for a, b in zip(steps, steps[1:])) for steps, _ in want[:80]]
    assert min(whys.count("objective"), whys.count("evol_x"), whys.count("none"), sum(switched_off)) >= 5, (whys, switched_off)
    steps, why = by_name["late"]
    assert why == "late" and len(steps) == 52 and steps[24][1:] == [1, 1, 1, 60] and steps[25][1:] == [0, 0, 0, 26]
    steps, why = by_name["late, rules off from the start"]
    assert why == "late" and len(steps) == 26            # the first iteration past ind_ref + 25, and the residual has grown
    assert by_name["window, spike at 9"][0][59][1:] == [0, 0, 0, 60] and by_name["window, spike at 10"][0][-1][1:] == [1, 1, 1, 70]      # outside / inside the fifty
    assert by_name["settled"][1] == "evol_x" and len(by_name["settled"][0]) == 6
    assert by_name["settled, objective"][1] == "objective" and len(by_name["settled, objective"][0]) == 7
    for name in ("nan evol_x", "nan obj", "nan feasibility"):      # a NaN in the window keeps the rule from stopping there
        assert len(by_name[name][0]) > len(by_name[name + " (without the NaN)"][0]), name
