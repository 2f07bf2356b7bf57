"""Every l1 threshold search of the engine against the exact threshold (tests/l1_exact.py), bit for bit.

A: the stand-alone projector.  B: the search of the iteration, call by call through the phase-level API, with the route
of every search asserted from the engine's diagnostics.  C: the searches of the feasibility estimates.  D: cardinality
sets in the same chains.  The oracle's arithmetic around the prox is the engine's own bits (test_phases_lockstep holds
the element-wise sets to array_equal under the same formulas), so the vector a search sees is captured inside the oracle's
prox and the engine's theta is checked on exactly that vector."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import card_exact as XC
from tests import l1_exact as X

pytestmark = pytest.mark.gpu

TFS = [np.float32, np.float64]
WORST = {}                       # precision -> largest |theta_e - theta*| / theta_tol seen so far (printed: pytest -rP)


def note(TF, r):
    if r is not None:
        k = np.dtype(TF).name
        WORST[k] = max(WORST.get(k, 0.0), r)
        print(f"theta error / theta_tol: {r:.3f} (largest so far in {k}: {WORST[k]:.3f})")


def heavy(rng, n, TF):
    return (rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(TF)


# =================================================================================================================
# A. the stand-alone projector
# =================================================================================================================
def vectors(TF):
    rng = np.random.default_rng(2025)
    out = []
    for n in (1, 5, 63, 64, 65, 1000, 4099):
        out.append((f"heavy-{n}", heavy(rng, n, TF)))
    n = 4099
    out.append(("twenty-octaves", (np.sign(rng.standard_normal(n)) * 2.0 ** rng.uniform(-10, 10, n)).astype(TF)))
    two = np.where(rng.random(n) < 0.3, 1.5, 0.75) * np.sign(rng.standard_normal(n))
    out.append(("two-valued", two.astype(TF)))
    z = heavy(rng, n, TF)
    z[::3] = 0
    z[1::7] = TF(-0.0)
    out.append(("zeros", z))
    out.append(("all-active", ((2.0 + rng.random(1000)) * np.sign(rng.standard_normal(1000))).astype(TF)))
    return out


@pytest.mark.parametrize("TF", TFS)
def test_projector_is_the_exact_threshold(sipx, TF):
    g = sipx.compgrid((1.0, 1.0), (10, 10))
    for name, v in vectors(TF):
        a1 = float(np.abs(v.astype(np.float64)).sum())
        for frac in (0.01, 0.3, 0.6, 0.999) + ((0.8,) if name == "all-active" else ()):
            b = float(TF(frac * a1))
            P = sipx.Projector(sipx.set_definitions("l1", "identity", 0.0, b, ("matrix", "")), g, TF)
            y = P(v.copy())
            try:
                X.check_l1_output(v, y, b)
            except AssertionError as e:
                raise AssertionError(f"{name}, radius {frac} ||v||_1: {e}") from None
        w = (v * TF(0.25)).astype(TF)               # feasible for the last radius: back bit for bit
        assert X.same_bits(P(w.copy()), w), name


def cluster_vector(rng, n, TF):
    """n magnitudes within 1 % of theta (b = 1e-4 n, theta* about 0.99943) whose COLD bracket holds 95 % of them: 4 % at
    0.99, 95 % uniform in [0.9993, 0.9997], 1 % at 1.0001.  The cold decision (decide_body, no probes yet) brackets theta
    between the Newton step from 0, mean - b / n, and the secant from vmax, vmax (1 - b / ||v||_1): (0.99903, 0.99999].  It
    estimates what that bracket holds from its share of [0, vmax], a few hundred, so no refinement pass narrows it."""
    u = rng.random(n)
    a = np.where(u < 0.04, 0.99, np.where(u < 0.99, 0.9993 + 0.0004 * rng.random(n), 1.0001))
    return (a * np.sign(rng.standard_normal(n))).astype(TF)


def cold_bracket(v, b):
    """(lo, hi, estimated population) of decide_body's first decision of a cold search: virtual probes 0 and vmax."""
    a = np.abs(v.astype(np.float64))
    S, C, vmax = a.sum(), float((a > 0).sum()), a.max()
    lo = (S - b) / C * (1.0 - 1e-9)
    hi = min((S - b) * vmax / S * (1.0 + 1e-9), vmax)
    return lo, hi, C * min(1.0, 2.0 * (hi - lo) / vmax)


@pytest.mark.parametrize("TF", TFS)
def test_projector_on_a_vector_whose_cold_bracket_holds_2_to_the_17(sipx, TF):
    """Just above L1_CAP = 131072 entries, all within 1 % of theta.  By the engine's rule of the cold decision (restated in
    cold_bracket) the compaction gathers more than 2^17 = SOLVE_COOP_MIN magnitudes without a refinement pass in front, which
    is when the 32 workgroups of k_l1_solve share the sweeps.  The stand-alone projector hands out no diagnostics: that the
    same cold search on the same vector does gather that many and is solved cooperatively is asserted through a context, case
    "coop-cold" below."""
    n = 140000
    v = cluster_vector(np.random.default_rng(7), n, TF)
    b = float(TF(1e-4 * n))
    a = np.abs(v.astype(np.float64))
    lo, hi, pop = cold_bracket(v, b)
    th = X.exact_theta(a, b)[0]
    assert lo < th <= hi and np.all(np.abs(a / th - 1) < 0.01)
    assert int(((a > lo) & (a <= hi)).sum()) >= 2 ** 17 and pop < 131072.0
    g = sipx.compgrid((1.0, 1.0), (10, 10))
    P = sipx.Projector(sipx.set_definitions("l1", "identity", 0.0, b, ("matrix", "")), g, TF)
    X.check_l1_output(v, P(v.copy()), b)


# =================================================================================================================
# B - D. chains of y/l updates with x fixed
# =================================================================================================================
# A set of a chain: (kind, operator, data, radius, plan).
#   kind "l1":    data names the vector the FIRST search sees (l0 = rho (s - w), so v_1 = s - l0 / rho is w up to rounding):
#                   "heavy"   randn * exp(randn), scaled to four times the mean magnitude of s = A x
#                   "uniform" magnitudes uniform in [0, 4 mean|s|]
#                   "two"     two-valued magnitudes {1, 1.002} mean|s| (almost everything inside a 1 % range around theta)
#                   "s"       l0 = 0: the first search sees s = A x itself
#                 radius: fraction of ||w||_1
#   kind "card" / "cardf": l0 = 0, k = 30 % of the rows / of a slice
# plan: one (rho factor, gamma, route) per call; rho_k = rho_{k-1} * factor, both per set.  With x fixed and gamma small,
#   v_{k+1} = v_k + gamma (s - v_k + theta_k sgn) on the active entries: gamma steers how far theta moves.  A change of rho
#   rescales the multiplier term (and the engine's prediction of theta with it).  After a feasible call l is zero and
#   y = v, so only a gamma outside [0, 2] -- an extrapolation, v = s - (1 - gamma)(y - s) -- makes the set infeasible again.
# Routes (asserted from debug_proj and, in the batched chain, from the launches of the call):
#   cold        no previous theta; fallback sweeps
#   hit         warm, full first pass, spec_ok == 1, no fallback pass
#   lean        the previous solve announced a lean pass (lean == 1) and it settled the search (spec_ok == 1)
#   lean-miss   lean pass, theta left the range: refinement pass + compaction (the `refine` word itself is zero again
#               once the stage-1 decision has run: the launched k_pass<M_PROBE> is what shows it)
#   window      full first pass, theta outside the speculative range but inside the outermost probes (64 hw)
#   beyond      full first pass, theta beyond the outermost probe
#   lean-far    lean pass, theta beyond where the outermost probe of a full pass would have been: the same two sweeps
#   overflow    the speculative gather overflowed a workgroup's LDS buffer (overflow > 0), fallback sweeps
#   sampled     the probes were centred by the sampled estimate (sampled == 1)
#   cold-refine cold, and the bracket held so much that a refinement pass ran behind the full first pass
#   beyond-refine  as beyond, and the bracket between the outermost probe and the end of the axis held so much that a refinement
#               pass ran (single-set case: the launch is this set's)
#   coop        k_l1_solve, launched with its SOLVE_G workgroups by a per-set chain (the batched chain solves a settled search
#               inside k_spec_finish with one workgroup per set), on 2^17 gathered magnitudes or more: cooperative sweeps, and
#               michelot_its is not the -1 of an abandoned barrier
#   feasible    need == 0, y = v
#   stale       the first infeasible search after a feasible call (theta_prev is stale)
#   any         not part of the table (the set only accompanies the others)
G, S = 1e-4, 3e-2          # gammas: theta moves by about a hundredth of a percent / by a few percent


def plan(*steps):
    return list(steps)


HITS = plan((1, 1, "cold"), (1, G, "hit"), (1, G, "lean"), (1, S, "lean-miss"), (1, S, "window"), (1, G, "hit"), (1, 1, "lean-far"))
# (call 5: rho doubles, the multiplier term and theta with it halve; the prediction rescaled by rho_old / rho_new holds)
FAR = plan((1, 1, "cold"), (1, 1, "beyond"), (1, G, "hit"), (1, G, "lean"), (2, G, "lean"), (1, G, "lean"), (1, G, "lean"))
FEAS = plan((1, 1, "cold"), (1, G, "hit"), (16, 1, "feasible"), (1, -31, "stale"), (1, G, "hit"), (16, 1, "feasible"), (1, -31, "stale"))
SHORT = plan((1, 1, "cold"), (1, G, "hit"), (1, G, "lean"))
CARD3 = plan(*[(1, 1, "card")] * 3)
ALLACT = plan((1, 1, "cold"), (1, G, "hit"), (1, G, "hit"))      # (every entry active: the solve never announces a lean pass)

CASES = {
    # the headline list; n1 % 4 == 0: the vector kernels, the searches batched, another route per set in one call
    "c3-vec": dict(n=(36, 20, 9), batched=True, sets=[("bounds",), ("l1", "D_x", "heavy", 0.3, HITS), ("l1", "D_y", "heavy", 0.5, FAR),
                                        ("l1", "D_z", "heavy", 0.5, FEAS)]),
    # odd n1: one scalar pass per set
    "c3-odd": dict(n=(33, 17, 6), sets=[("bounds",), ("l1", "D_x", "heavy", 0.3, HITS), ("l1", "D_y", "heavy", 0.5, FAR),
                                        ("l1", "D_z", "heavy", 0.5, FEAS)]),
    # three blocks (two in 2-D), M != N, pads inside the vector
    "tv-3d": dict(n=(36, 20, 9), sets=[("bounds",), ("l1", "TV", "heavy", 0.3, HITS)]),
    "tv-2d": dict(n=(33, 27), sets=[("bounds",), ("l1", "TV", "heavy", 0.4, FAR)]),
    # identity, every entry active (the lv - 1 cap of the scan)
    # (the probes bracket Michelot's root (||v||_1 - b) / lv; theta is the reference's (||v||_1 - min|v| - b) / (lv - 1), 1 % below it
    #  at lv = 720 and min|v| = 8 theta: once the range has narrowed to 0.2 % the bracket misses it -- two more sweeps, the same theta)
    "l1id": dict(n=(36, 20), x="band", all_active=True,
                 sets=[("bounds",), ("l1", "identity", "s", 0.9, plan((1, 1, "cold"), (1, G, "hit"), (1, G, "window")))]),
    # all-active on D_z: |D_z x| in [2, 3], b = 0.8 ||.||_1 -- a pad counted as a zero element changes min|v| and lv - 1
    "all-active-dz-vec": dict(n=(36, 20, 9), x="ramp-z", all_active=True, sets=[("bounds",), ("l1", "D_z", "s", 0.8, ALLACT)]),
    "all-active-dz-odd": dict(n=(33, 17, 6), x="ramp-z", all_active=True, sets=[("bounds",), ("l1", "D_z", "s", 0.8, ALLACT)]),
    # the per-set chains on the set streams, the per-set y/l kernels, the sampled prediction on a small grid
    "per-set-chains": dict(n=(36, 20, 9), batched=False, env={"SIPX_SEARCH_BATCH": "0"},
                           sets=[("bounds",), ("l1", "D_x", "heavy", 0.3, HITS), ("l1", "D_z", "heavy", 0.5, FEAS)]),
    "per-set-yl": dict(n=(36, 20, 9), batched=False, env={"SIPX_YL_MULTI": "0"},
                       sets=[("bounds",), ("l1", "D_x", "heavy", 0.3, HITS), ("l1", "D_z", "heavy", 0.5, FAR)]),
    "sampled": dict(n=(36, 20, 9), env={"SIPX_L1_SAMPLE_RUNS": "16"},
                    sets=[("bounds",), ("l1", "D_x", "heavy", 0.3, plan((1, 1, "cold"), (1, 1, "sampled"), (1, S, "any"), (1, 1, "sampled"))),
                          ("l1", "D_z", "heavy", 0.5, plan((1, 1, "cold"), (1, G, "any"), (2, G, "any"), (1, 1, "any")))]),
    # Speculative overflow: a workgroup of the SIPX_PASS_GRID launch sweeps BLOCK * 4 = 1024 grid points per round and offers
    # nblk magnitudes per point to its LDS buffer of SPEC_CAP = 1024 values; below 5 * CUs * 1024 grid points there is one
    # round, so one block per point can never overflow: the smallest case is a two-block operator (TV in 2-D) on a grid that
    # fills one workgroup, 1024 = 32 x 32 points -- 1984 magnitudes, nearly all of them within the range.
    "overflow": dict(n=(32, 32), sets=[("bounds",), ("l1", "TV", "two", 0.001, plan((1, 1, "cold"), (1, G, "overflow"), (1, G, "any")))]),
    # A refinement pass behind a FULL first pass needs more than max(L1_CAP = 131072, len / 64) magnitudes in the bracket the
    # Newton / secant steps leave, counted as C * min(1, 2 (hi - lo) / vmax) (decide_body).  Magnitudes uniform in [0, 1] with
    # b = ||v||_1 / 4: theta* = 1/2, Newton from 0 gives 3/8, the secant from vmax 3/4, so 3/4 of the 193536 rows count.
    "cold-refine": dict(n=(64, 64, 48), batched=True,
                        sets=[("bounds",), ("l1", "D_x", "uniform", 0.25, plan((1, 1, "cold-refine"), (1, G, "hit")))]),
    # ... and behind the full first pass of a WARM search: b = 0.9 ||v||_1 leaves a small theta; gamma = 3 (an extrapolation, as
    # after a feasible call) then moves it 17 times up, beyond the outermost probe, and the bracket (1.64 theta_prev, vmax] holds
    # nearly every magnitude.
    "warm-refine": dict(n=(64, 64, 48), batched=True,
                        sets=[("bounds",), ("l1", "D_x", "uniform", 0.9, plan((1, 1, "cold"), (1, 3, "beyond-refine"), (1, G, "hit")))]),
    # Two-valued magnitudes on the same grid, per-set chains (SIPX_SEARCH_BATCH=0: k_l1_solve on SOLVE_G = 32 workgroups): the
    # second search gathers all 193536 of them through the speculative range (at most 1024 per workgroup: no overflow with one
    # block per point), more than SOLVE_COOP_MIN = 2^17, so the sweeps of the solve are shared.
    "coop": dict(n=(64, 64, 48), batched=False, env={"SIPX_SEARCH_BATCH": "0"},
                 sets=[("bounds",), ("l1", "D_x", "two", 0.001, plan((1, 1, "cold"), (1, G, "coop")))]),
    # The vector of the stand-alone test above as x of an identity set (l0 = 0: the first search sees x): the COLD search's
    # compaction gathers 95 % of 140000 magnitudes, solved cooperatively; the warm one gathers them through the range.
    "coop-cold": dict(n=(400, 350), x="cluster", batched=False, env={"SIPX_SEARCH_BATCH": "0"},
                      sets=[("bounds",), ("l1", "identity", "s", ("per-entry", 1e-4), plan((1, 1, "coop"), (1, G, "coop")))]),
    # D: cardinality in the same chains (integer x, rho a power of two: the tie groups survive the arithmetic)
    "card-dz": dict(n=(36, 20, 9), x="integers", sets=[("bounds",), ("l1", "D_x", "heavy", 0.3, SHORT), ("card", "D_z", plan(*[(1, 1, "card")] * 3))]),
    "cardf-dy": dict(n=(36, 20, 9), x="integers", sets=[("bounds",), ("l1", "D_z", "heavy", 0.3, SHORT),
                                                         ("cardf", "D_y", ("slice", "z"), plan(*[(1, 1, "card")] * 3))]),
    # the whole-vector search on its hostile inputs (tests/test_gpu_card_exact.py drives and checks these)
    # |D_z x| in {0, 1}: 23040 rows, about 11500 ones -- one tie group above CARD_CAP; n1 % 4 == 0: the vector kernel
    "card-dz-big-vec": dict(n=(48, 32, 16), x="binary", sets=[("bounds",), ("card", "D_z", CARD3)]),
    "card-dz-big-odd": dict(n=(45, 32, 17), x="binary", sets=[("bounds",), ("card", "D_z", CARD3)]),          # the scalar kernel
    # three padded blocks (two in 2-D), M != N: the index order across blocks and pads decides who survives
    "card-tv-3d": dict(n=(36, 20, 9), x="integers", sets=[("bounds",), ("card", "TV", CARD3)]),
    "card-tv-2d": dict(n=(33, 27), x="integers", sets=[("bounds",), ("card", "TV", CARD3)]),
    # the outlier stretches (0, vmax]: the five passes of the cold search run out with everything but the outlier in the bracket
    "card-id-outlier": dict(n=(120, 100), x="outlier", sets=[("bounds",), ("card", "identity", CARD3)]),
    # call 2, gamma = 3 (an extrapolation, as after a feasible call of an l1 set): the dropped entries come back four times as
    # large, tau more than doubles -- the warm bracket (2 tau_prev, vmax]; call 3, rho * 16: the multiplier term all but
    # vanishes, v is s = A x again and tau the first call's, less than half of the second's -- the warm bracket (0, tau_prev / 2]
    "card-moves": dict(n=(48, 32, 16), x="heavy", sets=[("bounds",), ("card", "D_z", plan((1, 1, "card"), (1, 3, "card"), (16, 1, "card")))]),
}


def make_x(kind, n, TF, rng):
    if kind == "ramp-z":                     # differences along z of magnitude in [2, 3], random signs
        d = (2.0 + rng.random(n)) * np.sign(rng.standard_normal(n))
        return np.cumsum(d, axis=len(n) - 1).astype(TF).reshape(-1, order="F")
    if kind == "band":                       # magnitudes in [2, 3]
        return ((2.0 + rng.random(n)) * np.sign(rng.standard_normal(n))).astype(TF).reshape(-1, order="F")
    if kind == "cluster":
        return cluster_vector(rng, int(np.prod(n)), TF)
    if kind == "integers":
        return rng.integers(0, 6, n).astype(TF).reshape(-1, order="F")
    if kind == "binary":                     # layers of equal jumps: |D_z x| is 0 or 1
        return rng.integers(0, 2, n).astype(TF).reshape(-1, order="F")
    if kind == "outlier":                    # magnitudes in [1, 2] and one entry of 1e9 (tests/card_exact.py, `outlier`)
        x = ((1.0 + rng.random(n)) * np.sign(rng.standard_normal(n))).astype(TF).reshape(-1, order="F")
        x[len(x) // 3] = TF(1e9)
        return x
    if kind == "heavy":
        return heavy(rng, int(np.prod(n)), TF)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    return (2.0 * z + rng.standard_normal(n)).astype(TF).reshape(-1, order="F")


def build(mod, n, TF, sets, radii, cards):
    h = tuple(1.0 for _ in n)
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF)
    c = []
    for i, s in enumerate(sets):
        if s[0] == "bounds":
            c.append(mod.set_definitions("bounds", "identity", -1.0, 1.5, ("matrix", "")))
        elif s[0] == "l1":
            c.append(mod.set_definitions("l1", s[1], 0.0, radii[i], ("matrix", "")))
        elif s[0] == "card":
            c.append(mod.set_definitions("cardinality", s[1], 0, cards[i], ("matrix", "")))
        else:
            c.append(mod.set_definitions("cardinality", s[1], 0, cards[i], s[2]))
    P, A, prop = mod.setup_constraints(c, g, TF)
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


class Chain:
    """One context, x fixed; step() makes one ctx.update_y_l and replays it in the oracle from the engine's own state.
    sipx = None: no engine at all -- oracle_step() advances the same chain in the oracle alone (what the ranks of a
    slab-decomposed context are held to by a parent that has no context of its own)."""

    def __init__(self, sipx, case, TF, rho0=8.0, stats=True, **ctx_kw):
        """ctx_kw: device, owned, attach of host.build_context (a rank of a slab-decomposed context)."""
        self.sipx, self.TF, self.stats = sipx, TF, stats
        n, sets = case["n"], case["sets"]
        rng = np.random.default_rng(len(n) * 1000 + n[0])
        go = O.compgrid(tuple(1.0 for _ in n), n)
        self.x = make_x(case.get("x", "model"), n, TF, rng)
        self.m = (self.x + TF(0.1) * rng.standard_normal(len(self.x)).astype(TF)).astype(TF)
        self.sets, self.p = sets, len(sets) + 1
        self.l1 = [i for i, s in enumerate(sets) if s[0] == "l1"]
        self.card = [i for i, s in enumerate(sets) if s[0] in ("card", "cardf")]
        self.rho = np.full(self.p, rho0)
        radii, cards, l0, y0 = {}, {}, [], []
        self.b = {}
        for i, s in enumerate(sets):
            op = "identity" if s[0] == "bounds" else s[1]
            Ai, _, _, tdn, _ = O.get_TD_operator(go, op, TF)
            sv = O.csc_mul(Ai, self.x)
            M = len(sv)
            li = np.zeros(M, TF)
            if s[0] == "bounds":
                li = rng.standard_normal(M).astype(TF)
            elif s[0] == "l1":
                ms = float(np.abs(sv.astype(np.float64)).mean())
                if s[2] == "heavy":
                    w = heavy(rng, M, np.float64)
                    w = (w * (4.0 * ms / np.abs(w).mean())).astype(TF)
                elif s[2] == "uniform":
                    w = (rng.random(M) * 4.0 * ms * np.sign(rng.standard_normal(M))).astype(TF)
                elif s[2] == "two":
                    w = (np.where(rng.random(M) < 0.5, 1.0, 1.002) * ms * np.sign(rng.standard_normal(M))).astype(TF)
                else:
                    w = sv
                if s[2] != "s":
                    li = (TF(rho0) * (sv - w)).astype(TF)
                if isinstance(s[3], tuple):              # ("per-entry", beta): b = beta * rows
                    radii[i] = float(TF(s[3][1] * M))
                else:
                    radii[i] = float(TF(s[3] * float(np.abs(w.astype(np.float64)).sum())))
                self.b[i] = radii[i]
            elif s[0] == "card":
                cards[i] = int(case.get("card_frac", 0.3) * M)
            else:
                ax = {"x": 0, "y": 1, "z": len(n) - 1}[s[2][1]]
                cards[i] = max(1, int(0.3 * (int(np.prod(tdn)) // tdn[ax])))
            l0.append(li)
            y0.append(sv.copy())
        l0.append(rng.standard_normal(len(self.x)).astype(TF))          # the distance term
        y0.append(self.x.copy())
        self.cards = cards
        self.go, self.oo, self.Po, self.Ao, self.propo, _ = build(O, n, TF, sets, radii, cards)
        self.ctx = None
        if sipx is not None:
            gs, os_, Ps, As, props, AtAs = build(sipx, n, TF, sets, radii, cards)
            os_.zero_ini_guess = False
            os_.rho_ini = [float(r) for r in self.rho]
            self.ctx = sipx.host.build_context(self.m, AtAs, As, props, Ps, gs, os_, x=self.x, l=l0, y=y0, **ctx_kw)
        self.y, self.l = [v.copy() for v in y0], [v.copy() for v in l0]
        self.diag = {i: None for i in self.l1}
        self.batched = None
        self.calls = 0

    def close(self):
        if self.ctx is not None:
            self.ctx.close()

    def oracle_step(self, factors, gamma):
        """The same call in the oracle alone.  Returns {cardinality set: dict(v, y, l)} and advances y, l."""
        TF, p = self.TF, self.p
        self.rho = self.rho * np.asarray(factors, np.float64)
        rho, gam = self.rho.astype(TF), np.asarray(gamma, np.float64).astype(TF)
        seen = {}

        def card_prox(i):
            def f(v):
                seen[i] = v.copy()
                return self.Po[i](v)
            return f
        prox = [card_prox(i) if i in self.card else self.Po[i] for i in range(p - 1)]
        prox.append(lambda v: O.prox_l2s(v, rho[p - 1], self.m))
        z = lambda: [np.zeros(self.Ao[i].shape[0], TF) for i in range(p)]

        class L:
            pass
        log = L()
        log.r_pri = np.zeros((1, p)); log.r_dual = np.zeros((1, p)); log.set_feasibility = np.zeros((1, p - 1))
        O.update_y_l(self.x.copy(), p, 1, self.y, z(), self.l, z(), rho, gam, prox, self.Ao, log, self.Po, 1, z(), z(), z())
        self.calls += 1
        return {i: dict(v=seen[i], y=self.y[i].copy(), l=self.l[i].copy()) for i in self.card}

    def step(self, factors, gamma, flags=0, it=1):
        """One call.  Returns {set: record}; every l1 / cardinality set has been checked when it returns."""
        TF, p, ctx = self.TF, self.p, self.ctx
        self.rho = self.rho * np.asarray(factors, np.float64)
        rho, gam = self.rho.astype(TF), np.asarray(gamma, np.float64).astype(TF)
        c0 = ctx.kernel_stats_all(-1)["batched_searches"]
        if self.stats:                        # (the launches of this call: asserted on in the batched chain only)
            ctx.kernel_stats_all(2)
        rp, rd, fe = ctx.update_y_l(it, flags, rho.astype(np.float64), gam.astype(np.float64))
        launches = {k["name"]: k["launches"] for k in ctx.kernel_stats_all(0)["kernels"]} if self.stats else {}
        c1 = ctx.kernel_stats_all(-1)["batched_searches"]
        # searches this call sent through the batched chain, and how many of them needed their fallback sweeps
        self.batched = (c1["searches"] - c0["searches"], c1["fallbacks"] - c0["fallbacks"])
        _, le, ye = ctx.download()
        dg = {i: ctx.debug_proj(i, 0) for i in self.l1}
        dgc = {i: ctx.debug_proj(i, 0) for i in self.card}      # need, lo, hi, vmax, gathered (n_compact at the selection), refine
        # the oracle from the state the engine had before the call; the l1 prox thresholds with the ENGINE's theta
        seen = {}

        def l1_prox(i):
            def f(v):
                seen[i] = v.copy()
                return X.soft(v, TF(dg[i]["theta"])) if dg[i]["need"] else v
            return f

        def card_prox(i):
            def f(v):
                seen[i] = v.copy()
                return self.Po[i](v)
            return f
        prox = [l1_prox(i) if i in self.l1 else card_prox(i) if i in self.card else self.Po[i] for i in range(p - 1)]
        prox.append(lambda v: O.prox_l2s(v, rho[p - 1], self.m))
        z = lambda: [np.zeros(self.Ao[i].shape[0], TF) for i in range(p)]
        y, l = [v.copy() for v in self.y], [v.copy() for v in self.l]

        class L:
            pass
        log = L()
        log.r_pri = np.zeros((1, p)); log.r_dual = np.zeros((1, p)); log.set_feasibility = np.zeros((1, p - 1))
        O.update_y_l(self.x.copy(), p, 1, y, z(), l, z(), rho, gam, prox, self.Ao, log, self.Po, 1, z(), z(), z())
        out = {}
        for i in self.l1:
            d, v = dg[i], seen[i]
            tag = f"call {self.calls + 1}, set {i}"
            try:
                r = X.check_l1_output(v, ye[i], self.b[i], d["theta"])
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}; diagnostics {d}") from None
            note(TF, r)
            assert X.same_bits(le[i], l[i]), f"{tag}: l is not the oracle's bit for bit"
            fz = X.feasibility(v, self.b[i])
            if fz > 0:
                assert d["need"] == 0 and X.same_bits(ye[i], v), tag
            if fz < 0:
                assert d["need"] == 1, tag
            out[i] = dict(d=d, prev=self.diag[i], v=v, launches=launches, fz=fz)
        for i in self.card:
            assert X.same_bits(ye[i], y[i]), f"call {self.calls + 1}, cardinality set {i}: y is not the oracle's bit for bit"
            assert X.same_bits(le[i], l[i]), f"call {self.calls + 1}, cardinality set {i}: l"
            if self.sets[i][0] == "card":
                try:
                    XC.check_card_output(seen[i], ye[i], self.cards[i])
                except AssertionError as e:
                    raise AssertionError(f"call {self.calls + 1}, cardinality set {i}: {e}; diagnostics {dgc[i]}") from None
            out[i] = dict(v=seen[i], y=ye[i], d=dgc[i])
        self.y, self.l = ye, le
        self.diag = dg
        self.calls += 1
        self.last = dict(rp=rp, rd=rd, fe=fe, rho=rho)
        return out


def route_of(rec, batched, rescaled):
    """What the diagnostics say the search did (see the legend above)."""
    d, prev, ln = rec["d"], rec["prev"], rec["launches"]
    if not d["need"]:
        return "feasible"
    names = []
    if prev is None or not prev["theta_prev"] > 0:
        names.append("cold")
    elif not prev["need"]:
        names.append("stale")
    if d["sampled"]:
        names.append("sampled")
    if d["overflow"] > 0:
        names.append("overflow")
    elif d["spec_ok"]:
        names.append("lean" if (prev is not None and prev["lean"]) else "hit")
    elif prev is not None and prev["theta_prev"] > 0 and not rescaled and not d["sampled"]:
        c, hw = 0.5 * (prev["spec_hi"] + prev["spec_lo"]), 0.5 * (prev["spec_hi"] - prev["spec_lo"])
        far = abs(d["theta"] - c) > 64 * hw
        if prev["lean"]:
            names.append("lean-far" if far else "lean-miss")
        else:
            names.append("beyond" if far else "window")
    if not batched and d["gathered"] >= 2 ** 17 and d["michelot_its"] > 0:
        names.append("coop")
    if batched and not d["spec_ok"]:
        assert ln.get("k_pass<M_COMPACT>", 0) >= 1, "a search without spec_ok must have run its compaction pass"
        if rec["alone"] and ln.get("k_pass<M_PROBE>", 0) >= 1:      # (the only fallback of the call: the launch is this set's)
            names += [r + "-refine" for r in ("cold", "beyond") if r in names]
    return "+".join(names)


def run_case(sipx, TF, name, monkeypatch, after_call=None):
    case = CASES[name]
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    # "batched": True -- the searches must go through the batched chain; False -- they must not; absent -- as the engine decides
    want_batched = case.get("batched")
    ch = Chain(sipx, case, TF, stats=want_batched is not False)
    try:
        plans = {i: s[-1] for i, s in enumerate(case["sets"]) if s[0] != "bounds"}
        ncalls = max(len(pl) for pl in plans.values())
        for k in range(ncalls):
            fac, gam = np.ones(ch.p), np.ones(ch.p)
            for i, pl in plans.items():
                if k < len(pl):
                    fac[i], gam[i] = pl[k][0], pl[k][1]
            out = ch.step(fac, gam)
            batched = ch.batched[0] > 0
            assert want_batched is None or batched == want_batched, (ch.batched, want_batched)
            fell = [i for i in ch.l1 if out[i]["d"]["need"] and not out[i]["d"]["spec_ok"]]
            if batched:
                assert ch.batched == (len(ch.l1), len(fell)), (ch.batched, fell)
            for i in ch.l1:          # (a cardinality set launches passes of its own: no launch of such a call is attributed)
                out[i]["alone"] = fell == [i] and not ch.card
            for i in ch.l1:
                want = plans[i][k][2] if k < len(plans[i]) else "any"
                got = route_of(out[i], batched, fac[i] != 1)
                d = out[i]["d"]
                print(f"{name} {np.dtype(TF).name} {'batched' if batched else 'per-set'} call {k + 1} set {i}: intended {want}, took {got}; theta {d['theta']:.9g} "
                      f"need {d['need']:.0f} spec_ok {d['spec_ok']:.0f} overflow {d['overflow']:.0f} gathered {d['gathered']:.0f} "
                      f"michelot {d['michelot_its']:.0f} lean(next) {d['lean']:.0f} sampled {d['sampled']:.0f} hw {d['hw']:.3g} "
                      f"probe launches {out[i]['launches'].get('k_pass<M_PROBE>', 0)}")
                if want != "any":
                    assert want in got.split("+"), f"{name} call {k + 1} set {i}: intended route {want}, the search took {got}: {d}"
                # refine > 0: the refinement pass was launched.  The batched chain launches it for every falling set of a call as
                # soon as one of them asks for it, so the launch is this set's only where no other set fell back (the single-set
                # cases tv-3d, cold-refine; in c3-vec where the other sets hit)
                if want in ("lean-miss", "lean-far") and batched and out[i]["alone"]:
                    assert out[i]["launches"].get("k_pass<M_PROBE>", 0) >= 1
                if got in ("window", "beyond") and batched and out[i]["alone"] and len(out[i]["v"]) < 2 ** 17:
                    assert out[i]["launches"].get("k_pass<M_PROBE>", 0) == 0      # (the bracket cannot hold more than L1_CAP)
                if case.get("all_active"):
                    a = np.abs(out[i]["v"].astype(np.float64))
                    th, C, _ = X.exact_theta(a, ch.b[i])
                    assert d["need"] == 1 and C == len(a) - 1 and th < a.min(), "the case was meant to keep every entry active"
            if batched and not fell and not ch.card:      # no fallback pass
                ln = out[ch.l1[0]]["launches"]
                assert ln.get("k_pass<M_COMPACT>", 0) == 0 and ln.get("k_pass<M_PROBE>", 0) == 0, ln
            for i in ch.card:
                v = np.abs(out[i]["v"])
                print(f"{name} call {k + 1} cardinality set {i}: kept {int((out[i]['y'] != 0).sum())} of {len(v)}")
            if after_call:
                after_call(ch, k, out)
    finally:
        ch.close()


@pytest.mark.parametrize("TF", TFS)
@pytest.mark.parametrize("name", [k for k in CASES if not k.startswith("card")])
def test_iteration_searches_are_exact(sipx, TF, name, monkeypatch):
    run_case(sipx, TF, name, monkeypatch)


# ---- D: cardinality in the same chains -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", TFS)
@pytest.mark.parametrize("name", ["card-dz", "cardf-dy"])
def test_cardinality_in_the_same_chains(sipx, TF, name, monkeypatch):
    """y of the cardinality set is the oracle's projection of the captured v bit for bit (asserted in Chain.step), and on EVERY
    call -- the cold one and the two with a warm tau_prev -- the k-th place falls inside a tie group (integer differences).  The
    l1 set beside it is driven and checked through its plan like every other."""
    case = CASES[name]
    straddles = {}

    def count(ch, call, out):
        i = ch.card[0]
        k, v = ch.cards[i], out[i]["v"]
        if case["sets"][i][0] == "card":
            cols = [np.abs(v)]
        else:                                  # per z-slice of the D_y grid
            n = case["n"]
            cols = [np.abs(c) for c in v.reshape((n[0], n[1] - 1, n[2]), order="F").transpose(2, 0, 1).reshape(n[2], -1)]
        straddles[call] = 0
        for a in cols:
            tau = np.sort(a)[::-1][k - 1]
            if (a > tau).sum() < k < (a >= tau).sum():
                straddles[call] += 1
    run_case(sipx, TF, name, monkeypatch, after_call=count)
    assert len(straddles) == 3 and all(c >= 1 for c in straddles.values()), straddles


# ---- C: the searches of the feasibility estimates --------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", TFS)
@pytest.mark.parametrize("n,runs", [((36, 20, 9), None), ((33, 17, 6), None), ((36, 20, 9), "16")])
def test_feasibility_searches_are_exact(sipx, TF, n, runs, monkeypatch):
    """update_y_l with YL_FEAS on an iteration that is a multiple of ten: theta of the search on s = A x against the exact one,
    the returned feasibility against ||soft(s, theta_e) - s|| / (||s|| + 100 eps) in float64 from the TF elements, to 8 eps(TF):
    one TF rounding per element difference (exact in the float64 sums), float64 sums on the engine's side, one rounding each
    of the two norms and of the quotient (3 * eps / 2), and a margin.  Twice (the second search is warm); the D_z set has a
    radius above ||s||_1 (feasible: 0).  runs: SIPX_L1_SAMPLE_RUNS, so that the sampled estimate in front of these searches
    (run_batched, feas_ps) is taken on a small grid too."""
    if runs:
        monkeypatch.setenv("SIPX_L1_SAMPLE_RUNS", runs)
    case = dict(n=n, sets=[("bounds",), ("l1", "D_x", "heavy", 0.05, []), ("l1", "D_y", "heavy", 0.1, []),
                           ("l1", "D_z", "heavy", 0.5, [])])
    ch = Chain(sipx, case, TF)
    eps = float(np.finfo(TF).eps)
    try:
        seen_inf, seen_feas, sampled = 0, 0, 0
        for call, it in enumerate((10, 20)):
            ch.step(np.ones(ch.p), np.where(np.arange(ch.p) > 0, 1.0 if call == 0 else G, 1.0), flags=sipx.host.YL_FEAS, it=it)
            fe = ch.last["fe"]
            for i in ch.l1:
                s = O.csc_mul(ch.Ao[i], ch.x)
                d = ch.ctx.debug_proj(i, 1)
                fz = X.feasibility(s, ch.b[i])
                if fz > 0:
                    assert d["need"] == 0 and fe[i] == 0.0, (i, d, fe[i])
                    seen_feas += 1
                    continue
                assert fz < 0 and d["need"] == 1
                th, C, S = X.exact_theta(np.abs(s.astype(np.float64)), ch.b[i])
                tol = X.theta_tol(C, S, ch.b[i], th, TF)
                note(TF, abs(d["theta"] - th) / tol)
                assert abs(d["theta"] - th) <= tol, (i, call, d, th, tol)
                ps = X.soft(s, TF(d["theta"])).astype(np.float64)
                s64 = s.astype(np.float64)
                ref = np.sqrt(((ps - s64) ** 2).sum()) / (np.sqrt((s64 ** 2).sum()) + 100 * eps)
                print(f"feasibility set {i} call {call + 1}: engine {fe[i]!r} reference {ref!r}; spec_ok {d['spec_ok']:.0f} "
                      f"sampled {d['sampled']:.0f} lean(next) {d['lean']:.0f} gathered {d['gathered']:.0f}")
                sampled += int(d["sampled"])
                if call == 1 and not runs:     # the warm search: s has not moved, the range around the first theta holds it
                    assert d["spec_ok"] == 1, (i, d)
                assert abs(fe[i] - ref) <= 8 * eps * ref, (i, call, fe[i], ref)
                seen_inf += 1
        assert seen_inf >= 4 and seen_feas >= 2
        assert (sampled > 0) == bool(runs), sampled
    finally:
        ch.close()
