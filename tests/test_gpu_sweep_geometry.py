"""The one-sweep y/l update (k_yl_multi, csrc/kernels_multi.hip) at its tile, segment and chunk seams.

1. CPU: the launch geometry restated in tests/sweep_geometry.py; every shape of its table has the seams it is listed for, in
   both precisions.
2. GPU: single ctx.update_y_l calls -- plain, first iteration + feasibility estimates, Barzilai-Borwein sums -- replayed in the
   numpy oracle from the state the engine had, through the sweep and through the per-set kernels (SIPX_YL_MULTI=0): y and l of
   every set bit for bit, the sums at the tolerances of test_phases_lockstep, the right-hand side of the new iterate bit for
   bit.  Every instantiated block layout at one seam shape of its dimension, the two headline lists at every shape.
3. GPU: 27 whole iterations, sweep against per-set kernels (the assertions of test_one_sweep_update_is_bit_identical), at the
   seam shapes; with rho and gamma fixed every iteration writes the next right-hand side from inside the sweep.

A grid here has at most 18480 points; SIPX_MULTI_ZCHUNK puts chunk edges inside it."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O      # checker only
from tests import l1_exact as X
from tests import sweep_geometry as SG
from tests import test_gpu_round3 as R3
from tests.test_gpu_parity import _problem, model

TFS = [np.float32, np.float64]


# =================================================================================================================
# 1. the geometry table proves itself (no GPU)
# =================================================================================================================
@pytest.mark.parametrize("TF", TFS)
@pytest.mark.parametrize("e", SG.TABLE, ids=lambda e: "x".join(map(str, e["n"])))
def test_table_shapes_have_the_seams_they_are_listed_for(e, TF):
    g = SG.geometry(e["n"], TF, e["zchunk"])
    assert int(np.prod(e["n"])) <= 20000
    assert g["LX"] * g["TY"] == SG.MULTI_NT and g["LX"] <= 64 and g["lg"] == min(int(np.ceil(np.log2(g["nvx"]))), 6)
    assert g["xsplit"] == (len(e["n"]) == 2)
    assert sum(g["tile_lanes"]) == g["nvx"] and len(g["tile_lanes"]) == g["tiles_x"]
    assert sum(g["chunks"]) == e["n"][-1] and len(g["tile_rows"]) == g["tiles_y"]
    for name in e["props"]:
        assert SG.PROPERTIES[name](g), f"{e['n']} {np.dtype(TF).name}: not '{name}' any more: {g}"
    for k, v in e["facts"][np.dtype(TF).name].items():
        assert g[k] == v, f"{e['n']} {np.dtype(TF).name}: {k} is {g[k]}, listed as {v}"


def test_every_listed_property_is_hit_in_two_and_three_dimensions():
    """Each seam property is covered by some shape of the table in each precision; the ones that exist in both dimensions, in both."""
    for TF in TFS:
        hit = {}
        for e in SG.TABLE:
            g = SG.geometry(e["n"], TF, e["zchunk"])
            for name in e["props"]:
                hit.setdefault(name, set()).add(len(e["n"]))
        assert set(hit) == set(SG.PROPERTIES), set(SG.PROPERTIES) - set(hit)
        for name in ("two tiles along x", "last tile ragged", "LX <= 2", "three chunks, last one short"):
            assert hit[name] == {2, 3}, (name, hit[name])


# =================================================================================================================
# 2. one update_y_l call against the oracle, on both routes
# =================================================================================================================
# every layout of SIPX_LAYOUTS (kernels_multi.hip), as a set list
LISTS_3D = [
    ["bounds", "l1:D_x", "l1:D_y", "l1:D_z"],                   # C3: I X Y Z D
    ["bounds", "l1:TV"],                                        # C5: I [Z Y X] D
    ["bounds", "l1:D_x", "l1:D_z"],                             # I X Z D
    ["bounds", "l1:D_z"],                                       # I Z D
    ["bounds", "l1:D_y"],                                       # I Y D
    ["bounds", "l1:D_x"],                                       # I X D
    ["bounds", "l1:TV", "annulus"],                             # I [Z Y X] I D
    ["bounds", "l1:TV", "l2"],                                  # the same layout, the l2 ball in it
    ["bounds"],                                                 # I D
    ["bounds", "l1:D_x", "l1:D_y", "l1:D_z", "annulus"],        # I X Y Z I D
]
LISTS_2D = [
    ["bounds", "l1:TV"],                                        # C2: I [Z X] D
    ["bounds", "l1:D_z", "l1:D_x"],                             # I Z X D
    ["bounds", "l1:D_x", "l1:D_z"],                             # I X Z D
    ["bounds", "l1:D_x"],                                       # I X D
    ["bounds", "l1:D_z"],                                       # I Z D
    ["bounds"],                                                 # I D
]
C3, C2 = LISTS_3D[0], LISTS_2D[0]
SEAM_3D, SEAM_2D = (264, 10, 7), (1304, 11)
ORACLE_CASES = ([(SEAM_3D, k) for k in LISTS_3D] + [(SEAM_2D, k) for k in LISTS_2D] +
                [(e["n"], C3) for e in SG.TABLE if len(e["n"]) == 3 and e["n"] != SEAM_3D] +
                [(e["n"], C2) for e in SG.TABLE if len(e["n"]) == 2 and e["n"] != SEAM_2D])


def _case_id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    if isinstance(v, list):
        return "+".join(k.replace("l1:", "") for k in v)
    return None


def _set_chunk(monkeypatch, n):
    zc = SG.entry(n)["zchunk"]
    if zc:
        monkeypatch.setenv("SIPX_MULTI_ZCHUNK", str(zc))
    else:
        monkeypatch.delenv("SIPX_MULTI_ZCHUNK", raising=False)


class _Log:
    def __init__(self, it, p):
        self.r_pri, self.r_dual, self.set_feasibility = np.zeros((it, p)), np.zeros((it, p)), np.zeros((2, p - 1))


def _first_difference(a, b, shape=None):
    bad = np.nonzero(X._bits(a) != X._bits(b))[0]
    at = f"row {bad[0]}" if shape is None else f"row {bad[0]} = grid index {tuple(int(c) for c in np.unravel_index(bad[0], shape, order='F'))}"
    return f"{len(bad)} of {len(a)} entries differ, first at {at}: engine {a[bad[0]]!r}, oracle {b[bad[0]]!r}"


class Replay:
    """A set list on a grid in a random warm state (x, y, l, unequal rho and gamma), and the oracle's side of one update_y_l
    call from the state an engine context had before it."""

    def __init__(self, n, kinds, TF):
        self.n, self.kinds, self.TF = n, kinds, TF
        self.h = SG.entry(n)["h"]
        self.m = model(n, TF, seed=3)
        self.go, _, self.Po, self.Ao, self.propo, _ = _problem(O, n, self.h, TF, kinds, self.m)
        self.p, self.N = len(self.Ao), len(self.m)
        p, m = self.p, self.m
        rng = np.random.default_rng(7 + len(kinds))
        self.x0 = (m + 50 * rng.standard_normal(self.N)).astype(TF)
        self.y0 = [O.csc_mul(self.Ao[i], self.x0) + (5 * rng.standard_normal(self.Ao[i].shape[0])).astype(TF) * TF(0.01) for i in range(p)]
        self.l0 = [rng.standard_normal(self.Ao[i].shape[0]).astype(TF) for i in range(p)]
        # unequal penalties; relaxation 1 (the branch without x_hat) on the first set, other values on the rest, the distance term included
        self.rho = np.array([10.0, 3.0, 7.0, 2.0, 5.0, 4.0][:p - 1] + [6.0], TF)
        self.gamma = np.array([1.0, 1.3, 1.7, 1.1, 1.5, 1.2][:p - 1] + [1.25], TF)
        self.rho64, self.gam64 = self.rho.astype(np.float64), self.gamma.astype(np.float64)
        self.l1 = [i for i, k in enumerate(kinds) if k.startswith("l1:")]
        self.scaled = [i for i, k in enumerate(kinds) if k in ("annulus", "l2")]
        # the radius of an l1 ball as _problem states it, as the number of the working precision both sides round it to
        self.b = {i: float(TF(0.5 * np.abs(O.get_TD_operator(self.go, kinds[i][3:], TF)[0] @ m).sum())) for i in self.l1}
        nm = float(np.linalg.norm(m.astype(np.float64)))
        self.sigma = {i: (TF(0.9 * nm), TF(0.98 * nm)) if kinds[i] == "annulus" else (TF(0.0), TF(0.9 * nm)) for i in self.scaled}
        self.off_scale = []                    # (tag, set, ulps): calls whose annulus / l2 scale was not the oracle's TF number

    def shape_of(self, i):
        """grid shape of the rows of set i when it is one block (identity or one difference), else None"""
        k = self.kinds[i] if i < self.p - 1 else "bounds"
        op = k[3:] if k.startswith("l1:") else "identity"
        if op == "identity":
            return self.n
        if op == "TV":
            return None
        ax = {"D_x": 0, "D_y": 1, "D_z": len(self.n) - 1}[op]
        return tuple(d - 1 if a == ax else d for a, d in enumerate(self.n))

    def scaled_prox(self, i, ye, seen, tag):
        """l2 ball / annulus: the oracle's projection; where the engine's y is v * c for a TF number c within 3 ulps of the
        oracle's scale sigma / ||v||_2, that y (noted in off_scale).  Both scales divide by a norm rounded to TF from a float64
        sum of squares taken in another order: the rounded norms differ by at most one ulp, the quotient by at most two more."""
        TF = self.TF
        lo, hi = self.sigma[i]

        def f(v):
            seen[i] = v.copy()
            ref = self.Po[i](v.copy())
            if X.same_bits(ref, ye[i]) or X.same_bits(ref, v):
                return ref
            nl2 = O.nrm2(v, TF)
            c0 = TF((hi if nl2 > hi else lo) / nl2)
            for ulps in (1, 2, 3):
                for way in (TF(np.inf), TF(-np.inf)):
                    c = c0
                    for _ in range(ulps):
                        c = np.nextafter(c, way)
                    cand = (v * c).astype(TF)
                    if X.same_bits(cand, ye[i]):
                        self.off_scale.append((tag, i, ulps if way > 0 else -ulps))
                        return cand
            return ref
        return f

    def call(self, sipx, ctx, x, x_old, y_in, l_in, it, flags, sweep, tag):
        """ctx.update_y_l(it, flags) with x on the device, replayed from (y_in, l_in); every assertion of part 2 but the BB rule."""
        TF, p = self.TF, self.p
        eps = np.finfo(TF).eps
        ctx.kernel_stats_all(2)
        rp, rd, fe = ctx.update_y_l(it, flags, self.rho64, self.gam64)
        names = {k["name"] for k in ctx.kernel_stats_all(0)["kernels"]}
        assert ("k_yl_multi" in names) == sweep, (tag, sorted(names))
        _, le, ye = ctx.download()
        obj, evol = ctx.log_scalars()
        dg = {i: ctx.debug_proj(i, 0) for i in self.l1}
        seen = {}

        def l1_prox(i):                         # as Chain.step: the oracle thresholds with the ENGINE's theta, held to the exact one below
            def f(v):
                seen[i] = v.copy()
                return X.soft(v, TF(dg[i]["theta"])) if dg[i]["need"] else v
            return f
        prox = [l1_prox(i) if i in self.l1 else self.scaled_prox(i, ye, seen, tag) if i in self.scaled else self.Po[i] for i in range(p - 1)]
        prox.append(lambda v: O.prox_l2s(v, self.rho[p - 1], self.m))
        z = lambda: [np.zeros(self.Ao[i].shape[0], TF) for i in range(p)]
        y, l = [v.copy() for v in y_in], [v.copy() for v in l_in]
        y_old, l_old, x_hat, r_pri, s = z(), z(), z(), z(), z()
        log = _Log(it, p)
        O.update_y_l(x.copy(), p, it, y, y_old, l, l_old, self.rho, self.gamma, prox, self.Ao, log, self.Po, 2, x_hat, r_pri, s)
        for i in self.l1:
            try:
                X.check_l1_output(seen[i], ye[i], self.b[i], dg[i]["theta"])
            except AssertionError as e:
                raise AssertionError(f"{tag}, l1 set {i}: {e}; diagnostics {dg[i]}") from None
            fz = X.feasibility(seen[i], self.b[i])
            assert fz == 0 or dg[i]["need"] == (1 if fz < 0 else 0), (tag, i, fz, dg[i])
        for i in self.scaled:
            # test_projectors' bound for these two projectors, whatever scale was taken
            assert np.allclose(ye[i], self.Po[i](seen[i].copy()), rtol=4 * eps, atol=0), (tag, i)
        for i in range(p):
            assert X.same_bits(ye[i], y[i]), f"{tag}, y of set {i}: {_first_difference(ye[i], y[i], self.shape_of(i))}"
            assert X.same_bits(le[i], l[i]), f"{tag}, l of set {i}: {_first_difference(le[i], l[i], self.shape_of(i))}"
        rt = 2e-5 if TF == np.float32 else 1e-11
        print(f"{tag}: r_pri {rp} / {log.r_pri[it - 1]}; r_dual {rd} / {log.r_dual[it - 1]}; obj {obj!r} evol_x {evol!r}")
        assert np.allclose(rp, log.r_pri[it - 1], rtol=rt), (tag, rp, log.r_pri[it - 1])
        assert np.allclose(rd, log.r_dual[it - 1], rtol=10 * rt, atol=1e-30), (tag, rd, log.r_dual[it - 1])
        # r_dual is the one returned number a recomputed seam value reaches (y and l are point-wise), and one wrong point of
        # 18480 moves it by less than the bound above in Float32.  With y and y_old the oracle's bits, A'(y - y_old) is the
        # oracle's bit for bit (the products and their order are those of the right-hand side below); what is left is a float64
        # sum of squares in another order (N 2^-53), its square root rounded to TF and one TF product with rho on either side:
        # two roundings apart at the most, 2 eps; 4 eps asked.
        assert np.allclose(rd, log.r_dual[it - 1], rtol=4 * eps, atol=1e-30), (tag, "r_dual beyond 4 eps", rd, log.r_dual[it - 1])
        if flags & sipx.host.YL_FEAS:
            assert it % 10 == 0
            print(f"{tag}: feasibility {fe} / {log.set_feasibility[1]}")
            assert np.allclose(fe, log.set_feasibility[1], rtol=10 * rt, atol=1e-12), (tag, fe, log.set_feasibility[1])
        nd = O.nrm2(x - self.m, TF)
        assert np.isclose(obj, float(TF(0.5) * TF(nd * nd)), rtol=4 * eps), (tag, obj)
        assert np.isclose(evol, float(O.nrm2(x_old - x, TF) / O.nrm2(x, TF)), rtol=1e-4), (tag, evol)
        # the right-hand side of the new iterate (src/rhs_compose.jl:24-36): short sums of products added in set order
        ctx.rhs_compose(self.rho64)
        rhs, want = ctx.get_rhs(), O.rhs_compose(le, ye, self.rho, self.Ao, p, self.N)
        assert X.same_bits(rhs, want), f"{tag}, right-hand side: {_first_difference(rhs, want, self.n)}"
        return dict(ye=ye, le=le, y=y, l=l, y_old=y_old, l_old=l_old, s=s)

    def run(self, sipx, monkeypatch, sweep):
        """The four calls of a route in one context: plain from the warm state; first iteration + feasibility estimates on
        iteration 10; an x-step, then Barzilai-Borwein sums and the rule; another x-step, then plain again (x_old != x)."""
        TF, p, H = self.TF, self.p, sipx.host
        route = "sweep" if sweep else "per-set"
        monkeypatch.setenv("SIPX_YL_MULTI", "1" if sweep else "0")
        _set_chunk(monkeypatch, self.n)
        gs, os_, Ps, As, props, AtAs = _problem(sipx, self.n, self.h, TF, self.kinds, self.m)
        os_.zero_ini_guess = False
        os_.rho_ini = [float(r) for r in self.rho]
        ctx = sipx.host.build_context(self.m, AtAs, As, props, Ps, gs, os_, x=self.x0, l=self.l0, y=self.y0)
        try:
            x = self.x0
            r0 = self.call(sipx, ctx, x, x, self.y0, self.l0, 1, 0, sweep, f"{route}, plain")
            r1 = self.call(sipx, ctx, x, x, r0["ye"], r0["le"], 10, H.YL_FIRST | H.YL_FEAS, sweep, f"{route}, first + feasibility")
            # the snapshots of the first iteration (PARSDMM.jl:164-180)
            l_hat_0 = [r1["l_old"][i] + TF(self.rho[i]) * (-r1["s"][i] + r1["y_old"][i]) for i in range(p)]
            y_0, l_0, s_0 = r1["ye"], r1["le"], r1["s"]
            tol, _, _, _ = ctx.argmin_x(2, 1.0)              # (the right-hand side is the one composed at the end of the call above)
            x2, _, _ = ctx.download(False)
            assert np.isfinite(x2).all() and not np.array_equal(x2, x)
            r2 = self.call(sipx, ctx, x2, x, r1["ye"], r1["le"], 2, H.YL_BB, sweep, f"{route}, BB")
            rho_o, gam_o = self.rho.copy(), self.gamma.copy()
            l_hat = [np.zeros_like(v) for v in l_0]
            O.adapt_rho_gamma(gam_o, rho_o, True, True, r2["y"], r2["y_old"], r2["s"], s_0, r2["l"], l_hat_0, l_0, r2["l_old"], y_0, p, l_hat)
            rho_s, gam_s = ctx.adapt_rho_gamma(True, True, self.rho64, self.gam64)
            # the rule divides sums that agree to the order of summation (float64 accumulation on both sides)
            rt_bb = 5e-5 if TF == np.float32 else 1e-10
            print(f"{route}, BB rule: rho {rho_s} / {rho_o}; gamma {gam_s} / {gam_o}")
            assert np.allclose(rho_s, rho_o, rtol=rt_bb) and np.allclose(gam_s, gam_o, rtol=rt_bb), (route, rho_s, rho_o, gam_s, gam_o)
            ctx.argmin_x(3, tol)
            x3, _, _ = ctx.download(False)
            self.call(sipx, ctx, x3, x2, r2["ye"], r2["le"], 3, 0, sweep, f"{route}, plain after an x-step")
        finally:
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("TF", TFS, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("n,kinds", ORACLE_CASES, ids=_case_id)
def test_update_y_l_equals_the_oracle_at_the_seams(sipx, monkeypatch, n, kinds, TF):
    """Every set's y and l bit for bit against oracle.update_y_l at working precision (bounds, l1, annulus, l2, distance
    term), through k_yl_multi and through the per-set kernels.  l1 sets as Chain.step compares them: the oracle thresholds
    with the engine's theta, which l1_exact.check_l1_output holds to the exact threshold.  Annulus and l2: y is v times ONE
    number of the working precision, the oracle's scale or -- the norm comes from a float64 sum taken in another order -- a
    neighbour within 3 ulps (printed), and within test_projectors' 4 eps of the oracle's projection; l then bit for bit.
    r_pri, r_dual, feasibility estimates, obj, evol_x and the Barzilai-Borwein rule at test_phases_lockstep's tolerances."""
    S = Replay(n, kinds, TF)
    for sweep in (True, False):
        S.run(sipx, monkeypatch, sweep)
    for tag, i, ulps in S.off_scale:
        print(f"{_case_id(n)} {_case_id(kinds)} {np.dtype(TF).name}: {tag}, set {i}: scale {ulps:+d} ulp from the oracle's")


# =================================================================================================================
# 3. whole iterations at the seams, fused right-hand side included
# =================================================================================================================
FIXED = {"adjust_rho": False, "adjust_gamma": False}        # rho cannot change: every iteration writes the next right-hand side
STEP_CASES = [((264, 10, 7), C3, {}), ((4, 260, 5), C3, {}), ((1304, 11), C2, {}), ((264, 9), C2, {}),
              ((264, 10, 7), C3, FIXED), ((1304, 11), C2, FIXED)]


@pytest.mark.gpu
@pytest.mark.parametrize("TF", TFS, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("n,kinds,okw", STEP_CASES, ids=lambda v: "fixed-rho" if v == FIXED else ("adaptive" if v == {} else _case_id(v)))
def test_whole_iterations_at_the_seams(sipx, monkeypatch, n, kinds, okw, TF):
    """test_one_sweep_update_is_bit_identical (27 iterations, sweep against per-set kernels: x, every y_i and l_i and the
    rho / gamma histories bit for bit in Float32, its Float64 tolerances) on the table's shapes -- among them the first
    Float64 grids with more than one tile along x."""
    _set_chunk(monkeypatch, n)
    R3.test_one_sweep_update_is_bit_identical(sipx, monkeypatch, n, SG.entry(n)["h"], kinds, TF, okw, True)
