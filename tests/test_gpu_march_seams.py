"""The x-step's z-marching kernels (k_cds_march, k_rhs_march; csrc/kernels_cds.hip, csrc/kernels_sets.hip) at their tile, wave and
chunk seams, against the numpy oracle.

1. CPU: the launch geometry restated in tests/march_geometry.py; every shape of its table has the seams it is listed for, per
   kernel and precision, and every property is hit by both kernels in both precisions.
2. CPU: the point-wise bound of part 3 rejects a product with ONE wrong seam point, which test_phases_lockstep's norm
   tolerance accepts in Float32.
3. GPU: one x-step from a state far from the solution (the oracle's CG takes at least 6 iterations) on four routes -- flat
   unfused, march unfused on the bands, march fused on the bands, march fused on the class table -- each in a context of its
   own and proved by the engine's route counters: apply_Q before and after a Q update and the right-hand side bit for bit,
   the CG count, and x POINT-WISE against the oracle; the routes against each other bit for bit.  The flat 5-band pair
   k_cds / k_cds_fused on 2-D seam shapes the same way.
4. GPU: k_rhs_march against oracle.rhs_compose and against k_rhs bit for bit, every block layout at the shape with two tiles
   along x; lists the march refuses fall back to k_rhs.

A grid here has at most 20000 points; SIPX_CDS_MARCH_ZCHUNK / SIPX_RHS_MARCH_ZCHUNK put chunk edges inside it."""
import functools

import numpy as np
import pytest

from oracle import parsdmm_oracle as O      # checker only
from tests import l1_exact as X
from tests import march_geometry as MG
from tests.test_gpu_parity import _problem, model
from tests.test_gpu_sweep_geometry import LISTS_3D, _case_id, _first_difference

TFS = [np.float32, np.float64]
C3, TV = ["bounds", "l1:D_x", "l1:D_y", "l1:D_z"], ["bounds", "l1:TV"]       # band order 1 / band order 2 of the march
TOL_REF = {np.float32: 1e-5, np.float64: 1e-10}


def _combo_id(c):
    return f"{c[0]}-{c[1]}"


# =================================================================================================================
# 1. the geometry table proves itself (no GPU)
# =================================================================================================================
@pytest.mark.parametrize("combo", MG.ALL4, ids=_combo_id)
@pytest.mark.parametrize("e", MG.TABLE, ids=lambda e: "x".join(map(str, e["n"])))
def test_march_table_shapes_have_the_seams_they_are_listed_for(e, combo):
    kernel, prec = combo
    NT = MG.KERNELS[kernel][0]
    g = MG.geometry(kernel, e["n"], np.dtype(prec).type, e["zchunk"])
    assert int(np.prod(e["n"])) <= 20000
    assert g["LX"] * g["TY"] == NT and g["LX"] <= 64 and g["lg"] == min(int(np.ceil(np.log2(g["nvx"]))), 6)
    assert sum(g["tile_lanes"]) == g["nvx"] and len(g["tile_lanes"]) == g["tiles_x"]
    assert sum(g["tile_rows"]) == e["n"][1] and len(g["tile_rows"]) == g["tiles_y"]
    assert sum(g["chunks"]) == e["n"][2] and g["zchunk"] == e["zchunk"] and g["items"] == g["tiles_x"] * g["tiles_y"] * len(g["chunks"])
    for name in e["props"][combo]:
        assert MG.PROPERTIES[name](g), f"{e['n']} {combo}: not '{name}' any more: {g}"
    for k, v in e["facts"][combo].items():
        assert g[k] == v, f"{e['n']} {combo}: {k} is {g[k]}, listed as {v}"


def test_every_march_property_is_hit_by_both_kernels_in_both_precisions():
    for combo in MG.ALL4:
        hit = {name for e in MG.TABLE for name in e["props"][combo]}
        assert hit == set(MG.PROPERTIES), (combo, set(MG.PROPERTIES) - hit)
    # the shape the fallback and layout cases of part 4 and the teeth test run on
    assert all("two tiles along x, the last one ragged" in MG.entry(MG.SEAM_X)["props"][c] for c in MG.ALL4)


# =================================================================================================================
# the state the x-step starts from, and the oracle's side of it (computed once per case, never written to)
# =================================================================================================================
class XState:
    """A set list on a grid with unit spacings in a state FAR from the solution -- x0 = m + 50 randn, y_i = A_i m + 30 randn,
    l_i = randn, unequal rho -- so that CG has work to do; the oracle's right-hand side, Q, x-step (iteration 3, where a far
    state makes the tolerance the reference one) and products before and after a Q update."""

    def __init__(self, n, kinds, TF):
        self.n, self.kinds, self.TF = n, kinds, TF
        self.h = (1.0,) * len(n)
        self.m = m = model(n, TF, seed=3)
        self.go, _, self.Po, self.Ao, self.propo, self.AtAo = _problem(O, n, self.h, TF, kinds, m)
        self.p, self.N = p, N = len(self.Ao), len(m)
        rng = np.random.default_rng(11 + len(kinds))
        self.x0 = (m + 50 * rng.standard_normal(N)).astype(TF)
        self.y0 = [O.csc_mul(self.Ao[i], m) + (30 * rng.standard_normal(self.Ao[i].shape[0])).astype(TF) for i in range(p)]
        self.l0 = [rng.standard_normal(self.Ao[i].shape[0]).astype(TF) for i in range(p)]
        self.rho = np.array([10.0, 3.0, 7.0, 2.0, 5.0, 4.0][:p - 1] + [6.0], TF)          # as tests/test_gpu_sweep_geometry.Replay
        self.rho64 = self.rho.astype(np.float64)
        self.rho2 = [float(r) * (1.5 if i % 2 else 0.75) for i, r in enumerate(self.rho)]
        self.v = rng.standard_normal(N).astype(TF)                                           # what apply_Q is taken on
        self.rhs = O.rhs_compose(self.l0, self.y0, self.rho, self.Ao, p, N)
        for a in (self.x0, self.v, self.rhs, *self.y0, *self.l0):
            a.setflags(write=False)

    @functools.cached_property
    def xstep(self):
        TF = self.TF
        Q, off = O.assemble_Q(self.AtAo, self.propo.AtA_offsets, self.rho, TF)
        want0 = O.Ax_CDS(self.v, Q, off)
        x, it, relres, tol = O.argmin_x(Q, self.rhs, self.x0.copy(), TF(TOL_REF[TF]), 3, off)

        class L: pass
        log = L(); log.rho = np.array([self.rho])
        Q2 = O.Q_update(Q.copy(order="F"), self.AtAo, self.propo, np.array(self.rho2, TF), list(range(self.p)), log, 0, off)
        want1 = O.Ax_CDS(self.v, Q2, off)
        for a in (x, want0, want1, Q):
            a.setflags(write=False)
        return dict(Q=Q, off=off, x=x, it=int(it), relres=float(relres), tol=float(tol), Qv=want0, Qv_updated=want1)

    def context(self, sipx, monkeypatch, env):
        for k in ("SIPX_CDS_MARCH", "SIPX_CDS_MARCH_ZCHUNK", "SIPX_CG_FUSED", "SIPX_Q_TABLE", "SIPX_RHS_MARCH", "SIPX_RHS_MARCH_ZCHUNK"):
            if k in env:
                monkeypatch.setenv(k, env[k])
            else:
                monkeypatch.delenv(k, raising=False)
        gs, os_, Ps, As, props, AtAs = _problem(sipx, self.n, self.h, self.TF, self.kinds, self.m)
        os_.zero_ini_guess = False
        os_.rho_ini = [float(r) for r in self.rho]
        return sipx.host.build_context(self.m, AtAs, As, props, Ps, gs, os_, x=self.x0, l=self.l0, y=self.y0)


@functools.lru_cache(maxsize=None)
def _state(n, kinds, TF):
    return XState(n, list(kinds), TF)


def _routes_3d(zchunk):
    march = {"SIPX_CDS_MARCH": "2", "SIPX_CDS_MARCH_ZCHUNK": str(zchunk)}
    mk = lambda form, modes: [f"k_cds_march<MODE={k}>/{form}" for k in modes]
    # name -> (switches, routes that must have run, substrings no launched route may have)
    return {
        "flat": ({"SIPX_CDS_MARCH": "0", "SIPX_CG_FUSED": "0"}, ["k_cds<MODE=0>", "k_cds<MODE=1>", "k_cds<MODE=2>"], MG.FLAT_ONLY + ["k_cds_fused"]),
        "march": ({**march, "SIPX_Q_TABLE": "0", "SIPX_CG_FUSED": "0"}, mk("bands", (0, 1, 2)), MG.MARCH_ONLY + ["/table", "MODE=3"]),
        "march-fused": ({**march, "SIPX_Q_TABLE": "0", "SIPX_CG_FUSED": "1"}, mk("bands", (0, 1, 2, 3)), MG.MARCH_ONLY + ["/table"]),
        "march-fused-table": ({**march, "SIPX_Q_TABLE": "1", "SIPX_CG_FUSED": "1"}, mk("table", (0, 1, 2, 3)), MG.MARCH_ONLY + ["/bands"]),
    }


ROUTES_2D = {
    "flat": ({"SIPX_CG_FUSED": "0"}, ["k_cds<MODE=0>", "k_cds<MODE=1>", "k_cds<MODE=2>"], MG.FLAT_ONLY + ["k_cds_fused"]),
    "flat-fused": ({"SIPX_CG_FUSED": "1"}, ["k_cds<MODE=0>", "k_cds<MODE=1>", "k_cds<MODE=2>", "k_cds_fused"], MG.FLAT_ONLY),
}


def _x_step(sipx, monkeypatch, S, name, route):
    """One route in a context of its own: assertions 1-4 against the oracle; returns (x, cg_it, relres, max |x - x_oracle|)."""
    env, must, never = route
    TF, R = S.TF, S.xstep
    eps = np.finfo(TF).eps
    tag = f"{_case_id(S.n)} {_case_id(S.kinds)} {np.dtype(TF).name} {name}"
    ctx = S.context(sipx, monkeypatch, env)
    try:
        before = MG.routes(ctx)
        y0 = ctx.apply_Q(S.v)
        ctx.rhs_compose(S.rho64)
        rhs = ctx.get_rhs()
        tol, cg_it, relres, flag = ctx.argmin_x(3, TOL_REF[TF])
        x, _, _ = ctx.download(False)
        ctx.q_update(S.rho2, [float(r) for r in S.rho])
        y1 = ctx.apply_Q(S.v)
        took = MG.ran(MG.routes(ctx), before)
    finally:
        ctx.close()
    MG.assert_route(took, must, never, tag)
    assert X.same_bits(y0, R["Qv"]), f"{tag}, apply_Q: {_first_difference(y0, R['Qv'], S.n)}"
    assert X.same_bits(y1, R["Qv_updated"]), f"{tag}, apply_Q after q_update: {_first_difference(y1, R['Qv_updated'], S.n)}"
    assert X.same_bits(rhs, S.rhs), f"{tag}, right-hand side: {_first_difference(rhs, S.rhs, S.n)}"
    worst, at = MG.max_difference(x, R["x"], S.n)
    bound = MG.pointwise_bound(TF, R["it"], S.N, R["x"], S.x0)
    print(f"{tag}: cg_it {cg_it} / {R['it']}, relres {relres!r} / {R['relres']!r}, tol {tol!r}; max |x - x_oracle| = {worst:.3e} at {at}, bound {bound:.3e}")
    assert cg_it == R["it"] and flag == 0, (tag, cg_it, R["it"], flag)
    assert abs(tol - R["tol"]) <= 8 * eps * abs(R["tol"]), (tag, tol, R["tol"])               # test_phases_lockstep's tolerances
    assert abs(relres - R["relres"]) <= 1e-3 * R["relres"], (tag, relres, R["relres"])
    assert worst <= bound, f"{tag}: max |x - x_oracle| = {worst:.3e} at grid index {at} (engine {x[np.ravel_multi_index(at, S.n, order='F')]!r}), beyond {bound:.3e}"
    return x, cg_it, relres, worst


def _same(tag, a, b, n):
    (xa, ia, ra, _), (xb, ib, rb, _) = a, b
    assert ia == ib and ra == rb, (tag, ia, ib, ra, rb)
    assert X.same_bits(xa, xb), f"{tag}: {_first_difference(xa, xb, n)}"


# =================================================================================================================
# 2. the point-wise check has teeth (no GPU)
# =================================================================================================================
@pytest.mark.parametrize("TF", TFS, ids=lambda t: np.dtype(t).name)
def test_pointwise_bound_rejects_one_wrong_seam_point(TF):
    """oracle.cg with a product whose row at the first point of the second x-tile (grid row 3 of plane 4) takes its left
    neighbour from one element further left: CG still converges, in the clean run's iterations.  The point-wise bound of
    the x-step test rejects the result by more than 100 x in both precisions; test_phases_lockstep's norm bound (50 eps)
    ACCEPTS it in Float32 -- why the check is point-wise.  (Measured, (264,10,7) C3: Float32 8 iterations either way, max |dx| 2.15 at the
    faulty row = 2560 x the bound, relative 2-norm 5.78e-6 < 5.96e-6; Float64 max |dx| 3.04 = 4.7e7 x the bound.)"""
    S = _state(MG.SEAM_X, tuple(C3), TF)
    R = S.xstep
    row = MG.second_tile_row(S.n, TF, 3, 4)
    bad = MG.faulty_product(O.Ax_CDS, R["Q"], R["off"], row)
    tol = TF(R["tol"])
    x, flag, relres, it = O.cg(bad, S.rhs, tol, 1000, S.x0.copy())
    worst, at = MG.max_difference(x, R["x"], S.n)
    bound = MG.pointwise_bound(TF, R["it"], S.N, R["x"], S.x0)
    rel2 = np.linalg.norm(x.astype(np.float64) - R["x"]) / np.linalg.norm(R["x"].astype(np.float64))
    print(f"{np.dtype(TF).name}: faulty row {row} = {tuple(int(c) for c in np.unravel_index(row, S.n, order='F'))}: cg_it {it} / {R['it']}, flag {flag}, "
          f"relres {relres!r} / {R['relres']!r}; max |dx| {worst:.3e} at {at} = {worst / bound:.3g} x the bound; relative 2-norm {rel2:.3e}")
    assert R["it"] >= 6 and flag == 0
    assert at == tuple(int(c) for c in np.unravel_index(row, S.n, order="F"))
    assert worst >= 100 * bound, (worst, bound)
    if TF == np.float32:
        assert it == R["it"]
        assert rel2 <= 50 * np.finfo(TF).eps, rel2          # the norm test would have let it through


# =================================================================================================================
# 3. the x-step against the oracle, route by route
# =================================================================================================================
XSTEP_3D = [(e["n"], k) for e in MG.TABLE for k in (C3, TV)]
XSTEP_2D = [(n, k) for n in ((1304, 11), (264, 9)) for k in (TV, ["bounds", "l1:D_x", "l1:D_z"])]


@pytest.mark.gpu
@pytest.mark.parametrize("TF", TFS, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("n,kinds", XSTEP_3D, ids=_case_id)
def test_x_step_equals_the_oracle_at_the_march_seams(sipx, monkeypatch, n, kinds, TF):
    """apply_Q (before and after q_update) and rhs_compose bit for bit, cg_it, flag, tol and relres as test_phases_lockstep,
    and max |x - x_oracle| <= 4 cg_it c eps max |x_oracle - x0| (march_geometry.pointwise_bound) on the flat, the marched, the
    fused marched and the class-table route, each proved by the route counters.  Fused against unfused and table against
    bands: x, cg_it, relres bit for bit; march against flat: bit for bit in Float32, the bound in Float64.
    Measured max |x - x_oracle| (printed per case and route): Float32 exactly 0 on every route of every case, here and in two
    dimensions; Float64 at most 9.095e-13 (two ulps of a value near 4000; bounds 5e-9 ... 6.5e-8), on every route alike."""
    S = _state(n, tuple(kinds), TF)
    assert S.xstep["it"] >= 6, f"precondition: the oracle's CG takes {S.xstep['it']} iterations from this state"
    out = {name: _x_step(sipx, monkeypatch, S, name, r) for name, r in _routes_3d(MG.entry(n)["zchunk"]).items()}
    _same("fused against unfused march", out["march-fused"], out["march"], n)
    _same("table against bands", out["march-fused-table"], out["march-fused"], n)
    if TF == np.float32:
        _same("march against flat", out["march"], out["flat"], n)
    else:
        d, at = MG.max_difference(out["march"][0], out["flat"][0], n)
        assert out["march"][1] == out["flat"][1]
        assert d <= MG.pointwise_bound(TF, S.xstep["it"], S.N, S.xstep["x"], S.x0), ("march against flat", d, at)


@pytest.mark.gpu
@pytest.mark.parametrize("TF", TFS, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("n,kinds", XSTEP_2D, ids=_case_id)
def test_x_step_equals_the_oracle_on_the_flat_pair_in_two_dimensions(sipx, monkeypatch, n, kinds, TF):
    """The same state and checks on the 5-band k_cds / k_cds_fused pair at 2-D seam shapes: each against the oracle, fused
    against unfused bit for bit."""
    S = _state(n, tuple(kinds), TF)
    assert S.xstep["it"] >= 6, f"precondition: the oracle's CG takes {S.xstep['it']} iterations from this state"
    out = {name: _x_step(sipx, monkeypatch, S, name, r) for name, r in ROUTES_2D.items()}
    _same("fused against unfused", out["flat-fused"], out["flat"], n)


# =================================================================================================================
# 4. k_rhs_march against the oracle and against k_rhs
# =================================================================================================================
RHS_CASES = [(MG.SEAM_X, k) for k in LISTS_3D] + [(e["n"], k) for e in MG.TABLE if e["n"] != MG.SEAM_X for k in (C3, TV)]


def _rhs(sipx, monkeypatch, S, env, route):
    ctx = S.context(sipx, monkeypatch, env)
    try:
        before = MG.routes(ctx)
        ctx.rhs_compose(S.rho64)
        rhs = ctx.get_rhs()
        took = MG.ran(MG.routes(ctx), before)
    finally:
        ctx.close()
    assert took == {route: 1}, f"{_case_id(S.n)} {_case_id(S.kinds)} {env}: the forced route was not taken: expected one launch of {route}, launched {took}"
    return rhs


@pytest.mark.gpu
@pytest.mark.parametrize("TF", TFS, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("n,kinds", RHS_CASES, ids=_case_id)
def test_marched_rhs_equals_the_oracle_at_the_seams(sipx, monkeypatch, n, kinds, TF):
    """get_rhs() through k_rhs_march (forced, in the table's chunks; proved by the route counter) bit for bit against
    oracle.rhs_compose and against k_rhs (SIPX_RHS_MARCH=0), from y and l of the far state with unequal rho."""
    S = _state(n, tuple(kinds), TF)
    marched = _rhs(sipx, monkeypatch, S, {"SIPX_RHS_MARCH": "2", "SIPX_RHS_MARCH_ZCHUNK": str(MG.entry(n)["zchunk"])}, "k_rhs_march")
    flat = _rhs(sipx, monkeypatch, S, {"SIPX_RHS_MARCH": "0"}, "k_rhs")
    assert X.same_bits(marched, S.rhs), f"k_rhs_march against the oracle: {_first_difference(marched, S.rhs, n)}"
    assert X.same_bits(flat, S.rhs), f"k_rhs against the oracle: {_first_difference(flat, S.rhs, n)}"
    assert X.same_bits(marched, flat)


# more than RM_MAXB = 8 blocks (1 + 3 + 3 + 1 + 1 + the distance term = 10); more than RM_MAXY = 3 y-difference blocks within
# 8 blocks (1 + four times D_y + the distance term = 6)
FALLBACKS = [(["bounds", "l1:TV", "l1:TV", "l1:D_x", "l1:D_z"], "blocks"), (["bounds", "l1:D_y", "l1:D_y", "l1:D_y", "l1:D_y"], "y-blocks")]


@pytest.mark.gpu
@pytest.mark.parametrize("TF", TFS, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("kinds,why", FALLBACKS, ids=lambda v: v if isinstance(v, str) else None)
def test_rhs_lists_the_march_refuses_fall_back_to_k_rhs(sipx, monkeypatch, kinds, why, TF):
    """With the march forced, a list with more blocks than k_rhs_march takes (RM_MAXB), or more y-difference blocks than it has
    LDS slots for (RM_MAXY), runs k_rhs -- the counter shows it -- and gives the oracle's bits."""
    S = _state(MG.SEAM_X, tuple(kinds), TF)
    blocks = [3 if k == "l1:TV" else 1 for k in kinds] + [1]
    ny = sum(k in ("l1:D_y", "l1:TV") for k in kinds)
    assert (sum(blocks) > MG.RM_MAXB) if why == "blocks" else (sum(blocks) <= MG.RM_MAXB and ny > MG.RM_MAXY)
    rhs = _rhs(sipx, monkeypatch, S, {"SIPX_RHS_MARCH": "2", "SIPX_RHS_MARCH_ZCHUNK": str(MG.entry(MG.SEAM_X)["zchunk"])}, "k_rhs")
    assert X.same_bits(rhs, S.rhs), f"k_rhs against the oracle: {_first_difference(rhs, S.rhs, S.n)}"
