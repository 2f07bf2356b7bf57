"""Every whole-vector cardinality search of the engine against the exact stable selection (tests/card_exact.py), bit for bit.

A: the stand-alone projector (SRC 0, a fresh search per call: always cold).  B: the search of the iteration, call by call
through the chains of tests/test_gpu_l1_exact.py, with the bracket and the gathered count of every search read from the
engine's diagnostics and held against predict_route.  C: the search of the feasibility estimate.  D: the slab-decomposed
search on ragged slabs, and its exchange-segment overflow as an error on every rank.  tests/test_card_exact_cpu.py asserts
that every constructed input below takes the route it was constructed for."""
import os

import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import card_exact as C
from tests import l1_exact as X
from tests.test_gpu_l1_exact import CASES, Chain, run_case

pytestmark = pytest.mark.gpu

TFS = [np.float32, np.float64]


# =================================================================================================================
# A. the stand-alone projector
# =================================================================================================================
def project(sipx, v, k):
    g = sipx.compgrid((1.0, 1.0), (10, 10))
    P = sipx.Projector(sipx.set_definitions("cardinality", "identity", 0, int(k), ("matrix", "")), g, v.dtype.type)
    return P(v.copy())


def hold(sipx, tag, v, k):
    y = project(sipx, v, k)
    try:
        C.check_card_output(v, y, k)
    except AssertionError as e:
        raise AssertionError(f"{tag}, k = {k}: {e}") from None
    assert np.array_equal(y, O.project_cardinality(v.copy(), k)), (tag, k)


@pytest.mark.parametrize("TF", TFS)
def test_projector_at_every_length_and_k(sipx, TF):
    """Lengths around the wave, the block, a workgroup's round of four blocks and CARD_CAP; k at both exits ("nothing
    survives", "every non-zero survives": nnz, nnz + 1, n - 1, n, n + 5) and one short of them; exact zeros of both signs."""
    for n in C.LENGTHS:
        v = C.length_vector(n, TF)
        for k in C.ks_for(v):
            hold(sipx, f"length {n}", v, k)


NAMES = [e[0] for e in C.named_vectors(np.float32)]


@pytest.mark.parametrize("TF", TFS)
@pytest.mark.parametrize("name", NAMES)
def test_projector_on_the_named_vectors(sipx, TF, name):
    """The routes of tests/card_exact.py, named_vectors: refined below the cap, passes run out above it (an outlier, tie groups
    above the cap under the index bisection), probes collapsed onto a bracket one ulp wide, the bottom of the number range."""
    _, v, ks, cls = [e for e in C.named_vectors(TF) if e[0] == name][0]
    for k in ks:
        r = C.predict_route(v, k, TF)
        print(f"{name} {np.dtype(TF).name} k = {k} ({cls}): predicted {r['passes']} passes, {r['gathered']} gathered, ran out {r['ran_out']}")
        hold(sipx, name, v, k)


# =================================================================================================================
# B. the search inside the iteration
# =================================================================================================================
TIES = ("card-dz-big-vec", "card-dz-big-odd", "card-tv-3d", "card-tv-2d")


def kth(v, k):
    return float(np.sort(np.abs(v))[::-1][k - 1])


def hold_search(tag, TF, v, k, d, tau_prev):
    """The diagnostics of one search against the exact tau and predict_route (tau_prev None: a cold search).  The bracket holds
    tau and the compaction gathered exactly what lies in it; bracket, count and "the passes ran out" are the predicted ones --
    on a warm search too, which is more than "on the predicted side of the cap".  Returns the prediction."""
    r = C.predict_route(v, k, TF, probes=None if tau_prev is None else C.warm_probes(tau_prev, TF))
    assert r["exit"] == "search" and d["need"] == 1, (tag, r, d)
    tau = kth(v, k)
    got = dict(lo=d["lo"], hi=d["hi"], gathered=int(d["gathered"]), ran_out=bool(d["refine"]))
    print(f"{tag}: tau {tau!r}; predicted {r}; engine {got}")
    assert d["vmax"] == float(np.abs(v).max()), (tag, d)
    assert d["lo"] < tau <= d["hi"], (tag, tau, d)
    a = np.abs(v).astype(np.float64)
    assert int(d["gathered"]) == int(((a > d["lo"]) & (a <= d["hi"])).sum()), (tag, d)
    assert int(d["gathered"]) == r["gathered"] and bool(d["refine"]) == r["ran_out"], (tag, r, d)
    assert (d["lo"], d["hi"]) == (r["lo"], r["hi"]), (tag, r, d)
    return r


@pytest.mark.parametrize("TF", TFS)
@pytest.mark.parametrize("name", [k for k in CASES if k.startswith("card-") and k != "card-dz"])
def test_cardinality_searches_of_the_iteration(sipx, TF, name, monkeypatch):
    """Three calls (cold, warm, warm).  y and l are the oracle's bit for bit and y passes check_card_output on the captured v
    (Chain.step); the engine's bracket holds the exact tau; the cold search (l0 = 0: v = A x) and the warm ones end in the bracket
    predict_route says and gather exactly what it holds; in the tie cases the k-th place straddles a tie group on every call."""
    state = dict(tau_prev=None, routes=[])

    def after(ch, call, out):
        i = ch.card[0]
        v, k = out[i]["v"], ch.cards[i]
        tag = f"{name} {np.dtype(TF).name} call {call + 1}"
        if call == 0:
            assert np.array_equal(v, O.csc_mul(ch.Ao[i], ch.x)), tag
        r = hold_search(tag, TF, v, k, out[i]["d"], state["tau_prev"])
        st, tau, group = C.straddles(v, k)
        if name in TIES:
            assert st, (tag, tau, group)
        state["routes"].append((r, st, group, float(tau), state["tau_prev"]))
        state["tau_prev"] = float(tau)
    run_case(sipx, TF, name, monkeypatch, after_call=after)
    rt = state["routes"]
    assert len(rt) == 3
    if name.startswith("card-dz-big"):           # the tie group of the ones is above the cap: passes run out, all of it gathered
        assert rt[0][2] > C.CAP and rt[0][0]["ran_out"] and rt[0][0]["gathered"] == rt[0][2]
    if name == "card-tv-3d":
        assert rt[0][0]["passes"] == 1 and rt[0][3] == 3.0 and rt[0][2] > 2000
    if name == "card-id-outlier":
        assert rt[0][0]["ran_out"] and rt[0][0]["gathered"] == 11999
    if name == "card-moves":                     # the warm brackets (2 tau_prev, vmax] and (0, tau_prev / 2]
        assert rt[1][3] > float(TF(2.0 * rt[1][4])) and rt[1][0]["lo"] == float(TF(2.0 * rt[1][4]))
        assert rt[2][3] <= float(TF(0.5 * rt[2][4])) and rt[2][0]["hi"] <= float(TF(0.5 * rt[2][4]))


# =================================================================================================================
# C. the feasibility estimate
# =================================================================================================================
@pytest.mark.parametrize("TF", TFS)
@pytest.mark.parametrize("name,frac", [("card-dz-big-vec", 0.3), ("card-tv-3d", 0.3), ("card-dz-big-vec", 0.6)])
def test_feasibility_estimate_of_a_cardinality_set(sipx, TF, name, frac):
    """update_y_l with YL_FEAS at it = 10 and 20: the search on s = A x under the feasibility estimate (psf).  The returned
    feasibility against ||P(s) - s|| / (||s|| + 100 eps) in float64 from the TF elements of the exact selection, to the 8 eps(TF)
    of test_feasibility_searches_are_exact (its docstring derives it); the bracket of the search holds the exact tau.  Both
    searches are warm: the first from the tau of the initial feasibility estimate, taken on A m when the context was built, the
    second from its own.  frac = 0.6: k is above the non-zeros of s, every one of them survives and the feasibility is exactly 0."""
    case = dict(CASES[name], card_frac=frac)
    ch = Chain(sipx, case, TF)
    eps = float(np.finfo(TF).eps)
    try:
        i = ch.card[0]
        k = ch.cards[i]
        s = O.csc_mul(ch.Ao[i], ch.x)
        nnz = int((s != 0).sum())
        ps = O.project_cardinality(s.copy(), k)
        C.check_card_output(s, ps, k)
        s64 = s.astype(np.float64)
        ref = np.sqrt(((ps.astype(np.float64) - s64) ** 2).sum()) / (np.sqrt((s64 ** 2).sum()) + 100 * eps)
        sm = O.csc_mul(ch.Ao[i], ch.m)                  # the initial feasibility estimate searched |A m|
        tau_prev = kth(sm, k) if C.predict_route(sm, k, TF)["exit"] == "search" else None
        for call, it in enumerate((10, 20)):
            ch.step(np.ones(ch.p), np.ones(ch.p), flags=sipx.host.YL_FEAS, it=it)
            fe = ch.last["fe"][i]
            d = ch.ctx.debug_proj(i, 1)
            print(f"{name} {np.dtype(TF).name} k = {k} of {len(s)} (nnz {nnz}) call {call + 1}: feasibility engine {fe!r} reference {ref!r}")
            if frac > 0.5:
                assert k >= nnz and d["need"] == 0 and fe == 0.0 and ref == 0.0, (fe, d)
                continue
            assert k < nnz and ref > 0
            hold_search(f"feasibility {name} {np.dtype(TF).name} call {call + 1}", TF, s, k, d, tau_prev)
            tau_prev = kth(s, k)
            assert abs(fe - ref) <= 8 * eps * ref, (call, fe, ref)
    finally:
        ch.close()


# =================================================================================================================
# D. the slab-decomposed search
# =================================================================================================================
def _card_slab_worker(rank, world, port, out, name, env):
    import datetime
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **env)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    try:
        import torch
        from __graft_entry__ import load_package
        sipx = load_package()
        from sipx import sharded
        keep = []

        def attach(cx):
            keep.append(sharded.attach_comm(cx, dist, torch.device("cuda", 0), "torch"))
            cx.set_decomp("slab")
        case = CASES[name]
        res, ch = dict(err=""), None
        try:
            ch = Chain(sipx, case, np.float32, stats=False, device=0, owned=sharded.shard_sets(len(case["sets"]) + 1, world, rank), attach=attach)
            i = ch.card[0]
            for call, (fac, gam, _) in enumerate(case["sets"][i][-1]):
                f, g = np.ones(ch.p), np.ones(ch.p)
                f[i], g[i] = fac, gam
                rec = ch.step(f, g)[i]                 # (holds this rank's y, l to the oracle's replay from this rank's own state)
                d = rec["d"]
                res[f"y{call}"], res[f"l{call}"] = rec["y"], ch.l[i]
                res[f"d{call}"] = np.array([d["need"], d["lo"], d["hi"], d["vmax"], d["gathered"], d["refine"]])
        except sipx.SipxError as e:
            res = dict(err=str(e))
        finally:
            if ch is not None:
                ch.close()
        np.savez(os.path.join(out, f"r{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


def _spawn(tmp_path, world, name, env, offset):
    import torch.multiprocessing as mp
    mp.spawn(_card_slab_worker, args=(world, 32300 + os.getpid() % 1000 + offset, str(tmp_path), name, env), nprocs=world, join=True)
    return [np.load(tmp_path / f"r{r}.npz") for r in range(world)]


@pytest.mark.timeout(400)
@pytest.mark.parametrize("world,name", [(3, "card-dz-big-vec"), (2, "card-tv-3d")])
def test_slab_decomposed_search_is_the_stable_selection(sipx, tmp_path, world, name):
    """Float32, every rank on GPU 0, three calls (cold, warm, warm).  y and l of the cardinality set are complete on every rank:
    identical on all of them, the oracle's own chain bit for bit (replayed here without an engine), and the stable selection.
    A tie cut by local index, or segments strung together out of rank order, keeps other entries of the tie group.
    world 3, 16 planes as 6 + 6 + 4: the cut through the 11499 ones of the cold call falls inside the middle rank's planes --
    the first rank keeps all its ties, the last none.  world 2, TV: the blocks, and the z-block's halo plane, are split."""
    res = _spawn(tmp_path, world, name, {}, world)
    assert all(str(r["err"]) == "" for r in res), [str(r["err"]) for r in res]
    case = CASES[name]
    ref = Chain(None, case, np.float32)
    i = ref.card[0]
    k = ref.cards[i]
    for call, (fac, gam, _) in enumerate(case["sets"][i][-1]):
        f, g = np.ones(ref.p), np.ones(ref.p)
        f[i], g[i] = fac, gam
        o = ref.oracle_step(f, g)[i]
        for r in range(world):
            assert X.same_bits(res[r][f"y{call}"], res[0][f"y{call}"]) and X.same_bits(res[r][f"l{call}"], res[0][f"l{call}"]), (call, r)
            assert np.array_equal(res[r][f"d{call}"], res[0][f"d{call}"]), (call, r)
        y = res[0][f"y{call}"]
        C.check_card_output(o["v"], y, k)
        assert X.same_bits(y, o["y"]) and X.same_bits(res[0][f"l{call}"], o["l"]), call
        st, tau, group = C.straddles(o["v"], k)
        d = res[0][f"d{call}"]
        print(f"{name} world {world} call {call + 1}: tau {tau!r} in a group of {group}; engine bracket ({d[1]!r}, {d[2]!r}], gathered {d[4]:.0f}, ran out {d[5]:.0f}")
        assert st and d[0] == 1 and d[1] < float(tau) <= d[2]
        if name == "card-dz-big-vec" and call == 0:
            n = case["n"]
            tie = (np.abs(o["v"]) == tau).reshape((n[0], n[1], n[2] - 1), order="F")
            kept = (y != 0).reshape(tie.shape, order="F") & tie
            per = [(int(kept[:, :, a:b].sum()), int(tie[:, :, a:b].sum())) for a, b in ((0, 6), (6, 12), (12, 15))]
            print("kept ties per slab", per)
            assert group > C.CAP and per[0][0] == per[0][1] > 0 and 0 < per[1][0] < per[1][1] and per[2][0] == 0 < per[2][1], per


@pytest.mark.timeout(400)
def test_slab_overflow_of_a_cardinality_search_is_an_error_on_every_rank(sipx, tmp_path):
    """SIPX_GATHER_CAP=1024: an exchange segment holds a few hundred (index, magnitude) pairs, a rank's share of the 11499 ties
    cannot fit.  Both ranks return the SAME error, which names the search and the exchange segment -- no NaN iterate, no rank left
    in a collective (test_slab_gather_overflow_is_an_error_on_every_rank asserts this for l1)."""
    res = _spawn(tmp_path, 2, "card-dz-big-vec", {"SIPX_GATHER_CAP": "1024"}, 7)
    errs = [str(r["err"]) for r in res]
    print(errs[0])
    assert errs[0] and errs[0] == errs[1], errs
    assert "exchange segment" in errs[0] and "cardinality" in errs[0], errs[0]
    assert "cardinality search of set 1" in errs[0] or "initial feasibility of set 1" in errs[0], errs[0]
