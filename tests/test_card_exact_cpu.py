"""tests/card_exact.py on the CPU: the contract against the oracle's stable selection, the planted errors it must reject, and
the premise of every constructed input of tests/test_gpu_card_exact.py -- an input that stops exercising its route fails here."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import card_exact as C

TFS = [np.float32, np.float64]


@pytest.mark.parametrize("TF", TFS)
def test_contract_holds_for_the_oracle_on_every_input(TF):
    for n in C.LENGTHS:
        v = C.length_vector(n, TF)
        assert n < 7 or ((v == 0).sum() >= 2 and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all())
        for k in C.ks_for(v):
            C.check_card_output(v, O.project_cardinality(v.copy(), k), k)
    for name, v, ks, _ in C.named_vectors(TF):
        for k in ks:
            C.check_card_output(v, O.project_cardinality(v.copy(), k), k)


def test_the_sign_of_a_zero_is_not_part_of_the_contract():
    v = np.array([3, -0.0, 0.0, -2, 1], np.float32)
    C.check_card_output(v, np.array([3, 0.0, -0.0, -2, 0], np.float32), 2)
    C.check_card_output(v, np.array([3, -0.0, 0.0, -2, -0.0], np.float32), 2)


@pytest.mark.parametrize("TF", TFS)
def test_planted_errors_are_rejected_with_index_and_rule(TF):
    _, v, ks, _ = [e for e in C.named_vectors(TF) if e[0] == "big-tie"][0]
    k = ks[1]
    y = O.project_cardinality(v.copy(), k)
    C.check_card_output(v, y, k)
    tie = np.abs(v) == TF(0.75)
    kept, dropped = np.nonzero(tie & (y != 0))[0], np.nonzero(tie & (y == 0))[0]
    assert len(kept) == 5000 and len(dropped) == 5000
    # one tie kept out of index order: the last kept tie swapped for the first dropped one
    w = y.copy()
    for gone in (kept[-1], kept[0]):
        w = y.copy()
        w[gone], w[dropped[0]] = 0, v[dropped[0]]
        with pytest.raises(AssertionError, match=rf"rule 4 .* broke at index {gone}\b"):
            C.check_card_output(v, w, k)
    # one entry too many
    w = y.copy()
    w[dropped[0]] = v[dropped[0]]
    with pytest.raises(AssertionError, match=rf"rule 2 .* first difference at index {dropped[0]}\b"):
        C.check_card_output(v, w, k)
    # a kept value altered by one ulp
    w = y.copy()
    i = int(np.nonzero(y != 0)[0][17])
    w[i] = np.nextafter(w[i], TF(np.inf))
    with pytest.raises(AssertionError, match=rf"rule 1 .* broke at index {i}\b"):
        C.check_card_output(v, w, k)
    # a larger magnitude dropped for a smaller one
    big, small = int(np.argmax(np.abs(v))), int(np.nonzero((np.abs(v) < TF(0.75)) & (v != 0))[0][0])
    w = y.copy()
    w[big], w[small] = 0, v[small]
    with pytest.raises(AssertionError, match=rf"rule 3 .* broke at index {min(big, small)}\b"):
        C.check_card_output(v, w, k)


def test_predict_route_exits_and_warm_probes():
    v = np.array([0, 3, -2, 0, 1], np.float32)
    assert C.predict_route(v, 3, np.float32)["exit"] == "all" and C.predict_route(v, 5, np.float32)["exit"] == "all"
    assert C.predict_route(v, 0, np.float32)["exit"] == "none"
    r = C.predict_route(v, 2, np.float32)
    assert (r["exit"], r["passes"], r["lo"], r["hi"], r["gathered"]) == ("search", 0, 0.0, 3.0, 3)
    # a warm search around tau_prev = 2: the probes 1.998 and 2.002 bracket the second largest magnitude
    r = C.predict_route(v, 2, np.float32, probes=C.warm_probes(2.0, np.float32))
    assert r["lo"] == float(np.float32(2.0 * 0.999)) and r["hi"] == float(np.float32(2.0 * 1.001)) and r["gathered"] == 1
    # tau left [0.5, 2] tau_prev: the outermost probes are the bracket's ends
    r = C.predict_route(v, 2, np.float32, probes=C.warm_probes(0.75, np.float32))
    assert r["lo"] == 1.5 and r["hi"] == 3.0 and r["gathered"] == 2
    r = C.predict_route(v, 2, np.float32, probes=C.warm_probes(5.0, np.float32))
    assert r["lo"] == 0.0 and r["hi"] == 2.5 and r["gathered"] == 2


@pytest.mark.parametrize("TF", TFS)
def test_every_constructed_input_takes_its_intended_route(TF):
    seen = set()
    for name, v, ks, cls in C.named_vectors(TF):
        assert len(v) <= 100000
        for k in ks:
            r = C.predict_route(v, k, TF)
            st, tau, group = C.straddles(v, k)
            print(f"{np.dtype(TF).name} {name} k = {k}: {r}; tie group at the k-th place {group}")
            assert r["exit"] == "search" and r["lo"] < float(tau) <= r["hi"], (name, k, r)
            seen.add(cls)
            if cls == "refined":
                assert r["passes"] >= 1 and not r["ran_out"] and r["gathered"] <= C.CAP, (name, k, r)
            elif cls == "ran-out":
                assert r["passes"] == 5 and r["ran_out"] and r["gathered"] > C.CAP, (name, k, r)
            elif cls == "collapsed":
                assert r["passes"] == 5 and r["ran_out"] and r["gathered"] > C.CAP and r["collapsed"] >= 24, (name, k, r)
                assert np.nextafter(TF(r["lo"]), TF(np.inf)) == TF(r["hi"])           # one ulp wide: three whole passes decided nothing
            else:
                assert cls == "bottom" and r["passes"] == 0 and r["hi"] < 2 * float(np.finfo(TF).tiny)
                sub = np.abs(v) < np.finfo(TF).tiny
                assert 1000 < sub.sum() < 4000 and (v[sub] != 0).all() and (v < 0).any() and (v > 0).any()
            if name == "uniform":
                assert r["passes"] == 2 and 1000 < r["gathered"] < 1500
            if name == "outlier":
                assert r["gathered"] == 49999 and r["lo"] == 0.0
            if name in ("big-tie", "all-tie", "cluster", "subnormal-ties"):
                assert st, (name, k)                        # #{|v| > tau} < k < #{|v| >= tau}
            if name in ("big-tie", "all-tie", "subnormal-ties"):
                assert group > C.CAP, (name, group)
            if name == "big-tie":
                assert group == 10000 and float(tau) == 0.75 and 10000 <= r["gathered"] < 10100
            if name == "all-tie":
                assert r["gathered"] == len(v) == 20000
            if name == "cluster":
                assert r["passes"] == 4
                if TF == np.float32:                        # 30000 entries on the 8193 floats of [1, 1 + 2^-10]: 97 % of them occupied
                    u = np.unique(np.abs(v))
                    assert len(u) > 0.97 * 8193 and u[0] >= 1 and u[-1] <= 1 + 2.0 ** -10 and group >= 2
    assert seen == {"refined", "ran-out", "collapsed", "bottom"}
