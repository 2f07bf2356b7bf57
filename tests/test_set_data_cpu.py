"""CPU-side checks of Solver (one context, many projections, the vectors of a data-bearing set replaced in between): everything
that can be wrong with its arguments is refused on the host, with a message that names the argument, before libsipx.so is
loaded."""
import numpy as np
import pytest

from tests.test_device_io_cpu import FakeCuda

TF, n = np.float32, (12, 10, 4)


@pytest.fixture
def solver(sipx, monkeypatch):
    """{scalar bounds, element-wise box on TV, per-fiber bounds along z on D_z, histogram} on a 12 x 10 x 4 grid, and a library
    that must not be touched."""
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(sipx.host, "lib", no_library)
    g = sipx.compgrid((1.0, 1.0, 1.0), n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=5)
    N = 480
    M = 11 * 10 * 4 + 12 * 9 * 4 + 12 * 10 * 3
    c = [sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")),
         sipx.set_definitions("bounds", "TV", np.zeros(M, TF), np.ones(M, TF), ("tensor", "")),
         sipx.set_definitions("bounds", "D_z", np.zeros(3, TF), np.ones(3, TF), ("fiber", "z")),
         sipx.set_definitions("histogram", "identity", np.zeros(N, TF), np.ones(N, TF), ("tensor", "")),
         sipx.set_definitions("bounds", "DCT", np.zeros(N, TF), np.ones(N, TF), ("tensor", ""))]
    P, A, prop = sipx.setup_constraints(c, g, TF)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    S = sipx.Solver(AtA, A, prop, P, g, opt, TF)
    S.sizes = dict(N=N, M=M)
    return S


def test_the_solver_is_exported_with_the_two_symbols(sipx):
    assert sipx.Solver is sipx.host.Solver
    assert {"sipx_set_data", "sipx_set_data_dev"} <= set(sipx.EXPORTED_SYMBOLS)
    assert callable(sipx.Context.set_data) and callable(sipx.Context.set_data_dev)


def test_shapes_are_checked_per_kind(sipx, solver):
    M, N = solver.sizes["M"], solver.sizes["N"]
    with pytest.raises(sipx.SipxError, match=f"lb has {N} entries, {M} are needed"):
        solver.set_data(1, np.zeros(N, TF), np.zeros(M, TF))
    with pytest.raises(sipx.SipxError, match="ub has 4 entries, 3 are needed"):        # fibers of D_z along z: n3 - 1
        solver.set_data(2, np.zeros(3, TF), np.zeros(4, TF))
    with pytest.raises(sipx.SipxError, match=f"ub has 3 entries, {N} are needed"):
        solver.set_data(3, ub=np.zeros(3, TF))
    with pytest.raises(sipx.SipxError, match="lb must be 1-D"):
        solver.set_data(3, lb=np.zeros((N, 1), TF))
    with pytest.raises(sipx.SipxError, match=f"lb has {M + 1} entries"):
        solver.set_data(1, FakeCuda(M + 1), FakeCuda(M))
    solver.set_data(1)                          # nothing given: nothing to do, nothing loaded


def test_dtypes_are_checked(sipx, solver):
    M = solver.sizes["M"]
    with pytest.raises(sipx.SipxError, match="lb has dtype float64: not the working precision"):
        solver.set_data(1, np.zeros(M), np.zeros(M, TF))
    with pytest.raises(sipx.SipxError, match="ub has dtype torch.float64: not the working precision"):
        solver.set_data(1, FakeCuda(M), FakeCuda(M, "torch.float64"))
    with pytest.raises(sipx.SipxError, match="lb must be a numpy array"):
        solver.set_data(1, [0.0] * M, None)


def test_host_and_device_vectors_do_not_mix(sipx, solver):
    M = solver.sizes["M"]
    with pytest.raises(sipx.SipxError, match="both be numpy arrays or both be tensors"):
        solver.set_data(1, np.zeros(M, TF), FakeCuda(M))
    import torch
    with pytest.raises(sipx.SipxError, match="lb must live on a GPU"):
        solver.set_data(1, torch.zeros(M), torch.zeros(M))
    with pytest.raises(sipx.SipxError, match="ub must be contiguous"):
        solver.set_data(1, FakeCuda(M), FakeCuda(M, contiguous=False))


def test_tensors_on_another_device_are_refused(sipx, solver):
    M = solver.sizes["M"]
    with pytest.raises(sipx.SipxError, match=r"ub lives on cuda:1, lb on cuda:0"):
        solver.set_data(1, FakeCuda(M), FakeCuda(M, device="cuda:1"))
    solver.device = 0
    with pytest.raises(sipx.SipxError, match=r"the tensors live on cuda:1, the Solver on cuda:0"):
        solver.set_data(1, FakeCuda(M, device="cuda:1"), FakeCuda(M, device="cuda:1"))
    with pytest.raises(sipx.SipxError, match=r"the tensors live on cuda:1, the Solver on cuda:0"):
        solver(FakeCuda(solver.sizes["N"], device="cuda:1"))


def test_sets_without_replaceable_data_are_refused(sipx, solver):
    N = solver.sizes["N"]
    for i, what in ((0, "bounds on identity"), (4, "bounds on DCT")):
        with pytest.raises(sipx.SipxError, match=rf"set {i} \({what}\) holds no replaceable vectors.*build a new Solver"):
            solver.set_data(i, np.zeros(N, TF), np.ones(N, TF))
    with pytest.raises(sipx.SipxError, match="index 5 is the distance term"):
        solver.set_data(5, np.zeros(N, TF), np.ones(N, TF))
    for i in (-1, 6):
        with pytest.raises(sipx.SipxError, match=r"out of range \(5 sets\)"):
            solver.set_data(i, np.zeros(N, TF), np.ones(N, TF))
    with pytest.raises(sipx.SipxError, match="index must be an integer"):
        solver.set_data("1", np.zeros(N, TF), np.ones(N, TF))


def test_the_call_checks_its_arguments_like_parsdmm_device(sipx, solver):
    N, rows = solver.sizes["N"], solver.rows
    assert rows == [N, solver.sizes["M"], 360, N, N, N]
    with pytest.raises(sipx.SipxError, match=f"m has {N + 1} entries, {N} are needed"):
        solver(FakeCuda(N + 1))
    with pytest.raises(sipx.SipxError, match=f"m has {N - 1} entries, {N} are needed"):
        solver(np.zeros(N - 1, TF))
    with pytest.raises(sipx.SipxError, match="m has dtype float64"):
        solver(np.zeros(N))
    with pytest.raises(sipx.SipxError, match="m has dtype torch.float64"):
        solver(FakeCuda(N, "torch.float64"))
    with pytest.raises(sipx.SipxError, match="m must be a numpy array or a torch tensor"):
        solver([0.0] * N)
    with pytest.raises(sipx.SipxError, match=r"y\[1\] has 480 entries"):
        solver(FakeCuda(N), y=[FakeCuda(N) for _ in rows])
    with pytest.raises(sipx.SipxError, match=r"x lives on cuda:1, m on cuda:0"):
        solver(FakeCuda(N), x=FakeCuda(N, device="cuda:1"))
    with pytest.raises(sipx.SipxError, match="x must be a numpy vector"):
        solver(np.zeros(N, TF), x=FakeCuda(N))
    with pytest.raises(sipx.SipxError, match="l needs one numpy vector per term"):
        solver(np.zeros(N, TF), l=[np.zeros(N, TF)])
    with pytest.raises(sipx.SipxError, match="out x has 7 entries"):
        solver(FakeCuda(N), out=(FakeCuda(7), None, None))
    with pytest.raises(sipx.SipxError, match="out takes preallocated tensors"):
        solver(np.zeros(N, TF), out=(np.zeros(N, TF), None, None))
    with pytest.raises(sipx.SipxError, match="outputs must be"):
        solver(np.zeros(N, TF), outputs="l")


def test_the_list_is_checked_when_the_solver_is_made(sipx, solver):
    args = (solver.AtA, solver.TD_OP, solver.set_Prop, solver.P_sub, solver.comp_grid, solver.options)
    with pytest.raises(sipx.SipxError, match="one operator per set plus the identity"):
        sipx.Solver(args[0], args[1][:-1], *args[2:], TF)
    with pytest.raises(sipx.SipxError, match=r"P_sub\[0\] must be a Projector"):
        sipx.Solver(args[0], args[1], args[2], [lambda v: v] + args[3][1:], args[4], args[5], TF)
    with pytest.raises(sipx.SipxError, match=r"P_sub\[0\] was set up in float32, the Solver in float64"):
        sipx.Solver(*args, np.float64)
    with pytest.raises(sipx.SipxError, match="FL must be Float32 or Float64"):
        sipx.Solver(*args, np.float16)


def test_a_closed_solver_refuses_and_the_caches_do_not_know_it(sipx, solver):
    assert not sipx.host._ctx_cache or all(c is not solver.ctx for c in sipx.host._ctx_cache.values())
    with solver as S:
        assert S is solver and not S.closed
    assert solver.closed and solver.ctx is None
    with pytest.raises(sipx.SipxError, match="has been closed"):
        solver.set_data(1, np.zeros(3, TF), None)
    with pytest.raises(sipx.SipxError, match="has been closed"):
        solver(np.zeros(solver.sizes["N"], TF))
