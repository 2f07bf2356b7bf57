"""CPU-side checks of PARSDMM_device (the device-resident form of the whole solve): everything that can be wrong with its tensor
arguments is refused on the host, with a message that names the argument, before libsipx.so is loaded; and the package does
not pull torch in when it is imported."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def problem(sipx, monkeypatch):
    """{bounds, l1 on TV} on a 12 x 10 grid, and a library that must not be touched."""
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(sipx.host, "lib", no_library)
    TF, n = np.float32, (12, 10)
    g = sipx.compgrid((1.0, 1.0), n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=5)
    c = [sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("matrix", "")),
         sipx.set_definitions("l1", "TV", 0.0, 3.0, ("matrix", ""))]
    P, A, prop = sipx.setup_constraints(c, g, TF)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    rows = [a.shape[0] for a in A]
    assert rows == [120, 11 * 10 + 12 * 9, 120]
    return dict(args=(AtA, A, prop, P, g, opt), N=120, rows=rows)


class FakeCuda:
    """Stands in for a tensor on a GPU where there is none: the checks read its attributes only."""
    __module__ = "torch"

    def __init__(self, n, dtype="torch.float32", contiguous=True, shape=None, device="cuda:0"):
        import torch
        self.dtype = getattr(torch, dtype.split(".")[1])
        self.shape = (n,) if shape is None else shape
        self.device = torch.device(device)
        self.is_cuda = self.device.type == "cuda"
        self._c = contiguous

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        raise AssertionError("a pointer was taken before the arguments were checked")


def test_cpu_tensor_is_refused_before_any_library_load(sipx, problem):
    import torch
    with pytest.raises(sipx.SipxError, match=r"\bm must live on a GPU"):
        sipx.PARSDMM_device(torch.zeros(problem["N"]), *problem["args"])


def test_numpy_array_is_refused(sipx, problem):
    with pytest.raises(sipx.SipxError, match="m must be a torch tensor"):
        sipx.PARSDMM_device(np.zeros(problem["N"], np.float32), *problem["args"])


def test_wrong_dtype_is_refused(sipx, problem):
    import torch
    with pytest.raises(sipx.SipxError, match="m must be Float32 or Float64"):
        sipx.PARSDMM_device(torch.zeros(problem["N"], dtype=torch.float16), *problem["args"])
    m = FakeCuda(problem["N"])
    with pytest.raises(sipx.SipxError, match=r"x has dtype torch.float64: not the working precision"):
        sipx.PARSDMM_device(m, *problem["args"], x=FakeCuda(problem["N"], "torch.float64"))
    with pytest.raises(sipx.SipxError, match=r"y\[1\] has dtype torch.float64"):
        ys = [FakeCuda(r, "torch.float64" if i == 1 else "torch.float32") for i, r in enumerate(problem["rows"])]
        sipx.PARSDMM_device(m, *problem["args"], y=ys)


def test_non_contiguous_tensor_is_refused(sipx, problem):
    import torch
    with pytest.raises(sipx.SipxError, match="m must live on a GPU"):      # (a real strided CPU tensor: the device comes first)
        sipx.PARSDMM_device(torch.zeros(2 * problem["N"])[::2], *problem["args"])
    with pytest.raises(sipx.SipxError, match="m must be contiguous"):
        sipx.PARSDMM_device(FakeCuda(problem["N"], contiguous=False), *problem["args"])
    with pytest.raises(sipx.SipxError, match=r"l\[0\] must be contiguous"):
        ls = [FakeCuda(r, contiguous=(i != 0)) for i, r in enumerate(problem["rows"])]
        sipx.PARSDMM_device(FakeCuda(problem["N"]), *problem["args"], l=ls)
    with pytest.raises(sipx.SipxError, match="m must be 1-D"):
        sipx.PARSDMM_device(FakeCuda(problem["N"], shape=(12, 10)), *problem["args"])


def test_wrongly_sized_tensors_are_refused(sipx, problem):
    N, rows = problem["N"], problem["rows"]
    with pytest.raises(sipx.SipxError, match=f"m has {N + 1} entries, {N} are needed"):
        sipx.PARSDMM_device(FakeCuda(N + 1), *problem["args"])
    with pytest.raises(sipx.SipxError, match=f"x has {N - 1} entries"):
        sipx.PARSDMM_device(FakeCuda(N), *problem["args"], x=FakeCuda(N - 1))
    with pytest.raises(sipx.SipxError, match=rf"l\[1\] has {N} entries, {rows[1]} are needed"):
        sipx.PARSDMM_device(FakeCuda(N), *problem["args"], l=[FakeCuda(N) for _ in rows])
    with pytest.raises(sipx.SipxError, match=r"out x has 7 entries"):
        sipx.PARSDMM_device(FakeCuda(N), *problem["args"], out=(FakeCuda(7), None, None))


def test_list_of_the_wrong_length_is_refused(sipx, problem):
    N, rows = problem["N"], problem["rows"]
    with pytest.raises(sipx.SipxError, match=r"l needs one vector per term \(sets plus the distance term\): 3, not 2"):
        sipx.PARSDMM_device(FakeCuda(N), *problem["args"], l=[FakeCuda(r) for r in rows[:2]])
    with pytest.raises(sipx.SipxError, match=r"y needs one vector per term"):
        sipx.PARSDMM_device(FakeCuda(N), *problem["args"], y=FakeCuda(N))
    with pytest.raises(sipx.SipxError, match=r"out y needs one vector per term"):
        sipx.PARSDMM_device(FakeCuda(N), *problem["args"], out=(None, [FakeCuda(r) for r in rows], [FakeCuda(rows[0])]))


def test_tensors_on_another_device_are_refused(sipx, problem):
    with pytest.raises(sipx.SipxError, match=r"x lives on cuda:1, m on cuda:0"):
        sipx.PARSDMM_device(FakeCuda(problem["N"]), *problem["args"], x=FakeCuda(problem["N"], device="cuda:1"))


def test_outputs_argument_is_checked(sipx, problem):
    with pytest.raises(sipx.SipxError, match="outputs must be"):
        sipx.PARSDMM_device(FakeCuda(problem["N"]), *problem["args"], outputs="l")


def test_importing_the_package_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); from __graft_entry__ import load_package; s = load_package(); "
            "assert hasattr(s, 'PARSDMM_device'); print('torch' in sys.modules)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, cwd=ROOT)
    assert out.stdout.strip() == "False", out.stdout + out.stderr
