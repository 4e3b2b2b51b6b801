"""Look-ahead of the block-column Cholesky (chol_col.hip): the launch of column k - 1 parks the leader's accumulators for
column k (slabs 0 .. k - 2) in block k of the inverse table, the leader of launch k runs the last slab only.  The matrix core
sees the same operands in the same order, so gp_col_leader = 1 (look-ahead) and 2 (the leader forms its whole product) must
agree bit for bit.  n = 64: one column; n = 192: the first size where a parked accumulator is consumed; n = 256: two."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, BATCH = 64, 3


@pytest.fixture(scope="module")
def lib(built_lib):
    assert torch.cuda.is_available()
    return built_lib


_REF = {}


def _system(n):
    """SPD matrices shaped like the GP system (exp((cos - 1) / 0.2) Gram + 0.1 I), right-hand sides, f64 factor and solution"""
    if n not in _REF:
        g = np.random.Generator(np.random.PCG64(300 + n))
        y = torch.from_numpy(g.standard_normal(size=(BATCH, n, 40), dtype=np.float32))
        yn = y / y.norm(dim=-1, keepdim=True)
        A = torch.exp((yn @ yn.transpose(1, 2) - 1.0) / 0.2) + 0.1 * torch.eye(n)
        Ft = torch.from_numpy(g.standard_normal(size=(BATCH, D, n), dtype=np.float32))
        Lref = torch.linalg.cholesky(A.double())
        _REF[n] = (A, Ft, Lref, torch.cholesky_solve(Ft.transpose(1, 2).double(), Lref))
    return _REF[n]


@pytest.mark.parametrize("n", [64, 192, 256])
def test_lookahead_is_bit_identical_and_carries_nothing_between_solves(lib, n):
    A, Ft, Lref, Xref = _system(n)
    # one (n + D) x n matrix per item, items (n + D) * n floats apart: the augmented form (chol_col.hip)
    buf = torch.empty((BATCH, (n + D) * n), device="cuda")
    LT = torch.empty((BATCH, n, n), device="cuda")
    Linv = torch.empty((BATCH, n // 64, 64, 64), device="cuda")
    LinvT = torch.empty_like(Linv)
    A_dev, Ft_dev = A.reshape(BATCH, -1).cuda(), Ft.reshape(BATCH, -1).cuda()
    outs = {}
    try:
        # (1, 1): two solves back to back on the same buffers - what the first one parked (and the inverses it left where the
        # second one parks) must not reach the second one's result
        for mode in (1, 1, 2):
            assert lib.roma_tuning(b"gp_col_leader", mode) == 0
            buf[:, :n * n] = A_dev
            buf[:, n * n:] = Ft_dev
            rc = lib.roma_op_cholesky_solve_t(C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + n * n * 4), C.c_void_p(LT.data_ptr()),
                                              C.c_void_p(Linv.data_ptr()), C.c_void_p(LinvT.data_ptr()), n, D, BATCH, None)
            assert rc == 0, lib.roma_last_error().decode()
            torch.cuda.synchronize()
            X = buf[:, n * n:].reshape(BATCH, D, n).cpu()
            L = torch.tril(buf[:, :n * n].reshape(BATCH, n, n)).cpu()
            outs.setdefault(mode, []).append((X, L, Linv.cpu(), LinvT.cpu()))
    finally:
        lib.roma_tuning(b"gp_col_leader", -1)
    for got in (outs[1][0], outs[1][1]):
        for a, b in zip(got, outs[2][0]):
            assert torch.equal(a, b)
    for X, L, _, _ in (outs[1][0], outs[2][0]):  # the f64 bounds of tests/test_gpu_ops.py::test_cholesky_solve*
        assert torch.allclose(X.transpose(1, 2).double(), Xref, atol=2e-4, rtol=1e-4), float((X.transpose(1, 2).double() - Xref).abs().max())
        assert torch.allclose(L.double(), Lref, atol=1e-4), float((L.double() - Lref).abs().max())
