"""GPU tests of the fit path's workspace layouts (InvLayout / MllLayout, bo_fit.hip; the LU slot,
bo_lu.hip): bo_compute_mll_each_jitter and bo_invert_k_ex, called through ctypes in a workspace of
exactly the reported size between two guard regions, write neither guard, and every output is bit
for bit that of the same call through bo.kernels on the package's ordinary workspace.

The buffer is filled with 0xA5 (flag words far past any version, statuses set, offsets out of
range), the workspace starts at its byte 4096 (256-aligned) and ws_bytes is the exact size.

  n = 33, 3 objectives    two column blocks, ragged: MLL, the Cholesky inverse, the LU inverse
  n = 1537, 1 objective   49 column blocks: launch-per-step is the default (path counts checked)
  n = 2049, 1 objective   one row past the LU's capacity: Gauss-Jordan (path 2 and its count)"""
import ctypes as C

import numpy as np
import pytest

import fit_layout_model as M
from test_gpu_fit_sweep import _problem as _sweep_problem

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xA5
_PROBLEMS = {}


def _problem(n, n_obj):
    if (n, n_obj) not in _PROBLEMS:
        _PROBLEMS[(n, n_obj)] = _sweep_problem(n, n_obj, 2)
    return _PROBLEMS[(n, n_obj)]


@pytest.fixture(scope="module")
def bo():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import bayesopt_smart_amd as bo
    bo._lib.load()
    return bo


class _Guarded:
    """A workspace of exactly `nbytes` in the middle of a buffer of its own."""

    def __init__(self, nbytes):
        import torch
        assert nbytes > 0 and nbytes % 256 == 0
        self.nbytes = int(nbytes)
        self.buf = torch.empty(self.nbytes + 2 * GUARD, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 256 == 0
        self.buf.fill_(FILL)

    def check(self):
        import torch
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == FILL).all()), "written below the workspace"
        assert bool((self.buf[GUARD + self.nbytes:] == FILL).all()), "written past the workspace"


def _stream(bo):
    return bo.device.stream_handle(bo.device.require_device())


def _delta(before, after):
    return {k: after[k] - before[k] for k in after}


def _vec(v):
    return (C.c_double * len(v))(*[float(a) for a in v])


def _mll_guarded(bo, n, n_obj):
    """bo_compute_mll_each_jitter in a guarded workspace: terms and kernel_matrix bit-equal to bo.kernels';
    returns how the guarded call moved bo_fit_path_counts."""
    import torch
    lib = bo._lib.load()
    x, y, pm, pv, ls, _, _ = _problem(n, n_obj)
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    km = torch.zeros((n_obj, n, n), dtype=torch.float64, device="cuda")
    nbytes = lib.bo_compute_mll_workspace_size(n_obj, n)
    assert nbytes == M.mll_layout(n, n_obj)[1]
    g = _Guarded(nbytes)
    out = (C.c_double * n_obj)()
    before = bo._lib.fit_path_counts()
    st = lib.bo_compute_mll_each_jitter(out, xd.data_ptr(), xd.shape[1], yd.data_ptr(), yd.stride(0), km.data_ptr(), n,
                                        n_obj, _vec(pm), _vec(pv), _vec(ls), n, 1e-8, g.ptr, g.nbytes, _stream(bo))
    moved = _delta(before, bo._lib.fit_path_counts())
    g.check()
    assert st == bo._lib.OK, st
    km_ref = torch.zeros_like(km)
    ref = bo.kernels._mll_terms(xd, yd, km_ref, pm, pv, ls, n, list(range(n_obj)), jitter=1e-8)
    got = np.array([out[o] for o in range(n_obj)])
    want = np.array([ref[o] for o in range(n_obj)])
    assert np.all(np.isfinite(want))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(km.cpu().numpy(), km_ref.cpu().numpy())
    return moved


def _inv_guarded(bo, n, n_obj, lu):
    """bo_invert_k_ex in a guarded workspace: K^-1 and the paths bit-equal to bo.kernels.invert_k's; returns
    K^-1, the paths, and how the guarded call moved bo_invert_k_path_counts and bo_fit_path_counts."""
    import torch
    lib = bo._lib.load()
    km = torch.tensor(_problem(n, n_obj)[5], device="cuda")
    nbytes = lib.bo_invert_k_workspace_size(n_obj, n)
    assert nbytes == M.inv_layout(n, n_obj)[1]
    g = _Guarded(nbytes)
    out = torch.zeros((n_obj, n, n), dtype=torch.float64, device="cuda")
    hint = (C.c_int32 * n_obj)(*([1 if lu else 0] * n_obj))
    taken = (C.c_int32 * n_obj)(*([-1] * n_obj))
    before = bo._lib.invert_k_path_counts(), bo._lib.fit_path_counts()
    st = lib.bo_invert_k_ex(out.data_ptr(), km.data_ptr(), n, n_obj, n, 1e-6, hint, taken, g.ptr, g.nbytes, _stream(bo))
    moved = _delta(before[0], bo._lib.invert_k_path_counts()), _delta(before[1], bo._lib.fit_path_counts())
    g.check()
    assert st == bo._lib.OK, st
    ref_taken = []
    ref = bo.kernels.invert_k(n, km, lu_hint=[lu] * n_obj, paths=ref_taken)
    assert [int(t) for t in taken] == ref_taken
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, ref.cpu().numpy())
    return got, ref_taken, moved[0], moved[1]


def test_two_ragged_blocks_mll(bo):
    assert _mll_guarded(bo, 33, 3) == {"persistent": 1, "launches": 0, "aborted": 0}


@pytest.mark.parametrize("path", ["cholesky", "lu"])
def test_two_ragged_blocks_inverse(bo, path):
    _, taken, inv_moved, fit_moved = _inv_guarded(bo, 33, 3, lu=path == "lu")
    assert taken == [{"cholesky": 0, "lu": 1}[path]] * 3
    assert inv_moved[path] == 3 and sum(inv_moved.values()) == 3, inv_moved
    # the hint on every objective skips the factorisation altogether
    assert fit_moved == {"persistent": 0 if path == "lu" else 1, "launches": 0, "aborted": 0}


def test_launch_per_step_above_48_blocks(bo):
    n = 1537
    assert -(-n // 32) == 49
    assert _mll_guarded(bo, n, 1) == {"persistent": 0, "launches": 1, "aborted": 0}
    _, taken, inv_moved, fit_moved = _inv_guarded(bo, n, 1, lu=False)
    assert taken == [0] and inv_moved == {"cholesky": 1, "lu": 0, "gauss_jordan": 0}
    assert fit_moved == {"persistent": 0, "launches": 1, "aborted": 0}


def test_gauss_jordan_one_row_past_the_lu(bo):
    """The Gauss-Jordan driver's arrays (the matrix pair, piv, perm, its status word): guards, bit equality
    with the ordinary workspace, path 2 and its count.

    Not asserted: the sweep's residual rule |(K + 1e-6 I) X - I|_max <= max(10 res_LAPACK, 1e-12).  The
    library from before the layouts were single-sourced misses it on this problem (cond 7.6e5): residual
    4.25e-10 against LAPACK's 2.05e-11, 20.8x, on an MI355X.  The inverse here is bit for bit that one, so
    the rule is left to the change that improves Gauss-Jordan's accuracy; the residual is printed."""
    n = M.LU_MAX_N + 1
    assert n == 2049
    km, cond = _problem(n, 1)[5], _problem(n, 1)[6]
    got, taken, inv_moved, _ = _inv_guarded(bo, n, 1, lu=True)
    assert taken == [2]
    assert inv_moved == {"cholesky": 0, "lu": 0, "gauss_jordan": 1}, inv_moved
    a = km[0] + 1e-6 * np.eye(n)
    res_got = np.abs(a @ got[0] - np.eye(n)).max()
    print(f"N {n} Gauss-Jordan: cond {cond:.1e}, residual {res_got:.2e} (LAPACK's: 2.05e-11)")
    # an inverse at all (a scrambled pivot or permutation array leaves O(1)): the first-order bound
    # n eps cond of elimination with partial pivoting, 3.5e-7 here
    assert res_got <= n * np.finfo(np.float64).eps * cond
