"""The fit path's workspace sizes and layouts, without a GPU.

bo_invert_k_workspace_size and bo_compute_mll_workspace_size (callers cache what they return) against
the independent restatement in tests/fit_layout_model.py; the model's own invariants; and how the size
functions and the entry points treat n_obj = 0, n_obj = 9 (> BO_MAX_OBJ) and n = 0."""
import ctypes as C

import numpy as np
import pytest

import fit_layout_model as M

NS = [1, 31, 32, 33, 512, 1536, 1537, 2048, 2049, 4096, 32768]
N_OBJ = [1, 2, 3, 8]


@pytest.fixture(scope="module")
def lib():
    from bayesopt_smart_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("n_obj", N_OBJ)
def test_totals_equal_the_model(lib, n_obj):
    for n in NS:
        assert lib.bo_invert_k_workspace_size(n_obj, n) == M.inv_layout(n, n_obj)[1], ("inverse", n)
        assert lib.bo_compute_mll_workspace_size(n_obj, n) == M.mll_layout(n, n_obj)[1], ("mll", n)


def _check_arrays(arrays, total, aligned):
    end = 0
    starts = []
    for name, off, used in arrays:
        assert off >= end, (name, "overlaps the array before it")
        if aligned:
            assert off % 256 == 0, name
        if used:
            starts.append(off)
        end = off + used
    assert end <= total
    assert starts == sorted(set(starts)), "offsets of the arrays in use are strictly increasing"


@pytest.mark.parametrize("n_obj", N_OBJ)
def test_model_invariants(n_obj):
    for n in NS:
        inv, inv_total = M.inv_layout(n, n_obj)
        _check_arrays(inv, inv_total, aligned=True)
        assert inv_total % 256 == 0
        names = {k: (off, used) for k, off, used in inv}
        # the Gauss-Jordan pair exists exactly above the LU's capacity, where the LU cannot run
        assert (names["bufA"][1] > 0) == (names["bufB"][1] > 0) == (n > M.LU_MAX_N)
        if n <= M.LU_MAX_N:
            assert names["bufA"][0] == names["bufB"][0] == names["piv"][0]
            # ... and below it the LU batch of every objective fits the augmented matrices' region
            assert M.lu_workspace(n, n_obj) <= M.geo_bytes(M.geo(n, n_obj, True))
        assert 4 * max(M.INV_STATUS_GJ, M.INV_STATUS_ABORT) < 4 * (M.MAX_OBJ + 4) <= 256 < 512
        assert M.INV_STATUS_GJ >= M.MAX_OBJ and M.INV_STATUS_ABORT >= M.MAX_OBJ and M.INV_STATUS_GJ != M.INV_STATUS_ABORT
        mll, mll_total = M.mll_layout(n, n_obj)
        _check_arrays(mll, mll_total, aligned=True)
        assert mll_total % 256 == 0
        host, host_total = M.mll_host(n, n_obj)
        _check_arrays(host, host_total, aligned=False)
        assert [k for k, _, _ in host] == ["part", "status", "abort", "done"]
        assert all(off % 4 == 0 for _, off, _ in host) and host[0][1] % 8 == 0
    for n in [1, 15, 16, 17, 512, 2048]:
        slot, total = M.lu_slot(n)
        _check_arrays(slot, total, aligned=True)
        assert M.lu_workspace(n, n_obj) == n_obj * total + 256


def test_flag_words_hold_every_flag_of_the_persistent_schedule():
    for n, n_obj, ident in [(33, 3, True), (33, 3, False), (1536, 8, True), (1536, 8, False)]:
        g = M.geo(n, n_obj, ident)
        nbt = g["nbt"]
        rb = 2 * nbt if ident else nbt + 1
        per = nbt * nbt + rb * nbt + nbt * nbt
        # the last word any pf_* accessor can reach: tverC[nbt - 1][nbt - 1] of the last objective
        last = 16 + (n_obj - 1) * per + nbt * nbt + rb * nbt + (nbt - 1) * nbt + (nbt - 1)
        assert last == M.flag_words(g) - 1


def test_rejections(lib):
    from bayesopt_smart_amd import _lib
    for size in (lib.bo_invert_k_workspace_size, lib.bo_compute_mll_workspace_size):
        assert size(0, 64) == 0 and size(-1, 64) == 0 and size(3, 0) == 0 and size(3, -5) == 0
    # the size functions do not know BO_MAX_OBJ (they return the formula's value); the entry points reject it
    assert lib.bo_invert_k_workspace_size(9, 64) == M.inv_layout(64, 9)[1] > 0
    assert lib.bo_compute_mll_workspace_size(9, 64) == M.mll_layout(64, 9)[1] > 0
    # host buffers only: every call below is rejected before any device work
    n = 4
    km = np.zeros((9, n, n))
    out = np.zeros((9, n, n))
    x = np.zeros((n, 2))
    y = np.zeros((n, 9))
    v = (C.c_double * 9)(*([1.0] * 9))
    mll = (C.c_double * 9)()
    p = lambda a: a.ctypes.data  # noqa: E731

    def inv(n_obj, nn):
        return lib.bo_invert_k_ex(p(out), p(km), n, n_obj, nn, 1e-6, None, None, None, 0, None)

    def mll_each(n_obj, nn):
        return lib.bo_compute_mll_each_jitter(mll, p(x), 2, p(y), 9, p(km), n, n_obj, v, v, v, nn, 1e-8, None, 0, None)

    for call in (inv, mll_each):
        assert call(0, n) == _lib.ERR_ARG
        assert call(9, n) == _lib.ERR_ARG
        assert call(3, 0) == _lib.ERR_ARG
        assert call(3, n) == _lib.ERR_WORKSPACE          # valid arguments, no workspace
    assert inv(3, 32769) == _lib.ERR_ARG                  # ld < n comes first
    assert lib.bo_invert_k_ex(p(out), p(km), 1 << 16, 3, 32769, 1e-6, None, None, None, 0, None) == _lib.ERR_UNSUPPORTED
