"""tests/bucb_layout_model.py against the library's size queries, without a GPU: the model's total is
bo_select_batch_bucb_workspace_size and bo_select_batch_gibbon_workspace_size, and no more than
bo_select_batch_kb_workspace_size (whose layout opens with the update's); the model's own invariants."""
import ctypes as C

import numpy as np
import pytest

import bucb_layout_model as M


@pytest.fixture(scope="module")
def lib():
    from bayesopt_smart_amd import _lib
    return _lib.load()


def fill(d, n_train, dim, n_obj, q, n_cand, ld, var_out, grid):
    from bayesopt_smart_amd import _lib
    d.n_obj, d.dim, d.n_train, d.ld_k = n_obj, dim, n_train, n_train + 3
    d.q, d.n_cand, d.cand_offset, d.ld = q, n_cand, 0, ld
    d.cand_kind = _lib.CAND_GRID if grid else _lib.CAND_F64
    for k in range(min(dim, 8)):
        d.grid_lo[k], d.grid_shape[k] = -3, (n_cand if k == dim - 1 else 1)
    for o in range(min(n_obj, 8)):
        d.prior_var[o], d.length_scale[o] = 1.0 + o, 2.0
    d.jitter, d.min_variance = 1e-6, 1e-10
    d.var_out = 4096 if var_out else None       # only compared with NULL by the size queries
    return d


def sizes(lib, n_train, dim, n_obj, q, n_cand, ld, var_out, grid=False):
    """(bucb, gibbon, kb or None) workspace bytes of one descriptor."""
    from bayesopt_smart_amd import _lib
    b = fill(_lib.BucbDesc(), n_train, dim, n_obj, q, n_cand, ld, var_out, grid)
    g = fill(_lib.GibbonDesc(), n_train, dim, n_obj, q, n_cand, ld, var_out, grid)
    kb = None
    if n_obj <= 4:
        k = fill(_lib.KbDesc(), n_train, dim, n_obj, q, n_cand, ld, var_out, grid)
        k.n_front, k.form, k.box_capacity = 3, 0, 64
        kb = lib.bo_select_batch_kb_workspace_size(C.byref(k))
    return (lib.bo_select_batch_bucb_workspace_size(C.byref(b)),
            lib.bo_select_batch_gibbon_workspace_size(C.byref(g)), kb)


def check(lib, n_train, dim, n_obj, q, n_cand, ld, var_out, grid=False):
    lay = M.layout(n_train, dim, n_obj, q, n_cand, ld, var_out)
    key = (n_train, dim, n_obj, q, n_cand, ld, var_out, grid)
    bucb, gibbon, kb = sizes(lib, *key)
    assert bucb == gibbon == lay["total"] > 0, key
    if kb is not None:
        assert kb >= lay["total"] and kb > 0, key
    # the model's own invariants: aligned, in order, no overlap, inside the total
    end = 0
    for name in M.ORDER:
        if name not in lay:
            assert name == "var" and var_out
            continue
        off, shape, dtype = lay[name]
        assert off % 256 == 0 and off >= end, (key, name)
        end = off + int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert end <= lay["total"] and lay["total"] % 256 == 0, key
    assert ("var" in lay) == (not var_out)


@pytest.mark.parametrize("var_out", [True, False])
def test_edges(lib, var_out):
    for n_cand in (1, 255, 256, 257):
        for q in (1, 48):
            for n_obj in (1, 8):
                for dim in (1, 8):
                    check(lib, 37, dim, n_obj, q, n_cand, n_cand + 3, var_out)
    check(lib, 1, 1, 1, 1, 1, 1, var_out)
    check(lib, 65536, 8, 8, 48, 1 << 20, 1 << 20, var_out)          # the largest training set
    check(lib, 30, 2, 2, 5, 257, 257, var_out, grid=True)


def test_random_descriptors(lib):
    rng = np.random.default_rng(7)
    for _ in range(400):
        n_cand = int(rng.integers(1, 5000))
        check(lib, int(rng.integers(1, 3000)), int(rng.integers(1, 9)), int(rng.integers(1, 9)),
              int(rng.integers(1, 49)), n_cand, n_cand + int(rng.integers(0, 70)), bool(rng.integers(0, 2)),
              grid=bool(rng.integers(0, 2)))


def test_bad_descriptors_have_no_size(lib):
    for key in [(0, 2, 2, 5, 100, 100, True), (10, 0, 2, 5, 100, 100, True), (10, 9, 2, 5, 100, 100, True),
                (10, 2, 0, 5, 100, 100, True), (10, 2, 9, 5, 100, 100, True), (10, 2, 2, 0, 100, 100, True),
                (10, 2, 2, 49, 100, 100, True), (10, 2, 2, 5, 0, 100, True), (10, 2, 2, 5, 100, 99, True)]:
        bucb, gibbon, kb = sizes(lib, *key)
        assert bucb == 0 and gibbon == 0 and not kb, key


def test_read_returns_the_region():
    lay = M.layout(5, 3, 2, 4, 300, 303, True)
    ws = np.zeros(lay["total"], dtype=np.uint8)
    off, shape, _ = lay["dd"]
    ws[off:off + 64] = np.arange(8.0).view(np.uint8)
    np.testing.assert_array_equal(M.read(ws, lay, "dd"), np.arange(8.0).reshape(2, 4))
    assert M.read(ws, lay, "pick").dtype == np.int64 and M.read(ws, lay, "ok").shape == (2,)
