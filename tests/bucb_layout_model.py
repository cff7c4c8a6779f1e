"""The workspace layout of the hallucinated-observation update (make_layout, bo_bucb_impl.h) restated
in plain Python, independently of the library, so that a test can read the update's intermediate
state back from a workspace tensor it allocated itself.

Every region is 256-byte aligned, in this order; `total` follows the last one:

    xc [N][dimp] f64      pc [q][dimp] f64         kx [n_obj][N] f64       kp [n_obj][q] f64
    wv [n_obj][q][N] f64  coef [n_obj][q][q] f64   dd [n_obj][q] f64       u [n_obj][N + q] f64
    ok [n_obj] int32      pick [q] int64           mask (bo_excl_mask_bytes(n_cand))
    partial [ceil(n_cand / 256)] {f64, int64}      var [n_obj][ld] f64 -- only when var_out is NULL

dimp = (dim + 1) & ~1.  bo_select_batch_bucb, bo_select_batch_gibbon and bo_select_batch_kb all place
this layout at workspace offset 0; bo_kb.hip appends its own regions after `total` (and uses a
`partial` of its own there).
"""
import numpy as np

THREADS = 256          # kThreads: candidates per workgroup of the candidate pass
TOP_ENTRY_BYTES = 16   # sizeof(TopEntry): double v, long long i

ORDER = ("xc", "pc", "kx", "kp", "wv", "coef", "dd", "u", "ok", "pick", "mask", "partial", "var")


def a256(b):
    return (b + 255) // 256 * 256


def excl_mask_bytes(n_cand):
    """bo_excl_mask_bytes: one bit per candidate in 32-bit words, two spare words, 256-byte aligned."""
    return a256(((max(n_cand, 0) + 31) // 32 + 2) * 4)


def layout(n_train, dim, n_obj, q, n_cand, ld=None, var_out=True):
    """dict name -> (offset, shape, dtype) of every region, plus "total", "dimp" and "blocks".
    `var` is present only when var_out is NULL (var_out=False); ld defaults to n_cand."""
    ld = n_cand if ld is None else ld
    dimp = (dim + 1) & ~1
    blocks = (n_cand + THREADS - 1) // THREADS
    f8, i4, i8, u4 = np.float64, np.int32, np.int64, np.uint32
    regions = [("xc", (n_train, dimp), f8), ("pc", (q, dimp), f8), ("kx", (n_obj, n_train), f8),
               ("kp", (n_obj, q), f8), ("wv", (n_obj, q, n_train), f8), ("coef", (n_obj, q, q), f8),
               ("dd", (n_obj, q), f8), ("u", (n_obj, n_train + q), f8), ("ok", (n_obj,), i4), ("pick", (q,), i8),
               ("mask", (excl_mask_bytes(n_cand) // 4,), u4), ("partial", (blocks, 2), f8)]
    if not var_out:
        regions.append(("var", (n_obj, ld), f8))
    out, off = {}, 0
    for name, shape, dtype in regions:
        out[name] = (off, shape, dtype)
        off += a256(int(np.prod(shape)) * np.dtype(dtype).itemsize)
    out["total"], out["dimp"], out["blocks"] = off, dimp, blocks
    return out


def read(ws_bytes, lay, name):
    """Region `name` of a workspace given as a numpy uint8 array, as a copy with its shape and type."""
    off, shape, dtype = lay[name]
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(ws_bytes[off:off + n].tobytes(), dtype=dtype).reshape(shape).copy()
