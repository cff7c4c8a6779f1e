"""The fit path's workspace layouts restated in plain Python, independently of the library: the
inverse's workspace (bo_invert_k_workspace_size), the MLL's (bo_compute_mll_workspace_size) with
its pinned host block, and one slot of the blocked LU (bo_lu.hip).

Written from the formulas the entry points used before they shared a layout struct:

    inverse:  geo_bytes + lu + 2 a256(4 n) + 512 + flag_bytes,
              lu = 2 a256(8 n^2) above the LU's capacity (Gauss-Jordan's matrix pair), else 0;
              pointers A, bufA = A + geo_bytes, bufB = bufA + gj, piv = bufB + gj,
              perm = piv + a256(4 n), status = perm + a256(4 n), flags = status + 512;
              status words BO_MAX_OBJ + 1 (Gauss-Jordan) and BO_MAX_OBJ + 2 (abort)
    MLL:      geo_bytes + a256(8 n_obj (2 nbt + 1) + 4 BO_MAX_OBJ) + 512 + flag_bytes, flags last;
              pinned: n_obj (2 nbt + 1) doubles, n_obj status ints, abort, done
    LU slot:  a256(8 Na n_p) + a256(4 nbs PREC) + a256(4 n_p) + a256(8 nbs 512); n_lu slots + 256

Each layout is a list of (name, offset, bytes) in address order plus the total."""

NB = 32            # column block of the augmented Cholesky
MAX_OBJ = 8        # BO_MAX_OBJ
LU_MAX_N = 2048    # bo_lu_max_n(): 512 threads x 4 rows
LU_LB, LU_PREC = 16, 72


def a256(x):
    return (x + 255) // 256 * 256


def geo(n, n_obj, ident):
    nbt = -(-n // NB)
    n_p = nbt * NB
    na = 2 * n_p if ident else n_p + NB
    ncols = 2 * n_p if ident else n_p
    return dict(n=n, n_obj=n_obj, ident=ident, nbt=nbt, Na=na, ncols=ncols, ostride=na * ncols)


def geo_bytes(g):
    return a256(8 * g["n_obj"] * g["ostride"])


def flag_words(g):
    """[0] dequeue counter, [1] abort, [2] exit counter, 16 reserved in all; then per objective the
    panel flags [nbt][nbt], the L part's tile versions [RB][nbt] and C's [nbt][nbt]"""
    nbt = g["nbt"]
    rb = 2 * nbt if g["ident"] else nbt + 1
    return 16 + g["n_obj"] * (2 * nbt * nbt + rb * nbt)


def flag_bytes(g):
    return a256(4 * flag_words(g))


def _carve(parts):
    out, at = [], 0
    for name, padded, used in parts:
        out.append((name, at, used))
        at += padded
    return out, at


def inv_layout(n, n_obj):
    g = geo(n, n_obj, True)
    gj = a256(8 * n * n) if n > LU_MAX_N else 0
    used_gj = 8 * n * n if n > LU_MAX_N else 0
    return _carve([("A", geo_bytes(g), 8 * n_obj * g["ostride"]), ("bufA", gj, used_gj), ("bufB", gj, used_gj),
                   ("piv", a256(4 * n), 4 * n), ("perm", a256(4 * n), 4 * n), ("status", 512, 4 * (MAX_OBJ + 4)),
                   ("flags", flag_bytes(g), 4 * flag_words(g))])


INV_STATUS_GJ, INV_STATUS_ABORT = MAX_OBJ + 1, MAX_OBJ + 2


def mll_layout(n, n_obj):
    g = geo(n, n_obj, False)
    part = 8 * n_obj * (2 * g["nbt"] + 1) + 4 * MAX_OBJ
    return _carve([("A", geo_bytes(g), 8 * n_obj * g["ostride"]), ("spare", a256(part) + 512, 0),
                   ("flags", flag_bytes(g), 4 * flag_words(g))])


def mll_host(n, n_obj):
    g = geo(n, n_obj, False)
    part = 8 * n_obj * (2 * g["nbt"] + 1)
    return _carve([("part", part, part), ("status", 4 * n_obj, 4 * n_obj), ("abort", 4, 4), ("done", 4, 4)])


def lu_slot(n):
    n_p = -(-n // LU_LB) * LU_LB
    nbs = n_p // LU_LB
    sizes = [("A", 8 * n_p * n_p), ("prec", 4 * nbs * LU_PREC), ("sinv", 4 * n_p), ("tinv", 8 * nbs * 512)]
    return _carve([(k, a256(b), b) for k, b in sizes])


def lu_workspace(n, n_lu):
    return n_lu * lu_slot(n)[1] + 256
