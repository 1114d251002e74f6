"""The dealer's Lasso lookup witness on the device (`cozk_lasso_witness`; co-jolt/src/jolt/vm/instruction_lookups/witness.rs:85-150):
read_cts / E / final_cts of every memory from the address columns, the memory flags and the subtables, in one batched call."""
import ctypes

from . import _lib as L
from .engine import Vec

LASSO_SYMBOLS = ["cozk_lasso_witness", "cozk_lasso_tile"]
LASSO_MAX_M = 1 << 16
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_lasso_witness.restype = _i
    l.cozk_lasso_witness.argtypes = [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp]
    l.cozk_lasso_tile.restype = _sz
    l.cozk_lasso_tile.argtypes = []
    return l


def __getattr__(name):
    if name == "LASSO_TILE":  # steps per tile of the loaded library (COZK_LASSO_TILE)
        return int(_decl().cozk_lasso_tile())
    raise AttributeError(name)


def lasso_witness(ctx, dims, subtables, flags, mem_dim, mem_subtable):
    """dims: U32 Vecs of n addresses; subtables: U32 Vecs of M entries; flags: one U8 Vec of n entries per memory, None = the
    memory is used at every step; mem_dim / mem_subtable: per memory, which dim it reads and which subtable it looks up.
    Returns (read_cts, E, final_cts): lists of U32 Vecs, n, n and M entries per memory.  A flagged address >= M, M > 65536 or
    an inconsistent argument raises CozkError (COZK_ERR_INVALID_ARG) and returns nothing."""
    l = _decl()
    n_mem = len(mem_dim)
    if len(flags) != n_mem or len(mem_subtable) != n_mem:
        raise ValueError("flags, mem_dim and mem_subtable have one entry per memory")
    d = (_vp * len(dims))(*[v.h for v in dims])
    s = (_vp * len(subtables))(*[v.h for v in subtables])
    f = (_vp * n_mem)(*[v.h if v is not None else None for v in flags])
    md = (_i * n_mem)(*mem_dim)
    ms = (_i * n_mem)(*mem_subtable)
    rc, E, fc = (_vp * n_mem)(), (_vp * n_mem)(), (_vp * n_mem)()
    ctx.check(l.cozk_lasso_witness(ctx.h, d, len(dims), s, len(subtables), f, md, ms, n_mem, rc, E, fc))
    wrap = lambda arr: [Vec(ctx, _vp(arr[m]), L.SCALAR_U32) for m in range(n_mem)]
    return wrap(rc), wrap(E), wrap(fc)
