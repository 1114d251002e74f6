"""Lasso counters over an identity table of any length (`cozk_time_counters`) and the dealer's timestamp range-check witness made of
them (`cozk_timestamp_range_witness`; jolt-core's TimestampRangeCheckPolynomials::generate_witness, whose four families
jolt/witness.rs:384-409 shares as public vectors): read_cts / final_cts of the read timestamps and of global time minus the read
timestamp, from the t_read columns that `rw_memory_witness` returns."""
import ctypes

from . import _lib as L
from .engine import Vec

TS_RANGE_SYMBOLS = ["cozk_time_counters", "cozk_timestamp_range_witness"]
TIME_COUNTERS_MAX_COLS = 16
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_time_counters.restype = _i
    l.cozk_time_counters.argtypes = [_vp, _vp, _sz, _sz, _vp, _vp]
    l.cozk_timestamp_range_witness.restype = _i
    l.cozk_timestamp_range_witness.argtypes = [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]
    return l


def _wrap(ctx, arr, k):
    return [Vec(ctx, _vp(arr[c]), L.SCALAR_U32) for c in range(k)]


def time_counters(ctx, keys, M):
    """keys: one U32 Vec of n keys per column (1 to 16 columns), each column on its own over an identity table of M entries (any M
    below 2^32).  Returns (read_cts, final_cts): per column a U32 Vec of n entries, the number of earlier steps with the same key
    (time order), and a U32 Vec of M entries, the number of steps with that key.  A key >= M or an inconsistent argument raises
    CozkError (COZK_ERR_INVALID_ARG) and returns nothing."""
    l = _decl()
    k = len(keys)
    rc, fc = (_vp * max(1, k))(), (_vp * max(1, k))()
    ctx.check(l.cozk_time_counters(ctx.h, (_vp * max(1, k))(*[v.h for v in keys]), k, M, rc, fc))
    return _wrap(ctx, rc, k), _wrap(ctx, fc, k)


def timestamp_range_witness(ctx, t_read, M):
    """t_read: one U32 Vec of n read timestamps per slot, as `rw_memory_witness` returns them; M >= n: the table's length (Jolt: the
    padded trace length).  Returns (read_cts_read_timestamp, read_cts_global_minus_read, final_cts_read_timestamp,
    final_cts_global_minus_read): four lists with one U32 Vec per slot, n entries in the first two and M in the last two.
    t_read[s][j] > j or an inconsistent argument raises CozkError (COZK_ERR_INVALID_ARG) and returns nothing."""
    l = _decl()
    ns = len(t_read)
    out = [(_vp * max(1, ns))() for _ in range(4)]
    ctx.check(l.cozk_timestamp_range_witness(ctx.h, (_vp * max(1, ns))(*[v.h for v in t_read]), ns, M, *out))
    return tuple(_wrap(ctx, arr, ns) for arr in out)
