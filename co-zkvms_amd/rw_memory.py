"""The dealer's read-write memory witness on the device (`cozk_rw_memory_witness`; jolt-core's
ReadWriteMemoryPolynomials::generate_witness, before read_write_memory/witness.rs:34-93 shares it): v_read / t_read / v_written of
every slot and v_final / t_final of the one register + RAM memory, from the address columns, the written values and the write flags."""
import ctypes

from . import _lib as L
from .engine import Vec

RW_MEMORY_SYMBOLS = ["cozk_rw_memory_witness"]
RW_MEMORY_MAX_SLOTS = 8
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def _decl():
    l = L.lib()
    l.cozk_rw_memory_witness.restype = _i
    l.cozk_rw_memory_witness.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]
    return l


def rw_memory_witness(ctx, addr, v_write, is_write, v_init):
    """addr: one U8 or U32 Vec of n addresses per slot, the operations ordered by (step, slot); v_write: per slot a U32 Vec of n
    written values, None = the slot only reads; is_write: per slot a U8 Vec of n flags, None = every step writes (None where v_write
    is None); v_init: U32 Vec of MEM words.  Returns (v_read, t_read, v_written, v_final, t_final): three lists with one entry per
    slot (U32 Vecs of n entries; v_written None for a slot without flags) and two U32 Vecs of MEM entries.  An address >= MEM or an
    inconsistent argument raises CozkError (COZK_ERR_INVALID_ARG) and returns nothing."""
    l = _decl()
    ns = len(addr)
    if len(v_write) != ns or len(is_write) != ns:
        raise ValueError("addr, v_write and is_write have one entry per slot")
    handles = lambda vs: (_vp * max(1, ns))(*[v.h if v is not None else None for v in vs])
    vr, tr, vw = (_vp * max(1, ns))(), (_vp * max(1, ns))(), (_vp * max(1, ns))()
    vf, tf = _vp(), _vp()
    ctx.check(l.cozk_rw_memory_witness(ctx.h, handles(addr), handles(v_write), handles(is_write), ns, v_init.h, vr, tr, vw, ctypes.byref(vf), ctypes.byref(tf)))
    wrap = lambda arr: [Vec(ctx, _vp(arr[s]), L.SCALAR_U32) if arr[s] else None for s in range(ns)]
    return wrap(vr), wrap(tr), wrap(vw), Vec(ctx, vf, L.SCALAR_U32), Vec(ctx, tf, L.SCALAR_U32)
