"""ctypes loader for libcozk.so (the HIP engine behind include/cozk.h).

There is deliberately NO CPU fallback: if the shared library is missing, or no MI355X is visible
when a context is created, the product path raises.  (The CPU restatement under oracle/ is test
infrastructure and is never imported from here.)
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcozk.so")

OK = 0
ERR_NO_DEVICE = -5

SCALAR_FR, SCALAR_U8, SCALAR_U16, SCALAR_U32, SCALAR_U64, SCALAR_I64 = range(6)
LOW_TO_HIGH, HIGH_TO_LOW = 0, 1
MODE_PLAIN, MODE_REP3 = 1, 2
LAYER_GROUP_MAX = 32
SPARTAN_GROUP_FIRST, SPARTAN_GROUP_SECOND = 1, 2
OP_ADD, OP_SUB, OP_MUL = 0, 1, 2
# collation forms of the primary sumcheck's instruction table (include/cozk.h COZK_G_*)
(G_CONCAT, G_PRODUCT, G_LTU, G_NOT_PRODUCT, G_NOT_LTU, G_SLT, G_NOT_SLT, G_LTE, G_NOT_FIRST, G_DIV0, G_UNSIGNED_REM, G_SIGNED_REM,
 G_ZERO) = range(13)
PRIMARY_MAX_MEMS = 20


PRF_KEY_BYTES = 32


def prf_key(k):
    """a 32-byte ChaCha12 PRF key for the ABI: bytes of length 32, or None (all-zero key, unmasked calls only)"""
    if k is None:
        return None
    k = bytes(k)
    if len(k) != PRF_KEY_BYTES:
        raise ValueError("PRF keys are %d bytes" % PRF_KEY_BYTES)
    return k


class CozkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"cozk error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libcozk.so once; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        _lib = ctypes.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_i = ctypes.c_int
_u64 = ctypes.c_uint64
_pp = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); also the list the symbol-export test checks against include/cozk.h
SIGNATURES = {
    "cozk_device_count": (_i, [ctypes.POINTER(_i)]),
    "cozk_ctx_create": (_i, [_i, _pp]),
    "cozk_ctx_destroy": (_i, [_vp]),
    "cozk_last_error": (ctypes.c_char_p, [_vp]),
    "cozk_ctx_synchronize": (_i, [_vp]),
    "cozk_ctx_stream": (_i, [_vp, _pp]),
    "cozk_vec_upload": (_i, [_vp, _vp, _sz, _i, _pp]),
    "cozk_vec_narrow": (_i, [_vp, _vp, _i, _pp]),
    "cozk_vec_alloc": (_i, [_vp, _sz, _i, _pp]),
    "cozk_vec_download": (_i, [_vp, _vp, _vp]),
    "cozk_vec_free": (_i, [_vp]),
    "cozk_vec_len": (_sz, [_vp]),
    "cozk_vec_device_ptr": (_vp, [_vp]),
    "cozk_vec_fill_random": (_i, [_vp, _vp, _u64, _i]),
    "cozk_vec_scale": (_i, [_vp, _vp, _vp]),
    "cozk_layer_compute_cubic_evals": (_i, [_vp, _vp, _vp, _vp]),
    "cozk_vec_binop": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "cozk_bases_upload": (_i, [_vp, _vp, _vp, _sz, _i, _pp]),
    "cozk_bases_from_scalars": (_i, [_vp, _vp, _vp, _i, _pp]),
    "cozk_bases_download": (_i, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "cozk_bases_free": (_i, [_vp]),
    "cozk_bases_len": (_sz, [_vp]),
    "cozk_bases_pair_sums": (_i, [_vp, _vp, _i, _pp]),
    "cozk_msm": (_i, [_vp, _vp, _sz, _vp, _i, _sz, _vp, ctypes.POINTER(_i)]),
    "cozk_msm_vec": (_i, [_vp, _vp, _sz, _vp, _vp, ctypes.POINTER(_i)]),
    "cozk_batch_msm_vec": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "cozk_batch_msm_slices": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "cozk_g1_sum": (_i, [_vp, _vp, _vp, _sz, _vp, ctypes.POINTER(_i)]),
    "cozk_g1_mul": (_i, [_vp, _vp, _i, _vp, _vp, ctypes.POINTER(_i)]),
    "cozk_poly_create": (_i, [_vp, _i, _vp, _vp, _pp]),
    "cozk_poly_chunk": (_i, [_vp, _vp, _sz, _sz, _pp]),
    "cozk_poly_free": (_i, [_vp]),
    "cozk_poly_len": (_sz, [_vp]),
    "cozk_poly_mode": (_i, [_vp]),
    "cozk_poly_download": (_i, [_vp, _vp, _vp, _vp]),
    "cozk_poly_share_view": (_i, [_vp, _vp, _i, _pp]),
    "cozk_poly_bind": (_i, [_vp, _vp, _vp, _i]),
    "cozk_poly_get_coeff": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "cozk_eq_evals": (_i, [_vp, _vp, _i, _pp]),
    "cozk_poly_batch_evaluate_at_chi": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "cozk_eq_plus_one_evals": (_i, [_vp, _vp, _i, _pp]),
    "cozk_poly_batch_dot_public": (_i, [_vp, _vp, _sz, _vp, _sz, _vp]),
    "cozk_poly_dot_product_with_public": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cozk_poly_linear_combination": (_i, [_vp, _vp, _vp, _sz, _i, _i, _pp]),
    "cozk_open_quadratic_evals": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "cozk_prod_sumcheck_evals": (_i, [_vp, _vp, _sz, _i, _vp]),
    "cozk_spartan_first_round": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "cozk_spartan_second_round": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cozk_sparse_matvec3": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _pp, _pp, _pp]),
    "cozk_pst_fold": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cozk_layer_create": (_i, [_vp, _i, _vp, _vp, _i, _pp]),
    "cozk_layer_free": (_i, [_vp]),
    "cozk_layer_len": (_sz, [_vp]),
    "cozk_layer_download": (_i, [_vp, _vp, _vp, _vp]),
    "cozk_layer_clone": (_i, [_vp, _vp, _pp]),
    "cozk_layer_bind": (_i, [_vp, _vp, _vp]),
    "cozk_layer_compute_cubic": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cozk_ctx_set_resident_rounds": (_i, [_vp, _i]),
    "cozk_rep3_share_vec": (_i, [_vp, _vp, ctypes.c_char_p, ctypes.c_char_p, _u64, _i, _pp, _pp]),
    "cozk_rep3_scatter": (_i, [_vp, _vp, ctypes.c_char_p, ctypes.c_char_p, _u64, _vp, _i, _pp, _pp]),
    "cozk_vec_fill_prf": (_i, [_vp, _vp, ctypes.c_char_p, _u64]),
    "cozk_vec_add_scalar": (_i, [_vp, _vp, _vp]),
    "cozk_shamir_share_vec": (_i, [_vp, _vp, ctypes.c_char_p, _i, _i, _u64, _vp]),
    "cozk_shamir_eval_vec": (_i, [_vp, _vp, _i, _i, _vp]),
    "cozk_shamir_scatter": (_i, [_vp, _vp, ctypes.c_char_p, _i, _i, _u64, _vp, _vp]),
    "cozk_shamir_lagrange": (_i, [_vp, _sz, _vp]),
    "cozk_shamir_combine_vec": (_i, [_vp, _vp, _vp, _sz, _i, _pp]),
    "cozk_shamir_mul_deal": (_i, [_vp, _vp, _vp, ctypes.c_char_p, _i, _i, _u64, _vp]),
    "cozk_shamir_mul_inproc": (_i, [_vp, _vp, _vp, _vp, _i, _i, _u64, _vp]),
    "cozk_shamir_mul_deal_pairs": (_i, [_vp, _vp, ctypes.c_char_p, _i, _i, _u64, _vp]),
    "cozk_shamir_mul_pairs_inproc": (_i, [_vp, _vp, _vp, _i, _i, _u64, _vp]),
    "cozk_shamir_gp_prove_inproc": (_i, [_vp, _vp, _sz, _vp, _vp, _i, _i, _u64, _u64, ctypes.c_char_p, _i, _pp]),
    "cozk_shamir_gp_free": (_i, [_vp]),
    "cozk_shamir_gp_get_result": (_i, [_vp, _vp]),
    "cozk_shamir_gp_get_stats": (_i, [_vp, _vp]),
    "cozk_shamir_gp_proof_bytes": (_i, [_vp, _vp, _sz]),
    "cozk_shamir_gp_point_len": (_sz, [_vp]),
    "cozk_shamir_gp_final": (_i, [_vp, _vp, _vp]),
    "cozk_shamir_gp_msgs_len": (_sz, [_vp]),
    "cozk_shamir_gp_msgs": (_i, [_vp, _vp, _sz]),
    "cozk_shamir_gp_finals_len": (_sz, [_vp]),
    "cozk_shamir_gp_finals": (_i, [_vp, _vp, _sz]),
    "cozk_shamir_mul_vec": (_i, [_vp, _vp, _vp, ctypes.c_char_p, _i, _u64, _pp]),
    "cozk_shamir_rand_deal": (_i, [_vp, _sz, ctypes.c_char_p, _i, _i, _u64, _vp, _vp]),
    "cozk_shamir_rand_extract": (_i, [_vp, _vp, _i, _i, _vp]),
    "cozk_shamir_rand_inproc": (_i, [_vp, _vp, _sz, _i, _i, _u64, _vp, _vp]),
    "cozk_shamir_rand_vec": (_i, [_vp, _sz, ctypes.c_char_p, _i, _u64, _vp, _vp]),
    "cozk_shamir_mul_mask": (_i, [_vp, _vp, _vp, _vp, _pp]),
    "cozk_shamir_mul_king_inproc": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "cozk_shamir_mul_king_vec": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _pp]),
    "cozk_shamir_mul_mask_pairs": (_i, [_vp, _vp, _vp, _sz, _pp]),
    "cozk_shamir_king_finish": (_i, [_vp, _vp, _i, _vp, _sz, _i, _vp, _vp]),
    "cozk_shamir_mul_king_pairs_inproc": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "cozk_shamir_gp_prep_inproc": (_i, [_vp, _vp, _sz, _sz, _i, _i, _u64, _pp]),
    "cozk_shamir_gp_prep_free": (_i, [_vp]),
    "cozk_shamir_gp_prep_get_result": (_i, [_vp, _vp]),
    "cozk_shamir_gp_prove_king_inproc": (_i, [_vp, _vp, _sz, _vp, _i, ctypes.c_char_p, _i, _pp]),
    "cozk_shamir_tgp_prove_inproc": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _i, _u64, _u64, ctypes.c_char_p, _i, _pp]),
    "cozk_shamir_tgp_prep_inproc": (_i, [_vp, _vp, _sz, _sz, _i, _i, _u64, _pp]),
    "cozk_shamir_tgp_prove_king_inproc": (_i, [_vp, _vp, _sz, _vp, _vp, _i, ctypes.c_char_p, _i, _pp]),
    "cozk_shamir_gp_toggle_claims": (_i, [_vp, _vp, _vp]),
    "cozk_shamir_gp_get_toggle_stats": (_i, [_vp, _vp]),
    "cozk_shamir_combine_points": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _vp, ctypes.POINTER(_i)]),
    "cozk_layer_round": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "cozk_fingerprint_leaves": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _i, _i, _vp, _vp, _sz, _sz]),
    "cozk_layer_prove_rounds": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "cozk_layer_final_claims": (_i, [_vp, _vp, _vp]),
    "cozk_layer_group_create": (_i, [_vp, _vp, _i, _pp]),
    "cozk_layer_group_round": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cozk_layer_group_final": (_i, [_vp, _vp, _vp, _i, _vp]),
    "cozk_layer_group_free": (_i, [_vp]),
    "cozk_spartan_group_create": (_i, [_vp, _i, _vp, _i, _vp, _pp]),
    "cozk_spartan_group_round": (_i, [_vp, _vp, _vp]),
    "cozk_spartan_group_final": (_i, [_vp, _vp, _i, _vp]),
    "cozk_spartan_group_len": (_sz, [_vp]),
    "cozk_spartan_group_pub_download": (_i, [_vp, _vp]),
    "cozk_spartan_group_free": (_i, [_vp]),
    "cozk_outer_group_create": (_i, [_vp, _vp, _i, _pp]),
    "cozk_outer_group_round": (_i, [_vp, _vp, _vp, _vp]),
    "cozk_outer_group_final": (_i, [_vp, _vp, _i, _vp]),
    "cozk_outer_group_len": (_sz, [_vp]),
    "cozk_outer_group_free": (_i, [_vp]),
    "cozk_primary_group_create": (_i, [_vp, _vp, _i, ctypes.c_char_p, _pp]),
    "cozk_primary_group_level": (_i, [_vp, _i, _u64, ctypes.POINTER(_sz)]),
    "cozk_primary_group_round_finish": (_i, [_vp, _vp]),
    "cozk_primary_group_len": (_sz, [_vp]),
    "cozk_primary_group_level_buffer": (_i, [_vp, _i, _i, _pp, ctypes.POINTER(_sz)]),
    "cozk_primary_group_free": (_i, [_vp]),
    "cozk_primary_group_create_king": (_i, [_vp, _vp, _i, _pp]),
    "cozk_primary_group_level_king": (_i, [_vp, _i, _vp, _vp, _sz, ctypes.POINTER(_sz)]),
    "cozk_primary_group_staging_bytes": (_sz, [_vp]),
    "cozk_primary_level_elems": (_sz, [_vp, _i]),
    "cozk_primary_plan": (_i, [_vp, _vp, _sz, _vp, _i, _vp, ctypes.POINTER(_u64)]),
    "cozk_shift_group_create": (_i, [_vp, _vp, _i, _vp, _pp]),
    "cozk_shift_group_round": (_i, [_vp, _vp, _vp]),
    "cozk_shift_group_final": (_i, [_vp, _vp, _i, _vp]),
    "cozk_shift_group_len": (_sz, [_vp]),
    "cozk_shift_group_pub_download": (_i, [_vp, _vp]),
    "cozk_shift_group_free": (_i, [_vp]),
    "cozk_toggle_group_create": (_i, [_vp, _vp, _sz, _vp, _i, _i, _pp]),
    "cozk_toggle_group_layer_outputs": (_i, [_vp, _vp, _vp]),
    "cozk_toggle_group_round": (_i, [_vp, _vp, _vp, _vp]),
    "cozk_toggle_group_bind": (_i, [_vp, _vp]),
    "cozk_toggle_group_final_claims": (_i, [_vp, _vp, _vp, _i]),
    "cozk_toggle_group_free": (_i, [_vp]),
    "cozk_sparse_layer_create": (_i, [_vp, _i, _sz, _vp, _vp, _vp, _i, _pp]),
    "cozk_toggle_sparse_output": (_i, [_vp, _vp, _i, _pp]),
    "cozk_sparse_layer_free": (_i, [_vp]),
    "cozk_sparse_layer_len": (_sz, [_vp]),
    "cozk_sparse_layer_count": (_sz, [_vp]),
    "cozk_sparse_layer_bytes": (_sz, [_vp]),
    "cozk_sparse_layer_next_count": (_i, [_vp, _vp, ctypes.POINTER(_sz)]),
    "cozk_sparse_layer_output_local": (_i, [_vp, _vp, _i, ctypes.c_char_p, ctypes.c_char_p, _u64, _pp]),
    "cozk_sparse_layer_from_output": (_i, [_vp, _vp, _vp, _vp, _i, _pp]),
    "cozk_sparse_layer_bind": (_i, [_vp, _vp, _vp]),
    "cozk_sparse_layer_round": (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
    "cozk_sparse_layer_to_dense": (_i, [_vp, _vp, _i, _pp]),
    "cozk_sparse_layer_download": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cozk_sparse_get_stats": (_i, [_vp, _vp]),
    "cozk_sparse_reset_stats": (_i, [_vp]),
    "cozk_layer_output_local": (_i, [_vp, _vp, _i, ctypes.c_char_p, ctypes.c_char_p, _u64, _pp]),
    "cozk_rep3_mul_vec_local": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, ctypes.c_char_p, ctypes.c_char_p, _u64, _pp]),
    "cozk_layer_claimed_outputs": (_i, [_vp, _vp, _vp]),
    "cozk_spliteq_new": (_i, [_vp, _vp, _i, _pp]),
    "cozk_spliteq_free": (_i, [_vp]),
    "cozk_spliteq_lens": (_i, [_vp, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "cozk_spliteq_bind": (_i, [_vp, _vp, _vp]),
    "cozk_spliteq_download": (_i, [_vp, _vp, _vp, _vp]),
    "cozk_prof_enable": (_i, [_vp, _i]),
    "cozk_prof_read": (_i, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "cozk_prof_kernel_name": (ctypes.c_char_p, [_i]),
    "cozk_prof_read_kernel": (_i, [_vp, _i, ctypes.POINTER(_u64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_u64)]),
    "cozk_layer_as_poly": (_i, [_vp, _vp, _pp]),
    "cozk_ring_unique_id": (_i, [_vp]),
    "cozk_ring_init": (_i, [_vp, ctypes.c_char_p, _i, _i]),
    "cozk_ring_destroy": (_i, [_vp]),
    "cozk_ring_info": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_u64)]),
    "cozk_reshare": (_i, [_vp, _vp, _vp]),
    "cozk_rep3_mul_vec": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_char_p, ctypes.c_char_p, _u64, _pp, _pp]),
    "cozk_ring_all_to_all": (_i, [_vp, _vp, _vp]),
    "cozk_ring_net_native": (_i, [_vp, _vp]),
    "cozk_wire_g1_encode": (_i, [_vp, _i, _vp]),
    "cozk_wire_g1_decode": (_i, [_vp, _vp, ctypes.POINTER(_i)]),
    "cozk_bench_montmul": (_i, [_vp, _sz, _i, _i, ctypes.POINTER(ctypes.c_double)]),
}


def _declare(l):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype = res
        fn.argtypes = args


class HarnessHandle:
    """One in-process prove harness of the C ABI: `PREFIX_create / _error / _destroy / _prove / _proof_bytes` over the
    CONFIG and RESULT structures.  A subclass fills a CONFIG and hands it to `_open`; EXTRA declares its other entry points
    (full name -> (restype, argtypes))."""
    PREFIX = CONFIG = RESULT = None
    EXTRA = {}

    @classmethod
    def _decl(cls):
        l = lib()
        sigs = {"_create": (_i, [ctypes.POINTER(cls.CONFIG), _pp]), "_error": (ctypes.c_char_p, [_vp]), "_destroy": (_i, [_vp]),
                "_prove": (_i, [_vp, _i, ctypes.POINTER(cls.RESULT)]), "_proof_bytes": (_i, [_vp, _vp, _sz])}
        for name, (res, args) in [(cls.PREFIX + k, v) for k, v in sigs.items()] + list(cls.EXTRA.items()):
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        return l

    def _f(self, suffix):
        return getattr(self._l, self.PREFIX + suffix)

    def _open(self, cfg, *args, create="_create"):
        """create(&cfg, *args, &h); a harness that fails to build reports its error, is destroyed, and raises CozkError"""
        self._l = self._decl()
        self.cfg = cfg
        h = ctypes.c_void_p()
        rc = self._f(create)(ctypes.byref(cfg), *args, ctypes.byref(h))
        self.h = h
        if rc != OK:
            msg = self.last_error() if h else ""
            self.close()
            raise CozkError(rc, msg or "?")

    def prove(self, verify=True):
        res = self.RESULT()
        rc = self._f("_prove")(self.h, 1 if verify else 0, ctypes.byref(res))
        if rc != OK:
            raise CozkError(rc, self.last_error() or "?")
        return res

    def proof_bytes(self, res):
        n = int(res.proof_len)
        buf = (ctypes.c_uint8 * n)()
        rc = self._f("_proof_bytes")(self.h, buf, n)
        if rc != OK:
            raise CozkError(rc, "proof_bytes")
        return bytes(buf)

    def last_error(self):
        return (self._f("_error")(self.h) or b"").decode()

    def close(self):
        if getattr(self, "h", None):
            self._f("_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
