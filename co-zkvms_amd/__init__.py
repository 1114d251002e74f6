"""co-zkvms_amd: MI355X-native engine for the sumcheck + polynomial-commitment hot path of
ChainSafe/co-zkvms (co-jolt / co-noir-spartan workers).  HIP kernels + C ABI live in csrc/ and are
loaded from libcozk.so (no CPU fallback); this package is the host-side mirror of the reference's
interfaces for that path.  Import with importlib.import_module("co-zkvms_amd")."""
from . import _lib
from ._lib import (CozkError, SCALAR_FR, SCALAR_U8, SCALAR_U16, SCALAR_U32, SCALAR_U64, SCALAR_I64,
                   LOW_TO_HIGH, HIGH_TO_LOW, MODE_PLAIN, MODE_REP3, OP_ADD, OP_SUB, OP_MUL)
from .engine import (Context, Vec, Bases, FR_MOD, FQ_MOD, fr_to_mont_limbs, mont_limbs_to_int,
                     point_to_abi, point_from_abi, wire_g1_encode, wire_g1_decode,
                     shamir_eval, shamir_lagrange, shamir_combine, shamir_combine_points, shamir_mul,
                     shamir_rand_deal, shamir_rand_extract, shamir_rand, shamir_mul_king, shamir_mul_pairs, shamir_gp_prove,
                     shamir_king_finish, shamir_mul_king_pairs, shamir_gp_prep, shamir_gp_prove_king, ShamirGpPrep, ShamirGpPrepResult,
                     ShamirGpProof, ShamirGpResult, ShamirGpStats, ShamirGpToggleStats, shamir_tgp_prove, shamir_tgp_prep,
                     shamir_tgp_prove_king)
from .poly import (Rep3DensePolynomial, Rep3DenseInterleavedPolynomial, SplitEqPolynomial, LayerGroup, eq_evals,
                   open_quadratic_evals, pst_fold, prod_sumcheck_evals, spartan_first_round, spartan_second_round,
                   sparse_matvec3, fingerprint_leaves, rep3_mul_vec_local)
from .harness import Harness, HarnessConfig, HarnessResult
from .spartan import SpartanHarness, SpartanConfig, SpartanResult
from .lookups import SparseLayer, SparseStats, sparse_stats, sparse_reset_stats, PrimaryGroup
from . import lasso
from .lasso import lasso_witness
from . import rw_memory
from .rw_memory import rw_memory_witness, RW_MEMORY_SYMBOLS
from . import ts_range
from .ts_range import time_counters, timestamp_range_witness, TS_RANGE_SYMBOLS
from . import ts_proof
from .ts_proof import (compact_batch_evaluate_at_chi, compact_linear_combination, timestamp_range_leaves, TS_PROOF_SYMBOLS, TsProof,
                       TsProofConfig, TsProofResult)
from . import rw_proof
from .rw_proof import rw_memory_leaves, rw_memory_init_final_leaves, RW_PROOF_SYMBOLS, RwProof, RwProofConfig, RwProofResult
from . import rw_proof_rep3
from .rw_proof_rep3 import (rw_memory_shared_leaves, rw_memory_shared_init_final_leaves, RW_PROOF_REP3_SYMBOLS, RwProofRep3, RwProofRep3Config,
                            RwProofRep3Result)
from . import memory_proof
from .memory_proof import OutputCheck, MemoryProof, MemoryProofConfig, MemoryProofResult, MEMORY_PROOF_SYMBOLS
from . import memory_proof_rep3
from .memory_proof_rep3 import MemoryProofRep3, MemoryProofRep3Config, MemoryProofRep3Result, MEMORY_PROOF_REP3_SYMBOLS
from . import bytecode
from .bytecode import (bytecode_witness, bytecode_leaves, bytecode_init_final_leaves, BYTECODE_SYMBOLS, BytecodeProof, BytecodeProofConfig,
                       BytecodeProofResult)
from . import shamir_spartan
from .shamir_spartan import SpartanGroup, ShamirSpartanHarness, ShamirSpartanConfig, ShamirSpartanResult
from . import shamir_jolt_spartan
from .shamir_jolt_spartan import OuterGroup, ShiftGroup, ShamirJoltSpartanHarness, ShamirJoltSpartanConfig, ShamirJoltSpartanResult
from . import shamir_primary
from .shamir_primary import ShamirPrimary, ShamirPrimaryConfig, ShamirPrimaryResult
