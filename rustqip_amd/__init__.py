"""rustqip_amd — MI355X-native backend for RustQIP's gate-application hot path.

Public surface (mirrors the reference names for this path):
  ops      MatrixOp, make_matrix_op, make_sparse_matrix_op, make_swap_op, make_control_op, inverse_op, CircuitError
  parametric  ParamGate and its constructors (rx, ry, rz, phase, rxx, ryy, rzz, pauli_rotation, generator_gate), gradient_plan
  state    apply_op, apply_op_overwrite, apply_op_row (host-pointer twins; any element type P: complex, real, integer),
           apply_op_device (the same on device slices), HipState (device-resident Complex<P> state), make_op_matrix
  builder  HipBuilder (LocalBuilder's run loop on the GPU)
  circuits workload generators of BASELINE.json's configs
  classical  copy, add, add_const, exp_mod_into, phase_oracle on qubit registers: thin calls of HipState.apply_function
  multiplex  rotation, select_gates, controlled, prepare_register: thin calls of HipState.apply_multiplexed
  fourier  qft, iqft, qft_ops, phase_estimation_readout, order_finding: thin calls of HipState.apply_qft
  noise    Channel and the usual Kraus families, trajectory and average: thin calls of HipState.apply_channels
Importing the package loads rustqip_amd/lib/libqip_hip.so and fails loudly if it is missing.
"""
from . import _ffi  # noqa: F401  (raises ImportError when the HIP library is absent)
from .ops import (CircuitError, MatrixOp, Representation, algorithmic_bytes, flip_bits, inverse_op, make_control_op,
                  make_matrix_op, make_sparse_matrix_op, make_swap_op, validate_op)
from .state import (HipState, QipHipError, apply_op, apply_op_device, apply_op_overwrite, apply_op_row, device_count,
                    make_op_matrix, set_global_option)
from .builder import Conditioned, HipBuilder, Measurements, Register, lower_to_matrix_op
from .state import DeviceSlice, HipProgram, expect_pauli_passes, ext_abi_version, pauli_rotation_passes, pauli_sum_passes, von_neumann_entropy
from .state import channel_passes, function_passes, multiplexed_table_bytes, qft_passes, krylov_bar, tridiagonal_eigh, tridiagonal_propagator_column
from . import circuits  # noqa: F401  (workload generators: rustqip_amd.circuits)
from . import parametric  # noqa: F401  (parametrised gates and the plan of HipState.circuit_gradient)
from . import replay  # noqa: F401  (flat circuit-replay format)
from . import classical  # noqa: F401  (classical reversible arithmetic on registers through HipState.apply_function)
from . import multiplex  # noqa: F401  (multiplexed rotations, gate lists and state preparation through HipState.apply_multiplexed)
from . import noise  # noqa: F401  (noise channels by quantum trajectories through HipState.apply_channels)
from . import fourier  # noqa: F401  (the quantum Fourier transform of a register and what it closes, through HipState.apply_qft)

__all__ = [
    "CircuitError", "MatrixOp", "Representation", "algorithmic_bytes", "flip_bits", "make_control_op",
    "make_matrix_op", "make_sparse_matrix_op", "make_swap_op", "validate_op", "HipState", "QipHipError",
    "apply_op", "apply_op_device", "apply_op_overwrite", "apply_op_row", "device_count", "make_op_matrix", "set_global_option", "Conditioned",
    "HipBuilder", "Measurements", "Register", "lower_to_matrix_op", "HipProgram", "DeviceSlice", "circuits", "replay", "ext_abi_version", "expect_pauli_passes",
    "pauli_rotation_passes", "pauli_sum_passes", "von_neumann_entropy", "krylov_bar", "tridiagonal_eigh", "tridiagonal_propagator_column",
    "inverse_op", "parametric", "classical", "function_passes", "noise", "channel_passes", "multiplex", "multiplexed_table_bytes",
    "fourier", "qft_passes",
]
