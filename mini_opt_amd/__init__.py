"""mini_opt_amd -- MI355X-native batched interior-point Newton steps behind mini_opt's QP API.

Only what the hot path needs: csrc/ (HIP kernels + C ABI, built into lib/libminiopt_hip.so), qp.py (host mirror of
mini_opt::QP / QPInteriorPointSolver for batches), diff.py (solve_qp: autograd through a solve), synth.py (synthetic workloads),
sharding.py (multi-GPU batch shards).
"""
from . import _lib  # noqa: F401
from ._lib import MiniOptError, build  # noqa: F401


_DIFF_EXPORTS = ("solve_qp", "kkt_solve", "qp_gradients", "qp_gradients_shared", "qp_gradients_blocks", "qp_gradients_eq_blocks",
                 "qp_gradients_blocks_shared", "QPSolveFunction",
                 "QPSolveBlocksFunction", "adjoint_status", "qp_tangent_rhs", "qp_jvp", "tangent_status",
                 "qp_tangent_rhs_blocks", "qp_jvp_blocks", "qp_gradients_blocks_weighted", "qp_tangent_rhs_blocks_weighted",
                 "qp_jvp_blocks_weighted", "QPSolveWeightedBlocksFunction", "qp_gradients_blocks_weighted_shared")


_QP_EXPORTS = ("ResidualLayout", "ResidualLoss", "loss_weights", "linearize_blocks",   # residual-block input and its robust losses
                "covariance")                                                         # parameter covariance of a fit


def __getattr__(name):  # the differentiable front end needs torch: imported on first use, like qp
    if name in _DIFF_EXPORTS:
        from . import diff
        return getattr(diff, name)
    if name in _QP_EXPORTS:
        from . import qp
        return getattr(qp, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
