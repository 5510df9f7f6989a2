"""irlmx -- MI355X-native MaxEnt-IRL inner loop.

Host side in Python on PyTorch-ROCm tensors, compute in hand-written HIP
kernels for gfx950 behind the C ABI of ``libirlmx.so`` (include/irlmx.h).

* ``irlmx.DeviceMDP``  -- transition model resident in HBM (stencil / ELL)
* ``irlmx.ops``        -- batched device ops: backward, forward SVF, soft VI, VI,
  policy evaluation and the expected value difference, demonstration rollouts,
  their statistics and log-likelihood, and the same for the time-indexed
  policies of the finite-horizon models (include/irlmx_timed.h)
* ``irlmx.batch``      -- batched IRL gradient steps (B instances per call)
* ``maxent`` / ``solver`` (next to this package) -- numpy drop-ins for the
  reference modules of the same names.
"""

from ._lib import IrlmxError, load, require_device  # noqa: F401
from .mdp import DeviceMDP  # noqa: F401
from . import ops  # noqa: F401
from .ops import backward_maxent_extended, execution_plan  # noqa: F401
from .ops import expected_value_difference, policy_evaluation  # noqa: F401
from .ops import demo_log_likelihood, rollout  # noqa: F401
from .ops import backward_maxent_horizon, forward_svf_horizon, soft_backward_horizon  # noqa: F401
from .ops import demo_log_likelihood_horizon, expected_value_difference_horizon, rollout_horizon, value_horizon  # noqa: F401
from .ops import expected_svf_horizon, expected_svf_horizon_plan  # noqa: F401

__version__ = "0.1.0"
