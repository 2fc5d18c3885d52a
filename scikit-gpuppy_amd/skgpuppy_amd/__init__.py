"""skgpuppy_amd -- MI355X-native drop-in for the GP hot path of scikit-gpuppy.

Same class names / signatures as the reference modules skgpuppy.Covariance, skgpuppy.GaussianProcess
and skgpuppy.UncertaintyPropagation; the arithmetic runs in hand-written HIP kernels (libgpx.so)
behind a ctypes C-ABI (include/gpx.h).  Importing this package without the built library fails.
"""
from . import _gpx  # noqa: F401  (fails loudly when libgpx.so is missing)
from .Covariance import Covariance, GaussianCovariance, MaternCovariance, PeriodicCovariance, SPGPCovariance, tracedot  # noqa: F401
from .GaussianProcess import GaussianProcess, PseudoInputGP  # noqa: F401
from .UncertaintyPropagation import (  # noqa: F401
    UncertaintyPropagationApprox,
    UncertaintyPropagationExact,
    UncertaintyPropagationGA,
    UncertaintyPropagationLinear,
    UncertaintyPropagation,
    UncertaintyPropagationMC,
    UncertaintyPropagationNumericalHG,
)

from .InverseUncertaintyPropagation import (  # noqa: F401,E402
    InverseUncertaintyPropagation,
    InverseUncertaintyPropagationApprox,
    InverseUncertaintyPropagationNumerical,
)

from .SensitivityAnalysis import SensitivityAnalysis  # noqa: F401,E402

__all__ = [
    "SensitivityAnalysis",
    "Covariance", "GaussianCovariance", "MaternCovariance", "PeriodicCovariance", "SPGPCovariance", "GaussianProcess", "PseudoInputGP",
    "UncertaintyPropagationGA",
    "UncertaintyPropagationApprox", "UncertaintyPropagationExact", "UncertaintyPropagationLinear", "tracedot",
    "UncertaintyPropagation", "UncertaintyPropagationMC", "UncertaintyPropagationNumericalHG",
    "InverseUncertaintyPropagation", "InverseUncertaintyPropagationApprox", "InverseUncertaintyPropagationNumerical",
]
