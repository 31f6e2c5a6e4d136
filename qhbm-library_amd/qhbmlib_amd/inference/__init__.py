"""Inference (reference: qhbmlib/inference/__init__.py:32-47)."""
from qhbmlib_amd.inference import ebm  # noqa: F401
from qhbmlib_amd.inference.captured import CapturedLoss
from qhbmlib_amd.inference.ebm import (AnalyticEnergyInference, BernoulliEnergyInference,
                                       EnergyInference, EnergyInferenceBase,
                                       GibbsWithGradientsInference)
from qhbmlib_amd.inference.ebm_utils import probabilities
from qhbmlib_amd.inference.ensemble_metrics import (EnsembleMetrics, differentiable_cross_gram, ensemble_metrics,
                                                    matrix_elements)
from qhbmlib_amd.inference.information import information_matrix, natural_gradient
from qhbmlib_amd.inference.krylov import (KrylovSpace, StreamedKrylovSpace, ThermalSweep, ground_state, krylov_space,
                                          spectrum_extremes, thermal_sweep)
from qhbmlib_amd.inference.qhbm import QHBM
from qhbmlib_amd.inference.qhbm_utils import density_matrix, fidelity
from qhbmlib_amd.inference.qmhl_loss import qmhl
from qhbmlib_amd.inference.qnn import (AnalyticQuantumInference, QuantumInference,
                                       SampledQuantumInference)
from qhbmlib_amd.inference.qnn_utils import unitary
from qhbmlib_amd.inference.reduced import (apply_operator, mutual_information, reduced_density_matrix,
                                           sampled_ensemble_reduced, sampled_reduced_density_matrix, subsystem_entropy,
                                           trace_distance)
from qhbmlib_amd.inference.state_metrics import StateMetrics, state_metrics, weighted_gram
from qhbmlib_amd.inference.thermal import (ThermalEnsemble, imaginary_time_evolution, real_time_evolution,
                                           thermal_ensemble)
from qhbmlib_amd.inference.vqt_loss import vqt
from qhbmlib_amd._engine import cross_gram

__all__ = ["AnalyticEnergyInference", "AnalyticQuantumInference", "BernoulliEnergyInference", "CapturedLoss",
           "EnergyInference", "EnergyInferenceBase", "EnsembleMetrics", "GibbsWithGradientsInference", "KrylovSpace", "QHBM", "QuantumInference",
           "SampledQuantumInference", "StateMetrics", "StreamedKrylovSpace", "ThermalEnsemble", "ThermalSweep", "apply_operator", "cross_gram", "density_matrix", "differentiable_cross_gram", "ensemble_metrics",
           "fidelity", "ground_state", "imaginary_time_evolution", "information_matrix", "krylov_space", "matrix_elements", "mutual_information",
           "natural_gradient", "probabilities", "qmhl", "real_time_evolution", "reduced_density_matrix",
           "sampled_ensemble_reduced", "sampled_reduced_density_matrix", "spectrum_extremes", "state_metrics", "subsystem_entropy", "thermal_ensemble",
           "thermal_sweep", "trace_distance", "unitary", "vqt", "weighted_gram"]
