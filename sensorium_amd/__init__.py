"""sensorium_amd — MI355X-native DwiseNeuro training/inference hot path (drop-in for lRomul/sensorium's
``src/models/dwiseneuro.py`` + ``src/losses.py`` + the ``MouseModel`` step of ``src/argus_models.py``).

Importing the package loads ``csrc/libdwiseneuro_hip.so`` (hand-written gfx950 kernels behind a C-ABI,
include/dwn.h) and fails loudly if it is missing — there is no PyTorch/CPU fallback path.
"""
from . import _lib  # noqa: F401  (raises ImportError when the HIP library is absent)
from .dwiseneuro import DwiseNeuro  # noqa: F401
from .losses import MiceCorrelationLoss, MicePoissonCorrelationLoss, MicePoissonLoss  # noqa: F401
from .shifter import DwiseNeuroGaze, GazeShifter  # noqa: F401
from .modulator import BehaviorModulator, DwiseNeuroBehavior  # noqa: F401
from .spatial import DwiseNeuroSpatial, SpatialGain  # noqa: F401
from .stimuli import PARAM_NAMES, DriftingGabor, NoiseStimulus  # noqa: F401
from .attribution import optimal_gabor, tuning_curve  # noqa: F401
from . import receptive_fields  # noqa: F401
from .receptive_fields import GAUSS_FIT_COLUMNS, GaussianFits, ReceptiveFields, StaAccumulator, fit_gaussian2d  # noqa: F401
from .evaluation import FrameCut, TrialScorer, evaluate_trials  # noqa: F401
from . import population  # noqa: F401
from .population import CorrelationMatrices, PairwiseComparison, PairwiseCorrelation, population_structure  # noqa: F401
from .population import ModesComparison, PopulationModes, compare_modes  # noqa: F401

__all__ = ["DwiseNeuro", "DwiseNeuroGaze", "GazeShifter", "DwiseNeuroBehavior", "BehaviorModulator", "DwiseNeuroSpatial", "SpatialGain", "MicePoissonLoss", "MiceCorrelationLoss", "MicePoissonCorrelationLoss",
           "DriftingGabor", "PARAM_NAMES", "tuning_curve", "optimal_gabor", "FrameCut", "TrialScorer", "evaluate_trials",
           "NoiseStimulus", "receptive_fields", "StaAccumulator", "ReceptiveFields",
           "GaussianFits", "GAUSS_FIT_COLUMNS", "fit_gaussian2d", "population", "PairwiseCorrelation", "CorrelationMatrices",
           "PairwiseComparison", "population_structure", "PopulationModes", "ModesComparison", "compare_modes"]
