from .forecast import ensemble_scores  # noqa: F401
from .guidance import Guidance  # noqa: F401
from .metrics import DTWMetrics, FrechetDistance, KernelMMD, SinkhornDivergence  # noqa: F401
